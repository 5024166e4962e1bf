// vgl_gvcf.hip -- gVCF blocks of a tile on the device (ABI 7 additions: vgl_gvcf_workspace_bytes, vgl_gvcf_blocks_device).
// The host writer's block machine (host/vcfgl_main.cpp GvcfBlocker::prepare, prepare_gvcf_block() of the reference) reduces to rules
// on neighbouring kept sites (site_status >= 0; skipped sites are transparent):
//   blockable  n_alleles_obs == 1 and r > 0, r = the index of the first --gvcf-dps threshold above the site's smallest per-sample DP
//              (the number of thresholds when none is)
//   continues  blockable, the previous kept site blockable, same contig, pos0 <= prev pos0 + 1, same r
//   founds     blockable and does not continue;  a record: kept and not blockable
// and the block aggregates (per-sample min DP, MIN_DP, the lexicographically smallest signed (PL[1], PL[2]); PL[0], alleles and QS
// of the founder) do not depend on the order in which members are combined.  Five passes:
//   k_gvcf_site   a sub-group of W = min(64, pow2 >= N) lanes per site: min DP over the samples, r, the flags (N = 1: one lane per
//                 site; N >= 64: one wavefront per site, coalesced over samples)
//   k_gvcf_scan   one workgroup, chunks of SCAN_NT sites with carries: the previous kept site (max-scan), continue / found flags,
//                 item and block numbers (sum scans), MIN_DP (segmented min scan), the item list, each block's last member, the
//                 record status array (block sites -> -1, the formatter's "skipped"), the first site that joins a block while it or
//                 the founder has n_alleles != 2 (the host's "Unexpected number of PL values")
//   k_gvcf_init   slots of the blocks that cross an aggregation chunk: DP = INT32_MAX, PL key = ~0
//   k_gvcf_agg    one lane per (chunk of CH sites, sample), consecutive lanes = consecutive samples: running min of DP and of the PL key
//                 over each block's run inside the chunk; a block wholly inside the chunk is stored, a crossing one combined with
//                 vector atomicMin (int32 DP; PL key = (PL1 ^ 0x80000000) << 32 | (PL2 ^ 0x80000000), which orders as the signed pair)
//   k_gvcf_final  one lane per (block, sample): the block's DP slab and its PL slab (founder's PL[0], the key's PL[1], PL[2]; a founder
//                 with n_alleles != 2 -- legal alone -- keeps its nG values)
// Min is order-free: the output is deterministic.  Only vector stores and vector atomics write memory.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vcfgl_hip.h"

namespace {

constexpr int NT = 256;
constexpr int SCAN_NT = 1024;
constexpr int CH = 32;                  // sites per aggregation chunk
constexpr int32_t BIG = 0x7fffffff;

struct GvcfArgs {
    int32_t N, n_sites, n_dps;
    const int32_t* st; const int32_t* nobs; const int32_t* na; const int32_t* contig; const int64_t* pos0;
    const int32_t* dp; int64_t dp_stride; const int32_t* pl; int64_t pl_stride; const int32_t* dps;
    vgl_gvcf_item* items; int32_t* counts;
    int32_t* blk_dp; int32_t* blk_pl; int32_t* blk_na; int32_t* blk_status; int32_t* rec_status;
    // workspace
    int32_t* smin;      // [n_sites] the site's min DP; after k_gvcf_scan the running min of its block (segmented scan)
    int32_t* flag;      // [n_sites] kept | blockable << 1 | r << 2
    int32_t* item_of;   // [n_sites] item of a kept site
    int32_t* blk_of;    // [n_sites] block of a block site, -1 otherwise
    int32_t* blk_item;  // [n_sites] item of block b
    int32_t* wdp;       // [n_sites * N]
    uint64_t* wkey;     // [n_sites * N]
};

__device__ inline uint64_t pl_key(int32_t p1, int32_t p2) {
    return ((uint64_t)((uint32_t)p1 ^ 0x80000000u) << 32) | (uint64_t)((uint32_t)p2 ^ 0x80000000u);
}

__global__ __launch_bounds__(NT) void k_gvcf_site(GvcfArgs A, int W) {
    const int tid = threadIdx.x, j = tid & (W - 1);
    const int64_t i = (int64_t)blockIdx.x * (NT / W) + tid / W;
    int32_t m = BIG;
    if (i < A.n_sites)
        for (int s = j; s < A.N; s += W) { const int32_t v = A.dp[i * A.dp_stride + s]; m = v < m ? v : m; }
    for (int o = 1; o < W; o <<= 1) { const int32_t y = __shfl_xor(m, o, 64); m = y < m ? y : m; }
    if (i >= A.n_sites || j != 0) return;
    int r = 0;
    while (r < A.n_dps && !(m < A.dps[r])) ++r;
    const int kept = A.st[i] >= 0, blockable = kept && A.nobs[i] == 1 && r > 0;
    A.smin[i] = m;
    A.flag[i] = kept | blockable << 1 | r << 2;
}

// inclusive scan of one value per lane over the workgroup (op: sum / max / segmented min), returns the workgroup's total in *tot
template <class T, class Op>
__device__ T wg_scan(T x, T* part, T* tot, Op op) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const T y = __shfl_up(x, o, 64); if (lane >= o) x = op(y, x); }
    if (lane == 63) part[wv] = x;
    __syncthreads();
    T before = part[0], t = part[0];
    for (int w = 1; w < SCAN_NT / 64; ++w) { if (w < wv) before = op(before, part[w]); t = op(t, part[w]); }
    if (wv > 0) x = op(before, x);
    *tot = t;
    __syncthreads();
    return x;
}

// segmented min: (value, head) pairs; a head starts a new segment
struct Seg { int32_t v; int32_t h; };
struct SegOp { __device__ Seg operator()(Seg a, Seg b) const { return b.h ? b : Seg{a.v < b.v ? a.v : b.v, a.h}; } };
__device__ inline Seg shfl_up_seg(Seg x, int o) { return Seg{__shfl_up(x.v, o, 64), __shfl_up(x.h, o, 64)}; }

template <class Op>
__device__ Seg wg_scan_seg(Seg x, Seg* part, Seg* tot, Op op) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const Seg y = shfl_up_seg(x, o); if (lane >= o) x = op(y, x); }
    if (lane == 63) part[wv] = x;
    __syncthreads();
    Seg before = part[0], t = part[0];
    for (int w = 1; w < SCAN_NT / 64; ++w) { if (w < wv) before = op(before, part[w]); t = op(t, part[w]); }
    if (wv > 0) x = op(before, x);
    *tot = t;
    __syncthreads();
    return x;
}

__device__ inline void close_block(const GvcfArgs& A, int32_t p) {      // p = the last member of its block
    const int32_t it = A.item_of[p];
    A.items[it].last = p;
    A.items[it].min_dp = A.smin[p];
}

__global__ __launch_bounds__(SCAN_NT) void k_gvcf_scan(GvcfArgs A) {
    __shared__ int32_t part[SCAN_NT / 64];
    __shared__ Seg spart[SCAN_NT / 64];
    __shared__ int32_t err;
    const int tid = threadIdx.x;
    if (tid == 0) err = BIG;
    auto imax = [](int32_t a, int32_t b) { return a > b ? a : b; };
    auto isum = [](int32_t a, int32_t b) { return a + b; };
    int32_t c_kept = -1, c_found = -1, c_items = 0, c_blocks = 0;
    Seg c_seg{BIG, 1};
    for (int b0 = 0; b0 < A.n_sites; b0 += SCAN_NT) {
        const int32_t i = b0 + tid;
        const bool in = i < A.n_sites;
        const int32_t f = in ? A.flag[i] : 0;
        const int kept = f & 1, blockable = (f >> 1) & 1, r = f >> 2;
        int32_t tot;
        // previous kept site: the inclusive max-scan of the lane before (the carry for the chunk's first lane)
        __shared__ int32_t lastmk[SCAN_NT / 64];
        int32_t mk = wg_scan(kept ? i : -1, part, &tot, imax);
        mk = imax(mk, c_kept);
        int32_t prev = __shfl_up(mk, 1, 64);
        if ((tid & 63) == 63) lastmk[tid >> 6] = mk;
        __syncthreads();
        if ((tid & 63) == 0) prev = (tid == 0) ? c_kept : lastmk[(tid >> 6) - 1];
        bool cont = false;
        if (in && blockable && prev >= 0) {
            const int32_t pf = A.flag[prev];
            cont = ((pf >> 1) & 1) && (pf >> 2) == r && A.contig[prev] == A.contig[i] && A.pos0[i] <= A.pos0[prev] + 1;
        }
        const int start = kept && !cont, found = blockable && !cont;
        int32_t ni = wg_scan((int32_t)start, part, &tot, isum);
        const int32_t item = c_items + ni - 1;
        const int32_t n_items_tot = tot;
        int32_t nb = wg_scan((int32_t)found, part, &tot, isum);
        const int32_t blk = c_blocks + nb - 1;
        const int32_t n_blocks_tot = tot;
        int32_t fd = wg_scan(found ? i : -1, part, &tot, imax);
        fd = imax(fd, c_found);
        Seg sg{blockable ? A.smin[i < A.n_sites ? i : 0] : BIG, start};
        Seg stot;
        sg = wg_scan_seg(sg, spart, &stot, SegOp());
        sg = SegOp()(c_seg, sg);
        if (in) {
            if (kept) A.item_of[i] = item;
            A.blk_of[i] = blockable ? blk : -1;
            A.rec_status[i] = (kept && !blockable) ? A.st[i] : -1;
            if (blockable) A.smin[i] = sg.v;
            if (start) {
                vgl_gvcf_item t;
                t.kind = blockable ? VGL_GVCF_BLOCK : VGL_GVCF_RECORD;
                t.first = i; t.last = i; t.founder = i; t.dpr = blockable ? r : 0;
                t.min_dp = blockable ? sg.v : A.smin[i]; t.block = blockable ? blk : -1; t.reserved = 0;
                A.items[item] = t;
            }
            if (found) { A.blk_na[blk] = A.na[i]; A.blk_status[blk] = 0; A.blk_item[blk] = item; }
            if (cont && (A.na[i] != 2 || A.na[fd] != 2)) atomicMin(&err, i);
        }
        __syncthreads();                                              // item_of / smin of this chunk are visible
        // the kept site before an item start closes its block
        if (in && start && prev >= 0 && ((A.flag[prev] >> 1) & 1)) close_block(A, prev);
        c_kept = imax(c_kept, lastmk[SCAN_NT / 64 - 1]);
        c_items += n_items_tot; c_blocks += n_blocks_tot;
        {
            __shared__ int32_t lf;
            if (tid == SCAN_NT - 1) lf = fd;
            __syncthreads();
            c_found = imax(c_found, lf);
        }
        c_seg = SegOp()(c_seg, stot);
        __syncthreads();
    }
    if (tid == 0) {
        if (c_kept >= 0 && ((A.flag[c_kept] >> 1) & 1)) close_block(A, c_kept);
        A.counts[0] = c_items; A.counts[1] = c_blocks; A.counts[2] = err == BIG ? -1 : err; A.counts[3] = 0;
    }
    for (int32_t b = c_blocks + tid; b < A.n_sites; b += SCAN_NT) { A.blk_status[b] = -1; A.blk_na[b] = 2; A.blk_item[b] = -1; }
}

__device__ inline bool owned(const GvcfArgs& A, int32_t b) {         // every member of block b in one aggregation chunk
    const vgl_gvcf_item& t = A.items[A.blk_item[b]];
    return t.first / CH == t.last / CH;
}

__global__ __launch_bounds__(NT) void k_gvcf_init(GvcfArgs A) {
    const int64_t x = (int64_t)blockIdx.x * NT + threadIdx.x;
    const int64_t b = x / A.N;
    if (b >= A.counts[1] || owned(A, (int32_t)b)) return;
    A.wdp[x] = BIG;
    A.wkey[x] = ~0ull;
}

__device__ inline void flush(const GvcfArgs& A, int32_t b, int s, int32_t m, uint64_t k) {
    const int64_t x = (int64_t)b * A.N + s;
    if (owned(A, b)) { A.wdp[x] = m; A.wkey[x] = k; }
    else { atomicMin(&A.wdp[x], m); atomicMin((unsigned long long*)&A.wkey[x], (unsigned long long)k); }
}

__global__ __launch_bounds__(NT) void k_gvcf_agg(GvcfArgs A) {
    const int64_t x = (int64_t)blockIdx.x * NT + threadIdx.x;
    const int64_t c = x / A.N;
    const int s = (int)(x - c * A.N);
    const int64_t i0 = c * CH;
    if (i0 >= A.n_sites) return;
    const int64_t i1 = i0 + CH < A.n_sites ? i0 + CH : A.n_sites;
    int32_t cur = -1, m = BIG;
    uint64_t k = ~0ull;
    for (int64_t i = i0; i < i1; ++i) {
        const int32_t b = A.blk_of[i];
        if (b < 0) continue;
        if (b != cur) {
            if (cur >= 0) flush(A, cur, s, m, k);
            cur = b; m = BIG; k = ~0ull;
        }
        const int32_t v = A.dp[i * A.dp_stride + s];
        m = v < m ? v : m;
        const int32_t* p = A.pl + i * A.pl_stride + (int64_t)s * 3;     // (a member with n_alleles != 2 is the reported error case)
        const uint64_t q = pl_key(p[1], p[2]);
        k = q < k ? q : k;
    }
    if (cur >= 0) flush(A, cur, s, m, k);
}

__global__ __launch_bounds__(NT) void k_gvcf_final(GvcfArgs A) {
    const int64_t x = (int64_t)blockIdx.x * NT + threadIdx.x;
    const int64_t b = x / A.N;
    const int s = (int)(x - b * A.N);
    if (b >= A.counts[1]) return;
    const int32_t f = A.items[A.blk_item[b]].founder;
    const int nA = A.na[f], nG = nA * (nA + 1) / 2;
    A.blk_dp[b * A.N + s] = A.wdp[x];
    if ((int64_t)(s + 1) * nG > A.pl_stride) return;                  // (a slab too small for the founder's nG: nothing to copy)
    const int32_t* src = A.pl + (int64_t)f * A.pl_stride + (int64_t)s * nG;
    int32_t* dst = A.blk_pl + b * A.pl_stride + (int64_t)s * nG;
    if (nA == 2) {
        const uint64_t k = A.wkey[x];
        dst[0] = src[0];
        dst[1] = (int32_t)((uint32_t)(k >> 32) ^ 0x80000000u);
        dst[2] = (int32_t)((uint32_t)k ^ 0x80000000u);
    } else {
        for (int g = 0; g < nG; ++g) dst[g] = src[g];
    }
}

// the aggregates of the first and the last block -> edge [2][N] DP, then [2][pl_stride] PL (the record-loop entry's copy-back)
__global__ __launch_bounds__(NT) void k_gvcf_edges(GvcfArgs A, int32_t* edge) {
    const int32_t nb = A.counts[1];
    if (nb <= 0) return;
    const int which = blockIdx.y;
    const int64_t b = which ? nb - 1 : 0;
    for (int64_t x = (int64_t)blockIdx.x * NT + threadIdx.x; x < A.N; x += (int64_t)gridDim.x * NT) edge[which * (int64_t)A.N + x] = A.blk_dp[b * A.N + x];
    int32_t* ep = edge + 2 * (int64_t)A.N + which * A.pl_stride;
    for (int64_t x = (int64_t)blockIdx.x * NT + threadIdx.x; x < A.pl_stride; x += (int64_t)gridDim.x * NT) ep[x] = A.blk_pl[b * A.pl_stride + x];
}

inline int64_t al(int64_t v) { return (v + 255) & ~(int64_t)255; }

GvcfArgs make_args(int32_t n_samples, int32_t n_sites, const vgl_gvcf_in* in, const vgl_gvcf_out* out, void* ws) {
    GvcfArgs A;
    memset(&A, 0, sizeof A);
    A.N = n_samples; A.n_sites = n_sites; A.n_dps = in->n_dps;
    A.st = in->site_status; A.nobs = in->n_alleles_obs; A.na = in->n_alleles; A.contig = in->contig; A.pos0 = in->pos0;
    A.dp = in->dp; A.dp_stride = in->dp_site_stride; A.pl = in->pl; A.pl_stride = in->pl_site_stride; A.dps = in->dps;
    A.items = out->items; A.counts = out->counts; A.blk_dp = out->block_dp; A.blk_pl = out->block_pl; A.blk_na = out->block_n_alleles;
    A.blk_status = out->block_status; A.rec_status = out->record_status;
    char* p = (char*)ws;
    const int64_t S = n_sites, E = (int64_t)n_sites * n_samples;
    A.smin = (int32_t*)p; p += al(S * 4);
    A.flag = (int32_t*)p; p += al(S * 4);
    A.item_of = (int32_t*)p; p += al(S * 4);
    A.blk_of = (int32_t*)p; p += al(S * 4);
    A.blk_item = (int32_t*)p; p += al(S * 4);
    A.wkey = (uint64_t*)p; p += al(E * 8);
    A.wdp = (int32_t*)p;
    return A;
}

}  // namespace

extern "C" int vgl_pack_set_error(int code, const char* msg);       // vgl_host.cpp: records the message for vgl_last_error()

extern "C" int64_t vgl_gvcf_workspace_bytes(int32_t n_samples, int32_t n_sites) {
    if (n_samples < 0 || n_sites < 0) return -1;
    const int64_t S = n_sites, E = (int64_t)n_sites * n_samples;
    return 5 * al(S * 4) + al(E * 8) + al(E * 4);
}

extern "C" int vgl_gvcf_blocks_device(int32_t device, int32_t n_samples, int32_t n_sites, const vgl_gvcf_in* in, const vgl_gvcf_out* out,
                                      void* workspace, int64_t workspace_bytes, void* hip_stream) {
    if (!in || !out || n_samples < 1 || n_sites < 0 || in->n_dps < 0 || (in->n_dps > 0 && !in->dps))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_gvcf_blocks_device: bad argument");
    if (!out->counts) return vgl_pack_set_error(VGL_E_ARG, "vgl_gvcf_blocks_device: null counts");
    if (n_sites > 0 && (!in->site_status || !in->n_alleles_obs || !in->n_alleles || !in->contig || !in->pos0 || !in->dp || !in->pl ||
                        !out->items || !out->block_dp || !out->block_pl || !out->block_n_alleles || !out->block_status || !out->record_status))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_gvcf_blocks_device: null array");
    if (in->dp_site_stride < n_samples || in->pl_site_stride < 3 * (int64_t)n_samples)
        return vgl_pack_set_error(VGL_E_ARG, "vgl_gvcf_blocks_device: dp_site_stride < n_samples or pl_site_stride < 3 n_samples");
    if (n_sites > 0 && (!workspace || workspace_bytes < vgl_gvcf_workspace_bytes(n_samples, n_sites)))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_gvcf_blocks_device: workspace smaller than vgl_gvcf_workspace_bytes()");
    if (hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_gvcf_blocks_device: hipSetDevice failed");
    hipStream_t st = (hipStream_t)hip_stream;
    if (n_sites == 0) {
        if (hipMemsetAsync(out->counts, 0, 4 * sizeof(int32_t), st) != hipSuccess ||
            hipMemsetAsync(out->counts + 2, 0xFF, sizeof(int32_t), st) != hipSuccess)
            return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_gvcf_blocks_device: hipMemsetAsync failed");
        return VGL_OK;
    }
    const GvcfArgs A = make_args(n_samples, n_sites, in, out, workspace);
    int W = 1;
    while (W < 64 && W < n_samples) W <<= 1;
    const int64_t E = (int64_t)n_sites * n_samples, C = ((int64_t)n_sites + CH - 1) / CH * n_samples;
    if ((E + NT - 1) / NT > 0x7fffffff || (C + NT - 1) / NT > 0x7fffffff) return vgl_pack_set_error(VGL_E_ARG, "vgl_gvcf_blocks_device: tile too large");
    hipLaunchKernelGGL(k_gvcf_site, dim3((unsigned)((n_sites + NT / W - 1) / (NT / W))), dim3(NT), 0, st, A, W);
    hipLaunchKernelGGL(k_gvcf_scan, dim3(1), dim3(SCAN_NT), 0, st, A);
    hipLaunchKernelGGL(k_gvcf_init, dim3((unsigned)((E + NT - 1) / NT)), dim3(NT), 0, st, A);
    hipLaunchKernelGGL(k_gvcf_agg, dim3((unsigned)((C + NT - 1) / NT)), dim3(NT), 0, st, A);
    hipLaunchKernelGGL(k_gvcf_final, dim3((unsigned)((E + NT - 1) / NT)), dim3(NT), 0, st, A);
    if (hipGetLastError() != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_gvcf_blocks_device: a launch failed");
    return VGL_OK;
}

// (library-internal, for vgl_simulate_tile_gvcf_async) the first and last block's aggregates into `edge` after vgl_gvcf_blocks_device
extern "C" int vgl_gvcf_edges_device(int32_t n_samples, int32_t n_sites, const vgl_gvcf_in* in, const vgl_gvcf_out* out, void* workspace,
                                     int32_t* edge, void* hip_stream) {
    if (n_sites == 0) return VGL_OK;
    const GvcfArgs A = make_args(n_samples, n_sites, in, out, workspace);
    const int64_t n = in->pl_site_stride > n_samples ? in->pl_site_stride : n_samples;
    const unsigned gx = (unsigned)((n + NT - 1) / NT < 64 ? (n + NT - 1) / NT : 64);
    hipLaunchKernelGGL(k_gvcf_edges, dim3(gx, 2), dim3(NT), 0, (hipStream_t)hip_stream, A, edge);
    if (hipGetLastError() != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_gvcf_edges_device: a launch failed");
    return VGL_OK;
}
