// vgl_bcfin.hip -- the FORMAT/GT vectors of BCF records decoded on the device (ABI 7 additions: vgl_bcfin_workspace_bytes,
// vgl_bcfin_decode_device, vgl_bcfin_host_*).  The mirror image of vgl_vcfin.hip for the binary format: the host program's read_bcf +
// make_site are the specification, the per-sample rule is vgl_bcfin_core.h.  Per record, the GT vector of every sample (n values of
// BCF type int8 / int16 / int32, a fixed stride: no scan, no LDS) becomes the packed byte (b1 << 4) | b0 that the tile calls take, and
// the non-missing allele indices are summed.  A record with a value outside the plain rule, a GT type that is no integer type, n < 1
// or n_alleles outside 1 .. 5 gets the status VGL_BCFIN_HOST: its row is unspecified and the caller decodes it.
//   k_bcfin_check   every slice [gt_begin, gt_begin + n_samples * n * w) of a record with an integer type and n >= 1 against gt_bytes;
//                   one flag word
//   k_bcfin_decode  workgroups of 256 lanes, one record per wavefront, no LDS, no barrier.  int8 with n == 2 (what every writer
//                   emits for diploid calls): a lane takes 8 samples -- 16 bytes in, 8 packed bytes out -- per step, the last
//                   N % 8 samples one by one.  Any other type and n: one sample per lane and step, its values assembled from single
//                   bytes.  Slices and rows start at any address (BCF records are not aligned; rows are not when N % 8 != 0): the
//                   16- and 8-byte accesses go through memcpy and never leave the slice or the row.  The allele sum and the status
//                   are wavefront reductions that lane 0 stores.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vcfgl_hip.h"
#include "vgl_device.h"
#include "vgl_bcfin_core.h"

namespace {

constexpr int NT = 256;                  // lanes per workgroup
constexpr int WAVES = NT / 64;           // records per workgroup
constexpr int64_t WS_BYTES = 256;        // the flag word of k_bcfin_check

struct BcfinArgs {
    const uint8_t* gt; int64_t gt_bytes; int32_t n_records, N;
    const int64_t* gt_begin; const int32_t* gt_type; const int32_t* gt_n; const int32_t* n_alleles; const int8_t* allele_map;
    uint8_t* gt_out; int32_t* allelesum_out; int32_t* status_out;
};

// does the slice of a record with an integer type and n >= 1 lie inside the bytes?  (w = 0 or n < 1: nothing is read, nothing to check)
__host__ __device__ inline bool slice_ok(const int64_t begin, const int w, const int32_t n, const int64_t N, const int64_t gt_bytes) {
    if (w == 0 || n < 1) return true;
    if (begin < 0 || begin > gt_bytes) return false;
    return (gt_bytes - begin) / (N * w) >= (int64_t)n;                 // (N * w <= 2^33: no overflow, whatever n is)
}

__global__ void __launch_bounds__(NT) k_bcfin_check(int32_t n_records, int64_t gt_bytes, int32_t N, const int64_t* __restrict__ gt_begin,
                                                    const int32_t* __restrict__ gt_type, const int32_t* __restrict__ gt_n, uint32_t* __restrict__ flag) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n_records; i += (int64_t)gridDim.x * NT)
        bad |= !slice_ok(gt_begin[i], vgl_bcfin::width(gt_type[i]), gt_n[i], N, gt_bytes);
    if (__any(bad) && (threadIdx.x & 63) == 0) *flag = 1u;       // (every writer stores the same word)
}

__global__ void __launch_bounds__(NT) k_bcfin_decode(const BcfinArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t rec = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (rec >= A.n_records) return;                                    // (wavefront-uniform, as everything up to the loops is)
    const int64_t N = A.N;
    const int type = A.gt_type[rec], n = A.gt_n[rec], nal = A.n_alleles[rec];
    const int64_t begin = A.gt_begin[rec];
    const int w = vgl_bcfin::width(type);
    // outside what the rule describes: the caller's record.  A slice outside the bytes is refused by the entry point; never read it
    if (!vgl_bcfin::describable(type, n, nal) || !slice_ok(begin, w, n, N, A.gt_bytes)) {
        if (lane == 0) { A.status_out[rec] = VGL_BCFIN_HOST; A.allelesum_out[rec] = 0; }
        return;
    }
    const uint32_t map = vgl_bcfin::map_word(A.allele_map + rec * 5);
    const uint8_t* __restrict__ src = A.gt + begin;
    uint8_t* __restrict__ row = A.gt_out + rec * N;
    int sum = 0, bad = 0;
    if (w == 1 && n == 2) {
        for (int64_t s0 = (int64_t)lane * vgl_bcfin::OCT; s0 < N; s0 += 64 * vgl_bcfin::OCT) {
            if (s0 + vgl_bcfin::OCT <= N) {                            // bytes [2 s0, 2 s0 + 16) of the slice, bytes [s0, s0 + 8) of the row
                uint32_t in[4], out[2];
                memcpy(in, src + 2 * s0, 16);
                if (!vgl_bcfin::oct8(in, nal, map, out, sum)) bad = 1;
                memcpy(row + s0, out, 8);
            } else {
                for (int64_t s = s0; s < N; s++) {
                    uint32_t b; int t;
                    if (!vgl_bcfin::sample(src + 2 * s, 1, 2, nal, map, b, t)) bad = 1;
                    row[s] = (uint8_t)b; sum += t;
                }
            }
        }
    } else {
        const int64_t stride = (int64_t)n * w;
        for (int64_t s = lane; s < N; s += 64) {
            uint32_t b; int t;
            if (!vgl_bcfin::sample(src + s * stride, w, n, nal, map, b, t)) bad = 1;
            row[s] = (uint8_t)b; sum += t;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { sum += __shfl_down(sum, d, 64); bad |= __shfl_down(bad, d, 64); }
    if (lane == 0) { A.allelesum_out[rec] = sum; A.status_out[rec] = bad ? VGL_BCFIN_HOST : VGL_BCFIN_OK; }
}

int launch_decode(const BcfinArgs& A, hipStream_t st) {
    hipLaunchKernelGGL(k_bcfin_decode, dim3((unsigned)((A.n_records + WAVES - 1) / WAVES)), dim3(NT), 0, st, A);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

static_assert(VGL_BCFIN_OK == vgl_bcfin::ST_OK && VGL_BCFIN_HOST == vgl_bcfin::ST_HOST, "the statuses of the header and of the core");

extern "C" int vgl_pack_set_error(int code, const char* msg);       // vgl_host.cpp: records the message for vgl_last_error()

extern "C" int64_t vgl_bcfin_workspace_bytes(int32_t n_samples, int32_t n_records) {
    if (n_samples <= 0 || n_records < 0) return -1;
    return WS_BYTES;
}

extern "C" int vgl_bcfin_decode_device(int32_t device, const uint8_t* gt, int64_t gt_bytes, int32_t n_records, const int64_t* gt_begin,
                                       const int32_t* gt_type, const int32_t* gt_n, const int32_t* n_alleles, const int8_t* allele_map,
                                       int32_t n_samples, uint8_t* gt_out, int32_t* allelesum_out, int32_t* status_out, void* workspace,
                                       void* hip_stream) {
    if (n_records < 0 || n_samples <= 0 || gt_bytes < 0) return vgl_pack_set_error(VGL_E_ARG, "vgl_bcfin_decode_device: bad argument");
    if (n_records > 0 && (!gt || !gt_begin || !gt_type || !gt_n || !n_alleles || !allele_map || !gt_out || !allelesum_out || !status_out || !workspace))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_bcfin_decode_device: null argument");
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcfin_decode_device: no HIP device is available");
    if (device < 0 || device >= nd || hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcfin_decode_device: no such device");
    if (n_records == 0) return VGL_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    // the slices are described by device memory: one small kernel compares them with gt_bytes and the call waits for its one word --
    // a slice outside the bytes is refused before the decoder is launched (the decode itself is not waited for)
    uint32_t* flag = (uint32_t*)workspace; uint32_t h_flag = 0;
    if (hipMemsetAsync(flag, 0, sizeof(uint32_t), st) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcfin_decode_device: hipMemsetAsync failed");
    const int cg = (n_records + NT - 1) / NT < 1024 ? (n_records + NT - 1) / NT : 1024;
    hipLaunchKernelGGL(k_bcfin_check, dim3((unsigned)cg), dim3(NT), 0, st, n_records, gt_bytes, n_samples, gt_begin, gt_type, gt_n, flag);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h_flag, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcfin_decode_device: the argument check failed to run");
    if (h_flag) return vgl_pack_set_error(VGL_E_ARG, "vgl_bcfin_decode_device: a GT slice lies outside the bytes (0 <= gt_begin, gt_begin + n_samples * n * width <= gt_bytes)");
    BcfinArgs A{gt, gt_bytes, n_records, n_samples, gt_begin, gt_type, gt_n, n_alleles, allele_map, gt_out, allelesum_out, status_out};
    if (launch_decode(A, st) != 0) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcfin_decode_device: the launch failed");
    return VGL_OK;
}

// ---- host batches (vgl_bcfin_host_*): what a program without HIP of its own (the host program) uses -----------------------------
struct vgl_bcfin_host {
    int device = 0; int32_t N = 0, max_records = 0; int64_t max_gt = 0;
    hipStream_t st = nullptr;
    struct Slot {
        uint8_t* h_in = nullptr; uint8_t* d_in = nullptr;          // the GT slices back to back, then the five per-record arrays (one copy up)
        uint8_t* h_out = nullptr; uint8_t* d_out = nullptr;        // rows, sums, statuses (one copy down)
        int32_t n = 0; hipEvent_t done = nullptr; bool busy = false;
        int64_t off_sum = 0, off_status = 0;                       // this batch's sums and statuses in h_out / d_out, behind its rows
    } s[2];
    int next = 0;
    int64_t in_bytes = 0, out_bytes = 0;                           // capacity of h_in / d_in and of h_out / d_out
};

extern "C" int vgl_bcfin_host_destroy(vgl_bcfin_host* h) {
    if (!h) return VGL_OK;
    (void)hipSetDevice(h->device);
    if (h->st) (void)hipStreamSynchronize(h->st);
    for (auto& S : h->s) {
        if (S.d_in) (void)hipFree(S.d_in);
        if (S.d_out) (void)hipFree(S.d_out);
        if (S.h_in) (void)hipHostFree(S.h_in);
        if (S.h_out) (void)hipHostFree(S.h_out);
        if (S.done) (void)hipEventDestroy(S.done);
    }
    if (h->st) (void)hipStreamDestroy(h->st);
    delete h;
    return VGL_OK;
}

extern "C" int vgl_bcfin_host_create(int32_t device, int32_t n_samples, int32_t max_records, int64_t max_gt_bytes, vgl_bcfin_host** out) {
    if (!out || n_samples <= 0 || max_records <= 0 || max_gt_bytes <= 0) return vgl_pack_set_error(VGL_E_ARG, "vgl_bcfin_host_create: bad argument");
    *out = nullptr;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcfin_host_create: no HIP device is available");
    if (device < 0 || device >= nd) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcfin_host_create: no such device");
    if (hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcfin_host_create: hipSetDevice failed");
    vgl_bcfin_host* h = new vgl_bcfin_host;
    h->device = device; h->N = n_samples; h->max_records = max_records; h->max_gt = max_gt_bytes;
    auto up = [](int64_t x) { return (x + 255) & ~(int64_t)255; };
    const int64_t L = max_records;
    h->in_bytes = up(max_gt_bytes) + up(L * 8) + 3 * up(L * 4) + up(L * 5);
    h->out_bytes = up(L * (int64_t)n_samples) + 2 * up(L * 4);
    bool ok = hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) == hipSuccess;
    for (auto& S : h->s)
        ok = ok && hipMalloc((void**)&S.d_in, (size_t)h->in_bytes) == hipSuccess && hipMalloc((void**)&S.d_out, (size_t)h->out_bytes) == hipSuccess &&
             hipHostMalloc((void**)&S.h_in, (size_t)h->in_bytes, hipHostMallocDefault) == hipSuccess &&
             hipHostMalloc((void**)&S.h_out, (size_t)h->out_bytes, hipHostMallocDefault) == hipSuccess &&
             hipEventCreateWithFlags(&S.done, hipEventDisableTiming) == hipSuccess;
    if (!ok) { vgl_bcfin_host_destroy(h); return vgl_pack_set_error(VGL_E_NOMEM, "vgl_bcfin_host_create: device or page-locked memory could not be allocated"); }
    *out = h;
    return VGL_OK;
}

extern "C" int vgl_bcfin_host_submit(vgl_bcfin_host* h, const uint8_t* src, int64_t src_bytes, int32_t n_records, const int64_t* gt_begin,
                                     const int32_t* gt_type, const int32_t* gt_n, const int32_t* n_alleles, const int8_t* allele_map, int32_t* ticket) {
    if (!h || !ticket || n_records < 0 || n_records > h->max_records || src_bytes < 0 ||
        (n_records > 0 && (!src || !gt_begin || !gt_type || !gt_n || !n_alleles || !allele_map)))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_bcfin_host_submit: bad argument");
    // only the GT slices go into the staging, back to back: what lies between them in src (the other FORMAT fields, the shared blocks)
    // never crosses the link.  First their ranges and their total, so that a refused batch leaves the staging as it was
    int64_t total = 0;
    for (int32_t i = 0; i < n_records; i++) {
        const int w = vgl_bcfin::width(gt_type[i]);
        if (!slice_ok(gt_begin[i], w, gt_n[i], h->N, src_bytes))
            return vgl_pack_set_error(VGL_E_ARG, "vgl_bcfin_host_submit: a GT slice lies outside the bytes (0 <= gt_begin, gt_begin + n_samples * n * width <= src_bytes)");
        if (w != 0 && gt_n[i] >= 1) total += (int64_t)h->N * gt_n[i] * w;
        if (total > h->max_gt) return vgl_pack_set_error(VGL_E_ARG, "vgl_bcfin_host_submit: the batch's GT slices exceed max_gt_bytes");
    }
    const int k = h->next;
    auto& S = h->s[k];
    if (S.busy) return vgl_pack_set_error(VGL_E_ARG, "vgl_bcfin_host_submit: two batches are in flight (vgl_bcfin_host_wait the older one first)");
    if (hipSetDevice(h->device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcfin_host_submit: hipSetDevice failed");
    S.n = n_records;
    if (n_records > 0) {
        // slices and arrays lie back to back in the staging (sized by n_records) and go up in one copy; rows, sums and statuses come
        // down in one.  Once something is enqueued a failure waits for the stream: the staging is read by it
        auto up = [](int64_t x) { return (x + 255) & ~(int64_t)255; };
        const int64_t L = n_records;
        const int64_t o_beg = up(total), o_type = o_beg + up(L * 8), o_n = o_type + up(L * 4), o_nal = o_n + up(L * 4), o_map = o_nal + up(L * 4);
        const int64_t in_used = o_map + L * 5;
        S.off_sum = up(L * h->N); S.off_status = S.off_sum + up(L * 4);
        const int64_t out_used = S.off_status + L * 4;
        int64_t* packed = (int64_t*)(S.h_in + o_beg);
        int64_t at = 0;
        for (int32_t i = 0; i < n_records; i++) {
            const int w = vgl_bcfin::width(gt_type[i]);
            const int64_t len = (w != 0 && gt_n[i] >= 1) ? (int64_t)h->N * gt_n[i] * w : 0;
            packed[i] = at;
            if (len > 0) memcpy(S.h_in + at, src + gt_begin[i], (size_t)len);
            at += len;
        }
        memcpy(S.h_in + o_type, gt_type, (size_t)L * 4); memcpy(S.h_in + o_n, gt_n, (size_t)L * 4);
        memcpy(S.h_in + o_nal, n_alleles, (size_t)L * 4); memcpy(S.h_in + o_map, allele_map, (size_t)L * 5);
        auto fail = [&](const char* msg) { (void)hipStreamSynchronize(h->st); return vgl_pack_set_error(VGL_E_NODEVICE, msg); };
        if (hipMemcpyAsync(S.d_in, S.h_in, (size_t)in_used, hipMemcpyHostToDevice, h->st) != hipSuccess) return fail("vgl_bcfin_host_submit: copy to the device failed");
        BcfinArgs A{S.d_in, total, n_records, h->N, (const int64_t*)(S.d_in + o_beg), (const int32_t*)(S.d_in + o_type), (const int32_t*)(S.d_in + o_n),
                    (const int32_t*)(S.d_in + o_nal), (const int8_t*)(S.d_in + o_map), S.d_out, (int32_t*)(S.d_out + S.off_sum), (int32_t*)(S.d_out + S.off_status)};
        if (launch_decode(A, h->st) != 0) return fail("vgl_bcfin_host_submit: the launch failed");
        if (hipMemcpyAsync(S.h_out, S.d_out, (size_t)out_used, hipMemcpyDeviceToHost, h->st) != hipSuccess) return fail("vgl_bcfin_host_submit: copy back failed");
    }
    if (hipEventRecord(S.done, h->st) != hipSuccess) { (void)hipStreamSynchronize(h->st); return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcfin_host_submit: enqueue failed"); }
    S.busy = true;
    *ticket = k;
    h->next = k ^ 1;
    return VGL_OK;
}

extern "C" int vgl_bcfin_host_wait(vgl_bcfin_host* h, int32_t ticket, const uint8_t** gt, const int32_t** allelesum, const int32_t** status) {
    if (!h || ticket < 0 || ticket > 1 || !gt || !allelesum || !status || !h->s[ticket].busy) return vgl_pack_set_error(VGL_E_ARG, "vgl_bcfin_host_wait: bad ticket");
    auto& S = h->s[ticket];
    if (hipSetDevice(h->device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcfin_host_wait: hipSetDevice failed");
    if (hipEventSynchronize(S.done) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcfin_host_wait: the decode failed");
    S.busy = false;
    *gt = S.h_out; *allelesum = (const int32_t*)(S.h_out + S.off_sum); *status = (const int32_t*)(S.h_out + S.off_status);
    return VGL_OK;
}
