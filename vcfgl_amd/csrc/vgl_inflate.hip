// vgl_inflate.hip -- BGZF input inflated on the device (ABI 7 additions: vgl_inflate_workspace_bytes, vgl_inflate_members_device;
// vgl_inflate_host_* in hostlib/batch.h launches k_inflate_member through vgl_launch_inflate_members).  The counterpart of vgl_bgzf.hip: BGZF members are independent gzip members of at most 64 KiB of output, so
// every member is decoded by a workgroup of its own with its output window in LDS.  zlib's inflate is the specification; a member
// the decoder does not take to its exact end (ISIZE bytes, the trailer's CRC32, the data ending where the trailer begins) gets the
// status VGL_INFLATE_HOST and the caller inflates it itself.  Nothing is guessed on the device.
//   k_inflate_check   the members' ranges against the buffers: one flag word
//   k_inflate_member  one workgroup of ONE wavefront per member.  The symbol decode of a member is serial (vgl_inflate_core.h: every
//                     lane runs it on the same values, so the wavefront's control flow is uniform); what the 64 lanes share out is
//                     the bytes of every match and stored block, the write-out and the CRC32.  One wavefront and not four: the
//                     decode is a chain of dependent LDS reads of some hundred cycles per symbol, tens of thousands of symbols per
//                     member, against some ten thousand cycles for write-out and CRC32 together -- more lanes would shorten only
//                     the latter, and a second wavefront would turn the ordering of every match's copy behind the stores before it
//                     (a wavefront's own LDS operations are in order) into a workgroup barrier per match.  The parallelism is
//                     across members: 76.0 KiB of LDS per workgroup is two members per CU, 512 members resident on 256 CUs.
//     LDS             the window (64 KiB + 16: the member's byte j lies at index j + (address of its first output byte & 15), so
//                     that 16-byte LDS reads and 16-byte global stores are aligned together), the decode tables of the current
//                     block (4 KiB) and, when the deflate data is at most 8 KiB (VCF text compresses below a twentieth), the data
//                     itself; longer data is read from global memory through the same bit reader, four bytes at a time.
//     matches         resolved in LDS, from bytes before the match's start only (vgl_inflate_core.h)
//     write-out       lane-striped 16-byte stores between a head and a tail of single bytes, bounded by isize
//     CRC32           64 slices of 1024 bytes aligned to the member's end, one per lane, combined by the tree of GF(2) shift
//                     operators the compressor uses (vgl_crc32.hip.h: levels 4..9, through wavefront shuffles)
// The kernel reads no byte outside [begin, begin + csize) clamped to the source and writes no byte outside [out_off, out_off + isize)
// clamped to the destination, whatever the bytes hold.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vcfgl_hip.h"
#include "vgl_device.h"
#include "vgl_crc32.hip.h"
#include "vgl_inflate_core.h"

namespace {

constexpr int NT = 64;                     // one wavefront per member
constexpr int IN_LDS = 8192;               // deflate data of at most this many bytes is staged in LDS
constexpr int GRID_MAX = 1 << 16;
constexpr int64_t WS_BYTES = 256;          // the flag word of k_inflate_check

__constant__ CrcShifts c_crc_shift = make_crc_shifts();

using InflateArgs = VglInflateArgs;

__device__ __forceinline__ bool range_bad(const InflateArgs& A, const int64_t b, const int32_t c, const int64_t o, const int32_t n) {
    return b < 0 || c < 0 || b > A.src_bytes || (int64_t)c > A.src_bytes - b || n < 0 || n > 65536 || o < 0 || o > A.dst_cap || (int64_t)n > A.dst_cap - o;
}

__global__ void __launch_bounds__(256) k_inflate_check(const InflateArgs A, uint32_t* __restrict__ flag) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < A.n_members; i += (int64_t)gridDim.x * 256)
        bad |= range_bad(A, A.begin[i], A.csize[i], A.out_off[i], A.isize[i]);
    if (__any(bad) && (threadIdx.x & 63) == 0) *flag = 1u;       // (every writer stores the same word)
}

struct Smem {
    alignas(16) uint8_t win[65536 + 16];
    alignas(16) uint8_t in[IN_LDS];
    vgl_inflate_tabs tabs;
};
static_assert(sizeof(Smem) <= 81920, "two member workgroups per CU");

__global__ void __launch_bounds__(NT) k_inflate_member(const InflateArgs A) {
    __shared__ Smem sm;
    const int lane = threadIdx.x;
    for (int64_t m = blockIdx.x; m < A.n_members; m += gridDim.x) {
        const int64_t begin = A.begin[m], out_off = A.out_off[m];
        const int32_t csize = A.csize[m], isize = A.isize[m];
        int bad = range_bad(A, begin, csize, out_off, isize);                 // (k_inflate_check refused it already: nothing is touched)
        int32_t size = 0, at = 0; uint32_t crc_want = 0, isize_want = 0;
        if (!bad) bad = !vgl_bgzf_member_at(A.src + begin, 0, csize, size, at, crc_want, isize_want) || size != csize || isize_want != (uint32_t)isize;
        if (bad) { if (lane == 0) A.status[m] = VGL_INFLATE_HOST; continue; }
        const uint8_t* in = A.src + begin + at;
        const int32_t in_len = csize - at - 8;
        uint8_t* out = A.dst + out_off;
        const int shift = (int)((uintptr_t)out & 15);
        uint8_t* win = sm.win + shift;
        const uint8_t* data = in;
        if (in_len <= IN_LDS) {
            for (int i = lane; i < in_len; i += NT) sm.in[i] = in[i];
            data = sm.in;
        }
        __syncthreads();
        const int rc = vgl_inflate_core(data, in_len, win, isize, &sm.tabs, lane, NT);
        __syncthreads();
        uint32_t r = 0;
        if (rc == 0) {
            // ---- write-out: [0, head) bytes, 16-byte rows up to tail, bytes again
            int head = (16 - shift) & 15; if (head > isize) head = isize;
            const int rows = (isize - head) >> 4, tail = head + (rows << 4);
            if (lane < head) out[lane] = win[lane];
            for (int i = lane; i < rows; i += NT) *(uint4*)(out + head + 16 * i) = *(const uint4*)(win + head + 16 * i);
            if (tail + lane < isize) out[tail + lane] = win[tail + lane];
            // ---- CRC32: lane l covers [isize - 1024 (64 - l), isize - 1024 (63 - l)) clipped to the member; byte 0's slice starts from 0xffffffff
            int b0 = isize - 1024 * (NT - lane);
            const int b1 = isize - 1024 * (NT - 1 - lane);
            if (b1 > 0) {
                if (b0 <= 0) { b0 = 0; r = 0xffffffffu; }
                int i = b0;
                for (; i < b1 && ((shift + i) & 3); ++i) r = crc32_byte(r, win[i]);
                for (; i + 4 <= b1; i += 4) r = crc32_word(r, *(const uint32_t*)(win + i));
                for (; i < b1; ++i) r = crc32_byte(r, win[i]);
            } else if (isize == 0 && lane == NT - 1) r = 0xffffffffu;         // (an empty member: the register's start, inverted below)
#pragma unroll
            for (int k = 0; k < 6; ++k) {                                      // right operands are whole blocks of 1024 * 2^k bytes
                const uint32_t right = __shfl_down(r, 1 << k, 64);
                if ((lane & ((2 << k) - 1)) == 0) r = gf2_apply(c_crc_shift.s[4 + k], r) ^ right;
            }
        }
        if (lane == 0) A.status[m] = (rc == 0 && (r ^ 0xffffffffu) == crc_want) ? VGL_INFLATE_OK : VGL_INFLATE_HOST;
        __syncthreads();                                                       // LDS is reused by the next member
    }
}

}  // namespace

extern "C" int vgl_launch_inflate_members(const VglInflateArgs* a, void* stream) {
    const int64_t g = a->n_members < GRID_MAX ? a->n_members : GRID_MAX;
    hipLaunchKernelGGL(k_inflate_member, dim3((unsigned)g), dim3(NT), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int vgl_pack_set_error(int code, const char* msg);       // vgl_host.cpp: records the message for vgl_last_error()

extern "C" int64_t vgl_inflate_workspace_bytes(int64_t n_members) {
    if (n_members < 0) return -1;
    return WS_BYTES;
}

extern "C" int vgl_inflate_members_device(int32_t device, const uint8_t* src, int64_t src_bytes, int64_t n_members, const int64_t* begin,
                                          const int32_t* csize, const int64_t* out_off, const int32_t* isize, uint8_t* dst, int64_t dst_cap,
                                          int32_t* status, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    if (n_members < 0 || src_bytes < 0 || dst_cap < 0) return vgl_pack_set_error(VGL_E_ARG, "vgl_inflate_members_device: bad argument");
    if (n_members > 0 && (!src || !begin || !csize || !out_off || !isize || !status || !workspace || (dst_cap > 0 && !dst)))
        return vgl_pack_set_error(VGL_E_ARG, "vgl_inflate_members_device: null argument");
    if (n_members > 0 && workspace_bytes < WS_BYTES) return vgl_pack_set_error(VGL_E_ARG, "vgl_inflate_members_device: workspace smaller than vgl_inflate_workspace_bytes(n_members)");
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_inflate_members_device: no HIP device is available");
    if (device < 0 || device >= nd || hipSetDevice(device) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_inflate_members_device: no such device");
    if (n_members == 0) return VGL_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    const InflateArgs A{src, src_bytes, n_members, begin, csize, out_off, isize, dst, dst_cap, status};
    // the ranges are device memory: one small kernel compares them with the buffers and the call waits for its one word -- a range
    // outside them is refused before the decoder is launched (the decode itself is not waited for)
    uint32_t* flag = (uint32_t*)workspace; uint32_t h_flag = 0;
    if (hipMemsetAsync(flag, 0, sizeof(uint32_t), st) != hipSuccess) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_inflate_members_device: hipMemsetAsync failed");
    const int64_t cg = (n_members + 255) / 256 < 1024 ? (n_members + 255) / 256 : 1024;
    hipLaunchKernelGGL(k_inflate_check, dim3((unsigned)cg), dim3(256), 0, st, A, flag);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h_flag, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_inflate_members_device: the argument check failed to run");
    if (h_flag) return vgl_pack_set_error(VGL_E_ARG, "vgl_inflate_members_device: a member's range lies outside the buffers (0 <= begin, begin + csize <= src_bytes, "
                                                      "0 <= isize <= 65536, 0 <= out_off, out_off + isize <= dst_cap)");
    if (vgl_launch_inflate_members(&A, st) != 0) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_inflate_members_device: the launch failed");
    return VGL_OK;
}
