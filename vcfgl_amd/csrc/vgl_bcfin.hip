// vgl_bcfin.hip -- the FORMAT/GT vectors of BCF records decoded on the device (ABI 7 additions: vgl_bcfin_workspace_bytes,
// vgl_bcfin_decode_device; vgl_bcfin_host_* in hostlib/batch.h launches k_bcfin_decode through vgl_launch_bcfin_decode).  The mirror image of vgl_vcfin.hip for the binary format: the host program's read_bcf +
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

using BcfinArgs = VglBcfinArgs;
using vgl_bcfin::slice_ok;

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

}  // namespace

extern "C" int vgl_launch_bcfin_decode(const VglBcfinArgs* a, void* stream) {
    hipLaunchKernelGGL(k_bcfin_decode, dim3((unsigned)((a->n_records + WAVES - 1) / WAVES)), dim3(NT), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

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
    if (vgl_launch_bcfin_decode(&A, st) != 0) return vgl_pack_set_error(VGL_E_NODEVICE, "vgl_bcfin_decode_device: the launch failed");
    return VGL_OK;
}
