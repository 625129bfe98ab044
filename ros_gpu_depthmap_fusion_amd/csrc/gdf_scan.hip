// gdf_scan.hip — exclusive scan of u32 words for gfx950 (gdf_scan.hpp): out[i] = sum of in[< i],
// out[m] = the total.
//
//   k_scan_block   one block, any m (a carry between its chunks of kScanTile)
//   k_scan_sums    the sum of each tile of kScanTile words
//   k_scan_apply   each tile scanned, on top of the exclusive scan of the tile sums
#include <hip/hip_runtime.h>

#include "gdf_scan.hpp"

namespace gdf {
namespace {

constexpr int kT = kScanThreads;
constexpr uint32_t kScanOneBlock = 8 * kScanTile;  // up to here one block scans alone (one launch)

// the thread's 4 words of the tile at `first` and their sum
__device__ __forceinline__ uint32_t scan_load(const uint32_t* in, uint32_t m, uint32_t first,
                                              uint32_t v[4]) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        v[k] = first + k < m ? in[first + k] : 0u;
        s += v[k];
    }
    return s;
}

// ... and their places, o the first
__device__ __forceinline__ void scan_store(uint32_t* in, uint32_t* out, uint32_t m, uint32_t first,
                                           const uint32_t v[4], uint32_t o, int zero_in) {
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        if (first + k < m) {
            if (zero_in) in[first + k] = 0u;
            out[first + k] = o;
            o += v[k];
        }
}

__global__ __launch_bounds__(kT) void k_scan_block(uint32_t* in, uint32_t* out, uint32_t m, int zero_in,
                                                    uint32_t* total_out) {
    __shared__ uint32_t sh[4];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < m; base += kScanTile) {
        const uint32_t first = base + threadIdx.x * 4u;
        uint32_t v[4], tot;
        const uint32_t s = scan_load(in, m, first, v);
        const uint32_t o = carry + block_excl_scan(s, &tot, sh);  // (its barriers order reads before writes)
        scan_store(in, out, m, first, v, o, zero_in);
        carry += tot;
    }
    if (threadIdx.x == 0) {
        out[m] = carry;
        if (total_out) *total_out = carry;
    }
}

__global__ __launch_bounds__(kT) void k_scan_sums(const uint32_t* in, uint32_t m, uint32_t* sums) {
    __shared__ uint32_t sh[4];
    uint32_t v[4], tot;
    block_excl_scan(scan_load(in, m, blockIdx.x * kScanTile + threadIdx.x * 4u, v), &tot, sh);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// sums: the exclusive scan of the tile sums, sums[ntiles] = the total
__global__ __launch_bounds__(kT) void k_scan_apply(uint32_t* in, const uint32_t* sums, uint32_t* out,
                                                    uint32_t m, uint32_t ntiles, int zero_in,
                                                    uint32_t* total_out) {
    __shared__ uint32_t sh[4];
    const uint32_t first = blockIdx.x * kScanTile + threadIdx.x * 4u;
    uint32_t v[4], tot;
    const uint32_t s = scan_load(in, m, first, v);
    const uint32_t o = sums[blockIdx.x] + block_excl_scan(s, &tot, sh);
    scan_store(in, out, m, first, v, o, zero_in);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[m] = sums[ntiles];
        if (total_out) *total_out = sums[ntiles];
    }
}

}  // namespace

hipError_t launch_excl_scan(uint32_t* in, uint32_t* out, uint32_t m, uint32_t* sums, bool zero_in,
                            uint32_t* total_out, hipStream_t st) {
    const int z = zero_in ? 1 : 0;
    if (m <= kScanOneBlock) {
        hipLaunchKernelGGL(k_scan_block, dim3(1), dim3(kT), 0, st, in, out, m, z, total_out);
        return hipGetLastError();
    }
    const uint32_t nt = (m + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(k_scan_sums, dim3(nt), dim3(kT), 0, st, in, m, sums);
    hipLaunchKernelGGL(k_scan_block, dim3(1), dim3(kT), 0, st, sums, sums, nt, 0, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_scan_apply, dim3(nt), dim3(kT), 0, st, in, sums, out, m, nt, z, total_out);
    return hipGetLastError();
}

}  // namespace gdf
