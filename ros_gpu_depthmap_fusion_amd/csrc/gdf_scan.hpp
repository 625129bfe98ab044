// gdf_scan.hpp — the exclusive scan of u32 words (gdf_scan.hip) and its 256-thread block scan, shared
// by the radius filter (gdf_filter.hip) and the object-points stage (gdf_object_points.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gdf {

constexpr int kScanThreads = 256;      // block size of the scan kernels and of block_excl_scan: 4 waves
constexpr uint32_t kScanTile = 1024;   // words per scan tile (256 threads x 4)

// words of the scan workspace for an m-item scan (the tile sums)
inline size_t scan_words(size_t m) { return (m + kScanTile - 1) / kScanTile + 1; }

// Exclusive scan of m u32 words: out[i] = sum of in[< i], out[m] = the total (also to *total_out when
// not null).  in == out is allowed; zero_in (in != out only) leaves in[0 .. m) zero.  sums holds
// scan_words(m) words.  One block scans alone up to 8 tiles (one launch), else tile sums -> one-block
// scan of the sums -> apply (three launches).
hipError_t launch_excl_scan(uint32_t* in, uint32_t* out, uint32_t m, uint32_t* sums, bool zero_in,
                            uint32_t* total_out, hipStream_t st);

// inclusive scan of v over the wave's 64 lanes by op (associative)
template <class Op>
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, Op op) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v = op(v, t);
    }
    return v;
}

// exclusive scan of v over the block's 256 threads; *total = the block's sum.  sh: 4 words
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* total, uint32_t* sh) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan(v, [](uint32_t x, uint32_t y) { return x + y; });
    if (lane == 63u) sh[w] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanThreads / 64; ++k) {
        const uint32_t s = sh[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();  // (sh may be rewritten by the caller's next scan)
    *total = tot;
    return base + incl - v;
}

}  // namespace gdf
