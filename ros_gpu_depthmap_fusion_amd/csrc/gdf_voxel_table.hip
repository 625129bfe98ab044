// gdf_voxel_table.hip — the voxel table of a list of cell indices, for gfx950
// (include/gdf_segment.h).
//
// The rule: vox_cells = the distinct cells below num_cells, ascending; point_voxel[i] = the place of
// cells[i] in it (GDF_VOX_NONE for a cell at or above num_cells); vox_counts[g] = the rows of voxel
// g.  Bit marks, popcounts, an integer scan and integer adds: the result is exact and order-free.
//
//   (clear)       hipMemsetAsync of the bitmap: one bit per cell.  Unlike the object-points
//                 workspace it HAS to be zero before the marks
//   k_vt_mark     one thread per row: bit (c & 31) of word (c >> 5); a lane whose cell equals the
//                 lane below it leaves the OR to that lane, and a bit seen set is not set again
//   k_vt_rows     popcount sum of every row of kVtRowWords bitmap words
//   scan          exclusive scan of the row sums (gdf_scan.hip); its total is G
//   k_vt_expand   one thread per bitmap word: word_rank[w] = the row's prefix + a row-wide scan of
//                 the popcounts; the cell of every set bit to vox_cells, 0 to the same vox_counts
//   k_vt_rank     one thread per row: point_voxel = word_rank[w] + popc(word & below(b)); one add
//                 into vox_counts per run of equal cells and wave
//   k_vt_weights  weights[j] = vox_counts[index[j]]
#include <hip/hip_runtime.h>

#include "gdf_voxel_table.hpp"

namespace gdf {
namespace {

constexpr int kT = 256;  // block size of every kernel here: 4 waves
static_assert(kVtRowWords <= 64 && (kVtRowWords & (kVtRowWords - 1)) == 0 && kT % kVtRowWords == 0,
              "a counted row is a power-of-two group of lanes inside one wave");

__device__ __forceinline__ uint32_t vt_n(const uint32_t* n_dev, uint32_t n_cap) {
    return n_dev ? min(*n_dev, n_cap) : n_cap;
}

// the first row of the call (a segmented table skips the rows before its first segment)
__device__ __forceinline__ uint32_t vt_first(const VoxTableArgs& a) { return a.first_dev ? *a.first_dev : 0u; }

// the cell of row i; kVtNone for a row outside [first, n) and for a cell outside the grid
__device__ __forceinline__ uint32_t vt_cell(const VoxTableArgs& a, uint32_t n, uint64_t i) {
    if (i >= n || i < vt_first(a)) return kVtNone;
    const uint32_t c = a.cells[i];
    return c < a.num_cells ? c : kVtNone;
}

__global__ __launch_bounds__(kT) void k_vt_mark(const VoxTableArgs a) {
    const uint32_t n = vt_n(a.n_dev, a.n_cap);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c = vt_cell(a, n, (uint64_t)blockIdx.x * kT + threadIdx.x);
    const uint32_t below = __shfl_up(c, 1, 64);  // (every lane of the wave is here)
    if (c != kVtNone && (lane == 0u || below != c)) {
        // a bit that is seen set needs no OR (a frame's runs hit the same few voxels thousands of
        // times); a stale 0 only costs the OR
        const uint32_t bit = 1u << (c & 31u);
        if (!(__hip_atomic_load(&a.bitmap[c >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit))
            (void)__hip_atomic_fetch_or(&a.bitmap[c >> 5], bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the sum of v over the lane's group of kVtRowWords lanes (every lane gets it)
__device__ __forceinline__ uint32_t row_sum(uint32_t v) {
#pragma unroll
    for (int d = 1; d < (int)kVtRowWords; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(kT) void k_vt_rows(const VoxTableArgs a, uint32_t words) {
    const uint32_t w = blockIdx.x * kT + threadIdx.x;
    const uint32_t s = row_sum(w < words ? (uint32_t)__popc(a.bitmap[w]) : 0u);
    if (w % kVtRowWords == 0u && w < words) a.row_rank[w / kVtRowWords] = s;
}

__global__ __launch_bounds__(kT) void k_vt_expand(const VoxTableArgs a, uint32_t words) {
    const uint32_t w = blockIdx.x * kT + threadIdx.x;
    const uint32_t lr = threadIdx.x % kVtRowWords;  // the word's place in its row
    uint32_t bits = w < words ? a.bitmap[w] : 0u;
    const uint32_t p = (uint32_t)__popc(bits);
    uint32_t incl = p;
#pragma unroll
    for (int d = 1; d < (int)kVtRowWords; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, kVtRowWords);
        if (lr >= (uint32_t)d) incl += t;
    }
    if (w == 0u) {  // (the scan before this launch left G)
        const uint32_t G = *a.G;
        *a.limited = a.limit_dev ? min(G, *a.limit_dev) : G;
    }
    if (w >= words) return;
    uint32_t g = a.row_rank[w / kVtRowWords] + incl - p;
    a.word_rank[w] = g;
    while (bits) {
        const uint32_t b = (uint32_t)__ffs((int)bits) - 1u;
        bits &= bits - 1u;
        if (g < a.vox_cap) {  // (always: G <= min(n, num_cells))
            a.vox_cells[g] = w * 32u + b;
            a.vox_counts[g] = 0u;
        }
        ++g;
    }
}

__global__ __launch_bounds__(kT) void k_vt_rank(const VoxTableArgs a) {
    const uint32_t n = vt_n(a.n_dev, a.n_cap);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
    const uint32_t c = vt_cell(a, n, i);
    uint32_t g = kVtNone;
    if (c != kVtNone) g = a.word_rank[c >> 5] + (uint32_t)__popc(a.bitmap[c >> 5] & ((1u << (c & 31u)) - 1u));
    if (i < n && i >= vt_first(a)) a.point_voxel[i] = g;
    // runs of equal cells inside the wave: the head adds the run's length (an outside row or one
    // beyond n differs from every cell, so it ends a run; its own run adds nothing)
    const uint32_t below = __shfl_up(c, 1, 64);
    const bool head = lane == 0u || below != c;
    const uint64_t heads = __ballot(head);
    if (head && c != kVtNone && g < a.vox_cap) {
        const uint64_t rest = lane == 63u ? 0ull : heads >> (lane + 1u);
        const uint32_t len = rest ? (uint32_t)__ffsll((unsigned long long)rest) : 64u - lane;
        (void)__hip_atomic_fetch_add(&a.vox_counts[g], len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kT) void k_vt_weights(const uint32_t* vox_counts, const uint32_t* index,
                                                    const uint32_t* total, uint32_t n_cap,
                                                    uint32_t* weights) {
    const uint32_t n = min(*total, n_cap);
    const uint64_t j = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (j < n) weights[j] = vox_counts[index[j]];
}

inline uint32_t blocks(uint64_t n) { return (uint32_t)((n + kT - 1) / kT); }

}  // namespace

hipError_t launch_voxel_table(const VoxTableArgs& a, hipStream_t st, hipEvent_t* ev) {
    const uint32_t words = vt_words(a.num_cells), rows = vt_rows(a.num_cells);
    hipError_t e;
    auto mark = [&](uint32_t k) { return ev ? hipEventRecord(ev[k], st) : hipSuccess; };
    if ((e = mark(0)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.bitmap, 0, (size_t)words * 4, st)) != hipSuccess) return e;
    if ((e = mark(1)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_vt_mark, dim3(blocks(a.n_cap)), dim3(kT), 0, st, a);
    if ((e = mark(2)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_vt_rows, dim3(blocks(words)), dim3(kT), 0, st, a, words);
    if ((e = launch_excl_scan(a.row_rank, a.row_rank, rows, a.sums, false, a.G, st)) != hipSuccess) return e;
    if ((e = mark(3)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_vt_expand, dim3(blocks(words)), dim3(kT), 0, st, a, words);
    if ((e = mark(4)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_vt_rank, dim3(blocks(a.n_cap)), dim3(kT), 0, st, a);
    if ((e = mark(5)) != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t launch_voxel_weights(const uint32_t* vox_counts, const uint32_t* index,
                                const uint32_t* total, uint32_t n_cap, uint32_t* weights,
                                hipStream_t st) {
    if (n_cap == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vt_weights, dim3(blocks(n_cap)), dim3(kT), 0, st, vox_counts, index, total,
                       n_cap, weights);
    return hipGetLastError();
}

}  // namespace gdf
