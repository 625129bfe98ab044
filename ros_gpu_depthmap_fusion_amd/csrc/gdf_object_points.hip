// gdf_object_points.hip — object id per point and the points grouped by object, for gfx950
// (include/gdf_segment.h).
//
// The rule: id = merged[lstart[z] + labels[cell]] (GDF_OBJ_NONE for a cell outside the grid or a
// background cell); voxels[o] = the AREA sum of o's foreground labels; a point is kept iff its id
// is below nobj and keep[id]; the kept points are partitioned by id, stable in input order.
// Integer gathers, integer adds and a stable sort: the result is exact and order-free.
//
//   k_op_ids      one thread per point, the lstart table through LDS
//   k_op_sizes    one thread per label: atomicAdd of AREA into voxels[merged[k]]
//   k_op_keep     keep[o] = voxels[o] >= max(min_voxels, 1)
//   per 8-bit digit of the id, lowest first (an LSD radix sort of (id, index) pairs):
//     k_op_hist     per tile of kOpTile items, the items per digit -> hist[digit][tile]
//     scan          exclusive scan of hist: where each tile's items of each digit go
//     k_op_scatter  the pairs to their places, rank inside the tile from per-wave ballots
//   k_op_gather   out[j] = pts[index[j]], index[j]
//   k_op_starts   obj_start[o] = the first sorted pair with id >= o (binary search)
//
// Dropped points leave in the first pass (they take part in no count).  A tile is walked wave by
// wave: wave w owns items [512 w, 512 w + 512) of the tile, 64 at a time, so "earlier in the tile"
// is (wave, round, lane) order and the rank of an item among the tile's items of its digit is
//   (items of the digit in earlier waves) + (in earlier rounds of this wave) + (in lower lanes).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gdf_object_points.hpp"
#include "gdf_scan.hpp"

namespace gdf {
namespace {

constexpr int kT = 256;  // block size of every kernel here: 4 waves
constexpr uint32_t kWaves = kT / 64;
constexpr uint32_t kRounds = kOpTile / kT;  // 64-item rounds per wave and tile

__device__ __forceinline__ uint32_t op_n(const uint32_t* n_dev, uint32_t n_cap) {
    return n_dev ? min(*n_dev, n_cap) : n_cap;
}

__global__ __launch_bounds__(kT) void k_op_ids(const ObjIdArgs a, uint32_t lds_layers) {
    extern __shared__ uint32_t s_lstart[];
    for (uint32_t z = threadIdx.x; z < lds_layers; z += kT) s_lstart[z] = a.lstart[z];
    __syncthreads();
    const uint32_t n = op_n(a.n_dev, a.n_cap);
    const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = a.cells[i];
    uint32_t id = kOpNone;
    if ((uint64_t)c < a.ncells) {
        const uint32_t z = c / a.WH;  // < L
        const uint32_t lab = a.labels[c];
        if (lab != 0u) {
            const uint32_t k = (lds_layers ? s_lstart[z] : a.lstart[z]) + lab;
            if (k < a.T) id = a.merged[k];  // (always, for the labelling's own tables)
        }
    }
    a.ids[i] = id;
}

__global__ __launch_bounds__(kT) void k_op_sizes(const ObjSizeArgs a) {
    const uint32_t k = blockIdx.x * kT + threadIdx.x;
    if (k >= a.T) return;
    // the background labels are the lstart values: the layer of k is the last z with lstart[z] <= k
    uint32_t lo = 0, hi = a.L;
    while (lo + 1u < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.lstart[mid] <= k) lo = mid; else hi = mid;
    }
    if (a.lstart[lo] == k) return;
    const uint32_t o = a.merged[k];
    if (o < a.nobj) atomicAdd(&a.voxels[o], (uint32_t)a.stats5[5u * (size_t)k + 4u]);
}

__global__ __launch_bounds__(kT) void k_op_keep(const ObjSizeArgs a) {
    const uint32_t o = blockIdx.x * kT + threadIdx.x;
    if (o < a.nobj) a.keep[o] = a.voxels[o] >= max(a.min_voxels, 1u) ? 1 : 0;
}

// ---- the partition passes -----------------------------------------------------------------------
// Item i of a pass: the first pass reads ids (index = i) and drops what is not kept, a later pass
// reads the pairs the pass before wrote.  false: the item takes no part.
template <bool kFirst>
__device__ __forceinline__ bool op_load(const ObjGroupArgs& a, const uint2* src, uint32_t n,
                                        uint64_t i, uint32_t* key, uint32_t* idx) {
    *key = 0;
    *idx = 0;
    if (i >= n) return false;
    if (kFirst) {
        const uint32_t id = a.ids[i];
        *key = id;
        *idx = (uint32_t)i;
        if (id >= a.nobj) return false;  // GDF_OBJ_NONE too
        return !a.keep || a.keep[id] != 0;
    }
    const uint2 p = src[i];
    *key = p.x;
    *idx = p.y;
    return true;
}

template <bool kFirst>
__device__ __forceinline__ uint32_t op_pass_n(const ObjGroupArgs& a) {
    return kFirst ? op_n(a.n_dev, a.n_cap) : min(*a.total, a.n_cap);
}

// the lanes of the wave that take part and hold digit d (8 ballots); every lane calls it
__device__ __forceinline__ uint64_t op_match(uint32_t d, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < 8u; ++b) {
        const bool bit = (d >> b & 1u) != 0;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

__device__ __forceinline__ uint64_t op_item(uint32_t r) {
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    return (uint64_t)blockIdx.x * kOpTile + w * (kOpTile / kWaves) + r * 64u + lane;
}

template <bool kFirst>
__global__ __launch_bounds__(kT) void k_op_hist(const ObjGroupArgs a, const uint2* src, uint32_t shift) {
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t n = op_pass_n<kFirst>(a);
    const uint32_t lane = threadIdx.x & 63u;
    if ((uint64_t)blockIdx.x * kOpTile < n) {  // (block-uniform)
        for (uint32_t r = 0; r < kRounds; ++r) {
            uint32_t key, idx;
            const bool valid = op_load<kFirst>(a, src, n, op_item(r), &key, &idx);
            const uint32_t d = key >> shift & 255u;
            const uint64_t m = op_match(d, valid);
            if (valid && lane == (uint32_t)__ffsll((unsigned long long)m) - 1u)
                atomicAdd(&cnt[d], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    a.hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = cnt[threadIdx.x];
}

// hist holds its exclusive scan: hist[d][tile] = where this tile's first item of digit d goes
template <bool kFirst>
__global__ __launch_bounds__(kT) void k_op_scatter(const ObjGroupArgs a, const uint2* src, uint2* dst,
                                                    uint32_t shift) {
    __shared__ uint32_t cnt[kWaves][256];
    const uint32_t n = op_pass_n<kFirst>(a);
    if ((uint64_t)blockIdx.x * kOpTile >= n) return;  // (block-uniform: an empty tile)
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t k = 0; k < kWaves; ++k) cnt[k][threadIdx.x] = 0;
    __syncthreads();
    uint32_t key[kRounds], idx[kRounds];
    uint32_t vmask = 0;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const bool valid = op_load<kFirst>(a, src, n, op_item(r), &key[r], &idx[r]);
        if (valid) vmask |= 1u << r;
        const uint32_t d = key[r] >> shift & 255u;
        const uint64_t m = op_match(d, valid);
        if (valid && lane == (uint32_t)__ffsll((unsigned long long)m) - 1u)
            atomicAdd(&cnt[w][d], (uint32_t)__popcll(m));  // (only wave w touches cnt[w])
    }
    __syncthreads();
    {  // thread d: the wave counts of digit d become the waves' first places
        uint32_t base = a.hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x];
#pragma unroll
        for (uint32_t k = 0; k < kWaves; ++k) {
            const uint32_t c = cnt[k][threadIdx.x];
            cnt[k][threadIdx.x] = base;
            base += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const bool valid = (vmask >> r & 1u) != 0;
        const uint32_t d = key[r] >> shift & 255u;
        const uint64_t m = op_match(d, valid);
        const uint32_t leader = m ? (uint32_t)__ffsll((unsigned long long)m) - 1u : 0u;
        uint32_t first = 0;
        // the rounds of a wave reach cnt[w][d] in program order: round r's items before r + 1's
        if (valid && lane == leader) first = atomicAdd(&cnt[w][d], (uint32_t)__popcll(m));
        first = __shfl(first, (int)leader, 64);
        if (valid) {
            const uint32_t pos = first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (pos < a.n_cap) dst[pos] = make_uint2(key[r], idx[r]);
        }
    }
}

__global__ __launch_bounds__(kT) void k_op_gather(const ObjGroupArgs a, const uint2* fin) {
    const uint32_t m = min(*a.total, a.n_cap);
    const uint64_t j = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (j >= m) return;
    const uint32_t i = fin[j].y;
    if (i >= a.n_cap) return;
    a.out[j] = a.pts[i];
    a.index[j] = i;
}

// the sorted ids are non-decreasing: obj_start[o] = the number of kept points with id < o
__global__ __launch_bounds__(kT) void k_op_starts(const ObjGroupArgs a, const uint2* fin) {
    const uint32_t m = min(*a.total, a.n_cap);
    const uint32_t o = blockIdx.x * kT + threadIdx.x;
    if (o > a.nobj) return;
    uint32_t lo = 0, hi = m;  // fin[< lo].x < o <= fin[>= hi].x
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (fin[mid].x < o) lo = mid + 1u; else hi = mid;
    }
    a.obj_start[o] = lo;
}

}  // namespace

hipError_t launch_object_ids(const ObjIdArgs& a, hipStream_t st) {
    if (a.n_cap == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)a.n_cap + kT - 1) / kT);
    const uint32_t lds = a.L <= kOpLdsLayers ? a.L : 0u;
    hipLaunchKernelGGL(k_op_ids, dim3(blocks), dim3(kT), (size_t)lds * 4, st, a, lds);
    return hipGetLastError();
}

hipError_t launch_object_sizes(const ObjSizeArgs& a, hipStream_t st) {
    if (a.T) hipLaunchKernelGGL(k_op_sizes, dim3((a.T + kT - 1) / kT), dim3(kT), 0, st, a);
    if (a.nobj) hipLaunchKernelGGL(k_op_keep, dim3((a.nobj + kT - 1) / kT), dim3(kT), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_object_group(const ObjGroupArgs& a, hipStream_t st, hipEvent_t* ev) {
    const uint32_t nt = std::max(op_tiles(a.n_cap), 1u);
    const uint32_t m = 256u * nt;
    const uint32_t passes = op_passes(a.nobj);
    hipError_t e;
    int k = 0;
    if (ev && (e = hipEventRecord(ev[k++], st)) != hipSuccess) return e;
    const uint2* src = nullptr;
    for (uint32_t p = 0; p < passes; ++p) {
        uint2* dst = a.pairs[p & 1u];
        const uint32_t shift = 8u * p;
        if (p == 0)
            hipLaunchKernelGGL(k_op_hist<true>, dim3(nt), dim3(kT), 0, st, a, src, shift);
        else
            hipLaunchKernelGGL(k_op_hist<false>, dim3(nt), dim3(kT), 0, st, a, src, shift);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = launch_excl_scan(a.hist, a.hist, m, a.sums, false, a.total, st)) != hipSuccess) return e;
        if (ev && (e = hipEventRecord(ev[k++], st)) != hipSuccess) return e;
        if (p == 0)
            hipLaunchKernelGGL(k_op_scatter<true>, dim3(nt), dim3(kT), 0, st, a, src, dst, shift);
        else
            hipLaunchKernelGGL(k_op_scatter<false>, dim3(nt), dim3(kT), 0, st, a, src, dst, shift);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (ev && (e = hipEventRecord(ev[k++], st)) != hipSuccess) return e;
        src = dst;
    }
    const uint32_t pblocks = std::max((uint32_t)(((uint64_t)a.n_cap + kT - 1) / kT), 1u);
    hipLaunchKernelGGL(k_op_gather, dim3(pblocks), dim3(kT), 0, st, a, src);
    if (ev && (e = hipEventRecord(ev[k++], st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_op_starts, dim3(a.nobj / kT + 1u), dim3(kT), 0, st, a, src);
    if (ev && (e = hipEventRecord(ev[k++], st)) != hipSuccess) return e;
    return hipGetLastError();
}

}  // namespace gdf
