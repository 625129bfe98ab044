// gdf_object_segments.hip — the object layer per segment of the rows, for gfx950
// (include/gdf_segment.h): one segment per frame of a batch.
//
// The rules: a row i lies in segment s iff start'[s] <= i < start'[s + 1], with start' the given
// starts made non-decreasing and clamped to the row count.  The partition groups the kept rows by
// (segment, object id), the voxel table ranks the distinct (segment, cell) pairs.  Both are §12's
// and §14's passes on a composite word, so the results stay exact and order-free:
//
//   k_os_starts   one block, once per call: the clamped starts (at most 65 words); every later pass
//                 reads this table, and its last word is the row count of the §12 / §14 passes
//   k_os_keys     one thread per row: key = s * nobj + id (GDF_OBJ_NONE for a dropped row), the
//                 starts through LDS; §12's partition then runs on the keys with nseg * nobj groups
//   k_os_gstarts  seg_out_start[s] = grp_start[s * nobj]
//   k_os_cells    one thread per row: composite cell = s * C + c (GDF_VOX_NONE for an outside row);
//                 §14's table then runs on the composites with nseg * C cells, so equal cells on
//                 the two sides of a segment border are different words to its lane dedup
//   k_os_finish   vox_cells back to plain cells; vox_seg_start[s] = the rank of bit s * C
//
// The segment of a row: the last s with start'[s] <= i, by a binary search of the LDS copy.  A wave
// whose first and last row lie in one segment (almost every wave: a frame has thousands of rows)
// takes the segment of its first row, counted by one ballot over the starts.
#include <hip/hip_runtime.h>

#include "gdf_object_points.hpp"
#include "gdf_object_segments.hpp"
#include "gdf_voxel_table.hpp"

namespace gdf {
namespace {

constexpr int kT = 256;  // block size of every kernel here: 4 waves

__global__ __launch_bounds__(kT) void k_os_starts(const SegStartArgs a) {
    if (threadIdx.x != 0) return;
    const uint32_t n = a.n_dev ? min(*a.n_dev, a.n_cap) : a.n_cap;
    if (!a.seg_start) {  // (nseg == 1)
        a.out[0] = 0;
        a.out[1] = n;
        return;
    }
    uint32_t m = 0;
    for (uint32_t s = 0; s <= a.nseg; ++s) {  // (at most 65 words: a serial running maximum)
        m = max(m, a.seg_start[s]);
        a.out[s] = min(m, n);
    }
}

// the clamped starts to LDS; every thread of the block calls it
__device__ __forceinline__ void os_stage(uint32_t* s_st, const uint32_t* starts, uint32_t nseg) {
    if (threadIdx.x <= nseg) s_st[threadIdx.x] = starts[threadIdx.x];  // (nseg + 1 <= 65 < kT)
    __syncthreads();
}

// the last s < nseg with st[s] <= i, for st[0] <= i < st[nseg] (so nseg >= 1 and st[s + 1] > i)
__device__ __forceinline__ uint32_t os_search(const uint32_t* st, uint32_t nseg, uint32_t i) {
    uint32_t lo = 0, hi = nseg;  // st[lo] <= i < st[hi]
    while (lo + 1u < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (st[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// The segment of row i, or nseg for a row in no segment.  Every lane of the wave calls it (rows at
// and beyond st[nseg] included).  The shortcut: lane l holds start l, so one ballot counts the
// starts at or below the wave's first row i0 (they are a prefix: the starts do not decrease); when
// the start after them lies beyond the wave's last row, the whole wave is in that one segment.
__device__ __forceinline__ uint32_t os_segment(const uint32_t* st, uint32_t nseg, uint32_t i) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i0 = i - lane;
    const uint32_t c = (uint32_t)__popcll(__ballot(lane < nseg && st[lane] <= i0));  // (nseg <= 64)
    if (c != 0u && (uint64_t)i0 + 63u < st[c]) return c - 1u;  // (wave-uniform; c <= nseg)
    if (i < st[0] || i >= st[nseg]) return nseg;
    return os_search(st, nseg, i);
}

__global__ __launch_bounds__(kT) void k_os_keys(const SegKeyArgs a) {
    __shared__ uint32_t s_st[kOsMaxSegs + 1];
    os_stage(s_st, a.starts, a.nseg);
    const uint32_t n = min(s_st[a.nseg], a.n_cap);
    const uint64_t i64 = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if ((uint64_t)blockIdx.x * kT >= n) return;  // (block-uniform; below it i64 < 2^32)
    const uint32_t i = (uint32_t)i64;
    const uint32_t s = os_segment(s_st, a.nseg, i);
    if (i >= n) return;
    uint32_t key = kOpNone;
    if (s < a.nseg) {
        const uint32_t id = a.ids[i];
        if (id < a.nobj && (!a.keep || a.keep[id] != 0)) key = s * a.nobj + id;  // < nseg * nobj <= 2^24
    }
    a.keys[i] = key;
}

__global__ __launch_bounds__(kT) void k_os_gstarts(const uint32_t* grp_start, uint32_t nseg, uint32_t nobj,
                                                    uint32_t* seg_out) {
    if (threadIdx.x <= nseg) seg_out[threadIdx.x] = grp_start[(size_t)threadIdx.x * nobj];
}

__global__ __launch_bounds__(kT) void k_os_cells(const SegCellArgs a) {
    __shared__ uint32_t s_st[kOsMaxSegs + 1];
    os_stage(s_st, a.starts, a.nseg);
    const uint32_t n = min(s_st[a.nseg], a.n_cap);
    const uint64_t i64 = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if ((uint64_t)blockIdx.x * kT >= n) return;  // (block-uniform; below it i64 < 2^32)
    const uint32_t i = (uint32_t)i64;
    const uint32_t s = os_segment(s_st, a.nseg, i);
    if (i >= n) return;
    uint32_t comp = kVtNone;
    if (s < a.nseg) {
        const uint32_t c = a.cells[i];
        if (c < a.C) comp = s * a.C + c;  // < nseg * C <= 2^28
    }
    a.comp[i] = comp;
}

__global__ __launch_bounds__(kT) void k_os_finish(const SegTableFinishArgs a) {
    const uint32_t G = min(*a.G, a.vox_cap);
    const uint32_t g = blockIdx.x * kT + threadIdx.x;
    if (g < G) {
        const uint32_t comp = a.vox_cells[g];
        a.vox_cells[g] = comp - (comp / a.C) * a.C;
    }
    if (blockIdx.x == 0 && threadIdx.x <= a.nseg) {
        const uint32_t s = threadIdx.x;
        uint32_t r = G;
        if (s < a.nseg) {  // the set bits below bit s * C (s * C < nseg * C: a word of the bitmap)
            const uint32_t b = s * a.C;
            r = a.word_rank[b >> 5] + (uint32_t)__popc(a.bitmap[b >> 5] & ((1u << (b & 31u)) - 1u));
        }
        a.vox_seg_start[s] = min(r, G);
    }
}

inline uint32_t blocks(uint64_t n) { return (uint32_t)((n + kT - 1) / kT); }

}  // namespace

hipError_t launch_segment_starts(const SegStartArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_os_starts, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_segment_keys(const SegKeyArgs& a, hipStream_t st) {
    if (a.n_cap == 0) return hipSuccess;
    hipLaunchKernelGGL(k_os_keys, dim3(blocks(a.n_cap)), dim3(kT), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_segment_group_starts(const uint32_t* grp_start, uint32_t nseg, uint32_t nobj,
                                       uint32_t* seg_out, hipStream_t st) {
    hipLaunchKernelGGL(k_os_gstarts, dim3(1), dim3(kT), 0, st, grp_start, nseg, nobj, seg_out);
    return hipGetLastError();
}

hipError_t launch_segment_cells(const SegCellArgs& a, hipStream_t st) {
    if (a.n_cap == 0) return hipSuccess;
    hipLaunchKernelGGL(k_os_cells, dim3(blocks(a.n_cap)), dim3(kT), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_segment_table_finish(const SegTableFinishArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_os_finish, dim3(blocks(a.vox_cap > 0 ? a.vox_cap : 1u)), dim3(kT), 0, st, a);
    return hipGetLastError();
}

}  // namespace gdf
