// gdf_filter.hip — radius outlier filter for gfx950 (include/gdf_filter.h).
//
// The rule (binary32, no contraction): a point is kept iff it lies inside the box and at least
// min_neighbors other inside points j have d2 = (dx*dx + dy*dy) + dz*dz <= r2.  The kernels search
// through cells whose edge exceeds the radius by 2^-10 (radius_plan), so a point's neighbours all
// lie in the 3x3x3 cells around its own; the cells only select candidates - every candidate is
// decided by the rule's own arithmetic, and counting is order-free, so the result does not depend on
// the cells or on the order in which points arrive in them.
//
// One pipeline, instantiated per cell table (RadiusTable; kSparse below):
//
//   k_rf_assign   inside test, cell, rank in the cell (returning integer atomic add)
//   scan          exclusive scan of the cell counters (the pass that reads them last zeroes them)
//   k_rf_scatter  xyz + original index into cell order
//   k_rf_count    per cell-ordered point: its own cell, then the other candidates, exit at
//                 min_neighbors; the keep flag goes to the ORIGINAL index
//   k_rf_tile_count, scan, k_rf_compact   stable compaction of the flagged input points
//
// Dense: one cloud, a cell is its linear index in a grid over the box, and the x-neighbours of a
// cell are contiguous in cell order (27 cells are 9 runs).
//
// Sparse: the same rule per segment (per frame of a batch); the cells of all
// segments live in one open-addressing table of H slots (linear probing, load <= 0.5) keyed by
// seg << 30 | cz << 20 | cy << 10 | cx, so a lookup never leaves its segment and the cells are sized
// to the radius whatever the box and the segment count.  A cell is its slot; k_rf_assign inserts the
// key, k_rf_count finds the other <= 26 cells by key lookup, and k_rf_compact also writes out_start
// and resets the table.  Which slot a cell gets and the order of the points inside it vary from run
// to run; both only order the candidates of an order-free count.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "gdf_filter.hpp"

namespace gdf {
void set_last_error(const std::string& msg);

// the plan of both cell structures: the dense grid caps the product of the axes, the sparse table
// does not
int radius_plan(RadiusTable table, const gdf_radius_filter_params* p, RadiusPlan* out) {
    if (!p || !out) {
        set_last_error("radius filter: null parameters");
        return GDF_ERR_ARG;
    }
    const float r2 = p->radius * p->radius;
    bool ok = std::isfinite(p->radius) && p->radius > 0.0f && std::isfinite(r2) && r2 > 0.0f;
    for (int a = 0; a < 3 && ok; ++a)
        ok = std::isfinite(p->lower[a]) && std::isfinite(p->upper[a]) && p->lower[a] <= p->upper[a];
    if (!ok) {
        set_last_error("radius filter: lower / upper / radius must be finite, lower <= upper, "
                       "radius > 0 and radius^2 finite and > 0");
        return GDF_ERR_ARG;
    }
    RadiusPlan q{};
    q.r2 = r2;
    // below 2^-100 the squares of the distance arithmetic leave binary32's normal range and the
    // margin proof's relative error bounds with it: one cell (every pair is a candidate)
    const bool tiny = r2 < 0x1p-100f;
    const double step = (double)p->radius * (1.0 + 0x1p-10);
    double ext[3];
    for (int a = 0; a < 3; ++a) {
        ext[a] = (double)p->upper[a] - (double)p->lower[a];
        double c = std::floor(ext[a] / step);
        if (tiny || ext[a] > 0x1p100 || !(c >= 1.0)) c = 1.0;  // (p - lower would leave f32's range)
        q.cells[a] = (uint32_t)std::min<double>(c, (double)kRfMaxAxisCells);
    }
    while (table == RadiusTable::Dense &&
           (uint64_t)q.cells[0] * q.cells[1] * q.cells[2] > kRfMaxCells) {
        int m = 0;
        for (int a = 1; a < 3; ++a)
            if (q.cells[a] > q.cells[m]) m = a;
        q.cells[m] = (q.cells[m] + 1) / 2;  // (halving rounds up: never to 0, edge only grows)
    }
    for (int a = 0; a < 3; ++a) {
        q.edge[a] = ext[a] / q.cells[a];
        q.inv[a] = q.cells[a] > 1 ? (float)(1.0 / q.edge[a]) : 0.0f;
    }
    q.ncells = q.cells[0] * q.cells[1] * q.cells[2];  // (<= 2^30: it fits uncapped too)
    *out = q;
    return GDF_OK;
}

namespace {

constexpr int kT = 256;  // block size of every kernel here: 4 waves
static_assert(kT == kScanThreads, "block_excl_scan scans 256 threads");

__device__ __forceinline__ bool rf_inside(const RadiusArgs& a, float4 p) {
    return p.x >= a.lo[0] && p.x <= a.hi[0] && p.y >= a.lo[1] && p.y <= a.hi[1] && p.z >= a.lo[2] &&
           p.z <= a.hi[2];
}

// a cell coordinate of an inside point
// monotone in p (p >= lo): f32 subtraction of a constant, multiplication by a positive constant,
// floor and the clamp are all monotone
__device__ __forceinline__ uint32_t rf_axis(float p, float lo, float inv, uint32_t cells) {
    if (cells <= 1u) return 0u;
    const float t = floorf(__fmul_rn(__fsub_rn(p, lo), inv));
    return (uint32_t)fminf(t, (float)(cells - 1u));
}

// The rule itself: the candidates [b, e) of the cell order against point p = `me` (m cell-ordered
// points in all); true once `need` neighbours are counted in *cnt.
__device__ __forceinline__ bool rf_candidates(const RadiusArgs& a, const float4& me, uint32_t p,
                                              uint32_t m, uint32_t b, uint32_t e, uint32_t need,
                                              uint32_t* cnt) {
    e = min(e, m);
    for (uint32_t j = b; j < e; ++j) {
        if (j == p) continue;
        const float4 q = a.sorted[j];
        const float dx = __fsub_rn(me.x, q.x), dy = __fsub_rn(me.y, q.y), dz = __fsub_rn(me.z, q.z);
        const float d2 =
            __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
        if (d2 <= a.r2 && ++*cnt >= need) return true;
    }
    return false;
}

// The segment table in LDS: sh[k] = max over j <= k of min(start[j], n_cap), k <= nseg (entries
// behind nseg repeat sh[nseg]).  Clamped and non-decreasing whatever the device table holds, so
// no content of it takes an access outside the per-point buffers.  sh: kRfMaxSegs + 1 words.
__device__ __forceinline__ void rfs_load_segs(const RadiusArgs& a, uint32_t* sh) {
    const uint32_t t = threadIdx.x;
    if (t < 64u) {  // wave 0
        uint32_t v = 0;
        if (a.seg_start) {
            if (t <= a.nseg) v = min(a.seg_start[t], a.n_cap);
        } else if (t >= 1u) {
            v = min(*a.n_dev, a.n_cap);
        }
        v = wave_incl_scan(v, [](uint32_t x, uint32_t y) { return max(x, y); });
        sh[t] = v;
        if (t == 63u) {
            uint32_t last = 0;
            if (a.seg_start && a.nseg == kRfMaxSegs) last = min(a.seg_start[kRfMaxSegs], a.n_cap);
            sh[kRfMaxSegs] = max(v, last);
        }
    }
    __syncthreads();
}

// the segment of point i, sh[0] <= i < sh[nseg]: the s with sh[s] <= i < sh[s + 1]
__device__ __forceinline__ uint32_t rfs_seg_of(const uint32_t* sh, uint32_t nseg, uint32_t i) {
    uint32_t lo = 0, hi = nseg;  // sh[lo] <= i < sh[hi]
    while (lo + 1u < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sh[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t rfs_hash(uint64_t key, uint32_t mask) {
    uint32_t h = (uint32_t)key * 0x9E3779B1u ^ (uint32_t)(key >> 32) * 0x85EBCA6Bu;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return h & mask;
}

// words of the segment table a kernel holds in LDS (the dense grid has none)
template <bool kSparse>
constexpr uint32_t kSegWords = kSparse ? kRfMaxSegs + 1 : 1;

// The points of the call: Dense n_dev / n_cap; Sparse the end of the last segment, with the segment
// table loaded into seg (every thread of the block calls it).
template <bool kSparse>
__device__ __forceinline__ uint32_t rf_points(const RadiusArgs& a, uint32_t* seg) {
    if constexpr (kSparse) {
        rfs_load_segs(a, seg);
        return seg[a.nseg];
    } else {
        return a.n_dev ? min(*a.n_dev, a.n_cap) : a.n_cap;
    }
}

// Per input point: inside test, its cell, its rank in the cell.  Dense: the cell is the linear index
// of its coordinates.  Sparse: the cell is the slot its key is inserted at.  A slot changes exactly once per call, from empty to its key, so a plain (possibly
// stale, cached) load can be wrong in one way only: it reads empty where a key already stands.
// That sends the lane to the CAS, and the CAS result is authoritative: it returns the key that
// stands there, or empty when this lane's key was written.  A load that reads a key reads the
// slot's final value.  The probe is bounded by H steps (never reached at load <= 0.5): a corrupted
// table ends the kernel instead of spinning, and the point is dropped.
template <bool kSparse>
__global__ __launch_bounds__(kT) void k_rf_assign(const RadiusArgs a) {
    __shared__ uint32_t seg[kSegWords<kSparse>];
    const uint32_t n = rf_points<kSparse>(a, seg);
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;  // (Sparse: behind the last segment: not read, no flag written)
    if constexpr (kSparse) {
        a.cell[i] = kRfNone;
        a.keep[i] = 0;
        if (i < seg[0]) return;  // before the first segment: in no segment
    }
    const float4 p = a.in[i];
    if (!rf_inside(a, p)) {
        if constexpr (!kSparse) {
            a.cell[i] = kRfNone;
            a.keep[i] = 0;
        }
        return;
    }
    const uint32_t cx = rf_axis(p.x, a.lo[0], a.inv[0], a.cells[0]);
    const uint32_t cy = rf_axis(p.y, a.lo[1], a.inv[1], a.cells[1]);
    const uint32_t cz = rf_axis(p.z, a.lo[2], a.inv[2], a.cells[2]);
    if constexpr (!kSparse) {
        const uint32_t c = cx + a.cells[0] * (cy + a.cells[1] * cz);
        a.cell[i] = c;
        a.rank[i] = atomicAdd(&a.cnt[c], 1u);
    } else {
        const uint64_t key = (uint64_t)rfs_seg_of(seg, a.nseg, i) << 30 | (uint64_t)cz << 20 |
                             (uint64_t)cy << 10 | cx;
        const uint32_t mask = a.nslots - 1u;
        uint32_t h = rfs_hash(key, mask);
        for (uint32_t step = 0; step < a.nslots; ++step) {
            uint64_t k = a.keys[h];
            if (k == kRfEmptyKey) {
                k = atomicCAS(reinterpret_cast<unsigned long long*>(a.keys + h),
                              (unsigned long long)kRfEmptyKey, (unsigned long long)key);
                if (k == kRfEmptyKey) k = key;  // this lane wrote it
            }
            if (k == key) {
                a.rank[i] = atomicAdd(&a.cnt[h], 1u);
                a.cell[i] = h;
                return;
            }
            h = (h + 1u) & mask;
        }
    }
}

template <bool kSparse>
__global__ __launch_bounds__(kT) void k_rf_scatter(const RadiusArgs a) {
    __shared__ uint32_t seg[kSegWords<kSparse>];
    const uint32_t n = rf_points<kSparse>(a, seg);
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = a.cell[i];
    if (kSparse ? c >= a.nslots : c == kRfNone) return;  // (kRfNone either way)
    const uint32_t pos = a.start[c] + a.rank[i];  // < start[M] <= n
    if (pos >= a.n_cap) return;                   // (only counters not zero on entry get here)
    const float4 p = a.in[i];
    a.sorted[pos] = make_float4(p.x, p.y, p.z, __uint_as_float(i));
    a.scell[pos] = c;
}

template <bool kSparse>
__global__ __launch_bounds__(kT) void k_rf_count(const RadiusArgs a) {
    const uint32_t m = min(a.start[kSparse ? a.nslots : a.ncells], a.n_cap);
    const uint32_t p = blockIdx.x * kT + threadIdx.x;
    if (p >= m) return;
    const float4 me = a.sorted[p];
    const uint32_t need = a.min_neighbors;
    uint32_t cnt = 0;
    // candidates [b, e) of the cell order; true once `need` neighbours are counted
    auto scan = [&](uint32_t b, uint32_t e) { return rf_candidates(a, me, p, m, b, e, need, &cnt); };
    if (need > 0u) {
        const uint32_t nx = a.cells[0], ny = a.cells[1], nz = a.cells[2];
        uint32_t c = a.scell[p], cx, cy, cz;
        [[maybe_unused]] uint32_t mask;
        [[maybe_unused]] uint64_t segbits;
        if constexpr (kSparse) {
            mask = a.nslots - 1u;
            c &= mask;
            const uint64_t key = a.keys[c];  // (the table is read-only here)
            cx = (uint32_t)key & 1023u, cy = (uint32_t)(key >> 10) & 1023u,
            cz = (uint32_t)(key >> 20) & 1023u;
            segbits = key >> 30 << 30;
        } else {
            const uint32_t t = c / nx;
            cx = c % nx, cy = t % ny, cz = t / ny;
        }
        const uint32_t x0 = cx > 0u ? cx - 1u : 0u, x1 = min(cx + 1u, nx - 1u);
        const uint32_t y0 = cy > 0u ? cy - 1u : 0u, y1 = min(cy + 1u, ny - 1u);
        const uint32_t z0 = cz > 0u ? cz - 1u : 0u, z1 = min(cz + 1u, nz - 1u);
        bool done = scan(a.start[c], a.start[c + 1u]);
        if constexpr (kSparse) {
            // the neighbour cells stay inside the plan (clamped per axis) and inside the segment (its
            // bits of the key are kept); a lookup ends at the key or at an empty slot, after H steps
            // at the latest.  (Loading the first probe of all 26 cells before looking at any was
            // measured: 169 VGPRs, 4-8 % off a sparse cloud's call, up to 37 % onto a dense batch's.)
            for (uint32_t z = z0; z <= z1 && !done; ++z)
                for (uint32_t y = y0; y <= y1 && !done; ++y)
                    for (uint32_t x = x0; x <= x1 && !done; ++x) {
                        if (x == cx && y == cy && z == cz) continue;
                        const uint64_t want = segbits | (uint64_t)z << 20 | (uint64_t)y << 10 | x;
                        uint32_t g = rfs_hash(want, mask);
                        for (uint32_t step = 0; step < a.nslots; ++step) {
                            const uint64_t k = a.keys[g];
                            if (k == want) {
                                done = scan(a.start[g], a.start[g + 1u]);
                                break;
                            }
                            if (k == kRfEmptyKey) break;
                            g = (g + 1u) & mask;
                        }
                    }
        } else {
            // the point's own cell first, then its two x-neighbours: where a cell is much wider than
            // the radius (the 2^22-cell cap) the neighbours that end the count early are found there
            if (!done && cx > 0u) done = scan(a.start[c - 1u], a.start[c]);
            if (!done && cx + 1u < nx) done = scan(a.start[c + 1u], a.start[c + 2u]);
            for (uint32_t z = z0; z <= z1 && !done; ++z)
                for (uint32_t y = y0; y <= y1 && !done; ++y) {
                    if (z == cz && y == cy) continue;
                    // the x-neighbours of a cell are contiguous in cell order: one run per (y, z)
                    const uint32_t row = nx * (y + ny * z);
                    done = scan(a.start[row + x0], a.start[row + x1 + 1u]);
                }
        }
    }
    const uint32_t orig = __float_as_uint(me.w);
    if (orig < a.n_cap) a.keep[orig] = cnt >= need ? 1 : 0;
}

// kept points of the 4 consecutive input points of this thread (tile of kRfTile per block), below n
__device__ __forceinline__ uint32_t rf_flags(const RadiusArgs& a, uint32_t n, uint64_t first) {
    uint32_t f = 0;
    if (first < n) {
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
            if ((uint32_t)first + k < n && a.keep[(uint32_t)first + k]) f |= 1u << k;
    }
    return f;
}

template <bool kSparse>
__global__ __launch_bounds__(kT) void k_rf_tile_count(const RadiusArgs a) {
    __shared__ uint32_t seg[kSegWords<kSparse>];
    __shared__ uint32_t sh[4];
    const uint32_t n = rf_points<kSparse>(a, seg);
    const uint32_t f = rf_flags(a, n, (uint64_t)blockIdx.x * kRfTile + threadIdx.x * 4u);
    uint32_t tot;
    block_excl_scan(__popc(f), &tot, sh);
    if (threadIdx.x == 0) a.tile_cnt[blockIdx.x] = tot;
}

// the flagged points of a thread to their places, o the first
__device__ __forceinline__ void rf_store(const RadiusArgs& a, uint32_t f, uint32_t first, uint32_t o) {
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        if (f >> k & 1u) {
            if (o < a.n_cap) a.out[o] = a.in[first + k];
            ++o;
        }
}

// The last kernel of the call.  Sparse: besides the compaction it writes out_start (each segment
// start by the block whose tile holds it) and empties the slots its points' cells took - every
// reader of the table has run - so the table is empty again at the next call.
template <bool kSparse>
__global__ __launch_bounds__(kT) void k_rf_compact(const RadiusArgs a, uint32_t ntiles) {
    __shared__ uint32_t seg[kSegWords<kSparse>];
    __shared__ uint32_t sh[4];
    const uint32_t n = rf_points<kSparse>(a, seg);
    const uint64_t tile0 = (uint64_t)blockIdx.x * kRfTile;
    const uint64_t first = tile0 + threadIdx.x * 4u;
    const uint32_t f = rf_flags(a, n, first);
    uint32_t tot;
    const uint32_t o = a.tile_off[blockIdx.x] + block_excl_scan(__popc(f), &tot, sh);
    if constexpr (kSparse) {
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
            if (first + k < n) {
                const uint32_t h = a.cell[(uint32_t)first + k];
                if (h < a.nslots) a.keys[h] = kRfEmptyKey;  // (the same value from every point of a cell)
            }
    }
    rf_store(a, f, (uint32_t)first, o);
    if constexpr (kSparse) {
        __shared__ uint32_t s_off[kT], s_flags[kT];
        s_off[threadIdx.x] = o;
        s_flags[threadIdx.x] = f;
        __syncthreads();
        if (threadIdx.x <= a.nseg) {
            const uint64_t b = seg[threadIdx.x];
            if (b >= tile0 && b < tile0 + kRfTile) {
                const uint32_t j = (uint32_t)(b - tile0) >> 2, r = (uint32_t)(b - tile0) & 3u;
                a.out_start[threadIdx.x] = s_off[j] + __popc(s_flags[j] & ((1u << r) - 1u));
            } else if (blockIdx.x == 0 && b >= (uint64_t)ntiles * kRfTile) {
                a.out_start[threadIdx.x] = a.tile_off[ntiles];  // (n_cap a multiple of the tile)
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.out_count = a.tile_off[ntiles];
}

template <bool kSparse>
hipError_t launch(const RadiusArgs& a, hipStream_t st) {
    const uint32_t pblocks = std::max<uint32_t>((a.n_cap + kT - 1) / kT, 1u);
    const uint32_t nt = std::max<uint32_t>(rf_tiles(a.n_cap), 1u);
    const uint32_t M = kSparse ? a.nslots : a.ncells;
    hipError_t e;
    hipLaunchKernelGGL(k_rf_assign<kSparse>, dim3(pblocks), dim3(kT), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_excl_scan(a.cnt, a.start, M, a.cell_sums, true, nullptr, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_rf_scatter<kSparse>, dim3(pblocks), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(k_rf_count<kSparse>, dim3(pblocks), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(k_rf_tile_count<kSparse>, dim3(nt), dim3(kT), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_excl_scan(a.tile_cnt, a.tile_off, nt, a.tile_sums, false, nullptr, st)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_rf_compact<kSparse>, dim3(nt), dim3(kT), 0, st, a, nt);
    return hipGetLastError();
}

int plan_out(RadiusTable table, const gdf_radius_filter_params* params, uint32_t cells[3],
             float edge[3]) {
    RadiusPlan q;
    const int rc = radius_plan(table, params, &q);
    if (rc != GDF_OK) return rc;
    for (int a = 0; a < 3; ++a) {
        if (cells) cells[a] = q.cells[a];
        if (edge) edge[a] = (float)q.edge[a];
    }
    return GDF_OK;
}

}  // namespace

hipError_t launch_radius_filter(const RadiusArgs& a, hipStream_t st) {
    return a.table == RadiusTable::Sparse ? launch<true>(a, st) : launch<false>(a, st);
}

}  // namespace gdf

extern "C" int gdf_radius_filter_plan_sparse(const gdf_radius_filter_params* params,
                                             uint32_t cells[3], float edge[3]) {
    return gdf::plan_out(gdf::RadiusTable::Sparse, params, cells, edge);
}

extern "C" int gdf_radius_filter_plan(const gdf_radius_filter_params* params, uint32_t cells[3],
                                      float edge[3]) {
    return gdf::plan_out(gdf::RadiusTable::Dense, params, cells, edge);
}
