// gdf_filter.hip — radius outlier filter for gfx950 (include/gdf_filter.h).
//
// The rule (binary32, no contraction): a point is kept iff it lies inside the box and at least
// min_neighbors other inside points j have d2 = (dx*dx + dy*dy) + dz*dz <= r2.  The kernels search
// through a dense cell grid whose edge exceeds the radius by 2^-10 (radius_plan), so a point's
// neighbours all lie in the 3x3x3 cells around its own; the grid only selects candidates - every
// candidate is decided by the rule's own arithmetic, and counting is order-free, so the result does
// not depend on the grid or on the order in which points arrive in their cells.
//
//   k_rf_cell     inside test, cell id, rank in the cell (returning integer atomic add)
//   scan          exclusive scan of the cell counters (the pass that reads them last zeroes them)
//   k_rf_scatter  xyz + original index into cell order
//   k_rf_count    per cell-ordered point: its own cell, then the other candidates as x-runs (27
//                 cells are 9 runs), exit at min_neighbors; the keep flag goes to the ORIGINAL index
//   k_rf_tile_count, scan, k_rf_compact   stable compaction of the flagged input points
//
// The second half of the file is the same rule per segment (per frame of a batch) over a sparse,
// hashed cell table (k_rfs_*): cells sized to the radius whatever the box and the segment count.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "gdf_filter.hpp"

namespace gdf {
void set_last_error(const std::string& msg);

namespace {
// the plan of both cell structures: the dense grid caps the product of the axes, the sparse table
// (cap_product false) does not
int plan_cells(const gdf_radius_filter_params* p, RadiusPlan* out, bool cap_product) {
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
    while (cap_product && (uint64_t)q.cells[0] * q.cells[1] * q.cells[2] > kRfMaxCells) {
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
}  // namespace

int radius_plan(const gdf_radius_filter_params* p, RadiusPlan* out) { return plan_cells(p, out, true); }
int radius_plan_sparse(const gdf_radius_filter_params* p, RadiusPlan* out) {
    return plan_cells(p, out, false);
}

namespace {

constexpr int kT = 256;  // block size of every kernel here: 4 waves

__device__ __forceinline__ uint32_t rf_n(const RadiusArgs& a) {
    return a.n_dev ? min(*a.n_dev, a.n_cap) : a.n_cap;
}

// monotone in p (p >= lo): f32 subtraction of a constant, multiplication by a positive constant,
// floor and the clamp are all monotone
__device__ __forceinline__ uint32_t rf_axis(float p, float lo, float inv, uint32_t cells) {
    if (cells <= 1u) return 0u;
    const float t = floorf(__fmul_rn(__fsub_rn(p, lo), inv));
    return (uint32_t)fminf(t, (float)(cells - 1u));
}

// exclusive scan of v over the block's 256 threads; *total = the block's sum.  sh: 4 words
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* total, uint32_t* sh) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += t;
    }
    if (lane == 63u) sh[w] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < kT / 64; ++k) {
        const uint32_t s = sh[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();  // (sh may be rewritten by the caller's next scan)
    *total = tot;
    return base + incl - v;
}

__global__ __launch_bounds__(kT) void k_rf_cell(const RadiusArgs a) {
    const uint32_t n = rf_n(a);
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const float4 p = a.in[i];
    const bool inside = p.x >= a.lo[0] && p.x <= a.hi[0] && p.y >= a.lo[1] && p.y <= a.hi[1] &&
                        p.z >= a.lo[2] && p.z <= a.hi[2];
    if (!inside) {
        a.cell[i] = kRfNone;
        a.keep[i] = 0;
        return;
    }
    const uint32_t cx = rf_axis(p.x, a.lo[0], a.inv[0], a.cells[0]);
    const uint32_t cy = rf_axis(p.y, a.lo[1], a.inv[1], a.cells[1]);
    const uint32_t cz = rf_axis(p.z, a.lo[2], a.inv[2], a.cells[2]);
    const uint32_t c = cx + a.cells[0] * (cy + a.cells[1] * cz);
    a.cell[i] = c;
    a.rank[i] = atomicAdd(&a.cnt[c], 1u);
}

__global__ __launch_bounds__(kT) void k_rf_scatter(const RadiusArgs a) {
    const uint32_t n = rf_n(a);
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = a.cell[i];
    if (c == kRfNone) return;
    const uint32_t pos = a.start[c] + a.rank[i];  // < start[ncells] <= n
    if (pos >= a.n_cap) return;                   // (only counters not zero on entry get here)
    const float4 p = a.in[i];
    a.sorted[pos] = make_float4(p.x, p.y, p.z, __uint_as_float(i));
    a.scell[pos] = c;
}

__global__ __launch_bounds__(kT) void k_rf_count(const RadiusArgs a) {
    const uint32_t m = min(a.start[a.ncells], a.n_cap);
    const uint32_t p = blockIdx.x * kT + threadIdx.x;
    if (p >= m) return;
    const float4 me = a.sorted[p];
    const uint32_t need = a.min_neighbors;
    uint32_t cnt = 0;
    if (need > 0u) {
        const uint32_t c = a.scell[p];
        const uint32_t nx = a.cells[0], ny = a.cells[1], nz = a.cells[2];
        const uint32_t cx = c % nx, t = c / nx, cy = t % ny, cz = t / ny;
        const uint32_t x0 = cx > 0u ? cx - 1u : 0u, x1 = min(cx + 1u, nx - 1u);
        const uint32_t y0 = cy > 0u ? cy - 1u : 0u, y1 = min(cy + 1u, ny - 1u);
        const uint32_t z0 = cz > 0u ? cz - 1u : 0u, z1 = min(cz + 1u, nz - 1u);
        // candidates [b, e) of the cell order; true once `need` neighbours are counted
        auto scan = [&](uint32_t b, uint32_t e) {
            e = min(e, m);
            for (uint32_t j = b; j < e; ++j) {
                if (j == p) continue;
                const float4 q = a.sorted[j];
                const float dx = __fsub_rn(me.x, q.x), dy = __fsub_rn(me.y, q.y),
                            dz = __fsub_rn(me.z, q.z);
                const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)),
                                           __fmul_rn(dz, dz));
                if (d2 <= a.r2 && ++cnt >= need) return true;
            }
            return false;
        };
        // the point's own cell first, then its two x-neighbours: where a cell is much wider than
        // the radius (the 2^22-cell cap) the neighbours that end the count early are found there
        bool done = scan(a.start[c], a.start[c + 1u]);
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
    const uint32_t orig = __float_as_uint(me.w);
    if (orig < a.n_cap) a.keep[orig] = cnt >= need ? 1 : 0;
}

// kept points of the 4 consecutive input points of this thread (tile of kRfTile per block)
__device__ __forceinline__ uint32_t rf_flags(const RadiusArgs& a, uint32_t n, uint32_t first) {
    uint32_t f = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        if (first + k < n && a.keep[first + k]) f |= 1u << k;
    return f;
}

__global__ __launch_bounds__(kT) void k_rf_tile_count(const RadiusArgs a) {
    __shared__ uint32_t sh[4];
    const uint32_t n = rf_n(a);
    const uint64_t first = (uint64_t)blockIdx.x * kRfTile + threadIdx.x * 4u;
    const uint32_t f = first < n ? rf_flags(a, n, (uint32_t)first) : 0u;
    uint32_t tot;
    block_excl_scan(__popc(f), &tot, sh);
    if (threadIdx.x == 0) a.tile_cnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kT) void k_rf_compact(const RadiusArgs a, uint32_t ntiles) {
    __shared__ uint32_t sh[4];
    const uint32_t n = rf_n(a);
    const uint64_t first = (uint64_t)blockIdx.x * kRfTile + threadIdx.x * 4u;
    const uint32_t f = first < n ? rf_flags(a, n, (uint32_t)first) : 0u;
    uint32_t tot;
    uint32_t o = a.tile_off[blockIdx.x] + block_excl_scan(__popc(f), &tot, sh);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        if (f >> k & 1u) {
            if (o < a.n_cap) a.out[o] = a.in[(uint32_t)first + k];
            ++o;
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.out_count = a.tile_off[ntiles];
}

// ---- exclusive scan of m u32 words: out[i] = sum of in[< i], out[m] = the total ---------------
// one block, any m (a carry between its chunks of kRfTile); in == out is allowed
__global__ __launch_bounds__(kT) void k_rf_scan_block(uint32_t* in, uint32_t* out, uint32_t m,
                                                       int zero_in) {
    __shared__ uint32_t sh[4];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < m; base += kRfTile) {
        const uint32_t first = base + threadIdx.x * 4u;
        uint32_t v[4], s = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            v[k] = first + k < m ? in[first + k] : 0u;
            s += v[k];
        }
        uint32_t tot;
        uint32_t o = carry + block_excl_scan(s, &tot, sh);  // (its barriers order reads before writes)
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
            if (first + k < m) {
                if (zero_in) in[first + k] = 0u;
                out[first + k] = o;
                o += v[k];
            }
        carry += tot;
    }
    if (threadIdx.x == 0) out[m] = carry;
}

__global__ __launch_bounds__(kT) void k_rf_scan_sums(const uint32_t* in, uint32_t m, uint32_t* sums) {
    __shared__ uint32_t sh[4];
    const uint32_t first = blockIdx.x * kRfTile + threadIdx.x * 4u;
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) s += first + k < m ? in[first + k] : 0u;
    uint32_t tot;
    block_excl_scan(s, &tot, sh);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// sums: the exclusive scan of the tile sums, sums[ntiles] = the total
__global__ __launch_bounds__(kT) void k_rf_scan_apply(uint32_t* in, const uint32_t* sums, uint32_t* out,
                                                       uint32_t m, uint32_t ntiles, int zero_in) {
    __shared__ uint32_t sh[4];
    const uint32_t first = blockIdx.x * kRfTile + threadIdx.x * 4u;
    uint32_t v[4], s = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        v[k] = first + k < m ? in[first + k] : 0u;
        s += v[k];
    }
    uint32_t tot;
    uint32_t o = sums[blockIdx.x] + block_excl_scan(s, &tot, sh);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        if (first + k < m) {
            if (zero_in) in[first + k] = 0u;
            out[first + k] = o;
            o += v[k];
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[m] = sums[ntiles];
}

constexpr uint32_t kScanOneBlock = 8 * kRfTile;  // up to here one block scans alone (one launch)

hipError_t rf_scan(uint32_t* in, uint32_t* out, uint32_t m, uint32_t* sums, int zero_in,
                   hipStream_t st) {
    if (m <= kScanOneBlock) {
        hipLaunchKernelGGL(k_rf_scan_block, dim3(1), dim3(kT), 0, st, in, out, m, zero_in);
        return hipGetLastError();
    }
    const uint32_t nt = rf_tiles(m);
    hipLaunchKernelGGL(k_rf_scan_sums, dim3(nt), dim3(kT), 0, st, in, m, sums);
    hipLaunchKernelGGL(k_rf_scan_block, dim3(1), dim3(kT), 0, st, sums, sums, nt, 0);
    hipLaunchKernelGGL(k_rf_scan_apply, dim3(nt), dim3(kT), 0, st, in, sums, out, m, nt, zero_in);
    return hipGetLastError();
}

// ==== the segmented filter over a sparse cell table ===========================
// The same rule per segment; the cells of all segments live in one open-addressing table of H
// slots (linear probing, load <= 0.5) keyed by seg << 30 | cz << 20 | cy << 10 | cx, so a lookup
// never leaves its segment and the cells are sized to the radius whatever the box.
//
//   k_rfs_insert   segment, inside test, cell key, its slot (insert), rank in the slot
//   scan           exclusive scan of the H slot counters (zeroes them)
//   k_rfs_scatter  xyz + original index into slot order
//   k_rfs_count    own cell, then the other <= 26 cells by key lookup; flag to the ORIGINAL index
//   k_rfs_tile_count, scan, k_rfs_compact   stable compaction, out_start, and the table's reset
//
// Which slot a cell gets and the order of the points inside it vary from run to run; both only
// order the candidates of an order-free count.

// The segment table in LDS: sh[k] = max over j <= k of min(start[j], n_cap), k <= nseg (entries
// behind nseg repeat sh[nseg]).  Clamped and non-decreasing whatever the device table holds, so
// no content of it takes an access outside the per-point buffers.  sh: kRfMaxSegs + 1 words.
__device__ __forceinline__ void rfs_load_segs(const RadiusSegArgs& a, uint32_t* sh) {
    const uint32_t t = threadIdx.x;
    if (t < 64u) {  // wave 0
        uint32_t v = 0;
        if (a.seg_start) {
            if (t <= a.nseg) v = min(a.seg_start[t], a.n_cap);
        } else if (t >= 1u) {
            v = min(*a.n_dev, a.n_cap);
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(v, d, 64);
            if (t >= (uint32_t)d) v = max(v, u);
        }
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

// Insert.  A slot changes exactly once per call, from empty to its key, so a plain (possibly
// stale, cached) load can be wrong in one way only: it reads empty where a key already stands.
// That sends the lane to the CAS, and the CAS result is authoritative: it returns the key that
// stands there, or empty when this lane's key was written.  A load that reads a key reads the
// slot's final value.  The probe is bounded by H steps (never reached at load <= 0.5): a corrupted
// table ends the kernel instead of spinning, and the point is dropped.
__global__ __launch_bounds__(kT) void k_rfs_insert(const RadiusSegArgs a) {
    __shared__ uint32_t seg[kRfMaxSegs + 1];
    rfs_load_segs(a, seg);
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= seg[a.nseg]) return;  // behind the last segment: not read, no flag written
    a.slot[i] = kRfNone;
    a.keep[i] = 0;
    if (i < seg[0]) return;        // before the first segment: in no segment
    const float4 p = a.in[i];
    const bool inside = p.x >= a.lo[0] && p.x <= a.hi[0] && p.y >= a.lo[1] && p.y <= a.hi[1] &&
                        p.z >= a.lo[2] && p.z <= a.hi[2];
    if (!inside) return;
    const uint64_t cx = rf_axis(p.x, a.lo[0], a.inv[0], a.cells[0]);
    const uint64_t cy = rf_axis(p.y, a.lo[1], a.inv[1], a.cells[1]);
    const uint64_t cz = rf_axis(p.z, a.lo[2], a.inv[2], a.cells[2]);
    const uint64_t key = (uint64_t)rfs_seg_of(seg, a.nseg, i) << 30 | cz << 20 | cy << 10 | cx;
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
            a.slot[i] = h;
            return;
        }
        h = (h + 1u) & mask;
    }
}

__global__ __launch_bounds__(kT) void k_rfs_scatter(const RadiusSegArgs a) {
    __shared__ uint32_t seg[kRfMaxSegs + 1];
    rfs_load_segs(a, seg);
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= seg[a.nseg]) return;
    const uint32_t h = a.slot[i];
    if (h >= a.nslots) return;                    // kRfNone
    const uint32_t pos = a.start[h] + a.rank[i];  // < start[H] <= n
    if (pos >= a.n_cap) return;                   // (only counters not zero on entry get here)
    const float4 p = a.in[i];
    a.sorted[pos] = make_float4(p.x, p.y, p.z, __uint_as_float(i));
    a.sslot[pos] = h;
}

__global__ __launch_bounds__(kT) void k_rfs_count(const RadiusSegArgs a) {
    const uint32_t m = min(a.start[a.nslots], a.n_cap);
    const uint32_t p = blockIdx.x * kT + threadIdx.x;
    if (p >= m) return;
    const float4 me = a.sorted[p];
    const uint32_t need = a.min_neighbors;
    uint32_t cnt = 0;
    if (need > 0u) {
        const uint32_t mask = a.nslots - 1u;
        const uint32_t h = a.sslot[p] & mask;
        const uint64_t key = a.keys[h];  // (the table is read-only here)
        const uint32_t cx = (uint32_t)key & 1023u, cy = (uint32_t)(key >> 10) & 1023u,
                       cz = (uint32_t)(key >> 20) & 1023u;
        const uint64_t segbits = key >> 30 << 30;
        const uint32_t x0 = cx > 0u ? cx - 1u : 0u, x1 = min(cx + 1u, a.cells[0] - 1u);
        const uint32_t y0 = cy > 0u ? cy - 1u : 0u, y1 = min(cy + 1u, a.cells[1] - 1u);
        const uint32_t z0 = cz > 0u ? cz - 1u : 0u, z1 = min(cz + 1u, a.cells[2] - 1u);
        // candidates [b, e) of the slot order; true once `need` neighbours are counted
        auto scan = [&](uint32_t b, uint32_t e) {
            e = min(e, m);
            for (uint32_t j = b; j < e; ++j) {
                if (j == p) continue;
                const float4 q = a.sorted[j];
                const float dx = __fsub_rn(me.x, q.x), dy = __fsub_rn(me.y, q.y),
                            dz = __fsub_rn(me.z, q.z);
                const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)),
                                           __fmul_rn(dz, dz));
                if (d2 <= a.r2 && ++cnt >= need) return true;
            }
            return false;
        };
        bool done = scan(a.start[h], a.start[h + 1u]);
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
    }
    const uint32_t orig = __float_as_uint(me.w);
    if (orig < a.n_cap) a.keep[orig] = cnt >= need ? 1 : 0;
}

// kept points of the 4 consecutive input points of this thread, below n = start[nseg]
__device__ __forceinline__ uint32_t rfs_flags(const RadiusSegArgs& a, uint32_t n, uint32_t first) {
    uint32_t f = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        if (first + k < n && a.keep[first + k]) f |= 1u << k;
    return f;
}

__global__ __launch_bounds__(kT) void k_rfs_tile_count(const RadiusSegArgs a) {
    __shared__ uint32_t seg[kRfMaxSegs + 1];
    __shared__ uint32_t sh[4];
    rfs_load_segs(a, seg);
    const uint32_t n = seg[a.nseg];
    const uint64_t first = (uint64_t)blockIdx.x * kRfTile + threadIdx.x * 4u;
    const uint32_t f = first < n ? rfs_flags(a, n, (uint32_t)first) : 0u;
    uint32_t tot;
    block_excl_scan(__popc(f), &tot, sh);
    if (threadIdx.x == 0) a.tile_cnt[blockIdx.x] = tot;
}

// The last kernel of the call: besides the compaction it writes out_start (each segment start by
// the block whose tile holds it) and empties the slots its points' cells took - every reader of
// the table has run - so the table is empty again at the next call.
__global__ __launch_bounds__(kT) void k_rfs_compact(const RadiusSegArgs a, uint32_t ntiles) {
    __shared__ uint32_t seg[kRfMaxSegs + 1];
    __shared__ uint32_t sh[4];
    __shared__ uint32_t s_off[kT], s_flags[kT];
    rfs_load_segs(a, seg);
    const uint32_t n = seg[a.nseg];
    const uint64_t tile0 = (uint64_t)blockIdx.x * kRfTile;
    const uint64_t first = tile0 + threadIdx.x * 4u;
    const uint32_t f = first < n ? rfs_flags(a, n, (uint32_t)first) : 0u;
    uint32_t tot;
    uint32_t o = a.tile_off[blockIdx.x] + block_excl_scan(__popc(f), &tot, sh);
    s_off[threadIdx.x] = o;
    s_flags[threadIdx.x] = f;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        if (first + k < n) {
            const uint32_t h = a.slot[(uint32_t)first + k];
            if (h < a.nslots) a.keys[h] = kRfEmptyKey;  // (the same value from every point of a cell)
        }
        if (f >> k & 1u) {
            if (o < a.n_cap) a.out[o] = a.in[(uint32_t)first + k];
            ++o;
        }
    }
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
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.out_count = a.tile_off[ntiles];
}

}  // namespace

hipError_t launch_radius_filter_segments(const RadiusSegArgs& a, hipStream_t st) {
    const uint32_t pblocks = std::max<uint32_t>((a.n_cap + kT - 1) / kT, 1u);
    const uint32_t nt = std::max<uint32_t>(rf_tiles(a.n_cap), 1u);
    hipError_t e;
    hipLaunchKernelGGL(k_rfs_insert, dim3(pblocks), dim3(kT), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = rf_scan(a.cnt, a.start, a.nslots, a.cell_sums, 1, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_rfs_scatter, dim3(pblocks), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(k_rfs_count, dim3(pblocks), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(k_rfs_tile_count, dim3(nt), dim3(kT), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = rf_scan(a.tile_cnt, a.tile_off, nt, a.tile_sums, 0, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_rfs_compact, dim3(nt), dim3(kT), 0, st, a, nt);
    return hipGetLastError();
}

hipError_t launch_radius_filter(const RadiusArgs& a, hipStream_t st) {
    const uint32_t pblocks = std::max<uint32_t>((a.n_cap + kT - 1) / kT, 1u);
    const uint32_t nt = std::max<uint32_t>(rf_tiles(a.n_cap), 1u);
    hipError_t e;
    hipLaunchKernelGGL(k_rf_cell, dim3(pblocks), dim3(kT), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = rf_scan(a.cnt, a.start, a.ncells, a.cell_sums, 1, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_rf_scatter, dim3(pblocks), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(k_rf_count, dim3(pblocks), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(k_rf_tile_count, dim3(nt), dim3(kT), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = rf_scan(a.tile_cnt, a.tile_off, nt, a.tile_sums, 0, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_rf_compact, dim3(nt), dim3(kT), 0, st, a, nt);
    return hipGetLastError();
}

}  // namespace gdf

extern "C" int gdf_radius_filter_plan_sparse(const gdf_radius_filter_params* params,
                                             uint32_t cells[3], float edge[3]) {
    gdf::RadiusPlan q;
    const int rc = gdf::radius_plan_sparse(params, &q);
    if (rc != GDF_OK) return rc;
    for (int a = 0; a < 3; ++a) {
        if (cells) cells[a] = q.cells[a];
        if (edge) edge[a] = (float)q.edge[a];
    }
    return GDF_OK;
}

extern "C" int gdf_radius_filter_plan(const gdf_radius_filter_params* params, uint32_t cells[3],
                                      float edge[3]) {
    gdf::RadiusPlan q;
    const int rc = gdf::radius_plan(params, &q);
    if (rc != GDF_OK) return rc;
    for (int a = 0; a < 3; ++a) {
        if (cells) cells[a] = q.cells[a];
        if (edge) edge[a] = (float)q.edge[a];
    }
    return GDF_OK;
}
