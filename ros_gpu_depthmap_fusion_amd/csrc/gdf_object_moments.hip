// gdf_object_moments.hip — per-object moments of the grouped clouds, for gfx950
// (include/gdf_segment.h).
//
// The rule: t[a] = (p[a] - lower[a]) / cell[a] in f32; a row is measured iff 0 <= t[a] <= gs[a] on
// every axis (NaN fails); q[a] = min((u32)(256 t[a]), 256 gs[a] - 1).  Per object the measured
// rows' count, the min and max of q, the sums of q[a] and of q[a] q[b]; the other rows only count
// as `outside`.  All sums are integers, so they are exact and order-free: any reduction shape
// gives the same bits.
//
// The rows are grouped, so object o owns the rows [obj_start[o], obj_start[o + 1]) and a chunk of
// kOmChunk rows holds a contiguous run of objects.
//
//   k_om_tiles   one wave per chunk (four chunks per block).  The wave walks its chunk 64 rows a
//                round and keeps one record per lane in registers while the round's rows all
//                belong to the object it is at (the common case: no search, no cross-lane work).
//                A round with a change of object finds each lane's object by a search in
//                obj_start that gallops from the object the wave is at, then runs one inclusive
//                scan over the lanes of equal object (26 words, 6 steps) for all the round's
//                objects at once: the lane of an object's last row ends with the object's rows of
//                the round and writes them, all such lanes at a time, so one object per row costs
//                one scan per 64 rows.  The round's last object goes on in the lanes' registers.
//                A piece that is its whole object goes to moments[o]; of the other pieces a chunk
//                has at most two: the end of an object that began before the chunk (head slot)
//                and the beginning of one that runs past its end (tail slot).
//   k_om_finish  one wave per object: an object without rows gets the empty record; one that
//                crosses a chunk edge gets the sum of its first chunk's tail slot and the head
//                slots of the other chunks it spans, kOmFinishWidth slots a step.
//
// No atomics, and nothing to zero: whether a piece is whole is decided from obj_start alone, in
// both kernels alike, so every slot k_om_finish reads was written by k_om_tiles in the same call.
#include <hip/hip_runtime.h>

#include <limits>

#include "gdf_kernels.hpp"
#include "gdf_object_moments.hpp"

namespace gdf {
namespace {

constexpr int kT = 256;  // block size of both kernels: 4 waves
constexpr uint32_t kWaves = kT / 64;
constexpr uint32_t kRounds = kOmChunk / 64;
static_assert(kWaves * kOmChunk == kOpTile, "a block of k_om_tiles walks one tile of the partition");

static_assert(sizeof(gdf_obj_moments) == 104, "the record of include/gdf_segment.h");

// one record in registers: 8 u32 and 9 u64
struct OmAcc {
    uint32_t count, outside, qmin[3], qmax[3];
    uint64_t sum[3], sum2[6];
};

__device__ __forceinline__ void om_clear(OmAcc& r) {
    r.count = r.outside = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.qmin[k] = 0xFFFFFFFFu;
        r.qmax[k] = 0;
        r.sum[k] = 0;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) r.sum2[k] = 0;
}

// the row's q; false: not measured
__device__ __forceinline__ bool om_measure(const ObjMomentArgs& a, const float4 p, uint32_t q[3]) {
    const float v[3] = {p.x, p.y, p.z};
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t = (v[k] - a.lower[k]) / a.cell[k];
        const bool in = 0.0f <= t && t <= (float)a.gs[k];
        // (t <= 65536: the product is exact and below 2^24 + 1)
        q[k] = in ? min((uint32_t)(t * (float)kOmSubdiv), kOmSubdiv * a.gs[k] - 1u) : 0u;
        ok = ok && in;
    }
    return ok;
}

__device__ __forceinline__ void om_add_row(OmAcc& r, bool measured, const uint32_t q[3]) {
    if (!measured) {
        ++r.outside;
        return;
    }
    ++r.count;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.qmin[k] = min(r.qmin[k], q[k]);
        r.qmax[k] = max(r.qmax[k], q[k]);
        r.sum[k] += q[k];
    }
    r.sum2[0] += (uint64_t)q[0] * q[0];
    r.sum2[1] += (uint64_t)q[0] * q[1];
    r.sum2[2] += (uint64_t)q[0] * q[2];
    r.sum2[3] += (uint64_t)q[1] * q[1];
    r.sum2[4] += (uint64_t)q[1] * q[2];
    r.sum2[5] += (uint64_t)q[2] * q[2];
}

__device__ __forceinline__ void om_store(gdf_obj_moments* dst, const OmAcc& r) {
    gdf_obj_moments m;
    m.count = r.count;
    m.outside = r.outside;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        m.qmin[k] = r.qmin[k];
        m.qmax[k] = r.qmax[k];
        m.sum[k] = r.sum[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) m.sum2[k] = r.sum2[k];
    *dst = m;
}

__device__ __forceinline__ uint64_t om_shfl_xor(uint64_t v, int mask) {
    const uint32_t lo = __shfl_xor((uint32_t)v, mask, 64);
    const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), mask, 64);
    return (uint64_t)hi << 32 | lo;
}

// every lane ends with the wave's record (all 64 lanes call it)
__device__ __forceinline__ void om_wave_reduce(OmAcc& r) {
#pragma unroll
    for (int mask = 32; mask > 0; mask >>= 1) {
        r.count += __shfl_xor(r.count, mask, 64);
        r.outside += __shfl_xor(r.outside, mask, 64);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r.qmin[k] = min(r.qmin[k], (uint32_t)__shfl_xor(r.qmin[k], mask, 64));
            r.qmax[k] = max(r.qmax[k], (uint32_t)__shfl_xor(r.qmax[k], mask, 64));
            r.sum[k] += om_shfl_xor(r.sum[k], mask);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) r.sum2[k] += om_shfl_xor(r.sum2[k], mask);
    }
}

// the object of row j < obj_start[nobj]: the last o with obj_start[o] <= j (in [0, nobj) whatever
// obj_start holds)
__device__ __forceinline__ uint32_t om_object_of(const uint32_t* os, uint32_t nobj, uint32_t j) {
    uint32_t lo = 0, hi = nobj;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (os[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

// a += b
__device__ __forceinline__ void om_combine(OmAcc& a, const OmAcc& b) {
    a.count += b.count;
    a.outside += b.outside;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.qmin[k] = min(a.qmin[k], b.qmin[k]);
        a.qmax[k] = max(a.qmax[k], b.qmax[k]);
        a.sum[k] += b.sum[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) a.sum2[k] += b.sum2[k];
}

__device__ __forceinline__ uint64_t om_shfl_up(uint64_t v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d, 64);
    const uint32_t hi = __shfl_up((uint32_t)(v >> 32), d, 64);
    return (uint64_t)hi << 32 | lo;
}

// the record of the lane d below (all 64 lanes call it)
__device__ __forceinline__ OmAcc om_shfl_up(const OmAcc& r, int d) {
    OmAcc u;
    u.count = __shfl_up(r.count, d, 64);
    u.outside = __shfl_up(r.outside, d, 64);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u.qmin[k] = __shfl_up(r.qmin[k], d, 64);
        u.qmax[k] = __shfl_up(r.qmax[k], d, 64);
        u.sum[k] = om_shfl_up(r.sum[k], d);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) u.sum2[k] = om_shfl_up(r.sum2[k], d);
    return u;
}

// The partial table holds a record as 26 words, word k of slot i at partial[k P + i] with P =
// 2 om_chunks(n_cap) slots (chunk c: head slot 2 c, tail slot 2 c + 1), so that the lanes of
// k_om_finish, one slot each, read neighbouring words.
__device__ __forceinline__ void om_store_slot(uint32_t* part, size_t P, size_t i, const OmAcc& r) {
    uint32_t* w = part + i;
    w[0 * P] = r.count;
    w[1 * P] = r.outside;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        w[(2 + k) * P] = r.qmin[k];
        w[(5 + k) * P] = r.qmax[k];
        w[(8 + 2 * k) * P] = (uint32_t)r.sum[k];
        w[(9 + 2 * k) * P] = (uint32_t)(r.sum[k] >> 32);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        w[(14 + 2 * k) * P] = (uint32_t)r.sum2[k];
        w[(15 + 2 * k) * P] = (uint32_t)(r.sum2[k] >> 32);
    }
}

__device__ __forceinline__ void om_load_slot(const uint32_t* part, size_t P, size_t i, OmAcc& r) {
    const uint32_t* w = part + i;
    r.count = w[0 * P];
    r.outside = w[1 * P];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.qmin[k] = w[(2 + k) * P];
        r.qmax[k] = w[(5 + k) * P];
        r.sum[k] = (uint64_t)w[(9 + 2 * k) * P] << 32 | w[(8 + 2 * k) * P];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) r.sum2[k] = (uint64_t)w[(15 + 2 * k) * P] << 32 | w[(14 + 2 * k) * P];
}

// the object of row j at or after `from` (obj_start[from] <= j): gallop, then bisect; in
// [from, nobj) whatever obj_start holds
__device__ __forceinline__ uint32_t om_object_from(const uint32_t* os, uint32_t nobj, uint32_t from,
                                                   uint32_t j) {
    uint32_t lo = from, hi, step = 1;
    for (;;) {
        hi = lo + step;
        if (hi >= nobj) {
            hi = nobj;
            break;
        }
        if (os[hi] > j) break;
        lo = hi;
        step <<= 1;
    }
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (os[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

// The rows of object o = [s, e) that chunk c = rows [cb, ce) holds: to moments[o] when they are all
// of o, else to the chunk's head slot (o began before the chunk) or tail slot (o runs past its end)
__device__ __forceinline__ void om_store_piece(const ObjMomentArgs& a, const OmAcc& r, uint32_t o,
                                               uint32_t s, uint32_t e, uint32_t c, uint32_t cb,
                                               uint32_t ce) {
    if (s >= cb && e <= ce)
        om_store(a.moments + o, r);
    else
        om_store_slot(a.partial, (size_t)2 * om_chunks(a.n_cap), 2 * (size_t)c + (s < cb ? 0u : 1u), r);
}

__global__ __launch_bounds__(kT) void k_om_tiles(const ObjMomentArgs a) {
    const uint32_t n = min(*a.total, a.n_cap);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t c64 = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (c64 * kOmChunk >= n) return;  // (wave-uniform: a chunk behind the rows)
    const uint32_t c = (uint32_t)c64, cb = c * kOmChunk;
    const uint32_t ce = (uint32_t)min((uint64_t)cb + kOmChunk, (uint64_t)n);
    // the object the wave is at, its rows [cur_s, cur_e), and whether `acc` holds rows of it (one
    // record per lane; all wave-uniform but acc)
    uint32_t cur = om_object_of(a.obj_start, a.nobj, cb);
    uint32_t cur_s = a.obj_start[cur], cur_e = a.obj_start[cur + 1];
    bool have = false;
    OmAcc acc;
    om_clear(acc);
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t base = cb + r * 64u;
        if (base >= ce) break;  // (wave-uniform)
        const uint32_t j = base + lane;
        const bool valid = j < ce;
        uint32_t q[3] = {0, 0, 0};
        bool measured = false;
        if (valid) measured = om_measure(a, a.pts[j], q);
        const uint32_t last = min(base + 64u, ce) - 1u;
        if (last < cur_e) {  // the whole round belongs to `cur`: no search, no cross-lane work
            if (valid) om_add_row(acc, measured, q);
            have = true;
            continue;
        }
        // A change of object inside the round.  What the wave carries of `cur`, in every lane:
        OmAcc carry = acc;
        bool carried = have;
        const uint32_t carry_o = cur, carry_s = cur_s, carry_e = cur_e;
        if (carried) om_wave_reduce(carry);
        // every lane's object and its rows
        uint32_t o = kOpNone, s = 0, e = 0;
        if (valid) {
            o = om_object_from(a.obj_start, a.nobj, cur, j);
            s = a.obj_start[o];
            e = a.obj_start[o + 1];
        }
        const int last_lane = (int)(last - base);
        const uint32_t o_first = __builtin_amdgcn_readfirstlane(__shfl(o, 0, 64));
        const uint32_t o_last = __builtin_amdgcn_readfirstlane(__shfl(o, last_lane, 64));
        if (carried && o_first != carry_o) {  // `cur` ended with the round before
            if (lane == 0) om_store_piece(a, carry, carry_o, carry_s, carry_e, c, cb, ce);
            carried = false;
        }
        // inclusive scan over the lanes of one object (they are neighbours): the lane of an
        // object's last row ends with the object's rows of this round, and writes them - a row
        // that is a whole object by itself without having met another lane
        OmAcc v;
        om_clear(v);
        if (valid) om_add_row(v, measured, q);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const OmAcc u = om_shfl_up(v, d);
            const uint32_t ou = __shfl_up(o, d, 64);
            if (lane >= (uint32_t)d && ou == o) om_combine(v, u);
        }
        if (valid && o != o_last && j + 1u == e) {
            if (carried && o == carry_o) om_combine(v, carry);
            om_store_piece(a, v, o, s, e, c, cb, ce);
        }
        // the round's last object goes on
        om_clear(acc);
        if (valid && o == o_last) om_add_row(acc, measured, q);
        cur = o_last;
        cur_s = __builtin_amdgcn_readfirstlane(__shfl(s, last_lane, 64));
        cur_e = __builtin_amdgcn_readfirstlane(__shfl(e, last_lane, 64));
        have = true;
    }
    if (have) {
        om_wave_reduce(acc);
        if (lane == 0) om_store_piece(a, acc, cur, cur_s, cur_e, c, cb, ce);
    }
}

__global__ __launch_bounds__(kT) void k_om_finish(const ObjMomentArgs a) {
    const uint32_t n = min(*a.total, a.n_cap);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t o64 = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (o64 >= a.nobj) return;  // (wave-uniform)
    const uint32_t o = (uint32_t)o64;
    const uint32_t s = a.obj_start[o], e = min(a.obj_start[o + 1], n);
    OmAcc acc;
    om_clear(acc);
    if (s >= e) {  // no rows
        if (lane == 0) om_store(a.moments + o, acc);
        return;
    }
    const uint32_t c0 = s / kOmChunk, c1 = (e - 1u) / kOmChunk;  // c1 < om_chunks(n_cap)
    if (c0 == c1) return;  // k_om_tiles wrote it
    const size_t P = (size_t)2 * om_chunks(a.n_cap);
    // the tail slot of the first chunk, then the head slots of the others: slots 2 c0 + 1, 2 c0 + 2,
    // 2 c0 + 4, ...; kOmFinishWidth of them a step
    // (a lane past the end loads the last slot again and drops it: loads without a branch, so
    // that those of four steps are in flight together - the steps are latency, not bytes)
#pragma unroll 4
    for (uint32_t step = c0; step <= c1; step += kOmFinishWidth) {
        const uint32_t c = min(step + lane, c1);
        OmAcc u;
        om_load_slot(a.partial, P, 2 * (size_t)c + (c == c0 ? 1u : 0u), u);
        if (step + lane > c1) om_clear(u);
        om_combine(acc, u);
    }
    om_wave_reduce(acc);
    if (lane == 0) om_store(a.moments + o, acc);
}

}  // namespace

hipError_t launch_object_moments(const ObjMomentArgs& a, hipStream_t st) {
    const uint32_t tiles = (om_chunks(a.n_cap) + kWaves - 1) / kWaves;
    if (tiles) hipLaunchKernelGGL(k_om_tiles, dim3(tiles), dim3(kT), 0, st, a);
    if (a.nobj) hipLaunchKernelGGL(k_om_finish, dim3((a.nobj + kWaves - 1) / kWaves), dim3(kT), 0, st, a);
    return hipGetLastError();
}

}  // namespace gdf

// ---- host: centroid, covariance and world bounds from the records (no GPU, no handle) -------------
extern "C" int gdf_obj_shapes_from_moments(const gdf_obj_moments* m, uint32_t nobj, const float lower[3],
                                           const float cell[3], gdf_obj_shape* out) {
    if (!lower || !cell || (nobj && (!m || !out))) {
        gdf::set_last_error("object shapes: null argument");
        return GDF_ERR_ARG;
    }
    static const int A[6] = {0, 0, 0, 1, 1, 2}, B[6] = {0, 1, 2, 1, 2, 2};  // xx xy xz yy yz zz
    double c[3], l[3];
    for (int a = 0; a < 3; ++a) {
        c[a] = (double)cell[a] / 256.0;
        l[a] = (double)lower[a];
    }
    for (uint32_t o = 0; o < nobj; ++o) {
        const gdf_obj_moments& r = m[o];
        gdf_obj_shape& s = out[o];
        if (r.count == 0) {
            const double nan = std::numeric_limits<double>::quiet_NaN();
            for (int a = 0; a < 3; ++a) s.centroid[a] = s.min_world[a] = s.max_world[a] = nan;
            for (int k = 0; k < 6; ++k) s.cov[k] = nan;
            continue;
        }
        const double N = (double)r.count;
        for (int a = 0; a < 3; ++a) {
            s.centroid[a] = l[a] + c[a] * ((double)r.sum[a] / N + 0.5);
            s.min_world[a] = l[a] + c[a] * (double)r.qmin[a];
            s.max_world[a] = l[a] + c[a] * (double)((uint64_t)r.qmax[a] + 1u);
        }
        for (int k = 0; k < 6; ++k) {
            // exact in 128-bit integers, converted once (round to nearest even)
            const __int128 num = (__int128)((unsigned __int128)r.count * r.sum2[k]) -
                                 (__int128)((unsigned __int128)r.sum[A[k]] * r.sum[B[k]]);
            s.cov[k] = ((double)num / (N * N)) * c[A[k]] * c[B[k]];
        }
    }
    return GDF_OK;
}
