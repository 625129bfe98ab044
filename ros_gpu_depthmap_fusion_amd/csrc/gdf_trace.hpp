// gdf_trace.hpp — the diagnostic build's trace hooks (libgdf_trace.so, -DGDF_TRACE_GROUPS), and
// the only file that names that macro.  gdf_kernels.hip includes it once and wraps every hook in
// GDF_TRACE(...): the product build drops those tokens (no wait, no kernel argument, no anchor -
// its kernels are the ones the source shows), the trace build keeps them: the recorders below,
// their stamps and the 8-word records that tools/group_trace.py, gruns_trace.py, sel_trace.py and
// mask_trace.py read.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace gdf {

#ifdef GDF_TRACE_GROUPS

constexpr uint32_t kMaskTraceSlots = 1u << 14;  // per k_mask_px block
constexpr uint32_t kSelTraceSlots = 1u << 16;   // per k_sel tile
constexpr uint32_t kRunTraceSlots = 1u << 14;   // per k_group_runs tile
constexpr uint32_t kTraceSlots = 1u << 16;      // per queued group of k_group_runs_big
__device__ unsigned long long g_mtrace[kMaskTraceSlots][8];
__device__ unsigned long long g_strace[kSelTraceSlots][8];
__device__ unsigned long long g_rtrace[kRunTraceSlots][8];
__device__ unsigned long long g_gtrace[kTraceSlots][8];

// HW_ID (hwreg 4: wave, simd, pipe, cu, sh, se) bits 0..15 and XCC_ID (hwreg 20) bits 0..3
__device__ __forceinline__ unsigned long long trace_hw_id() {
    return (unsigned)__builtin_amdgcn_s_getreg(4 | (15 << 11)) & 0xFFFFu;
}
__device__ __forceinline__ unsigned long long trace_xcc_id() {
    return (unsigned)__builtin_amdgcn_s_getreg(20 | (15 << 11)) & 0xFu;
}

// (tools/mask_trace.py) per k_mask_px block: wall clock at entry and exit, then wave 0's cycles in
// each phase - segment geometry and camera, band loads landed, LDS stores + barrier, the filter,
// the ballots + publish barrier, the scan tail - each phase closed by a wait for this wave's
// outstanding memory operations (which the product kernel does not do)
struct MaskTrace {
    unsigned long long w0, t[7];
    __device__ __forceinline__ MaskTrace() : w0(wall_clock64()), t{} { stamp(0); }
    __device__ __forceinline__ void stamp(int i) {
        __builtin_amdgcn_s_waitcnt(0);
        t[i] = clock64();
    }
    // the stamp once two (uniform) fields of the camera are in registers
    __device__ __forceinline__ void stamp_after(int i, const void* p, uint32_t w) {
        asm volatile("" ::"s"(p), "s"(w));
        stamp(i);
    }
    __device__ __forceinline__ void store() {
        stamp(6);
        if (threadIdx.x == 0 && blockIdx.x < kMaskTraceSlots) {
            unsigned long long* g = g_mtrace[blockIdx.x];
            g[0] = w0;
            g[1] = wall_clock64();
            for (int k = 1; k < 7; ++k) g[k + 1] = t[k] - t[k - 1];
        }
    }
};

// (tools/sel_trace.py) per k_sel tile: the wall clock (100 MHz) at block entry, ticket, end of the
// counting pass (every wave past the barrier), end of the look-back, and block end; the hardware
// id of wave 0
struct SelTrace {
    unsigned long long w[4];
    __device__ __forceinline__ void stamp(int i) { w[i] = wall_clock64(); }
    __device__ __forceinline__ void store(uint32_t tile) {
        __syncthreads();
        if (threadIdx.x == 0 && tile < kSelTraceSlots) {
            unsigned long long* t = g_strace[tile];
            for (int k = 0; k < 4; ++k) t[k] = w[k];
            t[4] = wall_clock64();
            t[5] = trace_hw_id() | (trace_xcc_id() << 16);
            t[6] = blockIdx.x;
        }
    }
};

// (tools/gruns_trace.py) per k_group_runs tile: the wall clock (100 MHz) at block entry, tile
// start, after the run records and block scans, after the tile's offset / last-group end, after
// the staged sums, at the tile's end; the hardware id of wave 0, the block
struct RunsTrace {
    unsigned long long w[5];
    __device__ __forceinline__ void stamp(int i) { w[i] = wall_clock64(); }
    __device__ __forceinline__ void store(uint32_t tile) {
        if (threadIdx.x == 0 && tile < kRunTraceSlots) {
            unsigned long long* g = g_rtrace[tile];
            for (int k = 0; k < 5; ++k) g[k] = w[k];
            g[5] = wall_clock64();
            g[6] = trace_hw_id() | (trace_xcc_id() << 16);
            g[7] = blockIdx.x;
        }
    }
};

// (tools/group_trace.py) per queued group of k_group_runs_big: wall clock start / end, points,
// chunks, cycles in the sums / at the barriers / in the fetches, and the CU it ran on
struct GroupTrace {
    unsigned long long w0, c0, acc[5], b[6];
    // the queue's two regions, in the last slot
    __device__ __forceinline__ static void queue(uint32_t na, uint32_t nh, uint32_t cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            g_gtrace[kTraceSlots - 1][0] = 0;
            g_gtrace[kTraceSlots - 1][1] = na;
            g_gtrace[kTraceSlots - 1][2] = nh;
            g_gtrace[kTraceSlots - 1][3] = cap;
        }
    }
    __device__ __forceinline__ void begin() {
        for (int k = 0; k < 5; ++k) acc[k] = 0;
        w0 = wall_clock64();
        c0 = clock64();
    }
    // block_stream_sum, per chunk: clk(0..5) around the two barriers, the fetch and the sum
    __device__ __forceinline__ void clk(int i) { b[i] = clock64(); }
    __device__ __forceinline__ void chunk() {
        acc[0] += (b[1] - b[0]) + (b[3] - b[2]);  // barriers
        acc[1] += b[2] - b[1];                    // LDS stores (waits for the loads)
        acc[2] += b[4] - b[3];                    // fetch issue
        acc[3] += b[5] - b[4];                    // sum
        acc[4] += 1;
    }
    __device__ __forceinline__ void store_block(uint32_t t, uint32_t np) {
        if (threadIdx.x == 128 && t < kTraceSlots) {  // (wave 2: z)
            unsigned long long* g = g_gtrace[t];
            g[0] = w0;
            g[1] = wall_clock64();
            g[2] = ((unsigned long long)np << 32) | (unsigned)acc[4];
            g[3] = clock64() - c0;
            g[4] = acc[0];
            g[5] = acc[1];
            g[6] = acc[2];
            g[7] = acc[3] | (trace_hw_id() << 40) | (trace_xcc_id() << 56);
        }
    }
    __device__ __forceinline__ void store_wave(uint32_t t, uint32_t np) {
        if ((threadIdx.x & 63) == 0 && t < kTraceSlots) {
            unsigned long long* g = g_gtrace[t];
            g[0] = w0;
            g[1] = wall_clock64();
            g[2] = ((unsigned long long)np << 32) | ((np + 255u) / 256u);
            g[3] = clock64() - c0;
            g[4] = g[5] = g[6] = 0;
            g[7] = (trace_hw_id() << 40) | (trace_xcc_id() << 56);
        }
    }
};

template <class T, size_t N>
static int trace_read(void* dst, size_t bytes, const T (&sym)[N]) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(sym), std::min(bytes, sizeof(sym)), 0,
                                    hipMemcpyDeviceToHost);
}
template <class T, size_t N>
static int trace_clear(const T (&sym)[N]) {
    static T zero[N];
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(sym), zero, sizeof(zero), 0, hipMemcpyHostToDevice);
}
extern "C" int gdf_debug_group_trace(void* dst, size_t bytes) { return trace_read(dst, bytes, g_gtrace); }
extern "C" int gdf_debug_group_trace_clear() { return trace_clear(g_gtrace); }
extern "C" int gdf_debug_sel_trace(void* dst, size_t bytes) { return trace_read(dst, bytes, g_strace); }
extern "C" int gdf_debug_sel_trace_clear() { return trace_clear(g_strace); }
extern "C" int gdf_debug_runs_trace(void* dst, size_t bytes) { return trace_read(dst, bytes, g_rtrace); }
extern "C" int gdf_debug_runs_trace_clear() { return trace_clear(g_rtrace); }
extern "C" int gdf_debug_mask_trace(void* dst, size_t bytes) { return trace_read(dst, bytes, g_mtrace); }

#define GDF_TRACE(...) __VA_ARGS__

#else  // the product build: nothing

#define GDF_TRACE(...)

#endif

}  // namespace gdf
