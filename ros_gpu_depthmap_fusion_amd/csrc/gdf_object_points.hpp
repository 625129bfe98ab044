// gdf_object_points.hpp — launch interface of the object-points stage (gdf_object_points.hip; the
// segmenter's entry points of include/gdf_segment.h call it).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdf.h"
#include "gdf_scan.hpp"

namespace gdf {

constexpr uint32_t kOpTile = 2048;            // items per partition tile (256 threads x 8 rounds)
constexpr uint32_t kOpMaxObjects = 1u << 24;  // nobj cap: three 8-bit passes
constexpr uint32_t kOpNone = 0xFFFFFFFFu;     // GDF_OBJ_NONE
constexpr uint32_t kOpLdsLayers = 8192;       // up to here the lstart table goes through LDS

inline uint32_t op_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + kOpTile - 1) / kOpTile); }
// words of the digit table of an n_cap-item call (256 digits per tile, digit-major) + the total
inline size_t op_hist_words(uint32_t n_cap) { return (size_t)256 * op_tiles(n_cap) + 1; }
inline size_t op_scan_words(size_t m) { return scan_words(m); }
// 8-bit passes that order ids below nobj: 1 up to 256 objects, 2 up to 65 536, 3 up to 2^24
inline uint32_t op_passes(uint32_t nobj) { return nobj <= 256u ? 1u : nobj <= 65536u ? 2u : 3u; }

// step 1: ids[i] for i < n = n_dev ? min(*n_dev, n_cap) : n_cap
struct ObjIdArgs {
    const uint32_t* cells;
    const uint32_t* n_dev;
    uint32_t n_cap;
    const uint16_t* labels;   // [L][H][W]
    const uint32_t* lstart;   // [L]
    const uint32_t* merged;   // [T]
    uint32_t T;
    uint32_t WH, L;
    uint64_t ncells;          // W * H * L
    uint32_t* ids;            // [n_cap]
};
hipError_t launch_object_ids(const ObjIdArgs& a, hipStream_t st);

// steps 2 and 3: voxels[nobj] (ZERO on entry) and keep[nobj]
struct ObjSizeArgs {
    const int32_t* stats5;    // [T][5]
    const uint32_t* merged;   // [T]
    const uint32_t* lstart;   // [L], strictly increasing (every layer has its background label)
    uint32_t L, T, nobj, min_voxels;
    uint32_t* voxels;
    uint8_t* keep;
};
hipError_t launch_object_sizes(const ObjSizeArgs& a, hipStream_t st);

// step 4: the points i < n with ids[i] < nobj and (keep == nullptr or keep[ids[i]]), stably
// partitioned by id.  Every per-point buffer holds n_cap items (at least 1); nothing has to be zero
// on entry and nothing is left behind.
struct ObjGroupArgs {
    const float4* pts;
    const uint32_t* ids;
    const uint32_t* n_dev;
    uint32_t n_cap, nobj;
    const uint8_t* keep;
    uint2* pairs[2];          // [n_cap] (id, index) ping-pong
    uint32_t* hist;           // [op_hist_words(n_cap)]
    uint32_t* sums;           // [op_scan_words(op_hist_words(n_cap))]
    uint32_t* total;          // the kept count
    float4* out;              // [n_cap]
    uint32_t* index;          // [n_cap]
    uint32_t* obj_start;      // [nobj + 1]
};
// ev != nullptr: 2 * passes + 3 events recorded around the passes (tools/object_points_bench.py):
// ev[0], then one after each pass's (count + scan), each pass's scatter, the gather and the starts
hipError_t launch_object_group(const ObjGroupArgs& a, hipStream_t st, hipEvent_t* ev);

// The frame's compacted points for the segmenter's stage call, with the refusals of
// gdf_radius_filter(GDF_RF_POINTS); GDF_OK or the error code (last error set).  gdf_engine.cpp.
struct FramePoints {
    const float4* pts;
    const uint32_t* coords;
    const uint32_t* n_dev;
    uint32_t cap;
    uint32_t gs[3];
    hipStream_t stream;
    int device;
};

int engine_frame_points(::gdf_engine* e, FramePoints* out);

}  // namespace gdf
