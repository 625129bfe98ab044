// gdf_object_moments.hpp — launch interface of the per-object moments of the grouped clouds
// (gdf_object_moments.hip; gdf_seg_object_moments of include/gdf_segment.h calls it).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdf_object_points.hpp"
#include "gdf_segment.h"

namespace gdf {

constexpr uint32_t kOmSubdiv = 256;      // GDF_OBJ_SUBDIV: fixed-point steps per cell
constexpr uint32_t kOmMaxGrid = 65536;   // cells per axis: q < 2^24
constexpr uint32_t kOmChunk = 512;       // rows one wave walks: the unit of the partial slots
constexpr uint32_t kOmFinishWidth = 64;  // partial slots one finish step reduces: one per lane
static_assert(kOpTile % kOmChunk == 0, "whole chunks per tile of the partition");

constexpr uint32_t om_chunks(uint32_t n) { return (uint32_t)(((uint64_t)n + kOmChunk - 1) / kOmChunk); }
// records (104 B each, kept as 26 planes of words) of the partial table of an n_cap-row call: per
// chunk one head and one tail slot
inline size_t om_partial_records(uint32_t n_cap) { return (size_t)2 * (om_chunks(n_cap) + 1); }
// (256 max gs - 1)^2 n_cap < 2^64: no sum of an n_cap-row call can wrap
inline bool om_sums_fit(const uint32_t gs[3], uint32_t n_cap) {
    uint32_t g = gs[0] > gs[1] ? gs[0] : gs[1];
    g = g > gs[2] ? g : gs[2];
    const unsigned __int128 m = (unsigned __int128)kOmSubdiv * g - 1;
    return (m * m * n_cap) >> 64 == 0;
}

// moments[o] for every o < nobj over the rows [obj_start[o], obj_start[o + 1]) of pts, n =
// min(*total, n_cap) rows in all (obj_start[nobj] == n).  Nothing has to be zero on entry: every
// partial slot that is read was written by the same call.
struct ObjMomentArgs {
    const float4* pts;          // [n_cap] grouped rows
    const uint32_t* obj_start;  // [nobj + 1], non-decreasing
    const uint32_t* total;      // device word
    uint32_t n_cap, nobj;
    float lower[3], cell[3];
    uint32_t gs[3];
    gdf_obj_moments* moments;   // [nobj]
    uint32_t* partial;          // [26 words][2 om_chunks(n_cap) slots], within om_partial_records(n_cap)
};
hipError_t launch_object_moments(const ObjMomentArgs& a, hipStream_t st);

}  // namespace gdf
