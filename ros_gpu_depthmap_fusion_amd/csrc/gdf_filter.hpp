// gdf_filter.hpp — the radius outlier filter's launch interface (gdf_filter.hip; the engine's entry
// points of include/gdf_filter.h call it).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdf_filter.h"

namespace gdf {

constexpr uint32_t kRfMaxAxisCells = 1024;     // cells per axis (the plan's margin proof needs <= 1024)
constexpr uint32_t kRfMaxCells = 1u << 22;     // cells in all
constexpr uint32_t kRfTile = 1024;             // items per scan / compaction tile (256 threads x 4)
constexpr uint32_t kRfNone = 0xFFFFFFFFu;      // cell id of a point outside the box

// The cell plan (host, pure).  inv[a] = RN(1 / edge[a]) for an axis with more than one cell, else 0:
// a point's cell coordinate is min(floor((p - lower) * inv), cells - 1).
struct RadiusPlan {
    uint32_t cells[3];
    double edge[3];
    float inv[3];
    uint32_t ncells;
    float r2;
};
// GDF_OK or GDF_ERR_ARG (with the last-error message set)
int radius_plan(const gdf_radius_filter_params* p, RadiusPlan* out);

inline uint32_t rf_tiles(uint32_t n) { return (n + kRfTile - 1) / kRfTile; }
// words of the scan workspace for an m-item scan (the tile sums)
inline size_t rf_scan_words(uint32_t m) { return (size_t)rf_tiles(m) + 1; }

// One filter call.  n = n_dev ? min(*n_dev, n_cap) : n_cap; every per-point buffer holds n_cap items
// (at least 1).  cnt: ncells + 1 words, ZERO on entry and zero again when the launches have run.
struct RadiusArgs {
    const float4* in;
    const uint32_t* n_dev;
    uint32_t n_cap;
    float lo[3], hi[3], inv[3];
    uint32_t cells[3];
    uint32_t ncells;
    float r2;
    uint32_t min_neighbors;
    uint32_t* cell;       // [n_cap] cell id per input point (kRfNone: outside)
    uint32_t* rank;       // [n_cap] arrival rank inside its cell
    uint32_t* cnt;        // [ncells + 1] per-cell counters
    uint32_t* start;      // [ncells + 1] exclusive scan of cnt; [ncells] = inside points
    uint32_t* cell_sums;  // [rf_scan_words(ncells)]
    float4* sorted;       // [n_cap] xyz + original index, in cell order
    uint32_t* scell;      // [n_cap] cell id per cell-ordered point
    uint8_t* keep;        // [n_cap] keep flag per input point
    uint32_t* tile_cnt;   // [rf_tiles(n_cap) + 1] kept points per tile of kRfTile input points
    uint32_t* tile_off;   // [rf_tiles(n_cap) + 1] their exclusive scan
    uint32_t* tile_sums;  // [rf_scan_words(rf_tiles(n_cap))]
    float4* out;          // [n_cap]
    uint32_t* out_count;
};
hipError_t launch_radius_filter(const RadiusArgs& a, hipStream_t st);

}  // namespace gdf
