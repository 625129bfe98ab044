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

// ---- the segmented filter over a sparse (hashed) cell table ------------------------------------
constexpr uint32_t kRfMaxSegs = 64;                  // segments per call (6 bits of the cell key)
constexpr uint32_t kRfMaxSegPoints = 1u << 30;       // n_cap of a segmented call (the table has 2^31 slots at most)
constexpr uint64_t kRfEmptyKey = ~uint64_t(0);       // an empty slot of the table

// The per-axis rule of radius_plan with no cap on the product (cells sized to the radius whatever
// the box): the 3x3x3 proof needs cells <= 1024 per axis and edge >= radius (1 + 2^-10) only.
int radius_plan_sparse(const gdf_radius_filter_params* p, RadiusPlan* out);

// slots of the table for n_cap points: the power of two >= 2 max(n_cap, 512) (load <= 0.5)
inline uint32_t rf_table_slots(uint32_t n_cap) {
    uint32_t h = 1024;
    while (h < 2u * (n_cap > 512u ? n_cap : 512u)) h <<= 1;
    return h;
}

// One segmented call: segment s holds the points [start[s], start[s + 1]) of `in`, the starts read
// from seg_start (device, nseg + 1 words; clamped to n_cap and made non-decreasing on read), or -
// seg_start == nullptr, nseg == 1 - the one segment [0, min(*n_dev, n_cap)).  Every per-point buffer
// holds n_cap items (at least 1).  keys: nslots words, all kRfEmptyKey on entry and again when the
// launches have run; cnt: nslots + 1 words, zero on entry and again afterwards.
struct RadiusSegArgs {
    const float4* in;
    uint32_t n_cap;
    const uint32_t* seg_start;
    const uint32_t* n_dev;
    uint32_t nseg;
    float lo[3], hi[3], inv[3];
    uint32_t cells[3];
    float r2;
    uint32_t min_neighbors;
    uint32_t nslots;      // H, a power of two
    uint64_t* keys;       // [H] seg << 30 | cz << 20 | cy << 10 | cx of the cell a slot holds
    uint32_t* cnt;        // [H + 1] points per slot
    uint32_t* start;      // [H + 1] exclusive scan of cnt; [H] = inside points
    uint32_t* cell_sums;  // [rf_scan_words(H)]
    uint32_t* slot;       // [n_cap] slot of each input point's cell (kRfNone: outside)
    uint32_t* rank;       // [n_cap] arrival rank inside its cell
    float4* sorted;       // [n_cap] xyz + original index, in slot order
    uint32_t* sslot;      // [n_cap] slot per slot-ordered point
    uint8_t* keep;        // [n_cap] keep flag per input point (written below start[nseg] only)
    uint32_t* tile_cnt;   // [rf_tiles(n_cap) + 1]
    uint32_t* tile_off;   // [rf_tiles(n_cap) + 1]
    uint32_t* tile_sums;  // [rf_scan_words(rf_tiles(n_cap))]
    float4* out;          // [n_cap] the kept points of all segments back to back
    uint32_t* out_start;  // [nseg + 1] kept points before start[s]; [nseg] = the total
    uint32_t* out_count;  // the total
};
hipError_t launch_radius_filter_segments(const RadiusSegArgs& a, hipStream_t st);

}  // namespace gdf
