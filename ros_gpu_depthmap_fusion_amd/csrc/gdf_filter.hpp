// gdf_filter.hpp — the radius outlier filter's launch interface (gdf_filter.hip; the engine's entry
// points of include/gdf_filter.h call it).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdf_filter.h"
#include "gdf_scan.hpp"

namespace gdf {

constexpr uint32_t kRfMaxAxisCells = 1024;     // cells per axis (the plan's margin proof needs <= 1024)
constexpr uint32_t kRfMaxCells = 1u << 22;     // cells in all (dense grid)
constexpr uint32_t kRfTile = 1024;             // items per compaction tile (256 threads x 4)
constexpr uint32_t kRfNone = 0xFFFFFFFFu;      // cell id of a point outside the box
constexpr uint32_t kRfMaxSegs = 64;            // segments per sparse call (6 bits of the cell key)
constexpr uint32_t kRfMaxSegPoints = 1u << 30; // n_cap of a sparse call (the table has 2^31 slots at most)
constexpr uint64_t kRfEmptyKey = ~uint64_t(0); // an empty slot of the table

// How the cells of a call are named and found: a dense grid over the box (one cloud, a cell is its
// linear index), or a sparse, hashed table (one cloud per segment, a cell is the slot of its key).
enum class RadiusTable { Dense, Sparse };

// The cell plan (host, pure).  inv[a] = RN(1 / edge[a]) for an axis with more than one cell, else 0:
// a point's cell coordinate is min(floor((p - lower) * inv), cells - 1).
struct RadiusPlan {
    uint32_t cells[3];
    double edge[3];
    float inv[3];
    uint32_t ncells;
    float r2;
};
// GDF_OK or GDF_ERR_ARG (with the last-error message set).  Dense caps the product of the axes at
// kRfMaxCells; Sparse is the same per-axis rule with no cap on the product (cells sized to the radius
// whatever the box): the 3x3x3 proof needs cells <= 1024 per axis and edge >= radius (1 + 2^-10) only.
int radius_plan(RadiusTable table, const gdf_radius_filter_params* p, RadiusPlan* out);

inline uint32_t rf_tiles(uint32_t n) { return (n + kRfTile - 1) / kRfTile; }
inline size_t rf_scan_words(uint32_t m) { return scan_words(m); }

// slots of the sparse table for n_cap points: the power of two >= 2 max(n_cap, 512) (load <= 0.5)
inline uint32_t rf_table_slots(uint32_t n_cap) {
    uint32_t h = 1024;
    while (h < 2u * (n_cap > 512u ? n_cap : 512u)) h <<= 1;
    return h;
}

// One filter call.  Every per-point buffer holds n_cap items (at least 1).  M = ncells (Dense) or
// nslots (Sparse) is the table's length; cnt: M + 1 words, ZERO on entry and zero again when the
// launches have run.
//   Dense:  n = n_dev ? min(*n_dev, n_cap) : n_cap points of `in`, one cloud.
//   Sparse: segment s holds the points [start[s], start[s + 1]) of `in`, the starts read from
//           seg_start (device, nseg + 1 words; clamped to n_cap and made non-decreasing on read), or -
//           seg_start == nullptr, nseg == 1 - the one segment [0, min(*n_dev, n_cap)).  keys: nslots
//           words, all kRfEmptyKey on entry and again when the launches have run.
struct RadiusArgs {
    RadiusTable table;
    const float4* in;
    const uint32_t* n_dev;
    uint32_t n_cap;
    float lo[3], hi[3], inv[3];
    uint32_t cells[3];
    float r2;
    uint32_t min_neighbors;
    uint32_t* cell;       // [n_cap] cell (index or slot) per input point (kRfNone: outside)
    uint32_t* rank;       // [n_cap] arrival rank inside its cell
    uint32_t* cnt;        // [M + 1] points per cell
    uint32_t* start;      // [M + 1] exclusive scan of cnt; [M] = inside points
    uint32_t* cell_sums;  // [rf_scan_words(M)]
    float4* sorted;       // [n_cap] xyz + original index, in cell order
    uint32_t* scell;      // [n_cap] cell per cell-ordered point
    uint8_t* keep;        // [n_cap] keep flag per input point (Sparse: written below start[nseg] only)
    uint32_t* tile_cnt;   // [rf_tiles(n_cap) + 1] kept points per tile of kRfTile input points
    uint32_t* tile_off;   // [rf_tiles(n_cap) + 1] their exclusive scan
    uint32_t* tile_sums;  // [rf_scan_words(rf_tiles(n_cap))]
    float4* out;          // [n_cap] the kept points (of all segments back to back)
    uint32_t* out_count;  // the total
    // Dense only
    uint32_t ncells;
    // Sparse only
    uint32_t nslots;      // H, a power of two
    uint64_t* keys;       // [H] seg << 30 | cz << 20 | cy << 10 | cx of the cell a slot holds
    const uint32_t* seg_start;
    uint32_t nseg;
    uint32_t* out_start;  // [nseg + 1] kept points before start[s]; [nseg] = the total
};
hipError_t launch_radius_filter(const RadiusArgs& a, hipStream_t st);

}  // namespace gdf
