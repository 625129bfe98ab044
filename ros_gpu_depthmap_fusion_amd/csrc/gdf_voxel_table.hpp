// gdf_voxel_table.hpp — launch interface of the voxel table (gdf_voxel_table.hip; the segmenter's
// entry points of include/gdf_segment.h call it).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdf.h"
#include "gdf_scan.hpp"

namespace gdf {

constexpr uint32_t kVtNone = 0xFFFFFFFFu;       // GDF_VOX_NONE
constexpr uint32_t kVtMaxCells = 1u << 28;      // num_cells cap: a bitmap of 32 MB
constexpr uint32_t kVtRowWords = 64;            // bitmap words per counted row (2048 cells)

inline uint32_t vt_words(uint32_t num_cells) { return (num_cells + 31u) / 32u; }
inline uint32_t vt_rows(uint32_t num_cells) {
    return (vt_words(num_cells) + kVtRowWords - 1u) / kVtRowWords;
}
// words of the scan workspace of a num_cells table
inline size_t vt_scan_words(uint32_t num_cells) { return scan_words(vt_rows(num_cells)); }

// The table of cells[i], i < n = n_dev ? min(*n_dev, n_cap) : n_cap (n_cap >= 1, 0 < num_cells <=
// kVtMaxCells).  Nothing has to be zero on entry: the call clears the bitmap itself, and the other
// buffers are written before they are read.
struct VoxTableArgs {
    const uint32_t* cells;
    const uint32_t* n_dev;
    const uint32_t* first_dev;  // nullptr, or a device word: rows below it are neither read nor written
    uint32_t n_cap, num_cells;
    uint32_t* bitmap;        // [vt_words(num_cells)]
    uint32_t* row_rank;      // [vt_rows(num_cells) + 1]: row sums, then their exclusive scan
    uint32_t* sums;          // [vt_scan_words(num_cells)]
    uint32_t* word_rank;     // [vt_words(num_cells)]
    uint32_t* G;             // the number of voxels
    const uint32_t* limit_dev;  // nullptr, or a device word:
    uint32_t* limited;       //   *limited = min(G, *limit_dev) (G without limit_dev)
    uint32_t vox_cap;        // min(n_cap, num_cells) >= G: a voxel has a row and a cell of its own
    uint32_t* vox_cells;     // [vox_cap]
    uint32_t* vox_counts;    // [vox_cap]
    uint32_t* point_voxel;   // [n_cap]
};
// ev != nullptr: 6 events around the passes: ev[0], then one after the clear, the mark, the row
// sums + scan, the expand and the rank
constexpr uint32_t kVtEvents = 6;
hipError_t launch_voxel_table(const VoxTableArgs& a, hipStream_t st, hipEvent_t* ev);

// weights[j] = vox_counts[index[j]] for j < min(*total, n_cap)
hipError_t launch_voxel_weights(const uint32_t* vox_counts, const uint32_t* index,
                                const uint32_t* total, uint32_t n_cap, uint32_t* weights,
                                hipStream_t st);

// The frame's voxelized rows for gdf_seg_object_voxels, next to engine_frame_points (which gives the
// coords and the refusals of the compacted side); GDF_ERR_STATE before the frame's voxelize.
// gdf_engine.cpp.
struct FrameVoxels {
    const float4* vox;
    const uint32_t* n_dev;   // the kVoxCount device word
    uint32_t cap;            // rows d_vox holds
};

int engine_frame_voxels(::gdf_engine* e, FrameVoxels* out);

}  // namespace gdf
