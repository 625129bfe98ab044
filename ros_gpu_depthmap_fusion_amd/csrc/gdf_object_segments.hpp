// gdf_object_segments.hpp — launch interface of the segmented object layer
// (gdf_object_segments.hip; the segmenter's entry points of include/gdf_segment.h call it;
// DESIGN.md §15): the partition and the voxel table per segment of the rows, one segment per frame
// of a batch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdf.h"

namespace gdf {

constexpr uint32_t kOsMaxSegs = 64;  // segments per call (the radius filter's bound)

// The segment table of a call, read once: out[s] = min(max(seg_start[0..s]), n) for s <= nseg, with
// n = n_dev ? min(*n_dev, n_cap) : n_cap.  seg_start == nullptr: the one segment {0, n} (nseg == 1).
// out[nseg] is the end of the rows that the passes after it look at.
struct SegStartArgs {
    const uint32_t* seg_start;  // [nseg + 1] or nullptr
    const uint32_t* n_dev;
    uint32_t nseg, n_cap;
    uint32_t* out;              // [nseg + 1]
};
hipError_t launch_segment_starts(const SegStartArgs& a, hipStream_t st);

// keys[i] = s(i) * nobj + ids[i] for the rows i < starts[nseg] that lie in a segment, have an id
// below nobj and (keep == nullptr or keep[id]); kOpNone for the other rows below starts[nseg].
// starts: launch_segment_starts' table.  nseg * nobj <= kOpMaxObjects.
struct SegKeyArgs {
    const uint32_t* ids;
    const uint32_t* starts;
    uint32_t nseg, n_cap, nobj;
    const uint8_t* keep;
    uint32_t* keys;             // [n_cap]
};
hipError_t launch_segment_keys(const SegKeyArgs& a, hipStream_t st);

// seg_out[s] = grp_start[s * nobj] for s <= nseg
hipError_t launch_segment_group_starts(const uint32_t* grp_start, uint32_t nseg, uint32_t nobj,
                                       uint32_t* seg_out, hipStream_t st);

// comp[i] = s(i) * C + cells[i] for the rows of a segment with cells[i] < C; kVtNone for the other
// rows below starts[nseg].  nseg * C <= kVtMaxCells.
struct SegCellArgs {
    const uint32_t* cells;
    const uint32_t* starts;
    uint32_t nseg, n_cap, C;
    uint32_t* comp;             // [n_cap]
};
hipError_t launch_segment_cells(const SegCellArgs& a, hipStream_t st);

// After launch_voxel_table on comp with num_cells = nseg * C: vox_cells back to plain cells
// (composite - s * C) and vox_seg_start[s] = the voxels with a composite cell below s * C, read from
// the table's own bitmap ranks; vox_seg_start[nseg] = G.
struct SegTableFinishArgs {
    const uint32_t* bitmap;
    const uint32_t* word_rank;
    const uint32_t* G;
    uint32_t nseg, C, vox_cap;
    uint32_t* vox_cells;        // [vox_cap]
    uint32_t* vox_seg_start;    // [nseg + 1]
};
hipError_t launch_segment_table_finish(const SegTableFinishArgs& a, hipStream_t st);

// The addressed slot's batch for the segmenter's batch stage calls, next to FramePoints /
// FrameVoxels: the compacted points and coords of all frames with d_fstart, and the voxelized rows
// with d_fvox.  fstart / fvox are nullptr for a single frame (the one segment {0, *n_dev}).  The
// refusals of engine_frame_points other than the batch one; GDF_ERR_STATE for a batch without frame
// ranges.  gdf_engine.cpp.
struct BatchPoints {
    const float4* pts;
    const uint32_t* coords;
    const uint32_t* fstart;   // [nframes + 1] or nullptr
    const uint32_t* n_dev;
    uint32_t cap, nframes;
    uint32_t gs[3];
    hipStream_t stream;
    int device;
};
int engine_batch_points(::gdf_engine* e, BatchPoints* out);

struct BatchVoxels {
    const float4* vox;
    const uint32_t* fvox;     // [nframes + 1] or nullptr
    const uint32_t* n_dev;    // the kVoxCount device word
    uint32_t cap;             // rows d_vox holds
};
int engine_batch_voxels(::gdf_engine* e, BatchVoxels* out);

}  // namespace gdf
