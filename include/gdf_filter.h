/*
 * gdf_filter.h — radius outlier filter on the fused cloud (C-ABI, part of libgdf.so).
 *
 * The component reads enable_radius_filter, radius_filter_radius, radius_filter_min_neighbors and
 * radius_filter_{min,max}_{x,y,z} (src/gpu_depthmap_fusion_component.cpp:1146,1179-1187) and its
 * per-frame sequence still names the call, radiusFilter(min, max, radius, minNeighbors) /
 * bypassRadiusFilter() right after voxelize (component.cpp:414-421); the reference engine no longer
 * implements it.  The rule below is therefore this library's specification.
 *
 *   inside     lower[a] <= p[a] && p[a] <= upper[a] on all three axes (NaN is outside); points
 *              outside are dropped and are nobody's neighbour
 *   distance   inside i != j: dx = xi - xj (dy, dz alike), d2 = (dx*dx + dy*dy) + dz*dz in binary32,
 *              that order, no contraction
 *   neighbour  d2 <= r2, r2 = radius * radius in binary32 (coincident points are neighbours of each
 *              other; a point is not its own neighbour)
 *   keep       inside and at least min_neighbors neighbours (0: every inside point)
 *   output     the kept points in input order, all four words bit for bit, and their count
 *
 * The result is defined by this rule alone: the cell grid the kernels search through never changes
 * a bit of it.  Everything is enqueued on the engine's current stream with no host wait.
 */
#ifndef GDF_FILTER_H_
#define GDF_FILTER_H_

#include "gdf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gdf_radius_filter_params {
    float lower[3], upper[3];
    float radius;
    uint32_t min_neighbors;
} gdf_radius_filter_params;

#define GDF_RF_POINTS 0    /* the frame's compacted points  (m_points)           */
#define GDF_RF_VOXELIZED 1 /* the frame's voxelized points  (m_points_voxelized) */

/* GDF_ERR_ARG unless lower, upper and radius are finite, lower[a] <= upper[a] (equal: a flat box),
 * radius > 0 and r2 is finite and > 0.  The cell plan of valid parameters (no engine, no GPU):
 * per axis cells = max(1, floor((upper - lower) / (radius (1 + 2^-10)))) in double, capped at 1024,
 * the largest axis halved until the product is <= 2^22; edge = (upper - lower) / cells.  (A radius
 * whose r2 is below 2^-100 plans one cell: squares that small leave binary32's normal range.) */
int gdf_radius_filter_plan(const gdf_radius_filter_params* params, uint32_t cells[3], float edge[3]);

/* The filter over n float4 points in device memory: the kept points to out_points_device
 * (capacity n), their count to out_count_device, and - keep_device != NULL - a u8 keep flag per
 * input point.  in and out must not alias (GDF_ERR_ARG); n = 0 is valid. */
int gdf_radius_filter_points(gdf_engine* engine, const float* in_points_device, uint32_t n,
                             const gdf_radius_filter_params* params, float* out_points_device,
                             uint32_t* out_count_device, uint8_t* keep_device);

/* Stage call on the addressed slot's results (the count stays on the device): source
 * GDF_RF_POINTS after the frame's compaction, GDF_RF_VOXELIZED after its voxelize.  GDF_ERR_STATE
 * before that stage, for a multi-frame batch and for a frame armed with the emit partition. */
int gdf_radius_filter(gdf_engine* engine, int source, const gdf_radius_filter_params* params);

/* Armed (sticky until disabled): a single frame's gdf_process_frame ends with the filter, on the
 * slot's stream, outside the frame's captured graph.  The source is the voxelized cloud when
 * enable_voxel_filter && !defer_voxelize, else the points (component.cpp:392-401).  A batch or a
 * deferred-voxelize frame processed while armed fails with GDF_ERR_STATE before any launch.
 * params may be NULL when enable == 0. */
int gdf_set_radius_filter(gdf_engine* engine, int enable, const gdf_radius_filter_params* params);

/* The filtered results of the addressed slot, valid until that slot's next gdf_clear;
 * GDF_ERR_STATE when no filter ran on its frame (m_points_filtered, component.cpp:494). */
int gdf_get_filtered_count(gdf_engine* engine, uint32_t* out);
int gdf_download_filtered_points(gdf_engine* engine, float* out_xyzw, uint32_t capacity,
                                 uint32_t* out_count);
int gdf_get_device_filtered(gdf_engine* engine, const float** points, const uint32_t** count_device);

/* ---- the filter per segment (per frame of a batch), over a sparse cell table -----------------
 *
 * For segments [start[s], start[s + 1]), s < nseg, of an array of float4 points the result for
 * segment s is exactly the rule above applied to that segment alone: a point of another segment
 * is nobody's neighbour.  The output is the kept points of all segments back to back, in segment
 * order and then input order, all four words bit for bit.  The cells live in a hashed table keyed
 * by segment and cell, sized by the points; it never changes a bit of the result.
 *
 * The sparse cell plan: the per-axis rule and the guards of gdf_radius_filter_plan (cells =
 * max(1, floor((upper - lower) / (radius (1 + 2^-10)))) capped at 1024, one cell in all for
 * r2 < 2^-100, one cell on an axis longer than 2^100) with no cap on the product.  The argument
 * checks are the same. */
int gdf_radius_filter_plan_sparse(const gdf_radius_filter_params* params, uint32_t cells[3],
                                  float edge[3]);

/* The segmented filter over device memory.  seg_start_device holds nseg + 1 u32 words, 1 <= nseg
 * <= 64; the starts are clamped to n_cap and made non-decreasing on read, and the table and the
 * points must not change while the call is in flight.  Kept points go to out_points_device
 * (capacity n_cap), out_seg_start_device[s] (nseg + 1 words) is the number of kept points before
 * start[s] - [0] = 0, [nseg] = the total, which also goes to out_count_device.  keep_device !=
 * NULL: a u8 keep flag per input point i < start[nseg]; bytes behind that are left untouched and
 * the points there are not read.  GDF_ERR_ARG for nseg outside 1..64, in == out, n_cap above 2^30
 * and bad params; n_cap = 0 is valid. */
int gdf_radius_filter_segments(gdf_engine* engine, const float* in_points_device, uint32_t n_cap,
                               const uint32_t* seg_start_device, uint32_t nseg,
                               const gdf_radius_filter_params* params, float* out_points_device,
                               uint32_t* out_seg_start_device, uint32_t* out_count_device,
                               uint8_t* keep_device);

/* Stage call on the addressed slot's frame or batch, one segment per frame: GDF_RF_POINTS takes the
 * device point ranges of the batch, GDF_RF_VOXELIZED its voxel ranges; a single frame is the one
 * segment {0, count}, the count read on the device.  GDF_ERR_STATE before that stage and for a
 * frame armed with the emit partition. */
int gdf_radius_filter_batch(gdf_engine* engine, int source, const gdf_radius_filter_params* params);

/* Armed (sticky until disabled), for multi-frame batches only: a batch's gdf_process_frame ends
 * with the segmented filter, on the slot's stream, outside the captured graph; the source is chosen
 * as gdf_set_radius_filter chooses it.  A deferred-voxelize batch processed while armed fails with
 * GDF_ERR_STATE before any launch.  Single frames stay governed by gdf_set_radius_filter alone, and
 * a batch processed with only that arm set still fails with GDF_ERR_STATE. */
int gdf_set_radius_filter_batch(gdf_engine* engine, int enable,
                                const gdf_radius_filter_params* params);

/* The ranges of the addressed slot's filtered result: filtered_start[f] is the first filtered point
 * of frame f, nframes + 1 entries ([nframes] = the count; {0, count} after a single-cloud filter).
 * filtered_start may be NULL to ask for out_frames alone.  gdf_get_filtered_count,
 * gdf_download_filtered_points and gdf_get_device_filtered serve the concatenated result. */
int gdf_get_filtered_ranges(gdf_engine* engine, uint32_t* filtered_start, uint32_t capacity,
                            uint32_t* out_frames);
/* ... the same table on the device (nseg + 1 words); GDF_ERR_STATE unless the slot's last filter
 * was a segmented one. */
int gdf_get_device_filtered_ranges(gdf_engine* engine, const uint32_t** start_device, uint32_t* nseg);

#ifdef __cplusplus
}
#endif

#endif /* GDF_FILTER_H_ */
