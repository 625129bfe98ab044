/*
 * gdf_segment.h — C-ABI of the GPU object-segmentation front end.
 *
 * Replaces the first half of GPUDepthmapFusion::objectSegmentation
 * (src/gpu_depthmap_fusion.cpp:2552-2575): labelVoxels (:1872-2011, OpenCV on the CPU in the
 * reference), uploadVoxelLabels (:2013-2073), prepareLayersConnections (:2075-2151),
 * computeLayersConnections (:2200-2214, shader/layers_connections.glsl:96-122) and
 * downloadLayersConnections (:2215-2241), plus mergeLabelsAcrossLayers (:2243-2361, host).
 * createCCObjects (:2364-2550) without its OpenCV shapes, and objectTracking (:2727-2944), stay out
 * of scope; gdf_seg_create_objects gives the objects' aggregate fields.
 *
 * Input: a device u8 occupancy grid of `layers` z-layers of height x width cells, x fastest
 * (m_occupancyGrid; layer i is the cv::Mat_<uint8_t>(height, width) view m_occupancyLayers[i],
 * fusion.cpp:1824-1839); a cell is foreground when non-zero.  Outputs, all with the reference's
 * layouts (flat, layer after layer):
 *   labels            u16 [layers][height][width]        m_ccLabeledLayersData
 *   num_labels        u32 [layers] (background included)  m_ccNumLabelsPerLayer
 *   stats             i32 [total_labels][5]               m_ccStatsData {LEFT, TOP, WIDTH, HEIGHT, AREA}
 *   centroids         f64 [total_labels][2]               m_ccCentroidsData
 *   labels_to_contours i32 [total_labels]                 m_labelsToContoursPerLayer (-1: none)
 *   contours          per layer, findContours order       m_contoursPerLayer (points x, y)
 *   connections       u8 [sum numA*numB] + starts         m_ccLayersConnectionsData / ...DataStarts
 *   merged            u32 [total_labels]                  m_ccLabelsMerged
 * Label numbering follows OpenCV's default 8-connectivity labelling (components ranked by their
 * first 2x2 block in block-raster order), contours follow findContours(RETR_EXTERNAL,
 * CHAIN_APPROX_NONE) — see DESIGN.md §9 for the restated semantics (parity unpinned: OpenCV is
 * absent from the reference tree and from this image).
 */
#ifndef GDF_SEGMENT_H_
#define GDF_SEGMENT_H_

#include <stdint.h>

#include "gdf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gdf_segmenter gdf_segmenter;

typedef struct gdf_seg_counts {
    uint32_t width, height, layers;
    uint32_t total_labels;          /* sum of num_labels                    */
    uint32_t total_contours;        /* sum over layers of contours          */
    uint64_t total_contour_points;  /* points of all contours               */
    uint64_t connection_bytes;      /* sum over layer pairs of numA * numB  */
} gdf_seg_counts;

/* flags of gdf_seg_label_layers */
#define GDF_SEG_CONTOURS 1u     /* run findContours + labelsToContours (labelVoxels :1935-1952) */
#define GDF_SEG_CONNECTIONS 2u  /* build the layer connection matrices (:2075-2214)            */
#define GDF_SEG_ALL 3u

int gdf_seg_create(int device, gdf_segmenter** out);
int gdf_seg_destroy(gdf_segmenter* seg);
/* a caller-owned hipStream_t (NULL: the segmenter's own stream) */
int gdf_seg_set_stream(gdf_segmenter* seg, void* hip_stream);

/* objectSegmentation front end (fusion.cpp:2554-2567) on a device grid.  Synchronises the stream
 * once, after the per-layer label counts (they size the stats and the connection matrices, as
 * in the reference, fusion.cpp:2085-2093); the rest is enqueued. */
int gdf_seg_label_layers(gdf_segmenter* seg, const uint8_t* grid_device, uint32_t width,
                         uint32_t height, uint32_t layers, uint32_t flags);
/* the same on an engine's current u8 occupancy grid, on the engine's stream */
int gdf_seg_label_engine_grid(gdf_segmenter* seg, gdf_engine* engine, uint32_t flags);

int gdf_seg_get_counts(gdf_segmenter* seg, gdf_seg_counts* out);
/* downloads (synchronise); capacities in elements of the output type */
int gdf_seg_download_labels(gdf_segmenter* seg, uint16_t* out, uint64_t capacity);
int gdf_seg_download_num_labels(gdf_segmenter* seg, uint32_t* out, uint32_t capacity);
int gdf_seg_download_stats(gdf_segmenter* seg, int32_t* stats5, double* centroids2,
                           uint32_t capacity_labels);
int gdf_seg_download_connections(gdf_segmenter* seg, uint8_t* out, uint64_t capacity,
                                 uint64_t* starts, uint32_t starts_capacity);
/* contours in findContours order, layer after layer: contours_per_layer[layers],
 * sizes[total_contours] (points per contour), points_xy[2 * total_contour_points] */
int gdf_seg_download_contours(gdf_segmenter* seg, int32_t* labels_to_contours,
                              uint32_t* contours_per_layer, uint32_t* sizes, int32_t* points_xy,
                              uint64_t points_capacity);
/* mergeLabelsAcrossLayers (fusion.cpp:2243-2361): merged[label of layer i at
 * sum(num_labels[<i]) + label] and the number of merged objects (background objects included,
 * as in m_ccLabelsMergedGrouper); needs GDF_SEG_CONNECTIONS */
int gdf_seg_merge_labels(gdf_segmenter* seg, uint32_t* merged, uint32_t capacity,
                         uint32_t* num_objects);
/* createCCObjects (fusion.cpp:2364-2550) without the OpenCV shapes (minAreaRect /
 * minEnclosingCircle of the contours, SURVEY §8(f) rank 4, out of scope): one record per merged
 * object, in merged-label order (background objects included, as m_ccObjects), with the
 * reference's float/int arithmetic; `components` receives every object's global label indices in
 * grouped order (UIntGrouper: ascending index), object i's at [first_component,
 * first_component + num_components).  lower / cell_size: the grid's GridMeta lower bound and
 * cell size (voxelCoordToWorldCoord, fusion.cpp:1720-1730).  Needs gdf_seg_merge_labels' inputs
 * (GDF_SEG_CONNECTIONS) and GDF_SEG_CONTOURS for the contour point counts. */
typedef struct gdf_cc_object {
    uint32_t label, num_components, num_layers, first_component;
    float centroid[2];                        /* mean of the components' centroids (cv::Point2f) */
    int32_t min_voxel[3], max_voxel[3], aabb_voxel[3];
    float center_voxel[3], center_world[3], min_world[3], max_world[3], aabb_world[3];
    uint32_t num_contour_points;              /* points of the components' external contours */
} gdf_cc_object;
int gdf_seg_create_objects(gdf_segmenter* seg, const float lower[3], const float cell_size[3],
                           gdf_cc_object* objects, uint32_t capacity, uint32_t* components,
                           uint32_t components_capacity, uint32_t* num_objects);
/* device pointers of the results (valid until the next gdf_seg_label_*) */
int gdf_seg_get_device_results(gdf_segmenter* seg, const uint16_t** labels, const int32_t** stats5,
                               const double** centroids2, const uint8_t** connections);

/* ---- object id per point and the points grouped by object ---------------------
 *
 * No reference counterpart; the rule is this library's specification.  With W, H, L the labelled
 * grid, lstart[z] = sum(num_labels[< z]), merged / nobj as gdf_seg_merge_labels gives them:
 *   id      c = cells[i] (x + y W + z W H, as computeVoxelCoords writes it); c >= W H L or
 *           labels[c] == 0 (a background cell): GDF_OBJ_NONE; else merged[lstart[c / (W H)] + labels[c]]
 *   voxels  voxels[o] = sum of stats[k][AREA] over the foreground labels k with merged[k] == o
 *           (a label is foreground unless k == lstart[z] for some z; a background object has 0)
 *   keep    keep[o] = voxels[o] >= max(min_voxels, 1); a point is kept iff id < nobj and keep[id]
 *   output  ids[n] in input order (independent of keep); the kept points partitioned by object,
 *           object o's at [obj_start[o], obj_start[o + 1]) in input order, all four words bit for
 *           bit; obj_start[0] = 0, obj_start[nobj] = the kept total (also a device count word);
 *           index[j] = the input index of output point j; voxels[nobj]
 * Integer gathers, integer adds and a stable partition: the result is exact.  Everything is
 * enqueued with no host wait, except that the first call after a labelling waits once for nobj
 * (as gdf_seg_merge_labels does) and that a workspace buffer that has to grow is reallocated
 * (the workspace is grow-only: a steady stream of frames stops growing).  The input count may be
 * a device word (count_device != NULL: n = min(*count_device, n_cap)); rows at and beyond n are
 * neither read nor written.  Results stay valid until the next gdf_seg_label_* or the next
 * gdf_seg_group_points / gdf_seg_object_points / gdf_seg_object_voxels (below).
 * Streams: the labelling and these calls may run on different streams (the segmenter's and an
 * engine's), in any order; a call whose stream differs from the previous call's waits on the
 * device for that call's work, so no host wait is needed between them. */
#define GDF_OBJ_NONE 0xFFFFFFFFu

/* ids alone, on any device arrays, on the segmenter's stream; needs a labelling with
 * GDF_SEG_CONNECTIONS (GDF_ERR_STATE) */
int gdf_seg_point_object_ids(gdf_segmenter* seg, const uint32_t* cells_device, uint32_t n_cap,
                             const uint32_t* count_device, uint32_t* ids_out_device);

/* the partition alone, on any (points, ids), on the segmenter's stream: keep_device u8[nobj] or
 * NULL (keep all); ids >= nobj are dropped.  Independent of the labelling.  GDF_ERR_ARG for null
 * pointers, nobj == 0 and nobj > 2^24; n_cap == 0 succeeds with empty results. */
int gdf_seg_group_points(gdf_segmenter* seg, const float* points_device, const uint32_t* ids_device,
                         uint32_t n_cap, const uint32_t* count_device, uint32_t nobj,
                         const uint8_t* keep_device);

/* The whole rule on the engine's compacted points, its voxel coords and its device-side count, on
 * the engine's stream.  GDF_ERR_STATE, before any launch: no labelling or one without
 * GDF_SEG_CONNECTIONS; W, H, L differ from the engine's grid size; and what
 * gdf_radius_filter(GDF_RF_POINTS) refuses on the engine's side (before the frame's compaction, a
 * multi-frame batch, a frame armed with the emit partition); an engine on another device than
 * the segmenter's.  GDF_ERR_ARG for nobj > 2^24. */
int gdf_seg_object_points(gdf_segmenter* seg, gdf_engine* engine, uint32_t min_voxels);

/* the object count and the kept total of the last call (waits) */
int gdf_seg_get_object_points(gdf_segmenter* seg, uint32_t* nobj, uint32_t* total);
/* the input count n of the last call, i.e. the length of ids (waits); it belongs to that call
 * and does not follow the engine's later frames */
int gdf_seg_get_object_points_input(gdf_segmenter* seg, uint32_t* n);
/* Downloads (wait); every pointer may be NULL.  ids: the n ids of gdf_seg_object_points; points_xyzw
 * and index: total rows; obj_start: nobj + 1 words; voxels: nobj words.  ids and voxels are
 * GDF_ERR_STATE after gdf_seg_group_points (it computes neither).  GDF_ERR_CAPACITY when a
 * capacity (in rows / words; obj_capacity >= nobj + 1) is too small. */
int gdf_seg_download_object_points(gdf_segmenter* seg, uint32_t* ids, uint32_t ids_capacity,
                                   float* points_xyzw, uint32_t* index, uint32_t points_capacity,
                                   uint32_t* obj_start, uint32_t* voxels, uint32_t obj_capacity);
/* the same on the device; ids and voxels are NULL after gdf_seg_group_points */
int gdf_seg_get_device_object_points(gdf_segmenter* seg, const uint32_t** ids, const float** points,
                                     const uint32_t** index, const uint32_t** obj_start,
                                     const uint32_t** voxels, const uint32_t** count_device);
/* Instrumentation: with enable != 0 the next group / object-points calls record events around
 * their passes; gdf_seg_get_object_points_times (waits) then gives the last call's times in
 * milliseconds: [ids + sizes (0 for gdf_seg_group_points)], per 8-bit pass [count + scan, scatter],
 * [gather], [starts]: 2 * passes + 3 values. */
int gdf_seg_set_profiling(gdf_segmenter* seg, int enable);
int gdf_seg_get_object_points_times(gdf_segmenter* seg, float* ms, uint32_t capacity,
                                    uint32_t* count);

/* ---- per-object moments of the grouped clouds -----------------------------------
 *
 * No reference counterpart; the rule is this library's specification.  Inputs: the grouped result
 * of the last gdf_seg_group_points / gdf_seg_object_points (rows points[total], obj_start[nobj + 1],
 * total a device word) and the grid of gdf_compute_voxel_coords: lower[3], cell[3] (f32), gs[3].
 * For a row p and axis a, with S = GDF_OBJ_SUBDIV:
 *   t[a] = (p[a] - lower[a]) / cell[a]     in f32, correctly rounded, not contracted (the
 *                                          expression of computeVoxelCoords)
 *   measured iff 0 <= t[a] && t[a] <= (float)gs[a] on all three axes (NaN fails)
 *   q[a] = min((uint32)(t[a] * S), S * gs[a] - 1)       (the product is exact; truncation)
 * so q[a] / S is the clamped voxel coordinate of every measured row.  Object o's record covers its
 * rows [obj_start[o], obj_start[o + 1]); unmeasured rows add to `outside` only.  Integer sums:
 * exact and independent of the order of the rows. */
#define GDF_OBJ_SUBDIV 256u

typedef struct gdf_obj_moments {
    uint32_t count, outside;      /* measured rows; the other rows of the object        */
    uint32_t qmin[3], qmax[3];    /* over measured rows; count == 0: 0xFFFFFFFF and 0   */
    uint64_t sum[3];              /* sum of q[a]                                        */
    uint64_t sum2[6];             /* sum of q[a] q[b] for xx, xy, xz, yy, yz, zz        */
} gdf_obj_moments;

/* Enqueued on the stream of the call that produced the grouped result, with no host wait (a
 * workspace buffer that has to grow is reallocated).  GDF_ERR_ARG: a null pointer, a cell[a] that
 * is not > 0, a grid_size[a] that is 0 or above 65536, and (256 max(grid_size) - 1)^2 * n_cap >=
 * 2^64 with n_cap the capacity of the grouped result (below it no sum can wrap).  GDF_ERR_STATE:
 * no grouped result (before any group call, or after a gdf_seg_label_* since the last one).
 * Every refusal comes before the first launch and leaves an earlier result alone.  The records
 * stay valid as long as the grouped result does. */
int gdf_seg_object_moments(gdf_segmenter* seg, const float lower[3], const float cell[3],
                           const uint32_t grid_size[3]);
/* nobj records (waits); GDF_ERR_CAPACITY when capacity < nobj, GDF_ERR_STATE without records */
int gdf_seg_download_object_moments(gdf_segmenter* seg, gdf_obj_moments* out, uint32_t capacity);
/* the same on the device */
int gdf_seg_get_device_object_moments(gdf_segmenter* seg, const gdf_obj_moments** moments);

/* Centroid, covariance and bounds in world units from the records: a pure host function (no GPU,
 * no handle).  In doubles, in exactly this order, with N = count, c_a = (double)cell[a] / 256.0,
 * l_a = (double)lower[a]:
 *   centroid[a]  = l_a + c_a * ((double)sum[a] / (double)N + 0.5)
 *   cov[ab]      = ((double)(N sum2[ab] - sum[a] sum[b]) / ((double)N * (double)N)) * c_a * c_b
 *                  (the numerator exact in 128-bit integers, converted once, to nearest even)
 *   min_world[a] = l_a + c_a * (double)qmin[a]
 *   max_world[a] = l_a + c_a * (double)(qmax[a] + 1)
 * count == 0 gives NaN in every field.  cov in the order of sum2. */
typedef struct gdf_obj_shape {
    double centroid[3];
    double cov[6];
    double min_world[3], max_world[3];
} gdf_obj_shape;

int gdf_obj_shapes_from_moments(const gdf_obj_moments* m, uint32_t nobj, const float lower[3],
                                const float cell[3], gdf_obj_shape* out);

/* ---- the voxel table of a list of cells; object ids for the voxelized cloud -----
 *
 * No reference counterpart; the rule is this library's specification.  Inputs: cells[n] (u32),
 * num_cells = C, and n as a value or a device word (count_device != NULL: n = min(*count_device,
 * n_cap)).
 *   outside      a row with cells[i] >= C marks nothing, counts nowhere and gets
 *                point_voxel[i] = GDF_VOX_NONE
 *   vox_cells    vox_cells[G]: the distinct cells below C, ascending; G is a device word too
 *   point_voxel  point_voxel[i] = the index of cells[i] in vox_cells
 *   vox_counts   vox_counts[g] = the number of rows with point_voxel == g
 * Rows at and beyond n are neither read nor written.  All outputs are integers and no output
 * depends on an order of execution: the result is exact.
 * The voxelize of gdf.h emits one row per distinct key of the frame's voxel coords, in ascending
 * key order, so with cells = the frame's coords and C = the grid's cell count, voxel g of the table
 * is voxelized row g: vox_counts[g] is the number of compacted points behind that row (the weight of
 * its mean) and point_voxel[i] is the voxelized row that compacted point i was folded into.
 * C is bounded by 2^28 cells: the table marks one bit per cell, a bitmap of at most 32 MB, which
 * (unlike the workspace of the object points) every call clears before its marks.
 * The workspace is grow-only, as the object points' is.  Results stay valid until the next
 * gdf_seg_label_*, gdf_seg_voxel_table or gdf_seg_object_voxels. */
#define GDF_VOX_NONE 0xFFFFFFFFu

/* the rule on any device array, on the segmenter's stream; needs no labelling.  GDF_ERR_ARG: a null
 * cells pointer, num_cells == 0, num_cells > 2^28.  n_cap == 0 succeeds with G = 0.  A refusal
 * leaves an earlier result readable. */
int gdf_seg_voxel_table(gdf_segmenter* seg, const uint32_t* cells_device, uint32_t n_cap,
                        const uint32_t* count_device, uint32_t num_cells);

/* Object ids for the engine's voxelized cloud, on the engine's stream: the table of the frame's
 * voxel coords; ids[g] = the object id of vox_cells[g] (the id rule above, G of them); voxels and
 * keep as gdf_seg_object_points computes them; the engine's voxelized rows partitioned by those
 * ids; weights[j] = vox_counts[index[j]].  The grouped result is THE grouped result of the
 * segmenter: it replaces an earlier gdf_seg_group_points / gdf_seg_object_points result, and
 * gdf_seg_get_object_points, gdf_seg_download_object_points, gdf_seg_get_device_object_points and
 * gdf_seg_object_moments work on it unchanged, with ids of G entries and index[j] a voxel index
 * (a voxelized row).  gdf_seg_object_moments on it is unweighted: every voxelized row counts once.
 * The rows grouped are min(G, the voxelize's own device count) of the engine's voxelized rows: the
 * two counts are equal for a frame's own coords, and the minimum keeps any mismatch inside the rows
 * the voxelize wrote.
 * Refusals, all before the first launch: what gdf_seg_object_points refuses, and GDF_ERR_STATE
 * before the frame's voxelize.  No host wait apart from the one for nobj after a labelling. */
int gdf_seg_object_voxels(gdf_segmenter* seg, gdf_engine* engine, uint32_t min_voxels);

/* G and n of the last table (waits) */
int gdf_seg_get_voxel_table(gdf_segmenter* seg, uint32_t* num_voxels, uint32_t* n);
/* Downloads (wait); every pointer may be NULL.  vox_cells and vox_counts: G words (vox_capacity);
 * point_voxel: n words (point_capacity); weights: the kept total of the grouped voxel rows
 * (weights_capacity), GDF_ERR_STATE unless the table is gdf_seg_object_voxels' and its grouped
 * result still stands.  GDF_ERR_CAPACITY when a capacity is too small. */
int gdf_seg_download_voxel_table(gdf_segmenter* seg, uint32_t* vox_cells, uint32_t* vox_counts,
                                 uint32_t vox_capacity, uint32_t* point_voxel,
                                 uint32_t point_capacity, uint32_t* weights,
                                 uint32_t weights_capacity);
/* the same on the device; weights is NULL where the download refuses it; count_device: G */
int gdf_seg_get_device_voxel_table(gdf_segmenter* seg, const uint32_t** vox_cells,
                                   const uint32_t** vox_counts, const uint32_t** point_voxel,
                                   const uint32_t** weights, const uint32_t** count_device);
/* With gdf_seg_set_profiling on, the last table call's times in milliseconds (waits): [clear],
 * [mark], [row sums + scan], [expand], [rank]: 5 values; after gdf_seg_object_voxels also
 * [ids + sizes], [group], [weights]: 8 values. */
int gdf_seg_get_voxel_table_times(gdf_segmenter* seg, float* ms, uint32_t capacity,
                                  uint32_t* count);

/* ---- the object layer per segment of the rows; per frame of a batch --------------
 *
 * No reference counterpart; the rules are this library's specification.
 *   segments     seg_start[nseg + 1]: u32 words on the device, 1 <= nseg <= 64, made non-decreasing
 *                and clamped to n_cap on read, as gdf_radius_filter_segments does:
 *                start'[s] = min(max(seg_start[0..s]), n_cap).  Row i lies in segment s iff
 *                start'[s] <= i < start'[s + 1]; rows in no segment are neither read nor written;
 *                empty segments are legal anywhere.
 *   partition    a row is kept iff ids[i] < nobj and (keep == NULL or keep[ids[i]]); its group is
 *                g = s(i) * nobj + ids[i].  The output is the kept rows stably partitioned by g:
 *                segment-major, then object, then input order, all four words bit for bit.
 *                grp_start[nseg * nobj + 1] ([0] = 0, the last = the kept total, a device word too)
 *                takes obj_start's place; index[j] is the (global) input row of output row j;
 *                seg_out_start[s] = grp_start[s * nobj], nseg + 1 words.  Segment s's part equals
 *                gdf_seg_group_points on the rows [start'[s], start'[s + 1]) alone, with index
 *                shifted by start'[s] and obj_start by seg_out_start[s].
 *   table        a row with cells[i] >= C is outside and gets point_voxel[i] = GDF_VOX_NONE; else
 *                its key is (s(i), cells[i]).  vox_cells[G]: the plain cells of the distinct keys,
 *                segment-major and ascending inside a segment; vox_seg_start[nseg + 1]: the first
 *                voxel of each segment, [nseg] = G (a device word too); point_voxel[i]: the global
 *                voxel index; vox_counts[g]: the rows with point_voxel == g.  Segment s's part
 *                equals gdf_seg_voxel_table on its rows alone, shifted by vox_seg_start[s].
 * All integers, a stable partition: the results are exact.
 *
 * A segmented grouped result is THE grouped result of the segmenter and a segmented table THE
 * table; the getters and downloads above serve them unchanged, with these sizes:
 *   obj_start   nseg * nobj + 1 words (grp_start), so obj_capacity must be at least that;
 *               gdf_seg_get_object_points still reports nobj (the labelling's, or the argument) and
 *               the kept total; ids are plain object ids, voxels nobj words
 *   moments     gdf_seg_object_moments on the result gives nseg * nobj records in group order, one
 *               per (segment, object); gdf_seg_download_object_moments needs that capacity, and the
 *               device getter's array has that length.  gdf_obj_shapes_from_moments is unchanged
 *               (pass nseg * nobj as its count).
 * Bounds: nseg * nobj <= 2^24 and nseg * C <= 2^28, else GDF_ERR_ARG.  GDF_ERR_ARG too for nseg
 * outside 1..64, nobj == 0, C == 0 and null pointers; n_cap == 0 succeeds with empty results.  Every
 * refusal comes before the first launch and leaves an earlier result readable.  No host wait (the
 * stage calls: the one for nobj after a labelling); the workspace is grow-only. */
int gdf_seg_group_points_segments(gdf_segmenter* seg, const float* points_device,
                                  const uint32_t* ids_device, uint32_t n_cap,
                                  const uint32_t* seg_start_device, uint32_t nseg, uint32_t nobj,
                                  const uint8_t* keep_device);
int gdf_seg_voxel_table_segments(gdf_segmenter* seg, const uint32_t* cells_device, uint32_t n_cap,
                                 const uint32_t* seg_start_device, uint32_t nseg, uint32_t num_cells);

/* The stage calls on an engine's batch, on the engine's stream: one segment per frame, the segments
 * being the engine's own device ranges (the tables gdf_get_batch_ranges downloads: the frames' point
 * ranges for the compacted points and coords, their voxel ranges for the voxelized rows); a single
 * frame is the one segment {0, its device count}.  Ids are taken against the segmenter's current
 * labelling, normally gdf_seg_label_engine_grid after the batch (the grid after the batch's last
 * frame); a batch's coords hold plain cells, so the id of a row is the rule of
 * gdf_seg_object_points on its cell, and voxels / keep are that call's.  With an occupancy lifetime
 * below the batch's frame count, cells of earlier frames may have decayed: their points get
 * GDF_OBJ_NONE, which is the rule and no error.
 * gdf_seg_object_points_batch: ids[n] of all frames' points and the points partitioned by
 * (frame, object).  gdf_seg_object_voxels_batch: the segmented table of the batch's coords; ids[G] of
 * vox_cells; the engine's voxelized rows, min(G, the voxelize's own count) of them, partitioned by
 * (frame of the voxel, object); weights as gdf_seg_object_voxels gives them.  On an engine's batch
 * vox_seg_start equals the engine's voxel ranges.
 * GDF_ERR_STATE: what gdf_seg_object_points / gdf_seg_object_voxels refuse, except the multi-frame
 * batch; a batch without frame ranges.  GDF_ERR_ARG: nframes * nobj > 2^24, nframes * cells > 2^28.
 * The profiled times are those of the single-frame calls (the composite pass before the table's
 * clear is not among them). */
int gdf_seg_object_points_batch(gdf_segmenter* seg, gdf_engine* engine, uint32_t min_voxels);
int gdf_seg_object_voxels_batch(gdf_segmenter* seg, gdf_engine* engine, uint32_t min_voxels);

/* seg_out_start of the segmented grouped result: nseg and, with seg_out_start != NULL, its nseg + 1
 * words (waits; GDF_ERR_CAPACITY below that).  GDF_ERR_STATE when the grouped result is not a
 * segmented one. */
int gdf_seg_get_group_segments(gdf_segmenter* seg, uint32_t* nseg, uint32_t* seg_out_start,
                               uint32_t capacity);
int gdf_seg_get_device_group_segments(gdf_segmenter* seg, const uint32_t** seg_out_start_device,
                                      uint32_t* nseg);
/* vox_seg_start of the segmented table, in the same way */
int gdf_seg_get_voxel_segments(gdf_segmenter* seg, uint32_t* nseg, uint32_t* vox_seg_start,
                               uint32_t capacity);
int gdf_seg_get_device_voxel_segments(gdf_segmenter* seg, const uint32_t** vox_seg_start_device,
                                      uint32_t* nseg);

#ifdef __cplusplus
}
#endif

#endif /* GDF_SEGMENT_H_ */
