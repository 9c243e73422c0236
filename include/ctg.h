/*
 * ctg.h -- C ABI of the MI355X-native RAG + edge-feature library (libctg.so).
 *
 * This is the drop-in boundary for the hot path of cluster_tools' multicut
 * feature stage.  In the reference, the job bodies call the pybind11 module
 * ``nifty.distributed`` (C++, third party, pinned nifty >=v1.0.7 in
 * conda-recipe/meta.yaml:30).  Each entry point below replaces the array-level
 * work of one of those calls; the N5 I/O those calls do stays in the Python
 * host layer (cluster_tools_amd/ndist.py), which mirrors the reference's
 * function names and arguments:
 *
 *   ctg_rag_features(... data=NULL)   <- ndist.computeMergeableRegionGraph
 *                                        graph/initial_sub_graphs.py:124-129
 *   ctg_rag_features(... boundary)    <- ndist.extractBlockFeaturesFromBoundaryMaps_{float32,uint8}
 *                                        features/block_edge_features.py:127-134
 *   ctg_rag_features(... affinities)  <- ndist.extractBlockFeaturesFromAffinityMaps_{float32,uint8}
 *                                        features/block_edge_features.py:138-145
 *   ctg_merge_stats                   <- ndist.mergeSubgraphs / ndist.mergeFeatureBlocks
 *                                        graph/merge_sub_graphs.py:130-135,
 *                                        features/merge_edge_features.py:141-147
 *   ctg_map_edge_ids                  <- ndist.mapEdgeIds / Graph.findEdges
 *                                        graph/map_edge_ids.py:116-119, test/graph/test_graph.py:92
 *   ctg_unique_labels                 <- the per-block ``nodes`` of computeMergeableRegionGraph
 *                                        test/graph/test_graph.py:53-60
 *   ctg_merge_feature_rows            <- ndist.mergeFeatureBlocks on reference-layout
 *                                        (10-column) sub_features rows,
 *                                        features/merge_edge_features.py:141-147
 *   ctg_label_overlaps                <- ndist.computeAndSerializeLabelOverlaps
 *                                        node_labels/block_node_labels.py:161
 *   ctg_merge_overlaps, ctg_max_overlaps <- ndist.mergeAndSerializeOverlaps
 *                                        node_labels/merge_node_labels.py:149
 *   ctg_morphology                    <- ndist.computeAndSerializeMorphology
 *                                        morphology/block_morphology.py:134
 *   ctg_merge_morphology, ctg_morphology_rows <- ndist.mergeAndSerializeMorphology
 *                                        morphology/merge_morphology.py:130
 *   ctg_region_features               <- _block_features, from np.unique to the feature arrays
 *                                        features/region_features.py:159-171
 *   ctg_merge_region_features, ctg_region_rows <- _extract_and_merge_region_features
 *                                        features/merge_region_features.py:109-158
 *   ctg_assignment_dense, ctg_apply_assignment  <- nifty.tools.take, write/write.py:164-166
 *   ctg_assignment_sparse, ctg_apply_assignment <- np.unique, the dict and nifty.tools.takeDict,
 *                                        write/write.py:170-181
 *   ctg_assignment_info               <- _write_maxlabel, write/write.py:281-289
 *   ctg_threshold_components          <- vu.normalize, the comparison and skimage.morphology.label,
 *                                        thresholded_components/block_components.py:161-182
 *   ctg_merge_assignments             <- nufd.boost_ufd and relabelConsecutive,
 *                                        thresholded_components/merge_assignments.py:125-132
 *   ctg_distance_transform            <- vigra.filters.distanceTransform and
 *                                        scipy.ndimage.distance_transform_edt,
 *                                        watershed/watershed.py:140-161,
 *                                        distances/object_distances.py:109-113,
 *                                        morphology/region_centers.py:122
 *   ctg_seeded_watershed              <- vigra.analysis.watershedsNew(hmap, seeds=...) and the
 *                                        size filter of elf's watershed,
 *                                        watershed/watershed_from_seeds.py:143-204
 *
 * Conventions: plain pointers and sizes; ``mem`` says whether array
 * arguments live in host memory (CTG_MEM_HOST) or in device memory of the
 * current HIP device (CTG_MEM_DEVICE); ``stream`` is a hipStream_t (NULL =
 * default stream).  Every function returns CTG_OK (0) or a negative status;
 * ctg_last_error() returns a thread-local message (the Python shim raises
 * RuntimeError with it, as pybind11 does for nifty's C++ exceptions).
 * Results are library-owned handles released with ctg_free().
 *
 * Streams (tests/test_gpu_streams.py holds every call below to this):
 *   - Every GPU operation of a call -- kernels, memsets, copies, the sorts and
 *     scans -- is issued on the call's ``stream``.  The library never issues
 *     work on the null stream unless that is the stream it was given, and never
 *     waits for it: a caller on a non-blocking stream is neither delayed by nor
 *     ordered against unrelated work on the null stream.  The only device-wide
 *     wait the library asks for is ctg_trim's (and ctg_diag_bounds' in CTG_DIAG
 *     builds); ctg_init makes the device's workspace on its first call and
 *     queues nothing.  What HIP itself does inside hipMalloc and hipFree is not
 *     the library's to promise: a call whose buffers outgrow the cached ones
 *     (the first call of a size, a call after ctg_trim, a purge of the pool on
 *     an out-of-memory) allocates or frees device memory, and the runtime may
 *     wait for the device there; steady-state calls reach neither.
 *   - Calls that return synchronised -- every operation of the call has
 *     completed when it returns (it has waited for ``stream``, unless it had
 *     nothing to issue: an empty input or box), outputs in host or device
 *     memory are complete, and the inputs may be reused or freed at once:
 *     ctg_rag_features, ctg_rag_blocks,
 *     ctg_unique_labels, ctg_unique_values, ctg_unique_pairs, ctg_merge_stats,
 *     ctg_merge_feature_rows, ctg_map_edge_ids with CTG_MEM_HOST,
 *     ctg_label_overlaps, ctg_merge_overlaps, ctg_max_overlaps, ctg_morphology,
 *     ctg_merge_morphology, ctg_morphology_rows, ctg_region_features,
 *     ctg_merge_region_features, ctg_region_rows, ctg_assignment_dense,
 *     ctg_assignment_sparse, ctg_apply_assignment, ctg_threshold_components,
 *     ctg_merge_assignments, ctg_distance_transform and ctg_seeded_watershed
 *     (with or without info, host or device memory) and ctg_mgpu_merge.
 *   - Calls that return with their work queued on ``stream`` (device memory
 *     only, no scratch of the library's pool): ctg_map_edge_ids with
 *     CTG_MEM_DEVICE, ctg_synth_volume, ctg_synth_affinities,
 *     ctg_filter_conv_axis, ctg_filter_combine, ctg_sym_eigenvalues,
 *     ctg_mgpu_sample, ctg_mgpu_split and ctg_mgpu_pack (a pack of a
 *     CTG_DEFER_STATS table reads the workspace's records, which a later scan
 *     on any stream overwrites: that pack alone is waited for).  Work queued on the
 *     same stream afterwards sees their finished outputs.  Until that work
 *     completes the caller must keep the inputs and outputs alive and
 *     unchanged, must not read the outputs from the host or from another stream
 *     without an event or a synchronisation, and (ctg_mgpu_*) must not free the
 *     handle the call reads.  Small host arguments (shapes, offsets, taps,
 *     counts_all) are consumed before the call returns.
 *   - The result accessors (ctg_result_copy_*) are host-synchronous: the data is
 *     at ``dst`` when they return.  They copy on a non-blocking stream of the
 *     library's own, so they do not depend on the null stream; a handle's
 *     tables are complete on every stream because the calls that fill them
 *     return synchronised.  A device ``dst`` must not be in use by work that is
 *     still queued.  ctg_morphology_rows, ctg_region_rows and ctg_max_overlaps
 *     read a handle on the stream they are given.
 *   - Calls on different streams of one device may follow one another freely
 *     (they are serialised per device by a lock).  The library's block pool
 *     knows nothing of streams, so a block returns to it while work that uses
 *     it is queued only inside a call that waits for its stream before it
 *     returns; every call that draws scratch from the pool is of that kind,
 *     where it succeeds and where it fails: a scope that owns pool blocks
 *     holds a guard below them that waits for the stream on every return path
 *     before a block goes back (csrc/ctg_buffers.h: StreamWait), so a call
 *     that fails after it queued work (a launch or copy that HIP refused, an
 *     allocation that failed half way) has waited as well.  The two face-scan
 *     calls and ctg_mgpu_merge keep the guards they had: ctg_rag_blocks waits
 *     on every path, ctg_rag_features once its adjacency filter exists and
 *     ctg_mgpu_merge once its merge scratch does; if one of these two fails
 *     with CTG_ERR_HIP before that, synchronise the stream before the next call.
 */
#ifndef CTG_H_
#define CTG_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTG_OK 0
#define CTG_ERR_ARG -1
#define CTG_ERR_HIP -2
#define CTG_ERR_NOMEM -3
#define CTG_ERR_UNSUPPORTED -4
#define CTG_ERR_STALE -5   /* a CTG_DEFER_STATS handle whose records were overwritten by a later call */

#define CTG_MEM_HOST 0
#define CTG_MEM_DEVICE 1

#define CTG_DATA_NONE 0   /* graph only */
#define CTG_DATA_F32 1
#define CTG_DATA_U8 2     /* mapped to [0,1] by /255 before binning (SURVEY OPEN-7) */

/* ctg_rag_features flags */
#define CTG_KEEP_STATS 1      /* keep mergeable per-edge statistics (ctg_result_copy_stats) */
#define CTG_NO_NODES 4        /* ctg_rag_blocks: skip the per-block node lists */
#define CTG_NO_ADJ_FILTER 2   /* affinities: keep sample pairs that are not nearest-neighbour
                                 edges of this array (their records carry no ADJ bit); the
                                 caller filters after a merge or by an edge list */
#define CTG_DEFER_STATS 8     /* with CTG_KEEP_STATS, for the ctg_mgpu_* exchange: no statistics
                                 rows are written; ctg_mgpu_pack / ctg_mgpu_merge rebuild a row's
                                 statistics from the call's records where the exchange needs them
                                 (rows sent to another rank, own rows that meet a received key).
                                 The records stay in the device's workspace, so the handle serves
                                 ctg_mgpu_pack / ctg_mgpu_merge only until the next ctg_rag_*,
                                 ctg_merge_stats or ctg_trim call on that device (then
                                 CTG_ERR_STALE), and
                                 ctg_result_copy_stats has no rows to copy.  Boundary maps without
                                 ignore_label; any other call writes the CTG_KEEP_STATS rows. */

#define CTG_MAX_CHANNELS 24
#define CTG_N_FEATURES 10
#define CTG_NBINS 40
#define CTG_WIDE_RECORD_WORDS 48  /* u32 words of one wide statistics record */

typedef struct ctg_result ctg_result;

/* version / device */
int ctg_version(void);
int ctg_init(int device);
const char* ctg_last_error(void);
int ctg_device_count(int* count);

/*
 * RAG (+ edge features) of one 3-D label array.
 *   labels     uint64 (label_bits=64) or uint32 (label_bits=32), C-order (Z,Y,X);
 *              X at most 2^32 / 40 (107 M) voxels: the scan's row loads carry
 *              32-bit byte offsets (wider arrays are refused)
 *   data       NULL, boundary map (Z,Y,X) or channel-first affinities (C,Z,Y,X)
 *   offsets    NULL for a boundary map, else n_channels x 3 int32 (z,y,x) offsets
 *   own_begin, own_end  faces / samples are counted only when their owning
 *              voxel lies in [own_begin, own_end): the upper voxel of a face, the
 *              voxel p of an affinity sample.  NULL = 0 / shape.  A 1-voxel
 *              own_begin is the lower-halo geometry of increaseRoi=True.
 *   ignore_label  drop edges that contain label 0 (nodes still contain 0)
 *   hist_lo/hi    histogram range (nifty: [0,1])
 *   flags         CTG_KEEP_STATS | CTG_NO_ADJ_FILTER
 * Result: sorted unique edges (u<v, lexicographic), sorted unique nodes and,
 * if data != NULL, an (E,10) float64 feature table
 * [mean, var, min, q10, q25, q50, q75, q90, max, count].
 */
int ctg_rag_features(const void* labels, int label_bits,
                     const void* data, int data_kind,
                     int n_channels, const int32_t* offsets,
                     const int64_t* shape, const int64_t* own_begin, const int64_t* own_end,
                     int ignore_label, double hist_lo, double hist_hi,
                     int flags, int mem, void* stream, ctg_result** out);

/*
 * Batched per-block sub-graphs and features (the ndist per-block calls in
 * one launch): block b is a C-order array of shape[b] starting at element
 * label_offset[b] of `labels` (and data_offset[b] of `data`; affinities
 * channel-first, C x shape).  For every block:
 *   nodes    sorted unique labels of the own box (inner block,
 *            test/graph/test_graph.py:53-60)
 *   edges    sorted unique (u<v) keys of the faces with both voxels in the
 *            graph box (increaseRoi: [begin-1, end), test_graph.py:42-84)
 *   features (data != NULL) per edge, the 10 features of the samples owned by
 *            the block -- boundary faces / affinity voxels whose upper voxel /
 *            voxel p lies in the own box; edges of the graph box without owned
 *            samples get count 0 (block_edge_features.py:127-145).  With
 *            affinities a sample counts only if its pair is an edge of the
 *            block's sub-graph.
 * Rows [edge_off[b], edge_off[b+1]) of the edge / feature / stats tables and
 * [node_off[b], node_off[b+1]) of the node table belong to block b
 * (ctg_result_block_offsets).  Replaces the per-block loops of
 * ndist.computeMergeableRegionGraph (graph/initial_sub_graphs.py:124-129) and
 * ndist.extractBlockFeaturesFrom*Maps_* (features/block_edge_features.py:127-145).
 */
typedef struct ctg_block_desc {
    int64_t label_offset;
    int64_t data_offset;
    int64_t shape[3];
    int64_t own_begin[3], own_end[3];
    int64_t graph_begin[3], graph_end[3];
} ctg_block_desc;

int ctg_rag_blocks(const void* labels, int label_bits, const void* data, int data_kind, int n_channels,
                   const int32_t* offsets, const ctg_block_desc* blocks, int n_blocks, int64_t labels_len,
                   int64_t data_len, int ignore_label, double hist_lo, double hist_hi, int flags, int mem,
                   void* stream, ctg_result** out);
int ctg_result_num_blocks(const ctg_result* r);
/* page-locked host buffers for staging batched inputs (H2D at full PCIe rate) */
void* ctg_host_alloc(int64_t bytes);
void ctg_host_free(void* p);
int ctg_result_block_offsets(const ctg_result* r, int64_t* edge_off, int64_t* node_off);

/* sorted unique labels of labels[begin:end] (box in array coordinates) */
int ctg_unique_labels(const uint64_t* labels, const int64_t* shape,
                      const int64_t* begin, const int64_t* end,
                      int mem, void* stream, ctg_result** out);

/* sorted unique values of an (n,) uint64 list -> result nodes (union of the
 * per-slab node lists of the multi-GPU path; ndist.mergeSubgraphs node union,
 * graph/merge_sub_graphs.py:130-135) */
int ctg_unique_values(const uint64_t* values, int64_t n, int mem, void* stream, ctg_result** out);

/* Combine partial statistics tables (wide records, one per (part, edge)) into
 * one table: counts add, moments combine exactly (re-pivoted shifted sums,
 * i.e. Chan's pairwise rule), min/max elementwise, histograms add.
 *   keys     n x 2 uint64 (u,v) per record;
 *   sums     n x 2 float64 (S1, S2) = (sum(x - p), sum((x - p)^2)) about the
 *            record's pivot p = the float32 in record word 45 (0: power sums);
 *   records  n x CTG_WIDE_RECORD_WORDS uint32: 42 histogram slots, count|ADJ,
 *            ordered min, ordered max, pivot bits, 2 zero words. */
int ctg_merge_stats(const uint64_t* keys, const double* sums, const uint32_t* records,
                    int64_t n, double hist_lo, double hist_hi, int keep_stats,
                    int mem, void* stream, ctg_result** out);

/* Multi-GPU z-slab plan (SURVEY §8(b) ctg_mgpu_*; replaces the reference's
 * block-grid job split, graph/initial_sub_graphs.py:110-129 with
 * utils/volume_utils.py blocks_in_volume, for one rank per GPU): rank `rank` of
 * `world_size` owns planes [out[1], out[2]) = [Z*rank/W, Z*(rank+1)/W) of a
 * volume of Z planes and reads [out[0], out[2]): below its owned range as many
 * halo planes as the face / offsets reach down (1 for boundary maps and
 * nearest-neighbour affinities, max(-o_z) for long-range offsets), none for
 * rank 0.  ctg_rag_features' own_begin[0] is out[1] - out[0].  Positive z
 * offsets (a partner above the slab) with world_size > 1 are
 * CTG_ERR_UNSUPPORTED: the z-slab layout has no upper halo.  Host-only: needs
 * no device. */
int ctg_mgpu_slab(int64_t Z, int world_size, int rank, const int64_t* offsets, int n_channels, int64_t* out);

/* Multi-GPU combine of the ranks' partial tables (replaces the
 * block -> merge step of ndist.mergeSubgraphs, graph/merge_sub_graphs.py:130-135,
 * and ndist.mergeFeatureBlocks, features/merge_edge_features.py:141-147, at the
 * scale of whole GPUs).  `local` is a rank's CTG_KEEP_STATS result of its slab
 * (affinities: also CTG_NO_ADJ_FILTER).  The global sorted edge table is
 * range-partitioned by u; the host runs the collectives (RCCL over xGMI via
 * torch.distributed in cluster_tools_amd/dist.py) between these steps, all
 * arrays in device memory of the current device:
 *   1. ctg_mgpu_sample -> meta (CTG_MGPU_SAMPLES + 1 int64): evenly spaced u
 *      values (unsigned order as int64: u xor 2^63) and the edge count;
 *      all_gather of meta -> meta_all (world x (CTG_MGPU_SAMPLES + 1));
 *   2. ctg_mgpu_split -> counts (world x 2 int64): rows and node ids this rank
 *      sends to each rank (its own entry: what it keeps); all_gather ->
 *      counts_all (world x world x 2, [src][dst][rows, nodes]), read to host;
 *   3. ctg_mgpu_pack -> send (int64 words): for every dst != rank with data, in
 *      rank order, rows x CTG_MGPU_ROW_WORDS words ((u, v), (S1, S2) bits, the
 *      48-word wide record) then the node ids; all_to_all with those sizes ->
 *      recv (segments of every src != rank in rank order);
 *   4. ctg_mgpu_merge -> *out: this rank's shard of the global table (sorted
 *      edges, features, nodes); equal keys combine exactly (counts and
 *      histograms add, moments by Chan's rule), affinity partials keep keys
 *      whose ADJ bit some record carries.  `local`'s arrays move into the shard
 *      (a range of them when nothing was received: no copy); ctg_free(local)
 *      is still required.  counts_all is host memory.
 * world_size <= CTG_MGPU_MAX_WORLD. */
#define CTG_MGPU_SAMPLES 1024
#define CTG_MGPU_ROW_WORDS 28
#define CTG_MGPU_MAX_WORLD 32
int ctg_mgpu_sample(const ctg_result* local, int64_t* meta, void* stream);
int ctg_mgpu_split(const ctg_result* local, const int64_t* meta_all, int world_size, int64_t* counts, void* stream);
int ctg_mgpu_pack(const ctg_result* local, const int64_t* counts_all, int world_size, int rank, int64_t* send,
                  void* stream);
int ctg_mgpu_merge(ctg_result* local, const int64_t* recv, const int64_t* counts_all, int world_size, int rank,
                   double hist_lo, double hist_hi, void* stream, ctg_result** out);

/* Merge reference-layout feature rows (n x 10 float64, [mean, var, min,
 * q10..q90, max, count]) of global edges ids[i] in [id_begin, id_end) into
 * out ((id_end - id_begin) x 10): count sum, count-weighted mean, exact pooled
 * variance, min / max over rows with count > 0, count-weighted quantiles.
 * Edges without rows get zero rows.  An id outside the range is CTG_ERR_ARG. */
int ctg_merge_feature_rows(const uint64_t* ids, const double* rows, int64_t n, int64_t id_begin, int64_t id_end,
                           double* out, int mem, void* stream);

/* sorted unique (u,v) pairs of an (n,2) uint64 list (union of block sub-graph
 * edge lists, ndist.mergeSubgraphs); result nodes = unique endpoints */
int ctg_unique_pairs(const uint64_t* pairs, int64_t n, int mem, void* stream, ctg_result** out);

/*
 * Label overlaps (NodeLabelWorkflow): the contingency table of two label
 * volumes over the box [begin, end) (NULL = 0 / shape) -- for every pair
 * (a, b) = (labels[p], values[p]) that occurs, the number of voxels p.
 * Replaces the array work of ndist.computeAndSerializeLabelOverlaps
 * (node_labels/block_node_labels.py:161; its N5 chunk is written by
 * cluster_tools_amd/ndist.py).
 *   labels, values  uint64 (bits = 64) or uint32 (bits = 32), C-order (Z,Y,X),
 *                   both of `shape`; any label value, 2^32 and above included
 *   with_ignore     skip voxels whose *value* equals ignore_label
 *                   (block_node_labels.py:152-156 applies it to that volume)
 * Result: edges = the distinct (a, b) pairs, sorted lexicographically;
 * ctg_result_copy_counts = their voxel counts (uint64); nodes = the distinct a,
 * ascending.  An empty box, or one whose every voxel is ignored, gives an
 * empty result; a box outside the array is CTG_ERR_ARG; a box of 2^32 voxels
 * or more is CTG_ERR_UNSUPPORTED.  ctg_result_info: the (pair, count) records
 * the scan wrote, and how many of them bypassed the workgroup tables.
 * The overlaps calls keep their records in buffers of their own: they leave the
 * workspace's records alone, so a CTG_DEFER_STATS handle of the same device
 * stays valid across them.
 */
int ctg_label_overlaps(const void* labels, int label_bits, const void* values, int value_bits,
                       const int64_t* shape, const int64_t* begin, const int64_t* end,
                       int with_ignore, uint64_t ignore_label, int mem, void* stream, ctg_result** out);

/* Combine partial overlap tables -- n rows (a, b) with uint64 counts, in any
 * order -- into one table of the form above: equal pairs add their counts.
 * The array work of ndist.mergeAndSerializeOverlaps
 * (node_labels/merge_node_labels.py:149). */
int ctg_merge_overlaps(const uint64_t* pairs, const uint64_t* counts, int64_t n, int mem, void* stream,
                       ctg_result** out);

/* Per label a in [label_begin, label_end): out_labels[a - label_begin] = the b
 * with the largest count in the overlaps result r, out_counts (may be NULL) =
 * that count; 0 / 0 for labels without a row.  Equal counts go to the smallest
 * b (nifty's rule is not in the reference; test/node_labels/test_node_labels.py:31-33
 * masks ties out).  The max_overlap branch of ndist.mergeAndSerializeOverlaps
 * (node_labels/merge_node_labels.py:149-155). */
int ctg_max_overlaps(const ctg_result* r, uint64_t label_begin, uint64_t label_end, uint64_t* out_labels,
                     uint64_t* out_counts, int mem, void* stream);

/*
 * Segment morphology (MorphologyWorkflow): per label of the box [begin, end)
 * (NULL = 0 / shape) of a label volume the voxel count, the integer coordinate
 * sums and the bounding box.  The coordinate of the voxel at array index p is
 * p + origin (NULL = 0; the block's begin when `labels` is one block of a
 * volume).  Replaces the array work of ndist.computeAndSerializeMorphology
 * (morphology/block_morphology.py:134; its N5 chunk is written by
 * cluster_tools_amd/ndist.py).
 *   labels   uint64 (label_bits = 64) or uint32 (32), C-order (Z,Y,X) of `shape`;
 *            any label value, 2^32 and above included; label 0 is a label like
 *            any other
 * Result: nodes = the distinct labels, ascending; ctg_result_copy_moments = an
 * (N,10) uint64 table [n, sum z, sum y, sum x, min z, min y, min x, max z,
 * max y, max x] (max inclusive); ctg_morphology_rows = the float64 rows
 *   [id, size, com_z, com_y, com_x, min_z, min_y, min_x, max_z, max_y, max_x]
 * of block_morphology.py:128-133, com = (double)sum / (double)n.  An empty box
 * gives an empty result; a box outside the array is CTG_ERR_ARG; a box of 2^32
 * voxels or more is CTG_ERR_UNSUPPORTED; origin + end must stay below 2^31 on
 * every axis (CTG_ERR_ARG), so no sum reaches 2^63.  ctg_result_info: the
 * records the scan wrote, and how many of them bypassed the workgroup tables.
 * Like the overlaps calls these keep their records in buffers of their own: a
 * CTG_DEFER_STATS handle of the same device stays valid across them.
 */
#define CTG_MORPH_COLS 11
int ctg_morphology(const void* labels, int label_bits, const int64_t* shape,
                   const int64_t* begin, const int64_t* end, const int64_t* origin,
                   int mem, void* stream, ctg_result** out);

/* Combine partial morphology tables -- n rows of the 11-column float64 form, in
 * any order -- into one result of the form above: per id the sizes add, the
 * boxes fold, and the coordinate sums add as integers, each row's sum recovered
 * as rint(com * size).  The recovery is exact while a row's sum is below 2^51
 * (a block of 2^32 voxels at coordinates up to 2^19), and the merged table then
 * equals one ctg_morphology call over the whole volume bit for bit; past that
 * bound the sums are rounded.  Rows of size 0 (the zero rows of absent labels)
 * add nothing.  An id that is not an integer in [0, 2^53), or a negative or
 * non-finite entry, is CTG_ERR_ARG.  The array work of
 * ndist.mergeAndSerializeMorphology (morphology/merge_morphology.py:130). */
int ctg_merge_morphology(const double* rows, int64_t n, int mem, void* stream, ctg_result** out);

/* the (N,10) uint64 moments of a morphology result */
int ctg_result_copy_moments(const ctg_result* r, uint64_t* dst, int mem);

/* The float64 rows of a morphology result: `rows` (may be NULL) receives the
 * (N,11) rows of its labels in ascending order; `out` (may be NULL) is a dense
 * (label_end - label_begin, 11) table that receives the row of every label in
 * [label_begin, label_end) at label - label_begin and zeros for absent labels
 * (what an unwritten chunk of the output dataset reads as).  A table with a
 * label of 2^53 or more is CTG_ERR_UNSUPPORTED: the id column cannot hold it. */
int ctg_morphology_rows(const ctg_result* r, uint64_t label_begin, uint64_t label_end,
                        double* out, double* rows, int mem, void* stream);

/*
 * Region features (RegionFeaturesWorkflow): per label of the box [begin, end)
 * (NULL = 0 / shape) of a label volume the voxel count and the sum, the minimum
 * and the maximum of the samples of `data` at its voxels.  Replaces the array
 * work of _block_features (features/region_features.py:159-171: np.unique, the
 * dict relabelling and vigra.analysis.extractRegionFeatures); the chunk is
 * written by cluster_tools_amd/features.py.
 *   labels   uint64 (label_bits = 64) or uint32 (32), C-order (Z,Y,X) of `shape`;
 *            any label value, 2^32 and above included; label 0 is a label like
 *            any other unless it is the ignore label
 *   data     CTG_DATA_F32 or CTG_DATA_U8, of `shape` (a channel of a 4-D input is
 *            that channel's plane, region_features.py:155); samples enter as they
 *            are, u8 as their integer value -- the normalisation of
 *            region_features.py:151-157 is ctg_region_rows' `norm`
 *   has_ignore  voxels whose *label* equals ignore_label are not counted and
 *            that label gets no row (vigra's ignoreLabel, region_features.py:170-171)
 * Result: nodes = the distinct counted labels, ascending; ctg_result_copy_region
 * = their counts (uint64), sums (float64) and (min, max) (float32).  A sum is
 * made of float64 adds of the samples, each exact, in no fixed order: where
 * every partial sum is representable (u8 data; f32 data on a grid such as
 * k / 256) the bits are the same in every run and across a merge, otherwise two
 * orders of n terms differ by at most 2 (n - 1) 2^-53 sum|x|.  Non-finite
 * samples: sums follow IEEE; the min and max of a label that holds a NaN are
 * unspecified.  An empty box, or one whose every voxel is ignored, gives an
 * empty result; a box outside the array is CTG_ERR_ARG; a box of 2^32 voxels or
 * more is CTG_ERR_UNSUPPORTED.  ctg_result_info: the records the scan wrote,
 * and how many of them bypassed the workgroup tables.  Like the overlaps calls
 * these keep their records in buffers of their own: a CTG_DEFER_STATS handle of
 * the same device stays valid across them.  Every argument error is found
 * before any GPU work and leaves *out NULL.
 */
#define CTG_REGION_COLS 5
#define CTG_REGION_SUMS 0       /* rows [id, count, sum, min, max]: the chunk form ctg_merge_region_features reads */
#define CTG_REGION_FEATURES 1   /* rows [id, count, mean, minimum, maximum], normalised */
int ctg_region_features(const void* labels, int label_bits, const void* data, int data_kind,
                        const int64_t* shape, const int64_t* begin, const int64_t* end,
                        int has_ignore, uint64_t ignore_label, int mem, void* stream, ctg_result** out);

/* Combine partial region tables -- n rows of the 5-column float64 sum form, in
 * any order -- into one result of the form above: per id the counts add
 * (uint64), the sums add (float64), min and max fold.  Sums stay sums until the
 * one division of ctg_region_rows, where merge_feats
 * (features/merge_region_features.py:94-106) re-weights means block by block in
 * float32; for exactly summable data the merged table equals one
 * ctg_region_features call over the whole volume bit for bit.  Rows of count 0
 * add nothing.  An id that is not an integer in [0, 2^53), or a negative or
 * non-finite count, is CTG_ERR_ARG.  The array work of
 * _extract_and_merge_region_features (features/merge_region_features.py:109-156). */
int ctg_merge_region_features(const double* rows, int64_t n, int mem, void* stream, ctg_result** out);

/* The float64 rows of a region-features result, in `form`: CTG_REGION_SUMS
 * [id, count, sum, min, max], or CTG_REGION_FEATURES [id, count, mean, minimum,
 * maximum] with mean = (sum / (double)count) / norm, minimum = min / norm,
 * maximum = max / norm -- norm 255.0 for uint8 input and 1.0 otherwise
 * (vu.normalize, features/region_features.py:151-157); norm must be finite and
 * positive.  `rows` (may be NULL) receives the (N,5) rows of the labels in
 * ascending order; `out` (may be NULL) is a dense (label_end - label_begin, 5)
 * table that receives the row of every label in [label_begin, label_end) at
 * label - label_begin and zeros for absent labels (what
 * features/merge_region_features.py:157 makes of their 0 / 0).  A table with a
 * label of 2^53 or more is CTG_ERR_UNSUPPORTED: the id column cannot hold it. */
int ctg_region_rows(const ctg_result* r, uint64_t label_begin, uint64_t label_end, int form, double norm,
                    double* out, double* rows, int mem, void* stream);

/* the (N,) uint64 counts, (N,) float64 sums and (N,2) float32 (min, max) of a
 * region-features result, which hold any label; each destination may be NULL
 * (the feats['count'] ... arrays of features/region_features.py:170) */
int ctg_result_copy_region(const ctg_result* r, uint64_t* counts, double* sums, float* minmax, int mem);

/*
 * Write (WriteWorkflow, and every task that ends in nifty.tools.take /
 * takeDict): a node assignment A, uploaded once, and its application to label
 * arrays, out[i] = A(labels[i] + (labels[i] != 0 ? offset : 0)).
 *
 * ctg_assignment_dense   <- the table that nifty.tools.take indexes, write/write.py:164-166:
 *                           A(l) = table[l]; l >= n is out of range (the assert of write.py:164).
 *                           The handle holds a copy of the table.
 * ctg_assignment_sparse  <- the dict of write/write.py:170-181 (np.unique, the dict
 *                           comprehension, nifty.tools.takeDict): A(keys[i]) = values[i], keys in
 *                           any order.  A key given twice is CTG_ERR_ARG, the message holds the
 *                           count.  0 is a key like any other: without it, zero voxels are missing.
 * ctg_assignment_info    <- _write_maxlabel, write/write.py:281-289: n entries / pairs, the
 *                           largest value (0 for an empty assignment) and the kind; each
 *                           destination may be NULL
 * ctg_assignment_free    a NULL handle is fine
 */
#define CTG_ASSIGN_DENSE 0
#define CTG_ASSIGN_SPARSE 1
#define CTG_ERR_MISSING -6   /* ctg_apply_assignment: a label without an entry (the outputs are written all the same) */
typedef struct ctg_assignment ctg_assignment;
int ctg_assignment_dense(const uint64_t* table, int64_t n, int mem, void* stream, ctg_assignment** out);
int ctg_assignment_sparse(const uint64_t* keys, const uint64_t* values, int64_t n, int mem, void* stream,
                          ctg_assignment** out);
int ctg_assignment_info(const ctg_assignment* a, int64_t* n, uint64_t* max_value, int* kind);
void ctg_assignment_free(ctg_assignment* a);

/* Apply an assignment to a flat array of n labels (write/write.py:194-200 with
 * the lookups of :166 / :181; one call serves the blocks of a job).
 *   labels      n labels, uint64 (label_bits = 64) or uint32 (32), aligned to their size
 *   seg_begin   NULL: one segment [0, n) without offset (n_seg is not looked at).  Else
 *               n_seg + 1 host entries that ascend from 0 to n: segment k is
 *               [seg_begin[k], seg_begin[k + 1]) and nonzero labels in it are shifted by
 *               seg_offset[k] (host, n_seg entries) before the lookup; an empty segment is fine
 *   out         n uint64 values (`mem` as labels), or NULL: check only -- the same
 *               counts, nothing written.  out == labels (64-bit labels) works in place.
 *   seg_nonzero host, one word per segment: its nonzero input voxels (write.py:230
 *               skips blocks where it is 0)
 *   missing     host, 2 words: [0] the voxels whose shifted label is out of range
 *               (dense) or absent (sparse), [1] the smallest such label (0 if none).  A
 *               shift that wraps past 2^64 always counts, with the unshifted label as
 *               its candidate for [1].
 * A missing voxel's output is its shifted label.  With allow_missing (sparse
 * only: allow_empty_assignments, write.py:173-174) that is the result and the
 * call succeeds, missing[] still reporting them; otherwise any missing voxel makes the
 * call CTG_ERR_MISSING, the message naming the count and the smallest label,
 * with every output written.  Argument errors (CTG_ERR_ARG) are found before
 * any GPU work: null pointers, label_bits, n < 0, a seg_begin that does not
 * ascend from 0 to n, allow_missing with a dense assignment, in place with
 * 32-bit labels, misaligned arrays.  The call uses call-sized buffers only: a
 * CTG_DEFER_STATS handle of the same device stays valid across it. */
int ctg_apply_assignment(const ctg_assignment* a, const void* labels, int label_bits, int64_t n,
                         const int64_t* seg_begin, const uint64_t* seg_offset, int64_t n_seg, int allow_missing,
                         uint64_t* out, uint64_t* seg_nonzero, uint64_t* missing, int mem, void* stream);

/*
 * Thresholded components (ThresholdedComponentsWorkflow): the connected
 * components of a thresholded box, and the union-find merge of the block-offset
 * ids that the block faces join.
 *
 * ctg_threshold_components <- vu.normalize, the comparison, np.sum,
 *                           skimage.morphology.label and max of _cc_block /
 *                           _cc_block_with_mask,
 *                           thresholded_components/block_components.py:161-182, :211-233
 *   data        the (Z,Y,X) array, float32 (CTG_DATA_F32) or uint8 (CTG_DATA_U8);
 *               shape / begin / end as ctg_label_overlaps (NULL: the whole array)
 *   mask        NULL, or a uint8 array of the same shape: a voxel whose mask is 0 is
 *               background (block_components.py:225)
 *   normalize   0: the sample widened to float32 is compared.  Else the value of
 *               vu.normalize (utils/volume_utils.py:98-105) over the box: v = x - min, and
 *               v /= max(x - min) where that is > 0 -- float32 arithmetic, the divide
 *               correctly rounded.  A NaN in the box makes numpy's minimum NaN: the result
 *               is empty.  Without normalize a NaN voxel is background in every mode.
 *   mode        v > threshold, v < threshold or v == threshold, in float32
 *   connectivity 1, 2 or 3: voxels with 0 < |dz| + |dy| + |dx| <= connectivity are
 *               neighbours (6, 18, 26 of them; skimage's label on a boolean array: 3)
 *   out         box-shaped uint64: 0 for the background, components numbered
 *               1 .. *n_components in raster (C) order of each component's first voxel --
 *               scipy.ndimage.label's numbering
 * A box outside the array, a bad data_kind, mode or connectivity is CTG_ERR_ARG;
 * a box of 2^32 voxels or more is CTG_ERR_UNSUPPORTED.
 *
 * ctg_merge_assignments  <- nufd.boost_ufd(labels), ufd.merge, ufd.find and
 *                           relabelConsecutive(keep_zeros=True, start_label=1),
 *                           thresholded_components/merge_assignments.py:125-132
 *   pairs       (n, 2) uint64 ids to unite, in any order, repeats allowed
 *   table       n_labels uint64: table[0] = 0, every other id maps to 1 + the rank of
 *               its set's smallest member among those of all sets of 1 .. n_labels - 1
 *               (the consecutive table the reference computes and then does not save,
 *               merge_assignments.py:131)
 *   max_id      the largest entry of table
 * A pair member that is 0 or not below n_labels is CTG_ERR_ARG and the table is
 * not written; n_labels of 2^32 or more is CTG_ERR_UNSUPPORTED.
 *
 * Both calls use call-sized buffers only: a CTG_DEFER_STATS handle of the same
 * device stays valid across them.  ctg_last_timings of a profiled call:
 * ctg_threshold_components [0] range, [1] tiles, [2] seams, [3] flatten,
 * [4] scan, [5] write, [6] total; ctg_merge_assignments [0] init, [1] pairs,
 * [2] flatten, [3] scan, [4] write, [6] total.
 */
#define CTG_CC_GREATER 0
#define CTG_CC_LESS 1
#define CTG_CC_EQUAL 2
int ctg_threshold_components(const void* data, int data_kind, const void* mask, const int64_t* shape,
                             const int64_t* begin, const int64_t* end, float threshold, int mode, int normalize,
                             int connectivity, uint64_t* out, int mem, void* stream, uint64_t* n_components);
int ctg_merge_assignments(const uint64_t* pairs, int64_t n, uint64_t n_labels, uint64_t* table, int mem,
                          void* stream, uint64_t* max_id);

/*
 * The exact Euclidean distance transform of a box.
 *
 * ctg_distance_transform <- vigra.filters.distanceTransform of _apply_dt
 *                           (watershed/watershed.py:140-161), of fit_to_hmap
 *                           (utils/volume_utils.py:296-325) and of
 *                           upsample_skeletons.py:121;
 *                           scipy.ndimage.distance_transform_edt of
 *                           _labels_and_distances (distances/object_distances.py:109-113)
 *                           and of region_centers_for_label_range
 *                           (morphology/region_centers.py:106-133)
 *   src, src_kind, src_bits  the (Z,Y,X) array and the predicate P on it:
 *               CTG_EDT_SRC_NONZERO  uint8 / bool (src_bits 8), P = x != 0
 *               CTG_EDT_SRC_GREATER  float32 (src_bits 32), P = x > (float)threshold in
 *                                    float32; a NaN is not greater (watershed.py:143
 *                                    without the cast)
 *               CTG_EDT_SRC_EQUAL    uint32 or uint64 labels (src_bits 32 / 64),
 *                                    P = x == label; label may be 2^32 or above
 *                                    (object_distances.py:111, region_centers.py:118
 *                                    without the host-side mask)
 *               shape / begin / end as ctg_label_overlaps (NULL: the whole array)
 *   pitch       NULL (1, 1, 1), or the voxel size (z, y, x), each finite and > 0
 *               (pixel_pitch, sampling)
 *   flags       CTG_EDT_TO_BACKGROUND  the seeds are the voxels where P fails (scipy's
 *                                      distance_transform_edt, vigra's background=False);
 *                                      without it they are those where P holds (vigra's
 *                                      background=True)
 *               CTG_EDT_2D             every z-slice of the box on its own
 *                                      (watershed.py:151-155)
 *               CTG_EDT_OUT_D2         out is box-shaped float64 and receives D2 itself (the
 *                                      square of scipy's float64 result)
 *   out         box-shaped float32.  For a voxel p whose nearest seed of the box is q,
 *               d = p - q in index units:
 *                 D2  = (dz*pz)*(dz*pz) + (dy*py)*(dy*py) + (dx*px)*(dx*px)   float64, this order
 *                 out = (float)sqrt(D2)                       sqrt correctly rounded in float64
 *               Nothing outside the box is a seed.  A voxel whose domain (the box; with
 *               CTG_EDT_2D its slice) holds no seed gets the domain's diagonal,
 *               (float)sqrt((nz*pz)^2 + (ny*py)^2 + (nx*px)^2) -- without the z term in
 *               2-D mode --, a finite strict upper bound of every distance there.
 *   info        NULL, or 4 host words: [0] the seeds in the box, [1] the voxels written
 *               with the diagonal, [2] the flat C-order index in the box of the first voxel
 *               with the largest D2 (the diagonal's square for voxels without a seed; ties go
 *               to the smallest index), [3] that D2 as float64 bits.  The arg-max is taken
 *               on D2, not on the float32 output, as np.argmax of scipy's float64 result
 *               (region_centers.py:125).
 * With integer-valued pitches and (nz*pz)^2 + (ny*py)^2 + (nx*px)^2 < 2^53 every
 * term is exact and the result equals
 * distance_transform_edt(~seeds, sampling=pitch).astype(float32) bit for bit; with
 * other pitches a different choice among near-equal seeds moves it by at most 1
 * float32 ulp.
 * Argument errors, found before any GPU work: a null src / shape / out, a box
 * outside the array, a bad src_kind, src_bits, flag or mem, a pitch that is not
 * finite and positive: CTG_ERR_ARG.  A box of 2^32 voxels or more, or an axis of
 * the box of 32768 or more: CTG_ERR_UNSUPPORTED.  An empty box writes nothing
 * (info is zeroed) and succeeds.  The call uses call-sized buffers only: a
 * CTG_DEFER_STATS handle of the same device stays valid across it.
 * ctg_last_timings of a profiled call: [0] x pass, [1] y pass, [2] z pass,
 * [6] total.
 */
#define CTG_EDT_SRC_NONZERO 0
#define CTG_EDT_SRC_GREATER 1
#define CTG_EDT_SRC_EQUAL 2
#define CTG_EDT_TO_BACKGROUND 1
#define CTG_EDT_2D 2
#define CTG_EDT_OUT_D2 4
int ctg_distance_transform(const void* src, int src_kind, int src_bits, const int64_t* shape, const int64_t* begin,
                           const int64_t* end, double threshold, uint64_t label, const double* pitch, int flags,
                           void* out, int mem, void* stream, uint64_t* info);

/*
 * The seeded watershed of a box: every voxel takes the label of the seed it is
 * flooded from.
 *
 * ctg_seeded_watershed <- vigra.analysis.watershedsNew(hmap, seeds=...) of
 *                         _ws_block / _ws_block_masked
 *                         (watershed/watershed_from_seeds.py:143-204), of
 *                         watershed/watershed.py:227,246,
 *                         two_pass_watershed.py:166,207, fit_to_hmap
 *                         (utils/volume_utils.py:313,332) and
 *                         postprocess/filling_size_filter.py:134, with the size
 *                         filter of elf's watershed
 *   hmap        the (Z,Y,X) float32 heights.  +-inf are ordinary values; a NaN in
 *               the box is CTG_ERR_ARG, found before anything is written
 *   seeds, seed_bits   the (Z,Y,X) uint32 or uint64 seeds (seed_bits 32 / 64), 0 =
 *               no seed; a label may be 2^32 or above
 *               shape / begin / end as ctg_label_overlaps (NULL: the whole array)
 *   flags       CTG_WS_2D   only the y and x edges exist: every z-slice of the box
 *                           floods on its own
 *   size_filter 0 (none), or the voxels a label must have to stay (below)
 *   out         box-shaped uint64.  It may be `seeds` itself where the seeds are
 *               64-bit and the box is the whole array (vigra's out=labels, the
 *               in-place dataset of watershed_from_seeds); it must not overlap
 *               the seeds in any other way
 *   info        NULL, or 4 host words: [0] the largest label written, [1] the
 *               voxels left 0, [2] the rounds of the last flood, [3] the labels
 *               the size filter dropped (counted per domain)
 *
 * The result is defined by a rule, not by an execution order.  The voxels of
 * the box are the nodes of a graph whose edges join 6-neighbours (with
 * CTG_WS_2D the y and x neighbours).  k(h) is the order-preserving u32 image of
 * a float32: -0 is taken as +0, a value with the sign bit set maps to ~bits,
 * any other to bits | 0x80000000.  lin is the C-order index inside the box; the
 * id of an edge is 3 * lin(its lower voxel) + axis (z 0, y 1, x 2).  Edges are
 * strictly ordered by the triple
 *     ( max(k(h_u), k(h_v)), min(k(h_u), k(h_v)), id ).
 * The result is the minimum spanning forest of the graph under that order with
 * all seeded voxels contracted into one root: take the edges in ascending
 * order and join the two sets unless they are one set already or both hold a
 * seed (Kruskal).  A voxel takes the label of the seeded voxel its tree hangs
 * from; a seeded voxel keeps its label; a voxel whose domain (the box, with
 * CTG_WS_2D its slice) holds no seed stays 0.
 * Every voxel so gets a label whose pass height -- the smallest, over the paths
 * to a seed, of the largest height on the path -- is minimal over all seeds.
 * vigra's priority flood with FIFO ties gives the same label wherever one
 * label alone attains that minimum, and may differ only where two labels tie
 * in it: there this rule splits by the lower end's height and then along
 * raster order, not by arrival time.
 * size_filter [UPSTREAM, unverified: elf's apply_size_filter restated]: after
 * the flood every label with fewer than size_filter voxels in a domain becomes
 * 0 there, its seeds included, and the flood runs again with the surviving
 * segments, whole, as seeds; where nothing survives the domain is all 0.
 *
 * Argument errors, found before any GPU work: a null hmap / seeds / shape /
 * out, a box outside the array, a box of more than 2^30 voxels (an edge id
 * must fit 32 bits), a bad seed_bits, flag or mem, an `out` that is the seeds
 * where that is not allowed: CTG_ERR_ARG.  An empty box writes nothing (info is
 * zeroed) and succeeds.  The call uses call-sized buffers only (20 bytes per
 * voxel): a CTG_DEFER_STATS handle of the same device stays valid across it.
 * ctg_last_timings of a profiled call, summed over the rounds and both floods:
 * [0] init, [1] pick and hook, [2] apply and chase, [3] size filter, [4] write,
 * [6] first launch to last.
 */
#define CTG_WS_2D 1
int ctg_seeded_watershed(const float* hmap, const void* seeds, int seed_bits, const int64_t* shape,
                         const int64_t* begin, const int64_t* end, int flags, uint64_t size_filter, uint64_t* out,
                         int mem, void* stream, uint64_t* info);

/* position of each query (u,v) in the sorted global edge table, -1 if absent */
int ctg_map_edge_ids(const uint64_t* global_edges, int64_t n_global,
                     const uint64_t* query, int64_t n_query, int64_t* out_ids,
                     int mem, void* stream);

/* result accessors; dst lives in host (CTG_MEM_HOST) or device memory */
int64_t ctg_result_num_edges(const ctg_result* r);
int64_t ctg_result_num_nodes(const ctg_result* r);
int ctg_result_copy_edges(const ctg_result* r, uint64_t* dst, int mem);
int ctg_result_copy_nodes(const ctg_result* r, uint64_t* dst, int mem);
int ctg_result_copy_features(const ctg_result* r, double* dst, int mem);
int ctg_result_copy_stats(const ctg_result* r, double* sums_dst, uint32_t* records_dst, int mem);
/* the (E,) uint64 voxel counts of an overlaps result (ctg_label_overlaps, ctg_merge_overlaps) */
int ctg_result_copy_counts(const ctg_result* r, uint64_t* dst, int mem);
/* device pointers for zero-copy consumers (valid until ctg_free) */
const uint64_t* ctg_result_device_edges(const ctg_result* r);
const double* ctg_result_device_features(const ctg_result* r);
int ctg_result_info(const ctg_result* r, int64_t* n_records, int64_t* n_direct);
void ctg_free(ctg_result* r);

/* deterministic synthetic volumes (Voronoi supervoxels + boundary map), device */
int ctg_synth_volume(uint64_t* labels, float* boundary, const int64_t* shape,
                     int64_t z_offset, const int64_t* global_shape, int cell,
                     uint64_t seed, uint64_t label_offset, double noise_amp, void* stream);
/* Filter-feature branch (features/block_edge_features.py:151-238): the
 * fastfilters / vigra filters vu.apply_filter runs (utils/volume_utils.py:80-94),
 * on device float32 arrays (cluster_tools_amd/fastfilters.py).
 * ctg_filter_conv_axis: out[p] = sum_k taps[k] in[reflect(p + (k - n_taps/2) e_axis)],
 *   C-order shape[ndim] (ndim <= 3), odd n_taps <= 257, mirror borders. */
int ctg_filter_conv_axis(const float* in, float* out, const int64_t* shape, int ndim, int axis, const float* taps,
                         int n_taps, void* stream);
/* op 0: sqrt(a^2+b^2+c^2), 1: a+b+c (b, c may be NULL), 2: a*b, 3: a-b; n elements */
int ctg_filter_combine(int op, const float* a, const float* b, const float* c, float* out, int64_t n, void* stream);
/* eigenvalues (descending) of n symmetric dim x dim matrices (dim 2 or 3), upper-triangle
 * components as planes comps[k*n + i]; out (n, dim) */
int ctg_sym_eigenvalues(const float* comps, int dim, int64_t n, float* out, void* stream);

int ctg_synth_affinities(const float* boundary, float* affs, const int64_t* shape,
                         int n_channels, const int32_t* offsets, void* stream);

/*
 * Native N5 / zarr chunk I/O (host memory; zlib + a thread pool).  The ndist
 * mirror reads the ROIs and writes the varlength chunks of the per-block path
 * through these (z5's role in the reference: graph/initial_sub_graphs.py:72-75,
 * features/block_edge_features.py:63-64, 236).
 *   format       CTG_IO_N5 | CTG_IO_ZARR_DOT (i.j.k keys) | CTG_IO_ZARR_SLASH
 *   big_endian   1: stored elements are big-endian (N5; zarr '>' dtypes)
 *   compression  CTG_IO_RAW | CTG_IO_GZIP (writes gzip streams: N5 {"type":"gzip"},
 *                zarr "gzip") | CTG_IO_ZLIB (writes zlib streams: N5 "useZlib":
 *                true, zarr "zlib"); reads auto-detect gzip and zlib for both
 */
#define CTG_IO_N5 0
#define CTG_IO_ZARR_DOT 1
#define CTG_IO_ZARR_SLASH 2
#define CTG_IO_RAW 0
#define CTG_IO_GZIP 1
#define CTG_IO_ZLIB 2
/* C-order box [begin, end) of a chunked dataset into `out`; missing chunks are
 * filled with the dtype_size-byte pattern fill_value (native byte order), or
 * zeros when fill_value is NULL */
int ctg_io_read_box(const char* ds_path, int format, int dtype_size, int big_endian, int ndim, const int64_t* shape,
                    const int64_t* chunks, int compression, const int64_t* begin, const int64_t* end, void* out,
                    int n_threads, const void* fill_value);
/* varlength N5 chunks at n_chunks grid positions: out[i] = malloc'ed native-
 * endian elements (free with ctg_io_free), n_out[i] = count, or NULL / -1 if
 * the chunk does not exist */
int ctg_io_read_varlen(const char* ds_path, int dtype_size, int ndim, int64_t n_chunks, const int64_t* positions,
                       int compression, void** out, int64_t* n_out, int n_threads);
void ctg_io_free(void* p);
/* drop the decoded-chunk cache of ctg_io_read_box (budget: env CTG_IO_CACHE_MB,
 * default 4096; an entry is reused only while its file keeps its inode, size,
 * mtime and ctime -- every writer here replaces chunk files by rename) */
void ctg_io_cache_clear(void);
/* cache counters since process start: out[0] chunk reads the cache served
 * (decoded, or in flight on the readahead pool), out[1] decodes on the
 * caller's threads, out[2] decodes by the readahead pool */
void ctg_io_cache_stats(int64_t* out);
/* drop the cached decodes of one chunk file (writers outside ctg_io call it) */
void ctg_io_cache_drop(const char* chunk_path);
/* write n_chunks chunks (default mode with chunk_shapes, or N5 varlength) */
int ctg_io_write_chunks(const char* ds_path, int format, int dtype_size, int big_endian, int ndim, int64_t n_chunks,
                        const int64_t* positions, const int64_t* chunk_shapes, const void* const* data,
                        const int64_t* n_elements, int varlen, int compression, int level, int n_threads);

/* release every device block the library caches on the current device
 * (workspace and allocator pool); result handles stay valid */
int ctg_trim(void);

/* profiling: per-phase device milliseconds of the last ctg_rag_features call
 * (HIP events on the call's stream): [0] face scan, [1] key pack, [2] sort,
 * [3] segment, [4] reduce+finalize, [5] nodes, [6] total; of a ctg_label_overlaps,
 * ctg_morphology or ctg_region_features call: [0] scan, [2] sort, [3] run heads + prefix sums,
 * [4] run sums / folds, [6] total; of a ctg_apply_assignment call: [0] = [6] the kernel */
int ctg_set_profiling(int on);
int ctg_last_timings(double* ms, int n);

/* Which way the last record sort of this thread's device went (the back half of
 * every scan call, of ctg_merge_stats and of the unique-pairs calls): the first
 * n (<= CTG_SORT_WORDS) of
 *   [CTG_SORT_PATH]     0 packed keys, bucket pass + segmented sort; 1 packed keys,
 *                       onesweep; 2 (key, index) pairs, bucket pass + segmented sort;
 *                       3 pairs, onesweep with wide digits; 4 pairs, onesweep with the
 *                       default digits; CTG_SORT_PATH_GROUP the group sort; -1 no record
 *   [CTG_SORT_PACKED]   the record slot rode in the sort key
 *   [CTG_SORT_GROUP_TRIED] the records were offered to the group sort,
 *   [CTG_SORT_GROUP_DONE]  which took them, or declined for
 *   [CTG_SORT_GROUP_WHY]   0 nothing (taken, or not offered), 1 no record or 2^32 and more,
 *                       2 more than 63 key bits, 3 bucket-local key and slot past 64 bits,
 *                       4 more than 32 key bits below the group bits (1 - 4: before any
 *                       launch), 5 a bucket above the LDS capacity
 *   [CTG_SORT_GROUP_SHIFT], [CTG_SORT_GROUP_BUCKETS] the group sort's bucket shift and
 *                       bucket count (-1, 0: it chose none)
 *   [CTG_SORT_GROUP_LARGEST] the largest bucket as read back (-1: not read)
 *   [CTG_SORT_IB], [CTG_SORT_NB], [CTG_SORT_UB] bits of the record slot, of the largest
 *                       label and of the key's u field
 *   [CTG_SORT_N]        records
 * Host values the call held anyway: no device read, no synchronisation. */
#define CTG_SORT_PATH 0
#define CTG_SORT_PACKED 1
#define CTG_SORT_GROUP_TRIED 2
#define CTG_SORT_GROUP_DONE 3
#define CTG_SORT_GROUP_WHY 4
#define CTG_SORT_GROUP_SHIFT 5
#define CTG_SORT_GROUP_BUCKETS 6
#define CTG_SORT_GROUP_LARGEST 7
#define CTG_SORT_IB 8
#define CTG_SORT_NB 9
#define CTG_SORT_UB 10
#define CTG_SORT_N 11
#define CTG_SORT_WORDS 12
#define CTG_SORT_PATH_GROUP 5
int ctg_last_sort(int64_t* out, int n);

/* Which plane loop the waves of the last face scan of this thread's device
 * took (ctg_rag_features; a ctg_rag_blocks call reports zeros): the first n
 * (<= CTG_SCAN_WORDS) of
 *   [CTG_SCAN_WAVES]          waves of the launch of wide tiles (0: no such launch)
 *   [CTG_SCAN_INTERIOR_WAVES] those of them whose columns, rows and planes, and the
 *                             neighbour above each, all lie in the owned box: they walk
 *                             their planes without ownership masks (0 with
 *                             CTG_SCAN_INTERIOR=0 in the environment, and for the
 *                             channel-loop kernels of affinity maps, which have one loop)
 *   [CTG_SCAN_NARROW_WAVES], [CTG_SCAN_NARROW_INTERIOR_WAVES] the same of the launch of
 *                             narrow tiles (boundary maps of fragmented volumes; where the
 *                             device picks the width, both launches are reported and one
 *                             of them exits at once)
 * Host values the call held anyway: no device read, no synchronisation. */
#define CTG_SCAN_WAVES 0
#define CTG_SCAN_INTERIOR_WAVES 1
#define CTG_SCAN_NARROW_WAVES 2
#define CTG_SCAN_NARROW_INTERIOR_WAVES 3
#define CTG_SCAN_WORDS 4
int ctg_last_scan(int64_t* out, int n);

/* bounds checks of CTG_DIAG builds (no reference counterpart: hardening): the
 * first index into a call-sized workspace buffer (records, sorted positions,
 * run tables, permutations, node bitmaps, exchange rows) that reached past
 * the current call's count since the last query.  Returns 0 (none) or 1 with
 * out[0] = source file (1 ctg_api, 2 ctg_scan, 3 ctg_sort, 4 ctg_reduce,
 * 5 ctg_mgpu, 6 ctg_overlap, 7 ctg_morph,
 * 8 ctg_region), out[1] = line, out[2] = index, out[3] = bound; clears them.
 * Product builds: CTG_ERR_UNSUPPORTED. */
int ctg_diag_bounds(uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* CTG_H_ */
