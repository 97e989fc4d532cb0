/*
 * ucoslam_hip.h — C ABI of the MI355X (gfx950) tracking hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Every entry point names the reference interface (file:line in lambdaloop/ucoslam-cv3)
 * whose work it replaces.  The C++ adaptors in include/ucoslam_hip/ mirror the
 * reference class surfaces on top of these calls; INTEGRATION.md shows the
 * reference-side binding.
 *
 * Conventions
 *   - every function returns 0 on success, a negative UH_E* code on failure;
 *     uh_last_error() returns a thread-local message for the last failure.
 *   - "_dev" entry points take DEVICE pointers, enqueue on the context stream
 *     and do not synchronise; the others take HOST pointers, copy in/out and
 *     return when results are in the caller's buffers.
 *   - there is NO CPU fallback: without a usable HIP device every call fails
 *     with UH_ENODEVICE.
 */
#ifndef UCOSLAM_HIP_H
#define UCOSLAM_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UH_OK          0
#define UH_EINVAL     -1   /* bad argument (the reference throws std::runtime_error here) */
#define UH_ENODEVICE  -2   /* no HIP device / HIP runtime failure */
#define UH_ENOTBUILT  -3   /* index/vocabulary not built (reference: search() returns false) */
#define UH_ENOMEM     -4
#define UH_ECAPACITY  -5   /* caller's output buffer too small */

typedef struct uh_ctx uh_ctx;

/* Context = one GPU + one HIP stream (+ scratch owned by the stage objects).
 * hip_stream is a hipStream_t; NULL means the device's default (null) stream, which is also
 * what torch.cuda.current_stream().cuda_stream is (0) unless a side stream is current.
 * uh_ctx_create_private() creates and owns a non-blocking stream instead. */
int         uh_ctx_create(int device, void* hip_stream, uh_ctx** out);
int         uh_ctx_create_private(int device, uh_ctx** out);
/* A private stream confined to a share of the GPU's compute units: mask bits [first_bit, first_bit + n_bits) of
 * hipExtStreamCreateWithCUMask — on MI355X bit p is CU p / 8 of XCD p % 8, so a contiguous range takes the same number of CUs from every
 * XCD.  For hosts that run the mapper's local BA (latency-bound, <= 94 workgroups) beside the tracker's wide launches, as the reference
 * runs them on two threads (system.cpp / mapmanager.cpp:150): disjoint ranges keep the two from sharing a CU. */
int         uh_ctx_create_private_cus(int device, int first_bit, int n_bits, uh_ctx** out);
void        uh_ctx_destroy(uh_ctx* ctx);
int         uh_ctx_synchronize(uh_ctx* ctx);
void*       uh_ctx_stream(uh_ctx* ctx);
/* pinned host memory for the buffers handed to the host-pointer entry points (asynchronous DMA instead of staged copies) */
void*       uh_host_alloc(size_t bytes);
void        uh_host_free(void* p);
const char* uh_last_error(void);
/* Per-kernel timing for measurement (bench.py roofline leg): when enabled every kernel launch of the stage objects
 * bound to this context is bracketed by HIP events on the context stream.  report: "<kernel> <calls> <total_ms>\n" lines. */
int         uh_prof_enable(uh_ctx* ctx, int on);
int         uh_prof_reset(uh_ctx* ctx);
int         uh_prof_report(uh_ctx* ctx, char* buf, size_t cap);
/* library/ABI version: major*10000 + minor*100 + patch */
int         uh_version(void);

/* ------------------------------------------------------------------------
 * Hamming brute-force kNN  — replaces xflann::Index (Linear) build/search:
 *   3rdparty/xflann/xflann/index.cpp:45 (build), :77-103 (search + sort),
 *   impl/linear.h:68-86 (_knnsearch<Hamming_x64_32bytes>), impl/resultset.h:64-135
 *   (max-heap ResultSet), index.h:119-134 (exchange sort).
 * Results are bit-identical to the reference INCLUDING the heap array order of
 * unsorted rows and the order of equal distances in sorted rows.
 * Unfilled slots (nt < nn): index -1, distance 0   (linear.h:82-85).
 * ------------------------------------------------------------------------ */
typedef struct uh_knn uh_knn;

int  uh_knn_create(uh_ctx* ctx, uh_knn** out);
void uh_knn_destroy(uh_knn* idx);

/* build: train = nt rows of desc_bytes (must be 32 = ORB) bytes, row stride in bytes.
 * Host pointer; the rows are copied to HBM (reference LinearParams(store_data=1)). */
int uh_knn_build(uh_knn* idx, const uint8_t* train, int nt, size_t stride, int desc_bytes);
/* build from rows already resident in HBM (contiguous nt x 32, 16-byte aligned); not copied. */
int uh_knn_build_dev(uh_knn* idx, const uint8_t* d_train, int nt);
/* restrict the scan to train rows [begin,end) (multi-GPU sharding of the train set);
 * indices stay global.  Default = [0,nt). */
int uh_knn_set_shard(uh_knn* idx, int begin, int end);
int uh_knn_size(const uh_knn* idx);
/* Exact search: how many queries one wave serves (1 = default, 2, 4; rows with nn > 15 always use 1).  Results are identical.  With
 * more queries per wave the search itself takes longer (8000 x 10 000 x nn=10: 163 / 185 / 250 us) but moves 1/2 or 1/4 of the
 * L1/L2 traffic and keeps 1/2 or 1/4 of the waves resident — the setting for a matcher that runs beside latency-bound work on
 * another stream (next to the local BA the whole tracking step is 6 % faster at 4). */
int  uh_knn_set_queries_per_wave(uh_knn* index, int queries_per_wave);

/* search: queries nq x 32 (row stride q_stride bytes), outputs nq x nn int32 row-major.
 * sorted: 0/1 as KnnSearchParams(maxChecks,sorted); max_dist: -1 = kNN, >=0 = radius bound
 * (SearchParams maxDist, resultset.h:66). */
int uh_knn_search(uh_knn* idx, const uint8_t* queries, int nq, size_t q_stride, int nn,
                  int32_t* indices, int32_t* distances, int sorted, int max_dist);
int uh_knn_search_dev(uh_knn* idx, const uint8_t* d_queries, int nq, int nn,
                      int32_t* d_indices, int32_t* d_distances, int sorted, int max_dist);

/* Hierarchical k-means form of the index — xflann::Index::build(features, HKMeansParams(k, maxIters)) (index.cpp:52-57,
 * impl/kmeansindexcreator.{h,cpp}) and search(..., KnnSearchParams(maxChecks, sorted)) through KMeansIndex::_knnsearch_nn
 * (impl/kmeansindex.h:356-410): the APPROXIMATE index FrameMatcher_Flann builds per train frame (framematcher.cpp:213 k=32,
 * maxIters=0; :239 nn=10, maxChecks=16, unsorted).  Results are bit-identical to the reference: same tree (std::shuffle of a
 * default std::mt19937 picks the centres), same best-bin-first order, same ResultSet rows; unfilled slots index -1, distance 0.
 * build: host pointer, contiguous n x 32 bytes; 2 <= k <= 64; maxIters as HKMeansParams (0 = the matcher's setting, -1 = until
 * convergence; rounds move the centres to the bitwise majority of their clusters).  More than k identical descriptors make
 * the reference recurse without end: reported as UH_EINVAL.  uh_knn_kmeans_blob exposes the block data in the reference's own
 * serialised layout (the bytes KMeansIndex::toStream writes after its 48-byte header).
 * search: maxChecks as the reference (<= 0 returns empty rows, like the reference's loop condition); the pairs (nn=1,maxChecks=1)
 * and (nn=2,maxChecks<=2) select the reference's greedy descents (kmeansindex.h:226-352), which are defective for binary
 * descriptors — their int32 "best distance" is initialised with uint32 max = -1, so no child ever compares smaller and every
 * query returns the same row with distance -1 (observed on the real library) — and are refused here with UH_EINVAL. */
int uh_knn_build_kmeans(uh_knn* idx, const uint8_t* features, int n, int k, int max_iters);
int uh_knn_kmeans_blob(uh_knn* idx, const uint8_t** data, uint64_t* size);
/* host-only build (test hook, no GPU): writes min(cap, size) bytes of the block data to out, the full size to *size */
int uh_knn_kmeans_build_host(const uint8_t* features, int n, int k, int max_iters, uint8_t* out, uint64_t cap, uint64_t* size);
int uh_knn_search_kmeans(uh_knn* idx, const uint8_t* queries, int nq, int nn, int max_checks, int sorted,
                         int32_t* indices, int32_t* distances);
int uh_knn_search_kmeans_dev(uh_knn* idx, const uint8_t* d_queries, int nq, int nn, int max_checks, int sorted,
                             int32_t* d_indices, int32_t* d_distances);

/* Sharded search (multi-GPU): phase 1 emits, per query, the candidates the local
 * heap ACCEPTED while scanning this shard, in train-index order (a superset of what
 * the global heap accepts).  cand = nq x cap entries, each (dist<<32 | global index);
 * counts = nq int32 (count > cap means overflow: that row must be rescanned).
 * Phase 2 replays the concatenation of all shards' candidate lists (in shard order)
 * through the exact ResultSet semantics.  lists: nshards blocks of [nq x cap],
 * counts: nshards blocks of [nq]. */
int uh_knn_scan_shard_dev(uh_knn* idx, const uint8_t* d_queries, int nq, int nn, int max_dist,
                          uint64_t* d_cand, int32_t* d_counts, int cap);
/* Query rows [*d_valid_rows, nq) of every following uh_knn_scan_shard_dev are not scanned and emit EMPTY lists (NULL: all rows count).
 * For a caller whose query buffer is a fixed-capacity frame block of which only the first `count` rows — a number that lives on the
 * device — are this frame's descriptors (FrameExtractor's output, frameextractor.cpp:270-340, fed to the sharded matcher): rows left
 * over from an earlier frame must not be able to overflow a list. */
int uh_knn_set_valid_rows_dev(uh_knn* idx, const int32_t* d_valid_rows);
int uh_knn_replay_dev(uh_knn* idx, const uint8_t* d_queries, int nq, int nn, int sorted, int max_dist,
                      const uint64_t* d_cand_all, const int32_t* d_counts_all, int nshards, int cap,
                      int32_t* d_indices, int32_t* d_distances);
/* Ranks that hold ONLY their tile of a sharded train set ("each GPU emits local top-k per query with GLOBAL train
 * indices"): the index is built over the tile's rows, uh_knn_set_row_offset gives row 0's global index (used by
 * uh_knn_scan_shard_dev), and uh_knn_replay_tiles_dev replays the gathered lists without ever touching train rows — a list
 * that overflowed its cap sets *d_overflow (device int32, zeroed by the caller) instead of being rescanned. */
/* xflann::Index::toStream / fromStream (index.cpp:153-188) for the hierarchical k-means index: 8-byte signature 12837333433, 8-byte
 * std::hash<std::string>("kmeans"), then KMeansIndex::toStream (kmeansindex.cpp:209-216) = signature 55824124 + 40-byte params + block
 * data.  Byte-identical to what the real library writes for the same features (tests/golden/hkmeans_stream_golden.npz); a stream
 * written by the real library loads and searches identically.  Linear has no stream form in the reference ("Not yet", linear.cpp:78). */
int uh_knn_to_stream(uh_knn* idx, uint8_t* out, uint64_t cap, uint64_t* size);
int uh_knn_from_stream(uh_knn* idx, const uint8_t* data, uint64_t nbytes);
int uh_knn_set_row_offset(uh_knn* idx, int offset);
int uh_knn_replay_tiles_dev(uh_knn* idx, const uint8_t* d_queries, int nq, int nn, int sorted, int max_dist,
                            const uint64_t* d_cand_all, const int32_t* d_counts_all, int nshards, int cap,
                            int32_t* d_indices, int32_t* d_distances, int32_t* d_overflow);
/* ... on lists that still sit inside gathered messages: shard s's blocks begin cand_stride (uint64 elements) / count_stride (int32
 * elements) behind shard s-1's — what uh_fstream_finish_dev uses, nothing is unpacked before the replay */
int uh_knn_replay_tiles_strided_dev(uh_knn* idx, const uint8_t* d_queries, int nq, int nn, int sorted, int max_dist,
                                    const uint64_t* d_cand_all, size_t cand_stride, const int32_t* d_counts_all, size_t count_stride,
                                    int nshards, int cap, int32_t* d_indices, int32_t* d_distances, int32_t* d_overflow);

/* ------------------------------------------------------------------------
 * ORB extractor — replaces ucoslam::ORBextractor behind Feature2DSerializable:
 *   src/featureextractors/feature2dserializable.h:30-95 (plugin surface, FeatParams :34-60)
 *   src/featureextractors/ORBextractor.cpp:1139 detectAndCompute_impl -> :1247-1353 compute
 * Output is layout-compatible with what the reference hands back:
 *   uh_keypoint == cv::KeyPoint (7 x 4 bytes, ORBextractor.cpp:1297 memcpy), descriptors N x 32 CV_8U.
 * Keypoints come in level order, within a level in the reference's cell-row-major /
 * retainBest-permuted order.
 * ------------------------------------------------------------------------ */
typedef struct uh_orb uh_orb;

typedef struct uh_keypoint {       /* cv::KeyPoint */
    float x, y;                    /* pt, level-0 coordinates */
    float size;                    /* 31 * scale[octave], truncated to int (ORBextractor.cpp:1046) */
    float angle;                   /* degrees [0,360), cv::fastAtan2 of the intensity centroid */
    float response;                /* FAST-9/16 corner score */
    int32_t octave;
    int32_t class_id;              /* -1 */
} uh_keypoint;

typedef struct uh_feat_params {    /* Feature2DSerializable::FeatParams (feature2dserializable.h:34-60) */
    int32_t nthreads;              /* accepted for interface parity; the GPU path ignores it */
    int32_t maxFeatures;           /* default 4000 */
    int32_t nOctaveLevels;         /* default 8 */
    float   scaleFactor;           /* default 1.2 */
    float   sensitivity;           /* default 0 */
} uh_feat_params;

int  uh_orb_create(uh_ctx* ctx, uh_orb** out);
void uh_orb_destroy(uh_orb* orb);
/* detectAndCompute_impl re-runs precalculateParams when params change (:1142-1145); thresholds reset to 20/7 */
int  uh_orb_set_params(uh_orb* orb, const uh_feat_params* params);
int  uh_orb_get_params(const uh_orb* orb, uh_feat_params* params);
/* Feature2DSerializable::toStream / fromStream (feature2dserializable.cpp:76-113) + ORBextractor::toStream_impl / fromStream_impl
 * (ORBextractor.cpp:417-423): u64 signature 1828374733, u64 type tag (F2D_ORB = 0), parameter string (u32 length + bytes), raw FeatParams.
 * to_stream with out == NULL only reports *size.  from_stream fails with the reference's message on a wrong signature and refuses
 * the grid-extractor type tags. */
int  uh_orb_to_stream(const uh_orb* orb, const char* str_params, uint8_t* out, uint64_t cap, uint64_t* size);
int  uh_orb_from_stream(uh_orb* orb, const uint8_t* data, uint64_t nbytes, char* str_params_out, uint64_t str_cap, uint64_t* consumed);
/* FrameExtractor::toStream / fromStream (src/utils/frameextractor.cpp:651-884 / :886-1136, signature 1923123): the extractor block of a
 * reference `.slm` checkpoint — the Feature2DSerializable stream above, the frame counter, three flags, marker size, the FeatParams in
 * use, maxDescDistance, then the aruco::MarkerDetector stream (3rdparty/aruco/aruco/markerdetector.cpp:256-277, behind u64 13213) and the
 * ucoslam::Params stream (src/ucoslamtypes.cpp:63-121).  The two trailing sub-streams belong to subsystems that stay with the host:
 * fromStream walks them and reports where they lie (offsets / lengths into `data`), toStream writes the bytes it is given verbatim or,
 * with NULL, what the reference's default-constructed objects write.  The HIP extractor detects no markers: detect_markers = 1 needs
 * the host's own detector stream on writing and allow_markers on reading, and is refused otherwise. */
typedef struct uh_frame_extractor_state {
    uint32_t counter;               /* frames processed so far */
    uint8_t  remove_from_markers, detect_markers, detect_keypoints;
    float    marker_size;           /* Params::aruco_markerSize */
    uh_feat_params feat_params;     /* the FeatParams the extractor is run with */
    float    max_desc_distance;     /* Params::maxDescDistance */
} uh_frame_extractor_state;
int  uh_frame_extractor_to_stream(const uh_orb* orb, const char* str_params, const uh_frame_extractor_state* state, const uint8_t* aruco_stream,
                                  uint64_t aruco_bytes, const uint8_t* params_stream, uint64_t params_bytes, uint8_t* out, uint64_t cap, uint64_t* size);
int  uh_frame_extractor_from_stream(uh_orb* orb, const uint8_t* data, uint64_t nbytes, int allow_markers, uh_frame_extractor_state* state,
                                    char* str_params_out, uint64_t str_cap, uint64_t* aruco_off, uint64_t* aruco_bytes, uint64_t* params_off,
                                    uint64_t* params_bytes, uint64_t* consumed);
/* ucoslam::Params as a stream carries it (src/ucoslamtypes.cpp:63-121 toStream, :123-180 fromStream: u64 9837138769928 ... u64 1837138769921):
 * the members the hot path and its host glue are driven by, parsed; the ArUco members are walked over.  Errors carry the reference's
 * messages ("Invalid signature", "Reached EOF without finding end signature"). */
typedef struct uh_params_view {
    uint8_t detect_markers, detect_keypoints, kp_non_maxima_suppression, force_initialization_from_markers, remove_keypoints_into_markers,
            run_sequential, auto_adjust_kp_sensitivity, relocalization_with_keypoints, relocalization_with_markers;
    int8_t  kp_descriptor_type;             /* DescriptorTypes::Type (int8): 1 = DESC_ORB */
    float   target_focus, kf_min_confidence, max_desc_distance, baseline_median_depth_ratio_min, aruco_marker_size, kf_culling, th_ref_ratio,
            scale_factor, min_base_line, kpt_image_scale_factor;
    int32_t max_new_points, proj_dist_thr, nthreads_feature_detector, max_visible_frames_per_marker, min_num_proj_points, max_features, n_octave_levels;
    char    global_optimizer[32];           /* "g2o" */
} uh_params_view;
int uh_params_from_stream(const uint8_t* data, uint64_t nbytes, uh_params_view* out, uint64_t* consumed);

/* System::saveToFile / readFromFile (src/utils/system.cpp:8099-8720), the `.slm` checkpoint:
 *   u64 182312 | Map | Params | se3 pose (6 x f32) | i64 current keyframe | bool initialised | STATE i32 | MODES i32 | Frame current |
 *   Frame previous | FrameExtractor | MapManager | cv::Mat (i32 rows, cols, type + data) | i64 | u64
 * The hot path owns Params and the FrameExtractor block; Map / Frame / MapManager are the host's containers
 * and carry no length — only their own readers know where they end.  Reading is therefore sectioned:
 *   uh_system_stream_begin   checks the signature, says where the Map block starts (8)
 *   [host: Map::fromStream]
 *   uh_system_stream_state   on the bytes behind the Map: Params + the five state members; *consumed = where the current Frame starts
 *   [host: Frame::fromStream x 2]
 *   uh_frame_extractor_from_stream
 *   [host: MapManager::fromStream]
 *   uh_system_stream_tail    the cv::Mat header (its data stays in place: offset / length) and the two trailing integers
 * and uh_system_to_stream composes a checkpoint from the host's blocks (opaque bytes; a missing one is refused by name), the extractor
 * block of uh_frame_extractor_to_stream and the values below.  params == NULL writes the Params block the extractor block ends with. */
typedef struct uh_system_state {
    float   cur_pose_rt[6];                 /* se3: rx ry rz tx ty tz (NaN = invalid) */
    int64_t current_keyframe;               /* -1 = none */
    uint8_t is_initialized;
    int32_t state;                          /* STATE_TRACKING = 0, STATE_LOST = 1 */
    int32_t mode;                           /* MODE_SLAM = 0, MODE_LOCALIZATION = 1 */
} uh_system_state;
typedef struct uh_system_tail {
    int32_t  mat_rows, mat_cols, mat_type;  /* cv::Mat header (io_utils.cpp:21-37); rows x cols == 0: no data */
    uint64_t mat_data_offset, mat_data_bytes;   /* (reader) where the matrix data lies behind `data` */
    int64_t  last_value_i64;                /* System's trailing int64 member (-1 by default) */
    uint64_t last_value_u64;                /* System's trailing uint64 member (0 by default) */
} uh_system_tail;
typedef struct uh_system_parts {
    const uint8_t* map;         uint64_t map_bytes;          /* host: Map::toStream */
    const uint8_t* params;      uint64_t params_bytes;       /* Params::toStream bytes, or NULL */
    uh_system_state state;
    const uint8_t* cur_frame;   uint64_t cur_frame_bytes;    /* host: Frame::toStream */
    const uint8_t* prev_frame;  uint64_t prev_frame_bytes;
    const uint8_t* extractor;   uint64_t extractor_bytes;    /* uh_frame_extractor_to_stream */
    const uint8_t* map_manager; uint64_t map_manager_bytes;  /* host: MapManager::toStream */
    uh_system_tail tail;        const uint8_t* mat_data;
} uh_system_parts;
int uh_system_stream_begin(const uint8_t* data, uint64_t nbytes, uint64_t* map_offset);
int uh_system_stream_state(const uint8_t* data, uint64_t nbytes, uh_params_view* params, uh_system_state* state, uint64_t* params_bytes, uint64_t* consumed);
int uh_system_stream_tail(const uint8_t* data, uint64_t nbytes, uh_system_tail* tail, uint64_t* consumed);
int uh_system_to_stream(const uh_system_parts* parts, uint8_t* out, uint64_t cap, uint64_t* size);
int  uh_orb_set_blur(uh_orb* orb, int do_blur);            /* ORBextractor::doGaussianBlur() (ORBextractor.h:112) */
int  uh_orb_set_sensitivity(uh_orb* orb, float v);         /* ORBextractor::setSensitivity (ORBextractor.cpp:457-466) */
int  uh_orb_set_nonmaxima(uh_orb* orb, int on);            /* debug string "orb_nonmaxima" (ORBextractor.cpp:1146-1148,1176-1205): radius-3
                                                              suppression per level before the descriptors; kept keypoints get class_id 1 */
/* Multi-GPU extraction of one frame ("pyramid levels sharded"): this instance extracts pyramid levels
 * [first_level, end_level) only (end_level < 0: to the last level).  Per-level budgets, thresholds and cell grids stay those
 * of the full level count (ORBextractor.cpp:501-513 fixes them per level), the resize chain is built redundantly up to
 * end_level-1 (level l reads level l-1, :1379), so the shards' outputs concatenated in level order are the full extraction's
 * rows, bit for bit.  An empty range yields zero keypoints. */
int  uh_orb_set_level_range(uh_orb* orb, int first_level, int end_level);
int  uh_orb_max_keypoints(const uh_orb* orb);              /* = maxFeatures: upper bound of *n_out */

/* One frame, host buffers: img = h rows of w bytes (CV_8UC1), row stride in bytes.
 * kps/desc must hold `cap` entries; *n_out receives the keypoint count (UH_ECAPACITY if n > cap).
 * An empty image (NULL / w<=0 / h<=0) returns 0 keypoints silently (ORBextractor.cpp:1254). */
int uh_orb_extract(uh_orb* orb, const uint8_t* img, int w, int h, size_t stride,
                   uh_keypoint* kps, uint8_t* desc, int cap, int* n_out);
/* The frame as the camera delivers it and the keypoints as Frame stores them — the two per-frame steps FrameExtractor performs around the
 * extractor (src/utils/frameextractor.cpp:2960,3046 cv::cvtColor(COLOR_BGR2GRAY) for three-channel input; :3985 undistortPoints(kpts,
 * ImageParams) = src/basictypes/misc.cpp:269-293: cv::undistortPoints, then x*fx + cx in float) done on the device inside the same launches:
 *   channels  1 (CV_8UC1), 3 (BGR) or 4 (BGRA) interleaved bytes per pixel, row stride in bytes
 *   und_xy    NULL, or cap x 2 floats receiving Frame::und_kpts[i].pt for every returned keypoint (needs uh_orb_set_camera)
 * uh_orb_set_camera: ImageParams' CameraMatrix (CV_32F) and Distorsion (k1 k2 p1 p2 [k3 [k4 k5 k6]], n_dist of them; 0 = none: the result is
 * still the float round trip (x - cx)/fx*fx + cx of the reference, not the input).  NULL switches the camera off.
 * uh_undistort_points_host: the same arithmetic on the host (no GPU) for n points. */
typedef struct uh_camera { float fx, fy, cx, cy; float dist[8]; int32_t n_dist; } uh_camera;
int uh_orb_set_camera(uh_orb* orb, const uh_camera* cam);
int uh_orb_extract_frame(uh_orb* orb, const uint8_t* img, int w, int h, size_t stride, int channels,
                         uh_keypoint* kps, uint8_t* desc, float* und_xy, int cap, int* n_out);
int uh_undistort_points_host(const uh_camera* cam, const float* xy, int n, float* out_xy);
/* The Frame that FrameExtractor::process produces, kept ON THE DEVICE for the tracker (src/utils/frameextractor.cpp:430-520 detectAndCompute,
 * :3985 undistortPoints, :4258 Frame::create_kdtree -> src/basictypes/picoflann.h:150-163,238-345): uh_orb_extract_frame_dev is
 * uh_orb_extract_frame (same host outputs, same completion) that also leaves the descriptors and the undistorted keypoints in `frame`
 * (HBM) and enqueues ONE more launch behind its completion word which builds picoflann's kd-tree there, node for node what the reference
 * builds on the CPU (up to 4096 keypoints; needs uh_orb_set_camera).  uh_projmatch_set_frame_dev adopts such a frame: nothing goes
 * device -> host -> device, no tree is built on the host.  A frame object is overwritten by the next extraction into it: keep two to
 * hold the previous frame.  uh_dev_frame_tree (inspection / tests) waits for the build and copies the tree out: nodes24_out as in
 * uh_projmatch_debug_tree with room for 2n/5 + 2 nodes, leaf_idx_out / leaf_octave_out n entries, leaf_xy_out 2n floats (any may be NULL). */
typedef struct uh_dev_frame uh_dev_frame;
int  uh_dev_frame_create(uh_ctx* ctx, uh_dev_frame** out);
void uh_dev_frame_destroy(uh_dev_frame* frame);
/* Who builds the kd-tree of a device frame.  on_host = 0 (default): the build launches behind the extraction (the host does nothing but wait).
 * on_host = 1: no build launch; uh_projmatch_set_frame_dev builds the tree on the calling core from the host copy of the undistorted keypoints
 * (frame->und_kpts / n_kpts of its uh_proj_frame argument, exactly the arrays uh_orb_extract_frame_dev returned) and uploads nodes and leaf records
 * into the frame object — the descriptors still never cross the host link a second time.  Same tree, byte for byte; the faster route while a
 * core is free (Frame::create_kdtree, frameextractor.cpp:4258). */
int  uh_dev_frame_set_tree_builder(uh_dev_frame* frame, int32_t on_host);
/* a frame that was not extracted here (read from a file, made by another extractor) into a device frame object: n undistorted keypoints (x, y, octave
 * are used) and their n x 32 descriptor bytes; the tree is built as for an extracted frame.  Synchronous — a utility, not the per-frame path. */
int  uh_dev_frame_upload(uh_dev_frame* frame, const uh_keypoint* und_kpts, int32_t n, const uint8_t* desc);
int  uh_orb_extract_frame_dev(uh_orb* orb, const uint8_t* img, int w, int h, size_t stride, int channels,
                              uh_keypoint* kps, uint8_t* desc, float* und_xy, int cap, int* n_out, uh_dev_frame* frame);
/* the same call in two halves: _begin returns as soon as the undistorted keypoints — x, y, octave; the other fields come with _end — are on the host
 * (*und_kpts_early: this object's array, valid until the next extraction), so that the caller builds the kd-tree (uh_projmatch_set_frame_dev with
 * uh_dev_frame_set_tree_builder(frame, 1)) while the descriptors are still being computed; _end completes kps / desc / und_xy.  No other
 * extraction on this object in between. */
int  uh_orb_extract_frame_dev_begin(uh_orb* orb, const uint8_t* img, int w, int h, size_t stride, int channels,
                                    uh_keypoint* kps, uint8_t* desc, float* und_xy, int cap, int* n_out, uh_dev_frame* frame, const uh_keypoint** und_kpts_early);
int  uh_orb_extract_frame_dev_end(uh_orb* orb, int* n_out);
int  uh_dev_frame_tree(uh_dev_frame* frame, int32_t* n_kpts, int32_t* n_nodes, void* nodes24_out, uint32_t* leaf_idx_out, float* leaf_xy_out,
                       int32_t* leaf_octave_out, double* root_box4, int32_t* max_depth);
/* `batch` frames resident in HBM (frame f at d_imgs + f*frame_stride); outputs per frame at
 * d_kps + f*cap_per_frame, d_desc + f*cap_per_frame*32, d_counts[f].  Asynchronous on the context stream. */
int uh_orb_extract_dev(uh_orb* orb, const uint8_t* d_imgs, int w, int h, size_t stride, size_t frame_stride,
                       int batch, uh_keypoint* d_kps, uint8_t* d_desc, int cap_per_frame, int32_t* d_counts);
/* The same for `batch` frames in HOST memory, results to host memory (fixed-capacity blocks: frame f's rows at kps + f*cap, desc + f*cap*32,
 * counts[f] of them valid; cap >= maxFeatures): one H2D copy, the batched launch set, three D2H copies, one synchronisation. */
int uh_orb_extract_batch(uh_orb* orb, const uint8_t* imgs, int w, int h, size_t stride, size_t frame_stride, int batch,
                         uh_keypoint* kps, uint8_t* desc, int cap, int32_t* counts);
/* Verification tap: copy level `level` of frame `frame` (which: 0 pyramid, 1 FAST strength map) to `out`
 * (w*h bytes, may be NULL to query the size). */
int uh_orb_debug_level(uh_orb* orb, int frame, int level, int which, uint8_t* out, int* w_out, int* h_out);

/* ------------------------------------------------------------------------
 * Stereo / RGB-D frames: Frame::depth per keypoint — FrameExtractor::processStereo and process_rgbd (src/utils/frameextractor.cpp from
 * :1419) for kptImageScaleFactor == 1 (the resize branch is not built: a host that sets another factor keeps the reference's extractor).
 * Per left keypoint i (depth[i] = 0 unless every step succeeds):
 *   row    r = int(std::round(und.y)); candidates = the right keypoints j with int(std::round(pt.y)) == r (a right keypoint whose rounded
 *          row is outside the image is in no row), skipping right.pt.x > left.und.x and |octave difference| > 1
 *   match  smallest 256-bit Hamming distance d with float(d) < max_desc_dist; among equals the lowest j
 *   SAD    6 x 6 windows (cv::Range(c-3, c+3)) of the UNBLURRED gray images around the rounded centres (both must satisfy 3 <= c, c+3 < size),
 *          the right one shifted by -7 .. 7; first smallest sum of absolute differences
 *   depth  only if that minimum is strictly inside the evaluated offsets: parabola through the three costs (double), xr = right.pt.x + delta,
 *          depth = float(double(bl * fx) / (double(und.x) - xr)) with bl * fx a float product.  Negative / infinite values are kept.
 * Bit for bit the reference's result, with two deviations where the reference reads out of bounds or throws: a left row outside
 * [0, rows) has no candidates (the reference indexes a std::vector unchecked), and the offsets stop where the shifted window still lies
 * inside the image (the reference throws cv::Exception there; ORB keypoints keep 16 px from the border, so neither occurs in its own use).
 *
 * uh_stereo_depth: the operator on caller-supplied HOST arrays (uploads, three launches, one wait).  Keypoints are cv::KeyPoint records: pt and
 * octave are read.  depth_out: n_left floats; match_out: NULL, or n_left ints receiving the matched right index or -1.
 * uh_stereo_depth_dev: every pointer (images, keypoints, descriptors, outputs) is device memory, descriptors 16-byte aligned; asynchronous on
 * the context stream.  uh_stereo_depth_host: the same result from the same arithmetic on the CPU, no GPU involved.
 * ------------------------------------------------------------------------ */
typedef struct uh_stereo_args {
    const uint8_t* left;  size_t left_stride;      /* CV_8UC1, rows x cols, row stride in bytes */
    const uint8_t* right; size_t right_stride;
    int32_t cols, rows;                            /* of the left image */
    int32_t right_cols, right_rows;                /* must equal cols, rows */
    int32_t n_left;  const uh_keypoint* left_und_kpts; const uint8_t* left_desc;    /* Frame::und_kpts, Frame::desc (n x 32) */
    int32_t n_right; const uh_keypoint* right_kpts;    const uint8_t* right_desc;   /* detectAndCompute of the right image */
    float bl, fx;                                  /* ImageParams::bl (> 0), fx() */
    float max_desc_dist;                           /* Params::maxDescDistance */
} uh_stereo_args;
int uh_stereo_depth(uh_ctx* ctx, const uh_stereo_args* args, float* depth_out, int32_t* match_out);
int uh_stereo_depth_dev(uh_ctx* ctx, const uh_stereo_args* args, float* d_depth_out, int32_t* d_match_out);
int uh_stereo_depth_host(const uh_stereo_args* args, float* depth_out, int32_t* match_out);
/* process_rgbd's gather alone: depth[i] = float(D(cvRound(kpts[i].pt))) * depth_scale where that pixel is non-zero, else 0 (kpts = the
 * DISTORTED keypoints; a pixel outside the depth image gives 0 where the reference reads unchecked).  depth_stride in bytes (even). */
int uh_rgbd_depth(uh_ctx* ctx, const uh_keypoint* kpts, int32_t n, const uint16_t* depth_img, int32_t cols, int32_t rows, size_t depth_stride,
                  float depth_scale, float* depth_out);
int uh_rgbd_depth_host(const uh_keypoint* kpts, int32_t n, const uint16_t* depth_img, int32_t cols, int32_t rows, size_t depth_stride,
                       float depth_scale, float* depth_out);

/* FrameExtractor::processStereo in one call: gray conversion and extraction of both images, then the three stereo launches, one wait.
 * Needs uh_orb_set_camera (fx, und_kpts) and uh_orb_set_stereo (bl > 0, max_desc_dist).  Left outputs (kps, desc, und_xy, *n_out, and
 * `frame` if not NULL) are exactly uh_orb_extract_frame / uh_orb_extract_frame_dev of the left image; depth receives *n_out floats (room
 * for cap).  right_out (NULL, or for inspection): the right image's keypoints / descriptors / count, exactly uh_orb_extract of the right
 * gray image; kps / desc hold uh_orb_max_keypoints entries.  Both images are w x h with the same channel count and row stride (bytes). */
typedef struct uh_stereo_right { uh_keypoint* kps; uint8_t* desc; int32_t n; } uh_stereo_right;
int uh_orb_set_stereo(uh_orb* orb, float bl, float max_desc_dist);
int uh_orb_extract_stereo(uh_orb* orb, const uint8_t* left, const uint8_t* right, int w, int h, size_t stride, int channels,
                          uh_keypoint* kps, uint8_t* desc, float* und_xy, float* depth, int cap, int* n_out, uh_dev_frame* frame,
                          uh_stereo_right* right_out);
/* FrameExtractor::process_rgbd in one call: uh_orb_extract_frame (uh_orb_extract_frame_dev when `frame` is not NULL) plus the depth gather
 * behind it on the device, one wait.  depth_img: h rows of w uint16, depth_stride in bytes; depth_scale = ImageParams::rgb_depthscale. */
int uh_orb_extract_rgbd(uh_orb* orb, const uint8_t* img, int w, int h, size_t stride, int channels, const uint16_t* depth_img, size_t depth_stride,
                        float depth_scale, uh_keypoint* kps, uint8_t* desc, float* und_xy, float* depth, int cap, int* n_out, uh_dev_frame* frame);

/* ------------------------------------------------------------------------
 * Bundle adjustment — replaces GlobalOptimizerG2O behind the GlobalOptimizer plugin:
 *   src/optimization/globaloptimizer.h:28-68       setParams / optimize(bool* stopASAP) / getResults
 *   src/optimization/globaloptimizer_g2o.cpp:77-401 (graph build), :418-464 (two-pass LM), :466-537 (results)
 *   3rdparty/g2o: Levenberg + BlockSolver_6_3 (Schur) + LinearSolverEigen (LDLT) + Huber
 * The caller flattens the map exactly as setParams does (INTEGRATION.md shows the adaptor):
 *   frames  : pose_f2g as the reference stores it (row-major 4x4 float, cv::Mat CV_32F), fixed flag
 *             (FIXED_WITHPOINTS / FIXED_WITHOUTPOINTS both = 1), intrinsics fx fy cx cy
 *   points  : float xyz (MapPoint::getCoordinates)
 *   obs     : one monocular EdgeSE3ProjectXYZ per (point, frame): undistorted keypoint (float x,y) and
 *             information scalar 1/scaleFactor[octave] (globaloptimizer_g2o.cpp:96-97,244)
 * Arithmetic is fp64 like g2o; poses agree with the reference within 1e-6 (se3 state), see DESIGN.md.
 * Up to 64 non-fixed frames run the local-BA form (two launches per LM trial, reduced system in one
 * workgroup's LDS); more (global BA, up to 4096) run the wide form: sparse camera-pair lists, blocked dense LDL^T in HBM.
 * Stereo / RGB-D observations (EdgeStereoSE3ProjectXYZ, typesg2o.h:327-409: three residual rows u, v, u_right) enter through the
 * *_stereo entries below; such a problem runs the launch chain or the wide form (the persistent one-launch form is monocular).
 * ------------------------------------------------------------------------ */
typedef struct uh_ba uh_ba;

typedef struct uh_ba_problem {
    int32_t n_frames, n_points, n_obs;
    const float*   poses_f2g;       /* n_frames x 16 */
    const uint8_t* fixed;           /* n_frames */
    const float*   intr;            /* n_frames x 4: fx fy cx cy */
    const float*   points;          /* n_points x 3 */
    const int32_t* obs_point;       /* n_obs */
    const int32_t* obs_frame;       /* n_obs */
    const float*   obs_uv;          /* n_obs x 2 */
    const double*  obs_inv_sigma;   /* n_obs: (double)_InvScaleFactors[octave], i.e. (double)(float)(1. / scaleFactor[octave]) — the reference stores
                                     * the inverse scale factors as float (globaloptimizer_g2o.h:76), g2o sees that value widened */
} uh_ba_problem;

typedef struct uh_ba_params {
    int32_t n_iters;                /* ParamSet::nIters: pass 1 runs n_iters, pass 2 runs 2*n_iters (local BA: 5) */
    double  huber_delta;            /* <= 0 -> sqrt(5.99) */
    double  chi2_threshold;         /* <= 0 -> 5.99 */
    float   min_chi2_between_iter;  /* SparseOptimizer::optimize(iters, minChi2BetweenIter): 1 from BA */
} uh_ba_params;

int  uh_ba_create(uh_ctx* ctx, uh_ba** out);
void uh_ba_destroy(uh_ba* ba);
/* = setParams: snapshots the problem into HBM; the caller's arrays may change afterwards. params may be NULL. */
int  uh_ba_set_problem(uh_ba* ba, const uh_ba_problem* problem, const uh_ba_params* params);
/* = optimize(bool* stopASAP): runs both passes from the snapshot; *stop_asap (may be NULL) is polled while waiting. */
int  uh_ba_optimize(uh_ba* ba, const volatile uint8_t* stop_asap);
/* pinned device-visible force-stop byte owned by the optimiser (write 1 from any thread to stop between trials) */
/* asynchronous form: runs uh_ba_optimize on a worker thread owned by the object — the reference runs GlobalOptimizer::optimize
 * on its mapper thread beside the tracker (mapmanager.cpp:150) — and uh_ba_wait returns its result (UH_OK or the error).
 * One optimisation in flight per object; set_problem / get_results only between wait and the next optimize.
 * Both sides of the hand-over spin before they sleep (the worker for the next request: <= 0.3 ms; uh_ba_wait for the result: <= 2 ms),
 * because an optimisation is half a millisecond and a futex wake-up is 10-20 us of it: a caller that wants its core back while a
 * long (global) optimisation runs should do other work before calling uh_ba_wait, not rely on uh_ba_wait to block at once. */
int  uh_ba_optimize_async(uh_ba* ba, const volatile uint8_t* stop_asap);
int  uh_ba_wait(uh_ba* ba);
uint8_t* uh_ba_stop_flag(uh_ba* ba);
/* = getResults: poses n_frames x 16 float (fixed frames returned unchanged), points n_points x 3 float, per-observation
 * chi2 (as last evaluated by the optimiser) and bad-association flag (chi2 > 5.99 or point behind the camera);
 * iters_out[2] = outer iterations executed in pass 1 / pass 2.  Any output pointer may be NULL. */
int  uh_ba_get_results(uh_ba* ba, float* poses_out, float* points_out, double* chi2_out, uint8_t* bad_out, int32_t* iters_out);
int  uh_ba_get_pose_state(uh_ba* ba, double* pose7_out);   /* n_frames x (qx qy qz qw tx ty tz), fp64 */

/* ---- the same three phases without a host copy on either side (what the C++ adaptor's flatten_for_ba / getResults use).
 * A local BA is a NEW problem per keyframe (mapmanager.cpp:11388-11405 setParams + optimize on the mapper thread, :1267-1305
 * getResults on the tracker thread), so setParams and getResults are on the clock as much as optimize:
 *   uh_ba_map_staging   the optimiser owns ONE pinned, device-visible staging block; the caller writes the flattened problem straight
 *                       into it (observations as 24-byte records) — capacities are rounded up and kept across problems
 *   uh_ba_set_problem_staged   = setParams on what the staging block holds: one H2D copy + one kernel that scatters the observation
 *                       indices into a (point x frame) table in HBM; nothing is built on the host, nothing is synchronised.
 *                       An observation whose point / frame index is out of range is refused here; a (point, frame) pair that
 *                       occurs twice is detected by that kernel and reported by the following uh_ba_optimize (UH_EINVAL).
 *   uh_ba_results_view  = getResults in place: pointers into the pinned result block the optimisation kernel wrote (valid until the
 *                       next set_problem on this object); uh_ba_get_results copies from the same block.
 * uh_ba_set_problem (arrays anywhere in host memory) converts into the staging block and takes the same path. */
typedef struct uh_ba_obs {          /* one monocular EdgeSE3ProjectXYZ (globaloptimizer_g2o.cpp:224-249) */
    int32_t point, frame;           /* indices into points / frames of this problem */
    float   u, v;                   /* undistorted keypoint */
    double  inv_sigma;              /* (double)_InvScaleFactors[octave] */
} uh_ba_obs;                        /* 24 bytes */

typedef struct uh_ba_staging {
    float*     poses_f2g;           /* cap_frames x 16 */
    uint8_t*   fixed;               /* cap_frames */
    float*     intr;                /* cap_frames x 4 */
    float*     points;              /* cap_points x 3 */
    uh_ba_obs* obs;                 /* cap_obs */
    int32_t    cap_frames, cap_points, cap_obs;
} uh_ba_staging;

typedef struct uh_ba_results_view {
    const float*   poses;           /* n_frames x 16 (fixed frames unchanged) */
    const float*   points;          /* n_points x 3 */
    const double*  chi2;            /* n_obs */
    const uint8_t* bad;             /* n_obs */
    const double*  pose_state;      /* n_frames x 7 (qx qy qz qw tx ty tz) */
    int32_t        iters[2];
    int32_t        n_frames, n_points, n_obs;
} uh_ba_results_view;

int  uh_ba_map_staging(uh_ba* ba, int n_frames, int n_points, int max_obs, uh_ba_staging* out);
int  uh_ba_set_problem_staged(uh_ba* ba, int n_frames, int n_points, int n_obs, const uh_ba_params* params);
int  uh_ba_results_view_get(uh_ba* ba, uh_ba_results_view* out);
/* setParams + optimize on the object's worker thread (the reference's mapper thread does exactly these two calls back to back);
 * problem == NULL: the staging block (n_frames / n_points / n_obs as given).  The caller's arrays must stay valid until uh_ba_wait. */
int  uh_ba_solve_async(uh_ba* ba, const uh_ba_problem* problem, int n_frames, int n_points, int n_obs, const uh_ba_params* params,
                       const volatile uint8_t* stop_asap);
/* which form the current problem runs in: 0 launch chain (9+ free keyframes that do not fit the persistent form), 1 persistent
 * one-launch kernel, 2 wide (global BA); *lanes_per_landmark_out (may be NULL) = the persistent form's padded number of free cameras */
int  uh_ba_form(uh_ba* ba, int* lanes_per_landmark_out);
/* the per-observation chi2 is an extra of this ABI (GlobalOptimizer::getResults does not return it) and three quarters of the bytes the
 * optimisation kernel hands over: uh_ba_want_chi2(ba, 0) leaves it out from the next set_problem on (chi2_out must then be NULL) */
int  uh_ba_want_chi2(uh_ba* ba, int on);

/* ---- stereo / RGB-D observations (globaloptimizer_g2o.cpp:229-272).  Per observation the depth Frame::getDepth(kp): depth <= 0 is
 * the monocular edge above; depth > 0 is a three-row edge with mbf = bl * fx and kp_ur = u - mbf / depth formed in float as the
 * reference forms them, information I3 * inv_sigma, Huber width thHuber3D and outlier limit Chi3D (globaloptimizer_g2o.h:112-117).
 * A problem in which no observation has depth > 0 takes exactly the monocular route of uh_ba_set_problem / _staged (same form, same
 * kernels, same results).  With at least one, uh_ba_form reports 0 or 2; optimize / optimize_async / wait / get_results /
 * get_pose_state / stop flag / want_chi2 work unchanged, uh_ba_results_view_get refuses as for every chain / wide problem.  A landmark
 * with a single (three-row) observation is accepted (:142).  Refused with UH_EINVAL, nothing launched: stereo == NULL or a NULL
 * array while n_obs > 0, a non-finite depth, depth > 0 on a frame whose baseline is not finite and positive, more than 4096 free
 * keyframes.  uh_ba_solve_async has no stereo form. */
typedef struct uh_ba_stereo {
    const float* obs_depth;         /* n_obs: Frame::getDepth(kp); <= 0 -> monocular edge */
    const float* frame_bl;          /* n_frames: Frame::imageParams.bl of that frame */
    double huber_delta_3d;          /* <= 0 -> (double)(float)sqrt(7.815f) */
    double chi2_threshold_3d;       /* <= 0 -> (double)7.815f */
} uh_ba_stereo;

typedef struct uh_ba_staging_stereo {   /* uh_ba_staging + the two stereo arrays (host memory owned by the optimiser) */
    float*     poses_f2g;           /* cap_frames x 16 */
    uint8_t*   fixed;               /* cap_frames */
    float*     intr;                /* cap_frames x 4 */
    float*     points;              /* cap_points x 3 */
    uh_ba_obs* obs;                 /* cap_obs (24-byte records) */
    float*     obs_depth;           /* cap_obs */
    float*     frame_bl;            /* cap_frames */
    int32_t    cap_frames, cap_points, cap_obs;
} uh_ba_staging_stereo;

int  uh_ba_set_problem_stereo(uh_ba* ba, const uh_ba_problem* problem, const uh_ba_stereo* stereo, const uh_ba_params* params);
int  uh_ba_map_staging_stereo(uh_ba* ba, int n_frames, int n_points, int max_obs, uh_ba_staging_stereo* out);
int  uh_ba_set_problem_staged_stereo(uh_ba* ba, int n_frames, int n_points, int n_obs, const uh_ba_params* params,
                                     double huber_delta_3d, double chi2_threshold_3d);

/* ---- squared planar markers with free poses (globaloptimizer_g2o.cpp:156-171, 277-352, 451-455, 526-527; MarkerEdge, typesg2o.h:108-167).
 * Every marker is a free SE3 vertex of the pose part (six parameters, exp(update) * estimate), linked by one eight-row edge to every
 * frame that sees it: error = und_corners - the projection of the four corners (-+size/2, +-size/2, 0) through c2g * g2m rounded to
 * float, g2o's numeric central differences (delta = (double)1e-4f) on both vertices, information edge_weight * I8 (the frame's
 * frame_MarkerWeight, :281-299 — flatten_for_ba_markers computes it), NO robust kernel; the edges are never excluded or flagged and
 * are the same in both passes; their chi2 is part of the Levenberg decision, the chi2 stop and the lambda initialisation.  A fixed
 * frame's edge contributes the marker's diagonal block and right-hand side only.
 * markers == NULL or n_edges == 0: exactly uh_ba_set_problem / uh_ba_set_problem_stereo (stereo != NULL).  Otherwise the problem runs
 * in the wide form whatever its size (uh_ba_form reports 2), n_points = n_obs = 0 included; optimize / optimize_async / wait /
 * get_results / get_pose_state / stop flag / want_chi2 work unchanged, uh_ba_results_view_get refuses as for every wide problem.
 * Refused with UH_EINVAL, nothing launched: a NULL array, edge_marker / edge_frame out of range, a (marker, frame) pair that occurs
 * twice, a weight or a size that is not finite and > 0, a non-finite pose or corner, more than 4096 free keyframes + markers.
 * Not covered: the planar constraint between markers (ParamSet::InPlaneMarkers, :355-398), the staged and solve_async routes. */
typedef struct uh_ba_markers {
    int32_t n_markers;
    const float*   pose_g2m;        /* n_markers x 16, row-major 4x4 (Marker::pose_g2m) */
    const float*   size;            /* n_markers (Marker::size) */
    int32_t n_edges;
    const int32_t* edge_marker;     /* n_edges */
    const int32_t* edge_frame;      /* n_edges: index into the problem's frames */
    const float*   und_corners;     /* n_edges x 8: x0 y0 .. x3 y3 (MarkerObservation::und_corners) */
    const double*  edge_weight;     /* n_edges: information = w * I8 */
} uh_ba_markers;
int  uh_ba_set_problem_markers(uh_ba* ba, const uh_ba_problem* problem, const uh_ba_stereo* stereo /* or NULL */, const uh_ba_markers* markers,
                               const uh_ba_params* params);
/* after optimize: the marker poses as float 4x4 (getResults, :526-527), their fp64 state (qx qy qz qw tx ty tz; may be NULL) and the
 * chi2 of every marker edge at the final estimate (may be NULL) */
int  uh_ba_get_marker_results(uh_ba* ba, float* pose_g2m_out /* n_markers x 16 */, double* pose7_out /* n_markers x 7 or NULL */,
                              double* edge_chi2_out /* n_edges or NULL */);

/* ------------------------------------------------------------------------
 * Loop-closure pose graph — replaces loopClosurePathOptimizationg2o (src/optimization/graphoptsim3.cpp:74-168): g2o's Levenberg
 * (lambda_init 1e-16, 20 iterations, BlockSolver_7_3 with an exact LDL^T) over VertexSim3Expmap / EdgeSim3 (typesg2o.h:673-749) on
 * the essential graph of all keyframes.
 *   vertices  one per pose: Sim3(Quaternion(R), t, 1) from the float 4x4; vertex idx_new starts at expected_pose_new, vertex idx_old is
 *             fixed; fix_scale is VertexSim3Expmap::_fix_scale of every vertex
 *   edges     EdgeSim3 (vertex 0 = edge_i, vertex 1 = edge_j) with measurement Sjw * Siw^-1 from the INPUT poses (only the closing
 *             edge (idx_new, idx_old), in either order, takes expected_pose_new for the new keyframe), information weight * I7;
 *             the same pair may occur more than once and in either order
 *   Jacobians g2o's numeric central differences with step (double)fd_delta — BaseBinaryEdge::_delta_der, a float, 1e-9f
 *   results   [sR | t/s] rounded to float for EVERY pose (a pose without edges and the fixed one go through the quaternion round trip
 *             and nothing else), and the Sim3 state
 * Refused before anything is launched: UH_EINVAL for a NULL array, idx_new / idx_old or an edge end out of range, an edge from a
 * pose to itself, idx_new == idx_old, a non-finite weight, params out of range; UH_ECAPACITY for more than UH_POSEGRAPH_MAX_POSES
 * poses (the system is dense: 7 n x 7 n doubles, 1.6 GB at the cap).  Without any edge the poses come back after the conversion
 * round trip with 0 iterations.  The call is synchronous on the context's stream.
 * ------------------------------------------------------------------------ */
#define UH_POSEGRAPH_MAX_POSES 2048
#define UH_POSEGRAPH_MAX_ITERS 256
typedef struct uh_posegraph uh_posegraph;

typedef struct uh_posegraph_problem {
    int32_t n_poses;
    const float*   pose_f2g;           /* n_poses x 16, row-major 4x4 */
    int32_t n_edges;
    const int32_t* edge_i;             /* n_edges: index of the edge's first pose */
    const int32_t* edge_j;             /* n_edges: index of its second pose */
    const float*   edge_weight;        /* n_edges, or NULL = 1 for every edge */
    int32_t idx_new, idx_old;          /* IdClosesLoopNew / IdClosesLoopOld as indices */
    const float*   expected_pose_new;  /* 16 */
    int32_t fix_scale;
} uh_posegraph_problem;

typedef struct uh_posegraph_params {   /* 0 = the reference's value */
    int32_t max_iters;                 /* 20; at most UH_POSEGRAPH_MAX_ITERS */
    double  lambda_init;               /* 1e-16 */
    float   fd_delta;                  /* 1e-9f; widened to double as g2o widens _delta_der */
} uh_posegraph_params;

typedef struct uh_posegraph_info {
    int32_t iterations;                /* what SparseOptimizer::optimize returns */
    double  lambda;                    /* the final damping */
    double  chi2_before, chi2_after;   /* at the initial and at the returned estimates */
} uh_posegraph_info;

int  uh_posegraph_create(uh_ctx* ctx, uh_posegraph** out);
void uh_posegraph_destroy(uh_posegraph* pg);
/* the argument checks of uh_posegraph_optimize alone (host only, no device needed); params may be NULL */
int  uh_posegraph_check_problem(const uh_posegraph_problem* problem, const uh_posegraph_params* params);
int  uh_posegraph_optimize(uh_posegraph* pg, const uh_posegraph_problem* problem, const uh_posegraph_params* params /* or NULL */);
/* every output may be NULL.  state8: qx qy qz qw tx ty tz s; trials: Levenberg trials of each iteration (`iterations` entries, room for
 * max_iters) */
int  uh_posegraph_get_results(uh_posegraph* pg, float* poses_out /* n_poses x 16 */, double* state8_out /* n_poses x 8 */,
                              uh_posegraph_info* info, int32_t* trials_out);
/* the first linearisation of the latest optimize: per edge the error (7), d error / d vertex 0 and / d vertex 1 (7 x 7 row-major
 * each, zero for the fixed vertex) and the measurement (8, as state8) */
int  uh_posegraph_debug_linearisation(uh_posegraph* pg, double* err_out, double* Ji_out, double* Jj_out, double* meas_out);

/* ------------------------------------------------------------------------
 * Bag of words — replaces fbow::Vocabulary::transform / fBow::score:
 *   3rdparty/fbow/fbow/fbow.h:54-116 (class surface), fbow.cpp:51-90 (transform with level), :92-143 (normalised
 *   transform), :171-190 (stream format), :192-243 (score); UcoSLAM call site keyframedatabase.cpp:310-322 (level 3).
 * The GPU does the per-descriptor tree descent; the std::map containers of the reference API are assembled by the
 * host adaptor from the per-descriptor triples, in feature order (keeps the reference's float summation order).
 * ------------------------------------------------------------------------ */
typedef struct uh_bow uh_bow;
int  uh_bow_create(uh_ctx* ctx, uh_bow** out);
void uh_bow_destroy(uh_bow* bow);
/* Vocabulary::fromStream: `stream` = u64 signature 55824124 + raw params struct (120 bytes) + block blob */
int  uh_bow_load(uh_bow* bow, const void* stream, size_t nbytes);
/* same, from an already split params struct (fbow::Vocabulary::params, 120 bytes) and blob */
int  uh_bow_set(uh_bow* bow, const void* params120, const void* blob);
int  uh_bow_get_params(const uh_bow* bow, void* params120);
/* per descriptor i: word[i] (0xFFFFFFFF if the descent ends without a leaf), weight[i], node[i] = node id at `level`
 * (valid[i] = 0 if never recorded).  Empty input fails like the reference ("No input data"). */
int  uh_bow_transform(uh_bow* bow, const uint8_t* desc, int n, size_t stride, int desc_bytes, int level,
                      uint32_t* word, float* weight, uint32_t* node, uint8_t* valid);
int  uh_bow_transform_dev(uh_bow* bow, const uint8_t* d_desc, int n, int level,
                          uint32_t* d_word, float* d_weight, uint32_t* d_node, uint8_t* d_valid);
double uh_bow_score(const uint32_t* ids1, const float* w1, int n1, const uint32_t* ids2, const float* w2, int n2);

/* KPFrameDataBase (src/map_types/keyframedatabase.cpp:150-238): the keyframes' bags of words resident in HBM.  add / del mirror
 * KPFrameDataBase::add / del (the bag is the fBow of uh_bow_transform(desc, 3): words ascending, raw weights).  query is the
 * first half of relocalizationCandidates (:195-238): per keyframe the number of query words it shares and fBow::score (one lane
 * per keyframe, products added in ascending word order like the reference), then on the host maxCommonWords, the 0.8 cut and
 * the min_score cut; it returns the surviving frames (`frame_score`) in ascending id order.  The covisibility accumulation that
 * follows (:241-275) needs CovisGraph and stays with the caller (ucoslam_cv3_amd.bow.KPFrameDataBase shows it). */
typedef struct uh_bowdb uh_bowdb;
int  uh_bowdb_create(uh_ctx* ctx, uh_bowdb** out);
void uh_bowdb_destroy(uh_bowdb* db);
int  uh_bowdb_size(const uh_bowdb* db);
int  uh_bowdb_add(uh_bowdb* db, uint32_t frame_id, const uint32_t* words, const float* weights, int n);
int  uh_bowdb_del(uh_bowdb* db, uint32_t frame_id);
int  uh_bowdb_query(uh_bowdb* db, const uint32_t* words, const float* weights, int n, const uint32_t* excluded, int n_excluded,
                    float min_score, uint32_t* frame_ids_out, uint32_t* nobs_out, double* score_out, int cap);

/* ------------------------------------------------------------------------
 * FrameMatcher_Flann post-filter (host policy around the index) — src/utils/framematcher.cpp:228-319:
 * per query best/second-best scan over the nn columns IN ROW ORDER (min distance gate, octave gap, optional epipolar
 * gate 3.84*sigma^2, ratio test against a same-octave runner-up), filter_ambiguous_train (misc.cpp:153-185), then the
 * 30-bin orientation histogram keeping the three dominant bins (:290-316, computeThreeMaxima :67-108).
 * Returns the number of matches written (>= 0) or a negative UH_E* code.
 * ------------------------------------------------------------------------ */
typedef struct uh_dmatch {          /* cv::DMatch */
    int32_t queryIdx, trainIdx, imgIdx;
    float   distance;
} uh_dmatch;

typedef struct uh_match_filter_args {
    int32_t nq, nn;
    const int32_t* indices;         /* nq x nn rows of uh_knn_search (unsorted heap order, as FrameMatcher passes sorted=false) */
    const int32_t* distances;
    const uint32_t* map_idx_query;  /* row -> keypoint index of the query frame (manageMode), NULL = identity */
    const uint32_t* map_idx_train;  /* index row -> keypoint index of the train frame, NULL = identity */
    const int32_t* q_octave; const float* q_angle; const float* q_pt;   /* query und_kpts fields; q_pt (x,y) only for F12 */
    const int32_t* t_octave; const float* t_angle; const float* t_pt;   /* train und_kpts fields */
    const float* scale_factors;     /* query frame scaleFactors (only with F12) */
    const float* F12;               /* row-major 3x3 fundamental matrix (getFund12: uh_fundamental_12) or NULL (no epipolar gate) */
    float min_desc_dist, nn_match_ratio;
    int32_t check_orientation, max_octave_diff;
    /* sizes of the arrays above; > 0: every mapped keypoint index / octave is range-checked (UH_EINVAL), 0: unchecked */
    int32_t n_query_kpts, n_train_kpts, n_levels;
} uh_match_filter_args;

int uh_match_filter(const uh_match_filter_args* args, uh_dmatch* out, int cap);
/* filter_ambiguous_train (by_train != 0) / filter_ambiguous_query (by_train == 0), in place; returns the new count */
int uh_filter_ambiguous(uh_dmatch* matches, int n, int by_train);

/* FrameMatcher_BoW::match / matchEpipolar (framematcher.cpp:395-535): features of the two frames that share a vocabulary node
 * (Frame::bowvector_level, the fbow::fBow2 of uh_bow_transform at level 3) are compared all against all.  A frame comes as the
 * node map in std::map order — ascending node ids, per node the feature indices in push_back order — plus the keypoint arrays
 * and `used` = isUsed(frame, idx, mode) (:373-379: not FLAG_NONMAXIMA, and assigned / unassigned as the mode asks; NULL = all).
 * Hamming distances and the order-dependent best / "last not better" bookkeeping (:441-476) run on the GPU, the acceptance
 * rule, filter_ambiguous_train and the orientation histogram on the host.  Matches: queryIdx / trainIdx = keypoint indices.
 * A node with an empty list is refused (the reference's loop would never advance past it, :436). */
typedef struct uh_bow_frame {
    int32_t n_nodes;
    const uint32_t* node_ids;       /* n_nodes, ascending */
    const int32_t* node_ptr;        /* n_nodes + 1 offsets into feat_idx */
    const uint32_t* feat_idx;       /* keypoint indices, node lists back to back */
    int32_t n_kpts;
    const uint8_t* desc;            /* n_kpts x 32 */
    const int32_t* octave; const float* angle;   /* und_kpts fields */
    const float* pt;                /* n_kpts x 2 (x, y); only read with F12 */
    const uint8_t* used;            /* n_kpts or NULL */
} uh_bow_frame;
typedef struct uh_bow_match_args {
    uh_bow_frame query, train;
    const float* scale_factors; int32_t n_levels;   /* query frame scaleFactors (only with F12) */
    const float* F12;               /* row-major 3x3 fundamental matrix (getFund12: uh_fundamental_12) or NULL */
    float min_desc_dist, nn_match_ratio;
    int32_t check_orientation, max_octave_diff;
} uh_bow_match_args;
typedef struct uh_bowmatch uh_bowmatch;
int  uh_bowmatch_create(uh_ctx* ctx, uh_bowmatch** out);
void uh_bowmatch_destroy(uh_bowmatch* bm);
int  uh_bowmatch_match(uh_bowmatch* bm, const uh_bow_match_args* args, uh_dmatch* out, int cap);

/* getFund12 (framematcher.cpp:58-64) -> computeF12(eye, Ktrain, RT, Kquery) (misc.cpp:893-920): the F12 that uh_match_filter_args::F12
 * and uh_bow_match_args::F12 take for one (train, query) pair.  Host only.  Both cameras as fx fy cx cy; RT = FQ2T, the row-major
 * float 4x4 query.pose_f2g * train.pose_f2g.inv(); F12_out row-major 3x3.  The upper-triangular K is inverted in closed form; every
 * cv::Mat product of the chain accumulates its elements in double and rounds once, as OpenCV's float GEMM does — UNPINNED, like the
 * products of uh_newpoints_run (a fixture of computeF12 outputs from a machine with OpenCV would pin it). */
int  uh_fundamental_12(const float* intr4_train, const float* intr4_query, const float* RT, float* F12_out /* 9 */);

/* ------------------------------------------------------------------------
 * New map points — replaces, for one new keyframe and all its covisible neighbours, the loop of MapManager that follows matchEpipolar
 * (src/utils/mapmanager.cpp:10087-10696, line numbers of the de-obfuscated text): Triangulate(newKF, neighbour, RT, matches)
 * (src/basictypes/misc.cpp:923-1041), the distance-ratio / octave-ratio check, and the merge per keypoint of the new keyframe.
 *
 * Roles (misc.cpp's names mislead): the new keyframe is Triangulate's `Train`, the neighbour its `Query`; RT = neighbour.pose_f2g *
 * newKF.pose_f2g.inv() takes the new keyframe's camera to the neighbour's (p3dC2 = R p3dC1 + t); a match's trainIdx is a keypoint of
 * the new keyframe, its queryIdx one of the neighbour.
 *
 * Per match, in this order (status code of the branch that refuses it):
 *   1  cos of the two rays < 0 or > 0.9998 (:989-997)            6  chi2 of the reprojection in the new keyframe > max_chi2, weighted by
 *   2  fourth component of A's null vector == 0 (:936)              1 / scaleFactor^2 of its keypoint's octave (:1017-1022)
 *   3  a coordinate is not finite (:1003)                        7  the same in the neighbour (:1025-1031)
 *   4  depth <= 0 in the new keyframe's camera (:1007)           8  distance of pg = pose_g2f * p3d to either camera centre is 0
 *   5  depth <= 0 in the neighbour's camera (:1013)              9  ratioDist * ratio_factor < ratioOctave || ratioDist > ratioOctave * ratio_factor
 *   0  accepted                                                     with ratioDist = dist1 / dist2, ratioOctave = sf_new[oct] / sf_nb[oct]
 * ratio_factor is the reference's 1.5f * params.scaleFactor; max_chi2 its 5.998.
 *
 * Merge (:10416-10696): the accepted matches of all pairs, in pair order then match order, grouped by trainIdx.  Each group becomes one
 * point, in ascending trainIdx: position and descriptor distance of the CHOSEN candidate, observations (new keyframe, trainIdx) then
 * every candidate's (neighbour, queryIdx) in list order.  merge_rule picks the candidate:
 *   UH_NEWPOINTS_MERGE_SMALLEST_OCTAVE  the first candidate whose neighbour keypoint has the strictly smallest octave — what the
 *                                       reference's loop is written to find (and ORB-SLAM's intent)
 *   UH_NEWPOINTS_MERGE_AS_COMPILED      the LAST candidate — what the reference does as compiled: the loop compares each octave with a
 *                                       running minimum that it never assigns (:10525-10618), so every candidate wins in turn
 *
 * Float conventions: float expressions in the reference's written order without contraction.  Two things cannot follow the reference
 * byte for byte, because it computes them inside OpenCV, which cannot be built here — both UNPINNED:
 *   - the null vector: cv::SVD in float there; here a one-sided Jacobi in double on the float A, the three quotients rounded to float once
 *   - the products taken through cv::Mat's operator* (P2 = K2 [R|t], R p + t, R' ray; the chain of uh_fundamental_12): each element
 *     accumulated in double and rounded once (OpenCV's float GEMM); xn / cv::norm(xn) as a multiplication by (float)(1 / norm)
 * One fixture of Triangulate outputs and one of computeF12 outputs, generated where OpenCV exists, would pin them.
 *
 * Refused with UH_EINVAL before anything is launched, uh_last_error() naming the pair and the match: a queryIdx / trainIdx outside
 * the keypoint counts, an octave of a matched keypoint outside n_levels, a trainIdx twice within one pair (matchEpipolar's closing
 * filter_ambiguous_train rules it out; the kernels rely on it), more than UH_NEWPOINTS_MAX_KPTS keypoints in the new keyframe (the
 * merge is one workgroup), more than UH_NEWPOINTS_MAX_PAIRS pairs, a neighbour with more than 128 levels or 2^24 - 1 matches (a cell
 * of the candidate table holds both).  The call is synchronous on the context's stream: one upload, two
 * kernels, one download, one wait; the results are bit-reproducible run to run.
 * ------------------------------------------------------------------------ */
#define UH_NEWPOINTS_MAX_KPTS  16384
#define UH_NEWPOINTS_MAX_PAIRS 1024
#define UH_NEWPOINTS_MERGE_SMALLEST_OCTAVE 0
#define UH_NEWPOINTS_MERGE_AS_COMPILED     1
typedef struct uh_newpoints uh_newpoints;

typedef struct uh_newpoints_pair {     /* one neighbour */
    float RT[16];                      /* neighbour.pose_f2g * newKF.pose_f2g.inv(), row-major 4x4 */
    float intr4[4];                    /* fx fy cx cy */
    float cam_center[3];               /* Frame::getCameraCenter */
    int32_t n_levels;
    const float* scale_factors;        /* n_levels */
    int32_t n_kpts;
    const float* pt;                   /* n_kpts x 2, undistorted */
    const int32_t* octave;             /* n_kpts */
    int32_t n_matches;
    const uh_dmatch* matches;          /* queryIdx = the neighbour's keypoint, trainIdx = the new keyframe's */
} uh_newpoints_pair;

typedef struct uh_newpoints_args {
    float intr4[4];                    /* the new keyframe: fx fy cx cy */
    float pose_g2f[16];                /* pose_f2g.inv() as the caller's Se3Transform gives it (camera -> global) */
    float cam_center[3];
    int32_t n_levels;
    const float* scale_factors;
    int32_t n_kpts;                    /* <= UH_NEWPOINTS_MAX_KPTS */
    const float* pt;
    const int32_t* octave;
    int32_t n_pairs;
    const uh_newpoints_pair* pairs;
    float max_chi2;                    /* the reference: 5.998 */
    float ratio_factor;                /* the reference: 1.5f * params.scaleFactor */
    int32_t merge_rule;                /* UH_NEWPOINTS_MERGE_* */
} uh_newpoints_args;

/* Pointers into pinned memory owned by the handle, valid until its next run or its destruction (as uh_ba_results_view). */
typedef struct uh_newpoints_result {
    int32_t n_total;                   /* matches of all pairs; the per-match arrays are concatenated in pair order */
    const uint8_t* status;             /* n_total: the codes above */
    const float*   xyz_cam;            /* n_total x 3: Triangulate's return value, in the new keyframe's camera frame; NaN where it leaves NaN */
    int32_t n_new;
    int32_t n_obs;                     /* obs_ptr[n_new] */
    const int32_t* kp_idx;             /* n_new, ascending: the keypoint of the new keyframe */
    const float*   xyz_global;         /* n_new x 3: pg of the chosen candidate */
    const float*   distance;           /* n_new: its match distance */
    const int32_t* chosen_pair;        /* n_new */
    const int32_t* chosen_match;       /* n_new: index in that pair's match list */
    const int32_t* obs_ptr;            /* n_new + 1: CSR offsets into obs_pair / obs_kpt */
    const int32_t* obs_pair;           /* -1 = the new keyframe itself (always a list's first entry), else the pair */
    const int32_t* obs_kpt;            /* the keypoint in that frame */
} uh_newpoints_result;

int  uh_newpoints_create(uh_ctx* ctx, uh_newpoints** out);
void uh_newpoints_destroy(uh_newpoints* np);
int  uh_newpoints_run(uh_newpoints* np, const uh_newpoints_args* args, uh_newpoints_result* result);

/* ------------------------------------------------------------------------
 * One frame stream sharded over the GPUs of a node (BASELINE config 5): pyramid levels of frame t, the map's train tiles
 * and the fbow descent of frame t-1 sharded over `world` ranks (one process per GPU), ONE all-gather of fixed-size messages per frame.
 * The producers write straight into the send buffer and the exact replay reads the gathered lists where they lie (csrc/fstream.hip);
 * counts stay on the device, a step never synchronises with the host.  Results trail the input by one frame (software pipeline).
 *   ext   an extractor with its FeatParams set (uh_orb_set_params); its level range is set per call
 *   tile  a uh_knn built over THIS rank's rows [nt*rank/world, nt*(rank+1)/world) with uh_knn_set_row_offset(first global row)
 *   voc   optional vocabulary (NULL: no bag-of-words slices in the message)
 * The collective is RCCL's all-gather on the context's stream: uh_fstream_comm_unique_id on rank 0 -> the 128 bytes reach every rank by
 * any host channel -> uh_fstream_comm_init everywhere (librccl is loaded with dlopen); or uh_fstream_set_comm with the host's own
 * ncclComm_t; world == 1 needs neither.  uh_fstream_put_message serves hosts with another transport.
 * ------------------------------------------------------------------------ */
typedef struct uh_fstream uh_fstream;
typedef struct uh_fstream_params {
    int32_t rank, world;
    int32_t nn;                     /* neighbours per query (FrameMatcher: 10) */
    int32_t max_features;           /* = FeatParams::maxFeatures: rows per frame, queries per search */
    int32_t cand_cap;               /* accept-list capacity per (query, tile); an overflow is reported, see d_overflow */
    int32_t sorted;                 /* KnnSearchParams::sorted */
    int32_t bow_level;              /* Vocabulary::transform level (keyframedatabase.cpp:319: 3) */
} uh_fstream_params;
int    uh_fstream_create(uh_ctx* ctx, uh_orb* ext, uh_knn* tile, uh_bow* voc, const uh_fstream_params* params, uh_fstream** out);
void   uh_fstream_destroy(uh_fstream* fs);
size_t uh_fstream_message_bytes(const uh_fstream* fs);
void*  uh_fstream_send_buffer(uh_fstream* fs);      /* device, message_bytes */
void*  uh_fstream_recv_buffer(uh_fstream* fs);      /* device, world x message_bytes, rank order */
int    uh_fstream_comm_unique_id(uint8_t id_out[128]);
int    uh_fstream_comm_init(uh_fstream* fs, const uint8_t id[128]);
int    uh_fstream_set_comm(uh_fstream* fs, void* nccl_comm);
int    uh_fstream_comm_ranks(uh_fstream* fs);       /* ncclCommCount of the communicator in use (1 without one); < 0 on error */
int    uh_fstream_put_message(uh_fstream* fs, int rank, const void* d_message);
/* step t: this rank's levels [level_first, level_end) of the frame (device image), its tile's accept lists and its fbow slice for frame t-1 */
int    uh_fstream_local_dev(uh_fstream* fs, const uint8_t* d_frame, int w, int h, size_t stride, int level_first, int level_end);
int    uh_fstream_exchange(uh_fstream* fs);
/* frame t complete (d_kps / d_desc: max_features rows, *d_count valid) and frame t-1's rows (d_prev_*: max_features x nn, the first
 * *d_prev_count valid; 0 on the first step) + its fbow triples (max_features each, or NULL).  *d_overflow: bit 0 an accept list exceeded
 * cand_cap (retry the frame with a larger capacity), bit 1 a message header was out of range.  All pointers are device pointers. */
int    uh_fstream_finish_dev(uh_fstream* fs, uh_keypoint* d_kps, uint8_t* d_desc, int32_t* d_count, int32_t* d_prev_indices,
                             int32_t* d_prev_distances, int32_t* d_prev_count, uint32_t* d_bow_word, float* d_bow_weight, uint32_t* d_bow_node,
                             uint8_t* d_bow_valid, int32_t* d_overflow);

/* ------------------------------------------------------------------------
 * Pose-only optimisation — replaces PnPSolver::solvePnp (monocular, stereo / RGB-D matches and squared planar markers):
 *   src/optimization/pnpsolver.h:30-38, pnpsolver.cpp:116-409; edge types typesg2o.h:414-471, :521-650; kernel :82-105.
 * Inputs per match i: map point p3d[i] (float xyz, MapPoint::getCoordinates), undistorted keypoint kp[i] (float x,y),
 * inv_sigma[i] = 1/scaleFactors[octave] (float, :230), weight[i] = 1 or 0.5 for unstable points (:215-216).
 * Outputs: pose (row-major 4x4 float), bad[i] (1 = outlier: the reference marks DMatch::imgIdx = -1), outer iterations of the
 * four rounds.  Returns the inlier count (>= 0, solvePnp's return value) or a negative UH_E* code.
 * Degenerate matches are not refused, they are solved as the reference solves them (tests/golden/pnp_hard_golden.npz): zero
 * information everywhere fails every factorisation (one iteration of ten trials per round, the pose comes back as it went in);
 * a map point on the camera plane of the input pose makes the sums and lambda non-finite (one trial per round, no match is
 * relabelled, the pose comes back as it went in).
 * ------------------------------------------------------------------------ */
typedef struct uh_pnp uh_pnp;
int  uh_pnp_create(uh_ctx* ctx, uh_pnp** out);
void uh_pnp_destroy(uh_pnp* pnp);
int  uh_pnp_solve(uh_pnp* pnp, const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp,
                  const float* inv_sigma, const float* weight, float* pose_out, uint8_t* bad_out, int32_t* iters_out4,
                  double* state_out7);
/* device-resident form: d_work = n*32 bytes of scratch (16-byte aligned; only touched beyond 3000 matches); d_result5 = {inliers, iters[4]};
 * one launch, asynchronous on the context stream */
int  uh_pnp_solve_dev(uh_pnp* pnp, const float* d_pose_f2g, const float* d_intr4, int n, const float* d_p3d, const float* d_kp,
                      const float* d_inv_sigma, const float* d_weight, void* d_work, float* d_pose_out, uint8_t* d_bad_out,
                      int32_t* d_result5, double* d_state7);
/* Stereo / RGB-D observations (pnpsolver.cpp:205-276): depth[i] = Frame::getDepth(queryIdx) of match i; depth <= 0 keeps the monocular
 * edge, depth > 0 gives EdgeStereoSE3ProjectXYZOnlyPose (typesg2o.h:521-590) with the measurement (x, y, x - bl * fx / depth), the same
 * information, the robust weight doubled, Huber sqrt(7.815) and outliers above chi2 7.815.  bl = imageParams.bl; must be > 0 when any
 * depth is > 0.  The caller passes the same weights as for uh_pnp_solve (the doubling happens inside).  depth == NULL, or every depth
 * <= 0, returns what uh_pnp_solve returns, bit for bit. */
int  uh_pnp_solve_stereo(uh_pnp* pnp, const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp,
                         const float* inv_sigma, const float* weight, const float* depth, float bl, float* pose_out, uint8_t* bad_out,
                         int32_t* iters_out4, double* state_out7);
/* device-resident form: d_depth (n floats, device) or NULL (= uh_pnp_solve_dev); with d_depth, bl must be > 0 and d_work holds n*36 bytes */
int  uh_pnp_solve_stereo_dev(uh_pnp* pnp, const float* d_pose_f2g, const float* d_intr4, int n, const float* d_p3d, const float* d_kp,
                             const float* d_inv_sigma, const float* d_weight, const float* d_depth, float bl, void* d_work,
                             float* d_pose_out, uint8_t* d_bad_out, int32_t* d_result5, double* d_state7);
/* Marker observations (pnpsolver.cpp:280-386): one MarkerEdgeOnlyProject (typesg2o.h:414-471) per marker in the same optimisation as the
 * keypoint edges.  The caller selects the markers as :281-299 does (the frame's markers with a valid pose_g2m that a neighbour keyframe of
 * currentKeyFrame sees) and flattens them; the solver does the rest as the reference: weight_marker = (0.3f * (n + markers) / (1 - 0.3f)) /
 * float(sum of the kernel weights) (+inf without matches), projections rounded to float, g2o's numeric Jacobian with delta = 1e-4f, one Huber
 * decision per marker (sqrt(15.507)), the kernel dropped for good when the marker's chi2 exceeds 15.507 after a round or from the third
 * round on.  Markers are never excluded and never counted: the return value stays the number of good keypoint matches.  With markers all
 * four rounds run (no stop below 10 good matches), and n = 0 matches is valid (p3d, kp, inv_sigma, weight and bad_out may then be NULL).
 * markers == NULL or markers->n == 0 returns what uh_pnp_solve_stereo returns, bit for bit (n = 0 too: pose in, 0).  Refused before anything
 * is launched: NULL arrays with n > 0, n outside [0, UH_PNP_MAX_MARKERS], a non-finite or non-positive size. */
#define UH_PNP_MAX_MARKERS 32
typedef struct uh_pnp_markers {
    int32_t n;                 /* marker_poses.size() after the caller's selection (pnpsolver.cpp:281-299); 0..UH_PNP_MAX_MARKERS */
    const float* pose_g2m;     /* n x 16, row-major 4x4: Marker::pose_g2m */
    const float* size;         /* n: Marker::size */
    const float* und_corners;  /* n x 8: MarkerObservation::und_corners, x0 y0 .. x3 y3 */
} uh_pnp_markers;
int  uh_pnp_solve_markers(uh_pnp* pnp, const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp,
                          const float* inv_sigma, const float* weight, const float* depth /* or NULL */, float bl,
                          const uh_pnp_markers* markers /* or NULL */, float* pose_out, uint8_t* bad_out, int32_t* iters_out4,
                          double* state_out7);
/* device-resident form: the three arrays of `markers` are device arrays as well (the sizes are not read on the host); one asynchronous launch */
int  uh_pnp_solve_markers_dev(uh_pnp* pnp, const float* d_pose_f2g, const float* d_intr4, int n, const float* d_p3d, const float* d_kp,
                              const float* d_inv_sigma, const float* d_weight, const float* d_depth /* or NULL */, float bl,
                              const uh_pnp_markers* markers /* or NULL */, void* d_work, float* d_pose_out, uint8_t* d_bad_out,
                              int32_t* d_result5, double* d_state7);

/* ------------------------------------------------------------------------
 * Projection matcher — replaces Map::matchFrameToMapPoints (src/map.cpp:651-770) on flattened inputs:
 *   frame side  Frame::und_kpts / desc / scaleFactors / imageParams.CameraMatrix / minXY,maxXY (map_types/frame.h:60-81) and the
 *               kd-tree over und_kpts (Frame::create_kdtree, frame.h:124; picoflann.h) — rebuilt bit-identically by set_frame
 *   map side    the candidate map points AFTER the reference's id filtering (getMapPointsInFrames / lastFIdxSeen, map.cpp:657-668,
 *               which stays host code): ids, getCoordinates(), normal, get{Min,Max}DistanceInvariance(), descriptor
 * match() returns the DMatch list (queryIdx = keypoint, trainIdx = map point id, imgIdx = -1, distance = Hamming as float)
 * after filter_ambiguous_query, in map-point order like the reference; optional per-point outputs: best keypoint before the
 * ambiguity filter (-1 = none), its distance, and the "visible" flags (markMapPointsAsVisible: the caller applies
 * MapPoint::setVisible() to the flagged points).  Returns the number of matches (>= 0) or a negative UH_E* code.
 * ------------------------------------------------------------------------ */
typedef struct uh_proj_frame {
    const uh_keypoint* und_kpts;    /* cv::KeyPoint: pt and octave are read */
    int32_t n_kpts;
    const uint8_t* desc;            /* n_kpts x 32 */
    const float* scale_factors;     /* Frame::scaleFactors */
    int32_t n_levels;
    float fx, fy, cx, cy;           /* CameraMatrix(0,0) (1,1) (0,2) (1,2) */
    int32_t min_x, min_y, max_x, max_y;   /* Frame::minXY / maxXY (cv::Point, i.e. ints; defaults 0,0 / INT_MAX,INT_MAX) */
} uh_proj_frame;

typedef struct uh_map_points {
    int32_t n;
    const uint32_t* ids;            /* n */
    const float* pos3d;             /* n x 3 */
    const float* normal;            /* n x 3 */
    const float* min_dist;          /* n */
    const float* max_dist;          /* n */
    const uint8_t* desc;            /* n x 32 */
} uh_map_points;

typedef struct uh_projmatch uh_projmatch;
int  uh_projmatch_create(uh_ctx* ctx, uh_projmatch** out);
void uh_projmatch_destroy(uh_projmatch* pm);
int  uh_projmatch_set_frame(uh_projmatch* pm, const uh_proj_frame* frame);
/* the frame uh_orb_extract_frame_dev left on the device; `params` gives scale factors, camera and image bounds (its desc is ignored; its
 * und_kpts / n_kpts too unless the frame's tree is built by the host core, uh_dev_frame_set_tree_builder(f, 1): then they are the frame's
 * undistorted keypoints, exactly as many as its last extraction or upload gave the host, or UH_EINVAL).  `frame` must stay alive and
 * un-overwritten while the matcher uses it. */
int  uh_projmatch_set_frame_dev(uh_projmatch* pm, uh_dev_frame* frame, const uh_proj_frame* params);
int  uh_projmatch_match(uh_projmatch* pm, const float* pose_f2g /* row-major 4x4 */, const uh_map_points* points,
                        float min_desc_dist, float max_repj_dist, uh_dmatch* matches_out, int32_t cap,
                        int32_t* best_kp_out /* n or NULL */, float* best_dist_out /* n or NULL */, uint8_t* visible_out /* n or NULL */);
/* The tracker's projection search against the PREVIOUS frame (src/utils/system.cpp:5930-6460, private member of System; the
 * source is token-pasted, line numbers are statement starts after preprocessing; called at :6559-6565 with
 * (maxDescDistance*1.5, projDistThr) before PnPSolver::solvePnp).  The caller flattens the loop header (:5969-6089): one item
 * per keypoint i of the previous frame whose ids[i] names a valid, non-bad map point, in keypoint order — that point's id and
 * coordinates, und_kpts[i].octave and descriptor row i.  Per item: Frame::project(p, true, true) (frame.h:140-161) with
 * `pose_f2g` = the current frame's pose, radius maxRepjDist * scaleFactors[octave], candidates of exactly that octave in
 * kd-tree order, best (from minDescDist + 0.01) / second WITHOUT demotion, accepted iff best < 0.7 * second; then
 * filter_ambiguous_query.  The frame is the one given to uh_projmatch_set_frame.  Returns the number of matches or < 0. */
typedef struct uh_prev_points {
    int32_t n;
    const uint32_t* ids;            /* n: map point ids (DMatch::trainIdx) */
    const float* pos3d;             /* n x 3: MapPoint::getCoordinates() */
    const int32_t* octave;          /* n: prev.und_kpts[i].octave, each in [0, n_levels) */
    const uint8_t* desc;            /* n x 32: prev.desc rows */
} uh_prev_points;
int  uh_projmatch_match_prev(uh_projmatch* pm, const float* pose_f2g /* row-major 4x4 */, const uh_prev_points* points,
                             float min_desc_dist, float max_repj_dist, uh_dmatch* matches_out, int32_t cap,
                             int32_t* best_kp_out /* n or NULL */, float* best_dist_out /* n or NULL */);
/* The tracker's pose estimation for one frame as ONE call (src/utils/system.cpp:6559-6954, raw line numbers of the statement starts;
 * pnpsolver.cpp:116-409; map.cpp:651-770), on the device between the launches with ONE wait at the end (csrc/track.hpp):
 *   - the search against the previous frame (uh_projmatch_match_prev);
 *   - with MORE than min_inliers matches (:6595) the first PnPSolver::solvePnp from pose0 (:6626).  With min_inliers matches or fewer the
 *     reference runs its FrameMatcher fallback against the reference keyframe (:6664-6780), which this call does not: it reports no first
 *     solve (inliers1 = 0, iters1 = 0, pose1 = pose0, bad_prev all 0), as if the fallback had found nothing.  A caller that has the
 *     fallback runs it itself when n_prev <= min_inliers;
 *   - the decision (:6646, :6813): tracked iff inliers1 is MORE than min_inliers — the refined pose and map_radius_tracked, and EVERY match
 *     of the first search (its outliers too: solvePnp only flags them, :6842) is kept and its map point marked as seen this frame; else
 *     pose0, map_radius_lost and the first matches are dropped (:6877);
 *   - Map::matchFrameToMapPoints over `map` (:6897) without the points seen this frame (map.cpp:657-668): a candidate whose row is the
 *     prev_map_row of a first-search match cannot match; matches_map is that search's list after this exclusion;
 *   - the union of the kept first matches and matches_map under filter_ambiguous_query (:6913, :6931) and the second solvePnp from the
 *     decided pose (:6954).
 * The same as uh_projmatch_match_prev -> look-ups -> uh_pnp_solve -> uh_projmatch_match -> exclusion, union, uh_filter_ambiguous,
 * look-ups -> uh_pnp_solve one after the other, bit for bit.  Look-ups: keypoint = the frame's undistorted keypoint, inv_sigma =
 * inv_sigma_levels[its octave]; first solve — the candidate's own position; second solve — the position of row prev_map_row[i] of `map`
 * when that is >= 0, else the candidate's own.  Weight, in both solves (pnpsolver.cpp:210-211): map_weight[prev_map_row[i]] for an item
 * with prev_map_row[i] >= 0, map_weight of its row for a map candidate, 1 for a previous-frame item outside the local map — this entry has
 * no input for those items' stability (uh_track_pose_stereo's prev_weight has).  Needs a device-resident frame (uh_orb_extract_frame_dev +
 * uh_projmatch_set_frame_dev, either tree builder) of <= 4096 keypoints; pm and pnp on the same context.  Refuses a prev_map_row outside
 * [-1, map->n) before anything is launched. */
typedef struct uh_track_args {
    const float* pose0;                 /* predicted pose f2g, row-major 4x4 */
    const float* intr4;                 /* fx fy cx cy */
    const float* inv_sigma_levels;      /* n_levels: 1 / scaleFactor per octave (the solver's per-match inv_sigma) */
    int32_t n_levels;
    const uh_prev_points* prev;         /* candidates of the previous-frame search */
    const int32_t* prev_map_row;        /* prev->n: row of the same map point in `map`, or -1; NULL = all -1 */
    const uh_map_points* map;           /* candidates of the local-map search */
    const float* map_weight;            /* map->n: the solver weight of each map point (0.5 for unstable ones); NULL = all 1 */
    float prev_min_desc_dist, prev_max_repj_dist;   /* system.cpp:6559-6565: maxDescDistance * 1.5, projDistThr */
    float map_min_desc_dist, map_radius_tracked, map_radius_lost;   /* :6762-6881: maxDescDistance * 2, 4 px, projDistThr */
    int32_t min_inliers;                /* 30: the first solve runs with MORE matches than this, the frame is tracked with MORE inliers */
} uh_track_args;
typedef struct uh_track_result {
    uh_dmatch* matches_prev; uint8_t* bad_prev; int32_t cap_prev;    /* in: buffers (>= prev->n); out: the first search's matches and the first solve's outlier flags */
    uh_dmatch* matches_map; int32_t cap_map;                          /* >= map->n: the second search's own matches (points seen by the first search excluded) */
    uh_dmatch* matches_all; uint8_t* bad_all; int32_t cap_all;        /* >= prev->n + map->n: the union the second solve ran on, its outlier flags */
    int32_t n_prev, n_map, n_all, tracked, inliers1, inliers2;
    int32_t iters1[4], iters2[4];
    float pose1[16], pose2[16];
} uh_track_result;
int  uh_track_pose(uh_projmatch* pm, uh_pnp* pnp, const uh_track_args* args, uh_track_result* result);
/* uh_track_pose for stereo / RGB-D frames: both solves are uh_pnp_solve_stereo's, with depth[queryIdx] gathered per match on the device.
 *   depth        the frame's n keypoints: Frame::getDepth per keypoint (<= 0: none); NULL = monocular (the solves of uh_track_pose)
 *   bl           imageParams.bl; > 0 when any depth is > 0
 *   prev_weight  prev->n: the solver weight (MapPoint::isStable: 1 or 0.5) of each previous-frame item, or NULL (= uh_track_pose: weight 1
 *                for items outside the local map).  An item's weight in both solves is map_weight[prev_map_row] when that row is >= 0, else
 *                prev_weight[i] (pnpsolver.cpp:210-211 in every solvePnp call).
 * The caller passes the same weights as for monocular frames (the stereo edges double theirs inside the solver).  With depth == NULL and
 * prev_weight == NULL the results equal uh_track_pose's. */
typedef struct uh_track_stereo {
    const float* depth;
    float bl;
    const float* prev_weight;
} uh_track_stereo;
int  uh_track_pose_stereo(uh_projmatch* pm, uh_pnp* pnp, const uh_track_args* args, const uh_track_stereo* stereo, uh_track_result* result);
/* uh_track_pose_stereo for a host that runs with markers: the same markers enter BOTH solves as in uh_pnp_solve_markers (currentKeyFrame is
 * the same in both reference calls).  Everything else stays as documented above: the first solve runs only with MORE than min_inliers
 * matches, the frame is tracked iff that solve has MORE than min_inliers inliers (markers are never counted) — a host that wants a
 * marker-only pose for a frame with too few matches calls uh_pnp_solve_markers itself.  Still one wait and no extra launch.  stereo and
 * markers may each be NULL; markers == NULL or markers->n == 0 is uh_track_pose_stereo (uh_track_pose when stereo is NULL as well). */
int  uh_track_pose_markers(uh_projmatch* pm, uh_pnp* pnp, const uh_track_args* args, const uh_track_stereo* stereo /* or NULL */,
                           const uh_pnp_markers* markers /* or NULL */, uh_track_result* result);
/* test hook: the flattened kd-tree of the current frame (24-byte nodes {float divlow, divhigh; int32 left, right, leaf_begin;
 * int16 leaf_count, col}), the leaf index list, the root box {x.min, x.max, y.min, y.max} and the tree depth */
int  uh_projmatch_debug_tree(uh_projmatch* pm, int32_t* n_nodes, const void** nodes24, const uint32_t** leaf_idx,
                             double* root_box4, int32_t* max_depth);
/* the same build as a host-only function (no GPU needed): nodes24_out has room for 2n+2 nodes, leaf_idx_out for n entries */
int  uh_kdtree_build_host(const float* xy, int32_t n, int32_t* n_nodes, void* nodes24_out, uint32_t* leaf_idx_out,
                          double* root_box4, int32_t* max_depth);

/* ------------------------------------------------------------------------
 * Fuse search — one projection search of the mapper's search-and-fuse step (src/utils/mapmanager.cpp, the private member of MapManager
 * that returns vector<uint32_t> and takes Frame&: ORB-SLAM's SearchInNeighbors), the stage between the new map points and local BA.
 * The reference runs it once per neighbour keyframe with the new keyframe's points and once with every neighbour's points against the
 * new keyframe; each of those K + 1 searches is one call here, and the caller applies a call's events (fuseMapPoints /
 * addMapPointObservation, which rewrite normals, distances and descriptors) before the next: ucoslam_hip::MapPointFuser
 * (adaptors.hpp) and fuse.py's search_in_neighbors do exactly that.  Within one call no point depends on another.
 *
 * Per point of the table, in this order (status code of what ends it):
 *   1  skip[i] != 0 (the caller's tests: not a map point, bad, already observed in the searched frame)
 *   2  Frame::project(p, true, true) is NaN: depth < 0, or outside [min, max) of the image bounds (frame.h:140-159)
 *   3  dist = cv::norm(camera centre - p) < 0.8f * min or > 1.2f * max distance invariance (both ends are kept)
 *   4  MapPoint::getViewCos(camera centre) < 0.5 (mappoint.h:99)
 *   then level = predictScale(dist, max) of the NEW keyframe (predict_scale_factors[1], predict_n_levels; frame.h:129-136),
 *   radius = th * target scale_factors[level], times `widen` where viewCos < 0.98, Frame::getKeyPointsInRegion(p2d, radius, level - 1,
 *   level) in kd-tree order (frame.cpp:102-115), and the FIRST keypoint of the strictly smallest Hamming distance below
 *   (float)(max_desc_dist + 1e-3):
 *   0  found: best_kp / best_dist          5  none: best_kp = -1, best_dist = the threshold (as for codes 1-4)
 * The camera centre is Frame::getCameraCenter of pose_f2g (frame.h:189-197).  th = 0 means the reference's 2.5; widen is 1.4f for a
 * neighbour keyframe (first half) and 1 for the new keyframe (second half).
 *
 * The point table lives in pinned memory of the handle as 64-byte records: uh_fuse_set_points packs it once per keyframe insertion,
 * uh_fuse_update_points rewrites the rows the apply step changed (new_values holds n_rows points, the k-th for rows[k]).  ids is not read.
 * uh_fuse_search: `target` / `target_params` are the argument pair of uh_projmatch_set_frame_dev, with either tree builder; target ==
 * NULL uploads the host arrays of target_params into a frame object of the handle first (a utility path).  One launch, one wait, on the
 * context's stream.  uh_fuse_search_host is the same search on the calling core from host arrays (uh_kdtree_build_host's tree, no GPU
 * needed): the same three outputs bit for bit.
 *
 * Refused with UH_EINVAL before any launch: predict_n_levels > the target's n_levels (the reference would index past the target's
 * scaleFactors) or < 2, more than 16 target levels, a row outside the table, a device frame without a complete kd-tree, a tree deeper
 * than 62 levels, more than 4096 keypoints (what a device frame holds; both forms), more than uh_fuse_max_points() points.  A walk
 * stack overflow inside the launch is reported as UH_EINVAL as well, never as a result.
 * ------------------------------------------------------------------------ */
#define UH_FUSE_FOUND       0
#define UH_FUSE_SKIPPED     1
#define UH_FUSE_NO_PROJECT  2
#define UH_FUSE_DISTANCE    3
#define UH_FUSE_VIEW_COS    4
#define UH_FUSE_NO_KEYPOINT 5
typedef struct uh_fuse uh_fuse;
int  uh_fuse_create(uh_ctx* ctx, uh_fuse** out);
void uh_fuse_destroy(uh_fuse* f);
int32_t uh_fuse_max_points(void);
int  uh_fuse_set_points(uh_fuse* f, const uh_map_points* points);
int  uh_fuse_update_points(uh_fuse* f, int32_t n_rows, const int32_t* rows, const uh_map_points* new_values);
int  uh_fuse_search(uh_fuse* f, uh_dev_frame* target /* or NULL */, const uh_proj_frame* target_params, const float* pose_f2g /* row-major 4x4 */,
                    const float* predict_scale_factors, int32_t predict_n_levels, const uint8_t* skip /* n or NULL */, float th, float widen,
                    float max_desc_dist, int32_t* best_kp_out, float* best_dist_out, uint8_t* status_out);
int  uh_fuse_search_host(const uh_map_points* points, const uh_proj_frame* target_params, const float* pose_f2g, const float* predict_scale_factors,
                         int32_t predict_n_levels, const uint8_t* skip /* n or NULL */, float th, float widen, float max_desc_dist,
                         int32_t* best_kp_out, float* best_dist_out, uint8_t* status_out);

/* test hooks of the device builder (csrc/kdbuild.hpp): the same outputs from the build kernel (n <= 4096; threads 0 = default, 256 or
 * 512), and — host only — the permutation its restatement of libstdc++'s std::sort gives n float keys (compared with std::sort itself) */
int  uh_kdtree_build_dev(uh_ctx* ctx, const float* xy, int32_t n, int32_t threads, int32_t* n_nodes, void* nodes24_out, uint32_t* leaf_idx_out,
                         double* root_box4, int32_t* max_depth);
int  uh_kdtree_sort_restated_host(const float* keys, int32_t n, uint32_t* perm_out);

/* ------------------------------------------------------------------------
 * Measurement hooks (used by scripts/time_ba.py and scripts/knn_push_bench.py; not part of the drop-in surface).
 * uh_ba_debug_clocks: the 64 phase timestamps the BA kernels of the latest LM step left behind (100 MHz wall clock; slots in
 * csrc/ba.hip, UH_BA_CLK).  uh_knn_debug_push_cycles: shader cycles of n heap pushes at row width k for the cross-lane and the
 * scalar formulation of the result heap and an empty loop (out3[0..2]).
 * ------------------------------------------------------------------------ */
int uh_ba_debug_clocks(uh_ba* ba, int64_t* out64);
/* a background launch of a chosen character (0 sleeping waves, 1 integer VALU, 2 streaming loads over d_buf, 3 LDS traffic) on ctx's
 * stream, for scripts/time_interference.py: what about a neighbouring launch slows the latency-bound BA chain down */
int uh_debug_background(uh_ctx* ctx, int mode, int blocks, int iters, const void* d_buf, size_t buf_bytes, void* d_sink);
int uh_knn_debug_push_cycles(uh_knn* knn, int k, int n, long long* out3);
/* shader-clock stamps of the pose-only solves that follow (on = 1) — out512[0] kernel entry, [1] matches staged, [2] rounds done,
 * [3] results posted, [4] passes over the matches, [5 ..] per-pass stamps; out512 (may be NULL) receives the stamps of the last solve and
 * MUST hold 512 entries (4096 bytes: the whole stamp block is copied) */
int uh_pnp_debug_clocks(uh_pnp* pnp, int on, long long* out512);

/* ------------------------------------------------------------------------
 * Relocalisation RANSAC: PnPSolver::solvePnPRansac (src/optimization/pnpsolver.cpp:36-114), batched over the candidate keyframes of one
 * lost frame (System::relocalize runs it once per candidate) and over the hypotheses of each.  Lives on the uh_pnp object.
 *
 * Per problem and iteration `it`: the four matches samples[4 it .. 4 it + 3] give a three-point pose (the reference calls cv::solvePnP
 * with SOLVEPNP_P3P): EVERY real solution with positive point distances of the three-point problem of samples 0-2 on pixels normalised
 * with intr4, in double; among them the one with the smallest squared reprojection error of sample 3 (normalised coordinates, double),
 * the lowest solution index on ties, solutions numbered in ascending (distance of sample 2) / (distance of sample 0).  No solution —
 * no real root, coincident or collinear sample points (sin^2 of the angle at sample 0 below 1e-16), non-finite sample data: the
 * iteration is skipped and its count is -1.  The pose goes matrix -> Rodrigues vector in double (direct axis-angle extraction, own
 * branches below sin(theta) = 1e-5), then through Se3Transform(rv, tv): cast to float rt[6], the 3x4 built in float in the written order
 * (se3transform.h:143-176; cos / sin in double on the float angle, rounded once).  Every match j is then tested as :75-100 do it, in
 * float in the written order: inlier iff distX * distX + distY * distY < 5.99f and not getViewCos(camCenter) < 0.5.  There is no test of
 * the depth's sign (a point behind the camera can be an inlier); a zero depth gives inf / NaN and a false comparison.  The FIRST
 * iteration with the strictly largest count >= 1 wins: rt6 / pose are its pose and inliers its inliers in ascending j; ok = 1 iff it has
 * at least 4.  With fewer the pose is STILL the winner's (the reference overwrites posef2g_io before it returns false); with no winner
 * rt6 = rt6_in.  pose = Se3Transform::set(rt6), 4x4 row-major.
 * UNPINNED (no OpenCV exists in the build container): (a) the three-point solver — any method meeting the contract above gives the same
 * answers up to rounding on well-conditioned samples; the closed form used is in csrc/p3p_math.hpp; (b) cv::Rodrigues re-orthonormalises
 * by SVD first; (c) whether the unqualified cos / sin of se3transform.h:157-158 are the double or the float functions; (d) OpenCV 4 orders
 * the solutions by the error over all four points, OpenCV 3 by the fourth.
 * One packed upload, two launches (whatever the number of problems), one download, ONE wait on the context's stream.  A problem with
 * n < 4 is valid: ok = 0, n_inliers = 0, best_iter = -1, rt6 = rt6_in, counts all -1, and nothing is launched for it.  Refused with
 * UH_EINVAL before anything is launched: NULL arrays with n > 0, cap < n, a sample index outside [0, n), an index twice within one
 * sample, n / iters / n_problems beyond the caps below, iters < 1, non-finite intrinsics.  Non-finite coordinates are NOT refused: they
 * are scored as the reference scores them.  The hypothesis masks live in device scratch of the uh_pnp object: 8 * ceil(n / 64) bytes per
 * hypothesis (128 MiB when every cap is reached at once).
 * ------------------------------------------------------------------------ */
#define UH_RANSAC_MAX_PROBLEMS 64
#define UH_RANSAC_MAX_ITERS    1024
#define UH_RANSAC_MAX_MATCHES  16384
typedef struct uh_ransac_problem {      /* one candidate keyframe */
    int32_t n;                          /* matches; < 4 is valid and gives ok = 0 without a launch for it */
    const float* p3d;                   /* n x 3  MapPoint::getCoordinates() */
    const float* normal;                /* n x 3  MapPoint normal (getViewCos) */
    const float* kp;                    /* n x 2  und_kpts[queryIdx].pt */
    int32_t iters;                      /* maxIters, 1..UH_RANSAC_MAX_ITERS */
    const int32_t* samples;             /* iters x 4 indices into the matches */
    const float* rt6_in;                /* posef2g_io as it goes in (rvec, tvec) */
} uh_ransac_problem;
typedef struct uh_ransac_result {
    int32_t ok, n_inliers, best_iter;   /* best_iter = -1: no hypothesis had an inlier */
    float rt6[6], pose[16];
    int32_t* inliers; int32_t cap;      /* in: buffer of >= n entries */
    int32_t* counts;                    /* iters entries or NULL: count per hypothesis, -1 = skipped */
} uh_ransac_result;
int uh_pnp_ransac(uh_pnp* pnp, const float* intr4, int n_problems, const uh_ransac_problem* problems, uh_ransac_result* results);
/* Host code: the samples the reference draws for n matches and `iters` iterations — std::random_shuffle of libstdc++ on ONE index vector
 * that starts as the identity and carries its permutation from one iteration to the next (for i in 1..n-1: j = rand() % (i + 1), swap),
 * the first four entries after each shuffle.  Draws (n - 1) * iters numbers from libc rand(): a host that calls srand as the reference's
 * process would gets the reference's samples, and rand()'s state ends where the reference leaves it.  n >= 4. */
int uh_pnp_ransac_samples(int n, int iters, int32_t* samples_out /* iters x 4 */);
/* test hook: ONE hypothesis of a problem on the device, every solution in double (R row-major then t, 12 per solution), the pick
 * (-1: skipped) and the chosen (rvec, tvec) before its cast to float */
int uh_pnp_ransac_debug_hypothesis(uh_pnp* pnp, const float* intr4, const uh_ransac_problem* problem, int iter,
        int32_t* n_solutions, double* Rt_4x12 /* every solution */, int32_t* chosen, double* rvec_tvec6);
/* measurement hook (scripts/time_pnp_ransac.py): uniform_roots = 1 makes the calls that follow run the form of the hypothesis kernel in which
 * every lane takes all four roots one after the other; 0 (the default) the form with one root per lane.  The results are equal bit for bit. */
int uh_pnp_ransac_debug_form(uh_pnp* pnp, int uniform_roots);
/* test hook: the real roots of n <= UH_RANSAC_MAX_ITERS quartics A0 + A1 v + .. + A4 v^4 (A_nx5, five doubles each) as the hypothesis kernel's
 * root finder returns them, one launch, one lane per quartic: ascending, the absent ones +inf, and their number */
int uh_pnp_ransac_debug_roots(uh_pnp* pnp, int n, const double* A_nx5, double* roots_nx4, int32_t* n_roots);

/* ------------------------------------------------------------------------
 * System::relocalize's pose search (src/utils/system.cpp ~4950-5500) for ALL candidate keyframes of one lost frame as ONE call
 * (csrc/relocalize.hpp): what uh_pnp_ransac -> per survivor uh_projmatch_match -> id -> row look-ups -> uh_pnp_solve give one after the
 * other, bit for bit, on the device between the launches with ONE wait on the context's stream at the end.  The number of launches does
 * not depend on n_candidates.  Per candidate c, in the caller's order:
 *   - fewer than min_matches_ransac matches: the candidate takes no part (no RANSAC problem, no samples drawn)      stage UH_RELOC_FEW_MATCHES
 *   - solvePnPRansac over its matches; the count afterwards is n_inliers when ok, else ALL its matches (the reference ignores the return
 *     value and a failed call leaves the list untouched); fewer than min_matches_after_ransac stops it              stage UH_RELOC_FEW_AFTER_RANSAC
 *   - Map::matchFrameToMapPoints over `points` from the RANSAC result's pose (the winner's even when ok == 0; Se3Transform(rt6_in) when no
 *     hypothesis had an inlier), radius map_radius, after filter_ambiguous_query; fewer than min_matches_map stops it   stage UH_RELOC_FEW_MAP
 *   - PnPSolver::solvePnp (monocular) from that pose over those matches: p3d = the matched row of `points`, kp = the frame's undistorted
 *     keypoint, inv_sigma = inv_sigma_levels[its octave], weight = weight[row]; n_good = matches with bad == 0; fewer than min_good stops
 *     it                                                                                                            stage UH_RELOC_FEW_GOOD
 *   - else                                                                                                           stage UH_RELOC_SOLVED
 * best = the solved candidate with the strictly largest n_good (the first on ties), -1 without one; pose / n_matches are its pose_solve / n_good.
 * Preconditions as uh_track_pose: a device-resident frame (uh_orb_extract_frame_dev or uh_dev_frame_upload, then
 * uh_projmatch_set_frame_dev with either tree builder) of <= 4096 keypoints; pm and pnp on one context.
 * samples == NULL: the call draws them itself with the routine behind uh_pnp_ransac_samples, in candidate order and only for candidates
 * that pass the first gate, so libc rand() ends where the chain of single calls leaves it.
 * Fields of a stage a candidate never reached keep NEUTRAL values: ok = n_inliers = n_map = solve_inliers = n_good = 0, best_iter = -1,
 * iters = {0,0,0,0}, rt6 / pose_ransac / pose_solve all zero, nothing written to inliers / matches_map / bad.  (A candidate stopped at
 * UH_RELOC_FEW_MAP has its matches_map; bad, pose_solve, iters, solve_inliers and n_good are neutral.)
 * Refused with UH_EINVAL before anything is launched: NULL arrays with n > 0, a query_idx outside the frame's keypoints, cap_map below
 * min(points->n, keypoints) or cap_inliers below n (with a non-NULL inliers), what uh_pnp_ransac refuses for samples, sizes and intrinsics
 * (max_iters outside 1..UH_RANSAC_MAX_ITERS, n beyond UH_RANSAC_MAX_MATCHES, n_candidates outside 0..UH_RANSAC_MAX_PROBLEMS), n_levels
 * outside 1..16, a map_radius <= 0, a frame that is not device-resident or has more than 4096 keypoints.  Non-finite coordinates are not
 * refused (see uh_pnp_ransac).  n_candidates == 0 is valid: best = -1, nothing is launched.
 * ------------------------------------------------------------------------ */
enum { UH_RELOC_FEW_MATCHES = 0, UH_RELOC_FEW_AFTER_RANSAC = 1, UH_RELOC_FEW_MAP = 2, UH_RELOC_FEW_GOOD = 3, UH_RELOC_SOLVED = 4 };
typedef struct uh_reloc_args {
    const float* intr4;                 /* fx fy cx cy */
    const float* inv_sigma_levels;      /* n_levels: 1 / scaleFactor per octave */
    int32_t n_levels;
    float map_min_desc_dist;            /* 2 x maxDescDistance */
    float map_radius;                   /* 2.5 */
    int32_t max_iters;                  /* 50: RANSAC iterations per candidate */
    int32_t min_matches_ransac, min_matches_after_ransac, min_matches_map, min_good;   /* 25, 15, 30, 30: a count BELOW the gate stops the candidate */
} uh_reloc_args;
typedef struct uh_reloc_candidate {
    int32_t n;                          /* matches of the lost frame against this keyframe */
    const int32_t* query_idx;           /* n: DMatch::queryIdx, the frame's keypoint */
    const float* p3d;                   /* n x 3: the matched map point's coordinates */
    const float* normal;                /* n x 3: its normal */
    const float* rt6_in;                /* the keyframe's pose_f2g as (rvec, tvec) */
    const int32_t* samples;             /* max_iters x 4, or NULL: drawn by the call */
    const uh_map_points* points;        /* the candidate's own point list (getNeighborsVLevel2(kf, true)); n == 0 is valid */
    const float* weight;                /* points->n: the solver weight per point (0.5 for unstable ones); NULL = all 1 */
} uh_reloc_candidate;
typedef struct uh_reloc_step {          /* per candidate; in: the buffers and their capacities */
    int32_t stage;                      /* UH_RELOC_* */
    int32_t ok, n_inliers, best_iter;   /* solvePnPRansac's result */
    float rt6[6], pose_ransac[16];
    int32_t* inliers; int32_t cap_inliers;    /* NULL, or >= n entries: the winner's inliers, ascending */
    int32_t n_map;                      /* matches of the projection search; trainIdx = the point's id */
    uh_dmatch* matches_map; uint8_t* bad; int32_t cap_map;   /* >= min(points->n, the frame's keypoints) entries each (may be NULL when that is 0) */
    float pose_solve[16];
    int32_t iters[4], solve_inliers, n_good;
} uh_reloc_step;
typedef struct uh_reloc_result {
    int32_t best;                       /* winning candidate or -1 */
    float pose[16];                     /* its pose_solve (all zero when best == -1) */
    int32_t n_matches;                  /* its n_good (0 when best == -1) */
    uh_reloc_step* steps;               /* n_candidates entries */
} uh_reloc_result;
int uh_relocalize_pose(uh_projmatch* pm, uh_pnp* pnp, const uh_reloc_args* args, int n_candidates, const uh_reloc_candidate* cands,
                       uh_reloc_result* result);

/* ------------------------------------------------------------------------
 * Test hooks: ONE reduced-system solve S x = b (fp64 L D L^T without pivoting) in a chosen production form, on a system the caller gives.
 * The hooks load [S; b^T] into the layout the form expects and call the device functions (form 7: the launches) the optimisers call;
 * no problem has to be set.  S is n x n row-major and only its lower triangle is read; n = 6 nfree for the bundle adjustment.
 *   form 1  row per lane, as the persistent kernel runs it          nfree 1..10     5  packed triangle in LDS, MFMA update   nfree 1..32
 *   form 2  two rows per lane, as the persistent kernel runs it     nfree 11..16    6  row stride in HBM, MFMA update        nfree 1..64
 *   form 3  row per lane, the launch chain's fused solve            nfree 1..10     7  blocked, 64-column panels (wide form) nfree 1..341
 *   form 4  two rows per lane, the launch chain's fused solve       nfree 11..21
 * x [n]: the solution, all zeros where the solve failed.  failed: 1 where a pivot was zero or not finite (the optimisers reject the trial).
 * LD [(n + 1) x (n + 1)] row-major (may be NULL): the form's matrix as the factorisation leaves it — L strictly below the diagonal, row n =
 * z = D^-1 L^-1 b (form 7 substitutes in that row, panel by panel from the last: only the last 64-column panel's part of it is still z).
 * The diagonal holds D in forms 5, 6, 7; forms 1-4 do not keep D.  On and above the diagonal, and in column n, the forms leave
 * what their updates happened to write (forms 2, 4: zeros on and above the diagonal of rows 0 .. n - 1; forms 5, 7: untouched words);
 * the words the hook did not load from S and b are set to NaN beforehand in forms 1-6 (production leaves them uninitialised) and to zero in
 * form 7 (production clears the matrix).  UH_EINVAL, nothing launched: a form outside 1..7, nfree outside the form's range, a NULL array.
 * uh_posegraph_debug_solve: the same for the pose graph's blocked solve with its skip of empty 64-row groups (csrc/dense_ldlt.hpp), any
 * 1 <= n <= 4096; LD as in form 7; x is whatever the substitution gave where the solve failed (the optimiser rejects that trial unseen).
 * ------------------------------------------------------------------------ */
int uh_ba_debug_solve(uh_ba* ba, int form, int nfree, const double* S, const double* b, double* x, double* LD, int* failed);
int uh_posegraph_debug_solve(uh_posegraph* pg, int n, const double* S, const double* b, double* x, double* LD, int* failed);

/* ------------------------------------------------------------------------
 * Map initialiser: MapInitializer's two-view "initialise" (src/utils/mapinitializer.cpp:152-201, ORB-SLAM's Initializer) — 200 homography
 * and 200 fundamental hypotheses from 8-point samples, each scored over every match, the model choice RH = SH / (SH + SF) > 0.40, the
 * decomposition of the chosen model into eight or four (R, t) candidates, and one triangulate-and-check pass (CheckRT) per candidate.
 * The keypoint route only; what the caller _9813592252344743680 adds (pose = [R | t * min_distance]) is included.
 *
 * A match is (train, query): train indexes kp1 (the reference frame), query indexes kp2.  Per hypothesis the eight matches
 * samples[8 it .. 8 it + 7] give the normalised 8-point system (both normalisations are sequential float sums over ALL keypoints of a frame,
 * taken on the host), its null vector in double, the de-normalised float model, and the reference's sequential float score in match
 * order with the inlier mask.  The FIRST hypothesis with the strictly largest score > 0 wins for each model.  States per match of the
 * winning candidate: 0 not an inlier of the chosen model, 1 rejected by CheckRT, 2 counted with cosine >= 0.99998 (its point is stored,
 * the keypoint is not marked triangulated), 3 counted and good, 4 non-finite triangulation (the keypoint's flag is CLEARED).  The
 * per-keypoint scatter runs on the host in match order, so duplicate reference keypoints resolve as in the reference's loop.
 * The arithmetic, its float conventions, the SIGN RULE for singular vectors and what is UNPINNED are in csrc/mapinit_math.hpp.
 * One upload, two launches, one download, ONE wait.  n_matches < min_matches: ok = 0 without a launch.  A chosen model without a
 * winning hypothesis (the reference would hand an empty matrix to OpenCV) gives ok = 0, winner = -1.
 * Refused with UH_EINVAL before any launch: min_matches < 8, iterations outside [1, UH_MAPINIT_MAX_ITERS], more than
 * UH_MAPINIT_MAX_MATCHES matches, a match index outside its keypoint array, a sample index outside [0, n_matches), NULL arrays,
 * non-finite intrinsics or sigma <= 0, a result buffer below its stated size.
 * uh_mapinit_run_host is the same function on the calling core (no GPU needed): equal bit for bit in everything but the parallaxes
 * (acos of the host's libm against the device's).
 * ------------------------------------------------------------------------ */
#define UH_MAPINIT_MAX_ITERS    1024
#define UH_MAPINIT_MAX_MATCHES  16384
#define UH_MAPINIT_NONE         0
#define UH_MAPINIT_HOMOGRAPHY   1
#define UH_MAPINIT_FUNDAMENTAL  2
typedef struct uh_mapinit uh_mapinit;
typedef struct uh_mapinit_args {
    const float* intr4;                    /* fx, fy, cx, cy of the undistorted camera */
    const float* kp1; int32_t n_kp1;       /* n_kp1 x 2  und_kpts of the reference frame */
    const float* kp2; int32_t n_kp2;       /* n_kp2 x 2  und_kpts of the second frame */
    const int32_t* matches; int32_t n_matches;   /* n_matches x 2  (trainIdx -> kp1, queryIdx -> kp2) */
    float sigma;                           /* 1.0 */
    int32_t iterations;                    /* 200 */
    int32_t min_matches;                   /* 50 (minNumMatches), at least 8 */
    float min_parallax;                    /* 1.0 */
    int32_t min_triangulated;              /* 50 */
    float min_distance;                    /* Params::minDistance: the baseline the unit translation is scaled to */
    const int32_t* samples;                /* iterations x 8 indices into the matches, or NULL: drawn as uh_mapinit_samples draws them */
} uh_mapinit_args;
typedef struct uh_mapinit_result {
    int32_t ok, model, winner;             /* model: UH_MAPINIT_*; winner: index of the chosen (R, t) candidate or -1 */
    int32_t best_h, best_f;                /* winning hypothesis of each model, -1: none scored above 0 */
    float score_h, score_f, rh;
    int32_t n_candidates, n_inliers;       /* 8 / 4 (0: ReconstructH's singular-value exit); inliers N of the chosen model */
    int32_t n_good[8]; float parallax[8];  /* per candidate, in the written order */
    float R[9], t[3], pose[16];            /* the winner's (unit t); pose = [R | t * min_distance], row-major 4x4; zeros unless ok */
    int32_t n_out;                         /* surviving matches */
    int32_t* matches_out;                  /* in: buffer of n_matches x 2 */
    float* points_out;                     /* in: buffer of n_matches x 3, the survivors' points in match order */
    uint8_t* triangulated;                 /* in: n_kp1 bytes or NULL (vbTriangulated) */
    float* p3d;                            /* in: n_kp1 x 3 or NULL (vP3D) */
    uint8_t* state;                        /* in: n_matches bytes or NULL, the per-match states above */
    int32_t* index_out;                    /* in: n_matches entries or NULL: each survivor's index into the input matches */
    int32_t cap_matches;                 /* in: entries of matches_out / points_out / state (>= n_matches) */
} uh_mapinit_result;
int  uh_mapinit_create(uh_ctx* ctx, uh_mapinit** out);
void uh_mapinit_destroy(uh_mapinit* mi);
int  uh_mapinit_run(uh_mapinit* mi, const uh_mapinit_args* args, uh_mapinit_result* result);
int  uh_mapinit_run_host(const uh_mapinit_args* args, uh_mapinit_result* result);
/* Host code: the reference's draw (:167-182).  Calls srand(0) — as the reference does inside this function — and then draws 8 * iterations
 * numbers from libc rand(): per iteration the available list is reset to the identity and eight times j = rand() % size is taken and
 * overwritten with the last entry.  SIDE EFFECT: rand()'s state is reseeded and ends where the reference leaves it.  n >= 8. */
int  uh_mapinit_samples(int32_t n, int32_t iterations, int32_t* samples_out /* iterations x 8 */);
/* test hook: ONE hypothesis from the device (model UH_MAPINIT_HOMOGRAPHY / _FUNDAMENTAL): the de-normalised matrix taken in double from the
 * device's double null vector (H21 = T2^-1 Hn T1; F21 = T2^T rank2(Fn) T1), the float matrix the score used, the score and the mask
 * (ceil(n_matches / 64) words, bit j % 64 of word j / 64 = match j) */
int  uh_mapinit_debug_hypothesis(uh_mapinit* mi, const uh_mapinit_args* args, int32_t model, int32_t iter, double* M9_double, float* M9_float,
                                 float* score, uint64_t* mask_words);
/* test hook: the SECOND launch alone on a planted winner — the float model matrix M9 (H21 or F21) and its inlier mask (words as above) take
 * the place of the hypotheses' winner (iterations is read as 1; the result's scores are 1 and 0, best_h / best_f are 0 and -1).  It reaches
 * states no keypoint input can: a non-finite coordinate never is an inlier of a scored hypothesis (its chi-square is inf or NaN, and it
 * spoils the frame's normalisation), and a finite one triangulates to a finite point.  mi = NULL runs the host form. */
int  uh_mapinit_debug_reconstruct(uh_mapinit* mi, const uh_mapinit_args* args, int32_t model, const float* M9, const uint64_t* mask_words,
                                  uh_mapinit_result* result);

#ifdef __cplusplus
}
#endif
#endif /* UCOSLAM_HIP_H */
