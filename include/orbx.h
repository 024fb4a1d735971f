/*
 * orbx.h -- C ABI of the MI355X-native ORB extraction + Hamming matching library
 * (liborbx.so, built from orbslam2commentedbyxcm_amd/csrc/).
 *
 * This is the drop-in boundary for ORB-SLAM2's per-frame hot path.  Every entry
 * point names the reference interface it replaces (paths relative to the
 * reference repository, xcmworkharder/OrbSlam2CommentedByXcm):
 *
 *   ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 *       include/ORBextractor.h:93, src/ORBextractor.cc:438-550  -> orbx_extractor_create
 *   ORBextractor::operator()(image, mask, keypoints, descriptors)
 *       include/ORBextractor.h:111, src/ORBextractor.cc:1513-1629 -> orbx_extract,
 *       orbx_extract_batch, orbx_extract_batch_device
 *   ORBextractor::Get{Levels,ScaleFactor,ScaleFactors,InverseScaleFactors,
 *       ScaleSigmaSquares,InverseScaleSigmaSquares}
 *       include/ORBextractor.h:119-159                              -> orbx_extractor_levels
 *   ORBextractor::mvImagePyramid (public member read by Frame::ComputeStereoMatches)
 *       include/ORBextractor.h:162, src/Frame.cc:682,782,810,816    -> orbx_pyramid_level
 *   ORBmatcher::DescriptorDistance(a, b)
 *       include/ORBmatcher.h:65, src/ORBmatcher.cc:1983-2003        -> orbx_hamming,
 *       orbx_hamming_matrix_device
 *   ORBmatcher candidate scoring inside SearchByProjection / SearchForTriangulation
 *       src/ORBmatcher.cc:61-173, 1620-1789, 1792-1924, 850-1056     -> orbx_window_match
 *
 * Conventions: every function returns an int status (ORBX_OK = 0, ORBX_EMPTY = 1
 * for the reference's silent empty-image no-op, negative on error) and never
 * throws.  All pointers are plain host or device pointers; no C++ or torch types
 * cross this boundary.  One extractor owns one HIP stream and is not re-entrant
 * (like the reference's stateful ORBextractor); distinct extractors may be used
 * from distinct threads concurrently (Frame.cc:127-131).
 */
#ifndef ORBX_H
#define ORBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_OK 0
#define ORBX_EMPTY 1
#define ORBX_ERR_ARG -1
#define ORBX_ERR_HIP -2
#define ORBX_ERR_CAPACITY -3
#define ORBX_ERR_UNSUPPORTED -4
#define ORBX_ERR_STATE -5

#define ORBX_MAX_LEVELS 32

/* Binary-identical to cv::KeyPoint {Point2f pt; float size, angle, response; int octave, class_id;} */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbx_keypoint;

/* The five YAML parameters of Tracking.cc:129-149 (ORBextractor.{nFeatures,scaleFactor,
 * nLevels,iniThFAST,minThFAST}). */
typedef struct {
    int nfeatures;
    float scale_factor;
    int nlevels;
    int ini_th_fast;
    int min_th_fast;
} orbx_extractor_params;

typedef struct orbx_extractor orbx_extractor;

/* ORBextractor::ORBextractor.  Selects HIP device `device`, creates one stream. */
int orbx_extractor_create(const orbx_extractor_params* params, int device, orbx_extractor** out);
void orbx_extractor_destroy(orbx_extractor* ex);

/* GetLevels/GetScaleFactors/...: each non-null array receives nlevels floats. */
int orbx_extractor_levels(const orbx_extractor* ex, int* nlevels, float* scale, float* inv_scale,
                          float* sigma2, float* inv_sigma2);
/* mnFeaturesPerLevel (ORBextractor.h:212): nlevels ints. */
int orbx_extractor_features_per_level(const orbx_extractor* ex, int* features);

/* Upper bound on keypoints one W x H frame can produce (size `cap` with it). */
int orbx_extractor_max_keypoints(orbx_extractor* ex, int width, int height, int* max_kps);

/* ORBextractor::operator() on one host image (row stride in bytes).  Keypoints in
 * the reference order (level-major, octree-list order), coordinates scaled to level
 * 0; descriptors n x 32 bytes.  Returns ORBX_EMPTY (outputs untouched) for an empty
 * image, ORBX_ERR_CAPACITY if more than `cap` keypoints were found (*n_out then
 * holds the required count).  Frame size: pyramid levels under 62 px on a side hold no
 * FAST cell and keep no keypoints, as in the reference (ORBextractor.cc:1047-1085); a
 * frame with a level under 33 px returns ORBX_ERR_UNSUPPORTED (the reference's
 * DistributeOctTree divides by a zero or negative size there, cc:674-676), as do
 * levels over 4096 px and aspect ratios beyond 16 octree roots. */
int orbx_extract(orbx_extractor* ex, const uint8_t* img, int width, int height, size_t stride,
                 orbx_keypoint* kps, uint8_t* desc, int cap, int* n_out);

/* Wall time (microseconds) of the newest orbx_extract / orbx_extract_batch host call on
 * `ex`, entry to return: what a C++ caller pays per call (diagnostics; -1 for NULL). */
double orbx_extractor_last_call_us(const orbx_extractor* ex);

/* The same for B host images of one size; frame b writes kps[b*cap ...],
 * desc[b*cap*32 ...] and n_per_frame[b]. */
int orbx_extract_batch(orbx_extractor* ex, int batch, const uint8_t* const* imgs, int width,
                       int height, size_t stride, orbx_keypoint* kps, uint8_t* desc, int cap,
                       int* n_per_frame);

/* Device-resident fast path: d_imgs holds B frames (frame b at d_imgs + b*frame_pitch,
 * rows `stride` bytes apart) already in HBM; outputs are device pointers as above.
 * Work is enqueued on the extractor's stream (or on `stream` if non-null, a
 * hipStream_t) and the call returns without synchronising.  n_per_frame[b] receives
 * the full count even when it exceeds cap (only cap keypoints are then written). */
int orbx_extract_batch_device(orbx_extractor* ex, int batch, const uint8_t* d_imgs,
                              size_t frame_pitch, int width, int height, size_t stride,
                              orbx_keypoint* d_kps, uint8_t* d_desc, int cap, int* d_n_per_frame,
                              void* stream);

/* The extractor's hipStream_t (as void*). */
void* orbx_extractor_stream(orbx_extractor* ex);

/* Scheduling hook for running other work beside a batched extraction (no reference
 * counterpart): from now on every extraction records `*event` (a hipEvent_t owned by the
 * extractor) on its stream right after stage `stage` -- 1 pyramid, 2 blur + FAST
 * strength, 3 FAST cells, 4 octree; 0 stops recording.  orbx_stream_wait_event makes
 * another stream wait for the latest record (hipStreamWaitEvent). */
int orbx_extractor_set_stage_event(orbx_extractor* ex, int stage, void** event);
int orbx_stream_wait_event(void* stream, void* event);

/* A HIP stream on `device`.  cu_stride k > 1: its kernels run only on compute units 0,
 * k, 2k, ... (hipExtStreamCreateWithCUMask: default priority, and a blocking stream --
 * it synchronises with the null stream, so a caller that issues null-stream work beside
 * it serialises against it); otherwise a non-blocking stream from
 * hipStreamCreateWithPriority with `priority` (HIP's range: lower numbers are higher
 * priorities; 0 = default).  The batched front end creates its matcher
 * stream with it before the extraction lanes' streams, so that the three busy streams
 * get hardware queues of their own.  No reference counterpart:
 * ORB-SLAM2 tracks one frame at a time.  Release with orbx_stream_destroy. */
int orbx_stream_create(int device, int cu_stride, int priority, void** stream);
int orbx_stream_destroy(void* stream);

/* Kernel status of the last extraction (any path), per frame: 0 = complete; bit 0
 * (ORBX_STATUS_NODE_OVERFLOW) = an octree level needed more nodes than its capacity
 * (or held more than 65535 FAST keypoints, the octree's u16 counters),
 * bit 1 (ORBX_STATUS_ITERATIONS) = an octree loop hit its iteration guard; either way
 * that frame's keypoints are truncated and differ from the reference's DistributeOctTree
 * (ORBextractor.cc:667-1013).  The host paths (orbx_extract, orbx_extract_batch) turn a
 * non-zero status into ORBX_ERR_STATE; orbx_extract_batch_device returns before the
 * kernels run, so its callers read the status here.  Synchronises with the last
 * extraction's stream; flags (nullable) receives `batch` ints, *any their OR. */
#define ORBX_STATUS_NODE_OVERFLOW 1
#define ORBX_STATUS_ITERATIONS 2
int orbx_extractor_status(orbx_extractor* ex, int batch, int* flags, int* any);
/* The same without synchronising: the device array of per-frame status words (int32
 * [last batch]), valid after the last extraction's stream reaches that point and until
 * the next extraction. */
int orbx_extractor_status_device(orbx_extractor* ex, const int32_t** d_status);
/* Test hook: cap every level's octree node capacity at `cap` (0 = the bound the
 * reference's algorithm guarantees, max(N+4, 4*nIni+4) per level), so that the overflow
 * status can be exercised.  Frees the extractor's buffers (pyramids included) after
 * draining the whole device; takes effect at the next extraction. */
int orbx_extractor_set_node_capacity(orbx_extractor* ex, int cap);

/* Level 0 of the pyramid is the input image (ORBextractor.cc:1688-1690).  With enable = 1,
 * orbx_extract_batch_device reads it in place from the caller's device frames instead of
 * copying it into the extractor's pyramid (when the frames are 16-byte aligned, their
 * frame pitch a multiple of 16 and their row stride a multiple of 64; otherwise it is
 * copied as before).  The frames must then stay unchanged while the pyramid is in use:
 * orbx_pyramid_level(_device) returns level 0 from them, and the stereo matchers
 * (orbx_compute_stereo_matches(_batch_device)) read the octave-0 SAD windows of
 * Frame::ComputeStereoMatches (Frame.cc:800-835) there.  Frames in a pitched layout
 * (rows a multiple of 64 bytes apart) qualify at any width. */
int orbx_extractor_set_level0_in_place(orbx_extractor* ex, int enable);

/* Per-stage HIP-event timing (ms) of extraction calls, averaged over the (up to 64)
 * most recent calls made since orbx_extractor_set_timing(ex, 1), which also resets the
 * average.  Events are recorded on the launch stream between the stages, so a timed
 * loop is measured without synchronising inside it.  Names are static strings.
 * enable = 2 + s (s = 0 pyramid .. 4 describe) records only stage s's two boundary events
 * (each recorded event costs the pipelined step ~0.2 %: bench.py times one stage live);
 * stage_times then returns that stage alone. */
int orbx_extractor_set_timing(orbx_extractor* ex, int enable);
int orbx_extractor_stage_times(orbx_extractor* ex, int max_stages, const char** names, float* ms,
                               int* n_stages);

/* mvImagePyramid[level] of frame `frame` of the last extraction: copies the level
 * ROI (w x h) into host memory `dst` with row stride dst_stride. */
int orbx_pyramid_level(orbx_extractor* ex, int frame, int level, uint8_t* dst, size_t dst_stride,
                       int* w, int* h);
/* Device pointer + row pitch of a pyramid level of the last device extraction. */
int orbx_pyramid_level_device(orbx_extractor* ex, int frame, int level, const uint8_t** d_ptr,
                              size_t* pitch, int* w, int* h);

/* ORBmatcher::DescriptorDistance on two 32-byte host descriptors; returns 0..256. */
int orbx_hamming(const uint8_t* a32, const uint8_t* b32);

/* dist[i*nb + j] = Hamming(a_i, b_j) for device descriptor arrays (32 B rows). */
int orbx_hamming_matrix_device(const uint8_t* d_a, int na, const uint8_t* d_b, int nb,
                               int32_t* d_dist, void* stream);

/* Windowed candidate scoring shared by the SearchByProjection overloads and
 * SearchForTriangulation: for query q (32 B descriptor at d_qdesc + 32*q) the
 * candidates are d_cand[d_cand_off[q] .. d_cand_off[q+1]) (indices into the target
 * descriptor array, in the reference's iteration order).  Outputs per query:
 * best/second-best distance, best candidate position (index into the target array,
 * -1 if none), and the target levels of best and second (as SearchByProjection
 * tracks them, ORBmatcher.cc:140-152).  `tie_last` = 0: strict < keeps the first
 * equal candidate (SearchByProjection); 1: the last equal candidate wins the best
 * slot (SearchForTriangulation, ORBmatcher.cc:955).  Device pointers, async. */
int orbx_window_match_device(const uint8_t* d_qdesc, int nq, const uint8_t* d_tdesc,
                             const int32_t* d_tlevel, const int32_t* d_cand_off,
                             const int32_t* d_cand, int tie_last, int32_t* d_best_idx,
                             int32_t* d_best_dist, int32_t* d_best_level, int32_t* d_second_dist,
                             int32_t* d_second_level, void* stream);

/* Host-pointer convenience wrapper of orbx_window_match_device (synchronous). */
int orbx_window_match(int device, const uint8_t* qdesc, int nq, const uint8_t* tdesc, int nt,
                      const int32_t* tlevel, const int32_t* cand_off, const int32_t* cand,
                      int tie_last, int32_t* best_idx, int32_t* best_dist, int32_t* best_level,
                      int32_t* second_dist, int32_t* second_level);

/* ------------------------------------------------------------------ matcher */

/* The Frame / KeyFrame fields the ORBmatcher functions read (include/Frame.h,
 * include/KeyFrame.h), as plain host arrays. */
typedef struct {
    int n;                       /* N */
    const orbx_keypoint* keys;   /* mvKeysUn */
    const uint8_t* desc;         /* mDescriptors, n x 32 */
    const float* u_right;        /* mvuRight (n) or NULL (monocular) */
    float fx, fy, cx, cy, bf, b; /* fx, fy, cx, cy, mbf, mb */
    float min_x, max_x, min_y, max_y; /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    int nlevels;
    const float* scale_factors;  /* mvScaleFactors */
    const float* level_sigma2;   /* mvLevelSigma2 */
    float Tcw[12];               /* mTcw rows 0..2, row-major */
} orbx_frame_view;

/* MapPoint fields, indexed by MapPoint id (the ids stand in for MapPoint*).  Fields a
 * call does not read may be NULL: max/min_distance and normal are read only by the
 * KeyFrame / Sim3 projections (a13, a14).  n < 2^30 for the projection searches (their
 * claims carry a flag in bit 30; larger tables fail with ORBX_ERR_ARG). */
typedef struct {
    int n;
    const float* pos;            /* GetWorldPos(), n x 3 (may be NULL where unused) */
    const uint8_t* desc;         /* GetDescriptor(), n x 32 */
    const int32_t* observations; /* Observations() */
    const uint8_t* bad;          /* isBad() or NULL */
    const float* max_distance;   /* mfMaxDistance (GetMaxDistanceInvariance() = 1.2f * it) */
    const float* min_distance;   /* mfMinDistance (GetMinDistanceInvariance() = 0.8f * it) */
    const float* normal;         /* GetNormal(), n x 3 */
} orbx_mappoints;

/* Frame::IsInFrustum outputs per MapPoint id (Frame.cc:412-477), read by
 * SearchByProjection(Frame&, vector<MapPoint*>, th). */
typedef struct {
    const uint8_t* in_view;      /* mbTrackInView */
    const float* proj_x;         /* mTrackProjX */
    const float* proj_y;         /* mTrackProjY */
    const float* proj_xr;        /* mTrackProjXR */
    const int32_t* scale_level;  /* mnTrackScaleLevel */
    const float* view_cos;       /* mTrackViewCos */
} orbx_track;

typedef struct orbx_matcher orbx_matcher;

/* Failure of the sequential replay (every SearchByProjection form): its fixpoint has an
 * iteration guard that no valid input reaches.  The single-call forms below then return
 * ORBX_ERR_STATE (the MapPoint output is partial); the batched device forms
 * (orbx_match_sequence_device(_ex), orbx_search_local_points_device) write -1 into that
 * frame's nmatches entry, which a caller must treat as a failed frame, never as a count. */

/* ORBmatcher::ORBmatcher(nnratio, checkOri) (ORBmatcher.h:57), bound to HIP device
 * `device` with its own stream and scratch buffers. */
int orbx_matcher_create(int device, float nnratio, int check_ori, orbx_matcher** out);
void orbx_matcher_destroy(orbx_matcher* m);

/* Size limits of the four single-call SearchByProjection forms below.  The frame whose
 * keypoints are searched (f, cur, kf) holds at most 8191 keypoints: the sorted grid encodes
 * a keypoint's position in 13 bits.  n >= 8192 returns ORBX_ERR_UNSUPPORTED, decided before
 * anything is uploaded or launched; the caller's arrays are untouched.  The number of
 * queries (nq, the last frame's or keyframe's keypoints, npoints) is bounded only by
 * memory: queries are not position-encoded, and every nq works with every n <= 8191.
 * The searched frame's nlevels is 1..32 for the first two forms (F, CurrentFrame against
 * LastFrame) and 2..32 for the KeyFrame and Sim3 forms, whose PredictScale needs
 * scale_factors[1]; anything else is ORBX_ERR_ARG, checked on entry before the level tables
 * are read.  Every keypoint octave is below nlevels; the frame's top levels may be empty. */

/* SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, const float th)
 * ORBmatcher.cc:61-173.  frame_mp (F.mvpMapPoints as MapPoint ids, -1 = NULL) is
 * updated in place; queries = vpMapPoints ids in order. */
int orbx_search_by_projection_local(orbx_matcher* m, const orbx_frame_view* f, int32_t* frame_mp,
                                    const int32_t* queries, int nq, const orbx_mappoints* mps,
                                    const orbx_track* trk, float th, int* nmatches);

/* SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
 * ORBmatcher.cc:1620-1789 (TrackWithMotionModel, Tracking.cc:966-994). */
int orbx_search_by_projection_frame(orbx_matcher* m, const orbx_frame_view* cur, int32_t* cur_mp,
                                    const orbx_frame_view* last, const int32_t* last_mp,
                                    const uint8_t* last_outlier, const orbx_mappoints* mps, float th,
                                    int mono, int* nmatches);

/* SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound,
 * th, ORBdist) ORBmatcher.cc:1792-1924 (relocalisation, Tracking.cc:1629-1653).  kf: the
 * KeyFrame's keypoints (angles for the rotation check), kf_mp: GetMapPointMatches() as ids
 * (-1 = NULL), already_found: per MapPoint id (sAlreadyFound) or NULL.  cur_mp
 * (CurrentFrame.mvpMapPoints as ids) is updated in place.  Reads mps pos, desc, bad,
 * max_distance, min_distance. */
int orbx_search_by_projection_keyframe(orbx_matcher* m, const orbx_frame_view* cur, int32_t* cur_mp,
                                       const orbx_frame_view* kf, const int32_t* kf_mp,
                                       const uint8_t* already_found, const orbx_mappoints* mps, float th,
                                       int orb_dist, int* nmatches);

/* SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints,
 * vector<MapPoint*>& vpMatched, int th) ORBmatcher.cc:398-520 (LoopClosing::ComputeSim3,
 * LoopClosing.cc:417).  Scw: 3x4 row-major [sR | st].  points: vpPoints as ids; matched:
 * vpMatched as ids (kf->n entries, -1 = NULL), updated in place.  Reads mps pos, desc,
 * bad, max_distance, min_distance, normal. */
int orbx_search_by_projection_sim3(orbx_matcher* m, const orbx_frame_view* kf, const float* Scw,
                                   const int32_t* points, int npoints, int32_t* matched,
                                   const orbx_mappoints* mps, int th, int* nmatches);

/* Batched TrackWithMotionModel matching (Tracking.cc:966-994) over a device-resident
 * sequence produced by orbx_extract_batch_device: for b >= 1, frame b (CurrentFrame)
 * is matched against frame b-1 (LastFrame) with SearchByProjection(..., th, bMono=1)
 * semantics (ORBmatcher.cc:1620-1789).  Every keypoint i of frame b-1 carries
 * MapPoint id i at depth `depth` on its viewing ray (Observations() > 0).  d_Tcw: B x 12
 * floats (rows 0..2 of each mTcw).  Outputs (device): d_cur_mp [B][cap] (frame 0 stays
 * -1) and d_nmatches [B].  Asynchronous on `stream` (or the matcher's stream). */
int orbx_match_sequence_device(orbx_matcher* m, int batch, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                               const int32_t* d_n, int cap, const float* d_Tcw, float fx, float fy, float cx,
                               float cy, float min_x, float max_x, float min_y, float max_y,
                               const float* scale_factors, int nlevels, float depth, float th,
                               int32_t* d_cur_mp, int32_t* d_nmatches, void* stream);

/* The general form: a sequence of Frames in the orbx_extract_batch_device layout, for
 * b >= 1 frame b (CurrentFrame) matched against frame b-1 (LastFrame) with
 * SearchByProjection(CurrentFrame, LastFrame, th, mono) (ORBmatcher.cc:1620-1789),
 * including the stereo / RGB-D octave ranges for motion along the optical axis
 * (bForward / bBackward, cc:1650-1701) and the mvuRight check (cc:1722-1729).
 * LastFrame keypoint i's MapPoint (id i, Observations() > 0) sits at mp_pos
 * (LastFrame.mvpMapPoints[i]->GetWorldPos()) or, without mp_pos, at `depth` on its
 * viewing ray; has_mp clears keypoints with no MapPoint or flagged mvbOutlier.
 * Both sequence forms: where no LDS layout of the matcher's footprint
 * (orbx_matcher_set_footprint) holds cap keypoints x nlevels octave buckets -- at 8 levels
 * cap >= 6730 in footprints 0, 1, 3, 4; at 32 levels cap >= 2661 in every footprint but 2;
 * cap >= 8192 in footprints 0, 1, 3, 4, 5 -- the call returns ORBX_ERR_UNSUPPORTED before
 * anything is launched, the outputs untouched.  Footprint 2 (the split launches) holds
 * every cap below 8192 at every nlevels. */
typedef struct {
    int batch;                    /* B frames */
    const orbx_keypoint* kps;     /* [B][cap] mvKeysUn (device) */
    const uint8_t* desc;          /* [B][cap][32] mDescriptors */
    const int32_t* n;             /* [B] keypoint counts */
    int cap;
    const float* Tcw;             /* [B][12] mTcw rows 0..2 (device) */
    const float* u_right;         /* [B][cap] mvuRight (device) or NULL */
    const float* mp_pos;          /* [B][cap][3] (device) or NULL */
    const uint8_t* has_mp;        /* [B][cap] (device) or NULL = every keypoint */
    float depth;                  /* MapPoint depth when mp_pos is NULL */
    float fx, fy, cx, cy, bf, b;  /* fx, fy, cx, cy, mbf, mb (mb > 0 unless mono) */
    float min_x, max_x, min_y, max_y;
    int nlevels;
    const float* scale_factors;   /* host: mvScaleFactors (nlevels) */
    float th;
    int mono;                     /* bMono */
    int global_ids;               /* 0: MapPoint id = LastFrame keypoint index i; 1: id = (b-1)*cap + i */
    int32_t* cur_mp;              /* [B][cap] out: CurrentFrame.mvpMapPoints as MapPoint ids, -1 */
    int32_t* nmatches;            /* [B] out (frame 0: 0) */
    const int32_t* mp_obs;        /* [B*cap] Observations() per MapPoint id (device; needs global_ids), or
                                     NULL: every MapPoint has Observations() > 0.  A claim by a MapPoint
                                     with 0 observations (UpdateLastFrame's temporal points) does not
                                     block the keypoint (ORBmatcher.cc:1716-1718) */
    int retry_below;              /* TrackWithMotionModel's retry (Tracking.cc:988-994): a pair with fewer
                                     than retry_below matches is searched again from an empty
                                     mvpMapPoints at 2*th (the reference: 20); 0 = one search */
} orbx_sequence;
int orbx_match_sequence_device_ex(orbx_matcher* m, const orbx_sequence* seq, void* stream);

/* Tracking::SearchLocalPoints (Tracking.cc:1280-1336) for B Frames in HBM -- the
 * per-frame TrackLocalMap search.  For frame b:
 *   1. mvpMapPoints (frame_mp [b][cap], MapPoint ids, -1 = NULL; e.g. the
 *      orbx_match_sequence_device_ex output with global ids): bad MapPoints are set to
 *      NULL, the rest are "seen" and not projected again (Tracking.cc:1286-1299);
 *   2. Frame::IsInFrustum(pMP, viewing_cos_limit) (Frame.cc:412-477) for every entry of
 *      frame b's local map (mvpLocalMapPoints, local_ids[local_off[b] .. local_off[b+1]))
 *      that is neither seen nor bad;
 *   3. SearchByProjection(F, vpLocalMapPoints, th) (ORBmatcher.cc:61-173) with the
 *      matcher's nnratio (Tracking uses ORBmatcher(0.8)) over the points in view, in list
 *      order: frame_mp is updated in place, nmatches [b] receives its count.
 * MapPoints live in a device table indexed by id.  local_off is a host array (B + 1
 * ints: it sizes the launch); every other pointer is a device pointer.  cap must stay
 * below 8192 (keypoints); a local map may hold up to 2^20 MapPoints.  Where no LDS layout
 * of the matcher's footprint holds cap keypoints x the largest local map x nlevels (the
 * limits of orbx_match_sequence_device_ex; a larger local map only moves the query state
 * out of LDS), the call returns ORBX_ERR_UNSUPPORTED before anything is launched, frame_mp
 * and nmatches untouched; footprint 2 holds every valid size.  Asynchronous on `stream` (or
 * the matcher's). */
typedef struct {
    int n;                        /* MapPoints in the table */
    const float* pos;             /* [n][3] GetWorldPos() */
    const uint8_t* desc;          /* [n][32] GetDescriptor() */
    const float* normal;          /* [n][3] GetNormal() */
    const float* max_distance;    /* [n] mfMaxDistance */
    const float* min_distance;    /* [n] mfMinDistance */
    const int32_t* observations;  /* [n] Observations() */
    const uint8_t* bad;           /* [n] isBad() or NULL */
} orbx_mappoints_device;

typedef struct {
    int batch;
    const orbx_keypoint* kps;     /* [B][cap] mvKeysUn */
    const uint8_t* desc;          /* [B][cap][32] mDescriptors */
    const int32_t* n;             /* [B] keypoint counts */
    int cap;
    const float* u_right;         /* [B][cap] mvuRight or NULL */
    const float* Tcw;             /* [B][12] mTcw rows 0..2 */
    float fx, fy, cx, cy, bf;
    float min_x, max_x, min_y, max_y;
    int nlevels;
    const float* scale_factors;   /* host: mvScaleFactors (nlevels) */
    const int32_t* local_off;     /* host: [B + 1] */
    const int32_t* local_ids;     /* device: local map MapPoint ids, frame after frame; ids (here and in
                                     frame_mp) must be < mps->n: an id outside the table is treated as
                                     a NULL entry (never read out of bounds) */
    float th;                     /* 1; 3 for RGB-D; 5 right after a relocalisation (Tracking.cc:1320-1331) */
    float viewing_cos_limit;      /* 0.5 (Tracking.cc:1314) */
    int32_t* frame_mp;            /* [B][cap] in/out */
    int32_t* nmatches;            /* [B] out */
} orbx_local_map_batch;
int orbx_search_local_points_device(orbx_matcher* m, const orbx_mappoints_device* mps,
                                    const orbx_local_map_batch* lm, void* stream);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)
 * (ORBmatcher.cc:228-392; Tracking::TrackReferenceKeyFrame / Relocalization).
 * kf_mp[i]: MapPoint id of KF keypoint i, -1 for NULL or isBad().  FeatureVectors as
 * CSR (nodes ascending, indices ascending within a node).  matches [f->n] out: the KF
 * MapPoint id matched to each frame keypoint, -1 = none.  Uses the matcher's nnratio
 * and checkOri. */
int orbx_search_by_bow_frame(orbx_matcher* m, const orbx_frame_view* kf, const int32_t* kf_mp,
                             const int32_t* kf_fv_node, const int32_t* kf_fv_off, const int32_t* kf_fv_idx,
                             int kf_fv_n, const orbx_frame_view* f, const int32_t* f_fv_node, const int32_t* f_fv_off,
                             const int32_t* f_fv_idx, int f_fv_n, int32_t* matches, int* nmatches);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)
 * (ORBmatcher.cc:696-839; LoopClosing::ComputeSim3).  mp1 / mp2: MapPoint ids, -1 for
 * NULL or isBad().  matches12 [kf1->n] out: KF2's MapPoint id matched to each KF1
 * keypoint, -1 = none. */
int orbx_search_by_bow_keyframes(orbx_matcher* m, const orbx_frame_view* kf1, const int32_t* mp1,
                                 const int32_t* fv1_node, const int32_t* fv1_off, const int32_t* fv1_idx, int fv1_n,
                                 const orbx_frame_view* kf2, const int32_t* mp2, const int32_t* fv2_node,
                                 const int32_t* fv2_off, const int32_t* fv2_idx, int fv2_n, int32_t* matches12,
                                 int* nmatches);

/* ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched,
 * vector<int>& vnMatches12, int windowSize) (ORBmatcher.cc:539-683;
 * Tracking::MonocularInitialization).  prev_matched [f1->n][2] in/out; matches12
 * [f1->n] out (F2 index or -1).  Frames of up to 2^20 keypoints whose working set
 * fits one workgroup's LDS (16 B per keypoint: n1, n2 <= ~8k). */
int orbx_search_for_initialization(orbx_matcher* m, const orbx_frame_view* f1, const orbx_frame_view* f2,
                                   float* prev_matched, int32_t* matches12, int window_size, int* nmatches);

/* ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, float th)
 * (ORBmatcher.cc:1067-1221; LocalMapping::SearchInNeighbors): the search part.  For
 * each points[k] (MapPoint id, -1 = NULL) not flagged in skip[id] (isBad() ||
 * IsInKeyFrame(pKF)), best[k] receives the KF keypoint it fuses with (distance <=
 * TH_LOW, Fuse's chi-square gate on mvuRight) or -1.  No MapPoint's search depends on
 * another's, so all run at once; the caller then runs the reference's Replace /
 * AddObservation loop in order over best[], re-checking isBad() / IsInKeyFrame(). */
int orbx_fuse(orbx_matcher* m, const orbx_frame_view* kf, const int32_t* points, int npoints, const uint8_t* skip,
              const orbx_mappoints* mps, float th, int32_t* best);

/* ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th,
 * vector<MapPoint*>& vpReplacePoint) (ORBmatcher.cc:1226-1352; LoopClosing::SearchAndFuse):
 * the search part; skip[id] = isBad() || pKF->GetMapPoints().count(pMP).  Scw: 3 x 4
 * row-major [sR | st]. */
int orbx_fuse_sim3(orbx_matcher* m, const orbx_frame_view* kf, const float* Scw, const int32_t* points, int npoints,
                   const uint8_t* skip, const orbx_mappoints* mps, float th, int32_t* best);

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
 * (ORBmatcher.cc:1361-1602; LoopClosing::ComputeSim3).  mp1 / mp2: GetMapPointMatches()
 * as ids (-1 = NULL); already1 / already2: vbAlreadyMatched1/2 from the incoming
 * vpMatches12 (may be NULL = none); R12 row-major 3 x 3, t12 3.  matches12 [kf1->n]
 * in/out (KF2 MapPoint ids): mutual matches are written, other entries are left as
 * they are.  *nfound = number written. */
int orbx_search_by_sim3(orbx_matcher* m, const orbx_frame_view* kf1, const int32_t* mp1, const uint8_t* already1,
                        const orbx_frame_view* kf2, const int32_t* mp2, const uint8_t* already2,
                        const orbx_mappoints* mps, float s12, const float* R12, const float* t12, float th,
                        int32_t* matches12, int* nfound);

/* MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:295-360) for nmp MapPoints at once:
 * MapPoint k's descriptors (good observations, observation-map order) are
 * desc[off[k] .. off[k+1]) (32 B each).  best[k] = index within that list of the
 * descriptor with the smallest median distance (-1 when empty); out_desc [nmp][32]
 * (optional) receives it. */
int orbx_compute_distinctive_descriptors(int device, int nmp, const int32_t* off, const uint8_t* desc, int32_t* best,
                                         uint8_t* out_desc);
int orbx_compute_distinctive_descriptors_device(int nmp, const int32_t* d_off, const uint8_t* d_desc, int32_t* d_best,
                                                uint8_t* d_out_desc, void* stream);

/* Footprint of orbx_match_sequence_device's search: 0 (default) = one 1024-thread
 * workgroup per problem with keypoint descriptors and query state in LDS (fastest alone);
 * 1 = 256 threads and global-memory query state; 2 = split into three launches (grid
 * sort per problem, scoring spread over all problems' queries, one wave per problem for
 * the ordered commit); 3 = one wave per problem; 4 = lean: 1024 threads with only the
 * sorted grid and the claims in LDS (descriptors, query state and angles in global
 * memory), the form that leaves the most LDS to extraction running concurrently on
 * another stream; 5 = lean split: mode 4's workgroup sorts and scores, then a one-wave
 * kernel with only the claims in LDS replays.  Same results in every mode. */
int orbx_matcher_set_footprint(orbx_matcher* m, int mode);

/* HIP-event timing of orbx_match_sequence_device and orbx_compute_stereo_matches_batch_device:
 * milliseconds averaged over the (up to 64) most recent calls since
 * orbx_matcher_set_timing(m, 1). */
int orbx_matcher_set_timing(orbx_matcher* m, int enable);
int orbx_matcher_last_ms(orbx_matcher* m, float* ms);
/* Wall time (microseconds) of the newest drop-in host call on m (the SearchByProjection
 * overloads, SearchForTriangulation, SearchByBoW, SearchForInitialization, Fuse,
 * SearchBySim3, ComputeStereoMatches): entry to return, i.e. what a C++ caller such as
 * Tracking pays per call, without any binding overhead.  -1 for a null matcher. */
double orbx_matcher_last_call_us(const orbx_matcher* m);

/* SearchForTriangulation(KF1, KF2, F12, vMatchedPairs, bOnlyStereo)
 * ORBmatcher.cc:850-1056 (LocalMapping::CreateNewMapPoints, LocalMapping.cc:305).
 * DBoW2 FeatureVectors as CSR: node ids ascending (fv_node[k]), keypoints of node k
 * at fv_idx[fv_off[k] .. fv_off[k+1]).  pairs receives (idx1, idx2) in idx1 order
 * (capacity 2*kf1->n ints); *npairs the count. */
int orbx_search_for_triangulation(orbx_matcher* m, const orbx_frame_view* kf1, const uint8_t* kf1_has_mp,
                                  const int32_t* fv1_node, const int32_t* fv1_off, const int32_t* fv1_idx,
                                  int fv1_n, const orbx_frame_view* kf2, const uint8_t* kf2_has_mp,
                                  const int32_t* fv2_node, const int32_t* fv2_off, const int32_t* fv2_idx,
                                  int fv2_n, const float* F12, int only_stereo, int32_t* pairs, int* npairs);

/* One KeyFrame as SearchForTriangulation reads it, left in HBM by the batched device
 * calls (frame b of their [B][cap] layouts): orbx_extract_batch_device (keys, desc, n),
 * orbx_compute_stereo_matches_batch_device (u_right), orbx_vocabulary_transform_batch_device
 * (the FeatureVector CSR fv_node / fv_off / fv_idx / nfv).  Device pointers, except Tcw:
 * the pose stays a host value as in the reference (KeyFrame::GetPose). */
typedef struct {
    const orbx_keypoint* keys;   /* mvKeysUn (cap slots) */
    const uint8_t* desc;         /* mDescriptors (cap x 32) */
    const int32_t* n;            /* N (one device int; min(*n, cap) keypoints are read) */
    const float* u_right;        /* mvuRight (cap) or NULL (monocular) */
    const uint8_t* has_mp;       /* GetMapPoint(i) != NULL (cap) */
    const int32_t* fv_node;      /* mFeatVec node ids, ascending (cap) */
    const int32_t* fv_off;       /* node k's keypoints: fv_idx[fv_off[k] .. fv_off[k+1]) (cap + 1) */
    const int32_t* fv_idx;       /* (cap) */
    const int32_t* nfv;          /* node count (one device int) */
    float Tcw[12];               /* host: mTcw rows 0..2 */
} orbx_keyframe_device;

/* LocalMapping::CreateNewMapPoints' matching loop (LocalMapping.cc:235-305) over many
 * keyframe pairs at once: for p < npairs, SearchForTriangulation(KF1 = kfs[pairs[2p]],
 * KF2 = kfs[pairs[2p+1]], F12 + 9p, vMatchedPairs, only_stereo) (ORBmatcher.cc:850-1056),
 * with the matcher's checkOri (LocalMapping uses ORBmatcher(0.6, false)).  `cam` gives
 * the shared intrinsics fx, fy, cx, cy and the level tables (nlevels, scale_factors,
 * level_sigma2); its keys / desc / u_right / Tcw are not read.  pairs and F12 (row-major
 * 3x3, LocalMapping::ComputeF12) are host arrays; the epipole comes from the host poses.
 * Outputs (device): d_matches12 [P][cap] (vMatches12: KF2 index or -1), d_pairs
 * [P][cap][2] (vMatchedPairs, idx1 order) and d_npairs [P].  Enqueued on `stream` (or the
 * matcher's) without synchronising; the host tables are staged through pinned memory, so
 * they may be reused on return.  Successive calls on one matcher must use one stream
 * (they share its device work area).  cap <= 8192. */
int orbx_search_for_triangulation_batch_device(orbx_matcher* m, int nkf, const orbx_keyframe_device* kfs,
                                               const orbx_frame_view* cam, int npairs, const int32_t* pairs,
                                               const float* F12, int only_stereo, int cap, int32_t* d_matches12,
                                               int32_t* d_pairs, int32_t* d_npairs, void* stream);

/* Frame::ComputeStereoMatches (Frame.cc:673-885) of one stereo Frame, as the stereo Frame
 * constructor runs it (Frame.cc:99-178): the left image was extracted by `ex_left` (frame
 * `left_frame` of its last extraction, mpORBextractorLeft) and the right image by
 * `ex_right` (frame `right_frame`, mpORBextractorRight); the two may be one extractor
 * holding both images.  The SAD refinement reads both extractors' mvImagePyramid
 * (Frame.cc:782-818).  left: mvKeys / mDescriptors / mbf; keys_r / desc_r: mvKeysRight /
 * mDescriptorsRight.  maxD = mbf / minZ (this fork reads mb before it is set,
 * Frame.cc:711-713; upstream's value is fx).  Writes mvuRight and mvDepth (n_left floats
 * each, -1 = no match), including this fork's in-loop outlier pass (Frame.cc:868-884).
 * Host buffers; synchronous.  At most 8192 keypoints per image, and the row index of a
 * pair must fit 150 KB of LDS: ((nlevels + 1) * rows + 2) * 4 <= 153600 bytes (8 levels:
 * 4266 rows; 12 levels: 2953 rows).  Beyond either limit both forms return
 * ORBX_ERR_UNSUPPORTED before any upload or launch (this form's outputs are all -1). */
int orbx_compute_stereo_matches(orbx_matcher* m, orbx_extractor* ex_left, int left_frame, orbx_extractor* ex_right,
                                int right_frame, const orbx_frame_view* left, const orbx_keypoint* keys_r,
                                const uint8_t* desc_r, int n_right, float max_disparity, float* u_right,
                                float* depth);

/* The same for B stereo Frames in HBM (configs[2]): pair b's left image is frame
 * left_frame0 + b of ex_left's last extraction with keypoints d_kps_l + b*cap
 * (min(d_n_l[b], cap) of them, the orbx_extract_batch_device layout), its right image
 * frame right_frame0 + b of ex_right's.  Scale factors come from the extractors.
 * Outputs d_u_right / d_depth [B][cap] (slots past a pair's count are -1).  Enqueued on
 * `stream` (or the matcher's) without synchronising: the caller orders it after both
 * extractions (and before either extractor's next extraction, which overwrites the
 * pyramids).  cap <= 8192. */
int orbx_compute_stereo_matches_batch_device(orbx_matcher* m, orbx_extractor* ex_left, int left_frame0,
                                             orbx_extractor* ex_right, int right_frame0, int batch,
                                             const orbx_keypoint* d_kps_l, const uint8_t* d_desc_l,
                                             const int32_t* d_n_l, const orbx_keypoint* d_kps_r,
                                             const uint8_t* d_desc_r, const int32_t* d_n_r, int cap, float bf,
                                             float max_disparity, float* d_u_right, float* d_depth, void* stream);

/* ---- Frame: undistortion and grid (§8(f) rank 3) ----
 * Camera intrinsics and distortion: Frame::mK and Frame::mDistCoef [k1 k2 p1 p2 (k3)]
 * (Tracking.cc:60-92; k3 = 0 when the settings have four coefficients). */
typedef struct {
    float fx, fy, cx, cy;
    float k1, k2, p1, p2, k3;
} orbx_camera;

/* Frame::UndistortKeyPoints (Frame.cc:586-628): cv::undistortPoints(mvKeys, K, D,
 * noArray(), K) on every keypoint; mvKeysUn = mvKeys when k1 == 0.  Host buffers of n
 * keypoints (keys_un may equal keys). */
int orbx_undistort_keypoints(int device, const orbx_camera* cam, const orbx_keypoint* keys, int n,
                             orbx_keypoint* keys_un);
/* Same over the orbx_extract_batch_device layout (frame b at d_keys + b*cap, min(d_n[b], cap)
 * keypoints) into d_keys_un [B][cap].  Asynchronous on `stream`. */
int orbx_undistort_keypoints_device(const orbx_camera* cam, int batch, const orbx_keypoint* d_keys,
                                    const int32_t* d_n, int cap, orbx_keypoint* d_keys_un, void* stream);
/* Frame::ComputeImageBounds (Frame.cc:636-665): bounds = {mnMinX, mnMaxX, mnMinY, mnMaxY}. */
int orbx_compute_image_bounds(int device, const orbx_camera* cam, int cols, int rows, float* bounds);
/* Frame::AssignFeaturesToGrid (Frame.cc:351-370, PosInGrid 558-567) as CSR: cell
 * c = ix * FRAME_GRID_ROWS + iy (64 x 48) holds cell_idx[cell_start[c] .. cell_start[c+1]),
 * ascending; keypoints outside the grid are left out.  n <= 8192. */
int orbx_assign_features_to_grid(int device, const orbx_keypoint* keys_un, int n, const float* bounds,
                                 int32_t* cell_start, int32_t* cell_idx);
/* Batched: d_cell_start [B][3073], d_cell_idx [B][cap], cap <= 8192.  Asynchronous. */
int orbx_assign_features_to_grid_device(int batch, const orbx_keypoint* d_keys_un, const int32_t* d_n, int cap,
                                        const float* bounds, int32_t* d_cell_start, int32_t* d_cell_idx,
                                        void* stream);

/* The MapPoints a stereo / RGB-D keyframe is born with (Tracking::CreateNewKeyFrame,
 * Tracking.cc:1069-1121) for B frames in HBM, as an orbx_mappoints_device table with id
 * b*cap + i: for every keypoint i < n[b] with depth z > 0 (d_depth [B][cap] = mvDepth, the
 * caller's selection of close points; or `const_depth` for every keypoint when d_depth is
 * NULL), pos = Frame::UnprojectStereo(i) (Frame.cc:912-927) and normal / mfMaxDistance /
 * mfMinDistance from MapPoint::UpdateNormalAndDepth with the frame as the only observation
 * (MapPoint.cc:386-439); observations 1, bad 0.  Other slots: bad 1, observations 0.
 * Outputs [B*cap] (pos, normal: x3).  scale_factors is a host array.  Asynchronous. */
int orbx_create_mappoints_device(int batch, const orbx_keypoint* d_kps, const int32_t* d_n, int cap,
                                 const float* d_depth, float const_depth, const float* d_Tcw, float fx, float fy,
                                 float cx, float cy, const float* scale_factors, int nlevels, float* d_pos,
                                 float* d_normal, float* d_max_distance, float* d_min_distance,
                                 int32_t* d_observations, uint8_t* d_bad, void* stream);

/* Tracking::UpdateLastFrame (Tracking.cc:893-954) for B stereo / RGB-D LastFrames in HBM
 * (none of them the last keyframe): the keypoints with mvDepth > 0 are visited nearest
 * first (pairs (depth, index) ascending); one without a MapPoint, or whose MapPoint has
 * Observations() < 1, gets a temporal MapPoint at Frame::UnprojectStereo(i) (Frame.cc:
 * 912-927) with Observations() 0; the walk ends after the first point beyond th_depth
 * (mThDepth = mbf * ThDepth / fx) once more than 100 points were visited.  In: d_obs_in
 * [B][cap] Observations() of LastFrame.mvpMapPoints (-1 = NULL) and d_pos_in [B][cap][3]
 * their world positions, or both NULL (no MapPoints).  Out: d_mp_obs [B][cap] (-1 = none),
 * d_mp_pos [B][cap][3], d_has_mp [B][cap] -- the orbx_sequence mp_obs / mp_pos / has_mp
 * inputs of the following TrackWithMotionModel search (global ids b*cap + i).  The outputs
 * may alias the inputs.  Asynchronous. */
int orbx_update_last_frame_device(int batch, const orbx_keypoint* d_kps, const int32_t* d_n, int cap,
                                  const float* d_depth, const float* d_Tcw, float fx, float fy, float cx, float cy,
                                  float th_depth, const int32_t* d_obs_in, const float* d_pos_in, int32_t* d_mp_obs,
                                  float* d_mp_pos, uint8_t* d_has_mp, void* stream);

/* ---- RGB-D Frame (configs[4]) ----
 * Frame::Frame(imGray, imDepth, ...) for RGB-D (Frame.cc:192-264) after ExtractORB:
 * UndistortKeyPoints (Frame.cc:586-628) and ComputeStereoFromRGBD (Frame.cc:888-909), with
 * Tracking::GrabImageRGBD's depth conversion (Tracking.cc:265-271) applied to the pixels the
 * lookup reads.  For keypoint i (mvKeys[i] = kps, mvKeysUn[i] = kps_un):
 *   d = imDepth.at<float>((int)kp.y, (int)kp.x), imDepth = the depth image converted to
 *       CV_32F with scale mDepthMapFactor (= 1 / DepthMapFactor, Tracking.cc:166-170):
 *       a u16 image always (d = (float)raw * factor), an f32 image only when
 *       |factor - 1| > 1e-5 (d = raw * factor), else as is;
 *   d > 0: mvDepth[i] = d, mvuRight[i] = kpU.x - mbf / d; otherwise both -1.
 * A keypoint outside the depth image (never one the extractor produced) gets -1 (the
 * reference's Mat::at would read out of bounds). */
#define ORBX_DEPTH_U16 0
#define ORBX_DEPTH_F32 1
typedef struct {
    int batch;                   /* B frames in the orbx_extract_batch_device layout */
    const orbx_keypoint* kps;    /* [B][cap] mvKeys (device): the depth lookup positions */
    orbx_keypoint* kps_un;       /* [B][cap] mvKeysUn (device): written when a camera is given,
                                    read otherwise */
    const int32_t* n;            /* [B] keypoint counts */
    int cap;
    const void* depth;           /* frame b's depth image at depth + b*frame_bytes, rows
                                    row_bytes apart (device) */
    int depth_type;              /* ORBX_DEPTH_U16 (TUM's 16-bit PNG) or ORBX_DEPTH_F32 */
    int width, height;           /* depth image size (the gray image's) */
    long long row_bytes, frame_bytes;
    float depth_map_factor;      /* Tracking's mDepthMapFactor (1 / DepthMapFactor) */
    float bf;                    /* mbf */
    float* u_right;              /* [B][cap] out: mvuRight (slots >= n[b]: -1) */
    float* depth_out;            /* [B][cap] out: mvDepth (slots >= n[b]: -1) */
} orbx_rgbd_batch;
/* cam non-NULL: UndistortKeyPoints into kps_un and the depth lookup in one pass; NULL:
 * kps_un holds mvKeysUn already.  Asynchronous on `stream`. */
int orbx_compute_stereo_from_rgbd_device(const orbx_camera* cam, const orbx_rgbd_batch* rb, void* stream);
/* One RGB-D Frame from host buffers (the drop-in Frame constructor): n keypoints, a
 * width x height depth image with rows row_bytes apart.  keys_un: out when cam is
 * non-NULL, else in.  u_right / depth_out: n floats. */
int orbx_compute_stereo_from_rgbd(int device, const orbx_camera* cam, const orbx_keypoint* keys, int n,
                                  const void* depth, int depth_type, int width, int height, size_t row_bytes,
                                  float depth_map_factor, float bf, orbx_keypoint* keys_un, float* u_right,
                                  float* depth_out);

/* ---- DBoW2 vocabulary (TemplatedVocabulary<FORB::TDescriptor, FORB>, §8(f) rank 1) ----
 * The tree lives in HBM as its CSR edge list.  Scoring / weighting
 * codes are DBoW2's enums (BowVector.h:29-56): scoring L1_NORM 0, L2_NORM 1,
 * CHI_SQUARE 2, KL 3, BHATTACHARYYA 4, DOT_PRODUCT 5; weighting TF_IDF 0, TF 1, IDF 2,
 * BINARY 3. */
typedef struct orbx_vocabulary orbx_vocabulary;

/* TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1338-1424; called by
 * System.cc:67): header "k L scoring weighting", then one node per line "parent
 * isLeaf d0..d31 weight".  Same header range checks; empty lines are skipped (the
 * reference turns a trailing one into a root child with an uninitialised descriptor);
 * a malformed node line or a parent id that does not precede the node is ORBX_ERR_ARG. */
int orbx_vocabulary_load_text_file(const char* path, int device, orbx_vocabulary** out);
/* Same from an in-memory text of `len` bytes. */
int orbx_vocabulary_load_text(const char* text, size_t len, int device, orbx_vocabulary** out);
void orbx_vocabulary_destroy(orbx_vocabulary* voc);
/* m_k, m_L, m_scoring, m_weighting, node count (incl. root), size() (words). */
int orbx_vocabulary_info(const orbx_vocabulary* voc, int* k, int* L, int* scoring, int* weighting, int* nnodes,
                         int* nwords);
/* The vocabulary's hipStream_t (as void*). */
void* orbx_vocabulary_stream(orbx_vocabulary* voc);

/* TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup)
 * (TemplatedVocabulary.h:1220-1259) for n descriptors (host buffers, n x 32 B).
 * node may be NULL.  A leaf reached above level L - levelsup reports the deepest
 * node (the reference leaves nid unset there). */
int orbx_vocabulary_transform_features(orbx_vocabulary* voc, const uint8_t* desc, int n, int levelsup,
                                       int32_t* word, double* weight, int32_t* node);

/* TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup)
 * (TemplatedVocabulary.h:1127-1186) for one frame of n <= 8192 descriptors (host
 * buffers), as called by Frame::ComputeBoW / KeyFrame::ComputeBoW with levelsup 4
 * (Frame.cc:573-583, KeyFrame.cc:66-74).  BowVector: (bow_word[j], bow_value[j]),
 * j < *nbow, ascending words.  FeatureVector: node fv_node[j] (ascending) holds the
 * features fv_idx[fv_off[j] .. fv_off[j+1]) (ascending), j < *nfv.  Capacities: n
 * entries, fv_off n + 1. */
int orbx_vocabulary_transform(orbx_vocabulary* voc, const uint8_t* desc, int n, int levelsup, int32_t* bow_word,
                              double* bow_value, int* nbow, int32_t* fv_node, int32_t* fv_off, int32_t* fv_idx,
                              int* nfv);

/* Batched device path over the orbx_extract_batch_device layout: frame b's
 * descriptors at d_desc + b*cap*32, min(d_n[b], cap) of them, cap <= 8192.  Outputs
 * (device) per frame: d_bow_word / d_bow_value / d_fv_node / d_fv_idx [B][cap],
 * d_fv_off [B][cap+1], d_nbow / d_nfv [B]; optional d_feat_word / d_feat_node [B][cap]
 * (the word and level-(L - levelsup) node of every feature; NULL = not wanted).
 * Asynchronous on `stream` (or the vocabulary's stream). */
int orbx_vocabulary_transform_batch_device(orbx_vocabulary* voc, int batch, const uint8_t* d_desc,
                                           const int32_t* d_n, int cap, int levelsup, int32_t* d_feat_word,
                                           int32_t* d_feat_node, int32_t* d_bow_word, double* d_bow_value,
                                           int32_t* d_nbow, int32_t* d_fv_node, int32_t* d_fv_off,
                                           int32_t* d_fv_idx, int32_t* d_nfv, void* stream);

/* HIP-event timing of transform calls (events on the launch stream), averaged over
 * the (up to 64) most recent calls: the tree walk and the per-frame vector build. */
int orbx_vocabulary_set_timing(orbx_vocabulary* voc, int enable);
int orbx_vocabulary_stage_times(orbx_vocabulary* voc, float* walk_ms, float* frame_ms);

/* ---- KeyFrameDatabase: L1 BoW score and candidate detection (since orbx 0.2) ----
 * KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:31-307) with the
 * stored keyframes' BowVectors in HBM, and the score both detections use: L1Scoring::score
 * (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).  Same candidates, in the same order,
 * with the same float scores as the reference.  Only L1_NORM is built (ORB-SLAM2's
 * vocabulary is TF_IDF / L1_NORM).  A BowVector is a pair of arrays (words ascending,
 * values), the orbx_vocabulary_transform(_batch_device) layout.  DESIGN.md §4.14. */
typedef struct orbx_kfdb orbx_kfdb;
#define ORBX_KFDB_MAX_KEYFRAMES 8192 /* ceiling of max_keyframes */
#define ORBX_KFDB_COVIS 10           /* GetBestCovisibilityKeyFrames(10) */

/* L1Scoring::score(v1, v2) (ScoringObject.cpp:23-68) on two host BowVectors: the shared
 * words in ascending order, score += fabs(vi - wi) - fabs(vi) - fabs(wi) from 0.0, then
 * -score / 2.0 -- so two vectors without a shared word give -0.0.  Host only; needs no GPU. */
int orbx_bow_score(const int32_t* w1, const double* v1, int n1, const int32_t* w2, const double* v2, int n2,
                   double* score);

/* KeyFrameDatabase::KeyFrameDatabase(voc) (cc:31-34) on the vocabulary's device: room for
 * keyframe ids 0 .. max_keyframes - 1 (at most ORBX_KFDB_MAX_KEYFRAMES = 8192: one workgroup
 * orders a query's candidates) of up to `cap` <= 8192 words each; HBM: 12 bytes x
 * max_keyframes x cap.  A vocabulary whose scoring is not L1_NORM: ORBX_ERR_UNSUPPORTED.
 * One database owns one stream and is not re-entrant; a call that names another stream
 * first waits for the database's previous work. */
int orbx_kfdb_create(const orbx_vocabulary* voc, int max_keyframes, int cap, orbx_kfdb** out);
void orbx_kfdb_destroy(orbx_kfdb* db);
/* max_keyframes, cap, number of stored keyframes (each nullable). */
int orbx_kfdb_info(const orbx_kfdb* db, int* max_keyframes, int* cap, int* size);
/* The database's hipStream_t (as void*). */
void* orbx_kfdb_stream(orbx_kfdb* db);

/* KeyFrameDatabase::add (cc:37-43) for n keyframes: keyframe ids[i] (host array; caller-chosen,
 * in [0, max_keyframes)) stores BowVector i of d_bow_word / d_bow_value [n][src_cap], d_nbow [n]
 * (device; the orbx_vocabulary_transform_batch_device outputs).  A database that cannot hold
 * n more keyframes: ORBX_ERR_CAPACITY; an id that is stored already (or twice in ids):
 * ORBX_ERR_STATE; a BowVector longer than the database's cap: ORBX_ERR_CAPACITY; nothing is
 * stored then.  The new keyframe has an empty covisibility list and reloc_score 0.0f: the
 * reference's mRelocScore is never initialised (KeyFrame.cc:32-64), and this is the value
 * pinned for it.  Reads d_nbow back (synchronises the stream); the copy itself is enqueued. */
int orbx_kfdb_add_batch_device(orbx_kfdb* db, int n, const int32_t* ids, const int32_t* d_bow_word,
                               const double* d_bow_value, const int32_t* d_nbow, int src_cap, void* stream);
/* The same for one keyframe from a host BowVector of n words (the drop-in add(pKF)). */
int orbx_kfdb_add(orbx_kfdb* db, int id, const int32_t* word, const double* value, int n);
/* KeyFrameDatabase::erase (cc:46-60): the other keyframes keep their relative order; the id
 * may be added again and is then the newest.  An id that is not stored: ORBX_ERR_STATE. */
int orbx_kfdb_erase(orbx_kfdb* db, int id);
/* KeyFrameDatabase::clear (cc:63-66). */
int orbx_kfdb_clear(orbx_kfdb* db);
/* KeyFrame::GetBestCovisibilityKeyFrames(10) of a stored keyframe as the detections read it
 * (cc:153, 268): n <= 10 keyframe ids (host), in the list's order.  Ids that are not stored
 * (erased, or outside the database) never count. */
int orbx_kfdb_set_covisibility(orbx_kfdb* db, int id, const int32_t* best, int n);
/* mRelocScore of every id (max_keyframes floats, host; 0 for ids that are not stored):
 * the score a relocalisation query last gave the keyframe.  Synchronous. */
int orbx_kfdb_reloc_scores(orbx_kfdb* db, float* scores);

/* float si = mpVoc->score(query, KF) (cc:133, 251) of one query BowVector (device: qcap slots,
 * *d_qn of them used) against the stored keyframes d_ids [nids] (device) -- the minScore loop
 * of LoopClosing.cc:119-132 in one launch.  d_score [nids] (device); NaN for an id that is
 * not stored.  Asynchronous on `stream` (or the database's). */
int orbx_kfdb_score_device(orbx_kfdb* db, const int32_t* d_qword, const double* d_qvalue, const int32_t* d_qn,
                           int qcap, const int32_t* d_ids, int nids, float* d_score, void* stream);

/* KeyFrameDatabase::DetectRelocalizationCandidates(F) (cc:206-307) for B query BowVectors in
 * HBM (d_qword / d_qvalue [B][qcap], d_qn [B]; qcap <= 8192): exactly what B single calls in
 * the order b = 0 .. B-1 give, the keyframes' persistent reloc_score included (a group sums
 * the mRelocScore of every covisible candidate, scored by this query or left by an earlier
 * one, cc:275-281).  Outputs (device): d_cand [B][max_cand] keyframe ids in the reference's
 * order, d_ncand [B] the full count (only max_cand ids are written); optional diagnostics
 * d_words [B][max_keyframes] (shared words, 0 = no candidate) and d_score [B][max_keyframes]
 * (si, -1 = not scored), NULL = not wanted.  Asynchronous on `stream` (or the database's);
 * after add / erase / clear / set_covisibility the first call uploads the membership and
 * waits for that copy. */
int orbx_kfdb_detect_relocalization_candidates_device(orbx_kfdb* db, int batch, const int32_t* d_qword,
                                                      const double* d_qvalue, const int32_t* d_qn, int qcap,
                                                      int32_t* d_cand, int max_cand, int32_t* d_ncand,
                                                      int32_t* d_words, float* d_score, void* stream);
/* KeyFrameDatabase::DetectLoopCandidates(pKF, minScore) (cc:79-195) for B independent
 * queries: query b's GetConnectedKeyFrames() are the ids d_conn_ids[d_conn_off[b] ..
 * d_conn_off[b+1]) (device CSR, B + 1 offsets; d_conn_ids may be NULL when every set is
 * empty) and d_min_score [b] its minScore (device).  Outputs as above; connected keyframes
 * report 0 words. */
int orbx_kfdb_detect_loop_candidates_device(orbx_kfdb* db, int batch, const int32_t* d_qword, const double* d_qvalue,
                                            const int32_t* d_qn, int qcap, const int32_t* d_conn_off,
                                            const int32_t* d_conn_ids, const float* d_min_score, int32_t* d_cand,
                                            int max_cand, int32_t* d_ncand, int32_t* d_words, float* d_score,
                                            void* stream);
/* The single-query host forms (the drop-in calls of Tracking::Relocalization, Tracking.cc:1524,
 * and LoopClosing::DetectLoop, LoopClosing.cc:136): host BowVector of n words in, cand
 * [max_cand] and *ncand out.  More than max_cand candidates: ORBX_ERR_CAPACITY with *ncand
 * the count.  Synchronous. */
int orbx_kfdb_detect_relocalization_candidates(orbx_kfdb* db, const int32_t* word, const double* value, int n,
                                               int32_t* cand, int max_cand, int* ncand);
int orbx_kfdb_detect_loop_candidates(orbx_kfdb* db, const int32_t* word, const double* value, int n,
                                     const int32_t* connected, int nconnected, float min_score, int32_t* cand,
                                     int max_cand, int* ncand);

/* ---- Optimizer::PoseOptimization: motion-only bundle adjustment after the searches ----
 * Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:299-502) with the parts of g2o it
 * runs (OptimizationAlgorithmLevenberg, the dense 6x6 LDLT, EdgeSE3ProjectXYZOnlyPose /
 * EdgeStereoSE3ProjectXYZOnlyPose, RobustKernelHuber, SE3Quat), for B Frames in HBM in one
 * launch: one persistent workgroup per frame runs the four rounds of up to ten
 * Levenberg-Marquardt iterations.  Float inputs are widened to double, everything after
 * is double.  Sums over edges have a fixed shape (no floating-point atomics): a frame's
 * results are the same bytes whatever the batch around it.  DESIGN.md §4.15.
 *   Edges, in keypoint order: keypoint i with a MapPoint (frame_mp[i] in [0, n_mp); -1 or
 *   an id outside the table is NULL) is monocular if u_right is NULL or u_right[i] < 0
 *   (cc:346), stereo otherwise; information = I * inv_level_sigma2[octave] (an octave
 *   outside [0, nlevels) is clamped into it).
 *   Outputs: Tcw_opt (Converter::toCvMat of the recovered SE3Quat); outlier = mvbOutlier
 *   (in/out: entries of keypoints without a MapPoint are left as they are); ninliers = the
 *   return value nInitialCorrespondences - nBad; ninit = nInitialCorrespondences; trace
 *   (nullable) per round {LM iterations run, linear solves tried}, 0 for rounds not run.
 *   Fewer than 3 edges (cc:428): ninliers 0, Tcw_opt = Tcw, the flags of the keypoints
 *   with MapPoints cleared.
 *   Epilogue (Tracking.cc:1004-1017), optional: discard_outliers sets the outliers'
 *   frame_mp entries to -1 and clears their flags; nmatches_map (nullable) counts the
 *   inliers whose MapPoint has Observations() > 0 (mp_obs [n_mp], NULL: every one has).
 * inv_level_sigma2 is a host array; every other pointer is a device pointer.  Asynchronous
 * on `stream` (or the matcher's). */
#define ORBX_POSE_OPT_LDS_EDGES 1984 /* frames of up to this many edges keep them in LDS */
typedef struct {
    int batch;
    const orbx_keypoint* kps;       /* [B][cap] mvKeysUn */
    const int32_t* n;               /* [B] keypoint counts */
    int cap;
    const float* u_right;           /* [B][cap] mvuRight or NULL (every edge monocular) */
    int32_t* frame_mp;              /* [B][cap] mvpMapPoints as MapPoint ids; written only with discard_outliers */
    int n_mp;                       /* MapPoints in the table */
    const float* mp_pos;            /* [n_mp][3] GetWorldPos() */
    const float* inv_level_sigma2;  /* host: mvInvLevelSigma2 (nlevels) */
    int nlevels;
    float fx, fy, cx, cy, bf;
    const float* Tcw;               /* [B][12] mTcw rows 0..2 */
    float* Tcw_opt;                 /* [B][12] out */
    uint8_t* outlier;               /* [B][cap] in/out */
    int32_t* ninliers;              /* [B] out */
    int32_t* ninit;                 /* [B] out */
    int32_t* trace;                 /* [B][4][2] out or NULL */
    int discard_outliers;
    const int32_t* mp_obs;          /* [n_mp] Observations() or NULL */
    int32_t* nmatches_map;          /* [B] out or NULL */
} orbx_pose_optimization_batch;
int orbx_pose_optimization_batch_device(orbx_matcher* m, const orbx_pose_optimization_batch* po, void* stream);

/* The drop-in single-frame call on host arrays (keys [n], u_right [n] or NULL, frame_mp
 * [n], mp_pos [n_mp][3], Tcw [12] in; Tcw_opt [12], outlier [n] (in/out), *ninit, trace
 * [4][2] (nullable), *ninliers out): one upload, the batch kernel with B = 1, one
 * synchronisation.  The same bytes as the batch form gives for that frame. */
int orbx_pose_optimization(orbx_matcher* m, const orbx_keypoint* keys, int n, const float* u_right,
                           const int32_t* frame_mp, const float* mp_pos, int n_mp, const float* inv_level_sigma2,
                           int nlevels, float fx, float fy, float cx, float cy, float bf, const float* Tcw,
                           float* Tcw_opt, uint8_t* outlier, int* ninit, int32_t* trace, int* ninliers);

/* ---- Sim3Solver: Horn's closed form under RANSAC for a batch of loop candidates ----
 * Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc:37-534) as LoopClosing::ComputeSim3
 * drives it (LoopClosing.cc:243-377: one solver per candidate, iterate(5) round-robin), for B
 * candidates in HBM: the link between orbx_search_by_bow_keyframes and orbx_search_by_sim3.
 * Float inputs are widened to double, everything after is double, outputs are rounded to
 * float once.  No sum crosses lanes in floating point: a candidate's results are the same
 * bytes whatever the batch around it and however its iterations are cut into calls.  The
 * host reads nothing back between a set and the end of an iterate.  DESIGN.md §4.16.
 *
 * The library owns no random generator: the caller supplies the three draws of every
 * iteration (orbx_sim3_draws gives the reference's).
 *
 * orbx_sim3_create (the workspace and per-candidate state for up to max_batch candidates of
 * up to cap slots and max_iterations <= ORBX_SIM3_MAX_ITERATIONS iterations) borrows the
 * matcher's device and stream; the matcher must outlive it.  orbx_sim3_destroy waits for that
 * stream; after the library's unload destructor it releases nothing. */
#define ORBX_SIM3_MAX_ITERATIONS 4096
#define ORBX_SIM3_STATUS_BAD_DRAW 1 /* status bit 0: a walked iteration had a draw outside [0, N - j) */
typedef struct orbx_sim3 orbx_sim3;
int orbx_sim3_create(orbx_matcher* m, int max_batch, int cap, int max_iterations, orbx_sim3** out);
void orbx_sim3_destroy(orbx_sim3* s);

/* The constructor (cc:37-129) and SetRansacParameters(probability, min_inliers,
 * max_iterations) (cc:132-185) for `batch` candidates of one camera pair.
 *   Slot i < n1 (mN1) of a candidate is kept iff mp1[i] (vpKeyFrameMP1) and mp2[i]
 *   (vpMatched12) both lie in [0, n_mp): -1, any negative id or one outside the table skips
 *   the slot (the caller maps NULL, isBad() and GetIndexInKeyFrame() < 0 to -1; cc:70-87).
 *   Kept slots in slot order are the N correspondences (mvnIndices1).  mvX3Dc = Rcw Xw + tcw
 *   per keyframe, mvP1im1 / mvP2im2 by FromCameraToImage without a depth check (cc:527),
 *   mvnMaxError = 9.210 * level_sigma2[octave] truncated to an integer as the reference's
 *   vector<size_t> does (Sim3Solver.h:143-144): 9, 13, 19, ... at scale 1.2; octaves are
 *   clamped into [0, nlevels).  The iteration cap is cc:145-181 at N, evaluated by the host's
 *   libm for every n in 0..cap and looked up on the device.  mnIterations and mnBestInliers
 *   are reset to 0.
 *   draws [batch][max_iterations][3] is read by the later iterate calls, indexed by the
 *   absolute iteration, and must stay valid until the next set: draw j of an iteration is
 *   RandomInt(0, N - 1 - j) (cc:224) and must lie in [0, N - j); otherwise that iteration has
 *   a NaN hypothesis and 0 inliers, and ORBX_SIM3_STATUS_BAD_DRAW is set once it is walked.
 * level_sigma2, K1 and K2 are host arrays, every other pointer is a device pointer (all are
 * host pointers, and batch is 1, for orbx_sim3_set).  Asynchronous on `stream` (or the
 * matcher's); the calls on one solver share its workspace, so the caller keeps them in
 * order: one stream for a set and its iterates, or events between streams. */
typedef struct {
    int batch;
    int cap;                    /* slots per candidate row, <= the solver's cap */
    const int32_t* n1;          /* [B] mN1 = vpMatched12.size(), clamped into [0, cap] */
    const int32_t* mp1;         /* [B][cap] vpKeyFrameMP1 as MapPoint ids */
    const int32_t* mp2;         /* [B][cap] vpMatched12 as MapPoint ids */
    const int32_t* oct1;        /* [B][cap] kp1.octave */
    const int32_t* oct2;        /* [B][cap] kp2.octave */
    int n_mp;                   /* MapPoints in the table */
    const float* mp_pos;        /* [n_mp][3] GetWorldPos() */
    const float* Tcw1;          /* [B][12] pKF1's pose, rows 0..2 */
    const float* Tcw2;          /* [B][12] pKF2's pose */
    const float* level_sigma2;  /* host: mvLevelSigma2 (nlevels), each in [0, 2^24 / 9.21) */
    int nlevels;
    const float* K1;            /* host: fx fy cx cy of pKF1 */
    const float* K2;            /* host: ... of pKF2 */
    int fix_scale;              /* mbFixScale: the scale is exactly 1 */
    double probability;         /* in (0, 1) */
    int min_inliers;
    int max_iterations;         /* <= the solver's */
    const int32_t* draws;       /* [B][max_iterations][3] */
} orbx_sim3_batch;
int orbx_sim3_set_batch_device(orbx_sim3* s, const orbx_sim3_batch* in, void* stream);

/* iterate(n_iterations, bNoMore, vbInliers, nInliers) (cc:188-274) on every candidate of the
 * batch in force; find() (cc:277-281) is n_iterations = max_iterations.  Per candidate, with
 * inl_k the inlier count of absolute iteration k (err1 < thr1 && err2 < thr2, strict, cc:460):
 * inl_k >= mnBestInliers replaces the best state (a tie goes to the later iteration), and if
 * also inl_k > min_inliers the call returns that hypothesis: found 1, n_inliers, T12, and
 * inliers [n1] set at mvnIndices1 (entries beyond n1 are left untouched); no_more stays 0 on
 * that return.  Otherwise found 0, n_inliers 0, all flags 0, T12 all 0 (the empty Mat), and
 * no_more = mnIterations >= the cap.  N < min_inliers (cc:195) or N < 3: no_more at once, no
 * iteration.  A hypothesis whose |v| is exactly 0 (cc:371, identical point sets) is NaN, has
 * 0 inliers, and becomes the best state while mnBestInliers is 0, as IEEE gives it.
 *   best_R [9], best_t [3], best_s: GetEstimatedRotation / Translation / Scale (NaN before
 *   any best state); best_inliers = mnBestInliers; best_iteration = the absolute iteration
 *   that holds the best state, -1 if none; iterations = mnIterations after the call; n_pairs
 *   = N; status = the ORBX_SIM3_STATUS_* bits.  Every output is a nullable device array
 *   (host pointers to one candidate's for orbx_sim3_iterate). */
typedef struct {
    int32_t* found;           /* [B] */
    int32_t* no_more;         /* [B] */
    int32_t* n_inliers;       /* [B] */
    uint8_t* inliers;         /* [B][cap] */
    float* T12;               /* [B][16] */
    float* best_R;            /* [B][9] */
    float* best_t;            /* [B][3] */
    float* best_s;            /* [B] */
    int32_t* best_inliers;    /* [B] */
    int32_t* best_iteration;  /* [B] */
    int32_t* iterations;      /* [B] */
    int32_t* n_pairs;         /* [B] */
    int32_t* status;          /* [B] */
} orbx_sim3_result;
int orbx_sim3_iterate_device(orbx_sim3* s, int n_iterations, const orbx_sim3_result* out, void* stream);

/* The single-candidate host forms: every pointer of the structs is a host pointer (batch 1;
 * draws [max_iterations][3] is copied).  orbx_sim3_set uploads once; orbx_sim3_iterate runs
 * the batch kernels with B = 1, synchronises once and gives the same bytes as the batch form
 * gives that candidate.  Its wall time is the matcher's orbx_matcher_last_call_us. */
int orbx_sim3_set(orbx_sim3* s, const orbx_sim3_batch* in);
int orbx_sim3_iterate(orbx_sim3* s, int n_iterations, const orbx_sim3_result* out);

/* The reference's draws for n correspondences: draws [iterations][3], draw j =
 * RandomInt(0, n - 1 - j) = int(((double)rand() / ((double)RAND_MAX + 1.0)) * (n - j))
 * (DUtils/Random.cpp:47-49) over the C library's rand(); 0, without a rand() call, where
 * n - j <= 0.  One deviation: the draws of all iterations are taken up front, where the
 * reference stops consuming rand() at the returning iteration.  Host only, no GPU. */
int orbx_sim3_draws(int32_t* draws, int n, int iterations);

/* ---- PnPsolver: EPnP under RANSAC for a batch of relocalisation candidates ----
 * PnPsolver (include/PnPsolver.h, src/PnPsolver.cc:80-1345) as Tracking::Relocalization drives
 * it (Tracking.cc:1511-1684: one solver per candidate keyframe, iterate(5) round-robin), for B
 * candidates in HBM, a candidate being one pair (lost frame, candidate keyframe): the link
 * between orbx_search_by_bow_frame and orbx_pose_optimization_batch_device.  Float inputs are
 * widened to double, everything after is double except CheckInliers' mixed precision (below),
 * poses are rounded to float once per result.  No sum crosses lanes in floating point: a
 * candidate's results are the same bytes whatever the batch around it and however its
 * iterations are cut into calls.  The host reads nothing back between a set and the end of
 * an iterate.  DESIGN.md §4.21.
 *
 * What the reference leaves to OpenCV is fixed here (csrc/orbx_epnp.h): the SVDs of the
 * symmetric 3x3 PW0^T PW0 and 12x12 M^T M are a one-sided cyclic Jacobi on the matrix itself
 * (pairs (p, q), p < q, in lexicographic order; a pair is rotated unless gamma == 0 or |gamma|
 * <= 8 eps sqrt(alpha beta); the sweeps end with the first that rotates nothing, at most 30),
 * values descending with the higher index the smaller on a tie, vectors as the Jacobi leaves
 * them (no sign normalisation), v[0..3] the vectors of the four smallest values, smallest
 * first; cvInvert(CC) is rows u_i^T / k_i in closed form (zero where k_i == 0);
 * cvSolve(CV_SVD) is least squares through the same Jacobi on L, dropping the columns with
 * |b_j| <= 2 eps sum |b_k|; qr_solve (cc:1211-1345) is restated operation for operation with
 * its eta == 0 return, the increment starting at 0; estimate_R_and_t's 3x3 SVD is the
 * Initializer's (u_2 = u_0 x u_1 on b_2's side).  With minimal sets of 4 the hypotheses
 * depend on these choices; what a call returns after Refine() does not where the keypoints
 * are exact.
 *
 * The library owns no random generator: the caller supplies the four draws of every
 * iteration (orbx_pnp_draws gives the reference's).
 *
 * orbx_pnp_create (the workspace and per-candidate state for up to max_batch candidates of up
 * to cap slots and max_draws <= ORBX_PNP_MAX_DRAWS iterations with draws) borrows the
 * matcher's device and stream; the matcher must outlive it.  orbx_pnp_destroy waits for that
 * stream; after the library's unload destructor it releases nothing. */
#define ORBX_PNP_MAX_DRAWS 4096
#define ORBX_PNP_STATUS_BAD_DRAW 1 /* status bit 0: a walked iteration had a draw outside [0, N - j) */
#define ORBX_PNP_STATUS_NO_DRAWS 2 /* status bit 1: a call ended at an iteration >= n_draws */
typedef struct orbx_pnp orbx_pnp;
int orbx_pnp_create(orbx_matcher* m, int max_batch, int cap, int max_draws, orbx_pnp** out);
void orbx_pnp_destroy(orbx_pnp* s);

/* The constructor (cc:80-128) and SetRansacParameters(probability, min_inliers,
 * max_iterations, min_set, epsilon, th2) (cc:141-190) for `batch` candidates of one camera.
 *   Slot i < n of a candidate is kept iff matches[i] (vpMapPointMatches, as
 *   orbx_search_by_bow_frame writes it: the MapPoint id, -1 for none) lies in [0, n_mp); any
 *   negative id or one outside the table skips the slot (the caller maps NULL and isBad() to
 *   -1; cc:96-118).  Kept slots in slot order are the N correspondences (mvKeyPointIndices):
 *   mvP2D = kps[i].pt (mvKeysUn), mvP3Dw = mp_pos[matches[i]], mvMaxError =
 *   level_sigma2[octave] * th2 as a float product (cc:189), octaves clamped into [0, nlevels).
 *   The parameters follow cc:141-183 with their quirks, evaluated by the host's libm for every
 *   n in 0..cap and looked up on the device at N: mRansacMinInliers = max(int((float)N *
 *   epsilon), min_inliers, min_set); epsilon is raised to (float)mRansacMinInliers / N;
 *   mRansacMaxIts = 1 if mRansacMinInliers == N, else ceil(log(1 - p) / log(1 - pow(epsilon,
 *   3))) (the exponent is 3), clamped with max(1, min(., max_iterations)).  Only min_set == 4
 *   is accepted (ORBX_ERR_ARG otherwise).  mnIterations and mnBestInliers are reset to 0.
 *   draws [batch][n_draws][4], n_draws >= max_iterations, is read by the later iterate calls,
 *   indexed by the absolute iteration, and must stay valid until the next set: draw j of an
 *   iteration is RandomInt(0, N - 1 - j) (cc:239) and must lie in [0, N - j); otherwise that
 *   iteration has a NaN hypothesis and 0 inliers, and ORBX_PNP_STATUS_BAD_DRAW is set once it
 *   is walked.  The four are applied without replacement by the swap-with-last of cc:239-249.
 * level_sigma2 is a host array, every other pointer is a device pointer (all are host
 * pointers, and batch is 1, for orbx_pnp_set).  Asynchronous on `stream` (or the matcher's);
 * the calls on one solver share its workspace, so the caller keeps them in order. */
typedef struct {
    int batch;
    int cap;                    /* slots per candidate row, <= the solver's cap */
    const orbx_keypoint* kps;   /* [B][cap] F.mvKeysUn */
    const int32_t* n;           /* [B] vpMapPointMatches.size(), clamped into [0, cap] */
    const int32_t* matches;     /* [B][cap] vpMapPointMatches as MapPoint ids, -1 = none */
    int n_mp;                   /* MapPoints in the table */
    const float* mp_pos;        /* [n_mp][3] GetWorldPos() */
    const float* level_sigma2;  /* host: F.mvLevelSigma2 (nlevels) */
    int nlevels;
    float fx, fy, cx, cy;       /* F.fx F.fy F.cx F.cy */
    double probability;         /* in (0, 1): 0.99 */
    int min_inliers;            /* 10 */
    int max_iterations;         /* 300; <= n_draws */
    int min_set;                /* 4 */
    float epsilon;              /* in [0, 1]: 0.5 */
    float th2;                  /* 5.991 */
    const int32_t* draws;       /* [B][n_draws][4] */
    int n_draws;                /* <= the solver's max_draws */
} orbx_pnp_batch;
int orbx_pnp_set_batch_device(orbx_pnp* s, const orbx_pnp_batch* in, void* stream);

/* iterate(n_iterations, bNoMore, vbInliers, nInliers) (cc:200-323) on every candidate of the
 * batch in force; find() (cc:193-197) is n_iterations = max_iterations on a fresh set.  The
 * loop condition is `mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`
 * (cc:226, an OR): the first call runs to the iteration cap unless it returns, a later call
 * runs n_iterations more, beyond the cap.  An iteration whose absolute index is >= n_draws
 * is not run: the call ends with found 0, no_more 1 and ORBX_PNP_STATUS_NO_DRAWS.
 *   With inl_k the CheckInliers count of iteration k's hypothesis (compute_pose on its four
 *   correspondences), the iteration qualifies if inl_k >= mRansacMinInliers; inl_k >
 *   mnBestInliers then replaces the best state (a tie keeps the earlier iteration; mBestTcw is
 *   rounded to float there, cc:270-276), and Refine() (cc:326-378) runs compute_pose on
 *   mvbBestInliers -- the best state's, not the current hypothesis' -- and CheckInliers for
 *   its pose; it succeeds on a refined count > mRansacMinInliers (strict).  On success the call
 *   returns found 1, refined 1, the refined Tcw, the refined flags at mvKeyPointIndices and
 *   their count; no_more stays 0.  Refine is a function of the best state alone, so its
 *   result is computed when the best state changes and reused by later qualifying iterations
 *   (a success is returned again by the next qualifying iteration, as the reference does).
 *   A call that ends without that return gives no_more = mnIterations >= mRansacMaxIts, and
 *   then, if mnBestInliers >= mRansacMinInliers, found 1, refined 0, mBestTcw, the best
 *   state's flags and count.  Otherwise found 0, n_inliers 0, all flags 0, Tcw all 0.
 *   N < mRansacMinInliers (cc:210): no_more at once, no iteration.
 *   CheckInliers (cc:381-418) keeps the reference's precision: Xc, Yc, invZc are the double
 *   expressions rounded to float, ue / ve double, distX / distY the double differences rounded
 *   to float, error2 = distX * distX + distY * distY in float with each operation rounded
 *   (never fused), error2 < mvMaxError[i] strict; a NaN error2 is an outlier.
 *   inliers / frame_mp [n] are written for the slots i < n only: frame_mp[i] = matches[i]
 *   where inliers[i], else -1 (Tracking.cc:1600-1612), so orbx_pose_optimization_batch_device
 *   can start from Tcw and frame_mp where they lie.  best_Tcw is mBestTcw (NaN before any best
 *   state), best_iteration the absolute iteration that holds it (-1 if none), iterations =
 *   mnIterations after the call, n_corr = N, min_inliers_used / max_its_used the adjusted
 *   parameters, status the ORBX_PNP_STATUS_* bits.  Every output is a nullable device array
 *   (host pointers to one candidate's for orbx_pnp_iterate). */
typedef struct {
    int32_t* found;             /* [B] */
    int32_t* no_more;           /* [B] */
    int32_t* n_inliers;         /* [B] */
    uint8_t* inliers;           /* [B][cap] */
    float* Tcw;                 /* [B][12] rows 0..2, as orbx_pose_optimization_batch.Tcw reads it */
    int32_t* frame_mp;          /* [B][cap] */
    float* best_Tcw;            /* [B][12] */
    int32_t* best_inliers;      /* [B] */
    int32_t* best_iteration;    /* [B] */
    int32_t* refined;           /* [B] whether Tcw came from Refine() */
    int32_t* iterations;        /* [B] */
    int32_t* n_corr;            /* [B] */
    int32_t* min_inliers_used;  /* [B] */
    int32_t* max_its_used;      /* [B] */
    int32_t* status;            /* [B] */
} orbx_pnp_result;
int orbx_pnp_iterate_device(orbx_pnp* s, int n_iterations, const orbx_pnp_result* out, void* stream);

/* The single-candidate host forms: every pointer of the structs is a host pointer (batch 1;
 * draws [n_draws][4] is copied).  orbx_pnp_set uploads once; orbx_pnp_iterate runs the batch
 * kernels with B = 1, synchronises once and gives the same bytes as the batch form gives that
 * candidate.  Its wall time is the matcher's orbx_matcher_last_call_us. */
int orbx_pnp_set(orbx_pnp* s, const orbx_pnp_batch* in);
int orbx_pnp_iterate(orbx_pnp* s, int n_iterations, const orbx_pnp_result* out);

/* The reference's draws for n correspondences: draws [iterations][4], draw j =
 * RandomInt(0, n - 1 - j) (DUtils/Random.cpp:47-49) over the C library's rand(); 0, without a
 * rand() call, where n - j <= 0.  The same deviation as orbx_sim3_draws: the draws of all
 * iterations are taken up front.  Host only, no GPU. */
int orbx_pnp_draws(int32_t* draws, int n, int iterations);

/* ---- Optimizer::OptimizeSim3: the Sim3 refinement of loop candidates ----
 * Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (src/Optimizer.cc:
 * 1173-1358) as LoopClosing::ComputeSim3 calls it between SearchBySim3 and the nInliers >= 20
 * test (LoopClosing.cc:344-355), with the parts of g2o it runs (VertexSim3Expmap,
 * EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ with g2o's numeric Jacobian, g2o::Sim3,
 * RobustKernelHuber, the dense 7x7 LDLT, OptimizationAlgorithmLevenberg), for B candidates in
 * HBM in one launch: one persistent workgroup per candidate runs optimize(5), the chi2 test,
 * optimize(5 or 10) from the current estimate and the final test.  Float inputs are widened to
 * double, everything after is double, outputs are rounded to float once.  Sums over edges have
 * a fixed shape (no floating-point atomics): a candidate's results are the same bytes
 * whatever the batch around it.  DESIGN.md §4.17.
 *   Pairs, in slot order: slot i < n1 is kept iff mp1[i] and matches12[i] lie in [0, n_mp)
 *   and idx2[i] in [0, n2) (the caller maps NULL, isBad() and GetIndexInKeyFrame() < 0 to
 *   -1).  P3D1c = R1w mp_pos[mp1[i]] + t1w and P3D2c likewise are rounded to float as the
 *   reference's CV_32F matrices are; obs1 = kps1[i], obs2 = kps2[idx2[i]]; information =
 *   I * inv_level_sigma2_k[octave] of the respective keyframe (octaves clamped into
 *   [0, nlevels)); the Huber delta is the float sqrt(th2).
 *   matches12 is in/out: the entries of pairs rejected by either test (e12.chi2() > th2 ||
 *   e21.chi2() > th2, in double) become -1, as vpMatches1 entries become NULL.
 *   Outputs: R12_opt / t12_opt / s12_opt = rotation().toRotationMatrix(), translation(),
 *   scale() of the recovered vertex; ninliers = the return value nIn; ncorr =
 *   nCorrespondences; nbad = nBad of the first test; trace per optimisation {LM iterations
 *   run, linear solves tried}, 0 when not run.  nCorrespondences - nBad < 10 (cc:1331):
 *   ninliers 0, the Sim3 outputs are the inputs' bytes, the first test's rejections stay.
 *   R12 / t12 / s12 have the layout of orbx_sim3_result.best_R / best_t / best_s.
 * inv_level_sigma2_1 / _2, K1 and K2 are host arrays; every other pointer is a device
 * pointer.  ninliers, ncorr, nbad and trace may be NULL.  Asynchronous on `stream` (or the
 * matcher's). */
typedef struct {
    int batch;
    int cap1;                          /* slots per candidate row */
    const int32_t* n1;                 /* [B] vpMatches1.size(), clamped into [0, cap1] */
    const orbx_keypoint* kps1;         /* [B][cap1] pKF1->mvKeysUn */
    const int32_t* mp1;                /* [B][cap1] pKF1->GetMapPointMatches() as MapPoint ids */
    int32_t* matches12;                /* [B][cap1] in/out: vpMatches1 as MapPoint ids */
    const int32_t* idx2;               /* [B][cap1] GetIndexInKeyFrame(pKF2) of matches12[i] */
    int cap2;
    const int32_t* n2;                 /* [B] pKF2's keypoints, clamped into [0, cap2] */
    const orbx_keypoint* kps2;         /* [B][cap2] pKF2->mvKeysUn */
    int n_mp;                          /* MapPoints in the table */
    const float* mp_pos;               /* [n_mp][3] GetWorldPos() */
    const float* Tcw1;                 /* [B][12] pKF1's pose, rows 0..2 */
    const float* Tcw2;                 /* [B][12] pKF2's pose */
    const float* inv_level_sigma2_1;   /* host: pKF1->mvInvLevelSigma2 (nlevels) */
    const float* inv_level_sigma2_2;   /* host: pKF2->mvInvLevelSigma2 (nlevels) */
    int nlevels;
    const float* K1;                   /* host: fx fy cx cy of pKF1 */
    const float* K2;                   /* host: ... of pKF2 */
    const float* R12;                  /* [B][9] */
    const float* t12;                  /* [B][3] */
    const float* s12;                  /* [B] */
    float th2;
    int fix_scale;
    float* R12_opt;                    /* [B][9] out */
    float* t12_opt;                    /* [B][3] out */
    float* s12_opt;                    /* [B] out */
    int32_t* ninliers;                 /* [B] out or NULL */
    int32_t* ncorr;                    /* [B] out or NULL */
    int32_t* nbad;                     /* [B] out or NULL */
    int32_t* trace;                    /* [B][2][2] out or NULL */
} orbx_optimize_sim3_batch;
int orbx_optimize_sim3_batch_device(orbx_matcher* m, const orbx_optimize_sim3_batch* os, void* stream);

/* The single-candidate host form: every pointer of the struct is a host pointer and batch is
 * 1 (n1 / n2 point to one count each; cap1 >= *n1, cap2 >= *n2).  One upload, the batch kernel
 * with B = 1, one synchronisation; the same bytes as the batch form gives that candidate. */
int orbx_optimize_sim3(orbx_matcher* m, const orbx_optimize_sim3_batch* os);

/* ---- Optimizer::LocalBundleAdjustment: batched Schur-complement Levenberg-Marquardt ----
 * Optimizer::LocalBundleAdjustment (src/Optimizer.cc:586-853) from the assembled graph to the
 * recovered estimates, as LocalMapping::Run calls it (LocalMapping.cc:75), with the g2o it
 * runs (OptimizationAlgorithmLevenberg, BlockSolver_6_3 with the Schur complement,
 * EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ with their analytic Jacobians, the robust
 * quadratic form of BaseBinaryEdge, RobustKernelHuber, SE3Quat), for B local maps in HBM in one
 * launch: one persistent workgroup per problem runs optimize(5), the chi2 / depth test,
 * optimize(10) on the edges that passed and the final test.  The covisibility walk that
 * chooses the keyframes and points (cc:526-583) stays with the caller (or with
 * orbx_local_ba_assemble_device on a covisibility graph), as does the erasure of the flagged
 * observations (orbx_local_ba_apply_device); the UpdateNormalAndDepth of the write-back
 * (cc:828-853) is orbx_update_normal_and_depth_device over pt_id after a refresh of the
 * observations.  The stop flag (pbStopFlag)
 * is not supported: bDoMore is always true.  Float inputs are widened to double, everything
 * after is double (but the two float intermediates of the stereo projection), outputs are
 * rounded to float once.  Every sum has a fixed shape (no floating-point atomics) and no
 * workgroup waits on another: a problem's results are the same bytes whatever the batch
 * around it.  The reduced system is factored by a dense unpivoted LDL^T in natural order;
 * only an exactly zero pivot is a failed solve.  DESIGN.md §4.20.
 *   Problem b owns rows kf_off[b] .. kf_off[b + 1] of the keyframe table and rows pt_off[b] ..
 *   pt_off[b + 1] of the point table; point j owns observations obs_off[j] .. obs_off[j + 1]
 *   (offsets over the whole tables, ascending).  Observation o is keypoint obs_kp[o] of the
 *   problem's keyframe obs_kf[o] (an index within the problem's rows), whose keypoints are row
 *   kf_slot[] of kps / u_right.  Edge order is point order, then the order within a point; a
 *   keyframe appears once among a point's observations.  An observation with an index outside
 *   its table, or whose keyframe an earlier observation of its point names, is no edge (its flags
 *   stay 0) and sets
 *   ORBX_LOCAL_BA_STATUS_BAD_INDEX.
 *   kf_fixed: lFixedCameras and mnId == 0.  An edge is monocular iff u_right < 0 (cc:679; all
 *   are when u_right is NULL); information = I * inv_level_sigma2[octave] (octaves clamped
 *   into [0, nlevels)); the Huber deltas are the floats sqrt(5.991) / sqrt(7.815).
 *   Outputs: kf_Tcw_opt = Converter::toCvMat(SE3Quat) of every keyframe that is not fixed, the
 *   input's bytes of a fixed one; pt_pos_opt; erase[o] = vToErase; level1[o] = the edge left
 *   the second optimisation; n_erase; trace per optimisation {LM iterations, linear solves};
 *   status = the ORBX_LOCAL_BA_STATUS_* bits.  A problem without a keyframe that may move
 *   (NO_FREE_KF), or with more of them than min(max_free_kf, ORBX_LOCAL_BA_MAX_FREE_KF)
 *   (CAPACITY), returns its inputs, no flag set and a zero trace.  An optimisation with no
 *   active edge, or none at a keyframe that may move, runs no iteration.
 * inv_level_sigma2 is a host array; every other pointer is a device pointer.  level1 and trace
 * may be NULL.  Asynchronous on `stream` (or the matcher's). */
#define ORBX_LOCAL_BA_MAX_FREE_KF 64
#define ORBX_LOCAL_BA_STATUS_CAPACITY 1
#define ORBX_LOCAL_BA_STATUS_NO_FREE_KF 2
#define ORBX_LOCAL_BA_STATUS_BAD_INDEX 4
typedef struct {
    int batch;
    const int32_t* kf_off;           /* [B + 1] */
    int n_kf;                        /* rows of the keyframe table */
    const float* kf_Tcw;             /* [n_kf][12] GetPose(), rows 0..2 */
    const uint8_t* kf_fixed;         /* [n_kf] */
    const int32_t* kf_slot;          /* [n_kf] row of kps / u_right */
    const int32_t* pt_off;           /* [B + 1] */
    int n_pt;                        /* rows of the point table */
    const float* pt_pos;             /* [n_pt][3] GetWorldPos() */
    const int32_t* obs_off;          /* [n_pt + 1] */
    int n_obs;
    const int32_t* obs_kf;           /* [n_obs] */
    const int32_t* obs_kp;           /* [n_obs] */
    int n_slots, cap;
    const orbx_keypoint* kps;        /* [n_slots][cap] mvKeysUn */
    const float* u_right;            /* [n_slots][cap] mvuRight, or NULL */
    const float* inv_level_sigma2;   /* host: mvInvLevelSigma2 (nlevels) */
    int nlevels;
    float fx, fy, cx, cy, bf;
    int max_free_kf;                 /* keyframes that may move per problem that the workspace is
                                        sized for; 0: ORBX_LOCAL_BA_MAX_FREE_KF */
    float* kf_Tcw_opt;               /* [n_kf][12] out */
    float* pt_pos_opt;               /* [n_pt][3] out */
    uint8_t* erase;                  /* [n_obs] out */
    uint8_t* level1;                 /* [n_obs] out or NULL */
    int32_t* n_erase;                /* [B] out */
    int32_t* trace;                  /* [B][2][2] out or NULL */
    int32_t* status;                 /* [B] out */
} orbx_local_ba_batch;
int orbx_local_bundle_adjustment_batch_device(orbx_matcher* m, const orbx_local_ba_batch* lba, void* stream);

/* The single-problem host form: every pointer of the struct is a host pointer and batch is 1
 * (kf_off = {0, n_kf}, pt_off = {0, n_pt}).  One upload, the batch kernel with B = 1, one
 * synchronisation; the same bytes as the batch form gives that problem. */
int orbx_local_bundle_adjustment(orbx_matcher* m, const orbx_local_ba_batch* lba);

/* ---- Optimizer::BundleAdjustment / GlobalBundleAdjustemnt: batched envelope Schur-complement LM ----
 * Optimizer::BundleAdjustment (src/Optimizer.cc:41-281) from the assembled graph (cc:79-233) to
 * the recovered estimates (cc:236-280), as Tracking::CreateInitialMapMonocular (Tracking.cc:761,
 * 20 iterations) and LoopClosing::RunGlobalBundleAdjustment (LoopClosing.cc:715, 10 iterations)
 * call it, for B maps in HBM in one launch: one persistent workgroup per problem runs
 * initializeOptimization() and one optimize(iterations) with the g2o of the local bundle
 * adjustment above (the same edges, Jacobians, quadratic form, Huber kernel, Schur complement
 * and Levenberg-Marquardt).  There are no chi2 or depth tests, no second optimisation and no
 * erase flags, and no cap on the keyframes: the reduced system S is a block envelope (skyline)
 * of 6 x 6 blocks in table order, factored by the LDL^T of the essential graph below, which
 * gives the bytes of the dense factorisation; only an exactly zero (or non-finite) pivot is a
 * failed solve, which is a rejected trial.  The stop flag (pbStopFlag) is not supported: the
 * iteration count is the caller's lever.  Float inputs are widened to double, everything after
 * is double (but the two float intermediates of the stereo projection), outputs are rounded to
 * float once.  Every sum has one owner and a fixed shape (no floating-point atomics) and no
 * workgroup waits on another: a problem's results are the same bytes whatever the batch around
 * it.  DESIGN.md §4.23.  With the caller: which keyframes and points are good (bad ones are
 * not passed), whether the results go to SetPose / SetWorldPos or to mTcwGBA / mPosGBA (the
 * nLoopKF switch), the spanning-tree propagation of LoopClosing.cc:740-800,
 * ComputeSceneMedianDepth and the rescale of the initial map.  The UpdateNormalAndDepth that
 * ends the write-back of a point when nLoopKF == 0 (cc:273, the CreateInitialMapMonocular path)
 * is orbx_update_normal_and_depth_device on pt_pos_opt and kf_Tcw_opt once they are in the
 * map's tables (§4.27).
 *   The tables are those of orbx_local_ba_batch, with the same rules for observations that
 *   are no edges (ORBX_GLOBAL_BA_STATUS_BAD_INDEX).  Edge order is point order, then the
 *   caller's order within a point (the reference's orders are pointer orders); the order of S
 *   is table order.  kf_fixed: mnId == 0 in the reference.  An edge is monocular iff
 *   u_right < 0; the Huber deltas are the floats sqrt(5.99) (cc:115 -- not the local bundle
 *   adjustment's 5.991) and sqrt(7.815), used iff robust != 0 (bRobust).
 *   iterations: nIterations; 0 means 10.  max_env_blocks: orbx_global_ba_envelope gives a
 *   problem's.  dense != 0 forces the full envelope (first[f] = 0; a test switch: the same
 *   bytes, F (F + 1) / 2 blocks).
 *   Outputs: kf_Tcw_opt = Converter::toCvMat(SE3Quat) of EVERY keyframe (cc:236-254 writes the
 *   fixed ones too, so a fixed pose comes back as its round trip through the normalised
 *   quaternion, not as its input bytes); pt_pos_opt; pt_included[j] = 0 for a point without an
 *   edge (vbNotIncludedMP, cc:223-228), which keeps its input bytes; trace = {LM iterations,
 *   linear solves}; chi2 = {initial, final} active robust chi2; status = the
 *   ORBX_GLOBAL_BA_STATUS_* bits.  A keyframe that may move but has no edge is not active and
 *   keeps its estimate.  A problem without a keyframe that may move (NO_FREE_KF; the reference
 *   is undefined for it), or whose envelope has more than max_env_blocks blocks (CAPACITY),
 *   returns its inputs' bytes, pt_included = 0 and a zero trace and chi2.  With no edge, or none
 *   at a keyframe that may move, no iteration runs.
 * inv_level_sigma2 is a host array; every other pointer is a device pointer.  trace and chi2
 * may be NULL.  Asynchronous on `stream` (or the matcher's). */
#define ORBX_GLOBAL_BA_STATUS_CAPACITY 1
#define ORBX_GLOBAL_BA_STATUS_NO_FREE_KF 2
#define ORBX_GLOBAL_BA_STATUS_BAD_INDEX 4
typedef struct {
    int batch;
    const int32_t* kf_off;           /* [B + 1] */
    int n_kf;                        /* rows of the keyframe table */
    const float* kf_Tcw;             /* [n_kf][12] GetPose(), rows 0..2 */
    const uint8_t* kf_fixed;         /* [n_kf] */
    const int32_t* kf_slot;          /* [n_kf] row of kps / u_right */
    const int32_t* pt_off;           /* [B + 1] */
    int n_pt;                        /* rows of the point table */
    const float* pt_pos;             /* [n_pt][3] GetWorldPos() */
    const int32_t* obs_off;          /* [n_pt + 1] */
    int n_obs;
    const int32_t* obs_kf;           /* [n_obs] */
    const int32_t* obs_kp;           /* [n_obs] */
    int n_slots, cap;
    const orbx_keypoint* kps;        /* [n_slots][cap] mvKeysUn */
    const float* u_right;            /* [n_slots][cap] mvuRight, or NULL */
    const float* inv_level_sigma2;   /* host: mvInvLevelSigma2 (nlevels) */
    int nlevels;
    float fx, fy, cx, cy, bf;
    int iterations;                  /* nIterations; 0: 10 */
    int robust;                      /* bRobust */
    int64_t max_env_blocks;          /* 6 x 6 blocks per problem that the workspace is sized for */
    int dense;                       /* test switch: the full envelope */
    float* kf_Tcw_opt;               /* [n_kf][12] out */
    float* pt_pos_opt;               /* [n_pt][3] out */
    uint8_t* pt_included;            /* [n_pt] out */
    int32_t* trace;                  /* [B][2] out or NULL */
    double* chi2;                    /* [B][2] out or NULL */
    int32_t* status;                 /* [B] out */
} orbx_global_ba_batch;
int orbx_global_bundle_adjustment_batch_device(orbx_matcher* m, const orbx_global_ba_batch* ga, void* stream);

/* The single-problem host form: every pointer of the struct is a host pointer and batch is 1
 * (kf_off = {0, n_kf}, pt_off = {0, n_pt}).  One upload, the batch kernel with B = 1, one
 * synchronisation; the same bytes as the batch form gives that problem. */
int orbx_global_bundle_adjustment(orbx_matcher* m, const orbx_global_ba_batch* ga);

/* The blocks of one problem's envelope: over the keyframes that are not fixed and have an
 * observation (an edge here: obs_kf in [0, n_kf) -- keypoints, slots, octaves and u_right are
 * not looked at, so this is an upper bound where the kernel finds observations that are no
 * edges), indexed in table order, sum of f - first[f] + 1 with first[f] the smallest index
 * among f and the keyframes that share a point with it.  Host only, no GPU. */
int orbx_global_ba_envelope(int n_kf, const uint8_t* kf_fixed, int n_pt, const int32_t* obs_off,
                            const int32_t* obs_kf, int n_obs, int64_t* blocks);

/* ---- Optimizer::OptimizeEssentialGraph: batched Sim3 pose-graph Levenberg-Marquardt ----
 * Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:873-1150) from the assembled graph to
 * the recovered estimates, as LoopClosing::CorrectLoop calls it (LoopClosing.cc:621), with the
 * g2o it runs (OptimizationAlgorithmLevenberg with setUserLambdaInit(1e-16) and optimize(20),
 * BlockSolver_7_3 with nothing marginalised, VertexSim3Expmap, EdgeSim3 with information = I,
 * no robust kernel and g2o's central-difference Jacobians, Sim3::log in full), for B maps in
 * HBM in one launch: one persistent workgroup per problem.  Float inputs are widened to
 * double, everything after is double, outputs are rounded to float once.  Every sum has one
 * owner and a fixed shape (no floating-point atomics) and no workgroup waits on another: a
 * problem's results are the same bytes whatever the batch around it.  The linear system is
 * factored by a block-envelope (skyline) LDL^T without pivoting in natural (mnId) order that
 * gives the bytes of the dense factorisation; only an exactly zero (or non-finite) pivot is
 * a failed solve, which is a rejected trial.  There is no cap on keyframes.  DESIGN.md §4.22.
 * Before it, CorrectLoop's Sim3 propagation and first map-point correction
 * (LoopClosing.cc:482-571) are orbx_correct_loop_propagate_device and the graph is built on the
 * device by orbx_essential_graph_assemble_device; after it, the UpdateNormalAndDepth of
 * cc:1148 is orbx_update_normal_and_depth_device on pt_pos_opt and kf_Tcw_opt (all three
 * below).  With the caller: SearchAndFuse's map mutation between the two and
 * the write-back of the results into its map (the global bundle adjustment that follows is
 * orbx_global_bundle_adjustment_batch_device above).
 *   Problem b owns rows kf_off[b] .. kf_off[b + 1] of the keyframe table (the good keyframes
 *   in ascending mnId), edge_off[b] .. of the edge table and pt_off[b] .. of the point table
 *   (offsets over the whole tables, ascending).  kf_Tcw is the pose that gives the
 *   non-corrected Sim3(Rcw, tcw, 1) of cc:994-1000 -- for a corrected keyframe the pose from
 *   before CorrectLoop overwrote it (LoopClosing.cc:518-522).  The vertex estimate vScw is
 *   corr_S[kf_corr[k]] (q xyzw, t, s: CorrectedSim3) where kf_corr[k] >= 0, the non-corrected
 *   Sim3 otherwise.  loop_kf[b] (an index within the problem's rows) is fixed.
 *   Edge e joins vertex 0 = edge_v[e][0] = i and vertex 1 = edge_v[e][1] = j (indices within
 *   the problem's rows); its measurement is vScw[j] * vScw[i]^-1 for edge_kind 0 (the
 *   LoopConnections edges, cc:954-986) and Snc[j] * Snc[i]^-1 for kind 1 (spanning tree, loop
 *   and covisibility edges, cc:989-1089).  Edge order is the caller's, which is g2o's
 *   insertion order (essential_graph_edges in the Python package writes it, with the
 *   keyframes walked in ascending mnId); a pair may repeat, in either orientation.  An edge with an index outside the
 *   rows, i == j or an unknown kind is no edge and sets ORBX_ESSENTIAL_GRAPH_STATUS_BAD_INDEX,
 *   as does a kf_corr outside [-1, n_corr) (taken as -1) and a pt_ref outside the rows (the
 *   point keeps its input bytes).  A keyframe without a valid edge keeps its estimate.
 *   Outputs: kf_Tcw_opt = [R | t / s] of every keyframe's Sim3 (the fixed one's too, as in the
 *   reference); pt_pos_opt = correctedSwr.map(Srw.map(P)) with r = pt_ref[p] (cc:1125-1142:
 *   mnCorrectedReference where mnCorrectedByKF is the current keyframe, the reference keyframe
 *   otherwise -- resolved by the caller); Scw_opt = the Sim3 estimates; trace = {LM
 *   iterations, linear solves}; chi2 = {initial, final}; status = the
 *   ORBX_ESSENTIAL_GRAPH_STATUS_* bits.  A problem whose loop_kf lies outside its rows
 *   (NO_FIXED_KF), or whose envelope has more than max_env_blocks blocks (CAPACITY), returns
 *   its inputs (Scw_opt = vScw) with a zero trace and chi2.  If no keyframe may move and has
 *   an edge, no iteration runs.
 *   iterations: 0 means the reference's 20.  dense != 0 forces the full envelope (first[f] =
 *   0; a test switch: the same bytes, F (F + 1) / 2 blocks).
 * Every pointer is a device pointer.  Scw_opt, trace and chi2 may be NULL.  Asynchronous on
 * `stream` (or the matcher's). */
#define ORBX_ESSENTIAL_GRAPH_STATUS_CAPACITY 1
#define ORBX_ESSENTIAL_GRAPH_STATUS_NO_FIXED_KF 2
#define ORBX_ESSENTIAL_GRAPH_STATUS_BAD_INDEX 4
typedef struct {
    int batch;
    const int32_t* kf_off;           /* [B + 1] */
    int n_kf;                        /* rows of the keyframe table */
    const float* kf_Tcw;             /* [n_kf][12] rows 0..2 of the non-corrected pose */
    const int32_t* kf_corr;          /* [n_kf] row of corr_S, or -1 */
    const double* corr_S;            /* [n_corr][8] CorrectedSim3: q xyzw, t, s */
    int n_corr;
    const int32_t* loop_kf;          /* [B] */
    const int32_t* edge_off;         /* [B + 1] */
    int n_edges;
    const int32_t* edge_v;           /* [n_edges][2] */
    const int32_t* edge_kind;        /* [n_edges] */
    const int32_t* pt_off;           /* [B + 1] */
    int n_pt;
    const float* pt_pos;             /* [n_pt][3] GetWorldPos() */
    const int32_t* pt_ref;           /* [n_pt] */
    int fix_scale;                   /* bFixScale */
    int iterations;                  /* 0: 20 */
    int64_t max_env_blocks;          /* 7 x 7 blocks per problem that the workspace is sized for
                                        (orbx_essential_graph_envelope gives a problem's) */
    int dense;                       /* test switch: the full envelope */
    float* kf_Tcw_opt;               /* [n_kf][12] out */
    float* pt_pos_opt;               /* [n_pt][3] out */
    double* Scw_opt;                 /* [n_kf][8] out or NULL */
    int32_t* trace;                  /* [B][2] out or NULL */
    double* chi2;                    /* [B][2] out or NULL */
    int32_t* status;                 /* [B] out */
} orbx_essential_graph_batch;
int orbx_optimize_essential_graph_batch_device(orbx_matcher* m, const orbx_essential_graph_batch* eg, void* stream);

/* The single-problem host form: every pointer of the struct is a host pointer and batch is 1
 * (kf_off = {0, n_kf}, edge_off = {0, n_edges}, pt_off = {0, n_pt}).  One upload, the batch
 * kernel with B = 1, one synchronisation; the same bytes as the batch form gives that problem. */
int orbx_optimize_essential_graph(orbx_matcher* m, const orbx_essential_graph_batch* eg);

/* The blocks of one problem's envelope: over the keyframes other than `fixed` that have an
 * edge (an edge here: both indices in [0, n_kf) and different -- the kinds are not looked at),
 * indexed in order, sum of f - first[f] + 1 with first[f] the smallest index among f and its
 * neighbours.  Host only, no GPU. */
int orbx_essential_graph_envelope(int n_kf, int fixed, const int32_t* edge_v, int n_edges, int64_t* blocks);

/* ---- LocalMapping::CreateNewMapPoints: triangulation and tests of the matched pairs ----
 * The second half of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:307-501) for the
 * vMatchedPairs that orbx_search_for_triangulation_batch_device left in HBM, with
 * KeyFrame::UnprojectStereo (src/KeyFrame.cc:666-679) and MapPoint::UpdateNormalAndDepth for
 * the two observations of a new point (src/MapPoint.cc:386-439).  One thread per matched pair.
 * Float inputs are widened to double, everything after is double, outputs are rounded to float
 * once; no floating-point value crosses lanes, so a pair's bytes are the same whatever the
 * batch around it.  DESIGN.md §4.18.
 *
 * One KeyFrame as the triangulation reads it.  Device pointers (cap slots each), except Tcw. */
typedef struct {
    const orbx_keypoint* keys_un; /* mvKeysUn */
    const orbx_keypoint* keys;    /* mvKeys (UnprojectStereo reads these) or NULL: keys_un */
    const float* u_right;         /* mvuRight or NULL (monocular) */
    const float* depth;           /* mvDepth or NULL: the float mbf / (keys[i].x - u_right[i]), as
                                   * ComputeStereoMatches derived it (Frame.cc:852-856); gathered
                                   * neighbours carry u_right but not mvDepth */
    const int32_t* n;             /* N (one int; min(*n, cap) keypoints are read) */
    float Tcw[12];                /* host: mTcw rows 0..2 */
} orbx_keyframe_geom_device;

/* Per pair slot [p][k], k < npairs[p] (slots past a row's count are neither read nor written).
 * Every pointer may be NULL.
 *   reason: 0 accepted, 1 no branch (low parallax and no stereo; also a stereo branch whose
 *     mvDepth is not positive, where the reference dereferences an empty Mat), 2 w == 0 (cc:384),
 *     3 z1 <= 0, 4 z2 <= 0, 5 reprojection in KF1 (cc:412-430), 6 reprojection in KF2 (cc:437-454;
 *     its stereo form uses KF1's mbf, cc:446: the call has one mbf), 7 dist1 == 0 || dist2 == 0,
 *     8 scale ratio (cc:475), 9 idx1 outside [0, N1) or idx2 outside [0, N2).
 *   method: the branch taken, 1 linear (cc:369-387), 2 UnprojectStereo of KF1, 3 of KF2, 0 none
 *     (reasons 1 and 9).  A rejected slot keeps the branch it was rejected after.
 *   pos, normal, max_distance, min_distance: the new MapPoint's mWorldPos, mNormalVector,
 *     mfMaxDistance, mfMinDistance (the orbx_mappoints_device columns); 0 in rejected slots.
 *   nnew[p]: accepted slots of row p; new_idx[p][j], j < nnew[p]: their k in pair order, the
 *     order the reference creates the MapPoints in (entries from nnew[p] on are not written).
 * Octaves are clamped into [0, nlevels).  ratioFactor = 1.5 * scale_factors[1]. */
typedef struct {
    uint8_t* reason;       /* [P][cap] */
    uint8_t* method;       /* [P][cap] */
    float* pos;            /* [P][cap][3] */
    float* normal;         /* [P][cap][3] */
    float* max_distance;   /* [P][cap] */
    float* min_distance;   /* [P][cap] */
    int32_t* nnew;         /* [P] */
    int32_t* new_idx;      /* [P][cap] */
} orbx_new_mappoints;

/* For p < npairs: KF1 = kfs[pairs[2p]], KF2 = kfs[pairs[2p+1]] (host table, the one the search
 * call takes), matched pairs d_pairs[p][k] = (idx1, idx2), k < min(d_npairs[p], cap), exactly as
 * orbx_search_for_triangulation_batch_device leaves them.  `cam` gives fx, fy, cx, cy and the
 * level tables (nlevels, scale_factors, level_sigma2); mb and mbf are KF1's (the reference
 * reads pKF2->mb for KF2's stereo parallax: one rig, one value).  Enqueued on `stream` (or the
 * matcher's) without synchronising; the host tables are staged through pinned memory, so they
 * may be reused on return.  cap <= 8192.
 * Pairs are independent: in the reference a point created with neighbour i makes
 * SearchForTriangulation skip that idx1 for neighbour i+1 (GetMapPoint(idx1) is set by then);
 * the batched search does not see that, and neither does this call -- a caller that wants the
 * reference's sequence drops, in neighbour order, the new points whose idx1 an earlier
 * neighbour already filled.  ComputeDistinctiveDescriptors of the new points is
 * orbx_compute_distinctive_descriptors_device over their two observations; adding them to the
 * map (orbx_mappoints_device rows, AddObservation, AddMapPoint) stays with the caller.
 * ORBX_ERR_ARG, decided before any device call: a null required pointer, cap <= 0 or > 8192, a
 * negative count, bad level tables, a pair index outside [0, nkf). */
int orbx_triangulate_pairs_batch_device(orbx_matcher* m, int nkf, const orbx_keyframe_geom_device* kfs,
                                        const orbx_frame_view* cam, int npairs, const int32_t* pairs, int cap,
                                        const int32_t* d_pairs, const int32_t* d_npairs, float mb, float mbf,
                                        const orbx_new_mappoints* out, void* stream);

/* The single-pair host form: every pointer of kf1, kf2 and out is a host pointer (kf->n points
 * to one count, arrays of *n entries), matched: nmatched x (idx1, idx2), nmatched <= 8192; out's
 * rows have nmatched slots (nnew: one int).  One upload, the batch kernel with one keyframe
 * pair, one synchronisation; the same bytes as the batch form gives that pair.  Its wall time
 * is orbx_matcher_last_call_us. */
int orbx_triangulate_pairs(orbx_matcher* m, const orbx_keyframe_geom_device* kf1,
                           const orbx_keyframe_geom_device* kf2, const orbx_frame_view* cam, int nmatched,
                           const int32_t* matched, float mb, float mbf, const orbx_new_mappoints* out);

/* ---- Initializer: H / F RANSAC and two-view reconstruction of monocular initialisation ----
 * Initializer::Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated)
 * (src/Initializer.cc:64-165) with everything under it -- Normalize (cc:1138-1200),
 * FindHomography / FindFundamental (cc:179-309), ComputeH21 / ComputeF21 (cc:318-440),
 * CheckHomography (cc:450-590), CheckFundamental (cc:597-735), ReconstructF (cc:749-890),
 * ReconstructH (cc:905-1097), Triangulate, CheckRT (cc:1215-1379), DecomposeE -- for B
 * independent frame pairs in HBM: the consumer of orbx_search_for_initialization's matches12.
 * Float inputs are widened to double, everything after is double (thresholds 5.991, 3.841,
 * 0.99998, 1.00001, 0.40 included), outputs are rounded to float once.  Floating-point sums
 * over keypoints or correspondences have a fixed shape that depends only on n1 / n2 / N: a
 * frame pair's bytes do not depend on the batch around it.  The host reads nothing back
 * during a call.  DESIGN.md §4.19.
 *   Correspondences: the slots i < n1 with 0 <= matches12[i] < n2, in slot order (mvMatches12,
 *   cc:77-85); any other value skips the slot; N is their count.  Normalize runs over all n1
 *   (n2) keypoints; a zero deviation gives inf / NaN as IEEE gives it, such hypotheses score 0
 *   through failed comparisons and never become best.
 *   sets [B][max_iterations][8] are indices into the N correspondences (mvSets;
 *   orbx_initializer_sets gives the reference's).  A set with an index outside [0, N) or a
 *   repeated index scores 0 for both models and sets ORBX_INIT_STATUS_BAD_SET.  N < 8: no
 *   iteration, ok = 0, ORBX_INIT_STATUS_TOO_FEW (the reference is undefined there).
 *   Best hypothesis: currentScore > score, strictly, from score = 0 (cc:235, 303): a tie keeps
 *   the EARLIER iteration -- the opposite of Sim3Solver's `>=` (orbx_sim3_iterate_device).  If
 *   no iteration scores above 0 the model matrix is the empty Mat (all 0) without inliers.
 *   RH = SH / (SH + SF) > 0.40 reconstructs from H, otherwise (NaN included) from F, both with
 *   minParallax 1.0 and minTriangulated 50.  The SVDs are one-sided Jacobi iterations in
 *   double; their sign and order freedom only permutes the 4 / 8 motion hypotheses, and both
 *   selection rules are blind to that.
 * K is a host array; every other pointer is a device pointer (all are host pointers, and
 * batch is 1, for orbx_initializer_initialize).
 *
 * orbx_initializer_create (the workspace for up to max_batch pairs of up to kcap <= 8192
 * keypoints and max_iterations <= ORBX_INIT_MAX_ITERATIONS) borrows the matcher's device and
 * stream; the matcher must outlive it.  orbx_initializer_destroy waits for that stream; after
 * the library's unload destructor it releases nothing. */
#define ORBX_INIT_MAX_ITERATIONS 4096
#define ORBX_INIT_STATUS_BAD_SET 1 /* status bit 0: a set had an index outside [0, N) or a repeated one */
#define ORBX_INIT_STATUS_TOO_FEW 2 /* status bit 1: N < 8 */
typedef struct orbx_initializer orbx_initializer;
int orbx_initializer_create(orbx_matcher* m, int max_batch, int kcap, int max_iterations, orbx_initializer** out);
void orbx_initializer_destroy(orbx_initializer* s);

typedef struct {
    int batch;
    int kcap;                    /* keypoint slots per row, <= the solver's kcap */
    const int32_t* n1;           /* [B] keypoints of the reference frame, clamped into [0, kcap] */
    const int32_t* n2;           /* [B] keypoints of the current frame */
    const orbx_keypoint* keys1;  /* [B][kcap] mvKeysUn of the reference frame; x and y are read */
    const orbx_keypoint* keys2;  /* [B][kcap] mvKeysUn of the current frame */
    const int32_t* matches12;    /* [B][kcap] vMatches12 as orbx_search_for_initialization leaves it */
    const float* K;              /* host: fx fy cx cy */
    float sigma;                 /* mSigma, 1.0 in Tracking */
    int max_iterations;          /* mMaxIterations, 200 in Tracking; <= the solver's */
    const int32_t* sets;         /* [B][max_iterations][8] */
} orbx_initializer_batch;

/* Every output is a nullable device array (host pointers to one pair's for
 * orbx_initializer_initialize).
 *   ok: Initialize's return value.  model: 0 = ReconstructH ran, 1 = ReconstructF.
 *   n_matches = N.  SH, SF, RH: the scores and their ratio.  best_it_H / best_it_F: the
 *   iteration that holds the best score, -1 if none.  H21 / F21: its matrix (scale and sign
 *   are as free as in the reference), all 0 if none.
 *   inliers_H / inliers_F: vbMatchesInliersH / F indexed by the frame-1 keypoint, 0 at
 *   unmatched slots below n1; n_inliers_H / F their counts.
 *   R21, t21: all 0 (the empty Mat) when ok is 0.  p3d, triangulated: vP3D and vbTriangulated
 *   of the winning hypothesis as CheckRT leaves them (zero point, flag 0 where it wrote
 *   nothing); all 0 below n1 when ok is 0.
 *   best_good, second_good: ReconstructH's bestGood and secondBestGood; for ReconstructF
 *   maxGood and the largest of the other three counts.  n_similar: ReconstructF's, 0 for H.
 *   parallax: the chosen hypothesis's (ReconstructH: bestParallax, -1 if no hypothesis has a
 *   good point; 0 where d1/d2 or d2/d3 fails, with both counts 0).
 *   status: the ORBX_INIT_STATUS_* bits.
 * Entries of the [B][kcap] arrays at and beyond n1 are left untouched. */
typedef struct {
    int32_t* ok;            /* [B] */
    int32_t* model;         /* [B] */
    int32_t* n_matches;     /* [B] */
    float* SH;              /* [B] */
    float* SF;              /* [B] */
    float* RH;              /* [B] */
    int32_t* best_it_H;     /* [B] */
    int32_t* best_it_F;     /* [B] */
    float* H21;             /* [B][9] */
    float* F21;             /* [B][9] */
    uint8_t* inliers_H;     /* [B][kcap] */
    uint8_t* inliers_F;     /* [B][kcap] */
    int32_t* n_inliers_H;   /* [B] */
    int32_t* n_inliers_F;   /* [B] */
    float* R21;             /* [B][9] */
    float* t21;             /* [B][3] */
    float* p3d;             /* [B][kcap][3] */
    uint8_t* triangulated;  /* [B][kcap] */
    int32_t* best_good;     /* [B] */
    int32_t* second_good;   /* [B] */
    int32_t* n_similar;     /* [B] */
    float* parallax;        /* [B] */
    int32_t* status;        /* [B] */
} orbx_initializer_result;

/* Asynchronous on `stream` (or the matcher's); the calls on one solver share its workspace,
 * so the caller keeps them in order.  ORBX_ERR_ARG, decided before any device call: a null
 * argument or required pointer, batch outside [0, max_batch], kcap outside [1, the solver's],
 * max_iterations outside [1, the solver's], sigma not positive. */
int orbx_initializer_initialize_device(orbx_initializer* s, const orbx_initializer_batch* in,
                                       const orbx_initializer_result* out, void* stream);

/* The single-pair host form: every pointer of the structs is a host pointer and batch is 1
 * (keys1 / matches12 hold *n1 entries, keys2 *n2, sets [max_iterations][8]; the per-keypoint
 * outputs hold *n1 entries).  One upload, the batch kernels with B = 1, one synchronisation;
 * the same bytes as the batch form gives that pair.  Its wall time is
 * orbx_matcher_last_call_us. */
int orbx_initializer_initialize(orbx_initializer* s, const orbx_initializer_batch* in,
                                const orbx_initializer_result* out);

/* The reference's mvSets for n correspondences (cc:103-123): sets [iterations][8], per
 * iteration 8 draws RandomInt(0, size - 1) = int(((double)rand() / ((double)RAND_MAX + 1.0))
 * * size) (DUtils/Random.cpp:47-49) without replacement, each removed by a swap with the back
 * and a pop.  n < 8 gives zeros.  One deviation: srand(0) is called on every call, where the
 * reference's SeedRandOnce(0) seeds once per process -- the first Initialize of a process is
 * reproduced, later ones restart the sequence.  Host only, no GPU. */
int orbx_initializer_sets(int32_t* sets, int n, int iterations);

/* ---- The covisibility graph: MapPoint observations, KeyFrame::UpdateConnections ----
 * A device-resident covisibility graph over keyframe ids 0 .. max_keyframes - 1 (DESIGN.md
 * §4.24).  The map it reads is the caller's, by device pointer: kf_mp [n_keyframes][cap] =
 * mvpMapPoints as MapPoint ids (-1 = NULL; an id outside [0, n_mappoints) counts as NULL),
 * kf_n [n_keyframes] the rows' lengths (clamped into [0, cap]), kf_bad [n_keyframes] /
 * mp_bad [n_mappoints] = isBad() or NULL.  The keyframe id stands in for the reference's
 * KeyFrame* wherever its order is a pointer order (std::map<KeyFrame*, ...>).  All integer
 * work: results are exact and do not depend on scheduling.
 *
 * orbx_covis_refresh_observations_device builds MapPoint::GetObservations() for every MapPoint
 * as a CSR: point p owns obs_off[p] .. obs_off[p + 1] of obs_kf / obs_idx, ascending keyframe
 * id.  Rows of bad keyframes contribute nothing (SetBadFlag erased their observations).  Where a
 * row names one MapPoint at several indices the lowest index holds the observation, the others
 * count as NULL in every later call (the cleaned copy of the table, `mp` of the view) and the
 * keyframe's status gets ORBX_COVIS_STATUS_DUPLICATE (rewritten by every refresh).  The graph
 * keeps kf_n, kf_bad and mp_bad and reads them in the later calls; it reads kf_mp only here, so
 * a change of the table takes effect with the next refresh.
 *
 * orbx_covis_update_connections_device is KeyFrame::UpdateConnections (KeyFrame.cc:324-415)
 * for the Q keyframes ids[0 .. Q) (a host array), with the result of calling it on ids[0],
 * ids[1], ... in order: the row mConnectedKeyFrameWeights (ascending id, entries below the
 * threshold of 15 included), mvpOrderedConnectedKeyFrames / mvOrderedWeights (weight descending,
 * id descending among equal weights; the entries >= 15, or pKFmax alone -- the lowest id among
 * the maxima -- when there is none), mbFirstConnection and mpParent (the list's front, set once,
 * never for id 0).  An empty counter leaves the keyframe untouched.  AddConnection
 * (cc:139-153) on the connected keyframes inserts or overwrites one entry of their rows and,
 * only when the entry is new or its weight differs, re-orders their whole row, entries below
 * 15 included (UpdateBestCovisibles, cc:160-182).  A bad keyframe among ids is skipped with
 * ORBX_COVIS_STATUS_BAD_KEYFRAME; a row of more than max_conn entries, the keyframe's own or
 * one that a message would grow, sets ORBX_COVIS_STATUS_CAPACITY and leaves that keyframe's
 * state untouched (all of a batch's messages to it are then dropped).  A repeated id is ORBX_ERR_ARG.  The status bits but DUPLICATE are sticky.
 *
 * orbx_covis_erase_keyframe_device is the connection part of SetBadFlag (cc:506-508, 519-520):
 * EraseConnection(id) on every keyframe of id's row, each re-ordered if it held the entry, then
 * id's row and list are cleared.  Id 0 is a no-op.  mbNotErase, the children's new parents and
 * EraseObservation stay with the caller, who sets kf_bad and refreshes the observations;
 * orbx_covis_set_bad_flag_device below is the whole of SetBadFlag.
 *
 * Rows in LDS: one workgroup counts a keyframe's connections in an LDS histogram while
 * max_keyframes <= ORBX_COVIS_LDS_KEYFRAMES (orbx_debug_set "covis_lds_keyframes" lowers the
 * bound for graphs created afterwards), in a global row above it; the results are the same.
 * ORBX_ERR_ARG, decided before any device call: a null graph or required pointer, a negative
 * size, max_conn > ORBX_COVIS_MAX_CONN, cap > 8192, an id outside the graph, a repeated id.
 * The calls are asynchronous on `stream` (or the graph's own); a call on another stream first
 * waits for the last one. */
typedef struct orbx_covis orbx_covis;
#define ORBX_COVIS_MAX_CONN 8192
#define ORBX_COVIS_LDS_KEYFRAMES 8192
#define ORBX_COVIS_STATUS_CAPACITY 1
#define ORBX_COVIS_STATUS_BAD_KEYFRAME 2
#define ORBX_COVIS_STATUS_DUPLICATE 4
int orbx_covis_create(int device, int max_keyframes, int cap, int max_mappoints, int max_conn, orbx_covis** out);
void orbx_covis_destroy(orbx_covis* g);
void* orbx_covis_stream(orbx_covis* g);
int orbx_covis_refresh_observations_device(orbx_covis* g, int n_keyframes, const int32_t* kf_mp, const int32_t* kf_n,
                                           const uint8_t* kf_bad, int n_mappoints, const uint8_t* mp_bad, void* stream);
/* The host form: the map as host arrays, copied into the graph's own buffer (which then serves
 * the later calls) on the graph's stream. */
int orbx_covis_refresh_observations(orbx_covis* g, int n_keyframes, const int32_t* kf_mp, const int32_t* kf_n,
                                    const uint8_t* kf_bad, int n_mappoints, const uint8_t* mp_bad);
int orbx_covis_update_connections_device(orbx_covis* g, const int32_t* ids, int Q, void* stream);
int orbx_covis_erase_keyframe_device(orbx_covis* g, int id, void* stream);

/* The graph's arrays by device pointer, for the caller's own kernels (valid until the graph is
 * destroyed; read them on the stream of the last call or after synchronising it). */
typedef struct {
    int max_keyframes, cap, max_mappoints, max_conn;
    int n_keyframes, n_mappoints;   /* of the last refresh */
    const int32_t* obs_off;         /* [n_mappoints + 1] */
    const int32_t* obs_kf;          /* [obs_off[n_mappoints]] */
    const int32_t* obs_idx;
    const int32_t* mp;              /* [max_keyframes][cap] the cleaned copy of kf_mp */
    const int32_t* row_kf;          /* [max_keyframes][max_conn] mConnectedKeyFrameWeights */
    const int32_t* row_w;
    const int32_t* row_n;           /* [max_keyframes] */
    const int32_t* ordered_kf;      /* [max_keyframes][max_conn] mvpOrderedConnectedKeyFrames */
    const int32_t* ordered_w;       /* mvOrderedWeights */
    const int32_t* ordered_n;       /* [max_keyframes] */
    const int32_t* parent;          /* [max_keyframes] mpParent, -1 = NULL */
    const uint8_t* first;           /* [max_keyframes] mbFirstConnection */
    const int32_t* status;          /* [max_keyframes] ORBX_COVIS_STATUS_* */
} orbx_covis_view;
int orbx_covis_view_device(orbx_covis* g, orbx_covis_view* view);
/* Host convenience: waits for the graph's last call and copies `bytes` bytes of one of the
 * view's arrays (from src, a device address) to the host. */
int orbx_covis_read(orbx_covis* g, const void* src, void* dst, size_t bytes);

/* GetBestCovisibilityKeyFrames(N) (cc:201-209) of every keyframe: out [max_keyframes][N] (-1
 * behind the list's end), out_n [max_keyframes]; device pointers. */
int orbx_covis_best_covisibles_device(orbx_covis* g, int N, int32_t* out, int32_t* out_n, void* stream);
/* GetCovisiblesByWeight(w) (cc:212-229) of every keyframe: a prefix of the ordered list, its
 * length in out_n [max_keyframes]; out [max_keyframes][max_conn] (-1 behind it) or NULL.  As
 * the reference: upper_bound on the descending weights, and the explicit empty result only
 * when the search reached the end and the last weight is below w. */
int orbx_covis_covisibles_by_weight_device(orbx_covis* g, int w, int32_t* out, int32_t* out_n, void* stream);
/* Host convenience: keyframe id's ordered list (what orbx_kfdb_set_covisibility takes): *n =
 * its length, the first min(*n, cap) entries to kf and, unless NULL, w.  Synchronises. */
int orbx_covis_ordered(orbx_covis* g, int id, int32_t* kf, int32_t* w, int cap, int* n);

/* ---- Optimizer::LocalBundleAdjustment's graph assembly and write-back on the device ----
 * orbx_local_ba_assemble_device runs Optimizer.cc:526-583 and the edge walk of cc:656-760 for
 * B current keyframes cur_kf[0 .. B) (a host array) on the covisibility graph `g`, whose
 * observations are those of the last refresh (refresh after kf_mp or a bad flag changed), and
 * writes the tables of orbx_local_ba_batch:
 *   keyframe rows of a problem: cur_kf, then its GetVectorCovisibleKeyFrames() in list order
 *   without the bad ones (lLocalKeyFrames), then lFixedCameras in the order of the walk (points
 *   in lLocalMapPoints order, each point's observers in ascending id); kf_fixed = 1 for the
 *   fixed cameras and for id 0, kf_slot = kf_id = the keyframe id, kf_Tcw from kf_pose;
 *   point rows: lLocalMapPoints in first-appearance order (the local keyframes in list order,
 *   each one's row in index order; NULL, bad and later copies of a duplicate skipped), pt_pos
 *   from mp_pos, pt_id the MapPoint id;
 *   observations: per point its observers in ascending id as (row within the problem's
 *   keyframe rows, keypoint index); obs_off is compact over the batch, obs_off[pt_off[B]] the
 *   total.
 * kf_off / pt_off [B + 1], counts [B][3] = {keyframe rows, point rows, observations} and status
 * [B] are written on the device.  max_kf_rows / max_pt_rows / max_obs are the tables' capacities
 * for the whole batch (obs_off holds max_pt_rows + 1): a problem that does not fit what the
 * problems before it left gets empty ranges, zero counts and ORBX_LOCAL_BA_STATUS_CAPACITY; the
 * others are laid out as if it were not there.  Nothing is read back: pass the capacities as
 * n_kf / n_pt / n_obs of orbx_local_bundle_adjustment_batch_device, which clamps against them.
 * Every pointer but cur_kf is a device pointer.  Asynchronous on `stream` (or the graph's). */
typedef struct {
    int batch;
    const int32_t* cur_kf;     /* host [B] */
    const float* kf_pose;      /* [max_keyframes][12] GetPose() rows 0..2, by keyframe id */
    const float* mp_pos;       /* [n_mappoints][3] GetWorldPos(), by MapPoint id */
    int max_kf_rows, max_pt_rows, max_obs;
    int32_t* kf_off;           /* [B + 1] out */
    float* kf_Tcw;             /* [max_kf_rows][12] out */
    uint8_t* kf_fixed;         /* [max_kf_rows] out */
    int32_t* kf_slot;          /* [max_kf_rows] out */
    int32_t* kf_id;            /* [max_kf_rows] out */
    int32_t* pt_off;           /* [B + 1] out */
    float* pt_pos;             /* [max_pt_rows][3] out */
    int32_t* pt_id;            /* [max_pt_rows] out */
    int32_t* obs_off;          /* [max_pt_rows + 1] out */
    int32_t* obs_kf;           /* [max_obs] out */
    int32_t* obs_kp;           /* [max_obs] out */
    int32_t* counts;           /* [B][3] out */
    int32_t* status;           /* [B] out */
} orbx_local_ba_assembly;
int orbx_local_ba_assemble_device(orbx_covis* g, const orbx_local_ba_assembly* a, void* stream);

/* The index part of Optimizer.cc:828-853 after orbx_local_bundle_adjustment_batch_device on the
 * assembled tables: kf_Tcw_opt of the keyframes that are not fixed goes to kf_pose through
 * kf_id, pt_pos_opt to mp_pos through pt_id, and for every erase[o] kf_mp[keyframe][keypoint]
 * = -1 (EraseMapPointMatch; erase or kf_mp NULL: skipped).  What EraseObservation does to a
 * point's nObs, reference keyframe and badness stays with the caller; UpdateNormalAndDepth is
 * orbx_update_normal_and_depth_device on the ids of pt_id, after a refresh of the observations.
 * Device pointers; asynchronous on `stream` (or the graph's). */
typedef struct {
    int batch;
    int max_kf_rows, max_pt_rows;   /* the tables' capacities, as assembled */
    const int32_t* kf_off;
    const int32_t* kf_id;
    const uint8_t* kf_fixed;
    const float* kf_Tcw_opt;
    const int32_t* pt_off;
    const int32_t* pt_id;
    const float* pt_pos_opt;
    const int32_t* obs_off;
    const int32_t* obs_kf;
    const int32_t* obs_kp;
    const uint8_t* erase;           /* [n_obs] or NULL */
    int n_keyframes, n_mappoints, cap;
    float* kf_pose;                 /* [n_keyframes][12] in/out */
    float* mp_pos;                  /* [n_mappoints][3] in/out */
    int32_t* kf_mp;                 /* [n_keyframes][cap] in/out or NULL */
} orbx_local_ba_apply;
int orbx_local_ba_apply_device(orbx_covis* g, const orbx_local_ba_apply* a, void* stream);

/* ---- Tracking::UpdateLocalMap and TrackLocalMap's tally on the device ----
 * orbx_update_local_map_device runs Tracking::UpdateLocalKeyFrames and UpdateLocalPoints
 * (Tracking.cc:1342-1500) for B frames on the covisibility graph `g`, whose observations are
 * those of the last refresh.  The keyframe id stands in for KeyFrame* wherever the reference
 * iterates a map or set of pointers.  For frame b, literally:
 *   votes (cc:1393-1408): for each index i < min(n[b], cap) of frame_mp[b], an id that is
 *   negative or outside [0, n_mappoints) counts as NULL, a bad MapPoint is written back as -1
 *   (cc:1405), every other entry adds one vote to each of its observers (a MapPoint at two
 *   indices votes twice);
 *   an empty counter (cc:1411) sets ORBX_LOCAL_MAP_STATUS_EMPTY and leaves local_kf[b],
 *   local_kf_n[b] (in/out; the count is clamped into [0, max_local_kf], ids outside the graph's
 *   keyframes contribute no points) and ref_kf[b] as they are on entry; UpdateLocalPoints still
 *   runs over that list;
 *   strategy 1 (cc:1423-1442): the voted keyframes in ascending id; pKFmax is the lowest id among
 *   the maxima.  The observation CSR holds no keyframe that was bad at the refresh, so the
 *   isBad() skip cannot fire through it; the test is kept because kf_bad is read when the call
 *   runs and may have changed since;
 *   strategy 2 (cc:1445-1493) over the strategy-1 entries only, in order, stopping once the list
 *   holds more than 80: the first of the entry's best 10 ordered neighbours that is neither bad
 *   nor local, then its first child in ascending id that is neither, then its parent, which is
 *   not tested for badness -- a parent that was not yet local is appended and ends the whole
 *   walk (the reference's break leaves the outer loop).  The children of k are the keyframes c
 *   that are not bad and have parent[c] == k; `parent` is the graph's own array unless the
 *   caller passes one (orbx_covis_set_bad_flag_device and orbx_keyframe_culling_device keep the
 *   graph's own array right through a cull; after a loop closure the caller owns the tree);
 *   ref_kf[b] = pKFmax when there is one;
 *   UpdateLocalPoints (cc:1354-1380): the local keyframes in list order, each row of the graph's
 *   cleaned table in index order (whether or not the keyframe is bad now), the first appearance
 *   of every MapPoint that is not bad.
 * Everything is written on the device and nothing is read back: local_kf [B][max_local_kf] with
 * local_kf_n [B], ref_kf [B], local_off [B + 1] (compact over the batch), local_ids [max_total],
 * counts [B][2] = {local keyframes, local points} and status [B].  A frame whose list exceeds
 * max_local_kf, whose points exceed max_local_points, or whose points do not fit what the
 * frames before it left of max_total gets ORBX_LOCAL_MAP_STATUS_CAPACITY, local_kf_n = 0, an
 * empty range, zero counts, and ref_kf and frame_mp as if untouched (its row of local_kf is
 * unspecified); every other frame is laid out as if that frame were not there.  This is a
 * deviation outside the reference.  Entries of local_kf behind local_kf_n are unspecified.
 * ORBX_ERR_ARG, decided before any device call: a null required pointer, a negative size, cap
 * different from the graph's, a call before any refresh.  Every pointer is a device pointer.
 * Asynchronous on `stream` (or the graph's). */
#define ORBX_LOCAL_MAP_STATUS_CAPACITY 1
#define ORBX_LOCAL_MAP_STATUS_EMPTY 2
typedef struct {
    int batch;
    int cap;                   /* row length of frame_mp: the graph's cap */
    int32_t* frame_mp;         /* [B][cap] mCurrentFrame.mvpMapPoints as ids, in/out */
    const int32_t* n;          /* [B] mCurrentFrame.N */
    const int32_t* parent;     /* [max_keyframes] mpParent, -1 = NULL; NULL: the graph's */
    int max_local_kf, max_local_points, max_total;
    int32_t* local_kf;         /* [B][max_local_kf] mvpLocalKeyFrames, in/out */
    int32_t* local_kf_n;       /* [B] in/out */
    int32_t* ref_kf;           /* [B] mpReferenceKF, in/out */
    int32_t* local_off;        /* [B + 1] out */
    int32_t* local_ids;        /* [max_total] mvpLocalMapPoints, frame after frame, out */
    int32_t* counts;           /* [B][2] out */
    int32_t* status;           /* [B] out */
} orbx_local_map_update;
int orbx_update_local_map_device(orbx_covis* g, const orbx_local_map_update* u, void* stream);
/* The host form: every array of `u` on the host, staged through the graph's own buffer on the
 * graph's stream; synchronises. */
int orbx_update_local_map(orbx_covis* g, const orbx_local_map_update* u);

/* orbx_search_local_points_device with local_off as a device array, taken as written by
 * orbx_update_local_map_device: lm->local_off is ignored, the scratch is sized by max_total and
 * the launch by max_local_points, and each frame's range is clamped into both bounds, so that a
 * wrong offset is never read or written past them.  Nothing is read back. */
int orbx_search_local_points_offsets_device(orbx_matcher* m, const orbx_mappoints_device* mps,
                                            const orbx_local_map_batch* lm, const int32_t* d_local_off,
                                            int max_local_points, int max_total, void* stream);

/* TrackLocalMap's tally after the second PoseOptimization (Tracking.cc:1047-1081) for B frames:
 * matches_inliers[b] counts the entries i < min(n[b], cap) of frame_mp[b] that are not NULL (an id
 * outside [0, n_mappoints) counts as NULL), not outliers and, unless only_tracking, have
 * observations > 0; each entry that is not an outlier adds one to mp_found[id] (IncreaseFound(),
 * an integer atomicAdd whose sum does not depend on order; NULL: skipped); with `stereo` an
 * outlier's entry becomes -1; ok[b] = 0 when matches_inliers[b] < 30, or < 50 with
 * recently_relocalised[b] (NULL: no frame), else 1.  IncreaseVisible is done by the search.
 * Device pointers; runs on the graph's device, asynchronous on `stream` (or the graph's). */
typedef struct {
    int batch, cap;
    int32_t* frame_mp;                    /* [B][cap] in/out */
    const int32_t* n;                     /* [B] */
    const uint8_t* outlier;               /* [B][cap] mvbOutlier */
    int n_mappoints;
    const int32_t* observations;          /* [n_mappoints] Observations() */
    int only_tracking, stereo;
    const uint8_t* recently_relocalised;  /* [B] mnId < mnLastRelocFrameId + mMaxFrames, or NULL */
    int32_t* mp_found;                    /* [n_mappoints] mnFound, in/out, or NULL */
    int32_t* matches_inliers;             /* [B] out */
    uint8_t* ok;                          /* [B] out */
} orbx_track_local_map_tally;
int orbx_track_local_map_tally_device(orbx_covis* g, const orbx_track_local_map_tally* t, void* stream);

/* ---- LocalMapping::KeyFrameCulling, MapPointCulling and the full KeyFrame::SetBadFlag (§4.26) ----
 * The map tables that the culls read and change, by device pointer.  kf_mp, kf_bad and mp_bad
 * are the arrays of the graph's last orbx_covis_refresh_observations_device (the host form keeps
 * a copy of its own: ORBX_ERR_ARG); the other tables are [n_keyframes][cap] beside kf_mp.  Every
 * call below reads the graph's cleaned table, so a MapPoint named at two indices of a row counts
 * once (a deviation: the reference's mvpMapPoints would count it twice in nMPs), and ends by
 * running the observation refresh's launches on the mutated kf_mp: the observation CSR and the
 * cleaned table the graph holds afterwards are those of a fresh refresh.
 *
 * orbx_keyframe_culling_device is LocalMapping::KeyFrameCulling (LocalMapping.cc:708-775) for the
 * current keyframe cur_kf.  The candidates are its GetVectorCovisibleKeyFrames(), taken once in
 * list order (cand, n_cand); id 0 is skipped (cc:718), and so is a keyframe that is bad already
 * (outside the reference, whose lists hold none).  For each index of a candidate's cleaned row:
 * NULL and bad MapPoints are skipped, unless monocular so is mvDepth > mThDepth || mvDepth < 0,
 * every other entry counts into nMPs, and into nRedundantObservations when Observations() > 3
 * (MapPoint.cc:134-146: an observation with mvuRight >= 0 counts 2) and at least 3 other
 * observers have mvKeysUn[idx].octave <= scaleLevel + 1.  The candidate is culled when
 * (double)nRedundantObservations > 0.9 * (double)nMPs.  SetBadFlag runs inside the loop, so later
 * candidates are counted on the state it left.  cand_counts [max_conn][3] = {nMPs,
 * nRedundantObservations, 0 | 1 culled | 2 only marked mbToBeErased}; culled [max_conn] in cull
 * order, n_culled; n_new_bad_mp the MapPoints that went bad; status ORBX_CULL_STATUS_*.  One
 * current keyframe per call: several calls on one graph at a time would race on the state that
 * the reference serialises.
 *
 * orbx_covis_set_bad_flag_device is KeyFrame::SetBadFlag (KeyFrame.cc:492-598) on ids[0], ids[1],
 * ... (a host array) in order, which is also what KeyFrame::SetErase (cc:476-489) runs once the
 * caller cleared mbNotErase.  Id 0 returns (cc:497); kf_not_erase sets only kf_to_be_erased
 * (cc:500-503); a keyframe that is bad already is left alone.  EraseConnection(this) on every
 * keyframe of the row, each re-ordered, entries below 15 included, if it held the entry
 * (cc:506-508, 607-620); EraseObservation(this) on every entry (cc:510-512, MapPoint.cc:152-180):
 * when a MapPoint's nObs falls to <= 2 its own SetBadFlag runs (MapPoint.cc:195-212): mp_bad is
 * set and its entry becomes -1 in every remaining observer, in kf_mp and in the graph's cleaned
 * table; the culled keyframe's own row keeps its entries.  The row and list are cleared
 * (cc:519-520).  The children (the keyframes that are not bad and have parent == id; not id's
 * own parent, a cycle that the reference's tree cannot hold) get new
 * parents (cc:522-584): sParentCandidates = {mpParent}; while children remain, the largest
 * GetWeight over (child in ascending id) x (position in that child's ordered list) whose keyframe
 * is a candidate -- strict >, the first in that order wins a tie --; that child's parent changes,
 * it becomes a candidate; when a round finds nothing every remaining child gets mpParent.  The
 * graph's own `parent` array is changed.  A culled keyframe whose parent is -1 is outside the
 * reference (it dereferences NULL): children that find no candidate get -1 and status gets
 * ORBX_CULL_STATUS_NO_PARENT.  kf_bad[id] = 1 (cc:592).  mTcp, Map::EraseKeyFrame and
 * KeyFrameDatabase::erase stay with the caller.
 *
 * orbx_map_point_culling_device is LocalMapping::MapPointCulling (LocalMapping.cc:185-220) over
 * recent[0 .. *n_recent) (mlpRecentAddedMapPoints; distinct ids), in order: a bad point (or an id
 * outside the map) is dropped; GetFoundRatio() = (float)mp_found / (float)mp_visible < 0.25f (one
 * correctly rounded float division; 0 / 0 does not compare less) -> SetBadFlag and drop;
 * (int)cur_kf_id - mp_first_kf >= 2 && Observations() <= cnThObs (2 monocular, else 3) ->
 * SetBadFlag and drop; a difference >= 3 -> drop; else kept.  The kept entries are compacted in
 * order, *n_recent is rewritten, *n_culled counts the SetBadFlags.
 *
 * orbx_covis_observation_counts_device writes Observations() of every MapPoint from the
 * observation CSR (0 for a bad one): what orbx_track_local_map_tally.observations takes.
 *
 * ORBX_ERR_ARG, decided before any device call: a null graph or required pointer, a negative
 * max_recent, a call before any refresh, kf_bad / mp_bad that are not the arrays the graph kept,
 * a graph last refreshed through the host form, an id outside the graph, a repeated id.  All
 * pointers are device pointers unless noted; nothing is read back; asynchronous on `stream` (or
 * the graph's own).  orbx_debug_set "cull_serial": the walk counts every candidate itself. */
#define ORBX_CULL_STATUS_NO_PARENT 1
typedef struct {
    int32_t* kf_mp;                /* [n_keyframes][cap], in/out: the table of the last refresh */
    uint8_t* kf_bad;               /* [n_keyframes] in/out; must be the array of the last refresh */
    uint8_t* mp_bad;               /* [n_mappoints] in/out; likewise */
    const orbx_keypoint* kf_keys_un; /* [n_keyframes][cap]: .octave is read (KeyFrameCulling only) */
    const float* kf_u_right;       /* [n_keyframes][cap] mvuRight, NULL: every observation counts 1 */
    const float* kf_depth;         /* [n_keyframes][cap] mvDepth; required unless monocular */
    const float* kf_th_depth;      /* [n_keyframes] mThDepth; required unless monocular */
    const uint8_t* kf_not_erase;   /* [n_keyframes] mbNotErase or NULL */
    uint8_t* kf_to_be_erased;      /* [n_keyframes] mbToBeErased, in/out, or NULL */
} orbx_map_tables;
int orbx_keyframe_culling_device(orbx_covis* g, const orbx_map_tables* m, int cur_kf, int monocular,
                                 int32_t* cand, int32_t* cand_counts, int32_t* n_cand, int32_t* culled,
                                 int32_t* n_culled, int32_t* n_new_bad_mp, int32_t* status, void* stream);
int orbx_covis_set_bad_flag_device(orbx_covis* g, const orbx_map_tables* m, const int32_t* ids /* host */, int Q,
                                   int32_t* n_new_bad_mp, int32_t* status, void* stream);
int orbx_map_point_culling_device(orbx_covis* g, const orbx_map_tables* m, int cur_kf_id, int monocular,
                                  int32_t* recent, int32_t* n_recent, int max_recent, const int32_t* mp_first_kf,
                                  const int32_t* mp_found, const int32_t* mp_visible, int32_t* n_culled, void* stream);
int orbx_covis_observation_counts_device(orbx_covis* g, const float* kf_u_right, int32_t* out, void* stream);

/* ---- MapPoint::UpdateNormalAndDepth in its general form, on the observation CSR (§4.27) ----
 * MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:386-439) for the MapPoints ids[0 .. n_ids) (a
 * device array), or for every MapPoint of the last refresh when ids is NULL: the call that
 * LoopClosing::CorrectLoop (LoopClosing.cc:554), Optimizer::OptimizeEssentialGraph
 * (Optimizer.cc:1148), the write-back of LocalBundleAdjustment (cc:828-853) and that of
 * Optimizer::BundleAdjustment when nLoopKF == 0 (cc:273) end with.  Per point, on the observers that the graph's observation CSR holds (the
 * keyframes that are not bad), in ascending keyframe id:
 *   normal = the mean of (P - Ow_i) / |P - Ow_i|, Ow_i = -R^T t of kf_Tcw[i];
 *   dist = |P - Ow_ref|, ref = mp_ref_kf[p] (mpRefKF is the caller's);
 *   level = kf_keys_un[ref][index of ref among the point's observations].octave, clamped into
 *   [0, nlevels); max_distance = dist * scale_factors[level]; min_distance = max_distance /
 *   scale_factors[nlevels - 1].
 * A bad point and a point without observations are left untouched (cc:393, 400).  If ref is not
 * among the observers the reference's observations[pRefKF] inserts index 0: index 0 is read and
 * *status gets ORBX_NORMAL_STATUS_REF_NOT_OBSERVER.  An id outside the MapPoints of the last
 * refresh, or a ref outside its keyframes, leaves the point untouched and sets
 * ORBX_NORMAL_STATUS_BAD_INDEX.  Float inputs are widened to double, everything after is double
 * (one sum per point, in observer order: no floating-point atomics), the outputs are rounded to
 * float once.  The reference's own arithmetic is float with cv::norm's double accumulation; the
 * difference is within the tolerance that tests/correct_loop_spread.py measures.
 * ORBX_ERR_ARG, decided before any device call: a null graph, struct, table or status, a
 * negative n_ids, nlevels outside 1..32, a call before any refresh.  scale_factors is a host
 * array; every other pointer is a device pointer; status is one int32 that the call rewrites.
 * Nothing is read back; asynchronous on `stream` (or the graph's own). */
#define ORBX_NORMAL_STATUS_REF_NOT_OBSERVER 1
#define ORBX_NORMAL_STATUS_BAD_INDEX 2
typedef struct {
    const float* kf_Tcw;              /* [n_keyframes][12] rows 0..2 of GetPose() */
    const orbx_keypoint* kf_keys_un;  /* [n_keyframes][cap]: .octave is read */
    const int32_t* mp_ref_kf;         /* [n_mappoints] mpRefKF->mnId */
    const float* mp_pos;              /* [n_mappoints][3] GetWorldPos() */
    const float* scale_factors;       /* host: mvScaleFactors (nlevels) */
    int nlevels;
    float* normal;                    /* [n_mappoints][3] mNormalVector, in/out */
    float* max_distance;              /* [n_mappoints] mfMaxDistance, in/out */
    float* min_distance;              /* [n_mappoints] mfMinDistance, in/out */
} orbx_normal_depth;
int orbx_update_normal_and_depth_device(orbx_covis* g, const orbx_normal_depth* a, const int32_t* ids, int n_ids,
                                        int32_t* status, void* stream);

/* ---- LoopClosing::CorrectLoop: Sim3 propagation and the essential graph's assembly (§4.27) ----
 * The two calls between orbx_optimize_sim3_batch_device and
 * orbx_optimize_essential_graph_batch_device, on the graph and the map tables in HBM.  The
 * keyframe id stands in for KeyFrame* wherever the reference iterates a map or set of pointers
 * (§4.24).  Between the two calls the caller runs its fusion (SearchAndFuse, MapPoint::Replace:
 * LoopClosing.cc:574-593) on kf_mp and refreshes the observations.  AddLoopEdge (cc:626-627), the
 * propagation after the global bundle adjustment (cc:745-805) and DetectLoop's consistency groups
 * stay with the caller.
 *
 * orbx_correct_loop_propagate_device is LoopClosing.cc:482-571 for mpCurrentKF = cur_kf:
 *   a. UpdateConnections(cur_kf) (cc:482); conn = GetVectorCovisibleKeyFrames(cur_kf) in list
 *      order without the keyframes that are bad (outside the reference, whose lists hold none) or
 *      beyond the last refresh, then cur_kf (cc:488-489): conn[0 .. *n_conn).
 *   b. mg2oScw is Scw (8 doubles: q xyzw, t, s), or, when Scw is NULL, Sim3(sim3_R, sim3_t,
 *      sim3_s) * Sim3(Rmw, tmw, 1) of kf_Tcw[matched_kf] (cc:359-362; the layout of
 *      orbx_optimize_sim3_batch.R12_opt / t12_opt / s12_opt of one candidate).  Per member i =
 *      conn[j]: kf_Tcw_nc[j] = the bytes of kf_Tcw[i] (NonCorrectedSim3 = Sim3(Riw, tiw, 1));
 *      corr_S[j] = CorrectedSim3 = Sim3(Ric, tic, 1) * Scw with Tic = Tiw * Twc formed in double
 *      (the reference: a float cv::Mat product), Scw itself for cur_kf; kf_corr[i] = j, -1 for
 *      every other keyframe of the graph.  These are orbx_essential_graph_batch's corr_S and the
 *      source of its kf_corr.
 *   c. cc:526-555 over the graph's cleaned rows.  The reference walks CorrectedSim3 in key order
 *      and mnCorrectedByKF lets the first member that holds a point correct it: here the owner of
 *      a point is the smallest member id among its observers (the observation CSR), and only the
 *      thread of (owner, point) acts.  NULL entries, bad points and points whose input
 *      mp_corrected_by_kf is cur_kf are skipped.  The owner writes mp_pos =
 *      CorrectedSwi.map(Siw.map(P)) (rounded to float), mp_corrected_by_kf = cur_kf,
 *      mp_corrected_ref = owner, and runs UpdateNormalAndDepth (above) on the state the reference
 *      has at that moment: an observer that is a member with a smaller id than the owner has its
 *      corrected pose already (SetPose runs after a member's points, cc:566), every other
 *      observer its input pose.
 *   d. kf_Tcw[i] = [R | t / s] of corr_S (cc:558-566), after all points; UpdateConnections of
 *      every member (cc:570) as one batch.
 * status (one int32, rewritten) gets the ORBX_NORMAL_STATUS_* bits of (c).
 *
 * orbx_essential_graph_assemble_device runs after the caller's fusion and refresh: it takes the
 * first call's conn, n_conn, kf_corr and kf_Tcw_nc and writes the tables that
 * orbx_essential_graph_batch takes for one problem.
 *   1. LoopConnections (cc:595-618).  The reference walks the members in list order and takes
 *      vpPreviousNeighbors = GetVectorCovisibleKeyFrames() of member i inside that loop, just
 *      before UpdateConnections(i): LoopConnections[i] = (the keys of i's row afterwards) -
 *      vpPreviousNeighbors - members.  Here each member's ordered list AND row are snapshot at
 *      entry, then UpdateConnections runs on the members as one batch.  vpPreviousNeighbors of
 *      member i is its ordered list at entry, unless the UpdateConnections of a member before it
 *      in conn added or changed its entry in i's row (AddConnection, KeyFrame.cc:139-153: its
 *      new weight w is >= 15 or i is its pKFmax, and w differs from the entry i's row held at
 *      entry): UpdateBestCovisibles (cc:160-182) then re-ordered i's whole row, entries below 15
 *      included, and vpPreviousNeighbors is every key of i's row at entry.  (Members that such
 *      updates add are removed anyway.)  This gives the sets of the sequential walk
 *      (tests/test_correct_loop_model.py).  Output: members in ascending id, each set in
 *      ascending id, as the CSR lc_off[*n_conn + 1], lc_kf, lc_w (GetWeight after all updates),
 *      lc_member.  conn, n_conn, kf_corr and kf_Tcw_nc must be the output of
 *      orbx_correct_loop_propagate_device on this graph: the kernels index the graph's rows with
 *      conn and only clamp the count.
 *   2. Vertices: the keyframes of the last refresh that are not bad, ascending id: kf_ids[row],
 *      kf_row[id] (-1 for a bad one; [max_keyframes]), *n_rows, *loop_row = kf_row[loop_kf],
 *      kf_corr_rows[row] = kf_corr[id], kf_Tcw_rows[row] = kf_Tcw_nc of a member, the current
 *      kf_Tcw otherwise.
 *   3. Edges in the order of the Python package's essential_graph_edges: every kind-0 edge of
 *      cc:954-986 over the LoopConnections CSR (the cur_kf - loop_kf pair is admitted below
 *      min_feat), then per keyframe in ascending id its kind-1 edges (cc:989-1089): the parent
 *      (the graph's `parent`), its loop edges to smaller ids (loop_off / loop_kf_ids: GetLoopEdges()
 *      as a CSR over keyframe ids, ascending within a row), and the prefix of its ordered list
 *      with weight >= min_feat without the parent, its children (the good keyframes whose parent
 *      it is, §4.26), its loop edges, bad keyframes, ids not below its own and pairs inserted as
 *      kind 0.  An edge to a keyframe without a row is dropped and sets BAD_KEYFRAME.  edge_v
 *      holds rows; edge_off = {0, *n_edges}.  More edges than max_edges (or more LoopConnections
 *      than max_lc): ORBX_ASSEMBLY_STATUS_CAPACITY, *n_edges (lc_off[*n_conn]) holds the need,
 *      nothing is written past the capacity, and the edges are not written at all when the
 *      LoopConnections did not fit.
 *   4. pt_ref (cc:1125-1133) of every MapPoint of the last refresh: kf_row[mp_corrected_ref[p]]
 *      where mp_corrected_by_kf[p] == cur_kf, else kf_row[mp_ref_kf[p]]; -1 for a bad point or a
 *      reference outside the keyframes.  The optimiser leaves a point with pt_ref = -1 its input
 *      bytes and reports ORBX_ESSENTIAL_GRAPH_STATUS_BAD_INDEX.  pt_off = {0, n_mappoints}.
 *   5. *env_blocks = what orbx_essential_graph_envelope gives for these rows, loop_row and edges.
 * The first assembly on a graph allocates its workspace: 3 (max_conn + 1) max_conn ints for the
 * members' lists and rows at entry, and a few arrays of max_keyframes ints.
 *
 * ORBX_ERR_ARG, decided before any device call: a null graph, struct or required pointer, cur_kf
 * / matched_kf / loop_kf outside the keyframes of the last refresh, a negative max_edges or
 * max_lc, nlevels outside 1..32, a call before any refresh.  scale_factors is a host array;
 * every other pointer is a device pointer.  Nothing is read back; no floating-point atomics; no
 * workgroup waits on another; asynchronous on `stream` (or the graph's own). */
typedef struct {
    int cur_kf;
    const double* Scw;             /* [8] mg2oScw, or NULL: composed from the four below */
    const float* sim3_R;           /* [9] OptimizeSim3's R12_opt of the accepted candidate */
    const float* sim3_t;           /* [3] t12_opt */
    const float* sim3_s;           /* [1] s12_opt */
    int matched_kf;                /* mpMatchedKF */
    float* kf_Tcw;                 /* [n_keyframes][12] in/out */
    float* mp_pos;                 /* [n_mappoints][3] in/out */
    int32_t* mp_corrected_by_kf;   /* [n_mappoints] mnCorrectedByKF, in/out */
    int32_t* mp_corrected_ref;     /* [n_mappoints] mnCorrectedReference, in/out */
    const int32_t* mp_ref_kf;      /* [n_mappoints] */
    const orbx_keypoint* kf_keys_un; /* [n_keyframes][cap] */
    const float* scale_factors;    /* host (nlevels) */
    int nlevels;
    float* normal;                 /* [n_mappoints][3] in/out */
    float* max_distance;           /* [n_mappoints] in/out */
    float* min_distance;           /* [n_mappoints] in/out */
    int32_t* conn;                 /* [max_conn + 1] out */
    int32_t* n_conn;               /* [1] out */
    double* corr_S;                /* [max_conn + 1][8] out */
    int32_t* kf_corr;              /* [max_keyframes] out */
    float* kf_Tcw_nc;              /* [max_conn + 1][12] out */
    int32_t* status;               /* [1] out */
} orbx_correct_loop_propagate;
int orbx_correct_loop_propagate_device(orbx_covis* g, const orbx_correct_loop_propagate* a, void* stream);

#define ORBX_ASSEMBLY_STATUS_CAPACITY 1
#define ORBX_ASSEMBLY_STATUS_BAD_KEYFRAME 2
typedef struct {
    int cur_kf, loop_kf, min_feat; /* min_feat: 100 (Optimizer.cc:908) */
    const int32_t* conn;           /* [max_conn + 1] of the propagation */
    const int32_t* n_conn;         /* [1] */
    const int32_t* kf_corr;        /* [max_keyframes] */
    const float* kf_Tcw_nc;        /* [max_conn + 1][12] */
    const float* kf_Tcw;           /* [n_keyframes][12] the current poses */
    const int32_t* loop_off;       /* [n_keyframes + 1] GetLoopEdges() as a CSR */
    const int32_t* loop_kf_ids;    /* [loop_off[n_keyframes]] ascending within a row */
    const int32_t* mp_corrected_by_kf; /* [n_mappoints] */
    const int32_t* mp_corrected_ref;   /* [n_mappoints] */
    const int32_t* mp_ref_kf;      /* [n_mappoints] */
    int max_lc, max_edges;
    int32_t* lc_off;               /* [max_conn + 2] out */
    int32_t* lc_member;            /* [max_conn + 1] out: the members, ascending id */
    int32_t* lc_kf;                /* [max_lc] out */
    int32_t* lc_w;                 /* [max_lc] out */
    int32_t* kf_ids;               /* [n_keyframes] out */
    int32_t* kf_row;               /* [max_keyframes] out */
    int32_t* n_rows;               /* [1] out */
    int32_t* kf_off;               /* [2] out: {0, *n_rows} */
    int32_t* loop_row;             /* [1] out */
    int32_t* kf_corr_rows;         /* [n_keyframes] out */
    float* kf_Tcw_rows;            /* [n_keyframes][12] out */
    int32_t* edge_v;               /* [max_edges][2] out */
    int32_t* edge_kind;            /* [max_edges] out */
    int32_t* n_edges;              /* [1] out */
    int32_t* edge_off;             /* [2] out: {0, min(*n_edges, max_edges)} */
    int32_t* pt_ref;               /* [n_mappoints] out */
    int32_t* pt_off;               /* [2] out: {0, n_mappoints} */
    int64_t* env_blocks;           /* [1] out */
    int32_t* status;               /* [1] out: ORBX_ASSEMBLY_STATUS_* */
} orbx_essential_graph_assembly;
int orbx_essential_graph_assemble_device(orbx_covis* g, const orbx_essential_graph_assembly* a, void* stream);

/* Alternative kernel forms and diagnostics switches, process-wide (tests and A/B tools;
 * the product reads no environment).  Names: "pz_seg" (pyramid levels per launch, 0 = one
 * launch), "pz_byte" (byte-read k_pyramid), "desc_tiles" (tile-major describe),
 * "extract_dma" (single host call through DMA copies), "replay_threads" (64..1024),
 * "dup_stage" (launch extraction stage k twice), "oct_stamps" / "call_stamps" /
 * "match_stamps" (phase stamps to stderr), "covis_lds_keyframes" (the covisibility graph's LDS
 * bound, read by orbx_covis_create), "cull_serial" (orbx_keyframe_culling_device without the
 * speculative pass), "essgraph_stamps" (orbx_optimize_essential_graph*:
 * problem 0's wall-clock ticks in the linearisations and in the linear solves to stderr;
 * synchronises the stream).  value < 0 restores the default; name NULL
 * restores every default.  Every form gives the same results.  A frame size's plan reads
 * pz_seg / pz_byte / desc_tiles when an extractor first plans it. */
int orbx_debug_set(const char* name, int value);

/* Library / device info. */
const char* orbx_version(void);
int orbx_device_count(int* n);
const char* orbx_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_H */
