/*
 * orbgpu.h -- C ABI of the MI355X-native ORB-SLAM3 front-end / local-BA hot path (liborbgpu.so).
 *
 * Plain pointers, sizes and int status codes only (no OpenCV, Eigen, torch or C++ types), so the
 * reference's C++ (through include/orbgpu_cv.hpp) or any FFI can bind it.
 * Each entry point names the reference interface it replaces (file:line in the reference tree).
 *
 * Threading (reference semantics): calls on DIFFERENT handles may run
 * concurrently from different threads; a single handle is not thread-safe (like one
 * ORB_SLAM3::ORBextractor object, whose mvImagePyramid is per-object state).
 */
#ifndef ORBGPU_H
#define ORBGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------------------------- */
#define ORB_OK 0
#define ORB_ERR_EMPTY (-1)     /* empty image: ORBextractor::operator() returns -1 (src/ORBextractor.cc:1561-1562) */
#define ORB_ERR_ARG (-2)       /* invalid argument (null pointer, size beyond the handle's capacity, ...) */
#define ORB_ERR_CAPACITY (-3)  /* caller's output capacity too small; the needed count is still reported */
#define ORB_ERR_DEVICE (-4)    /* HIP runtime error (no GPU, launch failure, out of memory) */
#define ORB_ERR_ABORTED (-5)   /* stopped through the caller's stop flag (LocalBA pbStopFlag) */
#define ORB_ERR_INTERNAL (-6)  /* a device-side capacity guard tripped (should not happen) */

/* cv::KeyPoint memory layout (28 bytes): pt.x, pt.y, size, angle, response, octave, class_id */
typedef struct orb_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orb_keypoint_t;

/* ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
 * (include/ORBextractor.h:52-53; values from the YAML keys ORBextractor.* e.g.
 * Examples/Monocular/EuRoC.yaml:50-56) */
typedef struct orb_params {
    int32_t nfeatures;
    float scale_factor;
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
} orb_params_t;

typedef struct orb_extractor_s* orb_extractor_t;

/* Query the library: returns the number of visible HIP devices (0 = none), never fails. */
int orb_device_count(void);
/* Human readable message for the last error on this thread. */
const char* orb_last_error(void);

/* ---- ORBextractor (src/ORBextractor.cc) ------------------------------------------------------ */

/* Create an extractor for frames up to max_width x max_height, batches up to max_batch frames.
 * Replaces ORBextractor::ORBextractor (src/ORBextractor.cc:468-571).  Allocates all device
 * buffers once; no allocation happens per call. */
int orb_extractor_create(const orb_params_t* params, int max_width, int max_height, int max_batch,
                         orb_extractor_t* out);
int orb_extractor_destroy(orb_extractor_t h);

/* GetLevels/GetScaleFactors/GetInverseScaleFactors/GetScaleSigmaSquares/GetInverseScaleSigmaSquares
 * (include/ORBextractor.h:61-83) and the per-level feature budget mnFeaturesPerLevel.
 * Each array receives nlevels values; any pointer may be NULL. */
int orb_extractor_scales(orb_extractor_t h, float* scale, float* inv_scale, float* sigma2,
                         float* inv_sigma2, int32_t* features_per_level);

/* ORBextractor::operator()(image, mask, keypoints, descriptors, vLappingArea)
 * (src/ORBextractor.cc:1557-1682; called from Frame::ExtractORB src/Frame.cc:513-523).
 * Host buffers, synchronous.  image: 8-bit gray, row stride `stride` bytes.  kps/desc hold `cap`
 * entries (desc: cap x 32 bytes).  Keypoints are placed as the reference does: those with
 * lap_x0 <= x <= lap_x1 (level-0 coordinates) from the end backwards, the others from the front.
 * Returns monoIndex (>= 0, the number of front-placed keypoints), ORB_ERR_EMPTY for an empty
 * image, or another negative status.  *n_kps receives the keypoint count (also when the capacity
 * is too small). */
int orb_extract(orb_extractor_t h, const uint8_t* image, int width, int height, int stride,
                int lap_x0, int lap_x1, orb_keypoint_t* kps, uint8_t* desc, int cap, int* n_kps);

/* Batched, device-resident, asynchronous form (the throughput path; no reference counterpart --
 * it runs operator() on n frames at once).  d_images: n frames, frame f at d_images + f*frame_stride,
 * rows `stride` bytes apart.  Frame f writes d_kps[f*cap ...], d_desc[(f*cap ...)*32] and
 * d_counts[2f] = number of keypoints, d_counts[2f+1] = monoIndex (or ORB_ERR_CAPACITY if the frame
 * had more than cap keypoints; then d_counts[2f] still holds the count).  stream: hipStream_t
 * (NULL = default stream).  Returns after enqueueing.  The outputs (and d_images) may also be pinned,
 * device-mapped host memory (hipHostMalloc): the kernels then read / write it over the link, which is
 * how a host-input pipeline skips the download copy. */
int orb_extract_batch_device(orb_extractor_t h, const uint8_t* d_images, int n, int width, int height,
                             int stride, size_t frame_stride, int lap_x0, int lap_x1,
                             orb_keypoint_t* d_kps, uint8_t* d_desc, int cap, int32_t* d_counts,
                             void* stream);

/* Scheduling of a batch on the device path (no reference counterpart).  mode 1 (the default): the
 * early levels' FAST, quad-tree and descriptors run on the handle's side streams beside the small
 * pyramid levels -- the shortest time for one batch alone.  mode 0: a batch runs as one chain on the
 * caller's stream -- the higher throughput when several handles keep batches in flight on their own
 * streams (their side streams would share the process's hardware queues).  Results are identical;
 * takes effect at the next call. */
int orb_extractor_set_overlap(orb_extractor_t h, int mode);

/* mvImagePyramid[level] of frame `frame` of the last call (include/ORBextractor.h:83; read by
 * Frame::ComputeStereoMatches src/Frame.cc:1126,1249).  Gives the device address of the view
 * (first pixel of the level image inside its padded plane), its size and row pitch.  On the device
 * only a 3-pixel REFLECT_101 border around the view is written (all that the stereo matcher's SAD
 * windows and the descriptor's blur reach); the plane extends 19 pixels each way. */
int orb_extractor_level(orb_extractor_t h, int frame, int level, const uint8_t** d_view, int* width,
                        int* height, int* pitch);
/* Copy the padded level plane ((w+38) x (h+38), row-major, tight) to host memory, with its whole
 * 19-pixel border REFLECT_101 as the reference's copyMakeBorder makes it (src/ORBextractor.cc:1712-1716,
 * 1734-1736): the part beyond the device's 3-pixel border is filled on the host. */
int orb_extractor_level_download(orb_extractor_t h, int frame, int level, uint8_t* host_padded);

/* ---- REGISTER_TIMES (include/Settings.h:24, src/Tracking.cc:318-420) ------------------------- */
/* Wall-clock stage timers with the reference's names: "ORB Extraction" (orb_extract; mTimeORB_Ext,
 * src/Frame.cc:132-146), "Stereo Matching" (orb_compute_stereo_matches; src/Frame.cc:158-170), "LBA"
 * (the host side of Optimizer::LocalBundleAdjustment in include/orbgpu_optimizer.hpp, gather to
 * write-back, as vdLBA_ms brackets the whole call, src/LocalMapping.cc:208-219; no sample when the
 * shim returns kFallback).  Off by default.  orb_timers_enable(1) (or ORBGPU_REGISTER_TIMES=1): every
 * orb_extract / orb_compute_stereo_matches call records a sample -- one per image, where the reference
 * records one per Frame (a stereo pair's two extractions, run in parallel, are one sample).
 * orb_timers_enable(2) (or ORBGPU_REGISTER_TIMES=2): no per-call samples; the caller brackets its
 * Frame and records it with orb_timer_add, as Frame.cc does.  orb_timer_stats gives mean and
 * population std (calcAverage / calcDeviation, src/Tracking.cc:189-208); orb_timers_write writes them
 * as ExecMean.txt lines ("ORB Extraction: mean$\pm$std", fixed with 5 decimals: `f << fixed`,
 * src/Tracking.cc:327, then setprecision(5), :335). */
int orb_timers_enable(int on);
/* The timer mode (0 off, 1 per-call brackets, 2 caller brackets only). */
int orb_timers_enabled(void);
int orb_timers_reset(void);
int orb_timer_add(const char* name, double ms);
int orb_timer_stats(const char* name, double* mean_ms, double* std_ms, long long* count);
int orb_timers_write(const char* path);

/* ---- ORBmatcher (src/ORBmatcher.cc) ---------------------------------------------------------- */

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:2384-2404) on host data, for ABI completeness. */
int orb_descriptor_distance(const uint8_t* a, const uint8_t* b);

/* Brute-force Hamming matching on device data: for each query i (n_query x 32 B) find the best and
 * second-best train descriptor (n_train x 32 B).  Writes best_idx[i], best_dist[i], second_dist[i]
 * (256+1 = "none").  The distance is DescriptorDistance.  Device pointers, async on `stream`. */
int orb_hamming_knn2_device(const uint8_t* d_query, int n_query, const uint8_t* d_train, int n_train,
                            int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second_dist,
                            void* stream);

/* Cross-frame matching on a batch of device feature blocks (the extractor's [F][cap] layout, e.g. the
 * C4 all-gather's): for each pair p = (query frame pairs[2p], train frame pairs[2p+1]) every query
 * descriptor's best / second-best train descriptor, as orb_hamming_knn2_device (DescriptorDistance,
 * src/ORBmatcher.cc:2384-2404; first index on ties).  Frame f holds counts[f * count_stride] descriptors
 * (read on the device); outputs are [n_pairs][cap], rows beyond the query frame's count get
 * (-1, 257, 257).  cap <= 2048.  One launch, async on `stream`. */
int orb_hamming_knn2_frames_device(const uint8_t* d_desc, const int32_t* d_counts, int count_stride, int cap,
                                   const int32_t* d_pairs, int n_pairs, int32_t* d_best_idx, int32_t* d_best_dist,
                                   int32_t* d_second_dist, void* stream);

/* ---- ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:1046-1324) ------------------------- */

/* Flat view of the KeyFrame fields SearchForTriangulation reads (host memory).  Pinhole camera,
 * no second camera (mpCamera2 == NULL, NLeft == -1): the configuration LocalMapping runs for
 * monocular / stereo / RGB-D pinhole rigs. */
typedef struct orb_kf_view {
    int32_t n;                     /* KeyFrame::N */
    const orb_keypoint_t* kps_un;  /* mvKeysUn (n) */
    const uint8_t* desc;           /* mDescriptors, n x 32 bytes, row-major */
    const float* u_right;          /* mvuRight (n); NULL = monocular (every entry -1) */
    const uint8_t* has_mappoint;   /* n flags, 1 = GetMapPoint(i) != NULL; NULL = no map points */
    int32_t n_nodes;               /* mFeatVec.size() (DBoW2::FeatureVector, a std::map) */
    const uint32_t* fv_node;       /* node ids, strictly ascending (map order) */
    const int32_t* fv_offset;      /* n_nodes + 1 CSR offsets into fv_index */
    const int32_t* fv_index;       /* feature indices, each node's vector in its order */
    float fx, fy, cx, cy;          /* mpCamera->mvParameters (Pinhole::toK_, src/CameraModels/Pinhole.cpp:168-173) */
    int32_t nlevels;               /* <= 12 */
    const float* scale_factors;    /* mvScaleFactors (nlevels) */
    const float* level_sigma2;     /* mvLevelSigma2 (nlevels) */
} orb_kf_view_t;

/* Per-pair geometry SearchForTriangulation derives from the two poses (src/ORBmatcher.cc:1063-1090):
 * T12 = T1w * Tw2 (R12 row-major, t12) and the epipole ep = pKF2->mpCamera->project(T2w * Cw1).
 * A C++ caller fills it with Sophus exactly as the reference does; orb_kf_pair_geometry computes
 * it from two 3x4 [R|t] poses for callers without Sophus. */
typedef struct orb_kf_pair_geom {
    float R12[9];
    float t12[3];
    float ep[2];
} orb_kf_pair_geom_t;

typedef struct orb_matcher_s* orb_matcher_t;

/* ORBmatcher(float nnratio, bool checkOri) (include/ORBmatcher.h:40).  The handle owns device
 * staging buffers and a stream; one handle per thread (like one ORBmatcher object). */
int orb_matcher_create(float nnratio, int check_orientation, orb_matcher_t* out);
int orb_matcher_destroy(orb_matcher_t m);

/* ---- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:438-529), batched over map points.
 * Point p's descriptors are rows [offsets[p], offsets[p+1]) of desc (n x 32 bytes): the reference's
 * vDescriptors, i.e. the observations in std::map order, left then right index, bad keyframes
 * skipped.  best[p] receives the row (within the point) whose median distance to the point's rows
 * (index floor(0.5 (N - 1)) of the sorted row, self included) is the smallest, the first one on ties,
 * or -1 for a point without rows; out[32 p ..] receives that descriptor (mDescriptor), untouched for
 * an empty point (the reference returns early).  N < 65536 per point: the host entry rejects a larger
 * point with ORB_ERR_ARG; the device entry cannot see the offsets, so its caller keeps that limit. */
/* Host arrays through the matcher handle's staging buffers, synchronous. */
int orb_compute_distinctive_descriptors(orb_matcher_t m, const uint8_t* desc, const int32_t* offsets, int n_points,
                                        int32_t* best, uint8_t* out);
/* Device arrays (d_offsets: n_points + 1 ints, d_desc / d_out 16-byte aligned), async on `stream`. */
int orb_compute_distinctive_descriptors_device(const uint8_t* d_desc, const int32_t* d_offsets, int n_points,
                                               int32_t* d_best, uint8_t* d_out, void* stream);

/* T1w, T2w: 3x4 row-major [R|t] world->camera poses (float); fx..cy: camera of KF2. */
int orb_kf_pair_geometry(const float T1w[12], const float T2w[12], float fx2, float fy2, float cx2, float cy2,
                         orb_kf_pair_geom_t* out);

/* SearchForTriangulation(pKF1, pKF2[p], vMatchedPairs, bOnlyStereo, bCoarse) for n_pairs
 * neighbours of one keyframe in one launch (LocalMapping::CreateNewMapPoints calls it once per
 * covisible KF, src/LocalMapping.cc:610).  Host memory, synchronous.  Writes
 * matches12[p * kf1->n + i] = matched index in kf2s[p] or -1 (vMatchedPairs is the list of
 * (i, matches12[i]) with matches12[i] >= 0 in increasing i) and n_matches[p] (the return value). */
int orb_search_for_triangulation(orb_matcher_t m, const orb_kf_view_t* kf1, const orb_kf_view_t* kf2s,
                                 const orb_kf_pair_geom_t* geoms, int n_pairs, int only_stereo, int coarse,
                                 int32_t* matches12, int32_t* n_matches);

/* The same search on device-resident keyframes: the features orb_extract_batch_device wrote (d_kps /
 * d_desc at frame f * cap, the count at d_counts[2 f]), the u_right orb_compute_stereo_matches_batch_device
 * wrote and the FeatureVector orb_bow_transform_frames_device wrote, with no host hop for any of them
 * (the chain KeyFrame::ComputeBoW -> LocalMapping::CreateNewMapPoints, src/KeyFrame.cc:109,
 * src/LocalMapping.cc:536-610, after the stereo Frame of src/Frame.cc:136-146).  Counts are read on
 * the device; `cap` bounds them. */
typedef struct orb_kf_device {
    const orb_keypoint_t* kps;     /* device: mvKeysUn, cap entries */
    const uint8_t* desc;           /* device: cap x 32 bytes */
    const int32_t* n;              /* device: KeyFrame::N (e.g. &d_counts[2 f] of orb_extract_batch_device) */
    const float* u_right;          /* device: mvuRight (cap), NULL = monocular */
    const uint8_t* has_mappoint;   /* device: cap flags (GetMapPoint(i) != NULL), NULL = none */
    const int32_t* fv_node;        /* device: FeatureVector node ids, ascending */
    const int32_t* fv_begin;       /* device: n_nodes + 1 offsets into fv_feat */
    const int32_t* fv_feat;        /* device: feature indices, each node's in ascending order */
    const int32_t* n_nodes;        /* device: FeatureVector size (e.g. &d_bow_counts[2 f + 1]) */
    int32_t cap;                   /* upper bound of *n and *n_nodes */
    float fx, fy, cx, cy;          /* host: pinhole parameters */
    int32_t nlevels;               /* <= 12 */
    const float* scale_factors;    /* host: mvScaleFactors */
    const float* level_sigma2;     /* host: mvLevelSigma2 */
} orb_kf_device_t;

/* SearchForTriangulation(kf1s[pair_kf1[p]], kf2s[p]) for p < n_pairs in one launch, device-resident,
 * asynchronous on `stream`: the neighbours of one new keyframe (pair_kf1 = NULL: every pair uses
 * kf1s[0]), or of several queued keyframes.  With C = max over kf1s of cap:
 * d_matches12[p * C + i] = index in kf2s[p] or -1 (i < C); d_n_matches[p] = the count.  The pair
 * geometry and F12 are uploaded from the host (a few hundred bytes per pair).  Counts are clamped to
 * cap; a keyframe whose *n is negative or above cap, or whose *n_nodes is negative (a frame the
 * extractor flagged ORB_ERR_CAPACITY, which the BoW transform passes on), gets no matches and its
 * pairs report d_n_matches[p] = ORB_ERR_CAPACITY. */
int orb_search_for_triangulation_device(orb_matcher_t m, const orb_kf_device_t* kf1s, int n_kf1,
                                        const orb_kf_device_t* kf2s, const int32_t* pair_kf1,
                                        const orb_kf_pair_geom_t* geoms, int n_pairs, int only_stereo, int coarse,
                                        int32_t* d_matches12, int32_t* d_n_matches, void* stream);

/* ---- ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (src/ORBmatcher.cc:260-494) ----
 * The matcher of Tracking::TrackReferenceKeyFrame (src/Tracking.cc:3943) and, once per candidate
 * keyframe, of Tracking::Relocalization.  Single camera (F.Nleft == -1, mpCamera2 == NULL).  Only
 * features under the same FeatureVector node are compared; inside a node the keyframe's features are
 * visited in stored order, each taking its best frame feature among those no earlier one took (best /
 * second best with strict `<` from 256 / -1 / 256, the first index on ties), accepted when
 * bestDist1 <= TH_LOW and bestDist1 < mfNNratio * bestDist2; then, with mbCheckOrientation, the rotation
 * histogram (factor 1 / HISTO_LENGTH as upstream has it) and ComputeThreeMaxima.  nnratio and
 * check_orientation come from the handle.
 *
 * n_kfs keyframes against one frame in one launch (host memory, synchronous, through the handle's
 * staging buffers and stream).  Of a view the search reads n, kps_un (the angle; mvKeys and mvKeysUn share
 * it), desc and the three fv_* arrays, and of a keyframe its usable flags: point_ok[p][i] = 1 when
 * pKF->GetMapPointMatches()[i] is non-NULL and not isBad() (point_ok or point_ok[p] NULL: the view's
 * has_mappoint; that NULL too: no usable map point).  Writes matches[p * frame->n + iF] = the keyframe
 * feature whose map point vpMapPointMatches[iF] receives, or -1, and n_matches[p] (the return value).  A
 * view that lists a feature twice or an index >= n gives ORB_ERR_ARG. */
int orb_search_by_bow(orb_matcher_t m, const orb_kf_view_t* kfs, const uint8_t* const* point_ok, int n_kfs,
                      const orb_kf_view_t* frame, int32_t* matches, int32_t* n_matches);

/* The same on device-resident sides (the orb_extract_batch_device / orb_bow_transform_frames_device
 * layout of orb_kf_device_t, for the frames too), asynchronous on `stream`: pair p searches keyframe
 * kfs[p] against frames[pair_frame[p]] (pair_frame NULL: frames[0]).  d_point_ok[p]: the keyframe's
 * device flag array (cap entries; d_point_ok or the entry NULL: its has_mappoint).  Of a side the search
 * reads kps, desc, n, the fv_* arrays, n_nodes and cap (< 2^20).  With C = max over frames of cap:
 * d_matches[p * C + iF] (-1 past the frame's count), d_n_matches[p].  Counts are read on the device and
 * clamped to cap; a side whose *n is negative or above cap, or whose *n_nodes is negative (flagged
 * ORB_ERR_CAPACITY by its producer), gives d_n_matches[p] = ORB_ERR_CAPACITY and no matches. */
int orb_search_by_bow_device(orb_matcher_t m, const orb_kf_device_t* kfs, const uint8_t* const* d_point_ok, int n_pairs,
                             const orb_kf_device_t* frames, int n_frames, const int32_t* pair_frame,
                             int32_t* d_matches, int32_t* d_n_matches, void* stream);

/* ---- ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (src/ORBmatcher.cc:893-1044) ----
 * Loop closing's matcher of the current keyframe against each keyframe of a candidate's window
 * (src/LoopClosing.cc:840-851), single camera (NLeft == -1).  The node walk of the overload above with both
 * sides masked (ok[i] = 1: the feature's map point is non-NULL and not isBad()), the claim mark on the second
 * side (vbMatched2, set at acceptance and not released when the rotation check later removes the match), the
 * result indexed by the first side's features, and the acceptance bestDist1 < TH_LOW, strict, and
 * (float)bestDist1 < mfNNratio * (float)bestDist2.  The rotation histogram is over idx1 with
 * kps1[idx1].angle - kps2[bestIdx2].angle and factor 1 / HISTO_LENGTH.
 *
 * kf1 against n_pairs second keyframes in one launch (host memory, synchronous).  ok1: kf1->n flags, ok2s[p]:
 * kf2s[p].n flags (ok1, ok2s or ok2s[p] NULL: the view's has_mappoint; that NULL too: no usable map point).
 * Writes matches12[p * kf1->n + idx1] = the matched feature of kf2s[p] (vpMatches12[idx1] is the caller's
 * mvpMapPoints2[that index]) or -1, and n_matches[p] (the return value).  Views are validated as in
 * orb_search_by_bow. */
int orb_search_by_bow_kf(orb_matcher_t m, const orb_kf_view_t* kf1, const uint8_t* ok1, const orb_kf_view_t* kf2s,
                         const uint8_t* const* ok2s, int n_pairs, int32_t* matches12, int32_t* n_matches);

/* The same on device-resident sides, asynchronous on `stream`: pair p searches kf1s[pair_kf1[p]] (pair_kf1
 * NULL: kf1s[0]) against kf2s[p].  d_ok1[k]: device flags of kf1s[k] (cap entries), d_ok2[p]: of kf2s[p] (either
 * array or an entry NULL: the side's has_mappoint).  With C = max over kf1s of cap: d_matches12[p * C + idx1]
 * (-1 past the count), d_n_matches[p].  Counts are read on the device; a side whose *n is negative or above
 * cap, or whose *n_nodes is negative, gives d_n_matches[p] = ORB_ERR_CAPACITY and an all -1 row.  Every
 * argument is checked before anything is launched or written; the number of launches does not depend on
 * n_pairs. */
int orb_search_by_bow_kf_device(orb_matcher_t m, const orb_kf_device_t* kf1s, int n_kf1, const uint8_t* const* d_ok1,
                                const orb_kf_device_t* kf2s, const uint8_t* const* d_ok2, const int32_t* pair_kf1,
                                int n_pairs, int32_t* d_matches12, int32_t* d_n_matches, void* stream);

/* ---- Frame::UndistortKeyPoints (src/Frame.cc:1003-1051): mvKeysUn from mvKeys by cv::undistortPoints
 * (OpenCV 4.x: five fixed-point iterations of the inverse k1 k2 p1 p2 k3 model in double, P = K, the
 * result rounded to float; parity with a real OpenCV build unpinned), on the extractor's device layout:
 * frame f's keypoints at d_kps[f * cap], its count at d_counts[2 f] (orb_extract_batch_device).
 * d_kps_un receives the same records with pt undistorted (i < count; the rest is not written); a frame
 * flagged ORB_ERR_CAPACITY is skipped.  K = (fx, fy, cx, cy); dist = mDistCoef (n_dist 4 or 5 floats);
 * dist[0] == 0 copies mvKeys, as the reference does.  d_kps_un may equal d_kps.  Async on `stream`. */
int orb_undistort_keypoints_device(const orb_keypoint_t* d_kps, const int32_t* d_counts, int n_frames, int cap,
                                   const float K[4], const float* dist, int n_dist, orb_keypoint_t* d_kps_un,
                                   void* stream);

/* ---- ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono) (src/ORBmatcher.cc:1951-2185)
 * Pinhole frames without a second camera (Nleft == -1). */

/* The current frame: keypoints, descriptors, the feature grid bounds (Frame::mnMinX.., the grid
 * element inverse sizes; FRAME_GRID_COLS x ROWS = 64 x 48, include/Frame.h:44-45) and its pose. */
typedef struct orb_frame_view {
    int32_t n;
    const orb_keypoint_t* kps_un;   /* mvKeysUn */
    const uint8_t* desc;            /* mDescriptors, n x 32 */
    const float* u_right;           /* mvuRight (n); NULL = monocular */
    float min_x, max_x, min_y, max_y;       /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    float grid_inv_w, grid_inv_h;           /* mfGridElementWidthInv, mfGridElementHeightInv */
    float fx, fy, cx, cy;                   /* mpCamera parameters */
    float bf, b;                            /* mbf, mb */
    int32_t nlevels;
    const float* scale_factors;             /* mvScaleFactors (nlevels) */
    float Tcw[12];                          /* GetPose(), 3x4 row-major [R|t] */
} orb_frame_view_t;

/* The last frame's tracked map points, indexed like LastFrame's keypoints. */
typedef struct orb_last_points {
    int32_t n;                      /* LastFrame.N */
    const uint8_t* valid;           /* mvpMapPoints[i] != NULL && !mvbOutlier[i] */
    const uint8_t* observed;        /* mvpMapPoints[i]->Observations() > 0 */
    const float* xyz;               /* mvpMapPoints[i]->GetWorldPos(), n x 3 */
    const uint8_t* desc;            /* mvpMapPoints[i]->GetDescriptor(), n x 32 */
    const orb_keypoint_t* kps_un;   /* LastFrame.mvKeysUn (octave and angle) */
    float Tcw[12];                  /* LastFrame.GetPose() */
} orb_last_points_t;

/* match[i2] receives the LastFrame index whose map point was assigned to current keypoint i2 (-1:
 * none).  Like the reference, points are processed in index order and a keypoint already holding
 * a map point with observations is skipped by later points; `check_ori` comes from the matcher
 * handle.  Returns the number of matches in *n_matches.  Host memory, synchronous. */
int orb_search_by_projection_frame(orb_matcher_t m, const orb_frame_view_t* cur, const orb_last_points_t* last,
                                   float th, int mono, int32_t* match, int32_t* n_matches);

/* ---- ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints)
 * (src/ORBmatcher.cc:46-240, called from Tracking::SearchLocalPoints).  The local map points with the
 * tracking fields Frame::isInFrustum wrote into them (src/Frame.cc:667-773). */
typedef struct orb_local_points {
    int32_t n;                      /* vpMapPoints.size() */
    const uint8_t* track_in_view;   /* mbTrackInView */
    const uint8_t* is_bad;          /* isBad() */
    const uint8_t* observed;        /* Observations() > 0 */
    const float* track_proj;        /* n x 3: mTrackProjX, mTrackProjY, mTrackProjXR */
    const float* track_view_cos;    /* mTrackViewCos */
    const float* track_depth;       /* mTrackDepth */
    const int32_t* track_level;     /* mnTrackScaleLevel */
    const uint8_t* desc;            /* GetDescriptor(), n x 32 */
} orb_local_points_t;

/* frame_taken[i]: F.mvpMapPoints[i] != NULL && ->Observations() > 0 before the call (NULL: none).
 * match[i] receives the index into vpMapPoints of the map point assigned to keypoint i by this
 * call (-1: none); points are processed in order and the ratio test uses the handle's nnratio. */
int orb_search_by_projection_local(orb_matcher_t m, const orb_frame_view_t* frame, const uint8_t* frame_taken,
                                   const orb_local_points_t* pts, float th, int far_points, float th_far_points,
                                   int32_t* match, int32_t* n_matches);

/* ---- The same two searches on device-resident frames (the tracking chain of Tracking::TrackWithMotionModel
 * -> TrackLocalMap, src/Tracking.cc:4112-4217, 4742-4825, without a host hop between the stages).  The
 * current frame's keypoints are the extractor's (or orb_undistort_keypoints_device's) device outputs;
 * counts are read on the device and clamped to `cap`.  Host scalars (pose, bounds, camera) travel in the
 * struct.  Results land in device memory, asynchronously on `stream`: d_match[i] for i < cap (-1 past
 * the frame's count), *d_n_matches.  Every candidate list is sized for the whole frame, so no call is
 * redone; scratch is allocated and freed on `stream`.  The matcher handle contributes only its ratio
 * and orientation flag (calls on different streams may share it). */
typedef struct orb_frame_device {
    const orb_keypoint_t* kps_un;   /* device: mvKeysUn, cap entries */
    const uint8_t* desc;            /* device: cap x 32 */
    const int32_t* n;               /* device: N (e.g. &d_counts[2 f] of orb_extract_batch_device) */
    const float* u_right;           /* device: mvuRight (cap), NULL = monocular */
    int32_t cap;                    /* upper bound of *n, <= 16384 */
    float min_x, max_x, min_y, max_y;       /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    float grid_inv_w, grid_inv_h;           /* mfGridElementWidthInv, mfGridElementHeightInv */
    float fx, fy, cx, cy;                   /* mpCamera parameters */
    float bf, b;                            /* mbf, mb */
    int32_t nlevels;
    const float* scale_factors;             /* host: mvScaleFactors (nlevels) */
    float Tcw[12];                          /* host: GetPose(), 3x4 row-major [R|t] */
} orb_frame_device_t;

/* The last frame's tracked map points, device arrays indexed like its keypoints (cap entries). */
typedef struct orb_last_points_device {
    const int32_t* n;               /* device: LastFrame.N */
    int32_t cap;
    const uint8_t* valid;           /* mvpMapPoints[i] != NULL && !mvbOutlier[i] */
    const uint8_t* observed;        /* mvpMapPoints[i]->Observations() > 0 */
    const float* xyz;               /* mvpMapPoints[i]->GetWorldPos(), cap x 3 */
    const uint8_t* desc;            /* mvpMapPoints[i]->GetDescriptor(), cap x 32 */
    const orb_keypoint_t* kps_un;   /* LastFrame.mvKeysUn (octave and angle) */
    float Tcw[12];                  /* host: LastFrame.GetPose() */
} orb_last_points_device_t;

/* Local map points, device arrays (n on the host: the size of mvpLocalMapPoints), e.g. the outputs of
 * orb_is_in_frustum_device for the tracking fields. */
typedef struct orb_local_points_device {
    int32_t n;
    const uint8_t* track_in_view;
    const uint8_t* is_bad;
    const uint8_t* observed;
    const float* track_proj;        /* n x 3 */
    const float* track_view_cos;
    const float* track_depth;
    const int32_t* track_level;
    const uint8_t* desc;            /* n x 32 */
} orb_local_points_device_t;

int orb_search_by_projection_frame_device(orb_matcher_t m, const orb_frame_device_t* cur,
                                          const orb_last_points_device_t* last, float th, int mono, int32_t* d_match,
                                          int32_t* d_n_matches, void* stream);
/* d_frame_taken: device, cap flags (NULL: none). */
int orb_search_by_projection_local_device(orb_matcher_t m, const orb_frame_device_t* frame, const uint8_t* d_frame_taken,
                                          const orb_local_points_device_t* pts, float th, int far_points,
                                          float th_far_points, int32_t* d_match, int32_t* d_n_matches, void* stream);

/* ---- Frame::isInFrustum (src/Frame.cc:667-773, pinhole, Nleft == -1) + MapPoint::PredictScale
 * (src/MapPoint.cc:715-731): the tracking fields of the local map points that
 * orb_search_by_projection_local reads.  Per point: Pc = Rcw P + tcw, depth > 0, projection inside
 * [mnMinX, mnMaxX] x [mnMinY, mnMaxY], distance to mOw inside [0.8 mfMinDistance, 1.2 mfMaxDistance],
 * viewing cosine against the normal >= viewingCosLimit, predicted level ceil(log(mfMaxDistance /
 * dist) / mfLogScaleFactor) clamped to [0, mnScaleLevels).  Float arithmetic as the reference build
 * contracts it (see oracle/orb_frustum_oracle.cpp). */
typedef struct orb_frustum_frame {
    float Tcw[12];              /* [mRcw | mtcw], row-major 3 x 4 */
    float Ow[3];                /* mOw (camera centre) */
    float fx, fy, cx, cy, bf;   /* pinhole parameters, mbf */
    float min_x, max_x, min_y, max_y;  /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    float log_scale_factor;     /* mfLogScaleFactor */
    int32_t n_levels;           /* mnScaleLevels */
} orb_frustum_frame_t;

/* Host arrays: pos / normal n x 3 (GetWorldPos, GetNormal), min_dist / max_dist (mfMinDistance,
 * mfMaxDistance).  Writes in_view (mbTrackInView), proj n x 3 (mTrackProjX, mTrackProjY -- also set,
 * as in the reference, when only the distance / angle tests fail; -1 before the image test --
 * and mTrackProjXR), depth (mTrackDepth), level (mnTrackScaleLevel), view_cos (mTrackViewCos);
 * fields the reference leaves untouched for rejected points are written as 0.  Synchronous;
 * returns the number of points in view. */
int orb_is_in_frustum(const orb_frustum_frame_t* frame, int n, const float* pos, const float* normal,
                      const float* min_dist, const float* max_dist, float viewing_cos_limit, uint8_t* in_view,
                      float* proj, float* depth, int32_t* level, float* view_cos);
/* The same on device arrays, async on `stream`. */
int orb_is_in_frustum_device(const orb_frustum_frame_t* frame, int n, const float* d_pos, const float* d_normal,
                             const float* d_min_dist, const float* d_max_dist, float viewing_cos_limit,
                             uint8_t* d_in_view, float* d_proj, float* d_depth, int32_t* d_level, float* d_view_cos,
                             void* stream);

/* The same with the frame's pose read on the device: d_pose7 is PoseOptimization's output (the
 * g2o SE3Quat vector tx ty tz qx qy qz qw); the frame's Tcw / Ow follow Frame::SetPose on its float cast
 * (src/Optimizer.cc:390-395, src/Frame.cc:533-599: the quaternion normalised, Eigen's rotation matrix, Ow =
 * q^-1 (-t)); frame->Tcw and frame->Ow are ignored.  The link between PoseOptimization and
 * SearchLocalPoints in the device tracking chain. */
int orb_is_in_frustum_pose_device(const orb_frustum_frame_t* frame, const double* d_pose7, int n, const float* d_pos,
                                  const float* d_normal, const float* d_min_dist, const float* d_max_dist,
                                  float viewing_cos_limit, uint8_t* d_in_view, float* d_proj, float* d_depth,
                                  int32_t* d_level, float* d_view_cos, void* stream);

/* ---- ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th, bRight = false) (src/ORBmatcher.cc:1326-1534)
 * The search half (steps 1-6, :1356-1506) of the matcher LocalMapping::SearchInNeighbors runs once per
 * target keyframe and once in the other direction (src/LocalMapping.cc:917-1066), for jobs (keyframe k,
 * point i), k < n_kfs, i < points->n: all keyframes share one point set.  Single camera (NLeft == -1).  Per
 * job: Pc = Rcw P + tcw; Pc.z < 0 rejected; (u, v) = Pinhole::project; KeyFrame::IsInImage (half open: u >=
 * min_x && u < max_x, v likewise); ur = u - bf / Pc.z; the distance to Ow inside [0.8 mfMinDistance, 1.2
 * mfMaxDistance]; PO . normal >= 0.5 dist; MapPoint::PredictScale(dist, pKF) (src/MapPoint.cc:688-706);
 * radius = th * mvScaleFactors[level]; KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:843-891: cells ix outer,
 * iy inner, a cell's keypoints in index order, |dx| < r && |dy| < r, no level filter); per keypoint the
 * octave in [level - 1, level] and the chi-square gate (mvuRight[idx] >= 0: (ex^2 + ey^2 + er^2) *
 * mvInvLevelSigma2[octave] > 7.8 rejected, else (ex^2 + ey^2) * ... > 5.99; the float product compared in
 * double); the first minimum of DescriptorDistance from 256 / -1.  Float arithmetic as the reference build
 * contracts it (oracle/orb_frustum_oracle.cpp, oracle/orb_projection_oracle.cpp).
 *   best_idx[k * n + i] = bestIdx when bestDist <= TH_LOW (50), else -1 (also for a skipped job);
 *   best_dist[k * n + i] = bestDist, the minimum found (256 when none or skipped).
 * The map mutation (step 7, :1506-1527: Replace / AddObservation / AddMapPoint) stays with the caller
 * (include/orbgpu_matcher.hpp), like every other map write.  The keyframe's grid (KeyFrame::mGrid) is
 * built on the device from kps_un and the bounds. */
typedef struct orb_fuse_kf {
    orb_frame_view_t frame;         /* N, mvKeysUn, mDescriptors, mvuRight, bounds, grid inverses, camera, mbf,
                                       levels, mvScaleFactors, GetPose() (`b` is not read); nlevels <= 12 */
    float Ow[3];                    /* GetCameraCenter() */
    const float* inv_level_sigma2;  /* mvInvLevelSigma2 (nlevels) */
    float log_scale_factor;         /* mfLogScaleFactor */
} orb_fuse_kf_t;

/* The same around a device-resident keyframe: the count is read on the device (cap <= 16384); a negative
 * or over-cap count (a frame its producer flagged ORB_ERR_CAPACITY) gives no matches for that keyframe
 * (-1 / 256 everywhere).  scale_factors and inv_level_sigma2 are host arrays. */
typedef struct orb_fuse_kf_device {
    orb_frame_device_t frame;
    float Ow[3];
    const float* inv_level_sigma2;  /* host: mvInvLevelSigma2 (nlevels) */
    float log_scale_factor;
} orb_fuse_kf_device_t;

/* vpMapPoints as flat arrays (host memory); n <= 2^20. */
typedef struct orb_fuse_points {
    int32_t n;
    const float* pos;               /* GetWorldPos(), n x 3 */
    const float* normal;            /* GetNormal(), n x 3 */
    const float* min_dist;          /* mfMinDistance (raw, as orb_is_in_frustum takes it) */
    const float* max_dist;          /* mfMaxDistance */
    const uint8_t* desc;            /* GetDescriptor(), n x 32 */
} orb_fuse_points_t;

/* The same on device arrays (desc 16-byte aligned); n on the host. */
typedef struct orb_fuse_points_device {
    int32_t n;
    const float* pos;
    const float* normal;
    const float* min_dist;
    const float* max_dist;
    const uint8_t* desc;
} orb_fuse_points_device_t;

/* Host memory, synchronous, through the handle's staging buffers and stream.  skip[k * n + i] != 0: the
 * job is not searched (vpMapPoints[i] NULL, isBad() or IsInKeyFrame(kfs[k])); skip may be NULL (no job
 * skipped), best_dist may be NULL.  th > 0.  n == 0 or n_kfs == 0: ORB_OK, nothing launched. */
int orb_fuse(orb_matcher_t m, const orb_fuse_kf_t* kfs, int n_kfs, const orb_fuse_points_t* points,
             const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist);
/* The same on device arrays (d_skip, d_best_idx, d_best_dist: n_kfs x n), asynchronous on `stream`;
 * scratch (the grids) is allocated and freed on `stream`.  n_kfs <= 65535. */
int orb_fuse_device(orb_matcher_t m, const orb_fuse_kf_device_t* kfs, int n_kfs,
                    const orb_fuse_points_device_t* points, const uint8_t* d_skip, float th, int32_t* d_best_idx,
                    int32_t* d_best_dist, void* stream);

/* ---- Loop closing's Sim3 searches, batched (src/LoopClosing.cc:976, :1005, :1265, :2712, :2765) --------
 * ORBmatcher::SearchByProjection(KF, Scw, vpPoints, vpMatched, th, ratioHamming) (src/ORBmatcher.cc:496-619),
 * its overload that also fills vpMatchedKF (:621-733) and the search half of ORBmatcher::Fuse(KF, Scw,
 * vpPoints, th, vpReplacePoint) (:1547-1651).  A job is one call of one of them: keyframe kfs[kf], the pose
 * (Tcw = SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale()), Ow = Tcw.inverse().translation(), both
 * computed by the caller), the points pool[first .. first + count), th, ratioHamming and a mode.  Jobs of one
 * call may share a keyframe (one keyframe against B candidate poses) or a point range (ten keyframes against
 * one window); the number of kernel launches does not depend on the job count.  Single pinhole camera
 * (NLeft == -1).  Per point p of job b, in the reference's order: skipped when skip[] is set; Pc = Rcw P +
 * tcw; Pc.z < 0 rejected; (u, v) by the mode; KeyFrame::IsInImage (half open: u >= min_x && u < max_x, v
 * likewise); the distance to Ow inside [0.8 mfMinDistance, 1.2 mfMaxDistance]; PO . normal >= 0.5 dist;
 * MapPoint::PredictScale(dist, pKF); radius = th * mvScaleFactors[level]; KeyFrame::GetFeaturesInArea (cells
 * ix outer, iy inner, a cell's keypoints in index order, |dx| < r && |dy| < r); per keypoint the octave in
 * [level - 1, level]; the first minimum of DescriptorDistance.  There is no chi-square gate and no u_R.
 * Float arithmetic as the reference build contracts it (oracle/orb_projection_oracle.cpp).
 *   ORB_S3P_CLAIM_PROJECT  (:496)  u = fx * Pc.x / Pc.z + cx (Pinhole::project).  Points are taken in order, a
 *                          keypoint that an earlier point of the job matched, or that taken0 flags
 *                          (vpMatched[idx] != NULL before the call), is skipped by every later point (:589);
 *                          a match needs (float)bestDist <= 50 * ratioHamming.
 *   ORB_S3P_CLAIM_INVZ     (:621)  the same with invz = 1 / Pc.z, x = Pc.x * invz, u = fx * x + cx (one fma).
 *   ORB_S3P_FUSE           (:1547) Pinhole::project, no claims, bestDist <= 50; ratio_hamming and taken0 are
 *                          not read.  The map mutation (:1655-1672) stays with the caller.
 * Outputs.  The points of job b sit at off(b) + p, off(b) = the sum of the counts of the jobs before b, in
 * skip, best_idx and best_dist (sum-of-counts entries each); matched and taken0 have `stride` entries per
 * job, stride >= every keyframe's N (capacity, for the device entry).
 *   matched[b * stride + j]  the point p of job b that was matched to keypoint j, or -1 (also where taken0 is
 *                            set, past the keyframe's count, and everywhere for a FUSE job);
 *   nmatches[b]              the reference's return value (for FUSE: the points with bestDist <= 50, nFused);
 *   best_idx[off(b) + p]     the keypoint point p was matched to, or -1;
 *   best_dist[off(b) + p]    claim modes: the distance of that match, 256 without one; FUSE: the minimum
 *                            found, as orb_fuse reports it (256 when none, skipped or gated).
 * The result is the sequential loop's for any input: nothing is truncated.
 * Limits: n_jobs <= 65535, n_kfs <= 1024, N / cap <= 16384, pool <= 2^20 points, at most 2^24 points over all
 * jobs (ORB_ERR_CAPACITY beyond); nlevels <= 12, th > 0, 0 < 50 * ratioHamming < 256 in the claim modes
 * (ORB_ERR_ARG).  Every argument is checked before anything is launched or written. */
enum { ORB_S3P_CLAIM_PROJECT = 0, ORB_S3P_CLAIM_INVZ = 1, ORB_S3P_FUSE = 2 };

typedef struct orb_sim3_projection_kf {
    orb_frame_view_t frame;         /* N, mvKeysUn, mDescriptors, bounds, grid inverses, camera, levels,
                                       mvScaleFactors (u_right, bf, b and Tcw are not read) */
    float log_scale_factor;         /* mfLogScaleFactor */
} orb_sim3_projection_kf_t;

/* The same around a device-resident keyframe: the count is read on the device; a negative or over-cap
 * count gives an empty result for every job of that keyframe.  scale_factors is a host array. */
typedef struct orb_sim3_projection_kf_device {
    orb_frame_device_t frame;
    float log_scale_factor;
} orb_sim3_projection_kf_device_t;

typedef struct orb_sim3_projection_job {
    int32_t kf;                     /* index into kfs */
    int32_t first, count;           /* the job's points: pool[first .. first + count) */
    int32_t mode;                   /* ORB_S3P_* */
    float th, ratio_hamming;
    float Tcw[12];                  /* 3x4 row-major [R | t] of the SE3 taken from Scw */
    float Ow[3];                    /* its camera centre */
} orb_sim3_projection_job_t;

/* Host memory, synchronous, through the handle's staging buffers and stream.  skip (isBad() ||
 * spAlreadyFound.count(pMP)), taken0 and best_dist may be NULL.  n_jobs == 0: ORB_OK, nothing written. */
int orb_sim3_projection(orb_matcher_t m, const orb_sim3_projection_kf_t* kfs, int n_kfs,
                        const orb_sim3_projection_job_t* jobs, int n_jobs, const orb_fuse_points_t* pool,
                        const uint8_t* skip, const uint8_t* taken0, int stride, int32_t* matched, int32_t* nmatches,
                        int32_t* best_idx, int32_t* best_dist);
/* The same on device arrays (the job records stay on the host), asynchronous on `stream`; scratch is
 * allocated and freed on `stream`. */
int orb_sim3_projection_device(orb_matcher_t m, const orb_sim3_projection_kf_device_t* kfs, int n_kfs,
                               const orb_sim3_projection_job_t* jobs, int n_jobs, const orb_fuse_points_device_t* pool,
                               const uint8_t* d_skip, const uint8_t* d_taken0, int stride, int32_t* d_matched,
                               int32_t* d_nmatches, int32_t* d_best_idx, int32_t* d_best_dist, void* stream);

/* ---- LocalMapping::CreateNewMapPoints, the triangulation half (src/LocalMapping.cc:626-910) ----------
 * For every match (idx1, idx2 = matches12[p][idx1] >= 0) of keyframe 1 against neighbour p, in one call:
 * the parallax test (:720-783), GeometricTools::Triangulate (src/GeometricTools.cc:63-90) or
 * KeyFrame::UnprojectStereo (src/KeyFrame.cc:905-924), the two depth tests (:794-800), the two reprojection
 * chi-square tests (:804-860: 5.991 sigma2 mono, 7.8 sigma2 stereo, u2_r with keyframe 1's mbf as :853 has
 * it) and the distance / octave test (:866-884).  Then the rule of the neighbour loop: upstream gives idx1 a
 * map point as soon as one neighbour succeeds and later neighbours no longer match that idx1, so the
 * smallest p whose job is ORB_NP_OK keeps it and every later ORB_NP_OK at the same idx1 becomes
 * ORB_NP_TAKEN.  The survivors are emitted as records in upstream's creation order (p ascending, then idx1
 * ascending), each with MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:567-642) of its two observations
 * (reference keyframe = keyframe 1, level = kp1.octave).  A caller that stops early at CheckNewKeyFrames()
 * (:568) before neighbour k uses the records with p < k: they are a prefix and do not depend on later
 * neighbours.  Single pinhole camera (NLeft == -1, mpCamera2 == NULL); the two-camera branch (:665-715) is
 * not implemented.  The baseline / median-depth pre-tests (:575-601) stay with the caller, who leaves a
 * skipped neighbour out; step 6's map mutation (:888-909) stays with the caller too
 * (include/orbgpu_matcher.hpp, ORBmatcher::CreateNewMapPoints).
 *
 * Float32 as upstream computes it, contractions as the reference build makes them (the list heads
 * csrc/orb_newpoints.hip); invz = 1.0 / z in double, rounded; the chi-square sums compared as doubles with
 * the double products 5.991 * sigma2 / 7.8 * sigma2; cos(2 atan2(mb / 2, depth)) in double, rounded once
 * (as (d^2 - a^2) / (d^2 + a^2), with the libm pair's values for an infinite a or d).
 * The 4x4 null vector is a float one-sided Jacobi (csrc/orb_svd4.h): at least as accurate as LAPACK's float SVD, not
 * bit-identical to Eigen's JacobiSVD.  Comparisons keep upstream's form, so non-finite values fall through
 * the same gates. */
#define ORB_NP_NO_MATCH 0      /* matches12 < 0, an index past a count, or a pair flagged ORB_ERR_CAPACITY */
#define ORB_NP_LOW_PARALLAX 1  /* the final else (:780-783): no stereo and very low parallax */
#define ORB_NP_TRI_W_ZERO 2    /* Triangulate false: x3Dh(3) == 0 */
#define ORB_NP_STEREO_DEPTH 3  /* UnprojectStereo false: mvDepth <= 0 */
#define ORB_NP_Z1 4            /* z1 <= 0 */
#define ORB_NP_Z2 5            /* z2 <= 0 */
#define ORB_NP_CHI2_1 6        /* reprojection error in keyframe 1 */
#define ORB_NP_CHI2_2 7        /* reprojection error in the neighbour */
#define ORB_NP_DIST_ZERO 8     /* dist1 == 0 || dist2 == 0 */
#define ORB_NP_FAR 9           /* mbFarPoints && (dist1 >= mThFarPoints || dist2 >= mThFarPoints) */
#define ORB_NP_SCALE 10        /* ratioDist against ratioOctave * ratioFactor */
#define ORB_NP_OK 11           /* the job triangulated and this neighbour keeps idx1 */
#define ORB_NP_TAKEN 12        /* the job triangulated, an earlier neighbour already gave idx1 its point */

/* What triangulation reads of a keyframe besides the search's view (host values unless noted). */
typedef struct orb_newpoints_kf_extra {
    float Tcw[12];                  /* GetPose().matrix3x4(), row-major */
    float Ow[3];                    /* GetCameraCenter(), as orb_fuse takes it */
    float mb, mbf, invfx, invfy;
    const float* depth;             /* mvDepth (host entry: n host floats; device entry: cap device floats);
                                       NULL = monocular (read only where u_right >= 0) */
    const orb_keypoint_t* kps_raw;  /* mvKeys, which UnprojectStereo reads; NULL = the view's mvKeysUn */
} orb_newpoints_kf_extra_t;

/* Host keyframe: of `view` the call reads n, kps_un, u_right, fx..cy, nlevels, scale_factors, level_sigma2. */
typedef struct orb_newpoints_kf {
    orb_kf_view_t view;
    orb_newpoints_kf_extra_t extra;
} orb_newpoints_kf_t;

/* Device keyframe: of `view` the call reads kps, n, u_right, cap, fx..cy, nlevels and the two host arrays. */
typedef struct orb_newpoints_kf_device {
    orb_kf_device_t view;
    orb_newpoints_kf_extra_t extra;
} orb_newpoints_kf_device_t;

typedef struct orb_newpoints_params {
    int32_t inertial;      /* mbInertial: the mono parallax limit is 0.9996 instead of 0.9998 */
    int32_t far_points;    /* mbFarPoints */
    float th_far_points;   /* mThFarPoints */
    float ratio_factor;    /* 1.5f * mfScaleFactor of keyframe 1 */
} orb_newpoints_params_t;

/* One new map point (48 bytes), in creation order. */
typedef struct orb_newpoint {
    int32_t p;             /* the neighbour: kf2s[p] */
    int32_t idx1, idx2;    /* the two observations */
    float x3d[3];          /* the world position */
    int32_t from_stereo;   /* bPointStereo */
    float normal[3];       /* mNormalVector */
    float min_dist;        /* mfMinDistance */
    float max_dist;        /* mfMaxDistance */
} orb_newpoint_t;

/* The outputs of both entries, with C the row stride of matches12 (host entry: max(kf1 n, 1); device entry:
 * kf1's cap): status [P x C] int32 (ORB_NP_*), x3d [P x C x 3] float (the position wherever one was
 * computed, i.e. status >= ORB_NP_Z1; else 0), from_stereo [P x C] uint8, taken_by [C] int32 (the
 * neighbour that keeps idx1, or -1), records [C] (an idx1 yields at most one point), n_new [1] int32. */
typedef struct orb_newpoints_out {
    int32_t* status;
    float* x3d;
    uint8_t* from_stereo;
    int32_t* taken_by;
    orb_newpoint_t* records;
    int32_t* n_new;
} orb_newpoints_out_t;

/* Host arrays through the matcher handle's staging buffers and stream, synchronous.  matches12 [n_pairs x
 * max(kf1 n, 1)] and n_matches [n_pairs] as orb_search_for_triangulation wrote them (n_matches NULL: no pair
 * is flagged; a negative n_matches[p] yields no points for pair p and its matches12 row is not read).  n_pairs <=
 * 1024, n <= 2^20 per keyframe and n_pairs * ceil(n1 / 256) <= 65536 (the record offsets come from a scan every
 * block repeats over that many counts); an octave outside [0, nlevels) or, in a pair that is not flagged, a
 * match index >= the neighbour's n gives ORB_ERR_ARG.  n_pairs == 0:
 * ORB_OK, n_new = 0, taken_by = -1. */
int orb_create_new_map_points(orb_matcher_t m, const orb_newpoints_kf_t* kf1, const orb_newpoints_kf_t* kf2s,
                              int n_pairs, const orb_newpoints_params_t* params, const int32_t* matches12,
                              const int32_t* n_matches, const orb_newpoints_out_t* out);

/* Device-resident, asynchronous on `stream`: the host never waits for the kernels or for the search before them,
 * and nothing is copied back.  Like orb_fuse_device the call does wait (hipEventSynchronize) until the previous
 * device-entry call on the same handle has copied its argument records out of the handle's pinned slot, that is
 * behind whatever was queued before that copy on its stream.  n_pairs * ceil(cap / 256) <= 65536.  d_matches12 [n_pairs x kf1 cap] and
 * d_n_matches [n_pairs] exactly as orb_search_for_triangulation_device (one first keyframe) wrote them,
 * ORB_ERR_CAPACITY in d_n_matches[p] included (no points for that pair).  `out` holds device pointers.
 * Counts are read on the device and clamped to cap; a keyframe with a flagged count, an index past a
 * count or an octave outside [0, nlevels) gives ORB_NP_NO_MATCH for the job.  The argument records and
 * the scan's scratch are allocated and freed on `stream`. */
int orb_create_new_map_points_device(orb_matcher_t m, const orb_newpoints_kf_device_t* kf1,
                                     const orb_newpoints_kf_device_t* kf2s, int n_pairs,
                                     const orb_newpoints_params_t* params, const int32_t* d_matches12,
                                     const int32_t* d_n_matches, const orb_newpoints_out_t* out, void* stream);

/* ---- Frame::ComputeStereoMatches (src/Frame.cc:1102-1358) ------------------------------------ */

/* Stereo matching of a rectified pair, on the two extractors' device pyramids (mvImagePyramid of
 * mpORBextractorLeft / mpORBextractorRight, src/Frame.cc:1241,1262) and their keypoints /
 * descriptors: per left keypoint the row-band Hamming search (TH_HIGH start, octave +-1, u range
 * [uL - bf/b, uL], accept < (TH_HIGH+TH_LOW)/2), the 11x11 SAD over +-5 px at the keypoint's
 * level, the parabola sub-pixel fit, the disparity test, then the median cull
 * (SAD >= 1.5*1.4*median dropped).  Writes mvuRight / mvDepth (-1 = no match) for the left
 * keypoints.  `left` and `right` must have extracted frames of the same size with the same
 * parameters; the pyramids of their last extraction are read.
 *
 * Host arrays, frame 0 of each handle (after orb_extract): returns the number of keypoints kept
 * (>= 0) or a negative status.  Synchronous. */
int orb_compute_stereo_matches(orb_extractor_t left, orb_extractor_t right, const orb_keypoint_t* kps_l, int n_l,
                               const uint8_t* desc_l, const orb_keypoint_t* kps_r, int n_r, const uint8_t* desc_r,
                               float bf, float b, float* u_right, float* depth);
/* Device batch: frames 0..n-1 of both handles (after orb_extract_batch_device), keypoints
 * [n][cap] and counts [n][2] (element 0 = keypoint count) exactly as orb_extract_batch_device wrote
 * them.  Writes u_right / depth [n][cap_l] and kept[n].  Async on `stream`. */
int orb_compute_stereo_matches_batch_device(orb_extractor_t left, orb_extractor_t right, int n,
                                            const orb_keypoint_t* d_kps_l, const int32_t* d_counts_l,
                                            const uint8_t* d_desc_l, int cap_l, const orb_keypoint_t* d_kps_r,
                                            const int32_t* d_counts_r, const uint8_t* d_desc_r, int cap_r,
                                            float bf, float b, float* d_u_right, float* d_depth, int32_t* d_kept,
                                            void* stream);

/* ---- DBoW2 TemplatedVocabulary::transform (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1125-1260)
 * KeyFrame::ComputeBoW / Frame::ComputeBoW (src/KeyFrame.cc:109, src/Frame.cc:1010) call
 * mpORBvocabulary->transform(descriptors, mBowVec, mFeatVec, 4).  Per descriptor: descend the tree
 * from the root taking, at every level, the first child of minimal DescriptorDistance (FORB); the
 * leaf gives the word and its weight; the node passed at level L - levelsup is the FeatureVector
 * node.  TF_IDF / TF weighting: BowVector += weight per word (words with weight 0 are stop words
 * and skipped), then the scoring's normalisation (L1 for ORBvoc's L1_NORM).  The vocabulary is
 * given as flat arrays (ORBvoc.txt itself is not shipped with the reference: .MISSING_LARGE_BLOBS). */

typedef struct orb_vocabulary_view {
    int32_t k, L;                 /* m_k, m_L (the tree may be unbalanced) */
    int32_t weighting;            /* DBoW2 WeightingType: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY */
    int32_t scoring;              /* DBoW2 ScoringType: 0 L1_NORM, 1 L2_NORM, 2 CHI_SQUARE, 3 KL, 4 BHATTACHARYYA, 5 DOT_PRODUCT */
    int32_t n_nodes;              /* node 0 = root */
    const int32_t* child_begin;   /* n_nodes + 1: children of node i = child_idx[child_begin[i] .. child_begin[i+1]) in Node::children order */
    const int32_t* child_idx;
    const uint8_t* desc;          /* n_nodes x 32 bytes (the root's is unused) */
    const int32_t* word_id;       /* per node: WordId of a leaf, -1 for inner nodes */
    const double* weight;         /* per node: the leaf's WordValue */
} orb_vocabulary_view_t;

typedef struct orb_vocabulary_s* orb_vocabulary_t;

/* Upload a vocabulary (copied; the view may be freed afterwards). */
int orb_vocabulary_create(const orb_vocabulary_view_t* view, orb_vocabulary_t* out);
int orb_vocabulary_destroy(orb_vocabulary_t v);

/* transform() of n descriptors (host, n x 32 bytes).  Outputs, each with capacity n:
 * bow_word / bow_value (BowVector in ascending WordId order, *n_words entries), fv_node (FeatureVector
 * nodes ascending, *n_nodes entries), fv_begin (n_nodes + 1 offsets into fv_feat), fv_feat (feature
 * indices, ascending within a node).  Synchronous.  n <= 8192. */
int orb_bow_transform(orb_vocabulary_t v, const uint8_t* desc, int n, int levelsup, int32_t* bow_word,
                      double* bow_value, int32_t* n_words, int32_t* fv_node, int32_t* fv_begin, int32_t* fv_feat,
                      int32_t* n_nodes);
/* Device batch: frames f = 0..n_frames-1 hold descriptors d_desc[frame_begin[f] .. frame_begin[f+1])
 * (d_frame_begin: n_frames + 1 device ints, each frame <= 8192).  Per frame f the outputs start at
 * frame_begin[f] in every array (capacity = the frame's count; fv_begin: frame_begin[f] + f, with
 * count + 1 entries); d_counts[2 f] = n_words, d_counts[2 f + 1] = n_nodes.  Async on `stream`. */
int orb_bow_transform_batch_device(orb_vocabulary_t v, const uint8_t* d_desc, const int32_t* d_frame_begin,
                                   int n_frames, int n_total, int levelsup, int32_t* d_bow_word,
                                   double* d_bow_value, int32_t* d_fv_node, int32_t* d_fv_begin, int32_t* d_fv_feat,
                                   int32_t* d_counts, void* stream);
/* The same on the frames as orb_extract_batch_device leaves them: frame f's descriptors at
 * d_desc[f * cap * 32 ..], its count at d_kp_counts[2 f] (<= cap, <= 8192).  Per frame f the outputs
 * start at f * cap in every array (fv_begin at f * (cap + 1)); d_counts[2 f] = n_words,
 * d_counts[2 f + 1] = n_nodes.  A frame the extractor flagged (d_kp_counts[2 f + 1] ==
 * ORB_ERR_CAPACITY, or a count outside [0, cap]) is not read: both its counts are ORB_ERR_CAPACITY.
 * Async on `stream`. */
int orb_bow_transform_frames_device(orb_vocabulary_t v, const uint8_t* d_desc, const int32_t* d_kp_counts, int n_frames,
                                    int cap, int levelsup, int32_t* d_bow_word, double* d_bow_value, int32_t* d_fv_node,
                                    int32_t* d_fv_begin, int32_t* d_fv_feat, int32_t* d_counts, void* stream);

/* ---- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1740-2188) ----------------------------- */
/* The shim keeps the reference's graph gather (B1, src/Optimizer.cc:1744-1855) and the culling /
 * write-back (B10, :2107-2185) on the host and hands the flattened g2o problem across this ABI; the
 * library runs g2o's Levenberg-Marquardt (optimization_algorithm_levenberg.cpp:61-169) with the
 * BlockSolver_6_3 Schur complement (block_solver.hpp:354-486) on the GPU, FP64 throughout. */

typedef struct orb_ba_camera {  /* per keyframe: pKFi->fx, fy, cx, cy, mbf (floats upstream) */
    float fx, fy, cx, cy, bf;
} orb_ba_camera_t;

typedef struct orb_ba_edge {
    int32_t point;      /* index into the point arrays (vertex 0 of the g2o edge) */
    int32_t pose;       /* index into the pose arrays (vertex 1) */
    int32_t stereo;     /* 0: ORB_SLAM3::EdgeSE3ProjectXYZ (u, v), Huber sqrt(5.991);
                           1: g2o::EdgeStereoSE3ProjectXYZ (u, v, u_right), Huber sqrt(7.815) */
    float inv_sigma2;   /* pKFi->mvInvLevelSigma2[kpUn.octave]: information = I * inv_sigma2 */
    double obs[3];      /* measurement (obs[2] unused for mono edges) */
} orb_ba_edge_t;

typedef struct orb_ba_problem {
    int32_t n_poses, n_points, n_edges;
    double* pose;                         /* n_poses x 7, in/out: g2o::SE3Quat::toVector (tx ty tz qx qy qz qw) of Tcw */
    const int64_t* pose_id;               /* vertex ids (KeyFrame::mnId), unique */
    const uint8_t* pose_fixed;            /* 1 = setFixed(true) (the map's init KF and the fixed covisible KFs) */
    const orb_ba_camera_t* pose_camera;   /* n_poses */
    double* point;                        /* n_points x 3, in/out: world position */
    const int64_t* point_id;              /* vertex ids (MapPoint::mnId + maxKFid + 1), above every pose id */
    const orb_ba_edge_t* edges;           /* n_edges, in insertion (edge id) order */
} orb_ba_problem_t;

typedef struct orb_ba_options {
    int32_t iterations;                   /* optimizer.optimize(10) (src/Optimizer.cc:2101) */
    double user_lambda_init;              /* 0: tau * max diag(H) (tau = 1e-5); >0: setUserLambdaInit */
    const volatile int32_t* stop_flag;    /* pbStopFlag (polled between iterations and trials), may be NULL */
    const volatile uint8_t* stop_flag_bool;  /* the same for a C++ `bool* pbStopFlag` (one byte, nonzero = stop),
                                                as LocalMapping passes &mbAbortBA (src/LocalMapping.cc:208); may be NULL */
} orb_ba_options_t;

typedef struct orb_ba_result {
    int32_t iterations;       /* iterations run (SparseOptimizer::optimize's return value) */
    int32_t trials;           /* LM trials (linear solves) over all iterations */
    int32_t terminated;       /* 1 if the algorithm returned Terminate (no progress / 3 bad steps) */
    int32_t stopped;          /* 1 if the stop flag ended the run */
    double initial_chi2;      /* robust chi2 before the first update */
    double final_chi2;        /* robust chi2 of the accepted state */
    double lambda;            /* final LM damping */
} orb_ba_result_t;

typedef struct orb_ba_s* orb_ba_t;

int orb_ba_create(orb_ba_t* out);
int orb_ba_destroy(orb_ba_t h);

/* Optimise `problem` in place (poses and points).  edge_chi2[e] receives e->chi2() as the culling
 * pass reads it after optimize() (the error of the last evaluated state, robust kernel not applied)
 * and edge_depth_ok[e] e->isDepthPositive() for the final estimates (either may be NULL).
 * Returns ORB_OK, ORB_ERR_ABORTED if the stop flag was set before the first iteration, or an error. */
int orb_ba_optimize(orb_ba_t h, orb_ba_problem_t* problem, const orb_ba_options_t* options, double* edge_chi2,
                    uint8_t* edge_depth_ok, orb_ba_result_t* result);

/* ---- Optimizer::PoseOptimization (src/Optimizer.cc:55-415) ------------------------------------ */
/* Motion-only BA of tracking, batched over frames.  Per frame: one g2o::VertexSE3Expmap (Tcw) and a
 * unary edge per matched MapPoint -- ORB_SLAM3::EdgeSE3ProjectXYZOnlyPose (mono, Huber sqrt(5.991))
 * or g2o::EdgeStereoSE3ProjectXYZOnlyPose (mvuRight >= 0, Huber sqrt(7.815)) -- then 4 rounds of
 * optimize(10) with g2o's Levenberg-Marquardt and LinearSolverDense, each round restarting from the
 * frame's pose, re-classifying every edge by chi2 > 5.991 / 7.815 (the error of the last evaluated
 * state for active edges, recomputed for outliers), the robust kernels removed after round 2, and
 * the early exit when the frame has fewer than 10 edges.  Pinhole, single camera (mpCamera2 ==
 * NULL); the fisheye two-camera edge (EdgeSE3ProjectXYZOnlyPoseToBody) is not covered. */

typedef struct orb_pose_edge {
    double xw[3];        /* pMP->GetWorldPos().cast<double>() */
    double obs[3];       /* kpUn.pt.x, kpUn.pt.y, mvuRight[i] (stereo only) */
    float inv_sigma2;    /* mvInvLevelSigma2[kpUn.octave] */
    int32_t stereo;      /* mvuRight[i] >= 0 */
} orb_pose_edge_t;

typedef struct orb_pose_frame {
    double pose[7];          /* Tcw as g2o::SE3Quat::toVector (tx ty tz qx qy qz qw), in */
    orb_ba_camera_t cam;     /* fx, fy, cx, cy, mbf */
    int32_t edge_begin;      /* this frame's edges: edges[edge_begin, edge_begin + n_edges) */
    int32_t n_edges;         /* = nInitialCorrespondences */
} orb_pose_frame_t;

/* Host arrays, synchronous.  pose_out[7 f]: the optimised Tcw (unchanged when the frame has fewer
 * than 3 edges); outlier[e]: mvbOutlier of edge e after the last round; inliers[f]: the return value
 * of PoseOptimization (nInitialCorrespondences - nBad, 0 below 3 correspondences). */
int orb_pose_optimization(int n_frames, const orb_pose_frame_t* frames, int n_edges, const orb_pose_edge_t* edges,
                          double* pose_out, uint8_t* outlier, int32_t* inliers);
/* The same on device arrays, asynchronous on `stream` (one workgroup per frame). */
int orb_pose_optimization_device(int n_frames, const orb_pose_frame_t* d_frames, int n_edges,
                                 const orb_pose_edge_t* d_edges, double* d_pose_out, uint8_t* d_outlier,
                                 int32_t* d_inliers, void* stream);

/* ---- the device tracking chain's glue (Tracking::TrackWithMotionModel / TrackLocalMap,
 * src/Tracking.cc:4112-4217, 4234-4300) between the matchers and PoseOptimization, on device arrays.
 * PoseOptimization's graph for one device frame (src/Optimizer.cc:93-180): an edge per keypoint i < N
 * whose map point is d_match_b[i] (>= 0, a row of d_xyz_b) or else d_match_a[i] (a row of d_xyz_a), in
 * keypoint order; stereo when u_right[i] >= 0; information inv_level_sigma2[octave] (host, nlevels);
 * the camera from the frame view.  The start pose is d_pose (device, 7 doubles: the previous
 * optimisation's result) or else pose (host).  Writes *d_frame (edge_begin 0, n_edges = the count),
 * d_edges (up to cap) and d_edge_kp[e] = the keypoint of edge e.  d_match_b may be NULL. */
int orb_tracking_pose_edges_device(const orb_frame_device_t* frame, const int32_t* d_match_a, const float* d_xyz_a,
                                   const int32_t* d_match_b, const float* d_xyz_b, const float* inv_level_sigma2,
                                   const double* d_pose, const double pose[7], orb_pose_frame_t* d_frame,
                                   orb_pose_edge_t* d_edges, int32_t* d_edge_kp, void* stream);
/* TrackWithMotionModel's outlier discard (src/Tracking.cc:4180-4203): each edge PoseOptimization marked
 * an outlier clears its keypoint's map point in both match arrays; d_n_out[0] = the edges kept,
 * d_n_out[1] = those whose map point has observations (nmatchesMap; d_observed_a / _b per table row,
 * NULL = all observed).  d_match_b may be NULL.  d_taken (optional, cap entries): afterwards, whether
 * keypoint i holds a map point with observations -- SearchByProjection(F, local points)'s skip set. */
int orb_tracking_discard_outliers_device(const orb_pose_frame_t* d_frame, const int32_t* d_edge_kp,
                                         const uint8_t* d_outlier, int32_t* d_match_a, const uint8_t* d_observed_a,
                                         int32_t* d_match_b, const uint8_t* d_observed_b, int32_t* d_n_out, int cap,
                                         uint8_t* d_taken, void* stream);
/* SearchLocalPoints' skip of the map points the frame has seen (src/Tracking.cc:4745-4766, 4778, the
 * mnLastFrameSeen test): local map point j is the last frame's row d_last_row[j] (-1: not tracked by the
 * last frame); when a keypoint's d_match_a (cap entries: SearchByProjection(LastFrame)'s assignments
 * BEFORE the discard, since the discarded outliers are marked seen too, :4195) names that row,
 * d_in_view[j] (orb_is_in_frustum*_device's output) is cleared.  last_cap <= 16384. */
int orb_tracking_local_seen_device(const int32_t* d_match_a, int cap, int last_cap, const int32_t* d_last_row,
                                   int n_local, uint8_t* d_in_view, void* stream);

/* The whole chain in one call (the sequence above): SearchByProjection(F, LastFrame)
 * -> PoseOptimization -> isInFrustum at the new pose + the seen skip -> discard -> SearchByProjection(F,
 * local points) -> PoseOptimization, every stage async on `stream`.  The caller owns the per-frame
 * device buffers (sized for frame->cap; m1 / m2 and the pose outputs are the results) and the local
 * map's tracking-field arrays (local->track_* are written by the frustum stage).
 *
 * With params->motion_gate, TrackWithMotionModel's decisions run on the device with no host sync
 * (src/Tracking.cc:4149-4217): fewer than 20 matches -> the search again with 2 th; still fewer than 20
 * -> TrackWithMotionModel returns false: no PoseOptimization, no local-map stages; after the first
 * PoseOptimization and the discard, nmatchesMap < 10 -> it returns false too and the local-map stages
 * are skipped (the reference's Track() then runs TrackReferenceKeyFrame: orb_track_reference_kf_device
 * below).  The per-frame status word says which (ORB_TRACK_*).  For a frame that fails: m1 holds the last search's matches
 * (status FAIL_SEARCH: not discarded, no graph: n_edges 0, pose1 = the motion model's pose) or the
 * discarded ones (FAIL_MAP); m2 is all -1 and n_match[1] 0; the second graph is empty and pose2 is the
 * pose the Frame keeps after TrackWithMotionModel (pose1 through Frame::SetPose's float round trip);
 * the local map's track_* fields hold the frustum test at pose1 (no reference step reads them before
 * recomputing them). */
#define ORB_TRACK_RETRIED 1      /* the first search found < 20: the 2 th search ran */
#define ORB_TRACK_FAIL_SEARCH 2  /* < 20 matches after the retry: TrackWithMotionModel false */
#define ORB_TRACK_FAIL_MAP 4     /* nmatchesMap < 10 after PoseOptimization: TrackWithMotionModel false */
typedef struct orb_tracking_chain_params {
    float th_motion;            /* TrackWithMotionModel's th: 7 stereo, 15 otherwise (src/Tracking.cc:4141-4146) */
    int32_t mono;               /* bMono of SearchByProjection(F, LastFrame) */
    float th_local;             /* SearchLocalPoints' th (src/Tracking.cc:4801-4823) */
    int32_t far_points;         /* mpLocalMapper->mbFarPoints */
    float th_far_points;        /* mpLocalMapper->mThFarPoints */
    float viewing_cos_limit;    /* isInFrustum's 0.5 */
    int32_t motion_gate;        /* 1: TrackWithMotionModel's retry / failure decisions on the device (above);
                                   0: every stage runs on every frame with th_motion as given */
} orb_tracking_chain_params_t;

typedef struct orb_tracking_chain_buffers {
    int32_t* m1;                /* cap: SearchByProjection(LastFrame)'s last-frame row per keypoint, after the discard */
    int32_t* m2;                /* cap: SearchByProjection(local)'s local point per keypoint */
    int32_t* n_match;           /* 2: the two searches' counts */
    orb_pose_frame_t* frames;   /* 2: the two PoseOptimization graphs' frame records */
    orb_pose_edge_t* edges1;    /* cap */
    orb_pose_edge_t* edges2;    /* cap */
    int32_t* edge_kp1;          /* cap: keypoint of each edge */
    int32_t* edge_kp2;
    uint8_t* outlier1;          /* cap: mvbOutlier per edge */
    uint8_t* outlier2;
    double* poses;              /* 14: the two optimised poses (SE3Quat vectors) */
    int32_t* inliers;           /* 2: the two PoseOptimization returns */
    int32_t* n_out;             /* 2: nmatches after the discard, nmatchesMap */
    uint8_t* taken;             /* cap: SearchLocalPoints' skip set */
    void* scratch;              /* orb_tracking_chain_scratch_bytes(cap, last cap, local points), reused stage
                                   after stage on the stream (required) */
    int32_t* status;            /* 1: ORB_TRACK_* bits (0: tracked by the motion model); NULL: not reported */
} orb_tracking_chain_buffers_t;

/* Scratch bytes of one chain call for frames of `cap` keypoints, a last frame of `last_cap` and `n_local`
 * local map points (the largest of its stages'). */
size_t orb_tracking_chain_scratch_bytes(int cap, int last_cap, int n_local);

/* m_motion: ORBmatcher(0.9, true); m_local: ORBmatcher(0.8) (the handles' ratio / orientation).
 * local: the local map's view (track_* arrays written here); pos / normal / min_dist / max_dist:
 * GetWorldPos / GetNormal / mfMinDistance / mfMaxDistance per local point; last_row: -1 or the last
 * frame's row holding the point (NULL: none holds one).  frustum: the frame's bounds, camera, log scale
 * and levels (its pose fields are ignored).  pose7: the motion model's pose as PoseOptimization reads
 * it (tx ty tz qx qy qz qw of the frame's float pose; frame->Tcw must be the same pose). */
int orb_tracking_chain_device(orb_matcher_t m_motion, orb_matcher_t m_local, const orb_frame_device_t* frame,
                              const orb_last_points_device_t* last, const orb_local_points_device_t* local,
                              const float* d_pos, const float* d_normal, const float* d_min_dist,
                              const float* d_max_dist, const int32_t* d_last_row, const orb_frustum_frame_t* frustum,
                              const float* inv_level_sigma2, const double pose7[7],
                              const orb_tracking_chain_params_t* params, const orb_tracking_chain_buffers_t* bufs,
                              void* stream);

/* The chain over a batch of frames in one call: every stage is one launch for the whole batch (one
 * grid row per frame), so B frames cost one host crossing and ~20 launches instead of B of each, and
 * the frames' single-workgroup stages (the resolve, PoseOptimization) run side by side over the CUs.
 * Frame b's results are the single call's on the same inputs, bit for bit.  All frames share `cap`
 * (their frame views' cap); a last frame and a local map per frame; at most 65535 frames per call. */
typedef struct orb_tracking_chain_frame {
    const orb_frame_device_t* frame;
    const orb_last_points_device_t* last;
    const orb_local_points_device_t* local;   /* its track_* arrays are written */
    const float* pos;                         /* the local map's fields, as orb_tracking_chain_device */
    const float* normal;
    const float* min_dist;
    const float* max_dist;
    const int32_t* last_row;                  /* NULL: no local point is held by the last frame */
    const orb_frustum_frame_t* frustum;
    const float* inv_level_sigma2;            /* host, nlevels floats */
    double pose7[7];                          /* the motion model's pose (tx ty tz qx qy qz qw) */
} orb_tracking_chain_frame_t;

typedef struct orb_tracking_chain_batch_buffers {
    int32_t* m1;                /* B x cap */
    int32_t* m2;                /* B x cap */
    int32_t* n_match;           /* B x 2 */
    orb_pose_frame_t* frames;   /* 2 x B (B = the call's n_frames): the first graphs, then the second ones */
    orb_pose_edge_t* edges1;    /* B x cap (frame b's edges from b cap on) */
    orb_pose_edge_t* edges2;    /* B x cap */
    int32_t* edge_kp1;          /* B x cap */
    int32_t* edge_kp2;          /* B x cap */
    uint8_t* outlier1;          /* B x cap */
    uint8_t* outlier2;          /* B x cap */
    double* poses;              /* 2 x B x 7 (B = the call's n_frames) */
    int32_t* inliers;           /* 2 x B */
    int32_t* n_out;             /* B x 2 */
    uint8_t* taken;             /* B x cap */
    void* scratch;              /* orb_tracking_chain_batch_scratch_bytes(B, cap, max last cap, max local points) */
    int32_t* status;            /* B: ORB_TRACK_* bits per frame; NULL: not reported */
} orb_tracking_chain_batch_buffers_t;

size_t orb_tracking_chain_batch_scratch_bytes(int n_frames, int cap, int last_cap, int n_local);
/* Release the pinned host staging the batch calls keep for `scratch`: waits until the last call made
 * with it has finished on the device (every kernel, not only its argument copies), then frees the
 * staging; call it before the scratch or the call's output buffers are freed or reused for something
 * else.  A NULL or unknown scratch is a no-op.
 * Memory: the scratch holds, per frame, the SearchByProjection candidate lists (8 B per (point,
 * keypoint) pair: cap x max(last cap, local points) x 8 B) -- e.g. cap 2048 and 2048 points: 32 MiB per
 * frame, 16 GiB for 512 frames; orb_tracking_chain_batch_scratch_bytes gives the exact size. */
int orb_tracking_chain_batch_release(void* scratch);
int orb_tracking_chain_batch_device(orb_matcher_t m_motion, orb_matcher_t m_local, int n_frames,
                                    const orb_tracking_chain_frame_t* frames, const orb_tracking_chain_params_t* params,
                                    const orb_tracking_chain_batch_buffers_t* bufs, void* stream);

/* ---- Tracking::TrackReferenceKeyFrame (src/Tracking.cc:3931-4000) on device arrays, no host hop,
 * asynchronous on `stream`: where Tracking::Track hands a frame the motion model could not track (the
 * chain's ORB_TRACK_FAIL_SEARCH / ORB_TRACK_FAIL_MAP, the first frame after initialisation or a
 * relocalisation).  The caller has run Frame::ComputeBoW (orb_bow_transform_frames_device).
 *   SearchByBoW(mpReferenceKF, mCurrentFrame) with m = ORBmatcher(0.7, true)     -> match, n_match
 *   nmatches < 15: returns false -- status ORB_TRACK_REF_FAIL_BOW, no graph (n_edges 0), pose = pose7, the
 *     matches stay as the search left them, n_out 0 (a side flagged ORB_ERR_CAPACITY ends here too)
 *   PoseOptimization from the last frame's pose (pose7, an input): orb_tracking_pose_edges_device with
 *     d_match_a = match and d_xyz_a = d_xyz, then orb_pose_optimization_device         -> pose, outlier
 *   the outlier discard (:3966-3994, orb_tracking_discard_outliers_device with d_observed)  -> match, n_out
 *   nmatchesMap < 10 and not imu: status ORB_TRACK_REF_FAIL_MAP (imu: the IMU sensors return true, :3996)
 * kf / d_point_ok: as orb_search_by_bow_device.  d_observed, d_xyz: per keyframe feature, its map point's
 * Observations() > 0 (NULL: all) and GetWorldPos() (cap x 3).  frame_bow: the frame as SearchByBoW reads it;
 * frame: the same frame as PoseOptimization reads it (mvKeysUn, mvuRight, camera; the same cap).  The
 * status bits continue the ORB_TRACK_* word. */
#define ORB_TRACK_REF_FAIL_BOW 8   /* SearchByBoW found < 15: TrackReferenceKeyFrame false */
#define ORB_TRACK_REF_FAIL_MAP 16  /* nmatchesMap < 10 after PoseOptimization: TrackReferenceKeyFrame false */
typedef struct orb_track_reference_kf_buffers {
    int32_t* match;             /* cap: the keyframe feature whose map point keypoint i holds, after the discard */
    int32_t* n_match;           /* 1: SearchByBoW's return */
    orb_pose_frame_t* frame;    /* 1: the PoseOptimization graph's frame record */
    orb_pose_edge_t* edges;     /* cap */
    int32_t* edge_kp;           /* cap: keypoint of each edge */
    uint8_t* outlier;           /* cap: mvbOutlier per edge */
    double* pose;               /* 7: the optimised pose (SE3Quat vector) */
    int32_t* inliers;           /* 1: PoseOptimization's return */
    int32_t* n_out;             /* 2: nmatches after the discard, nmatchesMap */
    void* scratch;              /* orb_track_reference_kf_scratch_bytes(cap) (required) */
    int32_t* status;            /* 1: 0 (tracked) or an ORB_TRACK_REF_* bit; NULL: not reported */
} orb_track_reference_kf_buffers_t;

size_t orb_track_reference_kf_scratch_bytes(int cap);
int orb_track_reference_kf_device(orb_matcher_t m, const orb_kf_device_t* kf, const uint8_t* d_point_ok,
                                  const uint8_t* d_observed, const float* d_xyz, const orb_kf_device_t* frame_bow,
                                  const orb_frame_device_t* frame, const float* inv_level_sigma2, const double pose7[7],
                                  int imu, const orb_track_reference_kf_buffers_t* bufs, void* stream);

/* ---- Sim3Solver (src/Sim3Solver.cc; the loop / merge candidates of src/LoopClosing.cc:899-913) ----------
 * The RANSAC of Sim3Solver::iterate for n_problems candidates in one call: every hypothesis of every
 * problem is evaluated (ComputeSim3 + CheckInliers, :311-439) and the reference's serial control flow is a
 * selection over the counts.  Pinhole cameras only (fx * x / z + cx), like the rest of the library.
 *
 * One problem is what the Sim3Solver constructor gathers (:71-118): the camera-frame points mvX3Dc1 /
 * mvX3Dc2, the thresholds mvnMaxError1 / 2 = (float)(9.210 * sigma2) and the two cameras; the library
 * computes mvP1im1 / mvP2im2 itself.  The sample triples are an input: the reference draws them with
 * DUtils::Random::RandomInt, and that generator and its state belong to the caller (row h: the three
 * indices of iteration h, in draw order).
 *
 * Per hypothesis: Horn's closed form in FP64 on the float32 points, T12 and T21 rounded to float32 once;
 * the reprojections in float32 without contraction; inlier = err1 < max_err1[i] && err2 < max_err2[i], no
 * depth gate.  A hypothesis whose transform is not finite (|v| = 0: the two triples differ by a
 * translation) scores 0.  n < min_inliers (the reference's bNoMore on entry): nothing is evaluated, winner =
 * best = -1, inlier_mask zero, the per-hypothesis arrays are not written. */
typedef struct orb_sim3_problem {
    int32_t n;               /* correspondences, 0 .. 2^20 */
    const float* x3dc1;      /* n x 3: mvX3Dc1 */
    const float* x3dc2;      /* n x 3: mvX3Dc2 */
    const float* max_err1;   /* n: mvnMaxError1 */
    const float* max_err2;   /* n: mvnMaxError2 */
    float cam1[4], cam2[4];  /* fx, fy, cx, cy of pKF1's and pKF2's pinhole camera */
    int32_t fix_scale;       /* mbFixScale */
    int32_t min_inliers;     /* mRansacMinInliers */
    int32_t n_hyp;           /* mRansacMaxIts, 1 .. 1024 */
    const int32_t* samples;  /* n_hyp x 3 indices into 0 .. n-1, the three of a row distinct */
} orb_sim3_problem_t;

typedef struct orb_sim3_out {
    int32_t* hyp_inliers;    /* n_hyp: mnInliersi of every hypothesis (-1: invalid triple, device form only) */
    float* hyp_t12;          /* n_hyp x 12: mT12i's rows [s R | t] */
    float* hyp_scale;        /* n_hyp: ms12i */
    int32_t* winner;         /* 1: the first hypothesis with hyp_inliers > min_inliers, or -1 */
    int32_t* best;           /* 1: the last hypothesis attaining the maximum count (the reference updates its
                                best on >=), or -1 when nothing was evaluated */
    uint8_t* inlier_mask;    /* n: mvbInliersi of winner if there is one, else of best */
    uint64_t* hyp_mask;      /* n_hyp x ceil(n / 64) words, bit i & 63 of word i >> 6 = point i: every
                                hypothesis's inliers; NULL (production callers): not reported */
} orb_sim3_out_t;

/* Host pointers.  Every triple is checked: an index outside 0 .. n-1 or repeated in its row is ORB_ERR_ARG.
 * n_problems == 0: ORB_OK, nothing launched. */
int orb_sim3_ransac(const orb_sim3_problem_t* problems, int n_problems, const orb_sim3_out_t* outs);
/* Device pointers inside the (host) problem and output records, no host hop, asynchronous on `stream`.
 * The triples cannot be checked here: a row with an index out of range or repeated is not read, its
 * hypothesis reports hyp_inliers -1 and a NaN transform, and it is never selected. */
int orb_sim3_ransac_device(const orb_sim3_problem_t* problems, int n_problems, const orb_sim3_out_t* outs,
                           void* stream);

/* ---- The Sim3 problems of loop closing's BoW candidates (src/LoopClosing.cc:855-881, src/Sim3Solver.cc:71-118)
 * From the matches12 rows of orb_search_by_bow_kf[_device] (the current keyframe KF1 against every keyframe of
 * every candidate's window) to the arrays orb_sim3_problem_t takes, for n_cand candidates in one call.
 * Candidate c owns the pairs [group[c], group[c+1]) in window order j.  Map points are indices into one pool
 * (xyz, and an optional bad flag per point); a keyframe lists its features' points in mp_id (-1: NULL).
 *
 * The merge, exactly as :855-881: (j, k) in lexicographic order, a non-bad point not seen yet for the candidate
 * is inserted: num_bow[c]++ (numBoWMatches), matched_point[c][k] = its id (vpMatchedPoints), matched_pair[c][k]
 * = j (vpKeyFrameMatchedMP).  A later j that inserts another new point at the same k overwrites the slot and
 * the count keeps both: num_bow is the number of distinct points, not of filled slots.  pair_ok[p] = 0 (the
 * window keyframe is NULL or bad, :842) leaves pair p out.
 *
 * The gather, as the Sim3Solver constructor (:71-118) for every candidate whatever num_bow is (the gate of
 * LoopClosing.cc:889 is the caller's): in increasing k the slots with matched_point >= 0, ok1[k] set and the
 * matched point not bad.  indexKF1 = k and indexKF2 = the matched feature of pair matched_pair[c][k]: this
 * rests on the map's invariant that a keyframe lists a point at the index the point lists for the keyframe;
 * a caller that must honour GetIndexInKeyFrame < 0 passes obs_ok.  Entry i < n[c], in that order (the
 * caller's random triples index it): idx1 (mvnIndices1), x3dc1 = Rcw1 X1w + tcw1, x3dc2 = Rcw2[c] X2w + tcw2[c]
 * (the candidate's pose for every window keyframe's point, as the reference has it), max_err1 / 2 =
 * (float)(9.210 * sigma2) of the keypoint's octave in KF1 / in the matched window keyframe (a slot whose keypoint's
 * octave lies outside 0 .. nlevels-1 on either side, where the reference would read past mvLevelSigma2, is dropped
 * like one with obs_ok unset).  float32, each
 * component fma(r2, z, fma(r0, x, r1 * y)) + t, the order of the Sim3 searches.  Entries past n[c] hold idx1 -1
 * and zeros.  Row c of every per-slot output starts at c * stride (x3dc: 3 * c * stride): the pointers
 * x3dc1 + 3 c stride, ... go into orb_sim3_problem_t unchanged, with n = n[c]. */
typedef struct orb_loop_bow_kf {
    int32_t n;                  /* features (device form: the capacity): the bound of every index into the arrays */
    const int32_t* mp_id;       /* n: the feature's map point in the pool, -1 = NULL */
    const orb_keypoint_t* kps;  /* n: mvKeysUn (the octave is read) */
    const uint8_t* obs_ok;      /* n flags, NULL = all set: the point's GetIndexInKeyFrame(this keyframe) >= 0 */
    int32_t nlevels;            /* 1 .. 12 */
    float level_sigma2[12];     /* mvLevelSigma2 */
} orb_loop_bow_kf_t;

typedef struct orb_loop_bow_in {
    orb_loop_bow_kf_t kf1;          /* the current keyframe; kf1.n <= stride */
    const uint8_t* ok1;             /* kf1.n flags: map point non-NULL and not isBad(); NULL: from mp_id and bad */
    float Tcw1[12];                 /* 3x4 row-major [Rcw1 | tcw1] */
    int32_t n_pairs, n_cand;        /* <= 65535 each */
    const orb_loop_bow_kf_t* kf2s;  /* host array, n_pairs: the window keyframes, candidate after candidate */
    const uint8_t* pair_ok;         /* host array, n_pairs, or NULL (all set) */
    const int32_t* group;           /* host array, n_cand + 1: group[0] = 0 <= ... <= group[n_cand] = n_pairs */
    const float* Tcw2;              /* host array, n_cand x 12: the candidates' poses (pMostBoWMatchesKF = pKFi) */
    int32_t n_points;               /* the pool */
    const float* xyz;               /* n_points x 3: GetWorldPos() */
    const uint8_t* bad;             /* n_points flags (isBad()), NULL = none */
    const int32_t* matches12;       /* n_pairs x stride: row p = SearchByBoW(KF1, window keyframe p) */
    int32_t stride;                 /* C: the row length of matches12 and of every per-slot output, < 2^20 */
} orb_loop_bow_in_t;

typedef struct orb_loop_bow_out {
    int32_t* matched_point;  /* n_cand x stride */
    int32_t* matched_pair;   /* n_cand x stride: j, or -1 */
    int32_t* num_bow;        /* n_cand */
    int32_t* n;              /* n_cand: the problem's correspondences */
    int32_t* idx1;           /* n_cand x stride */
    float* x3dc1;            /* n_cand x stride x 3 */
    float* x3dc2;            /* n_cand x stride x 3 */
    float* max_err1;         /* n_cand x stride */
    float* max_err2;         /* n_cand x stride */
} orb_loop_bow_out_t;

/* Host form: mp_id, kps, obs_ok, ok1, xyz, bad, matches12 and the outputs are host arrays; synchronous, through
 * the handle's staging buffers.  Device form: those are device arrays (matches12 straight from
 * orb_search_by_bow_kf_device; the five tables marked `host array` stay on the host), asynchronous on `stream`,
 * no host hop: the caller reads n back, draws its triples and calls orb_sim3_ransac_device.  Every argument is
 * checked before anything is launched or written (ORB_ERR_ARG); the number of launches does not depend on
 * n_pairs or n_cand, and nothing the size of the pool is cleared. */
int orb_loop_bow_problems(orb_matcher_t m, const orb_loop_bow_in_t* in, const orb_loop_bow_out_t* out);
int orb_loop_bow_problems_device(orb_matcher_t m, const orb_loop_bow_in_t* in, const orb_loop_bow_out_t* out,
                                 void* stream);

/* ---- Optimizer::OptimizeSim3 (src/Optimizer.cc:4195-4494; called per loop / merge candidate at
 * src/LoopClosing.cc:689 and :991) ------------------------------------------------------------------------
 * The Levenberg-Marquardt refinement of S12 on one 7-DoF vertex with two reprojection edges per matched pair
 * (e12 = obs1 - project1(S12 P2c), e21 = obs2 - project2(S12^-1 P1c)), for n_problems candidates in one
 * call, FP64.  The whole schedule runs on the device: optimize(5) with Huber sqrt(th2), the first cull on the
 * stored errors (those of the last state the solver evaluated), the early return when fewer than 10 pairs are
 * left, optimize(10 or 5) without kernels, the second cull at the final estimate.  The edges are
 * differentiated numerically as g2o does (central differences, delta 1e-9).  Pinhole cameras only.
 *
 * One problem is the gathered graph (:4254-4407), one entry per pair that got its two edges, in gather order.
 * At most ORB_OPTSIM3_MAX_PAIRS pairs: the pairs live in the workgroup's LDS (88 bytes each); a larger n is
 * ORB_ERR_ARG. */
#define ORB_OPTSIM3_MAX_PAIRS 1024
typedef struct orb_optsim3_problem {
    int32_t n;                   /* nCorrespondences, 0 .. ORB_OPTSIM3_MAX_PAIRS */
    const double* p1c;           /* n x 3: P3D1c (float32 R1w X + t1w, cast to double) */
    const double* p2c;           /* n x 3: P3D2c */
    const double* obs1;          /* n x 2: mvKeysUn[i].pt of KF1 */
    const double* obs2;          /* n x 2: mvKeysUn[i2].pt of KF2, or the normalised (x / z, y / z) when i2 < 0 */
    const float* inv_sigma2_1;   /* n: information of e12 */
    const float* inv_sigma2_2;   /* n: information of e21 */
    float cam1[4], cam2[4];      /* fx, fy, cx, cy of pKF1's and pKF2's pinhole camera */
    double s12[8];               /* g2oS12 in g2o::Sim3::operator[] order: qx qy qz qw tx ty tz s */
    float th2;                   /* > 0 */
    int32_t fix_scale;           /* bFixScale */
} orb_optsim3_problem_t;

typedef struct orb_optsim3_out {
    double* s12_out;   /* 8: the refined g2oS12; the input when the call returns through the < 10 exit */
    int32_t* n_in;     /* 1: the reference's return value */
    int32_t* n_bad;    /* 1: nBad of the first cull */
    uint8_t* inlier;   /* n: 1 exactly where the reference leaves vpMatches1 set (NULL allowed when n == 0) */
    double* chi2_12;   /* n: each pair's last e12->chi2(): at the final estimate for the pairs that passed the
                          first cull, else as the first cull saw it; NULL: not reported */
    double* chi2_21;   /* n: the same for e21; NULL: not reported */
} orb_optsim3_out_t;

/* Host pointers, synchronous.  Arguments are checked before anything is touched.  n_problems == 0: ORB_OK,
 * nothing launched.  n == 0: n_in = n_bad = 0, s12_out = s12. */
int orb_optimize_sim3(const orb_optsim3_problem_t* problems, int n_problems, const orb_optsim3_out_t* outs);
/* Device pointers inside the (host) problem and output records, no host hop, asynchronous on `stream`. */
int orb_optimize_sim3_device(const orb_optsim3_problem_t* problems, int n_problems, const orb_optsim3_out_t* outs,
                             void* stream);

/* ---- multi-GPU local BA: one process per GPU, every rank passes the same
 * problem; rank r owns a contiguous, edge-balanced range of the landmarks and their edges, and
 * the ranks all-reduce the partial Hpp/b_p, the partial reduced camera system (S, b_S) of each LM
 * trial and the chi2 / scale partials.  Every rank factors S and updates the poses identically,
 * and the results of all ranks are identical. */
#define ORB_BA_SUM 0
#define ORB_BA_MAX 1
/* In-place all-reduce of n doubles in host memory across the ranks; returns 0 on success. */
typedef int (*orb_ba_host_reduce_fn)(void* ctx, double* host_buf, size_t n, int op);

/* ncclGetUniqueId of the RCCL loaded in the process (librccl.so.1); 128 bytes. */
int orb_ba_dist_unique_id(uint8_t id[128]);
/* Attach an RCCL communicator (ncclCommInitRank over `id`) to the handle: device all-reduces. */
int orb_ba_dist_init_rccl(orb_ba_t h, const uint8_t id[128], int world, int rank);
/* Attach a host-memory reducer instead (e.g. an MPI or gloo all-reduce). */
int orb_ba_dist_init_host(orb_ba_t h, orb_ba_host_reduce_fn fn, void* ctx, int world, int rank);

#ifdef __cplusplus
}
#endif

#endif /* ORBGPU_H */
