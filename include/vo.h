/*
 * vo.h — C-ABI of libvo, the MI355X-native stereo visual-odometry front end.
 *
 * Drop-in boundary.  The reference (ivario123/r7020e-visual-
 * odometry, MATLAB) has no native interface: its per-frame path calls
 * MathWorks toolbox functions from VO.m.  Each entry point below replaces one
 * of those calls; a MATLAB maintainer binds them through the MEX gateways
 * shown in INTEGRATION.md (path shadowing), a Python user through ctypes
 * (r7020e-visual-odometry_amd/vo.py).
 *
 *   entry point            replaces (reference call site)
 *   ---------------------  ---------------------------------------------------
 *   vo_undistort /         undistortImage(I, intrinsics)  VO.m:75-76 (Brown-Conrady
 *   vo_undistort_batch_dev remap, bilinear); vo_set_distortion puts it ahead of
 *   vo_set_distortion      the scale space of the loop-body entries
 *   vo_sift                detectSIFTFeatures + extractFeatures(...,"SIFT")
 *                          VO.m:79-84
 *   vo_describe /          extractFeatures(I, points, "Method", "SIFT") at points the caller
 *   vo_describe_batch      gives (VO.m:83-84 outside the fused path); vo_check_points is
 *   vo_check_points        their host-side argument check
 *   vo_set_strongest       points = selectStrongest(points, N) between the two
 *                          (VO.m:140,206,217-218), in every entry that detects
 *   vo_match               matchFeatures(F1, F2)  VO.m:87,283,293,311,323
 *   vo_match_ex /          [indexPairs, matchMetric] = matchFeatures(F1, F2,
 *   vo_match_f32_ex        'Unique', u, 'MatchThreshold', t, 'MaxRatio', r)
 *   vo_match_radius /      [indexPairs, matchMetric] = matchFeaturesInRadius(F1, F2, points2,
 *   vo_match_radius_f32    centerPoints, radius, ...): guided stereo / guided tracking
 *   vo_track               find_remaining_points  VO.m:280-334 (4 matches +
 *                          gathers), fused on device
 *   vo_triangulate         triangulate(x1, x2, P1, P2)  VO.m:113-116,
 *                          CreateLandmarksFromFeatures.m:7
 *   vo_triangulate_ex      [worldPoints, reprojectionErrors, validIndex] = triangulate(...):
 *   vo_fetch_track_quality the toolbox call's other two outputs, and the same two for the
 *                          loop's own triangulation of the tracked points (VO.m:113-116)
 *   vo_estworldpose        estworldpose(imagePts, worldPts, intrinsics)
 *                          VO.m:123-127 (P3P + MSAC)
 *   vo_refine_pose         bundleAdjustmentMotion(xyzPoints, imagePoints, absolutePose,
 *   vo_set_pose_refinement intrinsics) on estworldpose's pose and inliers (VO.m:123-130): as a
 *   vo_fetch_pose_refinement call, and as an optional stage of the loop body
 *   vo_est_fundamental /   estimateFundamentalMatrix(matchedPoints1, matchedPoints2, Method = "MSAC" |
 *   vo_est_fundamental_batch "Norm8Point"): the epipolar check of 2-D/2-D matches after matchFeatures
 *   vo_track_points /      vision.PointTracker (initialize on one image, step on the next): pyramidal
 *   vo_track_points_batch  Lucas-Kanade with MaxBidirectionalError, between frames or between the cameras
 *   vo_detect_corners /    detectMinEigenFeatures / detectHarrisFeatures(I, MinQuality, FilterSize, ROI):
 *   vo_detect_corners_batch cornerPoints for the tracker, without a scale space
 *   vo_disparity_sgm /     disparitySGM(I1, I2, DisparityRange = , UniquenessThreshold = ): dense
 *   vo_disparity_sgm_batch semi-global matching on a census cost
 *   vo_reconstruct_scene   reconstructScene(disparityMap, reprojectionMatrix): the dense scene
 *   vo_landmarks           new-landmark filter VO.m:145-158 +
 *                          CreateLandmarksFromFeatures.m:1-21
 *   vo_step / vo_step_batch the whole loop body VO.m:70-161 (features stay
 *                          device-resident between frames)
 *   vo_step_submit_dev /   the same loop body, pipelined: batch n+1's SIFT
 *   vo_step_collect        overlaps batch n's geometry and host pose chain
 *   vo_sift_match_batch    VO.m:79-87 for a batch of independent stereo pairs
 *                          (the benchmark workload, BASELINE.json configs[1])
 *   vo_sift_ex /           the same calls taking MATLAB's column-major storage
 *   vo_match_f32 /         (images, n x 128 single descriptors) without a host
 *   vo_step_batch_ex       transpose or conversion (zero-copy MEX gateways)
 *   vo_set_landmark_frame  sharded sequences: camera-frame landmark rows, moved
 *   vo_landmarks_to_world* to the world after the gathered pose chain
 *   vo_landmarks_world_dev (CreateLandmarksFromFeatures.m:17, VO.m:130; the
 *   vo_chain_poses         _dev form on the rank's own rows, on the device)
 *
 * Conventions
 *  - Return value: VO_OK (0) or a negative VO_ERR_* code.  vo_last_error()
 *    gives a message.  VO_ERR_TOO_FEW_POINTS / VO_ERR_NO_CONSENSUS mirror the
 *    errors estworldpose throws (the reference crashes; we report and the
 *    step holds the previous pose).
 *  - Buffers are caller-allocated host memory with explicit capacities, unless
 *    a function name ends in _dev (device pointers, stream-ordered).
 *  - Images: uint8, row-major with leading dimension `ld` (bytes per row).
 *    (MATLAB is column-major: the MEX shim passes the transpose view, see
 *    INTEGRATION.md.)
 *  - Image coordinates are MATLAB 1-based pixel coordinates (x = column).
 *  - Index pairs are 1-based uint32 [P][2] row-major, ascending in column 0,
 *    exactly as matchFeatures returns them.
 *  - Matrices are row-major doubles: P1/P2 3x4 premultiply camera matrices,
 *    K 3x3, rigid transforms 4x4 (R2022b rigidtform3d.A convention).
 *  - One context per device; a context is not thread-safe.
 */
#ifndef VO_H
#define VO_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VO_OK                  0
#define VO_ERR_ARG            -1
#define VO_ERR_HIP            -2
#define VO_ERR_TOO_FEW_POINTS -3
#define VO_ERR_NO_CONSENSUS   -4
#define VO_ERR_CAPACITY       -5
#define VO_ERR_STATE          -6

/* vo_step_out.flags / vo_pair_stats.flags: a capacity was exceeded and the frame's feature
 * sets are incomplete (results then differ from an uncapped run) */
#define VO_FLAG_KEYPOINTS   1    /* an image detected more than max_keypoints keypoints */
#define VO_FLAG_CANDIDATES  2    /* an image's extremum candidates exceeded 4 x max_keypoints */

#define VO_DESC_LEN 128
#define VO_MAX_BATCH 512         /* largest max_batch of vo_create */
#define VO_STEP_DEPTH 3          /* batches vo_step_submit_dev keeps in flight */

/* detectSIFTFeatures / extractFeatures defaults (MATLAB R2022b+).
 * contrast_threshold is in OpenCV units: MATLAB's ContrastThreshold 0.0133
 * equals 0.04 / NumLayersInOctave.
 *
 * Accepted ranges.  vo_create checks the block before any HIP call and returns NULL, with the
 * offending field named in vo_last_error(NULL), for anything else:
 *   n_octave_layers     1 .. 5.
 *   sigma               finite, > 0, and small enough that every blur of the scale space has a
 *                       kernel radius of at most 40 (VO_SIFT_MAX_RADIUS in vo_spec.h).  Level i
 *                       (1 .. n_octave_layers + 2) blurs with
 *                         s_i = sigma 2^((i - 1) / L) sqrt(2^(2 / L) - 1),  L = n_octave_layers,
 *                       at radius (round(8 s_i + 1) | 1) / 2; the top level binds:
 *                       sigma <= 1.45 at L = 1, 3.55 at L = 2, 5.2 at L = 3, 6.5 at L = 4,
 *                       7.7 at L = 5.  (The default sigma 1.6 is therefore refused at L = 1.)
 *   contrast_threshold  finite, >= 0.  The extremum pre-test uses floor(0.5 ct / L * 255), which is 0
 *                       below ct = 2 L / 255.
 *   edge_threshold      finite, > 0.
 *   upsample            0 or non-zero (non-zero: first octave is the x2 upsampled image).
 *   max_keypoints       >= 16.
 * Every accepted block gives the CPU specification's keypoints and descriptors bit for bit. */
typedef struct {
    int32_t n_octave_layers;      /* NumLayersInOctave, 3 */
    float   sigma;                /* Sigma, 1.6 */
    float   contrast_threshold;   /* 0.04  (= 0.0133 * 3) */
    float   edge_threshold;       /* EdgeThreshold, 10 */
    int32_t upsample;             /* 1: first octave is the x2 upsampled image */
    int32_t max_keypoints;        /* capacity per image (keypoints beyond it are dropped, flagged) */
} vo_sift_params;

/* matchFeatures defaults: Method Exhaustive, Metric SSD, MatchThreshold 1.0
 * (percent), MaxRatio 0.6, Unique false. */
typedef struct {
    float match_threshold;        /* percent; SSD threshold = 0.04 * match_threshold on unit vectors */
    float max_ratio;              /* 0.6 */
} vo_match_params;

/* estworldpose defaults (VO.m:123-127 calls it with no options: MaxNumTrials 1000).
 * The BASELINE configs[2] bench passes max_num_trials = 2048 explicitly. */
typedef struct {
    int32_t  max_num_trials;      /* 1000 (MATLAB default); hypothesis slots the context allocates */
    double   confidence;          /* percent, 99 */
    double   max_reprojection_error; /* pixels, 1 */
    uint32_t seed;                /* Philox key (frame index is mixed in by vo_step) */
} vo_ransac_params;

typedef struct {
    double P1[12];   /* left camera 3x4 (VO.m:27-29) */
    double P2[12];   /* right camera 3x4 (VO.m:30-32) */
    double K[9];     /* left intrinsics (VO.m:35-38,50) */
} vo_calib;

typedef struct {
    float   x, y;        /* Location, 1-based */
    float   size;        /* keypoint diameter in image pixels (OpenCV KeyPoint.size) */
    float   angle;       /* orientation in degrees [0,360) (OpenCV convention) */
    float   response;    /* |DoG| at the refined extremum (Metric) */
    int32_t octave;      /* octave index, -1 = upsampled */
    int32_t layer;       /* layer within octave 1..n_octave_layers (vo_describe takes 0..n_octave_layers + 2) */
    float   scale;       /* Scale = size / 2 in image pixels */
} vo_keypoint;

typedef struct vo_ctx vo_ctx;

/* Defaults for every parameter block. */
void vo_default_sift_params(vo_sift_params* p);
void vo_default_match_params(vo_match_params* p);
void vo_default_ransac_params(vo_ransac_params* p);

/* Create a context on HIP device `device` for images of rows x cols, able to
 * process up to max_batch (1..VO_MAX_BATCH) stereo frames per call.  calib may be NULL (then
 * vo_step/vo_landmarks are unavailable until vo_set_calib). Returns NULL on
 * failure (message via vo_last_error(NULL)). */
vo_ctx* vo_create(int device, int rows, int cols, int max_batch,
                  const vo_calib* calib, const vo_sift_params* sift,
                  const vo_match_params* match, const vo_ransac_params* ransac);
void vo_destroy(vo_ctx* ctx);
int  vo_set_calib(vo_ctx* ctx, const vo_calib* calib);
const char* vo_last_error(const vo_ctx* ctx);

/* detectSIFTFeatures + extractFeatures for one image (host buffers).
 * kps[capacity], desc[capacity][128] (uint8 values; MATLAB gets them as
 * single).  *n_out = number of keypoints (may exceed capacity: then only
 * `capacity` are written and VO_ERR_CAPACITY is returned). */
int vo_sift(vo_ctx* ctx, const uint8_t* img, int rows, int cols, int ld,
            vo_keypoint* kps, uint8_t* desc, int capacity, int* n_out);

/* The same for an image in MATLAB's own storage: col_major = 1 means pixel (r, c) at
 * img[c * ld + r] (ld >= rows; a MEX gateway passes mxGetUint8s(I) with ld = rows, no
 * transpose on the host; the device transposes).  col_major = 0 is vo_sift. */
int vo_sift_ex(vo_ctx* ctx, const uint8_t* img, int rows, int cols, int ld, int col_major,
               vo_keypoint* kps, uint8_t* desc, int capacity, int* n_out);

/* ---- extractFeatures at caller-given points ----------------------------- */
/* features = extractFeatures(I, points, "Method", "SIFT") for points the caller chose: detections
 * that were moved, rescaled or re-oriented, points of another detector, a grid, SIFTPoints built by
 * hand (OpenCV's compute() on provided keypoints, in this library's conventions).
 *
 * Spec.  For a context with SIFT block p (L = n_octave_layers) and a point q, only x, y, scale,
 * angle, octave and layer are read; size and response are ignored.
 *   o       = q.octave + (p.upsample ? 1 : 0)          plane index, 0 <= o < n_octaves
 *   oscale  = (float)(1 << o) * (p.upsample ? 0.5f : 1.0f)
 *   loc_off = p.upsample ? 0.75f : 1.0f
 *   xo = (q.x - loc_off) / oscale;  yo = (q.y - loc_off) / oscale;  scl = q.scale / oscale
 *   desc = descriptor(G(o, q.layer), xo, yo, q.angle, scl)
 * with descriptor() the arithmetic of the detecting entries, unchanged, on Gaussian level q.layer
 * of octave o (the level vo_fetch_gaussian returns).  This is the exact inverse of the mapping
 * vo_sift writes its keypoints with -- a power-of-two scaling and one rounding each way, and only
 * round(xo), round(yo) and scl enter the descriptor -- so describing vo_sift's own keypoints
 * reproduces vo_sift's descriptors (away from a .5 tie of xo or yo).
 *
 * Accepted points (anything else: VO_ERR_ARG naming the index of the first offending point,
 * decided on the host before anything is enqueued):
 *   - x, y, scale, angle finite, |x|, |y| < 2^20.  Points outside the image are legal: their
 *     windows hold fewer samples or none, and a window without a sample gives 128 zeros;
 *   - 0 <= angle <= 360;
 *   - 0 <= o < vo_num_octaves(rows, cols, upsample) and 0 <= layer <= L + 2: every level of the
 *     pyramid, not only the layers 1..L a detection has (SIFTPoints built by hand: layer 0);
 *   - the uncapped window radius round(VO_SIFT_DESCR_SCL * scl * sqrt(2)f * (VO_SIFT_DESCR_W + 1)
 *     * 0.5f) in 1 .. VO_SIFT_DESCR_RMAX = 127, about 0.1 <= scl <= 11.9.  The upper bound keeps
 *     vo_spec.h's proof that the u32 fixed-point bins cannot overflow: it counts the samples of a
 *     spatial bin from hist_width = 3 scl, which holds only while the cap at 127 does not bind.
 *     Where the image diagonal caps the radius instead (octave planes with (int)sqrt(rows^2 +
 *     cols^2) < 127) the plane has fewer than 8100 pixels and a bin cannot collect more samples
 *     than that: 8100 * 361 * 2^10 < 2^32.
 * n <= max_keypoints per image; beyond that VO_ERR_CAPACITY.
 *
 * vo_check_points is host-only and stateless (no context, no device): VO_OK, or VO_ERR_ARG with
 * *first_bad (may be NULL) = index of the first point that breaks a rule above; a NULL p or pts
 * (with n > 0), n < 0 or rows/cols < 1 give VO_ERR_ARG with *first_bad = -1. */
int vo_check_points(const vo_sift_params* p, int rows, int cols, const vo_keypoint* pts, int n, int* first_bad);
/* One image (host buffers, image conventions of vo_sift_ex): desc[n][128], row i for point i in
 * the caller's order.  n = 0 is legal and launches nothing (the context stays as it was).
 * The scale space runs as for vo_sift; no detection stage runs (no extremum test, refinement,
 * orientation, selection); the points become descriptor records on the device and one descriptor
 * launch sized for any accepted scale describes them.  vo_set_strongest and vo_set_distortion do
 * not apply (the points are already chosen; like vo_sift this replaces one toolbox call).  Refused
 * (VO_ERR_STATE) while step batches are pending; the loop state (features, pose, landmarks) is
 * untouched.  Afterwards vo_fetch_gaussian reads this call's scale space, while vo_fetch_keypoints,
 * vo_fetch_stereo_pairs, vo_fetch_candidate_counts and vo_fetch_detected_count -- results of a
 * detecting call -- return VO_ERR_STATE until the next call that detects. */
int vo_describe(vo_ctx* ctx, const uint8_t* img, int rows, int cols, int ld, int col_major,
                const vo_keypoint* pts, int n, uint8_t* desc);
/* The same for n_img images (1 .. 2 x max_batch) of the context's size laid out as vo_step_batch_ex
 * lays out frames (row-major: image i at imgs + i * rows * ld; col_major: at imgs + i * ld * cols).
 * Image i's points are pts + i * pts_stride, n_pts[i] <= pts_stride of them, its descriptors
 * desc + i * pts_stride * 128; rows beyond n_pts[i] are left untouched.  (VO.m:83-84 describes a
 * left and a right image: two images with their own counts.)  A refused point is reported as
 * "image i point k" in vo_last_error. */
int vo_describe_batch(vo_ctx* ctx, const uint8_t* imgs, int ld, int col_major, int n_img,
                      const vo_keypoint* pts, const int32_t* n_pts, int pts_stride, uint8_t* desc);

/* ---- undistortImage (VO.m:75-76) --------------------------------------- */
/* One camera's cameraIntrinsics: Brown-Conrady radial + tangential distortion.  The arithmetic
 * is spelled out in vo_spec.h (vo_undistort_pos / vo_undistort_u8): f64 sampling map, bilinear
 * taps, 0 outside the image, rint back to uint8 -- kitti.undistort bit for bit. */
typedef struct {
    double K[9];           /* this camera's intrinsics, row-major, K[1] = skew, K[3] = 0, last row 0 0 1;
                              principal point in 0-based pixel indices (MATLAB's PrincipalPoint - 1) */
    double radial[3];      /* k1 k2 k3  (cameraIntrinsics RadialDistortion; k3 = 0 for two) */
    double tangential[2];  /* p1 p2 */
} vo_distortion;

/* J = undistortImage(I, intrinsics) for host buffers: OutputView 'same', bilinear, FillValues 0.
 * rows / cols must be the context's (as for vo_sift_ex); img as vo_sift_ex takes it (col_major,
 * ld); out has the input's storage order with leading dimension ld_out, and the bytes of each of
 * its lines beyond cols (beyond rows for column-major storage) are left untouched.  VO_ERR_ARG:
 * a non-finite coefficient or K entry, fx or fy zero, K[3] non-zero, a last row other than 0 0 1,
 * mismatched sizes, ld / ld_out too small. */
int vo_undistort(vo_ctx* ctx, const uint8_t* img, int rows, int cols, int ld, int col_major,
                 const vo_distortion* d, uint8_t* out, int ld_out);
/* The same for B >= 1 tightly packed row-major device frames (rows*cols bytes each) of one
 * camera, stream-ordered on vo_stream(); d_out must not overlap d_in (VO_ERR_ARG). */
int vo_undistort_batch_dev(vo_ctx* ctx, const uint8_t* d_in, int B, const vo_distortion* d,
                           uint8_t* d_out);
/* VO.m:75-76 inside the loop body: once set, vo_step, vo_step_batch, vo_step_batch_ex,
 * vo_step_batch_dev, vo_step_submit_dev and vo_sift_match_batch_dev undistort every frame on the
 * device (one k_undistort launch per batch part, both cameras) ahead of the scale space.  vo_sift /
 * vo_sift_ex replace detectSIFTFeatures alone and do not.  A NULL side, or one whose five
 * coefficients are all zero, passes through; with both sides passing through nothing is launched
 * or allocated and every result is that of a context that never set a distortion.  The first
 * non-trivial call allocates the rectified frames (2 x max_batch x rows x cols bytes).
 * VO_ERR_STATE while step batches are pending. */
int vo_set_distortion(vo_ctx* ctx, const vo_distortion* left, const vo_distortion* right);
/* Diagnostic (like vo_fetch_gaussian): the undistorted image 2*frame + side of the last batched
 * call, rows*cols bytes row-major (capacity in bytes).  Synchronises like the other vo_fetch_*
 * calls.  VO_ERR_STATE when no distortion is set. */
int vo_fetch_rectified(vo_ctx* ctx, int image, uint8_t* out, int capacity);

/* points = selectStrongest(points, n) between detectSIFTFeatures and extractFeatures (the knob
 * VO.m:140, 206 name: "limit the number of points kept"; VO.m:217-218).  Per image: the detections
 * in detection order, stably sorted by response (Metric) descending -- the key is (response
 * descending, detection index ascending) -- and the first min(n, count) kept.  The result is in
 * sorted order also when n >= count.  The orientation peaks of one candidate share a response and
 * are consecutive, so a cut inside such a group keeps its first peaks.
 * n = 0 (the default) is off: nothing is launched and every result is that of a context that never
 * set it.  1 <= n <= max_keypoints turns it on for every entry that detects: vo_sift / vo_sift_ex
 * (it is a SIFTPoints operation, so unlike the distortion it applies there), vo_sift_match_batch_dev
 * and the vo_step* entries.  Only the n selected keypoints are described and matched; n_left /
 * n_right of vo_step_out and vo_pair_stats, vo_sift's *n_out and vo_fetch_keypoints' n are the
 * selected counts, while VO_FLAG_KEYPOINTS / VO_FLAG_CANDIDATES (and vo_sift's VO_ERR_CAPACITY)
 * still follow the detected counts.  Takes effect with the next call and keeps the loop state.  The
 * first n > 0 allocates the comparison keys (12 bytes per candidate slot).
 * VO_ERR_ARG for any other n, VO_ERR_STATE while step batches are pending; the setting is then
 * unchanged. */
int vo_set_strongest(vo_ctx* ctx, int n);
/* The keypoint count ahead of the selection of image 2*frame + side of the last call (with the
 * selection off: the count vo_fetch_keypoints reports).  Synchronises like the other vo_fetch_*. */
int vo_fetch_detected_count(vo_ctx* ctx, int image, int* n_detected);

/* matchFeatures(F1, F2) on SIFT descriptors (uint8 rows of 128).
 * pairs[capacity][2] 1-based; *n_pairs = matches found. */
int vo_match(vo_ctx* ctx, const uint8_t* F1, int n1, const uint8_t* F2, int n2,
             uint32_t* pairs, int capacity, int* n_pairs);

/* matchFeatures(F1, F2) on single-precision descriptor matrices exactly as MATLAB holds
 * extractFeatures' output (VO.m:83-87): n x 128 single with integer values 0..255.
 * col_major = 1: element (i, k) at F[i + k * ld] (MATLAB storage; ld >= n), so a MEX gateway
 * passes mxGetSingles(prhs[k]) with ld = n and no transpose or conversion; col_major = 0:
 * F[i * ld + k] (ld >= 128).  The matrices are copied to the device as they lie and packed to
 * u8 rows there.  Non-integer or out-of-range values -> VO_ERR_ARG.  Same results as vo_match. */
int vo_match_f32(vo_ctx* ctx, const float* F1, int n1, int ld1, const float* F2, int n2, int ld2,
                 int col_major, uint32_t* pairs, int capacity, int* n_pairs);

/* matchFeatures(F1, F2, 'MatchThreshold', t, 'MaxRatio', r, 'Unique', u) with the second
 * output: [indexPairs, matchMetric].
 *  - match_threshold in (0, 25] percent.  MATLAB allows up to 100; libvo stops at 25, where the
 *    SSD threshold 0.04f * 25 is exactly 1.0f: every accepted pair then has a cosine >= 0.5, the
 *    range in which SSD = 2 - 2c is exact and strictly decreasing, which the cosine-domain ranking
 *    of the match kernels relies on.  Larger values return VO_ERR_ARG.
 *  - max_ratio in (0, 1].
 *  - unique = 1 is the toolbox's findUniqueIndices rule (the forward-backward check): for every
 *    F2 row j, back(j) = the F1 row with the smallest SSD over ALL F1 rows (not only the accepted
 *    ones), the lowest row on ties; an accepted pair (i, j) is kept iff back(j) == i.
 *  - reserved must be 0. */
typedef struct {
    float   match_threshold;   /* percent, (0, 25] */
    float   max_ratio;         /* (0, 1] */
    int32_t unique;            /* 0 | 1 */
    int32_t reserved;          /* 0 */
} vo_match_opts;
void vo_default_match_opts(vo_match_opts* o);            /* 1.0, 0.6, 0, 0 */

/* vo_match / vo_match_f32 with options and matchMetric.  opts == NULL: the context's
 * vo_match_params, unique 0 -- the pairs are then exactly vo_match's / vo_match_f32's.  metric
 * (may be NULL) receives [capacity] floats: metric[k] is the SSD of pair k, the value the
 * thresholds were applied to (u8-valued rows: 2 - 2c of the exact-integer path; general single
 * features: the float SSD).  Errors as vo_match: VO_ERR_CAPACITY, empty sets allowed, refused
 * while step batches are pending. */
int vo_match_ex(vo_ctx* ctx, const uint8_t* F1, int n1, const uint8_t* F2, int n2, const vo_match_opts* opts,
                uint32_t* pairs, float* metric, int capacity, int* n_pairs);
int vo_match_f32_ex(vo_ctx* ctx, const float* F1, int n1, int ld1, const float* F2, int n2, int ld2, int col_major,
                    const vo_match_opts* opts, uint32_t* pairs, float* metric, int capacity, int* n_pairs);

/* ---- matchFeaturesInRadius ------------------------------------------------ */
/* [indexPairs, matchMetric] = matchFeaturesInRadius(features1, features2, points2, centerPoints,
 * radius, ...): matchFeatures whose candidates of F1 row i are only the F2 rows j whose point lies
 * in the closed circle of radius r_i about centre i -- guided stereo (a disparity range about the
 * left point) and guided tracking (about last frame's position or its reprojection).  The ratio
 * test runs over the candidates alone, so a repeated structure elsewhere in the image does not
 * kill the match; the result is not a filter of vo_match_ex's.
 *  - points2 [n2][2] and centers [n1][2] single (x, y); radius [n_radius], n_radius = 1 (one radius
 *    for every row) or n1.
 *  - scores: vo_match_ex's sv(i, j) = 2 - 2c, c = ((float)dot * inv|F1_i|) * inv|F2_j|.
 *  - candidates of row i: C_i = { j : d2(i, j) <= r2_i }, dx = x2_j - cx_i, dy = y2_j - cy_i,
 *    d2 = dx * dx + dy * dy, r2_i = r_i * r_i: float32 basic operations in this order, no fma
 *    (vo_spec.h: vo_radius_gate).  A point exactly on the circle is a candidate; a radius whose
 *    square overflows to +inf admits every column.
 *  - forward step: best and second-best sv over C_i (a multiset; ties -> lowest j).  No candidate:
 *    no pair.  One candidate: the second is +inf, the ratio 0, accepted iff best <= 0.04f *
 *    MatchThreshold.  An exact duplicate pair inside the circle gives 0 / 0 and fails, as in vo_match.
 *  - unique: back(j) = argmin_i sv(i, j) over the rows i with j in C_i (the same gate, bit for bit),
 *    lowest i on ties; an accepted (i, j) is kept iff back(j) == i.
 *  - pairs ascending in F1, 1-based; metric[k] = sv of pair k; opts as vo_match_ex (NULL: the
 *    context's vo_match_params, unique 0).
 * VO_ERR_ARG, before anything is enqueued and naming the first offending row: a non-finite
 * coordinate, a radius that is not finite and > 0, n_radius other than 1 or n1, bad opts.
 * n1 = 0 or n2 = 0 is legal (no pair).  VO_ERR_CAPACITY, VO_ERR_STATE while step batches are pending
 * and *n_pairs beyond capacity as vo_match_ex.
 * vo_match_radius_f32 takes the matrices as MATLAB holds them: col_major applies to the features
 * (ld1 / ld2, as vo_match_f32) and to the two point matrices (element (i, k) at P[i + k * n]).
 * Feature rows must hold integers in [0, 255]; any other single features -> VO_ERR_ARG. */
int vo_match_radius(vo_ctx* ctx, const uint8_t* F1, int n1, const uint8_t* F2, int n2,
                    const float* points2, const float* centers, const float* radius, int n_radius,
                    const vo_match_opts* opts, uint32_t* pairs, float* metric, int capacity, int* n_pairs);
int vo_match_radius_f32(vo_ctx* ctx, const float* F1, int n1, int ld1, const float* F2, int n2, int ld2, int col_major,
                        const float* points2, const float* centers, const float* radius, int n_radius,
                        const vo_match_opts* opts, uint32_t* pairs, float* metric, int capacity, int* n_pairs);

/* find_remaining_points (VO.m:280-334) on device.  old = previous frame's
 * stereo-aligned set (n_old rows, left/right row-aligned); cur = current
 * frame's full left (n_cl) / right (n_cr) sets.  Writes K row-aligned rows:
 * idx_out[K][3] = 1-based rows {old_row, cur_left_row, cur_right_row}
 * (old left and right stay row-aligned through VO.m:287-329), *K_out. */
int vo_track(vo_ctx* ctx,
             const uint8_t* old_l_desc, const uint8_t* old_r_desc, int n_old,
             const uint8_t* cur_l_desc, int n_cl, const uint8_t* cur_r_desc, int n_cr,
             uint32_t* idx_out, int capacity, int* K_out);

/* triangulate: n points, x1/x2 [n][2] float (1-based pixels), P1/P2 3x4
 * row-major -> X [n][3] double (values rounded through single, as MATLAB
 * returns single for single inputs). */
int vo_triangulate(vo_ctx* ctx, const float* x1, const float* x2, int n,
                   const double P1[12], const double P2[12], double* X);

/* ---- triangulate's reprojectionErrors and validIndex -------------------- */
/* [worldPoints, reprojectionErrors, validIndex] = triangulate(x1, x2, P1, P2): what a caller filters
 * triangulations with (VO.m's own crude form: CreateLandmarksFromFeatures.m:9-15 drops z < 0, z > 80).
 *
 * Spec (vo_spec.h vo_tri_quality, shared by the device and the CPU reference).  For point k with
 * X = (X0, X1, X2) the doubles vo_triangulate returns -- the single-rounded values the caller
 * sees, not the unrounded null vector, so both outputs can be reproduced from X, x1, x2, P1 and P2
 * alone -- and for view i with P = Pi and (u, v) = xi[k] widened to double, in f64 basic operations
 * in this order, no contraction:
 *   h0 = ((P[0]*X0 + P[1]*X1) + P[2]*X2) + P[3]
 *   h1 = ((P[4]*X0 + P[5]*X1) + P[6]*X2) + P[7]
 *   w  = ((P[8]*X0 + P[9]*X1) + P[10]*X2) + P[11]
 *   du = h0 / w - u;   dv = h1 / w - v;   e_i = sqrt(du*du + dv*dv)
 *   reproj_err[k] = (float)((e_1 + e_2) * 0.5)   mean reprojection distance over the two views, in
 *                                                pixels; single, as the toolbox returns for single points
 *   valid[k]      = (w_1 > 0) && (w_2 > 0)       the sign of each view's third homogeneous coordinate:
 *                                                for P = K [R t] the depth in that camera, the
 *                                                toolbox's "in front of both cameras"
 * Nothing is clamped.  A NaN w fails the comparison, so valid is 0; reproj_err is whatever IEEE
 * arithmetic gives: NaN or +-inf where X is not finite (a non-finite pixel coordinate, a point that
 * overflows single) or a w is 0.  A zero-disparity pair triangulates to a finite point beyond 1e17
 * on the side its rounding falls, with a small error.  A point behind the cameras (negative
 * disparity) reprojects perfectly -- only valid tells.
 *
 * reproj_err [n] and valid [n] may each be NULL; with both NULL this is vo_triangulate exactly.  X is
 * bit-equal to vo_triangulate's in every case.  Same chunk loop over max_keypoints rows, same
 * argument errors, refused (VO_ERR_STATE) while step batches are pending; n = 0 is legal and
 * launches nothing.  The first call that asks for either output allocates the context's quality
 * buffers (5 bytes per keypoint slot); a context that never asks allocates and launches nothing. */
int vo_triangulate_ex(vo_ctx* ctx, const float* x1, const float* x2, int n,
                      const double P1[12], const double P2[12],
                      double* X, float* reproj_err, uint8_t* valid);

/* estworldpose:img [n][2] double (1-based pixels), world [n][3] double,
 * K 3x3 -> T 4x4 camera pose in world (rigidtform3d.A), inliers[n] (0/1),
 * *n_inliers.  frame_key is mixed into the Philox key.  Returns
 * VO_ERR_TOO_FEW_POINTS (n < 4) or VO_ERR_NO_CONSENSUS like MATLAB throws. */
int vo_estworldpose(vo_ctx* ctx, const double* img, const double* world, int n,
                    const double K[9], const vo_ransac_params* params, uint32_t frame_key,
                    double T[16], uint8_t* inliers, int* n_inliers);

/* ---- bundleAdjustmentMotion: pose refinement after estworldpose --------- */
/* refinedPose = bundleAdjustmentMotion(xyzPoints, imagePoints, absolutePose, intrinsics), the call
 * the toolbox's stereo visual-odometry recipe makes right after estworldpose (VO.m:123-130 takes
 * estworldpose's pose as it is: the pose of the best three-point sample).  Motion-only bundle
 * adjustment: least squares on the squared pixel reprojection error over the used points, the
 * points held fixed, by Levenberg-Marquardt.
 *
 * Spec (vo_spec.h vo_refine_*, shared by the device and the CPU reference; f64, + - * / and sqrt in
 * the order written there, no contraction, so both give the same bytes):
 *  - the state is the extrinsics R, t (Xc = R X + t); T (rigidtform3d.A, as vo_estworldpose returns
 *    it) converts with R = T[0:3,0:3]', t = -R T[0:3,3] and back as vo_estworldpose builds its T;
 *  - used set U = { k : use[k] != 0 and zc_k > 0 at T_in }, fixed for the call; n_used = |U|;
 *  - a pass at a pose sums, over U, J'J (21 numbers), J'r (6) and r'r for the residual
 *    r = projection - img[k] (K upper triangular: fx, skew, cx, fy, cy) and its Jacobian under the
 *    left perturbation Xc' = Xc + w x Xc + v; a point of U with !(zc > 0) at that pose adds nothing
 *    and marks the pass `behind`.  Sums run in 64 partials (partial l: points k = l mod 64,
 *    ascending) joined by the tree p[i] += p[i + off], off = 32 .. 1;
 *  - a step solves (H + lambda diag(H)) d = -g by a 6x6 Cholesky (a pivot not > 0: no step,
 *    lambda *= 10) and retracts with the unit quaternion (1, w / 2) / sqrt(1 + |w|^2 / 4):
 *    R' = dR R, t' = dR t + v;
 *  - the loop makes one pass per trial while passes < max_iterations: the candidate is accepted iff
 *    its pass is not `behind` and its cost c' < c (then lambda = max(lambda / 10, 1e-12), and the loop
 *    ends CONVERGED when c - c' <= relative_tolerance * c or c' <= absolute_tolerance * n_used),
 *    otherwise lambda *= 10; lambda > 1e12 ends it with DAMPING, the pass budget with MAX_ITER.
 * cost_final <= cost_initial always, and the output is the last accepted pose; with no accepted step
 * (accepted == 0) T_out is T_in bit for bit.  n_used < 3 (TOO_FEW) and a non-finite first pass
 * (DEGENERATE) return the input pose; their one pass counts (passes = 1). */
#define VO_REFINE_CONVERGED   0
#define VO_REFINE_MAX_ITER    1
#define VO_REFINE_DAMPING     2
#define VO_REFINE_DEGENERATE -1
#define VO_REFINE_TOO_FEW    -3

typedef struct {
    int32_t max_iterations;      /* passes over the points, 1 .. 100; default 20 (MaxIterations) */
    double  relative_tolerance;  /* finite, >= 0; default 1e-9 (RelativeTolerance) */
    double  absolute_tolerance;  /* px^2 per used point, finite, >= 0; default 0 (AbsoluteTolerance) */
    double  lambda0;             /* first damping, 1e-12 .. 1e12; default 1e-3 */
} vo_refine_params;

typedef struct {
    int32_t status;              /* VO_REFINE_* */
    int32_t n_used, passes, accepted;
    double  cost_initial, cost_final;   /* sum of squared pixel residuals over U */
} vo_refine_stats;

void vo_default_refine_params(vo_refine_params* p);

/* img [n][2] double (1-based pixels), world [n][3] double, use [n] (NULL = all), K 3x3, T_in 4x4 the
 * pose to start from (vo_estworldpose's T) -> T_out 4x4, *stats (may be NULL).  p NULL = defaults.
 * Buffers and capacity as vo_estworldpose (frame slot 0 of buffer set 0; n > max_keypoints is
 * VO_ERR_CAPACITY; like the other standalone calls it ends the loop state of vo_step).
 * VO_ERR_ARG, checked on the host before anything is enqueued and naming the first offending
 * index: a non-finite value in img, world, K or T_in; a last row of T_in other than 0 0 0 1;
 * parameters outside the ranges above.  VO_ERR_STATE while step batches are pending.  n = 0 is
 * legal and launches nothing: T_out = T_in, TOO_FEW with n_used 0, passes 1, costs 0.
 * Returns VO_OK whenever it ran: the refinement's own outcome is stats->status. */
int vo_refine_pose(vo_ctx* ctx, const double* img, const double* world, int n, const uint8_t* use,
                   const double K[9], const double T_in[16], const vo_refine_params* p,
                   double T_out[16], vo_refine_stats* stats);

/* ---- estimateFundamentalMatrix: the epipolar check of 2-D/2-D matches ---- */
/* [F, inliersIndex, status] = estimateFundamentalMatrix(matchedPoints1, matchedPoints2,
 * Method = "MSAC" | "Norm8Point", NumTrials, DistanceThreshold, Confidence), the geometric filter a
 * feature pipeline applies right after matchFeatures.  Convention: [x2 1] F [x1 1]' = 0, F 3x3
 * row-major with unit Frobenius norm and F[8] >= 0; points are single 1-based pixels.
 *
 * Spec (vo_spec.h vo_fund_*, shared by the device and the CPU reference; f64, + - * / and sqrt in
 * the order written there, no contraction, so both give the same bytes):
 *  - a fit normalises each image's points (centroid c, mean distance d, s = sqrt(2) / d; a scale
 *    that is not finite: no model), sums the 45 entries of A'A for the rows
 *    [bx ax, bx ay, bx, by ax, by ay, by, ax, ay, 1], takes the eigenvector of its smallest
 *    eigenvalue by cyclic two-sided Jacobi (at most 30 sweeps; a pair is skipped when
 *    |a_pq| <= 2^-53 (|a_pp| + |a_qq|)), removes the smallest singular value with the smallest
 *    eigenvector v of Fh'Fh (F' = Fh - (Fh v) v'), denormalises (T2' F' T1), divides by the Frobenius
 *    norm and negates if F[8] < 0; a non-finite F: no model;
 *  - a sample's 8 points are summed sequentially in sample order; a fit over a mask in 64 partials
 *    (partial l: the used points k = l mod 64, ascending) joined by p[i] += p[i + off],
 *    off = 32 .. 1, in three passes (centroids, mean distances, the 45 sums);
 *  - the distance is Sampson's, in px^2; inlier iff d < distance_threshold (a NaN fails); the MSAC
 *    score is the sum of min(d, threshold) in the same 64 partials;
 *  - MSAC: slot s of the problem with key k draws 8 indices per attempt from two Philox4x32-10 calls
 *    (counter {s, attempt, k, 0xF8A70000 / 0xF8A70001}, key {seed, 0x9E3779B9}), up to 16 attempts
 *    for 8 distinct ones; a slot without a sample or without a model is no trial.  Slots are replayed
 *    in order, a strictly smaller score wins, and after each improvement the trial bound becomes
 *    min(bound, ceil(log(1 - conf) / log(1 - w^8))), w = n_in / n (log(1 - w^8) == 0: no bound);
 *  - the mask is the best slot's inliers and F the masked fit over it.
 * Status (the return value of the single call, status[f] of the batch): VO_OK; VO_ERR_TOO_FEW_POINTS
 * for n < 8 (the toolbox's status 1); VO_ERR_NO_CONSENSUS for no valid slot, fewer than 8 inliers or
 * a refit without a model (status 2) -- F and the mask are then 0.  VO_FUND_NORM8 is the masked fit
 * over all n points, no sampling (mask all 1).  RANSAC, LMedS, LTS and the algebraic distance are
 * not implemented: any other method is VO_ERR_ARG. */
#define VO_FUND_NORM8 0
#define VO_FUND_MSAC  1

typedef struct {
    int32_t  method;              /* VO_FUND_NORM8 or VO_FUND_MSAC (default) */
    int32_t  num_trials;          /* NumTrials, 1 .. 100000; default 500 */
    double   distance_threshold;  /* DistanceThreshold, px^2, finite and > 0; default 0.01 */
    double   confidence;          /* Confidence, percent, in (0, 100); default 99 */
    uint32_t seed;                /* Philox key word; default 0x5EED */
} vo_fund_params;

void vo_default_fund_params(vo_fund_params* p);

/* x1, x2 [n][2] single host buffers (as vo_triangulate takes them) -> F [9], inliers [n] (0/1, may be
 * NULL), *n_inliers (may be NULL).  params NULL = the defaults; key is mixed into the Philox counter
 * (a frame index, say).  Returns the status above.  VO_ERR_ARG, checked on the host before anything
 * is enqueued and naming the first offending row: a non-finite coordinate, parameters outside the
 * ranges above.  VO_ERR_CAPACITY for n > max_keypoints, VO_ERR_STATE while step batches are pending.
 * n < 8 launches nothing.  The first call that launches allocates the call's own buffers (17 bytes
 * per point, 6 KiB per problem); a context that never calls allocates and launches nothing.  The
 * loop state (features, pose, landmarks) and every other entry are untouched. */
int vo_est_fundamental(vo_ctx* ctx, const float* x1, const float* x2, int n, const vo_fund_params* params,
                       uint32_t key, double F[9], uint8_t* inliers, int* n_inliers);

/* B problems (0 .. max_batch) in one launch: problem f has n_pts[f] points (0 .. pts_stride) at
 * x1 / x2 + f * pts_stride * 2, pts_stride <= max_keypoints, and key key0 + f.  Outputs F [B][9],
 * inliers [B][pts_stride] (may be NULL; 0 beyond n_pts[f]), n_inliers [B] (may be NULL), status [B].
 * Problem f's outputs equal the single call's with key0 + f, by bytes.  Returns VO_OK when it ran
 * (per-problem outcomes are in status), or the refusals of the single call. */
int vo_est_fundamental_batch(vo_ctx* ctx, const float* x1, const float* x2, int pts_stride, const int32_t* n_pts, int B,
                             const vo_fund_params* params, uint32_t key0, double* F, uint8_t* inliers,
                             int32_t* n_inliers, int32_t* status);

/* ---- vision.PointTracker: pyramidal Lucas-Kanade point tracking ---- */
/* [points, validity, scores] = tracker(I) of a vision.PointTracker initialised on the first image:
 * every point is carried from img0 to img1 with sub-pixel precision, no second detection, and an
 * optional forward-backward test.  The toolbox's tracker is closed; the spec chosen here is the
 * algorithm of OpenCV 4.x calcOpticalFlowPyrLK in fixed point (vo_spec.h vo_klt_*, DESIGN 3.5.3,
 * shared by the device and the CPU reference, so both give the same bytes):
 *  - pyramid: u8 levels of (rows + 1) / 2 x (cols + 1) / 2, 5 x 5 binomial under reflect-101;
 *  - per level, coarse to fine, a bw x bh window: 14-bit bilinear weights, grey levels with 5
 *    fractional bits, Scharr derivatives, reads clamped to the level; the template's 2 x 2
 *    gradient matrix (flat iff minEig < 1e-4 or det < FLT_EPSILON), then up to max_iterations
 *    steps, stopping when |delta|^2 <= 1e-4 (EPS), when two successive steps cancel to 0.01 px
 *    (OSC, half a step back) or at the budget (MAXIT).  A window corner i is out iff i.x < -bw,
 *    i.x >= cols_l, i.y < -bh or i.y >= rows_l;
 *  - a template that is out or flat, or an iteration whose window is out, at a level above 0
 *    leaves the level's starting estimate as it was (levels_skipped counts them); at level 0 it
 *    ends the point.  After level 0 a result outside [0, cols - 1] x [0, rows - 1] is lost;
 *  - score = 1 - sqrt(SSD / (bw bh)) / 8160 from one more window pass at the result (0 for a point
 *    that is not valid) [EXT: the toolbox says only "based on SSD"];
 *  - with a finite max_bidirectional_error every forward-valid point is tracked back from its
 *    result, img1 -> img0, same parameters, no guess; valid iff that pass is valid and the
 *    distance to the original point is <= the maximum.
 * Points are single 1-based pixels, x = column.  A point that is not valid returns its input
 * position.  With img0 the left image, img1 the right one and guess = left - (d, 0) this is stereo
 * tracking. */
#define VO_KLT_OK 0            /* tracked */
#define VO_KLT_TEMPLATE_OUT 1  /* level-0 template window outside the admissible range */
#define VO_KLT_LOST 2          /* window left the level during the level-0 iterations, or the result left the image */
#define VO_KLT_FLAT 3          /* level-0 minEig / determinant test */
#define VO_KLT_BIDIR 4         /* back pass failed or bidirectional error above the maximum */
#define VO_KLT_STOP_NONE 0
#define VO_KLT_STOP_EPS 1
#define VO_KLT_STOP_OSC 2
#define VO_KLT_STOP_MAXIT 3

typedef struct {
    int32_t num_pyramid_levels;      /* 1 .. 6, default 3 (NumPyramidLevels) */
    int32_t block_size[2];           /* {height, width}, odd, 5 .. 31, default 31 31 (BlockSize) */
    int32_t max_iterations;          /* 1 .. 50, default 30 (MaxIterations) */
    float   max_bidirectional_error; /* > 0, or +inf (default): off (MaxBidirectionalError) */
} vo_klt_params;

/* stop and iterations are those of the forward pass at level 0; bidir_error is NaN unless the back
 * pass ran and was valid */
typedef struct { uint8_t status, stop, iterations, levels_skipped; float bidir_error; } vo_klt_info;

void vo_default_klt_params(vo_klt_params* p);

/* img0, img1: host images taken as vo_sift_ex takes them (rows x cols the context's; row-major with
 * row stride ld >= cols, or col_major with column stride ld >= rows).  pts0 [n][2], guess [n][2]
 * (may be NULL: start from pts0), params NULL = the defaults -> pts1 [n][2], valid [n], scores [n]
 * (may be NULL), info [n] (may be NULL).  VO_ERR_ARG, decided on the host before anything is
 * enqueued and naming the first offending point or field: a point or guess that is not finite or
 * has |x| or |y| >= 2^20, parameters outside the ranges above.  VO_ERR_CAPACITY for n >
 * max_keypoints, VO_ERR_STATE while step batches are pending.  n = 0 launches nothing.  The first
 * call that launches allocates the call's own buffers (pyramid planes of both images, points and
 * results; they grow to the largest batch seen); a context that never calls allocates and launches
 * nothing.  The loop state, have_features and every other entry are untouched. */
int vo_track_points(vo_ctx* ctx, const uint8_t* img0, const uint8_t* img1, int rows, int cols, int ld, int col_major,
                    const float* pts0, const float* guess, int n, const vo_klt_params* params, float* pts1, uint8_t* valid,
                    float* scores, vo_klt_info* info);

/* n_pairs (1 .. max_batch) pairs in one launch: imgs0 / imgs1 hold the pairs' first / second images
 * consecutively (as vo_describe_batch takes images); pair f has n_pts[f] points (0 .. pts_stride) at
 * pts0 / guess + f * pts_stride * 2, pts_stride <= max_keypoints.  Outputs [n_pairs][pts_stride];
 * rows beyond n_pts[f] are untouched.  Pair f equals the single call, by bytes. */
int vo_track_points_batch(vo_ctx* ctx, const uint8_t* imgs0, const uint8_t* imgs1, int ld, int col_major, int n_pairs,
                          const float* pts0, const float* guess, const int32_t* n_pts, int pts_stride,
                          const vo_klt_params* params, float* pts1, uint8_t* valid, float* scores, vo_klt_info* info);

/* diagnostic: level `level` of image 2 * pair + which (which 0: img0, 1: img1) of the last launching
 * track call -> out (tightly packed rows), *rows, *cols.  VO_ERR_STATE before such a call,
 * VO_ERR_CAPACITY (with *rows, *cols set) when capacity < rows * cols. */
int vo_fetch_klt_level(vo_ctx* ctx, int image, int level, uint8_t* out, int capacity, int* rows, int* cols);

/* ---- detectMinEigenFeatures / detectHarrisFeatures: cornerPoints ---- */
/* points = detectMinEigenFeatures(I, MinQuality = , FilterSize = , ROI = ) (Shi-Tomasi, the detector the
 * toolbox pairs with vision.PointTracker) and detectHarrisFeatures(...).  The toolbox's implementation is
 * closed; the spec chosen here (vo_spec.h vo_corner_*, DESIGN 3.5.4, shared by the device and the CPU
 * reference, so both give the same bytes):
 *  - central differences of the u8 image under replicate, their three products smoothed by the
 *    separable filter_size x filter_size Gaussian (sigma = filter_size / 3) in 12-bit integer weights:
 *    exact integers up to the response;
 *  - metric (f32, in the units of a [0, 1] image): the smaller eigenvalue of the smoothed matrix, or
 *    det - 0.04 trace^2 (Harris), in f64;
 *  - a corner is a pixel of the ROI with metric > min_quality * (the ROI's maximum metric) that is a
 *    local maximum of its 8 neighbours inside the image, the first of an equal pair winning [EXT: the
 *    toolbox uses imregionalmax]; a maximum that is not positive gives no corners;
 *  - Location = the pixel, 1-based (x = column), plus a per-axis parabolic offset in [-0.5, 0.5] (0 beside
 *    the image border); Metric = the pixel's metric [EXT: the toolbox reports the fitted peak];
 *  - corners come ascending in (row, column); with strongest = N > 0 the N strongest, metric descending,
 *    raster order ascending among equals (cornerPoints.selectStrongest(N)). */
#define VO_CORNER_MINEIG 0
#define VO_CORNER_HARRIS 1

typedef struct {
    int32_t method;        /* VO_CORNER_MINEIG (default) | VO_CORNER_HARRIS */
    int32_t filter_size;   /* odd, 3 .. 15, default 5 (FilterSize) */
    float   min_quality;   /* [0, 1], default 0.01 (MinQuality) */
    int32_t strongest;     /* 0 = all, else 1 .. max_keypoints */
    int32_t roi[4];        /* x y w h, 1-based (ROI); w = 0: whole image */
} vo_corner_params;

void vo_default_corner_params(vo_corner_params* p);

/* img: a host image taken as vo_sift_ex takes it (rows x cols the context's; row-major with row stride
 * ld >= cols, or col_major with column stride ld >= rows); params NULL = the defaults -> loc [capacity][2]
 * (x, y), metric [capacity], *n_out.  VO_ERR_ARG, decided on the host before anything is enqueued and
 * naming the field: a parameter outside the ranges above, an ROI with w or h < 1 or not inside the image.
 * VO_ERR_STATE while step batches are pending.  VO_ERR_CAPACITY with *n_out the true count and nothing
 * written: more corners than the device list holds (4 x max_keypoints), or more to return than
 * capacity.  The first call that launches allocates the call's own buffers (images, metric planes,
 * lists, maxima; they grow to the largest batch seen); a context that never calls allocates and launches
 * nothing.  The loop state, have_features and every other entry are untouched. */
int vo_detect_corners(vo_ctx* ctx, const uint8_t* img, int rows, int cols, int ld, int col_major, const vo_corner_params* params,
                      float* loc, float* metric, int capacity, int* n_out);

/* n_img (1 .. 2 x max_batch) consecutive images (as vo_describe_batch takes them) in one launch per kernel;
 * image i's results at loc + i * stride * 2, metric + i * stride, its count in n_out[i] and VO_OK or
 * VO_ERR_CAPACITY (as above, capacity = stride) in status[i]; rows beyond the count are untouched.  The
 * return value is VO_OK when the call ran, whatever the images' statuses.  Image i equals the single call,
 * by bytes. */
int vo_detect_corners_batch(vo_ctx* ctx, const uint8_t* imgs, int ld, int col_major, int n_img, const vo_corner_params* params,
                            float* loc, float* metric, int stride, int32_t* n_out, int32_t* status);

/* diagnostic: the metric plane of image `image` of the last launching call -> out [rows][cols].
 * VO_ERR_STATE before such a call, VO_ERR_CAPACITY when capacity < rows * cols. */
int vo_fetch_corner_metric(vo_ctx* ctx, int image, float* out, int capacity);

/* ---- disparitySGM / reconstructScene: dense stereo depth ---- */
/* disparityMap = disparitySGM(I1, I2, DisparityRange = , UniquenessThreshold = ) on a rectified pair (left
 * I1, right I2), then xyzPoints = reconstructScene(disparityMap, reprojectionMatrix).  The toolbox's
 * disparitySGM is closed; the spec chosen here (vo_spec.h vo_sgm_*, DESIGN 3.5.5, shared by the device
 * and the CPU reference, so both give the same bytes) is Hirschmueller's semi-global matching with the
 * toolbox's documented parameters, all integers up to the sub-pixel offset:
 *  - disparities d = min + k, k = 0 .. D - 1, D = max - min;
 *  - cost: the Hamming distance of 62-bit census words over a 7 x 9 window under replicate [EXT], the
 *    right image's column x - d clamped to the image;
 *  - eight paths with penalties p1 (a change of one disparity) and p2 (any other change) [EXT], summed;
 *  - the winner is the smallest sum, the lowest disparity among equals; with v the smallest sum more
 *    than one disparity away it is unreliable iff 100 v < (100 + uniqueness_threshold) * its sum (the
 *    toolbox's documented rule), invalid iff its column x - d lies outside the right image [EXT];
 *  - a parabola through the winner's neighbours gives the sub-pixel part (f32) [EXT];
 *  - an unreliable or invalid pixel is NaN, as the toolbox returns it.  No left-right check, no speckle
 *    filter, no median. */
#ifndef VO_SGM_GROUP
#define VO_SGM_GROUP 8            /* pairs a group; vo_spec.h defines it for a translation unit without this header */
#endif

typedef struct {
    int32_t disparity_range[2];   /* [min, max]; max - min in 8, 16, .. 128; -1024 <= min < max <= 1024; default 0 128 (DisparityRange) */
    int32_t uniqueness_threshold; /* 0 .. 100, default 15 (UniquenessThreshold) */
    int32_t p1, p2;               /* 0 <= p1 <= p2 <= 255, default 10 120 [EXT] */
} vo_sgm_params;

void vo_default_sgm_params(vo_sgm_params* p);

/* left, right: host images taken as vo_sift_ex takes them (rows x cols the context's; row-major with row
 * stride ld >= cols, or col_major with column stride ld >= rows); params NULL = the defaults -> disp, single
 * precision in the input's storage order with stride ld_out (>= cols, or >= rows for col_major; the padding
 * is left untouched).  VO_ERR_ARG, decided on the host before anything is enqueued and naming the field: a
 * parameter outside the ranges above.  VO_ERR_STATE while step batches are pending.  The first call that
 * launches allocates the call's own buffers (census words, the sums S -- 2 * rows * cols * D bytes a pair --
 * and the staging of a group); a context that never calls allocates and launches nothing.  The loop state,
 * have_features and every other entry are untouched. */
int vo_disparity_sgm(vo_ctx* ctx, const uint8_t* left, const uint8_t* right, int rows, int cols, int ld, int col_major,
                     const vo_sgm_params* params, float* disp, int ld_out);

/* n_pairs >= 1 consecutive pairs (lefts and rights each laid out as vo_track_points_batch takes its images)
 * -> disp [n_pairs][rows * cols], tightly packed in the input's storage order.  The pairs run in groups of
 * at most VO_SGM_GROUP, for which the workspace is sized.  Pair f equals the single call, by bytes. */
int vo_disparity_sgm_batch(vo_ctx* ctx, const uint8_t* lefts, const uint8_t* rights, int ld, int col_major, int n_pairs,
                           const vo_sgm_params* params, float* disp);

/* the same on device memory: d_lefts, d_rights [B][rows][cols] packed row-major -> d_disp [B][rows * cols]
 * row-major.  Stream-ordered on the context's stream (vo_stream), not synchronised. */
int vo_disparity_sgm_batch_dev(vo_ctx* ctx, const uint8_t* d_lefts, const uint8_t* d_rights, int B, const vo_sgm_params* params,
                               float* d_disp);

/* diagnostic: the sums S [rows][cols][D] of pair `pair` of the last launching call (of its last group: a
 * pair of an earlier group is VO_ERR_ARG).  VO_ERR_STATE before such a call, VO_ERR_CAPACITY when capacity
 * < rows * cols * D. */
int vo_fetch_sgm_cost(vo_ctx* ctx, int pair, uint16_t* S, long capacity);

/* the reprojection matrix Q (row-major 4 x 4, [X Y Z W]' = Q [x y d 1]') of a rectified pair from its 3 x 4
 * projection matrices (row-major, as VO.m:27-47 reads them): P = [fx 0 cx tx; 0 fy cy 0; 0 0 1 0] with
 * P1's tx = 0, P2's tx != 0 and equal fx, fy, cy; anything else is VO_ERR_ARG.  With b = -tx2 / fx and
 * s = fx / fy: Q = [1 0 0 -cx1; 0 s 0 -s cy; 0 0 0 fx; 0 0 1/b -(cx1 - cx2)/b].  Host only, stateless. */
int vo_reprojection_matrix(const double P1[12], const double P2[12], double Q[16]);

/* xyzPoints = reconstructScene(disparityMap, Q): disp as vo_disparity_sgm returns it (rows x cols the
 * context's, stride ld) -> xyz, tightly packed: [rows][cols][3] for row-major input, three column-major
 * planes (MATLAB's rows x cols x 3) for col_major.  Pixel (x, y), 1-based: h = Q [x y d 1]' in f64,
 * xyz = (float)(h(1:3) / h(4)); a NaN disparity gives three NaNs; nothing is clamped. */
int vo_reconstruct_scene(vo_ctx* ctx, const float* disp, int rows, int cols, int ld, int col_major, const double Q[16], float* xyz);

/* new-landmark filter (VO.m:145-158) + CreateLandmarksFromFeatures.
 * l_pos/r_pos [S][2] current stereo-matched locations; old_l/old_r [K][2]
 * remaining_old_features locations; pose 4x4 world pose.  Appends rows to
 * out[capacity][3]; *rows_out = rows appended (max(2, last kept odd index),
 * zero rows kept exactly as the reference does). */
int vo_landmarks(vo_ctx* ctx, const float* l_pos, const float* r_pos, int S,
                 const float* old_l, const float* old_r, int K,
                 const double pose[16], double* out, int capacity, int* rows_out);

/* ---- fused per-frame step (the VO.m loop body) ----------------------- */
typedef struct {
    int32_t status;          /* VO_OK, or VO_ERR_* for this frame (pose held) */
    int32_t n_left, n_right; /* detected keypoints */
    int32_t n_stereo;        /* stereo matches S (VO.m:87) */
    int32_t n_tracked;       /* K after find_remaining_points (0 on frame 1) */
    int32_t n_inliers;       /* MSAC inliers */
    int32_t n_landmarks;     /* landmark rows appended this frame */
    int32_t flags;           /* VO_FLAG_* capacity flags of this frame's two images */
    double  rel_pose[16];    /* rel_pose.A (identity on frame 1) */
    double  pose[16];        /* world pose after this frame (pose.A) */
} vo_step_out;

/* Process one stereo frame.  Keeps `features` (stereo subset) on device for
 * the next call.  Landmarks accumulate inside the context (vo_get_landmarks). */
int vo_step(vo_ctx* ctx, const uint8_t* left, const uint8_t* right, int ld, vo_step_out* out);

/* Process B consecutive frames (host buffers, B*rows*ld bytes each).  The
 * per-frame work is batched across frames on the GPU; only the 4x4 pose
 * chain is sequential (host).  Equivalent to B calls of vo_step. */
int vo_step_batch(vo_ctx* ctx, const uint8_t* lefts, const uint8_t* rights, int ld, int B,
                  vo_step_out* outs);
/* Same with a storage-order flag: col_major = 1 takes B column-major (MATLAB) frames, frame n
 * at lefts + n * ld * cols, pixel (r, c) at [c * ld + r]. */
int vo_step_batch_ex(vo_ctx* ctx, const uint8_t* lefts, const uint8_t* rights, int ld, int col_major, int B,
                     vo_step_out* outs);
/* Same, inputs already in device memory (tightly packed rows*cols each). */
int vo_step_batch_dev(vo_ctx* ctx, const uint8_t* d_lefts, const uint8_t* d_rights, int B,
                      vo_step_out* outs);

/* Pipelined form of vo_step_batch_dev (same results, bit for bit).  submit enqueues the
 * device half of B frames and returns; collect waits for the oldest submitted batch and
 * runs the host half (pose chain, landmark append), writing its B outputs.  Consecutive
 * batches alternate two buffer sets, so batch n+1's SIFT overlaps batch n's tracking /
 * MSAC / landmark kernels and the host work of collect(n); batch n+2's SIFT waits for batch
 * n's geometry on the device, not for collect(n).  At most VO_STEP_DEPTH (3) batches may be
 * pending (submit(n+3) needs collect(n) first); other calls on the context are refused
 * while any is pending.  Inputs of a submit made while another batch is pending must be
 * ready on the device at the call (the first submit is ordered after vo_stream()). */
int vo_step_submit_dev(vo_ctx* ctx, const uint8_t* d_lefts, const uint8_t* d_rights, int B);
int vo_step_collect(vo_ctx* ctx, vo_step_out* outs, int capacity, int* n);
int vo_steps_pending(const vo_ctx* ctx);

/* Visualisation data of frame `frame` of the most recently collected batch (valid until
 * that buffer set is reused, i.e. the next-but-one submit; VO_ERR_STATE once that batch is
 * submitted, so a driver that visualises keeps at most two batches pending): the tracked points'
 * previous-frame left positions, current left image points and triangulated world points
 * (remaining_old_features.l_pos / .pos of VO.m:106-116), and every current left detection
 * (l_pos, VO.m:79).  Any output pointer may be NULL. */
int vo_fetch_tracks(vo_ctx* ctx, int frame, float* old_l, float* cur_l, double* world, float* det, int capacity,
                    int* n_tracked, int* n_det);
/* The quality of the same tracked points: row k belongs to row k of vo_fetch_tracks for the same
 * frame.  old_r [capacity][2] is the right-image position of the old stereo pair (with old_l the
 * pair VO.m:113-116 triangulates into world[k]); reproj_err [capacity] and valid [capacity] are
 * vo_triangulate_ex's two outputs for world[k] from (old_l[k], old_r[k]) under the context's
 * calibration P1, P2 -- a quality measure for what goes into estworldpose.  The loop itself does not
 * use them: the kernel runs at this call, on the collected buffer set, and no step launches it.
 * State rules as vo_fetch_tracks: VO_ERR_STATE for a frame outside the last collected batch and
 * once that batch's buffer set is reused by a pending batch; any output pointer may be NULL;
 * *n_tracked is clamped to max_keypoints.  A frame without tracked points (frame 1) launches
 * nothing.  Synchronises like the other vo_fetch_* calls. */
int vo_fetch_track_quality(vo_ctx* ctx, int frame, float* old_r, float* reproj_err, uint8_t* valid,
                           int capacity, int* n_tracked);

/* bundleAdjustmentMotion as a stage of the loop body (VO.m:123-130).  With p non-NULL every entry
 * that runs the loop body (vo_step, vo_step_batch*, vo_step_submit_dev / vo_step_collect) launches
 * the refinement kernel after the MSAC kernel, on the same stream, for the batch's frames whose MSAC
 * status is VO_OK: vo_refine_pose on the frame's tracked points (vo_fetch_tracks' cur_l and world)
 * with the MSAC inlier mask as `use`, starting from the MSAC pose and replacing it.
 * vo_step_out.rel_pose and .pose are then the refined ones (the pose chain and the landmarks' world
 * transform follow); status, n_inliers and the mask stay MSAC's.  p NULL turns it off.  Off (the
 * default) launches and allocates nothing, and every result is that of a context that never set it.
 * The first non-NULL call allocates the per-frame stats (max_batch x 32 bytes per buffer set).
 * VO_ERR_ARG for parameters out of range, VO_ERR_STATE while step batches are pending; the setting
 * survives vo_reset. */
int vo_set_pose_refinement(vo_ctx* ctx, const vo_refine_params* p);
/* The refinement's stats of frame `frame` of the last collected batch.  State rules of
 * vo_fetch_tracks (VO_ERR_STATE for a frame outside that batch and once its buffer set is reused by
 * a pending batch); VO_ERR_STATE when that batch ran with the refinement off.  A frame whose MSAC
 * failed, or frame 1, was not refined: TOO_FEW with n_used 0, passes 0. */
int vo_fetch_pose_refinement(vo_ctx* ctx, int frame, vo_refine_stats* out);

/* Landmarks accumulated so far ([rows][3] double, world frame). */
int vo_get_landmarks(vo_ctx* ctx, double* out, int capacity, int* rows);

/* Sharded sequences: CreateLandmarksFromFeatures.m:17 transforms the
 * new points by the world pose, which a rank that starts mid-sequence does not know until
 * the relative poses of every earlier rank are gathered and chained.  With
 * vo_set_landmark_frame(ctx, 1) the context keeps each appended row in the CAMERA frame
 * instead: X [rows][3] float (the triangulated point, as CreateLandmarksFromFeatures.m:7
 * returns it) and keep[rows] (0 = one of the reference's zero rows, :2).  After the chain,
 * vo_landmarks_to_world applies :17 with the frame's world pose; the result equals the
 * world-frame rows a single-process run appends, bit for bit.  Mode 0 (default) = world rows
 * (vo_get_landmarks).  Changing the mode clears the accumulated rows.  Camera-frame rows stay
 * in device memory; vo_get_landmark_rows copies them to the host. */
int vo_set_landmark_frame(vo_ctx* ctx, int camera);
int vo_get_landmark_rows(vo_ctx* ctx, float* X, uint8_t* keep, int capacity, int* rows);
/* CreateLandmarksFromFeatures.m:17 on the device for the context's own camera-frame rows:
 * poses[f] (n_frames x 16 row-major double) is the chained world pose of the f-th frame the
 * context collected since vo_reset / vo_set_landmark_frame (n_frames must equal that count;
 * frames without rows, e.g. a shard's halo frame, still take a slot).  Writes the world rows
 * as float32 x, y, z to DEVICE memory d_out [capacity][3] -- the values are single-rounded,
 * so float32 holds exactly the doubles vo_landmarks_to_world returns; keep = 0 rows are the
 * reference's zero rows.  *rows = row count (d_out NULL: count only).  Synchronises the
 * context's stream before returning, so d_out is ready for any other stream (RCCL). */
int vo_landmarks_world_dev(vo_ctx* ctx, const double* poses, int n_frames, float* d_out, long capacity, long* rows);
/* Host-only, stateless: out[i] = keep[i] ? single(pose * [X[i]; 1]) : 0 (row-major 4x4 pose). */
int vo_landmarks_to_world(const double pose[16], const float* X, const uint8_t* keep, int n, double* out);
/* The same for a whole gathered sequence: frame f's rows_per_frame[f] consecutive rows with
 * poses[f] (n_frames x 16 row-major); sum(rows_per_frame) must equal n_rows. */
int vo_landmarks_to_world_frames(const double* poses, const int32_t* rows_per_frame, int n_frames, const float* X,
                                 const uint8_t* keep, long n_rows, double* out);
/* Host-only: the VO.m:130 world-pose chain over gathered relative poses (n x 16 row-major),
 * pose = pose * rel[f] for frames whose status is VO_OK (status NULL: every frame), the pose
 * after frame f into out[f]; pose0 NULL = identity.  Same arithmetic as vo_step_collect. */
int vo_chain_poses(const double* rel, const int32_t* status, int n, const double* pose0, double* out);
/* Reset loop state (features, pose, landmarks). */
int vo_reset(vo_ctx* ctx);
/* Global index of the next frame (the MSAC Philox key of frame i is
 * seed, frame i); a rank that starts a sequence shard at frame k sets k here. */
int vo_set_frame_index(vo_ctx* ctx, long frame_index);

/* ---- benchmark workload: SIFT + stereo match on B independent pairs ---- */
typedef struct {
    int32_t n_left, n_right, n_stereo, flags;   /* flags: VO_FLAG_* */
} vo_pair_stats;

/* Device buffers: d_lefts/d_rights are B tightly packed rows*cols images.
 * Stream-ordered on the context's stream; stats (host) are written after the
 * call completes (the call synchronises only when stats != NULL). */
int vo_sift_match_batch_dev(vo_ctx* ctx, const uint8_t* d_lefts, const uint8_t* d_rights, int B,
                            vo_pair_stats* stats);

/* Device-side results of the last batched call, for parity tests:
 * keypoints and descriptors of image i (2*frame + side) and stereo pairs of
 * a frame.  Host output buffers.  After vo_describe / vo_describe_batch, which detect nothing,
 * vo_fetch_keypoints, vo_fetch_stereo_pairs, vo_fetch_candidate_counts and vo_fetch_detected_count
 * return VO_ERR_STATE until the next detecting call; vo_fetch_gaussian reads the describe call's
 * scale space. */
int vo_fetch_keypoints(vo_ctx* ctx, int image, vo_keypoint* kps, uint8_t* desc, int capacity, int* n);
int vo_fetch_stereo_pairs(vo_ctx* ctx, int frame, uint32_t* pairs, int capacity, int* n);
/* Extremum candidates of image i in the last batched call (uncapped: above 4 x max_keypoints
 * the list was truncated, VO_FLAG_CANDIDATES) and how many passed refinement (contrast, edge
 * and the outer-level extremum test) -- the counts the feature kernels' byte model prices. */
int vo_fetch_candidate_counts(vo_ctx* ctx, int image, int* n_cand, int* n_accepted);
/* Gaussian scale-space level G(octave, level) of image i from the last batched
 * call (rows x cols floats, tightly packed; out == NULL only reports the size).
 * Diagnostic: the scale space has no MATLAB counterpart (detectSIFTFeatures
 * keeps it internal, VO.m:79-80); parity tests compare it with the oracle. */
int vo_fetch_gaussian(vo_ctx* ctx, int image, int octave, int level, float* out, int capacity, int* rows, int* cols);

/* HIP stream the context launches on (hipStream_t as void*), and per-kernel
 * timing over the last call (for bench.py's roofline; ms). */
void* vo_stream(vo_ctx* ctx);
int vo_set_profiling(vo_ctx* ctx, int enable);

/* Batch calls run SIFT in two phases on two internal streams forked from
 * vo_stream(): the scale space (bandwidth-bound) and the feature stages +
 * stereo matching (latency-bound).  vo_set_concurrency(n) additionally splits a
 * batch into n parts (1..4, default 1) so the features of part k overlap the
 * scale space of part k+1.  vo_sift_match_batch_dev without stats is
 * asynchronous: consecutive calls alternate between two buffer sets, so the
 * scale space of call N+1 overlaps the feature stages of call N; inputs are
 * read after earlier work on vo_stream() and must stay valid until the call
 * completes (vo_fetch_* / any synchronising call wait for it).  Results are
 * identical for any n and any call pattern. */
int vo_set_concurrency(vo_ctx* ctx, int n_streams);
int vo_kernel_times(vo_ctx* ctx, const char** names, double* ms, int* calls, int capacity, int* n);

#ifdef __cplusplus
}
#endif
#endif /* VO_H */
