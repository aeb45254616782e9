/*
 * vo_mex.c — MATLAB MEX gateway of libvo: the reference-side binding of the drop-in boundary.
 *
 * VO.m calls Computer Vision Toolbox functions; MATLAB resolves a name to the first match on
 * its path, so the `.m` files next to this gateway (undistortImage.m, detectSIFTFeatures.m,
 * extractFeatures.m, matchFeatures.m, matchFeaturesInRadius.m, triangulate.m, estworldpose.m, bundleAdjustmentMotion.m,
 * CreateLandmarksFromFeatures.m) shadow the
 * toolbox and the reference's own CreateLandmarksFromFeatures.m without editing VO.m.  Each
 * calls this one gateway with a command string:
 *
 *   J = vo_mex('undistort', I, cam, name, value, ...)
 *        undistortImage(I, intrinsics)                                   VO.m:75-76
 *        cam = [fx fy cx cy skew k1 k2 k3 p1 p2] (1 x 10 double) with cx, cy as MATLAB's
 *        PrincipalPoint (1-based: libvo gets cx - 1, cy - 1); an interpolation string and the
 *        options 'OutputView', 'FillValues' only at their defaults (vo:undistortImage:options)
 *   vo_mex('distortion', cam_l, cam_r)
 *        VO.m:75-76 inside the 'step' command: both cameras' cam rows ([] = none), kept for the
 *        session and applied to every context 'step' creates (vo_set_distortion)
 *   vo_mex('strongest', N)
 *        points = selectStrongest(points, N) between detectSIFTFeatures and extractFeatures
 *        (VO.m:140,206,217-218), in 'sift' and 'step': N kept for the session and applied to
 *        every context they create (vo_set_strongest); 0 = off
 *   [loc, scale, ori, metric, desc, octave, layer] = vo_mex('sift', I)
 *        detectSIFTFeatures + extractFeatures(..,"Method","SIFT")        VO.m:79-84
 *   desc = vo_mex('describe', I, loc, scale, ori, octave, layer)
 *        extractFeatures(I, points, "Method", "SIFT") at caller-given points (vo_describe): the
 *        SIFTPoints properties Location, Scale, Orientation (radians), Octave, Layer
 *   [indexPairs, matchMetric] = vo_mex('match', F1, F2, name, value, ...)
 *        matchFeatures(F1, F2)                                   VO.m:87,283,293,311,323
 *        and its options 'Unique', 'MatchThreshold', 'MaxRatio' (names case-insensitive; 'Method',
 *        'Metric', 'Prenormalized' only at their defaults; anything else: vo:matchFeatures:options)
 *   [indexPairs, matchMetric] = vo_mex('matchradius', F1, F2, points2, centerPoints, radius, name, value, ...)
 *        matchFeaturesInRadius(F1, F2, points2, centerPoints, radius): guided stereo / tracking; all
 *        five single; matchFeatures' options (vo:matchFeaturesInRadius:options)
 *   [X, reprojectionErrors, validIndex] = vo_mex('triangulate', x1, x2, P1, P2)
 *        triangulate                              VO.m:113-116, CreateLandmarksFromFeatures.m:7
 *        one output: vo_triangulate; two or three: vo_triangulate_ex (N x 1 single mean reprojection
 *        distance in pixels, N x 1 logical "in front of both cameras")
 *   [A, inliers, status] = vo_mex('estworldpose', imagePoints, worldPoints, K, opts)
 *        estworldpose (P3P + MSAC)                                       VO.m:123-127
 *   [refinedA, reprojectionErrors] = vo_mex('refinepose', xyzPoints, imagePoints, A, K, opts)
 *        bundleAdjustmentMotion(xyzPoints, imagePoints, absolutePose, intrinsics) right after
 *        estworldpose (VO.m:123-130): vo_refine_pose; M x 1 double pixel distances at the refined pose
 *   [F, inliersIndex, status] = vo_mex('fundamental', matchedPoints1, matchedPoints2, opts)
 *        estimateFundamentalMatrix(matchedPoints1, matchedPoints2, Method = "MSAC" | "Norm8Point"), the
 *        epipolar check right after matchFeatures: vo_est_fundamental; F 3 x 3 double with
 *        [x2 1] F [x1 1]' = 0, M x 1 logical, int32 status (0, 1 = fewer than 8 points, 2 = not enough inliers)
 *   [points, validity, scores] = vo_mex('trackpoints', I0, I1, points, opts)
 *        one step of a vision.PointTracker initialised with points on I0 and stepped to I1 (pyramidal
 *        Lucas-Kanade): vo_track_points; M x 2 single, M x 1 logical, M x 1 single (matlab/voPointTracker.m)
 *   [Location, Metric] = vo_mex('corners', I, opts)
 *        detectMinEigenFeatures / detectHarrisFeatures(I, MinQuality = , FilterSize = , ROI = ): vo_detect_corners;
 *        N x 2 single [x y] 1-based, N x 1 single (matlab/detectMinEigenFeatures.m, matlab/detectHarrisFeatures.m)
 *   disparityMap = vo_mex('disparitysgm', I1, I2, opts)
 *        disparitySGM(I1, I2, DisparityRange = , UniquenessThreshold = ) of a rectified pair: vo_disparity_sgm;
 *        rows x cols single, NaN where unreliable (matlab/disparitySGM.m)
 *   xyz = vo_mex('reconstructscene', disparityMap, Q)
 *        reconstructScene(disparityMap, reprojectionMatrix): vo_reconstruct_scene; rows x 3 cols single, the
 *        memory of MATLAB's rows x cols x 3 (matlab/reconstructScene.m reshapes it)
 *   rows = vo_mex('landmarks', features_l, features_r, P1, P2, A)
 *        CreateLandmarksFromFeatures.m:2-18 (the rows before the :20 append)
 *   [rel_A, A, status, nLandmarks] = vo_mex('step', Il, Ir, P1, P2)
 *        the whole loop body VO.m:70-161, `features` kept on the device
 *   L = vo_mex('landmarks_all'); vo_mex('reset'); vo_mex('close')
 *
 * Storage: MATLAB arrays are column-major and are handed to libvo as they lie wherever the
 * C-ABI takes a storage-order flag (images: vo_sift_ex / vo_step_batch_ex with col_major = 1,
 * ld = rows; N x 128 single descriptors: vo_match_f32 with col_major = 1, ld = N).  Small
 * matrices (points, 3x4 / 3x3 / 4x4) are transposed here into the ABI's row-major form.
 *
 * Errors: every libvo status becomes mexErrMsgIdAndTxt (which does not return); estworldpose's
 * two failures carry MATLAB-style identifiers, or come back as `status` (1 = not enough points,
 * 2 = not enough inliers: estworldpose's own codes) when the caller asks for that output.
 * One libvo context per MATLAB session (device 0), released by mexAtExit.
 *
 * Build in MATLAB:  mex -R2018a vo_mex.c -I<repo>/include -L<repo>/r7020e-visual-odometry_amd/lib -lvo
 * (tests/mex_shim builds this same file against a minimal mx-API for the test suite).
 */
#include "mex.h"
#include "vo.h"
#include <stdint.h>
#include <string.h>

#define VO_MEX_CAPACITY 16384            /* vo_sift_params.max_keypoints default */

static vo_ctx* g_ctx = NULL;
static int g_rows = 0, g_cols = 0;

/* vo_undistort / vo_set_distortion through weak references: a gateway linked with a libvo that
 * lacks them still loads and serves every other command; 'undistort' and 'distortion' then raise
 * vo:undistortImage:unavailable. */
extern __typeof__(vo_undistort) vo_undistort __attribute__((weak));
extern __typeof__(vo_set_distortion) vo_set_distortion __attribute__((weak));

/* vo_set_strongest likewise: without it 'strongest' raises vo:selectStrongest:unavailable */
extern __typeof__(vo_set_strongest) vo_set_strongest __attribute__((weak));

/* the 'strongest' command's N, applied to every context of the session (0 = off) */
static int g_strongest = 0;

/* the 'distortion' command's cameras, applied to every context of the session */
static vo_distortion g_dist[2];
static int g_has_dist[2] = {0, 0};

static void cleanup(void)
{
    if (g_ctx) vo_destroy(g_ctx);
    g_ctx = NULL;
    g_rows = g_cols = 0;
}

static void check(int rc)
{
    if (rc == VO_OK) return;
    if (rc == VO_ERR_TOO_FEW_POINTS)
        mexErrMsgIdAndTxt("vision:estworldpose:notEnoughPoints", "%s", vo_last_error(g_ctx));
    if (rc == VO_ERR_NO_CONSENSUS)
        mexErrMsgIdAndTxt("vision:estworldpose:notEnoughInliers", "%s", vo_last_error(g_ctx));
    if (rc == VO_ERR_ARG) mexErrMsgIdAndTxt("vo:badArgument", "%s", vo_last_error(g_ctx));
    if (rc == VO_ERR_CAPACITY) mexErrMsgIdAndTxt("vo:capacity", "%s", vo_last_error(g_ctx));
    mexErrMsgIdAndTxt("vo:error", "%s", vo_last_error(g_ctx));
}

/* The session's context.  Image commands need one of their image size (a new size replaces
 * the context and its loop state); the others run on whatever context exists. */
static void need_ctx(int rows, int cols)
{
    if (g_ctx && rows > 0 && (rows != g_rows || cols != g_cols)) cleanup();
    if (!g_ctx) {
        if (rows <= 0) { rows = 64; cols = 64; }          /* size-independent commands */
        g_ctx = vo_create(0, rows, cols, 1, NULL, NULL, NULL, NULL);   /* defaults = VO.m's (1000 MSAC trials) */
        if (!g_ctx) mexErrMsgIdAndTxt("vo:create", "%s", vo_last_error(NULL));
        g_rows = rows;
        g_cols = cols;
        mexAtExit(cleanup);
        if ((g_has_dist[0] || g_has_dist[1]) && vo_set_distortion) {
            const int rc = vo_set_distortion(g_ctx, g_has_dist[0] ? &g_dist[0] : NULL, g_has_dist[1] ? &g_dist[1] : NULL);
            if (rc != VO_OK) mexErrMsgIdAndTxt("vo:badArgument", "%s", vo_last_error(g_ctx));
        }
        if (g_strongest > 0 && vo_set_strongest && vo_set_strongest(g_ctx, g_strongest) != VO_OK)
            mexErrMsgIdAndTxt("vo:badArgument", "%s", vo_last_error(g_ctx));
    }
}

static void need_args(int nrhs, int want, const char* cmd)
{
    if (nrhs != want) mexErrMsgIdAndTxt("vo:nargin", "vo_mex('%s', ...) takes %d arguments, got %d", cmd, want - 1, nrhs - 1);
}

static void need_real(const mxArray* a, mxClassID cls, long rows, long cols, const char* what)
{
    if (mxGetClassID(a) != cls || mxIsComplex(a) || mxGetNumberOfDimensions(a) != 2)
        mexErrMsgIdAndTxt("vo:badArgument", "%s: wrong class or dimensions", what);
    if ((rows >= 0 && (long)mxGetM(a) != rows) || (cols >= 0 && (long)mxGetN(a) != cols))
        mexErrMsgIdAndTxt("vo:badArgument", "%s must be %ld x %ld", what, rows, cols);
}

/* r x c double matrix (column-major) -> row-major */
static void to_row_major(const mxArray* a, double* out, int r, int c, const char* what)
{
    need_real(a, mxDOUBLE_CLASS, r, c, what);
    const double* p = mxGetDoubles(a);
    for (int i = 0; i < r; ++i)
        for (int j = 0; j < c; ++j) out[i * c + j] = p[(size_t)j * r + i];
}

/* row-major 4x4 -> new MATLAB 4x4 double */
static mxArray* mat4_to_mx(const double* T)
{
    mxArray* m = mxCreateDoubleMatrix(4, 4, mxREAL);
    double* o = mxGetDoubles(m);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) o[j * 4 + i] = T[4 * i + j];
    return m;
}

/* n x k points, single or double, column-major -> row-major float (MATLAB Location is single) */
static float* points_f32(const mxArray* a, int k, int* n, const char* what)
{
    if ((!mxIsSingle(a) && !mxIsDouble(a)) || mxIsComplex(a) || mxGetNumberOfDimensions(a) != 2 ||
        ((int)mxGetN(a) != k && mxGetM(a) > 0))
        mexErrMsgIdAndTxt("vo:badArgument", "%s must be an N x %d single or double matrix", what, k);
    const int m = (int)mxGetM(a);
    float* v = (float*)mxMalloc(sizeof(float) * ((size_t)m * k + 1));
    if (mxIsSingle(a)) {
        const float* p = mxGetSingles(a);
        for (int i = 0; i < m; ++i) for (int j = 0; j < k; ++j) v[(size_t)i * k + j] = p[(size_t)j * m + i];
    } else {
        const double* p = mxGetDoubles(a);
        for (int i = 0; i < m; ++i) for (int j = 0; j < k; ++j) v[(size_t)i * k + j] = (float)p[(size_t)j * m + i];
    }
    *n = m;
    return v;
}

/* n x k double points, column-major -> row-major double */
static double* points_f64(const mxArray* a, int k, int n, const char* what)
{
    need_real(a, mxDOUBLE_CLASS, n, k, what);
    const double* p = mxGetDoubles(a);
    double* v = (double*)mxMalloc(sizeof(double) * ((size_t)n * k + 1));
    for (int i = 0; i < n; ++i) for (int j = 0; j < k; ++j) v[(size_t)i * k + j] = p[(size_t)j * n + i];
    return v;
}

/* calibration from the two 3x4 camera matrices VO.m:27-32 builds (K = P1(:, 1:3)) */
static vo_calib calib_from(const mxArray* P1, const mxArray* P2)
{
    vo_calib cal;
    to_row_major(P1, cal.P1, 3, 4, "P1");
    to_row_major(P2, cal.P2, 3, 4, "P2");
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) cal.K[3 * i + j] = cal.P1[4 * i + j];
    return cal;
}

static void cmd_sift(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    need_args(nrhs, 2, "sift");
    const mxArray* I = prhs[1];                       /* uint8 rows x cols, column-major */
    need_real(I, mxUINT8_CLASS, -1, -1, "I");
    const int rows = (int)mxGetM(I), cols = (int)mxGetN(I);
    need_ctx(rows, cols);
    const int cap = VO_MEX_CAPACITY;
    int n = 0;
    vo_keypoint* kp = (vo_keypoint*)mxMalloc(sizeof(vo_keypoint) * cap);
    uint8_t* d = (uint8_t*)mxMalloc((size_t)cap * VO_DESC_LEN);
    check(vo_sift_ex(g_ctx, mxGetUint8s(I), rows, cols, rows, 1, kp, d, cap, &n));
    plhs[0] = mxCreateNumericMatrix(n, 2, mxSINGLE_CLASS, mxREAL);      /* Location, 1-based [x y] */
    float* loc = mxGetSingles(plhs[0]);
    for (int i = 0; i < n; ++i) { loc[i] = kp[i].x; loc[(size_t)n + i] = kp[i].y; }
    if (nlhs > 1) {
        plhs[1] = mxCreateNumericMatrix(n, 1, mxSINGLE_CLASS, mxREAL);  /* Scale */
        for (int i = 0; i < n; ++i) mxGetSingles(plhs[1])[i] = kp[i].scale;
    }
    if (nlhs > 2) {
        plhs[2] = mxCreateNumericMatrix(n, 1, mxSINGLE_CLASS, mxREAL);  /* Orientation: radians */
        for (int i = 0; i < n; ++i) mxGetSingles(plhs[2])[i] = (float)((double)kp[i].angle * (3.14159265358979323846 / 180.0));
    }
    if (nlhs > 3) {
        plhs[3] = mxCreateNumericMatrix(n, 1, mxSINGLE_CLASS, mxREAL);  /* Metric */
        for (int i = 0; i < n; ++i) mxGetSingles(plhs[3])[i] = kp[i].response;
    }
    if (nlhs > 4) {
        plhs[4] = mxCreateNumericMatrix(n, VO_DESC_LEN, mxSINGLE_CLASS, mxREAL);   /* N x 128 single */
        float* D = mxGetSingles(plhs[4]);
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < VO_DESC_LEN; ++k) D[(size_t)k * n + i] = (float)d[(size_t)i * VO_DESC_LEN + k];
    }
    if (nlhs > 5) {
        plhs[5] = mxCreateNumericMatrix(n, 1, mxINT32_CLASS, mxREAL);   /* Octave */
        for (int i = 0; i < n; ++i) mxGetInt32s(plhs[5])[i] = kp[i].octave;
    }
    if (nlhs > 6) {
        plhs[6] = mxCreateNumericMatrix(n, 1, mxINT32_CLASS, mxREAL);   /* Layer */
        for (int i = 0; i < n; ++i) mxGetInt32s(plhs[6])[i] = kp[i].layer;
    }
    mxFree(kp);
    mxFree(d);
}

/* vo_describe through a weak reference as well: without it 'describe' raises
 * vo:extractFeatures:unavailable */
extern __typeof__(vo_describe) vo_describe __attribute__((weak));

/* n x 1 int32 or double column -> int32 values (SIFTPoints.Octave / .Layer are int32) */
static int32_t* column_i32(const mxArray* a, int n, const char* what)
{
    if ((mxGetClassID(a) != mxINT32_CLASS && !mxIsDouble(a)) || mxIsComplex(a) || mxGetNumberOfDimensions(a) != 2 ||
        (int)mxGetM(a) != n || ((int)mxGetN(a) != 1 && n > 0))
        mexErrMsgIdAndTxt("vo:badArgument", "%s must be an N x 1 int32 or double column", what);
    int32_t* v = (int32_t*)mxMalloc(sizeof(int32_t) * ((size_t)n + 1));
    for (int i = 0; i < n; ++i) {
        if (mxIsDouble(a)) {
            const double d = mxGetDoubles(a)[i];
            if (!(d >= -2147483648.0 && d <= 2147483647.0) || d != (double)(int32_t)d) {
                mxFree(v);
                mexErrMsgIdAndTxt("vo:badArgument", "%s must hold integers", what);
            }
            v[i] = (int32_t)d;
        } else {
            v[i] = mxGetInt32s(a)[i];
        }
    }
    return v;
}

/* desc = vo_mex('describe', I, loc, scale, ori, octave, layer): extractFeatures(I, points, "Method",
 * "SIFT") at caller-given points -- loc N x 2 [x y] 1-based, scale N x 1, ori N x 1 in radians as
 * SIFTPoints.Orientation (libvo takes degrees: (float)((double)ori * (180 / pi))), octave and layer
 * N x 1 -> N x 128 single, row i for point i.  vo_describe checks the values (vo:badArgument names
 * the first offending point). */
static void cmd_describe(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    (void)nlhs;
    need_args(nrhs, 7, "describe");
    const mxArray* I = prhs[1];
    need_real(I, mxUINT8_CLASS, -1, -1, "I");
    if (!vo_describe)
        mexErrMsgIdAndTxt("vo:extractFeatures:unavailable", "this libvo has no vo_describe: it describes only the points its own "
                          "detectSIFTFeatures returned; link a newer libvo");
    int n = 0, ns = 0, no = 0;
    float* loc = points_f32(prhs[2], 2, &n, "points.Location");
    float* scale = points_f32(prhs[3], 1, &ns, "points.Scale");
    float* ori = points_f32(prhs[4], 1, &no, "points.Orientation");
    if (ns != n || no != n) {
        mxFree(loc); mxFree(scale); mxFree(ori);
        mexErrMsgIdAndTxt("vo:badArgument", "Location, Scale and Orientation differ in length");
    }
    int32_t* octave = column_i32(prhs[5], n, "points.Octave");
    int32_t* layer = column_i32(prhs[6], n, "points.Layer");
    const int rows = (int)mxGetM(I), cols = (int)mxGetN(I);
    vo_keypoint* kp = (vo_keypoint*)mxMalloc(sizeof(vo_keypoint) * ((size_t)n + 1));
    for (int i = 0; i < n; ++i) {
        kp[i].x = loc[2 * i]; kp[i].y = loc[2 * i + 1];
        kp[i].scale = scale[i]; kp[i].size = scale[i] * 2.0f;
        kp[i].angle = (float)((double)ori[i] * (180.0 / 3.14159265358979323846));
        kp[i].response = 0.0f;
        kp[i].octave = octave[i]; kp[i].layer = layer[i];
    }
    mxFree(loc); mxFree(scale); mxFree(ori); mxFree(octave); mxFree(layer);
    uint8_t* d = (uint8_t*)mxMalloc((size_t)(n + 1) * VO_DESC_LEN);
    need_ctx(rows, cols);
    const int rc = vo_describe(g_ctx, mxGetUint8s(I), rows, cols, rows, 1, kp, n, d);
    if (rc != VO_OK) { mxFree(kp); mxFree(d); check(rc); }
    plhs[0] = mxCreateNumericMatrix(n, VO_DESC_LEN, mxSINGLE_CLASS, mxREAL);
    float* D = n ? mxGetSingles(plhs[0]) : NULL;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < VO_DESC_LEN; ++k) D[(size_t)k * n + i] = (float)d[(size_t)i * VO_DESC_LEN + k];
    mxFree(kp);
    mxFree(d);
}

/* vo_match_f32_ex through a weak reference: a gateway linked with a libvo that lacks the entry
 * still loads and serves matchFeatures(F1, F2); options and the second output then raise
 * vo:matchFeatures:options. */
extern __typeof__(vo_match_f32_ex) vo_match_f32_ex __attribute__((weak));

/* the function whose options match_options is parsing: its name, and the identifier of its errors */
static const char* g_opt_fn = "matchFeatures";
static const char* g_opt_id = "vo:matchFeatures:options";

static void bad_option(const char* why, const char* name)
{
    mexErrMsgIdAndTxt(g_opt_id, "%s: %s '%s' (libvo implements Unique, MatchThreshold in (0, 25], "
                      "MaxRatio in (0, 1] and the defaults of Method, Metric and Prenormalized)", g_opt_fn, why, name);
}

static int same_nocase(const char* a, const char* b)
{
    for (; *a && *b; ++a, ++b) {
        const int x = (*a >= 'A' && *a <= 'Z') ? *a + 32 : *a, y = (*b >= 'A' && *b <= 'Z') ? *b + 32 : *b;
        if (x != y) return 0;
    }
    return *a == *b;
}

/* real scalar of class logical / double / single (with any_numeric: also uint8, int32, uint32) */
static int scalar_value(const mxArray* a, int any_numeric, double* v)
{
    if (mxIsComplex(a) || mxGetM(a) != 1 || mxGetN(a) != 1) return 0;
    switch (mxGetClassID(a)) {
    case mxDOUBLE_CLASS: *v = mxGetDoubles(a)[0]; return 1;
    case mxSINGLE_CLASS: *v = (double)mxGetSingles(a)[0]; return 1;
    case mxLOGICAL_CLASS: if (!any_numeric) return 0; *v = mxGetLogicals(a)[0] ? 1.0 : 0.0; return 1;
    case mxUINT8_CLASS: if (!any_numeric) return 0; *v = (double)mxGetUint8s(a)[0]; return 1;
    case mxINT32_CLASS: if (!any_numeric) return 0; *v = (double)mxGetInt32s(a)[0]; return 1;
    case mxUINT32_CLASS: if (!any_numeric) return 0; *v = (double)mxGetUint32s(a)[0]; return 1;
    default: return 0;
    }
}

/* matchFeatures' name-value pairs prhs[first..] (matchFeaturesInRadius': the same rules): 1 if one
 * of Unique / MatchThreshold / MaxRatio is given (then *o holds them over the defaults).  Method,
 * Metric and Prenormalized are accepted only where they restate the default; anything else raises
 * g_opt_id (vo:matchFeatures:options, vo:matchFeaturesInRadius:options). */
static int match_options(int first, int nrhs, const mxArray* prhs[], vo_match_opts* o)
{
    int given = 0;
    o->match_threshold = 1.0f; o->max_ratio = 0.6f; o->unique = 0; o->reserved = 0;
    if ((nrhs - first) % 2) bad_option("a name without a value after", first == 3 ? "features2" : "radius");
    for (int k = first; k < nrhs; k += 2) {
        char name[32], text[32];
        double v = 0.0;
        const mxArray* val = prhs[k + 1];
        if (!mxIsChar(prhs[k]) || mxGetString(prhs[k], name, sizeof name)) bad_option("option name is not a short string:", "?");
        if (same_nocase(name, "Unique")) {
            if (!scalar_value(val, 1, &v)) bad_option("not a logical or numeric scalar:", name);
            o->unique = v != 0.0;
            given = 1;
        } else if (same_nocase(name, "MatchThreshold") || same_nocase(name, "MaxRatio")) {
            if (!scalar_value(val, 0, &v)) bad_option("not a double or single scalar:", name);
            if (same_nocase(name, "MaxRatio")) o->max_ratio = (float)v; else o->match_threshold = (float)v;
            given = 1;
        } else if (same_nocase(name, "Method") || same_nocase(name, "Metric")) {
            const char* dflt = same_nocase(name, "Method") ? "Exhaustive" : "SSD";
            if (!mxIsChar(val) || mxGetString(val, text, sizeof text) || !same_nocase(text, dflt))
                bad_option("only the default is implemented for", name);
        } else if (same_nocase(name, "Prenormalized")) {
            if (!scalar_value(val, 1, &v) || v != 0.0) bad_option("only the default is implemented for", name);
        } else {
            bad_option("unknown option", name);
        }
    }
    return given;
}

/* cam = [fx fy cx cy skew k1 k2 k3 p1 p2], 1 x 10 double, principal point 1-based (MATLAB's
 * PrincipalPoint) -> vo_distortion (0-based pixel indices) */
static void cam_row(const mxArray* a, vo_distortion* d, const char* what)
{
    need_real(a, mxDOUBLE_CLASS, 1, 10, what);
    const double* v = mxGetDoubles(a);
    memset(d, 0, sizeof(*d));
    d->K[0] = v[0]; d->K[1] = v[4]; d->K[2] = v[2] - 1.0;
    d->K[4] = v[1]; d->K[5] = v[3] - 1.0;
    d->K[8] = 1.0;
    d->radial[0] = v[5]; d->radial[1] = v[6]; d->radial[2] = v[7];
    d->tangential[0] = v[8]; d->tangential[1] = v[9];
}

static void bad_undistort_option(const char* why, const char* name)
{
    mexErrMsgIdAndTxt("vo:undistortImage:options", "undistortImage: %s '%s' (libvo implements bilinear interpolation, "
                      "OutputView 'same' and FillValues 0)", why, name);
}

/* undistortImage's trailing arguments prhs[3..]: an optional interpolation string ('linear' or
 * 'bilinear', the default) and name-value pairs, accepted only where they restate the default */
static void undistort_options(int nrhs, const mxArray* prhs[])
{
    char name[32], text[32];
    int k = 3;
    if (k < nrhs && mxIsChar(prhs[k]) && !mxGetString(prhs[k], name, sizeof name) &&
        (same_nocase(name, "linear") || same_nocase(name, "bilinear") || same_nocase(name, "nearest") ||
         same_nocase(name, "cubic") || same_nocase(name, "bicubic"))) {
        if (!same_nocase(name, "linear") && !same_nocase(name, "bilinear")) bad_undistort_option("interpolation", name);
        ++k;
    }
    if ((nrhs - k) % 2) bad_undistort_option("a name without a value after", "intrinsics");
    for (; k < nrhs; k += 2) {
        double v = 1.0;
        const mxArray* val = prhs[k + 1];
        if (!mxIsChar(prhs[k]) || mxGetString(prhs[k], name, sizeof name)) bad_undistort_option("option name is not a short string:", "?");
        if (same_nocase(name, "OutputView")) {
            if (!mxIsChar(val) || mxGetString(val, text, sizeof text) || !same_nocase(text, "same"))
                bad_undistort_option("only the default is implemented for", name);
        } else if (same_nocase(name, "FillValues")) {
            if (!scalar_value(val, 1, &v) || v != 0.0) bad_undistort_option("only the default is implemented for", name);
        } else {
            bad_undistort_option("unknown option", name);
        }
    }
}

/* J = vo_mex('undistort', I, cam, ...): the column-major uint8 image as it lies */
static void cmd_undistort(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    (void)nlhs;
    if (nrhs < 3) need_args(nrhs, 3, "undistort");
    const mxArray* I = prhs[1];
    need_real(I, mxUINT8_CLASS, -1, -1, "I");
    vo_distortion d;
    cam_row(prhs[2], &d, "intrinsics");
    undistort_options(nrhs, prhs);
    if (!vo_undistort)
        mexErrMsgIdAndTxt("vo:undistortImage:unavailable", "this libvo has no vo_undistort: undistort on the host, or link a newer libvo");
    const int rows = (int)mxGetM(I), cols = (int)mxGetN(I);
    need_ctx(rows, cols);
    plhs[0] = mxCreateNumericMatrix(rows, cols, mxUINT8_CLASS, mxREAL);
    check(vo_undistort(g_ctx, mxGetUint8s(I), rows, cols, rows, 1, &d, mxGetUint8s(plhs[0]), rows));
}

/* vo_mex('distortion', cam_l, cam_r): [] (0 x 0) = that camera passes through */
static void cmd_distortion(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    (void)nlhs;
    (void)plhs;
    need_args(nrhs, 3, "distortion");
    vo_distortion d[2];
    int has[2];
    for (int k = 0; k < 2; ++k) {
        has[k] = mxGetM(prhs[1 + k]) * mxGetN(prhs[1 + k]) != 0;
        if (has[k]) cam_row(prhs[1 + k], &d[k], k ? "intrinsics_r" : "intrinsics_l");
    }
    if (!vo_set_distortion)
        mexErrMsgIdAndTxt("vo:undistortImage:unavailable", "this libvo has no vo_set_distortion: undistort on the host, or link a newer libvo");
    if (g_ctx) check(vo_set_distortion(g_ctx, has[0] ? &d[0] : NULL, has[1] ? &d[1] : NULL));
    for (int k = 0; k < 2; ++k) {
        g_has_dist[k] = has[k];
        if (has[k]) g_dist[k] = d[k];
    }
}

/* vo_mex('strongest', N): N = 0 turns the selection off */
static void cmd_strongest(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    (void)nlhs;
    (void)plhs;
    need_args(nrhs, 2, "strongest");
    need_real(prhs[1], mxDOUBLE_CLASS, 1, 1, "N");
    const double v = mxGetDoubles(prhs[1])[0];
    if (!(v >= 0.0 && v <= (double)VO_MEX_CAPACITY) || v != (double)(int)v)
        mexErrMsgIdAndTxt("vo:badArgument", "N must be an integer in 0 .. %d", VO_MEX_CAPACITY);
    if (!vo_set_strongest)
        mexErrMsgIdAndTxt("vo:selectStrongest:unavailable", "this libvo has no vo_set_strongest: select on the host, or link a newer libvo");
    if (g_ctx) check(vo_set_strongest(g_ctx, (int)v));
    g_strongest = (int)v;
}

/* [indexPairs, matchMetric] = vo_mex('match', F1, F2, name, value, ...) */
static void cmd_match(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    if (nrhs < 3) need_args(nrhs, 3, "match");
    if (nlhs > 2) mexErrMsgIdAndTxt("vo:matchFeatures:options", "matchFeatures returns at most [indexPairs, matchMetric]");
    for (int k = 1; k <= 2; ++k)
        if (mxGetM(prhs[k]) > 0) need_real(prhs[k], mxSINGLE_CLASS, -1, VO_DESC_LEN, k == 1 ? "features1" : "features2");
    vo_match_opts opts;
    g_opt_fn = "matchFeatures";
    g_opt_id = "vo:matchFeatures:options";
    const int ex = match_options(3, nrhs, prhs, &opts) || nlhs > 1;
    if (ex && !vo_match_f32_ex)
        mexErrMsgIdAndTxt("vo:matchFeatures:options", "this libvo has no vo_match_f32_ex: matchFeatures(F1, F2) with the default "
                          "options and one output only");
    need_ctx(0, 0);
    const int n1 = (int)mxGetM(prhs[1]), n2 = (int)mxGetM(prhs[2]);
    int P = 0;
    uint32_t* pr = (uint32_t*)mxMalloc(sizeof(uint32_t) * 2 * ((size_t)n1 + 1));
    float* mt = (float*)mxMalloc(sizeof(float) * ((size_t)n1 + 1));
    /* N x 128 single exactly as extractFeatures returned it: col_major = 1, ld = N */
    const float* f1 = n1 ? mxGetSingles(prhs[1]) : NULL;
    const float* f2 = n2 ? mxGetSingles(prhs[2]) : NULL;
    if (ex) check(vo_match_f32_ex(g_ctx, f1, n1, n1 ? n1 : 1, f2, n2, n2 ? n2 : 1, 1, &opts, pr, mt, n1 + 1, &P));
    else check(vo_match_f32(g_ctx, f1, n1, n1 ? n1 : 1, f2, n2, n2 ? n2 : 1, 1, pr, n1 + 1, &P));
    plhs[0] = mxCreateNumericMatrix(P, 2, mxUINT32_CLASS, mxREAL);
    uint32_t* o = mxGetUint32s(plhs[0]);
    for (int i = 0; i < P; ++i) { o[i] = pr[2 * i]; o[(size_t)P + i] = pr[2 * i + 1]; }
    if (nlhs > 1) {
        plhs[1] = mxCreateNumericMatrix(P, 1, mxSINGLE_CLASS, mxREAL);      /* matchMetric */
        memcpy(mxGetSingles(plhs[1]), mt, sizeof(float) * (size_t)P);
    }
    mxFree(pr);
    mxFree(mt);
}

/* vo_match_radius_f32 through a weak reference: with a libvo that lacks it 'matchradius' raises
 * vo:matchFeaturesInRadius:unavailable and every other command runs as before */
extern __typeof__(vo_match_radius_f32) vo_match_radius_f32 __attribute__((weak));

/* [indexPairs, matchMetric] = vo_mex('matchradius', F1, F2, points2, centerPoints, radius, name, value, ...)
 * matchFeaturesInRadius: F1 n1 x 128 and F2 n2 x 128 single as extractFeatures returned them,
 * points2 n2 x 2 and centerPoints n1 x 2 single [x y], radius single, a scalar or n1 values -- all
 * handed over as they lie (col_major = 1).  Shapes are checked here (vo:badArgument), the values by
 * libvo; the options are matchFeatures' (vo:matchFeaturesInRadius:options). */
static void cmd_matchradius(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    if (nrhs < 6) need_args(nrhs, 6, "matchradius");
    if (nlhs > 2) mexErrMsgIdAndTxt("vo:matchFeaturesInRadius:options", "matchFeaturesInRadius returns at most [indexPairs, matchMetric]");
    for (int k = 1; k <= 2; ++k)
        if (mxGetM(prhs[k]) > 0) need_real(prhs[k], mxSINGLE_CLASS, -1, VO_DESC_LEN, k == 1 ? "features1" : "features2");
    const int n1 = (int)mxGetM(prhs[1]), n2 = (int)mxGetM(prhs[2]);
    need_real(prhs[3], mxSINGLE_CLASS, n2, 2, "points2");
    need_real(prhs[4], mxSINGLE_CLASS, n1, 2, "centerPoints");
    need_real(prhs[5], mxSINGLE_CLASS, -1, -1, "radius");
    const int nr = (int)(mxGetM(prhs[5]) * mxGetN(prhs[5]));
    if ((mxGetM(prhs[5]) != 1 && mxGetN(prhs[5]) != 1) || (nr != 1 && nr != n1))
        mexErrMsgIdAndTxt("vo:badArgument", "radius must be a scalar or hold one value per row of features1");
    vo_match_opts opts;
    g_opt_fn = "matchFeaturesInRadius";
    g_opt_id = "vo:matchFeaturesInRadius:options";
    match_options(6, nrhs, prhs, &opts);
    if (!vo_match_radius_f32)
        mexErrMsgIdAndTxt("vo:matchFeaturesInRadius:unavailable", "this libvo has no vo_match_radius_f32: match with matchFeatures "
                          "and filter by distance, or link a newer libvo");
    need_ctx(0, 0);
    int P = 0;
    uint32_t* pr = (uint32_t*)mxMalloc(sizeof(uint32_t) * 2 * ((size_t)n1 + 1));
    float* mt = (float*)mxMalloc(sizeof(float) * ((size_t)n1 + 1));
    const int rc = vo_match_radius_f32(g_ctx, n1 ? mxGetSingles(prhs[1]) : NULL, n1, n1 ? n1 : 1, n2 ? mxGetSingles(prhs[2]) : NULL, n2,
                                       n2 ? n2 : 1, 1, n2 ? mxGetSingles(prhs[3]) : NULL, n1 ? mxGetSingles(prhs[4]) : NULL,
                                       mxGetSingles(prhs[5]), nr, &opts, pr, mt, n1 + 1, &P);
    if (rc != VO_OK) { mxFree(pr); mxFree(mt); check(rc); }
    plhs[0] = mxCreateNumericMatrix(P, 2, mxUINT32_CLASS, mxREAL);
    uint32_t* o = mxGetUint32s(plhs[0]);
    for (int i = 0; i < P; ++i) { o[i] = pr[2 * i]; o[(size_t)P + i] = pr[2 * i + 1]; }
    if (nlhs > 1) {
        plhs[1] = mxCreateNumericMatrix(P, 1, mxSINGLE_CLASS, mxREAL);      /* matchMetric */
        memcpy(mxGetSingles(plhs[1]), mt, sizeof(float) * (size_t)P);
    }
    mxFree(pr);
    mxFree(mt);
}

/* vo_triangulate_ex through a weak reference: with a libvo that lacks it the one-output call runs
 * as before and [worldPoints, reprojectionErrors, validIndex] raises vo:triangulate:unavailable */
extern __typeof__(vo_triangulate_ex) vo_triangulate_ex __attribute__((weak));

/* [worldPoints, reprojectionErrors, validIndex] = vo_mex('triangulate', x1, x2, P1, P2) */
static void cmd_triangulate(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    need_args(nrhs, 5, "triangulate");
    if (nlhs > 3) mexErrMsgIdAndTxt("vo:badArgument", "triangulate returns at most [worldPoints, reprojectionErrors, validIndex]");
    if (nlhs > 1 && !vo_triangulate_ex)
        mexErrMsgIdAndTxt("vo:triangulate:unavailable", "this libvo has no vo_triangulate_ex: worldPoints = triangulate(...) only, "
                          "or link a newer libvo");
    int n = 0, n2 = 0;
    float* x1 = points_f32(prhs[1], 2, &n, "matchedPoints1");
    float* x2 = points_f32(prhs[2], 2, &n2, "matchedPoints2");
    if (n != n2) mexErrMsgIdAndTxt("vo:badArgument", "matchedPoints1 and matchedPoints2 differ in length");
    double P1[12], P2[12];
    to_row_major(prhs[3], P1, 3, 4, "cameraMatrix1");
    to_row_major(prhs[4], P2, 3, 4, "cameraMatrix2");
    need_ctx(0, 0);
    double* X = (double*)mxMalloc(sizeof(double) * 3 * ((size_t)n + 1));
    if (nlhs > 1) {
        float* err = (float*)mxMalloc(sizeof(float) * ((size_t)n + 1));
        uint8_t* ok = (uint8_t*)mxMalloc((size_t)n + 1);
        check(vo_triangulate_ex(g_ctx, x1, x2, n, P1, P2, X, err, nlhs > 2 ? ok : NULL));
        plhs[1] = mxCreateNumericMatrix(n, 1, mxSINGLE_CLASS, mxREAL);      /* reprojectionErrors */
        memcpy(mxGetSingles(plhs[1]), err, sizeof(float) * (size_t)n);
        if (nlhs > 2) {
            plhs[2] = mxCreateLogicalMatrix(n, 1);                           /* validIndex */
            mxLogical* L = mxGetLogicals(plhs[2]);
            for (int i = 0; i < n; ++i) L[i] = ok[i] != 0;
        }
        mxFree(err);
        mxFree(ok);
    } else {
        check(vo_triangulate(g_ctx, x1, x2, n, P1, P2, X));
    }
    plhs[0] = mxCreateNumericMatrix(n, 3, mxSINGLE_CLASS, mxREAL);     /* single, as for single inputs */
    float* o = mxGetSingles(plhs[0]);
    for (int i = 0; i < n; ++i) for (int a = 0; a < 3; ++a) o[(size_t)a * n + i] = (float)X[3 * i + a];
    mxFree(x1);
    mxFree(x2);
    mxFree(X);
}

/* opts (optional 5th argument): [MaxNumTrials Confidence MaxReprojectionError] double */
static void cmd_estworldpose(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    if (nrhs != 4 && nrhs != 5) need_args(nrhs, 4, "estworldpose");
    const int n = (int)mxGetM(prhs[1]);
    double* img = points_f64(prhs[1], 2, n, "imagePoints");
    double* wld = points_f64(prhs[2], 3, n, "worldPoints");
    double K[9], T[16];
    to_row_major(prhs[3], K, 3, 3, "intrinsics.K");
    need_ctx(0, 0);
    vo_ransac_params rp;
    vo_default_ransac_params(&rp);
    if (nrhs == 5) {
        need_real(prhs[4], mxDOUBLE_CLASS, 1, 3, "opts");
        const double* o = mxGetDoubles(prhs[4]);
        rp.max_num_trials = (int32_t)o[0];
        rp.confidence = o[1];
        rp.max_reprojection_error = o[2];
    }
    uint8_t* inl = (uint8_t*)mxMalloc((size_t)n + 1);
    int nin = 0;
    memset(inl, 0, (size_t)n + 1);
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
    const int rc = vo_estworldpose(g_ctx, img, wld, n, K, &rp, 0, T, inl, &nin);
    if (nlhs > 2 && (rc == VO_ERR_TOO_FEW_POINTS || rc == VO_ERR_NO_CONSENSUS)) {
        /* estworldpose's status output: 1 = not enough points, 2 = not enough inliers */
        plhs[2] = mxCreateDoubleScalar(rc == VO_ERR_TOO_FEW_POINTS ? 1.0 : 2.0);
        for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
        memset(inl, 0, (size_t)n + 1);
    } else {
        check(rc);
        if (nlhs > 2) plhs[2] = mxCreateDoubleScalar(0.0);
    }
    plhs[0] = mat4_to_mx(T);
    if (nlhs > 1) {
        plhs[1] = mxCreateLogicalMatrix(n, 1);
        mxLogical* L = mxGetLogicals(plhs[1]);
        for (int i = 0; i < n; ++i) L[i] = inl[i] != 0;
    }
    mxFree(img);
    mxFree(wld);
    mxFree(inl);
}

/* vo_refine_pose through a weak reference: with a libvo that lacks it 'refinepose' raises
 * vo:bundleAdjustmentMotion:unavailable and every other command runs as before */
extern __typeof__(vo_refine_pose) vo_refine_pose __attribute__((weak));
extern __typeof__(vo_default_refine_params) vo_default_refine_params __attribute__((weak));

/* sqrt(du^2 + dv^2) as the hardware instruction (no errno path: the gateway links no libm of its own) */
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("no-math-errno")))
#endif
static double pixel_norm(double du, double dv) { return __builtin_sqrt(du * du + dv * dv); }

/* [refinedPose, reprojectionErrors] = vo_mex('refinepose', xyzPoints, imagePoints, A, K, opts)
 * bundleAdjustmentMotion(xyzPoints, imagePoints, absolutePose, intrinsics) after estworldpose
 * (VO.m:123-130): xyzPoints M x 3 and imagePoints M x 2 double, A the 4 x 4 absolutePose.A, K 3 x 3;
 * opts (optional) = [MaxIterations AbsoluteTolerance RelativeTolerance] double.  reprojectionErrors:
 * M x 1 double, each point's pixel distance at the refined pose, computed here from the outputs. */
static void cmd_refinepose(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    if (nrhs != 5 && nrhs != 6) need_args(nrhs, 5, "refinepose");
    if (nlhs > 2) mexErrMsgIdAndTxt("vo:badArgument", "bundleAdjustmentMotion returns at most [refinedPose, reprojectionErrors]");
    if (!vo_refine_pose || !vo_default_refine_params)
        mexErrMsgIdAndTxt("vo:bundleAdjustmentMotion:unavailable", "this libvo has no vo_refine_pose: keep estworldpose's pose, "
                          "or link a newer libvo");
    const int n = (int)mxGetM(prhs[1]);
    double* wld = points_f64(prhs[1], 3, n, "xyzPoints");
    double* img = points_f64(prhs[2], 2, n, "imagePoints");
    double A[16], K[9], T[16];
    to_row_major(prhs[3], A, 4, 4, "absolutePose.A");
    to_row_major(prhs[4], K, 3, 3, "intrinsics.K");
    vo_refine_params rp;
    vo_default_refine_params(&rp);
    if (nrhs == 6) {
        need_real(prhs[5], mxDOUBLE_CLASS, 1, 3, "opts");
        const double* o = mxGetDoubles(prhs[5]);
        rp.max_iterations = (o[0] >= 1.0 && o[0] <= 100.0 && o[0] == (double)(int32_t)o[0]) ? (int32_t)o[0] : 0;   /* 0: refused by libvo */
        rp.absolute_tolerance = o[1];
        rp.relative_tolerance = o[2];
    }
    need_ctx(0, 0);
    const int rc = vo_refine_pose(g_ctx, img, wld, n, NULL, K, A, &rp, T, NULL);
    if (rc != VO_OK) { mxFree(wld); mxFree(img); check(rc); }
    plhs[0] = mat4_to_mx(T);
    if (nlhs > 1) {
        plhs[1] = mxCreateDoubleMatrix(n, 1, mxREAL);
        double* e = n ? mxGetDoubles(plhs[1]) : NULL;
        double R[9], t[3];
        for (int i = 0; i < 3; ++i) { R[3 * i] = T[i]; R[3 * i + 1] = T[4 + i]; R[3 * i + 2] = T[8 + i]; }
        for (int i = 0; i < 3; ++i) t[i] = -(R[3 * i] * T[3] + R[3 * i + 1] * T[7] + R[3 * i + 2] * T[11]);
        for (int k = 0; k < n; ++k) {
            const double* X = wld + 3 * (size_t)k;
            const double xc = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
            const double yc = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
            const double zc = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
            const double du = (K[0] * (xc / zc) + K[1] * (yc / zc) + K[2]) - img[2 * (size_t)k];
            const double dv = (K[4] * (yc / zc) + K[5]) - img[2 * (size_t)k + 1];
            e[k] = pixel_norm(du, dv);
        }
    }
    mxFree(wld);
    mxFree(img);
}

/* vo_est_fundamental through a weak reference: with a libvo that lacks it 'fundamental' raises
 * vo:estimateFundamentalMatrix:unavailable and every other command runs as before */
extern __typeof__(vo_est_fundamental) vo_est_fundamental __attribute__((weak));
extern __typeof__(vo_default_fund_params) vo_default_fund_params __attribute__((weak));

/* [F, inliersIndex, status] = vo_mex('fundamental', matchedPoints1, matchedPoints2, opts)
 * matchedPoints M x 2 single or double; opts (optional) = [Method NumTrials DistanceThreshold Confidence]
 * double, Method 0 = Norm8Point, 1 = MSAC.  Without the status output the two failures raise
 * vision:estimateFundamentalMatrix:notEnoughPts / :notEnoughInliers, as the toolbox does; with it F is
 * zeros(3) and inliersIndex all false. */
static void cmd_fundamental(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    if (nrhs != 3 && nrhs != 4) need_args(nrhs, 3, "fundamental");
    if (nlhs > 3) mexErrMsgIdAndTxt("vo:badArgument", "estimateFundamentalMatrix returns at most [F, inliersIndex, status]");
    if (!vo_est_fundamental || !vo_default_fund_params)
        mexErrMsgIdAndTxt("vo:estimateFundamentalMatrix:unavailable", "this libvo has no vo_est_fundamental: call the toolbox's "
                          "estimateFundamentalMatrix, or link a newer libvo");
    int n = 0, n2 = 0;
    float* x1 = points_f32(prhs[1], 2, &n, "matchedPoints1");
    float* x2 = points_f32(prhs[2], 2, &n2, "matchedPoints2");
    if (n != n2) mexErrMsgIdAndTxt("vo:badArgument", "matchedPoints1 and matchedPoints2 differ in length");
    vo_fund_params fp;
    vo_default_fund_params(&fp);
    if (nrhs == 4) {
        need_real(prhs[3], mxDOUBLE_CLASS, 1, 4, "opts");
        const double* o = mxGetDoubles(prhs[3]);
        fp.method = (o[0] == 0.0 || o[0] == 1.0) ? (int32_t)o[0] : -1;                                          /* -1, 0: refused by libvo */
        fp.num_trials = (o[1] >= 1.0 && o[1] <= 100000.0 && o[1] == (double)(int32_t)o[1]) ? (int32_t)o[1] : 0;
        fp.distance_threshold = o[2];
        fp.confidence = o[3];
    }
    need_ctx(0, 0);
    double F[9];
    uint8_t* inl = (uint8_t*)mxMalloc((size_t)n + 1);
    memset(inl, 0, (size_t)n + 1);
    const int rc = vo_est_fundamental(g_ctx, x1, x2, n, &fp, 0, F, inl, NULL);
    mxFree(x1);
    mxFree(x2);
    if (rc == VO_ERR_TOO_FEW_POINTS || rc == VO_ERR_NO_CONSENSUS) {
        if (nlhs < 3) {
            mxFree(inl);
            mexErrMsgIdAndTxt(rc == VO_ERR_TOO_FEW_POINTS ? "vision:estimateFundamentalMatrix:notEnoughPts"
                                                          : "vision:estimateFundamentalMatrix:notEnoughInliers",
                              "%s", vo_last_error(g_ctx));
        }
    } else if (rc != VO_OK) {
        mxFree(inl);
        check(rc);
    }
    plhs[0] = mxCreateDoubleMatrix(3, 3, mxREAL);
    double* o = mxGetDoubles(plhs[0]);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[j * 3 + i] = F[3 * i + j];
    if (nlhs > 1) {
        plhs[1] = mxCreateLogicalMatrix(n, 1);
        mxLogical* L = mxGetLogicals(plhs[1]);
        for (int i = 0; i < n; ++i) L[i] = inl[i] != 0;
    }
    if (nlhs > 2) {
        plhs[2] = mxCreateNumericMatrix(1, 1, mxINT32_CLASS, mxREAL);
        *mxGetInt32s(plhs[2]) = rc == VO_OK ? 0 : (rc == VO_ERR_TOO_FEW_POINTS ? 1 : 2);
    }
    mxFree(inl);
}

/* vo_track_points through a weak reference: with a libvo that lacks it 'trackpoints' raises
 * vo:PointTracker:unavailable and every other command runs as before */
extern __typeof__(vo_track_points) vo_track_points __attribute__((weak));
extern __typeof__(vo_default_klt_params) vo_default_klt_params __attribute__((weak));

/* [points, validity, scores] = vo_mex('trackpoints', I0, I1, points, opts)
 * I0, I1 uint8 images of one size; points M x 2 single or double [x y] 1-based; opts (optional) =
 * [NumPyramidLevels BlockHeight BlockWidth MaxIterations MaxBidirectionalError] double (Inf: no
 * bidirectional test).  A point that is not valid keeps its input position, as the toolbox's does. */
static void cmd_trackpoints(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    if (nrhs != 4 && nrhs != 5) need_args(nrhs, 4, "trackpoints");
    if (nlhs > 3) mexErrMsgIdAndTxt("vo:badArgument", "trackpoints returns at most [points, validity, scores]");
    if (!vo_track_points || !vo_default_klt_params)
        mexErrMsgIdAndTxt("vo:PointTracker:unavailable", "this libvo has no vo_track_points: use the toolbox's "
                          "vision.PointTracker, or link a newer libvo");
    const mxArray* I0 = prhs[1];
    const mxArray* I1 = prhs[2];
    need_real(I0, mxUINT8_CLASS, -1, -1, "I0");
    need_real(I1, mxUINT8_CLASS, (long)mxGetM(I0), (long)mxGetN(I0), "I1");
    vo_klt_params kp;
    vo_default_klt_params(&kp);
    if (nrhs == 5) {
        need_real(prhs[4], mxDOUBLE_CLASS, 1, 5, "opts");
        const double* o = mxGetDoubles(prhs[4]);
        int32_t* f[4] = {&kp.num_pyramid_levels, &kp.block_size[0], &kp.block_size[1], &kp.max_iterations};
        for (int k = 0; k < 4; ++k)                                   /* not an integer in 0 .. 1000: 0, refused by libvo */
            *f[k] = (o[k] >= 0.0 && o[k] <= 1000.0 && o[k] == (double)(int32_t)o[k]) ? (int32_t)o[k] : 0;
        kp.max_bidirectional_error = (float)o[4];
    }
    int n = 0;
    float* pts = points_f32(prhs[3], 2, &n, "points");
    const int rows = (int)mxGetM(I0), cols = (int)mxGetN(I0);
    float* out = (float*)mxMalloc(sizeof(float) * 2 * ((size_t)n + 1));
    float* sc = (float*)mxMalloc(sizeof(float) * ((size_t)n + 1));
    uint8_t* ok = (uint8_t*)mxMalloc((size_t)n + 1);
    need_ctx(rows, cols);
    const int rc = vo_track_points(g_ctx, mxGetUint8s(I0), mxGetUint8s(I1), rows, cols, rows, 1, pts, NULL, n, &kp, out, ok, sc, NULL);
    mxFree(pts);
    if (rc != VO_OK) { mxFree(out); mxFree(sc); mxFree(ok); check(rc); }
    plhs[0] = mxCreateNumericMatrix(n, 2, mxSINGLE_CLASS, mxREAL);
    float* P = n ? mxGetSingles(plhs[0]) : NULL;
    for (int i = 0; i < n; ++i) { P[i] = out[2 * i]; P[(size_t)n + i] = out[2 * i + 1]; }
    if (nlhs > 1) {
        plhs[1] = mxCreateLogicalMatrix(n, 1);
        mxLogical* L = mxGetLogicals(plhs[1]);
        for (int i = 0; i < n; ++i) L[i] = ok[i] != 0;
    }
    if (nlhs > 2) {
        plhs[2] = mxCreateNumericMatrix(n, 1, mxSINGLE_CLASS, mxREAL);
        float* S = n ? mxGetSingles(plhs[2]) : NULL;
        for (int i = 0; i < n; ++i) S[i] = sc[i];
    }
    mxFree(out); mxFree(sc); mxFree(ok);
}

/* vo_detect_corners through a weak reference: with a libvo that lacks it 'corners' raises
 * vo:cornerPoints:unavailable and every other command runs as before */
extern __typeof__(vo_detect_corners) vo_detect_corners __attribute__((weak));
extern __typeof__(vo_default_corner_params) vo_default_corner_params __attribute__((weak));
#define VO_MEX_CORNER_CAP 65536     /* the device list of the session's context: 4 x the default max_keypoints */

/* [Location, Metric] = vo_mex('corners', I, opts)
 * I uint8 image; opts (optional) = [method FilterSize MinQuality strongest x y w h] double, method 0 = MinEigen,
 * 1 = Harris, strongest 0 = all, w = 0 = the whole image (ROI 1-based, as MATLAB gives it).  Corners come
 * ascending in (row, column), or the `strongest` strongest. */
static void cmd_corners(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    if (nrhs != 2 && nrhs != 3) need_args(nrhs, 2, "corners");
    if (nlhs > 2) mexErrMsgIdAndTxt("vo:badArgument", "corners returns at most [Location, Metric]");
    if (!vo_detect_corners || !vo_default_corner_params)
        mexErrMsgIdAndTxt("vo:cornerPoints:unavailable", "this libvo has no vo_detect_corners: use the toolbox's "
                          "detectMinEigenFeatures / detectHarrisFeatures, or link a newer libvo");
    const mxArray* I = prhs[1];
    need_real(I, mxUINT8_CLASS, -1, -1, "I");
    vo_corner_params cp;
    vo_default_corner_params(&cp);
    if (nrhs == 3) {
        need_real(prhs[2], mxDOUBLE_CLASS, 1, 8, "opts");
        const double* o = mxGetDoubles(prhs[2]);
        int32_t* f[7] = {&cp.method, &cp.filter_size, &cp.strongest, &cp.roi[0], &cp.roi[1], &cp.roi[2], &cp.roi[3]};
        const int at[7] = {0, 1, 3, 4, 5, 6, 7};
        for (int k = 0; k < 7; ++k) {                                 /* not an integer in 0 .. 2^20: -1, refused by libvo */
            const double v = o[at[k]];
            *f[k] = (v >= 0.0 && v <= 1048576.0 && v == (double)(int32_t)v) ? (int32_t)v : -1;
        }
        cp.min_quality = (float)o[2];
    }
    const int rows = (int)mxGetM(I), cols = (int)mxGetN(I);
    float* loc = (float*)mxMalloc(sizeof(float) * 2 * VO_MEX_CORNER_CAP);
    float* met = (float*)mxMalloc(sizeof(float) * VO_MEX_CORNER_CAP);
    int n = 0;
    need_ctx(rows, cols);
    const int rc = vo_detect_corners(g_ctx, mxGetUint8s(I), rows, cols, rows, 1, &cp, loc, met, VO_MEX_CORNER_CAP, &n);
    if (rc != VO_OK) { mxFree(loc); mxFree(met); check(rc); }
    plhs[0] = mxCreateNumericMatrix(n, 2, mxSINGLE_CLASS, mxREAL);
    float* P = n ? mxGetSingles(plhs[0]) : NULL;
    for (int i = 0; i < n; ++i) { P[i] = loc[2 * i]; P[(size_t)n + i] = loc[2 * i + 1]; }
    if (nlhs > 1) {
        plhs[1] = mxCreateNumericMatrix(n, 1, mxSINGLE_CLASS, mxREAL);
        float* M = n ? mxGetSingles(plhs[1]) : NULL;
        for (int i = 0; i < n; ++i) M[i] = met[i];
    }
    mxFree(loc); mxFree(met);
}

/* vo_disparity_sgm / vo_reconstruct_scene through weak references: with a libvo that lacks them the two
 * commands raise vo:disparitySGM:unavailable after their argument checks and every other command runs as
 * before */
extern __typeof__(vo_disparity_sgm) vo_disparity_sgm __attribute__((weak));
extern __typeof__(vo_default_sgm_params) vo_default_sgm_params __attribute__((weak));
extern __typeof__(vo_reconstruct_scene) vo_reconstruct_scene __attribute__((weak));

/* disparityMap = vo_mex('disparitysgm', I1, I2, opts)
 * I1, I2 uint8 images of one size (left, right; rectified); opts (optional) = [min max UniquenessThreshold] or
 * [min max UniquenessThreshold p1 p2] double.  The images go to libvo as MATLAB holds them and the map is
 * written into the output array: no copy, no transpose on the host. */
static void cmd_disparitysgm(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    if (nrhs != 3 && nrhs != 4) need_args(nrhs, 3, "disparitysgm");
    if (nlhs > 1) mexErrMsgIdAndTxt("vo:badArgument", "disparitysgm returns disparityMap");
    const mxArray* I1 = prhs[1];
    const mxArray* I2 = prhs[2];
    need_real(I1, mxUINT8_CLASS, -1, -1, "I1");
    need_real(I2, mxUINT8_CLASS, (long)mxGetM(I1), (long)mxGetN(I1), "I2");
    if (nrhs == 4) {
        need_real(prhs[3], mxDOUBLE_CLASS, 1, -1, "opts");
        if (mxGetN(prhs[3]) != 3 && mxGetN(prhs[3]) != 5) mexErrMsgIdAndTxt("vo:badArgument", "opts must be 1 x 3 or 1 x 5");
    }
    if (!vo_disparity_sgm || !vo_default_sgm_params)
        mexErrMsgIdAndTxt("vo:disparitySGM:unavailable", "this libvo has no vo_disparity_sgm: use the toolbox's "
                          "disparitySGM, or link a newer libvo");
    vo_sgm_params sp;
    vo_default_sgm_params(&sp);
    if (nrhs == 4) {
        const double* o = mxGetDoubles(prhs[3]);
        const int n = (int)mxGetN(prhs[3]);
        int32_t* f[5] = {&sp.disparity_range[0], &sp.disparity_range[1], &sp.uniqueness_threshold, &sp.p1, &sp.p2};
        for (int k = 0; k < n; ++k)                                   /* not an integer in -2^20 .. 2^20: refused by libvo */
            *f[k] = (o[k] >= -1048576.0 && o[k] <= 1048576.0 && o[k] == (double)(int32_t)o[k]) ? (int32_t)o[k] : INT32_MIN;
    }
    const int rows = (int)mxGetM(I1), cols = (int)mxGetN(I1);
    need_ctx(rows, cols);
    plhs[0] = mxCreateNumericMatrix(rows, cols, mxSINGLE_CLASS, mxREAL);
    check(vo_disparity_sgm(g_ctx, mxGetUint8s(I1), mxGetUint8s(I2), rows, cols, rows, 1, &sp, mxGetSingles(plhs[0]), rows));
}

/* xyz = vo_mex('reconstructscene', disparityMap, Q)
 * disparityMap rows x cols single; Q 4 x 4 double with [X Y Z W]' = Q * [x y d 1]' (include/vo.h's).  xyz is
 * rows x (3 cols) single: the three column-major planes of MATLAB's rows x cols x 3, written in place. */
static void cmd_reconstructscene(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    need_args(nrhs, 3, "reconstructscene");
    if (nlhs > 1) mexErrMsgIdAndTxt("vo:badArgument", "reconstructscene returns xyzPoints");
    const mxArray* D = prhs[1];
    need_real(D, mxSINGLE_CLASS, -1, -1, "disparityMap");
    double Q[16];
    to_row_major(prhs[2], Q, 4, 4, "Q");
    if (!vo_reconstruct_scene)
        mexErrMsgIdAndTxt("vo:disparitySGM:unavailable", "this libvo has no vo_reconstruct_scene: use the toolbox's "
                          "reconstructScene, or link a newer libvo");
    const int rows = (int)mxGetM(D), cols = (int)mxGetN(D);
    need_ctx(rows, cols);
    plhs[0] = mxCreateNumericMatrix(rows, (size_t)3 * cols, mxSINGLE_CLASS, mxREAL);
    check(vo_reconstruct_scene(g_ctx, mxGetSingles(D), rows, cols, rows, 1, Q, mxGetSingles(plhs[0])));
}

/* CreateLandmarksFromFeatures(features_l, features_r, P1, P2, pose, ~) rows (:2-18): VO.m:145-158
 * has already filtered the points, so libvo's own filter runs against no old points (K = 0). */
static void cmd_landmarks(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    (void)nlhs;
    need_args(nrhs, 6, "landmarks");
    int S = 0, S2 = 0;
    float* l = points_f32(prhs[1], 2, &S, "features_l");
    float* r = points_f32(prhs[2], 2, &S2, "features_r");
    if (S != S2) mexErrMsgIdAndTxt("vo:badArgument", "features_l and features_r differ in length");
    const vo_calib cal = calib_from(prhs[3], prhs[4]);
    double A[16];
    to_row_major(prhs[5], A, 4, 4, "pose.A");
    need_ctx(0, 0);
    check(vo_set_calib(g_ctx, &cal));
    int rows = 0;
    const int cap = S + 2;                             /* max(2, last kept odd row) <= S + 2 */
    double* out = (double*)mxMalloc(sizeof(double) * 3 * (size_t)cap);
    check(vo_landmarks(g_ctx, l, r, S, NULL, NULL, 0, A, out, cap, &rows));
    plhs[0] = mxCreateDoubleMatrix(rows, 3, mxREAL);
    double* o = mxGetDoubles(plhs[0]);
    for (int i = 0; i < rows; ++i) for (int a = 0; a < 3; ++a) o[(size_t)a * rows + i] = out[3 * i + a];
    mxFree(l);
    mxFree(r);
    mxFree(out);
}

static void cmd_step(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    need_args(nrhs, 5, "step");
    const mxArray* Il = prhs[1];
    need_real(Il, mxUINT8_CLASS, -1, -1, "Il");
    const int rows = (int)mxGetM(Il), cols = (int)mxGetN(Il);
    need_real(prhs[2], mxUINT8_CLASS, rows, cols, "Ir");
    const vo_calib cal = calib_from(prhs[3], prhs[4]);
    need_ctx(rows, cols);
    check(vo_set_calib(g_ctx, &cal));
    vo_step_out o;
    check(vo_step_batch_ex(g_ctx, mxGetUint8s(Il), mxGetUint8s(prhs[2]), rows, 1, 1, &o));
    plhs[0] = mat4_to_mx(o.rel_pose);
    if (nlhs > 1) plhs[1] = mat4_to_mx(o.pose);
    if (nlhs > 2) plhs[2] = mxCreateDoubleScalar((double)o.status);
    if (nlhs > 3) plhs[3] = mxCreateDoubleScalar((double)o.n_landmarks);
}

static void cmd_landmarks_all(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    (void)nlhs;
    (void)prhs;
    need_args(nrhs, 1, "landmarks_all");
    int rows = 0;
    if (g_ctx) check(vo_get_landmarks(g_ctx, NULL, 0, &rows));
    double* out = (double*)mxMalloc(sizeof(double) * 3 * ((size_t)rows + 1));
    if (rows) check(vo_get_landmarks(g_ctx, out, rows, &rows));
    plhs[0] = mxCreateDoubleMatrix(rows, 3, mxREAL);
    double* o = mxGetDoubles(plhs[0]);
    for (int i = 0; i < rows; ++i) for (int a = 0; a < 3; ++a) o[(size_t)a * rows + i] = out[3 * i + a];
    mxFree(out);
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[])
{
    char cmd[32];
    if (nrhs < 1 || !mxIsChar(prhs[0]) || mxGetString(prhs[0], cmd, sizeof cmd))
        mexErrMsgIdAndTxt("vo:nargin", "vo_mex(command, ...): first argument must be a command string");
    if (!strcmp(cmd, "sift")) cmd_sift(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "describe")) cmd_describe(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "undistort")) cmd_undistort(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "distortion")) cmd_distortion(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "strongest")) cmd_strongest(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "match")) cmd_match(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "matchradius")) cmd_matchradius(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "triangulate")) cmd_triangulate(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "estworldpose")) cmd_estworldpose(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "refinepose")) cmd_refinepose(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "fundamental")) cmd_fundamental(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "trackpoints")) cmd_trackpoints(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "corners")) cmd_corners(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "disparitysgm")) cmd_disparitysgm(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "reconstructscene")) cmd_reconstructscene(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "landmarks")) cmd_landmarks(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "step")) cmd_step(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "landmarks_all")) cmd_landmarks_all(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "reset")) { if (g_ctx) check(vo_reset(g_ctx)); }
    else if (!strcmp(cmd, "close")) cleanup();
    else mexErrMsgIdAndTxt("vo:cmd", "vo_mex: unknown command '%s'", cmd);
}
