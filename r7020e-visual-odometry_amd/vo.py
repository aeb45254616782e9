"""Python host mirror of the reference's per-frame call surface, over the
libvo C-ABI (include/vo.h).

The reference (VO.m) calls MathWorks toolbox functions; this module exposes
the same names with the same argument meaning and error behaviour, each
running on the MI355X through libvo.so:

    undistortImage                         VO.m:75-76
    detectSIFTFeatures / extractFeatures   VO.m:79-84
    matchFeatures                          VO.m:87,283,293,311,323
    find_remaining_points                  VO.m:280-334
    triangulate                            VO.m:113-116
    estworldpose                           VO.m:123-127
    bundleAdjustmentMotion                 after VO.m:123-127 (refine_pose, set_pose_refinement)
    estimateFundamentalMatrix              after matchFeatures (est_fundamental, est_fundamental_batch)
    vision.PointTracker                    pyramidal KLT between frames or cameras (track_points, PointTracker)
    detectMinEigenFeatures / detectHarrisFeatures   cornerPoints for the tracker (detect_corners, detect_corners_batch)
    disparitySGM / reconstructScene        dense stereo depth (disparity_sgm, disparity_sgm_batch, reconstruct_scene)
    CreateLandmarksFromFeatures           CreateLandmarksFromFeatures.m:1-21
    VisualOdometry.step                    the VO.m loop body (VO.m:70-161)

Coordinates are MATLAB 1-based.  Index pairs are 1-based uint32 (P x 2).
There is no CPU fallback: if libvo.so cannot be loaded or no GPU is present,
every call raises VOError.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG = Path(__file__).resolve().parent
LIBPATH = PKG / "lib" / "libvo.so"

VO_OK = 0
VO_ERR_ARG = -1
VO_ERR_HIP = -2
VO_ERR_TOO_FEW_POINTS = -3
VO_ERR_NO_CONSENSUS = -4
VO_ERR_CAPACITY = -5
VO_ERR_STATE = -6
STEP_DEPTH = 3            # VO_STEP_DEPTH: batches vo_step_submit_dev keeps in flight
UNDISTORT_CHUNK = 16      # VO_UD_CHUNK (csrc/vo_internal.h): frames per k_undistort thread


class VOError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libvo error {code}: {msg}")
        self.code = code


class SiftParams(C.Structure):
    _fields_ = [("n_octave_layers", C.c_int32), ("sigma", C.c_float), ("contrast_threshold", C.c_float),
                ("edge_threshold", C.c_float), ("upsample", C.c_int32), ("max_keypoints", C.c_int32)]


class MatchParams(C.Structure):
    _fields_ = [("match_threshold", C.c_float), ("max_ratio", C.c_float)]


class MatchOpts(C.Structure):
    _fields_ = [("match_threshold", C.c_float), ("max_ratio", C.c_float), ("unique", C.c_int32), ("reserved", C.c_int32)]


class RansacParams(C.Structure):
    _fields_ = [("max_num_trials", C.c_int32), ("confidence", C.c_double),
                ("max_reprojection_error", C.c_double), ("seed", C.c_uint32)]


class RefineParams(C.Structure):
    """vo_refine_params: bundleAdjustmentMotion's MaxIterations, RelativeTolerance, AbsoluteTolerance
    (px^2 per used point) and the first Levenberg-Marquardt damping."""
    _fields_ = [("max_iterations", C.c_int32), ("relative_tolerance", C.c_double),
                ("absolute_tolerance", C.c_double), ("lambda0", C.c_double)]


class FundParams(C.Structure):
    """vo_fund_params: estimateFundamentalMatrix's Method (VO_FUND_NORM8 / VO_FUND_MSAC), NumTrials,
    DistanceThreshold (px^2), Confidence (percent) and the Philox seed."""
    _fields_ = [("method", C.c_int32), ("num_trials", C.c_int32), ("distance_threshold", C.c_double),
                ("confidence", C.c_double), ("seed", C.c_uint32)]


class KltParams(C.Structure):
    """vo_klt_params: vision.PointTracker's NumPyramidLevels, BlockSize ({height, width}), MaxIterations and
    MaxBidirectionalError (+inf: off)."""
    _fields_ = [("num_pyramid_levels", C.c_int32), ("block_size", C.c_int32 * 2), ("max_iterations", C.c_int32),
                ("max_bidirectional_error", C.c_float)]


class KltInfo(C.Structure):
    _fields_ = [("status", C.c_uint8), ("stop", C.c_uint8), ("iterations", C.c_uint8), ("levels_skipped", C.c_uint8),
                ("bidir_error", C.c_float)]


class CornerParams(C.Structure):
    """vo_corner_params: method (VO_CORNER_MINEIG | VO_CORNER_HARRIS), FilterSize, MinQuality, strongest (0: all)
    and ROI (x y w h, 1-based; w = 0: the whole image)."""
    _fields_ = [("method", C.c_int32), ("filter_size", C.c_int32), ("min_quality", C.c_float), ("strongest", C.c_int32),
                ("roi", C.c_int32 * 4)]


class SgmParams(C.Structure):
    """vo_sgm_params: DisparityRange [min, max] (max - min in 8, 16, .. 128), UniquenessThreshold (0 .. 100) and the
    path penalties p1 <= p2 (0 .. 255)."""
    _fields_ = [("disparity_range", C.c_int32 * 2), ("uniqueness_threshold", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32)]


class RefineStats(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_used", C.c_int32), ("passes", C.c_int32), ("accepted", C.c_int32),
                ("cost_initial", C.c_double), ("cost_final", C.c_double)]


class Calib(C.Structure):
    _fields_ = [("P1", C.c_double * 12), ("P2", C.c_double * 12), ("K", C.c_double * 9)]


class Distortion(C.Structure):
    """vo_distortion: one camera's intrinsics (row-major K, 0-based principal point) and its
    Brown-Conrady coefficients (cameraIntrinsics RadialDistortion / TangentialDistortion)."""
    _fields_ = [("K", C.c_double * 9), ("radial", C.c_double * 3), ("tangential", C.c_double * 2)]


class Keypoint(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("size", C.c_float), ("angle", C.c_float),
                ("response", C.c_float), ("octave", C.c_int32), ("layer", C.c_int32), ("scale", C.c_float)]


class StepOut(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_left", C.c_int32), ("n_right", C.c_int32),
                ("n_stereo", C.c_int32), ("n_tracked", C.c_int32), ("n_inliers", C.c_int32),
                ("n_landmarks", C.c_int32), ("flags", C.c_int32),
                ("rel_pose", C.c_double * 16), ("pose", C.c_double * 16)]


class PairStats(C.Structure):
    _fields_ = [("n_left", C.c_int32), ("n_right", C.c_int32), ("n_stereo", C.c_int32), ("flags", C.c_int32)]


KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("layer", "<i4"), ("scale", "<f4")])
STEP_DTYPE = np.dtype([("status", "<i4"), ("n_left", "<i4"), ("n_right", "<i4"), ("n_stereo", "<i4"),
                       ("n_tracked", "<i4"), ("n_inliers", "<i4"), ("n_landmarks", "<i4"), ("flags", "<i4"),
                       ("rel_pose", "<f8", (4, 4)), ("pose", "<f8", (4, 4))])
REFINE_STATS_DTYPE = np.dtype([("status", "<i4"), ("n_used", "<i4"), ("passes", "<i4"), ("accepted", "<i4"),
                               ("cost_initial", "<f8"), ("cost_final", "<f8")])
# vo_refine_stats.status
VO_REFINE_CONVERGED, VO_REFINE_MAX_ITER, VO_REFINE_DAMPING, VO_REFINE_DEGENERATE, VO_REFINE_TOO_FEW = 0, 1, 2, -1, -3

# vo_fund_params.method
VO_FUND_NORM8, VO_FUND_MSAC = 0, 1
FUND_METHODS = {"Norm8Point": VO_FUND_NORM8, "MSAC": VO_FUND_MSAC}
FUND_MAX_TRIALS = 100000

# vo_klt_info.status / .stop
VO_KLT_OK, VO_KLT_TEMPLATE_OUT, VO_KLT_LOST, VO_KLT_FLAT, VO_KLT_BIDIR = 0, 1, 2, 3, 4
VO_KLT_STOP_NONE, VO_KLT_STOP_EPS, VO_KLT_STOP_OSC, VO_KLT_STOP_MAXIT = 0, 1, 2, 3
KLT_INFO_DTYPE = np.dtype([("status", "u1"), ("stop", "u1"), ("iterations", "u1"), ("levels_skipped", "u1"),
                           ("bidir_error", "<f4")])
KLT_MAX_COORD = 1048576.0

VO_CORNER_MINEIG, VO_CORNER_HARRIS = 0, 1
VO_SGM_GROUP, VO_SGM_MAX_D = 8, 128

# exported symbols (tests check the library exports every one)
EXPORTS = [
    "vo_default_sift_params", "vo_default_match_params", "vo_default_ransac_params", "vo_create", "vo_destroy",
    "vo_set_calib", "vo_last_error", "vo_sift", "vo_match", "vo_track", "vo_triangulate", "vo_estworldpose",
    "vo_landmarks", "vo_step", "vo_step_batch", "vo_step_batch_dev", "vo_step_submit_dev", "vo_step_collect",
    "vo_steps_pending", "vo_fetch_tracks", "vo_get_landmarks", "vo_reset",
    "vo_sift_match_batch_dev", "vo_fetch_keypoints", "vo_fetch_stereo_pairs", "vo_fetch_gaussian", "vo_stream", "vo_set_profiling",
    "vo_kernel_times", "vo_set_frame_index", "vo_set_concurrency",
    "vo_set_landmark_frame", "vo_get_landmark_rows", "vo_landmarks_to_world", "vo_match_f32",
    "vo_sift_ex", "vo_step_batch_ex", "vo_chain_poses", "vo_landmarks_to_world_frames", "vo_landmarks_world_dev",
    "vo_fetch_candidate_counts", "vo_default_match_opts", "vo_match_ex", "vo_match_f32_ex",
    "vo_undistort", "vo_undistort_batch_dev", "vo_set_distortion", "vo_fetch_rectified",
    "vo_set_strongest", "vo_fetch_detected_count",
    "vo_check_points", "vo_describe", "vo_describe_batch",
    "vo_triangulate_ex", "vo_fetch_track_quality",
    "vo_default_refine_params", "vo_refine_pose", "vo_set_pose_refinement", "vo_fetch_pose_refinement",
    "vo_match_radius", "vo_match_radius_f32",
    "vo_default_fund_params", "vo_est_fundamental", "vo_est_fundamental_batch",
    "vo_default_klt_params", "vo_track_points", "vo_track_points_batch", "vo_fetch_klt_level",
    "vo_default_corner_params", "vo_detect_corners", "vo_detect_corners_batch", "vo_fetch_corner_metric",
    "vo_default_sgm_params", "vo_disparity_sgm", "vo_disparity_sgm_batch", "vo_disparity_sgm_batch_dev", "vo_fetch_sgm_cost",
    "vo_reprojection_matrix", "vo_reconstruct_scene",
]

_libs: dict = {}


def load_library(path: str | os.PathLike | None = None):
    """Load libvo.so (built in-tree by __graft_entry__.build()).  Raises if absent.  One handle
    per path (the default path, or $VO_LIBPATH, unless `path` is given)."""
    p = Path(path) if path else Path(os.environ.get("VO_LIBPATH", LIBPATH))
    key = str(p.resolve()) if p.exists() else str(p)
    if key in _libs:
        return _libs[key]
    if not p.exists():
        raise VOError(VO_ERR_STATE, f"{p} not built; run __graft_entry__.build() (make -C csrc)")
    # One HIP runtime per process: torch ships its own libamdhip64.so.7 (same
    # soname as /opt/rocm's).  Loading torch first makes libvo bind to that
    # runtime, so device pointers from torch tensors and torch.distributed
    # (RCCL) share one runtime with libvo.  Without torch, libvo uses /opt/rocm.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(str(p))
    P = C.POINTER
    vp = C.c_void_p
    L.vo_default_sift_params.argtypes = [P(SiftParams)]
    L.vo_default_match_params.argtypes = [P(MatchParams)]
    L.vo_default_ransac_params.argtypes = [P(RansacParams)]
    L.vo_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, P(Calib), P(SiftParams), P(MatchParams), P(RansacParams)]
    L.vo_create.restype = vp
    L.vo_destroy.argtypes = [vp]
    L.vo_destroy.restype = None
    L.vo_set_calib.argtypes = [vp, P(Calib)]
    L.vo_last_error.argtypes = [vp]
    L.vo_last_error.restype = C.c_char_p
    L.vo_sift.argtypes = [vp, P(C.c_uint8), C.c_int, C.c_int, C.c_int, P(Keypoint), P(C.c_uint8), C.c_int, P(C.c_int)]
    L.vo_match.argtypes = [vp, P(C.c_uint8), C.c_int, P(C.c_uint8), C.c_int, P(C.c_uint32), C.c_int, P(C.c_int)]
    L.vo_sift_ex.argtypes = [vp, P(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, P(Keypoint), P(C.c_uint8), C.c_int,
                             P(C.c_int)]
    L.vo_step_batch_ex.argtypes = [vp, P(C.c_uint8), P(C.c_uint8), C.c_int, C.c_int, C.c_int, P(StepOut)]
    L.vo_match_f32.argtypes = [vp, P(C.c_float), C.c_int, C.c_int, P(C.c_float), C.c_int, C.c_int, C.c_int,
                               P(C.c_uint32), C.c_int, P(C.c_int)]
    L.vo_default_match_opts.argtypes = [P(MatchOpts)]
    L.vo_match_ex.argtypes = [vp, P(C.c_uint8), C.c_int, P(C.c_uint8), C.c_int, P(MatchOpts), P(C.c_uint32), P(C.c_float),
                              C.c_int, P(C.c_int)]
    L.vo_match_f32_ex.argtypes = [vp, P(C.c_float), C.c_int, C.c_int, P(C.c_float), C.c_int, C.c_int, C.c_int, P(MatchOpts),
                                  P(C.c_uint32), P(C.c_float), C.c_int, P(C.c_int)]
    if hasattr(L, "vo_match_radius"):    # (absent from an older library timed beside this one: tools/match_radius_times.py)
        L.vo_match_radius.argtypes = [vp, P(C.c_uint8), C.c_int, P(C.c_uint8), C.c_int, P(C.c_float), P(C.c_float), P(C.c_float),
                                      C.c_int, P(MatchOpts), P(C.c_uint32), P(C.c_float), C.c_int, P(C.c_int)]
        L.vo_match_radius_f32.argtypes = [vp, P(C.c_float), C.c_int, C.c_int, P(C.c_float), C.c_int, C.c_int, C.c_int,
                                          P(C.c_float), P(C.c_float), P(C.c_float), C.c_int, P(MatchOpts), P(C.c_uint32),
                                          P(C.c_float), C.c_int, P(C.c_int)]
    L.vo_undistort.argtypes = [vp, P(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, P(Distortion), P(C.c_uint8), C.c_int]
    L.vo_undistort_batch_dev.argtypes = [vp, vp, C.c_int, P(Distortion), vp]
    L.vo_set_distortion.argtypes = [vp, P(Distortion), P(Distortion)]
    L.vo_fetch_rectified.argtypes = [vp, C.c_int, P(C.c_uint8), C.c_int]
    L.vo_set_strongest.argtypes = [vp, C.c_int]
    L.vo_fetch_detected_count.argtypes = [vp, C.c_int, P(C.c_int)]
    if hasattr(L, "vo_describe"):        # (absent from an older library timed beside this one: tools/describe_times.py)
        L.vo_check_points.argtypes = [P(SiftParams), C.c_int, C.c_int, P(Keypoint), C.c_int, P(C.c_int)]
        L.vo_describe.argtypes = [vp, P(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, P(Keypoint), C.c_int, P(C.c_uint8)]
        L.vo_describe_batch.argtypes = [vp, P(C.c_uint8), C.c_int, C.c_int, C.c_int, P(Keypoint), P(C.c_int32), C.c_int,
                                        P(C.c_uint8)]
    L.vo_track.argtypes = [vp, P(C.c_uint8), P(C.c_uint8), C.c_int, P(C.c_uint8), C.c_int, P(C.c_uint8), C.c_int,
                           P(C.c_uint32), C.c_int, P(C.c_int)]
    L.vo_triangulate.argtypes = [vp, P(C.c_float), P(C.c_float), C.c_int, P(C.c_double), P(C.c_double), P(C.c_double)]
    L.vo_triangulate_ex.argtypes = [vp, P(C.c_float), P(C.c_float), C.c_int, P(C.c_double), P(C.c_double), P(C.c_double),
                                    P(C.c_float), P(C.c_uint8)]
    L.vo_fetch_track_quality.argtypes = [vp, C.c_int, P(C.c_float), P(C.c_float), P(C.c_uint8), C.c_int, P(C.c_int)]
    L.vo_estworldpose.argtypes = [vp, P(C.c_double), P(C.c_double), C.c_int, P(C.c_double), P(RansacParams),
                                  C.c_uint32, P(C.c_double), P(C.c_uint8), P(C.c_int)]
    if hasattr(L, "vo_refine_pose"):     # (absent from an older library timed beside this one: tools/refine_times.py)
        L.vo_default_refine_params.argtypes = [P(RefineParams)]
        L.vo_default_refine_params.restype = None
        L.vo_refine_pose.argtypes = [vp, P(C.c_double), P(C.c_double), C.c_int, P(C.c_uint8), P(C.c_double), P(C.c_double),
                                     P(RefineParams), P(C.c_double), P(RefineStats)]
        L.vo_set_pose_refinement.argtypes = [vp, P(RefineParams)]
        L.vo_fetch_pose_refinement.argtypes = [vp, C.c_int, P(RefineStats)]
    if hasattr(L, "vo_est_fundamental"):     # (absent from an older library timed beside this one)
        L.vo_default_fund_params.argtypes = [P(FundParams)]
        L.vo_default_fund_params.restype = None
        L.vo_est_fundamental.argtypes = [vp, P(C.c_float), P(C.c_float), C.c_int, P(FundParams), C.c_uint32, P(C.c_double),
                                         P(C.c_uint8), P(C.c_int)]
        L.vo_est_fundamental_batch.argtypes = [vp, P(C.c_float), P(C.c_float), C.c_int, P(C.c_int32), C.c_int, P(FundParams),
                                               C.c_uint32, P(C.c_double), P(C.c_uint8), P(C.c_int32), P(C.c_int32)]
    if hasattr(L, "vo_track_points"):        # (absent from an older library timed beside this one)
        L.vo_default_klt_params.argtypes = [P(KltParams)]
        L.vo_default_klt_params.restype = None
        L.vo_track_points.argtypes = [vp, P(C.c_uint8), P(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_float), P(C.c_float),
                                      C.c_int, P(KltParams), P(C.c_float), P(C.c_uint8), P(C.c_float), P(KltInfo)]
        L.vo_track_points_batch.argtypes = [vp, P(C.c_uint8), P(C.c_uint8), C.c_int, C.c_int, C.c_int, P(C.c_float), P(C.c_float),
                                            P(C.c_int32), C.c_int, P(KltParams), P(C.c_float), P(C.c_uint8), P(C.c_float),
                                            P(KltInfo)]
        L.vo_fetch_klt_level.argtypes = [vp, C.c_int, C.c_int, P(C.c_uint8), C.c_int, P(C.c_int), P(C.c_int)]
    if hasattr(L, "vo_detect_corners"):      # (absent from an older library timed beside this one)
        L.vo_default_corner_params.argtypes = [P(CornerParams)]
        L.vo_default_corner_params.restype = None
        L.vo_detect_corners.argtypes = [vp, P(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, P(CornerParams), P(C.c_float),
                                        P(C.c_float), C.c_int, P(C.c_int)]
        L.vo_detect_corners_batch.argtypes = [vp, P(C.c_uint8), C.c_int, C.c_int, C.c_int, P(CornerParams), P(C.c_float),
                                              P(C.c_float), C.c_int, P(C.c_int32), P(C.c_int32)]
        L.vo_fetch_corner_metric.argtypes = [vp, C.c_int, P(C.c_float), C.c_int]
    if hasattr(L, "vo_disparity_sgm"):       # (absent from an older library timed beside this one)
        L.vo_default_sgm_params.argtypes = [P(SgmParams)]
        L.vo_default_sgm_params.restype = None
        L.vo_disparity_sgm.argtypes = [vp, P(C.c_uint8), P(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, P(SgmParams), P(C.c_float),
                                       C.c_int]
        L.vo_disparity_sgm_batch.argtypes = [vp, P(C.c_uint8), P(C.c_uint8), C.c_int, C.c_int, C.c_int, P(SgmParams), P(C.c_float)]
        L.vo_disparity_sgm_batch_dev.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_int, P(SgmParams), C.c_void_p]
        L.vo_fetch_sgm_cost.argtypes = [vp, C.c_int, P(C.c_uint16), C.c_long]
        L.vo_reprojection_matrix.argtypes = [P(C.c_double), P(C.c_double), P(C.c_double)]
        L.vo_reconstruct_scene.argtypes = [vp, P(C.c_float), C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_double), P(C.c_float)]
    L.vo_landmarks.argtypes = [vp, P(C.c_float), P(C.c_float), C.c_int, P(C.c_float), P(C.c_float), C.c_int,
                               P(C.c_double), P(C.c_double), C.c_int, P(C.c_int)]
    L.vo_step.argtypes = [vp, P(C.c_uint8), P(C.c_uint8), C.c_int, P(StepOut)]
    L.vo_step_batch.argtypes = [vp, P(C.c_uint8), P(C.c_uint8), C.c_int, C.c_int, P(StepOut)]
    L.vo_step_batch_dev.argtypes = [vp, vp, vp, C.c_int, P(StepOut)]
    L.vo_step_submit_dev.argtypes = [vp, vp, vp, C.c_int]
    L.vo_step_collect.argtypes = [vp, P(StepOut), C.c_int, P(C.c_int)]
    L.vo_steps_pending.argtypes = [vp]
    L.vo_fetch_tracks.argtypes = [vp, C.c_int, P(C.c_float), P(C.c_float), P(C.c_double), P(C.c_float), C.c_int,
                                  P(C.c_int), P(C.c_int)]
    L.vo_get_landmarks.argtypes = [vp, P(C.c_double), C.c_int, P(C.c_int)]
    L.vo_reset.argtypes = [vp]
    L.vo_set_frame_index.argtypes = [vp, C.c_long]
    L.vo_sift_match_batch_dev.argtypes = [vp, vp, vp, C.c_int, P(PairStats)]
    L.vo_fetch_keypoints.argtypes = [vp, C.c_int, P(Keypoint), P(C.c_uint8), C.c_int, P(C.c_int)]
    L.vo_fetch_stereo_pairs.argtypes = [vp, C.c_int, P(C.c_uint32), C.c_int, P(C.c_int)]
    L.vo_fetch_candidate_counts.argtypes = [vp, C.c_int, P(C.c_int), P(C.c_int)]
    L.vo_fetch_gaussian.argtypes = [vp, C.c_int, C.c_int, C.c_int, P(C.c_float), C.c_int, P(C.c_int), P(C.c_int)]
    L.vo_stream.argtypes = [vp]
    L.vo_stream.restype = vp
    L.vo_set_profiling.argtypes = [vp, C.c_int]
    L.vo_set_concurrency.argtypes = [vp, C.c_int]
    L.vo_set_landmark_frame.argtypes = [vp, C.c_int]
    L.vo_get_landmark_rows.argtypes = [vp, P(C.c_float), P(C.c_uint8), C.c_int, P(C.c_int)]
    L.vo_landmarks_to_world.argtypes = [P(C.c_double), P(C.c_float), P(C.c_uint8), C.c_int, P(C.c_double)]
    L.vo_landmarks_to_world_frames.argtypes = [P(C.c_double), P(C.c_int32), C.c_int, P(C.c_float), P(C.c_uint8), C.c_long,
                                               P(C.c_double)]
    L.vo_chain_poses.argtypes = [P(C.c_double), P(C.c_int32), C.c_int, P(C.c_double), P(C.c_double)]
    L.vo_landmarks_world_dev.argtypes = [vp, P(C.c_double), C.c_int, vp, C.c_long, P(C.c_long)]
    L.vo_kernel_times.argtypes = [vp, P(C.c_char_p), P(C.c_double), P(C.c_int), C.c_int, P(C.c_int)]
    _libs[key] = L
    return L


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _f32_views(F1, F2, who: str):
    """Two n x 128 float32 matrices as the f32 entries take them, without a copy where their
    storage allows: -> (A, ld1, B, ld2, col_major).  A Fortran-ordered array (MATLAB's layout) and
    a C-ordered one (any row stride) go through as they lie; the second follows the first's order."""
    def view(F):
        F = np.asarray(F)
        if F.dtype != np.float32 or F.ndim != 2 or F.shape[1] != 128:
            raise VOError(VO_ERR_ARG, f"{who}: n x 128 float32 matrices")
        if F.strides[0] == 4 and F.strides[1] % 4 == 0 and F.shape[0] > 0:       # column-major
            return F, F.strides[1] // 4, 1
        if F.strides[1] == 4 and F.strides[0] % 4 == 0:
            return F, max(F.strides[0] // 4, 128), 0
        F = np.ascontiguousarray(F)
        return F, 128, 0
    (A, la, ca), (B, lb, cb) = view(F1), view(F2)
    if A.shape[0] and B.shape[0] and ca != cb:
        B, lb, cb = (np.asfortranarray(B), B.shape[0], 1) if ca else (np.ascontiguousarray(B), 128, 0)
    return A, la, B, lb, (ca if A.shape[0] else cb)


def _radius_args(n1: int, n2: int, points2, centers, radius, who: str, order: str = "C"):
    """points2 n2 x 2, centers n1 x 2 and radius (a scalar or n1 values) as float32 arrays in
    storage order `order`; the values themselves are checked by libvo."""
    P2 = np.asarray(points2, np.float32).reshape(-1, 2) if np.size(points2) else np.zeros((0, 2), np.float32)
    Cn = np.asarray(centers, np.float32).reshape(-1, 2) if np.size(centers) else np.zeros((0, 2), np.float32)
    r = np.ascontiguousarray(np.asarray(radius, np.float32).reshape(-1))
    if P2.shape[0] != n2 or Cn.shape[0] != n1:
        raise VOError(VO_ERR_ARG, f"{who}: points2 must be n2 x 2 and centers n1 x 2")
    P2 = np.asfortranarray(P2) if order == "F" else np.ascontiguousarray(P2)
    Cn = np.asfortranarray(Cn) if order == "F" else np.ascontiguousarray(Cn)
    return P2, Cn, r


def default_sift_params(max_keypoints: int = 16384) -> SiftParams:
    p = SiftParams()
    load_library().vo_default_sift_params(C.byref(p))
    p.max_keypoints = max_keypoints
    return p


def default_match_params() -> MatchParams:
    p = MatchParams()
    load_library().vo_default_match_params(C.byref(p))
    return p


def default_ransac_params() -> RansacParams:
    p = RansacParams()
    load_library().vo_default_ransac_params(C.byref(p))
    return p


def default_refine_params(**overrides) -> RefineParams:
    """vo_default_refine_params (20 passes, relative tolerance 1e-9, absolute 0, lambda0 1e-3), with
    any field overridden by keyword."""
    p = RefineParams()
    load_library().vo_default_refine_params(C.byref(p))
    for k, v in overrides.items():
        if k not in dict(RefineParams._fields_):
            raise VOError(VO_ERR_ARG, f"default_refine_params: no field {k}")
        setattr(p, k, v)
    return p


def default_fund_params(**overrides) -> FundParams:
    """vo_default_fund_params (MSAC, 500 trials, DistanceThreshold 0.01 px^2, Confidence 99 %, seed
    0x5EED), with any field overridden by keyword.  Host only: no library, no device."""
    p = FundParams(VO_FUND_MSAC, 500, 0.01, 99.0, 0x5EED)
    for k, v in overrides.items():
        if k not in dict(FundParams._fields_):
            raise VOError(VO_ERR_ARG, f"default_fund_params: no field {k}")
        setattr(p, k, v)
    return p


def check_fund_params(p: FundParams) -> None:
    """vo_est_fundamental's parameter ranges (include/vo.h), checked on the host: VOError(VO_ERR_ARG)
    naming the offending field."""
    bad = None
    if p.method not in (VO_FUND_NORM8, VO_FUND_MSAC):
        bad = "method (VO_FUND_NORM8 or VO_FUND_MSAC; RANSAC, LMedS and LTS are not implemented)"
    elif not 1 <= p.num_trials <= FUND_MAX_TRIALS:
        bad = "num_trials"
    elif not (np.isfinite(p.distance_threshold) and p.distance_threshold > 0.0):
        bad = "distance_threshold"
    elif not 0.0 < p.confidence < 100.0:
        bad = "confidence"
    if bad:
        raise VOError(VO_ERR_ARG, f"est_fundamental: parameter out of range: {bad}")


def fund_points(matchedPoints1, matchedPoints2, who: str = "est_fundamental"):
    """The two point lists as [n][2] float32 (n x 2 arrays, or keypoint arrays with fields x, y), checked
    on the host: equal lengths and finite coordinates, else VOError(VO_ERR_ARG) naming the first
    offending row."""
    out = []
    for k, pts in enumerate((matchedPoints1, matchedPoints2)):
        a = np.asarray(pts)
        if a.dtype.names and "x" in a.dtype.names:
            a = np.stack([a["x"], a["y"]], 1)
        if a.size == 0:
            a = np.zeros((0, 2), np.float32)
        if a.ndim != 2 or a.shape[1] != 2:
            raise VOError(VO_ERR_ARG, f"{who}: matchedPoints{k + 1} must be n x 2")
        a = np.ascontiguousarray(a, np.float32)
        bad = np.flatnonzero(~np.isfinite(a).all(1))
        if len(bad):
            raise VOError(VO_ERR_ARG, f"{who}: matchedPoints{k + 1} row {int(bad[0])} is not finite")
        out.append(a)
    if len(out[0]) != len(out[1]):
        raise VOError(VO_ERR_ARG, f"{who}: matchedPoints1 and matchedPoints2 differ in length")
    return out[0], out[1]


def default_klt_params(**overrides) -> KltParams:
    """vo_default_klt_params (3 levels, BlockSize [31 31], 30 iterations, MaxBidirectionalError inf), with
    any field overridden by keyword (block_size: (height, width)).  Host only: no library, no device."""
    p = KltParams(3, (C.c_int32 * 2)(31, 31), 30, float("inf"))
    for k, v in overrides.items():
        if k not in dict(KltParams._fields_):
            raise VOError(VO_ERR_ARG, f"default_klt_params: no field {k}")
        if k == "block_size":
            v = (C.c_int32 * 2)(int(v[0]), int(v[1]))
        setattr(p, k, v)
    return p


def check_klt_params(p: KltParams) -> None:
    """vo_track_points' parameter ranges (include/vo.h), checked on the host: VOError(VO_ERR_ARG) naming
    the offending field."""
    bad = None
    if not 1 <= p.num_pyramid_levels <= 6:
        bad = "num_pyramid_levels (1 .. 6)"
    elif any(not (5 <= b <= 31 and b % 2 == 1) for b in p.block_size):
        bad = "block_size (odd, 5 .. 31)"
    elif not 1 <= p.max_iterations <= 50:
        bad = "max_iterations (1 .. 50)"
    elif not p.max_bidirectional_error > 0.0:
        bad = "max_bidirectional_error (> 0 or inf)"
    if bad:
        raise VOError(VO_ERR_ARG, f"track_points: parameter out of range: {bad}")


def klt_points(points, who: str = "track_points", name: str = "points") -> np.ndarray:
    """A point list as [n][2] float32 (an n x 2 array, or a keypoint array with fields x, y), checked on the
    host by vo_check_points' finiteness rule (finite, |x|, |y| < 2^20): VOError(VO_ERR_ARG) naming the first
    offending row."""
    a = np.asarray(points)
    if a.dtype.names and "x" in a.dtype.names:
        a = np.stack([a["x"], a["y"]], 1)
    if a.size == 0:
        a = np.zeros((0, 2), np.float32)
    if a.ndim != 2 or a.shape[1] != 2:
        raise VOError(VO_ERR_ARG, f"{who}: {name} must be n x 2")
    a = np.ascontiguousarray(a, np.float32)
    bad = np.flatnonzero(~(np.isfinite(a) & (np.abs(a) < KLT_MAX_COORD)).all(1))
    if len(bad):
        raise VOError(VO_ERR_ARG, f"{who}: {name} row {int(bad[0])} must be finite and below 2^20 in magnitude")
    return a


def default_corner_params(**overrides) -> CornerParams:
    """vo_default_corner_params (VO_CORNER_MINEIG, FilterSize 5, MinQuality 0.01, all corners, the whole image),
    with any field overridden by keyword (roi: (x, y, w, h), 1-based, or None).  Host only: no library, no device."""
    p = CornerParams(VO_CORNER_MINEIG, 5, 0.01, 0, (C.c_int32 * 4)(0, 0, 0, 0))
    for k, v in overrides.items():
        if k not in dict(CornerParams._fields_):
            raise VOError(VO_ERR_ARG, f"default_corner_params: no field {k}")
        if k == "roi":
            v = (C.c_int32 * 4)(0, 0, 0, 0) if v is None else (C.c_int32 * 4)(*(int(e) for e in v))
        setattr(p, k, v)
    return p


def check_corner_params(p: CornerParams, rows: int, cols: int, max_keypoints: int) -> None:
    """vo_detect_corners' parameter ranges (include/vo.h), checked on the host: VOError(VO_ERR_ARG) naming the
    offending field."""
    bad = None
    x, y, w, h = p.roi
    if p.method not in (VO_CORNER_MINEIG, VO_CORNER_HARRIS):
        bad = "method (VO_CORNER_MINEIG | VO_CORNER_HARRIS)"
    elif not (3 <= p.filter_size <= 15 and p.filter_size % 2 == 1):
        bad = "filter_size (odd, 3 .. 15)"
    elif not 0.0 <= p.min_quality <= 1.0:
        bad = "min_quality (0 .. 1)"
    elif not 0 <= p.strongest <= max_keypoints:
        bad = "strongest (0, or 1 .. max_keypoints)"
    elif w != 0 and (w < 1 or h < 1):
        bad = "roi (w, h >= 1)"
    elif w != 0 and (x < 1 or y < 1 or x > cols or y > rows or w > cols - (x - 1) or h > rows - (y - 1)):
        bad = "roi (x y w h, 1-based, inside the image)"
    if bad:
        raise VOError(VO_ERR_ARG, f"detect_corners: parameter out of range: {bad}")


def default_sgm_params(**overrides) -> SgmParams:
    """vo_default_sgm_params (DisparityRange [0 128], UniquenessThreshold 15, p1 10, p2 120), with any field
    overridden by keyword (disparity_range: (min, max)).  Host only: no library, no device."""
    p = SgmParams((C.c_int32 * 2)(0, 128), 15, 10, 120)
    for k, v in overrides.items():
        if k not in dict(SgmParams._fields_):
            raise VOError(VO_ERR_ARG, f"default_sgm_params: no field {k}")
        if k == "disparity_range":
            v = (C.c_int32 * 2)(*(int(e) for e in v))
        setattr(p, k, v)
    return p


def check_sgm_params(p: SgmParams, who: str = "disparity_sgm") -> None:
    """vo_disparity_sgm's parameter ranges (include/vo.h), checked on the host: VOError(VO_ERR_ARG) naming the
    offending field."""
    lo, hi = p.disparity_range
    bad = None
    if lo < -1024 or hi > 1024 or lo >= hi:
        bad = "disparity_range (-1024 <= min < max <= 1024)"
    elif (hi - lo) % 8 != 0 or hi - lo > VO_SGM_MAX_D:
        bad = "disparity_range (max - min in 8, 16, .. 128)"
    elif not 0 <= p.uniqueness_threshold <= 100:
        bad = "uniqueness_threshold (0 .. 100)"
    elif not 0 <= p.p1 <= 255:
        bad = "p1 (0 .. 255)"
    elif not p.p1 <= p.p2 <= 255:
        bad = "p2 (p1 .. 255)"
    if bad:
        raise VOError(VO_ERR_ARG, f"{who}: parameter out of range: {bad}")


def reprojection_matrix(P1, P2) -> np.ndarray:
    """vo_reprojection_matrix: Q [4, 4] float64 of a rectified pair from its 3 x 4 projection matrices (the
    rectified pairs VO.m:27-47 reads); VOError(VO_ERR_ARG) for any other pair."""
    a = np.ascontiguousarray(np.asarray(P1, np.float64).reshape(-1))
    b = np.ascontiguousarray(np.asarray(P2, np.float64).reshape(-1))
    if a.size != 12 or b.size != 12:
        raise VOError(VO_ERR_ARG, "reprojection_matrix: two 3 x 4 projection matrices")
    Q = np.zeros(16, np.float64)
    if load_library().vo_reprojection_matrix(_p(a, C.c_double), _p(b, C.c_double), _p(Q, C.c_double)) != VO_OK:
        raise VOError(VO_ERR_ARG, "reprojection_matrix: not a rectified pair [fx 0 cx tx; 0 fy cy 0; 0 0 1 0] with equal fx, fy, cy, "
                                  "P1's tx = 0 and P2's tx != 0")
    return Q.reshape(4, 4)


def _image_view(img, who: str):
    """A 2-D uint8 image as the image entries take it, without a copy where its storage allows:
    -> (img, ld, col_major)."""
    img = np.asarray(img, np.uint8)
    if img.ndim != 2:
        raise VOError(VO_ERR_ARG, f"{who}: a 2-D uint8 image")
    rows, cols = img.shape
    if rows > 1 and img.strides[0] == 1 and img.strides[1] >= rows:
        return img, img.strides[1], 1
    if img.strides[1] == 1 and img.strides[0] >= cols:
        return img, img.strides[0], 0
    return np.ascontiguousarray(img), cols, 0


def _refine_stats(s: RefineStats) -> np.ndarray:
    out = np.zeros((), REFINE_STATS_DTYPE)
    for name, _ in RefineStats._fields_:
        out[name] = getattr(s, name)
    return out


def calib_from(P1, P2, K=None) -> Calib:
    c = Calib()
    c.P1[:] = [float(v) for v in np.asarray(P1, np.float64).reshape(-1)]
    c.P2[:] = [float(v) for v in np.asarray(P2, np.float64).reshape(-1)]
    K = np.asarray(P1, np.float64)[:, :3] if K is None else np.asarray(K, np.float64)
    c.K[:] = [float(v) for v in K.reshape(-1)]
    return c


def distortion_from(K, radial=(0.0, 0.0, 0.0), tangential=(0.0, 0.0)) -> Distortion:
    """vo_distortion from a 3x3 K (0-based principal point, K[0][1] the skew) and cameraIntrinsics'
    RadialDistortion (2 or 3 entries: k1 k2 [k3]) / TangentialDistortion (p1 p2).  In
    kitti.undistort's order (k1, k2, p1, p2[, k3]) that is radial = (k1, k2, k3),
    tangential = (p1, p2): see distortion_from_kitti."""
    radial = [float(v) for v in np.asarray(radial, np.float64).reshape(-1)]
    tangential = [float(v) for v in np.asarray(tangential, np.float64).reshape(-1)]
    if len(radial) not in (2, 3) or len(tangential) != 2:
        raise VOError(VO_ERR_ARG, "distortion_from: radial has 2 or 3 entries, tangential 2")
    K = np.asarray(K, np.float64)
    if K.shape != (3, 3):
        raise VOError(VO_ERR_ARG, "distortion_from: K is 3x3")
    d = Distortion()
    d.K[:] = [float(v) for v in K.reshape(-1)]
    d.radial[:] = radial + [0.0] * (3 - len(radial))
    d.tangential[:] = tangential
    return d


def distortion_from_kitti(K, dist) -> Distortion:
    """vo_distortion from kitti.undistort's coefficient tuple (k1, k2, p1, p2[, k3]; shorter
    tuples are padded with zeros, as kitti.undistort_map pads them)."""
    k = [float(v) for v in dist] + [0.0] * (5 - len(dist))
    return distortion_from(K, (k[0], k[1], k[4]), (k[2], k[3]))


def as_keypoints(points) -> np.ndarray:
    """A point set as a contiguous KP_DTYPE array (vo_keypoint rows), the form Context.describe
    takes.  Accepted: a KP_DTYPE array (what sift / detectSIFTFeatures return, or any edit of one),
    or a structured array / mapping of equal-length columns with at least x, y and scale; angle
    (degrees), octave and layer default to 0 -- SIFTPoints built by hand: base octave, level 0 --
    and size to 2 * scale.  Anything else raises VOError(VO_ERR_ARG); the values themselves are
    checked by the library (check_points)."""
    if isinstance(points, np.ndarray) and points.dtype == KP_DTYPE:
        if points.ndim != 1:
            raise VOError(VO_ERR_ARG, "points: a 1-D keypoint array")
        return np.ascontiguousarray(points)
    if isinstance(points, np.ndarray) and points.dtype.names:
        cols = {k: points[k] for k in points.dtype.names}
    elif isinstance(points, dict):
        cols = points
    else:
        raise VOError(VO_ERR_ARG, "points: a keypoint array (vo.KP_DTYPE) or columns x, y, scale[, angle, octave, layer]")
    missing = [k for k in ("x", "y", "scale") if k not in cols]
    unknown = [k for k in cols if k not in KP_DTYPE.names]
    if missing or unknown:
        raise VOError(VO_ERR_ARG, f"points: missing columns {missing}, unknown columns {unknown}")
    n = len(np.atleast_1d(cols["x"]))
    out = np.zeros(n, KP_DTYPE)
    for k, v in cols.items():
        v = np.atleast_1d(np.asarray(v))
        if v.shape != (n,):
            raise VOError(VO_ERR_ARG, f"points: column {k} has shape {v.shape}, not ({n},)")
        out[k] = v
    if "size" not in cols:
        out["size"] = out["scale"] * np.float32(2)
    return out


def check_points(points, rows: int, cols: int, sift: SiftParams | None = None) -> int:
    """vo_check_points (host only, no device): -1 when every point is one vo_describe accepts on a
    rows x cols image under SIFT block `sift` (default: the defaults), else the index of the first
    point that is not."""
    pts = as_keypoints(points)
    p = sift or default_sift_params()
    bad = C.c_int(-1)
    rc = load_library().vo_check_points(C.byref(p), rows, cols, pts.ctypes.data_as(C.POINTER(Keypoint)), len(pts),
                                        C.byref(bad))
    if rc != VO_OK and bad.value < 0:
        raise VOError(rc, "vo_check_points: bad arguments")
    return bad.value


class Context:
    """One libvo context (one HIP device, fixed image size, up to max_batch frames per call)."""

    def __init__(self, rows: int = 375, cols: int = 1242, max_batch: int = 1, device: int = 0, calib: Calib | None = None,
                 sift: SiftParams | None = None, match: MatchParams | None = None, ransac: RansacParams | None = None,
                 lib=None):
        self.lib = lib if lib is not None else load_library()
        self.rows, self.cols, self.max_batch = rows, cols, max_batch
        self.sift_params = sift or default_sift_params()
        self.match_params = match or default_match_params()
        self.ransac_params = ransac or default_ransac_params()
        h = self.lib.vo_create(device, rows, cols, max_batch, C.byref(calib) if calib else None,
                               C.byref(self.sift_params), C.byref(self.match_params), C.byref(self.ransac_params))
        if not h:
            raise VOError(VO_ERR_HIP, self.lib.vo_last_error(None).decode())
        self.h = C.c_void_p(h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.vo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, allow=()):
        if rc != VO_OK and rc not in allow:
            raise VOError(rc, self.lib.vo_last_error(self.h).decode())
        return rc

    # ---- detectSIFTFeatures + extractFeatures ----
    def sift(self, img: np.ndarray):
        """A Fortran-ordered image (MATLAB's layout) goes to vo_sift_ex untransposed."""
        img = np.asarray(img, np.uint8)
        if img.ndim != 2:
            raise VOError(VO_ERR_ARG, "sift: a 2-D uint8 image")
        rows, cols = img.shape
        # zero-copy only for positive strides the ABI can express (ld >= rows column-major,
        # ld >= cols row-major); flipped or otherwise strided views are packed first
        if rows > 1 and img.strides[0] == 1 and img.strides[1] >= rows:
            col_major, ld = 1, img.strides[1]
        elif img.strides[1] == 1 and img.strides[0] >= cols:
            col_major, ld = 0, img.strides[0]
        else:
            img = np.ascontiguousarray(img)
            col_major, ld = 0, cols
        cap = self.sift_params.max_keypoints
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 128), np.uint8)
        n = C.c_int(0)
        self._check(self.lib.vo_sift_ex(self.h, _p(img, C.c_uint8), img.shape[0], img.shape[1], ld, col_major,
                                        kps.ctypes.data_as(C.POINTER(Keypoint)), _p(desc, C.c_uint8), cap, C.byref(n)))
        return kps[: n.value].copy(), desc[: n.value].copy()

    # ---- extractFeatures at given points ----
    def describe(self, img: np.ndarray, points) -> np.ndarray:
        """SIFT descriptors [len(points), 128] uint8 of caller-given points on `img` (vo_describe),
        row i for point i.  points: see as_keypoints; x, y, scale, angle, octave and layer are read
        (the rules are vo_check_points')."""
        img = np.asarray(img, np.uint8)
        if img.ndim != 2:
            raise VOError(VO_ERR_ARG, "describe: a 2-D uint8 image")
        pts = as_keypoints(points)
        rows, cols = img.shape
        if rows > 1 and img.strides[0] == 1 and img.strides[1] >= rows:
            col_major, ld = 1, img.strides[1]
        elif img.strides[1] == 1 and img.strides[0] >= cols:
            col_major, ld = 0, img.strides[0]
        else:
            img = np.ascontiguousarray(img)
            col_major, ld = 0, cols
        desc = np.zeros((len(pts), 128), np.uint8)
        self._check(self.lib.vo_describe(self.h, _p(img, C.c_uint8), rows, cols, ld, col_major,
                                         pts.ctypes.data_as(C.POINTER(Keypoint)), len(pts), _p(desc, C.c_uint8)))
        return desc

    def describe_batch(self, imgs: np.ndarray, points_list) -> list:
        """vo_describe_batch: imgs [n_img, rows, cols] (1 .. 2 * max_batch images), points_list one
        point set per image (their counts may differ, 0 included) -> a list of [n_i, 128] uint8."""
        imgs = np.ascontiguousarray(imgs, np.uint8)
        if imgs.ndim != 3 or len(points_list) != imgs.shape[0]:
            raise VOError(VO_ERR_ARG, "describe_batch: imgs [n_img, rows, cols] and one point set per image")
        sets = [as_keypoints(p) for p in points_list]
        counts = np.array([len(s) for s in sets], np.int32)
        stride = int(counts.max()) if len(sets) else 0
        pts = np.zeros((len(sets), max(stride, 1)), KP_DTYPE)
        for i, s in enumerate(sets):
            pts[i, : len(s)] = s
        desc = np.zeros((len(sets), max(stride, 1), 128), np.uint8)
        self._check(self.lib.vo_describe_batch(self.h, _p(imgs, C.c_uint8), imgs.shape[2], 0, imgs.shape[0],
                                               pts.ctypes.data_as(C.POINTER(Keypoint)), _p(counts, C.c_int32), stride,
                                               _p(desc, C.c_uint8)))
        return [desc[i, : counts[i]].copy() for i in range(len(sets))]

    # ---- undistortImage ----
    def undistort(self, img: np.ndarray, K, radial=(0.0, 0.0, 0.0), tangential=(0.0, 0.0), col_major: bool = False) -> np.ndarray:
        """J = undistortImage(I, intrinsics) (vo_undistort): a 2-D uint8 image of the context's
        size; col_major hands it over, and takes the result back, in MATLAB's storage.  A row-major
        view with a row stride >= cols (e.g. a slice of a wider array) goes through as it lies."""
        img = np.asarray(img, np.uint8)
        if img.ndim != 2:
            raise VOError(VO_ERR_ARG, "undistort: a 2-D uint8 image")
        rows, cols = img.shape
        d = distortion_from(K, radial, tangential)
        if col_major:
            src = np.asfortranarray(img)
            out = np.empty((rows, cols), np.uint8, order="F")
            ld = ld_out = rows
        else:
            src = img if img.strides[1] == 1 and img.strides[0] >= cols else np.ascontiguousarray(img)
            out = np.empty((rows, cols), np.uint8)
            ld, ld_out = src.strides[0], cols
        self._check(self.lib.vo_undistort(self.h, _p(src, C.c_uint8), rows, cols, ld, 1 if col_major else 0, C.byref(d),
                                          _p(out, C.c_uint8), ld_out))
        return out

    def undistort_batch_dev(self, d_in: int, d_out: int, B: int, K, radial=(0.0, 0.0, 0.0), tangential=(0.0, 0.0)) -> None:
        """vo_undistort_batch_dev: B tightly packed device frames at d_in -> d_out (device
        pointers), stream-ordered on the context's stream (synchronise before reading d_out)."""
        d = distortion_from(K, radial, tangential)
        self._check(self.lib.vo_undistort_batch_dev(self.h, C.c_void_p(d_in or None), B, C.byref(d), C.c_void_p(d_out or None)))

    def set_distortion(self, left: Distortion | None = None, right: Distortion | None = None) -> None:
        """VO.m:75-76 inside the loop body (vo_set_distortion): step*, sift_match_batch_dev then
        undistort every frame on the device first.  None, or all-zero coefficients, passes a
        camera through; (None, None) restores the context's behaviour without distortion."""
        self._check(self.lib.vo_set_distortion(self.h, C.byref(left) if left is not None else None,
                                               C.byref(right) if right is not None else None))

    def fetch_rectified(self, image: int) -> np.ndarray:
        """The undistorted image 2*frame + side of the last batched call (vo_fetch_rectified)."""
        out = np.empty((self.rows, self.cols), np.uint8)
        self._check(self.lib.vo_fetch_rectified(self.h, image, _p(out, C.c_uint8), out.size))
        return out

    # ---- SIFTPoints.selectStrongest ----
    def set_strongest(self, n: int) -> None:
        """points = selectStrongest(points, n) between detection and description in every entry
        that detects (vo_set_strongest): per image the n keypoints of largest response, sorted by
        response descending with ties in detection order.  0 turns it off (the default)."""
        self._check(self.lib.vo_set_strongest(self.h, int(n)))

    def fetch_detected_count(self, image: int) -> int:
        """The keypoint count of image 2*frame + side of the last call ahead of the selection
        (vo_fetch_detected_count)."""
        n = C.c_int(0)
        self._check(self.lib.vo_fetch_detected_count(self.h, image, C.byref(n)))
        return n.value

    # ---- matchFeatures ----
    def _match_opts(self, unique, match_threshold, max_ratio) -> MatchOpts:
        """The options of vo_match_ex / vo_match_f32_ex; an omitted threshold is the context's."""
        return MatchOpts(self.match_params.match_threshold if match_threshold is None else match_threshold,
                         self.match_params.max_ratio if max_ratio is None else max_ratio, int(bool(unique)), 0)

    def match(self, F1: np.ndarray, F2: np.ndarray, *, unique: bool = False, match_threshold: float | None = None,
              max_ratio: float | None = None, return_metric: bool = False):
        """matchFeatures(F1, F2) on uint8 descriptors.  The keywords are matchFeatures' Unique,
        MatchThreshold (percent, (0, 25]) and MaxRatio ((0, 1]); return_metric=True returns
        (pairs, matchMetric) -- vo_match_ex.  Without keywords: vo_match."""
        F1 = np.ascontiguousarray(F1, np.uint8)
        F2 = np.ascontiguousarray(F2, np.uint8)
        cap = max(F1.shape[0], 1)
        pairs = np.zeros((cap, 2), np.uint32)
        n = C.c_int(0)
        if not unique and match_threshold is None and max_ratio is None and not return_metric:
            self._check(self.lib.vo_match(self.h, _p(F1, C.c_uint8), F1.shape[0], _p(F2, C.c_uint8), F2.shape[0],
                                          _p(pairs, C.c_uint32), cap, C.byref(n)))
            return pairs[: n.value].copy()
        opts = self._match_opts(unique, match_threshold, max_ratio)
        metric = np.zeros(cap, np.float32)
        self._check(self.lib.vo_match_ex(self.h, _p(F1, C.c_uint8), F1.shape[0], _p(F2, C.c_uint8), F2.shape[0], C.byref(opts),
                                         _p(pairs, C.c_uint32), _p(metric, C.c_float), cap, C.byref(n)))
        return (pairs[: n.value].copy(), metric[: n.value].copy()) if return_metric else pairs[: n.value].copy()

    def match_f32(self, F1: np.ndarray, F2: np.ndarray, *, unique: bool = False, match_threshold: float | None = None,
                  max_ratio: float | None = None, return_metric: bool = False):
        """matchFeatures on single-precision n x 128 matrices in their own storage order
        (vo_match_f32): a Fortran-ordered array (MATLAB's layout) goes through without a
        transpose, a C-ordered one (any row stride) likewise.  Keywords as for match()
        (vo_match_f32_ex)."""
        A, la, B, lb, order = _f32_views(F1, F2, "match_f32")
        cap = max(A.shape[0], 1)
        pairs = np.zeros((cap, 2), np.uint32)
        n = C.c_int(0)
        pa = A.ctypes.data_as(C.POINTER(C.c_float)) if A.shape[0] else None
        pb = B.ctypes.data_as(C.POINTER(C.c_float)) if B.shape[0] else None
        if not unique and match_threshold is None and max_ratio is None and not return_metric:
            self._check(self.lib.vo_match_f32(self.h, pa, A.shape[0], la, pb, B.shape[0], lb, order,
                                              _p(pairs, C.c_uint32), cap, C.byref(n)))
            return pairs[: n.value].copy()
        opts = self._match_opts(unique, match_threshold, max_ratio)
        metric = np.zeros(cap, np.float32)
        self._check(self.lib.vo_match_f32_ex(self.h, pa, A.shape[0], la, pb, B.shape[0], lb, order, C.byref(opts),
                                             _p(pairs, C.c_uint32), _p(metric, C.c_float), cap, C.byref(n)))
        return (pairs[: n.value].copy(), metric[: n.value].copy()) if return_metric else pairs[: n.value].copy()

    # ---- matchFeaturesInRadius ----
    def match_in_radius(self, F1: np.ndarray, F2: np.ndarray, points2, centers, radius, *, unique: bool = False,
                        match_threshold: float | None = None, max_ratio: float | None = None, return_metric: bool = False):
        """matchFeaturesInRadius(F1, F2, points2, centerPoints, radius) on uint8 descriptors
        (vo_match_radius): F1 row i is matched only against the F2 rows whose point (points2, n2 x 2)
        lies within radius (a scalar, or one per F1 row) of centers[i], the circle closed; the ratio
        test and Unique run over those candidates alone.  Keywords as for match()."""
        F1 = np.ascontiguousarray(F1, np.uint8).reshape(-1, 128)
        F2 = np.ascontiguousarray(F2, np.uint8).reshape(-1, 128)
        P2, Cn, r = _radius_args(F1.shape[0], F2.shape[0], points2, centers, radius, "match_in_radius")
        cap = max(F1.shape[0], 1)
        pairs = np.zeros((cap, 2), np.uint32)
        metric = np.zeros(cap, np.float32)
        n = C.c_int(0)
        opts = self._match_opts(unique, match_threshold, max_ratio)
        self._check(self.lib.vo_match_radius(self.h, _p(F1, C.c_uint8), F1.shape[0], _p(F2, C.c_uint8), F2.shape[0],
                                             _p(P2, C.c_float), _p(Cn, C.c_float), _p(r, C.c_float), len(r), C.byref(opts),
                                             _p(pairs, C.c_uint32), _p(metric, C.c_float), cap, C.byref(n)))
        return (pairs[: n.value].copy(), metric[: n.value].copy()) if return_metric else pairs[: n.value].copy()

    def match_in_radius_f32(self, F1: np.ndarray, F2: np.ndarray, points2, centers, radius, *, unique: bool = False,
                            match_threshold: float | None = None, max_ratio: float | None = None, return_metric: bool = False):
        """match_in_radius on single-precision n x 128 matrices with integer values 0..255 in their
        own storage order (vo_match_radius_f32); the point matrices go in the features' order."""
        A, la, B, lb, order = _f32_views(F1, F2, "match_in_radius_f32")
        P2, Cn, r = _radius_args(A.shape[0], B.shape[0], points2, centers, radius, "match_in_radius_f32", "F" if order else "C")
        cap = max(A.shape[0], 1)
        pairs = np.zeros((cap, 2), np.uint32)
        metric = np.zeros(cap, np.float32)
        n = C.c_int(0)
        pa = A.ctypes.data_as(C.POINTER(C.c_float)) if A.shape[0] else None
        pb = B.ctypes.data_as(C.POINTER(C.c_float)) if B.shape[0] else None
        opts = self._match_opts(unique, match_threshold, max_ratio)
        self._check(self.lib.vo_match_radius_f32(self.h, pa, A.shape[0], la, pb, B.shape[0], lb, order, _p(P2, C.c_float),
                                                 _p(Cn, C.c_float), _p(r, C.c_float), len(r), C.byref(opts),
                                                 _p(pairs, C.c_uint32), _p(metric, C.c_float), cap, C.byref(n)))
        return (pairs[: n.value].copy(), metric[: n.value].copy()) if return_metric else pairs[: n.value].copy()

    # ---- benchmark workload: SIFT + stereo match of B pairs resident on device ----
    def sift_match_batch_dev(self, d_lefts: int, d_rights: int, B: int, stats: bool = True):
        st = (PairStats * B)() if stats else None
        self._check(self.lib.vo_sift_match_batch_dev(self.h, C.c_void_p(d_lefts), C.c_void_p(d_rights), B, st))
        if stats:
            return [(s.n_left, s.n_right, s.n_stereo, s.flags) for s in st]
        return None

    def fetch_keypoints(self, image: int, descriptors: bool = True):
        """(keypoints, descriptors) of `image` in the last batched call; descriptors=False
        skips the descriptor copy (returns None for them)."""
        cap = self.sift_params.max_keypoints
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 128), np.uint8) if descriptors else None
        n = C.c_int(0)
        self._check(self.lib.vo_fetch_keypoints(self.h, image, kps.ctypes.data_as(C.POINTER(Keypoint)),
                                                _p(desc, C.c_uint8) if descriptors else None, cap, C.byref(n)))
        m = min(n.value, cap)
        return kps[:m].copy(), (desc[:m].copy() if descriptors else None)

    def fetch_candidate_counts(self, image: int) -> tuple[int, int]:
        """(extremum candidates, candidates accepted by the refinement) of `image` in the last
        batched call (vo_fetch_candidate_counts)."""
        nc, na = C.c_int(0), C.c_int(0)
        self._check(self.lib.vo_fetch_candidate_counts(self.h, image, C.byref(nc), C.byref(na)))
        return nc.value, na.value

    def fetch_stereo_pairs(self, frame: int) -> np.ndarray:
        cap = self.sift_params.max_keypoints
        pairs = np.zeros((cap, 2), np.uint32)
        n = C.c_int(0)
        self._check(self.lib.vo_fetch_stereo_pairs(self.h, frame, _p(pairs, C.c_uint32), cap, C.byref(n)))
        return pairs[: min(n.value, cap)].copy()

    def fetch_gaussian(self, image: int, octave: int, level: int) -> np.ndarray:
        """Gaussian level G(octave, level) of image `image` of the last batched call (diagnostic)."""
        r, c = C.c_int(0), C.c_int(0)
        self._check(self.lib.vo_fetch_gaussian(self.h, image, octave, level, None, 0, C.byref(r), C.byref(c)))
        out = np.empty((r.value, c.value), np.float32)
        self._check(self.lib.vo_fetch_gaussian(self.h, image, octave, level, _p(out, C.c_float), out.size, None, None))
        return out

    # ---- find_remaining_points ----
    def track(self, old_l, old_r, cur_l, cur_r) -> np.ndarray:
        """-> idx [K, 3] 1-based rows {old_row, cur_left_row, cur_right_row}."""
        a = [np.ascontiguousarray(x, np.uint8).reshape(-1, 128) for x in (old_l, old_r, cur_l, cur_r)]
        cap = max(x.shape[0] for x in a) + 1
        idx = np.zeros((cap, 3), np.uint32)
        n = C.c_int(0)
        self._check(self.lib.vo_track(self.h, _p(a[0], C.c_uint8), _p(a[1], C.c_uint8), a[0].shape[0],
                                      _p(a[2], C.c_uint8), a[2].shape[0], _p(a[3], C.c_uint8), a[3].shape[0],
                                      _p(idx, C.c_uint32), cap, C.byref(n)))
        return idx[: n.value].copy()

    # ---- triangulate ----
    def triangulate(self, x1, x2, P1, P2, quality=False):
        """worldPoints [n, 3].  quality=True is [worldPoints, reprojectionErrors, validIndex] =
        triangulate(...) (vo_triangulate_ex): -> (X, err float32 [n], valid bool [n]), err the mean
        reprojection distance in pixels, valid the points in front of both cameras.  quality="err" /
        "valid" asks the library for that output alone (the other is None)."""
        x1 = np.ascontiguousarray(x1, np.float32).reshape(-1, 2)
        x2 = np.ascontiguousarray(x2, np.float32).reshape(-1, 2)
        P1 = np.ascontiguousarray(P1, np.float64)
        P2 = np.ascontiguousarray(P2, np.float64)
        n = x1.shape[0]
        X = np.zeros((n, 3))
        if not quality:
            self._check(self.lib.vo_triangulate(self.h, _p(x1, C.c_float), _p(x2, C.c_float), n,
                                                _p(P1, C.c_double), _p(P2, C.c_double), _p(X, C.c_double)))
            return X
        if quality not in (True, "err", "valid"):
            raise VOError(VO_ERR_ARG, "triangulate: quality is False, True, 'err' or 'valid'")
        err = np.zeros(n, np.float32) if quality in (True, "err") else None
        valid = np.zeros(n, np.uint8) if quality in (True, "valid") else None
        self._check(self.lib.vo_triangulate_ex(self.h, _p(x1, C.c_float), _p(x2, C.c_float), n, _p(P1, C.c_double),
                                               _p(P2, C.c_double), _p(X, C.c_double),
                                               _p(err, C.c_float) if err is not None else None,
                                               _p(valid, C.c_uint8) if valid is not None else None))
        return X, err, valid.astype(bool) if valid is not None else None

    # ---- estworldpose ----
    def estworldpose(self, imagePoints, worldPoints, K, params: RansacParams | None = None, frame_key: int = 0,
                     raise_on_failure: bool = True):
        """-> (status, T 4x4 camera pose in world, inlier mask, n_inliers).  Like MATLAB,
        raises on < 4 points / no consensus unless raise_on_failure=False."""
        img = np.ascontiguousarray(imagePoints, np.float64).reshape(-1, 2)
        world = np.ascontiguousarray(worldPoints, np.float64).reshape(-1, 3)
        K = np.ascontiguousarray(K, np.float64)
        T = np.zeros(16)
        inl = np.zeros(max(img.shape[0], 1), np.uint8)
        nin = C.c_int(0)
        rc = self.lib.vo_estworldpose(self.h, _p(img, C.c_double), _p(world, C.c_double), img.shape[0], _p(K, C.c_double),
                                      C.byref(params) if params else None, frame_key, _p(T, C.c_double),
                                      _p(inl, C.c_uint8), C.byref(nin))
        if raise_on_failure:
            self._check(rc)
        else:
            self._check(rc, allow=(VO_ERR_TOO_FEW_POINTS, VO_ERR_NO_CONSENSUS))
        return rc, T.reshape(4, 4), inl[: img.shape[0]].astype(bool), nin.value

    # ---- bundleAdjustmentMotion ----
    def refine_pose(self, imagePoints, worldPoints, T, K, use=None, params: RefineParams | None = None):
        """refinedPose = bundleAdjustmentMotion(worldPoints, imagePoints, T, intrinsics) on the points
        with use != 0 (None: all), e.g. estworldpose's pose and inlier mask (vo_refine_pose).
        -> (T 4x4, stats record of REFINE_STATS_DTYPE: status VO_REFINE_*, n_used, passes, accepted,
        cost_initial, cost_final in px^2)."""
        img = np.ascontiguousarray(imagePoints, np.float64).reshape(-1, 2)
        world = np.ascontiguousarray(worldPoints, np.float64).reshape(-1, 3)
        if img.shape[0] != world.shape[0]:
            raise VOError(VO_ERR_ARG, "refine_pose: imagePoints and worldPoints differ in length")
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        T = np.ascontiguousarray(T, np.float64).reshape(16)
        u = None
        if use is not None:
            u = np.ascontiguousarray(np.asarray(use) != 0, np.uint8).reshape(-1)
            if u.shape[0] != img.shape[0]:
                raise VOError(VO_ERR_ARG, "refine_pose: use and imagePoints differ in length")
        out = np.zeros(16)
        st = RefineStats()
        self._check(self.lib.vo_refine_pose(self.h, _p(img, C.c_double), _p(world, C.c_double), img.shape[0],
                                            _p(u, C.c_uint8) if u is not None else None, _p(K, C.c_double), _p(T, C.c_double),
                                            C.byref(params) if params is not None else None, _p(out, C.c_double), C.byref(st)))
        return out.reshape(4, 4), _refine_stats(st)

    def set_pose_refinement(self, params: RefineParams | None) -> None:
        """bundleAdjustmentMotion after estworldpose in every entry that runs the loop body
        (vo_set_pose_refinement): rel_pose / pose are then the refined ones.  None turns it off."""
        self._check(self.lib.vo_set_pose_refinement(self.h, C.byref(params) if params is not None else None))

    def fetch_pose_refinement(self, frame: int) -> np.ndarray:
        """The refinement's stats record of `frame` of the last collected batch (vo_fetch_pose_refinement)."""
        st = RefineStats()
        self._check(self.lib.vo_fetch_pose_refinement(self.h, frame, C.byref(st)))
        return _refine_stats(st)

    # ---- estimateFundamentalMatrix ----
    def est_fundamental(self, matchedPoints1, matchedPoints2, params: FundParams | None = None, key: int = 0,
                        raise_on_failure: bool = False):
        """[F, inliersIndex, status] = estimateFundamentalMatrix(matchedPoints1, matchedPoints2, ...)
        (vo_est_fundamental) -> (status, F 3x3 with [x2 1] F [x1 1]' = 0, inlier mask [n] bool, n_inliers).
        status is VO_OK, VO_ERR_TOO_FEW_POINTS (n < 8) or VO_ERR_NO_CONSENSUS (F and the mask are then 0);
        with raise_on_failure the last two raise, as the toolbox does when status is not requested."""
        x1, x2 = fund_points(matchedPoints1, matchedPoints2)
        p = params if params is not None else default_fund_params()
        check_fund_params(p)
        n = len(x1)
        F = np.zeros(9)
        inl = np.zeros(max(n, 1), np.uint8)
        nin = C.c_int(0)
        rc = self.lib.vo_est_fundamental(self.h, _p(x1, C.c_float), _p(x2, C.c_float), n, C.byref(p), int(key) & 0xFFFFFFFF,
                                         _p(F, C.c_double), _p(inl, C.c_uint8), C.byref(nin))
        self._check(rc, allow=() if raise_on_failure else (VO_ERR_TOO_FEW_POINTS, VO_ERR_NO_CONSENSUS))
        return rc, F.reshape(3, 3), inl[:n].astype(bool), nin.value

    def est_fundamental_batch(self, x1, x2, n_pts, params: FundParams | None = None, key0: int = 0):
        """B problems in one launch (vo_est_fundamental_batch): x1, x2 [B][pts_stride][2] float32, problem f
        uses its first n_pts[f] rows and the key key0 + f -> (status [B], F [B, 3, 3], inliers
        [B, pts_stride] bool, n_inliers [B])."""
        x1 = np.ascontiguousarray(x1, np.float32)
        x2 = np.ascontiguousarray(x2, np.float32)
        n_pts = np.ascontiguousarray(n_pts, np.int32).reshape(-1)
        B = len(n_pts)
        if x1.shape != x2.shape or x1.ndim != 3 or x1.shape[0] != B or x1.shape[2] != 2:
            raise VOError(VO_ERR_ARG, "est_fundamental_batch: x1 and x2 must both be [B][pts_stride][2]")
        stride = x1.shape[1]
        for f in range(B):
            if not 0 <= n_pts[f] <= stride:
                raise VOError(VO_ERR_ARG, f"est_fundamental_batch: n_pts[{f}] is outside 0 .. pts_stride")
            fund_points(x1[f, :n_pts[f]], x2[f, :n_pts[f]], f"est_fundamental_batch: problem {f}")
        p = params if params is not None else default_fund_params()
        check_fund_params(p)
        F = np.zeros((max(B, 1), 9))
        inl = np.zeros((max(B, 1), max(stride, 1)), np.uint8)
        nin = np.zeros(max(B, 1), np.int32)
        st = np.zeros(max(B, 1), np.int32)
        self._check(self.lib.vo_est_fundamental_batch(self.h, _p(x1, C.c_float), _p(x2, C.c_float), stride, _p(n_pts, C.c_int32), B,
                                                      C.byref(p), int(key0) & 0xFFFFFFFF, _p(F, C.c_double), _p(inl, C.c_uint8),
                                                      _p(nin, C.c_int32), _p(st, C.c_int32)))
        return st[:B], F[:B].reshape(B, 3, 3), inl[:B, :stride].astype(bool), nin[:B]

    # ---- vision.PointTracker ----
    def track_points(self, img0: np.ndarray, img1: np.ndarray, points, guess=None, params: KltParams | None = None):
        """Pyramidal Lucas-Kanade from img0 to img1 (vo_track_points): points [n][2] 1-based pixels, guess
        [n][2] or None -> (points1 [n][2] float32, valid [n] bool, scores [n] float32, info [n] KLT_INFO_DTYPE).
        A point that is not valid keeps its input position.  Images of one storage (both Fortran-ordered,
        or both row-major with one row stride) go through as they lie."""
        a, b = np.asarray(img0, np.uint8), np.asarray(img1, np.uint8)
        if a.ndim != 2 or a.shape != b.shape:
            raise VOError(VO_ERR_ARG, "track_points: two 2-D uint8 images of one size")
        rows, cols = a.shape
        if rows > 1 and a.strides == b.strides and a.strides[0] == 1 and a.strides[1] >= rows:
            col_major, ld = 1, a.strides[1]
        elif a.strides == b.strides and a.strides[1] == 1 and a.strides[0] >= cols:
            col_major, ld = 0, a.strides[0]
        else:
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            col_major, ld = 0, cols
        pts = klt_points(points)
        g = None if guess is None else klt_points(guess, name="guess")
        if g is not None and len(g) != len(pts):
            raise VOError(VO_ERR_ARG, "track_points: guess and points differ in length")
        p = params if params is not None else default_klt_params()
        check_klt_params(p)
        n = len(pts)
        out = np.zeros((max(n, 1), 2), np.float32)
        valid = np.zeros(max(n, 1), np.uint8)
        scores = np.zeros(max(n, 1), np.float32)
        info = np.zeros(max(n, 1), KLT_INFO_DTYPE)
        self._check(self.lib.vo_track_points(self.h, _p(a, C.c_uint8), _p(b, C.c_uint8), rows, cols, ld, col_major, _p(pts, C.c_float),
                                             _p(g, C.c_float) if g is not None else None, n, C.byref(p), _p(out, C.c_float),
                                             _p(valid, C.c_uint8), _p(scores, C.c_float), info.ctypes.data_as(C.POINTER(KltInfo))))
        return out[:n], valid[:n].astype(bool), scores[:n], info[:n]

    def track_points_batch(self, imgs0: np.ndarray, imgs1: np.ndarray, points_list, guess_list=None,
                           params: KltParams | None = None) -> list:
        """vo_track_points_batch: imgs0, imgs1 [n_pairs, rows, cols], one point set per pair (their counts may
        differ, 0 included), guess_list None or one guess set per pair -> a list of track_points' tuples."""
        imgs0, imgs1 = np.ascontiguousarray(imgs0, np.uint8), np.ascontiguousarray(imgs1, np.uint8)
        if imgs0.ndim != 3 or imgs0.shape != imgs1.shape or len(points_list) != imgs0.shape[0]:
            raise VOError(VO_ERR_ARG, "track_points_batch: imgs0, imgs1 [n_pairs, rows, cols] and one point set per pair")
        B = imgs0.shape[0]
        sets = [klt_points(q, f"track_points_batch: pair {f}") for f, q in enumerate(points_list)]
        counts = np.array([len(q) for q in sets], np.int32)
        stride = int(counts.max()) if B else 0
        pts = np.zeros((B, max(stride, 1), 2), np.float32)
        g = None
        if guess_list is not None:
            if len(guess_list) != B:
                raise VOError(VO_ERR_ARG, "track_points_batch: one guess set per pair")
            g = np.zeros_like(pts)
        for f, q in enumerate(sets):
            pts[f, : len(q)] = q
            if g is not None:
                gq = klt_points(guess_list[f], f"track_points_batch: pair {f}", "guess")
                if len(gq) != len(q):
                    raise VOError(VO_ERR_ARG, f"track_points_batch: pair {f}: guess and points differ in length")
                g[f, : len(q)] = gq
        p = params if params is not None else default_klt_params()
        check_klt_params(p)
        out = np.zeros_like(pts)
        valid = np.zeros((B, max(stride, 1)), np.uint8)
        scores = np.zeros((B, max(stride, 1)), np.float32)
        info = np.zeros((B, max(stride, 1)), KLT_INFO_DTYPE)
        self._check(self.lib.vo_track_points_batch(self.h, _p(imgs0, C.c_uint8), _p(imgs1, C.c_uint8), imgs0.shape[2], 0, B,
                                                   _p(pts, C.c_float), _p(g, C.c_float) if g is not None else None,
                                                   _p(counts, C.c_int32), stride, C.byref(p), _p(out, C.c_float), _p(valid, C.c_uint8),
                                                   _p(scores, C.c_float), info.ctypes.data_as(C.POINTER(KltInfo))))
        return [(out[f, : counts[f]].copy(), valid[f, : counts[f]].astype(bool), scores[f, : counts[f]].copy(),
                 info[f, : counts[f]].copy()) for f in range(B)]

    def fetch_klt_level(self, image: int, level: int) -> np.ndarray:
        """Diagnostic (vo_fetch_klt_level): pyramid level `level` of image 2 * pair + which of the last track call."""
        r, q = C.c_int(0), C.c_int(0)
        out = np.zeros(self.rows * self.cols, np.uint8)
        self._check(self.lib.vo_fetch_klt_level(self.h, image, level, _p(out, C.c_uint8), out.size, C.byref(r), C.byref(q)))
        return out[: r.value * q.value].reshape(r.value, q.value).copy()

    # ---- detectMinEigenFeatures / detectHarrisFeatures ----
    def detect_corners(self, img: np.ndarray, params: CornerParams | None = None, capacity: int | None = None):
        """cornerPoints of one image (vo_detect_corners) -> (Location [n][2] float32 = (x, y) 1-based, Metric [n]
        float32), ascending in (row, column), or the params.strongest strongest.  capacity: rows the call may
        return (default: the device list's 4 x max_keypoints).  More corners than that: VOError(VO_ERR_CAPACITY)
        whose .count is the true count.  The image goes through as it lies (see sift)."""
        img = np.asarray(img, np.uint8)
        if img.ndim != 2:
            raise VOError(VO_ERR_ARG, "detect_corners: a 2-D uint8 image")
        rows, cols = img.shape
        if rows > 1 and img.strides[0] == 1 and img.strides[1] >= rows:
            col_major, ld = 1, img.strides[1]
        elif img.strides[1] == 1 and img.strides[0] >= cols:
            col_major, ld = 0, img.strides[0]
        else:
            img = np.ascontiguousarray(img)
            col_major, ld = 0, cols
        p = params if params is not None else default_corner_params()
        check_corner_params(p, self.rows, self.cols, self.sift_params.max_keypoints)
        cap = 4 * self.sift_params.max_keypoints if capacity is None else int(capacity)
        loc = np.zeros((max(cap, 1), 2), np.float32)
        met = np.zeros(max(cap, 1), np.float32)
        n = C.c_int(0)
        rc = self.lib.vo_detect_corners(self.h, _p(img, C.c_uint8), rows, cols, ld, col_major, C.byref(p), _p(loc, C.c_float),
                                        _p(met, C.c_float), cap, C.byref(n))
        if rc == VO_ERR_CAPACITY:
            e = VOError(rc, self.lib.vo_last_error(self.h).decode())
            e.count = n.value
            raise e
        self._check(rc)
        return loc[: n.value].copy(), met[: n.value].copy()

    def detect_corners_batch(self, imgs: np.ndarray, params: CornerParams | None = None, capacity: int | None = None) -> list:
        """vo_detect_corners_batch: imgs [n_img, rows, cols] -> one (Location, Metric, status, count) per image;
        status VO_OK, or VO_ERR_CAPACITY with empty arrays and the true count."""
        imgs = np.ascontiguousarray(imgs, np.uint8)
        if imgs.ndim != 3:
            raise VOError(VO_ERR_ARG, "detect_corners_batch: imgs [n_img, rows, cols]")
        B = imgs.shape[0]
        p = params if params is not None else default_corner_params()
        check_corner_params(p, self.rows, self.cols, self.sift_params.max_keypoints)
        cap = 4 * self.sift_params.max_keypoints if capacity is None else int(capacity)
        loc = np.zeros((max(B, 1), max(cap, 1), 2), np.float32)
        met = np.zeros((max(B, 1), max(cap, 1)), np.float32)
        n, st = np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int32)
        self._check(self.lib.vo_detect_corners_batch(self.h, _p(imgs, C.c_uint8), imgs.shape[2], 0, B, C.byref(p), _p(loc, C.c_float),
                                                     _p(met, C.c_float), cap, _p(n, C.c_int32), _p(st, C.c_int32)))
        return [(loc[i, : n[i]].copy(), met[i, : n[i]].copy(), VO_OK, int(n[i])) if st[i] == VO_OK else
                (np.zeros((0, 2), np.float32), np.zeros(0, np.float32), int(st[i]), int(n[i])) for i in range(B)]

    def fetch_corner_metric(self, image: int = 0) -> np.ndarray:
        """Diagnostic (vo_fetch_corner_metric): the metric plane [rows, cols] float32 of image `image` of the last
        detect_corners call."""
        out = np.zeros((self.rows, self.cols), np.float32)
        self._check(self.lib.vo_fetch_corner_metric(self.h, image, _p(out, C.c_float), out.size))
        return out

    # ---- disparitySGM / reconstructScene ----
    def disparity_sgm(self, left: np.ndarray, right: np.ndarray, params: SgmParams | None = None) -> np.ndarray:
        """disparityMap = disparitySGM(I1, I2) of one rectified pair (vo_disparity_sgm) -> [rows, cols] float32, NaN
        where the match is unreliable or falls outside the right image.  The images go through as they lie (see
        sift), the second in the first's storage order; the map has that order too."""
        left, ld, col_major = _image_view(left, "disparity_sgm")
        right = np.asarray(right, np.uint8)
        if right.shape != left.shape:
            raise VOError(VO_ERR_ARG, "disparity_sgm: two images of one size")
        rows, cols = left.shape
        if col_major:
            right = np.asfortranarray(right)
            ld_r = rows
        else:
            right = np.ascontiguousarray(right)
            ld_r = cols
        if ld_r != ld:                                     # one stride for both: pack the first as well
            left = np.asfortranarray(left) if col_major else np.ascontiguousarray(left)
            ld = ld_r
        p = params if params is not None else default_sgm_params()
        check_sgm_params(p)
        out = np.zeros((rows, cols), np.float32, order="F" if col_major else "C")
        self._check(self.lib.vo_disparity_sgm(self.h, _p(left, C.c_uint8), _p(right, C.c_uint8), rows, cols, ld, col_major, C.byref(p),
                                              _p(out, C.c_float), rows if col_major else cols))
        return out

    def disparity_sgm_batch(self, lefts: np.ndarray, rights: np.ndarray, params: SgmParams | None = None) -> np.ndarray:
        """vo_disparity_sgm_batch: lefts, rights [n_pairs, rows, cols] -> [n_pairs, rows, cols] float32; the pairs
        run in groups of VO_SGM_GROUP."""
        lefts, rights = np.ascontiguousarray(lefts, np.uint8), np.ascontiguousarray(rights, np.uint8)
        if lefts.ndim != 3 or lefts.shape != rights.shape or lefts.shape[0] < 1:
            raise VOError(VO_ERR_ARG, "disparity_sgm_batch: lefts, rights [n_pairs, rows, cols]")
        p = params if params is not None else default_sgm_params()
        check_sgm_params(p, "disparity_sgm_batch")
        out = np.zeros(lefts.shape, np.float32)
        self._check(self.lib.vo_disparity_sgm_batch(self.h, _p(lefts, C.c_uint8), _p(rights, C.c_uint8), lefts.shape[2], 0,
                                                    lefts.shape[0], C.byref(p), _p(out, C.c_float)))
        return out

    def disparity_sgm_batch_dev(self, d_lefts: int, d_rights: int, B: int, d_disp: int, params: SgmParams | None = None) -> None:
        """vo_disparity_sgm_batch_dev: B tightly packed row-major device pairs at d_lefts, d_rights -> float32 maps
        at d_disp (device pointers), stream-ordered on the context's stream (synchronise before reading)."""
        p = params if params is not None else default_sgm_params()
        check_sgm_params(p, "disparity_sgm_batch_dev")
        self._check(self.lib.vo_disparity_sgm_batch_dev(self.h, C.c_void_p(d_lefts or None), C.c_void_p(d_rights or None), B, C.byref(p),
                                                        C.c_void_p(d_disp or None)))

    def fetch_sgm_cost(self, pair: int, D: int) -> np.ndarray:
        """Diagnostic (vo_fetch_sgm_cost): the summed path costs S [rows, cols, D] uint16 of pair `pair` of the last
        disparity_sgm* call (of its last group of VO_SGM_GROUP pairs); D = that call's max - min."""
        out = np.zeros((self.rows, self.cols, int(D)), np.uint16)
        self._check(self.lib.vo_fetch_sgm_cost(self.h, pair, _p(out, C.c_uint16), out.size))
        return out

    def reconstruct_scene(self, disp: np.ndarray, Q) -> np.ndarray:
        """xyzPoints = reconstructScene(disparityMap, Q) (vo_reconstruct_scene) -> [rows, cols, 3] float32, in the
        map's storage order (a Fortran-ordered map gives a Fortran-ordered rows x cols x 3 array, as MATLAB holds
        it); NaN where the disparity is NaN."""
        disp = np.asarray(disp, np.float32)
        if disp.ndim != 2:
            raise VOError(VO_ERR_ARG, "reconstruct_scene: a 2-D float32 disparity map")
        rows, cols = disp.shape
        if rows > 1 and disp.strides[0] == 4 and disp.strides[1] >= 4 * rows and disp.strides[1] % 4 == 0:
            col_major, ld = 1, disp.strides[1] // 4
        elif disp.strides[1] == 4 and disp.strides[0] >= 4 * cols and disp.strides[0] % 4 == 0:
            col_major, ld = 0, disp.strides[0] // 4
        else:
            disp = np.ascontiguousarray(disp)
            col_major, ld = 0, cols
        q = np.ascontiguousarray(np.asarray(Q, np.float64).reshape(-1))
        if q.size != 16:
            raise VOError(VO_ERR_ARG, "reconstruct_scene: Q is 4 x 4")
        out = np.zeros((rows, cols, 3), np.float32, order="F" if col_major else "C")
        self._check(self.lib.vo_reconstruct_scene(self.h, _p(disp, C.c_float), rows, cols, ld, col_major, _p(q, C.c_double),
                                                  _p(out, C.c_float)))
        return out

    # ---- new-landmark filter + CreateLandmarksFromFeatures ----
    def landmarks(self, l_pos, r_pos, old_l, old_r, pose) -> np.ndarray:
        a = [np.ascontiguousarray(x, np.float32).reshape(-1, 2) for x in (l_pos, r_pos, old_l, old_r)]
        pose = np.ascontiguousarray(pose, np.float64)
        cap = a[0].shape[0] + 2
        out = np.zeros((cap, 3))
        rows = C.c_int(0)
        self._check(self.lib.vo_landmarks(self.h, _p(a[0], C.c_float), _p(a[1], C.c_float), a[0].shape[0],
                                          _p(a[2], C.c_float), _p(a[3], C.c_float), a[2].shape[0],
                                          _p(pose, C.c_double), _p(out, C.c_double), cap, C.byref(rows)))
        return out[: rows.value].copy()

    # ---- the VO.m loop body ----
    def step_batch(self, lefts: np.ndarray, rights: np.ndarray, col_major: bool = False) -> np.ndarray:
        """B frames [B, rows, cols]; with col_major the frames are handed over in MATLAB's
        storage (each frame column-major: pixel (r, c) at c * rows + r)."""
        L, R = np.asarray(lefts, np.uint8), np.asarray(rights, np.uint8)
        B = L.shape[0]
        if col_major:
            L = np.ascontiguousarray(np.swapaxes(L, 1, 2))       # [B, cols, rows] = B column-major frames
            R = np.ascontiguousarray(np.swapaxes(R, 1, 2))
            ld = L.shape[2]
        else:
            L, R = np.ascontiguousarray(L), np.ascontiguousarray(R)
            ld = L.shape[2]
        outs = np.zeros(B, STEP_DTYPE)
        self._check(self.lib.vo_step_batch_ex(self.h, _p(L, C.c_uint8), _p(R, C.c_uint8), ld, 1 if col_major else 0, B,
                                              outs.ctypes.data_as(C.POINTER(StepOut))))
        return outs

    def step_batch_dev(self, d_lefts: int, d_rights: int, B: int) -> np.ndarray:
        outs = np.zeros(B, STEP_DTYPE)
        self._check(self.lib.vo_step_batch_dev(self.h, C.c_void_p(d_lefts), C.c_void_p(d_rights), B,
                                               outs.ctypes.data_as(C.POINTER(StepOut))))
        return outs

    def step_submit_dev(self, d_lefts: int, d_rights: int, B: int) -> None:
        """Pipelined step_batch_dev, device half (vo_step_submit_dev): returns at once."""
        self._check(self.lib.vo_step_submit_dev(self.h, C.c_void_p(d_lefts), C.c_void_p(d_rights), B))

    def step_collect(self) -> np.ndarray:
        """Outputs of the oldest submitted batch (vo_step_collect)."""
        outs = np.zeros(self.max_batch, STEP_DTYPE)
        n = C.c_int(0)
        self._check(self.lib.vo_step_collect(self.h, outs.ctypes.data_as(C.POINTER(StepOut)), self.max_batch, C.byref(n)))
        return outs[: n.value].copy()

    def steps_pending(self) -> int:
        return int(self.lib.vo_steps_pending(self.h))

    def fetch_tracks(self, frame: int) -> dict:
        """Visualisation data of `frame` of the last collected batch (vo_fetch_tracks):
        old_l / cur_l [K, 2] (1-based), world [K, 3], det [N, 2] (all current left detections)."""
        nt, nd = C.c_int(0), C.c_int(0)
        self._check(self.lib.vo_fetch_tracks(self.h, frame, None, None, None, None, 0, C.byref(nt), C.byref(nd)))
        cap = max(nt.value, nd.value, 1)
        old = np.zeros((cap, 2), np.float32)
        cur = np.zeros((cap, 2), np.float32)
        world = np.zeros((cap, 3))
        det = np.zeros((cap, 2), np.float32)
        self._check(self.lib.vo_fetch_tracks(self.h, frame, _p(old, C.c_float), _p(cur, C.c_float), _p(world, C.c_double),
                                             _p(det, C.c_float), cap, C.byref(nt), C.byref(nd)))
        k, n = nt.value, nd.value
        return {"old_l": old[:k].copy(), "cur_l": cur[:k].copy(), "world": world[:k].copy(), "det": det[:n].copy()}

    def fetch_track_quality(self, frame: int):
        """Quality of fetch_tracks(frame)'s rows, row for row (vo_fetch_track_quality): -> (old_r [K, 2]
        the old stereo pair's right-image positions, err float32 [K] mean reprojection distance of
        world[k] in pixels, valid bool [K] in front of both cameras), under the context's P1, P2."""
        nt = C.c_int(0)
        self._check(self.lib.vo_fetch_track_quality(self.h, frame, None, None, None, 0, C.byref(nt)))
        cap = max(nt.value, 1)
        old_r = np.zeros((cap, 2), np.float32)
        err = np.zeros(cap, np.float32)
        valid = np.zeros(cap, np.uint8)
        self._check(self.lib.vo_fetch_track_quality(self.h, frame, _p(old_r, C.c_float), _p(err, C.c_float),
                                                    _p(valid, C.c_uint8), cap, C.byref(nt)))
        k = nt.value
        return old_r[:k].copy(), err[:k].copy(), valid[:k].astype(bool)

    def step(self, left: np.ndarray, right: np.ndarray):
        return self.step_batch(left[None], right[None])[0]

    def get_landmarks(self) -> np.ndarray:
        rows = C.c_int(0)
        self._check(self.lib.vo_get_landmarks(self.h, None, 0, C.byref(rows)))
        out = np.zeros((max(rows.value, 1), 3))
        self._check(self.lib.vo_get_landmarks(self.h, _p(out, C.c_double), rows.value, C.byref(rows)))
        return out[: rows.value].copy()

    def set_landmark_frame(self, camera: bool):
        """Keep landmark rows in the camera frame (sharded sequences) instead of the world."""
        self._check(self.lib.vo_set_landmark_frame(self.h, 1 if camera else 0))

    def get_landmark_rows(self):
        """Camera-frame landmark rows appended so far -> (X [L, 3] float32, keep [L] bool)."""
        rows = C.c_int(0)
        self._check(self.lib.vo_get_landmark_rows(self.h, None, None, 0, C.byref(rows)))
        X = np.zeros((max(rows.value, 1), 3), np.float32)
        keep = np.zeros(max(rows.value, 1), np.uint8)
        self._check(self.lib.vo_get_landmark_rows(self.h, _p(X, C.c_float), _p(keep, C.c_uint8), rows.value,
                                                  C.byref(rows)))
        return X[: rows.value].copy(), keep[: rows.value].astype(bool)

    def landmark_row_count(self) -> int:
        """Camera-frame landmark rows held on the device (vo_set_landmark_frame(ctx, 1))."""
        rows = C.c_int(0)
        self._check(self.lib.vo_get_landmark_rows(self.h, None, None, 0, C.byref(rows)))
        return rows.value

    def landmarks_world_dev(self, poses, d_out: int, capacity: int) -> int:
        """CreateLandmarksFromFeatures.m:17 on the device (vo_landmarks_world_dev): the context's
        camera-frame rows moved to the world with poses[f], the chained world pose of its f-th
        collected frame, written as float32 [rows, 3] to device memory at d_out (e.g. a torch
        tensor's data_ptr(), `capacity` rows).  Returns the row count; d_out is ready on return."""
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        rows = C.c_long(0)
        self._check(self.lib.vo_landmarks_world_dev(self.h, _p(P, C.c_double), P.shape[0], C.c_void_p(d_out or None),
                                                    int(capacity), C.byref(rows)))
        return rows.value

    def reset(self):
        self._check(self.lib.vo_reset(self.h))

    def set_frame_index(self, idx: int):
        self._check(self.lib.vo_set_frame_index(self.h, idx))

    def set_calib(self, calib: Calib):
        self._check(self.lib.vo_set_calib(self.h, C.byref(calib)))

    # ---- profiling ----
    def set_profiling(self, on: bool):
        self._check(self.lib.vo_set_profiling(self.h, 1 if on else 0))

    def set_concurrency(self, n_streams: int):
        """Split each batch into n parts (1..4) pipelined over the scale-space and feature streams; results unchanged."""
        self._check(self.lib.vo_set_concurrency(self.h, int(n_streams)))

    def kernel_times(self) -> dict:
        n = C.c_int(0)
        self._check(self.lib.vo_kernel_times(self.h, None, None, None, 0, C.byref(n)))
        m = n.value
        names = (C.c_char_p * m)()
        ms = (C.c_double * m)()
        calls = (C.c_int * m)()
        self._check(self.lib.vo_kernel_times(self.h, names, ms, calls, m, C.byref(n)))
        return {names[i].decode(): (ms[i], calls[i]) for i in range(m)}

    def stream(self) -> int:
        return self.lib.vo_stream(self.h) or 0


def landmarks_to_world(pose, X, keep) -> np.ndarray:
    """CreateLandmarksFromFeatures.m:17 on camera-frame rows (vo_landmarks_to_world): rows with
    keep=False stay the reference's zero rows."""
    pose = np.ascontiguousarray(pose, np.float64).reshape(4, 4)
    X = np.ascontiguousarray(X, np.float32).reshape(-1, 3)
    k = np.ascontiguousarray(keep, np.uint8).reshape(-1)
    out = np.zeros((X.shape[0], 3))
    rc = load_library().vo_landmarks_to_world(_p(pose, C.c_double), _p(X, C.c_float), _p(k, C.c_uint8), X.shape[0],
                                               _p(out, C.c_double))
    if rc != VO_OK:
        raise VOError(rc, "vo_landmarks_to_world: bad arguments")
    return out


def chain_poses(rel, status=None, pose0=None) -> np.ndarray:
    """VO.m:130 world-pose chain (vo_chain_poses): frames with status != 0 hold the pose."""
    rel = np.ascontiguousarray(rel, np.float64).reshape(-1, 16)
    st = None if status is None else np.ascontiguousarray(status, np.int32).reshape(-1)
    p0 = None if pose0 is None else np.ascontiguousarray(pose0, np.float64).reshape(16)
    out = np.zeros((rel.shape[0], 16))
    rc = load_library().vo_chain_poses(_p(rel, C.c_double), None if st is None else _p(st, C.c_int32), rel.shape[0],
                                       None if p0 is None else _p(p0, C.c_double), _p(out, C.c_double))
    if rc != VO_OK:
        raise VOError(rc, "vo_chain_poses: bad arguments")
    return out.reshape(-1, 4, 4)


def landmarks_to_world_frames(poses, rows_per_frame, X, keep) -> np.ndarray:
    """CreateLandmarksFromFeatures.m:17 for a whole gathered sequence (vo_landmarks_to_world_frames)."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
    n = np.ascontiguousarray(rows_per_frame, np.int32).reshape(-1)
    X = np.ascontiguousarray(X, np.float32).reshape(-1, 3)
    k = np.ascontiguousarray(keep, np.uint8).reshape(-1)
    out = np.zeros((X.shape[0], 3))
    rc = load_library().vo_landmarks_to_world_frames(_p(poses, C.c_double), _p(n, C.c_int32), poses.shape[0],
                                                     _p(X, C.c_float), _p(k, C.c_uint8), X.shape[0], _p(out, C.c_double))
    if rc != VO_OK:
        raise VOError(rc, "vo_landmarks_to_world_frames: rows and per-frame counts disagree")
    return out


# ---------------------------------------------------------------------------
# MATLAB-named functional API (one shared default context per image size)
# ---------------------------------------------------------------------------
_ctx_cache: dict = {}


def _default_ctx(rows: int, cols: int) -> Context:
    key = (rows, cols)
    if key not in _ctx_cache:
        _ctx_cache[key] = Context(rows, cols, 1)
    return _ctx_cache[key]


def _sift_strongest(I: np.ndarray, strongest):
    """sift() of the default context with selectStrongest(points, strongest) for this call only."""
    ctx = _default_ctx(*I.shape)
    ctx.set_strongest(0 if strongest is None else strongest)
    try:
        return ctx.sift(I)
    finally:
        ctx.set_strongest(0)


def detectSIFTFeatures(I: np.ndarray, strongest: int | None = None):
    """detectSIFTFeatures(I) (VO.m:79-80) fused with its descriptor pass: returns
    (points, descriptors) where points is a structured array with MATLAB
    1-based Location (x, y), Scale, Orientation (angle), Metric (response).
    strongest=N is selectStrongest(detectSIFTFeatures(I), N): the N points of largest Metric,
    sorted, and only their descriptors computed."""
    return _sift_strongest(I, strongest)


def undistortImage(I: np.ndarray, K, radial=(0.0, 0.0, 0.0), tangential=(0.0, 0.0)) -> np.ndarray:
    """undistortImage(I, intrinsics) (VO.m:75-76): K is the 3x3 intrinsic matrix with the principal
    point in 0-based pixel indices, radial / tangential the intrinsics' RadialDistortion (2 or 3
    entries) and TangentialDistortion.  OutputView 'same', bilinear, FillValues 0."""
    I = np.asarray(I)
    return _default_ctx(*I.shape).undistort(I, K, radial, tangential)


def extractFeatures(I: np.ndarray, points=None, Method: str = "SIFT", strongest: int | None = None):
    """extractFeatures(I, points, "Method", "SIFT") (VO.m:83-84) -> (features, validPoints).
    With `points` (see as_keypoints) exactly those points are described, in their order
    (Context.describe): detections that were moved, rescaled or re-oriented, another detector's
    points, a grid; every point is valid, so validPoints is the given set.  `strongest` does not
    combine with given points (they are already chosen): VOError(VO_ERR_ARG).
    points=None detects as well: SIFT descriptors are computed in the same device pass as
    detection; strongest=N describes selectStrongest(points, N) only."""
    if Method != "SIFT":
        raise VOError(VO_ERR_ARG, "only Method 'SIFT' is on the hot path")
    if points is not None:
        if strongest is not None:
            raise VOError(VO_ERR_ARG, "extractFeatures: strongest applies to detection, not to given points")
        pts = as_keypoints(points)
        I = np.asarray(I)
        if I.ndim != 2 or I.dtype != np.uint8:
            raise VOError(VO_ERR_ARG, "extractFeatures: a 2-D uint8 image")
        return _default_ctx(*I.shape).describe(I, pts), pts
    kps, desc = _sift_strongest(I, strongest)
    return desc, kps


def matchFeatures(features1: np.ndarray, features2: np.ndarray, *, unique: bool = False, match_threshold: float | None = None,
                  max_ratio: float | None = None, return_metric: bool = False):
    """matchFeatures (Exhaustive, SSD; defaults MatchThreshold 1, MaxRatio 0.6, Unique false).
    Keywords as for Context.match; return_metric=True returns (indexPairs, matchMetric)."""
    return _default_ctx(375, 1242).match(features1, features2, unique=unique, match_threshold=match_threshold,
                                         max_ratio=max_ratio, return_metric=return_metric)


def matchFeaturesInRadius(features1: np.ndarray, features2: np.ndarray, points2, centerPoints, radius, *, unique: bool = False,
                          match_threshold: float | None = None, max_ratio: float | None = None, return_metric: bool = False):
    """matchFeaturesInRadius(features1, features2, points2, centerPoints, radius): matchFeatures
    restricted, for every row of features1, to the features2 rows whose point lies within `radius`
    (a scalar or one per row) of that row's centre.  points2 may be an n2 x 2 array or a keypoint
    array with fields x, y (what detectSIFTFeatures returns).  Keywords as for matchFeatures."""
    p2 = np.asarray(points2)
    if p2.dtype.names and "x" in p2.dtype.names:
        p2 = np.stack([p2["x"], p2["y"]], 1)
    return _default_ctx(375, 1242).match_in_radius(features1, features2, p2, centerPoints, radius, unique=unique,
                                                   match_threshold=match_threshold, max_ratio=max_ratio,
                                                   return_metric=return_metric)


def estimateFundamentalMatrix(matchedPoints1, matchedPoints2, Method: str = "MSAC", NumTrials: int = 500,
                              DistanceThreshold: float = 0.01, Confidence: float = 99.0, key: int = 0, **other):
    """[F, inliersIndex, status] = estimateFundamentalMatrix(matchedPoints1, matchedPoints2, Method=...,
    NumTrials=..., DistanceThreshold=..., Confidence=...) -> (F 3x3, inliersIndex [n] bool, status).
    Method "MSAC" or "Norm8Point"; "RANSAC", "LMedS", "LTS", DistanceType "Algebraic" and every other
    option are not implemented: VOError(VO_ERR_ARG).  status follows the toolbox: 0, 1 (fewer than 8
    points), 2 (not enough inliers); F is then zero."""
    if other.get("DistanceType", "Sampson") != "Sampson" or set(other) - {"DistanceType"}:
        raise VOError(VO_ERR_ARG, "estimateFundamentalMatrix: only Method, NumTrials, DistanceThreshold, Confidence and "
                                  "DistanceType 'Sampson' are implemented")
    if Method not in FUND_METHODS:
        raise VOError(VO_ERR_ARG, f"estimateFundamentalMatrix: Method {Method!r} is not implemented (MSAC, Norm8Point)")
    x1, x2 = fund_points(matchedPoints1, matchedPoints2, "estimateFundamentalMatrix")
    p = default_fund_params(method=FUND_METHODS[Method], num_trials=int(NumTrials), distance_threshold=float(DistanceThreshold),
                            confidence=float(Confidence))
    check_fund_params(p)
    rc, F, inl, _ = _default_ctx(375, 1242).est_fundamental(x1, x2, p, key)
    return F, inl, {VO_OK: 0, VO_ERR_TOO_FEW_POINTS: 1, VO_ERR_NO_CONSENSUS: 2}[rc]


class PointTracker:
    """vision.PointTracker's shape on a Context: initialize(points, I), then step(I) -> (points, validity,
    scores) carries the points from the previous image to I; set_points replaces them (and their
    validity).  Points that were lost stay where they were last seen and stay invalid, as the toolbox
    keeps them, until set_points."""

    def __init__(self, ctx: "Context", NumPyramidLevels: int = 3, BlockSize=(31, 31), MaxIterations: int = 30,
                 MaxBidirectionalError: float = float("inf")):
        self.ctx = ctx
        self.params = default_klt_params(num_pyramid_levels=int(NumPyramidLevels), block_size=BlockSize,
                                         max_iterations=int(MaxIterations), max_bidirectional_error=float(MaxBidirectionalError))
        check_klt_params(self.params)
        self.image = None
        self.points = np.zeros((0, 2), np.float32)
        self.validity = np.zeros(0, bool)

    def initialize(self, points, I) -> None:
        I = np.asarray(I, np.uint8)
        if I.shape != (self.ctx.rows, self.ctx.cols):
            raise VOError(VO_ERR_ARG, "PointTracker.initialize: a 2-D uint8 image of the context's size")
        self.image = I.copy()
        self.set_points(points)

    def set_points(self, points, validity=None) -> None:
        self.points = klt_points(points, "PointTracker.set_points").copy()
        self.validity = np.ones(len(self.points), bool) if validity is None else np.asarray(validity, bool).copy()
        if len(self.validity) != len(self.points):
            raise VOError(VO_ERR_ARG, "PointTracker.set_points: validity and points differ in length")

    def step(self, I):
        if self.image is None:
            raise VOError(VO_ERR_STATE, "PointTracker.step: initialize first")
        I = np.asarray(I, np.uint8)
        idx = np.flatnonzero(self.validity)
        pts, ok, sc, _ = self.ctx.track_points(self.image, I, self.points[idx], params=self.params)
        scores = np.zeros(len(self.points), np.float32)
        self.points[idx] = pts
        self.validity[idx] = ok
        scores[idx] = sc
        self.image = I.copy()
        return self.points.copy(), self.validity.copy(), scores


def _detect_corners(I, method: int, MinQuality: float, FilterSize: int, ROI):
    I = np.asarray(I)
    if I.ndim != 2 or I.dtype != np.uint8:
        raise VOError(VO_ERR_ARG, "a 2-D uint8 image")
    p = default_corner_params(method=method, min_quality=float(MinQuality), filter_size=int(FilterSize), roi=ROI)
    return _default_ctx(*I.shape).detect_corners(I, p)


def detectMinEigenFeatures(I, MinQuality: float = 0.01, FilterSize: int = 5, ROI=None):
    """detectMinEigenFeatures(I, MinQuality = , FilterSize = , ROI = ) -> (Location [n][2] (x, y) 1-based, Metric [n]):
    Shi-Tomasi corners, the points vision.PointTracker is initialised with."""
    return _detect_corners(I, VO_CORNER_MINEIG, MinQuality, FilterSize, ROI)


def detectHarrisFeatures(I, MinQuality: float = 0.01, FilterSize: int = 5, ROI=None):
    """detectHarrisFeatures(I, MinQuality = , FilterSize = , ROI = ) -> (Location, Metric): Harris-Stephens corners,
    det - 0.04 trace^2 of the same smoothed gradient matrix."""
    return _detect_corners(I, VO_CORNER_HARRIS, MinQuality, FilterSize, ROI)


def disparitySGM(I1, I2, DisparityRange=(0, 128), UniquenessThreshold: int = 15):
    """disparityMap = disparitySGM(I1, I2, DisparityRange = , UniquenessThreshold = ) of a rectified pair: semi-global
    matching on a census cost -> [rows, cols] float32, NaN where unreliable."""
    I1, I2 = np.asarray(I1), np.asarray(I2)
    if I1.ndim != 2 or I1.dtype != np.uint8 or I2.shape != I1.shape or I2.dtype != np.uint8:
        raise VOError(VO_ERR_ARG, "two 2-D uint8 images of one size")
    p = default_sgm_params(disparity_range=DisparityRange, uniqueness_threshold=int(UniquenessThreshold))
    return _default_ctx(*I1.shape).disparity_sgm(I1, I2, p)


def reconstructScene(disparityMap, reprojectionMatrix):
    """xyzPoints = reconstructScene(disparityMap, reprojectionMatrix) -> [rows, cols, 3] float32."""
    d = np.asarray(disparityMap, np.float32)
    if d.ndim != 2:
        raise VOError(VO_ERR_ARG, "a 2-D disparity map")
    return _default_ctx(*d.shape).reconstruct_scene(d, reprojectionMatrix)
