"""Reference of SIFTPoints.selectStrongest(points, N) as libvo applies it between
detectSIFTFeatures and extractFeatures (vo_set_strongest), and the VO.m loop restated over the
oracle's per-call functions so the selection can be inserted after `sift`.

select(): detections in detection order (the order oracle.sift returns them), stably sorted by
response descending, the first min(N, count) kept.  The result is in sorted order also when
N >= count.

loop(): oracle/vo_ref.c's oracle_run_sequence call by call (sift, match, track, triangulate,
estworldpose, landmarks).  With N=None it equals oracle.run_sequence bit for bit
(tests/test_strongest.py checks that), so loop(N) is the loop body with the selection and
nothing else changed."""
import numpy as np

import oracle

VO_OK = 0


def order(kps, N):
    """Row indices of selectStrongest(points, N): (response descending, detection index ascending)."""
    return np.argsort(-kps["response"], kind="stable")[:N]


def select(kps, desc, N):
    o = order(kps, N)
    return kps[o], desc[o]


def mat4_mul(A, B):
    """vo_ref.c mat4_mul: T[i][j] = ((A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j]) + A[i][3] B[3][j]"""
    return A[:, 0:1] * B[0] + A[:, 1:2] * B[1] + A[:, 2:3] * B[2] + A[:, 3:4] * B[3]


def _xy(kps, idx):
    return np.stack([kps["x"][idx], kps["y"][idx]], axis=1).astype(np.float32).reshape(-1, 2)


def detect(L, R):
    """[(oracle.sift(L[f]), oracle.sift(R[f]))]: the detections loop() starts from, so several
    loops over one sequence (different N) share them."""
    return [(oracle.sift(l), oracle.sift(r)) for l, r in zip(L, R)]


def loop(L, R, P1, P2, N=None, key0=0, feats=None):
    """-> (outs [F] oracle.STEP_DTYPE, landmarks [rows, 3] world): the VO.m loop (VO.m:64-232) with
    selectStrongest(points, N) after each image's detection (N=None: none).  feats: detect(L, R),
    computed here when omitted."""
    P1 = np.ascontiguousarray(P1, np.float64)
    P2 = np.ascontiguousarray(P2, np.float64)
    K = np.ascontiguousarray(P1[:, :3])
    F = len(L)
    outs = np.zeros(F, oracle.STEP_DTYPE)
    pose = np.eye(4)
    lms = []
    feat = None                                   # (fl_pos, fr_pos, fl_desc, fr_desc) of the previous frame
    for f in range(F):
        (kl, dl), (kr, dr) = feats[f] if feats is not None else (oracle.sift(L[f]), oracle.sift(R[f]))
        if N is not None:
            kl, dl = select(kl, dl, N)
            kr, dr = select(kr, dr, N)
        pairs = oracle.match(dl, dr)
        a, b = pairs[:, 0].astype(np.int64) - 1, pairs[:, 1].astype(np.int64) - 1
        sl, sr = _xy(kl, a), _xy(kr, b)           # stereo subset (VO.m:141-144 / 207-210)
        o = outs[f]
        o["n_left"], o["n_right"], o["n_stereo"] = len(kl), len(kr), len(pairs)
        o["rel_pose"] = np.eye(4)
        if feat is not None:
            fl_pos, fr_pos, fl_desc, fr_desc = feat
            t = oracle.track(fl_desc, fr_desc, dl, dr)
            oi, ci = t[:, 0].astype(np.int64) - 1, t[:, 1].astype(np.int64) - 1
            ol, orr = fl_pos[oi].reshape(-1, 2), fr_pos[oi].reshape(-1, 2)
            img = _xy(kl, ci).astype(np.float64)
            wld = oracle.triangulate(ol, orr, P1, P2)
            st, T, _, nin = oracle.estworldpose(img, wld, K, None, key0 + f)
            o["n_tracked"], o["status"], o["n_inliers"] = len(t), st, nin
            if st == VO_OK:
                o["rel_pose"] = T
                pose = mat4_mul(pose, T)
            rows = oracle.landmarks(sl, sr, ol, orr, P1, P2, pose)    # the pose after the update
            o["n_landmarks"] = len(rows)
            lms.append(rows)
        o["pose"] = pose
        feat = (sl, sr, dl[a], dr[b])             # features = stereo subset (VO.m:225-230)
    return outs, (np.concatenate(lms) if lms else np.zeros((0, 3)))


def tie_image():
    """128 x 192: identical 32 x 32 tiles (4 x 4 blocks of an 8 x 8 random pattern), so keypoints
    at shifts that are multiples of 32 repeat with bit-equal responses."""
    base = np.random.default_rng(3).integers(0, 256, (8, 8)).astype(np.uint8)
    return np.tile(np.kron(base, np.ones((4, 4), np.uint8)), (4, 6))


def cut_kinds(kps):
    """(tie cuts, multi-peak cuts) of the sorted order: cut positions N (1 <= N < count) between
    two different candidates of equal response, and inside one candidate's orientation peaks."""
    o = order(kps, len(kps))
    s = kps[o]
    same_resp = s["response"][:-1] == s["response"][1:]
    same_cand = same_resp & (o[1:] == o[:-1] + 1)
    for k in ("x", "y", "size", "octave", "layer"):
        same_cand &= s[k][:-1] == s[k][1:]
    return int((same_resp & ~same_cand).sum()), int(same_cand.sum())
