"""selectStrongest (vo_set_strongest) on the CPU: the reference the GPU tests compare with
(tests/strongest_ref.py) is pinned to the oracle, the tie fixture is shown to have the ties and
straddled orientation groups it is there for, and the MEX gateway's 'strongest' command is
checked against a libvo that lacks vo_set_strongest."""
import numpy as np
import pytest

import mexshim
import strongest_ref as sr

STEP_FIELDS = ("status", "n_left", "n_right", "n_stereo", "n_tracked", "n_inliers", "n_landmarks", "flags", "rel_pose", "pose")


@pytest.fixture(scope="module")
def seq(syn):
    L, R, _ = syn.sequence(5, 188, 621, scale=0.5)
    P1, P2 = syn.calib(0.5)
    return L, R, P1, P2


def test_loop_without_selection_is_the_oracle_sequence(oracle, seq):
    L, R, P1, P2 = seq
    ref_outs, ref_lm = oracle.run_sequence(L, R, P1, P2)
    outs, lm = sr.loop(L, R, P1, P2)
    for k in STEP_FIELDS:
        assert np.array_equal(outs[k], ref_outs[k]), k
    assert len(ref_lm) > 1000 and lm.shape == ref_lm.shape and np.array_equal(lm, ref_lm)
    assert (ref_outs["status"][1:] == 0).all()


def test_selection_is_per_image_so_a_shard_equals_the_whole_run(oracle, seq):
    """Frames [2, 5) with the halo frame 2 and the MSAC key of the global frame index give the
    records of frames 3, 4 of the whole run (what kitti.run_shard relies on)."""
    L, R, P1, P2 = seq
    whole, _ = sr.loop(L, R, P1, P2, N=150)
    assert (whole["status"][1:] == 0).all() and (whole["n_left"] == 150).all() and (whole["n_tracked"][1:] >= 40).all()
    part, _ = sr.loop(L[2:], R[2:], P1, P2, N=150, key0=2)
    for k in ("status", "n_left", "n_right", "n_stereo", "n_tracked", "n_inliers", "n_landmarks", "rel_pose"):
        assert np.array_equal(part[k][1:], whole[k][3:]), k


def test_select_is_the_stable_descending_sort(oracle):
    kps, desc = oracle.sift(sr.tie_image())
    n = len(kps)
    for N in (1, 7, n - 1, n, n + 1, 16384):
        k, d = sr.select(kps, desc, N)
        assert len(k) == min(N, n) and len(d) == len(k)
        assert (np.diff(k["response"]) <= 0).all()
    k, d = sr.select(kps, desc, n)
    o = sr.order(kps, n)
    assert sorted(o.tolist()) == list(range(n)) and not np.array_equal(o, np.arange(n))   # a permutation, not the identity
    ties = k["response"][:-1] == k["response"][1:]
    assert (o[1:][ties] > o[:-1][ties]).all()                     # equal responses keep detection order


def test_tie_fixture_has_ties_and_straddled_peaks(oracle):
    """Measured with the oracle: 692 keypoints, 421 cut positions between two different
    candidates of equal response, 221 inside a multi-peak candidate."""
    kps, desc = oracle.sift(sr.tie_image())
    assert kps["response"].min() >= 0 and np.isfinite(kps["response"]).all()
    n_tie, n_peak = sr.cut_kinds(kps)
    print(f"tie image: {len(kps)} keypoints, {n_tie} tie cuts, {n_peak} multi-peak cuts")
    assert n_tie >= 100 and n_peak >= 50
    # a wrong tie rule is visible: highest-index-first picks other descriptors at most cuts
    o = sr.order(kps, len(kps))
    rev = np.lexsort((-np.arange(len(kps)), -kps["response"].astype(np.float64)))
    differs = sum(not np.array_equal(desc[np.sort(o[:N])], desc[np.sort(rev[:N])]) for N in range(1, len(kps)))
    print(f"highest-index-first tie rule: another descriptor set at {differs} of {len(kps) - 1} cuts")
    assert differs >= 100


IMG = np.zeros((20, 30), np.uint8)


def test_mex_strongest_unavailable_against_an_older_libvo():
    """The fake libvo has no vo_set_strongest: the gateway still loads (weak reference), raises
    vo:selectStrongest:unavailable for the command and serves the others."""
    mexshim.build()
    m = mexshim.Mex(mexshim.FAKE)
    try:
        with pytest.raises(mexshim.MexError) as e:
            m.call("strongest", np.float64(100), nout=0)
        assert e.value.ident == "vo:selectStrongest:unavailable"
        with pytest.raises(mexshim.MexError) as e:
            m.call("strongest", np.float64(0), nout=0)
        assert e.value.ident == "vo:selectStrongest:unavailable"
        for bad in (np.float64(-1), np.float64(2.5), np.float64(1e9), np.uint8(3)):
            with pytest.raises(mexshim.MexError) as e:
                m.call("strongest", bad, nout=0)
            assert e.value.ident == "vo:badArgument"
        with pytest.raises(mexshim.MexError) as e:
            m.call("strongest", nout=0)
        assert e.value.ident == "vo:nargin"
        # every other command still works with that libvo
        assert m.call("sift", IMG, nout=1).shape == (5, 2)
        rng = np.random.default_rng(2)
        F1 = rng.integers(0, 256, (7, 128)).astype(np.float32)
        F2 = rng.integers(0, 256, (6, 128)).astype(np.float32)
        assert m.call("match", F1, F2).dtype == np.uint32
        x = rng.uniform(0, 100, (4, 2)).astype(np.float32)
        assert m.call("triangulate", x, x, rng.normal(size=(3, 4)), rng.normal(size=(3, 4))).shape == (4, 3)
        rel, A, st, nl = m.call("step", IMG, IMG, rng.normal(size=(3, 4)), rng.normal(size=(3, 4)), nout=4)
        assert rel.shape == (4, 4) and A.shape == (4, 4)
        K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]])
        A, inl, st = m.call("estworldpose", rng.uniform(0, 1000, (6, 2)), rng.normal(size=(6, 3)), K, nout=3)
        assert A.shape == (4, 4) and st[0, 0] == 0
        assert m.call("landmarks", x, x, rng.normal(size=(3, 4)), rng.normal(size=(3, 4)), np.eye(4)).shape[1] == 3
        m.call("landmarks_all")
        m.call("reset", nout=0)
        m.call("close", nout=0)
    finally:
        m.at_exit()
