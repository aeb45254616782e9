"""CPU: the reference of vo_refine_pose (tests/pose_refine_ref: include/vo_spec.h's vo_refine_*
functions, which k_refine_pose calls, summed in the normative order) against an independent
evaluation written here and in pose_refine_ref.minimise_longdouble from the definitions
(numpy.longdouble, Rodrigues exponential, plain Gauss-Newton to a fixed point).

Measured on the development machine (x86-64, gcc -O2 -ffp-contract=off), geom_ref.pose_err to the
planted pose / to the longdouble minimiser, worst of the three seeds of each n:

  (a) noise-free, start 0.3 deg / 5 cm off          reference      longdouble
      n = 3                                          6.93e-13       6.02e-13
      n = 4                                          1.70e-14       7.04e-15
      n = 6                                          7.77e-15       2.00e-15
      n = 65                                         1.94e-15       8.88e-16
  (b) 0.2 px noise: |reference - longdouble minimiser|, relative cost difference
      n = 64                                         1.25e-11       3.5e-14
      n = 129                                        1.23e-11       1.6e-14
      n = 500                                        3.63e-11       2.3e-14

Three points determine the pose with no redundancy, so n = 3 carries the conditioning of the P3P
problem (both evaluations are off by the same 6e-13: it is the rounding of the f64 pixel inputs).
In (b) the reference stops once a step lowers the cost by less than 1e-9 of it, the minimiser runs
on: their distance is what that stop leaves.  The asserted bounds are 100 x the reference column.
(d): the median pose_err over the 20 seeds was 9.2e-3 before and 7.9e-4 after refinement."""
import numpy as np
import pytest

import geom_ref as G
import pose_refine_ref as P

MEASURED_A = {3: 6.93e-13, 4: 1.70e-14, 6: 7.77e-15, 65: 1.94e-15}
MEASURED_B = {64: 1.25e-11, 129: 1.23e-11, 500: 3.63e-11}
MARGIN = 100.0


def check_invariants(T0, T, st, max_iterations=20):
    """(c): what holds exactly in every case."""
    assert st["cost_final"] <= st["cost_initial"]
    assert st["accepted"] <= st["passes"] - 1 <= max_iterations - 1
    R = T[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
    assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    if st["accepted"] == 0:
        assert T.tobytes() == np.ascontiguousarray(T0, np.float64).tobytes()
        assert st["cost_final"] == st["cost_initial"]


def _case(tag, n, seed, noise):
    rng = np.random.default_rng([tag, n, seed])
    uv, Xw, K = G.pose_problem(rng, n, 0.0, noise=noise)
    return uv, Xw, K, P.start_pose(rng, 0.3, 0.05)


@pytest.mark.parametrize("n", [3, 4, 6, 65])
def test_noise_free_reaches_the_planted_pose(n):
    for seed in range(3):
        uv, Xw, K, T0 = _case(0xA, n, seed, 0.0)
        T, st = P.refine(uv, Xw, T0, K)
        check_invariants(T0, T, st)
        R, t, _ = P.minimise_longdouble(uv, Xw, T0, K)
        e_ref, e_ld = P.pose_err_T(T), G.pose_err(R, t, P.PLANTED_R, P.PLANTED_T)
        print(f"n {n} seed {seed}: reference {e_ref:.3g} longdouble {e_ld:.3g} {st}")
        assert st["n_used"] == n and st["status"] in (P.CONVERGED, P.MAX_ITER, P.DAMPING)
        assert e_ref <= MARGIN * MEASURED_A[n]
        assert e_ld <= MARGIN * MEASURED_A[n]


@pytest.mark.parametrize("n", [64, 129, 500])
def test_noisy_agrees_with_the_longdouble_minimiser(n):
    for seed in range(3):
        uv, Xw, K, T0 = _case(0xB, n, seed, 0.2)
        T, st = P.refine(uv, Xw, T0, K)
        check_invariants(T0, T, st)
        R, t, c = P.minimise_longdouble(uv, Xw, T0, K)
        Rr, tr = P.from_T(T)
        d = G.pose_err(Rr, tr, R, t)
        rel = abs(st["cost_final"] - c) / c
        print(f"n {n} seed {seed}: pose difference {d:.3g}, relative cost difference {rel:.3g} {st}")
        assert st["status"] == P.CONVERGED
        assert d <= MARGIN * MEASURED_B[n]
        assert rel <= 1e-6
        # the reported costs are the sums of squared residuals at the two poses
        assert abs(st["cost_initial"] - P.cost_ld(T0, uv, Xw, K)) <= 1e-12 * st["cost_initial"]
        assert abs(st["cost_final"] - P.cost_ld(T, uv, Xw, K)) <= 1e-12 * st["cost_final"]


def test_sums_are_the_normal_equations():
    """One pass against J^T J, J^T r and r^T r of a numerical Jacobian (central differences of the
    residuals under the left perturbation), on a skewed K and a `use` mask."""
    rng = np.random.default_rng(0x5A5)
    uv, Xw, _ = G.pose_problem(rng, 70, 0.0, noise=0.5)
    K = np.array([[700.0, 1.5, 600.0], [0.0, 705.0, 190.0], [0.0, 0.0, 1.0]])
    uv = G.project(K, P.PLANTED_R, P.PLANTED_T, Xw) + rng.normal(0, 0.5, uv.shape)
    use = rng.random(70) < 0.7
    T0 = P.start_pose(rng, 0.3, 0.05)
    s, n_used = P.sums(uv, Xw, T0, K, use)
    assert n_used == int(use.sum())
    R0, t0 = P.from_T(T0)

    def res(d):
        dR = G.rodrigues(d[:3], np.linalg.norm(d[:3])) if np.any(d[:3]) else np.eye(3)
        return (G.project(K, dR @ R0, dR @ t0 + d[3:], Xw[use]) - uv[use]).reshape(-1)

    h = 1e-6
    J = np.stack([(res(h * e) - res(-h * e)) / (2 * h) for e in np.eye(6)], 1)
    r = res(np.zeros(6))
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = s[:21]
    H = H + np.triu(H, 1).T
    assert np.abs(H - J.T @ J).max() <= 1e-6 * np.abs(H).max()
    assert np.abs(s[21:27] - J.T @ r).max() <= 1e-6 * np.abs(s[21:27]).max()
    assert abs(s[27] - r @ r) <= 1e-12 * s[27]


@pytest.mark.parametrize("max_iterations", [1, 2, 5])
def test_iteration_cap(max_iterations):
    uv, Xw, K, T0 = _case(0xB, 129, 0, 0.2)
    T, st = P.refine(uv, Xw, T0, K, max_iterations=max_iterations)
    check_invariants(T0, T, st, max_iterations)
    if max_iterations <= 2:
        assert st["status"] == P.MAX_ITER and st["passes"] == max_iterations and st["accepted"] == max_iterations - 1


def test_too_few_returns_the_input_pose_by_bytes():
    uv, Xw, K, T0 = _case(0xB, 64, 1, 0.2)
    behind = np.zeros(64, bool)
    for name, args in (("use all zero", (uv, Xw, np.zeros(64, bool))),
                       ("two used", (uv, Xw, np.arange(64) % 40 == 3)),
                       ("n = 2", (uv[:2], Xw[:2], None)),
                       ("n = 0", (uv[:0], Xw[:0], None))):
        T, st = P.refine(args[0], args[1], T0, K, use=args[2])
        print(name, st)
        check_invariants(T0, T, st)
        assert st["status"] == P.TOO_FEW and st["accepted"] == 0 and st["passes"] == 1
        assert T.tobytes() == T0.tobytes()
        assert st["n_used"] == (0 if args[2] is not None and not args[2].any() else min(2, len(args[0])))
    # points at or behind the camera plane at the start are not in U: three used points remain
    Xw2 = Xw.copy()
    R0, t0 = P.from_T(T0)
    behind[3:] = True
    Xw2[behind] = (np.array([0.5, 0.1, -2.0]) - t0) @ R0          # camera-frame z = -2 at the start
    T, st = P.refine(uv, Xw2, T0, K)
    check_invariants(T0, T, st)
    assert st["n_used"] == 3 and st["status"] != P.TOO_FEW


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_candidate_that_puts_a_used_point_behind_the_camera_is_rejected(seed):
    """A point 0.05 m in front of the planted camera, a start 1 m behind it: the first step --
    recomputed here in numpy from the pass's sums -- overshoots and carries that point behind the
    camera plane, so the reference must reject it: fewer accepted than trial passes, and it still
    ends at the minimum."""
    uv, Xw, K, T0 = P.behind_case(seed)
    s, n_used = P.sums(uv, Xw, T0, K)
    assert n_used == 40
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = s[:21]
    H = H + np.triu(H, 1).T
    d = np.linalg.solve(H + 1e-3 * np.diag(np.diag(H)), -s[21:27])
    R0, t0 = P.from_T(T0)
    dR = G.rodrigues(d[:3], np.linalg.norm(d[:3]))
    z = ((dR @ R0) @ Xw[0] + dR @ t0 + d[3:])[2]
    assert z < -0.01, z
    T, st = P.refine(uv, Xw, T0, K)
    check_invariants(T0, T, st)
    print(f"seed {seed}: first candidate z = {z:.3f}, {st}")
    assert st["accepted"] < st["passes"] - 1
    R, t, c = P.minimise_longdouble(uv, Xw, P.to_T(P.PLANTED_R, P.PLANTED_T), K)
    assert abs(st["cost_final"] - c) <= 1e-6 * c


def test_refinement_on_the_msac_mask_improves_the_pose(oracle):
    """(d): 20 seeds of 300 points, 30 % outliers, 0.2 px noise; estworldpose as the oracle runs it
    (geom_ref.msac_replay), then the refinement on its inlier mask.  The median error to the planted
    pose must drop."""
    before, after = [], []
    for seed in range(20):
        rng = np.random.default_rng([0xD, seed])
        uv, Xw, K = G.pose_problem(rng, 300, 0.3, noise=0.2)
        res = G.msac_replay(oracle, uv, Xw, K, frame_key=seed)
        assert res["status"] == 0
        T, st = P.refine(uv, Xw, res["T"], K, use=res["mask"])
        check_invariants(res["T"], T, st)
        assert st["n_used"] == res["n_inliers"]
        before.append(P.pose_err_T(res["T"]))
        after.append(P.pose_err_T(T))
    print(f"median pose_err before {np.median(before):.3g}, after {np.median(after):.3g}")
    assert np.median(after) < np.median(before)
