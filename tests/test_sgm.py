"""disparitySGM / reconstructScene on the CPU: tests/sgm_ref (the CPU build of include/vo_spec.h's vo_sgm_* /
vo_reconstruct_* functions, which the device is held to by bytes in test_gpu_sgm.py) against tests/sgm_np_ref.py,
an independent NumPy restatement; the reprojection matrix; reconstructScene against the oracle's DLT triangulate;
the census of branches the table reaches; the quality of the spec on rendered scenes; the same C under
AddressSanitizer and UBSan as a stand-alone program."""
import subprocess

import numpy as np
import pytest

import sgm_np_ref as N
import sgm_ref as R

TABLE = R.TABLE


@pytest.mark.parametrize("i", range(len(TABLE)), ids=[c["name"] for c in TABLE])
def test_reference_equals_the_numpy_restatement(i):
    c = TABLE[i]
    left, right = R.pair(c["kind"], c["rows"], c["cols"], c["dmin"], c["D"])
    S, disp = N.disparity(left, right, c["dmin"], c["D"], c["P1"], c["P2"], c["U"])
    r = R.result(i)
    assert r["S"].tobytes() == S.tobytes()
    assert r["disp"].tobytes() == disp.tobytes()
    assert int(r["S"].max()) <= 8 * (62 + c["P2"])


def test_census_words():
    img = np.random.default_rng(5).integers(0, 256, (19, 23)).astype(np.uint8)
    assert R.census(img).tobytes() == N.census(img).tobytes()
    assert int(R.census(img).max()) < 1 << 62
    assert not R.census(np.full((9, 12), 77, np.uint8)).any()


def test_step_and_select_at_their_edges():
    # the four arguments of the inner minimum, one at a time
    assert R.step(7, 5, 9, 9, 5, 10, 120) == 7              # L(k) itself (it is the minimum: - m leaves 0)
    assert R.step(7, 40, 5, 40, 5, 10, 120) == 7 + 10       # L(k - 1) + P1
    assert R.step(7, 40, 40, 5, 5, 10, 120) == 7 + 10       # L(k + 1) + P1
    assert R.step(7, 200, 200, 200, 5, 10, 120) == 7 + 120  # m + P2
    assert R.step(62, 317, 0x3FFF, 0x3FFF, 317, 255, 255) == 62                 # both neighbours absent
    # the selection: lowest k on ties; the offset of +0.5 when the upper neighbour ties; k* at either end
    S = np.array([9, 5, 5, 9, 9, 9, 9, 9], np.uint16)
    assert R.select(S, 0, 20, 64, 0) == np.float32(1.5)
    assert R.select(S[::-1].copy(), 0, 20, 64, 0) == np.float32(5.5)            # 9 9 9 9 9 5 5 9: k* = 5, S(6) ties
    assert R.select(np.array([1, 5, 9, 9, 9, 9, 9, 9], np.uint16), -3, 20, 64, 0) == np.float32(-3.0)
    assert R.select(np.array([9, 9, 9, 9, 9, 9, 5, 1], np.uint16), 0, 20, 64, 0) == np.float32(7.0)
    # uniqueness: v = 9 (k = 0 and 2 are within one of k* = 1): 100 * 9 < (100 + U) * 8 from U = 13 on
    T = np.array([9, 8, 9, 9, 9, 9, 9, 9], np.uint16)
    assert R.select(T, 0, 20, 64, 12) == np.float32(1.0) and np.isnan(R.select(T, 0, 20, 64, 13))
    # validity: the matched column x - d outside 0 .. cols - 1
    assert np.isnan(R.select(S, 0, 0, 64, 0)) and R.select(S, 0, 1, 64, 0) == np.float32(1.5)
    assert np.isnan(R.select(S, -4, 61, 64, 0)) and R.select(S, -4, 60, 64, 0) == np.float32(-2.5)
    assert R.select(np.zeros(8, np.uint16), 0, 5, 64, 100) == np.float32(0.0)   # V == 0 is never unreliable
    nan = R.select(S, 0, 0, 64, 0)
    assert np.array([nan]).view(np.uint32)[0] == R.NAN_BITS


def test_reprojection_matrix_and_its_refusals(syn):
    P0, P1 = syn.calib(1.0)
    rc, Q = R.reprojection(P0, P1)
    b = 386.1448 / 718.856
    assert rc == 0
    assert np.array_equal(Q, np.array([[1, 0, 0, -607.1928], [0, 1, 0, -185.2157], [0, 0, 0, 718.856], [0, 0, 1 / b, -0.0 / b]]))
    P2 = P1.copy(); P2[0, 2] = 600.0; P2[1, 1] = 2 * 718.856
    P0b = P0.copy(); P0b[1, 1] = 2 * 718.856
    rc, Q = R.reprojection(P0b, P2)
    assert rc == 0 and Q[1, 1] == 0.5 and Q[1, 3] == -0.5 * 185.2157 and Q[3, 3] == -(607.1928 - 600.0) / b
    bad = []
    for k in (1, 3, 4, 7, 8, 9, 11):
        A = P0.copy().reshape(-1); A[k] = 0.5; bad.append((A, P1))
        if k != 3:
            B = P1.copy().reshape(-1); B[k] = 0.5; bad.append((P0, B))
    B = P1.copy(); B[0, 3] = 0.0; bad.append((P0, B))                 # no baseline
    B = P1.copy(); B[2, 2] = 2.0; bad.append((P0, B))
    A = P0.copy(); A[2, 2] = 2.0; bad.append((A, P1))
    B = P1.copy(); B[0, 0] = 700.0; bad.append((P0, B))               # fx differs
    B = P1.copy(); B[1, 1] = 700.0; bad.append((P0, B))               # fy differs
    B = P1.copy(); B[1, 2] = 180.0; bad.append((P0, B))               # cy differs
    B = P1.copy(); B[0, 3] = np.nan; bad.append((P0, B))
    B = P1.copy(); B[0, 2] = np.inf; bad.append((P0, B))
    for A, B in bad:
        assert R.reprojection(A, B)[0] == -1


def test_vo_reprojection_matrix_is_the_reference(vo, syn):
    P0, P1 = syn.calib(0.25)
    assert vo.reprojection_matrix(P0, P1).tobytes() == R.reprojection(P0, P1)[1].tobytes()
    with pytest.raises(vo.VOError) as e:
        vo.reprojection_matrix(P1, P1)
    assert e.value.code == vo.VO_ERR_ARG
    with pytest.raises(vo.VOError):
        vo.reprojection_matrix(P0[:, :3], P1)


def _ulps(a, b):
    """the distance of two float32 arrays of one sign pattern in units of the last place"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def test_reconstruct_scene_agrees_with_the_oracles_triangulate(oracle, syn):
    """Integer disparities under KITTI-00's P0 / P1: the DLT triangulation of (x, y), (x - d, y) is the same point.
    Both are single roundings of values accurate far below an ulp of single, so they differ by a rounding flip at
    the most: 1 ulp per coordinate."""
    P0, P1 = syn.calib(1.0)
    rc, Q = R.reprojection(P0, P1)
    rows, cols = 24, 40
    rng = np.random.default_rng(3)
    disp = rng.integers(1, 128, (rows, cols)).astype(np.float32)
    xyz = R.reconstruct(disp, Q)
    assert xyz.tobytes() == N.reconstruct(disp, Q).tobytes()
    y, x = np.mgrid[1:rows + 1, 1:cols + 1]
    # anywhere in a KITTI image: shift the block's coordinates through Q's last column instead of a large map
    for ox, oy in ((0, 0), (1200, 350), (600, 180)):
        Qs = Q.copy()
        Qs[0, 3] += ox; Qs[1, 3] += oy
        got = R.reconstruct(disp, Qs)
        x1 = np.stack([x + ox, y + oy], -1).reshape(-1, 2).astype(np.float32)
        x2 = x1.copy(); x2[:, 0] -= disp.reshape(-1)
        X = oracle.triangulate(x1, x2, P0, P1).astype(np.float32).reshape(rows, cols, 3)
        assert (np.sign(X) == np.sign(got)).all()
        assert int(_ulps(X, got).max()) <= 1
    nan = disp.copy(); nan[3, 5] = np.nan
    out = R.reconstruct(nan, Q)
    assert (out[3, 5].view(np.uint32) == R.NAN_BITS).all() and not np.isnan(np.delete(out.reshape(-1, 3), 3 * cols + 5, 0)).any()
    # both storage orders hold the same numbers
    F = R.reconstruct(np.asfortranarray(disp), Q)
    assert F.flags.f_contiguous and np.array_equal(F, xyz)


def test_the_table_reaches_every_branch():
    n = np.zeros(R.N_COUNTERS, np.int64)
    per_case = []
    for i in range(len(TABLE)):
        per_case.append(R.result(i)["counters"])
        n += per_case[-1]
    for q in range(8):
        assert n[R.C_FIRST + q] > 0, q                                         # a path's first pixel, every direction
        for a in range(4):
            assert n[R.C_ARG + 4 * q + a] > 0, (q, a)                          # every argument of the inner min chosen
    assert n[R.C_NO_LOWER] > 0 and n[R.C_NO_UPPER] > 0
    assert n[R.C_TIE] > 0 and n[R.C_K_FIRST] > 0 and n[R.C_K_LAST] > 0
    assert n[R.C_PLUS_HALF] > 0 and n[R.C_SUBPIXEL] > n[R.C_PLUS_HALF]
    # The lowest k wins a tie, so S(k* - 1) > V strictly: den = 2 ((S(k* - 1) - V) + (S(k* + 1) - V)) > 0 at every
    # interior winner and the offset lies in (-0.5, 0.5].  den == 0 and -0.5 cannot occur; the census says so.
    assert n[R.C_DEN_ZERO] == 0 and n[R.C_MINUS_HALF] == 0
    assert n[R.C_INVALID_LEFT] > 0 and n[R.C_INVALID_RIGHT] > 0
    assert n[R.C_UNRELIABLE] > 0 and n[R.C_V_ZERO] > 0 and n[R.C_RETURNED] > 0
    for c, k in zip(TABLE, per_case):
        if c["dmin"] >= 0:
            assert k[R.C_INVALID_RIGHT] == 0, c["name"]                        # only negative disparities leave by the right
        if c["U"] == 0:
            assert k[R.C_UNRELIABLE] == 0, c["name"]                           # v < V cannot happen
        if c["kind"] == "flat":
            assert k[R.C_V_ZERO] == c["rows"] * c["cols"] and k[R.C_UNRELIABLE] == 0, c["name"]
        if c["kind"] == "stripes" and c["D"] >= 16 and c["U"] >= 15:
            assert k[R.C_UNRELIABLE] > 0, c["name"]                            # the period of 8 lies inside the range
    by = {c["name"]: k for c, k in zip(TABLE, per_case)}
    assert by["37x53_D16_-4_stripes_U100"][R.C_UNRELIABLE] > by["37x53_D16_-4_stripes"][R.C_UNRELIABLE]


# ---- quality, on the reference alone ----
def _depth(syn, planes, cam_x, rows, cols, K):
    """the depth map of the fronto-parallel planes for a camera at (cam_x, 0, 0) looking along z"""
    ys, xs = np.mgrid[0:rows, 0:cols].astype(np.float64)
    xn, yn = (xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1]
    Z = np.full((rows, cols), np.inf)
    for p in planes:
        X, Y = cam_x + p.z * xn, p.z * yn
        hit = (p.z < Z) & (X >= p.x0) & (X <= p.x1) & (Y >= p.y0) & (Y <= p.y1)
        Z[hit] = p.z
    return Z


QUALITY = {}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_quality_on_rendered_planes(syn, seed):
    """synthetic's planes scenes at calib(0.25), 94 x 310, D = 32, the defaults: of the pixels visible in both views
    at least 0.95 reliable, of those at least 0.98 within 1 px of f b / Z."""
    scale, rows, cols, D = 0.25, 94, 310, 32
    P0, P1 = syn.calib(scale)
    K = P0[:, :3]
    f, B = K[0, 0], syn.baseline_m()
    planes = syn.random_scene(seed, rows, cols, f=f, px_per_cell=16.0 * scale)
    rng = np.random.default_rng(seed ^ 0xABCDEF)
    left = syn._to_u8(syn._render(planes, np.eye(3), np.zeros(3), rows, cols, K), rng, 2.0)
    right = syn._to_u8(syn._render(planes, np.eye(3), np.array([B, 0.0, 0.0]), rows, cols, K), rng, 2.0)
    Zl, Zr = _depth(syn, planes, 0.0, rows, cols, K), _depth(syn, planes, B, rows, cols, K)
    truth = f * B / Zl
    xr = np.arange(cols)[None, :] - truth
    xi = np.clip(np.rint(xr).astype(int), 0, cols - 1)
    both = (xr >= 0) & (xr <= cols - 1) & (np.take_along_axis(Zr, xi, 1) == Zl)
    disp = R.disparity(left, right, 0, D)["disp"]
    reliable = both & ~np.isnan(disp)
    frac_reliable = reliable.sum() / both.sum()
    frac_good = (np.abs(disp[reliable] - truth[reliable]) <= 1.0).sum() / reliable.sum()
    QUALITY[seed] = (frac_reliable, frac_good)
    print(f"seed {seed}: visible in both {both.mean():.3f}, reliable {frac_reliable:.4f}, within 1 px {frac_good:.4f}")
    assert frac_reliable >= 0.95
    assert frac_good >= 0.98


def test_sanitizer_run_of_the_whole_table(tmp_path):
    """tests/sgm_ref/sgm_ref_main.c: the same C under -fsanitize=address,undefined, as a stand-alone program, over
    every row of the table; what it prints equals the library's results."""
    R.build("asan")
    for i, c in enumerate(TABLE):
        f = tmp_path / (c["name"] + ".bin")
        left, right = R.pair(c["kind"], c["rows"], c["cols"], c["dmin"], c["D"])
        R.write_problem(f, left, right, c["dmin"], c["D"], c["P1"], c["P2"], c["U"])
        out = subprocess.run([str(R.MAIN), str(f)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.split("\n")[:-1] == R.main_lines(R.result(i)), c["name"]
