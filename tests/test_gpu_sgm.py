"""GPU: disparitySGM through libvo.so (vo_disparity_sgm, vo_disparity_sgm_batch, vo_disparity_sgm_batch_dev,
vo_fetch_sgm_cost; k_sgm_census, k_sgm_paths, k_sgm_select) against the CPU build of the same include/vo_spec.h
functions (tests/sgm_ref, which test_sgm.py holds to a NumPy restatement and whose census it asserts): the
disparity map and the summed path costs S are equal by bytes for the whole table.

The shapes are the smallest at which each mechanism can go wrong:
  16 x 16,  D 8        the smallest context; D far below a wave; every census tile clipped
  16 x 20,  D 64       D > cols: most reads clamped, most pixels invalid
  37 x 53,  D 16, -4   odd sizes; negative disparities; the clamp at the right edge; diagonals cut by the bottom
  53 x 37,  D 32       rows > cols: diagonals cut by the sides
  24 x 150, D 64       one lane per disparity; census tiles across three columns of tiles
  20 x 200, D 128, 3   two disparities per lane: the k +- 1 exchange across lanes
  17 x 65,  D 24       D not a power of two: idle-lane masks
each on a shifted texture, a flat image (everything ties), stripes of period 8 (ambiguous) and a two-plane step
with its occlusion; one shape also at P1 = P2 = 0, P1 = P2 = 255, U = 0 and U = 100."""
import ctypes as C

import numpy as np
import pytest

import sgm_ref as R

pytestmark = pytest.mark.gpu

TABLE = R.TABLE


@pytest.fixture(scope="module")
def ctxs(vo):
    c = {(rows, cols): vo.Context(rows, cols, 2, sift=vo.default_sift_params(64)) for rows, cols, _, _ in R.SHAPES}
    c[(16, 24)] = vo.Context(16, 24, 2, sift=vo.default_sift_params(64))
    yield c
    for x in c.values():
        x.close()


def _params(vo, c):
    return vo.default_sgm_params(disparity_range=(c["dmin"], c["dmin"] + c["D"]), uniqueness_threshold=c["U"], p1=c["P1"], p2=c["P2"])


@pytest.mark.parametrize("i", range(len(TABLE)), ids=[c["name"] for c in TABLE])
def test_table_equals_the_reference_by_bytes(vo, ctxs, i):
    c, exp = TABLE[i], R.result(i)
    ctx = ctxs[(c["rows"], c["cols"])]
    left, right = R.pair(c["kind"], c["rows"], c["cols"], c["dmin"], c["D"])
    disp = ctx.disparity_sgm(left, right, _params(vo, c))
    S = ctx.fetch_sgm_cost(0, c["D"])
    assert S.tobytes() == exp["S"].tobytes(), int(np.abs(S.astype(int) - exp["S"].astype(int)).max())
    assert disp.dtype == np.float32 and disp.shape == (c["rows"], c["cols"])
    assert disp.tobytes() == exp["disp"].tobytes()


def test_default_params_are_the_librarys(vo):
    p = vo.SgmParams()
    vo.load_library().vo_default_sgm_params(C.byref(p))
    q = vo.default_sgm_params()
    assert bytes(p) == bytes(q) and tuple(p.disparity_range) == (0, 128) and (p.uniqueness_threshold, p.p1, p.p2) == (15, 10, 120)


def test_col_major_and_padded_inputs(vo, ctxs):
    """MATLAB's storage, padded leading dimensions either way, and an ld_out whose padding is left untouched."""
    rows, cols, D, dmin = 37, 53, 16, -4
    ctx = ctxs[(rows, cols)]
    i = next(k for k, c in enumerate(TABLE) if c["name"] == "37x53_D16_-4_step")
    exp = R.result(i)["disp"]
    left, right = R.pair("step", rows, cols, dmin, D)
    p = vo.default_sgm_params(disparity_range=(dmin, dmin + D))
    F = ctx.disparity_sgm(np.asfortranarray(left), np.asfortranarray(right), p)
    assert F.flags.f_contiguous and np.asarray(F).tobytes(order="C") == exp.tobytes()
    P8, PF = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    for cm in (0, 1):
        major, minor = (rows, cols) if cm else (cols, rows)               # contiguous extent, strided extent
        ld, ld_out = major + 5, major + 3
        bufs = []
        for img in (left, right):
            b = np.full((minor, ld), 0xEE, np.uint8)
            b[:, :major] = img.T if cm else img
            bufs.append(b)
        out = np.full((minor, ld_out), -7.0, np.float32)
        rc = ctx.lib.vo_disparity_sgm(ctx.h, bufs[0].ctypes.data_as(P8), bufs[1].ctypes.data_as(P8), rows, cols, ld, cm, C.byref(p),
                                      out.ctypes.data_as(PF), ld_out)
        assert rc == vo.VO_OK
        assert (out[:, major:] == -7.0).all()
        got = out[:, :major].T if cm else out[:, :major]
        assert np.ascontiguousarray(got).tobytes() == exp.tobytes(), cm


def test_batch_of_nine_crosses_the_group_and_equals_the_single_calls(vo, ctxs):
    """9 pairs of different content at 16 x 24: a full group of 8 and a group of one; pair f is the single call, by
    bytes, through the host batch and the device batch; the sums kept are the last group's."""
    import torch
    rows, cols, D = 16, 24, 16
    ctx = ctxs[(rows, cols)]
    kinds = ["texture", "flat", "stripes", "step", "texture", "step", "stripes", "texture", "step"]
    pairs = [R.pair(k, rows, cols, 0, D, seed=f) for f, k in enumerate(kinds)]
    L, Rt = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    p = vo.default_sgm_params(disparity_range=(0, D))
    single = [ctx.disparity_sgm(L[f], Rt[f], p) for f in range(9)]
    for f in range(9):
        assert single[f].tobytes() == R.disparity(L[f], Rt[f], 0, D)["disp"].tobytes(), f
    got = ctx.disparity_sgm_batch(L, Rt, p)
    assert got.shape == (9, rows, cols)
    for f in range(9):
        assert got[f].tobytes() == single[f].tobytes(), f
    assert ctx.fetch_sgm_cost(8, D).tobytes() == R.disparity(L[8], Rt[8], 0, D)["S"].tobytes()
    with pytest.raises(vo.VOError) as e:
        ctx.fetch_sgm_cost(7, D)                                           # an earlier group's: gone
    assert e.value.code == vo.VO_ERR_ARG
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(Rt).cuda()
    dd = torch.full((9, rows, cols), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.disparity_sgm_batch_dev(dl.data_ptr(), dr.data_ptr(), 9, dd.data_ptr(), p)
    torch.cuda.synchronize()
    dev = dd.cpu().numpy()
    for f in range(9):
        assert dev[f].tobytes() == single[f].tobytes(), f
    # column-major batches, as vo_track_points_batch takes its images
    Lf, Rf = (np.ascontiguousarray(a.transpose(0, 2, 1)) for a in (L[:3], Rt[:3]))
    out = np.zeros((3, cols, rows), np.float32)
    P8 = C.POINTER(C.c_uint8)
    assert ctx.lib.vo_disparity_sgm_batch(ctx.h, Lf.ctypes.data_as(P8), Rf.ctypes.data_as(P8), rows, 1, 3, C.byref(p),
                                          out.ctypes.data_as(C.POINTER(C.c_float))) == vo.VO_OK
    for f in range(3):
        assert np.ascontiguousarray(out[f].T).tobytes() == single[f].tobytes(), f


def test_refusals(vo, ctxs):
    rows, cols = 37, 53
    ctx = ctxs[(rows, cols)]
    left, right = (np.ascontiguousarray(a) for a in R.pair("texture", rows, cols, -4, 16))
    lib, h = ctx.lib, ctx.h
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    out = np.zeros((rows, cols), np.float32)

    def call(params=None, r=rows, q=cols, ld=cols, cm=0, ld_out=cols, l=left, o=out):
        return lib.vo_disparity_sgm(h, P(l, C.c_uint8) if l is not None else None, P(right, C.c_uint8), r, q, ld, cm,
                                    C.byref(params) if params is not None else None, P(o, C.c_float) if o is not None else None, ld_out)

    ok = vo.default_sgm_params(disparity_range=(-4, 12))
    assert call(ok) == vo.VO_OK and out.tobytes() == R.disparity(left, right, -4, 16)["disp"].tobytes()
    assert call(None) == vo.VO_OK and out.tobytes() == R.disparity(left, right, 0, 128)["disp"].tobytes()     # NULL: the defaults
    assert call(ok, r=rows + 1) == vo.VO_ERR_ARG and call(ok, q=cols - 1) == vo.VO_ERR_ARG and call(ok, ld=cols - 1) == vo.VO_ERR_ARG
    assert call(ok, cm=2) == vo.VO_ERR_ARG and call(ok, ld_out=cols - 1) == vo.VO_ERR_ARG and call(ok, cm=1, ld=rows - 1) == vo.VO_ERR_ARG
    assert call(ok, l=None) == vo.VO_ERR_ARG and call(ok, o=None) == vo.VO_ERR_ARG
    for kw, word in ((dict(disparity_range=(0, 12)), "disparity_range (max - min"), (dict(disparity_range=(0, 136)), "disparity_range (max - min"),
                     (dict(disparity_range=(8, 8)), "disparity_range (-1024"), (dict(disparity_range=(16, 8)), "disparity_range (-1024"),
                     (dict(disparity_range=(-1032, -1024)), "disparity_range (-1024"), (dict(disparity_range=(1016, 1032)), "disparity_range (-1024"),
                     (dict(uniqueness_threshold=-1), "uniqueness_threshold"), (dict(uniqueness_threshold=101), "uniqueness_threshold"),
                     (dict(p1=-1), "p1"), (dict(p1=256, p2=256), "p1"), (dict(p1=11, p2=10), "p2"), (dict(p2=256), "p2")):
        bad = vo.default_sgm_params(**kw)
        assert call(bad) == vo.VO_ERR_ARG, kw
        assert word in lib.vo_last_error(h).decode(), kw
        with pytest.raises(vo.VOError) as e:
            vo.check_sgm_params(bad)
        assert word in str(e.value), kw
    assert call(vo.default_sgm_params(disparity_range=(-1024, -1016))) == vo.VO_OK
    assert call(vo.default_sgm_params(disparity_range=(896, 1024), p1=0, p2=0, uniqueness_threshold=100)) == vo.VO_OK
    for n_pairs in (0, -1):
        assert lib.vo_disparity_sgm_batch(h, P(left, C.c_uint8), P(right, C.c_uint8), cols, 0, n_pairs, None, P(out, C.c_float)) == vo.VO_ERR_ARG
        assert lib.vo_disparity_sgm_batch_dev(h, C.c_void_p(8), C.c_void_p(8), n_pairs, None, C.c_void_p(8)) == vo.VO_ERR_ARG
    assert lib.vo_disparity_sgm_batch_dev(h, None, C.c_void_p(8), 1, None, C.c_void_p(8)) == vo.VO_ERR_ARG
    with pytest.raises(vo.VOError):
        ctx.disparity_sgm(left[:-1], right[:-1])
    with pytest.raises(vo.VOError) as e:
        ctx.fetch_sgm_cost(1, 128)                                                 # the last call had one pair
    assert e.value.code == vo.VO_ERR_ARG
    small = np.zeros(8, np.uint16)
    assert lib.vo_fetch_sgm_cost(h, 0, P(small, C.c_uint16), 8) == vo.VO_ERR_CAPACITY


def test_quiet_context_and_untouched_loop(vo, syn):
    """Two vo_step calls with a vo_disparity_sgm between them give the outputs of two without it (and the same
    landmarks); a context that never calls launches none of the kernels and has no sums to fetch."""
    rows, cols, scale = 150, 497, 0.4
    L, Rt, _ = syn.sequence(2, rows=rows, cols=cols, scale=scale)
    cal = vo.calib_from(*syn.calib(scale))
    outs = []
    kernels = {"k_sgm_census", "k_sgm_paths_rows", "k_sgm_paths_cols", "k_sgm_paths_diag", "k_sgm_paths_anti", "k_sgm_select"}
    for between in (False, True):
        ctx = vo.Context(rows, cols, 1, calib=cal)
        try:
            ctx.set_profiling(True)
            rec = [ctx.step(L[0], Rt[0])]
            if between:
                d = ctx.disparity_sgm(L[0], Rt[0], vo.default_sgm_params(disparity_range=(0, 48)))
                assert d.tobytes() == R.disparity(L[0], Rt[0], 0, 48)["disp"].tobytes()
            else:
                with pytest.raises(vo.VOError) as e:
                    ctx.fetch_sgm_cost(0, 48)
                assert e.value.code == vo.VO_ERR_STATE
            rec.append(ctx.step(L[1], Rt[1]))
            names = set(ctx.kernel_times())
            assert (kernels <= names) if between else not (kernels & names), names
            outs.append((np.array(rec).tobytes(), ctx.get_landmarks().tobytes()))
        finally:
            ctx.close()
    assert outs[0] == outs[1]


def test_refused_while_step_batches_are_pending(vo, syn):
    """VO_ERR_STATE while a submitted step batch has not been collected; the same calls run afterwards."""
    import torch
    rows, cols, scale = 150, 497, 0.4
    L, Rt, _ = syn.sequence(2, rows=rows, cols=cols, scale=scale)
    L, Rt = np.ascontiguousarray(L), np.ascontiguousarray(Rt)
    ctx = vo.Context(rows, cols, 1, calib=vo.calib_from(*syn.calib(scale)))
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(Rt).cuda()
    dd = torch.zeros((1, rows, cols), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = vo.default_sgm_params(disparity_range=(0, 8))
    try:
        ctx.step_submit_dev(dl.data_ptr(), dr.data_ptr(), 1)
        for f in (lambda: ctx.disparity_sgm(L[0], Rt[0], p), lambda: ctx.disparity_sgm_batch(L[:1], Rt[:1], p),
                  lambda: ctx.disparity_sgm_batch_dev(dl.data_ptr(), dr.data_ptr(), 1, dd.data_ptr(), p),
                  lambda: ctx.reconstruct_scene(np.zeros((rows, cols), np.float32), np.eye(4))):
            with pytest.raises(vo.VOError) as e:
                f()
            assert e.value.code == vo.VO_ERR_STATE
        ctx.step_collect()
        assert np.isfinite(ctx.disparity_sgm(L[0], Rt[0], p)).any()
    finally:
        ctx.close()
