"""GPU: the corner detector through libvo.so (vo_detect_corners, vo_detect_corners_batch, vo_fetch_corner_metric;
k_corner_metric, k_corner_count, k_corner_emit, k_corner_rank) against the CPU build of the same
include/vo_spec.h functions (tests/corner_ref, which test_corner.py holds to a float64 restatement and whose
census it asserts): locations, metrics, counts and the metric plane are equal by bytes for the whole table.
Contexts are the smallest the table needs (40 x 56, 37 x 53 and 64 x 64 images, max_keypoints 512 and 16)."""
import ctypes as C

import numpy as np
import pytest

import corner_ref as R

pytestmark = pytest.mark.gpu

TABLE = R.table()


@pytest.fixture(scope="module")
def ctxs(vo):
    c = {(size, k): vo.Context(*R.SIZES[size], 2, sift=vo.default_sift_params(k)) for size in R.SIZES for k in (R.MAX_KEYPOINTS, 16)}
    yield c
    for x in c.values():
        x.close()


def _params(vo, p):
    return vo.default_corner_params(method=p["method"], filter_size=p["f"], min_quality=p["min_quality"], strongest=p["strongest"],
                                    roi=p["roi"])


def _same(got, exp):
    loc, met = got
    assert exp["status"] == R.OK
    assert loc.dtype == np.float32 and met.dtype == np.float32 and loc.shape == (exp["count"], 2) and met.shape == (exp["count"],)
    assert met.tobytes() == exp["metric"].tobytes()
    assert loc.tobytes() == exp["loc"].tobytes(), np.abs(loc - exp["loc"]).max()


def _detect(vo, ctx, img, p, exp):
    """One call held to the reference record: results by bytes, or the overflow with the true count."""
    if exp["status"] == R.OK:
        _same(ctx.detect_corners(img, _params(vo, p)), exp)
    else:
        with pytest.raises(vo.VOError) as e:
            ctx.detect_corners(img, _params(vo, p))
        assert e.value.code == vo.VO_ERR_CAPACITY and e.value.count == exp["count"]


@pytest.mark.parametrize("row", range(len(TABLE)), ids=[t["name"] for t in TABLE])
def test_table_equals_the_reference_by_bytes(vo, ctxs, row):
    t, exp = TABLE[row], R.results()[row]
    p = t["params"]
    ctx = ctxs[(t["image"][0], p["max_keypoints"])]
    _detect(vo, ctx, R.image(t["image"]), p, exp)
    plane = ctx.fetch_corner_metric(0)
    assert plane.tobytes() == exp["plane"].tobytes(), np.abs(plane - exp["plane"]).max()


def test_default_params_are_the_librarys(vo):
    p = vo.CornerParams()
    vo.load_library().vo_default_corner_params(p)
    d = vo.default_corner_params()
    assert (p.method, p.filter_size, p.min_quality, p.strongest, tuple(p.roi)) == \
           (d.method, d.filter_size, d.min_quality, d.strongest, tuple(d.roi)) == (0, 5, np.float32(0.01), 0, (0, 0, 0, 0))


LATTICE = (83, 200)


@pytest.mark.parametrize("f", [3, 5, 15])
def test_lattice_on_every_residue_of_the_tile(vo, f):
    """Corners on every residue of the kernel's 64 x 16 tile, in an image of 4 x 6 tiles whose last tiles are cut:
    a wrong halo or seam moves a metric and with it a corner."""
    img = R.lattice(*LATTICE)
    exp = R.detect(img, f=f, min_quality=0.0)
    pr, pc = np.rint(exp["loc"][:, 1] - 1).astype(int), np.rint(exp["loc"][:, 0] - 1).astype(int)
    assert set(pc % 64) == set(range(64)) and set(pr % 16) == set(range(16)), (sorted(set(pc % 64)), sorted(set(pr % 16)))
    ctx = vo.Context(*LATTICE, 1, sift=vo.default_sift_params(R.MAX_KEYPOINTS))
    try:
        _same(ctx.detect_corners(img, vo.default_corner_params(filter_size=f, min_quality=0.0)), exp)
        assert ctx.fetch_corner_metric(0).tobytes() == exp["plane"].tobytes()
        roi = (60, 13, 75, 40)                                    # a ROI that starts and ends inside tiles
        _same(ctx.detect_corners(img, vo.default_corner_params(filter_size=f, min_quality=0.0, roi=roi)),
              R.detect(img, f=f, min_quality=0.0, roi=roi))
    finally:
        ctx.close()


def test_col_major_and_padded_inputs(vo, ctxs):
    ctx = ctxs[("b", R.MAX_KEYPOINTS)]
    img = R.image("b:noise")
    rows, cols = img.shape                                        # 37 x 53
    exp = R.detect(img)
    _same(ctx.detect_corners(np.asfortranarray(img)), exp)
    wide = np.full((rows, cols + 13), 255, np.uint8)
    wide[:, :cols] = img
    tall = np.full((rows + 5, cols), 255, np.uint8, order="F")
    tall[:rows] = img
    _same(ctx.detect_corners(wide[:, :cols]), exp)                # row-major, ld > cols
    _same(ctx.detect_corners(tall[:rows]), exp)                   # column-major, ld > rows


def test_ragged_batch_equals_the_single_calls(vo, ctxs):
    """Many, one and no corners in one launch; image i is the single call, by bytes; rows beyond a count are untouched."""
    ctx = ctxs[("a", R.MAX_KEYPOINTS)]
    rows, cols = R.SIZES["a"]
    one = np.full((rows, cols), 30, np.uint8)
    one[17, 23] = 220
    imgs = np.stack([R.image("a:noise"), one, R.image("a:flat"), R.image("a:squares")])
    for p in (vo.default_corner_params(), vo.default_corner_params(method=vo.VO_CORNER_HARRIS, filter_size=7, strongest=6)):
        batch = ctx.detect_corners_batch(imgs, p)
        counts = []
        for i, (loc, met, st, n) in enumerate(batch):
            exp = R.detect(imgs[i], method=p.method, f=p.filter_size, strongest=p.strongest)
            single = ctx.detect_corners(imgs[i], p)
            assert st == vo.VO_OK and n == exp["count"]
            _same((loc, met), exp)
            _same(single, exp)
            counts.append(n)
        assert counts[1] == 1 and counts[2] == 0 and counts[0] > 5
    # the raw entry: a stride below the first image's count -> its status alone is VO_ERR_CAPACITY; untouched rows
    stride = 20
    loc = np.full((4, stride, 2), -7.0, np.float32)
    met = np.full((4, stride), -7.0, np.float32)
    n, st = np.zeros(4, np.int32), np.zeros(4, np.int32)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = ctx.lib.vo_detect_corners_batch(ctx.h, P(imgs, C.c_uint8), cols, 0, 4, None, P(loc, C.c_float), P(met, C.c_float), stride,
                                         P(n, C.c_int32), P(st, C.c_int32))
    assert rc == vo.VO_OK
    exp = [R.detect(im) for im in imgs]
    assert list(n) == [e["count"] for e in exp] and list(st) == [vo.VO_ERR_CAPACITY, vo.VO_OK, vo.VO_OK, vo.VO_OK]
    assert (loc[0] == -7.0).all() and (met[0] == -7.0).all()
    for i in (1, 2, 3):
        assert loc[i, :n[i]].tobytes() == exp[i]["loc"].tobytes() and (loc[i, n[i]:] == -7.0).all() and (met[i, n[i]:] == -7.0).all()


def test_full_size_image_at_the_defaults(vo):
    """375 x 1242, the defaults, through the module function: the one full-size case."""
    rng = np.random.default_rng(7)
    img = np.clip(np.rint(128.0 + 40.0 * R._blur(rng.standard_normal((375, 1242)), 1.5) / 0.19), 0, 255).astype(np.uint8)
    exp = R.detect(img, max_keypoints=16384)
    assert exp["count"] > 1000
    _same(vo.detectMinEigenFeatures(img), exp)
    assert vo._default_ctx(375, 1242).fetch_corner_metric(0).tobytes() == exp["plane"].tobytes()
    loc, met = vo.detectHarrisFeatures(img, MinQuality=0.05, FilterSize=7, ROI=(100, 50, 600, 200))
    _same((loc, met), R.detect(img, method=R.HARRIS, f=7, min_quality=0.05, roi=(100, 50, 600, 200), max_keypoints=16384))


def test_strongest_on_a_row_with_ties(vo, ctxs):
    ctx = ctxs[("a", R.MAX_KEYPOINTS)]
    img = R.image("a:quad")
    full = R.detect(img)
    assert len(set(np.sort(full["metric"])[1:].tolist())) == 1 and full["count"] == 5  # four equal corners and a weaker one
    for n in (1, 2, 3, 4, 5, 6, 512):
        _same(ctx.detect_corners(img, vo.default_corner_params(strongest=n)), R.detect(img, strongest=n))
    img = R.image("a:noise")
    for n in (1, 7, 78, 79, 80):                                                   # 79 corners
        _same(ctx.detect_corners(img, vo.default_corner_params(strongest=n)), R.detect(img, strongest=n))
    # more corners than one rank tile holds (256)
    c = ctxs[("c", R.MAX_KEYPOINTS)]
    img = R.image("c:white")
    assert R.detect(img, f=3, min_quality=0.0)["count"] > 256
    exp = R.detect(img, f=3, min_quality=0.0, strongest=200)
    assert exp["count"] == 200
    _same(c.detect_corners(img, vo.default_corner_params(filter_size=3, min_quality=0.0, strongest=200)), exp)


def test_overflow_returns_the_true_count(vo, ctxs):
    ctx = ctxs[("c", 16)]
    img = R.image("c:white")
    exp = R.detect(img, f=3, min_quality=0.0, max_keypoints=16)
    assert exp["status"] == R.ERR_CAPACITY and exp["count"] > 64
    for strongest in (0, 5):
        with pytest.raises(vo.VOError) as e:
            ctx.detect_corners(img, vo.default_corner_params(filter_size=3, min_quality=0.0, strongest=strongest))
        assert e.value.code == vo.VO_ERR_CAPACITY and e.value.count == exp["count"]
    # the caller's capacity: one short, then exact
    big = ctxs[("c", R.MAX_KEYPOINTS)]
    p = vo.default_corner_params(filter_size=3, min_quality=0.0)
    with pytest.raises(vo.VOError) as e:
        big.detect_corners(img, p, capacity=exp["count"] - 1)
    assert e.value.code == vo.VO_ERR_CAPACITY and e.value.count == exp["count"]
    _same(big.detect_corners(img, p, capacity=exp["count"]), R.detect(img, f=3, min_quality=0.0))


def test_refusals(vo, ctxs):
    ctx = ctxs[("a", R.MAX_KEYPOINTS)]
    img = np.ascontiguousarray(R.image("a:noise"))
    rows, cols = img.shape
    lib, h = ctx.lib, ctx.h
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    loc, met, n = np.zeros((2048, 2), np.float32), np.zeros(2048, np.float32), C.c_int(0)

    def call(params=None, r=rows, q=cols, ld=cols, cm=0, cap=2048):
        return lib.vo_detect_corners(h, P(img, C.c_uint8), r, q, ld, cm, C.byref(params) if params is not None else None,
                                     P(loc, C.c_float), P(met, C.c_float), cap, C.byref(n))

    assert call() == vo.VO_OK and n.value == R.detect(img)["count"]
    assert call(r=rows + 1) == vo.VO_ERR_ARG and call(q=cols - 1) == vo.VO_ERR_ARG and call(ld=cols - 1) == vo.VO_ERR_ARG
    assert call(cm=2) == vo.VO_ERR_ARG and call(cap=-1) == vo.VO_ERR_ARG
    for kw, word in ((dict(method=2), "method"), (dict(filter_size=4), "filter_size"), (dict(filter_size=17), "filter_size"),
                     (dict(filter_size=1), "filter_size"), (dict(min_quality=-0.5), "min_quality"), (dict(min_quality=1.25), "min_quality"),
                     (dict(min_quality=float("nan")), "min_quality"), (dict(strongest=-1), "strongest"), (dict(strongest=513), "strongest"),
                     (dict(roi=(1, 1, -2, 5)), "roi (w, h"), (dict(roi=(1, 1, 5, 0)), "roi (w, h"), (dict(roi=(0, 1, 5, 5)), "inside"),
                     (dict(roi=(53, 1, 5, 5)), "inside"), (dict(roi=(1, 37, 5, 5)), "inside"), (dict(roi=(57, 1, 1, 1)), "inside")):
        assert call(params=vo.default_corner_params(**kw)) == vo.VO_ERR_ARG, kw
        assert word in lib.vo_last_error(h).decode(), kw
    assert call(params=vo.default_corner_params(roi=(56, 40, 1, 1))) == vo.VO_OK
    st, cnt = np.zeros(8, np.int32), np.zeros(8, np.int32)
    for n_img in (0, 5):                                                           # 1 .. 2 x max_batch = 4
        assert lib.vo_detect_corners_batch(h, P(img, C.c_uint8), cols, 0, n_img, None, P(loc, C.c_float), P(met, C.c_float), 16,
                                           P(cnt, C.c_int32), P(st, C.c_int32)) == vo.VO_ERR_ARG
    with pytest.raises(vo.VOError):
        ctx.detect_corners(img[:-1])
    with pytest.raises(vo.VOError) as e:
        ctx.fetch_corner_metric(1)                                                 # the last call had one image
    assert e.value.code == vo.VO_ERR_ARG


def test_quiet_context_and_untouched_loop(vo, syn):
    """Two vo_step calls with a vo_detect_corners between them give the outputs of two without it (and the same
    landmarks); a context that never detects corners launches none of the kernels and has no plane to fetch."""
    rows, cols, scale = 150, 497, 0.4
    L, Rt, _ = syn.sequence(2, rows=rows, cols=cols, scale=scale)
    cal = vo.calib_from(*syn.calib(scale))
    outs = []
    kernels = {"k_corner_metric", "k_corner_count", "k_corner_emit", "k_corner_rank"}
    for between in (False, True):
        ctx = vo.Context(rows, cols, 1, calib=cal)
        try:
            ctx.set_profiling(True)
            rec = [ctx.step(L[0], Rt[0])]
            if between:
                loc, met = ctx.detect_corners(L[0], vo.default_corner_params(strongest=200))
                exp = R.detect(L[0], strongest=200, max_keypoints=16384)
                assert len(loc) == 200 and loc.tobytes() == exp["loc"].tobytes() and met.tobytes() == exp["metric"].tobytes()
            else:
                with pytest.raises(vo.VOError) as e:
                    ctx.fetch_corner_metric(0)
                assert e.value.code == vo.VO_ERR_STATE
            rec.append(ctx.step(L[1], Rt[1]))
            names = set(ctx.kernel_times())
            assert (kernels <= names) if between else not (kernels & names), names
            outs.append((np.array(rec).tobytes(), ctx.get_landmarks().tobytes()))
        finally:
            ctx.close()
    assert outs[0] == outs[1]


def test_refused_while_step_batches_are_pending(vo, syn):
    """VO_ERR_STATE while a submitted step batch has not been collected; the same call runs afterwards."""
    import torch
    rows, cols, scale = 150, 497, 0.4
    L, Rt, _ = syn.sequence(2, rows=rows, cols=cols, scale=scale)
    L, Rt = np.ascontiguousarray(L), np.ascontiguousarray(Rt)
    ctx = vo.Context(rows, cols, 1, calib=vo.calib_from(*syn.calib(scale)))
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(Rt).cuda()
    torch.cuda.synchronize()
    try:
        ctx.step_submit_dev(dl.data_ptr(), dr.data_ptr(), 1)
        with pytest.raises(vo.VOError) as e:
            ctx.detect_corners(L[0])
        assert e.value.code == vo.VO_ERR_STATE
        ctx.step_collect()
        assert len(ctx.detect_corners(L[0])[0]) > 10
    finally:
        ctx.close()
