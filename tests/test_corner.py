"""CPU: the corner detector's reference (tests/corner_ref, the CPU build of include/vo_spec.h's vo_corner_*
functions, which the GPU suite compares the kernels with by bytes) against corner_f64_ref.py, an independent
float64 restatement of DESIGN.md 3.5.4, on rendered corners at known places, and the census that shows the
shared table reaches every branch of the spec.  The host refusals of the Python layer and the sanitizer run of
the same C (a stand-alone program, host code only) are here too.  Each test prints its figures before it asserts."""
import subprocess

import numpy as np
import pytest

import corner_f64_ref as F
import corner_ref as R
import klt_ref as K

TABLE = R.table()
NAMES = [t["name"] for t in TABLE]

# The rows held to the float64 restatement: generated textures without exact ties (the engineered images of the
# census tie by construction and are not strict peaks).
F64_ROWS = ["squares_a", "checker_a", "blobs_a", "noise_a", "squares_b", "checker_b", "blobs_b", "noise_b", "squares_c", "checker_c",
            "blobs_c", "noise_c", "squares_a_harris", "checker_b_harris_f3", "noise_c_f3", "checker_c_f9", "noise_b_f9",
            "squares_c_f15", "noise_a_f15", "blobs_c_harris_f15", "noise_a_q0", "noise_b_q50", "noise_a_roi_boundary",
            "noise_a_roi_excl", "squares_c_roi_harris"]
# A float64 corner is compared when it clears the threshold and beats each of its neighbours by this fraction of its
# own metric (a strict peak); a reference corner must be a float64 corner when every comparison is loosened by the
# same fraction.  The reference's plane differs from the float64 one by the 12-bit weights (each within 2^-13 of
# its true value) and the final f32 rounding: at the fixture corners by 1e-5 .. 1.1e-3 of the metric (printed
# below), most at FilterSize 15, whose tail weights are the smallest.  Were 2e-3 too small for a row, its two sets
# would differ and the test would fail; the rows are those whose reference corners stay within the 10 % the
# comparison may drop (noise at FilterSize 15 on the 64 x 64 image has peaks too flat for that and is left to
# the GPU suite's byte comparison).
MARGIN = 2e-3
# largest |position difference| measured over F64_ROWS: 3.04e-2 px (noise_a_f15: the flattest peaks; at most 9.9e-4
# px at FilterSize <= 5); the gate is 4 x that, the margin klt_ref uses
MEASURED_DEV = 3.04e-2
GATE = 4.0 * MEASURED_DEV


def _pixels(rec):
    return np.rint(rec["loc"][:, 1] - 1).astype(int), np.rint(rec["loc"][:, 0] - 1).astype(int)


def test_weight_tables():
    for f, q in R.WEIGHTS.items():
        assert R.weights(f) == q, f
        assert sum(q) == 4096 and len(q) == f and min(q) > 0 and q == q[::-1]


def test_names_are_unique_and_every_row_ran():
    assert len(set(NAMES)) == len(NAMES) and set(F64_ROWS) <= set(NAMES)
    for t, r in zip(TABLE, R.results()):
        assert r["status"] in (R.OK, R.ERR_CAPACITY) and r["plane"].shape == R.SIZES[t["image"][0]]


def test_reference_equals_the_float64_restatement():
    worst_dev, worst_rel, compared = 0.0, 0.0, 0
    for name in F64_ROWS:
        t, r = TABLE[NAMES.index(name)], R.results()[NAMES.index(name)]
        p = t["params"]
        assert r["status"] == R.OK and p["strongest"] == 0 and r["count"] > 0
        m = F.metric_plane(R.image(t["image"]), p["method"], p["f"])
        strict = F.corner_mask(m, p["min_quality"], p["roi"], MARGIN)
        loose = F.corner_mask(m, p["min_quality"], p["roi"], -MARGIN)
        pr, pc = _pixels(r)
        ref = np.zeros(m.shape, bool)
        ref[pr, pc] = True
        assert ref.sum() == r["count"]
        rel = float((np.abs(r["plane"] - m)[ref] / m[ref]).max())
        dropped = int((ref & ~strict).sum())
        L = F.locations(m, strict)
        dev = max([max(abs(L[(a, b)][0] - x), abs(L[(a, b)][1] - y)) for (x, y), a, b in zip(r["loc"], pr, pc) if (a, b) in L] or [0.0])
        print(f"{name:26s} corners {r['count']:4d} compared {int(strict.sum()):4d} dropped {dropped:2d} plane rel {rel:.2e} "
              f"position {dev:.2e} px")
        # the two sets are equal on the strict corners: every strict float64 corner is a reference corner, and
        # every reference corner is a float64 corner at least loosely
        assert not (strict & ~ref).any() and not (ref & ~loose).any(), name
        assert dropped <= 0.1 * r["count"], (name, dropped, r["count"])
        assert dev <= GATE, (name, dev)
        worst_dev, worst_rel, compared = max(worst_dev, dev), max(worst_rel, rel), compared + int(strict.sum())
    print(f"largest position deviation {worst_dev:.3e} px (gate {GATE:.3e}), largest plane deviation {worst_rel:.2e}, {compared} corners")
    assert worst_dev <= GATE and compared > 900


def test_known_l_and_x_corners_are_found():
    """Every rendered corner has a detection within FilterSize / 2 = 2.5 px (the response window that sees it), its
    own; the largest distances are printed for DESIGN.md 3.5.4 (L-corners: the peak of either response lies inside
    the corner, about 1.4 - 2 px along its diagonal)."""
    worst = {}
    for size, (rows, cols) in R.SIZES.items():
        for method in (R.MINEIG, R.HARRIS):
            for kind, truth, q in (("L", np.concatenate([R.corners_of(s) for s in R.SQUARES[size]]), 0.01),
                                   ("X", R.x_corners(rows, cols), 0.3)):
                rec = R.detect(R.image(f"{size}:{'squares' if kind == 'L' else 'checker'}"), method=method, min_quality=q)
                d = np.sqrt(((truth[:, None] - rec["loc"][None].astype(np.float64)) ** 2).sum(2))
                near = d.argmin(1)
                assert len(set(near.tolist())) == len(truth) and d.min(1).max() <= 2.5, (size, method, kind, d.min(1))
                worst[(kind, method)] = max(worst.get((kind, method), 0.0), float(d.min(1).max()))
    print({f"{k} {'Harris' if m else 'MinEig'}": round(v, 3) for (k, m), v in worst.items()})
    assert worst[("X", R.MINEIG)] < 0.1           # an X-corner is symmetric: no bias to speak of


def _census():
    c = dict(eq_row=0, eq_col=0, eq_diag=0, half_plus=0, half_minus=0, den_zero=0, top=0, bottom=0, left=0, right=0, image_corner=0,
             flat=0, harris_nonpositive=0, q0=0, q1_empty=0, roi_1x1=0, roi_max_on_boundary=0,
             roi_threshold_follows=0, strongest_cuts_tie=0, strongest_all_sorted=0, overflow=0, f=set())
    for t, r in zip(TABLE, R.results()):
        p, plane = t["params"], r["plane"]
        rows, cols = plane.shape
        c["f"].add(p["f"])
        x0, y0, w, h = (1, 1, cols, rows) if p["roi"] is None else p["roi"]
        sub = plane[y0 - 1:y0 - 1 + h, x0 - 1:x0 - 1 + w]
        mmax = float(sub.max())
        if r["status"] == R.ERR_CAPACITY:
            assert r["count"] > 4 * p["max_keypoints"] and len(r["loc"]) == 0
            c["overflow"] += 1
            continue
        if mmax <= 0:
            assert r["count"] == 0
            if R.image(t["image"]).std() == 0:
                c["flat"] += 1
            elif p["method"] == R.HARRIS:
                c["harris_nonpositive"] += 1
            continue
        if p["strongest"]:
            full = R.detect(R.image(t["image"]), **dict(p, strongest=0))
            order = np.lexsort((np.arange(full["count"]), -full["metric"].astype(np.float64)))[:p["strongest"]]
            assert r["loc"].tobytes() == full["loc"][order].tobytes() and r["metric"].tobytes() == full["metric"][order].tobytes()
            if p["strongest"] < full["count"] and full["metric"][order[-1]] == np.sort(full["metric"])[::-1][p["strongest"]]:
                c["strongest_cuts_tie"] += 1
            if p["strongest"] >= full["count"] and full["count"] > 1 and (np.diff(order) < 0).any():
                c["strongest_all_sorted"] += 1
            continue
        pr, pc = _pixels(r)
        assert (np.diff(pr * cols + pc) > 0).all()                      # ascending in (row, column)
        assert (r["metric"] == plane[pr, pc]).all() and (r["metric"] > np.float32(p["min_quality"]) * np.float32(mmax)).all()
        dx, dy = r["loc"][:, 0] - (pc + 1), r["loc"][:, 1] - (pr + 1)
        for a, b, ex, ey in zip(pr, pc, dx, dy):
            z = plane[a, b]
            c["eq_row"] += int(b + 1 < cols and plane[a, b + 1] == z)
            c["eq_col"] += int(a + 1 < rows and plane[a + 1, b] == z)
            c["eq_diag"] += int(a + 1 < rows and ((b + 1 < cols and plane[a + 1, b + 1] == z) or (b > 0 and plane[a + 1, b - 1] == z))
                                and not (b + 1 < cols and plane[a, b + 1] == z) and plane[a + 1, b] != z)
            on_side = a in (0, rows - 1) or b in (0, cols - 1)
            if 0 < b < cols - 1:
                c["den_zero"] += int((plane[a, b - 1] - z) + (plane[a, b + 1] - z) == 0)
            else:
                assert ex == 0
            if 0 < a < rows - 1:
                c["den_zero"] += int((plane[a - 1, b] - z) + (plane[a + 1, b] - z) == 0)
            else:
                assert ey == 0
            if a in (0, rows - 1) and b in (0, cols - 1):
                c["image_corner"] += 1
            elif on_side:
                c[{0: "top", rows - 1: "bottom"}.get(a) or {0: "left", cols - 1: "right"}[b]] += 1
        c["half_plus"] += int((dx == 0.5).sum() + (dy == 0.5).sum())
        c["half_minus"] += int((dx == -0.5).sum() + (dy == -0.5).sum())
        assert (np.abs(dx) <= 0.5).all() and (np.abs(dy) <= 0.5).all()
        c["q0"] += int(p["min_quality"] == 0.0 and r["count"] > 0)
        if p["roi"] is not None:
            assert ((pc + 1 >= x0) & (pc + 1 < x0 + w) & (pr + 1 >= y0) & (pr + 1 < y0 + h)).all()
            c["roi_1x1"] += int(w == 1 and h == 1 and r["count"] == 1)
            ar, ac = np.unravel_index(np.argmax(sub), sub.shape)
            c["roi_max_on_boundary"] += int((ar in (0, h - 1) or ac in (0, w - 1)) and w > 1 and h > 1)
            gmax = float(plane.max())
            c["roi_threshold_follows"] += int(mmax < gmax and bool(((r["metric"] > p["min_quality"] * mmax) &
                                                                     (r["metric"] <= p["min_quality"] * gmax)).any()))
        if p["min_quality"] == 1.0:
            c["q1_empty"] += int(r["count"] == 0)
    return c


def test_census_of_the_table():
    c = _census()
    print(c)
    for key in ("eq_row", "eq_col", "eq_diag", "half_plus", "top", "bottom", "left", "right", "flat", "harris_nonpositive", "q0", "q1_empty",
                "roi_1x1", "roi_max_on_boundary", "roi_threshold_follows", "strongest_cuts_tie", "strongest_all_sorted", "overflow"):
        assert c[key] > 0, key
    assert c["image_corner"] >= 4 and {3, 5, 15} <= c["f"]
    # Unreachable at a detected corner, by the local-maximum rule: the neighbour before the corner on either axis
    # precedes it in row-major order, so l < z strictly and z >= g, hence den = (l - z) + (g - z) < 0 and
    # 0.5 (l - g) / den > -0.5.  Both are asserted as never reached, and vo_corner_offset itself is driven through
    # them below.
    assert c["den_zero"] == 0 and c["half_minus"] == 0


def test_offset_function_at_its_edges():
    """vo_corner_offset where no detected corner takes it: den == 0, the clamp at -0.5, a minimum (den > 0)."""
    assert R.offset(1.0, 1.0, 1.0) == 0.0 and R.offset(0.5, 1.0, 1.5) == 0.0            # den == 0
    assert R.offset(1.0, 1.0, 0.25) == -0.5 and R.offset(1.5, 1.0, 0.0) == -0.5         # l == z > g; clamped
    assert R.offset(0.25, 1.0, 1.0) == 0.5 and R.offset(0.0, 1.0, 1.5) == 0.5
    assert R.offset(2.0, 1.0, 3.0) == 0.0                                               # den > 0
    assert R.offset(0.5, 1.0, 0.5) == 0.0
    assert R.offset(0.5, 1.0, 0.75) == np.float32(0.5) * np.float32(0.5 - 0.75) / np.float32((0.5 - 1.0) + (0.75 - 1.0))


def test_capacity_of_the_caller():
    img = R.image("a:noise")
    full = R.detect(img)
    short = R.detect(img, capacity=full["count"] - 1)
    assert short["status"] == R.ERR_CAPACITY and short["count"] == full["count"]
    exact = R.detect(img, capacity=full["count"])
    assert exact["status"] == R.OK and exact["loc"].tobytes() == full["loc"].tobytes()


def test_python_refusals(vo):
    """Every host refusal of the Python layer: VOError(VO_ERR_ARG) naming the field, without a library."""
    ok = vo.default_corner_params()
    vo.check_corner_params(ok, 40, 56, 512)
    assert (ok.method, ok.filter_size, ok.strongest, tuple(ok.roi)) == (vo.VO_CORNER_MINEIG, 5, 0, (0, 0, 0, 0))
    assert ok.min_quality == np.float32(0.01)
    for kw, word in ((dict(method=2), "method"), (dict(method=-1), "method"), (dict(filter_size=4), "filter_size"),
                     (dict(filter_size=1), "filter_size"), (dict(filter_size=17), "filter_size"), (dict(min_quality=-0.01), "min_quality"),
                     (dict(min_quality=1.5), "min_quality"), (dict(min_quality=float("nan")), "min_quality"), (dict(strongest=-1), "strongest"),
                     (dict(strongest=513), "strongest"), (dict(roi=(1, 1, -1, 5)), "roi"), (dict(roi=(1, 1, 5, 0)), "roi"),
                     (dict(roi=(0, 1, 5, 5)), "roi"), (dict(roi=(1, 0, 5, 5)), "roi"), (dict(roi=(53, 1, 5, 5)), "roi"),
                     (dict(roi=(1, 37, 5, 5)), "roi"), (dict(roi=(57, 1, 1, 1)), "roi"), (dict(roi=(1, 41, 1, 1)), "roi")):
        with pytest.raises(vo.VOError) as e:
            vo.check_corner_params(vo.default_corner_params(**kw), 40, 56, 512)
        assert e.value.code == vo.VO_ERR_ARG and word in str(e.value), kw
    for kw in (dict(roi=(56, 40, 1, 1)), dict(roi=(1, 1, 56, 40)), dict(strongest=512), dict(min_quality=0.0), dict(min_quality=1.0),
               dict(filter_size=3), dict(filter_size=15), dict(method=vo.VO_CORNER_HARRIS), dict(roi=None)):
        vo.check_corner_params(vo.default_corner_params(**kw), 40, 56, 512)
    with pytest.raises(vo.VOError):
        vo.default_corner_params(no_such_field=1)
    for name in ("vo_default_corner_params", "vo_detect_corners", "vo_detect_corners_batch", "vo_fetch_corner_metric"):
        assert name in vo.EXPORTS


def test_sanitizer_run_of_the_border_roi_and_overflow_rows(tmp_path):
    """tests/corner_ref/corner_ref_main.c: the same C under -fsanitize=address,undefined, as a stand-alone program,
    over the rows whose windows leave the image, whose ROI ends at an image side, and whose list overflows; its
    output equals the library's."""
    R.build("asan")
    ran = 0
    for row, rec in zip(TABLE, R.results()):
        if not any(w in row["name"] for w in ("border", "roi", "overflow", "k16", "f15")):
            continue
        f = tmp_path / (row["name"] + ".bin")
        p = row["params"]
        R.write_problem(f, R.image(row["image"]), p["method"], p["f"], p["min_quality"], p["strongest"], p["roi"], p["max_keypoints"])
        out = subprocess.run([str(R.MAIN), str(f)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.split("\n")[:-1] == R.main_lines(rec), row["name"]
        ran += 1
    # an ROI that ends in the image's last row and column
    img = R.image("b:noise")
    rows, cols = img.shape
    roi = (cols - 6, rows - 4, 7, 5)
    f = tmp_path / "roi_last.bin"
    R.write_problem(f, img, roi=roi)
    out = subprocess.run([str(R.MAIN), str(f)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split("\n")[:-1] == R.main_lines(R.detect(img, roi=roi))
    assert ran >= 12


def test_corners_feed_the_tracker():
    """corner_ref on klt_ref's noise-free 97 x 121 image, then klt_ref (defaults, 31 x 31) to its copy shifted by
    (3.25, -2.5) px.  DESIGN.md 3.5.3 records a median error of at most 0.019 px for noise-free rows, on points at
    least 24 px from every side; the detector's corners in that region are held to it (measured 0.0158 px, 94
    corners).  Over all corners the median is 0.0223 px: two thirds of them lie within 24 px of a side, where the
    31 x 31 window is clipped and the copy, shifted periodically, shows other content."""
    img0, img1 = K.images("a:s0")
    rows, cols = img0.shape
    rec = R.detect(img0)
    assert rec["status"] == R.OK and rec["count"] > 100
    out = K.track(img0, img1, rec["loc"])
    err = np.sqrt(((out["pts1"] - rec["loc"] - np.float32(K.SHIFT)) ** 2).sum(1))
    x, y = rec["loc"][:, 0], rec["loc"][:, 1]
    inner = (x >= 25) & (x <= cols - 24) & (y >= 25) & (y <= rows - 24)
    v = out["valid"]
    print(f"{rec['count']} corners, {int(v.sum())} tracked, median error {np.median(err[v]):.4f} px; {int(inner.sum())} at least 24 px "
          f"inside, {int((v & inner).sum())} tracked, median {np.median(err[v & inner]):.4f} px, largest {err[v & inner].max():.4f} px")
    assert v[inner].all() and inner.sum() >= 50 and v.mean() > 0.9
    assert np.median(err[v & inner]) <= 0.019
