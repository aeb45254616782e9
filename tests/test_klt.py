"""CPU: the specification of the point tracker (include/vo_spec.h vo_klt_*), through its CPU
build tests/klt_ref -- the functions k_klt_pyr and k_klt_track call, which tests/test_gpu_klt.py compares
with the kernels by bytes.  Here the reference is held to its properties (identical images, a known
sub-pixel shift), its pyramid to a direct numpy evaluation by bytes, its positions to an independent
float64 restatement (tests/klt_f64_ref.py), and a census is asserted so that the table the GPU test
replays reaches every outcome.  The host refusals of the Python layer and the sanitizer run of the same C
(a stand-alone program, host code only) are here too.  Each test prints its figures before it asserts."""
import subprocess

import numpy as np
import pytest

import klt_f64_ref as F
import klt_ref as R

TABLE = R.table()
NAMES = [row["name"] for row in TABLE]

# The largest |pts1 - pts1_f64| measured over the compared rows (interior points, windows >= 11, noise <= 8,
# both evaluations valid with the same outcome at every level): 1.35e-3 px (row shift_a_31_L6; 595 of 600 rows
# kept).  The gate is 4 x that: the margin covers rint ties in the weights, not retuning.
F64_MEASURED = 1.35e-3
F64_GATE = 4 * F64_MEASURED
F64_MAX_DROPPED = 0.10


def _row(name):
    i = NAMES.index(name)
    return TABLE[i], R.results()[i]


@pytest.mark.parametrize("name", ["same_a_31_L3", "same_b_5_L1"])
def test_identical_images_return_the_input_points(name):
    row, rec = _row(name)
    dev = np.abs(rec["pts1"] - row["pts"]).max()
    print(name, "max |pts1 - pts0|", dev)
    assert rec["valid"].all()
    assert dev <= 1e-5
    assert (rec["info"]["stop"] == R.STOP_EPS).all() and (rec["info"]["iterations"] == 1).all()
    assert (rec["info"]["status"] == R.OK).all() and np.isnan(rec["info"]["bidir_error"]).all()
    assert (rec["scores"] == 1.0).all()


@pytest.mark.parametrize("key", ["a:s0", "b:s8", "a:const"])
def test_pyramid_equals_a_direct_numpy_evaluation_by_bytes(key):
    for img in R.images(key):
        got, exp = R.pyramid(img, 6), F.pyramid(img, 6)
        assert [g.shape for g in got] == R.level_dims(*img.shape, 6)
        for l, (g, e) in enumerate(zip(got, exp)):
            assert g.dtype == np.uint8 and g.tobytes() == e.tobytes(), (key, l)


def test_a_subpixel_shift_is_recovered():
    for name in ("shift_a_31_L3", "shift_a_11_L3", "shift_b_31_L3", "shift_a_31_L1", "shift_a_31_L6"):
        row, rec = _row(name)
        d = rec["pts1"] - row["pts"] - np.float32(row["shift"])
        med = float(np.median(np.hypot(d[:, 0], d[:, 1])[rec["valid"]]))
        print(name, "median error", med, "valid", int(rec["valid"].sum()), "of", len(d))
        assert rec["valid"].all() and med < 0.05          # quantised, band-limited textures: a few hundredths of a pixel


def test_invalid_points_return_their_input_and_score_zero():
    for row, rec in zip(TABLE, R.results()):
        bad = ~rec["valid"]
        assert np.array_equal(rec["valid"], rec["info"]["status"] == R.OK)
        assert rec["pts1"][bad].tobytes() == row["pts"][bad].tobytes()
        assert (rec["scores"][bad] == 0.0).all()
        s = rec["scores"][~bad]
        assert ((s > 0.0) & (s <= 1.0)).all()


def _clipped_sides(row, rec):
    """Which image sides clip the level-0 window of a valid point's result: (left, right, top, bottom)."""
    bh, bw = row["params"]["block"]
    rows, cols = R.images(row["images"])[0].shape
    p = rec["pts1"][rec["valid"]] - 1.0
    hx, hy = (bw - 1) * 0.5, (bh - 1) * 0.5
    return np.array([(p[:, 0] - hx < 0).any(), (p[:, 0] + hx > cols - 1).any(), (p[:, 1] - hy < 0).any(), (p[:, 1] + hy > rows - 1).any()])


def test_census():
    """What the table reaches; tests/test_gpu_klt.py replays every row against the kernel by bytes."""
    res = R.results()
    info = np.concatenate([r["info"] for r in res])
    valid = np.concatenate([r["valid"] for r in res])
    print("status", np.bincount(info["status"], minlength=5), "stop", np.bincount(info["stop"], minlength=4))
    assert set(info["status"]) == {R.OK, R.TEMPLATE_OUT, R.LOST, R.FLAT, R.BIDIR}
    assert set(info["stop"]) == {R.STOP_NONE, R.STOP_EPS, R.STOP_OSC, R.STOP_MAXIT}
    assert ((info["levels_skipped"] > 0) & valid).any()
    # the window leaving the level during the level-0 iterations, and the result leaving the image
    lost = info[info["status"] == R.LOST]
    assert (lost["stop"] == R.STOP_NONE).any() and (lost["stop"] != R.STOP_NONE).any()
    sides = np.zeros(4, bool)
    for row, rec in zip(TABLE, res):
        if row["name"].startswith("sides_"):
            sides |= _clipped_sides(row, rec)
    assert sides.all(), sides
    # integer coordinates: w00 = 16384
    assert any((row["pts"] == np.rint(row["pts"])).all(1).any() for row in TABLE)
    blocks = {tuple(row["params"]["block"]) for row in TABLE}
    assert {(5, 5), (31, 31), (7, 21)} <= blocks
    assert {1, 3, 6} <= {row["params"]["levels"] for row in TABLE}
    row, rec = _row("shift_a_31_it1")
    assert row["params"]["max_it"] == 1 and (rec["info"]["iterations"] == 1).all()
    assert set(rec["info"]["stop"]) <= {R.STOP_EPS, R.STOP_MAXIT} and (rec["info"]["stop"] == R.STOP_MAXIT).any()
    # a guess rescues a 30-px shift which fails without it
    row, rec = _row("far_a_11_L1")
    e = np.hypot(*(rec["pts1"] - row["pts"] - np.float32(row["shift"])).T)
    assert not (rec["valid"] & (e < 1.0)).any()
    row, rec = _row("far_a_11_L1_guess")
    e = np.hypot(*(rec["pts1"] - row["pts"] - np.float32(row["shift"])).T)
    assert rec["valid"].all() and e.max() < 0.1, e.max()
    # bidirectional accept and reject
    for name in ("bidir_a_31_L3", "bidir_a_5_L3_n25"):
        row, rec = _row(name)
        e, st = rec["info"]["bidir_error"], rec["info"]["status"]
        assert (e[st == R.OK] <= row["params"]["max_bidir"]).all()
        rej = st == R.BIDIR
        assert (np.isnan(e[rej]) | (e[rej] > row["params"]["max_bidir"])).all()
    assert _row("bidir_a_31_L3")[1]["valid"].all()
    st = _row("bidir_a_5_L3_n25")[1]["info"]["status"]
    assert (st == R.OK).any() and (st == R.BIDIR).any()


def test_bidirectional_pass_only_removes_points():
    """The forward result of an accepted point is the one-way result, by bytes."""
    for name, one_way in (("bidir_a_31_L3", "shift_a_31_L3"), ("bidir_a_5_L3_n25", "noisy_a_5_L3")):
        (_, rec), (_, fwd) = _row(name), _row(one_way)
        ok = rec["valid"]
        assert fwd["valid"][ok].all() and rec["pts1"][ok].tobytes() == fwd["pts1"][ok].tobytes()
        assert rec["scores"][ok].tobytes() == fwd["scores"][ok].tobytes()


def test_reference_agrees_with_the_float64_restatement():
    worst, total, kept = 0.0, 0, 0
    for row, rec in zip(TABLE, R.results()):
        if not row["compare"]:
            continue
        assert min(row["params"]["block"]) >= 11 and row["guess"] is None
        p = row["params"]
        pts1, status, codes = F.track(*R.images(row["images"]), row["pts"], None, p["levels"], p["block"], p["max_it"])
        same = rec["valid"] & (status == F.OK) & (codes == rec["level_codes"]).all(1)
        dev = np.abs(pts1 - rec["pts1"]).max(1)
        print(row["name"], "rows", len(same), "kept", int(same.sum()), "max dev", float(dev[same].max()))
        total += len(same)
        kept += int(same.sum())
        worst = max(worst, float(dev[same].max()))
    print("worst", worst, "kept", kept, "of", total)
    assert total >= 240 and total - kept <= F64_MAX_DROPPED * total
    assert worst <= F64_GATE


def test_host_refusals(vo):
    d = vo.default_klt_params()
    assert (d.num_pyramid_levels, tuple(d.block_size), d.max_iterations, d.max_bidirectional_error) == (3, (31, 31), 30, float("inf"))
    vo.check_klt_params(d)
    for bad in (dict(num_pyramid_levels=0), dict(num_pyramid_levels=7), dict(block_size=(3, 31)), dict(block_size=(31, 33)),
                dict(block_size=(12, 31)), dict(max_iterations=0), dict(max_iterations=51), dict(max_bidirectional_error=0.0),
                dict(max_bidirectional_error=-1.0), dict(max_bidirectional_error=float("nan"))):
        with pytest.raises(vo.VOError) as e:
            vo.check_klt_params(vo.default_klt_params(**bad))
        assert e.value.code == vo.VO_ERR_ARG and next(iter(bad)).split("_")[0] in str(e.value), bad
    with pytest.raises(vo.VOError):
        vo.default_klt_params(window=5)
    for pts, word in ((np.zeros((3, 3)), "n x 2"), ([[1.0, np.nan]], "row 0"), ([[1, 1], [np.inf, 2]], "row 1"),
                      ([[1, 1], [2, 2], [3, -2.0 ** 20]], "row 2")):
        with pytest.raises(vo.VOError) as e:
            vo.klt_points(pts)
        assert e.value.code == vo.VO_ERR_ARG and word in str(e.value)
    assert vo.klt_points(np.zeros((0, 2))).shape == (0, 2)
    assert vo.klt_points(np.zeros(2, vo.KP_DTYPE)).shape == (2, 2)
    assert vo.KLT_INFO_DTYPE == R.INFO_DTYPE and vo.KLT_INFO_DTYPE.itemsize == 8


def test_sanitizer_run_of_the_clipped_and_outside_rows(tmp_path):
    """tests/klt_ref/klt_ref_main.c: the same C under -fsanitize=address,undefined, as a stand-alone program,
    over the rows whose windows are clipped or outside the image; its output equals the library's."""
    R.build("asan")
    ran = 0
    for row, rec in zip(TABLE, R.results()):
        if "sides" not in row["name"] and not row["name"].startswith("const_b_5"):
            continue
        f = tmp_path / (row["name"] + ".bin")
        p = row["params"]
        R.write_problem(f, *R.images(row["images"]), row["pts"], row["guess"], p["levels"], p["block"], p["max_it"], p["max_bidir"])
        out = subprocess.run([str(R.MAIN), str(f)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.split("\n")[:-1] == R.main_lines(rec), row["name"]
        ran += 1
    assert ran >= 6
