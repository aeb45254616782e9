"""csrc/blur_plan.h, the one place that decides how a scale-space blur is launched, against a
transcription of the rules as they stood before the header existed, when they were spread over
sift.hip's launch_blur_r (form, columns per lane, tag, band height, bands, grid strips),
blur_latency_bound (full bands: the fork octave of the two chains) and sift_enqueue_pyramid's own
condition for the octave-0 base from the u8 image.

The header is compiled with the host compiler (oracle/blur_plan_eval.cpp).  It must agree with the
transcription everywhere but in one region: there the old caller took the u8 base (tabled radius,
R >= 64) while the old launcher would not stream it (R < TH), and launched the tiled kernel with a
null source plane.  The plan does not stream there either, so the caller stages the float plane.

The transcriptions of sift.hip's small_plan and fork octave used below live in tests/blur_census.py,
which lists every launch of a call from these plans.  tests/test_blur_census.py walks this file's
sweep (ROWS, COLS, N_IMG) once more for the staged u8 base: every band of every streamed BaseU8
plan stages at most bs_u8_rows(r) source rows, the size of k_blur_stream's LDS array."""
import numpy as np
import pytest

import blur_census
from blur_census import BASE_FLOAT, BASE_U8, BS_P, FIELDS, LEVEL, fork_octave

TABLED = (5, 6, 8, 10, 13)

ROWS = np.arange(16, 4097, dtype=np.int64)
COLS = np.array(sorted({16, 128, 129, 1400, 1401, 2484, 4096}
                       | {m + d for step in (240, 128, 256) for m in range(step, 4097, step) for d in (-1, 0, 1)}),
                dtype=np.int64)
N_IMG = (1, 2, 4, 128, 136, 144, 512, 514)
RADII = (4, 5, 6, 7, 8, 10, 13, 14)


@pytest.fixture(scope="module")
def plan_lib(oracle):
    return blur_census.load_plan_lib(oracle)


def header_plan(lib, role, r, n_img, rows=ROWS, cols=COLS):
    return blur_census.header_plan(lib, role, r, n_img, rows, cols)


def old_bs_sw(r, cpl, tag):
    """bs_sw: output columns per strip (halo-lane layout at 4-column lanes, r <= 5, not probe bit 32)."""
    rh = (r + cpl - 1) // cpl * cpl
    hl = (cpl == 4) & (r <= 5) & ((tag & 32) == 0)
    return 64 * cpl - np.where(hl, 2 * rh, 0)


def old_rules(role, r, n_img, rows=ROWS, cols=COLS):
    """-> (fields, hole).  Fields of a launch that did not stream are 0; full_bands is
    blur_latency_bound negated, for level blurs only.  hole: the u8 base taken by the caller and
    refused by the launcher ("streamed" is 2 there: neither form the plan knows)."""
    R, Cc = np.asarray(rows, np.int64)[:, None], np.asarray(cols, np.int64)[None, :]
    R, Cc = np.broadcast_arrays(R, Cc)
    base = role != LEVEL
    tabled = r in TABLED                                         # launch_blur's switch: RAD > 0
    # launch_blur_r
    cpl = np.where((not base) & (Cc <= 1400), 2, 4)
    n_strips = (Cc + 64 * cpl - 1) // (64 * cpl)
    rows_total = R * n_strips * n_img
    TH = np.minimum(min(128, 96) if base else 128, rows_total // 2048)
    TH = np.maximum(BS_P, TH // BS_P * BS_P)
    streams = tabled & (R >= TH) & (R > r + BS_P + 2)
    tag = {LEVEL: 0, BASE_FLOAT: 1, BASE_U8: 5}[role]            # base && src == nullptr: 5; base: 1
    cpl_launch = np.where(base, 4, cpl)
    sw = old_bs_sw(r, cpl_launch, tag)
    hole = np.zeros(R.shape, bool)
    if role == BASE_U8:
        taken = tabled & (R >= 64)                               # sift_enqueue_pyramid: stream_r && R >= 64
        hole = taken & ~streams
        streams = taken & streams                                # not taken: k_base_src, then the float-plane base
    f = {"streamed": streams, "cpl": cpl_launch, "tag": np.full(R.shape, tag), "th": TH, "n_bands": (R + TH - 1) // TH,
         "n_strips": (Cc + sw - 1) // sw}
    f = {k: np.where(streams, v, 0).astype(np.int32) for k, v in f.items()}
    f["streamed"][hole] = 2                                      # a third form: the tiled kernel, no source plane
    # blur_latency_bound, with the level blur's columns per lane whatever the radius
    lc = np.where(Cc <= 1400, 2, 4)
    ls = (Cc + 64 * lc - 1) // (64 * lc)
    latency_bound = R * ls * n_img // 2048 < 128
    f["full_bands"] = (~latency_bound if role == LEVEL else np.zeros(R.shape, bool)).astype(np.int32)
    return f, hole


@pytest.mark.parametrize("role", [LEVEL, BASE_FLOAT, BASE_U8])
def test_plan_equals_the_old_rules(plan_lib, role):
    hole_total = 0
    for r in RADII:
        for n_img in N_IMG:
            new = header_plan(plan_lib, role, r, n_img)
            old, hole = old_rules(role, r, n_img)
            differs = np.zeros(hole.shape, bool)
            for k in FIELDS:
                differs |= new[k] != old[k]
            # the plan differs from the old rules exactly where the old rules launched the tiled
            # kernel without a source plane, and there it does not stream
            assert np.array_equal(differs, hole), (role, r, n_img, np.argwhere(differs != hole)[:5])
            assert not new["streamed"][hole].any()
            hole_total += int(hole.sum())
            # a streamed plan: whole bands of BS_P-row blocks inside the plane, one reflection fold
            s = new["streamed"] == 1
            Rr = np.broadcast_to(ROWS[:, None], s.shape)
            assert (Rr[s] >= new["th"][s]).all() and (Rr[s] > r + BS_P + 2).all() and (new["th"][s] % BS_P == 0).all()
            assert (new["th"][s] >= BS_P).all() and (new["n_bands"][s] >= 1).all() and (new["n_strips"][s] >= 1).all()
            if role == BASE_U8:
                assert (new["th"][s] <= 96).all() and (Rr[s] >= 64).all()
            if r in TABLED:
                assert s[Rr >= 128].all()                        # a tabled radius streams every plane of a band's height
            else:
                assert not s.any()
    if role != BASE_U8:
        assert hole_total == 0
    else:
        # the size of the region, from the old rules alone: 64 <= R < TH <= 96 needs R n_strips
        # n_img / 2048 >= 68, i.e. n_img >= 128 in this sweep (17 strips at 4096 columns and over)
        want = 0
        for r in TABLED:
            for n_img in N_IMG:
                for c in COLS:
                    ns = (int(c) + 255) // 256
                    for R in range(64, 96):
                        th = max(4, min(96, R * ns * n_img // 2048) // 4 * 4)
                        want += R < th
        assert hole_total == want and want > 0
        print(f"u8 base points of the sweep that no longer stream: {hole_total}")


def test_the_hole_shape_of_the_issue(plan_lib):
    """32 x 2048 images (R = 64, C = 4096, 16 nominal strips): the old launcher's TH passes 64 from
    136 images on; the plan streams the u8 base below that and stages the float plane from there."""
    for n_img, streams in ((128, 1), (135, 1), (136, 0), (144, 0), (512, 0)):
        new = header_plan(plan_lib, BASE_U8, 5, n_img, [64], [4096])
        assert new["streamed"][0, 0] == streams, n_img
        flt = header_plan(plan_lib, BASE_FLOAT, 5, n_img, [64], [4096])
        assert flt["streamed"][0, 0] == streams                   # the staged plane's blur is tiled there too


@pytest.mark.parametrize("rows,cols", [(375, 1242), (1080, 1920)])
def test_fork_octave_does_not_move(plan_lib, rows, cols):
    from r7020e_visual_odometry_amd import roofline
    dims = roofline.octave_dims(rows, cols)
    forks = {}
    for frames in (1, 16, 32, 64, 128, 256, 512):                # bench.py: --batch, --seq-batch, --large-batch
        n_img = 2 * frames
        new = fork_octave(dims, lambda R, Cc: bool(header_plan(plan_lib, LEVEL, 6, n_img, [R], [Cc])["full_bands"][0, 0]))
        old = fork_octave(dims, lambda R, Cc: bool(old_rules(LEVEL, 6, n_img, [R], [Cc])[0]["full_bands"][0, 0]))
        assert new == old, (frames, new, old)
        forks[frames] = new
    assert forks[1] == 1                                         # nothing at full bands: the default fork
    print(f"{rows} x {cols}: fork octave by frames per batch {forks}")
