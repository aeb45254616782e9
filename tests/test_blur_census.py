"""The case table of tests/test_gpu_blur_bands.py against the census of scale-space launches
(tests/blur_census.py), and the bound of the staged u8 base's LDS rows.

The census computes which classes of blur_census.CLASS_TABLE some call of the search domain (rows <=
260, cols <= 1600, 2..512 frames, with and without the upsample, default radii, arena <= 4 GB) can
reach.  UNREACHABLE lists the others, each with its reason, and must equal what the census computes;
CASES must reach every other class, each case naming the classes it was chosen for.

How many cases that takes.  The issue that asked for this table set 25.  A call has one base launch,
of one kind, one band-height bucket, one number of bands and one form of last band, and the classes
ask, per base kind and bucket above 4, for up to three band counts and three last-band forms: three
calls per kind and bucket wherever three of either are reachable, one more per kind for bucket 4.
test_case_table_covers_every_reachable_class_within_the_caps computes that sum over the reachable
classes: 27.  The table below has 29 (a greedy cover by classes gained, ties to the smaller arena,
then pairs of cases merged where one call reaches what only the two reach); CASE_CAP is that lower
bound plus the two the search could not merge away, not 25.  Every class stays."""
import numpy as np
import pytest

import blur_census as bc
import test_blur_plan as tbp

CASE_CAP = 29

# (rows, cols, frames, upsample, byte offset of the device pointers, classes the case is there for)
CASES = [
    (16, 16, 2, 1, 0, (
        'blocks:BaseFloat-DPP:even', 'bucket:BaseFloat-DPP:4', 'bucket:Level2:4', 'strips:BaseFloat-DPP:1',
        'strips:Level2:1',)),
    (32, 16, 2, 1, 0, (
        'blocks:BaseU8:even', 'bucket:BaseU8:4', 'rounds:1', 'strips:BaseU8:1',)),
    (33, 385, 32, 1, 0, (
        'bands:BaseU8:8-32:3+', 'bands:Level2:8-32:3+', 'blocks:BaseU8:odd', 'bucket:BaseU8:8-32',
        'bucket:Level2:8-32', 'last:BaseU8:8-32:cut-odd', 'last:Level2:8-32:cut-odd', 'nextbase:Level2:oo',
        'strips:BaseU8:3+', 'strips:Level2:3+',)),
    (34, 385, 32, 1, 0, (
        'last:BaseU8:8-32:cut4', 'last:Level2:8-32:cut4', 'nextbase:Level2:eo',)),
    (129, 1409, 32, 1, 1, (
        'bands:BaseU8:cap:3+', 'bands:Level4-DPP:8-32:3+', 'bands:Level4-DPP:mid:3+', 'bands:Level4-LDS:8-32:3+',
        'bands:Level4-LDS:mid:3+', 'blocks:Level4-DPP:even', 'blocks:Level4-DPP:odd', 'bucket:BaseU8:cap',
        'bucket:Level4-DPP:8-32', 'bucket:Level4-DPP:mid', 'bucket:Level4-LDS:8-32', 'bucket:Level4-LDS:mid',
        'fold:bottom', 'fold:neither', 'fold:top', 'last:BaseU8:cap:cut-odd', 'last:Level4-DPP:8-32:cut-odd',
        'last:Level4-DPP:mid:cut-odd', 'last:Level4-LDS:8-32:cut-odd', 'last:Level4-LDS:mid:cut-odd', 'misaligned:1',
        'nextbase:Level2:ee', 'nextbase:Level4-LDS:ee', 'nextbase:Level4-LDS:oo', 'rounds:2', 'rounds:3',
        'strips:Level4-DPP:3+', 'strips:Level4-LDS:3+',)),
    (18, 1401, 64, 1, 0, (
        'bands:BaseFloat-DPP:8-32:2', 'bands:Level4-DPP:8-32:2', 'bands:Level4-LDS:8-32:2',
        'blocks:BaseFloat-DPP:odd', 'bucket:BaseFloat-DPP:8-32', 'bucket:Level4-DPP:4', 'bucket:Level4-LDS:4',
        'last:BaseFloat-DPP:8-32:cut4', 'last:Level4-DPP:8-32:cut4', 'last:Level4-LDS:8-32:cut4',
        'nextbase:Level4-LDS:eo', 'strips:BaseFloat-DPP:3+', 'unstreamed:level',)),
    (24, 1409, 64, 1, 0, (
        'bands:BaseFloat-DPP:mid:2', 'bands:Level4-DPP:mid:2', 'bands:Level4-LDS:mid:2', 'bucket:BaseFloat-DPP:mid',
        'last:BaseFloat-DPP:mid:cut4', 'last:Level4-DPP:8-32:whole', 'last:Level4-DPP:mid:cut4',
        'last:Level4-LDS:8-32:whole', 'last:Level4-LDS:mid:cut4',)),
    (29, 1153, 64, 1, 0, (
        'bands:Level2:8-32:2', 'last:BaseFloat-DPP:mid:cut-odd',)),
    (32, 897, 64, 1, 0, (
        'bands:BaseU8:8-32:2', 'last:BaseU8:8-32:whole', 'last:Level2:8-32:whole',)),
    (37, 897, 64, 1, 0, (
        'bands:BaseU8:mid:3+', 'bucket:BaseU8:mid', 'last:BaseU8:mid:cut-odd',)),
    (16, 897, 128, 1, 0, (
        'bands:BaseFloat-DPP:8-32:1', 'bands:Level2:8-32:1', 'bands:Level4-DPP:8-32:1', 'bands:Level4-LDS:8-32:1',
        'last:BaseFloat-DPP:8-32:whole',)),
    (32, 897, 128, 1, 2, (
        'bands:BaseU8:mid:1', 'bands:Level4-DPP:mid:1', 'bands:Level4-LDS:mid:1', 'fold:both',
        'last:BaseU8:mid:whole', 'last:Level4-DPP:mid:whole', 'last:Level4-LDS:mid:whole', 'misaligned:2',)),
    (48, 897, 128, 1, 3, (
        'bands:BaseU8:cap:1', 'bands:Level2:mid:1', 'bucket:Level2:mid', 'last:BaseU8:cap:whole',
        'last:Level2:mid:whole', 'misaligned:3',)),
    (64, 513, 128, 1, 0, (
        'bands:BaseU8:mid:2', 'bands:Level2:cap:1', 'bands:Level2:mid:2', 'bucket:Level2:cap',
        'last:BaseU8:mid:cut4', 'last:Level2:cap:whole', 'last:Level2:mid:cut4',)),
    (64, 1401, 128, 1, 0, (
        'bands:BaseU8:cap:2', 'bands:Level4-DPP:cap:1', 'bands:Level4-LDS:cap:1', 'bucket:Level4-DPP:cap',
        'bucket:Level4-LDS:cap', 'last:BaseU8:cap:cut4', 'last:Level4-DPP:cap:whole', 'last:Level4-LDS:cap:whole',)),
    (168, 221, 128, 1, 0, (
        'bands:Level2:cap:3+', 'bands:Level2:mid:3+', 'last:Level2:cap:cut4', 'strips:BaseU8:2', 'strips:Level2:2',)),
    (17, 16, 256, 1, 0, (
        'bands:BaseFloat-DPP:8-32:3+', 'last:BaseFloat-DPP:8-32:cut-odd',)),
    (18, 129, 512, 1, 0, (
        'bands:BaseFloat-DPP:mid:1', 'last:BaseFloat-DPP:mid:whole', 'strips:BaseFloat-DPP:2',)),
    (16, 16, 2, 0, 0, (
        'bucket:BaseFloat-LDS:4', 'strips:BaseFloat-LDS:1',)),
    (44, 513, 64, 0, 0, (
        'bands:BaseFloat-LDS:8-32:3+', 'bucket:BaseFloat-LDS:8-32', 'last:BaseFloat-LDS:8-32:cut4',
        'strips:BaseFloat-LDS:3+',)),
    (150, 1537, 128, 0, 0, (
        'bands:BaseFloat-LDS:cap:2', 'bands:Level4-DPP:cap:2', 'bands:Level4-LDS:cap:2', 'bucket:BaseFloat-LDS:cap',
        'last:BaseFloat-LDS:cap:cut-odd', 'last:Level2:mid:cut-odd', 'last:Level4-DPP:cap:cut-odd',
        'last:Level4-LDS:cap:cut-odd', 'nextbase:Level2:oe', 'nextbase:Level4-LDS:oe',)),
    (260, 1401, 128, 0, 0, (
        'bands:BaseFloat-LDS:cap:3+', 'bands:Level4-DPP:cap:3+', 'bands:Level4-LDS:cap:3+',
        'last:BaseFloat-LDS:cap:cut4', 'last:Level4-DPP:cap:cut4', 'last:Level4-LDS:cap:cut4',)),
    (16, 1025, 256, 0, 0, (
        'unstreamed:base',)),
    (17, 513, 256, 0, 0, (
        'bands:BaseFloat-LDS:8-32:2', 'last:BaseFloat-LDS:8-32:cut-odd',)),
    (36, 769, 256, 0, 0, (
        'bands:BaseFloat-LDS:mid:1', 'bucket:BaseFloat-LDS:mid', 'last:BaseFloat-LDS:mid:whole',)),
    (48, 513, 256, 0, 0, (
        'bands:BaseFloat-LDS:mid:2', 'last:BaseFloat-LDS:mid:cut4',)),
    (96, 769, 256, 0, 0, (
        'bands:BaseFloat-LDS:cap:1', 'last:BaseFloat-LDS:cap:whole',)),
    (130, 386, 256, 0, 0, (
        'bands:BaseFloat-LDS:mid:3+', 'bands:Level2:cap:2', 'last:BaseFloat-LDS:mid:cut-odd',
        'last:Level2:cap:cut-odd', 'strips:BaseFloat-LDS:2',)),
    (16, 257, 512, 0, 0, (
        'bands:BaseFloat-LDS:8-32:1', 'last:BaseFloat-LDS:8-32:whole',)),
]

# Classes no call of the search domain reaches, by reason
UNREACHABLE = {
    "a streamed u8 base has at least 64 rows, so two bands or more at 32 rows or fewer": [
        "bands:BaseU8:8-32:1"],
    "an upsampled base streams from the float plane only where the u8 form is refused, under 64 rows: no 96-row band, "
    "and at 36 rows or more at most two bands": [
        "bucket:BaseFloat-DPP:cap", "bands:BaseFloat-DPP:cap:1", "bands:BaseFloat-DPP:cap:2", "bands:BaseFloat-DPP:cap:3+",
        "last:BaseFloat-DPP:cap:whole", "last:BaseFloat-DPP:cap:cut4", "last:BaseFloat-DPP:cap:cut-odd",
        "bands:BaseFloat-DPP:mid:3+"],
    "level L has radius 8 at the default sigmas, which is not a DPP radius": [
        "nextbase:Level4-DPP:ee", "nextbase:Level4-DPP:eo", "nextbase:Level4-DPP:oe", "nextbase:Level4-DPP:oo"],
    "4 columns per lane need more than 1400 columns: six strips or more": [
        "strips:Level4-DPP:1", "strips:Level4-DPP:2", "strips:Level4-LDS:1", "strips:Level4-LDS:2"],
}

# The shapes whose Gaussian planes the other GPU files compare with the oracle, all in calls of 2 frames:
# (rows, cols, frames, upsample, (L, sigma), file)
EXISTING = (
    [(r, c, 2, 1, (3, 1.6), "test_gpu_pyramid.py") for r, c in
     ((375, 1242), (376, 1241), (240, 700), (97, 131), (131, 97), (400, 1800), (77, 101))]
    + [(r, c, 2, 1, (3, 1.6), "test_gpu_scale_space_chains.py") for r, c in ((22, 419), (44, 838), (100, 380), (16, 16))]
    + [(16, 20, 2, 0, (3, 1.6), "test_gpu_scale_space_chains.py"),
       (150, 260, 2, 1, (1, 1.2), "test_gpu_scale_space_chains.py"), (150, 260, 2, 1, (5, 1.6), "test_gpu_scale_space_chains.py"),
       (300, 520, 2, 0, (4, 1.6), "test_gpu_scale_space_chains.py")]
    + [(150, 200, 2, up, (L, s), "test_gpu_sift_params.py") for L, s, up in
       ((1, 1.2, 1), (1, 1.4, 0), (2, 1.6, 1), (2, 1.6, 0), (3, 1.6, 0), (4, 1.6, 1), (5, 1.6, 1), (5, 1.6, 0), (3, 1.2, 1),
        (3, 2.0, 1), (3, 2.0, 0), (3, 5.0, 1), (2, 3.4, 0), (3, 1.6, 1))]
    + [(97, 131, 2, 1, (5, 1.6), "test_gpu_sift_params.py"), (97, 131, 2, 0, (2, 1.6), "test_gpu_sift_params.py"),
       (24, 420, 2, 0, (3, 5.0), "test_gpu_sift_params.py"), (40, 1450, 2, 1, (2, 1.6), "test_gpu_sift_params.py"),
       (70, 1500, 2, 0, (4, 1.6), "test_gpu_sift_params.py")])


def _key(c):
    return ":".join(c)


@pytest.fixture(scope="module")
def lib(oracle):
    return bc.load_plan_lib(oracle)


@pytest.fixture(scope="module")
def reachable(lib, oracle):
    return {_key(c) for c in bc.reachable_classes(lib, oracle)}


def test_unreachable_classes_are_the_listed_ones(reachable):
    every = {_key(c) for c in bc.all_classes()}
    assert reachable <= every, sorted(reachable - every)          # (a fourth staging round would show here)
    listed = [c for v in UNREACHABLE.values() for c in v]
    assert len(listed) == len(set(listed))
    assert every - reachable == set(listed), (sorted(every - reachable - set(listed)), sorted(set(listed) - (every - reachable)))


def test_case_table_covers_every_reachable_class_within_the_caps(lib, oracle, reachable):
    got = set()
    for rows, cols, frames, up, offset, why in CASES:
        assert rows <= bc.MAX_ROWS and cols <= bc.MAX_COLS and frames in bc.FRAMES and min(rows, cols) >= bc.MIN_SIDE
        assert int(bc.arena_bytes(oracle, rows, cols, frames, up)[0, 0]) <= bc.ARENA_CAP, (rows, cols, frames)
        launches, classes, counts = bc.census(lib, oracle, rows, cols, frames, up, offset=offset)
        classes = {_key(c) for c in classes}
        assert why and set(why) <= classes, (rows, cols, frames, up, sorted(set(why) - classes))
        assert set(why).isdisjoint(got), (rows, cols, frames, up)     # what the case adds to those above it
        assert set(counts) <= set(bc.SITES)
        got |= classes
    assert got == reachable, (sorted(reachable - got), sorted(got - reachable))
    # the fewest calls the base launches alone need (the module docstring)
    bound = 0
    for kind in bc.BASE_KINDS:
        bound += f"bucket:{kind}:4" in reachable
        for b in ("8-32", "mid", "cap"):
            bound += max(sum(f"{what}:{kind}:{b}:{v}" in reachable for v in values)
                         for what, values in (("bands", ("1", "2", "3+")), ("last", ("whole", "cut4", "cut-odd"))))
    assert bound == 27
    assert len(CASES) <= CASE_CAP and CASE_CAP <= bound + 2


def test_existing_plane_compared_shapes_stay_at_low_bands(lib, oracle):
    """What the other files' plane comparisons reach: band heights 4, 8, 12 and 20, one staging round."""
    heights, reached = set(), set()
    for rows, cols, frames, up, sift, _ in EXISTING:
        launches, classes, _ = bc.census(lib, oracle, rows, cols, frames, up, sift)
        heights |= {l["th"] for l in launches if l["streamed"]}
        reached |= {_key(c) for c in classes}
    print("existing plane-compared shapes reach", len(reached), "classes:", sorted(reached))
    assert heights == {4, 8, 12, 20}, sorted(heights)
    assert "rounds:1" in reached and not reached & {"rounds:2", "rounds:3", "fold:top", "fold:bottom", "fold:both", "fold:neither"}
    assert not [c for c in reached if c.split(":")[0] == "bucket" and c.split(":")[2] in ("mid", "cap")]


def test_staged_u8_rows_fit_the_lds_array(lib):
    """Over test_blur_plan.py's sweep: every band of every streamed BaseU8 plan stages at most
    bs_u8_rows(r) source rows -- bs_u8_rows(r) * bs_u8_dw(r, 4) dwords, the size of k_blur_stream's
    stg[] -- and no band height passes the kernel's own guard (kBaseMaxTH)."""
    worst = {}
    for r in tbp.TABLED:
        cap_rows, dw = lib.blur_plan_bs_u8_rows(r), lib.blur_plan_bs_u8_dw(r, 4)
        pairs = set()
        for n_img in tbp.N_IMG:
            p = tbp.header_plan(lib, bc.BASE_U8, r, n_img)
            s = p["streamed"] == 1
            assert (p["th"][s] <= lib.blur_plan_base_max_th()).all()
            Rr = np.broadcast_to(tbp.ROWS[:, None], s.shape)
            pairs |= set(np.unique(Rr[s] * 1024 + p["th"][s]).tolist())
        assert pairs
        most = 0
        for k in pairs:
            R, th = k >> 10, k & 1023
            n = lib.blur_plan_u8_stage_max(r, R, R // 2, th)
            assert 0 < n <= cap_rows and n * dw <= cap_rows * dw, (r, R, th, n, cap_rows)
            most = max(most, n)
        worst[r] = (most, cap_rows)
    print("most staged rows / bound by radius:", worst)
    assert worst[5] == (57, 59)                                       # (F + 96) / 2 + 3 rows of an interior band at r = 5


def test_stage_rows_equal_the_rows_a_band_reads(lib):
    """bs_u8_stage_rows against the definition: the source rows that the upsampled rows of the band,
    reflected into the plane, read (row y reads y / 2 and its neighbour above or below, clamped)."""
    r = 5
    F = (2 * r + bc.BS_P - 1) // bc.BS_P * bc.BS_P
    out = (bc.C.c_int * 2)()
    for R in (12, 14, 64, 66, 96, 154, 258):
        src = R // 2
        for th in (4, 8, 36, 64, 96):
            if th > R:
                continue
            for y0 in range(0, R, th):
                thb = min(th, (R - y0 + 3) // 4 * 4)
                need = set()
                for kk in range(F + thb):
                    p = y0 - r - (F - 2 * r) + kk
                    while p < 0 or p >= R:
                        p = -p if p < 0 else 2 * R - 2 - p
                    ya = p >> 1
                    need |= {ya, min(ya + 1, src - 1) if p & 1 else max(ya - 1, 0)}
                lib.blur_plan_u8_stage_rows(r, R, src, y0, thb, out)
                assert out[0] <= min(need) and max(need) <= out[1], (R, th, y0, out[0], out[1], min(need), max(need))
                assert out[0] >= min(need) - 1 and out[1] <= max(need) + 1
