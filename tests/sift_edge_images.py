"""Fixture images for the SIFT stages after the scale space, and the census of the branches they
reach.  Test infrastructure (tests/test_sift_f64_ref.py, tests/test_gpu_sift_stages.py).

Every image is 96 x 144 uint8 and generated here, deterministically, from Gaussian blobs, patches
and one synthetic texture; `analyse` runs the float64 reference (tests/sift_f64_ref.py) on the
planes of oracle.pyramid, and `census` counts, over PARAM_SETS, the members of every class of
CENSUS_CLASSES.  Each class needs CENSUS_MIN members, and no candidate and no orientation peak of
a fixture image may be *undecided*: closer to one of its decisions than the bands below.  The
images are the outcome of a seed search over their generators (see images()) in which the reference
alone showed both.

The candidate bands are 8 x the largest oracle-to-reference gap measured over the fixture set on
the quantity the decision is taken on, rounded up, and within caps of 1e-4 on the offset and 1e-3
relative on the contrast and edge tests.  tests/test_sift_f64_ref.py measures the gaps again,
holds the bands to them and explains the orientation's figures:

    quantity                                  measured gap   band
    offset (via x, y in image px)             7.4e-6         OFFSET_BAND    6e-5
    contrast (via the response, relative)     1.51e-7        CONTRAST_BAND  1.3e-6
    edge terms (float32 against float64)      1.34e-6        EDGE_BAND      1.2e-5
    arctangent (degrees)                      0.00956        ATAN_BAND      0.01 (the polynomial's bound)

An orientation peak is undecided when a change of the smoothed histogram within its uncertainty
(Orientation.uncertainty: samples within ATAN_BAND of a bin boundary, HIST_QUANTUM per sample for
the oracle's fixed-point sums, HIST_RELATIVE of the maximum for float32) could turn its 0.8 max test
or a strict-maximum test; an orientation's angles are compared tightly when that change moves no
peak by ANGLE_DECIDED either.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import sift_f64_ref as ref

ROWS, COLS = 96, 144
# (n_octave_layers, upsample)
PARAM_SETS = ((3, 1), (2, 0), (4, 1))
SIGMA, CONTRAST, EDGE = 1.6, 0.04, 10.0
CENSUS_MIN = 3

OFFSET_BAND = 6e-5           # 8 x 7.5e-6 px
CONTRAST_BAND = 1.3e-6       # 8 x 1.6e-7 rounded up, relative
EDGE_BAND = 1.2e-5           # 8 x 1.4e-6 rounded up, of the squared size of the Hessian
ATAN_BAND = 0.01             # degrees
HIST_QUANTUM = 2.0 ** -11    # per sample
HIST_RELATIVE = 1e-6         # per bin, of the maximum
ANGLE_DECIDED = 0.125        # degrees


def _u8(acc, base=110.0):
    return np.clip(np.rint(base + acc), 0, 255).astype(np.uint8)


def _blob(acc, y, x, s1, s2, theta, amp):
    """A Gaussian blob of sigmas s1, s2 along axes turned by theta.  Blobs are elongated a little:
    a round one has a flat orientation histogram, whose peaks no arithmetic decides."""
    ys, xs = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    u = (xs - x) * math.cos(theta) + (ys - y) * math.sin(theta)
    v = -(xs - x) * math.sin(theta) + (ys - y) * math.cos(theta)
    acc += amp * np.exp(-(u * u / (2 * s1 * s1) + v * v / (2 * s2 * s2)))


def _sides(seed):
    """3 to 5 blobs of sigma 1.2 .. 4.7, centred 5 .. 8 px from a side."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((ROWS, COLS))
    for _ in range(rng.integers(3, 6)):
        side, d, t = rng.integers(0, 4), 5 + 3 * rng.random(), rng.random()
        y, x = [(d, 15 + t * (COLS - 30)), (ROWS - 1 - d, 15 + t * (COLS - 30)),
                (15 + t * (ROWS - 30), d), (15 + t * (ROWS - 30), COLS - 1 - d)][side]
        s = 1.2 + 3.5 * rng.random()
        _blob(acc, y, x, s, s * (1.25 + 0.5 * rng.random()), rng.random() * math.pi,
              (80 + 40 * rng.random()) * rng.choice([-1, 1]))
    return _u8(acc)


def _corners(seed):
    """One blob 5 .. 8 px from both sides of each corner."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((ROWS, COLS))
    for cy, cx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        d1, d2, s = 5 + 3 * rng.random(), 5 + 3 * rng.random(), 1.2 + 3 * rng.random()
        _blob(acc, d1 if cy == 0 else ROWS - 1 - d1, d2 if cx == 0 else COLS - 1 - d2, s, s * (1.25 + 0.5 * rng.random()),
              rng.random() * math.pi, (80 + 40 * rng.random()) * rng.choice([-1, 1]))
    return _u8(acc)


def _large(seed):
    """One blob of sigma 19 .. 26 px: detected in the last octave that has an interior."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((ROWS, COLS))
    s = 19 + 7 * rng.random()
    _blob(acc, 44 + 8 * rng.random(), 56 + 32 * rng.random(), s, s * (1.05 + 0.2 * rng.random()), rng.random() * math.pi,
          (100 + 50 * rng.random()) * rng.choice([-1, 1]))
    return _u8(acc, 128.0 if acc.sum() < 0 else 60.0)


def _patches(seed):
    """2 or 3 patches of 22 x 22 px, each a corner or junction of two edges 50 .. 130 degrees apart
    with different steps on its two wedges: several dominant gradient directions per keypoint."""
    rng = np.random.default_rng(seed)
    img = np.full((ROWS, COLS), 100.0)
    for _ in range(rng.integers(2, 4)):
        y0, x0, s = rng.integers(6, ROWS - 30), rng.integers(6, COLS - 30), 22
        py, px = np.mgrid[0:s, 0:s]
        a = rng.random() * math.pi
        b = a + math.radians(50 + 80 * rng.random())
        u = (px - s / 2) * math.cos(a) + (py - s / 2) * math.sin(a)
        v = (px - s / 2) * math.cos(b) + (py - s / 2) * math.sin(b)
        img[y0: y0 + s, x0: x0 + s] += ((u > 0) & (v > 0)) * (90 + 50 * rng.random()) + ((u < 0) & (v < 0)) * (40 * rng.random())
    img += rng.normal(0.0, 1.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _texture(seed):
    """The left image of a synthetic stereo pair with 28 px per texture cell."""
    from r7020e_visual_odometry_amd import synthetic as syn
    sd = syn.SEED_BASE + 100 + seed
    return syn.stereo_pair(sd, ROWS, COLS, planes=syn.random_scene(sd, ROWS, COLS, px_per_cell=28.0))[0]


# The seeds are the outcome of a search: of 300 .. 360 seeds per kind, the images kept are among
# those in which, at every parameter set, the reference finds no undecided candidate and no
# undecided orientation peak, chosen so that the census fills.
@functools.lru_cache(maxsize=None)
def images():
    """-> tuple of (name, image); an even count, so that they fill stereo frames."""
    out = [
        ("texture_a", _texture(353)), ("texture_b", _texture(334)),
        ("patches_a", _patches(285)), ("patches_b", _patches(3)),
        ("large_a", _large(0)), ("large_b", _large(1)), ("large_c", _large(7)),
        ("sides_a", _sides(103)), ("corners", _corners(69)),
        ("sides_b", _sides(247)), ("sides_c", _sides(2)), ("sides_d", _sides(260)),
    ]
    assert len(out) % 2 == 0 and all(im.shape == (ROWS, COLS) and im.dtype == np.uint8 for _, im in out)
    return tuple(out)


def sift_params(oracle, L, upsample, cap=16384):
    return oracle.SiftParams(L, SIGMA, CONTRAST, EDGE, upsample, cap)


class Analysis:
    """The reference's account of one image at one parameter set."""

    def __init__(self, img, L, upsample):
        import oracle
        p = sift_params(oracle, L, upsample)
        self.L, self.upsample = L, upsample
        self.G, self.D = ref.planes(oracle.pyramid(img, p), img.shape[0], img.shape[1], L, bool(upsample))
        self.cand = ref.candidates(self.D, L, CONTRAST)
        self.refined = [ref.refine(self.D[o], L, l, r, c, SIGMA, CONTRAST, EDGE) if full else None
                        for o, l, r, c, full in self.cand]
        self.ori = [ref.orientations(self.G[self.cand[i][0]][q.layer], q.r, q.c, q.scale)
                    if q is not None and q.outcome == "accepted" else None for i, q in enumerate(self.refined)]
        # the last octave a keypoint can lie in: planes of at most 2 * BORDER rows or columns have no interior
        self.last_octave = max(o for o, d in enumerate(self.D) if min(d.shape[1:]) > 2 * ref.BORDER)

    def outcome_codes(self):
        return np.array([ref.OUTCOMES.index(q.outcome) if q is not None else ref.OUTCOMES.index("outer")
                         for q in self.refined], np.int64)

    def counts(self):
        codes = self.outcome_codes()
        return len(codes), int((codes == 0).sum())

    def undecided_candidates(self):
        """Indices of the candidates with a decision inside its band."""
        return [i for i, q in enumerate(self.refined) if q is not None and
                (q.offset_margin < OFFSET_BAND or q.contrast_margin < CONTRAST_BAND or q.edge_margin < EDGE_BAND)]

    def orientation_uncertainty(self, i):
        return self.ori[i].uncertainty(ATAN_BAND, HIST_QUANTUM, HIST_RELATIVE)

    def undecided_peaks(self):
        """Indices of the accepted candidates with an undecided orientation peak: a 0.8 max test or
        a strict-maximum test that a change within the histogram's uncertainty could turn."""
        return [i for i, h in enumerate(self.ori) if h is not None and h.undecided(self.orientation_uncertainty(i))]

    def undecided_orientations(self):
        """Indices of the accepted candidates whose peak set, or a peak angle by more than
        ANGLE_DECIDED, could change within the histogram's uncertainty: the others' angles are
        compared with the oracle's."""
        out = []
        for i, h in enumerate(self.ori):
            if h is not None:
                u = self.orientation_uncertainty(i)
                if h.undecided(u) or h.angle_bound(u) > ANGLE_DECIDED:
                    out.append(i)
        return out

    def oct_scale(self, o):
        """(pixels of the image per sample of octave o, offset of the 1-based Location)."""
        return ((2.0 ** o) * 0.5, 0.75) if self.upsample else (2.0 ** o, 1.0)


@functools.lru_cache(maxsize=None)
def analyse(index: int, L: int, upsample: int) -> Analysis:
    return Analysis(images()[index][1], L, upsample)


CENSUS_CLASSES = (
    "refine: converged without moving", "refine: converged after an r/c move", "refine: converged after a layer move",
    "refine: left the domain by border", "refine: left the domain by layer", "refine: no convergence in 5 steps",
    "refine: contrast reject", "refine: edge reject",
    "refine: start on r = 5", "refine: start on r = R-6", "refine: start on c = 5", "refine: start on c = C-6",
    "orientation: clipped top", "orientation: clipped bottom", "orientation: clipped left", "orientation: clipped right",
    "orientation: exactly 2 peaks", "orientation: >= 3 peaks", "orientation: peak at bin 0 or 35",
    "descriptor: clipped top", "descriptor: clipped bottom", "descriptor: clipped left", "descriptor: clipped right",
    "descriptor: radius at the hypot cap", "descriptor: keypoint in the last octave",
)


def census_of(a: Analysis, decided_only: bool = False) -> dict:
    """Members of every class; with decided_only the orientation and descriptor classes count only
    the keypoints whose orientation is decided."""
    n = dict.fromkeys(CENSUS_CLASSES, 0)
    skip = set(a.undecided_orientations()) if decided_only else set()
    for i, q in enumerate(a.refined):
        if q is None:
            continue
        o, _, r, c, _ = a.cand[i]
        R, C = a.D[o].shape[1:]
        n["refine: start on r = 5"] += r == ref.BORDER
        n["refine: start on r = R-6"] += r == R - ref.BORDER - 1
        n["refine: start on c = 5"] += c == ref.BORDER
        n["refine: start on c = C-6"] += c == C - ref.BORDER - 1
        if q.outcome == "accepted":
            n["refine: converged without moving"] += q.moves == 0
            n["refine: converged after an r/c move"] += q.moved_rc
            n["refine: converged after a layer move"] += q.moved_layer
        n["refine: left the domain by border"] += q.outcome == "left_domain" and q.left_by == "border"
        n["refine: left the domain by layer"] += q.outcome == "left_domain" and q.left_by == "layer"
        n["refine: no convergence in 5 steps"] += q.outcome == "no_convergence"
        n["refine: contrast reject"] += q.outcome == "contrast"
        n["refine: edge reject"] += q.outcome == "edge"
        h = a.ori[i]
        if h is None or i in skip:
            continue
        for s in ref.SIDES:
            n[f"orientation: clipped {s}"] += h.clipped[s]
        n["orientation: exactly 2 peaks"] += len(h.angles) == 2
        n["orientation: >= 3 peaks"] += len(h.angles) >= 3
        n["orientation: peak at bin 0 or 35"] += any(b in (0, ref.ORI_BINS - 1) for b in h.peak_bins)
        if not h.angles:
            continue
        w = ref.descriptor_window(a.G[o][q.layer].shape, q.x, q.y, q.scale)
        for s in ref.SIDES:
            n[f"descriptor: clipped {s}"] += w.clipped[s]
        n["descriptor: radius at the hypot cap"] += w.at_cap
        n["descriptor: keypoint in the last octave"] += o == a.last_octave
    return {k: int(v) for k, v in n.items()}


@functools.lru_cache(maxsize=None)
def census(L: int, upsample: int, decided_only: bool = False) -> dict:
    tot = dict.fromkeys(CENSUS_CLASSES, 0)
    for i in range(len(images())):
        for k, v in census_of(analyse(i, L, upsample), decided_only).items():
            tot[k] += v
    return tot


def census_total(decided_only: bool = False) -> dict:
    tot = dict.fromkeys(CENSUS_CLASSES, 0)
    for L, up in PARAM_SETS:
        for k, v in census(L, up, decided_only).items():
            tot[k] += v
    return tot
