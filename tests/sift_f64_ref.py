"""An independent float64 restatement of SIFT's stages after the scale space: extremum scan,
sub-pixel refinement, orientation assignment and the descriptor.  Test infrastructure.

Written from the published algorithm -- Lowe, "Distinctive Image Features from Scale-Invariant
Keypoints" (IJCV 2004), sections 3.1, 4, 4.1, 5 and 6, with OpenCV's constants as DESIGN.md §3.1
lists them -- in plain numpy and `math`: float64 throughout, libm `atan2`, `exp`, `hypot`, true
sums.  It shares no code, header or expression order with oracle/sift_ref.c or include/vo_spec.h
and calls nothing through ctypes.  Its input is the Gaussian and difference-of-Gaussian planes of
one image (`planes(oracle.pyramid(...))`), which tests/test_oracle_kat.py holds to a float64
convolution level by level.

Every decision the algorithm takes on a computed number is returned with its *margin*, the
distance of that number from the value at which the decision flips, so that a caller can tell a
decided case from one that float32 rounding may turn either way.

Coordinates: (r, c) = (row, column) of an octave's plane; layers are the DoG levels 1..L.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

BORDER = 5                    # no extremum within 5 samples of a plane's side
MAX_STEPS = 5                 # Newton steps of the refinement
ORI_BINS = 36
ORI_SIGMA = 1.5               # orientation window sigma, in units of the keypoint's scale
ORI_RADIUS = 3.0 * ORI_SIGMA
ORI_PEAK_RATIO = 0.8
DESC_WIDTH = 4                # 4 x 4 spatial bins
DESC_BINS = 8                 # 8 orientation bins each
DESC_SCALE = 3.0              # a spatial bin is 3 * scale samples wide
DESC_CLIP = 0.2
DESC_FACTOR = 512.0
DESC_RADIUS_CAP = 127         # the window radius never exceeds 127

OUTCOMES = ("accepted", "left_domain", "no_convergence", "contrast", "edge", "overflow", "outer")
SIDES = ("top", "bottom", "left", "right")


def planes(flat: np.ndarray, rows: int, cols: int, L: int, upsample: bool):
    """Split oracle.pyramid's flat array -> (G, D): per octave a float64 array [L + 3, R, C] of
    Gaussian levels and one [L + 2, R, C] of their differences (DESIGN.md §4's arena order)."""
    r, c = (2 * rows, 2 * cols) if upsample else (rows, cols)
    G, D, off, o = [], [], 0, 0
    while off < flat.size:
        if o:
            r, c = r // 2, c // 2
        n = r * c
        G.append(flat[off: off + (L + 3) * n].reshape(L + 3, r, c).astype(np.float64))
        off += (L + 3) * n
        D.append(flat[off: off + (L + 2) * n].reshape(L + 2, r, c).astype(np.float64))
        off += (L + 2) * n
        o += 1
    assert off == flat.size
    return G, D


# ---------------------------------------------------------------------------------------------
# extremum scan
# ---------------------------------------------------------------------------------------------
def _block_extremum(level: np.ndarray, val: np.ndarray) -> np.ndarray:
    """For every interior sample: is val the largest (val > 0) or smallest (val < 0) of the 3 x 3
    block of `level` around it, ties allowed?  Arrays are the interior [1:-1, 1:-1]."""
    R, C = level.shape
    hi = np.full((R - 2, C - 2), -np.inf)
    lo = np.full((R - 2, C - 2), np.inf)
    for dy in range(3):
        for dx in range(3):
            s = level[dy: R - 2 + dy, dx: C - 2 + dx]
            hi = np.maximum(hi, s)
            lo = np.minimum(lo, s)
    return np.where(val > 0, val >= hi, val <= lo)


def candidates(D, L: int, contrast_threshold: float):
    """The extremum candidates in scan order (octave, layer, r, c).  Lowe §3.1: a DoG sample
    larger or smaller than its 26 neighbours, after the pre-threshold |D| > floor(0.5 * t / L * 255).
    -> int array [n, 5]: octave, layer, r, c, full.  A row is listed when the sample is an extremum
    against the neighbours that lie in the layers 1..L (the candidate count include/vo.h documents
    for vo_fetch_candidate_counts); full = 1 when it also is against DoG level 0 or L + 1, i.e. it
    passes the whole 26-neighbour test.  Values are float32 numbers compared exactly, so this stage
    has no margin."""
    thr = math.floor(0.5 * contrast_threshold / L * 255.0)
    out = []
    for o, d in enumerate(D):
        R, C = d.shape[1:]
        if R <= 2 * BORDER or C <= 2 * BORDER:
            continue
        for layer in range(1, L + 1):
            val = d[layer][1:-1, 1:-1]
            ok = np.abs(val) > thr
            full = np.ones_like(ok)
            for nb in (layer - 1, layer, layer + 1):
                e = _block_extremum(d[nb], val)
                if 1 <= nb <= L:
                    ok &= e
                else:
                    full &= e
            inner = np.zeros_like(ok)
            b = BORDER - 1
            inner[b: ok.shape[0] - b, b: ok.shape[1] - b] = True
            rc = np.argwhere(ok & inner)
            for r, c in rc:
                out.append((o, layer, r + 1, c + 1, int(full[r, c])))
    return np.array(out, np.int64).reshape(-1, 5)


# ---------------------------------------------------------------------------------------------
# refinement
# ---------------------------------------------------------------------------------------------
@dataclass
class Refined:
    outcome: str
    moves: int = 0                    # Newton steps that moved the integer sample
    moved_rc: bool = False
    moved_layer: bool = False
    left_by: str = ""                 # left_domain: "border" or "layer"
    r: int = 0                        # the integer sample the outcome was decided at
    c: int = 0
    layer: int = 0
    x: float = 0.0                    # accepted: refined column / row in the octave, scale in octave
    y: float = 0.0                    # samples (sigma 2^((layer + offset) / L)), |contrast|
    scale: float = 0.0
    response: float = 0.0
    largest_offset: float = 0.0       # max |offset| of the last step
    offset_margin: float = math.inf   # min over steps and axes of ||offset| - nearest k + 0.5| (see refine)
    contrast_margin: float = math.inf  # (|contrast| L - t) / t
    edge_margin: float = math.inf     # min |edge_terms|: det from 0 and tr^2 e from (e + 1)^2 det, relative


def _derivatives(d, layer, r, c):
    """Gradient and Hessian of D(x, y, s) by central differences, image values scaled to [0, 1]."""
    q = d[layer - 1: layer + 2, r - 1: r + 2, c - 1: c + 2] / 255.0        # [s, y, x]
    g = np.array([q[1, 1, 2] - q[1, 1, 0], q[1, 2, 1] - q[1, 0, 1], q[2, 1, 1] - q[0, 1, 1]]) / 2.0
    v = q[1, 1, 1]
    dxx = q[1, 1, 2] + q[1, 1, 0] - 2.0 * v
    dyy = q[1, 2, 1] + q[1, 0, 1] - 2.0 * v
    dss = q[2, 1, 1] + q[0, 1, 1] - 2.0 * v
    dxy = (q[1, 2, 2] - q[1, 2, 0] - q[1, 0, 2] + q[1, 0, 0]) / 4.0
    dxs = (q[2, 1, 2] - q[2, 1, 0] - q[0, 1, 2] + q[0, 1, 0]) / 4.0
    dys = (q[2, 2, 1] - q[2, 0, 1] - q[0, 2, 1] + q[0, 0, 1]) / 4.0
    H = np.array([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]])
    return v, g, H


def edge_terms(dxx, dyy, dxy, e):
    """The two numbers the edge test decides on, each relative to the size of the 2 x 2 Hessian
    they are quadratic forms of: det / size and (tr^2 e - (e + 1)^2 det) / ((e + 1)^2 size), size =
    dxx^2 + dyy^2 + 2 dxy^2 (which, unlike |dxx dyy| + dxy^2, does not vanish along an edge, where
    one second derivative is a rounding residue).  Evaluated in the arguments' own precision (a
    test measures float32 against float64)."""
    size = dxx * dxx + dyy * dyy + (dxy * dxy + dxy * dxy)
    det = dxx * dyy - dxy * dxy
    tr = dxx + dyy
    if not size > 0:
        return size * 0, size * 0
    return det / size, (tr * tr * e - (e + 1) * (e + 1) * det) / ((e + 1) * (e + 1) * size)


def _half_margin(x: float) -> float:
    """Distance of |x| from the nearest k + 0.5: where `|x| < 0.5` or round(x) changes."""
    a = abs(x)
    return abs(a - (math.floor(a) + 0.5))


def refine(d, L: int, layer: int, r: int, c: int, sigma: float, contrast_threshold: float,
           edge_threshold: float) -> Refined:
    """Lowe §4 and §4.1 on one candidate of an octave's DoG stack d [L + 2, R, C]: Newton steps
    offset = -H^-1 g until every |offset| < 0.5, moving the sample by round(offset) otherwise (at
    most 5 steps, inside the border and the layers 1..L); then |D(offset)| L >= t and the ratio of
    principal curvatures tr^2 / det < (e + 1)^2 / e."""
    R, C = d.shape[1:]
    out = Refined("accepted")
    off = np.zeros(3)
    for step in range(MAX_STEPS + 1):
        if step == MAX_STEPS:
            out.outcome = "no_convergence"
            break
        _, g, H = _derivatives(d, layer, r, c)
        # a singular system takes a zero step
        try:
            off = -np.linalg.solve(H, g)
        except np.linalg.LinAlgError:
            off = np.zeros(3)
        out.largest_offset = float(np.abs(off).max())
        if np.all(np.abs(off) < 0.5):
            out.offset_margin = min(out.offset_margin, 0.5 - out.largest_offset)
            break
        if np.any(np.abs(off) > (2 ** 31 - 1) // 3):
            out.outcome = "overflow"
            break
        dc, dr, dl = (int(round(v)) for v in off)          # round half to even
        if (not 0 <= layer + dl <= L + 1 or not BORDER - 1 <= c + dc <= C - BORDER
                or not BORDER - 1 <= r + dr <= R - BORDER):
            # lands two or more samples outside: no rounding tie brings it back, only convergence would
            out.offset_margin = min(out.offset_margin, out.largest_offset - 0.5)
        else:
            out.offset_margin = min(out.offset_margin, min(_half_margin(v) for v in off))
        c, r, layer = c + dc, r + dr, layer + dl
        out.moves += 1
        out.moved_rc |= bool(dc or dr)
        out.moved_layer |= bool(dl)
        if layer < 1 or layer > L:
            out.outcome, out.left_by = "left_domain", "layer"
            break
        if c < BORDER or c >= C - BORDER or r < BORDER or r >= R - BORDER:
            out.outcome, out.left_by = "left_domain", "border"
            break
    out.r, out.c, out.layer = r, c, layer
    if out.outcome != "accepted":
        return out
    v, g, H = _derivatives(d, layer, r, c)
    contrast = v + 0.5 * float(g @ off)
    if contrast_threshold > 0:
        out.contrast_margin = abs(abs(contrast) * L - contrast_threshold) / contrast_threshold
    if abs(contrast) * L < contrast_threshold:
        out.outcome = "contrast"
        return out
    e = edge_threshold
    det_rel, ratio_rel = edge_terms(H[0, 0], H[1, 1], H[0, 1], e)
    out.edge_margin = min(abs(det_rel), abs(ratio_rel))
    tr = H[0, 0] + H[1, 1]
    det = H[0, 0] * H[1, 1] - H[0, 1] * H[0, 1]
    if det <= 0 or tr * tr * e >= (e + 1) ** 2 * det:
        out.outcome = "edge"
        return out
    out.x, out.y = c + off[0], r + off[1]
    out.scale = sigma * 2.0 ** ((layer + off[2]) / L)
    out.response = abs(contrast)
    return out


# ---------------------------------------------------------------------------------------------
# orientation
# ---------------------------------------------------------------------------------------------
def _window(g, r, c, radius):
    """Samples (i, j) of the square window of `radius` around (r, c) whose central differences
    exist (not on the plane's outermost ring) -> (i, j, dx, dy, clipped sides)."""
    R, C = g.shape
    y0, y1 = max(r - radius, 1), min(r + radius, R - 2)
    x0, x1 = max(c - radius, 1), min(c + radius, C - 2)
    clipped = {"top": r - radius < 1, "bottom": r + radius > R - 2, "left": c - radius < 1, "right": c + radius > C - 2}
    if y1 < y0 or x1 < x0:
        z = np.zeros(0)
        return z, z, z, z, clipped
    ys, xs = np.mgrid[y0: y1 + 1, x0: x1 + 1]
    dx = g[ys, xs + 1] - g[ys, xs - 1]
    dy = g[ys - 1, xs] - g[ys + 1, xs]                      # y up: angles counter-clockwise on screen
    return (ys - r).ravel(), (xs - c).ravel(), dx.ravel(), dy.ravel(), clipped


def _atan2_deg(dy, dx):
    a = np.degrees(np.arctan2(dy, dx))
    return np.where(a < 0, a + 360.0, a)


@dataclass
class Orientation:
    hist: np.ndarray                  # the smoothed 36-bin histogram
    angles: list                      # peak angles in degrees [0, 360), ascending bin
    peak_bins: list
    threshold_margin: np.ndarray      # per bin  hist - 0.8 max
    maximum_margin: np.ndarray        # per bin  min(hist - left, hist - right)
    clipped: dict
    radius: int
    bin_count: np.ndarray             # samples per raw bin
    sample_mass: np.ndarray           # per sample: weight x gradient magnitude
    sample_edge: np.ndarray           # per sample: degrees from its angle to the nearest bin boundary

    def uncertainty(self, angle_band: float, quantum: float, relative: float) -> float:
        """A bound on what any smoothed bin can move by when (1) every sample within `angle_band`
        degrees of a bin boundary may fall into the neighbouring bin -- moving a mass m between
        adjacent raw bins moves a smoothed bin by at most 3/16 m, the largest step of
        [1 4 6 4 1] / 16 -- (2) every sample's contribution is off by `quantum` and (3) every bin by
        `relative` of the maximum."""
        flip = 3.0 / 16.0 * float(self.sample_mass[self.sample_edge < angle_band].sum())
        n = self.bin_count.astype(np.float64)
        smooth = (6.0 * n + 4.0 * (np.roll(n, 1) + np.roll(n, -1)) + np.roll(n, 2) + np.roll(n, -2)) / 16.0
        return flip + quantum * float(smooth.max()) + relative * float(self.hist.max())

    def undecided(self, u: float) -> bool:
        """Whether some bin's peak status hangs on a comparison that a change of u in every bin
        could turn (2 u, 1.8 u for the 0.8 max test), while the bin's other comparison holds or could."""
        t, m = self.threshold_margin, self.maximum_margin
        return bool(np.any(((np.abs(t) <= 1.8 * u) & (m > -2 * u)) | ((np.abs(m) <= 2 * u) & (t > -1.8 * u))))

    def angle_bound(self, u: float) -> float:
        """A bound, in degrees, on how far a change of u in every bin moves a peak's parabola vertex:
        with p = (l - r) / (2 den), den = l - 2 c + r and |l - r| <= |den| at a maximum,
        |dp| <= u / |den| + |l - r| 4 u / (2 den^2) <= 3 u / (|den| - 4 u)."""
        worst = 0.0
        for k in self.peak_bins:
            den = abs(self.hist[k - 1] - 2.0 * self.hist[k] + self.hist[(k + 1) % ORI_BINS])
            worst = max(worst, math.inf if den <= 4 * u else 360.0 / ORI_BINS * 3.0 * u / (den - 4 * u))
        return worst


def orientations(g, r: int, c: int, scale: float, atan2_deg=_atan2_deg) -> Orientation:
    """Lowe §5 at sample (r, c) of the Gaussian level g: gradient magnitudes of a window of radius
    round(4.5 scale), weighted by a Gaussian of sigma 1.5 scale, into 36 bins of 10 degrees; the
    histogram smoothed circularly by [1 4 6 4 1] / 16; every local maximum within 80 % of the
    largest is a peak, placed by the parabola through it and its two neighbours.  The angle is
    reported as 360 - 10 bin (clockwise on screen).  `atan2_deg` lets a test measure what another
    arctangent does to the histogram; the reference's own is libm's."""
    radius = int(round(ORI_RADIUS * scale))
    i, j, dx, dy, clipped = _window(g, r, c, radius)
    sw = ORI_SIGMA * scale
    w = np.exp(-(i * i + j * j) / (2.0 * sw * sw))
    mag = np.hypot(dx, dy)
    pos = atan2_deg(dy, dx) * (ORI_BINS / 360.0)           # in bins
    b = np.rint(pos).astype(np.int64) % ORI_BINS
    edge = np.abs(pos - np.floor(pos) - 0.5) * (360.0 / ORI_BINS)
    raw = np.bincount(b, weights=w * mag, minlength=ORI_BINS)
    h = (6.0 * raw + 4.0 * (np.roll(raw, 1) + np.roll(raw, -1)) + np.roll(raw, 2) + np.roll(raw, -2)) / 16.0
    top = h.max()
    left, right = np.roll(h, 1), np.roll(h, -1)
    tm = h - ORI_PEAK_RATIO * top
    mm = np.minimum(h - left, h - right)
    angles, bins = [], []
    for k in range(ORI_BINS):
        if h[k] > left[k] and h[k] > right[k] and h[k] >= ORI_PEAK_RATIO * top:
            pos = k + 0.5 * (left[k] - right[k]) / (left[k] - 2.0 * h[k] + right[k])
            pos %= ORI_BINS
            angles.append((360.0 - 360.0 / ORI_BINS * pos) % 360.0)
            bins.append(k)
    return Orientation(h, angles, bins, tm, mm, clipped, radius, np.bincount(b, minlength=ORI_BINS), w * mag, edge)


# ---------------------------------------------------------------------------------------------
# descriptor
# ---------------------------------------------------------------------------------------------
@dataclass
class Descriptor:
    values: np.ndarray                # the 128 values before rounding to u8 (not saturated)
    clipped: dict
    radius: int
    at_cap: bool                      # the radius was cut to floor(hypot(rows, cols))
    samples: int                      # samples that contributed


@dataclass
class DescriptorWindow:
    pr: int
    pc: int
    radius: int
    at_cap: bool
    clipped: dict


def descriptor_window(shape, x: float, y: float, scale: float) -> DescriptorWindow:
    """The square sample window of descriptor(): centre round(y), round(x), radius
    round(3 scale sqrt(2) (4 + 1) / 2) cut to floor(hypot(rows, cols)) and to 127."""
    R, C = shape
    pc, pr = int(round(x)), int(round(y))                  # round half to even
    radius = int(round(DESC_SCALE * scale * math.sqrt(2.0) * (DESC_WIDTH + 1) * 0.5))
    cap = int(math.hypot(R, C))
    at_cap = radius > cap
    radius = min(radius, cap, DESC_RADIUS_CAP)
    clipped = {"top": pr - radius < 1, "bottom": pr + radius > R - 2, "left": pc - radius < 1, "right": pc + radius > C - 2}
    return DescriptorWindow(pr, pc, radius, at_cap, clipped)


def descriptor(g, x: float, y: float, angle: float, scale: float) -> Descriptor:
    """Lowe §6 at (x, y) = (column, row) of the Gaussian level g for a keypoint of orientation
    `angle` (degrees, as orientations() reports it) and octave-relative `scale`: a 4 x 4 grid of
    cells 3 scale wide, turned with the keypoint, centred on round(x), round(y); each sample's
    gradient magnitude, weighted by a Gaussian of sigma 2 cells, is split trilinearly between the
    neighbouring cells and the 8 orientation bins; the 128-vector is normalised, clipped at 0.2,
    normalised again and scaled by 512."""
    d, n = DESC_WIDTH, DESC_BINS
    ori = (360.0 - angle) % 360.0
    win = descriptor_window(g.shape, x, y, scale)
    pr, pc, radius, at_cap = win.pr, win.pc, win.radius, win.at_cap
    cell = DESC_SCALE * scale
    i, j, dx, dy, clipped = _window(g, pr, pc, radius)
    ct, st = math.cos(math.radians(ori)) / cell, math.sin(math.radians(ori)) / cell
    cr = j * ct - i * st                                    # rotated position in cells
    rr = j * st + i * ct
    rb = rr + d / 2 - 0.5                                   # cell coordinates: centres at 0..3
    cb = cr + d / 2 - 0.5
    keep = (rb > -1) & (rb < d) & (cb > -1) & (cb < d)
    rb, cb, cr, rr, dx, dy = rb[keep], cb[keep], cr[keep], rr[keep], dx[keep], dy[keep]
    w = np.exp(-(cr * cr + rr * rr) / (0.5 * d * d))
    mag = np.hypot(dx, dy) * w
    ob = (_atan2_deg(dy, dx) - ori) * (n / 360.0)
    r0, c0, o0 = np.floor(rb), np.floor(cb), np.floor(ob)
    fr, fc, fo = rb - r0, cb - c0, ob - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
    H = np.zeros((d, d, n))
    for ar in (0, 1):
        wr = fr if ar else 1.0 - fr
        for ac in (0, 1):
            wc = fc if ac else 1.0 - fc
            for ao in (0, 1):
                wo = fo if ao else 1.0 - fo
                ri, ci, oi = r0 + ar, c0 + ac, (o0 + ao) % n
                inside = (ri >= 0) & (ri < d) & (ci >= 0) & (ci < d)
                np.add.at(H, (ri[inside], ci[inside], oi[inside]), (mag * wr * wc * wo)[inside])
    v = H.ravel()
    norm = math.sqrt(float(v @ v))
    v = np.minimum(v, DESC_CLIP * norm)
    norm = math.sqrt(float(v @ v))
    v = v * (DESC_FACTOR / max(norm, 2.0 ** -23))
    return Descriptor(v, clipped, radius, at_cap, int(keep.sum()))


def to_u8(values: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(values), 0, 255).astype(np.uint8)
