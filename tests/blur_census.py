"""A census of the scale-space launches: for a batched call (rows, cols, frames, SIFT parameters)
every launch sift_enqueue_pyramid makes, in order, with the plan csrc/blur_plan.h gives it, and
the classes of that launch that a test of the streaming blur has to have seen (CLASS_TABLE).

Each plan comes from libblur_plan.so (oracle/blur_plan_eval.cpp compiles the header itself), the
octave count and the kernel radii from the oracle (oracle_num_octaves, oracle_gauss_radius).  What
is transcribed here is the dispatch around the plans -- sift.hip's small_plan and
sift_enqueue_pyramid -- and tests/test_gpu_blur_bands.py holds that transcription to the library
by the launch counts of a profiled call.

Planes per call: vo_api.hip's enqueue_sift_stereo splits the B frames of a call into parts =
min(n_sub, B) (vo_set_concurrency, 1 unless set) and passes 2 * nf planes of each part to
sift_enqueue_pyramid, nf = B (p + 1) / parts - B p / parts.  The two carry slots are part of the
arena (build_pyramid_geometry gets 2 * max_batch + 2 images, in each of the two buffer sets) but of
no launch: planes_per_call().

Everything is written over grids: rows and cols may be 1-D arrays, every quantity of a launch is
then an array over rows x cols, which is how reachable_classes() walks the whole search domain.
census() is the same code at one point."""
import ctypes as C
import math
from pathlib import Path

import numpy as np

LEVEL, BASE_FLOAT, BASE_U8 = 0, 1, 2
FIELDS = ("streamed", "cpl", "tag", "th", "n_bands", "n_strips", "full_bands")
BS_P = 4
STAGE_ROUND_DWORDS = 64 * 16        # blur_stream_body's staging loop: 64 lanes x SCH = 16 loads per round
SMALL_PX = 9216                     # sift.hip VO_SMALL_PX
KINDS = ("BaseU8", "BaseFloat-DPP", "BaseFloat-LDS", "Level2", "Level4-DPP", "Level4-LDS")
DPP_KINDS = ("BaseU8", "BaseFloat-DPP", "Level4-DPP")
BASE_KINDS = KINDS[:3]
SITES = ("k_blur_base", "k_blur_fused", "k_down", "k_base_src<true>", "k_base_src<false>", "k_blur_small")
REFUSALS = ("untabled radius", "plane shorter than one band", "rows <= radius + 6", "u8 base under 64 rows")

# The search domain of the issue, and the arena a case may take
MAX_ROWS, MAX_COLS, MIN_SIDE = 260, 1600, 16
FRAMES = (2, 8, 32, 64, 128, 256, 512)
ARENA_CAP = 4 << 30
DEFAULT_SIFT = (3, 1.6)

# The classes, per kind of streamed launch unless a row says otherwise.  (name, values, scope)
CLASS_TABLE = (
    ("bucket", ("4", "8-32", "mid", "cap"), "band height: 4, 8..32, 36..cap-4, cap (96 base, 128 levels); per kind"),
    ("bands", ("1", "2", "3+"), "bands per plane; per kind and bucket above 4"),
    ("last", ("whole", "cut4", "cut-odd"), "last band whole, cut to a multiple of 4 rows, cut with R % 4 != 0; per kind and bucket above 4"),
    ("strips", ("1", "2", "3+"), "strips of the grid; per kind"),
    ("blocks", ("even", "odd"), "(F + THb) / P of the first or the last band; per DPP kind"),
    ("nextbase", ("ee", "eo", "oe", "oo"), "next octave's rows, columns even/odd where level L stores it above bucket 4; per level kind"),
    ("rounds", ("1", "2", "3"), "staging rounds of a band of the u8 base"),
    ("fold", ("top", "bottom", "both", "neither"), "a band of the u8 base at 2 or more rounds folding at the top, the bottom, both, neither"),
    ("misaligned", ("1", "2", "3"), "source pointer modulo 4, u8 base at 2 or more rounds"),
    ("unstreamed", ("base", "level"), "at 128 planes or more, a tabled radius the plan does not stream"),
)


def load_plan_lib(oracle):
    lib = C.CDLL(str(Path(oracle.__file__).resolve().parent / "build" / "libblur_plan.so"))
    P = C.POINTER(C.c_int)
    lib.blur_plan_sweep.argtypes = [C.c_int, C.c_int, C.c_int, P, C.c_int, P, C.c_int, P]
    lib.blur_plan_sweep.restype = None
    lib.blur_plan_u8_stage_rows.argtypes = [C.c_int] * 5 + [P]
    lib.blur_plan_u8_stage_rows.restype = None
    assert lib.blur_plan_bs_p() == BS_P
    return lib


def header_plan(lib, role, r, n_img, rows, cols):
    """blur_plan(role, rows[i], cols[j], n_img, r) -> {field: [len(rows), len(cols)] int32}"""
    R, Cc = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(cols, np.int32)
    out = np.full((len(FIELDS), len(R), len(Cc)), -1, np.int32)
    P = C.POINTER(C.c_int)
    lib.blur_plan_sweep(role, r, n_img, R.ctypes.data_as(P), len(R), Cc.ctypes.data_as(P), len(Cc), out.ctypes.data_as(P))
    return dict(zip(FIELDS, out))


def small_octave(dims, maxr=13):
    """small_plan of sift.hip: the first octave from which all fit k_small_pyr's LDS.  dims: (rows,
    cols) per octave, ints or arrays that broadcast against each other."""
    o_small = np.int64(len(dims)) + 0 * dims[0][0] * dims[0][1]
    alive = o_small == len(dims)
    for o in range(len(dims) - 1, 0, -1):
        px = [r * c for r, c in dims[o:]]
        mx = np.maximum.reduce(px)
        cap = (mx + 3) & ~3
        bcap = (np.maximum.reduce(px[1:]) + 3) & ~3 if len(px) > 1 else 0
        rt = np.maximum.reduce([r for r, _ in dims[o:]]) + 2 * maxr
        ct = np.maximum.reduce([c for _, c in dims[o:]]) + 2 * maxr
        lds = 4 * (3 * cap + bcap) + 4 * (rt + ct)
        alive = alive & ~((mx > SMALL_PX) | (lds > 160 * 1024))
        o_small = np.where(alive, o, o_small)
    return int(o_small) if np.ndim(o_small) == 0 else o_small


def fork_octave(dims, full_bands):
    """sift_enqueue_pyramid: octave 1, moved down past every octave still at full bands."""
    o_small = small_octave(dims)
    o_fork = min(1, o_small - 1)
    while o_fork + 1 < o_small and full_bands(*dims[o_fork + 1]):
        o_fork += 1
    return o_fork


def planes_per_call(frames, n_sub=1):
    """planes of each sift_enqueue_pyramid of a call of `frames` frames (see the module docstring)"""
    parts = min(n_sub, frames)
    return [2 * (frames * (p + 1) // parts - frames * p // parts) for p in range(parts)]


def radii(oracle, L=3, sigma=1.6, upsample=1):
    """kernel radii of the base blur and of levels 1..L+2: vo_spec.h's sigmas through the oracle's
    kernel-size function"""
    init = 1.0 if upsample else 0.5
    sig = [math.sqrt(max(sigma * sigma - init * init, 0.01))]
    for i in range(1, L + 3):
        prev = math.exp((i - 1) * math.log(2.0) / L) * sigma
        tot = prev * math.exp(math.log(2.0) / L)
        sig.append(math.sqrt(tot * tot - prev * prev))
    return [oracle.lib().oracle_gauss_radius(s) for s in sig]


def _n_octaves(oracle, rows, cols, upsample):
    m = np.minimum(rows[:, None], cols[None, :])
    lut = {int(v): oracle.lib().oracle_num_octaves(int(v), int(v), upsample) for v in np.unique(m)}
    return np.vectorize(lut.get, otypes=[np.int64])(m)


_tabled_cache = {}


def _tabled(lib, r):
    """whether radius r has compiled instantiations: the plan streams a tall plane of one image"""
    if r not in _tabled_cache:
        _tabled_cache[r] = bool(header_plan(lib, LEVEL, r, 1, [4096], [4096])["streamed"][0, 0])
    return _tabled_cache[r]


def arena_bytes(oracle, rows, cols, frames, upsample=1, L=3):
    """the scale-space arena of one buffer set of a context of max_batch = frames: the L + 3
    Gaussian planes of every octave of 2 * frames + 2 images (build_pyramid_geometry's py.total
    floats; the context holds two such sets): [len(rows), len(cols)] bytes"""
    rows, cols = np.atleast_1d(rows).astype(np.int64), np.atleast_1d(cols).astype(np.int64)
    n_oct = _n_octaves(oracle, rows, cols, upsample)
    R, Cc = (rows * 2, cols * 2) if upsample else (rows, cols)
    floats = np.zeros(n_oct.shape, np.int64)
    for o in range(int(n_oct.max())):
        plane = (R >> o)[:, None] * (((Cc >> o) + 255) // 256 * 256)[None, :]
        floats += np.where(o < n_oct, (L + 3) * plane, 0)
    return (2 * frames + 2) * 4 * floats


_band_cache = {}


def u8_bands(lib, r, R, th):
    """the bands of a streamed BaseU8 launch of an R-row plane (source image R / 2 rows) at band
    height th: [(y0, THb, sr0, sr1, rounds, folds_top, folds_bottom)]"""
    key = (r, R, th)
    if key not in _band_cache:
        F = (2 * r + BS_P - 1) // BS_P * BS_P
        E = F - 2 * r
        swd = lib.blur_plan_bs_u8_dw(r, 4)
        out, o = [], (C.c_int * 2)()
        for b in range((R + th - 1) // th):
            y0 = b * th
            thb = min(th, (R - y0 + BS_P - 1) // BS_P * BS_P)
            lib.blur_plan_u8_stage_rows(r, R, R // 2, y0, thb, o)
            total = (o[1] - o[0] + 1) * swd
            p_lo = y0 - r - E
            out.append((y0, thb, o[0], o[1], -(-total // STAGE_ROUND_DWORDS), p_lo < 0, p_lo + F + thb - 1 >= R))
        _band_cache[key] = out
    return _band_cache[key]


_U8_BITS = ("rounds:1", "rounds:2", "rounds:3", "rounds:4+", "fold:top", "fold:bottom", "fold:both", "fold:neither")


def _u8_bits(lib, r, R, th):
    bits = 0
    for _, _, _, _, rounds, top, bot in u8_bands(lib, r, R, th):
        bits |= 1 << (min(rounds, 4) - 1)
        if rounds >= 2:
            bits |= 1 << (4 + (2 if top and bot else 0 if top else 1 if bot else 3))
    return bits


def walk(lib, oracle, rows, cols, n_img, upsample=1, sift=DEFAULT_SIFT):
    """The launches of one sift_enqueue_pyramid + sift_enqueue_small of n_img planes over the grid
    rows x cols, in order.  Each launch is a dict: site, octave, level, kind ("" unless streamed
    somewhere), r, and arrays over the grid -- mask (the launch is made), R, C, the plan's fields,
    and for a level L: nb (stores the next base), nbR, nbC."""
    rows, cols = np.atleast_1d(rows).astype(np.int64), np.atleast_1d(cols).astype(np.int64)
    L, sigma = sift
    krad = radii(oracle, L, sigma, upsample)
    n_oct = _n_octaves(oracle, rows, cols, upsample)
    R0, C0 = (rows * 2, cols * 2) if upsample else (rows, cols)
    dR, dC = [R0 >> o for o in range(int(n_oct.max()))], [C0 >> o for o in range(int(n_oct.max()))]
    o_small = np.zeros(n_oct.shape, np.int64)
    for n in np.unique(n_oct):
        d = [(dR[o][:, None], dC[o][None, :]) for o in range(int(n))]
        o_small = np.where(n_oct == n, small_octave(d, max(krad[1:])), o_small)
    shape = n_oct.shape
    out = []

    def add(site, o, level, mask, role=None, r=0, plan=None, **kw):
        e = {"site": site, "octave": o, "level": level, "mask": np.broadcast_to(mask, shape), "role": role, "r": r,
             "R": np.broadcast_to(dR[o][:, None], shape), "C": np.broadcast_to(dC[o][None, :], shape), "n_img": n_img}
        if plan is not None:
            e.update(plan)
            e["streamed"] = plan["streamed"].astype(bool)
            hl = bool(lib.blur_plan_bs_hl(r, 4, 0 if role == LEVEL else 1))
            e["kinds"] = {
                BASE_U8: ("BaseU8",), BASE_FLOAT: ("BaseFloat-DPP" if hl else "BaseFloat-LDS",),
                LEVEL: ("Level2", "Level4-DPP" if hl else "Level4-LDS")}[role]
            # which rule refused a launch that is not streamed, in blur_plan()'s order: a label for the
            # record only (the band height is restated for it); whether a launch streams is the plan's word
            cpl = np.where(e["C"] <= 1400, 2, 4) if role == LEVEL else 4
            th = np.maximum(BS_P, np.minimum(128 if role == LEVEL else 96, e["R"] * ((e["C"] + 64 * cpl - 1) // (64 * cpl)) * n_img // 2048)
                            // BS_P * BS_P)
            e["refused"] = np.where(e["streamed"], -1, 0 if not _tabled(lib, r) else np.where(
                e["R"] < th, 1, np.where(e["R"] <= r + BS_P + 2, 2, 3)))
        e.update(kw)
        out.append(e)
        return e

    base_done = np.zeros(shape, bool)
    for o in range(int(o_small.max())):
        large = o < o_small
        if o == 0:
            from_u8 = np.zeros(shape, bool)
            if upsample:
                pl = header_plan(lib, BASE_U8, krad[0], n_img, dR[0], dC[0])
                from_u8 = pl["streamed"].astype(bool)
                add("k_blur_base", 0, 0, large & from_u8, BASE_U8, krad[0], pl)
            add("k_base_src<true>" if upsample else "k_base_src<false>", 0, 0, large & ~from_u8)
            pl = header_plan(lib, BASE_FLOAT, krad[0], n_img, dR[0], dC[0])
            s = pl["streamed"].astype(bool)
            add("k_blur_base", 0, 0, large & ~from_u8 & s, BASE_FLOAT, krad[0], pl)
            add("k_blur_fused", 0, 0, large & ~from_u8 & ~s, BASE_FLOAT, krad[0], pl)
        else:
            add("k_down", o, 0, large & ~base_done)
        for i in range(1, L + 3):
            pl = header_plan(lib, LEVEL, krad[i], n_img, dR[o], dC[o])
            kw = {}
            if i == L:
                base_done = large & pl["streamed"].astype(bool) & (o + 1 < o_small)
                nR = dR[o + 1] if o + 1 < len(dR) else dR[o] // 2
                nC = dC[o + 1] if o + 1 < len(dC) else dC[o] // 2
                kw = {"nb": base_done, "nbR": np.broadcast_to(nR[:, None], shape), "nbC": np.broadcast_to(nC[None, :], shape)}
            add("k_blur_fused", o, i, large, LEVEL, krad[i], pl, **kw)
    out.append({"site": "k_blur_small", "octave": -1, "level": 0, "mask": o_small < n_oct, "role": None, "r": 0,
                "R": np.zeros(shape, np.int64), "C": np.zeros(shape, np.int64), "n_img": n_img})
    return out


def _bucket(th, cap):
    return np.where(th == 4, 0, np.where(th <= 32, 1, np.where(th < cap, 2, 3)))


def launch_classes(lib, e):
    """{class: bool grid} of one launch of walk(): the classes of CLASS_TABLE it is in"""
    out = {}
    if e.get("role") is None:
        return out
    m, R, Cc = e["mask"], e["R"], e["C"]
    if e["n_img"] >= 128 and _tabled(lib, e["r"]) and e["role"] != BASE_U8:
        out[("unstreamed", "base" if e["role"] == BASE_FLOAT else "level")] = m & ~e["streamed"]
    s = m & e["streamed"]
    if not s.any():
        return out
    th, nb, ns = np.maximum(e["th"], BS_P), e["n_bands"], e["n_strips"]
    cap = 96 if e["role"] != LEVEL else 128
    bucket = _bucket(th, cap)
    last = R - (nb - 1) * th                                          # rows of the last band
    thb_last = (last + BS_P - 1) // BS_P * BS_P
    for kind in e["kinds"]:
        k = s & (e["cpl"] == (2 if kind == "Level2" else 4))
        if not k.any():
            continue
        for b, name in enumerate(CLASS_TABLE[0][1]):
            kb = k & (bucket == b)
            out[("bucket", kind, name)] = kb
            if b:
                out[("bands", kind, name, "1")] = kb & (nb == 1)
                out[("bands", kind, name, "2")] = kb & (nb == 2)
                out[("bands", kind, name, "3+")] = kb & (nb >= 3)
                out[("last", kind, name, "whole")] = kb & (last == th)
                out[("last", kind, name, "cut4")] = kb & (last < th) & (R % 4 == 0)
                out[("last", kind, name, "cut-odd")] = kb & (last < th) & (R % 4 != 0)
        out[("strips", kind, "1")] = k & (ns == 1)
        out[("strips", kind, "2")] = k & (ns == 2)
        out[("strips", kind, "3+")] = k & (ns >= 3)
        if kind in DPP_KINDS:
            F = (2 * e["r"] + BS_P - 1) // BS_P * BS_P
            first = np.where(nb > 1, th, thb_last)
            for par, name in enumerate(CLASS_TABLE[4][1]):
                out[("blocks", kind, name)] = k & (((F + first) // BS_P % 2 == par) | ((F + thb_last) // BS_P % 2 == par))
        if "nb" in e:
            for pr in (0, 1):
                for pc in (0, 1):
                    out[("nextbase", kind, "eo"[pr] + "eo"[pc])] = k & e["nb"] & (bucket > 0) & (e["nbR"] % 2 == pr) & (e["nbC"] % 2 == pc)
    if e["role"] == BASE_U8:
        bits = np.zeros(s.shape, np.int64)
        keys, inv = np.unique((R * 1024 + th)[s], return_inverse=True)
        bits[s] = np.array([_u8_bits(lib, e["r"], int(k) >> 10, int(k) & 1023) for k in keys], np.int64)[inv]
        for i, name in enumerate(_U8_BITS):
            out[tuple(name.split(":"))] = s & ((bits >> i) & 1 == 1)
    return out


def all_classes():
    """every class of CLASS_TABLE, reachable or not"""
    out = set()
    for kind in KINDS:
        for b in CLASS_TABLE[0][1]:
            out.add(("bucket", kind, b))
            if b != "4":
                out |= {("bands", kind, b, v) for v in CLASS_TABLE[1][1]} | {("last", kind, b, v) for v in CLASS_TABLE[2][1]}
        out |= {("strips", kind, v) for v in CLASS_TABLE[3][1]}
        if kind in DPP_KINDS:
            out |= {("blocks", kind, v) for v in CLASS_TABLE[4][1]}
        if kind not in BASE_KINDS:
            out |= {("nextbase", kind, v) for v in CLASS_TABLE[5][1]}
    for name, values, _ in CLASS_TABLE[6:]:
        out |= {(name, v) for v in values}
    return out


def census(lib, oracle, rows, cols, frames, upsample=1, sift=DEFAULT_SIFT, offset=0, n_sub=1):
    """One call -> (launches, classes, site counts).  launches: the launches made, in order, as
    plain records; classes: the set of classes reached; counts: {site: launches} as a profiled
    call reports them.  offset: the byte offset of the device pointers (the misaligned classes)."""
    launches, classes, counts = [], set(), {}
    for n_img in planes_per_call(frames, n_sub):
        for e in walk(lib, oracle, [rows], [cols], n_img, upsample, sift):
            if not e["mask"][0, 0]:
                continue
            counts[e["site"]] = counts.get(e["site"], 0) + 1
            rec = {"site": e["site"], "octave": e["octave"], "level": e["level"], "R": int(e["R"][0, 0]), "C": int(e["C"][0, 0]),
                   "r": e["r"], "n_img": n_img, "streamed": False}
            if e["role"] is not None:
                rec["streamed"] = bool(e["streamed"][0, 0])
                if rec["streamed"]:
                    th, nb = int(e["th"][0, 0]), int(e["n_bands"][0, 0])
                    cpl = int(e["cpl"][0, 0])
                    last = rec["R"] - (nb - 1) * th
                    F = (2 * e["r"] + BS_P - 1) // BS_P * BS_P
                    thb = (last + BS_P - 1) // BS_P * BS_P
                    rec.update(kind=e["kinds"][0] if len(e["kinds"]) == 1 or cpl == 2 else e["kinds"][1], th=th, n_bands=nb,
                               n_strips=int(e["n_strips"][0, 0]), last_rows=last, r_mod_4=rec["R"] % 4,
                               blocks_first=(F + (th if nb > 1 else thb)) // BS_P % 2, blocks_last=(F + thb) // BS_P % 2,
                               next_base=bool(e["nb"][0, 0]) if "nb" in e else False)
                    if rec["next_base"]:
                        rec["next_parity"] = (int(e["nbR"][0, 0]) % 2, int(e["nbC"][0, 0]) % 2)
                    if e["role"] == BASE_U8:
                        bands = u8_bands(lib, e["r"], rec["R"], th)
                        rec["staging_rounds"] = max(b[4] for b in bands)
                        rec["staged_rows"] = [b[3] - b[2] + 1 for b in bands]
                else:
                    rec["refused"] = REFUSALS[int(e["refused"][0, 0])]
            launches.append(rec)
            for c, g in launch_classes(lib, e).items():
                if g[0, 0]:
                    classes.add(c)
    if ("rounds", "2") in classes or ("rounds", "3") in classes:
        if offset % 4:
            classes.add(("misaligned", str(offset % 4)))
    return launches, classes, counts


def domain_grids(lib, oracle, frames, upsample, rows=None, cols=None):
    """{class: bool grid over rows x cols} of the calls of `frames` frames in the search domain
    whose arena is within ARENA_CAP, and that arena"""
    rows = np.arange(MIN_SIDE, MAX_ROWS + 1) if rows is None else rows
    cols = np.arange(MIN_SIDE, MAX_COLS + 1) if cols is None else cols
    arena = arena_bytes(oracle, rows, cols, frames, upsample)
    ok = arena <= ARENA_CAP
    out = {}
    for n_img in planes_per_call(frames):
        for e in walk(lib, oracle, rows, cols, n_img, upsample):
            for c, g in launch_classes(lib, e).items():
                g = g & ok
                out[c] = out[c] | g if c in out else g
    return out, arena


def reachable_classes(lib, oracle):
    """the classes some call of the search domain reaches"""
    got = set()
    for frames in FRAMES:
        for up in (1, 0):
            grids, _ = domain_grids(lib, oracle, frames, up)
            got |= {c for c, g in grids.items() if g.any()}
    if ("rounds", "2") in got or ("rounds", "3") in got:
        got |= {("misaligned", v) for v in "123"}
    return got
