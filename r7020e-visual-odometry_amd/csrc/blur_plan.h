// blur_plan.h — how one scale-space blur is launched.  Plain host C++ (no HIP types), so the
// CPU suite compiles it too (oracle/blur_plan_eval.cpp); sift.hip launches what blur_plan()
// says and states none of these rules itself.
#pragma once

namespace vo {

// Kernel radii with compiled instantiations (the default sigmas' radii): k_blur_stream,
// k_blur_fused<r> and k_small_pyr's register-blocked passes.  Any other radius runs the
// runtime-radius forms.
#define VO_BLUR_RADII(X) X(5) X(6) X(8) X(10) X(13)

constexpr bool blur_radius_tabled(int r)
{
#define VO_BLUR_IS_R(RR) || r == RR
    return false VO_BLUR_RADII(VO_BLUR_IS_R);
#undef VO_BLUR_IS_R
}

// k_blur_stream's TAG template argument: the launch's role ...
constexpr int kTagLevel = 0;                // level blur of a float plane
constexpr int kTagBase = 1;                 // octave-0 base from a float plane (never stores a next-octave base)
constexpr int kTagBaseU8 = kTagBase | 4;    // 5: octave-0 base with the x2 upsample of the u8 image fused
// ... or-ed with the instrumentation bits of tools/blur_probe.hip and tools/base_probe.hip
constexpr int kTagCachedStores = 2;         // plain instead of non-temporal stores
constexpr int kTagNoRowPass = 8;
constexpr int kTagNoColPass = 16;
constexpr int kTagNoLds = 32;               // no LDS staging of the row
constexpr int kTagNoHalo = 64;              // no halo loads

#define BS_P 4            // prefetch depth (rows); 6 for the octave-0 base measured the same

// halo floats each side, rounded up to whole CPL-column vectors
constexpr int bs_rh(int r, int cpl) { return (r + cpl - 1) / cpl * cpl; }
// halo-lane layout of the streaming blur (sift.hip, "Row-window exchange"): 4-column lanes, r <= 5
constexpr int kBlurDppMaxR = 5;
constexpr bool bs_hl(int r, int cpl, int tag) { return cpl == 4 && r <= kBlurDppMaxR && !(tag & kTagNoLds); }
// output columns per strip
constexpr int bs_sw(int r, int cpl, int tag) { return 64 * cpl - (bs_hl(r, cpl, tag) ? 2 * bs_rh(r, cpl) : 0); }

// staged row length of the LDS row exchange: the strip's input columns and the halo each side
constexpr int bs_rw(int r, int cpl) { return 64 * cpl + 2 * bs_rh(r, cpl); }

// band height bound of the staged octave-0 base (kTagBaseU8): 8.7 KB of staged rows, so 16
// one-wave workgroups per CU fit (128: 11.1 KB, 14).  k_blur_stream's LDS is sized for it.
constexpr int kBaseMaxTH = 96;

// The staged octave-0 base keeps the u8 source rows of its band in LDS (sift.hip, U8Src).
// staged row length in dwords: the upsampled span of a wave (64 CPL columns + 2 RH halo) needs
// (64 CPL + 2 RH) / 2 + 3 source bytes; + 3 for the row's misalignment, + 4 for the word pair
constexpr int bs_u8_dw(int r, int cpl) { return ((64 * cpl + 2 * bs_rh(r, cpl)) / 2 + 3 + 3 + 4 + 3) / 4; }
// staged rows: a band reads F + TH upsampled rows (F = 2r + E, E < P), i.e. at most half as many
// source rows + 3 (the neighbour row of each end, rounding)
constexpr int bs_u8_rows(int r) { return (2 * r + BS_P + kBaseMaxTH) / 2 + 4; }
// The source rows [sr0, sr1] that the band of th output rows from row y0 of the R-row upsampled
// plane stages, of an image of src_rows rows.  The band reads the upsampled rows y0 - r - E ..
// y0 - r - E + F + th - 1, F the ring-fill steps; rows past either edge of the plane are
// reflected (101) back into it, which can reach beyond the range the unreflected rows span; an
// upsampled row y reads source rows y / 2 and its neighbour above or below.
// tests/test_blur_census.py holds sr1 - sr0 + 1 <= bs_u8_rows(r) over every streamed BaseU8 plan.
struct BsU8Rows { int sr0, sr1; };
constexpr BsU8Rows bs_u8_stage_rows(int r, int R, int src_rows, int y0, int th)
{
    const int F = (2 * r + BS_P - 1) / BS_P * BS_P, E = F - 2 * r;
    const int p_lo = y0 - r - E, p_hi = y0 - r - E + F + th - 1;
    int ymin = p_lo < 0 ? 0 : p_lo, ymax = p_hi >= R ? R - 1 : p_hi;
    if (p_lo < 0) { const int f = -p_lo < R - 1 ? -p_lo : R - 1; ymax = ymax > f ? ymax : f; }
    if (p_hi >= R) { const int f = 2 * R - 2 - p_hi > 0 ? 2 * R - 2 - p_hi : 0; ymin = ymin < f ? ymin : f; }
    const int a = (ymin >> 1) - 1, b = (ymax >> 1) + 1;
    return BsU8Rows{a > 0 ? a : 0, b < src_rows - 1 ? b : src_rows - 1};
}

enum class BlurRole { Level, BaseFloat, BaseU8 };

struct BlurPlan {
    BlurRole role;
    bool streamed;       // k_blur_stream; otherwise the tiled k_blur_fused, which reads a float plane
    // streamed launches (0 otherwise): columns per lane, TAG, band height, bands per plane, and
    // the strips per row that the grid covers
    int cpl, tag, th, n_bands, n_strips;
    // Level: the band height is not lowered for want of waves -- the plane is HBM-bound rather
    // than latency-bound (sift_enqueue_pyramid picks the fork octave of its two chains by it)
    bool full_bands;
};

constexpr int blur_bands(int R, int th) { return (R + th - 1) / th; }
constexpr int blur_grid_strips(int C, int r, int cpl, int tag) { return (C + bs_sw(r, cpl, tag) - 1) / bs_sw(r, cpl, tag); }

// The plan of one blur of n_img planes of R x C with kernel radius r.
//
// Band height: a multiple of BS_P, at most 128 rows, lowered on small octaves until the launch
// has ~2048 waves (8 per CU; 1024 measured ~1.5 % slower) -- small planes are latency-bound.
// Level blurs of planes at most 1400 columns wide use 2 columns per lane (128-column strips,
// half the ring registers): more waves and fewer idle lanes at the narrow octaves.  (2 columns
// per lane for the octave-0 levels of radius >= 13 / 10 / 8 too measured -0.8 / -0.9 / -4.3 %,
// profiles/r06_v_ab_fullpath_cpl_refine.txt.)
//
// The wave count behind the band height is taken at nominal strips of 64 cpl columns, while
// the grid covers the row in strips of bs_sw() output columns (240 rather than 256 at r = 5
// with 4-column lanes, whose outer lanes hold only halo).  The two differ on purpose: the
// measured band heights of every shape were set with the nominal count, so it stays.
//
// A BaseU8 plan that does not stream leaves the caller to stage the float plane (k_base_src)
// and to plan the blur again as BaseFloat: only a streamed launch can read the u8 image.
constexpr BlurPlan blur_plan(BlurRole role, int R, int C, int n_img, int r)
{
    constexpr int kMaxTH = 128, kWaveTarget = 2048, kCpl2MaxC = 1400, kU8MinRows = 64;
    const bool base = role != BlurRole::Level;
    const int cpl = (!base && C <= kCpl2MaxC) ? 2 : 4;
    const int tag = role == BlurRole::BaseU8 ? kTagBaseU8 : base ? kTagBase : kTagLevel;
    const long waves_rows = (long)R * ((C + 64 * cpl - 1) / (64 * cpl)) * n_img / kWaveTarget;
    const long cap = base && kBaseMaxTH < kMaxTH ? kBaseMaxTH : kMaxTH;
    int th = (int)(waves_rows < cap ? waves_rows : cap) / BS_P * BS_P;
    if (th < BS_P) th = BS_P;
    BlurPlan p{role, false, 0, 0, 0, 0, 0, !base && waves_rows >= kMaxTH};
    // streamed: a compiled radius, at least one whole band, one reflection fold per band edge;
    // the staged u8 form from 64 rows up
    if (!blur_radius_tabled(r) || R < th || R <= r + BS_P + 2 || (role == BlurRole::BaseU8 && R < kU8MinRows)) return p;
    p.streamed = true;
    p.cpl = cpl; p.tag = tag; p.th = th;
    p.n_bands = blur_bands(R, th);
    p.n_strips = blur_grid_strips(C, r, cpl, tag);
    return p;
}

}  // namespace vo
