/*
 * vo_spec.h — deterministic arithmetic primitives shared by the HIP product
 * path and the CPU oracle.
 *
 * Why this file exists
 * --------------------
 * The reference (VO.m) calls closed MathWorks toolbox functions whose
 * internals are not available.  Our parity bar is therefore
 * "GPU result == CPU restatement, bit for bit" for every integer/index
 * output (keypoint sets, match index pairs, inlier masks).  That is only
 * possible if both sides evaluate *the same* sequence of IEEE-754 basic
 * operations.  Basic ops (+ - * / sqrt, fmaf, rint, floor, int<->float
 * casts) are correctly rounded on both gfx950 (hipcc default float mode) and
 * x86-64 SSE; libm transcendentals are NOT identical across the two.  So every
 * transcendental the path needs (exp, atan2, sin/cos, log) is defined here as
 * a fixed polynomial/range-reduction recipe built only from basic ops, and
 * both sides are compiled with -ffp-contract=off (explicit fmaf where wanted).
 *
 * These are *spec primitives*: they define what the path computes.  The KAT
 * tests (tests/test_spec_math.py) pin each one against libm/numpy to a stated
 * tolerance.
 *
 * Usable from C (gcc, oracle) and HIP (hipcc, product).
 */
#ifndef VO_SPEC_H
#define VO_SPEC_H

#include <stdint.h>

#if defined(__HIPCC__)
#define VO_HD __host__ __device__ __forceinline__
#define VO_UNROLL _Pragma("unroll")
#else
#include <math.h>
#define VO_HD static inline
#define VO_UNROLL
#endif

/* ------------------------------------------------------------------------ */
/* Bit casts                                                                 */
/* ------------------------------------------------------------------------ */
VO_HD float vo_u32_as_f32(uint32_t u) { union { uint32_t u; float f; } c; c.u = u; return c.f; }
VO_HD uint32_t vo_f32_as_u32(float f) { union { uint32_t u; float f; } c; c.f = f; return c.u; }
VO_HD double vo_u64_as_f64(uint64_t u) { union { uint64_t u; double f; } c; c.u = u; return c.f; }
VO_HD uint64_t vo_f64_as_u64(double f) { union { uint64_t u; double f; } c; c.f = f; return c.u; }

/* round-half-even to int (cvRound semantics for |x| < 2^31) */
VO_HD int vo_round(float x) { return (int)rintf(x); }
VO_HD int vo_floor(float x) { return (int)floorf(x); }

/* ------------------------------------------------------------------------ */
/* exp (float).  Range reduction x = k*ln2 + r, |r| <= ln2/2, degree-7 Taylor */
/* in Horner form with explicit fmaf.  Returns 0 for x < -87.  Max rel error */
/* vs libm ~2 ulp (pinned in tests).                                         */
/* ------------------------------------------------------------------------ */
VO_HD float vo_expf(float x)
{
    if (x < -87.0f) return 0.0f;
    if (x > 88.0f) x = 88.0f;
    float kf = rintf(x * 1.44269504088896341f);
    float r = x - kf * 0.693145751953125f;          /* ln2 hi (exact product for |k|<=128) */
    r = r - kf * 1.42860682030941723212e-6f;        /* ln2 lo */
    float p = 1.98412698e-4f;                       /* 1/5040 */
    p = fmaf(p, r, 1.38888889e-3f);                 /* 1/720 */
    p = fmaf(p, r, 8.33333333e-3f);                 /* 1/120 */
    p = fmaf(p, r, 4.16666667e-2f);                 /* 1/24 */
    p = fmaf(p, r, 1.66666667e-1f);                 /* 1/6 */
    p = fmaf(p, r, 0.5f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    int k = (int)kf;
    /* p in [0.7, 1.42]; scale by 2^k in two steps to stay normal */
    int k1 = k / 2, k2 = k - k1;
    float s1 = vo_u32_as_f32((uint32_t)(k1 + 127) << 23);
    float s2 = vo_u32_as_f32((uint32_t)(k2 + 127) << 23);
    return (p * s1) * s2;
}

/* vo_expf on [-87, 0], for callers whose argument is a bounded non-positive quadratic form (the
 * SIFT window weights): the clamps never fire there, and p * 2^k is formed by one ldexp instead
 * of two scale factors.  Both forms are the one correctly rounded value of p * 2^k (the first
 * scale product is exact), so the result equals vo_expf(x) bit for bit on the whole domain --
 * checked for every float in [-87, 0] by oracle_spec_check_expf_nonpos (tests/test_spec_math.py). */
VO_HD float vo_expf_nonpos(float x)
{
    float kf = rintf(x * 1.44269504088896341f);
    float r = x - kf * 0.693145751953125f;
    r = r - kf * 1.42860682030941723212e-6f;
    float p = 1.98412698e-4f;
    p = fmaf(p, r, 1.38888889e-3f);
    p = fmaf(p, r, 8.33333333e-3f);
    p = fmaf(p, r, 4.16666667e-2f);
    p = fmaf(p, r, 1.66666667e-1f);
    p = fmaf(p, r, 0.5f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    return ldexpf(p, (int)kf);
}

/* ------------------------------------------------------------------------ */
/* Reciprocal of d in [2^-100, 2^100] by an integer seed and three Newton    */
/* steps r <- r + r (1 - d r), each two fmaf: basic ops only, so GPU == CPU  */
/* bit for bit.  The seed 0x7EF311C3 - bits(d) is within 12.5 % of 1/d; the  */
/* steps square the relative error (1.6e-2, 2.4e-4, 6e-8), so the result is  */
/* within ~2 ulp of 1/d (pinned against 1/d in tests/test_spec_math.py).     */
/* On gfx950 it is 7 full-rate VALU ops against the IEEE division's 11, one  */
/* of them the quarter-rate v_rcp_f32.                       */
/* ------------------------------------------------------------------------ */
VO_HD float vo_rcp_nr(float d)
{
    float r = vo_u32_as_f32(0x7EF311C3u - vo_f32_as_u32(d));
    float e = fmaf(-d, r, 1.0f);
    r = fmaf(r, e, r);
    e = fmaf(-d, r, 1.0f);
    r = fmaf(r, e, r);
    e = fmaf(-d, r, 1.0f);
    return fmaf(r, e, r);
}

/* ------------------------------------------------------------------------ */
/* Descriptor window weight, separable.  OpenCV weighs a descriptor sample  */
/* by exp((c_rot^2 + r_rot^2) s) with c_rot^2 + r_rot^2 = (i^2 + j^2) /      */
/* hist_width^2 (a rotation).  The spec takes the product of the two         */
/* one-dimensional factors (s' = s / hist_width^2),                          */
/*   w(i, j) = vo_sift_wt(s', |i|) * vo_sift_wt(s', |j|),                    */
/* equal in exact arithmetic and within float rounding of OpenCV's value,    */
/* so k_desc reads both factors from a per-keypoint table of radius + 1      */
/* entries instead of evaluating an exp per sample.  k^2 s' must lie in      */
/* [-87, 0] (vo_expf_nonpos): at most ~1.6 over the rotated square.  (The    */
/* orientation window keeps one exp of (i^2 + j^2) s: there the table's two  */
/* LDS reads per sample measured slower than the exp)        */
/* ------------------------------------------------------------------------ */
VO_HD float vo_sift_wt(float s, int k) { return vo_expf_nonpos((float)(k * k) * s); }

/* ------------------------------------------------------------------------ */
/* atan2 in DEGREES, result in [0, 360): OpenCV's fastAtan2 (the published  */
/* 7th-order polynomial cv::hal::fastAtan2 applies in SIFT's orientation     */
/* histogram and descriptor), with lo = min(|x|,|y|), hi = max:              */
/*   c = lo / (hi + DBL_EPSILON),  a = (((p7 c^2 + p5) c^2 + p3) c^2 + p1) c */
/* in degrees, then the octant/quadrant folds.  Deterministic form: the      */
/* quotient is lo * vo_rcp_nr(hi + DBL_EPSILON) (within 2 ulp of OpenCV's    */
/* division) and the Horner steps are fmaf; select-only, no branches.  The   */
/* polynomial's own error against the true atan2 is < 0.01 deg.  A result    */
/* that rounds up to 360 (y < 0 at a vanishing angle) wraps to 0.            */
/* ------------------------------------------------------------------------ */
VO_HD float vo_atan2_deg(float y, float x)
{
    const float ax = fabsf(x), ay = fabsf(y);
    const int swap = ay > ax;
    const float lo = swap ? ax : ay, hi = swap ? ay : ax;
    const float c = lo * vo_rcp_nr(hi + 2.220446049250313e-16f);
    const float c2 = c * c;
    const float p1 = 0.9997878412794807f * 57.29577951308232f, p3 = -0.3258083974640975f * 57.29577951308232f;
    const float p5 = 0.1555786518463281f * 57.29577951308232f, p7 = -0.04432655554792128f * 57.29577951308232f;
    float a = fmaf(fmaf(fmaf(p7, c2, p5), c2, p3), c2, p1) * c;
    a = swap ? 90.0f - a : a;
    a = x < 0.0f ? 180.0f - a : a;
    a = y < 0.0f ? 360.0f - a : a;
    return a >= 360.0f ? 0.0f : a;
}

/* ------------------------------------------------------------------------ */
/* sin / cos of an angle given in DEGREES, any finite value.                 */
/* Reduction in degrees (exact fmodf-free: integer quadrant), then Taylor.   */
/* ------------------------------------------------------------------------ */
VO_HD void vo_sincos_deg(float deg, float *s_out, float *c_out)
{
    /* quadrant q = round(deg/90), residual in [-45, 45] degrees */
    float qf = rintf(deg * (1.0f / 90.0f));
    float rd = deg - qf * 90.0f;                      /* exact for |deg| < 2^15 */
    float r = rd * 0.017453292519943296f;             /* radians, |r| <= pi/4 */
    float r2 = r * r;
    float s = -2.50521084e-8f;                        /* -1/11! */
    s = fmaf(s, r2, 2.75573192e-6f);                  /* 1/9! */
    s = fmaf(s, r2, -1.98412698e-4f);                 /* -1/7! */
    s = fmaf(s, r2, 8.33333333e-3f);                  /* 1/5! */
    s = fmaf(s, r2, -1.66666667e-1f);                 /* -1/3! */
    s = s * r2;
    s = fmaf(s, r, r);
    float c = 2.08767570e-9f;                         /* 1/12! */
    c = fmaf(c, r2, -2.75573192e-7f);                 /* -1/10! */
    c = fmaf(c, r2, 2.48015873e-5f);                  /* 1/8! */
    c = fmaf(c, r2, -1.38888889e-3f);                 /* -1/6! */
    c = fmaf(c, r2, 4.16666667e-2f);                  /* 1/4! */
    c = fmaf(c, r2, -0.5f);
    c = fmaf(c, r2, 1.0f);
    int q = ((int)qf) & 3;
    float so, co;
    if (q == 0)      { so = s;  co = c;  }
    else if (q == 1) { so = c;  co = -s; }
    else if (q == 2) { so = -s; co = -c; }
    else             { so = -c; co = s;  }
    *s_out = so; *c_out = co;
}

/* ------------------------------------------------------------------------ */
/* double exp / log (host+device), basic ops only.                           */
/* ------------------------------------------------------------------------ */
VO_HD double vo_exp_d(double x)
{
    if (x < -708.0) return 0.0;
    if (x > 709.0) x = 709.0;
    double kf = rint(x * 1.4426950408889634);
    double r = x - kf * 6.93147180369123816490e-01;
    r = r - kf * 1.90821492927058770002e-10;
    /* Taylor to r^13, |r| <= 0.347 -> truncation < 1e-17 */
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    int64_t k = (int64_t)kf;
    int64_t k1 = k / 2, k2 = k - k1;
    double s1 = vo_u64_as_f64((uint64_t)(k1 + 1023) << 52);
    double s2 = vo_u64_as_f64((uint64_t)(k2 + 1023) << 52);
    return (p * s1) * s2;
}

/* natural log for x > 0 (returns -inf-ish sentinel -1e308 for x <= 0) */
VO_HD double vo_log_d(double x)
{
    if (!(x > 0.0)) return -1.0e308;
    uint64_t u = vo_f64_as_u64(x);
    int e = (int)((u >> 52) & 0x7ff);
    if (e == 0) {                           /* subnormal: scale up */
        x = x * 18014398509481984.0;       /* 2^54 */
        u = vo_f64_as_u64(x);
        e = (int)((u >> 52) & 0x7ff) - 54;
    }
    e -= 1023;
    double m = vo_u64_as_f64((u & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL); /* [1,2) */
    if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
    double s = (m - 1.0) / (m + 1.0);        /* |s| <= 0.1716 */
    double s2 = s * s;
    double p = 1.0 / 23.0;
    p = fma(p, s2, 1.0 / 21.0);
    p = fma(p, s2, 1.0 / 19.0);
    p = fma(p, s2, 1.0 / 17.0);
    p = fma(p, s2, 1.0 / 15.0);
    p = fma(p, s2, 1.0 / 13.0);
    p = fma(p, s2, 1.0 / 11.0);
    p = fma(p, s2, 1.0 / 9.0);
    p = fma(p, s2, 1.0 / 7.0);
    p = fma(p, s2, 1.0 / 5.0);
    p = fma(p, s2, 1.0 / 3.0);
    p = fma(p, s2, 1.0);
    double lm = 2.0 * s * p;
    return (double)e * 6.93147180559945286227e-01 + lm;
}

/* ------------------------------------------------------------------------ */
/* Philox4x32-10 counter-based RNG (Salmon et al., SC'11).                   */
/* ------------------------------------------------------------------------ */
typedef struct { uint32_t v[4]; } vo_u32x4;

VO_HD vo_u32x4 vo_philox4x32_10(vo_u32x4 ctr, uint32_t k0, uint32_t k1)
{
    for (int i = 0; i < 10; ++i) {
        uint64_t p0 = (uint64_t)0xD2511F53u * ctr.v[0];
        uint64_t p1 = (uint64_t)0xCD9E8D57u * ctr.v[2];
        uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        vo_u32x4 n;
        n.v[0] = hi1 ^ ctr.v[1] ^ k0;
        n.v[1] = lo1;
        n.v[2] = hi0 ^ ctr.v[3] ^ k1;
        n.v[3] = lo0;
        ctr = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return ctr;
}

/* unbiased-enough index in [0, n) from a u32 (multiply-shift; spec) */
VO_HD uint32_t vo_rand_index(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * n) >> 32); }

/* ------------------------------------------------------------------------ */
/* Fixed-point histogram accumulation.  Integer addition is associative, so  */
/* the GPU may add contributions in any order (LDS atomics, per-lane rows,   */
/* several copies) and still equal the oracle's serial loop bit for bit.     */
/* Orientation and descriptor histograms: unsigned 32-bit fixed point at     */
/* 2^-10.  A weight v >= 0 is pre-scaled by 2^10 (exact: a power of two) and  */
/* enters as rintf(v).  Overflow-free by construction, |dI| <= 255 so one     */
/* weight is < 361*2^10:                                                      */
/*  - descriptor: a spatial bin collects fewer than (2*hist_width+2)^2 <=     */
/*    5.5e3 samples once the radius is capped at VO_SIFT_DESCR_RMAX           */
/*    (hist_width <= 36.3): < 2.1e9 < 2^32;                                   */
/*  - orientation: bins are summed in 64 bits (any window size).              */
/* A bin converts back with one correct rounding: (float)sum * 2^-10.        */
/* Rounding: floor(v + 1/2) (half up).  v + 1/2 is exact for v < 2^22, far  */
/* above any weight, so this is one v_cvt_rpi_i32_f32 on the GPU.           */
/* ------------------------------------------------------------------------ */
#define VO_DESC_FX_SCALE 1024.0f
VO_HD uint32_t vo_desc_fx_quant(float v_scaled) { return (uint32_t)floorf(v_scaled + 0.5f); }
VO_HD float vo_desc_fx_to_float(uint32_t s) { return (float)s * (1.0f / VO_DESC_FX_SCALE); }
VO_HD float vo_hist_fx_to_float(uint64_t s) { return (float)s * (1.0f / VO_DESC_FX_SCALE); }

/* ------------------------------------------------------------------------ */
/* SIFT scale-space constants (spec, OpenCV-4.x conventions).  Computed on  */
/* the host by both the oracle and libvo with the deterministic exp/log     */
/* above, so the float kernels are identical.                                */
/* ------------------------------------------------------------------------ */
#define VO_SIFT_MAX_LAYERS 8      /* n_octave_layers <= 5 -> levels <= 8 */
#define VO_SIFT_MAX_OCTAVES 16
#define VO_SIFT_MAX_RADIUS 40
#define VO_SIFT_BORDER 5
#define VO_SIFT_MAX_INTERP 5
#define VO_SIFT_ORI_BINS 36
#define VO_SIFT_ORI_SIG 1.5f
#define VO_SIFT_ORI_RADIUS 4.5f   /* 3 * 1.5 */
#define VO_SIFT_ORI_PEAK 0.8f
#define VO_SIFT_DESCR_W 4
#define VO_SIFT_DESCR_BINS 8
#define VO_SIFT_DESCR_SCL 3.0f
#define VO_SIFT_DESCR_MAG_THR 0.2f
#define VO_SIFT_DESCR_INT_FCTR 512.0f
#define VO_SIFT_DESCR_RMAX 127     /* descriptor window radius cap (38 at the defaults); (2 RMAX + 1)^2 < 2^16 */
#define VO_SIFT_MAX_PEAKS 18      /* strict local maxima in a 36-bin circle */
#define VO_FLT_EPSILON 1.19209290e-07f

/* round-half-even for doubles (cvRound) */
VO_HD int vo_round_d(double x) { return (int)rint(x); }

/* number of octaves: cvRound(log2(min(base rows, cols)) - 2) - firstOctave */
VO_HD int vo_num_octaves(int rows, int cols, int upsample)
{
    int br = upsample ? rows * 2 : rows, bc = upsample ? cols * 2 : cols;
    int m = br < bc ? br : bc;
    double l2 = vo_log_d((double)m) / 0.69314718055994531;
    int n = vo_round_d(l2 - 2.0) + (upsample ? 1 : 0);
    if (n < 1) n = 1;
    if (n > VO_SIFT_MAX_OCTAVES) n = VO_SIFT_MAX_OCTAVES;
    return n;
}

/* sigma of the incremental blur producing level i (i=1..L+2) from level i-1;
 * sig[0] = sigma (the octave base's absolute blur). */
VO_HD void vo_level_sigmas(int L, double sigma, double* sig)
{
    sig[0] = sigma;
    for (int i = 1; i < L + 3; ++i) {
        double sig_prev = vo_exp_d((double)(i - 1) * 0.69314718055994531 / (double)L) * sigma;
        double sig_total = sig_prev * vo_exp_d(0.69314718055994531 / (double)L);
        sig[i] = sqrt(sig_total * sig_total - sig_prev * sig_prev);
    }
}

/* blur applied to the (upsampled) input to reach `sigma` (SIFT_INIT_SIGMA .5) */
VO_HD double vo_base_sigma(double sigma, int upsample)
{
    double init = upsample ? 1.0 : 0.5;     /* 0.5 * 2 when upsampled */
    double v = sigma * sigma - init * init;
    if (v < 0.01) v = 0.01;
    return sqrt(v);
}

/* Radius vo_gauss_kernel gives for s (ksize / 2), without building the kernel; -1 when s is not
 * finite and positive or the radius exceeds VO_SIFT_MAX_RADIUS (the bound keeps the int cast defined). */
VO_HD int vo_gauss_radius(double s)
{
    if (!(s > 0.0) || !(s * 8.0 + 1.0 < 4.0 * VO_SIFT_MAX_RADIUS)) return -1;
    int r = (vo_round_d(s * 8.0 + 1.0) | 1) / 2;
    return r <= VO_SIFT_MAX_RADIUS ? r : -1;
}

/* Gaussian kernel (getGaussianKernel for float images, ksize = round(8s+1)|1).
 * Writes k[0..radius] (centre first); returns radius, or -1 (nothing written) if it is > cap-1
 * or > VO_SIFT_MAX_RADIUS (the size of t[] below). */
VO_HD int vo_gauss_kernel(double s, float* k, int cap)
{
    int r = vo_gauss_radius(s);
    if (r < 0 || r + 1 > cap) return -1;
    int ksize = 2 * r + 1;
    double t[2 * VO_SIFT_MAX_RADIUS + 1];
    double sum = 0.0, scale2x = -0.5 / (s * s);
    for (int i = 0; i < ksize; ++i) {
        double x = (double)(i - r);
        t[i] = vo_exp_d(scale2x * x * x);
        sum += t[i];
    }
    sum = 1.0 / sum;
    for (int i = 0; i <= r; ++i) k[i] = (float)(t[r + i] * sum);
    return r;
}

/* Whether every blur of the scale space has a kernel: the base blur and the level blurs 1..L+2
 * (vo_base_sigma, vo_level_sigmas) all within VO_SIFT_MAX_RADIUS.  The top level binds:
 * sigma <~ 1.45 at L = 1, 3.55 at L = 2, 5.2 at L = 3, 6.5 at L = 4, 7.7 at L = 5. */
VO_HD int vo_sift_radii_ok(int L, double sigma, int upsample)
{
    if (L < 1 || L + 3 > VO_SIFT_MAX_LAYERS || !(sigma > 0.0)) return 0;
    double sig[VO_SIFT_MAX_LAYERS];
    vo_level_sigmas(L, sigma, sig);
    if (vo_gauss_radius(vo_base_sigma(sigma, upsample)) < 0) return 0;
    for (int i = 1; i < L + 3; ++i)
        if (vo_gauss_radius(sig[i]) < 0) return 0;
    return 1;
}

/* reflect-101 border index (OpenCV BORDER_REFLECT_101, iterated) */
VO_HD int vo_reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) {
        if (p < 0) p = -p;
        else p = 2 * n - 2 - p;
    }
    return p;
}

/* ------------------------------------------------------------------------ */
/* undistortImage (VO.m:75-76): Brown-Conrady sampling map, bilinear taps,   */
/* 0 outside, rint back to u8.  f64 throughout, no contraction; every        */
/* expression below is kitti.undistort_map / kitti.undistort term by term,   */
/* in the order Python parses them (k2 * r2 * r2 = (k2 * r2) * r2,           */
/* 2.0 * p1 * x * y = ((2 * p1) * x) * y).  Pixel indices (u, v) are         */
/* 0-based (u = column); s is the skew K[0][1].                              */
/* ------------------------------------------------------------------------ */
typedef struct {
    double fx, fy, s, cx, cy;     /* K[0][0], K[1][1], K[0][1], K[0][2], K[1][2] */
    double k1, k2, k3, p1, p2;    /* radial, tangential */
} vo_bc_cam;

/* where output pixel (u, v) samples the distorted image */
VO_HD void vo_undistort_pos(const vo_bc_cam* m, int u, int v, double* us, double* vs)
{
    double y = ((double)v - m->cy) / m->fy;
    double x = ((double)u - m->cx - m->s * y) / m->fx;
    double r2 = x * x + y * y;
    double rad = 1.0 + m->k1 * r2 + m->k2 * r2 * r2 + m->k3 * r2 * r2 * r2;
    double xd = x * rad + 2.0 * m->p1 * x * y + m->p2 * (r2 + 2.0 * x * x);
    double yd = y * rad + m->p1 * (r2 + 2.0 * y * y) + 2.0 * m->p2 * x * y;
    *us = m->fx * xd + m->s * yd + m->cx;
    *vs = m->fy * yd + m->cy;
}

/* A position outside [-1, cols) x [-1, rows) has no tap inside the image and gives 0; NaN and
 * +-inf fail the comparisons, so the test is made here, in f64, before any integer conversion. */
VO_HD int vo_undistort_inside(double us, double vs, int rows, int cols)
{
    return us >= -1.0 && us < (double)cols && vs >= -1.0 && vs < (double)rows;
}

/* the four taps (0.0 for a tap outside the image) at fractions ax = us - floor(us),
 * ay = vs - floor(vs), summed left to right, rounded half to even and clamped to u8 */
VO_HD uint8_t vo_undistort_u8(double t00, double t01, double t10, double t11, double ax, double ay)
{
    double o = t00 * (1.0 - ax) * (1.0 - ay) + t01 * ax * (1.0 - ay) + t10 * (1.0 - ax) * ay + t11 * ax * ay;
    o = rint(o);
    o = o < 0.0 ? 0.0 : (o > 255.0 ? 255.0 : o);
    return (uint8_t)o;
}

/* ------------------------------------------------------------------------ */
/* triangulate and estworldpose: the DLT point, Grunert's   */
/* P3P on either side of its root finder, and the pose MSAC's sample, trial  */
/* bound, replay and camera pose.  One definition for the kernels            */
/* (k_gather_tri, k_tri_list, k_lm_tri, k_msac; geom.hip) and the oracle     */
/* (oracle/vo_ref.c), equal by bytes: f64 + - * / and sqrt in the order      */
/* written, no contraction, vo_log_d the only transcendental.  The float64   */
/* numpy references of tests/geom_ref.py are the independent check.          */
/* ------------------------------------------------------------------------ */
/* One point from two views: the null vector of the 4x4 DLT system by one-sided Jacobi (Hestenes),
 * at most 30 sweeps, rotations skipped at |g| <= 1e-15 sqrt(a b); the column of the smallest norm
 * (the first of equals), dehomogenised and rounded through single as MATLAB returns single for
 * single inputs.  P1 / P2 3x4 row-major.  Every index is a compile-time constant once unrolled,
 * which keeps A and V in registers on the device. */
VO_HD void vo_dlt_point(float u1f, float v1f, float u2f, float v2f, const double* P1, const double* P2, double* X)
{
    double u1 = u1f, v1 = v1f, u2 = u2f, v2 = v2f;
    double A[4][4];   /* A[row][col] */
    VO_UNROLL
    for (int c = 0; c < 4; ++c) {
        A[0][c] = u1 * P1[8 + c] - P1[c];
        A[1][c] = v1 * P1[8 + c] - P1[4 + c];
        A[2][c] = u2 * P2[8 + c] - P2[c];
        A[3][c] = v2 * P2[8 + c] - P2[4 + c];
    }
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 30; ++sweep) {
        int rotated = 0;
        VO_UNROLL
        for (int p = 0; p < 3; ++p)
            VO_UNROLL
            for (int q = p + 1; q < 4; ++q) {
                double al = 0, be = 0, ga = 0;
                VO_UNROLL
                for (int i = 0; i < 4; ++i) {
                    al = al + A[i][p] * A[i][p];
                    be = be + A[i][q] * A[i][q];
                    ga = ga + A[i][p] * A[i][q];
                }
                if (ga == 0.0 || fabs(ga) <= 1e-15 * sqrt(al * be)) continue;
                rotated = 1;
                double zeta = (be - al) / (2.0 * ga);
                double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                double c = 1.0 / sqrt(1.0 + t * t);
                double s = c * t;
                VO_UNROLL
                for (int i = 0; i < 4; ++i) {
                    double ap = A[i][p], aq = A[i][q];
                    A[i][p] = c * ap - s * aq;
                    A[i][q] = s * ap + c * aq;
                    double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - s * vq;
                    V[i][q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    int jmin = 0;
    double nmin = 0;
    VO_UNROLL
    for (int j = 0; j < 4; ++j) {
        double nj = 0;
        VO_UNROLL
        for (int i = 0; i < 4; ++i) nj = nj + A[i][j] * A[i][j];
        if (j == 0 || nj < nmin) { nmin = nj; jmin = j; }
    }
    double x = 0, y = 0, z = 0, w = 1;   /* column jmin, selected without a runtime index */
    VO_UNROLL
    for (int j = 0; j < 4; ++j)
        if (j == jmin) { x = V[0][j]; y = V[1][j]; z = V[2][j]; w = V[3][j]; }
    X[0] = (double)(float)(x / w);
    X[1] = (double)(float)(y / w);
    X[2] = (double)(float)(z / w);
}

/* Squared pixel error of X under Xc = R X + t (R 3x3 row-major) and the intrinsics K (fx = K[0],
 * s = K[1], cx = K[2], fy = K[4], cy = K[5]); +inf for a point not in front of the camera. */
VO_HD double vo_pose_reproj_err2(const double* R, const double* t, const double* K, const double* X, const double* uv)
{
    double xc = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
    double yc = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
    double zc = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
    if (!(zc > 0)) return INFINITY;
    double xn = xc / zc, yn = yc / zc;
    double u = K[0] * xn + K[1] * yn + K[2];
    double v = K[4] * yn + K[5];
    double du = u - uv[0], dv = v - uv[1];
    return du * du + dv * dv;
}

/* P3P: Grunert's quartic in v = s3 / s1 (Haralick et al. 1994), coefficients by polynomial algebra.
 * vo_p3p_setup builds the quartic P of three correspondences, the caller finds its real roots in
 * ascending order with its own root finder (the oracle's recursive real_roots, the kernel's
 * register-resident templates), and vo_p3p_pose turns one root into a pose.  The caller owns the
 * loop over the roots and stops at the fourth pose. */
VO_HD void vo_p3p_pmul(const double* a, int da, const double* b, int db, double* out)
{
    for (int i = 0; i <= da + db; ++i) out[i] = 0.0;
    for (int i = 0; i <= da; ++i)
        for (int j = 0; j <= db; ++j) out[i + j] = out[i + j] + a[i] * b[j];
}

VO_HD void vo_p3p_bearing(const double* K, double u, double v, double* f)
{
    double yn = (v - K[5]) / K[4];
    double xn = (u - K[2] - K[1] * yn) / K[0];
    double n = sqrt(xn * xn + yn * yn + 1.0);
    f[0] = xn / n; f[1] = yn / n; f[2] = 1.0 / n;
}

VO_HD void vo_p3p_cross3(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

VO_HD int vo_p3p_normalize3(double* a)
{
    double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (!(n > 0)) return 0;
    a[0] = a[0] / n; a[1] = a[1] / n; a[2] = a[2] / n;
    return 1;
}

/* rotation R (row-major) and t with Pc = R Pw + t from 3 congruent points */
VO_HD int vo_p3p_align3(const double Pw[3][3], const double Pc[3][3], double* R, double* t)
{
    double ew[3][3], ec[3][3];   /* ew[k] = k-th basis vector */
    double d1[3], d2[3];
    for (int i = 0; i < 3; ++i) { ew[0][i] = Pw[1][i] - Pw[0][i]; d1[i] = Pw[2][i] - Pw[0][i]; }
    if (!vo_p3p_normalize3(ew[0])) return 0;
    vo_p3p_cross3(ew[0], d1, ew[2]);
    if (!vo_p3p_normalize3(ew[2])) return 0;
    vo_p3p_cross3(ew[2], ew[0], ew[1]);
    for (int i = 0; i < 3; ++i) { ec[0][i] = Pc[1][i] - Pc[0][i]; d2[i] = Pc[2][i] - Pc[0][i]; }
    if (!vo_p3p_normalize3(ec[0])) return 0;
    vo_p3p_cross3(ec[0], d2, ec[2]);
    if (!vo_p3p_normalize3(ec[2])) return 0;
    vo_p3p_cross3(ec[2], ec[0], ec[1]);
    /* R = Ec * Ew^T : R[i][j] = sum_k ec[k][i] * ew[k][j] */
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = ec[0][i] * ew[0][j] + ec[1][i] * ew[1][j] + ec[2][i] * ew[2][j];
    double mw[3], mc[3];
    for (int i = 0; i < 3; ++i) {
        mw[i] = (Pw[0][i] + Pw[1][i] + Pw[2][i]) / 3.0;
        mc[i] = (Pc[0][i] + Pc[1][i] + Pc[2][i]) / 3.0;
    }
    for (int i = 0; i < 3; ++i) t[i] = mc[i] - (R[3 * i] * mw[0] + R[3 * i + 1] * mw[1] + R[3 * i + 2] * mw[2]);
    return 1;
}

/* j: unit bearings of the image points; u = N(v) / D(v), s1 = sqrt(b2 / Q(v));
 * P = D^2 + N^2 - 2 cg N D - (c2 / b2) Q D^2, coefficient i at x^i */
typedef struct { double j[3][3], b2, N[3], D[2], Q[3], P[5]; } vo_p3p;

/* returns 0 for a degenerate world triangle (two points coincide, or a NaN) */
VO_HD int vo_p3p_setup(const double img[3][2], const double world[3][3], const double* K, vo_p3p* s)
{
    for (int i = 0; i < 3; ++i) vo_p3p_bearing(K, img[i][0], img[i][1], s->j[i]);
    double dv[3];
    for (int i = 0; i < 3; ++i) dv[i] = world[1][i] - world[2][i];
    double a2 = dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2];
    for (int i = 0; i < 3; ++i) dv[i] = world[0][i] - world[2][i];
    double b2 = dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2];
    for (int i = 0; i < 3; ++i) dv[i] = world[0][i] - world[1][i];
    double c2 = dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2];
    if (!(a2 > 0 && b2 > 0 && c2 > 0)) return 0;
    double ca = s->j[1][0] * s->j[2][0] + s->j[1][1] * s->j[2][1] + s->j[1][2] * s->j[2][2];  /* cos alpha: rays 2,3 */
    double cb = s->j[0][0] * s->j[2][0] + s->j[0][1] * s->j[2][1] + s->j[0][2] * s->j[2][2];  /* cos beta:  rays 1,3 */
    double cg = s->j[0][0] * s->j[1][0] + s->j[0][1] * s->j[1][1] + s->j[0][2] * s->j[1][2];  /* cos gamma: rays 1,2 */
    double Kq = (a2 - c2) / b2, cb2 = c2 / b2;
    s->b2 = b2;
    s->N[0] = 1.0 + Kq; s->N[1] = -2.0 * Kq * cb; s->N[2] = Kq - 1.0;
    s->D[0] = 2.0 * cg; s->D[1] = -2.0 * ca;
    s->Q[0] = 1.0; s->Q[1] = -2.0 * cb; s->Q[2] = 1.0;
    double DD[3], NN[5], ND[4], QDD[5];
    vo_p3p_pmul(s->D, 1, s->D, 1, DD);
    vo_p3p_pmul(s->N, 2, s->N, 2, NN);
    vo_p3p_pmul(s->N, 2, s->D, 1, ND);
    vo_p3p_pmul(s->Q, 2, DD, 2, QDD);
    for (int i = 0; i < 5; ++i) {
        double v = NN[i] - cb2 * QDD[i];
        if (i < 3) v = v + DD[i];
        if (i < 4) v = v - 2.0 * cg * ND[i];
        s->P[i] = v;
    }
    return 1;
}

/* The pose of root v: 1 and (R, t) with Xc = R Xw + t when v > 0, D(v) != 0, u > 0, Q(v) > 0 and
 * the two triangles align; world is the triangle given to vo_p3p_setup. */
VO_HD int vo_p3p_pose(const vo_p3p* s, const double world[3][3], double v, double* R, double* t)
{
    if (!(v > 0)) return 0;
    double Dv = s->D[0] + s->D[1] * v;
    if (Dv == 0.0) return 0;
    double u = (s->N[0] + s->N[1] * v + s->N[2] * v * v) / Dv;
    if (!(u > 0)) return 0;
    double Qv = s->Q[0] + s->Q[1] * v + s->Q[2] * v * v;
    if (!(Qv > 0)) return 0;
    double s1 = sqrt(s->b2 / Qv), s2 = u * s1, s3 = v * s1;
    double Pc[3][3];
    for (int i = 0; i < 3; ++i) { Pc[0][i] = s1 * s->j[0][i]; Pc[1][i] = s2 * s->j[1][i]; Pc[2][i] = s3 * s->j[2][i]; }
    return vo_p3p_align3(world, Pc, R, t);
}

/* Slot `slot` of the frame with key `key`: up to 16 attempts, each 4 indices from one Philox call
 * (counter {slot, attempt, key, 0x5EED}, key words {seed, 0x9E3779B9}); the first attempt whose 4
 * indices are distinct is the sample.  Returns 0 when all 16 fail (n < 4 always does). */
VO_HD int vo_pose_sample(uint32_t seed, uint32_t key, uint32_t slot, uint32_t n, uint32_t* idx)
{
    for (uint32_t att = 0; att < 16; ++att) {
        vo_u32x4 c = {{slot, att, key, 0x5EEDu}};
        vo_u32x4 r = vo_philox4x32_10(c, seed, 0x9E3779B9u);
        for (int q = 0; q < 4; ++q) idx[q] = vo_rand_index(r.v[q], n);
        if (idx[0] != idx[1] && idx[0] != idx[2] && idx[0] != idx[3] && idx[1] != idx[2] && idx[1] != idx[3] && idx[2] != idx[3])
            return 1;
    }
    return 0;
}

/* Trials after which a sample of 4 inliers was drawn with probability conf (a fraction), at the
 * inlier ratio w = n_in / n: ceil(log(1 - conf) / log(1 - w^4)) clamped to [1, INT_MAX], w^4 =
 * ((w w) w) w.  w^4 <= 1e-300 (or NaN) gives INT_MAX: no bound.  At w = 1 the logarithm is -inf, the
 * quotient +0 and the result 1.  A logarithm that is not negative -- the 0 of a w^4 below half an ulp
 * of 1 -- gives 1.  This is not vo_fund_trials_needed with another exponent and stays apart from it:
 * that one tests w^8 >= 1 first and answers a zero logarithm with "no bound" (DESIGN 3.5.2). */
VO_HD int vo_pose_trials_needed(int n_in, int n, double conf)
{
    double w = (double)n_in / (double)n;
    double w4 = w * w * w * w;
    if (!(w4 > 1e-300)) return 0x7fffffff;
    double den = vo_log_d(1.0 - w4);
    if (!(den < 0)) return 1;
    double num = vo_log_d(1.0 - conf);
    double N = ceil(num / den);
    if (N > 2147483647.0) return 0x7fffffff;
    if (N < 1.0) return 1;
    return (int)N;
}

/* The sum of an MSAC score, of a refinement pass and of a masked Norm8 fit: 64 lane-strided partials
 * (partial l adds the items k = l (mod 64), ascending) joined by the pairwise tree
 *     p[i] = p[i] + p[i + off]  for i < off,  off = 32, 16, .. 1,
 * each a single IEEE addition; the sum is p[0].  m values per partial are summed side by side;
 * partial l is at p + l * stride, the result in p[0 .. m).  VO_REFINE_LANES and VO_FUND_LANES name
 * the 64.  On the device this function is wave_sum (csrc/wave.h), one partial per lane. */
VO_HD void vo_tree_sum(double* p, int stride, int m)
{
    for (int off = 32; off >= 1; off >>= 1)
        for (int i = 0; i < off; ++i)
            for (int q = 0; q < m; ++q) p[i * stride + q] = p[i * stride + q] + p[(i + off) * stride + q];
}

/* The sequential MSAC loop, replayed slot by slot in slot order over (valid, score, n_in):
 *     vo_pose_replay_begin(&r, max_num_trials);
 *     for slot = 0 .. max_num_trials - 1, while !vo_pose_replay_done(&r):  vo_pose_replay_slot(...)
 * An invalid slot (no 4 distinct indices, or a sample without a pose) counts as no trial.  A valid
 * one counts, and replaces the best iff its score is strictly smaller; the bound is then
 * min(bound, vo_pose_trials_needed).  Done once trials >= bound.  Returns 1 when the slot became
 * the best (a caller that does not keep every slot keeps its R, t). */
typedef struct { int bound, trials, best, best_in; double best_score; } vo_pose_replay;

VO_HD void vo_pose_replay_begin(vo_pose_replay* r, int max_num_trials)
{
    r->bound = max_num_trials; r->trials = 0; r->best = -1; r->best_in = 0;
    r->best_score = INFINITY;
}

VO_HD int vo_pose_replay_done(const vo_pose_replay* r) { return r->trials >= r->bound; }

VO_HD int vo_pose_replay_slot(vo_pose_replay* r, int slot, int valid, double score, int n_in, int n, double conf)
{
    if (!valid) return 0;
    r->trials = r->trials + 1;
    if (!(score < r->best_score)) return 0;
    r->best_score = score; r->best = slot; r->best_in = n_in;
    int need = vo_pose_trials_needed(n_in, n, conf);
    if (need < r->bound) r->bound = need;
    return 1;
}

/* The camera pose in the world, rigidtform3d.A row-major, of the extrinsics Xc = R X + t:
 * [R^T, -R^T t; 0 0 0 1]. */
VO_HD void vo_pose_to_T(const double* R, const double* t, double* T)
{
    VO_UNROLL
    for (int i = 0; i < 3; ++i) {
        T[4 * i] = R[i]; T[4 * i + 1] = R[3 + i]; T[4 * i + 2] = R[6 + i];
        T[4 * i + 3] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
    }
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}

/* ------------------------------------------------------------------------ */
/* triangulate's second and third outputs (reprojectionErrors, validIndex)   */
/* of one point.  X is the point as vo_triangulate returns it -- the doubles */
/* already rounded through single, not the unrounded null vector -- so a     */
/* caller reproduces both values from the outputs alone.  (u1, v1), (u2, v2) */
/* are the single pixel positions, P1 / P2 3x4 row-major.  f64 basic ops in  */
/* the order written, no contraction.  Per view:                             */
/*   h0 = ((P[0] X0 + P[1] X1) + P[2] X2) + P[3],  h1 likewise on row 1,     */
/*   w on row 2;  e = sqrt((h0 / w - u)^2 + (h1 / w - v)^2)                  */
/* *err = (float)((e1 + e2) * 0.5), the mean reprojection distance; returns  */
/* valid = w1 > 0 && w2 > 0 (for P = K [R t]: in front of both cameras).     */
/* Nothing is clamped: a NaN w fails the comparison (valid 0), and err is    */
/* what IEEE arithmetic gives (NaN or +-inf for a non-finite X or w = 0).    */
/* ------------------------------------------------------------------------ */
VO_HD double vo_tri_view_err(const double* X, double u, double v, const double* P, double* w_out)
{
    double h0 = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3];
    double h1 = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7];
    double w = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
    double du = h0 / w - u;
    double dv = h1 / w - v;
    *w_out = w;
    return sqrt(du * du + dv * dv);
}

VO_HD int vo_tri_quality(const double* X, float u1, float v1, float u2, float v2, const double* P1, const double* P2,
                         float* err)
{
    double w1, w2;
    double e1 = vo_tri_view_err(X, (double)u1, (double)v1, P1, &w1);
    double e2 = vo_tri_view_err(X, (double)u2, (double)v2, P2, &w2);
    *err = (float)((e1 + e2) * 0.5);
    return (w1 > 0.0) && (w2 > 0.0);
}

/* ------------------------------------------------------------------------ */
/* bundleAdjustmentMotion after estworldpose (VO.m:123-130): motion-only     */
/* bundle adjustment, Levenberg-Marquardt on the squared pixel residuals of  */
/* the used points with the points held fixed.  One definition for the       */
/* kernel (k_refine_pose, geom.hip) and the CPU reference                    */
/* (tests/pose_refine_ref), equal by bytes: f64 only, + - * / and sqrt in    */
/* the order written, no contraction, no libm.  include/vo.h has the         */
/* interface-level description.                                              */
/*                                                                           */
/* State: extrinsics R (3x3 row-major), t with Xc = R X + t -- MsacHyp's     */
/* convention.  A pose given as rigidtform3d.A converts with                 */
/* vo_refine_from_T and back with vo_refine_to_T (vo_pose_to_T by name).    */
/* Used set U = { k : use[k] != 0 and zc_k > 0 at the initial pose }, fixed  */
/* for the call: every pass re-evaluates zc_k at the initial pose from its   */
/* third row (z0 = R0[6..8], t0[2]) instead of storing a mask.               */
/* ------------------------------------------------------------------------ */
#define VO_REFINE_CONVERGED   0
#define VO_REFINE_MAX_ITER    1
#define VO_REFINE_DAMPING     2
#define VO_REFINE_DEGENERATE -1
#define VO_REFINE_TOO_FEW    -3
#define VO_REFINE_LAMBDA_MIN 1e-12
#define VO_REFINE_LAMBDA_MAX 1e12
#define VO_REFINE_NSUM 28           /* 21 of H's upper triangle row-major, 6 of g, the cost */
#define VO_REFINE_LANES 64          /* partial sums: partial l adds the points k = l (mod 64), ascending; joined by vo_tree_sum */

VO_HD void vo_refine_from_T(const double* T, double* R, double* t)
{
    VO_UNROLL
    for (int i = 0; i < 3; ++i) {
        R[3 * i] = T[i]; R[3 * i + 1] = T[4 + i]; R[3 * i + 2] = T[8 + i];
    }
    VO_UNROLL
    for (int i = 0; i < 3; ++i) t[i] = -(R[3 * i] * T[3] + R[3 * i + 1] * T[7] + R[3 * i + 2] * T[11]);
}

VO_HD void vo_refine_to_T(const double* R, const double* t, double* T) { vo_pose_to_T(R, t, T); }

/* One point of one pass at the pose (R, t).  Returns 1 when the point is in U (0: it adds nothing).
 * A point of U with !(zc > 0) at this pose adds nothing and sets *behind.  Otherwise, with K read as
 * vo_pose_reproj_err2 reads it (fx = K[0], s = K[1], cx = K[2], fy = K[4], cy = K[5]):
 *   residual  ru = (fx xn + s yn + cx) - u,  rv = (fy yn + cy) - v,   xn = xc / zc, yn = yc / zc
 *   rows of the Jacobian for the left perturbation Xc' = Xc + w x Xc + v:  (Xc x a, a), (Xc x b, b)
 *   with a = (fx / zc, s / zc, -(fx xn + s yn) / zc),  b = (0, fy / zc, -(fy yn) / zc)
 * and acc[0..20] += Ju_i Ju_j + Jv_i Jv_j (i <= j, row-major), acc[21..26] += Ju_i ru + Jv_i rv,
 * acc[27] += ru ru + rv rv. */
VO_HD int vo_refine_point(const double* R, const double* t, const double* z0, const double* K, const double* X,
                          const double* uv, int use, double* acc, int* behind)
{
    double zi = z0[0] * X[0] + z0[1] * X[1] + z0[2] * X[2] + z0[3];
    if (!use || !(zi > 0.0)) return 0;
    double xc = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
    double yc = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
    double zc = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
    if (!(zc > 0.0)) { *behind = 1; return 1; }
    double xn = xc / zc, yn = yc / zc;
    double pu = K[0] * xn + K[1] * yn;
    double pv = K[4] * yn;
    double ru = (pu + K[2]) - uv[0];
    double rv = (pv + K[5]) - uv[1];
    double a0 = K[0] / zc, a1 = K[1] / zc, a2 = -(pu / zc);
    double b1 = K[4] / zc, b2 = -(pv / zc);
    double Ju[6], Jv[6];
    Ju[0] = yc * a2 - zc * a1; Ju[1] = zc * a0 - xc * a2; Ju[2] = xc * a1 - yc * a0;
    Ju[3] = a0; Ju[4] = a1; Ju[5] = a2;
    Jv[0] = yc * b2 - zc * b1; Jv[1] = -(xc * b2); Jv[2] = xc * b1;
    Jv[3] = 0.0; Jv[4] = b1; Jv[5] = b2;
    int q = 0;
    VO_UNROLL
    for (int i = 0; i < 6; ++i) {
        VO_UNROLL
        for (int j = i; j < 6; ++j) {
            acc[q] = acc[q] + (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
            ++q;
        }
    }
    VO_UNROLL
    for (int i = 0; i < 6; ++i) acc[21 + i] = acc[21 + i] + (Ju[i] * ru + Jv[i] * rv);
    acc[27] = acc[27] + (ru * ru + rv * rv);
    return 1;
}

/* (H + lambda diag(H)) d = -g by a 6x6 Cholesky in a fixed order; H is the row-major upper triangle.
 * Returns 0 ("no step") at a pivot that is not > 0. */
VO_HD int vo_refine_solve(const double* H, const double* g, double lambda, double* d)
{
    double A[6][6], L[6][6], y[6];
    int q = 0;
    VO_UNROLL
    for (int i = 0; i < 6; ++i) {
        VO_UNROLL
        for (int j = i; j < 6; ++j) {
            A[j][i] = H[q];                       /* the lower triangle is what the factor reads */
            ++q;
        }
    }
    VO_UNROLL
    for (int i = 0; i < 6; ++i) A[i][i] = A[i][i] + lambda * A[i][i];
    int ok = 1;
    VO_UNROLL
    for (int j = 0; j < 6; ++j) {
        double s = A[j][j];
        VO_UNROLL
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
        if (!(s > 0.0)) ok = 0;
        double dj = sqrt(s);
        L[j][j] = dj;
        VO_UNROLL
        for (int i = j + 1; i < 6; ++i) {
            double r = A[i][j];
            VO_UNROLL
            for (int k = 0; k < j; ++k) r = r - L[i][k] * L[j][k];
            L[i][j] = r / dj;
        }
    }
    VO_UNROLL
    for (int i = 0; i < 6; ++i) {
        double s = -g[i];
        VO_UNROLL
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    VO_UNROLL
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        VO_UNROLL
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * d[k];
        d[i] = s / L[i][i];
    }
    return ok;
}

/* Retraction of the step d = (w, v): q = (1, w / 2) / sqrt(1 + |w|^2 / 4), dR from the unit quaternion
 * by the polynomial formula, R' = dR R, t' = dR t + v. */
VO_HD void vo_refine_retract(const double* R, const double* t, const double* d, double* Rn, double* tn)
{
    double hx = 0.5 * d[0], hy = 0.5 * d[1], hz = 0.5 * d[2];
    double n = sqrt(1.0 + (hx * hx + hy * hy + hz * hz));
    double w = 1.0 / n, x = hx / n, y = hy / n, z = hz / n;
    double D[9];
    D[0] = 1.0 - 2.0 * (y * y + z * z); D[1] = 2.0 * (x * y - w * z); D[2] = 2.0 * (x * z + w * y);
    D[3] = 2.0 * (x * y + w * z); D[4] = 1.0 - 2.0 * (x * x + z * z); D[5] = 2.0 * (y * z - w * x);
    D[6] = 2.0 * (x * z - w * y); D[7] = 2.0 * (y * z + w * x); D[8] = 1.0 - 2.0 * (x * x + y * y);
    VO_UNROLL
    for (int i = 0; i < 3; ++i) {
        VO_UNROLL
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = D[3 * i] * R[j] + D[3 * i + 1] * R[3 + j] + D[3 * i + 2] * R[6 + j];
        tn[i] = (D[3 * i] * t[0] + D[3 * i + 1] * t[1] + D[3 * i + 2] * t[2]) + d[3 + i];
    }
}

/* The Levenberg-Marquardt loop, one pass over the points per trial, as a state machine around the
 * caller's pass (the kernel's wave-wide one, the reference's loop over 64 partials):
 *
 *     vo_refine_begin(&st, R, t, lambda0);
 *     sums, n_used, behind <- pass at (st.R, st.t)
 *     vo_refine_first(&st, sums, n_used);
 *     while (vo_refine_propose(&st, max_iterations)) {
 *         sums, behind <- pass at (st.Rc, st.tc)
 *         vo_refine_update(&st, sums, behind, relative_tolerance, absolute_tolerance);
 *     }
 *
 * A pass is the 28 sums of vo_refine_point over the points, summed in 64 partials (partial l: the
 * points k = l mod 64 in ascending k, from +0) and then the tree p[i] = p[i] + p[i + off] for
 * off = 32 .. 1, i < off; the result is p[0].
 * first: n_used < 3 ends with TOO_FEW, a non-finite sum with DEGENERATE; both keep the input pose.
 * propose: MAX_ITER once passes >= max_iterations; otherwise solve at lambda, lambda *= 10 on "no
 * step", DAMPING once lambda > lambda_max; the candidate is (Rc, tc).
 * update: accept iff !behind && c' < c (a NaN c' fails).  On accept take the candidate and its H, g,
 * lambda = max(lambda / 10, lambda_min), CONVERGED when c - c' <= relative_tolerance * c or
 * c' <= absolute_tolerance * n_used; otherwise lambda *= 10.
 * (R, t) is always the last accepted pose, c its cost: cost_final <= cost_initial. */
typedef struct {
    double R[9], t[3];              /* the last accepted pose */
    double Rc[9], tc[3];            /* the candidate */
    double H[21], g[6], c;          /* sums at (R, t) */
    double c0, lambda;
    int status, n_used, passes, accepted, done;
} vo_refine_state;

VO_HD void vo_refine_begin(vo_refine_state* s, const double* R, const double* t, double lambda0)
{
    VO_UNROLL
    for (int i = 0; i < 9; ++i) { s->R[i] = R[i]; s->Rc[i] = R[i]; }
    VO_UNROLL
    for (int i = 0; i < 3; ++i) { s->t[i] = t[i]; s->tc[i] = t[i]; }
    s->lambda = lambda0;
    s->status = VO_REFINE_MAX_ITER; s->n_used = 0; s->passes = 0; s->accepted = 0; s->done = 0;
    s->c = 0.0; s->c0 = 0.0;
}

VO_HD void vo_refine_first(vo_refine_state* s, const double* sums, int n_used)
{
    s->n_used = n_used;
    s->passes = 1;
    s->c = sums[27];
    s->c0 = sums[27];
    int finite = 1;
    VO_UNROLL
    for (int i = 0; i < VO_REFINE_NSUM; ++i) if (!(sums[i] - sums[i] == 0.0)) finite = 0;
    if (n_used < 3) { s->status = VO_REFINE_TOO_FEW; s->done = 1; }
    else if (!finite) { s->status = VO_REFINE_DEGENERATE; s->done = 1; }
    VO_UNROLL
    for (int i = 0; i < 21; ++i) s->H[i] = sums[i];
    VO_UNROLL
    for (int i = 0; i < 6; ++i) s->g[i] = sums[21 + i];
}

VO_HD int vo_refine_propose(vo_refine_state* s, int max_iterations)
{
    if (s->done) return 0;
    if (s->passes >= max_iterations) { s->status = VO_REFINE_MAX_ITER; s->done = 1; return 0; }
    for (;;) {
        if (s->lambda > VO_REFINE_LAMBDA_MAX) { s->status = VO_REFINE_DAMPING; s->done = 1; return 0; }
        double d[6];
        if (vo_refine_solve(s->H, s->g, s->lambda, d)) {
            vo_refine_retract(s->R, s->t, d, s->Rc, s->tc);
            return 1;
        }
        s->lambda = s->lambda * 10.0;
    }
}

VO_HD void vo_refine_update(vo_refine_state* s, const double* sums, int behind, double relative_tolerance,
                            double absolute_tolerance)
{
    s->passes = s->passes + 1;
    double cn = sums[27];
    if (!behind && cn < s->c) {
        double drop = s->c - cn;
        int conv = (drop <= relative_tolerance * s->c) || (cn <= absolute_tolerance * (double)s->n_used);
        VO_UNROLL
        for (int i = 0; i < 9; ++i) s->R[i] = s->Rc[i];
        VO_UNROLL
        for (int i = 0; i < 3; ++i) s->t[i] = s->tc[i];
        VO_UNROLL
        for (int i = 0; i < 21; ++i) s->H[i] = sums[i];
        VO_UNROLL
        for (int i = 0; i < 6; ++i) s->g[i] = sums[21 + i];
        s->c = cn;
        s->accepted = s->accepted + 1;
        double l = s->lambda / 10.0;
        s->lambda = l > VO_REFINE_LAMBDA_MIN ? l : VO_REFINE_LAMBDA_MIN;
        if (conv) { s->status = VO_REFINE_CONVERGED; s->done = 1; }
    } else {
        s->lambda = s->lambda * 10.0;
    }
}

/* ------------------------------------------------------------------------ */
/* matchFeaturesInRadius: the spatial gate of one (F1 row, F2 column) pair    */
/* and its lower bound over a box of positions.  (x2, y2) is the column's     */
/* point, (cx, cy) the row's centre, r2 = r * r the row's squared radius.     */
/* f32 basic ops in the order written, no contraction: two subtractions, two  */
/* multiplies, one add.  The circle is closed (d2 == r2 is inside); r2 = +inf */
/* (a radius whose square overflows) admits every column.                     */
/* ------------------------------------------------------------------------ */
VO_HD float vo_radius_d2(float x2, float y2, float cx, float cy)
{
    float dx = x2 - cx;
    float dy = y2 - cy;
    float sx = dx * dx;
    float sy = dy * dy;
    return sx + sy;
}

VO_HD int vo_radius_gate(float x2, float y2, float cx, float cy, float r2) { return vo_radius_d2(x2, y2, cx, cy) <= r2; }

/* Lower bound of vo_radius_d2 between the point (px, py) and every point q   */
/* of the box [xmin, xmax] x [ymin, ymax], whichever of the two is the centre */
/* (the forward pass bounds a tile of F2 points against the row's centre, the */
/* backward pass a tile of centres against the row's point).  It holds in     */
/* float32, not only in real arithmetic: for px < xmin <= qx, round-to-       */
/* nearest subtraction is monotone, so fl(xmin - px) <= fl(qx - px); for      */
/* px > xmax >= qx likewise fl(px - xmax) <= fl(px - qx); fl(a - b) =         */
/* -fl(b - a), so either is <= |dx| as vo_radius_d2 computes it whichever     */
/* operand comes first; inside the interval the bound is 0.  Multiply and add */
/* are monotone on non-negatives, so bx * bx + by * by <= dx * dx + dy * dy.  */
/* ------------------------------------------------------------------------ */
VO_HD float vo_radius_box_lb(float xmin, float xmax, float ymin, float ymax, float px, float py)
{
    float bx = fmaxf(fmaxf(xmin - px, px - xmax), 0.0f);
    float by = fmaxf(fmaxf(ymin - py, py - ymax), 0.0f);
    float sx = bx * bx;
    float sy = by * by;
    return sx + sy;
}

/* ------------------------------------------------------------------------ */
/* estimateFundamentalMatrix: normalised 8-point fit, Sampson distance and   */
/* the MSAC loop's pieces.  One definition for the kernel (k_fund_msac,      */
/* geom.hip) and the CPU reference (tests/fund_ref), equal by bytes: f64     */
/* only, + - * / and sqrt in the order written, no contraction, no libm      */
/* (vo_log_d for the trial bound).  Convention: [x2 1] F [x1 1]' = 0, F 3x3  */
/* row-major; points are single 1-based pixels widened to double.            */
/*                                                                           */
/* Work arrays (the 9x9 problem's 45 + 81 doubles) are addressed with a      */
/* stride: element e of an array lives at a[e * stride].  The reference      */
/* passes 1; the kernel keeps a chunk's hypotheses in LDS, element-major      */
/* across the chunk's slots (stride = slots), so lanes on neighbouring slots */
/* touch neighbouring banks.  The stride moves values, it computes nothing.  */
/* ------------------------------------------------------------------------ */
#define VO_FUND_SAMPLE 8
#define VO_FUND_ATTEMPTS 16          /* draws of 8 indices before a slot is invalid */
#define VO_FUND_NSUM 45              /* upper triangle of A'A, row-major */
#define VO_FUND_NWORK (45 + 81)      /* ... and the eigenvector matrix */
#define VO_FUND_LANES 64             /* partial sums of a masked fit: partial l adds the used points k = l (mod 64); joined by vo_tree_sum */
#define VO_FUND_SWEEP_CAP 30         /* cyclic Jacobi sweeps, at most */
#define VO_FUND_SKIP_EPS 1.1102230246251565e-16   /* 2^-53: a_pq is negligible beside |a_pp| + |a_qq| */
#define VO_FUND_SQRT2 1.4142135623730951
#define VO_FUND_TAG0 0xF8A70000u     /* Philox counter word 3 of the two draws (k_msac's is 0x5EED) */
#define VO_FUND_TAG1 0xF8A70001u
#define VO_FUND_NO_BOUND 0x7fffffff

/* index of (i, j), i <= j, in the row-major upper triangle of an n x n symmetric matrix */
VO_HD int vo_fund_tri(int n, int i, int j) { return i * n - (i * (i - 1)) / 2 + (j - i); }

VO_HD int vo_fund_finite(double v) { return v - v == 0.0; }

/* One rotation's parameters from (a_pp, a_qq, a_pq).  Returns 1 (skip: nothing is written) iff
 * |a_pq| <= 2^-53 (|a_pp| + |a_qq|) (a NaN is never skipped); otherwise
 *   theta = (a_qq - a_pp) / (2 a_pq),  t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)),  sgn(0) = 1,
 *   c = 1 / sqrt(t^2 + 1),  s = t c. */
VO_HD int vo_fund_rot(double app, double aqq, double apq, double* t, double* c, double* s)
{
    if (fabs(apq) <= VO_FUND_SKIP_EPS * (fabs(app) + fabs(aqq))) return 1;
    const double theta = (aqq - app) / (2.0 * apq);
    const double den = fabs(theta) + sqrt(theta * theta + 1.0);
    const double tt = (theta < 0.0 ? -1.0 : 1.0) / den;
    const double cc = 1.0 / sqrt(tt * tt + 1.0);
    *t = tt; *c = cc; *s = tt * cc;
    return 0;
}

/* (x, y) <- (c x - s y, s x + c y): what a rotation does to (a_kp, a_kq), k != p, q, and to (v_kp, v_kq), every k */
VO_HD void vo_fund_rot_xy(double c, double s, double* x, double* y)
{
    const double x0 = *x, y0 = *y;
    *x = c * x0 - s * y0;
    *y = s * x0 + c * y0;
}

/* index of the smallest diagonal entry of A (ties: the lowest; a NaN never wins) */
VO_HD int vo_fund_argmin_diag(const double* A, int n, int stride)
{
    int jmin = 0;
    double dmin = A[0];
    for (int j = 1; j < n; ++j) {
        const double d = A[vo_fund_tri(n, j, j) * stride];
        if (d < dmin || (dmin != dmin && d == d)) { dmin = d; jmin = j; }
    }
    return jmin;
}

/* Cyclic two-sided Jacobi on the symmetric n x n matrix A (upper triangle, vo_fund_tri) with the
 * eigenvector matrix V (n x n row-major, set to the identity here) carried along.  Pairs (p, q),
 * p < q, row-major; each pair is vo_fund_rot on (a_pp, a_qq, a_pq), then, unless skipped,
 *   a_pp -= t a_pq,  a_qq += t a_pq,  a_pq = 0,  and vo_fund_rot_xy on every (a_kp, a_kq), (v_kp, v_kq).
 * The element updates of one rotation are independent of one another, so their order (and who
 * performs them: the kernel spreads them over a group of lanes) does not change a bit.
 * The loop ends after the first sweep that rotates nothing, or after VO_FUND_SWEEP_CAP sweeps.
 * Returns the index of the smallest diagonal entry (vo_fund_argmin_diag), whose eigenvector is
 * column j of V: V[k * n + j].  *sweeps_out (may be NULL) counts the sweeps run. */
VO_HD int vo_fund_jacobi(double* A, double* V, int n, int stride, int* sweeps_out)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[(i * n + j) * stride] = i == j ? 1.0 : 0.0;
    int sweeps = 0;
    for (; sweeps < VO_FUND_SWEEP_CAP;) {
        int rotated = 0;
        for (int p = 0; p < n - 1; ++p) {
            for (int q = p + 1; q < n; ++q) {
                const int ipp = vo_fund_tri(n, p, p) * stride, iqq = vo_fund_tri(n, q, q) * stride;
                const int ipq = vo_fund_tri(n, p, q) * stride;
                const double apq = A[ipq], app = A[ipp], aqq = A[iqq];
                double t, c, s;
                if (vo_fund_rot(app, aqq, apq, &t, &c, &s)) continue;
                rotated = 1;
                A[ipp] = app - t * apq;
                A[iqq] = aqq + t * apq;
                A[ipq] = 0.0;
                for (int k = 0; k < n; ++k) {
                    if (k == p || k == q) continue;
                    const int ikp = (k < p ? vo_fund_tri(n, k, p) : vo_fund_tri(n, p, k)) * stride;
                    const int ikq = (k < q ? vo_fund_tri(n, k, q) : vo_fund_tri(n, q, k)) * stride;
                    double x = A[ikp], y = A[ikq];
                    vo_fund_rot_xy(c, s, &x, &y);
                    A[ikp] = x;
                    A[ikq] = y;
                }
                for (int k = 0; k < n; ++k) {
                    const int ikp = (k * n + p) * stride, ikq = (k * n + q) * stride;
                    double x = V[ikp], y = V[ikq];
                    vo_fund_rot_xy(c, s, &x, &y);
                    V[ikp] = x;
                    V[ikq] = y;
                }
            }
        }
        ++sweeps;
        if (!rotated) break;
    }
    if (sweeps_out) *sweeps_out = sweeps;
    return vo_fund_argmin_diag(A, n, stride);
}

/* One image's normalisation from its sums: centroid c = sum / m, then (second call) the scale
 * s = sqrt(2) / (dsum / m).  T = [s 0 -s cx; 0 s -s cy; 0 0 1] is kept as N = (s, cx, cy). */
VO_HD double vo_fund_dist(double x, double y, double cx, double cy)
{
    double dx = x - cx, dy = y - cy;
    return sqrt(dx * dx + dy * dy);
}

/* the 45 products of one normalised pair's design row, added to acc[q * stride] (upper triangle, row-major):
 * a = s1 (x1 - c1), b = s2 (x2 - c2), row = [bx ax, bx ay, bx, by ax, by ay, by, ax, ay, 1] */
VO_HD void vo_fund_row(const double* N1, const double* N2, double x1, double y1, double x2, double y2, double* acc, int stride)
{
    double ax = N1[0] * (x1 - N1[1]), ay = N1[0] * (y1 - N1[2]);
    double bx = N2[0] * (x2 - N2[1]), by = N2[0] * (y2 - N2[2]);
    double r[9];
    r[0] = bx * ax; r[1] = bx * ay; r[2] = bx; r[3] = by * ax; r[4] = by * ay; r[5] = by; r[6] = ax; r[7] = ay; r[8] = 1.0;
    int q = 0;
    VO_UNROLL
    for (int i = 0; i < 9; ++i) {
        VO_UNROLL
        for (int j = i; j < 9; ++j) {
            acc[q * stride] = acc[q * stride] + r[i] * r[j];
            ++q;
        }
    }
}

/* A sample's fit: the 8 points idx[0..7] of x1 / x2 ([n][2] single) summed sequentially in sample
 * order from +0, in three passes (centroids, mean distances, the 45 sums).  Writes N1, N2 and
 * M[q * stride]; returns 0 (no model) when either scale is not finite. */
VO_HD int vo_fund_fit_sample(const float* x1, const float* x2, const uint32_t* idx, double* N1, double* N2, double* M, int stride)
{
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    VO_UNROLL
    for (int k = 0; k < VO_FUND_SAMPLE; ++k) {
        s[0] = s[0] + (double)x1[2 * idx[k]]; s[1] = s[1] + (double)x1[2 * idx[k] + 1];
        s[2] = s[2] + (double)x2[2 * idx[k]]; s[3] = s[3] + (double)x2[2 * idx[k] + 1];
    }
    const double m = (double)VO_FUND_SAMPLE;
    N1[1] = s[0] / m; N1[2] = s[1] / m; N2[1] = s[2] / m; N2[2] = s[3] / m;
    double d1 = 0.0, d2 = 0.0;
    VO_UNROLL
    for (int k = 0; k < VO_FUND_SAMPLE; ++k) {
        d1 = d1 + vo_fund_dist((double)x1[2 * idx[k]], (double)x1[2 * idx[k] + 1], N1[1], N1[2]);
        d2 = d2 + vo_fund_dist((double)x2[2 * idx[k]], (double)x2[2 * idx[k] + 1], N2[1], N2[2]);
    }
    N1[0] = VO_FUND_SQRT2 / (d1 / m);
    N2[0] = VO_FUND_SQRT2 / (d2 / m);
    if (!vo_fund_finite(N1[0]) || !vo_fund_finite(N2[0])) return 0;
    for (int q = 0; q < VO_FUND_NSUM; ++q) M[q * stride] = 0.0;
    for (int k = 0; k < VO_FUND_SAMPLE; ++k)
        vo_fund_row(N1, N2, (double)x1[2 * idx[k]], (double)x1[2 * idx[k] + 1], (double)x2[2 * idx[k]], (double)x2[2 * idx[k] + 1], M,
                    stride);
    return 1;
}

/* From M (W[0..44]) and the two normalisations to F: the null vector of M (Jacobi at 9x9, V in
 * W[45..125]), rank 2 by v = the smallest eigenvector of Fh' Fh (Jacobi at 3x3, in W[0..5] and
 * W[45..53], which the 9x9 problem no longer needs) and F' = Fh - (Fh v) v', then F = T2' F' T1,
 * divided by its Frobenius norm (squares summed in index order) and negated if F[8] < 0.
 * Returns 0 (no model, F untouched) when a value of F is not finite.  sweeps (may be NULL): the
 * two Jacobi calls' sweep counts. */
VO_HD int vo_fund_solve_tail(double* W, int stride, int j9, const double* N1, const double* N2, double* F, int* sweeps);

VO_HD int vo_fund_solve(double* W, int stride, const double* N1, const double* N2, double* F, int* sweeps)
{
    const int j9 = vo_fund_jacobi(W, W + VO_FUND_NSUM * stride, 9, stride, sweeps);
    return vo_fund_solve_tail(W, stride, j9, N1, N2, F, sweeps);
}

/* vo_fund_solve after its 9x9 Jacobi, whose result is column j9 of V */
VO_HD int vo_fund_solve_tail(double* W, int stride, int j9, const double* N1, const double* N2, double* F, int* sweeps)
{
    double* V = W + VO_FUND_NSUM * stride;
    double Fh[9];
    VO_UNROLL
    for (int k = 0; k < 9; ++k) Fh[k] = V[(k * 9 + j9) * stride];
    VO_UNROLL
    for (int i = 0; i < 3; ++i) {
        VO_UNROLL
        for (int j = i; j < 3; ++j)
            W[vo_fund_tri(3, i, j) * stride] = (Fh[i] * Fh[j] + Fh[3 + i] * Fh[3 + j]) + Fh[6 + i] * Fh[6 + j];
    }
    const int j3 = vo_fund_jacobi(W, V, 3, stride, sweeps ? sweeps + 1 : sweeps);
    double v[3], Fv[3], G[9], H[9];
    VO_UNROLL
    for (int k = 0; k < 3; ++k) v[k] = V[(k * 3 + j3) * stride];
    VO_UNROLL
    for (int i = 0; i < 3; ++i) Fv[i] = (Fh[3 * i] * v[0] + Fh[3 * i + 1] * v[1]) + Fh[3 * i + 2] * v[2];
    VO_UNROLL
    for (int i = 0; i < 3; ++i) {
        VO_UNROLL
        for (int j = 0; j < 3; ++j) G[3 * i + j] = Fh[3 * i + j] - Fv[i] * v[j];
    }
    const double s1 = N1[0], ox1 = -(N1[0] * N1[1]), oy1 = -(N1[0] * N1[2]);
    const double s2 = N2[0], ox2 = -(N2[0] * N2[1]), oy2 = -(N2[0] * N2[2]);
    VO_UNROLL
    for (int i = 0; i < 3; ++i) {                     /* H = F' T1 */
        H[3 * i] = G[3 * i] * s1;
        H[3 * i + 1] = G[3 * i + 1] * s1;
        H[3 * i + 2] = (G[3 * i] * ox1 + G[3 * i + 1] * oy1) + G[3 * i + 2];
    }
    VO_UNROLL
    for (int j = 0; j < 3; ++j) {                     /* G = T2' H */
        G[j] = s2 * H[j];
        G[3 + j] = s2 * H[3 + j];
        G[6 + j] = (ox2 * H[j] + oy2 * H[3 + j]) + H[6 + j];
    }
    double nn = 0.0;
    VO_UNROLL
    for (int k = 0; k < 9; ++k) nn = nn + G[k] * G[k];
    nn = sqrt(nn);
    int ok = 1;
    VO_UNROLL
    for (int k = 0; k < 9; ++k) {
        G[k] = G[k] / nn;
        if (!vo_fund_finite(G[k])) ok = 0;
    }
    if (!ok) return 0;
    const int neg = G[8] < 0.0;
    VO_UNROLL
    for (int k = 0; k < 9; ++k) F[k] = neg ? -G[k] : G[k];
    return 1;
}

/* Sampson distance of one pair (px^2): r^2 / ((F x1)_0^2 + (F x1)_1^2 + (F' x2)_0^2 + (F' x2)_1^2),
 * r = x2' F x1.  0 / 0 is NaN, which fails every comparison (no inlier, scored as the threshold). */
VO_HD double vo_fund_sampson(const double* F, double x1, double y1, double x2, double y2)
{
    double l0 = (F[0] * x1 + F[1] * y1) + F[2];
    double l1 = (F[3] * x1 + F[4] * y1) + F[5];
    double l2 = (F[6] * x1 + F[7] * y1) + F[8];
    double r = (x2 * l0 + y2 * l1) + l2;
    double m0 = (F[0] * x2 + F[3] * y2) + F[6];
    double m1 = (F[1] * x2 + F[4] * y2) + F[7];
    double den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
    return (r * r) / den;
}

/* Slot `slot` of the problem with key `key`: up to 16 attempts, each 8 indices from two Philox
 * calls (counter {slot, attempt, key, TAG0 / TAG1}, key words {seed, 0x9E3779B9}); the first
 * attempt whose 8 indices are distinct is the sample.  Returns 0 when all 16 fail (n < 8 always
 * does); *attempts (may be NULL) gets the attempts used. */
VO_HD int vo_fund_sample(uint32_t seed, uint32_t key, uint32_t slot, uint32_t n, uint32_t* idx, int* attempts)
{
    int ok = 0;
    uint32_t att = 0;
    for (; att < VO_FUND_ATTEMPTS && !ok; ++att) {
        vo_u32x4 c0 = {{slot, att, key, VO_FUND_TAG0}};
        vo_u32x4 c1 = {{slot, att, key, VO_FUND_TAG1}};
        vo_u32x4 r0 = vo_philox4x32_10(c0, seed, 0x9E3779B9u);
        vo_u32x4 r1 = vo_philox4x32_10(c1, seed, 0x9E3779B9u);
        VO_UNROLL
        for (int q = 0; q < 4; ++q) { idx[q] = vo_rand_index(r0.v[q], n); idx[4 + q] = vo_rand_index(r1.v[q], n); }
        ok = 1;
        VO_UNROLL
        for (int i = 0; i < VO_FUND_SAMPLE; ++i) {
            VO_UNROLL
            for (int j = i + 1; j < VO_FUND_SAMPLE; ++j)
                if (idx[i] == idx[j]) ok = 0;
        }
    }
    if (attempts) *attempts = (int)att;
    return ok;
}

/* Trials after which a sample of 8 inliers was drawn with probability conf (a fraction), at the
 * inlier ratio w = n_in / n: ceil(log(1 - conf) / log(1 - w^8)), w^8 = ((w w)^2)^2.  w^8 >= 1 gives
 * 1; log(1 - w^8) == 0 (w^8 below half an ulp of 1, w < 0.01) gives VO_FUND_NO_BOUND: no inlier
 * ratio that small ends the loop early. */
VO_HD int vo_fund_trials_needed(int n_in, int n, double conf)
{
    double w = (double)n_in / (double)n;
    double w2 = w * w;
    double w4 = w2 * w2;
    double w8 = w4 * w4;
    if (w8 >= 1.0) return 1;
    double den = vo_log_d(1.0 - w8);
    if (den == 0.0) return VO_FUND_NO_BOUND;
    double N = ceil(vo_log_d(1.0 - conf) / den);
    if (N > 2147483647.0) return VO_FUND_NO_BOUND;
    if (N < 1.0) return 1;
    return (int)N;
}

/* The sequential MSAC loop, replayed slot by slot in slot order over (valid, score, n_in):
 *     vo_fund_replay_begin(&r, num_trials);
 *     for slot = 0 .. num_trials - 1, while !vo_fund_replay_done(&r):  vo_fund_replay_slot(...)
 * An invalid slot (no 8 distinct indices, or a sample without a model) counts as no trial.  A valid
 * one counts, and replaces the best iff its score is strictly smaller; the bound is then
 * min(bound, vo_fund_trials_needed).  Done once trials >= bound.  Returns 1 when the slot became
 * the best (the caller keeps its F). */
typedef struct { int bound, trials, best, best_in; double best_score; } vo_fund_replay;

VO_HD void vo_fund_replay_begin(vo_fund_replay* r, int num_trials)
{
    r->bound = num_trials; r->trials = 0; r->best = -1; r->best_in = 0;
    r->best_score = vo_u64_as_f64(0x7ff0000000000000ULL);
}

VO_HD int vo_fund_replay_done(const vo_fund_replay* r) { return r->trials >= r->bound; }

VO_HD int vo_fund_replay_slot(vo_fund_replay* r, int slot, int valid, double score, int n_in, int n, double conf)
{
    if (!valid) return 0;
    r->trials = r->trials + 1;
    if (!(score < r->best_score)) return 0;
    r->best_score = score; r->best = slot; r->best_in = n_in;
    int need = vo_fund_trials_needed(n_in, n, conf);
    if (need < r->bound) r->bound = need;
    return 1;
}

/* ------------------------------------------------------------------------ */
/* vision.PointTracker: pyramidal Lucas-Kanade in fixed point (the algorithm */
/* of OpenCV 4.x calcOpticalFlowPyrLK, restated).  Shared by   */
/* k_klt_pyr / k_klt_track and the CPU reference (tests/klt_ref).            */
/*                                                                           */
/* Pyramid: u8; level l + 1 has (rows_l + 1) / 2 x (cols_l + 1) / 2 pixels,   */
/* each the 5 x 5 binomial w_i w_j, w = 1 4 6 4 1 (the 25 weights add to 256), */
/* of level l under reflect-101, (sum + 128) >> 8 (vo_klt_pyr_pixel).         */
/* Reads while tracking clamp the pixel index to the level (replicate).      */
/*                                                                           */
/* Bounds (what the kernel's packing relies on).  A pixel is 0 .. 255.  The   */
/* three rounded weights w00, w01, w10 are >= 0 and their exact sum           */
/* (1 - ab) 16384 is <= 16384, so rounding each to nearest makes their sum    */
/* at most 16385: w11 = 16384 - w00 - w01 - w10 >= -1, and the four weights   */
/* add to 16384 by construction.                                              */
/*  - I = bil(pixel, 9): the sum lies in [-255, 255 * 16385], so              */
/*    I in [(-255 + 256) >> 9, (255 * 16385 + 256) >> 9] = [0, 8160]; the same */
/*    for the second image's sample, hence |diff| <= 8160.                    */
/*  - |gx|, |gy| <= (3 + 10 + 3) * 255 = 4080, so with w11 >= 0 (all but the  */
/*    one-ulp case above) |Ix| <= (4080 * 16384 + 8192) >> 14 = 4080; with     */
/*    w11 = -1 the a-priori bound is (4080 * 16386 + 8192) >> 14 = 4081.  I,   */
/*    Ix, Iy fit int16 either way.                                            */
/*  - a lane's partial over 16 samples: |diff Ix| <= 8160 * 4081 = 33300960,  */
/*    x 16 = 532815360 < 2^31; Ix^2 <= 16654561, x 16 < 2^28; diff^2 <=        */
/*    66585600, x 16 = 1065369600 < 2^31.  int32 holds every partial.         */
/*  - a 31 x 31 window: 961 * 33300960 = 3.2e10 > 2^31: window sums are int64. */
/* Every window sum is therefore an exact integer and its order is free; the  */
/* float part below is f32 basic operations in the order written.             */
/* ------------------------------------------------------------------------ */
#define VO_KLT_OK 0
#define VO_KLT_TEMPLATE_OUT 1
#define VO_KLT_LOST 2
#define VO_KLT_FLAT 3
#define VO_KLT_BIDIR 4
#define VO_KLT_STOP_NONE 0
#define VO_KLT_STOP_EPS 1
#define VO_KLT_STOP_OSC 2
#define VO_KLT_STOP_MAXIT 3
#define VO_KLT_MAX_LEVELS 6
#define VO_KLT_MIN_WIN 5
#define VO_KLT_MAX_WIN 31
#define VO_KLT_MAX_ITER 50
#define VO_KLT_LANE_SAMPLES 16                /* ceil(961 / 64): samples s = lane + 64 k, k < 16 */
#define VO_KLT_W_ONE 16384
#define VO_KLT_FS 9.5367431640625e-07f        /* 2^-20 */
#define VO_KLT_MIN_EIG 1e-4f
#define VO_KLT_EPS2 1e-4f                     /* (0.01 px)^2 */
#define VO_KLT_OSC 0.01f
#define VO_KLT_SCORE_DEN 8160.0f              /* 255 * 32 */

/* sizes of level l (l >= 0) of a rows x cols image */
VO_HD int vo_klt_level_dim(int n, int l)
{
    for (int k = 0; k < l; ++k) n = (n + 1) / 2;
    return n;
}

/* pixel (r, c) of level l + 1 from level l (src, rows x cols, row stride ld) */
VO_HD int vo_klt_pyr_pixel(const uint8_t* src, int rows, int cols, int ld, int r, int c)
{
    const int w[5] = {1, 4, 6, 4, 1};
    int sum = 0;
    VO_UNROLL
    for (int i = -2; i <= 2; ++i) {
        const uint8_t* row = src + (long)vo_reflect101(2 * r + i, rows) * ld;
        int h = 0;
        VO_UNROLL
        for (int j = -2; j <= 2; ++j) h += w[j + 2] * (int)row[vo_reflect101(2 * c + j, cols)];
        sum += w[i + 2] * h;
    }
    return (sum + 128) >> 8;
}

VO_HD int vo_klt_scharr(int a0, int a1, int b0, int b1, int c0, int c1)   /* 3 (a1 - a0) + 10 (b1 - b0) + 3 (c1 - c0) */
{
    return 3 * (a1 - a0) + 10 * (b1 - b0) + 3 * (c1 - c0);
}

/* Window corner q -> 1 and (ix, iy, w[4] = w00 w01 w10 w11), or 0 when the corner is out:
 * i.x < -bw || i.x >= cols || i.y < -bh || i.y >= rows.  The test is made on floorf's float (the
 * same outcome as on the integer wherever the integer exists; a corner too far for an int, or a
 * NaN, is out), so no conversion overflows. */
VO_HD int vo_klt_corner(float qx, float qy, int bw, int bh, int rows, int cols, int* ix, int* iy, int* w)
{
    const float fx = floorf(qx), fy = floorf(qy);
    if (!(fx >= (float)(-bw) && fx < (float)cols && fy >= (float)(-bh) && fy < (float)rows)) return 0;
    const float a = qx - fx, b = qy - fy;
    *ix = (int)fx; *iy = (int)fy;
    w[0] = (int)rintf((1.0f - a) * (1.0f - b) * 16384.0f);
    w[1] = (int)rintf(a * (1.0f - b) * 16384.0f);
    w[2] = (int)rintf((1.0f - a) * b * 16384.0f);
    w[3] = VO_KLT_W_ONE - w[0] - w[1] - w[2];
    return 1;
}

VO_HD int vo_klt_bil(int f00, int f01, int f10, int f11, const int* w, int n)
{
    return (f00 * w[0] + f01 * w[1] + f10 * w[2] + f11 * w[3] + (1 << (n - 1))) >> n;
}

/* the template's sums -> 1 and (A11, A12, A22, 1 / D), or 0: flat */
VO_HD int vo_klt_gradient_matrix(int64_t sxx, int64_t sxy, int64_t syy, int bw, int bh, float* A)
{
    const float A11 = (float)sxx * VO_KLT_FS, A12 = (float)sxy * VO_KLT_FS, A22 = (float)syy * VO_KLT_FS;
    const float D = A11 * A22 - A12 * A12;
    const float d = A11 - A22;
    const float minEig = (A22 + A11 - sqrtf(d * d + 4.0f * A12 * A12)) / (float)(2 * bw * bh);
    if (minEig < VO_KLT_MIN_EIG || D < VO_FLT_EPSILON) return 0;
    A[0] = A11; A[1] = A12; A[2] = A22; A[3] = 1.0f / D;
    return 1;
}

/* one iteration's sums -> delta */
VO_HD void vo_klt_delta(const float* A, int64_t s1, int64_t s2, float* dx, float* dy)
{
    const float b1 = (float)s1 * VO_KLT_FS, b2 = (float)s2 * VO_KLT_FS;
    *dx = (A[1] * b2 - A[2] * b1) * A[3];
    *dy = (A[1] * b1 - A[0] * b2) * A[3];
}

/* After q += delta, next = q + h: the stop of iteration j (prev: the delta of iteration j - 1).
 * OSC moves next back by half the step. */
VO_HD int vo_klt_stop(int j, float dx, float dy, float pdx, float pdy, float* nx, float* ny)
{
    if (dx * dx + dy * dy <= VO_KLT_EPS2) return VO_KLT_STOP_EPS;
    if (j > 0 && fabsf(dx + pdx) < VO_KLT_OSC && fabsf(dy + pdy) < VO_KLT_OSC) {
        *nx = *nx - 0.5f * dx; *ny = *ny - 0.5f * dy;
        return VO_KLT_STOP_OSC;
    }
    return VO_KLT_STOP_NONE;
}

VO_HD float vo_klt_score(int64_t s2, int bw, int bh)
{
    return 1.0f - sqrtf((float)s2 / (float)(bw * bh)) / VO_KLT_SCORE_DEN;
}

/* after level 0: inside [0, cols - 1] x [0, rows - 1] (a NaN is outside) */
VO_HD int vo_klt_inside(float x, float y, int rows, int cols)
{
    return x >= 0.0f && x <= (float)(cols - 1) && y >= 0.0f && y <= (float)(rows - 1);
}

VO_HD float vo_klt_bidir_error(float x, float y, float x0, float y0)
{
    const float dx = x - x0, dy = y - y0;
    return sqrtf(dx * dx + dy * dy);
}

/* ------------------------------------------------------------------------ */
/* detectMinEigenFeatures / detectHarrisFeatures: cornerPoints. */
/* Shared by k_corner_metric / k_corner_count / k_corner_emit / k_corner_rank */
/* and the CPU reference (tests/corner_ref).  Integers up to the response,    */
/* then f64 basic operations and sqrt in the order written.                   */
/*                                                                           */
/* Image u8, every read clamped to the image.  Ix(r, c) = p(r, c + 1) -       */
/* p(r, c - 1), Iy(r, c) = p(r + 1, c) - p(r - 1, c), both in [-255, 255]; the */
/* products Ix^2, Iy^2, Ix Iy have magnitude <= 255^2 = 65025.  A product at   */
/* an index outside the image is the product at the clamped index.            */
/*                                                                           */
/* Window: f x f (odd, 3 .. 15), separable, integer weights q_k >= 0 of       */
/* vo_corner_weights that add to 4096 exactly.                                */
/*  - horizontal pass h = sum_j q_j prod: |h| <= (sum_j q_j) 65025 =          */
/*    4096 * 65025 = 266342400 < 2^31 = 2147483648: int32 holds it and every  */
/*    partial sum (all q_j >= 0, so partial sums of |q_j prod| only grow);    */
/*  - vertical pass v = sum_i q_i h: |v| <= 4096 * 266342400 = 1090938470400 */
/*    < 2^41 = 2199023255552: int64, and exact as a double (< 2^53).          */
/* A, B, C = v of Ix^2, Iy^2, Ix Iy: the exact 2-D sums scaled by 2^24, so the */
/* order of either sum is free.                                               */
/* ------------------------------------------------------------------------ */
#define VO_CORNER_MINEIG 0
#define VO_CORNER_HARRIS 1
#define VO_CORNER_MIN_FILTER 3
#define VO_CORNER_MAX_FILTER 15
#define VO_CORNER_W_ONE 4096
#define VO_CORNER_HARRIS_K 0.04
#define VO_CORNER_S (5.9604644775390625e-08 / 65025.0)   /* 2^-24 / 255^2: the units of a [0, 1] image */

/* the f 1-D weights: q_k = rint(4096 w_k / sum w), w_k = exp(-k^2 / (2 sigma^2)), sigma = f / 3, in
 * host double, then the centre takes what is missing from 4096.  Host only (libvo's entry and the
 * reference call it; the kernels get the integers). */
static inline void vo_corner_weights(int f, int* q)
{
    const int R = (f - 1) / 2;
    const double sigma = (double)f / 3.0;
    double w[VO_CORNER_MAX_FILTER], sum = 0.0;
    int total = 0;
    for (int k = -R; k <= R; ++k) { w[k + R] = exp(-(double)(k * k) / (2.0 * sigma * sigma)); sum += w[k + R]; }
    for (int k = 0; k < f; ++k) { q[k] = (int)rint(4096.0 * w[k] / sum); total += q[k]; }
    q[R] += VO_CORNER_W_ONE - total;
}

VO_HD int vo_corner_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

/* the response of the smoothed matrix [A C; C B] (scaled by 2^24 * 65025) */
VO_HD float vo_corner_response(int method, int64_t A, int64_t B, int64_t C)
{
    const double a = (double)A, b = (double)B, c = (double)C, S = VO_CORNER_S;
    if (method == VO_CORNER_HARRIS) {
        const double tr = a + b;
        return (float)((((a * b) - (c * c)) - VO_CORNER_HARRIS_K * (tr * tr)) * (S * S));
    }
    const double d = a - b;
    return (float)((0.5 * ((a + b) - sqrt(d * d + 4.0 * (c * c)))) * S);
}

/* the ROI's maximum is taken from 0: a metric that is not positive does not count */
VO_HD uint32_t vo_corner_max_bits(float m) { return m > 0.0f ? vo_f32_as_u32(m) : 0u; }

/* pixel (r, c) of the tightly packed metric plane m: above the threshold (thr = min_quality * mmax, mmax
 * > 0 checked by the caller) and a local maximum of its 8 neighbours inside the image -- strictly above
 * those that precede it in row-major order, not below those that follow, so the first pixel of an equal
 * pair wins */
VO_HD int vo_corner_is_corner(const float* m, int rows, int cols, int r, int c, float thr)
{
    const float z = m[(long)r * cols + c];
    if (!(z > thr)) return 0;
    for (int dr = -1; dr <= 1; ++dr)
        for (int dc = -1; dc <= 1; ++dc) {
            const int rr = r + dr, cc = c + dc;
            if ((dr == 0 && dc == 0) || rr < 0 || rr >= rows || cc < 0 || cc >= cols) continue;
            const float n = m[(long)rr * cols + cc];
            const int before = dr < 0 || (dr == 0 && dc < 0);
            if (before ? !(z > n) : !(z >= n)) return 0;
        }
    return 1;
}

/* sub-pixel offset along one axis from the metrics at -1, 0, +1 (f32, in this order) */
VO_HD float vo_corner_offset(float l, float z, float g)
{
    const float den = (l - z) + (g - z);
    float d = den < 0.0f ? 0.5f * (l - g) / den : 0.0f;
    if (d < -0.5f) d = -0.5f;
    if (d > 0.5f) d = 0.5f;
    return d;
}

/* Location (x, y), 1-based, of the corner at pixel (r, c); the offset of an axis with a neighbour
 * outside the image is 0 */
VO_HD void vo_corner_location(const float* m, int rows, int cols, int r, int c, float* x, float* y)
{
    const float z = m[(long)r * cols + c];
    const float dx = (c > 0 && c < cols - 1) ? vo_corner_offset(m[(long)r * cols + c - 1], z, m[(long)r * cols + c + 1]) : 0.0f;
    const float dy = (r > 0 && r < rows - 1) ? vo_corner_offset(m[(long)(r - 1) * cols + c], z, m[(long)(r + 1) * cols + c]) : 0.0f;
    *x = (float)(c + 1) + dx;
    *y = (float)(r + 1) + dy;
}

/* selectStrongest's key (vo_set_strongest's order): metric descending, then position in the raster-ordered
 * list ascending.  A corner's metric is positive, so its bits order as a u32. */
VO_HD uint64_t vo_corner_key(float metric, uint32_t index) { return (uint64_t)vo_f32_as_u32(metric) << 32 | (uint64_t)(~index); }

/* ------------------------------------------------------------------------ */
/* disparitySGM / reconstructScene: dense stereo depth.        */
/* Shared by k_sgm_census / k_sgm_paths / k_sgm_select / k_reconstruct and    */
/* the CPU reference (tests/sgm_ref).  Integers up to the sub-pixel offset    */
/* (one f32 division, one f32 addition); reconstructScene is f64 basic        */
/* operations in the order written.                                           */
/*                                                                           */
/* Disparities searched: d = dmin + k, k = 0 .. D - 1, D = dmax - dmin in     */
/* 8, 16, .. 128.  Census: 7 rows x 9 columns about the pixel under           */
/* replicate, one bit per neighbour in raster order, the centre left out,     */
/* 1 iff neighbour < centre: 62 bits.  C(y, x, k) = popcount(cL(y, x) ^       */
/* cR(y, clamp(x - (dmin + k)))) in 0 .. 62.  Eight paths r; at a path's      */
/* first pixel L_r = C, else with m = min_j L_r(p - r, j)                     */
/*   L_r(p, k) = C + min(L(k), L(k - 1) + P1, L(k + 1) + P1, m + P2) - m,     */
/* a neighbour outside 0 .. D - 1 absent.  By induction L_r <= 62 + P2 <=     */
/* 317 (the last argument bounds the minimum by P2 above m), so S = sum_r L_r */
/* <= 8 * 317 = 2536 fits a uint16_t and every intermediate an int.           */
/* ------------------------------------------------------------------------ */
#define VO_SGM_MAX_D 128
#ifndef VO_SGM_GROUP
#define VO_SGM_GROUP 8
#endif
#define VO_SGM_NDIR 8
#define VO_SGM_CENSUS_RY 3
#define VO_SGM_CENSUS_RX 4
#define VO_SGM_ABSENT 0x3fff      /* an absent neighbour: above every L + P */
#define VO_NAN_BITS 0x7fc00000u   /* the NaN both entries return */

VO_HD int vo_sgm_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

/* the direction r of path set q = 0 .. 7 as (dy, dx): q and q ^ 1 are opposite */
VO_HD void vo_sgm_dir(int q, int* dy, int* dx)
{
    const int s = (q & 1) ? -1 : 1;
    const int h = q >> 1;                      /* 0: along a row, 1: along a column, 2: diagonal, 3: anti-diagonal */
    *dy = h == 0 ? 0 : s;
    *dx = h == 0 ? s : (h == 1 ? 0 : (h == 2 ? s : -s));
}

/* the census word of pixel (y, x) of a tightly packed u8 image */
VO_HD uint64_t vo_sgm_census(const uint8_t* img, int rows, int cols, int y, int x)
{
    const int c = img[(long)y * cols + x];
    uint64_t w = 0;
    for (int dy = -VO_SGM_CENSUS_RY; dy <= VO_SGM_CENSUS_RY; ++dy)
        for (int dx = -VO_SGM_CENSUS_RX; dx <= VO_SGM_CENSUS_RX; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const int n = img[(long)vo_sgm_clamp(y + dy, rows) * cols + vo_sgm_clamp(x + dx, cols)];
            w = (w << 1) | (uint64_t)(n < c ? 1 : 0);
        }
    return w;
}

VO_HD int vo_sgm_popcount(uint64_t w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(w);
#else
    return __builtin_popcountll(w);
#endif
}

/* the right image's column that disparity d pairs with column x (clamped: the volume is total) */
VO_HD int vo_sgm_right_col(int x, int d, int cols) { return vo_sgm_clamp(x - d, cols); }

/* one step of a path at one disparity: c = C(p, k); lk, lm, lp = L_r(p - r, k), (k - 1), (k + 1), the last
 * two VO_SGM_ABSENT outside 0 .. D - 1; m = min_j L_r(p - r, j) */
VO_HD int vo_sgm_step(int c, int lk, int lm, int lp, int m, int P1, int P2)
{
    int best = lk;
    if (lm + P1 < best) best = lm + P1;
    if (lp + P1 < best) best = lp + P1;
    if (m + P2 < best) best = m + P2;
    return c + best - m;
}

/* the disparity of one pixel in column x from its D sums S: the winner (lowest k on ties), the uniqueness
 * test, the validity of the matched column, the sub-pixel offset.  NaN: unreliable or invalid. */
VO_HD float vo_sgm_select(const uint16_t* S, int D, int dmin, int x, int cols, int U)
{
    int ks = 0;
    uint32_t V = S[0];
    for (int k = 1; k < D; ++k) if (S[k] < V) { V = S[k]; ks = k; }
    uint32_t v = 0xffffu;
    for (int k = 0; k < D; ++k) if ((k < ks - 1 || k > ks + 1) && S[k] < v) v = S[k];
    const int d = dmin + ks, xr = x - d;
    if (100u * v < (100u + (uint32_t)U) * V) return vo_u32_as_f32(VO_NAN_BITS);
    if (xr < 0 || xr > cols - 1) return vo_u32_as_f32(VO_NAN_BITS);
    if (ks > 0 && ks < D - 1) {
        const int a = S[ks - 1], b = S[ks + 1];
        const int den = 2 * (a - 2 * (int)V + b);
        /* the lowest k wins a tie, so a > V strictly and den = 2 ((a - V) + (b - V)) > 0 at every interior winner:
         * the test never fails and the offset lies in (-0.5, +0.5]; it stands for the division's sake */
        if (den > 0) return (float)d + (float)(a - b) / (float)den;
    }
    return (float)d;
}

/* reconstructScene at pixel (x1, y1), 1-based, x = column; Q row-major 4 x 4 */
VO_HD void vo_reconstruct_point(const double* Q, int x1, int y1, float disp, float* xyz)
{
    if (disp != disp) { xyz[0] = xyz[1] = xyz[2] = vo_u32_as_f32(VO_NAN_BITS); return; }
    const double x = (double)x1, y = (double)y1, d = (double)disp;
    double h[4];
    for (int i = 0; i < 4; ++i) h[i] = ((Q[4 * i] * x + Q[4 * i + 1] * y) + Q[4 * i + 2] * d) + Q[4 * i + 3];
    for (int i = 0; i < 3; ++i) xyz[i] = (float)(h[i] / h[3]);
}

/* Q of a rectified pair from its 3 x 4 projection matrices (row-major), host only: 0, or -1 when the pair
 * is not of the form [fx 0 cx tx; 0 fy cy 0; 0 0 1 0] with P1's tx = 0, P2's tx != 0 and equal fx, fy, cy */
static inline int vo_reprojection_from_projections(const double* P1, const double* P2, double* Q)
{
    static const int zeros[7] = {1, 3, 4, 7, 8, 9, 11};
    for (int k = 0; k < 12; ++k) if (!(P1[k] == P1[k] && P2[k] == P2[k] && P1[k] - P1[k] == 0.0 && P2[k] - P2[k] == 0.0)) return -1;
    for (int k = 0; k < 7; ++k) {
        if (P1[zeros[k]] != 0.0) return -1;
        if (zeros[k] != 3 && P2[zeros[k]] != 0.0) return -1;
    }
    if (P2[3] == 0.0 || P1[10] != 1.0 || P2[10] != 1.0) return -1;
    if (P1[0] != P2[0] || P1[5] != P2[5] || P1[6] != P2[6] || P1[0] == 0.0 || P1[5] == 0.0) return -1;
    const double fx = P1[0], fy = P1[5], cy = P1[6], cx1 = P1[2], cx2 = P2[2];
    const double b = -P2[3] / P2[0], s = fx / fy;
    for (int k = 0; k < 16; ++k) Q[k] = 0.0;
    Q[0] = 1.0; Q[3] = -cx1;
    Q[5] = s; Q[7] = -s * cy;
    Q[11] = fx;
    Q[14] = 1.0 / b; Q[15] = -(cx1 - cx2) / b;
    return 0;
}

#endif /* VO_SPEC_H */
