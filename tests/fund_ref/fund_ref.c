/* CPU reference of vo_est_fundamental (test infrastructure): include/vo_spec.h's own vo_fund_*
 * functions -- the ones k_fund_msac calls -- around the normative loops: a masked fit's three
 * passes in 64 partials (partial l the used points k = l mod 64 ascending, joined by
 * vo_tree_sum), the score in the same 64 partials, and the sequential
 * MSAC loop slot by slot.  Compiled with the oracle's flags (no contraction, no fast-math).
 * x1, x2 [n][2] single 1-based pixels.  Status codes are include/vo.h's. */
#include <stdint.h>
#include <string.h>
#include "vo_spec.h"

#define FUND_OK 0
#define FUND_TOO_FEW -3
#define FUND_NO_CONSENSUS -4
#define FUND_NORM8 0
#define FUND_MSAC 1

/* census of one call (int32 each) */
enum {
    CN_TRIALS, CN_BOUND, CN_BEST, CN_SLOTS, CN_REATTEMPT, CN_NO_SAMPLE, CN_NO_MODEL, CN_NAN_DIST, CN_NO_BOUND, CN_SWEEPS9,
    CN_SWEEPS3, CN_IMPROVED, CN_TIES, CN_REFIT_MODEL, CN_COUNT
};

/* masked Norm8: mask NULL = all -> 1 and F, or 0 (no model) */
static int fit_masked(const float* x1, const float* x2, int n, const uint8_t* mask, double* F, int* sweeps)
{
    static double p[VO_FUND_LANES][VO_FUND_NSUM];
    double N1[3], N2[3], W[VO_FUND_NWORK];
    int m = 0;
    for (int l = 0; l < VO_FUND_LANES; ++l) {
        for (int q = 0; q < 4; ++q) p[l][q] = 0.0;
        for (int k = l; k < n; k += VO_FUND_LANES) {
            if (mask && !mask[k]) continue;
            ++m;
            p[l][0] = p[l][0] + (double)x1[2 * k]; p[l][1] = p[l][1] + (double)x1[2 * k + 1];
            p[l][2] = p[l][2] + (double)x2[2 * k]; p[l][3] = p[l][3] + (double)x2[2 * k + 1];
        }
    }
    vo_tree_sum(&p[0][0], VO_FUND_NSUM, 4);
    N1[1] = p[0][0] / (double)m; N1[2] = p[0][1] / (double)m; N2[1] = p[0][2] / (double)m; N2[2] = p[0][3] / (double)m;
    for (int l = 0; l < VO_FUND_LANES; ++l) {
        p[l][0] = 0.0; p[l][1] = 0.0;
        for (int k = l; k < n; k += VO_FUND_LANES) {
            if (mask && !mask[k]) continue;
            p[l][0] = p[l][0] + vo_fund_dist((double)x1[2 * k], (double)x1[2 * k + 1], N1[1], N1[2]);
            p[l][1] = p[l][1] + vo_fund_dist((double)x2[2 * k], (double)x2[2 * k + 1], N2[1], N2[2]);
        }
    }
    vo_tree_sum(&p[0][0], VO_FUND_NSUM, 2);
    N1[0] = VO_FUND_SQRT2 / (p[0][0] / (double)m);
    N2[0] = VO_FUND_SQRT2 / (p[0][1] / (double)m);
    if (!vo_fund_finite(N1[0]) || !vo_fund_finite(N2[0])) return 0;
    for (int l = 0; l < VO_FUND_LANES; ++l) {
        for (int q = 0; q < VO_FUND_NSUM; ++q) p[l][q] = 0.0;
        for (int k = l; k < n; k += VO_FUND_LANES) {
            if (mask && !mask[k]) continue;
            vo_fund_row(N1, N2, (double)x1[2 * k], (double)x1[2 * k + 1], (double)x2[2 * k], (double)x2[2 * k + 1], p[l], 1);
        }
    }
    vo_tree_sum(&p[0][0], VO_FUND_NSUM, VO_FUND_NSUM);
    for (int q = 0; q < VO_FUND_NSUM; ++q) W[q] = p[0][q];
    return vo_fund_solve(W, 1, N1, N2, F, sweeps);
}

static double score(const double* F, const float* x1, const float* x2, int n, double thr, int* n_in, int* n_nan)
{
    double p[VO_FUND_LANES];
    int cnt = 0;
    for (int l = 0; l < VO_FUND_LANES; ++l) {
        p[l] = 0.0;
        for (int k = l; k < n; k += VO_FUND_LANES) {
            double e = vo_fund_sampson(F, (double)x1[2 * k], (double)x1[2 * k + 1], (double)x2[2 * k], (double)x2[2 * k + 1]);
            if (e < thr) ++cnt;
            if (e != e && n_nan) ++*n_nan;
            p[l] = p[l] + (e < thr ? e : thr);
        }
    }
    vo_tree_sum(p, 1, 1);
    *n_in = cnt;
    return p[0];
}

static void note_sweeps(int32_t* census, const int* sw)
{
    if (!census) return;
    if (sw[0] > census[CN_SWEEPS9]) census[CN_SWEEPS9] = sw[0];
    if (sw[1] > census[CN_SWEEPS3]) census[CN_SWEEPS3] = sw[1];
}

/* -> status; F [9], inliers [n] (may be NULL), *n_inliers, best_F [9] (may be NULL: the best slot's
 * own F, the one the mask was taken with), census [CN_COUNT] (may be NULL) */
int fund_ref(const float* x1, const float* x2, int n, int method, int num_trials, double thr, double conf_percent, uint32_t seed,
             uint32_t key, double* F, uint8_t* inliers, int32_t* n_inliers, double* best_F, int32_t* census)
{
    int sw[2] = {0, 0};
    for (int q = 0; q < 9; ++q) F[q] = 0.0;
    if (best_F) for (int q = 0; q < 9; ++q) best_F[q] = 0.0;
    if (inliers) memset(inliers, 0, (size_t)(n > 0 ? n : 0));
    *n_inliers = 0;
    if (census) memset(census, 0, sizeof(int32_t) * CN_COUNT);
    if (census) census[CN_BEST] = -1;
    if (n < VO_FUND_SAMPLE) return FUND_TOO_FEW;
    if (method == FUND_NORM8) {
        double Fo[9];
        if (!fit_masked(x1, x2, n, NULL, Fo, sw)) return FUND_NO_CONSENSUS;
        note_sweeps(census, sw);
        if (census) census[CN_REFIT_MODEL] = 1;
        memcpy(F, Fo, sizeof(Fo));
        if (inliers) memset(inliers, 1, (size_t)n);
        *n_inliers = n;
        return FUND_OK;
    }
    const double conf = conf_percent / 100.0;
    vo_fund_replay r;
    double Fb[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    vo_fund_replay_begin(&r, num_trials);
    int slot = 0;
    for (; slot < num_trials && !vo_fund_replay_done(&r); ++slot) {
        uint32_t idx[VO_FUND_SAMPLE];
        double N1[3], N2[3], W[VO_FUND_NWORK], Fs[9];
        int att = 0, n_in = 0, nan = 0;
        if (!vo_fund_sample(seed, key, (uint32_t)slot, (uint32_t)n, idx, &att)) {
            if (census) census[CN_NO_SAMPLE]++;
            continue;
        }
        if (census && att > 1) census[CN_REATTEMPT]++;
        if (!vo_fund_fit_sample(x1, x2, idx, N1, N2, W, 1) || !vo_fund_solve(W, 1, N1, N2, Fs, sw)) {
            if (census) census[CN_NO_MODEL]++;
            continue;
        }
        note_sweeps(census, sw);
        double sc = score(Fs, x1, x2, n, thr, &n_in, &nan);
        if (census && nan) census[CN_NAN_DIST]++;
        if (census && sc == r.best_score) census[CN_TIES]++;
        if (vo_fund_replay_slot(&r, slot, 1, sc, n_in, n, conf)) {
            memcpy(Fb, Fs, sizeof(Fb));
            if (census) {
                census[CN_IMPROVED]++;
                if (vo_fund_trials_needed(n_in, n, conf) == VO_FUND_NO_BOUND) census[CN_NO_BOUND]++;
            }
        }
    }
    if (census) { census[CN_TRIALS] = r.trials; census[CN_BOUND] = r.bound; census[CN_BEST] = r.best; census[CN_SLOTS] = slot; }
    if (r.best < 0 || r.best_in < VO_FUND_SAMPLE) return FUND_NO_CONSENSUS;
    if (best_F) memcpy(best_F, Fb, sizeof(Fb));
    static uint8_t mask[1 << 20];
    if (n > (1 << 20)) return FUND_NO_CONSENSUS;
    int cnt = 0;
    for (int k = 0; k < n; ++k) {
        mask[k] = vo_fund_sampson(Fb, (double)x1[2 * k], (double)x1[2 * k + 1], (double)x2[2 * k], (double)x2[2 * k + 1]) < thr;
        cnt += mask[k];
    }
    double Fo[9];
    if (!fit_masked(x1, x2, n, mask, Fo, sw)) return FUND_NO_CONSENSUS;
    note_sweeps(census, sw);
    if (census) census[CN_REFIT_MODEL] = 1;
    memcpy(F, Fo, sizeof(Fo));
    if (inliers) memcpy(inliers, mask, (size_t)n);
    *n_inliers = cnt;
    return FUND_OK;
}

/* the pieces, for the tests that hold them to an independent evaluation */
int fund_ref_norm8(const float* x1, const float* x2, int n, const uint8_t* mask, double* F, int32_t* sweeps)
{
    int sw[2] = {0, 0};
    int ok = fit_masked(x1, x2, n, mask, F, sw);
    sweeps[0] = sw[0]; sweeps[1] = sw[1];
    return ok;
}

int fund_ref_sample_fit(const float* x1, const float* x2, const uint32_t* idx, double* F, int32_t* sweeps)
{
    double N1[3], N2[3], W[VO_FUND_NWORK];
    int sw[2] = {0, 0};
    int ok = vo_fund_fit_sample(x1, x2, idx, N1, N2, W, 1) && vo_fund_solve(W, 1, N1, N2, F, sw);
    sweeps[0] = sw[0]; sweeps[1] = sw[1];
    return ok;
}

void fund_ref_sampson(const double* F, const float* x1, const float* x2, int n, double* d)
{
    for (int k = 0; k < n; ++k)
        d[k] = vo_fund_sampson(F, (double)x1[2 * k], (double)x1[2 * k + 1], (double)x2[2 * k], (double)x2[2 * k + 1]);
}

int fund_ref_sample(uint32_t seed, uint32_t key, uint32_t slot, uint32_t n, uint32_t* idx, int32_t* attempts)
{
    int a = 0;
    int ok = vo_fund_sample(seed, key, slot, n, idx, &a);
    *attempts = a;
    return ok;
}

int fund_ref_trials_needed(int n_in, int n, double conf) { return vo_fund_trials_needed(n_in, n, conf); }

int fund_ref_jacobi(double* A, double* V, int n, int32_t* sweeps)
{
    int s = 0;
    int j = vo_fund_jacobi(A, V, n, 1, &s);
    *sweeps = s;
    return j;
}
