/*
 * vo_ref.c — CPU restatement of the VO.m per-frame path outside SIFT.
 * TEST INFRASTRUCTURE ONLY (see oracle.h).  "parity unpinned" vs MATLAB.
 *
 *   oracle_match        matchFeatures defaults (VO.m:87,283,293,311,323)
 *   oracle_track        find_remaining_points (VO.m:280-334)
 *   oracle_triangulate  triangulate, linear DLT + SVD null vector (VO.m:113-116)
 *   oracle_p3p          P3P (Grunert's quartic, Haralick et al. 1994 review)
 *   oracle_estworldpose estworldpose: P3P inside MSAC (VO.m:123-127)
 *   oracle_landmarks    VO.m:145-158 + CreateLandmarksFromFeatures.m:1-21
 *   oracle_run_sequence VO.m:64-232 (loop, state, quirks Q1-Q5)
 * Spec choices are written down in DESIGN.md §3.
 */
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "oracle.h"
#include "vo_spec.h"

/* ======================================================================= */
/* matchFeatures                                                            */
/* ======================================================================= */
static float inv_norm_u8(const uint8_t* a)
{
    int32_t s = 0;
    for (int k = 0; k < VO_DESC_LEN; ++k) s += (int32_t)a[k] * (int32_t)a[k];
    return s > 0 ? 1.0f / sqrtf((float)s) : 0.0f;
}

/* normalized SSD from the exact integer dot product */
static float ssd_u8(const uint8_t* a, const uint8_t* b, float ia, float ib)
{
    int32_t d = 0;
    for (int k = 0; k < VO_DESC_LEN; ++k) d += (int32_t)a[k] * (int32_t)b[k];
    float c = ((float)d * ia) * ib;
    return 2.0f - 2.0f * c;
}

#ifdef VO_CV_LITERAL
/* MATLAB-literal matchFeatures (Exhaustive, SSD, Prenormalized false): single rows
 * normalised to unit L2 in float, SSD as a sequential float sum of squared differences */
static void unit_rows(const uint8_t* A, const int* ia, int n, float* out)
{
    for (int i = 0; i < n; ++i) {
        const uint8_t* a = A + (size_t)ia[i] * VO_DESC_LEN;
        float s = 0;
        for (int k = 0; k < VO_DESC_LEN; ++k) s += (float)a[k] * (float)a[k];
        float nrm = sqrtf(s);
        for (int k = 0; k < VO_DESC_LEN; ++k) out[(size_t)i * VO_DESC_LEN + k] = nrm > 0 ? (float)a[k] / nrm : 0.0f;
    }
}

static int match_idx(const uint8_t* A, const int* ia, int n1, const uint8_t* B, const int* ib, int n2,
                     const vo_match_params* p, int* out1, int* out2)
{
    float* fa = (float*)malloc(sizeof(float) * VO_DESC_LEN * (n1 > 0 ? n1 : 1));
    float* fb = (float*)malloc(sizeof(float) * VO_DESC_LEN * (n2 > 0 ? n2 : 1));
    unit_rows(A, ia, n1, fa);
    unit_rows(B, ib, n2, fb);
    const float T = p->match_threshold * 0.04f;
    int P = 0;
    for (int i = 0; i < n1; ++i) {
        const float* a = fa + (size_t)i * VO_DESC_LEN;
        float best = INFINITY, second = INFINITY;
        int bidx = -1;
        for (int j = 0; j < n2; ++j) {
            const float* b = fb + (size_t)j * VO_DESC_LEN;
            float s = 0;
            for (int k = 0; k < VO_DESC_LEN; ++k) { float t = a[k] - b[k]; s += t * t; }
            if (s < best) { second = best; best = s; bidx = j; }
            else if (s < second) second = s;
        }
        if (bidx < 0) continue;
        if (!(best <= T)) continue;
        if (!(best / second <= p->max_ratio)) continue;
        out1[P] = i; out2[P] = bidx; P++;
    }
    free(fa); free(fb);
    return P;
}
#else
/* generic match on gathered rows: F1 rows = A[ia[i]], F2 rows = B[ib[j]] */
static int match_idx(const uint8_t* A, const int* ia, int n1, const uint8_t* B, const int* ib, int n2,
                     const vo_match_params* p, int* out1, int* out2)
{
    float* inb = (float*)malloc(sizeof(float) * (n2 > 0 ? n2 : 1));
    for (int j = 0; j < n2; ++j) inb[j] = inv_norm_u8(B + (size_t)ib[j] * VO_DESC_LEN);
    const float T = p->match_threshold * 0.04f;
    int P = 0;
    for (int i = 0; i < n1; ++i) {
        const uint8_t* a = A + (size_t)ia[i] * VO_DESC_LEN;
        float ina = inv_norm_u8(a);
        float best = INFINITY, second = INFINITY;
        int bidx = -1;
        for (int j = 0; j < n2; ++j) {
            float s = ssd_u8(a, B + (size_t)ib[j] * VO_DESC_LEN, ina, inb[j]);
            if (s < best) { second = best; best = s; bidx = j; }
            else if (s < second) second = s;
        }
        if (bidx < 0) continue;
        if (!(best <= T)) continue;
        float ratio = best / second;
        if (!(ratio <= p->max_ratio)) continue;
        out1[P] = i; out2[P] = bidx; P++;
    }
    free(inb);
    return P;
}
#endif

int oracle_match(const uint8_t* F1, int n1, const uint8_t* F2, int n2, const vo_match_params* p,
                 uint32_t* pairs, int capacity)
{
    int* ia = (int*)malloc(sizeof(int) * (n1 + 1));
    int* ib = (int*)malloc(sizeof(int) * (n2 + 1));
    int* o1 = (int*)malloc(sizeof(int) * (n1 + 1));
    int* o2 = (int*)malloc(sizeof(int) * (n1 + 1));
    for (int i = 0; i < n1; ++i) ia[i] = i;
    for (int j = 0; j < n2; ++j) ib[j] = j;
    int P = match_idx(F1, ia, n1, F2, ib, n2, p, o1, o2);
    for (int k = 0; k < P && k < capacity; ++k) { pairs[2 * k] = (uint32_t)o1[k] + 1; pairs[2 * k + 1] = (uint32_t)o2[k] + 1; }
    free(ia); free(ib); free(o1); free(o2);
    return P;
}

/* matchFeatures on general single-precision features (libvo vo_match_f32 when the rows are not
 * u8-valued): rows normalised to unit L2 (a_k = f_k / sqrtf(fmaf chain of f_k^2), zero rows stay
 * zero), SSD as the fmaf chain of (a_k - b_k)^2 over k = 0..127, then the u8 path's selection
 * (smallest / second smallest, ties to the lowest F2 row; SSD <= 0.04 * MatchThreshold; ratio
 * <= MaxRatio).  Element k of row i: F[col_major ? k * ld + i : i * ld + k]. */
static void norm_rows_f32(const float* F, int n, int ld, int col_major, float* out)
{
    for (int i = 0; i < n; ++i) {
        float n2 = 0.0f;
        for (int k = 0; k < VO_DESC_LEN; ++k) {
            const float v = col_major ? F[(size_t)k * ld + i] : F[(size_t)i * ld + k];
            n2 = fmaf(v, v, n2);
        }
        const float nrm = sqrtf(n2);
        for (int k = 0; k < VO_DESC_LEN; ++k) {
            const float v = col_major ? F[(size_t)k * ld + i] : F[(size_t)i * ld + k];
            out[(size_t)i * VO_DESC_LEN + k] = nrm > 0.0f ? v / nrm : 0.0f;
        }
    }
}

int oracle_match_f32(const float* F1, int n1, int ld1, const float* F2, int n2, int ld2, int col_major,
                     const vo_match_params* p, uint32_t* pairs, int capacity)
{
    float* a = (float*)malloc(sizeof(float) * VO_DESC_LEN * (size_t)(n1 > 0 ? n1 : 1));
    float* b = (float*)malloc(sizeof(float) * VO_DESC_LEN * (size_t)(n2 > 0 ? n2 : 1));
    norm_rows_f32(F1, n1, ld1, col_major, a);
    norm_rows_f32(F2, n2, ld2, col_major, b);
    const float T = p->match_threshold * 0.04f;
    int P = 0;
    for (int i = 0; i < n1; ++i) {
        float best = INFINITY, second = INFINITY;
        int bidx = -1;
        for (int j = 0; j < n2; ++j) {
            float s = 0.0f;
            for (int k = 0; k < VO_DESC_LEN; ++k) {
                const float d = a[(size_t)i * VO_DESC_LEN + k] - b[(size_t)j * VO_DESC_LEN + k];
                s = fmaf(d, d, s);
            }
            if (s < best) { second = best; best = s; bidx = j; }
            else if (s < second) second = s;
        }
        if (bidx < 0 || !(best <= T) || !(best / second <= p->max_ratio)) continue;
        if (P < capacity) { pairs[2 * P] = (uint32_t)i + 1; pairs[2 * P + 1] = (uint32_t)bidx + 1; }
        P++;
    }
    free(a); free(b);
    return P;
}

/* ======================================================================= */
/* find_remaining_points (VO.m:280-334) as index composition                 */
/* ======================================================================= */
int oracle_track(const uint8_t* old_l, const uint8_t* old_r, int n_old,
                 const uint8_t* cur_l, int n_cl, const uint8_t* cur_r, int n_cr,
                 const vo_match_params* p, uint32_t* idx_out, int capacity)
{
    int nmax = n_old + n_cl + n_cr + 1;
    int* old_idx = (int*)malloc(sizeof(int) * nmax);
    int* cl = (int*)malloc(sizeof(int) * nmax);
    int* cr = (int*)malloc(sizeof(int) * nmax);
    int* m1 = (int*)malloc(sizeof(int) * nmax);
    int* m2 = (int*)malloc(sizeof(int) * nmax);
    int* tmp = (int*)malloc(sizeof(int) * nmax);
    int* all = (int*)malloc(sizeof(int) * nmax);
    for (int i = 0; i < nmax; ++i) all[i] = i;
    int n_o = n_old;
    for (int i = 0; i < n_o; ++i) old_idx[i] = i;
    /* lm = matchFeatures(cur.l_desc, old.l_desc)  VO.m:283; old <- old(lm(:,2))  :287-290 */
    int nlm = match_idx(cur_l, all, n_cl, old_l, old_idx, n_o, p, m1, m2);
    for (int k = 0; k < nlm; ++k) tmp[k] = old_idx[m2[k]];
    for (int k = 0; k < nlm; ++k) { old_idx[k] = tmp[k]; cl[k] = m1[k]; }   /* cur.l <- cur.l(lm(:,1)) :305-306 */
    n_o = nlm;
    /* rm = matchFeatures(cur.r_desc, old.r_desc)  VO.m:293; old <- old(rm(:,2))  :297-300 */
    int nrm = match_idx(cur_r, all, n_cr, old_r, old_idx, n_o, p, m1, m2);
    for (int k = 0; k < nrm; ++k) tmp[k] = old_idx[m2[k]];
    for (int k = 0; k < nrm; ++k) { old_idx[k] = tmp[k]; cr[k] = m1[k]; }   /* cur.r <- cur.r(rm(:,1)) :307-308 */
    n_o = nrm;
    /* cm = matchFeatures(cur.l_desc, cur.r_desc)  VO.m:311; gathers :314-317 */
    int ncm = match_idx(cur_l, cl, nlm, cur_r, cr, nrm, p, m1, m2);
    for (int k = 0; k < ncm; ++k) tmp[k] = cl[m1[k]];
    int* cl2 = (int*)malloc(sizeof(int) * nmax);
    int* cr2 = (int*)malloc(sizeof(int) * nmax);
    for (int k = 0; k < ncm; ++k) { cl2[k] = tmp[k]; cr2[k] = cr[m2[k]]; }
    /* last = matchFeatures(cur.l_desc, old.l_desc)  VO.m:323; gathers :326-333 */
    int nlast = match_idx(cur_l, cl2, ncm, old_l, old_idx, n_o, p, m1, m2);
    for (int k = 0; k < nlast && k < capacity; ++k) {
        idx_out[3 * k + 0] = (uint32_t)old_idx[m2[k]] + 1;
        idx_out[3 * k + 1] = (uint32_t)cl2[m1[k]] + 1;
        idx_out[3 * k + 2] = (uint32_t)cr2[m1[k]] + 1;
    }
    free(old_idx); free(cl); free(cr); free(m1); free(m2); free(tmp); free(all); free(cl2); free(cr2);
    return nlast;
}

/* ======================================================================= */
/* triangulate: vo_spec.h's vo_dlt_point per row                            */
/* ======================================================================= */
void oracle_triangulate(const float* x1, const float* x2, int n, const double P1[12],
                        const double P2[12], double* X)
{
    for (int i = 0; i < n; ++i) vo_dlt_point(x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1], P1, P2, X + 3 * i);
}

/* ======================================================================= */
/* P3P: Grunert's quartic in v = s3/s1, coefficients by polynomial algebra   */
/* ======================================================================= */
static double peval(const double* a, int deg, double x)
{
    double r = a[deg];
    for (int i = deg - 1; i >= 0; --i) r = r * x + a[i];
    return r;
}

/* real roots of sum a[i] x^i (deg <= 4), ascending; deterministic
 * recursive-derivative bracketing + bisection. */
static int real_roots(const double* a_in, int deg, double* roots)
{
    double a[5];
    for (int i = 0; i <= deg; ++i) a[i] = a_in[i];
    /* drop negligible leading coefficients */
    double amax = 0;
    for (int i = 0; i <= deg; ++i) if (fabs(a[i]) > amax) amax = fabs(a[i]);
    if (amax == 0.0) return 0;
    while (deg > 0 && fabs(a[deg]) <= 1e-14 * amax) deg--;
    if (deg == 0) return 0;
    if (deg == 1) { roots[0] = -a[0] / a[1]; return 1; }
    if (deg == 2) {
        double disc = a[1] * a[1] - 4.0 * a[2] * a[0];
        if (disc < 0) return 0;
        double sq = sqrt(disc);
        double q = -0.5 * (a[1] + (a[1] >= 0 ? sq : -sq));
        double r1 = q / a[2], r2 = (q != 0.0) ? a[0] / q : r1;
        if (r1 <= r2) { roots[0] = r1; roots[1] = r2; } else { roots[0] = r2; roots[1] = r1; }
        return 2;
    }
    double d[4] = {0, 0, 0, 0};
    for (int i = 1; i <= deg; ++i) d[i - 1] = a[i] * (double)i;
    double crit[4];
    int nc = real_roots(d, deg - 1, crit);
    /* Cauchy bound */
    double B = 0;
    for (int i = 0; i < deg; ++i) { double t = fabs(a[i] / a[deg]); if (t > B) B = t; }
    B = B + 1.0;
    double pts[6];
    int np = 0;
    pts[np++] = -B;
    for (int i = 0; i < nc; ++i) if (crit[i] > -B && crit[i] < B) pts[np++] = crit[i];
    pts[np++] = B;
    int nr = 0;
    for (int k = 0; k + 1 < np; ++k) {
        double lo = pts[k], hi = pts[k + 1];
        double flo = peval(a, deg, lo), fhi = peval(a, deg, hi);
        if (flo == 0.0) { if (nr == 0 || roots[nr - 1] != lo) roots[nr++] = lo; continue; }
        if ((flo < 0) == (fhi < 0)) continue;
        for (int it = 0; it < 200; ++it) {
            double mid = 0.5 * (lo + hi);
            if (mid <= lo || mid >= hi) break;
            double fm = peval(a, deg, mid);
            if (fm == 0.0) { lo = hi = mid; break; }
            if ((fm < 0) == (flo < 0)) { lo = mid; flo = fm; } else hi = mid;
        }
        roots[nr++] = 0.5 * (lo + hi);
    }
    return nr;
}

int oracle_p3p(const double img[3][2], const double world[3][3], const double K[9],
               double Rs[4][9], double ts[4][3])
{
    vo_p3p p;
    if (!vo_p3p_setup(img, world, K, &p)) return 0;
    double roots[4];
    int nr = real_roots(p.P, 4, roots);
    int ns = 0;
    for (int k = 0; k < nr && ns < 4; ++k)
        if (vo_p3p_pose(&p, world, roots[k], Rs[ns], ts[ns])) ns++;
    return ns;
}

/* ======================================================================= */
/* estworldpose: P3P + MSAC                                 */
/* ======================================================================= */
/* one hypothesis slot: returns 1 if valid (R,t filled) */
static int msac_hypothesis(const double* img, const double* world, int n, const double K[9], uint32_t seed,
                           uint32_t frame_key, uint32_t s, double R[9], double t[3])
{
    uint32_t idx[4];
    if (!vo_pose_sample(seed, frame_key, s, (uint32_t)n, idx)) return 0;
    double im3[3][2], w3[3][3];
    for (int q = 0; q < 3; ++q) {
        im3[q][0] = img[2 * idx[q]]; im3[q][1] = img[2 * idx[q] + 1];
        for (int i = 0; i < 3; ++i) w3[q][i] = world[3 * idx[q] + i];
    }
    double Rs[4][9], ts[4][3];
    int ns = oracle_p3p(im3, w3, K, Rs, ts);
    int best = -1;
    double be = INFINITY;
    for (int k = 0; k < ns; ++k) {
        double e = vo_pose_reproj_err2(Rs[k], ts[k], K, world + 3 * idx[3], img + 2 * idx[3]);
        if (e < be) { be = e; best = k; }
    }
    if (best < 0) return 0;
    memcpy(R, Rs[best], sizeof(double) * 9);
    memcpy(t, ts[best], sizeof(double) * 3);
    return 1;
}

/* MSAC score: 64 lane-strided partial sums + vo_tree_sum */
static double msac_score(const double R[9], const double t[3], const double* img, const double* world, int n,
                         const double K[9], double thr, int* n_in)
{
    double part[64];
    int cnt = 0;
    for (int l = 0; l < 64; ++l) part[l] = 0.0;
    for (int k = 0; k < n; ++k) {
        double e = vo_pose_reproj_err2(R, t, K, world + 3 * k, img + 2 * k);
        if (e < thr) cnt++;
        part[k & 63] = part[k & 63] + (e < thr ? e : thr);
    }
    vo_tree_sum(part, 1, 1);
    *n_in = cnt;
    return part[0];
}

int oracle_estworldpose(const double* img, const double* world, int n, const double K[9],
                        const vo_ransac_params* p, uint32_t frame_key, double T[16],
                        uint8_t* inliers, int* n_inliers)
{
    if (n_inliers) *n_inliers = 0;
    if (n < 4) return VO_ERR_TOO_FEW_POINTS;
    const double thr = p->max_reprojection_error * p->max_reprojection_error;
    const double conf = p->confidence / 100.0;
    vo_pose_replay r;
    vo_pose_replay_begin(&r, p->max_num_trials);
    double bR[9], bt[3];
    for (int s = 0; s < p->max_num_trials && !vo_pose_replay_done(&r); ++s) {
        double R[9], t[3], sc = 0;
        int nin = 0;
        const int valid = msac_hypothesis(img, world, n, K, p->seed, frame_key, (uint32_t)s, R, t);
        if (valid) sc = msac_score(R, t, img, world, n, K, thr, &nin);
        if (vo_pose_replay_slot(&r, s, valid, sc, nin, n, conf)) {
            memcpy(bR, R, sizeof(bR)); memcpy(bt, t, sizeof(bt));
        }
    }
    if (r.best < 0 || r.best_in < 4) return VO_ERR_NO_CONSENSUS;
    int cnt = 0;
    for (int k = 0; k < n; ++k) {
        double e = vo_pose_reproj_err2(bR, bt, K, world + 3 * k, img + 2 * k);
        int in = e < thr;
        if (inliers) inliers[k] = (uint8_t)in;
        cnt += in;
    }
    if (n_inliers) *n_inliers = cnt;
    vo_pose_to_T(bR, bt, T);   /* camera pose in world */
    return VO_OK;
}

/* ======================================================================= */
/* landmarks: VO.m:145-160 + CreateLandmarksFromFeatures.m                  */
/* ======================================================================= */
/* CreateLandmarksFromFeatures.m:1-16 in the camera frame: X[rows][3] (the triangulated
 * point, single-rounded as vo_dlt_point returns it) and keep[rows] (0 = zero row).  Returns
 * rows; only min(rows, capacity) are written. */
int oracle_landmark_rows(const float* l_pos, const float* r_pos, int S, const float* old_l,
                         const float* old_r, int K, const double P1[12], const double P2[12],
                         float* X_out, uint8_t* keep, int capacity)
{
    int* idx = (int*)malloc(sizeof(int) * (S + 1));
    int M = 0;
    for (int j = 0; j < S; ++j) {
        int hit = 0;
        for (int k = 0; k < K && !hit; ++k)
            if (old_l[2 * k] == l_pos[2 * j] || old_l[2 * k + 1] == l_pos[2 * j + 1]) hit = 1;
        for (int k = 0; k < K && !hit; ++k)
            if (old_r[2 * k] == r_pos[2 * j] || old_r[2 * k + 1] == r_pos[2 * j + 1]) hit = 1;
        if (!hit) idx[M++] = j;
    }
    /* landmarks = zeros(size(features_l,2),3) -> 2 rows; grows to last kept odd i */
    int rows = 2;
    for (int r = 0; r < 2 && r < capacity; ++r) { keep[r] = 0; X_out[3 * r] = X_out[3 * r + 1] = X_out[3 * r + 2] = 0.0f; }
    for (int i = 0; i < M; i += 2) {   /* 1-based odd i <-> 0-based even */
        double X[3];
        vo_dlt_point(l_pos[2 * idx[i]], l_pos[2 * idx[i] + 1], r_pos[2 * idx[i]], r_pos[2 * idx[i] + 1], P1, P2, X);
        if (X[2] < 0) continue;
        if (X[2] > 80) continue;
        for (int r = rows; r < i + 1 && r < capacity; ++r) { keep[r] = 0; X_out[3 * r] = X_out[3 * r + 1] = X_out[3 * r + 2] = 0.0f; }
        if (i + 1 > rows) rows = i + 1;
        if (i < capacity) {
            keep[i] = 1;
            for (int a = 0; a < 3; ++a) X_out[3 * i + a] = (float)X[a];
        }
    }
    free(idx);
    return rows;
}

/* CreateLandmarksFromFeatures.m:17: world = single(pose * [X; 1]) for kept rows. */
void oracle_landmarks_to_world(const double pose[16], const float* X, const uint8_t* keep, int n, double* out)
{
    for (int m = 0; m < n; ++m)
        for (int a = 0; a < 3; ++a) {
            if (!keep[m]) { out[3 * m + a] = 0.0; continue; }
            const double x0 = X[3 * m], x1 = X[3 * m + 1], x2 = X[3 * m + 2];
            double w = pose[4 * a] * x0 + pose[4 * a + 1] * x1 + pose[4 * a + 2] * x2 + pose[4 * a + 3];
            out[3 * m + a] = (double)(float)w;
        }
}

int oracle_landmarks(const float* l_pos, const float* r_pos, int S, const float* old_l,
                     const float* old_r, int K, const double P1[12], const double P2[12],
                     const double pose[16], double* out, int capacity)
{
    int cap = S + 2;
    float* X = (float*)malloc(sizeof(float) * 3 * cap);
    uint8_t* keep = (uint8_t*)malloc(cap);
    int rows = oracle_landmark_rows(l_pos, r_pos, S, old_l, old_r, K, P1, P2, X, keep, cap);
    if (out) oracle_landmarks_to_world(pose, X, keep, rows < capacity ? rows : capacity, out);
    free(X);
    free(keep);
    return rows;
}

/* ======================================================================= */
/* the loop: VO.m:64-232                                                    */
/* ======================================================================= */
static void mat4_mul(const double* A, const double* B, double* C)
{
    double T[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            T[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j] + A[4 * i + 3] * B[12 + j];
    memcpy(C, T, sizeof(T));
}

static const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

long oracle_run_sequence(const uint8_t* lefts, const uint8_t* rights, int F, int rows, int cols,
                         const vo_calib* calib, const vo_sift_params* sp, const vo_match_params* mp,
                         const vo_ransac_params* rp, vo_step_out* outs, double* lm_out, long lm_cap,
                         uint32_t key0, float* lm_cam_X, uint8_t* lm_cam_keep)
{
    if (!oracle_sift_params_ok(sp)) return -1;
    int cap = sp->max_keypoints;
    vo_keypoint *kl = malloc(sizeof(vo_keypoint) * cap), *kr = malloc(sizeof(vo_keypoint) * cap);
    uint8_t *dl = malloc((size_t)cap * 128), *dr = malloc((size_t)cap * 128);
    /* features state (stereo subset of previous frame) */
    float *fl_pos = malloc(sizeof(float) * 2 * cap), *fr_pos = malloc(sizeof(float) * 2 * cap);
    uint8_t *fl_desc = malloc((size_t)cap * 128), *fr_desc = malloc((size_t)cap * 128);
    int nf = 0, have_features = 0;
    uint32_t* pairs = malloc(sizeof(uint32_t) * 2 * cap);
    uint32_t* tidx = malloc(sizeof(uint32_t) * 3 * cap);
    double *img = malloc(sizeof(double) * 2 * cap), *wld = malloc(sizeof(double) * 3 * cap);
    float *ol = malloc(sizeof(float) * 2 * cap), *orr = malloc(sizeof(float) * 2 * cap);
    float *sl = malloc(sizeof(float) * 2 * cap), *sr = malloc(sizeof(float) * 2 * cap);
    double pose[16];
    memcpy(pose, I4, sizeof(pose));
    long lm_rows = 0;
    size_t fsz = (size_t)rows * cols;
    for (int f = 0; f < F; ++f) {
        vo_step_out* o = &outs[f];
        memset(o, 0, sizeof(*o));
        int nl = oracle_sift(lefts + f * fsz, rows, cols, cols, sp, kl, dl, cap);
        int nr = oracle_sift(rights + f * fsz, rows, cols, cols, sp, kr, dr, cap);
        if (nl > cap) nl = cap;
        if (nr > cap) nr = cap;
        int S = oracle_match(dl, nl, dr, nr, mp, pairs, cap);
        o->n_left = nl; o->n_right = nr; o->n_stereo = S;
        memcpy(o->rel_pose, I4, sizeof(I4));
        /* stereo subset (VO.m:141-144 / 207-210) */
        for (int k = 0; k < S; ++k) {
            int a = (int)pairs[2 * k] - 1, b = (int)pairs[2 * k + 1] - 1;
            sl[2 * k] = kl[a].x; sl[2 * k + 1] = kl[a].y;
            sr[2 * k] = kr[b].x; sr[2 * k + 1] = kr[b].y;
        }
        if (have_features) {
            int Kt = oracle_track(fl_desc, fr_desc, nf, dl, nl, dr, nr, mp, tidx, cap);
            o->n_tracked = Kt;
            for (int k = 0; k < Kt; ++k) {
                int oi = (int)tidx[3 * k] - 1, ci = (int)tidx[3 * k + 1] - 1;
                ol[2 * k] = fl_pos[2 * oi]; ol[2 * k + 1] = fl_pos[2 * oi + 1];
                orr[2 * k] = fr_pos[2 * oi]; orr[2 * k + 1] = fr_pos[2 * oi + 1];
                img[2 * k] = kl[ci].x; img[2 * k + 1] = kl[ci].y;
            }
            oracle_triangulate(ol, orr, Kt, calib->P1, calib->P2, wld);
            double T[16];
            int nin = 0;
            int st = oracle_estworldpose(img, wld, Kt, calib->K, rp, key0 + (uint32_t)f, T, NULL, &nin);
            o->status = st;
            o->n_inliers = nin;
            if (st == VO_OK) {
                memcpy(o->rel_pose, T, sizeof(T));
                mat4_mul(pose, T, pose);
            }
            long room = lm_cap - lm_rows;
            int room_i = room > 0 ? (int)(room < 0x7fffffff ? room : 0x7fffffff) : 0;
            int rows_added;
            if (lm_cam_X)        /* camera-frame rows for a sharded run (world transform after the chain) */
                rows_added = oracle_landmark_rows(sl, sr, S, ol, orr, Kt, calib->P1, calib->P2,
                                                  lm_cam_X + 3 * lm_rows, lm_cam_keep + lm_rows, room_i);
            else
                rows_added = oracle_landmarks(sl, sr, S, ol, orr, Kt, calib->P1, calib->P2, pose,
                                              lm_out ? lm_out + 3 * lm_rows : NULL, room_i);
            o->n_landmarks = rows_added;
            lm_rows += rows_added;
        }
        memcpy(o->pose, pose, sizeof(pose));
        /* features = stereo subset (VO.m:225-230) */
        for (int k = 0; k < S; ++k) {
            int a = (int)pairs[2 * k] - 1, b = (int)pairs[2 * k + 1] - 1;
            fl_pos[2 * k] = sl[2 * k]; fl_pos[2 * k + 1] = sl[2 * k + 1];
            fr_pos[2 * k] = sr[2 * k]; fr_pos[2 * k + 1] = sr[2 * k + 1];
            memcpy(fl_desc + (size_t)k * 128, dl + (size_t)a * 128, 128);
            memcpy(fr_desc + (size_t)k * 128, dr + (size_t)b * 128, 128);
        }
        nf = S;
        have_features = 1;
    }
    free(kl); free(kr); free(dl); free(dr); free(fl_pos); free(fr_pos); free(fl_desc); free(fr_desc);
    free(pairs); free(tidx); free(img); free(wld); free(ol); free(orr); free(sl); free(sr);
    return lm_rows;
}

int oracle_sift_match_pair(const uint8_t* left, const uint8_t* right, int rows, int cols,
                           const vo_sift_params* sp, const vo_match_params* mp,
                           int* n_left, int* n_right)
{
    if (!oracle_sift_params_ok(sp)) return -1;
    int cap = sp->max_keypoints;
    vo_keypoint *kl = malloc(sizeof(vo_keypoint) * cap), *kr = malloc(sizeof(vo_keypoint) * cap);
    uint8_t *dl = malloc((size_t)cap * 128), *dr = malloc((size_t)cap * 128);
    uint32_t* pairs = malloc(sizeof(uint32_t) * 2 * cap);
    int nl = oracle_sift(left, rows, cols, cols, sp, kl, dl, cap);
    int nr = oracle_sift(right, rows, cols, cols, sp, kr, dr, cap);
    if (nl > cap) nl = cap;
    if (nr > cap) nr = cap;
    int S = oracle_match(dl, nl, dr, nr, mp, pairs, cap);
    if (n_left) *n_left = nl;
    if (n_right) *n_right = nr;
    free(kl); free(kr); free(dl); free(dr); free(pairs);
    return S;
}
