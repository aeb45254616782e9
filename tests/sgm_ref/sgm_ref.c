/* CPU reference of vo_disparity_sgm / vo_reconstruct_scene (test infrastructure): include/vo_spec.h's
 * vo_sgm_* / vo_reconstruct_* functions around the normative loops of DESIGN.md 3.5.5.  The device kernels
 * (csrc/sgm.hip) give the same bytes.  The counters name the branches a case reaches (tests/sgm_ref.py has
 * their indices). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "vo_spec.h"

enum {
    SGM_C_FIRST = 0,        /* + q: a path's first pixel in direction q */
    SGM_C_ARG = 8,          /* + 4 q + a: argument a of the inner min chosen (the first of equals) in direction q */
    SGM_C_NO_LOWER = 40,    /* k - 1 absent */
    SGM_C_NO_UPPER = 41,    /* k + 1 absent */
    SGM_C_TIE = 42,         /* the minimum of S reached more than once */
    SGM_C_K_FIRST = 43,     /* k* = 0 */
    SGM_C_K_LAST = 44,      /* k* = D - 1 */
    SGM_C_DEN_ZERO = 45,    /* den == 0 at an interior k* of a returned pixel */
    SGM_C_PLUS_HALF = 46,   /* offset exactly +0.5 */
    SGM_C_MINUS_HALF = 47,  /* offset exactly -0.5 */
    SGM_C_INVALID_LEFT = 48,   /* matched column < 0 */
    SGM_C_INVALID_RIGHT = 49,  /* matched column > cols - 1 */
    SGM_C_UNRELIABLE = 50,
    SGM_C_V_ZERO = 51,
    SGM_C_RETURNED = 52,    /* pixels with a number */
    SGM_C_SUBPIXEL = 53,    /* of them, with an offset applied */
    SGM_N_COUNTERS = 56
};

int sgm_ref_n_counters(void) { return SGM_N_COUNTERS; }
float sgm_ref_select(const uint16_t* S, int D, int dmin, int x, int cols, int U) { return vo_sgm_select(S, D, dmin, x, cols, U); }
int sgm_ref_step(int c, int lk, int lm, int lp, int m, int P1, int P2) { return vo_sgm_step(c, lk, lm, lp, m, P1, P2); }
int sgm_ref_reprojection(const double* P1, const double* P2, double* Q) { return vo_reprojection_from_projections(P1, P2, Q); }

void sgm_ref_census(const uint8_t* img, int rows, int cols, uint64_t* out)
{
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) out[(size_t)y * cols + x] = vo_sgm_census(img, rows, cols, y, x);
}

static void count_select(const uint16_t* S, int D, int dmin, int x, int cols, int U, int64_t* n)
{
    int ks = 0, ties = 0;
    uint32_t V = S[0], v = 0xffffu;
    for (int k = 1; k < D; ++k) if (S[k] < V) { V = S[k]; ks = k; }
    for (int k = 0; k < D; ++k) {
        if (k != ks && S[k] == V) ties = 1;
        if ((k < ks - 1 || k > ks + 1) && S[k] < v) v = S[k];
    }
    n[SGM_C_TIE] += ties;
    n[SGM_C_K_FIRST] += ks == 0;
    n[SGM_C_K_LAST] += ks == D - 1;
    n[SGM_C_V_ZERO] += V == 0;
    if (100u * v < (100u + (uint32_t)U) * V) { n[SGM_C_UNRELIABLE]++; return; }
    const int xr = x - (dmin + ks);
    if (xr < 0) { n[SGM_C_INVALID_LEFT]++; return; }
    if (xr > cols - 1) { n[SGM_C_INVALID_RIGHT]++; return; }
    n[SGM_C_RETURNED]++;
    if (ks > 0 && ks < D - 1) {
        const int a = S[ks - 1], b = S[ks + 1], den = 2 * (a - 2 * (int)V + b);
        if (den == 0) { n[SGM_C_DEN_ZERO]++; return; }
        n[SGM_C_SUBPIXEL]++;
        n[SGM_C_PLUS_HALF] += 2 * (a - b) == den;
        n[SGM_C_MINUS_HALF] += 2 * (a - b) == -den;
    }
}

/* Tightly packed u8 images -> S [rows][cols][D] (may be NULL) and disp [rows][cols]; counters (may be NULL)
 * SGM_N_COUNTERS int64, added to.  0, or -1 when memory runs out. */
int sgm_ref_disparity(const uint8_t* left, const uint8_t* right, int rows, int cols, int dmin, int D, int P1, int P2, int U,
                      uint16_t* S_out, float* disp, int64_t* counters)
{
    const size_t px = (size_t)rows * cols;
    uint64_t* cl = malloc(sizeof(uint64_t) * px);
    uint64_t* cr = malloc(sizeof(uint64_t) * px);
    uint8_t* C = malloc(px * D);
    uint16_t* L = malloc(sizeof(uint16_t) * px * D);
    uint16_t* S = S_out ? S_out : malloc(sizeof(uint16_t) * px * D);
    int64_t dummy[SGM_N_COUNTERS];
    int64_t* n = counters ? counters : dummy;
    if (!cl || !cr || !C || !L || !S) { free(cl); free(cr); free(C); free(L); if (!S_out) free(S); return -1; }
    sgm_ref_census(left, rows, cols, cl);
    sgm_ref_census(right, rows, cols, cr);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x)
            for (int k = 0; k < D; ++k)
                C[((size_t)y * cols + x) * D + k] =
                    (uint8_t)vo_sgm_popcount(cl[(size_t)y * cols + x] ^ cr[(size_t)y * cols + vo_sgm_right_col(x, dmin + k, cols)]);
    memset(S, 0, sizeof(uint16_t) * px * D);
    for (int q = 0; q < VO_SGM_NDIR; ++q) {
        int dy, dx;
        vo_sgm_dir(q, &dy, &dx);
        const int fwd = dy > 0 || (dy == 0 && dx > 0);             /* the predecessor comes earlier in raster order */
        for (size_t i = 0; i < px; ++i) {
            const size_t p = fwd ? i : px - 1 - i;
            const int y = (int)(p / cols), x = (int)(p % cols), py = y - dy, qx = x - dx;
            const uint8_t* c = C + p * D;
            uint16_t* l = L + p * D;
            if (py < 0 || py >= rows || qx < 0 || qx >= cols) {
                for (int k = 0; k < D; ++k) l[k] = c[k];
                n[SGM_C_FIRST + q]++;
            } else {
                const uint16_t* b = L + ((size_t)py * cols + qx) * D;
                int m = b[0];
                for (int k = 1; k < D; ++k) if (b[k] < m) m = b[k];
                for (int k = 0; k < D; ++k) {
                    const int lm = k > 0 ? b[k - 1] : VO_SGM_ABSENT, lp = k < D - 1 ? b[k + 1] : VO_SGM_ABSENT;
                    l[k] = (uint16_t)vo_sgm_step(c[k], b[k], lm, lp, m, P1, P2);
                    const int cand[4] = {b[k], lm + P1, lp + P1, m + P2};
                    int a = 0;
                    for (int j = 1; j < 4; ++j) if (cand[j] < cand[a]) a = j;
                    n[SGM_C_ARG + 4 * q + a]++;
                    n[SGM_C_NO_LOWER] += k == 0;
                    n[SGM_C_NO_UPPER] += k == D - 1;
                }
            }
            for (int k = 0; k < D; ++k) S[p * D + k] = (uint16_t)(S[p * D + k] + l[k]);
        }
    }
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            const uint16_t* s = S + ((size_t)y * cols + x) * D;
            disp[(size_t)y * cols + x] = vo_sgm_select(s, D, dmin, x, cols, U);
            count_select(s, D, dmin, x, cols, U, n);
        }
    free(cl); free(cr); free(C); free(L);
    if (!S_out) free(S);
    return 0;
}

/* disp tightly packed, row-major [rows][cols] or col_major [cols][rows] -> xyz [rows][cols][3], or three
 * column-major planes */
void sgm_ref_reconstruct(const float* disp, int rows, int cols, int col_major, const double* Q, float* xyz)
{
    const size_t px = (size_t)rows * cols;
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            float p[3];
            const size_t i = col_major ? (size_t)x * rows + y : (size_t)y * cols + x;
            vo_reconstruct_point(Q, x + 1, y + 1, disp[i], p);
            for (int k = 0; k < 3; ++k) xyz[col_major ? k * px + i : 3 * i + k] = p[k];
        }
}
