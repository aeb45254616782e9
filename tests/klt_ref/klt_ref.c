/* CPU reference of vo_track_points (test infrastructure): include/vo_spec.h's own vo_klt_*
 * functions -- the ones k_klt_pyr and k_klt_track call -- around the normative loops of DESIGN
 * 3.5.3: the pyramid, the level loop, the template, the iterations, the score pass and the back
 * pass.  Window sums are int64 in sample order (exact integers: any order gives the same bytes).
 * Compiled with the oracle's flags (no contraction, no fast-math).  Images are tightly packed
 * row-major u8; points are single 1-based pixels, x = column. */
#include <stdint.h>
#include <string.h>
#include "vo_spec.h"

typedef struct { uint8_t status, stop, iterations, levels_skipped; float bidir_error; } klt_info;
typedef struct { const uint8_t* p; int rows, cols; } klt_level;

/* per-level record of the forward pass (census and the comparison with the float64 restatement):
 * VO_KLT_STOP_* for a level that iterated to a stop, 16 + VO_KLT_* for one that ended otherwise */
#define LV_NOT_RUN 255

static int px(const klt_level* L, int r, int c)
{
    r = r < 0 ? 0 : r >= L->rows ? L->rows - 1 : r;
    c = c < 0 ? 0 : c >= L->cols ? L->cols - 1 : c;
    return L->p[(long)r * L->cols + c];
}
static int gx(const klt_level* L, int r, int c)
{
    return vo_klt_scharr(px(L, r - 1, c - 1), px(L, r - 1, c + 1), px(L, r, c - 1), px(L, r, c + 1), px(L, r + 1, c - 1), px(L, r + 1, c + 1));
}
static int gy(const klt_level* L, int r, int c)
{
    return vo_klt_scharr(px(L, r - 1, c - 1), px(L, r + 1, c - 1), px(L, r - 1, c), px(L, r + 1, c), px(L, r - 1, c + 1), px(L, r + 1, c + 1));
}

/* total bytes of `levels` levels; off[l] the offset of level l */
long klt_ref_layout(int rows, int cols, int levels, long* off)
{
    long t = 0;
    for (int l = 0; l < levels; ++l) {
        if (off) off[l] = t;
        t += (long)vo_klt_level_dim(rows, l) * vo_klt_level_dim(cols, l);
    }
    return t;
}

void klt_ref_pyramid(const uint8_t* img, int rows, int cols, int levels, uint8_t* out)
{
    long off[VO_KLT_MAX_LEVELS];
    klt_ref_layout(rows, cols, levels, off);
    memcpy(out, img, (size_t)rows * cols);
    for (int l = 0; l + 1 < levels; ++l) {
        const int r0 = vo_klt_level_dim(rows, l), c0 = vo_klt_level_dim(cols, l);
        const int r1 = (r0 + 1) / 2, c1 = (c0 + 1) / 2;
        for (int r = 0; r < r1; ++r)
            for (int c = 0; c < c1; ++c) out[off[l + 1] + (long)r * c1 + c] = (uint8_t)vo_klt_pyr_pixel(out + off[l], r0, c0, c0, r, c);
    }
}

typedef struct {
    int status, stop, iterations, skipped;
    float x, y, score;
    uint8_t lv[VO_KLT_MAX_LEVELS];
} klt_pass;

/* one pass (forward, or back with the images swapped): (x0, y0) 0-based in A, tracked into B */
static void track_pass(const klt_level* A, const klt_level* B, int L, float x0, float y0, int has_guess, float g0x, float g0y, int bw,
                       int bh, int max_it, int want_score, klt_pass* r)
{
    short I[VO_KLT_MAX_WIN * VO_KLT_MAX_WIN], Ix[VO_KLT_MAX_WIN * VO_KLT_MAX_WIN], Iy[VO_KLT_MAX_WIN * VO_KLT_MAX_WIN];
    const float hx = (float)(bw - 1) * 0.5f, hy = (float)(bh - 1) * 0.5f;
    float nx = 0.0f, ny = 0.0f;
    int w[4], ix, iy;
    r->status = VO_KLT_OK; r->stop = VO_KLT_STOP_NONE; r->iterations = 0; r->skipped = 0; r->score = 0.0f;
    r->x = x0; r->y = y0;
    memset(r->lv, LV_NOT_RUN, sizeof(r->lv));
    for (int l = L - 1; l >= 0; --l) {
        const float sc = 1.0f / (float)(1 << l);
        const float px0 = x0 * sc, py0 = y0 * sc;
        const klt_level* a = A + l;
        const klt_level* b = B + l;
        if (l == L - 1) { nx = (has_guess ? g0x : x0) * sc; ny = (has_guess ? g0y : y0) * sc; }
        else { nx = 2.0f * nx; ny = 2.0f * ny; }
        int why = VO_KLT_OK;
        float Am[4];
        /* template */
        if (!vo_klt_corner(px0 - hx, py0 - hy, bw, bh, a->rows, a->cols, &ix, &iy, w)) why = VO_KLT_TEMPLATE_OUT;
        else {
            int64_t sxx = 0, sxy = 0, syy = 0;
            for (int y = 0; y < bh; ++y)
                for (int x = 0; x < bw; ++x) {
                    const int rr = iy + y, cc = ix + x, s = y * bw + x;
                    const int v = vo_klt_bil(px(a, rr, cc), px(a, rr, cc + 1), px(a, rr + 1, cc), px(a, rr + 1, cc + 1), w, 9);
                    const int dx = vo_klt_bil(gx(a, rr, cc), gx(a, rr, cc + 1), gx(a, rr + 1, cc), gx(a, rr + 1, cc + 1), w, 14);
                    const int dy = vo_klt_bil(gy(a, rr, cc), gy(a, rr, cc + 1), gy(a, rr + 1, cc), gy(a, rr + 1, cc + 1), w, 14);
                    I[s] = (short)v; Ix[s] = (short)dx; Iy[s] = (short)dy;
                    sxx += (int64_t)dx * dx; sxy += (int64_t)dx * dy; syy += (int64_t)dy * dy;
                }
            if (!vo_klt_gradient_matrix(sxx, sxy, syy, bw, bh, Am)) why = VO_KLT_FLAT;
        }
        int stop = VO_KLT_STOP_NONE, j = 0;
        if (why == VO_KLT_OK) {
            float qx = nx - hx, qy = ny - hy, mx = nx, my = ny, pdx = 0.0f, pdy = 0.0f;
            for (j = 0; j < max_it; ++j) {
                if (!vo_klt_corner(qx, qy, bw, bh, b->rows, b->cols, &ix, &iy, w)) { why = VO_KLT_LOST; break; }
                int64_t s1 = 0, s2 = 0;
                for (int y = 0; y < bh; ++y)
                    for (int x = 0; x < bw; ++x) {
                        const int rr = iy + y, cc = ix + x, s = y * bw + x;
                        const int diff = vo_klt_bil(px(b, rr, cc), px(b, rr, cc + 1), px(b, rr + 1, cc), px(b, rr + 1, cc + 1), w, 9) - I[s];
                        s1 += (int64_t)diff * Ix[s]; s2 += (int64_t)diff * Iy[s];
                    }
                float dx, dy;
                vo_klt_delta(Am, s1, s2, &dx, &dy);
                qx = qx + dx; qy = qy + dy;
                mx = qx + hx; my = qy + hy;
                stop = vo_klt_stop(j, dx, dy, pdx, pdy, &mx, &my);
                if (stop != VO_KLT_STOP_NONE) { ++j; break; }
                pdx = dx; pdy = dy;
            }
            if (why == VO_KLT_OK) {
                if (stop == VO_KLT_STOP_NONE) stop = VO_KLT_STOP_MAXIT;
                nx = mx; ny = my;
            }
        }
        r->lv[l] = (uint8_t)(why == VO_KLT_OK ? stop : 16 + why);
        if (l == 0) { r->stop = why == VO_KLT_OK ? stop : VO_KLT_STOP_NONE; r->iterations = j; }
        if (why != VO_KLT_OK) {
            if (l == 0) { r->status = why; return; }
            r->skipped = r->skipped + 1;
        }
    }
    if (!vo_klt_inside(nx, ny, A[0].rows, A[0].cols)) { r->status = VO_KLT_LOST; return; }
    r->x = nx; r->y = ny;
    /* the level-0 template is still in I; the corner of a point inside the image is never out */
    if (want_score && vo_klt_corner(nx - hx, ny - hy, bw, bh, B[0].rows, B[0].cols, &ix, &iy, w)) {
        int64_t s2 = 0;
        for (int y = 0; y < bh; ++y)
            for (int x = 0; x < bw; ++x) {
                const int rr = iy + y, cc = ix + x;
                const int diff = vo_klt_bil(px(B, rr, cc), px(B, rr, cc + 1), px(B, rr + 1, cc), px(B, rr + 1, cc + 1), w, 9) - I[y * bw + x];
                s2 += (int64_t)diff * diff;
            }
        r->score = vo_klt_score(s2, bw, bh);
    }
}

/* pyr0, pyr1: klt_ref_pyramid's output for the two images.  guess may be NULL; max_bidir +inf: no
 * back pass.  level_codes [n][VO_KLT_MAX_LEVELS] (may be NULL): the forward pass' per-level record. */
void klt_ref_track(const uint8_t* pyr0, const uint8_t* pyr1, int rows, int cols, const float* pts0, const float* guess, int n,
                   int levels, int bh, int bw, int max_it, float max_bidir, float* pts1, uint8_t* valid, float* scores, klt_info* info,
                   uint8_t* level_codes)
{
    klt_level A[VO_KLT_MAX_LEVELS], B[VO_KLT_MAX_LEVELS];
    long off[VO_KLT_MAX_LEVELS];
    klt_ref_layout(rows, cols, levels, off);
    for (int l = 0; l < levels; ++l) {
        A[l].p = pyr0 + off[l]; B[l].p = pyr1 + off[l];
        A[l].rows = B[l].rows = vo_klt_level_dim(rows, l);
        A[l].cols = B[l].cols = vo_klt_level_dim(cols, l);
    }
    const int bidir = max_bidir < vo_u32_as_f32(0x7f800000u);
    for (int i = 0; i < n; ++i) {
        const float x0 = pts0[2 * i] - 1.0f, y0 = pts0[2 * i + 1] - 1.0f;
        klt_pass f, bk;
        track_pass(A, B, levels, x0, y0, guess != 0, guess ? guess[2 * i] - 1.0f : 0.0f, guess ? guess[2 * i + 1] - 1.0f : 0.0f, bw, bh,
                   max_it, 1, &f);
        int status = f.status;
        float e = vo_u32_as_f32(0x7fc00000u);
        if (status == VO_KLT_OK && bidir) {
            track_pass(B, A, levels, f.x, f.y, 0, 0.0f, 0.0f, bw, bh, max_it, 0, &bk);
            if (bk.status != VO_KLT_OK) status = VO_KLT_BIDIR;
            else {
                e = vo_klt_bidir_error(bk.x, bk.y, x0, y0);
                if (!(e <= max_bidir)) status = VO_KLT_BIDIR;
            }
        }
        const int ok = status == VO_KLT_OK;
        pts1[2 * i] = ok ? f.x + 1.0f : pts0[2 * i];
        pts1[2 * i + 1] = ok ? f.y + 1.0f : pts0[2 * i + 1];
        valid[i] = (uint8_t)ok;
        if (scores) scores[i] = ok ? f.score : 0.0f;
        if (info) {
            info[i].status = (uint8_t)status; info[i].stop = (uint8_t)f.stop; info[i].iterations = (uint8_t)f.iterations;
            info[i].levels_skipped = (uint8_t)f.skipped; info[i].bidir_error = e;
        }
        if (level_codes) memcpy(level_codes + (long)i * VO_KLT_MAX_LEVELS, f.lv, VO_KLT_MAX_LEVELS);
    }
}
