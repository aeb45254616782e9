/* CPU reference of vo_detect_corners (test infrastructure): include/vo_spec.h's vo_corner_* functions
 * around the normative loops of DESIGN.md 3.5.4.  The device kernels (csrc/corner.hip) give the same
 * bytes. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "vo_spec.h"

void corner_ref_weights(int f, int* q) { vo_corner_weights(f, q); }
float corner_ref_offset(float l, float z, float g) { return vo_corner_offset(l, z, g); }

/* the f32 metric plane [rows][cols] of a tightly packed u8 image; 0, or -1 when memory runs out */
int corner_ref_metric(const uint8_t* img, int rows, int cols, int method, int f, float* metric)
{
    const int R = (f - 1) / 2;
    int q[VO_CORNER_MAX_FILTER];
    vo_corner_weights(f, q);
    const size_t px = (size_t)rows * cols;
    int32_t* prod = malloc(sizeof(int32_t) * 3 * px);
    int32_t* hor = malloc(sizeof(int32_t) * 3 * px);
    if (!prod || !hor) { free(prod); free(hor); return -1; }
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const int ix = (int)img[(size_t)r * cols + vo_corner_clamp(c + 1, cols)] - (int)img[(size_t)r * cols + vo_corner_clamp(c - 1, cols)];
            const int iy = (int)img[(size_t)vo_corner_clamp(r + 1, rows) * cols + c] - (int)img[(size_t)vo_corner_clamp(r - 1, rows) * cols + c];
            const size_t o = (size_t)r * cols + c;
            prod[o] = ix * ix; prod[px + o] = iy * iy; prod[2 * px + o] = ix * iy;
        }
    for (int k = 0; k < 3; ++k)
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                int32_t h = 0;
                for (int j = 0; j < f; ++j) h += q[j] * prod[k * px + (size_t)r * cols + vo_corner_clamp(c + j - R, cols)];
                hor[k * px + (size_t)r * cols + c] = h;
            }
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            int64_t v[3];
            for (int k = 0; k < 3; ++k) {
                v[k] = 0;
                for (int i = 0; i < f; ++i) v[k] += (int64_t)q[i] * hor[k * px + (size_t)vo_corner_clamp(r + i - R, rows) * cols + c];
            }
            metric[(size_t)r * cols + c] = vo_corner_response(method, v[0], v[1], v[2]);
        }
    free(prod); free(hor);
    return 0;
}

typedef struct { uint64_t key; uint32_t at; } ranked;
static int by_key_desc(const void* a, const void* b)
{
    const uint64_t x = ((const ranked*)a)->key, y = ((const ranked*)b)->key;
    return x > y ? -1 : (x < y ? 1 : 0);
}

/* The detector on a tightly packed image.  roi: x y w h, 1-based, or NULL (the whole image; the caller
 * has checked it lies inside).  list_cap: the device list's capacity (4 x max_keypoints).  metric_plane
 * (may be NULL) receives the plane.  -> 0 with *n_out corners in loc [n][2] = (x, y), metric [n]; 1:
 * more corners than list_cap, or more to return than capacity (*n_out the true count, nothing
 * written); -1: out of memory. */
int corner_ref_detect(const uint8_t* img, int rows, int cols, int method, int f, float min_quality, int strongest, const int* roi,
                      int list_cap, float* metric_plane, float* loc, float* metric, int capacity, int* n_out)
{
    const size_t px = (size_t)rows * cols;
    float* m = metric_plane ? metric_plane : malloc(sizeof(float) * px);
    if (!m) return -1;
    int rc = corner_ref_metric(img, rows, cols, method, f, m);
    if (rc) { if (!metric_plane) free(m); return rc; }
    const int x0 = roi ? roi[0] - 1 : 0, y0 = roi ? roi[1] - 1 : 0, w = roi ? roi[2] : cols, h = roi ? roi[3] : rows;
    uint32_t mb = 0;
    for (int r = y0; r < y0 + h; ++r)
        for (int c = x0; c < x0 + w; ++c) {
            const uint32_t b = vo_corner_max_bits(m[(size_t)r * cols + c]);
            if (b > mb) mb = b;
        }
    const float mmax = vo_u32_as_f32(mb);
    const float thr = min_quality * mmax;
    /* count, then list (raster order) */
    long count = 0;
    if (mmax > 0.0f)
        for (int r = y0; r < y0 + h; ++r)
            for (int c = x0; c < x0 + w; ++c) count += vo_corner_is_corner(m, rows, cols, r, c, thr);
    const long n_ret = strongest > 0 && count > strongest ? strongest : count;
    *n_out = (int)(count > list_cap ? count : n_ret);
    if (count > list_cap || n_ret > capacity) { if (!metric_plane) free(m); return 1; }
    float* lx = malloc(sizeof(float) * 2 * (size_t)(count + 1));
    float* lm = malloc(sizeof(float) * (size_t)(count + 1));
    ranked* rk = malloc(sizeof(ranked) * (size_t)(count + 1));
    if (!lx || !lm || !rk) { free(lx); free(lm); free(rk); if (!metric_plane) free(m); return -1; }
    long k = 0;
    if (mmax > 0.0f)
        for (int r = y0; r < y0 + h; ++r)
            for (int c = x0; c < x0 + w; ++c)
                if (vo_corner_is_corner(m, rows, cols, r, c, thr)) {
                    vo_corner_location(m, rows, cols, r, c, &lx[2 * k], &lx[2 * k + 1]);
                    lm[k] = m[(size_t)r * cols + c];
                    rk[k].key = vo_corner_key(lm[k], (uint32_t)k);
                    rk[k].at = (uint32_t)k;
                    ++k;
                }
    if (strongest > 0) qsort(rk, (size_t)count, sizeof(ranked), by_key_desc);     /* keys are distinct */
    for (long i = 0; i < n_ret; ++i) {
        const uint32_t a = rk[i].at;
        loc[2 * i] = lx[2 * a]; loc[2 * i + 1] = lx[2 * a + 1]; metric[i] = lm[a];
    }
    free(lx); free(lm); free(rk);
    if (!metric_plane) free(m);
    return 0;
}
