/*
 * describe_ref.c — CPU reference of vo_describe: the descriptor of caller-given points.
 * TEST INFRASTRUCTURE ONLY.
 *
 * The oracle's scale space and descriptor are static functions of oracle/sift_ref.c; including
 * that file reaches build_pyramid, descriptor and free_pyramid as they are, without copying or
 * editing them.  What this file adds is the spec of include/vo.h ("extractFeatures at
 * caller-given points"): the inverse of oracle_sift's output mapping, from a vo_keypoint's public
 * fields back to descriptor()'s inputs.
 *
 * Built with oracle/Makefile's CFLAGS (-ffp-contract=off: every float op an IEEE basic op).
 */
#include "../../oracle/sift_ref.c"

/* the uncapped descriptor window radius of an octave-relative scale (descriptor()'s expression) */
int describe_ref_radius(float scl)
{
    const float hist_width = VO_SIFT_DESCR_SCL * scl;
    return vo_round(hist_width * 1.4142135623730951f * (float)(VO_SIFT_DESCR_W + 1) * 0.5f);
}

/* desc[n][128] of pts[0..n) on img.  Returns n; -1 for a parameter block the oracle refuses;
 * -(2 + i) when point i names an octave or a level the pyramid does not have. */
int describe_ref(const uint8_t* img, int rows, int cols, int ld, const vo_sift_params* p, const vo_keypoint* pts, int n,
                 uint8_t* desc)
{
    if (!oracle_sift_params_ok(p)) return -1;
    pyramid_t py;
    build_pyramid(img, rows, cols, ld, p, &py);
    int rc = n;
    for (int i = 0; i < n; ++i) {
        const vo_keypoint* q = &pts[i];
        const int o = q->octave + (p->upsample ? 1 : 0);
        if (o < 0 || o >= py.n_oct || q->layer < 0 || q->layer > py.L + 2) { rc = -(2 + i); break; }
        const octave_t* oc = &py.oct[o];
        const float oscale = (float)(1 << o) * (p->upsample ? 0.5f : 1.0f);
        const float loc_off = p->upsample ? 0.75f : 1.0f;
        const float xo = (q->x - loc_off) / oscale, yo = (q->y - loc_off) / oscale, scl = q->scale / oscale;
        descriptor(oc->g[q->layer], oc->rows, oc->cols, xo, yo, q->angle, scl, desc + (size_t)i * VO_DESC_LEN);
    }
    free_pyramid(&py);
    return rc;
}
