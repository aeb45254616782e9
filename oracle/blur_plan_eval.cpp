/*
 * blur_plan_eval.cpp — exports csrc/blur_plan.h (the launch plan of the scale-space blurs,
 * plain host C++) so tests/test_blur_plan.py can pin it.  TEST INFRASTRUCTURE ONLY.
 */
#include "blur_plan.h"

/* out[f][i][j], f = 0 streamed, 1 cpl, 2 tag, 3 th, 4 n_bands, 5 n_strips, 6 full_bands, of
 * blur_plan(role, R[i], C[j], n_img, r); role: 0 level, 1 base from a float plane, 2 base from u8 */
extern "C" void blur_plan_sweep(int role, int r, int n_img, const int* R, int nR, const int* C, int nC, int* out)
{
    const long n = (long)nR * nC;
    for (int i = 0; i < nR; ++i)
        for (int j = 0; j < nC; ++j) {
            const vo::BlurPlan p = vo::blur_plan((vo::BlurRole)role, R[i], C[j], n_img, r);
            int* o = out + (long)i * nC + j;
            o[0 * n] = p.streamed; o[1 * n] = p.cpl; o[2 * n] = p.tag; o[3 * n] = p.th;
            o[4 * n] = p.n_bands; o[5 * n] = p.n_strips; o[6 * n] = p.full_bands;
        }
}

extern "C" int blur_plan_bs_p(void) { return BS_P; }

/* the LDS sizing of k_blur_stream and the staged u8 base's row range, for tests/blur_census.py */
extern "C" int blur_plan_bs_rw(int r, int cpl) { return vo::bs_rw(r, cpl); }
extern "C" int blur_plan_bs_sw(int r, int cpl, int tag) { return vo::bs_sw(r, cpl, tag); }
extern "C" int blur_plan_bs_hl(int r, int cpl, int tag) { return vo::bs_hl(r, cpl, tag); }
extern "C" int blur_plan_bs_u8_dw(int r, int cpl) { return vo::bs_u8_dw(r, cpl); }
extern "C" int blur_plan_bs_u8_rows(int r) { return vo::bs_u8_rows(r); }
extern "C" int blur_plan_base_max_th(void) { return vo::kBaseMaxTH; }
/* out[0], out[1] = the source rows [sr0, sr1] that the band of th rows from row y0 stages */
extern "C" void blur_plan_u8_stage_rows(int r, int R, int src_rows, int y0, int th, int* out)
{
    const vo::BsU8Rows s = vo::bs_u8_stage_rows(r, R, src_rows, y0, th);
    out[0] = s.sr0; out[1] = s.sr1;
}
/* the most source rows any band of an R-row plane stages at band height th, with the bands as
 * k_blur_stream cuts them: y0 = band * th, the last band cut to the plane in whole BS_P-row blocks */
extern "C" int blur_plan_u8_stage_max(int r, int R, int src_rows, int th)
{
    int most = 0;
    for (int y0 = 0; y0 < R; y0 += th) {
        const int cut = (R - y0 + BS_P - 1) / BS_P * BS_P;
        const vo::BsU8Rows s = vo::bs_u8_stage_rows(r, R, src_rows, y0, th < cut ? th : cut);
        if (s.sr1 - s.sr0 + 1 > most) most = s.sr1 - s.sr0 + 1;
    }
    return most;
}
