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
