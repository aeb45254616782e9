/* CPU reference of triangulate's reprojectionErrors / validIndex (test infrastructure):
 * include/vo_spec.h's own vo_tri_quality -- the function k_tri_quality calls -- over arrays,
 * compiled with the oracle's flags (no contraction, no fast-math).
 * x1, x2 [n][2] single pixel positions, X [n][3] the doubles vo_triangulate returns, P1 / P2 3x4
 * row-major -> err [n], valid [n]. */
#include <stdint.h>
#include "vo_spec.h"

void tri_quality_ref(const float* x1, const float* x2, const double* X, int n, const double* P1, const double* P2,
                     float* err, uint8_t* valid)
{
    for (int k = 0; k < n; ++k)
        valid[k] = (uint8_t)vo_tri_quality(X + 3 * k, x1[2 * k], x1[2 * k + 1], x2[2 * k], x2[2 * k + 1], P1, P2, err + k);
}
