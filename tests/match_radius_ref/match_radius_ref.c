/* CPU build of matchFeaturesInRadius' two spec functions (test infrastructure): include/vo_spec.h's
 * own vo_radius_gate and vo_radius_box_lb -- the text k_match_radius compiles -- over arrays,
 * compiled with the oracle's flags (no contraction, no fast-math).
 * radius_gate_ref: points2 [n2][2], centers [n1][2], radius [n_radius] (1 or n1), r2 = r * r in
 * float32 as k_radius_meta forms it -> in [n1][n2] (1 = column j is a candidate of row i).
 * radius_box_ref: boxes [nb][4] = {xmin, xmax, ymin, ymax}, points [n][2] -> lb [n][nb]. */
#include <stddef.h>
#include <stdint.h>
#include "vo_spec.h"

void radius_gate_ref(const float* points2, int n2, const float* centers, int n1, const float* radius, int n_radius, uint8_t* in)
{
    for (int i = 0; i < n1; ++i) {
        const float r = radius[n_radius == 1 ? 0 : i];
        const float r2 = r * r;
        for (int j = 0; j < n2; ++j)
            in[(size_t)i * n2 + j] = (uint8_t)vo_radius_gate(points2[2 * j], points2[2 * j + 1], centers[2 * i], centers[2 * i + 1], r2);
    }
}

void radius_box_ref(const float* boxes, int nb, const float* points, int n, float* lb)
{
    for (int i = 0; i < n; ++i)
        for (int b = 0; b < nb; ++b)
            lb[(size_t)i * nb + b] = vo_radius_box_lb(boxes[4 * b], boxes[4 * b + 1], boxes[4 * b + 2], boxes[4 * b + 3],
                                                      points[2 * i], points[2 * i + 1]);
}
