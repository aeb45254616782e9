/* CPU reference of vo_refine_pose (test infrastructure): include/vo_spec.h's own vo_refine_*
 * functions -- the ones k_refine_pose calls -- around a pass that sums the points in the normative
 * order (64 partials, partial l the points k = l mod 64 ascending, then vo_tree_sum), compiled with
 * the oracle's flags (no contraction, no fast-math).
 * img [n][2], world [n][3], use [n] or NULL (= all), K 3x3 and T_in 4x4 row-major ->
 * T_out 4x4, stat = {status, n_used, passes, accepted}, cost = {cost_initial, cost_final}.
 * T_out is T_in by bytes when no step was accepted. */
#include <stdint.h>
#include <string.h>
#include "vo_spec.h"

static void pass(const double* R, const double* t, const double* z0, const double* K, const double* img, const double* world,
                 const uint8_t* use, int n, double* sums, int* n_used, int* behind)
{
    static double p[VO_REFINE_LANES][VO_REFINE_NSUM];
    int cnt = 0;
    *behind = 0;
    for (int l = 0; l < VO_REFINE_LANES; ++l) {
        for (int q = 0; q < VO_REFINE_NSUM; ++q) p[l][q] = 0.0;
        for (int k = l; k < n; k += VO_REFINE_LANES)
            cnt += vo_refine_point(R, t, z0, K, world + 3 * k, img + 2 * k, use ? use[k] : 1, p[l], behind);
    }
    vo_tree_sum(&p[0][0], VO_REFINE_NSUM, VO_REFINE_NSUM);
    for (int q = 0; q < VO_REFINE_NSUM; ++q) sums[q] = p[0][q];
    *n_used = cnt;
}

void pose_refine_ref(const double* img, const double* world, int n, const uint8_t* use, const double* K, const double* T_in,
                     int max_iterations, double relative_tolerance, double absolute_tolerance, double lambda0,
                     double* T_out, int32_t* stat, double* cost)
{
    double R[9], t[3], z0[4], sums[VO_REFINE_NSUM];
    int n_used = 0, behind = 0;
    vo_refine_state st;
    vo_refine_from_T(T_in, R, t);
    z0[0] = R[6]; z0[1] = R[7]; z0[2] = R[8]; z0[3] = t[2];
    vo_refine_begin(&st, R, t, lambda0);
    pass(st.R, st.t, z0, K, img, world, use, n, sums, &n_used, &behind);
    vo_refine_first(&st, sums, n_used);
    while (vo_refine_propose(&st, max_iterations)) {
        int m;
        pass(st.Rc, st.tc, z0, K, img, world, use, n, sums, &m, &behind);
        vo_refine_update(&st, sums, behind, relative_tolerance, absolute_tolerance);
    }
    if (st.accepted > 0) vo_refine_to_T(st.R, st.t, T_out);
    else memcpy(T_out, T_in, sizeof(double) * 16);
    stat[0] = st.status; stat[1] = st.n_used; stat[2] = st.passes; stat[3] = st.accepted;
    cost[0] = st.c0; cost[1] = st.c;
}

/* the pieces, for the tests that hold them to an independent evaluation */
void pose_refine_pass(const double* img, const double* world, int n, const uint8_t* use, const double* K, const double* T,
                      double* sums, int32_t* n_used)
{
    double R[9], t[3], z0[4];
    int m = 0, behind = 0;
    vo_refine_from_T(T, R, t);
    z0[0] = R[6]; z0[1] = R[7]; z0[2] = R[8]; z0[3] = t[2];
    pass(R, t, z0, K, img, world, use, n, sums, &m, &behind);
    *n_used = m;
}
