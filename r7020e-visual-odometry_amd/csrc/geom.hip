// geom.hip — tracking + geometry stages of the per-frame path (see vo_geom.h).
//
//   find_remaining_points (VO.m:280-334)  four match jobs per frame whose row
//       sets are index lists; each step's finishing kernel (k_match_finish,
//       match.hip) composes its (i, j) pairs into the next step's lists, so no
//       descriptor is ever copied.
//   triangulate (VO.m:113-116)            k_gather_tri: one lane per tracked
//       point, linear DLT + one-sided Jacobi SVD in f64 (vo_dlt_point).
//   estworldpose (VO.m:123-127)           k_msac: one block per frame walks the
//       hypothesis slots in chunks of 64 -- a lane per slot (Philox sample,
//       Grunert P3P, 4th-point disambiguation), a wave per slot score
//       (lane-strided partial MSAC sums + fixed shuffle tree), then the
//       sequential adaptive-termination replay of the chunk -- until the replay
//       stops; msac_final: inlier mask + camera pose.
//   bundleAdjustmentMotion (after VO.m:123-127, optional)  k_refine_pose: one wave per frame runs
//       the Levenberg-Marquardt loop of vo_spec.h's vo_refine_* over the MSAC inliers and replaces
//       the frame's pose.
//   estimateFundamentalMatrix (after matchFeatures; vo_est_fundamental)  k_fund_msac: one block per
//       problem, k_msac's lazy chunks over vo_spec.h's vo_fund_* -- normalised 8-point hypotheses whose
//       9 x 9 Jacobi eigenproblems live in LDS, eight lanes per hypothesis; Sampson scores, the replay,
//       the best slot's mask and the masked refit in the same launch.
//   landmarks(VO.m:145-160, CreateLandmarksFromFeatures.m)  k_stereo_pos,
//       k_lm_filter (any-x-or-y equality test, quirk Q3) + block compaction,
//       k_lm_tri (odd rows, z gates).  (One fused block per frame measured
//       3.5x slower: 0.27 vs 0.075 ms per batch for positions + filter.)  The world transform needs the chained pose and runs
//       on the host after the 4x4 chain.
// The arithmetic of triangulate and estworldpose (DLT, P3P, the MSAC sample, bound, replay and pose)
// is vo_spec.h's, compiled here and by oracle/vo_ref.c; only the quartic's root finder exists in two
// forms (real_roots_trim below, real_roots there), operation for operation.
#include "vo_geom.h"
#include "wave.h"
#include <cstring>
#include <cstdlib>

namespace vo {

hipError_t geom_alloc(DevPool& pool, GeomBuffers& g, int max_frames, int kp_cap, int n_hyp)
{
    g.max_frames = max_frames; g.kp_cap = kp_cap; g.n_hyp = n_hyp;
    const size_t F = max_frames, K = kp_cap;
    hipError_t e = (hipError_t)pool.group({
        DevPool::req(g.lists, F * TL_COUNT * K), DevPool::req(g.list_n, F * 4), DevPool::req(g.step_i, 4 * F * K),
        DevPool::req(g.step_j, 4 * F * K), DevPool::req(g.step_n, 4 * F), DevPool::req(g.world, F * K * 3),
        DevPool::req(g.imgpt, F * K * 2), DevPool::req(g.oldpos, F * K * 4), DevPool::req(g.inliers, F * K),
        DevPool::req(g.hyp, F * n_hyp), DevPool::req(g.fg, F), DevPool::req(g.spos, F * K * 4), DevPool::req(g.s_n, F),
        DevPool::req(g.lm_new, F * K), DevPool::req(g.lm_M, F), DevPool::req(g.lm_X, F * K * 3),
        DevPool::req(g.lm_keep, F * K), DevPool::req(g.lm_rows, F)});
    if (e == hipSuccess) e = hipMemset(g.step_n, 0, sizeof(int) * 4 * F);
    if (e == hipSuccess) e = hipMemset(g.list_n, 0, sizeof(int) * 4 * F);
    return e;
}

hipError_t geom_alloc_refine(DevPool& pool, GeomBuffers& g)
{
    return g.refine ? hipSuccess : (hipError_t)pool.alloc(g.refine, (size_t)g.max_frames);
}

static inline int* glist(const GeomBuffers& g, int f, int l) { return g.lists + ((size_t)f * TL_COUNT + l) * g.kp_cap; }

void geom_fill_track_jobs(const GeomBuffers& g, MatchJob* jobs, int M, int first, const SiftBuffers& sb,
                          int* pair_i, int* pair_j, int* pair_n, int kp_cap)
{
    const size_t ds = (size_t)kp_cap * VO_DESC_LEN;
    auto D = [&](int slot) { return (const uint8_t*)(sb.desc + slot * ds); };
    auto Mt = [&](int slot) { return (const DescMeta*)(sb.meta + (size_t)slot * kp_cap); };
    for (int f = 0; f < M; ++f) {
        const int cl = 2 * f, cr = 2 * f + 1;
        const int pl = f ? 2 * (f - 1) : 2 * M, pr = pl + 1;
        const int pp = f ? f - 1 : M;
        for (int s = 0; s < 4; ++s) {
            MatchJob& J = jobs[first + s * M + f];
            memset(&J, 0, sizeof(J));
            J.out_i = g.step_i + ((size_t)s * M + f) * kp_cap;
            J.out_j = g.step_j + ((size_t)s * M + f) * kp_cap;
            J.out_n = g.step_n + s * M + f;
            J.cap = kp_cap;
        }
        // step 0: lm = matchFeatures(cur.l_desc, old.l_desc)            VO.m:283
        MatchJob& J0 = jobs[first + 0 * M + f];
        J0.d1 = D(cl); J0.m1 = Mt(cl); J0.idx1 = nullptr; J0.n1 = sb.n_kp + cl;
        J0.d2 = D(pl); J0.m2 = Mt(pl); J0.idx2 = pair_i + (size_t)pp * kp_cap; J0.n2 = pair_n + pp;
        // step 1: rm = matchFeatures(cur.r_desc, old.r_desc)            VO.m:293
        MatchJob& J1 = jobs[first + 1 * M + f];
        J1.d1 = D(cr); J1.m1 = Mt(cr); J1.idx1 = nullptr; J1.n1 = sb.n_kp + cr;
        J1.d2 = D(pr); J1.m2 = Mt(pr); J1.idx2 = glist(g, f, TL_OR1); J1.n2 = g.list_n + 4 * f + 0;
        // step 2: cm = matchFeatures(cur.l_desc, cur.r_desc)            VO.m:311
        MatchJob& J2 = jobs[first + 2 * M + f];
        J2.d1 = D(cl); J2.m1 = Mt(cl); J2.idx1 = glist(g, f, TL_CL); J2.n1 = g.list_n + 4 * f + 0;
        J2.d2 = D(cr); J2.m2 = Mt(cr); J2.idx2 = glist(g, f, TL_CR); J2.n2 = g.list_n + 4 * f + 1;
        // step 3: last = matchFeatures(cur.l_desc, old.l_desc)          VO.m:323
        MatchJob& J3 = jobs[first + 3 * M + f];
        J3.d1 = D(cl); J3.m1 = Mt(cl); J3.idx1 = glist(g, f, TL_CL2); J3.n1 = g.list_n + 4 * f + 2;
        J3.d2 = D(pl); J3.m2 = Mt(pl); J3.idx2 = glist(g, f, TL_OL2); J3.n2 = g.list_n + 4 * f + 1;
    }
}

// ---------------------------------------------------------------------------
// DLT triangulation (vo_spec.h vo_dlt_point)
// ---------------------------------------------------------------------------
struct CalibDev { double P1[12], P2[12], K[9]; };

// gather tracked positions and triangulate the old stereo pair. grid (blocks, B)
__global__ void k_gather_tri(const vo_keypoint* __restrict__ kp, int kp_cap, const int* __restrict__ lists,
                             const int* __restrict__ list_n, float* __restrict__ oldpos, double* __restrict__ imgpt,
                             double* __restrict__ world, int M, CalibDev cal)
{
    const int f = blockIdx.y, K = kp_cap;
    int n = list_n[4 * f + 3];
    const int cl = 2 * f;
    const int pl = f ? 2 * (f - 1) : 2 * M, pr = pl + 1;
    const int* L = lists + (size_t)f * TL_COUNT * K;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const vo_keypoint ol = kp[(size_t)pl * K + L[TL_OLF * K + k]];
        const vo_keypoint orr = kp[(size_t)pr * K + L[TL_ORF * K + k]];
        const vo_keypoint cu = kp[(size_t)cl * K + L[TL_CLF * K + k]];
        float* op = oldpos + ((size_t)f * K + k) * 4;
        op[0] = ol.x; op[1] = ol.y; op[2] = orr.x; op[3] = orr.y;
        double* ip = imgpt + ((size_t)f * K + k) * 2;
        ip[0] = cu.x; ip[1] = cu.y;
        double X[3];
        vo_dlt_point(ol.x, ol.y, orr.x, orr.y, cal.P1, cal.P2, X);
        double* w = world + ((size_t)f * K + k) * 3;
        w[0] = X[0]; w[1] = X[1]; w[2] = X[2];
    }
}

// standalone triangulation of position quads (x1, y1, x2, y2)
__global__ void k_tri_list(const float* __restrict__ pos, int n, CalibDev cal, double* __restrict__ X)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        double Y[3];
        vo_dlt_point(pos[4 * k], pos[4 * k + 1], pos[4 * k + 2], pos[4 * k + 3], cal.P1, cal.P2, Y);
        X[3 * k] = Y[0]; X[3 * k + 1] = Y[1]; X[3 * k + 2] = Y[2];
    }
}

// triangulate's reprojectionErrors / validIndex (vo_spec.h vo_tri_quality) of triangulated quads:
// one lane per point, grid (blocks, frames).  Frame f: n[f * n_stride] points (clamped to cap),
// quads pos + f * cap * 4, points X + f * cap * 3; err / valid are one frame's [cap] entries per
// frame.  Launched only by vo_triangulate_ex and vo_fetch_track_quality, never by a step.
__global__ void k_tri_quality(const float* __restrict__ pos, const double* __restrict__ X, const int* __restrict__ n,
                              int n_stride, int n_val, int cap, CalibDev cal, float* __restrict__ err,
                              uint8_t* __restrict__ valid)
{
    const int f = blockIdx.y;
    int m = n ? n[(size_t)f * n_stride] : n_val;
    m = m < 0 ? 0 : (m > cap ? cap : m);
    const float4* q = reinterpret_cast<const float4*>(pos) + (size_t)f * cap;
    const double* Xf = X + (size_t)f * cap * 3;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < m; k += gridDim.x * blockDim.x) {
        const float4 p = q[k];
        const double Y[3] = {Xf[3 * k], Xf[3 * k + 1], Xf[3 * k + 2]};
        float e;
        const int ok = vo_tri_quality(Y, p.x, p.y, p.z, p.w, cal.P1, cal.P2, &e);
        err[(size_t)f * cap + k] = e;
        valid[(size_t)f * cap + k] = (uint8_t)ok;
    }
}

// ---------------------------------------------------------------------------
// P3P (vo_spec.h vo_p3p_setup / vo_p3p_pose) — the deterministic bracketing/bisection
// root finder that runs between the two (template recursion = the oracle's real_roots).
// ---------------------------------------------------------------------------
// Register-resident form: every array index is a compile-time constant (fixed-degree solvers
// selected by a switch on the trimmed degree, roots appended through select chains), so the
// coefficients, critical points and roots stay in VGPRs -- the dynamically indexed form
// lived in scratch and its bisection loop waited on scratch loads every iteration.  Same
// operations in the same order as the oracle (real_roots in oracle/vo_ref.c): the trim
// keeps the largest i >= 1 with !(|a_i| <= 1e-14 amax), Horner as r = r*x + a_i.
template <int D>
__device__ __forceinline__ double peval_fixed(const double* a, double x)
{
    double r = a[D];
#pragma unroll
    for (int i = D - 1; i >= 0; --i) r = r * x + a[i];
    return r;
}

template <int N>
__device__ __forceinline__ void push_root(double* r, int& nr, double v)
{
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (i == nr) r[i] = v;
    nr++;
}

template <int MAXD>
__device__ int real_roots_trim(const double* a, double* roots);

// one bracketed interval: an exact zero at lo, or bisection to adjacent doubles (<= 200 halvings)
template <int D, int N>
__device__ __forceinline__ void bisect_interval(const double* a, double lo, double hi, double* roots, int& nr,
                                                double& last)
{
    double flo = peval_fixed<D>(a, lo), fhi = peval_fixed<D>(a, hi);
    if (flo == 0.0) {
        if (nr == 0 || last != lo) { push_root<N>(roots, nr, lo); last = lo; }
        return;
    }
    if ((flo < 0) == (fhi < 0)) return;
    for (int it = 0; it < 200; ++it) {
        double mid = 0.5 * (lo + hi);
        if (mid <= lo || mid >= hi) break;
        double fm = peval_fixed<D>(a, mid);
        if (fm == 0.0) { lo = hi = mid; break; }
        if ((fm < 0) == (flo < 0)) { lo = mid; flo = fm; } else hi = mid;
    }
    last = 0.5 * (lo + hi);
    push_root<N>(roots, nr, last);
}

// exact degree D >= 3: critical points from the derivative, then one bisection per bracket
template <int D>
__device__ __forceinline__ int real_roots_fixed(const double* a, double* roots)
{
    double d[D];
#pragma unroll
    for (int i = 1; i <= D; ++i) d[i - 1] = a[i] * (double)i;
    double crit[D - 1];
    const int nc = real_roots_trim<D - 1>(d, crit);
    double B = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) { double t = fabs(a[i] / a[D]); if (t > B) B = t; }
    B = B + 1.0;
    int nr = 0;
    double last = 0.0, prev = -B;
#pragma unroll
    for (int k = 0; k < D - 1; ++k) {
        if (k < nc && crit[k] > -B && crit[k] < B) {
            bisect_interval<D, D>(a, prev, crit[k], roots, nr, last);
            prev = crit[k];
        }
    }
    bisect_interval<D, D>(a, prev, B, roots, nr, last);
    return nr;
}

template <int MAXD>
__device__ int real_roots_trim(const double* a, double* roots)
{
    double amax = 0;
#pragma unroll
    for (int i = 0; i <= MAXD; ++i) if (fabs(a[i]) > amax) amax = fabs(a[i]);
    if (amax == 0.0) return 0;
    int deg = 0;
#pragma unroll
    for (int i = 1; i <= MAXD; ++i) if (!(fabs(a[i]) <= 1e-14 * amax)) deg = i;
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
    if constexpr (MAXD >= 4) {
        if (deg == 4) return real_roots_fixed<4>(a, roots);
    }
    if constexpr (MAXD >= 3) {
        return real_roots_fixed<3>(a, roots);
    }
    return 0;
}

struct MsacArgs {
    const double* img; const double* world; const int* n; int n_stride;   // n[f * n_stride]
    MsacHyp* hyp; FrameGeom* fg; uint8_t* inliers;
    int kp_cap, n_hyp, max_trials;
    double thr, conf;
    uint32_t seed;
    uint32_t key0;           // frame key of frame 0 (frame f uses key0 + f)
    double K[9];
};

__device__ __forceinline__ int msac_n(const MsacArgs& a, int f)
{
    int n = a.n[(size_t)f * a.n_stride];
    return n < 0 ? 0 : (n > a.kp_cap ? a.kp_cap : n);
}

// hypothesis slot s of frame f: Philox sample, Grunert P3P, 4th-point disambiguation
__device__ void msac_hyp_slot(const MsacArgs& a, int f, int s, int n)
{
    MsacHyp* h = a.hyp + (size_t)f * a.n_hyp + s;
    h->valid = 0;
    if (n < 4 || s >= a.max_trials) return;
    const double* img = a.img + (size_t)f * a.kp_cap * 2;
    const double* world = a.world + (size_t)f * a.kp_cap * 3;
    uint32_t idx[4];
    if (!vo_pose_sample(a.seed, a.key0 + (uint32_t)f, (uint32_t)s, (uint32_t)n, idx)) return;
    double im3[3][2], w3[3][3];
    for (int q = 0; q < 3; ++q) {
        im3[q][0] = img[2 * idx[q]]; im3[q][1] = img[2 * idx[q] + 1];
        for (int i = 0; i < 3; ++i) w3[q][i] = world[3 * idx[q] + i];
    }
    vo_p3p p;
    if (!vo_p3p_setup(im3, w3, a.K, &p)) return;
    double roots[4];
    const int nr = real_roots_trim<4>(p.P, roots);
    // of at most four poses, the one with the smallest error at the 4th point (the first of equals)
    double R[9], t[3], be = INFINITY;
    int ns = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k >= nr) break;
        double Rk[9], tk[3];
        if (!vo_p3p_pose(&p, w3, roots[k], Rk, tk)) continue;
        const double e = vo_pose_reproj_err2(Rk, tk, a.K, world + 3 * idx[3], img + 2 * idx[3]);
        if (e < be) {
            be = e;
            for (int q = 0; q < 9; ++q) R[q] = Rk[q];
            for (int q = 0; q < 3; ++q) t[q] = tk[q];
        }
        if (++ns == 4) break;
    }
    if (!(be < INFINITY)) return;
    for (int q = 0; q < 9; ++q) h->R[q] = R[q];
    for (int q = 0; q < 3; ++q) h->t[q] = t[q];
    h->valid = 1;
}

// MSAC score of one valid slot by one wave: 64 lane-strided partials + the fixed tree (wave_sum)
__device__ __forceinline__ void msac_score_slot(const MsacArgs& a, int f, int s, int n, int lane)
{
    MsacHyp* h = a.hyp + (size_t)f * a.n_hyp + s;
    const double* img = a.img + (size_t)f * a.kp_cap * 2;
    const double* world = a.world + (size_t)f * a.kp_cap * 3;
    double R[9], tt[3];
    for (int q = 0; q < 9; ++q) R[q] = h->R[q];
    for (int q = 0; q < 3; ++q) tt[q] = h->t[q];
    double part = 0.0;
    int cnt = 0;
    for (int k = lane; k < n; k += 64) {
        double e = vo_pose_reproj_err2(R, tt, a.K, world + 3 * k, img + 2 * k);
        if (e < a.thr) cnt++;
        part = part + (e < a.thr ? e : a.thr);
    }
    part = wave_sum(part);
    cnt = wave_sum_xor(cnt);
    if (lane == 0) { h->score = part; h->n_in = cnt; }
}

// inlier mask + camera pose of the chosen slot (one wave)
__device__ void msac_final(const MsacArgs& a, int f, int n, int best, int status, int lane)
{
    FrameGeom* g = a.fg + f;
    if (status != VO_OK) {
        if (lane == 0) {
            g->n_inliers = 0;
            for (int q = 0; q < 16; ++q) g->T[q] = (q % 5 == 0) ? 1.0 : 0.0;
        }
        return;
    }
    const MsacHyp* h = a.hyp + (size_t)f * a.n_hyp + best;
    double R[9], t[3];
    for (int q = 0; q < 9; ++q) R[q] = h->R[q];
    for (int q = 0; q < 3; ++q) t[q] = h->t[q];
    const double* img = a.img + (size_t)f * a.kp_cap * 2;
    const double* world = a.world + (size_t)f * a.kp_cap * 3;
    int cnt = 0;
    for (int k = lane; k < n; k += 64) {
        const int in = vo_pose_reproj_err2(R, t, a.K, world + 3 * k, img + 2 * k) < a.thr;
        a.inliers[(size_t)f * a.kp_cap + k] = (uint8_t)in;
        cnt += in;
    }
    cnt = wave_sum(cnt);
    if (lane == 0) {
        g->n_inliers = cnt;
        vo_pose_to_T(R, t, g->T);
    }
}

// Lazy MSAC: one 1024-thread block per frame walks the slots in chunks of 64 -- generate the
// chunk's hypotheses (lane per slot), score its valid ones (wave per slot), replay the
// sequential adaptive-termination loop over the chunk (thread 0, state carried across chunks)
// -- and stops at the chunk where the replay stops.  At the ~97 % inlier ratios of the KITTI
// path the replay needs ~3 trials, so one chunk of 64 replaces 2048 eager slots.  Same
// slots, same per-slot arithmetic, same replay: results identical to the eager kernels.
#ifndef VO_MSAC_CHUNK
#define VO_MSAC_CHUNK 64          // slots per chunk after the first (<= 64: one lane per slot)
#endif
#ifndef VO_MSAC_FIRST
#define VO_MSAC_FIRST 64          // slots of the first chunk (<= VO_MSAC_CHUNK)
#endif
#ifndef VO_MSAC_T
#define VO_MSAC_T 1024            // 16 waves: a chunk's 64 slots scored 4 per wave (one block per frame)
#endif

__global__ __launch_bounds__(VO_MSAC_T) void k_msac(MsacArgs a)
{
    __shared__ int s_best, s_status, s_done;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = msac_n(a, f);
    const int limit = a.max_trials < a.n_hyp ? a.max_trials : a.n_hyp;
    FrameGeom* g = a.fg + f;
    vo_pose_replay r;                                       // thread 0's
    vo_pose_replay_begin(&r, a.max_trials);
    if (tid == 0) s_done = n < 4;
    __syncthreads();
    for (int c0 = 0, c1 = min(VO_MSAC_FIRST, limit); !s_done && c0 < limit;
         c0 = c1, c1 = min(c1 + VO_MSAC_CHUNK, limit)) {
        if (tid < c1 - c0) msac_hyp_slot(a, f, c0 + tid, n);
        __syncthreads();                                    // the chunk's slots are written
        for (int s = c0 + wv; s < c1; s += VO_MSAC_T / 64)
            if (a.hyp[(size_t)f * a.n_hyp + s].valid) msac_score_slot(a, f, s, n, lane);
        __syncthreads();                                    // ... and scored
        if (tid == 0) {
            for (int s = c0; s < c1 && !vo_pose_replay_done(&r); ++s) {
                const MsacHyp* h = a.hyp + (size_t)f * a.n_hyp + s;
                vo_pose_replay_slot(&r, s, h->valid, h->score, h->n_in, n, a.conf);
            }
            s_done = vo_pose_replay_done(&r);               // (the last chunk ends the loop by c0 < limit)
        }
        __syncthreads();
    }
    if (tid == 0) {
        int status = VO_OK;
        if (n < 4) status = VO_ERR_TOO_FEW_POINTS;
        else if (r.best < 0 || r.best_in < 4) status = VO_ERR_NO_CONSENSUS;
        s_best = r.best;
        s_status = status;
        g->status = status;
        g->best = r.best;
        g->n_tracked = n;
    }
    __syncthreads();
    if (wv) return;
    msac_final(a, f, n, s_best, s_status, lane);
}

// ---------------------------------------------------------------------------
// bundleAdjustmentMotion after estworldpose (VO.m:123-130; vo_spec.h vo_refine_*)
// ---------------------------------------------------------------------------
struct RefineArgs {
    const double* img; const double* world; const uint8_t* use; const int* n; int n_stride;   // n[f * n_stride]
    FrameGeom* fg; vo_refine_stats* stats;
    int kp_cap, need_ok;
    vo_refine_params p;
    double K[9];
};

// One pass of the wave over the frame's points: lane l sums the points k = l (mod 64) in ascending
// k, then wave_sum -- the fixed tree of msac_score_slot; all 64 lanes end with the bits of the
// tree's p[0], so every decision taken on the sums is wave-uniform.
__device__ __forceinline__ void refine_pass(const double* K, const double* img, const double* world, const uint8_t* use, int n,
                                            int lane, const double* R, const double* t, const double* z0, double* sums,
                                            int& n_used, int& behind)
{
#pragma unroll
    for (int q = 0; q < VO_REFINE_NSUM; ++q) sums[q] = 0.0;
    int cnt = 0, bh = 0;
    for (int k = lane; k < n; k += VO_REFINE_LANES)
        cnt += vo_refine_point(R, t, z0, K, world + 3 * k, img + 2 * k, use[k], sums, &bh);
    wave_sum_xor<VO_REFINE_NSUM>(sums);
    n_used = wave_sum_xor(cnt);
    behind = wave_sum_xor(bh) != 0;                         // bh is 0 or 1 per lane: any lane's
}

// Wave-uniform doubles moved, not computed (the bits stay): into scalar registers, and parked
// across a pass as lane q of one register pair.  The pass then holds its 28 accumulators and a
// point's temporaries in vector registers; the pose it runs at lives in scalar registers and the
// accepted pose with its H, g (39 doubles, dead weight during a pass) in two vector registers.
__device__ __forceinline__ double uniform_f64(double v)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ double unpark_f64(double pk, int q)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(pk), q), __builtin_amdgcn_readlane(__double2loint(pk), q));
}

// One wave per frame runs the whole Levenberg-Marquardt loop: no LDS, no barrier, no atomics.  The
// kernel is latency-bound like k_msac (a frame's points, 41 bytes each, stay in cache after the
// first pass).  Starts from fg[f].T and overwrites it when a step was accepted.
__global__ __launch_bounds__(64) void k_refine_pose(RefineArgs a)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    FrameGeom* g = a.fg + f;
    vo_refine_stats* so = a.stats + f;
    if (a.need_ok && g->status != VO_OK) {                  // MSAC failed, or frame 1: not refined
        if (lane == 0) {
            so->status = VO_REFINE_TOO_FEW; so->n_used = 0; so->passes = 0; so->accepted = 0;
            so->cost_initial = 0.0; so->cost_final = 0.0;
        }
        return;
    }
    int n = a.n[(size_t)f * a.n_stride];
    n = n < 0 ? 0 : (n > a.kp_cap ? a.kp_cap : n);
    const double* img = a.img + (size_t)f * a.kp_cap * 2;
    const double* world = a.world + (size_t)f * a.kp_cap * 3;
    const uint8_t* use = a.use + (size_t)f * a.kp_cap;
    double T[16], R[9], t[3], z0[4], sums[VO_REFINE_NSUM];
#pragma unroll
    for (int q = 0; q < 16; ++q) T[q] = g->T[q];
    vo_refine_from_T(T, R, t);
    z0[0] = uniform_f64(R[6]); z0[1] = uniform_f64(R[7]); z0[2] = uniform_f64(R[8]); z0[3] = uniform_f64(t[2]);
    vo_refine_state st;
    vo_refine_begin(&st, R, t, a.p.lambda0);
    int n_used, behind;
    refine_pass(a.K, img, world, use, n, lane, st.R, st.t, z0, sums, n_used, behind);
    vo_refine_first(&st, sums, n_used);
    while (vo_refine_propose(&st, a.p.max_iterations)) {
        double pk = 0.0, Rc[9], tc[3];
#pragma unroll
        for (int q = 0; q < 21; ++q) pk = lane == q ? st.H[q] : pk;
#pragma unroll
        for (int q = 0; q < 6; ++q) pk = lane == 21 + q ? st.g[q] : pk;
#pragma unroll
        for (int q = 0; q < 9; ++q) { pk = lane == 27 + q ? st.R[q] : pk; Rc[q] = uniform_f64(st.Rc[q]); }
#pragma unroll
        for (int q = 0; q < 3; ++q) { pk = lane == 36 + q ? st.t[q] : pk; tc[q] = uniform_f64(st.tc[q]); }
        int m;
        refine_pass(a.K, img, world, use, n, lane, Rc, tc, z0, sums, m, behind);
#pragma unroll
        for (int q = 0; q < 21; ++q) st.H[q] = unpark_f64(pk, q);
#pragma unroll
        for (int q = 0; q < 6; ++q) st.g[q] = unpark_f64(pk, 21 + q);
#pragma unroll
        for (int q = 0; q < 9; ++q) { st.R[q] = unpark_f64(pk, 27 + q); st.Rc[q] = Rc[q]; }
#pragma unroll
        for (int q = 0; q < 3; ++q) { st.t[q] = unpark_f64(pk, 36 + q); st.tc[q] = tc[q]; }
        vo_refine_update(&st, sums, behind, a.p.relative_tolerance, a.p.absolute_tolerance);
    }
    if (lane == 0) {
        if (st.accepted > 0) {
            vo_refine_to_T(st.R, st.t, T);
#pragma unroll
            for (int q = 0; q < 16; ++q) g->T[q] = T[q];
        }
        so->status = st.status; so->n_used = st.n_used; so->passes = st.passes; so->accepted = st.accepted;
        so->cost_initial = st.c0; so->cost_final = st.c;
    }
}

// ---------------------------------------------------------------------------
// estimateFundamentalMatrix (vo_est_fundamental; vo_spec.h vo_fund_*)
// ---------------------------------------------------------------------------
struct FundArgs {
    const float* x1; const float* x2; const int* n; int stride;    // problem f: x1 + f * stride * 2, n[f] points
    FundHyp* hyp; FundOut* out; uint8_t* inliers;                  // hyp [B][VO_FUND_CHUNK], inliers [B][stride]
    int method, num_trials;
    double thr, conf;
    uint32_t seed, key0;
};

#define VO_FUND_T 512             // 8 waves, two per SIMD: 256 VGPRs each, which the solve needs to stay out of scratch
#define VO_FUND_WAVES (VO_FUND_T / 64)
#define VO_FUND_GROUP 8           // lanes that share one hypothesis' 9x9 Jacobi: 64 slots x 8 lanes = the block
static_assert(VO_FUND_CHUNK == 64 && VO_FUND_CHUNK * VO_FUND_GROUP == VO_FUND_T, "one group of lanes per slot of the chunk");

// vo_fund_jacobi at 9 x 9 by a group of 8 lanes of one wave, lane g of the group.  A rotation's 16
// independent element pairs -- (a_kp, a_kq) for the 7 k outside {p, q}, (v_kp, v_kq) for the 9 rows --
// are two per lane: lane g < 7 takes the A pair of the g-th such k and V's row g + 1, lane 7 V's rows
// 0 and 8; lane 0 also writes a_pp, a_qq, a_pq.  Every lane evaluates vo_fund_rot on the same three
// values, so the skip and the sweep count are uniform in the group, and each element goes through
// vo_fund_rot_xy exactly as in the serial loop: the bits are vo_fund_jacobi's.  The group's lanes run
// in lockstep (one wave, the same control flow) and the LDS serves a wave's accesses in program order:
// within a rotation every load is issued before the first store, and no two lanes touch one element,
// so no barrier is needed; the accesses are volatile so that none is kept in a register or moved
// across another.  Ap, Vp: column i of the element-major block (stride VO_FUND_CHUNK).
typedef volatile __attribute__((address_space(3))) double lds_vf64;
__device__ __forceinline__ int fund_jacobi9_group(double* Ap, double* Vp, int g)
{
    lds_vf64* A = (lds_vf64*)Ap;                          // (named LDS: volatile accesses through a generic pointer stay flat)
    lds_vf64* V = (lds_vf64*)Vp;
    constexpr int n = 9, S = VO_FUND_CHUNK;
    for (int e = g; e < n * n; e += VO_FUND_GROUP) V[e * S] = (e / n == e % n) ? 1.0 : 0.0;
    for (int sweeps = 0; sweeps < VO_FUND_SWEEP_CAP; ++sweeps) {
        int rotated = 0;
        for (int p = 0; p < n - 1; ++p) {
            for (int q = p + 1; q < n; ++q) {
                const int ipp = vo_fund_tri(n, p, p) * S, iqq = vo_fund_tri(n, q, q) * S, ipq = vo_fund_tri(n, p, q) * S;
                const double apq = A[ipq], app = A[ipp], aqq = A[iqq];
                double t, c, s;
                if (vo_fund_rot(app, aqq, apq, &t, &c, &s)) continue;
                rotated = 1;
                int i0, i1;                                   // the lane's first pair
                if (g < 7) {
                    int k = g;
                    if (k >= p) ++k;
                    if (k >= q) ++k;
                    i0 = (k < p ? vo_fund_tri(n, k, p) : vo_fund_tri(n, p, k)) * S;
                    i1 = (k < q ? vo_fund_tri(n, k, q) : vo_fund_tri(n, q, k)) * S;
                } else {
                    i0 = p * S;                               // V's row 0
                    i1 = q * S;
                }
                lds_vf64* B = g < 7 ? A : V;
                const int r = g < 7 ? g + 1 : 8;              // ... and V's row r as the second
                const int j0 = (r * n + p) * S, j1 = (r * n + q) * S;
                double x0 = B[i0], y0 = B[i1], x1 = V[j0], y1 = V[j1];
                vo_fund_rot_xy(c, s, &x0, &y0);
                vo_fund_rot_xy(c, s, &x1, &y1);
                B[i0] = x0; B[i1] = y0;
                V[j0] = x1; V[j1] = y1;
                if (g == 0) {
                    A[ipp] = app - t * apq;
                    A[iqq] = aqq + t * apq;
                    A[ipq] = 0.0;
                }
            }
        }
        if (!rotated) break;
    }
    return vo_fund_argmin_diag(Ap, n, S);
}

// The solve of one column of W by its group: the 9 x 9 Jacobi by all lanes of the group, the rest
// (vo_fund_solve_tail: rank 2 with the serial 3 x 3 Jacobi, denormalisation) by the group's lane 0,
// which holds N1, N2 and gets F.  Called by whole waves; `member`: the lane's group has a slot,
// `ok` (uniform in the group): the slot has a design matrix.  -> the model flag, valid in lane 0.
__device__ __forceinline__ int fund_solve_group(double* W, int g, int member, int ok, const double* N1, const double* N2, double* F)
{
    int j9 = 0;
    if (member && ok) j9 = fund_jacobi9_group(W, W + VO_FUND_NSUM * VO_FUND_CHUNK, g);
    int res = 0;
    if (member && ok && g == 0) res = vo_fund_solve_tail(W, VO_FUND_CHUNK, j9, N1, N2, F, nullptr);
    return res;
}

// slot `slot` of the problem, as the chunk's slot i, by the group of 8 lanes tid / 8 == i: lane 0 of
// the group draws the sample and sums the design matrix into column i of the element-major LDS
// block W (element e at W[e * 64 + i]), the group solves it, lane 0 stores F.  Called by whole waves.
__device__ __forceinline__ void fund_hyp_slot(const FundArgs& a, const float* x1, const float* x2, int n, uint32_t key, int slot,
                                              int i, int member, int lane, double* W, FundHyp* hyp)
{
    const int g = lane & (VO_FUND_GROUP - 1);
    double N1[3], N2[3], F[9];
    int ok = 0;
    if (member && g == 0) {
        uint32_t idx[VO_FUND_SAMPLE];
        ok = vo_fund_sample(a.seed, key, (uint32_t)slot, (uint32_t)n, idx, nullptr);
        if (ok) ok = vo_fund_fit_sample(x1, x2, idx, N1, N2, W + i, VO_FUND_CHUNK);
    }
    ok = __shfl(ok, lane & ~(VO_FUND_GROUP - 1));
    ok = fund_solve_group(W + i, g, member, ok, N1, N2, F);
    if (member && g == 0) {
        FundHyp* h = hyp + i;
        h->valid = ok;
        if (ok) {
#pragma unroll
            for (int q = 0; q < 9; ++q) h->F[q] = F[q];
        }
    }
}

// MSAC score of one valid slot by one wave: 64 lane-strided partials + the fixed tree (msac_score_slot)
__device__ __forceinline__ void fund_score_slot(FundHyp* h, const float* x1, const float* x2, int n, double thr, int lane)
{
    double F[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) F[q] = h->F[q];
    double part = 0.0;
    int cnt = 0;
    for (int k = lane; k < n; k += VO_FUND_LANES) {
        const float2 p1 = ((const float2*)x1)[k], p2 = ((const float2*)x2)[k];
        double e = vo_fund_sampson(F, (double)p1.x, (double)p1.y, (double)p2.x, (double)p2.y);
        if (e < thr) cnt++;
        part = part + (e < thr ? e : thr);
    }
    part = wave_sum(part);
    cnt = wave_sum(cnt);
    if (lane == 0) { h->score = part; h->n_in = cnt; }
}

// The masked Norm8 fit by one wave: lane l is partial l of the three passes; the 45 sums of the last
// pass accumulate in LDS (column l of W), are joined through registers and land in column 0, which
// the wave's first group solves.  -> 1 and F (valid in lane 0), or 0, wave-uniform.
__device__ __forceinline__ int fund_refit(const float* x1, const float* x2, const uint8_t* mask, int n, int lane, double* W, double* F)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int m = 0;
    for (int k = lane; k < n; k += VO_FUND_LANES) {
        if (!mask[k]) continue;
        const float2 p1 = ((const float2*)x1)[k], p2 = ((const float2*)x2)[k];
        ++m;
        s0 = s0 + (double)p1.x; s1 = s1 + (double)p1.y; s2 = s2 + (double)p2.x; s3 = s3 + (double)p2.y;
    }
    m = wave_sum(m);
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
    double N1[3], N2[3];
    N1[1] = s0 / (double)m; N1[2] = s1 / (double)m; N2[1] = s2 / (double)m; N2[2] = s3 / (double)m;
    double d1 = 0.0, d2 = 0.0;
    for (int k = lane; k < n; k += VO_FUND_LANES) {
        if (!mask[k]) continue;
        const float2 p1 = ((const float2*)x1)[k], p2 = ((const float2*)x2)[k];
        d1 = d1 + vo_fund_dist((double)p1.x, (double)p1.y, N1[1], N1[2]);
        d2 = d2 + vo_fund_dist((double)p2.x, (double)p2.y, N2[1], N2[2]);
    }
    d1 = wave_sum(d1); d2 = wave_sum(d2);
    N1[0] = VO_FUND_SQRT2 / (d1 / (double)m);
    N2[0] = VO_FUND_SQRT2 / (d2 / (double)m);
    if (!vo_fund_finite(N1[0]) || !vo_fund_finite(N2[0])) return 0;            // wave-uniform: the sums are
    for (int q = 0; q < VO_FUND_NSUM; ++q) W[q * VO_FUND_CHUNK + lane] = 0.0;
    for (int k = lane; k < n; k += VO_FUND_LANES) {
        if (!mask[k]) continue;
        const float2 p1 = ((const float2*)x1)[k], p2 = ((const float2*)x2)[k];
        vo_fund_row(N1, N2, (double)p1.x, (double)p1.y, (double)p2.x, (double)p2.y, W + lane, VO_FUND_CHUNK);
    }
    for (int q = 0; q < VO_FUND_NSUM; ++q) {
        const double v = wave_sum(W[q * VO_FUND_CHUNK + lane]);
        if (lane == 0) W[q * VO_FUND_CHUNK] = v;
    }
    const int ok = fund_solve_group(W, lane & (VO_FUND_GROUP - 1), lane < VO_FUND_GROUP, 1, N1, N2, F);   // lanes 0 .. 7 on column 0
    return __shfl(ok, 0);
}

// One 512-thread block per problem, k_msac's lazy chunks: generate the chunk's 64 hypotheses (a
// group of 8 lanes each, so every lane of the block works on the Jacobi solves: fund_jacobi9_group),
// score the valid ones (wave per slot), replay the sequential loop over the chunk (thread 0), stop at
// the chunk where the replay stops; then the best slot's mask and the masked refit (wave 0) in the
// same launch.  Only the chunk's slots and the best F so far are kept: memory per problem does not
// grow with num_trials.  The 9x9 eigenproblem's 45 + 81 doubles per hypothesis live in LDS,
// element-major across the chunk (63 KiB), addressed with runtime indices there instead of in scratch.
__global__ __launch_bounds__(VO_FUND_T) void k_fund_msac(FundArgs a)
{
    __shared__ double s_w[VO_FUND_NWORK * VO_FUND_CHUNK];
    __shared__ double s_F[9];
    __shared__ int s_done, s_status;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int n = a.n[f];
    n = n < 0 ? 0 : (n > a.stride ? a.stride : n);
    const float* x1 = a.x1 + (size_t)f * a.stride * 2;
    const float* x2 = a.x2 + (size_t)f * a.stride * 2;
    FundHyp* hyp = a.hyp + (size_t)f * VO_FUND_CHUNK;
    FundOut* out = a.out + f;
    uint8_t* mask = a.inliers + (size_t)f * a.stride;
    const uint32_t key = a.key0 + (uint32_t)f;
    int status = n < VO_FUND_SAMPLE ? VO_ERR_TOO_FEW_POINTS : VO_OK;
    if (status == VO_OK && a.method == VO_FUND_MSAC) {
        vo_fund_replay r;                                   // thread 0's
        vo_fund_replay_begin(&r, a.num_trials);
        if (tid == 0) s_done = 0;
        __syncthreads();
        for (int c0 = 0; c0 < a.num_trials && !s_done; c0 += VO_FUND_CHUNK) {
            const int cn = min(VO_FUND_CHUNK, a.num_trials - c0);
            const int i = tid / VO_FUND_GROUP;
            fund_hyp_slot(a, x1, x2, n, key, c0 + i, i, i < cn, lane, s_w, hyp);
            __syncthreads();                                    // the chunk's slots are written
            for (int s = wv; s < cn; s += VO_FUND_WAVES)
                if (hyp[s].valid) fund_score_slot(hyp + s, x1, x2, n, a.thr, lane);
            __syncthreads();                                    // ... and scored
            if (tid == 0) {
                for (int s = 0; s < cn && !vo_fund_replay_done(&r); ++s) {
                    const FundHyp* h = hyp + s;
                    if (vo_fund_replay_slot(&r, c0 + s, h->valid, h->score, h->n_in, n, a.conf)) {
#pragma unroll
                        for (int q = 0; q < 9; ++q) s_F[q] = h->F[q];
                    }
                }
                s_done = vo_fund_replay_done(&r);
            }
            __syncthreads();
        }
        if (tid == 0) s_status = (r.best < 0 || r.best_in < VO_FUND_SAMPLE) ? VO_ERR_NO_CONSENSUS : VO_OK;
        __syncthreads();
        status = s_status;
    }
    if (status == VO_OK) {                                  // the mask the refit runs over
        double F[9];
        if (a.method == VO_FUND_MSAC) {
#pragma unroll
            for (int q = 0; q < 9; ++q) F[q] = s_F[q];
        }
        for (int k = tid; k < n; k += VO_FUND_T) {
            int in = 1;
            if (a.method == VO_FUND_MSAC) {
                const float2 p1 = ((const float2*)x1)[k], p2 = ((const float2*)x2)[k];
                in = vo_fund_sampson(F, (double)p1.x, (double)p1.y, (double)p2.x, (double)p2.y) < a.thr;
            }
            mask[k] = (uint8_t)in;
        }
        __syncthreads();                                    // the mask is written (status is block-uniform)
    }
    if (wv) return;
    double F[9];
    int cnt = 0;
    if (status == VO_OK) {
        for (int k = lane; k < n; k += VO_FUND_LANES) cnt += mask[k];
        cnt = wave_sum(cnt);
        if (!fund_refit(x1, x2, mask, n, lane, s_w, F)) status = VO_ERR_NO_CONSENSUS;
    }
    if (status != VO_OK) {
        cnt = 0;
        for (int k = lane; k < n; k += VO_FUND_LANES) mask[k] = 0;
    }
    for (int k = n + lane; k < a.stride; k += VO_FUND_LANES) mask[k] = 0;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 9; ++q) out->F[q] = status == VO_OK ? F[q] : 0.0;
        out->status = status;
        out->n_inliers = cnt;
    }
}

// ---------------------------------------------------------------------------
// landmarks
// ---------------------------------------------------------------------------
// stereo subset positions of frame f (VO.m:141-142): spos[f][j] = (lx, ly, rx, ry)
__global__ void k_stereo_pos(const vo_keypoint* __restrict__ kp, int kp_cap, const int* __restrict__ pair_i,
                             const int* __restrict__ pair_j, const int* __restrict__ pair_n, float* __restrict__ spos,
                             int* __restrict__ s_n)
{
    const int f = blockIdx.y, K = kp_cap;
    int n = pair_n[f];
    if (n > K) n = K;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const vo_keypoint l = kp[(size_t)(2 * f) * K + pair_i[(size_t)f * K + j]];
        const vo_keypoint r = kp[(size_t)(2 * f + 1) * K + pair_j[(size_t)f * K + j]];
        float* p = spos + ((size_t)f * K + j) * 4;
        p[0] = l.x; p[1] = l.y; p[2] = r.x; p[3] = r.y;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) s_n[f] = n;
}

// new-landmark filter (VO.m:147-154) + compaction.  one block (1024) per frame.
// old positions: oldpos[f][k] (x1, y1, x2, y2) for k < *kn (kn[f * kn_stride]).
// flags: per-frame byte scratch (lm_keep, rewritten later by k_lm_tri).
__global__ __launch_bounds__(1024) void k_lm_filter(const float* __restrict__ spos, const int* __restrict__ s_n,
                                                    const float* __restrict__ oldpos, const int* __restrict__ kn,
                                                    int kn_stride, int kp_cap, uint8_t* __restrict__ flags,
                                                    int* __restrict__ lm_new, int* __restrict__ lm_M,
                                                    int* __restrict__ lm_rows)
{
    // One block per frame.  Stereo matches are taken 1024 at a time (one per thread,
    // rounds keep the ascending order of the compaction); the old points are staged
    // through LDS 1024 at a time and every thread compares its match against all of
    // them (broadcast reads).  hit = any old left x == lx or any old left y == ly, or
    // likewise on the right (VO.m:150-151, exact float equality).
    __shared__ uint32_t sh[16];
    __shared__ float4 so[1024];
    const int f = blockIdx.x, tid = threadIdx.x, K = kp_cap;
    int S = s_n[f];
    if (S > K) S = K;
    int nk = kn[(size_t)f * kn_stride];
    if (nk > K) nk = K;
    if (nk < 0) nk = 0;
    const float4* sp = reinterpret_cast<const float4*>(spos + (size_t)f * K * 4);
    const float4* op = reinterpret_cast<const float4*>(oldpos + (size_t)f * K * 4);
    uint8_t* fl = flags + (size_t)f * K;
    uint32_t done = 0;                                      // new landmarks emitted by earlier rounds
    for (int j0 = 0; j0 < S; j0 += 1024) {
        const int j = j0 + tid;
        const bool valid = j < S;
        const float4 p = valid ? sp[j] : float4{0.0f, 0.0f, 0.0f, 0.0f};
        // one lane-mask accumulator per coordinate (v_cmp + s_or per compare); 8 LDS
        // reads in flight per unrolled step; slots past the chunk end hold NaN (never equal)
        bool hx = false, hy = false, hz = false, hw = false;
        for (int k0 = 0; k0 < nk; k0 += 1024) {
            __syncthreads();
            so[tid] = k0 + tid < nk ? op[k0 + tid] : float4{NAN, NAN, NAN, NAN};
            __syncthreads();
            const int kc = (min(1024, nk - k0) + 7) & ~7;
            for (int k = 0; k < kc; k += 8) {
                float4 o[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) o[u] = so[k + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    hx |= o[u].x == p.x;
                    hy |= o[u].y == p.y;
                    hz |= o[u].z == p.z;
                    hw |= o[u].w == p.w;
                }
            }
        }
        const bool hit = hx || hy || hz || hw;
        const uint32_t isnew = (valid && !hit) ? 1u : 0u;
        if (valid) fl[j] = (uint8_t)isnew;
        uint32_t total;
        const uint32_t pos = block_excl_scan<16>(isnew, sh, &total);
        if (isnew) lm_new[(size_t)f * K + done + pos] = j;
        done += total;
    }
    __syncthreads();
    if (tid == 0) {
        lm_M[f] = (int)done;
        lm_rows[f] = 2;                                     // zeros(size(features_l,2),3): 2 rows
        for (int m = (int)done; m < 2; ++m) fl[m] = 0;      // rows beyond M stay zero rows
    }
}

// CreateLandmarksFromFeatures: odd 1-based rows (even 0-based), triangulate, z gates.  Every
// row up to max(M, 2) is written: the kept point, or a zero row (odd rows, rows failing a z
// gate, and the two preallocated rows of CreateLandmarksFromFeatures.m:2 when M < 2) -- the
// camera-frame rows vo_get_landmark_rows returns equal oracle_landmark_rows', zero rows included.
__global__ void k_lm_tri(const float* __restrict__ spos, const int* __restrict__ lm_new, const int* __restrict__ lm_M,
                         int kp_cap, CalibDev cal, float* __restrict__ lm_X, uint8_t* __restrict__ lm_keep,
                         int* __restrict__ lm_rows)
{
    const int f = blockIdx.y, K = kp_cap;
    const int M = lm_M[f];
    const int n = M > 2 ? M : 2;
    for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < n; m += gridDim.x * blockDim.x) {
        uint8_t keep = 0;
        double X[3] = {0.0, 0.0, 0.0};
        if ((m & 1) == 0 && m < M) {
            const int j = lm_new[(size_t)f * K + m];
            const float* p = spos + ((size_t)f * K + j) * 4;
            vo_dlt_point(p[0], p[1], p[2], p[3], cal.P1, cal.P2, X);
            keep = !(X[2] < 0) && !(X[2] > 80);
            if (keep) atomicMax(lm_rows + f, m + 1);
        }
        float* o = lm_X + ((size_t)f * K + m) * 3;
        o[0] = keep ? (float)X[0] : 0.0f; o[1] = keep ? (float)X[1] : 0.0f; o[2] = keep ? (float)X[2] : 0.0f;
        lm_keep[(size_t)f * K + m] = keep;
    }
}

// ---------------------------------------------------------------------------
// host enqueue
// ---------------------------------------------------------------------------
static CalibDev calib_dev(const vo_calib& c)
{
    CalibDev d;
    memcpy(d.P1, c.P1, sizeof(d.P1));
    memcpy(d.P2, c.P2, sizeof(d.P2));
    memcpy(d.K, c.K, sizeof(d.K));
    return d;
}

static MsacArgs msac_args(GeomBuffers& g, const double* img, const double* world, const int* n, int n_stride,
                          const double K[9], const vo_ransac_params& rp, uint32_t key0)
{
    MsacArgs a;
    a.img = img; a.world = world; a.n = n; a.n_stride = n_stride;
    a.hyp = g.hyp; a.fg = g.fg; a.inliers = g.inliers;
    a.kp_cap = g.kp_cap; a.n_hyp = g.n_hyp; a.max_trials = rp.max_num_trials < g.n_hyp ? rp.max_num_trials : g.n_hyp;
    a.thr = rp.max_reprojection_error * rp.max_reprojection_error;
    a.conf = rp.confidence / 100.0;
    a.seed = rp.seed;
    a.key0 = key0;
    memcpy(a.K, K, sizeof(a.K));
    return a;
}

static void msac_enqueue(const MsacArgs& a, int B, hipStream_t s)
{
    VO_LAUNCH(k_msac, dim3(B), dim3(VO_MSAC_T), 0, s, a);
}

void track_enqueue(GeomBuffers& g, const MatchBuffers& mb, const MatchJob* d_track_jobs, const StepArgs& a,
                   const vo_match_params& mp, hipStream_t s)
{
    const int B = a.B, M = a.max_frames, K = a.kp_cap;
    for (int step = 0; step < 4; ++step) {           // the composition inside match_launch's finishing kernel (csrc/match.hip)
        MatchCompose cp{g.lists, g.list_n, a.pair_i, a.pair_j, M, K, step, 0};
        match_launch(mb, d_track_jobs + step * M, B, mp, s, &cp);
    }
}

void geom_enqueue(GeomBuffers& g, const MatchBuffers& mb, const MatchJob* d_track_jobs, const StepArgs& a,
                  const vo_match_params& mp, hipStream_t s)
{
    const int B = a.B, M = a.max_frames, K = a.kp_cap;
    track_enqueue(g, mb, d_track_jobs, a, mp, s);
    CalibDev cal = calib_dev(a.calib);
    VO_LAUNCH(k_gather_tri, dim3(16, B), dim3(64), 0, s, a.sb->kp, K, g.lists, g.list_n, g.oldpos, g.imgpt, g.world, M, cal);
    MsacArgs ma = msac_args(g, g.imgpt, g.world, g.list_n + 3, 4, a.calib.K, a.rp, (uint32_t)a.frame_index0);
    msac_enqueue(ma, B, s);
    if (a.refine_on) refine_launch(g, g.imgpt, g.world, g.inliers, g.list_n + 3, 4, a.calib.K, a.refine, B, 1, s);
    VO_LAUNCH(k_stereo_pos, dim3(16, B), dim3(256), 0, s, a.sb->kp, K, a.pair_i, a.pair_j, a.pair_n, g.spos, g.s_n);
    VO_LAUNCH(k_lm_filter, dim3(B), dim3(1024), 0, s, g.spos, g.s_n, g.oldpos, g.list_n + 3, 4, K, g.lm_keep, g.lm_new,
              g.lm_M, g.lm_rows);
    VO_LAUNCH(k_lm_tri, dim3(16, B), dim3(64), 0, s, g.spos, g.lm_new, g.lm_M, K, cal, g.lm_X, g.lm_keep, g.lm_rows);
}

// block f: its offset is the sum of the earlier frames' row counts (a loop over them: any B up to
// VO_MAX_BATCH), then a plain copy
__global__ __launch_bounds__(256) void k_lm_pack(const float* __restrict__ lm_X, const uint8_t* __restrict__ lm_keep,
                                                 const int* __restrict__ lm_rows, int kp_cap, float* __restrict__ pX,
                                                 uint8_t* __restrict__ pkeep)
{
    const int f = blockIdx.x, tid = threadIdx.x;
    __shared__ int off;
    if (tid < 64) {
        int v = 0;
        for (int g2 = tid; g2 < f; g2 += 64) v += min(lm_rows[g2], kp_cap);
        v = wave_sum(v);
        if (tid == 0) off = v;
    }
    __syncthreads();
    const int n = min(lm_rows[f], kp_cap);
    const float* X = lm_X + (size_t)f * kp_cap * 3;
    for (int e = tid; e < 3 * n; e += 256) pX[(size_t)off * 3 + e] = X[e];
    for (int e = tid; e < n; e += 256) pkeep[off + e] = lm_keep[(size_t)f * kp_cap + e];
}

void lm_pack_launch(GeomBuffers& g, int B, float* pX, uint8_t* pkeep, hipStream_t s)
{
    VO_LAUNCH(k_lm_pack, dim3(B), dim3(256), 0, s, g.lm_X, g.lm_keep, g.lm_rows, g.kp_cap, pX, pkeep);
}

// block f: frame f's rows, one thread per row.  The f64 products and sums are those of the host
// lm_world (vo_api.hip) in the same order (no contraction: -ffp-contract=off), so the single-rounded
// world rows equal a single-process run's bit for bit.
__global__ __launch_bounds__(256) void k_lm_world(const double* __restrict__ poses, const long long* __restrict__ off,
                                                  const float* __restrict__ X, const uint8_t* __restrict__ keep,
                                                  float* __restrict__ out)
{
    const int f = blockIdx.x;
    const long long a = off[f], b = off[f + 1];
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = poses[(size_t)16 * f + k];
    for (long long r = a + threadIdx.x; r < b; r += 256) {
        float w[3] = {0.0f, 0.0f, 0.0f};
        if (keep[r]) {
            const double x0 = X[3 * r], x1 = X[3 * r + 1], x2 = X[3 * r + 2];
#pragma unroll
            for (int i = 0; i < 3; ++i) w[i] = (float)(P[4 * i] * x0 + P[4 * i + 1] * x1 + P[4 * i + 2] * x2 + P[4 * i + 3]);
        }
        out[3 * r] = w[0]; out[3 * r + 1] = w[1]; out[3 * r + 2] = w[2];
    }
}

void lm_world_launch(const double* poses, const long long* off, int n_frames, const float* X, const uint8_t* keep,
                     float* out, hipStream_t s)
{
    if (n_frames <= 0) return;
    VO_LAUNCH(k_lm_world, dim3(n_frames), dim3(256), 0, s, poses, off, X, keep, out);
}

void triangulate_launch(const float* pos, int n, const vo_calib& c, double* X, hipStream_t s)
{
    if (n <= 0) return;
    int blocks = (n + 63) / 64;
    if (blocks > 1024) blocks = 1024;
    VO_LAUNCH(k_tri_list, dim3(blocks), dim3(64), 0, s, pos, n, calib_dev(c), X);
}

void tri_quality_launch(const float* pos, const double* X, const int* n, int n_stride, int n_val, int frames, int cap,
                        const vo_calib& c, float* err, uint8_t* valid, hipStream_t s)
{
    if (frames <= 0 || cap <= 0 || (!n && n_val <= 0)) return;
    int blocks = ((n || n_val > cap ? cap : n_val) + 63) / 64;
    if (blocks > 1024) blocks = 1024;
    VO_LAUNCH(k_tri_quality, dim3(blocks, frames), dim3(64), 0, s, pos, X, n, n_stride, n_val, cap, calib_dev(c), err, valid);
}

void estworldpose_launch(GeomBuffers& g, const double* img, const double* world, const int* n, const double K[9],
                         const vo_ransac_params& rp, uint32_t frame_key, hipStream_t s)
{
    MsacArgs ma = msac_args(g, img, world, n, 0, K, rp, frame_key);
    msac_enqueue(ma, 1, s);
}

void refine_launch(GeomBuffers& g, const double* img, const double* world, const uint8_t* use, const int* n, int n_stride,
                   const double K[9], const vo_refine_params& p, int frames, int need_ok, hipStream_t s)
{
    if (frames <= 0) return;
    RefineArgs a;
    a.img = img; a.world = world; a.use = use; a.n = n; a.n_stride = n_stride;
    a.fg = g.fg; a.stats = g.refine;
    a.kp_cap = g.kp_cap; a.need_ok = need_ok;
    a.p = p;
    memcpy(a.K, K, sizeof(a.K));
    VO_LAUNCH(k_refine_pose, dim3(frames), dim3(64), 0, s, a);
}

hipError_t fund_reserve(DevPool& pool, FundBuffers& fb, int B, int pts_stride)
{
    const size_t pts = (size_t)B * pts_stride;
    if (pts > fb.cap_pts) {
        const int e = pool.grow({DevPool::req(fb.x1, 2 * pts), DevPool::req(fb.x2, 2 * pts), DevPool::req(fb.inliers, pts)});
        if (e) return (hipError_t)e;
        fb.cap_pts = pts;
    }
    if (B > fb.cap_B) {
        const int e = pool.grow({DevPool::req(fb.n, (size_t)B), DevPool::req(fb.hyp, (size_t)B * VO_FUND_CHUNK),
                                 DevPool::req(fb.out, (size_t)B)});
        if (e) return (hipError_t)e;
        fb.cap_B = B;
    }
    return hipSuccess;
}

void fund_launch(FundBuffers& fb, int B, int pts_stride, const vo_fund_params& p, uint32_t key0, hipStream_t s)
{
    if (B <= 0) return;
    FundArgs a;
    a.x1 = fb.x1; a.x2 = fb.x2; a.n = fb.n; a.stride = pts_stride;
    a.hyp = fb.hyp; a.out = fb.out; a.inliers = fb.inliers;
    a.method = p.method; a.num_trials = p.num_trials;
    a.thr = p.distance_threshold;
    a.conf = p.confidence / 100.0;
    a.seed = p.seed; a.key0 = key0;
    VO_LAUNCH(k_fund_msac, dim3(B), dim3(VO_FUND_T), 0, s, a);
}

void landmarks_launch(GeomBuffers& g, const int* kn, const vo_calib& c, hipStream_t s)
{
    CalibDev cal = calib_dev(c);
    VO_LAUNCH(k_lm_filter, dim3(1), dim3(1024), 0, s, g.spos, g.s_n, g.oldpos, kn, 0, g.kp_cap, g.lm_keep, g.lm_new, g.lm_M,
              g.lm_rows);
    VO_LAUNCH(k_lm_tri, dim3(16, 1), dim3(64), 0, s, g.spos, g.lm_new, g.lm_M, g.kp_cap, cal, g.lm_X, g.lm_keep, g.lm_rows);
}

}  // namespace vo
