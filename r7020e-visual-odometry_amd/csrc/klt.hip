// klt.hip — vision.PointTracker on the device: pyramidal Lucas-Kanade in the fixed-point arithmetic
// of include/vo_spec.h (vo_klt_*; DESIGN.md 3.5.3 is the spec, 9p the kernel).
//
// k_klt_pyr builds one level of every image of a call in one launch, a byte per thread.
//
// k_klt_track is one wave per point and pair, KLT_WAVES waves per block with nothing shared between
// them (no block barrier; a wave whose point does not exist returns at once).  The level loop, the
// forward pass, the score pass and the back pass all run inside the launch.  Per level the wave
// stages the clamped (bw + 3) x (bh + 3) u8 patch of the template image through its own LDS slice,
// so the sample loop has no border logic, and keeps the template's I, Ix, Iy of its samples
// s = lane + 64 k (k < 16, fully unrolled) in 24 registers as packed int16.  Per iteration the four
// taps of a sample of the second image are read straight from L1 / L2 with clamped indices: staging
// the (bw + 1) x (bh + 1) patch through the same LDS slice was measured 17 - 20 % slower (DESIGN.md
// 9p); the score pass, which runs once, still stages.  Lane partials are int32 (bounds: vo_spec.h),
// the window sums int64 through wave_sum, so every lane holds the same sums and takes the
// same f32 step: control flow is wave-uniform.
#include "vo_internal.h"
#include "wave.h"

namespace vo {

#define KLT_WAVES 4
#define KLT_SLICE 1168                // >= (31 + 3)^2 = 1156 bytes, a multiple of 16

struct KltArgs {
    const uint8_t* planes;            // level-major: level l of image i at lvl_off(l) + i * rows_l * cols_l
    const float* pts0; const float* guess; const int* n;
    float* pts1; uint8_t* valid; float* scores; vo_klt_info* info;
    int rows, cols, n_pairs, stride;  // image i = which * n_pairs + pair
    int levels, bw, bh, max_it, bidir;
    float max_bidir;
};

__global__ __launch_bounds__(256) void k_klt_pyr(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows, int cols,
                                                 int n_img)
{
    const int r1 = (rows + 1) / 2, c1 = (cols + 1) / 2;
    const int t = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
    if (t >= r1 * c1 || img >= n_img) return;
    const int r = t / c1, c = t - r * c1;
    dst[(size_t)img * r1 * c1 + t] = (uint8_t)vo_klt_pyr_pixel(src + (size_t)img * rows * cols, rows, cols, cols, r, c);
}

// the wave's own LDS traffic only: LDS operations of one wave complete in order, so all that is
// needed between the staging stores and the sample loads (and back) is that the compiler keeps them
// in program order
static __device__ __forceinline__ void klt_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// P[y * pw + x] = level pixel (oy + y, ox + x), indices clamped to the level
static __device__ __forceinline__ void klt_stage(uint8_t* P, const uint8_t* __restrict__ img, int rows, int cols, int ox, int oy,
                                                 int pw, int ph, int lane)
{
    klt_wave_sync();
    const int qd = 64 / pw, rm = 64 - qd * pw, total = pw * ph;
    int y = lane / pw, x = lane - y * pw;
    for (int e = lane; e < total; e += 64) {
        const int r = min(max(oy + y, 0), rows - 1), c = min(max(ox + x, 0), cols - 1);
        P[e] = img[(size_t)r * cols + c];
        x += rm; y += qd;
        if (x >= pw) { x -= pw; ++y; }
    }
    klt_wave_sync();
}

__global__ __launch_bounds__(KLT_WAVES * 64) void k_klt_track(KltArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[KLT_WAVES][KLT_SLICE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.y, k = blockIdx.x * KLT_WAVES + wave;
    if (k >= a.n[f]) return;
    uint8_t* P = lds[wave];
    const int bw = a.bw, bh = a.bh, nwin = bw * bh, L = a.levels;
    const int qd = 64 / bw, rm = 64 - qd * bw;              // sample s + 64 from sample s
    const int y_first = lane / bw, x_first = lane - y_first * bw;
    const float hx = (float)(bw - 1) * 0.5f, hy = (float)(bh - 1) * 0.5f;
    const size_t pt = (size_t)f * a.stride + k;
    const float in_x = a.pts0[2 * pt], in_y = a.pts0[2 * pt + 1];
    const float x0 = in_x - 1.0f, y0 = in_y - 1.0f;
    const int n_img = 2 * a.n_pairs;

    uint32_t tA[VO_KLT_LANE_SAMPLES];                        // I | Ix << 16
    uint32_t tB[VO_KLT_LANE_SAMPLES / 2];                    // Iy of samples 2 m | 2 m + 1 << 16

    int status = VO_KLT_OK, f_stop = VO_KLT_STOP_NONE, f_it = 0, f_skip = 0;
    float f_x = x0, f_y = y0, score = 0.0f, err = vo_u32_as_f32(0x7fc00000u);

    for (int pass = 0; pass < 2; ++pass) {
        const int imgA = pass ? a.n_pairs + f : f, imgB = pass ? f : a.n_pairs + f;
        const float sx = pass ? f_x : x0, sy = pass ? f_y : y0;
        const bool has_guess = pass == 0 && a.guess != nullptr;
        const float gx0 = has_guess ? a.guess[2 * pt] - 1.0f : sx, gy0 = has_guess ? a.guess[2 * pt + 1] - 1.0f : sy;
        int p_status = VO_KLT_OK, p_stop = VO_KLT_STOP_NONE, p_it = 0, p_skip = 0;
        float nx = 0.0f, ny = 0.0f;
        for (int l = L - 1; l >= 0; --l) {
            int rows = a.rows, cols = a.cols;
            size_t off = 0;
            for (int q = 0; q < l; ++q) { off += (size_t)n_img * rows * cols; rows = (rows + 1) / 2; cols = (cols + 1) / 2; }
            const uint8_t* A = a.planes + off + (size_t)imgA * rows * cols;
            const uint8_t* B = a.planes + off + (size_t)imgB * rows * cols;
            const float sc = 1.0f / (float)(1 << l);
            if (l == L - 1) { nx = gx0 * sc; ny = gy0 * sc; }
            else { nx = 2.0f * nx; ny = 2.0f * ny; }
            int why = VO_KLT_OK, w[4], ix, iy;
            float Am[4];
            if (!vo_klt_corner(sx * sc - hx, sy * sc - hy, bw, bh, rows, cols, &ix, &iy, w)) why = VO_KLT_TEMPLATE_OUT;
            else {
                const int pw = bw + 3;
                klt_stage(P, A, rows, cols, ix - 1, iy - 1, pw, bh + 3, lane);
                int sxx = 0, sxy = 0, syy = 0;
                int x = x_first, y = y_first;
#pragma unroll
                for (int kk = 0; kk < VO_KLT_LANE_SAMPLES; ++kk) {
                    int I = 0, Ix = 0, Iy = 0;
                    if (lane + 64 * kk < nwin) {
                        const uint8_t* b = P + y * pw + x;
                        int v[4][4];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 4; ++j) v[i][j] = b[i * pw + j];
                        int g[2][2], h[2][2];
#pragma unroll
                        for (int i = 1; i <= 2; ++i)
#pragma unroll
                            for (int j = 1; j <= 2; ++j) {
                                g[i - 1][j - 1] = vo_klt_scharr(v[i - 1][j - 1], v[i - 1][j + 1], v[i][j - 1], v[i][j + 1], v[i + 1][j - 1],
                                                                v[i + 1][j + 1]);
                                h[i - 1][j - 1] = vo_klt_scharr(v[i - 1][j - 1], v[i + 1][j - 1], v[i - 1][j], v[i + 1][j], v[i - 1][j + 1],
                                                                v[i + 1][j + 1]);
                            }
                        I = vo_klt_bil(v[1][1], v[1][2], v[2][1], v[2][2], w, 9);
                        Ix = vo_klt_bil(g[0][0], g[0][1], g[1][0], g[1][1], w, 14);
                        Iy = vo_klt_bil(h[0][0], h[0][1], h[1][0], h[1][1], w, 14);
                        sxx += Ix * Ix; sxy += Ix * Iy; syy += Iy * Iy;
                    }
                    tA[kk] = ((uint32_t)I & 0xffffu) | ((uint32_t)Ix << 16);
                    if (kk & 1) tB[kk >> 1] |= (uint32_t)Iy << 16;
                    else tB[kk >> 1] = (uint32_t)Iy & 0xffffu;
                    x += rm; y += qd;
                    if (x >= bw) { x -= bw; ++y; }
                }
                const int64_t txx = wave_sum(sxx), txy = wave_sum(sxy), tyy = wave_sum(syy);
                if (!vo_klt_gradient_matrix(txx, txy, tyy, bw, bh, Am)) why = VO_KLT_FLAT;
            }
            int stop = VO_KLT_STOP_NONE, j = 0;
            if (why == VO_KLT_OK) {
                float qx = nx - hx, qy = ny - hy, mx = nx, my = ny, pdx = 0.0f, pdy = 0.0f;
                for (j = 0; j < a.max_it; ++j) {
                    if (!vo_klt_corner(qx, qy, bw, bh, rows, cols, &ix, &iy, w)) { why = VO_KLT_LOST; break; }
                    int s1 = 0, s2 = 0;
                    int x = x_first, y = y_first;
#pragma unroll
                    for (int kk = 0; kk < VO_KLT_LANE_SAMPLES; ++kk) {
                        if (lane + 64 * kk < nwin) {
                            const int r0 = min(max(iy + y, 0), rows - 1), r1 = min(max(iy + y + 1, 0), rows - 1);
                            const int c0 = min(max(ix + x, 0), cols - 1), c1 = min(max(ix + x + 1, 0), cols - 1);
                            const uint8_t* b0 = B + (size_t)r0 * cols;
                            const uint8_t* b1 = B + (size_t)r1 * cols;
                            const int I = (int)(tA[kk] & 0xffffu), Ix = (int)tA[kk] >> 16;
                            const int Iy = (kk & 1) ? (int)tB[kk >> 1] >> 16 : (int)(int16_t)(tB[kk >> 1] & 0xffffu);
                            const int diff = vo_klt_bil(b0[c0], b0[c1], b1[c0], b1[c1], w, 9) - I;
                            s1 += diff * Ix; s2 += diff * Iy;
                        }
                        x += rm; y += qd;
                        if (x >= bw) { x -= bw; ++y; }
                    }
                    float dx, dy;
                    vo_klt_delta(Am, wave_sum(s1), wave_sum(s2), &dx, &dy);
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
            if (l == 0) { p_stop = why == VO_KLT_OK ? stop : VO_KLT_STOP_NONE; p_it = j; }
            if (why != VO_KLT_OK) {
                if (l == 0) p_status = why;
                else ++p_skip;
            }
        }
        if (p_status == VO_KLT_OK && !vo_klt_inside(nx, ny, a.rows, a.cols)) p_status = VO_KLT_LOST;
        if (pass == 0) {
            status = p_status; f_stop = p_stop; f_it = p_it; f_skip = p_skip;
            if (status != VO_KLT_OK) break;
            f_x = nx; f_y = ny;
            // the score pass: the level-0 template is still in tA; the corner of a point inside the image is never out
            int w[4], ix, iy;
            if (vo_klt_corner(nx - hx, ny - hy, bw, bh, a.rows, a.cols, &ix, &iy, w)) {
                const int pw = bw + 1;
                klt_stage(P, a.planes + (size_t)imgB * a.rows * a.cols, a.rows, a.cols, ix, iy, pw, bh + 1, lane);
                int64_t s2 = 0;
                int x = x_first, y = y_first;
#pragma unroll
                for (int kk = 0; kk < VO_KLT_LANE_SAMPLES; ++kk) {
                    if (lane + 64 * kk < nwin) {
                        const uint8_t* b = P + y * pw + x;
                        const int diff = vo_klt_bil(b[0], b[1], b[pw], b[pw + 1], w, 9) - (int)(tA[kk] & 0xffffu);
                        s2 += diff * diff;
                    }
                    x += rm; y += qd;
                    if (x >= bw) { x -= bw; ++y; }
                }
                score = vo_klt_score(wave_sum(s2), bw, bh);
            }
            if (!a.bidir) break;
        } else {
            if (p_status != VO_KLT_OK) status = VO_KLT_BIDIR;
            else {
                err = vo_klt_bidir_error(nx, ny, x0, y0);
                if (!(err <= a.max_bidir)) status = VO_KLT_BIDIR;
            }
        }
    }
    if (lane == 0) {
        const bool ok = status == VO_KLT_OK;
        a.pts1[2 * pt] = ok ? f_x + 1.0f : in_x;
        a.pts1[2 * pt + 1] = ok ? f_y + 1.0f : in_y;
        a.valid[pt] = ok ? 1 : 0;
        a.scores[pt] = ok ? score : 0.0f;
        vo_klt_info o;
        o.status = (uint8_t)status; o.stop = (uint8_t)f_stop; o.iterations = (uint8_t)f_it; o.levels_skipped = (uint8_t)f_skip;
        o.bidir_error = err;
        a.info[pt] = o;
    }
}

// bytes of the six levels of one rows x cols image
static size_t klt_image_bytes(int rows, int cols)
{
    size_t t = 0;
    for (int l = 0; l < VO_KLT_MAX_LEVELS; ++l) t += (size_t)vo_klt_level_dim(rows, l) * vo_klt_level_dim(cols, l);
    return t;
}

size_t klt_level_offset(int rows, int cols, int n_pairs, int level)
{
    size_t t = 0;
    for (int l = 0; l < level; ++l) t += (size_t)2 * n_pairs * vo_klt_level_dim(rows, l) * vo_klt_level_dim(cols, l);
    return t;
}

hipError_t klt_reserve(DevPool& pool, KltBuffers& kb, int rows, int cols, int n_pairs, int pts_stride)
{
    if (n_pairs > kb.cap_pairs) {
        const int e = pool.grow({DevPool::req(kb.planes, 2 * (size_t)n_pairs * klt_image_bytes(rows, cols)),
                                 DevPool::req(kb.n, (size_t)n_pairs)});
        if (e) return (hipError_t)e;
        kb.cap_pairs = n_pairs;
    }
    const size_t pts = std::max<size_t>((size_t)n_pairs * pts_stride, 1);
    if (pts > kb.cap_pts) {
        const int e = pool.grow({DevPool::req(kb.pts0, 2 * pts), DevPool::req(kb.guess, 2 * pts), DevPool::req(kb.pts1, 2 * pts),
                                 DevPool::req(kb.valid, pts), DevPool::req(kb.scores, pts), DevPool::req(kb.info, pts)});
        if (e) return (hipError_t)e;
        kb.cap_pts = pts;
    }
    return hipSuccess;
}

void klt_pyr_launch(KltBuffers& kb, int rows, int cols, int n_pairs, int levels, hipStream_t s)
{
    for (int l = 0; l + 1 < levels; ++l) {
        const int r0 = vo_klt_level_dim(rows, l), c0 = vo_klt_level_dim(cols, l);
        const int r1 = (r0 + 1) / 2, c1 = (c0 + 1) / 2;
        VO_LAUNCH(k_klt_pyr, dim3((r1 * c1 + 255) / 256, 2 * n_pairs), dim3(256), 0, s,
                  (const uint8_t*)kb.planes + klt_level_offset(rows, cols, n_pairs, l),
                  kb.planes + klt_level_offset(rows, cols, n_pairs, l + 1), r0, c0, 2 * n_pairs);
    }
}

void klt_track_launch(KltBuffers& kb, int rows, int cols, int n_pairs, int pts_stride, int max_n, bool has_guess,
                      const vo_klt_params& p, hipStream_t s)
{
    if (n_pairs <= 0 || max_n <= 0) return;
    KltArgs a;
    a.planes = kb.planes; a.pts0 = kb.pts0; a.guess = has_guess ? kb.guess : nullptr; a.n = kb.n;
    a.pts1 = kb.pts1; a.valid = kb.valid; a.scores = kb.scores; a.info = kb.info;
    a.rows = rows; a.cols = cols; a.n_pairs = n_pairs; a.stride = pts_stride;
    a.levels = p.num_pyramid_levels; a.bh = p.block_size[0]; a.bw = p.block_size[1]; a.max_it = p.max_iterations;
    a.max_bidir = p.max_bidirectional_error;
    a.bidir = p.max_bidirectional_error < vo_u32_as_f32(0x7f800000u) ? 1 : 0;
    VO_LAUNCH(k_klt_track, dim3((max_n + KLT_WAVES - 1) / KLT_WAVES, n_pairs), dim3(KLT_WAVES * 64), 0, s, a);
}

}  // namespace vo
