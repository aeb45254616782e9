// corner.hip — detectMinEigenFeatures / detectHarrisFeatures on the device: the integer gradient matrix
// and f64 response of include/vo_spec.h (vo_corner_*; DESIGN.md 3.5.4 is the spec, 9q the kernels).
//
// k_corner_metric: one workgroup per CORNER_TW x CORNER_TH tile of one image, all images of a call in
// one launch.  The u8 tile with a halo of (f - 1) / 2 + 1 is staged through LDS with clamped indices;
// the horizontal pass forms the three products of a tap from four LDS bytes (at the clamped index, so
// a product outside the image is the product at the border) and leaves its int32 sums in LDS; the
// vertical pass is int64, the response f64, the metric f32.  The ROI's maximum is joined as the bits of
// a non-negative float: a wave reduction, an LDS word per wave, one atomic per workgroup.
//
// k_corner_count / k_corner_emit: a workgroup owns CORNER_CHUNK consecutive pixels of the ROI's raster.
// The first counts its corners; the second adds up the counts of the chunks before its own, tests again
// (one metric read for almost every pixel) and writes its corners at their raster rank, so the list is
// in (row, column) order whatever order the workgroups run in.  The last chunk writes the true total.
//
// k_corner_rank (strongest > 0): selectStrongest's scheme -- 256 corners per workgroup against all of
// the image's, keys staged through LDS in tiles of 256 -- a corner's rank is the number of larger keys,
// and ranks below N are written to the ranked list.
#include "vo_internal.h"
#include "wave.h"

namespace vo {

#define CORNER_TW 64
#define CORNER_TH 16
#define CORNER_RMAX ((VO_CORNER_MAX_FILTER - 1) / 2)     // 7
#define CORNER_HMAX (CORNER_RMAX + 1)                    // 8: the products' halo plus the gradients' pixel
#define CORNER_PW (CORNER_TW + 2 * CORNER_HMAX)          // 80
#define CORNER_PH (CORNER_TH + 2 * CORNER_HMAX)          // 32
#define CORNER_HROWS (CORNER_TH + 2 * CORNER_RMAX)       // 30
#define CORNER_CHUNK 1024                                // ROI pixels per workgroup of count / emit
#define CORNER_RANK_BLOCKS 16

struct CornerArgs {
    const uint8_t* img; float* metric; uint32_t* mmax;
    int rows, cols, f, method;
    int x0, y0, w, h;                                    // the ROI, 0-based
    int q[VO_CORNER_MAX_FILTER];
};

__global__ __launch_bounds__(256) void k_corner_metric(CornerArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t P[CORNER_PH][CORNER_PW];
    __shared__ int H[3][CORNER_HROWS][CORNER_TW];
    __shared__ int sq[VO_CORNER_MAX_FILTER + 1];
    __shared__ uint32_t wmax[4];
    const int tid = threadIdx.x;
    const int rows = a.rows, cols = a.cols, f = a.f, R = (f - 1) / 2, hl = R + 1;
    const int tx0 = blockIdx.x * CORNER_TW, ty0 = blockIdx.y * CORNER_TH;
    const size_t plane = (size_t)blockIdx.z * rows * cols;
    const uint8_t* __restrict__ img = a.img + plane;
    const int ox = tx0 - hl, oy = ty0 - hl;              // image coordinates of P[0][0]
    if (tid < VO_CORNER_MAX_FILTER) sq[tid] = a.q[tid];
    {
        const int pw = CORNER_TW + 2 * hl, ph = CORNER_TH + 2 * hl;
        for (int e = tid; e < pw * ph; e += 256) {
            const int y = e / pw, x = e - y * pw;
            P[y][x] = img[(size_t)vo_corner_clamp(oy + y, rows) * cols + vo_corner_clamp(ox + x, cols)];
        }
    }
    __syncthreads();
    // horizontal pass: row y of H is image row clamp(ty0 - R + y), column x image column tx0 + x
    for (int e = tid; e < (CORNER_TH + 2 * R) * CORNER_TW; e += 256) {
        const int y = e >> 6, x = e & (CORNER_TW - 1);
        const int r = vo_corner_clamp(ty0 - R + y, rows);
        const int ly = r - oy, lyu = vo_corner_clamp(r - 1, rows) - oy, lyd = vo_corner_clamp(r + 1, rows) - oy;
        int hxx = 0, hyy = 0, hxy = 0;
        for (int j = 0; j < f; ++j) {
            const int c = vo_corner_clamp(tx0 + x + j - R, cols);
            const int lx = c - ox, lxl = vo_corner_clamp(c - 1, cols) - ox, lxr = vo_corner_clamp(c + 1, cols) - ox;
            const int ix = (int)P[ly][lxr] - (int)P[ly][lxl];
            const int iy = (int)P[lyd][lx] - (int)P[lyu][lx];
            const int w = sq[j];
            hxx += w * (ix * ix); hyy += w * (iy * iy); hxy += w * (ix * iy);
        }
        H[0][y][x] = hxx; H[1][y][x] = hyy; H[2][y][x] = hxy;
    }
    __syncthreads();
    // vertical pass, response, the ROI's maximum
    uint32_t best = 0;
    const int x = tid & (CORNER_TW - 1), c = tx0 + x;
    for (int y = tid >> 6; y < CORNER_TH; y += 4) {
        const int r = ty0 + y;
        if (r >= rows || c >= cols) continue;
        int64_t A = 0, B = 0, C = 0;
        for (int i = 0; i < f; ++i) {
            // H row y + i is image row ty0 + y + i - R before clamping; a clamped row holds the border row's sums
            const int64_t w = sq[i];
            A += w * H[0][y + i][x]; B += w * H[1][y + i][x]; C += w * H[2][y + i][x];
        }
        const float m = vo_corner_response(a.method, A, B, C);
        a.metric[plane + (size_t)r * cols + c] = m;
        if (r >= a.y0 && r < a.y0 + a.h && c >= a.x0 && c < a.x0 + a.w) best = max(best, vo_corner_max_bits(m));
    }
    best = wave_max(best);
    if ((tid & 63) == 0) wmax[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        const uint32_t b = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
        if (b) atomicMax(a.mmax + blockIdx.z, b);
    }
}

struct CornerSelArgs {
    const float* metric; const uint32_t* mmax;
    int* cnt;                                            // [n_img][n_chunks]
    int* total;                                          // [n_img]
    float* loc; float* met;                              // [n_img][cap][2], [n_img][cap]
    int rows, cols, x0, y0, w, h, n_chunks, cap;
    float min_quality;
};

// pixel i of the ROI's raster -> corner or not
static __device__ __forceinline__ bool corner_test(const CornerSelArgs& a, const float* __restrict__ m, int i, float thr, int& r, int& c)
{
    if (i >= a.w * a.h) return false;
    const int y = i / a.w;
    r = a.y0 + y; c = a.x0 + (i - y * a.w);
    return vo_corner_is_corner(m, a.rows, a.cols, r, c, thr) != 0;
}

__global__ __launch_bounds__(256) void k_corner_count(CornerSelArgs a)
{
    __shared__ int wc[4];
    const int tid = threadIdx.x, img = blockIdx.y;
    const float* __restrict__ m = a.metric + (size_t)img * a.rows * a.cols;
    const float mmax = __uint_as_float(a.mmax[img]);
    const float thr = a.min_quality * mmax;
    int n = 0;
    if (mmax > 0.0f)
        for (int k = 0; k < CORNER_CHUNK / 256; ++k) {
            int r, c;
            n += corner_test(a, m, blockIdx.x * CORNER_CHUNK + k * 256 + tid, thr, r, c) ? 1 : 0;
        }
    n = block_sum<4>(n, wc);
    if (tid == 0) a.cnt[(size_t)img * a.n_chunks + blockIdx.x] = n;
}

__global__ __launch_bounds__(256) void k_corner_emit(CornerSelArgs a)
{
    __shared__ int wc[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, img = blockIdx.y;
    const float* __restrict__ m = a.metric + (size_t)img * a.rows * a.cols;
    const int* __restrict__ cnt = a.cnt + (size_t)img * a.n_chunks;
    const float mmax = __uint_as_float(a.mmax[img]);
    const float thr = a.min_quality * mmax;
    // corners in the chunks before this one
    int before = 0;
    for (int b = tid; b < (int)blockIdx.x; b += 256) before += cnt[b];
    int base = block_sum<4>(before, wc);
    if ((int)blockIdx.x == a.n_chunks - 1 && tid == 0) a.total[img] = base + cnt[blockIdx.x];
    if (!(mmax > 0.0f) || cnt[blockIdx.x] == 0) return;       // block-uniform
    for (int k = 0; k < CORNER_CHUNK / 256; ++k) {
        int r = 0, c = 0;
        const bool is = corner_test(a, m, blockIdx.x * CORNER_CHUNK + k * 256 + tid, thr, r, c);
        int n_wave;
        int pos = base + wave_rank(is, &n_wave);
        __syncthreads();                                      // the previous round's readers are done
        if (lane == 0) wc[wave] = n_wave;
        __syncthreads();
        for (int v = 0; v < wave; ++v) pos += wc[v];
        if (is && pos < a.cap) {
            float x, y;
            vo_corner_location(m, a.rows, a.cols, r, c, &x, &y);
            const size_t o = (size_t)img * a.cap + pos;
            a.loc[2 * o] = x; a.loc[2 * o + 1] = y;
            a.met[o] = m[(size_t)r * a.cols + c];
        }
        base += wc[0] + wc[1] + wc[2] + wc[3];
    }
}

__global__ __launch_bounds__(256) void k_corner_rank(const int* __restrict__ total, const float* __restrict__ loc,
                                                     const float* __restrict__ met, float* __restrict__ sloc,
                                                     float* __restrict__ smet, int cap, int limit)
{
    __shared__ unsigned long long sk[256];
    const int img = blockIdx.y, tid = threadIdx.x;
    const size_t base = (size_t)img * cap;
    const int n = total[img];
    if (n > cap) return;                                      // overflow: the host reports it, nothing is ranked
    for (int r0 = blockIdx.x * 256; r0 < n; r0 += gridDim.x * 256) {       // block-uniform
        const int i = r0 + tid;
        const unsigned long long mine = i < n ? vo_corner_key(met[base + i], (uint32_t)i) : ~0ull;
        int rank = 0;
        for (int c0 = 0; c0 < n; c0 += 256) {
            const int j = c0 + tid;
            __syncthreads();                                  // the previous tile's readers are done
            sk[tid] = j < n ? vo_corner_key(met[base + j], (uint32_t)j) : 0ull;    // padding: below every key
            __syncthreads();
#pragma unroll 16
            for (int q = 0; q < 256; ++q) rank += sk[q] > mine ? 1 : 0;
        }
        if (i < n && rank < limit) {
            const size_t o = base + rank;
            sloc[2 * o] = loc[2 * (base + i)]; sloc[2 * o + 1] = loc[2 * (base + i) + 1];
            smet[o] = met[base + i];
        }
    }
}

static int corner_chunks(int w, int h) { return (w * h + CORNER_CHUNK - 1) / CORNER_CHUNK; }

hipError_t corner_reserve(DevPool& pool, CornerBuffers& cb, int rows, int cols, int n_img, int list_cap)
{
    if (n_img <= cb.cap_img) return hipSuccess;
    const size_t px = (size_t)rows * cols, lists = (size_t)n_img * list_cap;
    const int e = pool.grow({DevPool::req(cb.img, n_img * px), DevPool::req(cb.metric, n_img * px), DevPool::req(cb.mmax, (size_t)n_img),
                             DevPool::req(cb.cnt, (size_t)n_img * corner_chunks(cols, rows)), DevPool::req(cb.total, (size_t)n_img),
                             DevPool::req(cb.loc, 2 * lists), DevPool::req(cb.met, lists), DevPool::req(cb.sloc, 2 * lists),
                             DevPool::req(cb.smet, lists)});
    if (e) return (hipError_t)e;
    cb.cap_img = n_img; cb.list_cap = list_cap;
    return hipSuccess;
}

hipError_t corner_launch(CornerBuffers& cb, int rows, int cols, int n_img, const vo_corner_params& p, const int* roi0, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(cb.mmax, 0, sizeof(uint32_t) * n_img, s);
    if (e != hipSuccess) return e;
    CornerArgs a;
    a.img = cb.img; a.metric = cb.metric; a.mmax = cb.mmax;
    a.rows = rows; a.cols = cols; a.f = p.filter_size; a.method = p.method;
    a.x0 = roi0[0]; a.y0 = roi0[1]; a.w = roi0[2]; a.h = roi0[3];
    for (int k = 0; k < VO_CORNER_MAX_FILTER; ++k) a.q[k] = 0;
    vo_corner_weights(p.filter_size, a.q);
    VO_LAUNCH(k_corner_metric, dim3((cols + CORNER_TW - 1) / CORNER_TW, (rows + CORNER_TH - 1) / CORNER_TH, n_img), dim3(256), 0, s, a);
    CornerSelArgs b;
    b.metric = cb.metric; b.mmax = cb.mmax; b.cnt = cb.cnt; b.total = cb.total; b.loc = cb.loc; b.met = cb.met;
    b.rows = rows; b.cols = cols; b.x0 = a.x0; b.y0 = a.y0; b.w = a.w; b.h = a.h;
    b.n_chunks = corner_chunks(a.w, a.h); b.cap = cb.list_cap; b.min_quality = p.min_quality;
    VO_LAUNCH(k_corner_count, dim3(b.n_chunks, n_img), dim3(256), 0, s, b);
    VO_LAUNCH(k_corner_emit, dim3(b.n_chunks, n_img), dim3(256), 0, s, b);
    if (p.strongest > 0)
        VO_LAUNCH(k_corner_rank, dim3(CORNER_RANK_BLOCKS, n_img), dim3(256), 0, s, (const int*)cb.total, (const float*)cb.loc,
                  (const float*)cb.met, cb.sloc, cb.smet, cb.list_cap, p.strongest);
    return hipSuccess;
}

}  // namespace vo
