// undistort.hip — undistortImage (VO.m:75-76) on the device: the Brown-Conrady remap of
// include/vo_spec.h (vo_undistort_pos, vo_undistort_inside, vo_undistort_u8), bit for bit
// kitti.undistort.
//
// The sampling map depends only on the camera, so a thread evaluates it once (f64, two IEEE
// divisions per pixel) for its 4 adjacent output pixels of one row and then walks the
// VO_UD_CHUNK frames of its chunk: per frame and pixel two 16-bit loads (the two taps of a row are
// adjacent bytes), the bilinear sum in f64 and one packed store.  Over a batch the kernel reads
// and writes each image byte about once and needs no per-pixel table in memory.
#include "vo_internal.h"

namespace vo {

struct UndistortArgs {
    UndistortSide side[2];
    size_t in_stride, out_stride;
    int rows, cols, B, n_chunk;
};

// 4 output bytes (n < 4 at a row's tail) to p: one dword where p is 4-B aligned, two shorts where
// it is 2-B aligned (tightly packed frames of odd pitch put every other row there), bytes
// otherwise.  The alignment is the same for every full lane of a wave (one row, one frame).
static __device__ __forceinline__ void ud_store(uint8_t* p, int n, uint32_t w)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (n == 4 && (a & 3) == 0) {
        *reinterpret_cast<uint32_t*>(p) = w;
    } else if (n == 4 && (a & 1) == 0) {
        reinterpret_cast<uint16_t*>(p)[0] = (uint16_t)(w & 0xffffu);
        reinterpret_cast<uint16_t*>(p)[1] = (uint16_t)(w >> 16);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n) p[i] = (uint8_t)((w >> (8 * i)) & 0xffu);
    }
}

// grid: x = groups of 256 columns (64 lanes x 4 pixels), y = row, z = side * n_chunk + chunk
__global__ __launch_bounds__(64) void k_undistort(UndistortArgs a)
{
    const int side = blockIdx.z / a.n_chunk, chunk = blockIdx.z - side * a.n_chunk;
    const UndistortSide S = side ? a.side[1] : a.side[0];     // (a select of scalars, not an indexed copy)
    const int v = blockIdx.y, u0 = 4 * (blockIdx.x * 64 + threadIdx.x);
    if (u0 >= a.cols) return;
    const int n = min(4, a.cols - u0);
    const int f0 = chunk * VO_UD_CHUNK, f1 = min(a.B, f0 + VO_UD_CHUNK);
    const int ld = a.cols;
    const size_t o_out = (size_t)v * ld + u0;
    if (S.copy) {
        for (int f = f0; f < f1; ++f) {
            const uint8_t* ip = S.in + (size_t)f * a.in_stride + o_out;
            uint32_t w = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) w |= (uint32_t)ip[i < n ? i : 0] << (8 * i);
            ud_store(S.out + (size_t)f * a.out_stride + o_out, n, w);
        }
        return;
    }
    // the map of the thread's pixels.  The two taps of a row are adjacent bytes, fetched as one
    // 16-bit load at column xl <= cols - 2 (any alignment), so both bytes are inside the row:
    // xl = x0, taps = low / high byte; at x0 = -1 xl = 0 and tap 01 is the low byte; at
    // x0 = cols - 1 xl = cols - 2 and tap 00 is the high byte.  o00 = offset of row y0's pair
    // (y0 clamped to 0); fl bits 0-3 = taps 00, 01, 10, 11 inside the image, bit 4 / 5 = tap
    // 00 / 01 is the pair's high byte, bit 6 = the lower row is one row on.  A pixel past the
    // row's end, or one whose position has no tap inside the image, keeps fl = 0 and zero
    // fractions: its four taps read as 0.0 and it stores 0.
    typedef uint16_t __attribute__((aligned(1))) u16_any;
    uint32_t o00[4], fl[4];
    double ax[4], ay[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o00[i] = 0; fl[i] = 0; ax[i] = 0.0; ay[i] = 0.0;
        if (i >= n) continue;
        double us, vs;
        vo_undistort_pos(&S.cam, u0 + i, v, &us, &vs);
        if (!vo_undistort_inside(us, vs, a.rows, a.cols)) continue;
        const double xf = floor(us), yf = floor(vs);
        ax[i] = us - xf;
        ay[i] = vs - yf;
        const int x0 = (int)xf, y0 = (int)yf;                       // [-1, cols - 1], [-1, rows - 1]
        const uint32_t okx0 = x0 >= 0, okx1 = x0 + 1 < a.cols, oky0 = y0 >= 0, oky1 = y0 + 1 < a.rows;
        const int xl = okx1 ? (okx0 ? x0 : 0) : a.cols - 2, yc = oky0 ? y0 : 0;
        o00[i] = (uint32_t)(yc * ld + xl);
        fl[i] = (okx0 & oky0) | ((okx1 & oky0) << 1) | ((okx0 & oky1) << 2) | ((okx1 & oky1) << 3) |
                ((okx1 ^ 1u) << 4) | ((okx0 & okx1) << 5) | ((oky0 & oky1) << 6);
    }
    // (not unrolled: 2 and 4 frames per iteration measured the same)
    for (int f = f0; f < f1; ++f) {
        const uint8_t* ip = S.in + (size_t)f * a.in_stride;
        uint32_t t[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // both pairs are inside the frame: row yc, and one row on only where that row exists
            const uint32_t dy = ((fl[i] >> 6) & 1u) * (uint32_t)ld;
            const uint32_t w0 = *reinterpret_cast<const u16_any*>(ip + o00[i]);
            const uint32_t w1 = *reinterpret_cast<const u16_any*>(ip + o00[i] + dy);
            const uint32_t s0 = (fl[i] >> 1) & 8u, s1 = (fl[i] >> 2) & 8u;      // bit 4 / bit 5 -> shift 0 or 8
            t[i][0] = (w0 >> s0) & 0xffu; t[i][1] = (w0 >> s1) & 0xffu;
            t[i][2] = (w1 >> s0) & 0xffu; t[i][3] = (w1 >> s1) & 0xffu;
        }
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // a tap outside the image is 0.0 (masked as an integer, then the exact u8 -> f64 conversion)
            const double t00 = (double)((fl[i] & 1u) ? t[i][0] : 0u), t01 = (double)((fl[i] & 2u) ? t[i][1] : 0u);
            const double t10 = (double)((fl[i] & 4u) ? t[i][2] : 0u), t11 = (double)((fl[i] & 8u) ? t[i][3] : 0u);
            w |= (uint32_t)vo_undistort_u8(t00, t01, t10, t11, ax[i], ay[i]) << (8 * i);
        }
        ud_store(S.out + (size_t)f * a.out_stride + o_out, n, w);
    }
}

void undistort_launch(const UndistortSide* sides, int n_sides, int rows, int cols, int B, size_t in_stride,
                      size_t out_stride, hipStream_t s)
{
    UndistortArgs a;
    a.side[0] = sides[0];
    a.side[1] = sides[n_sides > 1 ? 1 : 0];
    a.in_stride = in_stride; a.out_stride = out_stride;
    a.rows = rows; a.cols = cols; a.B = B;
    a.n_chunk = (B + VO_UD_CHUNK - 1) / VO_UD_CHUNK;
    const dim3 grid((cols + 255) / 256, rows, n_sides * a.n_chunk);
    VO_LAUNCH(k_undistort, grid, dim3(64), 0, s, a);
}

}  // namespace vo
