// sgm.hip — disparitySGM / reconstructScene on the device: semi-global matching on a census cost in the
// integer arithmetic of include/vo_spec.h (vo_sgm_*, vo_reconstruct_*; DESIGN.md 3.5.5 is the spec, 9t the
// kernels).
//
// k_sgm_census: one workgroup per SGM_TW x SGM_TH tile of one image (left and right images of every pair
// of a group in one launch).  The u8 tile with its 3-row / 4-column halo is staged through LDS with clamped
// indices; each thread forms the 62-bit words of four pixels from LDS bytes.
//
// k_sgm_paths<H, NPL>: one wave per path of path set H (0: rows, 1: columns, 2: diagonals, 3:
// anti-diagonals), four paths per workgroup.  A lane owns NPL adjacent disparities (1 for D <= 64, 2
// above); lanes beyond D hold VO_SGM_ABSENT, which no minimum picks.  L_r of the previous pixel lives in
// registers; a step takes the census words loaded one step ahead, the minimum by wave_min, the k +- 1
// neighbours by wave_shift_up / wave_shift_down, and moves the lane's 2 * NPL bytes of S.  The wave walks
// its path forwards (direction 2 H) and then backwards (2 H + 1) over the same pixels, so the four
// launches of a group need no atomics: within a launch a pixel's sums belong to one wave, and a lane
// meets only its own addresses again.  The first launch's forward walk stores S, everything after adds.
//
// k_sgm_select: one thread per pixel runs vo_sgm_select over the pixel's D contiguous sums.
// k_reconstruct: one thread per pixel, vo_reconstruct_point.
#include <algorithm>
#include "vo_internal.h"
#include "wave.h"

namespace vo {

#define SGM_TW 64
#define SGM_TH 16
#define SGM_PW (SGM_TW + 2 * VO_SGM_CENSUS_RX)           // 72
#define SGM_PH (SGM_TH + 2 * VO_SGM_CENSUS_RY)           // 22

// img(z): z = 2 * pair + side
__global__ __launch_bounds__(256) void k_sgm_census(const uint8_t* __restrict__ lefts, const uint8_t* __restrict__ rights, int rows,
                                                    int cols, uint64_t* __restrict__ cen)
{
    __shared__ uint8_t P[SGM_PH][SGM_PW];
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * SGM_TW, ty0 = blockIdx.y * SGM_TH;
    const size_t px = (size_t)rows * cols;
    const uint8_t* __restrict__ img = ((blockIdx.z & 1) ? rights : lefts) + (size_t)(blockIdx.z >> 1) * px;
    const int ox = tx0 - VO_SGM_CENSUS_RX, oy = ty0 - VO_SGM_CENSUS_RY;
    for (int e = tid; e < SGM_PW * SGM_PH; e += 256) {
        const int y = e / SGM_PW, x = e - y * SGM_PW;
        P[y][x] = img[(size_t)vo_sgm_clamp(oy + y, rows) * cols + vo_sgm_clamp(ox + x, cols)];
    }
    __syncthreads();
    const int x = tid & (SGM_TW - 1), c = tx0 + x;
    for (int y = tid >> 6; y < SGM_TH; y += 4) {
        const int r = ty0 + y;
        if (r >= rows || c >= cols) continue;
        const int ctr = P[y + VO_SGM_CENSUS_RY][x + VO_SGM_CENSUS_RX];
        uint64_t w = 0;
#pragma unroll
        for (int dy = 0; dy <= 2 * VO_SGM_CENSUS_RY; ++dy)
#pragma unroll
            for (int dx = 0; dx <= 2 * VO_SGM_CENSUS_RX; ++dx) {
                if (dy == VO_SGM_CENSUS_RY && dx == VO_SGM_CENSUS_RX) continue;
                w = (w << 1) | (uint64_t)((int)P[y + dy][x + dx] < ctr ? 1 : 0);
            }
        cen[(size_t)blockIdx.z * px + (size_t)r * cols + c] = w;
    }
}

struct SgmArgs {
    const uint64_t* cen;                                 // [pair][2][rows][cols]
    uint16_t* S;                                         // [pair][rows][cols][D]
    int rows, cols, D, dmin, P1, P2;
};

// one walk of len pixels from (y0, x0) in steps of (dy, dx): direction r = (dy, dx)
template <int NPL>
static __device__ __forceinline__ void sgm_walk(const uint64_t* __restrict__ cl, const uint64_t* __restrict__ cr, uint16_t* S,
                                                const SgmArgs& a, int y0, int x0, int dy, int dx, int len, bool add)
{
    const int lane = threadIdx.x & 63, k0 = lane * NPL;
    const int cols = a.cols, D = a.D;
    const bool act = k0 < D;                             // D is a multiple of 8: a lane's disparities are inside together
    uint32_t L[NPL];
    uint64_t wl = cl[(size_t)y0 * cols + x0], wr[NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) wr[q] = act ? cr[(size_t)y0 * cols + vo_sgm_right_col(x0, a.dmin + k0 + q, cols)] : 0ull;
    for (int t = 0; t < len; ++t) {
        const int y = y0 + t * dy, x = x0 + t * dx;
        uint64_t nl = 0ull, nr[NPL];
#pragma unroll
        for (int q = 0; q < NPL; ++q) nr[q] = 0ull;
        if (t + 1 < len) {                               // the next step's words: they do not depend on the recurrence
            const int ny = y + dy, nx = x + dx;
            nl = cl[(size_t)ny * cols + nx];
#pragma unroll
            for (int q = 0; q < NPL; ++q) if (act) nr[q] = cr[(size_t)ny * cols + vo_sgm_right_col(nx, a.dmin + k0 + q, cols)];
        }
        uint16_t* sp = S + ((size_t)y * cols + x) * D + k0;
        uint32_t old = 0;
        if (add && act) old = NPL == 2 ? *reinterpret_cast<const uint32_t*>(sp) : (uint32_t)*sp;
        int c[NPL];
#pragma unroll
        for (int q = 0; q < NPL; ++q) c[q] = vo_sgm_popcount(wl ^ wr[q]);
        if (t == 0) {
#pragma unroll
            for (int q = 0; q < NPL; ++q) L[q] = act ? (uint32_t)c[q] : (uint32_t)VO_SGM_ABSENT;
        } else {
            uint32_t mine = L[0];
            if (NPL == 2) mine = min(mine, L[NPL - 1]);
            const int m = (int)wave_min(mine);
            const uint32_t below = wave_shift_up(L[NPL - 1], (uint32_t)VO_SGM_ABSENT);     // L(k0 - 1)
            const uint32_t above = wave_shift_down(L[0], (uint32_t)VO_SGM_ABSENT);         // L(k0 + NPL)
            uint32_t n[NPL];
            if (NPL == 1) {
                n[0] = (uint32_t)vo_sgm_step(c[0], (int)L[0], (int)below, (int)above, m, a.P1, a.P2);
            } else {
                n[0] = (uint32_t)vo_sgm_step(c[0], (int)L[0], (int)below, (int)L[NPL - 1], m, a.P1, a.P2);
                n[NPL - 1] = (uint32_t)vo_sgm_step(c[NPL - 1], (int)L[NPL - 1], (int)L[0], (int)above, m, a.P1, a.P2);
            }
#pragma unroll
            for (int q = 0; q < NPL; ++q) L[q] = act ? n[q] : (uint32_t)VO_SGM_ABSENT;
        }
        if (act) {
            if (NPL == 2) *reinterpret_cast<uint32_t*>(sp) = ((old & 0xffffu) + L[0]) | (((old >> 16) + L[NPL - 1]) << 16);
            else *sp = (uint16_t)(old + L[0]);
        }
        wl = nl;
#pragma unroll
        for (int q = 0; q < NPL; ++q) wr[q] = nr[q];
    }
}

template <int H, int NPL>
__global__ __launch_bounds__(256) void k_sgm_paths(SgmArgs a, int first)
{
    const int rows = a.rows, cols = a.cols;
    const int path = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_paths = H == 0 ? rows : (H == 1 ? cols : rows + cols - 1);
    if (path >= n_paths) return;                         // the whole wave
    const size_t px = (size_t)rows * cols;
    const uint64_t* __restrict__ cl = a.cen + (size_t)blockIdx.y * 2 * px;
    const uint64_t* __restrict__ cr = cl + px;
    uint16_t* S = a.S + (size_t)blockIdx.y * px * a.D;
    int y0, x0, dy, dx, len;
    if (H == 0) { y0 = path; x0 = 0; dy = 0; dx = 1; len = cols; }
    else if (H == 1) { y0 = 0; x0 = path; dy = 1; dx = 0; len = rows; }
    else if (H == 2) {
        dy = 1; dx = 1;
        if (path < cols) { y0 = 0; x0 = path; } else { y0 = path - cols + 1; x0 = 0; }
        len = min(rows - y0, cols - x0);
    } else {
        dy = 1; dx = -1;
        if (path < cols) { y0 = 0; x0 = path; } else { y0 = path - cols + 1; x0 = cols - 1; }
        len = min(rows - y0, x0 + 1);
    }
    sgm_walk<NPL>(cl, cr, S, a, y0, x0, dy, dx, len, !first);
    sgm_walk<NPL>(cl, cr, S, a, y0 + (len - 1) * dy, x0 + (len - 1) * dx, -dy, -dx, len, true);
}

// pixel i of the output's storage order: row-major (y, x) = (i / cols, i % cols), col_major (i % rows, i / rows)
__global__ __launch_bounds__(256) void k_sgm_select(const uint16_t* __restrict__ S, int rows, int cols, int D, int dmin, int U,
                                                    int col_major, float* __restrict__ disp)
{
    const size_t px = (size_t)rows * cols;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= px) return;
    const int y = col_major ? (int)(i % rows) : (int)(i / cols), x = col_major ? (int)(i / rows) : (int)(i % cols);
    const uint16_t* s = S + ((size_t)blockIdx.y * px + (size_t)y * cols + x) * D;
    disp[(size_t)blockIdx.y * px + i] = vo_sgm_select(s, D, dmin, x, cols, U);
}

struct ReconQ { double q[16]; };

__global__ __launch_bounds__(256) void k_reconstruct(const float* __restrict__ disp, int rows, int cols, int col_major, ReconQ Q,
                                                     float* __restrict__ xyz)
{
    const size_t px = (size_t)rows * cols;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= px) return;
    const int y = col_major ? (int)(i % rows) : (int)(i / cols), x = col_major ? (int)(i / rows) : (int)(i % cols);
    float p[3];
    vo_reconstruct_point(Q.q, x + 1, y + 1, disp[i], p);
#pragma unroll
    for (int k = 0; k < 3; ++k) xyz[col_major ? (size_t)k * px + i : 3 * i + k] = p[k];
}

hipError_t sgm_reserve(DevPool& pool, SgmBuffers& sb, int rows, int cols, int n_group, int D, bool host_io)
{
    const size_t px = (size_t)rows * cols;
    if (n_group > sb.cap_pairs || D > sb.cap_D) {
        const int G = std::max(n_group, sb.cap_pairs), Dn = std::max(D, sb.cap_D);
        const int e = pool.grow({DevPool::req(sb.cen, (size_t)2 * G * px), DevPool::req(sb.S, (size_t)G * px * Dn)});
        if (e) return (hipError_t)e;
        sb.cap_pairs = G; sb.cap_D = Dn;
        sb.last_pairs = 0;                               // the sums of the last call went with the old buffer
    }
    if (host_io && n_group > sb.cap_io) {
        const int e = pool.grow({DevPool::req(sb.img, (size_t)2 * n_group * px), DevPool::req(sb.disp, (size_t)n_group * px)});
        if (e) return (hipError_t)e;
        sb.cap_io = n_group;
    }
    return hipSuccess;
}

template <int NPL>
static void sgm_paths_launch(const SgmArgs& a, int G, hipStream_t s)
{
    const int rows = a.rows, cols = a.cols, diag = rows + cols - 1;
    VO_LAUNCH_NAMED("k_sgm_paths_rows", (k_sgm_paths<0, NPL>), dim3((rows + 3) / 4, G), dim3(256), 0, s, a, 1);
    VO_LAUNCH_NAMED("k_sgm_paths_cols", (k_sgm_paths<1, NPL>), dim3((cols + 3) / 4, G), dim3(256), 0, s, a, 0);
    VO_LAUNCH_NAMED("k_sgm_paths_diag", (k_sgm_paths<2, NPL>), dim3((diag + 3) / 4, G), dim3(256), 0, s, a, 0);
    VO_LAUNCH_NAMED("k_sgm_paths_anti", (k_sgm_paths<3, NPL>), dim3((diag + 3) / 4, G), dim3(256), 0, s, a, 0);
}

void sgm_launch(SgmBuffers& sb, const uint8_t* d_lefts, const uint8_t* d_rights, int rows, int cols, int G, const vo_sgm_params& p,
                int col_major, float* d_disp, hipStream_t s)
{
    const int D = p.disparity_range[1] - p.disparity_range[0];
    const size_t px = (size_t)rows * cols;
    VO_LAUNCH(k_sgm_census, dim3((cols + SGM_TW - 1) / SGM_TW, (rows + SGM_TH - 1) / SGM_TH, 2 * G), dim3(256), 0, s, d_lefts, d_rights,
              rows, cols, sb.cen);
    SgmArgs a;
    a.cen = sb.cen; a.S = sb.S; a.rows = rows; a.cols = cols; a.D = D; a.dmin = p.disparity_range[0]; a.P1 = p.p1; a.P2 = p.p2;
    if (D <= 64) sgm_paths_launch<1>(a, G, s); else sgm_paths_launch<2>(a, G, s);
    VO_LAUNCH(k_sgm_select, dim3((unsigned)((px + 255) / 256), G), dim3(256), 0, s, (const uint16_t*)sb.S, rows, cols, D, a.dmin,
              p.uniqueness_threshold, col_major, d_disp);
}

hipError_t reconstruct_reserve(DevPool& pool, SgmBuffers& sb, int rows, int cols)
{
    if (sb.rin) return hipSuccess;
    const size_t px = (size_t)rows * cols;
    return (hipError_t)pool.group({DevPool::req(sb.rin, px), DevPool::req(sb.xyz, 3 * px)});
}

void reconstruct_launch(const float* d_disp, int rows, int cols, int col_major, const double* Q, float* d_xyz, hipStream_t s)
{
    ReconQ q;
    for (int k = 0; k < 16; ++k) q.q[k] = Q[k];
    const size_t px = (size_t)rows * cols;
    VO_LAUNCH(k_reconstruct, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, d_disp, rows, cols, col_major, q, d_xyz);
}

}  // namespace vo
