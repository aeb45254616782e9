// base_probe.hip — where the octave-0 base kernel's time goes (instrumentation, not libvo).
// k_blur_stream<5, TAG=5> builds G0 (x2 upsample fused, r = 5 blur) of 128 images of 375 x 1242
// u8 into 750 x 2484 planes (pitch 2560), as bench's batch of 64 stereo frames does.  Variants:
// TAG bits 8 (no row pass), 16 (no column pass), 32 (no LDS staging); and a write-only strip
// reference (every wave stores its band rows, nothing else) = the floor of this store pattern.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I include -I r7020e-visual-odometry_amd/csrc tools/base_probe.hip -o tools/base_probe
#include "../r7020e-visual-odometry_amd/csrc/sift.hip"
#include <cstdio>
#include <hip/hip_ext.h>

using namespace vo;
namespace vo {
thread_local Profiler* g_prof = nullptr;
void Profiler::begin(const char*, hipStream_t) {}
void Profiler::end(hipStream_t) {}
void Profiler::collect() {}
void Profiler::reset_totals() {}
Profiler::~Profiler() {}
}

// MODE 0: strips of sw columns (sw = 256: aligned 1-KB row segments; 240: the base kernel's
// halo-lane strips, 960-B segments that start mid-line for every other strip), XCD-contiguous
// ids, strip fastest, non-temporal stores; 1: no XCD remap; 2: plain stores; 3: each wave writes
// TH KB of contiguous bytes instead (same total, bounded to the buffer); 16 + n: MODE 0 paced by
// s_sleep n after every row (the base kernel issues one row store per ~row-pass of work)
template <int MODE>
__global__ __launch_bounds__(64) void k_store_strip(float* __restrict__ b, int pitch, int R, size_t plane, int n_strips,
                                                    int n_bands, int TH, int sw, size_t cap_f4)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int bid = MODE == 1 ? (int)blockIdx.x : xcd_remap(blockIdx.x, gridDim.x);
    if (MODE == 3) {
        const size_t first = (size_t)bid * TH * 64;
        if (first + (size_t)TH * 64 > cap_f4) return;
        f4* p = reinterpret_cast<f4*>(b) + first + threadIdx.x;
        const f4 v = {1.0f, 2.0f, 3.0f, (float)bid};
        for (int k = 0; k < TH; ++k) __builtin_nontemporal_store(v, p + (size_t)k * 64);
        return;
    }
    const int strip = bid % n_strips, tb = bid / n_strips, band = tb % n_bands, img = tb / n_bands;
    const int x0 = strip * sw, y0 = min(band * TH, R - TH);
    const int xl = x0 + 4 * (int)threadIdx.x;
    if (4 * (int)threadIdx.x >= sw || xl + 4 > pitch) return;
    float* bp = b + img * plane;
    const f4 v = {1.0f, 2.0f, 3.0f, (float)img};
    for (int k = 0; k < TH; ++k) {
        f4* q = reinterpret_cast<f4*>(bp + (size_t)(y0 + k) * pitch + xl);
        if (MODE == 2) *q = v; else __builtin_nontemporal_store(v, q);
        if constexpr (MODE >= 16) __builtin_amdgcn_s_sleep(MODE - 16);   // paced: ~64 (MODE-16) cycles per row
    }
}

// throughput-bound VALU work (8 independent FMA chains per lane): its time must scale with the
// number of CUs a stream may use, which checks that a CU mask is honoured
__global__ __launch_bounds__(64) void k_valu(float* out, int iters)
{
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = threadIdx.x * 1e-3f + j;
    for (int i = 0; i < iters; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = __builtin_fmaf(a[j], 1.0001f, 1e-7f);
    float t = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) t += a[j];
    if (t == 12345.0f) out[blockIdx.x] = t;
}

static float run_valu(float* out, hipStream_t st)
{
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    hipLaunchKernelGGL(k_valu, dim3(16384), dim3(64), 0, st, out, 2000);
    hipEventRecord(a, st);
    hipLaunchKernelGGL(k_valu, dim3(16384), dim3(64), 0, st, out, 2000);
    hipEventRecord(b, st);
    hipEventSynchronize(b);
    float ms;
    hipEventElapsedTime(&ms, a, b);
    return 1000.0f * ms;
}

template <int TAG>
static float run(const uint8_t* u8, float* dst, size_t plane, int pitch, int R, int C, int n_img, int TH, const Kern& K,
                 hipStream_t st = 0)
{
    // strips of bs_sw(5, 4, TAG) output columns (halo-lane layout: 240)
    const int n_strips = blur_grid_strips(C, 5, 4, TAG), n_bands = blur_bands(R, TH);
    const int blocks = n_strips * n_bands * n_img;
    const size_t fs = (size_t)(R / 2) * (C / 2);
    ImageSrc isrc{u8, u8 + fs * (n_img / 2), fs, C / 2, 0};
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    for (int w = 0; w < 2; ++w)
        hipLaunchKernelGGL((k_blur_stream<5, TAG, 4>), dim3(blocks), dim3(64), 0, st, nullptr, 0, plane, pitch, R, C, dst, K,
                           n_strips, n_bands, TH, isrc, R / 2, C / 2);
    hipEventRecord(a, st);
    for (int i = 0; i < 10; ++i)
        hipLaunchKernelGGL((k_blur_stream<5, TAG, 4>), dim3(blocks), dim3(64), 0, st, nullptr, 0, plane, pitch, R, C, dst, K,
                           n_strips, n_bands, TH, isrc, R / 2, C / 2);
    hipEventRecord(b, st);
    hipEventSynchronize(b);
    float ms;
    hipEventElapsedTime(&ms, a, b);
    return 100.0f * ms;
}

int main()
{
    const int R = 750, C = 2484, n = 128, pitch = 2560;
    const size_t plane = (size_t)R * pitch;
    float* dst;
    uint8_t* u8;
    hipMalloc(&dst, sizeof(float) * plane * n);
    hipMalloc(&u8, (size_t)(R / 2) * (C / 2) * n);
    hipMemset(u8, 77, (size_t)(R / 2) * (C / 2) * n);
    Kern K{};
    K.r = 5;
    for (int j = 0; j <= 5; ++j) K.k[j] = 1.0f / 11;
    const double gb = 4.0 * R * C * n / 1e9;
    auto store_only = [&](auto kern, int TH, int sw) {
        const int n_strips = (C + sw - 1) / sw, n_bands = (R + TH - 1) / TH;
        const size_t cap = plane * n / 4;
        hipEvent_t a, b;
        hipEventCreate(&a); hipEventCreate(&b);
        hipLaunchKernelGGL(kern, dim3(n_strips * n_bands * n), dim3(64), 0, 0, dst, pitch, R, plane, n_strips, n_bands, TH, sw, cap);
        hipEventRecord(a);
        for (int i = 0; i < 10; ++i)
            hipLaunchKernelGGL(kern, dim3(n_strips * n_bands * n), dim3(64), 0, 0, dst, pitch, R, plane, n_strips, n_bands, TH, sw, cap);
        hipEventRecord(b);
        hipEventSynchronize(b);
        float ms;
        hipEventElapsedTime(&ms, a, b);
        return 100.0f * ms;     // us per launch
    };
    auto store_only_s = [&](hipStream_t st) {
        const int TH = 128, n_strips = (C + 255) / 256, n_bands = (R + TH - 1) / TH;
        hipEvent_t a, b;
        hipEventCreate(&a); hipEventCreate(&b);
        hipLaunchKernelGGL(k_store_strip<0>, dim3(n_strips * n_bands * n), dim3(64), 0, st, dst, pitch, R, plane, n_strips, n_bands, TH, 256, (size_t)0);
        hipEventRecord(a, st);
        for (int i = 0; i < 10; ++i)
            hipLaunchKernelGGL(k_store_strip<0>, dim3(n_strips * n_bands * n), dim3(64), 0, st, dst, pitch, R, plane, n_strips, n_bands, TH, 256, (size_t)0);
        hipEventRecord(b, st);
        hipEventSynchronize(b);
        float ms;
        hipEventElapsedTime(&ms, a, b);
        return 100.0f * ms;
    };
    for (int TH : {64, 128}) {
        const int nb = (R + TH - 1) / TH;
        auto gbs = [&](int sw) { return 4.0 * sw * TH * ((C + sw - 1) / sw) * nb * n / 1e9; };   // bytes the strip stores write
        const float m0 = store_only(k_store_strip<0>, TH, 256), m1 = store_only(k_store_strip<1>, TH, 256);
        const float m2 = store_only(k_store_strip<2>, TH, 256), m3 = store_only(k_store_strip<3>, TH, 256);
        const float m4 = store_only(k_store_strip<0>, TH, 240), m5 = store_only(k_store_strip<0>, TH, 224);
        const float m6 = store_only(k_store_strip<2>, TH, 240);
        printf("TH %3d store-only TB/s: 256-col strips %5.2f | no XCD remap %5.2f | plain stores %5.2f | contiguous %5.2f | "
               "240-col %5.2f | 224-col %5.2f | 240-col plain %5.2f\n", TH, gbs(256) / m0 * 1e3, gbs(256) / m1 * 1e3,
               gbs(256) / m2 * 1e3, gbs(256) / m3 * 1e3, gbs(240) / m4 * 1e3, gbs(224) / m5 * 1e3, gbs(240) / m6 * 1e3);
    }
    for (int TH : {64, 128}) {
        const int nb = (R + TH - 1) / TH;
        const double g = 4.0 * 256 * TH * ((C + 255) / 256) * nb * n / 1e9;
        printf("TH %3d paced store-only TB/s: s_sleep 1 %5.2f | 2 %5.2f | 4 %5.2f | 8 %5.2f | 15 %5.2f\n", TH,
               g / store_only(k_store_strip<17>, TH, 256) * 1e3, g / store_only(k_store_strip<18>, TH, 256) * 1e3,
               g / store_only(k_store_strip<20>, TH, 256) * 1e3, g / store_only(k_store_strip<24>, TH, 256) * 1e3,
               g / store_only(k_store_strip<31>, TH, 256) * 1e3);
    }
    for (int TH : {32, 64, 96}) {                          // the staged base takes bands of <= kBaseMaxTH (96) rows
        const float ms = store_only(k_store_strip<0>, TH, 256) / 100.0f;
        const float t0 = run<kTagBaseU8>(u8, dst, plane, pitch, R, C, n, TH, K);
        const float t8 = run<kTagBaseU8 | kTagNoRowPass>(u8, dst, plane, pitch, R, C, n, TH, K);
        const float t24 = run<kTagBaseU8 | kTagNoRowPass | kTagNoColPass>(u8, dst, plane, pitch, R, C, n, TH, K);
        const float t56 = run<kTagBaseU8 | kTagNoRowPass | kTagNoColPass | kTagNoLds>(u8, dst, plane, pitch, R, C, n, TH, K);
        printf("TH %3d: store-only %6.1f us (%5.2f TB/s) | base %6.1f us (%5.2f TB/s) | no-row %6.1f | no row/col %6.1f | "
               "no row/col/LDS %6.1f\n", TH, 100.0f * ms, gb / (100.0f * ms) * 1e3, t0, gb / t0 * 1e3, t8, t24, t56);
    }
    // the same kernels on CU-masked streams: interleaved masks (bit i set when i % div == 0) and
    // contiguous ones (the first n_cu / div bits); the VALU-bound kernel shows whether a mask binds
    int n_cu = 0;
    hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, 0);
    printf("CUs %d\n", n_cu);
    for (int contig = 0; contig < 2; ++contig)
        for (int div : {1, 2, 4, 8, 64}) {
            uint32_t m[16] = {};
            for (int i = 0; i < n_cu && i < 512; ++i)
                if (contig ? i < n_cu / div : i % div == 0) m[i / 32] |= 1u << (i % 32);
            hipStream_t st;
            const hipError_t e = hipExtStreamCreateWithCUMask(&st, (uint32_t)((n_cu + 31) / 32), m);
            if (e != hipSuccess) { printf("%s 1/%d: %s\n", contig ? "contiguous" : "interleaved", div, hipGetErrorString(e)); continue; }
            printf("%s CU mask 1/%d: VALU-bound %7.1f us | base %6.1f us (TH 96) | store-only %6.1f us\n",
                   contig ? "contiguous" : "interleaved", div, run_valu(reinterpret_cast<float*>(u8), st),
                   div <= 8 ? run<kTagBaseU8>(u8, dst, plane, pitch, R, C, n, 96, K, st) : 0.0f, div <= 8 ? store_only_s(st) : 0.0f);
        }
    return 0;
}
