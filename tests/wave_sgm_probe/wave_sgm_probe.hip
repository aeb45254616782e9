// wave_sgm_probe.hip — thin kernels around wave_shift_up / wave_shift_down of csrc/wave.h and around the step
// k_sgm_paths builds from them with wave_min (test infrastructure, not part of libvo.so).  Every thread loads
// its element, calls the collective and stores what the call returned for that thread; tests/wave_sgm_probe.py
// compares every thread's value with a NumPy restatement.
//
// Arrays are [nblocks][nwaves * 64] 4-byte elements; one launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave.h"

namespace wave_sgm_probe {

using namespace vo;

enum Fn { FN_SHIFT_UP = 0, FN_SHIFT_DOWN, FN_MIN_AND_NEIGHBOURS, FN_COUNT };

template <typename T, bool UP>
__global__ __launch_bounds__(256) void k_shift(const T* __restrict__ in, T fill, T* __restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    out[e] = UP ? wave_shift_up(in[e], fill) : wave_shift_down(in[e], fill);
}

// the three collectives of one path step on the same register, as k_sgm_paths issues them: out0 = the wave's
// minimum, out1 = the lower neighbour's value, out2 = the upper neighbour's
__global__ __launch_bounds__(256) void k_min_and_neighbours(const uint32_t* __restrict__ in, uint32_t fill, uint32_t* __restrict__ out0,
                                                            uint32_t* __restrict__ out1, uint32_t* __restrict__ out2)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t v = in[e];
    out0[e] = wave_min(v);
    out1[e] = wave_shift_up(v, fill);
    out2[e] = wave_shift_down(v, fill);
}

}  // namespace wave_sgm_probe

// host: in [n] 4-byte elements, n = nblocks * nwaves * 64; out0 (and out1, out2 for fn 2) [n].  type: 0 uint32, 1 float.
// -> 0, -1 (arguments) or a hipError_t
extern "C" int wave_sgm_probe_run(int fn, int type, int nwaves, int nblocks, const void* in, const void* fill, void* out0, void* out1,
                                  void* out2)
{
    using namespace wave_sgm_probe;
    if (fn < 0 || fn >= FN_COUNT || type < 0 || type > 1 || nwaves < 1 || nwaves > 4 || nblocks < 1 || nblocks > 256 || !in || !fill || !out0)
        return -1;
    if (fn == FN_MIN_AND_NEIGHBOURS && (type != 0 || !out1 || !out2)) return -1;
    const size_t n = (size_t)nblocks * nwaves * 64, bytes = 4 * n;
    void* d[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t err = hipSuccess;
    for (int k = 0; k < 4 && err == hipSuccess; ++k) err = hipMalloc(&d[k], bytes);
    if (err == hipSuccess) err = hipMemcpy(d[0], in, bytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        const dim3 grid(nblocks), block(nwaves * 64);
        if (fn == FN_MIN_AND_NEIGHBOURS)
            hipLaunchKernelGGL(k_min_and_neighbours, grid, block, 0, 0, (const uint32_t*)d[0], *(const uint32_t*)fill, (uint32_t*)d[1],
                               (uint32_t*)d[2], (uint32_t*)d[3]);
        else if (type == 0 && fn == FN_SHIFT_UP)
            hipLaunchKernelGGL((k_shift<uint32_t, true>), grid, block, 0, 0, (const uint32_t*)d[0], *(const uint32_t*)fill, (uint32_t*)d[1]);
        else if (type == 0)
            hipLaunchKernelGGL((k_shift<uint32_t, false>), grid, block, 0, 0, (const uint32_t*)d[0], *(const uint32_t*)fill, (uint32_t*)d[1]);
        else if (fn == FN_SHIFT_UP)
            hipLaunchKernelGGL((k_shift<float, true>), grid, block, 0, 0, (const float*)d[0], *(const float*)fill, (float*)d[1]);
        else
            hipLaunchKernelGGL((k_shift<float, false>), grid, block, 0, 0, (const float*)d[0], *(const float*)fill, (float*)d[1]);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(out0, d[1], bytes, hipMemcpyDeviceToHost);
    if (err == hipSuccess && fn == FN_MIN_AND_NEIGHBOURS) err = hipMemcpy(out1, d[2], bytes, hipMemcpyDeviceToHost);
    if (err == hipSuccess && fn == FN_MIN_AND_NEIGHBOURS) err = hipMemcpy(out2, d[3], bytes, hipMemcpyDeviceToHost);
    for (int k = 0; k < 4; ++k) if (d[k]) (void)hipFree(d[k]);
    return (int)err;
}
