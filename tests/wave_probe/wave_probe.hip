// wave_probe.hip — thin kernels around the collectives of csrc/wave.h and csrc/match_merge.h (test
// infrastructure, not part of libvo.so).  Every thread loads its input element(s), calls one collective
// and stores what the call returned for that thread; tests/wave_probe.py compares every thread's value
// with a NumPy restatement.  Built with csrc/Makefile's flags, so the bodies are the ones the kernels get.
//
// Layout of every array: [nblocks][rounds][NWAVES * 64] elements (wave_sum_xor<N>: N values per element),
// block b handles its `rounds` slices in turn, all in one launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave.h"
#include "match_merge.h"

namespace wave_probe {

using namespace vo;

enum Fn {
    FN_WAVE_SUM = 0, FN_WAVE_SUM_XOR, FN_WAVE_SUM_XOR_N, FN_WAVE_MAX, FN_WAVE_MIN, FN_WAVE_INCL_SCAN, FN_WAVE_RANK,
    FN_BLOCK_EXCL_SCAN, FN_BLOCK_SUM, FN_BLOCK_EXSCAN_1024, FN_BLOCK_EXSCAN_256, FN_TOP2C_MERGE_LANES, FN_TOP2S_MERGE_WAVE,
    FN_MATCH_PLACE, FN_COUNT
};
enum Ty { TY_I32 = 0, TY_U32, TY_F32, TY_I64, TY_F64, TY_COUNT };

__device__ __forceinline__ size_t elem(int rounds, int r)
{
    return ((size_t)blockIdx.x * rounds + r) * blockDim.x + threadIdx.x;
}

struct OpSum { template <typename T> static __device__ __forceinline__ T run(T v) { return wave_sum(v); } };
struct OpSumXor { template <typename T> static __device__ __forceinline__ T run(T v) { return wave_sum_xor(v); } };
struct OpMax { template <typename T> static __device__ __forceinline__ T run(T v) { return wave_max(v); } };
struct OpMin { template <typename T> static __device__ __forceinline__ T run(T v) { return wave_min(v); } };
struct OpScan { template <typename T> static __device__ __forceinline__ T run(T v) { return wave_incl_scan(v); } };

// one value per thread through a wave function; blocks of 1 or 4 waves
template <typename Op, typename T>
__global__ __launch_bounds__(256) void k_wave(const T* __restrict__ in, T* __restrict__ out, int rounds)
{
    for (int r = 0; r < rounds; ++r) {
        const size_t e = elem(rounds, r);
        out[e] = Op::run(in[e]);
    }
}

template <int N, typename T>
__global__ __launch_bounds__(256) void k_wave_sum_xor_n(const T* __restrict__ in, T* __restrict__ out, int rounds)
{
    for (int r = 0; r < rounds; ++r) {
        const size_t e = elem(rounds, r);
        T v[N];
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = in[e * N + q];
        wave_sum_xor<N>(v);
#pragma unroll
        for (int q = 0; q < N; ++q) out[e * N + q] = v[q];
    }
}

__global__ __launch_bounds__(256) void k_wave_rank(const int* __restrict__ in, int* __restrict__ rank, int* __restrict__ count, int rounds)
{
    for (int r = 0; r < rounds; ++r) {
        const size_t e = elem(rounds, r);
        int cnt;
        rank[e] = wave_rank(in[e] != 0, &cnt);
        count[e] = cnt;
    }
}

// called in a loop over the same LDS words: "free again at return"
template <int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) void k_block_excl_scan(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                 uint32_t* __restrict__ total, int rounds)
{
    __shared__ uint32_t sh[NWAVES];
    for (int r = 0; r < rounds; ++r) {
        const size_t e = elem(rounds, r);
        uint32_t t;
        out[e] = block_excl_scan<NWAVES>(in[e], sh, &t);
        total[e] = t;
    }
}

// sh is read until the next barrier: the caller's barrier stands between the calls
template <int NWAVES, typename T>
__global__ __launch_bounds__(NWAVES * 64) void k_block_sum(const T* __restrict__ in, T* __restrict__ out, int rounds)
{
    __shared__ T sh[NWAVES];
    for (int r = 0; r < rounds; ++r) {
        const size_t e = elem(rounds, r);
        if (r) __syncthreads();
        out[e] = block_sum<NWAVES, T>(in[e], sh);
    }
}

__global__ __launch_bounds__(1024) void k_block_exscan_1024(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                            uint32_t* __restrict__ total, int rounds)
{
    __shared__ uint32_t sh[32];
    for (int r = 0; r < rounds; ++r) {
        const size_t e = elem(rounds, r);
        uint32_t t;
        out[e] = block_exscan_1024(in[e], sh, &t);
        total[e] = t;
    }
}

__global__ __launch_bounds__(256) void k_block_exscan_256(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int rounds)
{
    __shared__ uint32_t sh[4];
    for (int r = 0; r < rounds; ++r) {
        const size_t e = elem(rounds, r);
        if (r) __syncthreads();                                   // it ends without one
        out[e] = block_exscan_256(in[e], sh);
    }
}

template <bool S>
__global__ __launch_bounds__(256) void k_top2(const float* __restrict__ ib, const int* __restrict__ ii, const float* __restrict__ is,
                                              float* __restrict__ ob, int* __restrict__ oi, float* __restrict__ os, int rounds)
{
    for (int r = 0; r < rounds; ++r) {
        const size_t e = elem(rounds, r);
        float b = ib[e], s = is[e];
        int i = ii[e];
        if constexpr (S) top2s_merge_wave(b, i, s);
        else top2c_merge_lanes(b, i, s, 32);
        ob[e] = b;
        oi[e] = i;
        os[e] = s;
    }
}

// base is carried from round to round, as k_match_finish carries it from tile to tile
__global__ __launch_bounds__(256) void k_match_place(const int* __restrict__ in, uint32_t* __restrict__ pos, uint32_t* __restrict__ base_out,
                                                     int rounds)
{
    __shared__ uint32_t wsum[4];
    uint32_t base = 0;
    for (int r = 0; r < rounds; ++r) {
        const size_t e = elem(rounds, r);
        pos[e] = match_place(in[e] != 0, wsum, base);
        base_out[e] = base;
    }
}

struct Arrays {
    size_t bytes[6] = {0, 0, 0, 0, 0, 0};       // in0 in1 in2 out0 out1 out2
    void* dev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

template <typename T> T* in_(Arrays& a, int k) { return (T*)a.dev[k]; }
template <typename T> T* out_(Arrays& a, int k) { return (T*)a.dev[3 + k]; }

template <typename Op>
bool launch_wave(int type, Arrays& a, dim3 g, dim3 b, int rounds)
{
    switch (type) {
    case TY_I32: k_wave<Op, int><<<g, b>>>(in_<int>(a, 0), out_<int>(a, 0), rounds); return true;
    case TY_U32: k_wave<Op, uint32_t><<<g, b>>>(in_<uint32_t>(a, 0), out_<uint32_t>(a, 0), rounds); return true;
    default: break;
    }
    if constexpr (!std::is_same_v<Op, OpScan>) {
        if (type == TY_F32) { k_wave<Op, float><<<g, b>>>(in_<float>(a, 0), out_<float>(a, 0), rounds); return true; }
    }
    if constexpr (std::is_same_v<Op, OpSum> || std::is_same_v<Op, OpSumXor>) {
        if (type == TY_I64) { k_wave<Op, int64_t><<<g, b>>>(in_<int64_t>(a, 0), out_<int64_t>(a, 0), rounds); return true; }
        if (type == TY_F64) { k_wave<Op, double><<<g, b>>>(in_<double>(a, 0), out_<double>(a, 0), rounds); return true; }
    }
    return false;
}

template <int NW>
bool launch_block_sum(int type, Arrays& a, dim3 g, int rounds)
{
    const dim3 b(NW * 64);
    switch (type) {
    case TY_I32: k_block_sum<NW, int><<<g, b>>>(in_<int>(a, 0), out_<int>(a, 0), rounds); return true;
    case TY_U32: k_block_sum<NW, uint32_t><<<g, b>>>(in_<uint32_t>(a, 0), out_<uint32_t>(a, 0), rounds); return true;
    case TY_F32: k_block_sum<NW, float><<<g, b>>>(in_<float>(a, 0), out_<float>(a, 0), rounds); return true;
    case TY_F64: k_block_sum<NW, double><<<g, b>>>(in_<double>(a, 0), out_<double>(a, 0), rounds); return true;
    default: return false;
    }
}

template <int NW>
bool launch_excl_scan(Arrays& a, dim3 g, int rounds)
{
    k_block_excl_scan<NW><<<g, dim3(NW * 64)>>>(in_<uint32_t>(a, 0), out_<uint32_t>(a, 0), out_<uint32_t>(a, 1), rounds);
    return true;
}

const size_t TY_SIZE[TY_COUNT] = {4, 4, 4, 8, 8};

// which arrays (fn, type) uses and how large each is; false: no such kernel
bool plan(int fn, int type, int nwaves, size_t n, Arrays& a)
{
    if (type < 0 || type >= TY_COUNT) return false;
    const size_t es = TY_SIZE[type];
    const bool wave_block = nwaves == 1 || nwaves == 4;
    const bool t4 = type == TY_I32 || type == TY_U32 || type == TY_F32;
    switch (fn) {
    case FN_WAVE_SUM: case FN_WAVE_SUM_XOR:
        if (!wave_block) return false;
        a.bytes[0] = a.bytes[3] = n * es;
        return true;
    case FN_WAVE_SUM_XOR_N:
        if (!wave_block || (type != TY_I32 && type != TY_F64)) return false;
        a.bytes[0] = a.bytes[3] = n * es * (type == TY_I32 ? 3 : 28);
        return true;
    case FN_WAVE_MAX: case FN_WAVE_MIN:
        if (!wave_block || (type != TY_F32 && type != TY_U32)) return false;
        a.bytes[0] = a.bytes[3] = n * 4;
        return true;
    case FN_WAVE_INCL_SCAN:
        if (!wave_block || (type != TY_I32 && type != TY_U32)) return false;
        a.bytes[0] = a.bytes[3] = n * 4;
        return true;
    case FN_WAVE_RANK:
        if (!wave_block || type != TY_I32) return false;
        a.bytes[0] = a.bytes[3] = a.bytes[4] = n * 4;
        return true;
    case FN_BLOCK_EXCL_SCAN:
        if (type != TY_U32) return false;
        if (nwaves != 1 && nwaves != 2 && nwaves != 3 && nwaves != 4 && nwaves != 8 && nwaves != 15 && nwaves != 16) return false;
        a.bytes[0] = a.bytes[3] = a.bytes[4] = n * 4;
        return true;
    case FN_BLOCK_SUM:
        if (!(t4 || type == TY_F64)) return false;
        if (nwaves != 1 && nwaves != 2 && nwaves != 3 && nwaves != 4 && nwaves != 16) return false;
        a.bytes[0] = a.bytes[3] = n * es;
        return true;
    case FN_BLOCK_EXSCAN_1024:
        if (type != TY_U32 || nwaves != 16) return false;
        a.bytes[0] = a.bytes[3] = a.bytes[4] = n * 4;
        return true;
    case FN_BLOCK_EXSCAN_256:
        if (type != TY_U32 || nwaves != 4) return false;
        a.bytes[0] = a.bytes[3] = n * 4;
        return true;
    case FN_TOP2C_MERGE_LANES: case FN_TOP2S_MERGE_WAVE:
        if (!wave_block || type != TY_F32) return false;
        for (int k = 0; k < 6; ++k) a.bytes[k] = n * 4;
        return true;
    case FN_MATCH_PLACE:
        if (type != TY_I32 || nwaves != 4) return false;
        a.bytes[0] = a.bytes[3] = a.bytes[4] = n * 4;
        return true;
    default:
        return false;
    }
}

bool launch(int fn, int type, int nwaves, Arrays& a, dim3 g, int rounds)
{
    const dim3 b(nwaves * 64);
    switch (fn) {
    case FN_WAVE_SUM: return launch_wave<OpSum>(type, a, g, b, rounds);
    case FN_WAVE_SUM_XOR: return launch_wave<OpSumXor>(type, a, g, b, rounds);
    case FN_WAVE_SUM_XOR_N:
        if (type == TY_I32) k_wave_sum_xor_n<3, int><<<g, b>>>(in_<int>(a, 0), out_<int>(a, 0), rounds);
        else k_wave_sum_xor_n<28, double><<<g, b>>>(in_<double>(a, 0), out_<double>(a, 0), rounds);
        return true;
    case FN_WAVE_MAX: return launch_wave<OpMax>(type, a, g, b, rounds);
    case FN_WAVE_MIN: return launch_wave<OpMin>(type, a, g, b, rounds);
    case FN_WAVE_INCL_SCAN: return launch_wave<OpScan>(type, a, g, b, rounds);
    case FN_WAVE_RANK: k_wave_rank<<<g, b>>>(in_<int>(a, 0), out_<int>(a, 0), out_<int>(a, 1), rounds); return true;
    case FN_BLOCK_EXCL_SCAN:
        switch (nwaves) {
        case 1: return launch_excl_scan<1>(a, g, rounds);
        case 2: return launch_excl_scan<2>(a, g, rounds);
        case 3: return launch_excl_scan<3>(a, g, rounds);
        case 4: return launch_excl_scan<4>(a, g, rounds);
        case 8: return launch_excl_scan<8>(a, g, rounds);
        case 15: return launch_excl_scan<15>(a, g, rounds);
        case 16: return launch_excl_scan<16>(a, g, rounds);
        default: return false;
        }
    case FN_BLOCK_SUM:
        switch (nwaves) {
        case 1: return launch_block_sum<1>(type, a, g, rounds);
        case 2: return launch_block_sum<2>(type, a, g, rounds);
        case 3: return launch_block_sum<3>(type, a, g, rounds);
        case 4: return launch_block_sum<4>(type, a, g, rounds);
        case 16: return launch_block_sum<16>(type, a, g, rounds);
        default: return false;
        }
    case FN_BLOCK_EXSCAN_1024:
        k_block_exscan_1024<<<g, b>>>(in_<uint32_t>(a, 0), out_<uint32_t>(a, 0), out_<uint32_t>(a, 1), rounds);
        return true;
    case FN_BLOCK_EXSCAN_256: k_block_exscan_256<<<g, b>>>(in_<uint32_t>(a, 0), out_<uint32_t>(a, 0), rounds); return true;
    case FN_TOP2C_MERGE_LANES:
        k_top2<false><<<g, b>>>(in_<float>(a, 0), in_<int>(a, 1), in_<float>(a, 2), out_<float>(a, 0), out_<int>(a, 1), out_<float>(a, 2), rounds);
        return true;
    case FN_TOP2S_MERGE_WAVE:
        k_top2<true><<<g, b>>>(in_<float>(a, 0), in_<int>(a, 1), in_<float>(a, 2), out_<float>(a, 0), out_<int>(a, 1), out_<float>(a, 2), rounds);
        return true;
    case FN_MATCH_PLACE: k_match_place<<<g, b>>>(in_<int>(a, 0), out_<uint32_t>(a, 0), out_<uint32_t>(a, 1), rounds); return true;
    default: return false;
    }
}

}  // namespace wave_probe

// Runs collective `fn` at (type, nwaves) over nblocks blocks x rounds slices.  host[k] / bytes[k], k = 0 .. 5:
// the three input and three output arrays (unused ones: null / 0).  The sizes must be the ones the kernel
// will index, or nothing is launched.  Returns the HIP error code (0 = success), -1 for a bad argument.
extern "C" int wave_probe_run(int fn, int type, int nwaves, int nblocks, int rounds, void* const* host, const size_t* bytes)
{
    using namespace wave_probe;
    if (nblocks < 1 || nblocks > 256 || rounds < 1 || rounds > 8 || nwaves < 1 || nwaves > 16) return -1;
    Arrays a;
    if (!plan(fn, type, nwaves, (size_t)nblocks * rounds * nwaves * 64, a)) return -1;
    for (int k = 0; k < 6; ++k)
        if (bytes[k] != a.bytes[k] || ((a.bytes[k] != 0) != (host[k] != nullptr))) return -1;
    hipError_t err = hipSuccess;
    for (int k = 0; k < 6 && err == hipSuccess; ++k)
        if (a.bytes[k]) err = hipMalloc(&a.dev[k], a.bytes[k]);
    for (int k = 0; k < 3 && err == hipSuccess; ++k)
        if (a.bytes[k]) err = hipMemcpy(a.dev[k], host[k], a.bytes[k], hipMemcpyHostToDevice);
    for (int k = 3; k < 6 && err == hipSuccess; ++k)
        if (a.bytes[k]) err = hipMemset(a.dev[k], 0xA5, a.bytes[k]);       // an element never stored shows
    if (err == hipSuccess) {
        if (!launch(fn, type, nwaves, a, dim3(nblocks), rounds)) err = hipErrorInvalidValue;
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    for (int k = 3; k < 6 && err == hipSuccess; ++k)
        if (a.bytes[k]) err = hipMemcpy(host[k], a.dev[k], a.bytes[k], hipMemcpyDeviceToHost);
    for (int k = 0; k < 6; ++k)
        if (a.dev[k]) (void)hipFree(a.dev[k]);
    return (int)err;
}
