// wave.h — the wave (64 lanes) and block collectives of libvo's kernels, each once.  Device only.
//
// Every function is called by a whole wave, converged: all 64 lanes active and at the same call;
// blocks are 1-D, and the block functions are called by every thread of NWAVES whole waves.  An
// inactive lane is no fault: the row shifts read 0 or stale registers for it, the result is wrong.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace vo {

// Lane 0's p[0] of  p[l] = op(p[l], p[l + off]), off = 32 .. 1  over the 64 lanes' 4-byte values, in
// every lane, without LDS: v_permlane32_swap / v_permlane16_swap give lanes < 32 / 16 the value of
// lane l + 32 / 16, DPP row_shl that of lane l + 8 .. 1 in the lane's row of 16.  A lane whose row has
// no such lane gets 0 (ZERO: a sum) or its own value; lane 0 always has one.
template <bool ZERO, typename T, typename Op>
__device__ __forceinline__ T wave_tree(T v, Op op)
{
    static_assert(sizeof(T) == 4, "one register per lane");
    auto bits = [](T x) { return __builtin_bit_cast(int, x); };
    auto val = [](int x) { return __builtin_bit_cast(T, x); };
#define VO_ROW_SHL(n) val(ZERO ? __builtin_amdgcn_update_dpp(0, bits(v), 0x100 + n, 0xF, 0xF, true) \
                               : __builtin_amdgcn_update_dpp(bits(v), bits(v), 0x100 + n, 0xF, 0xF, false))
    v = op(v, val(__builtin_amdgcn_permlane32_swap(bits(v), bits(v), false, false)[1]));
    v = op(v, val(__builtin_amdgcn_permlane16_swap(bits(v), bits(v), false, false)[1]));
    v = op(v, VO_ROW_SHL(8));
    v = op(v, VO_ROW_SHL(4));
    v = op(v, VO_ROW_SHL(2));
    v = op(v, VO_ROW_SHL(1));
#undef VO_ROW_SHL
    return val(__builtin_amdgcn_readlane(bits(v), 0));
}

// The sum of the 64 lanes' values by the pairwise tree of vo_spec.h's vo_tree_sum,
// p[l] = p[l] + p[l + off] for off = 32 .. 1, in every lane.  The value is the tree's p[0] bit for
// bit for either body: the 4-byte one computes lane 0's tree and broadcasts it; the 8-byte one is the
// xor butterfly, where each level adds the same two values in both partner lanes and IEEE addition
// commutes, so all lanes hold the same bits at every level and lane 0's are those of p[0].
template <typename T>
__device__ __forceinline__ T wave_sum_xor(T v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + (T)__shfl_xor(v, off);
    return v;
}
// N sums side by side, level by level, so that the N shuffles of a level are in flight together
template <int N, typename T>
__device__ __forceinline__ void wave_sum_xor(T* v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = v[q] + (T)__shfl_xor(v[q], off);
    }
}
// (wave_sum_xor by name: k_refine_pose's 28 sums, and the counts beside the double sums there and in
// k_msac)
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "int, uint32_t, float; int64_t, double");
    if constexpr (sizeof(T) == 4) return wave_tree<true>(v, [](T a, T b) { return a + b; });
    else return wave_sum_xor(v);
}

// maximum / minimum of the 64 lanes' values (float, uint32_t; order-free), in every lane
template <typename T>
__device__ __forceinline__ T wave_max(T v)
{
    if constexpr (std::is_same_v<T, float>) return wave_tree<false>(v, [](float a, float b) { return fmaxf(a, b); });
    else return wave_tree<false>(v, [](T a, T b) { return a > b ? a : b; });
}
template <typename T>
__device__ __forceinline__ T wave_min(T v)
{
    if constexpr (std::is_same_v<T, float>) return wave_tree<false>(v, [](float a, float b) { return fminf(a, b); });
    else return wave_tree<false>(v, [](T a, T b) { return a < b ? a : b; });
}

// The 64-lane shifts by one: lane l gets lane l - 1's value (wave_shift_up; lane 0 gets fill) or lane
// l + 1's (wave_shift_down; lane 63 gets fill).  4-byte values, one ds_bpermute each, no LDS storage.
template <typename T>
__device__ __forceinline__ T wave_shift_up(T v, T fill)
{
    static_assert(sizeof(T) == 4, "one register per lane");
    const int lane = threadIdx.x & 63;
    const T x = __builtin_bit_cast(T, __builtin_amdgcn_ds_bpermute(((lane - 1) & 63) << 2, __builtin_bit_cast(int, v)));
    return lane == 0 ? fill : x;
}
template <typename T>
__device__ __forceinline__ T wave_shift_down(T v, T fill)
{
    static_assert(sizeof(T) == 4, "one register per lane");
    const int lane = threadIdx.x & 63;
    const T x = __builtin_bit_cast(T, __builtin_amdgcn_ds_bpermute(((lane + 1) & 63) << 2, __builtin_bit_cast(int, v)));
    return lane == 63 ? fill : x;
}

// inclusive prefix sum over the lanes (int, uint32_t): lane l gets x[0] + .. + x[l], lane 63 the
// wave's total.  DPP row shifts within the rows of 16, then the row broadcasts.
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v)
{
    static_assert(std::is_integral_v<T> && sizeof(T) == 4, "int, uint32_t");
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);   // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);   // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);  // row_bcast:15 into rows 1, 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);  // row_bcast:31 into rows 2, 3
    return (T)x;
}

// the number of lanes below this one whose pred is set; *count = the wave's number of set lanes
__device__ __forceinline__ int wave_rank(bool pred, int* count)
{
    const unsigned long long m = __ballot(pred);
    *count = __popcll(m);
    return __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// Exclusive prefix sum of one value per thread over a block of NWAVES waves (up to 64), in thread
// order; *total = the block's sum, in every thread.  sh: NWAVES words of LDS, free again at return
// (the function ends with a barrier, so it may be called in a loop).
template <int NWAVES>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t* total)
{
    static_assert(NWAVES >= 1 && NWAVES <= 64, "the waves' totals are scanned by one wave's lanes");
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t x = wave_incl_scan(v);
    if (lane == 63) sh[wid] = x;
    __syncthreads();
    const int s = (int)wave_incl_scan(lane < NWAVES ? sh[lane] : 0u);      // every wave scans the totals itself
    const uint32_t before = wid ? (uint32_t)__builtin_amdgcn_readlane(s, wid - 1) : 0u;
    *total = (uint32_t)__builtin_amdgcn_readlane(s, NWAVES - 1);
    __syncthreads();
    return before + x - v;
}

// The sum of one value per thread over a block of NWAVES waves, in every thread: wave_sum, then the
// waves' totals through LDS, added in wave order.  sh: NWAVES words, read until the next barrier.
template <int NWAVES, typename T>
__device__ __forceinline__ T block_sum(T v, T* sh)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = sh[0];
#pragma unroll
    for (int w = 1; w < NWAVES; ++w) s += sh[w];
    return s;
}

// Block-wide exclusive scan of one value per thread (1024 threads).  The candidate compaction
// (k_seg_count, k_seg_scan, k_seg_emit, k_scan_cands) keeps these bodies instead of wave.h's
// block_excl_scan / block_sum: with those the four kernels were faster and the 256-frame step
// 0.6 - 1.7 % slower in three sessions out of three.  They stand here, beside the
// functions they are held equal to, so that tests/wave_probe can call them.  sh: 32 words
// (block_exscan_1024, free again at return) / 4 words (block_exscan_256, 256 threads, read until the
// caller's next barrier).
__device__ __forceinline__ uint32_t block_exscan_1024(uint32_t v, uint32_t* sh, uint32_t* total)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) sh[wid] = x;
    __syncthreads();
    if (wid == 0) {
        uint32_t s = lane < 16 ? sh[lane] : 0;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            uint32_t y = __shfl_up(s, o);
            if (lane >= o) s += y;
        }
        if (lane < 16) sh[16 + lane] = s;
    }
    __syncthreads();
    uint32_t before = wid ? sh[16 + wid - 1] : 0;
    *total = sh[16 + 15];
    __syncthreads();
    return before + x - v;
}

__device__ __forceinline__ uint32_t block_exscan_256(uint32_t v, uint32_t* sh)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) sh[wid] = x;
    __syncthreads();
    uint32_t before = 0;
    for (int q = 0; q < wid; ++q) before += sh[q];
    return before + x - v;
}

}  // namespace vo
