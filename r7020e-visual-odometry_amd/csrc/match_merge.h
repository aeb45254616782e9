// match_merge.h — the collectives of match.hip that are its own type: the two top-2 merges and the
// placement of a tile's accepted rows.  Device only; the contracts of wave.h hold (whole waves,
// converged, 1-D blocks).  They stand in a header so that tests/wave_probe can call them.
#pragma once
#include "wave.h"

namespace vo {

// (b,i,s) <- merge with (b2,i2,s2): lexicographic max on (value, -index), and the
// second largest value of the union multiset.  Associative & commutative.
__device__ __forceinline__ void top2c_merge(float& b, int& i, float& s, float b2, int i2, float s2)
{
    const float ns = fmaxf(fmaxf(s, s2), fminf(b, b2));
    if (b2 > b || (b2 == b && i2 < i)) { b = b2; i = i2; }
    s = ns;
}
// top2c_merge with the lane at xor distance off (whole wave, converged)
__device__ __forceinline__ void top2c_merge_lanes(float& b, int& i, float& s, int off)
{
    const float b2 = __shfl_xor(b, off), s2 = __shfl_xor(s, off);
    const int i2 = __shfl_xor(i, off);
    top2c_merge(b, i, s, b2, i2, s2);
}
// The f32 kernels rank by SSD and a lane may hold no column yet (idx < 0, best = inf): the wave's 64
// (best, idx, second) joined by lexicographic min on (value, index) over the lanes that hold one, and
// the second smallest value of the union multiset; the result in every lane (whole wave, converged)
__device__ __forceinline__ void top2s_merge_wave(float& best, int& bidx, float& second)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float b2 = __shfl_xor(best, off), s2 = __shfl_xor(second, off);
        const int i2 = __shfl_xor(bidx, off);
        const float ns = fminf(fminf(second, s2), fmaxf(best, b2));
        if (i2 >= 0 && (bidx < 0 || b2 < best || (b2 == best && i2 < bidx))) { best = b2; bidx = i2; }
        second = ns;
    }
}

// A tile's accepted rows in thread order after the `base` rows of the earlier tiles: this thread's
// position if it holds one (ok), and base moves past the tile.  Whole 256-thread block; wsum (4 words)
// is free again at return.
__device__ __forceinline__ uint32_t match_place(bool ok, uint32_t* wsum, uint32_t& base)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int cnt;
    uint32_t pos = base + (uint32_t)wave_rank(ok, &cnt);
    if (lane == 0) wsum[wid] = (uint32_t)cnt;
    __syncthreads();
    for (int w = 0; w < wid; ++w) pos += wsum[w];
    base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return pos;
}

}  // namespace vo
