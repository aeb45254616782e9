// match.hip — matchFeatures (VO.m:87,283,293,311,323) on gfx950.
//
// SIFT descriptors are u8-valued (0..255).  The SSD of unit-normalised rows
// (matchFeatures' Metric SSD on normalised features) is computed from the
// EXACT integer dot product:  ssd = 2 - 2 * ((float)dot * inv|a|) * inv|b|
// (DESIGN.md §3.3).  The dot products run on the i8 matrix cores:
// v_mfma_i32_32x32x32_i8 on (a - 128) x (b - 128), corrected by the row sums
//   dot(a,b) = dot(a',b') + 128 (sum a + sum b) - 2^21,
// so the result is exact and order-free; MFMA throughput is 8x the v_dot4
// VALU path.  The top-2 search is fused into the MFMA epilogue: the tile is computed
// transposed (F2 columns x F1 rows), so each lane keeps (best, idx, second) for ONE F1
// row over the F2 columns it holds, the two half-waves that share a row merge with a
// (value, index) total order, and the F2 chunks merge in k_match_finish (one workgroup
// per job), which also applies MatchThreshold / MaxRatio and writes the pairs in
// ascending F1 order.
#include "vo_internal.h"
#include "vo_geom.h"
#include "wave.h"
#include "match_merge.h"

namespace vo {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float vo_f2 __attribute__((ext_vector_type(2)));
typedef float vo_f4 __attribute__((ext_vector_type(4)));

// Ranking in the cosine domain.  The spec's SSD is sv = 2 - 2c with
// c = ((float)dot * inv|a|) * inv|b|; sv is a non-increasing function of c, so the
// k-th largest c maps to the k-th smallest sv, and for c >= 0.5 (sv <= 1, Sterbenz:
// 2 - 2c is exact) it is strictly decreasing.  Every accepted match has
// sv <= 0.04, so the argmax-c set equals the argmin-sv set there and the tie rule
// (lowest F2 index) picks the same column; the second-best SSD is recovered as
// 2 - 2 * (second-largest c).  Rows whose best sv > 1 may pick another index among
// sv ties but are rejected by the threshold either way.
// The merges themselves (top2c_merge, top2c_merge_lanes; top2s_merge_wave of the f32 kernels) are
// match_merge.h's.

// Pointers read from the job table are generic to the compiler, so loads through them became
// flat loads, which count in both vmcnt and lgkmcnt and can only be waited for with vmcnt(0) /
// lgkmcnt(0): every LDS wait of the tile loop also waited for the next tile's prefetch.  Every
// job pointer addresses global memory (device allocations), so its loads and stores go through the
// global address space.
template <class T>
__device__ __forceinline__ T gld(const T* p)
{
    return *(const __attribute__((address_space(1))) T*)p;
}
template <class T>
__device__ __forceinline__ void gst(T* p, T v)
{
    *(__attribute__((address_space(1))) T*)p = v;
}

__device__ __forceinline__ DescMeta gld_meta(const DescMeta* p)
{
    typedef int i2_t __attribute__((ext_vector_type(2)));
    const i2_t v = gld(reinterpret_cast<const i2_t*>(p));       // {sum, inv_norm bits}
    DescMeta m;
    m.sum = v.x;
    m.inv_norm = __int_as_float(v.y);
    return m;
}

__device__ __forceinline__ int job_rows(const int* p, int cap)
{
    int n = gld(p);
    return n < 0 ? 0 : (n > cap ? cap : n);
}

__device__ __forceinline__ v4i load_frag(const uint8_t* row, int off)
{
    v4i v = gld(reinterpret_cast<const v4i*>(row + off));
    v ^= (v4i){(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
    return v;
}

// One workgroup (4 waves) per (job, 128-row F1 block, CHUNK-column F2 chunk); wave w owns
// F1 rows [128 blk + 32 w, +32).  The F2 side is shared: each 32-column tile (4 KB of
// descriptors + metadata) is loaded once per workgroup, one 16-B load per thread, staged
// through a double-buffered LDS tile, and read by every wave as the MFMA A operand (the
// wave's F1 rows are the B operand, in registers): D = F2 tile x F1 rows, so lane l holds F1
// row l & 31 and 16 of the tile's columns.  Tile t+1 is written to LDS and tile t+2 is in
// flight from HBM/L2 while tile t runs its 4 MFMAs and epilogue.  Epilogue per accumulator
// element: dot = acc + 128 sa - 2^21 + 128 sb (one add3), c = ((float)dot * inv|a|) * inv|b|
// (packed muls, two columns at once); then one exact pre-test per tile -- the max of the
// lane's 16 values against its second best -- before the in-order top-2 update, which the wave
// skips when no lane passes.  (The untransposed tile -- D = F1 x F2, 16 rows' top-2 state per
// lane, 154 VGPRs, one wave vote per element -- measured 23 % slower isolated and cost the full
// path 3 %: its 3 waves per SIMD held register file the level blurs needed, r06_w.)
#define MP_ROWS 128
#define MP_LDS_ROW 144
#define VO_MP_MAX_JOBS 256        // jobs per launch (one per thread of the task-table prologue)
#ifndef VO_MP_BLOCKS
#define VO_MP_BLOCKS 5            // workgroups per CU the register budget of k_match_partial<1> is sized for (92 VGPRs)
#endif
#define MP_NBUF 2
#ifndef VO_RADIUS_PREREJECT
#define VO_RADIUS_PREREJECT 1     // k_match_radius: skip a tile whose box lies outside every row's circle (0: the A/B build of DESIGN.md 9n)
#endif
// NB: 32-row F1 sub-blocks per wave (MP_ROWS * NB rows per workgroup); NB = 2 runs two
// independent MFMA chains per tile on the same F2 fragments (half the LDS reads per MFMA)
// SWAP: the job's row side is the spec's F2 and its column side the spec's F1 (the backward pass
// of Unique): the two multiplies of c keep the spec's operand order, (dot * inv|F1|) * inv|F2|,
// so the backward values are the forward pass's bit for bit
template <int NB, bool SWAP = false>
__global__ __launch_bounds__(256, NB == 1 ? VO_MP_BLOCKS : 2) void k_match_partial(const MatchJob* __restrict__ jobs, int n_jobs,
                                                       MatchTop2* __restrict__ partial, int row_cap, int n_chunks_cap)
{
    constexpr int ROWS = MP_ROWS * NB;
    // F2 tile rows padded to 144 B (36 dwords): the 32 lanes of a half read 16 B at row l31,
    // so a 128-B stride would put them all on the same banks
    __shared__ __attribute__((aligned(16))) uint8_t bt[MP_NBUF][32 * MP_LDS_ROW];
    __shared__ __attribute__((aligned(16))) int bck[MP_NBUF][32];
    __shared__ __attribute__((aligned(16))) float binb[MP_NBUF][32];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, l31 = lane & 31;
    const int lr = tid >> 3, lseg = tid & 7;              // loader: row lr of the tile, bytes [16 lseg, +16)
    // task table: job j owns tasks [tstart[j], tstart[j+1]); job sizes are read on device
    // (counts of earlier kernels), one thread per job, then a block prefix sum
    __shared__ int tstart[VO_MP_MAX_JOBS + 1], jn1[VO_MP_MAX_JOBS], jnch[VO_MP_MAX_JOBS];
    __shared__ uint32_t wsum[4];
    {
        int my = 0;
        if (tid < n_jobs) {
            const int n1 = job_rows(jobs[tid].n1, row_cap), n2 = job_rows(jobs[tid].n2, row_cap);
            const int nch = (n2 + VO_MATCH_CHUNK - 1) / VO_MATCH_CHUNK;
            jn1[tid] = n1; jnch[tid] = nch;
            my = ((n1 + ROWS - 1) / ROWS) * nch;
        }
        uint32_t all;
        const uint32_t first = block_excl_scan<4>((uint32_t)my, wsum, &all);
        if (tid < n_jobs) tstart[tid] = (int)first;
        if (tid == 255) tstart[min(n_jobs, VO_MP_MAX_JOBS)] = (int)all;
        __syncthreads();
    }
    const int total = tstart[n_jobs];
    // (an XCD-contiguous task order -- one job's row blocks, which read the same F2 tiles, on one
    // XCD's L2 -- measured slower: 0.825 against 0.667 ms isolated, profiles/r06_r_ab_match_task.txt)
    for (int t = blockIdx.x; t < total; t += gridDim.x) {       // workgroup-uniform
        int jb = 0;
        // last job whose first task <= t (tstart is nondecreasing; empty jobs repeat a value): a
        // binary search of the task table, 8 dependent LDS reads where a linear scan took up to 255
        // (k_match_partial 0.623 against 0.667 / 0.679 ms isolated per 256-frame step,
        // profiles/r06_r_ab_match_task.txt)
        for (int step = VO_MP_MAX_JOBS / 2; step >= 1; step >>= 1)
            if (jb + step < n_jobs && tstart[jb + step] <= t) jb += step;
        const int n1 = jn1[jb], nch = jnch[jb];
        const int n2 = job_rows(jobs[jb].n2, row_cap);
        const long rel = t - tstart[jb];
        const MatchJob J = jobs[jb];
        const int blk = (int)(rel / nch), chunk = (int)(rel - (long)blk * nch);
        const int i0 = blk * ROWS + 32 * NB * wave, j0 = chunk * VO_MATCH_CHUNK;
        const int j1 = min(j0 + VO_MATCH_CHUNK, n2);
        // F1 fragments (the MFMA B operand) of sub-block sb: row i0 + 32 sb + l31, bytes
        // [32kk + 16h, +16); the lane's row's sum term and inverse norm; its running top-2 over
        // the F2 columns this lane sees (both halves hold the row)
        v4i a[NB][4];
        int rk1[NB];
        float ina1[NB], best1[NB], second1[NB];
        int bidx1[NB];
#pragma unroll
        for (int sb = 0; sb < NB; ++sb) {
            const int ia = i0 + 32 * sb + l31;
            rk1[sb] = -2097152;
            ina1[sb] = 0.0f;
            if (ia < n1) {
                const int ra = J.idx1 ? gld(J.idx1 + ia) : ia;
                const uint8_t* row = J.d1 + (size_t)ra * VO_DESC_LEN;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) a[sb][kk] = load_frag(row, 32 * kk + 16 * h);
                const DescMeta m = gld_meta(J.m1 + ra);
                rk1[sb] = 128 * m.sum - 2097152;
                ina1[sb] = m.inv_norm;
            } else {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) a[sb][kk] = (v4i){0, 0, 0, 0};
            }
            best1[sb] = -INFINITY; second1[sb] = -INFINITY; bidx1[sb] = -1;
        }
        // loader: column jt + lr (clamped into the chunk; the epilogue masks columns >= j1)
        v4i gv;
        DescMeta gm;
        auto gload = [&](int jt) {
            const int jc = min(jt + lr, j1 - 1);
            const int rb = J.idx2 ? gld(J.idx2 + jc) : jc;
            gv = gld(reinterpret_cast<const v4i*>(J.d2 + (size_t)rb * VO_DESC_LEN + 16 * lseg));
            if (lseg == 0) gm = gld_meta(J.m2 + rb);
        };
        auto lstore = [&](int buf) {                       // stored as b - 128 (the MFMA operand)
            *reinterpret_cast<v4i*>(&bt[buf][lr * MP_LDS_ROW + 16 * lseg]) =
                gv ^ (v4i){(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
            if (lseg == 0) { bck[buf][lr] = 128 * gm.sum; binb[buf][lr] = gm.inv_norm; }
        };
        // the tile's MFMAs: D = F2 tile (A operand, from LDS) x F1 rows (B operand, registers):
        // lane l holds F1 row i0 + 32 sb + l31 and F2 columns jt + (reg & 3) + 8 (reg >> 2) + 4 h,
        // reg = 0..15 -- ascending in reg, so the lane meets its columns in ascending order
        auto tile_mfma = [&](int bi, v16i (&accv)[NB]) {
            v4i b[4];
            const uint8_t* brow = &bt[bi][l31 * MP_LDS_ROW + 16 * h];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) b[kk] = *reinterpret_cast<const v4i*>(brow + 32 * kk);
#pragma unroll
            for (int sb = 0; sb < NB; ++sb) accv[sb] = (v16i){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int sb = 0; sb < NB; ++sb) accv[sb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(b[kk], a[sb][kk], accv[sb], 0, 0, 0);
        };
        auto tile_epilogue = [&](int bi, int jt, const v16i (&accv)[NB]) {
#pragma unroll
            for (int sb = 0; sb < NB; ++sb) {
                float cv[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    // the column metadata of regs 4q .. 4q+3: tile columns 8q + 4h .. +3 (one
                    // broadcast 16-B read each)
                    const v4i ck4 = *reinterpret_cast<const v4i*>(&bck[bi][8 * q + 4 * h]);
                    const vo_f4 ib4 = *reinterpret_cast<const vo_f4*>(&binb[bi][8 * q + 4 * h]);
#pragma unroll
                    for (int i = 0; i < 4; i += 2) {
                        // c = ((float)dot * inv|a|) * inv|b|, two columns at once as packed f32 muls
                        const vo_f2 fp = vo_f2{(float)(accv[sb][4 * q + i] + rk1[sb] + ck4[i]),
                                               (float)(accv[sb][4 * q + i + 1] + rk1[sb] + ck4[i + 1])};
                        const vo_f2 cp = SWAP ? (fp * vo_f2{ib4[i], ib4[i + 1]}) * vo_f2{ina1[sb], ina1[sb]}
                                              : (fp * vo_f2{ina1[sb], ina1[sb]}) * vo_f2{ib4[i], ib4[i + 1]};
                        cv[4 * q + i] = cp.x;
                        cv[4 * q + i + 1] = cp.y;
                    }
                }
                if (jt + 32 > j1) {                        // wave-uniform: the ragged last tile
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg)
                        cv[reg] = jt + (reg & 3) + 8 * (reg >> 2) + 4 * h < j1 ? cv[reg] : -INFINITY;
                }
                // exact pre-test: a tile whose 16 values are all <= the lane's second best changes
                // nothing (the update below leaves best / second / index as they are for c <= second).
                // (An integer pre-test before the float conversion -- the tile's dots against
                // floor(second / inv|a| / max inv|b| (1 - 2^-16)) -- was bit-exact but 27 % slower:
                // the bound with the tile's largest inv|b| rarely clears a whole wave, so it only
                // added work, profiles/r06_zd_ab_match_ibound.txt)
                float m = fmaxf(fmaxf(fmaxf(cv[0], cv[1]), fmaxf(cv[2], cv[3])), fmaxf(fmaxf(cv[4], cv[5]), fmaxf(cv[6], cv[7])));
                m = fmaxf(m, fmaxf(fmaxf(fmaxf(cv[8], cv[9]), fmaxf(cv[10], cv[11])), fmaxf(fmaxf(cv[12], cv[13]), fmaxf(cv[14], cv[15]))));
                if (__builtin_amdgcn_ballot_w64(m > second1[sb])) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const float c = cv[reg];
                        const bool g1 = c > best1[sb], g2 = c > second1[sb];
                        second1[sb] = g1 ? best1[sb] : (g2 ? c : second1[sb]);
                        best1[sb] = g1 ? c : best1[sb];
                        bidx1[sb] = g1 ? jt + (reg & 3) + 8 * (reg >> 2) + 4 * h : bidx1[sb];
                    }
                }
            }
        };
        // (a three-tile pipeline -- tile t+1's MFMAs issued before tile t's epilogue, 116 VGPRs at 4
        // waves per SIMD -- measured slower: 0.453 against 0.420 ms isolated, the 1080p block 0.121
        // against 0.129 of i8 peak, profiles/r06_za_ab_match_pipe_grid.txt)
        gload(j0);
        __syncthreads();                                   // previous task's readers are done with bt
        lstore(0);
        if (j0 + 32 < j1) gload(j0 + 32);
        int buf = 0;
        for (int jt = j0; jt < j1; jt += 32, buf ^= 1) {
            __syncthreads();                               // tile jt visible; tile jt-32's buffer free
            if (jt + 32 < j1) {
                lstore(buf ^ 1);                           // tile jt+32 (loaded one iteration ago)
                if (jt + 64 < j1) gload(jt + 64);
            }
            v16i accv[NB];
            tile_mfma(buf, accv);
            tile_epilogue(buf, jt, accv);
        }
#pragma unroll
        for (int sb = 0; sb < NB; ++sb) {
            top2c_merge_lanes(best1[sb], bidx1[sb], second1[sb], 32);
            const int row = i0 + 32 * sb + l31;
            if (h == 0 && row < n1) {
                MatchTop2 mt;
                mt.best = best1[sb]; mt.idx = bidx1[sb]; mt.second = second1[sb]; mt.pad = 0;
                partial[((size_t)jb * n_chunks_cap + chunk) * row_cap + row] = mt;
            }
        }
    }
}

// One 256-thread workgroup per job: the merge of the F2 chunks, the compaction of the accepted
// rows (and a tracking step's index composition) in one launch.  Rows go in tiles of 256 in
// ascending F1 order (coalesced partial reads): thread t merges row 256 k + t over the F2 chunks,
// back to SSD, and applies MatchThreshold / MaxRatio; the tile's accepted rows are placed by a
// block prefix sum after the running count, so the pairs come out in ascending F1 order.  With
// `compose` (a tracking step of find_remaining_points), the workgroup then applies that step's
// index composition to its frame's lists (VO.m:287-333) -- so a tracking step is two launches
// (partial, finish); as separate merge, compact and compose kernels it was four.  The placement is
// match_merge.h's match_place.
__global__ __launch_bounds__(256) void k_match_finish(const MatchJob* __restrict__ jobs, const MatchTop2* __restrict__ partial,
                                                      int row_cap, int n_chunks_cap, float T, float max_ratio,
                                                      MatchCompose cp, int with_compose)
{
    __shared__ uint32_t wsum[4];
    const int jb = blockIdx.x, tid = threadIdx.x;
    const MatchJob J = jobs[jb];
    const int n1 = job_rows(J.n1, row_cap), n2 = job_rows(J.n2, row_cap);
    const int nch = (n2 + VO_MATCH_CHUNK - 1) / VO_MATCH_CHUNK;
    const MatchTop2* P = partial + (size_t)jb * n_chunks_cap * row_cap;
    uint32_t base = 0;
    for (int r0 = 0; r0 < n1; r0 += 256) {                       // block-uniform
        const int r = r0 + tid;
        int acc = -1;
        if (r < n1) {
            float b = -INFINITY, s = -INFINITY;
            int i = -1;
            for (int c = 0; c < nch; ++c) {
                const MatchTop2 m = P[(size_t)c * row_cap + r];
                top2c_merge(b, i, s, m.best, m.idx, m.second);
            }
            const float bs = 2.0f - 2.0f * b, ss = 2.0f - 2.0f * s;      // SSD of best / second best
            acc = (i >= 0 && bs <= T && (bs / ss) <= max_ratio) ? i : -1;
        }
        const uint32_t pos = match_place(acc >= 0, wsum, base);
        if (acc >= 0 && pos < (uint32_t)J.cap) { gst(J.out_i + pos, r); gst(J.out_j + pos, acc); }
    }
    const int n_out = (int)(base < (uint32_t)J.cap ? base : (uint32_t)J.cap);
    if (tid == 0) gst(J.out_n, n_out);
    if (!with_compose) return;
    __syncthreads();                                              // the pairs are visible to the block
    // the index composition of tracking step cp.step for frame f = jb
    const int f = cp.f0 + jb, K = cp.kp_cap, M = cp.M, st = cp.step;
    int* L = cp.lists + (size_t)f * TL_COUNT * K;
    const int pp = f ? f - 1 : M;
    const int n = min(n_out, K);
    for (int k = tid; k < n; k += 256) {
        const int i = gld(J.out_i + k), j = gld(J.out_j + k);
        if (st == 0) {
            L[TL_OL1 * K + k] = cp.pair_i[(size_t)pp * K + j];
            L[TL_OR1 * K + k] = cp.pair_j[(size_t)pp * K + j];
            L[TL_CL * K + k] = i;
        } else if (st == 1) {
            L[TL_OL2 * K + k] = L[TL_OL1 * K + j];
            L[TL_OR2 * K + k] = L[TL_OR1 * K + j];
            L[TL_CR * K + k] = i;
        } else if (st == 2) {
            L[TL_CL2 * K + k] = L[TL_CL * K + i];
            L[TL_CR2 * K + k] = L[TL_CR * K + j];
        } else {
            L[TL_OLF * K + k] = L[TL_OL2 * K + j];
            L[TL_ORF * K + k] = L[TL_OR2 * K + j];
            L[TL_CLF * K + k] = L[TL_CL2 * K + i];
            L[TL_CRF * K + k] = L[TL_CR2 * K + i];
        }
    }
    if (tid == 0) cp.list_n[4 * f + st] = n;
}

// k_match_finish for vo_match_ex: the same merge, MatchThreshold / MaxRatio and ascending-F1
// placement, plus matchMetric (the accepted pair's SSD, bs) and, with `unique`, the toolbox's
// findUniqueIndices rule: an accepted pair (r, j) is kept iff r is the best F1 row of column j
// over ALL F1 rows, lowest row on ties.  `back` holds the backward pass's partials (F2 rows x F1
// chunks, k_match_partial<1, true>): their values are the forward c(i, j) bit for bit, and an
// accepted pair has c >= 0.5 (MatchThreshold <= 25), where argmax c (lowest index) is argmin SSD
// (lowest index).  With unique == 0 the pairs are exactly k_match_finish's.
__global__ __launch_bounds__(256) void k_match_finish_unique(const MatchJob* __restrict__ jobs, const MatchTop2* __restrict__ partial,
                                                             const MatchTop2* __restrict__ back, int row_cap, int n_chunks_cap,
                                                             float T, float max_ratio, int unique, float* __restrict__ metric)
{
    __shared__ uint32_t wsum[4];
    const int jb = blockIdx.x, tid = threadIdx.x;
    const MatchJob J = jobs[jb];
    const int n1 = job_rows(J.n1, row_cap), n2 = job_rows(J.n2, row_cap);
    const int nch = (n2 + VO_MATCH_CHUNK - 1) / VO_MATCH_CHUNK, nchb = (n1 + VO_MATCH_CHUNK - 1) / VO_MATCH_CHUNK;
    const MatchTop2* P = partial + (size_t)jb * n_chunks_cap * row_cap;
    const MatchTop2* PB = back + (size_t)jb * n_chunks_cap * row_cap;
    float* M = metric + (size_t)jb * row_cap;
    uint32_t base = 0;
    for (int r0 = 0; r0 < n1; r0 += 256) {                       // block-uniform
        const int r = r0 + tid;
        int acc = -1;
        float bs = 0.0f;
        if (r < n1) {
            float b = -INFINITY, s = -INFINITY;
            int i = -1;
            for (int c = 0; c < nch; ++c) {
                const MatchTop2 m = P[(size_t)c * row_cap + r];
                top2c_merge(b, i, s, m.best, m.idx, m.second);
            }
            bs = 2.0f - 2.0f * b;
            const float ss = 2.0f - 2.0f * s;                    // SSD of best / second best
            acc = (i >= 0 && bs <= T && (bs / ss) <= max_ratio) ? i : -1;
            if (unique && acc >= 0) {
                float bb = -INFINITY, sb = -INFINITY;
                int bi = -1;
                for (int c = 0; c < nchb; ++c) {
                    const MatchTop2 m = PB[(size_t)c * row_cap + acc];
                    top2c_merge(bb, bi, sb, m.best, m.idx, m.second);
                }
                if (bi != r) acc = -1;
            }
        }
        const uint32_t pos = match_place(acc >= 0, wsum, base);
        if (acc >= 0 && pos < (uint32_t)J.cap) { gst(J.out_i + pos, r); gst(J.out_j + pos, acc); gst(M + pos, bs); }
    }
    if (tid == 0) gst(J.out_n, (int)(base < (uint32_t)J.cap ? base : (uint32_t)J.cap));
}

// Descriptor metadata for externally supplied descriptors (vo_match on host data).
__global__ void k_desc_meta(const uint8_t* __restrict__ desc, DescMeta* __restrict__ meta, int n)
{
    const int lane = threadIdx.x & 63;
    for (long t = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < n; t += (long)gridDim.x * (blockDim.x >> 6)) {
        const uint8_t* d = desc + t * VO_DESC_LEN;
        int v0 = d[lane], v1 = d[lane + 64];
        const int sum = wave_sum(v0 + v1), sq = wave_sum(v0 * v0 + v1 * v1);
        if (lane == 0) { DescMeta m; m.sum = sum; m.inv_norm = sq > 0 ? 1.0f / sqrtf((float)sq) : 0.0f; meta[t] = m; }
    }
}

hipError_t match_alloc(DevPool& pool, MatchBuffers& b, int max_jobs, int row_cap)
{
    b.max_jobs = max_jobs;
    b.row_cap = row_cap;
    b.n_chunks = (row_cap + VO_MATCH_CHUNK - 1) / VO_MATCH_CHUNK;
    return (hipError_t)pool.alloc(b.partial, (size_t)max_jobs * b.n_chunks * row_cap);
}

hipError_t match_ex_alloc(DevPool& pool, MatchExBuffers& x, const MatchBuffers& b, const MatchJob& job_back)
{
    const size_t R = b.row_cap;
    hipError_t e = (hipError_t)pool.group({DevPool::req(x.job_back, 1), DevPool::req(x.partial_back, b.n_chunks * R),
                                           DevPool::req(x.metric, R), DevPool::req(x.back, R)});
    if (e != hipSuccess) return e;
    e = hipMemcpy(x.job_back, &job_back, sizeof(MatchJob), hipMemcpyHostToDevice);
    if (e != hipSuccess) { pool.release(x.job_back); pool.release(x.partial_back); pool.release(x.metric); pool.release(x.back); }
    return e;
}

MatchBuffers match_view(const MatchBuffers& b, int k0)
{
    MatchBuffers v = b;
    v.partial = b.partial + (size_t)k0 * b.n_chunks * b.row_cap;
    v.max_jobs = b.max_jobs - k0;
    return v;
}

void match_launch(const MatchBuffers& b, const MatchJob* d_jobs, int n_jobs, const vo_match_params& p, hipStream_t s,
                  const MatchCompose* compose)
{
    if (n_jobs <= 0) return;
    if (n_jobs > VO_MP_MAX_JOBS) {                       // the task table holds VO_MP_MAX_JOBS jobs
        MatchCompose rest;
        if (compose) {                                   // frames VO_MP_MAX_JOBS.. of a tracking step
            rest = *compose;
            rest.f0 += VO_MP_MAX_JOBS;
        }
        match_launch(b, d_jobs, VO_MP_MAX_JOBS, p, s, compose);
        match_launch(match_view(b, VO_MP_MAX_JOBS), d_jobs + VO_MP_MAX_JOBS, n_jobs - VO_MP_MAX_JOBS, p, s,
                     compose ? &rest : nullptr);
        return;
    }
#ifndef VO_TRACK_GRID
#define VO_TRACK_GRID 256         // k_match_partial workgroups for the tracking steps (stereo: 2048); 256 measured +1 % on the
                                  // full path over 2048 (fewer resident beside the SIFT streams), 64 / 128 / 512 / 8192 not
                                  // (profiles/r06_lm_ab_track_grid.txt)
#endif
#ifndef VO_STEREO_GRID
#define VO_STEREO_GRID 2048
#endif
    // (two F1 sub-blocks per wave for the stereo matches, k_match_partial<2> at 165 VGPRs: configs[1]
    // -1 %, the 1080p block 0.123 against 0.128 of i8 peak, profiles/r06_y_ab_match_nb2_chunk.txt)
    VO_LAUNCH_NAMED("k_match_partial", k_match_partial<1>, dim3(compose ? VO_TRACK_GRID : VO_STEREO_GRID), dim3(256), 0, s,
                    d_jobs, n_jobs, b.partial, b.row_cap, b.n_chunks);
    MatchCompose cp{};
    if (compose) cp = *compose;
    VO_LAUNCH(k_match_finish, dim3(n_jobs), dim3(256), 0, s, d_jobs, (const MatchTop2*)b.partial, b.row_cap, b.n_chunks,
              p.match_threshold * 0.04f, p.max_ratio, cp, compose ? 1 : 0);
}

void match_launch(const MatchBuffers& b, const MatchJob* d_jobs, int n_jobs, const vo_match_params& p, hipStream_t s)
{
    match_launch(b, d_jobs, n_jobs, p, s, nullptr);
}

// vo_match_ex: one job with explicit thresholds, matchMetric and (optionally) Unique.  The
// forward partials go to b's slot 0 as in match_launch; with `unique` the backward job (the same
// two descriptor sets with the sides exchanged) runs the SWAP instantiation into x.partial_back.
void match_launch_ex(const MatchBuffers& b, const MatchJob* d_job, const MatchExBuffers& x, const vo_match_params& p, int unique,
                     hipStream_t s)
{
    VO_LAUNCH_NAMED("k_match_partial", k_match_partial<1>, dim3(VO_STEREO_GRID), dim3(256), 0, s, d_job, 1, b.partial, b.row_cap,
                    b.n_chunks);
    if (unique)
        VO_LAUNCH_NAMED("k_match_partial_back", (k_match_partial<1, true>), dim3(VO_STEREO_GRID), dim3(256), 0, s,
                        (const MatchJob*)x.job_back, 1, x.partial_back, b.row_cap, b.n_chunks);
    VO_LAUNCH(k_match_finish_unique, dim3(1), dim3(256), 0, s, d_job, (const MatchTop2*)b.partial,
              (const MatchTop2*)x.partial_back, b.row_cap, b.n_chunks, p.match_threshold * 0.04f, p.max_ratio, unique, x.metric);
}

// ---------------------------------------------------------------------------
// matchFeaturesInRadius (vo_match_radius): matchFeatures whose candidates of F1 row i are the F2
// columns j with vo_radius_gate(x2_j, y2_j, cx_i, cy_i, r_i * r_i) ("In radius").
// ---------------------------------------------------------------------------
// One wave per aligned 32-row tile of either side (blocks [0, tiles1): F1, the rest: F2): lane l < 32
// writes row 32 tile + l's geometry -- F1: {cx, cy, r2 = r * r, 0}, F2: {x, y, 0, 0} -- and the
// half-wave reduces the tile's bounding box and, on the F1 side, its largest r2.  P holds the
// points as the caller does: row-major [n][2], or col_major: point (i, k) at P[i + k * n].
__global__ __launch_bounds__(64) void k_radius_meta(const float* __restrict__ centers, const float* __restrict__ radius, int n_radius,
                                                    int n1, const float* __restrict__ pts2, int n2, int col_major,
                                                    vo_geo4* __restrict__ geo1, vo_geo4* __restrict__ box1,
                                                    vo_geo4* __restrict__ geo2, vo_geo4* __restrict__ box2)
{
    const int tiles1 = (n1 + 31) >> 5, lane = threadIdx.x;
    const bool first = (int)blockIdx.x < tiles1;
    const int tile = first ? blockIdx.x : blockIdx.x - tiles1, n = first ? n1 : n2;
    const float* P = first ? centers : pts2;
    const int i = 32 * tile + lane;
    float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY, rmax = 0.0f;
    if (lane < 32 && i < n) {
        const float x = col_major ? P[i] : P[2 * (size_t)i], y = col_major ? P[(size_t)n + i] : P[2 * (size_t)i + 1];
        float r2 = 0.0f;
        if (first) { const float r = radius[n_radius == 1 ? 0 : i]; r2 = r * r; }
        (first ? geo1 : geo2)[i] = vo_geo4{x, y, r2, 0.0f};
        xmin = xmax = x; ymin = ymax = y; rmax = r2;
    }
    // lanes 32 .. 63 hold the identities, so the wave's extrema are the half-wave's
    xmin = wave_min(xmin); xmax = wave_max(xmax); ymin = wave_min(ymin); ymax = wave_max(ymax); rmax = wave_max(rmax);
    if (lane == 0) {
        vo_geo4* box = (first ? box1 : box2) + 2 * (size_t)tile;
        box[0] = vo_geo4{xmin, xmax, ymin, ymax};
        box[1] = vo_geo4{rmax, 0.0f, 0.0f, 0.0f};
    }
}

// One side of an in-radius pass: n descriptor rows, their metadata, geometry and tile boxes
struct RadiusSide {
    const uint8_t* d; const DescMeta* m; const vo_geo4* geo; const vo_geo4* box;
    int n, pad;
};

// k_match_partial<1, SWAP>'s tile scheme for a single job whose sizes the host knows: the same MFMA
// on (a - 128) x (b - 128) with the row-sum correction, the transposed tile (lane l holds row
// l & 31 of side R and 16 of the tile's columns of side Cs), the double-buffered column tile in LDS
// and the same MatchTop2 partials.  The tile's LDS rows also carry the columns' geometry and the
// tile's box.  !SWAP: R = F1 (centre and r2 per row), Cs = F2 (a point per column); SWAP (the
// backward pass of Unique): R = F2, Cs = F1.
// The gate: in the epilogue the lane sets cv[reg] = -INF for the columns outside the circle,
// evaluating vo_radius_gate on the spec's operands (the column's / row's point, the row's / column's
// centre and r2) in either pass, so the two passes agree bit for bit on who is a candidate.  The
// pre-test and the top-2 update are k_match_partial's: a row without a candidate ends with idx -1,
// one with a single candidate with second = -INF, which k_match_finish_unique turns into "no pair"
// and "ratio 0".
// Tile pre-reject: the wave skips the tile's MFMAs and epilogue when no live lane's
// vo_radius_box_lb against the tile's box is <= r2 (its own; SWAP: the tile's largest).  The bound
// is <= vo_radius_d2 of every column of the tile in float32 (the argument is vo_spec.h's), so a
// skipped tile holds no candidate of any of the wave's rows; the per-element gate is exact without
// it.  The loads, LDS stores and barriers stay unconditional.
template <bool SWAP>
__global__ __launch_bounds__(256, 4) void k_match_radius(RadiusSide R, RadiusSide Cs, MatchTop2* __restrict__ partial, int row_cap)
{
    __shared__ __attribute__((aligned(16))) uint8_t bt[MP_NBUF][32 * MP_LDS_ROW];
    __shared__ __attribute__((aligned(16))) int bck[MP_NBUF][32];
    __shared__ __attribute__((aligned(16))) float binb[MP_NBUF][32];
    __shared__ __attribute__((aligned(16))) float bgx[MP_NBUF][32], bgy[MP_NBUF][32], bgr[MP_NBUF][32];
    __shared__ __attribute__((aligned(16))) float bbox[MP_NBUF][8];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, l31 = lane & 31;
    const int lr = tid >> 3, lseg = tid & 7;              // loader: row lr of the tile, bytes [16 lseg, +16)
    const int n1 = R.n, n2 = Cs.n;                        // rows and columns of this pass
    const int nch = (n2 + VO_MATCH_CHUNK - 1) / VO_MATCH_CHUNK;
    const int total = ((n1 + MP_ROWS - 1) / MP_ROWS) * nch;
    for (int t = blockIdx.x; t < total; t += gridDim.x) {       // workgroup-uniform
        const int blk = t / nch, chunk = t - blk * nch;
        const int i0 = blk * MP_ROWS + 32 * wave, j0 = chunk * VO_MATCH_CHUNK;
        const int j1 = min(j0 + VO_MATCH_CHUNK, n2);
        const int ia = i0 + l31;
        const bool live = ia < n1;
        v4i a[4];
        int rk1 = -2097152;
        float ina1 = 0.0f;
        vo_geo4 rg = vo_geo4{0.0f, 0.0f, -1.0f, 0.0f};          // a dead lane's r2 admits nothing
        if (live) {
            const uint8_t* row = R.d + (size_t)ia * VO_DESC_LEN;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) a[kk] = load_frag(row, 32 * kk + 16 * h);
            const DescMeta m = gld_meta(R.m + ia);
            rk1 = 128 * m.sum - 2097152;
            ina1 = m.inv_norm;
            rg = gld(R.geo + ia);
        } else {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) a[kk] = (v4i){0, 0, 0, 0};
        }
        float best1 = -INFINITY, second1 = -INFINITY;
        int bidx1 = -1;
        // loader: column jt + lr (clamped into the chunk; the epilogue masks columns >= j1); thread
        // lseg 0 of a row brings its metadata, lseg 1 its geometry, and two threads the tile's box
        v4i gv;
        DescMeta gm;
        vo_geo4 gg = vo_geo4{0.0f, 0.0f, 0.0f, 0.0f}, gb = vo_geo4{0.0f, 0.0f, 0.0f, 0.0f};
        auto gload = [&](int jt) {
            const int jc = min(jt + lr, j1 - 1);
            gv = gld(reinterpret_cast<const v4i*>(Cs.d + (size_t)jc * VO_DESC_LEN + 16 * lseg));
            if (lseg == 0) gm = gld_meta(Cs.m + jc);
            if (lseg == 1) gg = gld(Cs.geo + jc);
            if (lseg == 2 && lr < 2) gb = gld(Cs.box + 2 * (size_t)(jt >> 5) + lr);
        };
        auto lstore = [&](int buf) {                       // stored as b - 128 (the MFMA operand)
            *reinterpret_cast<v4i*>(&bt[buf][lr * MP_LDS_ROW + 16 * lseg]) =
                gv ^ (v4i){(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
            if (lseg == 0) { bck[buf][lr] = 128 * gm.sum; binb[buf][lr] = gm.inv_norm; }
            if (lseg == 1) { bgx[buf][lr] = gg.x; bgy[buf][lr] = gg.y; bgr[buf][lr] = gg.z; }
            if (lseg == 2 && lr < 2) *reinterpret_cast<vo_geo4*>(&bbox[buf][4 * lr]) = gb;
        };
        auto tile = [&](int bi, int jt) {
            // D = column tile (A operand, from LDS) x rows (B operand, registers): lane l holds row
            // i0 + l31 and columns jt + (reg & 3) + 8 (reg >> 2) + 4 h, ascending in reg
            v4i b[4];
            const uint8_t* brow = &bt[bi][l31 * MP_LDS_ROW + 16 * h];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) b[kk] = *reinterpret_cast<const v4i*>(brow + 32 * kk);
            v16i acc = (v16i){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(b[kk], a[kk], acc, 0, 0, 0);
            float cv[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v4i ck4 = *reinterpret_cast<const v4i*>(&bck[bi][8 * q + 4 * h]);
                const vo_f4 ib4 = *reinterpret_cast<const vo_f4*>(&binb[bi][8 * q + 4 * h]);
                const vo_f4 gx4 = *reinterpret_cast<const vo_f4*>(&bgx[bi][8 * q + 4 * h]);
                const vo_f4 gy4 = *reinterpret_cast<const vo_f4*>(&bgy[bi][8 * q + 4 * h]);
                const vo_f4 gr4 = *reinterpret_cast<const vo_f4*>(&bgr[bi][8 * q + 4 * h]);
#pragma unroll
                for (int i = 0; i < 4; i += 2) {
                    // c = ((float)dot * inv|F1|) * inv|F2| in the spec's operand order, as k_match_partial
                    const vo_f2 fp = vo_f2{(float)(acc[4 * q + i] + rk1 + ck4[i]), (float)(acc[4 * q + i + 1] + rk1 + ck4[i + 1])};
                    const vo_f2 cp = SWAP ? (fp * vo_f2{ib4[i], ib4[i + 1]}) * vo_f2{ina1, ina1}
                                          : (fp * vo_f2{ina1, ina1}) * vo_f2{ib4[i], ib4[i + 1]};
                    cv[4 * q + i] = cp.x;
                    cv[4 * q + i + 1] = cp.y;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    // the gate, on the spec's operands in either pass: (F2 point, F1 centre, F1 r2)
                    const bool in = SWAP ? vo_radius_gate(rg.x, rg.y, gx4[i], gy4[i], gr4[i])
                                         : vo_radius_gate(gx4[i], gy4[i], rg.x, rg.y, rg.z);
                    cv[4 * q + i] = in ? cv[4 * q + i] : -INFINITY;
                }
            }
            if (jt + 32 > j1) {                            // wave-uniform: the ragged last tile
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    cv[reg] = jt + (reg & 3) + 8 * (reg >> 2) + 4 * h < j1 ? cv[reg] : -INFINITY;
            }
            // k_match_partial's exact pre-test and in-order top-2 update
            float m = fmaxf(fmaxf(fmaxf(cv[0], cv[1]), fmaxf(cv[2], cv[3])), fmaxf(fmaxf(cv[4], cv[5]), fmaxf(cv[6], cv[7])));
            m = fmaxf(m, fmaxf(fmaxf(fmaxf(cv[8], cv[9]), fmaxf(cv[10], cv[11])), fmaxf(fmaxf(cv[12], cv[13]), fmaxf(cv[14], cv[15]))));
            if (__builtin_amdgcn_ballot_w64(m > second1)) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const float c = cv[reg];
                    const bool g1 = c > best1, g2 = c > second1;
                    second1 = g1 ? best1 : (g2 ? c : second1);
                    best1 = g1 ? c : best1;
                    bidx1 = g1 ? jt + (reg & 3) + 8 * (reg >> 2) + 4 * h : bidx1;
                }
            }
        };
        gload(j0);
        __syncthreads();                                   // previous task's readers are done with the LDS tile
        lstore(0);
        if (j0 + 32 < j1) gload(j0 + 32);
        int buf = 0;
        for (int jt = j0; jt < j1; jt += 32, buf ^= 1) {
            __syncthreads();                               // tile jt visible; tile jt-32's buffer free
            if (jt + 32 < j1) {
                lstore(buf ^ 1);                           // tile jt+32 (loaded one iteration ago)
                if (jt + 64 < j1) gload(jt + 64);
            }
#if VO_RADIUS_PREREJECT
            const vo_f4 bx = *reinterpret_cast<const vo_f4*>(&bbox[buf][0]);
            const float lb = vo_radius_box_lb(bx.x, bx.y, bx.z, bx.w, rg.x, rg.y);
            if (__builtin_amdgcn_ballot_w64(live && lb <= (SWAP ? bbox[buf][4] : rg.z))) tile(buf, jt);
#else
            tile(buf, jt);
#endif
        }
        top2c_merge_lanes(best1, bidx1, second1, 32);
        if (h == 0 && live) {
            MatchTop2 mt;
            mt.best = best1; mt.idx = bidx1; mt.second = second1; mt.pad = 0;
            partial[(size_t)chunk * row_cap + ia] = mt;
        }
    }
}

hipError_t match_radius_alloc(DevPool& pool, MatchRadiusBuffers& r, const MatchBuffers& b)
{
    const size_t R = b.row_cap, T = 2 * ((R + 31) / 32);
    return (hipError_t)pool.group({DevPool::req(r.pts2, 2 * R), DevPool::req(r.centers, 2 * R), DevPool::req(r.radius, R),
                                   DevPool::req(r.geo1, R), DevPool::req(r.geo2, R), DevPool::req(r.box1, T),
                                   DevPool::req(r.box2, T)});
}

void match_radius_launch(const MatchBuffers& b, const MatchJob* d_job, const MatchExBuffers& x, const MatchRadiusBuffers& r,
                         const uint8_t* d1, const DescMeta* m1, int n1, const uint8_t* d2, const DescMeta* m2, int n2,
                         int col_major, int n_radius, const vo_match_params& p, int unique, hipStream_t s)
{
    if (n1 <= 0 || n2 <= 0) return;
    VO_LAUNCH(k_radius_meta, dim3((n1 + 31) / 32 + (n2 + 31) / 32), dim3(64), 0, s, (const float*)r.centers,
              (const float*)r.radius, n_radius, n1, (const float*)r.pts2, n2, col_major, r.geo1, r.box1, r.geo2, r.box2);
    const RadiusSide S1{d1, m1, r.geo1, r.box1, n1, 0}, S2{d2, m2, r.geo2, r.box2, n2, 0};
    const int nc1 = (n1 + VO_MATCH_CHUNK - 1) / VO_MATCH_CHUNK, nc2 = (n2 + VO_MATCH_CHUNK - 1) / VO_MATCH_CHUNK;
    const int fwd = ((n1 + MP_ROWS - 1) / MP_ROWS) * nc2, back = ((n2 + MP_ROWS - 1) / MP_ROWS) * nc1;
    VO_LAUNCH_NAMED("k_match_radius", k_match_radius<false>, dim3(std::min(fwd, VO_STEREO_GRID)), dim3(256), 0, s, S1, S2,
                    b.partial, b.row_cap);
    if (unique)
        VO_LAUNCH_NAMED("k_match_radius_back", k_match_radius<true>, dim3(std::min(back, VO_STEREO_GRID)), dim3(256), 0, s, S2, S1,
                        x.partial_back, b.row_cap);
    VO_LAUNCH(k_match_finish_unique, dim3(1), dim3(256), 0, s, d_job, (const MatchTop2*)b.partial,
              (const MatchTop2*)x.partial_back, b.row_cap, b.n_chunks, p.match_threshold * 0.04f, p.max_ratio, unique, x.metric);
}

// single-precision descriptor matrix (MATLAB's extractFeatures output: n x 128 single, integer
// values 0..255) -> packed u8 rows.  col_major: element (i, k) at F[i + k * ld] (MATLAB's own
// layout, so a MEX gateway passes mxGetSingles() without a copy); else F[i * ld + k].  One
// thread per element, the row index fastest for column-major input (coalesced reads).  A value
// that is not an integer in [0, 255] raises *bad.
__global__ __launch_bounds__(256) void k_pack_f32_desc(const float* __restrict__ F, int n, int ld, int col_major,
                                                       uint8_t* __restrict__ out, int* __restrict__ bad)
{
    const long total = (long)n * VO_DESC_LEN;
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        int i, k;
        float v;
        if (col_major) { i = (int)(t % n); k = (int)(t / n); v = F[(size_t)k * ld + i]; }
        else { i = (int)(t / VO_DESC_LEN); k = (int)(t % VO_DESC_LEN); v = F[(size_t)i * ld + k]; }
        const bool ok = v >= 0.0f && v <= 255.0f && v == rintf(v);
        out[(size_t)i * VO_DESC_LEN + k] = ok ? (uint8_t)v : 0;
        if (!ok) *bad = 1;
    }
}

void pack_f32_desc_launch(const float* F, int n, int ld, int col_major, uint8_t* out, int* bad, hipStream_t s)
{
    if (n <= 0) return;
    long total = (long)n * VO_DESC_LEN;
    int blocks = (int)std::min<long>((total + 255) / 256, 4096);
    VO_LAUNCH(k_pack_f32_desc, dim3(blocks), dim3(256), 0, s, F, n, ld, col_major, out, bad);
}

// ---------------------------------------------------------------------------
// matchFeatures on general single-precision features (vo_match_f32 when the rows are not
// u8-valued SIFT descriptors).  Spec, restated by the oracle's oracle_match_f32 (vo_ref.c):
//   a_k = f_k / nrm (0 if nrm == 0), nrm = sqrtf(fmaf chain of f_k^2 over k = 0..127);
//   ssd(i, j) = fmaf chain of (a_k - b_k)^2 over k = 0..127;
//   best / second = smallest / second smallest ssd of row i (multiset; ties -> lowest j);
//   accept best <= 0.04 * MatchThreshold and best / second <= MaxRatio (the u8 path's rule).
// k_f32_norm: one thread per row; F2 rows are written transposed ([128][n2]) so k_match_f32's
// lanes (one F2 column each) read them coalesced.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_f32_norm(const float* __restrict__ F, int n, int ld, int col_major, int transpose,
                                                  float* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    auto at = [&](int k) { return col_major ? F[(size_t)k * ld + i] : F[(size_t)i * ld + k]; };
    float n2 = 0.0f;
    for (int k = 0; k < VO_DESC_LEN; ++k) { const float v = at(k); n2 = fmaf(v, v, n2); }
    const float nrm = sqrtf(n2);
    for (int k = 0; k < VO_DESC_LEN; ++k) {
        const float v = nrm > 0.0f ? at(k) / nrm : 0.0f;
        out[transpose ? (size_t)k * n + i : (size_t)i * VO_DESC_LEN + k] = v;
    }
}

// one wave per F1 row (grid-stride): the row in LDS (broadcast reads), lane l scores columns
// l, l + 64, ... with the sequential fmaf chain, keeps its own top-2, and the wave merges the
// 64 top-2s with the order-free (value, index) rule; res[i] = accepted column or -1
__global__ __launch_bounds__(64) void k_match_f32(const float* __restrict__ A, int n1, const float* __restrict__ BT, int n2,
                                                  float T, float max_ratio, int* __restrict__ res)
{
    __shared__ float a[VO_DESC_LEN];
    const int lane = threadIdx.x;
    for (int i = blockIdx.x; i < n1; i += gridDim.x) {
        a[lane] = A[(size_t)i * VO_DESC_LEN + lane];
        a[lane + 64] = A[(size_t)i * VO_DESC_LEN + lane + 64];
        __syncthreads();
        float best = INFINITY, second = INFINITY;
        int bidx = -1;
        for (int j = lane; j < n2; j += 64) {
            float ssd = 0.0f;
            for (int k = 0; k < VO_DESC_LEN; ++k) {
                const float d = a[k] - BT[(size_t)k * n2 + j];
                ssd = fmaf(d, d, ssd);
            }
            if (ssd < best) { second = best; best = ssd; bidx = j; }
            else if (ssd < second) second = ssd;
        }
        top2s_merge_wave(best, bidx, second);
        if (lane == 0) res[i] = (bidx >= 0 && best <= T && best / second <= max_ratio) ? bidx : -1;
        __syncthreads();
    }
}

void match_f32_launch(const float* F1, int n1, int ld1, const float* F2, int n2, int ld2, int col_major, float* A, float* BT,
                      int* res, const vo_match_params& p, hipStream_t s)
{
    if (n1 <= 0) return;
    VO_LAUNCH(k_f32_norm, dim3((n1 + 255) / 256), dim3(256), 0, s, F1, n1, ld1, col_major, 0, A);
    if (n2 > 0) VO_LAUNCH(k_f32_norm, dim3((n2 + 255) / 256), dim3(256), 0, s, F2, n2, ld2, col_major, 1, BT);
    VO_LAUNCH(k_match_f32, dim3(std::min(n1, 8192)), dim3(64), 0, s, A, n1, BT, n2, p.match_threshold * 0.04f, p.max_ratio,
              res);
}

// k_match_f32 for vo_match_f32_ex: the same scores and top-2 per row; besides the accepted column
// (res, as k_match_f32 writes it) it stores the row's best SSD (best: matchMetric) and the best
// column regardless of the thresholds (arg: the backward pass of Unique).  Outputs may be null.
__global__ __launch_bounds__(64) void k_match_f32_ex(const float* __restrict__ A, int n1, const float* __restrict__ BT, int n2,
                                                     float T, float max_ratio, int* __restrict__ res, int* __restrict__ arg,
                                                     float* __restrict__ best_out)
{
    __shared__ float a[VO_DESC_LEN];
    const int lane = threadIdx.x;
    for (int i = blockIdx.x; i < n1; i += gridDim.x) {
        a[lane] = A[(size_t)i * VO_DESC_LEN + lane];
        a[lane + 64] = A[(size_t)i * VO_DESC_LEN + lane + 64];
        __syncthreads();
        float best = INFINITY, second = INFINITY;
        int bidx = -1;
        for (int j = lane; j < n2; j += 64) {
            float ssd = 0.0f;
            for (int k = 0; k < VO_DESC_LEN; ++k) {
                const float d = a[k] - BT[(size_t)k * n2 + j];
                ssd = fmaf(d, d, ssd);
            }
            if (ssd < best) { second = best; best = ssd; bidx = j; }
            else if (ssd < second) second = ssd;
        }
        top2s_merge_wave(best, bidx, second);
        if (lane == 0) {
            if (res) res[i] = (bidx >= 0 && best <= T && best / second <= max_ratio) ? bidx : -1;
            if (arg) arg[i] = bidx;
            if (best_out) best_out[i] = best;
        }
        __syncthreads();
    }
}

// vo_match_f32_ex on general features: the forward pass as match_f32_launch plus the metric; with
// `unique`, A and BT are then rewritten with the sides exchanged (stream order) and the same
// kernel gives back[j], the best F1 row of every F2 row -- the fmaf chain of (a_k - b_k)^2 is
// symmetric in its operands, so these are the forward scores.
void match_f32_launch_ex(const float* F1, int n1, int ld1, const float* F2, int n2, int ld2, int col_major, float* A, float* BT,
                         int* res, float* best, int* back, const vo_match_params& p, int unique, hipStream_t s)
{
    if (n1 <= 0) return;
    VO_LAUNCH(k_f32_norm, dim3((n1 + 255) / 256), dim3(256), 0, s, F1, n1, ld1, col_major, 0, A);
    if (n2 > 0) VO_LAUNCH(k_f32_norm, dim3((n2 + 255) / 256), dim3(256), 0, s, F2, n2, ld2, col_major, 1, BT);
    VO_LAUNCH(k_match_f32_ex, dim3(std::min(n1, 8192)), dim3(64), 0, s, (const float*)A, n1, (const float*)BT, n2,
              p.match_threshold * 0.04f, p.max_ratio, res, (int*)nullptr, best);
    if (!unique || n2 <= 0) return;
    VO_LAUNCH(k_f32_norm, dim3((n2 + 255) / 256), dim3(256), 0, s, F2, n2, ld2, col_major, 0, A);
    VO_LAUNCH(k_f32_norm, dim3((n1 + 255) / 256), dim3(256), 0, s, F1, n1, ld1, col_major, 1, BT);
    VO_LAUNCH(k_match_f32_ex, dim3(std::min(n2, 8192)), dim3(64), 0, s, (const float*)A, n2, (const float*)BT, n1, 0.0f, 0.0f,
              (int*)nullptr, back, (float*)nullptr);
}

void desc_meta_launch(const uint8_t* desc, DescMeta* meta, int n, hipStream_t s)
{
    if (n <= 0) return;
    int blocks = (n + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    VO_LAUNCH(k_desc_meta, dim3(blocks), dim3(256), 0, s, desc, meta, n);
}

}  // namespace vo
