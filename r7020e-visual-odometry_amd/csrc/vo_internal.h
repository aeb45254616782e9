// vo_internal.h — device data layout and kernel launch interfaces of libvo.
// Layout rationale: DESIGN.md §4.  All kernels are hand-written HIP for gfx950
// (wave64), compiled with -ffp-contract=off so every float operation is the
// IEEE basic op the spec (include/vo_spec.h) names.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include <string>
#include "vo.h"
#include "vo_spec.h"
#include "dev_pool.h"

#define VO_WAVE 64

namespace vo {

// ---------------------------------------------------------------------------
// Per-kernel HIP-event timing (vo_set_profiling).  When enabled every launch
// made through VO_LAUNCH is bracketed by two events on its stream; the
// durations are summed per kernel name after the call synchronises.
// ---------------------------------------------------------------------------
struct Profiler {
    bool on = false;
    std::vector<hipEvent_t> pool;
    int used = 0;
    std::vector<std::pair<const char*, int>> marks;   // (kernel name, start event index)
    std::vector<std::string> names;
    std::vector<double> ms;
    std::vector<int> calls;
    void begin(const char* name, hipStream_t s);
    void end(hipStream_t s);
    void collect();      // after the stream has synchronised
    void reset_totals();
    ~Profiler();
};
// the profiler of the API call running on this thread (vo_api.hip: CallScope), else null
extern thread_local Profiler* g_prof;

#define VO_LAUNCH_NAMED(name, kernel, grid, block, shmem, stream, ...)                     \
    do {                                                                                   \
        if (::vo::g_prof && ::vo::g_prof->on) ::vo::g_prof->begin(name, stream);           \
        hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);               \
        if (::vo::g_prof && ::vo::g_prof->on) ::vo::g_prof->end(stream);                   \
    } while (0)
#define VO_LAUNCH(kernel, grid, block, shmem, stream, ...) \
    VO_LAUNCH_NAMED(#kernel, kernel, grid, block, shmem, stream, __VA_ARGS__)

// ---------------------------------------------------------------------------
// Scale-space arena, image-major: the whole pyramid of one image is contiguous,
// G(o,i,img) = arena + img*istride + g_off[o][i], so any contiguous range of
// images is a pointer shift (sub-batches run concurrently on separate streams).
// DoG planes are not stored: D(o,i) = G(o,i+1) - G(o,i) where it is consumed.
// Rows are padded to a multiple of 256 floats (1 KiB): every row starts on a
// cache-line boundary and spans a whole number of the level blur's 256-column
// strips, so lanes past the last column store into padding instead of branching.
// ---------------------------------------------------------------------------
struct OctGeom {
    int rows, cols, pitch;
    int dmax;                           // descriptor window radius cap, (int)sqrt(cols^2 + rows^2)
    size_t plane;                       // rows * pitch (floats)
    size_t g_off[VO_SIFT_MAX_LAYERS];   // L+3 Gaussian levels
};

struct Pyramid {
    int n_oct, L, n_img;
    OctGeom oct[VO_SIFT_MAX_OCTAVES];
    float kern[VO_SIFT_MAX_LAYERS][VO_SIFT_MAX_RADIUS + 1];  // level blur kernels (level 0 = base)
    int krad[VO_SIFT_MAX_LAYERS];
    size_t istride;                      // floats per image (all octaves and levels)
    size_t total;                        // floats in the arena
    size_t tmp_plane;                    // floats per image of the horizontal-pass scratch
    // extrema word layout: per (octave, layer, interior row) the words of 64
    // absolute columns [64k, 64k+64); bits of border columns are 0
    int wbase[VO_SIFT_MAX_OCTAVES * 4 + 1];   // prefix over (o, layer-1) blocks; size n_oct*L+1
    int wrow[VO_SIFT_MAX_OCTAVES];            // words per row in octave o
    int n_words;                              // words per image
    // extremum-test units: (strip of 128 columns, band of VO_EXT_BAND interior rows)
    int ebase[VO_SIFT_MAX_OCTAVES + 1];       // prefix of units per octave
    int estrips[VO_SIFT_MAX_OCTAVES];         // strips per row in octave o
    int n_units;                              // units per image
    int n_seg;                                // 1024-word compaction segments per image
    int dcap;                                 // largest descriptor window radius the parameters allow
};

// k_desc's per-keypoint window tables in LDS (desc_tables), u32 words: a header of DT_HDR words
// (DT_ORI .. DT_LAYER below), the row table (2 dcap + 10 entries) and the separable window
// weights (dcap + 1 floats); stride rounded to 16 B.
#define DT_HDR 12
enum { DT_ORI, DT_PX, DT_PY, DT_RADIUS, DT_COS, DT_SIN, DT_NSAMP, DT_NROWS, DT_O, DT_LAYER };
static inline __host__ __device__ int dt_rtab_off() { return DT_HDR; }
static inline __host__ __device__ int dt_wtab_off(int dcap) { return DT_HDR + 2 * dcap + 10; }
static inline __host__ __device__ int dt_stride(int dcap) { return (DT_HDR + 3 * dcap + 11 + 3) & ~3; }

#ifndef VO_EXT_BAND
#define VO_EXT_BAND 30            // interior rows per extremum-test wave (a multiple of 3)
#endif
#define VO_SEG_WORDS 1024

// Packed candidate: c | r << 12 | layer << 24 | o << 27  (c, r < 4096)
__host__ __device__ inline uint32_t pack_cand(int o, int layer, int r, int c) {
    return (uint32_t)c | ((uint32_t)r << 12) | ((uint32_t)layer << 24) | ((uint32_t)o << 27);
}

// Refined candidate with its orientation peaks (output of refine_orient).
struct CandOut {
    float xo, yo, scl, response;
    int o, layer, r, c;
    int npk, pad0, pad1, pad2;
    float ang[VO_SIFT_MAX_PEAKS + 2];
};

// Internal keypoint record used by the descriptor kernel.
struct KpInt {
    float xo, yo, scl, angle;
    int o, layer, pad0, pad1;
};

// Per-descriptor metadata for matching: exact integer sums.
struct DescMeta {
    int32_t sum;      // sum of the 128 u8 values
    float inv_norm;   // 1/sqrtf((float)sum of squares), 0 if zero
};

// Buffers of the SIFT stage for a batch of n_img images.
struct SiftBuffers {
    float* arena = nullptr;
    float* tmp = nullptr;              // horizontal-pass scratch [n_img][tmp_plane]
    unsigned long long* mask = nullptr;  // [n_img][n_words]
    uint32_t* woff = nullptr;          // [n_img][n_seg] segment counts, then exclusive offsets
    uint32_t* cand = nullptr;          // [n_img][cand_cap]
    int* n_cand = nullptr;             // [n_img]  (uncapped count)
    int* acc = nullptr;                // [n_img][cand_cap] accepted candidates' indices (k_refine, any order)
    int* n_acc = nullptr;              // [n_img]
    CandOut* cout = nullptr;           // [n_img][cand_cap]
    uint32_t* koff = nullptr;          // [n_img][cand_cap]
    int* n_kp = nullptr;               // [n_img]  (uncapped count; with selectStrongest the selected count)
    int* n_det = nullptr;              // [n_img]  detected count ahead of selectStrongest (written only while it is on)
    unsigned long long* skey = nullptr;  // [n_img][cand_cap] selectStrongest keys in acc order (sift_alloc_select)
    uint32_t* snpk = nullptr;          // [n_img][cand_cap] ... and peak counts
    vo_keypoint* kp = nullptr;         // [n_img][kp_cap]
    KpInt* kpi = nullptr;              // [n_img][kp_cap]
    uint8_t* desc = nullptr;           // [n_img][kp_cap][128]
    DescMeta* meta = nullptr;          // [n_img][kp_cap]
    int cand_cap = 0, kp_cap = 0, n_img = 0;
};

// Image source for the first octave: image i of the batch is
// (i & 1 ? right : left) + (i >> 1) * frame_stride, row-major with ld.
struct ImageSrc {
    const uint8_t* left;
    const uint8_t* right;
    size_t frame_stride;
    int ld;
    int pad;
};

void build_pyramid_geometry(Pyramid& py, int rows, int cols, int n_img, const vo_sift_params& p);
// Parameters the SIFT kernels' fixed-point and window bounds admit (vo_create refuses others):
// 1..5 layers, sigma finite and > 0, every orientation window small enough for k_orient's u32 column
// sums, every blur radius at most VO_SIFT_MAX_RADIUS, finite thresholds (contrast >= 0, edge > 0).
// -> nullptr when supported, else the name of the offending field.  Host arithmetic only.
const char* sift_params_refusal(const vo_sift_params& p);
// View of images [img0, img0 + n) of b: every per-image array shifted (image-major layout).
SiftBuffers sift_view(const SiftBuffers& b, const Pyramid& py, int img0, int n);
// what the *_alloc functions allocate belongs to the pool (the context's), which frees it
hipError_t sift_alloc(DevPool& pool, SiftBuffers& b, const Pyramid& py, int kp_cap, int cand_cap);
hipError_t sift_alloc_select(DevPool& pool, SiftBuffers& b);     // selectStrongest's key arrays (first vo_set_strongest(n > 0))
// Enqueue the whole detect+describe pipeline for n_img images (<= allocated).
// d_py is a device copy of py.  strongest > 0: SIFTPoints.selectStrongest(points, strongest) between
// detection and description (k_sel_keys / k_sel_rank; needs sift_alloc_select); 0 launches neither.
void sift_enqueue(const Pyramid& py, SiftBuffers& b, const ImageSrc& src, int n_img,
                  const vo_sift_params& p, hipStream_t s, const Pyramid* d_py, int strongest = 0);
// The phases of sift_enqueue: the scale space of the large octaves (base, level blurs, octave
// bases; ev_o0, if given, is recorded once octave 0 is complete); its tail (the LDS-sized octaves
// and the extremum test of octaves [ext_o_begin, n_oct)); the extremum test of an octave range;
// and the feature stages (mask compaction, refinement, orientation, descriptors).  The batched
// path runs the extremum test of octave 0 on the feature stream as soon as ev_o0 fires, beside
// the scale space of octaves 1.., and the rest at the scale space's tail (vo_api.hip).
// The scale space as two chains (batched path, sift.hip: sift_enqueue_pyramid): with `down`, the
// octaves after the fork octave (1, or 0 when only octave 0 is a large one; a later one while the
// next octave's blurs are still HBM-bound) run on `down` once
// ev_fork -- recorded on s after the fork octave's level-L blur -- has fired, beside that octave's
// levels L+1, L+2 on s.  The caller enqueues sift_enqueue_small on `down` and orders the extremum
// test of octaves 1.. after the end of both s and `down`.  Streams and events belong to the caller;
// none is created here.
struct ScaleChains {
    hipStream_t down = nullptr;         // nullptr (or s): one chain on s
    hipEvent_t ev_fork = nullptr;
};
void sift_enqueue_pyramid(const Pyramid& py, SiftBuffers& b, const ImageSrc& src, int n_img,
                          const vo_sift_params& p, hipStream_t s, const Pyramid* d_py, hipEvent_t ev_o0 = nullptr,
                          const ScaleChains& ch = ScaleChains());
void sift_enqueue_pyramid_tail(const Pyramid& py, SiftBuffers& b, int n_img, const vo_sift_params& p, hipStream_t s,
                               const Pyramid* d_py, int ext_o_begin);
void sift_enqueue_extrema(const Pyramid& py, SiftBuffers& b, int n_img, const vo_sift_params& p, hipStream_t s,
                          const Pyramid* d_py, int o_begin, int o_end);
// the LDS-sized octaves o >= sift_small_octave(py) (one k_small_pyr launch; n_oct when none)
int sift_small_octave(const Pyramid& py);
void sift_enqueue_small(const Pyramid& py, SiftBuffers& b, int n_img, hipStream_t s, const Pyramid* d_py);
void sift_enqueue_features(const Pyramid& py, SiftBuffers& b, int n_img, const vo_sift_params& p, hipStream_t s,
                           const Pyramid* d_py, int strongest = 0);

// vo_describe: the scale space of n_img images (one chain on s, no extremum test), then the
// descriptors of caller-given points: b.kp holds the points' vo_keypoint rows [img][kp_cap] and
// b.n_kp their per-image counts (uploaded on s before the call; n_points = their sum, checked by
// the host against vo_check_points' rules); k_points writes b.kpi from them and k_desc_pts -- the
// descriptor code with window tables of capacity VO_SIFT_DESCR_RMAX -- b.desc and b.meta.
void sift_enqueue_describe(const Pyramid& py, SiftBuffers& b, const ImageSrc& src, int n_img, int n_points,
                           const vo_sift_params& p, hipStream_t s, const Pyramid* d_py);

// ---------------------------------------------------------------------------
// undistortImage (undistort.hip): k_undistort remaps B frames of one or two cameras in one
// launch.  Side k reads frame f at in + f * in_stride and writes it at out + f * out_stride, both
// row-major with leading dimension cols; copy = 1 passes the side through unchanged.
// ---------------------------------------------------------------------------
#define VO_UD_CHUNK 16            // frames per thread: the f64 map of its pixels is evaluated once per chunk
struct UndistortSide {
    vo_bc_cam cam;
    const uint8_t* in;
    uint8_t* out;
    int copy, pad;
};
void undistort_launch(const UndistortSide* sides, int n_sides, int rows, int cols, int B, size_t in_stride,
                      size_t out_stride, hipStream_t s);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize, 160 KB) once per (kernel, device)
void raise_lds_limit(const void* fn);

// ---------------------------------------------------------------------------
// Matching.  A match job compares F1 rows (desc[idx1[i]] for i < *n1) against
// F2 rows.  idx == nullptr means identity.  Counts are read on device.
// ---------------------------------------------------------------------------
struct MatchJob {
    const uint8_t* d1; const DescMeta* m1; const int* idx1; const int* n1;
    const uint8_t* d2; const DescMeta* m2; const int* idx2; const int* n2;
    int* out_i;      // [cap] F1 positions (0-based, position in the F1 list)
    int* out_j;      // [cap] F2 positions
    int* out_n;      // matches found
    int cap;
    int pad;
};

// Per (row, F2 chunk) top-2 in the cosine domain: best/second are the largest
// c = ((float)dot * inv|a|) * inv|b| values (SSD = 2 - 2c is non-increasing in c).
struct MatchTop2 { float best; int idx; float second; int pad; };

struct MatchBuffers {
    MatchTop2* partial = nullptr;    // [max_jobs][n_chunks][row_cap]
    int max_jobs = 0, row_cap = 0, n_chunks = 0;
};

#ifndef VO_MATCH_CHUNK
#define VO_MATCH_CHUNK 4096          // F2 columns per task (512/1024/2048 swept before; 4096: the tracking steps' ~2.1 k
                                     // columns in one chunk, match -10 % isolated, full path +1.3 %, r06_y)
#endif

hipError_t match_alloc(DevPool& pool, MatchBuffers& b, int max_jobs, int row_cap);
// View whose job slot 0 is slot k0 of b (partial-result rows of jobs k0, k0+1, ...).
MatchBuffers match_view(const MatchBuffers& b, int k0);
// d_jobs: device array of n_jobs jobs (prepared once per context); job k uses
// partial-result slot k.
// The index composition after tracking step `step` of find_remaining_points (VO.m:287-290,
// 297-300, 305-308, 314-317, 326-333) over lists [frame][TL_COUNT][kp_cap] (vo_geom.h), applied
// by match_launch's finishing kernel to the step's compacted pairs of job f (= frame f).
struct MatchCompose {
    int* lists; int* list_n;
    const int* pair_i; const int* pair_j;    // stereo pairs per pair slot (frame f-1's, or slot M)
    int M, kp_cap, step;
    int f0;                                  // frame of job 0 (a launch split at VO_MP_MAX_JOBS jobs)
};
void match_launch(const MatchBuffers& b, const MatchJob* d_jobs, int n_jobs, const vo_match_params& p,
                  hipStream_t s, const MatchCompose* compose);
void match_launch(const MatchBuffers& b, const MatchJob* d_jobs, int n_jobs, const vo_match_params& p,
                  hipStream_t s);
// vo_match_ex / vo_match_f32_ex (explicit thresholds, matchMetric, Unique): what they need beyond
// MatchBuffers, allocated by the first such call.  job_back is the single job with its two sides
// exchanged, partial_back its partial slot [n_chunks][row_cap] (rows = F2, chunks over F1),
// metric the accepted pairs' SSD in output order (u8 path) or per F1 row (float path), back the
// float path's best F1 row per F2 row.
struct MatchExBuffers {
    MatchJob* job_back = nullptr;
    MatchTop2* partial_back = nullptr;
    float* metric = nullptr;
    int* back = nullptr;
};
hipError_t match_ex_alloc(DevPool& pool, MatchExBuffers& x, const MatchBuffers& b, const MatchJob& job_back);   // all or nothing
// d_job: the job (device); its partials use b's slot 0 as in match_launch(b, d_job, 1, ...)
void match_launch_ex(const MatchBuffers& b, const MatchJob* d_job, const MatchExBuffers& x, const vo_match_params& p, int unique,
                     hipStream_t s);
void match_f32_launch_ex(const float* F1, int n1, int ld1, const float* F2, int n2, int ld2, int col_major, float* A, float* BT,
                         int* res, float* best, int* back, const vo_match_params& p, int unique, hipStream_t s);
// vo_match_radius / vo_match_radius_f32 (matchFeaturesInRadius): what they need beyond MatchBuffers
// and MatchExBuffers, allocated by the first such call.  pts2 / centers / radius are the caller's
// arrays as they lie; geo1 [row_cap] = {cx, cy, r2, 0} per F1 row, geo2 [row_cap] = {x, y, 0, 0} per
// F2 row; box1 / box2 two float4 per aligned 32-row tile: {xmin, xmax, ymin, ymax} of the tile's
// positions and {largest r2, 0, 0, 0} (F1 side; 0 on the F2 side).
typedef float vo_geo4 __attribute__((ext_vector_type(4)));
struct MatchRadiusBuffers {
    float* pts2 = nullptr;           // [row_cap][2]
    float* centers = nullptr;        // [row_cap][2]
    float* radius = nullptr;         // [row_cap]
    vo_geo4* geo1 = nullptr;
    vo_geo4* geo2 = nullptr;
    vo_geo4* box1 = nullptr;         // [2 * ceil(row_cap / 32)]
    vo_geo4* box2 = nullptr;
};
hipError_t match_radius_alloc(DevPool& pool, MatchRadiusBuffers& r, const MatchBuffers& b);   // all or nothing
// One in-radius match of the two staged descriptor sets d1 / d2 (metadata m1 / m2, n1, n2 > 0 rows):
// k_radius_meta over r's raw arrays (col_major: point (i, k) at P[i + k * n]; n_radius 1 or n1), the
// gated forward pass into b's slot 0, with `unique` the gated backward pass into x.partial_back,
// then k_match_finish_unique on d_job (whose counts are n1, n2).
void match_radius_launch(const MatchBuffers& b, const MatchJob* d_job, const MatchExBuffers& x, const MatchRadiusBuffers& r,
                         const uint8_t* d1, const DescMeta* m1, int n1, const uint8_t* d2, const DescMeta* m2, int n2,
                         int col_major, int n_radius, const vo_match_params& p, int unique, hipStream_t s);
void desc_meta_launch(const uint8_t* desc, DescMeta* meta, int n, hipStream_t s);
void pack_f32_desc_launch(const float* F, int n, int ld, int col_major, uint8_t* out, int* bad, hipStream_t s);
// matchFeatures on general single features (not u8-valued): normalised rows A [n1][128], F2
// normalised and transposed into BT [128][n2], res[i] = accepted F2 column of row i or -1
void match_f32_launch(const float* F1, int n1, int ld1, const float* F2, int n2, int ld2, int col_major, float* A, float* BT,
                      int* res, const vo_match_params& p, hipStream_t s);

// ---- vision.PointTracker (klt.hip): vo_track_points / vo_track_points_batch ----
// Buffers of their own, allocated by klt_reserve at the first launching call and grown to the
// largest batch seen, so the loop's buffer sets are never touched.  planes is level-major: level l
// of image i (i = which * n_pairs + pair) at klt_level_offset(l) + i * rows_l * cols_l, level 0 the
// staged images themselves.
struct KltBuffers {
    int cap_pairs = 0; size_t cap_pts = 0;
    int last_pairs = 0, last_levels = 0;          // of the last launching call (vo_fetch_klt_level)
    uint8_t* planes = nullptr;                    // [6 levels][2 n_pairs][rows_l][cols_l]
    int* n = nullptr;                             // [n_pairs]
    float* pts0 = nullptr; float* guess = nullptr; float* pts1 = nullptr;   // [n_pairs][pts_stride][2]
    uint8_t* valid = nullptr; float* scores = nullptr; vo_klt_info* info = nullptr;   // [n_pairs][pts_stride]
};
hipError_t klt_reserve(DevPool& pool, KltBuffers& kb, int rows, int cols, int n_pairs, int pts_stride);   // all or nothing per group
size_t klt_level_offset(int rows, int cols, int n_pairs, int level);
// k_klt_pyr: levels 1 .. levels - 1 of all 2 n_pairs images, one launch per level
void klt_pyr_launch(KltBuffers& kb, int rows, int cols, int n_pairs, int levels, hipStream_t s);
// k_klt_track: one wave per point and pair over kb.pts0 / kb.guess / kb.n -> kb.pts1, valid, scores, info
void klt_track_launch(KltBuffers& kb, int rows, int cols, int n_pairs, int pts_stride, int max_n, bool has_guess,
                      const vo_klt_params& p, hipStream_t s);

// ---- detectMinEigenFeatures / detectHarrisFeatures (corner.hip): vo_detect_corners[_batch] ----
// Buffers of their own, allocated by corner_reserve at the first launching call and grown to the
// largest batch seen, so the loop's buffer sets are never touched.  list_cap = 4 x max_keypoints.
struct CornerBuffers {
    int cap_img = 0, list_cap = 0;
    int last_img = 0;                             // of the last launching call (vo_fetch_corner_metric)
    uint8_t* img = nullptr;                       // [n_img][rows][cols]
    float* metric = nullptr;                      // [n_img][rows][cols]
    uint32_t* mmax = nullptr;                     // [n_img] the ROI's maximum, as the bits of a float >= 0
    int* cnt = nullptr;                           // [n_img][chunks of the whole image]
    int* total = nullptr;                         // [n_img] the true count
    float* loc = nullptr; float* met = nullptr;   // [n_img][list_cap][2], [n_img][list_cap]: raster order
    float* sloc = nullptr; float* smet = nullptr; // the same, ranked (strongest > 0)
};
hipError_t corner_reserve(DevPool& pool, CornerBuffers& cb, int rows, int cols, int n_img, int list_cap);   // all or nothing
// k_corner_metric, k_corner_count, k_corner_emit and, with p.strongest > 0, k_corner_rank over cb.img;
// roi0 = x y w h, 0-based, inside the image
hipError_t corner_launch(CornerBuffers& cb, int rows, int cols, int n_img, const vo_corner_params& p, const int* roi0, hipStream_t s);

// ---- disparitySGM / reconstructScene (sgm.hip): vo_disparity_sgm[_batch[_dev]], vo_reconstruct_scene ----
// Buffers of their own, allocated at the first launching call, so the loop's buffer sets are never
// touched.  The workspace (census words, the sums S) holds one group of at most VO_SGM_GROUP pairs at the
// largest D seen; img / disp stage the host entries' group; rin / xyz are vo_reconstruct_scene's.
struct SgmBuffers {
    int cap_pairs = 0, cap_D = 0, cap_io = 0;
    int last_pairs = 0, last_first = 0, last_D = 0;   // the last group of the last launching call (vo_fetch_sgm_cost)
    uint64_t* cen = nullptr;                          // [pair][2][rows][cols]
    uint16_t* S = nullptr;                            // [pair][rows][cols][D]
    uint8_t* img = nullptr;                           // [2][cap_io][rows][cols]: lefts, then rights
    float* disp = nullptr;                            // [cap_io][rows * cols]
    float* rin = nullptr; float* xyz = nullptr;       // [rows * cols], [3 * rows * cols]
};
hipError_t sgm_reserve(DevPool& pool, SgmBuffers& sb, int rows, int cols, int n_group, int D, bool host_io);   // all or nothing
// k_sgm_census, the four k_sgm_paths launches and k_sgm_select over G <= cap_pairs packed row-major pairs;
// d_disp [G][rows * cols] in row-major or (col_major) column-major order
void sgm_launch(SgmBuffers& sb, const uint8_t* d_lefts, const uint8_t* d_rights, int rows, int cols, int G, const vo_sgm_params& p,
                int col_major, float* d_disp, hipStream_t s);
hipError_t reconstruct_reserve(DevPool& pool, SgmBuffers& sb, int rows, int cols);
void reconstruct_launch(const float* d_disp, int rows, int cols, int col_major, const double* Q, float* d_xyz, hipStream_t s);

}  // namespace vo
