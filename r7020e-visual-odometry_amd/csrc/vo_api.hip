// vo_api.hip — the C-ABI of libvo (include/vo.h): context, staging and the
// orchestration of the per-frame pipeline on one HIP stream.
#include "vo_internal.h"
#include "vo_geom.h"
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdarg>
#include <string>
#include <vector>
#include <deque>
#include <algorithm>

namespace vo {

thread_local Profiler* g_prof = nullptr;

void Profiler::begin(const char* name, hipStream_t s)
{
    if (used + 2 > (int)pool.size()) {
        int add = std::max(64, (int)pool.size());
        for (int i = 0; i < add; ++i) { hipEvent_t e; hipEventCreate(&e); pool.push_back(e); }
    }
    marks.push_back({name, used});
    hipEventRecord(pool[used], s);
    used += 1;
}

void Profiler::end(hipStream_t s)
{
    hipEventRecord(pool[used], s);
    used += 1;
}

void Profiler::collect()
{
    for (auto& m : marks) {
        float t = 0.0f;
        hipEventElapsedTime(&t, pool[m.second], pool[m.second + 1]);
        std::string n(m.first);
        size_t k = 0;
        for (; k < names.size(); ++k) if (names[k] == n) break;
        if (k == names.size()) { names.push_back(n); ms.push_back(0.0); calls.push_back(0); }
        ms[k] += t;
        calls[k] += 1;
    }
    marks.clear();
    used = 0;
}

void Profiler::reset_totals() { names.clear(); ms.clear(); calls.clear(); marks.clear(); used = 0; }

Profiler::~Profiler() { for (auto e : pool) hipEventDestroy(e); }

}  // namespace vo

using namespace vo;

// the pool's way to the HIP runtime: every stream non-blocking, every event without timing
static int hip_make(PoolKind kind, size_t bytes, void** out)
{
    switch (kind) {
    case POOL_DEVICE: return hipMalloc(out, bytes);
    case POOL_PINNED: return hipHostMalloc(out, bytes, 0);
    case POOL_EVENT: return hipEventCreateWithFlags((hipEvent_t*)out, hipEventDisableTiming);
    default: return hipStreamCreateWithFlags((hipStream_t*)out, hipStreamNonBlocking);
    }
}
static void hip_drop(PoolKind kind, void* h)
{
    switch (kind) {
    case POOL_DEVICE: (void)hipFree(h); break;
    case POOL_PINNED: (void)hipHostFree(h); break;
    case POOL_EVENT: (void)hipEventDestroy((hipEvent_t)h); break;
    default: (void)hipStreamDestroy((hipStream_t)h);
    }
}

struct vo_ctx {
    // everything the context allocates, released when the context is deleted (the device selected)
    DevPool pool{PoolBackend{hip_make, hip_drop}};
    int device = 0, rows = 0, cols = 0, max_batch = 0;
    vo_sift_params sp;
    vo_match_params mp;
    vo_ransac_params rp;
    vo_calib calib;
    bool has_calib = false;
    hipStream_t stream = nullptr;
    // sub-batch concurrency: a batch's frames are split over n_sub streams that
    // fork from / join into `stream` (latency-bound SIFT stages of one part
    // overlap bandwidth-bound stages of another)
    static constexpr int MAX_SUB = 4;
    int n_sub = 1;
    hipStream_t sub[MAX_SUB] = {};                 // sub[0]: scale-space stream, sub[1]: feature stream
    hipEvent_t ev_fork = nullptr, ev_join[MAX_SUB] = {}, ev_o0[MAX_SUB] = {};
    // the scale space's second chain (octaves 2.. and k_small_pyr, beside octave 1's top levels):
    // ev_down[p] is recorded on sub[0] after the fork octave's level-L blur of part p, ev_top[p]
    // at the end of sub[0]'s chain, ev_join[p] at the end of this one
    hipStream_t down = nullptr;
    hipEvent_t ev_down[MAX_SUB] = {}, ev_top[MAX_SUB] = {};
    // Asynchronous batch pipeline (vo_sift_match_batch_dev): calls alternate between the two
    // buffer sets.  A call's scale space waits only for the previous use of its own set, so
    // the pyramid of call N+1 overlaps the latency-bound feature stages of call N.
    // Each set is the full per-frame state (image slots incl. the carried frame, pair slots
    // incl. the carry slot, stereo + tracking jobs, geometry buffers), so the full per-frame
    // path can also alternate sets (vo_step_submit_dev).  The synchronous single-image and
    // standalone entries (vo_sift, vo_describe, vo_track, ...) use set 0.
    struct BufferSet {
        SiftBuffers sb;                  // 2*max_batch + 2 image slots (last 2 = carried frame)
        MatchBuffers mb;                 // max_batch partial-result slots (a job's index within its launch)
        MatchJob* d_jobs = nullptr;      // [0, M) stereo, [M, 5M) tracking (job_stereo / job_track)
        int* pair_i = nullptr;           // stereo pairs per frame slot [max_batch + 1][kp_cap]
        int* pair_j = nullptr;
        int* pair_n = nullptr;           // [max_batch + 1]
        GeomBuffers gb;
        hipEvent_t ev_done = nullptr;    // the set's last SIFT + stereo match is done
        hipEvent_t ev_arena = nullptr;   // set's scale-space arena read for the last time (after k_desc)
        // the set's last SIFT call ran with vo_set_strongest on, so its n_det holds the detected
        // counts (otherwise n_kp does)
        bool sel_used = false;
        // the set's last step batch ran with vo_set_pose_refinement on, so gb.refine holds its stats
        bool refine_used = false;
    } set[2];
    int next_set = 0, last_set = 0;
    Pyramid py;
    Pyramid* d_py = nullptr;
    uint8_t* d_img = nullptr;        // image staging [2*max_batch][rows*cols]
    uint8_t* d_cm = nullptr;         // column-major (MATLAB) image staging, allocated on first use
    size_t cm_cap = 0;
    // vo_set_distortion: the loop-body entries undistort every frame ahead of the scale space
    // (enqueue_sift_stereo) into d_rect: left frames [0, max_batch), right frames [max_batch,
    // 2 max_batch), allocated by the first non-trivial call.  One buffer for both buffer sets and
    // every batch in flight: only the octave-0 base kernels read it, on the stream that writes it.
    bool ud_on[2] = {false, false};
    vo_bc_cam ud_cam[2] = {};
    uint8_t* d_rect = nullptr;
    int rect_B = 0;                  // frames of the last batched call that went through d_rect
    // vo_triangulate_ex / vo_fetch_track_quality: one frame's reprojection errors and validity flags
    // ([kp_cap] each), allocated by the first call that asks for either
    float* d_tq_err = nullptr;
    uint8_t* d_tq_valid = nullptr;
    // vo_set_strongest: SIFTPoints.selectStrongest(points, strongest) between detection and
    // description in every entry that detects (0 = off)
    int strongest = 0;
    // vo_set_pose_refinement: bundleAdjustmentMotion after MSAC in every entry that runs the loop body
    bool refine_on = false;
    vo_refine_params refine = {};
    // the last SIFT call was vo_describe / vo_describe_batch: set 0 holds a scale space and the
    // caller's points, no detections, so the fetches of a detecting call's results are refused
    bool described = false;
    // vo_match staging
    uint8_t* d_fd[2] = {nullptr, nullptr};
    DescMeta* d_fm[2] = {nullptr, nullptr};
    int* d_fn = nullptr;             // [2]
    MatchJob* d_job_single = nullptr;   // vo_match's one job over the staging above (partials: set 0's slot 0)
    float* d_ff[2] = {nullptr, nullptr};   // vo_match_f32 staging (single descriptors as MATLAB holds them)
    // vo_match_f32 on general (non-u8-valued) features: normalised F1, transposed F2, per-row result
    // (allocated on first use)
    float* d_fa = nullptr;
    float* d_fbt = nullptr;
    int* d_fres = nullptr;
    MatchExBuffers mx;               // vo_match_ex / vo_match_f32_ex (allocated on first use)
    MatchRadiusBuffers mr;           // vo_match_radius / vo_match_radius_f32 (allocated on first use)
    FundBuffers fund;                // vo_est_fundamental / vo_est_fundamental_batch (allocated on first use)
    KltBuffers klt;                  // vo_track_points / vo_track_points_batch (allocated on first use)
    CornerBuffers corner;            // vo_detect_corners / vo_detect_corners_batch (allocated on first use)
    SgmBuffers sgm;                  // vo_disparity_sgm* / vo_reconstruct_scene (allocated on first use)
    int* d_bad = nullptr;
    int* d_mi = nullptr; int* d_mj = nullptr; int* d_mn = nullptr;
    // Pipelined full path (vo_step_submit_dev / vo_step_collect): batch n uses buffer set
    // n & 1; its geometry runs on `stream` while the later batches' SIFT runs on sub[0..1].
    // Up to VO_STEP_DEPTH batches are in flight, so each batch also owns a result slot
    // (n mod VO_STEP_DEPTH): pinned host copies of the per-frame results, its packed landmark
    // rows on the device, and the event that ends the batch (geometry, carry into the other
    // set, result copies).  A slot outlives its buffer set's reuse by batch n+2.
    struct StepHost {
        FrameGeom* fg = nullptr; int* nkp = nullptr; int* ncand = nullptr; int* np = nullptr; int* rows = nullptr;
        int* ndet = nullptr;                               // detected counts (selectStrongest on; else nkp is both)
        float* pX = nullptr; uint8_t* pkeep = nullptr;     // the batch's packed landmark rows (pinned)
        float* d_pX = nullptr; uint8_t* d_pkeep = nullptr; // ... and on the device (k_lm_pack)
        hipEvent_t ev = nullptr;                           // end of the batch on `stream`
    };
    StepHost sh[VO_STEP_DEPTH];
    hipStream_t copy_stream = nullptr;
    struct Pending { int set, slot, B; bool first_tracked; bool sel; };
    std::deque<Pending> pending;
    int next_step_set = 0, next_slot = 0;
    std::vector<void*> lm_retired;                   // landmark stores replaced by a larger one (freed at reset)
    int last_step_set = -1, last_step_B = 0;          // the most recently collected batch (vo_fetch_tracks)
    std::string err;
    Profiler prof;
    int last_B = 0;
    // loop state (vo_step)
    long frame_index = 0;
    bool have_features = false;
    double pose[16];
    std::vector<double> landmarks;
    // camera-frame landmark rows (vo_set_landmark_frame(ctx, 1)): sharded sequences.  The rows
    // stay in device memory (appended by collect from the packed batch rows, a device-to-device
    // copy on `stream`), so the world transform after the gathered chain runs on the device and
    // only the world rows move (vo_landmarks_world_dev)
    int lm_camera = 0;
    float* d_lmX = nullptr;                       // [lm_cap][3]
    uint8_t* d_lmkeep = nullptr;                  // [lm_cap]
    size_t lm_cap = 0, lm_n = 0;
    std::vector<long long> lm_frame_off{0};       // row offset of every collected frame (+ end)
    double* d_lmw_pose = nullptr;                 // vo_landmarks_world_dev staging: poses, offsets
    long long* d_lmw_off = nullptr;
    int lmw_cap = 0;
};

static std::string g_create_err;

static int fail(vo_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_err = buf;
    return code;
}

#define HIPC(c, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(c, VO_ERR_HIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

static const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

extern "C" {

void vo_default_sift_params(vo_sift_params* p)
{
    p->n_octave_layers = 3; p->sigma = 1.6f; p->contrast_threshold = 0.04f; p->edge_threshold = 10.0f;
    p->upsample = 1; p->max_keypoints = 16384;
}
void vo_default_match_params(vo_match_params* p) { p->match_threshold = 1.0f; p->max_ratio = 0.6f; }
void vo_default_match_opts(vo_match_opts* o) { o->match_threshold = 1.0f; o->max_ratio = 0.6f; o->unique = 0; o->reserved = 0; }
void vo_default_ransac_params(vo_ransac_params* p)
{
    p->max_num_trials = 1000; p->confidence = 99.0; p->max_reprojection_error = 1.0; p->seed = 0x5EED;
}
void vo_default_refine_params(vo_refine_params* p)
{
    p->max_iterations = 20; p->relative_tolerance = 1e-9; p->absolute_tolerance = 0.0; p->lambda0 = 1e-3;
}
void vo_default_fund_params(vo_fund_params* p)
{
    p->method = VO_FUND_MSAC; p->num_trials = 500; p->distance_threshold = 0.01; p->confidence = 99.0; p->seed = 0x5EED;
}
void vo_default_klt_params(vo_klt_params* p)
{
    p->num_pyramid_levels = 3; p->block_size[0] = 31; p->block_size[1] = 31; p->max_iterations = 30;
    p->max_bidirectional_error = vo_u32_as_f32(0x7f800000u);
}
void vo_default_corner_params(vo_corner_params* p)
{
    p->method = VO_CORNER_MINEIG; p->filter_size = 5; p->min_quality = 0.01f; p->strongest = 0;
    for (int k = 0; k < 4; ++k) p->roi[k] = 0;
}
void vo_default_sgm_params(vo_sgm_params* p)
{
    p->disparity_range[0] = 0; p->disparity_range[1] = 128; p->uniqueness_threshold = 15; p->p1 = 10; p->p2 = 120;
}

const char* vo_last_error(const vo_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

void* vo_stream(vo_ctx* c) { return c ? (void*)c->stream : nullptr; }

// a set's job table: [0, M) stereo; [M, 5M) the four tracking steps (M = max_batch)
static int job_stereo(const vo_ctx*, int f) { return f; }
static int job_track(const vo_ctx* c, int step, int f) { return c->max_batch + step * c->max_batch + f; }
static int job_count(const vo_ctx* c) { return 5 * c->max_batch; }

// Buffer set k: its buffers, its job table (job_stereo / job_track) and its two events.  -> 0 or the
// runtime's error code, *what naming the step (the pool keeps whatever was made).
static int set_create(vo_ctx* c, int k, const char** what)
{
    vo_ctx::BufferSet& S = c->set[k];
    DevPool& pool = c->pool;
    const int M = c->max_batch, K = c->sp.max_keypoints, pair_slots = M + 1, n_jobs = job_count(c);
    int e;
    *what = "event";
    if ((e = pool.event(S.ev_done)) || (e = pool.event(S.ev_arena))) return e;
    *what = "sift buffers";
    if ((e = sift_alloc(pool, S.sb, c->py, K, 4 * K))) return e;
    *what = "match buffers";
    if ((e = match_alloc(pool, S.mb, M, K))) return e;
    *what = "jobs";
    if ((e = pool.alloc(S.d_jobs, n_jobs))) return e;
    *what = "pairs";
    if ((e = pool.group({DevPool::req(S.pair_i, (size_t)pair_slots * K), DevPool::req(S.pair_j, (size_t)pair_slots * K),
                         DevPool::req(S.pair_n, pair_slots)}))) return e;
    if ((e = hipMemset(S.pair_n, 0, sizeof(int) * pair_slots))) return e;
    *what = "geometry buffers";
    if ((e = geom_alloc(pool, S.gb, M, K, c->rp.max_num_trials))) return e;
    std::vector<MatchJob> jobs(n_jobs);
    memset(jobs.data(), 0, sizeof(MatchJob) * n_jobs);
    const size_t dstride = (size_t)K * VO_DESC_LEN;
    for (int f = 0; f < M; ++f) {
        MatchJob& J = jobs[job_stereo(c, f)];
        const int il = 2 * f, ir = 2 * f + 1;
        J.d1 = S.sb.desc + il * dstride; J.m1 = S.sb.meta + (size_t)il * K; J.idx1 = nullptr; J.n1 = S.sb.n_kp + il;
        J.d2 = S.sb.desc + ir * dstride; J.m2 = S.sb.meta + (size_t)ir * K; J.idx2 = nullptr; J.n2 = S.sb.n_kp + ir;
        J.out_i = S.pair_i + (size_t)f * K; J.out_j = S.pair_j + (size_t)f * K; J.out_n = S.pair_n + f;
        J.cap = K;
    }
    geom_fill_track_jobs(S.gb, jobs.data(), M, job_track(c, 0, 0), S.sb, S.pair_i, S.pair_j, S.pair_n, K);
    *what = "jobs copy";
    return hipMemcpy(S.d_jobs, jobs.data(), sizeof(MatchJob) * n_jobs, hipMemcpyHostToDevice);
}

// vo_create's streams, events and buffers.  -> 0 or the runtime's error code, `what` naming the step.
static int create_resources(vo_ctx* c, std::string& what)
{
    DevPool& pool = c->pool;
    const int max_batch = c->max_batch, kp_cap = c->sp.max_keypoints;
    int e;
    what = "stream";
    if ((e = pool.stream(c->stream))) return e;
    for (int k = 0; k < vo_ctx::MAX_SUB; ++k) {
        // every stream at the default priority: the forked SIFT streams must not rank below the
        // geometry / copy streams of the pipelined loop body (at the lowest priority the full
        // per-frame path dropped from 7.3 k to 5.4 k stereo frames/s), and the scale-space stream
        // at the highest priority measured within noise.  No CU masks: with masks that bind
        // (contiguous CU ranges), every split of the CUs between the two streams was 9-38 %
        // slower -- both streams are bound per CU and need the whole chip
        if ((e = pool.stream(c->sub[k]))) return e;
        what = "event";
        if ((e = pool.event(c->ev_join[k])) || (e = pool.event(c->ev_o0[k])) || (e = pool.event(c->ev_down[k])) ||
            (e = pool.event(c->ev_top[k]))) return e;
        what = "stream";
    }
    // (the down stream at the lowest / highest priority, forked after octave 0: 1-3 % slower than at
    // the default)
    if ((e = pool.stream(c->down)) || (e = pool.stream(c->copy_stream))) return e;
    what = "event";
    if ((e = pool.event(c->ev_fork))) return e;
    build_pyramid_geometry(c->py, c->rows, c->cols, 2 * max_batch + 2, c->sp);
    what = "pyramid";
    if ((e = pool.alloc(c->d_py, 1))) return e;
    what = "pyramid copy";
    if ((e = hipMemcpy(c->d_py, &c->py, sizeof(Pyramid), hipMemcpyHostToDevice))) return e;
    for (int k = 0; k < 2; ++k) {
        const char* step = "";
        if ((e = set_create(c, k, &step))) { what = std::string(step) + (k ? " (set 1)" : ""); return e; }
    }
    what = "staging";
    if ((e = pool.alloc(c->d_img, (size_t)2 * max_batch * c->rows * c->cols))) return e;
    for (int k = 0; k < 2; ++k)
        if ((e = pool.alloc(c->d_fd[k], (size_t)kp_cap * VO_DESC_LEN)) || (e = pool.alloc(c->d_fm[k], kp_cap)) ||
            (e = pool.alloc(c->d_ff[k], (size_t)kp_cap * VO_DESC_LEN))) return e;
    if ((e = pool.alloc(c->d_fn, 2)) || (e = pool.alloc(c->d_bad, 1)) || (e = pool.alloc(c->d_mi, kp_cap)) ||
        (e = pool.alloc(c->d_mj, kp_cap)) || (e = pool.alloc(c->d_mn, 1))) return e;
    {   // vo_match's job: the two staged descriptor sets (match_ex_buffers builds the exchanged one)
        MatchJob J;
        memset(&J, 0, sizeof(J));
        J.d1 = c->d_fd[0]; J.m1 = c->d_fm[0]; J.idx1 = nullptr; J.n1 = c->d_fn;
        J.d2 = c->d_fd[1]; J.m2 = c->d_fm[1]; J.idx2 = nullptr; J.n2 = c->d_fn + 1;
        J.out_i = c->d_mi; J.out_j = c->d_mj; J.out_n = c->d_mn; J.cap = kp_cap;
        what = "jobs";
        if ((e = pool.alloc(c->d_job_single, 1))) return e;
        what = "jobs copy";
        if ((e = hipMemcpy(c->d_job_single, &J, sizeof(MatchJob), hipMemcpyHostToDevice))) return e;
    }
    const size_t F = max_batch, R = F * kp_cap;          // frames and landmark rows of a batch
    for (int k = 0; k < VO_STEP_DEPTH; ++k) {
        vo_ctx::StepHost& H = c->sh[k];
        what = "event";
        if ((e = pool.event(H.ev))) return e;
        what = "packed rows";
        if ((e = pool.alloc(H.d_pX, 3 * R)) || (e = pool.alloc(H.d_pkeep, R))) return e;
        what = "pinned";
        if ((e = pool.pinned(H.fg, F)) || (e = pool.pinned(H.nkp, 2 * F)) || (e = pool.pinned(H.ncand, 2 * F)) ||
            (e = pool.pinned(H.ndet, 2 * F)) || (e = pool.pinned(H.np, F)) || (e = pool.pinned(H.rows, F)) ||
            (e = pool.pinned(H.pX, 3 * R)) || (e = pool.pinned(H.pkeep, R))) return e;
    }
    return 0;
}

vo_ctx* vo_create(int device, int rows, int cols, int max_batch, const vo_calib* calib, const vo_sift_params* sift,
                  const vo_match_params* match, const vo_ransac_params* ransac)
{
    if (rows < 16 || cols < 16 || rows > 2048 || cols > 2048 || max_batch < 1 || max_batch > VO_MAX_BATCH) {
        fail(nullptr, VO_ERR_ARG, "vo_create: bad size rows=%d cols=%d max_batch=%d", rows, cols, max_batch);
        return nullptr;
    }
    {   // the parameter block, like the size, is checked before any HIP call
        vo_sift_params sp;
        if (sift) sp = *sift; else vo_default_sift_params(&sp);
        if (const char* field = sift_params_refusal(sp)) {
            fail(nullptr, VO_ERR_ARG, "vo_create: unsupported sift params: %s (n_octave_layers=%d sigma=%g contrast_threshold=%g "
                 "edge_threshold=%g upsample=%d max_keypoints=%d)", field, sp.n_octave_layers, (double)sp.sigma,
                 (double)sp.contrast_threshold, (double)sp.edge_threshold, sp.upsample, sp.max_keypoints);
            return nullptr;
        }
    }
    if (hipSetDevice(device) != hipSuccess) { fail(nullptr, VO_ERR_HIP, "hipSetDevice(%d) failed", device); return nullptr; }
    vo_ctx* c = new vo_ctx();
    c->device = device; c->rows = rows; c->cols = cols; c->max_batch = max_batch;
    if (sift) c->sp = *sift; else vo_default_sift_params(&c->sp);
    if (match) c->mp = *match; else vo_default_match_params(&c->mp);
    if (ransac) c->rp = *ransac; else vo_default_ransac_params(&c->rp);
    if (calib) { c->calib = *calib; c->has_calib = true; }
    memcpy(c->pose, I4, sizeof(I4));
    std::string what;
    const int e = create_resources(c, what);
    if (e) {                                            // the context's pool frees what was made so far
        fail(nullptr, VO_ERR_HIP, "vo_create: %s: %s", what.c_str(), hipGetErrorString((hipError_t)e));
        delete c;
        return nullptr;
    }
    return c;
}

void vo_destroy(vo_ctx* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (g_prof == &c->prof) g_prof = nullptr;
    delete c;                                           // the pool: memory, then events, then streams
}

int vo_set_concurrency(vo_ctx* c, int n_streams)
{
    if (!c || n_streams < 1 || n_streams > vo_ctx::MAX_SUB) return VO_ERR_ARG;
    c->n_sub = n_streams;
    return VO_OK;
}

int vo_set_calib(vo_ctx* c, const vo_calib* calib)
{
    if (!c || !calib) return VO_ERR_ARG;
    c->calib = *calib;
    c->has_calib = true;
    return VO_OK;
}

int vo_set_profiling(vo_ctx* c, int enable)
{
    if (!c) return VO_ERR_ARG;
    c->prof.on = enable != 0;
    c->prof.reset_totals();
    return VO_OK;
}

// the sticky error of the launches enqueued so far
static int launch_status(vo_ctx* c)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? VO_OK : fail(c, VO_ERR_HIP, "launch: %s", hipGetErrorString(e));
}

// Synchronise the stream, collect profiling, translate errors.
static int finish(vo_ctx* c)
{
    hipError_t e = hipStreamSynchronize(c->stream);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipStreamSynchronize(c->sub[k]);
    if (e == hipSuccess) e = hipStreamSynchronize(c->down);
    if (e != hipSuccess) return fail(c, VO_ERR_HIP, "stream sync: %s", hipGetErrorString(e));
    const int rc = launch_status(c);
    if (rc) return rc;
    if (c->prof.on) c->prof.collect();
    return VO_OK;
}

// One entry's call on the context, constructed at its top: selects the device; refuses (status)
// while step batches are pending unless the entry is the step pipeline's own (the others reuse
// buffer set 0); points this thread's g_prof at the context's profiler while profiling is on, until
// the entry returns by whatever path; and with quiesce, makes `stream` -- on which such calls run
// over the context's own buffers -- wait for any batch still in flight on either buffer set (no
// host synchronisation).
struct CallScope {
    int status = VO_OK;
    explicit CallScope(vo_ctx* c, bool quiesce = true, bool step = false)
    {
        hipSetDevice(c->device);
        if (!step && !c->pending.empty()) {
            status = fail(c, VO_ERR_STATE, "asynchronous step batches pending (vo_step_collect first)");
            return;
        }
        g_prof = c->prof.on ? &c->prof : nullptr;
        if (quiesce)
            for (int k = 0; k < 2; ++k) hipStreamWaitEvent(c->stream, c->set[k].ev_done, 0);
    }
    ~CallScope() { g_prof = nullptr; }
    CallScope(const CallScope&) = delete;
};

int vo_kernel_times(vo_ctx* c, const char** names, double* ms, int* calls, int capacity, int* n)
{
    if (!c) return VO_ERR_ARG;
    hipSetDevice(c->device);
    if (c->prof.on) {                                  // asynchronous calls may still be in flight
        int rc = finish(c);
        if (rc) return rc;
    }
    int m = (int)c->prof.names.size();
    if (n) *n = m;
    for (int i = 0; i < m && i < capacity; ++i) {
        if (names) names[i] = c->prof.names[i].c_str();
        if (ms) ms[i] = c->prof.ms[i];
        if (calls) calls[i] = c->prof.calls[i];
    }
    return VO_OK;
}

// MATLAB images are column-major: pixel (r, c) of image n at src[n * ld * cols + c * ld + r]
// (ld >= rows).  32 x 32 LDS tile transpose into tightly packed row-major frames.
__global__ __launch_bounds__(256) void k_cm_to_rm_u8(const uint8_t* __restrict__ src, int ld, int rows, int cols,
                                                     uint8_t* __restrict__ dst)
{
    __shared__ uint8_t t[32][33];
    const int n = blockIdx.z, r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const uint8_t* s = src + (size_t)n * ld * cols;
    uint8_t* d = dst + (size_t)n * rows * cols;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k, r = r0 + tx;                  // lanes walk a source column (contiguous)
        if (c < cols && r < rows) t[k][tx] = s[(size_t)c * ld + r];
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int r = r0 + k, c = c0 + tx;                  // lanes walk a destination row
        if (r < rows && c < cols) d[(size_t)r * cols + c] = t[tx][k];
    }
}

// host images -> tightly packed row-major device frames at dst (n frames).  col_major: the
// buffer as MATLAB holds it (copied as it lies into the context's column-major staging, then
// transposed on the device).
static int stage_images(vo_ctx* c, const uint8_t* img, int ld, int col_major, int n, uint8_t* dst)
{
    const int rows = c->rows, cols = c->cols;
    if (!col_major) {
        HIPC(c, hipMemcpy2DAsync(dst, cols, img, ld, cols, (size_t)rows * n, hipMemcpyHostToDevice, c->stream));
        return VO_OK;
    }
    // exactly the bytes the frames span: the last column of the last frame ends `rows` bytes
    // into its ld-byte slot (a padded view, ld > rows, must not be read past its end)
    const size_t need = (size_t)ld * ((size_t)cols * n - 1) + rows;
    if (need > c->cm_cap) {
        HIPC(c, hipStreamSynchronize(c->stream));       // the old staging's last reader
        HIPC(c, (hipError_t)c->pool.grow({DevPool::req(c->d_cm, need)}));
        c->cm_cap = need;
    }
    HIPC(c, hipMemcpyAsync(c->d_cm, img, need, hipMemcpyHostToDevice, c->stream));
    VO_LAUNCH(k_cm_to_rm_u8, dim3((rows + 31) / 32, (cols + 31) / 32, n), dim3(256), 0, c->stream, c->d_cm, ld, rows, cols, dst);
    return VO_OK;
}

int vo_sift_ex(vo_ctx* c, const uint8_t* img, int rows, int cols, int ld, int col_major, vo_keypoint* kps, uint8_t* desc,
               int capacity, int* n_out)
{
    if (!c || !img || rows != c->rows || cols != c->cols || (col_major != 0 && col_major != 1) ||
        ld < (col_major ? rows : cols))
        return fail(c, VO_ERR_ARG, "vo_sift: bad arguments");
    CallScope call(c); if (call.status) return call.status;
    int rc_stage = stage_images(c, img, ld, col_major, 1, c->d_img);
    if (rc_stage) return rc_stage;
    ImageSrc src{c->d_img, c->d_img, (size_t)rows * cols, cols, 0};
    sift_enqueue(c->py, c->set[0].sb, src, 1, c->sp, c->stream, c->d_py, c->strongest);
    c->last_set = 0;                                   // vo_fetch_* now read this result (set 0)
    c->set[0].sel_used = c->strongest > 0;
    c->described = false;
    int n = 0, n_cand = 0, n_det = -1;
    HIPC(c, hipMemcpyAsync(&n, c->set[0].sb.n_kp, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (c->strongest > 0) HIPC(c, hipMemcpyAsync(&n_det, c->set[0].sb.n_det, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(&n_cand, c->set[0].sb.n_cand, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    int rc = finish(c);
    if (rc) return rc;
    if (n_out) *n_out = n;
    int m = std::min(std::min(n, c->set[0].sb.kp_cap), capacity);
    if (m > 0) {
        if (kps) HIPC(c, hipMemcpy(kps, c->set[0].sb.kp, sizeof(vo_keypoint) * m, hipMemcpyDeviceToHost));
        if (desc) HIPC(c, hipMemcpy(desc, c->set[0].sb.desc, (size_t)m * VO_DESC_LEN, hipMemcpyDeviceToHost));
    }
    if (n_cand > c->set[0].sb.cand_cap)
        return fail(c, VO_ERR_CAPACITY, "vo_sift: %d extremum candidates exceed the candidate list (%d = 4 x max_keypoints)",
                    n_cand, c->set[0].sb.cand_cap);
    if (n_det < 0) n_det = n;                          // selection off: the detected count
    if (n_det > c->set[0].sb.kp_cap)
        return fail(c, VO_ERR_CAPACITY, "vo_sift: %d keypoints exceed max_keypoints %d", n_det, c->set[0].sb.kp_cap);
    if (n > capacity) return fail(c, VO_ERR_CAPACITY, "vo_sift: %d keypoints exceed capacity %d", n, capacity);
    return VO_OK;
}

int vo_sift(vo_ctx* c, const uint8_t* img, int rows, int cols, int ld, vo_keypoint* kps, uint8_t* desc, int capacity,
            int* n_out)
{
    return vo_sift_ex(c, img, rows, cols, ld, 0, kps, desc, capacity, n_out);
}

// ---- extractFeatures at caller-given points (vo.h: "Spec") -----------------------------------
// nullptr when q is a point vo_describe accepts, else the rule it breaks.  Host arithmetic only; the
// radius is desc_tables' own float expression (this file is compiled with -ffp-contract=off too),
// compared as a float so that no scale overflows the conversion.
static const char* point_refusal(const vo_sift_params& p, int n_oct, const vo_keypoint& q)
{
    if (!std::isfinite(q.x) || !std::isfinite(q.y) || !std::isfinite(q.scale) || !std::isfinite(q.angle))
        return "x, y, scale and angle must be finite";
    if (!(std::fabs(q.x) < 1048576.0f) || !(std::fabs(q.y) < 1048576.0f)) return "|x|, |y| must be below 2^20";
    if (!(q.angle >= 0.0f && q.angle <= 360.0f)) return "angle outside [0, 360]";
    const int up = p.upsample ? 1 : 0;
    if (q.octave < -up || q.octave >= n_oct - up) return "octave outside the pyramid";
    if (q.layer < 0 || q.layer > p.n_octave_layers + 2) return "layer outside 0 .. n_octave_layers + 2";
    const float oscale = (float)(1 << (q.octave + up)) * (up ? 0.5f : 1.0f);
    const float scl = q.scale / oscale;
    const float hist_width = VO_SIFT_DESCR_SCL * scl;
    const float r = rintf(hist_width * 1.4142135623730951f * (float)(VO_SIFT_DESCR_W + 1) * 0.5f);
    if (!(r >= 1.0f && r <= (float)VO_SIFT_DESCR_RMAX)) return "scale gives a descriptor window radius outside 1 .. 127";
    return nullptr;
}

int vo_check_points(const vo_sift_params* p, int rows, int cols, const vo_keypoint* pts, int n, int* first_bad)
{
    if (first_bad) *first_bad = -1;
    if (!p || rows < 1 || cols < 1 || n < 0 || (n > 0 && !pts) || p->n_octave_layers < 1 || p->n_octave_layers > 5)
        return VO_ERR_ARG;
    const int n_oct = vo_num_octaves(rows, cols, p->upsample);
    for (int i = 0; i < n; ++i)
        if (point_refusal(*p, n_oct, pts[i])) {
            if (first_bad) *first_bad = i;
            return VO_ERR_ARG;
        }
    return VO_OK;
}

int vo_describe_batch(vo_ctx* c, const uint8_t* imgs, int ld, int col_major, int n_img, const vo_keypoint* pts,
                      const int32_t* n_pts, int pts_stride, uint8_t* desc)
{
    if (!c || !imgs || !n_pts || n_img < 1 || n_img > 2 * c->max_batch || pts_stride < 0 ||
        (col_major != 0 && col_major != 1) || ld < (col_major ? c->rows : c->cols))
        return fail(c, VO_ERR_ARG, "vo_describe: bad arguments");
    // every refusal before anything is enqueued
    if (!c->pending.empty()) return fail(c, VO_ERR_STATE, "asynchronous step batches pending (vo_step_collect first)");
    const int K = c->set[0].sb.kp_cap;
    long total = 0;
    int max_n = 0;
    for (int i = 0; i < n_img; ++i) {
        if (n_pts[i] < 0 || n_pts[i] > pts_stride)
            return fail(c, VO_ERR_ARG, "vo_describe: image %d has %d points, outside 0 .. pts_stride = %d", i, n_pts[i], pts_stride);
        if (n_pts[i] > K)
            return fail(c, VO_ERR_CAPACITY, "vo_describe: image %d has %d points, more than max_keypoints %d", i, n_pts[i], K);
        total += n_pts[i];
        max_n = std::max(max_n, n_pts[i]);
    }
    if (total > 0 && (!pts || !desc)) return fail(c, VO_ERR_ARG, "vo_describe: bad arguments");
    for (int i = 0; i < n_img; ++i)
        for (int k = 0; k < n_pts[i]; ++k) {
            const char* why = point_refusal(c->sp, c->py.n_oct, pts[(size_t)i * pts_stride + k]);
            if (why) return fail(c, VO_ERR_ARG, "vo_describe: image %d point %d: %s", i, k, why);
        }
    if (total == 0) return VO_OK;                      // nothing to describe: nothing is launched
    CallScope call(c); if (call.status) return call.status;
    // tightly packed row-major images are one contiguous block: one copy (a 2-D copy of a pageable
    // buffer goes row by row -- 1.4 s for 512 images of 375 x 1242, profiles/describe_times.txt)
    if (!col_major && ld == c->cols) {
        HIPC(c, hipMemcpyAsync(c->d_img, imgs, (size_t)c->rows * c->cols * n_img, hipMemcpyHostToDevice, c->stream));
    } else {
        int rc = stage_images(c, imgs, ld, col_major, n_img, c->d_img);
        if (rc) return rc;
    }
    // the points and their counts into the keypoint rows the detecting entries write (set 0)
    HIPC(c, hipMemcpy2DAsync(c->set[0].sb.kp, sizeof(vo_keypoint) * K, pts, sizeof(vo_keypoint) * pts_stride,
                             sizeof(vo_keypoint) * max_n, n_img, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->set[0].sb.n_kp, n_pts, sizeof(int) * n_img, hipMemcpyHostToDevice, c->stream));
    // consecutive images: slot i = (i & 1 ? right : left) + (i >> 1) * frame_stride
    const size_t fs = (size_t)c->rows * c->cols;
    ImageSrc src{c->d_img, c->d_img + fs, 2 * fs, c->cols, 0};
    sift_enqueue_describe(c->py, c->set[0].sb, src, n_img, (int)std::min<long>(total, INT_MAX), c->sp, c->stream, c->d_py);
    c->last_set = 0;                                   // vo_fetch_gaussian now reads this scale space (set 0)
    c->set[0].sel_used = false;
    c->described = true;                               // ... and the fetches of a detecting call have nothing to read
    // row i of image k for point i: full rows-of-stride copies where every image fills its stride
    // (one image always does), else image by image, leaving the rows beyond n_pts[i] untouched
    bool full = true;
    for (int i = 0; i < n_img; ++i) full = full && n_pts[i] == pts_stride;
    if (full) {
        HIPC(c, hipMemcpy2DAsync(desc, (size_t)pts_stride * VO_DESC_LEN, c->set[0].sb.desc, (size_t)K * VO_DESC_LEN,
                                 (size_t)pts_stride * VO_DESC_LEN, n_img, hipMemcpyDeviceToHost, c->stream));
    } else {
        for (int i = 0; i < n_img; ++i)
            if (n_pts[i] > 0)
                HIPC(c, hipMemcpyAsync(desc + (size_t)i * pts_stride * VO_DESC_LEN, c->set[0].sb.desc + (size_t)i * K * VO_DESC_LEN,
                                       (size_t)n_pts[i] * VO_DESC_LEN, hipMemcpyDeviceToHost, c->stream));
    }
    return finish(c);
}

int vo_describe(vo_ctx* c, const uint8_t* img, int rows, int cols, int ld, int col_major, const vo_keypoint* pts, int n,
                uint8_t* desc)
{
    if (!c || rows != c->rows || cols != c->cols || n < 0) return fail(c, VO_ERR_ARG, "vo_describe: bad arguments");
    const int32_t cnt = n;
    return vo_describe_batch(c, img, ld, col_major, 1, pts, &cnt, n, desc);
}

// ---- undistortImage (VO.m:75-76) -------------------------------------------------------------
// vo_distortion -> the kernel's camera block; false for a non-finite entry, fx or fy zero, a
// K[1][0] the model has no term for, or a last row other than 0 0 1.  *trivial: all five
// coefficients zero (the remap is the identity on u8 frames, kitti.undistort_identity).
static bool distortion_cam(const vo_distortion* d, vo_bc_cam* m, bool* trivial)
{
    for (int k = 0; k < 9; ++k) if (!std::isfinite(d->K[k])) return false;
    for (int k = 0; k < 3; ++k) if (!std::isfinite(d->radial[k])) return false;
    for (int k = 0; k < 2; ++k) if (!std::isfinite(d->tangential[k])) return false;
    if (d->K[0] == 0.0 || d->K[4] == 0.0 || d->K[3] != 0.0 || d->K[6] != 0.0 || d->K[7] != 0.0 || d->K[8] != 1.0) return false;
    m->fx = d->K[0]; m->s = d->K[1]; m->cx = d->K[2]; m->fy = d->K[4]; m->cy = d->K[5];
    m->k1 = d->radial[0]; m->k2 = d->radial[1]; m->k3 = d->radial[2];
    m->p1 = d->tangential[0]; m->p2 = d->tangential[1];
    *trivial = m->k1 == 0.0 && m->k2 == 0.0 && m->k3 == 0.0 && m->p1 == 0.0 && m->p2 == 0.0;
    return true;
}

int vo_undistort(vo_ctx* c, const uint8_t* img, int rows, int cols, int ld, int col_major, const vo_distortion* d,
                 uint8_t* out, int ld_out)
{
    if (!c || !img || !out || !d || rows != c->rows || cols != c->cols || (col_major != 0 && col_major != 1) ||
        ld < (col_major ? rows : cols) || ld_out < (col_major ? rows : cols))
        return fail(c, VO_ERR_ARG, "vo_undistort: bad arguments");
    UndistortSide S;
    bool trivial = false;
    if (!distortion_cam(d, &S.cam, &trivial))
        return fail(c, VO_ERR_ARG, "vo_undistort: intrinsics must be finite with fx, fy != 0, K[1][0] = 0 and a last row 0 0 1");
    CallScope call(c); if (call.status) return call.status;
    // staging frame 0 = the image (row-major), frame 1 = the result
    const size_t fs = (size_t)rows * cols;
    int rc = stage_images(c, img, ld, col_major, 1, c->d_img);
    if (rc) return rc;
    S.in = c->d_img; S.out = c->d_img + fs; S.copy = 0; S.pad = 0;
    undistort_launch(&S, 1, rows, cols, 1, fs, fs, c->stream);
    if (!col_major) {
        HIPC(c, hipMemcpy2DAsync(out, ld_out, S.out, cols, cols, rows, hipMemcpyDeviceToHost, c->stream));
    } else {
        // back to MATLAB's storage: the row-major result read as a column-major cols x rows
        // matrix is transposed into the column-major staging (which held the input: >= rows * cols)
        VO_LAUNCH(k_cm_to_rm_u8, dim3((cols + 31) / 32, (rows + 31) / 32, 1), dim3(256), 0, c->stream, S.out, cols, cols, rows,
                  c->d_cm);
        HIPC(c, hipMemcpy2DAsync(out, ld_out, c->d_cm, rows, rows, cols, hipMemcpyDeviceToHost, c->stream));
    }
    return finish(c);
}

int vo_undistort_batch_dev(vo_ctx* c, const uint8_t* d_in, int B, const vo_distortion* d, uint8_t* d_out)
{
    if (!c || !d_in || !d_out || !d || B < 1 || B > (1 << 19))
        return fail(c, VO_ERR_ARG, "vo_undistort_batch_dev: bad arguments");
    const size_t fs = (size_t)c->rows * c->cols;
    const uintptr_t pi = reinterpret_cast<uintptr_t>(d_in), po = reinterpret_cast<uintptr_t>(d_out);
    if (po < pi + fs * B && pi < po + fs * B)
        return fail(c, VO_ERR_ARG, "vo_undistort_batch_dev: d_out overlaps d_in");
    UndistortSide S;
    bool trivial = false;
    if (!distortion_cam(d, &S.cam, &trivial))
        return fail(c, VO_ERR_ARG, "vo_undistort_batch_dev: intrinsics must be finite with fx, fy != 0, K[1][0] = 0 and a last row 0 0 1");
    CallScope call(c, false); if (call.status) return call.status;
    S.in = d_in; S.out = d_out; S.copy = 0; S.pad = 0;
    undistort_launch(&S, 1, c->rows, c->cols, B, fs, fs, c->stream);
    return launch_status(c);                            // profiling events are collected by vo_kernel_times
}

int vo_set_distortion(vo_ctx* c, const vo_distortion* left, const vo_distortion* right)
{
    if (!c) return VO_ERR_ARG;
    if (!c->pending.empty()) return fail(c, VO_ERR_STATE, "vo_set_distortion: step batches pending (vo_step_collect first)");
    const vo_distortion* d[2] = {left, right};
    vo_bc_cam cam[2];
    bool on[2] = {false, false};
    for (int k = 0; k < 2; ++k) {
        if (!d[k]) continue;
        bool trivial = false;
        if (!distortion_cam(d[k], &cam[k], &trivial))
            return fail(c, VO_ERR_ARG, "vo_set_distortion: %s intrinsics must be finite with fx, fy != 0, K[1][0] = 0 and a last row 0 0 1",
                        k ? "right" : "left");
        on[k] = !trivial;
    }
    if ((on[0] || on[1]) && !c->d_rect) {
        hipSetDevice(c->device);
        HIPC(c, (hipError_t)c->pool.alloc(c->d_rect, (size_t)2 * c->max_batch * c->rows * c->cols));
    }
    for (int k = 0; k < 2; ++k) {
        c->ud_on[k] = on[k];
        if (on[k]) c->ud_cam[k] = cam[k];
    }
    c->rect_B = 0;
    return VO_OK;
}

int vo_fetch_rectified(vo_ctx* c, int image, uint8_t* out, int capacity)
{
    if (!c || !out) return fail(c, VO_ERR_ARG, "vo_fetch_rectified: bad arguments");
    if (!c->ud_on[0] && !c->ud_on[1]) return fail(c, VO_ERR_STATE, "vo_fetch_rectified: no distortion set (vo_set_distortion)");
    if (image < 0 || image >= 2 * c->rect_B) return fail(c, VO_ERR_ARG, "vo_fetch_rectified: image %d not in the last batched call", image);
    const size_t fs = (size_t)c->rows * c->cols;
    if (capacity < 0 || (size_t)capacity < fs) return fail(c, VO_ERR_CAPACITY, "vo_fetch_rectified: capacity %d < %zu", capacity, fs);
    hipSetDevice(c->device);
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipEventSynchronize(c->set[c->last_set].ev_done));
    const uint8_t* src = c->d_rect + ((size_t)(image & 1) * c->max_batch + (image >> 1)) * fs;
    HIPC(c, hipMemcpy(out, src, fs, hipMemcpyDeviceToHost));
    return VO_OK;
}

// The vo_fetch_* entries' shared start: wait for the last call's results, then pick the buffer set
// that holds image slot `image`.  Image slots below 2 * max_batch (and the frames' pair slots with
// them) are read from the last call's set (last_set: either set holds whole batches); the two carry
// slots, 2 * max_batch and 2 * max_batch + 1, always from set 0.  detections: the entry `who` reads
// what a detecting call left, which vo_describe does not leave.
static int fetch_set(vo_ctx* c, int image, const char* who, bool detections, vo_ctx::BufferSet** S)
{
    if (detections && c->described)
        return fail(c, VO_ERR_STATE, "%s: the last call described given points and detected nothing", who);
    hipSetDevice(c->device);
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipEventSynchronize(c->set[c->last_set].ev_done));
    *S = &c->set[image < 2 * c->max_batch ? c->last_set : 0];
    return VO_OK;
}

// m accepted pairs from two device index arrays as rows of 1-based (i, j)
static int read_pairs(vo_ctx* c, const int* d_i, const int* d_j, int m, uint32_t* pairs)
{
    if (m <= 0 || !pairs) return VO_OK;
    std::vector<int> ii(m), jj(m);
    HIPC(c, hipMemcpy(ii.data(), d_i, sizeof(int) * m, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(jj.data(), d_j, sizeof(int) * m, hipMemcpyDeviceToHost));
    for (int k = 0; k < m; ++k) { pairs[2 * k] = (uint32_t)ii[k] + 1; pairs[2 * k + 1] = (uint32_t)jj[k] + 1; }
    return VO_OK;
}

// ---- SIFTPoints.selectStrongest (VO.m:140, 206, 217-218: "limit the number of points kept") ----
int vo_set_strongest(vo_ctx* c, int n)
{
    if (!c) return VO_ERR_ARG;
    if (n < 0 || n > c->sp.max_keypoints)
        return fail(c, VO_ERR_ARG, "vo_set_strongest: n = %d outside 0 (off) .. max_keypoints = %d", n, c->sp.max_keypoints);
    if (!c->pending.empty()) return fail(c, VO_ERR_STATE, "vo_set_strongest: step batches pending (vo_step_collect first)");
    if (n > 0) {
        hipSetDevice(c->device);
        for (int k = 0; k < 2; ++k) HIPC(c, sift_alloc_select(c->pool, c->set[k].sb));
    }
    c->strongest = n;
    return VO_OK;
}

int vo_fetch_detected_count(vo_ctx* c, int image, int* n_detected)
{
    if (!c || image < 0 || image >= c->set[0].sb.n_img) return fail(c, VO_ERR_ARG, "vo_fetch_detected_count: bad image");
    vo_ctx::BufferSet* S = nullptr;
    int rc = fetch_set(c, image, "vo_fetch_detected_count", true, &S);
    if (rc) return rc;
    int cnt = 0;
    HIPC(c, hipMemcpy(&cnt, (S->sel_used ? S->sb.n_det : S->sb.n_kp) + image, sizeof(int), hipMemcpyDeviceToHost));
    if (n_detected) *n_detected = cnt;
    return VO_OK;
}

// ---- matchFeatures; with options: explicit thresholds, matchMetric, Unique --------------------
// opts == NULL: the context's parameters, unique 0
static int match_opts_resolve(vo_ctx* c, const vo_match_opts* o, vo_match_params* p, int* unique, const char* who)
{
    *p = c->mp;
    *unique = 0;
    if (!o) return VO_OK;
    if (!(o->match_threshold > 0.0f && o->match_threshold <= 25.0f))
        return fail(c, VO_ERR_ARG, "%s: MatchThreshold %g outside (0, 25]", who, (double)o->match_threshold);
    if (!(o->max_ratio > 0.0f && o->max_ratio <= 1.0f))
        return fail(c, VO_ERR_ARG, "%s: MaxRatio %g outside (0, 1]", who, (double)o->max_ratio);
    if ((o->unique != 0 && o->unique != 1) || o->reserved != 0)
        return fail(c, VO_ERR_ARG, "%s: unique must be 0 or 1 and reserved 0", who);
    p->match_threshold = o->match_threshold;
    p->max_ratio = o->max_ratio;
    *unique = o->unique;
    return VO_OK;
}

// what the entries with options need beyond vo_match's buffers, at the first such call
static int match_ex_buffers(vo_ctx* c, const char* who)
{
    if (c->mx.job_back) return VO_OK;
    MatchJob J;                                          // the vo_match job with its sides exchanged
    memset(&J, 0, sizeof(J));
    J.d1 = c->d_fd[1]; J.m1 = c->d_fm[1]; J.n1 = c->d_fn + 1;
    J.d2 = c->d_fd[0]; J.m2 = c->d_fm[0]; J.n2 = c->d_fn;
    const hipError_t e = match_ex_alloc(c->pool, c->mx, c->set[0].mb, J);
    if (e != hipSuccess) return fail(c, VO_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return VO_OK;
}

// matchFeatures on the two staged descriptor sets d_fd[0] (n1 rows) / d_fd[1] (n2 rows), inside a
// call.  ex: the entry with options (parameters p, unique, the pairs' metric); else the context's
// parameters through the hot path's match_launch.
static int match_staged(vo_ctx* c, int n1, int n2, bool ex, const vo_match_params& p, int unique, uint32_t* pairs,
                        float* metric, int capacity, int* n_pairs, const char* who)
{
    int rc = ex ? match_ex_buffers(c, who) : VO_OK;
    if (rc) return rc;
    int nn[2] = {n1, n2};
    HIPC(c, hipMemcpyAsync(c->d_fn, nn, sizeof(nn), hipMemcpyHostToDevice, c->stream));
    desc_meta_launch(c->d_fd[0], c->d_fm[0], n1, c->stream);
    desc_meta_launch(c->d_fd[1], c->d_fm[1], n2, c->stream);
    if (ex) match_launch_ex(c->set[0].mb, c->d_job_single, c->mx, p, unique, c->stream);
    else match_launch(c->set[0].mb, c->d_job_single, 1, c->mp, c->stream);
    int P = 0;
    HIPC(c, hipMemcpyAsync(&P, c->d_mn, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    rc = finish(c);
    if (rc) return rc;
    if (n_pairs) *n_pairs = P;
    const int m = std::min(P, capacity);
    if ((rc = read_pairs(c, c->d_mi, c->d_mj, m, pairs))) return rc;
    if (ex && m > 0 && metric) HIPC(c, hipMemcpy(metric, c->mx.metric, sizeof(float) * m, hipMemcpyDeviceToHost));
    if (P > capacity) return fail(c, VO_ERR_CAPACITY, "%s: %d pairs exceed capacity %d", who, P, capacity);
    return VO_OK;
}

// vo_match / vo_match_ex (ex: with opts and metric): check, upload both u8 sets, match
static int match_u8(vo_ctx* c, const char* who, bool ex, const uint8_t* F1, int n1, const uint8_t* F2, int n2,
                    const vo_match_opts* opts, uint32_t* pairs, float* metric, int capacity, int* n_pairs)
{
    if (!c || n1 < 0 || n2 < 0 || (n1 && !F1) || (n2 && !F2)) return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
    vo_match_params p = c->mp;
    int unique = 0;
    int rc = ex ? match_opts_resolve(c, opts, &p, &unique, who) : VO_OK;
    if (rc) return rc;
    if (n1 > c->set[0].sb.kp_cap || n2 > c->set[0].sb.kp_cap) return fail(c, VO_ERR_CAPACITY, "%s: more rows than max_keypoints", who);
    CallScope call(c); if (call.status) return call.status;
    if (n1) HIPC(c, hipMemcpyAsync(c->d_fd[0], F1, (size_t)n1 * VO_DESC_LEN, hipMemcpyHostToDevice, c->stream));
    if (n2) HIPC(c, hipMemcpyAsync(c->d_fd[1], F2, (size_t)n2 * VO_DESC_LEN, hipMemcpyHostToDevice, c->stream));
    return match_staged(c, n1, n2, ex, p, unique, pairs, metric, capacity, n_pairs, who);
}

int vo_match(vo_ctx* c, const uint8_t* F1, int n1, const uint8_t* F2, int n2, uint32_t* pairs, int capacity, int* n_pairs)
{
    return match_u8(c, "vo_match", false, F1, n1, F2, n2, nullptr, pairs, nullptr, capacity, n_pairs);
}

int vo_match_ex(vo_ctx* c, const uint8_t* F1, int n1, const uint8_t* F2, int n2, const vo_match_opts* opts, uint32_t* pairs,
                float* metric, int capacity, int* n_pairs)
{
    return match_u8(c, "vo_match_ex", true, F1, n1, F2, n2, opts, pairs, metric, capacity, n_pairs);
}

// vo_match_f32 / vo_match_f32_ex: check the arguments, copy both matrices to the device as they
// lie (d_ff) and pack them to u8 rows (d_fd); *bad = 1 if some value is not an integer in [0, 255]
static int stage_f32(vo_ctx* c, const float* F1, int n1, int ld1, const float* F2, int n2, int ld2, int col_major, int* bad,
                     const char* who)
{
    if (!c || n1 < 0 || n2 < 0 || (n1 && !F1) || (n2 && !F2) || (col_major != 0 && col_major != 1))
        return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
    if ((n1 && ld1 < (col_major ? n1 : VO_DESC_LEN)) || (n2 && ld2 < (col_major ? n2 : VO_DESC_LEN)))
        return fail(c, VO_ERR_ARG, "%s: leading dimension too small", who);
    if (n1 > c->set[0].sb.kp_cap || n2 > c->set[0].sb.kp_cap) return fail(c, VO_ERR_CAPACITY, "%s: more rows than max_keypoints", who);
    CallScope call(c); if (call.status) return call.status;
    HIPC(c, hipMemsetAsync(c->d_bad, 0, sizeof(int), c->stream));
    const float* src[2] = {F1, F2};
    const int n[2] = {n1, n2}, ld[2] = {ld1, ld2};
    for (int s = 0; s < 2; ++s) {
        if (!n[s]) continue;
        // the matrix as it lies in host memory (MATLAB: n x 128 column-major, ld = n), one copy
        const size_t elems = col_major ? (size_t)ld[s] * (VO_DESC_LEN - 1) + n[s] : (size_t)ld[s] * (n[s] - 1) + VO_DESC_LEN;
        if (elems > (size_t)c->set[0].sb.kp_cap * VO_DESC_LEN) return fail(c, VO_ERR_CAPACITY, "%s: matrix exceeds staging", who);
        HIPC(c, hipMemcpyAsync(c->d_ff[s], src[s], sizeof(float) * elems, hipMemcpyHostToDevice, c->stream));
        pack_f32_desc_launch(c->d_ff[s], n[s], ld[s], col_major, c->d_fd[s], c->d_bad, c->stream);
    }
    HIPC(c, hipMemcpyAsync(bad, c->d_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    return finish(c);
}

// the general-float path's buffers (normalised F1, transposed F2, per-row result): all three or
// none, so after a failed allocation the next call allocates again instead of launching on null
static int f32_buffers(vo_ctx* c, const char* who)
{
    if (c->d_fa) return VO_OK;
    const size_t K = c->set[0].sb.kp_cap;
    const int e = c->pool.group({DevPool::req(c->d_fa, K * VO_DESC_LEN), DevPool::req(c->d_fbt, K * VO_DESC_LEN),
                                 DevPool::req(c->d_fres, K)});
    return e ? fail(c, VO_ERR_HIP, "%s: %s", who, hipGetErrorString((hipError_t)e)) : VO_OK;
}

int vo_match_f32(vo_ctx* c, const float* F1, int n1, int ld1, const float* F2, int n2, int ld2, int col_major,
                 uint32_t* pairs, int capacity, int* n_pairs)
{
    int bad = 0;
    int rc = stage_f32(c, F1, n1, ld1, F2, n2, ld2, col_major, &bad, "vo_match_f32");
    if (rc) return rc;
    // u8-valued rows (libvo / SIFT descriptors, what VO.m passes): the exact-integer spec of the
    // hot path; any other single features: the float SSD spec (match_f32_launch)
    if (!bad) return match_staged(c, n1, n2, false, c->mp, 0, pairs, nullptr, capacity, n_pairs, "vo_match_f32");
    if ((rc = f32_buffers(c, "vo_match_f32")) != VO_OK) return rc;
    match_f32_launch(c->d_ff[0], n1, ld1, c->d_ff[1], n2, ld2, col_major, c->d_fa, c->d_fbt, c->d_fres, c->mp, c->stream);
    std::vector<int> res((size_t)n1 + 1);
    if (n1) HIPC(c, hipMemcpyAsync(res.data(), c->d_fres, sizeof(int) * n1, hipMemcpyDeviceToHost, c->stream));
    rc = finish(c);
    if (rc) return rc;
    int P = 0;
    for (int i = 0; i < n1; ++i) {
        if (res[i] < 0) continue;
        if (pairs && P < capacity) { pairs[2 * P] = (uint32_t)i + 1; pairs[2 * P + 1] = (uint32_t)res[i] + 1; }
        ++P;
    }
    if (n_pairs) *n_pairs = P;
    if (P > capacity) return fail(c, VO_ERR_CAPACITY, "vo_match_f32: %d pairs exceed capacity %d", P, capacity);
    return VO_OK;
}

int vo_match_f32_ex(vo_ctx* c, const float* F1, int n1, int ld1, const float* F2, int n2, int ld2, int col_major,
                    const vo_match_opts* opts, uint32_t* pairs, float* metric, int capacity, int* n_pairs)
{
    if (!c) return fail(c, VO_ERR_ARG, "vo_match_f32_ex: bad arguments");
    vo_match_params p;
    int unique = 0;
    int rc = match_opts_resolve(c, opts, &p, &unique, "vo_match_f32_ex");
    if (rc) return rc;
    int bad = 0;
    if ((rc = stage_f32(c, F1, n1, ld1, F2, n2, ld2, col_major, &bad, "vo_match_f32_ex")) != VO_OK) return rc;
    if (!bad) {
        CallScope call(c); if (call.status) return call.status;
        return match_staged(c, n1, n2, true, p, unique, pairs, metric, capacity, n_pairs, "vo_match_f32_ex");
    }
    if ((rc = f32_buffers(c, "vo_match_f32_ex")) != VO_OK || (rc = match_ex_buffers(c, "vo_match_f32_ex")) != VO_OK) return rc;
    CallScope call(c); if (call.status) return call.status;
    match_f32_launch_ex(c->d_ff[0], n1, ld1, c->d_ff[1], n2, ld2, col_major, c->d_fa, c->d_fbt, c->d_fres, c->mx.metric,
                        c->mx.back, p, unique, c->stream);
    std::vector<int> res((size_t)n1 + 1), back((size_t)n2 + 1);
    std::vector<float> best((size_t)n1 + 1);
    if (n1) HIPC(c, hipMemcpyAsync(res.data(), c->d_fres, sizeof(int) * n1, hipMemcpyDeviceToHost, c->stream));
    if (n1) HIPC(c, hipMemcpyAsync(best.data(), c->mx.metric, sizeof(float) * n1, hipMemcpyDeviceToHost, c->stream));
    if (unique && n1 && n2) HIPC(c, hipMemcpyAsync(back.data(), c->mx.back, sizeof(int) * n2, hipMemcpyDeviceToHost, c->stream));
    rc = finish(c);
    if (rc) return rc;
    int P = 0;
    for (int i = 0; i < n1; ++i) {
        if (res[i] < 0 || (unique && back[res[i]] != i)) continue;
        if (P < capacity) {
            if (pairs) { pairs[2 * P] = (uint32_t)i + 1; pairs[2 * P + 1] = (uint32_t)res[i] + 1; }
            if (metric) metric[P] = best[i];
        }
        ++P;
    }
    if (n_pairs) *n_pairs = P;
    if (P > capacity) return fail(c, VO_ERR_CAPACITY, "vo_match_f32_ex: %d pairs exceed capacity %d", P, capacity);
    return VO_OK;
}

// ---- matchFeaturesInRadius -----------------------------------------------------------------
// the in-radius entries' own arguments, checked before anything is enqueued: n_radius 1 or n1,
// finite coordinates, finite radii > 0 (the first offending index is named)
static int radius_args_check(vo_ctx* c, const char* who, int n1, int n2, const float* points2, const float* centers,
                             const float* radius, int n_radius, int col_major)
{
    if ((n2 && !points2) || (n1 && !centers) || !radius) return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
    if (n_radius != 1 && n_radius != n1) return fail(c, VO_ERR_ARG, "%s: n_radius %d is neither 1 nor n1 = %d", who, n_radius, n1);
    const float* P[2] = {points2, centers};
    const int n[2] = {n2, n1};
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < n[s]; ++i) {
            const float x = col_major ? P[s][i] : P[s][2 * (size_t)i], y = col_major ? P[s][(size_t)n[s] + i] : P[s][2 * (size_t)i + 1];
            if (!std::isfinite(x) || !std::isfinite(y))
                return fail(c, VO_ERR_ARG, "%s: %s row %d (%g, %g) is not finite", who, s ? "centers" : "points2", i, (double)x, (double)y);
        }
    for (int k = 0; k < n_radius; ++k)
        if (!(std::isfinite(radius[k]) && radius[k] > 0.0f))
            return fail(c, VO_ERR_ARG, "%s: radius %d (%g) is not finite and > 0", who, k, (double)radius[k]);
    return VO_OK;
}

// the in-radius match of the two staged descriptor sets, inside a call (as match_staged)
static int match_radius_staged(vo_ctx* c, int n1, int n2, const float* points2, const float* centers, const float* radius,
                               int n_radius, int col_major, const vo_match_params& p, int unique, uint32_t* pairs, float* metric,
                               int capacity, int* n_pairs, const char* who)
{
    if (n_pairs) *n_pairs = 0;
    if (n1 == 0 || n2 == 0) return VO_OK;                 // no pair; nothing is launched
    int rc = match_ex_buffers(c, who);
    if (rc) return rc;
    if (!c->mr.pts2) {
        const hipError_t e = match_radius_alloc(c->pool, c->mr, c->set[0].mb);
        if (e != hipSuccess) return fail(c, VO_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    int nn[2] = {n1, n2};
    HIPC(c, hipMemcpyAsync(c->d_fn, nn, sizeof(nn), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->mr.pts2, points2, sizeof(float) * 2 * n2, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->mr.centers, centers, sizeof(float) * 2 * n1, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->mr.radius, radius, sizeof(float) * n_radius, hipMemcpyHostToDevice, c->stream));
    desc_meta_launch(c->d_fd[0], c->d_fm[0], n1, c->stream);
    desc_meta_launch(c->d_fd[1], c->d_fm[1], n2, c->stream);
    match_radius_launch(c->set[0].mb, c->d_job_single, c->mx, c->mr, c->d_fd[0], c->d_fm[0], n1, c->d_fd[1], c->d_fm[1], n2,
                        col_major, n_radius, p, unique, c->stream);
    int P = 0;
    HIPC(c, hipMemcpyAsync(&P, c->d_mn, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    rc = finish(c);
    if (rc) return rc;
    if (n_pairs) *n_pairs = P;
    const int m = std::min(P, capacity);
    if ((rc = read_pairs(c, c->d_mi, c->d_mj, m, pairs))) return rc;
    if (m > 0 && metric) HIPC(c, hipMemcpy(metric, c->mx.metric, sizeof(float) * m, hipMemcpyDeviceToHost));
    if (P > capacity) return fail(c, VO_ERR_CAPACITY, "%s: %d pairs exceed capacity %d", who, P, capacity);
    return VO_OK;
}

int vo_match_radius(vo_ctx* c, const uint8_t* F1, int n1, const uint8_t* F2, int n2, const float* points2, const float* centers,
                    const float* radius, int n_radius, const vo_match_opts* opts, uint32_t* pairs, float* metric, int capacity,
                    int* n_pairs)
{
    const char* who = "vo_match_radius";
    if (!c || n1 < 0 || n2 < 0 || (n1 && !F1) || (n2 && !F2)) return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
    vo_match_params p;
    int unique = 0;
    int rc = match_opts_resolve(c, opts, &p, &unique, who);
    if (rc || (rc = radius_args_check(c, who, n1, n2, points2, centers, radius, n_radius, 0))) return rc;
    if (n1 > c->set[0].sb.kp_cap || n2 > c->set[0].sb.kp_cap) return fail(c, VO_ERR_CAPACITY, "%s: more rows than max_keypoints", who);
    CallScope call(c); if (call.status) return call.status;
    if (n1) HIPC(c, hipMemcpyAsync(c->d_fd[0], F1, (size_t)n1 * VO_DESC_LEN, hipMemcpyHostToDevice, c->stream));
    if (n2) HIPC(c, hipMemcpyAsync(c->d_fd[1], F2, (size_t)n2 * VO_DESC_LEN, hipMemcpyHostToDevice, c->stream));
    return match_radius_staged(c, n1, n2, points2, centers, radius, n_radius, 0, p, unique, pairs, metric, capacity, n_pairs, who);
}

int vo_match_radius_f32(vo_ctx* c, const float* F1, int n1, int ld1, const float* F2, int n2, int ld2, int col_major,
                        const float* points2, const float* centers, const float* radius, int n_radius, const vo_match_opts* opts,
                        uint32_t* pairs, float* metric, int capacity, int* n_pairs)
{
    const char* who = "vo_match_radius_f32";
    if (!c || n1 < 0 || n2 < 0 || (col_major != 0 && col_major != 1)) return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
    vo_match_params p;
    int unique = 0;
    int rc = match_opts_resolve(c, opts, &p, &unique, who);
    if (rc || (rc = radius_args_check(c, who, n1, n2, points2, centers, radius, n_radius, col_major))) return rc;
    int bad = 0;
    if ((rc = stage_f32(c, F1, n1, ld1, F2, n2, ld2, col_major, &bad, who)) != VO_OK) return rc;
    if (bad) return fail(c, VO_ERR_ARG, "%s: features must hold integers in [0, 255] (general single features are not matched in radius)", who);
    CallScope call(c); if (call.status) return call.status;
    return match_radius_staged(c, n1, n2, points2, centers, radius, n_radius, col_major, p, unique, pairs, metric, capacity,
                               n_pairs, who);
}

// vo_pair_stats.flags / vo_step_out.flags of one frame's n images: VO_FLAG_KEYPOINTS if an
// image detected more keypoints than max_keypoints, VO_FLAG_CANDIDATES if its extremum test
// (k_ext_inner's partial candidates included) produced more candidates than the list holds,
// so k_seg_emit dropped some in scan order and the keypoint set is incomplete
static int capacity_flags(const SiftBuffers& sb, const int* nkp, const int* ncand, int n)
{
    int fl = 0;
    for (int i = 0; i < n; ++i) {
        if (nkp[i] > sb.kp_cap) fl |= VO_FLAG_KEYPOINTS;
        if (ncand[i] > sb.cand_cap) fl |= VO_FLAG_CANDIDATES;
    }
    return fl;
}

// SIFT of 2B images + stereo matching of B frames into buffer set `set`.  The frames are
// split into `parts` (vo_set_concurrency); every part's scale space runs on sub[0] and its
// feature stages + stereo matching on sub[1] once that part's scale space is done, so the
// features of part k overlap the scale space of part k+1 (and of the next call, which uses
// the other set).  Inputs are ordered after earlier work on `stream`; the set's previous
// contents are released by its events (below).  With `join`, `stream` waits for the result.
// The arrangement of one part (with `chains`; without, `down`'s work follows on sub[0]):
//   sub[0]  waits for the set's arena (ev_arena: the previous call's last reader, k_desc -- not
//           that call's whole feature stream, whose stereo match reads descriptors only);
//           octave 0, ev_o0; octave 1's levels 1..L, ev_down, its levels L+1..L+2, ev_top (the
//           top chain; with no large octave 1 the fork follows octave 0's level L).
//   down    after ev_down (octave 1's level L has stored octave 2's base) the large octaves 2..
//           with all their levels, then the LDS-sized octaves (k_small_pyr); ev_join.  Ordered
//           behind sub[0]'s wait for the arena by ev_down.  One stream for both buffer sets: a call's
//           fork already follows the previous call's top chain on sub[0], and with `stream`, the two
//           forked streams and the copy stream of the pipelined loop a stream per set would be the
//           process's sixth.
//   sub[1]  after ev_o0 the extremum test of octave 0, beside the scale space of octaves 1..;
//           after ev_top and ev_join (both chains) the extremum test of octaves 1.., the feature
//           stages and the stereo match.  ev_arena and ev_done are recorded here, so they cover
//           both chains: the set's next call, the batch's slot event of the pipelined loop and
//           CallScope's quiesce wait for them as before.
// Forking after octave 0's level L instead (octaves 1.. beside octave 0's two widest blurs), with or
// without octave 1's top levels back on sub[0], and the down stream at another priority all measured
// 1-3 % slower than one chain: ev_o0 fires 9 ms later and the feature stream becomes the critical one
// (DESIGN.md §9j).
// The extremum test of octaves 1.. at the scale space's tail instead (round 3's placement, then
// 0.4 ms on the critical stream) measured 7.66-7.77 against 7.51-7.55 ms per 64-frame step and no
// better since.  k_small_pyr (one 1024-thread workgroup per image, ~120 KB of
// LDS: 0.13 ms isolated, ~1 ms in situ while it waits for a CU with that much free LDS) at the
// head of the feature stream's part, or on a stream of its own behind the last level blur,
// measured slower than waiting at the tail; on the down chain it follows octaves 2..
// beside octave 1's top levels (0.5-0.7 instead of 1.4-2.1 ms in situ).  Waiting for the set's
// ev_done (after the stereo match) instead of ev_arena cost the full path 1.4 %.
static int enqueue_sift_stereo(vo_ctx* c, int set, const uint8_t* d_l, const uint8_t* d_r, int B, bool join,
                               bool chains, bool fork = true)
{
    const size_t fs = (size_t)c->rows * c->cols;
    const int parts = std::min(c->n_sub, B);
    vo_ctx::BufferSet& S = c->set[set];
    hipStream_t sp = c->sub[0], st = c->sub[1];
    // (a synchronous profiled call -- bench.py's isolated pass -- keeps the scale space one chain
    // and starts the features after all of it, so its per-kernel durations stay undisturbed)
    const bool iso = c->prof.on && join;
    // The pipelined loop body (chains = false) keeps one chain as well: its geometry stream and copy
    // stream are busy beside the two forked ones, and with `down` as a fifth stream on four hardware
    // queues the full path lost 4 %
    const hipStream_t sd = (iso || !chains) ? sp : c->down;
    if (fork) {                                               // inputs / earlier work on `stream`
        HIPC(c, hipEventRecord(c->ev_fork, c->stream));
        HIPC(c, hipStreamWaitEvent(sp, c->ev_fork, 0));
    }
    // the set's arena free: its previous call's last reader (k_desc) is done -- the stereo match
    // of that call (descriptors only) may still run; everything else of the set is written by st,
    // in order behind it
    HIPC(c, hipStreamWaitEvent(sp, S.ev_arena, 0));
    const int o_small = sift_small_octave(c->py);
    const bool undist = c->ud_on[0] || c->ud_on[1];           // vo_set_distortion
    if (undist) c->rect_B = B;
    S.sel_used = c->strongest > 0;
    // scale space on sp; octave 0's extremum test on st as soon as octave 0 is built (beside the
    // scale space of octaves 1..), the other octaves' on st after the scale space -- the split
    // that balances the two streams
    for (int p = 0; p < parts; ++p) {
        const int f0 = B * p / parts, nf = B * (p + 1) / parts - f0;
        const uint8_t* pl = d_l + f0 * fs;
        const uint8_t* pr = d_r + f0 * fs;
        if (undist) {
            // VO.m:75-76: the part's frames of both cameras, undistorted into d_rect by one launch.
            // sp runs it behind the base kernels of every earlier part, call and batch -- the only
            // readers of d_rect -- so the one buffer serves both sets and all batches in flight.
            UndistortSide U[2];
            for (int k = 0; k < 2; ++k) {
                U[k].cam = c->ud_cam[k];
                U[k].in = k ? pr : pl;
                U[k].out = c->d_rect + ((size_t)k * c->max_batch + f0) * fs;
                U[k].copy = c->ud_on[k] ? 0 : 1;
                U[k].pad = 0;
            }
            undistort_launch(U, 2, c->rows, c->cols, nf, fs, fs, sp);
            pl = U[0].out;
            pr = U[1].out;
        }
        ImageSrc src{pl, pr, fs, c->cols, 0};
        SiftBuffers v = sift_view(S.sb, c->py, 2 * f0, 2 * nf);
        ScaleChains ch;
        ch.down = sd;
        ch.ev_fork = c->ev_down[p];
        sift_enqueue_pyramid(c->py, v, src, 2 * nf, c->sp, sp, c->d_py, c->ev_o0[p], ch);
        HIPC(c, hipEventRecord(c->ev_top[p], sp));              // the top chain's end
        sift_enqueue_small(c->py, v, 2 * nf, sd, c->d_py);
        HIPC(c, hipEventRecord(c->ev_join[p], sd));
    }
    for (int p = 0; p < parts; ++p) {
        const int f0 = B * p / parts, nf = B * (p + 1) / parts - f0;
        SiftBuffers v = sift_view(S.sb, c->py, 2 * f0, 2 * nf);
        HIPC(c, hipStreamWaitEvent(st, iso ? c->ev_join[p] : c->ev_o0[p], 0));
        sift_enqueue_extrema(c->py, v, 2 * nf, c->sp, st, c->d_py, 0, 1);
        // the end of both chains (one chain gave both by ev_join alone)
        HIPC(c, hipStreamWaitEvent(st, c->ev_top[p], 0));
        HIPC(c, hipStreamWaitEvent(st, c->ev_join[p], 0));
        sift_enqueue_extrema(c->py, v, 2 * nf, c->sp, st, c->d_py, 1, o_small);
        sift_enqueue_extrema(c->py, v, 2 * nf, c->sp, st, c->d_py, o_small, c->py.n_oct);
        sift_enqueue_features(c->py, v, 2 * nf, c->sp, st, c->d_py, c->strongest);
        if (p == parts - 1) HIPC(c, hipEventRecord(S.ev_arena, st));
        match_launch(match_view(S.mb, f0), S.d_jobs + job_stereo(c, f0), nf, c->mp, st);
    }
    HIPC(c, hipEventRecord(S.ev_done, st));
    if (join) HIPC(c, hipStreamWaitEvent(c->stream, S.ev_done, 0));
    c->last_set = set;
    c->described = false;
    return VO_OK;
}

int vo_sift_match_batch_dev(vo_ctx* c, const uint8_t* d_lefts, const uint8_t* d_rights, int B, vo_pair_stats* stats)
{
    if (!c || !d_lefts || !d_rights || B < 1 || B > c->max_batch) return fail(c, VO_ERR_ARG, "vo_sift_match_batch_dev: bad arguments");
    CallScope call(c, false); if (call.status) return call.status;
    const int set = c->next_set;
    c->next_set ^= 1;
    const bool sync = stats != nullptr;      // profiling events are collected by vo_kernel_times
    int rc = enqueue_sift_stereo(c, set, d_lefts, d_rights, B, sync, true);
    if (rc) return rc;
    c->last_B = B;
    if (!sync) return launch_status(c);
    const vo_ctx::BufferSet& S = c->set[set];
    std::vector<int> nk(2 * B), nc(2 * B), np(B);
    std::vector<int> nd;                     // detected counts: the flags' input (selection off: nk)
    HIPC(c, hipMemcpyAsync(nk.data(), S.sb.n_kp, sizeof(int) * 2 * B, hipMemcpyDeviceToHost, c->stream));
    if (c->strongest > 0) {
        nd.resize(2 * B);
        HIPC(c, hipMemcpyAsync(nd.data(), S.sb.n_det, sizeof(int) * 2 * B, hipMemcpyDeviceToHost, c->stream));
    }
    HIPC(c, hipMemcpyAsync(nc.data(), S.sb.n_cand, sizeof(int) * 2 * B, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(np.data(), S.pair_n, sizeof(int) * B, hipMemcpyDeviceToHost, c->stream));
    rc = finish(c);
    if (rc) return rc;
    if (stats) {
        for (int f = 0; f < B; ++f) {
            stats[f].n_left = nk[2 * f]; stats[f].n_right = nk[2 * f + 1]; stats[f].n_stereo = np[f];
            stats[f].flags = capacity_flags(c->set[0].sb, (nd.empty() ? nk : nd).data() + 2 * f, nc.data() + 2 * f, 2);
        }
    }
    return VO_OK;
}

int vo_fetch_keypoints(vo_ctx* c, int image, vo_keypoint* kps, uint8_t* desc, int capacity, int* n)
{
    if (!c || image < 0 || image >= c->set[0].sb.n_img) return fail(c, VO_ERR_ARG, "vo_fetch_keypoints: bad image");
    vo_ctx::BufferSet* S = nullptr;
    int rc = fetch_set(c, image, "vo_fetch_keypoints", true, &S);
    if (rc) return rc;
    const SiftBuffers& B = S->sb;
    int cnt = 0;
    HIPC(c, hipMemcpy(&cnt, B.n_kp + image, sizeof(int), hipMemcpyDeviceToHost));
    if (n) *n = cnt;
    int m = std::min(std::min(cnt, B.kp_cap), capacity);
    if (m > 0) {
        if (kps) HIPC(c, hipMemcpy(kps, B.kp + (size_t)image * B.kp_cap, sizeof(vo_keypoint) * m, hipMemcpyDeviceToHost));
        if (desc) HIPC(c, hipMemcpy(desc, B.desc + (size_t)image * B.kp_cap * VO_DESC_LEN, (size_t)m * VO_DESC_LEN, hipMemcpyDeviceToHost));
    }
    return VO_OK;
}

int vo_fetch_candidate_counts(vo_ctx* c, int image, int* n_cand, int* n_accepted)
{
    if (!c || image < 0 || image >= c->set[0].sb.n_img) return fail(c, VO_ERR_ARG, "vo_fetch_candidate_counts: bad image");
    vo_ctx::BufferSet* S = nullptr;
    int rc = fetch_set(c, image, "vo_fetch_candidate_counts", true, &S);
    if (rc) return rc;
    const SiftBuffers& B = S->sb;
    int v[2] = {0, 0};
    HIPC(c, hipMemcpy(&v[0], B.n_cand + image, sizeof(int), hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(&v[1], B.n_acc + image, sizeof(int), hipMemcpyDeviceToHost));
    if (n_cand) *n_cand = v[0];
    if (n_accepted) *n_accepted = v[1];
    return VO_OK;
}

int vo_fetch_gaussian(vo_ctx* c, int image, int octave, int level, float* out, int capacity, int* rows, int* cols)
{
    if (!c || image < 0 || image >= c->set[0].sb.n_img || octave < 0 || octave >= c->py.n_oct || level < 0 ||
        level >= c->py.L + 3)
        return fail(c, VO_ERR_ARG, "vo_fetch_gaussian: bad image/octave/level");
    vo_ctx::BufferSet* S = nullptr;
    int rc = fetch_set(c, image, "vo_fetch_gaussian", false, &S);
    if (rc) return rc;
    const SiftBuffers& B = S->sb;
    const OctGeom& g = c->py.oct[octave];
    if (rows) *rows = g.rows;
    if (cols) *cols = g.cols;
    if (!out) return VO_OK;
    if (capacity < g.rows * g.cols) return fail(c, VO_ERR_CAPACITY, "vo_fetch_gaussian: capacity %d < %d", capacity, g.rows * g.cols);
    const float* src = B.arena + (size_t)image * c->py.istride + g.g_off[level];
    HIPC(c, hipMemcpy2D(out, sizeof(float) * g.cols, src, sizeof(float) * g.pitch, sizeof(float) * g.cols, g.rows,
                        hipMemcpyDeviceToHost));
    return VO_OK;
}

int vo_fetch_stereo_pairs(vo_ctx* c, int frame, uint32_t* pairs, int capacity, int* n)
{
    if (!c || frame < 0 || frame >= c->max_batch) return fail(c, VO_ERR_ARG, "vo_fetch_stereo_pairs: bad frame");
    vo_ctx::BufferSet* S = nullptr;
    int rc = fetch_set(c, 2 * frame, "vo_fetch_stereo_pairs", true, &S);   // the frame's images and its pair slot: one set
    if (rc) return rc;
    int P = 0;
    HIPC(c, hipMemcpy(&P, S->pair_n + frame, sizeof(int), hipMemcpyDeviceToHost));
    if (n) *n = P;
    const size_t row = (size_t)frame * S->sb.kp_cap;
    return read_pairs(c, S->pair_i + row, S->pair_j + row, std::min(P, capacity), pairs);
}

}  // extern "C"

// ---- tracking / geometry / loop --------------------------------------------
static vo_calib calib_of(const double P1[12], const double P2[12], const double* K)
{
    vo_calib c;
    memcpy(c.P1, P1, sizeof(c.P1));
    memcpy(c.P2, P2, sizeof(c.P2));
    if (K) memcpy(c.K, K, sizeof(c.K));
    else for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) c.K[3 * i + j] = P1[4 * i + j];
    return c;
}

static StepArgs step_args(vo_ctx* c, int B, int set = 0)
{
    vo_ctx::BufferSet& S = c->set[set];
    StepArgs a;
    a.sb = &S.sb;
    a.pair_i = S.pair_i; a.pair_j = S.pair_j; a.pair_n = S.pair_n;
    a.max_frames = c->max_batch; a.B = B; a.kp_cap = c->set[0].sb.kp_cap;
    a.first_has_prev = c->have_features ? 1 : 0;
    a.frame_index0 = c->frame_index;
    a.calib = c->calib;
    a.rp = c->rp;
    a.refine_on = c->refine_on ? 1 : 0;
    a.refine = c->refine;
    return a;
}

static void mat4_mul(const double* A, const double* B, double* C)
{
    double T[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            T[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j] + A[4 * i + 3] * B[12 + j];
    memcpy(C, T, sizeof(T));
}

// world transform of one landmark row, rounded through single (CreateLandmarksFromFeatures.m:17)
static void lm_world(const double* pose, const float* X, double* out)
{
    const double x0 = X[0], x1 = X[1], x2 = X[2];
    for (int a = 0; a < 3; ++a) {
        double w = pose[4 * a] * x0 + pose[4 * a + 1] * x1 + pose[4 * a + 2] * x2 + pose[4 * a + 3];
        out[a] = (double)(float)w;
    }
}

// copy frame f's SIFT results + stereo pairs into the carry slots (prev of the next call's frame 0)
// Frame f of set `from` becomes the carried (previous) frame of set `to`: its keypoints,
// descriptors and stereo pairs are copied into `to`'s carry slots (image slots 2M, 2M+1,
// pair slot M), which frame 0 of the next batch tracks against.
static int enqueue_carry(vo_ctx* c, int from, int f, int to)
{
    const int M = c->max_batch, K = c->set[0].sb.kp_cap;
    const vo_ctx::BufferSet& A = c->set[from];
    const vo_ctx::BufferSet& Z = c->set[to];
    for (int side = 0; side < 2; ++side) {
        const int src = 2 * f + side, dst = 2 * M + side;
        HIPC(c, hipMemcpyAsync(Z.sb.kp + (size_t)dst * K, A.sb.kp + (size_t)src * K, sizeof(vo_keypoint) * K,
                               hipMemcpyDeviceToDevice, c->stream));
        HIPC(c, hipMemcpyAsync(Z.sb.desc + (size_t)dst * K * VO_DESC_LEN, A.sb.desc + (size_t)src * K * VO_DESC_LEN,
                               (size_t)K * VO_DESC_LEN, hipMemcpyDeviceToDevice, c->stream));
        HIPC(c, hipMemcpyAsync(Z.sb.meta + (size_t)dst * K, A.sb.meta + (size_t)src * K, sizeof(DescMeta) * K,
                               hipMemcpyDeviceToDevice, c->stream));
        HIPC(c, hipMemcpyAsync(Z.sb.n_kp + dst, A.sb.n_kp + src, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
        if (c->strongest > 0)
            HIPC(c, hipMemcpyAsync(Z.sb.n_det + dst, A.sb.n_det + src, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    }
    HIPC(c, hipMemcpyAsync(Z.pair_i + (size_t)M * K, A.pair_i + (size_t)f * K, sizeof(int) * K, hipMemcpyDeviceToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(Z.pair_j + (size_t)M * K, A.pair_j + (size_t)f * K, sizeof(int) * K, hipMemcpyDeviceToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(Z.pair_n + M, A.pair_n + f, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    return VO_OK;
}

// The VO.m loop body for B frames whose images are in device memory, split into a
// device half (submit: everything up to the per-frame results, asynchronous) and a host
// half (collect: pose chain VO.m:130-134 and landmark append CreateLandmarksFromFeatures.m:20).
// Batch n uses buffer set n & 1 and result slot n mod VO_STEP_DEPTH.  Its scale space (sub[0])
// waits only for the arena's last reader of batch n-2 (ev_arena); its feature stages and stereo
// matching (sub[1]) overwrite the keypoints, descriptors and stereo pairs that batch n-2's
// geometry reads, so they wait for the end of that batch on the GPU (its slot event) -- not for
// the host to collect it, so the scale space of batch n runs straight after batch n-1's while
// batch n-2's geometry finishes.  Its tracking, triangulation, MSAC and landmark kernels run on
// `stream` after the SIFT and after the previous batch's carry; then frame B-1 is carried into
// the other set, the landmark rows are packed into the slot and the small per-frame results
// are copied to the slot's pinned host memory.  With fork, the SIFT is also ordered after
// earlier work on `stream` (the synchronous calls' H2D copies).
static int submit_batch(vo_ctx* c, const uint8_t* d_l, const uint8_t* d_r, int B, bool fork)
{
    if (!c->has_calib) return fail(c, VO_ERR_STATE, "vo_step: no calibration (vo_set_calib)");
    if (c->pending.size() >= VO_STEP_DEPTH)
        return fail(c, VO_ERR_STATE, "vo_step_submit_dev: %d batches already pending (collect first)", VO_STEP_DEPTH);
    const int set = c->next_step_set, slot = c->next_slot;
    vo_ctx::BufferSet& S = c->set[set];
    for (const vo_ctx::Pending& q : c->pending)         // batch n-2 (same set), still in flight
        if (q.set == set) HIPC(c, hipStreamWaitEvent(c->sub[1], c->sh[q.slot].ev, 0));
    int rc = enqueue_sift_stereo(c, set, d_l, d_r, B, true, false, fork);   // `stream` waits for this set's SIFT
    if (rc) return rc;
    StepArgs a = step_args(c, B, set);
    S.refine_used = c->refine_on;
    geom_enqueue(S.gb, S.mb, S.d_jobs + job_track(c, 0, 0), a, c->mp, c->stream);
    vo_ctx::StepHost& H = c->sh[slot];
    HIPC(c, hipMemcpyAsync(H.fg, S.gb.fg, sizeof(FrameGeom) * B, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(H.nkp, S.sb.n_kp, sizeof(int) * 2 * B, hipMemcpyDeviceToHost, c->stream));
    if (c->strongest > 0)
        HIPC(c, hipMemcpyAsync(H.ndet, S.sb.n_det, sizeof(int) * 2 * B, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(H.ncand, S.sb.n_cand, sizeof(int) * 2 * B, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(H.np, S.pair_n, sizeof(int) * B, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(H.rows, S.gb.lm_rows, sizeof(int) * B, hipMemcpyDeviceToHost, c->stream));
    lm_pack_launch(S.gb, B, H.d_pX, H.d_pkeep, c->stream);
    if ((rc = enqueue_carry(c, set, B - 1, set ^ 1))) return rc;
    HIPC(c, hipEventRecord(H.ev, c->stream));
    if ((rc = launch_status(c))) return rc;
    c->pending.push_back({set, slot, B, c->have_features, c->strongest > 0});
    c->next_step_set ^= 1;
    c->next_slot = (slot + 1) % VO_STEP_DEPTH;
    c->have_features = true;
    c->frame_index += B;
    return VO_OK;
}

static int collect_batch(vo_ctx* c, vo_step_out* outs, int capacity, int* n_out)
{
    if (c->pending.empty()) return fail(c, VO_ERR_STATE, "vo_step_collect: no batch pending");
    const vo_ctx::Pending P = c->pending.front();
    if (capacity < P.B) return fail(c, VO_ERR_CAPACITY, "vo_step_collect: %d frames pending, capacity %d", P.B, capacity);
    const int K = c->set[0].sb.kp_cap, B = P.B;
    const vo_ctx::StepHost& H = c->sh[P.slot];
    if (c->prof.on) {                                  // profiling: events of every stream are collected
        int rc = finish(c);
        if (rc) return rc;
    } else {
        HIPC(c, hipEventSynchronize(H.ev));
    }
    // the batch's landmark rows, packed on the device in frame order (k_lm_pack): one copy each
    // of X and keep into pinned memory (per-frame copies into pageable vectors cost ~2 x B
    // staged transfers per batch)
    size_t total = 0;
    std::vector<size_t> roff(B + 1, 0);
    for (int f = 0; f < B; ++f) roff[f + 1] = roff[f] + (size_t)std::min(H.rows[f], K);
    total = roff[B];
    if (c->lm_camera) {
        // camera-frame rows stay on the device: the tracked frames' packed rows are appended to
        // the store by one device-to-device copy on `stream` (ordered before the next submit
        // into this slot, which reuses the packed buffer: it needs this collect first)
        const size_t first = (P.first_tracked ? 0 : roff[1]), add = total - first;
        if (add > 0) {
            if (c->lm_n + add > c->lm_cap) {
                // the store at least doubles; the old one is copied on `stream` (in order with the
                // appends) and retired until reset / destroy, so growth never waits for the pipeline
                const size_t cap = std::max<size_t>({c->lm_n + add, 2 * c->lm_cap, (size_t)1 << 16}), n_retired = c->lm_retired.size();
                float* oX = c->d_lmX;
                uint8_t* ok = c->d_lmkeep;
                if (c->pool.grow({DevPool::req(c->d_lmX, 3 * cap), DevPool::req(c->d_lmkeep, cap)}, &c->lm_retired))
                    return fail(c, VO_ERR_HIP, "vo_step_collect: landmark store of %zu rows", cap);
                hipError_t ge = hipSuccess;
                if (c->lm_n > 0) {
                    ge = hipMemcpyAsync(c->d_lmX, oX, sizeof(float) * 3 * c->lm_n, hipMemcpyDeviceToDevice, c->stream);
                    if (ge == hipSuccess) ge = hipMemcpyAsync(c->d_lmkeep, ok, c->lm_n, hipMemcpyDeviceToDevice, c->stream);
                }
                if (ge != hipSuccess) {
                    (void)hipStreamSynchronize(c->stream);   // the copies may be queued: let them drain
                    c->pool.release(c->d_lmX); c->pool.release(c->d_lmkeep);
                    c->d_lmX = oX; c->d_lmkeep = ok;         // back to the old store, no longer retired
                    c->lm_retired.resize(n_retired);
                    return fail(c, VO_ERR_HIP, "vo_step_collect: landmark store growth: %s", hipGetErrorString(ge));
                }
                c->lm_cap = cap;
            }
            HIPC(c, hipMemcpyAsync(c->d_lmX + 3 * c->lm_n, H.d_pX + 3 * first, sizeof(float) * 3 * add,
                                   hipMemcpyDeviceToDevice, c->stream));
            HIPC(c, hipMemcpyAsync(c->d_lmkeep + c->lm_n, H.d_pkeep + first, add, hipMemcpyDeviceToDevice, c->stream));
            c->lm_n += add;
        }
    } else if (total > 0) {
        HIPC(c, hipMemcpyAsync(H.pX, H.d_pX, sizeof(float) * 3 * total, hipMemcpyDeviceToHost, c->copy_stream));
        HIPC(c, hipMemcpyAsync(H.pkeep, H.d_pkeep, total, hipMemcpyDeviceToHost, c->copy_stream));
        HIPC(c, hipStreamSynchronize(c->copy_stream));
    }
    c->pending.pop_front();
    c->last_step_set = P.set;
    c->last_step_B = B;
    for (int f = 0; f < B; ++f) {
        vo_step_out& o = outs[f];
        memset(&o, 0, sizeof(o));
        o.n_left = H.nkp[2 * f]; o.n_right = H.nkp[2 * f + 1]; o.n_stereo = H.np[f];
        o.flags = capacity_flags(c->set[0].sb, (P.sel ? H.ndet : H.nkp) + 2 * f, H.ncand + 2 * f, 2);
        memcpy(o.rel_pose, I4, sizeof(I4));
        const bool tracked = f > 0 || P.first_tracked;
        if (c->lm_camera) {
            const size_t r = tracked ? roff[f + 1] - roff[f] : 0;
            c->lm_frame_off.push_back(c->lm_frame_off.back() + (long long)r);
        }
        if (tracked) {
            o.status = H.fg[f].status;
            o.n_tracked = H.fg[f].n_tracked;
            o.n_inliers = H.fg[f].n_inliers;
            if (o.status == VO_OK) {
                memcpy(o.rel_pose, H.fg[f].T, sizeof(H.fg[f].T));
                mat4_mul(c->pose, H.fg[f].T, c->pose);
            }
            const int r = (int)(roff[f + 1] - roff[f]);
            const float* Xf = H.pX + roff[f] * 3;
            const uint8_t* kf = H.pkeep + roff[f];
            o.n_landmarks = r;
            if (!c->lm_camera) {
                size_t base = c->landmarks.size();
                c->landmarks.resize(base + (size_t)r * 3, 0.0);
                for (int m = 0; m < r; ++m)
                    if (kf[m]) lm_world(c->pose, Xf + (size_t)m * 3, &c->landmarks[base + (size_t)m * 3]);
            }
        }
        memcpy(o.pose, c->pose, sizeof(c->pose));
    }
    if (n_out) *n_out = B;
    return VO_OK;
}

// synchronous form: submit + collect (nothing else may be pending)
static int run_batch(vo_ctx* c, const uint8_t* d_l, const uint8_t* d_r, int B, vo_step_out* outs)
{
    if (!c->pending.empty()) return fail(c, VO_ERR_STATE, "vo_step: asynchronous batches pending (vo_step_collect first)");
    int rc = submit_batch(c, d_l, d_r, B, true);
    if (rc) return rc;
    return collect_batch(c, outs, B, nullptr);
}

extern "C" {

int vo_step_batch_dev(vo_ctx* c, const uint8_t* d_l, const uint8_t* d_r, int B, vo_step_out* outs)
{
    if (!c || !d_l || !d_r || !outs || B < 1 || B > c->max_batch) return fail(c, VO_ERR_ARG, "vo_step_batch_dev: bad arguments");
    CallScope call(c); if (call.status) return call.status;
    return run_batch(c, d_l, d_r, B, outs);
}

int vo_step_batch_ex(vo_ctx* c, const uint8_t* lefts, const uint8_t* rights, int ld, int col_major, int B, vo_step_out* outs)
{
    if (!c || !lefts || !rights || !outs || B < 1 || B > c->max_batch || (col_major != 0 && col_major != 1) ||
        ld < (col_major ? c->rows : c->cols))
        return fail(c, VO_ERR_ARG, "vo_step_batch: bad arguments");
    CallScope call(c); if (call.status) return call.status;
    const size_t fs = (size_t)c->rows * c->cols;
    uint8_t* dl = c->d_img;
    uint8_t* dr = c->d_img + fs * B;
    int rc = stage_images(c, lefts, ld, col_major, B, dl);
    if (!rc) rc = stage_images(c, rights, ld, col_major, B, dr);
    return rc ? rc : run_batch(c, dl, dr, B, outs);
}

int vo_step_batch(vo_ctx* c, const uint8_t* lefts, const uint8_t* rights, int ld, int B, vo_step_out* outs)
{
    return vo_step_batch_ex(c, lefts, rights, ld, 0, B, outs);
}

int vo_step(vo_ctx* c, const uint8_t* left, const uint8_t* right, int ld, vo_step_out* out)
{
    return vo_step_batch(c, left, right, ld, 1, out);
}

int vo_step_submit_dev(vo_ctx* c, const uint8_t* d_l, const uint8_t* d_r, int B)
{
    if (!c || !d_l || !d_r || B < 1 || B > c->max_batch) return fail(c, VO_ERR_ARG, "vo_step_submit_dev: bad arguments");
    CallScope call(c, false, true); if (call.status) return call.status;
    // the first batch of a pipeline is ordered after earlier work on `stream`; later ones
    // overlap the previous batch's geometry (their inputs must be ready at the call)
    return submit_batch(c, d_l, d_r, B, c->pending.empty());
}

int vo_step_collect(vo_ctx* c, vo_step_out* outs, int capacity, int* n)
{
    if (!c || !outs) return fail(c, VO_ERR_ARG, "vo_step_collect: bad arguments");
    hipSetDevice(c->device);
    return collect_batch(c, outs, capacity, n);
}

int vo_steps_pending(const vo_ctx* c) { return c ? (int)c->pending.size() : 0; }

// The start of the entries that read the last collected step batch: frame in that batch, and its
// buffer set not reused by a pending one.  Selects the device.
static int collected_set(vo_ctx* c, int frame, const char* who, const vo_ctx::BufferSet** S)
{
    if (c->last_step_set < 0 || frame < 0 || frame >= c->last_step_B)
        return fail(c, VO_ERR_STATE, "%s: frame %d not in the last collected batch", who, frame);
    for (const vo_ctx::Pending& q : c->pending)
        if (q.set == c->last_step_set)
            return fail(c, VO_ERR_STATE, "%s: the collected batch's buffer set is reused by a pending batch", who);
    hipSetDevice(c->device);
    *S = &c->set[c->last_step_set];
    return VO_OK;
}

int vo_fetch_tracks(vo_ctx* c, int frame, float* old_l, float* cur_l, double* world, float* det, int capacity,
                    int* n_tracked, int* n_det)
{
    if (!c || capacity < 0) return fail(c, VO_ERR_ARG, "vo_fetch_tracks: bad arguments");
    const vo_ctx::BufferSet* Sp = nullptr;
    int rc = collected_set(c, frame, "vo_fetch_tracks", &Sp);
    if (rc) return rc;
    const vo_ctx::BufferSet& S = *Sp;
    const int K = c->set[0].sb.kp_cap;
    int n = 0, nd = 0;
    HIPC(c, hipMemcpy(&n, S.gb.list_n + 4 * frame + 3, sizeof(int), hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(&nd, S.sb.n_kp + 2 * frame, sizeof(int), hipMemcpyDeviceToHost));
    n = std::min(std::max(n, 0), K);
    nd = std::min(std::max(nd, 0), K);
    if (n_tracked) *n_tracked = n;
    if (n_det) *n_det = nd;
    const int m = std::min(n, capacity), md = std::min(nd, capacity);
    if (m > 0 && (old_l || cur_l || world)) {
        std::vector<float> op((size_t)m * 4);
        std::vector<double> ip((size_t)m * 2);
        HIPC(c, hipMemcpy(op.data(), S.gb.oldpos + (size_t)frame * K * 4, sizeof(float) * 4 * m, hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(ip.data(), S.gb.imgpt + (size_t)frame * K * 2, sizeof(double) * 2 * m, hipMemcpyDeviceToHost));
        if (world) HIPC(c, hipMemcpy(world, S.gb.world + (size_t)frame * K * 3, sizeof(double) * 3 * m, hipMemcpyDeviceToHost));
        for (int k = 0; k < m; ++k) {
            if (old_l) { old_l[2 * k] = op[4 * k]; old_l[2 * k + 1] = op[4 * k + 1]; }
            if (cur_l) { cur_l[2 * k] = (float)ip[2 * k]; cur_l[2 * k + 1] = (float)ip[2 * k + 1]; }
        }
    }
    if (det && md > 0) {
        std::vector<vo_keypoint> kp(md);
        HIPC(c, hipMemcpy(kp.data(), S.sb.kp + (size_t)(2 * frame) * K, sizeof(vo_keypoint) * md, hipMemcpyDeviceToHost));
        for (int k = 0; k < md; ++k) { det[2 * k] = kp[k].x; det[2 * k + 1] = kp[k].y; }
    }
    return VO_OK;
}

// the quality buffers of vo_triangulate_ex / vo_fetch_track_quality, at the first call that needs them
static int tri_quality_buffers(vo_ctx* c)
{
    const size_t K = c->set[0].sb.kp_cap;
    if (!c->d_tq_err) HIPC(c, (hipError_t)c->pool.group({DevPool::req(c->d_tq_err, K), DevPool::req(c->d_tq_valid, K)}));
    return VO_OK;
}

int vo_fetch_track_quality(vo_ctx* c, int frame, float* old_r, float* reproj_err, uint8_t* valid, int capacity, int* n_tracked)
{
    if (!c || capacity < 0) return fail(c, VO_ERR_ARG, "vo_fetch_track_quality: bad arguments");
    const vo_ctx::BufferSet* Sp = nullptr;
    int rc = collected_set(c, frame, "vo_fetch_track_quality", &Sp);
    if (rc) return rc;
    const vo_ctx::BufferSet& S = *Sp;
    const int K = c->set[0].sb.kp_cap;
    int n = 0;
    HIPC(c, hipMemcpy(&n, S.gb.list_n + 4 * frame + 3, sizeof(int), hipMemcpyDeviceToHost));
    n = std::min(std::max(n, 0), K);
    if (n_tracked) *n_tracked = n;
    const int m = std::min(n, capacity);
    if (m <= 0) return VO_OK;
    if (old_r) {
        std::vector<float> op((size_t)m * 4);
        HIPC(c, hipMemcpy(op.data(), S.gb.oldpos + (size_t)frame * K * 4, sizeof(float) * 4 * m, hipMemcpyDeviceToHost));
        for (int k = 0; k < m; ++k) { old_r[2 * k] = op[4 * k + 2]; old_r[2 * k + 1] = op[4 * k + 3]; }
    }
    if (reproj_err || valid) {
        // the collected batch's geometry is complete (vo_step_collect waited for it) and a pending
        // batch works on the other set, so the kernel runs on the copy stream, which holds no work
        // between calls, beside whatever `stream` still has queued
        if ((rc = tri_quality_buffers(c))) return rc;
        tri_quality_launch(S.gb.oldpos + (size_t)frame * K * 4, S.gb.world + (size_t)frame * K * 3, S.gb.list_n + 4 * frame + 3, 4,
                           0, 1, K, c->calib, c->d_tq_err, c->d_tq_valid, c->copy_stream);
        if (reproj_err) HIPC(c, hipMemcpyAsync(reproj_err, c->d_tq_err, sizeof(float) * m, hipMemcpyDeviceToHost, c->copy_stream));
        if (valid) HIPC(c, hipMemcpyAsync(valid, c->d_tq_valid, (size_t)m, hipMemcpyDeviceToHost, c->copy_stream));
        HIPC(c, hipStreamSynchronize(c->copy_stream));
        HIPC(c, hipGetLastError());
    }
    return VO_OK;
}

int vo_get_landmarks(vo_ctx* c, double* out, int capacity, int* rows)
{
    if (!c) return VO_ERR_ARG;
    int r = (int)(c->landmarks.size() / 3);
    if (rows) *rows = r;
    if (out) memcpy(out, c->landmarks.data(), sizeof(double) * 3 * std::min(r, capacity));
    return r > capacity && out ? fail(c, VO_ERR_CAPACITY, "vo_get_landmarks: %d rows exceed capacity %d", r, capacity) : VO_OK;
}

int vo_set_landmark_frame(vo_ctx* c, int camera)
{
    if (!c || (camera != 0 && camera != 1)) return fail(c, VO_ERR_ARG, "vo_set_landmark_frame: mode must be 0 (world) or 1 (camera)");
    if (!c->pending.empty()) return fail(c, VO_ERR_STATE, "vo_set_landmark_frame: batches pending");
    c->lm_camera = camera;
    c->landmarks.clear();
    c->lm_n = 0;
    c->lm_frame_off.assign(1, 0);
    return VO_OK;
}

int vo_get_landmark_rows(vo_ctx* c, float* X, uint8_t* keep, int capacity, int* rows)
{
    if (!c || capacity < 0) return fail(c, VO_ERR_ARG, "vo_get_landmark_rows: bad arguments");
    if (!c->lm_camera) return fail(c, VO_ERR_STATE, "vo_get_landmark_rows: context keeps world rows (vo_set_landmark_frame(ctx, 1) first)");
    if (!c->pending.empty()) return fail(c, VO_ERR_STATE, "vo_get_landmark_rows: batches pending");
    if (c->lm_n > (size_t)INT_MAX)    // the device store is size_t; this API counts in int (vo_landmarks_world_dev: long)
        return fail(c, VO_ERR_CAPACITY, "vo_get_landmark_rows: %zu rows exceed INT_MAX (use vo_landmarks_world_dev)", c->lm_n);
    const int r = (int)c->lm_n;
    if (rows) *rows = r;
    const int m = std::min(r, capacity);
    if (m > 0 && (X || keep)) {
        hipSetDevice(c->device);
        HIPC(c, hipStreamSynchronize(c->stream));
        if (X) HIPC(c, hipMemcpy(X, c->d_lmX, sizeof(float) * 3 * m, hipMemcpyDeviceToHost));
        if (keep) HIPC(c, hipMemcpy(keep, c->d_lmkeep, m, hipMemcpyDeviceToHost));
    }
    return r > capacity && (X || keep) ? fail(c, VO_ERR_CAPACITY, "vo_get_landmark_rows: %d rows exceed capacity %d", r, capacity) : VO_OK;
}

int vo_landmarks_world_dev(vo_ctx* c, const double* poses, int n_frames, float* d_out, long capacity, long* rows)
{
    if (!c || n_frames < 0 || capacity < 0 || (n_frames > 0 && !poses))
        return fail(c, VO_ERR_ARG, "vo_landmarks_world_dev: bad arguments");
    if (!c->lm_camera) return fail(c, VO_ERR_STATE, "vo_landmarks_world_dev: context keeps world rows (vo_set_landmark_frame(ctx, 1) first)");
    if (!c->pending.empty()) return fail(c, VO_ERR_STATE, "vo_landmarks_world_dev: batches pending");
    const int nf = (int)c->lm_frame_off.size() - 1;
    if (n_frames != nf)
        return fail(c, VO_ERR_ARG, "vo_landmarks_world_dev: %d poses for %d collected frames", n_frames, nf);
    const long r = (long)c->lm_n;
    if (rows) *rows = r;
    if (r == 0) return VO_OK;
    if (!d_out) return VO_OK;
    if (r > capacity) return fail(c, VO_ERR_CAPACITY, "vo_landmarks_world_dev: %ld rows exceed capacity %ld", r, capacity);
    hipSetDevice(c->device);
    if (nf > c->lmw_cap) {
        const int cap = std::max(nf, 1024);
        HIPC(c, (hipError_t)c->pool.grow({DevPool::req(c->d_lmw_pose, (size_t)16 * cap), DevPool::req(c->d_lmw_off, (size_t)cap + 1)}));
        c->lmw_cap = cap;
    }
    HIPC(c, hipMemcpyAsync(c->d_lmw_pose, poses, sizeof(double) * 16 * nf, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->d_lmw_off, c->lm_frame_off.data(), sizeof(long long) * (nf + 1), hipMemcpyHostToDevice,
                           c->stream));
    lm_world_launch(c->d_lmw_pose, c->d_lmw_off, nf, c->d_lmX, c->d_lmkeep, d_out, c->stream);
    const int rc = launch_status(c);
    if (rc) return rc;
    // d_out is read by the caller's streams (torch, RCCL) next: complete before returning
    HIPC(c, hipStreamSynchronize(c->stream));
    return VO_OK;
}

int vo_landmarks_to_world(const double pose[16], const float* X, const uint8_t* keep, int n, double* out)
{
    if (!pose || n < 0 || (n > 0 && (!X || !keep || !out))) return VO_ERR_ARG;
    for (int m = 0; m < n; ++m) {
        if (keep[m]) lm_world(pose, X + (size_t)m * 3, out + (size_t)m * 3);
        else out[3 * m] = out[3 * m + 1] = out[3 * m + 2] = 0.0;
    }
    return VO_OK;
}

int vo_chain_poses(const double* rel, const int32_t* status, int n, const double* pose0, double* out)
{
    if (n < 0 || (n > 0 && (!rel || !out))) return VO_ERR_ARG;
    double pose[16];
    memcpy(pose, pose0 ? pose0 : I4, sizeof(pose));
    for (int f = 0; f < n; ++f) {
        if (!status || status[f] == VO_OK) mat4_mul(pose, rel + (size_t)16 * f, pose);
        memcpy(out + (size_t)16 * f, pose, sizeof(pose));
    }
    return VO_OK;
}

int vo_landmarks_to_world_frames(const double* poses, const int32_t* rows_per_frame, int n_frames, const float* X,
                                 const uint8_t* keep, long n_rows, double* out)
{
    if (n_frames < 0 || n_rows < 0 || (n_frames > 0 && (!poses || !rows_per_frame))) return VO_ERR_ARG;
    long r = 0;
    for (int f = 0; f < n_frames; ++f) {
        const long k = rows_per_frame[f];
        if (k < 0 || r + k > n_rows) return VO_ERR_ARG;
        int rc = vo_landmarks_to_world(poses + (size_t)16 * f, X + 3 * r, keep + r, (int)k, out + 3 * r);
        if (rc) return rc;
        r += k;
    }
    return r == n_rows ? VO_OK : VO_ERR_ARG;
}

int vo_reset(vo_ctx* c)
{
    if (!c) return VO_ERR_ARG;
    hipSetDevice(c->device);
    // drops any pending asynchronous batches: wait for this context's streams only
    HIPC(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < vo_ctx::MAX_SUB; ++k) HIPC(c, hipStreamSynchronize(c->sub[k]));
    HIPC(c, hipStreamSynchronize(c->down));
    HIPC(c, hipStreamSynchronize(c->copy_stream));
    c->pending.clear();
    c->next_step_set = 0;
    c->next_slot = 0;
    for (void*& p : c->lm_retired) c->pool.release(p);
    c->lm_retired.clear();
    c->last_step_set = -1;
    c->have_features = false;
    c->frame_index = 0;
    memcpy(c->pose, I4, sizeof(I4));
    c->landmarks.clear();
    c->lm_n = 0;
    c->lm_frame_off.assign(1, 0);
    for (int k = 0; k < 2; ++k) HIPC(c, hipMemset(c->set[k].pair_n + c->max_batch, 0, sizeof(int)));
    return VO_OK;
}

int vo_set_frame_index(vo_ctx* c, long frame_index)
{
    if (!c || frame_index < 0) return VO_ERR_ARG;
    c->frame_index = frame_index;
    return VO_OK;
}

// Standalone calls use frame slot 0 and the carry slots: they invalidate the
// loop state of vo_step (call vo_reset before stepping again).
static int upload_desc(vo_ctx* c, int slot, const uint8_t* d, int n)
{
    const int K = c->set[0].sb.kp_cap;
    if (n) HIPC(c, hipMemcpyAsync(c->set[0].sb.desc + (size_t)slot * K * VO_DESC_LEN, d, (size_t)n * VO_DESC_LEN, hipMemcpyHostToDevice, c->stream));
    desc_meta_launch(c->set[0].sb.desc + (size_t)slot * K * VO_DESC_LEN, c->set[0].sb.meta + (size_t)slot * K, n, c->stream);
    HIPC(c, hipMemcpyAsync(c->set[0].sb.n_kp + slot, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));   // &n is a stack value
    return VO_OK;
}

int vo_track(vo_ctx* c, const uint8_t* old_l, const uint8_t* old_r, int n_old, const uint8_t* cur_l, int n_cl,
             const uint8_t* cur_r, int n_cr, uint32_t* idx_out, int capacity, int* K_out)
{
    if (!c || n_old < 0 || n_cl < 0 || n_cr < 0) return fail(c, VO_ERR_ARG, "vo_track: bad arguments");
    const int K = c->set[0].sb.kp_cap, M = c->max_batch;
    if (n_old > K || n_cl > K || n_cr > K) return fail(c, VO_ERR_CAPACITY, "vo_track: more rows than max_keypoints");
    CallScope call(c); if (call.status) return call.status;
    c->have_features = false;
    c->last_set = 0;                                   // set 0's descriptor slots are overwritten
    c->set[0].sel_used = false;
    int rc;
    if ((rc = upload_desc(c, 2 * M, old_l, n_old))) return rc;
    if ((rc = upload_desc(c, 2 * M + 1, old_r, n_old))) return rc;
    if ((rc = upload_desc(c, 0, cur_l, n_cl))) return rc;
    if ((rc = upload_desc(c, 1, cur_r, n_cr))) return rc;
    std::vector<int> iota(std::max(n_old, 1));
    for (int k = 0; k < n_old; ++k) iota[k] = k;
    if (n_old) {
        HIPC(c, hipMemcpy(c->set[0].pair_i + (size_t)M * K, iota.data(), sizeof(int) * n_old, hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(c->set[0].pair_j + (size_t)M * K, iota.data(), sizeof(int) * n_old, hipMemcpyHostToDevice));
    }
    HIPC(c, hipMemcpy(c->set[0].pair_n + M, &n_old, sizeof(int), hipMemcpyHostToDevice));
    StepArgs a = step_args(c, 1);
    track_enqueue(c->set[0].gb, c->set[0].mb, c->set[0].d_jobs + job_track(c, 0, 0), a, c->mp, c->stream);
    int n = 0;
    HIPC(c, hipMemcpyAsync(&n, c->set[0].gb.list_n + 3, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    rc = finish(c);
    if (rc) return rc;
    if (K_out) *K_out = n;
    const int m = std::min(n, capacity);
    if (m > 0 && idx_out) {
        std::vector<int> ol(m), cl(m), cr(m);
        HIPC(c, hipMemcpy(ol.data(), track_list(c->set[0].gb, 0, TL_OLF), sizeof(int) * m, hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(cl.data(), track_list(c->set[0].gb, 0, TL_CLF), sizeof(int) * m, hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(cr.data(), track_list(c->set[0].gb, 0, TL_CRF), sizeof(int) * m, hipMemcpyDeviceToHost));
        for (int k = 0; k < m; ++k) {
            idx_out[3 * k] = (uint32_t)ol[k] + 1;
            idx_out[3 * k + 1] = (uint32_t)cl[k] + 1;
            idx_out[3 * k + 2] = (uint32_t)cr[k] + 1;
        }
    }
    if (n > capacity) return fail(c, VO_ERR_CAPACITY, "vo_track: %d rows exceed capacity %d", n, capacity);
    return VO_OK;
}

// two [n][2] float arrays interleaved into quads out [n][4] = (a.x, a.y, b.x, b.y)
static void pack_quads(const float* a, const float* b, int n, float* out)
{
    for (int k = 0; k < n; ++k) { out[4 * k] = a[2 * k]; out[4 * k + 1] = a[2 * k + 1]; out[4 * k + 2] = b[2 * k]; out[4 * k + 3] = b[2 * k + 1]; }
}

// vo_triangulate / vo_triangulate_ex: chunks of max_keypoints points through set 0's frame slot 0,
// one k_tri_list each and, only when reproj_err or valid is asked for, one k_tri_quality
static int triangulate_chunks(vo_ctx* c, const char* who, const float* x1, const float* x2, int n, const double P1[12],
                              const double P2[12], double* X, float* reproj_err, uint8_t* valid)
{
    if (!c || n < 0 || (n && (!x1 || !x2 || !X)) || !P1 || !P2) return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
    CallScope call(c); if (call.status) return call.status;
    const bool quality = reproj_err || valid;
    int rc = quality && n > 0 ? tri_quality_buffers(c) : VO_OK;
    if (rc) return rc;
    const vo_calib cal = calib_of(P1, P2, nullptr);
    const int K = c->set[0].sb.kp_cap;
    const GeomBuffers& gb = c->set[0].gb;
    std::vector<float> q((size_t)std::min(n, K) * 4 + 4);
    for (int b = 0; b < n; b += K) {
        const int m = std::min(K, n - b);
        pack_quads(x1 + 2 * (size_t)b, x2 + 2 * (size_t)b, m, q.data());
        HIPC(c, hipMemcpyAsync(gb.oldpos, q.data(), sizeof(float) * 4 * m, hipMemcpyHostToDevice, c->stream));
        triangulate_launch(gb.oldpos, m, cal, gb.world, c->stream);
        if (quality) tri_quality_launch(gb.oldpos, gb.world, nullptr, 0, m, 1, K, cal, c->d_tq_err, c->d_tq_valid, c->stream);
        HIPC(c, hipMemcpyAsync(X + 3 * (size_t)b, gb.world, sizeof(double) * 3 * m, hipMemcpyDeviceToHost, c->stream));
        if (reproj_err) HIPC(c, hipMemcpyAsync(reproj_err + b, c->d_tq_err, sizeof(float) * m, hipMemcpyDeviceToHost, c->stream));
        if (valid) HIPC(c, hipMemcpyAsync(valid + b, c->d_tq_valid, (size_t)m, hipMemcpyDeviceToHost, c->stream));
        if ((rc = finish(c))) return rc;                // q is reused by the next chunk
    }
    return VO_OK;
}

int vo_triangulate(vo_ctx* c, const float* x1, const float* x2, int n, const double P1[12], const double P2[12], double* X)
{
    return triangulate_chunks(c, "vo_triangulate", x1, x2, n, P1, P2, X, nullptr, nullptr);
}

int vo_triangulate_ex(vo_ctx* c, const float* x1, const float* x2, int n, const double P1[12], const double P2[12], double* X,
                      float* reproj_err, uint8_t* valid)
{
    return triangulate_chunks(c, reproj_err || valid ? "vo_triangulate_ex" : "vo_triangulate", x1, x2, n, P1, P2, X, reproj_err, valid);
}

int vo_estworldpose(vo_ctx* c, const double* img, const double* world, int n, const double K9[9],
                    const vo_ransac_params* params, uint32_t frame_key, double T[16], uint8_t* inliers, int* n_inliers)
{
    if (!c || n < 0 || (n && (!img || !world)) || !K9 || !T) return fail(c, VO_ERR_ARG, "vo_estworldpose: bad arguments");
    if (n > c->set[0].sb.kp_cap) return fail(c, VO_ERR_CAPACITY, "vo_estworldpose: %d points exceed max_keypoints", n);
    const vo_ransac_params rp = params ? *params : c->rp;
    if (rp.max_num_trials > c->set[0].gb.n_hyp)
        return fail(c, VO_ERR_ARG, "vo_estworldpose: MaxNumTrials %d exceeds the context's %d hypothesis slots (vo_create ransac.max_num_trials)",
                    rp.max_num_trials, c->set[0].gb.n_hyp);
    if (n_inliers) *n_inliers = 0;
    if (n < 4) return fail(c, VO_ERR_TOO_FEW_POINTS, "estworldpose: need at least 4 points, got %d", n);
    CallScope call(c); if (call.status) return call.status;
    c->have_features = false;
    HIPC(c, hipMemcpyAsync(c->set[0].gb.imgpt, img, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->set[0].gb.world, world, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->d_fn, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
    estworldpose_launch(c->set[0].gb, c->set[0].gb.imgpt, c->set[0].gb.world, c->d_fn, K9, rp, frame_key, c->stream);
    FrameGeom g;
    HIPC(c, hipMemcpyAsync(&g, c->set[0].gb.fg, sizeof(g), hipMemcpyDeviceToHost, c->stream));
    if (inliers) HIPC(c, hipMemcpyAsync(inliers, c->set[0].gb.inliers, n, hipMemcpyDeviceToHost, c->stream));
    int rc = finish(c);
    if (rc) return rc;
    memcpy(T, g.T, sizeof(g.T));
    if (n_inliers) *n_inliers = g.n_inliers;
    if (g.status == VO_ERR_NO_CONSENSUS) return fail(c, g.status, "estworldpose: no consensus (MSAC found no model with >= 4 inliers)");
    if (g.status != VO_OK) return fail(c, g.status, "estworldpose failed (%d)", g.status);
    return VO_OK;
}

// -> nullptr when the block is inside the ranges of include/vo.h, else the offending field
static const char* refine_params_refusal(const vo_refine_params& p)
{
    if (p.max_iterations < 1 || p.max_iterations > 100) return "max_iterations";
    if (!(p.relative_tolerance >= 0.0 && p.relative_tolerance - p.relative_tolerance == 0.0)) return "relative_tolerance";
    if (!(p.absolute_tolerance >= 0.0 && p.absolute_tolerance - p.absolute_tolerance == 0.0)) return "absolute_tolerance";
    if (!(p.lambda0 >= VO_REFINE_LAMBDA_MIN && p.lambda0 <= VO_REFINE_LAMBDA_MAX)) return "lambda0";
    return nullptr;
}

// index of the first non-finite value, or -1
static long first_non_finite(const double* v, long n)
{
    for (long i = 0; i < n; ++i)
        if (!(v[i] - v[i] == 0.0)) return i;
    return -1;
}

int vo_refine_pose(vo_ctx* c, const double* img, const double* world, int n, const uint8_t* use, const double K9[9],
                   const double T_in[16], const vo_refine_params* params, double T_out[16], vo_refine_stats* stats)
{
    if (!c || n < 0 || (n && (!img || !world)) || !K9 || !T_in || !T_out) return fail(c, VO_ERR_ARG, "vo_refine_pose: bad arguments");
    const int cap = c->set[0].sb.kp_cap;
    if (n > cap) return fail(c, VO_ERR_CAPACITY, "vo_refine_pose: %d points exceed max_keypoints", n);
    vo_refine_params p;
    if (params) p = *params; else vo_default_refine_params(&p);
    if (const char* field = refine_params_refusal(p)) return fail(c, VO_ERR_ARG, "vo_refine_pose: parameter out of range: %s", field);
    long bad;
    if ((bad = first_non_finite(img, 2L * n)) >= 0)
        return fail(c, VO_ERR_ARG, "vo_refine_pose: imagePoints(%ld, %ld) is not finite (point index %ld)", bad / 2 + 1, bad % 2 + 1, bad / 2);
    if ((bad = first_non_finite(world, 3L * n)) >= 0)
        return fail(c, VO_ERR_ARG, "vo_refine_pose: worldPoints(%ld, %ld) is not finite (point index %ld)", bad / 3 + 1, bad % 3 + 1, bad / 3);
    if ((bad = first_non_finite(K9, 9)) >= 0) return fail(c, VO_ERR_ARG, "vo_refine_pose: K[%ld] is not finite", bad);
    if ((bad = first_non_finite(T_in, 16)) >= 0) return fail(c, VO_ERR_ARG, "vo_refine_pose: T_in[%ld] is not finite", bad);
    if (T_in[12] != 0.0 || T_in[13] != 0.0 || T_in[14] != 0.0 || T_in[15] != 1.0)
        return fail(c, VO_ERR_ARG, "vo_refine_pose: the last row of T_in is not 0 0 0 1");
    CallScope call(c); if (call.status) return call.status;
    if (n == 0) {                                       // nothing to launch: the pass over no points
        memcpy(T_out, T_in, sizeof(double) * 16);
        if (stats) *stats = vo_refine_stats{VO_REFINE_TOO_FEW, 0, 1, 0, 0.0, 0.0};
        return VO_OK;
    }
    GeomBuffers& gb = c->set[0].gb;
    HIPC(c, geom_alloc_refine(c->pool, gb));
    c->have_features = false;
    c->set[0].refine_used = false;                      // slot 0 of the set's stats is overwritten
    std::vector<uint8_t> ones;
    if (!use) { ones.assign((size_t)n, 1); use = ones.data(); }
    HIPC(c, hipMemcpyAsync(gb.imgpt, img, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(gb.world, world, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(gb.inliers, use, (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->d_fn, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync((char*)gb.fg + offsetof(FrameGeom, T), T_in, sizeof(double) * 16, hipMemcpyHostToDevice, c->stream));
    refine_launch(gb, gb.imgpt, gb.world, gb.inliers, c->d_fn, 0, K9, p, 1, 0, c->stream);
    FrameGeom g;
    vo_refine_stats st;
    HIPC(c, hipMemcpyAsync(&g, gb.fg, sizeof(g), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(&st, gb.refine, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    int rc = finish(c);
    if (rc) return rc;
    memcpy(T_out, g.T, sizeof(g.T));
    if (stats) *stats = st;
    return VO_OK;
}

int vo_set_pose_refinement(vo_ctx* c, const vo_refine_params* p)
{
    if (!c) return VO_ERR_ARG;
    if (!c->pending.empty()) return fail(c, VO_ERR_STATE, "vo_set_pose_refinement: step batches pending (vo_step_collect first)");
    if (!p) { c->refine_on = false; return VO_OK; }
    if (const char* field = refine_params_refusal(*p))
        return fail(c, VO_ERR_ARG, "vo_set_pose_refinement: parameter out of range: %s", field);
    hipSetDevice(c->device);
    for (int k = 0; k < 2; ++k) HIPC(c, geom_alloc_refine(c->pool, c->set[k].gb));
    c->refine = *p;
    c->refine_on = true;
    return VO_OK;
}

int vo_fetch_pose_refinement(vo_ctx* c, int frame, vo_refine_stats* out)
{
    if (!c || !out) return fail(c, VO_ERR_ARG, "vo_fetch_pose_refinement: bad arguments");
    const vo_ctx::BufferSet* Sp = nullptr;
    int rc = collected_set(c, frame, "vo_fetch_pose_refinement", &Sp);
    if (rc) return rc;
    const vo_ctx::BufferSet& S = *Sp;
    if (!S.refine_used || !S.gb.refine)
        return fail(c, VO_ERR_STATE, "vo_fetch_pose_refinement: the batch ran without pose refinement (vo_set_pose_refinement)");
    HIPC(c, hipMemcpy(out, S.gb.refine + frame, sizeof(*out), hipMemcpyDeviceToHost));
    return VO_OK;
}

// -> nullptr when the block is inside the ranges of include/vo.h, else the offending field
static const char* fund_params_refusal(const vo_fund_params& p)
{
    if (p.method != VO_FUND_NORM8 && p.method != VO_FUND_MSAC) return "method (VO_FUND_NORM8 or VO_FUND_MSAC)";
    if (p.num_trials < 1 || p.num_trials > 100000) return "num_trials";
    if (!(p.distance_threshold > 0.0 && p.distance_threshold - p.distance_threshold == 0.0)) return "distance_threshold";
    if (!(p.confidence > 0.0 && p.confidence < 100.0)) return "confidence";
    return nullptr;
}

int vo_est_fundamental_batch(vo_ctx* c, const float* x1, const float* x2, int pts_stride, const int32_t* n_pts, int B,
                             const vo_fund_params* params, uint32_t key0, double* F, uint8_t* inliers, int32_t* n_inliers,
                             int32_t* status)
{
    const char* who = "vo_est_fundamental";
    if (!c || B < 0 || pts_stride < 0 || (B && (!n_pts || !F || !status))) return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
    if (B > c->max_batch) return fail(c, VO_ERR_CAPACITY, "%s: %d problems exceed max_batch %d", who, B, c->max_batch);
    if (pts_stride > c->set[0].sb.kp_cap) return fail(c, VO_ERR_CAPACITY, "%s: %d points exceed max_keypoints", who, pts_stride);
    vo_fund_params p;
    if (params) p = *params; else vo_default_fund_params(&p);
    if (const char* field = fund_params_refusal(p)) return fail(c, VO_ERR_ARG, "%s: parameter out of range: %s", who, field);
    bool any = false;
    for (int f = 0; f < B; ++f) {
        const int n = n_pts[f];
        if (n < 0 || n > pts_stride) return fail(c, VO_ERR_ARG, "%s: n_pts[%d] = %d is outside 0 .. pts_stride", who, f, n);
        if (n && (!x1 || !x2)) return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
        for (int side = 0; side < 2; ++side) {
            const float* x = (side ? x2 : x1) + (size_t)f * pts_stride * 2;
            for (long e = 0; e < 2L * n; ++e)
                if (!std::isfinite(x[e]))
                    return fail(c, VO_ERR_ARG, "%s: matchedPoints%d(%ld, %ld) of problem %d is not finite (point index %ld)", who,
                                side + 1, e / 2 + 1, e % 2 + 1, f, e / 2);
        }
        any = any || n >= VO_FUND_SAMPLE;
    }
    CallScope call(c); if (call.status) return call.status;
    for (int f = 0; f < B; ++f) {                           // what a problem with n < 8 gives; the rest is overwritten
        for (int q = 0; q < 9; ++q) F[9 * (size_t)f + q] = 0.0;
        status[f] = VO_ERR_TOO_FEW_POINTS;
        if (n_inliers) n_inliers[f] = 0;
    }
    if (inliers && B) memset(inliers, 0, (size_t)B * pts_stride);
    if (!any) return VO_OK;                                 // nothing to launch
    FundBuffers& fb = c->fund;
    {
        const hipError_t e = fund_reserve(c->pool, fb, B, pts_stride);
        if (e != hipSuccess) return fail(c, VO_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    const size_t pts = (size_t)B * pts_stride;
    HIPC(c, hipMemcpyAsync(fb.x1, x1, sizeof(float) * 2 * pts, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(fb.x2, x2, sizeof(float) * 2 * pts, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(fb.n, n_pts, sizeof(int) * B, hipMemcpyHostToDevice, c->stream));
    fund_launch(fb, B, pts_stride, p, key0, c->stream);
    std::vector<FundOut> out((size_t)B);
    HIPC(c, hipMemcpyAsync(out.data(), fb.out, sizeof(FundOut) * B, hipMemcpyDeviceToHost, c->stream));
    if (inliers) HIPC(c, hipMemcpyAsync(inliers, fb.inliers, pts, hipMemcpyDeviceToHost, c->stream));
    int rc = finish(c);
    if (rc) return rc;
    for (int f = 0; f < B; ++f) {
        memcpy(F + 9 * (size_t)f, out[f].F, sizeof(double) * 9);
        status[f] = out[f].status;
        if (n_inliers) n_inliers[f] = out[f].n_inliers;
    }
    return VO_OK;
}

int vo_est_fundamental(vo_ctx* c, const float* x1, const float* x2, int n, const vo_fund_params* params, uint32_t key,
                       double F[9], uint8_t* inliers, int* n_inliers)
{
    if (!c || n < 0 || !F) return fail(c, VO_ERR_ARG, "vo_est_fundamental: bad arguments");
    if (n > c->set[0].sb.kp_cap) return fail(c, VO_ERR_CAPACITY, "vo_est_fundamental: %d points exceed max_keypoints", n);
    int32_t n32 = n, nin = 0, st = VO_OK;
    int rc = vo_est_fundamental_batch(c, x1, x2, n, &n32, 1, params, key, F, inliers, &nin, &st);
    if (n_inliers) *n_inliers = nin;
    if (rc) return rc;
    if (st == VO_ERR_TOO_FEW_POINTS) return fail(c, st, "estimateFundamentalMatrix: need at least 8 points, got %d", n);
    if (st == VO_ERR_NO_CONSENSUS) return fail(c, st, "estimateFundamentalMatrix: no consensus (no model with >= 8 inliers)");
    return st;
}

// ---- vision.PointTracker (vo.h: "pyramidal Lucas-Kanade point tracking") -----------------------
// -> nullptr when the block is inside the ranges of include/vo.h, else the offending field
static const char* klt_params_refusal(const vo_klt_params& p)
{
    if (p.num_pyramid_levels < 1 || p.num_pyramid_levels > VO_KLT_MAX_LEVELS) return "num_pyramid_levels (1 .. 6)";
    for (int k = 0; k < 2; ++k)
        if (p.block_size[k] < VO_KLT_MIN_WIN || p.block_size[k] > VO_KLT_MAX_WIN || !(p.block_size[k] & 1))
            return k ? "block_size[1] (odd, 5 .. 31)" : "block_size[0] (odd, 5 .. 31)";
    if (p.max_iterations < 1 || p.max_iterations > VO_KLT_MAX_ITER) return "max_iterations (1 .. 50)";
    if (!(p.max_bidirectional_error > 0.0f)) return "max_bidirectional_error (> 0 or +inf)";
    return nullptr;
}

int vo_track_points_batch(vo_ctx* c, const uint8_t* imgs0, const uint8_t* imgs1, int ld, int col_major, int n_pairs,
                          const float* pts0, const float* guess, const int32_t* n_pts, int pts_stride,
                          const vo_klt_params* params, float* pts1, uint8_t* valid, float* scores, vo_klt_info* info)
{
    const char* who = "vo_track_points";
    if (!c || !imgs0 || !imgs1 || !n_pts || n_pairs < 1 || pts_stride < 0 || (col_major != 0 && col_major != 1) ||
        ld < (col_major ? c->rows : c->cols))
        return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
    // every refusal before anything is enqueued
    if (n_pairs > c->max_batch) return fail(c, VO_ERR_CAPACITY, "%s: %d pairs exceed max_batch %d", who, n_pairs, c->max_batch);
    if (!c->pending.empty()) return fail(c, VO_ERR_STATE, "asynchronous step batches pending (vo_step_collect first)");
    const int K = c->set[0].sb.kp_cap;
    vo_klt_params p;
    if (params) p = *params; else vo_default_klt_params(&p);
    if (const char* field = klt_params_refusal(p)) return fail(c, VO_ERR_ARG, "%s: parameter out of range: %s", who, field);
    int max_n = 0;
    for (int f = 0; f < n_pairs; ++f) {
        const int n = n_pts[f];
        if (n < 0 || n > pts_stride) return fail(c, VO_ERR_ARG, "%s: n_pts[%d] = %d is outside 0 .. pts_stride = %d", who, f, n, pts_stride);
        if (n > K) return fail(c, VO_ERR_CAPACITY, "%s: pair %d has %d points, more than max_keypoints %d", who, f, n, K);
        max_n = std::max(max_n, n);
    }
    if (max_n > 0 && (!pts0 || !pts1 || !valid)) return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
    for (int f = 0; f < n_pairs; ++f)
        for (int which = 0; which < (guess ? 2 : 1); ++which) {
            const float* x = (which ? guess : pts0) + (size_t)f * pts_stride * 2;
            for (long e = 0; e < 2L * n_pts[f]; ++e)
                if (!std::isfinite(x[e]) || !(std::fabs(x[e]) < 1048576.0f))
                    return fail(c, VO_ERR_ARG, "%s: %s(%ld, %ld) of pair %d must be finite and below 2^20 in magnitude (point index %ld)",
                                who, which ? "guess" : "points", e / 2 + 1, e % 2 + 1, f, e / 2);
        }
    if (max_n == 0) return VO_OK;                            // nothing to track: nothing is launched
    CallScope call(c); if (call.status) return call.status;
    KltBuffers& kb = c->klt;
    {
        const hipError_t e = klt_reserve(c->pool, kb, c->rows, c->cols, n_pairs, pts_stride);
        if (e != hipSuccess) return fail(c, VO_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    const size_t fs = (size_t)c->rows * c->cols, pts = (size_t)n_pairs * pts_stride;
    for (int which = 0; which < 2; ++which) {                // level 0: the images themselves, img0s then img1s
        const uint8_t* src = which ? imgs1 : imgs0;
        uint8_t* dst = kb.planes + (size_t)which * n_pairs * fs;
        if (!col_major && ld == c->cols) HIPC(c, hipMemcpyAsync(dst, src, fs * n_pairs, hipMemcpyHostToDevice, c->stream));
        else { int rc = stage_images(c, src, ld, col_major, n_pairs, dst); if (rc) return rc; }
    }
    HIPC(c, hipMemcpyAsync(kb.pts0, pts0, sizeof(float) * 2 * pts, hipMemcpyHostToDevice, c->stream));
    if (guess) HIPC(c, hipMemcpyAsync(kb.guess, guess, sizeof(float) * 2 * pts, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(kb.n, n_pts, sizeof(int) * n_pairs, hipMemcpyHostToDevice, c->stream));
    klt_pyr_launch(kb, c->rows, c->cols, n_pairs, p.num_pyramid_levels, c->stream);
    klt_track_launch(kb, c->rows, c->cols, n_pairs, pts_stride, max_n, guess != nullptr, p, c->stream);
    kb.last_pairs = n_pairs; kb.last_levels = p.num_pyramid_levels;
    // rows beyond n_pts[f] stay as the caller has them: pair by pair
    for (int f = 0; f < n_pairs; ++f) {
        const size_t o = (size_t)f * pts_stride, n = (size_t)n_pts[f];
        if (!n) continue;
        HIPC(c, hipMemcpyAsync(pts1 + 2 * o, kb.pts1 + 2 * o, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(valid + o, kb.valid + o, n, hipMemcpyDeviceToHost, c->stream));
        if (scores) HIPC(c, hipMemcpyAsync(scores + o, kb.scores + o, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
        if (info) HIPC(c, hipMemcpyAsync(info + o, kb.info + o, sizeof(vo_klt_info) * n, hipMemcpyDeviceToHost, c->stream));
    }
    return finish(c);
}

int vo_track_points(vo_ctx* c, const uint8_t* img0, const uint8_t* img1, int rows, int cols, int ld, int col_major,
                    const float* pts0, const float* guess, int n, const vo_klt_params* params, float* pts1, uint8_t* valid,
                    float* scores, vo_klt_info* info)
{
    if (!c || rows != c->rows || cols != c->cols || n < 0) return fail(c, VO_ERR_ARG, "vo_track_points: bad arguments");
    if (n > c->set[0].sb.kp_cap) return fail(c, VO_ERR_CAPACITY, "vo_track_points: %d points exceed max_keypoints", n);
    const int32_t cnt = n;
    return vo_track_points_batch(c, img0, img1, ld, col_major, 1, pts0, guess, &cnt, n, params, pts1, valid, scores, info);
}

int vo_fetch_klt_level(vo_ctx* c, int image, int level, uint8_t* out, int capacity, int* rows, int* cols)
{
    if (!c || image < 0 || level < 0) return fail(c, VO_ERR_ARG, "vo_fetch_klt_level: bad arguments");
    const KltBuffers& kb = c->klt;
    if (kb.last_pairs == 0) return fail(c, VO_ERR_STATE, "vo_fetch_klt_level: no vo_track_points call has launched yet");
    if (image >= 2 * kb.last_pairs || level >= kb.last_levels)
        return fail(c, VO_ERR_ARG, "vo_fetch_klt_level: image %d, level %d outside the last call's %d images, %d levels", image, level,
                    2 * kb.last_pairs, kb.last_levels);
    const int r = vo_klt_level_dim(c->rows, level), q = vo_klt_level_dim(c->cols, level);
    if (rows) *rows = r;
    if (cols) *cols = q;
    if (!out || capacity < r * q) return fail(c, VO_ERR_CAPACITY, "vo_fetch_klt_level: %d bytes needed", r * q);
    CallScope call(c); if (call.status) return call.status;
    const size_t i = (size_t)(image & 1) * kb.last_pairs + (image >> 1);
    HIPC(c, hipMemcpyAsync(out, kb.planes + klt_level_offset(c->rows, c->cols, kb.last_pairs, level) + i * r * q, (size_t)r * q,
                           hipMemcpyDeviceToHost, c->stream));
    return finish(c);
}

// ---- detectMinEigenFeatures / detectHarrisFeatures (vo.h: "cornerPoints") ------------------------
// -> nullptr when the block is inside the ranges of include/vo.h, else the offending field; roi0 = the
// ROI 0-based (the whole image for w = 0)
static const char* corner_params_refusal(const vo_corner_params& p, int rows, int cols, int max_keypoints, int* roi0)
{
    if (p.method != VO_CORNER_MINEIG && p.method != VO_CORNER_HARRIS) return "method (VO_CORNER_MINEIG | VO_CORNER_HARRIS)";
    if (p.filter_size < VO_CORNER_MIN_FILTER || p.filter_size > VO_CORNER_MAX_FILTER || !(p.filter_size & 1))
        return "filter_size (odd, 3 .. 15)";
    if (!(p.min_quality >= 0.0f && p.min_quality <= 1.0f)) return "min_quality (0 .. 1)";
    if (p.strongest < 0 || p.strongest > max_keypoints) return "strongest (0, or 1 .. max_keypoints)";
    if (p.roi[2] == 0) { roi0[0] = 0; roi0[1] = 0; roi0[2] = cols; roi0[3] = rows; return nullptr; }
    if (p.roi[2] < 1 || p.roi[3] < 1) return "roi (w, h >= 1)";
    if (p.roi[0] < 1 || p.roi[1] < 1 || p.roi[0] > cols || p.roi[1] > rows || p.roi[2] > cols - (p.roi[0] - 1) ||
        p.roi[3] > rows - (p.roi[1] - 1))
        return "roi (x y w h, 1-based, inside the image)";
    roi0[0] = p.roi[0] - 1; roi0[1] = p.roi[1] - 1; roi0[2] = p.roi[2]; roi0[3] = p.roi[3];
    return nullptr;
}

int vo_detect_corners_batch(vo_ctx* c, const uint8_t* imgs, int ld, int col_major, int n_img, const vo_corner_params* params,
                            float* loc, float* metric, int stride, int32_t* n_out, int32_t* status)
{
    const char* who = "vo_detect_corners";
    if (!c || !imgs || !n_out || !status || n_img < 1 || n_img > 2 * c->max_batch || stride < 0 || (stride > 0 && (!loc || !metric)) ||
        (col_major != 0 && col_major != 1) || ld < (col_major ? c->rows : c->cols))
        return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
    // every refusal before anything is enqueued
    if (!c->pending.empty()) return fail(c, VO_ERR_STATE, "asynchronous step batches pending (vo_step_collect first)");
    const int K = c->set[0].sb.kp_cap;
    vo_corner_params p;
    if (params) p = *params; else vo_default_corner_params(&p);
    int roi0[4];
    if (const char* field = corner_params_refusal(p, c->rows, c->cols, K, roi0))
        return fail(c, VO_ERR_ARG, "%s: parameter out of range: %s", who, field);
    CallScope call(c); if (call.status) return call.status;
    CornerBuffers& cb = c->corner;
    {
        const hipError_t e = corner_reserve(c->pool, cb, c->rows, c->cols, n_img, 4 * K);
        if (e != hipSuccess) return fail(c, VO_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    const size_t fs = (size_t)c->rows * c->cols;
    if (!col_major && ld == c->cols) HIPC(c, hipMemcpyAsync(cb.img, imgs, fs * n_img, hipMemcpyHostToDevice, c->stream));
    else { int rc = stage_images(c, imgs, ld, col_major, n_img, cb.img); if (rc) return rc; }
    HIPC(c, corner_launch(cb, c->rows, c->cols, n_img, p, roi0, c->stream));
    cb.last_img = n_img;
    std::vector<int> total((size_t)n_img);
    HIPC(c, hipMemcpyAsync(total.data(), cb.total, sizeof(int) * n_img, hipMemcpyDeviceToHost, c->stream));
    int rc = finish(c);
    if (rc) return rc;
    const float* d_loc = p.strongest > 0 ? cb.sloc : cb.loc;
    const float* d_met = p.strongest > 0 ? cb.smet : cb.met;
    for (int i = 0; i < n_img; ++i) {
        const int count = total[i];
        const int n_ret = p.strongest > 0 ? std::min(count, p.strongest) : count;
        if (count > cb.list_cap || n_ret > stride) {
            n_out[i] = count > cb.list_cap ? count : n_ret;
            status[i] = VO_ERR_CAPACITY;
            continue;
        }
        n_out[i] = n_ret; status[i] = VO_OK;
        if (!n_ret) continue;
        HIPC(c, hipMemcpy(loc + (size_t)i * stride * 2, d_loc + (size_t)i * cb.list_cap * 2, sizeof(float) * 2 * n_ret, hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(metric + (size_t)i * stride, d_met + (size_t)i * cb.list_cap, sizeof(float) * n_ret, hipMemcpyDeviceToHost));
    }
    return VO_OK;
}

int vo_detect_corners(vo_ctx* c, const uint8_t* img, int rows, int cols, int ld, int col_major, const vo_corner_params* params,
                      float* loc, float* metric, int capacity, int* n_out)
{
    if (!c || rows != c->rows || cols != c->cols || capacity < 0 || !n_out) return fail(c, VO_ERR_ARG, "vo_detect_corners: bad arguments");
    int32_t n = 0, st = VO_OK;
    const int rc = vo_detect_corners_batch(c, img, ld, col_major, 1, params, loc, metric, capacity, &n, &st);
    if (rc) return rc;
    *n_out = n;
    if (st == VO_ERR_CAPACITY)
        return fail(c, VO_ERR_CAPACITY, "vo_detect_corners: %d corners exceed the device list (%d = 4 x max_keypoints) or the capacity %d", n,
                    c->corner.list_cap, capacity);
    return st;
}

int vo_fetch_corner_metric(vo_ctx* c, int image, float* out, int capacity)
{
    if (!c || image < 0) return fail(c, VO_ERR_ARG, "vo_fetch_corner_metric: bad arguments");
    const CornerBuffers& cb = c->corner;
    if (cb.last_img == 0) return fail(c, VO_ERR_STATE, "vo_fetch_corner_metric: no vo_detect_corners call has launched yet");
    if (image >= cb.last_img) return fail(c, VO_ERR_ARG, "vo_fetch_corner_metric: image %d outside the last call's %d images", image, cb.last_img);
    const size_t fs = (size_t)c->rows * c->cols;
    if (!out || capacity < 0 || (size_t)capacity < fs) return fail(c, VO_ERR_CAPACITY, "vo_fetch_corner_metric: %zu floats needed", fs);
    CallScope call(c); if (call.status) return call.status;
    HIPC(c, hipMemcpyAsync(out, cb.metric + (size_t)image * fs, sizeof(float) * fs, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
}

// ---- disparitySGM / reconstructScene (vo.h: "dense stereo depth") ---------------------------------
// -> nullptr when the block is inside the ranges of include/vo.h, else the offending field
static const char* sgm_params_refusal(const vo_sgm_params& p)
{
    const int lo = p.disparity_range[0], hi = p.disparity_range[1];
    if (lo < -1024 || hi > 1024 || lo >= hi) return "disparity_range (-1024 <= min < max <= 1024)";
    if ((hi - lo) % 8 != 0 || hi - lo > VO_SGM_MAX_D) return "disparity_range (max - min in 8, 16, .. 128)";
    if (p.uniqueness_threshold < 0 || p.uniqueness_threshold > 100) return "uniqueness_threshold (0 .. 100)";
    if (p.p1 < 0 || p.p1 > 255) return "p1 (0 .. 255)";
    if (p.p2 < p.p1 || p.p2 > 255) return "p2 (p1 .. 255)";
    return nullptr;
}

// the host entries: n_pairs pairs in groups of VO_SGM_GROUP through the staging of one group; ld_out is
// honoured for one pair, a batch's output is tightly packed
static int sgm_host(vo_ctx* c, const char* who, const uint8_t* lefts, const uint8_t* rights, int ld, int col_major, int n_pairs,
                    const vo_sgm_params* params, float* disp, int ld_out)
{
    if (!c || !lefts || !rights || !disp || n_pairs < 1 || n_pairs > (1 << 19) || (col_major != 0 && col_major != 1) ||
        ld < (col_major ? c->rows : c->cols) || ld_out < (col_major ? c->rows : c->cols))
        return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
    // every refusal before anything is enqueued
    if (!c->pending.empty()) return fail(c, VO_ERR_STATE, "asynchronous step batches pending (vo_step_collect first)");
    vo_sgm_params p;
    if (params) p = *params; else vo_default_sgm_params(&p);
    if (const char* field = sgm_params_refusal(p)) return fail(c, VO_ERR_ARG, "%s: parameter out of range: %s", who, field);
    CallScope call(c); if (call.status) return call.status;
    SgmBuffers& sb = c->sgm;
    const int rows = c->rows, cols = c->cols, D = p.disparity_range[1] - p.disparity_range[0];
    const int G = std::min(n_pairs, VO_SGM_GROUP);
    {
        if (G > sb.cap_pairs || D > sb.cap_D || G > sb.cap_io)
            HIPC(c, hipStreamSynchronize(c->stream));          // the old buffers' last reader (a _batch_dev call is not synchronised)
        const hipError_t e = sgm_reserve(c->pool, sb, rows, cols, G, D, true);
        if (e != hipSuccess) return fail(c, VO_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    const size_t fs = (size_t)rows * cols;
    const int major = col_major ? rows : cols, minor = col_major ? cols : rows;     // the output's contiguous and strided extents
    for (int g0 = 0; g0 < n_pairs; g0 += VO_SGM_GROUP) {
        const int g = std::min(VO_SGM_GROUP, n_pairs - g0);
        uint8_t* d_l = sb.img;
        uint8_t* d_r = sb.img + (size_t)sb.cap_io * fs;
        for (int which = 0; which < 2; ++which) {
            const uint8_t* src = (which ? rights : lefts) + (size_t)g0 * ld * (col_major ? cols : rows);
            uint8_t* dst = which ? d_r : d_l;
            if (!col_major && ld == cols) HIPC(c, hipMemcpyAsync(dst, src, fs * g, hipMemcpyHostToDevice, c->stream));
            else { int rc = stage_images(c, src, ld, col_major, g, dst); if (rc) return rc; }
        }
        sgm_launch(sb, d_l, d_r, rows, cols, g, p, col_major, sb.disp, c->stream);
        sb.last_pairs = g; sb.last_first = g0; sb.last_D = D;
        if (n_pairs == 1)
            HIPC(c, hipMemcpy2DAsync(disp, sizeof(float) * ld_out, sb.disp, sizeof(float) * major, sizeof(float) * major, minor,
                                     hipMemcpyDeviceToHost, c->stream));
        else
            HIPC(c, hipMemcpyAsync(disp + (size_t)g0 * fs, sb.disp, sizeof(float) * fs * g, hipMemcpyDeviceToHost, c->stream));
    }
    return finish(c);
}

int vo_disparity_sgm(vo_ctx* c, const uint8_t* left, const uint8_t* right, int rows, int cols, int ld, int col_major,
                     const vo_sgm_params* params, float* disp, int ld_out)
{
    if (!c || rows != c->rows || cols != c->cols) return fail(c, VO_ERR_ARG, "vo_disparity_sgm: bad arguments");
    return sgm_host(c, "vo_disparity_sgm", left, right, ld, col_major, 1, params, disp, ld_out);
}

int vo_disparity_sgm_batch(vo_ctx* c, const uint8_t* lefts, const uint8_t* rights, int ld, int col_major, int n_pairs,
                           const vo_sgm_params* params, float* disp)
{
    if (!c) return VO_ERR_ARG;
    if (n_pairs == 1 && (col_major == 0 || col_major == 1))       // the single call's copy with a tight stride
        return sgm_host(c, "vo_disparity_sgm_batch", lefts, rights, ld, col_major, 1, params, disp, col_major ? c->rows : c->cols);
    return sgm_host(c, "vo_disparity_sgm_batch", lefts, rights, ld, col_major, n_pairs, params, disp, 1 << 30);
}

int vo_disparity_sgm_batch_dev(vo_ctx* c, const uint8_t* d_lefts, const uint8_t* d_rights, int B, const vo_sgm_params* params,
                               float* d_disp)
{
    const char* who = "vo_disparity_sgm_batch_dev";
    if (!c || !d_lefts || !d_rights || !d_disp || B < 1 || B > (1 << 19)) return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
    if (!c->pending.empty()) return fail(c, VO_ERR_STATE, "asynchronous step batches pending (vo_step_collect first)");
    vo_sgm_params p;
    if (params) p = *params; else vo_default_sgm_params(&p);
    if (const char* field = sgm_params_refusal(p)) return fail(c, VO_ERR_ARG, "%s: parameter out of range: %s", who, field);
    CallScope call(c, false); if (call.status) return call.status;
    SgmBuffers& sb = c->sgm;
    const int D = p.disparity_range[1] - p.disparity_range[0];
    if (std::min(B, VO_SGM_GROUP) > sb.cap_pairs || D > sb.cap_D) {
        HIPC(c, hipStreamSynchronize(c->stream));              // the old workspace's last reader
        const hipError_t e = sgm_reserve(c->pool, sb, c->rows, c->cols, std::min(B, VO_SGM_GROUP), D, false);
        if (e != hipSuccess) return fail(c, VO_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    const size_t fs = (size_t)c->rows * c->cols;
    for (int g0 = 0; g0 < B; g0 += VO_SGM_GROUP) {
        const int g = std::min(VO_SGM_GROUP, B - g0);
        sgm_launch(sb, d_lefts + (size_t)g0 * fs, d_rights + (size_t)g0 * fs, c->rows, c->cols, g, p, 0, d_disp + (size_t)g0 * fs, c->stream);
        sb.last_pairs = g; sb.last_first = g0; sb.last_D = D;
    }
    return launch_status(c);                            // profiling events are collected by vo_kernel_times
}

int vo_fetch_sgm_cost(vo_ctx* c, int pair, uint16_t* S, long capacity)
{
    if (!c || pair < 0) return fail(c, VO_ERR_ARG, "vo_fetch_sgm_cost: bad arguments");
    const SgmBuffers& sb = c->sgm;
    if (sb.last_pairs == 0) return fail(c, VO_ERR_STATE, "vo_fetch_sgm_cost: no vo_disparity_sgm call has launched yet");
    if (pair < sb.last_first || pair >= sb.last_first + sb.last_pairs)
        return fail(c, VO_ERR_ARG, "vo_fetch_sgm_cost: pair %d outside the last call's last group, pairs %d .. %d", pair, sb.last_first,
                    sb.last_first + sb.last_pairs - 1);
    const size_t n = (size_t)c->rows * c->cols * sb.last_D;
    if (!S || capacity < 0 || (size_t)capacity < n) return fail(c, VO_ERR_CAPACITY, "vo_fetch_sgm_cost: %zu values needed", n);
    CallScope call(c); if (call.status) return call.status;
    HIPC(c, hipMemcpyAsync(S, sb.S + (size_t)(pair - sb.last_first) * n, sizeof(uint16_t) * n, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
}

int vo_reprojection_matrix(const double P1[12], const double P2[12], double Q[16])
{
    if (!P1 || !P2 || !Q) return VO_ERR_ARG;
    return vo_reprojection_from_projections(P1, P2, Q) ? VO_ERR_ARG : VO_OK;
}

int vo_reconstruct_scene(vo_ctx* c, const float* disp, int rows, int cols, int ld, int col_major, const double Q[16], float* xyz)
{
    const char* who = "vo_reconstruct_scene";
    if (!c || !disp || !Q || !xyz || rows != c->rows || cols != c->cols || (col_major != 0 && col_major != 1) ||
        ld < (col_major ? rows : cols))
        return fail(c, VO_ERR_ARG, "%s: bad arguments", who);
    if (!c->pending.empty()) return fail(c, VO_ERR_STATE, "asynchronous step batches pending (vo_step_collect first)");
    CallScope call(c); if (call.status) return call.status;
    SgmBuffers& sb = c->sgm;
    {
        const hipError_t e = reconstruct_reserve(c->pool, sb, rows, cols);
        if (e != hipSuccess) return fail(c, VO_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    const size_t fs = (size_t)rows * cols;
    const int major = col_major ? rows : cols, minor = col_major ? cols : rows;
    HIPC(c, hipMemcpy2DAsync(sb.rin, sizeof(float) * major, disp, sizeof(float) * ld, sizeof(float) * major, minor, hipMemcpyHostToDevice,
                             c->stream));
    reconstruct_launch(sb.rin, rows, cols, col_major, Q, sb.xyz, c->stream);
    HIPC(c, hipMemcpyAsync(xyz, sb.xyz, sizeof(float) * 3 * fs, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
}

int vo_landmarks(vo_ctx* c, const float* l_pos, const float* r_pos, int S, const float* old_l, const float* old_r, int Kn,
                 const double pose[16], double* out, int capacity, int* rows_out)
{
    if (!c || S < 0 || Kn < 0 || !pose || (S && (!l_pos || !r_pos)) || (Kn && (!old_l || !old_r)))
        return fail(c, VO_ERR_ARG, "vo_landmarks: bad arguments");
    if (!c->has_calib) return fail(c, VO_ERR_STATE, "vo_landmarks: no calibration");
    const int K = c->set[0].sb.kp_cap;
    if (S > K || Kn > K) return fail(c, VO_ERR_CAPACITY, "vo_landmarks: more rows than max_keypoints");
    CallScope call(c); if (call.status) return call.status;
    c->have_features = false;
    std::vector<float> sp((size_t)S * 4 + 4), op((size_t)Kn * 4 + 4);
    pack_quads(l_pos, r_pos, S, sp.data());
    pack_quads(old_l, old_r, Kn, op.data());
    int cnt[2] = {S, Kn};
    HIPC(c, hipMemcpyAsync(c->set[0].gb.spos, sp.data(), sizeof(float) * 4 * S, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->set[0].gb.oldpos, op.data(), sizeof(float) * 4 * Kn, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->set[0].gb.s_n, &cnt[0], sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->d_fn, &cnt[1], sizeof(int), hipMemcpyHostToDevice, c->stream));
    landmarks_launch(c->set[0].gb, c->d_fn, c->calib, c->stream);
    int rows = 0;
    HIPC(c, hipMemcpyAsync(&rows, c->set[0].gb.lm_rows, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    int rc = finish(c);
    if (rc) return rc;
    std::vector<float> X((size_t)rows * 3);
    std::vector<uint8_t> keep(rows);
    HIPC(c, hipMemcpy(X.data(), c->set[0].gb.lm_X, sizeof(float) * 3 * rows, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(keep.data(), c->set[0].gb.lm_keep, rows, hipMemcpyDeviceToHost));
    if (rows_out) *rows_out = rows;
    if (out) {
        for (int m = 0; m < rows && m < capacity; ++m) {
            out[3 * m] = out[3 * m + 1] = out[3 * m + 2] = 0.0;
            if (keep[m]) lm_world(pose, &X[(size_t)m * 3], out + 3 * m);
        }
    }
    if (rows > capacity) return fail(c, VO_ERR_CAPACITY, "vo_landmarks: %d rows exceed capacity %d", rows, capacity);
    return VO_OK;
}

}  // extern "C"
