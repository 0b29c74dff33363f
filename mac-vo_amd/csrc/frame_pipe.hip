// Native per-frame driver: one MACVO.run_pair of kernel launches per host call (SURVEY.md §8 A1-A22 call order)
//
// Replaces the host-side sequencing of Odometry/MACVO.py:173-311 (run_pair) + Module/Frontend/Frontend.py:215-232
// (estimate_pair) for the hot path.  The reference issues ~150 tiny torch ops per frame from Python; a Python loop over
// this library's own entry points still costs ~370 us of interpreter / ctypes time per frame, which is MORE than the
// ~330 us of GPU work (measured: the frame rate did not move when the volume GEMM got 4x faster).  Here the whole
// enqueue side is C++: ~30 launches per frame at 2-3 us each, two host calls per frame.
//
// Four HIP streams (created here, independent of the caller's) — four is the ceiling of this stack (a fifth queue costs a third of the frame rate).
// Classic layout (>= 3 lanes, mapping):
//   vol    the MFMA-bound cost-volume GEMM of frame t+1 (rotating volume buffers)
//   main   decoder side of a frame: 12 window lookups, (convex upsampling,) epilogue, dense selector, count -> host
//   back   pose-independent half of frame t's backend: gather, tracking, back-projection, covariances (one launch)
//   side   filters + rotation into the world frame + LM solve (one launch; the GPU analogue of the reference's optimizer child process,
//          Optimization/Interface.py:80-96)
// Round-5 layout (one- and two-lane pipes; `Knobs::alt` below): vol | main = even frames' decoder side | a second decoder-side stream = odd frames' |
//   side = backend + solve of every frame, in order; the GEMM leaves 32 CUs without a workgroup (Knobs::free_cus).
// Frame t+1's frontend is enqueued before frame t's `finish`, so the selector's host round trip (candidate count ->
// torch.randperm on the CPU, kept for bit-exact indices -> permutation back) never idles the GPU.
// Stream layouts measured on the bench (ms / frame): this one 0.3235; even / odd frames each entirely on their own
// frontend stream (no event between GEMM and lookups) 0.337 — the next frame's GEMM then collides with more of the
// latency-bound kernels and both stretch; ONE frontend stream for everything 0.373 — the ~3 us launch-to-launch gaps of
// the 15 small kernels are no longer hidden under the next GEMM.
//
// Memory: every device buffer lives in ONE caller-provided arena (a torch tensor in the Python host), carved up here;
// mv_frame_pipe_buffer reports where each piece is so the host can view results without copies.  Slots rotate so a
// stage never overwrites data a still-running stage of another stream reads (maps x3, everything else x2) and the
// cross-stream hazards are closed with events (see `enqueue` / `finish`).
#include "common.h"
#include "motion_dev.h"
#include "kp_draw_dev.h"
#include <atomic>
#include <chrono>
#include <stdio.h>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <random>
#include <thread>
#include <vector>
#include <new>
#include <stdlib.h>
#include <string.h>
#if defined(__linux__)
#include <sched.h>
#endif

#define MV_HIP(call)                                   \
    do {                                               \
        if ((call) != hipSuccess) return MV_ERR_LAUNCH; \
    } while (0)
#define MV_TRY(call)               \
    do {                           \
        const int rc_ = (call);    \
        if (rc_ != MV_OK) return rc_; \
    } while (0)

namespace {

// slot rotation for up to MAX_PENDING tracked frames in flight (enqueued, not finished): frame f's epilogue writes maps[f % N_MAPS]
// while the backend of frame f - MAX_PENDING may still read maps of f - MAX_PENDING and f - MAX_PENDING - 1
// N_CAND = MAX_PENDING + 1 (round 3): the candidate slot frame f's selector writes was last read by the backend of frame f - 4, not of the
// frame finished a moment ago — so that the enqueue of frame f never has to wait for the backend launch thread (below) to have ISSUED
// the newest finish.
#ifndef MV_MAX_PENDING
#define MV_MAX_PENDING 3
#endif
constexpr int MAX_PENDING = MV_MAX_PENDING, N_MAPS = MAX_PENDING + 2, N_CAND = MAX_PENDING + 1, N_PERM = 4, N_INEV = 8, MAX_VOL = 4, MAX_LK = 2;
constexpr int N_MOT = 8;   // motion_model: ring of per-finish motion slots (raw PoseNet output + composed prior of finish g -> slot g % N_MOT)
constexpr int N_BEV = 8;   // ring of per-finish backend events (finish g -> slot g % N_BEV): the device-driven frame waits for the exact finish whose reads free a slot

// selector modes that look at no map: no selector kernels, no candidate list, no count copy
inline bool kp_new_mode(int m) { return m == MV_KP_RANDOM || m == MV_KP_GRID || m == MV_KP_EXPLICIT; }
// rows a frame of such a pipe tracks (RANDOM / EXPLICIT: num_point = the capacity; GRID: the grid's own count, which may exceed num_point)
inline int frame_rows(const mvFramePipeConfig& c) {
    return c.selector_mode == MV_KP_GRID ? mvkp::grid_of(c.H, c.W, c.kp_mask_width, c.num_point, nullptr) : c.num_point;
}
// THE capacity rule: rows per lane of every per-keypoint table (arena, offsets, views, map_append)
inline int table_rows(const mvFramePipeConfig& c) {
    const int g = frame_rows(c);
    return g > c.num_point ? g : c.num_point;
}
inline int cap_of(const mvFramePipeConfig& c) {   // (a pipe without keypoints still carves one row)
    const int r = table_rows(c);
    return r > 0 ? r : 1;
}
enum { KPJ_PERM = 0, KPJ_HOST = 1, KPJ_DEV = 2, KPJ_RANDOM = 3, KPJ_GRID = 4 };   // FinishJob::kp — where a finish takes its keypoint rows from

struct Maps {
    float *disparity, *disparity_cov, *depth, *depth_cov, *match_flow, *match_cov;
    uint8_t* bad_mask;
    mvDepthMaps dm;   // depth, disparity, disparity_cov, depth_cov as the front launch reads them (describe_backend)
};

struct Backend {   // every table is [lanes, cap = num_point, ...]; rows beyond a lane's n_sel are dead (valid = 0)
    int64_t *perm, *kp0;
    float *kp0f, *kp1, *vals, *sigma0, *sigma1, *pos_Tc, *pos_Tw;
    uint8_t *inbound, *valid;
    double *rot, *cov0, *cov0w, *cov1, *pose64, *info;
    int32_t* n_valid;
    int32_t* live_dev;   // [lanes, 2] device-driven frame: selected keypoints = live rows, candidate count (written by the front launch's draw)
    int32_t n_sel[MV_MAX_LANES];
    bool rows_dev;       // the slot's frame took its rows and live-row counts from device memory (mv_frame_pipe_finish_keypoints_dev): the counts are in live_dev only
    // the slot's tables as the two backend launches take them, laid out once (describe_backend) and read-only afterwards
    mvFrontTables front;
    mvPosedSolve solve;   // ... with everything of the solve that does not change per finish (finish_issue fills in the poses and the live rows)
};

struct Pending {
    int maps, maps_prev, cand;
    bool has_cand;
    int ti;   // timing slot of the frame (mv_frame_pipe_time_volume), -1: not timed
    long sel_job = -1;   // MV_PIPE_SELECTOR_ON=late: the finish (job) that issues this frame's selector segment; -1: already issued
    long f = -1;         // frame index (alt layout: the backend waits for the previous frame's selector segment by its event)
};

// The selector segment of a frame (upsampling / epilogue / selector(s) / count copies): everything behind the frame's last lookup.
// Issued by mv_frame_pipe_enqueue itself, or — MV_PIPE_SELECTOR_ON=vol — deferred until the NEXT frame's GEMM has been queued, so that
// it lands behind that GEMM on the GEMM's stream.
struct SelSeg {
    mvFrameInputs in;
    long f;
    int k, m, ti, maps_prev;
    bool timed, with_selector, up;
    long need_issued;   // backend launch thread: finishes that must have been issued before the segment's slot-reuse wait
};

// One `finish` split in two: the host-visible bookkeeping (slot rotation, counts, views) happens on the calling thread, the
// launches are described by this job and issued either inline or by the backend launch thread.
struct FinishJob {
    Pending pd;
    long g;                 // finish index; backend slot k = g & 1
    int pose_from, pose_to; // pose slots: prior of the frame / its optimised pose
    bool skipped = false;   // mv_frame_pipe_skip since the previous finish: the local solve's frame is the previous keyframe's prior
    int n_max;
    int32_t n_sel[MV_MAX_LANES];
    int64_t n_cand[MV_MAX_LANES];   // seeded: candidate count per lane (the permutation is drawn by whoever issues the job)
    bool seeded;
    int kp = KPJ_PERM;              // != 0: (u, v) rows instead of a permutation over the candidate list — HOST: the caller's / drawn rows (in `perm` / the row
                                    // argument, [lanes, cap, 2]); DEV: kp_dev / nsel_dev behind e_kpin; RANDOM: drawn inside the front launch; GRID: computed there
    const int64_t* kp_dev = nullptr;
    const int32_t* nsel_dev = nullptr;
    bool device = false;            // device-driven frame: the permutation is drawn inside the front launch, n_sel is an upper bound (num_point)
    std::vector<int64_t> perm;      // explicit permutations [lanes, cap] (asynchronous issue: a copy of the caller's array)
    float* pose_sink;
    double t_count = 0, t_submit = 0;   // host clock (us): candidate count seen / job queued (MV_PIPE_HOST_STATS)
    bool has_sel;                   // MV_PIPE_SELECTOR_ON=late: the selector segment of the newest enqueued frame rides behind this backend
    SelSeg sel;
};

struct Carver {   // bump allocator over the arena (or a size counter when base == nullptr)
    char* base;
    size_t off = 0;
    template <typename T>
    T* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

// One sync edge of the driver: the event and whether it holds a record of the current generation.  Nothing waits for an edge that holds none: the three
// waits then return MV_OK without a HIP call.  The state is a relaxed atomic because the backend launch thread records edges the caller's thread waits for:
// all of those reads but one are ordered by `mu` (wait_issued / flush_jobs); the lean chain's volume release in issue_volume is not.
struct Ev {
    hipEvent_t e = nullptr;
    std::atomic<bool> rec{false};
    Ev() = default;
    Ev(Ev&& o) noexcept : e(o.e), rec(o.recorded()) { o.e = nullptr; }   // (movable, not copyable: the timing events live in vectors)
    ~Ev() { if (e) (void)hipEventDestroy(e); }
    int create(unsigned flags = hipEventDisableTiming) {   // (hipEventDefault: a timing event, as hipEventCreate makes it)
        return (flags == hipEventDefault ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, flags)) == hipSuccess ? MV_OK : MV_ERR_LAUNCH;
    }
    bool recorded() const { return rec.load(std::memory_order_relaxed); }
    void skip() { rec.store(false, std::memory_order_relaxed); }   // this generation is deliberately not recorded (the event may hold an older one)
    int record(hipStream_t s) {
        if (hipEventRecord(e, s) != hipSuccess) return MV_ERR_LAUNCH;
        rec.store(true, std::memory_order_relaxed);
        return MV_OK;
    }
    int wait(hipStream_t s) const {   // always a barrier packet
        return !recorded() || hipStreamWaitEvent(s, e, 0) == hipSuccess ? MV_OK : MV_ERR_LAUNCH;
    }
    // ... and when the event has already fired no barrier packet is queued at all (every hipStreamWaitEvent costs the waiting queue a few microseconds
    // even for a long-fired event)
    int wait_if_pending(hipStream_t s) const {
        if (!recorded()) return MV_OK;
        const hipError_t q = hipEventQuery(e);
        if (q == hipSuccess) return MV_OK;
        if (q != hipErrorNotReady) return MV_ERR_LAUNCH;
        return hipStreamWaitEvent(s, e, 0) == hipSuccess ? MV_OK : MV_ERR_LAUNCH;
    }
    int sync() const { return !recorded() || hipEventSynchronize(e) == hipSuccess ? MV_OK : MV_ERR_LAUNCH; }
};
template <int N>
int create_all(Ev (&a)[N]) {
    for (Ev& e : a) MV_TRY(e.create());
    return MV_OK;
}
template <int N>
struct EvRing {   // one edge per running frame / finish number: generation g lives in slot g % N
    Ev slot[N];
    Ev& operator[](long g) { return slot[g % N]; }
};

// Stream of a frame's selector segment (MV_PIPE_SELECTOR_ON; classic layout only).  `vol`, `late`, `own`: lower latency, lower throughput.
enum class SelOn {
    Decoder,   // main: in order behind the frame's lookups
    Back,      // the backend stream, behind an event on the last lookup: one lane 5.38 k vs 4.94 k frames/s, 32 lanes 7.43 k vs 7.64 k
    Own,       // a fifth stream
    Vol,       // the GEMM's stream, deferred until the next frame's GEMM has been queued
    Late       // the backend stream, handed to the next finish when two unfinished frames are in front (3-deep pipeline; profiles/r04_latency_ab.log)
};
// Stream of frame f + 1's operand pack (MV_PIPE_PACK_ON).  One lane, frames/s: in front of the GEMM on its stream 4.28 k, backend stream 4.09 k,
// decoder-side stream 3.11 k.
enum class PackOn { Vol, Back, Main, Side };
enum { SYNC_STREAM = 0, SYNC_HOST = 1, SYNC_NEWEST = 2 };   // mv_frame_pipe_sync's block_host

// Everything the environment, the lane count and the configuration decide about schedule and layout, resolved in ONE place (resolve_knobs) when a pipe is
// created, sized (mv_frame_pipe_arena_bytes) or asked for its depth (mv_frame_pipe_default_depth).  DESIGN appendix: the variables.
struct Knobs {
    // The round-5 layout, default for one- and two-lane pipes without mapping: two decoder-side streams (frame f's lookups on stream f % 2), backend +
    // solve in order on ONE stream — still four queues; a fifth costs a third of the frame rate (profiles/r05_pipe_ab.log run 15).  MV_PIPE_LAYOUT=classic,
    // or a placement that exists in the classic layout only (MV_PIPE_SELECTOR_ON, MV_PIPE_LOOKUPS_ON=vol), selects the classic one.
    bool alt;
    int n_lk;            // decoder-side streams: 2 (alt) or 1
    int n_volbuf;        // 3: the GEMM one frame ahead rewrites a buffer read two frames ago (272 vs 245 us per frame with 2); alt: three tracked frames in
                         // flight + that GEMM = 4 (6.95 k vs 6.74 k frames/s at 300 steps; 5: no gain)
    int default_depth;   // tracked frames the host should keep in flight: 3 (alt and batched pipes), the classic one-lane pipe 2
    SelOn sel_on;        // alt: Decoder; classic: MV_PIPE_SELECTOR_ON, else Back for one and two lanes
    PackOn pack_on;
    bool lookups_on_main;   // MV_PIPE_LOOKUPS_ON=vol: the lookups stay behind the GEMM on its stream (0.3256 vs 0.3197 ms per frame)
    int free_cus;        // CUs the GEMM leaves without a persistent workgroup, for the solve's: alt 32 (0 / 8 / 16 / 32 / 48 / 64 = 6.26 / 6.34 / 6.68 / 6.84 /
                         // 6.87 / 6.82 k frames/s, profiles/r05_pipe_ab.log), classic 0 (no gain); MV_PIPE_FREE_CUS
    bool alt_indep;      // alt: consecutive frames' selector segments may overlap (ordered segments: -6 %, profiles/r05_pipe_ab.log run 18)
    // MV_PIPE_LEAN (alt only): a device-driven frame's chain carries fewer packets.  A marker costs the queue ~6 us, a cross-queue barrier ~10
    // (profiles/r06_chain_gaps.log).  Two decisions:
    bool no_segment_markers;     // e_cand / e_seg behind a selector segment are recorded on demand only: the front launch follows in stream order
    bool front_frees_volume;     // a frame's front launch, not a marker behind its lookups, releases its volume buffer
    bool front_on_decoder;       // alt: a device-driven frame's front launch runs behind its selector segment on the decoder-side stream, the backend stream
                                 // carries the solves only (300 steps 6.83-6.95 k vs 6.60-6.64 k frames/s, profiles/r06_device_draw_ab.log); MV_PIPE_FRONT_ON=side
    bool fuse_backend;           // backend = front launch + posed solve; MV_PIPE_FUSE_BACKEND=0: the five-launch form
    int tiled_wish;              // MV_PIPE_TILED: 1 / 0, -1 unset = on for fp16 cells (32 lanes 11.8 k -> 13.3 k frames/s), off for fp32 cells (7.44 k vs 7.95 k)
    bool async_wish;             // backend launch thread: the configuration, else MV_PIPE_ASYNC_BACKEND, else on (one lane 6.01 k vs 5.26 k frames/s)
    bool async_explicit;         // ... and whether either of them chose (a device-driven pipe on a small host otherwise drops the thread: mv_frame_pipe_seed_lanes)
    double spin_us;              // how long the launch thread spins for a job before it sleeps (MV_PIPE_LAUNCH_SPIN_US; 250 where the process has >= 3 cores)
    int host_stats;              // MV_PIPE_HOST_STATS=1: mean host latencies, printed by destroy
    bool device_draw_wish;       // MV_PIPE_DEVICE_DRAW=0: host-drawn frames also where the device draw applies
};

}  // namespace

struct mvFramePipe {
    mvFramePipeConfig c;
    Knobs k;     // schedule and layout as resolved at create
    int plane, h8, w8, n8, KK;
    int lanes;   // independent sequences batched through every launch (= pairs / 2)
    size_t fb_count[MV_FB_PRIOR + 1];   // element count of each buffer mv_frame_pipe_buffer reports, recorded where it is carved
    char* arena;
    size_t arena_bytes;
    // device buffers
    float* vol[MAX_VOL];   // k.n_volbuf of them
    float* tok[2 * MAX_LK];   // two alternating token buffers per decoder-side stream
    void* planes[2];   // bf16x3 split planes of fmap1 / fmap2 (volume_split3)
    // volume_split = MV_PACK_BF16X3: packed three-piece operands of the streaming split GEMM, two sets (the pack of frame f + 1 may
    // run beside the GEMM of frame f); `packed` = the shape is covered by the streaming kernel (exact fp32 kernel otherwise)
    void* pk[2][2];
    int n2t;           // cells per volume slice: n8, or mv_tiled_slice_cells(h8, w8) for a tiled fp16 volume (a padded last tile row when h8 % 4 != 0)
    void* tile16;      // vol16 && tiled: operand 2 with its pixel rows in 4 x 4-tile order (mv_fmap_tile_rows16; written and read on the GEMM's stream)
    size_t pk_bytes;
    bool packed;
    bool vol16;        // volume_split = MV_VOL_ENC16 on a shape the out16 kernel covers: 2-byte cells (Fast mode as the reference computes it)
    bool tiled;        // MV_PIPE_TILED=1 && packed: operand 2 packed in 4 x 4-tile order -> the volume is tiled for mv_corr_lookup_tiled
                       // (the driver owns both the producer and the consumer of the volume; MV_FB_VOLUME then shows that layout)
    Ev e_lk[N_CAND];   // a frame's last lookup (decoder-side stream)
    Ev e_packed[2];
    float *up_flow, *up_cov;
    Maps maps[N_MAPS];
    void* kp_ws;
    size_t kp_ws_bytes;
    int32_t* cand[N_CAND];
    int32_t* count[N_CAND];
    float* stats[N_CAND];
    Backend be[2];
    mvCovConfig cov;   // the covariance model of every front launch (describe_backend)
    float* pose[3];   // [lanes, 7]
    float *intr, *bl;   // [lanes, 4], [lanes]
    int32_t* offs;    // [lanes + 1]: lane l owns rows [l * cap, (l + 1) * cap) of the backend tables
    // host
    int32_t* h_count[N_CAND];      // pinned
    int64_t* h_perm[N_PERM];  // pinned
    // streams / events
    hipStream_t s_vol, s_main, s_back, s_side;
    hipStream_t s_lk[MAX_LK];   // decoder-side streams: frame f's lookups run on s_lk[f % k.n_lk]; s_lk[0] = s_main
    EvRing<N_INEV> e_seg;        // alt: end of frame f's selector segment (the next frame's segment runs on the other decoder-side stream)
    void* kp_ws2;                // alt_indep: the odd frames' selector workspace
    Ev* vol_free_ev[MAX_VOL];    // what the GEMM that rewrites volume buffer k waits for (e_vol_free[k], or the ring event of the frame's front launch; null: nothing)

    hipStream_t s_sel;   // MV_PIPE_SELECTOR_ON=own: a fifth stream for the selector segment (nullptr otherwise)
    SelSeg deferred;     // MV_PIPE_SELECTOR_ON=vol: the newest frame's selector segment, not issued yet
    bool deferred_valid;
    EvRing<N_INEV> e_rest;    // inputs of the decoder side (coords, flow, ...) when the GEMM was issued ahead of them
    EvRing<N_INEV> e_in;
    Ev e_vol_done[MAX_VOL], e_vol_free[MAX_VOL], e_pgo;
    Ev e_cand[N_CAND];        // slot k holds this frame's selector segment (lean chain: recorded only when somebody asks)
    EvRing<N_BEV> e_backend;
    EvRing<N_PERM> e_perm;
    EvRing<N_BEV> e_kpin;     // finish g: the caller's stream when mv_frame_pipe_finish_keypoints_dev was called
    Ev e_release;             // the consumer's reads of result views enqueued so far (mv_frame_pipe_release)
    Ev e_posed[2];            // backend slot k: world-frame tables written (side stream, in front of the solve)
    Ev e_solved[2];           // backend slot k: its solve has finished reading the tables
    // state
    long n_enq, n_fin;
    long n_vol;            // volume GEMMs issued (n_enq <= n_vol <= n_enq + 1: at most one GEMM ahead of its frame's decoder side)
    Ev* e_in_of[MAX_VOL];  // per volume buffer: the input-ready event its GEMM waited for (the decoder side re-uses it)
    int pose_cur;
    int prior_slot;        // pose slot the newest finished frame started from (its motion-model prior)
    int solve_frame = MV_SOLVE_WORLD;   // mv_frame_pipe_set_solve_frame
    bool skipped = false;               // mv_frame_pipe_skip since the newest finish
    Ev e_map;
    Ev e_mapl[2];             // backend slot k: the map append (map_append_finished) has finished reading the slot's tables
                              // (recorded by the caller's thread behind flush_jobs, waited for by whoever issues the later finishes)
    int newest_maps;
    std::deque<Pending> pending;
    // dense-mapping tail (config.mapping; lanes == 1)
    int32_t* cand_m[N_CAND];
    int32_t* count_m[N_CAND];
    float* stats_m[N_CAND];
    int32_t* h_count_m[N_CAND];    // pinned
    int32_t* h_nvalid[2];          // pinned: observation count of backend slot k
    Ev e_nvalid[2];
    int64_t *mp_perm, *mp_uv;      // [map_num_point], [map_num_point, 2]
    float *mp_uvf, *mp_d, *mp_sdd, *mp_sigma, *mp_Tc, *mp_Tw;
    double* mp_cov;
    uint8_t* mp_color;
    int64_t* h_perm_m;             // pinned
    Ev e_maptail;                  // the map tail's last kernel (buffers + pinned permutation reusable)
    int mp_rows;                   // rows of the newest map tail (0: none for the newest finished frame)
    int last_maps_prev, last_cand;   // of the newest finished frame
    // native keypoint permutations (mv_frame_pipe_seed_lanes): one MT19937 per lane, the engine behind torch's CPU generator
    std::vector<std::mt19937> rng;
    std::vector<int32_t> perm_scratch;   // identity array of the partial Fisher-Yates, reused
    std::vector<int64_t> perm_host;      // [lanes, cap] permutations, or [lanes, cap, 2] drawn RandomSelector rows
    std::vector<int32_t> nsel_host;
    // Device-driven frame (round 6, mv_frame_pipe_seed_lanes with MV_PIPE_DEVICE_DRAW != 0): the same generators live in DEVICE memory and the permutation head is
    // drawn inside the backend's front launch (randperm_dev.h) from the count the selector left in device memory — no D2H count, no host wait, no host draw, no
    // H2D permutation: enqueue + finish of a frame are a fixed chain of launches.  Two state buffers: finish g reads rp_state[g & 1], writes rp_state[(g + 1) & 1].
    uint32_t* rp_state[2];   // [lanes, mv_randperm_state_words()]
    int dev_draw;
    long last_backend_frame = -1;   // frame index of the newest backend issued with keypoints (launch-thread / inline issuer only)
    // optional timing of the dominant kernel (bench.py roofline): event pairs around each volume GEMM on its stream
    int vol_timed[MAX_VOL];      // timing slot of the GEMM that filled each volume buffer (-1: not timed)
    std::vector<Ev> tv[8];       // per timing slot: GEMM start / end, last lookup done, selector done; backend start / end (backend stream), pose_apply
                                 // start / solve end (solve stream)
    int n_timed, timed_cap;
    int time_detail;   // 1 (default): a timed frame also records the six timeline events tv2..tv7 on three streams; 0: only the pair around its GEMM
    // Backend launch thread (round 3).  A one-lane stream is bound by the HOST: ~38 launches per frame at ~4 us each on one thread
    // (tools/host_breakdown.py: 172 us of host time per frame, 6 us of it waiting for the GPU).  With `async_backend` the ~10
    // launches of `finish` + the permutation draw are issued by this thread while the caller's thread already enqueues the next
    // frame's decoder side.  Everything that is not enqueue / enqueue_volume / wait_candidates / finish / release / buffer first
    // drains the job queue (`flush_jobs`), so the two threads never touch the same piece of driver state:
    //   caller's thread: pending, n_enq / n_fin / pose_cur / views, s_vol + s_main launches, the selector segment on s_back
    //   launch thread:   Backend tables, e_solved / e_posed / e_pgo / e_perm / e_backend, pinned permutation slots, rng
    // Cross-thread event edges: e_cand and e_release are recorded by the caller BEFORE the job is queued; e_backend is consumed by
    // the caller's enqueue only after `issued` says the launch thread has recorded it.
    int async_backend;      // k.async_wish, until something takes the thread away (no device, mv_frame_pipe_seed_lanes)
    int device;
    std::thread worker;
    std::mutex mu;
    std::condition_variable cv_job, cv_done;
    std::deque<FinishJob> jobs;
    long issued;            // finishes whose launches have all been issued (guarded by mu)
    std::atomic<long> n_submitted{0};   // jobs ever queued: what the launch thread spins on
    std::atomic<bool> stop_flag{false};
    double st_n = 0, st_count_to_submit = 0, st_submit_to_pick = 0, st_pick_to_issued = 0, st_wait = 0;
    double st_enq = 0, st_enq_lookups = 0, st_enq_seg = 0, st_vol = 0, st_fin = 0, st_calls = 0;   // us inside enqueue (its lookups / its selector segment), enqueue_volume, finish_device
    bool stop;
    int async_rc;           // first error of an asynchronously issued job, reported by the next call
    // TartanMotionNet prior (c.motion_model = MV_MOTION_TARTAN).  PoseNet input per maps slot (= per enqueued frame, written behind the frame's epilogue,
    // read by the caller's PoseNet); raw motion and composed prior per FINISH index g (slot g % N_MOT): mv_frame_pipe_set_motion writes the raw motion on
    // the caller's stream (e_motion_set), the finish composes prev pose @ Exp(raw * pose_norm) on the solve's stream (e_motion_used) into `prior`, which the
    // solve starts from and mv_frame_pipe_map_append registers.  A slot is rewritten only behind the events of its previous user.
    float* motion_in[N_MAPS];
    EvRing<N_MAPS> e_motion_in, e_motion_read;
    float* motion_raw[N_MOT];
    float* prior[N_MOT];
    float* pose_norm;       // [6] fp32
    EvRing<N_MOT> e_motion_set, e_motion_used;
    long motion_g[N_MOT];   // finish index whose raw motion the slot holds (-1: none)
};

static int affinity_cores() {
#if defined(__linux__)
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0) return CPU_COUNT(&set);
#endif
    const unsigned n = std::thread::hardware_concurrency();
    return n ? (int)n : 1;
}

static inline double now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static int wait_issued(mvFramePipe* p, long n);
static int flush_deferred(mvFramePipe* p);
static int issue_selector_segment(mvFramePipe* p, const SelSeg& d);
static int flush_jobs(mvFramePipe* p);
static void launch_thread_main(mvFramePipe* p);

// THE reader of the environment.  `async_backend`: the configuration's (1 on, -1 off, 0 = not said).
static Knobs resolve_knobs(int lanes, int mapping, int async_backend) {
    struct Var {
        const char* v;
        bool is(const char* s) const { return v && strcmp(v, s) == 0; }
        bool off() const { return v && atoi(v) == 0; }
        int num(int unset) const { return v ? atoi(v) : unset; }
    };
    const auto var = [](const char* name) { return Var{getenv(name)}; };
    const Var sel = var("MV_PIPE_SELECTOR_ON"), pack = var("MV_PIPE_PACK_ON"), lookups = var("MV_PIPE_LOOKUPS_ON"), async = var("MV_PIPE_ASYNC_BACKEND");
    Knobs k{};
    k.alt = !var("MV_PIPE_LAYOUT").is("classic") && lanes <= 2 && !mapping && !lookups.is("vol") && !sel.v;
    k.n_lk = k.alt ? 2 : 1;
    k.n_volbuf = k.alt ? 4 : 3;
    k.default_depth = (lanes > 2 || k.alt) ? 3 : 2;
    k.sel_on = k.alt ? SelOn::Decoder
             : sel.v ? (sel.is("back") ? SelOn::Back : sel.is("own") ? SelOn::Own : sel.is("vol") ? SelOn::Vol : sel.is("late") ? SelOn::Late : SelOn::Decoder)
                     : (lanes <= 2 ? SelOn::Back : SelOn::Decoder);
    k.pack_on = pack.is("back") ? PackOn::Back : pack.is("main") ? PackOn::Main : pack.is("side") ? PackOn::Side : PackOn::Vol;
    k.lookups_on_main = !lookups.is("vol");
    k.free_cus = var("MV_PIPE_FREE_CUS").num(k.alt ? 32 : 0);   // (multiples of 8: per XCD)
    k.alt_indep = k.alt;
    const bool lean = k.alt && !var("MV_PIPE_LEAN").off();
    k.front_on_decoder = k.alt && !var("MV_PIPE_FRONT_ON").is("side");
    k.no_segment_markers = lean && k.front_on_decoder;       // (alt: the segment is on the decoder-side stream, and there is no mapping tail)
    k.front_frees_volume = lean && k.n_volbuf > MAX_PENDING;  // (the GEMM that rewrites the buffer is issued after the frame's finish: enqueue)
    k.fuse_backend = !var("MV_PIPE_FUSE_BACKEND").off();
    k.tiled_wish = var("MV_PIPE_TILED").v ? var("MV_PIPE_TILED").num(0) != 0 : -1;
    k.async_wish = (async_backend ? async_backend : async.v ? (async.num(0) ? 1 : -1) : 1) > 0;
    k.async_explicit = async_backend || async.v;
    // a spinning launch thread needs a core of its own beside the caller's (and Python's): with fewer than three it sleeps on the condition variable instead
    const Var spin = var("MV_PIPE_LAUNCH_SPIN_US");
    k.spin_us = spin.v ? atof(spin.v) : (affinity_cores() >= 3 ? 250.0 : 0.0);
    k.host_stats = var("MV_PIPE_HOST_STATS").num(0);
    k.device_draw_wish = !var("MV_PIPE_DEVICE_DRAW").off();
    return k;
}

extern "C" int mv_frame_pipe_default_depth(int lanes, int mapping) { return resolve_knobs(lanes, mapping, 0).default_depth; }

static size_t carve(mvFramePipe* p, char* base) {
    const mvFramePipeConfig& c = p->c;
    Carver a{base};
    const size_t L = p->lanes;
    const size_t plane = p->plane, n8 = p->n8, B = c.pairs, N = (size_t)cap_of(c);
    // Every buffer mv_frame_pipe_buffer reports has a leading [lanes] dimension (VALS: [11, lanes, cap]; N = capacity rows, a lane's live rows: its n_sel).
    // `n` notes its element count, here and nowhere else, and hands it on to `take`.
    size_t* const n = p->fb_count;
    for (int k = 0; k < p->k.n_volbuf; ++k) p->vol[k] = a.take<float>(B * n8 * n8);
    n[MV_FB_VOLUME] = B * n8 * p->n2t;   // in cells, n2t per slice: 2-byte cells of a tiled slice padded to whole tiles still fit the buffer's n8 * n8 * 4 bytes
    for (int k = 0; k < 2 * (L <= 2 ? MAX_LK : 1); ++k) p->tok[k] = a.take<float>(n[MV_FB_TOKENS] = B * p->KK * n8);
    for (int k = 0; k < 2; ++k)
        p->planes[k] = (c.volume_split == 2 || c.volume_split == 3) ? (void*)a.take<uint16_t>(3 * B * n8 * c.C) : nullptr;
    // (ceil(n8 / 32) + 1 row blocks per pair: the rounded-up last block and the replica block the GEMM's ragged last sub-tile reads — n8 % 64 != 0, 376 x 784 and
    // 480 x 752 frames — are inside; the volume itself keeps its pitch of n8 cells)
    p->pk_bytes = p->packed ? mv_volume_pack_bytes((int)B, c.C, (int)n8, c.volume_split) : 0;
    for (int k = 0; k < 2; ++k)
        for (int o = 0; o < 2; ++o) p->pk[k][o] = p->packed ? (void*)a.take<char>(p->pk_bytes) : nullptr;
    // (carved for every Fast-mode pipe whose shape the tiled form covers — the sizing call knows the configuration, not MV_PIPE_TILED: 2 % of the volume buffers)
    p->tile16 = (c.volume_split == MV_VOL_ENC16 && c.radius == 4 && p->w8 % 4 == 0) ? (void*)a.take<uint16_t>(B * (size_t)mv_tiled_slice_cells(p->h8, p->w8) * c.C) : nullptr;
    // (covariance planes the frontend does not provide — c.frontend_nocov — are not carved: their pointers stay null all the way into the launches)
    const bool no_d = (c.frontend_nocov & MV_NOCOV_DEPTH) != 0, no_m = (c.frontend_nocov & MV_NOCOV_MATCH) != 0;
    p->up_flow = a.take<float>(B * 2 * plane);
    p->up_cov = (no_d && no_m) ? nullptr : a.take<float>(B * 2 * plane);
    for (int k = 0; k < N_MAPS; ++k) {   // every map is [lanes, ch, H, W]
        Maps& m = p->maps[k];
        m.disparity = a.take<float>(n[MV_FB_DISPARITY] = L * plane);
        m.disparity_cov = no_d ? nullptr : a.take<float>(n[MV_FB_DISPARITY_COV] = L * plane);
        m.depth = a.take<float>(n[MV_FB_DEPTH] = L * plane);
        m.depth_cov = no_d ? nullptr : a.take<float>(n[MV_FB_DEPTH_COV] = L * plane);
        m.match_flow = a.take<float>(n[MV_FB_MATCH_FLOW] = L * 2 * plane);
        m.match_cov = no_m ? nullptr : a.take<float>(n[MV_FB_MATCH_COV] = L * 3 * plane);
        m.bad_mask = a.take<uint8_t>(L * plane);
    }
    p->kp_ws_bytes = L * mv_kp_select_workspace_bytes(c.H, c.W);
    p->kp_ws = a.take<char>(p->kp_ws_bytes);
    p->kp_ws2 = L <= 2 ? a.take<char>(p->kp_ws_bytes) : nullptr;

    for (int k = 0; k < N_CAND; ++k) {
        p->cand[k] = a.take<int32_t>(n[MV_FB_CAND] = L * plane);
        p->count[k] = a.take<int32_t>(n[MV_FB_COUNT] = L * 4);
        p->stats[k] = a.take<float>(n[MV_FB_STATS] = L * 4);
    }
    for (int k = 0; k < 2; ++k) {
        Backend& b = p->be[k];
        b.perm = a.take<int64_t>(n[MV_FB_PERM] = L * N);
        b.kp0 = a.take<int64_t>(n[MV_FB_KP0] = L * 2 * N);
        b.kp0f = a.take<float>(n[MV_FB_KP0F] = L * 2 * N);
        b.kp1 = a.take<float>(n[MV_FB_KP1] = L * 2 * N);
        b.vals = a.take<float>(n[MV_FB_VALS] = L * 11 * N);
        b.sigma0 = a.take<float>(n[MV_FB_SIGMA0] = L * 3 * N);
        b.sigma1 = a.take<float>(n[MV_FB_SIGMA1] = L * 3 * N);
        b.pos_Tc = a.take<float>(n[MV_FB_POS_TC] = L * 3 * N);
        b.pos_Tw = a.take<float>(n[MV_FB_POS_TW] = L * 3 * N);
        b.inbound = a.take<uint8_t>(n[MV_FB_INBOUND] = L * N);
        b.valid = a.take<uint8_t>(n[MV_FB_VALID] = L * N);
        b.rot = a.take<double>(n[MV_FB_ROT] = L * 9);
        b.cov0 = a.take<double>(n[MV_FB_COV0] = L * 9 * N);
        b.cov0w = a.take<double>(n[MV_FB_COV0W] = L * 9 * N);
        b.cov1 = a.take<double>(n[MV_FB_COV1] = L * 9 * N);
        b.pose64 = a.take<double>(n[MV_FB_POSE64] = L * 7);
        b.info = a.take<double>(n[MV_FB_INFO] = L * 4);
        b.n_valid = a.take<int32_t>(n[MV_FB_NVALID] = L);
        b.live_dev = a.take<int32_t>(n[MV_FB_LIVE] = 2 * L);
    }
    for (int k = 0; k < 2; ++k) p->rp_state[k] = a.take<uint32_t>(L * (size_t)mv_randperm_state_words());
    if (c.mapping) {
        const size_t MP = c.map_num_point > 0 ? c.map_num_point : 1;
        for (int k = 0; k < N_CAND; ++k) {
            p->cand_m[k] = a.take<int32_t>(plane);
            p->count_m[k] = a.take<int32_t>(4);
            p->stats_m[k] = a.take<float>(4);
        }
        // (the dense-mapping tail's buffers are reported with the rows of the newest tail: `n` notes the elements per ROW)
        p->mp_perm = a.take<int64_t>(MP);
        p->mp_uv = a.take<int64_t>(2 * MP);
        p->mp_uvf = a.take<float>((n[MV_FB_MAP_UV] = 2) * MP);
        p->mp_d = a.take<float>((n[MV_FB_MAP_D] = 1) * MP);
        p->mp_sdd = a.take<float>((n[MV_FB_MAP_SDD] = 1) * MP);
        p->mp_sigma = a.take<float>(3 * MP);
        p->mp_Tc = a.take<float>((n[MV_FB_MAP_TC] = 3) * MP);
        p->mp_Tw = a.take<float>((n[MV_FB_MAP_TW] = 3) * MP);
        p->mp_cov = a.take<double>((n[MV_FB_MAP_COV] = 9) * MP);
        p->mp_color = a.take<uint8_t>((n[MV_FB_MAP_COLOR] = 3) * MP);
    }
    for (int k = 0; k < 3; ++k) p->pose[k] = a.take<float>(n[MV_FB_POSE] = L * 7);
    if (c.motion_model == MV_MOTION_TARTAN) {
        for (int k = 0; k < N_MAPS; ++k) p->motion_in[k] = a.take<float>(n[MV_FB_MOTION_IN] = L * (size_t)motion::OUT_C * motion::OUT_H * motion::OUT_W);
        for (int k = 0; k < N_MOT; ++k) {
            p->motion_raw[k] = a.take<float>(L * 6);
            p->prior[k] = a.take<float>(n[MV_FB_PRIOR] = L * 7);
        }
        p->pose_norm = a.take<float>(6);
    }
    p->intr = a.take<float>(L * 4);
    p->bl = a.take<float>(L);
    p->offs = a.take<int32_t>(L + 1);
    return (a.off + 255) & ~(size_t)255;
}

// What the two backend launches of every finish take and what never changes after `create`: the covariance configuration, each Maps slot's planes and each
// Backend slot's tables.  THE place where a slot's table pointers are spelled out; finish_issue names a slot.
static void describe_backend(mvFramePipe* p) {
    const mvFramePipeConfig& c = p->c;
    mvCovConfig& cv = p->cov = {};
    cv.model = c.cov_model; cv.modifiers = c.cov_modifiers;
    cv.cp = mvMatchCovParams{c.H, c.W, c.cov_kernel_size, 1, c.fx, c.fy, c.cx, c.cy, c.min_flow_cov_sq, c.min_depth_cov};
    cv.edge = c.edgewidth; cv.match_cov_default = c.match_cov_default;
    cv.nocov = c.frontend_nocov; cv.model_match_cov_default = c.cov_match_cov_default;
    for (Maps& m : p->maps) m.dm = mvDepthMaps{m.depth, m.disparity, m.disparity_cov, m.depth_cov};
    const int cap = cap_of(c);
    const size_t LN = (size_t)p->lanes * cap;   // value table is [11, lanes, cap]: each of its rows is one concatenated per-point column
    for (Backend& b : p->be) {
        b.front = mvFrontTables{b.kp0, b.kp0f, b.kp1, b.inbound, b.vals, b.sigma0, b.sigma1, b.pos_Tc, b.cov0, b.cov1};
        // (the observation filters: prologue of the solve's launch; mapping mode needs the count on the host first and keeps the launch)
        mvPosedSolve& sv = b.solve = {};
        sv.nprob = p->lanes; sv.offsets = p->offs; sv.cap = cap; sv.graph_type = c.graph_type; sv.intrinsics = p->intr; sv.baseline = p->bl;
        sv.pos_Tc = b.pos_Tc; sv.cov_Tc = b.cov0; sv.pos_Tw = b.pos_Tw; sv.cov_Tw = b.cov0w; sv.out_rot = b.rot;
        sv.pixel2_uv = b.kp1; sv.pixel2_d = b.vals + 4 * LN; sv.pixel2_disp = b.vals + 5 * LN; sv.pixel2_disp_cov = b.vals + 6 * LN;
        sv.pixel2_uv_cov = b.sigma1; sv.obs2_covTc = b.cov1;
        sv.filter_flags = c.mapping ? -1 : c.filters; sv.filter_min_depth = c.filter_min_depth; sv.filter_max_depth = c.max_depth;
        sv.inbound = b.inbound; sv.vals = b.vals; sv.valid = b.valid; sv.count_out = b.n_valid; sv.min_points = c.min_num_point; sv.params = &c.lm;
        sv.out_pose = b.pose64; sv.out_info = b.info;
    }
}

// The 1/8-resolution grid of an H x W frame and where the frame sits in its 8x upsampling.  The network pads a frame to multiples of 8, centred (the public
// InputPadder's "sintel" mode, which FlowFormerCov.inference selects: flownet.py:37-44), works on (H + hp) / 8 x (W + pw) / 8 maps and un-pads its dense outputs:
// frame pixel (y, x) is pixel (y + hp / 2, x + pw / 2) of the padded one.  Everything follows from H and W — no configuration; a multiple of 8 has no pad.
struct Eighth { int h8, w8, y0, x0; };
static Eighth eighth_dims(int H, int W) {
    int32_t pad[4];   // {left, right, top, bottom}
    mv_input_pad(H, W, pad);
    return Eighth{(H + pad[2] + pad[3]) / 8, (W + pad[0] + pad[1]) / 8, pad[2], pad[0]};
}

// convex upsampling into the pipe's H x W planes: the aligned kernel when the frame has no pad (the launches of every earlier build), the window form otherwise
static int upsample_frame(const mvFramePipe* p, const float* f8, const float* mask, float* out, int B, float mask_scale, int exp2_out, hipStream_t s) {
    const Eighth e = eighth_dims(p->c.H, p->c.W);
    if (8 * e.h8 == p->c.H && 8 * e.w8 == p->c.W) return mv_convex_upsample(f8, mask, out, B, p->h8, p->w8, mask_scale, exp2_out, s);
    return mv_convex_upsample_crop(f8, mask, out, B, p->h8, p->w8, e.y0, e.x0, p->c.H, p->c.W, mask_scale, exp2_out, s);
}

static int check_config(const mvFramePipeConfig* c) {
    MV_CHECK_ARG(c);
    MV_CHECK_ARG(c->H > 0 && c->W > 0 && c->H <= (1 << 14) && c->W <= (1 << 14));   // (eighth_dims; what a stage needs of H, W is checked with that stage below)
    // A side one above a multiple of 8 (a pad of 7: seven of the last coarse row's eight rows are replicas) stays an invalid configuration, as it has always been:
    // tests/test_abi_and_host.py pins H = 481 as refused.  Pads 0 .. 6 are taken; the kernels themselves handle 7 (tests/test_gpu_upsample_crop.py).
    MV_CHECK_ARG(c->H % 8 != 1 && c->W % 8 != 1);
    MV_CHECK_ARG(c->C > 0 && c->C % 16 == 0 && c->iters >= 0);
    MV_CHECK_ARG(c->pairs >= 2 && c->pairs % 2 == 0 && c->pairs / 2 <= MV_MAX_LANES);   // lane l = pairs 2l (stereo), 2l + 1 (temporal)
    MV_CHECK_ARG(c->radius >= 1 && c->radius <= 4);
    MV_CHECK_ARG(c->selector_mode == MV_KP_NODEPTH || c->selector_mode == MV_KP_FULL || kp_new_mode(c->selector_mode));
    MV_CHECK_ARG(c->num_point >= 0 && c->edgewidth >= 0 && c->min_num_point >= 0);
    if (kp_new_mode(c->selector_mode)) {
        MV_CHECK_ARG(c->kp_mask_width >= 0 && c->H > 2 * c->kp_mask_width && c->W > 2 * c->kp_mask_width);
        MV_CHECK_ARG(c->selector_mode != MV_KP_GRID || frame_rows(*c) > 0);   // (0: a grid step of 0, where the reference raises)
        MV_CHECK_ARG(table_rows(*c) <= MV_KP_TABLE_MAX);
        if (c->selector_mode == MV_KP_RANDOM && c->num_point > mvkp::MAX_POINT) return MV_ERR_UNSUPPORTED;   // (the front launch's 1024-word draw buffer)
        // the 31 x 31 covariance patch of a keypoint nearer to the border than its half width leaves the image: the reference wraps or raises, the kernel clamps
        MV_CHECK_ARG(c->cov_model == MV_COV_NONE || c->kp_mask_width >= c->cov_kernel_size / 2);
    }
    MV_CHECK_ARG(c->graph_type >= MV_GRAPH_ICP && c->graph_type <= MV_GRAPH_DISP);
    MV_CHECK_ARG(c->mapping == 0 || (c->mapping == 1 && c->pairs == 2 && c->map_num_point > 0 && c->map_mask_width >= 0));
    MV_CHECK_ARG(c->volume_split == 0 || c->volume_split == 2 || c->volume_split == 3 || c->volume_split == MV_PACK_BF16X3 ||
                 c->volume_split == MV_PACK_F16X2 || c->volume_split == MV_VOL_ENC16);
    MV_CHECK_ARG(!c->volume_split || c->volume_split == MV_VOL_ENC16 || c->feat_dtype == MV_F32);
    MV_CHECK_ARG(c->volume_split != MV_VOL_ENC16 || (c->feat_dtype == MV_F16 && c->radius == 4));   // (the lookup reads fp16 cells)
    MV_CHECK_ARG(!(c->volume_split == 2 || c->volume_split == 3) || c->layout == MV_LAYOUT_HWC);   // (the packed form takes either layout)
    MV_CHECK_ARG(c->cov_model >= MV_COV_MATCH && c->cov_model <= MV_COV_NONE && mv_cov_modifiers_ok(c->cov_modifiers));
    MV_CHECK_ARG(c->motion_model == MV_MOTION_STATIC || (c->motion_model == MV_MOTION_TARTAN && motion::crop_scale(c->H, c->W) >= 1));
    // A frontend without covariances (frontend_nocov; 0 = both there).  What reads a missing covariance is refused, not emulated: the reference asserts
    // on depth.cov in CovAwareSelector / MappingPointSelector / GaussianMixtureCovariance, needs match.cov in both CovAware selectors, and builds the
    // reproj / disp weights by inverting the -1 placeholders of pixel2_uv_cov / pixel2_disp_cov (Graphs.py:54-55,97-103,133).
    MV_CHECK_ARG((c->frontend_nocov & ~(MV_NOCOV_DEPTH | MV_NOCOV_MATCH)) == 0);
    if (c->frontend_nocov & MV_NOCOV_DEPTH)
        MV_CHECK_ARG(c->selector_mode != MV_KP_FULL && !c->mapping && c->cov_model != MV_COV_GMM && c->graph_type != MV_GRAPH_DISP);
    if (c->frontend_nocov & MV_NOCOV_MATCH) {
        MV_CHECK_ARG(c->selector_mode != MV_KP_FULL && c->selector_mode != MV_KP_NODEPTH && c->graph_type == MV_GRAPH_ICP);
        MV_CHECK_ARG(c->cov_model == MV_COV_NONE || c->cov_match_cov_default > 0.f);
    }
    return MV_OK;
}

// Everything that follows from the configuration, the lane count and the environment alone: the shapes, the knobs, which volume kernels cover the shape.
// What mv_frame_pipe_arena_bytes sizes and what mv_frame_pipe_create carves are the same because both start here.
static void derive_shape(mvFramePipe* p, const mvFramePipeConfig* cfg) {
    p->c = *cfg;
    p->plane = cfg->H * cfg->W;
    p->h8 = eighth_dims(cfg->H, cfg->W).h8;
    p->w8 = eighth_dims(cfg->H, cfg->W).w8;
    p->n8 = p->h8 * p->w8;
    p->KK = (2 * cfg->radius + 1) * (2 * cfg->radius + 1);
    p->lanes = cfg->pairs / 2;
    p->k = resolve_knobs(p->lanes, cfg->mapping, cfg->async_backend);
    p->packed = (cfg->volume_split == MV_PACK_BF16X3 || cfg->volume_split == MV_PACK_F16X2) &&
                mv_corr_volume_packed_supported(cfg->pairs, cfg->C, p->n8, p->n8, cfg->volume_split);
    // shapes outside the out16 kernel's domain keep the fp32-stored volume of the same 16-bit GEMM
    p->vol16 = cfg->volume_split == MV_VOL_ENC16 && mv_corr_volume_out16_supported(cfg->pairs, cfg->C, p->n8, p->n8, cfg->feat_dtype, cfg->layout);
    // Tiled volume + tiled lookup (Knobs::tiled_wish).  Fast mode's 2-byte cells: a tile is one 32-byte sector (mv_corr_lookup_tiled_vol16: B = 64 alone 115 -> 79 us)
    const bool want = p->k.tiled_wish < 0 ? p->vol16 : p->k.tiled_wish != 0;
    p->tiled = want && cfg->radius == 4 && (p->w8 % 4) == 0 &&
               (p->vol16 ? mv_corr_volume_out16_supported(cfg->pairs, cfg->C, p->n8, mv_tiled_slice_cells(p->h8, p->w8), cfg->feat_dtype, cfg->layout) != 0
                         : (p->packed && (p->h8 % 4) == 0));
    p->n2t = (p->tiled && p->vol16) ? mv_tiled_slice_cells(p->h8, p->w8) : p->n8;
}

extern "C" size_t mv_frame_pipe_arena_bytes(const mvFramePipeConfig* cfg) {
    if (check_config(cfg) != MV_OK) return 0;
    mvFramePipe tmp{};
    derive_shape(&tmp, cfg);
    return carve(&tmp, nullptr);
}

extern "C" int mv_frame_pipe_max_pending(void) { return MAX_PENDING; }

// THE list of the pipe's streams, in creation order, by role: `f` runs on every stream that exists and has one of the roles `which`.  Where backend and
// solve share a stream (alt) it is listed under both roles, so whoever synchronises "backend, then solve" does so twice, as it always has.
enum : unsigned { ST_VOL = 1, ST_DECODER = 2, ST_BACK = 4, ST_SIDE = 8, ST_SEL = 16, ST_ALL = 31 };
template <class F>
static int each_stream(const mvFramePipe* p, unsigned which, F f) {
    const struct { unsigned role; hipStream_t s; } all[] = {{ST_VOL, p->s_vol},   {ST_DECODER, p->s_lk[0]}, {ST_DECODER, p->s_lk[1]},
                                                            {ST_BACK, p->s_back}, {ST_SIDE, p->s_side},     {ST_SEL, p->s_sel}};
    static_assert(MAX_LK == 2, "the decoder-side streams are listed one by one");
    for (const auto& e : all)
        if ((which & e.role) && e.s && f(e.s) != hipSuccess) return MV_ERR_LAUNCH;
    return MV_OK;
}
static int sync_streams(const mvFramePipe* p, unsigned which) { return each_stream(p, which, hipStreamSynchronize); }

extern "C" void mv_frame_pipe_destroy(mvFramePipe* p) {
    if (!p) return;
    if (p->worker.joinable()) {
        {
            std::lock_guard<std::mutex> lk(p->mu);
            p->stop = true;
        }
        p->stop_flag.store(true, std::memory_order_relaxed);
        p->cv_job.notify_all();
        p->worker.join();   // (drains the queue first)
    }
    if (p->k.host_stats && p->st_calls > 0)
        fprintf(stderr, "[mv_frame_pipe host stats] per frame over %.0f device-driven frames: enqueue %.1f us (lookups %.1f, selector segment %.1f), enqueue_volume %.1f us, "
                        "finish_device %.1f us\n", p->st_calls, p->st_enq / p->st_calls, p->st_enq_lookups / p->st_calls, p->st_enq_seg / p->st_calls,
                p->st_vol / p->st_calls, p->st_fin / p->st_calls);
    if (p->k.host_stats && p->st_n > 0)
        fprintf(stderr, "[mv_frame_pipe host stats] finishes %.0f: wait for the candidate count %.1f us, count seen -> job queued %.1f us, queued -> picked up by the "
                        "launch thread %.1f us, picked up -> every launch issued %.1f us (means per frame)\n",
                p->st_n, p->st_wait / p->st_n, p->st_count_to_submit / p->st_n, p->st_submit_to_pick / p->st_n, p->st_pick_to_issued / p->st_n);
    (void)sync_streams(p, ST_ALL);
    for (int k = 0; k < 2; ++k) if (p->h_nvalid[k]) (void)hipHostFree(p->h_nvalid[k]);
    for (int k = 0; k < N_CAND; ++k) if (p->h_count_m[k]) (void)hipHostFree(p->h_count_m[k]);
    if (p->h_perm_m) (void)hipHostFree(p->h_perm_m);
    for (int k = 0; k < N_CAND; ++k) if (p->h_count[k]) (void)hipHostFree(p->h_count[k]);
    for (auto h : p->h_perm) if (h) (void)hipHostFree(h);
    (void)each_stream(p, p->s_back == p->s_side ? ST_ALL & ~ST_BACK : ST_ALL, hipStreamDestroy);
    delete p;   // (every Ev destroys its event: the streams were synchronised above)
}

static int create_impl(mvFramePipe* p) {
    const mvFramePipeConfig& c = p->c;
    int lo = 0, hi = 0;
    MV_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));   // hi = numerically lowest = highest priority
    // the GEMM and the decoder side run at normal priority; the short pose-dependent kernels go first when slots free up
    // (rounds 3-4 A/B, removed in round 5: confining the GEMM / the small kernels to disjoint CU sets with hipExtStreamCreateWithCUMask — any mask cost the
    // GEMM 12 % and the small kernels, grids sized for the whole chip, far more: 0.60-0.83 vs 0.32 ms per frame — and a raised queue priority for the
    // decoder-side stream: no gain.  profiles/r03_*; DESIGN.md changelog.)
    MV_HIP(hipStreamCreateWithPriority(&p->s_vol, hipStreamNonBlocking, 0));
    MV_HIP(hipStreamCreateWithPriority(&p->s_main, hipStreamNonBlocking, 0));
    p->s_lk[0] = p->s_main;
    for (int k = 1; k < p->k.n_lk; ++k) MV_HIP(hipStreamCreateWithPriority(&p->s_lk[k], hipStreamNonBlocking, 0));
    // (creation order matters on this stack: with `side` created before `back` the same schedule ran 15 % slower, profiles/r05_pipe_ab.log)
    if (!p->k.alt) MV_HIP(hipStreamCreateWithPriority(&p->s_back, hipStreamNonBlocking, hi));
    MV_HIP(hipStreamCreateWithPriority(&p->s_side, hipStreamNonBlocking, hi));
    if (p->k.alt) p->s_back = p->s_side;   // backend + solve of a frame in order on ONE stream: the fourth queue belongs to the odd frames' decoder side
    if (p->k.sel_on == SelOn::Own) MV_HIP(hipStreamCreateWithPriority(&p->s_sel, hipStreamNonBlocking, hi));
    MV_TRY(create_all(p->e_in.slot));
    MV_TRY(create_all(p->e_rest.slot));
    MV_TRY(create_all(p->e_vol_done));
    MV_TRY(create_all(p->e_vol_free));
    MV_TRY(create_all(p->e_cand));
    MV_TRY(create_all(p->e_backend.slot));
    MV_TRY(create_all(p->e_kpin.slot));
    if (c.motion_model == MV_MOTION_TARTAN) {
        MV_TRY(create_all(p->e_motion_in.slot));
        MV_TRY(create_all(p->e_motion_read.slot));
        MV_TRY(create_all(p->e_motion_set.slot));
        MV_TRY(create_all(p->e_motion_used.slot));
    }
    for (auto& g : p->motion_g) g = -1;
    MV_TRY(create_all(p->e_posed));
    MV_TRY(create_all(p->e_solved));
    MV_TRY(create_all(p->e_lk));
    MV_TRY(create_all(p->e_seg.slot));
    MV_TRY(create_all(p->e_nvalid));
    MV_TRY(create_all(p->e_packed));
    MV_TRY(create_all(p->e_mapl));
    MV_TRY(create_all(p->e_perm.slot));
    for (Ev* e : {&p->e_pgo, &p->e_maptail, &p->e_map, &p->e_release}) MV_TRY(e->create());
    for (int k = 0; k < N_CAND; ++k) MV_HIP(hipHostMalloc((void**)&p->h_count[k], (size_t)p->lanes * 4 * sizeof(int32_t), hipHostMallocDefault));
    for (int k = 0; k < 2; ++k) MV_HIP(hipHostMalloc((void**)&p->h_nvalid[k], (size_t)p->lanes * sizeof(int32_t), hipHostMallocDefault));
    if (c.mapping) {
        for (int k = 0; k < N_CAND; ++k) MV_HIP(hipHostMalloc((void**)&p->h_count_m[k], 4 * sizeof(int32_t), hipHostMallocDefault));
        MV_HIP(hipHostMalloc((void**)&p->h_perm_m, (size_t)c.map_num_point * sizeof(int64_t), hipHostMallocDefault));
    }
    const size_t N = (size_t)cap_of(c);
    for (int k = 0; k < N_PERM; ++k)   // (a slot holds a finish's permutations [lanes, cap] or its keypoint rows [lanes, cap, 2])
        MV_HIP(hipHostMalloc((void**)&p->h_perm[k], (size_t)p->lanes * N * 2 * sizeof(int64_t), hipHostMallocDefault));
    // constants: selector workspace zeroed once (mv_kp_select leaves it zeroed), identity pose, PGO scalars, offsets table
    MV_HIP(hipMemsetAsync(p->kp_ws, 0, p->kp_ws_bytes, p->s_main));
    if (p->kp_ws2) MV_HIP(hipMemsetAsync(p->kp_ws2, 0, p->kp_ws_bytes, p->s_main));
    const int L = p->lanes;
    std::vector<float> ident((size_t)L * 7, 0.f), intr((size_t)L * 4), bl((size_t)L, c.baseline);
    std::vector<int32_t> offs((size_t)L + 1);
    for (int l = 0; l < L; ++l) {
        ident[7 * l + 6] = 1.f;
        intr[4 * l] = c.fx; intr[4 * l + 1] = c.fy; intr[4 * l + 2] = c.cx; intr[4 * l + 3] = c.cy;
    }
    for (int l = 0; l <= L; ++l) offs[l] = (int32_t)(l * N);
    MV_HIP(hipMemcpyAsync(p->pose[0], ident.data(), ident.size() * sizeof(float), hipMemcpyHostToDevice, p->s_main));
    MV_HIP(hipMemcpyAsync(p->intr, intr.data(), intr.size() * sizeof(float), hipMemcpyHostToDevice, p->s_main));
    MV_HIP(hipMemcpyAsync(p->bl, bl.data(), bl.size() * sizeof(float), hipMemcpyHostToDevice, p->s_main));
    MV_HIP(hipMemcpyAsync(p->offs, offs.data(), offs.size() * sizeof(int32_t), hipMemcpyHostToDevice, p->s_main));
    static const float pose_norm[6] = {0.13f, 0.13f, 0.13f, 0.013f, 0.013f, 0.013f};   // TartanStereoVONetInterface.pose_norm (StereoVO_Interface.py:51-53)
    if (p->pose_norm) MV_HIP(hipMemcpyAsync(p->pose_norm, pose_norm, sizeof(pose_norm), hipMemcpyHostToDevice, p->s_main));
    p->time_detail = 1;
    MV_HIP(hipStreamSynchronize(p->s_main));   // the host vectors die here
    return MV_OK;
}

extern "C" int mv_frame_pipe_create(const mvFramePipeConfig* cfg, void* arena, size_t arena_bytes, mvFramePipe** out) {
    MV_CHECK_ARG(out && arena);
    MV_TRY(check_config(cfg));
    mvFramePipe* p = new (std::nothrow) mvFramePipe{};
    if (!p) return MV_ERR_WORKSPACE;
    derive_shape(p, cfg);
    p->arena = (char*)arena;
    p->arena_bytes = arena_bytes;
    if (((uintptr_t)arena & 255) != 0 || carve(p, p->arena) > arena_bytes) {
        delete p;
        return MV_ERR_WORKSPACE;
    }
    describe_backend(p);
    p->newest_maps = -1;
    const int rc = create_impl(p);
    if (rc != MV_OK) {
        mv_frame_pipe_destroy(p);
        return rc;
    }
    const bool have_device = hipGetDevice(&p->device) == hipSuccess;   // (the launch thread binds itself to it)
    p->async_backend = p->k.async_wish && have_device;
    if (p->async_backend) p->worker = std::thread(launch_thread_main, p);
    *out = p;
    return MV_OK;
}

extern "C" int mv_frame_pipe_set_pose(mvFramePipe* p, const float* pose7_host) {
    MV_CHECK_ARG(p && pose7_host);
    MV_TRY(flush_jobs(p));
    MV_TRY(p->e_pgo.sync());
    MV_HIP(hipMemcpy(p->pose[p->pose_cur], pose7_host, (size_t)p->lanes * 7 * sizeof(float), hipMemcpyHostToDevice));
    return MV_OK;
}

// ------------------------------------------------------------------------------------------------ frontend half
// volume GEMM of frame n_vol on its own stream; a buffer is rewritten only after the lookups that read it have finished
static int issue_volume(mvFramePipe* p, const mvFrameInputs* in, mvStream_t in_stream) {
    const mvFramePipeConfig& c = p->c;
    const long f = p->n_vol;
    const int k = (int)(f % p->k.n_volbuf);
    const int B = c.pairs;
    // inputs were produced on the caller's stream
    Ev& e_in = p->e_in[f];
    MV_TRY(e_in.record((hipStream_t)in_stream));
    p->e_in_of[k] = &e_in;
    MV_TRY(e_in.wait_if_pending(p->s_vol));
    if (p->vol_free_ev[k]) MV_TRY(p->vol_free_ev[k]->wait_if_pending(p->s_vol));
    const bool timed = p->n_timed < p->timed_cap;
    if (timed && !p->packed) MV_TRY(p->tv[0][p->n_timed].record(p->s_vol));
    if (p->packed) {
        void** pk = p->pk[f & 1];
        const PackOn on = p->k.pack_on;
        hipStream_t sp = on == PackOn::Vol ? p->s_vol : on == PackOn::Back ? p->s_back : on == PackOn::Main ? p->s_main : p->s_side;
        if (sp != p->s_vol) {
            MV_TRY(e_in.wait_if_pending(sp));
            // this operand set was last read by the GEMM of frame f - 2 (same stream order as the volume buffers' events)
            if (f >= 2) MV_TRY(p->e_vol_done[(f - 2) % p->k.n_volbuf].wait_if_pending(sp));
        }
        if (p->tiled)
            MV_TRY(mv_volume_pack_tiled((const float*)in->fmap1, (const float*)in->fmap2, pk[0], pk[1], B, c.C, p->n8, p->h8, p->w8,
                                        c.layout, c.volume_split, sp));
        else
            MV_TRY(mv_volume_pack((const float*)in->fmap1, (const float*)in->fmap2, pk[0], pk[1], B, c.C, p->n8, p->n8, c.layout,
                                  c.volume_split, sp));
        if (sp != p->s_vol) {
            MV_TRY(p->e_packed[f & 1].record(sp));
            MV_TRY(p->e_packed[f & 1].wait(p->s_vol));
        }
        // (round-4 A/B, removed: the GEMM waiting for the previous frame's lookups — each then has the chip to itself — cost 21 % of the frame rate)
        if (timed) MV_TRY(p->tv[0][p->n_timed].record(p->s_vol));   // the GEMM alone: behind the pack, wherever that ran
        MV_TRY(mv_corr_volume_packed_shared(pk[0], pk[1], p->vol[k], B, c.C, p->n8, p->n8, c.volume_split, p->k.free_cus, p->s_vol));
    } else if (c.volume_split == 2 || c.volume_split == 3) {
        const size_t nel = (size_t)B * p->n8 * c.C;
        MV_TRY(mv_split_bf16x3((const float*)in->fmap1, p->planes[0], nel, p->s_vol));
        MV_TRY(mv_split_bf16x3((const float*)in->fmap2, p->planes[1], nel, p->s_vol));
        MV_TRY(mv_corr_volume(p->planes[0], p->planes[1], p->vol[k], B, c.C, p->n8, p->n8,
                              c.volume_split == 2 ? MV_BF16X2 : MV_BF16X3, MV_LAYOUT_HWC, p->s_vol));
    } else if (p->vol16) {
        const void* op2 = in->fmap2;
        if (p->tiled) {
            MV_TRY(mv_fmap_tile_rows16(in->fmap2, p->tile16, B, c.C, p->h8, p->w8, p->s_vol));
            op2 = p->tile16;
        }
        MV_TRY(mv_corr_volume_out16(in->fmap1, op2, p->vol[k], B, c.C, p->n8, p->n2t, c.feat_dtype, c.layout, p->s_vol));
    } else {
        MV_TRY(mv_corr_volume(in->fmap1, in->fmap2, p->vol[k], B, c.C, p->n8, p->n8, c.feat_dtype, c.layout, p->s_vol));
    }
    p->vol_timed[k] = timed ? p->n_timed : -1;
    if (timed) MV_TRY(p->tv[1][p->n_timed++].record(p->s_vol));
    MV_TRY(p->e_vol_done[k].record(p->s_vol));
    p->n_vol = f + 1;
    return MV_OK;
}

// Optional early issue of the NEXT frame's volume GEMM (frame n_enq, before its mv_frame_pipe_enqueue): the GEMM only
// needs the feature maps and a free volume buffer, so the host can queue it one frame ahead — before it blocks on the
// previous frame's candidate count — and the GEMM stream never waits for the host (measured: ~93 us of idle per frame).
extern "C" int mv_frame_pipe_enqueue_volume(mvFramePipe* p, const mvFrameInputs* in, mvStream_t in_stream) {
    MV_CHECK_ARG(p && in && in->fmap1 && in->fmap2);
    MV_CHECK_ARG(p->n_vol == p->n_enq);                 // at most one GEMM ahead of its frame
    MV_CHECK_ARG(p->k.lookups_on_main);                   // the alternative layout keeps the lookups behind the GEMM on its stream
    // the volume buffer of frame n_vol was last read by the lookups of frame n_vol - 2: their event exists (frame enqueued)
    const double t_hs = p->k.host_stats ? now_us() : 0.0;
    MV_TRY(issue_volume(p, in, in_stream));
    if (p->k.host_stats) p->st_vol += now_us() - t_hs;
    // MV_PIPE_SELECTOR_ON=vol: the newest enqueued frame's selector segment goes behind this GEMM on the GEMM's stream — it needs that
    // frame's lookups, which finish about when this GEMM does, and then runs in the gap the GEMM stream idles in anyway, alone on the chip
    return p->k.sel_on == SelOn::Vol ? flush_deferred(p) : MV_OK;
}

// lean chain: the markers behind frame f's selector segment were not recorded; whoever needs them (a host-permuted finish, mv_frame_pipe_wait_candidates, a
// selector segment that depends on the previous one) records them now, on the frame's decoder-side stream — a later point of the same in-order stream
static int ensure_chain_events(mvFramePipe* p, long f, int cand_slot) {
    if (cand_slot >= 0 && !p->e_cand[cand_slot].recorded()) MV_TRY(p->e_cand[cand_slot].record(p->s_lk[f % p->k.n_lk]));
    if (p->k.alt && f >= 0 && !p->e_seg[f].recorded()) MV_TRY(p->e_seg[f].record(p->s_lk[f % p->k.n_lk]));
    return MV_OK;
}

// TartanMotionNet: the PoseNet input of the frame in maps slot m, behind the frame's epilogue on the segment's stream.  The slot was last read by the
// caller's PoseNet of frame f - N_MAPS (event of its mv_frame_pipe_set_motion, recorded on the caller's thread before this segment was described).
static int issue_motion_input(mvFramePipe* p, int m, hipStream_t s) {
    const mvFramePipeConfig& c = p->c;
    MV_TRY(p->e_motion_read[m].wait_if_pending(s));
    const Maps& mp = p->maps[m];
    MV_TRY(mv_motion_input_lanes(p->lanes, c.H, c.W, mp.match_flow, 2LL * p->plane, mp.depth, (long long)p->plane, c.fx, c.fy, c.cx, c.cy, c.bl_fx,
                                 p->motion_in[m], s));
    return p->e_motion_in[m].record(s);
}

static int issue_selector_segment(mvFramePipe* p, const SelSeg& d) {
    const mvFramePipeConfig& c = p->c;
    const mvFrameInputs* in = &d.in;
    const int k = d.k, m = d.m, ti = d.ti, B = c.pairs;
    const bool timed = d.timed, with_selector = d.with_selector, up = d.up;
    hipStream_t s = p->s_lk[d.f % p->k.n_lk];   // (same stream as the frame's lookups: in order behind them)
    if (p->k.sel_on != SelOn::Decoder) {   // everything behind the lookups continues on another stream (in order with the backends it must follow)
        s = p->k.sel_on == SelOn::Own ? p->s_sel : p->k.sel_on == SelOn::Vol ? p->s_vol : p->s_back;   // (Back and Late: the backend stream)
        MV_TRY(p->e_lk[k].wait(s));
    }
    // maps slot m and candidate slot k were last read by the backend of frame f - 2 (f - 3 for the maps) on `back`
    // (the newest backend event covers the older one: same stream)
    if (p->async_backend) {
        // Maps slot m and candidate slot k were last read by the backend of frame f - 4.  Of the three tracked frames behind it,
        // pending.size() are not finished yet and the others are the newest finishes: frame f - 4 is finish number
        // n_fin - 3 + pending.size() - 1, which the launch thread issued long ago (this wait does not block in steady state); any
        // backend event recorded at or after it orders this stream behind it (same stream).
        if (!with_selector) MV_TRY(flush_jobs(p));   // (re-)initialisation: no assumption about what is in flight
        long issued;
        {
            const long need = d.need_issued;
            MV_TRY(wait_issued(p, need < 0 ? 0 : need));
            std::lock_guard<std::mutex> lk(p->mu);
            issued = p->issued;
        }
        // (device-driven frame: a finish is issued right behind its frame's enqueue, so "the newest issued backend" would be the PREVIOUS frame's and the
        // segments would run one after the other; the ring holds the exact finish — frame f - 4's, long done — instead)
        const long w = p->dev_draw ? d.need_issued - 1 : issued - 1;
        if (w >= 0 && w < issued) MV_TRY(p->e_backend[w].wait_if_pending(s));
    } else if (p->n_fin > 0) {
        const long w = p->dev_draw ? d.need_issued - 1 : p->n_fin - 1;
        if (w >= 0) MV_TRY(p->e_backend[w].wait_if_pending(s));
    }
    MV_TRY(p->e_release.wait_if_pending(s));   // ... and by consumers of result views (mv_frame_pipe_release)
    // alt: the previous frame's segment ran on the OTHER decoder-side stream; this one reads its maps (FULL selector, and the backend's gathers
    // behind e_cand) and shares the selector workspace / upsampling buffers with it
    // (alt_indep: NODEPTH selector without upsampling reads nothing of the previous frame and has its own workspace — the segments may overlap and
    // the BACKEND waits for the previous frame's segment instead, finish_issue)
    const bool indep = p->k.alt_indep && !up && (c.selector_mode == MV_KP_NODEPTH || kp_new_mode(c.selector_mode));
    if (p->k.alt && !indep && d.f > 0) {
        MV_TRY(ensure_chain_events(p, d.f - 1, -1));
        MV_TRY(p->e_seg[d.f - 1].wait_if_pending(s));
    }
    void* const kp_ws = (indep && (d.f & 1)) ? p->kp_ws2 : p->kp_ws;
    Maps& mp = p->maps[m];
    const int nocov = c.frontend_nocov;
    // epilogue + the selector's first kernel in ONE launch (one launch and one pass over the maps less on the chain that bounds a single-sequence stream):
    // the NODEPTH selector on full-resolution inputs with both covariances
    const bool fused_select = with_selector && !up && !nocov && c.selector_mode == MV_KP_NODEPTH;
    if (up) {
        MV_TRY(upsample_frame(p, in->flow8, in->up_mask, p->up_flow, B, 0.25f, 0, s));
        if (!nocov) {
            MV_TRY(upsample_frame(p, in->cov8, in->cov_mask, p->up_cov, B, 1.0f, 1, s));
        } else if (nocov != (MV_NOCOV_DEPTH | MV_NOCOV_MATCH)) {
            // one side only: the covariance field of THAT pair of every lane (pair 2l = lane l's stereo pair, 2l + 1 its temporal pair); the other pair's
            // planes of cov8 / cov_mask / up_cov are neither read nor written
            for (int l = 0; l < p->lanes; ++l) {
                const size_t pr = 2 * (size_t)l + ((nocov & MV_NOCOV_DEPTH) ? 1 : 0);
                MV_TRY(upsample_frame(p, in->cov8 + pr * 2 * p->n8, in->cov_mask + pr * 576 * p->n8, p->up_cov + pr * 2 * p->plane, 1, 1.0f, 1, s));
            }
        }
        MV_TRY(mv_frontend_epilogue_lanes(p->up_flow, p->up_cov, 0, c.H, c.W, c.bl_fx, c.bl_fx_sq, mp.disparity,
                                          mp.disparity_cov, mp.depth, mp.depth_cov, nullptr, mp.match_flow, mp.match_cov,
                                          p->lanes, s));
    } else if (!fused_select) {
        MV_TRY(mv_frontend_epilogue_lanes(in->flow, in->logcov, 1, c.H, c.W, c.bl_fx, c.bl_fx_sq, mp.disparity,
                                          mp.disparity_cov, mp.depth, mp.depth_cov, nullptr, mp.match_flow, mp.match_cov,
                                          p->lanes, s));
    }
    const Pending pd{m, d.maps_prev, k, with_selector, ti};
    if (with_selector && c.motion_model == MV_MOTION_TARTAN && !fused_select) MV_TRY(issue_motion_input(p, m, s));
    if (with_selector) {
        mvKpSelectParams sp{c.H, c.W, c.selector_mode, c.kp_kernel_size, c.kp_mask_width, c.max_depth, c.max_depth_cov,
                            c.max_match_cov};
        const bool sel_kernels = !kp_new_mode(c.selector_mode);   // (Random / Grid / explicit keypoints: the segment ends with the epilogue)
        if (!sel_kernels) {
            // (nothing: the maps are written, the keypoints come with the finish)
        } else if (fused_select) {
            MV_TRY(mv_frontend_epilogue_select_lanes(in->flow, in->logcov, 1, c.bl_fx, c.bl_fx_sq, mp.disparity, mp.disparity_cov,
                                                     mp.depth, mp.depth_cov, nullptr, mp.match_flow, mp.match_cov, nullptr,
                                                     nullptr, &sp, kp_ws, p->kp_ws_bytes, p->cand[k], p->count[k],
                                                     p->stats[k], p->lanes, s));
            if (c.motion_model == MV_MOTION_TARTAN) MV_TRY(issue_motion_input(p, m, s));   // (the fused launch wrote the maps)
        } else if (c.selector_mode == MV_KP_NODEPTH) {
            MV_TRY(mv_kp_select_lanes(mp.match_cov, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &sp, kp_ws,
                                      p->kp_ws_bytes, p->cand[k], p->count[k], p->stats[k], p->lanes, s));
        } else {
            const Maps& m0 = p->maps[pd.maps_prev];
            MV_TRY(mv_kp_select_lanes(mp.match_cov, m0.depth, m0.depth_cov, mp.depth, mp.depth_cov, nullptr, nullptr, &sp,
                                      p->kp_ws, p->kp_ws_bytes, p->cand[k], p->count[k], p->stats[k], p->lanes, s));
        }
        if (!p->dev_draw && sel_kernels)   // (the device-driven frame reads the count where it is)
            MV_HIP(hipMemcpyAsync(p->h_count[k], p->count[k], (size_t)p->lanes * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (c.mapping) {
            // MappingPointSelector works on the PREVIOUS frame's depth maps (KeypointSelector.py:87-100; MACVO.py:315): its count
            // travels to the host with the tracking selector's
            const Maps& m0 = p->maps[pd.maps_prev];
            mvKpSelectParams spm{c.H, c.W, MV_KP_MAPPING, c.kp_kernel_size, c.map_mask_width, c.map_max_depth, c.map_max_depth_cov,
                                 c.max_match_cov};
            MV_TRY(mv_kp_select_lanes(nullptr, m0.depth, m0.depth_cov, nullptr, nullptr, nullptr, nullptr, &spm, p->kp_ws,
                                      p->kp_ws_bytes, p->cand_m[k], p->count_m[k], p->stats_m[k], 1, s));
            MV_HIP(hipMemcpyAsync(p->h_count_m[k], p->count_m[k], 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        // lean chain (device-driven, front launch in order behind this segment, segments independent): no marker here — e_cand is recorded on demand
        // (ensure_chain_events) and nothing waits for e_seg
        const bool no_markers = p->k.no_segment_markers && p->dev_draw && indep;
        if (no_markers) p->e_cand[k].skip();
        else MV_TRY(p->e_cand[k].record(s));
        if (timed) MV_TRY(p->tv[3][ti].record(s));
        if (p->k.alt) {
            if (no_markers) p->e_seg[d.f].skip();
            else MV_TRY(p->e_seg[d.f].record(s));
        }
    } else if (p->k.alt) {
        MV_TRY(p->e_seg[d.f].record(s));
    }
    return MV_OK;
}

static int flush_deferred(mvFramePipe* p) {
    if (!p->deferred_valid) return MV_OK;
    p->deferred_valid = false;
    return issue_selector_segment(p, p->deferred);
}
// in front of a wait for / finish of the OLDEST pending frame: its selector segment must have been issued.  MV_PIPE_SELECTOR_ON=late keeps
// the newest frame's segment for the finish that is about to happen, unless that newest frame IS the oldest pending one; a segment that
// travelled with an earlier finish has been issued once the launch thread is through with that job.
static int selector_of_front_issued(mvFramePipe* p) {
    if (p->k.sel_on != SelOn::Late || p->pending.size() <= 1) MV_TRY(flush_deferred(p));
    const long sj = p->pending.empty() ? -1 : p->pending.front().sel_job;
    return sj >= 0 ? wait_issued(p, sj + 1) : MV_OK;
}

extern "C" int mv_frame_pipe_enqueue(mvFramePipe* p, const mvFrameInputs* in, mvStream_t in_stream, int with_selector) {
    MV_CHECK_ARG(p && in && in->fmap1 && in->fmap2);
    const mvFramePipeConfig& c = p->c;
    MV_CHECK_ARG(c.iters == 0 || in->coords);
    const bool up = in->flow8 != nullptr;
    const bool any_cov = c.frontend_nocov != (MV_NOCOV_DEPTH | MV_NOCOV_MATCH);   // (a frontend without covariances hands over no logcov / cov8 / cov_mask)
    MV_CHECK_ARG(up ? (in->up_mask && (!any_cov || (in->cov8 && in->cov_mask))) : (in->flow && (!any_cov || in->logcov)));
    const long f = p->n_enq;
    const int k = (int)(f % N_CAND), m = (int)(f % N_MAPS);
    MV_CHECK_ARG(!with_selector || p->newest_maps >= 0);   // a tracked frame needs the previous frame's maps
    MV_CHECK_ARG(!with_selector || (int)p->pending.size() < MAX_PENDING);  // slot rotation covers MAX_PENDING tracked frames in flight
    const int B = c.pairs;
    const double t_hs0 = p->k.host_stats ? now_us() : 0.0;
    MV_TRY(flush_deferred(p));   // (the previous frame's selector segment, had nobody asked for it yet: frames stay in order)

    // ---- volume GEMM (own stream) unless mv_frame_pipe_enqueue_volume already issued it
    const bool ahead = p->n_vol != f;
    if (!ahead) MV_TRY(issue_volume(p, in, in_stream));
    const int kv = (int)(f % p->k.n_volbuf);   // volume buffer of this frame (k = its candidate / backend slot)
    const int ti = p->time_detail ? p->vol_timed[kv] : -1;   // timeline slot (the GEMM's own event pair was recorded by issue_volume)
    const bool timed = ti >= 0;

    // ---- decoder side on `main`, overlapping the next frame's GEMM.  (MV_PIPE_LOOKUPS_ON=vol keeps the lookups on the
    // GEMM's stream instead — no cross-stream event in front of the first lookup, GEMM undisturbed at 215 us — measured
    // 0.3256 vs 0.3197 ms per frame: behind a 215-us kernel each of the 12 launch boundaries costs ~9 us.)
    const size_t coord_stride = (size_t)B * 2 * p->n8;
    const int lk = (int)(f % p->k.n_lk);
    hipStream_t s = p->s_lk[lk];
    float* const* tok = p->tok + 2 * lk;
    if (ahead) {   // the GEMM's input event predates this call: order the decoder side after the caller's stream as of NOW
        MV_TRY(p->e_rest[f].record((hipStream_t)in_stream));
        MV_TRY(p->e_rest[f].wait_if_pending(s));
    }
    if (p->k.lookups_on_main) {
        MV_TRY(p->e_vol_done[kv].wait(s));   // also orders `s` after e_in (the GEMM stream waited for it)
        for (int it = 0; it < c.iters; ++it)
            MV_TRY(mv_lookup(p->vol[kv], p->vol16, p->tiled, in->coords + it * coord_stride, tok[it & 1], B, p->h8, p->w8, p->h8, p->w8, c.radius, s));
        // lean chain: this frame's front launch (same stream, behind the lookups) releases the buffer — its ring event exists before the GEMM that rewrites the
        // buffer is issued (that GEMM belongs to frame f + n_volbuf, enqueued only after this frame has been finished: MAX_PENDING < n_volbuf)
        const bool freed_by_front = p->k.front_frees_volume && p->dev_draw && with_selector && c.num_point > 0;
        if (freed_by_front) {
            p->vol_free_ev[kv] = &p->e_backend[p->n_fin + (long)p->pending.size()];
        } else {
            MV_TRY(p->e_vol_free[kv].record(s));
            p->vol_free_ev[kv] = &p->e_vol_free[kv];
        }
        if (timed) MV_TRY(p->tv[2][ti].record(s));
    } else {
        for (int it = 0; it < c.iters; ++it)
            MV_TRY(mv_lookup(p->vol[kv], p->vol16, p->tiled, in->coords + it * coord_stride, tok[it & 1], B, p->h8, p->w8, p->h8, p->w8, c.radius, p->s_vol));
        MV_TRY(p->e_vol_done[kv].record(p->s_vol));   // volume AND its lookups done
        MV_TRY(p->e_vol_done[kv].wait(s));            // also orders `s` after e_in
        p->vol_free_ev[kv] = nullptr;                 // vol[k] / tok are only touched on s_vol: stream order suffices
    }

    const double t_hs1 = p->k.host_stats ? now_us() : 0.0;
    SelSeg d{*in, f, k, m, ti, p->newest_maps, timed, with_selector != 0, up,
             p->n_fin - MAX_PENDING + (long)p->pending.size()};
    if (p->k.sel_on != SelOn::Decoder) MV_TRY(p->e_lk[k].record(s));   // the segment continues on another stream behind the last lookup
    // MV_PIPE_SELECTOR_ON=late: with two unfinished frames in front of it (the steady state of a 3-deep pipeline) the segment is
    // handed to the NEXT finish, which issues it right behind that frame's backend: the backend stream then holds
    // backend(f - 2), selector(f), backend(f - 1), selector(f + 1) ... — a backend waits behind ONE queued selector segment (whose
    // lookups are done by then) instead of two that still wait for their lookups (frame latency: see DESIGN, backend timeline)
    const bool late = p->k.sel_on == SelOn::Late && with_selector && p->pending.size() >= 2;
    if ((p->k.sel_on == SelOn::Vol && with_selector) || late) {
        p->deferred = d;            // issued behind the next frame's GEMM (mv_frame_pipe_enqueue_volume) / the next backend, or by whoever needs it first
        p->deferred_valid = true;
    } else {
        MV_TRY(issue_selector_segment(p, d));
    }
    if (with_selector) p->pending.push_back(Pending{m, p->newest_maps, k, true, ti, -1, f});
    p->newest_maps = m;
    p->n_enq = f + 1;
    if (p->k.host_stats) {
        const double t_hs2 = now_us();
        p->st_enq += t_hs2 - t_hs0;
        p->st_enq_lookups += t_hs1 - t_hs0;
        p->st_enq_seg += t_hs2 - t_hs1;
    }
    return MV_OK;
}

extern "C" int mv_frame_pipe_wait_motion_input(mvFramePipe* p, mvStream_t stream) {
    MV_CHECK_ARG(p && p->c.motion_model == MV_MOTION_TARTAN && !p->pending.empty() && p->pending.back().f == p->n_enq - 1);
    // the newest frame's selector segment (which writes the PoseNet input) must have been issued
    const long sj = p->pending.back().sel_job;
    if (sj >= 0) MV_TRY(wait_issued(p, sj + 1));
    else MV_TRY(flush_deferred(p));
    const int m = (int)((p->n_enq - 1) % N_MAPS);
    MV_CHECK_ARG(p->e_motion_in[m].recorded());
    return p->e_motion_in[m].wait((hipStream_t)stream);
}

extern "C" int mv_frame_pipe_set_motion(mvFramePipe* p, const float* motion_dev, mvStream_t stream) {
    MV_CHECK_ARG(p && motion_dev && p->c.motion_model == MV_MOTION_TARTAN && !p->pending.empty() && p->pending.back().f == p->n_enq - 1);
    const long g = p->n_fin + (long)p->pending.size() - 1;   // the finish index of the newest enqueued tracked frame
    const int k = (int)(g % N_MOT);
    hipStream_t s = (hipStream_t)stream;
    // the slot's previous user, finish g - N_MOT, composed its prior on the solve's stream: that launch must have been ISSUED before its event means anything
    if (p->e_motion_used[g].recorded()) {
        MV_TRY(wait_issued(p, g - N_MOT + 1));
        MV_TRY(p->e_motion_used[g].wait(s));
    }
    MV_HIP(hipMemcpyAsync(p->motion_raw[k], motion_dev, (size_t)p->lanes * 6 * sizeof(float), hipMemcpyDeviceToDevice, s));
    MV_TRY(p->e_motion_set[g].record(s));   // recorded before the frame's finish is queued: its solve waits for it
    p->motion_g[k] = g;
    return p->e_motion_read[p->n_enq - 1].record(s);   // ... and the PoseNet's reads of this frame's input are behind this point of `stream`
}

extern "C" int mv_frame_pipe_wait_candidates(mvFramePipe* p, int32_t* n_cand) {
    MV_CHECK_ARG(p && n_cand && !p->pending.empty());
    MV_TRY(selector_of_front_issued(p));
    const Pending& pd = p->pending.front();
    MV_TRY(ensure_chain_events(p, pd.f, pd.cand));
    if (kp_new_mode(p->c.selector_mode)) {   // no candidate list: the frame's row count is known (the mapping selector's count still travels behind e_cand)
        if (p->c.mapping) MV_TRY(p->e_cand[pd.cand].sync());
        for (int l = 0; l < p->lanes; ++l) n_cand[l] = frame_rows(p->c);
        return MV_OK;
    }
    MV_TRY(p->e_cand[pd.cand].sync());
    if (p->dev_draw)   // (the device-driven pipe has no per-frame count copy)
        MV_HIP(hipMemcpy(p->h_count[pd.cand], p->count[pd.cand], (size_t)p->lanes * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int l = 0; l < p->lanes; ++l) n_cand[l] = p->h_count[pd.cand][4 * l];
    return MV_OK;
}

// ------------------------------------------------------------------------------------------------ native permutations
// `selected[torch.randperm(n)[:numPoint]]` (Module/KeypointSelector.py:331,404) draws from torch's CPU generator, which is a
// standard MT19937 (at::mt19937, init_genrand(seed & 0xffffffff)), and torch.randperm on the CPU is the plain Fisher-Yates
//     r = arange(n); for i in 0 .. n - 2: z = random32() % (n - i); swap(r[i], r[i + z])          (ATen randperm_cpu, n < 2^32 / 20)
// Position i is final after iteration i, so the first numPoint outputs need numPoint swaps; the other n - 1 - numPoint draws only
// advance the generator.  One lane of the reference's own call costs ~45 us at n = 8000; 32 lanes are 1.4-3 ms per step on the
// host — more than the 2.6 ms volume GEMM of the whole batch leaves idle (measured: 1.9 ms of GEMM-stream idle per 32-lane step).
// Here: ~2 ns per draw, no allocation.  Identical bits to `torch.Generator().manual_seed(seed)` + torch.randperm
// (tests/test_gpu_lanes.py::test_native_seeded_lanes_equal_torch_generators).
extern "C" int mv_frame_pipe_seed_lanes(mvFramePipe* p, const uint64_t* seeds) {
    MV_CHECK_ARG(p && seeds);
    MV_TRY(flush_jobs(p));   // the launch thread's draw_perms reads rng / perm_host
    p->rng.clear();
    for (int l = 0; l < p->lanes; ++l) p->rng.emplace_back((uint32_t)(seeds[l] & 0xffffffffull));
    const int cap = cap_of(p->c);
    p->perm_host.assign((size_t)p->lanes * cap * (p->c.selector_mode == MV_KP_RANDOM ? 2 : 1), 0);
    p->nsel_host.assign((size_t)p->lanes, 0);
    {
        // ... and the same generators in device memory: the device-driven frame (default wherever it applies; Knobs::device_draw_wish).
        // Needs the two-launch backend, a head the device draw covers, and no dense-mapping tail (its second permutation is drawn by the Python side).
        p->dev_draw = p->k.device_draw_wish && p->k.fuse_backend && !p->c.mapping && p->c.num_point >= 1 && p->c.num_point <= mv_randperm_max_head() && p->pending.empty() &&
                      p->c.selector_mode != MV_KP_GRID && p->c.selector_mode != MV_KP_EXPLICIT;   // (nothing to draw)
        if (p->dev_draw && p->async_backend && !p->k.async_explicit && affinity_cores() < 3) {
            // One host thread on small hosts.  The launch thread existed to overlap the host draw + the backend launches with the caller's next enqueue while the caller
            // waited for candidate counts; a device-driven frame has no wait and no draw, and one thread issues it in ~105-140 us — about the frame period.  With the lean
            // chain (below) that is the edge: measured (profiles/r06_chain_gaps.log) one thread 6.99 / 6.85 / 6.64 k frames/s at 300 steps with issue times of 115 / 134 /
            // 143 us, with the launch thread taking the two backend launches (caller 92-103 us) 6.90 / 6.97 / 6.93 k and no low outliers on the 20-step line; pinned to one
            // or two cores both forms run at 5.9-6.1 k (the host-drawn frame: 3.9 k on one core).  So: the launch thread stays where the process has >= 3 cores.
            MV_TRY(flush_jobs(p));
            {
                std::lock_guard<std::mutex> lk(p->mu);
                p->stop = true;
            }
            p->stop_flag.store(true, std::memory_order_relaxed);
            p->cv_job.notify_all();
            if (p->worker.joinable()) p->worker.join();
            p->async_backend = 0;
        }
        if (p->dev_draw) {
            const size_t W = (size_t)mv_randperm_state_words();
            std::vector<uint32_t> st((size_t)p->lanes * W);
            for (int l = 0; l < p->lanes; ++l) MV_TRY(mv_mt19937_seed(seeds[l], st.data() + (size_t)l * W));
            MV_TRY(sync_streams(p, ST_BACK));      // (no front launch may be reading a generator: they run on the backend stream or on the
            MV_TRY(sync_streams(p, ST_DECODER));   //  decoder-side streams)
            MV_HIP(hipMemcpy(p->rp_state[p->n_fin & 1], st.data(), st.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
    }
    return MV_OK;
}

extern "C" int mv_frame_pipe_device_draw(const mvFramePipe* p) { return p && p->dev_draw ? 1 : 0; }
extern "C" int mv_frame_pipe_volume_tiled(const mvFramePipe* p) { return p && p->tiled ? 1 : 0; }   // the volume buffers' slices are in 4 x 4-cell tiles
extern "C" int mv_frame_pipe_host_threads(const mvFramePipe* p) { return p ? (p->async_backend ? 2 : 1) : 0; }   // the caller's (+ the backend launch thread)

static void randperm_head(std::mt19937& eng, int64_t n, int k, std::vector<int32_t>& r, int64_t* out) {
    if (n <= 0) return;
    if ((int64_t)r.size() < n) r.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) r[(size_t)i] = (int32_t)i;
    const int64_t swaps = k < n - 1 ? k : n - 1;
    for (int64_t i = 0; i < swaps; ++i) {
        const int64_t z = (int64_t)((uint32_t)eng()) % (n - i);
        const int32_t sav = r[(size_t)i];
        r[(size_t)i] = r[(size_t)(i + z)];
        r[(size_t)(i + z)] = sav;
    }
    if (n - 1 > swaps) eng.discard((unsigned long long)(n - 1 - swaps));   // the draws of the remaining iterations
    const int64_t m = k < n ? k : n;
    for (int64_t i = 0; i < m; ++i) out[i] = r[(size_t)i];
}

// ------------------------------------------------------------------------------------------------ pose-dependent half
// Host part of a finish: validate, take the frame off the pending list, rotate the slots and update everything the caller's
// thread reads afterwards (views, counts).  No HIP call.
static int finish_host(mvFramePipe* p, const int32_t* n_sel, float* pose_sink, FinishJob& j) {
    const mvFramePipeConfig& c = p->c;
    const int L = p->lanes;
    int n_max = 0;
    for (int l = 0; l < L; ++l) {
        MV_CHECK_ARG(n_sel[l] >= 0 && n_sel[l] <= table_rows(c));
        n_max = n_sel[l] > n_max ? n_sel[l] : n_max;
    }
    MV_CHECK_ARG(c.motion_model != MV_MOTION_TARTAN || p->motion_g[p->n_fin % N_MOT] == p->n_fin);   // mv_frame_pipe_set_motion for this frame first
    j.pd = p->pending.front();
    p->pending.pop_front();
    j.g = p->n_fin;
    j.has_sel = false;
    if (p->k.sel_on == SelOn::Late && p->deferred_valid && !p->pending.empty()) {   // (never the frame being finished: flush_deferred ran first)
        j.sel = p->deferred;
        j.has_sel = true;
        p->deferred_valid = false;
        p->pending.back().sel_job = j.g;
    }
    j.n_max = n_max;
    j.pose_sink = pose_sink;
    Backend& b = p->be[j.g & 1];
    for (int l = 0; l < L; ++l) b.n_sel[l] = j.n_sel[l] = n_sel[l];
    b.rows_dev = j.kp == KPJ_DEV;
    p->n_fin = j.g + 1;
    j.skipped = p->skipped;
    p->skipped = false;
    p->prior_slot = p->pose_cur;
    j.pose_from = p->pose_cur;
    j.pose_to = (p->pose_cur + 1) % 3;
    p->pose_cur = j.pose_to;
    p->mp_rows = 0;
    if (n_max > 0) {
        p->last_maps_prev = j.pd.maps_prev;
        p->last_cand = j.pd.cand;
    }
    return MV_OK;
}

// Where a finish's front launch takes its keypoint rows from (ps: the job's pinned permutation slot)
static mvKpSource kp_source_of(const mvFramePipe* p, const FinishJob& j, const Backend& b, int ps, bool perm_in_args) {
    mvKpSource src{};
    src.num_point = p->c.num_point; src.mask_width = p->c.kp_mask_width;
    src.state_in = p->rp_state[j.g & 1]; src.state_out = p->rp_state[(j.g + 1) & 1];   // (DRAW / RANDOM: finish g reads one state buffer and writes the other)
    if (j.kp == KPJ_PERM) {
        src.kind = j.device ? MV_KPSRC_DRAW : MV_KPSRC_PERM;
        src.cand = p->cand[j.pd.cand]; src.cand_lane_stride = (size_t)p->plane;
        if (j.device) {   // device-driven frame: the front launch draws the permutation itself (count and generator in device memory) and publishes the live-row count
            src.n_live_dev = p->count[j.pd.cand]; src.n_live_stride = 4;
            src.out_perm = b.perm; src.out_live = b.live_dev;
        } else {
            src.perm_dev = b.perm; src.perm_host = perm_in_args ? p->h_perm[ps] : nullptr;
            src.n_live = j.n_sel;
        }
    } else if (j.kp == KPJ_RANDOM || j.kp == KPJ_GRID) {
        // RandomSelector drawn inside the launch from the lane's device-resident generator, GridSelector computed from the row index
        src.kind = j.kp == KPJ_RANDOM ? MV_KPSRC_RANDOM : MV_KPSRC_GRID;
    } else if (j.kp == KPJ_DEV) {   // the caller's rows, read where they are; the live-row count stays on the device
        src.kind = MV_KPSRC_ROWS;
        src.rows = j.kp_dev; src.n_live_dev = j.nsel_dev; src.n_live_stride = 1; src.out_live = b.live_dev;
    } else {                        // ... or host rows, copied into kp0, which the front launch then reads in place
        src.kind = MV_KPSRC_ROWS;
        src.rows = b.kp0; src.n_live = j.n_sel;
    }
    return src;
}

// Device part: every launch of the frame's backend + solve.  Runs on the caller's thread, or on the launch thread (then it must
// not touch anything but the job, the Backend slot and the launch thread's own events / flags; what describe_backend laid out is read-only).
static int finish_issue(mvFramePipe* p, const FinishJob& j, const int64_t* perm_host) {
    const mvFramePipeConfig& c = p->c;
    const int L = p->lanes, cap = cap_of(c);
    const int n_max = j.n_max;
    const Pending& pd = j.pd;
    const long g = j.g;
    const int k = (int)(g & 1);
    Backend& b = p->be[k];
    const int32_t* n_sel = j.n_sel;
    // front_on_decoder (device-driven frames of the alt layout): the pose-independent launch goes behind the frame's own selector segment on its decoder-side
    // stream — in order, so no barrier for the selector; consecutive frames' front launches (other decoder-side stream each) are chained by the ring event of the
    // previous finish, which also orders the generator's state buffers and covers the previous frame's segment
    const bool on_dec = j.device && p->k.front_on_decoder;
    hipStream_t s = on_dec ? p->s_lk[j.pd.f % p->k.n_lk] : p->s_back;
    // a finish that draws nothing on the device, in a device-driven pipe: the generators move on to the buffer the NEXT finish reads, unchanged
    const auto pass_generators = [&] {
        return hipMemcpyAsync(p->rp_state[(g + 1) & 1], p->rp_state[g & 1], (size_t)L * (size_t)mv_randperm_state_words() * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
    };
    if (n_max == 0 && p->dev_draw) MV_HIP(pass_generators());
    const bool motion = c.motion_model == MV_MOTION_TARTAN;
    float* const prior = motion ? p->prior[g % N_MOT] : nullptr;
    if (motion) {   // prior = previous pose @ Exp(raw * pose_norm), on the solve's stream behind the previous solve and the caller's set_motion
        MV_TRY(p->e_motion_set[g].wait(p->s_side));
        MV_TRY(mv_pose_exp_compose(L, p->pose[j.pose_from], p->motion_raw[g % N_MOT], 6, p->pose_norm, prior, p->s_side));
        MV_TRY(p->e_motion_used[g].record(p->s_side));
    }
    if (n_max == 0) {   // nothing to track in any lane: the poses stay at the motion-model prior (MACVO.py:303-307)
        // The pose slots still rotate (MV_FB_POSE age a = the pose after the a-th newest finish) and the slot's events are
        // refreshed, so that everything keyed on "slot of finish g" (mv_frame_pipe_map_append, result views) sees this frame and
        // not the one two finishes back.  In-order on the side stream: behind the previous solve, no extra wait needed.
        MV_HIP(hipMemcpyAsync(p->pose[j.pose_to], motion ? prior : p->pose[j.pose_from], (size_t)L * 7 * sizeof(float), hipMemcpyDeviceToDevice,
                              p->s_side));
        if (j.pose_sink)
            MV_HIP(hipMemcpyAsync(j.pose_sink, p->pose[j.pose_to], (size_t)L * 7 * sizeof(float), hipMemcpyDeviceToDevice, p->s_side));
        MV_TRY(p->e_posed[k].record(p->s_side));
        MV_TRY(p->e_pgo.record(p->s_side));
        MV_TRY(p->e_solved[k].record(p->s_side));
        MV_TRY(p->e_cand[pd.cand].wait_if_pending(s));   // (lean chain: this frame's ring event also releases its volume buffer — not before its lookups are through)
        MV_TRY(p->e_backend[g].record(s));
        p->e_nvalid[k].skip();   // (mv_frame_pipe_wait_tracked then reports 0 observations: no mapping either)
        return MV_OK;
    }
    const mvFrontMaps fm{p->maps[pd.maps].match_flow, p->maps[pd.maps].match_cov, p->maps[pd.maps_prev].dm, p->maps[pd.maps].dm};
    const mvFrontTables& t = b.front;

    // Slot reuse.  This backend slot's tables were last read by the solve of frame g - 2 (side stream) and by whoever looked at
    // that frame's result views: the former has its event, the latter the event of mv_frame_pipe_release (a consumer that
    // reads views asynchronously on its own stream calls it before it asks for the next frame).
    if (s != p->s_side) MV_TRY(p->e_solved[k].wait_if_pending(s));   // (alt layout: backend and solve share one in-order stream)
    MV_TRY(p->e_release.wait_if_pending(s));
    // ... and by the map append (map_append_finished) of frame g - 2 on the backend stream: in order with a front launch that runs there, an event for one on a
    // decoder-side stream (a 64-lane append takes longer than a one-lane one: timing does not hold this off)
    if (s != p->s_back) MV_TRY(p->e_mapl[k].wait_if_pending(s));
    // permutations [lanes, cap] -> pinned slot -> device (ONE copy; rows beyond a lane's n_sel are never read)
    const int ps = (int)(g % N_PERM);
    if (!j.device && p->dev_draw) MV_HIP(pass_generators());   // (a host-permuted finish)
    const bool host_rows = !j.device && (j.kp == KPJ_PERM || j.kp == KPJ_HOST);   // a permutation or (u, v) rows from the host
    const size_t rw = j.kp == KPJ_HOST ? 2 : 1;                                     // int64 words per row
    if (host_rows) {
        MV_TRY(p->e_perm[g].sync());   // long done; keeps the slot reuse provably safe
        for (int l = 0; l < L; ++l)
            memcpy(p->h_perm[ps] + (size_t)l * cap * rw, perm_host + (size_t)l * cap * rw, (size_t)n_sel[l] * rw * sizeof(int64_t));
    }
    if (j.kp == KPJ_DEV) MV_TRY(p->e_kpin[g].wait(s));   // the caller's stream as of mv_frame_pipe_finish_keypoints_dev
    if (!on_dec) MV_TRY(p->e_cand[pd.cand].wait_if_pending(s));   // fired: the host has just read this frame's count (device-driven: a pending barrier)
    else if (g > 0) MV_TRY(p->e_backend[g - 1].wait_if_pending(s));
    // alt layout: the previous frame's maps (gathers below) were written by a segment on the other decoder-side stream, which e_cand does not cover.
    // (Slot f - 1 of e_seg is re-recorded by frame f - 1 + N_INEV, far beyond the frames in flight.)
    // ... unless the previous frame's backend ran on THIS stream and waited for that segment itself (its e_cand is recorded at the same point): stream order
    // then covers it, and a pending cross-queue barrier less sits in front of the backend (device-driven frames are issued long before their selector is done;
    // every unsatisfied barrier at the head of a queue costs the other queues dispatch latency, profiles/r06_device_draw_ab.log)
    const bool prev_here = p->k.alt && p->last_backend_frame == pd.f - 1;   // (on_dec: the previous front launch's event, waited for above, covers it too)
    if (p->k.alt && pd.f > 0 && !prev_here) MV_TRY(p->e_seg[pd.f - 1].wait_if_pending(s));
    p->last_backend_frame = pd.f;
    const int ti = pd.ti;
    if (ti >= 0) MV_TRY(p->tv[4][ti].record(s));
    const bool perm_in_args = j.kp == KPJ_PERM && L == 1 && n_max <= 256;   // one lane: the permutation rides in the kernel arguments (no pinned staging copy, no H2D node)
    if (!perm_in_args && host_rows) {   // (keypoint rows go straight into the frame's kp0 table, which the front launch then reads in place)
        const size_t perm_bytes = ((size_t)(L - 1) * cap + n_sel[L - 1]) * rw * sizeof(int64_t);
        MV_HIP(hipMemcpyAsync(j.kp == KPJ_HOST ? b.kp0 : b.perm, p->h_perm[ps], perm_bytes, hipMemcpyHostToDevice, s));
        MV_TRY(p->e_perm[g].record(s));
    }
    // Pose-INDEPENDENT part first: it overlaps the previous frames' solves.  The chain solve(t-1) -> backend(t) -> solve(t) is the
    // sequential dependency of visual odometry and, beside a GEMM that never pauses, it was the period of a single-sequence
    // stream (track 19 + back-projection 9 + covariances 48 + filters 21 + solve 108 us + launch gaps and two stream hops =
    // ~290 us).  Only the rotation into the world frame needs the previous pose (MACVO.py:273-281): it runs as one tiny kernel on
    // the SOLVE's stream right behind the previous solve, so the critical chain is solve -> mv_pose_apply_lanes -> solve on one
    // in-order stream.
    const bool fused = p->k.fuse_backend != 0;
    const mvKpSource src = kp_source_of(p, j, b, ps, perm_in_args);
    const auto obs_filter = [&] {
        return mv_obs_filter_lanes(t.inbound, t.cov0, t.cov1, t.vals, c.filters, c.filter_min_depth, c.max_depth, L, n_sel, cap, b.valid, b.n_valid, s);
    };
    if (fused || src.kind != MV_KPSRC_PERM) {
        // gather + track + back-projection + both covariance models = ONE launch
        MV_TRY(mv_backend_front(src, L, cap, fm, p->cov, t, s));
        // (the observation filters: prologue of the solve's launch below; mapping mode needs the count on the host first and keeps the launch)
        if (c.mapping && src.kind != MV_KPSRC_DRAW) MV_TRY(obs_filter());
    } else {   // MV_PIPE_FUSE_BACKEND=0: the five-launch form (the reference point of the bitwise test)
        MV_TRY(mv_kp_front_lanes(src.cand, src.cand_lane_stride, src.perm_dev, src.perm_host, L, n_sel, cap, fm.match_flow, fm.match_cov, fm.f0.depth,
                                 fm.f0.disp, fm.f0.sdisp, fm.f0.sdd, fm.f1.depth, fm.f1.disp, fm.f1.sdisp, fm.f1.sdd, c.H, c.W, c.edgewidth,
                                 c.match_cov_default, c.fx, c.fy, c.cx, c.cy, t.kp0_uv, t.kp0, t.kp1, t.inbound, t.vals, t.sigma0, t.sigma1, t.pos_Tc, s));
    }
    if (!fused) {   // (behind a fused front launch — keypoint rows — the covariances are computed again: same bits)
        mvObsCovLaunch d{};
        d.model = p->cov.model; d.modifiers = p->cov.modifiers; d.params = &p->cov.cp; d.lanes = L; d.n_live = n_sel; d.cap = cap;
        d.pair = true;
        d.set0.depth_map = fm.f0.depth; d.set0.kp_uv = t.kp0; d.set0.flow_cov = t.sigma0; d.set0.out_cov = t.cov0;
        d.set1.depth_map = fm.f1.depth; d.set1.kp_uv = t.kp1; d.set1.flow_cov = t.sigma1; d.set1.out_cov = t.cov1;
        d.depth_cov_map0 = fm.f0.sdd; d.depth_cov_map1 = fm.f1.sdd;
        if (c.frontend_nocov & MV_NOCOV_MATCH) {   // (set 1: the model's own sigma, the depth variance the tracking gathered at kp1 — value row 7)
            d.no_match_cov = true; d.model_match_cov_default = p->cov.model_match_cov_default;
            d.set1.flow_cov = nullptr;
            d.set1.depth_cov = fm.f1.sdd ? t.vals + 7 * (size_t)L * cap : nullptr;
        }
        MV_TRY(mv_obs_cov_launch(d, s));
        MV_TRY(obs_filter());
    }
    if (c.mapping) {   // the mapping decision of this frame (MACVO.py:303-307) needs the observation count on the host
        MV_HIP(hipMemcpyAsync(p->h_nvalid[k], b.n_valid, (size_t)L * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        MV_TRY(p->e_nvalid[k].record(s));
    }
    MV_TRY(p->e_backend[g].record(s));
    if (ti >= 0) MV_TRY(p->tv[5][ti].record(s));

    // ---- side stream: world-frame tables from the previous solve's pose (same stream: no event), then the LM solves of all
    // lanes in ONE launch (problem l = rows [l * cap, (l + 1) * cap), dead rows masked by `valid`); the optimised poses become
    // the next frame's priors (StaticMotionModel)
    hipStream_t ss = p->s_side;
    if (ss != s) MV_TRY(p->e_backend[g].wait(ss));   // (alt layout: backend + solve share one in-order stream)
    if (ti >= 0) MV_TRY(p->tv[6][ti].record(ss));
    mvPosedSolve sv = b.solve;
    sv.init_pose = p->pose[j.pose_from];
    sv.out_pose_f32 = p->pose[j.pose_to];
    if (p->solve_frame == MV_SOLVE_LOCAL) {
        // Local_TwoFrame_PGO: T_o2w = pose[frame_idx - 1] (Optimizer.py:119-121).  Nothing skipped: the previous keyframe's row, whose current pose is the
        // one the rows are rotated with.  Behind a skipped frame: that frame's row = the pose the previous keyframe was PUSHED with — its prior, i.e. the
        // slot finish g - 1 started from (two rotations back; solve g + 1 is the next to write it, behind this one on the same stream), or finish g - 1's
        // composed prior under the motion model.  (Before the first finish the previous keyframe is frame 0: prior == pose.)
        sv.ref_pose = !j.skipped || g == 0 ? p->pose[j.pose_from] : motion ? p->prior[(g - 1) % N_MOT] : p->pose[(j.pose_from + 2) % 3];
    }
    if (fused) {
        // ... and the pose-dependent half = ONE launch: the rotation into the world frame is the solve kernel's prologue, the caller's pose
        // sink its second output (the 28-byte device-to-device copy was a DMA node on the critical stream).  No e_posed: the world-frame
        // tables are consumed behind e_solved (mv_frame_pipe_map_append).
        sv.start_pose = prior;   // (motion model: LM starts from the prior)
        sv.pose_sink = j.pose_sink;
        sv.n_live = src.out_live ? nullptr : n_sel;
        sv.n_live_dev = src.out_live; sv.n_live_stride = 2;   // (given: the live-row count exists in device memory only, where the front launch published it)
        MV_TRY(mv_posed_solve(sv, ss));
    } else {
        MV_TRY(mv_pose_apply_lanes(sv.init_pose, sv.pos_Tc, sv.cov_Tc, L, n_sel, cap, sv.pos_Tw, sv.out_rot, sv.cov_Tw, ss));
        MV_TRY(p->e_posed[k].record(ss));
        sv.pos_Tc = nullptr;   // the plain solve (mv_pgo_solve; with ref_pose mv_pgo_solve_local): the world-frame tables and `valid` are inputs by now
        if (motion) sv.init_pose = prior;
        MV_TRY(mv_plain_solve(sv, ss));
        if (j.pose_sink)
            MV_HIP(hipMemcpyAsync(j.pose_sink, p->pose[j.pose_to], (size_t)L * 7 * sizeof(float), hipMemcpyDeviceToDevice, ss));
    }
    MV_TRY(p->e_solved[k].record(ss));   // (two adjacent records on one in-order stream, nothing between them: both fire behind the solve, in either order)
    MV_TRY(p->e_pgo.record(ss));
    if (ti >= 0) MV_TRY(p->tv[7][ti].record(ss));
    return MV_OK;
}

// permutations of a seeded job: torch.randperm of each lane's generator (see above)
void mv_kp_random_draw_host(std::mt19937& eng, int k, int H, int W, int mask, int64_t* out_uv);   // (kp_draw.hip)
static const int64_t* draw_perms(mvFramePipe* p, const FinishJob& j) {
    const int cap = cap_of(p->c);
    if (j.kp == KPJ_HOST) {   // a seeded RandomSelector frame: 2 * num_point words per lane, v rows first (same bits as the draw inside the front launch)
        for (int l = 0; l < p->lanes; ++l)
            mv_kp_random_draw_host(p->rng[(size_t)l], j.n_sel[l], p->c.H, p->c.W, p->c.kp_mask_width, p->perm_host.data() + 2 * (size_t)l * cap);
        return p->perm_host.data();
    }
    for (int l = 0; l < p->lanes; ++l)
        randperm_head(p->rng[(size_t)l], j.n_cand[l], p->c.num_point, p->perm_scratch, p->perm_host.data() + (size_t)l * cap);
    return p->perm_host.data();
}

// ------------------------------------------------------------------------------------------------ backend launch thread

static void launch_thread_main(mvFramePipe* p) {
    (void)hipSetDevice(p->device);
    long taken = 0;
    for (;;) {
        FinishJob j;
        // A job arrives once per frame period (~150 us) and sits on the frame's critical chain (selector count -> backend): waking a thread that
        // sleeps on a condition variable costs 30-60 us of it.  Spin on the submission counter for up to MV spin_us first (one period and a half),
        // sleep only when the stream has really gone quiet.
        if (p->k.spin_us > 0) {
            const double t_end = now_us() + p->k.spin_us;
            int it = 0;
            while (p->n_submitted.load(std::memory_order_acquire) == taken && !p->stop_flag.load(std::memory_order_relaxed)) {
#if defined(__x86_64__) || defined(__i386__)
                __builtin_ia32_pause();
#else
                std::this_thread::yield();
#endif
                if ((++it & 255) == 0 && now_us() > t_end) break;
            }
        }
        {
            std::unique_lock<std::mutex> lk(p->mu);
            p->cv_job.wait(lk, [&] { return p->stop || !p->jobs.empty(); });
            if (p->jobs.empty()) return;
            j = std::move(p->jobs.front());
            p->jobs.pop_front();
        }
        ++taken;
        const double t_pick = now_us();
        if (p->k.host_stats) { p->st_n += 1; p->st_submit_to_pick += t_pick - j.t_submit; p->st_count_to_submit += j.t_submit - j.t_count; }
        int rc = finish_issue(p, j, j.seeded ? draw_perms(p, j) : j.perm.data());
        if (p->k.host_stats) p->st_pick_to_issued += now_us() - t_pick;
        if (rc == MV_OK && j.has_sel) rc = issue_selector_segment(p, j.sel);
        {
            std::lock_guard<std::mutex> lk(p->mu);
            p->issued = j.g + 1;
            if (rc != MV_OK && p->async_rc == MV_OK) p->async_rc = rc;
        }
        p->cv_done.notify_all();
    }
}

// block until the launch thread has issued the first `n` finishes (n <= n_fin); returns the first asynchronous error
static int wait_issued(mvFramePipe* p, long n) {
    if (!p->async_backend) return MV_OK;
    std::unique_lock<std::mutex> lk(p->mu);
    p->cv_done.wait(lk, [&] { return p->issued >= n; });
    return p->async_rc;
}
static int flush_jobs(mvFramePipe* p) { return wait_issued(p, p->n_fin); }

static int submit_or_issue(mvFramePipe* p, FinishJob& j, const int64_t* perm_host) {
    if (!p->async_backend) {
        MV_TRY(finish_issue(p, j, j.seeded ? draw_perms(p, j) : perm_host));
        return j.has_sel ? issue_selector_segment(p, j.sel) : MV_OK;
    }
    if (!j.seeded && !j.device && (j.kp == KPJ_PERM || j.kp == KPJ_HOST) && j.n_max > 0) {
        const size_t cap = (size_t)cap_of(p->c) * (j.kp == KPJ_HOST ? 2 : 1);
        j.perm.assign(perm_host, perm_host + (size_t)p->lanes * cap);
    }
    int rc;
    j.t_submit = now_us();
    {
        std::lock_guard<std::mutex> lk(p->mu);
        rc = p->async_rc;
        p->jobs.push_back(std::move(j));
    }
    p->n_submitted.fetch_add(1, std::memory_order_release);
    p->cv_job.notify_one();
    return rc;
}

// What every finish does before it takes the frame off the pending list: the frame's selector segment is issued; `markers`: the chain events of this and
// the previous frame exist (lean chain: a finish whose front launch waits for the segment by event needs them); `map_count`: mapping mode —
// mv_frame_pipe_wait_tracked reads the mapping selector's count behind the frame's e_cand
static int finish_prologue(mvFramePipe* p, bool markers, bool map_count) {
    MV_TRY(selector_of_front_issued(p));
    const Pending& pd = p->pending.front();
    if (markers) {
        MV_TRY(ensure_chain_events(p, pd.f, pd.cand));
        if (pd.f > 0) MV_TRY(ensure_chain_events(p, pd.f - 1, -1));
    }
    if (map_count && p->c.mapping) MV_TRY(p->e_cand[pd.cand].sync());
    return MV_OK;
}
static FinishJob new_job(const mvFramePipe* p, int kp, bool seeded, bool device) {
    FinishJob j{};
    j.kp = kp; j.seeded = seeded; j.device = device;
    j.t_count = j.t_submit = p->k.host_stats ? now_us() : 0.0;
    return j;
}
// ... and last, for a frame whose every lane tracks `rows` rows (an upper bound where the live count exists on the device only: rows beyond are masked by `valid`)
static int finish_uniform(mvFramePipe* p, FinishJob& j, int rows, float* pose_sink) {
    int32_t nsel[MV_MAX_LANES];
    for (int l = 0; l < p->lanes; ++l) nsel[l] = rows;
    MV_TRY(finish_host(p, nsel, pose_sink, j));
    return submit_or_issue(p, j, nullptr);
}

// A frame of a RandomSelector / GridSelector pipe: every lane tracks frame_rows() rows, nothing to wait for.  kp = KPJ_HOST: drawn on the host by whoever issues
// the job (seeded), KPJ_RANDOM: drawn inside the front launch (device-driven), KPJ_GRID: computed there.
static int finish_rows(mvFramePipe* p, int kp, float* pose_sink, int32_t* n_cand_out, int32_t* n_sel_out) {
    // (the device-driven frame's front launch follows its segment in stream order or by a pending barrier: no markers)
    MV_TRY(finish_prologue(p, kp != KPJ_RANDOM || p->c.mapping, true));
    FinishJob j = new_job(p, kp, kp == KPJ_HOST, kp == KPJ_RANDOM);
    for (int l = 0; l < p->lanes; ++l) {
        if (n_cand_out) n_cand_out[l] = frame_rows(p->c);
        if (n_sel_out) n_sel_out[l] = frame_rows(p->c);
    }
    return finish_uniform(p, j, frame_rows(p->c), pose_sink);
}

// wait_candidates + permutations (per-lane generators of mv_frame_pipe_seed_lanes) + finish in one host call
extern "C" int mv_frame_pipe_finish_seeded(mvFramePipe* p, float* pose_sink, int32_t* n_cand_out, int32_t* n_sel_out) {
    MV_CHECK_ARG(p && !p->pending.empty());
    if (p->c.selector_mode == MV_KP_GRID) return finish_rows(p, KPJ_GRID, pose_sink, n_cand_out, n_sel_out);
    MV_CHECK_ARG((int)p->rng.size() == p->lanes && p->c.selector_mode != MV_KP_EXPLICIT);
    MV_CHECK_ARG(!p->dev_draw);   // (its generators live on the device: mv_frame_pipe_finish_device)
    if (p->c.selector_mode == MV_KP_RANDOM) return finish_rows(p, KPJ_HOST, pose_sink, n_cand_out, n_sel_out);
    MV_TRY(finish_prologue(p, false, false));
    const Pending& pd = p->pending.front();
    const double t_w0 = p->k.host_stats ? now_us() : 0.0;
    MV_TRY(p->e_cand[pd.cand].sync());
    FinishJob j = new_job(p, KPJ_PERM, true, false);
    if (p->k.host_stats) p->st_wait += j.t_count - t_w0;
    int32_t nsel[MV_MAX_LANES];
    for (int l = 0; l < p->lanes; ++l) {
        const int64_t n = p->h_count[pd.cand][4 * l];
        const int k = (int)(n < p->c.num_point ? n : p->c.num_point);
        j.n_cand[l] = n;
        nsel[l] = k;
        if (n_cand_out) n_cand_out[l] = (int32_t)n;
        if (n_sel_out) n_sel_out[l] = k;
    }
    MV_TRY(finish_host(p, nsel, pose_sink, j));
    return submit_or_issue(p, j, nullptr);
}

// The device-driven finish (round 6): nothing to wait for and nothing to draw — the frame's backend + solve are queued behind its selector segment by event, the
// permutation head is drawn inside the front launch.  The host learns the counts only if it asks (mv_frame_pipe_finished_counts).
extern "C" int mv_frame_pipe_finish_device(mvFramePipe* p, float* pose_sink) {
    MV_CHECK_ARG(p && !p->pending.empty());
    if (p->c.selector_mode == MV_KP_GRID) return finish_rows(p, KPJ_GRID, pose_sink, nullptr, nullptr);
    MV_CHECK_ARG(p->dev_draw);
    if (p->c.selector_mode == MV_KP_RANDOM) return finish_rows(p, KPJ_RANDOM, pose_sink, nullptr, nullptr);
    MV_TRY(finish_prologue(p, false, false));
    FinishJob j = new_job(p, KPJ_PERM, false, true);
    const int rc = finish_uniform(p, j, p->c.num_point, pose_sink);
    if (p->k.host_stats) { p->st_fin += now_us() - j.t_count; p->st_calls += 1; }
    return rc;
}

// candidate / selected-keypoint counts of the `age`-th newest FINISHED frame (age 0 or 1), read back from the frame's backend slot: blocks until that
// frame's front launch has run.  Off the hot path (result views, tests).
extern "C" int mv_frame_pipe_finished_counts(mvFramePipe* p, int age, int32_t* n_cand, int32_t* n_sel) {
    MV_CHECK_ARG(p && age >= 0 && age <= 1 && p->n_fin - 1 - age >= 0);
    const bool rows_dev = p->be[(p->n_fin - 1 - age) & 1].rows_dev;   // device rows with device counts: published by the front launch, on any pipe
    MV_CHECK_ARG(p->dev_draw || rows_dev);
    MV_TRY(flush_jobs(p));
    if (kp_new_mode(p->c.selector_mode) && !rows_dev) {   // (no candidate list: the row count is the configuration's)
        for (int l = 0; l < p->lanes; ++l) {
            if (n_sel) n_sel[l] = p->be[(p->n_fin - 1 - age) & 1].n_sel[l];
            if (n_cand) n_cand[l] = frame_rows(p->c);
        }
        return MV_OK;
    }
    const long g = p->n_fin - 1 - age;
    MV_TRY(p->e_backend[g].sync());
    std::vector<int32_t> h(2 * (size_t)p->lanes);
    MV_HIP(hipMemcpy(h.data(), p->be[g & 1].live_dev, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int l = 0; l < p->lanes; ++l) {
        if (n_sel) n_sel[l] = h[2 * l];
        if (n_cand) n_cand[l] = h[2 * l + 1];
    }
    return MV_OK;
}

// Bound how far the host runs ahead of the GPU in a device-driven stream: blocks until the front launch of the finish `lag` finishes back (0 = the newest) has run.
extern "C" int mv_frame_pipe_wait_finished(mvFramePipe* p, int lag) {
    MV_CHECK_ARG(p && lag >= 0 && lag < N_BEV - 1);
    const long g = p->n_fin - 1 - lag;
    if (g < 0) return MV_OK;
    MV_TRY(wait_issued(p, g + 1));
    // (polling with hipEventQuery before blocking was measured: no difference — the wait is 10-40 us per frame and two frames back, profiles/r06_chain_gaps.log)
    return p->e_backend[g].sync();
}

// Host-only probe of the driver's permutation generator (no GPU, no pipe): `calls` successive `torch.randperm(n[i])[:k]` of one
// generator seeded with `seed`, written to out[i * k .. i * k + min(k, n[i])) — what mv_frame_pipe_finish_seeded draws for one lane
// frame after frame.  Lets the CPU test suite pin the generator against torch itself.
extern "C" int mv_randperm_heads(uint64_t seed, const int64_t* n, int calls, int k, int64_t* out) {
    MV_CHECK_ARG(n && out && calls >= 0 && k >= 0);
    std::mt19937 eng((uint32_t)(seed & 0xffffffffull));
    std::vector<int32_t> scratch;
    for (int i = 0; i < calls; ++i) {
        MV_CHECK_ARG(n[i] >= 0 && n[i] < ((int64_t)1 << 31));
        randperm_head(eng, n[i], k, scratch, out + (size_t)i * k);
    }
    return MV_OK;
}

extern "C" int mv_frame_pipe_finish(mvFramePipe* p, const int64_t* perm_host, const int32_t* n_sel, float* pose_sink) {
    MV_CHECK_ARG(p && n_sel && !p->pending.empty() && !kp_new_mode(p->c.selector_mode));   // (a permutation needs a candidate list)
    for (int l = 0; l < p->lanes; ++l)
        MV_CHECK_ARG(n_sel[l] >= 0 && n_sel[l] <= p->c.num_point && (n_sel[l] == 0 || perm_host));
    MV_TRY(finish_prologue(p, true, false));       // (lean chain: a host-permuted finish waits for the markers)
    FinishJob j = new_job(p, KPJ_PERM, false, false);
    MV_TRY(finish_host(p, n_sel, pose_sink, j));
    return submit_or_issue(p, j, perm_host);
}

// Caller-supplied keypoints: any selector's (u, v) rows instead of a permutation over the driver's candidate list — valid for every selector_mode.
extern "C" int mv_frame_pipe_table_rows(const mvFramePipeConfig* cfg) { return check_config(cfg) == MV_OK ? table_rows(*cfg) : 0; }

extern "C" int mv_frame_pipe_finish_keypoints(mvFramePipe* p, const int64_t* kp_uv_host, const int32_t* n_sel, float* pose_sink) {
    MV_CHECK_ARG(p && n_sel && !p->pending.empty());
    const mvFramePipeConfig& c = p->c;
    const int cap = cap_of(c);
    const int64_t hw = c.cov_model == MV_COV_NONE ? 0 : c.cov_kernel_size / 2;   // the covariance patch must stay inside the image
    for (int l = 0; l < p->lanes; ++l) {
        MV_CHECK_ARG(n_sel[l] >= 0 && n_sel[l] <= table_rows(c) && (n_sel[l] == 0 || kp_uv_host));
        for (int i = 0; i < n_sel[l]; ++i) {
            const int64_t u = kp_uv_host[2 * ((size_t)l * cap + i)], v = kp_uv_host[2 * ((size_t)l * cap + i) + 1];
            MV_CHECK_ARG(u >= hw && u < c.W - hw && v >= hw && v < c.H - hw);
        }
    }
    MV_TRY(finish_prologue(p, true, true));
    FinishJob j = new_job(p, KPJ_HOST, false, false);
    MV_TRY(finish_host(p, n_sel, pose_sink, j));
    return submit_or_issue(p, j, kp_uv_host);
}

extern "C" int mv_frame_pipe_finish_keypoints_dev(mvFramePipe* p, const int64_t* kp_uv_dev, const int32_t* n_sel_dev, mvStream_t stream, float* pose_sink) {
    MV_CHECK_ARG(p && kp_uv_dev && n_sel_dev && !p->pending.empty() && p->k.fuse_backend && !p->c.mapping && table_rows(p->c) >= 1);
    MV_TRY(finish_prologue(p, true, true));
    FinishJob j = new_job(p, KPJ_DEV, false, false);
    j.kp_dev = kp_uv_dev;
    j.nsel_dev = n_sel_dev;
    MV_TRY(p->e_kpin[p->n_fin].record((hipStream_t)stream));   // recorded before the job is queued
    return finish_uniform(p, j, table_rows(p->c), pose_sink);
}

// Register the newest FINISHED frame in device-resident maps (call right after a finish), the one protocol behind both entry points: the frame's tables are
// handed to `launch` where they lie (no copies), on the backend stream behind the observation filter; `set_pose` then writes the optimised pose over the
// frame's prior on the solve stream (write_graph_data, Optimizer.py:104-108).  `f`: mvMapFrame or mvMapFrameLanes — the fields they share are filled here.
template <class Frame, class Launch, class SetPose>
static int map_append_finished(mvFramePipe* p, Frame& f, int prev_frame, const float* K_dev, const float* T_BS_dev, float baseline, Launch launch,
                               SetPose set_pose) {
    MV_TRY(flush_jobs(p));
    const mvFramePipeConfig& c = p->c;
    const long g = p->n_fin - 1;
    const int k = (int)(g & 1);
    const Backend& b = p->be[k];
    f.prev_frame = prev_frame;
    f.min_num_point = c.min_num_point;
    f.valid = b.valid;
    f.kp0 = b.kp0f; f.kp1 = b.kp1; f.vals = b.vals; f.sigma0 = b.sigma0; f.sigma1 = b.sigma1;
    f.cov0 = b.cov0; f.cov1 = b.cov1; f.pos_Tw = b.pos_Tw; f.cov0_world = b.cov0w;
    f.K = K_dev; f.T_BS = T_BS_dev;
    f.prior_pose = c.motion_model == MV_MOTION_TARTAN ? p->prior[g % N_MOT] : p->pose[p->prior_slot];   // push_keyframe(frame1, est_pose) (MACVO.py:282)
    f.baseline = baseline;
    MV_TRY((p->k.fuse_backend ? p->e_solved[k] : p->e_posed[k]).wait(p->s_back));   // pos_Tw / cov0_world come from the side stream
    MV_TRY(launch(b));
    MV_TRY(p->e_map.record(p->s_back));
    // The backend tables must outlive the append.  A front launch that runs on this stream is behind it in order; one on a decoder-side stream — the default of
    // the one-lane device-driven pipe — waits for e_mapl[k] before finish g + 2 rewrites the slot (finish_issue).  No packet for a pipe that has no such launch.
    if (p->k.front_on_decoder) MV_TRY(p->e_mapl[k].record(p->s_back));
    // the optimised pose goes in after the append wrote the prior
    MV_TRY(p->e_map.wait(p->s_side));
    MV_TRY(set_pose(p->pose[p->pose_cur]));
    return p->e_pgo.record(p->s_side);
}

// The one-lane form: a host descriptor of the one map, and the frame's colours.
extern "C" int mv_frame_pipe_map_append(mvFramePipe* p, const mvMapStores* stores, int frame_idx, int prev_frame,
                                        const float* K_dev, const float* T_BS_dev, float baseline, int64_t time_ns,
                                        const uint8_t* color_dev) {
    MV_CHECK_ARG(p && stores && K_dev && T_BS_dev && p->lanes == 1 && p->n_fin > 0 && frame_idx >= 0);
    mvMapFrame f{};
    f.table_stride = cap_of(p->c);
    f.color = color_dev;
    f.time_ns = time_ns;
    return map_append_finished(
        p, f, prev_frame, K_dev, T_BS_dev, baseline,
        [&](const Backend& b) {
            f.n_rows = b.n_sel[0];
            return mv_map_append(&f, stores, p->s_back);
        },
        [&](const float* pose) -> int {
            MV_HIP(hipMemcpyAsync(stores->pose + 7 * (size_t)frame_idx, pose, 7 * sizeof(float), hipMemcpyDeviceToDevice, p->s_side));
            return MV_OK;
        });
}

// Any lane count, every lane into its own map (a device array of descriptors): one launch for all lanes (mv_map_append_lanes), the optimised poses behind it
// by one launch on the solve stream (each lane's destination is another allocation).
extern "C" int mv_frame_pipe_map_append_lanes(mvFramePipe* p, const mvMapStores* stores_dev, int frame_idx, int prev_frame, const float* K_dev,
                                              const float* T_BS_dev, float baseline, const int64_t* time_ns) {
    MV_CHECK_ARG(p && stores_dev && K_dev && T_BS_dev && time_ns && p->n_fin > 0 && frame_idx >= 0);
    mvMapFrameLanes f{};
    f.lanes = p->lanes;
    f.cap = cap_of(p->c);
    f.time_ns = time_ns;
    return map_append_finished(
        p, f, prev_frame, K_dev, T_BS_dev, baseline,
        [&](const Backend& b) {
            f.n_rows = b.n_sel;   // (device-driven frames: the upper bound, `valid` compacts)
            return mv_map_append_lanes(&f, stores_dev, p->s_back);
        },
        [&](const float* poses) { return mv_map_set_pose_lanes(stores_dev, p->lanes, frame_idx, poses, p->s_side); });
}

// ------------------------------------------------------------------------------------------------ keyframe policy, local solve
extern "C" int mv_frame_pipe_set_solve_frame(mvFramePipe* p, int solve_frame) {
    MV_CHECK_ARG(p && (solve_frame == MV_SOLVE_WORLD || solve_frame == MV_SOLVE_LOCAL) && p->n_enq == 0);
    p->solve_frame = solve_frame;
    return MV_OK;
}

extern "C" int mv_frame_pipe_skip(mvFramePipe* p) {
    MV_CHECK_ARG(p && p->n_enq > 0);   // (between the finishes of the keyframes around it: the next finish consumes the note)
    p->skipped = true;
    return MV_OK;
}

// The skipped frame's row: push_keyframe(frame1, pose row of the previous keyframe, need_interp=True) (MACVO.py:177-179).  That row still holds the prior the
// keyframe was pushed with, so `launch` copies the pose from the prior slot — on the backend stream, in order with the pipe's own appends.  (It reads no
// backend slot: nothing for a front launch to wait for.)
template <class Launch>
static int map_skip_row(mvFramePipe* p, Launch launch) {
    MV_TRY(flush_jobs(p));
    const long g = p->n_fin - 1;   // the previous keyframe's finish (-1: frame 0, pushed at the pose set by mv_frame_pipe_set_pose)
    const float* prior = g < 0 ? p->pose[p->pose_cur] : p->c.motion_model == MV_MOTION_TARTAN ? p->prior[g % N_MOT] : p->pose[p->prior_slot];
    // The prior slot is written on the side stream in FRONT of finish g's solve (the slot that solve started from, or the prior composed for it).  The event
    // map_append_finished made this stream wait for when it registered finish g lies behind that write, so stream order already covers it and the wait
    // below adds nothing to the stream; it only keeps a caller that registers no keyframes correct.  (Not e_pgo: that is re-recorded behind the append's pose
    // copy and would put the backend stream behind work it does not depend on.)
    if (g >= 0) MV_TRY((p->k.fuse_backend ? p->e_solved[g & 1] : p->e_posed[g & 1]).wait(p->s_back));
    MV_TRY(launch(prior));
    return p->e_map.record(p->s_back);
}

extern "C" int mv_frame_pipe_map_skip(mvFramePipe* p, const mvMapStores* stores, int frame_idx, const float* K_dev, const float* T_BS_dev, float baseline,
                                      int64_t time_ns) {
    MV_CHECK_ARG(p && stores && K_dev && T_BS_dev && p->lanes == 1 && p->n_enq > 0 && frame_idx >= 1 && frame_idx < stores->cap_frames);
    return map_skip_row(p, [&](const float* prior) { return mv_map_append_skipped(stores, K_dev, T_BS_dev, prior, baseline, time_ns, p->s_back); });
}

extern "C" int mv_frame_pipe_map_skip_lanes(mvFramePipe* p, const mvMapStores* stores_dev, int frame_idx, const float* K_dev, const float* T_BS_dev,
                                            float baseline, const int64_t* time_ns) {
    MV_CHECK_ARG(p && stores_dev && K_dev && T_BS_dev && time_ns && p->n_enq > 0 && frame_idx >= 1);
    return map_skip_row(
        p, [&](const float* prior) { return mv_map_append_skipped_lanes(stores_dev, p->lanes, K_dev, T_BS_dev, prior, baseline, time_ns, p->s_back); });
}

// ------------------------------------------------------------------------------------------------ dense-mapping tail
extern "C" int mv_frame_pipe_wait_tracked(mvFramePipe* p, int32_t* n_valid, int32_t* n_cand_map) {
    MV_CHECK_ARG(p && n_valid && p->c.mapping && p->n_fin > 0);
    MV_TRY(flush_jobs(p));
    const int k = (int)((p->n_fin - 1) & 1);
    if (!p->e_nvalid[k].recorded()) {   // a frame without keypoints: nothing was tracked
        *n_valid = 0;
        if (n_cand_map) *n_cand_map = 0;
        return MV_OK;
    }
    MV_TRY(p->e_nvalid[k].sync());
    *n_valid = p->h_nvalid[k][0];
    if (n_cand_map) *n_cand_map = p->h_count_m[p->last_cand][0];   // (its copy preceded e_cand, which the host waited for before finish)
    return MV_OK;
}

extern "C" int mv_frame_pipe_map_points(mvFramePipe* p, const int64_t* perm_host, int n_sel, const float* image_dev,
                                        const mvMapStores* stores) {
    MV_CHECK_ARG(p && p->c.mapping && p->n_fin > 0 && n_sel >= 0 && n_sel <= p->c.map_num_point && (n_sel == 0 || perm_host));
    MV_TRY(flush_jobs(p));
    const mvFramePipeConfig& c = p->c;
    hipStream_t s = p->s_back;
    const Maps& m0 = p->maps[p->last_maps_prev];
    MV_TRY(p->e_maptail.sync());               // pinned permutation + map buffers of the previous tail (long done)
    MV_TRY(p->e_release.wait_if_pending(s));   // ... and consumers of its result views
    if (n_sel > 0) {
        memcpy(p->h_perm_m, perm_host, (size_t)n_sel * sizeof(int64_t));
        MV_HIP(hipMemcpyAsync(p->mp_perm, p->h_perm_m, (size_t)n_sel * sizeof(int64_t), hipMemcpyHostToDevice, s));
        MV_TRY(mv_kp_gather(p->cand_m[p->last_cand], p->mp_perm, n_sel, c.W, p->mp_uv, s));
        // prev_pose.Act (MACVO.py:334): the pose the frame started from = the previous frame's optimised pose
        MV_TRY(p->e_pgo.wait_if_pending(s));   // (the solve that produced it; the newest solve is recorded later on `side`: also fine)
        MV_TRY(mv_map_points(p->mp_uv, n_sel, m0.depth, m0.depth_cov, image_dev, c.H, c.W, c.fx, c.fy, c.cx, c.cy,
                             p->pose[p->prior_slot], c.match_cov_default, p->mp_uvf, p->mp_d, p->mp_sdd, p->mp_sigma, p->mp_Tc, p->mp_Tw,
                             image_dev ? p->mp_color : nullptr, s));
        MV_TRY(mv_obs_cov(c.cov_model, c.cov_modifiers, m0.depth, m0.depth_cov, p->mp_uvf, p->mp_sigma, p->mp_sdd, nullptr, &p->cov.cp, n_sel, p->mp_cov,
                          nullptr, nullptr, s));   // the same ObsCovModel (MACVO.py:324)
    }
    if (stores) {   // map_points.push + frame2map.add (also for n_sel == 0: the reference adds the empty range), behind the frame's registration
        MV_TRY(mv_map_append_points(stores, n_sel, p->mp_Tw, p->mp_cov, image_dev ? p->mp_color : nullptr, s));
    }
    p->mp_rows = n_sel;
    MV_TRY(p->e_maptail.record(s));
    return p->e_backend[p->n_fin - 1].record(s);   // the previous frame's maps stay in use until here (the next enqueue waits for this event)
}

extern "C" int mv_frame_pipe_release(mvFramePipe* p, mvStream_t stream) {
    MV_CHECK_ARG(p);
    return p->e_release.record((hipStream_t)stream);
}

extern "C" int mv_frame_pipe_sync(mvFramePipe* p, mvStream_t stream, int block_host) {
    MV_CHECK_ARG(p);
    MV_TRY(flush_deferred(p));
    MV_TRY(flush_jobs(p));   // everything finished so far has been issued
    if (block_host == SYNC_NEWEST)   // results of the newest FINISHED frame only: its solve (which ran behind its backend kernels)
        return p->e_pgo.wait((hipStream_t)stream);
    if (block_host != SYNC_STREAM) return sync_streams(p, ST_ALL);   // SYNC_HOST (and, as ever, any other value)
    // make `stream` wait for everything enqueued so far (every stream is visited even after a failure)
    Ev e;
    MV_TRY(e.create());
    int rc = MV_OK;
    const auto join = [&](hipStream_t q) {
        if (e.record(q) != MV_OK || e.wait((hipStream_t)stream) != MV_OK) rc = MV_ERR_LAUNCH;
        return hipSuccess;
    };
    (void)each_stream(p, ST_ALL & ~ST_DECODER, join);
    (void)each_stream(p, ST_DECODER, join);
    return rc;
}

extern "C" int mv_frame_pipe_time_volume(mvFramePipe* p, int max_launches) {
    MV_CHECK_ARG(p && max_launches >= 0 && max_launches <= (1 << 20));
    MV_TRY(flush_jobs(p));   // finish_issue on the launch thread records into tv3..tv7 (which may reallocate below)
    for (std::vector<Ev>& v : p->tv)
        while ((int)v.size() < max_launches) {
            Ev e;
            MV_TRY(e.create(hipEventDefault));   // (timing enabled)
            v.push_back(std::move(e));
        }
    p->n_timed = 0;
    p->timed_cap = max_launches;
    return MV_OK;
}

extern "C" int mv_frame_pipe_time_detail(mvFramePipe* p, int on) {
    MV_CHECK_ARG(p);
    MV_TRY(flush_jobs(p));
    p->time_detail = on ? 1 : 0;
    return MV_OK;
}

// The one reader of the timing events: for each timed frame i and each column c of `cols` (indices into mvFramePipe::tv), ms[i * |cols| + c] = time from the
// first timed GEMM start — `per_frame`: from frame i's own GEMM start — to that event.  Blocks until the streams `sync_a`, then `sync_b`, have drained.
// `detail`: columns that exist only under mv_frame_pipe_time_detail (no frames without it); a pair that cannot be read is -1 there, an error otherwise.
static int read_times(mvFramePipe* p, float* ms, int cap, int* n, std::initializer_list<int> cols, bool per_frame, bool detail, unsigned sync_a,
                      unsigned sync_b) {
    MV_CHECK_ARG(p && n && cap >= 0 && (cap == 0 || ms));
    MV_TRY(flush_jobs(p));   // (the launch thread records tv[3] .. tv[7])
    if (detail && !p->time_detail) { *n = 0; return MV_OK; }
    MV_TRY(sync_streams(p, sync_a));
    MV_TRY(sync_streams(p, sync_b));
    const int m = p->n_timed < cap ? p->n_timed : cap;
    float* out = ms;
    for (int i = 0; i < m; ++i)
        for (const int c : cols)
            if (hipEventElapsedTime(out++, p->tv[0][per_frame ? i : 0].e, p->tv[c][i].e) != hipSuccess) {
                if (!detail) return MV_ERR_LAUNCH;
                out[-1] = -1.f;
            }
    *n = m;
    return MV_OK;
}

// how long each timed GEMM took ...
extern "C" int mv_frame_pipe_volume_times(mvFramePipe* p, float* ms, int cap, int* n) { return read_times(p, ms, cap, n, {1}, true, false, ST_VOL, 0); }

// ... and when each STARTED, ms since the first one (the steady-state period of the very pass whose wall time is the bench line's `value`: only the event
// pairs around the GEMM are recorded in that pass)
extern "C" int mv_frame_pipe_volume_starts(mvFramePipe* p, float* ms, int cap, int* n) { return read_times(p, ms, cap, n, {0}, false, false, ST_VOL, 0); }

// timeline of the timed frames: for frame i, ms[4*i + {0,1,2,3}] = GEMM start, GEMM end, last lookup done, selector done, all relative to the first timed
// GEMM start (blocks until everything enqueued so far has finished)
extern "C" int mv_frame_pipe_timeline(mvFramePipe* p, float* ms, int cap_frames, int* n) {
    return read_times(p, ms, cap_frames, n, {0, 1, 2, 3}, false, true, ST_VOL | ST_DECODER | ST_BACK | ST_SEL, 0);
}

// ... and the backend side of the same frames: ms[4*i + {0,1,2,3}] = backend start, backend end (backend stream), pose_apply start, solve end (solve
// stream); -1 where a frame was not finished (or had no keypoints).  (Device-driven frames run the front launch on the decoder side.)
extern "C" int mv_frame_pipe_timeline_backend(mvFramePipe* p, float* ms, int cap_frames, int* n) {
    return read_times(p, ms, cap_frames, n, {4, 5, 6, 7}, false, true, ST_BACK | ST_SIDE, ST_DECODER);
}

extern "C" int mv_frame_pipe_buffer(mvFramePipe* p, int which, int age, void** ptr, size_t* count) {
    MV_CHECK_ARG(p && ptr && count && age >= 0);
    const mvFramePipeConfig& c = p->c;
    *ptr = nullptr;
    *count = 0;
    // frontend-side buffers: age 0 = the newest enqueued frame; backend-side: age 0 = the newest finished frame
    const long f = p->n_enq - 1 - age, g = p->n_fin - 1 - age;
    auto front = [&](int depth) { return f >= 0 && age < depth; };
    auto back = [&]() { return g >= 0 && age < 2; };
    const Backend* b = back() ? &p->be[g & 1] : nullptr;
    const Maps* m = front(N_MAPS) ? &p->maps[f % N_MAPS] : nullptr;
    const bool motion = c.motion_model == MV_MOTION_TARTAN, tail = c.mapping && age == 0;
    void* at = nullptr;   // where the buffer of that age is (null: no such age, or no such buffer in this pipe); its count is what `carve` noted
    switch (which) {
        // age limit: with a GEMM issued ahead (n_vol > n_enq) the buffer of frame f - 1 is being rewritten
        case MV_FB_VOLUME: if (front(p->n_vol > p->n_enq ? 1 : 2)) at = p->vol[f % p->k.n_volbuf]; break;
        case MV_FB_TOKENS: if (front(1) && c.iters > 0) at = p->tok[2 * (f % p->k.n_lk) + ((c.iters - 1) & 1)]; break;
        case MV_FB_DISPARITY: if (m) at = m->disparity; break;
        case MV_FB_DISPARITY_COV: if (m) at = m->disparity_cov; break;
        case MV_FB_DEPTH: if (m) at = m->depth; break;
        case MV_FB_DEPTH_COV: if (m) at = m->depth_cov; break;
        case MV_FB_MATCH_FLOW: if (m) at = m->match_flow; break;
        case MV_FB_MATCH_COV: if (m) at = m->match_cov; break;
        case MV_FB_CAND: if (front(N_CAND)) at = p->cand[f % N_CAND]; break;
        case MV_FB_COUNT: if (front(N_CAND)) at = p->count[f % N_CAND]; break;
        case MV_FB_STATS: if (front(N_CAND)) at = p->stats[f % N_CAND]; break;
        case MV_FB_KP0: if (b) at = b->kp0; break;
        case MV_FB_KP0F: if (b) at = b->kp0f; break;
        case MV_FB_KP1: if (b) at = b->kp1; break;
        case MV_FB_INBOUND: if (b) at = b->inbound; break;
        case MV_FB_VALS: if (b) at = b->vals; break;
        case MV_FB_SIGMA0: if (b) at = b->sigma0; break;
        case MV_FB_SIGMA1: if (b) at = b->sigma1; break;
        case MV_FB_POS_TC: if (b) at = b->pos_Tc; break;
        case MV_FB_POS_TW: if (b) at = b->pos_Tw; break;
        case MV_FB_ROT: if (b) at = b->rot; break;
        case MV_FB_COV0: if (b) at = b->cov0; break;
        case MV_FB_COV0W: if (b) at = b->cov0w; break;
        case MV_FB_COV1: if (b) at = b->cov1; break;
        case MV_FB_VALID: if (b) at = b->valid; break;
        case MV_FB_NVALID: if (b) at = b->n_valid; break;
        case MV_FB_POSE64: if (b) at = b->pose64; break;
        case MV_FB_INFO: if (b) at = b->info; break;
        case MV_FB_POSE: if (age <= 1) at = p->pose[(p->pose_cur + 3 - age) % 3]; break;
        case MV_FB_PERM: if (b) at = b->perm; break;
        case MV_FB_LIVE: if (b && p->dev_draw) at = b->live_dev; break;
        case MV_FB_MOTION_IN: if (motion && m) at = p->motion_in[f % N_MAPS]; break;
        case MV_FB_PRIOR: if (motion && back()) at = p->prior[g % N_MOT]; break;
        case MV_FB_MAP_UV: if (tail) at = p->mp_uvf; break;
        case MV_FB_MAP_D: if (tail) at = p->mp_d; break;
        case MV_FB_MAP_SDD: if (tail) at = p->mp_sdd; break;
        case MV_FB_MAP_TC: if (tail) at = p->mp_Tc; break;
        case MV_FB_MAP_TW: if (tail) at = p->mp_Tw; break;
        case MV_FB_MAP_COV: if (tail) at = p->mp_cov; break;
        case MV_FB_MAP_COLOR: if (tail) at = p->mp_color; break;
        default: break;
    }
    if (!at) return MV_ERR_INVALID_ARG;
    *ptr = at;
    *count = p->fb_count[which] * (which >= MV_FB_MAP_UV && which <= MV_FB_MAP_COLOR ? (size_t)p->mp_rows : 1);   // (the tail's buffers: per row)
    return MV_OK;
}
