// TEST INFRASTRUCTURE: the frame driver's schedule as text, on the CPU.
//
// Linked with the library's own objects and fake_hip.cpp (a HIP runtime that logs instead of executing), this program creates a frame pipe over a host-memory
// arena, runs a named scenario through the public C API of macvo_hip.h and prints every stream, launch, event edge and copy the driver issued, followed by
// mv_frame_pipe_arena_bytes and mv_frame_pipe_buffer of every MV_FB_* id.  tests/test_frame_pipe_trace_host.py compares the output with
// tests/golden/frame_pipe_trace_*.txt.
//
//   pipe_trace --list            "group name" of every scenario
//   pipe_trace NAME [--async]    the trace of one scenario (--async: with the backend launch thread; the interleaving is then timing-dependent)
//
// The arena is filled with the int32 value 400 before `create`, so every count the host reads back is 400.
#include "macvo_hip.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

extern "C" void fake_hip_arena(const void* base, size_t bytes);
extern "C" void fake_hip_event_query_ready(int ready);
extern "C" void fake_hip_note(const char* text);
extern "C" void fake_hip_dump(FILE* f);

namespace {

enum Pattern {
    SEEDS,     // integer seeds, as NativeHotPath.run: device-driven where the pipe allows it (finish_device, wait_finished), finish_seeded otherwise
    PERM,      // host permutations: wait_candidates + finish
    KP_HOST,   // finish_keypoints
    KP_DEV     // finish_keypoints_dev
};
enum MapMode { NO_MAP, MAP_ONE, MAP_LANES };
enum Timing { NO_TIMING, TIMING_DETAIL, TIMING_PAIRS };

struct Knob { const char* name; const char* value; };

struct Scenario {
    std::string group, name;
    // configuration (the rest is make_config's)
    int H = 64, W = 96, C = 256, lanes = 1;   // 64 x 96 with C = 256: the smallest shape the packed f16x2 GEMM covers
    int feat_dtype = MV_F32, layout = MV_LAYOUT_CHW, volume_split = MV_PACK_F16X2;
    int selector = MV_KP_NODEPTH, num_point = 50, mapping = 0, motion = MV_MOTION_STATIC, nocov = 0, graph = MV_GRAPH_REPROJ;
    std::vector<Knob> env;
    // call pattern
    Pattern pattern = SEEDS;
    int frames = 5;
    int depth = 0;              // tracked frames in flight of a host-driven pattern (0: mv_frame_pipe_default_depth)
    bool volume_ahead = true;   // enqueue_volume one frame ahead
    bool flow8 = false;         // 1/8-resolution fields + masks instead of upsampled flow
    MapMode map = NO_MAP;
    int skip_at = -1;           // this frame is skipped (mv_frame_pipe_skip + map_skip) under MV_SOLVE_LOCAL
    Timing timing = NO_TIMING;
    bool query_ready = false;   // hipEventQuery answers "ready"
};

std::vector<Scenario> scenarios() {
    std::vector<Scenario> all;
    const auto add = [&](Scenario s, const char* group, const std::string& name) {
        s.group = group; s.name = name;
        all.push_back(s);
        return s;
    };
    // ---- one lane (the round-5 layout) and three lanes (the classic batched layout)
    Scenario s;
    s.frames = 6;   // (four volume buffers, the GEMM one frame ahead: frame 5's is the first to wait for a tracked frame's release)
    const Scenario one_dd = add(s, "core", "one_device");
    Scenario base = one_dd;
    base.frames = 5;
    s = base; s.pattern = PERM;
    const Scenario one_perm = add(s, "core", "one_perm");
    s = base; s.env = {{"MV_PIPE_DEVICE_DRAW", "0"}};
    add(s, "core", "one_seeded");
    s = base; s.lanes = 3;
    const Scenario three_dd = add(s, "core", "three_device");
    s.env = {{"MV_PIPE_DEVICE_DRAW", "0"}};
    add(s, "core", "three_seeded");
    s = one_perm; s.lanes = 3;
    add(s, "core", "three_perm");
    s = one_perm; s.num_point = 300;   // (more than 256 rows: the permutation travels by copy, not in the kernel arguments)
    add(s, "core", "one_perm_300");
    s = base; s.num_point = 600;       // (more than the device draw covers: host-drawn)
    add(s, "core", "one_seeds_600");
    s = base; s.query_ready = true;
    add(s, "core", "one_device_query_ready");
    s = one_perm; s.query_ready = true;
    add(s, "core", "one_perm_query_ready");
    s = one_perm; s.mapping = 1;
    add(s, "core", "mapping");
    s.map = MAP_ONE;
    add(s, "core", "mapping_map");
    s = base; s.motion = MV_MOTION_TARTAN; s.H = 112; s.W = 160;
    add(s, "core", "motion_device");
    s.pattern = PERM;
    add(s, "core", "motion_perm");
    // ---- inputs
    s = base; s.flow8 = true;
    add(s, "inputs", "flow8_aligned_device");
    s.pattern = PERM;
    add(s, "inputs", "flow8_aligned_perm");
    s = base; s.flow8 = true; s.H = 60; s.W = 92;
    add(s, "inputs", "flow8_unpadded_device");
    s = base; s.H = 60; s.W = 92;
    add(s, "inputs", "unpadded_device");
    s = base; s.selector = MV_KP_RANDOM; s.nocov = MV_NOCOV_DEPTH;
    add(s, "inputs", "nocov_depth_random");
    s.selector = MV_KP_NODEPTH;
    add(s, "inputs", "nocov_depth_nodepth");
    s.flow8 = true;
    add(s, "inputs", "nocov_depth_flow8");
    s = base; s.selector = MV_KP_RANDOM; s.nocov = MV_NOCOV_DEPTH | MV_NOCOV_MATCH; s.graph = MV_GRAPH_ICP;
    add(s, "inputs", "nocov_both_random");
    s.flow8 = true;
    add(s, "inputs", "nocov_both_flow8");
    s = base; s.selector = MV_KP_GRID; s.nocov = MV_NOCOV_MATCH; s.graph = MV_GRAPH_ICP;
    add(s, "inputs", "nocov_match_grid");
    // ---- selectors
    s = base; s.selector = MV_KP_FULL;
    add(s, "selectors", "full_device");
    s.pattern = PERM;
    add(s, "selectors", "full_perm");
    s.lanes = 3;
    add(s, "selectors", "full_three_perm");
    s = base; s.selector = MV_KP_RANDOM;
    add(s, "selectors", "random_device");
    s.env = {{"MV_PIPE_DEVICE_DRAW", "0"}};
    add(s, "selectors", "random_host");
    s.lanes = 3;
    add(s, "selectors", "random_host_three");
    s = base; s.selector = MV_KP_GRID;
    add(s, "selectors", "grid");
    s = base; s.selector = MV_KP_EXPLICIT; s.pattern = KP_HOST;
    add(s, "selectors", "explicit_host");
    s.pattern = KP_DEV;
    add(s, "selectors", "explicit_dev");
    s.lanes = 3;
    add(s, "selectors", "explicit_dev_three");
    s = base; s.pattern = KP_HOST;   // (caller's rows on a CovAware pipe: the candidate list is bypassed)
    add(s, "selectors", "nodepth_keypoints_host");
    // ---- volume modes
    s = base; s.volume_split = 0;
    add(s, "volume", "exact_device");
    s = base; s.volume_split = 3; s.layout = MV_LAYOUT_HWC;
    add(s, "volume", "split3_hwc");
    s.volume_split = 2;
    add(s, "volume", "split2_hwc");
    s = base; s.volume_split = MV_PACK_BF16X3;
    add(s, "volume", "bf16x3");
    s = base; s.C = 48;   // (channels the packed kernel does not cover: the exact fp32 GEMM)
    add(s, "volume", "f16x2_uncovered");
    // (Fast mode's fp16 cells need token-major features and pairs * n8 * n8 >= 2^22 cells: 320 x 320 is 40 x 40 eighths)
    s = base; s.volume_split = MV_VOL_ENC16; s.feat_dtype = MV_F16; s.layout = MV_LAYOUT_HWC; s.H = 320; s.W = 320;
    const Scenario enc16 = add(s, "volume", "enc16_tiled");
    s.env = {{"MV_PIPE_TILED", "0"}};
    add(s, "volume", "enc16_rows");
    s = enc16; s.H = 304;   // (h8 = 38: a padded last tile row)
    add(s, "volume", "enc16_tiled_padded");
    s = enc16; s.W = 336;   // (w8 = 42: no tiling)
    add(s, "volume", "enc16_untileable");
    s = enc16; s.H = 64; s.W = 96;   // (a shape outside the fp16-cell kernel's domain keeps fp32 cells)
    add(s, "volume", "enc16_small_fp32_cells");
    s = base; s.env = {{"MV_PIPE_TILED", "1"}};
    add(s, "volume", "f16x2_tiled");
    // ---- map registration, keyframes
    s = base; s.map = MAP_ONE;
    add(s, "map", "map_one_device");
    s.pattern = PERM;
    add(s, "map", "map_one_perm");
    s = three_dd; s.map = MAP_LANES;
    add(s, "map", "map_lanes_device");
    s = base; s.map = MAP_LANES;
    add(s, "map", "map_lanes_one_device");
    s = base; s.map = MAP_ONE; s.skip_at = 3; s.frames = 6;
    add(s, "map", "skip_one_device");
    s = three_dd; s.map = MAP_LANES; s.skip_at = 3; s.frames = 6;
    add(s, "map", "skip_lanes_device");
    s = base; s.map = MAP_ONE; s.skip_at = 3; s.frames = 6; s.motion = MV_MOTION_TARTAN; s.H = 112; s.W = 160;
    add(s, "map", "skip_one_motion");
    s = base; s.map = MAP_ONE; s.skip_at = 3; s.frames = 6; s.env = {{"MV_PIPE_FUSE_BACKEND", "0"}, {"MV_PIPE_DEVICE_DRAW", "0"}};
    add(s, "map", "skip_one_five_launch");
    // ---- timing
    for (const Scenario& b : {one_dd, one_perm, three_dd}) {
        s = b; s.timing = TIMING_DETAIL;
        add(s, "timing", b.name + "_timed_detail");
        s.timing = TIMING_PAIRS;
        add(s, "timing", b.name + "_timed_pairs");
    }
    // ---- every environment variable the driver reads, at each non-default value
    static const Knob knobs[] = {
        {"MV_PIPE_LAYOUT", "classic"},    {"MV_PIPE_SELECTOR_ON", "main"}, {"MV_PIPE_SELECTOR_ON", "back"}, {"MV_PIPE_SELECTOR_ON", "own"},
        {"MV_PIPE_SELECTOR_ON", "vol"},   {"MV_PIPE_SELECTOR_ON", "late"}, {"MV_PIPE_PACK_ON", "back"},     {"MV_PIPE_PACK_ON", "main"},
        {"MV_PIPE_PACK_ON", "side"},      {"MV_PIPE_LOOKUPS_ON", "vol"},   {"MV_PIPE_FREE_CUS", "0"},       {"MV_PIPE_FREE_CUS", "16"},
        {"MV_PIPE_LEAN", "0"},            {"MV_PIPE_FRONT_ON", "side"},    {"MV_PIPE_FUSE_BACKEND", "0"},   {"MV_PIPE_DEVICE_DRAW", "0"},
        {"MV_PIPE_TILED", "1"},           {"MV_PIPE_ASYNC_BACKEND", "0"},  {"MV_PIPE_LAUNCH_SPIN_US", "0"}, {"MV_PIPE_HOST_STATS", "1"},
    };
    // (three lanes: the classic layout whatever MV_PIPE_LAYOUT / LEAN / FRONT_ON say, its selector segment on the decoder-side stream; DEVICE_DRAW=0 is
    // three_seeded; the launch thread's variables act on no schedule)
    const auto acts_on_classic = [](const Knob& k) {
        for (const char* n : {"MV_PIPE_LAYOUT", "MV_PIPE_LEAN", "MV_PIPE_FRONT_ON", "MV_PIPE_DEVICE_DRAW", "MV_PIPE_ASYNC_BACKEND", "MV_PIPE_LAUNCH_SPIN_US",
                              "MV_PIPE_HOST_STATS"})
            if (strcmp(k.name, n) == 0) return false;
        return strcmp(k.value, "main") != 0 && !(strcmp(k.name, "MV_PIPE_FREE_CUS") == 0 && strcmp(k.value, "0") == 0);
    };
    for (const Scenario& b : {one_dd, one_perm, three_dd})
        for (const Knob& k : knobs) {
            if (b.lanes > 2 && !acts_on_classic(k)) continue;
            s = b; s.env = {k};
            if (b.lanes > 2) s.frames = 4;   // (three volume buffers: frame 3's GEMM already rewrites one)
            s.volume_ahead = strcmp(k.name, "MV_PIPE_LOOKUPS_ON") != 0;   // (that placement keeps the lookups behind the GEMM: no GEMM ahead)
            const std::string group = std::string("knobs_") + b.name;
            add(s, group.c_str(), b.name + "_" + (k.name + 8) + "_" + k.value);
            if (strcmp(k.value, "late") == 0 && b.pattern == PERM) {   // (`late` defers a segment only with two unfinished frames in front of it)
                s.depth = 3;
                add(s, group.c_str(), b.name + "_" + (k.name + 8) + "_" + k.value + "_depth3");
            }
        }
    s = one_perm; s.mapping = 1; s.env = {{"MV_PIPE_SELECTOR_ON", "late"}}; s.depth = 3;
    add(s, "knobs_one_perm", "mapping_SELECTOR_ON_late_depth3");
    s = one_perm; s.lanes = 3; s.env = {{"MV_PIPE_SELECTOR_ON", "late"}}; s.depth = 3;
    add(s, "knobs_three_device", "three_perm_SELECTOR_ON_late_depth3");
    return all;
}

mvFramePipeConfig make_config(const Scenario& s, bool async) {
    mvFramePipeConfig c;
    memset(&c, 0, sizeof(c));
    c.H = s.H; c.W = s.W; c.C = s.C; c.pairs = 2 * s.lanes;
    c.iters = 2; c.radius = 4;
    c.feat_dtype = s.feat_dtype; c.layout = s.layout; c.volume_split = s.volume_split;
    c.selector_mode = s.selector;
    c.kp_kernel_size = 7; c.kp_mask_width = 16;
    c.num_point = s.num_point; c.edgewidth = 8; c.min_num_point = 10;
    c.graph_type = s.graph; c.filters = 1; c.cov_kernel_size = 31;
    c.mapping = s.mapping; c.map_num_point = 100; c.map_mask_width = 16;
    c.async_backend = async ? 1 : -1;
    c.fx = c.fy = 60.f; c.cx = 0.5f * s.W; c.cy = 0.5f * s.H; c.baseline = 0.25f;
    c.bl_fx = 15.f; c.bl_fx_sq = 225.f;
    c.match_cov_default = 0.25f; c.max_match_cov = 100.f; c.max_depth_cov = 250.f; c.max_depth = 15.f;
    c.min_flow_cov_sq = 0.0625f; c.min_depth_cov = 0.05f; c.filter_min_depth = 0.05f;
    c.map_max_depth = 5.f; c.map_max_depth_cov = 0.005f;
    mv_lm_default_params(&c.lm);
    c.cov_model = MV_COV_MATCH;
    c.motion_model = s.motion;
    c.frontend_nocov = s.nocov;
    c.cov_match_cov_default = 0.25f;
    return c;
}

#define CHECK(call)                                                                  \
    do {                                                                             \
        const int rc_ = (call);                                                      \
        if (rc_ != MV_OK) {                                                          \
            fake_hip_dump(stdout);                                                   \
            fprintf(stderr, "pipe_trace: %s -> %d (line %d)\n", #call, rc_, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

void note(const std::string& s) { fake_hip_note(s.c_str()); }

int run(const Scenario& sc, bool async) {
    for (const Knob& k : sc.env) setenv(k.name, k.value, 1);
    fake_hip_event_query_ready(sc.query_ready);
    const mvFramePipeConfig cfg = make_config(sc, async);
    const int L = sc.lanes;
    const size_t bytes = mv_frame_pipe_arena_bytes(&cfg);
    if (!bytes) { fprintf(stderr, "pipe_trace: invalid configuration\n"); return 1; }
    int32_t* arena = (int32_t*)aligned_alloc(256, bytes);
    for (size_t i = 0; i < bytes / 4; ++i) arena[i] = 400;
    fake_hip_arena(arena, bytes);
    // everything the caller hands over: never read by the host except by the copies the fake runtime executes (poses, raw motions), so one zeroed block serves
    std::vector<char> blob(1 << 20, 0);
    char* const dev = blob.data();
    mvFrameInputs in;
    memset(&in, 0, sizeof(in));
    in.fmap1 = dev; in.fmap2 = dev + 256; in.coords = (const float*)(dev + 512);
    const bool any_cov = sc.nocov != (MV_NOCOV_DEPTH | MV_NOCOV_MATCH);
    if (sc.flow8) {
        in.flow8 = (const float*)(dev + 768); in.up_mask = (const float*)(dev + 1024);
        if (any_cov) { in.cov8 = (const float*)(dev + 1280); in.cov_mask = (const float*)(dev + 1536); }
    } else {
        in.flow = (const float*)(dev + 768);
        if (any_cov) in.logcov = (const float*)(dev + 1280);
    }
    float* const sink = (float*)(dev + 4096);
    const float* const motion_raw = (const float*)(dev + 8192);
    const float* const K_dev = (const float*)(dev + 12288);
    const float* const T_BS_dev = (const float*)(dev + 12544);
    mvMapStores stores;
    memset(&stores, 0, sizeof(stores));
    {   // (every store must be there for mv_map_append to take the descriptor; only `pose` is ever written here)
        float* const f = (float*)(dev + 262144);
        double* const d = (double*)f;
        uint8_t* const u = (uint8_t*)f;
        int64_t* const i = (int64_t*)f;
        stores.K = stores.baseline = stores.T_BS = stores.pos_Tw = stores.pixel1_uv = stores.pixel2_uv = stores.pixel1_d = stores.pixel2_d = f;
        stores.pixel1_disp = stores.pixel2_disp = stores.pixel1_disp_cov = stores.pixel2_disp_cov = f;
        stores.pixel1_uv_cov = stores.pixel2_uv_cov = stores.pixel1_d_cov = stores.pixel2_d_cov = stores.mp_pos_Tw = f;
        stores.cov_Tw = stores.obs1_covTc = stores.obs2_covTc = stores.mp_cov_Tw = d;
        stores.need_interp = stores.color = stores.mp_color = u;
        stores.time_ns = stores.frame2match_ranges = stores.frame2match_num = stores.frame2map_ranges = stores.frame2map_num = i;
        stores.match2frame1 = stores.match2frame2 = stores.match2point = stores.point2match_edges = stores.point2match_deg = i;
    }
    stores.pose = (float*)(dev + 16384);
    stores.counts = (int64_t*)(dev + 32768);
    stores.max_pt_obs = 5; stores.max_frame_range = 2;
    stores.cap_frames = 64; stores.cap_match = 1 << 16; stores.cap_points = 1 << 16; stores.cap_map_points = 1 << 16;
    const mvMapStores* const stores_dev = (const mvMapStores*)(dev + 65536);
    const int cap = mv_frame_pipe_table_rows(&cfg) > 0 ? mv_frame_pipe_table_rows(&cfg) : 1;
    std::vector<int64_t> perm((size_t)L * cap), rows((size_t)L * cap * 2), perm_map(cfg.map_num_point), time_ns(L, 0);
    for (int l = 0; l < L; ++l)
        for (int i = 0; i < cap; ++i) {
            perm[(size_t)l * cap + i] = i;
            rows[2 * ((size_t)l * cap + i)] = 15 + i % (sc.W - 30);       // (inside the covariance patch's border)
            rows[2 * ((size_t)l * cap + i) + 1] = 15 + i % (sc.H - 30);
        }
    for (size_t i = 0; i < perm_map.size(); ++i) perm_map[i] = (int64_t)i;

    mvFramePipe* p = nullptr;
    CHECK(mv_frame_pipe_create(&cfg, arena, bytes, &p));
    if (sc.skip_at >= 0) CHECK(mv_frame_pipe_set_solve_frame(p, MV_SOLVE_LOCAL));
    if (sc.pattern == SEEDS) {
        uint64_t seeds[MV_MAX_LANES];
        for (int l = 0; l < L; ++l) seeds[l] = 1234 + l;
        CHECK(mv_frame_pipe_seed_lanes(p, seeds));
    }
    if (sc.timing != NO_TIMING) {
        CHECK(mv_frame_pipe_time_volume(p, 4));   // (fewer slots than frames: timed and untimed frames)
        CHECK(mv_frame_pipe_time_detail(p, sc.timing == TIMING_DETAIL));
    }
    const bool device = mv_frame_pipe_device_draw(p) || (sc.pattern == SEEDS && sc.selector == MV_KP_GRID && !sc.mapping);
    const int depth = sc.depth ? sc.depth : mv_frame_pipe_default_depth(L, sc.mapping);
    note("# device_draw " + std::to_string(mv_frame_pipe_device_draw(p)) + " volume_tiled " + std::to_string(mv_frame_pipe_volume_tiled(p)) + " depth " +
         std::to_string(depth));

    int n_frames_map = 0;   // rows of the map's frame store
    const auto enqueue = [&](int i) -> int {
        note("# enqueue frame " + std::to_string(i));
        CHECK(mv_frame_pipe_enqueue(p, &in, nullptr, i > 0));
        if (i > 0 && sc.motion == MV_MOTION_TARTAN) {
            CHECK(mv_frame_pipe_wait_motion_input(p, nullptr));
            CHECK(mv_frame_pipe_set_motion(p, motion_raw, nullptr));
        }
        return 0;
    };
    const auto skip = [&](int i) -> int {
        note("# skip frame " + std::to_string(i));
        CHECK(mv_frame_pipe_skip(p));
        if (sc.map == MAP_ONE) CHECK(mv_frame_pipe_map_skip(p, &stores, n_frames_map, K_dev, T_BS_dev, cfg.baseline, 0));
        if (sc.map == MAP_LANES) CHECK(mv_frame_pipe_map_skip_lanes(p, stores_dev, n_frames_map, K_dev, T_BS_dev, cfg.baseline, time_ns.data()));
        ++n_frames_map;
        return 0;
    };
    const auto finish = [&]() -> int {
        note("# finish");
        int32_t n_cand[MV_MAX_LANES], n_sel[MV_MAX_LANES];
        for (int l = 0; l < L; ++l) n_cand[l] = n_sel[l] = cap < sc.num_point ? cap : sc.num_point;
        if (sc.pattern == PERM) {
            CHECK(mv_frame_pipe_wait_candidates(p, n_cand));
            for (int l = 0; l < L; ++l) n_sel[l] = n_cand[l] < sc.num_point ? n_cand[l] : sc.num_point;
        }
        CHECK(mv_frame_pipe_release(p, nullptr));
        if (device) CHECK(mv_frame_pipe_finish_device(p, sink));
        else if (sc.pattern == SEEDS) CHECK(mv_frame_pipe_finish_seeded(p, sink, n_cand, n_sel));
        else if (sc.pattern == PERM) CHECK(mv_frame_pipe_finish(p, perm.data(), n_sel, sink));
        else if (sc.pattern == KP_HOST) CHECK(mv_frame_pipe_finish_keypoints(p, rows.data(), n_sel, sink));
        else CHECK(mv_frame_pipe_finish_keypoints_dev(p, (const int64_t*)(dev + 131072), (const int32_t*)(dev + 20480), nullptr, sink));
        if (!device) note("# n_cand " + std::to_string(n_cand[0]) + " n_sel " + std::to_string(n_sel[0]));
        if (sc.map == MAP_ONE)
            CHECK(mv_frame_pipe_map_append(p, &stores, n_frames_map, n_frames_map - 1, K_dev, T_BS_dev, cfg.baseline, 0, nullptr));
        if (sc.map == MAP_LANES)
            CHECK(mv_frame_pipe_map_append_lanes(p, stores_dev, n_frames_map, n_frames_map - 1, K_dev, T_BS_dev, cfg.baseline, time_ns.data()));
        ++n_frames_map;
        if (sc.mapping) {
            int32_t n_valid = 0, n_cand_map = 0;
            CHECK(mv_frame_pipe_wait_tracked(p, &n_valid, &n_cand_map));
            const int n = n_cand_map < cfg.map_num_point ? n_cand_map : cfg.map_num_point;
            note("# n_valid " + std::to_string(n_valid) + " n_cand_map " + std::to_string(n_cand_map));
            CHECK(mv_frame_pipe_map_points(p, perm_map.data(), n, nullptr, sc.map == MAP_ONE ? &stores : nullptr));
        }
        return 0;
    };

    if (device) {   // a frame is enqueued and finished in one go, the next frame's GEMM in between
        for (int i = 0; i < sc.frames; ++i) {
            if (i == sc.skip_at) { if (skip(i)) return 1; continue; }
            if (enqueue(i)) return 1;
            if (sc.volume_ahead && i + 1 < sc.frames && i + 1 != sc.skip_at) CHECK(mv_frame_pipe_enqueue_volume(p, &in, nullptr));
            if (i > 0 && finish()) return 1;
            CHECK(mv_frame_pipe_wait_finished(p, 2));
        }
    } else {        // up to `depth` tracked frames ahead of the one being finished, plus the GEMM of the one after
        int next = 0, pending = 0;
        bool vol = false;
        const auto pump = [&]() -> int {
            while (next < sc.frames && pending < depth && next != sc.skip_at) {
                if (enqueue(next)) return 1;
                pending += next > 0;
                ++next;
                vol = false;
            }
            if (sc.volume_ahead && next < sc.frames && next != sc.skip_at && !vol) {
                CHECK(mv_frame_pipe_enqueue_volume(p, &in, nullptr));
                vol = true;
            }
            return 0;
        };
        if (pump()) return 1;
        while (pending || next < sc.frames) {
            if (!pending && next == sc.skip_at) {   // (a skip takes effect once the frames in front of it have finished)
                if (skip(next)) return 1;
                ++next;
            } else {
                if (finish()) return 1;
                --pending;
            }
            if (pump()) return 1;
        }
    }
    note("# end of stream");
    CHECK(mv_frame_pipe_sync(p, nullptr, 0));
    CHECK(mv_frame_pipe_sync(p, nullptr, 2));
    if (sc.timing != NO_TIMING) {
        float ms[64];
        int n = 0;
        CHECK(mv_frame_pipe_volume_times(p, ms, 16, &n));
        note("# volume_times " + std::to_string(n));
        CHECK(mv_frame_pipe_volume_starts(p, ms, 16, &n));
        note("# volume_starts " + std::to_string(n));
        CHECK(mv_frame_pipe_timeline(p, ms, 16, &n));
        note("# timeline " + std::to_string(n));
        CHECK(mv_frame_pipe_timeline_backend(p, ms, 16, &n));
        note("# timeline_backend " + std::to_string(n));
    }
    if (mv_frame_pipe_device_draw(p)) {
        int32_t nc[MV_MAX_LANES], ns[MV_MAX_LANES];
        CHECK(mv_frame_pipe_finished_counts(p, 0, nc, ns));
        note("# finished_counts n_cand " + std::to_string(nc[0]) + " n_sel " + std::to_string(ns[0]));
    }
    note("# arena_bytes " + std::to_string(bytes));
    std::string none_ids;   // ids that report no buffer at any age, on one line
    for (int which = 0; which <= MV_FB_PRIOR; ++which) {   // one line per id: offset and count (or the error code) at ages 0, 1 and 2
        std::string line = "buffer " + std::to_string(which) + ":";
        bool any = false;
        for (int age = 0; age < 3; ++age) {
            void* ptr = nullptr;
            size_t count = 0;
            const int rc = mv_frame_pipe_buffer(p, which, age, &ptr, &count);
            if (rc != MV_OK) line += " " + std::to_string(rc);
            else line += " A+" + std::to_string((size_t)((char*)ptr - (char*)arena)) + " " + std::to_string(count);
            if (age < 2) line += " |";
            any = any || rc == MV_OK;
        }
        if (any) note(line);
        else none_ids += " " + std::to_string(which);
    }
    note("buffers that report MV_ERR_INVALID_ARG at every age:" + none_ids);
    CHECK(mv_frame_pipe_sync(p, nullptr, 1));
    note("# destroy");
    mv_frame_pipe_destroy(p);
    fake_hip_dump(stdout);
    free(arena);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::vector<Scenario> all = scenarios();
    if (argc >= 2 && strcmp(argv[1], "--list") == 0) {
        for (const Scenario& s : all) printf("%s %s\n", s.group.c_str(), s.name.c_str());
        return 0;
    }
    if (argc < 2) {
        fprintf(stderr, "usage: pipe_trace --list | NAME [--async]\n");
        return 2;
    }
    const bool async = argc >= 3 && strcmp(argv[2], "--async") == 0;
    for (const Scenario& s : all)
        if (s.name == argv[1]) return run(s, async);
    fprintf(stderr, "pipe_trace: no scenario %s\n", argv[1]);
    return 2;
}
