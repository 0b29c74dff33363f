// Host-side descriptors of a frame's backend = two launches: the front launch (frontend_ops.hip: mv_backend_front) and the posed solve
// (pgo_solve.hip: mv_posed_solve).  Internal: the public entry points of macvo_hip.h fill them from their positional arguments, the frame driver
// lays the parts that do not change per frame out once (frame_pipe.hip: describe_backend).  They are unpacked into the kernels' own argument structs.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "macvo_hip.h"

struct mvDepthMaps {   // one frame's dense maps, [lanes, H, W] each; only `depth` is required (sdd: also for MV_COV_GMM)
    const float *depth, *disp, *sdisp, *sdd;
};
struct mvFrontMaps {   // what the front launch reads: the match maps of the newer frame, the depth maps of both
    const float *match_flow, *match_cov;
    mvDepthMaps f0, f1;
};
struct mvFrontTables {   // per-keypoint outputs of the front launch, [lanes, cap, ...] (vals: [11, lanes, cap])
    int64_t* kp0_uv;
    float *kp0, *kp1;
    uint8_t* inbound;
    float *vals, *sigma0, *sigma1, *pos_Tc;
    double *cov0, *cov1;
};
struct mvCovConfig {   // mv_obs_cov's model + modifier chain, and the tracking constants that go with it
    int model;
    int32_t modifiers;
    mvMatchCovParams cp;
    int edge;
    float match_cov_default;
    int nocov;                        // MV_NOCOV_*: covariances the frontend does not provide (0 = all there)
    float model_match_cov_default;    // MV_NOCOV_MATCH: the model's own sigma of a keypoint without match covariance (Project2to3.py:133,216)
};
// Where the keypoint rows of a front launch come from (PM of backend_front_kernel); each kind reads only the fields named for it.
enum mvKpSourceKind {
    MV_KPSRC_PERM,     // a permutation over the candidate list, perm_dev (PM 0) or — perm_host, one lane, <= 256 rows — in the kernel arguments (PM 1); n_live
    MV_KPSRC_DRAW,     // the device-driven frame (round 6): the permutation is drawn inside the launch (PM 2) from the candidate count n_live_dev[l * n_live_stride] and
                       // state_in -> state_out, and published (out_perm, out_live).  The number of live rows never reaches the host: the grid covers num_point rows
                       // per lane and the waves beyond min(count, num_point) retire at once
    MV_KPSRC_ROWS,     // (PM 3) `rows` used as given: coordinates outside the image read pixel 0 and are marked out of bounds, a covariance patch that leaves the
                       // image is clamped — callers keep keypoints cov_kernel_size / 2 inside; live rows n_live[l] or n_live_dev[l * n_live_stride] clamped to
                       // [0, cap], published to out_live if given
    MV_KPSRC_RANDOM,   // (PM 4) RandomSelector: num_point rows per lane, mask_width from the border, drawn from state_in; the advanced generators go to state_out
    MV_KPSRC_GRID      // (PM 5) the mv_kp_grid_count(H, W, mask_width, num_point) rows of GridSelector
};
struct mvKpSource {
    int kind;
    const int32_t* cand;         // [lanes, cand_lane_stride] linear pixel indices
    size_t cand_lane_stride;
    const int64_t *perm_dev, *perm_host;   // [lanes, cap] indices into cand
    const int64_t* rows;         // int64 [lanes, cap, 2] (u, v) in device memory (may be the kp0_uv table itself)
    const int32_t* n_live;       // host [lanes]
    const int32_t* n_live_dev;   // device: lane l at n_live_dev[l * n_live_stride]
    int n_live_stride;
    const uint32_t* state_in;    // [lanes, mv_randperm_state_words()]
    uint32_t* state_out;         // != state_in
    int num_point, mask_width;
    int64_t* out_perm;           // [lanes, cap]
    int32_t* out_live;           // [lanes, 2]: the live-row count as the device-count solves read it
};

struct mvPosedSolve {   // mv_pgo_solve_posed*'s arguments; the plain mv_pgo_solve leaves pos_Tc null
    int nprob;
    const int32_t* offsets;
    int cap, graph_type;
    const float *init_pose, *start_pose;   // start_pose (optional): the LM start of the motion-model form, init_pose then only rotates the rows
    const float *intrinsics, *baseline;
    const float* pos_Tc;
    const double* cov_Tc;
    float* pos_Tw;       // written by the fold, read by the solve (plain solve: read only)
    double* cov_Tw;
    double* out_rot;
    const float *pixel2_uv, *pixel2_d, *pixel2_disp, *pixel2_disp_cov, *pixel2_uv_cov;
    const double* obs2_covTc;
    const int32_t* n_live;       // live rows per problem: host [nprob] ...
    const int32_t* n_live_dev;   // ... or device, problem l at n_live_dev[l * n_live_stride]
    int n_live_stride;
    int filter_flags;            // < 0: no filter prologue, `valid` is an input
    float filter_min_depth, filter_max_depth;
    const uint8_t* inbound;
    const float* vals;
    uint8_t* valid;
    int32_t* count_out;
    int min_points;
    const mvLMParams* params;
    double *out_pose, *out_info;
    float *out_pose_f32, *pose_sink;
    const float* ref_pose;       // (optional) T_o2w [nprob, 7]: solve in its frame (Local_TwoFrame_PGO)
};

struct mvCovKeypoints {   // one keypoint set of a covariance launch (CovSet of match_cov_dev.h): tables [lanes, cap, .], depth_map [lanes, H, W], rot [lanes, 9]
    const float *depth_map, *kp_uv;
    float* flow_cov;          // clamped in place
    const float* depth_cov;   // per-keypoint depth variance (optional: the patch statistic otherwise)
    const double* rot;
    double *out_cov, *out_cov_rot;
    float* out_stats;
};
struct mvObsCovLaunch {   // mv_match_cov* / mv_obs_cov*'s arguments: one launch of match_cov_kernel, obs_cov_kernel or obs_cov_nomatch_kernel
    int model;
    int32_t modifiers;
    const mvMatchCovParams* params;
    int lanes;
    const int32_t* n_live;   // host [lanes]
    int cap;
    mvCovKeypoints set0, set1;
    bool pair;               // set1 given: a frame's two calls (kp0 on depth0, kp1 on depth1) in one launch; both need params->use_patch_var
    const float *depth_cov_map0, *depth_cov_map1;   // dense depth variance [lanes, H, W] (MV_COV_GMM)
    bool no_match_cov;       // (pair) set 1 without match covariance: sigma (c, c, 0) with c = model_match_cov_default, its flow_cov is not read
    float model_match_cov_default;
};

// (hidden: the library exports the C entry points of macvo_hip.h only)
// frontend_ops.hip — the fused front launch (backend_front_kernel): keypoint rows + gather + track + back-projection + both covariance models
__attribute__((visibility("hidden"))) int mv_backend_front(const mvKpSource& src, int lanes, int cap, const mvFrontMaps& m, const mvCovConfig& cv,
                                                           const mvFrontTables& t, mvStream_t stream);
// pgo_solve.hip — filters + rotation into the world frame + LM solve in one launch (pgo_solve_kernel with the prologue)
__attribute__((visibility("hidden"))) int mv_posed_solve(const mvPosedSolve& d, mvStream_t stream);
// ... and the same launch without the prologue (mv_pgo_solve, mv_pgo_solve_local): d.pos_Tc null, pos_Tw / cov_Tw / valid are inputs
__attribute__((visibility("hidden"))) int mv_plain_solve(const mvPosedSolve& d, mvStream_t stream);
// match_cov.hip — the covariance model of one or both keypoint sets of a frame, the argument checks of every mv_match_cov* / mv_obs_cov* entry point
__attribute__((visibility("hidden"))) int mv_obs_cov_launch(const mvObsCovLaunch& d, mvStream_t stream);
// corr_lookup.hip — the window lookup on a volume of fp32 or (cells16) fp16 cells, row-major or (tiled) in 4 x 4-cell tiles
__attribute__((visibility("hidden"))) int mv_lookup(const void* vol, bool cells16, bool tiled, const float* coords, float* out, int B, int H1, int W1,
                                                    int H2, int W2, int radius, mvStream_t stream);
