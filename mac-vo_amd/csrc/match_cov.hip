// A13-A16 — MAC-VO 2D->3D covariance model, one 64-lane wave per keypoint
//
// Replaces Module/Covariance/Project2to3.py: MatchCovariance.estimate :124-181 (in-place clamp :131, patch gather
// :141-158, weighted mean/variance :161-172), Utility/Math.py:43-63 (gaussain_full_kernels), Covariance_2to3_full
// :377-423 (NED order z, x, y), create_3x3_matrix + .double() :426-433,:179, and optionally the world-frame
// rotation R cov R^T of Odometry/MACVO.py:273-281 (fp64 bmm(bmm(R, cov), R^T)).
//
// Reference quirk kept on purpose: local_filters[a][b] is the Gaussian at offset
// (x = a - h, y = b - h) with x <-> the FIRST covariance coordinate (u), while patches[a][b] is the depth at
// (v + a - h, u + b - h): the kernel is applied transposed relative to the patch.
//
// gfx950 design: latency-bound (0.8 MB for 200 keypoints).  A wave owns a keypoint: K*K taps are spread
// b-fastest over the lanes so each wave-wide load covers ~2 contiguous 124-B patch rows; taps and weights
// stay in registers (16 each for K = 31); three butterfly reductions (sum k, sum w*z, sum w*(z-mu)^2);
// lane 0 assembles the 3x3 in fp32 with the reference's op order, widens to fp64 and rotates.
//
// mv_obs_cov / mv_obs_cov_pair_lanes: GaussianMixtureCovariance (Project2to3.py:194-262), NoCovariance (:48-57) and the
// Modifier_Diagonalize / Modifier_Normalize chain (:281-323) on the same wave layout (obs_cov_kernel<MODEL, MODS>).  GMM gathers
// the dense depth-variance patch next to the depth patch (same transposed tap order) and keeps c + z^2 per tap (16 more VGPRs).
#include "common.h"
#include <math.h>
#include "match_cov_dev.h"

using namespace mvcov;

namespace {

__global__ __launch_bounds__(256) void match_cov_kernel(CovSet s0, CovSet s1, mvMatchCovParams p, int cap, mvLaneCounts cnt) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int pl = blockIdx.z;
    if (n >= cnt.n[pl]) return;  // whole wave exits together
    match_cov_wave(blockIdx.y ? s1 : s0, p, cap, pl, n);   // the frame's two keypoint sets (kp0 on depth0, kp1 on depth1) share a launch
}

// the other models of ICovariance2to3 and the modifier chain (mv_obs_cov); match_cov_kernel stays the MatchCovariance-without-modifiers form
template <int MODEL, bool MODS>
__global__ __launch_bounds__(256) void obs_cov_kernel(CovSet s0, CovSet s1, mvMatchCovParams p, int cap, mvLaneCounts cnt, int32_t mods,
                                                      const float* depth_cov_map0, const float* depth_cov_map1) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int pl = blockIdx.z;
    if (n >= cnt.n[pl]) return;
    match_cov_wave<MODEL, MODS>(blockIdx.y ? s1 : s0, p, cap, pl, n, mods, blockIdx.y ? depth_cov_map1 : depth_cov_map0);
}

// the pair launch of a frame whose matcher gives no covariance (mv_obs_cov_pair_nomatch_lanes): set 0 as ever, set 1 = match_cov_wave_nomatch.
// Instantiations of their own: match_cov_kernel / obs_cov_kernel stay as they are.
template <int MODEL, bool MODS>
__global__ __launch_bounds__(256) void obs_cov_nomatch_kernel(CovSet s0, CovSet s1, mvMatchCovParams p, int cap, mvLaneCounts cnt, int32_t mods,
                                                              const float* depth_cov_map0, const float* depth_cov_map1, float c1) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int pl = blockIdx.z;
    if (n >= cnt.n[pl]) return;
    if (blockIdx.y == 0)
        match_cov_wave<MODEL, MODS>(s0, p, cap, pl, n, mods, depth_cov_map0);
    else
        match_cov_wave_nomatch<MODEL, MODS>(s1, p, cap, pl, n, c1, mods, depth_cov_map1);
}

template <int MODEL>
void launch_nomatch(bool m, dim3 grid, hipStream_t st, const CovSet& s0, const CovSet& s1, const mvMatchCovParams& p, int cap, const mvLaneCounts& c,
                    int32_t mods, const float* dcm0, const float* dcm1, float c1) {
    if (m)
        hipLaunchKernelGGL((obs_cov_nomatch_kernel<MODEL, true>), grid, dim3(256), 0, st, s0, s1, p, cap, c, mods, dcm0, dcm1, c1);
    else
        hipLaunchKernelGGL((obs_cov_nomatch_kernel<MODEL, false>), grid, dim3(256), 0, st, s0, s1, p, cap, c, mods, dcm0, dcm1, c1);
}

int launch_obs_cov(int model, int32_t mods, dim3 grid, hipStream_t st, const CovSet& s0, const CovSet& s1, const mvMatchCovParams& p, int cap,
                   const mvLaneCounts& c, const float* dcm0, const float* dcm1) {
    const bool m = mods != 0;
    if (model == MV_COV_MATCH && !m)
        hipLaunchKernelGGL(match_cov_kernel, grid, dim3(256), 0, st, s0, s1, p, cap, c);
    else if (model == MV_COV_MATCH)
        hipLaunchKernelGGL((obs_cov_kernel<MV_COV_MATCH, true>), grid, dim3(256), 0, st, s0, s1, p, cap, c, mods, dcm0, dcm1);
    else if (model == MV_COV_GMM && !m)
        hipLaunchKernelGGL((obs_cov_kernel<MV_COV_GMM, false>), grid, dim3(256), 0, st, s0, s1, p, cap, c, mods, dcm0, dcm1);
    else if (model == MV_COV_GMM)
        hipLaunchKernelGGL((obs_cov_kernel<MV_COV_GMM, true>), grid, dim3(256), 0, st, s0, s1, p, cap, c, mods, dcm0, dcm1);
    else if (!m)
        hipLaunchKernelGGL((obs_cov_kernel<MV_COV_NONE, false>), grid, dim3(256), 0, st, s0, s1, p, cap, c, mods, dcm0, dcm1);
    else
        hipLaunchKernelGGL((obs_cov_kernel<MV_COV_NONE, true>), grid, dim3(256), 0, st, s0, s1, p, cap, c, mods, dcm0, dcm1);
    return mv_launch_status();
}

}  // namespace

// Every covariance entry point ends here: the one copy of the argument checks, of CovSet and of the grid.  A single form is lanes = 1, cap = N, one set.
int mv_obs_cov_launch(const mvObsCovLaunch& d, mvStream_t stream) {
    MV_CHECK_ARG(d.model >= MV_COV_MATCH && d.model <= MV_COV_NONE && mv_cov_modifiers_ok(d.modifiers) && d.params);
    mvLaneCounts c{};
    int n_max = 0;
    const int rc = check_lanes(d.lanes, d.n_live, d.cap, c, n_max);
    if (rc != MV_OK) return rc;
    if (n_max == 0) return MV_OK;
    const mvCovKeypoints &k0 = d.set0, &k1 = d.pair ? d.set1 : d.set0;
    MV_CHECK_ARG(k0.depth_map && k0.kp_uv && k0.flow_cov && k0.out_cov && k1.depth_map && k1.kp_uv && (k1.flow_cov || d.no_match_cov) && k1.out_cov);
    const mvMatchCovParams p = *d.params;
    MV_CHECK_ARG(p.H > 0 && p.W > 0 && p.kernel_size >= 1 && (p.kernel_size & 1));
    // (an oversized kernel is "unsupported", not "invalid": the single forms say so before they look at the depth variances, the pair forms behind that)
    if (!d.pair && p.kernel_size > MAX_K) return MV_ERR_UNSUPPORTED;
    MV_CHECK_ARG(p.use_patch_var || (!d.pair && k0.depth_cov));
    // the mixture model needs the depth model's variance: both dense maps and, for a set without match covariance, the one gathered at its keypoints
    MV_CHECK_ARG(d.model != MV_COV_GMM || (d.depth_cov_map0 && d.depth_cov_map1 && (!d.no_match_cov || k1.depth_cov)));
    if (p.kernel_size > MAX_K) return MV_ERR_UNSUPPORTED;
    MV_CHECK_ARG(!k0.out_cov_rot || k0.rot);
    const CovSet s0{k0.depth_map, k0.kp_uv, k0.flow_cov, k0.depth_cov, k0.rot, k0.out_cov, k0.out_cov_rot, k0.out_stats};
    const CovSet s1{k1.depth_map, k1.kp_uv, k1.flow_cov, k1.depth_cov, k1.rot, k1.out_cov, k1.out_cov_rot, k1.out_stats};
    const dim3 grid(mv_ceil_div(n_max, 4), d.pair ? 2 : 1, d.lanes);
    hipStream_t st = (hipStream_t)stream;
    if (!d.no_match_cov) return launch_obs_cov(d.model, d.modifiers, grid, st, s0, s1, p, d.cap, c, d.depth_cov_map0, d.depth_cov_map1);
    const bool m = d.modifiers != 0;
    if (d.model == MV_COV_MATCH)
        launch_nomatch<MV_COV_MATCH>(m, grid, st, s0, s1, p, d.cap, c, d.modifiers, d.depth_cov_map0, d.depth_cov_map1, d.model_match_cov_default);
    else if (d.model == MV_COV_GMM)
        launch_nomatch<MV_COV_GMM>(m, grid, st, s0, s1, p, d.cap, c, d.modifiers, d.depth_cov_map0, d.depth_cov_map1, d.model_match_cov_default);
    else
        launch_nomatch<MV_COV_NONE>(m, grid, st, s0, s1, p, d.cap, c, d.modifiers, d.depth_cov_map0, d.depth_cov_map1, d.model_match_cov_default);
    return mv_launch_status();
}

extern "C" int mv_obs_cov(int model, int32_t modifiers, const float* depth_map, const float* depth_cov_map, const float* kp_uv, float* flow_cov,
                          const float* depth_cov, const double* rot, const mvMatchCovParams* params, int N, double* out_cov, double* out_cov_rot,
                          float* out_stats, mvStream_t stream) {
    const int32_t n = N;
    mvObsCovLaunch d{};
    d.model = model; d.modifiers = modifiers; d.params = params; d.lanes = 1; d.n_live = &n; d.cap = N;
    d.set0 = mvCovKeypoints{depth_map, kp_uv, flow_cov, depth_cov, rot, out_cov, out_cov_rot, out_stats};
    d.depth_cov_map0 = d.depth_cov_map1 = depth_cov_map;
    return mv_obs_cov_launch(d, stream);
}

extern "C" int mv_obs_cov_pair_lanes(int model, int32_t modifiers, const float* depth_map0, const float* depth_cov_map0, const float* kp_uv0,
                                     float* flow_cov0, const double* rot0, double* out_cov0, double* out_cov_rot0, const float* depth_map1,
                                     const float* depth_cov_map1, const float* kp_uv1, float* flow_cov1, double* out_cov1,
                                     const mvMatchCovParams* params, int lanes, const int32_t* n_live, int cap, mvStream_t stream) {
    mvObsCovLaunch d{};
    d.model = model; d.modifiers = modifiers; d.params = params; d.lanes = lanes; d.n_live = n_live; d.cap = cap;
    d.pair = true;
    d.set0 = mvCovKeypoints{depth_map0, kp_uv0, flow_cov0, nullptr, rot0, out_cov0, out_cov_rot0, nullptr};
    d.set1 = mvCovKeypoints{depth_map1, kp_uv1, flow_cov1, nullptr, nullptr, out_cov1, nullptr, nullptr};
    d.depth_cov_map0 = depth_cov_map0; d.depth_cov_map1 = depth_cov_map1;
    return mv_obs_cov_launch(d, stream);
}

extern "C" int mv_obs_cov_pair_nomatch_lanes(int model, int32_t modifiers, const float* depth_map0, const float* depth_cov_map0, const float* kp_uv0,
                                             float* flow_cov0, const double* rot0, double* out_cov0, double* out_cov_rot0, const float* depth_map1,
                                             const float* depth_cov_map1, const float* kp_uv1, const float* depth_cov1, float model_match_cov_default,
                                             double* out_cov1, const mvMatchCovParams* params, int lanes, const int32_t* n_live, int cap,
                                             mvStream_t stream) {
    mvObsCovLaunch d{};
    d.model = model; d.modifiers = modifiers; d.params = params; d.lanes = lanes; d.n_live = n_live; d.cap = cap;
    d.pair = true;
    d.set0 = mvCovKeypoints{depth_map0, kp_uv0, flow_cov0, nullptr, rot0, out_cov0, out_cov_rot0, nullptr};
    d.set1 = mvCovKeypoints{depth_map1, kp_uv1, nullptr, depth_cov1, nullptr, out_cov1, nullptr, nullptr};
    d.depth_cov_map0 = depth_cov_map0; d.depth_cov_map1 = depth_cov_map1;
    d.no_match_cov = true; d.model_match_cov_default = model_match_cov_default;
    return mv_obs_cov_launch(d, stream);
}

// MatchCovariance without modifiers: (MV_COV_MATCH, 0) is what launch_obs_cov sends to match_cov_kernel
extern "C" int mv_match_cov(const float* depth_map, const float* kp_uv, float* flow_cov, const float* depth_cov,
                            const double* rot, const mvMatchCovParams* params, int N, double* out_cov,
                            double* out_cov_rot, float* out_stats, mvStream_t stream) {
    return mv_obs_cov(MV_COV_MATCH, 0, depth_map, nullptr, kp_uv, flow_cov, depth_cov, rot, params, N, out_cov, out_cov_rot, out_stats, stream);
}

extern "C" int mv_match_cov_pair_lanes(const float* depth_map0, const float* kp_uv0, float* flow_cov0, const double* rot0,
                                       double* out_cov0, double* out_cov_rot0, const float* depth_map1,
                                       const float* kp_uv1, float* flow_cov1, double* out_cov1,
                                       const mvMatchCovParams* params, int lanes, const int32_t* n_live, int cap,
                                       mvStream_t stream) {
    return mv_obs_cov_pair_lanes(MV_COV_MATCH, 0, depth_map0, nullptr, kp_uv0, flow_cov0, rot0, out_cov0, out_cov_rot0, depth_map1, nullptr, kp_uv1,
                                 flow_cov1, out_cov1, params, lanes, n_live, cap, stream);
}

extern "C" int mv_match_cov_pair(const float* depth_map0, const float* kp_uv0, float* flow_cov0, const double* rot0,
                                 double* out_cov0, double* out_cov_rot0, const float* depth_map1, const float* kp_uv1,
                                 float* flow_cov1, double* out_cov1, const mvMatchCovParams* params, int N,
                                 mvStream_t stream) {
    MV_CHECK_ARG(N >= 0);
    const int32_t n = N;
    return mv_match_cov_pair_lanes(depth_map0, kp_uv0, flow_cov0, rot0, out_cov0, out_cov_rot0, depth_map1, kp_uv1, flow_cov1,
                                   out_cov1, params, 1, &n, N, stream);
}

