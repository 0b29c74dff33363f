// TartanMotionNet's preprocessing and pose composition (Module/MotionModel.py:90-123, TartanVOStereo/StereoVO_Interface.py:158-194)
//
// The reference runs ~15 small torch launches per frame on full-resolution maps around the learned PoseNet: an H x W intrinsic
// layer, three crop + bilinear passes, reciprocal / nan_to_num / clamp / two scalar divisions, a cat and a PyPose compose.
// The PoseNet itself is the caller's (eager PyTorch, or posenet.hip); the rest is two launches here:
//
//   mv_motion_input_lanes   one thread per output pixel of a lane: the four bilinear taps of the cropped flow (2 planes), depth and
//                           intrinsic layer (computed at the tap from its row / column, never materialised), then the depth transform;
//                           writes [lanes, 5, 112, 160] fp32 (350 KB per lane) — latency-bound, ~10 reads and 5 writes per thread
//   mv_pose_exp_compose     one thread per pose: prior = prev @ Exp(raw * pose_norm) (motion_dev.h)
//
// Arithmetic and rounding order: motion_dev.h.
#include "common.h"
#include "motion_dev.h"

namespace {

struct MotionLaneArgs {
    const float* flow;    // lane l: flow + l * flow_stride -> [2, H, W]
    const float* depth;   // lane l: depth + l * depth_stride -> [H, W]
    long long flow_stride, depth_stride;
    int H, W;
    motion::Axis ah, aw;
    bool copy;            // cropped size == 112 x 160: F.interpolate copies (no tap arithmetic)
    float cx, cy, inv_fx, inv_fy, flow_norm;
    motion::DepthConsts dk;
    float* out;           // [lanes, 5, 112, 160]
};

__global__ __launch_bounds__(256) void motion_input_kernel(MotionLaneArgs a) {
    using namespace motion;
    constexpr int PLANE = OUT_H * OUT_W;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int lane = blockIdx.y;
    if (idx >= PLANE) return;
    const int h2 = idx / OUT_W, w2 = idx - h2 * OUT_W;
    const size_t HW = (size_t)a.H * a.W;
    const float* fu = a.flow + (size_t)lane * a.flow_stride;
    const float* fv = fu + HW;
    const float* dp = a.depth + (size_t)lane * a.depth_stride;
    float* o = a.out + (size_t)lane * OUT_C * PLANE + idx;

    float u, v, d, i0, i1;
    if (a.copy) {
        const int r = a.ah.off + h2, c = a.aw.off + w2;
        const size_t p = (size_t)r * a.W + c;
        u = fu[p]; v = fv[p]; d = dp[p];
        i0 = intrinsic_at(c, a.cy, a.inv_fy);
        i1 = intrinsic_at(r, a.cx, a.inv_fx);
    } else {
        const Taps t = taps_of(a.ah, a.aw, h2, w2);
        const size_t p00 = (size_t)t.r0 * a.W + t.c0, p01 = (size_t)t.r0 * a.W + t.c1;
        const size_t p10 = (size_t)t.r1 * a.W + t.c0, p11 = (size_t)t.r1 * a.W + t.c1;
        u = bilerp(t, fu[p00], fu[p01], fu[p10], fu[p11]);
        v = bilerp(t, fv[p00], fv[p01], fv[p10], fv[p11]);
        d = bilerp(t, dp[p00], dp[p01], dp[p10], dp[p11]);
        // channel 0 varies along columns only, channel 1 along rows only: the taps' values, interpolated like any other plane
        const float c0 = intrinsic_at(t.c0, a.cy, a.inv_fy), c1 = intrinsic_at(t.c1, a.cy, a.inv_fy);
        const float r0 = intrinsic_at(t.r0, a.cx, a.inv_fx), r1 = intrinsic_at(t.r1, a.cx, a.inv_fx);
        i0 = bilerp(t, c0, c1, c0, c1);
        i1 = bilerp(t, r0, r0, r1, r1);
    }
    o[0] = u * a.flow_norm;
    o[PLANE] = v * a.flow_norm;
    o[2 * PLANE] = depth_channel(d, a.dk);
    o[3 * PLANE] = i0;
    o[4 * PLANE] = i1;
}

__global__ __launch_bounds__(64) void pose_exp_compose_kernel(int n, const float* prev, const float* raw, long long raw_stride,
                                                              const float* norm, float* out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float nrm[6], r[6], pv[7], po[7];
#pragma unroll
    for (int k = 0; k < 6; ++k) { nrm[k] = norm[k]; r[k] = raw[(size_t)i * raw_stride + k]; }
#pragma unroll
    for (int k = 0; k < 7; ++k) pv[k] = prev[7 * (size_t)i + k];
    motion::pose_exp_compose(pv, r, nrm, po);
#pragma unroll
    for (int k = 0; k < 7; ++k) out[7 * (size_t)i + k] = po[k];
}

}  // namespace

extern "C" int mv_motion_input_lanes(int lanes, int H, int W, const float* flow, long long flow_lane_stride, const float* depth,
                                     long long depth_lane_stride, float fx, float fy, float cx, float cy, float bl_fx, float* out,
                                     mvStream_t stream) {
    using namespace motion;
    MV_CHECK_ARG(lanes >= 1 && lanes <= 65535 && flow && depth && out);
    MV_CHECK_ARG(crop_scale(H, W) >= 1);   // the frame must cover the 112 x 160 PoseNet input
    MV_CHECK_ARG(flow_lane_stride >= 2LL * H * W || lanes == 1);
    MV_CHECK_ARG(depth_lane_stride >= (long long)H * W || lanes == 1);
    const int s = crop_scale(H, W);
    MotionLaneArgs a;
    a.flow = flow; a.depth = depth;
    a.flow_stride = flow_lane_stride; a.depth_stride = depth_lane_stride;
    a.H = H; a.W = W;
    a.ah = axis_of(H, OUT_H * s, OUT_H);
    a.aw = axis_of(W, OUT_W * s, OUT_W);
    a.copy = a.ah.len == OUT_H && a.aw.len == OUT_W;
    a.cx = cx; a.cy = cy;
    a.inv_fx = 1.0f / fx;
    a.inv_fy = 1.0f / fy;
    a.flow_norm = 0.05f;                       // flow_norm (StereoVO_Interface.py:54)
    a.dk.bl_fx = bl_fx;
    a.dk.stereo_norm = 0.02f;                  // stereoNormFactor (:28)
    a.dk.inv_bl_fx = 1.0f / bl_fx;
    a.dk.inv_norm = 1.0f / (float)(0.02 * 0.25);   // float(stereoNormFactor * poseDepthNormFactor): a Python double, then the fp32 reciprocal
    a.out = out;
    dim3 grid((OUT_H * OUT_W + 255) / 256, lanes);
    hipLaunchKernelGGL(motion_input_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    return mv_launch_status();
}

extern "C" int mv_pose_exp_compose(int n, const float* prev, const float* raw, long long raw_stride, const float* pose_norm, float* out,
                                   mvStream_t stream) {
    MV_CHECK_ARG(n >= 0);
    if (n == 0) return MV_OK;
    MV_CHECK_ARG(prev && raw && pose_norm && out && raw_stride >= 6);
    hipLaunchKernelGGL(pose_exp_compose_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, n, prev, raw, raw_stride, pose_norm, out);
    return mv_launch_status();
}
