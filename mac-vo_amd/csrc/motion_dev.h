// TartanMotionNet's data-parallel arithmetic around the pose network (Module/MotionModel.py:90-123), shared by motion_model.hip
// (device) and by the CPU suite's host build (tests/test_motion_model_host.py compiles this header with g++).
//
// Replaces, per lane:
//   make_device_intrinsic_layer          Module/Network/TartanVOStereo/Utility.py:13-18 (called with (height, width) in the (w, h) slots)
//   cropAndResize (centerCropTo + F.interpolate(bilinear, align_corners=True))   StereoVO_Interface.py:162-174, Utility/Utils.py:65-72
//   reciprocal / nan_to_num / clamp / the two scalar divisions        StereoVO_Interface.py:183-186
//   torch.cat((flow * 0.05, depth, intrinsic), 1)                       :188
//   prev_pose @ pp.se3(pose.squeeze() * pose_norm).Exp()               MotionModel.py:112, StereoVO_Interface.py:194
//
// Every torch op of the reference is one rounding here, in its order (the library is built with -ffp-contract=off).  The one
// exception is the bilinear tap sum: ATen's upsample_bilinear2d kernel is compiled with HIP's default fp contraction, which fuses
// two of its multiplies into each sum; bilerp() spells those fmaf()s out (measured against torch on the device).
#pragma once
#include <math.h>
#include <float.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MV_MD __host__ __device__ __forceinline__
#else
#define MV_MD static inline
#endif

namespace motion {

constexpr int OUT_H = 112, OUT_W = 160, OUT_C = 5;   // the PoseNet input of TartanVO (StereoVO_Interface.py:179)

// centerCropTo of one axis followed by align_corners=True bilinear down to `out`: the crop keeps size - 2 * ((size - target) // 2)
// elements (one more than target when the difference is odd) and starts at (size - target) // 2; the source-index scale is
// area_pixel_compute_scale against the 112 x 160 output: (float)(len - 1) / (out - 1), a host fp32 division
struct Axis {
    int off, len;
    float scale;
};

MV_MD Axis axis_of(int size, int target, int out) {
    Axis a;
    const int to_crop = (size - target) / 2;
    a.off = to_crop;
    a.len = size - 2 * to_crop;
    a.scale = (float)(a.len - 1) / (float)(out - 1);
    return a;
}

// s = min(int(H / 112), int(W / 160)) (cropAndResize); 0 when the frame is smaller than the PoseNet input
MV_MD int crop_scale(int H, int W) {
    const int sh = H / OUT_H, sw = W / OUT_W;
    return sh < sw ? sh : sw;
}

struct Taps {
    int r0, r1, c0, c1;   // absolute rows / columns of the four taps (r1 == r0 / c1 == c0 at the last source row / column)
    float h0l, h1l, w0l, w1l;
};

// upsample_bilinear2d_out_frame's index arithmetic (area_pixel_compute_source_index of ATen/native/hip/UpSample.cuh) for output
// (h2, w2): h1r = scale * h2 rounded, h1lambda = h1r - h1 (not fused), h0lambda = 1 - h1lambda
MV_MD Taps taps_of(const Axis& ah, const Axis& aw, int h2, int w2) {
    Taps t;
    const float h1r = ah.scale * h2;
    int h1 = (int)h1r;
    h1 = h1 < ah.len - 1 ? h1 : ah.len - 1;   // (never taken: a guard for the addresses only)
    const int h1p = (h1 < ah.len - 1) ? 1 : 0;
    t.h1l = h1r - h1;
    t.h0l = 1.0f - t.h1l;
    const float w1r = aw.scale * w2;
    int w1 = (int)w1r;
    w1 = w1 < aw.len - 1 ? w1 : aw.len - 1;
    const int w1p = (w1 < aw.len - 1) ? 1 : 0;
    t.w1l = w1r - w1;
    t.w0l = 1.0f - t.w1l;
    t.r0 = ah.off + h1; t.r1 = t.r0 + h1p;
    t.c0 = aw.off + w1; t.c1 = t.c0 + w1p;
    return t;
}

// ATen: h0lambda * (w0lambda * a00 + w1lambda * a01) + h1lambda * (w0lambda * a10 + w1lambda * a11), which torch's device build
// evaluates as fma(h0l, fma(w0l, a00, w1l * a01), h1l * fma(w0l, a10, w1l * a11)) (each sum fuses its FIRST product)
MV_MD float bilerp(const Taps& t, float a00, float a01, float a10, float a11) {
    const float x0 = fmaf(t.w0l, a00, t.w1l * a01);
    const float x1 = fmaf(t.w0l, a10, t.w1l * a11);
    return fmaf(t.h0l, x0, t.h1l * x1);
}

// make_device_intrinsic_layer(meta.height, meta.width, fx, fy, cx, cy): the reference passes (height, width) into the (w, h) slots,
// so the meshgrid's first axis runs over ROWS with (fx, cx) and the second over COLUMNS with (fy, cy), stacked (hh, ww):
//   channel 0 = (col - cy + 0.5) / fy,   channel 1 = (row - cx + 0.5) / fx
// Kept as the reference computes it.  Each op one fp32 rounding; "/ fx" of a tensor by a host scalar is ATen's multiplication by
// the fp32 reciprocal (div_true_kernel_cuda), inv_fx = 1.0f / (float)fx.
MV_MD float intrinsic_at(int i, float o, float inv_f) {
    float v = (float)i - o;
    v = v + 0.5f;
    return v * inv_f;
}

struct DepthConsts {
    float bl_fx;       // (float)(frame_baseline * fx): the Python double product, rounded once
    float stereo_norm; // (float)0.02
    float inv_bl_fx;   // 1.0f / bl_fx
    float inv_norm;    // 1.0f / (float)(0.02 * 0.25)
};

// stereo = (bl * fx) / depth_resize         -> depth_resize.reciprocal() * bl_fx (Tensor.__rdiv__)
// stereo = nan_to_num(stereo * 0.02, nan=0) -> NaN -> 0, +-inf -> +-FLT_MAX
//          .clamp(min=0)
// depth  = stereo / (bl * fx) / (0.02 * 0.25)
MV_MD float depth_channel(float d, const DepthConsts& k) {
    float s = 1.0f / d;
    s = s * k.bl_fx;
    s = s * k.stereo_norm;
    if (s != s) s = 0.0f;
    else if (s == INFINITY) s = FLT_MAX;
    else if (s == -INFINITY) s = -FLT_MAX;
    s = fmaxf(s, 0.0f);
    s = s * k.inv_bl_fx;
    return s * k.inv_norm;
}

// ---------------------------------------------------------------------------------------------- se3 Exp + SE3 compose (fp32)
// PyPose 0.6.8 in the tensor dtype (restated in tests/golden/pypose_shim.py: _so3_exp, _so3_Jl, _Se3Algebra.Exp, LieTensor.__mul__):
//   phi = m[3:6], th = |phi|;  th > eps(fp32):  q = [phi sin(th/2)/th, cos(th/2)],  c1 = (1 - cos th)/th^2,  c2 = (th - sin th)/th^3
//                              otherwise:       q = [phi (0.5 - th^2/48 + th^4/3840), 1 - th^2/8 + th^4/384],  c1 = 0.5 - th^2/24,  c2 = 1/6 - th^2/120
//   t_e = (I + c1 K + c2 K K) rho;   out = [t_prev + q_prev.Act(t_e),  q_prev * q_e]   (right multiplication)
MV_MD void so3_act_f(const float* q, const float* p, float* o) {
    float uv0 = q[1] * p[2] - q[2] * p[1], uv1 = q[2] * p[0] - q[0] * p[2], uv2 = q[0] * p[1] - q[1] * p[0];
    uv0 = uv0 + uv0; uv1 = uv1 + uv1; uv2 = uv2 + uv2;
    o[0] = p[0] + q[3] * uv0 + (q[1] * uv2 - q[2] * uv1);
    o[1] = p[1] + q[3] * uv1 + (q[2] * uv0 - q[0] * uv2);
    o[2] = p[2] + q[3] * uv2 + (q[0] * uv1 - q[1] * uv0);
}

MV_MD void se3_exp_f(const float* m, float* t, float* q) {
    const float* rho = m;
    const float* phi = m + 3;
    const float th = sqrtf(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
    const float th2 = th * th, th4 = th2 * th2;
    const float eps = FLT_EPSILON;
    float imag, real, c1, c2;
    if (th > eps) {
        const float half = 0.5f * th;
        imag = sinf(half) / th;
        real = cosf(half);
        c1 = (1.0f - cosf(th)) / (th * th);
        c2 = (th - sinf(th)) / (th * th * th);
    } else {
        imag = 0.5f - th2 / 48.0f + th4 / 3840.0f;
        real = 1.0f - th2 / 8.0f + th4 / 384.0f;
        c1 = 0.5f - th2 / 24.0f;
        c2 = 1.0f / 6.0f - th2 / 120.0f;
    }
    q[0] = phi[0] * imag; q[1] = phi[1] * imag; q[2] = phi[2] * imag; q[3] = real;
    // K rho = phi x rho;  K K rho = phi x (phi x rho)
    const float k0 = phi[1] * rho[2] - phi[2] * rho[1], k1 = phi[2] * rho[0] - phi[0] * rho[2], k2 = phi[0] * rho[1] - phi[1] * rho[0];
    const float kk0 = phi[1] * k2 - phi[2] * k1, kk1 = phi[2] * k0 - phi[0] * k2, kk2 = phi[0] * k1 - phi[1] * k0;
    t[0] = rho[0] + c1 * k0 + c2 * kk0;
    t[1] = rho[1] + c1 * k1 + c2 * kk1;
    t[2] = rho[2] + c1 * k2 + c2 * kk2;
}

// out = prev @ Exp(raw * pose_norm): [7] fp32 each (tx ty tz qx qy qz qw)
MV_MD void pose_exp_compose(const float* prev, const float* raw, const float* norm, float* out) {
    float m[6];
    for (int k = 0; k < 6; ++k) m[k] = raw[k] * norm[k];
    float te[3], qe[4];
    se3_exp_f(m, te, qe);
    const float* qa = prev + 3;
    float at[3];
    so3_act_f(qa, te, at);
    out[0] = prev[0] + at[0]; out[1] = prev[1] + at[1]; out[2] = prev[2] + at[2];
    // SO3 mul: [aw bv + bw av + av x bv,  aw bw - av . bv]
    const float ax = qa[0], ay = qa[1], az = qa[2], aw = qa[3];
    const float bx = qe[0], by = qe[1], bz = qe[2], bw = qe[3];
    out[3] = aw * bx + bw * ax + (ay * bz - az * by);
    out[4] = aw * by + bw * ay + (az * bx - ax * bz);
    out[5] = aw * bz + bw * az + (ax * by - ay * bx);
    out[6] = aw * bw - (ax * bx + ay * by + az * bz);
}

}  // namespace motion
