// Local_TwoFrame_PGO — the two frame changes around the LM solve (Module/Optimization/TwoFramePGO/Optimizer.py:111-150), shared by the
// local instantiations of pgo_solve_kernel (pgo_solve.hip) and by tests/c_abi/pgo_local_twin.cpp (g++, host), like pgo_math.h.
//
//   world_to_optim  Optimizer.py:131-143   T_w2o = Inv(T_o2w)                      fp32  (:122)
//                                          T_c2o = T_w2o @ T_c2w                   fp32  (:137)
//                                          R_w2o = T_w2o.rotation().matrix()       fp32, widened to fp64 (:138)
//                                          pos_To = Act(T_w2o, pos_Tw)             fp32  (:141)
//                                          cov_To = (R_w2o cov_Tw) R_w2o^T         fp64  (:142)
//   optim_to_world  Optimizer.py:145-150   NormalizeQuat(T_o2w @ float(T_c2o))     fp32  (Utility/Math.py:124-133)
//
// Every fp32 operation is one rounding in PyPose's order (the library and the twin are built with -ffp-contract=off): SO3 Act is
// (p + w uv) + qv x uv with uv = 2 (qv x p); SO3 Mul is (aw bv + bw av) + av x bv | aw bw - ((ax bx + ay by) + az bz); Inv is (-Act(q^-1, t), q^-1);
// the quaternion norm of NormalizeQuat is the square root of the squares added left to right.  The one fused operation is inside the cross
// product: the reference's optimizer runs on the CPU (GraphInput(..., "cpu"), Optimizer.py:38), where torch.linalg.cross evaluates a component as
// fmsub(a1, b2, a2 * b1) — one product rounded, the other fused into the subtraction.  Spelled out here as fmaf, these stages carry the bits of the
// reference's own run (tests/golden/local_pgo.npz); pose_apply_dev.h's Act, which registers the rows in the world frame, keeps its unfused cross.
#pragma once
#include "pgo_math.h"

namespace pgo {

// torch.linalg.cross on the CPU, fp32
MV_HD void cross_f32(const float* a, const float* b, float* o) {
    o[0] = fmaf(a[1], b[2], -(a[2] * b[1]));
    o[1] = fmaf(a[2], b[0], -(a[0] * b[2]));
    o[2] = fmaf(a[0], b[1], -(a[1] * b[0]));
}

// PyPose SO3_Act in fp32: uv = 2 (qv x p); (p + w uv) + qv x uv
MV_HD void so3_act_f32(const float* q, const float* p, float* o) {
    float uv[3], c[3];
    cross_f32(q, p, uv);
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    cross_f32(q, uv, c);
    o[0] = (p[0] + q[3] * uv[0]) + c[0];
    o[1] = (p[1] + q[3] * uv[1]) + c[1];
    o[2] = (p[2] + q[3] * uv[2]) + c[2];
}

// pp.SE3.Inv in fp32: q^-1 = (-v, w), t^-1 = -Act(q^-1, t)
MV_HD void se3_inv_f32(const float* T, float* Ti) {
    const float qi[4] = {-T[3], -T[4], -T[5], T[6]};
    float r[3];
    so3_act_f32(qi, T, r);
    Ti[0] = -r[0]; Ti[1] = -r[1]; Ti[2] = -r[2];
    Ti[3] = qi[0]; Ti[4] = qi[1]; Ti[5] = qi[2]; Ti[6] = qi[3];
}

// pp.SE3 a @ b in fp32: t = a.t + Act(a.q, b.t), q = a.q * b.q
MV_HD void se3_mul_f32(const float* a, const float* b, float* o) {
    float r[3];
    so3_act_f32(a + 3, b, r);
    o[0] = a[0] + r[0]; o[1] = a[1] + r[1]; o[2] = a[2] + r[2];
    const float* av = a + 3; const float aw = a[6];
    const float* bv = b + 3; const float bw = b[6];
    float c[3];
    cross_f32(av, bv, c);
    o[3] = (aw * bv[0] + bw * av[0]) + c[0];
    o[4] = (aw * bv[1] + bw * av[1]) + c[1];
    o[5] = (aw * bv[2] + bw * av[2]) + c[2];
    o[6] = aw * bw - ((av[0] * bv[0] + av[1] * bv[1]) + av[2] * bv[2]);
}

// T.rotation().matrix() in fp32 (columns are SO3_Act(q, e_i)), widened to fp64: row-major R
MV_HD void se3_rotation_f64(const float* T, double* R) {
    MV_UNROLL
    for (int c = 0; c < 3; ++c) {
        const float e[3] = {c == 0 ? 1.f : 0.f, c == 1 ? 1.f : 0.f, c == 2 ? 1.f : 0.f};
        float col[3];
        so3_act_f32(T + 3, e, col);
        R[c] = (double)col[0]; R[3 + c] = (double)col[1]; R[6 + c] = (double)col[2];
    }
}

// what the solve needs of T_o2w before its LM loop
struct LocalFrame {
    float T_w2o[7];
    double R_w2o[9];
};

MV_HD void local_frame(const float* ref_pose /* T_o2w */, LocalFrame& f) {
    se3_inv_f32(ref_pose, f.T_w2o);
    se3_rotation_f64(f.T_w2o, f.R_w2o);
}

// pos_To = Act(T_w2o, pos_Tw) in fp32
MV_HD void local_point_f32(const LocalFrame& f, const float* pw, float* po) {
    float r[3];
    so3_act_f32(f.T_w2o + 3, pw, r);
    po[0] = r[0] + f.T_w2o[0]; po[1] = r[1] + f.T_w2o[1]; po[2] = r[2] + f.T_w2o[2];
}

// cov_To = (R cov_Tw) R^T in fp64 (the grouping of pose_apply_dev.h's sandwich)
MV_HD void local_cov_f64(const LocalFrame& f, const double* c, double* o) {
    const double* R = f.R_w2o;
    double tm[9];
    MV_UNROLL
    for (int i = 0; i < 3; ++i)
        MV_UNROLL
        for (int j = 0; j < 3; ++j) tm[3 * i + j] = (R[3 * i] * c[j] + R[3 * i + 1] * c[3 + j]) + R[3 * i + 2] * c[6 + j];
    MV_UNROLL
    for (int i = 0; i < 3; ++i)
        MV_UNROLL
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (tm[3 * i] * R[3 * j] + tm[3 * i + 1] * R[3 * j + 1]) + tm[3 * i + 2] * R[3 * j + 2];
}

// a loaded point (pgo_math.h's load_point has read the world-frame row) moved into the optimisation frame: pos from the fp32 row, the ICP
// graph's point covariance in place.  REPROJ / DISP never read cov_Tw.
template <int GT>
MV_HD void local_point(const LocalFrame& f, const float* pos_Tw_row, PointData<GT>& d) {
    float po[3];
    local_point_f32(f, pos_Tw_row, po);
    d.pw[0] = (double)po[0]; d.pw[1] = (double)po[1]; d.pw[2] = (double)po[2];
    if (GT == MV_GRAPH_ICP) {
        double o[9];
        local_cov_f64(f, d.Sp, o);
        MV_UNROLL
        for (int k = 0; k < 9; ++k) d.Sp[k] = o[k];
    }
}

// optim_to_world: the fp64 LM result cast to fp32, T_o2w @ it, quaternion normalised — all fp32
MV_HD void local_to_world_f32(const float* ref_pose /* T_o2w */, const double* t, const double* q, float* out) {
    const float Tc2o[7] = {(float)t[0], (float)t[1], (float)t[2], (float)q[0], (float)q[1], (float)q[2], (float)q[3]};
    float w[7];
    se3_mul_f32(ref_pose, Tc2o, w);
    const float n = sqrtf(((w[3] * w[3] + w[4] * w[4]) + w[5] * w[5]) + w[6] * w[6]);
    out[0] = w[0]; out[1] = w[1]; out[2] = w[2];
    out[3] = w[3] / n; out[4] = w[4] / n; out[5] = w[5] / n; out[6] = w[6] / n;
}

}  // namespace pgo
