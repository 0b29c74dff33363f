// SE(3) interpolation in fp64 — the arithmetic of Utility/Math.py:96-121 (interpolate_pose) through PyPose's SE3 Inv / Mul / Log / Exp (RESTATED from
// PyPose 0.6.8's published algorithm, UNPINNED: PyPose is not a vendored dependency), shared by
//   visual_map.hip   MotionInterpolate (Module/MapProcessor.py:52-76) and PoseInterpolate (:28-49) on the device-resident maps,
//   traj_assoc.hip   Trajectory.align_time / align_origin (Utility/Trajectory.py:105-114, 172-176, 188-191) for mv_traj_associate_lanes,
// and by tests/c_abi/assoc_twin.cpp (g++, host: a replay of one lane of each new kernel, which the CPU suite checks against tests/traj_assoc_ref.py
// BEFORE the kernels reach a GPU — test infrastructure only).
//
// Everything here is fp64 on exactly widened inputs; the caller rounds once, at its store.  The reference's own chain for an fp32 estimate is MIXED:
// fp32 Inv / @ / Log, an fp64 Exp (the proportion is fp64 and promotes the tangent), fp32 again after `.to(P_seg_start)` and after
// `from_evo(...).float()`.  That chain is not reproduced bit for bit — the transcendental functions differ and PyPose is not installed; the measured
// gap is ASSOC_F32_CHAIN_MEASURED in tests/traj_assoc_cases.py and DESIGN.md section 7.
//
// Plain C++ without fma(): the library and the twin are built with -ffp-contract=off, so both round every operation once, in this order.  Arrays
// are indexed by constants only, so on the device everything stays in registers.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "macvo_hip.h"

#if defined(__HIPCC__)
#define SE3_HD __host__ __device__ __forceinline__
#else
#define SE3_HD static inline
#endif

namespace se3i {

struct Se3d {
    double t[3], q[4];
};

SE3_HD void q_act(const double* q, const double* p, double* o) {   // PyPose SO3_Act
    double u0 = q[1] * p[2] - q[2] * p[1], u1 = q[2] * p[0] - q[0] * p[2], u2 = q[0] * p[1] - q[1] * p[0];
    u0 += u0; u1 += u1; u2 += u2;
    o[0] = p[0] + q[3] * u0 + (q[1] * u2 - q[2] * u1);
    o[1] = p[1] + q[3] * u1 + (q[2] * u0 - q[0] * u2);
    o[2] = p[2] + q[3] * u2 + (q[0] * u1 - q[1] * u0);
}
SE3_HD void q_mul(const double* a, const double* b, double* o) {   // PyPose SO3_Mul (x, y, z, w)
    o[0] = a[3] * b[0] + b[3] * a[0] + (a[1] * b[2] - a[2] * b[1]);
    o[1] = a[3] * b[1] + b[3] * a[1] + (a[2] * b[0] - a[0] * b[2]);
    o[2] = a[3] * b[2] + b[3] * a[2] + (a[0] * b[1] - a[1] * b[0]);
    o[3] = a[3] * b[3] - (a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
}
SE3_HD Se3d se3_mul(const Se3d& a, const Se3d& b) {
    Se3d o;
    double r[3];
    q_act(a.q, b.t, r);
    o.t[0] = a.t[0] + r[0]; o.t[1] = a.t[1] + r[1]; o.t[2] = a.t[2] + r[2];
    q_mul(a.q, b.q, o.q);
    return o;
}
SE3_HD Se3d se3_inv(const Se3d& a) {
    Se3d o;
    o.q[0] = -a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = a.q[3];
    double r[3];
    q_act(o.q, a.t, r);
    o.t[0] = -r[0]; o.t[1] = -r[1]; o.t[2] = -r[2];
    return o;
}
SE3_HD Se3d se3_normq(Se3d a) {   // Utility/Math.py:124-133 NormalizeQuat
    const double n = sqrt(a.q[0] * a.q[0] + a.q[1] * a.q[1] + a.q[2] * a.q[2] + a.q[3] * a.q[3]);
    a.q[0] /= n; a.q[1] /= n; a.q[2] /= n; a.q[3] /= n;
    return a;
}
SE3_HD void skew_sq_apply(const double* k, const double* v, double c1, double c2, double* o) {
    // o = v + c1 * (k x v) + c2 * (k x (k x v))
    const double a0 = k[1] * v[2] - k[2] * v[1], a1 = k[2] * v[0] - k[0] * v[2], a2 = k[0] * v[1] - k[1] * v[0];
    const double b0 = k[1] * a2 - k[2] * a1, b1 = k[2] * a0 - k[0] * a2, b2 = k[0] * a1 - k[1] * a0;
    o[0] = v[0] + c1 * a0 + c2 * b0;
    o[1] = v[1] + c1 * a1 + c2 * b1;
    o[2] = v[2] + c1 * a2 + c2 * b2;
}
// PyPose SE3_Log: phi = SO3_Log(q), rho = Jl^-1(phi) t   (tangent = [rho, phi])
SE3_HD void se3_log(const Se3d& a, double* xi) {
    const double eps = 2.220446049250313e-16;
    double v[3] = {a.q[0], a.q[1], a.q[2]}, w = a.q[3];
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    // PyPose SO3_Log: factor = 2 atan(|v| / w) / |v| (w != 0), with the small-|v| series 2/w - 2 |v|^2 / (3 w^3)
    double factor;
    if (n > eps) {
        factor = (fabs(w) > eps) ? 2.0 * atan(n / w) / n : (w >= 0 ? M_PI : -M_PI) / n;
    } else {
        factor = 2.0 / w - 2.0 * n * n / (3.0 * w * w * w);
    }
    double phi[3] = {v[0] * factor, v[1] * factor, v[2] * factor};
    const double th = sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
    // so3_Jl_inv = I - K/2 + c K^2, c = (1 - th cos(th/2) / (2 sin(th/2))) / th^2, series 1/12 + th^2/720
    double c;
    if (th > eps) {
        const double h = 0.5 * th;
        c = (1.0 - th * cos(h) / (2.0 * sin(h))) / (th * th);
    } else {
        c = 1.0 / 12.0 + th * th / 720.0;
    }
    skew_sq_apply(phi, a.t, -0.5, c, xi);
    xi[3] = phi[0]; xi[4] = phi[1]; xi[5] = phi[2];
}
// PyPose se3_Exp: t = Jl(phi) rho, q = so3_Exp(phi)
SE3_HD Se3d se3_exp(const double* xi) {
    const double eps = 2.220446049250313e-16;
    const double* phi = xi + 3;
    const double th = sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
    const double th2 = th * th, th4 = th2 * th2;
    Se3d o;
    double c1, c2, imag, real;
    if (th > eps) {
        c1 = (1.0 - cos(th)) / th2;
        c2 = (th - sin(th)) / (th2 * th);
        imag = sin(0.5 * th) / th;
        real = cos(0.5 * th);
    } else {
        c1 = 0.5 - th2 / 24.0;
        c2 = 1.0 / 6.0 - th2 / 120.0;
        imag = 0.5 - th2 / 48.0 + th4 / 3840.0;
        real = 1.0 - th2 / 8.0 + th4 / 384.0;
    }
    skew_sq_apply(phi, xi, c1, c2, o.t);
    o.q[0] = phi[0] * imag; o.q[1] = phi[1] * imag; o.q[2] = phi[2] * imag; o.q[3] = real;
    return o;
}
SE3_HD Se3d load_pose(const float* p) {
    Se3d o;
    o.t[0] = p[0]; o.t[1] = p[1]; o.t[2] = p[2];
    o.q[0] = p[3]; o.q[1] = p[4]; o.q[2] = p[5]; o.q[3] = p[6];
    return o;
}
SE3_HD Se3d load_pose(const double* p) {
    Se3d o;
    o.t[0] = p[0]; o.t[1] = p[1]; o.t[2] = p[2];
    o.q[0] = p[3]; o.q[1] = p[4]; o.q[2] = p[5]; o.q[3] = p[6];
    return o;
}

// interpolate_pose's segment (Utility/Math.py:116-119): Exp(prop * Log(Pe Ps^-1)) Ps
SE3_HD Se3d se3_interp(const Se3d& Ps, const Se3d& Pe, double prop) {
    double xi[6];
    se3_log(se3_mul(Pe, se3_inv(Ps)), xi);
    xi[0] *= prop; xi[1] *= prop; xi[2] *= prop; xi[3] *= prop; xi[4] *= prop; xi[5] *= prop;
    return se3_mul(se3_exp(xi), Ps);
}

SE3_HD bool finite_pose(const Se3d& p) {
    bool ok = true;
    ok &= fabs(p.t[0]) <= DBL_MAX; ok &= fabs(p.t[1]) <= DBL_MAX; ok &= fabs(p.t[2]) <= DBL_MAX;
    ok &= fabs(p.q[0]) <= DBL_MAX; ok &= fabs(p.q[1]) <= DBL_MAX; ok &= fabs(p.q[2]) <= DBL_MAX; ok &= fabs(p.q[3]) <= DBL_MAX;
    return ok;
}

// ------------------------------------------------------------------------------------------------ trajectory association, one lane
// What one lane of mv_traj_associate_lanes reads; the kernel and the host twin run the functions below on it, the kernel one query per thread.
struct AssocLane {
    const void *src, *ts, *tq, *origin;   // origin: the reference's first row or null
    int32_t T, Q;
    int64_t src_stride;                   // elements between source rows (>= 7)
    int32_t src_f64, time_i64, origin_f64, rebase;
};

constexpr int ASSOC_BAD_NONFINITE = 1, ASSOC_BAD_UNSORTED = 2;
constexpr int ASSOC_SEARCH_STEPS = 31;    // hard cap of the binary search: T < 2^31 needs no more

// Stamp i of a clock, as fp64.  Rebased (Trajectory.py:107-108) it is relative to the clock's own first element: int64 stamps are subtracted as
// integers and only the difference is converted (EuRoC's nanoseconds, about 1.4e18, do not fit fp64), fp64 stamps in fp64 as the reference does.
SE3_HD double assoc_stamp(const void* clock, int i64, int rebase, int i) {
    if (i64) {
        const int64_t* p = (const int64_t*)clock;
        return rebase ? (double)(int64_t)((uint64_t)p[i] - (uint64_t)p[0]) : (double)p[i];
    }
    const double* p = (const double*)clock;
    return rebase ? p[i] - p[0] : p[i];
}

SE3_HD Se3d assoc_raw_row(const void* rows, int f64, int64_t stride, int i) {
    return f64 ? load_pose((const double*)rows + (int64_t)i * stride) : load_pose((const float*)rows + (int64_t)i * stride);
}

// Source row i as the placement sees it.  With an origin row every source pose is first left-multiplied by ref_0 src_0^-1 (evo's align_origin as
// Trajectory.py:188-191 calls it, restated), its quaternion normalised and given w >= 0 — what evo's matrix round trip leaves.
SE3_HD Se3d assoc_row(const AssocLane& a, int i) {
    Se3d p = assoc_raw_row(a.src, a.src_f64, a.src_stride, i);
    if (!a.origin) return p;
    const Se3d A = se3_mul(se3_normq(assoc_raw_row(a.origin, a.origin_f64, 7, 0)), se3_inv(se3_normq(assoc_raw_row(a.src, a.src_f64, a.src_stride, 0))));
    p = se3_normq(se3_mul(A, se3_normq(p)));
    if (p.q[3] < 0) {
        p.q[0] = -p.q[0]; p.q[1] = -p.q[1]; p.q[2] = -p.q[2]; p.q[3] = -p.q[3];
    }
    return p;
}

// The lane-wide checks, item i of max(T, Q): ASSOC_BAD_* bits.  Math.py:97 asserts ts[i] < ts[i + 1] (on the stamps it is given: the rebased ones).
SE3_HD int assoc_check(const AssocLane& a, int i) {
    int bad = 0;
    if (i < a.T) {
        const double t0 = assoc_stamp(a.ts, a.time_i64, a.rebase, i);
        if (!(fabs(t0) <= DBL_MAX)) bad |= ASSOC_BAD_NONFINITE;
        if (i + 1 < a.T && !(t0 < assoc_stamp(a.ts, a.time_i64, a.rebase, i + 1))) bad |= ASSOC_BAD_UNSORTED;
        if (!finite_pose(assoc_raw_row(a.src, a.src_f64, a.src_stride, i))) bad |= ASSOC_BAD_NONFINITE;
        if (i == 0 && a.origin && !finite_pose(assoc_raw_row(a.origin, a.origin_f64, 7, 0))) bad |= ASSOC_BAD_NONFINITE;
    }
    if (i < a.Q && !(fabs(assoc_stamp(a.tq, a.time_i64, a.rebase, i)) <= DBL_MAX)) bad |= ASSOC_BAD_NONFINITE;
    return bad;
}

SE3_HD int assoc_status(int T, int bad) {
    return T < 1 ? (int)MV_TRAJ_TOO_SHORT : (bad & ASSOC_BAD_NONFINITE) ? (int)MV_TRAJ_NONFINITE : (bad & ASSOC_BAD_UNSORTED) ? (int)MV_TRAJ_UNSORTED : (int)MV_TRAJ_OK;
}

// Query j of an OK lane (Math.py:99-121): -> the pose, returns the `extrapolated` flag (~interp_mask).
SE3_HD int assoc_query(const AssocLane& a, int j, Se3d& out) {
    const double tq = assoc_stamp(a.tq, a.time_i64, a.rebase, j);
    if (tq <= assoc_stamp(a.ts, a.time_i64, a.rebase, 0)) {
        out = assoc_row(a, 0);
        return 1;
    }
    if (tq >= assoc_stamp(a.ts, a.time_i64, a.rebase, a.T - 1)) {
        out = assoc_row(a, a.T - 1);
        return 1;
    }
    // searchsorted(right=False): e = the first index with ts[e] >= tq; ts[lo] < tq <= ts[hi] holds throughout
    int lo = 0, hi = a.T - 1;
    for (int step = 0; step < ASSOC_SEARCH_STEPS && hi - lo > 1; ++step) {
        const int mid = lo + (hi - lo) / 2;
        if (assoc_stamp(a.ts, a.time_i64, a.rebase, mid) < tq) lo = mid; else hi = mid;
    }
    const double t_s = assoc_stamp(a.ts, a.time_i64, a.rebase, hi - 1), t_e = assoc_stamp(a.ts, a.time_i64, a.rebase, hi);
    const double prop = (tq - t_s) / (t_e - t_s);
    out = se3_interp(assoc_row(a, hi - 1), assoc_row(a, hi), prop);
    return 0;
}

// ------------------------------------------------------------------------------------------------ PoseInterpolate, one row
// PoseInterpolate.elaborate_map (Module/MapProcessor.py:33-45): bad = need_interp with the first and last five rows forced to 0.
SE3_HD bool pose_interp_bad(const uint8_t* need_interp, int T, int i) { return i >= 5 && i < T - 5 && need_interp[i] != 0; }

// Row i of a lane: false where the row is good; else `out` = se3_interp(pose[s], pose[e], prop) from its nearest good rows s < i < e (rows 4 and
// T - 5 are always good, so both walks end inside the table).  prop = float(i - s) / float(e - s): torch divides two int64 tensors in the default
// dtype, float32 (Utility/Math.py:114), then the product with the fp64 tangent widens it.
SE3_HD bool pose_interp_row(const float* pose, const uint8_t* need_interp, int T, int i, Se3d& out) {
    if (!pose_interp_bad(need_interp, T, i)) return false;
    int s = i - 1, e = i + 1;
    while (pose_interp_bad(need_interp, T, s)) --s;
    while (pose_interp_bad(need_interp, T, e)) ++e;
    const double prop = (double)((float)(i - s) / (float)(e - s));
    out = se3_interp(load_pose(pose + 7 * (size_t)s), load_pose(pose + 7 * (size_t)e), prop);
    return true;
}

}  // namespace se3i
