// Trajectory evaluation — the fp64 arithmetic of ATE / RTE / ROE / RPE (Evaluation/MetricsSeq.py:9-51 through evo 1.x, RESTATED, UNPINNED: evo is
// not a vendored dependency, so its published definition is written out here), shared by traj_eval.hip (device) and by tests/c_abi/traj_twin.cpp
// (g++, host: a replay of one lane in the kernel's reduction order, which the CPU suite checks against tests/traj_ref.py BEFORE the kernel reaches a
// GPU — test infrastructure only).
//
// Replaces, for time-associated tracks of equal length:
//   evo.core.transformations.quaternion_matrix      pose_to_rt
//   evo.core.geometry.umeyama_alignment             svd3 + umeyama_tail
//   evo.core.trajectory.PosePath3D.align / scale / transform / align_origin
//   evo.core.metrics.APE (translation_part) / RPE (translation_part, rotation_angle_deg, full_transformation; delta = 1 frame)
//
// Plain C++ without fma(): the library is built with -ffp-contract=off, the twin too, so both round every operation once, in this order.
// Every 3 x 3 array is indexed by constants only (the three Jacobi pairs are written out): nothing here is addressed at run time, so on the
// device everything stays in registers.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "macvo_hip.h"

#if defined(__HIPCC__)
#define TRAJ_HD __host__ __device__ __forceinline__
#else
#define TRAJ_HD static inline
#endif

namespace traj {

constexpr int THREADS = 256;        // workgroup size of traj_eval_kernel = the twin's replay width (4 waves of 64)
constexpr int JACOBI_SWEEPS = 24;   // hard cap: a 3 x 3 matrix converges in 5-7 sweeps; the loop ends here whatever the data are
constexpr double RAD2DEG = 57.295779513082320876798154814105;

struct Rt {
    double R[9];   // row-major
    double t[3];
};

TRAJ_HD void identity(Rt& a) {
    a.R[0] = 1; a.R[1] = 0; a.R[2] = 0;
    a.R[3] = 0; a.R[4] = 1; a.R[5] = 0;
    a.R[6] = 0; a.R[7] = 0; a.R[8] = 1;
    a.t[0] = a.t[1] = a.t[2] = 0;
}

// (tx ty tz qx qy qz qw) -> [R | t].  evo's quaternion_matrix: q is normalised through its squared norm n (q *= sqrt(2 / n), the matrix from the
// outer product), n < 4 eps gives the identity; q and -q give the same products.
TRAJ_HD void pose_to_rt(const double p[7], Rt& a) {
    a.t[0] = p[0]; a.t[1] = p[1]; a.t[2] = p[2];
    const double x = p[3], y = p[4], z = p[5], w = p[6];
    const double n = w * w + x * x + y * y + z * z;
    if (!(n >= 4.0 * DBL_EPSILON)) {
        a.R[0] = 1; a.R[1] = 0; a.R[2] = 0;
        a.R[3] = 0; a.R[4] = 1; a.R[5] = 0;
        a.R[6] = 0; a.R[7] = 0; a.R[8] = 1;
        return;
    }
    const double s = sqrt(2.0 / n);
    const double qw = w * s, qx = x * s, qy = y * s, qz = z * s;
    const double xx = qx * qx, yy = qy * qy, zz = qz * qz;
    const double xy = qx * qy, xz = qx * qz, yz = qy * qz;
    const double xw = qx * qw, yw = qy * qw, zw = qz * qw;
    a.R[0] = 1.0 - yy - zz; a.R[1] = xy - zw;       a.R[2] = xz + yw;
    a.R[3] = xy + zw;       a.R[4] = 1.0 - xx - zz; a.R[5] = yz - xw;
    a.R[6] = xz - yw;       a.R[7] = yz + xw;       a.R[8] = 1.0 - xx - yy;
}

TRAJ_HD void mat3_mul(const double A[9], const double B[9], double C[9]) {
    C[0] = A[0] * B[0] + A[1] * B[3] + A[2] * B[6];
    C[1] = A[0] * B[1] + A[1] * B[4] + A[2] * B[7];
    C[2] = A[0] * B[2] + A[1] * B[5] + A[2] * B[8];
    C[3] = A[3] * B[0] + A[4] * B[3] + A[5] * B[6];
    C[4] = A[3] * B[1] + A[4] * B[4] + A[5] * B[7];
    C[5] = A[3] * B[2] + A[4] * B[5] + A[5] * B[8];
    C[6] = A[6] * B[0] + A[7] * B[3] + A[8] * B[6];
    C[7] = A[6] * B[1] + A[7] * B[4] + A[8] * B[7];
    C[8] = A[6] * B[2] + A[7] * B[5] + A[8] * B[8];
}
// A^T B
TRAJ_HD void mat3_tmul(const double A[9], const double B[9], double C[9]) {
    C[0] = A[0] * B[0] + A[3] * B[3] + A[6] * B[6];
    C[1] = A[0] * B[1] + A[3] * B[4] + A[6] * B[7];
    C[2] = A[0] * B[2] + A[3] * B[5] + A[6] * B[8];
    C[3] = A[1] * B[0] + A[4] * B[3] + A[7] * B[6];
    C[4] = A[1] * B[1] + A[4] * B[4] + A[7] * B[7];
    C[5] = A[1] * B[2] + A[4] * B[5] + A[7] * B[8];
    C[6] = A[2] * B[0] + A[5] * B[3] + A[8] * B[6];
    C[7] = A[2] * B[1] + A[5] * B[4] + A[8] * B[7];
    C[8] = A[2] * B[2] + A[5] * B[5] + A[8] * B[8];
}
TRAJ_HD void mat3_vec(const double A[9], const double v[3], double o[3]) {
    o[0] = A[0] * v[0] + A[1] * v[1] + A[2] * v[2];
    o[1] = A[3] * v[0] + A[4] * v[1] + A[5] * v[2];
    o[2] = A[6] * v[0] + A[7] * v[1] + A[8] * v[2];
}
TRAJ_HD void mat3_tvec(const double A[9], const double v[3], double o[3]) {
    o[0] = A[0] * v[0] + A[3] * v[1] + A[6] * v[2];
    o[1] = A[1] * v[0] + A[4] * v[1] + A[7] * v[2];
    o[2] = A[2] * v[0] + A[5] * v[1] + A[8] * v[2];
}

// c = a b
TRAJ_HD void compose(const Rt& a, const Rt& b, Rt& c) {
    mat3_mul(a.R, b.R, c.R);
    double v[3];
    mat3_vec(a.R, b.t, v);
    c.t[0] = v[0] + a.t[0]; c.t[1] = v[1] + a.t[1]; c.t[2] = v[2] + a.t[2];
}
// c = a^-1 b  (R_a^T R_b, R_a^T (t_b - t_a)): the translations are differenced first, so a track far from the origin loses nothing
TRAJ_HD void inv_compose(const Rt& a, const Rt& b, Rt& c) {
    mat3_tmul(a.R, b.R, c.R);
    const double d[3] = {b.t[0] - a.t[0], b.t[1] - a.t[1], b.t[2] - a.t[2]};
    mat3_tvec(a.R, d, c.t);
}
TRAJ_HD void inverse(const Rt& a, Rt& c) {
    c.R[0] = a.R[0]; c.R[1] = a.R[3]; c.R[2] = a.R[6];
    c.R[3] = a.R[1]; c.R[4] = a.R[4]; c.R[5] = a.R[7];
    c.R[6] = a.R[2]; c.R[7] = a.R[5]; c.R[8] = a.R[8];
    double v[3];
    mat3_tvec(a.R, a.t, v);
    c.t[0] = -v[0]; c.t[1] = -v[1]; c.t[2] = -v[2];
}

// ---- the three error relations -------------------------------------------------------------------------------------------------------------
// APE, translation_part: || trans(A P_i) - trans(Q_i) || with A = [R | t] applied to the estimate whose translation was scaled by c first
TRAJ_HD double ate_error(const Rt& A, double c, const double p[3], const double q[3]) {
    const double s[3] = {c * p[0], c * p[1], c * p[2]};
    double v[3];
    mat3_vec(A.R, s, v);
    const double ex = (v[0] + A.t[0]) - q[0], ey = (v[1] + A.t[1]) - q[1], ez = (v[2] + A.t[2]) - q[2];
    return sqrt(ex * ex + ey * ey + ez * ez);
}
// RPE, delta = 1: E = (Q_i^-1 Q_j)^-1 (P_i^-1 P_j), j = i + 1.  A rigid left factor of the estimate cancels inside P_i^-1 P_j, so of the
// alignment only the scale c enters: trans(P_i^-1 P_j) = c R_i^T (t_j - t_i).
// -> rte = ||trans E||, roe = angle(rot E) in degrees, rpe = ||E - I_4||_F
TRAJ_HD void rel_errors(const Rt& Pi, const Rt& Pj, const Rt& Qi, const Rt& Qj, double c, double& rte, double& roe, double& rpe) {
    Rt dp, dq, E;
    inv_compose(Pi, Pj, dp);
    dp.t[0] *= c; dp.t[1] *= c; dp.t[2] *= c;
    inv_compose(Qi, Qj, dq);
    inv_compose(dq, dp, E);
    rte = sqrt(E.t[0] * E.t[0] + E.t[1] * E.t[1] + E.t[2] * E.t[2]);
    // rotation angle: sin(theta) * axis from the antisymmetric part, cos(theta) from the trace; atan2 of the two keeps small angles accurate
    // (acos of the trace loses half the digits there)
    const double vx = 0.5 * (E.R[7] - E.R[5]), vy = 0.5 * (E.R[2] - E.R[6]), vz = 0.5 * (E.R[3] - E.R[1]);
    const double sn = sqrt(vx * vx + vy * vy + vz * vz);
    const double cs = 0.5 * ((E.R[0] + E.R[4] + E.R[8]) - 1.0);
    roe = atan2(sn, cs) * RAD2DEG;
    const double a0 = E.R[0] - 1.0, a4 = E.R[4] - 1.0, a8 = E.R[8] - 1.0;
    rpe = sqrt(a0 * a0 + E.R[1] * E.R[1] + E.R[2] * E.R[2] + E.R[3] * E.R[3] + a4 * a4 + E.R[5] * E.R[5] + E.R[6] * E.R[6] + E.R[7] * E.R[7] +
               a8 * a8 + E.t[0] * E.t[0] + E.t[1] * E.t[1] + E.t[2] * E.t[2]);
}

// ---- 3 x 3 SVD: one-sided (Hestenes) Jacobi on C itself ------------------------------------------------------------------------------------
// One rotation of columns p, q of G (and of V) that makes the two columns of G orthogonal.  The test is RELATIVE (the cosine of the angle between
// the columns against eps), so a small singular value keeps its own relative accuracy and an exactly null column is never touched.
#define TRAJ_JACOBI_PAIR(p, q)                                                                                                                  \
    {                                                                                                                                           \
        const double al = G[p] * G[p] + G[3 + p] * G[3 + p] + G[6 + p] * G[6 + p];                                                              \
        const double be = G[q] * G[q] + G[3 + q] * G[3 + q] + G[6 + q] * G[6 + q];                                                              \
        const double ga = G[p] * G[q] + G[3 + p] * G[3 + q] + G[6 + p] * G[6 + q];                                                              \
        if (ga != 0.0 && fabs(ga) > DBL_EPSILON * sqrt(al) * sqrt(be)) {                                                                        \
            const double ze = (be - al) / (2.0 * ga);                                                                                           \
            const double tn = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));                                                      \
            const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;                                                                          \
            double a, b;                                                                                                                        \
            a = G[p]; b = G[q]; G[p] = cs * a - sn * b; G[q] = sn * a + cs * b;                                                                 \
            a = G[3 + p]; b = G[3 + q]; G[3 + p] = cs * a - sn * b; G[3 + q] = sn * a + cs * b;                                                 \
            a = G[6 + p]; b = G[6 + q]; G[6 + p] = cs * a - sn * b; G[6 + q] = sn * a + cs * b;                                                 \
            a = V[p]; b = V[q]; V[p] = cs * a - sn * b; V[q] = sn * a + cs * b;                                                                 \
            a = V[3 + p]; b = V[3 + q]; V[3 + p] = cs * a - sn * b; V[3 + q] = sn * a + cs * b;                                                 \
            a = V[6 + p]; b = V[6 + q]; V[6 + p] = cs * a - sn * b; V[6 + q] = sn * a + cs * b;                                                 \
            rotated = true;                                                                                                                     \
        }                                                                                                                                       \
    }
// swap columns p, q of G and V, and their norms, when column q is the longer one
#define TRAJ_SORT_PAIR(p, q, dp, dq)                                                                                                            \
    if (dq > dp) {                                                                                                                              \
        double s_;                                                                                                                              \
        s_ = dp; dp = dq; dq = s_;                                                                                                              \
        s_ = G[p]; G[p] = G[q]; G[q] = s_; s_ = G[3 + p]; G[3 + p] = G[3 + q]; G[3 + q] = s_; s_ = G[6 + p]; G[6 + p] = G[6 + q]; G[6 + q] = s_; \
        s_ = V[p]; V[p] = V[q]; V[q] = s_; s_ = V[3 + p]; V[3 + p] = V[3 + q]; V[3 + q] = s_; s_ = V[6 + p]; V[6 + p] = V[6 + q]; V[6 + q] = s_; \
    }

// C = U diag(d) V^T with d0 >= d1 >= d2 >= 0.  U's first two columns are the normalised columns of C V; its third is ALWAYS their cross product
// (which also completes a null column), so det(U) = +1 by construction; where the third column of C V points the other way, column 3 of V is negated
// instead — the same factorisation.  Only meaningful where d1 > 0 (the caller's rank rule); U is the identity otherwise.
TRAJ_HD void svd3(const double C[9], double U[9], double d[3], double V[9]) {
    double G[9];
    G[0] = C[0]; G[1] = C[1]; G[2] = C[2]; G[3] = C[3]; G[4] = C[4]; G[5] = C[5]; G[6] = C[6]; G[7] = C[7]; G[8] = C[8];
    V[0] = 1; V[1] = 0; V[2] = 0; V[3] = 0; V[4] = 1; V[5] = 0; V[6] = 0; V[7] = 0; V[8] = 1;
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        bool rotated = false;
        TRAJ_JACOBI_PAIR(0, 1)
        TRAJ_JACOBI_PAIR(0, 2)
        TRAJ_JACOBI_PAIR(1, 2)
        if (!rotated) break;
    }
    double d0 = sqrt(G[0] * G[0] + G[3] * G[3] + G[6] * G[6]);
    double d1 = sqrt(G[1] * G[1] + G[4] * G[4] + G[7] * G[7]);
    double d2 = sqrt(G[2] * G[2] + G[5] * G[5] + G[8] * G[8]);
    TRAJ_SORT_PAIR(0, 1, d0, d1)
    TRAJ_SORT_PAIR(1, 2, d1, d2)
    TRAJ_SORT_PAIR(0, 1, d0, d1)
    d[0] = d0; d[1] = d1; d[2] = d2;
    if (!(d1 > 0.0)) {
        U[0] = 1; U[1] = 0; U[2] = 0; U[3] = 0; U[4] = 1; U[5] = 0; U[6] = 0; U[7] = 0; U[8] = 1;
        return;
    }
    const double i0 = 1.0 / d0, i1 = 1.0 / d1;
    U[0] = G[0] * i0; U[3] = G[3] * i0; U[6] = G[6] * i0;
    U[1] = G[1] * i1; U[4] = G[4] * i1; U[7] = G[7] * i1;
    U[2] = U[3] * U[7] - U[6] * U[4];
    U[5] = U[6] * U[1] - U[0] * U[7];
    U[8] = U[0] * U[4] - U[3] * U[1];
    if (G[2] * U[2] + G[5] * U[5] + G[8] * U[8] < 0.0) {
        V[2] = -V[2]; V[5] = -V[5]; V[8] = -V[8];
    }
}
#undef TRAJ_JACOBI_PAIR
#undef TRAJ_SORT_PAIR

TRAJ_HD double det3(const double A[9]) {
    return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// evo's umeyama_alignment after the sums: C = (1/n) sum (y - mu_y)(x - mu_x)^T, sigma_x = (1/n) sum ||x - mu_x||^2, x = estimate, y = reference.
// Returns false where fewer than 2 singular values exceed DBL_EPSILON (absolute, as evo writes it: it raises there); d is filled either way.
TRAJ_HD bool umeyama_tail(const double C[9], double sigma_x, const double mu_x[3], const double mu_y[3], bool with_scale, Rt& A, double& c,
                          double d[3]) {
    double U[9], V[9];
    svd3(C, U, d, V);
    const int rank = (d[0] > DBL_EPSILON ? 1 : 0) + (d[1] > DBL_EPSILON ? 1 : 0) + (d[2] > DBL_EPSILON ? 1 : 0);
    if (rank < 2) return false;
    const double s2 = det3(V) < 0.0 ? -1.0 : 1.0;    // S = diag(1, 1, s2), s2 = sign(det U det V^T): svd3 makes det U = +1, det(V) = det(V^T)
    // R = U S V^T
    const double u2[3] = {U[2] * s2, U[5] * s2, U[8] * s2};
    A.R[0] = U[0] * V[0] + U[1] * V[1] + u2[0] * V[2];
    A.R[1] = U[0] * V[3] + U[1] * V[4] + u2[0] * V[5];
    A.R[2] = U[0] * V[6] + U[1] * V[7] + u2[0] * V[8];
    A.R[3] = U[3] * V[0] + U[4] * V[1] + u2[1] * V[2];
    A.R[4] = U[3] * V[3] + U[4] * V[4] + u2[1] * V[5];
    A.R[5] = U[3] * V[6] + U[4] * V[7] + u2[1] * V[8];
    A.R[6] = U[6] * V[0] + U[7] * V[1] + u2[2] * V[2];
    A.R[7] = U[6] * V[3] + U[7] * V[4] + u2[2] * V[5];
    A.R[8] = U[6] * V[6] + U[7] * V[7] + u2[2] * V[8];
    c = with_scale ? (d[0] + d[1] + s2 * d[2]) / sigma_x : 1.0;
    double v[3];
    mat3_vec(A.R, mu_x, v);
    A.t[0] = mu_y[0] - c * v[0]; A.t[1] = mu_y[1] - c * v[1]; A.t[2] = mu_y[2] - c * v[2];
    return true;
}

// evo's align_origin branch on the (already scaled) estimate: A = Q_0 P_0^-1
TRAJ_HD void origin_transform(const Rt& P0, double c, const Rt& Q0, Rt& A) {
    Rt Ps = P0, Pi;
    Ps.t[0] *= c; Ps.t[1] *= c; Ps.t[2] *= c;
    inverse(Ps, Pi);
    compose(Q0, Pi, A);
}

}  // namespace traj
