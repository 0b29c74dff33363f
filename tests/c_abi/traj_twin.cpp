// TEST INFRASTRUCTURE: host replay of traj_eval_kernel (mac-vo_amd/csrc/traj_eval.hip) for ONE lane.  It includes the kernel's own arithmetic header
// (csrc/traj_math.h) and repeats the kernel's five passes with the kernel's reduction order: traj::THREADS strided partials, a 64-lane xor butterfly per
// wave, the wave totals added in wave order.  Built by tests/traj_twin.py with g++ -ffp-contract=off.  The product never builds or loads it.
#include <vector>

#include "../../mac-vo_amd/csrc/traj_math.h"

namespace {

constexpr int WAVE = 64;
constexpr int WAVES = traj::THREADS / WAVE;

// common.h's wave_sum: v += shfl_xor(v, o) for o = 32 ... 1 — every lane ends with the same total; then the four totals in wave order
double block_sum(const double* part) {
    double w[WAVES];
    for (int wv = 0; wv < WAVES; ++wv) {
        double v[WAVE], nv[WAVE];
        for (int i = 0; i < WAVE; ++i) v[i] = part[wv * WAVE + i];
        for (int o = 32; o > 0; o >>= 1) {
            for (int i = 0; i < WAVE; ++i) nv[i] = v[i] + v[i ^ o];
            for (int i = 0; i < WAVE; ++i) v[i] = nv[i];
        }
        w[wv] = v[0];
    }
    double s = w[0];
    for (int j = 1; j < WAVES; ++j) s += w[j];
    return s;
}

void load_pose(const void* base, int f64, int64_t stride, int i, double p[7]) {
    if (f64) {
        const double* r = (const double*)base + (int64_t)i * stride;
        for (int k = 0; k < 7; ++k) p[k] = r[k];
    } else {
        const float* r = (const float*)base + (int64_t)i * stride;
        for (int k = 0; k < 7; ++k) p[k] = (double)r[k];
    }
}

struct Lane {
    const void *est, *ref;
    int est_f64, ref_f64;
    int64_t est_stride, ref_stride;
    int T;
};

void pose_errors(const Lane& a, int i, const traj::Rt& A, double c, double e[4]) {
    double p[7], q[7];
    traj::Rt Pi, Qi;
    load_pose(a.est, a.est_f64, a.est_stride, i, p);
    load_pose(a.ref, a.ref_f64, a.ref_stride, i, q);
    traj::pose_to_rt(p, Pi);
    traj::pose_to_rt(q, Qi);
    e[0] = traj::ate_error(A, c, Pi.t, Qi.t);
    e[1] = e[2] = e[3] = 0.0;
    if (i + 1 < a.T) {
        traj::Rt Pj, Qj;
        load_pose(a.est, a.est_f64, a.est_stride, i + 1, p);
        load_pose(a.ref, a.ref_f64, a.ref_stride, i + 1, q);
        traj::pose_to_rt(p, Pj);
        traj::pose_to_rt(q, Qj);
        traj::rel_errors(Pi, Pj, Qi, Qj, c, e[1], e[2], e[3]);
    }
}

}  // namespace

// row: double [MV_EVAL_TRAJ_COLS]; err (or null): double [4][err_stride]
extern "C" int traj_twin_lane(const void* est, const void* ref, int T, int est_f64, int ref_f64, int64_t est_stride, int64_t ref_stride, int align,
                              int correct_scale, double* row, double* err, int64_t err_stride) {
    if (T < 0 || T > MV_EVAL_TRAJ_MAX_POSES || est_stride < 7 || ref_stride < 7 || (err && err_stride < T)) return MV_ERR_INVALID_ARG;
    const Lane a{est, ref, est_f64, ref_f64, est_stride, ref_stride, T};
    const int N = traj::THREADS;
    const double qnan = NAN;
    std::vector<double> part(12 * N, 0.0);
    auto P = [&](int k) { return part.data() + k * N; };
    auto clear = [&]() { for (auto& x : part) x = 0.0; };

    // pass 1
    int bad = 0;
    for (int tid = 0; tid < N; ++tid)
        for (int i = tid; i < T; i += N) {
            double p[7], q[7];
            load_pose(est, est_f64, est_stride, i, p);
            load_pose(ref, ref_f64, ref_stride, i, q);
            for (int k = 0; k < 7; ++k) bad |= (int)!(fabs(p[k]) <= DBL_MAX) | (int)!(fabs(q[k]) <= DBL_MAX);
            for (int k = 0; k < 3; ++k) {
                P(k)[tid] += p[k];
                P(3 + k)[tid] += q[k];
            }
        }
    int status = T < 2 ? MV_TRAJ_TOO_SHORT : bad ? MV_TRAJ_NONFINITE : MV_TRAJ_OK;
    const double n = (double)T;
    double mu[6];
    for (int k = 0; k < 6; ++k) mu[k] = block_sum(P(k)) / n;

    // pass 2
    const bool need = align == MV_TRAJ_ALIGN_UMEYAMA || correct_scale;
    clear();
    if (status == MV_TRAJ_OK && need)
        for (int tid = 0; tid < N; ++tid)
            for (int i = tid; i < T; i += N) {
                double p[7], q[7];
                load_pose(est, est_f64, est_stride, i, p);
                load_pose(ref, ref_f64, ref_stride, i, q);
                const double x0 = p[0] - mu[0], x1 = p[1] - mu[1], x2 = p[2] - mu[2];
                const double y0 = q[0] - mu[3], y1 = q[1] - mu[4], y2 = q[2] - mu[5];
                P(0)[tid] += y0 * x0; P(1)[tid] += y0 * x1; P(2)[tid] += y0 * x2;
                P(3)[tid] += y1 * x0; P(4)[tid] += y1 * x1; P(5)[tid] += y1 * x2;
                P(6)[tid] += y2 * x0; P(7)[tid] += y2 * x1; P(8)[tid] += y2 * x2;
                P(9)[tid] += (x0 * x0 + x1 * x1) + x2 * x2;
            }
    double s2[10];
    for (int k = 0; k < 10; ++k) s2[k] = block_sum(P(k));

    // pass 3
    traj::Rt A;
    traj::identity(A);
    double c = 1.0, d[3] = {qnan, qnan, qnan};
    if (status == MV_TRAJ_OK) {
        traj::Rt Au;
        traj::identity(Au);
        if (need) {
            double C[9];
            for (int k = 0; k < 9; ++k) C[k] = s2[k] / n;
            if (!traj::umeyama_tail(C, s2[9] / n, mu, mu + 3, correct_scale != 0, Au, c, d)) status = MV_TRAJ_DEGENERATE;
        }
        if (status == MV_TRAJ_OK) {
            if (align == MV_TRAJ_ALIGN_UMEYAMA) {
                A = Au;
            } else if (align == MV_TRAJ_ALIGN_ORIGIN) {
                double p[7], q[7];
                traj::Rt P0, Q0;
                load_pose(est, est_f64, est_stride, 0, p);
                load_pose(ref, ref_f64, ref_stride, 0, q);
                traj::pose_to_rt(p, P0);
                traj::pose_to_rt(q, Q0);
                traj::origin_transform(P0, c, Q0, A);
            }
        }
    }
    for (int k = 0; k < MV_EVAL_TRAJ_COLS; ++k) row[k] = qnan;
    row[MV_EVAL_TRAJ_N_POSES] = n;
    row[MV_EVAL_TRAJ_N_PAIRS] = (double)(T > 0 ? T - 1 : 0);
    row[MV_EVAL_TRAJ_STATUS] = (double)status;
    row[MV_EVAL_TRAJ_D1] = d[0]; row[MV_EVAL_TRAJ_D2] = d[1]; row[MV_EVAL_TRAJ_D3] = d[2];
    if (status != MV_TRAJ_OK) {
        if (err)
            for (int m = 0; m < 4; ++m)
                for (int i = 0; i < T; ++i) err[m * err_stride + i] = qnan;
        return MV_OK;
    }

    // pass 4
    clear();
    for (int tid = 0; tid < N; ++tid)
        for (int i = tid; i < T; i += N) {
            double e[4];
            pose_errors(a, i, A, c, e);
            for (int m = 0; m < 4; ++m) {
                P(m)[tid] += e[m];
                P(4 + m)[tid] += e[m] * e[m];
            }
            if (err) {
                err[i] = e[0];
                if (i + 1 < T)
                    for (int m = 1; m < 4; ++m) err[m * err_stride + i] = e[m];
            }
        }
    double s4[8];
    for (int k = 0; k < 8; ++k) s4[k] = block_sum(P(k));
    const double np = (double)(T - 1);
    double mean[4] = {s4[0] / n, s4[1] / np, s4[2] / np, s4[3] / np};

    // pass 5
    clear();
    for (int tid = 0; tid < N; ++tid)
        for (int i = tid; i < T; i += N) {
            double e[4];
            pose_errors(a, i, A, c, e);
            const double d0 = e[0] - mean[0];
            P(0)[tid] += d0 * d0;
            if (i + 1 < T)
                for (int m = 1; m < 4; ++m) {
                    const double dm = e[m] - mean[m];
                    P(m)[tid] += dm * dm;
                }
        }
    for (int m = 0; m < 4; ++m) {
        const double cnt = m == 0 ? n : np;
        row[MV_EVAL_TRAJ_ATE_MEAN + 3 * m] = mean[m];
        row[MV_EVAL_TRAJ_ATE_STD + 3 * m] = sqrt(block_sum(P(m)) / cnt);
        row[MV_EVAL_TRAJ_ATE_RMSE + 3 * m] = sqrt(s4[4 + m] / cnt);
    }
    for (int k = 0; k < 9; ++k) row[MV_EVAL_TRAJ_R00 + k] = A.R[k];
    row[MV_EVAL_TRAJ_TX] = A.t[0]; row[MV_EVAL_TRAJ_TY] = A.t[1]; row[MV_EVAL_TRAJ_TZ] = A.t[2];
    row[MV_EVAL_TRAJ_SCALE] = c;
    return MV_OK;
}

// the SVD alone, for the CPU suite: C row-major -> U, d, V (C = U diag(d) V^T)
extern "C" void traj_twin_svd3(const double* C, double* U, double* d, double* V) { traj::svd3(C, U, d, V); }
