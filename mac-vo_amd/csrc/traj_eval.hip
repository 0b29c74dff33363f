// Trajectory evaluation (Evaluation/MetricsSeq.py:9-51, Evaluation/EvalSeq.py:53-64; evo 1.x restated, unpinned): ATE / RTE / ROE / RPE of up to
// MV_MAX_LANES time-associated tracks in ONE launch, one workgroup per lane.  Nothing passes between workgroups: no atomic, no counter, no wait.
// The arithmetic is traj_math.h; this file is the five passes over a lane's poses and their fixed-order fp64 sums.
//
//   pass 1  finiteness of every coordinate, the two position sums          -> mu_x, mu_y
//   pass 2  centred C = (1/n) sum (y - mu_y)(x - mu_x)^T and sigma_x       (centred first: tracks sit kilometres from the origin; Umeyama only)
//   pass 3  one thread: Jacobi SVD, R, t, c (or Q_0 P_0^-1), status        -> LDS, read by everyone
//   pass 4  the four error values per pose / pair, their sums and squares  -> mean, rmse
//   pass 5  the same values again, centred squares                         -> std (two passes, as np.std)
//
// A sum is: per-thread partial over i = tid, tid + 256, ... (ascending), wave_sum butterfly, the four wave totals added in wave order.  Its order
// depends on T alone, so a lane's row has the same bits alone, batched and at any lane index.  Pass 5 recomputes the errors instead of keeping them
// (T is up to 2^20 per lane; the poses are L2-resident after pass 1): the same instructions on the same inputs, so the same values.
#include "common.h"
#include "traj_math.h"

namespace {

constexpr int TRAJ_WAVES = traj::THREADS / MV_WAVE;

struct TrajArgs {
    const void* est[MV_MAX_LANES];
    const void* ref[MV_MAX_LANES];
    int32_t T[MV_MAX_LANES];
    int64_t est_stride, ref_stride;   // elements between rows
    int est_f64, ref_f64;
    int align, correct_scale;
    double* rows;                     // [lanes][MV_EVAL_TRAJ_COLS]
    double* err_out;                  // [lanes][4][err_stride] or null
    int64_t err_stride;
};

struct TrajShared {
    double part[TRAJ_WAVES][12];
    traj::Rt A;
    double c, d[3];
    int status;
    int bad[TRAJ_WAVES];
};

__device__ __forceinline__ void load_pose(const void* base, int f64, int64_t stride, int i, double p[7]) {
    if (f64) {
        const double* r = (const double*)base + (int64_t)i * stride;
#pragma unroll
        for (int k = 0; k < 7; ++k) p[k] = r[k];
    } else {
        const float* r = (const float*)base + (int64_t)i * stride;
#pragma unroll
        for (int k = 0; k < 7; ++k) p[k] = (double)r[k];
    }
}

// N sums at once: v[k] <- the workgroup's total of v[k], the same bits in every thread
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], TrajShared& sh) {
    static_assert(N <= 12, "TrajShared::part");
    const int lane = threadIdx.x & (MV_WAVE - 1), w = threadIdx.x / MV_WAVE;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) sh.part[w][k] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double s = sh.part[0][k];
#pragma unroll
        for (int j = 1; j < TRAJ_WAVES; ++j) s += sh.part[j][k];
        v[k] = s;
    }
    __syncthreads();
}

// the four error values of index i: e[0] = ATE_i (i < T), e[1..3] = RTE / ROE / RPE of the pair (i, i + 1) (i < T - 1)
__device__ __forceinline__ void pose_errors(const TrajArgs& a, const void* est, const void* ref, int T, int i, const traj::Rt& A, double c, double e[4]) {
    double p[7], q[7];
    traj::Rt Pi, Qi;
    load_pose(est, a.est_f64, a.est_stride, i, p);
    load_pose(ref, a.ref_f64, a.ref_stride, i, q);
    traj::pose_to_rt(p, Pi);
    traj::pose_to_rt(q, Qi);
    e[0] = traj::ate_error(A, c, Pi.t, Qi.t);
    e[1] = e[2] = e[3] = 0.0;
    if (i + 1 < T) {
        traj::Rt Pj, Qj;
        load_pose(est, a.est_f64, a.est_stride, i + 1, p);
        load_pose(ref, a.ref_f64, a.ref_stride, i + 1, q);
        traj::pose_to_rt(p, Pj);
        traj::pose_to_rt(q, Qj);
        traj::rel_errors(Pi, Pj, Qi, Qj, c, e[1], e[2], e[3]);
    }
}

__global__ void __launch_bounds__(traj::THREADS) traj_eval_kernel(const TrajArgs a) {
    __shared__ TrajShared sh;
    const int l = blockIdx.x, tid = threadIdx.x;
    const int T = a.T[l];
    const void* est = a.est[l];
    const void* ref = a.ref[l];
    double* row = a.rows + (int64_t)l * MV_EVAL_TRAJ_COLS;
    double* err = a.err_out ? a.err_out + (int64_t)l * 4 * a.err_stride : nullptr;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    // ---- pass 1: finiteness, position sums (T is uniform over the workgroup, so is every branch on it: the barriers below are reached by all)
    double s1[6] = {0, 0, 0, 0, 0, 0};
    int bad = 0;
    for (int i = tid; i < T; i += traj::THREADS) {
        double p[7], q[7];
        load_pose(est, a.est_f64, a.est_stride, i, p);
        load_pose(ref, a.ref_f64, a.ref_stride, i, q);
#pragma unroll
        for (int k = 0; k < 7; ++k) bad |= (int)!(fabs(p[k]) <= DBL_MAX) | (int)!(fabs(q[k]) <= DBL_MAX);
        s1[0] += p[0]; s1[1] += p[1]; s1[2] += p[2];
        s1[3] += q[0]; s1[4] += q[1]; s1[5] += q[2];
    }
    bad = __any(bad);
    if ((tid & (MV_WAVE - 1)) == 0) sh.bad[tid / MV_WAVE] = bad;
    block_sum(s1, sh);           // (its first barrier also publishes sh.bad)
    bad = 0;
#pragma unroll
    for (int j = 0; j < TRAJ_WAVES; ++j) bad |= sh.bad[j];

    int status = T < 2 ? MV_TRAJ_TOO_SHORT : bad ? MV_TRAJ_NONFINITE : MV_TRAJ_OK;
    const double n = (double)T;
    double mu[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) mu[k] = s1[k] / n;

    // ---- pass 2: centred covariance and sigma_x — only where Umeyama is asked for (ORIGIN / NONE without correct_scale skip it and pass 3's SVD)
    const bool need = a.align == MV_TRAJ_ALIGN_UMEYAMA || a.correct_scale;
    double s2[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (status == MV_TRAJ_OK && need) {
        for (int i = tid; i < T; i += traj::THREADS) {
            double p[7], q[7];
            load_pose(est, a.est_f64, a.est_stride, i, p);
            load_pose(ref, a.ref_f64, a.ref_stride, i, q);
            const double x0 = p[0] - mu[0], x1 = p[1] - mu[1], x2 = p[2] - mu[2];
            const double y0 = q[0] - mu[3], y1 = q[1] - mu[4], y2 = q[2] - mu[5];
            s2[0] += y0 * x0; s2[1] += y0 * x1; s2[2] += y0 * x2;
            s2[3] += y1 * x0; s2[4] += y1 * x1; s2[5] += y1 * x2;
            s2[6] += y2 * x0; s2[7] += y2 * x1; s2[8] += y2 * x2;
            s2[9] += (x0 * x0 + x1 * x1) + x2 * x2;
        }
    }
    block_sum(s2, sh);

    // ---- pass 3: the alignment, on one thread
    if (tid == 0) {
        traj::Rt A;
        traj::identity(A);
        double c = 1.0, d[3] = {qnan, qnan, qnan};
        if (status == MV_TRAJ_OK) {
            traj::Rt Au;
            traj::identity(Au);
            if (need) {
                double C[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) C[k] = s2[k] / n;
                if (!traj::umeyama_tail(C, s2[9] / n, mu, mu + 3, a.correct_scale != 0, Au, c, d)) status = MV_TRAJ_DEGENERATE;
            }
            if (status == MV_TRAJ_OK) {
                if (a.align == MV_TRAJ_ALIGN_UMEYAMA) {
                    A = Au;
                } else if (a.align == MV_TRAJ_ALIGN_ORIGIN) {
                    double p[7], q[7];
                    traj::Rt P0, Q0;
                    load_pose(est, a.est_f64, a.est_stride, 0, p);
                    load_pose(ref, a.ref_f64, a.ref_stride, 0, q);
                    traj::pose_to_rt(p, P0);
                    traj::pose_to_rt(q, Q0);
                    traj::origin_transform(P0, c, Q0, A);
                }
            }
        }
        sh.A = A;
        sh.c = c;
        sh.d[0] = d[0]; sh.d[1] = d[1]; sh.d[2] = d[2];
        sh.status = status;
    }
    __syncthreads();
    status = sh.status;
    const traj::Rt A = sh.A;
    const double c = sh.c;

    if (status != MV_TRAJ_OK) {
        if (tid < MV_EVAL_TRAJ_COLS) {
            double v = qnan;
            if (tid >= MV_EVAL_TRAJ_D1 && tid <= MV_EVAL_TRAJ_D3) v = sh.d[tid - MV_EVAL_TRAJ_D1];
            if (tid == MV_EVAL_TRAJ_N_POSES) v = (double)T;
            if (tid == MV_EVAL_TRAJ_N_PAIRS) v = (double)(T > 0 ? T - 1 : 0);
            if (tid == MV_EVAL_TRAJ_STATUS) v = (double)status;
            row[tid] = v;
        }
        if (err) {
            for (int i = tid; i < T; i += traj::THREADS) {
#pragma unroll
                for (int m = 0; m < 4; ++m) err[m * a.err_stride + i] = qnan;
            }
        }
        return;
    }

    // ---- pass 4: errors, sums and sums of squares
    double s4[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < T; i += traj::THREADS) {
        double e[4];
        pose_errors(a, est, ref, T, i, A, c, e);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            s4[m] += e[m];
            s4[4 + m] += e[m] * e[m];
        }
        if (err) {
            err[i] = e[0];
            if (i + 1 < T) {
                err[a.err_stride + i] = e[1];
                err[2 * a.err_stride + i] = e[2];
                err[3 * a.err_stride + i] = e[3];
            }
        }
    }
    block_sum(s4, sh);
    const double np = (double)(T - 1);
    double mean[4];
    mean[0] = s4[0] / n;
#pragma unroll
    for (int m = 1; m < 4; ++m) mean[m] = s4[m] / np;

    // ---- pass 5: centred squares
    double s5[4] = {0, 0, 0, 0};
    for (int i = tid; i < T; i += traj::THREADS) {
        double e[4];
        pose_errors(a, est, ref, T, i, A, c, e);
        const double d0 = e[0] - mean[0];
        s5[0] += d0 * d0;
        if (i + 1 < T) {
#pragma unroll
            for (int m = 1; m < 4; ++m) {
                const double dm = e[m] - mean[m];
                s5[m] += dm * dm;
            }
        }
    }
    block_sum(s5, sh);

    if (tid == 0) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const double cnt = m == 0 ? n : np;
            row[MV_EVAL_TRAJ_ATE_MEAN + 3 * m] = mean[m];
            row[MV_EVAL_TRAJ_ATE_STD + 3 * m] = sqrt(s5[m] / cnt);
            row[MV_EVAL_TRAJ_ATE_RMSE + 3 * m] = sqrt(s4[4 + m] / cnt);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) row[MV_EVAL_TRAJ_R00 + k] = A.R[k];
        row[MV_EVAL_TRAJ_TX] = A.t[0]; row[MV_EVAL_TRAJ_TY] = A.t[1]; row[MV_EVAL_TRAJ_TZ] = A.t[2];
        row[MV_EVAL_TRAJ_SCALE] = c;
        row[MV_EVAL_TRAJ_D1] = sh.d[0]; row[MV_EVAL_TRAJ_D2] = sh.d[1]; row[MV_EVAL_TRAJ_D3] = sh.d[2];
        row[MV_EVAL_TRAJ_N_POSES] = n;
        row[MV_EVAL_TRAJ_N_PAIRS] = np;
        row[MV_EVAL_TRAJ_STATUS] = (double)MV_TRAJ_OK;
    }
}

}  // namespace

extern "C" int mv_eval_traj_lanes(int lanes, const void* const* est, const void* const* ref, const int32_t* T, int est_dtype, int ref_dtype,
                                  int64_t est_row_stride, int64_t ref_row_stride, int align, int correct_scale, double* rows, double* err_out,
                                  int64_t err_stride, mvStream_t stream) {
    MV_CHECK_ARG(lanes >= 1 && lanes <= MV_MAX_LANES && est && ref && T && rows);
    MV_CHECK_ARG((est_dtype == MV_TRAJ_F32 || est_dtype == MV_TRAJ_F64) && (ref_dtype == MV_TRAJ_F32 || ref_dtype == MV_TRAJ_F64));
    MV_CHECK_ARG(est_row_stride >= 7 && ref_row_stride >= 7);
    MV_CHECK_ARG(align == MV_TRAJ_ALIGN_UMEYAMA || align == MV_TRAJ_ALIGN_ORIGIN || align == MV_TRAJ_ALIGN_NONE);
    TrajArgs a;
    for (int l = 0; l < lanes; ++l) {
        MV_CHECK_ARG(T[l] >= 0 && T[l] <= MV_EVAL_TRAJ_MAX_POSES);
        MV_CHECK_ARG(T[l] == 0 || (est[l] && ref[l]));
        MV_CHECK_ARG(!err_out || err_stride >= T[l]);
        a.est[l] = est[l];
        a.ref[l] = ref[l];
        a.T[l] = T[l];
    }
    for (int l = lanes; l < MV_MAX_LANES; ++l) {
        a.est[l] = a.ref[l] = nullptr;
        a.T[l] = 0;
    }
    a.est_stride = est_row_stride;
    a.ref_stride = ref_row_stride;
    a.est_f64 = est_dtype == MV_TRAJ_F64;
    a.ref_f64 = ref_dtype == MV_TRAJ_F64;
    a.align = align;
    a.correct_scale = correct_scale != 0;
    a.rows = rows;
    a.err_out = err_out;
    a.err_stride = err_stride;
    hipLaunchKernelGGL(traj_eval_kernel, dim3(lanes), dim3(traj::THREADS), 0, (hipStream_t)stream, a);
    return mv_launch_status();
}
