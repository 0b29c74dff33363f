// Trajectory time association (Utility/Trajectory.py:105-114: align_origin, the two clock rebases, align_time; :172-176 align_time ->
// Utility/Math.py:96-121 interpolate_pose; :188-191 align_origin — evo restated, unpinned): the step Evaluation/EvalSeq.py:36 runs before it scores a
// track, for up to MV_MAX_LANES tracks in ONE launch.  The arithmetic is se3_interp.h; this file is the launch shape.
//
//   grid (ceil(max Q / 256), lanes): the lane in blockIdx.y, one query per thread, per-lane pointers and lengths by value in the kernel argument.
//
// The lane-wide checks (sorted stamps, finite stamps / rows / origin row) are REPEATED by every workgroup of the lane: each scans the lane's T stamps and
// rows and Q query stamps (L2-resident after the first workgroup) and arrives at the same verdict on its own.  The alternatives are a second launch, or
// a hand-over between workgroups (a counter and a wait, or a flag written by workgroup 0 that the others cannot wait for without one); repeating the
// scan costs T / 256 loads per thread and keeps the launch free of atomics, counters and waits: nothing passes between workgroups, a lane's output
// depends on that lane's inputs alone, and its bits are the same alone, batched and at any lane index.  Workgroup 0 of a lane writes the status.
#include "common.h"
#include "se3_interp.h"

namespace {

constexpr int ASSOC_THREADS = 256;

struct AssocArgs {
    const void* src[MV_MAX_LANES];
    const void* ts[MV_MAX_LANES];
    const void* tq[MV_MAX_LANES];
    const void* origin[MV_MAX_LANES];
    void* out[MV_MAX_LANES];
    uint8_t* flag[MV_MAX_LANES];
    int32_t T[MV_MAX_LANES], Q[MV_MAX_LANES];
    int32_t* status;
    int64_t src_stride;
    int32_t src_f64, time_i64, origin_f64, out_f64, rebase;
};
static_assert(sizeof(AssocArgs) <= 4096, "kernel arguments");

__global__ void __launch_bounds__(ASSOC_THREADS) traj_assoc_kernel(const AssocArgs a) {
    const int l = blockIdx.y, tid = threadIdx.x;
    se3i::AssocLane ln;
    ln.src = a.src[l]; ln.ts = a.ts[l]; ln.tq = a.tq[l]; ln.origin = a.origin[l];
    ln.T = a.T[l]; ln.Q = a.Q[l];
    ln.src_stride = a.src_stride;
    ln.src_f64 = a.src_f64; ln.time_i64 = a.time_i64; ln.origin_f64 = a.origin_f64; ln.rebase = a.rebase;
    if ((int64_t)blockIdx.x * ASSOC_THREADS >= ln.Q && blockIdx.x != 0) return;   // (uniform over the workgroup: the barrier below is reached by all or none)

    int bad = 0;
    const int n = ln.T > ln.Q ? ln.T : ln.Q;
    for (int i = tid; i < n; i += ASSOC_THREADS) bad |= se3i::assoc_check(ln, i);
    const int nonfinite = __syncthreads_or(bad & se3i::ASSOC_BAD_NONFINITE);
    const int unsorted = __syncthreads_or(bad & se3i::ASSOC_BAD_UNSORTED);
    const int status = se3i::assoc_status(ln.T, (nonfinite ? se3i::ASSOC_BAD_NONFINITE : 0) | (unsorted ? se3i::ASSOC_BAD_UNSORTED : 0));
    if (blockIdx.x == 0 && tid == 0) a.status[l] = status;

    const int64_t j = (int64_t)blockIdx.x * ASSOC_THREADS + tid;
    if (j >= ln.Q) return;
    double o[7];
    int flag = 0;
    if (status == MV_TRAJ_OK) {
        se3i::Se3d p;
        flag = se3i::assoc_query(ln, (int)j, p);
        o[0] = p.t[0]; o[1] = p.t[1]; o[2] = p.t[2]; o[3] = p.q[0]; o[4] = p.q[1]; o[5] = p.q[2]; o[6] = p.q[3];
    } else {
        const double qnan = __longlong_as_double(0x7ff8000000000000LL);
        o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = o[6] = qnan;
    }
    if (a.out_f64) {
        double* r = (double*)a.out[l] + 7 * j;
#pragma unroll
        for (int k = 0; k < 7; ++k) r[k] = o[k];
    } else {
        float* r = (float*)a.out[l] + 7 * j;
#pragma unroll
        for (int k = 0; k < 7; ++k) r[k] = (float)o[k];   // the one rounding
    }
    a.flag[l][j] = (uint8_t)flag;
}

}  // namespace

extern "C" int mv_traj_associate_lanes(int lanes, const void* const* src, const void* const* src_time, const int32_t* T, const void* const* query_time,
                                       const int32_t* Q, const void* const* origin_ref, int src_dtype, int time_dtype, int origin_dtype, int out_dtype,
                                       int64_t src_row_stride, int rebase, void* const* out_poses, uint8_t* const* out_extrapolated, int32_t* status,
                                       mvStream_t stream) {
    MV_CHECK_ARG(lanes >= 1 && lanes <= MV_MAX_LANES && src && src_time && T && query_time && Q && out_poses && out_extrapolated && status);
    MV_CHECK_ARG((src_dtype == MV_TRAJ_F32 || src_dtype == MV_TRAJ_F64) && (out_dtype == MV_TRAJ_F32 || out_dtype == MV_TRAJ_F64));
    MV_CHECK_ARG(origin_dtype == MV_TRAJ_F32 || origin_dtype == MV_TRAJ_F64);
    MV_CHECK_ARG(time_dtype == MV_TRAJ_TIME_F64 || time_dtype == MV_TRAJ_TIME_I64);
    MV_CHECK_ARG(src_row_stride >= 7);
    AssocArgs a;
    int q_max = 0;
    for (int l = 0; l < lanes; ++l) {
        MV_CHECK_ARG(T[l] >= 0 && T[l] <= MV_EVAL_TRAJ_MAX_POSES && Q[l] >= 0 && Q[l] <= MV_EVAL_TRAJ_MAX_POSES);
        MV_CHECK_ARG(T[l] == 0 || (src[l] && src_time[l]));
        MV_CHECK_ARG(Q[l] == 0 || (query_time[l] && out_poses[l] && out_extrapolated[l]));
        a.src[l] = src[l];
        a.ts[l] = src_time[l];
        a.tq[l] = query_time[l];
        a.origin[l] = origin_ref && T[l] > 0 ? origin_ref[l] : nullptr;
        a.out[l] = out_poses[l];
        a.flag[l] = out_extrapolated[l];
        a.T[l] = T[l];
        a.Q[l] = Q[l];
        q_max = Q[l] > q_max ? Q[l] : q_max;
    }
    for (int l = lanes; l < MV_MAX_LANES; ++l) {
        a.src[l] = a.ts[l] = a.tq[l] = a.origin[l] = nullptr;
        a.out[l] = nullptr;
        a.flag[l] = nullptr;
        a.T[l] = a.Q[l] = 0;
    }
    a.status = status;
    a.src_stride = src_row_stride;
    a.src_f64 = src_dtype == MV_TRAJ_F64;
    a.time_i64 = time_dtype == MV_TRAJ_TIME_I64;
    a.origin_f64 = origin_dtype == MV_TRAJ_F64;
    a.out_f64 = out_dtype == MV_TRAJ_F64;
    a.rebase = rebase != 0;
    const int gx = q_max > 0 ? mv_ceil_div(q_max, ASSOC_THREADS) : 1;
    hipLaunchKernelGGL(traj_assoc_kernel, dim3(gx, lanes), dim3(ASSOC_THREADS), 0, (hipStream_t)stream, a);
    return mv_launch_status();
}
