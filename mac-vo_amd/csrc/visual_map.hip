// SURVEY §8(f) rank 4 — device-resident VisualMap: per-frame registration, output poses, MotionInterpolate
//
// Replaces, for the tracking map of one sequence:
//   Module/Map/VisualMap.py:15-133 (SoA stores frames / points / match + six edge tables) and Module/Map/Graph.py:19-298
//   (TensorBundle / AutoScalingBundle.push :86-104, DenseEdge_Multi.add :183-186, SparseEdge_Multi.add :144-147,
//   SingleEdge.set :228-229) as they are driven by Odometry/MACVO.py:158-171 (initialize), :244-311 (run_pair: MatchObs.init,
//   `match_obs[mask]`, points.push(...[mask]), push_keyframe, the six edge updates, the lost-track flag) — the reference does
//   all of it on the CPU after ~25 `.cpu()` copies per frame (MACVO.py:235-266);
//   Odometry/Interface.py:47-49 (body poses T_BS @ pose @ T_BS^-1 written to poses.npy);
//   Module/MapProcessor.py:52-76 (MotionInterpolate.elaborate_map) and :28-49 (PoseInterpolate.elaborate_map) + Utility/Math.py:96-133
//   (interpolate_pose, NormalizeQuat) — the se3 arithmetic of both is csrc/se3_interp.h.
//
// gfx950 design: all of this is a few KB per frame — one workgroup per call.  mv_map_append compacts the frame's kept rows
// (valid mask of mv_obs_filter, order preserved: `bundle[mask]`) with a wave-ballot scan and scatters them into the stores at
// the device-side running counts, so a frame is registered with ZERO host synchronisation and zero D2H copies; the host only
// tracks capacity UPPER bounds (rows pushed <= rows selected).
#include "common.h"
#include <math.h>
#include "se3_interp.h"   // Se3d and the fp64 SE(3) arithmetic MotionInterpolate / PoseInterpolate run on (shared with traj_assoc.hip and a host twin)

namespace {

using namespace se3i;

// ------------------------------------------------------------------------------------------------ registration
// One frame into one map, by one 256-thread workgroup: the body of map_append_kernel (one frame per launch) and of map_append_lanes_kernel (one workgroup per
// lane).  `fr` / `st` are wave-uniform; every row offset comes from st.counts and is checked against the capacities before the first store.
__device__ __forceinline__ void map_append_frame(const mvMapFrame& fr, const mvMapStores& st) {
    __shared__ int wave_cnt[4];
    __shared__ int base_match, base_point, frame_idx;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int64_t* cnt = st.counts;   // {n_frames, n_match, n_points, n_frames_need_interp}
    if (t == 0) {
        frame_idx = (int)cnt[0];
        base_match = (int)cnt[1];
        base_point = (int)cnt[2];
    }
    __syncthreads();
    const int F = frame_idx, M0 = base_match, P0 = base_point;
    // row offsets are device-side state: a caller whose capacity bookkeeping slipped must get an error, not a scribble
    if ((int64_t)F >= st.cap_frames || (int64_t)M0 + fr.n_rows > st.cap_match || (int64_t)P0 + fr.n_rows > st.cap_points) {
        if (t == 0) {
            cnt[4] += 1;
            if (fr.out_frame_idx) fr.out_frame_idx[0] = -1;
        }
        return;
    }
    int kept_total = 0;
    // rows are processed in chunks of 256 so that any n_rows works; order is preserved (== `bundle[mask]`)
    for (int r0 = 0; r0 < fr.n_rows; r0 += 256) {
        const int r = r0 + t;
        const bool keep = r < fr.n_rows && (fr.valid ? fr.valid[r] != 0 : true);
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int before = kept_total;
        for (int w = 0; w < wave; ++w) before += wave_cnt[w];
        const int chunk = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        if (keep) {
            const int k = before + __popcll(bal & ((1ull << lane) - 1ull));
            const size_t m = (size_t)M0 + k, p = (size_t)P0 + k, N = (size_t)fr.table_stride;
            // MatchObs (VisualMap.py:51-69; sources: Odometry/MACVO.py:244-266)
            st.pixel1_uv[2 * m] = fr.kp0[2 * r]; st.pixel1_uv[2 * m + 1] = fr.kp0[2 * r + 1];
            st.pixel2_uv[2 * m] = fr.kp1[2 * r]; st.pixel2_uv[2 * m + 1] = fr.kp1[2 * r + 1];
            st.pixel1_d[m] = fr.vals[0 * N + r];
            st.pixel1_disp[m] = fr.vals[1 * N + r];
            st.pixel1_disp_cov[m] = fr.vals[2 * N + r];
            st.pixel1_d_cov[m] = fr.vals[3 * N + r];
            st.pixel2_d[m] = fr.vals[4 * N + r];
            st.pixel2_disp[m] = fr.vals[5 * N + r];
            st.pixel2_disp_cov[m] = fr.vals[6 * N + r];
            st.pixel2_d_cov[m] = fr.vals[7 * N + r];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                st.pixel1_uv_cov[3 * m + c] = fr.sigma0[3 * r + c];
                st.pixel2_uv_cov[3 * m + c] = fr.sigma1[3 * r + c];
                st.pos_Tw[3 * p + c] = fr.pos_Tw[3 * r + c];
                st.color[3 * p + c] = fr.color ? fr.color[3 * r + c] : (uint8_t)0;
            }
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                st.obs1_covTc[9 * m + c] = fr.cov0[9 * (size_t)r + c];
                st.obs2_covTc[9 * m + c] = fr.cov1[9 * (size_t)r + c];
                st.cov_Tw[9 * p + c] = fr.cov0_world[9 * (size_t)r + c];
            }
            // edges: point -> match (new point: degree 0 -> slot 0), match -> point / frame1 / frame2
            int64_t* pe = st.point2match_edges + p * st.max_pt_obs;
            pe[0] = (int64_t)m;
            for (int c = 1; c < st.max_pt_obs; ++c) pe[c] = -1;
            st.point2match_deg[p] = 1;
            st.match2point[m] = (int64_t)p;
            st.match2frame1[m] = (int64_t)fr.prev_frame;
            st.match2frame2[m] = (int64_t)F;
        }
        kept_total += chunk;
        __syncthreads();
    }
    if (t == 0) {
        // push_keyframe (MACVO.py:339-347): the new frame enters the map at the motion-model prior; the optimised pose is
        // written over it later (write_graph_data, Optimizer.py:104-108)
        const size_t f = (size_t)F;
#pragma unroll
        for (int c = 0; c < 9; ++c) st.K[9 * f + c] = fr.K[c];
        st.baseline[f] = fr.baseline;
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            st.pose[7 * f + c] = fr.prior_pose ? fr.prior_pose[c] : (c == 6 ? 1.f : 0.f);
            st.T_BS[7 * f + c] = fr.T_BS[c];
        }
        st.time_ns[f] = fr.time_ns;
        // lost track (MACVO.py:303-307): fewer than min_num_point observations -> flagged for interpolation
        const bool lost = fr.prev_frame >= 0 && kept_total < fr.min_num_point;
        st.need_interp[f] = lost ? 1 : 0;
        // new frame's edge rows (AutoScalingBundle.push :97-104): no ranges yet
        for (int c = 0; c < 2 * st.max_frame_range; ++c) {
            st.frame2match_ranges[2 * st.max_frame_range * f + c] = -1;
            st.frame2map_ranges[2 * st.max_frame_range * f + c] = -1;
        }
        st.frame2match_num[f] = 0;
        st.frame2map_num[f] = 0;
        if (fr.prev_frame >= 0) {
            // frame2match.add(prev_frame, M0, n); frame2match.add(frame, M0, n)  (MACVO.py:290-291, Graph.py:183-186)
            const size_t pf = (size_t)fr.prev_frame;
            const int64_t np = st.frame2match_num[pf];
            if (np < st.max_frame_range) {
                st.frame2match_ranges[2 * (st.max_frame_range * pf + np)] = M0;
                st.frame2match_ranges[2 * (st.max_frame_range * pf + np) + 1] = kept_total;
                st.frame2match_num[pf] = np + 1;
            } else {
                cnt[4] += 1;   // DenseEdge_Multi.add raises when a frame runs out of range slots (Graph.py:183-186)
            }
            st.frame2match_ranges[2 * st.max_frame_range * f] = M0;
            st.frame2match_ranges[2 * st.max_frame_range * f + 1] = kept_total;
            st.frame2match_num[f] = 1;
        }
        cnt[0] = F + 1;
        cnt[1] = M0 + kept_total;
        cnt[2] = P0 + kept_total;
        if (lost) cnt[3] += 1;
        if (fr.out_frame_idx) fr.out_frame_idx[0] = F;
    }
}

__global__ __launch_bounds__(256) void map_append_kernel(mvMapFrame fr, mvMapStores st) { map_append_frame(fr, st); }

// Lane-batched registration: `lanes` independent sequences, each with its own map, in ONE launch.  The frames' tables are the frame driver's backend buffers
// as they lie ([lanes, cap, .] per keypoint, the value table [11, lanes, cap]); the per-lane host values ride in the kernel arguments; the maps' descriptors
// (~45 pointers each: too many for kernel arguments at 64 lanes) are a device-resident array indexed by the lane.
struct MapLaneFrames {
    int32_t lanes, cap, prev_frame, min_num_point;
    const uint8_t* valid;
    const float *kp0, *kp1, *vals, *sigma0, *sigma1;
    const double *cov0, *cov1;
    const float* pos_Tw;
    const double* cov0_world;
    const uint8_t* color;
    const float *K, *T_BS, *prior_pose;
    float baseline;
    int32_t n_rows[MV_MAX_LANES];
    int64_t time_ns[MV_MAX_LANES];
};
struct MapLaneTimes {
    int64_t t[MV_MAX_LANES];
};

__global__ __launch_bounds__(256) void map_append_lanes_kernel(MapLaneFrames a, const mvMapStores* __restrict__ stores) {
    const int l = blockIdx.x;   // one workgroup per lane: a lane that is refused returns on its own, the others never see it
    if (l >= a.lanes) return;
    const size_t o = (size_t)l * a.cap;
    mvMapFrame fr;
    fr.n_rows = a.n_rows[l];
    fr.table_stride = a.lanes * a.cap;   // value table [11, lanes, cap]: row stride lanes * cap, this lane's columns at l * cap
    fr.prev_frame = a.prev_frame;
    fr.min_num_point = a.min_num_point;
    fr.valid = a.valid ? a.valid + o : nullptr;
    fr.kp0 = a.kp0 + 2 * o; fr.kp1 = a.kp1 + 2 * o;
    fr.vals = a.vals + o;
    fr.sigma0 = a.sigma0 + 3 * o; fr.sigma1 = a.sigma1 + 3 * o;
    fr.cov0 = a.cov0 + 9 * o; fr.cov1 = a.cov1 + 9 * o;
    fr.pos_Tw = a.pos_Tw + 3 * o;
    fr.cov0_world = a.cov0_world + 9 * o;
    fr.color = a.color ? a.color + 3 * o : nullptr;
    fr.K = a.K;
    fr.T_BS = a.T_BS + 7 * (size_t)l;
    fr.prior_pose = a.prior_pose ? a.prior_pose + 7 * (size_t)l : nullptr;
    fr.baseline = a.baseline;
    fr.time_ns = a.time_ns[l];
    fr.out_frame_idx = nullptr;
    const mvMapStores st = stores[l];   // (wave-uniform loads)
    if (!st.counts) return;
    map_append_frame(fr, st);
}

// a non-keyframe (UniformKeyframe: Odometry/MACVO.py:177-179 -> push_keyframe(frame1, pose of the previous keyframe, need_interp=True), :339-348): one frame row
// flagged for interpolation, no match / point rows, no frame2match range; only the frame count advances (it is not a lost frame)
__device__ __forceinline__ void map_skip_row(const mvMapStores& st, const float* __restrict__ K, const float* __restrict__ T_BS, const float* __restrict__ pose,
                                             float baseline, int64_t time_ns) {
    int64_t* cnt = st.counts;
    const int64_t F = cnt[0];
    if (F >= st.cap_frames) {   // refused like any append when the store is full
        cnt[4] += 1;
        return;
    }
    const size_t f = (size_t)F;
    for (int c = 0; c < 9; ++c) st.K[9 * f + c] = K[c];
    st.baseline[f] = baseline;
    for (int c = 0; c < 7; ++c) {
        st.pose[7 * f + c] = pose[c];
        st.T_BS[7 * f + c] = T_BS[c];
    }
    st.time_ns[f] = time_ns;
    st.need_interp[f] = 1;
    for (int c = 0; c < 2 * st.max_frame_range; ++c) {
        st.frame2match_ranges[2 * st.max_frame_range * f + c] = -1;
        st.frame2map_ranges[2 * st.max_frame_range * f + c] = -1;
    }
    st.frame2match_num[f] = 0;
    st.frame2map_num[f] = 0;
    cnt[0] = F + 1;
}

__global__ void map_skip_kernel(mvMapStores st, const float* __restrict__ K, const float* __restrict__ T_BS, const float* __restrict__ pose, float baseline,
                                int64_t time_ns) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    map_skip_row(st, K, T_BS, pose, baseline, time_ns);
}

// ... of every lane: thread l writes lane l's row (its own map, its own pose and T_BS [lanes, 7], its own timestamp)
__global__ __launch_bounds__(MV_MAX_LANES) void map_skip_lanes_kernel(const mvMapStores* __restrict__ stores, int lanes, const float* __restrict__ K,
                                                                     const float* __restrict__ T_BS, const float* __restrict__ pose, float baseline,
                                                                     MapLaneTimes times) {
    const int l = threadIdx.x;
    if (blockIdx.x != 0 || l >= lanes) return;
    const mvMapStores st = stores[l];
    if (!st.counts) return;
    map_skip_row(st, K, T_BS + 7 * (size_t)l, pose + 7 * (size_t)l, baseline, times.t[l]);
}

// write_graph_data (Optimizer.py:104-108) of every lane: the optimised poses [lanes, 7] over the priors the frames were pushed with, row frame_idx of each map
__global__ void map_set_pose_lanes_kernel(const mvMapStores* __restrict__ stores, int lanes, int frame_idx, const float* __restrict__ pose) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 7 * lanes) return;
    const int l = i / 7;
    float* dst = stores[l].pose;
    if (!dst || frame_idx < 0 || (int64_t)frame_idx >= stores[l].cap_frames) return;
    dst[7 * (size_t)frame_idx + (i - 7 * l)] = pose[i];
}

// dense-mapping tail: map_points.push + frame2map.add for the newest frame (Odometry/MACVO.py:329-337)
__global__ __launch_bounds__(256) void map_append_points_kernel(mvMapStores st, int n, const float* __restrict__ pos, const double* __restrict__ cov,
                                                                 const uint8_t* __restrict__ color) {
    __shared__ int base, frame, ok;
    int64_t* cnt = st.counts;
    if (threadIdx.x == 0) {
        base = (int)cnt[5];
        frame = (int)cnt[0] - 1;
        const bool fits = frame >= 0 && (int64_t)base + n <= st.cap_map_points && st.frame2map_num[frame] < st.max_frame_range;
        ok = fits ? 1 : 0;
        if (!fits) cnt[4] += 1;
    }
    __syncthreads();
    if (!ok) return;
    const size_t P0 = (size_t)base;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            st.mp_pos_Tw[3 * (P0 + i) + c] = pos[3 * (size_t)i + c];
            st.mp_color[3 * (P0 + i) + c] = color ? color[3 * (size_t)i + c] : (uint8_t)0;
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) st.mp_cov_Tw[9 * (P0 + i) + c] = cov[9 * (size_t)i + c];
    }
    if (threadIdx.x == 0) {
        const size_t f = (size_t)frame;
        const int64_t k = st.frame2map_num[f];
        st.frame2map_ranges[2 * (st.max_frame_range * f + k)] = (int64_t)P0;
        st.frame2map_ranges[2 * (st.max_frame_range * f + k) + 1] = (int64_t)n;
        st.frame2map_num[f] = k + 1;
        cnt[5] = (int64_t)P0 + n;
    }
}

// body poses of Odometry/Interface.py:47-49: T_BS @ pose @ T_BS^-1, float32 arithmetic like pp.SE3(float32 tensors)
__global__ void body_poses_kernel(const float* __restrict__ pose, const float* __restrict__ T_BS, int T, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    const float* a = T_BS + 7 * (size_t)i;
    const float* b = pose + 7 * (size_t)i;
    auto act = [](const float* q, const float* p, float* o) {
        float u0 = q[1] * p[2] - q[2] * p[1], u1 = q[2] * p[0] - q[0] * p[2], u2 = q[0] * p[1] - q[1] * p[0];
        u0 += u0; u1 += u1; u2 += u2;
        o[0] = (p[0] + q[3] * u0) + (q[1] * u2 - q[2] * u1);
        o[1] = (p[1] + q[3] * u1) + (q[2] * u0 - q[0] * u2);
        o[2] = (p[2] + q[3] * u2) + (q[0] * u1 - q[1] * u0);
    };
    auto mulq = [](const float* x, const float* y, float* o) {
        o[0] = (x[3] * y[0] + y[3] * x[0]) + (x[1] * y[2] - x[2] * y[1]);
        o[1] = (x[3] * y[1] + y[3] * x[1]) + (x[2] * y[0] - x[0] * y[2]);
        o[2] = (x[3] * y[2] + y[3] * x[2]) + (x[0] * y[1] - x[1] * y[0]);
        o[3] = x[3] * y[3] - ((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]);
    };
    // ab = T_BS * pose
    float r[3], ab_t[3], ab_q[4];
    act(a + 3, b, r);
    ab_t[0] = a[0] + r[0]; ab_t[1] = a[1] + r[1]; ab_t[2] = a[2] + r[2];
    mulq(a + 3, b + 3, ab_q);
    // inv(T_BS) = (-q^-1 . t, q^-1)
    const float qi[4] = {-a[3], -a[4], -a[5], a[6]};
    float ti[3];
    act(qi, a, ti);
    ti[0] = -ti[0]; ti[1] = -ti[1]; ti[2] = -ti[2];
    float* o = out + 7 * (size_t)i;
    act(ab_q, ti, r);
    o[0] = ab_t[0] + r[0]; o[1] = ab_t[1] + r[1]; o[2] = ab_t[2] + r[2];
    mulq(ab_q, qi, o + 3);
}

// MotionInterpolate.elaborate_map (Module/MapProcessor.py:57-76), one workgroup, float64:
//   motions[i] = pose[i]^-1 pose[i+1]; a motion INTO a need_interp frame (except the first / last two) is replaced by the
//   se3-linear interpolation between its nearest good neighbours (interpolate_pose, Utility/Math.py:96-121); the track is
//   rebuilt as pose[0] @ cumprod(NormalizeQuat(motions)) and cast back to float32.
__global__ __launch_bounds__(256) void motion_interpolate_kernel(float* __restrict__ pose, const uint8_t* __restrict__ need_interp,
                                                                  int T, double* __restrict__ motions /* [T-1, 7] scratch */,
                                                                  int32_t* __restrict__ out_count) {
    const int t = threadIdx.x;
    const int Mn = T - 1;
    for (int i = t; i < Mn; i += blockDim.x) {
        const Se3d m = se3_mul(se3_inv(load_pose(pose + 7 * (size_t)i)), load_pose(pose + 7 * (size_t)(i + 1)));
        double* o = motions + 7 * (size_t)i;
        o[0] = m.t[0]; o[1] = m.t[1]; o[2] = m.t[2]; o[3] = m.q[0]; o[4] = m.q[1]; o[5] = m.q[2]; o[6] = m.q[3];
    }
    __threadfence_block();
    __syncthreads();
    auto bad = [&](int i) { return i >= 2 && i < Mn - 2 && need_interp[i + 1] != 0; };   // bad_mask[:2] = bad_mask[-2:] = False
    auto load_m = [&](int i) {
        const double* o = motions + 7 * (size_t)i;
        Se3d m;
        m.t[0] = o[0]; m.t[1] = o[1]; m.t[2] = o[2]; m.q[0] = o[3]; m.q[1] = o[4]; m.q[2] = o[5]; m.q[3] = o[6];
        return m;
    };
    int n_bad = 0;
    // interpolated motions go to registers first (a bad motion never serves as a neighbour, so order does not matter)
    for (int i = t; i < Mn; i += blockDim.x) {
        if (!bad(i)) continue;
        ++n_bad;
        int s = i - 1, e = i + 1;
        while (bad(s)) --s;
        while (bad(e)) ++e;
        const Se3d Ps = load_m(s), Pe = load_m(e);
        double xi[6];
        se3_log(se3_mul(Pe, se3_inv(Ps)), xi);
        // torch divides two int64 tensors in the default dtype (float32): Utility/Math.py:114
        const double prop = (double)((float)(i - s) / (float)(e - s));
#pragma unroll
        for (int c = 0; c < 6; ++c) xi[c] *= prop;
        const Se3d m = se3_mul(se3_exp(xi), Ps);
        double* o = motions + 7 * (size_t)i;   // safe: neighbours s, e are good entries, never rewritten
        o[0] = m.t[0]; o[1] = m.t[1]; o[2] = m.t[2]; o[3] = m.q[0]; o[4] = m.q[1]; o[5] = m.q[2]; o[6] = m.q[3];
    }
    n_bad = wave_sum(n_bad);
    __shared__ int tot;
    if (t == 0) tot = 0;
    __syncthreads();
    if ((t & 63) == 0 && n_bad) atomicAdd(&tot, n_bad);
    __threadfence_block();
    __syncthreads();
    if (t == 0) {
        if (out_count) out_count[0] = tot;
        // cumulative product with NormalizeQuat on both operands of every product (MapProcessor.py:73), in order
        Se3d acc = load_pose(pose);
        const Se3d p0 = acc;
        Se3d run;
        for (int i = 0; i < Mn; ++i) {
            const Se3d m = load_m(i);
            run = i == 0 ? m : se3_mul(se3_normq(run), se3_normq(m));
            acc = se3_mul(p0, run);
            float* o = pose + 7 * (size_t)(i + 1);
            o[0] = (float)acc.t[0]; o[1] = (float)acc.t[1]; o[2] = (float)acc.t[2];
            o[3] = (float)acc.q[0]; o[4] = (float)acc.q[1]; o[5] = (float)acc.q[2]; o[6] = (float)acc.q[3];
        }
    }
}

// PoseInterpolate.elaborate_map (Module/MapProcessor.py:33-45) on one pose table, by one 256-thread workgroup, float64 inside: a flagged row outside
// the first / last five becomes se3_interp of its nearest good rows (se3_interp.h: pose_interp_row).  A good row is never written and only good rows
// are read as neighbours, so the rows can be rewritten in place, in any order.  The edge flags are cleared in the table as the reference clears them
// (bad_mask is a view of the stored tensor); no flag that is read (rows 5 .. T - 6) is one that is cleared.
__device__ __forceinline__ void pose_interpolate_table(float* __restrict__ pose, uint8_t* __restrict__ need_interp, int T, uint8_t* __restrict__ mask) {
    for (int i = threadIdx.x; i < T; i += blockDim.x) {
        Se3d m;
        const bool bad = pose_interp_row(pose, need_interp, T, i, m);
        if (bad) {
            float* o = pose + 7 * (size_t)i;
            o[0] = (float)m.t[0]; o[1] = (float)m.t[1]; o[2] = (float)m.t[2];
            o[3] = (float)m.q[0]; o[4] = (float)m.q[1]; o[5] = (float)m.q[2]; o[6] = (float)m.q[3];
        }
        mask[i] = bad ? 1 : 0;
        if (i < 5 || i >= T - 5) need_interp[i] = 0;
    }
}

__global__ __launch_bounds__(256) void pose_interpolate_kernel(float* __restrict__ pose, uint8_t* __restrict__ need_interp, int T, uint8_t* __restrict__ mask) {
    pose_interpolate_table(pose, need_interp, T, mask);
}

struct MapLaneCounts {
    int32_t T[MV_MAX_LANES];
};

// ... of every lane: one workgroup per lane, each on its own map's pose / need_interp tables
__global__ __launch_bounds__(256) void pose_interpolate_lanes_kernel(const mvMapStores* __restrict__ stores, MapLaneCounts n, uint8_t* __restrict__ mask,
                                                                     int64_t mask_stride) {
    const int l = blockIdx.x;
    const mvMapStores st = stores[l];   // (wave-uniform loads)
    const int T = n.T[l];
    if (!st.pose || !st.need_interp || (int64_t)T > st.cap_frames) return;
    pose_interpolate_table(st.pose, st.need_interp, T, mask + (int64_t)l * mask_stride);
}

}  // namespace

extern "C" int mv_map_append(const mvMapFrame* frame, const mvMapStores* stores, mvStream_t stream) {
    MV_CHECK_ARG(frame && stores);
    const mvMapFrame& f = *frame;
    const mvMapStores& s = *stores;
    MV_CHECK_ARG(f.n_rows >= 0 && f.table_stride >= f.n_rows && f.K && f.T_BS && s.counts);
    MV_CHECK_ARG(f.n_rows == 0 || (f.kp0 && f.kp1 && f.vals && f.sigma0 && f.sigma1 && f.cov0 && f.cov1 && f.pos_Tw && f.cov0_world));
    MV_CHECK_ARG(s.max_pt_obs >= 1 && s.max_frame_range >= 1);
    MV_CHECK_ARG(s.cap_frames > 0 && s.cap_match > 0 && s.cap_points > 0);
    MV_CHECK_ARG(s.K && s.baseline && s.pose && s.T_BS && s.need_interp && s.time_ns && s.pos_Tw && s.cov_Tw && s.color);
    MV_CHECK_ARG(s.pixel1_uv && s.pixel2_uv && s.pixel1_d && s.pixel2_d && s.pixel1_disp && s.pixel2_disp && s.pixel1_disp_cov &&
                 s.pixel2_disp_cov && s.obs1_covTc && s.obs2_covTc && s.pixel1_uv_cov && s.pixel2_uv_cov && s.pixel1_d_cov &&
                 s.pixel2_d_cov);
    MV_CHECK_ARG(s.frame2match_ranges && s.frame2match_num && s.frame2map_ranges && s.frame2map_num && s.match2frame1 &&
                 s.match2frame2 && s.match2point && s.point2match_edges && s.point2match_deg);
    hipLaunchKernelGGL(map_append_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, f, s);
    return mv_launch_status();
}

extern "C" int mv_map_append_skipped(const mvMapStores* stores, const float* K_dev, const float* T_BS_dev, const float* pose_dev, float baseline,
                                     int64_t time_ns, mvStream_t stream) {
    MV_CHECK_ARG(stores && K_dev && T_BS_dev && pose_dev);
    const mvMapStores& s = *stores;
    MV_CHECK_ARG(s.counts && s.cap_frames > 0 && s.max_frame_range >= 1);
    MV_CHECK_ARG(s.K && s.baseline && s.pose && s.T_BS && s.need_interp && s.time_ns && s.frame2match_ranges && s.frame2match_num &&
                 s.frame2map_ranges && s.frame2map_num);
    hipLaunchKernelGGL(map_skip_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, s, K_dev, T_BS_dev, pose_dev, baseline, time_ns);
    return mv_launch_status();
}

// ------------------------------------------------------------------------------------------------ lane-batched forms (one launch for all lanes)
extern "C" int mv_map_append_lanes(const mvMapFrameLanes* frames, const mvMapStores* stores_dev, mvStream_t stream) {
    MV_CHECK_ARG(frames && stores_dev);
    const mvMapFrameLanes& f = *frames;
    MV_CHECK_ARG(f.lanes >= 1 && f.lanes <= MV_MAX_LANES && f.cap >= 0 && f.n_rows && f.time_ns && f.K && f.T_BS);
    MV_CHECK_ARG((int64_t)f.lanes * f.cap <= INT32_MAX);
    MapLaneFrames a{};
    int n_max = 0;
    for (int l = 0; l < f.lanes; ++l) {
        MV_CHECK_ARG(f.n_rows[l] >= 0 && f.n_rows[l] <= f.cap);
        a.n_rows[l] = f.n_rows[l];
        a.time_ns[l] = f.time_ns[l];
        n_max = f.n_rows[l] > n_max ? f.n_rows[l] : n_max;
    }
    MV_CHECK_ARG(n_max == 0 || (f.kp0 && f.kp1 && f.vals && f.sigma0 && f.sigma1 && f.cov0 && f.cov1 && f.pos_Tw && f.cov0_world));
    a.lanes = f.lanes; a.cap = f.cap; a.prev_frame = f.prev_frame; a.min_num_point = f.min_num_point;
    a.valid = f.valid; a.kp0 = f.kp0; a.kp1 = f.kp1; a.vals = f.vals; a.sigma0 = f.sigma0; a.sigma1 = f.sigma1;
    a.cov0 = f.cov0; a.cov1 = f.cov1; a.pos_Tw = f.pos_Tw; a.cov0_world = f.cov0_world; a.color = f.color;
    a.K = f.K; a.T_BS = f.T_BS; a.prior_pose = f.prior_pose; a.baseline = f.baseline;
    hipLaunchKernelGGL(map_append_lanes_kernel, dim3(f.lanes), dim3(256), 0, (hipStream_t)stream, a, stores_dev);
    return mv_launch_status();
}

extern "C" int mv_map_append_skipped_lanes(const mvMapStores* stores_dev, int lanes, const float* K_dev, const float* T_BS_dev, const float* pose_dev,
                                           float baseline, const int64_t* time_ns, mvStream_t stream) {
    MV_CHECK_ARG(stores_dev && lanes >= 1 && lanes <= MV_MAX_LANES && K_dev && T_BS_dev && pose_dev && time_ns);
    MapLaneTimes t{};
    for (int l = 0; l < lanes; ++l) t.t[l] = time_ns[l];
    hipLaunchKernelGGL(map_skip_lanes_kernel, dim3(1), dim3(MV_MAX_LANES), 0, (hipStream_t)stream, stores_dev, lanes, K_dev, T_BS_dev, pose_dev, baseline, t);
    return mv_launch_status();
}

extern "C" int mv_map_set_pose_lanes(const mvMapStores* stores_dev, int lanes, int frame_idx, const float* pose_dev, mvStream_t stream) {
    MV_CHECK_ARG(stores_dev && lanes >= 1 && lanes <= MV_MAX_LANES && frame_idx >= 0 && pose_dev);
    hipLaunchKernelGGL(map_set_pose_lanes_kernel, dim3(mv_ceil_div(7 * lanes, 256)), dim3(256), 0, (hipStream_t)stream, stores_dev, lanes, frame_idx, pose_dev);
    return mv_launch_status();
}

extern "C" int mv_map_append_points(const mvMapStores* stores, int n, const float* pos_Tw, const double* cov, const uint8_t* color,
                                    mvStream_t stream) {
    MV_CHECK_ARG(stores && n >= 0);
    const mvMapStores& s = *stores;
    MV_CHECK_ARG(s.counts && s.frame2map_ranges && s.frame2map_num && s.max_frame_range >= 1);
    MV_CHECK_ARG(s.cap_map_points > 0 && s.mp_pos_Tw && s.mp_cov_Tw && s.mp_color);
    MV_CHECK_ARG(n == 0 || (pos_Tw && cov));
    hipLaunchKernelGGL(map_append_points_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, s, n, pos_Tw, cov, color);
    return mv_launch_status();
}

extern "C" int mv_body_poses(const float* pose, const float* T_BS, int T, float* out, mvStream_t stream) {
    MV_CHECK_ARG(T >= 0);
    if (T == 0) return MV_OK;
    MV_CHECK_ARG(pose && T_BS && out);
    hipLaunchKernelGGL(body_poses_kernel, dim3(mv_ceil_div(T, 256)), dim3(256), 0, (hipStream_t)stream, pose, T_BS, T, out);
    return mv_launch_status();
}

extern "C" int mv_motion_interpolate(float* pose, const uint8_t* need_interp, int T, double* scratch, int32_t* out_count,
                                     mvStream_t stream) {
    MV_CHECK_ARG(T >= 0);
    if (T < 2) return MV_OK;
    MV_CHECK_ARG(pose && need_interp && scratch);
    hipLaunchKernelGGL(motion_interpolate_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pose, need_interp, T, scratch,
                       out_count);
    return mv_launch_status();
}

extern "C" int mv_pose_interpolate(float* pose, uint8_t* need_interp, int T, uint8_t* mask, mvStream_t stream) {
    MV_CHECK_ARG(T >= 0);
    if (T == 0) return MV_OK;
    MV_CHECK_ARG(pose && need_interp && mask);
    hipLaunchKernelGGL(pose_interpolate_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pose, need_interp, T, mask);
    return mv_launch_status();
}

extern "C" int mv_pose_interpolate_lanes(const mvMapStores* stores_dev, int lanes, const int32_t* T, uint8_t* mask, int64_t mask_stride, mvStream_t stream) {
    MV_CHECK_ARG(stores_dev && lanes >= 1 && lanes <= MV_MAX_LANES && T && mask);
    MapLaneCounts n{};
    for (int l = 0; l < lanes; ++l) {
        MV_CHECK_ARG(T[l] >= 0 && (int64_t)T[l] <= mask_stride);
        n.T[l] = T[l];
    }
    hipLaunchKernelGGL(pose_interpolate_lanes_kernel, dim3(lanes), dim3(256), 0, (hipStream_t)stream, stores_dev, n, mask, mask_stride);
    return mv_launch_status();
}
