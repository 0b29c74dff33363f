// TEST INFRASTRUCTURE: host replay of ONE lane of traj_assoc_kernel (mac-vo_amd/csrc/traj_assoc.hip) and of pose_interpolate_kernel
// (mac-vo_amd/csrc/visual_map.hip).  It includes the kernels' own arithmetic header (csrc/se3_interp.h) and runs the same per-lane functions in the
// kernels' order: the lane-wide checks, then one query / one row after the other, one rounding at the store.  Built by tests/assoc_twin.py with
// g++ -ffp-contract=off.  The product never builds or loads it.
//
// With -DASSOC_TWIN_MAIN it is a plain stand-alone program (its own main) for a host-only -fsanitize=address,undefined run.
#include <vector>

#include "../../mac-vo_amd/csrc/se3_interp.h"

namespace {

void store(const se3i::Se3d& p, int f64, void* out, int64_t j) {
    const double o[7] = {p.t[0], p.t[1], p.t[2], p.q[0], p.q[1], p.q[2], p.q[3]};
    for (int k = 0; k < 7; ++k) {
        if (f64) ((double*)out)[7 * j + k] = o[k];
        else ((float*)out)[7 * j + k] = (float)o[k];
    }
}

}  // namespace

extern "C" int assoc_twin_lane(const void* src, const void* ts, int T, const void* tq, int Q, const void* origin, int src_f64, int time_i64, int origin_f64,
                               int out_f64, int64_t src_stride, int rebase, void* out, uint8_t* flag) {
    se3i::AssocLane ln;
    ln.src = src; ln.ts = ts; ln.tq = tq; ln.origin = T > 0 ? origin : nullptr;
    ln.T = T; ln.Q = Q;
    ln.src_stride = src_stride;
    ln.src_f64 = src_f64; ln.time_i64 = time_i64; ln.origin_f64 = origin_f64; ln.rebase = rebase;
    int bad = 0;
    for (int i = 0; i < (T > Q ? T : Q); ++i) bad |= se3i::assoc_check(ln, i);
    const int status = se3i::assoc_status(T, bad);
    const double qnan = __builtin_nan("");
    for (int j = 0; j < Q; ++j) {
        se3i::Se3d p;
        int f = 0;
        if (status == MV_TRAJ_OK) {
            f = se3i::assoc_query(ln, j, p);
        } else {
            p.t[0] = p.t[1] = p.t[2] = p.q[0] = p.q[1] = p.q[2] = p.q[3] = qnan;
        }
        store(p, out_f64, out, j);
        flag[j] = (uint8_t)f;
    }
    return status;
}

// pose [T,7] fp32 and need_interp [T] in place, mask [T]: the rows are computed from the table as it is read — a bad row only reads good rows, which are
// never written, so the in-place order does not matter (as in the kernel)
extern "C" void pose_interp_twin_lane(float* pose, uint8_t* need_interp, int T, uint8_t* mask) {
    for (int i = 0; i < T; ++i) {
        se3i::Se3d m;
        const bool bad = se3i::pose_interp_row(pose, need_interp, T, i, m);
        if (bad) {
            float* o = pose + 7 * (size_t)i;
            o[0] = (float)m.t[0]; o[1] = (float)m.t[1]; o[2] = (float)m.t[2];
            o[3] = (float)m.q[0]; o[4] = (float)m.q[1]; o[5] = (float)m.q[2]; o[6] = (float)m.q[3];
        }
        mask[i] = bad ? 1 : 0;
        if (i < 5 || i >= T - 5) need_interp[i] = 0;
    }
}

#ifdef ASSOC_TWIN_MAIN
#include <stdio.h>
int main() {
    // exact-size heap buffers, so that a read or a write past a table is caught
    const int T = 37, Q = 91;
    std::vector<float> src(7 * T);
    std::vector<int64_t> ts(T), tq(Q);
    for (int i = 0; i < T; ++i) {
        const double a = 0.11 * i;
        const float row[7] = {(float)(0.3 * i), (float)sin(a), (float)(0.01 * i * i), 0.f, (float)sin(0.5 * a), 0.f, (float)cos(0.5 * a)};
        for (int k = 0; k < 7; ++k) src[7 * i + k] = row[k];
        ts[i] = 1403636579763555584LL + 50000000LL * i + (i ? 2 * i + 1 : 0);
    }
    for (int j = 0; j < Q; ++j) tq[j] = ts[0] - 70000000LL + 21000001LL * ((j * 37) % Q);
    const double origin[7] = {1, 2, 3, 0, 0, 0.6, 0.8};
    int rc = 0;
    for (int with_origin = 0; with_origin < 2; ++with_origin) {
        for (int len : {0, 1, 2, T}) {
            std::vector<double> out(7 * Q);
            std::vector<uint8_t> flag(Q);
            const int st = assoc_twin_lane(src.data(), ts.data(), len, tq.data(), Q, with_origin ? origin : nullptr, 0, 1, 1, 1, 7, 1, out.data(), flag.data());
            if (st != (len ? MV_TRAJ_OK : MV_TRAJ_TOO_SHORT)) rc = 1;
            for (int j = 0; j < 7 * Q && len; ++j) if (!(fabs(out[j]) <= DBL_MAX)) rc = 1;
        }
    }
    for (int len : {0, 1, 9, 10, 11, 12, T}) {
        std::vector<float> pose(src.begin(), src.begin() + 7 * len);
        std::vector<uint8_t> need(len), mask(len);
        for (int i = 0; i < len; ++i) need[i] = (i % 3) != 0;
        pose_interp_twin_lane(pose.data(), need.data(), len, mask.data());
        for (int i = 0; i < len; ++i) if (mask[i] != (i >= 5 && i < len - 5 && (i % 3) != 0)) rc = 1;
    }
    printf(rc ? "assoc_twin: FAILED\n" : "assoc_twin: OK\n");
    return rc;
}
#endif
