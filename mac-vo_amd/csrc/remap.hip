// Stereo rectification — what DataLoader/Dataset/EuRoC.py:143-174, 231-236 and VBR.py:60-64, 155-180 do with OpenCV on the host, as a host plan and two kernels:
//   mv_stereo_rectify_plan  cv2.stereoRectify(flags = CALIB_ZERO_DISPARITY, alpha = -1), once per sequence: Bouguet's method in double arithmetic, no GPU;
//   mv_rectify_maps         cv2.initUndistortRectifyMap(CV_32FC1), once per sequence: both cameras' maps in one launch, fp64 on the device, rounded once;
//   mv_remap_lanes          cv2.remap(INTER_LINEAR) of every left and right image and the loaders' float32 / 255, once per FRAME: one launch for every plane of
//                           every lane of every group; a pure integer gather (remap_math.h), bit for bit the formula.
// OpenCV is RESTATED, PARITY-UNPINNED (no dependency here).  Known differences of the plan: OpenCV keeps the four undistorted corners in float32, the plan in
// double (the principal point agrees to about 1e-4 px); OpenCV projects R onto the rotations through an SVD before it takes the rotation vector, the plan takes
// R as it is given.
//
// gfx950 shape of the remap.  A 256-thread workgroup owns a 16 x 64 output tile of one lane of one group (grid z = lane x group); a thread produces four
// x-adjacent pixels of ALL channels, so a map entry is read once: the two map loads are 16-byte vector loads where the address allows (a wave reads four whole
// 256-byte row segments per map) and scalar loads on the ragged edge.  The taps go through the cache hierarchy — rectification is close to the identity, so the
// threads of a wave read neighbouring source bytes.  A pixel whose four taps lie inside the source (all but a thin border) fetches the two x-adjacent taps of a
// row with ONE load (2 * C bytes interleaved: 2 + 4 bytes for C = 3, 8 bytes for C = 4; 2 bytes per channel planar) instead of one byte load per tap and
// channel; a border pixel takes the masked per-tap path of remap_math.h.  Each destination plane is written with one vector store per thread (16 B fp32, 8 B
// fp16 / bf16, 4 B uint8) where all four pixels are inside the row and the address is aligned.  No LDS, no scratch: every register array is indexed by
// unrolled constants, and the group's record is read from the kernel-argument segment at a wave-uniform offset (scalar loads).
#include "common.h"
#include "remap_math.h"

namespace {

constexpr int TH = 16, TW = 64, NT = 256;
constexpr int MAX_DIM = 1 << 15;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
typedef uint8_t u8x4 __attribute__((ext_vector_type(4)));

struct Group {
    const uint8_t* src;
    void* dst;
    const float* map_x;
    const float* map_y;
    long long src_lane_stride, dst_lane_stride, map_lane_stride;
    int channels, hwc, reverse, dst_dtype;
};

struct Args {
    Group g[MV_RM_MAX_GROUPS];
    int n_groups, src_h, src_w, out_h, out_w;
};
typedef const __attribute__((address_space(4))) Args* KernArgs;

__device__ __forceinline__ size_t elem_bytes(int dt) { return dt == MV_F32 ? 4 : (dt == MV_PP_U8 ? 1 : 2); }

__device__ __forceinline__ uint16_t bf16_bits(float v) {       // round to nearest even (the values are finite)
    uint32_t u = __float_as_uint(v);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// n (1..4) pixels of one output row of one plane at element index i: out / 255 for the float types, the integer itself for uint8
__device__ __forceinline__ void store4(void* dp, size_t i, int dt, const int32_t (&e)[4], int n) {
    if (dt == MV_PP_U8) {
        uint8_t* d = (uint8_t*)dp + i;
        const u8x4 h = {(uint8_t)e[0], (uint8_t)e[1], (uint8_t)e[2], (uint8_t)e[3]};
        if (n == 4 && ((uintptr_t)d & 3) == 0) {
            *reinterpret_cast<u8x4*>(d) = h;
        } else {
            d[0] = h.x;
            if (n > 1) d[1] = h.y;
            if (n > 2) d[2] = h.z;
            if (n > 3) d[3] = h.w;
        }
        return;
    }
    const f32x4 v = {rmm::unit(e[0]), rmm::unit(e[1]), rmm::unit(e[2]), rmm::unit(e[3])};
    if (dt == MV_F32) {
        float* d = (float*)dp + i;
        if (n == 4 && ((uintptr_t)d & 15) == 0) {
            *reinterpret_cast<f32x4*>(d) = v;
        } else {
            d[0] = v.x;
            if (n > 1) d[1] = v.y;
            if (n > 2) d[2] = v.z;
            if (n > 3) d[3] = v.w;
        }
        return;
    }
    // fp16 / bf16: the same 2-byte stores of the rounded bits
    u16x4 h;
    if (dt == MV_F16) {
        const f16x4 q = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
        __builtin_memcpy(&h, &q, 8);
    } else {
        h = u16x4{bf16_bits(v.x), bf16_bits(v.y), bf16_bits(v.z), bf16_bits(v.w)};
    }
    uint16_t* d = (uint16_t*)dp + i;
    if (n == 4 && ((uintptr_t)d & 7) == 0) {
        *reinterpret_cast<u16x4*>(d) = h;
    } else {
        d[0] = h.x;
        if (n > 1) d[1] = h.y;
        if (n > 2) d[2] = h.z;
        if (n > 3) d[3] = h.w;
    }
}

// four x-adjacent output pixels (ox .. ox + 3 of row oy; the caller has checked oy < oh and ox < ow) of all C channels of one lane
template <int C, bool HWC>
__device__ __forceinline__ void remap_body(const uint8_t* __restrict__ src, void* dst, const float* __restrict__ mx, const float* __restrict__ my, int reverse,
                                           int dst_dtype, int sh, int sw, int oh, int ow, int oy, int ox) {
    const int n = min(4, ow - ox);
    const size_t mi = (size_t)oy * ow + ox;
    float fx[4], fy[4];
    if (n == 4 && ((((uintptr_t)(mx + mi)) | ((uintptr_t)(my + mi))) & 15) == 0) {
        const f32x4 vx = *reinterpret_cast<const f32x4*>(mx + mi), vy = *reinterpret_cast<const f32x4*>(my + mi);
        fx[0] = vx.x, fx[1] = vx.y, fx[2] = vx.z, fx[3] = vx.w;
        fy[0] = vy.x, fy[1] = vy.y, fy[2] = vy.z, fy[3] = vy.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fx[j] = j < n ? mx[mi + j] : 0.f;                  // (a pixel past the row's end is computed from (0, 0) and never stored)
            fy[j] = j < n ? my[mi + j] : 0.f;
        }
    }
    const size_t plane = (size_t)sh * sw;
    int32_t v[C][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const rmm::Tap t = rmm::tap_of(fx[j], fy[j]);
        if (t.ok && rmm::interior(t, sw, sh)) {
            const size_t at = (size_t)t.iy * sw + t.ix;
            if constexpr (HWC) {                               // the two taps of a row are 2 * C adjacent bytes
                uint8_t r0[2 * C], r1[2 * C];
                __builtin_memcpy(r0, src + at * C, 2 * C);
                __builtin_memcpy(r1, src + (at + sw) * C, 2 * C);
#pragma unroll
                for (int c = 0; c < C; ++c) v[c][j] = rmm::blend(t, r0[c], r0[C + c], r1[c], r1[C + c]);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    uint8_t r0[2], r1[2];
                    __builtin_memcpy(r0, src + c * plane + at, 2);
                    __builtin_memcpy(r1, src + c * plane + at + sw, 2);
                    v[c][j] = rmm::blend(t, r0[0], r0[1], r1[0], r1[1]);
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c)
                v[c][j] = rmm::sample(t, sw, sh, [&](int y, int x) {
                    const size_t p = (size_t)y * sw + x;
                    return HWC ? src[p * C + c] : src[c * plane + p];
                });
        }
    }
    const size_t oplane = (size_t)oh * ow, eb = elem_bytes(dst_dtype);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        int32_t e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (C >= 3) e[j] = (reverse && c < 3) ? v[c < 3 ? 2 - c : c][j] : v[c][j];      // rmm::src_channel with constant indices on both sides
            else e[j] = v[c][j];
        }
        store4((char*)dst + (size_t)c * oplane * eb, mi, dst_dtype, e, n);
    }
}

__global__ __launch_bounds__(NT) void remap_lanes_kernel(const Args a) {
    const KernArgs ka = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = blockIdx.z / a.n_groups, gi = blockIdx.z - lane * a.n_groups;
    const int oy = blockIdx.y * TH + threadIdx.x / 16, ox = blockIdx.x * TW + (threadIdx.x % 16) * 4;
    if (oy >= a.out_h || ox >= a.out_w) return;
    const int C = ka->g[gi].channels, hwc = ka->g[gi].hwc, reverse = ka->g[gi].reverse, dt = ka->g[gi].dst_dtype;
    const uint8_t* src = ka->g[gi].src + (size_t)lane * ka->g[gi].src_lane_stride;
    void* dst = (char*)ka->g[gi].dst + (size_t)lane * ka->g[gi].dst_lane_stride * elem_bytes(dt);
    const float* mx = ka->g[gi].map_x + (size_t)lane * ka->g[gi].map_lane_stride;
    const float* my = ka->g[gi].map_y + (size_t)lane * ka->g[gi].map_lane_stride;
    // (wave-uniform: one body per launch in the usual case)
    if (C == 1) remap_body<1, false>(src, dst, mx, my, reverse, dt, a.src_h, a.src_w, a.out_h, a.out_w, oy, ox);
    else if (C == 3 && hwc) remap_body<3, true>(src, dst, mx, my, reverse, dt, a.src_h, a.src_w, a.out_h, a.out_w, oy, ox);
    else if (C == 3) remap_body<3, false>(src, dst, mx, my, reverse, dt, a.src_h, a.src_w, a.out_h, a.out_w, oy, ox);
    else if (hwc) remap_body<4, true>(src, dst, mx, my, reverse, dt, a.src_h, a.src_w, a.out_h, a.out_w, oy, ox);
    else remap_body<4, false>(src, dst, mx, my, reverse, dt, a.src_h, a.src_w, a.out_h, a.out_w, oy, ox);
}

struct MapArgs {
    mvRectifyCam cam[MV_RM_MAX_GROUPS];
    float *map_x, *map_y;
    int n_cams, out_h, out_w;
};
typedef const __attribute__((address_space(4))) MapArgs* MapKernArgs;

// one thread per map entry; a wave writes one 256-byte row segment of each map
__global__ __launch_bounds__(NT) void rectify_maps_kernel(const MapArgs a) {
    const MapKernArgs ka = (MapKernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    const int u = blockIdx.x * 64 + threadIdx.x % 64, v = blockIdx.y * 4 + threadIdx.x / 64, ci = blockIdx.z;
    if (u >= a.out_w || v >= a.out_h) return;
    const double x = ka->cam[ci].iR[0] * u + ka->cam[ci].iR[1] * v + ka->cam[ci].iR[2];
    const double y = ka->cam[ci].iR[3] * u + ka->cam[ci].iR[4] * v + ka->cam[ci].iR[5];
    const double w = ka->cam[ci].iR[6] * u + ka->cam[ci].iR[7] * v + ka->cam[ci].iR[8];
    const double k1 = ka->cam[ci].k[0], k2 = ka->cam[ci].k[1], p1 = ka->cam[ci].k[2], p2 = ka->cam[ci].k[3];
    const double k3 = ka->cam[ci].k[4], k4 = ka->cam[ci].k[5], k5 = ka->cam[ci].k[6], k6 = ka->cam[ci].k[7];
    const double xp = x / w, yp = y / w, r2 = xp * xp + yp * yp;
    const double kr = (1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2) / (1.0 + k4 * r2 + k5 * r2 * r2 + k6 * r2 * r2 * r2);
    const double xd = xp * kr + 2.0 * p1 * xp * yp + p2 * (r2 + 2.0 * xp * xp);
    const double yd = yp * kr + p1 * (r2 + 2.0 * yp * yp) + 2.0 * p2 * xp * yp;
    const size_t i = ((size_t)ci * a.out_h + v) * a.out_w + u;
    a.map_x[i] = (float)(ka->cam[ci].fx * xd + ka->cam[ci].cx);
    a.map_y[i] = (float)(ka->cam[ci].fy * yd + ka->cam[ci].cy);
}

// ---------------------------------------------------------------------------------------------------------------- the plan (host arithmetic, doubles)
void mat3_mul(const double* A, const double* B, double* out) {
    double r[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
    for (int i = 0; i < 9; ++i) out[i] = r[i];
}
void mat3_t(const double* A, double* out) {
    double r[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r[3 * i + j] = A[3 * j + i];
    for (int i = 0; i < 9; ++i) out[i] = r[i];
}
void mat3_vec(const double* A, const double* v, double* out) {
    double r[3];
    for (int i = 0; i < 3; ++i) r[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
    for (int i = 0; i < 3; ++i) out[i] = r[i];
}
double norm3(const double* v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
bool mat3_inv(const double* A, double* out) {
    const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
    const double det = A[0] * c0 + A[1] * c1 + A[2] * c2;
    if (!(fabs(det) > 0.0) || !isfinite(det)) return false;
    const double r[9] = {c0, A[2] * A[7] - A[1] * A[8], A[1] * A[5] - A[2] * A[4], c1, A[0] * A[8] - A[2] * A[6], A[2] * A[3] - A[0] * A[5],
                         c2, A[1] * A[6] - A[0] * A[7], A[0] * A[4] - A[1] * A[3]};
    for (int i = 0; i < 9; ++i) out[i] = r[i] / det;
    return true;
}

// rotation vector -> matrix: I + sin(th) [k]x + (1 - cos(th)) [k]x^2
void rodrigues(const double* v, double* R) {
    const double th = norm3(v);
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (th < 1e-300) {
        for (int i = 0; i < 9; ++i) R[i] = I[i];
        return;
    }
    const double k[3] = {v[0] / th, v[1] / th, v[2] / th};
    const double Kx[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
    double K2[9];
    mat3_mul(Kx, Kx, K2);
    const double s = sin(th), c1 = 1.0 - cos(th);
    for (int i = 0; i < 9; ++i) R[i] = I[i] + s * Kx[i] + c1 * K2[i];
}

// rotation matrix -> vector.  Away from pi: the antisymmetric part scaled by theta / sin(theta), theta = atan2(|r|, (trace - 1) / 2); at pi the
// antisymmetric part vanishes and the axis comes from the diagonal, its signs from the off-diagonal sums.
void inv_rodrigues(const double* R, double* om) {
    const double r[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double s = norm3(r), c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    const double th = atan2(s, c);
    if (s < 1e-5 && c < 0.0) {
        double a[3] = {sqrt(fmax(0.5 * (R[0] + 1.0), 0.0)), sqrt(fmax(0.5 * (R[4] + 1.0), 0.0)), sqrt(fmax(0.5 * (R[8] + 1.0), 0.0))};
        if (R[1] + R[3] < 0.0) a[1] = -a[1];
        if (R[2] + R[6] < 0.0) a[2] = -a[2];
        if (fabs(a[0]) < fabs(a[1]) && fabs(a[0]) < fabs(a[2]) && ((R[5] + R[7] > 0.0) != (a[1] * a[2] > 0.0))) a[2] = -a[2];
        const double n = norm3(a);
        for (int i = 0; i < 3; ++i) om[i] = n > 0.0 ? a[i] * (th / n) : 0.0;
        return;
    }
    for (int i = 0; i < 3; ++i) om[i] = s > 0.0 ? r[i] * (th / s) : 0.0;
}

// five fixed-point iterations of the inverse distortion model on a pixel of the original camera -> normalised coordinates
void undistort_point(double u, double v, const double* K, const double* k, double& x, double& y) {
    const double x0 = (u - K[2]) / K[0], y0 = (v - K[5]) / K[4];
    x = x0, y = y0;
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double ik = (1.0 + k[5] * r2 + k[6] * r2 * r2 + k[7] * r2 * r2 * r2) / (1.0 + k[0] * r2 + k[1] * r2 * r2 + k[4] * r2 * r2 * r2);
        const double dx = 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x), dy = k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y;
        x = (x0 - dx) * ik, y = (y0 - dy) * ik;
    }
}

bool all_finite(const double* p, int n) {
    for (int i = 0; i < n; ++i)
        if (!isfinite(p[i])) return false;
    return true;
}

}  // namespace

extern "C" int mv_stereo_rectify_plan(mvRectifyPlan* plan, const double* K1, const double* D1, int n_d1, const double* K2, const double* D2, int n_d2, int nx,
                                      int ny, const double* R, const double* T) {
    MV_CHECK_ARG(plan && K1 && D1 && K2 && D2 && R && T);
    for (int n : {n_d1, n_d2})
        if (n != 4 && n != 5 && n != 8) return MV_ERR_UNSUPPORTED;
    MV_CHECK_ARG(nx >= 1 && ny >= 1 && nx <= MAX_DIM && ny <= MAX_DIM);
    MV_CHECK_ARG(all_finite(K1, 9) && all_finite(K2, 9) && all_finite(D1, n_d1) && all_finite(D2, n_d2) && all_finite(R, 9) && all_finite(T, 3));
    MV_CHECK_ARG(norm3(T) > 0.0);
    mvRectifyPlan p = mvRectifyPlan{};
    const double* Ks[2] = {K1, K2};
    for (int i = 0; i < n_d1; ++i) p.cam[0].k[i] = D1[i];
    for (int i = 0; i < n_d2; ++i) p.cam[1].k[i] = D2[i];

    double om[3], rr[9], rrT[9], t[3];
    inv_rodrigues(R, om);
    const double half[3] = {-0.5 * om[0], -0.5 * om[1], -0.5 * om[2]};
    rodrigues(half, rr);
    mat3_vec(rr, T, t);
    const int idx = fabs(t[0]) > fabs(t[1]) ? 0 : 1;
    const double c = t[idx], nt = norm3(t);
    double uu[3] = {0, 0, 0};
    uu[idx] = c > 0 ? 1.0 : -1.0;
    double ww[3] = {t[1] * uu[2] - t[2] * uu[1], t[2] * uu[0] - t[0] * uu[2], t[0] * uu[1] - t[1] * uu[0]};
    const double nw = norm3(ww);
    if (nw > 0.0) {
        const double f = acos(fabs(c) / nt) / nw;
        for (int i = 0; i < 3; ++i) ww[i] *= f;
    }
    double wR[9], tn[3];
    rodrigues(ww, wR);
    mat3_t(rr, rrT);
    mat3_mul(wR, rrT, p.R1);
    mat3_mul(wR, rr, p.R2);
    mat3_vec(p.R2, T, tn);

    // the new focal length: the smaller of the two cameras', shrunk by a negative k1 so that the rectified image stays inside the source
    double fc = INFINITY;
    for (int k = 0; k < 2; ++k) {
        double f = Ks[k][4 * (idx ^ 1)];
        MV_CHECK_ARG(Ks[k][0] != 0.0 && Ks[k][4] != 0.0);
        if (p.cam[k].k[0] < 0.0) f *= 1.0 + p.cam[k].k[0] * ((double)nx * nx + (double)ny * ny) / (4.0 * f * f);
        fc = f < fc ? f : fc;
    }
    // the new principal point: the image centre minus the mean of the four rectified corners; CALIB_ZERO_DISPARITY gives both cameras the average
    double cc[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        const double* Rk = k == 0 ? p.R1 : p.R2;
        double ax = 0, ay = 0;
        for (int i = 0; i < 4; ++i) {
            double x, y;
            undistort_point((i % 2) * (nx - 1.0), (i / 2) * (ny - 1.0), Ks[k], p.cam[k].k, x, y);
            const double q[3] = {x, y, 1.0};
            double r[3];
            mat3_vec(Rk, q, r);
            ax += fc * r[0] / r[2], ay += fc * r[1] / r[2];
        }
        cc[0] += 0.5 * ((nx - 1) / 2.0 - ax / 4.0), cc[1] += 0.5 * ((ny - 1) / 2.0 - ay / 4.0);
    }
    const double P[12] = {fc, 0, cc[0], 0, 0, fc, cc[1], 0, 0, 0, 1, 0};
    for (int i = 0; i < 12; ++i) p.P1[i] = p.P2[i] = P[i];
    p.P2[4 * idx + 3] = tn[idx] * fc;
    for (int k = 0; k < 2; ++k) {
        const double Kn[9] = {fc, 0, cc[0], 0, fc, cc[1], 0, 0, 1};
        double M[9];
        mat3_mul(Kn, k == 0 ? p.R1 : p.R2, M);
        MV_CHECK_ARG(mat3_inv(M, p.cam[k].iR));
        p.cam[k].fx = Ks[k][0], p.cam[k].fy = Ks[k][4], p.cam[k].cx = Ks[k][2], p.cam[k].cy = Ks[k][5];
    }
    p.fc = fc;
    p.baseline = fabs(p.P2[4 * idx + 3] / fc);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) p.K[3 * i + j] = (float)p.P1[4 * i + j];
    p.width = nx, p.height = ny, p.idx = idx;
    MV_CHECK_ARG(isfinite(fc) && fc != 0.0 && all_finite(p.P1, 12) && all_finite(p.P2, 12) && all_finite(p.cam[0].iR, 9) && all_finite(p.cam[1].iR, 9));
    *plan = p;
    return MV_OK;
}

extern "C" int mv_rectify_maps(const mvRectifyCam* cams, int n_cams, int out_h, int out_w, float* map_x, float* map_y, mvStream_t stream) {
    MV_CHECK_ARG(cams && map_x && map_y && n_cams >= 1 && n_cams <= MV_RM_MAX_GROUPS);
    MV_CHECK_ARG(out_h >= 1 && out_w >= 1 && out_h <= MAX_DIM && out_w <= MAX_DIM);
    MV_CHECK_ARG((((uintptr_t)map_x | (uintptr_t)map_y) & 3) == 0);
    MapArgs a;
    for (int i = 0; i < MV_RM_MAX_GROUPS; ++i) a.cam[i] = i < n_cams ? cams[i] : mvRectifyCam{};
    a.map_x = map_x, a.map_y = map_y;
    a.n_cams = n_cams, a.out_h = out_h, a.out_w = out_w;
    const dim3 grid(mv_ceil_div(out_w, 64), mv_ceil_div(out_h, 4), n_cams), block(NT);
    hipLaunchKernelGGL(rectify_maps_kernel, grid, block, 0, (hipStream_t)stream, a);
    return mv_launch_status();
}

extern "C" int mv_remap_lanes(const mvRemapGroup* groups, int n_groups, int lanes, int src_h, int src_w, int out_h, int out_w, mvStream_t stream) {
    MV_CHECK_ARG(groups && n_groups >= 1 && n_groups <= MV_RM_MAX_GROUPS && lanes >= 1 && lanes <= MV_MAX_LANES);
    MV_CHECK_ARG(src_h >= 1 && src_w >= 1 && out_h >= 1 && out_w >= 1 && src_h <= MAX_DIM && src_w <= MAX_DIM && out_h <= MAX_DIM && out_w <= MAX_DIM);
    Args a;
    a.n_groups = n_groups, a.src_h = src_h, a.src_w = src_w, a.out_h = out_h, a.out_w = out_w;
    const int64_t src_plane = (int64_t)src_h * src_w, dst_plane = (int64_t)out_h * out_w;
    for (int i = 0; i < MV_RM_MAX_GROUPS; ++i) {
        Group& g = a.g[i];
        if (i >= n_groups) {
            g = Group{};
            continue;
        }
        const mvRemapGroup& u = groups[i];
        MV_CHECK_ARG(u.src && u.dst && u.map_x && u.map_y);
        if (u.channels != 1 && u.channels != 3 && u.channels != 4) return MV_ERR_UNSUPPORTED;
        if (u.src_dtype != MV_PP_U8) return MV_ERR_UNSUPPORTED;                    // float sources are not built
        MV_CHECK_ARG(u.layout == MV_RM_PLANAR || u.layout == MV_RM_HWC);
        MV_CHECK_ARG(u.dst_dtype == MV_PP_U8 || u.dst_dtype == MV_F32 || u.dst_dtype == MV_F16 || u.dst_dtype == MV_BF16);
        MV_CHECK_ARG(u.src_lane_stride >= u.channels * src_plane && u.dst_lane_stride >= u.channels * dst_plane);
        MV_CHECK_ARG(u.map_lane_stride == 0 || u.map_lane_stride >= dst_plane);
        const uintptr_t da = u.dst_dtype == MV_F32 ? 3 : (u.dst_dtype == MV_PP_U8 ? 0 : 1);
        MV_CHECK_ARG(((uintptr_t)u.dst & da) == 0 && (((uintptr_t)u.map_x | (uintptr_t)u.map_y) & 3) == 0);
        g.src = (const uint8_t*)u.src, g.dst = u.dst, g.map_x = u.map_x, g.map_y = u.map_y;
        g.src_lane_stride = u.src_lane_stride, g.dst_lane_stride = u.dst_lane_stride, g.map_lane_stride = u.map_lane_stride;
        g.channels = u.channels, g.hwc = u.layout == MV_RM_HWC, g.reverse = u.reverse_channels != 0, g.dst_dtype = u.dst_dtype;
    }
    const dim3 grid(mv_ceil_div(out_w, TW), mv_ceil_div(out_h, TH), lanes * n_groups), block(NT);
    hipLaunchKernelGGL(remap_lanes_kernel, grid, block, 0, (hipStream_t)stream, a);
    return mv_launch_status();
}
