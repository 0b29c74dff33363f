// Frame preprocessing — the resampling family of DataLoader/Transform.py:41-209 (ScaleFrame, CenterCropFrame, SmartResizeFrame, CastDataType) as ONE launch
// per frame: every plane of every lane is resampled, cropped or padded and converted by the same grid.  torchvision's tensor path (resize -> F.interpolate,
// center_crop) is RESTATED here, UNPINNED (torchvision is no dependency and is unpinned in the reference, requirements.txt:17).
//
// A plan (mv_preprocess_plan, host arithmetic below) describes, per axis, three steps that any foldable list of the four transforms reduces to:
//   window  = the source after the crops / pads in FRONT of the resize:  window(y, x) = src(y + win_y0, x + win_x0) inside a valid rectangle, 0 elsewhere
//   resized = window resampled to rs_h x rs_w (nearest-exact or antialiased bilinear; an axis of unchanged size is not resampled)
//   out     = the crops / pads BEHIND the resize:  out(y, x) = resized(y + out_y0, x + out_x0) inside a valid rectangle, 0 elsewhere
// An output pixel samples the SOURCE directly: no resized intermediate plane in HBM, no second launch, nothing synchronises.
//
// gfx950 shape.  A 256-thread workgroup owns a 16 x 64 output tile of one plane (grid z = lane x plane).
//   * gather kernel (nearest, and every plan without a resize — KITTI's 376 x 1241 -> 376 x 780 is a pure crop): a thread produces four consecutive output
//     columns of one row; bit-exact copies.  Four consecutive source elements are fetched by one vector load when the row is not resampled along x and the
//     address allows it.
//   * antialias kernel (bilinear): threads 0-63 / 64-79 compute the tile's 64 column / 16 row tap windows and fp32 weights (resample_math.h) into LDS; the WIDTH
//     pass then filters the tile's source-row footprint (at most (16 - 1) * 8 + 17 + 1 = 138 rows at the supported downscale of 8) straight from global
//     memory into a [138][64] fp32 LDS tile — lane = output column, so a wave's loads of one tap are one strided row segment —, the HEIGHT pass filters that
//     tile out of LDS with 16-byte reads (a thread = 4 columns of one row).  Width first, then height, as torch; 40.4 KB of static LDS.
//   * both store four elements with one vector store (16 B fp32, 8 B fp16 / bf16, 4 B bool) when all four are inside the row and the address is aligned, and
//     with predicated scalar stores otherwise (ragged right edge, rows of a width that is no multiple of four).
// Weight-0 taps inside a window are multiplied in (0 * NaN = NaN, as torch).  -ffp-contract=off: one rounding per product and per sum.
#include "common.h"
#include "resample_math.h"

namespace {

constexpr int TH = 16, TW = 64, NT = 256;
constexpr int TAPS = rsm::kMaxTaps;
constexpr int MAX_ROWS = (TH - 1) * rsm::kMaxScale + TAPS + 1;
constexpr int MAX_DIM = 1 << 15;          // every extent of a plan (source, window, resized, out): H * W stays inside an int

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
typedef uint8_t u8x4 __attribute__((ext_vector_type(4)));

struct Group {
    const void* src;
    void* dst;
    long long src_lane_stride, dst_lane_stride;
    int planes, kind, src_dtype, dst_dtype;
    int mid_dtype;        // the type the plane has when it is resampled: a CastDataType in front of the resize, else the source's (fp32 for uint8)
    int binarize;         // a bool mask through the bilinear filter: resampled != 0
};

struct Args {
    mvPreprocessPlan p;
    Group g[MV_PP_MAX_GROUPS];
    int n_groups, planes_per_lane;
};

__device__ __forceinline__ float round_to(float v, int dt) {
    if (dt == MV_F16) return (float)(_Float16)v;
    if (dt == MV_BF16) {                                   // round to nearest even; NaN -> the canonical quiet NaN (as c10::BFloat16)
        uint32_t u = __float_as_uint(v);
        if (v != v) return __uint_as_float(0x7FC00000u);
        u += 0x7FFFu + ((u >> 16) & 1u);
        return __uint_as_float(u & 0xFFFF0000u);
    }
    return v;
}

// an image's uint8 is widened as the reference's loaders widen it (float(u8) / 255, a true fp32 division); a mask's is a bool
__device__ __forceinline__ float widen_u8(uint8_t v, int kind) { return kind == MV_PP_MASK ? (v ? 1.f : 0.f) : (float)v / 255.0f; }
__device__ __forceinline__ float widen_f16(uint16_t v) {
    _Float16 h;
    __builtin_memcpy(&h, &v, 2);
    return (float)h;
}
__device__ __forceinline__ float widen_bf16(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

__device__ __forceinline__ float load_src(const void* p, size_t i, int dt, int kind) {
    switch (dt) {
        case MV_F32: return ((const float*)p)[i];
        case MV_F16: return widen_f16(((const uint16_t*)p)[i]);
        case MV_BF16: return widen_bf16(((const uint16_t*)p)[i]);
        default: return widen_u8(((const uint8_t*)p)[i], kind);
    }
}

// window(y, x): the source inside the valid rectangle (which the host has checked to lie inside the source), 0 elsewhere
__device__ __forceinline__ float win_load(const mvPreprocessPlan& p, const Group& g, const void* sp, int vy, int vx) {
    if (vy < p.win_vy0 || vy >= p.win_vy1 || vx < p.win_vx0 || vx >= p.win_vx1) return 0.f;
    return round_to(load_src(sp, (size_t)(vy + p.win_y0) * p.src_w + (vx + p.win_x0), g.src_dtype, g.kind), g.mid_dtype);
}

// four consecutive window elements of a row that lie inside the valid rectangle: one vector load where the address allows it
__device__ __forceinline__ f32x4 win_load4(const mvPreprocessPlan& p, const Group& g, const void* sp, int vy, int vx) {
    const size_t i = (size_t)(vy + p.win_y0) * p.src_w + (vx + p.win_x0);
    f32x4 v;
    if (g.src_dtype == MV_F32 && (((uintptr_t)((const float*)sp + i)) & 15) == 0) {
        v = *reinterpret_cast<const f32x4*>((const float*)sp + i);
    } else if (g.src_dtype == MV_F16 && (((uintptr_t)((const uint16_t*)sp + i)) & 7) == 0) {
        const u16x4 r = *reinterpret_cast<const u16x4*>((const uint16_t*)sp + i);
        v = f32x4{widen_f16(r.x), widen_f16(r.y), widen_f16(r.z), widen_f16(r.w)};
    } else if (g.src_dtype == MV_BF16 && (((uintptr_t)((const uint16_t*)sp + i)) & 7) == 0) {
        const u16x4 r = *reinterpret_cast<const u16x4*>((const uint16_t*)sp + i);
        v = f32x4{widen_bf16(r.x), widen_bf16(r.y), widen_bf16(r.z), widen_bf16(r.w)};
    } else if (g.src_dtype == MV_PP_U8 && (((uintptr_t)((const uint8_t*)sp + i)) & 3) == 0) {
        const u8x4 r = *reinterpret_cast<const u8x4*>((const uint8_t*)sp + i);
        v = f32x4{widen_u8(r.x, g.kind), widen_u8(r.y, g.kind), widen_u8(r.z, g.kind), widen_u8(r.w, g.kind)};
    } else {
        v = f32x4{load_src(sp, i, g.src_dtype, g.kind), load_src(sp, i + 1, g.src_dtype, g.kind), load_src(sp, i + 2, g.src_dtype, g.kind),
                  load_src(sp, i + 3, g.src_dtype, g.kind)};
    }
    return f32x4{round_to(v.x, g.mid_dtype), round_to(v.y, g.mid_dtype), round_to(v.z, g.mid_dtype), round_to(v.w, g.mid_dtype)};
}

// what follows the resampler for one element: the rounding to the plane's type (torchvision resizes a 16-bit plane in fp32 and rounds once), gt_flow's division by
// its round_scale (Transform.py:79-80: after the resize, a true division, rounded to the plane's type again) and the bool cast of a filtered mask
__device__ __forceinline__ float finish(const mvPreprocessPlan& p, const Group& g, int plane, float acc) {
    float r = round_to(acc, g.mid_dtype);
    if (g.kind == MV_PP_FLOW && p.scaled) r = round_to(r / (plane == 0 ? p.round_scale_u : p.round_scale_v), g.mid_dtype);
    if (g.binarize) r = r != 0.f ? 1.f : 0.f;
    return r;
}

// n (1..4) elements of one output row at element index i of the plane
__device__ __forceinline__ void store4(void* dp, size_t i, int dt, f32x4 v, int n) {
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
    } else if (dt == MV_F16) {
        _Float16* d = (_Float16*)dp + i;
        const f16x4 h = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
        if (n == 4 && ((uintptr_t)d & 7) == 0) {
            *reinterpret_cast<f16x4*>(d) = h;
        } else {
            d[0] = h.x;
            if (n > 1) d[1] = h.y;
            if (n > 2) d[2] = h.z;
            if (n > 3) d[3] = h.w;
        }
    } else if (dt == MV_BF16) {
        uint16_t* d = (uint16_t*)dp + i;
        const u16x4 h = {(uint16_t)(__float_as_uint(round_to(v.x, MV_BF16)) >> 16), (uint16_t)(__float_as_uint(round_to(v.y, MV_BF16)) >> 16),
                         (uint16_t)(__float_as_uint(round_to(v.z, MV_BF16)) >> 16), (uint16_t)(__float_as_uint(round_to(v.w, MV_BF16)) >> 16)};
        if (n == 4 && ((uintptr_t)d & 7) == 0) {
            *reinterpret_cast<u16x4*>(d) = h;
        } else {
            d[0] = h.x;
            if (n > 1) d[1] = h.y;
            if (n > 2) d[2] = h.z;
            if (n > 3) d[3] = h.w;
        }
    } else {                                                   // bool
        uint8_t* d = (uint8_t*)dp + i;
        const u8x4 h = {(uint8_t)(v.x != 0.f), (uint8_t)(v.y != 0.f), (uint8_t)(v.z != 0.f), (uint8_t)(v.w != 0.f)};
        if (n == 4 && ((uintptr_t)d & 3) == 0) {
            *reinterpret_cast<u8x4*>(d) = h;
        } else {
            d[0] = h.x;
            if (n > 1) d[1] = h.y;
            if (n > 2) d[2] = h.z;
            if (n > 3) d[3] = h.w;
        }
    }
}

// blockIdx.z -> (group, plane of the group, the plane's source and destination).  The group's record is read where the launch put it, in the kernel-argument
// segment (constant address space, `Args` is the only argument): the index is the same in every lane, so each field is one scalar load at a run-time offset.
// (Indexing the by-value argument itself at run time would copy the table to scratch; selecting field by field holds all 96 dwords of it in SGPRs.)
struct PlaneRef {
    int plane;
    const void* src;
    void* dst;
};
typedef const __attribute__((address_space(4))) Args* KernArgs;
__device__ __forceinline__ size_t elem_bytes(int dt) { return dt == MV_F32 ? 4 : (dt == MV_PP_U8 ? 1 : 2); }
__device__ __forceinline__ PlaneRef plane_of(const Args& a, Group& g) {
    const KernArgs ka = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = blockIdx.z / a.planes_per_lane;
    int q = blockIdx.z - lane * a.planes_per_lane, gi = 0;
    for (int k = 0; k + 1 < a.n_groups && k + 1 < MV_PP_MAX_GROUPS; ++k) {
        const int n = ka->g[k].planes;
        if (q < n) break;
        q -= n;
        gi = k + 1;
    }
    g.src = ka->g[gi].src, g.dst = ka->g[gi].dst;
    g.src_lane_stride = ka->g[gi].src_lane_stride, g.dst_lane_stride = ka->g[gi].dst_lane_stride;
    g.planes = ka->g[gi].planes, g.kind = ka->g[gi].kind, g.src_dtype = ka->g[gi].src_dtype, g.dst_dtype = ka->g[gi].dst_dtype;
    g.mid_dtype = ka->g[gi].mid_dtype, g.binarize = ka->g[gi].binarize;
    const size_t so = (size_t)lane * g.src_lane_stride + (size_t)q * a.p.src_h * a.p.src_w;
    const size_t dz = (size_t)lane * g.dst_lane_stride + (size_t)q * a.p.out_h * a.p.out_w;
    PlaneRef r;
    r.plane = q;
    r.src = (const char*)g.src + so * elem_bytes(g.src_dtype);
    r.dst = (char*)g.dst + dz * elem_bytes(g.dst_dtype);
    return r;
}

__global__ __launch_bounds__(NT) void preprocess_gather_kernel(const Args a) {
    const mvPreprocessPlan& p = a.p;
    Group g;
    const PlaneRef pr = plane_of(a, g);
    const int oy = blockIdx.y * TH + threadIdx.x / 16, ox = blockIdx.x * TW + (threadIdx.x % 16) * 4;
    if (oy >= p.out_h || ox >= p.out_w) return;
    const int n = min(4, p.out_w - ox);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (oy >= p.out_vy0 && oy < p.out_vy1) {
        const int vy = rsm::nearest_index(oy + p.out_y0, p.win_h, p.rs_h);
        const int vx0 = ox + p.out_x0;                      // (the window column of element 0 when x is not resampled)
        if (p.rs_w == p.win_w && n == 4 && ox >= p.out_vx0 && ox + 4 <= p.out_vx1 && vy >= p.win_vy0 && vy < p.win_vy1 && vx0 >= p.win_vx0 &&
            vx0 + 4 <= p.win_vx1) {
            v = win_load4(p, g, pr.src, vy, vx0);
        } else {
            float e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = ox + j;
                e[j] = 0.f;
                if (x >= p.out_vx0 && x < p.out_vx1) e[j] = win_load(p, g, pr.src, vy, rsm::nearest_index(x + p.out_x0, p.win_w, p.rs_w));
            }
            v = f32x4{e[0], e[1], e[2], e[3]};
        }
        v = f32x4{finish(p, g, pr.plane, v.x), finish(p, g, pr.plane, v.y), finish(p, g, pr.plane, v.z), finish(p, g, pr.plane, v.w)};
    }
    store4(pr.dst, (size_t)oy * p.out_w + ox, g.dst_dtype, v, n);
}

__global__ __launch_bounds__(NT) void preprocess_aa_kernel(const Args a) {
    __shared__ __attribute__((aligned(16))) float tmp[MAX_ROWS][TW];
    __shared__ float wx[TW * TAPS], wy[TH * TAPS];
    __shared__ int xmin_s[TW], xsz_s[TW], ymin_s[TH], ysz_s[TH];
    const mvPreprocessPlan& p = a.p;
    Group g;
    const PlaneRef pr = plane_of(a, g);
    const int tid = threadIdx.x;
    const int oy0 = blockIdx.y * TH, ox0 = blockIdx.x * TW;

    // the tile's tap windows and weights: one output column / row per thread; a column or row outside the valid rectangle (the pad) has no taps
    if (tid < TW) {
        const int x = ox0 + tid;
        int xmin = 0, n = 0;
        if (x < p.out_w && x >= p.out_vx0 && x < p.out_vx1) {
            const rsm::Window w = rsm::aa_window(x + p.out_x0, p.win_w, p.rs_w);
            xmin = w.xmin;
            n = rsm::aa_weights(x + p.out_x0, p.win_w, p.rs_w, w, &wx[tid * TAPS], TAPS);
        }
        xmin_s[tid] = xmin, xsz_s[tid] = n;
    } else if (tid < TW + TH) {
        const int r = tid - TW, y = oy0 + r;
        int ymin = 0, n = 0;
        if (y < p.out_h && y >= p.out_vy0 && y < p.out_vy1) {
            const rsm::Window w = rsm::aa_window(y + p.out_y0, p.win_h, p.rs_h);
            ymin = w.xmin;
            n = rsm::aa_weights(y + p.out_y0, p.win_h, p.rs_h, w, &wy[r * TAPS], TAPS);
        }
        ymin_s[r] = ymin, ysz_s[r] = n;
    }
    __syncthreads();

    // the window rows the tile's height pass reads: [fy0, fy0 + nrows)
    int fy0 = 0x7fffffff, fy1 = 0;
#pragma unroll
    for (int r = 0; r < TH; ++r)
        if (ysz_s[r] > 0) {
            fy0 = min(fy0, ymin_s[r]);
            fy1 = max(fy1, ymin_s[r] + ysz_s[r]);
        }
    const int nrows = fy1 > fy0 ? min(fy1 - fy0, MAX_ROWS) : 0;

    // width pass: window rows -> tmp[row][tile column], taps in ascending order
    {
        const int c = tid % TW;
        const int xmin = xmin_s[c], xn = xsz_s[c];
        for (int fr = tid / TW; fr < nrows; fr += NT / TW) {
            float acc = 0.f;
            for (int k = 0; k < xn; ++k) acc += wx[c * TAPS + k] * win_load(p, g, pr.src, fy0 + fr, xmin + k);
            tmp[fr][c] = acc;
        }
    }
    __syncthreads();

    // height pass out of LDS: a thread = four columns of one row
    const int r = tid / 16, c4 = (tid % 16) * 4;
    const int oy = oy0 + r, ox = ox0 + c4;
    if (oy >= p.out_h || ox >= p.out_w) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int yn = ysz_s[r], yb = ymin_s[r] - fy0;
    for (int k = 0; k < yn; ++k) {
        const int row = yb + k;
        if (row >= nrows) break;                               // (never taken at a supported scale: keeps every LDS read inside the tile)
        const float w = wy[r * TAPS + k];
        const f32x4 t = *reinterpret_cast<const f32x4*>(&tmp[row][c4]);
        acc = f32x4{acc.x + w * t.x, acc.y + w * t.y, acc.z + w * t.z, acc.w + w * t.w};
    }
    // (a pad column of a live row has no taps: its width pass wrote 0, so the sum above is 0; a pad row has no taps either)
    const f32x4 v = {finish(p, g, pr.plane, acc.x), finish(p, g, pr.plane, acc.y), finish(p, g, pr.plane, acc.z), finish(p, g, pr.plane, acc.w)};
    store4(pr.dst, (size_t)oy * p.out_w + ox, g.dst_dtype, v, min(4, p.out_w - ox));
}

// ---------------------------------------------------------------------------------------------------------------- the plan (host arithmetic)
// Python's round(k / 2.0) for k >= 0: half to even
int round_half_even_of_half(int k) {
    const int m = k / 2;
    return (k & 1) ? m + (m & 1) : m;
}

// torchvision's center_crop on one axis of an extent `ext` described by (offset, valid range): pad to `target` if smaller ((t - s) // 2 in front, the rest
// behind), else cut at int(round((s - t) / 2.0)).  new(x) = old(x + d).
void crop_axis(int32_t& ext, int32_t& off, int32_t& v0, int32_t& v1, int target) {
    const int s = ext;
    const int d = s < target ? -((target - s) / 2) : round_half_even_of_half(s - target);
    off += d;
    v0 = v0 - d > 0 ? v0 - d : 0;
    v1 = v1 - d < target ? v1 - d : target;
    if (v1 <= v0) v0 = v1 = 0;
    ext = target;
}

bool dtype_is_float(int dt) { return dt == MV_F32 || dt == MV_F16 || dt == MV_BF16; }

// every invariant the kernels' addressing rests on
bool plan_ok(const mvPreprocessPlan& p) {
    const int32_t dims[8] = {p.src_h, p.src_w, p.win_h, p.win_w, p.rs_h, p.rs_w, p.out_h, p.out_w};
    for (int i = 0; i < 8; ++i)
        if (dims[i] < 1 || dims[i] > MAX_DIM) return false;
    if (!(0 <= p.win_vy0 && p.win_vy0 <= p.win_vy1 && p.win_vy1 <= p.win_h && 0 <= p.win_vx0 && p.win_vx0 <= p.win_vx1 && p.win_vx1 <= p.win_w)) return false;
    if (p.win_vy1 > p.win_vy0 && !(p.win_vy0 + (int64_t)p.win_y0 >= 0 && p.win_vy1 + (int64_t)p.win_y0 <= p.src_h)) return false;
    if (p.win_vx1 > p.win_vx0 && !(p.win_vx0 + (int64_t)p.win_x0 >= 0 && p.win_vx1 + (int64_t)p.win_x0 <= p.src_w)) return false;
    if (!(0 <= p.out_vy0 && p.out_vy0 <= p.out_vy1 && p.out_vy1 <= p.out_h && 0 <= p.out_vx0 && p.out_vx0 <= p.out_vx1 && p.out_vx1 <= p.out_w)) return false;
    if (p.out_vy1 > p.out_vy0 && !(p.out_vy0 + (int64_t)p.out_y0 >= 0 && p.out_vy1 + (int64_t)p.out_y0 <= p.rs_h)) return false;
    if (p.out_vx1 > p.out_vx0 && !(p.out_vx0 + (int64_t)p.out_x0 >= 0 && p.out_vx1 + (int64_t)p.out_x0 <= p.rs_w)) return false;
    if (!p.scaled && (p.rs_h != p.win_h || p.rs_w != p.win_w)) return false;
    if (p.interp != MV_PP_NEAREST && p.interp != MV_PP_BILINEAR) return false;
    if (p.mid_dtype != -1 && !dtype_is_float(p.mid_dtype)) return false;
    if (p.out_dtype != -1 && !dtype_is_float(p.out_dtype)) return false;
    return true;
}

}  // namespace

extern "C" int mv_preprocess_plan(mvPreprocessPlan* plan, const mvPreprocessPlan* prev, int src_h, int src_w, const float* K, int kind, double a0, double a1,
                                  int mode) {
    MV_CHECK_ARG(plan);
    mvPreprocessPlan p;
    if (prev) {
        p = *prev;
        MV_CHECK_ARG(plan_ok(p));
    } else {
        MV_CHECK_ARG(src_h >= 1 && src_w >= 1 && src_h <= MAX_DIM && src_w <= MAX_DIM);
        p = mvPreprocessPlan{};
        p.src_h = p.win_h = p.rs_h = p.out_h = src_h;
        p.src_w = p.win_w = p.rs_w = p.out_w = src_w;
        p.win_vy1 = p.out_vy1 = src_h;
        p.win_vx1 = p.out_vx1 = src_w;
        p.interp = MV_PP_NEAREST;
        p.mid_dtype = p.out_dtype = -1;
        p.round_scale_u = p.round_scale_v = 1.f;
        for (int i = 0; i < 9; ++i) p.K[i] = K ? K[i] : (i % 4 == 0 ? 1.f : 0.f);
    }
    // CenterCropFrame.crop_stereo (Transform.py:109-127) of the frame as it stands: in front of a resize it moves the window, behind one the output
    auto crop = [&](int th, int tw) {
        const int cur_h = p.out_h, cur_w = p.out_w;
        if (!p.scaled) {
            crop_axis(p.win_h, p.win_y0, p.win_vy0, p.win_vy1, th);
            crop_axis(p.win_w, p.win_x0, p.win_vx0, p.win_vx1, tw);
            p.rs_h = p.out_h = p.win_h, p.rs_w = p.out_w = p.win_w;
            p.out_y0 = p.out_x0 = p.out_vy0 = p.out_vx0 = 0;
            p.out_vy1 = p.out_h, p.out_vx1 = p.out_w;
        } else {
            crop_axis(p.out_h, p.out_y0, p.out_vy0, p.out_vy1, th);
            crop_axis(p.out_w, p.out_x0, p.out_vx0, p.out_vx1, tw);
        }
        p.K[2] = p.K[2] - (float)((cur_w - tw) / 2.);         // the UN-rounded half difference: the reference's half-pixel disagreement with the crop
        p.K[5] = p.K[5] - (float)((cur_h - th) / 2.);
    };
    // ScaleFrame.scale_stereo (Transform.py:54-88) of the frame as it stands: Python doubles, int() truncation, K rows and (in the kernel) gt_flow divided in fp32
    auto scale = [&](double scale_u, double scale_v, int interp) -> int {
        const int cur_h = p.out_h, cur_w = p.out_w;
        MV_CHECK_ARG(scale_u > 0.0 && scale_v > 0.0 && scale_u <= 1e9 && scale_v <= 1e9);       // (NaN fails both)
        MV_CHECK_ARG(interp == MV_PP_NEAREST || interp == MV_PP_BILINEAR);
        const double fh = (double)cur_h / scale_v, fw = (double)cur_w / scale_u;
        MV_CHECK_ARG(fh >= 1.0 && fw >= 1.0 && fh < (double)MAX_DIM + 1.0 && fw < (double)MAX_DIM + 1.0);   // (target 0: the reference divides by zero)
        const int th = (int)fh, tw = (int)fw;
        const double rsv = (double)cur_h / (double)th, rsu = (double)cur_w / (double)tw;
        if (th != cur_h || tw != cur_w) {                      // (resize returns its input at an unchanged size: a unit scale is a copy)
            if (p.scaled) return MV_ERR_UNSUPPORTED;           // a second resize does not fold: the caller starts another plan
            p.scaled = 1, p.interp = interp;
            p.rs_h = p.out_h = th, p.rs_w = p.out_w = tw;
            p.out_y0 = p.out_x0 = p.out_vy0 = p.out_vx0 = 0;
            p.out_vy1 = th, p.out_vx1 = tw;
            p.round_scale_u = (float)rsu, p.round_scale_v = (float)rsv;
        }
        for (int c = 0; c < 3; ++c) {
            p.K[c] = p.K[c] / (float)rsu;
            p.K[3 + c] = p.K[3 + c] / (float)rsv;
        }
        return MV_OK;
    };

    switch (kind) {
        case MV_PP_SCALE: {
            const int e = scale(a0, a1, mode);
            if (e != MV_OK) return e;
            break;
        }
        case MV_PP_CENTER_CROP:
        case MV_PP_SMART_RESIZE: {
            MV_CHECK_ARG(a0 >= 1.0 && a1 >= 1.0 && a0 <= (double)MAX_DIM && a1 <= (double)MAX_DIM && a0 == (double)(int)a0 && a1 == (double)(int)a1);
            const int th = (int)a0, tw = (int)a1;
            if (kind == MV_PP_SMART_RESIZE) {                  // SmartResizeFrame.forward (Transform.py:197-209)
                const double sh = (double)p.out_h / (double)th, sw = (double)p.out_w / (double)tw;
                const double s = sh < sw ? sh : sw;
                const int e = scale(s, s, mode);
                if (e != MV_OK) return e;
            }
            crop(th, tw);               // (after SmartResize's scale it sees the resized frame — often one pixel short of the target: then it pads)
            break;
        }
        case MV_PP_CAST: {                                     // CastDataType (Transform.py:153-178): every plane, the mask included; K stays fp32
            MV_CHECK_ARG(dtype_is_float(mode));
            if (p.out_dtype != -1 && p.out_dtype != mode) return MV_ERR_UNSUPPORTED;      // two different roundings in a row do not fold
            if (!p.scaled) p.mid_dtype = mode;
            p.out_dtype = mode;
            break;
        }
        default: return MV_ERR_INVALID_ARG;
    }
    MV_CHECK_ARG(plan_ok(p));
    *plan = p;
    return MV_OK;
}

extern "C" int mv_preprocess_lanes(const mvPreprocessPlan* plan, const mvPreprocessGroup* groups, int n_groups, int lanes, mvStream_t stream) {
    MV_CHECK_ARG(plan && groups && n_groups >= 1 && n_groups <= MV_PP_MAX_GROUPS && lanes >= 1 && lanes <= MV_MAX_LANES);
    MV_CHECK_ARG(plan_ok(*plan));
    const mvPreprocessPlan& p = *plan;
    const bool aa = p.scaled && p.interp == MV_PP_BILINEAR;
    // the antialias kernel's LDS tile holds the footprint of a downscale of at most 8 per axis (the reference's resolution sweep goes to 4)
    if (aa && ((int64_t)p.win_h > (int64_t)rsm::kMaxScale * p.rs_h || (int64_t)p.win_w > (int64_t)rsm::kMaxScale * p.rs_w)) return MV_ERR_UNSUPPORTED;
    Args a;
    a.p = p;
    a.n_groups = n_groups;
    a.planes_per_lane = 0;
    const int64_t src_plane = (int64_t)p.src_h * p.src_w, dst_plane = (int64_t)p.out_h * p.out_w;
    for (int i = 0; i < MV_PP_MAX_GROUPS; ++i) {
        Group& g = a.g[i];
        if (i >= n_groups) {
            g = Group{};
            continue;
        }
        const mvPreprocessGroup& u = groups[i];
        MV_CHECK_ARG(u.src && u.dst && u.planes >= 1 && u.planes <= 16);
        MV_CHECK_ARG(u.kind == MV_PP_IMAGE || u.kind == MV_PP_FLOW || u.kind == MV_PP_MASK || u.kind == MV_PP_DEPTH);
        MV_CHECK_ARG(u.kind != MV_PP_FLOW || u.planes == 2);
        MV_CHECK_ARG(dtype_is_float(u.src_dtype) || (u.src_dtype == MV_PP_U8 && (u.kind == MV_PP_IMAGE || u.kind == MV_PP_MASK)));
        MV_CHECK_ARG(dtype_is_float(u.dst_dtype) || (u.dst_dtype == MV_PP_U8 && u.kind == MV_PP_MASK && u.src_dtype == MV_PP_U8));
        MV_CHECK_ARG(u.src_lane_stride >= u.planes * src_plane && u.dst_lane_stride >= u.planes * dst_plane);
        const uintptr_t sa = u.src_dtype == MV_F32 ? 3 : (u.src_dtype == MV_PP_U8 ? 0 : 1), da = u.dst_dtype == MV_F32 ? 3 : (u.dst_dtype == MV_PP_U8 ? 0 : 1);
        MV_CHECK_ARG(((uintptr_t)u.src & sa) == 0 && ((uintptr_t)u.dst & da) == 0);
        g.src = u.src, g.dst = u.dst;
        g.src_lane_stride = u.src_lane_stride, g.dst_lane_stride = u.dst_lane_stride;
        g.planes = u.planes, g.kind = u.kind, g.src_dtype = u.src_dtype, g.dst_dtype = u.dst_dtype;
        g.mid_dtype = p.mid_dtype != -1 ? p.mid_dtype : (u.src_dtype == MV_PP_U8 ? MV_F32 : u.src_dtype);
        // torchvision resizes a bool mask as fp32 and casts back without rounding: resampled != 0.  A mask CastDataType has already turned into numbers is a plane
        g.binarize = aa && u.kind == MV_PP_MASK && u.src_dtype == MV_PP_U8 && p.mid_dtype == -1;
        a.planes_per_lane += u.planes;
    }
    const dim3 grid(mv_ceil_div(p.out_w, TW), mv_ceil_div(p.out_h, TH), lanes * a.planes_per_lane), block(NT);
    if (grid.z > 65535 || grid.y > 65535) return MV_ERR_UNSUPPORTED;
    if (aa) hipLaunchKernelGGL(preprocess_aa_kernel, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(preprocess_gather_kernel, grid, block, 0, (hipStream_t)stream, a);
    return mv_launch_status();
}
