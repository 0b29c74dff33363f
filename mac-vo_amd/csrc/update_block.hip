// The decoder's recurrent update blocks in 16-bit operands: CovUpdateBlock (covhead.py:24-43: SepConvGRU, CovHead, mask x 0.25) and the gru / flow_head /
// mask members of FlowFormer's GMAUpdateBlock (covhead.py:112-114), one call each per decoder iteration.
//
//   update_to_nhwc_kernel        net [B,128,H,W] and inp [B,384,H,W] (NCHW through an LDS transpose, or channels-last as a copy) -> HX [M,512]
//   update_conv_kernel<F16,WM,WN> one convolution (1x5, 5x1, 3x3, 1x1; zero padding) as an implicit GEMM on v_mfma_f32_32x32x16_{bf16,f16}: the A operand
//                                is the packed weights (32 output channels), the B operand 32 consecutive pixels, so a lane's accumulator holds one pixel
//                                and 4 x 4 consecutive channels: NHWC stores are 8 bytes, NCHW stores run along the pixels.  A workgroup of WM x WN waves
//                                owns 32 WM pixels x 32 WN channels.  Per 64-channel chunk of K it stages, once, kh strips of 32 WM + kw - 1 consecutive
//                                pixels (144 B per pixel: 128 B + 16 B against bank conflicts) and serves every tap from them: tap (ky, kx) of pixel p is
//                                strip ky, slot p + kx; a tap outside the image is replaced by zero when the fragment is read.  The next chunk's strips
//                                are loaded into registers before a chunk's MFMAs and written to LDS after them.  The weights come straight
//                                from global memory in fragment order (1 KB per wave and k-step, shared through L2 by every workgroup).
//                                <2,2>: 64 pixels x 64 channels (Cout 256, 512, 576); <1,2>: 32 x 64 (Cout 128, 64 and the two-channel heads).
//                                Epilogues on the fp32 accumulator: bias, ReLU, power-of-two scale; the GRU gate pair (z; r * h); the GRU update.
//   update_pack_kernel           fp32 tensors -> fragments and biases of one launch, rounded to the operand type
//
// 9 launches for MV_UPDATE_FLOW, 11 for MV_UPDATE_COV, on the caller's stream; no atomics, no cross-workgroup waits, no host synchronisation, no allocation.
// Layer table, packed layout, rounding points and summation order: update_block_math.h.
#include "common.h"
#include "update_block_math.h"

namespace {

using namespace ublk;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <bool F16>
__device__ __forceinline__ float widen(uint16_t v) {
    if constexpr (F16) return (float)__builtin_bit_cast(_Float16, v);
    else return __uint_as_float((uint32_t)v << 16);
}
template <bool F16>
__device__ __forceinline__ uint16_t narrow(float f) {      // round to nearest even, as torch's .to(dtype)
    if constexpr (F16) return __builtin_bit_cast(uint16_t, (_Float16)f);
    else {
        uint32_t u = __float_as_uint(f);
        if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    }
}
template <bool F16>
__device__ __forceinline__ void widen4(uint2 v, float* o) {
    o[0] = widen<F16>((uint16_t)(v.x & 0xffffu)); o[1] = widen<F16>((uint16_t)(v.x >> 16));
    o[2] = widen<F16>((uint16_t)(v.y & 0xffffu)); o[3] = widen<F16>((uint16_t)(v.y >> 16));
}
template <bool F16>
__device__ __forceinline__ uint2 narrow4(const float* v) {
    return uint2{(uint32_t)narrow<F16>(v[0]) | ((uint32_t)narrow<F16>(v[1]) << 16), (uint32_t)narrow<F16>(v[2]) | ((uint32_t)narrow<F16>(v[3]) << 16)};
}
__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// ---------------------------------------------------------------------------------------------------------------- launch 0
__global__ __launch_bounds__(256) void update_to_nhwc_kernel(const uint16_t* net, const uint16_t* inp, uint16_t* hx, int P, int channels_last) {
    __shared__ uint16_t tile[64][66];
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
    const bool is_net = c0 < HID;
    const uint16_t* src = is_net ? net : inp;
    const int C = is_net ? HID : INP, cs = is_net ? c0 : c0 - HID;      // channels of the source, first source channel of this block
    if (channels_last) {
        for (int e = threadIdx.x; e < 4096; e += 256) {
            const int px = e >> 6, ch = e & 63, p = p0 + px;
            if (p < P) hx[((size_t)b * P + p) * HXC + c0 + ch] = src[((size_t)b * P + p) * C + cs + ch];
        }
        return;
    }
    for (int e = threadIdx.x; e < 4096; e += 256) {
        const int ch = e >> 6, px = e & 63, p = p0 + px;
        tile[ch][px] = p < P ? src[((size_t)b * C + cs + ch) * P + p] : (uint16_t)0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 4096; e += 256) {
        const int px = e >> 6, ch = e & 63, p = p0 + px;
        if (p < P) hx[((size_t)b * P + p) * HXC + c0 + ch] = tile[ch][px];
    }
}

// ---------------------------------------------------------------------------------------------------------------- the convolutions
struct ConvArgs {
    const uint16_t* src0;     // K channels [0, s0_ch): src0[m * s0_stride + ch]
    const uint16_t* src1;     // the rest: src1[m * s1_stride + ch - s0_ch]
    int s0_stride, s0_ch, s1_stride;
    const uint4* w;           // packed fragments
    const float* bias;        // [cout_pad]
    int M, P, H, W, kh, kw, nchunks;
    int epi, relu, cout;      // cout: live rows (NCHW stores)
    float scale;
    uint16_t* dst;            // EPI_STORE: NHWC [M, dst_stride] or null
    int dst_stride;
    uint16_t* nchw;           // [B, cout, H, W] or null
    uint16_t *hx, *z, *rh;    // EPI_GATES / EPI_UPDATE
};

constexpr int PSTR = 9;       // 16-byte units per staged pixel (8 of data)

template <bool F16, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void update_conv_kernel(ConvArgs a) {
    constexpr int BM = 32 * WM, NT = 64 * WM * WN;
    __shared__ uint4 lds[5 * BM * PSTR];      // 5x1: 5 strips of BM; 3x3: 3 (BM + 2); 1x5: BM + 4; 1x1: BM pixels
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, wm = wave % WM, wn = wave / WM, hf = l >> 5;
    const int m0 = blockIdx.x * BM, n0 = (blockIdx.y * WN + wn) * 32;
    const int SW = BM + a.kw - 1, ry = a.kh >> 1, rx = a.kw >> 1, taps = a.kh * a.kw;
    const int pl = wm * 32 + (l & 31), m = m0 + pl;      // this lane's pixel: column l & 31 of the wave's tile
    const bool mok = m < a.M;
    const int mm = mok ? m : 0, b = mm / a.P, p = mm - b * a.P, y = p / a.W, x = p - y * a.W;

    // C layout of 32x32x16: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 bv = *(const float4*)(a.bias + n0 + 8 * g + 4 * hf);
        acc[4 * g] = bv.x; acc[4 * g + 1] = bv.y; acc[4 * g + 2] = bv.z; acc[4 * g + 3] = bv.w;
    }
    const uint4* wp = a.w + (size_t)(n0 >> 5) * ((size_t)a.nchunks * taps * (CK / 16)) * 64 + l;

    // Staging: thread-owned 16-byte pieces (slot = strip pixel, part = 8 channels), NST per thread.  The pieces of chunk c + 1 are loaded into registers
    // before the MFMAs of chunk c are issued and written to LDS after them, so their latency hides behind a chunk's arithmetic.
    constexpr int NST = (5 * BM * 8 + NT - 1) / NT;
    const int npieces = a.kh * SW * 8;
    uint4 pre[NST];
    auto load_chunk = [&](int chunk) {
        const bool from0 = chunk * CK < a.s0_ch;
        const uint16_t* sp = from0 ? a.src0 + chunk * CK : a.src1 + (chunk * CK - a.s0_ch);
        const int sstr = from0 ? a.s0_stride : a.s1_stride;
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = threadIdx.x + i * NT;
            const int part = e & 7, slot = e >> 3, sy = slot / SW, sx = slot - sy * SW;
            const int ms = m0 + (sy - ry) * a.W + sx - rx;  // linear pixel: the tap's own pixel wherever the tap lies inside the image
            pre[i] = uint4{0, 0, 0, 0};
            if (e < npieces && ms >= 0 && ms < a.M) pre[i] = *(const uint4*)(sp + (size_t)ms * sstr + part * 8);
        }
    };
    load_chunk(0);
    for (int chunk = 0; chunk < a.nchunks; ++chunk) {
        __syncthreads();                                   // the previous chunk's fragments have been read
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = threadIdx.x + i * NT;
            if (e < npieces) lds[(e >> 3) * PSTR + (e & 7)] = pre[i];
        }
        __syncthreads();
        if (chunk + 1 < a.nchunks) load_chunk(chunk + 1);
        for (int t = 0; t < taps; ++t) {
            const int ty = t / a.kw, tx = t - ty * a.kw;
            const int yy = y + ty - ry, xx = x + tx - rx;
            const bool ok = mok && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
            const uint4* ap = lds + (ty * SW + pl + tx) * PSTR + hf;
            uint4 wv[CK / 16], av[CK / 16];
#pragma unroll
            for (int ks = 0; ks < CK / 16; ++ks) wv[ks] = wp[ks * 64];
#pragma unroll
            for (int ks = 0; ks < CK / 16; ++ks) av[ks] = ok ? ap[2 * ks] : uint4{0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < CK / 16; ++ks) {
                if constexpr (F16) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wv[ks]), __builtin_bit_cast(f16x8, av[ks]), acc, 0, 0, 0);
                else acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wv[ks]), __builtin_bit_cast(bf16x8, av[ks]), acc, 0, 0, 0);
            }
            wp += (CK / 16) * 64;
        }
    }
    if (!mok) return;

#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int c = n0 + 8 * g + 4 * hf;                 // four consecutive channels
        float v[4] = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        if (a.epi == EPI_GATES) {
            if (c < HID) {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = sigmoidf(v[i]);
                *(uint2*)(a.z + (size_t)m * HID + c) = narrow4<F16>(v);
            } else {
                float h[4];
                widen4<F16>(*(const uint2*)(a.hx + (size_t)m * HXC + c - HID), h);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = sigmoidf(v[i]) * h[i];
                *(uint2*)(a.rh + (size_t)m * HID + c - HID) = narrow4<F16>(v);
            }
        } else if (a.epi == EPI_UPDATE) {
            float h[4], z[4];
            widen4<F16>(*(const uint2*)(a.hx + (size_t)m * HXC + c), h);
            widen4<F16>(*(const uint2*)(a.z + (size_t)m * HID + c), z);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (1.f - z[i]) * h[i] + z[i] * tanhf(v[i]);
            const uint2 o = narrow4<F16>(v);
            *(uint2*)(a.hx + (size_t)m * HXC + c) = o;
            if (a.nchw) {
                const uint16_t o4[4] = {(uint16_t)(o.x & 0xffffu), (uint16_t)(o.x >> 16), (uint16_t)(o.y & 0xffffu), (uint16_t)(o.y >> 16)};
#pragma unroll
                for (int i = 0; i < 4; ++i) a.nchw[((size_t)b * a.cout + c + i) * a.P + p] = o4[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (a.relu) v[i] = v[i] < 0.f ? 0.f : v[i];      // torch's ReLU: NaN stays NaN
                v[i] *= a.scale;
            }
            const uint2 o = narrow4<F16>(v);
            if (a.dst) *(uint2*)(a.dst + (size_t)m * a.dst_stride + c) = o;
            if (a.nchw) {
                const uint16_t o4[4] = {(uint16_t)(o.x & 0xffffu), (uint16_t)(o.x >> 16), (uint16_t)(o.y & 0xffffu), (uint16_t)(o.y >> 16)};
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (c + i < a.cout) a.nchw[((size_t)b * a.cout + c + i) * a.P + p] = o4[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- packing
struct PackArgs {
    const float *w0, *w1, *b0, *b1;
    Conv c;
    uint16_t* wout;
    float* bout;
};

template <bool F16>
__global__ __launch_bounds__(256) void update_pack_kernel(PackArgs a) {
    const Conv& c = a.c;
    const int taps = c.kh * c.kw, K = taps * c.cin;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, nw = (size_t)c.cout_pad * K;
    if (e < nw) {
        const int row = (int)(e / K), k = (int)(e - (size_t)row * K);
        int tap, ch;
        k_source(c, k, tap, ch);
        float v = 0.f;
        if (row < c.rows[0]) v = a.w0[((size_t)row * c.cin + ch) * taps + tap];
        else if (row < c.cout) v = a.w1[((size_t)(row - c.rows[0]) * c.cin + ch) * taps + tap];
        a.wout[packed_w_index(c, row, k)] = narrow<F16>(v);
    } else if (e < nw + c.cout_pad) {
        const int row = (int)(e - nw);
        float v = 0.f;
        if (row < c.rows[0]) v = a.b0[row];
        else if (row < c.cout) v = a.b1[row - c.rows[0]];
        a.bout[row] = widen<F16>(narrow<F16>(v));
    }
}

const Plan* plan(int kind) {
    static Plan p[N_KINDS];
    static const bool ok = (build_plan(p[0], 0), build_plan(p[1], 1), true);
    return ok && kind >= 0 && kind < N_KINDS ? &p[kind] : nullptr;
}

template <bool F16>
void launch_conv(int cfg, const ConvArgs& a, int cout_pad, hipStream_t st) {
    if (cfg == 0) hipLaunchKernelGGL((update_conv_kernel<F16, 2, 2>), dim3(mv_ceil_div(a.M, 64), cout_pad / 64), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((update_conv_kernel<F16, 1, 2>), dim3(mv_ceil_div(a.M, 32), cout_pad / 64), dim3(128), 0, st, a);
}

bool operand_ok(int operand) { return operand == MV_F16 || operand == MV_BF16; }

}  // namespace

extern "C" int mv_update_block_tensor_count(int kind) {
    const Plan* p = plan(kind);
    return p ? p->n_tensors : 0;
}

extern "C" int mv_update_block_tensor_info(int kind, int i, char* name_buf /* >= 64 bytes */, int32_t* shape /* [4] */, int32_t* ndim) {
    const Plan* p = plan(kind);
    MV_CHECK_ARG(p && i >= 0 && i < p->n_tensors && name_buf && shape && ndim);
    const Tensor& t = p->tensors[i];
    memcpy(name_buf, t.name, sizeof(t.name));
    for (int d = 0; d < 4; ++d) shape[d] = d < t.ndim ? t.shape[d] : 0;
    *ndim = t.ndim;
    return MV_OK;
}

extern "C" size_t mv_update_block_packed_bytes(int kind, int operand) {
    const Plan* p = plan(kind);
    return p && operand_ok(operand) ? p->packed_bytes : 0;
}

extern "C" size_t mv_update_block_workspace_bytes(int kind, int B, int H, int W) {
    if (!plan(kind) || B < 1 || H < 1 || W < 1 || (int64_t)B * H * W > MAX_PIXELS) return 0;
    return ws_bytes(B * H * W);
}

extern "C" int mv_update_block_pack(int kind, int operand, const float* const* tensors, void* packed, mvStream_t stream) {
    const Plan* p = plan(kind);
    MV_CHECK_ARG(p && operand_ok(operand) && tensors && packed);
    for (int i = 0; i < p->n_tensors; ++i) MV_CHECK_ARG(tensors[i]);
    for (int ci = 0; ci < p->n_convs; ++ci) {
        PackArgs a;
        a.c = p->convs[ci];
        a.w0 = tensors[a.c.t_w[0]]; a.b0 = tensors[a.c.t_b[0]];
        a.w1 = tensors[a.c.t_w[1]]; a.b1 = tensors[a.c.t_b[1]];
        a.wout = (uint16_t*)((char*)packed + a.c.w_off);
        a.bout = (float*)((char*)packed + a.c.b_off);
        const size_t n = (size_t)a.c.cout_pad * a.c.kh * a.c.kw * a.c.cin + a.c.cout_pad;
        const dim3 grid((unsigned)((n + 255) / 256));
        if (operand == MV_F16) hipLaunchKernelGGL(update_pack_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL(update_pack_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    }
    return mv_launch_status();
}

extern "C" int mv_update_block_forward(int kind, int operand, const void* packed, const void* net, const void* inp, int B, int H, int W, int channels_last,
                                       void* net_out, void* delta, void* mask, void* workspace, mvStream_t stream) {
    const Plan* p = plan(kind);
    MV_CHECK_ARG(p && operand_ok(operand) && packed && net && inp && net_out && delta && mask && workspace);
    MV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && (int64_t)B * H * W <= MAX_PIXELS && (channels_last == 0 || channels_last == 1));
    const int P = H * W, M = B * P;
    hipStream_t st = (hipStream_t)stream;
    uint16_t* buf[N_BUFS];
    buf[0] = (uint16_t*)workspace;
    for (int i = 1; i < N_BUFS; ++i) buf[i] = buf[i - 1] + (size_t)M * BUF_CH[i - 1];
    hipLaunchKernelGGL(update_to_nhwc_kernel, dim3(mv_ceil_div(P, 64), HXC / 64, B), dim3(256), 0, st, (const uint16_t*)net, (const uint16_t*)inp, buf[BUF_HX], P,
                       channels_last);
    uint16_t* outs[4] = {nullptr, (uint16_t*)net_out, (uint16_t*)delta, (uint16_t*)mask};
    for (int ci = 0; ci < p->n_convs; ++ci) {
        const Conv& c = p->convs[ci];
        ConvArgs a;
        a.src0 = buf[c.src0] + c.src0_off; a.s0_stride = BUF_CH[c.src0]; a.s0_ch = c.src0_ch;
        a.src1 = c.src1 == BUF_NONE ? nullptr : buf[c.src1] + c.src1_off;
        a.s1_stride = c.src1 == BUF_NONE ? 0 : BUF_CH[c.src1];
        a.w = (const uint4*)((const char*)packed + c.w_off);
        a.bias = (const float*)((const char*)packed + c.b_off);
        a.M = M; a.P = P; a.H = H; a.W = W; a.kh = c.kh; a.kw = c.kw; a.nchunks = c.cin / CK;
        a.epi = c.epi; a.relu = c.relu; a.cout = c.cout; a.scale = c.scale;
        a.dst = c.dst == BUF_NONE ? nullptr : buf[c.dst];
        a.dst_stride = c.dst == BUF_NONE ? 0 : BUF_CH[c.dst];
        a.nchw = outs[c.nchw];
        a.hx = buf[BUF_HX]; a.z = buf[BUF_Z]; a.rh = buf[BUF_RH];
        if (operand == MV_F16) launch_conv<true>(c.cfg, a, c.cout_pad, st);
        else launch_conv<false>(c.cfg, a, c.cout_pad, st);
    }
    return mv_launch_status();
}
