// The 16-bit implicit-GEMM convolution family shared by csrc/update_block.hip and csrc/motion_encoder.hip (device code; each includes it once).
//
//   update_conv_kernel<F16,WM,WN> one convolution (1x5, 5x1, 3x3, 1x1; zero padding) as an implicit GEMM on v_mfma_f32_32x32x16_{bf16,f16}: the A operand
//                                is the packed weights (32 output channels), the B operand 32 consecutive pixels, so a lane's accumulator holds one pixel
//                                and 4 x 4 consecutive channels: NHWC stores are 8 bytes, NCHW stores run along the pixels.  A workgroup of WM x WN waves
//                                owns 32 WM pixels x 32 WN channels.  Per 64-channel chunk of K it stages, once, kh strips of 32 WM + kw - 1 consecutive
//                                pixels (144 B per pixel: 128 B + 16 B against bank conflicts) and serves every tap from them: tap (ky, kx) of pixel p is
//                                strip ky, slot p + kx; a tap outside the image is replaced by zero when the fragment is read.  The next chunk's strips
//                                are loaded into registers before a chunk's MFMAs and written to LDS after them.  The weights come straight
//                                from global memory in fragment order (1 KB per wave and k-step, shared through L2 by every workgroup).
//                                <2,2>: 64 pixels x 64 channels (Cout 256, 512, 576, 192); <1,2>: 32 x 64 (Cout 128, 126, 64 and the two-channel heads).
//                                Epilogues on the fp32 accumulator: bias, ReLU, power-of-two scale; the GRU gate pair (z; r * h); the GRU update.
//                                NCHW stores go to a tensor of nchw_ch channels, of which this launch writes rows [0, cout).
//   update_pack_kernel           fp32 tensors -> fragments and biases of one launch, rounded to the operand type; input channels [cin_src, cin) of the
//                                packed layout are zero (a K padded up to whole 64-channel chunks)
//
// Packed layout and k order: update_block_math.h (packed_w_index, k_source).
#pragma once
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

// ---------------------------------------------------------------------------------------------------------------- the convolutions
struct ConvArgs {
    const uint16_t* src0;     // K channels [0, s0_ch): src0[m * s0_stride + ch]
    const uint16_t* src1;     // the rest: src1[m * s1_stride + ch - s0_ch]
    int s0_stride, s0_ch, s1_stride;
    const uint4* w;           // packed fragments
    const float* bias;        // [cout_pad]
    int M, P, H, W, kh, kw, nchunks;
    int epi, relu, cout;      // cout: live rows (NCHW stores)
    int nchw_ch;              // channels of the NCHW tensor (>= cout; the rows go to its channels [0, cout))
    float scale;
    uint16_t* dst;            // EPI_STORE: NHWC [M, dst_stride] or null
    int dst_stride;
    uint16_t* nchw;           // [B, nchw_ch, H, W] or null
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
                for (int i = 0; i < 4; ++i) a.nchw[((size_t)b * a.nchw_ch + c + i) * a.P + p] = o4[i];
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
                    if (c + i < a.cout) a.nchw[((size_t)b * a.nchw_ch + c + i) * a.P + p] = o4[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- packing
struct PackArgs {
    const float *w0, *w1, *b0, *b1;
    Conv c;
    int cin_src;              // input channels of the fp32 tensors (<= c.cin; the packed channels from there on are zero)
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
        if (ch >= a.cin_src) v = 0.f;
        else if (row < c.rows[0]) v = a.w0[((size_t)row * a.cin_src + ch) * taps + tap];
        else if (row < c.cout) v = a.w1[((size_t)(row - c.rows[0]) * a.cin_src + ch) * taps + tap];
        a.wout[packed_w_index(c, row, k)] = narrow<F16>(v);
    } else if (e < nw + c.cout_pad) {
        const int row = (int)(e - nw);
        float v = 0.f;
        if (row < c.rows[0]) v = a.b0[row];
        else if (row < c.cout) v = a.b1[row - c.rows[0]];
        a.bout[row] = widen<F16>(narrow<F16>(v));
    }
}

// one launch of the packer: the stacked tensors of `c` (device fp32) -> packed + c.w_off / c.b_off
inline void launch_pack(int operand, const Conv& c, int cin_src, const float* w0, const float* b0, const float* w1, const float* b1, void* packed, hipStream_t st) {
    PackArgs a;
    a.c = c;
    a.cin_src = cin_src;
    a.w0 = w0; a.b0 = b0; a.w1 = w1; a.b1 = b1;
    a.wout = (uint16_t*)((char*)packed + c.w_off);
    a.bout = (float*)((char*)packed + c.b_off);
    const size_t n = (size_t)c.cout_pad * c.kh * c.kw * c.cin + c.cout_pad;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (operand == MV_F16) hipLaunchKernelGGL(update_pack_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(update_pack_kernel<false>, grid, dim3(256), 0, st, a);
}

template <bool F16>
void launch_conv(int cfg, const ConvArgs& a, int cout_pad, hipStream_t st) {
    if (cfg == 0) hipLaunchKernelGGL((update_conv_kernel<F16, 2, 2>), dim3(mv_ceil_div(a.M, 64), cout_pad / 64), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((update_conv_kernel<F16, 1, 2>), dim3(mv_ceil_div(a.M, 32), cout_pad / 64), dim3(128), 0, st, a);
}

bool operand_ok(int operand) { return operand == MV_F16 || operand == MV_BF16; }

}  // namespace
