// Forward of the TartanVO PoseNet that TartanMotionNet runs between a frame's enqueue and its finish (VOFlowRes config 1, stereo, down_scale,
// intrinsic; FlowPoseNet.py:45-166, StereoVO.py:21): [lanes, 5, 112, 160] fp32 -> [lanes, 6] raw motion, fp32 weights, activations and sums.
//
//   posenet_conv_kernel<MT,NT,KS,U>  one 3 x 3 convolution as an implicit GEMM on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32): a workgroup of KS
//                                    waves owns MT x NT tiles of 16 pixels x 16 channels and splits K over its waves; A comes straight from the
//                                    NCHW map (16 consecutive pixels x 4 channels per load, borders by predicate), B from the packed weights (one
//                                    256 B line per wave and step), U steps' loads at a time.  The partial sums meet in LDS in wave order; the epilogue adds the identity
//                                    and applies ReLU.  A layer's first block folds its 1 x 1 stride-2 downsample in as further K rows.
//                                    <2,2,4,8> serves the 56x80 and 28x40 maps, <1,1,8,16> the 14x20 and smaller ones: there M is 6..280 rows per lane
//                                    and a layer streams up to 2.4 MB of weights, so the grid tiles Cout by 16 (16 workgroups of 8 waves at 2x3).
//   posenet_head_kernel              the six linear layers, one workgroup per lane
//
// 3 + 2 * 23 + 1 = 50 launches on the caller's stream; no host synchronisation, no allocation, no atomics, no cross-workgroup wait.
// Layer table, packed layout and the summation order of every output: posenet_math.h (shared with the host twin of the tests).
#include "common.h"
#include "posenet_math.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

struct ConvArgs {
    const float* x;      // [lanes, cin, hin, win]
    const float* x2;     // downsample input [lanes, cin2, hin2, win2] or null
    const float* res;    // identity [lanes, cout, hout, wout] or null
    const float* w;      // packed weights of this launch
    const float* bias;   // [cout]
    float* y;            // [lanes, cout, hout, wout]
    int M, P, wout;      // rows (lanes * P), pixels per lane, output width
    int cin, cin4, hin, win, stride;   // cin4 = padded channels / 4
    int cin2, hin2, win2;
    int cout, K4a, K4;
};

template <int MT, int NT, int KS, int U>
__global__ __launch_bounds__(KS * 64) void posenet_conv_kernel(ConvArgs a) {
    __shared__ float part[KS][MT * NT * 4][64];
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, r = l & 15, kq = l >> 4;
    const int tile_m0 = blockIdx.x * MT, tile_n0 = blockIdx.y * NT;

    // this lane's A rows: one output pixel per M tile
    bool mok[MT];
    int oy[MT], ox[MT];
    const float *xb[MT], *x2b[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = (tile_m0 + i) * 16 + r;
        mok[i] = m < a.M;
        const int mm = mok[i] ? m : 0;
        const int lane = mm / a.P, p = mm - lane * a.P;
        oy[i] = p / a.wout;
        ox[i] = p - oy[i] * a.wout;
        xb[i] = a.x + (size_t)lane * a.cin * a.hin * a.win;
        x2b[i] = a.x2 ? a.x2 + (size_t)lane * a.cin2 * a.hin2 * a.win2 : nullptr;
    }
    const float* wb[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) wb[j] = a.w + (size_t)(tile_n0 + j) * a.K4 * 64 + l;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const float b0 = wave == 0 ? a.bias[(tile_n0 + j) * 16 + r] : 0.f;   // C layout: column = lane & 15 in all four registers
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i][j] = f32x4{b0, b0, b0, b0};
    }

    const int k4b = posenet::split_begin(a.K4, KS, wave), k4e = posenet::split_begin(a.K4, KS, wave + 1);
    const int ntap = a.cin2 ? 10 : 9;
    for (int t = 0; t < ntap; ++t) {
        const int seg_lo = t < 9 ? t * a.cin4 : a.K4a, seg_hi = t < 9 ? seg_lo + a.cin4 : a.K4;
        const int lo = seg_lo > k4b ? seg_lo : k4b, hi = seg_hi < k4e ? seg_hi : k4e;
        if (lo >= hi) continue;
        const float* ap[MT];
        bool ok[MT];
        int chw, creal;
        if (t < 9) {
            const int ky = t / 3, kx = t - 3 * ky;
            chw = a.hin * a.win;
            creal = a.cin;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int iy = oy[i] * a.stride - 1 + ky, ix = ox[i] * a.stride - 1 + kx;
                ok[i] = mok[i] && iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win;
                ap[i] = xb[i] + (ok[i] ? iy * a.win + ix : 0);
            }
        } else {
            chw = a.hin2 * a.win2;
            creal = a.cin2;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                ok[i] = mok[i];
                ap[i] = x2b[i] + (ok[i] ? 2 * oy[i] * a.win2 + 2 * ox[i] : 0);
            }
        }
        // U steps per round: their 2 U loads are issued together, then the MFMAs in k order (a wave's chain is latency-bound otherwise); the
        // steps of a last, partial round are skipped by wave-uniform branches
        for (int k4 = lo; k4 < hi; k4 += U) {
            float av[U][MT], bv[U][NT];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = (k4 + u - seg_lo) * 4 + kq;
                const bool live = k4 + u < hi;
#pragma unroll
                for (int i = 0; i < MT; ++i) av[u][i] = (live && ok[i] && c < creal) ? ap[i][(size_t)c * chw] : 0.f;
#pragma unroll
                for (int j = 0; j < NT; ++j) bv[u][j] = live ? wb[j][(size_t)(k4 + u) * 64] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (k4 + u < hi) {
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][i], bv[u][j], acc[i][j], 0, 0, 0);
                }
            }
        }
    }

    // the waves' partial sums, combined in wave order; C layout: row = 4 * (lane >> 4) + register, column = lane & 15
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) part[wave][(i * NT + j) * 4 + q][l] = acc[i][j][q];
    __syncthreads();
    for (int e = threadIdx.x; e < MT * NT * 256; e += KS * 64) {
        const int row = e & 15, col = (e >> 4) & 15, tile = e >> 8;   // consecutive threads = consecutive pixels of one channel
        const int i = tile / NT, j = tile - i * NT;
        const int slot = tile * 4 + (row & 3), pl = (row >> 2) * 16 + col;
        float s = part[0][slot][pl];
#pragma unroll
        for (int w = 1; w < KS; ++w) s += part[w][slot][pl];
        const int m = (tile_m0 + i) * 16 + row, n = (tile_n0 + j) * 16 + col;
        if (m >= a.M) continue;
        const int lane = m / a.P, p = m - lane * a.P;
        const size_t idx = ((size_t)lane * a.cout + n) * a.P + p;
        if (a.res) s += a.res[idx];
        a.y[idx] = posenet::relu(s);
    }
}

struct HeadArgs {
    const float* feat;   // [lanes, 1536]
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    float* out;          // [lanes, 6]
};

__global__ __launch_bounds__(posenet::HEAD_THREADS) void posenet_head_kernel(HeadArgs a) {
    using namespace posenet;
    __shared__ float f[FEAT], p1[HEAD_KS][2 * FC1], h1[2 * FC1], h2[2 * FC2];
    const int t = threadIdx.x, lane = blockIdx.x;
    for (int i = t; i < FEAT; i += HEAD_THREADS) f[i] = a.feat[(size_t)lane * FEAT + i];
    __syncthreads();
    {   // layer 1 of both branches: output j (trans 0..127, rot 128..255), K quarter q
        const int j = t & (2 * FC1 - 1), q = t >> 8;
        constexpr int KQ = FEAT / HEAD_KS;
        float s = q == 0 ? a.b1[j] : 0.f;
#pragma unroll 32
        for (int k = q * KQ; k < (q + 1) * KQ; ++k) s = fmaf(f[k], a.w1[(size_t)k * (2 * FC1) + j], s);
        p1[q][j] = s;
    }
    __syncthreads();
    if (t < 2 * FC1) {
        float s = p1[0][t];
#pragma unroll
        for (int q = 1; q < HEAD_KS; ++q) s += p1[q][t];
        h1[t] = relu(s);
    }
    __syncthreads();
    if (t < 2 * FC2) {
        const int br = t >> 5;
        float s = a.b2[t];
        for (int k = 0; k < FC1; ++k) s = fmaf(h1[br * FC1 + k], a.w2[k * (2 * FC2) + t], s);
        h2[t] = relu(s);
    }
    __syncthreads();
    if (t < 2 * FC3) {
        const int br = t / FC3;
        float s = a.b3[t];
        for (int k = 0; k < FC2; ++k) s = fmaf(h2[br * FC2 + k], a.w3[k * 8 + t], s);
        a.out[(size_t)lane * OUT_N + t] = s;
    }
}

const posenet::Plan* plan() {
    static posenet::Plan p;
    static const bool ok = posenet::build_plan(p);
    return ok ? &p : nullptr;
}

template <int CFG>
void launch_conv(const ConvArgs& a, hipStream_t stream) {
    constexpr int MT = posenet::CFG_MT[CFG], NT = posenet::CFG_NT[CFG], KS = posenet::CFG_KS[CFG];
    constexpr int U = 32 / (MT + NT);   // 32 loads in flight per lane
    dim3 grid(mv_ceil_div(a.M, MT * 16), a.cout / (NT * 16));
    hipLaunchKernelGGL((posenet_conv_kernel<MT, NT, KS, U>), grid, dim3(KS * 64), 0, stream, a);
}

}  // namespace

extern "C" int mv_posenet_tensor_count(void) { return posenet::N_TENSORS; }

extern "C" int mv_posenet_tensor_info(int i, char* name_buf /* >= 64 bytes */, int32_t* shape /* [4] */, int32_t* ndim) {
    const posenet::Plan* p = plan();
    MV_CHECK_ARG(p && i >= 0 && i < posenet::N_TENSORS && name_buf && shape && ndim);
    const posenet::Tensor& t = p->tensors[i];
    memcpy(name_buf, t.name, sizeof(t.name));
    for (int d = 0; d < 4; ++d) shape[d] = d < t.ndim ? t.shape[d] : 0;
    *ndim = t.ndim;
    return MV_OK;
}

extern "C" size_t mv_posenet_packed_bytes(void) {
    const posenet::Plan* p = plan();
    return p ? (size_t)p->packed_floats * sizeof(float) : 0;
}

extern "C" size_t mv_posenet_workspace_bytes(int lanes) {
    if (lanes < 1 || lanes > MV_MAX_LANES) return 0;
    return (size_t)lanes * posenet::WS_FLOATS_PER_LANE * sizeof(float);
}

extern "C" int mv_posenet_pack(const float* const* tensors_host, void* packed_host) {
    using namespace posenet;
    const Plan* p = plan();
    MV_CHECK_ARG(p && tensors_host && packed_host);
    for (int i = 0; i < N_TENSORS; ++i) MV_CHECK_ARG(tensors_host[i]);
    float* out = (float*)packed_host;
    for (int ci = 0; ci < N_CONVS; ++ci) {
        const Conv& c = p->convs[ci];
        const float* w = tensors_host[c.t_w];
        const float* dw = c.t_dsw >= 0 ? tensors_host[c.t_dsw] : nullptr;
        for (int n = 0; n < c.cout; ++n) {
            for (int k4 = 0; k4 < c.K4; ++k4)
                for (int kq = 0; kq < 4; ++kq) {
                    int tap, ch;
                    k_source(c, k4, kq, tap, ch);
                    float v;
                    if (tap < 9) v = ch < c.cin ? w[((size_t)n * c.cin + ch) * 9 + tap] : 0.f;
                    else v = dw[(size_t)n * c.ds_cin + ch];
                    out[packed_w_index(c, n, k4, kq)] = v;
                }
            const float b = tensors_host[c.t_b][n];
            out[c.b_off + n] = c.t_dsb >= 0 ? b + tensors_host[c.t_dsb][n] : b;
        }
    }
    const Head& h = p->head;
    for (int r = 0; r < 2; ++r) {
        const float *w1 = tensors_host[h.t_w[r][0]], *w2 = tensors_host[h.t_w[r][1]], *w3 = tensors_host[h.t_w[r][2]];
        for (int j = 0; j < FC1; ++j) {
            for (int k = 0; k < FEAT; ++k) out[h.w1 + (size_t)k * (2 * FC1) + r * FC1 + j] = w1[(size_t)j * FEAT + k];
            out[h.b1 + r * FC1 + j] = tensors_host[h.t_b[r][0]][j];
        }
        for (int j = 0; j < FC2; ++j) {
            for (int k = 0; k < FC1; ++k) out[h.w2 + k * (2 * FC2) + r * FC2 + j] = w2[j * FC1 + k];
            out[h.b2 + r * FC2 + j] = tensors_host[h.t_b[r][1]][j];
        }
        for (int j = 0; j < FC3; ++j) {
            for (int k = 0; k < FC2; ++k) out[h.w3 + k * 8 + r * FC3 + j] = w3[j * FC2 + k];
            out[h.b3 + r * FC3 + j] = tensors_host[h.t_b[r][2]][j];
        }
    }
    for (int k = 0; k < FC2; ++k) out[h.w3 + k * 8 + 6] = out[h.w3 + k * 8 + 7] = 0.f;
    out[h.b3 + 6] = out[h.b3 + 7] = 0.f;
    return MV_OK;
}

extern "C" int mv_posenet_forward_lanes(const void* packed_dev, const float* x, int lanes, float* out, void* workspace,
                                        float* const* stage_out, mvStream_t stream) {
    using namespace posenet;
    const Plan* p = plan();
    MV_CHECK_ARG(p && packed_dev && x && out && workspace);
    MV_CHECK_ARG(lanes >= 1 && lanes <= MV_MAX_LANES);
    const float* pk = (const float*)packed_dev;
    float* ws[3];
    ws[0] = (float*)workspace;
    ws[1] = ws[0] + (size_t)lanes * BUF_FLOATS[0];
    ws[2] = ws[1] + (size_t)lanes * BUF_FLOATS[1];
    float* buf[3] = {ws[0], ws[1], ws[2]};
    hipStream_t st = (hipStream_t)stream;
    int last = 0;
    for (int ci = 0; ci < N_CONVS; ++ci) {
        const Conv& c = p->convs[ci];
        // a stage the caller asked for is written to the caller's buffer, and the next launches read it from there
        buf[c.dst] = (c.stage >= 0 && stage_out && stage_out[c.stage]) ? stage_out[c.stage] : ws[c.dst];
        ConvArgs a;
        a.x = c.src < 0 ? x : buf[c.src];
        a.x2 = c.ds_cin ? buf[c.res] : nullptr;
        a.res = c.residual ? buf[c.res] : nullptr;
        a.w = pk + c.w_off;
        a.bias = pk + c.b_off;
        a.y = buf[c.dst];
        a.P = c.hout * c.wout;
        a.M = lanes * a.P;
        a.wout = c.wout;
        a.cin = c.cin; a.cin4 = c.cin_pad >> 2; a.hin = c.hin; a.win = c.win; a.stride = c.stride;
        a.cin2 = c.ds_cin; a.hin2 = c.ds_hin; a.win2 = c.ds_win;
        a.cout = c.cout; a.K4a = c.K4a; a.K4 = c.K4;
        if (c.cfg == 0) launch_conv<0>(a, st);
        else launch_conv<1>(a, st);
        last = c.dst;
    }
    HeadArgs h;
    h.feat = buf[last];
    h.w1 = pk + p->head.w1; h.b1 = pk + p->head.b1;
    h.w2 = pk + p->head.w2; h.b2 = pk + p->head.b2;
    h.w3 = pk + p->head.w3; h.b3 = pk + p->head.b3;
    h.out = out;
    hipLaunchKernelGGL(posenet_head_kernel, dim3(lanes), dim3(HEAD_THREADS), 0, st, h);
    return mv_launch_status();
}
