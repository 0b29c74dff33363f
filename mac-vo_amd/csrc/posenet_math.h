// The TartanVO PoseNet (VOFlowRes config 1, stereo, down_scale, intrinsic: Module/Network/TartanVOStereo/FlowPoseNet.py:45-166) as a launch
// plan: the canonical tensor list, the layer table, the packed weight layout and the order in which every output sums its products.  Plain
// C++ without a device dependency: posenet.hip (the kernels, the packer) and tests/c_abi/posenet_twin.cpp (the host replay) both include it, so
// the kernel and its twin cannot disagree on a border, a stride, a K range or a weight's place.
//
// One convolution launch is the implicit GEMM  Y[m][n] = act(sum_k A[m][k] W[k][n] + bias[n] (+ identity[m][n])),
//   m = lane * P + oy * wout + ox  (P = hout * wout; the lanes of a batch are further rows, nothing else),
//   n = output channel,
//   k = tap * cin_pad + c for the 3 x 3 taps (tap = 3 ky + kx, input pixel (oy * stride - 1 + ky, ox * stride - 1 + kx), zero outside the map and
//       for the padded channels c >= cin), followed — in the second launch of a layer's first block — by the ds_cin rows of the block's 1 x 1
//       stride-2 downsample, which read the BLOCK's input at (2 oy, 2 ox).
// K is walked in steps of 4 (one 16x16x4 fp32 MFMA).  The K4 steps are split over the KS waves of a workgroup: wave w owns the steps
// [split_begin(K4, KS, w), split_begin(K4, KS, w + 1)) and chains acc = fmaf(a, w, acc) over its k in ascending order, wave 0 starting from the bias
// (conv bias + downsample bias, added once in fp32 by the packer), the others from 0.  The partial sums are then added in wave order,
// ((p0 + p1) + p2) + ..., then the identity, then torch's ReLU (NaN stays NaN).  Nothing in that order depends on the lane count or on a row's
// place in a tile, so a lane's bits do not depend on its batch.
//
// The head (six linear layers, one launch, one workgroup per lane): layer 1 of both branches = 256 outputs over the 1536 NCHW-flattened
// features, K split in HEAD_KS contiguous quarters combined in the same wave order; layers 2 and 3 are single chains from the bias.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace posenet {

constexpr int IN_C = 5, IN_H = 112, IN_W = 160, OUT_N = 6;
constexpr int N_TENSORS = 120, N_CONVS = 49, N_STAGES = 6, MAX_LANES = 64;
constexpr int FEAT = 1536, FC1 = 128, FC2 = 32, FC3 = 3;
constexpr int HEAD_KS = 4, HEAD_THREADS = 2 * FC1 * HEAD_KS;   // 1024
constexpr long long N_PARAMS = 15135430;

// the two tilings of the convolution kernel: MT x NT tiles of 16 x 16 outputs per workgroup, K split over KS waves
constexpr int N_CFG = 2;
constexpr int CFG_MT[N_CFG] = {2, 1}, CFG_NT[N_CFG] = {2, 1}, CFG_KS[N_CFG] = {4, 8};

// workspace: three activation buffers per batch (floats per lane): two hold a stage's maps, the third a block's intermediate
constexpr long long BUF_FLOATS[3] = {32LL * 56 * 80, 32LL * 56 * 80, 64LL * 28 * 40};
constexpr long long WS_FLOATS_PER_LANE = BUF_FLOATS[0] + BUF_FLOATS[1] + BUF_FLOATS[2];

struct Tensor {
    char name[64];
    int ndim;
    int shape[4];
};

struct Conv {
    int cin, cin_pad, hin, win, stride, cout, hout, wout;
    int ds_cin, ds_hin, ds_win;      // the folded 1 x 1 stride-2 downsample (0 = none): it reads buffer `res`
    int residual;                    // 1: + identity (buffer `res`, same shape as the output)
    int cfg;                         // index into CFG_*
    int t_w, t_b, t_dsw, t_dsb;      // canonical tensor indices (-1 = none)
    int src, dst, res;               // activation buffers 0..2; src -1 = the network input
    int stage;                       // >= 0: this launch writes stage `stage` (firstconv, layer1..5)
    int K4a, K4;                     // K steps of the 3 x 3 taps, and in total
    long long w_off, b_off;          // float offsets into the packed buffer
};

struct Head {
    int t_w[2][3], t_b[2][3];        // [trans, rot][layer]
    long long w1, b1, w2, b2, w3, b3;   // packed: w1 [1536][256], b1 [256], w2 [128][64], b2 [64], w3 [32][8], b3 [8]
};

struct Plan {
    Tensor tensors[N_TENSORS];
    Conv convs[N_CONVS];
    Head head;
    int stage_c[N_STAGES], stage_h[N_STAGES], stage_w[N_STAGES];
    long long packed_floats;
};

constexpr int split_begin(int K4, int KS, int w) { return (int)((long long)w * K4 / KS); }

// where weight row k = 4 * k4 + kq of output channel n sits in a launch's packed block: per 16-channel tile, K4 steps of 64 floats in the
// B-operand order of the 16x16x4 MFMA (lane l: k = l >> 4, n = l & 15), so a wave's load is one contiguous 256 B line
inline long long packed_w_index(const Conv& c, int n, int k4, int kq) {
    return c.w_off + ((long long)(n >> 4) * c.K4 + k4) * 64 + kq * 16 + (n & 15);
}

// the source of row k = 4 * k4 + kq: tap 0..8 of the 3 x 3 kernel or 9 = the downsample, and the input channel (may be >= cin: padding)
inline void k_source(const Conv& c, int k4, int kq, int& tap, int& ch) {
    const int cin4 = c.cin_pad >> 2;
    if (k4 < c.K4a) {
        tap = k4 / cin4;
        ch = (k4 - tap * cin4) * 4 + kq;
    } else {
        tap = 9;
        ch = (k4 - c.K4a) * 4 + kq;
    }
}

inline int add_tensor(Plan& p, int& nt, const char* name, int ndim, int s0, int s1, int s2, int s3) {
    Tensor& t = p.tensors[nt];
    snprintf(t.name, sizeof(t.name), "%.60s", name);
    t.ndim = ndim;
    t.shape[0] = s0; t.shape[1] = s1; t.shape[2] = s2; t.shape[3] = s3;
    return nt++;
}

inline void add_conv_tensors(Plan& p, int& nt, const char* prefix, int cout, int cin, int k, int& tw, int& tb) {
    char nm[56];
    snprintf(nm, sizeof(nm), "%.40s.weight", prefix);
    tw = add_tensor(p, nt, nm, 4, cout, cin, k, k);
    snprintf(nm, sizeof(nm), "%.40s.bias", prefix);
    tb = add_tensor(p, nt, nm, 1, cout, 0, 0, 0);
}

inline void finish_conv(Conv& c, long long& off) {
    c.K4a = 9 * (c.cin_pad >> 2);
    c.K4 = c.K4a + (c.ds_cin >> 2);
    c.w_off = off;
    off += (long long)c.cout * c.K4 * 4;
    c.b_off = off;
    off += c.cout;
}

// the whole network; returns false if the table does not come out at 120 tensors / 49 launches (a programming error)
inline bool build_plan(Plan& p) {
    memset(&p, 0, sizeof(p));
    int nt = 0, nc = 0;
    long long off = 0;
    char nm[64];
    int cur = 0, C = IN_C, H = IN_H, W = IN_W;
    for (int i = 0; i < 3; ++i) {   // firstconv: 3 x 3 5 -> 32 stride 2, then two 32 -> 32, each + ReLU
        Conv& c = p.convs[nc++];
        snprintf(nm, sizeof(nm), "firstconv.%d.0", i);
        add_conv_tensors(p, nt, nm, 32, C, 3, c.t_w, c.t_b);
        c.t_dsw = c.t_dsb = -1;
        c.cin = C; c.cin_pad = (C + 7) & ~7; c.hin = H; c.win = W; c.stride = i == 0 ? 2 : 1; c.cout = 32;
        c.hout = (H - 1) / c.stride + 1; c.wout = (W - 1) / c.stride + 1;
        c.cfg = 0;
        c.src = i == 0 ? -1 : cur; c.dst = i == 0 ? 0 : cur ^ 1; c.res = -1; c.stage = i == 2 ? 0 : -1;
        finish_conv(c, off);
        cur = c.dst; C = 32; H = c.hout; W = c.wout;
    }
    p.stage_c[0] = C; p.stage_h[0] = H; p.stage_w[0] = W;
    const int blocks[5] = {3, 4, 6, 7, 3}, planes[5] = {64, 128, 128, 256, 256};
    for (int L = 0; L < 5; ++L) {
        for (int b = 0; b < blocks[L]; ++b) {
            const int s = b == 0 ? 2 : 1, Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1, Pn = planes[L];
            Conv& c1 = p.convs[nc++];
            snprintf(nm, sizeof(nm), "layer%d.%d.conv1.0", L + 1, b);
            add_conv_tensors(p, nt, nm, Pn, C, 3, c1.t_w, c1.t_b);
            c1.t_dsw = c1.t_dsb = -1;
            c1.cin = c1.cin_pad = C; c1.hin = H; c1.win = W; c1.stride = s; c1.cout = Pn; c1.hout = Ho; c1.wout = Wo;
            c1.cfg = L == 0 ? 0 : 1;
            c1.src = cur; c1.dst = 2; c1.res = -1; c1.stage = -1;
            finish_conv(c1, off);
            Conv& c2 = p.convs[nc++];
            snprintf(nm, sizeof(nm), "layer%d.%d.conv2", L + 1, b);
            add_conv_tensors(p, nt, nm, Pn, Pn, 3, c2.t_w, c2.t_b);
            c2.t_dsw = c2.t_dsb = -1;
            if (b == 0) {
                snprintf(nm, sizeof(nm), "layer%d.0.downsample", L + 1);
                add_conv_tensors(p, nt, nm, Pn, C, 1, c2.t_dsw, c2.t_dsb);
                c2.ds_cin = C; c2.ds_hin = H; c2.ds_win = W;
            } else {
                c2.residual = 1;
            }
            c2.cin = c2.cin_pad = Pn; c2.hin = Ho; c2.win = Wo; c2.stride = 1; c2.cout = Pn; c2.hout = Ho; c2.wout = Wo;
            c2.cfg = c1.cfg;
            c2.src = 2; c2.dst = cur ^ 1; c2.res = cur; c2.stage = b == blocks[L] - 1 ? L + 1 : -1;
            finish_conv(c2, off);
            cur ^= 1; C = Pn; H = Ho; W = Wo;
        }
        p.stage_c[L + 1] = C; p.stage_h[L + 1] = H; p.stage_w[L + 1] = W;
    }
    const char* br[2] = {"voflow_trans", "voflow_rot"};
    const int fin[3] = {FEAT, FC1, FC2}, fout[3] = {FC1, FC2, FC3};
    for (int r = 0; r < 2; ++r)
        for (int l = 0; l < 3; ++l) {
            snprintf(nm, sizeof(nm), l < 2 ? "%s.%d.0.weight" : "%s.%d.weight", br[r], l);
            p.head.t_w[r][l] = add_tensor(p, nt, nm, 2, fout[l], fin[l], 0, 0);
            snprintf(nm, sizeof(nm), l < 2 ? "%s.%d.0.bias" : "%s.%d.bias", br[r], l);
            p.head.t_b[r][l] = add_tensor(p, nt, nm, 1, fout[l], 0, 0, 0);
        }
    p.head.w1 = off; off += (long long)FEAT * 2 * FC1;
    p.head.b1 = off; off += 2 * FC1;
    p.head.w2 = off; off += (long long)FC1 * 2 * FC2;
    p.head.b2 = off; off += 2 * FC2;
    p.head.w3 = off; off += FC2 * 8;
    p.head.b3 = off; off += 8;
    p.packed_floats = off;
    return nt == N_TENSORS && nc == N_CONVS && C * H * W == FEAT;
}

inline long long tensor_numel(const Tensor& t) {
    long long n = 1;
    for (int d = 0; d < t.ndim; ++d) n *= t.shape[d];
    return n;
}

// torch's ReLU: NaN stays NaN (fmaxf would drop it).  constexpr: callable from the kernel and from the host twin alike
constexpr float relu(float v) { return v < 0.f ? 0.f : v; }

}  // namespace posenet
