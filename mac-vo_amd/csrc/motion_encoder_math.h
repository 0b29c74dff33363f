// The decoder's motion encoder (FlowFormer's GMAUpdateBlock.encoder, called at covhead.py:106): layer table, packed weight layout, workspace layout and
// rounding points of csrc/motion_encoder.hip.  Host and device; tests/motion_encoder_twin.py states the same things.
//
//   cor = relu(convc2(relu(convc1(corr))));  flo = relu(convf2(relu(convf1(flow))));  out = cat([relu(conv(cat([cor, flo]))), flow])
//
// Tensors (state_dict order; every weight [cout, cin, kh, kw], every bias [cout]):
//   convc1 [256,145,1,1], convc2 [192,256,3,3], convf1 [128,2,7,7], convf2 [64,128,3,3], conv [126,256,3,3]
//
// Workspace (NHWC, 16-bit, M = B H W pixels; 1 920 B per pixel):  CORR [M,192] | FIM [M,128] | C1 [M,256] | F1 [M,128] | CF [M,256]
//
// Launches (GEMMs of update_conv_dev.h: rows = output channels, columns = pixels m = (b, y, x), K = [64-channel chunk][tap (ky, kx)][channel in chunk]):
//   0  motion_stage_kernel: corr (NCHW or channels-last) -> CORR, channels 0..144 live, 145..191 STORED as zero;
//                           flow -> FIM = the 7x7 im2col of the two flow channels in (channel, tap) order: column k = ch * 49 + ky * 7 + kx holds
//                           flow[b, ch, y + ky - 3, x + kx - 3], zero where that lies outside the image; columns 98..127 STORED as zero.  (channel, tap)
//                           is the order of convf1.weight's own memory, so its [128, 98] matrix is packed as a 1x1 convolution as it lies;
//                           flow -> channels 126..127 of the output, bit for bit
//   1  convc1  1x1  CORR (192 = 145 + 47 zero-padded weight columns) -> 256, ReLU -> C1
//   2  convc2  3x3  C1 -> 192, ReLU -> CF[:, 0:192]
//   3  convf1  1x1  FIM (128 = 98 + 30 zero-padded weight columns) -> 128, ReLU -> F1
//   4  convf2  3x3  F1 -> 64, ReLU -> CF[:, 192:256]
//   5  conv    3x3  CF -> 126 of 128 packed rows, ReLU -> output channels 0..125 (NCHW [B,128,H,W])
// Neither torch.cat exists as a copy.  The padded weight columns are zero AND the padded workspace columns are stored as zero by launch 0: the workspace may
// hold anything on entry, and zero times a NaN bit pattern is NaN.
//
// Rounding: weights and biases are rounded to the operand type when packed; every product is exact in the fp32 accumulator; bias and ReLU are fp32 on the
// accumulator; a value is rounded (to nearest even) exactly once where it is stored: C1, CF (both parts), F1, output channels 0..125.  flow passes through
// exactly.  Summation order of one output: bias first, then K in the order above, 16 k per MFMA; fixed, so two calls return the same bits, and NCHW and
// channels-last inputs give the same bits.
#pragma once
#include "update_block_math.h"

namespace menc {

constexpr int CORR_C = 145, CORR_PAD = 192;             // correlation features: 64 latent + 81 window cells, padded to whole 64-channel chunks
constexpr int FLOW_TAPS = 49, FIM_LIVE = 2 * FLOW_TAPS, FIM_C = 128;
constexpr int OUT_C = 128, OUT_LIVE = 126;              // output channels; those the last convolution writes
constexpr int MAX_PIXELS = ublk::MAX_PIXELS;
constexpr int N_TENSORS = 10, N_LAYERS = 5;

enum Buf { BUF_CORR = 0, BUF_FIM, BUF_C1, BUF_F1, BUF_CF, N_BUFS, BUF_OUT = -1 };
constexpr int BUF_CH[N_BUFS] = {CORR_PAD, FIM_C, 256, 128, 256};

struct Layer {
    const char* name;
    int cout, cin_src, kh_src, kw_src;    // the module's tensor [cout, cin_src, kh_src, kw_src]
    int kh, kw, cin;                      // the launch: kernel and (padded) input channels; kh * kw * cin >= cin_src * kh_src * kw_src
    int pack_cin_src;                     // input channels of the tensor seen as [cout, pack_cin_src, kh, kw] (145; 98 = 2 * 49 for convf1 as 1x1)
    int src, dst, dst_off;                // workspace buffers; BUF_OUT: the NCHW output
    int cfg;                              // tile configuration of update_conv_dev.h: 0 = 64 px x 64 ch, 1 = 32 px x 64 ch
};

constexpr Layer LAYERS[N_LAYERS] = {
    {"convc1", 256, CORR_C, 1, 1, 1, 1, CORR_PAD, CORR_C, BUF_CORR, BUF_C1, 0, 0},
    {"convc2", 192, 256, 3, 3, 3, 3, 256, 256, BUF_C1, BUF_CF, 0, 0},
    {"convf1", 128, 2, 7, 7, 1, 1, FIM_C, FIM_LIVE, BUF_FIM, BUF_F1, 0, 1},
    {"convf2", 64, 128, 3, 3, 3, 3, 128, 128, BUF_F1, BUF_CF, 192, 1},
    {"conv", OUT_LIVE, 256, 3, 3, 3, 3, 256, 256, BUF_CF, BUF_OUT, 0, 1},
};

// Tensor i of the table: 2 l = LAYERS[l]'s weight, 2 l + 1 its bias.
inline void tensor_info(int i, ublk::Tensor& t) {
    const Layer& l = LAYERS[i >> 1];
    memset(&t, 0, sizeof(t));
    if (i & 1) {
        snprintf(t.name, sizeof(t.name), "%s.bias", l.name);
        t.shape[0] = l.cout; t.ndim = 1;
    } else {
        snprintf(t.name, sizeof(t.name), "%s.weight", l.name);
        t.shape[0] = l.cout; t.shape[1] = l.cin_src; t.shape[2] = l.kh_src; t.shape[3] = l.kw_src; t.ndim = 4;
    }
}

// The packed form of layer l as update_conv_dev.h reads it (fragments of packed_w_index, then cout_pad fp32 biases), the layers one after the other.
inline ublk::Conv packed_conv(int l) {
    ublk::Conv c;
    size_t off = 0;
    for (int i = 0; i <= l; ++i) {
        const Layer& L = LAYERS[i];
        memset(&c, 0, sizeof(c));
        c.kh = L.kh; c.kw = L.kw; c.cin = L.cin;
        c.cout = L.cout; c.cout_pad = (L.cout + 63) / 64 * 64;
        c.t_w[0] = 2 * i; c.t_b[0] = 2 * i + 1; c.rows[0] = L.cout;
        c.relu = 1; c.scale = 1.f; c.epi = ublk::EPI_STORE; c.cfg = L.cfg;
        c.w_off = off;
        off += (size_t)c.cout_pad * c.kh * c.kw * c.cin * 2;
        c.b_off = off;
        off += (size_t)c.cout_pad * 4;
    }
    return c;
}

inline size_t packed_bytes() {
    const ublk::Conv c = packed_conv(N_LAYERS - 1);
    return c.b_off + (size_t)c.cout_pad * 4;
}

inline size_t ws_bytes(int M) {
    size_t n = 0;
    for (int b = 0; b < N_BUFS; ++b) n += (size_t)M * BUF_CH[b] * 2;
    return n;
}

}  // namespace menc
