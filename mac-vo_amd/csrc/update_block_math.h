// The decoder's recurrent update blocks (covhead.py:24-43 CovUpdateBlock; covhead.py:112-114 = gru, flow_head, mask of FlowFormer's GMAUpdateBlock):
// layer table, packed weight layout and rounding points of csrc/update_block.hip.  Host and device; tests/update_block_twin.py states the same things.
//
// Tensors (state_dict order of the block; every weight [cout, cin, kh, kw], every bias [cout]):
//   COV : gru.conv{z1,r1,q1} [128,512,1,5], gru.conv{z2,r2,q2} [128,512,5,1], cov_head.conv1 [256,128,3,3], conv2 [128,256,3,3], conv3 [64,128,3,3],
//         conv4 [2,64,3,3], mask.0 [256,128,3,3], mask.2 [576,256,1,1]
//   FLOW: the same gru, flow_head.0 [256,128,3,3], flow_head.2 [2,256,3,3], mask.0, mask.2
//
// Launches (GEMMs: rows = output channels, columns = pixels m = (b, y, x), K = [64-channel chunk][tap (ky, kx)][channel in chunk]):
//   0  net, inp (NCHW or channels-last) -> HX [M,512] = [h | x], NHWC
//   1  zr1   1x5  [h | x]   -> 256: columns 0..127 z = sigmoid -> Z [M,128]; 128..255 r = sigmoid, r * h -> RH [M,128]
//   2  q1    1x5  [r h | x] -> 128: h' = (1 - z) * h + z * tanh(q) -> HX[:, 0:128] (in place: a launch reads h only at the element it writes)
//   3  zr2   5x1  as 1
//   4  q2    5x1  as 2, h' also to net_out (NCHW)
//   5  head1 3x3  h -> 512: [cov_head.conv1 | mask.0] (FLOW: [flow_head.0 | mask.0]), ReLU -> C1 [M,512]
//   COV : 6 conv2 3x3 C1[:, 0:256] -> C2 [M,128];  7 conv3 3x3 C2 -> ReLU -> C3 [M,64];  8 conv4 3x3 C3 -> delta (NCHW, 2 of 64 packed rows live)
//   FLOW: 6 flow_head.2 3x3 C1[:, 0:256] -> delta (NCHW)
//   last  mask.2 1x1 C1[:, 256:512] -> 576, x 0.25 for COV (covhead.py:42; FLOW's caller scales at covhead.py:122) -> mask (NCHW)
//
// Rounding: weights and biases are rounded to the operand type when packed (exact for a module already in that type); every product is exact in the
// fp32 accumulator of v_mfma_f32_32x32x16_{bf16,f16}; bias, sigmoid, tanh, the gate products, ReLU and the output scale are fp32 on the accumulator;
// a value is rounded (to nearest even) exactly once where it is stored: Z, RH, h' (both passes), C1, C2, C3, delta, mask.
// Summation order of one output: bias first, then K in the order above, 16 k per MFMA; fixed, so two calls return the same bits.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#ifdef __HIPCC__
#define UBLK_HD __host__ __device__
#else
#define UBLK_HD
#endif

namespace ublk {

constexpr int HID = 128, INP = 384, HXC = HID + INP;   // hidden, input, concatenated channels
constexpr int MASK_C = 576, HEAD_C = 256;
constexpr int CK = 64;                                  // channels per K chunk (one LDS stage)
constexpr int MAX_PIXELS = 1 << 20;                     // B * H * W
constexpr int N_KINDS = 2;
constexpr int MAX_TENSORS = 24, MAX_CONVS = 9;

enum Epi { EPI_GATES = 0, EPI_UPDATE = 1, EPI_STORE = 2 };
enum Buf { BUF_HX = 0, BUF_Z, BUF_RH, BUF_C1, BUF_C2, BUF_C3, N_BUFS, BUF_NONE = -1 };
constexpr int BUF_CH[N_BUFS] = {HXC, HID, HID, 2 * HEAD_C, HID, 64};   // channels (= pixel stride) of each NHWC workspace buffer

struct Tensor {
    char name[64];
    int shape[4], ndim;
};

// one launch of the convolution kernel; up to two stacked weight tensors (rows of the GEMM) that share one input
struct Conv {
    int kh, kw, cin, cout, cout_pad;      // cout_pad: packed rows (multiple of 64)
    int t_w[2], t_b[2], rows[2];          // tensor indices and rows of the stacked parts (rows[1] = 0: one part)
    int src0, src0_off, src0_ch;          // channels [0, src0_ch) of K come from buffer src0 at channel offset src0_off,
    int src1, src1_off;                   // the rest from src1 at src1_off - src0_ch + channel (BUF_NONE when src0 has them all)
    int epi, relu, dst, nchw;             // EPI_*; EPI_STORE: ReLU, NHWC buffer or BUF_NONE; nchw: 0 none, 1 net_out, 2 delta, 3 mask
    float scale;                          // power of two
    int cfg;                              // tile configuration: 0 = 64 px x 64 ch (4 waves), 1 = 32 px x 64 ch (2 waves)
    size_t w_off, b_off;                  // byte offsets into the packed buffer: fragments (16-bit), bias (fp32, cout_pad values)
};

struct Plan {
    int n_tensors, n_convs;
    Tensor tensors[MAX_TENSORS];
    Conv convs[MAX_CONVS];
    size_t packed_bytes;
};

inline int add_tensor(Plan& p, const char* name, int cout, int cin, int kh, int kw) {
    Tensor& w = p.tensors[p.n_tensors];
    snprintf(w.name, sizeof(w.name), "%s.weight", name);
    w.shape[0] = cout; w.shape[1] = cin; w.shape[2] = kh; w.shape[3] = kw; w.ndim = 4;
    Tensor& b = p.tensors[p.n_tensors + 1];
    snprintf(b.name, sizeof(b.name), "%s.bias", name);
    b.shape[0] = cout; b.shape[1] = b.shape[2] = b.shape[3] = 0; b.ndim = 1;
    p.n_tensors += 2;
    return p.n_tensors - 2;
}

inline Conv& add_conv(Plan& p, int kh, int kw, int cin, int tw0, int rows0, int tw1, int rows1) {
    Conv& c = p.convs[p.n_convs++];
    memset(&c, 0, sizeof(c));
    c.kh = kh; c.kw = kw; c.cin = cin;
    c.t_w[0] = tw0; c.t_b[0] = tw0 + 1; c.rows[0] = rows0;
    c.t_w[1] = tw1; c.t_b[1] = tw1 + 1; c.rows[1] = rows1;
    c.cout = rows0 + rows1;
    c.cout_pad = (c.cout + 63) / 64 * 64;
    c.src0 = BUF_HX; c.src0_ch = cin; c.src1 = BUF_NONE;
    c.epi = EPI_STORE; c.dst = BUF_NONE; c.scale = 1.f;
    c.w_off = p.packed_bytes;
    p.packed_bytes += (size_t)c.cout_pad * kh * kw * cin * 2;
    c.b_off = p.packed_bytes;
    p.packed_bytes += (size_t)c.cout_pad * 4;
    return c;
}

inline void build_plan(Plan& p, int kind) {
    memset(&p, 0, sizeof(p));
    int z[2], r[2], q[2];
    for (int s = 0; s < 2; ++s) {
        const int kh = s ? 5 : 1, kw = s ? 1 : 5;
        char nm[32];
        snprintf(nm, sizeof(nm), "gru.convz%d", s + 1); z[s] = add_tensor(p, nm, HID, HXC, kh, kw);
        snprintf(nm, sizeof(nm), "gru.convr%d", s + 1); r[s] = add_tensor(p, nm, HID, HXC, kh, kw);
        snprintf(nm, sizeof(nm), "gru.convq%d", s + 1); q[s] = add_tensor(p, nm, HID, HXC, kh, kw);
    }
    int h1, h2, h3 = -1, h4 = -1;
    if (kind == 0) {
        h1 = add_tensor(p, "cov_head.conv1", HEAD_C, HID, 3, 3);
        h2 = add_tensor(p, "cov_head.conv2", HID, HEAD_C, 3, 3);
        h3 = add_tensor(p, "cov_head.conv3", 64, HID, 3, 3);
        h4 = add_tensor(p, "cov_head.conv4", 2, 64, 3, 3);
    } else {
        h1 = add_tensor(p, "flow_head.0", HEAD_C, HID, 3, 3);
        h2 = add_tensor(p, "flow_head.2", 2, HEAD_C, 3, 3);
    }
    const int m0 = add_tensor(p, "mask.0", HEAD_C, HID, 3, 3), m2 = add_tensor(p, "mask.2", MASK_C, HEAD_C, 1, 1);

    for (int s = 0; s < 2; ++s) {
        const int kh = s ? 5 : 1, kw = s ? 1 : 5;
        Conv& g = add_conv(p, kh, kw, HXC, z[s], HID, r[s], HID);      // [h | x] is HX as it lies
        g.epi = EPI_GATES; g.cfg = 0;
        Conv& u = add_conv(p, kh, kw, HXC, q[s], HID, 0, 0);
        u.src0 = BUF_RH; u.src0_ch = HID; u.src1 = BUF_HX; u.src1_off = HID;
        u.epi = EPI_UPDATE; u.cfg = 1; u.nchw = s ? 1 : 0;
    }
    Conv& c1 = add_conv(p, 3, 3, HID, h1, HEAD_C, m0, HEAD_C);
    c1.relu = 1; c1.dst = BUF_C1; c1.cfg = 0;
    if (kind == 0) {
        Conv& c2 = add_conv(p, 3, 3, HEAD_C, h2, HID, 0, 0);
        c2.src0 = BUF_C1; c2.dst = BUF_C2; c2.cfg = 1;
        Conv& c3 = add_conv(p, 3, 3, HID, h3, 64, 0, 0);
        c3.src0 = BUF_C2; c3.relu = 1; c3.dst = BUF_C3; c3.cfg = 1;
        Conv& c4 = add_conv(p, 3, 3, 64, h4, 2, 0, 0);
        c4.src0 = BUF_C3; c4.nchw = 2; c4.cfg = 1;
    } else {
        Conv& f2 = add_conv(p, 3, 3, HEAD_C, h2, 2, 0, 0);
        f2.src0 = BUF_C1; f2.nchw = 2; f2.cfg = 1;
    }
    Conv& mk = add_conv(p, 1, 1, HEAD_C, m2, MASK_C, 0, 0);
    mk.src0 = BUF_C1; mk.src0_off = HEAD_C; mk.nchw = 3; mk.cfg = 0;
    mk.scale = kind == 0 ? 0.25f : 1.f;
}

// Packed weights of one launch: 16-byte units [32-row tile][k-step][lane 0..63]; lane l of k-step s holds row 32 tile + (l & 31), k = 16 s + 8 (l >> 5) + j,
// j = 0..7 (the A operand of v_mfma_f32_32x32x16).  k -> (chunk, tap, channel): k = (chunk * taps + tap) * CK + c.
UBLK_HD inline size_t packed_w_index(const Conv& c, int row, int k) {
    const int ksteps = c.kh * c.kw * c.cin / 16;
    const int tile = row >> 5, s = k >> 4, l = (row & 31) + 32 * ((k >> 3) & 1), j = k & 7;
    return (((size_t)tile * ksteps + s) * 64 + l) * 8 + j;
}
// the source element of GEMM column k: tap = ky * kw + kx, input channel ch
UBLK_HD inline void k_source(const Conv& c, int k, int& tap, int& ch) {
    const int taps = c.kh * c.kw, chunk = k / (taps * CK), rem = k - chunk * taps * CK;
    tap = rem / CK;
    ch = chunk * CK + rem % CK;
}

inline size_t ws_bytes(int M) {
    size_t n = 0;
    for (int b = 0; b < N_BUFS; ++b) n += (size_t)M * BUF_CH[b] * 2;
    return n;
}

}  // namespace ublk
