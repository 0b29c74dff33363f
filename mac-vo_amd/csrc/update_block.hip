// The decoder's recurrent update blocks in 16-bit operands: CovUpdateBlock (covhead.py:24-43: SepConvGRU, CovHead, mask x 0.25) and the gru / flow_head /
// mask members of FlowFormer's GMAUpdateBlock (covhead.py:112-114), one call each per decoder iteration.
//
//   update_to_nhwc_kernel        net [B,128,H,W] and inp [B,384,H,W] (NCHW through an LDS transpose, or channels-last as a copy) -> HX [M,512]
//   update_conv_kernel, update_pack_kernel: the shared convolution family and its packer, update_conv_dev.h
//
// 9 launches for MV_UPDATE_FLOW, 11 for MV_UPDATE_COV, on the caller's stream; no atomics, no cross-workgroup waits, no host synchronisation, no allocation.
// Layer table, packed layout, rounding points and summation order: update_block_math.h.
#include "update_conv_dev.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- launch 0
__global__ __launch_bounds__(256) void update_to_nhwc_kernel(const uint16_t* net, const uint16_t* inp, uint16_t* hx, int P, int channels_last) {
    __shared__ uint16_t tile[64][66];
    const int tiles = (P + 63) / 64, b = blockIdx.x / tiles, p0 = (blockIdx.x - b * tiles) * 64, c0 = blockIdx.y * 64;      // (B up to 2^20: the image index rides in x)
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

const Plan* plan(int kind) {
    static Plan p[N_KINDS];
    static const bool ok = (build_plan(p[0], 0), build_plan(p[1], 1), true);
    return ok && kind >= 0 && kind < N_KINDS ? &p[kind] : nullptr;
}

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
        const Conv& c = p->convs[ci];
        launch_pack(operand, c, c.cin, tensors[c.t_w[0]], tensors[c.t_b[0]], tensors[c.t_w[1]], tensors[c.t_b[1]], packed, (hipStream_t)stream);
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
    hipLaunchKernelGGL(update_to_nhwc_kernel, dim3(B * mv_ceil_div(P, 64), HXC / 64), dim3(256), 0, st, (const uint16_t*)net, (const uint16_t*)inp, buf[BUF_HX], P,
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
        a.epi = c.epi; a.relu = c.relu; a.cout = a.nchw_ch = c.cout; a.scale = c.scale;
        a.dst = c.dst == BUF_NONE ? nullptr : buf[c.dst];
        a.dst_stride = c.dst == BUF_NONE ? 0 : BUF_CH[c.dst];
        a.nchw = outs[c.nchw];
        a.hx = buf[BUF_HX]; a.z = buf[BUF_Z]; a.rh = buf[BUF_RH];
        if (operand == MV_F16) launch_conv<true>(c.cfg, a, c.cout_pad, st);
        else launch_conv<false>(c.cfg, a, c.cout_pad, st);
    }
    return mv_launch_status();
}
