// The decoder's motion encoder in 16-bit operands: GMAUpdateBlock.encoder (called at covhead.py:106), five convolutions with ReLUs around two
// concatenations, one call per decoder iteration.
//
//   motion_stage_kernel          corr [B,145,H,W] (NCHW through an LDS transpose, or channels-last through the same tile) -> CORR [M,192] with channels
//                                145..191 stored as zero; flow [B,2,H,W] -> FIM [M,128], its 7x7 im2col in (channel, tap) order with the taps outside the
//                                image and columns 98..127 stored as zero; flow -> output channels 126..127.  A workgroup owns 64 pixels of one image and
//                                one of four parts (three 64-channel groups of CORR; FIM and the pass-through).  Reads run along the pixels (NCHW) or the
//                                channels (channels-last), every workspace store is 16 bytes with eight lanes covering one 128-byte line.
//   update_conv_kernel, update_pack_kernel: the shared convolution family and its packer, update_conv_dev.h
//
// 6 launches on the caller's stream; no atomics, no cross-workgroup waits, no host synchronisation, no allocation.
// Layer table, packed layout, workspace layout, rounding points and summation order: motion_encoder_math.h.
#include "update_conv_dev.h"
#include "motion_encoder_math.h"

namespace {

using namespace menc;

__device__ __forceinline__ uint4 pack8(const uint16_t* v) {
    return uint4{(uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16), (uint32_t)v[4] | ((uint32_t)v[5] << 16),
                 (uint32_t)v[6] | ((uint32_t)v[7] << 16)};
}

// ---------------------------------------------------------------------------------------------------------------- launch 0
__global__ __launch_bounds__(256) void motion_stage_kernel(const uint16_t* corr, const uint16_t* flow, uint16_t* corr_ws, uint16_t* fim, uint16_t* out, int H,
                                                           int W, int channels_last) {
    __shared__ uint16_t tile[64][66];
    const int P = H * W, tiles = (P + 63) / 64, b = blockIdx.x / tiles, p0 = (blockIdx.x - b * tiles) * 64;      // (B up to 2^20: the image index rides in x)
    if (blockIdx.y < CORR_PAD / 64) {
        const int c0 = blockIdx.y * 64;
        for (int e = threadIdx.x; e < 4096; e += 256) {
            const int hi = e >> 6, lo = e & 63;
            const int ch = channels_last ? lo : hi, px = channels_last ? hi : lo, p = p0 + px, cg = c0 + ch;
            uint16_t v = 0;                                                    // channels 145..191: zero
            if (p < P && cg < CORR_C) v = channels_last ? corr[((size_t)b * P + p) * CORR_C + cg] : corr[((size_t)b * CORR_C + cg) * P + p];
            tile[ch][px] = v;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < 512; e += 256) {
            const int px = e >> 3, part = e & 7, p = p0 + px;
            if (p >= P) continue;
            uint16_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = tile[part * 8 + j][px];
            *(uint4*)(corr_ws + ((size_t)b * P + p) * CORR_PAD + c0 + part * 8) = pack8(v);
        }
        return;
    }
    // flow element (ch, pixel q) of image b
    auto fl = [&](int ch, int q) { return channels_last ? flow[((size_t)b * P + q) * 2 + ch] : flow[((size_t)b * 2 + ch) * P + q]; };
    for (int e = threadIdx.x; e < 64 * (FIM_C / 8); e += 256) {
        const int px = e >> 4, part = e & 15, p = p0 + px;
        if (p >= P) continue;
        const int y = p / W, x = p - y * W;
        uint16_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = part * 8 + j, ch = k / FLOW_TAPS, tap = k - ch * FLOW_TAPS, ky = tap / 7, kx = tap - ky * 7;
            const int yy = y + ky - 3, xx = x + kx - 3;
            v[j] = 0;                                                          // taps outside the image and columns 98..127: zero
            if (k < FIM_LIVE && yy >= 0 && yy < H && xx >= 0 && xx < W) v[j] = fl(ch, yy * W + xx);
        }
        *(uint4*)(fim + ((size_t)b * P + p) * FIM_C + part * 8) = pack8(v);
    }
    if (threadIdx.x < 128) {
        const int ch = threadIdx.x >> 6, p = p0 + (threadIdx.x & 63);
        if (p < P) out[((size_t)b * OUT_C + OUT_LIVE + ch) * P + p] = fl(ch, p);
    }
}

}  // namespace

extern "C" int mv_motion_encoder_tensor_count(void) { return N_TENSORS; }

extern "C" int mv_motion_encoder_tensor_info(int i, char* name_buf /* >= 64 bytes */, int32_t* shape /* [4] */, int32_t* ndim) {
    MV_CHECK_ARG(i >= 0 && i < N_TENSORS && name_buf && shape && ndim);
    ublk::Tensor t;
    tensor_info(i, t);
    memcpy(name_buf, t.name, sizeof(t.name));
    for (int d = 0; d < 4; ++d) shape[d] = d < t.ndim ? t.shape[d] : 0;
    *ndim = t.ndim;
    return MV_OK;
}

extern "C" size_t mv_motion_encoder_packed_bytes(int operand) { return operand_ok(operand) ? packed_bytes() : 0; }

extern "C" size_t mv_motion_encoder_workspace_bytes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || (int64_t)B * H * W > menc::MAX_PIXELS) return 0;
    return menc::ws_bytes(B * H * W);
}

extern "C" int mv_motion_encoder_pack(int operand, const float* const* tensors, void* packed, mvStream_t stream) {
    MV_CHECK_ARG(operand_ok(operand) && tensors && packed);
    for (int i = 0; i < N_TENSORS; ++i) MV_CHECK_ARG(tensors[i]);
    for (int l = 0; l < N_LAYERS; ++l)
        launch_pack(operand, packed_conv(l), LAYERS[l].pack_cin_src, tensors[2 * l], tensors[2 * l + 1], nullptr, nullptr, packed, (hipStream_t)stream);
    return mv_launch_status();
}

extern "C" int mv_motion_encoder_forward(int operand, const void* packed, const void* flow, const void* corr, int B, int H, int W, int channels_last, void* out,
                                         void* workspace, mvStream_t stream) {
    MV_CHECK_ARG(operand_ok(operand) && packed && flow && corr && out && workspace);
    MV_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && (int64_t)B * H * W <= menc::MAX_PIXELS && (channels_last == 0 || channels_last == 1));
    const int P = H * W, M = B * P;
    hipStream_t st = (hipStream_t)stream;
    uint16_t* buf[menc::N_BUFS];
    buf[0] = (uint16_t*)workspace;
    for (int i = 1; i < menc::N_BUFS; ++i) buf[i] = buf[i - 1] + (size_t)M * menc::BUF_CH[i - 1];
    hipLaunchKernelGGL(motion_stage_kernel, dim3(B * mv_ceil_div(P, 64), CORR_PAD / 64 + 1), dim3(256), 0, st, (const uint16_t*)corr, (const uint16_t*)flow,
                       buf[BUF_CORR], buf[BUF_FIM], (uint16_t*)out, H, W, channels_last);
    for (int l = 0; l < N_LAYERS; ++l) {
        const Layer& L = LAYERS[l];
        const ublk::Conv c = packed_conv(l);
        ConvArgs a;
        a.src0 = buf[L.src]; a.s0_stride = menc::BUF_CH[L.src]; a.s0_ch = L.cin;
        a.src1 = nullptr; a.s1_stride = 0;
        a.w = (const uint4*)((const char*)packed + c.w_off);
        a.bias = (const float*)((const char*)packed + c.b_off);
        a.M = M; a.P = P; a.H = H; a.W = W; a.kh = L.kh; a.kw = L.kw; a.nchunks = L.cin / CK;
        a.epi = EPI_STORE; a.relu = 1; a.cout = L.cout; a.nchw_ch = OUT_C; a.scale = 1.f;
        a.dst = L.dst == BUF_OUT ? nullptr : buf[L.dst] + L.dst_off;
        a.dst_stride = L.dst == BUF_OUT ? 0 : menc::BUF_CH[L.dst];
        a.nchw = L.dst == BUF_OUT ? (uint16_t*)out : nullptr;
        a.hx = a.z = a.rh = nullptr;
        if (operand == MV_F16) launch_conv<true>(L.cfg, a, c.cout_pad, st);
        else launch_conv<false>(L.cfg, a, c.cout_pad, st);
    }
    return mv_launch_status();
}
