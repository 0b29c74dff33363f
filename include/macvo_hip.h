/*
 * macvo_hip.h — C ABI of libmacvo_hip.so: the MI355X (gfx950) hot path of MAC-VO.
 *
 * Every entry point is what a binding for the reference's per-frame hot path would call
 * (the reference is pure Python, so the "FFI" is ctypes — see INTEGRATION.md for the stub a
 * maintainer adds on the reference side).  Each function cites the reference code it replaces
 * (paths relative to the MAC-VO checkout).
 *
 * Conventions
 *   - All data pointers are DEVICE pointers unless the parameter says "host".
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls only enqueue
 *     work: no hidden synchronisation, no allocation, no host<->device copies.  The caller
 *     owns every buffer and synchronises when it needs results.
 *   - Return value: MV_OK (0) or a negative MV_ERR_* code; nothing throws.
 *   - Tensors are dense row-major with the shapes given; N1 = H1*W1, N2 = H2*W2.
 */
#ifndef MACVO_HIP_H
#define MACVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mvStream_t;

enum {
    MV_OK = 0,
    MV_ERR_INVALID_ARG = -1,
    MV_ERR_UNSUPPORTED = -2,
    MV_ERR_LAUNCH = -3,
    MV_ERR_WORKSPACE = -4
};

enum {
    MV_F32 = 0,        /* fp32 operands, exact fp32 MFMA (bitwise an fmaf chain)                               */
    MV_F16 = 1,
    MV_BF16 = 2,
    MV_BF16X3 = 3,     /* fp32 operands pre-split by mv_split_bf16x3 into 3 bf16 planes; 6 bf16 MFMA products, fp32
                          accumulate: fp32-class accuracy (dropped terms O(2^-24)), not bitwise; layout HWC only     */
    MV_BF16X2 = 4,     /* the same planes, but only the two leading pieces (16 significant bits) and the 3 products
                          a0b1 + a1b0 + a0b0: relative error ~2^-16, finer than TF32 — the class the reference's fast
                          frontend runs this GEMM in (allow_tf32, Module/Frontend/Frontend.py:275-277); layout HWC only */
    MV_PACK_BF16X3 = 5,/* `mode` of mv_volume_pack / mv_corr_volume_packed: fp32 operands split into three bf16 pieces and
                          written in MFMA-fragment order; six piece products, fp32 accumulate (fp32-class, as MV_BF16X3) */
    MV_PACK_F16X2 = 6, /* the same with two fp16 pieces (11 + 11 bits) of every value after an exact power-of-two scaling of its
                          ROW (one pixel's feature vector) into fp16's range, three piece products, the scales undone exactly in
                          the epilogue: |error| <= ~2^-21 sum_k |a_k||b_k| — inside the exact path's parity bar, half the matrix
                          work of MV_PACK_BF16X3; the row scale is not clamped: any finite row of the fp32 range is carried */
    MV_VOL_ENC16 = 16  /* mvFramePipeConfig.volume_split only: 16-bit features, volume stored in the features' fp16 type */
};

/* feature-map memory layouts accepted by mv_corr_volume */
enum {
    MV_LAYOUT_CHW = 0, /* [B, C, N]  (NCHW feature maps, as the reference hands them over) */
    MV_LAYOUT_HWC = 1  /* [B, N, C]  (token-major / channels_last)                          */
};

/* most independent sequences ("lanes") one lane-batched launch / one frame pipe can carry (batch-32 frames = 32 lanes) */
#define MV_MAX_LANES 64

/* library ABI version (bumped on any signature change) and a static description string */
int mv_abi_version(void);
const char* mv_error_string(int code);

/* -------------------------------------------------------------------------------------------
 * A5  all-pairs cost volume.
 * Replaces FlowFormer `MemoryEncoder.corr` invoked at Module/Network/FlowFormerCov/flownet.py:26
 * (`corr = einsum('bhid,bhjd->bhij')`, heads = 1, no 1/sqrt(d)) and the `.float()` at flownet.py:27.
 *   out[b, i, j] = sum_c f1[b, c, i] * f2[b, c, j]          (== cost_maps [B*N1, 1, H2, W2] fp32)
 * in_dtype MV_F32: exact fp32 (v_mfma_f32_32x32x2_f32, one rounding per product, k ascending).
 * in_dtype MV_F16 / MV_BF16: 16-bit operands, fp32 accumulate, fp32 output (Fast mode).
 * in_dtype MV_BF16X3: f1/f2 are the [3][B][N][C] bf16 planes written by mv_split_bf16x3 from fp32 features
 *   (x = hi + mid + lo); the product is rebuilt from the 6 bf16 MFMA products with i + j <= 2.  The reference runs
 *   this GEMM in TF32/fp16 (Module/Frontend/Frontend.py:275-278), so this mode is at least as precise as its own.
 * Requirements: C % 16 == 0.  f1/f2 16-byte aligned.
 */
int mv_corr_volume(const void* f1, const void* f2, float* out, int B, int C, int N1, int N2,
                   int in_dtype, int layout, mvStream_t stream);

/* fp32 -> three bf16 planes (hi, mid, lo; residuals exact): planes[3][n] (uint16 bf16 bits), n % 4 == 0. */
int mv_split_bf16x3(const float* x, void* planes, size_t n, mvStream_t stream);
/* -------------------------------------------------------------------------------------------
 * (f)2 — the consumer of the cost volume: FlowFormer's cost PATCH EMBEDDING `proj` stack, fused (csrc/patch_embed.hip).
 * Replaces, per H2 x W2 slice of cost_maps (S = B*H1*W1 slices): F.pad to multiples of 8 -> Conv2d(1,16,6,stride 2,pad 2) -> ReLU ->
 * Conv2d(16,32,6,2,2) -> ReLU -> Conv2d(32,64,6,2,2) — PatchEmbed(patch_size 8, embed_dim 64) of FlowFormer's MemoryEncoder, reached from
 * Module/Network/FlowFormerCov/flownet.py:26; hyper-parameters Config/Train/Demo.yaml:20-36; token shape covhead.py:61-64.  The submodule's
 * source is absent from the reference checkout: shapes restated from the published FlowFormer sources (oracle/patch_embed.py), parity pinned
 * to F.conv2d.  16-bit matrix pipe, fp32 accumulate, intermediate maps in LDS (never in HBM).  operand_type = the 16-bit type of weights and
 * activations: MV_F16 (11 significant bits = TF32's mantissa, and the type MACVO_Fast.yaml:73 runs this encoder in) or MV_BF16 (bf16 encoders).
 *   mv_patch_embed_pack   OIHW fp32 weights + biases of the three Conv2d layers -> fragment-ordered 16-bit (+ fp32 biases), once per model
 *   mv_cost_patch_embed   cost_maps [S, H2, W2] fp32 -> token_layout ? [S, (H2/8)*(W2/8), 64] : [S, 64, H2/8, W2/8] fp32; operand_type must be
 *                         the one `packed` was built with
 *   mv_cost_patch_embed_supported   the slice sizes the kernels are instantiated for, each as the raw 1/8 slice and as the padded one PatchEmbed.forward
 *                                   hands to `proj`: 60 / 64 x 80 (640x480, 640x512 frames), 80 x 80 (640x640), 90 / 96 x 160 (1280x720), 47 x 98 /
 *                                   48 x 104 (KITTI, 376x784 frames) and 60 x 94 / 64 x 96 (EuRoC, 480x752); others: MV_ERR_UNSUPPORTED */
size_t mv_patch_embed_packed_bytes(void);
int mv_patch_embed_pack(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, void* packed,
                        int operand_type, mvStream_t stream);
int mv_cost_patch_embed_supported(int H2, int W2);
int mv_cost_patch_embed(const float* cost_maps, const void* packed, float* out, int S, int H2, int W2, int token_layout, int operand_type,
                        mvStream_t stream);
/* the same with the slices and / or the tokens in the 16-bit OPERAND type (row (f)2 as SURVEY.md words it: "the volume kept in bf16 / fp16"): in_dtype =
 * MV_F32 or operand_type — fp16 cells of mv_corr_volume_out16's volume go to the matrix pipe as they are; out_dtype = MV_F32 or operand_type — tokens in the
 * encoder's dtype (what Conv2d under MACVO_Fast.yaml:73-74's fp16 autocast returns).  No widening pass on either side: 9.6 + 10.2 KB of HBM traffic per
 * 60 x 80 slice instead of 19.2 + 20.5 KB.  (in MV_F32, out 16-bit) is not built: MV_ERR_UNSUPPORTED.  fp16 conversions saturate at +-65504. */
int mv_cost_patch_embed_t(const void* cost_maps, int in_dtype, const void* packed, void* out, int out_dtype, int S, int H2, int W2, int token_layout,
                          int operand_type, mvStream_t stream);
/* -------------------------------------------------------------------------------------------
 * A5, split + streaming form (csrc/corr_volume_split.hip): the same volume from fp32 feature maps on the 16-bit matrix pipe.
 * gfx950 has no TF32 MFMA; the reference runs this GEMM in TF32 / fp16 (Module/Frontend/Frontend.py:275-277,
 * Config/Experiment/MACVO/MACVO_Fast.yaml:69-76).  mode MV_PACK_BF16X3: x = p0 + p1 + p2 (bf16 pieces, residuals exact), product
 * rebuilt from the six piece products with i + j <= 2 — same parity bar as the exact fp32 path, not bitwise.
 *
 * mv_volume_pack       both feature maps ([B,C,N] for MV_LAYOUT_CHW, [B,N,C] for MV_LAYOUT_HWC, fp32) -> packed operands
 *                      [B][ceil(N/32)+1 row blocks][C/16 k-steps][pieces][64 lanes][8 x 16 bit], one launch;
 *                      mv_volume_pack_bytes(B, C, N, mode) bytes each (0 = unsupported mode / shape).
 * mv_corr_volume_packed  out[b,i,j] fp32 [B,N1,N2] from two packed operands (C == 256, N1 >= 32, any N2 >= 64, N1*N2 < 2^30:
 *                      mv_corr_volume_packed_supported; MV_ERR_UNSUPPORTED otherwise — callers then use mv_corr_volume(MV_F32)).
 *                      N2 % 64 != 0 (KITTI: 47 x 98 maps, EuRoC: 60 x 94): the last 64-column sub-tile of a row is partial — its
 *                      operand rows past N2 are the pack's copies of row N2 - 1, its stores are lane-masked.
 * Two entry points because the pack needs nothing but the feature maps: the frame driver issues it on another stream one
 * frame ahead of the GEMM. */
size_t mv_volume_pack_bytes(int B, int C, int N, int mode);
int mv_volume_pack(const float* f1, const float* f2, void* packed1, void* packed2, int B, int C, int N1, int N2, int layout,
                   int mode, mvStream_t stream);
/* mv_volume_pack with operand 2 (an H2 x W2 map, both multiples of 4) in 4 x 4-tile order: the GEMM's output columns then are that
 * order (see mv_corr_lookup_tiled); operand 1 and everything else as mv_volume_pack with N2 = H2 * W2 */
int mv_volume_pack_tiled(const float* f1, const float* f2, void* packed1, void* packed2, int B, int C, int N1, int H2, int W2,
                         int layout, int mode, mvStream_t stream);
int mv_corr_volume_packed_supported(int B, int C, int N1, int N2, int mode);
int mv_corr_volume_packed(const void* packed1, const void* packed2, float* out, int B, int C, int N1, int N2, int mode,
                          mvStream_t stream);
/* the same launch with `free_cus` compute units (rounded down to a multiple of 8) left without a persistent workgroup, for a caller that runs kernels
 * BESIDE the GEMM which cannot share a SIMD with its waves (mv_frame_pipe_*: the LM solve's workgroup).  Same bits for every value; 0 = mv_corr_volume_packed. */
int mv_corr_volume_packed_shared(const void* packed1, const void* packed2, float* out, int B, int C, int N1, int N2, int mode, int free_cus,
                                 mvStream_t stream);

/* Diagnostics: name of the kernel the calling thread's last mv_corr_volume dispatched ("" before the first call); the
 * string is static.  Used by the dispatch tests and by bench.py to name the kernel its roofline line is about. */
const char* mv_corr_volume_last_kernel(void);

/* -------------------------------------------------------------------------------------------
 * A6  (2r+1)^2 bilinear window lookup in each query's own cost slice.
 * Replaces FlowFormer `MemoryDecoder.encode_flow_token(cost_maps, coords1)` called at
 * Module/Network/FlowFormerCov/covhead.py:92 ("MUST run in fp32", :91) =
 * grid_sample(align_corners=True, padding_mode="zeros") on a [B*N1, 2r+1, 2r+1, 2] grid.
 *   vol    [B*N1, H2, W2] fp32;  coords [B, 2, H1, W1] fp32 (channel 0 = x, 1 = y)
 *   out    [B, (2r+1)^2, H1, W1] fp32; channel k = (2r+1)*i + j samples (x + i - r, y + j - r)
 * Requirements: 1 <= radius <= 4.
 */
int mv_corr_lookup(const float* vol, const float* coords, float* out, int B, int H1, int W1,
                   int H2, int W2, int radius, mvStream_t stream);

/* Fast mode (Config/Experiment/MACVO/MACVO_Fast.yaml:73-74: enc_dtype fp16): with 16-bit feature maps the reference's `einsum` returns the
 * volume in that 16-bit type and Module/Network/FlowFormerCov/flownet.py:27 merely widens it.  mv_corr_volume_out16 is that einsum with its ONE
 * rounding (fp32 accumulators -> round-to-nearest-even -> in_dtype) in the GEMM's epilogue and 2-byte cells: out [B, N1, N2] of in_dtype, half the
 * bytes of the output-bound kernel.  HWC feature maps, C = 128 / 256, an EVEN N2 >= 64 (a lane stores a column pair; N2 % 64 != 0: partial last
 * sub-tile, operand rows clamped to N2 - 1, lane-masked stores) and B * N1 * N2 >= 2^22 (mv_corr_volume_out16_supported; MV_ERR_UNSUPPORTED otherwise:
 * use mv_corr_volume + a cast).  mv_corr_lookup_vol16 is mv_corr_lookup on such an fp16 volume (cells widened on load = `cost_maps.float()`,
 * everything behind the load identical to the fp32 form); radius 4. */
int mv_corr_volume_out16_supported(int B, int C, int N1, int N2, int in_dtype, int layout);
int mv_corr_volume_out16(const void* f1, const void* f2, void* out, int B, int C, int N1, int N2, int in_dtype, int layout, mvStream_t stream);
int mv_corr_lookup_vol16(const void* vol_f16, const float* coords, float* out, int B, int H1, int W1, int H2, int W2, int radius,
                         mvStream_t stream);

/* The same lookup (same reference code, Module/Network/FlowFormerCov/covhead.py:92) on a volume whose per-query slices are stored in
 * 4 x 4-cell tiles: vol[(b N1 + q) H2 W2 + ((y / 4) * (W2 / 4) + x / 4) * 16 + (y % 4) * 4 + x % 4] — what mv_corr_volume_packed writes
 * when operand 2 was packed by mv_volume_pack_tiled.  Used inside the frame driver for >= 3 lanes, where it owns both the producer and
 * the consumer of the volume (the drop-in hook keeps the reference's [B*N1, 1, H2, W2]).  radius == 4, H2 % 4 == W2 % 4 == 0
 * (MV_ERR_UNSUPPORTED otherwise).  Results are bit-identical to mv_corr_lookup on the row-major volume. */
int mv_corr_lookup_tiled(const float* vol, const float* coords, float* out, int B, int H1, int W1,
                         int H2, int W2, int radius, mvStream_t stream);

/* Round 6: the tiled form for the Fast-mode volume's 2-byte cells.  mv_fmap_tile_rows16 writes the pixel rows of a 16-bit HWC feature map
 * [B, H, W, C] in 4 x 4-tile order (out[b][((y / 4) * (W / 4) + x / 4) * 16 + (y % 4) * 4 + x % 4][:] = f[b][y * W + x][:]; C % 8 == 0,
 * W % 4 == 0, out != f; ceil(H / 4) tile rows, the rows y >= H of the last one zero pixels: out is [B, mv_tiled_slice_cells(H, W), C]);
 * as operand 2 of mv_corr_volume_out16 (with N2 = mv_tiled_slice_cells) it makes the unchanged GEMM — the same `einsum` of
 * Module/Network/FlowFormerCov/flownet.py:26 — write every query's slice in the tile order above, where a tile is one aligned 32-byte
 * sector.  mv_corr_lookup_tiled_vol16 is mv_corr_lookup_vol16 (covhead.py:92 on `cost_maps.float()`) on that layout: ~338 B instead of
 * ~512 B per query, tokens bit-identical; a slice is mv_tiled_slice_cells(H2, W2) cells (the padding cells are exact zeros = the lookup's zero
 * padding).  vol 32-byte aligned; radius == 4, W2 % 4 == 0 (MV_ERR_UNSUPPORTED otherwise). */
int mv_tiled_slice_cells(int H, int W);   /* ceil(H / 4) * 4 * W; 0 when W % 4 != 0 */
int mv_fmap_tile_rows16(const void* f, void* out, int B, int C, int H, int W, mvStream_t stream);
int mv_corr_lookup_tiled_vol16(const void* vol_f16, const float* coords, float* out, int B, int H1, int W1, int H2, int W2, int radius,
                               mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * A8/A2  frontend epilogue: network output -> the typed records of IStereoDepth.Output / IMatcher.Output.
 * Replaces Module/Network/FlowFormerCov/flownet.py:44 (`exp(2*cov)`), Module/Frontend/Frontend.py:183-200
 * (`inference_2_depth`, `inference_2_match`), Module/Frontend/StereoDepth.py:270-282 and
 * Module/Frontend/Matching.py:28-40 (`from_partial_cov`).
 *   flow [2, 2, H, W] fp32 (sample 0 = stereo pair, sample 1 = temporal pair)
 *   logcov [2, 2, H, W] fp32 network log-sigma (cov = exp(2*logcov)); if cov_is_log == 0 it is already sigma^2
 *   outputs (all [H*W] planes, any may be NULL to skip):
 *   bl_fx = float(bl*fx), bl_fx_sq = float((bl*fx)**2), both evaluated in double by the caller exactly as
 *   the reference's Python scalars are, then rounded once to fp32 (what torch does with a Python scalar)
 *     disparity = |flow[0,0]|, disparity_cov = cov[0,0], depth = bl_fx * (1/disparity),
 *     depth_cov = bl_fx_sq * ((disparity_cov * (1/d^2)) / d^2), bad_mask = flow[0,0] <= 0 (uint8),
 *     match_flow [2,H,W] = flow[1], match_cov [3,H,W] = (cov[1,0], cov[1,1], 0)
 *   A frontend without covariances (MV_NOCOV_*; StereoDepth.py:121-128, Matching.py:142-147) says so through the outputs it leaves out:
 *   disparity_cov == depth_cov == NULL = no depth covariance, logcov[0] is not read; match_flow given and match_cov == NULL = no match
 *   covariance, logcov[1] is not read; logcov itself may be NULL when no covariance output is asked for.  Depth, disparity, bad_mask and
 *   match_flow are the same bits in every form.
 *   (A call that leaves those outputs out while passing logcov — legal before, though nothing in this library made it — now runs the
 *   partial kernel instead of the full one: the same bits for everything it writes.)
 */
int mv_frontend_epilogue(const float* flow, const float* logcov, int cov_is_log, int H, int W,
                         float bl_fx, float bl_fx_sq, float* disparity, float* disparity_cov,
                         float* depth, float* depth_cov, uint8_t* bad_mask, float* match_flow,
                         float* match_cov, mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * §8(f) rank 1  convex 8x upsampling (RAFT / FlowFormer `upsample_flow`), optionally fused with exp(2*x).
 * Replaces MemoryDecoder.upsample_flow at Module/Network/FlowFormerCov/covhead.py:124-126,133-135 (in-tree twin
 * Module/Network/PWCNet/pwc_cov/gru.py:40-52) and, with exp2_out = 1, the exp(2*cov) of flownet.py:44.
 *   flow [B, 2, h, w] fp32 (1/8 resolution);  mask [B, 576, h, w] fp32 (channel = tap*64 + sy*8 + sx)
 *   out  [B, 2, 8h, 8w] fp32 = sum_tap softmax_tap(mask_scale * mask) * (8 * flow at the tap's 3x3 neighbour, zero pad)
 *   the softmax weights are exp(m - max) * (1 / sum): one division per sub-pixel
 *   mask_scale: 0.25 for the flow branch (covhead.py:121), 1.0 for the log-sigma branch (scaled inside CovUpdateBlock :41)
 */
int mv_convex_upsample(const float* flow, const float* mask, float* out, int B, int h, int w,
                       float mask_scale, int exp2_out, mvStream_t stream);
/* the same with the mask in the decoder's own type: mask_dtype MV_F32 / MV_F16 / MV_BF16 ([B, 576, h, w] of that type, read as it is and
 * widened in registers — the arithmetic is the fp32 formula on the widened values; Fast mode, Config/Experiment/MACVO/MACVO_Fast.yaml:73-74:
 * the mask head runs under autocast and no `.float()` copy of the 11 MB mask is made).  flow and out stay fp32. */
int mv_convex_upsample_m(const float* flow, const void* mask, int mask_dtype, float* out, int B, int h, int w,
                         float mask_scale, int exp2_out, mvStream_t stream);
/* Frames whose sides are no multiples of 8.  The network pads such a frame, centred, before its encoders and un-pads its dense outputs (FlowFormerCov.inference,
 * flownet.py:37-44: `InputPadder(image1.shape)`, the public RAFT / FlowFormer padder in its default "sintel" mode — the FlowFormer submodule is unpinned in the
 * reference checkout; tools/flowformer_host.py states the padder).  mv_input_pad writes pad = {left, right, top, bottom} with left = ((-W) % 8) / 2 and
 * top = ((-H) % 8) / 2: the 1/8 maps are (H + top + bottom) / 8 x (W + left + right) / 8, frame pixel (y, x) is pixel (y + top, x + left) of the padded frame. */
void mv_input_pad(int H, int W, int32_t pad[4]);
/* mv_convex_upsample(_m) that stores only the window rows [y0, y0 + H) x columns [x0, x0 + W) of the 8h x 8w result (0 <= y0, y0 + H <= 8h, likewise x): the network's
 * `unpad` inside the kernel.  out [B, 2, H, W] fp32, dense (row pitch W), 4-byte aligned — nothing more is assumed, an odd H * W is fine;
 * out[b, c, y, x] has the bits mv_convex_upsample_m gives at (y + y0, x + x0).  Nothing outside `out` is written. */
int mv_convex_upsample_crop(const float* flow, const float* mask, float* out, int B, int h, int w, int y0, int x0, int H, int W,
                            float mask_scale, int exp2_out, mvStream_t stream);
int mv_convex_upsample_crop_m(const float* flow, const void* mask, int mask_dtype, float* out, int B, int h, int w, int y0, int x0,
                              int H, int W, float mask_scale, int exp2_out, mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * A10/A11 + MappingPointSelector  candidate generation for the covariance-aware keypoint selectors.
 * Replaces the dense part of Module/KeypointSelector.py: CovAwareSelector_NoDepth.select_point :362-400,
 * CovAwareSelector.select_point :260-327, MappingPointSelector.select_point :87-97 — quality map,
 * kernel_size x kernel_size min-NMS (NaN-propagating, equality test), border mask, (nan)median*1.5
 * thresholds with strict '<', optional validity masks, and torch.nonzero's row-major ordering.
 * The CPU `torch.randperm` (:331,:404,:98) stays on the host so indices are bit-exact; use
 * mv_kp_gather afterwards.
 */
enum { MV_KP_NODEPTH = 0, MV_KP_FULL = 1, MV_KP_MAPPING = 2,
       /* selectors that look at no map (mv_kp_random_lanes / mv_kp_grid, and as a frame pipe's selector_mode): */
       MV_KP_RANDOM = 3,      /* RandomSelector (KeypointSelector.py:103-118) */
       MV_KP_GRID = 4,        /* GridSelector (:216-247) */
       MV_KP_EXPLICIT = 5     /* frame pipe only: every frame's keypoints come from the caller (mv_frame_pipe_finish_keypoints[_dev]) */
};

typedef struct {
    int32_t H, W;
    int32_t mode;          /* MV_KP_* */
    int32_t kernel_size;   /* odd, 1..15 (NMS window)            */
    int32_t mask_width;    /* border exclusion in pixels (>= 1)  */
    float max_depth;       /* FULL: z0 < max_depth & z1 < max_depth; MAPPING: z0 < max_depth */
    float max_depth_cov;   /* FULL: min(max_depth_cov, 1.5*nanmedian); MAPPING: plain '<'    */
    float max_match_cov;   /* NODEPTH/FULL: min(max_match_cov, 1.5*median)                   */
} mvKpSelectParams;

/* bytes of scratch mv_kp_select needs for an H x W image.  The workspace must be ZERO-FILLED once after allocation;
 * every call leaves its internal counters zeroed again, so it can be reused call after call (on one stream). */
size_t mv_kp_select_workspace_bytes(int H, int W);

/*
 *   flow_cov   [3, H, W] fp32 (uu, vv, uv) — required for NODEPTH, optional (may be NULL) for FULL
 *   depth0/1, depth0_cov/1_cov [H, W] fp32 — FULL needs all four, MAPPING needs depth0 + depth0_cov
 *   mask_a, mask_b [H, W] uint8 (0 = reject) or NULL — depth0_est.mask / match_est.mask
 *   out_cand   [H*W] int32: linear indices v*W + u of the surviving pixels in row-major order
 *   out_count  [4] int32: {n_candidates, n_nms, 0, 0}
 *   out_stats  [4] fp32: {median_flow_q, thresh_flow_q, median_depth0_cov, thresh_depth0_cov}
 *
 * The second launch (medians, thresholds, compaction) keeps everything in registers and LDS while the NMS pixels ("records") and
 * the 64-pixel candidate words H * ceil(W / 64) both fit mv_kp_select_finish_capacity(H, W); past either limit the same steps run
 * against global memory — same results, several times slower.  Inputs that leave the in-register form: kernel_size 1 (every
 * non-NaN pixel is a record) from 128 x 128 up, noisy maps with kernel_size 3 from about 360 x 480 and with 5 at 720p, and any
 * image of more than 15 360 candidate words (taller than 768 rows at width 1280), whatever the window.
 */
int mv_kp_select(const float* flow_cov, const float* depth0, const float* depth0_cov,
                 const float* depth1, const float* depth1_cov, const uint8_t* mask_a,
                 const uint8_t* mask_b, const mvKpSelectParams* params /* host */, void* workspace,
                 size_t workspace_bytes, int32_t* out_cand, int32_t* out_count, float* out_stats,
                 mvStream_t stream);

/* Host only, launches nothing: what the in-register form of mv_kp_select's second launch holds for an H x W image in this
 * process — *max_records NMS pixels and *max_words candidate words (H * ceil(W / 64)) — for the variant the library would launch
 * (by the word count, and MV_KP_FINISH_SMALL_NT=512 in the environment, read once).  A call within both runs in registers, any
 * other against global memory; the results are the same.  MV_ERR_INVALID_ARG for non-positive sizes or null pointers. */
int mv_kp_select_finish_capacity(int H, int W, int32_t* max_records, int32_t* max_words);

/* selected[perm][..., 2:].roll(1, 1)  (KeypointSelector.py:331-332,404-405):
 *   out_uv[k] = (cand[perm[k]] % W, cand[perm[k]] / W) as int64 (u, v) */
int mv_kp_gather(const int32_t* cand, const int64_t* perm, int n_sel, int W, int64_t* out_uv,
                 mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * A12  keypoint tracking + the scalar-map gathers of Odometry/MACVO.py:198-232 in one launch.
 *   kp1 = kp0 + flow[:, v0, u0]; inbound = edge < u1 < W - edge & edge < v1 < H - edge (strict,
 *   Utility/Point.py:5-13); gathers at kp0 (integer) and at kp1 truncated toward zero
 *   (Module/Frontend/Frontend.py:117); match covariance read at the SOURCE pixel kp0 (:231);
 *   kp0 gets the constant sigma (match_cov_default, match_cov_default, 0) (:228-229).
 * Outputs are written for every input keypoint (row order preserved); `inbound` says which rows the
 * reference keeps.  kp0_uv int64 [N,2].  Planes are [H*W] fp32; match_cov is [3,H*W].
 *   out_kp0 [N,2] fp32 (= kp0 as float, or NULL); out_kp1 [N,2] fp32; out_inbound [N] uint8;
 *   out_vals [11, N] fp32 (SoA rows) = d0, disp0, sdisp0, sdd0, d1, disp1, sdisp1, sdd1, suu, svv, suv
 *   (for rows that are not inbound the kp1-side values are 0; absent maps give -1 like the reference)
 *   out_sigma0, out_sigma1 [N,3] fp32 or NULL: (uu, vv, uv) of kp0 / of the match, ready for mv_match_cov
 */
int mv_kp_track(const int64_t* kp0_uv, int N, const float* match_flow, const float* match_cov,
                const float* depth0, const float* disp0, const float* sdisp0, const float* sdd0,
                const float* depth1, const float* disp1, const float* sdisp1, const float* sdd1,
                int H, int W, int edge, float match_cov_default, float* out_kp0, float* out_kp1,
                uint8_t* out_inbound, float* out_vals, float* out_sigma0, float* out_sigma1,
                mvStream_t stream);

/* pixel2point_NED + world transform of Odometry/MACVO.py:240,273-281 (Utility/Point.py:15-17, pp.pixel2point):
 *   pos_Tc[n] = (d, ((u-cx)*d)/fx, ((v-cy)*d)/fy)   (fp32, NED)          kp_uv [N,2] fp32
 *   pos_Tw[n] = pose.Act(pos_Tc[n])                  (fp32, PyPose SO3_Act + t)  pose [7] fp32 device
 *   rot [9] fp64 = pose.rotation().matrix().to(float64) (matrix evaluated in fp32 like PyPose, then widened)
 * depth_vals[n * depth_stride] lets the caller pass a column of the mv_kp_track table directly.
 * Any of pos_Tc / pos_Tw / rot may be NULL. */
int mv_backproject(const float* kp_uv, const float* depth_vals, int depth_stride, float fx, float fy,
                   float cx, float cy, const float* pose, int N, float* pos_Tc, float* pos_Tw,
                   double* rot, mvStream_t stream);

/* Observation filters of Module/OutlierFilter.py fused into one validity mask (row order kept, no compaction):
 *   flags bit0 CovarianceSanityFilter :91-100 (no NaN/Inf in obs1_covTc / obs2_covTc)
 *         bit1 SimpleDepthFilter :103-121 (min_depth <= d1, d2 <= max_depth)
 *         bit2 LikelyFrontOfCamFilter :124-137 (d - 2*sqrt(sigma_d) > 0 for both observations)
 *   inbound [N] uint8 or NULL (border test of mv_kp_track); vals = the [11, N] SoA table of mv_kp_track
 *   valid [N] uint8; count [1] int32 = number of valid rows */
int mv_obs_filter(const uint8_t* inbound, const double* cov1, const double* cov2, const float* vals,
                  int flags, float min_depth, float max_depth, int N, uint8_t* valid, int32_t* count,
                  mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * A13-A16  MAC-VO covariance model.
 * Replaces Module/Covariance/Project2to3.py: MatchCovariance.estimate :124-181 (incl. the in-place
 * clamp of flow_cov :131), Utility/Math.py:43-63 (gaussain_full_kernels), Covariance_2to3_full
 * :377-423, create_3x3_matrix :426-433, and (optionally) the world-frame rotation
 * cov_Tw = R cov R^T of Odometry/MACVO.py:273-281.
 */
typedef struct {
    int32_t H, W;
    int32_t kernel_size;       /* odd, <= 31 */
    int32_t use_patch_var;     /* 1: weighted patch variance (flow_cov given or depth_cov NULL); 0: use depth_cov */
    float fx, fy, cx, cy;
    float min_flow_cov_sq;     /* config.min_flow_cov ** 2 (clamp applied to flow_cov[:, :2] IN PLACE) */
    float min_depth_cov;
} mvMatchCovParams;

/*
 *   depth_map [H, W] fp32; kp_uv [N, 2] fp32 (u, v) — patch centre = trunc(kp), (u - cx) uses the float
 *   flow_cov [N, 3] fp32 in/out (clamped in place); depth_cov [N] fp32 or NULL
 *   rot [9] fp64 row-major or NULL
 *   out_cov [N, 9] fp64 NED order (z, x, y); out_cov_rot [N, 9] fp64 = R cov R^T or NULL
 *   out_stats [N, 2] fp32 = (weighted mean depth, clamped variance) or NULL
 */
int mv_match_cov(const float* depth_map, const float* kp_uv, float* flow_cov,
                 const float* depth_cov, const double* rot, const mvMatchCovParams* params /* host */,
                 int N, double* out_cov, double* out_cov_rot, float* out_stats, mvStream_t stream);

/* Dense-mapping tail of run_pair (Odometry/MACVO.py:313-337, `mapping: true`): for the map pixels chosen by
 * MappingPointSelector (mv_kp_select MV_KP_MAPPING + mv_kp_gather, 2000 per frame) gather depth (:317) and its variance
 * (:320), pixel2point_NED (:318), prev_pose.Act (:334), the constant match sigma (:322-323) and optionally the colour
 * (imageL*255 -> uint8, :326-328).  The covariance of these points is one mv_match_cov call on out_uv / out_sigma
 * (:324 — note the reference stores it UNROTATED, in the camera frame).
 *   uv [N,2] int64; depth, depth_cov [H*W] fp32; image [3,H,W] fp32 in [0,1] or NULL; pose fp32[7] (device)
 *   out_uv [N,2], out_d [N], out_sdd [N], out_sigma [N,3], out_Tc [N,3], out_Tw [N,3] fp32, out_color [N,3] uint8 (NULL ok) */
int mv_map_points(const int64_t* uv, int N, const float* depth, const float* depth_cov, const float* image, int H, int W,
                  float fx, float fy, float cx, float cy, const float* pose, float match_cov_default, float* out_uv,
                  float* out_d, float* out_sdd, float* out_sigma, float* out_Tc, float* out_Tw, uint8_t* out_color,
                  mvStream_t stream);

/* Both ObsCovModel.estimate calls of one frame (Odometry/MACVO.py:241-242) in ONE launch: set 0 = kp0 on the previous
 * frame's depth map (+ optional world rotation, :273-281), set 1 = kp1 on the current depth map.  Same arithmetic as
 * two mv_match_cov calls with use_patch_var = 1 (both flow_cov arrays are clamped in place). */
int mv_match_cov_pair(const float* depth_map0, const float* kp_uv0, float* flow_cov0, const double* rot0,
                      double* out_cov0, double* out_cov_rot0, const float* depth_map1, const float* kp_uv1,
                      float* flow_cov1, double* out_cov1, const mvMatchCovParams* params /* host */, int N,
                      mvStream_t stream);

/* The other observation-covariance models of ICovariance2to3 (Module/Covariance/Project2to3.py), selected by `cov.obs.type:`.
 *   MV_COV_MATCH  MatchCovariance (:113-191) — exactly mv_match_cov
 *   MV_COV_GMM    GaussianMixtureCovariance (:194-262) + gaussian_mixture_mean_var (Utility/Math.py:66-93): the K x K patch is gathered
 *                 from the depth map AND the dense depth-variance map (depth_cov_map, required), the normalised Gaussian weights below
 *                 1e-3 are zeroed and the rest renormalised; mean = sum p z, var = (sum p (c + z^2) - mean^2) / 2 (the reference's /2),
 *                 NO min_depth_cov clamp; flow_cov[:, :2] is clamped in place; use_patch_var = 0 -> var = depth_cov.  Every weight below
 *                 the threshold -> NaN row (0 / 0), as in the reference.
 *   MV_COV_NONE   NoCovariance (:48-57): the fp64 identity; flow_cov is NOT clamped (read, written back unchanged).
 * modifiers: an ordered chain of up to 4 steps packed 4 bits per step, innermost (first applied) in bits 0-3, 0 = end of chain:
 *   MV_COVMOD_DIAG       Modifier_Diagonalize (:281-301): off-diagonal entries := 0
 *   MV_COVMOD_NORMALIZE  Modifier_Normalize (:305-323): cov /= det(cov) (the determinant itself, as the reference computes it)
 * both applied in fp64 to the camera-frame covariance, before R cov R^T (MACVO.py:241-281).
 * out_stats [N, 2] fp32 = (mean depth, variance) for MATCH / GMM, NaN for NONE. */
enum { MV_COV_MATCH = 0, MV_COV_GMM = 1, MV_COV_NONE = 2 };
enum { MV_COVMOD_DIAG = 1, MV_COVMOD_NORMALIZE = 2 };
/* Covariances a frontend does NOT provide (IFrontend.provide_cov, Frontend.py:137-139): the depth model's (no disparity variance, no depth
 * variance: FlowFormerDepth) and / or the matcher's (no match covariance: FlowFormerMatcher).  0 = both there, as everywhere before. */
enum { MV_NOCOV_DEPTH = 1, MV_NOCOV_MATCH = 2 };

int mv_obs_cov(int model, int32_t modifiers, const float* depth_map, const float* depth_cov_map, const float* kp_uv,
               float* flow_cov, const float* depth_cov, const double* rot, const mvMatchCovParams* params /* host */, int N,
               double* out_cov, double* out_cov_rot, float* out_stats, mvStream_t stream);

/* mv_match_cov_pair_lanes with a model and a modifier chain (use_patch_var = 1; depth_cov_map0/1 required for MV_COV_GMM). */
int mv_obs_cov_pair_lanes(int model, int32_t modifiers, const float* depth_map0, const float* depth_cov_map0, const float* kp_uv0,
                          float* flow_cov0, const double* rot0, double* out_cov0, double* out_cov_rot0, const float* depth_map1,
                          const float* depth_cov_map1, const float* kp_uv1, float* flow_cov1, double* out_cov1,
                          const mvMatchCovParams* params /* host */, int lanes, const int32_t* n_live, int cap, mvStream_t stream);
/* mv_obs_cov_pair_lanes of a frame whose matcher gives no covariance (MV_NOCOV_MATCH; MACVO.py:231-232,241-242): set 0 as above; set 1 is the model
 * called with flow_cov = None (Project2to3.py:128-135,162-172,211-218,254-255) — sigma = (c, c, 0) with c = model_match_cov_default (the covariance
 * model's OWN match_cov_default), not clamped by min_flow_cov; the depth variance is depth_cov1 [lanes, cap] (the depth-variance map gathered at the
 * truncated kp1: row 7 of mv_kp_track's value table) where the depth model gives one — MATCH then clamps it by min_depth_cov, GMM keeps its mixture mean
 * and takes this variance — and the patch statistic when depth_cov1 is NULL (MATCH only: GMM needs the depth model's variance).  The set-1 sigma table
 * is neither read nor written: it keeps the (-1, -1, -1) placeholders of MACVO.py:263. */
int mv_obs_cov_pair_nomatch_lanes(int model, int32_t modifiers, const float* depth_map0, const float* depth_cov_map0, const float* kp_uv0,
                                  float* flow_cov0, const double* rot0, double* out_cov0, double* out_cov_rot0, const float* depth_map1,
                                  const float* depth_cov_map1, const float* kp_uv1, const float* depth_cov1, float model_match_cov_default,
                                  double* out_cov1, const mvMatchCovParams* params /* host */, int lanes, const int32_t* n_live, int cap,
                                  mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * TartanMotionNet motion prior (Module/MotionModel.py:90-123): everything around the learned PoseNet.
 *
 * mv_motion_input_lanes: TartanStereoVOMotion.inference's input (StereoVO_Interface.py:177-188) for `lanes` frames in one launch:
 *   flow  lane l at flow + l * flow_lane_stride   [2, H, W] fp32 (the temporal match flow, match01.flow)
 *   depth lane l at depth + l * depth_lane_stride [H, W] fp32    (depth1.depth)
 *   out   [lanes, 5, 112, 160] fp32 = cat(flow * 0.05, depth transform, intrinsic layer) after cropAndResize(x, (112, 160)):
 *         centre crop to (112 s, 160 s), s = min(H / 112, W / 160) (an odd difference keeps one more row / column), bilinear with
 *         align_corners = True.  Depth: reciprocal * bl_fx * 0.02, NaN -> 0, +-inf -> +-FLT_MAX, clamp(min = 0), / bl_fx / 0.005.
 *         Intrinsic layer with the reference's swapped arguments: channel 3 = (col - cy + 0.5) / fy, channel 4 = (row - cx + 0.5) / fx.
 *   bl_fx = frame_baseline * fx as a double, rounded once.  Requires H >= 112 and W >= 160.
 * mv_pose_exp_compose: out[i] = prev[i] @ Exp(se3(raw[i] * pose_norm)) in fp32 (PyPose right multiplication, fp32 small-angle branch);
 *   prev / out [n, 7] (tx ty tz qx qy qz qw), raw row i at raw + i * raw_stride (6 values), pose_norm [6] (0.13 x 3, 0.013 x 3). */
int mv_motion_input_lanes(int lanes, int H, int W, const float* flow, long long flow_lane_stride, const float* depth,
                          long long depth_lane_stride, float fx, float fy, float cx, float cy, float bl_fx, float* out, mvStream_t stream);
int mv_pose_exp_compose(int n, const float* prev, const float* raw, long long raw_stride, const float* pose_norm, float* out,
                        mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * A17-A22  covariance-weighted two-frame pose-graph solve, batched over independent problems.
 * Replaces TwoFrame_PGO._optimize (Module/Optimization/TwoFramePGO/Optimizer.py:81-102), the residual
 * graphs + analytic Jacobians (Module/Optimization/TwoFramePGO/Graphs.py:33-231), LM_analytic.step
 * (Module/Optimization/PyposeOptimizers.py:160-194) and the PyPose 0.6.8 pieces they call
 * (Huber, FastTriggs, TrustRegion, PINV, StopOnPlateau, SE3 Exp/Act/Inv).  All arithmetic in fp64
 * after the fp32 buffer construction the reference performs (Optimizer.py:84-85).
 */
enum { MV_GRAPH_ICP = 0, MV_GRAPH_REPROJ = 1, MV_GRAPH_DISP = 2 };

typedef struct {
    double huber_delta;  /* 0.1   */
    double radius;       /* 1e3   (damping0 = 1/radius) */
    double tr_high, tr_low, tr_up, tr_down, tr_factor, tr_min, tr_max; /* .5 1e-3 2 .5 .5 1e-6 1e16 */
    double diag_min, diag_max; /* 1e-6 1e32 */
    double decreasing;   /* 1e-5  */
    double pinv_rcond;   /* 1e-15 */
    int32_t reject;      /* 16    */
    int32_t max_steps;   /* 10    */
    int32_t patience;    /* 2     */
    int32_t stop_on_reject; /* 1: StopOnPlateau ends the outer loop when the last step's reject_count >= this value
                             * (PyPose 0.6.x scheduler: `if optimizer.reject_count > 0` => 1, the default; `reject` (16)
                             * = "only after the maximum number of rejections"; 0 = rejections never stop the loop).
                             * PyPose is un-vendored (requirements.txt:1) => from memory, hence a named knob. */
} mvLMParams;

void mv_lm_default_params(mvLMParams* p /* host */);

/*
 * Problem p owns points [offsets[p], offsets[p+1]) of the concatenated per-point arrays.
 *   offsets [nprob+1] int32; init_pose [nprob,7] fp32 (tx ty tz qx qy qz qw);
 *   intrinsics [nprob,4] fp32 (fx fy cx cy); baseline [nprob] fp32
 *   pos_Tw [Ntot,3] fp32; cov_Tw [Ntot,9] fp64 (ICP only, else may be NULL)
 *   pixel2_uv [Ntot,2] fp32; pixel2_d [Ntot] fp32 (ICP); pixel2_disp, pixel2_disp_cov [Ntot] fp32 (DISP)
 *   pixel2_uv_cov [Ntot,3] fp32 (REPROJ/DISP); obs2_covTc [Ntot,9] fp64 (ICP)
 *   valid [Ntot] uint8 or NULL: rows with 0 are skipped (the reference drops them from the map instead:
 *     Odometry/MACVO.py:200-206 border filter, :269-270 outlier filter); min_points: a problem with fewer valid
 *     rows is not optimised and returns init_pose with steps = 0 (lost track, MACVO.py:303-307; pass 0 to disable)
 *   out_pose [nprob,7] fp64; out_info [nprob,4] fp64 = {final loss, outer steps, last reject_count, initial loss}
 *   out_pose_f32 [nprob,7] fp32 or NULL: `motion.float()` of write_graph_data (Optimizer.py:104-108)
 */
int mv_pgo_solve(int nprob, const int32_t* offsets, int graph_type, const float* init_pose,
                 const float* intrinsics, const float* baseline, const float* pos_Tw,
                 const double* cov_Tw, const float* pixel2_uv, const float* pixel2_d,
                 const float* pixel2_disp, const float* pixel2_disp_cov, const float* pixel2_uv_cov,
                 const double* obs2_covTc, const uint8_t* valid, int min_points,
                 const mvLMParams* params /* host */, double* out_pose, double* out_info,
                 float* out_pose_f32, mvStream_t stream);
/* mv_pgo_solve with the rest of the backend folded into the same launch (Module/OutlierFilter.py:91-141, Odometry/MACVO.py:273-281,
 * Optimizer.py:81-102).  Before a problem's rows are read its workgroup
 *   (1) filter_flags >= 0: runs the observation filters of mv_obs_filter_lanes over the problem's rows (inbound, cov_Tc = cov1, obs2_covTc = cov2, the
 *       [11, nprob, cap] value table `vals`; cap = rows per problem) and writes `valid_out` / `count_out` [nprob] — the solve then reads valid_out;
 *       filter_flags < 0: `valid` is an input as in mv_pgo_solve;
 *   (2) rotates the first n_live[prob] rows into the world frame with the problem's init_pose — pos_Tw = T p_cam (fp32 PyPose SE3 Act), cov_Tw = R cov_Tc
 *       R^T (fp64), out_rot [nprob, 9] = R — mv_pose_apply_lanes' arithmetic, written to pos_Tw / cov_Tw (cov_Tc / cov_Tw may both be NULL).
 * Same bits as the separate kernels.  pose_sink (or NULL): a second fp32 copy of the optimised poses [nprob, 7].  nprob <= MV_MAX_LANES.  The filters address a problem's
 * rows through `offsets` like the rest of the launch (rows [offsets[l], offsets[l + 1]), the value table's row stride = offsets[nprob]); the frame driver passes
 * the static table {0, cap, 2 cap, ...}.  n_live: host int32 [nprob], n_live[l] <= offsets[l + 1] - offsets[l]. */
int mv_pgo_solve_posed(int nprob, const int32_t* offsets, const int32_t* n_live, int cap, int graph_type, const float* init_pose,
                       const float* intrinsics, const float* baseline, const float* pos_Tc, const double* cov_Tc,
                       float* pos_Tw, double* cov_Tw, double* out_rot, const float* pixel2_uv, const float* pixel2_d,
                       const float* pixel2_disp, const float* pixel2_disp_cov, const float* pixel2_uv_cov,
                       const double* obs2_covTc, int filter_flags, float filter_min_depth, float filter_max_depth,
                       const uint8_t* inbound, const float* vals, uint8_t* valid, int32_t* count_out, int min_points,
                       const mvLMParams* params, double* out_pose, double* out_info, float* out_pose_f32, float* pose_sink,
                       mvStream_t stream);
/* ... of the device-driven frame (round 6): the live-row count of problem l is n_live_dev[l * n_live_stride] in DEVICE memory (<= cap; written by
 * mv_backend_front_draw_lanes earlier on the stream) — the number of selected keypoints never reaches the host.  Everything else as above. */
int mv_pgo_solve_posed_dev(int nprob, const int32_t* offsets, const int32_t* n_live_dev, int n_live_stride, int cap, int graph_type,
                           const float* init_pose, const float* intrinsics, const float* baseline, const float* pos_Tc, const double* cov_Tc,
                           float* pos_Tw, double* cov_Tw, double* out_rot, const float* pixel2_uv, const float* pixel2_d,
                           const float* pixel2_disp, const float* pixel2_disp_cov, const float* pixel2_uv_cov, const double* obs2_covTc,
                           int filter_flags, float filter_min_depth, float filter_max_depth, const uint8_t* inbound, const float* vals,
                           uint8_t* valid, int32_t* count_out, int min_points, const mvLMParams* params, double* out_pose, double* out_info,
                           float* out_pose_f32, float* pose_sink, mvStream_t stream);
/* The motion-model forms (TartanMotionNet: Odometry/MACVO.py:193-194,273-281,303-307): as mv_pgo_solve_posed / mv_pgo_solve_posed_dev, but the rows are
 * rotated into the world frame with init_pose (the previous pose) while LM starts from start_pose [nprob, 7] (the motion-model prior); a problem with
 * fewer than min_points valid rows returns start_pose.  The entry points above compile to the same kernels as before. */
int mv_pgo_solve_posed_motion(int nprob, const int32_t* offsets, const int32_t* n_live, int cap, int graph_type, const float* init_pose,
                              const float* start_pose, const float* intrinsics, const float* baseline, const float* pos_Tc, const double* cov_Tc,
                              float* pos_Tw, double* cov_Tw, double* out_rot, const float* pixel2_uv, const float* pixel2_d,
                              const float* pixel2_disp, const float* pixel2_disp_cov, const float* pixel2_uv_cov,
                              const double* obs2_covTc, int filter_flags, float filter_min_depth, float filter_max_depth,
                              const uint8_t* inbound, const float* vals, uint8_t* valid, int32_t* count_out, int min_points,
                              const mvLMParams* params, double* out_pose, double* out_info, float* out_pose_f32, float* pose_sink,
                              mvStream_t stream);
int mv_pgo_solve_posed_motion_dev(int nprob, const int32_t* offsets, const int32_t* n_live_dev, int n_live_stride, int cap, int graph_type,
                                  const float* init_pose, const float* start_pose, const float* intrinsics, const float* baseline,
                                  const float* pos_Tc, const double* cov_Tc, float* pos_Tw, double* cov_Tw, double* out_rot,
                                  const float* pixel2_uv, const float* pixel2_d, const float* pixel2_disp, const float* pixel2_disp_cov,
                                  const float* pixel2_uv_cov, const double* obs2_covTc, int filter_flags, float filter_min_depth,
                                  float filter_max_depth, const uint8_t* inbound, const float* vals, uint8_t* valid, int32_t* count_out,
                                  int min_points, const mvLMParams* params, double* out_pose, double* out_info, float* out_pose_f32,
                                  float* pose_sink, mvStream_t stream);
/* The local-frame forms (Local_TwoFrame_PGO: Module/Optimization/TwoFramePGO/Optimizer.py:111-150).  ref_pose [nprob,7] fp32 is T_o2w, the pose stored at map
 * index frame_idx - 1 when get_graph_data runs (:119-121).  world_to_optim (:131-143) and optim_to_world (:145-150, Utility/Math.py:124-133) in the reference's
 * precisions and order: T_w2o = Inv(ref_pose) and the LM start T_w2o @ start in fp32; every row read as pos_To = Act(T_w2o, pos_Tw) in fp32 and
 * cov_To = (R_w2o cov_Tw) R_w2o^T in fp64 with R_w2o the fp32 rotation matrix widened — the pos_Tw / cov_Tw tables keep their world-frame contents (in the
 * posed forms the world registration with init_pose still runs first and is what is stored); the unchanged LM loop; then
 * NormalizeQuat(ref_pose @ float(result)) in fp32 -> out_pose_f32 and pose_sink.  out_pose (fp64) keeps the local-frame LM result, out_info is as above.
 * A problem with fewer than min_points valid rows returns its start pose unchanged, in the world frame (Odometry/MACVO.py:303-307).
 * mv_pgo_solve_local: mv_pgo_solve + ref_pose.  mv_pgo_solve_posed_local(_dev): mv_pgo_solve_posed(_dev) + start_pose (NULL = init_pose; given = the
 * motion-model form, Odometry/MACVO.py:193-194) + ref_pose.  The entry points above compile to the same kernels as before. */
int mv_pgo_solve_local(int nprob, const int32_t* offsets, int graph_type, const float* init_pose, const float* ref_pose,
                       const float* intrinsics, const float* baseline, const float* pos_Tw, const double* cov_Tw,
                       const float* pixel2_uv, const float* pixel2_d, const float* pixel2_disp, const float* pixel2_disp_cov,
                       const float* pixel2_uv_cov, const double* obs2_covTc, const uint8_t* valid, int min_points,
                       const mvLMParams* params /* host */, double* out_pose, double* out_info, float* out_pose_f32, mvStream_t stream);
int mv_pgo_solve_posed_local(int nprob, const int32_t* offsets, const int32_t* n_live, int cap, int graph_type, const float* init_pose,
                             const float* start_pose, const float* ref_pose, const float* intrinsics, const float* baseline, const float* pos_Tc,
                             const double* cov_Tc, float* pos_Tw, double* cov_Tw, double* out_rot, const float* pixel2_uv, const float* pixel2_d,
                             const float* pixel2_disp, const float* pixel2_disp_cov, const float* pixel2_uv_cov, const double* obs2_covTc,
                             int filter_flags, float filter_min_depth, float filter_max_depth, const uint8_t* inbound, const float* vals,
                             uint8_t* valid, int32_t* count_out, int min_points, const mvLMParams* params, double* out_pose, double* out_info,
                             float* out_pose_f32, float* pose_sink, mvStream_t stream);
int mv_pgo_solve_posed_local_dev(int nprob, const int32_t* offsets, const int32_t* n_live_dev, int n_live_stride, int cap, int graph_type,
                                 const float* init_pose, const float* start_pose, const float* ref_pose, const float* intrinsics,
                                 const float* baseline, const float* pos_Tc, const double* cov_Tc, float* pos_Tw, double* cov_Tw, double* out_rot,
                                 const float* pixel2_uv, const float* pixel2_d, const float* pixel2_disp, const float* pixel2_disp_cov,
                                 const float* pixel2_uv_cov, const double* obs2_covTc, int filter_flags, float filter_min_depth,
                                 float filter_max_depth, const uint8_t* inbound, const float* vals, uint8_t* valid, int32_t* count_out,
                                 int min_points, const mvLMParams* params, double* out_pose, double* out_info, float* out_pose_f32,
                                 float* pose_sink, mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * A23  PWC-Net local correlation, forward (the reference's only hand-written CUDA kernel; non-default matcher path).
 * Replaces `FunctionCorrelation(tenFirst, tenSecond)` = `_FunctionCorrelation.forward`
 * (Module/Network/PWCNet/pwc/correlation.py:277-325; kernels :8-33 rearrange, :35-103 updateOutput):
 *   out[b, 9*(dy+4)+(dx+4), y, x] = (1/C) * sum_c first[b,c,y,x] * second[b,c,y+dy,x+dx],  dx,dy in [-4,4], zero padded.
 * first, second: [B, C, H, W] fp32 contiguous (NCHW, as the reference asserts :283-284); out: [B, 81, H, W] fp32.
 * Callers: pwc_model.py:178-233 (five pyramid levels), pwc_model_tartanvo.py:231,259, RAFTCov.py:7.
 */
int mv_local_corr81(const float* first, const float* second, float* out, int B, int C, int H, int W,
                    mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * SURVEY §8(f) rank 4  device-resident VisualMap (tracking map of one sequence), output poses, MotionInterpolate.
 * Replaces Module/Map/VisualMap.py:15-133 + Module/Map/Graph.py:19-298 as driven by Odometry/MACVO.py:158-171,244-311
 * (MatchObs.init, `match_obs[mask]`, points.push(...[mask]), push_keyframe, the six edge updates, the lost-track flag), which
 * the reference runs on the CPU behind ~25 `.cpu()` copies per frame; Odometry/Interface.py:47-49 (body poses of poses.npy);
 * Module/MapProcessor.py:52-76 (MotionInterpolate) with Utility/Math.py:96-133.  The stores are caller-owned device arrays
 * (SoA, the reference's field names / dtypes, VisualMap.py:23-69); `counts` is a DEVICE int64[6] = {frames, matches, points,
 * lost frames, refused appends, map points} advanced by the kernel itself, so registering a frame needs no host synchronisation: the host only has to keep
 * capacity >= an upper bound of the rows pushed (rows selected).
 */
typedef struct {
    /* frames  [cap_f, .] */
    float* K;                 /* [.,3,3] */
    float* baseline;          /* [.]     */
    float* pose;              /* [.,7]   sensor-to-world; prior at push time, overwritten by the optimised pose */
    float* T_BS;              /* [.,7]   */
    uint8_t* need_interp;     /* [.]     */
    int64_t* time_ns;         /* [.]     */
    /* points  [cap_p, .] */
    float* pos_Tw;            /* [.,3]   */
    double* cov_Tw;           /* [.,3,3] */
    uint8_t* color;           /* [.,3]   */
    /* match   [cap_m, .]  (VisualMap.py:51-69) */
    float *pixel1_uv, *pixel2_uv;                    /* [.,2] */
    float *pixel1_d, *pixel2_d, *pixel1_disp, *pixel2_disp, *pixel1_disp_cov, *pixel2_disp_cov;   /* [.,1] */
    double *obs1_covTc, *obs2_covTc;                 /* [.,3,3] */
    float *pixel1_uv_cov, *pixel2_uv_cov;            /* [.,3] */
    float *pixel1_d_cov, *pixel2_d_cov;              /* [.,1] */
    /* edges (Graph.py: DenseEdge_Multi ranges [n, max_deg, 2] + num [n]; SingleEdge mapping [n]; SparseEdge_Multi edges
     * [n, max_deg] + deg [n]); all int64, -1 = empty */
    int64_t *frame2match_ranges, *frame2match_num, *frame2map_ranges, *frame2map_num;
    int64_t *match2frame1, *match2frame2, *match2point;
    int64_t *point2match_edges, *point2match_deg;
    int64_t* counts;          /* device int64[6]: {frames, matches, points, lost frames, REFUSED appends (error word), map points} */
    int32_t max_pt_obs;       /* 5  (VisualMap.py:18) */
    int32_t max_frame_range;  /* 2  (VisualMap.py:19) */
    /* capacities (rows) of the frame / match / point stores and their edge tables.  The row offsets come from the DEVICE-side
     * counts, so the kernel itself refuses an append that would not fit (counts unchanged, counts[4] += 1, out_frame_idx = -1)
     * instead of writing past the stores; a frame2match range dropped because a frame already has max_frame_range ranges (the
     * reference raises there, Graph.py:183-186) is counted in counts[4] as well.  The host reads counts[4] at its next
     * synchronisation point (DeviceVisualMap.sizes -> MV_ERR_WORKSPACE). */
    int64_t cap_frames, cap_match, cap_points;
    /* dense map points of `mapping: true` (VisualMap.map_points, VisualMap.py:47-54; indexed by the frame2map edges) */
    float* mp_pos_Tw;         /* [cap_mp,3]   */
    double* mp_cov_Tw;        /* [cap_mp,3,3] camera-frame covariance, stored unrotated as the reference does (MACVO.py:324,334) */
    uint8_t* mp_color;        /* [cap_mp,3]   */
    int64_t cap_map_points;   /* 0 = no map-point store attached */
} mvMapStores;

/* one frame's observations as the tracking kernels leave them (row order of the selected keypoints; `valid` = border test
 * AND outlier filter, i.e. the rows the reference keeps, MACVO.py:200-206,269-270) */
typedef struct {
    int32_t n_rows;           /* selected keypoints of the frame (0 for the very first frame)           */
    int32_t table_stride;     /* row stride of the SoA `vals` table (>= n_rows)                          */
    int32_t prev_frame;       /* map index of the previous keyframe, -1 for the first frame (initialize) */
    int32_t min_num_point;    /* fewer kept rows => need_interp (MACVO.py:303-307)                       */
    const uint8_t* valid;     /* [n_rows] or NULL (keep all)                                             */
    const float *kp0, *kp1;   /* [n_rows,2] pixel1_uv / pixel2_uv                                        */
    const float* vals;        /* [11, table_stride] table of mv_kp_track                                 */
    const float *sigma0, *sigma1;       /* [n_rows,3] pixel1_uv_cov / pixel2_uv_cov (after the in-place clamp)  */
    const double *cov0, *cov1;          /* [n_rows,9] obs1_covTc / obs2_covTc                                   */
    const float* pos_Tw;      /* [n_rows,3]  */
    const double* cov0_world; /* [n_rows,9] R cov0 R^T (MACVO.py:273-281)                                */
    const uint8_t* color;     /* [n_rows,3] or NULL                                                      */
    const float* K;           /* [9] device */
    const float* T_BS;        /* [7] device */
    const float* prior_pose;  /* [7] device or NULL (identity): the pose the frame is pushed with         */
    float baseline;
    int64_t time_ns;
    int32_t* out_frame_idx;   /* device int32[1] or NULL: the map index the frame received                */
} mvMapFrame;

int mv_map_append(const mvMapFrame* frame /* host */, const mvMapStores* stores /* host */, mvStream_t stream);
/* Dense-mapping tail (Odometry/MACVO.py:329-337): `map_points.push(PointNode.init({pos_Tw, cov_Tw, color}))` +
 * `frame2map.add(frame_idx, num_map_orig, n)` for the NEWEST registered frame (counts[0] - 1).  n rows of pos_Tw [n,3] fp32,
 * cov [n,9] fp64, color [n,3] uint8 (NULL = zeros), all device.  Refused (counts[4] += 1) when the store or the frame's range
 * slots are full. */
int mv_map_append_points(const mvMapStores* stores /* host */, int n, const float* pos_Tw, const double* cov, const uint8_t* color,
                         mvStream_t stream);
/* A non-keyframe (UniformKeyframe: Module/KeyframeSelector.py:31-39; Odometry/MACVO.py:177-179 -> push_keyframe(frame1, pose of the previous keyframe,
 * need_interp=True), :339-348): ONE frame row with need_interp = 1 and pose_dev [7] fp32 (device), no frame2match range, no match rows, no point rows.  Only
 * counts[0] advances (counts[3], the lost frames, does not).  Refused (counts[4] += 1) when the frame store is full. */
int mv_map_append_skipped(const mvMapStores* stores /* host */, const float* K_dev, const float* T_BS_dev, const float* pose_dev, float baseline,
                          int64_t time_ns, mvStream_t stream);
/* out[i] = T_BS[i] @ pose[i] @ T_BS[i]^-1 in fp32 (Odometry/Interface.py:47-49) */
int mv_body_poses(const float* pose, const float* T_BS, int T, float* out, mvStream_t stream);
/* MotionInterpolate.elaborate_map on pose [T,7] in place (fp64 inside); scratch: double[7*(T-1)]; out_count int32[1] or NULL =
 * number of interpolated motions */
int mv_motion_interpolate(float* pose, const uint8_t* need_interp, int T, double* scratch, int32_t* out_count,
                          mvStream_t stream);

/* Lane-batched registration: `lanes` INDEPENDENT sequences, each into its OWN map, in one launch (one workgroup per lane).  This is what the reference's
 * multi-sequence driver does one sequence after the other (Scripts/Experiment/Experiment_MACVO.py:55-58: every sequence runs MACVO.run_pair and keeps its own
 * VisualMap) — per lane exactly mv_map_append: Odometry/MACVO.py:244-311,339-347 on Module/Map/VisualMap.py:15-133 + Module/Map/Graph.py:86-104,144-147,
 * 183-186,228-229.  The tables are the frame driver's backend buffers as they lie: per-keypoint tables [lanes, cap, .], the value table [11, lanes, cap] (row
 * stride lanes * cap, lane l at column l * cap), valid [lanes, cap] or NULL.  n_rows / time_ns are HOST arrays [lanes] (n_rows[l] <= cap; a device-driven frame
 * passes cap and lets `valid` compact); T_BS and prior_pose are device [lanes, 7]; K, baseline, prev_frame, min_num_point are the same for every lane.
 * stores_dev is a DEVICE array mvMapStores[lanes] (at MV_MAX_LANES x ~45 pointers the descriptors do not fit in kernel arguments); it must not be rewritten
 * while a launch that reads it may be in flight.  Refusal (counts[4] += 1, nothing else written) is decided per lane. */
typedef struct {
    int32_t lanes, cap;
    int32_t prev_frame;       /* map index of the previous keyframe (the lanes advance in lock-step), -1 for the first frame */
    int32_t min_num_point;
    const int32_t* n_rows;    /* HOST [lanes] */
    const int64_t* time_ns;   /* HOST [lanes] */
    const uint8_t* valid;     /* [lanes, cap] or NULL */
    const float *kp0, *kp1;   /* [lanes, cap, 2] */
    const float* vals;        /* [11, lanes, cap] */
    const float *sigma0, *sigma1;       /* [lanes, cap, 3] */
    const double *cov0, *cov1;          /* [lanes, cap, 9] */
    const float* pos_Tw;      /* [lanes, cap, 3] */
    const double* cov0_world; /* [lanes, cap, 9] */
    const uint8_t* color;     /* [lanes, cap, 3] or NULL */
    const float* K;           /* [9] device */
    const float* T_BS;        /* [lanes, 7] device */
    const float* prior_pose;  /* [lanes, 7] device or NULL (identity) */
    float baseline;
} mvMapFrameLanes;
int mv_map_append_lanes(const mvMapFrameLanes* frames /* host */, const mvMapStores* stores_dev /* DEVICE [lanes] */, mvStream_t stream);
/* mv_map_append_skipped for every lane (Odometry/MACVO.py:177-179,339-348): one need_interp row per lane with pose_dev[l] ([lanes, 7], each lane's prior) and
 * T_BS_dev[l]; time_ns is a HOST array [lanes]. */
int mv_map_append_skipped_lanes(const mvMapStores* stores_dev /* DEVICE [lanes] */, int lanes, const float* K_dev, const float* T_BS_dev, const float* pose_dev,
                                float baseline, const int64_t* time_ns /* host [lanes] */, mvStream_t stream);
/* write_graph_data (Module/Optimization/TwoFramePGO/Optimizer.py:104-108) for every lane: pose_dev [lanes, 7] over row frame_idx of each lane's frames.pose
 * (the lanes' stores are different allocations, so one copy cannot do it).  A row outside a lane's store is left alone. */
int mv_map_set_pose_lanes(const mvMapStores* stores_dev /* DEVICE [lanes] */, int lanes, int frame_idx, const float* pose_dev, mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * Lane-batched variants: the same kernels over `lanes` INDEPENDENT frames (sequences) in ONE launch.  This is the
 * reference's batching point (Module/Frontend/Frontend.py:219-224 concatenates pairs along the batch axis) carried through
 * the rest of run_pair, for BASELINE configs[4] (batch-32 frames per GPU).  Layout rule: every argument gains a leading
 * [lanes] dimension (maps [lanes, ch, H, W]; per-keypoint tables [lanes, cap, .] with `cap` rows of capacity per lane of
 * which n_live[l] are live — n_live is a HOST int32[lanes], travels as a kernel argument), EXCEPT the SoA value table of
 * mv_kp_track, which is [11, lanes, cap] so that each of its rows is one concatenated per-point column that mv_pgo_solve
 * takes directly (problem l = rows [l*cap, (l+1)*cap), dead rows masked by `valid`, which mv_obs_filter_lanes zeroes).
 * The plain entry points above are these with lanes = 1, cap = N.  MV_KP_MAPPING supports lanes = 1 only. */
int mv_frontend_epilogue_lanes(const float* flow, const float* logcov, int cov_is_log, int H, int W, float bl_fx,
                               float bl_fx_sq, float* disparity, float* disparity_cov, float* depth, float* depth_cov,
                               uint8_t* bad_mask, float* match_flow, float* match_cov, int lanes, mvStream_t stream);
/* workspace: lanes consecutive copies of mv_kp_select_workspace_bytes(H, W), zero-filled once */
int mv_kp_select_lanes(const float* flow_cov, const float* depth0, const float* depth0_cov, const float* depth1,
                       const float* depth1_cov, const uint8_t* mask_a, const uint8_t* mask_b,
                       const mvKpSelectParams* params /* host */, void* workspace, size_t workspace_bytes,
                       int32_t* out_cand /* [lanes, H*W] */, int32_t* out_count /* [lanes, 4] */,
                       float* out_stats /* [lanes, 4] */, int lanes, mvStream_t stream);
/* The pose-dependent remainder of a frame's backend (Odometry/MACVO.py:273-281), split off so that gather / track / back-projection /
 * covariances / filters can run before the previous frame's solve has finished: pos_Tw = T * pos_Tc (fp32 SE3 Act),
 * rot [lanes, 9] = R as fp64, cov_rot = R cov R^T (fp64).  Bit-identical to what mv_backproject(pose) and mv_match_cov(rot,
 * out_cov_rot) produce.  pose [lanes, 7] device; tables [lanes, cap, .]; pos_* / cov* pairs may be null together. */
int mv_pose_apply_lanes(const float* pose, const float* pos_Tc, const double* cov, int lanes, const int32_t* n_live /* host */,
                        int cap, float* pos_Tw, double* rot, double* cov_rot, mvStream_t stream);
/* mv_frontend_epilogue_lanes + mv_kp_select_lanes (MV_KP_NODEPTH) in one launch less: the selector's first kernel computes the
 * quality sigma_uu + sigma_vv from the network's covariance planes itself and writes the epilogue's maps for its own pixels.
 * Same results as the two calls in sequence, bit for bit (Frontend.py:183-200 + KeypointSelector.py:362-407).  Other
 * selector modes read the previous frame's maps too: MV_ERR_UNSUPPORTED. */
int mv_frontend_epilogue_select_lanes(const float* flow, const float* logcov, int cov_is_log, float bl_fx, float bl_fx_sq,
                                      float* disparity, float* disparity_cov, float* depth, float* depth_cov,
                                      uint8_t* bad_mask, float* match_flow, float* match_cov, const uint8_t* mask_a,
                                      const uint8_t* mask_b, const mvKpSelectParams* params /* host */, void* workspace,
                                      size_t workspace_bytes, int32_t* out_cand, int32_t* out_count, float* out_stats,
                                      int lanes, mvStream_t stream);
int mv_kp_gather_lanes(const int32_t* cand, size_t cand_lane_stride, const int64_t* perm /* [lanes, cap] */, int lanes,
                       const int32_t* n_live /* host */, int cap, int W, int64_t* out_uv /* [lanes, cap, 2] */,
                       mvStream_t stream);
/* mv_kp_gather_lanes + mv_kp_track_lanes + mv_backproject_lanes (camera frame, depth = the depth0 value the tracking gather
 * read) of a frame in ONE launch: same expressions, same bits (tests/test_gpu_backend.py::test_kp_front_equals_the_three_calls).
 * perm: device [lanes, cap] or — one lane, <= 256 rows — host: the indices then travel inside the kernel arguments (no copy). */
int mv_kp_front_lanes(const int32_t* cand, size_t cand_lane_stride, const int64_t* perm_dev, const int64_t* perm_host /* or NULL */,
                      int lanes, const int32_t* n_live /* host */, int cap, const float* match_flow, const float* match_cov,
                      const float* depth0, const float* disp0, const float* sdisp0, const float* sdd0, const float* depth1,
                      const float* disp1, const float* sdisp1, const float* sdd1, int H, int W, int edge, float match_cov_default,
                      float fx, float fy, float cx, float cy, int64_t* out_kp0_uv /* [lanes, cap, 2] */, float* out_kp0,
                      float* out_kp1, uint8_t* out_inbound, float* out_vals /* [11, lanes, cap] */, float* out_sigma0,
                      float* out_sigma1, float* out_pos_Tc /* [lanes, cap, 3] */, mvStream_t stream);
/* The pose-INDEPENDENT half of a frame's backend in one launch: mv_kp_front_lanes + mv_match_cov_pair_lanes (patch variance, no
 * rotation) — Odometry/MACVO.py:197-262, Module/Covariance/Project2to3.py:124-181 — with the same results bit for bit.  A wave = one keypoint of one of
 * the two keypoint sets.  cov_params: H, W, intrinsics, kernel size and clamps (use_patch_var must be 1).  The observation filters that follow are the
 * prologue of mv_pgo_solve_posed. */
int mv_backend_front_lanes(const int32_t* cand, size_t cand_lane_stride, const int64_t* perm_dev, const int64_t* perm_host, int lanes,
                           const int32_t* n_live, int cap, const float* match_flow, const float* match_cov, const float* depth0,
                           const float* disp0, const float* sdisp0, const float* sdd0, const float* depth1, const float* disp1,
                           const float* sdisp1, const float* sdd1, int edge, float match_cov_default, const mvMatchCovParams* cov_params,
                           int64_t* out_kp0_uv, float* out_kp0, float* out_kp1, uint8_t* out_inbound, float* out_vals, float* out_sigma0,
                           float* out_sigma1, float* out_pos_Tc, double* out_cov0, double* out_cov1, mvStream_t stream);
/* mv_backend_front_lanes of the device-driven frame (round 6): `selected_points[torch.randperm(n)[:numPoint]]` (Module/KeypointSelector.py:331,404) without
 * the host.  n = count_dev[l * count_stride] is read from device memory (where mv_kp_select_lanes left it: count_stride = 4), the permutation head is drawn
 * inside the launch from lane l's device-resident MT19937 state_in[l] (mv_mt19937_seed; same bits as torch's CPU generator + torch.randperm) and the advanced
 * generator is written to state_out[l] (a DIFFERENT buffer: every workgroup reads state_in).  out_perm [lanes, cap] int64 = the head, out_live [lanes, 2] =
 * {min(n, num_point), n}; rows beyond min(n, num_point) of the tables stay untouched.  num_point <= mv_randperm_max_head(). */
int mv_backend_front_draw_lanes(const int32_t* cand, size_t cand_lane_stride, const int32_t* count_dev, int count_stride, const uint32_t* state_in,
                                uint32_t* state_out, int num_point, int lanes, int cap, const float* match_flow, const float* match_cov,
                                const float* depth0, const float* disp0, const float* sdisp0, const float* sdd0, const float* depth1,
                                const float* disp1, const float* sdisp1, const float* sdd1, int edge, float match_cov_default,
                                const mvMatchCovParams* cov_params, int64_t* out_perm, int32_t* out_live, int64_t* out_kp0_uv, float* out_kp0,
                                float* out_kp1, uint8_t* out_inbound, float* out_vals, float* out_sigma0, float* out_sigma1, float* out_pos_Tc,
                                double* out_cov0, double* out_cov1, mvStream_t stream);
int mv_kp_track_lanes(const int64_t* kp0_uv, int lanes, const int32_t* n_live /* host */, int cap, const float* match_flow,
                      const float* match_cov, const float* depth0, const float* disp0, const float* sdisp0,
                      const float* sdd0, const float* depth1, const float* disp1, const float* sdisp1, const float* sdd1,
                      int H, int W, int edge, float match_cov_default, float* out_kp0, float* out_kp1,
                      uint8_t* out_inbound, float* out_vals /* [11, lanes, cap] */, float* out_sigma0, float* out_sigma1,
                      mvStream_t stream);
/* depth of lane l, row n = depth_vals[l * depth_lane_stride + n * depth_stride]; pose [lanes, 7]; rot [lanes, 9] */
int mv_backproject_lanes(const float* kp_uv, const float* depth_vals, int depth_stride, size_t depth_lane_stride, float fx,
                         float fy, float cx, float cy, const float* pose, int lanes, const int32_t* n_live /* host */,
                         int cap, float* pos_Tc, float* pos_Tw, double* rot, mvStream_t stream);
int mv_match_cov_pair_lanes(const float* depth_map0, const float* kp_uv0, float* flow_cov0, const double* rot0,
                            double* out_cov0, double* out_cov_rot0, const float* depth_map1, const float* kp_uv1,
                            float* flow_cov1, double* out_cov1, const mvMatchCovParams* params /* host */, int lanes,
                            const int32_t* n_live /* host */, int cap, mvStream_t stream);
/* vals = the [11, lanes, cap] table; valid [lanes, cap] (rows >= n_live[l] are written 0); count [lanes] */
int mv_obs_filter_lanes(const uint8_t* inbound, const double* cov1, const double* cov2, const float* vals, int flags,
                        float min_depth, float max_depth, int lanes, const int32_t* n_live /* host */, int cap,
                        uint8_t* valid, int32_t* count, mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * Native per-frame driver: the host-side sequencing of one `MACVO.run_pair` (Odometry/MACVO.py:173-311) and
 * `FlowFormerCovFrontend.estimate_pair` (Module/Frontend/Frontend.py:215-232) for the hot path, as two host calls per
 * frame instead of ~30 (a Python loop over the entry points above is interpreter-bound at ~370 us/frame, more than the
 * GPU work).  Internally: 4 HIP streams (volume GEMM | lookups+epilogue+selector | tracking..filter | LM solve),
 * rotating buffer slots carved out of ONE caller-provided device arena, events for every cross-stream hazard.
 *
 * Call order (frame 0 = MACVO.initialize :158-171, depth only):
 *     mv_frame_pipe_enqueue(p, &in0, s, 0);
 *     mv_frame_pipe_enqueue(p, &in1, s, 1);
 *     loop t = 1..: mv_frame_pipe_enqueue(p, &in[t+1], s, 1);          // next frame's frontend first (software pipeline)
 *                   mv_frame_pipe_enqueue_volume(p, &in[t+2], s);        // (optional) and the GEMM of the one after
 *                   mv_frame_pipe_wait_candidates(p, &n);                // host blocks on frame t's selector only
 *                   perm = torch.randperm(n)[:num_point]                 // stays on the host CPU: bit-exact indices
 *                   mv_frame_pipe_finish(p, perm, n_sel, pose_sink);     // backend + solve of frame t
 * At most three tracked frames may be in flight (enqueued, not finished): candidates x3, maps x5, volumes x3 rotate.
 *
 * Lanes (BASELINE configs[4], "batch-32 frames per GPU"): with pairs = 2 * lanes the pipe advances `lanes` INDEPENDENT
 * sequences in lock-step through the same launches — one volume GEMM of 2 * lanes pairs (pair 2l = lane l's stereo pair,
 * 2l + 1 its temporal pair, the batch axis of Frontend.py:219-220), lane-batched lookups / epilogue / selector / backend
 * kernels, and ONE mv_pgo_solve over `lanes` problems.  Every input of mvFrameInputs and every reported buffer then has
 * the leading dimension scaled by `lanes`; wait_candidates / finish / set_pose take per-lane arrays.
 */
typedef struct mvFramePipe mvFramePipe;

typedef struct {
    int32_t H, W;              /* image size: any with H % 8 != 1 and W % 8 != 1 (a pad of 7 stays refused) (mv_input_pad: the 1/8 maps below are h8 x w8 = ceil(H / 8) x ceil(W / 8), the network's centred pad; with
                                  flow8 / cov8 the pipe upsamples straight into the un-padded H x W window, mv_convex_upsample_crop) */
    int32_t C;                 /* feature channels (% 16 == 0) */
    int32_t pairs;             /* volume batch = 2 * lanes (<= 2 * MV_MAX_LANES): pair 2l stereo, 2l + 1 temporal of lane l */
    int32_t iters;             /* decoder iterations = window lookups per frame (12) */
    int32_t radius;            /* lookup radius (4) */
    int32_t feat_dtype;        /* MV_F32 | MV_F16 | MV_BF16 */
    int32_t layout;            /* MV_LAYOUT_* of the feature maps */
    int32_t volume_split;      /* MV_VOL_ENC16 (16): fp16 features, volume STORED in fp16 as the reference's Fast mode computes it
                                  (mv_corr_volume_out16 + mv_corr_lookup_vol16; shapes outside that kernel's domain keep fp32 cells) |
                                  0 exact fp32 | MV_PACK_F16X2 (6, the host side's default) | MV_PACK_BF16X3 (5): fp32 features of either
                                  layout packed on the device (mv_volume_pack, beside the previous frame's GEMM) +
                                  mv_corr_volume_packed, shapes it does not cover run the exact kernel | 3 | 2: fp32 HWC features through the round-1 plane split, multiplied
                                  as MV_BF16X3 / MV_BF16X2 */
    int32_t selector_mode;     /* MV_KP_NODEPTH | MV_KP_FULL | MV_KP_RANDOM | MV_KP_GRID | MV_KP_EXPLICIT (the last three enqueue no selector kernels, use
                                  kp_mask_width only, and size the per-keypoint tables by mv_frame_pipe_table_rows) */
    int32_t kp_kernel_size, kp_mask_width;
    int32_t num_point;         /* keypoints per frame (200) */
    int32_t edgewidth;         /* strict border of the tracked keypoints (32) */
    int32_t min_num_point;     /* fewer valid observations -> pose not optimised (MACVO.py:64,303-307) */
    int32_t graph_type;        /* MV_GRAPH_* */
    int32_t filters;           /* mv_obs_filter flags */
    int32_t cov_kernel_size;   /* 31 */
    int32_t mapping;           /* 1: dense-mapping tail of run_pair (Odometry/MACVO.py:313-337; `mapping: true`), lanes == 1 */
    int32_t map_num_point;     /* 2000 (:315) */
    int32_t map_mask_width;    /* MappingPointSelector args (Config/Experiment/MACVO/MACVO_Fast.yaml) */
    int32_t async_backend;     /* backend launch thread: the ~10 launches of `finish` (+ the permutation draw of finish_seeded) are issued by
                                  a second host thread while the caller's thread enqueues the next frame.  1 on, -1 off, 0 = environment
                                  MV_PIPE_ASYNC_BACKEND if set, else the library default.  Results are identical either way. */
    float fx, fy, cx, cy, baseline;
    float bl_fx, bl_fx_sq;     /* baseline*fx and its square, rounded once from double (StereoDepth.py:270-282) */
    float match_cov_default, max_match_cov, max_depth_cov, max_depth;
    float min_flow_cov_sq, min_depth_cov, filter_min_depth;
    float map_max_depth, map_max_depth_cov;   /* MappingPointSelector: z < map_max_depth, sigma_z^2 < map_max_depth_cov (KeypointSelector.py:87-100) */
    mvLMParams lm;
    int32_t cov_model;         /* MV_COV_* of all three covariance calls of a frame (both observation sets and the mapping tail); 0 = MatchCovariance */
    int32_t cov_modifiers;     /* modifier chain of mv_obs_cov; 0 = none */
    int32_t motion_model;      /* MV_MOTION_*: 0 = StaticMotionModel (the prior of a frame = the previous pose); 1 = TartanMotionNet: every tracked frame's
                                  PoseNet input is written to MV_FB_MOTION_IN right behind its epilogue, the caller runs the PoseNet and attaches its raw
                                  output with mv_frame_pipe_set_motion before the frame's finish; prior = previous pose @ Exp(raw * pose_norm) is the LM
                                  start, the pose of a frame without tracked keypoints and the frame's prior in mv_frame_pipe_map_append */
    int32_t frontend_nocov;    /* MV_NOCOV_* mask of the covariances the frontend does not provide; 0 = both there.  With a bit set the matching inputs
                                  (logcov / cov8 / cov_mask: NULL when both are) are not read, the covariance maps do not exist (mv_frame_pipe_buffer
                                  reports an error for them), the stored rows carry the reference's -1 placeholders (MACVO.py:253-263) and whatever would
                                  read a missing covariance is an invalid configuration: MV_NOCOV_DEPTH with MV_KP_FULL, mapping, MV_COV_GMM or
                                  MV_GRAPH_DISP; MV_NOCOV_MATCH with MV_KP_NODEPTH, MV_KP_FULL, MV_GRAPH_REPROJ or MV_GRAPH_DISP */
    float cov_match_cov_default;   /* MV_NOCOV_MATCH: the covariance model's own match_cov_default (Project2to3.py:133,216) — the sigma of the second
                                  observation; match_cov_default above stays the sigma of the first (MACVO.py:228) */
} mvFramePipeConfig;
enum { MV_MOTION_STATIC = 0, MV_MOTION_TARTAN = 1 };

/* what the learned layers hand over for one estimate_pair (device pointers, fp32 unless noted) */
typedef struct {
    const void* fmap1;      /* [pairs, C, h8, w8] (CHW) or [pairs, h8, w8, C] (HWC), feat_dtype; h8 x w8 = ceil(H / 8) x ceil(W / 8) */
    const void* fmap2;
    const float* coords;    /* [iters, pairs, 2, h8, w8]: coords1 entering each decoder iteration (covhead.py:85-92) */
    const float* flow;      /* [pairs, 2, H, W] last upsampled flow        } either these two (un-padded, as `inference` returns them) ... */
    const float* logcov;    /* [pairs, 2, H, W] last upsampled log-sigma   }  (logcov / cov8 / cov_mask: only the pairs  */
    const float* flow8;     /* [pairs, 2, h8, w8]   } ... or the 1/8-resolution fields + convex-upsampling */
    const float* cov8;      /* [pairs, 2, h8, w8]   }     masks of the last iteration (covhead.py:119-135); (whose covariance the   */
    const float* up_mask;   /* [pairs, 576, h8, w8] }     up_mask BEFORE its 0.25 scale, cov_mask after      */
    const float* cov_mask;  /* [pairs, 576, h8, w8] }   (frontend provides are read; NULL with both MV_NOCOV_* bits set)           */
} mvFrameInputs;

/* buffers reported by mv_frame_pipe_buffer (element counts, not bytes; MV_FB_VOLUME's element is the volume CELL: fp32, or fp16 — 2 bytes —
 * when the pipe was created with volume_split = MV_VOL_ENC16); each has a leading [lanes] dimension, per-keypoint
 * tables are [lanes, cap, .] with cap = mv_frame_pipe_table_rows(config) (= num_point except for MV_KP_GRID; a lane's live rows = its n_sel),
 * MV_FB_VALS is [11, lanes, cap] */
enum {
    MV_FB_VOLUME = 0, MV_FB_TOKENS, MV_FB_DISPARITY, MV_FB_DISPARITY_COV, MV_FB_DEPTH, MV_FB_DEPTH_COV, MV_FB_MATCH_FLOW,
    MV_FB_MATCH_COV, MV_FB_CAND, MV_FB_COUNT, MV_FB_STATS,                       /* frontend side: age counts enqueued frames */
    MV_FB_KP0, MV_FB_KP0F, MV_FB_KP1, MV_FB_INBOUND, MV_FB_VALS, MV_FB_SIGMA0, MV_FB_SIGMA1, MV_FB_POS_TC, MV_FB_POS_TW,
    MV_FB_ROT, MV_FB_COV0, MV_FB_COV0W, MV_FB_COV1, MV_FB_VALID, MV_FB_NVALID, MV_FB_POSE64, MV_FB_INFO,   /* backend side */
    MV_FB_POSE,                                                                  /* fp32 [lanes, 7]; age 0 = newest solve's output */
    /* dense-mapping tail of the newest finished frame (mapping = 1; rows = what mv_frame_pipe_map_points was called with) */
    MV_FB_MAP_UV, MV_FB_MAP_D, MV_FB_MAP_SDD, MV_FB_MAP_TC, MV_FB_MAP_TW, MV_FB_MAP_COV /* fp64 [.,9] */, MV_FB_MAP_COLOR /* u8 [.,3] */,
    /* device-driven frame (round 6): the permutation head the front launch drew, int64 [lanes, num_point]; int32 [lanes, 2] = selected keypoints, candidates */
    MV_FB_PERM, MV_FB_LIVE,
    /* motion_model = MV_MOTION_TARTAN: fp32 [lanes, 5, 112, 160] PoseNet input of an enqueued frame (age counts enqueued frames; valid on a stream after
     * mv_frame_pipe_wait_motion_input); fp32 [lanes, 7] motion-model prior of a finished frame (age 0 / 1) */
    MV_FB_MOTION_IN, MV_FB_PRIOR
};

size_t mv_frame_pipe_arena_bytes(const mvFramePipeConfig* cfg);           /* 0 = invalid configuration */
int mv_frame_pipe_max_pending(void);   /* how many tracked frames may be enqueued and not yet finished (the slot rotation this library was built with) */
/* how many tracked frames the host should keep in flight for this pipe shape (the stream layout the driver will pick for `lanes` sequences with / without
 * the dense-mapping tail): 3 for the two-decoder-stream layout of one- and two-lane pipes and for batched pipes, 2 for the classic one-lane layout */
int mv_frame_pipe_default_depth(int lanes, int mapping);
/* arena: device memory, 256-byte aligned, >= mv_frame_pipe_arena_bytes; must outlive the pipe */
int mv_frame_pipe_create(const mvFramePipeConfig* cfg, void* arena, size_t arena_bytes, mvFramePipe** out);
void mv_frame_pipe_destroy(mvFramePipe* p);
int mv_frame_pipe_set_pose(mvFramePipe* p, const float* pose7_host);      /* [lanes, 7] host: priors of the next frame (blocking) */
/* frontend half of a frame; inputs must be complete on `in_stream` (an event is recorded there) and stay untouched
 * until the frame's lookups ran.  with_selector = 0 for the very first frame. */
int mv_frame_pipe_enqueue(mvFramePipe* p, const mvFrameInputs* in, mvStream_t in_stream, int with_selector);
/* motion_model = MV_MOTION_TARTAN.  mv_frame_pipe_wait_motion_input: `stream` waits until the PoseNet input of the newest enqueued frame (MV_FB_MOTION_IN,
 * age 0) is written.  mv_frame_pipe_set_motion: attaches the raw PoseNet output [lanes, 6] fp32 (device, before pose_norm) to the newest enqueued tracked
 * frame: copied on `stream` into the pipe's slot for that frame's finish, with an event the frame's solve waits for; call it after the PoseNet's last read
 * of MV_FB_MOTION_IN (the slot is rewritten behind that event) and before the frame's finish. */
int mv_frame_pipe_wait_motion_input(mvFramePipe* p, mvStream_t stream);
int mv_frame_pipe_set_motion(mvFramePipe* p, const float* motion_dev, mvStream_t stream);
/* optional: issue the volume GEMM of the NEXT frame (the one the next mv_frame_pipe_enqueue will complete) right away; it
 * only needs fmap1 / fmap2 and a free volume buffer, so the host can queue it before it blocks on the previous frame's
 * candidate count and the GEMM stream never waits for the host.  At most one GEMM ahead. */
int mv_frame_pipe_enqueue_volume(mvFramePipe* p, const mvFrameInputs* in, mvStream_t in_stream);
int mv_frame_pipe_wait_candidates(mvFramePipe* p, int32_t* n_cand /* [lanes] host */);   /* oldest unfinished frame; blocks the host */
/* perm_host: int64 [lanes, num_point], row l = randperm(n_cand[l])[:num_point] (n_sel[l] entries used); n_sel: int32 [lanes]
 * host; pose_sink: device fp32 [lanes, 7] or NULL (copy of the new poses) */
int mv_frame_pipe_finish(mvFramePipe* p, const int64_t* perm_host, const int32_t* n_sel, float* pose_sink);
/* Native keypoint permutations.  The reference draws `torch.randperm(n)[:numPoint]` from torch's CPU generator
 * (Module/KeypointSelector.py:331,404) = MT19937 + Fisher-Yates (ATen randperm_cpu).  mv_frame_pipe_seed_lanes gives every lane
 * its own MT19937 seeded like `torch.Generator().manual_seed(seed)`; mv_frame_pipe_finish_seeded then replaces
 * wait_candidates + host randperm + finish by one call (first numPoint swaps, the remaining draws discarded: same bits, ~20x
 * less host time — what a 32-lane step needs).  n_cand_out / n_sel_out: [lanes] host or NULL. */
/* Dense-mapping tail (config.mapping = 1, lanes == 1; Odometry/MACVO.py:303-337).  The reference maps only when tracking
 * succeeded and then draws its SECOND randperm of the frame, so the host has to see the frame's observation count first:
 *   mv_frame_pipe_wait_tracked   blocks until the newest finished frame's filter count is on the host; returns it and the number
 *                                of MappingPointSelector candidates (found on the PREVIOUS frame's depth maps, on the decoder-side
 *                                stream next to the tracking selector);
 *   mv_frame_pipe_map_points     perm_host = randperm(n_cand_map)[:map_num_point]: gather, depth / variance gathers,
 *                                pixel2point_NED, prev_pose.Act, constant match sigma, colours (image_dev [3,H,W] fp32 in [0,1] or
 *                                NULL), the 31x31 covariance model (stored unrotated, :324) — into the MV_FB_MAP_* buffers — and,
 *                                with `stores`, map_points.push + frame2map.add (mv_map_append_points) behind this frame's
 *                                mv_frame_pipe_map_append.  Call order per frame: finish, [map_append], wait_tracked, [map_points]. */
int mv_frame_pipe_wait_tracked(mvFramePipe* p, int32_t* n_valid, int32_t* n_cand_map);
int mv_frame_pipe_map_points(mvFramePipe* p, const int64_t* perm_host, int n_sel, const float* image_dev,
                             const mvMapStores* stores /* host, or NULL */);
int mv_frame_pipe_seed_lanes(mvFramePipe* p, const uint64_t* seeds /* [lanes] host */);
/* host-only (no GPU): `calls` successive torch.randperm(n[i], generator=g)[:k] of ONE generator g = torch.Generator().manual_seed(seed),
 * as the seeded finish draws them for a lane (Module/KeypointSelector.py:331,404); out [calls, k] (row i: min(k, n[i]) entries) */
int mv_randperm_heads(uint64_t seed, const int64_t* n, int calls, int k, int64_t* out);
int mv_frame_pipe_finish_seeded(mvFramePipe* p, float* pose_sink, int32_t* n_cand_out, int32_t* n_sel_out);
/* Device-resident permutations (round 6).  The same draw — torch.randperm(n)[:k] of an MT19937 seeded like torch.Generator().manual_seed(seed),
 * Module/KeypointSelector.py:331,404 — made ON THE GPU from a candidate count that never leaves it: no D2H count, no host generator, no H2D permutation.
 * A lane's generator lives in device memory as mv_randperm_state_words() uint32 words (the 624-word block + the position of the next draw);
 *   mv_mt19937_seed            fills that representation on the host (copy it to the device);
 *   mv_randperm_head_lanes     one workgroup per lane: n = n_dev[l * n_stride]; writes out_perm[l * cap + (0 .. min(n, k)))  and
 *                              out_n_sel[l * n_sel_stride] = min(n, k); advances the lane's generator by max(n - 1, 0) draws (k <= mv_randperm_max_head());
 *   mv_randperm_heads_emulated host-only (no GPU): the same phase functions (csrc/randperm_dev.h) run thread by thread with `threads` emulated
 *                              threads — `calls` successive draws of one generator, out [calls, k] like mv_randperm_heads. */
int mv_randperm_state_words(void);
int mv_randperm_max_head(void);
int mv_mt19937_seed(uint64_t seed, uint32_t* state_host);
int mv_randperm_head_lanes(uint32_t* state, const int32_t* n_dev, int n_stride, int lanes, int k, int cap, int64_t* out_perm, int32_t* out_n_sel,
                           int n_sel_stride, mvStream_t stream);
int mv_randperm_heads_emulated(uint64_t seed, const int64_t* n, int calls, int k, int threads, int64_t* out);
/* The device-driven frame.  mv_frame_pipe_seed_lanes also places the generators in device memory and — unless MV_PIPE_DEVICE_DRAW=0, the dense-mapping tail is on or
 * num_point > mv_randperm_max_head() — switches the pipe to it (mv_frame_pipe_device_draw() == 1): a frame is then finished with mv_frame_pipe_finish_device,
 * which never waits: backend + solve are queued behind the frame's selector by event and the front launch (mv_backend_front_draw_lanes) draws the permutation
 * itself.  Same keypoints, same poses as mv_frame_pipe_finish_seeded.  mv_frame_pipe_finished_counts: the counts of the age-th newest finished frame
 * (0 or 1), for whoever needs them on the host (blocks until that frame's front launch has run). */
int mv_frame_pipe_device_draw(const mvFramePipe* p);
/* 1 when the pipe's volume buffers (the VOLUME view) hold every query's slice in 4 x 4-cell tiles (mv_corr_lookup_tiled / _tiled_vol16 read them):
 * Fast-mode pipes by default, split-precision pipes under MV_PIPE_TILED=1 */
int mv_frame_pipe_volume_tiled(const mvFramePipe* p);
int mv_frame_pipe_host_threads(const mvFramePipe* p);   /* 1: the caller issues everything; 2: + the backend launch thread (default where the process has >= 3 cores) */
int mv_frame_pipe_finish_device(mvFramePipe* p, float* pose_sink);
/* ---- RandomSelector, GridSelector and caller-supplied keypoints (ABI 8) -------------------------------------------------------------------------------
 * RandomSelector.select_point is `h = torch.randint(mask, H - mask, (k, 1)); w = torch.randint(mask, W - mask, (k, 1)); cat([w, h], 1)`.  On torch's CPU
 * generator (the generator the permutations above reproduce) that is one MT19937 word per element, `word % (high - low) + low`: a call advances the generator
 * by exactly 2 k words — the k rows' v, then their u — and a following torch.randperm continues in the same stream.  Duplicate rows are possible and kept.
 *   mv_kp_random_lanes     one workgroup per lane draws from the lane's device-resident generator (mv_mt19937_seed representation, `state` [lanes,
 *                          mv_randperm_state_words()], advanced in place) -> out_uv int64 [lanes, num_point, 2] (u, v); num_point <= mv_kp_random_max_point()
 *   mv_kp_random_emulated  host-only (no GPU): the same phase functions (csrc/kp_draw_dev.h) run with `threads` emulated threads; `calls` successive calls
 *                          of one generator seeded with `seed`, out [calls, num_point, 2]
 *   mv_kp_random_heads     host-only twin on the host's MT19937 (what mv_frame_pipe_finish_seeded draws for a lane of a MV_KP_RANDOM pipe); same layout
 * All three need H > 2 * mask_width and W > 2 * mask_width.
 * GridSelector is closed-form; it may return MORE rows than num_point (640 x 480, mask 32, 200 -> 11 x 21 = 231).  mv_kp_grid_count: the row count, 0 for the
 * shapes where the reference raises (a grid step of 0) or the masked image is empty; mv_kp_grid writes out_uv int64 [count, 2]. */
int mv_kp_random_max_point(void);
int mv_kp_random_lanes(uint32_t* state, int lanes, int num_point, int H, int W, int mask_width, int64_t* out_uv, mvStream_t stream);
int mv_kp_random_emulated(uint64_t seed, int calls, int num_point, int H, int W, int mask_width, int threads, int64_t* out);
/* mv_kp_random_emulated followed by ONE emulated torch.randperm(perm_n)[:perm_k] of the same generator (out_perm [perm_k], min(perm_n, perm_k) entries) */
int mv_kp_random_then_randperm_emulated(uint64_t seed, int calls, int num_point, int H, int W, int mask_width, int threads, int64_t* out, int64_t perm_n,
                                        int perm_k, int64_t* out_perm);
int mv_kp_random_heads(uint64_t seed, int calls, int num_point, int H, int W, int mask_width, int64_t* out);
int mv_kp_grid_count(int H, int W, int mask_width, int num_point);
int mv_kp_grid(int H, int W, int mask_width, int num_point, int64_t* out_uv, mvStream_t stream);
/* ---- GradientSelector and SparseGradienSelector: the image-gradient selectors (Module/KeypointSelector.py:121-158, :161-213) ---------------------------
 *   grad = |conv2d(imageL[0] [3, H, W], Laplacian [[0,1,0],[1,-4,1],[0,1,0]] over the three channels, padding = 1)|   (:129-135 — the zero padding makes the
 *          border pixels large; that is the reference and is kept)
 *   thr  = grad.mean() + grad_std * grad.std()  (unbiased), candidates = grad > thr (strict) inside the border mask [m:-m, m:-m] (:136-147) and — nms_size
 *          given — where grad == max_pool2d(grad, nms_size, stride 1, padding nms_size / 2): -inf padding, every tied maximum survives (:192-199)
 *   in torch.nonzero's row-major order (:147, :201).  mask_width = 0 is the empty slice 0:-0 and 2 * mask_width >= H or W an empty mask: zero candidates,
 *   no error.  A NaN pixel makes thr NaN: zero candidates.
 * Arithmetic (csrc/kp_grad_math.h, replayed on the host by tests/c_abi/kp_grad_twin.cpp): per channel ((up + down) + (left + right)) - 4 c in fp32, channels
 * added in order, fabsf; mean and std from fp64 sums of g and g^2 in a fixed order (per 64 x 16 tile, then the tiles in ascending index — no floating-point
 * atomics), var = (S2 - n mean^2) / (n - 1) in fp64, mean and sqrt(var) rounded to fp32 once, thr = mean + (float)grad_std * std in fp32.  A lane's bits are
 * the same from run to run, alone or batched.  On images whose values are multiples of 1 / 256 every step is exact and the candidates are those of torch.
 *   image      [lanes, 3, H, W] fp32 planar
 *   params     nms_size 0: GradientSelector; odd 1 .. 15: SparseGradienSelector (1 = the window is the pixel itself); an even or negative one, grad_std <= 0,
 *              non-positive sizes, null pointers: MV_ERR_INVALID_ARG; an odd one above 15: MV_ERR_UNSUPPORTED; all checked before anything is launched
 *   workspace  lanes * mv_kp_gradient_workspace_bytes(H, W) bytes, 8-byte aligned, no initial content required (MV_ERR_WORKSPACE when smaller)
 *   out_cand   [lanes, H * W] int32 v * W + u, out_count [lanes, 4] int32 {n_candidates, n_above_threshold (inside the border, before the NMS), 0, 0}:
 *              the layout of mv_kp_select_lanes, so mv_kp_gather(_lanes) applies;  out_stats [lanes, 4] fp32 {mean, std, thr, 0}
 * mv_kp_finish_device_lanes: `selected[torch.randperm(n)[:k]]` rolled to (u, v) (:150-151, :204-205) without the host.  One workgroup per lane reads
 * n = count_dev[l * count_stride], draws the permutation head from the lane's device-resident generator (mv_mt19937_seed representation, advanced in place
 * by max(n - 1, 0) draws, as mv_randperm_head_lanes does), gathers the rows from cand + l * cand_lane_stride and writes out_uv int64 [lanes, cap, 2] — rows at
 * or past min(n, k) are zero — and out_n_sel[l] = min(n, k).  k <= cap; k > mv_randperm_max_head(): MV_ERR_UNSUPPORTED.  Works on any candidate list of the
 * mv_kp_select layout. */
typedef struct {
    int32_t H, W;
    int32_t mask_width;    /* border exclusion in pixels; 0 selects nothing (the reference's empty slice) */
    int32_t nms_size;      /* 0: GradientSelector; odd 1 .. 15: SparseGradienSelector */
    float grad_std;        /* > 0 */
} mvKpGradParams;
size_t mv_kp_gradient_workspace_bytes(int H, int W);
int mv_kp_gradient_lanes(const float* image, const mvKpGradParams* params /* host */, void* workspace, size_t workspace_bytes, int32_t* out_cand,
                         int32_t* out_count, float* out_stats, int lanes, mvStream_t stream);
int mv_kp_finish_device_lanes(uint32_t* state, const int32_t* cand, size_t cand_lane_stride, const int32_t* count_dev, int count_stride, int lanes, int k,
                              int cap, int W, int64_t* out_uv, int32_t* out_n_sel, mvStream_t stream);
/* Frame pipe.  Rows of capacity per lane of every per-keypoint table (0: invalid configuration): max(num_point, grid count) for MV_KP_GRID, num_point otherwise.
 * A configuration is rejected when H <= 2 * kp_mask_width or W <= 2 * kp_mask_width (new modes), when the grid has a step of 0, when the capacity exceeds
 * MV_KP_TABLE_MAX (the observation filter and the solve walk a lane's rows with one 256-thread workgroup: "a few thousand" is what they are built and tested
 * for), when MV_KP_RANDOM asks for more than mv_kp_random_max_point() rows (the 1024-word draw buffer of the front launch), and — new modes with cov_model
 * MATCH / GMM — when kp_mask_width < cov_kernel_size / 2: the covariance patch of a keypoint closer to the border than that leaves the image, where the
 * reference wraps or raises and the kernel clamps.
 * With the three new modes a frame enqueues no selector kernel, no candidate list and no count copy; mv_frame_pipe_wait_candidates reports the row count.
 *   MV_KP_RANDOM  mv_frame_pipe_seed_lanes + mv_frame_pipe_finish_device (drawn inside the front launch) or mv_frame_pipe_finish_seeded (host draw): same bits
 *   MV_KP_GRID    either of the two (nothing is drawn)
 * mv_frame_pipe_finish_keypoints: the frame's keypoints as int64 (u, v) rows, kp_uv_host [lanes, cap, 2] with n_sel[l] <= cap live rows per lane.  Valid for
 * EVERY selector_mode (on a CovAware pipe it bypasses the candidate list; the generators of mv_frame_pipe_seed_lanes do not move).  Every row must lie inside
 * the image and — cov_model MATCH / GMM — at least cov_kernel_size / 2 from its border: checked here, MV_ERR_INVALID_ARG otherwise.
 * mv_frame_pipe_finish_keypoints_dev: the same from device memory (kp_uv_dev as above, n_sel_dev int32 [lanes], clamped to [0, cap]), read on the pipe's
 * streams behind everything enqueued on `stream` so far; never waits for the host.  PRECONDITION (not checked): rows as above.  A row outside the image is
 * marked out of bounds and a patch that leaves the image is clamped — nothing is read outside the maps — but such a frame no longer follows the reference.
 * Needs the two-launch backend (the default) and no dense-mapping tail.  The caller may reuse both arrays once `stream` has passed mv_frame_pipe_sync(p, stream, 2).
 * The host learns such a frame's live-row counts only if it asks: mv_frame_pipe_finished_counts reads them back (n_cand = n_sel = the clamped count), on any pipe. */
#define MV_KP_TABLE_MAX 4096
int mv_frame_pipe_table_rows(const mvFramePipeConfig* cfg);
int mv_frame_pipe_finish_keypoints(mvFramePipe* p, const int64_t* kp_uv_host, const int32_t* n_sel, float* pose_sink);
int mv_frame_pipe_finish_keypoints_dev(mvFramePipe* p, const int64_t* kp_uv_dev, const int32_t* n_sel_dev, mvStream_t stream, float* pose_sink);
int mv_frame_pipe_finished_counts(mvFramePipe* p, int age, int32_t* n_cand, int32_t* n_sel);
/* host-side flow control of a device-driven stream: blocks until the front launch of the finish `lag` finishes back (0 = the newest; lag <= 6) has run */
int mv_frame_pipe_wait_finished(mvFramePipe* p, int lag);
/* register the newest FINISHED frame in a device-resident map (mv_map_append on the pipe's own streams, no copies; lanes = 1):
 * frame_idx = the map index the frame receives (= frames pushed so far), prev_frame = the previous keyframe's index; the
 * optimised pose is written over the frame's prior once its solve has finished.  The host-descriptor form (and the one that takes
 * colours) of the one registration protocol described at mv_frame_pipe_map_append_lanes: same waits, same events. */
int mv_frame_pipe_map_append(mvFramePipe* p, const mvMapStores* stores /* host */, int frame_idx, int prev_frame,
                             const float* K_dev, const float* T_BS_dev, float baseline, int64_t time_ns,
                             const uint8_t* color_dev /* [n_sel,3] or NULL */);
/* The frame the pipe's LM solve runs in (Module/Optimization/TwoFramePGO/Optimizer.py:111-150).  MV_SOLVE_LOCAL: every finish solves in the frame of
 * ref_pose = pose[frame_idx - 1] (mv_pgo_solve_posed_local*) — the previous keyframe's current pose, which is what the rows are registered with, or, when
 * mv_frame_pipe_skip was called since the previous finish, the pose that keyframe was pushed with (its prior: MV_FB_PRIOR under MV_MOTION_TARTAN).  Call
 * before the first enqueue; any lane count.  A pipe on which none of the three calls below is made issues exactly the launches it issued before. */
enum { MV_SOLVE_WORLD = 0, MV_SOLVE_LOCAL = 1 };
int mv_frame_pipe_set_solve_frame(mvFramePipe* p, int solve_frame);
/* A non-keyframe passes (Odometry/MACVO.py:177-179): nothing of it is computed.  The pipe notes that the row in front of the next finished frame is a
 * skipped one, holding the previous keyframe's prior (its optimised pose is not written back before the next run_pair, :187). */
int mv_frame_pipe_skip(mvFramePipe* p);
/* ... and its row in the device-resident map (mv_map_append_skipped; lanes = 1): the pose is copied ON THE DEVICE from the previous keyframe's prior slot,
 * on the stream that carries the pipe's own mv_frame_pipe_map_append (row indices come from the device-side counter), without any host wait.
 * frame_idx = the map index the row receives (= frames pushed so far). */
int mv_frame_pipe_map_skip(mvFramePipe* p, const mvMapStores* stores /* host */, int frame_idx, const float* K_dev, const float* T_BS_dev,
                           float baseline, int64_t time_ns);
/* Registration for a pipe of ANY lane count (lanes >= 1), every lane into its own map (Scripts/Experiment/Experiment_MACVO.py:55-58 keeps one VisualMap
 * per sequence; per lane Odometry/MACVO.py:244-311,339-347 and :177-179): ONE mv_map_append_lanes / mv_map_append_skipped_lanes launch on the backend stream
 * behind the finish's e_solved / e_posed, then ONE mv_map_set_pose_lanes launch on the solve stream behind it (Optimizer.py:104-108).  stores_dev: DEVICE
 * mvMapStores[lanes]; T_BS_dev: [lanes, 7]; time_ns: HOST [lanes]; frame_idx / prev_frame are the same for every lane (lock-step).  Same call positions as the
 * one-lane forms.  There is ONE protocol: the two one-lane calls above run it with a host descriptor, mv_map_append / mv_map_append_skipped and a pose copy
 * in place of the lanes launches.  Either append records the event that guards its backend slot (one per slot, where front launches run on a decoder-side
 * stream): the front launch of the finish two later waits for it before it rewrites the tables the append read.  A pipe that never makes these calls issues
 * exactly the launches and waits it issued before. */
int mv_frame_pipe_map_append_lanes(mvFramePipe* p, const mvMapStores* stores_dev /* DEVICE [lanes] */, int frame_idx, int prev_frame, const float* K_dev,
                                   const float* T_BS_dev, float baseline, const int64_t* time_ns /* host [lanes] */);
int mv_frame_pipe_map_skip_lanes(mvFramePipe* p, const mvMapStores* stores_dev /* DEVICE [lanes] */, int frame_idx, const float* K_dev, const float* T_BS_dev,
                                 float baseline, const int64_t* time_ns /* host [lanes] */);
/* Result views and slot reuse: a consumer that reads result views (mv_frame_pipe_buffer) asynchronously on its own stream
 * calls this before it finishes the next frame; the pipe then orders the kernels that recycle those buffers behind
 * everything enqueued on `stream` so far.  (Host-synchronous consumers do not need it.) */
int mv_frame_pipe_release(mvFramePipe* p, mvStream_t stream);
/* block_host = 1: wait for all four streams on the host; 0: make `stream` wait for everything enqueued so far (including the
 * frontends of frames enqueued ahead); 2: make `stream` wait for the newest FINISHED frame's backend + solve only — what a
 * consumer of that frame's results needs while later frames are already queued */
int mv_frame_pipe_sync(mvFramePipe* p, mvStream_t stream, int block_host);
/* measurement hook (bench.py roofline): record a HIP-event pair around each of the next max_launches volume GEMMs on the
 * stream they run on (0 = off; restarts the count), and read the elapsed milliseconds back (blocks on that stream) */
int mv_frame_pipe_time_volume(mvFramePipe* p, int max_launches);
int mv_frame_pipe_volume_times(mvFramePipe* p, float* ms, int cap, int* n);
/* start of each timed GEMM, ms since the first timed one (same events) */
int mv_frame_pipe_volume_starts(mvFramePipe* p, float* ms, int cap, int* n);
/* on = 0: a timed frame records ONLY the event pair around its volume GEMM (what the roofline needs), not the six timeline events on the other three
 * streams — each is a barrier packet on a stream whose launch chain bounds a one-lane pipe; mv_frame_pipe_timeline[_backend] then report no frames.
 * Default 1.  bench.py times the contract's K steps with 0 and collects the timeline in a separate untimed pass. */
int mv_frame_pipe_time_detail(mvFramePipe* p, int on);
/* per timed frame: {GEMM start, GEMM end, last lookup done, selector done} in ms since the first timed GEMM start */
int mv_frame_pipe_timeline(mvFramePipe* p, float* ms, int cap_frames, int* n);
/* ... and {backend start, backend end, pose_apply start, solve end} of the same frames (-1: not finished / no keypoints) */
int mv_frame_pipe_timeline_backend(mvFramePipe* p, float* ms, int cap_frames, int* n);
/* where a result lives inside the arena; age 0 = newest frame that passed that stage, 1 = the one before */
int mv_frame_pipe_buffer(mvFramePipe* p, int which, int age, void** ptr, size_t* count);

/* ---- Frontend evaluation (Evaluation/EvalFlow.py, Evaluation/EvalDepth.py): one lane = one frame (B = 1, as every caller of the reference assumes),
 * lanes <= MV_MAX_LANES, any H, W >= 1 with H * W <= 2^22 (torch's fp32 quantile position q * (n - 1) is exact up to there; MV_ERR_INVALID_ARG beyond).
 * All launches go on `stream`; nothing synchronises with the host.  One fp32 row per lane is written to rows[lane][row_index][COLS] of a caller-owned
 * device table rows[lanes][rows_per_lane][COLS]; no other row is touched, so a pass over a sequence fills a table that is read back once.  Means are
 * fp64 sums of the fp32 per-pixel terms, reduced in an order that depends on (H, W) only, over the non-NaN terms (nanmean); an empty population gives a
 * NaN mean and a zero count (the reference raises there and skips the frame, EvalDepth.py:28-37).  Counts are exact integers stored as fp32.
 * Quantiles follow torch.nanquantile bit for bit: n non-NaN values, r = fp32(q) * fp32(n - 1), a = v[floor r], b = v[ceil r], w = r - floor r, d = b - a,
 * w < 0.5 ? a + w * d : b - d * (1 - w) (two +inf order statistics give NaN); the order statistics come from an exact radix select (-0.0 and +0.0 are equal
 * values, either may be returned).  workspace: mv_eval_workspace_bytes(lanes, H, W) bytes, 16-byte aligned, private to the call until it has finished
 * (0 = unsupported arguments). */
size_t mv_eval_workspace_bytes(int lanes, int H, int W);
/* EvalFlow.py:29-47 (evaluate_flow) and :82-127 (evaluate_flowcov).  Per pixel: eu = est_u - gt_u, ev = est_v - gt_v, epe = sqrtf(eu * eu + ev * ev);
 * mask = [apply_max_flow: est_u < max_flow && est_v < max_flow (signed, NaN compares false, :36-37)] && [valid: valid != 0].  apply_max_flow is off when
 * the caller passes the ground-truth mask (:32-34).  N_MASK = |mask|, N_MASK_FINITE = non-NaN epe inside it, N_FINITE = non-NaN epe of the lane;
 * MASKED_EPE = nanmean(epe[mask]), EPE = nanmean(epe), PXk = mean over the mask of (epe < k): a NaN epe inside the mask is a miss there.
 * est_cov (or NULL): planes sigma_uu and sigma_vv, cov_plane_stride floats apart (a third plane is ignored, as est_cov[:, :2] does, :78).  Then
 * det = cu * cv (= torch.det of the diagonal 2 x 2), pinv(c) = |c| > 1e-15f * max(|cu|, |cv|) ? 1 / c : 0 (Tensor.pinverse's rcond),
 * m = (eu * pinv(cu)) * eu + (ev * pinv(cv)) * ev, nll = logf(det) + square(sqrtf(m)) (:101, Utility/Math.py:146), uncertainty = det (:107);
 * T25 / T50 / T75 = nanquantile(uncertainty) over ALL pixels of the lane (:108-110); MASKED_NLL = nanmean(nll[mask]) over N_MASK_NLL terms,
 * Qxx_NLL = nanmean(nll[uncertainty < Txx]) (strict; the mask is not intersected, :115-117), N_Qxx = |uncertainty < Txx|.  The reference's own SVD raises
 * on a non-finite covariance; here a NaN covariance gives a NaN nll, which the means drop — that case is ours and is not pinned by the reference.
 * Without est_cov the NLL and threshold columns are NaN and N_Q* are 0.
 * grids (or NULL; needs est_cov): uint32 [lanes][2][100][100], (eu^2, cu) and (ev^2, cv) over ALL pixels (:120-127, GridRecorder.py:24-36): bin =
 * (int)(v * 4.0f) truncated toward zero, a pixel counts when both bins are in [0, 100); NaN and +-inf are not counted.  The grids ACCUMULATE (+=): the
 * caller zeroes them once per sequence.  epe_out / nll_out (or NULL): the per-pixel planes [lanes][H * W] (nll_out is written only with est_cov). */
enum {
    MV_EVAL_FLOW_MASKED_EPE = 0, MV_EVAL_FLOW_EPE, MV_EVAL_FLOW_PX1, MV_EVAL_FLOW_PX3, MV_EVAL_FLOW_PX5, MV_EVAL_FLOW_MASKED_NLL,
    MV_EVAL_FLOW_Q25_NLL, MV_EVAL_FLOW_Q50_NLL, MV_EVAL_FLOW_Q75_NLL, MV_EVAL_FLOW_T25, MV_EVAL_FLOW_T50, MV_EVAL_FLOW_T75,
    MV_EVAL_FLOW_N_MASK, MV_EVAL_FLOW_N_MASK_FINITE, MV_EVAL_FLOW_N_FINITE, MV_EVAL_FLOW_N_Q25, MV_EVAL_FLOW_N_Q50, MV_EVAL_FLOW_N_Q75,
    MV_EVAL_FLOW_N_MASK_NLL, MV_EVAL_FLOW_COLS
};
int mv_eval_flow_lanes(int lanes, int H, int W, const float* est_flow /* [2,H,W] per lane */, int64_t est_lane_stride,
                       const float* gt_flow /* [2,H,W] per lane */, int64_t gt_lane_stride, const float* est_cov /* or NULL */,
                       int64_t cov_plane_stride, int64_t cov_lane_stride, const uint8_t* valid /* [H,W] per lane or NULL */, int64_t valid_lane_stride,
                       float max_flow, int apply_max_flow, float* rows, int rows_per_lane, int row_index, uint32_t* grids /* or NULL */,
                       float* epe_out /* or NULL */, float* nll_out /* or NULL */, void* workspace, size_t workspace_bytes, mvStream_t stream);
/* EvalDepth.py:22-34 (evaluate_depth) and :57-82 (evaluate_depthcov).  err = |est - gt|, mask = est < max_depth; MASKED_ERR = nanmean(err[mask]),
 * ERR_25 / ERR_75 = nanquantile(err[mask]), ERR_50 = nanmedian(err[mask]) = the lower middle element, not the interpolated quantile.  est_cov [H,W]
 * (or NULL): e = est - gt, pinv(c) = c != 0 ? 1 / c : 0, nll = logf(c) + square(sqrtf((e * pinv(c)) * e)), uncertainty = c; thresholds, means and
 * counts as for flow.  grid (or NULL; needs est_cov): uint32 [lanes][100][100] of (e^2, c) with bin = (int)(v * 2.0f) (0 ... 50 in steps of 0.5),
 * accumulating.  err_out / nll_out as above. */
enum {
    MV_EVAL_DEPTH_MASKED_ERR = 0, MV_EVAL_DEPTH_ERR_25, MV_EVAL_DEPTH_ERR_50, MV_EVAL_DEPTH_ERR_75, MV_EVAL_DEPTH_MASKED_NLL,
    MV_EVAL_DEPTH_Q25_NLL, MV_EVAL_DEPTH_Q50_NLL, MV_EVAL_DEPTH_Q75_NLL, MV_EVAL_DEPTH_T25, MV_EVAL_DEPTH_T50, MV_EVAL_DEPTH_T75,
    MV_EVAL_DEPTH_N_MASK, MV_EVAL_DEPTH_N_MASK_FINITE, MV_EVAL_DEPTH_N_FINITE, MV_EVAL_DEPTH_N_Q25, MV_EVAL_DEPTH_N_Q50, MV_EVAL_DEPTH_N_Q75,
    MV_EVAL_DEPTH_N_MASK_NLL, MV_EVAL_DEPTH_COLS
};
int mv_eval_depth_lanes(int lanes, int H, int W, const float* est_depth /* [H,W] per lane */, int64_t est_lane_stride,
                        const float* gt_depth /* [H,W] per lane */, int64_t gt_lane_stride, const float* est_cov /* [H,W] per lane or NULL */,
                        int64_t cov_lane_stride, float max_depth, float* rows, int rows_per_lane, int row_index, uint32_t* grid /* or NULL */,
                        float* err_out /* or NULL */, float* nll_out /* or NULL */, void* workspace, size_t workspace_bytes, mvStream_t stream);

/* ---- Trajectory evaluation (Evaluation/MetricsSeq.py:9-51: evaluateRTE / evaluateATE / evaluateROE / evaluateRPE, and the statistics
 * Evaluation/EvalSeq.py:53-64 reads from their results): ATE, RTE, ROE, RPE of `lanes` finished tracks in ONE launch, one workgroup per lane, on `stream`;
 * nothing synchronises with the host and nothing is staged.  MetricsSeq.py hands the work to evo 1.x, which is not a vendored dependency: its published
 * definition is RESTATED here, UNPINNED (no evo run stands behind these numbers; SURVEY A21 treats PyPose the same way).  All arithmetic is fp64.
 *   Tracks: est[l] / ref[l] are DEVICE pointers held in HOST arrays [lanes] (they travel by value in the kernel argument, so every lane may read its own
 * allocation in place: a DeviceVisualMap's pose table, mv_body_poses' output); T[l] rows (tx ty tz qx qy qz qw) on both sides — the tracks are already
 * time-associated, one estimate row per reference row (Trajectory.from_sandbox's align_time / interpolate_pose is not part of this) —, est_row_stride /
 * ref_row_stride elements (>= 7) between rows, est_dtype / ref_dtype MV_TRAJ_F32 or MV_TRAJ_F64.  lanes <= MV_MAX_LANES, 0 <= T[l] <= MV_EVAL_TRAJ_MAX_POSES;
 * MV_ERR_INVALID_ARG otherwise.
 *   Pose -> matrix as evo's quaternion_matrix: q is normalised; q.q < 4 DBL_EPSILON gives the identity; q and -q are the same rotation.
 *   Alignment (MetricsSeq.py passes align=True, align_origin=True to all four; in evo `align` wins and align_origin is then ignored):
 * MV_TRAJ_ALIGN_UMEYAMA: x = estimate, y = reference positions, n = T, C = (1/n) sum (y - mu_y)(x - mu_x)^T, sigma_x = (1/n) sum |x - mu_x|^2 (both centred
 * before they are summed), C = U diag(d) V^T by one-sided Jacobi on C itself, S = diag(1, 1, det U det V^T < 0 ? -1 : 1), R = U S V^T,
 * c = correct_scale ? trace(diag(d) S) / sigma_x : 1, t = mu_y - c R mu_x; the estimate's translations are multiplied by c, then every pose is left-multiplied
 * by [R | t].  Fewer than two d_k above DBL_EPSILON (absolute, as evo writes it) is DEGENERATE: evo raises there and EvalSeq.py:66-68 emits a row of None.
 * MV_TRAJ_ALIGN_ORIGIN: the estimate is left-multiplied by Q_0 P_0^-1 (evo's align_origin branch); MV_TRAJ_ALIGN_NONE: nothing.  With correct_scale these two
 * scale the estimate's translations by Umeyama's c first (evo's only_scale) and take over its degenerate rule; without it they never are DEGENERATE, the
 * covariance pass and the SVD are skipped and d_1..d_3 are NaN.
 * (evo itself skips the origin step when it corrects the scale; its fp32 round trip through Trajectory.align_origin is not reproduced either.)
 *   ATE (ape, translation_part): e_i = |trans(P_i) - trans(Q_i)|, T values.  RTE / ROE / RPE (rpe, delta = 1 frame): E_i = (Q_i^-1 Q_i+1)^-1 (P_i^-1 P_i+1),
 * T - 1 values: |trans E_i|; the rotation angle of E_i in degrees (atan2 of the antisymmetric part's norm and the trace: accurate at small angles);
 * |E_i - I_4|_F.  Per metric mean, std = sqrt(mean((e - mean)^2)) (population form, two passes, as np.std) and rmse = sqrt(mean(e^2)).  Sums are taken in an
 * order that depends on T only: a lane's row has the same bits alone, batched and at any lane index.
 *   rows: DEVICE fp64 [lanes][MV_EVAL_TRAJ_COLS]: the 12 statistics, R (row-major), t, c, d_1..d_3, the pose count, the pair count, the status.  Any status
 * but MV_TRAJ_OK gives NaN in the 12 statistics and in R, t, c: TOO_SHORT (T < 2: evo finds no pairs and raises), NONFINITE (a NaN / inf coordinate — this
 * case is ours, the reference never sees it; d is NaN too), DEGENERATE (above; d holds what the rule saw; it covers T = 2).  Lanes are independent.
 *   err_out (or NULL): DEVICE fp64 [lanes][4][err_stride], err_stride >= every T[l]: ATE_i (T values), then RTE_i, ROE_i, RPE_i (T - 1 values each) — what
 * PlotSeq draws; NaN for a lane that is not OK; entries past a lane's counts are not written. */
enum { MV_TRAJ_F32 = 0, MV_TRAJ_F64 = 1 };
enum { MV_TRAJ_ALIGN_UMEYAMA = 0, MV_TRAJ_ALIGN_ORIGIN = 1, MV_TRAJ_ALIGN_NONE = 2 };
enum { MV_TRAJ_OK = 0, MV_TRAJ_TOO_SHORT = 1, MV_TRAJ_DEGENERATE = 2, MV_TRAJ_NONFINITE = 3 };
#define MV_EVAL_TRAJ_MAX_POSES (1 << 20)
enum {
    MV_EVAL_TRAJ_ATE_MEAN = 0, MV_EVAL_TRAJ_ATE_STD, MV_EVAL_TRAJ_ATE_RMSE, MV_EVAL_TRAJ_RTE_MEAN, MV_EVAL_TRAJ_RTE_STD, MV_EVAL_TRAJ_RTE_RMSE,
    MV_EVAL_TRAJ_ROE_MEAN, MV_EVAL_TRAJ_ROE_STD, MV_EVAL_TRAJ_ROE_RMSE, MV_EVAL_TRAJ_RPE_MEAN, MV_EVAL_TRAJ_RPE_STD, MV_EVAL_TRAJ_RPE_RMSE,
    MV_EVAL_TRAJ_R00, MV_EVAL_TRAJ_R01, MV_EVAL_TRAJ_R02, MV_EVAL_TRAJ_R10, MV_EVAL_TRAJ_R11, MV_EVAL_TRAJ_R12, MV_EVAL_TRAJ_R20, MV_EVAL_TRAJ_R21,
    MV_EVAL_TRAJ_R22, MV_EVAL_TRAJ_TX, MV_EVAL_TRAJ_TY, MV_EVAL_TRAJ_TZ, MV_EVAL_TRAJ_SCALE, MV_EVAL_TRAJ_D1, MV_EVAL_TRAJ_D2, MV_EVAL_TRAJ_D3,
    MV_EVAL_TRAJ_N_POSES, MV_EVAL_TRAJ_N_PAIRS, MV_EVAL_TRAJ_STATUS, MV_EVAL_TRAJ_COLS
};
int mv_eval_traj_lanes(int lanes, const void* const* est /* host [lanes] of device pointers */, const void* const* ref /* host [lanes] */,
                       const int32_t* T /* host [lanes] */, int est_dtype, int ref_dtype, int64_t est_row_stride, int64_t ref_row_stride, int align,
                       int correct_scale, double* rows, double* err_out /* or NULL */, int64_t err_stride, mvStream_t stream);

/* ---- Trajectory time association (Utility/Trajectory.py:105-114: what Trajectory.from_sandbox does between loading poses.npy / ref_poses.npy and
 * handing the tracks to evaluateATE / RTE / ROE / RPE, Evaluation/EvalSeq.py:36): align_origin (:188-191), the rebase of both clocks (:107-108) and
 * align_time (:172-176 -> Utility/Math.py:96-121 interpolate_pose) of `lanes` tracks in ONE launch on `stream` — one query per thread, the lane in
 * blockIdx.y; nothing synchronises with the host, nothing is staged and nothing passes between workgroups (every workgroup of a lane repeats the lane's
 * checks).  PyPose's SE3 Inv / Mul / Log / Exp and evo's align_origin are RESTATED here, UNPINNED (neither is a vendored dependency).
 *   Per lane l, read where they lie (HOST arrays [lanes] of DEVICE pointers, passed by value in the kernel argument): src[l] — T[l] rows
 * (tx ty tz qx qy qz qw), src_dtype MV_TRAJ_F32 / MV_TRAJ_F64, src_row_stride elements (>= 7) between rows —, src_time[l] — its T[l] stamps —,
 * query_time[l] — Q[l] stamps —, both clocks time_dtype MV_TRAJ_TIME_F64 or MV_TRAJ_TIME_I64, and origin_ref[l] (origin_ref or an entry may be NULL):
 * the first row [7] of a reference track in origin_dtype, which turns the origin alignment on.  0 <= T[l], Q[l] <= MV_EVAL_TRAJ_MAX_POSES.
 *   Rebase (`rebase` != 0; the reference always does it): each clock is taken relative to its own first element.  int64 stamps are subtracted as
 * integers and only the difference becomes fp64 (EuRoC's nanoseconds, about 1.4e18, do not fit fp64: the reference's astype(float) rounds them to
 * multiples of 256 ns); fp64 stamps are subtracted in fp64, as the reference does.
 *   Placement (Math.py:99-121): a query <= ts[0] gets source row 0, a query >= ts[T-1] the last row, copied (widened or rounded to out_dtype), flag 1;
 * otherwise e is the first index with ts[e] >= tq (searchsorted(right=False); a bounded binary search, <= 31 steps), s = e - 1, and the result is
 * Exp(prop Log(P_e P_s^-1)) P_s with prop = (tq - ts[s]) / (ts[e] - ts[s]), flag 0.  A query ON an interior stamp has prop = 1 and goes through
 * Exp(Log(.)): it is not a copy.  T = 1: every query copies row 0.  Queries may come in any order and may repeat.
 *   Origin: with origin_ref[l] every source pose is first left-multiplied by ref_0 src_0^-1, its quaternion normalised and given w >= 0 (what evo's
 * matrix round trip leaves) — before the placement, copies included.
 *   Arithmetic: fp64 throughout on the exactly widened inputs, ONE rounding at the store.  The reference's chain for an fp32 estimate is mixed (fp32
 * Inv / @ / Log, fp64 Exp, fp32 again after from_evo(...).float()) and is not reproduced bit for bit; DESIGN.md section 7 has the measured gap.
 *   Writes: out_poses[l] — [Q[l], 7] in out_dtype (the reference's P_container takes the source's dtype) —, out_extrapolated[l] — uint8 [Q[l]], the
 * reference's ~interp_mask —, status — DEVICE int32 [lanes]: MV_TRAJ_OK, TOO_SHORT (T = 0), UNSORTED (some ts[i] >= ts[i+1]: Math.py:97 asserts),
 * NONFINITE (a non-finite stamp, source row or origin row; it wins over UNSORTED).  A lane that is not OK gets NaN poses and flags 0; the other lanes
 * never see it. */
enum { MV_TRAJ_UNSORTED = 4 };   /* extends MV_TRAJ_OK .. MV_TRAJ_NONFINITE */
enum { MV_TRAJ_TIME_F64 = 0, MV_TRAJ_TIME_I64 = 1 };
int mv_traj_associate_lanes(int lanes, const void* const* src /* host [lanes] of device pointers */, const void* const* src_time /* host [lanes] */,
                            const int32_t* T /* host [lanes] */, const void* const* query_time /* host [lanes] */, const int32_t* Q /* host [lanes] */,
                            const void* const* origin_ref /* host [lanes] or NULL */, int src_dtype, int time_dtype, int origin_dtype, int out_dtype,
                            int64_t src_row_stride, int rebase, void* const* out_poses /* host [lanes] */,
                            uint8_t* const* out_extrapolated /* host [lanes] */, int32_t* status /* DEVICE [lanes] */, mvStream_t stream);

/* PoseInterpolate.elaborate_map (Module/MapProcessor.py:33-45) on pose [T,7] in place, one workgroup, fp64 inside, fp32 at the store:
 * bad = need_interp with the first five and the last five rows forced to 0 — and CLEARED in need_interp itself, as the reference clears them in the
 * stored table (AutoScalingTensor.tensor is a narrow view, TensorExtension.py:100-101) —; a bad row i becomes Exp(prop Log(P_e P_s^-1)) P_s from its
 * nearest good rows s < i < e, prop = float(i - s) / float(e - s) (a float32 division, Utility/Math.py:114).  Good rows are never written; T < 11
 * changes no pose.  mask: uint8 [T], 1 on the rows it rewrote (the reference's bad_idx as a mask); nothing is read back. */
int mv_pose_interpolate(float* pose, uint8_t* need_interp, int T, uint8_t* mask, mvStream_t stream);
/* ... of every lane's map in one launch (one workgroup per lane): pose / need_interp come from stores_dev[l], T[l] rows (HOST [lanes]; a lane whose T
 * exceeds its store's cap_frames is left alone), mask is DEVICE uint8 [lanes][mask_stride], mask_stride >= every T[l]. */
int mv_pose_interpolate_lanes(const mvMapStores* stores_dev /* DEVICE [lanes] */, int lanes, const int32_t* T /* host [lanes] */, uint8_t* mask,
                              int64_t mask_stride, mvStream_t stream);

/* ---- Frame preprocessing (DataLoader/Transform.py:41-209: ScaleFrame, CenterCropFrame, SmartResizeFrame, CastDataType — the `Preprocess` block of
 * Config/Experiment/Common/Preprocess.yaml that every KITTI / Zed / VBR run starts with, DataLoader/SequenceBase.py:120-141): a host-only plan and ONE launch
 * per frame that resamples, crops or pads and converts every plane of every lane.  torchvision's tensor path (resize -> F.interpolate, center_crop) is
 * RESTATED, UNPINNED: torchvision is no dependency and the reference does not pin it (requirements.txt:17).
 *
 * mvPreprocessPlan: any foldable list of the four transforms as three steps per axis —
 *   window   the source after the crops / pads in FRONT of the resize: window(y, x) = src(y + win_y0, x + win_x0) for win_vy0 <= y < win_vy1 and
 *            win_vx0 <= x < win_vx1, 0 elsewhere (center_crop zero-pads a frame smaller than the crop; False for the mask);
 *   resized  window resampled to rs_h x rs_w: MV_PP_NEAREST = InterpolationMode.NEAREST_EXACT (src = min(floorf((dst + 0.5f) * (float(in) / float(out))),
 *            in - 1) in fp32) or MV_PP_BILINEAR = bilinear, align_corners False, antialias True (per axis scale = in / out, support = max(scale, 1),
 *            center = scale (i + 0.5), taps [max(0, int(center - support + 0.5)), min(in, int(center + support + 0.5))), weights
 *            max(0, 1 - |(j - center + 0.5) / max(scale, 1)|) normalised to sum 1; width pass first, then height; a weight-0 tap is still multiplied in, so
 *            a NaN under it spreads as in torch; an axis of unchanged size is not resampled).  scaled = 0: no resize, rs = window;
 *   out      the crops / pads BEHIND the resize: out(y, x) = resized(y + out_y0, x + out_x0) inside [out_vy0, out_vy1) x [out_vx0, out_vx1), 0 elsewhere.
 *            For SmartResizeFrame: crop origin = (max(out_y0, 0), max(out_x0, 0)), pads = out_vy0 / out_h - out_vy1 rows, out_vx0 / out_w - out_vx1 columns.
 *   round_scale_u / _v: W / target_w and H / target_h of the resize as fp32 (Transform.py:65-66): gt_flow's planes are divided by them AFTER the resize (:79-80),
 *   a true fp32 division.  K: the intrinsics after the list, row-major 3 x 3: rows 0 / 1 divided by round_scale_u / _v (:71-72), K[0][2] / K[1][2] lowered by the
 *   UN-rounded half difference of a crop (:124-125) while the crop itself starts at Python's round((size - crop) / 2.0), half to EVEN — 376 x 1241 -> 376 x 780
 *   cuts at column 230 and lowers cx by 230.5: the half-pixel disagreement is the reference's and is reproduced.
 *   mid_dtype / out_dtype (-1 = none): CastDataType in front of the resize (taps and the resized plane are rounded to it) / anywhere (the type of every plane at
 *   the store, the mask included).  16-bit planes are resampled in fp32 and rounded once, as torchvision does.
 *
 * mv_preprocess_plan (host only; the reference's Python double arithmetic, int() truncation and half-to-even rounding in C, as mv_input_pad does for the padder):
 *   prev == NULL: the plan of ONE transform of a src_h x src_w frame with intrinsics K (host float[9], NULL = identity); prev != NULL: `prev` followed by the
 *   transform (src_h, src_w, K are ignored; plan may be prev) — a `Preprocess` list still costs one launch.  kind MV_PP_SCALE: a0 = scale_u, a1 = scale_v,
 *   mode = MV_PP_NEAREST / MV_PP_BILINEAR: target = int(size / scale); a target equal to the size is a copy.  MV_PP_CENTER_CROP: a0 = height, a1 = width.
 *   MV_PP_SMART_RESIZE: a0 = height, a1 = width, mode = interpolation: s = min(H / a0, W / a1), scale by (s, s), then the centre crop — after int() the resized
 *   frame is often one pixel short of the target (379 x 1250 -> 375 x 1240 for 376 x 780) and the crop pads a zero row / column.  MV_PP_CAST: mode = MV_F32 /
 *   MV_F16 / MV_BF16.  MV_ERR_UNSUPPORTED: the transform does not fold into `prev` (a second real resize, a second cast to another type): start a new plan
 *   from prev's output; MV_ERR_INVALID_ARG: a size outside [1, 32768], a scale that is not positive, a target of 0 rows or columns.
 *
 * mv_preprocess_lanes: the launch.  groups: HOST array of n_groups <= MV_PP_MAX_GROUPS plane groups, each `planes` planes per lane: src [lanes][planes][src_h]
 *   [src_w] with src_lane_stride ELEMENTS between lanes, dst [lanes][planes][out_h][out_w] likewise; kind MV_PP_IMAGE (src fp32 / fp16 / bf16 or MV_PP_U8,
 *   widened as float(u8) / 255.0f — what the reference's loaders do in front of the transform, a quarter of the upload), MV_PP_FLOW (2 planes: u, v; divided by
 *   their round_scale), MV_PP_MASK (src MV_PP_U8 = bool: a gather under MV_PP_NEAREST, resampled != 0 under MV_PP_BILINEAR — torchvision filters it as fp32 and
 *   casts back without rounding —; dst MV_PP_U8 or a float type), MV_PP_DEPTH.  dst_dtype: the store type, rounded once.  Nearest plans and plans without a
 *   resize are gathers: bit-exact.  Pointers need their element's alignment only (vector loads / stores are used where an address allows them).
 *   MV_PP_BILINEAR with a downscale above 8 on an axis: MV_ERR_UNSUPPORTED, nothing is launched (the reference's resolution sweep goes to 4). */
enum { MV_PP_SCALE = 0, MV_PP_CENTER_CROP = 1, MV_PP_SMART_RESIZE = 2, MV_PP_CAST = 3 };
enum { MV_PP_NEAREST = 0, MV_PP_BILINEAR = 1 };
enum { MV_PP_IMAGE = 0, MV_PP_FLOW = 1, MV_PP_MASK = 2, MV_PP_DEPTH = 3 };
enum { MV_PP_U8 = 7 };           /* extends MV_F32 / MV_F16 / MV_BF16 for mvPreprocessGroup.src_dtype / dst_dtype */
#define MV_PP_MAX_GROUPS 8
typedef struct mvPreprocessPlan {
    int32_t src_h, src_w;
    int32_t win_h, win_w, win_y0, win_x0, win_vy0, win_vy1, win_vx0, win_vx1;
    int32_t rs_h, rs_w;
    int32_t out_h, out_w, out_y0, out_x0, out_vy0, out_vy1, out_vx0, out_vx1;
    int32_t scaled, interp, mid_dtype, out_dtype;
    float round_scale_u, round_scale_v;
    float K[9];
} mvPreprocessPlan;
typedef struct mvPreprocessGroup {
    const void* src;
    void* dst;
    int64_t src_lane_stride, dst_lane_stride;
    int32_t planes, kind, src_dtype, dst_dtype;
} mvPreprocessGroup;
int mv_preprocess_plan(mvPreprocessPlan* plan /* host */, const mvPreprocessPlan* prev /* host or NULL */, int src_h, int src_w,
                       const float* K /* host [9] or NULL */, int kind, double a0, double a1, int mode);
int mv_preprocess_lanes(const mvPreprocessPlan* plan /* host */, const mvPreprocessGroup* groups /* host [n_groups] */, int n_groups, int lanes,
                        mvStream_t stream);

/* ---- Stereo rectification (DataLoader/Dataset/EuRoC.py:143-174, 231-236 and VBR.py:60-64, 155-180: cv2.stereoRectify(flags = CALIB_ZERO_DISPARITY,
 * alpha = -1) once per sequence, cv2.initUndistortRectifyMap(CV_32FC1) once per camera, cv2.remap(INTER_LINEAR) on every image, then float32 / 255): a
 * host-only plan in double arithmetic, one launch that builds both cameras' maps, one launch per frame that remaps every plane of every lane.  OpenCV is
 * RESTATED, PARITY-UNPINNED: it is no dependency here.  Known difference: OpenCV keeps the four undistorted image corners in float32, the plan keeps them in
 * double, so the rectified principal point agrees with OpenCV's to about 1e-4 px.  Fed EuRoC's public calibration the plan gives the baseline the reference
 * hard-codes (EuRoC.py:76, 0.1100778422).
 *
 * mv_stereo_rectify_plan (host only, no GPU; replaces cv2.stereoRectify, EuRoC.py:165-167 / VBR.py:175-177): K1, K2 row-major 3 x 3 doubles; D1, D2 n_d1 /
 *   n_d2 = 4, 5 or 8 coefficients k1 k2 p1 p2 [k3 [k4 k5 k6]] (missing ones are 0; another count: MV_ERR_UNSUPPORTED); image size (nx, ny) = (width,
 *   height); R (3 x 3), T (3): camera 1 to camera 2.  Bouguet's method:
 *     om = Rodrigues^-1(R); r_r = Rodrigues(-om / 2); t = r_r T; idx = |t.x| > |t.y| ? 0 : 1 (0 a horizontal rig, 1 a vertical one);
 *     c = t[idx]; uu = e_idx sign(c); ww = t x uu; if |ww| > 0: ww *= acos(|c| / |t|) / |ww|; wR = Rodrigues(ww);
 *     R1 = wR r_r^T, R2 = wR r_r, t_new = R2 T;
 *     per camera f = K[idx ^ 1][idx ^ 1], f *= 1 + k1 (nx^2 + ny^2) / (4 f^2) if k1 < 0; fc = the smaller of the two;
 *     per camera the corners (0 | nx - 1, 0 | ny - 1) are undistorted (five fixed-point iterations of the inverse model), rotated by R_k and projected with
 *     focal fc and a zero principal point; cc_k = ((nx - 1) / 2, (ny - 1) / 2) - their mean; both cameras get the average of cc_1 and cc_2;
 *     P1 = [fc 0 ccx 0; 0 fc ccy 0; 0 0 1 0], P2 = P1 with P2[idx][3] = t_new[idx] fc.
 *   The plan holds R1, R2, P1, P2 (row-major 3 x 4), per camera what the map builder needs (iR = (P[:3,:3] R_k)^-1, fx fy cx cy of the ORIGINAL camera, the
 *   eight coefficients), K = P1[:3,:3] as fp32 (the K of every later stage) and baseline = |P2[idx][3] / fc|.  MV_ERR_INVALID_ARG: |T| = 0, a non-finite
 *   input, a size outside [1, 32768].  alpha >= 0, the valid ROIs, Q and fisheye models are not built.
 *
 * mv_rectify_maps (one launch; replaces cv2.initUndistortRectifyMap, EuRoC.py:169-170 / VBR.py:179-180): for each of n_cams <= MV_RM_MAX_GROUPS cameras (HOST
 *   array) and each pixel (u, v) of an out_h x out_w grid: [x y w] = iR [u v 1]; x' = x / w, y' = y / w; r2 = x'^2 + y'^2;
 *   kr = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3); xd = x' kr + 2 p1 x' y' + p2 (r2 + 2 x'^2); yd = y' kr + p1 (r2 + 2 y'^2) +
 *   2 p2 x' y'; map_x = fx xd + cx, map_y = fy yd + cy — in fp64 on the device, rounded once to fp32.  map_x, map_y: DEVICE fp32 [n_cams][out_h][out_w]
 *   (cv2's CV_32FC1 pair: a map made elsewhere serves mv_remap_lanes as well).
 *
 * mv_remap_lanes (one launch per frame; replaces cv2.remap and the loaders' float32 / 255, EuRoC.py:224-236 / VBR.py:50-65): groups: HOST array of n_groups <=
 *   MV_RM_MAX_GROUPS groups (the left and the right images are two groups with their own maps), each with `channels` = 1, 3 or 4: src uint8 (src_dtype
 *   MV_PP_U8), layout MV_RM_HWC [lanes][src_h][src_w][channels] (what cv2.imread returns) or MV_RM_PLANAR [lanes][channels][src_h][src_w]; dst always planar
 *   [lanes][channels][out_h][out_w] of dst_dtype MV_PP_U8 / MV_F32 / MV_F16 / MV_BF16; map_x, map_y fp32 [out_h][out_w] with map_lane_stride ELEMENTS between
 *   lanes (0: one map for every lane, the usual case); lane strides in ELEMENTS; reverse_channels: destination channels 0 and 2 read source channels 2 and 0
 *   (VBR's BGR -> RGB; EuRoC keeps BGR).  Arithmetic (csrc/remap_math.h): cv2's fixed-point INTER_LINEAR for 8-bit images, BORDER_CONSTANT 0, in integers:
 *   s = rndne(map * 32) in fp32 (half to even); i = s >> 5 (floor), f = s & 31; taps outside the source count 0, each on its own; out = ((32 - fx)(32 - fy)
 *   p00 + fx (32 - fy) p01 + (32 - fx) fy p10 + fx fy p11 + 512) >> 10 — OpenCV's 15-bit weight table exactly.  Defined where OpenCV's result depends on the
 *   platform: a NaN entry, or one whose * 32 leaves [-2^30, 2^30], yields 0.  Float destinations store float(out) / 255.0f (a true division), rounded once
 *   more for fp16 / bf16.  MV_ERR_UNSUPPORTED (nothing is launched): channels other than 1, 3, 4; a source that is not uint8; MV_ERR_INVALID_ARG: more than
 *   MV_RM_MAX_GROUPS groups, sizes outside [1, 32768], strides smaller than a lane, misaligned maps or destinations.  INTER_CUBIC and float sources are not
 *   built. */
#define MV_RM_MAX_GROUPS 4
enum { MV_RM_PLANAR = 0, MV_RM_HWC = 1 };
typedef struct mvRectifyCam {
    double iR[9];              /* (P[:3,:3] R_k)^-1, row-major */
    double fx, fy, cx, cy;     /* the original camera */
    double k[8];               /* k1 k2 p1 p2 k3 k4 k5 k6 */
} mvRectifyCam;
typedef struct mvRectifyPlan {
    double R1[9], R2[9], P1[12], P2[12];
    mvRectifyCam cam[2];
    double fc, baseline;
    float K[9];                /* P1[:3,:3] */
    int32_t width, height, idx;
} mvRectifyPlan;
typedef struct mvRemapGroup {
    const void* src;
    void* dst;
    const float* map_x;
    const float* map_y;
    int64_t src_lane_stride, dst_lane_stride, map_lane_stride;
    int32_t channels, layout, reverse_channels, src_dtype, dst_dtype, reserved;
} mvRemapGroup;
int mv_stereo_rectify_plan(mvRectifyPlan* plan /* host */, const double* K1, const double* D1, int n_d1, const double* K2, const double* D2, int n_d2, int nx,
                           int ny, const double* R, const double* T);
int mv_rectify_maps(const mvRectifyCam* cams /* host [n_cams] */, int n_cams, int out_h, int out_w, float* map_x, float* map_y, mvStream_t stream);
int mv_remap_lanes(const mvRemapGroup* groups /* host [n_groups] */, int n_groups, int lanes, int src_h, int src_w, int out_h, int out_w, mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * The PoseNet of TartanMotionNet (Module/Network/TartanVOStereo/FlowPoseNet.py:45-166 as StereoVO.py:21 constructs it: VOFlowRes(config = 1,
 * stereo, down_scale, intrinsic, autoDistTarget = 0, no out_feature), called with scale_disp = 1): 51 convolutions and 6 linear layers,
 * 15 135 430 fp32 parameters in 120 tensors.  Forward only; fp32 weights, activations and accumulation (csrc/posenet.hip, csrc/posenet_math.h).
 *
 * mv_posenet_tensor_count / mv_posenet_tensor_info: the 120 tensors in the order of the module's state_dict(), with the reference's key names
 *   ("firstconv.0.0.weight", "layer3.0.downsample.bias", "voflow_rot.2.weight", ...); name_buf holds at least 64 bytes, shape[ndim..3] = 0.
 * mv_posenet_pack: host.  tensors_host[i] = tensor i, contiguous fp32; packed_host = mv_posenet_packed_bytes() bytes in the layout the kernels read
 *   (per launch: 16-channel tiles of K steps in MFMA operand order, a downsample's rows behind its block's second convolution, the summed bias).
 *   Pack once per network, upload once.
 * mv_posenet_forward_lanes: x [lanes, 5, 112, 160] fp32 (what mv_motion_input_lanes writes) -> out [lanes, 6] fp32 = cat(trans, rot), before the
 *   pose_norm scaling.  1 <= lanes <= MV_MAX_LANES.  50 launches on `stream`, no host synchronisation, allocation or copy.  workspace:
 *   mv_posenet_workspace_bytes(lanes) bytes (0 for an unsupported lane count), 16-byte aligned, contents irrelevant.  stage_out: NULL, or six device
 *   pointers (NULL entries are skipped) that receive the NCHW outputs of firstconv [32,56,80], layer1 [64,28,40], layer2 [128,14,20], layer3
 *   [128,7,10], layer4 [256,4,5] and layer5 [256,2,3] per lane.  A lane's output bits depend on neither `lanes` nor its place in the batch; two
 *   runs give the same bits; NaN propagates as in torch (ReLU keeps it). */
int mv_posenet_tensor_count(void);
int mv_posenet_tensor_info(int i, char* name_buf, int32_t* shape /* [4] */, int32_t* ndim);
size_t mv_posenet_packed_bytes(void);
size_t mv_posenet_workspace_bytes(int lanes);
int mv_posenet_pack(const float* const* tensors_host /* [120] */, void* packed_host);
int mv_posenet_forward_lanes(const void* packed_dev, const float* x, int lanes, float* out, void* workspace, float* const* stage_out /* host [6] or NULL */,
                             mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * The decoder's recurrent update blocks in 16-bit operands, one call per decoder iteration (csrc/update_block.hip, csrc/update_block_math.h).
 *   MV_UPDATE_COV   CovUpdateBlock.forward (Module/Network/FlowFormerCov/covhead.py:24-43): SepConvGRU (hidden 128, input 384; 1x5 then 5x1),
 *                   CovHead 128 -> 256 -> 128 -> 64 -> 2 (covhead.py:8-21), mask 128 -> 256 -> 576 scaled by 0.25 (covhead.py:42)
 *   MV_UPDATE_FLOW  covhead.py:112-114: the gru, flow_head (128 -> 256 -> 2) and mask (128 -> 256 -> 576, unscaled: the caller applies 0.25 at
 *                   covhead.py:122) members of FlowFormer's GMAUpdateBlock
 * operand: MV_F16 or MV_BF16 — the type of net, inp, the three outputs and the MFMA operands; accumulation and pointwise maths are fp32, a value is
 * rounded once where it is stored.  Not bit-equal to the eager 16-bit module, which rounds after every operator.
 *
 * mv_update_block_tensor_count / _tensor_info: the block's tensors in state_dict() order ("gru.convz1.weight", ..., "mask.2.bias"; COV 24, FLOW 20 =
 *   the gru.*, flow_head.* and mask.* entries of the GMAUpdateBlock); name_buf holds at least 64 bytes, shape[ndim..3] = 0.
 * mv_update_block_pack: device.  tensors[i] (host array of DEVICE pointers) = tensor i, contiguous fp32; packed = mv_update_block_packed_bytes(kind,
 *   operand) bytes, 16-byte aligned: per launch the weights in MFMA fragment order, rounded to the operand type, and the fp32 biases.  Pack once.
 * mv_update_block_forward: net [B,128,H,W], inp [B,384,H,W] (NCHW-contiguous, or channels-last memory when channels_last = 1) ->
 *   net_out [B,128,H,W], delta [B,2,H,W], mask [B,576,H,W], NCHW-contiguous.  net_out may be net.  B, H, W >= 1, B * H * W <= 2^20.  workspace:
 *   mv_update_block_workspace_bytes(kind, B, H, W) bytes (0 for sizes out of range), 16-byte aligned, contents irrelevant.  9 (FLOW) or 11 (COV)
 *   launches on `stream`; no atomics, host synchronisation or allocation; two calls give the same bits; NaN propagates as in torch (ReLU keeps it).
 * Arguments are checked before anything touches the device: MV_ERR_INVALID_ARG for a null pointer, an unknown kind or operand, a size out of range. */
enum { MV_UPDATE_COV = 0, MV_UPDATE_FLOW = 1 };
int mv_update_block_tensor_count(int kind);
int mv_update_block_tensor_info(int kind, int i, char* name_buf, int32_t* shape /* [4] */, int32_t* ndim);
size_t mv_update_block_packed_bytes(int kind, int operand);
int mv_update_block_pack(int kind, int operand, const float* const* tensors /* host [count] of device pointers */, void* packed, mvStream_t stream);
size_t mv_update_block_workspace_bytes(int kind, int B, int H, int W);
int mv_update_block_forward(int kind, int operand, const void* packed, const void* net, const void* inp, int B, int H, int W, int channels_last,
                            void* net_out, void* delta, void* mask, void* workspace, mvStream_t stream);

/* -------------------------------------------------------------------------------------------
 * The decoder's motion encoder in 16-bit operands, one call per decoder iteration (csrc/motion_encoder.hip, csrc/motion_encoder_math.h):
 * GMAUpdateBlock.encoder as called at covhead.py:106,
 *   out = cat([relu(conv(cat([relu(convc2(relu(convc1(corr)))), relu(convf2(relu(convf1(flow))))]))), flow])
 * with convc1 145 -> 256 (1x1), convc2 256 -> 192 (3x3), convf1 2 -> 128 (7x7), convf2 128 -> 64 (3x3), conv 256 -> 126 (3x3).
 * operand: MV_F16 or MV_BF16 - the type of flow, corr, out and the MFMA operands; accumulation, bias and ReLU are fp32, a value is rounded once where
 * it is stored; flow reaches channels 126..127 of out bit for bit.  Not bit-equal to the eager 16-bit module, which rounds after every operator.
 *
 * mv_motion_encoder_tensor_count / _tensor_info: the module's 10 tensors in state_dict() order ("convc1.weight", ..., "conv.bias"); name_buf holds at
 *   least 64 bytes, shape[ndim..3] = 0.
 * mv_motion_encoder_pack: device.  tensors[i] (host array of DEVICE pointers) = tensor i, contiguous fp32; packed = mv_motion_encoder_packed_bytes(operand)
 *   bytes, 16-byte aligned: per launch the weights in MFMA fragment order, rounded to the operand type, and the fp32 biases.  Pack once.
 * mv_motion_encoder_forward: flow [B,2,H,W], corr [B,145,H,W] (NCHW-contiguous, or both channels-last memory when channels_last = 1) ->
 *   out [B,128,H,W], NCHW-contiguous.  B, H, W >= 1, B * H * W <= 2^20.  workspace: mv_motion_encoder_workspace_bytes(B, H, W) bytes (1 920 per pixel; 0
 *   for sizes out of range), 16-byte aligned, contents irrelevant.  6 launches on `stream`; no atomics, host synchronisation or allocation; two calls
 *   and both layouts give the same bits; NaN propagates as in torch (ReLU keeps it).
 * Arguments are checked before anything touches the device: MV_ERR_INVALID_ARG for a null pointer, an unknown operand, a size out of range. */
int mv_motion_encoder_tensor_count(void);
int mv_motion_encoder_tensor_info(int i, char* name_buf, int32_t* shape /* [4] */, int32_t* ndim);
size_t mv_motion_encoder_packed_bytes(int operand);
int mv_motion_encoder_pack(int operand, const float* const* tensors /* host [10] of device pointers */, void* packed, mvStream_t stream);
size_t mv_motion_encoder_workspace_bytes(int B, int H, int W);
int mv_motion_encoder_forward(int operand, const void* packed, const void* flow, const void* corr, int B, int H, int W, int channels_last, void* out,
                              void* workspace, mvStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MACVO_HIP_H */
