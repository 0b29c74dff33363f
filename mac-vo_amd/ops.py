"""Torch-tensor front doors of the C ABI (``include/macvo_hip.h``).

PyTorch is only the allocator / stream provider here: each function validates shapes, allocates the
outputs, and hands raw device pointers plus the *current* HIP stream to ``libmacvo_hip.so``.  Nothing is
computed in torch and there is no fallback path — a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib as L

_DT = {torch.float32: L.MV_F32, torch.float16: L.MV_F16, torch.bfloat16: L.MV_BF16}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """Raw hipStream_t of torch's CURRENT stream on the current device.  `torch.cuda.current_stream()` builds a Python
    Stream object through several layers (~8 us per call, ~25 calls per frame); the raw getter is ~0.2 us."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _req(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise L.MacvoHipError(f"{name}: expected a GPU tensor (the HIP hot path has no CPU fallback)")
    if t.dtype != dtype:
        raise L.MacvoHipError(f"{name}: expected {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _u8(t: torch.Tensor | None) -> torch.Tensor | None:
    if t is None:
        return None
    if t.dtype == torch.bool:
        t = t.contiguous().view(torch.uint8)
    return _req(t, torch.uint8, "mask")


# ------------------------------------------------------------------------------------------- A5
def default_volume_precision() -> str:
    """THE default arithmetic of the fp32 cost volume — one value for ``corr_volume``, ``pipeline.HotPathConfig``,
    ``plugins.install_flowformer_hooks`` (hence every ``HIP_*`` frontend plugin, whose YAML key set is the reference's and cannot
    carry the choice) and ``bench.py``: ``"f16x2"``, the fastest form that keeps the fp32 parity bar
    (error <= ~2^-21 sum |a||b|, not narrower than the TF32 the reference runs this GEMM in, Frontend.py:275-277); shapes the
    streaming kernel does not cover fall back to "exact".  ``MACVO_HIP_VOLUME_PRECISION=exact|bf16x3|f16x2`` overrides it."""
    import os

    v = os.environ.get("MACVO_HIP_VOLUME_PRECISION", "f16x2")
    if v not in ("exact", "bf16x3", "f16x2"):
        raise L.MacvoHipError(f"MACVO_HIP_VOLUME_PRECISION={v!r}: expected exact | bf16x3 | f16x2")
    return v


def corr_volume(f1: torch.Tensor, f2: torch.Tensor, layout: str = "chw", out: torch.Tensor | None = None,
                precision: str | None = None) -> torch.Tensor:
    """All-pairs cost volume (FlowFormer ``MemoryEncoder.corr``; call site flownet.py:26-27).

    layout "chw": f1, f2 ``[B, C, H, W]`` (NCHW);  layout "hwc": ``[B, H, W, C]`` / ``[B, N, C]``.
    precision (fp32 inputs only; None = ``default_volume_precision()``, 16-bit inputs ignore it): "exact" = fp32 MFMA (bitwise fmaf chain); "f16x2" = rows scaled by a power of two into fp16's
    range, two fp16 pieces, three products (error <= ~2^-21 sum |a||b|: inside the parity bar, the fastest form); "bf16x3" = operands packed into three bf16 pieces
    (``volume_pack``) + the streaming six-product kernel on the 16-bit matrix pipe, fp32-class accuracy (same parity bar as
    "exact", not bitwise), either layout, shapes the kernel does not cover (C != 256, N1 < 32, N2 < 64 — any larger N2, multiple of 64 or not) fall back to "exact"; "split3" / "split2" = the
    round-1/2 tile kernels over pre-split planes (6 / 3 products; "split2": relative error ~2^-16, finer than TF32, the class
    the reference's fast frontend allows itself) — both layout "hwc" only.
    Returns ``cost_maps [B*H1*W1, 1, H2, W2]`` float32 (layout "hwc" with 3-D inputs: ``[B*N1, 1, 1, N2]``).
    """
    lib = L.load()
    if f1.dtype not in _DT or f1.dtype != f2.dtype:
        raise L.MacvoHipError(f"corr_volume: unsupported dtypes {f1.dtype}/{f2.dtype}")
    f1 = _req(f1, f1.dtype, "f1")
    f2 = _req(f2, f2.dtype, "f2")
    if layout == "chw":
        B, Cc, H1, W1 = f1.shape
        _, _, H2, W2 = f2.shape
        lay = L.MV_LAYOUT_CHW
    elif layout == "hwc":
        if f1.dim() == 4:
            B, H1, W1, Cc = f1.shape
            _, H2, W2, _ = f2.shape
        else:
            B, N1_, Cc = f1.shape
            H1, W1, H2, W2 = 1, N1_, 1, f2.shape[1]
        lay = L.MV_LAYOUT_HWC
    else:
        raise ValueError(layout)
    N1, N2 = H1 * W1, H2 * W2
    if out is None:
        out = torch.empty((B * N1, 1, H2, W2), dtype=torch.float32, device=f1.device)
    dt = _DT[f1.dtype]
    p1, p2 = f1, f2
    if precision is None:
        precision = default_volume_precision() if f1.dtype == torch.float32 else "exact"
    if precision in _PACK_MODE:
        if f1.dtype != torch.float32:
            raise L.MacvoHipError(f"corr_volume: precision='{precision}' splits float32 inputs")
        if lib.mv_corr_volume_packed_supported(B, Cc, N1, N2, _PACK_MODE[precision]):
            pk1, pk2 = volume_pack(f1, f2, layout, mode=precision)
            return corr_volume_packed(pk1, pk2, B, Cc, N1, N2, out=out, mode=precision)
        precision = "exact"
    if precision in ("split3", "split2"):
        if f1.dtype != torch.float32 or lay != L.MV_LAYOUT_HWC:
            raise L.MacvoHipError(f"corr_volume: precision='{precision}' needs float32 inputs in layout 'hwc'")
        p1 = torch.empty((3,) + tuple(f1.shape), dtype=torch.bfloat16, device=f1.device)
        p2 = torch.empty((3,) + tuple(f2.shape), dtype=torch.bfloat16, device=f2.device)
        L.check(lib.mv_split_bf16x3(f1.data_ptr(), p1.data_ptr(), f1.numel(), _stream()), "mv_split_bf16x3")
        L.check(lib.mv_split_bf16x3(f2.data_ptr(), p2.data_ptr(), f2.numel(), _stream()), "mv_split_bf16x3")
        dt = L.MV_BF16X3 if precision == "split3" else L.MV_BF16X2
    elif precision != "exact":
        raise ValueError(precision)
    L.check(lib.mv_corr_volume(p1.data_ptr(), p2.data_ptr(), out.data_ptr(), B, Cc, N1, N2, dt, lay, _stream()),
            "mv_corr_volume")
    return out


_PACK_MODE = {"bf16x3": L.MV_PACK_BF16X3, "f16x2": L.MV_PACK_F16X2}


def volume_pack(f1: torch.Tensor, f2: torch.Tensor, layout: str = "chw", out: "tuple | None" = None, mode: str = "bf16x3",
                tiled_hw: "tuple | None" = None):
    """fp32 feature maps -> the packed operands of ``corr_volume_packed`` (``mv_volume_pack``: both maps in one launch,
    MFMA-fragment order, row N - 1 replicated past the edge).  mode "bf16x3": three bf16 pieces; "f16x2": two fp16 pieces of
    every value after a per-row power-of-two scaling (+ the table of row exponents).  Returns two uint8 tensors (opaque).
    ``tiled_hw=(H2, W2)``: operand 2 in 4 x 4-tile order (``mv_volume_pack_tiled``) -> the volume comes out tiled for
    ``corr_lookup(..., tiled=True)``."""
    md = _PACK_MODE[mode]
    lib = L.load()
    f1 = _req(f1, torch.float32, "f1")
    f2 = _req(f2, torch.float32, "f2")
    if layout == "chw":
        B, Cc = f1.shape[0], f1.shape[1]
        N1, N2 = f1[0, 0].numel(), f2[0, 0].numel()
    else:
        B, Cc = f1.shape[0], f1.shape[-1]
        N1, N2 = f1[0, ..., 0].numel(), f2[0, ..., 0].numel()
    n1, n2 = lib.mv_volume_pack_bytes(B, Cc, N1, md), lib.mv_volume_pack_bytes(B, Cc, N2, md)
    if n1 == 0 or n2 == 0:
        raise L.MacvoHipError("volume_pack: unsupported shape (C % 16 != 0?)")
    p1, p2 = out if out is not None else (torch.empty(n1, dtype=torch.uint8, device=f1.device), torch.empty(n2, dtype=torch.uint8, device=f1.device))
    assert p1.numel() >= n1 and p2.numel() >= n2
    lay = L.MV_LAYOUT_CHW if layout == "chw" else L.MV_LAYOUT_HWC
    if tiled_hw is not None:
        H2, W2 = tiled_hw
        assert H2 * W2 == N2
        L.check(lib.mv_volume_pack_tiled(f1.data_ptr(), f2.data_ptr(), p1.data_ptr(), p2.data_ptr(), B, Cc, N1, H2, W2, lay, md, _stream()),
                "mv_volume_pack_tiled")
    else:
        L.check(lib.mv_volume_pack(f1.data_ptr(), f2.data_ptr(), p1.data_ptr(), p2.data_ptr(), B, Cc, N1, N2, lay, md, _stream()),
                "mv_volume_pack")
    return p1, p2


def corr_volume_packed(pk1: torch.Tensor, pk2: torch.Tensor, B: int, C_: int, N1: int, N2: int, out: torch.Tensor | None = None,
                       mode: str = "bf16x3", free_cus: int = 0) -> torch.Tensor:
    """The cost volume ``[B*N1, 1, 1, N2]`` fp32 from two packed operands (``mv_corr_volume_packed``: six bf16 / three fp16 piece
    products, fp32 accumulate; C = 256, N1 >= 32, any N2 >= 64).  ``free_cus``: compute units left without a persistent workgroup (``mv_corr_volume_packed_shared``;
    same bits)."""
    lib = L.load()
    if out is None:
        out = torch.empty((B * N1, 1, 1, N2), dtype=torch.float32, device=pk1.device)
    L.check(lib.mv_corr_volume_packed_shared(pk1.data_ptr(), pk2.data_ptr(), out.data_ptr(), B, C_, N1, N2, _PACK_MODE[mode], int(free_cus), _stream()),
            "mv_corr_volume_packed_shared")
    return out


def last_volume_kernel() -> str:
    """Name of the kernel the last ``corr_volume`` call of this thread dispatched (diagnostics: dispatch tests, bench.py)."""
    return (L.load().mv_corr_volume_last_kernel() or b"").decode()


# ------------------------------------------------------------------------------------------- A23
def local_corr81(first: torch.Tensor, second: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """PWC-Net ``FunctionCorrelation(tenFirst, tenSecond)`` forward (pwc/correlation.py:277-325): ``[B,C,H,W]`` x2 ->
    ``[B,81,H,W]``, channel ``9*(dy+4)+(dx+4)`` = mean over C of ``first[y,x] * second[y+dy,x+dx]``, zero padded."""
    lib = L.load()
    first = _req(first, torch.float32, "first")
    second = _req(second, torch.float32, "second")
    if first.shape != second.shape or first.dim() != 4:
        raise L.MacvoHipError("local_corr81: first / second must be [B,C,H,W] tensors of the same shape")
    B, Cc, H, W = first.shape
    if out is None:
        out = torch.empty((B, 81, H, W), dtype=torch.float32, device=first.device)
    L.check(lib.mv_local_corr81(first.data_ptr(), second.data_ptr(), out.data_ptr(), B, Cc, H, W, _stream()),
            "mv_local_corr81")
    return out


# ------------------------------------------------------------------------------------------- A6
def corr_lookup(cost_maps: torch.Tensor, coords: torch.Tensor, radius: int = 4, out: torch.Tensor | None = None,
                tiled: bool = False, image_hw: "tuple | None" = None) -> torch.Tensor:
    """``encode_flow_token(cost_maps, coords)`` (covhead.py:92): ``[B*N1,1,H2,W2]``, ``[B,2,H1,W1]`` -> ``[B,(2r+1)^2,H1,W1]``.
    ``tiled``: the slices of ``cost_maps`` are stored in 4 x 4-cell tiles (``volume_pack(tiled_hw=...)`` + ``corr_volume_packed``, or
    ``corr_volume_out16(tiled=True)``); ``image_hw=(H2, W2)``: the image the slices cover when a tiled fp16 slice carries a padded
    last tile row (H2 % 4 != 0: ``cost_maps`` is then ``[B*N1, 1, 4 * ceil(H2 / 4), W2]``)."""
    lib = L.load()
    vol16 = cost_maps.dtype == torch.float16                    # Fast mode: the volume as `corr_volume_out16` stores it
    cost_maps = _req(cost_maps, torch.float16 if vol16 else torch.float32, "cost_maps")
    coords = _req(coords, torch.float32, "coords")
    B, two, H1, W1 = coords.shape
    assert two == 2
    BN, _, H2, W2 = cost_maps.shape
    if BN != B * H1 * W1:
        raise L.MacvoHipError("corr_lookup: cost_maps / coords shape mismatch")
    if image_hw is not None:
        if not (tiled and vol16) or image_hw[1] != W2 or lib.mv_tiled_slice_cells(int(image_hw[0]), W2) != H2 * W2:
            raise L.MacvoHipError("corr_lookup: image_hw belongs to a tiled fp16 volume of mv_tiled_slice_cells(H2, W2) cells per slice")
        H2 = int(image_hw[0])
    K = 2 * radius + 1
    if out is None:
        out = torch.empty((B, K * K, H1, W1), dtype=torch.float32, device=coords.device)
    name = "mv_corr_lookup" + ("_tiled" if tiled else "") + ("_vol16" if vol16 else "")
    L.check(getattr(lib, name)(cost_maps.data_ptr(), coords.data_ptr(), out.data_ptr(), B, H1, W1, H2, W2, radius, _stream()), name)
    return out


def fmap_tile_rows16(f: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """A 16-bit HWC feature map ``[B, H, W, C]`` with its pixel rows in 4 x 4-tile order (``mv_fmap_tile_rows16``): operand 2 of
    ``corr_volume_out16`` for a tiled Fast-mode volume."""
    lib = L.load()
    if f.dtype not in (torch.float16, torch.bfloat16) or f.dim() != 4:
        raise L.MacvoHipError("fmap_tile_rows16: a [B, H, W, C] float16 / bfloat16 feature map")
    f = _req(f, f.dtype, "f")
    B, H, W, Cc = f.shape
    cells = lib.mv_tiled_slice_cells(H, W)
    if cells == 0:
        raise L.MacvoHipError("fmap_tile_rows16: W % 4 != 0")
    if out is None:
        out = torch.empty((B, cells // W, W, Cc), dtype=f.dtype, device=f.device)      # (rows >= H of the last tile row: zero pixels)
    assert out.numel() >= B * cells * Cc and out.dtype == f.dtype
    L.check(lib.mv_fmap_tile_rows16(f.data_ptr(), out.data_ptr(), B, Cc, H, W, _stream()), "mv_fmap_tile_rows16")
    return out


def corr_volume_out16(f1: torch.Tensor, f2: torch.Tensor, out: torch.Tensor | None = None, tiled: bool = False,
                      scratch: torch.Tensor | None = None) -> torch.Tensor | None:
    """Fast mode (enc_dtype fp16 / bf16, MACVO_Fast.yaml:73-74): the volume in the encoder's 16-bit type — what ``einsum`` returns there and
    flownet.py:27 widens — rounded ONCE in the GEMM's epilogue.  ``f1, f2 [B, H, W, C]`` (HWC) fp16 / bf16 -> ``[B*H1*W1, 1, H2, W2]`` of that
    dtype; ``None`` for shapes outside the streaming kernel's domain — C not 128 / 256, N2 < 64 or odd, B * N1 * N2 < 2^22 — (callers then cast ``corr_volume``'s fp32 result).
    ``tiled``: every slice in 4 x 4-cell tiles (``fmap_tile_rows16`` on ``f2`` first, into ``scratch`` if given) for
    ``corr_lookup(..., tiled=True)``."""
    lib = L.load()
    if f1.dtype not in (torch.float16, torch.bfloat16) or f1.dtype != f2.dtype or f1.dim() != 4:
        raise L.MacvoHipError("corr_volume_out16: [B, H, W, C] float16 / bfloat16 feature maps")
    f1, f2 = _req(f1, f1.dtype, "f1"), _req(f2, f2.dtype, "f2")
    B, H1, W1, Cc = f1.shape
    _, H2, W2, _ = f2.shape
    N1, N2 = H1 * W1, H2 * W2
    dt = _DT[f1.dtype]
    if tiled:                                                             # slices of mv_tiled_slice_cells(H2, W2) cells: a padded last tile row when H2 % 4 != 0
        N2 = lib.mv_tiled_slice_cells(H2, W2)
        if N2 == 0:
            return None
    if not lib.mv_corr_volume_out16_supported(B, Cc, N1, N2, dt, L.MV_LAYOUT_HWC):
        return None
    if out is None:
        out = torch.empty((B * N1, 1, N2 // W2, W2), dtype=f1.dtype, device=f1.device)
    if tiled:
        f2 = fmap_tile_rows16(f2, out=scratch)
    L.check(lib.mv_corr_volume_out16(f1.data_ptr(), f2.data_ptr(), out.data_ptr(), B, Cc, N1, N2, dt, L.MV_LAYOUT_HWC, _stream()),
            "mv_corr_volume_out16")
    return out


# ------------------------------------------------------------------------------------------- A8 / A2
@dataclass
class FrontendMaps:
    """The planes of IStereoDepth.Output / IMatcher.Output, each ``[1, C, H, W]`` float32 on the GPU.  ``depth_cov`` / ``disparity_cov``
    are None for a depth model without covariance, ``flow_cov`` for a matcher without (``provide_cov``, Frontend.py:137-139)."""
    depth: torch.Tensor
    depth_cov: torch.Tensor | None
    disparity: torch.Tensor
    disparity_cov: torch.Tensor | None
    bad_mask: torch.Tensor | None
    flow: torch.Tensor | None
    flow_cov: torch.Tensor | None


def frontend_cov_flags(frontend_cov) -> "tuple[bool, bool]":
    """``(depth model provides covariance, matcher provides covariance)`` as two bools (``IFrontend.provide_cov``)."""
    d, m = frontend_cov
    return bool(d), bool(m)


def frontend_epilogue(flow: torch.Tensor, cov: torch.Tensor | None, baseline: float, fx: float, cov_is_log: bool = True,
                      enforce_positive_disparity: bool = False, want_match: bool = True, provide_cov=(True, True)) -> FrontendMaps:
    """Network output ``flow, logcov [2,2,H,W]`` -> depth / match records (Frontend.py:183-200, flownet.py:44,
    StereoDepth.py:270-282, Matching.py:28-40) in one launch.  ``baseline``/``fx`` are Python floats exactly as
    ``frame.frame_baseline`` / ``frame.fx`` are in the reference.  ``provide_cov = (depth, match)``: a side without covariance
    (FlowFormerDepth / FlowFormerMatcher) gets no covariance planes (None in the result) and its sample of ``cov`` is not read;
    ``cov`` may be None when neither side has one.  The other planes are the same bits in every form."""
    lib = L.load()
    pd, pm = frontend_cov_flags(provide_cov)
    pm = pm and want_match
    flow = _req(flow, torch.float32, "flow")
    if cov is None:
        if pd or pm:
            raise L.MacvoHipError("frontend_epilogue: cov is None but provide_cov asks for a covariance")
    else:
        cov = _req(cov, torch.float32, "cov")
        assert flow.shape == cov.shape
    assert flow.shape[1] == 2
    assert flow.shape[0] == 2 or (flow.shape[0] == 1 and not want_match), "sample 0 = stereo pair, sample 1 = temporal pair"
    _, _, H, W = flow.shape
    dev = flow.device
    mk = lambda c: torch.empty((1, c, H, W), dtype=torch.float32, device=dev)  # noqa: E731
    disparity, depth = mk(1), mk(1)
    disparity_cov, depth_cov = (mk(1), mk(1)) if pd else (None, None)
    bad = torch.empty((1, 1, H, W), dtype=torch.bool, device=dev) if enforce_positive_disparity else None
    mflow = mk(2) if want_match else None
    mcov = mk(3) if pm else None
    bl_fx = float(baseline) * float(fx)            # python double product, rounded once to fp32 by ctypes
    L.check(lib.mv_frontend_epilogue(flow.data_ptr(), _ptr(cov) if (pd or pm) else None, int(cov_is_log), H, W, bl_fx, bl_fx ** 2,
                                     disparity.data_ptr(), _ptr(disparity_cov), depth.data_ptr(),
                                     _ptr(depth_cov), _ptr(bad), _ptr(mflow), _ptr(mcov), _stream()),
            "mv_frontend_epilogue")
    return FrontendMaps(depth, depth_cov, disparity, disparity_cov, bad, mflow, mcov)


def input_pad(H: int, W: int) -> tuple:
    """``(left, right, top, bottom)``: the centred pad to multiples of 8 that ``FlowFormerCov.inference`` applies to an ``H x W`` frame before its encoders
    and removes from its dense outputs (flownet.py:37-44, ``InputPadder(image1.shape)`` — the public padder's default "sintel" mode; the FlowFormer submodule is
    unpinned in the reference checkout, ``tools/flowformer_host.py`` states the padder).  The rule of ``mv_input_pad``, which the frame driver follows."""
    pad = (C.c_int32 * 4)()
    L.load().mv_input_pad(int(H), int(W), pad)
    return tuple(int(v) for v in pad)


def eighth_shape(H: int, W: int) -> tuple:
    """``(h8, w8)`` of the 1/8-resolution maps of an ``H x W`` frame: ``ceil(H / 8), ceil(W / 8)`` (:func:`input_pad`)."""
    left, right, top, bottom = input_pad(H, W)
    return (H + top + bottom) // 8, (W + left + right) // 8


def unpad_window(H: int, W: int) -> "tuple | None":
    """The ``crop=`` of :func:`convex_upsample` that un-pads the upsampled maps of an ``H x W`` frame; None for a frame without pad."""
    left, right, top, bottom = input_pad(H, W)
    return (top, left, H, W) if (left or right or top or bottom) else None


def convex_upsample(flow8: torch.Tensor, mask: torch.Tensor, mask_scale: float = 1.0, exp2_out: bool = False,
                    crop: "tuple | None" = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """RAFT / FlowFormer ``upsample_flow`` (covhead.py:124-126,133-135): ``[B,2,h,w], [B,576,h,w] -> [B,2,8h,8w]``;
    ``exp2_out`` fuses the ``exp(2 * cov)`` of flownet.py:44.  ``mask`` may be fp32, fp16 or bf16 (the decoder's autocast type in Fast mode);
    the result is the fp32 formula on the widened values.

    ``crop=(y0, x0, H, W)``: only that window of the result, ``[B,2,H,W]`` dense — the bits of ``convex_upsample(...)[..., y0:y0+H, x0:x0+W]`` without the
    padded intermediate and the slice copy (``mv_convex_upsample_crop_m``; the network's ``unpad``, see :func:`unpad_window`).  ``out`` (crop only): a contiguous
    fp32 ``[B,2,H,W]`` tensor to write, at any 4-byte-aligned address."""
    lib = L.load()
    flow8 = _req(flow8, torch.float32, "flow8")
    if mask.dtype not in _DT:
        raise TypeError(f"mask: fp32 / fp16 / bf16 expected, got {mask.dtype}")
    mask = _req(mask, mask.dtype, "mask")       # a 16-bit mask is read as it is (no widened copy) and widened in registers
    B, two, h, w = flow8.shape
    assert two == 2 and mask.shape == (B, 576, h, w)
    if crop is not None:
        y0, x0, H, W = (int(v) for v in crop)
        if not (0 <= y0 and 0 <= x0 and H > 0 and W > 0 and y0 + H <= 8 * h and x0 + W <= 8 * w):
            raise ValueError(f"crop {tuple(crop)} is no window of the {8 * h} x {8 * w} result")
        if out is None:
            out = torch.empty((B, 2, H, W), dtype=torch.float32, device=flow8.device)
        elif out.shape != (B, 2, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != flow8.device:
            raise ValueError("out: a contiguous fp32 [B, 2, H, W] tensor on the inputs' device expected")
        L.check(lib.mv_convex_upsample_crop_m(flow8.data_ptr(), mask.data_ptr(), _DT[mask.dtype], out.data_ptr(), B, h, w, y0, x0, H, W,
                                              float(mask_scale), int(exp2_out), _stream()), "mv_convex_upsample_crop_m")
        return out
    assert out is None, "out= belongs to the crop form"
    out = torch.empty((B, 2, 8 * h, 8 * w), dtype=torch.float32, device=flow8.device)
    L.check(lib.mv_convex_upsample_m(flow8.data_ptr(), mask.data_ptr(), _DT[mask.dtype], out.data_ptr(), B, h, w, float(mask_scale),
                                     int(exp2_out), _stream()), "mv_convex_upsample_m")
    return out


# ------------------------------------------------------------------------------------------- (f)2 cost patch-embed
class PatchEmbedWeights:
    """The three ``Conv2d`` layers of FlowFormer's cost ``PatchEmbed.proj`` (patch_size 8: 1 -> 16 -> 32 -> 64 channels, 6x6, stride 2,
    padding 2) packed once into the fragment order of ``mv_cost_patch_embed`` (16-bit weights, fp32 biases).

    ``operand``: the 16-bit type weights and activations are rounded to — ``"f16"`` (IEEE half: 11 significant bits, the mantissa of the
    TF32 the reference's fp32 configurations run their convolutions in, Frontend.py:275-277, and the type ``MACVO_Fast.yaml:73`` runs this
    encoder in) or ``"bf16"`` (for bf16 encoders).  None: by the dtype of ``w1`` — bf16 weights -> "bf16", fp16 / fp32 weights -> "f16"."""

    def __init__(self, w1, b1, w2, b2, w3, b3, operand: str | None = None):
        lib = L.load()
        if operand is None:
            operand = "bf16" if w1.dtype == torch.bfloat16 else "f16"
        if operand not in ("f16", "bf16"):
            raise L.MacvoHipError(f"PatchEmbedWeights: operand must be 'f16' or 'bf16', got {operand!r}")
        self.operand = operand
        self.operand_type = L.MV_F16 if operand == "f16" else L.MV_BF16
        ts = []
        for t, shp in zip((w1, b1, w2, b2, w3, b3), ((16, 1, 6, 6), (16,), (32, 16, 6, 6), (32,), (64, 32, 6, 6), (64,))):
            if tuple(t.shape) != shp:
                raise L.MacvoHipError(f"PatchEmbedWeights: expected a tensor of shape {shp}, got {tuple(t.shape)}")
            ts.append(_req(t.detach().float(), torch.float32, "patch-embed weight"))
        self.packed = torch.empty(int(lib.mv_patch_embed_packed_bytes()), dtype=torch.uint8, device=ts[0].device)
        L.check(lib.mv_patch_embed_pack(*[t.data_ptr() for t in ts], self.packed.data_ptr(), self.operand_type, _stream()), "mv_patch_embed_pack")
        self._keep = ts

    @classmethod
    def from_proj(cls, proj, operand: str | None = None) -> "PatchEmbedWeights":
        """``proj`` = the ``nn.Sequential(Conv2d, ReLU, Conv2d, ReLU, Conv2d)`` of a FlowFormer ``PatchEmbed`` (patch_size 8)."""
        convs = [m for m in proj if isinstance(m, torch.nn.Conv2d)]
        if len(convs) != 3 or any(c.kernel_size != (6, 6) or c.stride != (2, 2) or c.padding != (2, 2) or c.bias is None for c in convs):
            raise L.MacvoHipError("PatchEmbedWeights.from_proj: expected three Conv2d(k = 6, stride 2, padding 2, bias) layers (patch_size 8)")
        return cls(convs[0].weight, convs[0].bias, convs[1].weight, convs[1].bias, convs[2].weight, convs[2].bias, operand=operand)


def cost_patch_embed_supported(H2: int, W2: int) -> bool:
    return bool(L.load().mv_cost_patch_embed_supported(int(H2), int(W2)))


def cost_patch_embed(cost_maps: torch.Tensor, weights: PatchEmbedWeights, tokens: bool = False, out: torch.Tensor | None = None,
                     out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """``PatchEmbed.proj(F.pad(cost_maps))`` for every slice in one launch: ``cost_maps [S, 1, H2, W2]`` (fp32 as ``corr_volume`` returns it, or the
    16-bit cells of ``corr_volume_out16`` when that type is ``weights.operand``) -> ``[S, 64, H2/8, W2/8]``, or with ``tokens`` the flattened-transposed
    form ``[S, H2/8 * W2/8, 64]``.  Result dtype: ``out_dtype`` / ``out.dtype`` if given, else the input's (what ``Conv2d`` returns) — fp32 or the operand
    type.  16-bit matrix pipe (``weights.operand``) with fp32 accumulation; the two intermediate maps never leave LDS, a 16-bit slice goes to the matrix
    pipe as it is and nothing is widened on either side.  Raises for slice sizes the kernel does not cover (``cost_patch_embed_supported``) and for
    dtype combinations it does not build: callers keep their PyTorch layers for those."""
    lib = L.load()
    op_dtype = torch.float16 if weights.operand == "f16" else torch.bfloat16
    if cost_maps.dtype not in (torch.float32, op_dtype):
        raise L.MacvoHipError(f"cost_patch_embed: cost_maps must be float32 or the operand type {op_dtype}, got {cost_maps.dtype}")
    cost_maps = _req(cost_maps, cost_maps.dtype, "cost_maps")
    S, H2, W2 = cost_maps.shape[0], cost_maps.shape[-2], cost_maps.shape[-1]
    if cost_maps.numel() != S * H2 * W2:
        raise L.MacvoHipError("cost_patch_embed: cost_maps must be [S, 1, H2, W2] (one head)")
    h, w = (H2 + 7) // 8, (W2 + 7) // 8
    shape = (S, h * w, 64) if tokens else (S, 64, h, w)
    if out is not None:
        out_dtype = out.dtype
    elif out_dtype is None:
        out_dtype = cost_maps.dtype
    if out_dtype not in (torch.float32, op_dtype) or (out_dtype != torch.float32 and cost_maps.dtype == torch.float32):
        raise L.MacvoHipError(f"cost_patch_embed: {cost_maps.dtype} slices -> {out_dtype} tokens is not built (operand {op_dtype})")
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=cost_maps.device)
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise L.MacvoHipError(f"cost_patch_embed: out must be a contiguous tensor of shape {shape}")
    L.check(lib.mv_cost_patch_embed_t(cost_maps.data_ptr(), _DT[cost_maps.dtype], weights.packed.data_ptr(), out.data_ptr(), _DT[out_dtype], S, H2, W2,
                                      int(tokens), weights.operand_type, _stream()), "mv_cost_patch_embed_t")
    return out


# ------------------------------------------------------------------------------------------- A10 / A11
class KeypointCandidates:
    """Device-side result of the dense selector stage; ``finish`` applies the reference's CPU randperm, ``finish_device`` the same draw from a
    device-resident generator.  One frame: ``cand`` [H*W], ``count`` / ``stats`` [4].  A lane batch (``kp_gradient`` of ``[lanes, 3, H, W]``): ``cand``
    [lanes, H*W], ``count`` / ``stats`` [lanes, 4]; ``lane(l)`` is the one-frame view that ``n`` / ``candidates_vu`` / ``finish`` work on."""

    def __init__(self, cand: torch.Tensor, count: torch.Tensor, stats: torch.Tensor, W: int):
        self.cand, self.count, self.stats, self.W = cand, count, stats, W
        self._n = None

    @property
    def lanes(self) -> int:
        return 1 if self.cand.dim() == 1 else self.cand.shape[0]

    def lane(self, l: int) -> "KeypointCandidates":
        return self if self.cand.dim() == 1 else KeypointCandidates(self.cand[l], self.count[l], self.stats[l], self.W)

    def _one(self, what: str) -> None:
        if self.cand.dim() != 1:
            raise ValueError(f"KeypointCandidates.{what}: a lane batch; take one lane with lane(l) (or use finish_device)")

    @property
    def n(self) -> int:
        self._one("n")
        if self._n is None:
            self._n = int(self.count[0].item())  # the one host sync of the selector (reference has two)
        return self._n

    def candidates_vu(self) -> torch.Tensor:
        """``torch.nonzero(point_mask)[:, 2:]`` — (v, u) int64, row-major order."""
        lin = self.cand[: self.n].long()
        return torch.stack([lin // self.W, lin % self.W], dim=1)

    def finish(self, numPoint: int, staging: torch.Tensor | None = None, generator: "torch.Generator | None" = None) -> torch.Tensor:
        """``selected[torch.randperm(n)[:numPoint]][..., 2:].roll(1, 1)`` (KeypointSelector.py:331-332,404-405).
        The permutation comes from the global CPU generator exactly as in the reference.  ``staging``: optional pinned
        int64 buffer (>= numPoint) so the H2D copy of the permutation is truly asynchronous."""
        lib = L.load()
        n = self.n
        perm = (torch.randperm(n) if generator is None else torch.randperm(n, generator=generator))[:numPoint]
        n_sel = perm.numel()
        out = torch.empty((n_sel, 2), dtype=torch.int64, device=self.cand.device)
        if n_sel:
            if staging is not None:
                staging[:n_sel].copy_(perm)
                perm = staging[:n_sel]
            perm_d = perm.to(self.cand.device, non_blocking=True)
            L.check(lib.mv_kp_gather(self.cand.data_ptr(), perm_d.data_ptr(), n_sel, self.W, out.data_ptr(), _stream()),
                    "mv_kp_gather")
        return out

    def finish_device(self, numPoint: int, state: torch.Tensor) -> "tuple[torch.Tensor, torch.Tensor]":
        """The same draw and gather without the host (``mv_kp_finish_device_lanes``): ``(rows int64 [lanes, numPoint, 2], n_sel int32 [lanes])`` on the
        device, ``n_sel = min(n, numPoint)`` live rows per lane and zeros behind them.  ``state`` (``mt19937_state``, one generator per lane) is
        advanced in place as ``torch.randperm(n, generator=g)`` advances ``g``; the candidate count is read from device memory: no host sync."""
        lib = L.load()
        lanes = self.lanes
        if (state.dim() != 2 or state.shape != (lanes, lib.mv_randperm_state_words()) or state.dtype != torch.int32 or not state.is_contiguous()
                or state.device != self.cand.device):
            raise ValueError(f"finish_device: state must be the contiguous int32 [{lanes}, state_words] tensor of mt19937_state on the candidates' device")
        if numPoint < 0 or numPoint > lib.mv_randperm_max_head():
            raise ValueError(f"finish_device: numPoint {numPoint} outside 0 .. {lib.mv_randperm_max_head()} (the device draw's permutation head)")
        cap = max(numPoint, 1)      # (numPoint 0 still advances the generators, as torch.randperm(n)[:0] does)
        rows = torch.empty((lanes, cap, 2), dtype=torch.int64, device=self.cand.device)
        n_sel = torch.empty((lanes,), dtype=torch.int32, device=self.cand.device)
        stride = self.cand.shape[-1]
        L.check(lib.mv_kp_finish_device_lanes(state.data_ptr(), self.cand.data_ptr(), stride, self.count.data_ptr(), 4, lanes, numPoint, cap, self.W,
                                              rows.data_ptr(), n_sel.data_ptr(), _stream()), "mv_kp_finish_device_lanes")
        return rows[:, :numPoint], n_sel


# ------------------------------------------------------------------------------------------- RandomSelector / GridSelector
def mt19937_state(seeds, device) -> torch.Tensor:
    """Device-resident generators ``[len(seeds), mv_randperm_state_words()]`` (int32 bit patterns of the uint32 words), each with the bits of
    ``torch.Generator().manual_seed(seed)``: what ``kp_random`` and the device-drawn permutation heads advance."""
    import ctypes as C

    import numpy as np

    lib = L.load()
    W = lib.mv_randperm_state_words()
    st = np.zeros((len(seeds), W), dtype=np.uint32)
    for l, sd in enumerate(seeds):
        L.check(lib.mv_mt19937_seed(C.c_uint64(int(sd) & 0xFFFFFFFFFFFFFFFF), st[l].ctypes.data), "mv_mt19937_seed")
    return torch.from_numpy(st.view(np.int32)).to(device)


def _kp_shape_check(num_point: int, H: int, W: int, mask_width: int) -> None:
    if num_point < 0 or mask_width < 0 or H <= 2 * mask_width or W <= 2 * mask_width:
        raise ValueError(f"keypoint selector: need num_point >= 0 and an image larger than twice mask_width (H={H}, W={W}, mask_width={mask_width})")


def kp_random(state: torch.Tensor, num_point: int, H: int, W: int, mask_width: int) -> torch.Tensor:
    """``RandomSelector.select_point`` (KeypointSelector.py:103-118) of every lane's device-resident generator: int64 ``[lanes, num_point, 2]`` (u, v),
    bit for bit ``torch.randint`` of CPU generators seeded alike (first the rows' v, then their u).  ``state`` (``mt19937_state``) is advanced in place
    by ``2 * num_point`` draws."""
    _kp_shape_check(num_point, H, W, mask_width)
    lib = L.load()
    if state.dim() != 2 or state.shape[1] != lib.mv_randperm_state_words() or state.dtype != torch.int32 or not state.is_contiguous():
        raise ValueError("kp_random: state must be the contiguous int32 [lanes, state_words] tensor of mt19937_state")
    if num_point > lib.mv_kp_random_max_point():
        raise ValueError(f"kp_random: num_point {num_point} > {lib.mv_kp_random_max_point()} (the draw's word buffer)")
    out = torch.empty((state.shape[0], num_point, 2), dtype=torch.int64, device=state.device)
    L.check(lib.mv_kp_random_lanes(state.data_ptr(), state.shape[0], num_point, H, W, mask_width, out.data_ptr(), _stream()), "mv_kp_random_lanes")
    return out


def kp_grid_count(H: int, W: int, mask_width: int, num_point: int) -> int:
    """Rows ``GridSelector.select_point`` returns (KeypointSelector.py:216-247) — possibly MORE than ``num_point``; 0 where the reference raises."""
    return int(L.load().mv_kp_grid_count(H, W, mask_width, num_point))


def kp_grid(H: int, W: int, mask_width: int, num_point: int, device) -> torch.Tensor:
    """``GridSelector.select_point``: int64 ``[kp_grid_count(...), 2]`` (u, v)."""
    n = kp_grid_count(H, W, mask_width, num_point)
    if n <= 0:
        raise ValueError(f"kp_grid: empty grid or a grid step of 0 (H={H}, W={W}, mask_width={mask_width}, num_point={num_point}); the reference raises here")
    out = torch.empty((n, 2), dtype=torch.int64, device=device)
    L.check(L.load().mv_kp_grid(H, W, mask_width, num_point, out.data_ptr(), _stream()), "mv_kp_grid")
    return out


_ws_cache: dict = {}


def _kp_workspace(H: int, W: int, device) -> torch.Tensor:
    # one workspace per (shape, device, STREAM): the kernel needs its counters zero on entry and leaves them zero, so two
    # launches may share a workspace only when they are ordered, i.e. on the same stream
    key = (H, W, str(device), _stream())
    ws = _ws_cache.get(key)
    if ws is None:
        nbytes = L.load().mv_kp_select_workspace_bytes(H, W)
        ws = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=device)   # must start zeroed (see header)
        _ws_cache[key] = ws
    return ws


def kp_select(mode: str, H: int, W: int, flow_cov: torch.Tensor | None = None, depth0: torch.Tensor | None = None,
              depth0_cov: torch.Tensor | None = None, depth1: torch.Tensor | None = None,
              depth1_cov: torch.Tensor | None = None, mask_a: torch.Tensor | None = None,
              mask_b: torch.Tensor | None = None, kernel_size: int = 7, mask_width: int = 32,
              max_depth: float = 0.0, max_depth_cov: float = 0.0, max_match_cov: float = 0.0) -> KeypointCandidates:
    """Dense part of the covariance-aware selectors (KeypointSelector.py:87-97,260-327,362-400)."""
    lib = L.load()
    modes = {"nodepth": L.MV_KP_NODEPTH, "full": L.MV_KP_FULL, "mapping": L.MV_KP_MAPPING}
    dev = None
    ts = {}
    for name, t in (("flow_cov", flow_cov), ("depth0", depth0), ("depth0_cov", depth0_cov), ("depth1", depth1),
                    ("depth1_cov", depth1_cov)):
        if t is not None:
            t = _req(t, torch.float32, name)
            dev = t.device
        ts[name] = t
    ms = {}
    for name, t in (("mask_a", mask_a), ("mask_b", mask_b)):
        if t is not None:
            if t.dtype == torch.bool:
                t = t.contiguous().view(torch.uint8)
            t = _req(t, torch.uint8, name)
        ms[name] = t
    p = L.mvKpSelectParams(H, W, modes[mode], kernel_size, mask_width, max_depth, max_depth_cov, max_match_cov)
    ws = _kp_workspace(H, W, dev)
    cand = torch.empty((H * W,), dtype=torch.int32, device=dev)
    count = torch.empty((4,), dtype=torch.int32, device=dev)
    stats = torch.empty((4,), dtype=torch.float32, device=dev)
    L.check(lib.mv_kp_select(_ptr(ts["flow_cov"]), _ptr(ts["depth0"]), _ptr(ts["depth0_cov"]), _ptr(ts["depth1"]),
                             _ptr(ts["depth1_cov"]), _ptr(ms["mask_a"]), _ptr(ms["mask_b"]), C.byref(p),
                             ws.data_ptr(), ws.numel() * 8, cand.data_ptr(), count.data_ptr(), stats.data_ptr(),
                             _stream()), "mv_kp_select")
    return KeypointCandidates(cand, count, stats, W)


_grad_ws_cache: dict = {}


def kp_gradient(image: torch.Tensor, mask_width: int, grad_std: float, nms_size: "int | None" = None) -> KeypointCandidates:
    """Dense part of ``GradientSelector`` (``nms_size=None``) / ``SparseGradienSelector`` (KeypointSelector.py:121-158, :161-213) on ``imageL[0]``:
    ``image`` fp32 planar ``[3, H, W]`` (one frame) or ``[lanes, 3, H, W]`` (independent frames of one launch).  ``nms_size`` odd 1 .. 15."""
    lib = L.load()
    if image.dim() not in (3, 4) or image.shape[-3] != 3:
        raise ValueError(f"kp_gradient: image must be [3, H, W] or [lanes, 3, H, W], got {tuple(image.shape)}")
    if not isinstance(mask_width, int) or mask_width < 0 or not grad_std > 0:
        raise ValueError(f"kp_gradient: need an int mask_width >= 0 and grad_std > 0 (mask_width={mask_width!r}, grad_std={grad_std!r})")
    if nms_size is not None and (not isinstance(nms_size, int) or nms_size < 1 or nms_size % 2 == 0 or nms_size > 15):
        raise ValueError(f"kp_gradient: nms_size must be odd, 1 .. 15 (the NMS tile's halo), got {nms_size!r}")
    image = _req(image, torch.float32, "image")
    batched = image.dim() == 4
    lanes = image.shape[0] if batched else 1
    if lanes < 1 or lanes > L.MV_MAX_LANES:
        raise ValueError(f"kp_gradient: {lanes} lanes outside 1 .. {L.MV_MAX_LANES}")
    H, W = image.shape[-2:]
    dev = image.device
    key = (H, W, lanes, str(dev), _stream())     # (its content is rewritten by every call: one workspace per stream is enough)
    ws = _grad_ws_cache.get(key)
    if ws is None:
        ws = _grad_ws_cache[key] = torch.empty((lib.mv_kp_gradient_workspace_bytes(H, W) * lanes + 7) // 8, dtype=torch.int64, device=dev)
    p = L.mvKpGradParams(H, W, mask_width, nms_size or 0, float(grad_std))
    cand = torch.empty((lanes, H * W), dtype=torch.int32, device=dev)
    count = torch.empty((lanes, 4), dtype=torch.int32, device=dev)
    stats = torch.empty((lanes, 4), dtype=torch.float32, device=dev)
    L.check(lib.mv_kp_gradient_lanes(image.data_ptr(), C.byref(p), ws.data_ptr(), ws.numel() * 8, cand.data_ptr(), count.data_ptr(), stats.data_ptr(),
                                     lanes, _stream()), "mv_kp_gradient_lanes")
    return KeypointCandidates(cand, count, stats, W) if batched else KeypointCandidates(cand[0], count[0], stats[0], W)


def pose_apply(pose: torch.Tensor, pos_Tc: torch.Tensor, cov_Tc: torch.Tensor):
    """World-frame tables from camera-frame ones and a pose (``mv_pose_apply_lanes``, MACVO.py:273-281): returns
    ``(pos_Tw [N,3] f32, rot [9] f64, cov_Tw [N,3,3] f64)`` — what ``backproject(pose=...)`` / ``match_cov(rot=...)`` produce."""
    lib = L.load()
    pose = _req(pose.reshape(7), torch.float32, "pose")
    pos_Tc = _req(pos_Tc, torch.float32, "pos_Tc")
    cov_Tc = _req(cov_Tc, torch.float64, "cov_Tc")
    n = pos_Tc.shape[0]
    dev = pos_Tc.device
    pos_Tw = torch.empty_like(pos_Tc)
    rot = torch.empty(9, dtype=torch.float64, device=dev)
    cov_Tw = torch.empty_like(cov_Tc)
    cnt = (C.c_int32 * 1)(n)
    L.check(lib.mv_pose_apply_lanes(pose.data_ptr(), pos_Tc.data_ptr(), cov_Tc.data_ptr(), 1, cnt, n, pos_Tw.data_ptr(),
                                    rot.data_ptr(), cov_Tw.data_ptr(), _stream()), "mv_pose_apply_lanes")
    return pos_Tw, rot, cov_Tw


def frontend_epilogue_select(flow: torch.Tensor, cov: torch.Tensor, baseline: float, fx: float, cov_is_log: bool = True,
                             enforce_positive_disparity: bool = False, kernel_size: int = 7, mask_width: int = 32,
                             max_match_cov: float = 0.0, mask_a: torch.Tensor | None = None,
                             mask_b: torch.Tensor | None = None) -> "tuple[FrontendMaps, KeypointCandidates]":
    """``frontend_epilogue`` followed by ``kp_select("nodepth", ...)`` in one launch less (``mv_frontend_epilogue_select_lanes``):
    the selector's first kernel derives the quality map from the network's covariance planes itself and writes the epilogue's
    maps on the way.  Bit-identical to the two calls (``test_gpu_backend::test_fused_epilogue_selector_is_bitwise_the_two_calls``)."""
    lib = L.load()
    flow = _req(flow, torch.float32, "flow")
    cov = _req(cov, torch.float32, "cov")
    assert flow.shape == cov.shape and flow.shape[0] == 2 and flow.shape[1] == 2
    _, _, H, W = flow.shape
    dev = flow.device
    mk = lambda c: torch.empty((1, c, H, W), dtype=torch.float32, device=dev)  # noqa: E731
    disparity, disparity_cov, depth, depth_cov, mflow, mcov = mk(1), mk(1), mk(1), mk(1), mk(2), mk(3)
    bad = torch.empty((1, 1, H, W), dtype=torch.bool, device=dev) if enforce_positive_disparity else None
    ms = []
    for name, t in (("mask_a", mask_a), ("mask_b", mask_b)):
        if t is not None:
            if t.dtype == torch.bool:
                t = t.contiguous().view(torch.uint8)
            t = _req(t, torch.uint8, name)
        ms.append(t)
    p = L.mvKpSelectParams(H, W, L.MV_KP_NODEPTH, kernel_size, mask_width, 0.0, 0.0, max_match_cov)
    ws = _kp_workspace(H, W, dev)
    cand = torch.empty((H * W,), dtype=torch.int32, device=dev)
    count = torch.empty((4,), dtype=torch.int32, device=dev)
    stats = torch.empty((4,), dtype=torch.float32, device=dev)
    bl_fx = float(baseline) * float(fx)
    L.check(lib.mv_frontend_epilogue_select_lanes(flow.data_ptr(), cov.data_ptr(), int(cov_is_log), bl_fx, bl_fx ** 2,
                                                  disparity.data_ptr(), disparity_cov.data_ptr(), depth.data_ptr(),
                                                  depth_cov.data_ptr(), _ptr(bad), mflow.data_ptr(), mcov.data_ptr(),
                                                  _ptr(ms[0]), _ptr(ms[1]), C.byref(p), ws.data_ptr(), ws.numel() * 8,
                                                  cand.data_ptr(), count.data_ptr(), stats.data_ptr(), 1, _stream()),
            "mv_frontend_epilogue_select_lanes")
    return FrontendMaps(depth, depth_cov, disparity, disparity_cov, bad, mflow, mcov), KeypointCandidates(cand, count, stats, W)


# ------------------------------------------------------------------------------------------- A12
@dataclass
class TrackedKeypoints:
    kp0_uv: torch.Tensor      # [N,2] float32 (kp0 as float)
    kp1_uv: torch.Tensor      # [N,2] float32
    inbound: torch.Tensor     # [N] bool
    vals: torch.Tensor        # [11,N] float32 rows: d0 disp0 sdisp0 sdd0 d1 disp1 sdisp1 sdd1 suu svv suv
    sigma0: torch.Tensor      # [N,3] float32 default sigma of kp0
    sigma1: torch.Tensor      # [N,3] float32 match covariance (read at kp0)


def kp_track(kp0_uv: torch.Tensor, flow: torch.Tensor, flow_cov: torch.Tensor | None, depth0: FrontendMaps | dict,
             depth1: FrontendMaps | dict, edge: int, match_cov_default: float = 0.25) -> TrackedKeypoints:
    """kp1 = kp0 + flow[kp0], strict border test, and all per-keypoint gathers (MACVO.py:198-232) in one launch."""
    lib = L.load()
    kp0_uv = _req(kp0_uv, torch.int64, "kp0_uv")
    flow = _req(flow, torch.float32, "flow")
    _, _, H, W = flow.shape
    N = kp0_uv.shape[0]
    dev = flow.device

    def g(d, k):
        v = d[k] if isinstance(d, dict) else getattr(d, k)
        return None if v is None else _req(v, torch.float32, k)

    d0 = [g(depth0, k) for k in ("depth", "disparity", "disparity_cov", "depth_cov")]
    d1 = [g(depth1, k) for k in ("depth", "disparity", "disparity_cov", "depth_cov")]
    fc = None if flow_cov is None else _req(flow_cov, torch.float32, "flow_cov")
    kp0f = torch.empty((N, 2), dtype=torch.float32, device=dev)
    kp1 = torch.empty((N, 2), dtype=torch.float32, device=dev)
    inb = torch.empty((N,), dtype=torch.bool, device=dev)
    vals = torch.empty((11, N), dtype=torch.float32, device=dev)
    s0 = torch.empty((N, 3), dtype=torch.float32, device=dev)
    s1 = torch.empty((N, 3), dtype=torch.float32, device=dev)
    L.check(lib.mv_kp_track(kp0_uv.data_ptr(), N, flow.data_ptr(), _ptr(fc), *[_ptr(t) for t in d0],
                            *[_ptr(t) for t in d1], H, W, edge, match_cov_default, kp0f.data_ptr(), kp1.data_ptr(),
                            inb.data_ptr(), vals.data_ptr(), s0.data_ptr(), s1.data_ptr(), _stream()), "mv_kp_track")
    return TrackedKeypoints(kp0f, kp1, inb, vals, s0, s1)


# ------------------------------------------------------------------------------------------- A13-A16
def match_cov(depth_map: torch.Tensor, kp_uv: torch.Tensor, flow_cov: torch.Tensor, depth_cov: torch.Tensor | None,
              fx: float, fy: float, cx: float, cy: float, kernel_size: int = 31, min_flow_cov: float = 0.25,
              min_depth_cov: float = 0.05, use_patch_var: bool = True, rot: torch.Tensor | None = None,
              want_stats: bool = False):
    """MAC-VO covariance model (Project2to3.py:124-181,377-433; Math.py:43-63).  ``flow_cov [N,3]`` is clamped IN
    PLACE like the reference.  Returns ``cov [N,3,3] float64`` (GPU) and, if ``rot [3,3] float64`` is given,
    ``R cov R^T`` (MACVO.py:273-281)."""
    return obs_cov("match", depth_map, kp_uv, flow_cov, depth_cov, fx, fy, cx, cy, None, (), kernel_size, min_flow_cov, min_depth_cov, use_patch_var,
                   rot, want_stats)


def match_cov_pair(depth0: torch.Tensor, kp0_uv: torch.Tensor, sigma0: torch.Tensor, depth1: torch.Tensor,
                   kp1_uv: torch.Tensor, sigma1: torch.Tensor, fx: float, fy: float, cx: float, cy: float,
                   rot: torch.Tensor | None = None, kernel_size: int = 31, min_flow_cov: float = 0.25,
                   min_depth_cov: float = 0.05):
    """Both covariance-model calls of a frame (MACVO.py:241-242) in one launch -> (cov0, cov0_world | None, cov1)."""
    return obs_cov_pair("match", depth0, kp0_uv, sigma0, depth1, kp1_uv, sigma1, fx, fy, cx, cy, None, None, (), rot, kernel_size, min_flow_cov,
                        min_depth_cov)


COV_MODELS = {"match": L.MV_COV_MATCH, "gmm": L.MV_COV_GMM, "none": L.MV_COV_NONE}
COV_MODIFIERS = {"diag": L.MV_COVMOD_DIAG, "normalize": L.MV_COVMOD_NORMALIZE}


def cov_modifier_chain(modifiers) -> int:
    """``("diag", "normalize", ...)`` (innermost first, at most 4) -> the packed int32 chain of ``mv_obs_cov``."""
    mods = tuple(modifiers)
    if not mods:   # (the common case, on the per-frame path of HotPath)
        return 0
    if len(mods) > 4:
        raise ValueError(f"at most 4 covariance modifiers, got {mods}")
    chain = 0
    for i, m in enumerate(mods):
        if m not in COV_MODIFIERS:
            raise ValueError(f"unknown covariance modifier {m!r} (one of {sorted(COV_MODIFIERS)})")
        chain |= COV_MODIFIERS[m] << (4 * i)
    return chain


def _cov_model(model: str) -> int:
    if model not in COV_MODELS:
        raise ValueError(f"unknown covariance model {model!r} (one of {sorted(COV_MODELS)})")
    return COV_MODELS[model]


def obs_cov(model: str, depth_map: torch.Tensor, kp_uv: torch.Tensor, flow_cov: torch.Tensor, depth_cov: torch.Tensor | None,
            fx: float, fy: float, cx: float, cy: float, depth_cov_map: torch.Tensor | None = None, modifiers=(),
            kernel_size: int = 31, min_flow_cov: float = 0.25, min_depth_cov: float = 0.05, use_patch_var: bool = True,
            rot: torch.Tensor | None = None, want_stats: bool = False):
    """The observation-covariance models of ``ICovariance2to3`` (Project2to3.py): ``model`` "match" (MatchCovariance = :func:`match_cov`),
    "gmm" (GaussianMixtureCovariance: needs ``depth_cov_map`` = ``depth_est.cov``) or "none" (NoCovariance), followed by the modifier
    chain ``modifiers`` ("diag" = Modifier_Diagonalize, "normalize" = Modifier_Normalize; innermost first) on the camera-frame
    covariance.  ``flow_cov [N,3]`` is clamped IN PLACE by "match" / "gmm", left as it is by "none".  Returns like :func:`match_cov`."""
    lib = L.load()
    m, chain = _cov_model(model), cov_modifier_chain(modifiers)
    depth_map = _req(depth_map, torch.float32, "depth_map")
    H, W = depth_map.shape[-2:]
    if kp_uv.dtype != torch.float32:
        kp_uv = kp_uv.to(torch.float32)
    kp_uv = _req(kp_uv, torch.float32, "kp_uv")
    if flow_cov.dtype != torch.float32 or not flow_cov.is_contiguous() or not flow_cov.is_cuda:
        raise L.MacvoHipError("obs_cov: flow_cov must be a contiguous float32 GPU tensor (it is clamped in place)")
    if m == L.MV_COV_GMM and depth_cov_map is None:
        raise L.MacvoHipError("obs_cov: the gaussian-mixture model needs depth_cov_map (depth_est.cov)")
    N = kp_uv.shape[0]
    dev = depth_map.device
    dcm = None if depth_cov_map is None else _req(depth_cov_map, torch.float32, "depth_cov_map")
    dc = None if depth_cov is None else _req(depth_cov, torch.float32, "depth_cov")
    r = None if rot is None else _req(rot.to(dev), torch.float64, "rot")
    out = torch.empty((N, 3, 3), dtype=torch.float64, device=dev)
    out_rot = torch.empty((N, 3, 3), dtype=torch.float64, device=dev) if r is not None else None
    stats = torch.empty((N, 2), dtype=torch.float32, device=dev) if want_stats else None
    p = L.mvMatchCovParams(H, W, kernel_size, int(use_patch_var or dc is None), fx, fy, cx, cy, min_flow_cov ** 2,
                           min_depth_cov)
    L.check(lib.mv_obs_cov(m, chain, depth_map.data_ptr(), _ptr(dcm), kp_uv.data_ptr(), flow_cov.data_ptr(), _ptr(dc), _ptr(r),
                           C.byref(p), N, out.data_ptr(), _ptr(out_rot), _ptr(stats), _stream()), "mv_obs_cov")
    res = (out,)
    if out_rot is not None:
        res += (out_rot,)
    if want_stats:
        res += (stats,)
    return res[0] if len(res) == 1 else res


def obs_cov_pair(model: str, depth0: torch.Tensor, kp0_uv: torch.Tensor, sigma0: torch.Tensor, depth1: torch.Tensor,
                 kp1_uv: torch.Tensor, sigma1: torch.Tensor | None, fx: float, fy: float, cx: float, cy: float,
                 depth_cov_map0: torch.Tensor | None = None, depth_cov_map1: torch.Tensor | None = None, modifiers=(),
                 rot: torch.Tensor | None = None, kernel_size: int = 31, min_flow_cov: float = 0.25, min_depth_cov: float = 0.05,
                 n_live: "list[int] | None" = None, no_match_cov: bool = False, match_cov_default: float = 0.25,
                 depth_cov1: torch.Tensor | None = None):
    """Both ObsCovModel calls of a frame (MACVO.py:241-242) with the model / modifiers of :func:`obs_cov`, one launch
    (``mv_obs_cov_pair_lanes``).  Lane-batched when the inputs carry a leading lane axis: depth ``[L, H, W]``, keypoint
    tables ``[L, cap, .]`` and ``n_live`` (default: ``cap`` rows per lane); ``rot`` is then ``[L, 3, 3]``.
    ``no_match_cov`` — the matcher gives no covariance (``mv_obs_cov_pair_nomatch_lanes``): the second call is the model with
    ``flow_cov=None``, i.e. sigma ``(c, c, 0)`` with ``c = match_cov_default`` (the MODEL's own), unclamped, and the depth variance
    ``depth_cov1 [.., cap]`` (the depth-variance map gathered at kp1: ``tracked.vals[7]``) where the depth model has one, the patch
    statistic where it is None; ``sigma1`` is neither read nor written.
    -> (cov0, cov0_world | None, cov1)."""
    lib = L.load()
    m, chain = _cov_model(model), cov_modifier_chain(modifiers)
    d0, d1 = _req(depth0, torch.float32, "depth0"), _req(depth1, torch.float32, "depth1")
    k0, k1 = _req(kp0_uv, torch.float32, "kp0_uv"), _req(kp1_uv, torch.float32, "kp1_uv")
    for t_, nm in ((sigma0, "sigma0"),) + (() if no_match_cov else ((sigma1, "sigma1"),)):
        if t_.dtype != torch.float32 or not t_.is_contiguous() or not t_.is_cuda:
            raise L.MacvoHipError(f"obs_cov_pair: {nm} must be a contiguous float32 GPU tensor (clamped in place)")
    if m == L.MV_COV_GMM and (depth_cov_map0 is None or depth_cov_map1 is None):
        raise L.MacvoHipError("obs_cov_pair: the gaussian-mixture model needs both depth_cov_map0 and depth_cov_map1")
    H, W = d0.shape[-2:]
    lanes = k0.shape[0] if k0.dim() == 3 else 1
    cap = k0.shape[-2]
    assert k1.shape == k0.shape
    n_live = [cap] * lanes if n_live is None else [int(n) for n in n_live]
    dev = d0.device
    dcm0 = None if depth_cov_map0 is None else _req(depth_cov_map0, torch.float32, "depth_cov_map0")
    dcm1 = None if depth_cov_map1 is None else _req(depth_cov_map1, torch.float32, "depth_cov_map1")
    r = None if rot is None else _req(rot.to(dev), torch.float64, "rot")
    lead = (lanes, cap) if k0.dim() == 3 else (cap,)
    c0 = torch.empty(lead + (3, 3), dtype=torch.float64, device=dev)
    c1 = torch.empty(lead + (3, 3), dtype=torch.float64, device=dev)
    c0w = torch.empty(lead + (3, 3), dtype=torch.float64, device=dev) if r is not None else None
    p = L.mvMatchCovParams(H, W, kernel_size, 1, fx, fy, cx, cy, min_flow_cov ** 2, min_depth_cov)
    nl = (C.c_int32 * lanes)(*n_live)
    if no_match_cov:
        if m == L.MV_COV_GMM and depth_cov1 is None:
            raise L.MacvoHipError("obs_cov_pair: the gaussian-mixture model without match covariance needs depth_cov1 (the depth model's variance at kp1)")
        dc1 = None if depth_cov1 is None else _req(depth_cov1, torch.float32, "depth_cov1")
        assert dc1 is None or dc1.shape == k1.shape[:-1]
        L.check(lib.mv_obs_cov_pair_nomatch_lanes(m, chain, d0.data_ptr(), _ptr(dcm0), k0.data_ptr(), sigma0.data_ptr(), _ptr(r), c0.data_ptr(),
                                                  _ptr(c0w), d1.data_ptr(), _ptr(dcm1), k1.data_ptr(), _ptr(dc1), float(match_cov_default),
                                                  c1.data_ptr(), C.byref(p), lanes, nl, cap, _stream()), "mv_obs_cov_pair_nomatch_lanes")
        return c0, c0w, c1
    L.check(lib.mv_obs_cov_pair_lanes(m, chain, d0.data_ptr(), _ptr(dcm0), k0.data_ptr(), sigma0.data_ptr(), _ptr(r), c0.data_ptr(),
                                      _ptr(c0w), d1.data_ptr(), _ptr(dcm1), k1.data_ptr(), sigma1.data_ptr(), c1.data_ptr(), C.byref(p),
                                      lanes, nl, cap, _stream()), "mv_obs_cov_pair_lanes")
    return c0, c0w, c1


# ------------------------------------------------------------------------------------------- A17-A22
def lm_default_params() -> L.mvLMParams:
    p = L.mvLMParams()
    L.load().mv_lm_default_params(C.byref(p))
    return p


@dataclass
class PGOBatch:
    """Concatenated per-point arrays of ``nprob`` independent two-frame problems (all GPU tensors)."""
    offsets: torch.Tensor            # [nprob+1] int32
    init_pose: torch.Tensor          # [nprob,7] float32
    intrinsics: torch.Tensor         # [nprob,4] float32 (fx fy cx cy)
    baseline: torch.Tensor           # [nprob] float32
    pos_Tw: torch.Tensor             # [Ntot,3] float32
    pixel2_uv: torch.Tensor          # [Ntot,2] float32
    cov_Tw: torch.Tensor | None = None           # [Ntot,3,3] float64 (icp)
    pixel2_d: torch.Tensor | None = None         # [Ntot] float32 (icp)
    pixel2_disp: torch.Tensor | None = None      # [Ntot] float32 (disp)
    pixel2_disp_cov: torch.Tensor | None = None  # [Ntot] float32 (disp)
    pixel2_uv_cov: torch.Tensor | None = None    # [Ntot,3] float32 (reproj/disp)
    obs2_covTc: torch.Tensor | None = None       # [Ntot,3,3] float64 (icp)
    valid: torch.Tensor | None = None            # [Ntot] bool/uint8: rows to use (None = all)


_GRAPH = {"icp": L.MV_GRAPH_ICP, "reproj": L.MV_GRAPH_REPROJ, "disp": L.MV_GRAPH_DISP}


def pgo_solve(batch: PGOBatch, graph_type: str = "disp", params: L.mvLMParams | None = None, min_points: int = 0,
              out_pose_f32: torch.Tensor | None = None, ref_pose: torch.Tensor | None = None):
    """Batched two-frame PGO (Optimizer.py:81-102 + PyposeOptimizers.py:160-194) -> (pose [nprob,7] f64, info [nprob,4] f64).
    ``out_pose_f32`` (optional ``[nprob,7]`` float32 GPU tensor) receives ``motion.float()`` (Optimizer.py:104-108).
    ``ref_pose`` (``[nprob,7]`` float32, T_o2w): the ``Local_TwoFrame_PGO`` form (Optimizer.py:111-150) — the solve runs in that pose's frame, the
    returned fp64 pose is the local-frame LM result and ``out_pose_f32`` the world pose ``NormalizeQuat(ref_pose @ result)``."""
    lib = L.load()
    p = params or lm_default_params()
    nprob = batch.init_pose.shape[0]
    dev = batch.init_pose.device
    keep = []   # (contiguous copies stay alive until the launch is enqueued)

    def f32(t, n, dt=torch.float32):
        if t is not None:
            keep.append(_req(t, dt, n))
            return keep[-1]

    f64 = lambda t, n: f32(t, n, torch.float64)  # noqa: E731
    out_pose = torch.empty((nprob, 7), dtype=torch.float64, device=dev)
    out_info = torch.empty((nprob, 4), dtype=torch.float64, device=dev)
    head = [nprob, _req(batch.offsets, torch.int32, "offsets").data_ptr(), _GRAPH[graph_type], f32(batch.init_pose, "init_pose").data_ptr()]
    tail = [f32(batch.intrinsics, "intrinsics").data_ptr(),
            f32(batch.baseline, "baseline").data_ptr(), f32(batch.pos_Tw, "pos_Tw").data_ptr(),
            _ptr(f64(batch.cov_Tw, "cov_Tw")), f32(batch.pixel2_uv, "pixel2_uv").data_ptr(),
            _ptr(f32(batch.pixel2_d, "pixel2_d")), _ptr(f32(batch.pixel2_disp, "pixel2_disp")),
            _ptr(f32(batch.pixel2_disp_cov, "pixel2_disp_cov")),
            _ptr(f32(batch.pixel2_uv_cov, "pixel2_uv_cov")), _ptr(f64(batch.obs2_covTc, "obs2_covTc")),
            _ptr(f32(_u8(batch.valid), "valid", torch.uint8)), int(min_points), C.byref(p), out_pose.data_ptr(),
            out_info.data_ptr(), _ptr(out_pose_f32), _stream()]
    if ref_pose is None:
        L.check(lib.mv_pgo_solve(*head, *tail), "mv_pgo_solve")
    else:
        ref = f32(ref_pose, "ref_pose")
        assert ref.shape == (nprob, 7), ref.shape
        L.check(lib.mv_pgo_solve_local(*head, ref.data_ptr(), *tail), "mv_pgo_solve_local")
    return out_pose, out_info


# ------------------------------------------------------------------------------------------- A12 tail / X1
def backproject(kp_uv: torch.Tensor, depth_vals: torch.Tensor, K4: tuple, pose: torch.Tensor | None,
                want_rot: bool = False):
    """``pixel2point_NED`` (Point.py:15-17) + ``prev_pose.Act`` + ``rotation().matrix().double()`` (MACVO.py:240,273-281).
    ``depth_vals`` may be a strided column view (e.g. ``tracked.vals[:, 0]``).  Returns (pos_Tc, pos_Tw | None, rot | None)."""
    lib = L.load()
    if kp_uv.dtype != torch.float32:
        kp_uv = kp_uv.to(torch.float32)
    kp_uv = _req(kp_uv, torch.float32, "kp_uv")
    assert depth_vals.dtype == torch.float32 and depth_vals.is_cuda and depth_vals.dim() == 1
    stride = depth_vals.stride(0) if depth_vals.numel() > 1 else 1
    N = kp_uv.shape[0]
    dev = kp_uv.device
    pos_Tc = torch.empty((N, 3), dtype=torch.float32, device=dev)
    pos_Tw = torch.empty((N, 3), dtype=torch.float32, device=dev) if pose is not None else None
    rot = torch.empty((3, 3), dtype=torch.float64, device=dev) if (want_rot and pose is not None) else None
    pose_c = None if pose is None else _req(pose.reshape(-1), torch.float32, "pose")
    L.check(lib.mv_backproject(kp_uv.data_ptr(), depth_vals.data_ptr(), int(stride), *[float(k) for k in K4],
                               _ptr(pose_c), N, pos_Tc.data_ptr(), _ptr(pos_Tw), _ptr(rot), _stream()), "mv_backproject")
    return pos_Tc, pos_Tw, rot


@dataclass
class MapPoints:
    """Dense map points of one frame (MACVO.py:313-337): camera-frame covariance is UNROTATED, as the reference stores it."""
    uv: torch.Tensor            # [N,2] float32 (integer-valued pixel coordinates)
    depth: torch.Tensor         # [N]
    sigma_dd: torch.Tensor      # [N]  depth variance at the pixel
    pos_Tc: torch.Tensor        # [N,3]
    pos_Tw: torch.Tensor        # [N,3]
    cov_Tc: torch.Tensor        # [N,3,3] float64
    color: torch.Tensor | None  # [N,3] uint8


def map_points(uv: torch.Tensor, depth: torch.Tensor, depth_cov: torch.Tensor, K4: tuple, pose: torch.Tensor,
               image: torch.Tensor | None = None, match_cov_default: float = 0.25, kernel_size: int = 31,
               min_flow_cov: float = 0.25, min_depth_cov: float = 0.05, cov_model: str = "match", cov_modifiers=()) -> MapPoints:
    """Everything ``run_pair`` does for the dense map after the selector (MACVO.py:317-334) in two launches.  ``cov_model`` /
    ``cov_modifiers``: the ObsCovModel of :func:`obs_cov` (MACVO.py:324 uses the same model as the keypoints)."""
    lib = L.load()
    uv = _req(uv, torch.int64, "uv")
    depth = _req(depth, torch.float32, "depth")
    depth_cov = _req(depth_cov, torch.float32, "depth_cov")
    H, W = depth.shape[-2:]
    N, dev = uv.shape[0], depth.device
    img = None if image is None else _req(image.reshape(3, H, W), torch.float32, "image")
    f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)  # noqa: E731
    uvf, d, sdd, sig, Tc, Tw = f(N, 2), f(N), f(N), f(N, 3), f(N, 3), f(N, 3)
    col = torch.empty((N, 3), dtype=torch.uint8, device=dev) if img is not None else None
    pose_c = _req(pose.reshape(-1), torch.float32, "pose")
    L.check(lib.mv_map_points(uv.data_ptr(), N, depth.data_ptr(), depth_cov.data_ptr(), _ptr(img), H, W,
                              *[float(k) for k in K4], pose_c.data_ptr(), float(match_cov_default), uvf.data_ptr(),
                              d.data_ptr(), sdd.data_ptr(), sig.data_ptr(), Tc.data_ptr(), Tw.data_ptr(), _ptr(col), _stream()),
            "mv_map_points")
    cov = obs_cov(cov_model, depth, uvf, sig, sdd, *K4, depth_cov_map=depth_cov, modifiers=cov_modifiers, kernel_size=kernel_size,
                  min_flow_cov=min_flow_cov, min_depth_cov=min_depth_cov)
    return MapPoints(uvf, d, sdd, Tc, Tw, cov, col)


FILTER_COV_SANITY, FILTER_SIMPLE_DEPTH, FILTER_FRONT_OF_CAM = 1, 2, 4


def obs_filter(inbound: torch.Tensor | None, cov1: torch.Tensor | None, cov2: torch.Tensor | None,
               vals: torch.Tensor | None, flags: int = FILTER_COV_SANITY, min_depth: float = 0.0,
               max_depth: float = 0.0):
    """Fused observation filters (OutlierFilter.py:91-137) -> (valid [N] bool, count [1] int32), both on the GPU."""
    lib = L.load()
    sizes = [t.shape[0] for t in (inbound, cov1, cov2) if t is not None] + ([vals.shape[1]] if vals is not None else [])
    if not sizes or any(n != sizes[0] for n in sizes):
        raise L.MacvoHipError(f"obs_filter: inbound [N], cov1/cov2 [N,3,3] and vals [11,N] must agree on N (got {sizes})")
    N = sizes[0]
    dev = next(t for t in (inbound, cov1, cov2, vals) if t is not None).device
    valid = torch.empty((N,), dtype=torch.bool, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    c1 = None if cov1 is None else _req(cov1, torch.float64, "cov1")
    c2 = None if cov2 is None else _req(cov2, torch.float64, "cov2")
    vv = None if vals is None else _req(vals, torch.float32, "vals")
    L.check(lib.mv_obs_filter(_ptr(_u8(inbound)), _ptr(c1), _ptr(c2), _ptr(vv), flags, min_depth, max_depth, N,
                              valid.data_ptr(), count.data_ptr(), _stream()), "mv_obs_filter")
    return valid, count


# ---------------------------------------------------------------------------------------------- TartanMotionNet motion prior
MOTION_IN_SHAPE = (5, 112, 160)                                   # the PoseNet input of one frame (StereoVO_Interface.py:179)
POSE_NORM = (0.13, 0.13, 0.13, 0.013, 0.013, 0.013)               # TartanStereoVONetInterface.pose_norm (StereoVO_Interface.py:51-53)
_pose_norm_dev: dict = {}


def pose_norm(device) -> torch.Tensor:
    """``pose_norm`` as the fp32 device tensor the reference multiplies with (cached per device)."""
    dev = torch.device(device)
    t = _pose_norm_dev.get(dev)
    if t is None:
        t = _pose_norm_dev[dev] = torch.tensor(POSE_NORM, dtype=torch.float32, device=dev)
    return t


def motion_input(flow: torch.Tensor, depth: torch.Tensor, fx: float, fy: float, cx: float, cy: float, baseline: float,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """TartanStereoVOMotion.inference's PoseNet input (StereoVO_Interface.py:177-188) in one launch (``mv_motion_input_lanes``):
    temporal flow ``[2,H,W]`` / ``[1,2,H,W]`` or per lane ``[L,2,H,W]`` and depth ``[H,W]`` / ``[1,1,H,W]`` / ``[L,1,H,W]`` / ``[L,H,W]``
    -> ``[L,5,112,160]`` fp32.  ``fx, fy, cx, cy, baseline`` are the frame's Python floats (``meta.fx``, ``meta.frame_baseline``...);
    the intrinsic layer keeps the reference's swapped (height, width) arguments."""
    lib = L.load()
    flow = _req(flow, torch.float32, "flow")
    depth = _req(depth, torch.float32, "depth")
    H, W = flow.shape[-2:]
    if flow.shape[-3] != 2 or depth.shape[-2:] != (H, W):
        raise L.MacvoHipError(f"motion_input: flow [.,2,H,W] and depth [.,H,W] must agree (got {tuple(flow.shape)}, {tuple(depth.shape)})")
    lanes = flow.numel() // (2 * H * W)
    if depth.numel() != lanes * H * W:
        raise L.MacvoHipError(f"motion_input: {lanes} flow lanes but {depth.numel() // (H * W)} depth planes")
    if H < MOTION_IN_SHAPE[1] or W < MOTION_IN_SHAPE[2]:
        raise L.MacvoHipError(f"motion_input: a {H}x{W} frame does not cover the {MOTION_IN_SHAPE[1]}x{MOTION_IN_SHAPE[2]} PoseNet input")
    if out is None:
        out = torch.empty((lanes,) + MOTION_IN_SHAPE, dtype=torch.float32, device=flow.device)
    else:
        assert out.shape == (lanes,) + MOTION_IN_SHAPE and out.dtype == torch.float32 and out.is_contiguous()
    bl_fx = float(baseline) * float(fx)            # the reference's Python double product, rounded once to fp32 by ctypes
    L.check(lib.mv_motion_input_lanes(lanes, H, W, flow.data_ptr(), 2 * H * W, depth.data_ptr(), H * W, fx, fy, cx, cy, bl_fx,
                                      out.data_ptr(), _stream()), "mv_motion_input_lanes")
    return out


def pose_exp_compose(prev: torch.Tensor, raw: torch.Tensor, norm: torch.Tensor | None = None,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """``prev @ pp.se3(raw * pose_norm).Exp()`` in fp32 (MotionModel.py:112, StereoVO_Interface.py:194): ``prev [n,7]`` or ``[7]``, raw
    PoseNet output ``[n,6]`` or ``[6]`` -> ``[n,7]`` (``[7]`` for a single pose)."""
    lib = L.load()
    single = prev.dim() == 1
    prev = _req(prev.reshape(-1, 7), torch.float32, "prev")
    raw = _req(raw.reshape(-1, 6), torch.float32, "raw")
    n = prev.shape[0]
    if raw.shape[0] != n:
        raise L.MacvoHipError(f"pose_exp_compose: {n} poses but {raw.shape[0]} motions")
    nrm = pose_norm(prev.device) if norm is None else _req(norm.reshape(6), torch.float32, "norm")
    if out is None:
        out = torch.empty((n, 7), dtype=torch.float32, device=prev.device)
    L.check(lib.mv_pose_exp_compose(n, prev.data_ptr(), raw.data_ptr(), 6, nrm.data_ptr(), out.data_ptr(), _stream()),
            "mv_pose_exp_compose")
    return out.reshape(7) if single else out


# ---------------------------------------------------------------------------------------------- the PoseNet of TartanMotionNet
POSENET_STAGES = ("firstconv", "layer1", "layer2", "layer3", "layer4", "layer5")
POSENET_STAGE_SHAPES = ((32, 56, 80), (64, 28, 40), (128, 14, 20), (128, 7, 10), (256, 4, 5), (256, 2, 3))     # per lane, NCHW
_POSENET_PREFIXES = ("module.flowPoseNet.", "flowPoseNet.")       # the release checkpoint (a DataParallel StereoVONet), or its bare module


def posenet_tensor_table() -> "list[tuple[str, tuple[int, ...]]]":
    """(state-dict key, shape) of the PoseNet's 120 tensors in canonical order, as the library lists them."""
    lib = L.load()
    table = []
    name, shape, ndim = C.create_string_buffer(64), (C.c_int32 * 4)(), C.c_int32()
    for i in range(lib.mv_posenet_tensor_count()):
        L.check(lib.mv_posenet_tensor_info(i, name, shape, C.byref(ndim)), "mv_posenet_tensor_info")
        table.append((name.value.decode(), tuple(shape[d] for d in range(ndim.value))))
    return table


class PoseNet:
    """TartanVO's PoseNet (``VOFlowRes`` config 1, stereo, as ``StereoVONet.flowPoseNet``) forward in HIP: a callable
    ``[lanes,5,112,160] fp32 -> [lanes,6]`` raw motion (before ``pose_norm``) on the current torch stream — what ``HotPath``,
    ``NativeHotPath`` and ``HIP_TartanMotionNet`` take as ``pose_net``.  The weights are packed on the host and uploaded once at
    construction; a call allocates only its output and its workspace (torch's caching allocator), copies nothing from the host and
    does not synchronise.  ``net(x, return_stages=True)`` also returns the six stage outputs (firstconv, layer1..5), NCHW."""

    def __init__(self, state_dict, device="cuda"):
        lib = L.load()
        self.device = torch.device(device)
        tensors = []
        for key, shape in posenet_tensor_table():
            if key not in state_dict:
                raise L.MacvoHipError(f"PoseNet: the state dict has no tensor '{key}'")
            t = state_dict[key]
            if tuple(t.shape) != shape:
                raise L.MacvoHipError(f"PoseNet: tensor '{key}' has shape {tuple(t.shape)}, expected {shape}")
            tensors.append(t.detach().to("cpu", torch.float32).contiguous())
        ptrs = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        nbytes = lib.mv_posenet_packed_bytes()
        packed = torch.empty((nbytes // 4,), dtype=torch.float32)
        L.check(lib.mv_posenet_pack(ptrs, packed.data_ptr()), "mv_posenet_pack")
        self.packed = packed.to(self.device)

    @classmethod
    def from_state_dict(cls, state_dict, device="cuda") -> "PoseNet":
        """Bare keys (``firstconv.0.0.weight`` ...) or the release checkpoint's (``module.flowPoseNet.`` / ``flowPoseNet.`` prefixes; the
        ``flowNet`` / ``stereoNet`` tensors beside them are ignored)."""
        for prefix in _POSENET_PREFIXES:
            if any(k.startswith(prefix) for k in state_dict):
                state_dict = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
                break
        return cls(state_dict, device)

    @classmethod
    def from_file(cls, path: str, device="cuda") -> "PoseNet":
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd and not any(torch.is_tensor(v) for v in sd.values()):
            sd = sd["state_dict"]
        return cls.from_state_dict(sd, device)

    @classmethod
    def from_module(cls, module: "torch.nn.Module", device="cuda") -> "PoseNet":
        return cls.from_state_dict(module.state_dict(), device)

    def __call__(self, x: torch.Tensor, return_stages: bool = False):
        lib = L.load()
        x = _req(x, torch.float32, "x")
        if x.dim() != 4 or tuple(x.shape[1:]) != MOTION_IN_SHAPE or x.device != self.packed.device:
            raise L.MacvoHipError(f"PoseNet: x must be [lanes,5,112,160] fp32 on {self.packed.device} (got {tuple(x.shape)} on {x.device})")
        lanes = x.shape[0]
        nws = lib.mv_posenet_workspace_bytes(lanes)
        if nws == 0:
            raise L.MacvoHipError(f"PoseNet: {lanes} lanes are not supported (1 <= lanes <= {L.MV_MAX_LANES})")
        ws = torch.empty((nws // 4,), dtype=torch.float32, device=x.device)
        out = torch.empty((lanes, 6), dtype=torch.float32, device=x.device)
        stages, sp = None, None
        if return_stages:
            stages = [torch.empty((lanes,) + s, dtype=torch.float32, device=x.device) for s in POSENET_STAGE_SHAPES]
            sp = (C.c_void_p * 6)(*[s.data_ptr() for s in stages])
        L.check(lib.mv_posenet_forward_lanes(self.packed.data_ptr(), x.data_ptr(), lanes, out.data_ptr(), ws.data_ptr(), sp, _stream()),
                "mv_posenet_forward_lanes")
        return (out, stages) if return_stages else out


# ---------------------------------------------------------------------------------- the decoder's recurrent update blocks
UPDATE_KINDS = {"cov": L.MV_UPDATE_COV, "flow": L.MV_UPDATE_FLOW}
_UPDATE_OPERANDS = {"f16": (L.MV_F16, torch.float16), "bf16": (L.MV_BF16, torch.bfloat16)}


def _update_kind(kind) -> int:
    k = UPDATE_KINDS.get(kind, kind) if isinstance(kind, str) else kind
    if k not in (L.MV_UPDATE_COV, L.MV_UPDATE_FLOW):
        raise L.MacvoHipError(f"update block: kind must be 'cov' or 'flow', got {kind!r}")
    return int(k)


def update_block_tensor_table(kind) -> "list[tuple[str, tuple[int, ...]]]":
    """(state-dict key, shape) of the block's tensors in the module's order, as the library lists them: ``"cov"`` = ``CovUpdateBlock`` (24 tensors),
    ``"flow"`` = the ``gru`` / ``flow_head`` / ``mask`` members of FlowFormer's ``GMAUpdateBlock`` (20)."""
    lib, k = L.load(), _update_kind(kind)
    table = []
    name, shape, ndim = C.create_string_buffer(64), (C.c_int32 * 4)(), C.c_int32()
    for i in range(lib.mv_update_block_tensor_count(k)):
        L.check(lib.mv_update_block_tensor_info(k, i, name, shape, C.byref(ndim)), "mv_update_block_tensor_info")
        table.append((name.value.decode(), tuple(shape[d] for d in range(ndim.value))))
    return table


class UpdateBlockWeights:
    """The weights of one recurrent update block of the FlowFormerCov decoder, packed once into the fragment order of ``mv_update_block_forward``
    (16-bit weights in ``operand``, fp32 biases holding 16-bit values).  ``operand``: ``"bf16"`` / ``"f16"``; None: bf16 for bf16 tensors, f16 for fp16
    and fp32 ones.  A missing or mis-shaped tensor is named in the error, before anything touches the device."""

    def __init__(self, state_dict, kind, operand: str | None = None, device=None):
        lib = L.load()
        self.kind = _update_kind(kind)
        table = update_block_tensor_table(self.kind)
        tensors = []
        for key, shape in table:
            if key not in state_dict:
                raise L.MacvoHipError(f"UpdateBlockWeights: the state dict has no tensor '{key}'")
            t = state_dict[key]
            if tuple(t.shape) != shape:
                raise L.MacvoHipError(f"UpdateBlockWeights: tensor '{key}' has shape {tuple(t.shape)}, expected {shape}")
            tensors.append(t)
        if operand is None:
            operand = "bf16" if tensors[0].dtype == torch.bfloat16 else "f16"
        if operand not in _UPDATE_OPERANDS:
            raise L.MacvoHipError(f"UpdateBlockWeights: operand must be 'f16' or 'bf16', got {operand!r}")
        self.operand = operand
        self.operand_type, self.dtype = _UPDATE_OPERANDS[operand]
        device = torch.device(device) if device is not None else tensors[0].device
        ts = [_req(t.detach().to(device, torch.float32), torch.float32, "update-block weight") for t in tensors]
        with torch.cuda.device(device):
            self.packed = torch.empty(int(lib.mv_update_block_packed_bytes(self.kind, self.operand_type)), dtype=torch.uint8, device=device)
            ptrs = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            L.check(lib.mv_update_block_pack(self.kind, self.operand_type, ptrs, self.packed.data_ptr(), _stream()), "mv_update_block_pack")
        self._keep = ts          # (the pack kernels read them on the stream)

    @classmethod
    def from_module(cls, block, kind, operand: str | None = None, device=None) -> "UpdateBlockWeights":
        """``block``: a ``CovUpdateBlock`` (kind "cov"), a ``GMAUpdateBlock`` or any module / state dict that holds its ``gru.*``, ``flow_head.*`` and
        ``mask.*`` tensors (kind "flow"); other entries (``encoder.*``, ``aggregator.*``) are ignored."""
        sd = block if isinstance(block, dict) else block.state_dict()
        return cls(sd, kind, operand, device)


def update_block(net: torch.Tensor, inp: torch.Tensor, weights: UpdateBlockWeights, workspace: torch.Tensor | None = None):
    """One iteration of a recurrent update block: ``net [B,128,H,W]``, ``inp [B,384,H,W]`` in ``weights.dtype`` (NCHW, or both channels-last) ->
    ``(net, delta [B,2,H,W], mask [B,576,H,W])``, NCHW-contiguous, in that dtype.  Kind "cov" is ``CovUpdateBlock.forward`` (covhead.py:39-43, mask
    already scaled by 0.25); kind "flow" is covhead.py:112-114 (mask unscaled).  fp32 accumulation, one rounding per stored tensor; allocates the
    outputs and — unless ``workspace`` (uint8, at least ``mv_update_block_workspace_bytes``; its contents do not matter) is handed in — a workspace from
    torch's caching allocator, copies nothing from the host, does not synchronise."""
    lib = L.load()
    for t, c, name in ((net, 128, "net"), (inp, 384, "inp")):
        if not t.is_cuda or t.dtype != weights.dtype or t.dim() != 4 or t.shape[1] != c:
            raise L.MacvoHipError(f"update_block: {name} must be a [B,{c},H,W] {weights.dtype} GPU tensor (got {tuple(t.shape)} {t.dtype} on {t.device})")
    if net.shape[0] != inp.shape[0] or net.shape[2:] != inp.shape[2:] or net.device != weights.packed.device or inp.device != net.device:
        raise L.MacvoHipError(f"update_block: net {tuple(net.shape)} on {net.device} and inp {tuple(inp.shape)} on {inp.device} do not belong together")
    B, _, H, W = net.shape
    nws = lib.mv_update_block_workspace_bytes(weights.kind, B, H, W)
    if nws == 0:
        raise L.MacvoHipError(f"update_block: B x H x W = {B} x {H} x {W} is out of range (1 <= B * H * W <= 2^20)")
    cl = torch.channels_last
    channels_last = all(t.is_contiguous(memory_format=cl) and not t.is_contiguous() for t in (net, inp))
    if not channels_last:
        net, inp = net.contiguous(), inp.contiguous()
    if workspace is None:
        workspace = torch.empty((nws,), dtype=torch.uint8, device=net.device)
    elif workspace.dtype != torch.uint8 or workspace.device != net.device or not workspace.is_contiguous() or workspace.numel() < nws or workspace.data_ptr() % 16:
        raise L.MacvoHipError(f"update_block: workspace must be a contiguous, 16-byte aligned uint8 tensor of at least {nws} bytes on {net.device}")
    ws = workspace
    net_out = torch.empty((B, 128, H, W), dtype=weights.dtype, device=net.device)
    delta = torch.empty((B, 2, H, W), dtype=weights.dtype, device=net.device)
    mask = torch.empty((B, 576, H, W), dtype=weights.dtype, device=net.device)
    L.check(lib.mv_update_block_forward(weights.kind, weights.operand_type, weights.packed.data_ptr(), net.data_ptr(), inp.data_ptr(), B, H, W,
                                        int(channels_last), net_out.data_ptr(), delta.data_ptr(), mask.data_ptr(), ws.data_ptr(), _stream()),
            "mv_update_block_forward")
    return net_out, delta, mask


# ---------------------------------------------------------------------------------------------- the decoder's motion encoder
def motion_encoder_tensor_table() -> "list[tuple[str, tuple[int, ...]]]":
    """(state-dict key, shape) of the motion encoder's 10 tensors in the module's order (``convc1.weight`` ... ``conv.bias``), as the library lists them."""
    lib = L.load()
    table = []
    name, shape, ndim = C.create_string_buffer(64), (C.c_int32 * 4)(), C.c_int32()
    for i in range(lib.mv_motion_encoder_tensor_count()):
        L.check(lib.mv_motion_encoder_tensor_info(i, name, shape, C.byref(ndim)), "mv_motion_encoder_tensor_info")
        table.append((name.value.decode(), tuple(shape[d] for d in range(ndim.value))))
    return table


class MotionEncoderWeights:
    """The weights of the FlowFormerCov decoder's motion encoder (``GMAUpdateBlock.encoder``), packed once into the fragment order of
    ``mv_motion_encoder_forward`` (16-bit weights in ``operand``, fp32 biases holding 16-bit values; ``convc1`` and ``convf1`` zero-padded to whole
    64-channel chunks).  ``operand``: ``"bf16"`` / ``"f16"``; None: bf16 for bf16 tensors, f16 for fp16 and fp32 ones.  A missing or mis-shaped tensor is
    named in the error, before anything touches the device."""

    def __init__(self, state_dict, operand: str | None = None, device=None):
        lib = L.load()
        tensors = []
        for key, shape in motion_encoder_tensor_table():
            if key not in state_dict:
                raise L.MacvoHipError(f"MotionEncoderWeights: the state dict has no tensor '{key}'")
            t = state_dict[key]
            if tuple(t.shape) != shape:
                raise L.MacvoHipError(f"MotionEncoderWeights: tensor '{key}' has shape {tuple(t.shape)}, expected {shape}")
            tensors.append(t)
        if operand is None:
            operand = "bf16" if tensors[0].dtype == torch.bfloat16 else "f16"
        if operand not in _UPDATE_OPERANDS:
            raise L.MacvoHipError(f"MotionEncoderWeights: operand must be 'f16' or 'bf16', got {operand!r}")
        self.operand = operand
        self.operand_type, self.dtype = _UPDATE_OPERANDS[operand]
        device = torch.device(device) if device is not None else tensors[0].device
        ts = [_req(t.detach().to(device, torch.float32), torch.float32, "motion-encoder weight") for t in tensors]
        with torch.cuda.device(device):
            self.packed = torch.empty(int(lib.mv_motion_encoder_packed_bytes(self.operand_type)), dtype=torch.uint8, device=device)
            ptrs = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            L.check(lib.mv_motion_encoder_pack(self.operand_type, ptrs, self.packed.data_ptr(), _stream()), "mv_motion_encoder_pack")
        self._keep = ts          # (the pack kernels read them on the stream)

    @classmethod
    def from_module(cls, encoder, operand: str | None = None, device=None) -> "MotionEncoderWeights":
        """``encoder``: the ``MotionEncoder`` module, or any state dict that holds its ten tensors; other entries are ignored."""
        sd = encoder if isinstance(encoder, dict) else encoder.state_dict()
        return cls(sd, operand, device)


def motion_encoder(flow: torch.Tensor, corr: torch.Tensor, weights: MotionEncoderWeights, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """``MotionEncoder.forward(flow, corr)`` (covhead.py:106): ``flow [B,2,H,W]``, ``corr [B,145,H,W]`` in ``weights.dtype`` (``corr`` NCHW or
    channels-last, read as it lies; ``flow`` is brought to ``corr``'s layout when it has the other one, a copy of two channels) -> ``[B,128,H,W]``, NCHW-contiguous, in that dtype: channels 0..125 the features, 126..127 ``flow`` bit for bit.  fp32 accumulation, one
    rounding per stored tensor; allocates the output and — unless ``workspace`` (uint8, at least ``mv_motion_encoder_workspace_bytes``; its contents do
    not matter) is handed in — a workspace from torch's caching allocator, copies nothing from the host, does not synchronise."""
    lib = L.load()
    for t, c, name in ((flow, 2, "flow"), (corr, 145, "corr")):
        if not t.is_cuda or t.dtype != weights.dtype or t.dim() != 4 or t.shape[1] != c:
            raise L.MacvoHipError(f"motion_encoder: {name} must be a [B,{c},H,W] {weights.dtype} GPU tensor (got {tuple(t.shape)} {t.dtype} on {t.device})")
    if flow.shape[0] != corr.shape[0] or flow.shape[2:] != corr.shape[2:] or flow.device != weights.packed.device or corr.device != flow.device:
        raise L.MacvoHipError(f"motion_encoder: flow {tuple(flow.shape)} on {flow.device} and corr {tuple(corr.shape)} on {corr.device} do not belong together")
    B, _, H, W = flow.shape
    nws = lib.mv_motion_encoder_workspace_bytes(B, H, W)
    if nws == 0:
        raise L.MacvoHipError(f"motion_encoder: B x H x W = {B} x {H} x {W} is out of range (1 <= B * H * W <= 2^20)")
    cl = torch.channels_last
    # corr decides the layout and is read where it lies (a copy only when it is neither NCHW-contiguous nor channels-last); the two-channel flow follows it
    channels_last = corr.is_contiguous(memory_format=cl) and not corr.is_contiguous()
    if channels_last:
        flow = flow.contiguous(memory_format=cl)
    else:
        flow, corr = flow.contiguous(), corr.contiguous()
    if workspace is None:
        workspace = torch.empty((nws,), dtype=torch.uint8, device=flow.device)
    elif workspace.dtype != torch.uint8 or workspace.device != flow.device or not workspace.is_contiguous() or workspace.numel() < nws or workspace.data_ptr() % 16:
        raise L.MacvoHipError(f"motion_encoder: workspace must be a contiguous, 16-byte aligned uint8 tensor of at least {nws} bytes on {flow.device}")
    out = torch.empty((B, 128, H, W), dtype=weights.dtype, device=flow.device)
    with torch.cuda.device(flow.device):
        L.check(lib.mv_motion_encoder_forward(weights.operand_type, weights.packed.data_ptr(), flow.data_ptr(), corr.data_ptr(), B, H, W, int(channels_last),
                                              out.data_ptr(), workspace.data_ptr(), _stream()), "mv_motion_encoder_forward")
    return out


# ------------------------------------------------------------------------------------------- frontend evaluation
@dataclass
class EvalResult:
    """What ``eval_flow`` / ``eval_depth`` leave on the device: ``row`` = this call's ``[lanes, COLS]`` view of the table ``rows``
    (columns: ``_lib.EVAL_FLOW_COLS`` / ``EVAL_DEPTH_COLS``), the recorder grid(s) and the optional per-pixel planes.  Nothing here is a
    Python number: reading one is the caller's synchronisation."""
    row: torch.Tensor
    rows: torch.Tensor
    grids: torch.Tensor | None
    err: torch.Tensor | None
    nll: torch.Tensor | None


def _eval_workspace(lanes: int, H: int, W: int, device) -> torch.Tensor:
    # the kernels zero what they need per call, so launches may share a workspace when they are ordered: one per stream
    key = ("eval", lanes, H, W, str(device), _stream())
    ws = _ws_cache.get(key)
    if ws is None:
        nbytes = L.load().mv_eval_workspace_bytes(lanes, H, W)
        if nbytes == 0:
            raise L.MacvoHipError(f"eval: {lanes} lanes of {H}x{W} are not supported (lanes <= {L.MV_MAX_LANES}, H * W <= 2^22)")
        ws = _ws_cache[key] = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)
    return ws


def _eval_lanes(t: torch.Tensor, planes: int, name: str) -> torch.Tensor:
    """``[planes,H,W]`` or ``[L,planes,H,W]`` (``planes = 0``: ``[H,W]``, ``[L,H,W]`` or ``[L,1,H,W]``) -> contiguous fp32 ``[L,planes or 1,H,W]``."""
    t = _req(t, torch.float32, name)
    if planes == 0:
        if t.dim() == 4 and t.shape[1] != 1:
            raise L.MacvoHipError(f"{name}: expected [L,1,H,W], got {tuple(t.shape)}")
        if t.dim() not in (2, 3, 4):
            raise L.MacvoHipError(f"{name}: expected [H,W], [L,H,W] or [L,1,H,W], got {tuple(t.shape)}")
        return t.reshape(-1, 1, t.shape[-2], t.shape[-1]) if t.dim() != 2 else t.reshape(1, 1, *t.shape)
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[1] < planes:
        raise L.MacvoHipError(f"{name}: expected [L,{planes},H,W], got {tuple(t.shape)}")
    return t


def _eval_tables(kind: str, lanes: int, ncols: int, ngrids: int, rows, row: int, grids, has_cov: bool, device):
    if rows is None:
        rows = torch.full((lanes, row + 1, ncols), float("nan"), dtype=torch.float32, device=device)
    if (rows.dim() != 3 or rows.shape[0] != lanes or rows.shape[2] != ncols or rows.dtype != torch.float32 or not rows.is_cuda
            or not rows.is_contiguous()):
        raise L.MacvoHipError(f"{kind}: rows must be a contiguous fp32 GPU tensor [{lanes}, n_rows, {ncols}]")
    if not 0 <= row < rows.shape[1]:
        raise L.MacvoHipError(f"{kind}: row {row} outside a table of {rows.shape[1]} rows")
    if has_cov:
        shape = (lanes, ngrids, L.EVAL_GRID, L.EVAL_GRID) if ngrids > 1 else (lanes, L.EVAL_GRID, L.EVAL_GRID)
        if grids is None:
            grids = torch.zeros(shape, dtype=torch.int32, device=device)
        if tuple(grids.shape) != shape or grids.dtype not in (torch.int32, torch.uint32) or not grids.is_cuda or not grids.is_contiguous():
            raise L.MacvoHipError(f"{kind}: grids must be a contiguous int32 GPU tensor {shape} (it accumulates: zero it once per sequence)")
    elif grids is not None:
        raise L.MacvoHipError(f"{kind}: grids need a covariance")
    return rows, grids


def eval_flow(est_flow: torch.Tensor, gt_flow: torch.Tensor, est_cov: torch.Tensor | None = None, valid: torch.Tensor | None = None,
              max_flow: float = 128.0, apply_max_flow: bool = True, rows: torch.Tensor | None = None, row: int = 0,
              grids: torch.Tensor | None = None, planes: bool = False) -> EvalResult:
    """One frame per lane of ``evaluate_flow`` / ``evaluate_flowcov`` (EvalFlow.py:29-47, 82-127; ``mv_eval_flow_lanes``).  ``est_flow``, ``gt_flow``:
    ``[2,H,W]`` or ``[L,2,H,W]``; ``est_cov``: ``[L,2 or 3,H,W]`` (planes uu, vv; a third is ignored) or None; ``valid``: bool / uint8 ``[H,W]``, ``[L,H,W]``
    or ``[L,1,H,W]``, nonzero = valid.  ``rows`` (``[L, n_rows, len(EVAL_FLOW_COLS)]``) / ``row`` / ``grids`` (int32 ``[L,2,100,100]``): accumulate on the
    device over a sequence; allocated (grids zeroed) when absent.  ``planes=True`` also returns the per-pixel epe / nll maps."""
    lib = L.load()
    est = _eval_lanes(est_flow, 2, "est_flow")
    gt = _eval_lanes(gt_flow, 2, "gt_flow")
    lanes, _, H, W = est.shape
    if est.shape[1] != 2 or tuple(gt.shape) != tuple(est.shape):
        raise L.MacvoHipError(f"eval_flow: est_flow and gt_flow must both be [L,2,H,W] (got {tuple(est.shape)}, {tuple(gt.shape)})")
    cov = None
    if est_cov is not None:
        cov = _eval_lanes(est_cov, 2, "est_cov")
        if cov.shape[0] != lanes or tuple(cov.shape[2:]) != (H, W):
            raise L.MacvoHipError(f"eval_flow: est_cov {tuple(cov.shape)} does not match the flow {tuple(est.shape)}")
    vm = _u8(valid)
    if vm is not None and vm.numel() != lanes * H * W:
        raise L.MacvoHipError(f"eval_flow: valid has {vm.numel()} elements for {lanes} lanes of {H}x{W}")
    dev = est.device
    rows, grids = _eval_tables("eval_flow", lanes, len(L.EVAL_FLOW_COLS), 2, rows, row, grids, cov is not None, dev)
    epe = torch.empty((lanes, H, W), dtype=torch.float32, device=dev) if planes else None
    nll = torch.empty((lanes, H, W), dtype=torch.float32, device=dev) if planes and cov is not None else None
    ws = _eval_workspace(lanes, H, W, dev)
    n = H * W
    L.check(lib.mv_eval_flow_lanes(lanes, H, W, est.data_ptr(), 2 * n, gt.data_ptr(), 2 * n, _ptr(cov), n, 0 if cov is None else cov.shape[1] * n,
                                   _ptr(vm), n, float(max_flow), int(bool(apply_max_flow)), rows.data_ptr(), rows.shape[1], row, _ptr(grids),
                                   _ptr(epe), _ptr(nll), ws.data_ptr(), ws.numel() * 8, _stream()), "mv_eval_flow_lanes")
    return EvalResult(rows[:, row], rows, grids, epe, nll)


def eval_depth(est_depth: torch.Tensor, gt_depth: torch.Tensor, est_cov: torch.Tensor | None = None, max_depth: float = 80.0,
               rows: torch.Tensor | None = None, row: int = 0, grids: torch.Tensor | None = None, planes: bool = False) -> EvalResult:
    """One frame per lane of ``evaluate_depth`` / ``evaluate_depthcov`` (EvalDepth.py:22-34, 57-82; ``mv_eval_depth_lanes``).  Maps are ``[H,W]``,
    ``[L,H,W]`` or ``[L,1,H,W]``; ``grids``: int32 ``[L,100,100]``.  Otherwise as ``eval_flow``."""
    lib = L.load()
    est = _eval_lanes(est_depth, 0, "est_depth")
    gt = _eval_lanes(gt_depth, 0, "gt_depth")
    lanes, _, H, W = est.shape
    if tuple(gt.shape) != tuple(est.shape):
        raise L.MacvoHipError(f"eval_depth: est_depth {tuple(est.shape)} and gt_depth {tuple(gt.shape)} differ")
    cov = None
    if est_cov is not None:
        cov = _eval_lanes(est_cov, 0, "est_cov")
        if tuple(cov.shape) != tuple(est.shape):
            raise L.MacvoHipError(f"eval_depth: est_cov {tuple(cov.shape)} does not match the depth {tuple(est.shape)}")
    dev = est.device
    rows, grids = _eval_tables("eval_depth", lanes, len(L.EVAL_DEPTH_COLS), 1, rows, row, grids, cov is not None, dev)
    err = torch.empty((lanes, H, W), dtype=torch.float32, device=dev) if planes else None
    nll = torch.empty((lanes, H, W), dtype=torch.float32, device=dev) if planes and cov is not None else None
    ws = _eval_workspace(lanes, H, W, dev)
    n = H * W
    L.check(lib.mv_eval_depth_lanes(lanes, H, W, est.data_ptr(), n, gt.data_ptr(), n, _ptr(cov), n, float(max_depth), rows.data_ptr(), rows.shape[1],
                                    row, _ptr(grids), _ptr(err), _ptr(nll), ws.data_ptr(), ws.numel() * 8, _stream()), "mv_eval_depth_lanes")
    return EvalResult(rows[:, row], rows, grids, err, nll)


# ------------------------------------------------------------------------------------------- trajectory evaluation (MetricsSeq.py / EvalSeq.py)
@dataclass
class TrajEvalResult:
    """``rows``: fp64 ``[L, len(EVAL_TRAJ_COLS)]`` on the device (``_lib.EVAL_TRAJ_COLS`` names the columns; ``status`` is ``_lib.MV_TRAJ_*``);
    ``errors``: fp64 ``[L, 4, T_max]`` (ATE_i, then RTE_i / ROE_i / RPE_i; NaN where a lane has no value) or None; ``lengths``: the host-side T per lane."""
    rows: torch.Tensor
    errors: torch.Tensor | None
    lengths: list
    assoc_status: torch.Tensor | None = None      # int32 [L] of the association launch (``eval_trajectory`` with stamps), else None

    def column(self, name: str) -> torch.Tensor:
        return self.rows[:, L.EVAL_TRAJ_COLS.index(name)]


def _traj_side(tracks, name: str):
    """One side of ``eval_trajectory`` -> (tensors kept alive, dtype code, row stride in elements, lengths).  A track is read IN PLACE when it is a
    GPU tensor ``[T, >= 7]`` of fp32 / fp64 with unit column stride and every lane of the side shares dtype and row stride; otherwise the side is
    made contiguous on the device (a copy on the current stream: no synchronisation)."""
    if isinstance(tracks, torch.Tensor):
        if tracks.dim() == 2:
            tracks = [tracks]
        elif tracks.dim() == 3:
            tracks = list(tracks.unbind(0))
        else:
            raise L.MacvoHipError(f"{name}: expected [T,7], [L,T,7] or a list of [T,7] tracks, got {tuple(tracks.shape)}")
    tracks = list(tracks)
    for t in tracks:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise L.MacvoHipError(f"{name}: expected GPU tensors (the HIP hot path has no CPU fallback)")
        if t.dim() != 2 or t.shape[1] < 7:
            raise L.MacvoHipError(f"{name}: a track is [T,7] rows (tx ty tz qx qy qz qw), got {tuple(t.shape)}")
        if t.dtype not in (torch.float32, torch.float64):
            raise L.MacvoHipError(f"{name}: fp32 or fp64 tracks, got {t.dtype}")
    if len({t.dtype for t in tracks}) > 1:
        raise L.MacvoHipError(f"{name}: every lane of one side in the same dtype")
    live = [t for t in tracks if t.shape[0] > 1]
    strides = {t.stride(0) for t in live}
    if any(t.stride(1) != 1 for t in live) or len(strides) > 1 or any(s < 7 for s in strides):
        tracks = [t[:, :7].contiguous() for t in tracks]
        strides = {7}
    return tracks, (L.MV_TRAJ_F64 if tracks and tracks[0].dtype == torch.float64 else L.MV_TRAJ_F32), (strides.pop() if strides else 7), \
        [int(t.shape[0]) for t in tracks]


def eval_trajectory(est, ref, align: str = "umeyama", correct_scale: bool = False, errors: bool = False, est_time=None, ref_time=None,
                    align_time: str | None = None, align_origin: bool = False) -> TrajEvalResult:
    """ATE / RTE / ROE / RPE of every lane's track in one launch (``mv_eval_traj_lanes``; MetricsSeq.py:9-51, EvalSeq.py:53-64 — evo 1.x restated,
    parity-unpinned: evo is not a dependency of this library).  ``est`` / ``ref``: a list of per-lane ``[T_l, 7]`` GPU tensors (fp32 or fp64 per side,
    rows tx ty tz qx qy qz qw, read in place), or one ``[L, T, 7]`` tensor.  The tracks are time-associated: a lane whose estimate and reference
    lengths differ is refused.  ``align``: ``"umeyama"`` (the reference's setting), ``"origin"`` or ``"none"``.  Returns device tensors on the current
    stream; never synchronises.

    With ``est_time`` and ``ref_time`` (per-lane stamps, fp64 or int64) the tracks need not be associated: ``associate_trajectory`` runs first on the same
    stream — what ``Trajectory.from_sandbox`` does before EvalSeq.py:36 scores a track: both clocks rebased, ``align_time`` ``"est->gt"`` (the default
    with stamps; the estimate interpolated at the reference's stamps) or ``"gt->est"``, and with ``align_origin`` the estimate moved onto the
    reference's first pose first (``"est->gt"`` only).  The associated track is handed on in fp64 (the store is exact: no rounding between the two
    launches, where the reference rounds to fp32).  ``assoc_status`` then holds that launch's per-lane status; a lane that is not OK there reaches
    the evaluation as NaN rows and comes out ``NONFINITE``."""
    lib = L.load()
    if align not in L.TRAJ_ALIGN:
        raise L.MacvoHipError(f"eval_trajectory: align must be one of {sorted(L.TRAJ_ALIGN)}, got {align!r}")
    assoc_status = None
    if est_time is not None or ref_time is not None:
        if est_time is None or ref_time is None:
            raise L.MacvoHipError("eval_trajectory: est_time and ref_time come together")
        align_time = "est->gt" if align_time is None else align_time
        if align_time == "est->gt":
            a = associate_trajectory(est, est_time, ref_time, origin_ref=ref if align_origin else None, out_dtype=torch.float64)
            est = a.poses
        elif align_time == "gt->est" and not align_origin:
            a = associate_trajectory(ref, ref_time, est_time, out_dtype=torch.float64)
            ref = a.poses
        else:
            raise L.MacvoHipError(f"eval_trajectory: align_time {align_time!r} with align_origin={align_origin} (\"est->gt\", or \"gt->est\" without align_origin)")
        assoc_status = a.status
    elif align_time is not None or align_origin:
        raise L.MacvoHipError("eval_trajectory: align_time / align_origin need est_time and ref_time")
    e, e_dt, e_st, e_T = _traj_side(est, "est")
    r, r_dt, r_st, r_T = _traj_side(ref, "ref")
    lanes = len(e)
    if not 1 <= lanes <= L.MV_MAX_LANES or len(r) != lanes:
        raise L.MacvoHipError(f"eval_trajectory: {lanes} estimates and {len(r)} references (1 <= lanes <= {L.MV_MAX_LANES}, one reference per estimate)")
    for l, (a, b) in enumerate(zip(e_T, r_T)):
        if a != b:
            raise L.MacvoHipError(f"eval_trajectory: lane {l} has {a} estimated and {b} reference poses (tracks must be time-associated: one estimate row "
                                  "per reference row)")
        if a > L.EVAL_TRAJ_MAX_POSES:
            raise L.MacvoHipError(f"eval_trajectory: lane {l} has {a} poses (at most 2^20)")
    dev = e[0].device
    if any(t.device != dev for t in e + r):
        raise L.MacvoHipError("eval_trajectory: every track on the same device")
    rows = torch.empty((lanes, len(L.EVAL_TRAJ_COLS)), dtype=torch.float64, device=dev)
    t_max = max(max(e_T), 1)
    err = torch.full((lanes, 4, t_max), float("nan"), dtype=torch.float64, device=dev) if errors else None
    ep = (C.c_void_p * lanes)(*[t.data_ptr() if t.shape[0] else None for t in e])
    rp = (C.c_void_p * lanes)(*[t.data_ptr() if t.shape[0] else None for t in r])
    Ts = (C.c_int32 * lanes)(*e_T)
    with torch.cuda.device(dev):
        L.check(lib.mv_eval_traj_lanes(lanes, ep, rp, Ts, e_dt, r_dt, e_st, r_st, L.TRAJ_ALIGN[align], int(bool(correct_scale)), rows.data_ptr(),
                                       _ptr(err), t_max, _stream()), "mv_eval_traj_lanes")
    # (the launch is enqueued; the caching allocator keeps `e` / `r` copies valid for work already on this stream)
    return TrajEvalResult(rows, err, e_T, assoc_status)


# ------------------------------------------------------------------------------------------- trajectory association (Trajectory.from_sandbox)
@dataclass
class TrajAssocResult:
    """Per lane: ``poses`` ``[Q_l, 7]`` (the requested dtype), ``extrapolated`` uint8 ``[Q_l]`` (the reference's ``~interp_mask``); ``status``: int32
    ``[L]`` (``_lib.MV_TRAJ_*``).  Device tensors on the current stream."""
    poses: list
    extrapolated: list
    status: torch.Tensor


def _traj_clock(times, name: str, lanes: int, dev):
    """One clock side of ``associate_trajectory`` -> per-lane contiguous 1-D device tensors (fp64 or int64; anything else is widened to fp64)."""
    if isinstance(times, torch.Tensor):
        times = [times] if times.dim() == 1 else list(times.unbind(0))
    times = list(times)
    if len(times) != lanes:
        raise L.MacvoHipError(f"{name}: {len(times)} clocks for {lanes} lanes")
    out = []
    for t in times:
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise L.MacvoHipError(f"{name}: one 1-D tensor of stamps per lane")
        if t.dtype not in (torch.float64, torch.int64):
            t = t.to(torch.int64) if not t.dtype.is_floating_point else t.to(torch.float64)
        out.append(t.to(dev).contiguous())
    return out


def associate_trajectory(src, src_time, query_time, origin_ref=None, rebase: bool = True, out_dtype=None) -> TrajAssocResult:
    """``Trajectory.from_sandbox``'s association step (Utility/Trajectory.py:105-114) for every lane in one launch (``mv_traj_associate_lanes``):
    the optional origin alignment onto ``origin_ref`` (a reference track or its first row per lane), the rebase of both clocks to their own first stamp,
    and ``interpolate_pose`` (Utility/Math.py:96-121) of ``src`` at ``query_time``.  ``src``: per-lane ``[T_l, >= 7]`` GPU tensors or one stacked tensor,
    handled as ``eval_trajectory`` handles a side; the clocks: per-lane 1-D fp64 or int64 tensors (one dtype per launch: a mixed call is widened to fp64
    unless every clock is int64).  ``out_dtype``: fp32 or fp64, default the source's (as the reference's ``P_container``).  fp64 arithmetic, one
    rounding at the store; PyPose / evo restated, parity-unpinned.  Never synchronises."""
    lib = L.load()
    s, s_dt, s_st, s_T = _traj_side(src, "src")
    lanes = len(s)
    if not 1 <= lanes <= L.MV_MAX_LANES:
        raise L.MacvoHipError(f"associate_trajectory: {lanes} lanes (1 <= lanes <= {L.MV_MAX_LANES})")
    dev = s[0].device
    ts = _traj_clock(src_time, "src_time", lanes, dev)
    tq = _traj_clock(query_time, "query_time", lanes, dev)
    if len({t.dtype for t in ts + tq}) > 1:
        ts, tq = [t.double() for t in ts], [t.double() for t in tq]
    t_dt = L.MV_TRAJ_TIME_I64 if ts[0].dtype == torch.int64 else L.MV_TRAJ_TIME_F64
    Q = [int(t.shape[0]) for t in tq]
    for l in range(lanes):
        if ts[l].shape[0] != s_T[l]:
            raise L.MacvoHipError(f"associate_trajectory: lane {l} has {s_T[l]} poses and {ts[l].shape[0]} stamps")
        if max(s_T[l], Q[l]) > L.EVAL_TRAJ_MAX_POSES:
            raise L.MacvoHipError(f"associate_trajectory: lane {l} has {s_T[l]} poses and {Q[l]} queries (at most 2^20 each)")
    o_dt, org = L.MV_TRAJ_F64, None
    if origin_ref is not None:
        if isinstance(origin_ref, torch.Tensor):                  # one lane's track or first row, or the stacked [L, T, 7] / [L, 7]
            origin_ref = [origin_ref] if origin_ref.dim() == 1 or (origin_ref.dim() == 2 and lanes == 1) else list(origin_ref.unbind(0))
        o, o_dt, _, o_T = _traj_side([r.reshape(1, -1) if isinstance(r, torch.Tensor) and r.dim() == 1 else r for r in origin_ref], "origin_ref")
        if len(o) != lanes or any(n < 1 for n in o_T):
            raise L.MacvoHipError("associate_trajectory: origin_ref needs one reference track (or first row) per lane")
        org = [t[0, :7].contiguous() for t in o]
    if out_dtype is None:
        out_dtype = s[0].dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise L.MacvoHipError(f"associate_trajectory: out_dtype fp32 or fp64, got {out_dtype}")
    poses = [torch.empty((q, 7), dtype=out_dtype, device=dev) for q in Q]
    flags = [torch.empty((q,), dtype=torch.uint8, device=dev) for q in Q]
    status = torch.empty((lanes,), dtype=torch.int32, device=dev)

    def arr(ts_):
        return (C.c_void_p * lanes)(*[t.data_ptr() if t.numel() else None for t in ts_])

    with torch.cuda.device(dev):
        L.check(lib.mv_traj_associate_lanes(lanes, arr(s), arr(ts), (C.c_int32 * lanes)(*s_T), arr(tq), (C.c_int32 * lanes)(*Q),
                                            None if org is None else arr(org), s_dt, t_dt, o_dt, L.MV_TRAJ_F64 if out_dtype == torch.float64 else L.MV_TRAJ_F32,
                                            s_st, int(bool(rebase)), arr(poses), arr(flags), status.data_ptr(), _stream()), "mv_traj_associate_lanes")
    # (the launch is enqueued; the caching allocator keeps the copies made above valid for work already on this stream)
    return TrajAssocResult(poses, flags, status)


# ------------------------------------------------------------------------------------------- frame preprocessing (DataLoader/Transform.py)
class PlanDoesNotFold(L.MacvoHipError):
    """The transform cannot be folded into the plan it was appended to (a second real resize, a second cast to another type): start a new plan."""


_PP_KINDS = {"scale": L.MV_PP_SCALE, "crop": L.MV_PP_CENTER_CROP, "smart": L.MV_PP_SMART_RESIZE, "cast": L.MV_PP_CAST}
_PP_CAST = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
_PP_SRC = {torch.float32: L.MV_F32, torch.float16: L.MV_F16, torch.bfloat16: L.MV_BF16, torch.uint8: L.MV_PP_U8, torch.bool: L.MV_PP_U8}
_PP_TORCH = {L.MV_F32: torch.float32, L.MV_F16: torch.float16, L.MV_BF16: torch.bfloat16}


@dataclass
class PreprocessPlan:
    """What ``mv_preprocess_plan`` made of one transform or of a folded list: ``c`` is the C record the launch takes, ``K`` the intrinsics after the
    list (CPU fp32, ``[3, 3]`` or ``[B, 3, 3]`` as they were given)."""
    c: L.mvPreprocessPlan
    K: torch.Tensor

    @property
    def src_shape(self) -> tuple:
        return self.c.src_h, self.c.src_w

    @property
    def resized(self) -> tuple:
        """The frame the last crop sees: the resized frame, or the source when no resize is folded in (a unit scale is a copy)."""
        return (self.c.rs_h, self.c.rs_w) if self.c.scaled else (self.c.src_h, self.c.src_w)

    @property
    def height(self) -> int:
        return self.c.out_h

    @property
    def width(self) -> int:
        return self.c.out_w

    def _crop(self) -> tuple:
        c = self.c                 # the crops behind the resize — without a resize every crop has moved the window instead
        return (c.out_y0, c.out_x0, c.out_vy0, c.out_vy1, c.out_vx0, c.out_vx1) if c.scaled else (c.win_y0, c.win_x0, c.win_vy0, c.win_vy1, c.win_vx0, c.win_vx1)

    @property
    def origin(self) -> tuple:
        """``(top, left)`` of the crop (0 on an axis that is padded instead)."""
        y0, x0 = self._crop()[:2]
        return max(y0, 0), max(x0, 0)

    @property
    def pads(self) -> tuple:
        """``(top, bottom, left, right)`` zero rows / columns of the output."""
        _, _, vy0, vy1, vx0, vx1 = self._crop()
        return vy0, self.c.out_h - vy1, vx0, self.c.out_w - vx1

    @property
    def round_scale(self) -> tuple:
        """``(round_scale_u, round_scale_v)`` as fp32 values (``gt_flow``'s divisors)."""
        return self.c.round_scale_u, self.c.round_scale_v

    @property
    def out_dtype(self):
        return _PP_TORCH.get(self.c.out_dtype)

    def then(self, kind: str, **args) -> "PreprocessPlan":
        return preprocess_plan(0, 0, kind, prev=self, **args)


def preprocess_plan(H: int, W: int, kind: str, K: torch.Tensor | None = None, prev: "PreprocessPlan | None" = None, *, scale_u=None, scale_v=None,
                    height=None, width=None, interp: str = "nearest", dtype=None) -> PreprocessPlan:
    """``mv_preprocess_plan``: the host arithmetic of one transform of DataLoader/Transform.py on an ``H x W`` frame with intrinsics ``K`` — or, with
    ``prev``, of that transform appended to a plan (``H``, ``W``, ``K`` are then ignored).  ``kind``: ``"scale"`` (``scale_u``, ``scale_v``, ``interp``) =
    ScaleFrame, ``"crop"`` (``height``, ``width``) = CenterCropFrame, ``"smart"`` (``height``, ``width``, ``interp``) = SmartResizeFrame, ``"cast"``
    (``dtype``: "fp32" / "fp16" / "bf16" or the torch type) = CastDataType.  :class:`PlanDoesNotFold` when the transform does not fold into ``prev``."""
    lib = L.load()
    if kind not in _PP_KINDS:
        raise ValueError(f"preprocess_plan: kind {kind!r} is not one of {sorted(_PP_KINDS)}")
    if kind == "scale":
        a0, a1, mode = float(scale_u), float(scale_v), L.PP_INTERP[interp]
    elif kind == "cast":
        dt = _PP_CAST.get(dtype, dtype)
        if dt not in _DT:
            raise ValueError(f"preprocess_plan: cast to {dtype!r} (fp32, fp16 or bf16)")
        a0, a1, mode = 0.0, 0.0, _DT[dt]
    else:
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in (height, width)):
            raise ValueError(f"preprocess_plan: {kind} needs integer height and width, not {height!r}, {width!r}")
        a0, a1, mode = float(height), float(width), L.PP_INTERP[interp]
    if prev is not None:
        Kin = prev.K
    else:
        Kin = torch.eye(3) if K is None else K.detach().to("cpu", torch.float32)
    if Kin.shape[-2:] != (3, 3) or Kin.dim() not in (2, 3):
        raise ValueError(f"preprocess_plan: K must be [3, 3] or [B, 3, 3], not {tuple(Kin.shape)}")
    rows = Kin.reshape(-1, 9).contiguous()
    out_rows, rec = [], None
    for b in range(rows.shape[0]):                     # K goes through the same chain of fp32 operations for every matrix of a batch
        c = L.mvPreprocessPlan()
        kb = (C.c_float * 9)(*rows[b].tolist())
        if prev is not None:
            p = L.mvPreprocessPlan.from_buffer_copy(prev.c)
            p.K = kb
            code = lib.mv_preprocess_plan(C.byref(c), C.byref(p), 0, 0, None, _PP_KINDS[kind], a0, a1, mode)
        else:
            code = lib.mv_preprocess_plan(C.byref(c), None, int(H), int(W), kb, _PP_KINDS[kind], a0, a1, mode)
        if code == -2:
            raise PlanDoesNotFold(f"preprocess_plan: {kind} does not fold into the plan in front of it")
        L.check(code, "mv_preprocess_plan")
        out_rows.append(torch.tensor(list(c.K), dtype=torch.float32))
        rec = rec or c
    return PreprocessPlan(rec, torch.stack(out_rows).reshape(Kin.shape))


@dataclass
class PreprocessedFrame:
    """The planes ``preprocess`` wrote (device tensors ``[B, C, out_h, out_w]`` on the current stream; None where the input was None)."""
    imageL: torch.Tensor
    imageR: torch.Tensor | None = None
    gt_flow: torch.Tensor | None = None
    flow_mask: torch.Tensor | None = None
    gt_depth: torch.Tensor | None = None


def preprocess(plan: PreprocessPlan, imageL: torch.Tensor, imageR: torch.Tensor | None = None, gt_flow: torch.Tensor | None = None,
               flow_mask: torch.Tensor | None = None, gt_depth: torch.Tensor | None = None, out_dtype=None, out: "dict | None" = None) -> PreprocessedFrame:
    """``mv_preprocess_lanes``: every plane of a frame through ``plan`` in ONE launch on the current stream; never synchronises.  Planes are ``[B, C, H, W]``
    GPU tensors of the plan's source size (B = lanes, at most ``MV_MAX_LANES``): images fp32 / fp16 / bf16 or uint8 (widened as ``u8.float() / 255``), ``gt_flow``
    ``[B, 2, H, W]``, ``flow_mask`` ``[B, 1, H, W]`` bool, ``gt_depth`` ``[B, 1, H, W]``; any but ``imageL`` may be None.  ``out_dtype`` (or the plan's
    CastDataType): the type of every plane at the store, rounded once; otherwise a plane keeps its type (uint8 images become fp32, the mask stays bool).
    ``out``: optional ``{name: tensor}`` of contiguous outputs to write (any element-aligned address)."""
    lib = L.load()
    od = _PP_CAST.get(out_dtype, out_dtype) if out_dtype is not None else plan.out_dtype
    if od is not None and od not in _DT:
        raise ValueError(f"preprocess: out_dtype {out_dtype!r} (fp32, fp16 or bf16)")
    H, W = plan.src_shape
    B = imageL.shape[0]
    if not 1 <= B <= L.MV_MAX_LANES:
        raise L.MacvoHipError(f"preprocess: {B} lanes (1 <= lanes <= {L.MV_MAX_LANES})")
    kinds = {"imageL": L.MV_PP_IMAGE, "imageR": L.MV_PP_IMAGE, "gt_flow": L.MV_PP_FLOW, "flow_mask": L.MV_PP_MASK, "gt_depth": L.MV_PP_DEPTH}
    planes = {"imageL": imageL, "imageR": imageR, "gt_flow": gt_flow, "flow_mask": flow_mask, "gt_depth": gt_depth}
    groups, res, keep = [], {}, []
    for name, t in planes.items():
        if t is None:
            res[name] = None
            continue
        if not t.is_cuda:
            raise L.MacvoHipError(f"{name}: expected a GPU tensor (the HIP hot path has no CPU fallback)")
        if t.dim() != 4 or t.shape[0] != B or tuple(t.shape[-2:]) != (H, W) or t.dtype not in _PP_SRC:
            raise L.MacvoHipError(f"preprocess: {name} {tuple(t.shape)} {t.dtype}: expected [{B}, C, {H}, {W}] in fp32, fp16, bf16, uint8 or bool")
        kind, Cn = kinds[name], int(t.shape[1])
        if (kind == L.MV_PP_FLOW and Cn != 2) or (kind in (L.MV_PP_MASK, L.MV_PP_DEPTH) and Cn != 1) or not 1 <= Cn <= 16:
            raise L.MacvoHipError(f"preprocess: {name} has {Cn} planes")
        is_u8 = t.dtype in (torch.uint8, torch.bool)
        if is_u8 and kind not in (L.MV_PP_IMAGE, L.MV_PP_MASK):
            raise L.MacvoHipError(f"preprocess: {name} must be a floating-point plane")
        t = t.contiguous()
        if od is not None:
            dt = od
        elif kind == L.MV_PP_MASK and is_u8:
            dt = torch.bool
        else:
            dt = torch.float32 if is_u8 else t.dtype
        o = None if out is None else out.get(name)
        if o is None:
            o = torch.empty((B, Cn, plan.height, plan.width), dtype=dt, device=t.device)
        elif o.shape != (B, Cn, plan.height, plan.width) or o.dtype != dt or not o.is_contiguous() or o.device != t.device:
            raise ValueError(f"preprocess: out[{name!r}] must be a contiguous {dt} [{B}, {Cn}, {plan.height}, {plan.width}] tensor on the inputs' device")
        g = L.mvPreprocessGroup()
        g.src, g.dst = t.data_ptr(), o.data_ptr()
        g.src_lane_stride, g.dst_lane_stride = Cn * H * W, Cn * plan.height * plan.width
        g.planes, g.kind, g.src_dtype, g.dst_dtype = Cn, kind, _PP_SRC[t.dtype], _PP_SRC[dt]
        groups.append(g)
        keep.append(t)                 # (a contiguous copy made above must outlive the enqueue)
        res[name] = o
    arr = (L.mvPreprocessGroup * len(groups))(*groups)
    with torch.cuda.device(imageL.device):
        L.check(lib.mv_preprocess_lanes(C.byref(plan.c), arr, len(groups), B, _stream()), "mv_preprocess_lanes")
    return PreprocessedFrame(**res)


# ------------------------------------------------------------------------------------------- stereo rectification (DataLoader/Dataset/EuRoC.py, VBR.py)
@dataclass
class RectifyPlan:
    """What ``mv_stereo_rectify_plan`` made of a stereo calibration: ``c`` is the C record (its ``cam`` pair feeds ``rectify_maps``); ``R1``, ``R2`` ``[3, 3]``
    and ``P1``, ``P2`` ``[3, 4]`` are CPU fp64 tensors, ``K`` = ``P1[:3, :3]`` CPU fp32 ``[3, 3]``."""
    c: L.mvRectifyPlan
    R1: torch.Tensor
    R2: torch.Tensor
    P1: torch.Tensor
    P2: torch.Tensor
    K: torch.Tensor

    @property
    def baseline(self) -> float:
        return self.c.baseline

    @property
    def focal(self) -> float:
        return self.c.fc

    @property
    def idx(self) -> int:
        """0: a horizontal rig, 1: a vertical one."""
        return self.c.idx

    @property
    def size(self) -> tuple:
        """``(width, height)``."""
        return self.c.width, self.c.height


def _f64_host(a, n: int, name: str):
    t = torch.as_tensor(a, dtype=torch.float64).detach().to("cpu").reshape(-1)
    if n >= 0 and t.numel() != n:
        raise ValueError(f"stereo_rectify_plan: {name} has {t.numel()} values, expected {n}")
    return (C.c_double * t.numel())(*t.tolist()), t.numel()


def stereo_rectify_plan(K1, D1, K2, D2, size, R, T) -> RectifyPlan:
    """``mv_stereo_rectify_plan``: ``cv2.stereoRectify(K1, D1, K2, D2, size, R, T, flags=CALIB_ZERO_DISPARITY, alpha=-1)`` restated in C doubles on the host
    (EuRoC.py:165-167, VBR.py:175-177); no GPU is touched.  ``K`` ``[3, 3]``, ``D`` 4, 5 or 8 coefficients, ``size`` = ``(width, height)``, ``R`` ``[3, 3]`` and
    ``T`` ``[3]`` from camera 1 to camera 2."""
    lib = L.load()
    k1, _ = _f64_host(K1, 9, "K1")
    k2, _ = _f64_host(K2, 9, "K2")
    d1, n1 = _f64_host(D1, -1, "D1")
    d2, n2 = _f64_host(D2, -1, "D2")
    r, _ = _f64_host(R, 9, "R")
    t, _ = _f64_host(T, 3, "T")
    c = L.mvRectifyPlan()
    L.check(lib.mv_stereo_rectify_plan(C.byref(c), k1, d1, n1, k2, d2, n2, int(size[0]), int(size[1]), r, t), "mv_stereo_rectify_plan")
    f64 = lambda a, shape: torch.tensor(list(a), dtype=torch.float64).reshape(shape)          # noqa: E731
    return RectifyPlan(c, f64(c.R1, (3, 3)), f64(c.R2, (3, 3)), f64(c.P1, (3, 4)), f64(c.P2, (3, 4)), torch.tensor(list(c.K), dtype=torch.float32).reshape(3, 3))


def rectify_maps(plan: "RectifyPlan | list", out_h: int | None = None, out_w: int | None = None, device=None) -> tuple:
    """``mv_rectify_maps``: the ``cv2.initUndistortRectifyMap(..., CV_32FC1)`` pair of every camera of ``plan`` (or of a list of ``mvRectifyCam`` records) in ONE
    launch on the current stream -> ``(map_x, map_y)``, fp32 ``[n_cams, out_h, out_w]`` (default: the plan's image size).  fp64 on the device, rounded once."""
    lib = L.load()
    cams = list(plan.c.cam) if isinstance(plan, RectifyPlan) else list(plan)
    if isinstance(plan, RectifyPlan):
        out_h, out_w = plan.c.height if out_h is None else out_h, plan.c.width if out_w is None else out_w
    if not 1 <= len(cams) <= L.MV_RM_MAX_GROUPS:
        raise L.MacvoHipError(f"rectify_maps: {len(cams)} cameras (1 <= cameras <= {L.MV_RM_MAX_GROUPS})")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise L.MacvoHipError("rectify_maps: expected a GPU device (the HIP hot path has no CPU fallback)")
    mx = torch.empty((len(cams), int(out_h), int(out_w)), dtype=torch.float32, device=dev)
    my = torch.empty_like(mx)
    arr = (L.mvRectifyCam * len(cams))(*cams)
    with torch.cuda.device(dev):
        L.check(lib.mv_rectify_maps(arr, len(cams), int(out_h), int(out_w), mx.data_ptr(), my.data_ptr(), _stream()), "mv_rectify_maps")
    return mx, my


_RM_DST = {torch.uint8: L.MV_PP_U8, torch.float32: L.MV_F32, torch.float16: L.MV_F16, torch.bfloat16: L.MV_BF16}


def remap(images, maps, dtype=torch.float32, layout: str = "hwc", reverse_channels=False, out: "list | None" = None) -> list:
    """``mv_remap_lanes``: ``cv2.remap(image, map_x, map_y, INTER_LINEAR)`` (8-bit fixed point, constant border 0) of every image of every group in ONE launch
    on the current stream, and the loaders' ``float32 / 255`` (EuRoC.py:224-236, VBR.py:50-65); never synchronises.

    ``images``: a list of up to ``MV_RM_MAX_GROUPS`` uint8 GPU tensors (a single tensor is one group) of one source size and lane count — ``[lanes, H, W, C]``
    under ``layout="hwc"`` (what ``cv2.imread`` returns; ``[lanes, H, W]`` is C = 1) or ``[lanes, C, H, W]`` under ``"planar"``, C in 1, 3, 4.  ``maps``: one
    ``(map_x, map_y)`` pair per group, fp32 ``[h, w]`` (shared by the lanes) or ``[lanes, h, w]``.  ``dtype``: ``torch.float32`` / ``float16`` / ``bfloat16``
    (``out / 255``, a true division, rounded once more for the 16-bit types) or ``torch.uint8`` (the remapped bytes, planar).  ``reverse_channels`` (a bool, or
    one per group): BGR -> RGB.  Returns one ``[lanes, C, h, w]`` tensor per group."""
    lib = L.load()
    if isinstance(images, torch.Tensor):
        images, maps = [images], ([maps] if isinstance(maps[0], torch.Tensor) else maps)
    if layout not in ("hwc", "planar"):
        raise ValueError(f"remap: layout {layout!r} (hwc or planar)")
    if dtype not in _RM_DST:
        raise ValueError(f"remap: dtype {dtype!r} (uint8, float32, float16 or bfloat16)")
    if len(images) != len(maps) or (out is not None and len(out) != len(images)):
        raise ValueError("remap: one map pair (and one output) per group")
    rev = list(reverse_channels) if isinstance(reverse_channels, (list, tuple)) else [bool(reverse_channels)] * len(images)
    groups, res, keep = [], [], []
    lanes = src_hw = out_hw = None
    for i, (t, (mx, my)) in enumerate(zip(images, maps)):
        if not (t.is_cuda and mx.is_cuda and my.is_cuda):
            raise L.MacvoHipError("remap: expected GPU tensors (the HIP hot path has no CPU fallback)")
        if layout == "hwc" and t.dim() == 3:
            t = t.unsqueeze(-1)
        if t.dim() != 4:
            raise L.MacvoHipError(f"remap: image {tuple(t.shape)}: expected [lanes, H, W, C] (hwc) or [lanes, C, H, W] (planar)")
        B = int(t.shape[0])
        Cn, hw = (int(t.shape[3]), tuple(t.shape[1:3])) if layout == "hwc" else (int(t.shape[1]), tuple(t.shape[2:4]))
        if mx.dtype != torch.float32 or my.dtype != torch.float32 or mx.shape != my.shape or mx.dim() not in (2, 3) or (mx.dim() == 3 and mx.shape[0] != B):
            raise L.MacvoHipError(f"remap: maps must be an fp32 pair of one shape, [h, w] or [{B}, h, w], not {tuple(mx.shape)} / {tuple(my.shape)}")
        ohw = tuple(mx.shape[-2:])
        if lanes is None:
            lanes, src_hw, out_hw = B, hw, ohw
        if (B, hw, ohw) != (lanes, src_hw, out_hw):
            raise L.MacvoHipError("remap: every group of a launch has the same lane count, source size and map size")
        t, mx, my = t.contiguous(), mx.contiguous(), my.contiguous()
        o = None if out is None else out[i]
        if o is None:
            o = torch.empty((B, Cn, ohw[0], ohw[1]), dtype=dtype, device=t.device)
        elif o.shape != (B, Cn, ohw[0], ohw[1]) or o.dtype != dtype or not o.is_contiguous() or o.device != t.device:
            raise ValueError(f"remap: out[{i}] must be a contiguous {dtype} [{B}, {Cn}, {ohw[0]}, {ohw[1]}] tensor on the inputs' device")
        g = L.mvRemapGroup()
        g.src, g.dst, g.map_x, g.map_y = t.data_ptr(), o.data_ptr(), mx.data_ptr(), my.data_ptr()
        g.src_lane_stride, g.dst_lane_stride = Cn * hw[0] * hw[1], Cn * ohw[0] * ohw[1]
        g.map_lane_stride = ohw[0] * ohw[1] if mx.dim() == 3 else 0
        g.channels, g.layout, g.reverse_channels = Cn, L.MV_RM_HWC if layout == "hwc" else L.MV_RM_PLANAR, int(rev[i])
        g.src_dtype = L.MV_PP_U8 if t.dtype == torch.uint8 else _DT.get(t.dtype, -1)           # (anything but uint8 is refused by the library)
        g.dst_dtype = _RM_DST[dtype]
        groups.append(g)
        keep += [t, mx, my]                # (contiguous copies made above must outlive the enqueue)
        res.append(o)
    if not groups:
        raise ValueError("remap: no images")
    # (the group count, the lane count, the channel count and the source type are checked by the library: one place decides, its code is raised)
    arr = (L.mvRemapGroup * len(groups))(*groups)
    with torch.cuda.device(res[0].device):
        L.check(lib.mv_remap_lanes(arr, len(groups), lanes, src_hw[0], src_hw[1], out_hw[0], out_hw[1], _stream()), "mv_remap_lanes")
    return res
