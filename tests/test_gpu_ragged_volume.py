"""The ragged column edge of the streaming cost-volume kernels: N2 = H2 * W2 no multiple of 64 — the 1/8 maps of KITTI (47 x 98, N = 4606 = 71 * 64 + 62)
and EuRoC (60 x 94, N = 5640 = 88 * 64 + 8) frames, plus the smallest maps that clear the 16-bit streaming kernel's size floor (33 x 66: tail 2;
45 x 47: tail 3, an odd N).

Per kernel (`corr_volume_split_stream<f16x2 | bf16x3>`, `corr_volume_h_stream<out16>`): the dispatch, parity with the fp64
einsum at the project's bar 2e-5 sqrt(C), bit-equality with the ALIGNED path on `f2` padded with zero pixels to the next multiple of 64 and cropped (a
cell depends only on its own two feature rows; the f16x2 row scale is per pixel), and a guard region around the output that must stay untouched (the
lanes past N2 in the last sub-tile's stores are masked off, the rows past the end of `f2` are never read)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 256
BAR = 2e-5 * C ** 0.5                      # tests/test_gpu_corr.py, tests/test_gpu_split.py
SENTINEL = -12345.5                        # exactly representable in fp32, fp16 and bf16
GUARD = 192                                # cells in front of and behind the volume

# (B, (H1, W1), (H2, W2))
CASES = [(1, (33, 66), (33, 66)), (2, (33, 66), (33, 66)), (1, (45, 47), (45, 47)), (1, (47, 98), (47, 98)), (1, (60, 94), (60, 94)),
         (1, (47, 98), (60, 94))]
EVEN_CASES = [c for c in CASES if (c[2][0] * c[2][1]) % 2 == 0]


@functools.lru_cache(maxsize=2)
def _case(B, hw1, hw2, dt):
    """N(0,1) feature maps [B, C, H, W] (rounded to `dt` when it is a 16-bit type) and the fp64 einsum [B * N1, N2], computed once per case"""
    from oracle import corr

    g = torch.Generator().manual_seed(hw1[0] * 1000 + hw2[1] + B)
    f1, f2 = torch.randn(B, C, *hw1, generator=g), torch.randn(B, C, *hw2, generator=g)
    if dt != torch.float32:
        f1, f2 = f1.to(dt), f2.to(dt)
    ref = corr.corr_volume(f1, f2, torch.float64).view(B * hw1[0] * hw1[1], hw2[0] * hw2[1])
    return f1, f2, ref


def _guarded(n, dtype, gpu):
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype, device=gpu)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all())


def _flat(f, layout):
    """[B, C, H, W] -> the map as one row of pixels: [B, C, 1, N] (chw) / [B, 1, N, C] (hwc)"""
    B, Cc = f.shape[:2]
    f = f.reshape(B, Cc, 1, -1)
    return f.contiguous() if layout == "chw" else f.permute(0, 2, 3, 1).contiguous()


def _pad_pixels(f, layout, n_pad):
    z = list(f.shape)
    z[3 if layout == "chw" else 2] = n_pad
    return torch.cat([f, torch.zeros(z, dtype=f.dtype, device=f.device)], dim=3 if layout == "chw" else 2).contiguous()


@pytest.mark.parametrize("B,hw1,hw2", CASES)
def test_packed_volume_at_a_ragged_n2(gpu, B, hw1, hw2):
    from macvo_amd import ops

    f1, f2, ref = _case(B, hw1, hw2, torch.float32)
    N1, N2 = hw1[0] * hw1[1], hw2[0] * hw2[1]
    N2p = -(-N2 // 64) * 64
    assert N2 % 64 != 0
    for mode in ("f16x2", "bf16x3"):
        for layout in ("chw", "hwc"):
            a1, a2 = (f1, f2) if layout == "chw" else (f1.permute(0, 2, 3, 1).contiguous(), f2.permute(0, 2, 3, 1).contiguous())
            d1, d2 = a1.to(gpu), a2.to(gpu)
            buf, cells = _guarded(B * N1 * N2, torch.float32, gpu)
            out = ops.corr_volume(d1, d2, layout=layout, precision=mode, out=cells.view(B * N1, 1, *hw2))
            assert ops.last_volume_kernel() == f"corr_volume_split_stream<{mode}>", (mode, layout, ops.last_volume_kernel())
            assert out.data_ptr() == cells.data_ptr() and _guards_intact(buf, B * N1 * N2), (mode, layout)
            err = (out.view(B * N1, N2).cpu().double() - ref).abs().max().item()
            print(f"ragged packed volume {mode} {layout} B={B} N1={N1} N2={N2}: max |err| = {err:.3e} (bar {BAR:.3e})")
            assert err <= BAR, (mode, layout, err)
            # the aligned path on f2 padded with zero pixels, cropped: the same bits
            p1, p2 = _flat(f1, layout).to(gpu), _pad_pixels(_flat(f2, layout).to(gpu), layout, N2p - N2)
            full = ops.corr_volume(p1, p2, layout=layout, precision=mode)
            assert ops.last_volume_kernel() == f"corr_volume_split_stream<{mode}>" and full.shape == (B * N1, 1, 1, N2p)
            assert torch.equal(full.view(B * N1, N2p)[:, :N2], out.view(B * N1, N2)), (mode, layout)
            del full, buf, cells, out


def test_f16x2_row_exponents_at_the_ragged_edge(gpu):
    """rows scaled by 2^+-20 (tests/test_gpu_split.py:113-117) in the LAST, partial sub-tile of f2 and in the last row block of f1: the per-row exponent table is read
    for the clamped rows too, and the cells keep the accuracy relative to sum |a||b|"""
    from macvo_amd import ops

    B, N1, N2 = 1, 33 * 66, 47 * 98
    g = torch.Generator().manual_seed(17)
    f1, f2 = torch.randn(B, N1, C, generator=g), torch.randn(B, N2, C, generator=g)
    tail0 = (N2 // 64) * 64                                   # first column of the partial sub-tile
    f2[0, tail0] *= 2.0 ** 20
    f2[0, N2 - 1] *= 2.0 ** -20
    f2[0, N2 - 2] *= 2.0 ** 10
    f2[0, tail0 - 1] *= 2.0 ** -20
    f1[0, N1 - 1] *= 2.0 ** 20
    f1[0, 11] *= 2.0 ** -20
    f1[0, 5] = 0.0
    buf, cells = _guarded(B * N1 * N2, torch.float32, gpu)
    out = ops.corr_volume(f1.to(gpu), f2.to(gpu), layout="hwc", precision="f16x2", out=cells.view(B * N1, 1, 1, N2))
    assert ops.last_volume_kernel() == "corr_volume_split_stream<f16x2>" and _guards_intact(buf, B * N1 * N2)
    got = out.view(B, N1, N2).cpu().double()
    ref = torch.einsum("bid,bjd->bij", f1.double(), f2.double())
    scale = torch.einsum("bid,bjd->bij", f1.double().abs(), f2.double().abs())
    assert torch.isfinite(got).all() and (got[0, 5] == 0).all()
    assert ((got - ref).abs() / scale.clamp_min(1e-300)).max().item() <= 1e-6
    p2 = torch.cat([f2, torch.zeros(B, -(-N2 // 64) * 64 - N2, C)], dim=1)
    full = ops.corr_volume(f1.to(gpu), p2.to(gpu), layout="hwc", precision="f16x2")
    assert torch.equal(full.view(B * N1, -1)[:, :N2], out.view(B * N1, N2))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,hw1,hw2", CASES)
def test_16bit_streaming_volume_at_a_ragged_n2(gpu, dt, B, hw1, hw2):
    """2-byte cells for every even N2: the streaming kernel, equal to the fp32-cell volume rounded once.  An odd N2 with 2-byte cells is outside the kernel's
    domain (a lane stores a column PAIR as one dword) and says so.  fp32 cells at a ragged N2 stay with the tile kernel, which measured faster there."""
    from macvo_amd import ops

    f1, f2, ref = _case(B, hw1, hw2, dt)
    N1, N2 = hw1[0] * hw1[1], hw2[0] * hw2[1]
    N2p = -(-N2 // 64) * 64
    d1, d2 = f1.permute(0, 2, 3, 1).contiguous().to(gpu), f2.permute(0, 2, 3, 1).contiguous().to(gpu)
    buf, cells = _guarded(B * N1 * N2, torch.float32, gpu)
    v32 = ops.corr_volume(d1, d2, layout="hwc", out=cells.view(B * N1, 1, *hw2))
    assert ops.last_volume_kernel() == "corr_volume_h_hwc", ops.last_volume_kernel()
    assert _guards_intact(buf, B * N1 * N2)
    err = (v32.view(B * N1, N2).cpu().double() - ref).abs().max().item()
    print(f"ragged 16-bit streaming volume {dt} B={B} N1={N1} N2={N2}: max |err| = {err:.3e} (bar {BAR:.3e})")
    assert err <= BAR, err
    p1, p2 = d1.view(B, 1, N1, C), _pad_pixels(d2.view(B, 1, N2, C), "hwc", N2p - N2)
    full = ops.corr_volume(p1, p2, layout="hwc")                         # the aligned streaming kernel: the same bits as the tile kernel's
    assert ops.last_volume_kernel() == "corr_volume_h_stream"
    assert torch.equal(full.view(B * N1, N2p)[:, :N2], v32.view(B * N1, N2))
    dtc = ops.L.MV_F16 if dt == torch.float16 else ops.L.MV_BF16
    if N2 % 2:
        assert not ops.L.load().mv_corr_volume_out16_supported(B, C, N1, N2, dtc, ops.L.MV_LAYOUT_HWC)
        assert ops.corr_volume_out16(d1, d2) is None
        return
    assert ops.L.load().mv_corr_volume_out16_supported(B, C, N1, N2, dtc, ops.L.MV_LAYOUT_HWC)
    buf16, cells16 = _guarded(B * N1 * N2, dt, gpu)
    v16 = ops.corr_volume_out16(d1, d2, out=cells16.view(B * N1, 1, *hw2))
    assert v16 is not None and ops.last_volume_kernel() == "corr_volume_h_stream<out16>", ops.last_volume_kernel()
    assert _guards_intact(buf16, B * N1 * N2)
    assert v16.dtype == dt and torch.equal(v16, v32.to(dt))              # the same accumulators, rounded to nearest even once
    full16 = ops.corr_volume_out16(p1, p2)
    assert ops.last_volume_kernel() == "corr_volume_h_stream<out16>"
    assert torch.equal(full16.view(B * N1, N2p)[:, :N2], v16.view(B * N1, N2))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_out16_volume_with_128_channels_at_a_ragged_n2(gpu, dt):
    """C = 128: a DMA piece of the streaming kernel covers four rows of f2 instead of two, so the row clamp and the per-piece source offset take their other
    shape.  47 x 98 maps, B = 1 (B * N1 * N2 = 2.1e7 >= 2^22): parity, the padded-and-cropped aligned volume bit for bit, guards."""
    from macvo_amd import ops

    Cc, hw = 128, (47, 98)
    N = hw[0] * hw[1]
    Np = -(-N // 64) * 64
    g = torch.Generator().manual_seed(128)
    f1, f2 = torch.randn(1, N, Cc, generator=g).to(dt), torch.randn(1, N, Cc, generator=g).to(dt)
    ref = torch.einsum("bid,bjd->bij", f1.double(), f2.double())[0]
    d1, d2 = f1.view(1, *hw, Cc).to(gpu), f2.view(1, *hw, Cc).to(gpu)
    buf16, cells16 = _guarded(N * N, dt, gpu)
    v16 = ops.corr_volume_out16(d1, d2, out=cells16.view(N, 1, *hw))
    assert v16 is not None and ops.last_volume_kernel() == "corr_volume_h_stream<out16>", ops.last_volume_kernel()
    assert _guards_intact(buf16, N * N)
    v32 = ops.corr_volume(d1, d2, layout="hwc")
    assert (v32.view(N, N).cpu().double() - ref).abs().max().item() <= 2e-5 * Cc ** 0.5
    assert torch.equal(v16, v32.to(dt))
    p1, p2 = d1.view(1, 1, N, Cc), _pad_pixels(d2.view(1, 1, N, Cc), "hwc", Np - N)
    full16 = ops.corr_volume_out16(p1, p2)
    assert ops.last_volume_kernel() == "corr_volume_h_stream<out16>"
    assert torch.equal(full16.view(N, Np)[:, :N], v16.view(N, N))
