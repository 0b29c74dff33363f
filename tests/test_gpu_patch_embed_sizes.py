"""The fused cost patch embedding at the slice sizes of KITTI (376 x 784 frames: 47 x 98 slices, 48 x 104 after PatchEmbed.forward's F.pad) and EuRoC
(480 x 752: 60 x 94, padded 64 x 96) — `cost_patch_embed_strip_kernel` with 13 token columns (an odd count) and with rows of 98 / 94 cells, which start on
8-byte (fp32) / 4-byte (16-bit) boundaries only and are staged by cell pairs.  Bars: tests/test_gpu_patch_embed.py."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TWIN_TOL = {"bf16": 2e-3, "f16": 2.5e-4}      # vs the same-arithmetic twin, relative to the output scale (tests/test_gpu_patch_embed.py:15-16)
FP32_TOL = {"bf16": 2e-2, "f16": 2.5e-3}      # vs the fp32 chain
SIZES = [(47, 98), (48, 104), (60, 94), (64, 96)]
TOKEN_GRID = {(47, 98): (6, 13), (48, 104): (6, 13), (60, 94): (8, 12), (64, 96): (8, 12)}
DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def _twin(operand):
    from oracle import patch_embed as ope

    return ope.patch_embed_proj_bf16 if operand == "bf16" else ope.patch_embed_proj_f16


def _slices(S, H2, W2, seed, scale=16.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, 1, H2, W2, generator=g) * scale
    x[:, 0, H2 // 3, W2 // 5] += 200.0
    x[:, 0, H2 - 1, W2 - 1] -= 150.0          # the last cell: the padded rows / columns behind it must read as zeros
    x[:, 0, 0, W2 - 1] += 90.0                # the last cell of the first row: the next row starts right behind it
    x[:, 0, 0, 0] += 120.0
    return x


@pytest.mark.parametrize("operand", ["f16", "bf16"])
@pytest.mark.parametrize("S", [1, 7])
@pytest.mark.parametrize("H2,W2", SIZES)
def test_cost_patch_embed_at_the_kitti_and_euroc_sizes(gpu, H2, W2, S, operand):
    """fp32 and 16-bit cells in, fp32 and 16-bit tokens out, channel-major and token-major, against the conv2d chain in the same arithmetic and in fp32"""
    from macvo_amd import ops
    from oracle import patch_embed as ope

    assert ops.cost_patch_embed_supported(H2, W2)
    dt = DT[operand]
    h, w = TOKEN_GRID[(H2, W2)]
    W = ope.make_weights(seed=H2 + S)
    packed = ops.PatchEmbedWeights(*[wt.to(gpu) for wt in W], operand=operand)
    x = _slices(S, H2, W2, seed=S + W2)
    x16 = x.to(dt)
    for cells in (x, x16):
        ref_16 = _twin(operand)(cells.float(), *W)
        ref_32 = ope.patch_embed_proj(cells.float(), *W)
        assert ref_32.shape == (S, 64, h, w)
        scale = ref_32.abs().max().item()
        for tokens in (False, True):
            r16, r32 = (ope.to_tokens(ref_16), ope.to_tokens(ref_32)) if tokens else (ref_16, ref_32)
            got = ops.cost_patch_embed(cells.to(gpu), packed, tokens=tokens, out_dtype=torch.float32)
            assert got.dtype == torch.float32 and got.shape == ((S, h * w, 64) if tokens else (S, 64, h, w))
            e16, e32 = (got.cpu() - r16).abs().max().item(), (got.cpu() - r32).abs().max().item()
            print(f"patch embed {H2}x{W2} S={S} {operand} cells={cells.dtype} tokens={tokens}: twin {e16 / scale:.2e} (bar {TWIN_TOL[operand]:.1e}), "
                  f"fp32 {e32 / scale:.2e} (bar {FP32_TOL[operand]:.1e})")
            assert e16 <= TWIN_TOL[operand] * scale, (cells.dtype, tokens, e16, scale)
            assert e32 <= FP32_TOL[operand] * scale, (cells.dtype, tokens, e32, scale)
            if cells.dtype != torch.float32:
                # 16-bit cells == the fp32-cell kernel on the widened cells, bit for bit; 16-bit tokens == that result rounded once
                assert torch.equal(got, ops.cost_patch_embed(cells.float().to(gpu), packed, tokens=tokens))
                t16 = ops.cost_patch_embed(cells.to(gpu), packed, tokens=tokens)
                assert t16.dtype == dt and torch.equal(t16, got.to(dt)), tokens
            # a slice's tokens do not depend on its neighbours or on the workgroup that produced them
            solo = ops.cost_patch_embed(cells[S // 2: S // 2 + 1].to(gpu), packed, tokens=tokens, out_dtype=torch.float32)
            assert torch.equal(solo[0], got[S // 2])


@pytest.mark.parametrize("operand", ["f16", "bf16"])
@pytest.mark.parametrize("H2,W2", [(47, 98), (60, 94)])
def test_raw_slice_and_its_padded_form_give_the_same_tokens(gpu, H2, W2, operand):
    """what `PatchEmbed.forward` hands to `proj` (F.pad with zeros to multiples of 8) and the raw slice: the kernel pads the raw one itself — the same bits"""
    from macvo_amd import ops
    from oracle import patch_embed as ope

    W = ope.make_weights(seed=7)
    packed = ops.PatchEmbedWeights(*[wt.to(gpu) for wt in W], operand=operand)
    x = _slices(5, H2, W2, seed=3)
    for cells in (x, x.to(DT[operand])):
        raw = cells.to(gpu)
        padded = F.pad(raw, (0, (8 - W2 % 8) % 8, 0, (8 - H2 % 8) % 8)).contiguous()
        assert tuple(padded.shape[-2:]) in SIZES and padded.shape[-1] != W2
        for tokens in (False, True):
            assert torch.equal(ops.cost_patch_embed(raw, packed, tokens=tokens), ops.cost_patch_embed(padded, packed, tokens=tokens)), (cells.dtype, tokens)


@pytest.mark.parametrize("operand", ["f16", "bf16"])
def test_layers_one_by_one_at_47x98(gpu, operand):
    """the layer-isolating weights of tests/test_gpu_patch_embed.py::test_cost_patch_embed_layers_one_by_one on a 47 x 98 slice; probe 1 (box filters over every tap)
    is the one that catches a wrong right-hand halo or padding column"""
    from macvo_amd import ops
    from oracle import patch_embed as ope

    g = torch.Generator().manual_seed(5)
    x = torch.rand(3, 1, 47, 98, generator=g) * 4            # positive: the ReLUs are transparent
    for probe in range(4):
        w1, b1, w2, b2, w3, b3 = [torch.zeros_like(t) for t in ope.make_weights(0)]
        if probe == 0:
            w1[3, 0, 1, 4] = 1.0
            w2[7, 3, 5, 0] = 1.0
            w3[41, 7, 2, 3] = 1.0
        elif probe == 1:
            w1[0, 0] = 1.0 / 36
            w2[0, 0] = 1.0 / 36
            w3[0, 0] = 1.0 / 36
        elif probe == 2:
            gg = torch.Generator().manual_seed(9)
            w1 = (torch.rand(16, 1, 6, 6, generator=gg) > 0.7).float() * 0.25
            w2 = (torch.rand(32, 16, 6, 6, generator=gg) > 0.9).float() * 0.125
            w3 = (torch.rand(64, 32, 6, 6, generator=gg) > 0.9).float() * 0.125
            b1, b2, b3 = torch.rand(16, generator=gg), torch.rand(32, generator=gg), torch.rand(64, generator=gg) - 0.5
        else:
            w1[2, 0, 0, 0] = -1.0
            b1[2] = 2.0
            w2[5, 2, 3, 3] = 1.0
            b2[5] = -1.0
            w3[9, 5, 1, 1] = -1.0
        W = (w1, b1, w2, b2, w3, b3)
        packed = ops.PatchEmbedWeights(*[wt.to(gpu) for wt in W], operand=operand)
        ref = _twin(operand)(x, *W)
        tol = TWIN_TOL[operand] * max(ref.abs().max().item(), 1e-3)
        for tokens in (False, True):
            got = ops.cost_patch_embed(x.to(gpu), packed, tokens=tokens).cpu()
            want = ope.to_tokens(ref) if tokens else ref
            assert (got - want).abs().max().item() <= tol, (probe, tokens, (got - want).abs().max().item(), tol)


def test_flowformer_proj_hook_takes_the_fused_kernel_for_a_47x98_slice(gpu):
    """install_flowformer_hooks on a PatchEmbed stand-in (tests/test_gpu_patch_embed.py): an fp16 47 x 98 slice is padded to 48 x 104 by `forward` and goes through
    the fused kernel — the layers' result at the bf16-style bar of that test, and not the layers' bits"""
    import torch.nn as nn

    from macvo_amd import plugins

    class PatchEmbed(nn.Module):
        def __init__(self):
            super().__init__()
            self.proj = nn.Sequential(nn.Conv2d(1, 16, 6, 2, 2), nn.ReLU(), nn.Conv2d(16, 32, 6, 2, 2), nn.ReLU(), nn.Conv2d(32, 64, 6, 2, 2))

        def forward(self, x):
            x = F.pad(x, (0, (8 - x.shape[-1] % 8) % 8, 0, (8 - x.shape[-2] % 8) % 8))
            return self.proj(x)

    class Enc(nn.Module):
        def __init__(self):
            super().__init__()
            self.patch_embed = PatchEmbed()

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.memory_encoder = Enc()

    torch.manual_seed(0)
    m16 = Model().to(gpu).eval().half()
    x = _slices(9, 47, 98, seed=4).to(gpu).half()
    with torch.no_grad():
        want16 = m16.memory_encoder.patch_embed(x)
        done = plugins.install_flowformer_hooks(m16)
        assert "memory_encoder.patch_embed.proj" in done
        got16 = m16.memory_encoder.patch_embed(x)
    assert got16.dtype == torch.float16 and got16.shape == want16.shape == (9, 64, 6, 13)
    bar = (FP32_TOL["f16"] + 2 ** -11) * want16.float().abs().max().item()      # the operand bar + one output rounding
    assert (got16.float() - want16.float()).abs().max().item() <= bar
    assert not torch.equal(got16, want16)                                        # ... and it really was the kernel
