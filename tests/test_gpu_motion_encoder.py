"""GPU: the decoder's motion encoder (csrc/motion_encoder.hip) against the host twin (tests/motion_encoder_twin.py: same operands, same rounding points,
torch's summation order) and the fp64 module, plus structure (im2col tap / channel order, channel and row padding, the [cor | flo] split, layouts,
workspace, streams), bad values, refusals and the opt-in hook on the FlowFormerCov-shaped host network.

Bars (scale = max |twin| over channels 0..125): max |kernel - twin| <= 2 ulp(scale) = scale * 2^-6 (bf16) / 2^-9 (fp16); the kernel's error against the
fp64 module <= 1.25 x the eager 16-bit module's, both from the CPU references of motion_encoder_twin.case; channels 126..127 equal flow bit for bit."""
from __future__ import annotations

from types import SimpleNamespace

import pytest
import torch

from tests import motion_encoder_twin as T

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def weights(gpu):
    from macvo_amd import ops

    cache = {}

    def get(c: T.Case):
        key = (c.dtname, c.seed)
        if key not in cache:
            cache[key] = ops.MotionEncoderWeights.from_module({k: v.to(gpu) for k, v in c.sd.items()}, c.dtname)
        return cache[key]
    return get


def _call(gpu, w, flow, corr, **kw):
    from macvo_amd import ops

    out = ops.motion_encoder(flow.to(gpu), corr.to(gpu), w, **kw)
    torch.cuda.synchronize()
    return out


def _run(gpu, w, flow, corr, **kw):
    return _call(gpu, w, flow, corr, **kw).float().cpu()


def _same_bits(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _dirty_workspace(gpu, shape):
    from macvo_amd import _lib as L

    return torch.full((L.load().mv_motion_encoder_workspace_bytes(*shape),), 0xFF, dtype=torch.uint8, device=gpu)      # 0xFFFF: a NaN in both types


def _check_twin(dtname, got, twin, flow, what=""):
    """Finite elements of channels 0..125 within 2 ulp(scale) of the twin, the non-finite ones where the twin has them; flow passed through bit for bit."""
    scale = T.live_scale(twin)
    bar = 2 * T.ULP[dtname] * scale
    assert got.shape == twin.shape and scale > 0
    g, t = got[:, :T.LIVE], twin[:, :T.LIVE].float()
    assert torch.equal(torch.isnan(g), torch.isnan(t)) and torch.equal(torch.isinf(g), torch.isinf(t)), what
    fin = torch.isfinite(t)
    assert torch.equal(g[~fin & ~torch.isnan(t)], t[~fin & ~torch.isnan(t)]), what         # infinities: the same sign
    d = float((g[fin] - t[fin]).abs().max())
    print(f"{what}max |kernel - twin| = {d:.3e} = {d / (T.ULP[dtname] * scale):.2f} ulp(scale), bar {bar:.3e}")
    assert d <= bar, (what, d, bar)
    assert torch.equal(got[:, T.LIVE:].view(torch.int32), flow.float().view(torch.int32)), what      # (a NaN passes through as a NaN of the same bits)
    return d / (T.ULP[dtname] * scale)


@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtname", list(T.DTYPES))
def test_kernel_against_the_twin_and_the_fp64_module(gpu, weights, dtname, shape):
    """Both operands at (1, 5, 7): the image is smaller than the 7x7 halo; (2, 9, 18): partial tiles, a row and an image boundary inside one 32-pixel
    block; (3, 5, 7): three images in one 64-pixel tile; (1, 47, 98): KITTI's grid.  Measured on MI355X, in that order of shapes: max |kernel - twin| =
    0.48 / 0.16 / 0.46 / 0.55 ulp(scale) in bf16 and 0.48 / 0.62 / 0.46 / 0.55 in fp16 (bar 2); kernel error against the fp64 module = 1.00 x the eager
    module's in all eight cases (bar 1.25): the largest error of both is one element's last rounding."""
    c = T.case(dtname, shape)
    got = _run(gpu, weights(c), c.flow, c.corr)
    assert torch.isfinite(got).all()
    _check_twin(dtname, got, c.twin, c.flow)
    e_got, e_eager = T.rel_err(got, c.f64), T.rel_err(c.eager.float(), c.f64)
    print(f"kernel {e_got:.3e} eager {e_eager:.3e} of the fp64 module's scale (ratio {e_got / e_eager:.2f})")
    assert e_got <= 1.25 * e_eager, (e_got, e_eager)


_LAYER_CASES = [pytest.param(n, i, d, sh, id=f"{n}-{i}-{d}" + ("-3x5x7" if sh == (3, 5, 7) else ""))
                for d, sh in (("bf16", (2, 9, 18)), ("f16", (2, 9, 18)), ("bf16", (3, 5, 7))) for n in T.CONVS for i in range(len(T.LAYER_VARIANTS[n]))]


@pytest.mark.parametrize("conv,variant,dtname,shape", _LAYER_CASES)
def test_layers_one_by_one(gpu, conv, variant, dtname, shape):
    """The 49-tap x 2-channel im2col order, the 145-of-192 channel padding, the [cor | flo] column split of CF and the 126-of-128 row store: one
    convolution at a time gets scrambled one-hot weights (a random tap of a random input channel per output channel), the others pass a centre tap
    through, shifted over the channels so that between the variants of motion_encoder_twin.LAYER_VARIANTS EVERY row of the scrambled layer reaches the
    result — the flow branch through CF[:, 192:256] included (tests/test_motion_encoder_host.py proves that on the twin).  One non-zero product plus a
    bias of 0 or +-0.5 per output is exact in fp32 whatever the summation order, and there is no transcendental function in this block: bit equality
    with the twin, on a workspace full of NaN patterns.  Measured on MI355X: all 30 cases bit-equal."""
    from macvo_amd import ops

    c = T.case(dtname, shape)
    sd = T.selection_weights(c.sd, conv, 3, T.LAYER_VARIANTS[conv][variant])
    w = ops.MotionEncoderWeights.from_module({k: v.to(gpu) for k, v in sd.items()}, dtname)
    with torch.no_grad():
        st = T.stored(sd, c.flow, c.corr, c.dt)
        branch = "flow" if conv in ("convf1", "convf2") else "corr"          # ... and the result does depend on the branch under test
        other = T.stored(sd, torch.ones_like(c.flow) if branch == "flow" else c.flow, c.corr if branch == "flow" else torch.ones_like(c.corr), c.dt)
    twin = st["full"]
    assert all(float(st[k].abs().max()) > 0 for k in T.STORED) and not torch.equal(other["out"], st["out"])
    got = _run(gpu, w, c.flow, c.corr, workspace=_dirty_workspace(gpu, shape))
    assert torch.equal(got, twin), (conv, float((got - twin).abs().max()))


@pytest.mark.parametrize("shape", T.EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtname", list(T.DTYPES))
def test_edge_shapes(gpu, weights, dtname, shape):
    """One pixel; one row wider than a 32-pixel block (every vertical tap outside); one column (vertical neighbours linearly adjacent, every horizontal tap
    outside); two rows whose starts drift by one against the block.  Measured on MI355X, in that order: 0.00 / 0.00 / 0.11 / 0.00 ulp(scale) in bf16,
    0.00 / 0.22 / 0.45 / 0.42 in fp16 (bar 2)."""
    c = T.case(dtname, shape)
    got = _run(gpu, weights(c), c.flow, c.corr, workspace=_dirty_workspace(gpu, shape))
    _check_twin(dtname, got, c.twin, c.flow)


def test_more_images_than_a_grid_dimension_holds(gpu, weights):
    """B = 65 537 one-pixel images, beyond the 65 535 blocks a grid's y and z take: the image index rides in x.  Every image is its own 1 x 1 problem,
    so the twin on the CPU is cheap."""
    shape = (65537, 1, 1)
    c = T.case("bf16", (1, 1, 1))
    flow, corr = (t.to(c.dt) for t in T.make_inputs(shape, 5))
    with torch.no_grad():
        twin = T.forward(c.sd, flow, corr, c.dt)
    _check_twin("bf16", _run(gpu, weights(c), flow, corr), twin, flow, what="B = 65537: ")


@pytest.mark.parametrize("dtname", list(T.DTYPES))
def test_layouts_workspace_and_streams(gpu, weights, dtname):
    """NCHW and channels-last inputs, a second call, a workspace pre-filled with NaN bytes and a call on a side stream give the same bits; nothing is
    written outside the output or outside mv_motion_encoder_workspace_bytes (4 KiB guards around both, the slices aligned to 16 bytes and no more)."""
    from macvo_amd import _lib as L
    from macvo_amd import ops

    shape = (2, 9, 18)
    c = T.case(dtname, shape)
    w, flow, corr = weights(c), c.flow.to(gpu), c.corr.to(gpu)
    ref = _call(gpu, w, flow, corr)
    assert _same_bits(_call(gpu, w, flow, corr), ref)
    cl = torch.channels_last
    flow_cl, corr_cl = flow.contiguous(memory_format=cl), corr.contiguous(memory_format=cl)
    assert not flow_cl.is_contiguous() and not corr_cl.is_contiguous()
    assert _same_bits(_call(gpu, w, flow_cl, corr_cl), ref)
    assert _same_bits(_call(gpu, w, flow_cl, corr), ref) and _same_bits(_call(gpu, w, flow, corr_cl), ref)      # mixed layouts: flow follows corr
    assert _same_bits(_call(gpu, w, flow, corr, workspace=_dirty_workspace(gpu, shape)), ref)

    lib, guard = L.load(), 4096
    nws, nout = lib.mv_motion_encoder_workspace_bytes(*shape), ref.numel() * 2
    assert nws == 1920 * 2 * 9 * 18

    def guarded(n):
        big = torch.full((n + 2 * guard + 32,), 0xA5, dtype=torch.uint8, device=gpu)
        lo = guard + (16 - (big.data_ptr() + guard) % 32) % 32               # data_ptr + lo = 16 mod 32
        assert (big.data_ptr() + lo) % 32 == 16
        return big, lo
    big_ws, lo_ws = guarded(nws)
    big_out, lo_out = guarded(nout)
    for channels_last, f, co in ((0, flow, corr), (1, flow_cl, corr_cl)):
        big_ws.fill_(0xA5), big_out.fill_(0xA5)
        L.check(lib.mv_motion_encoder_forward(w.operand_type, w.packed.data_ptr(), f.data_ptr(), co.data_ptr(), *shape, channels_last,
                                              big_out.data_ptr() + lo_out, big_ws.data_ptr() + lo_ws, ops._stream()), "mv_motion_encoder_forward")
        torch.cuda.synchronize()
        assert torch.equal(big_out[lo_out:lo_out + nout].view(torch.int16), ref.view(torch.int16).reshape(-1))
        for big, lo, n in ((big_ws, lo_ws, nws), (big_out, lo_out, nout)):
            assert bool((big[:lo] == 0xA5).all()) and bool((big[lo + n:] == 0xA5).all())

    side = torch.cuda.Stream()
    flow_s, corr_s = torch.zeros_like(flow), torch.zeros_like(corr)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flow_s.copy_(flow)                                                      # inputs produced on the side stream just before the call
        corr_s.copy_(corr)
        out_s = ops.motion_encoder(flow_s, corr_s, w)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _same_bits(out_s, ref)


@pytest.mark.parametrize("which", ["flow", "corr"])
@pytest.mark.parametrize("dtname", list(T.DTYPES))
def test_one_nan_reaches_its_receptive_field_and_no_further(gpu, weights, dtname, which):
    """One NaN in flow (or corr) at the last pixel of image 0 of (2, 9, 18): the kernel's NaN set is the twin's (the 11 x 11, or 5 x 5, window clipped to
    image 0 in channels 0..125, and the pass-through element), the finite elements stay within the bar, and a workspace full of NaN patterns changes
    nothing."""
    c = T.case(dtname, T.NAN_SHAPE)
    flow, corr, twin = T.nan_case(dtname, which)
    assert 0 < int(torch.isnan(twin[0]).sum()) < twin[0].numel() and not torch.isnan(twin[1]).any()
    raw = _call(gpu, weights(c), flow, corr)
    _check_twin(dtname, raw.float().cpu(), twin, flow, what=f"NaN in {which}: ")
    assert _same_bits(_call(gpu, weights(c), flow, corr, workspace=_dirty_workspace(gpu, T.NAN_SHAPE)), raw)


@pytest.mark.parametrize("dtname", list(T.DTYPES))
def test_infinite_correlation_values(gpu, weights, dtname):
    """One +inf and one -inf in corr: convc1 spreads each over its pixel's 256 channels with the sign of the weight, ReLU keeps the +inf, and the 3x3
    layers sum infinities of both signs into NaN: the kernel's NaN set, its infinities and their signs are the twin's, the finite rest is within the bar."""
    c = T.case(dtname, T.NAN_SHAPE)
    corr = c.corr.clone()
    corr[0, 5, 2, 3], corr[0, 100, 6, 12] = float("inf"), float("-inf")
    with torch.no_grad():
        twin = T.forward(c.sd, c.flow, corr, c.dt)
    assert not torch.isfinite(twin[0]).all() and torch.isfinite(twin[1]).all()
    _check_twin(dtname, _run(gpu, weights(c), c.flow, corr), twin, c.flow, what="inf in corr: ")


def test_refusals_launch_nothing(gpu, weights):
    """Wrong channel counts, an fp32 operand, a workspace one byte short or off the 16-byte grid, mismatched devices, dtypes and shapes and a size beyond
    2^20 pixels all raise MacvoHipError, and neither the output handed to the C entry nor the workspace is written."""
    from macvo_amd import _lib as L
    from macvo_amd import ops

    lib = L.load()
    c = T.case("bf16", (1, 5, 7))
    w, flow, corr = weights(c), c.flow.to(gpu), c.corr.to(gpu)
    nws = lib.mv_motion_encoder_workspace_bytes(*c.shape)
    SENT = 0x5A
    ws = torch.full((nws + 16,), SENT, dtype=torch.uint8, device=gpu)
    out = torch.full((1, 128, 5, 7), -7.0, dtype=c.dt, device=gpu)

    def untouched():
        torch.cuda.synchronize()
        return bool((ws == SENT).all()) and bool((out == -7.0).all())

    def forward(operand, shape):
        return lib.mv_motion_encoder_forward(operand, w.packed.data_ptr(), flow.data_ptr(), corr.data_ptr(), *shape, 0, out.data_ptr(), ws.data_ptr(),
                                             ops._stream())
    big = (1, 17, 61681)
    assert big[1] * big[2] == 2 ** 20 + 1 and lib.mv_motion_encoder_workspace_bytes(*big) == 0
    for operand, shape in ((w.operand_type, big), (L.MV_F32, c.shape), (w.operand_type, (2 ** 20 + 1, 1, 1)), (w.operand_type, (1, 0, 7))):
        with pytest.raises(L.MacvoHipError):
            L.check(forward(operand, shape), "mv_motion_encoder_forward")
        assert untouched()
    one = torch.zeros(1, dtype=c.dt, device=gpu)
    with pytest.raises(L.MacvoHipError, match="out of range"):
        ops.motion_encoder(one.expand(1, 2, *big[1:]), one.expand(1, 145, *big[1:]), w, workspace=ws[:nws])
    with pytest.raises(L.MacvoHipError, match="flow must be"):
        ops.motion_encoder(torch.cat([flow, flow[:, :1]], dim=1), corr, w, workspace=ws[:nws])
    with pytest.raises(L.MacvoHipError, match="corr must be"):
        ops.motion_encoder(flow, corr[:, :144], w, workspace=ws[:nws])
    with pytest.raises(L.MacvoHipError, match="flow must be"):
        ops.motion_encoder(flow.float(), corr.float(), w, workspace=ws[:nws])
    with pytest.raises(L.MacvoHipError, match="corr must be"):
        ops.motion_encoder(flow, corr.half(), w, workspace=ws[:nws])
    with pytest.raises(L.MacvoHipError, match="corr must be"):
        ops.motion_encoder(flow, corr.cpu(), w, workspace=ws[:nws])
    with pytest.raises(L.MacvoHipError, match="workspace"):
        ops.motion_encoder(flow, corr, w, workspace=ws[:nws - 1])
    assert ws.data_ptr() % 16 == 0
    with pytest.raises(L.MacvoHipError, match="workspace"):
        ops.motion_encoder(flow, corr, w, workspace=ws[8:8 + nws])
    with pytest.raises(L.MacvoHipError, match="workspace"):
        ops.motion_encoder(flow, corr, w, workspace=ws[:nws].cpu())
    with pytest.raises(L.MacvoHipError, match="do not belong together"):
        ops.motion_encoder(torch.cat([flow, flow]), corr, w, workspace=ws[:nws])
    with pytest.raises(L.MacvoHipError, match="do not belong together"):
        ops.motion_encoder(flow, corr[:, :, :-1], w, workspace=ws[:nws])
    with pytest.raises(L.MacvoHipError, match="operand"):
        ops.MotionEncoderWeights({k: v.to(gpu) for k, v in c.sd.items()}, "f32")
    assert untouched()
    # ... and the same arguments, right, are taken: the sentinels go
    L.check(forward(w.operand_type, c.shape), "mv_motion_encoder_forward")
    torch.cuda.synchronize()
    assert _same_bits(out, ops.motion_encoder(flow, corr, w)) and not bool((ws[:nws] == SENT).all()) and bool((ws[nws:] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------- hook
def test_hook_fp32_decoder_keeps_its_layers_and_new_weights_repack(gpu, monkeypatch):
    """An fp32 decoder keeps its layers bit for bit; the same module in bf16 takes the kernels; after load_state_dict with a second seeded state (same
    storage, new version counters) and after .to(float16) (new storage, new operand) the fused call equals ops.motion_encoder on freshly packed weights of
    what the module then holds; a correlation input of another width runs the layers' own error path."""
    from macvo_amd import ops, plugins
    from tools import flowformer_host as FH

    def state(seed):
        torch.manual_seed(seed)
        return FH.MemoryCovDecoder(FH.demo_cfg()).state_dict()

    torch.manual_seed(0)
    dec = FH.MemoryCovDecoder(FH.demo_cfg()).to(gpu).eval()
    enc = dec.update_block.encoder
    flow, corr = (t.to(gpu) for t in T.make_inputs(T.SHAPES[1], 0))
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)     # the layers themselves must repeat their bits for the comparison to mean anything
    monkeypatch.delenv("MACVO_HIP_MOTION_ENCODER", raising=False)
    model = SimpleNamespace(memory_decoder=dec)
    with torch.no_grad():
        for _ in range(2):
            enc(flow, corr)
        ref = enc(flow, corr)
        names0 = plugins.install_flowformer_hooks(model)
        assert "memory_decoder.update_block.encoder" not in names0 and "forward" not in vars(enc)      # the flag off: as before
        names = plugins.install_flowformer_hooks(model, fuse_motion_encoder=True)
        assert names == names0 + ["memory_decoder.update_block.encoder"]
        fused = enc.forward.__self__
        assert torch.equal(enc(flow, corr), ref) and fused.fused_calls == 0

        def fresh(operand, f, co):
            return ops.motion_encoder(f, co, ops.MotionEncoderWeights(enc.state_dict(), operand))

        dec.to(torch.bfloat16)
        fb, cb = flow.bfloat16(), corr.bfloat16()
        first = enc(fb, cb)
        assert fused.fused_calls == 1 and first.shape == (2, 128, 9, 18) and first.dtype == torch.bfloat16
        assert _same_bits(first, fresh("bf16", fb, cb))
        assert fused.fused(fb.float(), cb) is None and fused.fused(fb.cpu(), cb.cpu()) is None and fused.fused(fb, cb[:, :81]) is None
        assert fused.fused_calls == 1

        ptrs = [p.data_ptr() for p in dec.parameters()]
        dec.load_state_dict(state(1))
        assert ptrs == [p.data_ptr() for p in dec.parameters()]            # in place: only the version counters tell
        second = enc(fb, cb)
        assert fused.fused_calls == 2 and _same_bits(second, fresh("bf16", fb, cb)) and not _same_bits(second, first)

        dec.to(torch.float16)
        third = enc(flow.half(), corr.half())
        assert fused.fused_calls == 3 and third.dtype == torch.float16 and set(fused._packed) == {"bf16", "f16"}
        assert _same_bits(third, fresh("f16", flow.half(), corr.half()))
    fb.requires_grad_(True)                                                 # anything that may need a gradient: the layers
    dec.to(torch.bfloat16)
    assert fused.fused(fb, cb) is None


def test_hooked_network_with_fused_motion_encoder(gpu, monkeypatch):
    """tools/flowformer_host.FlowFormerCovHost, Fast-mode dtypes (encoder fp16, decoder bf16), 96 x 64, B = 2, twelve iterations.  The deviation of the
    hooked bf16-decoder network from the same network with an fp32 decoder is what eager bf16 layers cost; with the motion encoder fused the deviation
    must stay within 1.25 x that (the update-block hook test's factor), for the flow and for sigma.  Measured on MI355X: flow 2.36e-3 px eager against
    2.13e-3 px fused, sigma 1.16e-3 against 1.14e-3 relative."""
    from macvo_amd import plugins
    from tools import flowformer_host as FH

    monkeypatch.delenv("MACVO_HIP_MOTION_ENCODER", raising=False)
    g = torch.Generator().manual_seed(2)
    a, b = torch.rand(2, 3, 64, 96, generator=g).to(gpu), torch.rand(2, 3, 64, 96, generator=g).to(gpu)

    def run(dec_dtype, fuse):
        torch.manual_seed(7)
        m = FH.FlowFormerCovHost(FH.demo_cfg(decoder_depth=12), torch.float16, dec_dtype).to(gpu).eval()
        names = plugins.install_flowformer_hooks(m, fuse_motion_encoder=fuse)
        with torch.inference_mode():
            f, c = m.inference(a, b)
        enc = m.memory_decoder.update_block.encoder
        calls = enc.forward.__self__.fused_calls if "forward" in vars(enc) else None
        return f.float(), c.float(), names, calls

    f32, c32, _, _ = run(torch.float32, None)
    f0, c0, names0, calls0 = run(torch.bfloat16, None)
    f1, c1, names1, calls = run(torch.bfloat16, True)
    _, _, names32, calls32 = run(torch.float32, True)
    assert calls0 is None and "memory_decoder.update_block.encoder" not in names0
    assert names1 == names0 + ["memory_decoder.update_block.encoder"] == names32
    assert calls == 12 and calls32 == 0
    assert torch.isfinite(f1).all() and torch.isfinite(c1).all()
    dev0, dev1 = float((f0 - f32).abs().max()), float((f1 - f32).abs().max())
    sig0, sig1 = float((c0 / c32 - 1).abs().max()), float((c1 / c32 - 1).abs().max())
    print(f"flow: eager bf16 decoder {dev0:.3e} px, fused motion encoder {dev1:.3e} px; sigma: {sig0:.3e} / {sig1:.3e} relative")
    assert dev0 > 0 and dev1 <= 1.25 * dev0, (dev1, dev0)
    assert sig1 <= 1.25 * sig0, (sig1, sig0)
