"""GPU: the decoder's recurrent update blocks (csrc/update_block.hip) against the host twin (tests/update_block_twin.py: same operands, same rounding
points, torch's summation order) and the fp64 module, plus structure (tap / channel / row order, zero padding, layouts, workspace, recurrence, graph
capture) and the opt-in hooks on the FlowFormerCov-shaped host network.

Bars (per output tensor, scale = max |twin output|): max |kernel - twin| <= 2 ulp(scale) = scale * 2^-6 (bf16) / 2^-9 (fp16); the kernel's error against
the fp64 module <= 1.25 x the eager 16-bit module's, both measured in the same test on the CPU references of update_block_twin.case."""
from __future__ import annotations

import pytest
import torch

from tests import update_block_twin as T

pytestmark = pytest.mark.gpu

KINDS = {T.COV: "cov", T.FLOW: "flow"}


@pytest.fixture(scope="module")
def weights(gpu):
    from macvo_amd import ops

    cache = {}

    def get(c: T.Case):
        key = (c.kind, c.dtname, c.seed)
        if key not in cache:
            cache[key] = ops.UpdateBlockWeights.from_module({k: v.to(gpu) for k, v in c.sd.items()}, KINDS[c.kind], c.dtname)
        return cache[key]
    return get


def _run(gpu, w, net, inp, **kw):
    from macvo_amd import ops

    out = ops.update_block(net.to(gpu), inp.to(gpu), w, **kw)
    torch.cuda.synchronize()
    return [t.float().cpu() for t in out]


def _check_twin(c: T.Case, got, twin, scale=None, factor=(1.0, 1.0, 1.0), what=""):
    for i, name in enumerate(T.OUTPUTS):
        s = c.scale[i] if scale is None else scale[i]
        bar = 2 * T.ULP[c.dtname] * s * factor[i]
        d = float((got[i] - twin[i].float()).abs().max())
        print(f"{what}{name}: max |kernel - twin| = {d:.3e} = {d / (T.ULP[c.dtname] * s) if s else 0:.2f} ulp(scale), bar {bar:.3e}")
        assert got[i].shape == twin[i].shape and torch.isfinite(got[i]).all()
        assert d <= bar, (what, name, d, bar)


@pytest.mark.parametrize("shape", T.SHAPES)
@pytest.mark.parametrize("dtname", list(T.DTYPES))
@pytest.mark.parametrize("kind", [T.COV, T.FLOW])
def test_block_against_the_twin_and_the_fp64_module(gpu, weights, kind, dtname, shape):
    """Both kinds, both operands, the three shapes: (1, 5, 7) is smaller than every halo and tile, (2, 9, 18) has partial tiles, a row and an image boundary
    inside a 32-pixel MFMA column block, (1, 47, 98) is KITTI's grid.  Measured on MI355X, worst over kinds and shapes: max |kernel - twin| = 0.56 / 0.55 /
    0.63 ulp(scale) for net / delta / mask in bf16 and 0.62 / 0.85 / 0.83 in fp16 (bar 2); kernel error against the fp64 module = 0.47-0.87 x the eager
    module's in bf16 and 0.55-0.95 x in fp16 (bar 1.25)."""
    c = T.case(kind, dtname, shape)
    got = _run(gpu, weights(c), c.net, c.inp)
    _check_twin(c, got, c.twin)
    for i, name in enumerate(T.OUTPUTS):
        e_got, e_eager = T.rel_err(got[i], c.f64[i]), T.rel_err(c.eager[i], c.f64[i])
        print(f"{name}: kernel {e_got:.3e} eager {e_eager:.3e} of the fp64 module's scale (ratio {e_got / e_eager:.2f})")
        assert e_got <= 1.25 * e_eager, (name, e_got, e_eager)


# ---------------------------------------------------------------------------------------------------------------- isolating weights
_COV_CONVS = [f"gru.conv{g}{s}" for s in (1, 2) for g in "zrq"] + [f"cov_head.conv{i}" for i in (1, 2, 3, 4)] + ["mask.0", "mask.2"]
_FLOW_CONVS = ["flow_head.0", "flow_head.2"]


def _selection_weights(sd, scrambled: str, seed: int):
    """Every convolution picks, per output channel, ONE input element: the centre tap of channel o % cin with gain 1 — except ``scrambled``, which picks a
    random tap of a random channel with gain +-1 or +-0.5.  One non-zero product per output: exact whatever the summation order, so the kernel can differ
    from the twin only where a tap, a channel, a row of a stacked GEMM or a padded border is wrong (or by the last place of sigmoid / tanh)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in sd.items():
        if k.endswith(".bias"):
            out[k] = (torch.randint(-1, 2, v.shape, generator=g) * 0.5).to(v.dtype)
            continue
        cout, cin, kh, kw = v.shape
        w = torch.zeros(v.shape)
        o = torch.arange(cout)
        if k[:-len(".weight")] == scrambled:
            ch, ty, tx = (torch.randint(0, n, (cout,), generator=g) for n in (cin, kh, kw))
            gain = torch.tensor([1.0, -1.0, 0.5, -0.5])[torch.randint(0, 4, (cout,), generator=g)]
        else:
            ch, ty, tx, gain = o % cin, torch.full((cout,), kh // 2), torch.full((cout,), kw // 2), torch.ones(cout)
        w[o, ch, ty, tx] = gain
        out[k] = w.to(v.dtype)
    return out


_ALL_CONVS = [(T.COV, n) for n in _COV_CONVS] + [(T.FLOW, n) for n in _FLOW_CONVS]
_THREE_IMAGES = (3, 5, 7)     # three images inside one 64-pixel tile: what the 1x5 and 5x1 taps of the GRU launches must not read across
# (kind, conv, operand, shape); the bf16 cases at (2, 9, 18) keep the ids they have always had
_LAYER_CASES = ([pytest.param(k, n, "bf16", T.SHAPES[1], id=f"{k}-{n}") for k, n in _ALL_CONVS]
                + [pytest.param(k, n, "f16", T.SHAPES[1], id=f"{k}-{n}-f16") for k, n in _ALL_CONVS]
                + [pytest.param(T.COV, n, d, _THREE_IMAGES, id=f"{T.COV}-{n}-{d}-3x5x7") for d in T.DTYPES for n in _COV_CONVS if n.startswith("gru.")])


@pytest.mark.parametrize("kind,conv,dtname,shape", _LAYER_CASES)
def test_layers_one_by_one(gpu, kind, conv, dtname, shape):
    """Tap order, 1x5 against 5x1, the channel order across the [h, x] / [r h, x] concatenation, the z / r row split, the conv1 | mask.0 pairing and the
    2-of-64-row conv4 / flow_head.2 launches: one convolution at a time gets scrambled one-hot weights, the others pass their centre tap through.  Both
    operand types at (2, 9, 18); the GRU convolutions also at (3, 5, 7), where a tile holds three images."""
    from macvo_amd import ops

    c = T.case(kind, dtname, shape)
    sd = _selection_weights(c.sd, conv, 3)
    w = ops.UpdateBlockWeights.from_module({k: v.to(gpu) for k, v in sd.items()}, KINDS[kind], dtname)
    with torch.no_grad():
        twin = T.forward(sd, kind, c.net, c.inp, c.dt)
    scale = [float(t.abs().max()) for t in twin]
    assert all(s > 0 for s in scale)
    _check_twin(c, _run(gpu, w, c.net, c.inp), twin, scale, what=conv + " ")


@pytest.mark.parametrize("kind,shape", [pytest.param(k, s, id=("flow-" if k == T.FLOW else "") + f"shape{i}")
                                        for k in (T.COV, T.FLOW) for i, s in enumerate(T.SHAPES[:2])])
def test_border_only_input(gpu, weights, kind, shape):
    """Only the border pixels of net and inp are non-zero: a wrong zero pad, or a tap read across the row, image or tile edge, moves interior outputs."""
    c = T.case(kind, "bf16", shape)
    B, H, W = shape
    keep = torch.zeros(1, 1, H, W, dtype=torch.bool)
    keep[..., 0, :] = keep[..., -1, :] = keep[..., :, 0] = keep[..., :, -1] = True
    net, inp = c.net * keep, c.inp * keep
    with torch.no_grad():
        twin = T.forward(c.sd, kind, net, inp, c.dt)
    _check_twin(c, _run(gpu, weights(c), net, inp), twin, [float(t.abs().max()) for t in twin])


def test_layout_determinism_and_dirty_workspace(gpu, weights):
    """Channels-last and NCHW inputs, a second call, and a workspace filled with NaN bit patterns beforehand all give the same bits."""
    _layout_determinism_and_dirty_workspace(gpu, weights, T.COV)


def test_layout_determinism_and_dirty_workspace_flow(gpu, weights):
    """The same for the FLOW members: their two-row flow_head.2 launch and the unscaled mask."""
    _layout_determinism_and_dirty_workspace(gpu, weights, T.FLOW)


def _layout_determinism_and_dirty_workspace(gpu, weights, kind):
    from macvo_amd import _lib as L

    c = T.case(kind, "f16", T.SHAPES[1])
    w = weights(c)
    ref = _run(gpu, w, c.net, c.inp)
    again = _run(gpu, w, c.net, c.inp)
    cl = torch.channels_last
    net_cl, inp_cl = c.net.to(gpu).contiguous(memory_format=cl), c.inp.to(gpu).contiguous(memory_format=cl)
    assert not net_cl.is_contiguous() and net_cl.is_contiguous(memory_format=cl)
    last = _run(gpu, w, net_cl, inp_cl)
    B, H, W = c.shape
    ws = torch.full((L.load().mv_update_block_workspace_bytes(w.kind, B, H, W),), 0xFF, dtype=torch.uint8, device=gpu)   # 0xFFFF: NaN in both types
    dirty = _run(gpu, w, c.net, c.inp, workspace=ws)
    for a, b, d, r in zip(again, last, dirty, ref):
        assert torch.equal(a, r) and torch.equal(b, r) and torch.equal(d, r)


@pytest.mark.parametrize("kind,dtname", [pytest.param(k, d, id=("flow-" if k == T.FLOW else "") + d) for k in (T.COV, T.FLOW) for d in T.DTYPES])
def test_recurrence_of_twelve_iterations(gpu, weights, kind, dtname):
    """Twelve calls feeding net back, against the twin's twelve.  Bar: the per-call 2 ulp(scale) times the drift the twin itself shows between fp32 and
    fp64 accumulation over twelve iterations relative to one (update_block_twin.recurrence of the same kind; measured on the CPU at (2, 9, 18): factors
    1.0-1.9 for bf16 and 1.0-1.8 for fp16 (COV), 1.9-2.1 and 1.0 (FLOW) — the GRU is contractive).  Measured on MI355X after twelve calls (COV): 0.58 / 0.44 / 0.68 ulp(scale) for net /
    delta / mask in both operand types, no more than after one call."""
    from macvo_amd import ops

    c = T.case(kind, dtname, T.SHAPES[1])
    twin12, scale12, factor, d = T.recurrence(kind, dtname, T.SHAPES[1], 12)
    print("twin fp32 against fp64 accumulation, / scale: one call", ["%.2e" % v for v in d[0]], "twelve", ["%.2e" % v for v in d[1]], "factor", factor)
    w, net, inp = weights(c), c.net.to(gpu), c.inp.to(gpu)
    for _ in range(12):
        net, delta, mask = ops.update_block(net, inp, w)
    torch.cuda.synchronize()
    _check_twin(c, [t.float().cpu() for t in (net, delta, mask)], twin12, scale12, factor, what="after 12 calls ")


def test_graph_capture_equals_the_eager_call(gpu, weights):
    from macvo_amd import ops

    c = T.case(T.FLOW, "bf16", T.SHAPES[1])
    w, net, inp = weights(c), c.net.to(gpu), c.inp.to(gpu)
    ref = ops.update_block(net, inp, w)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.update_block(net, inp, w)                      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.update_block(net, inp, w)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, ref):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- hooks
def test_fp32_decoder_falls_through_to_the_layers(gpu, monkeypatch):
    from macvo_amd import plugins
    from tools import flowformer_host as FH
    from types import SimpleNamespace

    torch.manual_seed(0)
    dec = FH.MemoryCovDecoder(FH.demo_cfg()).to(gpu).eval()
    net, inp = (t.to(gpu) for t in T.make_inputs(T.SHAPES[1], 0))
    ub = dec.update_block
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)     # the layers themselves must repeat their bits for the comparison to mean anything:
    with torch.no_grad():                                                 # deterministic convolution algorithms, chosen before the reference is taken
        for _ in range(2):
            dec.cov_update(net, inp)
            h = ub.gru(net, inp)
            ub.flow_head(h), ub.mask(h)
        ref = dec.cov_update(net, inp)
        rh = ub.gru(net, inp)
        rd, rm = ub.flow_head(rh), ub.mask(rh)
        names = plugins.install_flowformer_hooks(SimpleNamespace(memory_decoder=dec), fuse_update_blocks=True)
        assert "memory_decoder.cov_update.forward" in names and "memory_decoder.update_block.gru" in names
        got = dec.cov_update(net, inp)
        h = ub.gru(net, inp)
        assert all(torch.equal(a, b) for a, b in zip(got, ref))
        assert torch.equal(h, rh) and torch.equal(ub.flow_head(h), rd) and torch.equal(ub.mask(h), rm)
        assert dec.cov_update.forward.__self__.fused_calls == 0 and ub.gru.forward.__self__.fused_calls == 0
        # ... and the same modules in bf16 take the kernels; a tensor that is not the gru's result runs the head's own layers
        dec.to(torch.bfloat16)
        nb, ib = net.bfloat16(), inp.bfloat16()
        dec.cov_update(nb, ib)
        hb = ub.gru(nb, ib)
        db = ub.flow_head(hb)
        assert dec.cov_update.forward.__self__.fused_calls == 1 and ub.gru.forward.__self__.fused_calls == 1
        assert torch.equal(ub.flow_head(hb.clone()), type(ub.flow_head).forward(ub.flow_head, hb)) and db.shape == (2, 2, 9, 18)


def test_hooked_network_with_fused_update_blocks(gpu):
    """tools/flowformer_host.FlowFormerCovHost, Fast-mode dtypes (encoder fp16, decoder bf16), 640 x 480, B = 2, twelve iterations.  The deviation of the
    hooked bf16-decoder network from the same network with an fp32 decoder is what eager bf16 layers cost; with the update blocks fused the deviation
    must stay within 1.25 x that, for the flow and for sigma.  Measured on MI355X: flow 3.4e-3 px eager against 3.0e-3 px fused, sigma 1.95e-3 against
    1.6-1.8e-3 relative."""
    from macvo_amd import plugins
    from tools import flowformer_host as FH

    g = torch.Generator().manual_seed(2)
    a, b = torch.rand(2, 3, 480, 640, generator=g).to(gpu), torch.rand(2, 3, 480, 640, generator=g).to(gpu)

    def run(dec_dtype, fuse):
        torch.manual_seed(7)
        m = FH.FlowFormerCovHost(FH.demo_cfg(decoder_depth=12), torch.float16, dec_dtype).to(gpu).eval()
        names = plugins.install_flowformer_hooks(m, fuse_update_blocks=fuse)
        with torch.inference_mode():
            f, c = m.inference(a, b)
        calls = m.memory_decoder.cov_update.forward.__self__.fused_calls if fuse else 0
        return f.float(), c.float(), names, calls

    f32, c32, _, _ = run(torch.float32, False)
    f0, c0, names0, _ = run(torch.bfloat16, False)
    f1, c1, names1, calls = run(torch.bfloat16, True)
    assert names1 == names0 + ["memory_decoder.cov_update.forward"] + [f"memory_decoder.update_block.{n}" for n in ("gru", "flow_head", "mask")]
    assert calls == 12
    assert torch.isfinite(f1).all() and torch.isfinite(c1).all()
    dev0, dev1 = float((f0 - f32).abs().max()), float((f1 - f32).abs().max())
    sig0, sig1 = float((c0 / c32 - 1).abs().max()), float((c1 / c32 - 1).abs().max())
    print(f"flow: eager bf16 decoder {dev0:.3e} px, fused update blocks {dev1:.3e} px; sigma: {sig0:.3e} / {sig1:.3e} relative")
    assert dev0 > 0 and dev1 <= 1.25 * dev0, (dev1, dev0)
    assert sig1 <= 1.25 * sig0, (sig1, sig0)
