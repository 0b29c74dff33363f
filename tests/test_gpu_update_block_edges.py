"""GPU: the decoder's recurrent update blocks (csrc/update_block.hip) away from the centre of their domain: degenerate geometry, batch independence,
non-finite inputs, packing from fp32, memory and streams, refusals, and the hooks after the weights change.

Bars: against the host twin (tests/update_block_twin.py) the 2 ulp(scale) per output of tests/test_gpu_update_block.py, with the scale taken over the
twin's finite values; everything else is bit for bit.  tests/test_update_block_host.py keeps the conditions these tests rest on (scales > 0, the twin's
own summation order worth at most 1 ulp(scale), the NaN case's footprint) on the CPU."""
from __future__ import annotations

import pytest
import torch

from tests import update_block_twin as T
from tests.test_gpu_update_block import KINDS, _check_twin, weights  # noqa: F401  (weights: the module-scoped fixture, one pack per seeded block)

pytestmark = pytest.mark.gpu

KIND_DT = [(k, d) for k in (T.COV, T.FLOW) for d in T.DTYPES]
BITS = {"bf16": 0x7F80, "f16": 0x7C00}     # the 16-bit pattern of +inf: anything above it (sign cleared) is a NaN


def _call(gpu, w, net, inp, **kw):
    """ops.update_block on host or device tensors; the three device tensors as they are."""
    from macvo_amd import ops

    return ops.update_block(net.to(gpu), inp.to(gpu), w, **kw)


def _same_bits(a, b) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _all_same_bits(got, ref) -> bool:
    return len(got) == len(ref) and all(_same_bits(a, b) for a, b in zip(got, ref))


def _host(out):
    torch.cuda.synchronize()
    return [t.float().cpu() for t in out]


# ---------------------------------------------------------------------------------------------------------------- a. geometry
@pytest.mark.parametrize("shape", T.EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind,dtname", KIND_DT)
def test_edge_shapes_against_the_twin(gpu, weights, kind, dtname, shape):
    """update_block_twin.EDGE_SHAPES: M = 1 and M = 6 (a wholly dead wave in the 4-wave tile), one row, one column (W = 1: every horizontal tap of the
    staged strip is another row's pixel and only the mask keeps it out), W = 3, three images in one 64-pixel tile, an image boundary on a tile edge, rows
    of 33.  Bar: 2 ulp(scale) per output against the twin.  Measured on MI355X, worst over kinds and shapes: max |kernel - twin| = 0.08 / 0.50 / 0.47
    ulp(scale) for net / delta / mask in bf16 and 0.77 / 0.79 / 0.87 in fp16 (bar 2)."""
    c = T.case(kind, dtname, shape)
    _check_twin(c, _host(_call(gpu, weights(c), c.net, c.inp)), c.twin)


# ---------------------------------------------------------------------------------------------------------------- b. batch independence
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 4, 16)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind,dtname", KIND_DT)
def test_an_image_does_not_depend_on_its_batch(gpu, weights, kind, dtname, shape):
    """The batch call equals the call on each image alone, bit for bit: a pixel's operation sequence (bias, then chunk, tap, k-step, padded taps as exact
    zeros: update_block_math.h) does not depend on its column in a tile or on what the neighbouring columns hold."""
    c = T.case(kind, dtname, shape)
    w, net, inp = weights(c), c.net.to(gpu), c.inp.to(gpu)
    full = _call(gpu, w, net, inp)
    for b in range(shape[0]):
        solo = _call(gpu, w, net[b:b + 1], inp[b:b + 1])
        for name, f, s in zip(T.OUTPUTS, full, solo):
            assert _same_bits(f[b:b + 1], s), (name, b)


# ---------------------------------------------------------------------------------------------------------------- c. non-finite inputs
def _dirty_workspace(gpu, w, shape):
    from macvo_amd import _lib as L

    return torch.full((L.load().mv_update_block_workspace_bytes(w.kind, *shape),), 0xFF, dtype=torch.uint8, device=gpu)     # 0xFFFF: NaN in both types


@pytest.mark.parametrize("kind,dtname", KIND_DT)
def test_one_nan_spreads_as_far_as_the_module_spreads_it(gpu, weights, kind, dtname):
    """update_block_twin.NAN_CASE: one NaN in net at the last pixel of image 0.  The kernel's non-finite elements are exactly the twin's (the receptive
    field, clipped at the corner: a padded tap is replaced, not multiplied by zero, so nothing leaks through a row end, the image boundary or a dead
    lane), its finite elements stay within 2 ulp(scale) of the twin's with the scale over the twin's finite values, image 1 keeps the bits it has without
    the NaN, and a workspace full of NaN patterns changes nothing.  Measured on MI355X, finite elements, worst over kinds: 0.30 / 0.48 / 0.42
    ulp(scale) for net / delta / mask in bf16 and 0.61 / 0.59 / 0.83 in fp16 (bar 2)."""
    c = T.case(kind, dtname, T.NAN_CASE[0])
    net, twin, scale = T.nan_case(kind, dtname)
    w = weights(c)
    raw = _call(gpu, w, net, c.inp)
    clean = _call(gpu, w, c.net, c.inp)
    dirty = _call(gpu, w, net, c.inp, workspace=_dirty_workspace(gpu, w, c.shape))
    got = _host(raw)
    for i, name in enumerate(T.OUTPUTS):
        bad = ~torch.isfinite(twin[i])
        assert torch.equal(~torch.isfinite(got[i]), bad), name
        d = float((got[i] - twin[i].float())[~bad].abs().max())
        bar = 2 * T.ULP[dtname] * scale[i]
        print(f"{name}: {int(bad.sum())} non-finite elements; finite: max |kernel - twin| = {d:.3e} = {d / (T.ULP[dtname] * scale[i]):.2f} ulp(scale), bar {bar:.3e}")
        assert d <= bar, (name, d, bar)
        assert _same_bits(raw[i][1], clean[i][1]), name
    assert _all_same_bits(dirty, raw)


@pytest.mark.parametrize("kind,dtname", KIND_DT)
def test_infinite_inputs_are_squashed_as_the_module_squashes_them(gpu, weights, kind, dtname):
    """One +inf and one -inf in inp, far enough apart that no 1x5 or 5x1 window holds both (inf - inf would be a NaN in the module too): the gates
    saturate to 0 or 1 and tanh to +-1, so every output is finite, within the bar of the twin, and a workspace full of NaN patterns changes nothing."""
    c = T.case(kind, dtname, T.NAN_CASE[0])
    inp = c.inp.clone()
    inp[0, 5, 2, 3], inp[0, 200, 6, 12] = float("inf"), float("-inf")
    twin, scale = T.twin_outputs(c.sd, kind, c.net, inp, c.dt)
    assert all(torch.isfinite(t).all() for t in twin) and all(s > 0 for s in scale)
    w = weights(c)
    raw = _call(gpu, w, c.net, inp)
    _check_twin(c, _host(raw), twin, scale, what="inf ")          # (asserts that the kernel's outputs are finite)
    assert not _all_same_bits(raw, _call(gpu, w, c.net, c.inp))   # ... and the infinities were not simply dropped
    assert _all_same_bits(_call(gpu, w, c.net, inp, workspace=_dirty_workspace(gpu, w, c.shape)), raw)


# ---------------------------------------------------------------------------------------------------------------- d. packing from fp32
def _f32(bits):
    return torch.tensor(bits, dtype=torch.int32).view(torch.float32)       # (positive patterns only)


def _awkward_values() -> torch.Tensor:
    """fp32 values whose rounding to bf16 or fp16 can go wrong, both signs of each; the NaN is placed separately."""
    bits = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0x404A, 0x0001, 0x0002, 0x007F, 0x0080, 0x7F7E, 0x7F7F):       # bf16 ties: low half exactly 0x8000, even and odd
        bits += [(hi << 16) | 0x8000, (hi << 16) | 0x7FFF, (hi << 16) | 0x8001]                      # neighbour; and one fp32 ulp to either side
    for k in (0, 1, 2, 3, 1022, 1023):                                                                # fp16 ties: 1 + k 2^-10 + 2^-11, even and odd k
        base = 0x3F800000 | (k << 13)
        bits += [base | 0x1000, base | 0x0FFF, base | 0x1001]
    pos = _f32(bits)
    two = lambda e: 2.0 ** e
    pos = torch.cat([pos, torch.tensor([
        65504.0, 65519.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e5, 3.3e38, 3.4e38,              # around and above the fp16 maximum; bf16 -> inf
        two(-14), two(-14) - two(-25), two(-14) - two(-26), 6e-5, 1e-6,                               # the fp16 subnormal range: its top, values in it
        two(-24), two(-25), 3 * two(-25), two(-25) * 1.0001, two(-25) * 0.9999, 5 * two(-25),        # its ties (0 | 2^-24 | 2^-23 | 3 * 2^-24) and bottom
        two(-26), 1e-10, 1e-38, 1e-40, two(-149), 0.0], dtype=torch.float32)])                       # below it: fp32 subnormals, zero
    return torch.cat([pos, -pos])


@pytest.mark.parametrize("kind", [T.COV, T.FLOW])
def test_packing_rounds_as_torch_does(gpu, kind):
    """An fp32 state dict is a supported input (operand None: f16), and update_pack_kernel's narrow<> then has to round: ties to even in both parities,
    overflow to inf, fp16 and bf16 subnormals, -0 and NaN are written over a few hundred entries of every weight and bias tensor (all entries of the
    short ones).  The packed bytes must be those of the same state dict rounded by torch.Tensor.to on the host; a NaN has to be a NaN in both, whatever
    its payload.  Nothing here knows the packed layout."""
    from macvo_amd import ops

    vals = _awkward_values()
    g = torch.Generator().manual_seed(11)
    sd = {}
    for k, v in T.make_block(kind, 0).state_dict().items():
        t = v.detach().clone().float()
        flat = t.view(-1)
        n = min(flat.numel(), 2 * vals.numel())
        at = torch.randperm(flat.numel(), generator=g)[:n]
        flat[at] = vals[torch.randperm(vals.numel(), generator=g)].repeat(2)[:n]
        flat[at[0]] = float("nan")
        sd[k] = t
    assert ops.UpdateBlockWeights({k: v.to(gpu) for k, v in sd.items()}, KINDS[kind]).operand == "f16"
    for dtname, dt in T.DTYPES.items():
        got = ops.UpdateBlockWeights({k: v.to(gpu) for k, v in sd.items()}, KINDS[kind], dtname).packed
        ref = ops.UpdateBlockWeights({k: v.to(dt).to(gpu) for k, v in sd.items()}, KINDS[kind], dtname).packed
        torch.cuda.synchronize()
        a, b = got.cpu().view(torch.int16).int() & 0xFFFF, ref.cpu().view(torch.int16).int() & 0xFFFF
        a32, b32 = got.cpu().view(torch.float32), ref.cpu().view(torch.float32)
        nan16 = ((a & 0x7FFF) > BITS[dtname]) & ((b & 0x7FFF) > BITS[dtname])              # a 16-bit weight that is a NaN in both ...
        nan32 = (torch.isnan(a32) & torch.isnan(b32)).repeat_interleave(2)                  # ... or half of an fp32 bias that is
        wrong = (a != b) & ~nan16 & ~nan32
        print(f"{dtname}: {a.numel()} 16-bit units, {int((a != b).sum())} differ, {int(wrong.sum())} of them not NaN in both; "
              f"{int(((a & 0x7FFF) > BITS[dtname]).sum())} NaN patterns")
        assert int(nan16.sum()) >= len(sd) // 2 and int(torch.isnan(a32).sum()) >= len(sd) // 2     # the NaNs arrived, in weights and in biases
        assert not wrong.any(), (dtname, int(wrong.sum()), [hex(int(v)) for v in a[wrong][:8]], [hex(int(v)) for v in b[wrong][:8]])


# ---------------------------------------------------------------------------------------------------------------- e. memory and streams
@pytest.mark.parametrize("shape", [(2, 9, 18), (3, 5, 7)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind,dtname", [(T.COV, "bf16"), (T.FLOW, "f16")])
def test_memory_views_and_streams(gpu, weights, kind, dtname, shape):
    """Nothing is written outside mv_update_block_workspace_bytes (4 KiB guards on both sides of a slice that is aligned to 16 bytes and no more); inputs
    aligned to 2 bytes only, net channels-last with inp NCHW, and batch-strided views give the plain call's bits; so does a call on a side stream whose
    inputs are produced on that stream just before (a launch on any other stream would read them too early), and two calls in a row on one workspace."""
    from macvo_amd import _lib as L

    c = T.case(kind, dtname, shape)
    w, net, inp = weights(c), c.net.to(gpu), c.inp.to(gpu)
    ref = _call(gpu, w, net, inp)

    nws, guard = L.load().mv_update_block_workspace_bytes(w.kind, *shape), 4096
    big = torch.full((nws + 2 * guard + 32,), 0xA5, dtype=torch.uint8, device=gpu)
    lo = guard + (16 - (big.data_ptr() + guard) % 32) % 32                   # data_ptr + lo = 16 mod 32
    ws = big[lo:lo + nws]
    assert ws.data_ptr() % 32 == 16
    assert _all_same_bits(_call(gpu, w, net, inp, workspace=ws), ref)
    assert bool((big[:lo] == 0xA5).all()) and bool((big[lo + nws:] == 0xA5).all())
    assert not bool((ws == 0xA5).all())                                      # (the workspace handed in is the one that was used)

    def off_by_one(t):
        flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device=gpu)
        flat[1:] = t.reshape(-1)
        v = flat[1:].view(t.shape)
        assert v.data_ptr() % 4 == 2 and v.is_contiguous()
        return v
    assert _all_same_bits(_call(gpu, w, off_by_one(net), off_by_one(inp)), ref)
    net_cl = net.contiguous(memory_format=torch.channels_last)
    assert not net_cl.is_contiguous()
    assert _all_same_bits(_call(gpu, w, net_cl, inp), ref)
    assert _all_same_bits(_call(gpu, w, off_by_one(net_cl.permute(0, 2, 3, 1)).permute(0, 3, 1, 2), inp.contiguous(memory_format=torch.channels_last)), ref)

    def every_other(t):
        wide = torch.full((2 * t.shape[0],) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=gpu)
        wide[::2] = t
        return wide[::2]
    assert _all_same_bits(_call(gpu, w, every_other(net), every_other(inp)), ref)

    side = torch.cuda.Stream()
    net_s, inp_s = torch.zeros_like(net), torch.zeros_like(inp)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda._sleep(2_000_000)                                         # about a millisecond of device time ahead of the inputs
        net_s.copy_(net)
        inp_s.copy_(inp)
        out_s = _call(gpu, w, net_s, inp_s)
    torch.cuda.current_stream().wait_stream(side)
    assert _all_same_bits(out_s, ref)

    n2, i2 = (t.to(c.dt).to(gpu) for t in T.make_inputs(shape, 77))
    solo2 = _call(gpu, w, n2, i2)
    shared = torch.empty(nws, dtype=torch.uint8, device=gpu)
    first = _call(gpu, w, net, inp, workspace=shared)
    second = _call(gpu, w, n2, i2, workspace=shared)
    assert _all_same_bits(first, ref) and _all_same_bits(second, solo2) and not _all_same_bits(second, ref)


# ---------------------------------------------------------------------------------------------------------------- f. refusals
def test_refusals_launch_nothing(gpu, weights):
    """B * H * W = 2^20 + 1 (= 1 x 17 x 61681, presented as stride-0 views and as bare pointers: nothing of that size is allocated), a wrong dtype, a
    workspace one byte short, a workspace off the 16-byte grid and mismatched batch shapes all raise MacvoHipError, and neither the outputs handed to the C
    entry nor the workspace handed to ops.update_block is written."""
    from macvo_amd import _lib as L
    from macvo_amd import ops

    lib = L.load()
    c = T.case(T.COV, "bf16", (1, 5, 7))
    w, net, inp = weights(c), c.net.to(gpu), c.inp.to(gpu)
    B, H, W = c.shape
    nws = lib.mv_update_block_workspace_bytes(w.kind, B, H, W)
    SENT = 0x5A
    ws = torch.full((nws + 16,), SENT, dtype=torch.uint8, device=gpu)
    outs = [torch.full((B, ch, H, W), -7.0, dtype=c.dt, device=gpu) for ch in (128, 2, 576)]

    def untouched():
        torch.cuda.synchronize()
        return bool((ws == SENT).all()) and all(bool((t == -7.0).all()) for t in outs)

    big = (1, 17, 61681)
    assert big[1] * big[2] == 2 ** 20 + 1
    assert lib.mv_update_block_workspace_bytes(w.kind, *big) == 0 and lib.mv_update_block_workspace_bytes(w.kind, 1, 1024, 1024) > 0

    def forward(operand, shape):
        return lib.mv_update_block_forward(w.kind, operand, w.packed.data_ptr(), net.data_ptr(), inp.data_ptr(), *shape, 0,
                                           *[t.data_ptr() for t in outs], ws.data_ptr(), ops._stream())
    for operand, shape in ((w.operand_type, big), (L.MV_F32, c.shape), (w.operand_type, (2 ** 20 + 1, 1, 1))):
        with pytest.raises(L.MacvoHipError):
            L.check(forward(operand, shape), "mv_update_block_forward")
        assert untouched()
    one = torch.zeros(1, dtype=c.dt, device=gpu)
    with pytest.raises(L.MacvoHipError, match="out of range"):
        ops.update_block(one.expand(1, 128, *big[1:]), one.expand(1, 384, *big[1:]), w, workspace=ws[:nws])
    with pytest.raises(L.MacvoHipError, match="net must be"):
        ops.update_block(net.float(), inp, w, workspace=ws[:nws])
    with pytest.raises(L.MacvoHipError, match="inp must be"):
        ops.update_block(net, inp.half(), w, workspace=ws[:nws])
    with pytest.raises(L.MacvoHipError, match="workspace"):
        ops.update_block(net, inp, w, workspace=ws[:nws - 1])
    assert ws.data_ptr() % 16 == 0
    with pytest.raises(L.MacvoHipError, match="workspace"):
        ops.update_block(net, inp, w, workspace=ws[8:8 + nws])
    with pytest.raises(L.MacvoHipError, match="do not belong together"):
        ops.update_block(torch.cat([net, net]), inp, w, workspace=ws[:nws])
    with pytest.raises(L.MacvoHipError, match="do not belong together"):
        ops.update_block(net, inp[:, :, :-1], w, workspace=ws[:nws])
    assert untouched()
    # ... and the same arguments, right, are taken: the sentinels go
    L.check(forward(w.operand_type, c.shape), "mv_update_block_forward")
    torch.cuda.synchronize()
    assert _all_same_bits(outs, ops.update_block(net, inp, w)) and not bool((ws[:nws] == SENT).all()) and bool((ws[nws:] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------- g. hooks
def test_hooks_follow_the_weights(gpu, monkeypatch):
    """The hooked decoder in bf16 at (2, 9, 18): after load_state_dict with a second seeded state (same storage, new version counters) and after
    .to(float16) (new storage, new operand) the fused call equals ops.update_block on freshly packed weights of what the module then holds; and the
    FLOW members serve flow_head / mask from the fused call only for the very tensor the last gru call returned."""
    from types import SimpleNamespace

    from macvo_amd import ops, plugins
    from tools import flowformer_host as FH

    def state(seed):
        torch.manual_seed(seed)
        return FH.MemoryCovDecoder(FH.demo_cfg()).state_dict()

    torch.manual_seed(0)
    dec = FH.MemoryCovDecoder(FH.demo_cfg()).to(gpu).eval().to(torch.bfloat16)
    names = plugins.install_flowformer_hooks(SimpleNamespace(memory_decoder=dec), fuse_update_blocks=True)
    assert "memory_decoder.cov_update.forward" in names and "memory_decoder.update_block.gru" in names
    cov, ub = dec.cov_update, dec.update_block
    fused_cov, fused_flow = cov.forward.__self__, ub.gru.forward.__self__
    net, inp = (t.to(gpu) for t in T.make_inputs(T.SHAPES[1], 0))

    def fresh(kind, operand, n, i):
        sd = cov.state_dict() if kind == "cov" else {f"{m}.{k}": v for m in ("gru", "flow_head", "mask") for k, v in getattr(ub, m).state_dict().items()}
        return ops.update_block(n, i, ops.UpdateBlockWeights(sd, kind, operand))

    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # the members' own layers must repeat their bits (as in the fp32 test)
    with torch.no_grad():
        nb, ib = net.bfloat16(), inp.bfloat16()
        first = cov(nb, ib)
        first_h = ub.gru(nb, ib)
        assert fused_cov.fused_calls == 1 and fused_flow.fused_calls == 1
        assert _all_same_bits(first, fresh("cov", "bf16", nb, ib)) and _same_bits(first_h, fresh("flow", "bf16", nb, ib)[0])

        ptrs = [p.data_ptr() for p in dec.parameters()]
        dec.load_state_dict(state(1))
        assert ptrs == [p.data_ptr() for p in dec.parameters()]            # in place: only the version counters tell
        second = cov(nb, ib)
        second_h = ub.gru(nb, ib)
        assert fused_cov.fused_calls == 2 and fused_flow.fused_calls == 2
        assert _all_same_bits(second, fresh("cov", "bf16", nb, ib)) and _same_bits(second_h, fresh("flow", "bf16", nb, ib)[0])
        assert not any(_same_bits(a, b) for a, b in zip(second, first)) and not _same_bits(second_h, first_h)

        dec.to(torch.float16)
        nh, ih = net.half(), inp.half()
        third = cov(nh, ih)
        assert fused_cov.fused_calls == 3 and all(t.dtype == torch.float16 for t in third) and set(fused_cov._packed) == {"bf16", "f16"}
        assert _all_same_bits(third, fresh("cov", "f16", nh, ih))

        # FLOW members, two gru calls in a row: only the second result is served from the fused call
        h1 = ub.gru(nh, ih)
        h2 = ub.gru(h1, ih)
        assert fused_flow.fused_calls == 4
        want = fresh("flow", "f16", h1, ih)
        assert _same_bits(h2, want[0])
        for member, fused_out in ((ub.flow_head, want[1]), (ub.mask, want[2])):
            own = type(member).forward
            own(member, h1)                                                # (the layers choose their algorithm before the comparison)
            assert _same_bits(member(h1), own(member, h1)) and member(h1) is not fused_flow._last[1] and member(h1) is not fused_flow._last[2]
            got = member(h2)
            assert _same_bits(got, fused_out) and any(got is t for t in fused_flow._last[1:])
