"""The decoder's motion encoder off the GPU: the host twin (tests/motion_encoder_twin.py) against MotionEncoder.forward, what the accumulation order is
worth against the GPU test's bar, the conditions under which that test means something (ReLU leaves enough of every stored tensor alive), the NaN
footprints, the library's tensor table and the argument checks of the new entry points."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from tests import motion_encoder_twin as T
from tools import flowformer_host as FH

INVALID_ARG = -1     # MV_ERR_INVALID_ARG (include/macvo_hip.h)
CASES = [(d, s, seed) for d in T.DTYPES for s in T.SHAPES for seed in (0, 1, 2, 3)]


@pytest.mark.parametrize("acc,tol", [(torch.float32, 0.0), (torch.float64, 1e-12)])
def test_unrounded_twin_is_the_module(acc, tol):
    """With no rounding the twin is MotionEncoder.forward: bit for bit in fp32, to 1e-12 of the scale in fp64."""
    m = T.make_module(0).to(acc)
    flow, corr = (t.to(acc) for t in T.make_inputs(T.SHAPES[1], 0))
    with torch.no_grad():
        ref = m(flow, corr)
        got = T.forward(m.state_dict(), flow, corr, None, acc)
    assert got.shape == ref.shape == (2, 128, 9, 18) and got.dtype == acc
    assert float((got - ref).abs().max()) <= tol * float(ref.abs().max())
    assert torch.equal(got[:, T.LIVE:], flow)


@pytest.mark.parametrize("dtname,shape,seed", CASES)
def test_accumulation_order_is_worth_less_than_an_ulp_and_relu_hides_nothing(dtname, shape, seed):
    """Moving the twin from fp32 to fp64 accumulation moves every stored tensor (C1, cor, F1, flo, out) by less than 1 ulp(scale): measured over seeds 0-3,
    the four shapes and both operands at most 0.55 ulp (bf16) and 0.64 ulp (fp16), and 0 only at some 35-pixel bf16 cases — so the GPU test's bar of
    2 ulp(scale) is neither vacuous nor violated by the reference itself.  And every stored tensor has at least 25 % non-zero elements (measured
    0.47-0.55), so ReLU cannot hide a wrong layer."""
    c = T.Case(dtname, shape, seed) if seed else T.case(dtname, shape)
    for name in T.STORED:
        a, b = c.stored[name].double(), c.stored64[name]
        scale = float(a.abs().max())
        moved = float((a - b).abs().max()) / (T.ULP[dtname] * scale)
        alive = float((a != 0).double().mean())
        print(f"{name}: fp32 -> fp64 accumulation {moved:.2f} ulp(scale), non-zero {alive:.2f}")
        assert scale > 0 and moved < 1.0, (name, moved)
        assert alive >= 0.25, (name, alive)
    assert c.scale == float(c.twin[:, :T.LIVE].abs().max()) < float(c.flow.float().abs().max())      # the pass-through flow does not set the scale
    assert torch.equal(c.twin[:, T.LIVE:], c.flow.float())


def _window(shape, r):
    """The (2 r + 1)^2 window around T.NAN_AT's pixel, clipped to image 0: a [B,1,H,W] mask."""
    B, H, W = shape
    _, _, y, x = T.NAN_AT
    m = torch.zeros(B, 1, H, W, dtype=torch.bool)
    m[0, 0, max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
    return m


@pytest.mark.parametrize("dtname", list(T.DTYPES))
def test_nan_footprints_are_the_receptive_fields(dtname):
    """One NaN in flow at the last pixel of image 0 of (2, 9, 18) reaches the 11 x 11 window (7x7, 3x3, 3x3) clipped to that image in every one of channels
    0..125, plus that one element of the pass-through; one NaN in corr reaches the 5 x 5 window (1x1, 3x3, 3x3).  Neither reaches image 1."""
    for which, r in (("flow", 5), ("corr", 2)):
        _, _, twin = T.nan_case(dtname, which)
        nan = torch.isnan(twin)
        assert torch.equal(nan[:, :T.LIVE], _window(T.NAN_SHAPE, r).expand(-1, T.LIVE, -1, -1)), which
        through = torch.zeros_like(nan[:, T.LIVE:])
        if which == "flow":
            through[T.NAN_AT] = True
        assert torch.equal(nan[:, T.LIVE:], through) and not nan[1].any()
        assert torch.isfinite(twin[~nan]).all()


def test_tensor_table_is_the_modules_state_dict():
    from macvo_amd import _lib as L
    from macvo_amd import ops

    sd = FH.MotionEncoder(T.COR_PLANES).state_dict()
    assert ops.motion_encoder_tensor_table() == [(k, tuple(v.shape)) for k, v in sd.items()]
    enc = FH.GMAUpdateBlock(FH.demo_cfg()).encoder
    assert ops.motion_encoder_tensor_table() == [(k, tuple(v.shape)) for k, v in enc.state_dict().items()]
    lib = L.load()
    assert lib.mv_motion_encoder_tensor_count() == 10 and lib.mv_abi_version() == 8


def test_entry_points_check_their_arguments():
    from macvo_amd import _lib as L

    lib = L.load()
    name, shape, ndim = C.create_string_buffer(64), (C.c_int32 * 4)(), C.c_int32()
    assert lib.mv_motion_encoder_tensor_info(4, name, shape, C.byref(ndim)) == L.MV_OK
    assert name.value == b"convf1.weight" and tuple(shape) == (128, 2, 7, 7) and ndim.value == 4
    assert lib.mv_motion_encoder_tensor_info(9, name, shape, C.byref(ndim)) == L.MV_OK
    assert name.value == b"conv.bias" and tuple(shape) == (126, 0, 0, 0) and ndim.value == 1
    for i in (-1, 10):
        assert lib.mv_motion_encoder_tensor_info(i, name, shape, C.byref(ndim)) == INVALID_ARG
    assert lib.mv_motion_encoder_tensor_info(0, None, shape, C.byref(ndim)) == INVALID_ARG
    assert lib.mv_motion_encoder_tensor_info(0, name, None, C.byref(ndim)) == INVALID_ARG
    assert lib.mv_motion_encoder_tensor_info(0, name, shape, None) == INVALID_ARG

    n_params = sum(v.numel() for v in FH.MotionEncoder(T.COR_PLANES).state_dict().values())
    for op in (L.MV_F16, L.MV_BF16):
        # fragments of 256 x 192, 192 x 2304, 128 x 128, 64 x 1152, 128 x 2304 in 16 bits and 256 + 192 + 128 + 64 + 128 fp32 biases
        assert lib.mv_motion_encoder_packed_bytes(op) == 2 * (256 * 192 + 192 * 2304 + 128 * 128 + 64 * 1152 + 128 * 2304) + 4 * 768 >= 2 * n_params
    assert lib.mv_motion_encoder_packed_bytes(L.MV_F32) == 0
    assert lib.mv_motion_encoder_workspace_bytes(2, 60, 80) == 1920 * 2 * 60 * 80
    for B, H, W in ((0, 5, 7), (1, 0, 7), (1, 5, 0), (-1, 5, 7), (1, 1025, 1024), (65536, 65536, 1)):
        assert lib.mv_motion_encoder_workspace_bytes(B, H, W) == 0
    assert lib.mv_motion_encoder_workspace_bytes(1, 1024, 1024) > 0

    # pack and forward refuse before anything touches the device (the pointers are never dereferenced)
    buf = torch.zeros(16)
    p = buf.data_ptr()
    ptrs = (C.c_void_p * 10)(*([p] * 10))
    assert lib.mv_motion_encoder_pack(L.MV_BF16, None, p, None) == INVALID_ARG
    assert lib.mv_motion_encoder_pack(L.MV_BF16, ptrs, None, None) == INVALID_ARG
    assert lib.mv_motion_encoder_pack(L.MV_F32, ptrs, p, None) == INVALID_ARG
    ptrs[7] = None
    assert lib.mv_motion_encoder_pack(L.MV_BF16, ptrs, p, None) == INVALID_ARG

    good = [L.MV_BF16, p, p, p, 1, 5, 7, 0, p, p, None]
    for idx in (1, 2, 3, 8, 9):                              # packed, flow, corr, out, workspace
        args = list(good)
        args[idx] = None
        assert lib.mv_motion_encoder_forward(*args) == INVALID_ARG
    for idx, bad in ((0, L.MV_F32), (0, 7), (4, 0), (5, 0), (6, 0), (5, -3), (7, 2), (4, 1 << 21)):
        args = list(good)
        args[idx] = bad
        assert lib.mv_motion_encoder_forward(*args) == INVALID_ARG
    args = list(good)
    args[4:7] = [4, 1024, 1024]                              # B * H * W beyond 2^20
    assert lib.mv_motion_encoder_forward(*args) == INVALID_ARG


def test_missing_and_misshaped_tensors_name_the_key():
    from macvo_amd import _lib as L
    from macvo_amd import ops

    sd = T.make_module(0).state_dict()
    with pytest.raises(L.MacvoHipError, match=r"convf2\.bias"):
        ops.MotionEncoderWeights({k: v for k, v in sd.items() if k != "convf2.bias"}, "bf16", device="cpu")
    with pytest.raises(L.MacvoHipError, match=r"convc1\.weight.*\(256, 145, 1, 1\)"):
        ops.MotionEncoderWeights(FH.MotionEncoder(81).state_dict(), "bf16", device="cpu")
    with pytest.raises(L.MacvoHipError, match="operand"):
        ops.MotionEncoderWeights(sd, "f32", device="cpu")


def test_hook_is_off_by_default_and_leaves_other_encoders_alone(monkeypatch):
    """Without the flag (argument None, variable unset) the returned list and the module are as before; with it the name is appended and forward rebound;
    an encoder over other than 145 correlation channels keeps its layers; CPU tensors run the original layers, bit for bit."""
    from macvo_amd import plugins

    monkeypatch.delenv("MACVO_HIP_MOTION_ENCODER", raising=False)
    torch.manual_seed(0)
    dec = FH.MemoryCovDecoder(FH.demo_cfg()).eval()
    model = SimpleNamespace(memory_decoder=dec)
    enc = dec.update_block.encoder
    names0 = plugins.install_flowformer_hooks(model)
    assert "memory_decoder.update_block.encoder" not in names0 and "forward" not in vars(enc)
    assert plugins.install_flowformer_hooks(model, fuse_motion_encoder=False) == names0 and "forward" not in vars(enc)
    keys = list(enc.state_dict())
    flow, corr = T.make_inputs(T.SHAPES[0], 0)
    with torch.no_grad():
        ref = enc(flow, corr)
    monkeypatch.setenv("MACVO_HIP_MOTION_ENCODER", "on")
    assert plugins.install_flowformer_hooks(model) == names0 + ["memory_decoder.update_block.encoder"]
    fused = enc.forward.__self__
    assert list(enc.state_dict()) == keys
    with torch.no_grad():
        assert torch.equal(enc(flow, corr), ref) and fused.fused_calls == 0      # CPU fp32: the layers
    monkeypatch.delenv("MACVO_HIP_MOTION_ENCODER")
    other = FH.MemoryCovDecoder(FH.demo_cfg()).eval()
    other.update_block.encoder = FH.MotionEncoder(81)
    names = plugins.install_flowformer_hooks(SimpleNamespace(memory_decoder=other), fuse_motion_encoder=True)
    assert names == names0 and "forward" not in vars(other.update_block.encoder)


@pytest.mark.parametrize("layer", T.CONVS)
@pytest.mark.parametrize("dtname,shape", [("bf16", (2, 9, 18)), ("f16", (2, 9, 18)), ("bf16", (3, 5, 7))])
def test_one_hot_cases_show_every_row_of_the_scrambled_layer(dtname, shape, layer):
    """The one-hot layer cases of the GPU test compare the result only.  Between the pass-through variants of motion_encoder_twin.LAYER_VARIANTS every
    output row of the scrambled layer reaches channels 0..125 of the twin's result (setting the row to zero changes it) — the flow branch through
    CF[:, 192:256] and rows 126 and up of convc1 / convc2 included; and with the flow branch scrambled the result changes when flow does."""
    c = T.case(dtname, shape)
    rows = set()
    for shifts in T.LAYER_VARIANTS[layer]:
        sd = T.selection_weights(c.sd, layer, 3, shifts)
        rows |= T.observed_rows(sd, layer, c.flow, c.corr, c.dt)
        if layer in ("convf1", "convf2"):
            with torch.no_grad():
                assert not torch.equal(T.stored(sd, torch.ones_like(c.flow), c.corr, c.dt)["out"], T.stored(sd, c.flow, c.corr, c.dt)["out"])
    assert rows == set(range(c.sd[layer + ".weight"].shape[0])), sorted(set(range(c.sd[layer + ".weight"].shape[0])) - rows)
