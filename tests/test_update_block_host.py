"""The decoder's recurrent update blocks off the GPU: the restated CovUpdateBlock against the reference class's golden, the host twin against the eager
16-bit module and the fp64 module, the library's tensor tables, the argument checks of the new entry points, checkpoint errors and the hooks' default."""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from macvo_amd import _lib as L
from macvo_amd import ops, plugins
from tests import update_block_twin as T
from tests.golden.make_golden_update_block import N_PARAMS, state_dict_sha256
from tools import flowformer_host as FH

INVALID_ARG = -1     # MV_ERR_INVALID_ARG (include/macvo_hip.h)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cov_update_block.npz")
CASES = [(k, d, s) for d in T.DTYPES for k in (T.COV, T.FLOW) for s in T.SHAPES]


def test_restatement_equals_the_reference_class():
    """tools/flowformer_host.CovUpdateBlock against the reference's own covhead.CovUpdateBlock: fp32 bit for bit (same torch ops on the same weights),
    fp64 within 1e-12; the seeded weights are the ones the golden was made with."""
    g = np.load(GOLDEN)
    seed, shape = int(g["seed"]), tuple(int(v) for v in g["shape"])
    block = T.make_block(T.COV, seed)
    assert FH.parameter_count(block) == N_PARAMS == 3075202
    assert state_dict_sha256(block.state_dict()) == str(g["sha"]), (
        "make_block no longer generates the weights the golden was made with (torch's generator or the recipe changed): every comparison against "
        "tests/golden/cov_update_block.npz is void until it is regenerated")
    net, inp = T.make_inputs(shape, seed)
    assert np.array_equal(net.numpy(), g["net"]) and np.array_equal(inp.numpy(), g["inp"])
    with torch.no_grad():
        o32 = block(net, inp)
        o64 = block.double()(net.double(), inp.double())
    for name, a32, a64 in zip(T.OUTPUTS, o32, o64):
        assert np.array_equal(a32.numpy(), g[f"f32_{name}"]), name
        ref = g[f"f64_{name}"]
        assert np.abs(a64.numpy() - ref).max() <= 1e-12 * np.abs(ref).max(), name


@pytest.mark.parametrize("kind,dtname,shape", CASES)
def test_twin_is_no_worse_than_the_eager_module(kind, dtname, shape):
    """Against the fp64 module on the same 16-bit weights and inputs, the twin (one rounding per stored tensor) is within 1.0 x the error of the eager 16-bit
    module (one rounding per operator) for the seeds of update_block_twin.SEEDS — measured here 0.55-0.95 x, so the GPU test's 1.25 x leaves the quarter for
    the summation order.  And the 2 ulp(scale) bar of the GPU test is not vacuous: moving the twin from fp32 to fp64 accumulation moves its outputs by at
    most 6.6e-3 scale (bf16; 2 ulp = 1.56e-2) and 7.8e-4 scale (fp16; 2 ulp = 1.95e-3) over these cases, i.e. up to 0.85 ulp, and by more than 0.1 ulp
    for every case with more than one M tile."""
    c = T.case(kind, dtname, shape)
    moved = 0.0
    for i, name in enumerate(T.OUTPUTS):
        e_twin, e_eager = T.rel_err(c.twin[i], c.f64[i]), T.rel_err(c.eager[i], c.f64[i])
        d64 = float((c.twin[i].double() - c.twin64[i]).abs().max())
        print(f"{name}: twin {e_twin:.2e} eager {e_eager:.2e} ratio {e_twin / e_eager:.2f}; fp32 -> fp64 accumulation {d64 / c.scale[i]:.2e} scale")
        assert e_twin <= 1.0 * e_eager, (name, e_twin, e_eager)
        assert d64 <= c.twin_bar(i), (name, d64, c.twin_bar(i))       # the bar covers a change of summation order ...
        moved = max(moved, d64 / (T.ULP[dtname] * c.scale[i]))
    if shape != T.SHAPES[0]:
        assert moved > 0.1                                             # ... and such a change is visible at that bar's scale


@pytest.mark.parametrize("kind,dtname,shape", [(k, d, s) for d in T.DTYPES for k in (T.COV, T.FLOW) for s in T.EDGE_SHAPES])
def test_edge_shapes_leave_the_gpu_bar_its_meaning(kind, dtname, shape):
    """What tests/test_gpu_update_block_edges.py relies on at update_block_twin.EDGE_SHAPES: every output has a scale to measure against (> 0), and the
    twin's own summation order is worth at most 1.0 ulp(scale) of the 2 ulp(scale) bar — fp32 against fp64 accumulation, measured here at most 0.91
    ((3, 5, 7) COV f16 delta).  A case that misses gets another seed in update_block_twin.SEEDS; the bar is not widened."""
    c = T.case(kind, dtname, shape)
    for i, name in enumerate(T.OUTPUTS):
        assert c.scale[i] > 0 and all(torch.isfinite(t).all() for t in (c.twin[i], c.twin64[i])), name
        d64 = float((c.twin[i].double() - c.twin64[i]).abs().max()) / (T.ULP[dtname] * c.scale[i])
        print(f"{name}: fp32 -> fp64 accumulation {d64:.2f} ulp(scale), scale {c.scale[i]:.3e}")
        assert d64 <= 1.0, (name, d64)


@pytest.mark.parametrize("dtname", list(T.DTYPES))
@pytest.mark.parametrize("kind", [T.COV, T.FLOW])
def test_one_nan_stays_inside_its_image_in_the_twin(kind, dtname):
    """The NaN case of the GPU test (update_block_twin.NAN_CASE: one NaN in net at the last pixel of image 0) asks something: in every output the twin's
    non-finite pixels of image 0 are a non-empty proper subset of its pixels (the receptive field: 5 x 5, 9 x 9 (COV; FLOW 7 x 7) and 6 x 6 pixels
    clipped at the corner: 25 / 81 / 36 of 162 for COV), whole pixels (every channel or none), and image 1 is wholly finite."""
    (B, H, W), _ = T.NAN_CASE
    _, out, scale = T.nan_case(kind, dtname)
    for name, t, s in zip(T.OUTPUTS, out, scale):
        bad = ~torch.isfinite(t)
        px = bad.any(dim=1)
        print(f"{name}: {int(px[0].sum())} of {H * W} pixels of image 0 are not finite")
        assert 0 < int(px[0].sum()) < H * W and not px[1].any() and s > 0, name
        assert torch.equal(bad.all(dim=1), px), name
        side = {"net": 5, "delta": 9 if kind == T.COV else 7, "mask": 6}[name]
        assert int(px[0].sum()) == side * side and px[0, H - side:, W - side:].all(), name


def test_tensor_tables_are_the_modules_state_dicts():
    cov = ops.update_block_tensor_table("cov")
    assert cov == [(k, tuple(v.shape)) for k, v in FH.CovUpdateBlock().state_dict().items()]
    assert sum(int(np.prod(s)) for _, s in cov) == N_PARAMS
    block = FH.GMAUpdateBlock(FH.demo_cfg())
    members = [(k, tuple(v.shape)) for k, v in block.state_dict().items() if k.split(".")[0] in ("gru", "flow_head", "mask")]
    assert ops.update_block_tensor_table("flow") == members
    assert ops.update_block_tensor_table("flow") == [(k, tuple(v.shape)) for k, v in T.FlowUpdateMembers().state_dict().items()]
    lib = L.load()
    assert lib.mv_update_block_tensor_count(L.MV_UPDATE_COV) == 24 and lib.mv_update_block_tensor_count(L.MV_UPDATE_FLOW) == 20
    assert lib.mv_abi_version() == 8


def test_entry_points_check_their_arguments():
    lib = L.load()
    name, shape, ndim = C.create_string_buffer(64), (C.c_int32 * 4)(), C.c_int32()
    assert lib.mv_update_block_tensor_info(0, 0, name, shape, C.byref(ndim)) == L.MV_OK
    assert name.value == b"gru.convz1.weight" and tuple(shape) == (128, 512, 1, 5) and ndim.value == 4
    assert lib.mv_update_block_tensor_info(1, 13, name, shape, C.byref(ndim)) == L.MV_OK
    assert name.value == b"flow_head.0.bias" and tuple(shape) == (256, 0, 0, 0) and ndim.value == 1
    for kind, i in ((0, -1), (0, 24), (1, 20), (2, 0), (-1, 0)):
        assert lib.mv_update_block_tensor_info(kind, i, name, shape, C.byref(ndim)) == INVALID_ARG
    assert lib.mv_update_block_tensor_info(0, 0, None, shape, C.byref(ndim)) == INVALID_ARG
    assert lib.mv_update_block_tensor_info(0, 0, name, None, C.byref(ndim)) == INVALID_ARG
    assert lib.mv_update_block_tensor_info(0, 0, name, shape, None) == INVALID_ARG
    assert lib.mv_update_block_tensor_count(2) == 0

    for op in (L.MV_F16, L.MV_BF16):
        assert lib.mv_update_block_packed_bytes(0, op) >= 2 * N_PARAMS and lib.mv_update_block_packed_bytes(1, op) > 0
    assert lib.mv_update_block_packed_bytes(0, L.MV_F32) == 0 and lib.mv_update_block_packed_bytes(2, L.MV_BF16) == 0
    assert lib.mv_update_block_workspace_bytes(0, 2, 60, 80) == 2 * lib.mv_update_block_workspace_bytes(0, 1, 60, 80) > 0
    for B, H, W in ((0, 5, 7), (1, 0, 7), (1, 5, 0), (-1, 5, 7), (1, 1025, 1024), (65536, 65536, 1)):
        assert lib.mv_update_block_workspace_bytes(0, B, H, W) == 0
    assert lib.mv_update_block_workspace_bytes(2, 1, 5, 7) == 0 and lib.mv_update_block_workspace_bytes(1, 1, 1024, 1024) > 0

    # pack and forward refuse before anything touches the device (the pointers are never dereferenced)
    buf = torch.zeros(16)
    p = buf.data_ptr()
    ptrs = (C.c_void_p * 24)(*([p] * 24))
    assert lib.mv_update_block_pack(0, L.MV_BF16, None, p, None) == INVALID_ARG
    assert lib.mv_update_block_pack(0, L.MV_BF16, ptrs, None, None) == INVALID_ARG
    assert lib.mv_update_block_pack(2, L.MV_BF16, ptrs, p, None) == INVALID_ARG
    assert lib.mv_update_block_pack(0, L.MV_F32, ptrs, p, None) == INVALID_ARG
    ptrs[17] = None
    assert lib.mv_update_block_pack(0, L.MV_BF16, ptrs, p, None) == INVALID_ARG

    good = [0, L.MV_BF16, p, p, p, 1, 5, 7, 0, p, p, p, p, None]
    for idx in (2, 3, 4, 9, 10, 11, 12):                    # packed, net, inp, net_out, delta, mask, workspace
        args = list(good)
        args[idx] = None
        assert lib.mv_update_block_forward(*args) == INVALID_ARG
    for idx, bad in ((0, 2), (0, -1), (1, L.MV_F32), (1, 7), (5, 0), (6, 0), (7, 0), (6, -3), (8, 2), (5, 1 << 21)):
        args = list(good)
        args[idx] = bad
        assert lib.mv_update_block_forward(*args) == INVALID_ARG
    args = list(good)
    args[5:8] = [4, 1024, 1024]                             # B * H * W beyond 2^20 (and beyond int32 when multiplied by the channel count)
    assert lib.mv_update_block_forward(*args) == INVALID_ARG


def test_missing_and_misshaped_tensors_name_the_key():
    sd = T.make_block(T.COV, 0).state_dict()
    bad = {k: v for k, v in sd.items() if k != "cov_head.conv3.bias"}
    with pytest.raises(L.MacvoHipError, match=r"cov_head\.conv3\.bias"):
        ops.UpdateBlockWeights.from_module(bad, "cov", "bf16")
    bad = dict(sd)
    bad["gru.convq2.weight"] = torch.zeros(128, 512, 1, 5)
    with pytest.raises(L.MacvoHipError, match=r"gru\.convq2\.weight.*\(128, 512, 1, 5\)"):
        ops.UpdateBlockWeights.from_module(bad, "cov", "bf16")
    with pytest.raises(L.MacvoHipError, match=r"flow_head\.0\.weight"):
        ops.UpdateBlockWeights.from_module(T.make_block(T.COV, 0), "flow", "bf16")      # a CovUpdateBlock has no flow head
    with pytest.raises(L.MacvoHipError, match="kind"):
        ops.UpdateBlockWeights.from_module(sd, "gma", "bf16")
    with pytest.raises(L.MacvoHipError, match="operand"):
        ops.UpdateBlockWeights.from_module(sd, "cov", "f32")


def _stand_in():
    torch.manual_seed(0)
    return SimpleNamespace(memory_decoder=FH.MemoryCovDecoder(FH.demo_cfg()))


def test_hooks_leave_the_update_blocks_alone_by_default(monkeypatch):
    """``fuse_update_blocks=None`` with the environment variable unset returns today's list and rebinds nothing on the two blocks; the variable or the
    argument adds the four names; on the CPU (or in fp32) the rebound forwards run the original layers, bit for bit."""
    monkeypatch.delenv("MACVO_HIP_UPDATE_BLOCK", raising=False)
    today = ["memory_decoder.encode_flow_token", "memory_decoder.upsample_flow"]
    m = _stand_in()
    assert plugins.install_flowformer_hooks(m) == today
    assert plugins.install_flowformer_hooks(m, fuse_update_blocks=False) == today
    dec = m.memory_decoder
    for mod in (dec.cov_update, dec.update_block.gru, dec.update_block.flow_head, dec.update_block.mask):
        assert "forward" not in vars(mod)
    monkeypatch.setenv("MACVO_HIP_UPDATE_BLOCK", "0")
    assert plugins.install_flowformer_hooks(_stand_in()) == today

    extra = ["memory_decoder.cov_update.forward"] + [f"memory_decoder.update_block.{n}" for n in ("gru", "flow_head", "mask")]
    monkeypatch.setenv("MACVO_HIP_UPDATE_BLOCK", "1")
    assert plugins.install_flowformer_hooks(_stand_in()) == today + extra
    monkeypatch.delenv("MACVO_HIP_UPDATE_BLOCK")
    ref, m = _stand_in(), _stand_in()
    assert plugins.install_flowformer_hooks(m, fuse_update_blocks=True) == today + extra
    keys = list(ref.memory_decoder.state_dict())
    assert list(m.memory_decoder.state_dict()) == keys                                   # the modules stay in place
    net, inp = T.make_inputs((1, 5, 7), 0)
    with torch.no_grad():
        for a, b in zip(m.memory_decoder.cov_update(net, inp), ref.memory_decoder.cov_update(net, inp)):
            assert torch.equal(a, b)
        ub, rub = m.memory_decoder.update_block, ref.memory_decoder.update_block
        h, rh = ub.gru(net, inp), rub.gru(net, inp)
        assert torch.equal(h, rh) and torch.equal(ub.flow_head(h), rub.flow_head(rh)) and torch.equal(ub.mask(h), rub.mask(rh))

    # a block that does not have the published shapes is left alone
    odd = _stand_in()
    odd.memory_decoder.cov_update.cov_head.conv4 = torch.nn.Conv2d(64, 4, 3, padding=1)
    got = plugins.install_flowformer_hooks(odd, fuse_update_blocks=True)
    assert "memory_decoder.cov_update.forward" not in got and "memory_decoder.update_block.gru" in got
