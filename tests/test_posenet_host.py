"""The PoseNet forward off the GPU: the seeded weight generator and the torch restatement against the reference class's golden, the
library's tensor table, the host twin of the kernels (packing, borders, strides, reduction order) against the fp64 restatement,
checkpoint loading and the argument checks of the new entry points."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest
import torch

from macvo_amd import _lib as L
from macvo_amd import ops
from tests import posenet_twin as T
from tools import posenet_torch as PT

INVALID_ARG = -1     # MV_ERR_INVALID_ARG (include/macvo_hip.h)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posenet.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("seed", T.WEIGHT_SEEDS)
def test_seeded_weights_reproduce_the_golden_digest(golden, seed):
    assert tuple(golden["weight_seeds"]) == T.WEIGHT_SEEDS and int(golden["input_seed"]) == T.INPUT_SEED
    sha = PT.state_dict_sha256(PT.seeded_state_dict(seed))
    assert sha == str(golden[f"s{seed}_sha"]), (
        f"seeded_state_dict({seed}) no longer generates the weights the golden was made with (torch's generator or the recipe changed): "
        "every comparison against tests/golden/posenet.npz is void until it is regenerated")


@pytest.mark.parametrize("seed", T.WEIGHT_SEEDS)
def test_restatement_equals_the_reference_class(golden, seed):
    """tools/posenet_torch.py against the reference's own VOFlowRes: fp32 bit for bit (same torch ops on the same machine), fp64 within 1e-12."""
    sd, x, y64, st64, _ = T.case(seed, 3)
    assert PT.state_dict_sha256(sd) == str(golden[f"s{seed}_sha"])
    with torch.no_grad():
        y32, st32 = PT.from_state_dict(sd)(x, return_stages=True)
    assert np.array_equal(y32.numpy(), golden[f"s{seed}_f32_out"])
    g64 = golden[f"s{seed}_f64_out"]
    assert np.abs(y64.numpy() - g64).max() <= 1e-12 * np.abs(g64).max()
    for name, a32, a64 in zip(PT.STAGES, st32, st64):
        idx = PT.sample_index(a32.numel())
        assert np.array_equal(a32.reshape(-1)[idx].numpy(), golden[f"s{seed}_f32_{name}"]), name
        g = golden[f"s{seed}_f64_{name}"]
        assert np.abs(a64.reshape(-1)[idx].numpy() - g).max() <= 1e-12 * np.abs(g).max(), name


def test_tensor_table_is_the_modules_state_dict():
    lib = L.load()
    assert lib.mv_posenet_tensor_count() == 120
    table = ops.posenet_tensor_table()
    assert table == PT.tensor_table()
    assert sum(int(np.prod(s)) for _, s in table) == PT.N_PARAMS == 15135430
    assert lib.mv_posenet_packed_bytes() >= 4 * 15135430
    assert ops.POSENET_STAGE_SHAPES == PT.STAGE_SHAPES and ops.POSENET_STAGES == PT.STAGES
    assert lib.mv_abi_version() == 8


@pytest.mark.parametrize("seed", T.WEIGHT_SEEDS)
def test_host_twin_meets_the_tolerance(seed):
    """The kernels' plan, packed layout and per-output fmaf order, replayed on the host for one lane, against the fp64 restatement: output and
    all six stages within 16 x the error of torch's own fp32 CPU forward."""
    ref = T.case(seed, 1)
    y, stages = T.forward(T.pack(ref[0]), ref[1])
    T.check_against_fp64(f"host twin, seed {seed}", y, stages, ref)


# ------------------------------------------------------------------------------------------------------------ checkpoint loading
class _HostPoseNet(ops.PoseNet):
    """ops.PoseNet whose packed weights stay on the host (the checks below need no GPU)."""

    def __init__(self, state_dict, device="cpu"):
        super().__init__(state_dict, "cpu")


def test_checkpoint_layouts_load(tmp_path):
    sd = PT.seeded_state_dict(11)
    ck = {"module.flowPoseNet." + k: v for k, v in sd.items()}
    ck["module.flowNet.conv1.weight"] = torch.zeros(4, 3, 3, 3)
    ck["module.stereoNet.conv1.weight"] = torch.zeros(2, 2)
    path = tmp_path / "posenet.pkl"
    torch.save(ck, path)
    ref = T.pack(sd)
    assert torch.equal(_HostPoseNet.from_file(str(path)).packed, ref)
    assert torch.equal(_HostPoseNet.from_state_dict({"flowPoseNet." + k: v for k, v in sd.items()}).packed, ref)
    assert torch.equal(_HostPoseNet.from_state_dict(sd).packed, ref)
    assert torch.equal(_HostPoseNet.from_module(PT.from_state_dict(sd)).packed, ref)


def test_missing_and_misshaped_tensors_name_the_key():
    sd = PT.seeded_state_dict(11)
    bad = {"module.flowPoseNet." + k: v for k, v in sd.items() if k != "layer3.0.downsample.bias"}
    with pytest.raises(L.MacvoHipError, match=r"layer3\.0\.downsample\.bias"):
        _HostPoseNet.from_state_dict(bad)
    bad = dict(sd)
    bad["voflow_rot.1.0.weight"] = torch.zeros(32, 127)
    with pytest.raises(L.MacvoHipError, match=r"voflow_rot\.1\.0\.weight.*\(32, 127\)"):
        _HostPoseNet.from_state_dict(bad)


# --------------------------------------------------------------------------------------------------------------- argument checks
def test_entry_points_check_their_arguments():
    lib = L.load()
    name, shape, ndim = C.create_string_buffer(64), (C.c_int32 * 4)(), C.c_int32()
    assert lib.mv_posenet_tensor_info(0, name, shape, C.byref(ndim)) == L.MV_OK
    assert name.value == b"firstconv.0.0.weight" and tuple(shape) == (32, 5, 3, 3) and ndim.value == 4
    for i in (-1, 120):
        assert lib.mv_posenet_tensor_info(i, name, shape, C.byref(ndim)) == INVALID_ARG
    assert lib.mv_posenet_tensor_info(0, None, shape, C.byref(ndim)) == INVALID_ARG
    assert lib.mv_posenet_tensor_info(0, name, None, C.byref(ndim)) == INVALID_ARG
    assert lib.mv_posenet_tensor_info(0, name, shape, None) == INVALID_ARG
    assert lib.mv_posenet_workspace_bytes(0) == 0 and lib.mv_posenet_workspace_bytes(65) == 0
    assert lib.mv_posenet_workspace_bytes(64) == 64 * lib.mv_posenet_workspace_bytes(1) > 0

    buf = torch.zeros(16)
    ptrs = (C.c_void_p * 120)(*([buf.data_ptr()] * 120))
    assert lib.mv_posenet_pack(None, buf.data_ptr()) == INVALID_ARG
    assert lib.mv_posenet_pack(ptrs, None) == INVALID_ARG
    ptrs[57] = None
    assert lib.mv_posenet_pack(ptrs, buf.data_ptr()) == INVALID_ARG     # a null tensor: refused before anything is read

    # the forward refuses before it launches (the pointers are never dereferenced on the host)
    p = buf.data_ptr()
    for lanes in (0, 65, -1):
        assert lib.mv_posenet_forward_lanes(p, p, lanes, p, p, None, None) == INVALID_ARG
    for k in range(4):
        args = [p, p, 1, p, p, None, None]
        args[(0, 1, 3, 4)[k]] = None
        assert lib.mv_posenet_forward_lanes(*args) == INVALID_ARG
