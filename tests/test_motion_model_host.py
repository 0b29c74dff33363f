"""CPU: the torch restatement of TartanMotionNet (tests/motion_model_ref.py) reproduces the reference's own preprocessing and
predict / update recorded in tests/golden/motion_model.npz bit for bit; the fp32 se3 Exp + compose of mac-vo_amd/csrc/motion_dev.h,
built for the host, against the PyPose shim; the `motion` mapping of HotPathConfig; the plugin's registration and config spec."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import motion_model_ref as R
from tests.golden import make_golden_motion_model as G
from tests.golden import pypose_shim as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "motion_model.npz")


@pytest.fixture(scope="module")
def g():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name,H,W,seed,special", G.CASES)
def test_restated_motion_input_matches_reference_golden(g, name, H, W, seed, special):
    cam = [float(v) for v in g["cam"]]
    flow, depth = G.inputs(H, W, seed, special)
    x = R.motion_input(flow, depth, *cam)
    assert x.shape == (1, 5, 112, 160) and x.dtype == torch.float32
    sample = x.reshape(-1)[G.sample_idx(x.numel())]
    ref = torch.from_numpy(g[f"{name}_sample"])
    assert torch.equal(sample.view(torch.int32) if not torch.isnan(sample).any() else sample.nan_to_num(7.0).view(torch.int32),
                       ref.view(torch.int32) if not torch.isnan(ref).any() else ref.nan_to_num(7.0).view(torch.int32))
    assert hashlib.sha256(x.contiguous().numpy().tobytes()).hexdigest() == str(g[f"{name}_sha"])
    raw = G.StandInPoseNet()(x).squeeze() * torch.tensor(R.POSE_NORM)
    assert torch.equal(raw, torch.from_numpy(g[f"{name}_raw"]))
    if special:   # the special depths reach the depth channel as zeros (NaN / negative / inf) and huge values (zero depth)
        assert bool((x[0, 2] == 0).any()) and float(x[0, 2].max()) > 1e30


def test_restated_predict_update_matches_reference_golden(g):
    cam = [float(v) for v in g["cam"]]
    m = R.MotionModelRef(G.StandInPoseNet(), pp, "cpu")
    poses = [m.predict(None, None, *cam)]
    for k in range(1, G.SEQ_FRAMES):
        m.update(G.seq_update(poses[-1], k))
        flow, depth = G.seq_inputs(k)
        poses.append(m.predict(flow, depth, *cam).clone())
    assert torch.equal(torch.stack(poses), torch.from_numpy(g["seq_poses"]))


def test_host_intrinsic_channels_keep_the_swapped_arguments(host):
    """make_device_intrinsic_layer(height, width, fx, fy, cx, cy): channel 3 of the PoseNet input runs along columns with (fy, cy), channel 4
    along rows with (fx, cx) — the reference's quirk, as motion_dev.h computes it (a copy-path 112x160 frame: the taps are the layer itself),
    against the reference's own layer restated in torch."""
    fx, fy, cx, cy = 2.0, 4.0, 1.0, 3.0
    lay = R.intrinsic_layer(112, 160, fx, fy, cx, cy, "cpu")          # [H, W, 2]
    out = (C.c_float * (2 * 112 * 160))()
    host.intrinsic(112, 160, C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy), out)
    got = torch.frombuffer(bytearray(out), dtype=torch.float32).reshape(2, 112, 160)
    # (torch's CPU division is a true division, the device one multiplies by the reciprocal: compare at one rounding)
    torch.testing.assert_close(got, lay.permute(2, 0, 1), rtol=2.0 ** -22, atol=0)
    assert float(got[0, 0, 5]) == (5 - cy + 0.5) * (1.0 / fy) and float(got[1, 7, 0]) == (7 - cx + 0.5) * (1.0 / fx)


_HOST_SRC = r'''
#include "motion_dev.h"
extern "C" void compose(int n, const float* prev, const float* raw, const float* norm, float* out) {
    for (int i = 0; i < n; ++i) motion::pose_exp_compose(prev + 7 * i, raw + 6 * i, norm, out + 7 * i);
}
extern "C" void intrinsic(int H, int W, float fx, float fy, float cx, float cy, float* out) {   // channels 3 and 4 of the PoseNet input
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            out[r * W + c] = motion::intrinsic_at(c, cy, 1.0f / fy);
            out[H * W + r * W + c] = motion::intrinsic_at(r, cx, 1.0f / fx);
        }
}
extern "C" void axis(int size, int target, int out, int* off_len, float* scale) {
    motion::Axis a = motion::axis_of(size, target, out);
    off_len[0] = a.off; off_len[1] = a.len; *scale = a.scale;
}
'''


@pytest.fixture(scope="module")
def host():
    d = tempfile.mkdtemp(prefix="motion_dev_")
    src = os.path.join(d, "motion_host.cpp")
    with open(src, "w") as f:
        f.write(_HOST_SRC)
    so = os.path.join(d, "libmotion_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "mac-vo_amd", "csrc"), "-I", os.path.join(ROOT, "include"), src, "-o", so], check=True)
    return C.CDLL(so)


def _host_compose(lib, prev, raw):
    prev, raw = prev.float().contiguous(), raw.float().contiguous()
    out = torch.empty_like(prev)
    norm = torch.tensor(R.POSE_NORM, dtype=torch.float32)
    lib.compose(prev.shape[0], C.c_void_p(prev.data_ptr()), C.c_void_p(raw.data_ptr()), C.c_void_p(norm.data_ptr()), C.c_void_p(out.data_ptr()))
    return out


def test_host_compose_against_shim(host):
    gen = torch.Generator().manual_seed(5)
    n = 64
    t = torch.randn(n, 3, generator=gen) * 3
    q = torch.randn(n, 4, generator=gen)
    prev = torch.cat([t, q / q.norm(dim=1, keepdim=True)], 1).float()
    raw = torch.randn(n, 6, generator=gen)
    raw[:16] *= 1e-6     # |phi| < fp32 eps: the Taylor branch
    raw[16:40] *= 30     # large angles
    raw[40:48] = 0.0     # zero motion
    out = _host_compose(host, prev, raw)
    ref64 = R.compose(prev.double(), raw.double(), pp)
    ref32 = R.compose(prev, raw, pp)
    assert (out.double() - ref64).abs()[:, :3].max() <= 64 * 2.0 ** -23 * 10
    assert (out.double() - ref64).abs()[:, 3:].max() <= 16 * 2.0 ** -23
    assert (out - ref32).abs().max() <= 64 * 2.0 ** -23 * 10
    assert torch.equal(out[40:48], prev[40:48])     # zero motion: the previous pose bit for bit


@pytest.mark.parametrize("size,target,off,length", [(480, 448, 16, 448), (485, 448, 18, 449), (640, 640, 0, 640), (651, 640, 5, 641),
                                                    (113, 112, 0, 113)])
def test_host_crop_axis(host, size, target, off, length):
    ol = (C.c_int * 2)()
    sc = C.c_float()
    host.axis(size, target, 112, ol, C.byref(sc))
    assert (ol[0], ol[1]) == (off, length)
    assert sc.value == float(np.float32(length - 1) / np.float32(111))


PAPER_MOTION = {"type": "TartanMotionNet", "args": {"weight": "./Model/MACVO_posenet.pkl", "device": "cuda"}}


def test_motion_config_fields():
    from macvo_amd.pipeline import HotPathConfig, motion_config_fields

    assert motion_config_fields(PAPER_MOTION) == {"motion_model": "tartan"}
    assert motion_config_fields(SimpleNamespace(type="TartanMotionNet", args=SimpleNamespace(weight="", device="cuda"))) == {"motion_model": "tartan"}
    assert motion_config_fields({"type": "StaticMotionModel", "args": None}) == {"motion_model": "static"}
    assert motion_config_fields({"type": "HIP_TartanMotionNet", "args": {}}) == {"motion_model": "tartan"}
    with pytest.raises(ValueError):
        motion_config_fields({"type": "GTMotionwithNoise", "args": {"noise_std": 0.0}})
    assert HotPathConfig().motion_model == "static"
    assert HotPathConfig(**motion_config_fields(PAPER_MOTION)).motion_model == "tartan"


def test_paper_yaml_motion_blocks():
    """Paper_Reproduce.yaml and every Ablation_Study/TartanAirv2_*.yaml name TartanMotionNet (where the reference checkout exists)."""
    import glob

    import yaml

    from macvo_amd.pipeline import motion_config_fields

    from tests.test_reference_abcs import REF

    base = os.path.join(REF, "Config", "Experiment", "MACVO")
    files = [os.path.join(base, "Paper_Reproduce.yaml")] + sorted(glob.glob(os.path.join(base, "Ablation_Study", "TartanAirv2_*.yaml")))
    files = [f for f in files if os.path.exists(f)]
    if not files:
        pytest.skip("needs the reference checkout (build container only)")
    for f in files:
        txt = open(f).read()
        cfg = yaml.load(txt, Loader=_loader())
        motion = _find(cfg, "motion")
        assert motion is not None, f
        assert motion_config_fields(motion) == {"motion_model": "tartan"}, f


def _loader():
    import yaml

    class L(yaml.SafeLoader):
        pass

    L.add_multi_constructor("!", lambda loader, suffix, node: None)
    return L


def _find(d, key):
    if isinstance(d, dict):
        if key in d and isinstance(d[key], dict) and "type" in d[key]:
            return d[key]
        for v in d.values():
            r = _find(v, key)
            if r is not None:
                return r
    return None


def test_plugin_registration_and_config_spec():
    from macvo_amd import interfaces as I
    from macvo_amd import plugins

    cls = plugins.HIP_TartanMotionNet
    assert issubclass(cls, I.IMotionModel)
    assert I.IMotionModel.__subclasses__() and cls in I.IMotionModel.__subclasses__()
    cls.is_valid_config(SimpleNamespace(weight="", device="cuda"))
    cls.is_valid_config(SimpleNamespace(weight="./Model/MACVO_posenet.pkl", device="cuda:0"))
    for bad in (SimpleNamespace(weight=3, device="cuda"), SimpleNamespace(weight="", device="tpu"), SimpleNamespace(device="cuda")):
        with pytest.raises((AssertionError, ValueError, KeyError)):
            cls.is_valid_config(bad)
