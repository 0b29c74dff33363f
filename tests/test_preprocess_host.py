"""CPU: the frame-preprocessing plan (mv_preprocess_plan), the resampler's host twin, the transform plugins' config handling — against the restatement of
DataLoader/Transform.py in tests/preprocess_ref.py (torchvision restated, parity-unpinned)."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import preprocess_ref as R
from tests import resample_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATASET_PAIRS = [(1241, 780), (1920, 1137), (1226, 780), (752, 640), (1080, 640), (376, 236), (1250, 1240), (379, 375), (40, 19), (27, 12)]


def _K(fx=320.5, fy=318.25, cx=321.75, cy=240.125):
    return torch.tensor([[[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]], dtype=torch.float32)


def _frame(H, W, seed=0, B=1):
    g = torch.Generator().manual_seed(seed)
    return R.stereo(torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g), _K().repeat(B, 1, 1),
                    gt_flow=torch.randn(B, 2, H, W, generator=g) * 5, flow_mask=torch.rand(B, 1, H, W, generator=g) > 0.4,
                    gt_depth=torch.rand(B, 1, H, W, generator=g) * 30 + 0.5)


# ------------------------------------------------------------------------------------------------- the restatement checks itself
def test_restatement_unit_scale_is_identity():
    d = _frame(21, 34)
    o = R.scale_stereo(R.apply(d, []), 1.0, 1.0, "bilinear")
    for n in ("imageL", "imageR", "gt_flow", "flow_mask", "gt_depth", "K"):
        assert torch.equal(getattr(o, n), getattr(d, n)), n


def test_restatement_kitti_is_a_crop():
    g = torch.Generator().manual_seed(1)
    d = R.stereo(torch.rand(1, 3, 376, 1241, generator=g), torch.rand(1, 3, 376, 1241, generator=g), _K(cx=609.5593, cy=172.854))
    o = R.smart_resize(R.apply(d, []), 376, 780, "nearest")
    assert torch.equal(o.imageL, d.imageL[..., :, 230:1010]) and torch.equal(o.imageR, d.imageR[..., :, 230:1010])
    assert o.K[0, 0, 2] == d.K[0, 0, 2] - 230.5 and o.K[0, 1, 2] == d.K[0, 1, 2] and (o.height, o.width) == (376, 780)
    assert torch.equal(o.K[0, :, :2], d.K[0, :, :2])


def test_restatement_short_by_one_pads_a_zero_row():
    d = _frame(27, 40)
    o = R.smart_resize(R.apply(d, []), 13, 16, "nearest")
    assert o.imageL.shape[-2:] == (13, 16)
    assert (o.imageL[..., -1, :] == 0).all() and (o.gt_depth[..., -1, :] == 0).all() and not o.flow_mask[..., -1, :].any()
    assert (o.imageL[..., :-1, :] != 0).any()


def test_formula_equals_torch_fp64():
    g = torch.Generator().manual_seed(2)
    for (h, w), size in (((37, 53), (13, 20)), ((20, 30), (33, 41)), ((48, 64), (31, 80)), ((30, 47), (30, 20))):
        x = torch.rand(1, 2, h, w, generator=g, dtype=torch.float64)
        ref = F.interpolate(x, size=list(size), mode="bilinear", align_corners=False, antialias=True)
        assert (R.aa_resize_f64(x, size) - ref).abs().max() < 1e-14


# ------------------------------------------------------------------------------------------------- mv_preprocess_plan
def _sweep_sizes():
    sizes = []
    for H in range(14, 701):
        for ar in (1.0, 1.5, 16 / 9, 3.3):
            sizes.append((H, int(round(H * ar))))
    return sizes + [(1080, 1920), (370, 1226), (376, 1241), (480, 752)]


def test_plan_equals_restatement_over_the_sweep():
    """SmartResizeFrame's plan == the Python restatement: resized size, output size, crop origin, pads, round scales and the bits of K."""
    from macvo_amd import ops

    K = _K()
    short, odd, cases = 0, 0, 0
    for (H, W) in _sweep_sizes():
        for (th, tw) in ((13, 16), (376, 780), (480, 640), (640, 640)):
            rs, org, pads, Kr = R.smart_geometry(H, W, th, tw, K)
            p = ops.preprocess_plan(H, W, "smart", K=K, height=th, width=tw, interp="nearest")
            assert p.resized == rs and (p.height, p.width) == (th, tw) and p.origin == org and p.pads == pads, (H, W, th, tw)
            assert torch.equal(p.K.view(torch.int32), Kr.view(torch.int32)), (H, W, th, tw)
            ru, rv = np.float32(W / rs[1]), np.float32(H / rs[0])
            assert p.round_scale == (float(ru), float(rv)) or rs == (H, W), (H, W, th, tw)
            short += rs[0] == th - 1 or rs[1] == tw - 1
            odd += (rs[0] - th) % 2 == 1 or (rs[1] - tw) % 2 == 1
            cases += 1
    assert short > 100 and odd > 100 and cases == len(_sweep_sizes()) * 4, (short, odd, cases)


def test_plan_scale_and_crop_alone_and_half_to_even():
    from macvo_amd import ops

    K = _K()
    # ScaleFrame 2.5 / 1.5 on 53 x 175: int(53 / 1.5) = 35, int(175 / 2.5) = 70
    p = ops.preprocess_plan(53, 175, "scale", K=K, scale_u=2.5, scale_v=1.5, interp="bilinear")
    d = R.scale_stereo(R.stereo(torch.zeros(1, 3, 53, 175), torch.zeros(1, 3, 53, 175), K), 2.5, 1.5, "nearest")
    assert (p.height, p.width) == (35, 70) == (d.height, d.width) and torch.equal(p.K.view(torch.int32), d.K.view(torch.int32))
    # CenterCropFrame: (1241 - 780) / 2 = 230.5 -> 230, (1243 - 780) / 2 = 231.5 -> 232 (half to even); K takes the un-rounded value
    for W, left in ((1241, 230), (1243, 232), (1242, 231)):
        p = ops.preprocess_plan(376, W, "crop", K=K, height=376, width=780)
        d = R.crop_stereo(R.stereo(torch.zeros(1, 1, 376, W), torch.zeros(1, 1, 376, W), K), 376, 780)
        assert p.c.win_x0 == left and p.origin == (0, left) and p.pads == (0, 0, 0, 0) and torch.equal(p.K.view(torch.int32), d.K.view(torch.int32))
    # a crop larger than the frame on one axis pads: (43 - 40) // 2 = 1 column in front, (43 - 40 + 1) // 2 = 2 behind; the other axis is cut
    p = ops.preprocess_plan(30, 40, "crop", K=K, height=20, width=43)
    assert p.pads == (0, 0, 1, 2) and p.origin == (5, 0) and (p.c.win_y0, p.c.win_x0) == (5, -1)
    # a target of zero rows is the reference's ZeroDivisionError
    with pytest.raises(Exception):
        ops.preprocess_plan(4, 40, "scale", K=K, scale_u=8.0, scale_v=8.0, interp="nearest")
    # a batch of intrinsics: every matrix goes through the same fp32 steps
    Kb = torch.cat([_K(), _K(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)])
    p = ops.preprocess_plan(370, 1226, "smart", K=Kb, height=376, width=780, interp="nearest")
    for b in range(2):
        assert torch.equal(p.K[b].view(torch.int32), R.smart_geometry(370, 1226, 376, 780, Kb[b:b + 1])[3][0].view(torch.int32))


def test_plan_chains_and_refuses_what_does_not_fold():
    from macvo_amd import ops

    K = _K()
    p = ops.preprocess_plan(60, 90, "crop", K=K, height=48, width=64).then("cast", dtype="fp16").then("scale", scale_u=2.0, scale_v=1.5, interp="bilinear")
    d = R.stereo(torch.zeros(1, 1, 60, 90), torch.zeros(1, 1, 60, 90), K)
    d = R.apply(d, [("crop", dict(height=48, width=64)), ("cast", dict(dtype="fp16")), ("scale", dict(scale_u=2.0, scale_v=1.5, interp="bilinear"))])
    assert (p.height, p.width) == (d.height, d.width) == (32, 32) and torch.equal(p.K.view(torch.int32), d.K.view(torch.int32))
    assert p.out_dtype == torch.float16 and p.c.mid_dtype == p.c.out_dtype and (p.c.win_h, p.c.win_w, p.c.win_y0, p.c.win_x0) == (48, 64, 6, 13)
    with pytest.raises(ops.PlanDoesNotFold):
        p.then("scale", scale_u=2.0, scale_v=2.0, interp="nearest")
    with pytest.raises(ops.PlanDoesNotFold):
        p.then("cast", dtype="bf16")
    q = p.then("scale", scale_u=1.0, scale_v=1.0, interp="nearest").then("crop", height=40, width=20)      # a unit scale folds into anything
    assert (q.height, q.width, q.pads, q.origin) == (40, 20, (4, 4, 0, 0), (0, 6))


# ------------------------------------------------------------------------------------------------- host twin
_TORCH_INDICES = r"""
import json, sys, torch, torch.nn.functional as F
pairs = [(i, o) for i in range(1, 201) for o in range(1, 201)] + json.loads(sys.argv[1])
out = []
for i, o in pairs:
    x = torch.arange(i, dtype=torch.float32).view(1, 1, 1, i)
    out.append(F.interpolate(x, size=(1, o), mode="nearest-exact")[0, 0, 0].to(torch.int32))
torch.save(torch.cat(out), sys.argv[2])
"""


def test_twin_nearest_indices_equal_torch(tmp_path):
    """Every (in, out) pair in 1..200 and the dataset pairs: the twin's source index == F.interpolate(mode="nearest-exact").

    torch is asked in a child process with ATEN_CPU_CAPABILITY=default: its nearest-exact kernel is `floorf((dst + 0.5) * scale)` in its source, and that build
    computes exactly this.  The AVX2 / AVX512 builds of the same source contract part of the row into a fused multiply-add and then differ from their own
    scalar lanes at exact ties ((dst + 0.5) * in / out an integer while float(in) / float(out) is rounded down): 10 of the 4 030 000 indices of this sweep
    (in 2..8, out 141..194) on the AVX512 machine this was written on, a set that changes with the tensor's shape; the in-process count is printed."""
    pairs = [(i, o) for i in range(1, 201) for o in range(1, 201)] + DATASET_PAIRS
    f = tmp_path / "idx.pt"
    env = dict(os.environ, ATEN_CPU_CAPABILITY="default")
    subprocess.run([sys.executable, "-c", _TORCH_INDICES, json.dumps(DATASET_PAIRS), str(f)], check=True, env=env)
    ref = torch.load(f).numpy()
    mine = np.concatenate([T.nearest(i, o) for i, o in pairs])
    assert mine.shape == ref.shape and np.array_equal(mine, ref), int((mine != ref).sum())
    here = 0
    for i, o in pairs:
        x = torch.arange(i, dtype=torch.float32).view(1, 1, 1, i)
        here += int((F.interpolate(x, size=(1, o), mode="nearest-exact")[0, 0, 0].numpy().astype(np.int32) != T.nearest(i, o)).sum())
    print(f"nearest-exact: {here} of {mine.size} indices differ from this process's torch build ({torch.backends.cpu.get_cpu_capability()})")


def test_twin_antialias_windows_and_weights():
    """xmin / xsize == the fp64 formula's exactly; the fp32 weights are the fp64 values rounded once."""
    pairs = DATASET_PAIRS + [(37, 13), (53, 20), (48, 31), (64, 47), (20, 33), (30, 41), (135, 17), (240, 30), (9, 9), (3, 200), (200, 3), (1, 7), (7, 1)]
    pairs += [(i, o) for i in range(1, 41) for o in range(1, 41)]
    for n_in, n_out in pairs:
        xmin, xsize, w = T.aa(n_in, n_out, cap=max(8, 2 * (n_in // n_out + 2) + 1))
        for i in range(n_out):
            rmin, rsize = R.aa_window(i, n_in, n_out)
            assert (xmin[i], xsize[i]) == (rmin, rsize), (n_in, n_out, i)
            rw = R.aa_weights(i, n_in, n_out)
            assert np.array_equal(w[i, :rsize], rw.astype(np.float32)) or np.abs(w[i, :rsize] - rw).max() <= 2.0 ** -24, (n_in, n_out, i)
            assert (w[i, rsize:] == 0).all()
    # the kernel's tap budget covers every window at its largest supported downscale
    lib = T.build()
    for n_out in range(1, 40):
        assert T.aa(8 * n_out, n_out)[1].max() <= lib.resample_twin_max_taps() and lib.resample_twin_max_scale() == 8


def test_twin_standalone_under_sanitizers():
    assert "resample_twin OK" in T.run_standalone_sanitized()


# ------------------------------------------------------------------------------------------------- plugins (host side)
def test_config_key_sets_are_the_references():
    from macvo_amd import transforms as X

    ok = {
        X.HIP_ScaleFrame: dict(scale_u=2, scale_v=1.5, interp="nearest"),
        X.HIP_CenterCropFrame: dict(height=376, width=780),
        X.HIP_SmartResizeFrame: dict(height=376, width=780, interp="bilinear"),
        X.HIP_CastDataType: dict(dtype="bf16"),
    }
    for cls, args in ok.items():
        cls.is_valid_config(SimpleNamespace(**args))
        X.IDataTransform.is_valid_config(SimpleNamespace(type=cls.__name__, args=SimpleNamespace(**args)))
        with pytest.raises(KeyError):                                  # an extra key
            cls.is_valid_config(SimpleNamespace(**args, extra=1))
        for k in args:                                                 # a missing key
            with pytest.raises(KeyError):
                cls.is_valid_config(SimpleNamespace(**{q: v for q, v in args.items() if q != k}))
    for cls, bad in ((X.HIP_ScaleFrame, dict(scale_u=0, scale_v=1, interp="nearest")), (X.HIP_ScaleFrame, dict(scale_u=1, scale_v=1, interp="bicubic")),
                     (X.HIP_CenterCropFrame, dict(height=376.0, width=780)), (X.HIP_SmartResizeFrame, dict(height=0, width=780, interp="nearest")),
                     (X.HIP_CastDataType, dict(dtype="fp64"))):
        with pytest.raises(ValueError):
            cls.is_valid_config(SimpleNamespace(**bad))


def test_smart_transform_folds_a_list_into_one_plan():
    from macvo_amd import transforms as X

    class Seq:
        def __init__(self):
            self.fns = None

        @staticmethod
        def name():
            return "KITTI"

        def transform(self, fns):
            self.fns = fns
            return self

    cfg = [dict(type="CenterCropFrame", args=dict(height=48, width=64)), dict(type="CastDataType", args=dict(dtype="fp16")),
           dict(type="ScaleFrame", args=dict(scale_u=2.0, scale_v=1.5, interp="bilinear"))]
    seq = X.smart_transform(Seq(), cfg)
    assert len(seq.fns) == 1
    plans = seq.fns[0].plans(60, 90, _K())
    assert len(plans) == 1 and (plans[0].height, plans[0].width) == (32, 32) and plans[0].out_dtype == torch.float16
    # two real resizes do not fold: two plans, the second planned on the first's output and K
    two = X.instantiate_transforms(cfg + [dict(type="HIP_SmartResizeFrame", args=dict(height=16, width=20, interp="nearest"))])
    assert len(two) == 1 and [(p.height, p.width) for p in two[0].plans(60, 90, _K())] == [(32, 32), (16, 20)]
    # the lookup by sequence type; a type the block does not name is left alone
    block = dict(KITTI=[dict(type="SmartResizeFrame", args=dict(height=376, width=780, interp="nearest"))], Zed=[])
    assert len(X.smart_transform(Seq(), block).fns) == 1
    other = Seq()
    other.name = lambda: "TartanAir"
    assert X.smart_transform(other, block) is other and other.fns is None

    # any other transform passes through unfused, between the folded runs
    class Flip(X.IDataTransform):
        def forward(self, frame):
            return frame

    mixed = X.fold_transforms([X.HIP_CenterCropFrame(SimpleNamespace(height=8, width=8)), X.HIP_CastDataType(SimpleNamespace(dtype="fp32")), Flip(None),
                               X.HIP_ScaleFrame(SimpleNamespace(scale_u=2, scale_v=2, interp="nearest"))])
    assert [type(t).__name__ for t in mixed] == ["_FoldedTransform", "Flip", "_FoldedTransform"]


def test_preprocess_config_fields_kitti_camera():
    from macvo_amd.pipeline import Camera, preprocess_config_fields

    block = SimpleNamespace(KITTI=[SimpleNamespace(type="SmartResizeFrame", args=SimpleNamespace(height=376, width=780, interp="nearest"))])
    cam = Camera(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, baseline=0.537, H=376, W=1241)
    out = preprocess_config_fields(block, "KITTI", cam)
    assert len(out["plans"]) == 1 and (out["camera"].H, out["camera"].W) == (376, 780)
    assert out["camera"].cx == float(torch.tensor(607.1928) - 230.5) and out["camera"].fx == float(torch.tensor(718.856)) and out["camera"].baseline == 0.537
    assert preprocess_config_fields(block, "TartanAir", cam) == {"plans": [], "camera": cam}
    with pytest.raises(ValueError):
        preprocess_config_fields([dict(type="AddImageNoise", args=dict(stdv=1.0))], "KITTI", cam)


def test_abi_stays_8_and_the_new_symbols_resolve():
    import macvo_amd._lib as L

    lib = L.load()
    assert lib.mv_abi_version() == 8 == L.ABI_VERSION
    assert lib.mv_preprocess_plan and lib.mv_preprocess_lanes
    import ctypes as C

    assert C.sizeof(L.mvPreprocessPlan) == 4 * (24 + 2 + 9) and C.sizeof(L.mvPreprocessGroup) == 48
    # the launch refuses before it launches: no GPU is needed to see a bilinear downscale above 8 or a broken plan turned away
    p = L.mvPreprocessPlan()
    assert lib.mv_preprocess_plan(C.byref(p), None, 135, 240, None, L.MV_PP_SCALE, 8.5, 8.5, L.MV_PP_BILINEAR) == 0
    g = L.mvPreprocessGroup(src=16, dst=16, src_lane_stride=135 * 240, dst_lane_stride=15 * 28, planes=1, kind=L.MV_PP_DEPTH, src_dtype=L.MV_F32,
                            dst_dtype=L.MV_F32)
    assert lib.mv_preprocess_lanes(C.byref(p), C.byref(g), 1, 1, None) == -2
    p.win_vx1 = 10 ** 6
    assert lib.mv_preprocess_lanes(C.byref(p), C.byref(g), 1, 1, None) == -1
