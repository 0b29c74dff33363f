"""GPU: stereo rectification — the remap kernel (``mv_remap_lanes``) against its host twin bit for bit, the map builder (``mv_rectify_maps``) against the fp64
formula of ``tests/rectify_ref.py``, ``StereoRectifier`` end to end on the EuRoC rig and chained into ``ops.preprocess``, and what the launch refuses.

The remap is a pure integer gather, so every comparison of it is for equality.  Float destinations are ``torch.tensor(u8, dtype=float32) / 255`` (a true
division), rounded once more by ``.to(dtype)`` for fp16 / bf16."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import preprocess_ref as PR
from tests import rectify_cases as RC
from tests import rectify_ref as RR
from tests import remap_twin as TW

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _as_dtype(u8: np.ndarray, dtype) -> torch.Tensor:
    t = torch.from_numpy(u8)
    if dtype == torch.uint8:
        return t
    f = torch.tensor(u8, dtype=torch.float32) / 255
    return f if dtype == torch.float32 else f.to(dtype)


_MAPS = {}


def _maps(per_lane: bool, seed: int):
    key = (per_lane, seed)
    if key not in _MAPS:
        _MAPS[key] = RC.crafted_maps(lanes=RC.LANES if per_lane else None, seed=seed)
    return _MAPS[key]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float16, torch.bfloat16], ids=["u8", "f32", "f16", "bf16"])
@pytest.mark.parametrize("per_lane", [False, True], ids=["shared_map", "lane_maps"])
@pytest.mark.parametrize("reverse", [False, True], ids=["keep", "reverse"])
@pytest.mark.parametrize("channels,layout", [(1, "hwc"), (1, "planar"), (3, "hwc"), (3, "planar")])
def test_remap_is_bit_exact(gpu, channels, layout, reverse, per_lane, dtype):
    """Source 37 x 53, output 29 x 61, 3 lanes, two groups (their own images and maps) in one launch; maps random within [-3, size + 3] plus the crafted
    entries of tests/rectify_cases.py: ties to even, (-1, 0), the right and lower border, -1.0, 1e9, +-inf, NaN."""
    from macvo_amd import ops

    srcs = [RC.images(channels, layout, seed=1), RC.images(channels, layout, seed=7)]
    maps = [_maps(per_lane, 3), _maps(per_lane, 4)]
    out = ops.remap([torch.from_numpy(s).to(gpu) for s in srcs], [(torch.from_numpy(mx).to(gpu), torch.from_numpy(my).to(gpu)) for mx, my in maps],
                    dtype=dtype, layout=layout, reverse_channels=reverse)
    torch.cuda.synchronize()
    assert len(out) == 2
    for o, s, (mx, my) in zip(out, srcs, maps):
        want = TW.remap_lanes_u8(s, mx, my, layout, reverse)
        assert o.shape == (RC.LANES, channels) + RC.OUT_HW
        assert _same_bits(o.cpu(), _as_dtype(want, dtype))


def test_remap_four_channels_and_mixed_groups(gpu):
    """C = 4 (the fourth channel stays in place under reverse_channels), both layouts; reverse given per group; a single tensor is one group."""
    from macvo_amd import ops

    mx, my = _maps(False, 3)
    dm = (torch.from_numpy(mx).to(gpu), torch.from_numpy(my).to(gpu))
    for layout in ("hwc", "planar"):
        srcs = [RC.images(4, layout, seed=2), RC.images(4, layout, seed=5)]
        out = ops.remap([torch.from_numpy(s).to(gpu) for s in srcs], [dm, dm], dtype=torch.uint8, layout=layout, reverse_channels=[True, False])
        for o, s, rev in zip(out, srcs, (True, False)):
            assert torch.equal(o.cpu(), torch.from_numpy(TW.remap_lanes_u8(s, mx, my, layout, rev)))
    one = ops.remap(torch.from_numpy(srcs[0]).to(gpu), dm, dtype=torch.uint8, layout="planar")
    assert len(one) == 1 and torch.equal(one[0].cpu(), torch.from_numpy(TW.remap_lanes_u8(srcs[0], mx, my, "planar", False)))


@pytest.mark.parametrize("hw", [(37, 53), (16, 64), (33, 130)])
def test_identity_map_returns_the_source(gpu, hw):
    from macvo_amd import ops

    H, W = hw
    src = RC.images(3, "hwc", src_hw=hw, lanes=2, seed=9)
    my, mx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    out = ops.remap(torch.from_numpy(src).to(gpu), (mx.to(gpu), my.to(gpu)), dtype=torch.uint8)[0]
    assert torch.equal(out.cpu(), torch.from_numpy(src).permute(0, 3, 1, 2))
    # a view whose data pointer is not 16-byte aligned takes the scalar map loads and the narrow stores: same bytes
    buf = torch.empty(2 * 3 * H * W + 1, dtype=torch.uint8, device=gpu)
    o2 = buf[1:].view(2, 3, H, W)
    mxo, myo = torch.empty(H * W + 1, device=gpu)[1:].view(H, W).copy_(mx), torch.empty(H * W + 1, device=gpu)[1:].view(H, W).copy_(my)
    ops.remap(torch.from_numpy(src).to(gpu), (mxo, myo), dtype=torch.uint8, out=[o2])
    assert torch.equal(o2.cpu(), torch.from_numpy(src).permute(0, 3, 1, 2))


def test_remap_indices_past_2_31(gpu):
    """64 lanes of 4 x 2048 x 4100 bytes: source and destination element indices pass 2^31 in the last lanes.  The first and the last lane against the twin."""
    from macvo_amd import ops

    lanes, Cn, H, W = 64, 4, 2048, 4100
    assert lanes * Cn * H * W > 2 ** 31
    g = torch.Generator(device=gpu).manual_seed(0)
    src = torch.randint(0, 256, (lanes, Cn, H, W), dtype=torch.uint8, device=gpu, generator=g)
    vy, vx = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=gpu), torch.arange(W, dtype=torch.float32, device=gpu), indexing="ij")
    mx = vx + (torch.rand(H, W, device=gpu, generator=g) * 6 - 3)
    my = vy + (torch.rand(H, W, device=gpu, generator=g) * 6 - 3)
    out = ops.remap(src, (mx, my), dtype=torch.uint8, layout="planar", reverse_channels=True)[0]
    torch.cuda.synchronize()
    for l in (0, lanes - 1):
        want = TW.remap_u8(src[l].cpu().numpy(), mx.cpu().numpy(), my.cpu().numpy(), "planar", True)
        assert torch.equal(out[l].cpu(), torch.from_numpy(want)), l


# ------------------------------------------------------------------------------------------------------------------------- the map builder
@pytest.mark.parametrize("hw", [(30, 47), (480, 752)])
def test_map_builder_within_one_ulp_of_fp64(gpu, hw):
    """Both cameras of the EuRoC rig in one launch: every device fp32 entry is within one fp32 ulp (np.spacing) of the fp64 twin rounded to fp32 — both sides
    carry errors far below an fp32 ulp, so the two roundings differ by at most one step.  Prints how many entries are not identical."""
    from macvo_amd import ops

    rig = RR.euroc_rig()
    if hw != (480, 752):
        rig = rig[:4] + ((hw[1], hw[0]),) + rig[5:]
    plan, ref = ops.stereo_rectify_plan(*rig), RR.plan(*rig)
    mx, my = ops.rectify_maps(plan, device=gpu)
    torch.cuda.synchronize()
    assert mx.shape == my.shape == (2,) + hw and mx.dtype == torch.float32
    differ = 0
    for cam in range(2):
        rx, ry = (m.astype(np.float32) for m in RR.maps(ref["cams"][cam], *hw))
        for dev_m, r in ((mx[cam].cpu().numpy(), rx), (my[cam].cpu().numpy(), ry)):
            assert np.all(np.abs(dev_m.astype(np.float64) - r.astype(np.float64)) <= np.spacing(np.abs(r)).astype(np.float64))
            differ += int((dev_m != r).sum())
    print(f"map builder {hw[0]} x {hw[1]}: {differ} of {4 * hw[0] * hw[1]} entries differ from the fp64 twin rounded to fp32 (each by one ulp)")
    # a list of camera records and an explicit grid: the right camera alone equals its slice of the pair
    rx2, ry2 = ops.rectify_maps([plan.c.cam[1]], hw[0], hw[1], device=gpu)
    assert torch.equal(rx2[0], mx[1]) and torch.equal(ry2[0], my[1])


# ------------------------------------------------------------------------------------------------------------------------- end to end
_E2E = {}


def _euroc_rectifier(gpu):
    """StereoRectifier on the EuRoC rig at 480 x 752, 2 lanes of random uint8 images, and the twin's uint8 result on the device's own maps — built once."""
    if not _E2E:
        from macvo_amd.rectify import StereoRectifier

        cal = json.load(open(os.path.join(ROOT, "tests", "golden", "euroc_calib.json")))
        c0, c1 = cal["cam0"], cal["cam1"]
        rect = StereoRectifier.from_body_frames(c0["T_BS"], c0["intrinsics"], c0["distortion"], c1["T_BS"], c1["intrinsics"], c1["distortion"],
                                                tuple(cal["resolution"]), device=gpu)
        rng = np.random.default_rng(11)
        imgs = [rng.integers(0, 256, (2, 480, 752, 3), dtype=np.uint8) for _ in range(2)]
        (lx, ly), (rx, ry) = rect.maps
        twin = [TW.remap_lanes_u8(imgs[0], lx.cpu().numpy(), ly.cpu().numpy()), TW.remap_lanes_u8(imgs[1], rx.cpu().numpy(), ry.cpu().numpy())]
        _E2E.update(rect=rect, imgs=imgs, twin=twin)
    return _E2E["rect"], _E2E["imgs"], _E2E["twin"]


def test_stereo_rectifier_end_to_end(gpu):
    from macvo_amd import ops

    rect, imgs, twin = _euroc_rectifier(gpu)
    assert rect.K.shape == (1, 3, 3) and rect.K.dtype == torch.float32 and np.array_equal(rect.K[0].numpy(), rect.P1.numpy()[:, :3].astype(np.float32))
    assert abs(rect.baseline - 0.1100778422) <= 5e-11 and (rect.width, rect.height) == (752, 480)
    # from_body_frames inverts T_BS_r with torch, tests/rectify_ref.py with numpy: the same plan up to the two inverses' rounding
    plan = ops.stereo_rectify_plan(*RR.euroc_rig())
    for a, b in ((rect.R1, plan.R1), (rect.R2, plan.R2), (rect.P1, plan.P1), (rect.P2, plan.P2)):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    L_, R_ = rect(torch.from_numpy(imgs[0]).to(gpu), torch.from_numpy(imgs[1]).to(gpu))
    torch.cuda.synchronize()
    assert L_.shape == R_.shape == (2, 3, 480, 752) and L_.dtype == torch.float32
    assert _same_bits(L_.cpu(), _as_dtype(twin[0], torch.float32)) and _same_bits(R_.cpu(), _as_dtype(twin[1], torch.float32))
    # VBR's order: BGR -> RGB is the same planes, reversed
    Lr, _ = rect(torch.from_numpy(imgs[0]).to(gpu), torch.from_numpy(imgs[1]).to(gpu), reverse_channels=True)
    assert torch.equal(Lr, L_.flip(1))


def test_rectify_then_preprocess_chain(gpu):
    """dtype = uint8 keeps planar uint8, which ops.preprocess takes through its MV_PP_U8 input: rectify, then a nearest SmartResizeFrame to 240 x 376
    (an exact scale of 2), against the twin's bytes through the CPU restatement of the transform — bit for bit, K included."""
    from macvo_amd import ops

    rect, imgs, twin = _euroc_rectifier(gpu)
    L8, R8 = rect(torch.from_numpy(imgs[0]).to(gpu), torch.from_numpy(imgs[1]).to(gpu), dtype=torch.uint8)
    assert L8.dtype == torch.uint8 and torch.equal(L8.cpu(), torch.from_numpy(twin[0])) and torch.equal(R8.cpu(), torch.from_numpy(twin[1]))
    pl = ops.preprocess_plan(rect.height, rect.width, "smart", K=rect.K, height=240, width=376, interp="nearest")
    got = ops.preprocess(pl, L8, R8)
    torch.cuda.synchronize()
    ref = PR.apply(PR.stereo(_as_dtype(twin[0], torch.float32), _as_dtype(twin[1], torch.float32), rect.K.repeat(2, 1, 1)),
                   [("smart", dict(height=240, width=376, interp="nearest"))])
    assert _same_bits(got.imageL.cpu(), ref.imageL) and _same_bits(got.imageR.cpu(), ref.imageR)
    assert torch.equal(pl.K, ref.K[:1])


# ------------------------------------------------------------------------------------------------------------------------- what the launch refuses
def test_remap_validation_launches_nothing(gpu):
    from macvo_amd import _lib as L

    lib = L.load()
    H, W, h, w = 8, 12, 6, 10
    src = torch.zeros(1, 4, H, W, dtype=torch.float32, device=gpu)          # (large enough for every row below)
    dst = torch.full((1, 4, h, w), 7.0, dtype=torch.float32, device=gpu)
    m = torch.zeros(h, w, device=gpu)

    def group(channels=3, src_dtype=L.MV_PP_U8, dst_dtype=L.MV_F32, layout=L.MV_RM_PLANAR):
        g = L.mvRemapGroup()
        g.src, g.dst, g.map_x, g.map_y = src.data_ptr(), dst.data_ptr(), m.data_ptr(), m.data_ptr()
        g.src_lane_stride, g.dst_lane_stride, g.map_lane_stride = channels * H * W, channels * h * w, 0
        g.channels, g.layout, g.reverse_channels, g.src_dtype, g.dst_dtype = channels, layout, 0, src_dtype, dst_dtype
        return g

    def call(groups, n=None, lanes=1):
        arr = (L.mvRemapGroup * len(groups))(*groups)
        return lib.mv_remap_lanes(arr, len(groups) if n is None else n, lanes, H, W, h, w, None)

    INVALID, UNSUPPORTED = -1, -2
    assert call([group(channels=2)]) == UNSUPPORTED
    assert call([group(src_dtype=L.MV_F32)]) == UNSUPPORTED and call([group(src_dtype=L.MV_F16)]) == UNSUPPORTED
    assert call([group()] * (L.MV_RM_MAX_GROUPS + 1)) == INVALID
    assert call([group()], n=0) == INVALID and call([group()], lanes=0) == INVALID and call([group()], lanes=L.MV_MAX_LANES + 1) == INVALID
    assert call([group(dst_dtype=5)]) == INVALID and call([group(layout=2)]) == INVALID
    short = group()
    short.dst_lane_stride -= 1
    assert call([short]) == INVALID
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())
    from macvo_amd import ops

    with pytest.raises(L.MacvoHipError, match=r"\(-2\)"):
        ops.remap(torch.zeros(1, H, W, 2, dtype=torch.uint8, device=gpu), (m, m))
    with pytest.raises(L.MacvoHipError, match=r"\(-2\)"):
        ops.remap(torch.zeros(1, H, W, 3, dtype=torch.float32, device=gpu), (m, m))
    u8 = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=gpu)
    with pytest.raises(L.MacvoHipError, match=r"\(-1\)"):
        ops.remap([u8] * 5, [(m, m)] * 5)
    assert lib.mv_rectify_maps((L.mvRectifyCam * 1)(), 0, h, w, m.data_ptr(), m.data_ptr(), None) == INVALID
    assert lib.mv_rectify_maps((L.mvRectifyCam * 5)(), 5, h, w, m.data_ptr(), m.data_ptr(), None) == INVALID
