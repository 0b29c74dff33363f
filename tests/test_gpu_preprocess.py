"""GPU: frame preprocessing (mv_preprocess_lanes) against the CPU restatement of DataLoader/Transform.py (tests/preprocess_ref.py).

Nearest plans and plans without a resize are gathers: bit-exact.  Bilinear plans are measured against the fp64 formula, with torch-CPU-fp32's own error
against the same formula on the same input as the yardstick (at most twice it: a different but equally valid summation order)."""
from types import SimpleNamespace

import pytest
import torch

from tests import preprocess_ref as R

pytestmark = pytest.mark.gpu
PLANES = ("imageL", "imageR", "gt_flow", "flow_mask", "gt_depth")


def _K(B=1):
    return torch.tensor([[[320.5, 0.0, 321.75], [0.0, 318.25, 240.125], [0.0, 0.0, 1.0]]], dtype=torch.float32).repeat(B, 1, 1)


def _frame(H, W, seed=0, B=1):
    g = torch.Generator().manual_seed(seed)
    return R.stereo(torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g), _K(B),
                    gt_flow=torch.randn(B, 2, H, W, generator=g) * 5, flow_mask=torch.rand(B, 1, H, W, generator=g) > 0.4,
                    gt_depth=torch.rand(B, 1, H, W, generator=g) * 30 + 0.5)


def _one_plan(steps, d):
    from macvo_amd.transforms import plan_steps

    plans = plan_steps(steps, d.height, d.width, d.K)
    assert len(plans) == 1
    return plans[0]


def _run(plan, d, dev, **kw):
    from macvo_amd import ops

    res = ops.preprocess(plan, *[None if getattr(d, n) is None else getattr(d, n).to(dev) for n in PLANES], **kw)
    torch.cuda.synchronize()
    return res


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _scales(h, w, th, tw):
    """ScaleFrame arguments whose int() truncation lands on (th, tw) whatever the last bit of the quotient does."""
    return dict(scale_u=w / (tw + 0.5), scale_v=h / (th + 0.5))


NEAREST_CASES = {
    "smart_pad_row_half_even": ((27, 40), [("smart", dict(height=13, width=16, interp="nearest"))]),          # resized 12 x 19: pad row, left = round(1.5) = 2
    "smart_scale_on_both_axes": ((53, 175), [("smart", dict(height=47, width=98, interp="nearest"))]),
    "smart_pure_crop_odd": ((47, 155), [("smart", dict(height=47, width=98, interp="nearest"))]),             # scale 1: a crop, 57 / 2 = 28.5 -> 28
    "smart_upscale": ((30, 47), [("smart", dict(height=40, width=40, interp="nearest"))]),
    "scale_u_differs_from_v": ((53, 175), [("scale", dict(scale_u=2.5, scale_v=1.5, interp="nearest"))]),
    "crop_larger_than_frame": ((30, 47), [("crop", dict(height=20, width=70))]),                               # zero-pad path on x, a cut on y
    "crop_of_a_bilinear_unit_scale": ((21, 70), [("scale", dict(scale_u=1.0, scale_v=1.0, interp="bilinear")), ("crop", dict(height=33, width=41))]),
    "two_tile_rows_and_columns": ((90, 300), [("smart", dict(height=37, width=131, interp="nearest"))]),
}


@pytest.mark.parametrize("case", sorted(NEAREST_CASES))
def test_nearest_and_crop_are_bit_exact(gpu, case):
    (H, W), steps = NEAREST_CASES[case]
    d = _frame(H, W, seed=3, B=2)
    ref = R.apply(d, steps)
    plan = _one_plan(steps, d)
    out = _run(plan, d, gpu)
    assert (plan.height, plan.width) == (ref.height, ref.width)
    for n in PLANES:
        assert _same_bits(getattr(out, n).cpu(), getattr(ref, n)), (case, n)
    assert _same_bits(plan.K, ref.K)
    if case == "smart_pad_row_half_even":
        assert plan.resized == (12, 19) and plan.pads == (0, 1, 0, 0) and plan.origin == (0, 2) and (out.imageL[..., -1, :] == 0).all()


BILINEAR_CASES = {"down_2p8": ((37, 53), (13, 20)), "down_1p4": ((48, 64), (31, 47)), "up": ((20, 30), (33, 41)), "down_7p9": ((135, 240), None)}


@pytest.mark.parametrize("case", sorted(BILINEAR_CASES))
def test_bilinear_error_against_fp64_within_twice_torch_fp32(gpu, case):
    """max |kernel - fp64 formula| <= 2 max |torch CPU fp32 - fp64 formula| per plane group, same input.

    Measured on an MI355X (kernel / torch per plane group): DESIGN.md section 7, "Frame preprocessing"."""
    (H, W), size = BILINEAR_CASES[case]
    steps = [("scale", dict(interp="bilinear", **(_scales(H, W, *size) if size else dict(scale_u=7.9, scale_v=7.9))))]
    d = _frame(H, W, seed=5, B=1)
    ref = R.apply(d, steps)
    plan = _one_plan(steps, d)
    size = (plan.height, plan.width)
    assert size == (ref.height, ref.width) and (BILINEAR_CASES[case][1] in (None, size))
    out = _run(plan, d, gpu)
    for name, got, src in (("images", torch.cat([out.imageL, out.imageR], 1), torch.cat([d.imageL, d.imageR], 1)), ("gt_depth", out.gt_depth, d.gt_depth)):
        f64 = R.aa_resize_f64(src, size)
        e_kernel = (got.cpu().double() - f64).abs().max().item()
        e_torch = (R.resize(src, size, "bilinear").double() - f64).abs().max().item()
        print(f"{case} {name}: kernel {e_kernel:.3e} torch-fp32 {e_torch:.3e}")
        assert e_kernel <= 2 * e_torch, (case, name, e_kernel, e_torch)
    # gt_flow: the resampled value divided by round_scale in fp32 (a true division): within the same bound of the restatement's fp64 value
    ru, rv = plan.round_scale
    f64 = R.aa_resize_f64(d.gt_flow, size) / torch.tensor([ru, rv], dtype=torch.float64).view(1, 2, 1, 1)
    e_kernel, e_torch = (out.gt_flow.cpu().double() - f64).abs().max().item(), (ref.gt_flow.double() - f64).abs().max().item()
    print(f"{case} gt_flow: kernel {e_kernel:.3e} torch-fp32 {e_torch:.3e}")
    assert e_kernel <= 2 * e_torch
    # the mask is `resampled != 0`; K to the bit
    assert _same_bits(out.flow_mask.cpu(), ref.flow_mask) and _same_bits(plan.K, ref.K)


def test_bilinear_nan_and_inf_spread_as_in_torch(gpu):
    H, W = 37, 53
    d = _frame(H, W, seed=7)
    d.gt_depth[0, 0, 5, 7] = float("nan")
    d.gt_depth[0, 0, 20, 30] = float("inf")
    d.gt_depth[0, 0, 36, 52] = float("-inf")
    d.gt_depth[0, 0, 0, 26] = float("inf")
    steps = [("scale", dict(interp="bilinear", **_scales(H, W, 13, 20)))]
    ref = R.apply(d, steps)
    out = _run(_one_plan(steps, d), d, gpu)
    got = out.gt_depth.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref.gt_depth)) and torch.isnan(got).sum() >= 3
    assert torch.equal(torch.isinf(got), torch.isinf(ref.gt_depth))
    fin = torch.isfinite(ref.gt_depth)
    assert (got[fin] - ref.gt_depth[fin]).abs().max() < 1e-4


def test_bilinear_downscale_above_8_is_refused_before_the_launch(gpu):
    from macvo_amd import ops

    d = _frame(135, 240, seed=9)
    steps = [("scale", dict(scale_u=8.5, scale_v=8.5, interp="bilinear"))]
    plan = _one_plan(steps, d)
    with pytest.raises(ops.L.MacvoHipError, match="unsupported"):
        _run(plan, d, gpu)
    torch.cuda.synchronize()
    steps[0][1]["interp"] = "nearest"                              # nearest has no limit
    out = _run(_one_plan(steps, d), d, gpu)
    assert _same_bits(out.gt_depth.cpu(), R.apply(d, steps).gt_depth)


@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
def test_uint8_sources_and_16_bit_outputs(gpu, interp):
    from macvo_amd import ops

    H, W = 53, 175
    g = torch.Generator().manual_seed(11)
    u8L, u8R = (torch.randint(0, 256, (2, 3, H, W), generator=g, dtype=torch.uint8) for _ in range(2))
    steps = [("smart", dict(height=47, width=98, interp=interp))]
    plan = _one_plan(steps, R.stereo(u8L, u8R, _K(2)))
    a = ops.preprocess(plan, u8L.to(gpu), u8R.to(gpu))                                            # uint8 in, absent optional planes
    b = ops.preprocess(plan, (u8L.float() / 255).to(gpu), (u8R.float() / 255).to(gpu))
    assert a.gt_flow is None and a.flow_mask is None and a.gt_depth is None and a.imageL.dtype == torch.float32
    assert _same_bits(a.imageL, b.imageL) and _same_bits(a.imageR, b.imageR)
    d = _frame(H, W, seed=12, B=2)
    f32 = _run(plan, d, gpu)
    for dt in (torch.float16, torch.bfloat16):
        o = _run(plan, d, gpu, out_dtype=dt)
        for n in PLANES:
            assert _same_bits(getattr(o, n), getattr(f32, n).to(dt)), (dt, n)
        # fp16 / bf16 planes in: resampled in fp32, rounded once — the restatement's bits for a gather, its fp32 path's rounding for the filter
        dh = SimpleNamespace(**{**vars(d), **{n: getattr(d, n).to(dt) for n in ("imageL", "imageR", "gt_flow", "gt_depth")}})
        oh, rh = _run(plan, dh, gpu), R.apply(dh, steps)
        for n in PLANES:
            got, want = getattr(oh, n).cpu(), getattr(rh, n)
            assert got.dtype == want.dtype
            if interp == "nearest":
                assert _same_bits(got, want), (dt, n)
            elif n == "flow_mask":
                # the bool mask does not depend on the other planes' type.  (Not against torch here: 175 -> 155 has exact ties — output column 78's
                # support ends exactly on a pixel centre — where torch's fp32 window gains a tap of weight 3e-6 that the formula excludes, so a lone
                # True pixel under it reads as coverage in torch-fp32 and as none in fp64; the tie-free shapes of the bilinear cases pin the mask.)
                assert _same_bits(got, f32.flow_mask.cpu()), dt
            else:
                assert (got.float() - want.float()).abs().max() <= 2.0 ** (-7 if dt == torch.bfloat16 else -10) * want.float().abs().max(), (dt, n)


def test_cast_in_front_of_the_resize_folds(gpu):
    """[CenterCropFrame, CastDataType, ScaleFrame] in one launch: the planes are rounded to fp16 BEFORE they are resampled, the mask becomes numbers."""
    d = _frame(60, 90, seed=13)
    steps = [("crop", dict(height=48, width=64)), ("cast", dict(dtype="fp16")), ("scale", dict(scale_u=2.0, scale_v=1.5, interp="nearest"))]
    ref = R.apply(d, steps)
    out = _run(_one_plan(steps, d), d, gpu)
    for n in PLANES:
        assert _same_bits(getattr(out, n).cpu(), getattr(ref, n)), n


@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
def test_three_lanes_equal_three_launches(gpu, interp):
    d = _frame(53, 175, seed=15, B=3)
    steps = [("smart", dict(height=47, width=98, interp=interp))]
    plan = _one_plan(steps, R.stereo(d.imageL[:1], d.imageR[:1], _K()))
    out = _run(plan, d, gpu)
    for l in range(3):
        one = SimpleNamespace(**{n: getattr(d, n)[l:l + 1] for n in PLANES})
        o = _run(plan, one, gpu)
        for n in PLANES:
            assert _same_bits(getattr(out, n)[l:l + 1], getattr(o, n)), (l, n)


@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
def test_odd_width_output_at_a_4_byte_aligned_address(gpu, interp):
    """Output rows of 131 floats starting one element into an allocation: 4-byte aligned, not 16: the vector stores give way to scalar ones where they must."""
    d = _frame(90, 300, seed=17, B=2)
    steps = [("smart", dict(height=37, width=131, interp=interp))]
    plan = _one_plan(steps, d)
    want = _run(plan, d, gpu)
    outs, bufs = {}, {}
    for n in PLANES:
        w = getattr(want, n)
        bufs[n] = torch.full((w.numel() + 2,), 1 if w.dtype == torch.bool else 7, dtype=w.dtype, device=gpu)
        outs[n] = bufs[n][1:1 + w.numel()].view(w.shape)
        assert outs[n].data_ptr() % 16 != 0 or w.element_size() < 4
    got = _run(plan, d, gpu, out=outs)
    for n in PLANES:
        assert got.__dict__[n].data_ptr() == outs[n].data_ptr() and _same_bits(outs[n], getattr(want, n)), n
        guard = 1 if bufs[n].dtype == torch.bool else 7
        assert bufs[n][0].item() == guard and bufs[n][-1].item() == guard                          # nothing outside the planes was written


def test_plugins_on_a_duck_typed_frame(gpu):
    from macvo_amd import ops, transforms as X
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath, preprocess_config_fields

    d = _frame(53, 175, seed=19)
    ref = R.smart_resize(R.apply(d, []), 47, 98, "nearest")
    frame = SimpleNamespace(stereo=R.apply(d, []))
    t = X.IDataTransform.instantiate("HIP_SmartResizeFrame", SimpleNamespace(height=47, width=98, interp="nearest"))
    assert t(frame) is frame
    torch.cuda.synchronize()
    st = frame.stereo
    assert (st.height, st.width) == (47, 98) and _same_bits(st.K, ref.K)
    for n in PLANES:
        assert getattr(st, n).is_cuda and _same_bits(getattr(st, n).cpu(), getattr(ref, n)), n
    # HIP_CastDataType alone, and the KITTI block of Config/Experiment/Common/Preprocess.yaml through the config mapper
    frame = X.HIP_CastDataType(SimpleNamespace(dtype="bf16"))(SimpleNamespace(stereo=R.apply(d, [])))
    torch.cuda.synchronize()
    for n in PLANES:
        assert _same_bits(getattr(frame.stereo, n).cpu(), getattr(R.cast(R.apply(d, []), "bf16"), n)), n
    block = dict(KITTI=[dict(type="SmartResizeFrame", args=dict(height=376, width=780, interp="nearest"))])
    out = preprocess_config_fields(block, "KITTI", Camera(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, baseline=0.537, H=376, W=1241))
    cam = out["camera"]
    assert (cam.H, cam.W) == (376, 780) and ops.eighth_shape(cam.H, cam.W) == (47, 98)
    hot = NativeHotPath(cam, HotPathConfig(), gpu)
    assert hot.cam is cam
    g = torch.Generator().manual_seed(21)
    u8 = torch.randint(0, 256, (1, 3, 376, 1241), generator=g, dtype=torch.uint8)
    res = ops.preprocess(out["plans"][0], u8.to(gpu), u8.flip(-1).to(gpu))
    assert _same_bits(res.imageL.cpu(), u8[..., 230:1010].float() / 255) and _same_bits(res.imageR.cpu(), u8.flip(-1)[..., 230:1010].float() / 255)
