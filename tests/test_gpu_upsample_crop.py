"""mv_convex_upsample_crop_m: convex 8x upsampling that stores only the un-padded window.  The arithmetic is the aligned kernel's, so the bar is bit
equality with the slice of `mv_convex_upsample_m` on the same inputs (whose parity with oracle.frontend.upsample_flow tests/test_gpu_corr.py::test_convex_upsample pins) — and
nothing outside the output may be written: the output is a view at an odd float offset into a NaN-filled buffer whose 64 floats on either side stay NaN."""
import pytest
import torch

from tests import unpad_ref

pytestmark = pytest.mark.gpu

B = 3
GUARD = 64
# coarse h x w, (H, W): the smallest shapes at which each case exists
SHAPES = [
    (5, 7, 40, 56),      # no pad: the window form accepts the whole result too
    (5, 7, 38, 52),      # even pads (2 and 4): one row / two columns off either side
    (5, 7, 37, 51),      # pads 3 and 5: asymmetric, odd rows, odd plane
    (5, 7, 33, 49),      # pad 7, the maximum: three rows / columns in front, four behind
    (9, 15, 70, 117),    # 135 coarse pixels: a second group of waves and tail lanes
]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def _run(gpu, h, w, H, W, dtype, exp2, seed):
    from macvo_amd import ops

    hp, pw, y0, x0 = unpad_ref.pad_of(H, W)
    assert (H + hp, W + pw) == (8 * h, 8 * w)
    flow8, mask = unpad_ref.upsample_case(B, h, w, seed)
    flow8, mask = flow8.to(gpu), mask.to(dtype).to(gpu)
    scale = 1.0 if exp2 else 0.25
    padded = ops.convex_upsample(flow8, mask, scale, exp2_out=exp2)
    n = B * 2 * H * W
    buf = torch.full((GUARD + 1 + n + GUARD,), float("nan"), device=gpu)
    out = buf[GUARD + 1: GUARD + 1 + n].view(B, 2, H, W)
    assert out.data_ptr() % 8 == 4                       # 4-byte aligned, not 8: nothing wider than a dword may be assumed
    got = ops.convex_upsample(flow8, mask, scale, exp2_out=exp2, crop=(y0, x0, H, W), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out, padded[..., y0: y0 + H, x0: x0 + W])
    assert torch.isnan(buf[: GUARD + 1]).all() and torch.isnan(buf[GUARD + 1 + n:]).all()
    # ... and without `out=`: a fresh dense tensor with the same bits
    assert torch.equal(ops.convex_upsample(flow8, mask, scale, exp2_out=exp2, crop=(y0, x0, H, W)), out)


@pytest.mark.parametrize("exp2", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("h,w,H,W", SHAPES)
def test_crop_equals_the_slice_of_the_padded_result_and_writes_nothing_else(gpu, h, w, H, W, dtype, exp2):
    _run(gpu, h, w, H, W, dtype, exp2, seed=h * 100 + W)


def test_crop_at_kitti_size(gpu):
    """47 x 98 maps -> 376 x 780: 2 columns off either side, no rows."""
    _run(gpu, 47, 98, 376, 780, torch.float32, True, seed=5)


def test_crop_windows_that_are_no_centred_pad(gpu):
    """The entry point takes any window of the result (the centred pad is the driver's rule, not the kernel's): one that starts deep inside, so that whole coarse
    rows and columns fall outside on either side."""
    from macvo_amd import ops

    h, w = 5, 7
    flow8, mask = unpad_ref.upsample_case(B, h, w, 11)
    flow8, mask = flow8.to(gpu), mask.to(gpu)
    padded = ops.convex_upsample(flow8, mask, 0.25)
    for (y0, x0, H, W) in ((9, 17, 13, 21), (0, 0, 1, 1), (39, 55, 1, 1), (17, 0, 9, 56)):
        n = B * 2 * H * W
        buf = torch.full((GUARD + 1 + n + GUARD,), float("nan"), device=gpu)
        out = buf[GUARD + 1: GUARD + 1 + n].view(B, 2, H, W)
        ops.convex_upsample(flow8, mask, 0.25, crop=(y0, x0, H, W), out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, padded[..., y0: y0 + H, x0: x0 + W]), (y0, x0, H, W)
        assert torch.isnan(buf[: GUARD + 1]).all() and torch.isnan(buf[GUARD + 1 + n:]).all()
