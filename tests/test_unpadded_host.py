"""Frames whose sides are no multiples of 8 (KITTI reaches the network as 376 x 780), host side: the pad rule against this project's statement of the
network's InputPadder, the frame driver's sizing call, the ABI and the new symbols.  No GPU."""
import ctypes as C

import pytest


def test_input_pad_is_the_networks_centred_pad():
    from macvo_amd import ops
    from tools.flowformer_host import InputPadder

    for H in range(1, 41):
        for W in range(1, 41):
            left, right, top, bottom = ops.input_pad(H, W)
            assert [left, right, top, bottom] == InputPadder((H, W))._pad, (H, W)
            assert ops.eighth_shape(H, W) == ((H + top + bottom) // 8, (W + left + right) // 8) == (-(-H // 8), -(-W // 8))
            win = ops.unpad_window(H, W)
            assert win == (None if (H % 8 == 0 and W % 8 == 0) else (top, left, H, W))
    assert ops.input_pad(376, 780) == (2, 2, 0, 0) and ops.eighth_shape(376, 780) == (47, 98)
    assert ops.input_pad(237, 315) == (2, 3, 1, 2) and ops.eighth_shape(237, 315) == (30, 40)


def _cfg_factory():
    from macvo_amd import _lib as L

    lib = L.load()
    lm = L.mvLMParams()
    lib.mv_lm_default_params(C.byref(lm))

    def cfg(**kw):
        d = dict(H=480, W=640, C=256, pairs=2, iters=12, radius=4, feat_dtype=L.MV_F32, layout=L.MV_LAYOUT_CHW, volume_split=L.MV_PACK_F16X2,
                 selector_mode=L.MV_KP_NODEPTH, kp_kernel_size=7, kp_mask_width=32, num_point=200, edgewidth=32,
                 min_num_point=10, graph_type=L.MV_GRAPH_DISP, filters=1, cov_kernel_size=31, fx=320.0, fy=320.0, cx=320.0,
                 cy=240.0, baseline=0.25, bl_fx=80.0, bl_fx_sq=6400.0, match_cov_default=0.25, max_match_cov=100.0,
                 max_depth_cov=250.0, max_depth=80.0, min_flow_cov_sq=0.0625, min_depth_cov=0.05, filter_min_depth=0.05,
                 map_max_depth=5.0, map_max_depth_cov=0.005, lm=lm)
        d.update(kw)
        return L.mvFramePipeConfig(**d)

    return L, lib, cfg


def test_arena_sizing_accepts_any_frame_size_and_keeps_the_aligned_ones():
    L, lib, cfg = _cfg_factory()
    size = lambda H, W, **kw: lib.mv_frame_pipe_arena_bytes(C.byref(cfg(H=H, W=W, **kw)))  # noqa: E731
    for H, W in ((376, 780), (237, 315), (480, 752), (236, 316)):
        assert size(H, W) > 0, (H, W)
    # a multiple of 8 has no pad: the arena of the build before this rule, byte for byte
    assert size(480, 640) == 868644352
    assert size(376, 784) == 804984320
    # the 1/8 maps of a padded frame are those of the padded size, the full-resolution planes shrink: KITTI's 376 x 780 needs a little less than 376 x 784
    assert 0 < size(376, 780) < size(376, 784)
    # what a stage needs of the frame is still checked: the PoseNet crop of the TartanVO motion model covers 112 x 160
    assert size(237, 315, motion_model=L.MV_MOTION_TARTAN) > 0
    assert size(111, 315, motion_model=L.MV_MOTION_TARTAN) == 0 and size(237, 159, motion_model=L.MV_MOTION_TARTAN) == 0
    assert size(0, 315) == 0 and size(237, -3) == 0
    # a side one above a multiple of 8 (pad 7) stays refused, as tests/test_abi_and_host.py has always pinned it for H = 481; pad 6 is taken
    assert size(481, 640) == 0 and size(480, 641) == 0 and size(233, 315) == 0
    assert size(482, 642) > 0
    assert size(61, 315, selector_mode=L.MV_KP_RANDOM) == 0 and size(66, 315, selector_mode=L.MV_KP_RANDOM) > 0     # (H > 2 * kp_mask_width)


def test_abi_and_new_symbols():
    from macvo_amd import _lib as L

    lib = L.load()
    assert lib.mv_abi_version() == L.ABI_VERSION == 8
    for sym in ("mv_input_pad", "mv_convex_upsample_crop", "mv_convex_upsample_crop_m", "mv_convex_upsample", "mv_convex_upsample_m"):
        assert getattr(lib, sym) is not None
    pad = (C.c_int32 * 4)()
    lib.mv_input_pad(376, 780, pad)
    assert list(pad) == [2, 2, 0, 0]


def test_crop_entry_point_refuses_windows_outside_the_result():
    """Argument checks run before any launch: no GPU is touched by a refused call."""
    from macvo_amd import _lib as L

    lib = L.load()
    invalid = -1                                  # MV_ERR_INVALID_ARG (include/macvo_hip.h)
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    call = lambda y0, x0, H, W, out=p: lib.mv_convex_upsample_crop(p, p, out, 1, 5, 7, y0, x0, H, W, 1.0, 0, None)  # noqa: E731
    for bad in ((-1, 0, 40, 56), (0, -1, 40, 56), (1, 0, 40, 56), (0, 1, 40, 56), (0, 0, 41, 56), (0, 0, 40, 57), (0, 0, 0, 56), (3, 2, 38, 52)):
        assert call(*bad) == invalid, bad
    assert call(1, 2, 37, 51, out=C.c_void_p(p.value + 2)) == invalid          # 4-byte alignment is all the output needs — and it needs that


def test_camera_shapes_are_checked_on_the_host():
    import torch

    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, FrameInputs, check_frame_shapes

    cam = Camera(fx=320.0, fy=320.0, cx=157.5, cy=118.5, baseline=0.25, H=237, W=315)
    ok = FrameInputs(fmap1=torch.zeros(2, 16, 30, 40), fmap2=torch.zeros(2, 16, 30, 40), coords=torch.zeros(1, 2, 2, 30, 40),
                     flow=torch.zeros(2, 2, 237, 315), logcov=torch.zeros(2, 2, 237, 315))
    check_frame_shapes(ok, cam)
    with pytest.raises(ops.L.MacvoHipError):
        check_frame_shapes(FrameInputs(fmap1=ok.fmap1, fmap2=ok.fmap2, coords=torch.zeros(1, 2, 2, 29, 39), flow=ok.flow, logcov=ok.logcov), cam)
    with pytest.raises(ops.L.MacvoHipError):
        check_frame_shapes(FrameInputs(fmap1=ok.fmap1, fmap2=ok.fmap2, coords=ok.coords, flow=torch.zeros(2, 2, 240, 320), logcov=ok.logcov), cam)
