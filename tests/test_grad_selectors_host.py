"""CPU: the image-gradient selectors (GradientSelector, SparseGradienSelector, SelectorCompose — Module/KeypointSelector.py:121-213, :51-75) off the GPU.

* tests/grad_selectors_ref.py (the torch restatement) reproduces the reference classes' golden rows.
* The host twin of the kernels (tests/c_abi/kp_grad_twin.cpp on mac-vo_amd/csrc/kp_grad_math.h) lists the restatement's candidates bit for bit on
  1/256-valued images, on which both are exact — behind a guard on the inputs: the fp64 threshold lies more than 1e-5 (about 20 ulp of it; torch's own
  fp32 threshold is within 1 ulp of the fp64 one) from every multiple of 1/256, the values such an image's gradient takes.
* Plugin configuration rules, the fp32 split of SelectorCompose, the host-side argument checks of the two entry points, pipeline.image_selector."""
import ctypes as C
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import grad_selectors_ref as GR
from tests import grad_sizes as GS
from tests import kp_grad_twin as TW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((96, 128), (61, 83), (33, 200))
SEEDS = (3, 5)
GUARD = 1e-5


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "grad_selectors.npz"))


def test_restatement_reproduces_the_reference_classes(golden):
    for ci, (H, W, iseed, m, gs, nms, n, seed) in enumerate(GR.GOLDEN_CASES):
        u8 = golden[f"image_{H}x{W}_{iseed}"]
        assert np.array_equal(u8, GR.quantised_u8(H, W, iseed)), "the stored image is the generator's"
        img = torch.from_numpy(u8.astype(np.float32)) / 256.0
        torch.manual_seed(seed)
        rows = GR.select(img, n, m, gs, nms)
        want = torch.from_numpy(golden[f"rows_{ci}"])
        assert rows.dtype == torch.int64 and torch.equal(rows, want), ci
    assert golden["rows_5"].shape == (0, 2) and 0 < golden["rows_3"].shape[0] < 500      # mask_width 0 selects nothing; n < numPoint returns all n
    c = GR.GOLDEN_COMPOSE
    img = GR.quantised_image(c["H"], c["W"], c["image_seed"])
    torch.manual_seed(c["seed"])
    rows = GR.compose([lambda k: GR.select(img, k, c["mask_width"], c["grad_std"]),
                       lambda k: GR.select(img, k, c["mask_width"], c["grad_std"], c["nms_size"])], c["weight"], c["num_point"])
    assert torch.equal(rows, torch.from_numpy(golden["compose_rows"]))


@pytest.mark.parametrize("H,W", SHAPES)
def test_twin_lists_the_restatements_candidates(H, W):
    for seed in SEEDS:
        img = GR.quantised_image(H, W, seed)
        for gs in (1.0, 2.0, 3.0):
            dist = GR.guard_distance(img, gs)
            assert dist > GUARD, (H, W, seed, gs, dist)                   # the guard on the INPUT: a threshold this far from every attainable value
            thr64 = GR.threshold_f64(img, gs)[1]
            for nms in (None, 1, 3, 7, 15):
                want = GR.candidates(img, 8, gs, nms).numpy().astype(np.int32)
                tw = TW.select(img, 8, gs, nms)
                assert np.array_equal(tw.cand, want), (H, W, seed, gs, nms)
                assert tw.n_above == GR.candidates(img, 8, gs).numel()
                assert abs(float(tw.stats[2]) - thr64) <= 4.8e-7            # the contract's figure: 1 ulp of a threshold in [4, 8)
            assert np.array_equal(tw.grad.view(np.int32), GR.image_grad(img)[0].numpy().view(np.int32))
            assert TW.select(img, 8, gs, 1).cand.tobytes() == TW.select(img, 8, gs).cand.tobytes()      # a 1 x 1 window is the plain selector
    img = GR.quantised_image(H, W, SEEDS[0])
    for m in (0, (min(H, W) + 1) // 2, max(H, W)):                        # the empty slice 0:-0 and 2m >= H or W: zero rows on both sides
        assert GR.candidates(img, m, 1.0, 3).numel() == 0 and TW.select(img, m, 1.0, 3).cand.size == 0
    zero = torch.zeros(3, H, W)
    tw = TW.select(zero, 4, 1.0)
    assert tw.cand.size == 0 and tuple(tw.stats) == (0.0, 0.0, 0.0) and GR.candidates(zero, 4, 1.0).numel() == 0      # thr = 0, strict >
    nan = img.clone()
    nan[1, H // 2, W // 2] = float("nan")
    assert TW.select(nan, 4, 1.0, 3).cand.size == 0 and GR.candidates(nan, 4, 1.0, 3).numel() == 0 and np.isnan(TW.select(nan, 4, 1.0).stats[2])
    blk = GR.block_constant_image(H, W, 9)
    assert GR.guard_distance(blk, 1.0) > GUARD
    tw, want = TW.select(blk, 4, 1.0, 7), GR.candidates(blk, 4, 1.0, 7)
    assert np.array_equal(tw.cand, want.numpy().astype(np.int32)) and want.numel() > 0
    g = GR.image_grad(blk)[0].flatten()[want]
    assert g.unique().numel() < want.numel(), "the block-constant image has tied maxima, and all of them are kept"


@pytest.mark.parametrize("seed", [3, 5, 7])
@pytest.mark.parametrize("H,W", list(GS.TABLE))
def test_twin_lists_the_restatements_candidates_at_the_path_sizes(H, W, seed):
    """The sizes of tests/grad_sizes.py (past one compaction pass, past one tile-sum chunk, below one tile): the twin is pinned to the restatement there
    before tests/test_gpu_grad_selectors_sizes.py compares the kernels with it."""
    GS.check_path(H, W)
    img = GR.quantised_image(H, W, seed)
    want_grad = GR.image_grad(img)[0].numpy().view(np.int32)
    for m in ((8, 1) if (H, W) in GS.TINY else (GS.mask_width_for(H, W),)):
        for gs in (1.0, 2.0, 3.0):
            if H * W > 1:           # (1 x 1: n - 1 = 0, the threshold is NaN on both sides and there is nothing to guard)
                dist = GR.guard_distance(img, gs)
                assert dist > GUARD, (H, W, seed, gs, dist)
                thr64 = GR.threshold_f64(img, gs)[1]
            n_above = GR.candidates(img, m, gs).numel()
            for nms in (None, 3, 15):
                want = GR.candidates(img, m, gs, nms).numpy().astype(np.int32)
                tw = TW.select(img, m, gs, nms)
                assert np.array_equal(tw.cand, want), (H, W, seed, m, gs, nms)
                assert tw.n_above == n_above
                assert np.array_equal(tw.grad.view(np.int32), want_grad)
                if H * W > 1:
                    assert abs(float(tw.stats[2]) - thr64) <= 4.8e-7
                else:
                    assert np.isfinite(tw.stats[0]) and np.isnan(tw.stats[1:]).all() and torch.isnan(GR.threshold(GR.image_grad(img), gs)).all()
                if (H, W) in GS.TINY and (m == 8 or H < 3):
                    assert want.size == 0 and tw.n_above == 0
            if (H, W) in GS.LARGE:
                assert n_above > 0


def test_twin_standalone_under_sanitizers():
    """The twin's own main as a stand-alone program with -fsanitize=address,undefined: host code only, nothing loaded into Python."""
    assert TW.run_standalone_sanitized().startswith("kp_grad_twin OK")


def test_plugin_config_rules_are_the_references():
    import macvo_amd.plugins as P
    from macvo_amd import interfaces as I

    G, S = P.HIP_GradientSelector, P.HIP_SparseGradienSelector
    assert I.IKeypointSelector.get_class("HIP_GradientSelector") is G and I.IKeypointSelector.get_class("HIP_SparseGradienSelector") is S
    assert I.IKeypointSelector.get_class("HIP_SelectorCompose") is P.HIP_SelectorCompose
    G.is_valid_config(NS(mask_width=0, grad_std=1))
    G.is_valid_config(NS(mask_width=32, grad_std=2.5, seed=7))
    for k in (1, 3, 15):
        S.is_valid_config(NS(mask_width=32, grad_std=1.5, nms_size=k))
    S.is_valid_config(NS(mask_width=32, grad_std=1.5, nms_size=7, seed=0))
    for bad in (NS(mask_width=-1, grad_std=1.0), NS(mask_width=1.0, grad_std=1.0), NS(mask_width=4, grad_std=0), NS(mask_width=4, grad_std=-1.0),
                NS(mask_width=4, grad_std="1"), NS(mask_width=4, grad_std=1.0, seed=-1), NS(mask_width=4, grad_std=1.0, seed=True)):
        with pytest.raises(ValueError):
            G.is_valid_config(bad)
    for k in (0, 2, 8, -3, 17, 3.0):       # even, negative, not an int: the reference's rule; 17: beyond the NMS tile's halo
        with pytest.raises(ValueError):
            S.is_valid_config(NS(mask_width=4, grad_std=1.0, nms_size=k))
    for cls, cfg in ((G, NS(mask_width=4)), (G, NS(mask_width=4, grad_std=1.0, nms_size=3)), (G, NS(mask_width=4, grad_std=1.0, device="cuda")),
                     (S, NS(mask_width=4, grad_std=1.0))):
        with pytest.raises(KeyError):          # the exact-key-set rule
            cls.is_valid_config(cfg)
    block = NS(type="HIP_SparseGradienSelector", args=NS(mask_width=32, grad_std=1.5, nms_size=7))
    I.IKeypointSelector.is_valid_config(block)
    assert isinstance(I.IKeypointSelector.instantiate(block.type, block.args), S)
    comp = NS(selector_args=[NS(type="HIP_GridSelector", args=NS(mask_width=32, device="cuda")), block], weight=[1, 2.5])
    P.HIP_SelectorCompose.is_valid_config(comp)
    for bad in (NS(selector_args=[block], weight=(1,)), NS(selector_args=[block], weight=["1"])):
        with pytest.raises(AssertionError):
            P.HIP_SelectorCompose.is_valid_config(bad)
    with pytest.raises(ValueError):
        P.HIP_SelectorCompose.is_valid_config(NS(selector_args=[NS(type="HIP_SparseGradienSelector", args=NS(mask_width=32, grad_std=1.5, nms_size=4))], weight=[1]))


@pytest.mark.parametrize("weight,num_point,want", [([1, 1, 1], 200, [66, 66, 66]), ([0.5, 0.25, 0.25], 200, [100, 50, 50]), ([1, 2], 100, [33, 66]),
                                                   ([0.1, 0.9], 10, [1, 9]), ([3], 7, [7])])
def test_selector_compose_splits_in_fp32(weight, num_point, want):
    import macvo_amd.plugins as P

    sub = NS(type="HIP_GradientSelector", args=NS(mask_width=4, grad_std=1.0))
    sel = P.HIP_SelectorCompose(NS(selector_args=[sub] * len(weight), weight=weight))
    assert sel.split(num_point) == want == GR.compose_split(weight, num_point)
    w = torch.tensor(weight)
    assert sel.weight.dtype == torch.float32 and torch.equal(sel.weight, w / w.sum())      # (integer weights divide into fp32 as well)
    assert all(isinstance(s, P.HIP_GradientSelector) for s in sel.selectors)


def test_entry_points_refuse_bad_arguments_on_the_host():
    """Every row is refused before anything is launched (no GPU needed, dummy pointers are never dereferenced)."""
    from macvo_amd import _lib as L

    lib = L.load()
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    P = 0x1000
    assert lib.mv_kp_gradient_workspace_bytes(0, 64) == 0 and lib.mv_kp_gradient_workspace_bytes(64, -1) == 0
    need = lib.mv_kp_gradient_workspace_bytes(48, 100)
    assert need >= 48 * 100 * 4 + 2 * 48 * 2 * 8 + 3 * 2 * 16

    def grad(image=P, params="ok", ws=P, ws_bytes=None, cand=P, count=P, stats=P, lanes=2, **kw):
        d = dict(H=48, W=100, mask_width=4, nms_size=3, grad_std=1.0)
        d.update(kw)
        p = L.mvKpGradParams(**d)
        return lib.mv_kp_gradient_lanes(image, C.byref(p) if params == "ok" else None, ws, need * lanes if ws_bytes is None else ws_bytes, cand, count, stats,
                                        lanes, None)

    for kw in (dict(image=None), dict(params=None), dict(ws=None), dict(cand=None), dict(count=None), dict(stats=None), dict(lanes=0),
               dict(lanes=L.MV_MAX_LANES + 1), dict(H=0), dict(W=-3), dict(mask_width=-1), dict(grad_std=0.0), dict(grad_std=-1.0),
               dict(grad_std=float("nan")), dict(nms_size=2), dict(nms_size=8), dict(nms_size=-1), dict(ws=P + 4)):
        assert grad(**kw) == INVALID, kw
    assert grad(nms_size=17) == UNSUPPORTED and grad(nms_size=16) == INVALID
    # sizes past the launch's limits: more tile rows than grid y takes, and v * W + u past an int32
    assert grad(H=16 * 65535 + 1, W=1) == INVALID and grad(H=65536, W=32768) == INVALID and grad(H=32768, W=65536, lanes=1) == INVALID
    assert grad(H=16 * 65535, W=1) == WORKSPACE and grad(H=65536, W=32767) == WORKSPACE      # the last sizes inside: refused for the workspace alone
    assert grad(ws_bytes=need * 2 - 1) == WORKSPACE and grad(ws_bytes=need, lanes=2) == WORKSPACE

    def fin(state=P, cand=P, stride=4800, count=P, count_stride=4, lanes=2, k=100, cap=100, W=100, out=P, nsel=P):
        return lib.mv_kp_finish_device_lanes(state, cand, stride, count, count_stride, lanes, k, cap, W, out, nsel, None)

    for kw in (dict(state=None), dict(cand=None), dict(count=None), dict(out=None), dict(nsel=None), dict(stride=0), dict(count_stride=0), dict(lanes=0),
               dict(lanes=L.MV_MAX_LANES + 1), dict(k=-1), dict(k=101), dict(cap=0, k=0), dict(W=0)):
        assert fin(**kw) == INVALID, kw
    head = lib.mv_randperm_max_head()
    assert fin(k=head + 1, cap=head + 1) == UNSUPPORTED


def test_ops_refuse_bad_arguments_before_the_library():
    from macvo_amd import ops

    img = torch.zeros(3, 16, 16)
    for kw in (dict(nms_size=2), dict(nms_size=17), dict(nms_size=0), dict(nms_size=3.0), dict(grad_std=0.0), dict(mask_width=-1), dict(mask_width=1.5)):
        a = dict(mask_width=4, grad_std=1.0)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.kp_gradient(img, **a)
    with pytest.raises(ValueError):
        ops.kp_gradient(torch.zeros(16, 16), 4, 1.0)
    with pytest.raises(ValueError):
        ops.kp_gradient(torch.zeros(2, 1, 16, 16), 4, 1.0)
    with pytest.raises(ops.L.MacvoHipError):           # no CPU fallback
        ops.kp_gradient(img, 4, 1.0)


def test_image_selector_maps_the_reference_blocks_and_refuses_the_rest():
    from macvo_amd.pipeline import image_selector, selector_config_fields

    args = dict(mask_width=32, grad_std=1.5)
    for t, a in (("GradientSelector", args), ("HIP_GradientSelector", args), ("SparseGradienSelector", dict(args, nms_size=7)),
                 ("HIP_SparseGradienSelector", dict(args, nms_size=7))):
        for block in ({"type": t, "args": a}, NS(type=t, args=NS(**a))):
            assert callable(image_selector(block, "cuda"))
            with pytest.raises(ValueError, match="no HIP form"):          # the pipe itself still has no such selector mode
                selector_config_fields(block)
            with pytest.raises(ValueError, match="image_selector"):       # ... and says where the rows come from
                selector_config_fields(block)
    with pytest.raises(ValueError, match="not an image selector"):
        image_selector({"type": "RandomSelector", "args": {"mask_width": 32, "device": "cuda"}}, "cuda")
    with pytest.raises(ValueError, match="not an image selector"):
        image_selector({"type": "SelectorCompose", "args": {}}, "cuda")
    with pytest.raises(ValueError, match="not a GPU device"):
        image_selector({"type": "GradientSelector", "args": args}, "cpu")
    for a in (dict(args, nms_size=4), dict(args, nms_size=17), dict(mask_width=32, grad_std=0, nms_size=3)):
        with pytest.raises(ValueError):
            image_selector({"type": "SparseGradienSelector", "args": a}, "cuda")
    with pytest.raises(KeyError):
        image_selector({"type": "GradientSelector", "args": dict(args, nms_size=3)}, "cuda")
    with pytest.raises(ValueError, match="no HIP form"):
        selector_config_fields({"type": "SelectorCompose", "args": {"mask_width": 32}})
