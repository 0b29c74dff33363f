"""CPU: RandomSelector / GridSelector without a GPU.  The torch restatements (tests/selectors_ref.py) and the library's host-side twins — the device
phase functions of csrc/kp_draw_dev.h emulated thread by thread (mv_kp_random_emulated), the host generator of the seeded finish (mv_kp_random_heads),
mv_kp_grid_count — reproduce the reference's own classes recorded in tests/golden/selectors.npz and torch.randint itself bit for bit; the frame
driver's configuration check knows the three new selector modes and the capacity rule; `selector_config_fields` maps every `keypoint` block of the
experiment YAMLs; the plugins register."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import selectors_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "selectors.npz")


@pytest.fixture(scope="module")
def g():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def lib():
    from macvo_amd import _lib as L

    return L.load()


def _torch_calls(seed, calls, n, H, W, m):
    gen = torch.Generator().manual_seed(seed)
    return torch.stack([SR.random_select(n, H, W, m, gen) for _ in range(calls)]).numpy(), gen


def test_golden_covers_the_cases_the_selectors_are_specified_on(g):
    assert [tuple(int(v) for v in r) for r in g["cases"]] == list(SR.CASES) and tuple(int(s) for s in g["seeds"]) == SR.RANDOM_SEEDS
    rows = {c: int(g[f"grid_{i}"].shape[0]) for i, c in enumerate(SR.CASES)}
    # GridSelector may return MORE rows than numPoint
    assert rows[(480, 640, 32, 200)] == 231 and rows[(720, 1280, 32, 200)] == 231 and rows[(480, 640, 32, 2000)] == 2048 and rows[(480, 640, 0, 200)] == 200
    assert (g["grid_raised"] == 1).all()      # the reference raises on every GRID_RAISES shape


@pytest.mark.parametrize("ci", range(len(SR.CASES)))
def test_restatements_match_reference_golden(g, ci):
    H, W, m, n = SR.CASES[ci]
    assert torch.equal(SR.grid_select(n, H, W, m), torch.from_numpy(g[f"grid_{ci}"]))
    for seed in SR.RANDOM_SEEDS:
        torch.manual_seed(seed)     # the global CPU generator, as the reference consumes it
        rows = torch.stack([SR.random_select(n, H, W, m) for _ in range(SR.RANDOM_CALLS)])
        assert rows.dtype == torch.int64 and torch.equal(rows, torch.from_numpy(g[f"random_{ci}_{seed}"]))
        assert torch.equal(torch.randperm(SR.RANDPERM_N)[: SR.RANDPERM_K], torch.from_numpy(g[f"randperm_{ci}_{seed}"]))
        assert int(rows[..., 0].min()) >= m and int(rows[..., 0].max()) < W - m and int(rows[..., 1].min()) >= m and int(rows[..., 1].max()) < H - m


@pytest.mark.parametrize("threads", (1, 64, 256, 1000))
def test_emulated_device_draw_and_host_twin_equal_golden_and_torch_randint(g, lib, threads):
    """2 * numPoint words per call: numPoint 200 x 8 frames crosses the 624-word block boundary inside frames 2, 4, 5 and 7; numPoint 512 needs two block
    steps inside one call.  The permutation drawn afterwards from the same state is torch.randperm's."""
    for ci, (H, W, m, n) in enumerate(SR.CASES):
        if n > lib.mv_kp_random_max_point():
            out = np.zeros((1, n, 2), dtype=np.int64)
            assert lib.mv_kp_random_emulated(C.c_uint64(5), 1, n, H, W, m, threads, out.ctypes.data) == -2      # MV_ERR_UNSUPPORTED
            continue
        for seed in SR.RANDOM_SEEDS:
            gold = g[f"random_{ci}_{seed}"]
            calls = gold.shape[0]
            assert calls >= 8
            out = np.full((calls, n, 2), -1, dtype=np.int64)
            perm = np.full((SR.RANDPERM_K,), -1, dtype=np.int64)
            assert lib.mv_kp_random_then_randperm_emulated(C.c_uint64(seed), calls, n, H, W, m, threads, out.ctypes.data, SR.RANDPERM_N, SR.RANDPERM_K,
                                                           perm.ctypes.data) == 0
            assert np.array_equal(out, gold), (ci, seed, threads)
            assert np.array_equal(perm, g[f"randperm_{ci}_{seed}"]), (ci, seed, threads)
            out2 = np.full_like(out, -1)
            assert lib.mv_kp_random_emulated(C.c_uint64(seed), calls, n, H, W, m, threads, out2.ctypes.data) == 0 and np.array_equal(out2, gold)
            host = np.full_like(out, -1)
            assert lib.mv_kp_random_heads(C.c_uint64(seed), calls, n, H, W, m, host.ctypes.data) == 0 and np.array_equal(host, gold)
    # ... and against torch.randint directly, other seeds, a long run (16 frames of 200 = 6400 words, ten blocks) and 512 rows per call
    for seed, calls, n, H, W, m in ((7, 16, 200, 480, 640, 32), (99, 5, 512, 720, 1280, 31), (2 ** 35 + 3, 9, 313, 96, 128, 0), (1, 700, 1, 64, 64, 3)):
        ref, gen = _torch_calls(seed & 0xFFFFFFFF if seed >= 2 ** 32 else seed, calls, n, H, W, m)
        out = np.full((calls, n, 2), -1, dtype=np.int64)
        perm = np.full((200,), -1, dtype=np.int64)
        assert lib.mv_kp_random_then_randperm_emulated(C.c_uint64(seed), calls, n, H, W, m, threads, out.ctypes.data, 5000, 200, perm.ctypes.data) == 0
        assert np.array_equal(out, ref), (seed, threads)
        assert np.array_equal(perm, torch.randperm(5000, generator=gen)[:200].numpy()), (seed, threads)
        host = np.full_like(out, -1)
        assert lib.mv_kp_random_heads(C.c_uint64(seed), calls, n, H, W, m, host.ctypes.data) == 0 and np.array_equal(host, ref)


def test_random_draw_rejects_an_empty_masked_image(lib):
    out = np.zeros((1, 4, 2), dtype=np.int64)
    for (H, W, m) in ((64, 640, 32), (480, 64, 32), (480, 640, -1)):
        assert lib.mv_kp_random_emulated(C.c_uint64(1), 1, 4, H, W, m, 64, out.ctypes.data) == -1
        assert lib.mv_kp_random_heads(C.c_uint64(1), 1, 4, H, W, m, out.ctypes.data) == -1


def test_grid_count_matches_golden_and_is_zero_where_the_reference_raises(g, lib):
    for ci, (H, W, m, n) in enumerate(SR.CASES):
        assert lib.mv_kp_grid_count(H, W, m, n) == g[f"grid_{ci}"].shape[0] == SR.grid_count(n, H, W, m), SR.CASES[ci]
    for (H, W, m, n) in SR.GRID_RAISES:
        with pytest.raises((ZeroDivisionError, RuntimeError)):
            SR.grid_select(n, H, W, m)
        assert lib.mv_kp_grid_count(H, W, m, n) == 0
    # a sweep of shapes against the restatement (counts only)
    for H in (96, 192, 480, 720):
        for W in (128, 640, 1280):
            for m in (0, 5, 32):
                for n in (1, 2, 7, 50, 200, 999, 2000):
                    assert lib.mv_kp_grid_count(H, W, m, n) == SR.grid_count(n, H, W, m), (H, W, m, n)


def _cfg_factory():
    from macvo_amd import _lib as L

    lib = L.load()
    lm = L.mvLMParams()
    lib.mv_lm_default_params(C.byref(lm))

    def cfg(**kw):
        d = dict(H=480, W=640, C=256, pairs=2, iters=12, radius=4, feat_dtype=L.MV_F32, layout=L.MV_LAYOUT_CHW, volume_split=0,
                 selector_mode=L.MV_KP_NODEPTH, kp_kernel_size=7, kp_mask_width=32, num_point=200, edgewidth=32,
                 min_num_point=10, graph_type=L.MV_GRAPH_DISP, filters=1, cov_kernel_size=31, fx=320.0, fy=320.0, cx=320.0,
                 cy=240.0, baseline=0.25, bl_fx=80.0, bl_fx_sq=6400.0, match_cov_default=0.25, max_match_cov=100.0,
                 max_depth_cov=250.0, max_depth=80.0, min_flow_cov_sq=0.0625, min_depth_cov=0.05, filter_min_depth=0.05,
                 map_max_depth=5.0, map_max_depth_cov=0.005, lm=lm)
        d.update(kw)
        return L.mvFramePipeConfig(**d)

    return L, lib, cfg


def test_frame_pipe_config_knows_the_new_selector_modes_and_the_capacity_rule():
    L, lib, cfg = _cfg_factory()
    assert lib.mv_abi_version() == L.ABI_VERSION == 8
    assert (L.MV_KP_NODEPTH, L.MV_KP_FULL, L.MV_KP_MAPPING, L.MV_KP_RANDOM, L.MV_KP_GRID, L.MV_KP_EXPLICIT) == (0, 1, 2, 3, 4, 5)
    size = lambda **kw: lib.mv_frame_pipe_arena_bytes(C.byref(cfg(**kw)))  # noqa: E731
    rows = lambda **kw: lib.mv_frame_pipe_table_rows(C.byref(cfg(**kw)))  # noqa: E731
    base = size()
    n_rand, n_grid, n_expl = size(selector_mode=L.MV_KP_RANDOM), size(selector_mode=L.MV_KP_GRID), size(selector_mode=L.MV_KP_EXPLICIT)
    assert n_rand == n_expl == base > 0                      # same tables: capacity = num_point
    assert n_grid > base                                     # 231 rows of capacity instead of 200
    assert rows() == rows(selector_mode=L.MV_KP_RANDOM) == rows(selector_mode=L.MV_KP_EXPLICIT) == 200 and rows(selector_mode=L.MV_KP_GRID) == 231
    assert rows(selector_mode=L.MV_KP_GRID, kp_mask_width=0, cov_model=L.MV_COV_NONE) == 200
    assert rows(selector_mode=L.MV_KP_GRID, num_point=2000) == 2048
    # a grid with FEWER rows than num_point keeps num_point rows of capacity: 640 x 480, mask 0, 201 -> unit 10 -> 10 x 20 = 200 rows
    assert SR.grid_count(201, 480, 640, 0) == 200 and rows(selector_mode=L.MV_KP_GRID, num_point=201, kp_mask_width=0, cov_model=L.MV_COV_NONE) == 201
    assert size(selector_mode=L.MV_KP_MAPPING) == 0          # still not a pipe's selector
    assert size(selector_mode=6) == 0
    # the 31 x 31 covariance patch must stay inside the image: mask_width >= 15 for the patch-based models, anything for NoCovariance
    for mode in (L.MV_KP_RANDOM, L.MV_KP_GRID, L.MV_KP_EXPLICIT):
        assert size(selector_mode=mode, kp_mask_width=8, cov_model=L.MV_COV_MATCH) == 0
        assert size(selector_mode=mode, kp_mask_width=8, cov_model=L.MV_COV_GMM) == 0
        assert size(selector_mode=mode, kp_mask_width=8, cov_model=L.MV_COV_NONE) > 0
        assert size(selector_mode=mode, kp_mask_width=15) > 0 and size(selector_mode=mode, kp_mask_width=14) == 0
        assert size(selector_mode=mode, kp_mask_width=240) == 0 and size(selector_mode=mode, kp_mask_width=-1) == 0       # H <= 2 * mask
    assert size(kp_mask_width=8) == base                     # the CovAware modes are as they were
    # where the reference's GridSelector raises: count 0, no arena
    for (H, W, m, n) in SR.GRID_RAISES:
        Hc, Wc = (H + 7) // 8 * 8, (W + 7) // 8 * 8
        if lib.mv_kp_grid_count(Hc, Wc, m, n) == 0:
            assert size(H=Hc, W=Wc, kp_mask_width=m, num_point=n, selector_mode=L.MV_KP_GRID, cov_model=L.MV_COV_NONE) == 0
            assert rows(H=Hc, W=Wc, kp_mask_width=m, num_point=n, selector_mode=L.MV_KP_GRID, cov_model=L.MV_COV_NONE) == 0
    assert lib.mv_kp_grid_count(480, 640, 236, 200) == 0 and size(kp_mask_width=236, selector_mode=L.MV_KP_GRID, cov_model=L.MV_COV_NONE) == 0
    # capacities: the device draw covers mv_kp_random_max_point() rows, the tables MV_KP_TABLE_MAX
    assert lib.mv_kp_random_max_point() == 512
    assert size(selector_mode=L.MV_KP_RANDOM, num_point=512) > 0 and size(selector_mode=L.MV_KP_RANDOM, num_point=513) == 0
    assert size(selector_mode=L.MV_KP_EXPLICIT, num_point=L.MV_KP_TABLE_MAX) > 0 and size(selector_mode=L.MV_KP_EXPLICIT, num_point=L.MV_KP_TABLE_MAX + 1) == 0
    assert size(selector_mode=L.MV_KP_GRID, num_point=5000) == 0
    # lanes, the dense-mapping tail, the motion model and the covariance models combine with the new modes
    assert size(selector_mode=L.MV_KP_RANDOM, pairs=8) > 3 * base
    assert size(selector_mode=L.MV_KP_GRID, mapping=1, map_num_point=2000, map_mask_width=32) > 0
    assert size(selector_mode=L.MV_KP_RANDOM, motion_model=L.MV_MOTION_TARTAN, cov_model=L.MV_COV_GMM, cov_modifiers=L.MV_COVMOD_DIAG) > 0


# `keypoint` blocks of the experiment YAMLs (Config/Experiment/MACVO/**; `device: *device` = cuda, `max_depth: *max_depth` = auto), copied as data
_COVAWARE = {"type": "CovAwareSelector", "args": {"device": "cuda", "kernel_size": 7, "mask_width": 32, "max_depth": "auto", "max_depth_cov": 250.0,
                                                   "max_match_cov": 100.0}}
_RANDOM = {"type": "RandomSelector", "args": {"mask_width": 32, "device": "cuda"}}
_NODEPTH = {"type": "CovAwareSelector_NoDepth", "args": {"device": "cuda", "kernel_size": 7, "mask_width": 32, "max_match_cov": 100.0}}
KEYPOINT_BLOCKS = {
    "Ablation_Study/TartanAirv2_CovDiag.yaml": _COVAWARE, "Ablation_Study/TartanAirv2_CovKP.yaml": _COVAWARE,
    "Ablation_Study/TartanAirv2_CovOpt.yaml": _RANDOM, "Ablation_Study/TartanAirv2_Full.yaml": _COVAWARE,
    "Ablation_Study/TartanAirv2_NormDiag.yaml": _COVAWARE, "Ablation_Study/TartanAirv2_NormFrame.yaml": _COVAWARE,
    "Ablation_Study/TartanAirv2_NormPoint.yaml": _COVAWARE, "Ablation_Study/TartanAirv2_ScaleNorm.yaml": _COVAWARE,
    "Ablation_Study/TartanAirv2_Vanilla.yaml": _RANDOM, "MACVO_Fast.yaml": _NODEPTH, "MACVO_Performant.yaml": _NODEPTH,
}


def _ns(d):
    return SimpleNamespace(**{k: _ns(v) if isinstance(v, dict) else v for k, v in d.items()})


def test_selector_config_fields_maps_every_experiment_yaml():
    from macvo_amd.pipeline import Camera, HotPathConfig, check_selector, selector_config_fields, table_rows

    cam = Camera(320.0, 320.0, 320.0, 240.0, 0.25, 480, 640)
    want = {"CovAwareSelector": dict(selector="full", kp_mask_width=32, kp_kernel_size=7, max_depth="auto", max_depth_cov=250.0, max_match_cov=100.0),
            "RandomSelector": dict(selector="random", kp_mask_width=32),
            "CovAwareSelector_NoDepth": dict(selector="nodepth", kp_mask_width=32, kp_kernel_size=7, max_match_cov=100.0)}
    assert len(KEYPOINT_BLOCKS) == 11
    for name, block in KEYPOINT_BLOCKS.items():
        for form in (block, _ns(block), {"type": "HIP_" + block["type"], "args": block["args"]}):
            f = selector_config_fields(form)
            assert f == want[block["type"]], name
            cfg = HotPathConfig(**f)
            check_selector(cfg, cam)
            assert table_rows(cfg, cam) == 200
    f = selector_config_fields({"type": "GridSelector", "args": {"mask_width": 32, "device": "cuda"}})
    assert f == dict(selector="grid", kp_mask_width=32) and table_rows(HotPathConfig(**f), cam) == 231
    for t in ("GradientSelector", "SparseGradienSelector", "SelectorCompose", "NoKeypointSelector"):
        with pytest.raises(ValueError, match="no HIP form"):
            selector_config_fields({"type": t, "args": {"mask_width": 32}})
    # configuration-time rejections carry their reason
    with pytest.raises(ValueError, match="covariance patch"):
        check_selector(HotPathConfig(selector="random", kp_mask_width=8), cam)
    check_selector(HotPathConfig(selector="random", kp_mask_width=8, cov_model="none"), cam)
    check_selector(HotPathConfig(selector="nodepth", kp_mask_width=8), cam)          # the CovAware selectors are as they were
    with pytest.raises(ValueError, match="grid step of 0"):
        check_selector(HotPathConfig(selector="grid", kp_mask_width=236, cov_model="none"), cam)
    with pytest.raises(ValueError, match="leaves no pixel"):
        check_selector(HotPathConfig(selector="explicit", kp_mask_width=240), cam)
    with pytest.raises(ValueError, match="num_point 513"):
        check_selector(HotPathConfig(selector="random", num_point=513), cam)
    with pytest.raises(ValueError, match="selector must be one of"):
        check_selector(HotPathConfig(selector="gradient"), cam)
    # the NMS window of the CovAware selectors: odd, 1..15 (the kernel's halo) — refused here, not as MV_ERR_UNSUPPORTED on the first frame
    for sel in ("nodepth", "full"):
        for k in (1, 9, 15):
            check_selector(HotPathConfig(selector=sel, kp_kernel_size=k), cam)
        for k in (17, 0, 6, -1):
            with pytest.raises(ValueError, match="kp_kernel_size"):
                check_selector(HotPathConfig(selector=sel, kp_kernel_size=k), cam)
    check_selector(HotPathConfig(selector="grid", kp_kernel_size=17), cam)           # ... which the map-less selectors never read


def test_vanilla_and_covopt_blocks_instantiate_the_hip_plugins():
    import macvo_amd.plugins as P
    from macvo_amd import interfaces as I

    for name in ("Ablation_Study/TartanAirv2_Vanilla.yaml", "Ablation_Study/TartanAirv2_CovOpt.yaml"):
        block = _ns(KEYPOINT_BLOCKS[name])
        block.type = "HIP_" + block.type
        I.IKeypointSelector.is_valid_config(block)
        sel = I.IKeypointSelector.instantiate(block.type, block.args) if hasattr(I.IKeypointSelector, "instantiate") else I.IKeypointSelector.get_class(block.type)(block.args)
        assert isinstance(sel, P.HIP_RandomSelector)
    grid = SimpleNamespace(type="HIP_GridSelector", args=SimpleNamespace(mask_width=32, device="cuda"))
    I.IKeypointSelector.is_valid_config(grid)
    assert I.IKeypointSelector.get_class("HIP_GridSelector") is P.HIP_GridSelector
    P.HIP_RandomSelector.is_valid_config(SimpleNamespace(mask_width=32, device="cuda", seed=7))
    for bad in (SimpleNamespace(mask_width=-1, device="cuda"), SimpleNamespace(mask_width=32, device="tpu"), SimpleNamespace(mask_width=32, device="cuda", seed=-1),
                SimpleNamespace(mask_width=32, device="cuda", seed="x"), SimpleNamespace(mask_width=32, device="cpu", seed=3)):
        with pytest.raises(ValueError):
            P.HIP_RandomSelector.is_valid_config(bad)
    with pytest.raises(KeyError):
        P.HIP_RandomSelector.is_valid_config(SimpleNamespace(mask_width=32, device="cuda", extra=1))
    with pytest.raises(KeyError):
        P.HIP_GridSelector.is_valid_config(SimpleNamespace(mask_width=32))


def test_unseeded_random_plugin_is_the_reference_draw_on_the_global_cpu_generator(g):
    """device "cpu" keeps the rows on the host: bit-exact with the reference class's golden rows, in the same word stream as a following randperm."""
    import macvo_amd.plugins as P

    for ci, (H, W, m, n) in enumerate(SR.CASES[:2]):
        sel = P.HIP_RandomSelector(SimpleNamespace(mask_width=m, device="cpu"))
        frame = SimpleNamespace(height=H, width=W)
        torch.manual_seed(SR.RANDOM_SEEDS[0])
        rows = torch.stack([sel.select_point(frame, n, None, None, None) for _ in range(SR.RANDOM_CALLS)])
        assert torch.equal(rows, torch.from_numpy(g[f"random_{ci}_{SR.RANDOM_SEEDS[0]}"]))
        assert torch.equal(torch.randperm(SR.RANDPERM_N)[: SR.RANDPERM_K], torch.from_numpy(g[f"randperm_{ci}_{SR.RANDOM_SEEDS[0]}"]))
