"""GPU: covariance-free frontends in the native frame driver (``mvFramePipeConfig.frontend_nocov``).

* ``NativeHotPath`` against ``HotPath`` — bit for bit, every backend table and pose — for each (d, m), map-less selector, covariance model with
  and without modifiers, motion model, both input forms (upsampled fields, 1/8-resolution fields + convex-upsampling masks) and every finish
  mode the selector has (torch generators -> keypoint rows, host-seeded, drawn inside the front launch, explicit host / device keypoints); the
  five-launch backend too; (0, 1) with the CovAware selector;
* three lanes: each lane equals its solo run;
* the Vanilla golden through the driver (keypoints and stored rows bit-equal, covariances 5e-5, poses 1e-4);
* the device-resident map: the -1 placeholders arrive in the stored rows;
* ``mv_frame_pipe_create`` refusals, ``mv_frame_pipe_buffer`` errors for maps the pipe does not have;
* a default (1, 1) pipe before and after a cov-free pipe in the same process: identical bits."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import refrun, synth
from tests.test_gpu_covfree import _cfg_of, case, check_frame_against_golden
from tests.test_gpu_selectors_native import TABLES, _assert_same, _bits, _ins, _lane_frames, _Net, _snapshot

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DM = ((False, False), (True, False), (False, True))


def _strip(x, d, m):
    """The inputs a (d, m) frontend hands over: no covariance at all without both, else the full tensor with the unprovided pair poisoned (it must
    not be read)."""
    from dataclasses import replace

    def poison(t):
        if t is None:
            return None
        if not (d or m):
            return None
        t = t.clone()
        lanes = t.shape[0] // 2
        for l in range(lanes):
            if not d:
                t[2 * l] = float("nan")
            if not m:
                t[2 * l + 1] = float("nan")
        return t
    return replace(x, logcov=poison(x.logcov), cov8=poison(x.cov8), cov_mask=poison(x.cov_mask))


def _py_snapshot(r):
    ex, tr = r.extras, r.extras["tracked"]
    return dict(KP0=r.kp0_uv, KP0F=tr.kp0_uv, KP1=tr.kp1_uv, INBOUND=tr.inbound.view(torch.uint8), SIGMA0=tr.sigma0, SIGMA1=tr.sigma1, COV0=ex["cov0"],
                COV0W=ex["cov0_w"], COV1=ex["cov1"], VALID=ex["valid"].view(torch.uint8), POS_TW=ex["pos_Tw"], VALS=tr.vals, pose=r.pose)


def _assert_native_is_python(nat_snap, py, what):
    for k, v in py.items():
        a, b = nat_snap[k], v
        if k in ("INBOUND", "VALID"):
            a, b = a.view(torch.uint8), b.view(torch.uint8)
        if k == "VALS":
            inb = py["INBOUND"].bool()
            a, b = a[:, inb], b[:, inb]                 # (rows out of bounds: the fused launch and kp_track agree on what they store, compare live rows)
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (what, k)


def _upsampled_inputs(n, H, W, seed, dev):
    """FrameInputs in the 1/8-resolution form (flow8 / cov8 + masks), as tests/test_gpu_native.py builds them."""
    from macvo_amd.pipeline import FrameInputs

    cam, frames, _ = synth.make_sequence(n, H, W, C=32, iters=2, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    out = []
    for fr in frames:
        h8, w8 = H // 8, W // 8
        flow8 = torch.nn.functional.avg_pool2d(fr["flow"], 8) / 8.0
        cov8 = torch.nn.functional.avg_pool2d(fr["logcov"], 8)
        up_mask = torch.randn(2, 576, h8, w8, generator=g)
        cov_mask = torch.randn(2, 576, h8, w8, generator=g) * 0.25
        out.append(FrameInputs(fmap1=fr["fmap1"].to(dev), fmap2=fr["fmap2"].to(dev), coords=fr["coords"].to(dev), flow8=flow8.to(dev), cov8=cov8.to(dev),
                               up_mask=up_mask.to(dev), cov_mask=cov_mask.to(dev)))
    torch.cuda.synchronize()
    return cam, out


_COMBOS = [("random", "none", (), "static", False), ("random", "match", (), "tartan", False), ("grid", "match", ("diag", "normalize"), "static", False),
           ("grid", "none", ("diag",), "tartan", True), ("random", "match", ("normalize",), "static", True), ("explicit", "match", (), "static", False),
           ("explicit", "gmm", (), "static", False), ("explicit", "gmm", ("diag",), "static", True)]


# (the mixture model needs the depth model's covariance: without it the combination is refused, see the refusal tests)
@pytest.mark.parametrize("d,m,selector,cov_model,mods,motion,upsampled", [(d, m) + c for d, m in DM for c in _COMBOS if c[1] != "gmm" or d])
def test_native_equals_python_loop(gpu, monkeypatch, d, m, selector, cov_model, mods, motion, upsampled):
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath

    n_frames, H, W = 4, 192, 256
    if upsampled:
        cam, ins = _upsampled_inputs(n_frames, H, W, 23, gpu)
    else:
        cam, fr, _ = synth.make_sequence(n_frames, H, W, C=32, iters=2, seed=23)
        ins = _ins(fr, gpu)
    ins = [_strip(x, d, m) for x in ins]
    cfg = HotPathConfig(frontend_cov=(d, m), selector=selector, cov_model=cov_model, cov_modifiers=mods, motion_model=motion, graph_type="icp",
                        cov_match_cov_default=0.5, filters=7, kp_mask_width=32)
    net = (lambda: _Net(gpu)) if motion == "tartan" else (lambda: None)
    kps = None
    if selector == "explicit":
        g = torch.Generator().manual_seed(3)
        kps = [torch.stack([torch.randint(32, W - 32, (150,), generator=g), torch.randint(32, H - 32, (150,), generator=g)], dim=1) for _ in range(n_frames)]
    py = HotPath(Camera(**cam), cfg, gpu, keep_extras=True, pose_net=net(), generator=torch.Generator().manual_seed(9))
    py.initialize(ins[0])
    want = []
    for t in range(1, n_frames):
        r = py.step(ins[t], keypoints=None if kps is None else kps[t])
        torch.cuda.synchronize()
        want.append({k: v.clone() for k, v in _py_snapshot(r).items()})
        assert int(r.n_valid.item()) >= cfg.min_num_point
    modes = {"random": ("host", "seeded", "device"), "grid": ("device",), "explicit": ("host", "devkp")}[selector]
    for mode in modes:
        for fuse in (("1", "0") if mode == "host" else ("1",)):    # (the five-launch backend: host-fed finishes only, as before)
            monkeypatch.setenv("MV_PIPE_DEVICE_DRAW", "0" if mode == "seeded" else "1")
            monkeypatch.setenv("MV_PIPE_FUSE_BACKEND", fuse)
            gens = [torch.Generator().manual_seed(9)] if mode in ("host", "devkp") else [9]
            nat = NativeHotPath(Camera(**cam), cfg, gpu, keep_extras=True, generators=gens, pose_net=net())
            nat.initialize(ins[0])
            for t in range(1, n_frames):
                kp = None if kps is None else (kps[t].to(gpu) if mode == "devkp" else kps[t])
                r = nat.step(ins[t], keypoints=kp)
                torch.cuda.synchronize()
                snap = _snapshot(nat, r)[0]
                _assert_native_is_python(snap, want[t - 1], (d, m, selector, cov_model, mods, motion, upsampled, mode, fuse, t))
                if not m:
                    assert (snap["SIGMA1"] == -1).all()
                if not d:
                    assert (snap["VALS"][[2, 3]] == -1).all() and (snap["VALS"][[6, 7]][:, snap["INBOUND"].bool()] == -1).all()
                fm = nat.maps()
                assert (fm.depth_cov is None) == (not d) and (fm.flow_cov is None) == (not m)
            nat.close()


def test_covaware_selector_without_depth_covariance(gpu, monkeypatch):
    """(0, 1) keeps the CovAware selector (it reads match.cov only) and the reproj graph: host-drawn, host-seeded and device-drawn finishes."""
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath

    n_frames = 4
    cam, fr, _ = synth.make_sequence(n_frames, 192, 256, C=32, iters=2, seed=29)
    ins = [_strip(x, False, True) for x in _ins(fr, gpu)]
    cfg = HotPathConfig(frontend_cov=(False, True), selector="nodepth", graph_type="reproj", cov_modifiers=("diag",), filters=7)
    py = HotPath(Camera(**cam), cfg, gpu, keep_extras=True, generator=torch.Generator().manual_seed(4))
    py.initialize(ins[0])
    want = []
    for t in range(1, n_frames):
        r = py.step(ins[t])
        torch.cuda.synchronize()
        want.append({k: v.clone() for k, v in _py_snapshot(r).items()})
    for mode in ("host", "seeded", "device"):
        monkeypatch.setenv("MV_PIPE_DEVICE_DRAW", "0" if mode == "seeded" else "1")
        nat = NativeHotPath(Camera(**cam), cfg, gpu, keep_extras=True, generators=[torch.Generator().manual_seed(4)] if mode == "host" else [4])
        nat.initialize(ins[0])
        for t in range(1, n_frames):
            r = nat.step(ins[t])
            torch.cuda.synchronize()
            _assert_native_is_python(_snapshot(nat, r)[0], want[t - 1], (mode, t))
        nat.close()


@pytest.mark.parametrize("d,m", DM)
def test_three_lanes_equal_their_solo_runs(gpu, d, m):
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath, stack_lanes

    lanes, n_frames = 3, 4
    cam, per_lane = _lane_frames(lanes, n_frames, 41)
    ins = [[_strip(x, d, m) for x in _ins(fr, gpu)] for fr in per_lane]
    stacked = [stack_lanes([ins[l][t] for l in range(lanes)]) for t in range(n_frames)]
    cfg = HotPathConfig(frontend_cov=(d, m), selector="random", cov_model="match", cov_match_cov_default=0.5, graph_type="icp", filters=7)
    seeds = [3, 14, 15]
    hot = NativeHotPath(Camera(**cam), cfg, gpu, lanes=lanes, generators=list(seeds))
    hot.initialize(stacked[0])
    multi = []
    for t in range(1, n_frames):
        res = hot.step(stacked[t])
        torch.cuda.synchronize()
        multi.append(_snapshot(hot, res))
    hot.close()
    for l in range(lanes):
        solo = NativeHotPath(Camera(**cam), cfg, gpu, lanes=1, generators=[seeds[l]])
        solo.initialize(ins[l][0])
        for t in range(1, n_frames):
            res = solo.step(ins[l][t])
            torch.cuda.synchronize()
            _assert_same(_snapshot(solo, res), [multi[t - 1][l]], (d, m, l, t))
        solo.close()


def test_vanilla_golden_through_the_driver(gpu):
    from macvo_amd.pipeline import Camera, NativeHotPath
    from tests.test_gpu_covfree import _inputs

    z = np.load(os.path.join(ROOT, "tests", "golden", "covfree.npz"))
    gold = {k: z[k] for k in z.files}
    meta = json.loads(str(gold["meta"]))
    cam, maps, _ = refrun.tartanair_maps()
    ins = _inputs(maps, cam, gpu, False, False)
    for name in ("vanilla", "00_grid_match"):
        g = case(gold, name)
        hot = NativeHotPath(Camera(**cam), _cfg_of(meta, name), gpu, keep_extras=True, generators=[meta["seed"]])   # torch.Generator().manual_seed(seed)'s bits
        hot.initialize(ins[0])
        for t in range(1, len(ins)):
            r = hot.step(ins[t])
            torch.cuda.synchronize()
            check_frame_against_golden(g, t, r.extras, r.kp0_uv, r.pose, False, False, f"NativeHotPath {name}", exact_variances=True)
        hot.close()


def test_device_map_stores_the_placeholders(gpu):
    from macvo_amd.devmap import DeviceVisualMap
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath

    n_frames = 6
    cam, fr, _ = synth.make_sequence(n_frames, 240, 320, C=32, iters=2, seed=8)
    K = torch.tensor([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1.0]])
    for d, m in DM:
        ins = [_strip(x, d, m) for x in _ins(fr, gpu)]
        hot = NativeHotPath(Camera(**cam), HotPathConfig(frontend_cov=(d, m), selector="random", cov_model="match", graph_type="icp", filters=2),
                            gpu, generators=[5])
        dmap = DeviceVisualMap(gpu, init_size=64)
        hot.attach_map(dmap, K, None)
        hot.initialize(ins[0])
        for _ in hot.run(ins[1:]):
            pass
        hot.synchronize()
        got = dmap.serialize()
        hot.close()
        assert got["match//pixel1_uv"].shape[0] > 10 * (n_frames - 1) and not got["frames//need_interp"].any()
        for k in ("pixel1_d_cov", "pixel2_d_cov", "pixel1_disp_cov", "pixel2_disp_cov"):
            assert bool((got[f"match//{k}"] == -1).all()) == (not d), (d, m, k)
            assert d or got[f"match//{k}"].dtype == np.float32
        assert bool((got["match//pixel2_uv_cov"] == -1).all()) == (not m), (d, m)
        assert (got["match//pixel1_uv_cov"] == np.float32([0.25, 0.25, 0.0])).all()
        assert np.isfinite(got["match//obs2_covTc"]).all() and np.isfinite(got["points//cov_Tw"]).all()


def test_create_refusals_and_absent_buffers(gpu):
    from macvo_amd import _lib as L
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath

    cam, fr, _ = synth.make_sequence(2, 192, 256, C=32, iters=2, seed=2)
    ins = _ins(fr, gpu)
    ok = HotPathConfig(frontend_cov=(False, False), selector="random", cov_model="none", graph_type="icp")
    hot = NativeHotPath(Camera(**cam), ok, gpu, generators=[1])
    hot.initialize(_strip(ins[0], False, False))
    hot.step(_strip(ins[1], False, False))
    torch.cuda.synchronize()
    lib, pc = hot._lib, hot._pc
    ptr, cnt = C.c_void_p(), C.c_size_t()
    for name in ("DISPARITY_COV", "DEPTH_COV", "MATCH_COV"):
        rc = lib.mv_frame_pipe_buffer(hot._pipe, L.FB[name], 0, C.byref(ptr), C.byref(cnt))
        assert rc != 0 and not ptr.value and cnt.value == 0, name                # an error, never a stale slot
    for name in ("DEPTH", "DISPARITY", "MATCH_FLOW"):
        assert lib.mv_frame_pipe_buffer(hot._pipe, L.FB[name], 0, C.byref(ptr), C.byref(cnt)) == 0 and ptr.value
    # a frontend with covariances must still hand them over; one without may leave them out
    full = NativeHotPath(Camera(**cam), HotPathConfig(selector="random", graph_type="icp"), gpu, generators=[1])
    with pytest.raises(L.MacvoHipError):
        full.initialize(_strip(ins[0], False, False))
    full.close()
    # create: the existing invalid-configuration code for every refused combination
    arena = torch.empty(lib.mv_frame_pipe_arena_bytes(C.byref(pc)) + 256, dtype=torch.uint8, device=gpu)
    base = (arena.data_ptr() + 255) & ~255

    def create(**kw):
        bad = L.mvFramePipeConfig.from_buffer_copy(pc)
        for k, v in kw.items():
            setattr(bad, k, v)
        out = C.c_void_p()
        rc = lib.mv_frame_pipe_create(C.byref(bad), base, arena.numel() - 256, C.byref(out))
        if rc == 0:
            lib.mv_frame_pipe_destroy(out)
        return rc, lib.mv_frame_pipe_arena_bytes(C.byref(bad))
    want_rc, _ = create(radius=9)                                                # what an invalid configuration has always returned
    assert want_rc != 0
    for kw in (dict(graph_type=L.MV_GRAPH_DISP), dict(graph_type=L.MV_GRAPH_REPROJ), dict(selector_mode=L.MV_KP_NODEPTH), dict(selector_mode=L.MV_KP_FULL),
               dict(frontend_nocov=L.MV_NOCOV_DEPTH, cov_model=L.MV_COV_GMM), dict(frontend_nocov=L.MV_NOCOV_DEPTH, mapping=1, map_num_point=100),
               dict(frontend_nocov=L.MV_NOCOV_MATCH, cov_model=L.MV_COV_MATCH, cov_match_cov_default=0.0), dict(frontend_nocov=7)):
        rc, nbytes = create(**kw)
        assert rc == want_rc and nbytes == 0, kw
    assert create(frontend_nocov=L.MV_NOCOV_MATCH, cov_model=L.MV_COV_GMM)[1] > 0   # (1, 0) keeps the mixture model
    hot.close()


def test_default_pipe_is_untouched_by_a_covfree_pipe_in_the_same_process(gpu):
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath

    n_frames = 5
    cam, fr, _ = synth.make_sequence(n_frames, 192, 256, C=32, iters=2, seed=17)
    ins = _ins(fr, gpu)

    def default_run():
        hot = NativeHotPath(Camera(**cam), HotPathConfig(), gpu, keep_extras=True, generators=[21])
        hot.initialize(ins[0])
        out = []
        for t in range(1, n_frames):
            r = hot.step(ins[t])
            torch.cuda.synchronize()
            s = _snapshot(hot, r)
            fm = hot.maps()
            s[0].update(depth_cov=fm.depth_cov.clone(), flow_cov=fm.flow_cov.clone(), disparity_cov=fm.disparity_cov.clone(), depth=fm.depth.clone())
            out.append(s)
        hot.close()
        return out

    before = default_run()
    for d, m in DM:
        hot = NativeHotPath(Camera(**cam), HotPathConfig(frontend_cov=(d, m), selector="random", cov_model="match", graph_type="icp"), gpu, generators=[2])
        hot.initialize(_strip(ins[0], d, m))
        for t in range(1, n_frames):
            hot.step(_strip(ins[t], d, m))
        torch.cuda.synchronize()
        hot.close()
    after = default_run()
    assert all(s[0]["n_sel"] > 0 for s in before)
    for a, b in zip(before, after):
        _assert_same(a, b, "default pipe before / after")
