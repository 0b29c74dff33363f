"""GPU: the frame path end to end at an anisotropic camera (tests/cameras.ANISO_SMALL: fx = 150, fy = 190, cx = 151.25, cy = 127.5, baseline 0.4).
Every other sequence of the suite comes from ``tools.synth.make_camera`` (fx = fy = 320, centred, baseline 0.25), where passing fx for fy, cx for cy or
the wrong baseline anywhere between ``pipeline.py`` and the kernels goes unnoticed.

* ``HotPath`` against ``OracleHotPath`` with the assertions of test_gpu_pipeline.py (test_sequence_matches_oracle, test_dense_mapping_tail_matches_oracle);
* ``NativeHotPath`` against ``HotPath`` bit for bit with the assertion list of test_gpu_native.py::test_native_step_equals_python_step, dense-mapping tail included;
* two lanes of the native driver with device maps: each lane equals its solo run, the maps hold the camera's K and baseline, lane 0's map equals the
  oracle map fed with the same rows (test_gpu_visual_map.py::test_native_driver_fills_the_device_map);
* the motion prior on (test_gpu_motion_native.py::test_native_tartan_equals_python_tartan): the native driver against the Python loop, bit for bit.

All at 240 x 320, C = 32, one decoder iteration, 5 frames."""
import numpy as np
import pytest
import torch

from tests import cameras, synth

pytestmark = pytest.mark.gpu

H, W, N_FRAMES = 240, 320, 5
CAM = cameras.cam_dict(cameras.ANISO_SMALL)
CONFIGS = [("disp", "nodepth"), ("icp", "full"), ("reproj", "nodepth")]
MAPPING = dict(mapping=True, map_max_depth=13.0, map_max_depth_cov=0.5, map_num_point=300)


def _sequence(seed, image=False):
    assert (CAM["H"], CAM["W"]) == (H, W) and CAM["fx"] != CAM["fy"]
    cam, frames, poses = synth.make_sequence(N_FRAMES, H, W, C=32, iters=1, seed=seed, cam=CAM)
    assert cam == CAM
    if image:
        g = torch.Generator().manual_seed(1)
        for fr in frames:
            fr["image"] = torch.rand(1, 3, H, W, generator=g)
    return cam, frames, poses


def _inputs(frames, dev, **kw):
    from macvo_amd.pipeline import FrameInputs

    ins = [FrameInputs(**{k: v.to(dev) for k, v in fr.items()}, **(dict(time_ns=kw["time0"] + 33 * t) if "time0" in kw else {})) for t, fr in enumerate(frames)]
    torch.cuda.synchronize()
    return ins


@pytest.mark.parametrize("graph,selector", CONFIGS)
def test_hot_path_matches_oracle(gpu, graph, selector):
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig
    from oracle import se3
    from oracle.pipeline import OracleHotPath

    cam, frames, true_poses = _sequence(3)
    ora = OracleHotPath(cam, dict(graph_type=graph, selector=selector))
    hot = HotPath(Camera(**cam), HotPathConfig(graph_type=graph, selector=selector), gpu, keep_extras=True)
    ins = _inputs(frames, gpu)
    ora.initialize(frames[0])
    hot.initialize(ins[0])
    for t in range(1, N_FRAMES):
        torch.manual_seed(100 + t)
        ro = ora.step(frames[t])
        torch.manual_seed(100 + t)
        rh = hot.step(ins[t])
        torch.testing.assert_close(hot.last_tokens.cpu(), ora.last_tokens, rtol=1e-5, atol=2e-4)
        assert torch.equal(rh.kp0_uv.cpu(), ro["kp0_uv"]), f"frame {t}: keypoints differ"
        assert int(rh.n_valid.item()) == ro["n_valid"] and ro["n_valid"] >= 150
        ex = rh.extras
        inb = ex["tracked"].inbound.cpu()
        torch.testing.assert_close(ex["cov0"].cpu()[inb], ro["cov0"], rtol=2e-4, atol=1e-7)
        torch.testing.assert_close(ex["cov1"].cpu()[inb], ro["cov1"], rtol=2e-4, atol=1e-7)
        torch.testing.assert_close(ex["pos_Tw"].cpu()[inb], ro["pos_Tw"], rtol=1e-6, atol=1e-6)
        dt, dr = se3.pose_error(ro["pose"].double(), rh.pose.cpu().double())
        assert dt <= 1e-4 and dr <= 1e-4, (t, dt, dr)
        assert int(rh.info[0, 1].item()) == ro["steps"], (t, rh.info.cpu(), ro["steps"])
        et, er = se3.pose_error(true_poses[t], rh.pose.cpu().double())
        assert et < 0.05 and er < 0.01, (t, et, er)
        hot.pose = ro["pose"].to(gpu)


def test_dense_mapping_tail_matches_oracle(gpu):
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig
    from oracle.pipeline import OracleHotPath

    cam, frames, _ = _sequence(23, image=True)
    ora = OracleHotPath(cam, MAPPING)
    hot = HotPath(Camera(**cam), HotPathConfig(**MAPPING), gpu)
    ins = _inputs(frames, gpu)
    ora.initialize(frames[0])
    hot.initialize(ins[0])
    for t in range(1, N_FRAMES):
        torch.manual_seed(70 + t)
        ro = ora.step(frames[t])
        torch.manual_seed(70 + t)
        rh = hot.step(ins[t])
        torch.cuda.synchronize()
        assert torch.equal(rh.kp0_uv.cpu(), ro["kp0_uv"])
        m, mo = rh.map_points, ro["map"]
        assert m is not None and m.uv.shape[0] == 300
        assert torch.equal(m.uv.cpu().long(), mo["uv"]), t
        assert torch.equal(m.depth.cpu(), mo["depth"])
        torch.testing.assert_close(m.sigma_dd.cpu(), mo["sigma_dd"], rtol=1e-5, atol=0)
        torch.testing.assert_close(m.pos_Tc.cpu(), mo["pos_Tc"], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(m.pos_Tw.cpu(), mo["pos_Tw"], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(m.cov_Tc.cpu(), mo["cov_Tc"], rtol=2e-4, atol=1e-7)
        assert torch.equal(m.color.cpu(), mo["color"])
        hot.pose = ro["pose"].to(gpu)


@pytest.mark.parametrize("graph,selector,mapping", [c + (False,) for c in CONFIGS] + [("disp", "nodepth", True)])
def test_native_step_equals_python_step(gpu, graph, selector, mapping):
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath

    cam, frames, _ = _sequence(21, image=mapping)
    ins = _inputs(frames, gpu)
    kw = dict(graph_type=graph, selector=selector, **(MAPPING if mapping else {}))
    py = HotPath(Camera(**cam), HotPathConfig(**kw), gpu, keep_extras=True)
    nat = NativeHotPath(Camera(**cam), HotPathConfig(**kw), gpu, keep_extras=True)
    py.initialize(ins[0])
    nat.initialize(ins[0])
    for t in range(1, N_FRAMES):
        torch.manual_seed(300 + t)
        a = py.step(ins[t])
        torch.manual_seed(300 + t)
        b = nat.step(ins[t])
        torch.cuda.synchronize()
        assert torch.equal(py.last_tokens, nat.last_tokens)
        ma, mb = py.maps_prev_for_next, nat.maps()
        for f in ("depth", "depth_cov", "disparity", "disparity_cov", "flow", "flow_cov"):
            assert torch.equal(getattr(ma, f), getattr(mb, f)), f
        assert torch.equal(a.kp0_uv, b.kp0_uv), t
        assert torch.equal(a.n_valid, b.n_valid) and int(b.n_valid.item()) >= 150
        for k in ("cov0", "cov0_w", "cov1", "valid", "pos_Tw"):
            assert torch.equal(a.extras[k], b.extras[k]), k
        for f in ("kp0_uv", "kp1_uv", "inbound", "vals", "sigma0", "sigma1"):
            assert torch.equal(getattr(a.extras["tracked"], f), getattr(b.extras["tracked"], f)), f
        assert torch.equal(a.pose_f64, b.pose_f64) and torch.equal(a.info, b.info)
        assert torch.equal(a.pose, b.pose), t
        if mapping:
            assert a.map_points is not None and b.map_points is not None and b.map_points.uv.shape[0] == 300
            for f in ("uv", "depth", "sigma_dd", "pos_Tc", "pos_Tw", "cov_Tc", "color"):
                assert torch.equal(getattr(a.map_points, f), getattr(b.map_points, f)), (t, f)
    nat.close()


def test_two_lanes_with_device_maps_equal_solo_runs_and_the_oracle_map(gpu):
    from macvo_amd.devmap import DeviceVisualMap, DeviceVisualMaps
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath, stack_lanes
    from oracle import visual_map as VM
    from tests.test_gpu_map_lanes import _same

    lanes, seeds = 2, (5, 12)
    seqs = [_sequence(s) for s in (31, 44)]
    cam = seqs[0][0]
    time0 = (1_000_000, 2_000_000)
    ins = [_inputs(seqs[l][1], gpu, time0=time0[l]) for l in range(lanes)]
    K = torch.tensor([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1.0]])
    T_BS = torch.tensor([[0.05, 0.0, -0.1, 0, 0, 0, 1.0], [0.0, 0.2, 0.0, 0, 0, 0, 1.0]])
    starts = torch.tensor([[3.0, -2.0, 1.0, 0, 0, 0, 1.0], [0.0, 0.0, 0.0, 0, 0, 0, 1.0]])
    cfg = HotPathConfig(graph_type="disp")
    gens = lambda ss: [torch.Generator().manual_seed(int(s)) for s in ss]  # noqa: E731
    hot = NativeHotPath(Camera(**cam), cfg, gpu, lanes=lanes, generators=gens(seeds), keep_extras=True)
    mps = DeviceVisualMaps(lanes, gpu, init_size=16)
    hot.attach_maps(mps, K, T_BS)
    batched = [stack_lanes([ins[l][t] for l in range(lanes)]) for t in range(N_FRAMES)]
    hot.initialize(batched[0], init_pose=starts)
    ora = VM.OracleVisualMap()
    meta = dict(K=K, T_BS=T_BS[0], baseline=cam["baseline"])
    ora.push_frame(meta, dict(n=0, time_ns=time0[0], prior=starts[0]))
    prior = starts[0].clone()
    c = lambda x: x.cpu().clone()  # noqa: E731
    for t, res in enumerate(hot.run(batched[1:]), start=1):
        hot.sync_pose()
        torch.cuda.synchronize()
        r = res[0]
        ex, tr = r.extras, r.extras["tracked"]
        assert r.n_sel > 0
        fr = dict(n=r.n_sel, valid=c(ex["valid"]), kp0=c(tr.kp0_uv), kp1=c(tr.kp1_uv), vals=c(tr.vals), sigma0=c(tr.sigma0), sigma1=c(tr.sigma1),
                  cov0=c(ex["cov0"]), cov1=c(ex["cov1"]), pos_Tw=c(ex["pos_Tw"]), cov0w=c(ex["cov0_w"]), color=None, time_ns=time0[0] + 33 * t, prior=prior.clone())
        idx = ora.push_frame(meta, fr)
        prior = c(r.pose)
        ora.set_pose(idx, prior)
    hot.sync_all()
    torch.cuda.synchronize()
    got = mps.serialize()
    got_poses = [m.poses_array() for m in mps]
    hot.close()
    _same(got[0], ora.serialize(), "lane 0 vs the oracle map")
    Kn = K.numpy()
    for l in range(lanes):
        solo = NativeHotPath(Camera(**cam), cfg, gpu, generators=gens([seeds[l]]))
        sm = DeviceVisualMap(gpu, init_size=16)
        solo.attach_map(sm, K, T_BS[l])
        solo.initialize(ins[l][0], init_pose=starts[l])
        for _ in solo.run(ins[l][1:]):
            pass
        solo.sync_all()
        torch.cuda.synchronize()
        _same(got[l], sm.serialize(), f"lane {l} vs its solo run")
        assert np.array_equal(got_poses[l], sm.poses_array()), l
        solo.close()
        # ... and the Python-sequenced loop on the lane's frames and generator leaves the same poses (a lane and its solo run share the driver's wiring)
        py = HotPath(Camera(**cam), cfg, gpu, generator=gens([seeds[l]])[0])
        py.initialize(ins[l][0], init_pose=starts[l].to(gpu))
        py_poses = torch.stack([py.step(ins[l][t]).pose.clone() for t in range(1, N_FRAMES)])
        torch.cuda.synchronize()
        assert np.array_equal(got[l]["frames//pose"][1:], py_poses.cpu().numpy()), l
        # the camera, bit for bit, in every frame row
        assert got[l]["frames//K"].dtype == np.float32 and got[l]["frames//K"].shape == (N_FRAMES, 3, 3)
        assert all(np.array_equal(got[l]["frames//K"][t], Kn) for t in range(N_FRAMES)), l
        assert got[l]["frames//K"][0, 0, 0] == np.float32(150.0) and got[l]["frames//K"][0, 1, 1] == np.float32(190.0)
        assert np.array_equal(got[l]["frames//baseline"].reshape(-1), np.full(N_FRAMES, np.float32(cam["baseline"]), dtype=np.float32)), l
        assert got[l]["frames//need_interp"].tolist() == [False] * N_FRAMES
        assert got[l]["match//pixel1_uv"].shape[0] > 100
    assert not np.array_equal(got[0]["match//pixel1_uv"][:50], got[1]["match//pixel1_uv"][:50])


def test_native_motion_prior_equals_python_loop(gpu):
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath
    from tests.test_gpu_motion_native import _bits, _Net

    cam, frames, _ = _sequence(21)
    ins = _inputs(frames, gpu)
    cfg = HotPathConfig(graph_type="disp", motion_model="tartan")
    na, nb = _Net(gpu), _Net(gpu)
    py = HotPath(Camera(**cam), cfg, gpu, pose_net=na)
    nat = NativeHotPath(Camera(**cam), cfg, gpu, pose_net=nb)
    py.initialize(ins[0])
    nat.initialize(ins[0])
    start = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=gpu)
    for t in range(1, N_FRAMES):
        torch.manual_seed(300 + t)
        a = py.step(ins[t])
        torch.manual_seed(300 + t)
        b = nat.step(ins[t])
        torch.cuda.synchronize()
        assert torch.equal(_bits(na.inputs[-1]), _bits(nb.inputs[-1])), t
        assert torch.equal(a.kp0_uv, b.kp0_uv), t
        assert torch.equal(_bits(a.prior), _bits(b.prior)), t
        assert torch.equal(a.pose_f64, b.pose_f64) and torch.equal(a.info, b.info), t
        assert torch.equal(_bits(a.pose), _bits(b.pose)), t
        assert int(b.info[0, 1].item()) > 0, t
    assert (b.pose - start).abs().max() > 1e-3
    nat.close()
