"""GPU: the keypoint door of the native frame driver (ABI 8).

* Explicit keypoints reproduce the driver's own run: a `nodepth` pipe's recorded MV_FB_KP0 rows, fed to a second pipe through
  mv_frame_pipe_finish_keypoints (host) / _dev (device), give bit-identical backend tables and poses — nothing behind the keypoint row changed.
* selector "random" / "grid": HotPath and NativeHotPath in every finish mode (torch generators, host-seeded, drawn inside the front launch) select
  torch.randint's rows and agree on the poses as tests/test_gpu_native.py / tests/test_gpu_motion_native.py compare the same pairs of paths
  (bit-identical); each of two lanes equals its solo run.
* The Vanilla and CovOpt ablation combinations and a grid case against OracleHotPath with its selector call substituted by tests/selectors_ref.py."""
import pytest
import torch

from tests import cov_models_ref as R
from tests import selectors_ref as SR
from tests import synth

pytestmark = pytest.mark.gpu

TABLES = (("KP0", torch.int64, (2,)), ("KP0F", torch.float32, (2,)), ("KP1", torch.float32, (2,)), ("INBOUND", torch.uint8, ()),
          ("SIGMA0", torch.float32, (3,)), ("SIGMA1", torch.float32, (3,)), ("POS_TC", torch.float32, (3,)), ("POS_TW", torch.float32, (3,)),
          ("COV0", torch.float64, (3, 3)), ("COV0W", torch.float64, (3, 3)), ("COV1", torch.float64, (3, 3)), ("VALID", torch.uint8, ()))


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype in (torch.float32, torch.float64) else t


class _Net:
    """Seeded stand-in PoseNet, lane by lane (the one tests/test_gpu_motion_native.py uses)."""

    def __init__(self, dev, seed=7):
        g = torch.Generator().manual_seed(seed)
        self.A = (torch.randn(6, 5, generator=g) * 0.5).to(dev)
        self.b = (torch.randn(6, generator=g) * 0.3).to(dev)

    def __call__(self, x):
        return torch.cat([torch.tanh(x[l:l + 1].clamp(-1e3, 1e3).mean(dim=(2, 3))) @ self.A.T + self.b for l in range(x.shape[0])])


def _ins(frames, dev):
    from macvo_amd.pipeline import FrameInputs

    out = [FrameInputs(**{k: (None if v is None else v.to(dev)) for k, v in fr.items()}) for fr in frames]
    torch.cuda.synchronize()
    return out


def _lane_frames(lanes, n_frames, seed0, H=192, W=256):
    seqs = [synth.make_sequence(n_frames, H, W, C=64, iters=2, seed=seed0 + 13 * l) for l in range(lanes)]
    return seqs[0][0], [s[1] for s in seqs]


def _snapshot(hot, results):
    """Live rows of every backend table + per-lane scalars of the newest finished frame, cloned."""
    rs = results if isinstance(results, list) else [results]
    snap = []
    for r in rs:
        d = {name: r._rows(name, dt, tail).clone() for name, dt, tail in TABLES}
        n = r.n_sel
        d["VALS"] = hot._view("VALS", r._age(), torch.float32, (11, hot.lanes, hot._cap))[:, r.lane, :n].clone()
        d["pose"], d["n_sel"] = r.pose.clone(), n
        d["pose64"] = None if r.pose_f64 is None else r.pose_f64.clone()
        d["info"] = None if r.info is None else r.info.clone()
        d["n_valid"] = None if r.n_valid is None else r.n_valid.clone()
        d["prior"] = None if r.prior is None else r.prior.clone()
        d["map_uv"] = None if r.map_points is None else r.map_points.uv.clone()
        d["map_Tw"] = None if r.map_points is None else r.map_points.pos_Tw.clone()
        d["map_cov"] = None if r.map_points is None else r.map_points.cov_Tc.clone()
        snap.append(d)
    return snap


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for la, lb in zip(a, b):
        assert la.keys() == lb.keys()
        for k in la:
            x, y = la[k], lb[k]
            if isinstance(x, torch.Tensor):
                assert y is not None and x.shape == y.shape and torch.equal(_bits(x), _bits(y)), (what, k)
            else:
                assert x == y, (what, k)


@pytest.mark.parametrize("lanes,motion,mapping", [(1, "static", False), (2, "static", False), (1, "tartan", False), (2, "tartan", False),
                                                  (1, "static", True), (1, "tartan", True)])
def test_explicit_keypoints_reproduce_the_drivers_own_run(gpu, lanes, motion, mapping):
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath, stack_lanes

    n_frames = 5
    cam, per_lane = _lane_frames(lanes, n_frames, 31)
    ins = [_ins(fr, gpu) for fr in per_lane]
    stacked = [stack_lanes([ins[l][t] for l in range(lanes)]) for t in range(n_frames)]
    kw = dict(graph_type="icp", motion_model=motion, mapping=mapping)
    if mapping:
        kw.update(map_max_depth=13.0, map_max_depth_cov=0.5, map_num_point=500)
    net = (lambda: _Net(gpu)) if motion == "tartan" else (lambda: None)
    gens = lambda: [torch.Generator().manual_seed(5 + 7 * l) for l in range(lanes)]  # noqa: E731

    ref = NativeHotPath(Camera(**cam), HotPathConfig(selector="nodepth", **kw), gpu, lanes=lanes, generators=gens(), pose_net=net())
    ref.initialize(stacked[0])
    want, gen_before, n_cand = [], [], []
    for t in range(1, n_frames):
        gen_before.append(ref.generators[0].get_state())
        res = ref.step(stacked[t])
        torch.cuda.synchronize()
        want.append(_snapshot(ref, res))
        n_cand.append((res if lanes == 1 else res[0]).n_cand)
    ref.close()
    assert all(s["n_sel"] > 0 for fr in want for s in fr) and (not mapping or any(s["map_uv"] is not None for fr in want for s in fr))

    variants = [("explicit", "host"), ("nodepth", "host")] + ([] if mapping else [("explicit", "device"), ("nodepth", "device")])
    for selector, where in variants:
        hot = NativeHotPath(Camera(**cam), HotPathConfig(selector=selector, **kw), gpu, lanes=lanes, generators=gens(), pose_net=net())
        hot.initialize(stacked[0])
        for t in range(1, n_frames):
            cap = max(s["n_sel"] for s in want[t - 1])
            kp = torch.zeros((lanes, cap, 2), dtype=torch.int64)
            for l, s in enumerate(want[t - 1]):
                kp[l, : s["n_sel"]] = s["KP0"].cpu()
            x = stacked[t]
            x.keypoints = kp.to(gpu) if where == "device" else kp
            x.keypoint_counts = [s["n_sel"] for s in want[t - 1]]
            if mapping:   # the tail's permutation is drawn from the same generator BEHIND the frame's keypoint permutation: put the generator where the
                hot.generators[0].set_state(gen_before[t - 1])         # first pipe's tail found it (explicit keypoints draw nothing)
                torch.randperm(n_cand[t - 1], generator=hot.generators[0])
            res = hot.step(x)
            torch.cuda.synchronize()
            got = _snapshot(hot, res)
            x.keypoints = x.keypoint_counts = None
            _assert_same(got, want[t - 1], (selector, where, lanes, motion, mapping, t))
        hot.close()


def _run_native(cam, cfg, gpu, lanes, generators, stacked, net=None):
    """Pipelined run(): per frame the lanes' keypoints, poses and priors (cloned)."""
    from macvo_amd.pipeline import Camera, NativeHotPath

    hot = NativeHotPath(Camera(**cam), cfg, gpu, lanes=lanes, generators=generators, pose_net=net)
    hot.initialize(stacked[0])
    out = []
    for res in hot.run(stacked[1:]):
        rs = res if isinstance(res, list) else [res]
        hot.sync_pose()
        out.append([(r.kp0_uv.clone(), r.pose.clone(), None if r.prior is None else r.prior.clone()) for r in rs])
    torch.cuda.synchronize()
    dd = hot.device_driven
    hot.close()
    return out, dd


@pytest.mark.parametrize("motion", ["static", "tartan"])
def test_random_selector_every_finish_mode_and_lanes(gpu, monkeypatch, motion):
    """selector "random": HotPath (torch.randint on the lane's CPU generator) and NativeHotPath with torch generators (finish_keypoints),
    host-seeded (finish_seeded) and device-drawn (finish_device, RandomSelector inside the front launch) — the same keypoints as torch.randint bit
    for bit, the same poses bit for bit (the pairs tests/test_gpu_native.py and tests/test_gpu_motion_native.py compare bit for bit), each of two
    lanes equal to its solo run.  The seed produces duplicate keypoints, which are kept."""
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, stack_lanes

    lanes, n_frames, H, W, mask = 2, 5, 192, 256, 32
    cam, per_lane = _lane_frames(lanes, n_frames, 31, H, W)
    ins = [_ins(fr, gpu) for fr in per_lane]
    stacked = [stack_lanes([ins[l][t] for l in range(lanes)]) for t in range(n_frames)]
    seeds = [5, 12]
    cfg = HotPathConfig(selector="random", kp_mask_width=mask, graph_type="icp", motion_model=motion)
    net = (lambda: _Net(gpu)) if motion == "tartan" else (lambda: None)
    # what torch.randint draws, lane by lane and frame by frame
    want_kp = []
    for s in seeds:
        g = torch.Generator().manual_seed(s)
        want_kp.append([SR.random_select(cfg.num_point, H, W, mask, g) for _ in range(1, n_frames)])
    dup = sum(int(k.shape[0] - torch.unique(k, dim=0).shape[0]) for lane in want_kp for k in lane)
    assert dup >= 1, "the chosen seeds must produce at least one duplicate keypoint"

    runs = {}
    for mode in ("host", "seeded", "device"):
        monkeypatch.setenv("MV_PIPE_DEVICE_DRAW", "0" if mode == "seeded" else "1")
        gens = [torch.Generator().manual_seed(s) for s in seeds] if mode == "host" else list(seeds)
        runs[mode], dd = _run_native(cam, cfg, gpu, lanes, gens, stacked, net())
        assert dd == (mode == "device")
        for l in range(lanes):
            solo, _ = _run_native(cam, cfg, gpu, 1, [torch.Generator().manual_seed(seeds[l]) if mode == "host" else seeds[l]], ins[l], net())
            for t in range(n_frames - 1):
                assert torch.equal(solo[t][0][0], runs[mode][t][l][0]), (mode, l, t)
                assert torch.equal(_bits(solo[t][0][1]), _bits(runs[mode][t][l][1])), (mode, l, t)
    for mode in runs:
        for t in range(n_frames - 1):
            for l in range(lanes):
                kp, pose, prior = runs[mode][t][l]
                assert torch.equal(kp.cpu(), want_kp[l][t]), (mode, l, t)
                assert torch.equal(_bits(pose), _bits(runs["host"][t][l][1])), (mode, l, t)
                if prior is not None:
                    assert torch.equal(_bits(prior), _bits(runs["host"][t][l][2])), (mode, l, t)
    # the Python loop, lane by lane (its own generator argument)
    for l in range(lanes):
        py = HotPath(Camera(**cam), cfg, gpu, pose_net=net(), generator=torch.Generator().manual_seed(seeds[l]))
        py.initialize(ins[l][0])
        for t in range(1, n_frames):
            a = py.step(ins[l][t])
            torch.cuda.synchronize()
            assert torch.equal(a.kp0_uv.cpu(), want_kp[l][t - 1]), (l, t)
            assert torch.equal(_bits(a.pose), _bits(runs["host"][t - 1][l][1])), (l, t)
    assert (runs["host"][-1][0][1] - torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=gpu)).abs().max() > 1e-3


def test_random_selector_global_generator_and_mapping_tail(gpu):
    """Torch's global CPU generator, as the reference consumes it, with the dense-mapping tail: the frame's MappingPointSelector permutation is drawn
    after its keypoints from the same generator (MACVO.py:197 before :315) — native equals the Python loop bit for bit, map points included."""
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath

    H, W, n_frames = 240, 320, 4
    cam, frames, _ = synth.make_sequence(n_frames, H, W, C=64, iters=1, seed=23)
    cfg = HotPathConfig(selector="random", mapping=True, map_max_depth=13.0, map_max_depth_cov=0.5, map_num_point=500, graph_type="icp")
    py, nat = HotPath(Camera(**cam), cfg, gpu), NativeHotPath(Camera(**cam), cfg, gpu)
    ins = _ins(frames, gpu)
    py.initialize(ins[0])
    nat.initialize(ins[0])
    seen = 0
    for t in range(1, n_frames):
        torch.manual_seed(70 + t)
        a = py.step(ins[t])
        torch.manual_seed(70 + t)
        b = nat.step(ins[t])
        torch.cuda.synchronize()
        torch.manual_seed(70 + t)
        assert torch.equal(b.kp0_uv.cpu(), SR.random_select(cfg.num_point, H, W, cfg.kp_mask_width)), t
        assert torch.equal(a.kp0_uv, b.kp0_uv) and torch.equal(_bits(a.pose), _bits(b.pose)), t
        ma, mb = a.map_points, b.map_points
        assert (ma is None) == (mb is None), t
        if mb is not None:
            assert torch.equal(ma.uv, mb.uv) and torch.equal(_bits(ma.pos_Tw), _bits(mb.pos_Tw)) and torch.equal(_bits(ma.cov_Tc), _bits(mb.cov_Tc)), t
            seen += mb.uv.shape[0]
    assert seen > 0
    nat.close()
    with pytest.raises(Exception):      # integer seeds and mapping=True still do not combine
        NativeHotPath(Camera(**cam), cfg, gpu, generators=[3])


def test_grid_selector_231_rows_flow_through_tables_solve_and_map(gpu):
    """selector "grid" at 640 x 480 / 32 / 200: 231 rows (more than num_point) through the backend tables, the solve and map_append; native
    (both finish spellings) equals the Python loop bit for bit."""
    from macvo_amd import devmap
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath

    H, W, n_frames = 480, 640, 4
    cam, frames, _ = synth.make_sequence(n_frames, H, W, C=64, iters=2, seed=21)
    cfg = HotPathConfig(selector="grid", graph_type="icp")
    ins = _ins(frames, gpu)
    want = torch.as_tensor(SR.grid_select(200, H, W, 32))
    assert want.shape[0] == 231
    py = HotPath(Camera(**cam), cfg, gpu, keep_extras=True)
    nat = NativeHotPath(Camera(**cam), cfg, gpu, keep_extras=True)
    seeded = NativeHotPath(Camera(**cam), cfg, gpu, generators=[4])
    assert nat._cap == 231
    K = torch.tensor([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1.0]])
    dm = devmap.DeviceVisualMap(gpu)
    nat.attach_map(dm, K)
    for hp in (py, nat, seeded):
        hp.initialize(ins[0])
    for t in range(1, n_frames):
        a, b, c = py.step(ins[t]), nat.step(ins[t]), seeded.step(ins[t])
        torch.cuda.synchronize()
        assert b.n_sel == 231 and torch.equal(b.kp0_uv.cpu(), want) and torch.equal(a.kp0_uv.cpu(), want) and torch.equal(c.kp0_uv.cpu(), want)
        for k in ("cov0", "cov0_w", "cov1", "valid", "pos_Tw"):
            assert torch.equal(a.extras[k], b.extras[k]), (k, t)
        for f in ("kp0_uv", "kp1_uv", "inbound", "vals", "sigma0", "sigma1"):
            assert torch.equal(getattr(a.extras["tracked"], f), getattr(b.extras["tracked"], f)), (f, t)
        assert torch.equal(a.n_valid, b.n_valid) and int(b.n_valid.item()) > 0
        assert torch.equal(a.pose_f64, b.pose_f64) and torch.equal(a.info, b.info) and torch.equal(_bits(a.pose), _bits(b.pose)), t
        assert torch.equal(_bits(c.pose), _bits(b.pose)), t
    nat.synchronize()
    torch.cuda.synchronize()
    assert dm.n_frames == n_frames and dm.rows_upper == 231 * (n_frames - 1)      # every frame's 231 rows were handed to mv_map_append
    nat.close()
    seeded.close()


def _oracle_with(monkeypatch, cam, ocfg, select, cov_model, filters_flags, fmin, fmax):
    """OracleHotPath with its selector call substituted by `select` (tests/selectors_ref.py), its covariance call by the CPU restatement of the
    covariance model (tests/cov_models_ref.py, as tests/test_gpu_cov_models.py does) and its filter by the composition of the oracle's own filters."""
    from oracle import filters as OF
    from oracle import pipeline as opl
    from oracle.pipeline import OracleHotPath

    ora = OracleHotPath(cam, ocfg)
    monkeypatch.setattr(opl.selector, "cov_aware_selector_nodepth", lambda *a, **k: (select(), None, None))
    if cov_model == "none":
        monkeypatch.setattr(opl.covariance, "match_covariance", lambda kp, *a, **k: R.no_covariance(kp.shape[0]))
    seen = {}
    track, sanity = opl.frontend.track_keypoints, OF.covariance_sanity      # (the originals: both names are substituted below)

    def rec_track(*a, **k):
        seen["tr"] = track(*a, **k)
        return seen["tr"]

    def filt(cov0, cov1):
        tr = seen["tr"]
        ok = torch.ones(cov0.shape[0], dtype=torch.bool)
        if filters_flags & 1:
            ok &= sanity(cov0, cov1)
        if filters_flags & 2:
            ok &= OF.simple_depth(tr["kp0_d"].reshape(-1, 1), tr["kp1_d"].reshape(-1, 1), fmin, fmax)
        if filters_flags & 4:
            ok &= OF.likely_front_of_cam(tr["kp0_d"].reshape(-1, 1), tr["kp0_sigma_dd"].reshape(-1, 1), tr["kp1_d"].reshape(-1, 1),
                                         tr["kp1_sigma_dd"].reshape(-1, 1))
        return ok
    monkeypatch.setattr(opl.frontend, "track_keypoints", rec_track)
    monkeypatch.setattr(opl.filters, "covariance_sanity", filt)
    return ora


@pytest.mark.parametrize("name", ["vanilla", "covopt", "grid"])
def test_sequence_matches_oracle_with_mapless_selectors(gpu, monkeypatch, name):
    """Vanilla (RandomSelector + NoCovariance + SimpleDepthFilter + icp), CovOpt (RandomSelector, mask 32 + MatchCovariance + all three filters + icp)
    and a GridSelector case over 5 frames: keypoints bit-exact, poses within the 1e-4 of test_sequence_matches_oracle at the same step count."""
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath
    from oracle import se3

    n_frames, H, W = 5, 192, 256
    cam, frames, _ = synth.make_sequence(n_frames, H, W, C=64, iters=3, seed=3)
    all3 = ops.FILTER_COV_SANITY | ops.FILTER_SIMPLE_DEPTH | ops.FILTER_FRONT_OF_CAM
    selector, cov_model, flags = {"vanilla": ("random", "none", ops.FILTER_SIMPLE_DEPTH), "covopt": ("random", "match", all3),
                                  "grid": ("grid", "match", ops.FILTER_COV_SANITY)}[name]
    cfg = HotPathConfig(selector=selector, kp_mask_width=32, cov_model=cov_model, filters=flags, graph_type="icp")
    max_depth = cam["fx"] * cam["baseline"]
    select = (lambda: SR.random_select(cfg.num_point, H, W, 32)) if selector == "random" else (lambda: SR.grid_select(cfg.num_point, H, W, 32))
    ora = _oracle_with(monkeypatch, cam, dict(graph_type="icp"), select, cov_model, flags, cfg.filter_min_depth, max_depth)
    hot = HotPath(Camera(**cam), cfg, gpu)
    nat = NativeHotPath(Camera(**cam), cfg, gpu)
    ins = _ins(frames, gpu)
    ora.initialize(frames[0])
    hot.initialize(ins[0])
    nat.initialize(ins[0])
    for t in range(1, n_frames):
        torch.manual_seed(100 + t)
        ro = ora.step(frames[t])
        torch.manual_seed(100 + t)
        rh = hot.step(ins[t])
        torch.manual_seed(100 + t)
        rn = nat.step(ins[t])
        torch.cuda.synchronize()
        assert torch.equal(rh.kp0_uv.cpu(), ro["kp0_uv"]) and torch.equal(rn.kp0_uv.cpu(), ro["kp0_uv"]), t
        assert int(rh.n_valid.item()) == ro["n_valid"] == int(rn.n_valid.item()), t
        for r in (rh, rn):
            dt, dr = se3.pose_error(ro["pose"].double(), r.pose.cpu().double())
            assert dt <= 1e-4 and dr <= 1e-4, (name, t, dt, dr)
        assert int(rh.info[0, 1].item()) == ro["steps"], t
    nat.close()


def test_keypoint_door_argument_checks(gpu):
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath

    cam, frames, _ = synth.make_sequence(3, 192, 256, C=64, iters=1, seed=4)
    ins = _ins(frames, gpu)
    with pytest.raises(ValueError, match="covariance patch"):
        NativeHotPath(Camera(**cam), HotPathConfig(selector="explicit", kp_mask_width=8), gpu)
    hot = NativeHotPath(Camera(**cam), HotPathConfig(selector="explicit"), gpu)
    hot.initialize(ins[0])
    ok = torch.tensor([[40, 40], [100, 90], [40, 40]])
    r = hot.step(ins[1], keypoints=ok)
    torch.cuda.synchronize()
    assert r.n_sel == 3 and torch.equal(r.kp0_uv.cpu(), ok)
    hot.enqueue_frontend(ins[2])
    with pytest.raises(ValueError):                      # no keypoints for an explicit frame
        hot.finish()
    hot._kps[0] = (torch.tensor([[5, 40]]), None)        # a patch that leaves the image
    with pytest.raises(ValueError, match="inside"):
        hot.finish()
    # ... and the C entry point itself refuses it
    bad = torch.tensor([[[5, 40]]], dtype=torch.int64)
    nsel = (ops.C.c_int32 * 1)(1)
    assert hot._lib.mv_frame_pipe_finish_keypoints(hot._pipe, bad.data_ptr(), nsel, None) == -1
    hot._kps[0] = (ok, None)
    r = hot.finish()
    torch.cuda.synchronize()
    assert r.n_sel == 3
    # a permutation needs a candidate list
    perm = torch.zeros(4, dtype=torch.int64)
    hot.enqueue_frontend(ins[1])
    assert hot._lib.mv_frame_pipe_finish(hot._pipe, perm.data_ptr(), nsel, None) == -1
    hot._kps[0] = (ok, None)
    hot.finish()
    hot.close()
