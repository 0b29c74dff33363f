"""GPU: mv_obs_cov (GaussianMixtureCovariance, NoCovariance, modifier chains) against the reference's golden, bitwise against
mv_match_cov / its own pair-lanes form, the plugins, and the frame driver's three covariance paths against the per-call ABI."""
import os

import numpy as np
import pytest
import torch

from tests import cov_models_ref as R
from tests import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cov_models.npz")
EPS32 = 2.0 ** -23


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    z = np.load(GOLD)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _gmm_check(cov, ref, stats, g, kp, fc_clamped):
    """fp32 mixture variance = E[c + z^2] - mean^2 cancels: bar = c * eps32 * sum p (c + z^2) per row; rows whose fp64 weights sit
    within 1e-6 (relative) of the threshold may flip and are exempt."""
    K = tuple(float(x) for x in g["K"])
    w = g["gmm_weights"].double()
    near = ((w / 1e-3 - 1).abs() < 1e-6).any(dim=1)
    assert int(near.sum()) <= 2
    n = kp.shape[0]
    kl = kp.long()
    off = torch.arange(-15, 16)
    uu, vv = torch.meshgrid(off, off, indexing="ij")
    au, av = kl[:, 0:1] + uu.reshape(1, -1), kl[:, 1:2] + vv.reshape(1, -1)
    z = g["depth"][..., av, au].view(n, 31, 31).permute(0, 2, 1).flatten(1).double()
    c = g["dcov"][..., av, au].view(n, 31, 31).permute(0, 2, 1).flatten(1).double()
    p = w.clone()
    p[p < 1e-3] = 0
    p = p / p.sum(1, keepdim=True)
    e2 = ((c + z * z) * p).sum(1)
    bar = 64 * EPS32 * e2
    ok = ~near
    var_ref = ref[:, 0, 0]
    assert ((stats[:, 1].double() - var_ref).abs()[ok] <= bar[ok]).all()
    assert torch.equal(cov[:, 0, 0], stats[:, 1].double())
    mean_ref = (z * p).sum(1)
    torch.testing.assert_close(stats[ok, 0].double(), mean_ref[ok], rtol=1e-5, atol=0)


def test_obs_cov_gmm_none_modifiers_vs_golden(gpu, g):
    from macvo_amd import ops

    K = tuple(float(x) for x in g["K"])
    d, dc = g["depth"].to(gpu), g["dcov"].to(gpu)
    for kp in (g["kp_int"], g["kp_float"]):
        fc = g["flow_cov_in"].clone().to(gpu)
        cov, st = ops.obs_cov("gmm", d, kp.to(gpu), fc, None, *K, depth_cov_map=dc, want_stats=True)
        ref = g["gmm_int_flowcov"] if kp.dtype == torch.int64 else g["gmm_float_flowcov"]
        assert torch.equal(fc.cpu(), g["gmm_flow_cov_after"])                        # the in-place clamp, bitwise
        _gmm_check(cov.cpu(), ref, st.cpu(), g, kp, fc.cpu())
        torch.testing.assert_close(cov.cpu()[:, 1:, 1:], ref[:, 1:, 1:], rtol=2e-3, atol=1e-6)
    # a NaN match covariance gives a NaN row (the reference propagates it the same way) and leaves every other row's bits alone
    fcn = g["flow_cov_in"].clone()
    fcn[7, 0] = float("nan")
    base = ops.obs_cov("gmm", d, g["kp_float"].to(gpu), g["flow_cov_in"].clone().to(gpu), None, *K, depth_cov_map=dc).cpu()
    nan = ops.obs_cov("gmm", d, g["kp_float"].to(gpu), fcn.to(gpu), None, *K, depth_cov_map=dc).cpu()
    keep = torch.arange(48) != 7
    assert torch.isnan(nan[7]).all() and torch.equal(nan[keep], base[keep])
    # flow_cov absent + depth_cov given -> var = depth_cov (the plugin's handling, constant sigma, no clamp)
    s0 = torch.full((48, 3), 0.25, device=gpu)
    s0[:, 2] = 0
    cov = ops.obs_cov("gmm", d, g["kp_int"].to(gpu), s0, g["depth_cov_kp"].to(gpu), *K, depth_cov_map=dc, min_flow_cov=0.0,
                      use_patch_var=False)
    torch.testing.assert_close(cov.cpu(), g["gmm_int_nodefault"], rtol=2e-4, atol=1e-7)
    # NoCovariance: identity, flow_cov untouched
    fc = g["flow_cov_in"].clone().to(gpu)
    assert torch.equal(ops.obs_cov("none", d, g["kp_float"].to(gpu), fc, None, *K).cpu(), g["none"])
    assert torch.equal(fc.cpu(), g["flow_cov_in"])
    # modifier chains on MatchCovariance, and Diag(GMM)
    for key, chain in (("diag_match", ("diag",)), ("norm_match", ("normalize",)), ("norm_diag_match", ("diag", "normalize")),
                       ("diag_norm_match", ("normalize", "diag"))):
        cov = ops.obs_cov("match", d, g["kp_float"].to(gpu), g["flow_cov_in"].clone().to(gpu), None, *K, modifiers=chain).cpu()
        torch.testing.assert_close(cov, g[key], rtol=1e-3, atol=0, msg=key)
        base = ops.obs_cov("match", d, g["kp_float"].to(gpu), g["flow_cov_in"].clone().to(gpu), None, *K).cpu()
        torch.testing.assert_close(cov, R.apply_chain(base, chain), rtol=1e-12, atol=0, msg=key)
    cov = ops.obs_cov("gmm", d, g["kp_float"].to(gpu), g["flow_cov_in"].clone().to(gpu), None, *K, depth_cov_map=dc, modifiers=("diag",))
    assert (cov.cpu()[:, [0, 0, 1, 1, 2, 2], [1, 2, 0, 2, 0, 1]] == 0).all()


def test_obs_cov_match_is_match_cov_and_pair_lanes_equal_singles(gpu, g):
    from macvo_amd import ops

    K = tuple(float(x) for x in g["K"])
    d, dc = g["depth"].to(gpu), g["dcov"].to(gpu)
    kp = g["kp_float"].to(gpu)
    rot = torch.tensor([[0.6, -0.8, 0.0], [0.8, 0.6, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64, device=gpu)
    f1, f2 = g["flow_cov_in"].clone().to(gpu), g["flow_cov_in"].clone().to(gpu)
    a = ops.match_cov(d, kp, f1, None, *K, rot=rot, want_stats=True)
    b = ops.obs_cov("match", d, kp, f2, None, *K, rot=rot, want_stats=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(f1, f2)
    # two lanes, different depth maps and ragged live rows
    d2, dc2 = synth.depth_maps(120, 160, 9)
    D = torch.cat([g["depth"], d2]).reshape(2, 120, 160).to(gpu).contiguous()
    DC = torch.cat([g["dcov"], dc2]).reshape(2, 120, 160).to(gpu).contiguous()
    KP = torch.stack([g["kp_float"], g["kp_float"].flip(0)]).to(gpu).contiguous()
    R2 = torch.stack([rot, rot.t().contiguous()]).contiguous()
    live = [48, 31]
    for model, mods in (("gmm", ()), ("none", ()), ("match", ("diag", "normalize")), ("gmm", ("normalize",))):
        S0 = torch.stack([g["flow_cov_in"], g["flow_cov_in"].flip(0)]).to(gpu).contiguous()
        S1 = (S0 * 1.5).contiguous()
        s0c, s1c = S0.clone(), S1.clone()
        c0, c0w, c1 = ops.obs_cov_pair(model, D, KP, S0, D.flip(0).contiguous(), KP, S1, *K, depth_cov_map0=DC,
                                       depth_cov_map1=DC.flip(0).contiguous(), modifiers=mods, rot=R2, n_live=live)
        for l in range(2):
            n = live[l]
            a0, a0w = ops.obs_cov(model, D[l], KP[l, :n], s0c[l, :n].contiguous(), None, *K, depth_cov_map=DC[l], modifiers=mods, rot=R2[l])
            a1 = ops.obs_cov(model, D.flip(0)[l].contiguous(), KP[l, :n], s1c[l, :n].contiguous(), None, *K, depth_cov_map=DC.flip(0)[l].contiguous(),
                             modifiers=mods)
            for x, y in ((c0[l, :n], a0), (c0w[l, :n], a0w), (c1[l, :n], a1)):
                assert torch.equal(torch.nan_to_num(x, 7.0), torch.nan_to_num(y, 7.0)), (model, mods, l)


def test_plugins_nested_modifiers_and_no_covariance(gpu, g):
    from types import SimpleNamespace as NS

    from macvo_amd import plugins as P
    from macvo_amd.interfaces import ICovariance2to3

    K = tuple(float(x) for x in g["K"])
    frame = NS(fx=K[0], fy=K[1], cx=K[2], cy=K[3])
    dest = NS(depth=g["depth"].to(gpu), cov=g["dcov"].to(gpu))
    args = NS(kernel_size=31, match_cov_default=0.25, min_flow_cov=0.25, min_depth_cov=0.05, device="cuda")
    base = P.HIP_MatchCovariance(args).estimate(frame, g["kp_float"], dest, None, g["flow_cov_in"].clone())
    cfg = NS(type="HIP_Modifier_Normalize", args=NS(type="HIP_Modifier_Diagonalize", args=NS(type="HIP_MatchCovariance", args=args)))
    ICovariance2to3.is_valid_config(cfg)
    m = ICovariance2to3.instantiate(cfg.type, cfg.args)
    assert isinstance(m, P.HIP_Modifier_Normalize) and m._chain()[1] == ("diag", "normalize")
    out = m.estimate(frame, g["kp_float"], dest, None, g["flow_cov_in"].clone())
    assert out.device.type == "cpu" and out.dtype == torch.float64
    torch.testing.assert_close(out, R.apply_chain(base, ("diag", "normalize")), rtol=1e-12, atol=0)
    fc = g["flow_cov_in"].clone()
    eye = P.HIP_NoCovariance(None).estimate(frame, g["kp_float"], dest, None, fc)
    assert torch.equal(eye, g["none"]) and torch.equal(fc, g["flow_cov_in"])
    gm = P.HIP_GaussianMixtureCovariance(NS(kernel_size=31, match_cov_default=0.25, min_flow_cov=0.25, min_depth_cov=0.05))
    torch.testing.assert_close(gm.estimate(frame, g["kp_float"], dest, None, g["flow_cov_in"].clone())[:, 1:, 1:],
                               g["gmm_float_flowcov"][:, 1:, 1:], rtol=2e-3, atol=1e-6)


CHAINS = [("gmm", ()), ("none", ()), ("match", ("diag",)), ("match", ("diag", "normalize"))]
FB = {"KP0": (torch.int64, (2,)), "KP0F": (torch.float32, (2,)), "KP1": (torch.float32, (2,)), "SIGMA0": (torch.float32, (3,)),
      "SIGMA1": (torch.float32, (3,)), "COV0": (torch.float64, (3, 3)), "COV0W": (torch.float64, (3, 3)), "COV1": (torch.float64, (3, 3))}


def _inputs(frames, dev):
    from macvo_amd.pipeline import FrameInputs

    return [FrameInputs(**{k: (None if v is None else v.to(dev)) for k, v in fr.items()}) for fr in frames]


def _eq(x, y):
    return torch.equal(torch.nan_to_num(x, 7.0, 8.0, -8.0), torch.nan_to_num(y, 7.0, 8.0, -8.0))


@pytest.mark.parametrize("model,mods", CHAINS)
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("device_draw", ["0", "1"])
def test_frame_driver_tables_equal_obs_cov_on_its_own_keypoints(gpu, monkeypatch, model, mods, lanes, device_draw):
    """The frame driver's covariance tables (fused backend launch: device-drawn backend_front_kernel<2, .> or host-drawn <0|1, .>, 1 and 2
    lanes) are bit-identical to mv_obs_cov run on the driver's own keypoint tables and maps: COV0, COV0W (R = the driver's ROT), COV1, and
    SIGMA0 / SIGMA1 = the constant / match sigma, clamped by "match" / "gmm", untouched by "none"."""
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath, stack_lanes

    monkeypatch.setenv("MV_PIPE_DEVICE_DRAW", device_draw)
    n_frames = 4
    cam, frames, _ = synth.make_sequence(n_frames + lanes, 192, 256, C=32, iters=2, seed=11)
    ins = _inputs(frames, gpu)
    batches = ins if lanes == 1 else [stack_lanes([ins[(t + l) % len(ins)] for l in range(lanes)]) for t in range(n_frames)]
    cfg = HotPathConfig(num_point=60, graph_type="icp", cov_model=model, cov_modifiers=mods)
    hot = NativeHotPath(Camera(**cam), cfg, gpu, lanes=lanes, generators=[5 + 7 * l for l in range(lanes)])
    hot.initialize(batches[0])
    K = Camera(**cam).K4
    mcd = cfg.match_cov_default
    for t in range(1, n_frames):
        hot.enqueue_frontend(batches[t])
        res = hot.finish(None)
        assert hot.device_driven == (device_draw == "1")
        hot.sync_all()
        torch.cuda.synchronize()
        res = res if isinstance(res, list) else [res]
        cap = hot._cap
        v = {nm: hot._view(nm, 0, dt, (lanes, cap) + tail).clone() for nm, (dt, tail) in FB.items()}
        rot = hot._view("ROT", 0, torch.float64, (lanes, 9)).clone()
        for l in range(lanes):
            n = res[l].n_sel
            assert n > 0
            m0, m1 = hot.maps(1, l), hot.maps(0, l)             # frontend age 0 = the newest enqueued frame (this one)
            kp0 = v["KP0"][l, :n]
            s0 = torch.zeros(n, 3, device=gpu)
            s0[:, :2] = mcd
            mc = m1.flow_cov.reshape(3, -1)
            lin = kp0[:, 1] * cam["W"] + kp0[:, 0]
            s1 = mc[:, lin].t().contiguous()                    # the match sigma at the source pixel (MACVO.py:231)
            c0, c0w = ops.obs_cov(model, m0.depth, v["KP0F"][l, :n].contiguous(), s0, None, *K, depth_cov_map=m0.depth_cov, modifiers=mods,
                                  rot=rot[l].reshape(3, 3), kernel_size=cfg.cov_kernel_size, min_flow_cov=cfg.min_flow_cov,
                                  min_depth_cov=cfg.min_depth_cov)
            c1 = ops.obs_cov(model, m1.depth, v["KP1"][l, :n].contiguous(), s1, None, *K, depth_cov_map=m1.depth_cov, modifiers=mods,
                             kernel_size=cfg.cov_kernel_size, min_flow_cov=cfg.min_flow_cov, min_depth_cov=cfg.min_depth_cov)
            for nm, want in (("COV0", c0), ("COV0W", c0w), ("COV1", c1), ("SIGMA0", s0), ("SIGMA1", s1)):
                assert _eq(v[nm][l, :n], want), (model, mods, t, l, nm)
            if model == "none":
                assert torch.equal(v["SIGMA1"][l, :n], mc[:, lin].t())     # not clamped
            else:
                assert (v["SIGMA1"][l, :n, :2] >= cfg.min_flow_cov ** 2).all()
            if model == "gmm":                                  # the other lane's / the other frame's variance map would not do
                assert not _eq(c1, ops.obs_cov(model, m1.depth, v["KP1"][l, :n].contiguous(), s1.clone(), None, *K,
                                               depth_cov_map=(m0.depth_cov * 2).contiguous(), modifiers=mods))
    hot.close()


@pytest.mark.parametrize("model,mods", CHAINS)
def test_frame_driver_map_cov_equals_obs_cov(gpu, model, mods):
    """mapping = 1: MV_FB_MAP_COV (the dense-mapping tail's ObsCovModel call, MACVO.py:324) is mv_obs_cov on the map pixels, and the
    Python loop's map points (ops.map_points) carry the same pixels and bits."""
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath

    H, W, n_frames = 240, 320, 4
    cam, frames, _ = synth.make_sequence(n_frames, H, W, C=64, iters=1, seed=23)
    cfg = HotPathConfig(mapping=True, map_max_depth=13.0, map_max_depth_cov=0.5, map_num_point=500, graph_type="icp", cov_model=model,
                        cov_modifiers=mods)
    hot = NativeHotPath(Camera(**cam), cfg, gpu)
    py = HotPath(Camera(**cam), cfg, gpu, keep_extras=True)          # ops.map_points' model branch
    ins = _inputs(frames, gpu)
    hot.initialize(ins[0])
    py.initialize(ins[0])
    K = Camera(**cam).K4
    seen = 0
    for t in range(1, n_frames):
        torch.manual_seed(70 + t)
        res = hot.step(ins[t])
        torch.manual_seed(70 + t)
        rp = py.step(ins[t])
        torch.cuda.synchronize()
        m = res.map_points
        if m is None:
            assert rp.map_points is None
            continue
        n = m.uv.shape[0]
        seen += n
        m0 = hot.maps(1, 0)
        assert torch.equal(rp.map_points.uv, m.uv) and _eq(rp.map_points.cov_Tc, m.cov_Tc), (model, mods, t)
        sig = torch.zeros(n, 3, device=gpu)
        sig[:, :2] = cfg.match_cov_default
        want = ops.obs_cov(model, m0.depth, m.uv.contiguous(), sig, m.sigma_dd.contiguous(), *K, depth_cov_map=m0.depth_cov, modifiers=mods,
                           kernel_size=cfg.cov_kernel_size, min_flow_cov=cfg.min_flow_cov, min_depth_cov=cfg.min_depth_cov)
        assert _eq(m.cov_Tc, want), (model, mods, t)
    assert seen > 0
    hot.close()


def _oracle_cov(model, mods, depth_cov_of):
    """OracleHotPath's covariance call substituted by the CPU restatement of the model + modifiers (tests/cov_models_ref.py)."""
    from oracle import covariance

    match = covariance.match_covariance

    def cov(kp, depth_map, depth_cov, flow_cov, fx, fy, cx, cy, kernel_size=31, match_cov_default=0.25, min_flow_cov=0.25,
            min_depth_cov=0.05, return_aux=False):
        if model == "match":
            c = match(kp, depth_map, depth_cov, flow_cov, fx, fy, cx, cy, kernel_size=kernel_size, match_cov_default=match_cov_default,
                      min_flow_cov=min_flow_cov, min_depth_cov=min_depth_cov)
        elif model == "gmm":
            c = R.gmm_covariance(kp, depth_map, depth_cov_of(depth_map), depth_cov, flow_cov, fx, fy, cx, cy, kernel_size=kernel_size,
                                 match_cov_default=match_cov_default, min_flow_cov=min_flow_cov)
        else:
            c = R.no_covariance(kp.shape[0])
        return R.apply_chain(c, mods)
    return cov


@pytest.mark.parametrize("model,mods", CHAINS + [("match", ("normalize",)), ("match", ("normalize", "diag"))])
def test_sequence_matches_oracle_with_cov_model(gpu, monkeypatch, model, mods):
    """test_sequence_matches_oracle for every ablation chain on the ICP graph (where the covariances weight the solve): OracleHotPath with its
    covariance call substituted by the CPU restatement, HotPath (per-call obs_cov_pair) and NativeHotPath (fused launch) over 5 frames —
    keypoints bit-exact, the Python loop's covariances close to the oracle's, both poses within 1e-4 of the oracle at the same step count."""
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath
    from oracle import pipeline as opl
    from oracle import se3
    from oracle.pipeline import OracleHotPath

    n_frames = 5
    cam, frames, _ = synth.make_sequence(n_frames, 192, 256, C=64, iters=3, seed=3)
    ora = OracleHotPath(cam, dict(graph_type="icp"))
    maps = {}
    front = ora.frontend

    def rec_front(x):
        m = front(x)
        maps[id(m["depth"])] = m["cov"]
        return m
    ora.frontend = rec_front
    monkeypatch.setattr(opl.covariance, "match_covariance", _oracle_cov(model, mods, lambda d: maps[id(d)]))
    cfg = HotPathConfig(graph_type="icp", cov_model=model, cov_modifiers=mods)
    hot = HotPath(Camera(**cam), cfg, gpu, keep_extras=True)
    nat = NativeHotPath(Camera(**cam), cfg, gpu)
    ins = _inputs(frames, gpu)
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
        assert int(rh.n_valid.item()) == ro["n_valid"]
        if model != "gmm":                                      # (the mixture variance cancels in fp32: pinned by the golden test above)
            ex = rh.extras
            inb = ex["tracked"].inbound.cpu()
            torch.testing.assert_close(ex["cov0"].cpu()[inb], ro["cov0"], rtol=1e-3, atol=1e-7)
            torch.testing.assert_close(ex["cov1"].cpu()[inb], ro["cov1"], rtol=1e-3, atol=1e-7)
        for r in (rh, rn):
            dt, dr = se3.pose_error(ro["pose"].double(), r.pose.cpu().double())
            assert dt <= 1e-4 and dr <= 1e-4, (model, mods, t, dt, dr)
        assert int(rh.info[0, 1].item()) == ro["steps"], t
    nat.close()
