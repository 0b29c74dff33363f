"""GPU: covariance-free frontends (``provide_cov`` (d, m); (False, False) = Ablation_Study/TartanAirv2_Vanilla.yaml) in ops, HotPath and plugins.

* the epilogue with no / partial covariance: depth, disparity, flow planes bit-equal to the full epilogue's, the present covariance planes too;
* ``ops.obs_cov_pair(no_match_cov=True)``: every model x modifier chain x (depth variance given / absent) against the torch restatements
  (covariances: 5e-5 of the matrix scale, the project's bar against reference goldens), against the reference's own ``estimate(flow_cov=None)``
  results (tests/golden/covfree.npz) and BITWISE against the stand-alone ``mv_obs_cov`` with ``use_patch_var = 0``; the sigma table stays as it was;
* one frame pair through the ops in ``run_pair``'s order for the mixed goldens — the network's ``inference`` returns sigma^2 (``cov_is_log=False``),
  which is what the goldens replay: stored fp32 rows bit-equal, covariances 5e-5;
* ``HotPath`` sequences against the golden, every case: keypoints and stored rows bit for bit, covariances 5e-5, poses 1e-4 — the mixed cases with the
  covariance handed over as the golden's own sigma^2 (``FrameInputs.cov_is_log=False``), the CovAware + reproj case included, and once more as
  log-sigma (``0.5 * log``: exp(2 x) returns the stored value to 1 ulp only, so those runs compare the variance rows to 1e-6);
* ``HIP_FlowFormerDepth`` / ``HIP_FlowFormerMatcher`` and the covariance plugins with ``flow_cov=None`` in ``run_pair``'s call order vs the golden.

Reads only committed .npz data, never the reference tree."""
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import cov_models_ref as CM
from tests import covfree_ref as CR
from tests import refrun, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = {"vanilla": 2, "compose": 7, "sanity": 1}
COV_RTOL = refrun.TOL_KEYS["map/match//obs2_covTc"]        # 5e-5 of the matrix scale
POSE_TOL = 1e-4


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "covfree.npz"))
    g = {k: z[k] for k in z.files}
    g["meta"] = json.loads(str(g["meta"]))
    return g


def case(g, name):
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "/")}


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype in (torch.float32, torch.float64) else t


def cov_close(got, want, what):
    """row-relative (per 3 x 3 matrix) difference, as tests/refrun.compare_runs measures it"""
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if g.size == 0:
        return
    scale = np.abs(w).reshape(w.shape[0], -1).max(axis=1).reshape(-1, 1, 1)
    err = (np.abs(g - w) / np.maximum(scale, 1e-30)).max()
    print(f"{what}: max row-relative difference {err:.3e} (bound {COV_RTOL})")
    assert err <= COV_RTOL, (what, err)


# ------------------------------------------------------------------------------------------------------------------ epilogue
@pytest.mark.parametrize("cov_is_log", [True, False])
def test_partial_epilogue_is_bitwise_the_full_one(gpu, cov_is_log):
    from macvo_amd import _lib as L
    from macvo_amd import ops

    H, W = 96, 136
    g = torch.Generator().manual_seed(3)
    flow = (torch.randn(2, 2, H, W, generator=g) * 6).to(gpu)
    cov = (torch.randn(2, 2, H, W, generator=g) * 0.7 if cov_is_log else torch.rand(2, 2, H, W, generator=g) + 0.1).to(gpu)
    full = ops.frontend_epilogue(flow, cov, 0.25, 320.0, cov_is_log=cov_is_log, enforce_positive_disparity=True)
    for d, m in ((False, False), (True, False), (False, True)):
        c = cov.clone()
        if not d:
            c[0] = float("nan")                     # a side without covariance: its sample is not read
        if not m:
            c[1] = float("nan")
        for cin in ([None] if not (d or m) else []) + [c]:
            part = ops.frontend_epilogue(flow, cin, 0.25, 320.0, cov_is_log=cov_is_log, enforce_positive_disparity=True, provide_cov=(d, m))
            torch.cuda.synchronize()
            for k in ("depth", "disparity", "flow", "bad_mask"):
                assert torch.equal(_bits(getattr(part, k)), _bits(getattr(full, k))), (d, m, k)
            for k, have in (("depth_cov", d), ("disparity_cov", d), ("flow_cov", m)):
                if have:
                    assert torch.equal(_bits(getattr(part, k)), _bits(getattr(full, k))), (d, m, k)
                else:
                    assert getattr(part, k) is None, (d, m, k)
    with pytest.raises(L.MacvoHipError):
        ops.frontend_epilogue(flow, None, 0.25, 320.0, provide_cov=(True, False))
    # depth only (IStereoDepth.estimate of a model without covariance), and two lanes through the C entry point
    only = ops.frontend_epilogue(flow[0:1], None, 0.25, 320.0, want_match=False, provide_cov=(False, False))
    assert torch.equal(_bits(only.depth), _bits(full.depth)) and only.flow is None and only.depth_cov is None
    lib = L.load()
    fl2 = torch.cat([flow, flow.flip(0)]).contiguous()
    depth2, disp2, mf2 = (torch.empty((2, c_, H, W), device=gpu) for c_ in (1, 1, 2))
    L.check(lib.mv_frontend_epilogue_lanes(fl2.data_ptr(), None, 1, H, W, 80.0, 6400.0, disp2.data_ptr(), None, depth2.data_ptr(), None, None,
                                           mf2.data_ptr(), None, 2, None), "mv_frontend_epilogue_lanes")
    torch.cuda.synchronize()
    assert torch.equal(_bits(depth2[0:1]), _bits(full.depth)) and torch.equal(_bits(mf2[0:1]), _bits(full.flow))
    assert torch.equal(_bits(disp2[1, 0]), _bits(flow[1, 0].abs())) and torch.equal(_bits(mf2[1]), _bits(flow[0]))
    # a covariance output without its input is refused
    assert lib.mv_frontend_epilogue_lanes(fl2.data_ptr(), None, 1, H, W, 80.0, 6400.0, disp2.data_ptr(), disp2.data_ptr(), depth2.data_ptr(), None, None,
                                          mf2.data_ptr(), None, 2, None) != 0


# ------------------------------------------------------------------------------------------------------------------ covariance pair
def _frame1(gold):
    from oracle import frontend

    cam, maps, _ = refrun.tartanair_maps()
    disp = maps[1]["flow"][0:1, 0:1].abs()
    depth = frontend.disparity_to_depth(disp, cam["baseline"], cam["fx"])
    dcov = frontend.disparity_to_depth_cov(disp, maps[1]["cov"][0:1, 0:1], cam["baseline"], cam["fx"])
    return cam, depth, dcov, torch.from_numpy(gold["direct/kp"]), torch.from_numpy(gold["direct/depth_cov_kp"])


def _apply_chain(c, mods):
    """Modifier_Diagonalize / Modifier_Normalize on fp64 matrices with the determinant as the kernel documents it (match_cov_dev.h: the cofactor
    expansion along the first row).  For this fixture's near-singular matrices (condition ~1e5) torch.det's LU and the expansion differ by up to
    ~1e-11 relative — cancellation in either, not an error of one — so the 1e-12 bar of tests/test_gpu_cov_models.py is held against the same formula."""
    for name in mods:
        if name == "diag":
            c = CM.diagonalize(c)
        else:
            det = (c[:, 0, 0] * (c[:, 1, 1] * c[:, 2, 2] - c[:, 1, 2] * c[:, 2, 1]) - c[:, 0, 1] * (c[:, 1, 0] * c[:, 2, 2] - c[:, 1, 2] * c[:, 2, 0])) \
                + c[:, 0, 2] * (c[:, 1, 0] * c[:, 2, 1] - c[:, 1, 1] * c[:, 2, 0])
            c = c / det.reshape(-1, 1, 1)
    return c


@pytest.mark.parametrize("mods", [(), ("diag",), ("normalize",), ("diag", "normalize")])
@pytest.mark.parametrize("model,have_d", [("match", True), ("match", False), ("gmm", True), ("none", True), ("none", False)])
def test_obs_cov_pair_without_match_cov(gpu, gold, model, have_d, mods):
    from macvo_amd import ops
    from oracle import covariance

    cam, depth, dcov, kp, dc = _frame1(gold)
    K = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    c_model = gold["meta"]["model_match_cov_default"]
    g = torch.Generator().manual_seed(11)
    kp1 = kp.float() + torch.rand(kp.shape[0], 2, generator=g)                    # tracked positions are fractional
    dc1 = dcov[0, 0, kp1[:, 1].long(), kp1[:, 0].long()].contiguous()
    dc1[::7] = 0.01                                                               # below min_depth_cov: MatchCovariance clamps, the mixture does not
    s0 = torch.ones(kp.shape[0], 3) * 0.25
    s0[:, 2] = 0
    sig0, sig1 = s0.clone().to(gpu), torch.full((kp.shape[0], 3), -1.0, device=gpu)
    dmap = dcov.to(gpu) if (have_d or model == "gmm") else None
    got0, _, got1 = ops.obs_cov_pair(model, depth.to(gpu), kp.float().to(gpu), sig0, depth.to(gpu), kp1.to(gpu), None, *K,
                                     depth_cov_map0=dmap, depth_cov_map1=dmap, modifiers=mods, no_match_cov=True, match_cov_default=c_model,
                                     depth_cov1=dc1.to(gpu) if have_d else None)
    torch.cuda.synchronize()
    assert (sig1 == -1).all()
    # set 0 is the pair launch as it always was
    want0 = ops.obs_cov_pair(model, depth.to(gpu), kp.float().to(gpu), s0.clone().to(gpu), depth.to(gpu), kp.float().to(gpu), s0.clone().to(gpu), *K,
                             depth_cov_map0=dmap, depth_cov_map1=dmap, modifiers=mods)[0]
    assert torch.equal(_bits(got0), _bits(want0))
    # set 1, bitwise: the stand-alone kernel with the model's sigma (0.5 >= min_flow_cov^2: its clamp is the identity) and use_patch_var = 0
    s1 = torch.ones(kp.shape[0], 3) * c_model
    s1[:, 2] = 0
    alone = ops.obs_cov(model, depth.to(gpu), kp1.to(gpu), s1.to(gpu), dc1.to(gpu) if have_d else None, *K, depth_cov_map=dmap, modifiers=mods,
                        use_patch_var=not have_d)
    assert torch.equal(_bits(got1), _bits(alone)), (model, have_d, mods)
    # ... and the model's sigma is NOT clamped by min_flow_cov: with c below min_flow_cov^2 the clamped stand-alone call differs, the unclamped agrees
    if model != "none":
        small = 0.01
        low = ops.obs_cov_pair(model, depth.to(gpu), kp.float().to(gpu), s0.clone().to(gpu), depth.to(gpu), kp1.to(gpu), None, *K,
                               depth_cov_map0=dmap, depth_cov_map1=dmap, modifiers=mods, no_match_cov=True, match_cov_default=small,
                               depth_cov1=dc1.to(gpu) if have_d else None)[2]
        s_small = torch.ones(kp.shape[0], 3) * small
        s_small[:, 2] = 0
        unclamped = ops.obs_cov(model, depth.to(gpu), kp1.to(gpu), s_small.clone().to(gpu), dc1.to(gpu) if have_d else None, *K, depth_cov_map=dmap,
                                modifiers=mods, use_patch_var=not have_d, min_flow_cov=0.0)
        clamped = ops.obs_cov(model, depth.to(gpu), kp1.to(gpu), s_small.clone().to(gpu), dc1.to(gpu) if have_d else None, *K, depth_cov_map=dmap,
                              modifiers=mods, use_patch_var=not have_d, min_flow_cov=0.25)
        assert torch.equal(_bits(low), _bits(unclamped)) and not torch.equal(_bits(low), _bits(clamped))
    # the torch restatements (flow_cov=None)
    if model == "match":
        want = covariance.match_covariance(kp1, depth, dc1.clone() if have_d else None, None, *K, kernel_size=31, match_cov_default=c_model,
                                           min_flow_cov=0.25, min_depth_cov=0.05)
    elif model == "gmm":
        want = CM.gmm_covariance(kp1, depth, dcov, dc1.clone(), None, *K, kernel_size=31, match_cov_default=c_model, min_flow_cov=0.25)
    else:
        want = torch.eye(3, dtype=torch.float64).repeat(kp.shape[0], 1, 1)
    if not mods:
        cov_close(got1.cpu().numpy(), want.numpy(), f"obs_cov_pair nomatch {model} d={have_d}")
    else:
        # a modifier chain is checked as tests/test_gpu_cov_models.py checks it: as the reference's operation on the kernel's OWN unmodified result (1e-12) —
        # Modifier_Normalize divides by det(cov), which turns the model's 5e-5 into an unbounded relative error for the near-singular matrices of this fixture
        base = ops.obs_cov_pair(model, depth.to(gpu), kp.float().to(gpu), s0.clone().to(gpu), depth.to(gpu), kp1.to(gpu), None, *K,
                                depth_cov_map0=dmap, depth_cov_map1=dmap, no_match_cov=True, match_cov_default=c_model,
                                depth_cov1=dc1.to(gpu) if have_d else None)[2].cpu()
        cov_close(base.numpy(), want.numpy(), f"obs_cov_pair nomatch {model} d={have_d} (base of mods={mods})")
        torch.testing.assert_close(got1.cpu(), _apply_chain(base, mods), rtol=1e-12, atol=0)


def test_obs_cov_pair_without_match_cov_vs_the_reference_classes(gpu, gold):
    """The reference's own MatchCovariance / GaussianMixtureCovariance.estimate(..., flow_cov=None) at the golden's integer keypoints."""
    from macvo_amd import ops

    cam, depth, dcov, kp, dc = _frame1(gold)
    K = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    s0 = torch.ones(kp.shape[0], 3) * 0.25
    s0[:, 2] = 0
    for model, have_d, key in (("match", False, "direct/match_nodepthcov"), ("match", True, "direct/match_depthcov"), ("gmm", True, "direct/gmm_depthcov")):
        dmap = dcov.to(gpu) if model == "gmm" else None
        got = ops.obs_cov_pair(model, depth.to(gpu), kp.float().to(gpu), s0.clone().to(gpu), depth.to(gpu), kp.float().to(gpu), None, *K,
                               depth_cov_map0=dmap, depth_cov_map1=dmap, no_match_cov=True, match_cov_default=0.5,
                               depth_cov1=dc.to(gpu) if have_d else None)[2]
        cov_close(got.cpu().numpy(), gold[key], key)
    with pytest.raises(ops.L.MacvoHipError):
        ops.obs_cov_pair("gmm", depth.to(gpu), kp.float().to(gpu), s0.clone().to(gpu), depth.to(gpu), kp.float().to(gpu), None, *K,
                         depth_cov_map0=dcov.to(gpu), depth_cov_map1=dcov.to(gpu), no_match_cov=True)


# ------------------------------------------------------------------------------------------------------------------ sequences vs the golden
def _cfg_of(meta, name, **kw):
    from macvo_amd.pipeline import HotPathConfig

    d, m, sel, cov, outlier, graph = meta["cases"][name]
    return HotPathConfig(frontend_cov=(bool(d), bool(m)), selector={"RandomSelector": "random", "GridSelector": "grid"}.get(sel, "nodepth"),
                         cov_model="none" if cov == "NoCovariance" else "match", cov_match_cov_default=meta["model_match_cov_default"],
                         match_cov_default=meta["odom_match_cov_default"], filters=FILTERS[outlier], graph_type=graph, **kw)


def _inputs(maps, cam, gpu, d, m, C=32, sigma2=False):
    """FrameInputs of the TartanAir fixture: the stored flow; the covariance where a side provides one (None when neither does) — as log-sigma, or with
    ``sigma2`` as the golden's own sigma^2 (``cov_is_log=False``); feature maps / lookup coordinates of a synthetic stream (their consumer is not part
    of the hot path)."""
    from macvo_amd.pipeline import FrameInputs

    _, fr, _ = synth.make_sequence(len(maps), cam["H"], cam["W"], C=C, iters=1, seed=4)
    out = []
    for t, f in enumerate(maps):
        logcov = (f["cov"] if sigma2 else 0.5 * torch.log(f["cov"])).to(gpu) if (d or m) else None
        out.append(FrameInputs(fmap1=fr[t]["fmap1"].to(gpu), fmap2=fr[t]["fmap2"].to(gpu), coords=fr[t]["coords"].to(gpu), flow=f["flow"].to(gpu),
                               logcov=logcov, cov_is_log=not sigma2))
    torch.cuda.synchronize()
    return out


def check_frame_against_golden(g, t, ex, kp_all, pose, d, m, what, exact_variances):
    """One frame's HotPath / NativeHotPath extras against the rows the reference stored for it."""
    ranges = g["map/edge/frame2match/ranges"]
    lo, n = int(ranges[t, 0, 0]), int(ranges[t, 0, 1])
    tr, valid = ex["tracked"], ex["valid"].bool().cpu()
    assert int(valid.sum()) == n, (what, t, int(valid.sum()), n)
    rows = lambda x: x.cpu()[valid].numpy()  # noqa: E731
    assert np.array_equal(g["map/match//pixel1_uv"][lo:lo + n], rows(tr.kp0_uv)), (what, t)                # keypoints: bit-exact
    assert np.array_equal(g["map/match//pixel1_uv"][lo:lo + n], rows(kp_all.float())), (what, t)
    assert np.array_equal(g["map/match//pixel2_uv"][lo:lo + n], rows(tr.kp1_uv)), (what, t)
    vals = tr.vals.cpu()
    names = ("pixel1_d", "pixel1_disp", "pixel1_disp_cov", "pixel1_d_cov", "pixel2_d", "pixel2_disp", "pixel2_disp_cov", "pixel2_d_cov")
    for r, k in enumerate(names):
        want, got = g[f"map/match//{k}"][lo:lo + n, 0], vals[r][valid].numpy()
        if k.endswith("_cov") and d and not exact_variances:
            assert np.allclose(want, got, rtol=1e-6, atol=0), (what, t, k)
        else:
            assert np.array_equal(want, got), (what, t, k)                                                  # stored fp32 rows: bit-equal
    assert np.array_equal(g["map/match//pixel1_uv_cov"][lo:lo + n], rows(tr.sigma0)), (what, t)
    if m and not exact_variances:
        assert np.allclose(g["map/match//pixel2_uv_cov"][lo:lo + n], rows(tr.sigma1), rtol=1e-6, atol=0), (what, t)
    else:
        assert np.array_equal(g["map/match//pixel2_uv_cov"][lo:lo + n], rows(tr.sigma1)), (what, t)         # (-1, -1, -1) without m
    cov_close(rows(ex["cov0"]), g["map/match//obs1_covTc"][lo:lo + n], f"{what} frame {t} obs1_covTc")
    cov_close(rows(ex["cov1"]), g["map/match//obs2_covTc"][lo:lo + n], f"{what} frame {t} obs2_covTc")
    cov_close(rows(ex["cov0_w"]), g["map/points//cov_Tw"][lo:lo + n], f"{what} frame {t} cov_Tw")
    pw, gw = rows(ex["pos_Tw"]).astype(np.float64), g["map/points//pos_Tw"][lo:lo + n].astype(np.float64)
    err = (np.abs(pw - gw) / np.abs(gw).max(axis=1, keepdims=True)).max()
    assert err <= refrun.TOL_KEYS["map/points//pos_Tw"], (what, t, err)
    dp = np.abs(g["map/frames//pose"][t] - pose.cpu().numpy()).max()
    print(f"{what} frame {t}: {n} observations, max pose difference {dp:.3e} (bound {POSE_TOL})")
    assert dp <= POSE_TOL, (what, t, dp)


# (sigma2: the covariance handed over as the golden's own sigma^2 — every stored row bit-equal — or as log-sigma, whose exp(2 x) returns it to 1 ulp: the
# variance rows are then compared to 1e-6.  "01_nodepth_reproj" runs with sigma^2 only: the CovAware selector's candidate COUNT decides the whole
# permutation, and a quality map rebuilt from log-sigma is 1 ulp off the golden's.)
@pytest.mark.parametrize("name,sigma2", [("vanilla", False), ("00_grid_match", False), ("00_rand_match", False)] +
                         [(n, s2) for n in ("10_rand_match", "10_grid_none", "01_rand_match", "01_grid_match") for s2 in (True, False)] +
                         [("01_nodepth_reproj", True)])
def test_hot_path_sequences_match_the_reference_loop(gpu, gold, name, sigma2):
    from macvo_amd.pipeline import Camera, HotPath

    meta = gold["meta"]
    d, m = bool(meta["cases"][name][0]), bool(meta["cases"][name][1])
    cam, maps, _ = refrun.tartanair_maps()
    ins = _inputs(maps, cam, gpu, d, m, sigma2=sigma2)
    g = case(gold, name)
    torch.manual_seed(meta["seed"])                      # the selectors consume the global CPU generator, as the reference's do
    hot = HotPath(Camera(**cam), _cfg_of(meta, name), gpu, keep_extras=True)
    hot.initialize(ins[0])
    for t in range(1, len(ins)):
        r = hot.step(ins[t])
        torch.cuda.synchronize()
        if not d:
            assert r.extras["maps1"].depth_cov is None and r.extras["maps1"].disparity_cov is None
        if not m:
            assert r.extras["maps1"].flow_cov is None
        check_frame_against_golden(g, t, r.extras, r.kp0_uv, r.pose, d, m, f"HotPath {name}", exact_variances=sigma2 or not (d or m))


@pytest.mark.parametrize("name", ["10_rand_match", "10_grid_none", "01_rand_match", "01_grid_match", "01_nodepth_reproj"])
def test_ops_in_run_pair_order_match_the_mixed_goldens_bit_for_bit(gpu, gold, name):
    """The mixed frontends with the covariance as the network's ``inference`` returns it (sigma^2, cov_is_log=False) — the goldens' own input —
    through the launches HotPath.finish makes: every stored fp32 row bit-equal, covariances 5e-5."""
    from macvo_amd import ops
    from tests import selectors_ref as SR

    meta = gold["meta"]
    d, m, sel, covm, outlier, graph = meta["cases"][name]
    d, m = bool(d), bool(m)
    model = "none" if covm == "NoCovariance" else "match"
    cam, maps, _ = refrun.tartanair_maps()
    K4 = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    pose = torch.tensor([0, 0, 0, 0, 0, 0, 1], dtype=torch.float32, device=gpu)
    intr, bl = torch.tensor([K4], dtype=torch.float32, device=gpu), torch.tensor([cam["baseline"]], dtype=torch.float32, device=gpu)
    g = case(gold, name)
    ranges = g["map/edge/frame2match/ranges"]
    torch.manual_seed(meta["seed"])
    fm = lambda f: ops.frontend_epilogue(f["flow"].to(gpu), f["cov"].to(gpu), cam["baseline"], cam["fx"], cov_is_log=False, provide_cov=(d, m))  # noqa: E731
    maps0 = fm(maps[0])
    for t in range(1, len(maps)):
        maps1 = fm(maps[t])
        if sel == "CovAwareSelector_NoDepth":
            kp = ops.kp_select("nodepth", cam["H"], cam["W"], flow_cov=maps1.flow_cov, kernel_size=7, mask_width=32, max_match_cov=100.0).finish(200)
        else:
            kp = (SR.random_select(200, cam["H"], cam["W"], 32) if sel == "RandomSelector" else SR.grid_select(200, cam["H"], cam["W"], 32)).to(gpu)
        tr = ops.kp_track(kp, maps1.flow, maps1.flow_cov, maps0, maps1, 32, meta["odom_match_cov_default"])
        _, pos_Tw, rot = ops.backproject(tr.kp0_uv, tr.vals[0], K4, pose, want_rot=True)
        if m:
            c0, c0w, c1 = ops.obs_cov_pair(model, maps0.depth, tr.kp0_uv, tr.sigma0, maps1.depth, tr.kp1_uv, tr.sigma1, *K4, rot=rot)
        else:
            c0, c0w, c1 = ops.obs_cov_pair(model, maps0.depth, tr.kp0_uv, tr.sigma0, maps1.depth, tr.kp1_uv, None, *K4, rot=rot, no_match_cov=True,
                                           match_cov_default=meta["model_match_cov_default"], depth_cov1=tr.vals[7] if d else None)
        valid, _ = ops.obs_filter(tr.inbound, c0, c1, tr.vals, FILTERS[outlier], 0.05, cam["fx"] * cam["baseline"])
        torch.cuda.synchronize()
        valid = valid.cpu()
        lo, n = int(ranges[t, 0, 0]), int(ranges[t, 0, 1])
        assert int(valid.sum()) == n, (name, t)
        vals = tr.vals.cpu()
        for r, k in enumerate(("pixel1_d", "pixel1_disp", "pixel1_disp_cov", "pixel1_d_cov", "pixel2_d", "pixel2_disp", "pixel2_disp_cov", "pixel2_d_cov")):
            assert np.array_equal(g[f"map/match//{k}"][lo:lo + n, 0], vals[r][valid].numpy()), (name, t, k)
        assert np.array_equal(g["map/match//pixel2_uv_cov"][lo:lo + n], tr.sigma1.cpu()[valid].numpy()), (name, t)   # clamped in place with m, -1 without
        assert np.array_equal(g["map/match//pixel1_uv"][lo:lo + n], tr.kp0_uv.cpu()[valid].numpy())
        cov_close(c0.cpu()[valid].numpy(), g["map/match//obs1_covTc"][lo:lo + n], f"ops {name} frame {t} obs1_covTc")
        cov_close(c1.cpu()[valid].numpy(), g["map/match//obs2_covTc"][lo:lo + n], f"ops {name} frame {t} obs2_covTc")
        nk = kp.shape[0]
        offs = torch.tensor([0, nk], dtype=torch.int32, device=gpu)
        batch = ops.PGOBatch(offsets=offs, init_pose=pose.reshape(1, 7), intrinsics=intr, baseline=bl, pos_Tw=pos_Tw, pixel2_uv=tr.kp1_uv, cov_Tw=c0w,
                             pixel2_d=tr.vals[4], pixel2_disp=tr.vals[5], pixel2_disp_cov=tr.vals[6], pixel2_uv_cov=tr.sigma1, obs2_covTc=c1,
                             valid=valid.to(gpu))
        new_pose = torch.empty((1, 7), dtype=torch.float32, device=gpu)
        ops.pgo_solve(batch, graph, min_points=10, out_pose_f32=new_pose)
        torch.cuda.synchronize()
        pose = new_pose.reshape(7)
        dp = np.abs(g["map/frames//pose"][t] - pose.cpu().numpy()).max()
        print(f"ops {name} frame {t}: {n} observations, max pose difference {dp:.3e} (bound {POSE_TOL})")
        assert dp <= POSE_TOL, (name, t, dp)
        maps0 = maps1


def test_hot_path_refuses_what_reads_a_missing_covariance(gpu):
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig

    cam = Camera(320.0, 320.0, 320.0, 240.0, 0.25, 480, 640)
    for fc, kw in (((False, False), dict(selector="nodepth", graph_type="icp")), ((True, False), dict(selector="random", graph_type="reproj")),
                   ((False, True), dict(selector="nodepth", graph_type="disp")), ((False, True), dict(cov_model="gmm", graph_type="icp"))):
        with pytest.raises(ValueError, match="provides no covariance"):
            HotPath(cam, HotPathConfig(frontend_cov=fc, **kw), gpu)


# ------------------------------------------------------------------------------------------------------------------ plugins
class _PlainNet:
    """Stands in for the plain FlowFormer: ``inference(A, B) -> (flow [2, H, W], None)``, unbatched like the network's own (the reference's
    ``est_flow[:1]`` / ``flow.unsqueeze(0)`` rely on it); which of a frame's two pairs is asked for follows from B (right image = stereo pair)."""

    def __init__(self, maps, dev):
        self.maps = [f["flow"].to(dev) for f in maps]

    def inference(self, A, B):
        t = int(round(float(A[0, 0, 0, 0]) * 255.0))
        tb = int(round(float(B[0, 0, 0, 0]) * 255.0))
        if tb == 254:                                   # the right image carries the marker 254 / 255: stereo pair of frame t
            return self.maps[t][0].clone(), None
        return self.maps[tb][1].clone(), None            # temporal pair (frame t -> frame tb)

    def eval(self):
        return self


@pytest.mark.parametrize("name", ["vanilla", "00_rand_match"])
def test_plugins_in_run_pair_order_match_the_golden(gpu, gold, name):
    """HIP_FlowFormerDepth / HIP_FlowFormerMatcher (stand-in config.model), HIP_RandomSelector, the covariance plugin with flow_cov=None, on
    this repository's interface classes, called as run_pair calls them (MACVO.py:182-269) for every frame pair of the fixture."""
    import macvo_amd.plugins as P
    from macvo_amd import ops

    meta = gold["meta"]
    _, _, _, covm, outlier, _ = meta["cases"][name]
    cam, maps, _ = refrun.tartanair_maps()
    g = case(gold, name)
    H, W = cam["H"], cam["W"]
    net = _PlainNet(maps, gpu)
    ffargs = NS(weight="", device="cuda", model=net)
    P.HIP_FlowFormerDepth.is_valid_config(NS(weight="", device="cuda"))
    P.HIP_FlowFormerMatcher.is_valid_config(NS(weight="", device="cuda"))
    depth_m, match_m = P.HIP_FlowFormerDepth(ffargs), P.HIP_FlowFormerMatcher(ffargs)
    assert depth_m.provide_cov is False and match_m.provide_cov is False
    sel = P.HIP_RandomSelector(NS(mask_width=32, device="cuda"))
    if covm == "NoCovariance":
        cov_m = P.HIP_NoCovariance(None)
    else:
        cov_m = P.HIP_MatchCovariance(NS(device="cuda", kernel_size=31, match_cov_default=meta["model_match_cov_default"], min_depth_cov=0.05, min_flow_cov=0.25))

    def frame(t):
        L = torch.zeros(1, 3, H, W)
        L[0, :, 0, 0] = t / 255.0
        R = torch.zeros(1, 3, H, W)
        R[0, :, 0, 0] = 254 / 255.0
        return NS(imageL=L, imageR=R, height=H, width=W, fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], frame_baseline=cam["baseline"])

    ranges = g["map/edge/frame2match/ranges"]
    torch.manual_seed(meta["seed"])
    depth0 = depth_m.estimate(frame(0))
    for t in range(1, len(maps)):
        f0, f1 = frame(t - 1), frame(t)
        depth1, match01 = depth_m.estimate(f1), match_m.forward(f0, f1)
        assert depth1.cov is None and depth1.disparity_uncertainty is None and match01.cov is None            # Output(depth, disparity) / Output(flow)
        assert depth1.depth.shape == (1, 1, H, W) and depth1.disparity.shape == (1, 1, H, W) and match01.flow.shape == (1, 2, H, W)
        kp0 = sel.select_point(f0, 200, depth0, depth1, match01)
        tr = ops.kp_track(kp0, match01.flow, match01.cov, {"depth": depth0.depth, "disparity": depth0.disparity, "disparity_cov": None, "depth_cov": None},
                          {"depth": depth1.depth, "disparity": depth1.disparity, "disparity_cov": None, "depth_cov": None}, 32, 0.25)
        inb = tr.inbound
        k0, k1 = tr.kp0_uv[inb], tr.kp1_uv[inb]
        c0 = cov_m.estimate(f0, k0, depth0, None, tr.sigma0[inb].contiguous())
        c1 = cov_m.estimate(f1, k1, depth1, None, None)                                                  # kp1_sigma_uv is None (MACVO.py:231-232)
        d0, d1 = tr.vals[0][inb].cpu(), tr.vals[4][inb].cpu()
        keep = ~((d0 < 0.05) | (d0 > cam["fx"] * cam["baseline"]) | (d1 < 0.05) | (d1 > cam["fx"] * cam["baseline"]))   # SimpleDepthFilter (Vanilla's outlier block)
        assert outlier == "vanilla"
        lo, n = int(ranges[t, 0, 0]), int(ranges[t, 0, 1])
        assert int(keep.sum()) == n
        assert np.array_equal(g["map/match//pixel1_uv"][lo:lo + n], k0.cpu()[keep].numpy())
        assert np.array_equal(g["map/match//pixel2_uv"][lo:lo + n], k1.cpu()[keep].numpy())
        assert np.array_equal(g["map/match//pixel1_d"][lo:lo + n, 0], d0[keep].numpy()) and np.array_equal(g["map/match//pixel2_d"][lo:lo + n, 0], d1[keep].numpy())
        assert np.array_equal(g["map/match//pixel2_disp"][lo:lo + n, 0], tr.vals[5][inb].cpu()[keep].numpy())
        assert (tr.vals[7] == -1).all() or (tr.vals[7][inb] == -1).all()
        assert (tr.sigma1[inb] == -1).all()
        cov_close(c0[keep].numpy(), g["map/match//obs1_covTc"][lo:lo + n], f"plugins {name} frame {t} obs1_covTc")
        cov_close(c1[keep].numpy(), g["map/match//obs2_covTc"][lo:lo + n], f"plugins {name} frame {t} obs2_covTc")
        depth0 = depth1
    with pytest.raises(ops.L.MacvoHipError):                                                             # a batched flow is not the plain network's
        P._unbatched_flow(torch.zeros(2, 2, 8, 8), "test")
