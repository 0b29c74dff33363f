"""CPU: covariance-free frontends (``provide_cov`` (d, m) other than (True, True); Ablation_Study/TartanAirv2_Vanilla.yaml is (False, False)).

  * tests/covfree_ref.py — the torch restatement of the cov-free ``run_pair`` — against what the reference's own, unmodified loop stored
    (tests/golden/covfree.npz): keypoints and every stored row bit for bit, covariances and poses to 1e-6 (same host class, CPU both);
  * the config mappers (``frontend_config_fields``, ``filter_config_fields``, ``cov_config_fields``' new key, ``hot_path_config``) — in the build
    container on every experiment YAML of the reference, and the Vanilla YAML in ``HIP_*`` types through the reference's own validator;
  * every refusal of a configuration that would read a covariance the frontend does not give, in Python and in the C ABI;
  * the ABI: still version 8, the new symbols resolve, the config struct's new fields default to "both covariances there"."""
import ctypes as C
import json
import os
import subprocess
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import covfree_ref as CR
from tests import refrun
from tests.test_reference_abcs import REF  # noqa: E402  (the reference checkout the ABC test uses)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "covfree.npz")
FILTERS = {"vanilla": CR.FILTER_SIMPLE_DEPTH, "compose": 7, "sanity": CR.FILTER_COV_SANITY}
STORED = ("pixel1_disp", "pixel2_disp", "pixel1_disp_cov", "pixel2_disp_cov", "pixel1_d_cov", "pixel2_d_cov", "pixel1_uv_cov", "pixel2_uv_cov")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    g = {k: z[k] for k in z.files}
    g["meta"] = json.loads(str(g["meta"]))
    return g


def case(g, name):
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "/")}


def ref_cfg(meta, name) -> dict:
    d, m, sel, cov, outlier, graph = meta["cases"][name]
    return dict(frontend_cov=(bool(d), bool(m)), selector={"RandomSelector": "random", "GridSelector": "grid"}.get(sel, "nodepth"),
                cov_model="none" if cov == "NoCovariance" else "match", cov_match_cov_default=meta["model_match_cov_default"],
                match_cov_default=meta["odom_match_cov_default"], filters=FILTERS[outlier], graph_type=graph)


def test_golden_covers_the_contract(gold):
    meta = gold["meta"]
    assert meta["model_match_cov_default"] == 0.5 != meta["odom_match_cov_default"] == 0.25
    specs = meta["cases"]
    assert {(s[0], s[1]) for s in specs.values()} == {(0, 0), (1, 0), (0, 1)}
    assert {s[2] for s in specs.values()} >= {"RandomSelector", "GridSelector", "CovAwareSelector_NoDepth"}
    assert {s[3] for s in specs.values()} == {"NoCovariance", "MatchCovariance"} and "reproj" in {s[5] for s in specs.values()}
    assert specs["vanilla"] == [0, 0, "RandomSelector", "NoCovariance", "vanilla", "icp"]
    want = {"RandomSelector": [126, 124, 107], "GridSelector": [131, 132, 126], "CovAwareSelector_NoDepth": [172, 185, 185]}
    for name, s in specs.items():
        c = case(gold, name)
        assert not c["map/frames//need_interp"].any(), name                       # every frame was solved
        assert [int(r[0, 1]) for r in c["map/edge/frame2match/ranges"][1:]] == want[s[2]], name
        for k in ("pixel1_d_cov", "pixel2_d_cov", "pixel1_disp_cov", "pixel2_disp_cov"):
            assert bool((c[f"map/match//{k}"] == -1).all()) == (not s[0]), (name, k)
        assert bool((c["map/match//pixel2_uv_cov"] == -1).all()) == (not s[1]), name
        assert (c["map/match//pixel1_uv_cov"] == np.float32([0.25, 0.25, 0])).all(), name
        if s[3] == "NoCovariance":
            assert (c["map/match//obs2_covTc"] == np.eye(3)).all() and (c["map/match//obs1_covTc"] == np.eye(3)).all()


def test_restatement_reproduces_the_reference_loop(gold):
    cam, maps, _ = refrun.tartanair_maps()
    for name in gold["meta"]["cases"]:
        cfg = ref_cfg(gold["meta"], name)
        if cfg["selector"] == "nodepth":
            continue                                                                # (the CovAware selector has its own restatement: oracle/selector.py)
        g = case(gold, name)
        torch.manual_seed(gold["meta"]["seed"])
        ora = CR.CovFreeRef(cam, cfg)
        ora.initialize(dict(flow=maps[0]["flow"], cov_exp=maps[0]["cov"]))
        ranges = g["map/edge/frame2match/ranges"]
        for t in range(1, len(maps)):
            r = ora.step(dict(flow=maps[t]["flow"], cov_exp=maps[t]["cov"]))
            lo, n = int(ranges[t, 0, 0]), int(ranges[t, 0, 1])
            mk = r["mask"]
            assert r["solved"] and int(mk.sum()) == n, (name, t)
            assert np.array_equal(g["map/match//pixel1_uv"][lo:lo + n], r["kp0"][mk].float().numpy()), (name, t)
            assert np.array_equal(g["map/match//pixel2_uv"][lo:lo + n], r["kp1"][mk].numpy()), (name, t)
            assert np.array_equal(g["map/match//pixel1_d"][lo:lo + n, 0], r["kp0_d"][mk].numpy())
            assert np.array_equal(g["map/match//pixel2_d"][lo:lo + n, 0], r["kp1_d"][mk].numpy())
            for k in STORED:
                assert np.array_equal(g[f"map/match//{k}"][lo:lo + n], r["stored"][k][mk].numpy()), (name, t, k)
            assert np.allclose(g["map/match//obs1_covTc"][lo:lo + n], r["cov0"][mk].numpy(), rtol=1e-6, atol=1e-12), (name, t)
            assert np.allclose(g["map/match//obs2_covTc"][lo:lo + n], r["cov1"][mk].numpy(), rtol=1e-6, atol=1e-12), (name, t)
            assert np.abs(g["map/frames//pose"][t] - r["pose"].numpy()).max() < 1e-6, (name, t)


def test_direct_calls_without_flow_cov(gold):
    """``estimate(..., flow_cov=None)``: sigma = the model's (0.5, 0.5, 0) unclamped; with a depth_cov that IS the variance (clamped by
    min_depth_cov in MatchCovariance, as it is in the mixture model), without one the patch statistic."""
    from oracle import covariance, frontend
    from tests import cov_models_ref as CM

    cam, maps, _ = refrun.tartanair_maps()
    K = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    disp = maps[1]["flow"][0:1, 0:1].abs()
    depth = frontend.disparity_to_depth(disp, cam["baseline"], cam["fx"])
    dcov = frontend.disparity_to_depth_cov(disp, maps[1]["cov"][0:1, 0:1], cam["baseline"], cam["fx"])
    kp, dc = torch.from_numpy(gold["direct/kp"]), torch.from_numpy(gold["direct/depth_cov_kp"])
    assert torch.equal(dc, dcov[0, 0, kp[:, 1], kp[:, 0]])
    kw = dict(kernel_size=31, match_cov_default=0.5, min_flow_cov=0.25, min_depth_cov=0.05)
    a = covariance.match_covariance(kp, depth, None, None, *K, **kw)
    b = covariance.match_covariance(kp, depth, dc.clone(), None, *K, **kw)
    assert np.allclose(gold["direct/match_nodepthcov"], a.numpy(), rtol=1e-6, atol=1e-12)
    assert np.allclose(gold["direct/match_depthcov"], b.numpy(), rtol=1e-6, atol=1e-12)
    assert np.array_equal(gold["direct/match_depthcov"][:, 0, 0], dc.clamp(min=0.05).double().numpy())    # szz = the given variance
    kwg = dict(kernel_size=31, match_cov_default=0.5, min_flow_cov=0.25)
    c = CM.gmm_covariance(kp, depth, dcov, None, None, *K, **kwg)
    d = CM.gmm_covariance(kp, depth, dcov, dc.clone(), None, *K, **kwg)
    assert np.allclose(gold["direct/gmm_nodepthcov_arg"], c.numpy(), rtol=1e-5, atol=1e-12)
    assert np.allclose(gold["direct/gmm_depthcov"], d.numpy(), rtol=1e-5, atol=1e-12)
    assert np.array_equal(gold["direct/gmm_depthcov"][:, 0, 0], dc.double().numpy())                    # no clamp in the mixture model


# ----------------------------------------------------------------------------------------------------------------- config mappers
def _vanilla_block(prefix=""):
    ff = NS(device="cuda", weight="./Model/Flowformer_things_kitti.pth")
    return NS(
        name="MACVO_Ablation_vanilla",
        args=NS(device="cuda", edgewidth=32, num_point=200, match_cov_default=0.25, profile=False, mapping=False),
        cov=NS(obs=NS(type=prefix + "NoCovariance", args=None)),
        keypoint=NS(type=prefix + "RandomSelector", args=NS(mask_width=32, device="cuda")),
        mappoint=NS(type=prefix + "MappingPointSelector", args=NS(device="cuda", max_depth=5.0, max_depth_cov=0.005, mask_width=32)),
        frontend=NS(type="FrontendCompose", args=NS(depth=NS(type=prefix + "FlowFormerDepth", args=ff), match=NS(type=prefix + "FlowFormerMatcher", args=ff))),
        motion=NS(type=prefix + "TartanMotionNet", args=NS(weight="./Model/MACVO_posenet.pkl", device="cuda")),
        outlier=NS(type="FilterCompose", args=NS(filter_args=[NS(type="SimpleDepthFilter", args=NS(min_depth=0.05, max_depth="auto"))])),
        postprocess=NS(type="MotionInterpolate", args=None), keyframe=NS(type="AllKeyframe", args=None),
        optimizer=NS(type=prefix + "TwoFrame_PGO", args=NS(device="cpu", vectorize=True, parallel=True, graph_type="icp", autodiff=True)))


def test_config_mappers():
    from macvo_amd import ops
    from macvo_amd.pipeline import (HotPathConfig, cov_config_fields, filter_config_fields, frontend_config_fields, hot_path_config)

    assert HotPathConfig().frontend_cov == (True, True) and HotPathConfig().cov_match_cov_default == 0.25
    for t in ("FlowFormerCovFrontend", "CUDAGraph_FlowFormerCovFrontend", "HIP_FlowFormerCovFrontend", "HIP_CUDAGraph_FlowFormerCovFrontend"):
        assert frontend_config_fields(NS(type=t, args=NS())) == {"frontend_cov": (True, True)}
    for pd in ("", "HIP_"):
        for pm in ("", "HIP_"):
            for dn, dv in (("FlowFormerCovDepth", True), ("FlowFormerDepth", False)):
                for mn, mv in (("FlowFormerCovMatcher", True), ("FlowFormerMatcher", False)):
                    blk = {"type": "FrontendCompose", "args": {"depth": {"type": pd + dn, "args": {}}, "match": {"type": pm + mn, "args": {}}}}
                    assert frontend_config_fields(blk) == {"frontend_cov": (dv, mv)}
    for bad in (NS(type="TartanVOFrontend", args=NS()),
                NS(type="FrontendCompose", args=NS(depth=NS(type="GTDepth", args=NS()), match=NS(type="FlowFormerMatcher", args=NS()))),
                NS(type="FrontendCompose", args=NS(depth=NS(type="FlowFormerDepth", args=NS()), match=NS(type="GTMatcher", args=NS())))):
        with pytest.raises(ValueError):
            frontend_config_fields(bad)

    sd = NS(type="SimpleDepthFilter", args=NS(min_depth=0.1, max_depth="auto"))
    assert filter_config_fields(NS(type="CovarianceSanityFilter", args=NS())) == {"filters": ops.FILTER_COV_SANITY}
    assert filter_config_fields(NS(type="FilterCompose", args=NS(filter_args=[sd]))) == {"filters": ops.FILTER_SIMPLE_DEPTH, "filter_min_depth": 0.1,
                                                                                         "max_depth": "auto"}
    full = NS(type="FilterCompose", args=NS(filter_args=[NS(type="CovarianceSanityFilter", args=None), sd, NS(type="LikelyFrontOfCamFilter", args=None)]))
    assert filter_config_fields(full)["filters"] == 7
    assert filter_config_fields(NS(type="IdentityFilter", args=None)) == {"filters": 0}
    with pytest.raises(ValueError):
        filter_config_fields(NS(type="SomeOtherFilter", args=None))
    with pytest.raises(ValueError):
        filter_config_fields(NS(type="FilterCompose", args=NS(filter_args=[sd, NS(type="SimpleDepthFilter", args=NS(min_depth=0.1, max_depth=50.0))])))

    margs = NS(device="cuda", kernel_size=31, match_cov_default=0.5, min_depth_cov=0.05, min_flow_cov=0.25)
    f = cov_config_fields(NS(type="MatchCovariance", args=margs))
    assert f["cov_match_cov_default"] == 0.5 and f["cov_model"] == "match"
    assert cov_config_fields({"type": "NoCovariance", "args": None}) == {"cov_model": "none", "cov_modifiers": ()}

    for prefix in ("", "HIP_"):
        c = hot_path_config(_vanilla_block(prefix))
        assert c.frontend_cov == (False, False) and c.selector == "random" and c.cov_model == "none" and c.filters == ops.FILTER_SIMPLE_DEPTH
        assert c.graph_type == "icp" and c.motion_model == "tartan" and c.max_depth == "auto" and c.filter_min_depth == 0.05
        assert c.num_point == 200 and c.edgewidth == 32 and c.match_cov_default == 0.25 and c.mapping is False and c.kp_mask_width == 32
    assert hot_path_config(_vanilla_block(), feature_layout="hwc").feature_layout == "hwc"
    blk = _vanilla_block()                      # the selector's bound and the filter's differ: the pipe has one max_depth
    blk.keypoint = NS(type="CovAwareSelector_NoDepth", args=NS(device="cuda", kernel_size=7, mask_width=32, max_depth=40.0, max_match_cov=100.0))
    blk.frontend = NS(type="FlowFormerCovFrontend", args=NS())
    with pytest.raises(ValueError, match="max_depth"):
        hot_path_config(blk)
    blk.keypoint.args.max_depth = "auto"
    assert hot_path_config(blk).selector == "nodepth"
    blk = _vanilla_block()                      # a half-written mappoint block raises like the sibling mappers; an absent one is tolerated
    del blk.mappoint.args.max_depth_cov
    with pytest.raises(ValueError, match="max_depth_cov"):
        hot_path_config(blk)
    del blk.mappoint
    assert hot_path_config(blk).map_max_depth == 5.0
    blk = _vanilla_block()                      # what the mappers accept one by one, hot_path_config refuses as a whole
    blk.optimizer.args.graph_type = "reproj"
    with pytest.raises(ValueError, match="match"):
        hot_path_config(blk)


REFUSED = [   # (frontend_cov, HotPathConfig fields, a word of the message)
    ((False, True), dict(selector="full"), "depth"), ((False, True), dict(mapping=True), "depth"), ((False, True), dict(cov_model="gmm"), "depth"),
    ((False, True), dict(graph_type="disp"), "depth"), ((True, False), dict(selector="nodepth", graph_type="icp"), "match"),
    ((True, False), dict(selector="full", graph_type="icp"), "match"), ((True, False), dict(selector="random", graph_type="reproj"), "match"),
    ((True, False), dict(selector="random", graph_type="disp"), "match"), ((False, False), dict(selector="random", graph_type="disp"), "cov"),
    ((False, False), dict(selector="nodepth", graph_type="icp"), "match"), ((False, False), dict(selector="random", graph_type="icp", cov_model="gmm"), "depth"),
]
ACCEPTED = [((False, False), dict(selector="random", graph_type="icp", cov_model="none")), ((False, False), dict(selector="grid", graph_type="icp")),
            ((True, False), dict(selector="explicit", graph_type="icp", cov_model="gmm")), ((False, True), dict(selector="nodepth", graph_type="reproj")),
            ((False, True), dict(selector="nodepth", graph_type="icp", cov_modifiers=("diag",))), ((True, True), dict(selector="full", graph_type="disp", mapping=True))]


def test_python_refusals_name_the_missing_covariance():
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath, check_frontend_cov

    cam = Camera(320.0, 320.0, 320.0, 240.0, 0.25, 480, 640)
    for fc, kw, word in REFUSED:
        cfg = HotPathConfig(frontend_cov=fc, **kw)
        with pytest.raises(ValueError, match=word):
            check_frontend_cov(cfg)
        with pytest.raises(ValueError, match="provides no covariance"):
            NativeHotPath(cam, cfg)                                               # at configuration time, before any GPU work
    for fc, kw in ACCEPTED:
        check_frontend_cov(HotPathConfig(frontend_cov=fc, **kw))
    with pytest.raises(ValueError):
        check_frontend_cov(HotPathConfig(frontend_cov=(True,)))
    with pytest.raises(ValueError):
        check_frontend_cov(HotPathConfig(frontend_cov=(True, False), selector="random", graph_type="icp", cov_match_cov_default=0.0))


def test_c_abi_refusals_and_append_only_config():
    from macvo_amd import _lib as L
    from macvo_amd import ops

    lib = L.load()
    assert lib.mv_abi_version() == L.ABI_VERSION == 8
    assert (L.MV_NOCOV_DEPTH, L.MV_NOCOV_MATCH) == (1, 2)
    for sym in ("mv_obs_cov_pair_nomatch_lanes", "mv_frontend_epilogue", "mv_frontend_epilogue_lanes", "mv_frame_pipe_create", "mv_frame_pipe_buffer"):
        assert getattr(lib, sym) is not None
    names = [f[0] for f in L.mvFramePipeConfig._fields_]
    assert names[-2:] == ["frontend_nocov", "cov_match_cov_default"] and names[-3] == "motion_model"      # appended behind what was the last field
    lm = L.mvLMParams()
    lib.mv_lm_default_params(C.byref(lm))
    sel = {"nodepth": L.MV_KP_NODEPTH, "full": L.MV_KP_FULL, "random": L.MV_KP_RANDOM, "grid": L.MV_KP_GRID, "explicit": L.MV_KP_EXPLICIT}

    def size(fc=(True, True), selector="nodepth", graph_type="disp", cov_model="match", mapping=False, cov_match_cov_default=0.25, **kw):
        d = dict(H=480, W=640, C=256, pairs=2, iters=12, radius=4, feat_dtype=L.MV_F32, layout=L.MV_LAYOUT_CHW, volume_split=0,
                 selector_mode=sel[selector], kp_kernel_size=7, kp_mask_width=32, num_point=200, edgewidth=32, min_num_point=10,
                 graph_type=ops._GRAPH[graph_type], filters=1, cov_kernel_size=31, fx=320.0, fy=320.0, cx=320.0, cy=240.0, baseline=0.25, bl_fx=80.0,
                 bl_fx_sq=6400.0, match_cov_default=0.25, max_match_cov=100.0, max_depth_cov=250.0, max_depth=80.0, min_flow_cov_sq=0.0625,
                 min_depth_cov=0.05, filter_min_depth=0.05, map_max_depth=5.0, map_max_depth_cov=0.005, lm=lm, cov_model=ops.COV_MODELS[cov_model],
                 mapping=int(mapping), map_num_point=2000, map_mask_width=32,
                 frontend_nocov=(0 if fc[0] else L.MV_NOCOV_DEPTH) | (0 if fc[1] else L.MV_NOCOV_MATCH), cov_match_cov_default=cov_match_cov_default)
        d.update(kw)
        return lib.mv_frame_pipe_arena_bytes(C.byref(L.mvFramePipeConfig(**d)))

    base = size()
    assert base > 0 and size(cov_match_cov_default=0.0) == base                   # zero-initialised new fields = the configuration as it was
    for fc, kw, _ in REFUSED:
        kw = {k: v for k, v in kw.items()}
        assert size(fc, **kw) == 0, (fc, kw)
    for fc, kw in ACCEPTED:
        kw = {k: v for k, v in kw.items() if k != "cov_modifiers"}
        assert size(fc, **kw) > 0, (fc, kw)
    assert size((True, False), selector="random", graph_type="icp", cov_match_cov_default=0.0) == 0
    assert size((True, True), frontend_nocov=4) == 0
    # a missing covariance map is not carved: 2 planes per map slot for the depth side, 3 for the match side
    full, no_d, no_m, none = (size(fc, selector="random", graph_type="icp") for fc in ((True, True), (False, True), (True, False), (False, False)))
    assert full > no_d > none and full > no_m > none and (full - no_m) > (full - no_d)


# ----------------------------------------------------------------------------------------------------------------- against the reference tree
YAML_SCRIPT = r'''
import sys, glob
from pathlib import Path
sys.path.insert(0, %(root)r)
from tests import refrun
ref = refrun.import_reference()
import Module
import macvo_amd.plugins as P
from macvo_amd import ops
from macvo_amd.pipeline import hot_path_config, HotPathConfig
from Utility.Config import load_config
for name, base in (("HIP_FlowFormerDepth", Module.IStereoDepth), ("HIP_FlowFormerMatcher", Module.IMatcher)):
    cls = base.get_class(name)
    assert cls is getattr(P, name) and issubclass(cls, base), name
exp = Path(%(ref)r) / "Config/Experiment/MACVO"
files = sorted(glob.glob(str(exp / "Ablation_Study/*.yaml"))) + [str(exp / n) for n in ("Paper_Reproduce.yaml", "MACVO_Fast.yaml", "MACVO_Performant.yaml")]
assert len(files) >= 12
seen = {}
for f in files:
    cfg, _ = load_config(Path(f))
    c = hot_path_config(cfg.Odometry)
    assert isinstance(c, HotPathConfig)
    seen[Path(f).name] = c
v = seen["TartanAirv2_Vanilla.yaml"]
assert v.frontend_cov == (False, False) and v.selector == "random" and v.cov_model == "none" and v.filters == ops.FILTER_SIMPLE_DEPTH
assert v.graph_type == "icp" and v.motion_model == "tartan"
assert all(c.frontend_cov == (True, True) for n, c in seen.items() if n != "TartanAirv2_Vanilla.yaml")
assert seen["Paper_Reproduce.yaml"].filters == 7 and seen["MACVO_Fast.yaml"].mapping is True

# the Vanilla YAML with only its type: strings swapped to the HIP_* plugins, through the reference's own validator
cfg, _ = load_config(exp / "Ablation_Study/TartanAirv2_Vanilla.yaml")
od = cfg.Odometry
for node in (od.cov.obs, od.keypoint, od.mappoint, od.frontend.args.depth, od.frontend.args.match, od.motion, od.optimizer):
    node.type = "HIP_" + node.type
ref.OM.MACVO.is_valid_config(od)
c = hot_path_config(od)
assert c.frontend_cov == (False, False) and c.selector == "random" and c.cov_model == "none"
print("COVFREE_YAML_OK", len(files))
'''


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "Module")), reason="needs the reference checkout (build container only)")
def test_every_experiment_yaml_maps_and_vanilla_validates_with_hip_types(tmp_path):
    script = tmp_path / "yamls.py"
    script.write_text(YAML_SCRIPT % {"root": ROOT, "ref": REF})
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0 and "COVFREE_YAML_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.skipif(refrun.reference_root() is None or not os.path.isdir(os.path.join(REF, "Module")),
                    reason="needs the reference checkout (build container only)")
def test_generator_regenerates_the_golden(tmp_path, gold):
    """Same reference code, same exact-arithmetic inputs (fp64 LAPACK / libm may differ in the last bits between hosts)."""
    script = tmp_path / "regen.py"
    script.write_text("import sys, numpy as np\nsys.path.insert(0, %r)\nfrom tests.golden import make_golden_covfree as G\nfrom tests import refrun\n"
                      "ref = refrun.import_reference()\nfrom Utility.PrettyPrint import GlobalConsole\nGlobalConsole.quiet = True\n"
                      "cam, maps, poses = refrun.tartanair_maps()\nG.define_replay_modules(ref, maps)\n"
                      "r = G.run_case(ref, cam, maps, poses, G.CASES['vanilla'])\nnp.savez(sys.argv[1], **{k.replace('/', '|'): v for k, v in r.items()})\n"
                      % ROOT)
    out = tmp_path / "vanilla.npz"
    p = subprocess.run([sys.executable, str(script), str(out)], capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    z = np.load(out)
    run = {k.replace("|", "/"): z[k] for k in z.files}
    g = case(gold, "vanilla")
    for k, v in g.items():
        if v.dtype.kind == "f" and (k.endswith("covTc") or k.endswith("cov_Tw") or k.endswith("pos_Tw") or k.endswith("pose") or k == "poses_npy"):
            assert np.allclose(v, run[k], rtol=1e-6, atol=1e-6), k
        else:
            assert np.array_equal(v, run[k]), k
