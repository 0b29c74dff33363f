"""Writes tests/golden/covfree.npz: the reference's OWN, unmodified ``Odometry/MACVO.py`` loop (``tests/refrun``: ``from_config`` ->
``receive_frames`` -> ``run_pair``) with frontends that lack covariances — ``FrontendCompose`` of a replaying ``IStereoDepth`` / ``IMatcher``
pair whose ``provide_cov`` is (d, m) ∈ {(0,0), (1,0), (0,1)}; (0,0) is ``Config/Experiment/MACVO/Ablation_Study/TartanAirv2_Vanilla.yaml`` —
on the reference's unit-test TartanAir asset (``tests/refrun.tartanair_maps``), every module the reference's class on the CPU.  The replaying
modules do what ``FlowFormer[Cov]Depth`` / ``FlowFormer[Cov]Matcher`` do behind the network (StereoDepth.py:121-128,168-175, Matching.py:142-147,
188-193) with the reference's own ``disparity_to_depth(_cov)`` / ``from_partial_cov``.  Plus direct calls of ``MatchCovariance`` /
``GaussianMixtureCovariance.estimate`` with ``flow_cov=None``.

The covariance model's ``match_cov_default`` is 0.5, ``Odometry.args.match_cov_default`` 0.25: the two cannot be confused.  Every frame of
every case must be solved (no ``need_interp``, >= ``min_num_point`` observations), so no consumer can pass by skipping the solve.

Build-container only (needs the reference checkout):

    python tests/golden/make_golden_covfree.py
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import refrun  # noqa: E402

SEED = 1234
MODEL_MATCH_COV_DEFAULT = 0.5          # cov.obs args (the second observation's sigma when the matcher gives none)
ODOM_MATCH_COV_DEFAULT = 0.25          # Odometry.args (the first observation's sigma)
MIN_NUM_POINT = 10                     # MACVO.py:64

# name -> (depth provides cov, matcher provides cov, selector, covariance model, outlier block, graph)
CASES = {
    "vanilla":        (0, 0, "RandomSelector", "NoCovariance", "vanilla", "icp"),       # TartanAirv2_Vanilla.yaml
    "00_grid_match":  (0, 0, "GridSelector", "MatchCovariance", "compose", "icp"),
    "00_rand_match":  (0, 0, "RandomSelector", "MatchCovariance", "vanilla", "icp"),
    "10_rand_match":  (1, 0, "RandomSelector", "MatchCovariance", "compose", "icp"),
    "10_grid_none":   (1, 0, "GridSelector", "NoCovariance", "vanilla", "icp"),
    "01_rand_match":  (0, 1, "RandomSelector", "MatchCovariance", "compose", "icp"),
    "01_grid_match":  (0, 1, "GridSelector", "MatchCovariance", "vanilla", "icp"),
    "01_nodepth_reproj": (0, 1, "CovAwareSelector_NoDepth", "MatchCovariance", "compose", "reproj"),
}
# what a case keeps of tensor_map.npz (the colour / camera rows and the edge tables other than the frame ranges are pinned by macvo_run.npz already)
KEEP = ("map/frames//pose", "map/frames//need_interp", "map/points//pos_Tw", "map/points//cov_Tw", "map/edge/frame2match/ranges")


def _frame_index(img: torch.Tensor) -> int:
    return int(round(float(img[0, 0, 0, 0]) * 255.0))


def define_replay_modules(ref, maps):
    """``IStereoDepth`` / ``IMatcher`` classes (registered by subclassing) that replay the stored network outputs of the frame whose index is
    encoded in pixel (0, 0) of the left image (refrun.make_stereo_frames)."""
    from Module.Frontend.Matching import IMatcher
    from Module.Frontend.StereoDepth import IStereoDepth, disparity_to_depth, disparity_to_depth_cov

    class CovFreeReplayDepth(IStereoDepth):
        @property
        def provide_cov(self): return bool(self.config.provide_cov)

        def estimate(self, frame):
            f = maps[_frame_index(frame.imageL)]
            disparity = f["flow"][0:1, 0:1].abs()
            depth = disparity_to_depth(disparity, frame.frame_baseline, frame.fx)
            if not self.provide_cov:
                return IStereoDepth.Output(depth=depth, disparity=disparity)                       # FlowFormerDepth (StereoDepth.py:127-128)
            dcov = f["cov"][0:1, 0:1].clone()
            return IStereoDepth.Output(depth=depth, cov=disparity_to_depth_cov(disparity, dcov, frame.frame_baseline, frame.fx),
                                       disparity=disparity, disparity_uncertainty=dcov)           # FlowFormerCovDepth (:168-175)

        @classmethod
        def is_valid_config(cls, config): return

    class CovFreeReplayMatcher(IMatcher):
        @property
        def provide_cov(self): return bool(self.config.provide_cov)

        def forward(self, frame_t1, frame_t2):
            f = maps[_frame_index(frame_t2.imageL)]
            flow = f["flow"][1:2].clone()
            if not self.provide_cov:
                return IMatcher.Output(flow=flow)                                                  # FlowFormerMatcher (Matching.py:147)
            return IMatcher.Output.from_partial_cov(flow=flow, cov=f["cov"][1:2].clone())          # FlowFormerCovMatcher (:188-193)

        @classmethod
        def is_valid_config(cls, config): return

    return CovFreeReplayDepth, CovFreeReplayMatcher


def make_config(d: int, m: int, selector: str, cov: str, outlier: str, graph: str):
    dev = "cpu"
    if selector == "CovAwareSelector_NoDepth":
        kp = NS(type=selector, args=NS(device=dev, kernel_size=7, mask_width=32, max_match_cov=100.0))
    else:
        kp = NS(type=selector, args=NS(device=dev, mask_width=32))
    if cov == "NoCovariance":
        obs = NS(type="NoCovariance", args=None)
    else:
        obs = NS(type="MatchCovariance", args=NS(device=dev, kernel_size=31, match_cov_default=MODEL_MATCH_COV_DEFAULT, min_depth_cov=0.05, min_flow_cov=0.25))
    depth_filter = NS(type="SimpleDepthFilter", args=NS(min_depth=0.05, max_depth="auto"))
    if outlier == "vanilla":       # TartanAirv2_Vanilla.yaml
        out = NS(type="FilterCompose", args=NS(filter_args=[depth_filter]))
    elif outlier == "compose":     # Paper_Reproduce.yaml
        out = NS(type="FilterCompose", args=NS(filter_args=[NS(type="CovarianceSanityFilter", args=NS()), depth_filter,
                                                             NS(type="LikelyFrontOfCamFilter", args=NS())]))
    else:
        out = NS(type="CovarianceSanityFilter", args=NS())
    od = NS(
        name="covfree",
        args=NS(device=dev, edgewidth=32, num_point=200, match_cov_default=ODOM_MATCH_COV_DEFAULT, profile=False, mapping=False),
        cov=NS(obs=obs),
        keypoint=kp,
        mappoint=NS(type="MappingPointSelector", args=NS(max_depth=5.0, max_depth_cov=0.005, mask_width=32)),
        frontend=NS(type="FrontendCompose", args=NS(depth=NS(type="CovFreeReplayDepth", args=NS(provide_cov=bool(d))),
                                                    match=NS(type="CovFreeReplayMatcher", args=NS(provide_cov=bool(m))))),
        motion=NS(type="StaticMotionModel", args=NS()),
        outlier=out,
        postprocess=NS(type="MotionInterpolate", args=NS()),
        keyframe=NS(type="AllKeyframe", args=NS()),
        optimizer=NS(type="TwoFrame_PGO", args=NS(device=dev, vectorize=True, parallel=False, graph_type=graph, autodiff=False)),
    )
    return NS(Odometry=od)


def run_case(ref, cam, maps, poses, spec) -> dict:
    frames = refrun.make_stereo_frames(ref, cam, maps, poses)
    cfg = make_config(*spec)
    ref.OM.MACVO.is_valid_config(cfg.Odometry)
    torch.manual_seed(SEED)
    system = ref.OM.MACVO.from_config(cfg)
    assert tuple(system.Frontend.provide_cov) == (bool(spec[0]), bool(spec[1]))
    with tempfile.TemporaryDirectory() as tmp:
        box = ref.Sandbox(Path(tmp))
        system.receive_frames(frames, box)
        assert system.terminated and os.path.exists(box.path("tensor_map.npz")), "receive_frames swallowed an exception"
        tm = dict(np.load(box.path("tensor_map.npz")))
        out = {f"map/{k}": v for k, v in tm.items()}
        out["poses_npy"] = np.load(box.path("poses.npy"))
    return out


def direct_calls(ref, cam, maps) -> dict:
    """``estimate(..., flow_cov=None)`` of both patch models, with and without ``depth_cov``, on frame 1's depth maps at 64 integer keypoints."""
    from Module.Covariance import Project2to3 as P23
    from Module.Frontend.StereoDepth import disparity_to_depth, disparity_to_depth_cov

    f = maps[1]
    disparity = f["flow"][0:1, 0:1].abs()
    depth = disparity_to_depth(disparity, cam["baseline"], cam["fx"])
    dcov = disparity_to_depth_cov(disparity, f["cov"][0:1, 0:1], cam["baseline"], cam["fx"])
    g = torch.Generator().manual_seed(7)
    kp = torch.stack([torch.randint(32, cam["W"] - 32, (64,), generator=g), torch.randint(32, cam["H"] - 32, (64,), generator=g)], dim=1)
    dc = dcov[0, 0, kp[:, 1], kp[:, 0]].contiguous()
    frame = NS(fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"])
    args = dict(kernel_size=31, match_cov_default=MODEL_MATCH_COV_DEFAULT, min_flow_cov=0.25, min_depth_cov=0.05)
    mc = P23.MatchCovariance(NS(device="cpu", **args))
    gm = P23.GaussianMixtureCovariance(NS(**args))
    with_cov, without = NS(depth=depth, cov=dcov), NS(depth=depth, cov=None)
    return {"direct/kp": kp.numpy(), "direct/depth_cov_kp": dc.numpy(),
            "direct/match_nodepthcov": mc.estimate(frame, kp, without, None, None).numpy(),
            "direct/match_depthcov": mc.estimate(frame, kp, with_cov, dc.clone(), None).numpy(),
            "direct/gmm_nodepthcov_arg": gm.estimate(frame, kp, with_cov, None, None).numpy(),
            "direct/gmm_depthcov": gm.estimate(frame, kp, with_cov, dc.clone(), None).numpy()}


def main():
    assert os.path.isdir("/root/reference/Odometry") or os.environ.get("MACVO_REFERENCE_ROOT"), "runs in the build container (needs the reference checkout)"
    ref = refrun.import_reference()
    from Utility.PrettyPrint import GlobalConsole
    GlobalConsole.quiet = True
    cam, maps, poses = refrun.tartanair_maps()
    define_replay_modules(ref, maps)
    out = {"meta": np.array(json.dumps(dict(cases={k: list(v) for k, v in CASES.items()}, seed=SEED, model_match_cov_default=MODEL_MATCH_COV_DEFAULT,
                                            odom_match_cov_default=ODOM_MATCH_COV_DEFAULT)))}
    for name, spec in CASES.items():
        r = run_case(ref, cam, maps, poses, spec)
        ranges = r["map/edge/frame2match/ranges"]
        per_frame = [int(ranges[t, 0, 1]) for t in range(1, len(maps))]
        assert not r["map/frames//need_interp"].any(), (name, "need_interp")
        assert min(per_frame) >= MIN_NUM_POINT, (name, per_frame)
        d, m = spec[0], spec[1]
        if not d:
            for k in ("pixel1_d_cov", "pixel2_d_cov", "pixel1_disp_cov", "pixel2_disp_cov"):
                assert (r[f"map/match//{k}"] == -1).all(), (name, k)
        if not m:
            assert (r["map/match//pixel2_uv_cov"] == -1).all(), name
        for k, v in r.items():
            if k.startswith("map/match//") or k in KEEP or k == "poses_npy":
                out[f"{name}/{k}"] = v
        print(name, "observations per frame", per_frame)
    out.update(direct_calls(ref, cam, maps))
    path = os.path.join(ROOT, "tests", "golden", "covfree.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= 512 * 1024, size


if __name__ == "__main__":
    main()
