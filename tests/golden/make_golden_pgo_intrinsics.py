"""Writes tests/golden/pgo_intrinsics.npz: the reference's ``TwoFrame_PGO._optimize`` (Module/Optimization/TwoFramePGO/Optimizer.py:81-102) and
``Local_TwoFrame_PGO`` (:111-150), executed unmodified on ``tests/golden/pypose_shim.py``, on cameras that are not fx = fy = 320 (tests/cameras.py).

world cases   ``oracle.pgo.make_synthetic_problem(K=..., baseline=..., W=..., H=..., **case)`` for EUROC, KITTI, ANISO x icp, reproj, disp x four cases,
              ``STOP_ON_REJECT = 1``: per case the fp64 pose and [steps, reject_count, loss, max reject].  The problems are regenerated from the seed by the
              tests (as for pgo.npz); the parameters, camera included, are in the JSON string ``meta``.
local cases   the first ``LOCAL_CASES`` move of make_golden_local_keyframe.py applied to the ANISO seed = 6 problem, three graphs, in the layout of
              local_pgo.npz (keys ``c0/...``) so that the readers of that file read this one.

Build-container only (needs the reference checkout):

    python tests/golden/make_golden_pgo_intrinsics.py
"""
from __future__ import annotations

import json
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import cameras, refrun  # noqa: E402
from tests.golden import make_golden_local_keyframe as MLK  # noqa: E402

GRAPHS = MLK.GRAPHS
CAMERAS = ("EUROC", "KITTI", "ANISO")
CASES = [dict(n=200, seed=6), dict(n=37, seed=8), dict(n=120, seed=10, trans_sigma=0.4, rot_sigma=0.08), dict(n=200, seed=7, outlier_frac=0.1)]
LOCAL_CAMERA, LOCAL_CASE, LOCAL_MOVE, LOCAL_REF = "ANISO", MLK.LOCAL_CASES[0][0], MLK.LOCAL_CASES[0][1], MLK.LOCAL_CASES[0][2]


def camera_kwargs(name):
    c = cameras.BY_NAME[name]
    return dict(K=c.K, baseline=c.baseline, W=c.W, H=c.H)


def main():
    assert os.path.isdir("/root/reference/Odometry") or os.environ.get("MACVO_REFERENCE_ROOT"), "runs in the build container (needs the reference checkout)"
    refrun.import_reference()
    from oracle import pgo as opgo
    from tests.golden import pypose_shim as S
    import Module.Optimization.TwoFramePGO.Graphs as GR
    import Module.Optimization.TwoFramePGO.Optimizer as OPT

    pp = sys.modules["pypose"]
    SOP = S.StopOnPlateau
    SOP.STOP_ON_REJECT = 1
    raw = lambda t: t.detach().as_subclass(torch.Tensor)  # noqa: E731
    meta = dict(graphs=GRAPHS, cameras={n: camera_kwargs(n) for n in CAMERAS}, cases=CASES,
                local=dict(camera=LOCAL_CAMERA, case=LOCAL_CASE, move=list(LOCAL_MOVE), ref=LOCAL_REF))
    out = {"meta": np.array(json.dumps(meta))}
    # ---- world frame
    for cname in CAMERAS:
        for ci, c in enumerate(CASES):
            prob, _ = opgo.make_synthetic_problem(**camera_kwargs(cname), **c)
            for gname in GRAPHS:
                ctx = OPT.TwoFrame_PGO.init_context(NS(graph_type=gname, device="cpu", vectorize=True, parallel=False, autodiff=False))
                _, gout = OPT.TwoFrame_PGO._optimize(ctx, MLK._graph_input(GR, pp, prob, prob.init_pose))
                sch = SOP.last_instance
                out[f"{cname}/{gname}/{ci}/pose"] = raw(gout.motion).reshape(7).double().clone()
                out[f"{cname}/{gname}/{ci}/stats"] = np.array([sch.steps, sch.optimizer.reject_count, float(sch.optimizer.loss), max(sch.reject_hist)],
                                                              dtype=np.float64)
                print(f"{cname} case {ci} {gname}: steps {sch.steps} rejects {sch.optimizer.reject_count} (max {max(sch.reject_hist)}) loss {float(sch.optimizer.loss):.9g}")
    # ---- local frame (gen_local_pgo of make_golden_local_keyframe.py, one case)
    prob, _ = opgo.make_synthetic_problem(**camera_kwargs(LOCAL_CAMERA), **LOCAL_CASE)
    move = pp.SE3(MLK._move_pose(pp, LOCAL_MOVE))
    R = move.rotation().matrix().double()
    prob.init_pose = raw(move @ pp.SE3(prob.init_pose.float()))
    prob.pos_Tw = raw(move.Act(prob.pos_Tw.float()))
    prob.cov_Tw = R @ prob.cov_Tw @ R.transpose(-1, -2)
    assert LOCAL_REF is None
    ref_pose = prob.init_pose.clone()
    out["c0/move"], out["c0/ref_pose"] = raw(move), ref_pose
    for k in ("init_pose", "pos_Tw", "cov_Tw", "pixel2_uv", "pixel2_d", "pixel2_disp", "pixel2_disp_cov", "pixel2_uv_cov", "obs2_covTc", "K"):
        out[f"c0/{k}"] = getattr(prob, k)
    out["c0/baseline"] = np.array(prob.baseline, dtype=np.float32)
    for gname in GRAPHS:
        ctx = OPT.TwoFrame_PGO.init_context(NS(graph_type=gname, device="cpu", vectorize=True, parallel=False, autodiff=False))
        _, gout = OPT.TwoFrame_PGO._optimize(ctx, MLK._graph_input(GR, pp, prob, prob.init_pose))
        world_f32 = raw(gout.motion).reshape(7).double().float()
        T_o2w = pp.SE3(ref_pose.reshape(1, 7).clone())
        gin = OPT.Local_TwoFrame_PGO.world_to_optim(None, MLK._graph_input(GR, pp, prob, prob.init_pose), T_o2w.Inv())
        stage = {"T_c2o": raw(gin.init_motion).reshape(7).clone(), "pos_To": gin.points.data["pos_Tw"].clone(), "cov_To": gin.points.data["cov_Tw"].clone()}
        _, gout = OPT.TwoFrame_PGO._optimize(ctx, gin)
        sch = SOP.last_instance
        stage["pose_local"] = raw(gout.motion).reshape(7).double().clone()
        stage["stats"] = np.array([sch.steps, sch.optimizer.reject_count, float(sch.optimizer.loss), max(sch.reject_hist)], dtype=np.float64)
        gout = OPT.Local_TwoFrame_PGO.optim_to_world(None, gout, T_o2w)
        stage["pose_world_f32"] = raw(gout.motion).reshape(7).clone()
        stage["world_solve_f32"] = world_f32
        print(f"local {gname}: steps {sch.steps} rejects {sch.optimizer.reject_count}")
        for k, v in stage.items():
            if k in ("pos_To", "cov_To") and gname != GRAPHS[0]:
                assert np.array_equal(np.asarray(v), out[f"c0/{GRAPHS[0]}/{k}"])     # graph-independent: stored once
                continue
            out[f"c0/{gname}/{k}"] = np.asarray(v)
    MLK._save("pgo_intrinsics", out)


if __name__ == "__main__":
    main()
