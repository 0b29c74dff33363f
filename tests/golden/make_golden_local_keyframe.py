"""Writes tests/golden/local_pgo.npz and tests/golden/keyframe_run.npz: the reference's ``Local_TwoFrame_PGO`` (Module/Optimization/TwoFramePGO/
Optimizer.py:111-150) and ``UniformKeyframe`` (Module/KeyframeSelector.py:31-39, Odometry/MACVO.py:177-179), executed unmodified on
``tests/golden/pypose_shim.py``.

``local_pgo.npz``  direct calls ``world_to_optim`` -> ``TwoFrame_PGO._optimize`` -> ``optim_to_world`` on seeded problems of
                   ``oracle.pgo.make_synthetic_problem`` that have been moved rigidly about 1500 m away from the origin (with a rotation), so that a
                   solve in the local frame and one in the world frame differ by more than fp32 noise: the script asserts >= 1e-3 m in every case.
``keyframe_run.npz``  the reference's own loop (``tests/refrun``) with ``AllKeyframe`` / ``UniformKeyframe`` and both optimizers.

Build-container only (needs the reference checkout):

    python tests/golden/make_golden_local_keyframe.py [local_pgo] [keyframe_run]
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

GRAPHS = ("icp", "reproj", "disp")
# (problem of oracle.pgo.make_synthetic_problem, rigid move [tx ty tz | axis-angle], ref_pose = move @ Exp(this) @ init_pose or None: ref_pose = init_pose)
# case 3 is one of make_golden.py's reject-loop cases (bad prior: rejections in the first LM step)
LOCAL_CASES = [
    (dict(n=200, seed=6), (1500.0, -900.0, 300.0, 0.7, -0.6, 0.6), None),
    (dict(n=37, seed=8), (-1100.0, 1000.0, -450.0, -0.4, 0.9, 0.3), None),
    (dict(n=120, seed=10, trans_sigma=0.4, rot_sigma=0.08), (900.0, 1200.0, 600.0, 0.2, 0.3, -1.0), (0.3, -0.2, 0.1, 0.02, 0.01, -0.03)),
    (dict(n=60, seed=12, trans_sigma=2.0, rot_sigma=0.5), (1500.0, -900.0, 300.0, 0.7, -0.6, 0.6), None),
    (dict(n=200, seed=7, outlier_frac=0.1), (-1300.0, -700.0, 500.0, 1.0, 0.2, 0.4), (-0.5, 0.4, 0.2, -0.03, 0.02, 0.01)),
]
MIN_LOCAL_WORLD_DIFF = 1e-3     # m

MIN_NUM_POINT = 10              # MACVO.py:64
SEED = 1234
# name -> (refrun case, repeats of the 4-frame fixture, keyframe block, optimizer type, graph)
KEYFRAME_CASES = {
    "all_local_icp":    ("tartan_icp", 1, ("AllKeyframe", None), "Local_TwoFrame_PGO", "icp"),
    "all_local_reproj": ("tartan_reproj", 1, ("AllKeyframe", None), "Local_TwoFrame_PGO", "reproj"),
    "all_local_disp":   ("tartan_fast", 1, ("AllKeyframe", None), "Local_TwoFrame_PGO", "disp"),
    "u2_world_icp":     ("tartan_icp", 3, ("UniformKeyframe", 2), "TwoFrame_PGO", "icp"),
    "u2_local_icp":     ("tartan_icp", 3, ("UniformKeyframe", 2), "Local_TwoFrame_PGO", "icp"),
    "u3_world_icp":     ("tartan_icp", 3, ("UniformKeyframe", 3), "TwoFrame_PGO", "icp"),
    "u3_local_icp":     ("tartan_icp", 3, ("UniformKeyframe", 3), "Local_TwoFrame_PGO", "icp"),
    "u3_local_disp":    ("tartan_fast", 3, ("UniformKeyframe", 3), "Local_TwoFrame_PGO", "disp"),
}
KEEP = ("map/frames//pose", "map/frames//need_interp", "map/points//pos_Tw", "map/points//cov_Tw", "map/edge/frame2match/ranges")   # = make_golden_covfree.KEEP


# ------------------------------------------------------------------------------------------------------------ local_pgo.npz
def _move_pose(pp, six) -> torch.Tensor:
    """[tx ty tz | axis-angle] -> SE3 [7] fp32 (translation as given, rotation = so3 Exp)"""
    from tests.golden import pypose_shim as S

    q = S._so3_exp(torch.tensor(six[3:], dtype=torch.float64)).float()
    return torch.cat([torch.tensor(six[:3], dtype=torch.float32), q])


def _graph_input(GR, pp, prob, init_pose):
    obs = NS(data={"pixel2_uv": prob.pixel2_uv, "pixel2_d": prob.pixel2_d, "pixel2_disp": prob.pixel2_disp, "pixel2_disp_cov": prob.pixel2_disp_cov,
                   "pixel2_uv_cov": prob.pixel2_uv_cov, "obs2_covTc": prob.obs2_covTc})
    pts = NS(data={"pos_Tw": prob.pos_Tw.clone(), "cov_Tw": prob.cov_Tw.clone()})
    n = prob.pos_Tw.shape[0]
    return GR.GraphInput(frame_idx=torch.tensor([1]), from_idx=torch.tensor([0]), init_motion=pp.SE3(init_pose.reshape(1, 7).clone()),
                         baseline=torch.tensor([prob.baseline], dtype=torch.float32), observations=obs, points=pts, images_intrinsic=prob.K,
                         edges_index=torch.zeros(n, dtype=torch.long), device="cpu")


def gen_local_pgo():
    from oracle import pgo as opgo
    from tests.golden import pypose_shim as S
    import Module.Optimization.TwoFramePGO.Graphs as GR
    import Module.Optimization.TwoFramePGO.Optimizer as OPT

    pp = sys.modules["pypose"]
    SOP = S.StopOnPlateau
    SOP.STOP_ON_REJECT = 1
    raw = lambda t: t.detach().as_subclass(torch.Tensor)  # noqa: E731
    out = {"meta": np.array(json.dumps(dict(cases=[[c, list(m), None if r is None else list(r)] for c, m, r in LOCAL_CASES], graphs=GRAPHS)))}
    for ci, (c, move6, ref6) in enumerate(LOCAL_CASES):
        prob, _ = opgo.make_synthetic_problem(**c)
        move = pp.SE3(_move_pose(pp, move6))
        # the same problem seen from the moved world: T' = M @ T, p' = M p, S' = R S R^T
        R = move.rotation().matrix().double()
        prob.init_pose = raw(move @ pp.SE3(prob.init_pose.float()))
        prob.pos_Tw = raw(move.Act(prob.pos_Tw.float()))
        prob.cov_Tw = R @ prob.cov_Tw @ R.transpose(-1, -2)
        if ref6 is None:
            ref_pose = prob.init_pose.clone()
        else:
            e = S.LieTensor(torch.tensor(ref6, dtype=torch.float32), ltype="se3").Exp()
            ref_pose = raw(pp.SE3(prob.init_pose) @ e)
        out[f"c{ci}/move"] = raw(move)
        out[f"c{ci}/ref_pose"] = ref_pose
        for k in ("init_pose", "pos_Tw", "cov_Tw", "pixel2_uv", "pixel2_d", "pixel2_disp", "pixel2_disp_cov", "pixel2_uv_cov", "obs2_covTc", "K"):
            out[f"c{ci}/{k}"] = getattr(prob, k)
        out[f"c{ci}/baseline"] = np.array(prob.baseline, dtype=np.float32)
        for gname in GRAPHS:
            cfg = NS(graph_type=gname, device="cpu", vectorize=True, parallel=False, autodiff=False)
            ctx = OPT.TwoFrame_PGO.init_context(cfg)
            # the world-frame solve of the same problem (TwoFrame_PGO), pose = motion.float() (Optimizer.py:107-108)
            _, gout = OPT.TwoFrame_PGO._optimize(ctx, _graph_input(GR, pp, prob, prob.init_pose))
            world_f32 = raw(gout.motion).reshape(7).double().float()
            # Local_TwoFrame_PGO.get_graph_data (:121-123) -> _optimize -> write_graph_data (:128-129)
            T_o2w = pp.SE3(ref_pose.reshape(1, 7).clone())
            gin = OPT.Local_TwoFrame_PGO.world_to_optim(None, _graph_input(GR, pp, prob, prob.init_pose), T_o2w.Inv())
            stage = {"T_c2o": raw(gin.init_motion).reshape(7).clone(), "pos_To": gin.points.data["pos_Tw"].clone(),
                     "cov_To": gin.points.data["cov_Tw"].clone()}
            assert stage["T_c2o"].dtype == torch.float32 and stage["pos_To"].dtype == torch.float32 and stage["cov_To"].dtype == torch.float64
            _, gout = OPT.TwoFrame_PGO._optimize(ctx, gin)
            sch = SOP.last_instance
            stage["pose_local"] = raw(gout.motion).reshape(7).double().clone()
            stage["stats"] = np.array([sch.steps, sch.optimizer.reject_count, float(sch.optimizer.loss), max(sch.reject_hist)], dtype=np.float64)
            gout = OPT.Local_TwoFrame_PGO.optim_to_world(None, gout, T_o2w)
            stage["pose_world_f32"] = raw(gout.motion).reshape(7).clone()
            assert stage["pose_world_f32"].dtype == torch.float32
            stage["world_solve_f32"] = world_f32
            diff = float((stage["pose_world_f32"][:3].double() - world_f32[:3].double()).norm())
            print(f"case {ci} {gname}: steps {sch.steps} rejects {sch.optimizer.reject_count} (max {max(sch.reject_hist)})  |local - world| = {diff:.3e} m")
            assert diff >= MIN_LOCAL_WORLD_DIFF, (ci, gname, diff)
            for k, v in stage.items():
                if k in ("pos_To", "cov_To") and gname != GRAPHS[0]:
                    assert np.array_equal(np.asarray(v), out[f"c{ci}/{GRAPHS[0]}/{k}"])     # graph-independent: stored once
                    continue
                out[f"c{ci}/{gname}/{k}"] = np.asarray(v)
    _save("local_pgo", out)


# ------------------------------------------------------------------------------------------------------------ keyframe_run.npz
def run_keyframe_case(ref, spec) -> dict:
    base, repeat, (kf_type, freq), opt_type, graph = spec
    case = dict(refrun.CASES[base], graph=graph)     # (the base case as it is: with its dense-mapping tail, which draws from the same generator)
    cam, maps, poses = refrun.tartanair_maps()
    maps, poses = maps * repeat, poses.repeat(repeat, 1)
    frames = refrun.make_stereo_frames(ref, cam, maps, poses)
    cfg = refrun.make_config(case, "ref")
    cfg.Odometry.keyframe = NS(type=kf_type, args=NS() if freq is None else NS(keyframe_freq=freq))
    cfg.Odometry.optimizer.type = opt_type
    ref.OM.MACVO.is_valid_config(cfg.Odometry)
    cfg.Odometry.frontend.args.model = refrun.ReplayNet(maps, "cpu")
    torch.manual_seed(SEED)
    system = ref.OM.MACVO.from_config(cfg)
    pushed = {}

    def on_frame(frame, sysm, pb):      # after the last frame this is the flag column as the loop pushed it (terminate has not run yet)
        pushed["flags"] = sysm.graph.frames.data["need_interp"].tensor.clone().numpy()
        pushed["pose"] = sysm.graph.frames.data["pose"].tensor.clone().numpy()

    with tempfile.TemporaryDirectory() as tmp:
        box = ref.Sandbox(Path(tmp))
        system.receive_frames(frames, box, on_frame_finished=on_frame)
        assert system.terminated and os.path.exists(box.path("tensor_map.npz")), "receive_frames swallowed an exception"
        tm = dict(np.load(box.path("tensor_map.npz")))
        out = {f"map/{k}": v for k, v in tm.items()}
        out["poses_npy"] = np.load(box.path("poses.npy"))
    n = len(frames)
    out["need_interp_pushed"] = pushed["flags"][:n].astype(bool)
    out["pose_before_terminate"] = pushed["pose"][:n]
    return out


def gen_keyframe_run():
    ref = refrun.import_reference()
    from Utility.PrettyPrint import GlobalConsole
    GlobalConsole.quiet = True
    out = {}
    # Rows that do not depend on the pose (keypoints, gathered values, camera-frame covariances) are the same bits whatever the optimizer: a table equal to
    # the one of an earlier case here, or of the base case's world-frame run in macvo_run.npz, is stored as a reference ("same": key -> [file or "", key]).
    same = {}
    pinned = dict(np.load(os.path.join(ROOT, "tests", "golden", "macvo_run.npz")))
    for name, spec in KEYFRAME_CASES.items():
        r = run_keyframe_case(ref, spec)
        freq = spec[2][1] or 1
        n = r["need_interp_pushed"].shape[0]
        ranges = r["map/edge/frame2match/ranges"]
        key = [t for t in range(1, n) if t % freq == 0]
        per_key = [int(ranges[t, 0, 1]) for t in key]
        assert np.array_equal(r["need_interp_pushed"], np.arange(n) % freq != 0), (name, r["need_interp_pushed"])
        assert min(per_key) >= MIN_NUM_POINT, (name, per_key)                      # every keyframe is solved
        ser = r["map/frames//need_interp"].astype(bool)
        if freq > 1:
            assert ser[1:][2:-2].any(), (name, "no motion is interpolated", ser)        # MotionInterpolate clears the first and last two flags of frames[1:]
        for k, v in r.items():
            if k.startswith("map/match//") or k in KEEP or k in ("poses_npy", "need_interp_pushed", "pose_before_terminate"):
                twin = None
                if k.startswith("map/match//"):
                    base_key = f"{spec[0]}/{k}"
                    if spec[1] == 1 and base_key in pinned and np.array_equal(pinned[base_key], v):
                        twin = ["macvo_run.npz", base_key]
                    for other in KEYFRAME_CASES:
                        if twin is None and f"{other}/{k}" in out and np.array_equal(out[f"{other}/{k}"], v):
                            twin = ["", f"{other}/{k}"]
                if twin is None:
                    out[f"{name}/{k}"] = v
                else:
                    same[f"{name}/{k}"] = twin
        print(name, "observations per keyframe", per_key, "flags pushed", r["need_interp_pushed"].astype(int).tolist(), "serialised", ser.astype(int).tolist())
    out["meta"] = np.array(json.dumps(dict(cases={k: [v[0], v[1], list(v[2]), v[3], v[4]] for k, v in KEYFRAME_CASES.items()}, seed=SEED, same=same)))
    _save("keyframe_run", out)


def _save(name, out):
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **{k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()})
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= 512 * 1024, size


def main():
    assert os.path.isdir("/root/reference/Odometry") or os.environ.get("MACVO_REFERENCE_ROOT"), "runs in the build container (needs the reference checkout)"
    refrun.import_reference()
    only = set(sys.argv[1:])
    if not only or "local_pgo" in only:
        gen_local_pgo()
    if not only or "keyframe_run" in only:
        gen_keyframe_run()


if __name__ == "__main__":
    main()
