"""CPU: the PGO solve on cameras that are not fx = fy = 320 (tests/cameras.py: EUROC, KITTI, ANISO), against what the reference's own
``TwoFrame_PGO._optimize`` / ``Local_TwoFrame_PGO`` produced on them (tests/golden/pgo_intrinsics.npz, written by
tests/golden/make_golden_pgo_intrinsics.py).

  * ``oracle.pgo.solve`` at the bars of test_oracle_golden.py::test_pgo_matches_reference_in_tree_code;
  * the host twin of the kernel (tests/c_abi/pgo_twin.cpp, which includes csrc/pgo_math.h) at the bars of test_pgo_twin.py::test_twin_vs_reference_golden,
    also as ONE batch that interleaves the cameras, so that neighbouring problems differ in K and in baseline;
  * the local-frame twin and the torch restatement at the bars of test_local_keyframe_host.py;
  * ``tools.synth.make_sequence(cam=...)``: the default is what it was, bit for bit, and a given camera reaches the generated flow.

Replacing ``g.fy`` by ``g.fx`` in the reprojection residual or in the analytic Jacobian of csrc/pgo_math.h makes the twin tests of this file fail for
reproj and disp on EUROC and ANISO (KITTI has fx == fy: it is here for its principal point and its baseline * fx)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import cameras
from tests.test_local_keyframe_host import GRAPHS, check_against_golden, problem

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pgo_intrinsics.npz")
CPU = torch.device("cpu")
CAMERAS = ("EUROC", "KITTI", "ANISO")


def load_gold():
    z = np.load(GOLD)
    g = {k: z[k] for k in z.files}
    g["meta"] = json.loads(str(g["meta"]))
    return g


@pytest.fixture(scope="module")
def gold():
    return load_gold()


def world_cases(g, graph):
    """The twelve world-frame cases of a graph, INTERLEAVED by camera (EUROC 0, KITTI 0, ANISO 0, EUROC 1, ...): a list of
    (camera name, case index, PGOProblem, golden pose [7] f64, golden [steps, rejects, loss, max rejects])."""
    from oracle import pgo

    meta = g["meta"]
    assert tuple(meta["cameras"]) == CAMERAS and tuple(meta["graphs"]) == GRAPHS
    out = []
    for ci, c in enumerate(meta["cases"]):
        for cname in CAMERAS:
            ck = meta["cameras"][cname]
            prob, _ = pgo.make_synthetic_problem(K=tuple(ck["K"]), baseline=ck["baseline"], W=ck["W"], H=ck["H"], **c)
            out.append((cname, ci, prob, torch.from_numpy(g[f"{cname}/{graph}/{ci}/pose"]), [float(v) for v in g[f"{cname}/{graph}/{ci}/stats"]]))
    return out


def test_golden_is_what_the_issue_asks_for(gold):
    """Three cameras x three graphs x the four cases, the cameras those of tests/cameras.py (two of them with fx != fy), and one moved ANISO problem for
    the local form."""
    meta = gold["meta"]
    assert meta["cases"] == [dict(n=200, seed=6), dict(n=37, seed=8), dict(n=120, seed=10, trans_sigma=0.4, rot_sigma=0.08),
                             dict(n=200, seed=7, outlier_frac=0.1)]
    for cname in CAMERAS:
        c, ck = cameras.BY_NAME[cname], meta["cameras"][cname]
        assert (tuple(ck["K"]), ck["baseline"], ck["W"], ck["H"]) == (c.K, c.baseline, c.W, c.H)
        for graph in GRAPHS:
            for ci in range(4):
                assert gold[f"{cname}/{graph}/{ci}/pose"].shape == (7,) and gold[f"{cname}/{graph}/{ci}/stats"].shape == (4,)
    assert cameras.EUROC.fx != cameras.EUROC.fy and cameras.ANISO.fx != cameras.ANISO.fy and cameras.ANISO_SMALL.fx != cameras.ANISO_SMALL.fy
    assert meta["local"]["camera"] == "ANISO" and meta["local"]["case"] == dict(n=200, seed=6)
    K = gold["c0/K"]
    assert (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) == cameras.ANISO.K and float(gold["c0/baseline"]) == cameras.ANISO.baseline
    assert float(np.linalg.norm(gold["c0/move"][:3])) > 1200
    assert os.path.getsize(GOLD) <= 128 * 1024


@pytest.mark.parametrize("graph", GRAPHS)
def test_oracle_vs_reference_golden(gold, graph):
    from oracle import pgo, se3

    for cname, ci, prob, ref, (steps, rej, loss, max_rej) in world_cases(gold, graph):
        res = pgo.solve(prob, graph)
        dt, dr = se3.pose_error(ref, res.pose)
        assert dt < 1e-9 and dr < 1e-9, (cname, ci, dt, dr)
        assert res.steps == int(steps) and res.reject_count == int(rej), (cname, ci, res.steps, steps, res.reject_count, rej)
        assert abs(res.loss - loss) <= 1e-9 * max(1.0, abs(loss)), (cname, ci)
        assert max(h[1] for h in res.history) == int(max_rej), (cname, ci)


def check_world(cases, pose, info, what):
    """The bars of test_twin_vs_reference_golden / test_pgo_vs_reference_golden: pose 1e-8 m / rad, steps and rejects equal, loss 1e-6 relative."""
    from oracle import se3

    for k, (cname, ci, _, ref, (steps, rej, loss, _)) in enumerate(cases):
        dt, dr = se3.pose_error(ref, pose[k])
        assert dt <= 1e-8 and dr <= 1e-8, (what, cname, ci, dt, dr)
        assert int(info[k, 1]) == int(steps) and int(info[k, 2]) == int(rej), (what, cname, ci, info[k].tolist(), steps, rej)
        assert abs(float(info[k, 0]) - loss) <= 1e-6 * max(1.0, abs(loss)), (what, cname, ci, float(info[k, 0]), loss)


@pytest.mark.parametrize("graph", GRAPHS)
def test_twin_vs_reference_golden(gold, graph):
    """Each problem alone, then all twelve in one batch interleaved by camera (per-problem intrinsics and baseline), four-wave and one-wave form."""
    from tests import pgo_twin
    from tests.test_gpu_backend import _to_batch

    cases = world_cases(gold, graph)
    probs = [c[2] for c in cases]
    solo = [pgo_twin.solve(_to_batch([p], CPU), graph) for p in probs]
    check_world(cases, torch.cat([s[0] for s in solo]), torch.cat([s[1] for s in solo]), "twin solo")
    for spec in (1, 0):
        pose, info = pgo_twin.solve(_to_batch(probs, CPU), graph, spec=spec)
        check_world(cases, pose, info, f"twin batch spec={spec}")
        assert torch.equal(pose, torch.cat([s[0] for s in solo])) and torch.equal(info, torch.cat([s[1] for s in solo]))
    pose, info = pgo_twin.solve(_to_batch(probs, CPU), graph, nw=1)
    check_world(cases, pose, info, "twin batch nw=1")


@pytest.mark.parametrize("graph", GRAPHS)
def test_local_twin_and_restatement_vs_reference_golden(gold, graph):
    from tests import local_pgo_ref as LR
    from tests import pgo_local_twin
    from tests.test_gpu_backend import _to_batch

    prob, ref = problem(gold, 0)
    for spec in (1, 0):
        o = pgo_local_twin.solve(_to_batch([prob], CPU), ref.reshape(1, 7), graph, spec=spec)
        check_against_golden(gold, 0, graph, o.init_local[0], o.pos_To, o.cov_To, o.pose[0], int(o.info[0, 1]), int(o.info[0, 2]), float(o.info[0, 0]),
                             o.pose_f32[0], f"twin(spec={spec})")
    r = LR.solve(prob, ref, graph)
    check_against_golden(gold, 0, graph, r.local.init_pose, r.local.pos_Tw, r.local.cov_Tw, r.res.pose, r.res.steps, r.res.reject_count, r.res.loss,
                         r.pose_f32, "restatement", ulps=0 if LR.cross_is_fused() else 2)


def test_make_sequence_default_camera_is_unchanged():
    """``make_sequence`` with no camera == with ``cam=make_camera(H, W)``, bit for bit (bench.py and smoke() use the default); a given camera comes back
    as the camera and reaches the flow."""
    from tools import synth

    H, W = 96, 128
    kw = dict(n_frames=3, H=H, W=W, C=8, iters=1, seed=4)
    cam_a, fr_a, po_a = synth.make_sequence(**kw)
    cam_b, fr_b, po_b = synth.make_sequence(cam=synth.make_camera(H, W), **kw)
    assert cam_a == cam_b == synth.make_camera(H, W)
    assert len(fr_a) == len(fr_b) == 3
    for a, b in zip(fr_a, fr_b):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert all(torch.equal(a, b) for a, b in zip(po_a, po_b))
    c = cameras.cam_dict(cameras.ANISO_SMALL, H=H, W=W)
    cam_c, fr_c, po_c = synth.make_sequence(cam=c, **kw)
    assert cam_c == c and all(torch.equal(a, b) for a, b in zip(po_a, po_c))
    assert not torch.equal(fr_c[1]["flow"], fr_a[1]["flow"])
    # the stereo sample is fx * baseline / depth: at the same pose and plane only the camera changes it
    z0 = -fr_c[0]["flow"][0, 0]
    assert 0.5 * c["fx"] * c["baseline"] / 12.0 < float(z0.median()) < 2.0 * c["fx"] * c["baseline"] / 12.0
