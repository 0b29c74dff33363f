"""GPU: the PGO solve, back-projection, world registration and map points on cameras that are not fx = fy = 320 (tests/cameras.py).

1. ``ops.pgo_solve`` on EUROC, KITTI and ANISO against the reference's own optimizer (tests/golden/pgo_intrinsics.npz) and the host twin at the bars of
   test_gpu_golden.py::test_pgo_vs_reference_golden and test_gpu_backend.py::test_pgo_kernel_equals_host_twin; a batch that interleaves the cameras
   (neighbouring problems differ in K and in baseline) equal to its solo solves bit for bit, in the four-wave and in the one-wave (> 512 problems) form;
   the local form on the moved ANISO problem at the bars of test_gpu_local_pgo.py.
2. ``ops.backproject``, ``ops.pose_apply`` and ``ops.map_points`` against plain fp32 / fp64 references at large rotations, for n = 1, 200 and 257 rows.

Reads only committed .npz data, never the reference tree."""
import math

import pytest
import torch

from tests import cameras, pgo_local_twin, pgo_twin
from tests.test_local_keyframe_host import GRAPHS, check_against_golden, problem, stage
from tests.test_pgo_intrinsics_host import check_world, load_gold, world_cases

pytestmark = pytest.mark.gpu
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def gold():
    return load_gold()


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ================================================================================================================= 1. PGO
@pytest.mark.parametrize("graph", GRAPHS)
def test_pgo_vs_reference_golden_and_twin(gpu, gold, graph):
    from macvo_amd import ops
    from tests.test_gpu_backend import _to_batch

    cases = world_cases(gold, graph)
    probs = [c[2] for c in cases]
    pose, info = ops.pgo_solve(_to_batch(probs, gpu), graph)
    pose, info = pose.cpu(), info.cpu()
    check_world(cases, pose, info, "kernel")
    pose_t, info_t = pgo_twin.solve(_to_batch(probs, CPU), graph)
    assert torch.equal(info[:, 1:3], info_t[:, 1:3]), (info, info_t)
    torch.testing.assert_close(pose, pose_t, rtol=0, atol=1e-11)
    torch.testing.assert_close(info[:, 0], info_t[:, 0], rtol=1e-11, atol=1e-13)


def _default_problems():
    from oracle import pgo

    return [pgo.make_synthetic_problem(n=150, seed=12)[0], pgo.make_synthetic_problem(n=64, seed=11, outlier_frac=0.3)[0]]


@pytest.mark.parametrize("graph", GRAPHS)
def test_heterogeneous_batch_equals_solo_solves(gpu, gold, graph):
    """Twelve golden problems interleaved by camera plus two default-camera ones, as one batch: the bits of the fourteen solo solves.  Then the same
    fourteen inside > 512 problems (the one-wave form): the golden's and the twin's bars, and the same bits wherever the fourteen sit in the batch."""
    from macvo_amd import ops
    from oracle import pgo
    from tests.test_gpu_backend import _to_batch

    cases = world_cases(gold, graph)
    dflt = _default_problems()
    probs = [c[2] for c in cases]
    # E0 K0 A0 E1 | default | K1 A1 E2 | default | K2 A2 E3 K3 A3: the default camera shares ANISO's baseline and never sits next to it
    mixed = probs[:4] + [dflt[0]] + probs[4:7] + [dflt[1]] + probs[7:]
    where = [0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13]                     # the golden problems inside ``mixed``
    b = _to_batch(mixed, gpu)
    assert b.intrinsics.unique(dim=0).shape[0] == 4 and b.baseline.unique().numel() == 3
    assert all(not torch.equal(b.intrinsics[k], b.intrinsics[k + 1]) and b.baseline[k] != b.baseline[k + 1] for k in range(len(mixed) - 1))
    pose, info = ops.pgo_solve(b, graph)
    for k, p in enumerate(mixed):
        sp, si = ops.pgo_solve(_to_batch([p], gpu), graph)
        assert torch.equal(_bits(sp[0]), _bits(pose[k])) and torch.equal(_bits(si[0]), _bits(info[k])), (graph, k)
    check_world(cases, pose.cpu()[where], info.cpu()[where], "mixed batch")
    # one wave per problem
    pad = [pgo.make_synthetic_problem(n=20 + (k % 7), seed=100 + k)[0] for k in range(520)]
    big = mixed + pad
    bp, bi = ops.pgo_solve(_to_batch(big, gpu), graph)
    rp, ri = ops.pgo_solve(_to_batch(pad[:300] + mixed[::-1] + pad[300:], gpu), graph)
    torch.cuda.synchronize()
    back = list(range(300 + len(mixed) - 1, 299, -1))
    assert torch.equal(_bits(bp[: len(mixed)]), _bits(rp[back])) and torch.equal(_bits(bi[: len(mixed)]), _bits(ri[back])), graph
    assert torch.equal(_bits(bp[len(mixed) + 300:]), _bits(rp[len(mixed) + 300:]))
    bp, bi = bp.cpu(), bi.cpu()
    check_world(cases, bp[where], bi[where], "one-wave batch")
    tp, ti = pgo_twin.solve(_to_batch(big, CPU), graph)
    assert torch.equal(bi[:, 1:3], ti[:, 1:3])
    torch.testing.assert_close(bp, tp, rtol=0, atol=1e-11)
    torch.testing.assert_close(bi[:, 0], ti[:, 0], rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("graph", GRAPHS)
def test_local_solve_vs_reference_golden_and_twin(gpu, gold, graph):
    """The moved ANISO problem through ``ops.pgo_solve(ref_pose=...)``, as test_gpu_local_pgo.py tests local_pgo.npz; then in one batch with a
    default-camera problem of local_pgo.npz: the bits of the solo solves."""
    import json
    import os

    import numpy as np

    from macvo_amd import ops
    from oracle import se3
    from tests.test_gpu_backend import _to_batch

    p, ref = problem(gold, 0)
    assert p.K[0, 0] != p.K[1, 1]
    w32 = torch.zeros((1, 7), dtype=torch.float32, device=gpu)
    pose, info = ops.pgo_solve(_to_batch([p], gpu), graph, out_pose_f32=w32, ref_pose=ref.reshape(1, 7).to(gpu))
    torch.cuda.synchronize()
    pose_c, info_c, w32_c = pose.cpu(), info.cpu(), w32.cpu()
    check_against_golden(gold, 0, graph, stage(gold, 0, graph, "T_c2o"), stage(gold, 0, graph, "pos_To"), stage(gold, 0, graph, "cov_To"), pose_c[0],
                         int(info_c[0, 1]), int(info_c[0, 2]), float(info_c[0, 0]), w32_c[0], "kernel")
    tw = pgo_local_twin.solve(_to_batch([p], CPU), ref.reshape(1, 7), graph)
    dt, dr = se3.pose_error(tw.pose[0], pose_c[0])
    print(f"kernel vs twin, {graph}: {dt:.3e} m {dr:.3e} rad")
    assert torch.equal(info_c[0, 1:3], tw.info[0, 1:3])
    torch.testing.assert_close(pose_c, tw.pose, rtol=0, atol=1e-11)
    torch.testing.assert_close(info_c[:, 0], tw.info[:, 0], rtol=1e-11, atol=1e-13)
    assert torch.equal(w32_c[0], tw.pose_f32[0]), (graph, w32_c, tw.pose_f32)
    # next to a problem with another camera and another baseline
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_pgo.npz"))
    other = {k: z[k] for k in z.files}
    other["meta"] = json.loads(str(other["meta"]))
    q, qref = problem(other, 1)
    assert not torch.equal(q.K, p.K)
    s32 = torch.zeros((1, 7), dtype=torch.float32, device=gpu)
    qp, qi = ops.pgo_solve(_to_batch([q], gpu), graph, out_pose_f32=s32, ref_pose=qref.reshape(1, 7).to(gpu))
    b32 = torch.zeros((3, 7), dtype=torch.float32, device=gpu)
    bp, bi = ops.pgo_solve(_to_batch([q, p, q], gpu), graph, out_pose_f32=b32, ref_pose=torch.stack([qref, ref, qref]).to(gpu))
    torch.cuda.synchronize()
    assert torch.equal(_bits(bp[1]), _bits(pose[0])) and torch.equal(_bits(bi[1]), _bits(info[0])) and torch.equal(b32[1], w32[0])
    for k in (0, 2):
        assert torch.equal(_bits(bp[k]), _bits(qp[0])) and torch.equal(_bits(bi[k]), _bits(qi[0])) and torch.equal(b32[k], s32[0])


# ================================================================================================================= 2. back-projection
U24 = 2.0 ** -24
CAMS = (cameras.EUROC, cameras.KITTI, cameras.ANISO)


def _poses():
    """identity; ~170 degrees about a skew axis with |t| ~ 50; a generic unit quaternion with w < 0 (normalised in fp64, stored in fp32)."""
    ax = torch.tensor([1.0, 2.0, -1.5], dtype=torch.float64)
    ax = ax / ax.norm()
    half = math.radians(170.0) / 2
    big = torch.cat([torch.tensor([30.0, -35.0, 20.0], dtype=torch.float64), ax * math.sin(half), torch.tensor([math.cos(half)], dtype=torch.float64)])
    q = torch.tensor([0.3, -0.5, 0.4, -0.7], dtype=torch.float64)
    neg = torch.cat([torch.tensor([1.5, -2.25, 0.75], dtype=torch.float64), q / q.norm()])
    assert abs(float(big[:3].norm()) - 50.0) < 1.0 and float(neg[6]) < 0
    return {"identity": torch.tensor([0, 0, 0, 0, 0, 0, 1.0]), "rot170": big.float(), "w_negative": neg.float()}


@pytest.fixture(scope="module")
def rows():
    """Per camera: 257 float keypoints inside the image (the first four near its corners) and depths in [1, 60]; the tests take the first n."""
    out = {}
    for ci, c in enumerate(CAMS):
        g = torch.Generator().manual_seed(40 + ci)
        n = 257
        kp = torch.stack([torch.rand(n, generator=g) * (c.W - 1), torch.rand(n, generator=g) * (c.H - 1)], 1)
        kp[:4] = torch.tensor([[0.0, 0.0], [c.W - 1.0, 0.0], [0.0, c.H - 1.0], [c.W - 1.0, c.H - 1.0]])
        d = 1 + 59 * torch.rand(n, generator=g)
        d[0], d[1] = 1.0, 60.0
        out[c.name] = (kp.float(), d.float())
    return out


def _check_world_rows(pos_Tc, pos_Tw, pose, what):
    """pos_Tw against R p + t in fp64 (R the fp64 rotation matrix of the stored fp32 quaternion, p the fp32 camera-frame rows): per row
    8 * 2^-24 * (|p|_1 + |t|_1), eight fp32 roundings (quaternion -> matrix, three multiply-adds, one add)."""
    from oracle import se3

    R = se3.quat_to_matrix(pose[3:].double())
    p = pos_Tc.double()
    want = p @ R.T + pose[:3].double()
    err = (pos_Tw.double() - want).abs().max(dim=1).values
    bound = 8 * U24 * (p.abs().sum(dim=1) + pose[:3].double().abs().sum())
    worst = float((err / bound).max())
    print(f"{what}: pos_Tw max error {float(err.max()):.3e}, worst error / bound {worst:.3f}")
    assert (err <= bound).all(), (what, worst)


@pytest.mark.parametrize("n", [1, 200, 257])
@pytest.mark.parametrize("cam", CAMS, ids=lambda c: c.name)
def test_backproject_vs_plain_references(gpu, rows, cam, n):
    """``pos_Tc`` is BIT-EQUAL to ``oracle.frontend.pixel2point_NED`` evaluated in fp32 on the CPU (one subtraction, one multiplication and one
    correctly rounded division per component, in the order oracle/frontend.py documents; nothing there can be contracted into an FMA) — bit equality
    held, the rtol 1e-6 / atol 1e-6 of test_gpu_pipeline.py was not needed.  ``rot`` against ``oracle.se3.quat_to_matrix`` in fp64: each entry is at
    most six fp32 roundings of values <= 2 (PyPose's ``Act(I).T``: one product by w, a two-product difference, two sums), so 6 * 2^-23.  ``pos_Tw`` per row."""
    from macvo_amd import ops
    from oracle import frontend, se3

    kp, d = rows[cam.name][0][:n], rows[cam.name][1][:n]
    want_Tc = frontend.pixel2point_NED(kp, d, cameras.K_matrix(cam))
    assert want_Tc.dtype == torch.float32
    for name, pose in _poses().items():
        pos_Tc, pos_Tw, rot = ops.backproject(kp.to(gpu), d.to(gpu), cam.K, pose.to(gpu), want_rot=True)
        pos_Tc, pos_Tw, rot = pos_Tc.cpu(), pos_Tw.cpu(), rot.cpu()
        diff = (pos_Tc.double() - want_Tc.double()).abs()
        print(f"{cam.name} n={n} {name}: pos_Tc bit-equal {torch.equal(_bits(pos_Tc), _bits(want_Tc))}, max difference {float(diff.max()):.3e}")
        assert torch.equal(_bits(pos_Tc), _bits(want_Tc)), (cam.name, n, name)
        R = se3.quat_to_matrix(pose[3:].double())
        rerr = float((rot.reshape(3, 3) - R).abs().max())
        print(f"{cam.name} n={n} {name}: rot max error {rerr:.3e}")
        assert rot.dtype == torch.float64 and rerr <= 6 * 2.0 ** -23, (name, rerr)
        if name == "identity":
            assert torch.equal(rot.reshape(3, 3), torch.eye(3, dtype=torch.float64)) and torch.equal(_bits(pos_Tw), _bits(pos_Tc))
        _check_world_rows(pos_Tc, pos_Tw, pose, f"{cam.name} n={n} {name}")
    # no pose: camera-frame rows only, the same bits
    only_Tc, none_Tw, none_rot = ops.backproject(kp.to(gpu), d.to(gpu), cam.K, None)
    assert none_Tw is None and none_rot is None and torch.equal(_bits(only_Tc.cpu()), _bits(want_Tc))


@pytest.mark.parametrize("n", [1, 200, 257])
@pytest.mark.parametrize("cam", CAMS, ids=lambda c: c.name)
def test_pose_apply_vs_backproject_and_fp64_rotation(gpu, rows, cam, n):
    """``ops.pose_apply`` keeps its bitwise relation to ``backproject`` + ``match_cov(rot=...)`` at these cameras and poses, and its ``cov_w`` is
    ``oracle.covariance.rotate_covariance`` in fp64 (rtol 1e-12, the bound of test_match_cov)."""
    from macvo_amd import ops
    from oracle import covariance
    from tests import synth

    depth, _ = synth.depth_maps(cam.H, cam.W, 3)
    depth = depth.to(gpu)
    kp, d = rows[cam.name][0][:n].to(gpu), rows[cam.name][1][:n].to(gpu)
    g = torch.Generator().manual_seed(9)
    sigma = (torch.rand(n, 3, generator=g) * torch.tensor([2.0, 2.0, 0.2]) + torch.tensor([0.3, 0.3, -0.1])).float()
    for name, pose in _poses().items():
        pose = pose.to(gpu)
        pos_Tc, pos_Tw, rot = ops.backproject(kp, d, cam.K, pose, want_rot=True)
        cov, cov_w = ops.match_cov(depth, kp, sigma.clone().to(gpu), None, *cam.K, rot=rot.view(3, 3))
        pos_Tw2, rot2, cov_w2 = ops.pose_apply(pose, pos_Tc, cov)
        assert torch.equal(_bits(pos_Tw), _bits(pos_Tw2)), (cam.name, n, name)
        assert torch.equal(_bits(rot.reshape(9)), _bits(rot2)), (cam.name, n, name)
        assert torch.equal(_bits(cov_w), _bits(cov_w2)), (cam.name, n, name)
        assert not cov.isnan().any()
        torch.testing.assert_close(cov_w2.cpu(), covariance.rotate_covariance(rot2.cpu().view(3, 3), cov.cpu()), rtol=1e-12, atol=1e-14)
        _check_world_rows(pos_Tc.cpu(), pos_Tw2.cpu(), pose.cpu(), f"pose_apply {cam.name} n={n} {name}")


def test_map_points_vs_direct_indexing_and_oracle(gpu):
    """``ops.map_points`` on a 64 x 96 depth / depth-cov / image triple, 300 pixels (the four corners first), ANISO_SMALL scaled to that image and the
    w < 0 pose: ``uv``, ``depth``, ``sigma_dd`` and ``color`` bit-equal to direct indexing, ``pos_Tc`` bit-equal to ``pixel2point_NED`` in fp32,
    ``pos_Tw`` per row as above, ``cov_Tc`` against ``oracle.covariance.match_covariance`` at rtol 2e-4 / atol 1e-7 (test_dense_mapping_tail_matches_oracle)
    on the pixels whose 31 x 31 patch lies inside the image (the oracle cannot index the others)."""
    from macvo_amd import ops
    from oracle import covariance, frontend
    from tests import synth

    H, W, n = 64, 96, 300
    c = cameras.ANISO_SMALL
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731   (the kernel takes fp32 arguments: the same values on both sides)
    K4 = (f32(c.fx * W / c.W), f32(c.fy * H / c.H), f32(c.cx * W / c.W), f32(c.cy * H / c.H))
    assert K4[0] != K4[1]
    Km = torch.tensor([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1]], dtype=torch.float32)
    depth, dcov = synth.depth_maps(H, W, 3)
    g = torch.Generator().manual_seed(17)
    image = torch.rand(1, 3, H, W, generator=g)
    uv = torch.stack([torch.randint(0, W, (n,), generator=g), torch.randint(0, H, (n,), generator=g)], 1)
    uv[:4] = torch.tensor([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]])
    uv[4:154] = torch.stack([torch.randint(15, W - 15, (150,), generator=g), torch.randint(15, H - 15, (150,), generator=g)], 1)
    pose = _poses()["w_negative"]
    m = ops.map_points(uv.to(gpu), depth.to(gpu), dcov.to(gpu), K4, pose.to(gpu), image=image.to(gpu))
    torch.cuda.synchronize()
    assert torch.equal(m.uv.cpu(), uv.float())
    md = depth[0, 0, uv[:, 1], uv[:, 0]]
    assert torch.equal(_bits(m.depth.cpu()), _bits(md)) and torch.equal(_bits(m.sigma_dd.cpu()), _bits(dcov[0, 0, uv[:, 1], uv[:, 0]]))
    assert torch.equal(m.color.cpu(), (image[0][:, uv[:, 1], uv[:, 0]].T * 255).to(torch.uint8))
    want_Tc = frontend.pixel2point_NED(uv, md, Km)
    assert want_Tc.dtype == torch.float32 and torch.equal(_bits(m.pos_Tc.cpu()), _bits(want_Tc))
    _check_world_rows(m.pos_Tc.cpu(), m.pos_Tw.cpu(), pose, "map_points")
    inside = (uv[:, 0] >= 15) & (uv[:, 0] < W - 15) & (uv[:, 1] >= 15) & (uv[:, 1] < H - 15)
    assert int(inside.sum()) >= 150 and not inside[:4].any()
    suv = torch.ones(int(inside.sum()), 3) * 0.25
    suv[:, 2] = 0
    want_cov = covariance.match_covariance(uv[inside], depth, dcov[0, 0, uv[inside, 1], uv[inside, 0]], suv, *K4)
    torch.testing.assert_close(m.cov_Tc.cpu()[inside], want_cov, rtol=2e-4, atol=1e-7)
    assert not m.cov_Tc.isnan().any()
