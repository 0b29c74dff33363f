"""CPU: the ground the GPU tests of tests/test_gpu_backend_domain.py stand on.  The PGO kernel's host twin (tests/c_abi/pgo_twin.cpp on the kernel's own
pgo_math.h) against the oracle on correlated, singular, zero, tiny and indefinite pixel covariances, a first step past the Taylor branch and far / near-pi
priors; and the covariance oracle's own properties: an index clamp is an edge-replicated map, and what one fp32 evaluation costs against float64 per K."""
import pytest
import torch

from tests import backend_cases as bc
from tests import pgo_twin
from tests.test_gpu_backend import _to_batch

CPU = torch.device("cpu")


@pytest.mark.parametrize("nw", [4, 1])
@pytest.mark.parametrize("graph", bc.GRAPHS)
def test_twin_matches_oracle_outside_the_generator_domain(graph, nw):
    """Every pgo_cases() entry on each graph that reads what it edits: LM steps and reject count equal, pose within 1e-8 m / 1e-8 rad, loss rel 1e-8 — the
    bars of test_pgo_twin.py::test_twin_matches_oracle — in the 4-wave and the one-wave replay.  Measured: steps / rejects equal everywhere, pose
    <= 6.7e-13 m / 3.9e-14 rad (reproj; disp 5.9e-14 m, icp 1.3e-14 m).  indef in the far frame has an indefinite J^T W J in its second step: the reference's PINV
    solver steps on, and so does chol_solve6 through gauss_solve6 (without it the twin stopped after 3 steps where the oracle takes 10, 2.7e-2 m apart)."""
    from oracle import se3

    idx = [i for i, c in enumerate(bc.pgo_cases()) if graph in c[3]]
    assert len(idx) >= 18
    pose, info = pgo_twin.solve(_to_batch([bc.pgo_cases()[i][2] for i in idx], CPU), graph, nw=nw)
    worst = (0.0, 0.0)
    for k, i in enumerate(idx):
        name, frame = bc.pgo_cases()[i][:2]
        ref = bc.pgo_oracle(i, graph)
        dt, dr = se3.pose_error(ref.pose, pose[k])
        worst = (max(worst[0], dt), max(worst[1], dr))
        assert (int(info[k, 1]), int(info[k, 2])) == (ref.steps, ref.reject_count), (name, frame, info[k].tolist(), ref.steps, ref.reject_count)
        assert dt <= 1e-8 and dr <= 1e-8, (name, frame, dt, dr)
        assert info[k, 0].item() == pytest.approx(ref.loss, rel=1e-8, abs=1e-12), (name, frame)
    print(f"{graph} nw={nw}: worst pose error {worst[0]:.2e} m {worst[1]:.2e} rad over {len(idx)} problems")


def test_cases_reach_the_branches_they_name():
    """The inputs do what the table says: rank1 is exactly singular in fp32 and fp64, indef has a negative eigenvalue, corr is correlated on every row,
    bigstep's first step leaves the Taylor branch of se3_left_update (|phi| > 0.1 between prior and solution), the moved priors are far / near pi."""
    from oracle import se3

    cases = {(n, f): p for n, f, p, _ in bc.pgo_cases()}
    uvc = cases[("rank160", "id")].pixel2_uv_cov[: bc.EDIT_ROWS]
    for t in (uvc, uvc.double()):
        assert (t[:, 0] * t[:, 1] - t[:, 2] * t[:, 2] == 0).all()
    uvc = cases[("indef60", "id")].pixel2_uv_cov[: bc.EDIT_ROWS].double()
    assert (uvc[:, 0] * uvc[:, 1] - uvc[:, 2] ** 2 < 0).all()
    for n in (60, 300):
        uvc = cases[(f"corr{n}", "id")].pixel2_uv_cov.double()
        r = uvc[:, 2] / (uvc[:, 0] * uvc[:, 1]).sqrt()
        assert ((r.abs() - 0.8).abs() < 1e-6).all() and (r > 0).any() and (r < 0).any()
    assert (cases[("zero_all60", "id")].pixel2_disp_cov[: bc.EDIT_ROWS] == 0).all() and (cases[("zero_uv60", "id")].pixel2_disp_cov > 0).all()
    i = [c[:2] for c in bc.pgo_cases()].index(("bigstep60", "id"))
    for g in bc.GRAPHS:
        xi = se3.se3_log(se3.se3_mul(bc.pgo_oracle(i, g).pose, se3.se3_inv(bc.pgo_cases()[i][2].init_pose.double())))
        assert xi[3:].norm() > 0.1, (g, xi)
    far, pi = cases[("corr60", "far")].init_pose.double(), cases[("corr60", "pi")].init_pose.double()
    assert far[:3].norm() > 47 and 1.8 < se3.so3_log(far[3:]).norm() < 2.0
    assert 0 < torch.pi - se3.so3_log(pi[3:]).norm() <= 2.01e-4


@pytest.mark.parametrize("K", bc.COV_KS)
def test_index_clamp_is_an_edge_replicated_map(K):
    """What makes the border reference legitimate: for interior keypoints match_covariance(kp, depth) and match_covariance(kp + 16, replicate_pad(depth, 16),
    cx + 16, cy + 16) are bit-equal on float64 tensors (every coordinate is a multiple of 0.25, so u - cx is exact in both) — and the padded form is defined
    for the border keypoints, where the unpadded oracle's negative indices would wrap around."""
    c = bc.cov_cases()
    a = bc.cov_reference(K, "interior")
    b = bc.cov_oracle(c["kp"] + bc.PAD, bc.replicate_pad(c["depth"]), c["sigma_nan"], bc.shifted(c["K4"]), K, torch.float64)
    for x, y in zip(a, b):
        assert x.dtype == torch.float64 and torch.equal(torch.nan_to_num(x, 7.0), torch.nan_to_num(y, 7.0))
    kb = c["border"][K]
    assert kb.shape[0] == (14 if K == 1 else 18)
    wavg = bc.cov_reference(K, "border")[1]
    assert wavg[5].isnan() and wavg[torch.arange(kb.shape[0]) != 5].isfinite().all()       # (row 5 is sigma_nan's indefinite one)


def test_depth_map_is_textured():
    """The patch variance is the statistic under test: it must not sit on the min_depth_cov clamp (synth.depth_maps is that smooth)."""
    for K in bc.COV_KS:
        frac = bc.textured_fraction(K)
        print(f"K={K}: {frac:.3f} of the interior keypoints above the clamp")
        if K >= 7:
            assert frac >= 0.75, (K, frac)
    c = bc.cov_cases()
    assert int((c["sigma"][:, :2] < 0.0625).any(1).sum()) == 5
    s = c["sigma"].clone()
    s[:, :2].clamp_(min=0.0625)
    assert (s[:, 0] * s[:, 1] - s[:, 2] ** 2 > 0).all() and (c["sigma"][:, 2].abs() > 0.01).sum() > 50


@pytest.mark.parametrize("K", bc.COV_KS)
def test_fp32_oracle_distance_from_float64(K):
    """The number the GPU bar hangs on: the fp32 oracle against the oracle on float64 tensors, in the norms of the GPU test.  Measured: cov 1.1e-7 .. 1.8e-7,
    wavg <= 1.9e-7, wvar <= 1.6e-7 (K = 1: wavg exact).  Pinned loosely; the GPU test recomputes it at run time.
    The oracle on float64 tensors gathers, sums and projects in float64, but it still builds its Gaussian weights in fp32 and rounds the 3 x 3 to fp32 before
    widening it (``create_2x2_matrix`` / ``create_3x3_matrix`` / ``.float()`` in oracle/covariance.py), so it is no exact value either: bc.cov_float64 (every
    operation in float64) lies 1.8e-7 .. 2.4e-7 from it (K = 1: 3e-8), the size of one fp32 evaluation.  Printed and pinned as loosely."""
    e = bc.cov_e_ref(K)
    c = bc.cov_cases()
    t = bc.cov_float64(c["kp"], c["depth"], c["sigma_nan"], c["K4"], K)
    r = bc.cov_reference(K, "interior")
    d = (bc.block_err(r[0], t[0]), bc.rel_err(r[1], t[1]), bc.rel_err(r[2], t[2]))
    print(f"K={K}: fp32 oracle vs float64 oracle cov {e[0]:.3e} wavg {e[1]:.3e} wvar {e[2]:.3e}; float64 oracle vs all-float64 cov {d[0]:.3e} wavg {d[1]:.3e} "
          f"wvar {d[2]:.3e}")
    assert max(e) <= 1e-5 and max(d) <= 1e-5
    assert bc.cov_bar(K) == tuple(4 * max(x, 2.0 ** -23) for x in e)
