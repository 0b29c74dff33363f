"""GPU: the covariance model (mv_match_cov, mv_match_cov_pair, mv_obs_cov "gmm") and the PGO solve (mv_pgo_solve) outside the single point of their input
domain the rest of the suite reaches — every kernel size class, patches clipped at the map border, correlated / singular / zero / tiny / indefinite pixel
covariances, far and near-pi priors — against the float64 references of tests/backend_cases.py (tests/test_backend_domain_host.py checks those on the CPU)."""
import pytest
import torch

from tests import backend_cases as bc
from tests import cov_models_ref

pytestmark = pytest.mark.gpu


def _dev(c, gpu, *names):
    return [c[n].to(gpu) for n in names]


def _check(tag, K, got, ref):
    """cov, wavg, wvar of a kernel against the float64 reference, each within 4 x max(e_ref, 2^-23) (bc.cov_bar); prints every figure before asserting."""
    e = (bc.block_err(got[0].cpu(), ref[0]), bc.rel_err(got[1].cpu(), ref[1]), bc.rel_err(got[2].cpu(), ref[2]))
    bar, e_ref = bc.cov_bar(K), bc.cov_e_ref(K)
    print(f"{tag} K={K}: kernel cov {e[0]:.3e} wavg {e[1]:.3e} wvar {e[2]:.3e} | e_ref cov {e_ref[0]:.3e} wavg {e_ref[1]:.3e} wvar {e_ref[2]:.3e}")
    for name, x, b in zip(("cov", "wavg", "wvar"), e, bar):
        assert x <= b, (tag, K, name, x, b)


@pytest.mark.parametrize("K", bc.COV_KS)
def test_match_cov_every_kernel_size_interior_and_border(gpu, K):
    """ops.match_cov(..., want_stats=True) at K = 1 (one tap, the clamp), 3, 7, 9 (81 taps: one full lane round and a partial one), 15, 31 on 61 keypoints (the
    last workgroup has one live wave) of a textured map, and on keypoints whose patches are clipped at the border.  Reference: the oracle on float64 tensors;
    for the border set, on the map replicate-padded by 16.  Bar per quantity: 4 x max(e_ref, 2^-23), e_ref = the fp32 oracle's own distance from that reference on
    the interior inputs, computed at run time.  The NaN row (indefinite sigma) is NaN on both sides; the in-place clamp of flow_cov is bit-exact.
    Measured on an MI355X, kernel error interior / border | e_ref:
        K      cov                      wavg                     wvar
        1   1.14e-7 / 7.45e-8 | 1.14e-7   0 / 0 | 0                1.49e-8 / 1.49e-8 | 1.49e-8
        3   2.81e-7 / 2.75e-7 | 1.21e-7   1.90e-7 / 1.27e-7 | 1.22e-7   2.49e-7 / 2.70e-7 | 1.08e-7
        7   2.43e-7 / 1.82e-7 | 1.21e-7   2.29e-7 / 1.91e-7 | 1.48e-7   2.77e-7 / 1.55e-7 | 1.16e-7
        9   2.79e-7 / 2.29e-7 | 1.62e-7   2.33e-7 / 1.42e-7 | 1.87e-7   2.98e-7 / 2.20e-7 | 1.44e-7
        15  2.63e-7 / 2.90e-7 | 1.58e-7   2.97e-7 / 1.85e-7 | 1.67e-7   2.97e-7 / 3.36e-7 | 1.53e-7
        31  2.18e-7 / 2.02e-7 | 2.21e-7   2.10e-7 / 1.39e-7 | 1.67e-7   2.08e-7 / 2.35e-7 | 1.71e-7
    so the kernel sits at 0.3 .. 0.6 of its bar everywhere.  (Against bc.cov_float64, every operation in float64, the kernel's interior error is 0.9e-7 .. 2.2e-7:
    part of the figures above is the reference's own fp32 weights.)"""
    from macvo_amd import ops

    c = bc.cov_cases()
    depth, kp = _dev(c, gpu, "depth", "kp")
    fc = c["sigma_nan"].to(gpu)
    cov, st = ops.match_cov(depth, kp, fc, None, *c["K4"], kernel_size=K, want_stats=True)
    want = c["sigma_nan"].clone()
    want[:, :2].clamp_(min=0.0625)
    assert torch.equal(fc.cpu(), want) and cov.dtype == torch.float64
    assert cov[5].isnan().all() and st[5].isnan().all()
    _check("interior", K, (cov, st[:, 0], st[:, 1]), bc.cov_reference(K, "interior"))
    t = bc.cov_float64(c["kp"], c["depth"], c["sigma_nan"], c["K4"], K)
    print(f"   against the all-float64 restatement: cov {bc.block_err(cov.cpu(), t[0]):.3e} wavg {bc.rel_err(st[:, 0].cpu(), t[1]):.3e} "
          f"wvar {bc.rel_err(st[:, 1].cpu(), t[2]):.3e}")

    kb = c["border"][K]
    sb = c["sigma_nan"][: kb.shape[0]]
    cov_b, st_b = ops.match_cov(depth, kb.to(gpu), sb.to(gpu), None, *c["K4"], kernel_size=K, want_stats=True)
    _check("border", K, (cov_b, st_b[:, 0], st_b[:, 1]), bc.cov_reference(K, "border"))
    # border identity, bitwise: the index clamp is the edge-replicated map (all coordinates are multiples of 0.25: u - cx is exact in both)
    cov_p, st_p = ops.match_cov(bc.replicate_pad(c["depth"]).to(gpu), (kb + bc.PAD).to(gpu), sb.to(gpu), None, *bc.shifted(c["K4"]), kernel_size=K,
                                want_stats=True)
    assert torch.equal(torch.nan_to_num(cov_b, 7.0).view(torch.int64), torch.nan_to_num(cov_p, 7.0).view(torch.int64))
    assert torch.equal(torch.nan_to_num(st_b, 7.0).view(torch.int32), torch.nan_to_num(st_p, 7.0).view(torch.int32))


def test_match_cov_pair_second_set_at_the_border(gpu):
    """ops.match_cov_pair at K = 9 with the border keypoints as set 1 (blockIdx.y = 1) on the map and set 0 on its mirror image: set 1 within the float64 bar,
    both sets bitwise what the padded call gives, and set 1 bitwise the single call.  Measured on an MI355X: set 1 cov 2.29e-7, e_ref 1.62e-7."""
    from macvo_amd import ops

    K = 9
    c = bc.cov_cases()
    kb = c["border"][K]
    sb = c["sigma_nan"][: kb.shape[0]]
    d1, d0 = c["depth"], c["depth"].flip(-1).contiguous()

    def run(pad):
        m0, m1, k, K4 = (bc.replicate_pad(d0), bc.replicate_pad(d1), kb + bc.PAD, bc.shifted(c["K4"])) if pad else (d0, d1, kb, c["K4"])
        s0, s1 = sb.to(gpu), sb.to(gpu)
        c0, _, c1 = ops.match_cov_pair(m0.to(gpu), k.to(gpu), s0, m1.to(gpu), k.to(gpu), s1, *K4, kernel_size=K)
        return c0, c1, s0, s1

    a0, a1, s0, s1 = run(False)
    b0, b1, _, _ = run(True)
    ref = bc.cov_reference(K, "border")
    e = bc.block_err(a1.cpu(), ref[0])
    print(f"pair set 1 K={K}: kernel cov {e:.3e} | e_ref {bc.cov_e_ref(K)[0]:.3e}")
    assert e <= bc.cov_bar(K)[0]
    for x, y in ((a0, b0), (a1, b1)):
        assert torch.equal(torch.nan_to_num(x, 7.0).view(torch.int64), torch.nan_to_num(y, 7.0).view(torch.int64))
    single = ops.match_cov(d1.to(gpu), kb.to(gpu), sb.to(gpu), None, *c["K4"], kernel_size=K)
    assert torch.equal(torch.nan_to_num(a1, 7.0), torch.nan_to_num(single, 7.0)) and not torch.equal(torch.nan_to_num(a0, 7.0), torch.nan_to_num(a1, 7.0))
    want = sb.clone()
    want[:, :2].clamp_(min=0.0625)
    assert torch.equal(s0.cpu(), want) and torch.equal(s1.cpu(), want)


def test_gaussian_mixture_at_the_border(gpu):
    """ops.obs_cov("gmm", ...) (the wrapper tests/test_gpu_cov_models.py uses) at K = 9 on the border keypoints: bitwise the call on the padded maps, and within
    4 x max(e_ref, 2^-23) of tests/cov_models_ref.gmm_covariance on float64 tensors, e_ref = the same restatement in fp32 against it on the interior keypoints (the
    mixture variance E[c + z^2] - mean^2 cancels in fp32, and e_ref carries that).  No weight of the reference lies within 1e-4 (relative) of the model's 1e-3
    threshold, so no tap can flip.  Measured on an MI355X: cov interior 6.36e-5, border 2.90e-5, e_ref 2.89e-5 (bar 1.16e-4)."""
    from macvo_amd import ops

    K = 9
    c = bc.cov_cases()
    kb = c["border"][K]
    sb = c["sigma_nan"][: kb.shape[0]]

    def gmm(kp, depth, dcov, sigma, K4, dtype):
        out, w = cov_models_ref.gmm_covariance(kp.to(dtype), depth.to(dtype), dcov.to(dtype), None, sigma.clone().to(dtype), *K4, kernel_size=K,
                                               return_weights=True)
        assert ((w[~w.isnan()] / 1e-3 - 1).abs() > 1e-4).all()
        return out

    r64 = gmm(c["kp"], c["depth"], c["depth_cov"], c["sigma_nan"], c["K4"], torch.float64)
    e_ref = bc.block_err(gmm(c["kp"], c["depth"], c["depth_cov"], c["sigma_nan"], c["K4"], torch.float32), r64)
    ref_b = gmm(kb + bc.PAD, bc.replicate_pad(c["depth"]), bc.replicate_pad(c["depth_cov"]), sb, bc.shifted(c["K4"]), torch.float64)

    depth, dcov = _dev(c, gpu, "depth", "depth_cov")
    cov_i = ops.obs_cov("gmm", depth, c["kp"].to(gpu), c["sigma_nan"].to(gpu), None, *c["K4"], depth_cov_map=dcov, kernel_size=K)
    cov_b, st_b = ops.obs_cov("gmm", depth, kb.to(gpu), sb.to(gpu), None, *c["K4"], depth_cov_map=dcov, kernel_size=K, want_stats=True)
    cov_p, st_p = ops.obs_cov("gmm", bc.replicate_pad(c["depth"]).to(gpu), (kb + bc.PAD).to(gpu), sb.to(gpu), None, *bc.shifted(c["K4"]),
                              depth_cov_map=bc.replicate_pad(c["depth_cov"]).to(gpu), kernel_size=K, want_stats=True)
    e_i, e_b = bc.block_err(cov_i.cpu(), r64), bc.block_err(cov_b.cpu(), ref_b)
    print(f"gmm K={K}: kernel cov interior {e_i:.3e} border {e_b:.3e} | e_ref {e_ref:.3e}")
    assert max(e_i, e_b) <= 4 * max(e_ref, 2.0 ** -23)
    assert torch.equal(torch.nan_to_num(cov_b, 7.0).view(torch.int64), torch.nan_to_num(cov_p, 7.0).view(torch.int64))
    assert torch.equal(torch.nan_to_num(st_b, 7.0).view(torch.int32), torch.nan_to_num(st_p, 7.0).view(torch.int32))


def test_match_cov_rejects_kernel_sizes_before_any_launch(gpu):
    from macvo_amd import _lib as L
    from macvo_amd import ops

    c = bc.cov_cases()
    depth, kp = _dev(c, gpu, "depth", "kp")
    for K, what in ((33, "unsupported"), (4, "invalid argument")):
        fc = c["sigma"].to(gpu)
        with pytest.raises(L.MacvoHipError, match=what):
            ops.match_cov(depth, kp, fc, None, *c["K4"], kernel_size=K)
        with pytest.raises(L.MacvoHipError, match=what):
            ops.match_cov_pair(depth, kp, fc, depth, kp, fc, *c["K4"], kernel_size=K)
        with pytest.raises(L.MacvoHipError, match=what):
            ops.obs_cov("gmm", depth, kp, fc, None, *c["K4"], depth_cov_map=depth, kernel_size=K)
        assert torch.equal(fc.cpu(), c["sigma"])          # nothing ran: not even the in-place clamp


@pytest.mark.parametrize("nprob_pad", [0, 520])
@pytest.mark.parametrize("graph", bc.GRAPHS)
def test_pgo_outside_the_generator_domain(gpu, graph, nprob_pad):
    """All pgo_cases() in one batch per graph through ops.pgo_solve.  Against oracle.pgo.solve: steps equal, pose <= 1e-8 m / 1e-8 rad, loss rel 1e-8 (the bars
    of test_pgo_matches_oracle); against the host twin: steps and reject counts equal, pose atol 1e-11, loss rtol 1e-11 (the bars of
    test_pgo_kernel_equals_host_twin).  nprob_pad = 520 appends small problems so that the one-wave kernel solves the same cases.
    indef in the far frame is the case that needs gauss_solve6 (pgo_math.h): its second step's J^T W J has a negative eigenvalue, where the reference's PINV solver
    steps on and a Cholesky-only solve stopped after 3 steps instead of 10 (disp) with the pose 2.7e-2 m off.
    Measured on an MI355X, worst over the 27 cases (pad 0 / 520): against the oracle disp 6.9e-14 m 4.0e-15 rad, reproj 3.4e-13 / 1.4e-13 m 1.9e-14 rad,
    icp 2.1e-14 m 9.4e-16 rad; against the twin pose <= 1.0e-13, loss rel <= 2.4e-12."""
    from macvo_amd import ops
    from oracle import se3
    from tests import pgo_twin
    from tests.test_gpu_backend import _to_batch

    cases = bc.pgo_cases()
    probs = [c[2] for c in cases] + (bc.pgo_padding(nprob_pad) if nprob_pad else [])
    pose, info = ops.pgo_solve(_to_batch(probs, gpu), graph)
    pose, info = pose.cpu(), info.cpu()
    pose_t, info_t = pgo_twin.solve(_to_batch(probs, torch.device("cpu")), graph)
    worst = [0.0, 0.0]
    for k, (name, frame, _, _) in enumerate(cases):
        ref = bc.pgo_oracle(k, graph)
        dt, dr = se3.pose_error(ref.pose, pose[k])
        worst = [max(worst[0], dt), max(worst[1], dr)]
        assert int(info[k, 1]) == ref.steps, (name, frame, info[k].tolist(), ref.steps)
        assert dt <= 1e-8 and dr <= 1e-8, (name, frame, dt, dr)
        assert info[k, 0].item() == pytest.approx(ref.loss, rel=1e-8, abs=1e-12), (name, frame)
    print(f"{graph} pad={nprob_pad}: against the oracle {worst[0]:.2e} m {worst[1]:.2e} rad; against the twin pose {(pose - pose_t).abs().max():.2e}, "
          f"loss rel {((info[:, 0] - info_t[:, 0]).abs() / info_t[:, 0].abs()).max():.2e}")
    assert torch.equal(info[:, 1:3], info_t[:, 1:3]), (info[:27], info_t[:27])
    torch.testing.assert_close(pose, pose_t, rtol=0, atol=1e-11)
    torch.testing.assert_close(info[:, 0], info_t[:, 0], rtol=1e-11, atol=1e-13)
