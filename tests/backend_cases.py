"""TEST INFRASTRUCTURE: seeded inputs that take the covariance model (mv_match_cov, match_cov_dev.h) and the PGO solve (mv_pgo_solve*, pgo_math.h)
outside the one point of their input domain that ``synth.keypoints(border=32)`` / ``oracle.pgo.make_synthetic_problem`` reach, and the CPU references of
both.  Imports the oracle only, nothing of the product; the references are computed once per process and shared by tests/test_backend_domain_host.py
(CPU) and tests/test_gpu_backend_domain.py (GPU)."""
from __future__ import annotations

import copy
import functools

import torch
import torch.nn.functional as F

from oracle import covariance, pgo, se3

# ------------------------------------------------------------------------------------------------------------------- PGO
GRAPHS = ("disp", "reproj", "icp")
EDIT_ROWS = 20
# rigid moves of a whole problem: name -> (t, q before normalisation); "far" is about 47 m away with a ~110 deg rotation, "pi" is rotated to within 2e-4 rad of pi
FRAMES = {"id": None, "far": ((40.0, -25.0, 3.0), (0.5, -0.6, 0.3, 0.55)), "pi": ((5.0, 5.0, 5.0), (0.0, 0.0, 1.0, 1e-4))}


def _move(prob: pgo.PGOProblem, frame: str) -> pgo.PGOProblem:
    """The same problem seen from a world moved by T (the pattern of tests/golden/make_golden_local_keyframe.py): pos_Tw = T p rounded to fp32,
    cov_Tw = R cov R^T, init_pose = T (the generator's prior is the identity).  T is the fp32 pose both solvers are handed, widened to fp64."""
    prob = copy.deepcopy(prob)
    if FRAMES[frame] is None:
        return prob
    t, q = FRAMES[frame]
    q = torch.tensor(q, dtype=torch.float64)
    T32 = torch.cat([torch.tensor(t, dtype=torch.float64), q / q.norm()]).float()
    T = T32.double()
    assert torch.equal(prob.init_pose, torch.tensor([0, 0, 0, 0, 0, 0, 1], dtype=torch.float32))
    R = se3.quat_to_matrix(T[3:])
    prob.pos_Tw = se3.se3_act(T, prob.pos_Tw.double()).float()
    prob.cov_Tw = R @ prob.cov_Tw @ R.transpose(-1, -2)
    prob.init_pose = T32
    return prob


def _edited(name: str, n: int) -> pgo.PGOProblem:
    kw = dict(trans_sigma=1.0, rot_sigma=0.3) if name == "bigstep" else {}
    prob = pgo.make_synthetic_problem(n=n, seed=6, **kw)[0]
    uvc, m = prob.pixel2_uv_cov, EDIT_ROWS            # [N,3] fp32 (uu, vv, uv)
    geo = (uvc[:, 0] * uvc[:, 1]).sqrt()
    if name == "corr":                                # the off-diagonal term w01 = -c / det, every row
        g = torch.Generator().manual_seed(600 + n)
        sign = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
        uvc[:, 2] = sign * 0.8 * geo
    elif name == "rank1":                             # exactly singular in fp32 and fp64 (l2 == 0): the rank-1 projector branch
        uvc[:m] = torch.tensor([4.0, 1.0, 2.0])
    elif name == "zero_uv":                           # the all-zero 2x2 branch; w22 = 1 / s3 kept
        uvc[:m] = 0.0
    elif name == "zero_all":                          # ... and w22 = 0
        uvc[:m] = 0.0
        prob.pixel2_disp_cov[:m] = 0.0
    elif name == "tiny":                              # full rank at 1e-12: no absolute cutoff anywhere
        uvc[:m] *= 1e-12
    elif name == "indef":                             # negative eigenvalue: the pseudo-inverse is the plain (indefinite) inverse
        uvc[:m, 2] = 1.5 * geo[:m]
    else:
        assert name == "bigstep", name                # first LM step has |phi| > 0.1: the closed-form branch of se3_left_update
    # Left out on purpose: s_uv = float32(sqrt(s_uu * s_vv)).  Its covariance has a condition number of about 1e7; there the oracle's PINV step and the
    # kernel's Cholesky step legitimately part ways (on the CPU the host twin ended at loss 192, the oracle at 594): chaos, not a bug, so it is no test.
    return prob


@functools.lru_cache(maxsize=None)
def pgo_cases():
    """[(name, frame, problem, graphs)]: every edit of the table above in the three frames; ``graphs`` = the graphs that read what the case edits
    (disp and reproj for the covariance edits in the unmoved frame, all three for bigstep and for the moved frames).  n = 60 (one point per thread),
    plus n = 300 for corr and rank1 (N > 256: the several-points-per-thread 55-value build)."""
    out = []
    for name, n in (("corr", 60), ("corr", 300), ("rank1", 60), ("rank1", 300), ("zero_uv", 60), ("zero_all", 60), ("tiny", 60), ("indef", 60),
                    ("bigstep", 60)):
        base = _edited(name, n)
        for frame in FRAMES:
            graphs = GRAPHS if (frame != "id" or name == "bigstep") else ("disp", "reproj")
            out.append((f"{name}{n}", frame, _move(base, frame), graphs))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pgo_oracle(index: int, graph: str) -> pgo.PGOResult:
    """oracle.pgo.solve of pgo_cases()[index], once per process."""
    return pgo.solve(pgo_cases()[index][2], graph)


def pgo_padding(count: int = 520):
    """Small problems that push a batch over the 512-problem switch to the one-wave kernel (as test_pgo_kernel_equals_host_twin does)."""
    return [pgo.make_synthetic_problem(n=20 + (k % 7), seed=100 + k)[0] for k in range(count)]


# ------------------------------------------------------------------------------------------------------------------- covariance model
COV_KS = (1, 3, 7, 9, 15, 31)
PAD = 16                                              # >= 31 // 2: every tap of every border keypoint lies inside the padded map
MIN_DEPTH_COV = 0.05                                  # the default of ops.match_cov / oracle.covariance.match_covariance


def replicate_pad(depth: torch.Tensor) -> torch.Tensor:
    return F.pad(depth, (PAD, PAD, PAD, PAD), mode="replicate")


def border_keypoints(K: int, H: int, W: int) -> torch.Tensor:
    """Keypoints whose patches leave the map: corners, edge midpoints, h - 1 and h pixels inside each edge (h = K // 2: the last patch that is clipped and
    the first that is not), two fractional ones; all u, v >= 0 (``.long()`` truncates toward zero) and multiples of 0.25."""
    h = K // 2
    mu, mv = W / 2 + 0.25, H / 2 - 0.75
    pts = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (mu, 0), (mu, H - 1), (0, mv), (W - 1, mv)]
    for d in (h - 1, h):
        if d >= 0:                                    # (K = 1: there is no pixel "-1 inside" an edge)
            pts += [(d, mv), (W - 1 - d, mv), (mu, d), (mu, H - 1 - d)]
    pts += [(1.5, 2.5), (W - 1.25, H - 1.75)]
    kp = torch.tensor(pts, dtype=torch.float32)
    assert (kp * 4 == (kp * 4).round()).all() and (kp >= 0).all() and (kp[:, 0] <= W - 1).all() and (kp[:, 1] <= H - 1).all()
    return kp


@functools.lru_cache(maxsize=None)
def cov_cases() -> dict:
    """depth / depth_cov [1,1,96,128] fp32 (textured: the patch variance clears min_depth_cov on most rows, unlike synth.depth_maps), kp [61,2] (61 = 15 * 4 + 1:
    the last workgroup has one live wave) on the 0.25 grid inside [16, W - 16) x [16, H - 16), sigma [61,3] correlated and positive definite with rows 0..4
    below the 0.0625 clamp, sigma_nan = sigma with row 5 indefinite (NaN row), K4 with a principal point on the 0.25 grid, border[K] keypoints."""
    H, W, n = 96, 128, 61
    g = torch.Generator().manual_seed(4096)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = (6.0 + 2.0 * torch.sin(xx / 5.0) * torch.cos(yy / 7.0) + 3.0 * torch.rand(H, W, generator=g)).reshape(1, 1, H, W)
    depth_cov = (0.02 + 0.3 * torch.rand(H, W, generator=g)).reshape(1, 1, H, W)
    kp = torch.stack([torch.randint(4 * PAD, 4 * (W - PAD), (n,), generator=g), torch.randint(4 * PAD, 4 * (H - PAD), (n,), generator=g)], 1).float() / 4
    sigma = torch.exp(2 * 0.5 * torch.randn(n, 3, generator=g))
    sigma[:5, 0] = 0.01
    sigma[1:3, 1] = 0.02
    rho = 1.6 * torch.rand(n, generator=g) - 0.8
    sigma[:, 2] = rho * (sigma[:, 0].clamp(min=0.0625) * sigma[:, 1].clamp(min=0.0625)).sqrt()     # positive definite after the clamp too
    sigma_nan = sigma.clone()
    sigma_nan[5] = torch.tensor([0.3, 0.3, 0.5])
    K4 = (100.0, 100.0, 63.5, 47.25)
    return dict(H=H, W=W, depth=depth, depth_cov=depth_cov, kp=kp, sigma=sigma, sigma_nan=sigma_nan, K4=K4,
                border={K: border_keypoints(K, H, W) for K in COV_KS})


def shifted(K4):
    return (K4[0], K4[1], K4[2] + PAD, K4[3] + PAD)


def cov_oracle(kp, depth, sigma, K4, K: int, dtype):
    """oracle.covariance.match_covariance in fp32 (the reference's arithmetic) or on float64 tensors -> (cov [N,3,3] f64, wavg, wvar)."""
    cov, aux = covariance.match_covariance(kp.to(dtype), depth.to(dtype), None, sigma.clone().to(dtype), *K4, kernel_size=K, return_aux=True)
    return cov, aux["wavg"], aux["wvar"]


def cov_float64(kp, depth, sigma, K4, K: int, min_flow_cov: float = 0.25):
    """MatchCovariance with every operation in float64, weights included (the oracle on float64 tensors still builds its Gaussian weights in fp32): the
    yardstick of that reference itself, never a test's bar."""
    kp, z, s = kp.double(), depth.double()[0, 0], sigma.clone().double()
    s[:, :2].clamp_(min=min_flow_cov ** 2)
    off = torch.arange(-(K // 2), K // 2 + 1)
    a, b = [t[None] for t in torch.meshgrid(off, off, indexing="ij")]
    suu, svv, suv = [s[:, i, None, None] for i in range(3)]
    det = suu * svv - suv * suv
    q = -0.5 * ((svv * a * a - 2 * suv * a * b + suu * b * b) / det)      # the kernel transposed against the patch: a (the patch row offset) meets sigma_uu
    w = q.exp() / (2 * torch.pi * det.sqrt())
    w = w / w.sum((1, 2), keepdim=True)
    kl = kp.long()
    patch = z[kl[:, 1, None, None] + a, kl[:, 0, None, None] + b]
    wavg = (w * patch).sum((1, 2))
    wvar = (w * (patch - wavg[:, None, None]).square()).sum((1, 2)).clamp(min=MIN_DEPTH_COV)
    fx, fy, cx, cy = K4
    du, dv, d2, (suu, svv, suv) = kp[:, 0] - cx, kp[:, 1] - cy, wavg.square(), s.unbind(1)
    sxx = (du.square() * wvar + d2 * suu + suu * wvar) / fx ** 2
    syy = (dv.square() * wvar + d2 * svv + svv * wvar) / fy ** 2
    sxy = (du * dv * wvar + (d2 + wvar) * suv) / (fx * fy)
    sxz, syz = wvar * du / fx, wvar * dv / fy
    cov = torch.stack([wvar, sxz, syz, sxz, sxx, sxy, syz, sxy, syy], -1).reshape(-1, 3, 3)     # NED order (z, x, y)
    return cov, wavg, wvar


@functools.lru_cache(maxsize=None)
def cov_reference(K: int, which: str):
    """The float64 reference of cov_cases(): "interior" = the oracle on (kp, sigma_nan); "border" = the oracle on the map replicate-padded by 16 with the
    border keypoints and the principal point shifted by 16 — an index clamp is the same as an edge-replicated map (test_backend_domain_host.py proves the
    two forms bit-equal where both exist) — with sigma_nan's first rows as the match covariance."""
    c = cov_cases()
    if which == "interior":
        return cov_oracle(c["kp"], c["depth"], c["sigma_nan"], c["K4"], K, torch.float64)
    kb = c["border"][K]
    return cov_oracle(kb + PAD, replicate_pad(c["depth"]), c["sigma_nan"][: kb.shape[0]], shifted(c["K4"]), K, torch.float64)


def block_err(x: torch.Tensor, ref: torch.Tensor) -> float:
    """Covariance norm: per keypoint, max-abs of the 3 x 3 difference over max-abs of the reference block; the largest over the rows.  NaN rows must be the
    same rows, entirely NaN, on both sides."""
    x, ref = x.double(), ref.double()
    nan = ref.isnan().flatten(1).any(1)
    assert torch.equal(x.isnan().flatten(1).all(1), nan) and torch.equal(ref.isnan().flatten(1).all(1), nan)
    e = (x - ref)[~nan].abs().amax((1, 2)) / ref[~nan].abs().amax((1, 2))
    return float(e.max())


def rel_err(x: torch.Tensor, ref: torch.Tensor) -> float:
    """Plain relative error (wavg, wvar), NaN rows equal on both sides."""
    x, ref = x.double(), ref.double()
    nan = ref.isnan()
    assert torch.equal(x.isnan(), nan)
    return float(((x - ref)[~nan].abs() / ref[~nan].abs()).max())


@functools.lru_cache(maxsize=None)
def cov_e_ref(K: int):
    """(cov, wavg, wvar) distance of the fp32 oracle from the float64 one on the interior inputs: what one fp32 evaluation costs at this K."""
    c = cov_cases()
    r64 = cov_reference(K, "interior")
    r32 = cov_oracle(c["kp"], c["depth"], c["sigma_nan"], c["K4"], K, torch.float32)
    return block_err(r32[0], r64[0]), rel_err(r32[1], r64[1]), rel_err(r32[2], r64[2])


def cov_bar(K: int):
    """4 x max(e_ref, 2^-23) per quantity: a factor 2 for two independent fp32 evaluations, a factor 2 for the wave-tree sum order and device expf."""
    return tuple(4.0 * max(e, 2.0 ** -23) for e in cov_e_ref(K))


def textured_fraction(K: int) -> float:
    """Share of the interior keypoints (positive definite sigma) whose float64 patch variance clears min_depth_cov, i.e. does not sit on the clamp."""
    c = cov_cases()
    _, _, wvar = cov_oracle(c["kp"], c["depth"], c["sigma"], c["K4"], K, torch.float64)
    return float((wvar > MIN_DEPTH_COV).double().mean())
