"""GPU: the evaluation kernels (csrc/eval_metrics.hip through ops.eval_flow / ops.eval_depth, evaluation.FrontendEvaluator and the four
reference entry points) against tests/eval_ref.py on the CPU.

What is exact: the per-pixel error planes (bit-equal, NaN-equal), every count, px1/3/5, every threshold and err_25/50/75 (the select is exact and
the per-pixel values are bit-equal), the grids.  What carries a tolerance:
  * per-pixel nll: <= 4 ulp of max(|log det|, m) (device logf and host logf are each about 1 ulp off; the sum's rounding moves with them).
    Measured on the MI355X over the cases below: see NLL_ULP_MEASURED.
  * means of bit-equal terms (masked_epe, epe, masked_err): within 1 fp32 ulp of the fp64 reference mean.
  * NLL means: within 4 x the distance of eval_ref's own fp32 route from the fp64 closed form on that input, floor 2^-22 * mean|term|.
"""
import math
import os

import numpy as np
import pytest
import torch

from tests import eval_ref as ER

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
NLL = ("masked_nll", "q25_nll", "q50_nll", "q75_nll")
# worst per-pixel |nll_gpu - nll_ref| in ulp of max(|log det|, m), measured on the MI355X over every case of this file (bound: 4).  The distances come
# in steps of ulp(nll) = up to 2 ulp of that scale: 0, 1, 2 and 4 were seen, 4 in 9 of the 22 cases with a covariance (two logf results 1 ulp apart on
# either side of a rounding boundary of the sum); more than 4 needs a logf that is more than 1 ulp off.
NLL_ULP_MEASURED = 4.0


# ------------------------------------------------------------------------------------------------ cases
def flow_case(H, W, seed, lanes=1, cov=True, valid=True, max_flow=6.0, apply_max_flow=True, nan_frac=0.03, edit=None):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randn(lanes, 2, H, W, generator=g) * 4
    est = gt + torch.randn(lanes, 2, H, W, generator=g) * torch.exp(torch.randn(lanes, 2, H, W, generator=g))
    c = dict(kind="flow", est=est, gt=gt, cov=None, valid=None, maxv=max_flow, apply=apply_max_flow)
    if cov:
        c["cov"] = torch.cat([torch.exp(torch.randn(lanes, 2, H, W, generator=g) * 1.5), torch.zeros(lanes, 1, H, W)], 1)
    if valid:
        c["valid"] = torch.rand(lanes, 1, H, W, generator=g) > 0.15
    gt[torch.rand(lanes, 2, H, W, generator=g) < nan_frac] = NAN
    if edit:
        edit(c, g)
    return c


def depth_case(H, W, seed, lanes=1, cov=True, max_depth=30.0, nan_frac=0.03, edit=None):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(lanes, 1, H, W, generator=g) * 40 + 0.5
    est = gt + torch.randn(lanes, 1, H, W, generator=g) * torch.exp(torch.randn(lanes, 1, H, W, generator=g))
    c = dict(kind="depth", est=est, gt=gt, cov=None, maxv=max_depth)
    if cov:
        c["cov"] = torch.exp(torch.randn(lanes, 1, H, W, generator=g) * 1.5)
    gt[torch.rand(lanes, 1, H, W, generator=g) < nan_frac] = NAN
    if edit:
        edit(c, g)
    return c


def _quantised(c, g):       # 8 distinct uncertainties: every rank falls inside a run of ties, and `<` must stay strict
    lv = torch.tensor([0.25, 0.5, 0.5, 1.0, 2.0, 2.0, 4.0, 8.0])
    pick = torch.randint(0, 8, c["cov"][:, :1].shape, generator=g)
    if c["kind"] == "flow":
        c["cov"][:, 0:1] = lv[pick]
        c["cov"][:, 1:2] = 1.0
    else:
        c["cov"] = lv[pick]


def _infs(c, g):            # 40 % +inf uncertainties (t75 between two +inf = NaN), a few -inf / +inf errors
    m = torch.rand(c["cov"][:, :1].shape, generator=g) < 0.4
    c["cov"][:, 0:1][m] = INF
    c["est"].flatten()[::17] = INF
    c["gt"].flatten()[5::29] = -INF


def _odd_variances(c, g):   # zero, tiny-ratio and negative variances
    f = c["cov"][:, 0:1].flatten().clone()
    f[0::11] = 0.0
    f[1::11] = -f[1::11]
    f[2::11] = 1e-20
    if c["kind"] == "flow":
        f2 = c["cov"][:, 1:2].flatten().clone()
        f2[0::22] = 0.0
        f2[2::11] = 1.0
        f2[3::11] = -0.0
        c["cov"][:, 1:2] = f2.reshape(c["cov"][:, 1:2].shape)
    c["cov"][:, 0:1] = f.reshape(c["cov"][:, 0:1].shape)


def _all_nan_cov(c, g):
    c["cov"][:] = NAN


CASES = {
    "flow_37x53": lambda: flow_case(37, 53, 1),
    "flow_37x53_nocov_novalid": lambda: flow_case(37, 53, 2, cov=False, valid=False),
    "flow_37x53_gtmask": lambda: flow_case(37, 53, 3, apply_max_flow=False),
    "flow_36x52_vec": lambda: flow_case(36, 52, 4),                                  # H * W % 4 == 0: the 16-byte load path
    "flow_5x5": lambda: flow_case(5, 5, 5, nan_frac=0.0, valid=False, max_flow=1e9),   # n = 4k + 1: weight 0, less than one wavefront
    "flow_1x1": lambda: flow_case(1, 1, 6, nan_frac=0.0, valid=False, max_flow=1e9),
    "flow_quantised": lambda: flow_case(36, 52, 7, edit=_quantised),
    "flow_infs": lambda: flow_case(37, 53, 8, edit=_infs),
    "flow_odd_variances": lambda: flow_case(37, 53, 9, edit=_odd_variances),
    "flow_all_nan_cov": lambda: flow_case(20, 24, 10, edit=_all_nan_cov),
    "flow_empty_mask": lambda: flow_case(20, 24, 11, max_flow=-1e9),
    "flow_3lanes": lambda: flow_case(37, 53, 12, lanes=3),
    "flow_480x640_2lanes": lambda: flow_case(480, 640, 13, lanes=2, max_flow=8.0),
    "depth_37x53": lambda: depth_case(37, 53, 21),
    "depth_37x53_nocov": lambda: depth_case(37, 53, 22, cov=False),
    "depth_36x52_vec": lambda: depth_case(36, 52, 23),
    "depth_5x5": lambda: depth_case(5, 5, 24, nan_frac=0.0, max_depth=1e9),
    "depth_1x1": lambda: depth_case(1, 1, 25, nan_frac=0.0, max_depth=1e9),
    "depth_quantised": lambda: depth_case(36, 52, 26, edit=_quantised),
    "depth_infs": lambda: depth_case(37, 53, 27, edit=_infs),
    "depth_odd_variances": lambda: depth_case(37, 53, 28, edit=_odd_variances),
    "depth_all_nan_cov": lambda: depth_case(20, 24, 29, edit=_all_nan_cov),
    "depth_empty_mask": lambda: depth_case(20, 24, 30, max_depth=-1e9),
    "depth_empty_mask_nocov": lambda: depth_case(20, 24, 31, cov=False, max_depth=-1e9),
    "depth_3lanes": lambda: depth_case(37, 53, 32, lanes=3),
    "depth_480x640_2lanes": lambda: depth_case(480, 640, 33, lanes=2),
}
_case_cache: dict = {}


def get_case(name):
    """The case and its CPU reference, computed once and shared by the tests that need it (never modified)."""
    if name not in _case_cache:
        c = CASES[name]()
        refs, grids = [], None
        lanes = c["est"].shape[0]
        if c["cov"] is not None:
            grids = np.zeros((lanes, 2, 100, 100) if c["kind"] == "flow" else (lanes, 100, 100), np.uint32)
        for l in range(lanes):
            refs.append(ref_lane(c, l, None if grids is None else grids[l]))
        _case_cache[name] = (c, refs, grids)
    return _case_cache[name]


def ref_lane(c, l, grid):
    cov = None if c["cov"] is None else c["cov"][l]
    if c["kind"] == "flow":
        fr = ER.flow_frame(c["est"][l], c["gt"][l], cov, None if c["valid"] is None else c["valid"][l, 0], c["maxv"], c["apply"], grid)
        if cov is not None:
            fr["m64"] = ER.nll_means64("flow", c["est"][l], c["gt"][l], cov[:2], fr)
            fr["scale_px"] = ER.nll_scale("flow", c["est"][l], c["gt"][l], cov[:2])
    else:
        fr = ER.depth_frame(c["est"][l, 0], c["gt"][l, 0], None if cov is None else cov[0], c["maxv"], grid)
        if cov is not None:
            fr["m64"] = ER.nll_means64("depth", c["est"][l, 0], c["gt"][l, 0], cov[0], fr)
            fr["scale_px"] = ER.nll_scale("depth", c["est"][l, 0], c["gt"][l, 0], cov[0])
    return fr


# ------------------------------------------------------------------------------------------------ running and checking
def run_case(c, dev, rows=None, row=0, grids=None):
    from macvo_amd import ops

    d = lambda t: None if t is None else t.to(dev)   # noqa: E731
    if c["kind"] == "flow":
        r = ops.eval_flow(d(c["est"]), d(c["gt"]), d(c["cov"]), d(c["valid"]), c["maxv"], c["apply"], rows=rows, row=row, grids=grids, planes=True)
    else:
        r = ops.eval_depth(d(c["est"]), d(c["gt"]), d(c["cov"]), c["maxv"], rows=rows, row=row, grids=grids, planes=True)
    return dict(row=r.row.cpu().numpy(), grids=None if r.grids is None else r.grids.cpu().numpy().view(np.uint32), err=r.err.cpu(),
                nll=None if r.nll is None else r.nll.cpu(), res=r)


def same(a, b):
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or a == b


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal as fp32 values, NaN matching NaN (-0.0 == +0.0)."""
    return bool((((a == b) | (torch.isnan(a) & torch.isnan(b)))).all())


def check_planes(kind, ref, err_px, nll_px, stats):
    """The per-pixel stage on its own: error bit-equal, nll within 4 ulp of max(|log det|, m)."""
    assert bits_equal(err_px, ref["epe_px" if kind == "flow" else "err_px"])
    if ref["nll_px"] is None:
        return
    a, b = nll_px, ref["nll_px"]
    assert bool((torch.isnan(a) == torch.isnan(b)).all())
    fin = torch.isfinite(b)
    inf = ~fin & ~torch.isnan(b)
    assert bool((a[inf] == b[inf]).all())
    if fin.any():
        ulp = np.spacing(ref["scale_px"][fin].numpy().astype(np.float32)).astype(np.float64)
        d = float(((a[fin].double() - b[fin].double()).abs().numpy() / ulp).max())
        stats["nll_ulp"] = max(stats.get("nll_ulp", 0.0), d)
        print(f"nll per-pixel distance: {d:.3f} ulp of max(|log det|, m)")
        assert d <= 4.0


def nll_mean_tolerance(ref, k):
    """4 x the distance of eval_ref's fp32 route from the fp64 closed form on this input, floor 2^-22 * mean|term|."""
    pop = ref["mask_px"] if k == "masked_nll" else ref["unc_px"] < ref["t" + k[1:3]]
    t = ref["nll_px"][pop]
    t = t[~torch.isnan(t)]
    mean_abs = float(t.abs().double().mean()) if t.numel() else 0.0
    if not (math.isfinite(ref[k]) and math.isfinite(ref["m64"][k]) and math.isfinite(mean_abs)):
        return 0.0, mean_abs
    return max(4 * abs(ref[k] - ref["m64"][k]), 2.0 ** -22 * mean_abs), mean_abs


def check_row(kind, cols, row, ref):
    r = dict(zip(cols, (float(x) for x in row)))
    has_cov = ref["nll_px"] is not None
    # counts, rates, thresholds, order statistics: exact
    exact = ["n_mask", "n_mask_finite", "n_finite", "n_q25", "n_q50", "n_q75", "n_mask_nll", "t25", "t50", "t75"]
    exact += ["px1", "px3", "px5"] if kind == "flow" else ["err_25", "err_50", "err_75"]
    for k in exact:
        print(f"{k}: gpu {r[k]!r} ref {ref[k]!r}")
        assert same(r[k], ref[k]), k
    # means of bit-equal terms: within 1 fp32 ulp of the fp64 mean
    for k in (("masked_epe", "epe") if kind == "flow" else ("masked_err",)):
        print(f"{k}: gpu {r[k]!r} ref {ref[k]!r}")
        assert same(r[k], ref[k]) or abs(r[k] - ref[k]) <= float(np.spacing(np.float32(abs(ref[k])))), k
    for k in NLL:
        if not has_cov:
            assert math.isnan(r[k]), k
            continue
        tol, _ = nll_mean_tolerance(ref, k)
        print(f"{k}: gpu {r[k]!r} ref {ref[k]!r} fp64 route {ref['m64'][k]!r} tol {tol:.3e}")
        assert same(r[k], ref[k]) or abs(r[k] - ref[k]) <= tol, k
    return r


def check_lane(kind, cols, row, ref, err_px, nll_px, stats):
    check_planes(kind, ref, err_px, nll_px, stats)
    return check_row(kind, cols, row, ref)


def check_case(name, out, stats=None):
    c, refs, grids = get_case(name)
    from macvo_amd import _lib as L

    cols = L.EVAL_FLOW_COLS if c["kind"] == "flow" else L.EVAL_DEPTH_COLS
    stats = {} if stats is None else stats
    for l, ref in enumerate(refs):
        check_lane(c["kind"], cols, out["row"][l], ref, out["err"][l], None if out["nll"] is None else out["nll"][l], stats)
    if grids is not None:
        assert np.array_equal(out["grids"], grids)
    return stats


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", list(CASES))
def test_eval_matches_reference(gpu, name):
    c, _, _ = get_case(name)
    out = run_case(c, gpu)
    check_case(name, out)
    if "empty_mask" in name:
        from macvo_amd import _lib as L

        r = dict(zip(L.EVAL_FLOW_COLS if c["kind"] == "flow" else L.EVAL_DEPTH_COLS, out["row"][0]))
        assert r["n_mask"] == 0 and math.isnan(r["masked_epe" if c["kind"] == "flow" else "masked_err"])        # count 0, NaN row


@pytest.mark.parametrize("name", ["flow_37x53", "depth_37x53"])
def test_grids_accumulate_and_rows_in_the_middle_of_a_table(gpu, name):
    c, refs, grids = get_case(name)
    from macvo_amd import _lib as L

    ncols = len(L.EVAL_FLOW_COLS if c["kind"] == "flow" else L.EVAL_DEPTH_COLS)
    rows = torch.full((1, 5, ncols), 7.25, dtype=torch.float32, device=gpu)
    first = run_case(c, gpu, rows=rows, row=2)
    second = run_case(c, gpu, rows=rows, row=3, grids=first["res"].grids)
    assert np.array_equal(second["grids"], 2 * grids)
    host = rows.cpu()
    assert bool((host[:, [0, 1, 4]] == 7.25).all())                       # the other rows stay as they were
    assert torch.equal(host[:, 2].view(torch.int32), host[:, 3].view(torch.int32))
    first["grids"] = grids                                                # (checked above as the accumulated pair)
    first["row"] = host[:, 2].numpy()
    check_case(name, first)


@pytest.mark.parametrize("name", ["flow_37x53", "depth_37x53"])
def test_non_default_stream(gpu, name):
    c, _, _ = get_case(name)
    s = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out = run_case(c, gpu)
    check_case(name, out)


@pytest.mark.parametrize("name", ["flow_3lanes", "depth_3lanes", "flow_480x640_2lanes", "depth_480x640_2lanes"])
def test_lanes_equal_solo_runs_and_repeat_bitwise(gpu, name):
    c, _, _ = get_case(name)
    both = run_case(c, gpu)
    again = run_case(c, gpu)
    assert np.array_equal(both["row"].view(np.int32), again["row"].view(np.int32))          # the same call twice: the same bits
    assert np.array_equal(both["grids"], again["grids"])
    for l in range(c["est"].shape[0]):
        solo = run_case({k: (v[l:l + 1] if isinstance(v, torch.Tensor) else v) for k, v in c.items()}, gpu)
        assert np.array_equal(solo["row"][0].view(np.int32), both["row"][l].view(np.int32)), l
        assert np.array_equal(solo["grids"][0], both["grids"][l])
        assert torch.equal(solo["nll"][0].view(torch.int32), both["nll"][l].view(torch.int32))


def test_argument_checks(gpu):
    from macvo_amd import _lib as L
    from macvo_amd import ops

    z = torch.zeros(1, 2, 4, 4, device=gpu)
    with pytest.raises(L.MacvoHipError):
        ops.eval_flow(z, torch.zeros(1, 2, 4, 5, device=gpu))
    with pytest.raises(L.MacvoHipError):
        ops.eval_flow(z.cpu(), z.cpu())
    with pytest.raises(L.MacvoHipError):
        ops.eval_flow(z, z, rows=torch.zeros(1, 2, 19, device=gpu), row=2)
    with pytest.raises(L.MacvoHipError):
        ops.eval_depth(torch.zeros(2049, 2048, device=gpu), torch.zeros(2049, 2048, device=gpu))    # H * W > 2^22
    assert isinstance(ops.eval_flow(z, z).row, torch.Tensor)                                        # views, never a Python float


# ------------------------------------------------------------------------------------------------ fixture and public functions
def _tartan():
    z = np.load(os.path.join(ROOT, "tests", "golden", "tartanair_p000.npz"))
    depth = torch.from_numpy(z["depth"]).float()                                                    # [4, 320, 448]
    flow = (torch.from_numpy(z["flow_u16"].astype(np.float32)) - 32768.0) / 64.0                    # [3, 2, 320, 448]
    valid = torch.from_numpy(z["flow_mask"]) == 0                                                   # the fixture's mask: 0 = valid
    yy, xx = torch.meshgrid(torch.arange(320.0), torch.arange(448.0), indexing="ij")
    tex = torch.sin(xx * 0.37 + yy * 0.11) * torch.cos(yy * 0.23 - xx * 0.05)                       # deterministic texture error
    est_flow = flow + torch.stack([tex * 1.5, tex.flip(0) * 0.7])[None] * torch.tensor([1.0, 2.0, 0.5])[:, None, None, None]
    flow_cov = torch.stack([0.2 + (tex * 1.5) ** 2 * (1.5 + torch.cos(xx * 0.02)), 0.1 + (tex.flip(0) * 0.7) ** 2 * (0.5 + torch.sin(yy * 0.03) ** 2)])
    est_depth = depth * (1 + 0.05 * tex)[None]
    depth_cov = (0.05 * depth * tex[None]) ** 2 * (1.2 + torch.sin(xx * 0.01))[None] + 1e-3
    return dict(depth=depth, flow=flow, valid=valid, est_flow=est_flow, flow_cov=flow_cov[None].expand(3, -1, -1, -1).contiguous(),
                est_depth=est_depth, depth_cov=depth_cov)


def test_frontend_evaluator_on_the_tartanair_fixture(gpu):
    from macvo_amd import _lib as L
    from macvo_amd.evaluation import DepthPerformance, FrontendEvaluator

    t = _tartan()
    ev = FrontendEvaluator(320, 448, 1, gpu, capacity=2)                      # capacity 2: the flow table grows once, on the device
    fgrids, dgrid = np.zeros((2, 100, 100), np.uint32), np.zeros((100, 100), np.uint32)
    frefs, drefs = [], []
    for i in range(3):
        assert ev.push_flow(t["est_flow"][i].to(gpu), t["flow"][i].to(gpu), t["flow_cov"][i].to(gpu), t["valid"][i].to(gpu), 128.0, False) == i
        fr = ER.flow_frame(t["est_flow"][i], t["flow"][i], t["flow_cov"][i], t["valid"][i], 128.0, False, fgrids)
        fr["m64"] = ER.nll_means64("flow", t["est_flow"][i], t["flow"][i], t["flow_cov"][i], fr)
        frefs.append(fr)
    for i in range(4):
        ev.push_depth(t["est_depth"][i].to(gpu), t["depth"][i].to(gpu), t["depth_cov"][i].to(gpu), 80.0)
        fr = ER.depth_frame(t["est_depth"][i], t["depth"][i], t["depth_cov"][i], 80.0, dgrid)
        fr["m64"] = ER.nll_means64("depth", t["est_depth"][i], t["depth"][i], t["depth_cov"][i], fr)
        drefs.append(fr)
    res = ev.result()
    assert res.flow.shape == (1, 3, len(L.EVAL_FLOW_COLS)) and res.depth.shape == (1, 4, len(L.EVAL_DEPTH_COLS))
    assert np.array_equal(res.flow_grids[0], fgrids) and np.array_equal(res.depth_grid[0], dgrid) and fgrids.sum() > 1e5
    for kind, cols, got, refs in (("flow", L.EVAL_FLOW_COLS, res.flow[0], frefs), ("depth", L.EVAL_DEPTH_COLS, res.depth[0], drefs)):
        for row, ref in zip(got, refs):
            check_row(kind, cols, row, ref)
    # the sequence reducers on the read-back rows
    recs = res.depth_records()
    med = DepthPerformance.median([DepthPerformance(*(r[k] for k in ("masked_err", "err_25", "err_50", "err_75"))) for r in recs])
    assert med.err_50 == ER.seq_median([f["err_50"] for f in drefs]) and med.err_25 == ER.seq_median([f["err_25"] for f in drefs])


class _Matcher:
    provide_cov = True

    def __init__(self, o, dev):
        self.o, self.dev = o, dev

    def estimate(self, a, b):
        from macvo_amd.interfaces import IMatcher

        t = a.idx
        return IMatcher.Output(flow=self.o["est_flow"][t:t + 1].to(self.dev), cov=self.o["flow_cov"][t:t + 1].to(self.dev),
                               mask=self.o["match_mask"][t:t + 1].to(self.dev))


class _Depth:
    provide_cov = True

    def __init__(self, o, dev):
        self.o, self.dev = o, dev

    def estimate(self, a):
        from macvo_amd.interfaces import IStereoDepth

        t = a.idx
        return IStereoDepth.Output(depth=self.o["est_depth"][t:t + 1].to(self.dev), cov=self.o["depth_cov"][t:t + 1].to(self.dev))


def test_public_functions_against_the_reference_records(gpu):
    """evaluate_flow / evaluate_flowcov / evaluate_depth / evaluate_depthcov with fake modules on the golden's inputs, against eval_ref's sequence
    values under the per-frame tolerances above, and against the records the reference's own functions returned (tests/golden/eval.npz).  The
    reference reduces each frame with torch's fp32 nanmean, so its mean fields may sit 16 * 2^-24 * mean|term| (fp32 pairwise summation of
    <= 2^11 terms plus the division) from the exact mean of the same terms; that is added for the comparison with the records, nothing else is."""
    from types import SimpleNamespace

    from macvo_amd import evaluation as E
    from tests.test_eval_host import golden_flow_frames

    g = np.load(os.path.join(ROOT, "tests", "golden", "eval.npz"))
    o = {k: torch.from_numpy(g[k]) for k in ("gt_flow", "est_flow", "flow_cov", "match_mask", "flow_mask", "gt_depth", "est_depth", "depth_cov")}
    _, _, T, max_flow, max_depth = g["meta"]
    T = int(T)

    def frames():
        return [SimpleNamespace(frame_idx=t, stereo=SimpleNamespace(idx=t, gt_flow=o["gt_flow"][t:t + 1], flow_mask=o["flow_mask"][t:t + 1],
                                                                   gt_depth=o["gt_depth"][t:t + 1])) for t in range(T)]

    def close(what, got, ref64, tol, record, mean_abs):
        print(f"{what}: gpu {got!r} eval_ref {ref64!r} (tol {tol:.3e}) reference record {record!r}")
        assert same(got, ref64) or abs(got - ref64) <= tol, what
        assert same(got, record) or abs(got - record) <= tol + 16 * 2.0 ** -24 * mean_abs, what

    def ulp(x):
        return float(np.spacing(np.float32(abs(x))))

    def nll_checks(perf, refs, record, what):
        for i, k in enumerate(NLL):
            tols = [nll_mean_tolerance(f, k) for f in refs]
            close(f"{what}.{k}", getattr(perf, k), ER.seq_mean([f[k] for f in refs]), max(t for t, _ in tols) + ulp(record[i]), record[i],
                  max(m for _, m in tols))

    mask_before = o["flow_mask"].clone()
    for tag, gtm in (("", False), ("_gtmask", True)):
        p = E.evaluate_flow(_Matcher(o, gpu), frames(), float(max_flow), None, gtm)
        refs = golden_flow_frames(g, o, gtm, False)
        for i, k in enumerate(("masked_epe", "epe")):
            close("flow." + k, getattr(p, k), ER.seq_mean([f[k] for f in refs]), ulp(g["flow" + tag][i]), g["flow" + tag][i], g["flow" + tag][i])
        assert (p.px1, p.px3, p.px5) == tuple(g["flow" + tag][2:5])
        pc, grids = E.evaluate_flowcov(_Matcher(o, gpu), frames(), float(max_flow), gtm)
        assert np.array_equal(grids, g["flowcov_grids" + tag]) and grids.dtype == np.uint32
        refs = golden_flow_frames(g, o, gtm, True)
        for f, t in zip(refs, range(T - 1)):
            f["m64"] = ER.nll_means64("flow", o["est_flow"][t], o["gt_flow"][t], o["flow_cov"][t, :2], f)
        nll_checks(pc, refs, g["flowcov" + tag], "flowcov" + tag)
    assert torch.equal(o["flow_mask"], mask_before)                       # the frame's own mask is not modified
    refs = [ER.depth_frame(o["est_depth"][t, 0], o["gt_depth"][t, 0], o["depth_cov"][t, 0], float(max_depth)) for t in range(T)]
    for f, t in zip(refs, range(T)):
        f["m64"] = ER.nll_means64("depth", o["est_depth"][t, 0], o["gt_depth"][t, 0], o["depth_cov"][t, 0], f)
    d = E.evaluate_depth(_Depth(o, gpu), frames(), float(max_depth))
    close("depth.masked_err", d.masked_err, ER.seq_median([f["masked_err"] for f in refs]), ulp(g["depth"][0]), g["depth"][0], g["depth"][0])
    assert (d.err_25, d.err_50, d.err_75) == tuple(g["depth"][1:4])
    dc, grid = E.evaluate_depthcov(_Depth(o, gpu), frames(), float(max_depth))
    assert np.array_equal(grid, g["depthcov_grid"])
    nll_checks(dc, refs, g["depthcov"], "depthcov")
    # huge_epe_warn reads the rows after the sequence
    with pytest.warns(UserWarning, match="huge masked epe"):
        E.evaluate_flow(_Matcher(o, gpu), frames(), float(max_flow), huge_epe_warn=0.0)
