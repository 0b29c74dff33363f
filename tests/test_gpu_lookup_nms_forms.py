"""GPU parity of the window lookup's kernel forms (one barrier, wave-private output strips, the bank-conflict-free tap order) and of the NMS
launch (ballot offsets, early record reservation): every form against the CPU oracle and against its sibling forms, bit for bit where the
forms share their arithmetic."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ lookup
LB, LH1, LW1, LH2, LW2 = 2, 5, 7, 12, 20          # 35 queries: a ragged last workgroup for 16- and 32-query workgroups


def _lookup_coords():
    """[B, 2, H1, W1]: ordinary fractions everywhere, then one query each for the cases the kernel treats apart."""
    g = torch.Generator().manual_seed(21)
    co = torch.empty(LB, 2, LH1, LW1)
    co[:, 0] = torch.rand(LB, LH1, LW1, generator=g) * (LW2 - 1)
    co[:, 1] = torch.rand(LB, LH1, LW1, generator=g) * (LH2 - 1)
    special = [
        (6.0, 5.0), (0.0, 0.0), (19.0, 11.0),                       # exact integers (inside, first and last cell)
        (6.004, 5.003), (6.996, 5.997), (6.004, 5.997),             # fractions below 0.01 / above 0.99: the margin rows and columns
        (3.0 + 1.2e-7, 4.0 - 1.2e-7), (7.0 - 1e-4, 2.0 + 1e-4),     # next to an integer: the fp32 round trip may cross it
        (-2.3, 5.5), (21.6, 5.5), (9.5, -1.7), (9.5, 13.2),         # windows hanging over the left, right, top and bottom edges
        (-1.5, -2.5), (20.5, -0.5), (-3.2, 12.4), (21.1, 13.9),     # ... and over the four corners
        (-30.0, 4.0), (5.0, 42.0),                                  # 30 cells outside: every tap is zero
        (1.0e7, 3.0), (3.0, -1.0e7),                                # far outside (the origin clamp)
        (float("nan"), 3.0), (4.0, float("nan")),                   # NaN
    ]
    flat = co.view(LB, 2, LH1 * LW1)
    for i, (x, y) in enumerate(special):
        flat[i % LB, 0, 3 + i // LB] = x
        flat[i % LB, 1, 3 + i // LB] = y
    return co


@pytest.fixture(scope="module")
def lookup_case():
    """The volume (fp32 and the same cells rounded to fp16), the coordinates and the oracle's tokens per radius, computed once."""
    from oracle import corr

    g = torch.Generator().manual_seed(20)
    vol16 = (torch.randn(LB * LH1 * LW1, 1, LH2, LW2, generator=g) * 3).half()
    vol = vol16.float()                                                     # the fp16 forms widen exactly these cells
    coords = _lookup_coords()
    ref = {r: corr.corr_lookup(vol, coords, r) for r in (1, 2, 3, 4)}
    return vol, vol16, coords, ref


def _tile(v):
    """Row-major slices [N, 1, H2, W2] (H2, W2 multiples of 4) in the 4 x 4-cell tile order of the tiled lookups."""
    n, _, h, w = v.shape
    return v.view(n, h // 4, 4, w // 4, 4).permute(0, 1, 3, 2, 4).contiguous().view(n, 1, h, w)


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


def _close(a, ref):
    a, ref = torch.nan_to_num(a.cpu(), nan=7.0), torch.nan_to_num(ref, nan=7.0)
    torch.testing.assert_close(a, ref, rtol=1e-5, atol=2e-4)


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_row_major_lookup_matches_the_oracle(gpu, lookup_case, radius):
    from macvo_amd import ops

    vol, _, coords, ref = lookup_case
    _close(ops.corr_lookup(vol.to(gpu), coords.to(gpu), radius), ref[radius])


def test_tiled_and_fp16_cell_lookups_match_the_oracle_and_the_row_major_form(gpu, lookup_case):
    """Radius 4: the tiled fp32 kernel and both fp16-cell forms against the oracle, and — same cells, same arithmetic — bit for bit
    against the row-major fp32 kernel."""
    from macvo_amd import ops

    vol, vol16, coords, ref = lookup_case
    cd = coords.to(gpu)
    base = ops.corr_lookup(vol.to(gpu), cd, 4)
    forms = {
        "tiled fp32": ops.corr_lookup(_tile(vol).to(gpu), cd, 4, tiled=True),
        "row-major fp16": ops.corr_lookup(vol16.to(gpu), cd, 4),
        "tiled fp16": ops.corr_lookup(_tile(vol16).to(gpu), cd, 4, tiled=True),
    }
    for name, tok in forms.items():
        _close(tok, ref[4])
        assert _same(tok, base), name


def test_large_batch_lookup_forms_agree_and_match_the_oracle(gpu):
    """B x N1 = 14 x 4800 > 65536 queries on 8 x 12 slices: the 32-query workgroups of every form (no environment knob involved)."""
    from macvo_amd import ops
    from oracle import corr

    B, H1, W1, H2, W2 = 14, 60, 80, 8, 12
    g = torch.Generator().manual_seed(22)
    vol16 = (torch.randn(B * H1 * W1, 1, H2, W2, generator=g) * 3).half()
    vol = vol16.float()
    coords = torch.empty(B, 2, H1, W1)
    coords[:, 0] = torch.rand(B, H1, W1, generator=g) * (W2 + 6) - 3          # inside and up to 3 cells over every edge
    coords[:, 1] = torch.rand(B, H1, W1, generator=g) * (H2 + 6) - 3
    snap = torch.rand(B, 1, H1, W1, generator=g)
    coords = torch.where(snap < 0.1, coords.round(), coords)                  # exact integers ...
    coords = torch.where((snap >= 0.1) & (snap < 0.2), coords.round() + 0.004, coords)   # ... and the margin fetch
    coords[3, :, 7, 9] = float("nan")
    coords[5, 0, 8, 1] = 1.0e7
    cd, vd = coords.to(gpu), vol.to(gpu)
    base = ops.corr_lookup(vd, cd, 4)
    _close(base, corr.corr_lookup(vol, coords, 4))
    assert _same(ops.corr_lookup(_tile(vol).to(gpu), cd, 4, tiled=True), base)
    assert _same(ops.corr_lookup(vol16.to(gpu), cd, 4), base)
    assert _same(ops.corr_lookup(_tile(vol16).to(gpu), cd, 4, tiled=True), base)


# --------------------------------------------------------------------------------------------------------------------- NMS
NH, NW, NK, NMW = 40, 100, 7, 8          # 2.5 x 1.56 tiles of 16 x 64: ragged in both axes


def _nms_inputs(kind, lanes):
    g = torch.Generator().manual_seed(31)
    flow = torch.randn(lanes, 2, 2, NH, NW, generator=g) * 4
    cov = torch.randn(lanes, 2, 2, NH, NW, generator=g) * 0.5              # log-sigma
    if kind == "plateau":
        cov[:, 1, :, 10:40, 0:80] = -1.0        # constant over tile (1, 0) = rows 16..31, columns 0..63, and into its neighbours
    elif kind == "nan_patch":
        cov[:, 1, 0, 12:20, 30:45] = float("nan")
        cov[-1, 1, 1, 33, 70] = float("nan")
    elif kind == "all_nan":
        cov[:, 1] = float("nan")
    else:
        assert kind == "random"
    return flow, cov


def _select_lanes(lib, L, gpu, lanes, fused, flow, cov):
    """The fused launch, or mv_frontend_epilogue_lanes + mv_kp_select_lanes; returns every output as CPU tensors."""
    from macvo_amd import ops

    mk = lambda c, dt=torch.float32: torch.zeros(lanes, c, NH, NW, dtype=dt, device=gpu)  # noqa: E731
    out = {"disparity": mk(1), "disparity_cov": mk(1), "depth": mk(1), "depth_cov": mk(1), "bad_mask": mk(1, torch.uint8),
           "match_flow": mk(2), "match_cov": mk(3)}
    p = L.mvKpSelectParams(NH, NW, L.MV_KP_NODEPTH, NK, NMW, 0.0, 0.0, 100.0)
    nbytes = lib.mv_kp_select_workspace_bytes(NH, NW) * lanes
    ws = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=gpu)
    cand = torch.zeros(lanes, NH * NW, dtype=torch.int32, device=gpu)
    count = torch.zeros(lanes, 4, dtype=torch.int32, device=gpu)
    stats = torch.zeros(lanes, 4, dtype=torch.float32, device=gpu)
    s = ops._stream()
    o = {k: v.data_ptr() for k, v in out.items()}
    if fused:
        L.check(lib.mv_frontend_epilogue_select_lanes(flow.data_ptr(), cov.data_ptr(), 1, 80.0, 6400.0, o["disparity"], o["disparity_cov"],
                                                      o["depth"], o["depth_cov"], o["bad_mask"], o["match_flow"], o["match_cov"], None, None,
                                                      C.byref(p), ws.data_ptr(), ws.numel() * 8, cand.data_ptr(), count.data_ptr(),
                                                      stats.data_ptr(), lanes, s), "mv_frontend_epilogue_select_lanes")
    else:
        L.check(lib.mv_frontend_epilogue_lanes(flow.data_ptr(), cov.data_ptr(), 1, NH, NW, 80.0, 6400.0, o["disparity"], o["disparity_cov"],
                                               o["depth"], o["depth_cov"], o["bad_mask"], o["match_flow"], o["match_cov"], lanes, s),
                "mv_frontend_epilogue_lanes")
        L.check(lib.mv_kp_select_lanes(o["match_cov"], None, None, None, None, None, None, C.byref(p), ws.data_ptr(), ws.numel() * 8,
                                       cand.data_ptr(), count.data_ptr(), stats.data_ptr(), lanes, s), "mv_kp_select_lanes")
    torch.cuda.synchronize()
    assert int(ws.view(torch.int32).abs().max()) >= 0          # (the workspace stays readable)
    res = {k: v.cpu() for k, v in out.items()}
    res.update(cand=cand.cpu(), count=count.cpu(), stats=stats.cpu())
    return res


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("kind", ["random", "plateau", "nan_patch", "all_nan"])
def test_fused_nms_launch_equals_the_unfused_pair_and_the_oracle(gpu, kind, lanes):
    from macvo_amd import _lib as L
    from oracle import selector

    lib = L.load()
    flow, cov = _nms_inputs(kind, lanes)
    fd, cd = flow.to(gpu), cov.to(gpu)
    fu = _select_lanes(lib, L, gpu, lanes, True, fd, cd)
    un = _select_lanes(lib, L, gpu, lanes, False, fd, cd)
    for name in ("disparity", "disparity_cov", "depth", "depth_cov", "match_flow", "match_cov"):
        assert torch.equal(fu[name].view(torch.int32), un[name].view(torch.int32)), name
    assert torch.equal(fu["bad_mask"], un["bad_mask"])
    assert torch.equal(fu["count"], un["count"])                                            # candidates, records (= NMS pixels), 0, 0
    assert torch.equal(fu["stats"].view(torch.int32), un["stats"].view(torch.int32))
    for ln in range(lanes):
        n = int(fu["count"][ln, 0])
        assert torch.equal(fu["cand"][ln, :n], un["cand"][ln, :n])
        # the oracle on the covariance planes the launch wrote (exp(2 log-sigma): the expf of the device is part of the input here)
        fc = fu["match_cov"][ln:ln + 1]
        q = fc[:, 0] + fc[:, 1] - 2 * fc[:, 2]
        erode = -torch.nn.functional.max_pool2d(-q.unsqueeze(1), kernel_size=NK, stride=1, padding=NK // 2)
        n_nms = int(torch.logical_and(q.unsqueeze(1) == erode, ~q.unsqueeze(1).isnan()).sum())
        assert int(fu["count"][ln, 1]) == n_nms
        if kind == "all_nan":
            assert n_nms == 0 and n == 0 and bool(fu["stats"][ln, 0].isnan())
            continue
        if kind == "plateau":
            assert n_nms >= 1024                                                            # the whole 64 x 16 tile and more
        _, ref_cand, aux = selector.cov_aware_selector_nodepth(fc.clone(), 10, NK, NMW, 100.0)
        assert aux["n_nms"] == n_nms
        assert fu["stats"][ln, 0].item() == aux["median"]
        lin = fu["cand"][ln, :n].long()
        assert torch.equal(torch.stack([lin // NW, lin % NW], dim=1), ref_cand)
