"""GPU: the image-gradient selectors (mv_kp_gradient_lanes, mv_kp_finish_device_lanes, the HIP_ plugins, pipeline.image_selector).

* Exact against torch on 1/256-valued images (both sides are exact there), behind the guard of tests/test_grad_selectors_host.py on the inputs.
* General floats (k/255): the kernels equal their host twin bit for bit; against the torch restatement every differing pixel lies, in an fp64
  evaluation, within 2e-5 of the threshold or has a window neighbour within 2e-5 of it.  2e-5 is derived: a gradient is 14 fp32 additions on partial sums
  below 16, each off by at most half an ulp = 2^-21 — 14 * 2^-21 = 6.7e-6 per side, two sides and the threshold's own ulp stay below 2e-5.
* The seeded device draw against torch.Generator().manual_seed(seed) per lane; the plugins against the restatement and the reference's golden rows;
  the frame driver fed device rows + device counts against the same pipe fed host rows + list counts."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import grad_selectors_ref as GR
from tests import kp_grad_twin as TW
from tests import selectors_ref as SR
from tests import synth

pytestmark = pytest.mark.gpu

SHAPES = ((96, 128), (61, 83), (33, 200))       # 61 x 83: odd, narrower than two candidate words; 33 x 200: ragged in both directions, four words
GUARD = 1e-5
BAND = 2e-5
LANE_SEEDS = (3, 5, 7)                           # image seeds of the lanes: chosen so that the guards below hold on every shape
_cache: dict = {}


def _image(H, W, seed, denom=256):
    key = ("img", H, W, seed, denom)
    if key not in _cache:
        _cache[key] = GR.quantised_image(H, W, seed, denom)
    return _cache[key]


def _ref(H, W, seed, gs, nms, m=8, denom=256):
    """The restatement's candidate list (int32 numpy), computed once per case."""
    key = ("ref", H, W, seed, gs, nms, m, denom)
    if key not in _cache:
        _cache[key] = GR.candidates(_image(H, W, seed, denom), m, gs, nms).numpy().astype(np.int32)
    return _cache[key]


def _run(images, m, gs, nms):
    """ops.kp_gradient -> per lane (cand int32 numpy, count list, stats int32-bit numpy)."""
    from macvo_amd import ops

    c = ops.kp_gradient(images, m, gs, nms)
    torch.cuda.synchronize()
    cand, count, stats = c.cand.cpu().reshape(c.lanes, -1), c.count.cpu().reshape(c.lanes, 4), c.stats.cpu().reshape(c.lanes, 4)
    return [(cand[l, : int(count[l, 0])].numpy().copy(), count[l].tolist(), stats[l].numpy().view(np.int32).copy()) for l in range(c.lanes)]


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_exact_against_torch_on_quantised_images(gpu, H, W, lanes):
    seeds = LANE_SEEDS[:lanes]
    imgs = [_image(H, W, s) for s in seeds]
    dev = torch.stack(imgs).to(gpu)
    for gs in (1.0, 2.0, 3.0):
        for s, img in zip(seeds, imgs):
            assert GR.guard_distance(img, gs) > GUARD, (H, W, s, gs)          # the guard on the inputs
        plain = None
        for nms in (None, 1, 3, 7, 15):
            got = _run(dev if lanes > 1 else dev[0], 8, gs, nms)
            for l, s in enumerate(seeds):
                cand, count, stats = got[l]
                want = _ref(H, W, s, gs, nms)
                assert np.array_equal(cand, want), (H, W, s, gs, nms)
                assert count == [want.size, _ref(H, W, s, gs, None).size, 0, 0]
                assert abs(float(stats.view(np.float32)[2]) - GR.threshold_f64(img if lanes == 1 else imgs[l], gs)[1]) <= 4.8e-7
                if lanes > 1:   # a lane batched = the lane alone, bit for bit (candidates, counts, statistics)
                    alone = _run(dev[l], 8, gs, nms)[0]
                    assert np.array_equal(alone[0], cand) and alone[1] == count and np.array_equal(alone[2], stats)
            if nms is None:
                plain = got
            elif nms == 1:      # a 1 x 1 window is the plain selector
                assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) for a, b in zip(got, plain))


@pytest.mark.parametrize("H,W", SHAPES)
def test_edge_images_select_what_torch_selects(gpu, H, W):
    from macvo_amd import ops

    img = _image(H, W, 3)
    for m in (0, (min(H, W) + 1) // 2, max(H, W)):          # the empty slice 0:-0; 2m >= H or W: zero rows, no error
        for nms in (None, 3):
            assert GR.candidates(img, m, 1.0, nms).numel() == 0
            cand, count, _ = _run(img.to(gpu), m, 1.0, nms)[0]
            assert cand.size == 0 and count == [0, 0, 0, 0]
    nan = img.clone()
    nan[2, H // 3, W // 3] = float("nan")
    blk = GR.block_constant_image(H, W, 9)
    assert GR.guard_distance(blk, 1.0) > GUARD
    batch = torch.stack([torch.zeros(3, H, W), nan, blk]).to(gpu)
    for nms in (None, 7):
        zero_l, nan_l, blk_l = _run(batch, 4, 1.0, nms)
        assert zero_l[0].size == 0 and zero_l[1] == [0, 0, 0, 0] and not zero_l[2].any()                 # thr = 0, strict '>': nothing
        assert nan_l[0].size == 0 and nan_l[1] == [0, 0, 0, 0] and np.isnan(nan_l[2].view(np.float32)[:3]).all()
        want = GR.candidates(blk, 4, 1.0, nms).numpy().astype(np.int32)
        assert np.array_equal(blk_l[0], want) and want.size > 0
        if nms:
            g = GR.image_grad(blk)[0].flatten()[torch.from_numpy(want).long()]
            assert g.unique().numel() < want.size, "tied maxima exist and every one is kept"
    # n = 0: the device finish selects nothing and the generator does not move
    c = ops.kp_gradient(batch[:1], 4, 1.0, None)
    state = ops.mt19937_state([77], gpu)
    before = state.clone()
    rows, n_sel = c.finish_device(50, state)
    assert n_sel.tolist() == [0] and not rows.any() and torch.equal(state, before)


def _near_tie(g64: torch.Tensor, k: int) -> torch.Tensor:
    """[H, W] fp64: distance of every pixel's value to the nearest OTHER value in its k x k window (+inf outside the image)."""
    H, W = g64.shape
    cols = F.unfold(F.pad(g64[None, None], (k // 2,) * 4, value=float("inf")), k)[0]        # [k * k, H * W]
    d = (cols - g64.reshape(1, -1)).abs()
    d[k * k // 2] = float("inf")
    return d.min(dim=0).values.reshape(H, W)


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_general_floats_equal_the_twin_and_differ_from_torch_only_in_the_band(gpu, H, W, lanes):
    seeds = LANE_SEEDS[:lanes]
    imgs = [_image(H, W, s, 255) for s in seeds]
    dev = torch.stack(imgs).to(gpu)
    for gs, nms in ((1.0, None), (2.0, 3), (1.0, 7), (3.0, 15), (2.0, 1)):
        got = _run(dev if lanes > 1 else dev[0], 8, gs, nms)
        for l, s in enumerate(seeds):
            cand, count, stats = got[l]
            tw = TW.select(imgs[l], 8, gs, nms)
            assert np.array_equal(cand, tw.cand) and count == [tw.cand.size, tw.n_above, 0, 0], (H, W, s, gs, nms)
            assert np.array_equal(stats[:3], tw.stats.view(np.int32)), "mean, std and threshold: the twin's bits"
            want = _ref(H, W, s, gs, nms, denom=255)
            g64, thr64 = GR.threshold_f64(imgs[l], gs)
            band = (g64 - thr64).abs() <= BAND
            if nms and nms > 1:
                band |= _near_tie(g64, nms) <= BAND
            band = band.flatten().numpy()
            diff = np.setxor1d(cand, want)
            print(f"{H}x{W} seed {s} grad_std {gs} nms {nms}: {want.size} candidates, {diff.size} differ, {int(band[want].sum())} of torch's in the band")
            assert band[diff].all(), (H, W, s, gs, nms, diff[~band[diff]])
            assert band[want].sum() < 0.01 * want.size, "the restatement's own in-band population is below 1 % of its candidates on these inputs"


def test_seeded_device_draw_is_torch_randperm_per_lane(gpu):
    """Three successive calls on three lanes: n >= numPoint, n < numPoint, n = 0 and numPoint = mv_randperm_max_head()."""
    from macvo_amd import _lib as L
    from macvo_amd import ops

    H, W = 96, 128
    head = L.load().mv_randperm_max_head()
    a, b, zero = _image(H, W, 3), _image(H, W, 5), torch.zeros(3, H, W)
    calls = (((a, b, zero), 8, 1.0, None, head), ((b, zero, a), 8, 2.0, 7, 200), ((zero, a, b), 8, 1.0, 3, 64))
    seeds = (5, 1234, 99)
    gens = [torch.Generator().manual_seed(s) for s in seeds]
    state = ops.mt19937_state(seeds, gpu)
    seen = set()
    for images, m, gs, nms, k in calls:
        rows, n_sel = ops.kp_gradient(torch.stack(images).to(gpu), m, gs, nms).finish_device(k, state)
        rows, n_sel = rows.cpu(), n_sel.cpu().tolist()
        assert rows.shape == (3, k, 2) and rows.dtype == torch.int64
        for l in range(3):
            want = GR.select(images[l], k, m, gs, nms, generator=gens[l])
            assert n_sel[l] == want.shape[0] and torch.equal(rows[l, : n_sel[l]], want), (l, k, nms)
            assert not rows[l, n_sel[l]:].any(), "rows at or past n_sel are zero"
            seen.add("zero" if n_sel[l] == 0 else ("short" if n_sel[l] < k else "full"))
    assert seen == {"zero", "short", "full"}
    with pytest.raises(ValueError):
        ops.kp_gradient(a.to(gpu), 8, 1.0).finish_device(head + 1, state[:1].clone())


def _frame(img, dev=None):
    return NS(imageL=(img if dev is None else img.to(dev)).unsqueeze(0), height=img.shape[1], width=img.shape[2])


def test_plugins_reproduce_the_restatement_and_the_golden_rows(gpu):
    import os

    import macvo_amd.plugins as P

    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grad_selectors.npz"))
    for ci, (H, W, iseed, m, gs, nms, n, seed) in enumerate(GR.GOLDEN_CASES):
        img = torch.from_numpy(golden[f"image_{H}x{W}_{iseed}"].astype(np.float32)) / 256.0
        sel = P.HIP_GradientSelector(NS(mask_width=m, grad_std=gs)) if nms is None else P.HIP_SparseGradienSelector(NS(mask_width=m, grad_std=gs, nms_size=nms))
        for frame in (_frame(img), _frame(img, gpu)):        # a CPU image is moved to the GPU
            torch.manual_seed(seed)
            rows = sel.select_point(frame, n, None, None, None)
            assert rows.is_cuda and rows.dtype == torch.int64 and torch.equal(rows.cpu(), torch.from_numpy(golden[f"rows_{ci}"])), ci
        torch.manual_seed(seed)
        assert torch.equal(rows.cpu(), GR.select(img, n, m, gs, nms))
    # a seeded plugin: successive calls of one device-resident generator
    img = _image(96, 128, 3)
    sel = P.HIP_SparseGradienSelector(NS(mask_width=8, grad_std=1.0, nms_size=5, seed=31))
    g = torch.Generator().manual_seed(31)
    for n in (40, 500, 0, 40):
        assert torch.equal(sel.select_point(_frame(img, gpu), n, None, None, None).cpu(), GR.select(img, n, 8, 1.0, 5, generator=g))
    # SelectorCompose of the reference's golden case, and of a grid + a sparse-gradient + a seeded random selector
    c = GR.GOLDEN_COMPOSE
    img = _image(c["H"], c["W"], c["image_seed"])
    comp = P.HIP_SelectorCompose(NS(selector_args=[NS(type="HIP_GradientSelector", args=NS(mask_width=c["mask_width"], grad_std=c["grad_std"])),
                                                   NS(type="HIP_SparseGradienSelector", args=NS(mask_width=c["mask_width"], grad_std=c["grad_std"],
                                                                                                 nms_size=c["nms_size"]))], weight=list(c["weight"])))
    torch.manual_seed(c["seed"])
    assert torch.equal(comp.select_point(_frame(img, gpu), c["num_point"], None, None, None).cpu(), torch.from_numpy(golden["compose_rows"]))
    H, W = c["H"], c["W"]
    comp = P.HIP_SelectorCompose(NS(selector_args=[NS(type="HIP_GridSelector", args=NS(mask_width=8, device="cuda")),
                                                   NS(type="HIP_SparseGradienSelector", args=NS(mask_width=8, grad_std=2.0, nms_size=3)),
                                                   NS(type="HIP_RandomSelector", args=NS(mask_width=8, device="cuda", seed=17))], weight=[1, 1, 1]))
    g = torch.Generator().manual_seed(17)
    for call in range(2):
        torch.manual_seed(40 + call)
        rows = comp.select_point(_frame(img, gpu), 200, None, None, None)
        torch.manual_seed(40 + call)
        want = GR.compose([lambda k: SR.grid_select(k, H, W, 8), lambda k: GR.select(img, k, 8, 2.0, 3), lambda k: SR.random_select(k, H, W, 8, g)],
                          [1, 1, 1], 200)
        assert rows.is_cuda and torch.equal(rows.cpu(), want) and GR.compose_split([1, 1, 1], 200) == [66, 66, 66]


def test_image_selector_rows_and_counts(gpu):
    from macvo_amd.pipeline import image_selector

    H, W, k = 61, 83, 149                           # between the two images' candidate counts: one lane short, one full, one empty
    imgs = [_image(H, W, 3), torch.zeros(3, H, W), _image(H, W, 5)]
    block = {"type": "SparseGradienSelector", "args": {"mask_width": 4, "grad_std": 2.0, "nms_size": 3}}
    batch = torch.stack(imgs).to(gpu)
    seeded, gens = image_selector(block, gpu, seeds=[1, 2, 3]), [torch.Generator().manual_seed(s) for s in (1, 2, 3)]
    unseeded = image_selector(NS(type="HIP_SparseGradienSelector", args=NS(**block["args"])), gpu)
    for call in range(2):
        rows, counts = seeded(batch, k)
        torch.manual_seed(9 + call)
        rows_u, counts_u = unseeded(batch, k)
        torch.manual_seed(9 + call)
        for r, c, gen in ((rows, counts, gens), (rows_u, counts_u, [None] * 3)):
            assert r.is_cuda and c.is_cuda and r.shape == (3, k, 2) and r.dtype == torch.int64 and c.dtype == torch.int32 and c.shape == (3,)
            for l in range(3):
                want = GR.select(imgs[l], k, 4, 2.0, 3, generator=gen[l])
                n = int(c[l])
                assert n == want.shape[0] and torch.equal(r[l, :n].cpu(), want) and not r[l, n:].any()
        assert counts.tolist() == [148, 0, 149]


TABLES = (("KP0", torch.int64, (2,)), ("KP0F", torch.float32, (2,)), ("KP1", torch.float32, (2,)), ("POS_TW", torch.float32, (3,)),
          ("COV0", torch.float64, (3, 3)), ("COV1", torch.float64, (3, 3)), ("VALID", torch.uint8, ()))


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype in (torch.float32, torch.float64) else t


def test_driver_takes_device_rows_and_device_counts(gpu):
    """A NativeHotPath(selector="explicit") over four synthetic frames, fed device rows + device counts from image_selector: poses and stored keypoints
    are the bits of the same pipe fed the same rows as host tensors with list counts.  One frame selects nothing (an all-zero image)."""
    from macvo_amd.pipeline import Camera, FrameInputs, HotPathConfig, NativeHotPath, image_selector

    n_frames, H, W, k = 5, 192, 256, 200
    cam, frames, _ = synth.make_sequence(n_frames, H, W, C=64, iters=2, seed=31)
    ins = [FrameInputs(**{kk: (None if v is None else v.to(gpu)) for kk, v in fr.items()}) for fr in frames]
    images = [torch.zeros(3, H, W) if t == 3 else _image(H, W, 20 + t) for t in range(n_frames)]
    select = image_selector({"type": "SparseGradienSelector", "args": {"mask_width": 32, "grad_std": 1.0, "nms_size": 7}}, gpu, seeds=[123])
    fed = [None] + [select(images[t][None].to(gpu), k) for t in range(1, n_frames)]
    torch.cuda.synchronize()
    assert [int(c[0]) for _, c in fed[1:]].count(0) == 1 and max(int(c[0]) for _, c in fed[1:]) > 50

    def run(device_counts: bool):
        hot = NativeHotPath(Camera(**cam), HotPathConfig(selector="explicit", num_point=k, graph_type="icp"), gpu)
        hot.initialize(ins[0])
        out = []
        for t in range(1, n_frames):
            rows, counts = fed[t]
            x = ins[t]
            if device_counts:
                x.keypoints, x.keypoint_counts = rows, counts
            else:
                x.keypoints, x.keypoint_counts = rows.cpu(), [int(counts[0])]
            res = hot.step(x)
            if device_counts:
                assert res._n_sel is None, "the count did not reach the host on the way in"
            torch.cuda.synchronize()
            x.keypoints = x.keypoint_counts = None
            d = {name: res._rows(name, dt, tail).clone() for name, dt, tail in TABLES}
            d["pose"], d["n_sel"], d["n_cand"] = res.pose.clone(), res.n_sel, res.n_cand
            out.append(d)
        hot.close()
        return out

    want, got = run(False), run(True)
    assert [d["n_sel"] for d in want] == [int(c[0]) for _, c in fed[1:]] == [d["n_sel"] for d in got]
    for t, (a, b) in enumerate(zip(want, got)):
        assert a["n_cand"] == b["n_cand"] == a["n_sel"]
        for name in a:
            if isinstance(a[name], torch.Tensor):
                assert a[name].shape == b[name].shape and torch.equal(_bits(a[name]), _bits(b[name])), (t, name)
        assert torch.equal(a["KP0"].cpu(), fed[t + 1][0][0, : a["n_sel"]].cpu())
