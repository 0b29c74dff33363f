"""GPU: the image-gradient selectors past one compaction pass and one tile-sum chunk (tests/grad_sizes.py names the sizes and what each is the first to
reach), below one tile, on MV_MAX_LANES lanes, with ridges on the tile seams, on scaled / negated / overflowing values and with a device draw over a
candidate list of tens of thousands.

The helpers, the guard (1e-5) and the band (2e-5: 14 fp32 additions on partial sums below 16, which does not depend on the image size) are those of
tests/test_gpu_grad_selectors.py.  Every case first asserts, from its own H and W, the path it is there for."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import grad_selectors_ref as GR
from tests import grad_sizes as GS
from tests import kp_grad_twin as TW
from tests import test_gpu_grad_selectors as B
from tests.test_gpu_grad_selectors import BAND, GUARD, _image, _ref, _run

pytestmark = pytest.mark.gpu

LANE_SEEDS = (3, 5, 7)          # the guard holds for all three at every size of the table (thinnest: 1.29e-5 at 130 x 513, seed 7, grad_std 3.0)
_cache: dict = {}


def _twin(img, key, m, gs, nms):
    """TW.select of a cached image, computed once per case (key names the image)."""
    key = ("twin", key, m, gs, nms)
    if key not in _cache:
        _cache[key] = TW.select(img, m, gs, nms)
    return _cache[key]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("gs", [1.0, 2.0, 3.0])
@pytest.mark.parametrize("H,W", list(GS.LARGE) + list(GS.SMALL))
def test_exact_against_torch_and_the_twin_at_the_path_sizes(gpu, H, W, gs):
    """1/256-valued images: candidates = torch's = the twin's, statistics = the twin's bits; one lane, then three lanes each bit-identical to itself alone."""
    GS.check_path(H, W)
    m = GS.mask_width_for(H, W)
    imgs = [_image(H, W, s) for s in LANE_SEEDS]
    for s, img in zip(LANE_SEEDS, imgs):
        assert GR.guard_distance(img, gs) > GUARD, (H, W, s, gs)              # the guard on the inputs
    thr64 = [GR.threshold_f64(img, gs)[1] for img in imgs]
    dev = torch.stack(imgs).to(gpu)
    for nms in (None, 3, 15):
        alone = [_run(dev[l], m, gs, nms)[0] for l in range(3)]              # (lane 0 alone is the one-lane run)
        batch = _run(dev, m, gs, nms)
        for l, s in enumerate(LANE_SEEDS):
            cand, count, stats = alone[l]
            want, tw = _ref(H, W, s, gs, nms, m), _twin(imgs[l], (H, W, s, 256), m, gs, nms)
            assert np.array_equal(cand, want), (H, W, s, gs, nms)
            assert np.array_equal(cand, tw.cand), (H, W, s, gs, nms)
            assert count == [want.size, _ref(H, W, s, gs, None, m).size, 0, 0] and count[1] == tw.n_above
            assert np.array_equal(stats[:3], tw.stats.view(np.int32)), "mean, std and threshold: the twin's bits"
            assert abs(float(stats.view(np.float32)[2]) - thr64[l]) <= 4.8e-7
            assert _same(batch[l], alone[l]), (H, W, s, gs, nms, "a lane batched = the lane alone, bit for bit")
        if nms is None and max(H, W) > 2 * m + 2:
            assert all(a[0].size > 0 for a in alone)


@pytest.mark.parametrize("H,W", list(GS.TINY))
def test_images_smaller_than_any_border(gpu, H, W):
    """3 x 3, 2 x 2, 1 x 1: one ragged tile, no candidates under mask_width 8; the statistics are the twin's (1 x 1: n - 1 = 0, NaN std and thr as torch's)."""
    GS.check_path(H, W)
    imgs = [_image(H, W, s) for s in LANE_SEEDS]
    dev = torch.stack(imgs).to(gpu)
    for m in (8, 1):                # 8: no pixel inside the border; 1: the centre of 3 x 3 is, and is selected or not as torch says
        for nms in (None, 3, 15):
            batch = _run(dev, m, 1.0, nms)
            for l, img in enumerate(imgs):
                cand, count, stats = got = _run(dev[l], m, 1.0, nms)[0]
                assert _same(batch[l], got)
                tw = TW.select(img, m, 1.0, nms)
                f = stats.view(np.float32)
                if H * W == 1:
                    thr = GR.threshold(GR.image_grad(img), 1.0)
                    assert torch.isnan(thr).all() and np.isnan(tw.stats[1:]).all() and np.isnan(f[1:3]).all()
                    assert stats[0] == tw.stats.view(np.int32)[0] and np.isfinite(f[0]) and f[0] == float(GR.image_grad(img).mean())
                else:
                    assert GR.guard_distance(img, 1.0) > GUARD
                    assert np.array_equal(stats[:3], tw.stats.view(np.int32))
                want = GR.candidates(img, m, 1.0, nms).numpy().astype(np.int32)
                assert np.array_equal(cand, want) and np.array_equal(cand, tw.cand) and count[0] == want.size and count[1] == tw.n_above and count[2:] == [0, 0]
                if m == 8 or H < 3:
                    assert count == [0, 0, 0, 0]


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("H,W", [(130, 513), (3841, 65)])
def test_general_floats_at_the_path_sizes(gpu, H, W, lanes):
    """k/255 images: the kernels equal the twin bit for bit; a candidate that differs from torch lies in the band (tests/test_gpu_grad_selectors.py).

    Measured on an MI355X, seeds 3 / 5 / 7 (torch's candidates; of them in the band; candidates on which the kernels and torch differ):
      130 x 513   (1.0, None)  5359 /  5339 /  5429;  0 / 0 / 0;  0 / 0 / 0        (2.0, 3)  2174 / 2146 / 2219;  0 / 1 / 1;  0 / 1 / 0
                  (1.0, 7)     1137 /  1150 /  1137;  2 / 5 / 4;  1 / 1 / 1        (3.0, 15)  259 /  255 /  239;  0 / 0 / 0;  0 / 0 / 0
      3841 x 65   (1.0, None) 17386 / 17311 / 17363;  0 / 0 / 0;  0 / 0 / 0        (2.0, 3)  7045 / 7083 / 7108;  5 / 6 / 4;  4 / 2 / 2
                  (1.0, 7)     3677 /  3730 /  3704;  5 / 11 / 4; 2 / 11 / 2
    The largest in-band share is 0.43 % (5 of 1150) against the bar of 1 %."""
    p = GS.check_path(H, W)
    assert p.per >= 2
    seeds = LANE_SEEDS[:lanes]
    imgs = [_image(H, W, s, 255) for s in seeds]
    dev = torch.stack(imgs).to(gpu)
    cases = ((1.0, None), (2.0, 3), (1.0, 7)) + (((3.0, 15),) if (H, W) == (130, 513) else ())      # (15 x 15 windows over 250K pixels: half a GB of unfold)
    for gs, nms in cases:
        got = _run(dev if lanes > 1 else dev[0], 8, gs, nms)
        for l, s in enumerate(seeds):
            cand, count, stats = got[l]
            tw = _twin(imgs[l], (H, W, s, 255), 8, gs, nms)
            assert np.array_equal(cand, tw.cand) and count == [tw.cand.size, tw.n_above, 0, 0], (H, W, s, gs, nms)
            assert np.array_equal(stats[:3], tw.stats.view(np.int32)), "mean, std and threshold: the twin's bits"
            key = ("band", H, W, s, gs, nms)
            if key not in _cache:
                g64, thr64 = GR.threshold_f64(imgs[l], gs)
                band = (g64 - thr64).abs() <= BAND
                if nms and nms > 1:
                    band |= B._near_tie(g64, nms) <= BAND
                _cache[key] = band.flatten().numpy()
            band = _cache[key]
            want = _ref(H, W, s, gs, nms, denom=255)
            diff = np.setxor1d(cand, want)
            print(f"{H}x{W} seed {s} grad_std {gs} nms {nms}: {want.size} candidates, {diff.size} differ, {int(band[want].sum())} of torch's in the band")
            assert band[diff].all(), (H, W, s, gs, nms, diff[~band[diff]])
            assert band[want].sum() < 0.01 * want.size, "the restatement's own in-band population is below 1 % of its candidates on these inputs"


@pytest.mark.parametrize("H,W,block,seed", [(33, 130, 16, 3), (130, 513, 16, 3), (17, 65, 4, 9)])
def test_ridges_on_the_tile_seams(gpu, H, W, block, seed):
    """Block-constant images whose block edges fall on y % 16 == 0 and x % 64 == 0: tied maxima along and across the tile seams and through the halo
    corners, every one kept.

    Ties are asserted as fewer distinct gradient values than candidates, and directly: candidates with an equal value elsewhere in their own window.
    With 16 x 16 blocks (seed 3) both hold at every window size.  With 4 x 4 blocks a ridge of equal values is at most 4 pixels long, so a 7 x 7 or 15 x 15
    window keeps a handful of isolated maxima whose values are distinct (torch: 4 of 4 and 3 of 3 distinct at 17 x 65, and no seed of 0 .. 399 has ties
    at all three window sizes): there the ties are asserted at nms_size 3, the lists at all three."""
    img = GR.block_constant_image(H, W, seed, block=block)
    assert GR.guard_distance(img, 1.0) > GUARD
    assert 16 % block == 0 and 64 % block == 0 and H > 16 and W > 64           # a block edge on every tile seam, and a seam each way
    g2 = GR.image_grad(img)[0]
    g = g2.flatten()
    dev = img.to(gpu)
    for nms in (3, 7, 15):
        cand, count, stats = _run(dev, 2, 1.0, nms)[0]
        want, tw = GR.candidates(img, 2, 1.0, nms).numpy().astype(np.int32), TW.select(img, 2, 1.0, nms)
        assert np.array_equal(cand, want) and np.array_equal(cand, tw.cand), (H, W, block, nms)
        assert count == [want.size, tw.n_above, 0, 0] and np.array_equal(stats[:3], tw.stats.view(np.int32))
        assert want.size > 0
        if nms < block:
            idx = torch.from_numpy(want).long()
            assert g[idx].unique().numel() < want.size, "tied maxima exist and every one is kept"
            assert (B._near_tie(g2.double(), nms).flatten()[idx] == 0).any(), "a kept maximum has its equal inside its own window"
        if block == 16:         # candidates sit on the seams themselves: in a tile's first / last row or column
            v, u = want // W, want % W
            assert ((v % 16 == 0) | (v % 16 == 15)).any() and ((u % 64 == 0) | (u % 64 == 63)).any()


def test_max_lanes(gpu):
    """MV_MAX_LANES lanes, a different image each, all-zero lanes and a NaN lane among them: every lane is its twin."""
    from macvo_amd import _lib as L

    H, W, m, gs, nms = 33, 130, 4, 1.0, 7
    n = L.MV_MAX_LANES
    assert n == 64
    imgs = [_image(H, W, 100 + l) for l in range(n)]
    zero, nan = (0, 17, n - 1), 40
    for l in zero:
        imgs[l] = torch.zeros(3, H, W)
    imgs[nan] = imgs[nan].clone()
    imgs[nan][0, 16, 64] = float("nan")                                        # on the corner of four tiles
    got = _run(torch.stack(imgs).to(gpu), m, gs, nms)
    assert len(got) == n
    sizes = set()
    for l, (cand, count, stats) in enumerate(got):
        tw = TW.select(imgs[l], m, gs, nms)
        assert np.array_equal(cand, tw.cand) and count == [tw.cand.size, tw.n_above, 0, 0], l
        if l == nan:
            assert cand.size == 0 and np.isnan(stats.view(np.float32)[:3]).all() and np.isnan(tw.stats).all()
        else:
            assert np.array_equal(stats[:3], tw.stats.view(np.int32)), l
            assert (cand.size == 0) == (l in zero)
            sizes.add(cand.tobytes())
        assert stats[3] == 0
    assert len(sizes) == n - len(zero), "every lane has a candidate list of its own (the zero lanes share the empty one)"


def test_scaled_negated_and_overflowing_values(gpu):
    H, W, m, gs, nms = 33, 130, 4, 2.0, 7
    img = _image(H, W, 3)
    assert GR.guard_distance(img, gs) > GUARD
    dev = img.to(gpu)
    base = _run(dev, m, gs, nms)[0]
    assert np.array_equal(base[0], _ref(H, W, 3, gs, nms, m)) and base[0].size > 0
    f0 = base[2].view(np.float32)[:3]
    for s in (-20, 20):             # a power-of-two scaling of every step, no under- or overflow: the same candidates, the statistics scaled exactly
        cand, count, stats = _run(dev * 2.0 ** s, m, gs, nms)[0]
        assert np.array_equal(cand, base[0]) and count == base[1], s
        assert np.array_equal(stats.view(np.float32)[:3], f0 * np.float32(2.0 ** s)) and stats[3] == 0, s
        assert np.array_equal(cand, GR.candidates(img * 2.0 ** s, m, gs, nms).numpy().astype(np.int32))
    assert _same(_run(-dev, m, gs, nms)[0], base), "-image: the same candidates, the same statistics bits"
    other = _image(H, W, 5)
    other_alone = _run(other.to(gpu), m, gs, nms)[0]
    for bad_value in (float("inf"), float("-inf"), 3e38):                      # 3e38 overflows in the Laplacian's 4 * c
        bad = img.clone()
        bad[1, 16, 64] = bad_value
        tg = GR.image_grad(bad)
        # torch's: a NaN threshold and nothing selected (its mean is inf for 3e38; for +-inf its conv2d multiplies the stencil's zero corners: NaN)
        assert torch.isnan(GR.threshold(tg, gs)).all() and GR.candidates(bad, m, gs, nms).numel() == 0 and (bad_value != 3e38 or torch.isinf(tg.mean()))
        tw = TW.select(bad, m, gs, nms)
        assert tw.cand.size == 0 and tw.n_above == 0
        clean_a, bad_l, clean_b = _run(torch.stack([img, bad, other]).to(gpu), m, gs, nms)
        f = bad_l[2].view(np.float32)
        assert bad_l[0].size == 0 and bad_l[1] == [0, 0, 0, 0], bad_value
        assert f[0] == np.inf and np.isnan(f[1]) and np.isnan(f[2]) and tw.stats[0] == np.inf and np.isnan(tw.stats[1:]).all(), bad_value
        assert _same(clean_a, base) and _same(clean_b, other_alone), "the clean neighbours keep their bits"
        assert _same(_run(bad.to(gpu), m, gs, nms)[0], bad_l)


KITTI = (376, 1241)


def test_device_draw_on_a_long_candidate_list(gpu):
    """finish_device over about 43,000 candidates (the draw steps about 69 generator blocks of 624), twice on one generator, then over a short NMS list
    of the same image: the rows of torch.randperm of a generator seeded alike."""
    from macvo_amd import ops

    H, W = KITTI
    GS.check_path(H, W)
    img = _image(H, W, 3)
    dev = img.to(gpu)
    seed, k = 2024, 512
    g = torch.Generator().manual_seed(seed)
    state = ops.mt19937_state([seed], gpu)
    for gs, nms, lo, hi in ((1.0, None, 40000, 50000), (1.0, None, 40000, 50000), (3.0, 15, 1000, 4000)):
        assert GR.guard_distance(img, gs) > GUARD
        c = ops.kp_gradient(dev, 8, gs, nms)
        rows, n_sel = c.finish_device(k, state)
        n = int(c.count[0])
        assert lo < n < hi and n == _ref(H, W, 3, gs, nms).size, n
        want = GR.select(img, k, 8, gs, nms, generator=g)
        rows = rows.cpu()
        assert rows.shape == (1, k, 2) and rows.dtype == torch.int64 and n_sel.tolist() == [want.shape[0]] == [k]
        assert torch.equal(rows[0], want), (gs, nms)
    # zeros past n_sel need a list shorter than the head (512 at the most): a border that leaves two rows of the image, on the same generator
    c = ops.kp_gradient(dev, (H - 1) // 2, 1.0, None)
    rows, n_sel = c.finish_device(k, state)
    want = GR.select(img, k, (H - 1) // 2, 1.0, None, generator=g)
    n = int(n_sel[0])
    assert 0 < n == want.shape[0] < k and torch.equal(rows[0, :n].cpu(), want) and not rows[0, n:].any(), "rows at or past n_sel are zero"


def test_plugin_and_image_selector_at_kitti_size(gpu):
    import macvo_amd.plugins as P
    from macvo_amd.pipeline import image_selector

    H, W = KITTI
    img = _image(H, W, 3)
    m, gs, nms, k = 32, 2.0, 7, 300
    assert GR.guard_distance(img, gs) > GUARD
    select = image_selector({"type": "SparseGradienSelector", "args": {"mask_width": m, "grad_std": gs, "nms_size": nms}}, gpu, seeds=[41])
    rows, counts = select(img[None].to(gpu), k)
    want = GR.select(img, k, m, gs, nms, generator=torch.Generator().manual_seed(41))
    assert rows.shape == (1, k, 2) and counts.tolist() == [k] == [want.shape[0]] and torch.equal(rows[0].cpu(), want)
    sel = P.HIP_SparseGradienSelector(NS(mask_width=m, grad_std=gs, nms_size=nms))
    torch.manual_seed(43)
    got = sel.select_point(B._frame(img, gpu), k, None, None, None)
    torch.manual_seed(43)
    assert got.is_cuda and torch.equal(got.cpu(), GR.select(img, k, m, gs, nms))
