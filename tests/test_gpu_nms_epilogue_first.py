"""The selector's NMS launch with its epilogue first (every load of a thread in one burst at entry, the nine epilogue stores per pixel in front of the
NMS phases): the fused entry point against the separate epilogue followed by the un-fused selector, bit for bit on every output, at the smallest shapes
at which the kernel can go wrong — one 16 x 64 tile exactly, ragged last tiles in both axes, a width below one tile, a height below one tile —, with both
window sizes of the selectors, a border mask of 0 and one that leaves a strip of candidates, one and two lanes, log-sigma and plain covariance input,
and NaN / +-inf / very negative values in the tile, in the halo and on the image border.  The number of NMS pixels is checked against max_pool2d on the
CPU as well, so that the pair does not merely agree with itself.  One FULL and one MAPPING case through the un-fused kernel against the oracle's selectors
(FULL requests the two depths of its own pixels in front of the LDS phases now)."""
import pytest
import torch

from tests.selector_cases import inputs_on as _inputs_on, run as _run

pytestmark = pytest.mark.gpu

SHAPES = [(16, 64), (33, 130), (40, 72), (20, 50), (9, 70)]      # H x W; tiles are 16 x 64


@pytest.mark.parametrize("cov_is_log", [True, False])
@pytest.mark.parametrize("ksize", [7, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_fused_launch_is_bitwise_the_epilogue_then_the_selector(gpu, H, W, ksize, cov_is_log):
    from macvo_amd import _lib as L

    lib = L.load()
    few = (min(H, W) - 2) // 2                                      # leaves a strip two or three pixels wide
    for lanes in (1, 2):
        flow, cov = _inputs_on(gpu, H, W, lanes, cov_is_log)
        for mask_width in (0, few):
            tag = (lanes, mask_width)
            fu = _run(lib, L, gpu, H, W, lanes, True, flow, cov, cov_is_log, ksize, mask_width)
            un = _run(lib, L, gpu, H, W, lanes, False, flow, cov, cov_is_log, ksize, mask_width)
            for name in ("disparity", "disparity_cov", "depth", "depth_cov", "match_flow", "match_cov"):   # the nine planes, NaN payloads included
                assert torch.equal(fu[name].view(torch.int32), un[name].view(torch.int32)), (name, tag)
            assert torch.equal(fu["bad_mask"], un["bad_mask"]), tag
            assert torch.equal(fu["count"], un["count"]), tag        # candidates, records (= NMS pixels), 0, 0
            assert torch.equal(fu["stats"].view(torch.int32), un["stats"].view(torch.int32)), tag
            for ln in range(lanes):
                n = int(fu["count"][ln, 0])
                assert torch.equal(fu["cand"][ln, :n], un["cand"][ln, :n]), (tag, ln)
                if mask_width == 0:
                    assert n == 0                                    # `border[mw:-mw]` of the reference is empty for 0
                # the NMS pixels of max_pool2d(-q) on the covariance planes the launch wrote (the device's expf is part of the input here)
                q = (fu["match_cov"][ln, 0] + fu["match_cov"][ln, 1] - 2 * fu["match_cov"][ln, 2])[None, None]
                erode = -torch.nn.functional.max_pool2d(-q, kernel_size=ksize, stride=1, padding=ksize // 2)
                assert int(fu["count"][ln, 1]) == int(torch.logical_and(q == erode, ~q.isnan()).sum()), (tag, ln)
            # the maps themselves: what the epilogue is defined to write, from the CPU
            assert torch.equal(fu["disparity"][:, 0].view(torch.int32), flow[:, 0, 0].abs().cpu().view(torch.int32)), tag
            assert torch.equal(fu["match_flow"].view(torch.int32), flow[:, 1].cpu().view(torch.int32)), tag
            assert torch.equal(fu["bad_mask"][:, 0] != 0, flow[:, 0, 0].cpu() <= 0), tag
            if not cov_is_log:
                assert torch.equal(fu["match_cov"][:, :2].view(torch.int32), cov[:, 1].cpu().view(torch.int32)), tag
            assert int(fu["match_cov"][:, 2].view(torch.int32).abs().max()) == 0, tag


def test_fused_launch_matches_the_oracle_selector(gpu):
    """40 x 72, no special values: candidates, median and threshold of the fused launch against the oracle's CovAwareSelector_NoDepth."""
    from macvo_amd import _lib as L
    from oracle import selector

    H, W, mw = 40, 72, 6
    lib = L.load()
    g = torch.Generator().manual_seed(5)
    flow = (torch.randn(1, 2, 2, H, W, generator=g) * 4).to(gpu)
    cov = (torch.randn(1, 2, 2, H, W, generator=g) * 0.5).to(gpu)
    for ksize in (7, 3):
        fu = _run(lib, L, gpu, H, W, 1, True, flow, cov, True, ksize, mw)
        _, ref_cand, aux = selector.cov_aware_selector_nodepth(fu["match_cov"].clone(), 10, ksize, mw, 100.0)
        n = int(fu["count"][0, 0])
        lin = fu["cand"][0, :n].long()
        assert n > 0 and torch.equal(torch.stack([lin // W, lin % W], dim=1), ref_cand)
        assert int(fu["count"][0, 1]) == aux["n_nms"]
        assert fu["stats"][0, 0].item() == aux["median"]


def test_unfused_full_and_mapping_match_the_oracle(gpu):
    """FULL (its two depths are requested in front of the LDS phases now) and MAPPING at 40 x 100 — ragged tiles in both axes — against the oracle's selectors."""
    from macvo_amd import ops
    from oracle import selector
    from tools import synth

    H, W, mw = 40, 100, 5
    d0, d0c = synth.depth_maps(H, W, 3)
    d1, d1c = synth.depth_maps(H, W, 4)
    fc = synth.flow_cov_maps(H, W, 2)
    d0c[0, 0, 5, 7] = float("nan")
    d0[0, 0, 20, 64] = float("nan")                                 # a depth that fails `<` on a tile seam
    d1[0, 0, 17, 30] = float("inf")
    max_depth = 40.0                                                # the tilted plane spans 3..58 m: both outcomes of the depth test
    dv = lambda t: t.to(gpu)  # noqa: E731
    for flow_cov in (fc, None):
        torch.manual_seed(11)
        ref_px, ref_cand, aux = selector.cov_aware_selector(d0, d0c, d1, d1c, None if flow_cov is None else flow_cov.clone(), 20, max_depth, 7, mw,
                                                            250.0, 100.0)
        torch.manual_seed(11)
        c = ops.kp_select("full", H, W, flow_cov=None if flow_cov is None else dv(flow_cov), depth0=dv(d0), depth0_cov=dv(d0c), depth1=dv(d1),
                          depth1_cov=dv(d1c), kernel_size=7, mask_width=mw, max_depth=max_depth, max_depth_cov=250.0, max_match_cov=100.0)
        assert torch.equal(c.candidates_vu().cpu(), ref_cand)
        assert torch.equal(c.finish(20).cpu(), ref_px)
        assert c.stats[2].item() == aux["median_depth_cov"]
    torch.manual_seed(12)
    ref_px, ref_cand, _ = selector.mapping_point_selector(d0, d0c, 50, 20.0, 0.2, mw)
    assert ref_cand.shape[0] > 50
    torch.manual_seed(12)
    c = ops.kp_select("mapping", H, W, depth0=dv(d0), depth0_cov=dv(d0c), mask_width=mw, max_depth=20.0, max_depth_cov=0.2)
    assert torch.equal(c.candidates_vu().cpu(), ref_cand)
    assert torch.equal(c.finish(50).cpu(), ref_px)
