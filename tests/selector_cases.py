"""Inputs and the launch helper that the selector's GPU tests share (TEST INFRASTRUCTURE): network-shaped flow / covariance maps with NaN, +-inf and
plateau spots on the seams of the NMS kernel's 16 x 64 tiles, on the image corners and in the halo, and one call of the NODEPTH selector — fused with the
frontend epilogue or behind it — with every output brought back to the CPU.  Used by tests/test_gpu_nms_epilogue_first.py and
tests/test_gpu_selector_finish.py."""
import ctypes as C

import torch

BL_FX, BL_FX_SQ = 80.0, 6400.0


def inputs(H, W, lanes, cov_is_log):
    """flow, cov [lanes, 2, 2, H, W] on the CPU.  cov is log-sigma (expf(2 x) in the kernel) or the variance itself."""
    g = torch.Generator().manual_seed(1000 * H + W)
    flow = torch.randn(lanes, 2, 2, H, W, generator=g) * 4
    cov = torch.randn(lanes, 2, 2, H, W, generator=g) * 0.5
    if not cov_is_log:
        cov = cov.abs() + 0.01
    flow[:, 0, 0, 0, 0] = 0.0                                      # disparity 0: depth = inf, depth_cov = NaN (0 / 0 after the squares)
    flow[:, 0, 0, H - 1, W - 1] = -0.0
    flow[:, 0, 0, H // 2, W // 2] = float("nan")
    flow[:, 1, 0, 1, 1] = float("inf")
    nan, inf = float("nan"), float("inf")
    very_neg = -60.0 if cov_is_log else 1e-30                      # expf(-120) = 0 in fp32: a plateau of exact zeros with its neighbour
    # (row, column, value) on the two planes the quality map is made of: image corners and edges, the seams of the 16 x 64 tiles where there are
    # any (rows 15 | 16, columns 63 | 64: tile interior of one workgroup = halo of the next), and the interior
    spots = [(0, 0, nan), (0, W - 1, inf), (H - 1, 0, -inf), (H - 1, W - 1, very_neg), (H - 1, W - 2, very_neg), (0, W // 2, very_neg),
             (H // 2, 0, nan), (H // 2, W - 1, very_neg), (min(15, H - 1), min(63, W - 1), nan), (min(16, H - 1), min(64, W - 1), very_neg),
             (min(15, H - 1), min(64, W - 1), inf), (min(16, H - 1), min(62, W - 1), -inf), (H // 3, W // 3, very_neg), (H // 3, W // 3 + 1, very_neg),
             (2 * H // 3, 2 * W // 3, inf)]
    for i, (y, x, v) in enumerate(spots):
        if not cov_is_log and v == -inf:
            v = 0.0
        cov[:, 1, i % 2, y, x] = v
    cov[:, 0, 0, H // 2, W // 3] = nan                              # the stereo sample: disparity variance only
    cov[:, 0, 0, 0, W - 1] = very_neg
    if lanes > 1:
        cov[1, 1, :, :, W // 2:] += 0.25                            # the lanes differ
    return flow, cov


_cache = {}


def inputs_on(gpu, H, W, lanes, cov_is_log):
    key = (H, W, lanes, cov_is_log)
    if key not in _cache:
        _cache[key] = tuple(t.to(gpu) for t in inputs(H, W, lanes, cov_is_log))
    return _cache[key]


def run(lib, L, gpu, H, W, lanes, fused, flow, cov, cov_is_log, ksize, mask_width):
    """The fused launch, or mv_frontend_epilogue_lanes + mv_kp_select_lanes on the covariance planes it wrote; every output as CPU tensors."""
    from macvo_amd import ops

    mk = lambda c, dt=torch.float32: torch.full((lanes, c, H, W), 77, dtype=dt, device=gpu)  # noqa: E731
    out = {"disparity": mk(1), "disparity_cov": mk(1), "depth": mk(1), "depth_cov": mk(1), "bad_mask": mk(1, torch.uint8),
           "match_flow": mk(2), "match_cov": mk(3)}
    p = L.mvKpSelectParams(H, W, L.MV_KP_NODEPTH, ksize, mask_width, 0.0, 0.0, 100.0)
    nbytes = lib.mv_kp_select_workspace_bytes(H, W) * lanes
    ws = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=gpu)
    cand = torch.zeros(lanes, H * W, dtype=torch.int32, device=gpu)
    count = torch.zeros(lanes, 4, dtype=torch.int32, device=gpu)
    stats = torch.zeros(lanes, 4, dtype=torch.float32, device=gpu)
    s = ops._stream()
    o = {k: v.data_ptr() for k, v in out.items()}
    if fused:
        L.check(lib.mv_frontend_epilogue_select_lanes(flow.data_ptr(), cov.data_ptr(), int(cov_is_log), BL_FX, BL_FX_SQ, o["disparity"],
                                                      o["disparity_cov"], o["depth"], o["depth_cov"], o["bad_mask"], o["match_flow"],
                                                      o["match_cov"], None, None, C.byref(p), ws.data_ptr(), ws.numel() * 8, cand.data_ptr(),
                                                      count.data_ptr(), stats.data_ptr(), lanes, s), "mv_frontend_epilogue_select_lanes")
    else:
        L.check(lib.mv_frontend_epilogue_lanes(flow.data_ptr(), cov.data_ptr(), int(cov_is_log), H, W, BL_FX, BL_FX_SQ, o["disparity"],
                                               o["disparity_cov"], o["depth"], o["depth_cov"], o["bad_mask"], o["match_flow"], o["match_cov"],
                                               lanes, s), "mv_frontend_epilogue_lanes")
        L.check(lib.mv_kp_select_lanes(o["match_cov"], None, None, None, None, None, None, C.byref(p), ws.data_ptr(), ws.numel() * 8,
                                       cand.data_ptr(), count.data_ptr(), stats.data_ptr(), lanes, s), "mv_kp_select_lanes")
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in out.items()}
    res.update(cand=cand.cpu(), count=count.cpu(), stats=stats.cpu())
    return res


# ---------------------------------------------------------------------------------------------------- any mode, any workspace
def capacity(lib, H, W):
    """(records, candidate words) the in-register finishing form holds for H x W in this process: mv_kp_select_finish_capacity."""
    a, b = C.c_int32(), C.c_int32()
    assert lib.mv_kp_select_finish_capacity(H, W, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def fresh_workspace(lib, gpu, H, W, lanes=1):
    nbytes = lib.mv_kp_select_workspace_bytes(H, W) * lanes
    return torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=gpu)


def select(lib, L, gpu, mode, H, W, ksize, mask_width, maps, lanes=1, max_depth=0.0, max_depth_cov=0.0, max_match_cov=100.0, ws=None):
    """mv_kp_select_lanes on device maps (``maps``: flow_cov [lanes, 3, H, W], depth0 / depth0_cov / depth1 / depth1_cov [lanes, 1, H, W] fp32, mask_a /
    mask_b [lanes, 1, H, W] uint8; absent = NULL) on a fresh workspace or on ``ws``.  Returns the device outputs: cand [lanes, H * W] (filled with -1
    before the launch), count [lanes, 4], stats [lanes, 4]."""
    from macvo_amd import ops

    ptr = lambda name: None if maps.get(name) is None else maps[name].data_ptr()  # noqa: E731
    for name, t in maps.items():
        assert t is None or (t.is_contiguous() and t.shape[0] == lanes and t.shape[-2:] == (H, W)), name
    p = L.mvKpSelectParams(H, W, {"nodepth": L.MV_KP_NODEPTH, "full": L.MV_KP_FULL}[mode], ksize, mask_width, max_depth, max_depth_cov, max_match_cov)
    if ws is None:
        ws = fresh_workspace(lib, gpu, H, W, lanes)
    cand = torch.full((lanes, H * W), -1, dtype=torch.int32, device=gpu)
    count = torch.full((lanes, 4), -1, dtype=torch.int32, device=gpu)
    stats = torch.full((lanes, 4), -1.0, dtype=torch.float32, device=gpu)
    L.check(lib.mv_kp_select_lanes(ptr("flow_cov"), ptr("depth0"), ptr("depth0_cov"), ptr("depth1"), ptr("depth1_cov"), ptr("mask_a"), ptr("mask_b"),
                                   C.byref(p), ws.data_ptr(), ws.numel() * 8, cand.data_ptr(), count.data_ptr(), stats.data_ptr(), lanes,
                                   ops._stream()), "mv_kp_select_lanes")
    torch.cuda.synchronize()
    return {"cand": cand, "count": count, "stats": stats}


def synth_maps(H, W):
    """The synthetic maps of tools/synth.py on the CPU: flow_cov (seed 2), depth0 / depth0_cov (3), depth1 / depth1_cov (4); the tilted depth plane spans
    3 .. 58 m, so FULL_MAX_DEPTH gives both outcomes of the depth test."""
    from tools import synth

    d0, d0c = synth.depth_maps(H, W, 3)
    d1, d1c = synth.depth_maps(H, W, 4)
    return {"flow_cov": synth.flow_cov_maps(H, W, 2), "depth0": d0, "depth0_cov": d0c, "depth1": d1, "depth1_cov": d1c}


FULL_MAX_DEPTH, FULL_MAX_DEPTH_COV, MAX_MATCH_COV = 40.0, 250.0, 100.0
VARIANT_CASES = [(360, 480, 3), (96, 130, 7)]      # H, W, window: past 8192 records / far below (see finish_variant_child)
VARIANT_MASK_WIDTH = 8


def finish_variant_child(out_dir):
    """Runs in an interpreter of its own (MV_KP_FINISH_SMALL_NT is read once per process): VARIANT_CASES in NODEPTH and FULL, candidates / counts / stats and
    the capacities the library reported saved under ``out_dir``.  Under MV_KP_FINISH_SMALL_NT=512 the capacity must be that of the 512-thread variant."""
    import os

    from macvo_amd import _lib as L

    lib = L.load()
    gpu = torch.device("cuda:0")
    out = {}
    for (H, W, k) in VARIANT_CASES:
        caps = capacity(lib, H, W)
        if os.environ.get("MV_KP_FINISH_SMALL_NT") == "512":
            assert caps == (8192, 5120), caps
        maps = {n: t.to(gpu) for n, t in synth_maps(H, W).items()}
        for mode in ("nodepth", "full"):
            use = {"flow_cov": maps["flow_cov"]} if mode == "nodepth" else maps
            r = select(lib, L, gpu, mode, H, W, k, VARIANT_MASK_WIDTH, use, max_depth=FULL_MAX_DEPTH, max_depth_cov=FULL_MAX_DEPTH_COV,
                       max_match_cov=MAX_MATCH_COV)
            n = int(r["count"][0, 0])
            out[(H, W, k, mode)] = {"cand": r["cand"][0, :n].cpu(), "count": r["count"][0].cpu(), "stats": r["stats"][0].cpu(), "caps": caps}
    torch.save(out, os.path.join(out_dir, "variant.pt"))
