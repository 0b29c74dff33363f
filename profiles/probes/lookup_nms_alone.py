#!/usr/bin/env python
"""Alone-times of the two small chip-wide launches of the frame chain, back to back on an otherwise idle GPU: the radius-4 window lookup of
one frame (B = 2 pairs x 4800 queries, fp32 cells) and of a 64-pair batch, and the fused epilogue + selector entry point
mv_frontend_epilogue_select_lanes at 640 x 480 (kp_nms_kernel<true> + the finishing workgroup), beside the unfused selector.

    [MACVO_HIP_LIB=<another build's libmacvo_hip.so>] python profiles/probes/lookup_nms_alone.py [--reps 400] [--rounds 5]

Each figure is (time between two HIP events around `reps` launches) / reps = the launch's period when nothing else runs; the median and the
range over `rounds` repetitions are printed.  For an A/B, run the two builds in alternating processes."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from macvo_amd import _lib as L  # noqa: E402
from macvo_amd import ops  # noqa: E402


def period(fn, reps, rounds):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = L.load()
    print("library:", os.environ.get("MACVO_HIP_LIB") or L.LIB_PATH)
    g = torch.Generator().manual_seed(0)
    h8, w8 = 60, 80
    for B in (2, 64):
        vol = torch.randn(B * h8 * w8, 1, h8, w8, device=dev)
        ys, xs = torch.meshgrid(torch.arange(h8), torch.arange(w8), indexing="ij")
        coords = (torch.stack([xs, ys]).float()[None] + (torch.rand(B, 2, h8, w8, generator=g) * 2 - 1) * 8).to(dev)
        tok = torch.empty(B, 81, h8, w8, device=dev)
        s = ops._stream()
        args = (vol.data_ptr(), coords.data_ptr(), tok.data_ptr(), B, h8, w8, h8, w8, 4, s)
        med, lo, hi = period(lambda: lib.mv_corr_lookup(*args), a.reps if B == 2 else a.reps // 8, a.rounds)
        print(f"lookup r=4 fp32 cells  B={B:2d}  {med:7.2f} us  [{lo:.2f} .. {hi:.2f}]")
        del vol, coords, tok
    H, W = 480, 640
    flow = (torch.randn(2, 2, H, W, generator=g) * 4).to(dev)
    cov = (torch.randn(2, 2, H, W, generator=g) * 0.5).to(dev)
    med, lo, hi = period(lambda: ops.frontend_epilogue_select(flow, cov, 0.25, 320.0, kernel_size=7, mask_width=32, max_match_cov=100.0),
                         a.reps // 4, a.rounds)
    print(f"epilogue + selector, fused entry point (allocations of the wrapper included)  {med:7.2f} us  [{lo:.2f} .. {hi:.2f}]")
    # the same entry point with every buffer allocated once: the launches alone
    import ctypes as C
    mk = lambda c: torch.empty(1, c, H, W, device=dev)  # noqa: E731
    o = [mk(1), mk(1), mk(1), mk(1), mk(2), mk(3)]
    p = L.mvKpSelectParams(H, W, L.MV_KP_NODEPTH, 7, 32, 0.0, 0.0, 100.0)
    nbytes = lib.mv_kp_select_workspace_bytes(H, W)
    ws = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    cand = torch.empty(H * W, dtype=torch.int32, device=dev)
    count, stats = torch.empty(4, dtype=torch.int32, device=dev), torch.empty(4, device=dev)
    s = ops._stream()
    fargs = (flow.data_ptr(), cov.data_ptr(), 1, 80.0, 6400.0, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), None,
             o[4].data_ptr(), o[5].data_ptr(), None, None, C.byref(p), ws.data_ptr(), ws.numel() * 8, cand.data_ptr(), count.data_ptr(),
             stats.data_ptr(), 1, s)
    med, lo, hi = period(lambda: lib.mv_frontend_epilogue_select_lanes(*fargs), a.reps, a.rounds)
    print(f"mv_frontend_epilogue_select_lanes (kp_nms_kernel<true> + finishing workgroup)  {med:7.2f} us  [{lo:.2f} .. {hi:.2f}]")
    uargs = (o[5].data_ptr(), None, None, None, None, None, None, C.byref(p), ws.data_ptr(), ws.numel() * 8, cand.data_ptr(), count.data_ptr(),
             stats.data_ptr(), 1, s)
    med, lo, hi = period(lambda: lib.mv_kp_select_lanes(*uargs), a.reps, a.rounds)
    print(f"mv_kp_select_lanes        (kp_nms_kernel<false> + finishing workgroup)         {med:7.2f} us  [{lo:.2f} .. {hi:.2f}]")
    print("records / candidates of the last call:", int(count[1]), int(count[0]))


if __name__ == "__main__":
    main()
