"""640x480 one-lane NativeHotPath runs with and without frontend covariances in ONE process, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o trace -- python tools/covfree_run.py --configs vanilla,default-random,default

`vanilla` = Ablation_Study/TartanAirv2_Vanilla.yaml (frontend_cov (False, False), RandomSelector, NoCovariance, SimpleDepthFilter, icp): per frame
the volume GEMM, 12 lookups, frontend_epilogue_partial_kernel<false, false> (no covariance plane read or written), no selector kernel,
backend_front_kernel<4, 2, false, true> and the solve.  `default-random` is the same pipe with both covariances (frontend_epilogue_kernel,
backend_front_kernel<4, 0, false, false>: MatchCovariance on RandomSelector's rows) — the like-for-like rows to hold Vanilla's epilogue and front
launch against; `default` is HotPathConfig() as it is (fused epilogue + CovAware selector, permutation drawn in backend_front_kernel<2, 0, false,
false>).  `10` / `01` are the mixed frontends with MatchCovariance.  profiles/covfree_all_kernel_stats.csv is the trace of all five; DESIGN.md has the
per-frame launch list read off it."""
import argparse
import os
import sys
from dataclasses import replace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="vanilla,default-random,default")
    ap.add_argument("--frames", type=int, default=40)
    a = ap.parse_args()
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, FrameInputs, HotPathConfig, NativeHotPath
    from tools import synth

    dev = torch.device("cuda:0")
    cam, frames, _ = synth.make_sequence(4, 480, 640, C=256, iters=12, seed=3)
    ins = [FrameInputs(**{k: v.to(dev) for k, v in fr.items()}) for fr in frames]
    mapless = dict(selector="random", graph_type="icp", filters=ops.FILTER_SIMPLE_DEPTH)
    cfgs = {
        "vanilla": HotPathConfig(frontend_cov=(False, False), cov_model="none", **mapless),
        "default-random": HotPathConfig(**mapless),
        "default": HotPathConfig(),
        "10": HotPathConfig(frontend_cov=(True, False), **mapless),
        "01": HotPathConfig(frontend_cov=(False, True), **mapless),
    }
    for name in a.configs.split(","):
        cfg = cfgs[name]
        d, m = cfg.frontend_cov
        xs = ins if (d or m) else [replace(x, logcov=None) for x in ins]
        hot = NativeHotPath(Camera(**cam), cfg, dev, generators=[7])
        hot.initialize(xs[0])
        n_valid = []
        for t in range(a.frames):
            r = hot.step(xs[1 + t % 3])
            n_valid.append(int(r.n_valid.item()) if r.n_valid is not None else 0)
        torch.cuda.synchronize()
        print(f"config={name} frontend_cov={cfg.frontend_cov} frames={a.frames} observations(min)={min(n_valid)} pose={hot.pose.cpu().tolist()}")
        hot.close()


if __name__ == "__main__":
    main()
