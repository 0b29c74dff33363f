"""A one-lane 640x480 pipe (NativeHotPath, integer seed = the device-driven frame) with a chosen keypoint selector, software-pipelined through
run(), for a kernel trace and for driver-style frame rates:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o trace -- python tools/selector_run.py --selector random
    python tools/selector_run.py --selector nodepth --frames 300 --repeat 5      # prints one frames/s figure per repeat

(`--selector random | grid` enqueue no selector kernels and draw / compute the keypoint rows inside backend_front_kernel<4 | 5, ...>;
`nodepth` is the CovAware selector + the permutation draw of backend_front_kernel<2, ...>; profiles/selectors_*_kernel_stats.csv.  The library
of another build can be timed with MACVO_HIP_LIB=<path to its libmacvo_hip.so> for the selectors it knows.)"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--selector", default="random", choices=("nodepth", "full", "random", "grid"))
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    from macvo_amd.pipeline import Camera, FrameInputs, HotPathConfig, NativeHotPath
    from tools import synth

    dev = torch.device("cuda:0")
    cam, frames, _ = synth.make_sequence(4, 480, 640, C=256, iters=12, seed=3)
    hot = NativeHotPath(Camera(**cam), HotPathConfig(selector=a.selector), dev, generators=[a.seed])
    ins = [FrameInputs(**{k: v.to(dev) for k, v in fr.items()}, static=True) for fr in frames]
    hot.initialize(ins[0])
    for _ in hot.run(ins[1 + t % 3] for t in range(a.warmup)):
        pass
    torch.cuda.synchronize()
    fps = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        for _ in hot.run(ins[1 + t % 3] for t in range(a.frames)):
            pass
        torch.cuda.synchronize()
        fps.append(a.frames / (time.perf_counter() - t0))
    print(f"selector={a.selector} device_driven={hot.device_driven} frames={a.frames} frames_per_s={[round(f, 1) for f in fps]} pose={hot.pose.cpu().tolist()}")
    hot.close()


if __name__ == "__main__":
    main()
