"""A 20-frame 640x480 one-lane NativeHotPath with a chosen observation-covariance model, for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o trace -- python tools/cov_model_run.py --cov-model gmm

(the backend_front_kernel rows of OUT/.../trace_kernel_stats.csv are the fused covariance launch; profiles/cov_models_*.csv)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cov-model", default="match", choices=("match", "gmm", "none"))
    ap.add_argument("--cov-modifiers", default="", help="comma-separated, innermost first: diag,normalize")
    ap.add_argument("--frames", type=int, default=20)
    a = ap.parse_args()
    from macvo_amd.pipeline import Camera, FrameInputs, HotPathConfig, NativeHotPath
    from tools import synth

    dev = torch.device("cuda:0")
    cam, frames, _ = synth.make_sequence(4, 480, 640, C=256, iters=12, seed=3)
    mods = tuple(m for m in a.cov_modifiers.split(",") if m)
    hot = NativeHotPath(Camera(**cam), HotPathConfig(graph_type="icp", cov_model=a.cov_model, cov_modifiers=mods), dev, generators=[7])
    ins = [FrameInputs(**{k: v.to(dev) for k, v in fr.items()}) for fr in frames]
    hot.initialize(ins[0])
    for t in range(a.frames):
        hot.step(ins[1 + t % 3])
    torch.cuda.synchronize()
    print(f"cov_model={a.cov_model} modifiers={mods} frames={a.frames} pose={hot.pose.cpu().tolist()}")
    hot.close()


if __name__ == "__main__":
    main()
