"""A 20-frame 640x480 one-lane pipe (NativeHotPath, or HotPath with --driver python) with the TartanMotionNet prior and a stand-in PoseNet
(one small matmul), software-pipelined through run(), for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o trace -- python tools/motion_model_run.py --motion-model tartan

(the motion_input_kernel / pose_exp_compose_kernel rows of OUT/.../trace_kernel_stats.csv are the prior's two launches, the
pgo_solve_kernel rows the solve started from it; `--motion-model static` is the same loop without them; profiles/motion_model_*.csv)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--motion-model", default="tartan", choices=("static", "tartan"))
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--driver", default="native", choices=("native", "python"))
    a = ap.parse_args()
    from macvo_amd.pipeline import Camera, FrameInputs, HotPath, HotPathConfig, NativeHotPath
    from tools import synth

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    A, b = (torch.randn(6, 5, generator=g) * 0.5).to(dev), (torch.randn(6, generator=g) * 0.3).to(dev)

    def pose_net(x):   # stand-in for TartanVO's flowPoseNet: [L,5,112,160] -> [L,6]
        return torch.tanh(x.clamp(-1e3, 1e3).mean(dim=(2, 3))) @ A.T + b

    cam, frames, _ = synth.make_sequence(4, 480, 640, C=256, iters=12, seed=3)
    cls = NativeHotPath if a.driver == "native" else HotPath
    hot = cls(Camera(**cam), HotPathConfig(graph_type="icp", motion_model=a.motion_model), dev, pose_net=pose_net)
    ins = [FrameInputs(**{k: v.to(dev) for k, v in fr.items()}) for fr in frames]
    hot.initialize(ins[0])
    torch.manual_seed(0)
    for _ in hot.run(ins[1 + t % 3] for t in range(a.frames)):
        pass
    torch.cuda.synchronize()
    print(f"driver={a.driver} motion_model={a.motion_model} frames={a.frames} pose={hot.pose.cpu().tolist()}")


if __name__ == "__main__":
    main()
