"""A 20-frame 640x480 one-lane pipe (NativeHotPath, or HotPath with --driver python) with the TartanMotionNet prior and a stand-in PoseNet
(one small matmul), software-pipelined through run(), for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o trace -- python tools/motion_model_run.py --motion-model tartan

(the motion_input_kernel / pose_exp_compose_kernel rows of OUT/.../trace_kernel_stats.csv are the prior's two launches, the
pgo_solve_kernel rows the solve started from it; `--motion-model static` is the same loop without them; profiles/motion_model_*.csv).

``--pose-net standin`` (default) is that small matmul; ``torch`` runs the real PoseNet eagerly (tools/posenet_torch.py, seeded weights) and ``hip``
runs it through ``ops.PoseNet`` (posenet_conv_kernel / posenet_head_kernel rows: 50 launches per frame).  ``--forward-lanes N`` times the PoseNet
alone instead of the pipe: stream time per forward (events around 50 calls), host time per call and, for ``hip``, the launch count."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def forward_only(pose_net, a, dev, calls: int = 50) -> None:
    import time

    from tools import posenet_torch as PT

    x = PT.sample_input(3, 5).repeat((a.forward_lanes + 2) // 3, 1, 1, 1)[:a.forward_lanes].contiguous().to(dev)
    for _ in range(5):
        pose_net(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        pose_net(x)
    e1.record()
    host = (time.perf_counter() - t0) / calls
    torch.cuda.synchronize()
    launches = 50 if a.pose_net == "hip" else None      # 3 firstconv + 2 x 23 blocks + 1 head (mv_posenet_forward_lanes)
    print(f"pose_net={a.pose_net} lanes={a.forward_lanes} stream_us_per_forward={e0.elapsed_time(e1) / calls * 1e3:.1f} "
          f"host_us_per_call={host * 1e6:.1f} launches={launches}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--motion-model", default="tartan", choices=("static", "tartan"))
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--driver", default="native", choices=("native", "python"))
    ap.add_argument("--pose-net", default="standin", choices=("standin", "torch", "hip"))
    ap.add_argument("--forward-lanes", type=int, default=0, help="time the PoseNet alone on this many lanes (no pipe)")
    a = ap.parse_args()
    from macvo_amd.pipeline import Camera, FrameInputs, HotPath, HotPathConfig, NativeHotPath
    from tools import synth

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    A, b = (torch.randn(6, 5, generator=g) * 0.5).to(dev), (torch.randn(6, generator=g) * 0.3).to(dev)

    def pose_net(x):   # stand-in for TartanVO's flowPoseNet: [L,5,112,160] -> [L,6]
        return torch.tanh(x.clamp(-1e3, 1e3).mean(dim=(2, 3))) @ A.T + b

    if a.pose_net != "standin":
        from macvo_amd import ops
        from tools import posenet_torch as PT

        sd = PT.seeded_state_dict(11)
        if a.pose_net == "hip":
            pose_net = ops.PoseNet.from_state_dict(sd, dev)
        else:
            eager = PT.from_state_dict(sd, dev)
            pose_net = torch.inference_mode()(lambda x: eager(x))
    if a.forward_lanes:
        forward_only(pose_net, a, dev)
        return

    cam, frames, _ = synth.make_sequence(4, 480, 640, C=256, iters=12, seed=3)
    cls = NativeHotPath if a.driver == "native" else HotPath
    hot = cls(Camera(**cam), HotPathConfig(graph_type="icp", motion_model=a.motion_model), dev, pose_net=pose_net)
    ins = [FrameInputs(**{k: v.to(dev) for k, v in fr.items()}) for fr in frames]
    hot.initialize(ins[0])
    torch.manual_seed(0)
    for _ in hot.run(ins[1 + t % 3] for t in range(a.frames)):
        pass
    torch.cuda.synchronize()
    print(f"driver={a.driver} motion_model={a.motion_model} pose_net={a.pose_net} frames={a.frames} pose={hot.pose.cpu().tolist()}")


if __name__ == "__main__":
    main()
