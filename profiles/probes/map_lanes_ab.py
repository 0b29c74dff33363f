#!/usr/bin/env python
"""What one device-resident map per lane costs ("One map per lane of a batched pipe").

    python profiles/probes/map_lanes_ab.py kernel [--lanes 32 --cap 200 --reps 40]
        mv_map_append_lanes (one launch, one workgroup per lane) against `lanes` back-to-back mv_map_append launches on the SAME tables (lane slices of the
        [lanes, cap, .] / [11, lanes, cap] buffers: the one-frame kernel takes a row stride) — the only way the one-frame kernel can do the same work.
        Prints HIP-event times per frame; run it under `rocprofv3 --kernel-trace --stats` for the kernels' own durations.
    python profiles/probes/map_lanes_ab.py pipe [--variants plain,maps --lanes 32 --steps 300 --repeats 3] [--tree DIR]
        frames/s of a 32-lane pipe at 640 x 480 with and without maps attached, alternating in one process, a fresh pipe per measurement.
        Variant `map` attaches through attach_map instead of attach_maps (one map, --lanes 1).
        --tree DIR: import the package from another checkout (e.g. the parent commit, `--variants plain`) — same script, same frames, same call.
One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "pipe"])
    ap.add_argument("--lanes", type=int, default=32)
    ap.add_argument("--cap", type=int, default=200)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pool", type=int, default=6)
    ap.add_argument("--variants", default="plain,maps")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    root = os.path.abspath(args.tree or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    sys.path.insert(0, root)
    import torch

    (kernel if args.mode == "kernel" else pipe)(args, torch, root)


def kernel(args, torch, root):
    from macvo_amd import _lib as L
    from macvo_amd import ops
    from macvo_amd.devmap import DeviceVisualMaps

    dev, lanes, cap = torch.device("cuda:0"), args.lanes, args.cap
    lib = L.load()
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    t = dict(kp0=r(lanes, cap, 2), kp1=r(lanes, cap, 2), vals=r(11, lanes, cap), sigma0=r(lanes, cap, 3), sigma1=r(lanes, cap, 3), cov0=r(lanes, cap, 9).double(),
             cov1=r(lanes, cap, 9).double(), pos=r(lanes, cap, 3), cov0w=r(lanes, cap, 9).double(), prior=r(lanes, 7), tbs=r(lanes, 7), K=r(9))
    valid = (torch.rand(lanes, cap, generator=g) < 0.9).to(torch.uint8).to(dev)
    rows = (args.reps + 4) * cap
    size = 1 << (rows + 1).bit_length()
    a, b = DeviceVisualMaps(lanes, dev, init_size=size), DeviceVisualMaps(lanes, dev, init_size=size)
    n_rows, times = (C.c_int32 * lanes)(*[cap] * lanes), (C.c_int64 * lanes)(*range(lanes))
    p = lambda x: x.data_ptr()  # noqa: E731
    fl = L.mvMapFrameLanes(lanes=lanes, cap=cap, prev_frame=-1, min_num_point=10, n_rows=C.cast(n_rows, C.c_void_p), time_ns=C.cast(times, C.c_void_p),
                           valid=p(valid), kp0=p(t["kp0"]), kp1=p(t["kp1"]), vals=p(t["vals"]), sigma0=p(t["sigma0"]), sigma1=p(t["sigma1"]), cov0=p(t["cov0"]),
                           cov1=p(t["cov1"]), pos_Tw=p(t["pos"]), cov0_world=p(t["cov0w"]), color=None, K=p(t["K"]), T_BS=p(t["tbs"]), prior_pose=p(t["prior"]),
                           baseline=0.25)

    def one(l, prev):   # the one-frame kernel on lane l's slice of the same tables
        o = l * cap
        return L.mvMapFrame(n_rows=cap, table_stride=lanes * cap, prev_frame=prev, min_num_point=10, valid=p(valid) + o, kp0=p(t["kp0"]) + 8 * o,
                            kp1=p(t["kp1"]) + 8 * o, vals=p(t["vals"]) + 4 * o, sigma0=p(t["sigma0"]) + 12 * o, sigma1=p(t["sigma1"]) + 12 * o,
                            cov0=p(t["cov0"]) + 72 * o, cov1=p(t["cov1"]) + 72 * o, pos_Tw=p(t["pos"]) + 12 * o, cov0_world=p(t["cov0w"]) + 72 * o, color=None,
                            K=p(t["K"]), T_BS=p(t["tbs"]) + 28 * l, prior_pose=p(t["prior"]) + 28 * l, baseline=0.25, time_ns=l, out_frame_idx=None)

    st = ops._stream()
    stores_b = [m.stores() for m in b]
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    ms = {"lanes": [], "one_by_one": []}
    for i in range(args.reps + 4):
        prev = i - 1
        fl.prev_frame = prev
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        L.check(lib.mv_map_append_lanes(C.byref(fl), a.stores_dev(), st), "lanes")
        e1.record()
        for l in range(lanes):
            f = one(l, prev)
            L.check(lib.mv_map_append(C.byref(f), C.byref(stores_b[l]), st), "one")
        e2.record()
        torch.cuda.synchronize()
        if i >= 4:
            ms["lanes"].append(e0.elapsed_time(e1))
            ms["one_by_one"].append(e1.elapsed_time(e2))
    for ma, mb in zip(a, b):    # same tables -> same maps
        assert ma.counts.cpu().tolist() == mb.counts.cpu().tolist() and ma.counts.cpu()[4] == 0
        n = int(ma.counts.cpu()[1])
        assert torch.equal(ma.match["obs1_covTc"][:n], mb.match["obs1_covTc"][:n]) and torch.equal(ma.match["pixel2_d"][:n], mb.match["pixel2_d"][:n])
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    print(json.dumps({"probe": "map_lanes_kernel", "lanes": lanes, "cap": cap, "reps": args.reps, "event_ms_lanes_median": med(ms["lanes"]),
                      "event_ms_one_by_one_median": med(ms["one_by_one"]), "ratio": med(ms["one_by_one"]) / med(ms["lanes"]),
                      "event_ms_lanes_min_max": [min(ms["lanes"]), max(ms["lanes"])], "event_ms_one_by_one_min_max": [min(ms["one_by_one"]), max(ms["one_by_one"])]}))


def pipe(args, torch, root):
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, FrameInputs, HotPathConfig, NativeHotPath, stack_lanes
    from tools import synth

    dev, lanes, pool = torch.device("cuda:0"), args.lanes, args.pool
    cam, frames_cpu, _ = synth.make_sequence(pool, 480, 640, C=256, iters=12, seed=1000, pool=pool, closed_loop=True)
    frames = [FrameInputs(static=True, **{k: v.to(dev) for k, v in fr.items()}) for fr in frames_cpu]
    batches = [stack_lanes([frames[(t + l) % pool] for l in range(lanes)]) for t in range(pool)]
    K = torch.tensor([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1.0]])
    torch.cuda.synchronize()

    def measure(variant):
        hot = NativeHotPath(Camera(**cam), HotPathConfig(graph_type="disp", volume_precision=ops.default_volume_precision()), dev, lanes=lanes,
                            generators=[7 + l for l in range(lanes)])
        mps = None
        if variant in ("map", "maps"):
            from macvo_amd.devmap import DeviceVisualMap, DeviceVisualMaps

            rows = (args.steps + args.warmup + 2) * 200
            size = 1 << (rows + 1).bit_length()                                            # (no re-growth inside the timed region)
            if variant == "map":                                                           # the one-map call: --lanes 1
                mps = [DeviceVisualMap(dev, init_size=size)]
                hot.attach_map(mps[0], K)
            else:
                mps = DeviceVisualMaps(lanes, dev, init_size=size)
                hot.attach_maps(mps, K)
        hot.initialize(batches[0])
        sink = torch.zeros(args.steps, lanes, 7, device=dev)
        for _ in hot.run(batches[(1 + k) % pool] for k in range(args.warmup)):
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in hot.run((batches[(1 + args.warmup + k) % pool] for k in range(args.steps)), pose_sink=sink):
            pass
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out = {"probe": "map_lanes_pipe", "tag": args.tag, "variant": variant, "lanes": lanes, "steps": args.steps, "frames_per_s": args.steps * lanes / dt,
               "device_driven": bool(hot.device_driven)}
        if mps is not None:
            c = [m.counts.cpu().tolist() for m in mps]
            out["frames_in_map"], out["refused"] = c[0][0], sum(x[4] for x in c)
        hot.close()
        del hot, mps
        return out

    measure(args.variants.split(",")[0])        # clocks, allocator, first-use set-up
    for _ in range(args.repeats):
        for v in args.variants.split(","):
            print(json.dumps(measure(v)), flush=True)


if __name__ == "__main__":
    main()
