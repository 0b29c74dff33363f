#!/usr/bin/env python
"""Stand-alone timing of individual C-ABI kernels on the GPU box (HIP events, median of N launches).

    python tools/kernel_bench.py [volume_f32 volume_f16 lookup select cov pgo eval eval_traj traj_assoc remap rectify_maps ...] [--iters 50]

Used for A/B tuning and as the target of `rocprofv3 --pmc ...` runs (one kernel family per process).
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from macvo_amd import ops  # noqa: E402
from tools import synth  # noqa: E402


def timeit(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


def synth_coords(B, h8, w8, dev):
    g = torch.Generator().manual_seed(1)
    base = torch.stack([torch.arange(w8).float()[None].expand(h8, w8), torch.arange(h8).float()[:, None].expand(h8, w8)])[None]
    return (base + (torch.rand(B, 2, h8, w8, generator=g) * 2 - 1) * 8).to(dev)

# one call of a recurrent update block (csrc/update_block_math.h): (launch, kh * kw, cin, rows executed, rows that are real outputs)
UPDATE_LAUNCHES = {
    "cov": [("zr1 1x5", 5, 512, 256, 256), ("q1 1x5", 5, 512, 128, 128), ("zr2 5x1", 5, 512, 256, 256), ("q2 5x1", 5, 512, 128, 128),
            ("conv1|mask.0 3x3", 9, 128, 512, 512), ("conv2 3x3", 9, 256, 128, 128), ("conv3 3x3", 9, 128, 64, 64), ("conv4 3x3", 9, 64, 64, 2),
            ("mask.2 1x1", 1, 256, 576, 576)],
    "flow": [("zr1 1x5", 5, 512, 256, 256), ("q1 1x5", 5, 512, 128, 128), ("zr2 5x1", 5, 512, 256, 256), ("q2 5x1", 5, 512, 128, 128),
             ("flow_head.0|mask.0 3x3", 9, 128, 512, 512), ("flow_head.2 3x3", 9, 256, 64, 2), ("mask.2 1x1", 1, 256, 576, 576)],
}
MFMA16_PEAK_TFLOPS = 2500.0     # dense bf16 / fp16 MFMA rate of an MI355X


def update_block_case(a, dev, B, h8, w8):
    """The HIP update block against the eager PyTorch-ROCm module with the same bf16 weights and inputs, in this process: median, min and the 10th-90th
    percentile spread of each, the useful FLOP of every launch, and — with --launch-trace FILE, a rocprofv3 --kernel-trace CSV of THIS case — the
    measured time and achieved fraction of the 16-bit MFMA rate per launch."""
    from tests import update_block_twin as T

    M = B * h8 * w8
    for kind in a.update_kinds.split(","):
        block = T.make_block(T.COV if kind == "cov" else T.FLOW, 0).to(dev, torch.bfloat16)
        net, inp = (t.to(dev, torch.bfloat16) for t in T.make_inputs((B, h8, w8), 0))
        wts = ops.UpdateBlockWeights.from_module(block, kind, "bf16")
        launches = UPDATE_LAUNCHES[kind]
        useful = sum(2.0 * M * t * cin * real for _, t, cin, _, real in launches)

        def spread(fn):
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(max(a.iters, 20)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            ts.sort()
            return statistics.median(ts), ts[0], ts[len(ts) // 10], ts[len(ts) * 9 // 10]
        with torch.inference_mode():
            hip = spread(lambda: ops.update_block(net, inp, wts))
            eager = spread(lambda: block(net, inp))
        print(f"update_block {kind} bf16 B={B} {h8}x{w8} (M = {M}, {useful / 1e9:.2f} GFLOP): HIP {hip[0]:.1f} us (min {hip[1]:.1f}, p10-p90 {hip[2]:.1f}-{hip[3]:.1f}) = "
              f"{useful / hip[0] / 1e6 / MFMA16_PEAK_TFLOPS * 100:.1f}% of the 16-bit MFMA rate; eager {eager[0]:.1f} us (min {eager[1]:.1f}, p10-p90 "
              f"{eager[2]:.1f}-{eager[3]:.1f}); eager / HIP = {eager[0] / hip[0]:.2f}")
        if a.launch_trace:
            import csv
            rows = [r for r in csv.DictReader(open(a.launch_trace)) if "update_conv_kernel" in r["Kernel_Name"] or "update_to_nhwc" in r["Kernel_Name"]]
            rows.sort(key=lambda r: int(r["Start_Timestamp"]))
            per = len(launches) + 1
            first = next(i for i, r in enumerate(rows) if "update_to_nhwc" in r["Kernel_Name"])
            calls = [rows[i:i + per] for i in range(first, len(rows) - per + 1, per)]
            calls = [c for c in calls if "update_to_nhwc" in c[0]["Kernel_Name"] and all("update_conv" in r["Kernel_Name"] for r in c[1:])]
            calls = calls[len(calls) // 2:]                    # the second half of the whole calls: past the warm-up
            print(f"per launch, mean of {len(calls)} traced calls: us, executed GFLOP, % of the 16-bit MFMA rate")
            for j, name in enumerate(["to_nhwc"] + [n for n, *_ in launches]):
                us = statistics.mean((int(c[j]["End_Timestamp"]) - int(c[j]["Start_Timestamp"])) / 1e3 for c in calls)
                fl = 0.0 if j == 0 else 2.0 * M * launches[j - 1][1] * launches[j - 1][2] * launches[j - 1][3]
                print(f"  {name:24s} {us:8.1f} us {fl / 1e9:7.2f} GFLOP {fl / us / 1e6 / MFMA16_PEAK_TFLOPS * 100:6.1f}%")


# one call of the motion encoder (csrc/motion_encoder_math.h): (launch, kh * kw of the launch, cin of the launch, rows executed, useful MACs per pixel)
MOTION_LAUNCHES = [("convc1 1x1", 1, 192, 256, 256 * 145), ("convc2 3x3", 9, 256, 192, 192 * 9 * 256), ("convf1 as 1x1", 1, 128, 128, 128 * 98),
                   ("convf2 3x3", 9, 128, 64, 64 * 9 * 128), ("conv 3x3", 9, 256, 128, 126 * 9 * 256)]


def motion_encoder_case(a, dev, B, h8, w8):
    """The HIP motion encoder against the eager PyTorch-ROCm module with the same bf16 weights and inputs, in this process: median, min and the 10th-90th
    percentile spread of each (the update_block case's method), the useful FLOP of the module, and — with --launch-trace FILE, a rocprofv3 --kernel-trace
    CSV of THIS case — the measured time and achieved fraction of the 16-bit MFMA rate per launch."""
    from tests import motion_encoder_twin as T

    M = B * h8 * w8
    module = T.make_module(0).to(dev, torch.bfloat16)
    flow, corr = (t.to(dev, torch.bfloat16) for t in T.make_inputs((B, h8, w8), 0))
    wts = ops.MotionEncoderWeights.from_module(module, "bf16")
    useful = sum(2.0 * M * macs for *_, macs in MOTION_LAUNCHES)

    def spread(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(a.iters, 20)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts.sort()
        return statistics.median(ts), ts[0], ts[len(ts) // 10], ts[len(ts) * 9 // 10]
    with torch.inference_mode():
        hip = spread(lambda: ops.motion_encoder(flow, corr, wts))
        eager = spread(lambda: module(flow, corr))
    faster = eager[0] - hip[0] > eager[3] - eager[2]
    print(f"motion_encoder bf16 B={B} {h8}x{w8} (M = {M}, {useful / 1e9:.2f} GFLOP): HIP {hip[0]:.1f} us (min {hip[1]:.1f}, p10-p90 {hip[2]:.1f}-{hip[3]:.1f}) = "
          f"{useful / hip[0] / 1e6 / MFMA16_PEAK_TFLOPS * 100:.1f}% of the 16-bit MFMA rate; eager {eager[0]:.1f} us (min {eager[1]:.1f}, p10-p90 "
          f"{eager[2]:.1f}-{eager[3]:.1f}); eager / HIP = {eager[0] / hip[0]:.2f}; difference of medians {eager[0] - hip[0]:.1f} us "
          f"{'exceeds' if faster else 'does NOT exceed'} the eager p10-p90 spread of {eager[3] - eager[2]:.1f} us")
    if a.launch_trace:
        import csv
        rows = [r for r in csv.DictReader(open(a.launch_trace)) if "update_conv_kernel" in r["Kernel_Name"] or "motion_stage" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        per = len(MOTION_LAUNCHES) + 1
        first = next(i for i, r in enumerate(rows) if "motion_stage" in r["Kernel_Name"])
        calls = [rows[i:i + per] for i in range(first, len(rows) - per + 1, per)]
        calls = [c for c in calls if "motion_stage" in c[0]["Kernel_Name"] and all("update_conv" in r["Kernel_Name"] for r in c[1:])]
        calls = calls[len(calls) // 2:]                        # the second half of the whole calls: past the warm-up
        print(f"per launch, mean of {len(calls)} traced calls: us, executed GFLOP, % of the 16-bit MFMA rate")
        for j, name in enumerate(["motion_stage"] + [n for n, *_ in MOTION_LAUNCHES]):
            us = statistics.mean((int(c[j]["End_Timestamp"]) - int(c[j]["Start_Timestamp"])) / 1e3 for c in calls)
            fl = 0.0 if j == 0 else 2.0 * M * MOTION_LAUNCHES[j - 1][1] * MOTION_LAUNCHES[j - 1][2] * MOTION_LAUNCHES[j - 1][3]
            print(f"  {name:24s} {us:8.1f} us {fl / 1e9:7.2f} GFLOP {fl / us / 1e6 / MFMA16_PEAK_TFLOPS * 100:6.1f}%")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["volume_f32", "volume_f16", "lookup", "select", "cov", "pgo"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--H", type=int, default=480)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--B", type=int, default=2)
    ap.add_argument("--zeros", action="store_true", help="volume_split: all-zero operands (DVFS probe: same instruction stream, less switching power)")
    ap.add_argument("--launch-trace", default="", help="update_block, motion_encoder: a rocprofv3 --kernel-trace CSV of this case, for the per-launch table")
    ap.add_argument("--update-kinds", default="cov,flow", help="update_block: the kinds to time (a trace for --launch-trace holds one kind only)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W, B, C = a.H, a.W, a.B, 256
    h8, w8 = H // 8, W // 8
    n = h8 * w8
    g = torch.Generator().manual_seed(0)
    f1, f2 = torch.randn(B, C, h8, w8, generator=g).to(dev), torch.randn(B, C, h8, w8, generator=g).to(dev)
    flops = B * 2.0 * n * n * C
    vol = torch.empty((B * n, 1, h8, w8), dtype=torch.float32, device=dev)
    for w in a.what:
        if w == "volume_f32":
            med, mn = timeit(lambda: ops.corr_volume(f1, f2, "chw", out=vol), a.iters)
            print(f"volume_f32_chw  B={B} {med:8.1f} us (min {mn:.1f})  {flops / med / 1e6:7.1f} TFLOP/s  {flops / med / 1e6 / 157.3 * 100:.1f}% of f32 MFMA peak")
            a1, a2 = f1.permute(0, 2, 3, 1).contiguous(), f2.permute(0, 2, 3, 1).contiguous()
            med, mn = timeit(lambda: ops.corr_volume(a1, a2, "hwc", out=vol), a.iters)
            print(f"volume_f32_hwc  B={B} {med:8.1f} us (min {mn:.1f})  {flops / med / 1e6:7.1f} TFLOP/s")
            med, mn = timeit(lambda: ops.corr_volume(a1, a2, "hwc", out=vol, precision="split3"), a.iters)
            print(f"volume_split3_hwc B={B} {med:6.1f} us (min {mn:.1f})  {flops / med / 1e6:7.1f} TFLOP/s algorithmic")
        elif w == "volume_split":
            z1, z2 = (torch.zeros_like(f1), torch.zeros_like(f2)) if a.zeros else (f1, f2)
            for mode, nprod in (("bf16x3", 6), ("f16x2", 3)):
                if os.environ.get("MV_SPLIT_MODE", mode) != mode:
                    continue
                pk = ops.volume_pack(z1, z2, mode=mode)
                med, mn = timeit(lambda: ops.volume_pack(z1, z2, out=pk, mode=mode), a.iters)
                print(f"volume_pack  {mode} B={B} {med:8.1f} us (min {mn:.1f})")
                for _ in range(100):
                    ops.corr_volume_packed(pk[0], pk[1], B, C, n, n, out=vol, mode=mode)
                med, mn = timeit(lambda: ops.corr_volume_packed(pk[0], pk[1], B, C, n, n, out=vol, mode=mode), a.iters, warm=20)
                print(f"volume_split {mode} B={B} {med:8.1f} us (min {mn:.1f})  {flops / med / 1e6:7.1f} TFLOP/s algorithmic = {nprod * flops / med / 1e6 / 2500 * 100:.1f}% of the "
                      f"16-bit MFMA peak executed ({'zero' if a.zeros else 'random'} operands)")
        elif w == "update_block":
            update_block_case(a, dev, B, h8, w8)
        elif w == "motion_encoder":
            motion_encoder_case(a, dev, B, h8, w8)
        elif w == "patch_embed":
            # (f)2: both volumes of a frame (S = B n slices) through the fused conv stack; 2 x (36 + 16*36*... ) MAC per output, see DESIGN
            from tools.synth import patch_embed_weights
            if not ops.cost_patch_embed_supported(h8, w8):
                print(f"patch_embed: no kernel for {h8}x{w8} slices")
                continue
            Wt = [t.to(dev) for t in patch_embed_weights(0)]
            hp, wpd = (h8 + 7) // 8 * 8, (w8 + 7) // 8 * 8
            m1, m2, m3 = hp * wpd // 4, hp * wpd // 16, hp * wpd // 64
            volr = torch.randn(B * n, 1, h8, w8, device=dev) * 16
            outp = torch.empty((B * n, m3, 64), dtype=torch.float32, device=dev)
            fl = B * n * 2.0 * (m1 * 16 * 36 + m2 * 32 * 576 + m3 * 64 * 1152)
            byts = B * n * (h8 * w8 * 4 + m3 * 64 * 4.0)
            print(f"patch_embed: S = {B * n} slices {h8}x{w8} -> {m3} tokens, {fl / 1e9:.1f} GFLOP, MV_PE_STRIP={os.environ.get('MV_PE_STRIP', '0')}")
            for operand in ("f16", "bf16"):
                pk = ops.PatchEmbedWeights(*Wt, operand=operand)
                for _ in range(5):
                    ops.cost_patch_embed(volr, pk, tokens=True, out=outp)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                reps = max(3, a.iters // 5)
                e0.record()
                for _ in range(reps):
                    ops.cost_patch_embed(volr, pk, tokens=True, out=outp)
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / reps
                print(f"cost_patch_embed<{operand}> S={B * n} {us:8.1f} us  {fl / us / 1e6:7.1f} TFLOP/s algorithmic = {fl / us / 1e6 / 2500 * 100:.1f}% of the 16-bit MFMA peak; "
                      f"HBM {byts / us / 1e3:.0f} GB/s ({byts / 1e6:.0f} MB)")
                # Fast mode (row (f)2): 16-bit cells in, 16-bit tokens out — half the HBM bytes, no conversion in the staging
                dt16 = torch.float16 if operand == "f16" else torch.bfloat16
                vol16, out16 = volr.to(dt16), torch.empty((B * n, m3, 64), dtype=dt16, device=dev)
                for _ in range(5):
                    ops.cost_patch_embed(vol16, pk, tokens=True, out=out16)
                e0.record()
                for _ in range(reps):
                    ops.cost_patch_embed(vol16, pk, tokens=True, out=out16)
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / reps
                print(f"cost_patch_embed<{operand}, 16-bit in/out> S={B * n} {us:8.1f} us  {fl / us / 1e6:7.1f} TFLOP/s algorithmic = {fl / us / 1e6 / 2500 * 100:.1f}% of the 16-bit MFMA "
                      f"peak; HBM {byts / 2 / us / 1e3:.0f} GB/s ({byts / 2e6:.0f} MB)")
                del vol16, out16
            # the unfused form: the same three layers as PyTorch / MIOpen convolutions (bf16, channels_last), intermediates through HBM
            import torch.nn.functional as F
            if (h8, w8) != (60, 80):
                continue                                      # (the unfused chain at 720p is 3 x 10 GB of intermediates: skipped)
            xb = F.pad(volr, (0, 0, 0, 4)).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            wb = [t.to(torch.bfloat16) for t in Wt]
            def unfused():
                y = F.relu(F.conv2d(xb, wb[0], wb[1], stride=2, padding=2))
                y = F.relu(F.conv2d(y, wb[2], wb[3], stride=2, padding=2))
                return F.conv2d(y, wb[4], wb[5], stride=2, padding=2)
            try:
                for _ in range(2):
                    unfused()
                e0.record()
                for _ in range(3):
                    unfused()
                e1.record()
                torch.cuda.synchronize()
                print(f"  unfused torch conv2d chain (bf16, channels_last, MIOpen): {e0.elapsed_time(e1) * 1e3 / 3:8.1f} us")
            except Exception as e:  # noqa: BLE001
                print("  unfused torch conv2d chain failed:", repr(e)[:200])
        elif w == "dataset_ab":
            # KITTI / EuRoC frames (--H 376 --W 784: 47 x 98 maps, N = 4606; --H 480 --W 752: 60 x 94, N = 5640): N2 % 64 != 0.  Every kernel that serves such a frame
            # next to what served it before the ragged edge was built, in alternating rounds (the spread of a leg over the rounds is its run-to-run spread):
            #   fp32 features   : precision "exact" (the former dispatch for f16x2 / bf16x3 at these N)        vs  pack + corr_volume_split_stream<f16x2 | bf16x3>
            #   fp16 features   : 2-byte cells as corr_volume_h_hwc + cast (MV_H_STREAM=0 in the environment: another process)   vs  corr_volume_h_stream<out16>;
            #                     fp32 cells run corr_volume_h_hwc either way (no ragged streaming form: it measured slower)
            #   patch embedding : the three Conv2d layers (MIOpen) on the padded slices   vs  cost_patch_embed on the padded and on the RAW slices (fp32 cells; 16-bit cells in / tokens out)
            import torch.nn.functional as F
            from tools.synth import patch_embed_weights
            a1, a2 = f1.permute(0, 2, 3, 1).contiguous().half(), f2.permute(0, 2, 3, 1).contiguous().half()
            v16 = torch.empty((B * n, 1, h8, w8), dtype=torch.float16, device=dev)
            Wt = [t.to(dev) for t in patch_embed_weights(0)]
            pk = ops.PatchEmbedWeights(*Wt, operand="f16")
            S = n                                                  # one pair's slices
            m3 = ((h8 + 7) // 8) * ((w8 + 7) // 8)
            raw32 = torch.randn(S, 1, h8, w8, device=dev) * 16
            cells32 = F.pad(raw32, (0, (8 - w8 % 8) % 8, 0, (8 - h8 % 8) % 8)).contiguous()   # as PatchEmbed.forward hands them to `proj`
            raw16 = raw32.half()
            cells16 = cells32.half()
            tok32, tok16 = torch.empty((S, m3, 64), dtype=torch.float32, device=dev), torch.empty((S, m3, 64), dtype=torch.float16, device=dev)
            w16 = [t.half() for t in Wt]

            def layers(x, wts):
                y = F.relu(F.conv2d(x, wts[0], wts[1], stride=2, padding=2))
                y = F.relu(F.conv2d(y, wts[2], wts[3], stride=2, padding=2))
                return F.conv2d(y, wts[4], wts[5], stride=2, padding=2)

            def vol16_cast():                                       # 2-byte cells without the out16 kernel: the fp32-cell volume + a cast
                v16.copy_(ops.corr_volume(a1, a2, "hwc", out=vol))

            def vol16():                                            # (MV_H_STREAM=0 switches the fp32-cell dispatch only: that process takes the cast form here too)
                if os.environ.get("MV_H_STREAM", "1") == "0" or ops.corr_volume_out16(a1, a2, out=v16) is None:
                    vol16_cast()

            legs = [("volume fp32 exact", lambda: ops.corr_volume(f1, f2, "chw", out=vol, precision="exact")),
                    ("volume fp32 f16x2 (pack + GEMM)", lambda: ops.corr_volume(f1, f2, "chw", out=vol, precision="f16x2")),
                    ("volume fp32 bf16x3 (pack + GEMM)", lambda: ops.corr_volume(f1, f2, "chw", out=vol, precision="bf16x3")),
                    ("volume fp16 hwc, fp32 cells", lambda: ops.corr_volume(a1, a2, "hwc", out=vol)),
                    ("volume fp16 hwc, 2-byte cells", vol16),
                    ("patch embed: Conv2d layers fp32", lambda: layers(cells32, Wt)),
                    ("patch embed: fused, fp32 cells", lambda: ops.cost_patch_embed(cells32, pk, tokens=True, out=tok32)),
                    ("patch embed: Conv2d layers fp16", lambda: layers(cells16, w16)),
                    ("patch embed: fused, fp16 cells + tokens", lambda: ops.cost_patch_embed(cells16, pk, tokens=True, out=tok16)),
                    ("patch embed: fused, RAW fp32 cells", lambda: ops.cost_patch_embed(raw32, pk, tokens=True, out=tok32)),
                    ("patch embed: fused, RAW fp16 cells + tokens", lambda: ops.cost_patch_embed(raw16, pk, tokens=True, out=tok16))]
            rounds, res, names = 7, {k: [] for k, _ in legs}, {}
            for r in range(rounds):
                for k, fn in legs:
                    res[k].append(timeit(fn, max(3, a.iters // 10), warm=2 if r else 5)[0])
                    if k.startswith("volume"):
                        names[k] = ops.last_volume_kernel()
            print(f"dataset_ab {H}x{W}: maps {h8}x{w8}, N = {n} (N % 64 = {n % 64}), B = {B}, S = {S}, MV_H_STREAM={os.environ.get('MV_H_STREAM', '1')}; us per call, median of the rounds [min .. max]")
            for k, _ in legs:
                v = sorted(res[k])
                print(f"  {k:42s} {statistics.median(v):9.1f} [{v[0]:9.1f} .. {v[-1]:9.1f}]  {names.get(k, '')}")
        elif w == "volume_f16":
            for dt in (torch.float16, torch.bfloat16):
                a1, a2 = f1.permute(0, 2, 3, 1).contiguous().to(dt), f2.permute(0, 2, 3, 1).contiguous().to(dt)
                byts = B * (2.0 * n * C * 2 + 4.0 * n * n)
                med, mn = timeit(lambda: ops.corr_volume(a1, a2, "hwc", out=vol), a.iters)
                print(f"volume_{str(dt)[6:]}_hwc B={B} {med:8.1f} us (min {mn:.1f})  {byts / med / 1e3:7.1f} GB/s  {byts / med / 1e3 / 8000 * 100:.1f}% of HBM peak")
                v16 = ops.corr_volume_out16(a1, a2)
                if v16 is not None:
                    b16 = B * (2.0 * n * C * 2 + 2.0 * n * n)
                    med, mn = timeit(lambda: ops.corr_volume_out16(a1, a2, out=v16), a.iters)
                    print(f"volume_{str(dt)[6:]}_hwc_out16 B={B} {med:8.1f} us (min {mn:.1f})  {b16 / med / 1e3:7.1f} GB/s  {b16 / med / 1e3 / 8000 * 100:.1f}% of HBM peak ({b16 / 1e6:.0f} MB)")
                    if dt == torch.float16:
                        co = synth_coords(B, h8, w8, dev)
                        tok = ops.corr_lookup(v16, co, 4)
                        med, mn = timeit(lambda: ops.corr_lookup(v16, co, 4, out=tok), a.iters)
                        print(f"lookup_vol16 B={B} {med:8.1f} us (min {mn:.1f})")
                        vt = ops.corr_volume_out16(a1, a2, tiled=True)
                        med, mn = timeit(lambda: ops.corr_lookup(vt, co, 4, out=tok, tiled=True, image_hw=(h8, w8)), a.iters)
                        print(f"lookup_vol16_tiled B={B} {med:8.1f} us (min {mn:.1f})")
                        del vt
                        v32 = v16.float()
                        med, mn = timeit(lambda: ops.corr_lookup(v32, co, 4, out=tok), a.iters)
                        print(f"lookup_vol32 B={B} {med:8.1f} us (min {mn:.1f})")
                        del v32
                    del v16
                c1, c2 = f1.to(dt), f2.to(dt)
                med, mn = timeit(lambda: ops.corr_volume(c1, c2, "chw", out=vol), a.iters)
                print(f"volume_{str(dt)[6:]}_chw B={B} {med:8.1f} us (min {mn:.1f})  {byts / med / 1e3:7.1f} GB/s")
        elif w == "lookup":
            ops.corr_volume(f1, f2, "chw", out=vol)
            from tools.synth import coords_grid

            coords = (coords_grid(B, h8, w8) + (torch.rand(B, 2, h8, w8, generator=g) * 2 - 1) * 8).to(dev)
            tok = torch.empty((B, 81, h8, w8), dtype=torch.float32, device=dev)
            byts = B * (n * 100 * 4 + n * 8 + n * 81 * 4.0)
            med, mn = timeit(lambda: ops.corr_lookup(vol, coords, 4, out=tok), a.iters)
            print(f"lookup r=4      B={B} {med:8.1f} us (min {mn:.1f})  {byts / med / 1e3:7.1f} GB/s algorithmic")
        elif w == "localcorr":
            # PWC pyramid levels of a 640x448 input (pwc_model.py:178-233): (C, H, W)
            for (cc, hh, ww) in ((196, 7, 10), (128, 14, 20), (96, 28, 40), (64, 56, 80), (32, 112, 160)):
                a1, a2 = torch.randn(1, cc, hh, ww, generator=g).to(dev), torch.randn(1, cc, hh, ww, generator=g).to(dev)
                o = torch.empty(1, 81, hh, ww, device=dev)
                med, mn = timeit(lambda: ops.local_corr81(a1, a2, out=o), a.iters)
                fl = 2.0 * 81 * cc * hh * ww
                print(f"local_corr81 C={cc:3d} {hh}x{ww:<3d} {med:7.1f} us (min {mn:.1f})  {fl / med / 1e3:8.1f} GFLOP/s")
        elif w == "upsample":
            fl = torch.randn(B, 2, h8, w8, generator=g).to(dev)
            mk = torch.randn(B, 576, h8, w8, generator=g).to(dev)
            byts = B * (578 * n * 4 + 2 * 64 * n * 4.0)
            for mdt in (torch.float32, torch.bfloat16):
                mkd = mk.to(mdt)
                byts = B * ((576 * mkd.element_size() + 8) * n + 2 * 64 * n * 4.0)
                for _ in range(5):
                    ops.convex_upsample(fl, mkd, 0.25)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                reps = 4 * a.iters
                e0.record()
                for _ in range(reps):          # back to back: the figure is the kernel's period, not a launch + event round trip
                    ops.convex_upsample(fl, mkd, 0.25)
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / reps
                print(f"convex_upsample B={B} mask {str(mdt)[6:]} {us:8.2f} us back to back  {byts / us / 1e3:7.1f} GB/s  {byts / us / 1e3 / 8000 * 100:.1f}% of HBM peak ({byts / 1e6:.1f} MB)")
        elif w == "upsample_crop":
            # --H / --W of any size (376 x 780, 237 x 315): the window form against what a caller needed before it — the padded kernel and the
            # `.contiguous()` copy of the un-padded slice.  Back to back on one stream; under `rocprofv3 --kernel-trace --stats` the three kernels show by name.
            ch8, cw8 = ops.eighth_shape(H, W)
            win = ops.unpad_window(H, W) or (0, 0, H, W)
            y0, x0 = win[0], win[1]
            cfl = torch.randn(B, 2, ch8, cw8, generator=g).to(dev)
            cmk = torch.randn(B, 576, ch8, cw8, generator=g).to(dev)
            cout = torch.empty(B, 2, H, W, device=dev)
            legs = {"padded": lambda: ops.convex_upsample(cfl, cmkd, 1.0, True),
                    "padded + slice copy": lambda: ops.convex_upsample(cfl, cmkd, 1.0, True)[..., y0: y0 + H, x0: x0 + W].contiguous(),
                    "crop": lambda: ops.convex_upsample(cfl, cmkd, 1.0, True, crop=(y0, x0, H, W), out=cout)}
            for mdt in (torch.float32, torch.bfloat16):
                cmkd = cmk.to(mdt)
                for name, fn in legs.items():
                    for _ in range(5):
                        fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    reps = 4 * a.iters
                    e0.record()
                    for _ in range(reps):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    print(f"convex_upsample {ch8}x{cw8} -> {H}x{W} B={B} mask {str(mdt)[6:]:8s} {name:20s} {e0.elapsed_time(e1) * 1e3 / reps:8.2f} us back to back")
        elif w == "eval":
            # ops.eval_flow / ops.eval_depth with covariance (csrc/eval_metrics.hip) next to the same closed form in torch on the same device and inputs
            # (no SVD, no host read-back, masked means as where(...).nanmean()), lanes 1 and 32, in alternating rounds of back-to-back calls
            # (>= 200 calls per leg; the spread over the rounds is the run-to-run spread).  Under `rocprofv3 --kernel-trace --stats` the kernels show by name.
            def torch_grid(grid, a0, a1, scale):
                i0, i1 = (a0 * scale).to(torch.int64), (a1 * scale).to(torch.int64)      # NaN / inf -> INT64_MIN: outside, as numpy's astype(int)
                ok = (i0 >= 0) & (i0 < 100) & (i1 >= 0) & (i1 < 100)
                lane = torch.arange(a0.shape[0], device=a0.device)[:, None].expand_as(i0)
                grid.view(-1).index_add_(0, torch.where(ok, lane * 10000 + i0 * 100 + i1, 0).reshape(-1), ok.reshape(-1).to(grid.dtype))

            def torch_cov_fields(nll, unc, mask):
                nanv = torch.full_like(nll, float("nan"))
                out = [torch.where(mask, nll, nanv).nanmean(1)]
                qs = torch.nanquantile(unc, torch.tensor([0.25, 0.5, 0.75], device=unc.device), dim=1)
                return out + [torch.where(unc < qs[i][:, None], nll, nanv).nanmean(1) for i in range(3)] + [qs[0], qs[1], qs[2]]

            def torch_flow(est, gt, cov, valid, max_flow, gu, gv):
                L_ = est.shape[0]
                e = (est - gt).reshape(L_, 2, -1)
                eu, ev = e[:, 0], e[:, 1]
                epe = (eu * eu + ev * ev).sqrt()
                mask = (est[:, 0] < max_flow).reshape(L_, -1) & (est[:, 1] < max_flow).reshape(L_, -1) & valid.reshape(L_, -1)
                nanv = torch.full_like(epe, float("nan"))
                me = torch.where(mask, epe, nanv)
                nm = mask.sum(1).float()
                out = [me.nanmean(1), epe.nanmean(1)] + [((me < k).sum(1).float() / nm) for k in (1, 3, 5)]
                cu, cv = cov[:, 0].reshape(L_, -1), cov[:, 1].reshape(L_, -1)
                det = cu * cv
                cut = torch.maximum(cu.abs(), cv.abs()) * 1e-15
                pu, pv = torch.where(cu.abs() > cut, 1.0 / cu, 0.0), torch.where(cv.abs() > cut, 1.0 / cv, 0.0)
                r = ((eu * pu) * eu + (ev * pv) * ev).sqrt()
                out += torch_cov_fields(det.log() + r * r, det, mask)
                torch_grid(gu, eu * eu, cu, 4.0)
                torch_grid(gv, ev * ev, cv, 4.0)
                return torch.stack(out, 1)

            def torch_depth(est, gt, cov, max_depth, gd):
                L_ = est.shape[0]
                est, gt, c = est.reshape(L_, -1), gt.reshape(L_, -1), cov.reshape(L_, -1)
                e = est - gt
                mask = est < max_depth
                me = torch.where(mask, e.abs(), torch.full_like(e, float("nan")))
                out = [me.nanmean(1), torch.nanquantile(me, 0.25, dim=1), me.nanmedian(1).values, torch.nanquantile(me, 0.75, dim=1)]
                r = ((e * torch.where(c != 0, 1.0 / c, 0.0)) * e).sqrt()
                out += torch_cov_fields(c.log() + r * r, c, mask)
                torch_grid(gd, e * e, c, 2.0)
                return torch.stack(out, 1)

            for lanes in (1, 32):
                gt_f = torch.randn(lanes, 2, H, W, generator=g) * 4
                est_f = (gt_f + torch.randn(lanes, 2, H, W, generator=g) * torch.exp(torch.randn(lanes, 2, H, W, generator=g))).to(dev)
                cov_f = torch.exp(torch.randn(lanes, 2, H, W, generator=g) * 1.5).to(dev)
                valid = (torch.rand(lanes, 1, H, W, generator=g) > 0.15).to(dev)
                gt_d = torch.rand(lanes, 1, H, W, generator=g) * 40 + 0.5
                est_d = (gt_d + torch.randn(lanes, 1, H, W, generator=g)).to(dev)
                cov_d = torch.exp(torch.randn(lanes, 1, H, W, generator=g) * 1.5).to(dev)
                gt_f[torch.rand(lanes, 2, H, W, generator=g) < 0.03] = float("nan")
                gt_f, gt_d = gt_f.to(dev), gt_d.to(dev)
                from macvo_amd import _lib as L_

                frows = torch.empty(lanes, 1, len(L_.EVAL_FLOW_COLS), device=dev)
                drows = torch.empty(lanes, 1, len(L_.EVAL_DEPTH_COLS), device=dev)
                fgr = torch.zeros(lanes, 2, 100, 100, dtype=torch.int32, device=dev)
                dgr = torch.zeros(lanes, 100, 100, dtype=torch.int32, device=dev)
                tg = [torch.zeros(lanes, 100, 100, dtype=torch.int32, device=dev) for _ in range(3)]
                legs = [("eval_flow  HIP", lambda: ops.eval_flow(est_f, gt_f, cov_f, valid, 8.0, True, rows=frows, row=0, grids=fgr)),
                        ("eval_flow  torch closed form", lambda: torch_flow(est_f, gt_f, cov_f, valid, 8.0, tg[0], tg[1])),
                        ("eval_depth HIP", lambda: ops.eval_depth(est_d, gt_d, cov_d, 30.0, rows=drows, row=0, grids=dgr)),
                        ("eval_depth torch closed form", lambda: torch_depth(est_d, gt_d, cov_d, 30.0, tg[2]))]
                # same answers first (the HIP side is tested bit for bit elsewhere; this guards the comparator)
                hf, tf = legs[0][1]().row[:, :12], legs[1][1]()
                hd, td = legs[2][1]().row[:, :11], legs[3][1]()
                torch.cuda.synchronize()
                print(f"lanes {lanes}: max |HIP - torch| over the row fields: flow {float((hf - tf).abs().nan_to_num().max()):.3e} depth {float((hd - td).abs().nan_to_num().max()):.3e}")
                rounds, per = 5, max(8, (4 * a.iters) // 5)
                res = {k: [] for k, _ in legs}
                for k, fn in legs:
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                for _ in range(rounds):
                    for k, fn in legs:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(per):
                            fn()
                        e1.record()
                        torch.cuda.synchronize()
                        res[k].append(e0.elapsed_time(e1) * 1e3 / per)
                nb_f, nb_d = lanes * (H * W * (6 * 4 + 1) + 19 * 4 + 2 * 40000), lanes * (H * W * 3 * 4 + 18 * 4 + 40000)
                for k, _ in legs:
                    v = res[k]
                    print(f"{k:30s} {H}x{W} lanes {lanes:2d}: median {statistics.median(v):9.1f} us / call (rounds {min(v):.1f} .. {max(v):.1f}; {rounds * per} calls)")
                for kind, nb in (("flow", nb_f), ("depth", nb_d)):
                    h, t_ = statistics.median(res[f"eval_{kind:5s} HIP"]), statistics.median(res[f"eval_{kind:5s} torch closed form"])
                    print(f"eval_{kind}: torch / HIP = {t_ / h:.2f}x; algorithmic bytes {nb / 1e6:.2f} MB = {nb / 8e6:.2f} us at 8 TB/s; "
                          "launches per HIP call: 1 memset + 4 kernels")
        elif w == "eval_traj":
            # ops.eval_trajectory (csrc/traj_eval.hip: ATE / RTE / ROE / RPE, Umeyama alignment, one workgroup per lane) next to the same closed form in
            # torch on the same device (batched torch.linalg.svd) and to the numpy restatement with its read-back (tests/traj_ref.py, once: it is a
            # Python loop over the pairs)
            import time

            from tests import traj_ref as TR

            def quat_R(q):                                          # [..., 4] (x y z w) -> [..., 3, 3], evo's quaternion_matrix
                q = q * torch.sqrt(2.0 / (q * q).sum(-1, keepdim=True))
                x, y, z, w_ = q.unbind(-1)
                return torch.stack([1 - y * y - z * z, x * y - z * w_, x * z + y * w_, x * y + z * w_, 1 - x * x - z * z, y * z - x * w_,
                                    x * z - y * w_, y * z + x * w_, 1 - x * x - y * y], -1).reshape(*q.shape[:-1], 3, 3)

            def stats(e):
                m = e.mean(-1)
                return torch.stack([m, (e - m[:, None]).square().mean(-1).sqrt(), e.square().mean(-1).sqrt()], -1)

            def torch_traj(est, ref):                               # [L, T, 7] fp64 each -> [L, 12]
                x, y = est[..., :3], ref[..., :3]
                mx, my = x.mean(1, keepdim=True), y.mean(1, keepdim=True)
                cov = torch.einsum("lni,lnj->lij", y - my, x - mx) / x.shape[1]
                U, d, Vh = torch.linalg.svd(cov)
                s = torch.ones_like(d)
                s[:, 2] = torch.where(torch.linalg.det(U) * torch.linalg.det(Vh) < 0, -1.0, 1.0)
                R = (U * s[:, None, :]) @ Vh
                t = my[:, 0] - torch.einsum("lij,lj->li", R, mx[:, 0])
                ate = (torch.einsum("lij,lnj->lni", R, x) + t[:, None] - y).norm(dim=-1)
                Rp, Rq = quat_R(est[..., 3:]), quat_R(ref[..., 3:])
                dRp, dRq = Rp[:, :-1].transpose(-1, -2) @ Rp[:, 1:], Rq[:, :-1].transpose(-1, -2) @ Rq[:, 1:]
                dtp = torch.einsum("lnji,lnj->lni", Rp[:, :-1], x[:, 1:] - x[:, :-1])
                dtq = torch.einsum("lnji,lnj->lni", Rq[:, :-1], y[:, 1:] - y[:, :-1])
                E = dRq.transpose(-1, -2) @ dRp
                et = torch.einsum("lnji,lnj->lni", dRq, dtp - dtq)
                v = 0.5 * torch.stack([E[..., 2, 1] - E[..., 1, 2], E[..., 0, 2] - E[..., 2, 0], E[..., 1, 0] - E[..., 0, 1]], -1)
                roe = torch.rad2deg(torch.atan2(v.norm(dim=-1), 0.5 * (E.diagonal(dim1=-2, dim2=-1).sum(-1) - 1)))
                rpe = ((E - torch.eye(3, dtype=E.dtype, device=E.device)).square().sum((-1, -2)) + et.square().sum(-1)).sqrt()
                return torch.cat([stats(ate), stats(et.norm(dim=-1)), stats(roe), stats(rpe)], -1)

            for lanes, T in ((1, 1360), (32, 4096)):
                g = torch.Generator().manual_seed(4)
                pos = torch.cumsum(torch.randn(lanes, T, 3, generator=g, dtype=torch.float64) * 0.3, 1)
                quat = torch.cumsum(torch.randn(lanes, T, 4, generator=g, dtype=torch.float64) * 0.01, 1) + torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)
                ref = torch.cat([pos, quat / quat.norm(dim=-1, keepdim=True)], -1)
                qe = ref[..., 3:] + torch.randn(lanes, T, 4, generator=g, dtype=torch.float64) * 1e-3
                est = torch.cat([pos + torch.cumsum(torch.randn(lanes, T, 3, generator=g, dtype=torch.float64) * 0.004, 1), qe / qe.norm(dim=-1, keepdim=True)], -1)
                est, ref = est.to(dev), ref.to(dev)
                legs = [("eval_traj HIP", lambda: ops.eval_trajectory(est, ref)), ("eval_traj torch closed form", lambda: torch_traj(est, ref))]
                h, t_ = legs[0][1]().rows[:, :12], legs[1][1]()
                torch.cuda.synchronize()
                print(f"lanes {lanes}: max |HIP - torch| / |torch| over the 12 statistics: {float(((h - t_).abs() / t_.abs()).max()):.3e}")
                rounds, per = 5, max(8, (4 * a.iters) // 5)
                res = {k: [] for k, _ in legs}
                for k, fn in legs:
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                for _ in range(rounds):
                    for k, fn in legs:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(per):
                            fn()
                        e1.record()
                        torch.cuda.synchronize()
                        res[k].append(e0.elapsed_time(e1) * 1e3 / per)
                for k, _ in legs:
                    v = res[k]
                    print(f"{k:30s} lanes {lanes:2d} x {T} poses: median {statistics.median(v):9.1f} us / call (rounds {min(v):.1f} .. {max(v):.1f}; {rounds * per} calls)")
                t0 = time.perf_counter()
                eh, rh = est.cpu().numpy(), ref.cpu().numpy()       # the read-back the host route needs
                rows = [TR.stats_row(TR.evaluate(eh[l], rh[l])) for l in range(lanes)]
                host_us = (time.perf_counter() - t0) * 1e6
                worst = max(abs(a_ - b_) / abs(b_) for l in range(lanes) for a_, b_ in zip(h[l].tolist(), rows[l]))
                hm, tm = statistics.median(res["eval_traj HIP"]), statistics.median(res["eval_traj torch closed form"])
                print(f"{'eval_traj numpy restatement':30s} lanes {lanes:2d} x {T} poses: {host_us:9.0f} us (one call, read-back included); max |HIP - numpy| / |numpy| = {worst:.3e}")
                print(f"eval_traj lanes {lanes}: torch / HIP = {tm / hm:.2f}x, numpy / HIP = {host_us / hm:.0f}x; one launch, {lanes * T * 7 * 16 / 1e6:.2f} MB of poses")
        elif w == "traj_assoc":
            # ops.associate_trajectory (csrc/traj_assoc.hip: interpolate_pose, one query per thread, the lane in blockIdx.y) next to the same placement in
            # torch on the same device: searchsorted + the batched quaternion / se3 operations of oracle/se3.py, one lane after the other (the lanes'
            # lengths differ in general).  Sources are 10 x denser than the queries; same method as the eval_traj leg.
            from oracle import se3

            def torch_assoc(src, ts, tq):                           # per lane [T, 7], [T], [Q] fp64 -> [Q, 7]
                out = []
                for P, t, q in zip(src, ts, tq):
                    t, q = t - t[0], q - q[0]
                    e = torch.searchsorted(t, q, right=False).clamp(1, t.shape[0] - 1)
                    s = e - 1
                    prop = ((q - t[s]) / (t[e] - t[s])).unsqueeze(-1)
                    Ps, Pe = P[s], P[e]
                    r = se3.se3_mul(se3.se3_exp(prop * se3.se3_log(se3.se3_mul(Pe, se3.se3_inv(Ps)))), Ps)
                    r = torch.where((q <= t[0]).unsqueeze(-1), P[0], torch.where((q >= t[-1]).unsqueeze(-1), P[-1], r))
                    out.append(r)
                return out

            for lanes, Q in ((1, 1360), (32, 4096)):
                T = 10 * Q
                g = torch.Generator().manual_seed(5)
                pos = torch.cumsum(torch.randn(lanes, T, 3, generator=g, dtype=torch.float64) * 0.03, 1)
                quat = torch.cumsum(torch.randn(lanes, T, 4, generator=g, dtype=torch.float64) * 0.001, 1) + torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)
                src = list(torch.cat([pos, quat / quat.norm(dim=-1, keepdim=True)], -1).to(dev).unbind(0))
                ts = list((torch.cumsum(torch.rand(lanes, T, generator=g, dtype=torch.float64) * 0.01 + 0.005, 1) + 50.0).to(dev).unbind(0))
                tq = [t[0] - 0.02 + (t[-1] - t[0] + 0.04) * torch.rand(Q, generator=g, dtype=torch.float64).to(dev) for t in ts]
                legs = [("traj_assoc HIP", lambda: ops.associate_trajectory(src, ts, tq).poses), ("traj_assoc torch searchsorted", lambda: torch_assoc(src, ts, tq))]
                h, t_ = legs[0][1](), legs[1][1]()
                torch.cuda.synchronize()
                worst = max(float((a_ - b_).abs().max()) for a_, b_ in zip(h, t_))
                print(f"lanes {lanes}: max |HIP - torch| over the poses: {worst:.3e}")
                rounds, per = 5, max(8, (4 * a.iters) // 5)
                res = {k: [] for k, _ in legs}
                for k, fn in legs:
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                for _ in range(rounds):
                    for k, fn in legs:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(per):
                            fn()
                        e1.record()
                        torch.cuda.synchronize()
                        res[k].append(e0.elapsed_time(e1) * 1e3 / per)
                for k, _ in legs:
                    v = res[k]
                    print(f"{k:30s} lanes {lanes:2d} x {Q} queries over {T} poses: median {statistics.median(v):9.1f} us / call (rounds {min(v):.1f} .. {max(v):.1f}; "
                          f"{rounds * per} calls)")
                hm, tm = statistics.median(res["traj_assoc HIP"]), statistics.median(res["traj_assoc torch searchsorted"])
                print(f"traj_assoc lanes {lanes}: torch / HIP = {tm / hm:.2f}x; one launch, every workgroup of a lane repeats the lane's checks "
                      f"({lanes * T * 64 / 1e6:.2f} MB of source rows and stamps)")
        elif w in ("remap", "rectify_maps"):
            # stereo rectification at EuRoC size (csrc/remap.hip): two cameras, 480 x 752 x 3.  `remap`: uint8 HWC -> fp32 planar, 1 lane and 32 lanes, next to
            # torch's grid_sample on the same frames (bilinear, zeros padding, align_corners: float arithmetic on float images, so a yardstick only — it also
            # needs the uint8 -> float conversion and the HWC -> planar permute the kernel does on the fly, timed with it).  `rectify_maps`: both cameras' maps.
            # Back-to-back launches in alternating rounds (the spread over the rounds is the run-to-run spread).  Algorithmic bytes: the maps at 8 B per output
            # pixel, the source at C B, the destination at C (uint8) or 4 C (fp32) B.
            import torch.nn.functional as F

            from tests import rectify_ref as RR

            eh, ew, ec = 480, 752, 3
            plan = ops.stereo_rectify_plan(*RR.euroc_rig())
            mx, my = ops.rectify_maps(plan, device=dev)
            if w == "rectify_maps":
                rounds, per, res = 5, max(8, (4 * a.iters) // 5), []
                for _ in range(5):
                    ops.rectify_maps(plan, device=dev)
                torch.cuda.synchronize()
                for _ in range(rounds):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(per):
                        ops.rectify_maps(plan, device=dev)
                    e1.record()
                    torch.cuda.synchronize()
                    res.append(e0.elapsed_time(e1) * 1e3 / per)
                nb = 2 * eh * ew * 8
                med = statistics.median(res)
                print(f"rectify_maps 2 x {eh}x{ew}: median {med:8.2f} us / call, allocation of the two maps included (rounds {min(res):.2f} .. {max(res):.2f}; "
                      f"{rounds * per} calls); {nb / 1e6:.2f} MB written = {nb / med / 1e3:.0f} GB/s = {nb / med / 1e3 / 8000 * 100:.2f}% of HBM peak (fp64 arithmetic, once per sequence)")
                continue
            maps = [(mx[0], my[0]), (mx[1], my[1])]
            # grid_sample's grid: align_corners=True maps [-1, 1] onto pixel centres 0 .. size - 1
            grids = [torch.stack([m[0] * (2.0 / (ew - 1)) - 1.0, m[1] * (2.0 / (eh - 1)) - 1.0], -1) for m in maps]
            for lanes in (1, 32):
                imgs = [torch.randint(0, 256, (lanes, eh, ew, ec), dtype=torch.uint8, generator=g).to(dev) for _ in range(2)]
                outs = [torch.empty((lanes, ec, eh, ew), dtype=torch.float32, device=dev) for _ in range(2)]
                gexp = [gr[None].expand(lanes, eh, ew, 2) for gr in grids]

                def torch_leg():
                    return [F.grid_sample(im.permute(0, 3, 1, 2).float() / 255, gr, mode="bilinear", padding_mode="zeros", align_corners=True)
                            for im, gr in zip(imgs, gexp)]

                legs = [("remap HIP u8 -> fp32", lambda: ops.remap(imgs, maps, dtype=torch.float32, out=outs)),
                        ("remap HIP u8 -> u8", lambda: ops.remap(imgs, maps, dtype=torch.uint8)),
                        ("torch grid_sample (float)", torch_leg)]
                hh, tt = legs[0][1](), legs[2][1]()
                torch.cuda.synchronize()
                print(f"lanes {lanes}: max |HIP - grid_sample| = {max(float((x - y).abs().max()) for x, y in zip(hh, tt)):.3e} (1/32-pixel fixed point against float weights)")
                rounds, per = 5, max(8, (4 * a.iters) // 5)
                res = {k: [] for k, _ in legs}
                for k, fn in legs:
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                for _ in range(rounds):
                    for k, fn in legs:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(per):
                            fn()
                        e1.record()
                        torch.cuda.synchronize()
                        res[k].append(e0.elapsed_time(e1) * 1e3 / per)
                px = 2 * eh * ew
                # per output pixel of every lane: 8 B of maps, C B of source, C or 4 C B of destination; `once`: the shared map counted once per launch instead
                nbytes = {"remap HIP u8 -> fp32": lanes * px * (8 + ec * (1 + 4)), "remap HIP u8 -> u8": lanes * px * (8 + ec * (1 + 1))}
                for k, _ in legs:
                    v = res[k]
                    med = statistics.median(v)
                    tail = ""
                    if k in nbytes:
                        once = nbytes[k] - (lanes - 1) * px * 8
                        tail = (f"; {nbytes[k] / 1e6:.1f} MB algorithmic = {nbytes[k] / med / 1e3:.0f} GB/s = {nbytes[k] / med / 1e3 / 8000 * 100:.1f}% of HBM peak "
                                f"(shared maps counted once: {once / 1e6:.1f} MB = {once / med / 1e3 / 8000 * 100:.1f}%)")
                    print(f"{k:28s} 2 x {eh}x{ew}x{ec} lanes {lanes:2d}: median {med:9.2f} us / call (rounds {min(v):.2f} .. {max(v):.2f}; {rounds * per} calls){tail}")
                print(f"remap lanes {lanes}: grid_sample / HIP = {statistics.median(res['torch grid_sample (float)']) / statistics.median(res['remap HIP u8 -> fp32']):.2f}x; one launch")
        elif w == "grad_select":
            # GradientSelector / SparseGradienSelector (csrc/kp_gradient.hip) at 480 x 640, 1 lane and 32 lanes, 200 keypoints per lane: the dense part alone,
            # dense part + device finish (device-resident generators: nothing reaches the host inside the timed loop), and the same restatement run eagerly by
            # torch on the same GPU, lane by lane, with `randperm` on the CPU as the reference has it (one host read of the count per lane).  Back-to-back calls
            # in alternating rounds (the spread over the rounds is the run-to-run spread).  Algorithmic bytes per lane: three planes in, `grad` out and back.
            import torch.nn.functional as F

            from tests import grad_selectors_ref as GR

            gh, gw, k_pts, m_w, g_std = 480, 640, 200, 32, 1.0
            lap = torch.tensor(GR.LAPLACIAN).float().expand((1, 3, 3, 3)).to(dev)

            def torch_select(images, nms):
                out = []
                for l in range(images.shape[0]):
                    grad = F.conv2d(images[l:l + 1], lap, padding=1)[0].abs()
                    points = grad > (grad.mean(dim=(1, 2), keepdim=True) + g_std * grad.std(dim=(1, 2), keepdim=True))
                    border = torch.zeros_like(points)
                    border[..., m_w:-m_w, m_w:-m_w] = 1.0
                    points = points * border
                    if nms:
                        points = points * (grad == F.max_pool2d(grad, kernel_size=nms, stride=1, padding=nms // 2))
                    sel = torch.nonzero(points, as_tuple=False)
                    perm = torch.randperm(sel.shape[0])[:k_pts]
                    out.append(sel[perm.to(dev)][..., 1:].roll(shifts=1, dims=1))
                return out

            for lanes in (1, 32):
                images = torch.stack([GR.quantised_image(gh, gw, 40 + l) for l in range(lanes)]).to(dev)
                state = ops.mt19937_state(list(range(lanes)), dev)
                for name, nms in (("GradientSelector", None), ("SparseGradienSelector nms 7", 7)):
                    legs = [("HIP dense part", lambda: ops.kp_gradient(images, m_w, g_std, nms)),
                            ("HIP dense + device finish", lambda: ops.kp_gradient(images, m_w, g_std, nms).finish_device(k_pts, state)),
                            ("torch eager + CPU randperm", lambda: torch_select(images, nms))]
                    cand = legs[0][1]()
                    n_hip = cand.count[:, 0].tolist()
                    n_torch = [int(GR.candidates(images[l].cpu(), m_w, g_std, nms).numel()) for l in range(min(lanes, 2))]
                    print(f"{name}, lanes {lanes}: candidates of lane 0 {n_hip[0]} (torch on the CPU: {n_torch[0]}; images are 1/256-valued: equal counts expected)")
                    rounds, per = 5, max(8, (4 * a.iters) // 5)
                    res = {kk: [] for kk, _ in legs}
                    for kk, fn in legs:
                        for _ in range(5):
                            fn()
                    torch.cuda.synchronize()
                    for _ in range(rounds):
                        for kk, fn in legs:
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(per):
                                fn()
                            e1.record()
                            torch.cuda.synchronize()
                            res[kk].append(e0.elapsed_time(e1) * 1e3 / per)
                    nbytes = lanes * gh * gw * 4 * 5
                    for kk, _ in legs:
                        v = res[kk]
                        med = statistics.median(v)
                        tail = "" if kk.startswith("torch") else f"; {nbytes / 1e6:.1f} MB algorithmic = {nbytes / med / 1e3:.0f} GB/s = {nbytes / med / 1e3 / 8000 * 100:.1f}% of HBM peak"
                        print(f"{kk:28s} {name:28s} {gh}x{gw} lanes {lanes:2d}: median {med:9.2f} us / call (rounds {min(v):.2f} .. {max(v):.2f}; {rounds * per} calls){tail}")
                    print(f"grad_select {name}, lanes {lanes}: torch eager / HIP with finish = "
                          f"{statistics.median(res['torch eager + CPU randperm']) / statistics.median(res['HIP dense + device finish']):.2f}x")
        elif w == "select":
            fc = synth.flow_cov_maps(H, W, 2).to(dev)
            d0, d0c = [t.to(dev) for t in synth.depth_maps(H, W, 3)]
            d1, d1c = [t.to(dev) for t in synth.depth_maps(H, W, 4)]
            med, mn = timeit(lambda: ops.kp_select("nodepth", H, W, flow_cov=fc, kernel_size=7, mask_width=32, max_match_cov=100.0), a.iters)
            print(f"kp_select nodepth    {med:8.1f} us (min {mn:.1f})")
            med, mn = timeit(lambda: ops.kp_select("full", H, W, flow_cov=fc, depth0=d0, depth0_cov=d0c, depth1=d1, depth1_cov=d1c,
                                                   kernel_size=7, mask_width=32, max_depth=80.0, max_depth_cov=250.0, max_match_cov=100.0), a.iters)
            print(f"kp_select full       {med:8.1f} us (min {mn:.1f})")
            med, mn = timeit(lambda: ops.kp_select("mapping", H, W, depth0=d0, depth0_cov=d0c, mask_width=32, max_depth=20.0, max_depth_cov=0.2), a.iters)
            print(f"kp_select mapping    {med:8.1f} us (min {mn:.1f})")
        elif w == "cov":
            depth = synth.depth_maps(H, W, 3)[0].to(dev)
            for npt in (200, 2000):
                kp = synth.keypoints(npt, H, W, 5).float().to(dev)
                fc = (torch.ones(npt, 3) * 0.25).to(dev)
                med, mn = timeit(lambda: ops.match_cov(depth, kp, fc, None, 320.0, 320.0, 320.0, 240.0), a.iters)
                print(f"match_cov N={npt:5d}    {med:8.1f} us (min {mn:.1f})")
        elif w == "pgo":
            from tools.synth import pgo_batch as _to_batch, pgo_problem

            for nprob in (1, 8, 256, 4096):
                base = [pgo_problem(n=200, seed=6 + k)[0] for k in range(min(nprob, 8))]
                probs = [base[k % len(base)] for k in range(nprob)]
                batch = _to_batch(probs, dev)
                for gt in ("disp", "icp"):
                    med, mn = timeit(lambda: ops.pgo_solve(batch, gt), max(5, a.iters // 5))
                    print(f"pgo {gt:6s} nprob={nprob:5d} {med:9.1f} us (min {mn:.1f})  {nprob / med * 1e6:10.0f} solves/s")


if __name__ == "__main__":
    main()
