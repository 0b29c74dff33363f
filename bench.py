#!/usr/bin/env python
"""bench.py — stereo frames/sec of the MAC-VO hot path on MI355X (contract: see the task statement / DESIGN.md §Measurement).

One "step" = one ``run_pair`` of the hot path over one batch of ``--lanes`` 640x480 stereo frames (default 1 =
BASELINE.json configs[1], the 1-sequence stream; 32 = configs[4], batch-32 frames per GPU):
  all-pairs cost volumes (stereo + temporal pair of every lane in ONE launch) + 12 x 9x9 window lookups + frontend
  epilogue + covariance-aware keypoint selection (200 pts / frame, host randperm) + tracking gathers + 2 x covariance
  model + observation filter + covariance-weighted two-frame PGO (LM, <= 10 steps), all in hand-written HIP kernels
  behind the C ABI, inputs (feature maps, lookup coordinates, network flow / log-sigma) already resident in HBM.
The learned FlowFormer layers are not part of the step (their source and weights are absent from the reference).

N > 1: one process per GPU (torch.distributed / RCCL), each rank owns independent sequence(s) (weak scaling);
the only collective is one all_gather of the per-frame poses (+ timestamps + track lengths) at the end of the timed region.

A plain run (``--gpus 1 --steps N --warmup W``) sets up, warms up, times the N steps and prints the line: metric, value, unit,
higher_is_better, dtype, ms_per_step, the host figures of the timed pass and the configuration.  ``--dump-outputs DIR`` also writes
what the last timed step computed (poses, solver info, keypoints, lookup tokens) as DIR/<name>.npy.  Everything else is measured only
with ``--full``, which fills these fields of the line (null without it):
  roofline      dominant kernel (cost-volume GEMM): algorithmic FLOPs / HIP-event launch time, measured on its stream
  cpu_baseline  oracle/pipeline.py (torch-CPU ops shaped like the reference) on a bounded sample, N = 1 only
  parity        free-running HIP track vs the oracle's on the same frames: keypoints, per-frame pose diff, RTE
                (Evaluation/MetricsSeq.py:9-16 formula); rte_vs_oracle is BASELINE.json's "pose RTE vs reference"
  config4       a short second measurement at BASELINE configs[4] (32 lanes, B = 64 pairs per GEMM), N = 1 only
  decoder_loop  the HIP lookups / upsamplings interleaved with the PyTorch-ROCm kernels of a stand-in decoder network
                (tools/decoder_harness.py, loop structure of covhead.py:85-135) next to the back-to-back figure, N = 1 only
  end_to_end    images -> poses through the reference's own MACVO loop with a FlowFormerCov-shaped network (random weights, PyTorch-ROCm) as
                the learned frontend and the HIP plugins behind it, hooked vs unhooked (tools/end_to_end.py in a fresh interpreter), N = 1 only
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

# MI355X peaks (/opt/skills/guides/MI355X_MICROARCH.md §Chip-level parameters)
PEAK_F32_MFMA_TFLOPS = 157.3
PEAK_BF16_MFMA_TFLOPS = 2500.0
PEAK_HBM_GBS = 8000.0
MIN_TIMED_LAUNCHES = 200       # the roofline average is taken over at least this many GEMM launches
RAMP_SECONDS = 1.5             # untimed sustained load before the contract's warm-up: clocks ramp, queues are created
DUMP_BUDGET_BYTES = 64 * 10 ** 6   # --dump-outputs: all files together


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--lanes", "--batch-frames", dest="lanes", type=int, default=1,
                    help="independent sequences advanced per step on each GPU (1 = configs[1]; 32 = configs[4], batch-32 frames)")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--feat-dtype", choices=["f32", "f16", "bf16"], default="f32")
    ap.add_argument("--layout", choices=["chw", "hwc"], default="chw")
    ap.add_argument("--volume-precision", choices=["f16x2", "bf16x3", "exact", "split3", "split2"], default=None,
                    help="fp32 features: 'f16x2' (default) = rows scaled by a power of two into fp16's range, two fp16 pieces, three "
                         "products on the 16-bit matrix pipe, fp32 accumulate, scales undone exactly; 'bf16x3' = three bf16 pieces, six "
                         "products — both meet the parity bar of 'exact', not bitwise (the reference runs this GEMM in TF32, "
                         "Frontend.py:275-277); 'exact' = fp32 MFMA (bitwise fmaf chain).  The other two are reported as `other_precisions` "
                         "beside the default line; split3 / split2 = round-1 tile kernels (need --layout hwc)")
    ap.add_argument("--volume-store", choices=["fp32", "encoder"], default="fp32",
                    help="16-bit features (--feat-dtype f16 --layout hwc): 'encoder' stores the volume in fp16 with one rounding in the GEMM epilogue, as the "
                         "reference's Fast mode computes it (einsum of fp16 maps; flownet.py:26-27), and the lookups read the 2-byte cells")
    ap.add_argument("--exact-steps", type=int, default=60, help="steps of the extra legs with the other volume precisions beside the default line; 0 = skip")
    ap.add_argument("--graph", choices=["disp", "reproj", "icp"], default="disp")
    ap.add_argument("--pool", type=int, default=24, help="distinct synthetic frames (closed trajectory) kept in HBM")
    ap.add_argument("--feat-pool", type=int, default=0, help="distinct feature-map / lookup-coordinate sets among the resident frames "
                    "(0 = one per frame: every frame reads its own 19.7 MB of features; rounds 1-3 cycled two sets)")
    ap.add_argument("--cpu-frames", type=int, default=120, help="frames timed for the CPU baseline (rank 0, N=1 only)")
    ap.add_argument("--reference-frames", type=int, default=12, help="frames run through the reference's own MACVO loop on the host (parity + cpu_baseline kind "
                    "'reference'); needs oracle/_ref/pyref (python oracle/build_ref.py in the build container); 0 = skip")
    ap.add_argument("--parity-frames", type=int, default=48, help="free-running frames compared with the oracle (N=1 only)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU baseline and the parity leg")
    ap.add_argument("--config4-steps", type=int, default=100, help="steps of the extra configs[4] leg (32 lanes); 0 = skip")
    ap.add_argument("--fast-mode-steps", type=int, default=200, help="steps of the extra Fast-mode leg (fp16 features, fp16-stored tiled volume: one lane, then 32 lanes for a fifth of them); 0 = skip")
    ap.add_argument("--graphs", action="store_true", help="replay the decoder-side segment (12 lookups + epilogue + selector) as a hipGraph (measured slower than eager launches on ROCm 7.2: 2.46 k vs 2.60 k fps)")
    ap.add_argument("--driver", choices=["native", "python"], default="native",
                    help="host-side frame sequencing: the C++ driver (mv_frame_pipe_*) or the Python loop over the per-op entry points")
    ap.add_argument("--no-kernel-events", action="store_true", help="skip per-launch HIP events around the volume kernel")
    ap.add_argument("--no-ramp", action="store_true", help="skip the untimed clock-ramp phase")
    ap.add_argument("--end-to-end-frames", type=int, default=40, help="frames of the end_to_end leg (network included, reference's MACVO loop; the first "
                    "quarter is warm-up); 0 = skip")
    ap.add_argument("--plugin-frames", type=int, default=12, help="distinct frames handed to the plugin_path leg (replayed 3 x through the reference's MACVO loop with "
                    "the HIP plugins); 0 = skip")
    ap.add_argument("--no-decoder-leg", action="store_true", help="skip the decoder-loop harness leg (HIP lookups / upsamplings interleaved with PyTorch-ROCm kernels)")
    ap.add_argument("--host-randperm", action="store_true", help="one lane: draw the keypoint permutations with torch.randperm on the Python side (global CPU generator) "
                    "instead of the driver's native MT19937 + partial Fisher-Yates (bit-identical draws)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="TEST ONLY (N > 1 ranks on a 1-GPU box): every rank drives device 0 and the collectives run over gloo — real kernels, real gather_tracks, real "
                         "core pinning, no RCCL; the line is marked and its value is not a scaling measurement")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline, also measure and check everything else: HIP events around the volume GEMM (roofline, timeline), the other "
                         "volume precisions, CPU baseline + parity, Fast-mode, configs[4], decoder-loop, patch-embedding, per-kernel, plugin-path and "
                         "end-to-end legs (each still switchable by its own option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step as DIR/<name>.npy (float32 / float64, at most 64 MB in all)")
    ap.add_argument("--dry-collectives", action="store_true",
                    help="CPU-only plumbing check of the N-rank launch path: gloo backend, no kernels, synthetic tracks through the "
                         "same barrier / gather_tracks / max-over-ranks code; the line it prints is marked and is NOT a measurement")
    return ap.parse_args()


def self_launch(args) -> int:
    """``python bench.py --gpus N`` without a launcher (the form the round-end driver uses): re-exec this script under
    ``torch.distributed.run`` with one rank per GPU on 127.0.0.1 and hand its output (rank 0's one JSON line) through."""
    import socket
    import subprocess

    with socket.socket() as so:           # a free rendezvous port
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL across processes needs it on this stack
    # each rank runs two busy host threads (the caller and the driver's backend launch thread) plus torch's intra-op pool: give every
    # rank its own slice of the cores this process may use instead of 8 pool threads each on a small host
    ncores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    env.setdefault("OMP_NUM_THREADS", str(max(1, min(8, ncores // max(1, args.gpus) - 2))))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def dry_collectives(args, rank, world) -> None:
    """The N-rank control flow of ``main`` on CPU tensors over gloo: rendezvous, barrier, one gather_tracks of ragged tracks,
    max-over-ranks clock.  Exists so that the launch path of ``--gpus N`` is testable without N GPUs (tests/test_abi_and_host.py)."""
    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(backend="gloo")
    from macvo_amd.distributed import gather_tracks

    steps = args.steps
    poses = torch.zeros((steps, 7))
    poses[:, 6] = 1.0
    poses[:, 0] = rank
    stamps = torch.arange(steps, dtype=torch.int64) * 33_333_333
    dist.barrier()
    t0 = time.perf_counter()
    all_poses, all_stamps, lengths = gather_tracks(poses, stamps, dist)
    dist.barrier()
    tmax = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    ids = [None] * world
    dist.all_gather_object(ids, {"rank": rank, "local_rank": int(os.environ.get("LOCAL_RANK", "0"))})
    ok = all_poses.shape[0] == world and all(float(all_poses[r, 0, 0]) == r for r in range(world))
    if rank == 0:
        print(json.dumps({"metric": "DRY RUN of the multi-rank launch path (gloo, CPU, no kernels) - not a measurement",
                          "value": None, "unit": "stereo frames/s", "n_gpus": world, "steps": steps, "warmup": args.warmup,
                          "dry_collectives": True, "ranks_seen": dist.get_world_size(), "rank_ids": ids, "gather_ok": bool(ok),
                          "track_lengths": [int(x) for x in lengths]}), flush=True)
    dist.destroy_process_group()


def last_step_outputs(res, hot) -> dict:
    """What a caller of the timed path holds after its last step (``res``: that step's result, a list of them for lanes > 1): per lane
    the optimised pose (fp32 and fp64), the LM solve's {loss, steps, rejects, loss0}, the surviving observation count and the selected
    keypoints (concatenated in lane order; ``n_selected`` splits them), and the window-lookup tokens of the step's last decoder iteration."""
    import numpy as np

    lanes = res if isinstance(res, list) else [res]

    def f64(t, n):
        return np.full(n, np.nan) if t is None else t.detach().double().cpu().numpy().reshape(n)

    kps = [np.zeros((0, 2)) if r.kp0_uv is None else r.kp0_uv.cpu().double().numpy().reshape(-1, 2) for r in lanes]
    out = {"pose": np.stack([r.pose.detach().float().cpu().numpy().reshape(7) for r in lanes]),
           "pose_f64": np.stack([f64(r.pose_f64, 7) for r in lanes]),
           "solver_info": np.stack([f64(r.info, 4) for r in lanes]),
           "n_valid": np.concatenate([f64(r.n_valid, 1) for r in lanes]),
           "n_selected": np.array([float(len(k)) for k in kps]),
           "keypoints_uv": np.concatenate(kps)}
    if hot.last_tokens is not None:
        out["lookup_tokens"] = hot.last_tokens.float().cpu().numpy()
    return out


def write_outputs(out_dir: str, arrays: dict, budget: int = DUMP_BUDGET_BYTES) -> None:
    """``out_dir/<name>.npy`` per array: float32 stays float32, everything else becomes float64.  Smallest first, each may take an equal
    share of what is left of ``budget``; an array larger than its share is replaced by a fixed sample of its flattened elements (the same
    seeded indices in every run, so two runs stay comparable element for element)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    items = sorted(arrays.items(), key=lambda kv: kv[1].nbytes)
    left = budget
    for i, (name, a) in enumerate(items):
        a = np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64)
        cap = max(left - 128 * (len(items) - i), 0) // (len(items) - i) // a.itemsize      # (128 bytes: the .npy header)
        if a.size > cap:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, cap, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)
        left -= a.nbytes + 128


def volume_work(lanes, n_q, C, esz, osz=4):
    """Algorithmic work of one cost-volume launch: 2*N^2*C FLOP and 2*N*C*s + 4*N^2 bytes per pair (osz = 2: the Fast-mode
    volume stored in the encoder's 16-bit type, what the reference's fp16 einsum writes)."""
    pairs = 2 * lanes
    return pairs * 2.0 * n_q * n_q * C, pairs * (2.0 * n_q * C * esz + float(osz) * n_q * n_q)


def roofline_of(ms, args, lanes, n_q, C, timed_region_launches, traffic=None):
    enc16 = args.feat_dtype == "f16" and getattr(args, "volume_store", "fp32") == "encoder" and args.layout == "hwc" and C in (128, 256)
    flops, nbytes = volume_work(lanes, n_q, C, 4 if args.feat_dtype == "f32" else 2, 2 if enc16 else 4)
    avg_s = sum(ms) / len(ms) / 1e3
    srt = sorted(ms)
    common = {"avg_launch_us": round(avg_s * 1e6, 2), "median_launch_us": round(srt[len(srt) // 2] * 1e3, 2), "min_launch_us": round(srt[0] * 1e3, 2),
              "launch_time_note": "HIP-event pair on the GEMM's stream inside the running pipe: the mean (what `achieved` / `frac` use) includes the launches whose "
                                  "workgroups waited for CUs held by the other streams' kernels; rocprofv3's kernel duration for the same command is the committed "
                                  "profiles/r06_bench_kernel_stats.csv (r05c_* for round 5)",
              "launches": len(ms), "launches_in_timed_region": timed_region_launches,
              "algorithmic_flops_per_launch": flops, "algorithmic_bytes_per_launch": nbytes}
    prec = getattr(args, "_precision", args.volume_precision)
    if args.feat_dtype == "f32" and prec in ("f16x2", "bf16x3", "split3", "split2"):
        nprod = 3.0 if prec in ("split2", "f16x2") else 6.0
        ach = nprod * flops / avg_s / 1e12          # 16-bit MFMA FLOPs the kernel executes: `nprod` piece products per algorithmic product
        return {"bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s",
                "frac": round(ach / PEAK_BF16_MFMA_TFLOPS, 4), "traffic": traffic,
                "kernel": f"corr_volume_split_stream<{prec}>" if prec in ("bf16x3", "f16x2") else f"{prec} pre-pass + corr_volume_bf16x3_hwc<{int(nprod) // 3 + 1}>",
                "hbm_write_GBps": round(nbytes / avg_s / 1e9, 1),
                **common, "executed_flops_per_launch": nprod * flops, "algorithmic_tflops": round(flops / avg_s / 1e12, 2),
                "frac_algorithmic": round(flops / avg_s / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4),
                "algorithmic_vs_fp32_mfma_peak": round(flops / avg_s / 1e12 / PEAK_F32_MFMA_TFLOPS, 4),
                "frac_note": "frac = EXECUTED 16-bit FLOPs (3 or 6 piece products per fp32 product) / time / peak; frac_algorithmic = SURVEY 8(d)'s algorithmic "
                             "2 N^2 C B FLOPs / time / the same 2.5 PFLOP/s peak — the figure the round-5 review recomputed (0.10-0.12)",
                "note": f"achieved = {int(nprod)} 16-bit piece products per algorithmic fp32 product x algorithmic FLOPs / time, against the dense 16-bit "
                        "MFMA peak (2.5 PFLOP/s; with N(0,1) operands the chip's power limit holds a bare v_mfma_f32_32x32x16_bf16 stream at "
                        "~1.89 PFLOP/s = 0.76, profiles/probes/mfma16_probe.*; this kernel runs 1.3x faster on all-zero operands with identical cycle "
                        "counters = the clock, and inside its cycles the matrix pipe is busy 46 % (f16x2) / 63 % (bf16x3), "
                        "profiles/r03_split_wait_counters.log); algorithmic_vs_fp32_mfma_peak = algorithmic fp32 FLOPs / time against the 157.3 TFLOP/s "
                        "fp32-MFMA peak that bounds ANY exact-fp32 form of this GEMM (> 1 = beyond that roofline); the operand pack is a "
                        "separate launch in front of the GEMM and is not in this time"}
    if args.feat_dtype == "f32":
        ach = flops / avg_s / 1e12
        return {"bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                "frac": round(ach / PEAK_F32_MFMA_TFLOPS, 4), "traffic": traffic,
                "kernel": "corr_volume_f32_mixed_dma" if args.layout == "chw" else "corr_volume_f32_hwc", **common}
    ach = nbytes / avg_s / 1e9
    return {"bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(ach / PEAK_HBM_GBS, 4),
            "traffic": traffic, "kernel": ("corr_volume_h_stream<out16>" if enc16 else "corr_volume_h_stream") if (args.layout == "hwc" and C in (128, 256)) else "corr_volume_h_" + args.layout,
            **common}



def volume_lookup_parity(ops, frames, cfr, args, n_q, C, dev, picks, make_pipe):
    """The parity of the kernels the line TIMES, on the benchmark's own frames, at the line's precision, READ FROM THE BUFFERS THE TIMED PIPE WRITES
    (a fresh pipe of the line's configuration advances to the picked frame; its volume buffer ``MV_FB_VOLUME`` and its last token
    buffer are what the GEMM / lookup kernels inside the pipe produced).  Per picked frame: 96 sampled rows of the pipe's volume against a float64
    einsum (fp32 cells: absolute bar 2e-5 sqrt(C) and the error relative to sum |a||b|; fp16 cells of ``--volume-store encoder``: one fp16 ulp of the
    cell + 2e-6 sum |a||b|, as tests/test_gpu_fastmode.py), the pipe's last-iteration tokens and the tokens of all ``iters`` window lookups run on
    that same buffer against oracle.corr.corr_lookup (= ATen grid_sample, align_corners=True, zero padding; rtol 1e-5, atol 2e-4)."""
    from oracle import corr as ocorr

    g = torch.Generator().manual_seed(99)
    enc16 = args.feat_dtype == "f16" and args.volume_store == "encoder" and args.layout == "hwc"
    out = {"frames": list(picks), "volume_precision": args.volume_precision, "volume_source": "mv_frame_pipe_buffer(MV_FB_VOLUME) of a pipe advanced to the frame",
           "volume_cell_dtype": "f16" if enc16 else "f32", "volume_rows_sampled": 0, "volume_max_abs_err": 0.0,
           "volume_abs_bar": 2e-5 * C ** 0.5, "volume_max_err_rel_sum_abs": 0.0, "lookup_launches": 0, "lookup_max_abs_err": 0.0,
           "pipe_tokens_checked": 0, "lookup_tol": "rtol 1e-5, atol 2e-4 vs oracle.corr.corr_lookup (grid_sample) on the same volume"}
    ok = vol_ok = True
    h8, w8 = args.height // 8, args.width // 8
    for k in picks:
        fr, fc = frames[k], cfr[k]
        P = fr.fmap1.shape[0]
        hot = make_pipe(1, 0)
        torch.manual_seed(7)
        hot.initialize(frames[(k - 1) % len(frames)])
        hot.step(fr)
        torch.cuda.synchronize()
        tiled = bool(getattr(hot, "volume_tiled", False))     # Fast-mode pipes keep the slices in 4 x 4-cell tiles (a padded last tile row when h8 % 4 != 0):
        hp = -(-h8 // 4) * 4 if tiled else h8                 # ... the row-major view of the same cells for the checks
        vol_pipe = hot._view("VOLUME", 0, torch.float16 if enc16 else torch.float32, (P * n_q, 1, hp, w8))
        vol = vol_pipe.view(P * n_q, hp // 4, w8 // 4, 4, 4).permute(0, 1, 3, 2, 4).reshape(P * n_q, 1, hp, w8)[:, :, :h8].contiguous() if tiled else vol_pipe
        out["volume_tiled"] = tiled
        pipe_tok = hot.last_tokens.clone()
        out["volume_kernel"] = ops.last_volume_kernel()
        f1 = fc["fmap1"].reshape(P, C, n_q).double()          # cfr is CHW fp32 on the CPU
        f2 = fc["fmap2"].reshape(P, C, n_q).double()
        rows = torch.randint(0, P * n_q, (96,), generator=g)
        got = vol.view(P * n_q, n_q)[rows.to(dev)].cpu().double()
        b, i = rows // n_q, rows % n_q
        a = f1[b, :, i]                                        # [96, C]
        ref = torch.einsum("rc,rcn->rn", a, f2[b])
        mag = torch.einsum("rc,rcn->rn", a.abs(), f2[b].abs())
        err = (got - ref).abs()
        out["volume_rows_sampled"] += int(rows.numel())
        out["volume_max_abs_err"] = max(out["volume_max_abs_err"], float(err.max()))
        out["volume_max_err_rel_sum_abs"] = max(out["volume_max_err_rel_sum_abs"], float((err / mag.clamp_min(1e-300)).max()))
        if enc16:      # one rounding to fp16 in the GEMM epilogue: half an ulp of the cell (ulp = 2^-10 |x|, 2^-24 subnormal) + the fp32 accumulation
            bar = ref.abs().clamp_min(2.0 ** -14) * 2.0 ** -11 * 1.001 + 2e-6 * mag
            vol_ok = vol_ok and bool((err <= bar).all())
        elif args.feat_dtype == "f32":
            vol_ok = vol_ok and float(err.max()) <= out["volume_abs_bar"]
        else:          # 16-bit features, fp32 cells: fp32 accumulation of exact 16-bit products
            vol_ok = vol_ok and bool((err <= 2e-6 * mag + 1e-30).all())
        volc = vol.float().cpu()
        n_it = fr.coords.shape[0]
        rlast = ocorr.corr_lookup(volc, fc["coords"][n_it - 1], 4)
        ok = ok and bool(torch.allclose(pipe_tok.cpu(), rlast, rtol=1e-5, atol=2e-4))     # the tokens the pipe's own last lookup wrote
        out["pipe_tokens_checked"] += 1
        for it in range(n_it):
            tok = ops.corr_lookup(vol_pipe, fr.coords[it], 4, tiled=tiled, image_hw=(h8, w8) if (tiled and enc16) else None).cpu()      # the same lookup kernel the pipe runs (fp16-cell / tiled form under enc16), on the pipe's buffer
            rtok = rlast if it == n_it - 1 else ocorr.corr_lookup(volc, fc["coords"][it], 4)
            out["lookup_launches"] += 1
            out["lookup_max_abs_err"] = max(out["lookup_max_abs_err"], float((tok - rtok).abs().max()))
            ok = ok and bool(torch.allclose(tok, rtok, rtol=1e-5, atol=2e-4))
        hot.close()          # (result objects keep their pipe alive: close it, do not just drop the name — pipeline.NativeHotPath.close)
        del hot, vol, vol_pipe
    out["volume_within_bar"] = bool(vol_ok)
    out["within_bar"] = bool(ok and vol_ok)
    return out


def reference_loop_leg(cam, cfr, n_frames, cores, graph):
    """The reference's OWN ``Odometry/MACVO.py`` loop with the reference's own classes (CovAwareSelector_NoDepth, MatchCovariance,
    TwoFrame_PGO, FlowFormerCovFrontend.estimate_pair + VisualMap, StaticMotionModel, ...) on this host's cores, fed the benchmark's own
    network outputs (tests/refrun.py in a fresh interpreter; the tree comes from oracle/_ref/pyref, byte-compiled from the reference).
    Returns (seconds per run_pair, per-frame kept keypoints, poses) or None when the tree is absent."""
    import subprocess
    import tempfile

    import numpy as np

    from tests import refrun

    if refrun.reference_root() is None:
        return None
    with tempfile.TemporaryDirectory() as tmp:
        mf, of = os.path.join(tmp, "maps.npz"), os.path.join(tmp, "run.npz")
        np.savez(mf, flow=torch.stack([f["flow"] for f in cfr[:n_frames]]).numpy(),
                 cov=torch.stack([torch.exp(f["logcov"] * 2) for f in cfr[:n_frames]]).numpy(), cam=np.array(json.dumps(cam)))
        cmd = [sys.executable, os.path.join(ROOT, "tests", "refrun.py"), "--mode", "ref", "--case", "synth_fast", "--maps-file", mf, "--mapping", "0",
               "--graph", graph, "--threads", str(cores), "--out", of]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            return {"error": (p.stdout[-500:] + p.stderr[-1500:])}
        r = dict(np.load(of))
    fs = r["frame_s"]
    rng = r["map/edge/frame2match/ranges"]
    kps = [r["map/match//pixel1_uv"][int(rng[t, 0, 0]): int(rng[t, 0, 0]) + int(rng[t, 0, 1])] for t in range(1, n_frames)]
    return {"s_per_run_pair": float(fs[2:].mean()), "frames": int(n_frames), "kps": kps, "poses": r["map/frames//pose"],
            "graph": graph}


def end_to_end_leg(n_frames: int):
    """tools/end_to_end.py in a fresh interpreter (the reference's tree is imported there on shims): images -> poses, learned frontend included."""
    import subprocess

    cmd = [sys.executable, os.path.join(ROOT, "tools", "end_to_end.py"), "--frames", str(n_frames), "--warmup", str(max(3, n_frames // 4))]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)      # ~25 s on an MI355X box; a hung leg must not hold the line back
    for ln in reversed(p.stdout.splitlines()):
        if ln.startswith('{"end_to_end"'):
            return json.loads(ln)["end_to_end"]
    return {"error": (p.stdout[-300:] + p.stderr[-700:])}


def schedule_note(lanes: int) -> str:
    """Which stream layout / depth the native driver runs this pipe shape with (the library's own rule, csrc/frame_pipe.hip)."""
    from macvo_amd import _lib

    depth = int(os.environ.get("MV_PIPE_DEPTH", _lib.load().mv_frame_pipe_default_depth(lanes, 0)))
    alt = lanes <= 2 and os.environ.get("MV_PIPE_LAYOUT", "alt") != "classic" and "MV_PIPE_SELECTOR_ON" not in os.environ
    dd = os.environ.get("MV_PIPE_DEVICE_DRAW", "1") != "0"
    head = ("device-driven frames (round 6): a frame's whole launch chain — lookups, selector, backend with the permutation draw inside, solve — is queued by one host "
            "thread without any wait on the GPU, the volume GEMM one frame ahead, host flow control two finished frames back; " if dd else
            f"{depth} tracked frames in flight + the volume GEMM one frame ahead (host-drawn permutations: the host waits for each frame's candidate count); ")
    return (head +
            ("four streams: GEMM | even frames' lookups + selector | odd frames' lookups + selector | backend + solve; GEMM on all but 32 CUs" if alt else
             "four streams: GEMM | lookups + selector | backend | solve" if lanes > 2 else "four streams: GEMM | lookups | selector + backend | solve"))


def _parse_cpulist(text: str) -> list:
    out = []
    for part in text.strip().split(","):
        if not part:
            continue
        lo, _, hi = part.partition("-")
        out.extend(range(int(lo), int(hi or lo) + 1))
    return out


def gpu_local_cores(index: int) -> list:
    """Host cores on the NUMA node GPU `index` hangs off (sysfs `local_cpulist` of its PCI function), [] when that cannot be read."""
    try:
        p = torch.cuda.get_device_properties(index)
        bdf = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
        with open(f"/sys/bus/pci/devices/{bdf}/local_cpulist") as f:
            return _parse_cpulist(f.read())
    except Exception:  # noqa: BLE001 - older torch without the pci fields, containers without sysfs, ...
        return []


def thread_siblings(cpu: int) -> tuple:
    """The hardware threads of the physical core `cpu` belongs to (sysfs), (cpu,) when unknown."""
    try:
        with open(f"/sys/devices/system/cpu/cpu{cpu}/topology/thread_siblings_list") as f:
            return tuple(sorted(_parse_cpulist(f.read())))
    except Exception:  # noqa: BLE001
        return (cpu,)


def rank_core_slice(local_rank: int, local_world: int, allowed: list, gpu_cores_of, siblings_of=None) -> list:
    """The slice of `allowed` rank `local_rank` pins itself to.  NUMA-aware (round 6): ranks whose GPUs share a NUMA node split THAT node's PHYSICAL cores among them
    (the issuing thread's doorbell writes and signal reads stay on the GPU's socket, and no two ranks' busy threads land on hyperthreads of one core); when the
    topology cannot be read, or a node has fewer than two hardware threads per rank, the plain contiguous split of round 5.  `gpu_cores_of(i)` -> cores local to
    GPU i, `siblings_of(cpu)` -> the hardware threads of its core (pure function of its arguments: tested on the CPU)."""
    if local_world <= 1 or len(allowed) < 2 * local_world:
        return list(allowed)
    k = len(allowed) // local_world
    plain = allowed[local_rank * k:(local_rank + 1) * k]
    aset = set(allowed)
    nodes = [tuple(c for c in gpu_cores_of(i) if c in aset) for i in range(local_world)]
    mine = nodes[local_rank]
    if not mine or any(not n for n in nodes):
        return plain
    peers = [i for i in range(local_world) if nodes[i] == mine]
    sib = siblings_of or (lambda c: (c,))
    groups, seen = [], set()
    for c in mine:                       # physical cores of the node, in enumeration order, each with its allowed hardware threads
        if c in seen:
            continue
        g = tuple(t for t in sib(c) if t in aset and t in set(mine)) or (c,)
        seen.update(g)
        groups.append(g)
    per = len(groups) // len(peers)
    if per < 1 or per * len(groups[0]) < 2:
        return plain
    j = peers.index(local_rank)
    return sorted(t for g in groups[j * per:(j + 1) * per] for t in g)


def pin_rank_cores(local_rank: int, local_world: int, share_gpu: bool = False) -> list:
    """Confine this rank (the calling thread; torch's pool threads are created later and inherit the mask) to its own slice of the cores the process may use, so
    that the busy host thread of each of N ranks never shares a core with another rank's.  Returns the slice (printed as `host_cores_per_rank`).  No-op for a
    single rank."""
    if not hasattr(os, "sched_getaffinity"):
        return []
    cores = sorted(os.sched_getaffinity(0))
    if local_world <= 1 or len(cores) < 2 * local_world:
        return cores
    mine = rank_core_slice(local_rank, local_world, cores, (lambda i: []) if share_gpu else gpu_local_cores, thread_siblings)
    try:
        os.sched_setaffinity(0, mine)
    except OSError:
        return cores
    torch.set_num_threads(max(1, min(8, len(mine) - 2)))
    return mine


def patch_embed_leg(ops, vol, dev, reps=10):
    """(f)2, SURVEY §8(f) rank 2: the cost patch embedding of one frame (both volumes: S = 9600 slices of 60 x 80) through the fused kernel, next to
    the same three layers as PyTorch / MIOpen bf16 convolutions (intermediate maps through HBM).  Random Conv2d-default weights (no checkpoint).
    Algorithmic work per slice: 2 x (1280x16x36 + 320x32x576 + 80x64x1152) = 25.07 MFLOP; HBM: the slice in + the tokens out."""
    import torch.nn.functional as F

    from tools.synth import patch_embed_weights

    S, H2, W2 = vol.shape[0], vol.shape[-2], vol.shape[-1]
    if not ops.cost_patch_embed_supported(H2, W2):
        return None
    Wt = [t.to(dev) for t in patch_embed_weights(0)]
    pk = ops.PatchEmbedWeights(*Wt)                        # fp32 layers: IEEE-half operands (TF32's mantissa), the hook's choice for fp32 / fp16 encoders
    out = torch.empty((S, (H2 + 7) // 8 * ((W2 + 7) // 8), 64), dtype=torch.float32, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        ops.cost_patch_embed(vol, pk, tokens=True, out=out)
    e0.record()
    for _ in range(reps):
        ops.cost_patch_embed(vol, pk, tokens=True, out=out)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    hp_, wp_ = (H2 + 7) // 8 * 8, (W2 + 7) // 8 * 8
    fl = S * 2.0 * (hp_ * wp_ // 4 * 16 * 36 + hp_ * wp_ // 16 * 32 * 576 + hp_ * wp_ // 64 * 64 * 1152)      # the three layers' multiply-adds on the padded slice
    byts = S * (H2 * W2 * 4 + out.shape[1] * 64 * 4.0)
    leg = {"what": f"cost patch embedding of one frame's volumes (S = {S} slices {H2}x{W2} -> {out.shape[1]} tokens x 64), fused kernel mv_cost_patch_embed: 16-bit MFMA ({pk.operand} operands), fp32 "
                   "accumulate, both intermediate maps in LDS", "us_per_frame": round(us, 1), "algorithmic_gflop": round(fl / 1e9, 1),
           "roofline": {"bound": "mfma", "achieved": round(fl / us / 1e6, 1), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(fl / us / 1e6 / PEAK_BF16_MFMA_TFLOPS, 4),
                        "traffic": None, "kernel": ("cost_patch_embed_pipelined_kernel<%d,%d>" if (H2, W2) in ((60, 80), (64, 80)) else "cost_patch_embed_strip_kernel<%d,%d>") % (H2, W2), "algorithmic_hbm_bytes": byts, "hbm_GBps": round(byts / us / 1e3, 1)}}
    # Fast mode (row (f)2 as SURVEY words it): fp16 cells in (the out16 volume), fp16 tokens out — no widening pass on either side
    try:
        v16 = vol.half()
        o16 = torch.empty_like(out, dtype=torch.float16)
        for _ in range(3):
            ops.cost_patch_embed(v16, pk, tokens=True, out=o16)
        e0.record()
        for _ in range(reps):
            ops.cost_patch_embed(v16, pk, tokens=True, out=o16)
        e1.record()
        torch.cuda.synchronize()
        us16 = e0.elapsed_time(e1) * 1e3 / reps
        same = bool(torch.equal(o16, ops.cost_patch_embed(v16.float(), pk, tokens=True).half()))
        leg["fast_mode"] = {"what": "fp16 cells in, fp16 tokens out (mv_cost_patch_embed_t)", "us_per_frame": round(us16, 1), "achieved": round(fl / us16 / 1e6, 1),
                            "frac": round(fl / us16 / 1e6 / PEAK_BF16_MFMA_TFLOPS, 4), "algorithmic_hbm_bytes": byts / 2, "hbm_GB_per_frame": round(byts / 2e9, 4),
                            "hbm_GBps": round(byts / 2 / us16 / 1e3, 1), "kernel": leg["roofline"]["kernel"][:-1] + ",f16 in,f16 out>",
                            "tokens_equal_fp32_form_rounded_once": same}
        del v16, o16
    except Exception as e:  # noqa: BLE001
        leg["fast_mode"] = {"error": repr(e)[:200]}
    try:
        # parity of what was just timed: a few slices against the conv2d chain in the same arithmetic (16-bit operands, fp32 accumulation) — the oracle as the checker
        from oracle import patch_embed as ope

        idx = torch.tensor([0, S // 2, S - 1])
        ref = ope.to_tokens(ope.patch_embed_proj_16(vol[idx.to(dev)].cpu(), *[t.cpu() for t in Wt], dtype=torch.float16 if pk.operand == "f16" else torch.bfloat16))
        err = float((out[idx.to(dev)].cpu() - ref).abs().max())
        leg["parity"] = {"max_abs_err_vs_conv2d_chain_" + pk.operand: err, "scale": float(ref.abs().max()),
                         "within_bar": bool(err <= (2.5e-4 if pk.operand == "f16" else 2e-3) * float(ref.abs().max())),
                         "note": "FlowFormer submodule absent from the reference checkout: pinned to torch's F.conv2d on the published layer shapes"}
        xb = F.pad(vol, (0, (8 - W2 % 8) % 8, 0, (8 - H2 % 8) % 8)).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        wb = [t.to(torch.bfloat16) for t in Wt]

        def unfused():
            y = F.relu(F.conv2d(xb, wb[0], wb[1], stride=2, padding=2))
            y = F.relu(F.conv2d(y, wb[2], wb[3], stride=2, padding=2))
            return F.conv2d(y, wb[4], wb[5], stride=2, padding=2)

        for _ in range(2):
            unfused()
        e0.record()
        for _ in range(3):
            unfused()
        e1.record()
        torch.cuda.synchronize()
        leg["unfused_miopen_bf16_us_per_frame"] = round(e0.elapsed_time(e1) * 1e3 / 3, 1)
    except Exception as e:  # noqa: BLE001
        leg["unfused_error"] = repr(e)[:200]
    return leg


def kernels_leg(ops, frames, cam, args, dev, volume_roofline, patch_embed, n_q, C):
    """one roofline entry per SURVEY §8(d) kernel in the line the driver parses.  Every kernel ALONE on the GPU, launched back
    to back between two HIP events on the launch stream (>= 100 launches after >= 20 untimed ones; the figure is the kernel's period, so a
    launch-bound kernel shows up as such), algorithmic bytes / FLOPs exactly as §8(d) defines them, peak from MI355X_MICROARCH.md."""
    import statistics as st

    from tools import synth

    H, W = args.height, args.width
    h8, w8 = H // 8, W // 8

    def period_us(fn, n=100, warm=20):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    def hbm(name, us, nbytes, note=None, **extra):
        d = {"us": round(us, 2), "bound": "hbm", "algorithmic_bytes": nbytes, "achieved": round(nbytes / us / 1e3, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
             "frac": round(nbytes / us / 1e3 / PEAK_HBM_GBS, 4), **extra}
        if note:
            d["note"] = note
        out[name] = d

    out: dict = {}
    fr = frames[0]
    # volume: the line's own roofline object (HIP events inside the pipe) + alone
    if volume_roofline is not None:
        out["volume"] = {"kernel": volume_roofline.get("kernel"), "us": volume_roofline.get("isolated_avg_launch_us", volume_roofline["avg_launch_us"]),
                         "us_in_pipe": volume_roofline["avg_launch_us"], "bound": volume_roofline["bound"], "peak": volume_roofline["peak"], "unit": volume_roofline["unit"],
                         "algorithmic_flops": volume_roofline["algorithmic_flops_per_launch"], "algorithmic_bytes": volume_roofline["algorithmic_bytes_per_launch"],
                         "executed_flops": volume_roofline.get("executed_flops_per_launch"),
                         "frac": volume_roofline.get("isolated_frac", volume_roofline["frac"]), "frac_in_pipe": volume_roofline["frac"]}
    if args.feat_dtype != "f32" or args.layout != "chw":
        return out
    vol = ops.corr_volume(fr.fmap1, fr.fmap2)
    P = fr.fmap1.shape[0]                                                 # 2 pairs
    tok = torch.empty((P, 81, h8, w8), dtype=torch.float32, device=dev)
    it = [0]

    def lk():
        ops.corr_lookup(vol, fr.coords[it[0] % fr.coords.shape[0]], 4, out=tok)
        it[0] += 1

    look_bytes = P * (n_q * 100 * 4 + n_q * 8 + n_q * 81 * 4.0)           # §8(d): N (10 x 10 cells) 4 + N 8 + N 81 4 per pair
    hbm("lookup_B2", period_us(lk, 240), look_bytes, kernel="corr_lookup_kernel (one frame: 2 pairs)")
    # Fast mode: the same lookup on 2-byte cells
    try:
        h1, h2 = fr.fmap1.permute(0, 2, 3, 1).contiguous().half(), fr.fmap2.permute(0, 2, 3, 1).contiguous().half()
        v16 = ops.corr_volume_out16(h1, h2)
        if v16 is not None:
            hbm("volume_out16", period_us(lambda: ops.corr_volume_out16(h1, h2, out=v16)), P * (2.0 * n_q * C * 2 + 2.0 * n_q * n_q),
                kernel="corr_volume_h_stream<out16> (fp16 features -> fp16 cells: MACVO_Fast.yaml:73-74)")
            hbm("lookup_B2_vol16", period_us(lambda: ops.corr_lookup(v16, fr.coords[0], 4, out=tok), 240), P * (n_q * 100 * 2 + n_q * 8 + n_q * 81 * 4.0),
                kernel="corr_lookup on fp16 cells")
            vt16 = ops.corr_volume_out16(h1, h2, tiled=True)
            hbm("lookup_B2_vol16_tiled", period_us(lambda: ops.corr_lookup(vt16, fr.coords[0], 4, out=tok, tiled=True), 240),
                P * (n_q * 100 * 2 + n_q * 8 + n_q * 81 * 4.0), kernel="corr_lookup_tiled on fp16 cells in 4 x 4 tiles (one 32-B sector each)")
            del vt16
        del h1, h2, v16
    except Exception as e:  # noqa: BLE001
        out["volume_out16"] = {"error": repr(e)[:200]}
    del vol
    # convex upsampling: one call of the decoder loop (B = 2 fields), fp32 mask as covhead.py:121-135 hands it over, and the bf16 mask read as it is
    g = torch.Generator().manual_seed(3)
    fl8 = torch.randn(P, 2, h8, w8, generator=g).to(dev)
    mk = torch.randn(P, 576, h8, w8, generator=g).to(dev)
    ub = P * n_q * (576 * 4 + 8 + 128 * 4.0)
    hbm("convex_upsample", period_us(lambda: ops.convex_upsample(fl8, mk, 0.25), 240), ub, kernel="convex_upsample_kernel<f32 mask>")
    mk16 = mk.bfloat16()
    hbm("convex_upsample_bf16_mask", period_us(lambda: ops.convex_upsample(fl8, mk16, 0.25), 240), P * n_q * (576 * 2 + 8 + 128 * 4.0), kernel="convex_upsample_kernel<bf16 mask>")
    del mk, mk16
    # patch embedding: from its own leg
    if patch_embed and "roofline" in patch_embed:
        r = patch_embed["roofline"]
        out["patch_embed"] = {"us": patch_embed["us_per_frame"], "bound": "mfma", "algorithmic_flops": patch_embed["algorithmic_gflop"] * 1e9, "algorithmic_bytes": r["algorithmic_hbm_bytes"],
                              "achieved": r["achieved"], "peak": r["peak"], "unit": r["unit"], "frac": r["frac"], "kernel": r["kernel"]}
        if "fast_mode" in patch_embed:
            f = patch_embed["fast_mode"]
            out["patch_embed_fast_mode"] = {"us": f["us_per_frame"], "bound": "mfma", "algorithmic_flops": patch_embed["algorithmic_gflop"] * 1e9,
                                            "algorithmic_bytes": f["algorithmic_hbm_bytes"], "achieved": f["achieved"], "peak": r["peak"], "unit": r["unit"], "frac": f["frac"],
                                            "kernel": f["kernel"]}
    # selector, covariance, solve: latency-bound by §8(d)'s own account ("report us"); the HBM fraction is printed for completeness
    fc = synth.flow_cov_maps(H, W, 2).to(dev)
    hbm("selector", period_us(lambda: ops.kp_select("nodepth", H, W, flow_cov=fc, kernel_size=7, mask_width=32, max_match_cov=100.0)), 4.0 * H * W * 3 + H * W,
        note="CovAwareSelector_NoDepth candidate stage (kp_nms + kp_finish; the count D2H + host randperm + gather follow in `finish`): latency-bound, §8(d) asks for us",
        kernel="kp_nms_kernel + kp_finish_kernel")
    depth = synth.depth_maps(H, W, 3)[0].to(dev)
    kp = synth.keypoints(200, H, W, 5).float().to(dev)
    fcv = (torch.ones(200, 3) * 0.25).to(dev)
    K = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    hbm("covariance", period_us(lambda: ops.match_cov(depth, kp, fcv, None, *K)), 200 * (31 * 31 * 4 + 28 + 72.0), note="MatchCovariance, N = 200, 31 x 31 window: latency-bound",
        kernel="match_cov_kernel")
    try:
        from tools.synth import pgo_batch as _to_batch, pgo_problem

        prob, _ = pgo_problem(n=200, seed=6)
        batch = _to_batch([prob], dev)
        us = period_us(lambda: ops.pgo_solve(batch, args.graph), 60, 10)
        pose, info = ops.pgo_solve(batch, args.graph)
        steps = int(info[0, 0].item()) if info.dim() == 2 else int(info[0].item())
        out["solve"] = {"us": round(us, 2), "bound": "latency", "algorithmic_bytes_per_lm_iteration": 200 * 15 * 8, "lm_steps": steps,
                        "kernel": "pgo_solve_kernel (one problem, one workgroup: dependent fp64 chain; §8(d): report us/solve)", "frac": None}
        big = _to_batch([prob] * 4096, dev)
        usb = period_us(lambda: ops.pgo_solve(big, args.graph), 10, 3)
        out["solve_batched_4096"] = {"us": round(usb, 1), "solves_per_s": round(4096 / usb * 1e6), "bound": "latency", "frac": None}
        del big
    except Exception as e:  # noqa: BLE001
        out["solve"] = {"error": repr(e)[:200]}
    # configs[4]: the batched lookup, B = 64 pairs on a 5.9-GB volume
    if (H, W) == (480, 640):
        try:
            f1 = torch.randn(64, C, h8, w8, device=dev)
            f2 = torch.randn(64, C, h8, w8, device=dev)
            vb = ops.corr_volume(f1, f2)
            del f1, f2
            co = fr.coords[0].repeat(32, 1, 1, 1)
            tb = torch.empty((64, 81, h8, w8), dtype=torch.float32, device=dev)
            hbm("lookup_B64", period_us(lambda: ops.corr_lookup(vb, co, 4, out=tb), 40, 8), 64 * (n_q * 100 * 4 + n_q * 8 + n_q * 81 * 4.0), kernel="corr_lookup_kernel (configs[4]: 64 pairs)")
            del vb
            # ... and Fast mode's 2-byte cells: row-major and in 4 x 4 tiles
            h1 = torch.randn(64, h8, w8, C, device=dev).half()
            h2 = torch.randn(64, h8, w8, C, device=dev).half()
            b16 = 64 * (n_q * 100 * 2 + n_q * 8 + n_q * 81 * 4.0)
            v16 = ops.corr_volume_out16(h1, h2)
            if v16 is not None:
                hbm("lookup_B64_vol16", period_us(lambda: ops.corr_lookup(v16, co, 4, out=tb), 40, 8), b16, kernel="corr_lookup on fp16 cells (64 pairs)")
                ops.corr_volume_out16(h1, h2, out=v16, tiled=True)
                hbm("lookup_B64_vol16_tiled", period_us(lambda: ops.corr_lookup(v16, co, 4, out=tb, tiled=True), 40, 8), b16,
                    kernel="corr_lookup_tiled on fp16 cells in 4 x 4 tiles (64 pairs)")
            del v16, h1, h2, tb, co
        except Exception as e:  # noqa: BLE001
            out.setdefault("lookup_B64", {"error": repr(e)[:200]})
    torch.cuda.empty_cache()
    return out


def plugin_path_leg(cam, cfr, n_frames, graph):
    """VERDICT r4 missing #4: the cost of the drop-in path itself.  The reference's unmodified ``Odometry/MACVO.py`` loop with the HIP plugins behind its
    registries (``type: HIP_*``) and a replay network, on the benchmark's own network outputs: steady-state ms per ``run_pair`` (first 5 frames
    dropped) and, from a second run under cProfile, the three largest host costs per frame."""
    import subprocess
    import tempfile

    import numpy as np

    from tests import refrun

    if refrun.reference_root() is None:
        return None
    n_frames = min(n_frames, len(cfr))
    with tempfile.TemporaryDirectory() as tmp:
        mf = os.path.join(tmp, "maps.npz")
        np.savez(mf, flow=torch.stack([f["flow"] for f in cfr[:n_frames]]).numpy(),
                 cov=torch.stack([torch.exp(f["logcov"] * 2) for f in cfr[:n_frames]]).numpy(), cam=np.array(json.dumps(cam)))
        base = [sys.executable, os.path.join(ROOT, "tests", "refrun.py"), "--mode", "hip", "--case", "synth_fast", "--maps-file", mf, "--mapping", "0", "--graph", graph,
                "--repeat-maps", "3"]
        res = {}
        for tag, extra in (("timed", []), ("profiled", ["--cprofile"])):
            p = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
            ln = [x for x in p.stdout.splitlines() if x.startswith('{"case"')]
            if p.returncode != 0 or not ln:
                return {"error": tag + ": " + (p.stdout[-300:] + p.stderr[-900:])}
            res[tag] = json.loads(ln[-1])
    t = res["timed"]
    return {"what": "tests/refrun.py --mode hip: the reference's own MACVO.run_pair loop (Odometry/MACVO.py:173-337, unmodified) with HIP_FlowFormerCovFrontend (replay network: "
                    "the benchmark's own flow / sigma maps), HIP_CovAwareSelector_NoDepth, HIP_MatchCovariance, HIP_TwoFrame_PGO; one torch.cuda.synchronize per frame",
            "frames": t["frames"], "dropped_first": 5, "ms_per_run_pair": round(t["s_per_frame_after5"] * 1e3, 3), "ms_per_run_pair_median": round(t["s_per_frame_median"] * 1e3, 3),
            "classes": t["classes"], "host_top3_ms_per_frame": res["profiled"].get("host_top"),
            "note": "host_top3 from a second run under cProfile (tottime, own time of the function; the profiler inflates Python-heavy entries)"}


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    my_cores = pin_rank_cores(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", str(world))), args.share_gpu) if not args.dry_collectives else []
    if args.gpus > 1 and "RANK" not in os.environ:
        raise SystemExit(self_launch(args))      # one rank per GPU under torch.distributed.run, output handed through
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU")
    if args.dry_collectives:
        return dry_collectives(args, rank, world)
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP hot path has no CPU fallback)"
    dev_index = 0 if args.share_gpu else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = None
    if world > 1 or "RANK" in os.environ:  # launched by torch.distributed.run (also exercises RCCL at world = 1)
        import torch.distributed as dist_mod

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if torch.cuda.device_count() <= dev_index:
            raise SystemExit(f"rank {rank}: local rank {local_rank} has no GPU ({torch.cuda.device_count()} visible)")
        if args.share_gpu:
            dist_mod.init_process_group(backend="gloo")
        else:
            dist_mod.init_process_group(backend="nccl", device_id=dev)
        dist = dist_mod

    from macvo_amd import ops
    from macvo_amd.distributed import gather_tracks
    from macvo_amd.pipeline import Camera, FrameInputs, HotPath, HotPathConfig, NativeHotPath, stack_lanes
    from tools import synth

    if args.volume_precision is None:
        args.volume_precision = ops.default_volume_precision()      # the library's one default (f16x2): bench, plugins and drivers agree
    H, W, C = args.height, args.width, args.channels
    h8, w8 = H // 8, W // 8
    n_q = h8 * w8
    fdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.feat_dtype]
    native = args.driver == "native"
    use_graphs = args.graphs
    assert not (native and use_graphs), "--graphs belongs to the Python driver"
    assert args.lanes == 1 or native, "--lanes > 1 needs the native driver"
    assert args.pool % 6 == 0 or not use_graphs, "--pool must be a multiple of 6 with graphs (one graph per resident frame)"

    # ---- synthetic, seeded, per-rank sequence (closed trajectory so the pool can be cycled without a seam)
    cam, frames_cpu, truth = synth.make_sequence(args.pool, H, W, C=C, iters=args.iters, seed=1000 + rank, feat_dtype=fdt,
                                                 pool=args.feat_pool or args.pool, closed_loop=True)
    if args.layout == "hwc":
        for fr in frames_cpu:
            fr["fmap1"] = fr["fmap1"].permute(0, 2, 3, 1).contiguous()
            fr["fmap2"] = fr["fmap2"].permute(0, 2, 3, 1).contiguous()
    cache = {}

    def to_dev(t):
        k = t.data_ptr()
        if k not in cache:
            cache[k] = t.to(dev)
        return cache[k]

    frames = [FrameInputs(static=True, **{k: to_dev(v) for k, v in fr.items()}) for fr in frames_cpu]

    frames16: list = []

    def fast_frames():
        """The same frames as the encoder of MACVO_Fast.yaml:73-74 hands them over: fp16 HWC feature maps (built once, for the fast-mode leg)."""
        if not frames16:
            for fr in frames_cpu:
                f1, f2 = fr["fmap1"], fr["fmap2"]
                if args.layout == "chw":
                    f1, f2 = f1.permute(0, 2, 3, 1), f2.permute(0, 2, 3, 1)
                d = dict(fr, fmap1=f1.contiguous().half().to(dev), fmap2=f2.contiguous().half().to(dev))
                frames16.append(FrameInputs(static=True, **{k: (v if v.is_cuda else to_dev(v)) for k, v in d.items()}))
        return frames16

    def lane_batches(lanes, fast=False):
        """Step t of an L-lane pipe = frames (t + l) % pool of the closed trajectory, l = 0..L-1: every lane is the same
        kind of sequence at a different phase (consecutive frames per lane), stacked along the pair axis."""
        src = fast_frames() if fast else frames
        if lanes == 1:
            return src
        return [stack_lanes([src[(t + l) % args.pool] for l in range(lanes)]) for t in range(args.pool)]

    def make_pipe(lanes, seed, precision=None, keep_extras=False, fast=False):
        cfg = HotPathConfig(graph_type=args.graph, feature_layout=args.layout,
                            volume_precision=(precision or args.volume_precision) if args.feat_dtype == "f32" else "exact",
                            volume_store=args.volume_store, use_graphs=use_graphs)
        if fast:
            cfg = HotPathConfig(graph_type=args.graph, feature_layout="hwc", volume_precision="exact", volume_store="encoder")
        if native:
            # lanes > 1: integer seeds = the driver's native per-lane MT19937 generators (bit-identical to torch.Generator(seed) +
            # torch.randperm; 32 host-side torch.randperm calls per step were the bound of the 32-lane configuration)
            # lanes == 1 (round 5): the same native generator, seeded like the reference's `torch.manual_seed(seed)` — the line's parity block runs
            # this very mechanism against the oracle / the reference loop on torch's global generator (keypoints bit-exact); --host-randperm
            # restores torch.randperm on the Python side (45 us of host time per frame inside the selector -> backend gap)
            gens = None if (lanes == 1 and args.host_randperm) else [seed + l for l in range(lanes)]
            return NativeHotPath(Camera(**cam), cfg, dev, lanes=lanes, generators=gens, keep_extras=keep_extras)
        return HotPath(Camera(**cam), cfg, dev)

    coll_dev = torch.device("cpu") if args.share_gpu else dev      # gloo (test mode): scalar collectives on host tensors

    def barrier():
        if dist is not None:
            dist.barrier()

    last_timeline: dict = {}
    last_host: dict = {}
    last_period: dict = {}
    last_region: dict = {}

    def measure(lanes, steps, warmup, seed, with_events, precision=None, fast=False, dump_dir=None):
        """W untimed + K timed steps of an L-lane pipe.  Returns (elapsed s, poses, per-launch GEMM ms, launches in region).
        ``dump_dir``: write the last timed step's outputs there (:func:`last_step_outputs`)."""
        batches = lane_batches(lanes, fast)
        hot = make_pipe(lanes, seed, precision, fast=fast)
        torch.manual_seed(seed)  # the selector consumes the global CPU generator (reference behaviour) when lanes == 1
        hot.initialize(batches[0])
        t_idx = 1
        if use_graphs:   # setup: one pass over the resident frames captures their decoder-side hipGraphs
            for _ in hot.run(batches[(t_idx + k) % args.pool] for k in range(args.pool)):
                pass
            t_idx += args.pool
        if not args.no_ramp:   # untimed sustained load: the driver's short runs (--steps 20) would otherwise sample cold clocks
            t_end = time.perf_counter() + RAMP_SECONDS
            while time.perf_counter() < t_end:
                for _ in hot.run(batches[(t_idx + k) % args.pool] for k in range(args.pool)):
                    pass
                t_idx += args.pool
                torch.cuda.synchronize()
            # the ramp's length is wall-clock bound: restart the sequence where initialize() left it (whole passes over the pool, so the
            # previous frame is the initial one again; pose prior and permutation generators reset) - the warm-up and timed steps then
            # compute the same values in every run with the same arguments (--dump-outputs)
            hot.pose = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=dev)
            torch.manual_seed(seed)
            if getattr(hot, "_native_seeds", False):
                seeds = (ops.C.c_uint64 * lanes)(*[seed + l for l in range(lanes)])
                ops.L.check(hot._lib.mv_frame_pipe_seed_lanes(hot._pipe, seeds), "mv_frame_pipe_seed_lanes")
        shape = (steps, 7) if lanes == 1 else (steps, lanes, 7)
        poses = torch.zeros(shape, dtype=torch.float32, device=dev)
        stamps = torch.arange(steps, dtype=torch.int64, device=dev) * 33_333_333   # synthetic 30 Hz frame timestamps (ns)
        # the contract's W warm-up steps run exactly the timed code path (pose sink included: its first device-to-device copy
        # and the first gather set up lazily)
        n_ev = max(steps, MIN_TIMED_LAUNCHES) if with_events else 0
        if native and n_ev:
            # create the timing events NOW (8 hipEventCreate per timed frame: milliseconds of host time): between the warm-up and the timed region the GPU must not
            # idle longer than the contract's barrier + synchronize needs — after a few ms of idle the clocks take tens of ms of load to come back (§4)
            hot.time_volume(n_ev)
            hot.time_volume(0)
        warm_sink = torch.zeros((max(warmup, 1),) + shape[1:], dtype=torch.float32, device=dev)
        for _ in hot.run((batches[(t_idx + k) % args.pool] for k in range(warmup)), pose_sink=warm_sink):
            pass
        t_idx += warmup
        gather_tracks(torch.zeros((steps * lanes, 7), dtype=torch.float32, device=dev), stamps.repeat_interleave(lanes), dist)
        if dist is not None:  # warm the collectives used in / around the timed region (RCCL sets channels up lazily)
            dist.all_reduce(torch.zeros(1, dtype=torch.float64, device=coll_dev), op=dist.ReduceOp.MAX)
        import gc

        gc.collect()          # ... and no cyclic-GC pass inside the ~3.4 ms timed region (a generation-2 pass over this process' objects is a sizeable fraction of it)
        gc.disable()
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        if native and n_ev:
            # HIP-event pairs around the volume GEMM, recorded by the driver on its GEMM stream.  Only those (round 5): the six timeline events per
            # frame on the other three streams are barrier packets inside the launch chains that bound a one-lane pipe; the timeline is collected in a
            # separate untimed pass below
            hot.time_detail(bool(os.environ.get("MV_BENCH_TIMELINE_IN_REGION")))
            hot.time_volume(n_ev)
        t0 = time.perf_counter()
        # software-pipelined stream (frame t+1's frontend is queued before frame t's host randperm); K full run_pairs
        trace = []   # host time of every finished step (one perf_counter per step: where a hiccup inside the ~3.4 ms region sat is part of the line)
        h0 = (getattr(hot, "host_issue_s", 0.0), getattr(hot, "host_wait_s", 0.0), getattr(hot, "host_frames", 0))
        last = None
        for last in hot.run((batches[(t_idx + k) % args.pool] for k in range(steps)), pose_sink=poses):
            trace.append(time.perf_counter() - t0)
        t_run = time.perf_counter() - t0
        last_host.clear()
        if getattr(hot, "device_driven", False) and hot.host_frames > h0[2]:
            nf = hot.host_frames - h0[2]
            last_host.update({"device_driven": True, "host_threads": int(getattr(hot, "host_threads", 1)),
                              "host_issue_us_per_frame": round((hot.host_issue_s - h0[0]) / nf * 1e6, 1),
                              "host_flow_control_wait_us_per_frame": round((hot.host_wait_s - h0[1]) / nf * 1e6, 1),
                              "note": "timed pass: the CALLER's time issuing a frame's launches (enqueue + next GEMM + finish; with host_threads = 2 the two backend launches are "
                                      "issued by the launch thread; no wait on the GPU anywhere) and time blocked in the flow control that keeps the host two "
                                      "finished frames ahead of the GPU (= host slack)"})
        elif native:
            last_host.update({"device_driven": False, "host_threads": int(getattr(hot, "host_threads", 2)), "run_loop_us_per_frame": round(t_run / steps * 1e6, 1)})
        # the one collective of the job (no-op for N = 1): poses [T,7] + time_ns [T] + T of every rank
        all_poses, _, _ = gather_tracks(poses.reshape(-1, 7), stamps.repeat_interleave(lanes), dist)
        t_gather = time.perf_counter() - t0
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        gc.enable()
        if dump_dir is not None:      # now: the result's buffers are views that the next two frames of this pipe recycle
            write_outputs(dump_dir, last_step_outputs(last, hot))
        del last
        last_region.clear()
        if trace:
            gaps = [b - a for a, b in zip([0.0] + trace[:-1], trace)]
            gmax = max(range(len(gaps)), key=lambda i: gaps[i])
            srt = sorted(gaps)
            last_region.update({"elapsed_us": round(elapsed * 1e6, 1), "run_loop_returned_us": round(t_run * 1e6, 1), "gather_issued_us": round(t_gather * 1e6, 1),
                                "host_step_interval_us": {"median": round(srt[len(srt) // 2] * 1e6, 1), "max": round(gaps[gmax] * 1e6, 1), "max_at_step": gmax},
                                "note": "host clock inside the timed region: when the run loop returned its last result, when the pose gather was issued (it waits for the "
                                        "last frames: the drain), when everything was synchronised; the largest interval between two finished steps and where it sat"})
        if os.environ.get("MV_BENCH_TRACE") and rank == 0:
            print("[bench trace] step-finished times (us): " + " ".join(f"{x * 1e6:.0f}" for x in trace[:40]) +
                  f" | run() returned {t_run * 1e6:.0f} | gather issued {t_gather * 1e6:.0f} | synchronized {elapsed * 1e6:.0f}", file=sys.stderr)
        if dist is not None:
            tmax = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            elapsed = float(tmax.item())
        assert torch.isfinite(all_poses).all(), "non-finite pose in the benchmark stream"
        t_idx += steps
        ms = []
        if native and n_ev:
            extra = n_ev - steps   # short runs: keep the same stream going (untimed for `value`) until enough GEMMs are timed
            if extra > 0:
                for _ in hot.run(batches[(t_idx + k) % args.pool] for k in range(extra)):
                    pass
            ms = hot.volume_times_ms()
            starts = hot.volume_starts_ms()[:steps]          # the timed pass itself (not the separate timeline pass below)
            last_period.clear()
            if len(starts) >= 8:
                d = sorted(starts[i + 1] - starts[i] for i in range(len(starts) // 4, len(starts) - 1))
                last_period.update({"period_us_timed_pass": round(d[len(d) // 2] * 1e3, 1), "gemm_starts_used": len(d)})
            # where a step's time goes, from the HIP events the driver records on its own streams (tools/lane_timeline.py):
            # GEMM start -> next GEMM start = period; the part of it the GEMM stream idles; how far the decoder-side chain lags.
            # Untimed pass over the same stream with all eight events per frame.
            if not os.environ.get("MV_BENCH_TIMELINE_IN_REGION"):
                n_tl = min(200, n_ev)
                hot.time_detail(True)
                hot.time_volume(n_tl)
                t_idx += max(extra, 0)
                for _ in hot.run(batches[(t_idx + k) % args.pool] for k in range(n_tl)):
                    pass
            tl = hot.timeline_ms()
            if len(tl) > 12:
                import statistics as st

                lo, hi = len(tl) // 4, len(tl) - 2
                med = lambda xs: round(st.median(xs) * 1e3, 1)  # noqa: E731
                last_timeline.clear()
                last_timeline.update({
                    "period_us": med([tl[i + 1][0] - tl[i][0] for i in range(lo, hi)]),
                    "gemm_us": med([tl[i][1] - tl[i][0] for i in range(lo, hi)]),
                    "gemm_stream_idle_us": med([tl[i + 1][0] - tl[i][1] for i in range(lo, hi)]),
                    "gemm_end_to_last_lookup_us": med([tl[i][2] - tl[i][1] for i in range(lo, hi)]),
                    "last_lookup_to_selector_done_us": med([tl[i][3] - tl[i][2] for i in range(lo, hi)])})
                tb = hot.timeline_backend_ms()
                ok = [i for i in range(lo, min(hi, len(tb))) if min(tb[i]) >= 0]
                if len(ok) > 8:
                    last_timeline.update({
                        "selector_done_to_backend_start_us": med([tb[i][0] - tl[i][3] for i in ok]),
                        "backend_us": med([tb[i][1] - tb[i][0] for i in ok]),
                        "backend_end_to_pose_apply_us": med([tb[i][2] - tb[i][1] for i in ok]),
                        "pose_apply_plus_solve_us": med([tb[i][3] - tb[i][2] for i in ok]),
                        "gemm_start_to_pose_us": med([tb[i][3] - tl[i][0] for i in ok])})
        if hasattr(hot, "close"):
            hot.close()
        del hot
        return elapsed, all_poses, ms, min(steps, len(ms))

    # ---- per-launch HIP events around the dominant kernel for the Python driver (launch stream = torch's current stream)
    # the HIP events around the dominant kernel (roofline, timeline) are part of --full: a plain run times the steps alone
    with_events = args.full and not args.no_kernel_events
    vol_events = []
    if not native and with_events:
        orig_corr_volume = ops.corr_volume

        def timed_corr_volume(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = orig_corr_volume(*a, **k)
            e1.record()
            vol_events.append((e0, e1))
            return out

        ops.corr_volume = timed_corr_volume

    elapsed, main_poses, ms, in_region = measure(args.lanes, args.steps, args.warmup, 1234 + rank, with_events,
                                                 dump_dir=args.dump_outputs if rank == 0 else None)
    # every rank's gathered track: finite and not the zero padding (a rank that tracked nothing would show up here, not in `value`)
    rank_tracks_finite = [bool(torch.isfinite(main_poses[r]).all() and float(main_poses[r, :, 3:].abs().sum()) > 0) for r in range(main_poses.shape[0])]
    del main_poses
    main_timeline = dict(last_timeline)
    main_host, main_period, main_region = dict(last_host), dict(last_period), dict(last_region)
    if vol_events:
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in vol_events[-args.steps:]]
        in_region = len(ms)
        ops.corr_volume = orig_corr_volume

    # HBM traffic of the dominant kernel from a committed rocprofv3 --pmc pass over the same launch configuration
    # (scripts/pmc_gpu.sh -> profiles/*_pmc_corr_volume.json; PMC passes cannot be mixed into this run)
    traffic = traffic_file = None
    try:
        if (H, W, C, args.lanes) == (480, 640, 256, 1) and args.feat_dtype == "f32" and args.volume_precision in ("bf16x3", "f16x2"):
            path = next((q for q in (os.path.join(ROOT, "profiles", f"r{r:02d}_pmc_corr_volume_split_{args.volume_precision}.json") for r in (6, 5, 4, 3))
                         if os.path.exists(q)), "")
            if os.path.exists(path):
                traffic_file = os.path.basename(path)
                pm = json.load(open(path))
                want = "corr_volume_split_stream<2, true" if args.volume_precision == "f16x2" else "corr_volume_split_stream<3, false"
                key = next((k for k in pm if k.startswith(want)), None)
                if key is not None:
                    traffic = pm[key]["_derived"]["traffic_bytes_per_launch"]
        if (H, W, C, args.lanes) == (480, 640, 256, 1) and args.feat_dtype == "f32" and args.volume_precision == "exact":
            for name in ("r02_pmc_corr_volume.json", "r01_pmc_corr_volume.json"):
                path = os.path.join(ROOT, "profiles", name)
                if os.path.exists(path):
                    pm = json.load(open(path))
                    key = next((k for k in pm if k.startswith("corr_volume_f32_mixed" if args.layout == "chw" else "corr_volume_f32_hwc")), None)
                    if key is not None:
                        traffic = pm[key]["_derived"]["traffic_bytes_per_launch"]
                        break
        if (H, W, C, args.lanes) == (480, 640, 256, 1) and args.feat_dtype in ("f16", "bf16") and args.layout == "hwc" and args.volume_store == "fp32":
            path = os.path.join(ROOT, "profiles", "r02_pmc_corr_volume_16bit_stream.json")
            if os.path.exists(path):
                pm = json.load(open(path))
                key = next((k for k in pm if k.startswith("corr_volume_h_stream")), None)
                if key is not None:
                    traffic = pm[key]["_derived"]["traffic_bytes_per_launch"]
    except Exception:  # noqa: BLE001
        traffic = None
    roofline = roofline_of(ms, args, args.lanes, n_q, C, in_region, traffic) if ms else None
    if roofline is not None:
        # the committed rocprofv3 --kernel-trace --stats summary of this very command (profiles/r06_bench_kernel_stats.csv): the kernel's own duration (first wave in ->
        # last wave out), which the HIP-event pair above brackets from outside (it also holds the time the launch waited for CUs behind the pack)
        try:
            import csv as _csv

            kname = roofline.get("kernel", "")
            want = "corr_volume_split_stream<2, true" if "f16x2" in kname else ("corr_volume_split_stream<3, false" if "bf16x3" in kname else None)
            path = os.path.join(ROOT, "profiles", "r06_bench_kernel_stats.csv")
            if want and args.lanes == 1 and (H, W) == (480, 640) and os.path.exists(path):
                for row in _csv.DictReader(open(path)):
                    if want in row["Name"]:
                        us = float(row["AverageNs"]) / 1e3
                        fl = roofline["algorithmic_flops_per_launch"]
                        roofline["rocprofv3_committed"] = {"file": "profiles/r06_bench_kernel_stats.csv", "avg_launch_us": round(us, 2), "calls": int(row["Calls"]),
                                                           "frac_executed": round(roofline["executed_flops_per_launch"] / us / 1e6 / PEAK_BF16_MFMA_TFLOPS, 4),
                                                           "frac_algorithmic": round(fl / us / 1e6 / PEAK_BF16_MFMA_TFLOPS, 4),
                                                           "note": "NOT measured in this process: the committed trace of the same command on a builder box"}
                        break
        except Exception:  # noqa: BLE001
            pass
        roofline["traffic_source"] = (f"committed rocprofv3 --pmc pass over the same launch configuration (profiles/{traffic_file or '...'}): "
                                      "PMC passes cannot be mixed into a timed run; NOT measured in this process") if traffic is not None else None
    def isolated_us(lanes, precision):
        """The dominant kernel with the GPU to itself (back-to-back launches, HIP events): what the co-running lookups / selector /
        backend kernels of the neighbouring frames cost it inside the pipeline is the difference to avg_launch_us.  ~60 ms of
        launches first: after a few ms of idle the clocks need ~40 ms of load to come back (222 -> 190 us measured)."""
        b0 = lane_batches(lanes)[0]
        vol = ops.corr_volume(b0.fmap1, b0.fmap2, layout=args.layout, precision=precision)
        if precision in ("bf16x3", "f16x2") and ops.last_volume_kernel().startswith("corr_volume_split"):
            pk = ops.volume_pack(b0.fmap1, b0.fmap2, args.layout, mode=precision)       # the GEMM alone: the pack is a separate launch
            Bp = b0.fmap1.shape[0]
            launch = lambda: ops.corr_volume_packed(pk[0], pk[1], Bp, C, n_q, n_q, out=vol, mode=precision)  # noqa: E731
        else:
            launch = lambda: ops.corr_volume(b0.fmap1, b0.fmap2, layout=args.layout, out=vol, precision=precision)  # noqa: E731
        n_warm, n_iso = max(20, 300 // lanes), max(10, 100 // lanes)
        for _ in range(n_warm):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_iso):
            launch()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n_iso

    if roofline is not None and rank == 0 and args.feat_dtype == "f32" and args.volume_precision in ("exact", "bf16x3", "f16x2"):
        iso_us = isolated_us(args.lanes, args.volume_precision)
        roofline["isolated_avg_launch_us"] = round(iso_us, 2)
        roofline["isolated_frac"] = round(roofline["frac"] * roofline["avg_launch_us"] / iso_us, 4)

    # ---- the other volume precisions beside the default line: same stream, same step definition
    other_legs = None
    if args.full and rank == 0 and world == 1 and native and args.feat_dtype == "f32" and args.volume_precision in ("f16x2", "bf16x3", "exact") and args.exact_steps > 0:
        other_legs = {}
        what = {"exact": "v_mfma_f32_32x32x2_f32, bitwise an fmaf chain (the round-2 default)",
                "bf16x3": "three bf16 pieces per operand, six products (corr_volume_split_stream<bf16x3>)",
                "f16x2": "row-scaled, two fp16 pieces per operand, three products (corr_volume_split_stream<f16x2>)"}
        for prec in ("exact", "bf16x3", "f16x2"):
            if prec == args.volume_precision:
                continue
            args._precision = prec
            ee, _, mse, ine = measure(args.lanes, args.exact_steps, 5, 1234, not args.no_kernel_events, precision=prec)
            leg = {"what": "the same stream with volume_precision='%s': %s" % (prec, what[prec]),
                   "value": round(args.lanes * args.exact_steps / ee, 2), "unit": "stereo frames/s", "steps": args.exact_steps, "warmup": 5,
                   "ms_per_step": round(ee / args.exact_steps * 1e3, 4),
                   "roofline": roofline_of(mse, args, args.lanes, n_q, C, ine) if mse else None}
            if leg["roofline"] is not None:
                iso = isolated_us(args.lanes, prec)
                leg["roofline"]["isolated_avg_launch_us"] = round(iso, 2)
                leg["roofline"]["isolated_frac"] = round(leg["roofline"]["frac"] * leg["roofline"]["avg_launch_us"] / iso, 4)
            other_legs[prec] = leg
            del args._precision

    # ---- CPU baseline (oracle pipeline, torch-CPU ops shaped like the reference) on a bounded sample + free-running parity
    cpu_baseline = parity = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import metrics, se3
        from oracle.pipeline import OracleHotPath

        # 8 threads = what the reference's optimizer child uses (Optimization/Interface.py:254); more threads on a
        # many-core host make the small float64 LM ops slower (fork/join dominated), measured 34 s/frame at 256 threads
        cores = min(os.cpu_count() or 1, 8)
        torch.set_num_threads(cores)
        ora = OracleHotPath(cam, dict(graph_type=args.graph))
        cfr = [{k: (v.float() if v.dtype in (torch.float16, torch.bfloat16) else v) for k, v in fr.items()} for fr in frames_cpu]
        if args.layout == "hwc":
            for fr in cfr:
                fr["fmap1"] = fr["fmap1"].permute(0, 3, 1, 2).contiguous()
                fr["fmap2"] = fr["fmap2"].permute(0, 3, 1, 2).contiguous()
        torch.manual_seed(1234)
        ora.initialize(cfr[0])
        ora_track = [ora.step(cfr[1])]  # warm-up (thread pools, first-call overheads); part of the free-running track
        c0 = time.perf_counter()
        ncpu = 0
        while ncpu < args.cpu_frames and (time.perf_counter() - c0) < 25.0:
            ora_track.append(ora.step(cfr[(2 + ncpu) % args.pool]))
            ncpu += 1
        csec = time.perf_counter() - c0
        cpu_baseline = {"value": round(ncpu / csec, 3), "unit": "stereo frames/s", "cores": cores, "kind": "port",
                        "sample": f"{ncpu} frames of the same {W}x{H} workload through oracle/pipeline.py "
                                  f"(torch-CPU einsum volume, grid_sample lookup, max_pool2d selector, float64 dense-weight LM), "
                                  f"{csec:.1f} s"}
        # free-running parity: the HIP path on the same frames from the same start, chained on its OWN poses (no teacher
        # forcing), same CPU generator seed -> keypoints must be identical, poses within 1e-4; RTE per MetricsSeq.py:9-16
        if native and args.volume_precision in ("exact", "bf16x3", "f16x2") and args.feat_dtype == "f32":
            n_par = min(len(ora_track), max(args.parity_frames, 2))
            hot = make_pipe(1, 1234, keep_extras=True)       # native generator seeded 1234 (or, --host-randperm, the global generator below)
            torch.manual_seed(1234)
            hot.initialize(frames[0])
            sink = torch.zeros((n_par, 7), dtype=torch.float32, device=dev)
            kp_same = 0
            kept = []        # keypoints that survive the in-bound test and the observation filter = the rows the reference stores
            for t, r in enumerate(hot.run((frames[(1 + k) % args.pool] for k in range(n_par)), pose_sink=sink)):
                hot.sync_pose()
                kp_same += int(torch.equal(r.kp0_uv.cpu(), ora_track[t]["kp0_uv"]))
                if t < 16 and r.n_sel:
                    kept.append(r.kp0_uv[r.extras["valid"]].cpu().float().numpy())
            torch.cuda.synchronize()
            ident = torch.tensor([[0, 0, 0, 0, 0, 0, 1.0]])
            est = torch.cat([ident, sink.cpu()])
            orc = torch.cat([ident, torch.stack([o["pose"] for o in ora_track[:n_par]])])
            tru = torch.stack([truth[k % args.pool] for k in range(n_par + 1)])
            diffs = [se3.pose_error(orc[t].double(), est[t].double()) for t in range(1, n_par + 1)]
            m = metrics.rte(orc, est)
            parity = {"frames": n_par, "free_running": True, "keypoints_bit_exact_frames": kp_same,
                      "max_pose_dt_m": max(d[0] for d in diffs), "max_pose_dr_rad": max(d[1] for d in diffs),
                      "rte_vs_oracle": {k: m[k] for k in ("mean", "rmse", "max", "roe_max_rad")},
                      "rte_vs_truth": {"hip": metrics.rte(tru, est)["mean"], "oracle": metrics.rte(tru, orc)["mean"]},
                      "formula": "evo RPE translation part, delta = 1 frame (Evaluation/MetricsSeq.py:9-16)",
                      "within_north_star": bool(kp_same == n_par and max(d[0] for d in diffs) <= 1e-4 and max(d[1] for d in diffs) <= 1e-4)}
            hot.close()       # (`r` of the loop above still references the pipe: without this its four HIP streams linger beside the next legs' pipes)
            del hot
            # ... and the kernels the line times: volume rows vs fp64 einsum, every lookup's tokens vs the oracle, at the line's precision
            try:
                parity["volume_and_lookups"] = volume_lookup_parity(ops, frames, cfr, args, n_q, C, dev, sorted({0, args.pool // 2, args.pool - 1}), make_pipe)
                parity["within_north_star"] = bool(parity["within_north_star"] and parity["volume_and_lookups"]["within_bar"])
            except Exception as e:  # noqa: BLE001
                parity["volume_and_lookups"] = {"error": repr(e)[:300]}
            # ... and against the REFERENCE ITSELF: its own MACVO loop on this host, same network outputs, same generator seed
            n_ref = min(args.reference_frames, n_par + 1, args.pool)
            ref_leg = reference_loop_leg(cam, cfr, n_ref, cores, args.graph) if n_ref >= 3 else None
            if ref_leg is not None and "error" not in ref_leg:
                import numpy as np

                nk = min(len(kept), n_ref - 1)
                same = sum(int(kept[t].shape == ref_leg["kps"][t].shape and np.array_equal(kept[t], ref_leg["kps"][t])) for t in range(nk))
                rp = torch.from_numpy(ref_leg["poses"][1:n_ref]).double()
                dref = [se3.pose_error(rp[t], est[t + 1].double()) for t in range(n_ref - 1)]
                parity["vs_reference_loop"] = {
                    "what": "the reference's own unmodified Odometry/MACVO.py loop (reference selector / covariance model / TwoFrame_PGO / frontend "
                            "epilogue / VisualMap, CPU) on the same frames and generator seed, via tests/refrun.py + oracle/_ref/pyref",
                    "frames": n_ref - 1, "stored_keypoints_bit_exact_frames": same, "frames_compared_keypoints": nk,
                    "max_pose_dt_m": max(d[0] for d in dref), "max_pose_dr_rad": max(d[1] for d in dref),
                    "within_north_star": bool(same == nk and max(d[0] for d in dref) <= 1e-4 and max(d[1] for d in dref) <= 1e-4)}
                # the CPU baseline of kind "reference": the reference's loop covers everything from the network's outputs on (the backend
                # half + the frontend epilogue); the all-pairs volume and the 12 lookups live in the FlowFormer submodule, which is absent
                # from the checkout - their share is the torch-CPU restatement of the ops that submodule calls (einsum, grid_sample)
                from oracle import corr as ocorr

                tv0 = time.perf_counter()
                for k in range(2):
                    v = ocorr.corr_volume(cfr[k]["fmap1"].float(), cfr[k]["fmap2"].float(), torch.float32)
                    for it in range(cfr[k]["coords"].shape[0]):
                        ocorr.corr_lookup(v, cfr[k]["coords"][it], 4)
                vl_s = (time.perf_counter() - tv0) / 2
                port_fps = cpu_baseline["value"]
                cpu_baseline = {"value": round(1.0 / (ref_leg["s_per_run_pair"] + vl_s), 3), "unit": "stereo frames/s", "cores": cores, "kind": "reference",
                                "sample": f"{n_ref - 2} run_pair calls of the reference's own MACVO loop on the same {W}x{H} network outputs "
                                          f"({ref_leg['s_per_run_pair'] * 1e3:.0f} ms each: selector, 2 x covariance model, TwoFrame_PGO, map) + the volume and "
                                          f"{args.iters} lookups of 2 frames as the torch-CPU ops the absent FlowFormer submodule calls ({vl_s * 1e3:.0f} ms per frame)",
                                "parts": {"reference_run_pair_s": round(ref_leg["s_per_run_pair"], 4), "volume_lookups_torch_cpu_s": round(vl_s, 4),
                                          "oracle_port_pipeline_fps": port_fps}}
            elif ref_leg is not None:
                parity["vs_reference_loop"] = ref_leg
        elif native:
            # 16-bit feature lines (Fast mode): the free-running comparison above is defined on fp32 features, but the kernels THIS line times —
            # corr_volume_h_stream(<out16>) and the lookup on its cells — are checked on the pipe's own buffers all the same
            try:
                vl = volume_lookup_parity(ops, frames, cfr, args, n_q, C, dev, sorted({0, args.pool // 2, args.pool - 1}), make_pipe)
                parity = {"volume_and_lookups": vl, "within_north_star": bool(vl["within_bar"]), "free_running": False,
                          "rte_vs_oracle": {"mean": None}}
            except Exception as e:  # noqa: BLE001
                parity = {"volume_and_lookups": {"error": repr(e)[:300]}, "within_north_star": False, "rte_vs_oracle": {"mean": None}}

    # ---- Fast mode (MACVO_Fast.yaml:73-74: the encoder in fp16, so `einsum` returns — and the decoder reads — a 16-bit volume): the same frames as fp16 HWC
    # feature maps through mv_corr_volume_out16 (2-byte cells, tiled) + mv_corr_lookup_tiled_vol16.  A second workload, not the headline's configuration.
    # (Runs BEFORE the configs[4] leg: on this HIP stack a one-lane pipe — three normal-priority streams + one high-priority — created after a batched pipe —
    # two + two — has been destroyed maps two of its streams onto one hardware queue and runs 3.7x slower: 2.3 k instead of 8.4 k frames/s, profiles/r06_fast_mode.log.)
    fast_mode = None
    if (args.full and rank == 0 and world == 1 and native and args.fast_mode_steps > 0 and args.lanes == 1 and (H, W) == (480, 640) and args.feat_dtype == "f32"
            and C in (128, 256)):
        try:
            ef1 = measure(1, args.fast_mode_steps, 10, 2468, False, fast=True)[0]
            ef32 = measure(32, max(args.fast_mode_steps // 5, 10), 10, 2469, False, fast=True)[0]
            fast_mode = {"workload": "MACVO_Fast.yaml:73-74 arithmetic on the headline's frames: fp16 HWC feature maps, cost volume STORED in fp16 by the GEMM's epilogue "
                                     "(mv_corr_volume_out16) in 4 x 4-cell tiles (mv_fmap_tile_rows16), lookups on the 2-byte cells (mv_corr_lookup_tiled_vol16)",
                         "one_lane": {"value": round(args.fast_mode_steps / ef1, 2), "unit": "stereo frames/s", "steps": args.fast_mode_steps},
                         "lanes_32": {"value": round(32 * max(args.fast_mode_steps // 5, 10) / ef32, 2), "unit": "stereo frames/s", "steps": max(args.fast_mode_steps // 5, 10)},
                         "parity": "tests/test_gpu_fastmode.py (cells = the fp32 accumulators rounded once; tokens bit-equal to the fp32 lookup on the widened volume; "
                                   "pipe vs the oracle's Fast-mode arithmetic)"}
            frames16.clear()
        except Exception as e:  # noqa: BLE001
            fast_mode = {"error": repr(e)[:300]}

    # ---- configs[4]: batch-32 frames per GPU (B = 64 pairs per GEMM) — a short second measurement, N = 1 only
    config4 = None
    if args.full and rank == 0 and world == 1 and native and args.config4_steps > 0 and args.lanes == 1 and (H, W) == (480, 640):
        e4, _, ms4, in4 = measure(32, args.config4_steps, 10, 4321, not args.no_kernel_events)
        config4 = {"workload": "configs[4]: batch-32 640x480 frames per GPU = 32 lanes, one cost-volume GEMM of B = 64 pairs per step",
                   "value": round(32 * args.config4_steps / e4, 2), "unit": "stereo frames/s", "steps": args.config4_steps, "warmup": 10,
                   "ms_per_step": round(e4 / args.config4_steps * 1e3, 4),
                   "roofline": roofline_of(ms4, args, 32, n_q, C, in4) if ms4 else None,
                   "timeline": dict(last_timeline) or None,
                   "permutations": "native per-lane MT19937 + partial Fisher-Yates in the frame driver (bit-identical to torch.Generator(seed) + "
                                   "torch.randperm; 32 torch.randperm calls per step cost the host 1.4-3 ms)"}

    # ---- decoder-loop harness: the same lookups / upsamplings issued BETWEEN real PyTorch-ROCm kernels (GRU, convolutions,
    # attention of a stand-in network with the reference's loop structure, covhead.py:85-135) instead of back to back
    decoder_loop = None
    if args.full and rank == 0 and world == 1 and not args.no_decoder_leg and args.lanes == 1 and args.feat_dtype == "f32" and args.layout == "chw":
        try:
            from tools.decoder_harness import DecoderLoopHarness

            net = DecoderLoopHarness(dec_dtype=torch.bfloat16, depth=args.iters).to(dev).eval()
            vol = ops.corr_volume(frames[0].fmap1, frames[0].fmap2)
            memory = torch.randn(2 * n_q, 8, 128, device=dev)
            context = torch.randn(2, 256, h8, w8, device=dev)
            for _ in range(3):
                net(vol, memory, context)
            reps = 10
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                net(vol, memory, context)
            e1.record()
            torch.cuda.synchronize()
            loop_ms = e0.elapsed_time(e1) / reps
            net(vol, memory, context, time_hip=True)
            torch.cuda.synchronize()
            inter = net.hip_times_us()
            b0, b1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            tok = None
            b0.record()
            for it in range(args.iters * reps):
                tok = ops.corr_lookup(vol, frames[0].coords[it % args.iters], 4, out=tok)
            b1.record()
            torch.cuda.synchronize()
            decoder_loop = {"what": f"{args.iters}-iteration decoder loop of one estimate_pair (B = 2 pairs, {W}x{H}, bf16 stand-in network, fp32 HIP lookup + 2 convex upsamplings per iteration)",
                            "ms_per_estimate_pair": round(loop_ms, 3),
                            "hip_us_interleaved": {k: round(v, 2) for k, v in inter.items()},
                            "lookup_us_back_to_back": round(b0.elapsed_time(b1) * 1e3 / (args.iters * reps), 2),
                            "hip_share_of_loop": round(sum(v * (args.iters if k == "corr_lookup" else 2 * args.iters) for k, v in inter.items()) / (loop_ms * 1e3), 4)}
            del net, vol, memory, context
        except Exception as e:  # noqa: BLE001 - a measurement leg must not take the benchmark line down
            decoder_loop = {"error": repr(e)[:300]}

    # what RCCL actually connected: world size as the process group reports it + every rank's device (one all_gather of 2 ints)
    patch_embed = None
    if args.full and rank == 0 and world == 1 and not args.no_decoder_leg and args.lanes == 1 and args.feat_dtype == "f32":
        try:
            patch_embed = patch_embed_leg(ops, ops.corr_volume(frames[0].fmap1, frames[0].fmap2, layout=args.layout), dev)
        except Exception as e:  # noqa: BLE001 - a measurement leg must not take the benchmark line down
            patch_embed = {"error": repr(e)[:300]}
    kernels = plugin_path = None
    if args.full and rank == 0 and world == 1 and not args.no_decoder_leg and args.lanes == 1:
        try:
            kernels = kernels_leg(ops, frames, cam, args, dev, roofline, patch_embed, n_q, C)
        except Exception as e:  # noqa: BLE001 - a measurement leg must not take the benchmark line down
            kernels = {"error": repr(e)[:300]}
    if args.full and rank == 0 and world == 1 and args.lanes == 1 and args.plugin_frames > 0 and not args.no_cpu_baseline and args.feat_dtype == "f32":
        try:
            plugin_path = plugin_path_leg(cam, cfr, args.plugin_frames, args.graph)
            if plugin_path and "error" not in plugin_path and cpu_baseline and cpu_baseline.get("parts"):
                plugin_path["reference_cpu_ms_per_run_pair"] = round(cpu_baseline["parts"]["reference_run_pair_s"] * 1e3, 2)
        except Exception as e:  # noqa: BLE001
            plugin_path = {"error": repr(e)[:300]}
    end_to_end = None
    if args.full and rank == 0 and world == 1 and args.end_to_end_frames > 0 and args.lanes == 1 and (H, W) == (480, 640) and not args.no_cpu_baseline:
        try:
            end_to_end = end_to_end_leg(args.end_to_end_frames)
        except Exception as e:  # noqa: BLE001 - a measurement leg must not take the benchmark line down
            end_to_end = {"error": repr(e)[:300]}
    ranks_seen, rank_devices, rank_cores, rank_pose_ok = 1, [torch.cuda.current_device()], [my_cores], [True]
    rank_host = [main_host or None]
    if dist is not None:
        ranks_seen = dist.get_world_size()
        got = [None] * ranks_seen
        dist.all_gather_object(got, {"rank": rank, "device": torch.cuda.current_device(), "cores": my_cores, "steps_done": args.steps, "host": main_host or None})
        got = sorted(got, key=lambda d: d["rank"])
        rank_devices = [int(d["device"]) for d in got]
        rank_cores = [d["cores"] for d in got]
        rank_host = [d.get("host") for d in got]
    if rank == 0:
        total_frames = world * args.steps * args.lanes
        cfgname = {1: "configs[1]", 32: "configs[4]"}.get(args.lanes, f"{args.lanes}-lane variant of configs[1]")
        line = {
            "metric": "stereo frames/sec at 640x480 (hot path: cost volume + lookup, keypoint selection, covariance, PGO)",
            "value": round(total_frames / elapsed, 2),
            "unit": "stereo frames/s",
            "n_gpus": world,
            "ranks_seen": ranks_seen,
            "rank_devices": rank_devices,
            "host_cores_per_rank": len(my_cores) or None,
            "rank_core_slices": [[c[0], c[-1]] if c else None for c in rank_cores],       # (first, last core of the slice; NUMA-local slices are a core range + its hyperthread range)
            "rank_core_counts": [len(c) if c else None for c in rank_cores],
            "rank_pose_tracks_finite": rank_tracks_finite,
            "share_gpu_test_mode": bool(args.share_gpu),
            "host_threads_per_rank": ("%d busy (device-driven frames: the caller%s; nothing waits for the GPU)" % (main_host.get("host_threads", 1), " + the backend launch thread" if main_host.get("host_threads", 1) > 1 else "")
                                      if main_host.get("device_driven") else "2 busy (caller + backend launch thread)") +
                                     " + a torch pool of %d" % torch.get_num_threads(),
            "hot_path_only": True,
            "hot_path_only_note": "value = the SURVEY 8 hot path with the learned FlowFormer layers' outputs (feature maps, per-iteration coordinates, flow / "
                                  "covariance maps) resident in HBM; north_star's >= 200 frames/s END TO END is the end_to_end leg below and is NOT met",
            "end_to_end_fps": ((end_to_end or {}).get("hooked") or {}).get("fps") if isinstance(end_to_end, dict) else None,
            "period_us_timed_pass": main_period.get("period_us_timed_pass"),
            "host": main_host or None,
            "timed_region": main_region or None,
            "rank_host_issue_us_per_frame": [None if not h else h.get("host_issue_us_per_frame", h.get("run_loop_us_per_frame")) for h in rank_host],
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": {"f32": {"bf16x3": "f32 via bf16x3 (volume: fp32 operands split into three bf16 pieces, six products, fp32 accumulate) + f32 "
                                        "(lookup/covariance) + f64 (PGO)",
                              "f16x2": "f32 via f16x2 (volume: fp32 operands row-scaled by powers of two and split into two fp16 pieces, three "
                                       "products, fp32 accumulate, scales undone exactly) + f32 (lookup/covariance) + f64 (PGO)"}.get(
                                  args.volume_precision, "f32 (volume/lookup/covariance) + f64 (PGO)"),
                      "f16": "f16 in / f32 acc (volume) + f32 + f64 (PGO)",
                      "bf16": "bf16 in / f32 acc (volume) + f32 + f64 (PGO)"}[args.feat_dtype],
            "data": "synthetic (seeded planar-scene stereo stream, random feature maps; no weights/datasets available)",
            "rte_vs_oracle": None if parity is None else parity["rte_vs_oracle"]["mean"],
            "config": {"workload": f"{cfgname}: single MI355X, {W}x{H} synthetic stereo, HIP correlation volume + GN backend, "
                                   f"{args.lanes} sequence(s) per GPU in lock-step",
                       "per_step": f"{args.lanes} frame(s): {2 * args.lanes} cost volumes [{n_q}x{C}x{n_q}] in one launch + {args.iters} 9x9 lookups "
                                   f"+ epilogue + CovAwareSelector_NoDepth(200) + 2x MatchCovariance(31x31) + TwoFrame_PGO({args.graph})",
                       "lanes": args.lanes, "feature_dtype": args.feat_dtype, "feature_layout": args.layout,
                       "volume_precision": args.volume_precision, "hip_graphs": use_graphs, "host_driver": args.driver, "backend_launch_thread": (os.environ.get("MV_PIPE_ASYNC_BACKEND", "1") != "0") if args.driver == "native" else False,
                       "keypoint_permutations": ("torch.randperm on the Python side (global CPU generator)" if (args.host_randperm or not native) else
                                                 ("drawn ON THE GPU inside the backend's front launch: device-resident MT19937 (one-step block twist) + hashed partial "
                                                  "Fisher-Yates, candidate count read from device memory (csrc/randperm_dev.h) — " if main_host.get("device_driven") else
                                                  "driver-native MT19937 + partial Fisher-Yates on the host — ") +
                                                 "seeded like torch.manual_seed, bit-identical to torch.randperm: the parity block runs this mechanism against the "
                                                 "oracle and the reference loop on torch's global generator"),
                       "clock_ramp_s": 0.0 if args.no_ramp else RAMP_SECONDS,
                       "frame_schedule": schedule_note(args.lanes) if native else "python loop over the per-op entry points",
                       "excluded": "learned FlowFormer layers (source + weights absent from the reference checkout)",
                       "parallelism": f"{world * args.lanes} independent sequence(s), {args.lanes} per GPU; one all_gather of poses + timestamps"},
            "roofline": roofline,
            "timeline": main_timeline or None,
            "other_precisions": other_legs,
            "cpu_baseline": cpu_baseline,
            "parity": parity,
            "config4": config4,
            "fast_mode": fast_mode,
            "decoder_loop": decoder_loop,
            "patch_embed": patch_embed,
            "kernels": kernels,
            "plugin_path": plugin_path,
            "end_to_end": end_to_end,
            "multi_gpu_note": "no scaling curve has been measured by the builder (1-GPU boxes only): N > 1 is covered by a world-2 gloo test, a world-1 RCCL test and "
                              "2- and 8-rank rehearsals sharing one GPU (tests/test_gpu_bench.py)",
        }
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
