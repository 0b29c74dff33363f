"""Evaluation on the GPU: the reference's ``Evaluation/EvalFlow.py`` and ``Evaluation/EvalDepth.py`` (frontend), and ``Evaluation/MetricsSeq.py`` /
``Evaluation/EvalSeq.py`` (sequence metrics ATE / RTE / ROE / RPE: ``evaluateATE`` ... ``EvaluateSequences`` at the end of this file).

Two ways to call the frontend evaluation:

* ``FrontendEvaluator``: push estimates and ground truth frame by frame; every push enqueues one launch group (``ops.eval_flow`` /
  ``ops.eval_depth``) that writes one row per lane into a device-resident table and accumulates the error^2-vs-variance grids.  Nothing
  synchronises until ``result()``, the single read-back.
* ``evaluate_flow`` / ``evaluate_flowcov`` / ``evaluate_depth`` / ``evaluate_depthcov``: the reference's entry points, same names and arguments, for
  any object with the ``IMatcher`` / ``IStereoDepth`` ``estimate`` contract (``interfaces.py``) and any iterable of frames.  They return the
  reference's records (``Utility/Datatypes.py``); the ``*cov`` functions also return their recorder grid(s).  No figure is written.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from . import ops


# ------------------------------------------------------------------------------------------------ records (Utility/Datatypes.py:8-94)
def _mean(data) -> float:
    data = list(data)
    if not data:
        raise ValueError("mean() arg is an empty sequence")
    return sum(data) / len(data)


def _median(data) -> float:
    s = sorted(data)
    n = len(s)
    if n == 0:
        raise ValueError("median() arg is an empty sequence")
    return float(s[n // 2]) if n % 2 == 1 else (s[n // 2 - 1] + s[n // 2]) / 2.0


@dataclass
class FlowPerformance:
    masked_epe: float
    epe: float
    px1: float
    px3: float
    px5: float

    @classmethod
    def mean(cls, values: "list[FlowPerformance]") -> "FlowPerformance":
        return cls(**{k: sum(getattr(v, k) for v in values) / len(values) for k in ("masked_epe", "epe", "px1", "px3", "px5")})


@dataclass
class FlowCovPerformance:
    masked_nll: float
    q25_nll: float
    q50_nll: float
    q75_nll: float

    @classmethod
    def mean(cls, values: "list[FlowCovPerformance]") -> "FlowCovPerformance":
        return cls(**{k: _mean(getattr(v, k) for v in values) for k in ("masked_nll", "q25_nll", "q50_nll", "q75_nll")})


@dataclass
class DepthPerformance:
    masked_err: float
    err_25: float
    err_50: float
    err_75: float

    @classmethod
    def median(cls, values: "list[DepthPerformance]") -> "DepthPerformance":
        return cls(**{k: _median(getattr(v, k) for v in values) for k in ("masked_err", "err_25", "err_50", "err_75")})


@dataclass
class DepthCovPerformance:
    masked_nll: float
    q25_nll: float
    q50_nll: float
    q75_nll: float

    @classmethod
    def mean(cls, values: "list[DepthCovPerformance]") -> "DepthCovPerformance":
        return cls(**{k: _mean(getattr(v, k) for v in values) for k in ("masked_nll", "q25_nll", "q50_nll", "q75_nll")})


# ------------------------------------------------------------------------------------------------ device-resident accumulation
@dataclass
class EvaluationTables:
    """``FrontendEvaluator.result()``: host copies.  ``flow`` ``[lanes, n_flow, len(EVAL_FLOW_COLS)]``, ``depth`` ``[lanes, n_depth,
    len(EVAL_DEPTH_COLS)]`` (fp32 rows in push order), ``flow_grids`` uint32 ``[lanes, 2, 100, 100]`` ((eu^2, cu), (ev^2, cv)), ``depth_grid``
    uint32 ``[lanes, 100, 100]``."""
    flow: np.ndarray
    depth: np.ndarray
    flow_grids: np.ndarray
    depth_grid: np.ndarray

    def flow_records(self, lane: int = 0) -> "list[dict]":
        return [dict(zip(L.EVAL_FLOW_COLS, map(float, r))) for r in self.flow[lane]]

    def depth_records(self, lane: int = 0) -> "list[dict]":
        return [dict(zip(L.EVAL_DEPTH_COLS, map(float, r))) for r in self.depth[lane]]


class FrontendEvaluator:
    """Scores ``lanes`` sequences of ``H x W`` frames in lock step.  ``push_flow`` / ``push_depth`` enqueue on the current stream and advance
    the row index; they never synchronise.  ``result()`` reads everything back once."""

    def __init__(self, H: int, W: int, lanes: int = 1, device="cuda:0", capacity: int = 256):
        if not (1 <= lanes <= L.MV_MAX_LANES) or H < 1 or W < 1 or H * W > L.EVAL_MAX_PIXELS:
            raise L.MacvoHipError(f"FrontendEvaluator: {lanes} lanes of {H}x{W} are not supported (lanes <= {L.MV_MAX_LANES}, H * W <= 2^22)")
        self.H, self.W, self.lanes, self.device = H, W, lanes, torch.device(device)
        self._flow = self._table(capacity, len(L.EVAL_FLOW_COLS))
        self._depth = self._table(capacity, len(L.EVAL_DEPTH_COLS))
        self._flow_grids = torch.zeros((lanes, 2, L.EVAL_GRID, L.EVAL_GRID), dtype=torch.int32, device=self.device)
        self._depth_grid = torch.zeros((lanes, L.EVAL_GRID, L.EVAL_GRID), dtype=torch.int32, device=self.device)
        self.n_flow = self.n_depth = 0

    def _table(self, cap: int, ncols: int) -> torch.Tensor:
        return torch.full((self.lanes, max(1, cap), ncols), float("nan"), dtype=torch.float32, device=self.device)

    def _room(self, table: torch.Tensor, used: int) -> torch.Tensor:
        if used < table.shape[1]:
            return table
        grown = self._table(2 * table.shape[1], table.shape[2])          # a device-side copy on the current stream: no synchronisation
        grown[:, :used] = table[:, :used]
        return grown

    def reset(self) -> None:
        self._flow_grids.zero_()
        self._depth_grid.zero_()
        self.n_flow = self.n_depth = 0

    def push_flow(self, est_flow, gt_flow, est_cov=None, valid=None, max_flow: float = 128.0, apply_max_flow: bool = True) -> int:
        """One frame per lane (EvalFlow.py:29-47, 82-127).  Returns the row index the frame received."""
        self._flow = self._room(self._flow, self.n_flow)
        ops.eval_flow(est_flow, gt_flow, est_cov, valid, max_flow, apply_max_flow, rows=self._flow, row=self.n_flow,
                      grids=self._flow_grids if est_cov is not None else None)
        self.n_flow += 1
        return self.n_flow - 1

    def push_depth(self, est_depth, gt_depth, est_cov=None, max_depth: float = 80.0) -> int:
        """One frame per lane (EvalDepth.py:22-34, 57-82).  Returns the row index the frame received."""
        self._depth = self._room(self._depth, self.n_depth)
        ops.eval_depth(est_depth, gt_depth, est_cov, max_depth, rows=self._depth, row=self.n_depth,
                       grids=self._depth_grid if est_cov is not None else None)
        self.n_depth += 1
        return self.n_depth - 1

    def result(self) -> EvaluationTables:
        """The single read-back: both tables and the grids in one device-to-host copy."""
        parts = [self._flow[:, :self.n_flow].reshape(-1).view(torch.int32), self._depth[:, :self.n_depth].reshape(-1).view(torch.int32),
                 self._flow_grids.reshape(-1), self._depth_grid.reshape(-1)]
        host = torch.cat(parts).cpu().numpy()
        sizes = [p.numel() for p in parts]
        o = np.cumsum([0] + sizes)
        f, d, fg, dg = (host[o[i]:o[i + 1]] for i in range(4))
        return EvaluationTables(
            flow=f.view(np.float32).reshape(self.lanes, self.n_flow, len(L.EVAL_FLOW_COLS)).copy(),
            depth=d.view(np.float32).reshape(self.lanes, self.n_depth, len(L.EVAL_DEPTH_COLS)).copy(),
            flow_grids=fg.view(np.uint32).reshape(self.lanes, 2, L.EVAL_GRID, L.EVAL_GRID).copy(),
            depth_grid=dg.view(np.uint32).reshape(self.lanes, L.EVAL_GRID, L.EVAL_GRID).copy())


# ------------------------------------------------------------------------------------------------ the reference's entry points
def _one_lane(t: torch.Tensor, planes: int, what: str) -> torch.Tensor:
    if t.dim() != 4 or t.shape[0] != 1 or t.shape[1] < planes:
        raise L.MacvoHipError(f"{what}: expected a [1,{planes},H,W] map (one frame per call, as the reference), got {tuple(t.shape)}")
    return t


def _flow_sequence(matcher, seq, max_flow: float, use_gt_mask: bool, with_cov: bool):
    """Shared loop of evaluate_flow / evaluate_flowcov: -> (EvaluationTables or None, [(prev frame_idx, frame_idx)])."""
    ev, prev, pairs = None, None, []
    for frame in seq:
        if prev is None:
            prev = frame
            continue
        assert prev.stereo.gt_flow is not None, "To evaluate flow quality, must use sequence with ground truth flow."
        out = matcher.estimate(prev.stereo, frame.stereo)
        est = _one_lane(out.flow, 2, "matcher flow")
        gt = prev.stereo.gt_flow.to(est.device)
        cov = None
        if with_cov:
            assert out.cov is not None
            cov = _one_lane(out.cov, 2, "matcher cov")
        if use_gt_mask:
            assert prev.stereo.flow_mask is not None
            valid = prev.stereo.flow_mask.to(est.device)
            # EvalFlow.py:104-105 ANDs the matcher's mask into the covariance evaluation's mask (there in place, on the frame's own tensor: not reproduced)
            if with_cov and out.mask is not None:
                valid = torch.logical_and(valid, out.mask.to(est.device))
        else:
            valid = None if out.mask is None else out.mask.to(est.device)
        if ev is None:
            ev = FrontendEvaluator(est.shape[2], est.shape[3], 1, est.device)
        ev.push_flow(est, gt, cov, valid, max_flow, apply_max_flow=not use_gt_mask)
        pairs.append((getattr(prev, "frame_idx", len(pairs)), getattr(frame, "frame_idx", len(pairs) + 1)))
        prev = frame
    return (None if ev is None else ev.result()), pairs


@torch.inference_mode()
def evaluate_flow(matcher, seq, max_flow: float, huge_epe_warn: float | None = None, use_gt_mask: bool = False) -> FlowPerformance:
    """EvalFlow.py:13-56.  ``huge_epe_warn`` reads the rows after the sequence (no per-frame synchronisation) and warns."""
    tables, pairs = _flow_sequence(matcher, seq, max_flow, use_gt_mask, with_cov=False)
    recs = [] if tables is None else tables.flow_records()
    results = [FlowPerformance(**{k: r[k] for k in ("masked_epe", "epe", "px1", "px3", "px5")}) for r in recs]
    if huge_epe_warn is not None:
        for (a, b), r in zip(pairs, results):
            if r.masked_epe > huge_epe_warn:
                warnings.warn(f"Flow {a}->{b} huge masked epe (> {huge_epe_warn}): epe={r.masked_epe}")
    return FlowPerformance.mean(results)


@torch.inference_mode()
def evaluate_flowcov(matcher, seq, max_flow: float, use_gt_mask: bool = False):
    """EvalFlow.py:59-135 -> (FlowCovPerformance, uint32 grids [2,100,100]: (error_u^2, cov_u) and (error_v^2, cov_v))."""
    assert matcher.provide_cov, f"Cannot evaluate covariance for {matcher} since no cov is provided by the module."
    tables, _ = _flow_sequence(matcher, seq, max_flow, use_gt_mask, with_cov=True)
    recs = [] if tables is None else tables.flow_records()
    results = [FlowCovPerformance(**{k: r[k] for k in ("masked_nll", "q25_nll", "q50_nll", "q75_nll")}) for r in recs]
    grids = np.zeros((2, L.EVAL_GRID, L.EVAL_GRID), np.uint32) if tables is None else tables.flow_grids[0]
    return FlowCovPerformance.mean(results), grids


def _depth_sequence(depth, seq, max_depth: float, with_cov: bool):
    ev, idx = None, []
    for frame in seq:
        assert frame.stereo.gt_depth is not None, "To evaluate depth quality, must use trajectory with gtDepth"
        out = depth.estimate(frame.stereo)
        est = _one_lane(out.depth, 1, "depth")
        cov = None
        if with_cov:
            assert out.cov is not None, "IStereoDepth implementation did not provide cov estimation as promised (via provide_cov API)"
            cov = _one_lane(out.cov, 1, "depth cov")
        if ev is None:
            ev = FrontendEvaluator(est.shape[2], est.shape[3], 1, est.device)
        ev.push_depth(est, frame.stereo.gt_depth.to(est.device), cov, max_depth)
        idx.append(getattr(frame, "frame_idx", len(idx)))
    return (None if ev is None else ev.result()), idx


@torch.inference_mode()
def evaluate_depth(depth, seq, max_depth: float = 80.0) -> DepthPerformance:
    """EvalDepth.py:12-39: per-field median over the frames; a frame with an empty mask is skipped with a warning (the reference's quantile raises
    there and its try / except drops the frame)."""
    tables, idx = _depth_sequence(depth, seq, max_depth, with_cov=False)
    return depth_performance([] if tables is None else tables.depth_records(), idx, max_depth)


def depth_performance(records: "list[dict]", frame_idx: list, max_depth: float) -> DepthPerformance:
    """The sequence reduction of ``evaluate_depth`` on read-back rows: frames with an empty mask are dropped with a warning, then the per-field median."""
    results = []
    for i, r in zip(frame_idx, records):
        if r["n_mask"] == 0:
            warnings.warn(f"Failed to evaluate depth performance at frame {i} - reason:\nno pixel below max_depth = {max_depth}")
            continue
        results.append(DepthPerformance(**{k: r[k] for k in ("masked_err", "err_25", "err_50", "err_75")}))
    return DepthPerformance.median(results)


@torch.inference_mode()
def evaluate_depthcov(depth, seq, max_depth: float = 80.0):
    """EvalDepth.py:42-88 -> (DepthCovPerformance, uint32 grid [100,100] of (error^2, cov))."""
    assert depth.provide_cov, f"Cannot evaluate covariance for {depth} since no cov is provided by the module."
    tables, _ = _depth_sequence(depth, seq, max_depth, with_cov=True)
    recs = [] if tables is None else tables.depth_records()
    results = [DepthCovPerformance(**{k: r[k] for k in ("masked_nll", "q25_nll", "q50_nll", "q75_nll")}) for r in recs]
    grid = np.zeros((L.EVAL_GRID, L.EVAL_GRID), np.uint32) if tables is None else tables.depth_grid[0]
    return DepthCovPerformance.mean(results), grid


# ------------------------------------------------------------------------------------------------ sequence metrics (MetricsSeq.py, EvalSeq.py)
# ATE / RTE / ROE / RPE of finished tracks through ``ops.eval_trajectory`` (one launch for every lane).  The reference hands these to evo 1.x; evo is
# not a dependency here, so its published definition is RESTATED and stays parity-UNPINNED (include/macvo_hip.h).  Tracks are
# ``[T, 7]`` rows (tx ty tz qx qy qz qw), already time-associated, or — what ``poses.npy`` holds — ``[T, 8]`` timed rows / :class:`Trajectory` objects,
# which first go through ``Trajectory.from_sandbox``'s steps on the GPU (``ops.associate_trajectory``: ``align_origin``, the clock rebase,
# ``align_time`` / ``interpolate_pose``, in fp64 with one rounding — the reference's mixed fp32 / fp64 PyPose chain is not reproduced bit for bit).
# ``align_scale``, ``align_SE3``, ``as_motion`` / ``MotionSequence``, plots, ``Sandbox`` config parsing and evo's ``is_so3`` exception are out of scope.
class TrajectoryEvaluationError(RuntimeError):
    """A lane that evo would have raised on: ``status`` is ``TOO_SHORT``, ``DEGENERATE`` or ``NONFINITE``."""

    def __init__(self, status: str):
        super().__init__(f"trajectory evaluation: {status}")
        self.status = status


@dataclass
class TrajectoryMetric:
    """What the reference reads of an ``evo`` result: ``stats["mean" | "std" | "rmse"]`` and ``np_arrays["error_array"]``."""
    stats: dict
    np_arrays: dict

    @property
    def error_array(self) -> np.ndarray:
        return self.np_arrays["error_array"]


_TRAJ_METRICS = ("ate", "rte", "roe", "rpe")


def _track(t, device) -> torch.Tensor:
    t = t if isinstance(t, torch.Tensor) else torch.tensor(np.asarray(t))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.double()
    return t.to(device)


class Trajectory:
    """``Utility/Trajectory.py:33-206`` on device tensors: ``poses`` ``[T, 7]`` (fp32 or fp64), ``time`` ``[T]`` (fp64 or int64), ``frame_status``
    ``[T]`` bool.  ``align_time`` / ``align_origin`` run ``ops.associate_trajectory`` (one launch, no synchronisation)."""

    def __init__(self, poses: torch.Tensor, time: torch.Tensor, frame_status: torch.Tensor | None = None):
        self.poses, self.time = poses, time.to(poses.device)
        self.frame_status = torch.zeros((poses.shape[0],), dtype=torch.bool, device=poses.device) if frame_status is None else frame_status.to(poses.device)

    def __getitem__(self, index) -> "Trajectory":
        return Trajectory(self.poses[index], self.time[index], self.frame_status[index])

    @classmethod
    def _untimed(cls, data, timestamp, frame_status, device) -> "Trajectory":
        poses = torch.tensor(np.asarray(data, dtype=float)).to(device)
        if timestamp is None:
            timestamp = torch.arange(0, poses.shape[0], step=1)
        assert frame_status is None or frame_status.dtype == torch.bool
        return cls(poses, timestamp, frame_status)

    @classmethod
    def _timed(cls, data, frame_status, device) -> "Trajectory":
        data = np.asarray(data, dtype=float)
        assert frame_status is None or frame_status.dtype == torch.bool
        return cls(torch.tensor(data[:, 1:]).to(device), torch.tensor(data[:, 0]), frame_status)

    @classmethod
    def from_SE3_txt(cls, file, timestamp=None, frame_status=None, device="cuda") -> "Trajectory":
        return cls._untimed(np.loadtxt(file), timestamp, frame_status, device)

    @classmethod
    def from_SE3_numpy(cls, file, timestamp=None, frame_status=None, device="cuda") -> "Trajectory":
        return cls._untimed(np.load(file).astype(float), timestamp, frame_status, device)

    @classmethod
    def from_timed_SE3_txt(cls, file, frame_status=None, device="cuda") -> "Trajectory":
        return cls._timed(np.loadtxt(file, dtype=float), frame_status, device)

    @classmethod
    def from_timed_SE3_numpy(cls, file, frame_status=None, device="cuda") -> "Trajectory":
        return cls._timed(np.load(file).astype(float), frame_status, device)

    @classmethod
    def from_pair(cls, est_rows8, gt_rows8, align_time: str | None = "est->gt", frame_status=None, device="cuda"):
        """The arithmetic of ``from_sandbox`` (Trajectory.py:103-116) on ``[T, 8]`` timed rows -> ``(gt, est)``: the estimate moved onto the reference's
        first pose, both clocks rebased, then ``align_time``."""
        est, gt = cls._timed(est_rows8, frame_status, device), cls._timed(gt_rows8, None, device)
        est = est.align_origin(gt)
        gt.time = gt.time - gt.time[0]
        est.time = est.time - est.time[0]
        if align_time == "est->gt":
            est = est.align_time(gt.time)
        elif align_time == "gt->est":
            gt = gt.align_time(est.time)
        else:
            assert align_time is None, align_time
        return gt, est

    @classmethod
    def from_sandbox(cls, folder, align_time: str | None = "est->gt", device="cuda"):
        """``Trajectory.from_sandbox`` for a result folder: ``poses.npy``, ``ref_poses.npy`` and the optional ``frame_status.pth`` -> ``(gt, est)``."""
        import os

        for f in ("poses.npy", "ref_poses.npy"):
            assert os.path.exists(os.path.join(folder, f)), f"Unable to load {f} from {folder}"
        flag = os.path.join(folder, "frame_status.pth")
        frame_status = torch.load(flag, weights_only=True) if os.path.exists(flag) else None
        return cls.from_pair(np.load(os.path.join(folder, "poses.npy")), np.load(os.path.join(folder, "ref_poses.npy")), align_time, frame_status, device)

    @property
    def length(self) -> int:
        return int(self.poses.shape[0])

    @property
    def translation(self) -> torch.Tensor:
        return self.poses[:, :3]

    @property
    def rotation(self) -> torch.Tensor:
        return self.poses[:, 3:7]

    def align_time(self, new_time: torch.Tensor) -> "Trajectory":
        """Trajectory.py:172-176: the poses interpolated at ``new_time`` (no rebase: the clocks are used as they are); ``frame_status`` becomes the
        ``extrapolated`` flag."""
        r = ops.associate_trajectory([self.poses], [self.time], [new_time], rebase=False)
        return Trajectory(r.poses[0], new_time, r.extrapolated[0].bool())

    def align_origin(self, ref: "Trajectory") -> "Trajectory":
        """Trajectory.py:188-191: every pose left-multiplied by ``ref_0 self_0^-1``, quaternions normalised with ``w >= 0``, cast to fp32 as
        ``from_evo`` does.  Runs as an association at the track's own stamps, all flagged as placements of the aligned rows."""
        if self.length == 0:
            return Trajectory(self.poses.float(), self.time, self.frame_status)
        # the track queried at its own row indices: the end rows are copies of the aligned rows, an interior row is Exp(Log(P_i P_i-1^-1)) P_i-1 — the
        # aligned row itself to fp64 rounding, far below the fp32 store
        idx = torch.arange(self.length, dtype=torch.float64, device=self.poses.device)
        r = ops.associate_trajectory([self.poses], [idx], [idx], origin_ref=[ref.poses[:1]], rebase=False, out_dtype=torch.float32)
        return Trajectory(r.poses[0], self.time, self.frame_status)

    def crop(self, from_idx: int | None = None, to_idx: int | None = None) -> "Trajectory":
        return Trajectory(self.poses[from_idx:to_idx], self.time[from_idx:to_idx], self.frame_status[from_idx:to_idx])

    def scale(self, s: float) -> "Trajectory":
        """Trajectory.py:200-203 (evo's ``scale``: the translation columns multiplied)."""
        poses = self.poses.clone()
        poses[:, :3] *= s
        return Trajectory(poses, self.time, self.frame_status)

    def __repr__(self) -> str:
        return f"Trajectory(length={self.length})"


def _timed_side(t, device):
    """-> (poses [T, 7], stamps [T] or None): a :class:`Trajectory`, ``[T, 8]`` timed rows (the stamp first, as ``poses.npy``) or an untimed ``[T, 7]`` track."""
    if isinstance(t, Trajectory):
        return t.poses.to(device), t.time.to(device)
    t = _track(t, device)
    if t.dim() == 2 and t.shape[1] == 8:
        return t[:, 1:], t[:, 0].contiguous()
    return t, None


def _timed_pairs(ests, gts, device):
    """Both sides of a launch -> (est, gt, est_time, gt_time); the stamps are None unless EVERY track of the launch carries some (then the launch does
    what EvalSeq.py:36 does first: origin, rebase, est->gt)."""
    e, g = [_timed_side(t, device) for t in ests], [_timed_side(t, device) for t in gts]
    timed = [a[1] is not None for a in e + g]
    if any(timed) and not all(timed):
        raise ValueError("trajectory evaluation: timed ([T, 8] rows / Trajectory) and untimed ([T, 7]) tracks cannot be mixed in one call")
    if not any(timed):
        return [a[0] for a in e], [a[0] for a in g], None, None
    return [a[0] for a in e], [a[0] for a in g], [a[1] for a in e], [a[1] for a in g]


def _one_dtype(tracks: list) -> list:
    """``mv_eval_traj_lanes`` takes one dtype per side: a side that mixes fp32 and fp64 is widened (exactly) to fp64."""
    return tracks if len({t.dtype for t in tracks}) <= 1 else [t.double() for t in tracks]


def _device_of(*tracks) -> torch.device:
    for t in tracks:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device("cuda:0")


def _evaluate_metric(which: int, gt, est, correct_scale: bool) -> TrajectoryMetric:
    dev = _device_of(*[x.poses if isinstance(x, Trajectory) else x for x in (est, gt)])
    e, g, te, tg = _timed_pairs([est], [gt], dev)
    res = ops.eval_trajectory(e, g, "umeyama", correct_scale, errors=True, est_time=te, ref_time=tg, align_origin=te is not None)
    row = res.rows[0].cpu().numpy()                                   # the read-back
    status = int(row[L.EVAL_TRAJ_COLS.index("status")])
    if status != L.MV_TRAJ_OK:
        raise TrajectoryEvaluationError(L.TRAJ_STATUS[status])
    n = res.lengths[0] - (0 if which == 0 else 1)
    stats = dict(zip(("mean", "std", "rmse"), map(float, row[3 * which:3 * which + 3])))
    return TrajectoryMetric(stats, {"error_array": res.errors[0, which, :n].cpu().numpy()})


def evaluateATE(gt_traj, est_traj, correct_scale: bool = False) -> TrajectoryMetric:
    """MetricsSeq.py:18-24 (``main_ape.ape``, translation part, Umeyama alignment), metres."""
    return _evaluate_metric(0, gt_traj, est_traj, correct_scale)


def evaluateRTE(gt_traj, est_traj, correct_scale: bool = False) -> TrajectoryMetric:
    """MetricsSeq.py:9-16 (``main_rpe.rpe``, translation part, delta = 1 frame), metres per frame."""
    return _evaluate_metric(1, gt_traj, est_traj, correct_scale)


def evaluateROE(gt_traj, est_traj, correct_scale: bool = False) -> TrajectoryMetric:
    """MetricsSeq.py:26-41 (``main_rpe.rpe``, rotation angle, delta = 1 frame), degrees per frame."""
    return _evaluate_metric(2, gt_traj, est_traj, correct_scale)


def evaluateRPE(gt_traj, est_traj, correct_scale: bool = False) -> TrajectoryMetric:
    """MetricsSeq.py:43-51 (``main_rpe.rpe``, full transformation, delta = 1 frame), unit-less."""
    return _evaluate_metric(3, gt_traj, est_traj, correct_scale)


def trajectory_header(correct_scale: bool = False) -> list:
    """EvalSeq.py:77-83."""
    dec = "[S]" if correct_scale else ""
    return ["Trajectory"] + [x for m in ("ATE", "RTE", "ROE", "RPE") for x in (f"μ_{m}{dec}", f"σ_{m}", f"RMSE_{m}")]


def trajectory_rows(names, rows: np.ndarray) -> list:
    """EvalSeq.py:35-76 on read-back rows (``[n, len(EVAL_TRAJ_COLS)]``; a name with a None row had no estimate): one row per track — 12 figures, or
    12 None where the status is not OK, which is where the reference's try / except lands — then the ``"Average"`` row over the figures present."""
    st = L.EVAL_TRAJ_COLS.index("status")
    out = []
    for name, r in zip(names, rows):
        ok = r is not None and int(r[st]) == L.MV_TRAJ_OK
        out.append([name] + ([float(x) for x in r[:12]] if ok else [None] * 12))
    out.append(["Average"] + [_mean([r[i] for r in out if r[i] is not None]) for i in range(1, 13)])
    return out


def EvaluateSequences(tracks, correct_scale: bool = False):
    """EvalSeq.py:26-83 for tracks held in memory: ``tracks`` is a list of ``(name, gt [T,7], est [T,7] or None)``; either side may instead be ``[T, 8]``
    timed rows (what ``poses.npy`` holds) or a :class:`Trajectory` — then every track of the call must be timed, and each launch first does what
    ``Trajectory.from_sandbox(..., align_time="est->gt")`` does (EvalSeq.py:36), still with one read-back per ``MV_MAX_LANES`` tracks.  All tracks are scored by one launch per
    ``MV_MAX_LANES`` of them and read back once (a side that mixes fp32 and fp64 tracks is widened to fp64 for that launch).  Returns the reference's ``(header, rows)``: a track without an estimate, or one evo would raise on,
    gives a row of None; the last row is ``"Average"`` (it raises ``ValueError`` when no track could be scored, as the reference's ``mean`` does)."""
    tracks = list(tracks)
    have = [i for i, (_, _, est) in enumerate(tracks) if est is not None]
    rows: list = [None] * len(tracks)
    if have:
        dev = _device_of(*[x.poses if isinstance(x, Trajectory) else x for i in have for x in tracks[i][1:]])
        parts = []
        for s in range(0, len(have), L.MV_MAX_LANES):
            idx = have[s:s + L.MV_MAX_LANES]
            e, g, te, tg = _timed_pairs([tracks[i][2] for i in idx], [tracks[i][1] for i in idx], dev)
            parts.append(ops.eval_trajectory(_one_dtype(e), _one_dtype(g), "umeyama", correct_scale, est_time=te, ref_time=tg,
                                             align_origin=te is not None).rows)
        host = torch.cat(parts).cpu().numpy()                         # the read-back
        for i, r in zip(have, host):
            rows[i] = r
    return trajectory_header(correct_scale), trajectory_rows([t[0] for t in tracks], rows)
