"""Frontend evaluation on the GPU: the reference's ``Evaluation/EvalFlow.py`` and ``Evaluation/EvalDepth.py``.

Two ways to call it:

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
