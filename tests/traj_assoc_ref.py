"""TEST INFRASTRUCTURE: the restatement of the trajectory association step — ``Trajectory.from_sandbox``'s ``align_origin``, clock rebase and
``align_time`` (Utility/Trajectory.py:105-114, 172-176, 188-191) over ``interpolate_pose`` (Utility/Math.py:96-121) — and of
``PoseInterpolate.elaborate_map`` (Module/MapProcessor.py:33-45), in numpy / torch on ``oracle.se3`` (PyPose restated; imported read-only).

Two forms:
  ``ref64``      the semantics of ``mv_traj_associate_lanes`` in fp64 throughout;
  ``ref_chain``  the reference's own precision chain for an fp32 estimate: fp32 ``Inv`` / ``@`` / ``Log``, an fp64 ``Exp`` (the fp64 proportion promotes
                 the tangent), fp32 again after ``.to(P_seg_start)``, and fp32 poses after ``from_evo(...).float()`` where the origin is aligned.
UNPINNED: neither PyPose nor evo is importable, no run of either stands behind these figures."""
from __future__ import annotations

import numpy as np
import torch

from oracle import se3

STATUS = ("OK", "TOO_SHORT", "DEGENERATE", "NONFINITE", "UNSORTED")


def rebased(stamps: np.ndarray, rebase: bool = True) -> np.ndarray:
    """A clock as fp64.  int64 stamps are subtracted as integers, only the difference is converted; fp64 stamps are subtracted in fp64."""
    stamps = np.asarray(stamps)
    if stamps.size == 0:
        return stamps.astype(np.float64)
    if stamps.dtype == np.int64:
        return (stamps - stamps[0]).astype(np.float64) if rebase else stamps.astype(np.float64)
    return stamps - stamps[0] if rebase else stamps.astype(np.float64)


def _normq(p: torch.Tensor) -> torch.Tensor:
    return torch.cat([p[..., :3], p[..., 3:] / p[..., 3:].norm(dim=-1, keepdim=True)], dim=-1)


def align_origin(src: torch.Tensor, ref0: torch.Tensor) -> torch.Tensor:
    """evo's ``align_origin`` (restated): every pose left-multiplied by ``ref_0 src_0^-1``; the quaternion normalised, ``w >= 0``."""
    src = _normq(src)
    A = se3.se3_mul(_normq(ref0), se3.se3_inv(src[0]))
    out = _normq(se3.se3_mul(A.expand_as(src), src))
    out[:, 3:] = torch.where(out[:, 6:7] < 0, -out[:, 3:], out[:, 3:])
    return out


def status_of(src: np.ndarray, ts: np.ndarray, tq: np.ndarray, origin) -> str:
    if src.shape[0] == 0:
        return "TOO_SHORT"
    if not (np.isfinite(ts).all() and np.isfinite(tq).all() and np.isfinite(src[:, :7]).all() and (origin is None or np.isfinite(origin[:7]).all())):
        return "NONFINITE"
    if not (ts[:-1] < ts[1:]).all():                                  # Math.py:97
        return "UNSORTED"
    return "OK"


def _place(P: torch.Tensor, ts: np.ndarray, tq: np.ndarray, interp):
    """Math.py:99-121 on prepared poses: copies at and beyond both ends, ``interp(Ps, Pe, prop)`` between."""
    out = torch.empty((len(tq), 7), dtype=P.dtype)
    before, after = tq <= ts[0], tq >= ts[-1]
    mid = ~(before | after)
    out[torch.from_numpy(before)] = P[0]
    out[torch.from_numpy(after & ~before)] = P[-1]
    if mid.any():
        e = np.searchsorted(ts, tq[mid], side="left")
        s = e - 1
        prop = (tq[mid] - ts[s]) / (ts[e] - ts[s])
        out[torch.from_numpy(mid)] = interp(P[s], P[e], torch.from_numpy(prop))
    return out, (~mid).astype(np.uint8)


def _interp64(Ps, Pe, prop):
    xi = se3.se3_log(se3.se3_mul(Pe, se3.se3_inv(Ps)))
    return se3.se3_mul(se3.se3_exp(prop.unsqueeze(-1) * xi), Ps)


def ref64(src: np.ndarray, ts: np.ndarray, tq: np.ndarray, origin: np.ndarray | None = None, rebase: bool = True):
    """-> (poses fp64 ``[Q, 7]``, extrapolated uint8 ``[Q]``, status name).  A lane that is not OK: NaN poses, flags 0."""
    src = np.asarray(src)
    ts, tq = rebased(ts, rebase), rebased(tq, rebase)
    st = status_of(src, ts, tq, origin)
    if st != "OK":
        return np.full((len(tq), 7), np.nan), np.zeros(len(tq), np.uint8), st
    P = torch.from_numpy(np.array(src[:, :7], np.float64))
    if origin is not None:
        P = align_origin(P, torch.from_numpy(np.array(origin[:7], np.float64)))
    out, flag = _place(P, ts, tq, _interp64)
    return out.numpy(), flag, st


def ref_chain(src32: np.ndarray, ts: np.ndarray, tq: np.ndarray, origin: np.ndarray | None = None, rebase: bool = True):
    """The reference's chain for an fp32 estimate -> (poses fp32 ``[Q, 7]``, extrapolated)."""
    assert src32.dtype == np.float32
    ts, tq = rebased(ts, rebase), rebased(tq, rebase)
    P = torch.from_numpy(np.array(src32[:, :7]))
    if origin is not None:                                            # evo works on fp64 matrices; from_evo(...).float()
        P = align_origin(P.double(), torch.from_numpy(np.array(origin[:7], np.float64))).float()

    def interp(Ps, Pe, prop):
        xi = se3.se3_log(se3.se3_mul(Pe, se3.se3_inv(Ps)))            # fp32
        return se3.se3_mul(se3.se3_exp(prop.unsqueeze(-1) * xi).float(), Ps)   # fp64 Exp, .to(P_seg_start), fp32 @

    out, flag = _place(P, ts, tq, interp)
    return out.numpy(), flag


def pose_interpolate(pose32: np.ndarray, need_interp: np.ndarray):
    """``PoseInterpolate.elaborate_map`` in fp64 on the widened fp32 table -> (poses fp64 ``[T, 7]`` — good rows are the input's —, need_interp after the
    edge flags were cleared, mask of rewritten rows).  prop is the float32 division of Math.py:114 (int64 / int64 in torch's default dtype)."""
    P = torch.from_numpy(np.array(pose32, np.float32)).double()
    bad = np.array(need_interp, np.uint8) != 0
    bad[:5] = False
    bad[-5:] = False
    out = P.clone()
    good = np.nonzero(~bad)[0]
    idx = np.nonzero(bad)[0]
    if len(idx):
        e = np.searchsorted(good, idx, side="left")
        s_i, e_i = good[e - 1], good[e]
        prop = (torch.from_numpy(idx - s_i) / torch.from_numpy(e_i - s_i)).double()
        assert (torch.from_numpy(idx - s_i) / torch.from_numpy(e_i - s_i)).dtype == torch.float32
        out[idx] = _interp64(P[s_i], P[e_i], prop)
    return out.numpy(), bad.astype(np.uint8), bad.astype(np.uint8)


def max_segment_angle(src: np.ndarray) -> float:
    """The largest rotation between consecutive source poses, radians."""
    P = torch.from_numpy(np.array(src[:, :7], np.float64))
    if P.shape[0] < 2:
        return 0.0
    d = se3.quat_mul(P[1:, 3:], se3.quat_inv(P[:-1, 3:]))
    d = d / d.norm(dim=-1, keepdim=True)
    return float((2 * torch.atan2(d[:, :3].norm(dim=-1), d[:, 3].abs())).max())
