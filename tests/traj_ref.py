"""TEST INFRASTRUCTURE: the sequence metrics of ``Evaluation/MetricsSeq.py`` / ``Evaluation/EvalSeq.py`` restated in numpy fp64.

``MetricsSeq.py`` hands ATE / RTE / ROE / RPE to evo 1.x (``main_ape.ape`` / ``main_rpe.rpe`` with ``align=True, align_origin=True``).  evo is not
importable here, so this is a RESTATEMENT of evo's published code, UNPINNED: no evo run stands behind it.  It follows the definition literally —
4 x 4 matrices, ``numpy.linalg.svd``, scipy's ``Rotation`` for the angle, every pose transformed by the alignment before the relative errors are
taken — and raises where evo raises.  The kernel (``csrc/traj_eval.hip``) and its host twin are compared with it.

Out of scope, as for the kernel: ``Trajectory.from_sandbox``'s time association (``align_time`` -> ``interpolate_pose`` in fp32 PyPose arithmetic),
the fp32 round trip of its ``align_origin``, sandbox loading, plots, and evo's ``is_so3`` exception."""
from __future__ import annotations

import numpy as np
from scipy.spatial.transform import Rotation

EPS = float(np.finfo(np.float64).eps)
STATS = ("mean", "std", "rmse")
METRICS = ("ate", "rte", "roe", "rpe")


class TooShort(Exception):
    """evo finds no pairs for T < 2 and raises."""


class Degenerate(Exception):
    """evo's GeometryException("Degenerate covariance rank, Umeyama alignment is not possible")."""


class NonFinite(Exception):
    """A NaN / inf coordinate: our own case, the reference never sees it."""


def quaternion_matrix(q_wxyz: np.ndarray) -> np.ndarray:
    """evo.core.transformations.quaternion_matrix (3 x 3 part)."""
    q = np.array(q_wxyz, dtype=np.float64)
    n = float(np.dot(q, q))
    if n < 4.0 * EPS:
        return np.eye(3)
    q = q * np.sqrt(2.0 / n)
    q = np.outer(q, q)
    return np.array([[1.0 - q[2, 2] - q[3, 3], q[1, 2] - q[3, 0], q[1, 3] + q[2, 0]],
                     [q[1, 2] + q[3, 0], 1.0 - q[1, 1] - q[3, 3], q[2, 3] - q[1, 0]],
                     [q[1, 3] - q[2, 0], q[2, 3] + q[1, 0], 1.0 - q[1, 1] - q[2, 2]]])


def poses_se3(track: np.ndarray) -> np.ndarray:
    """``[T, 7]`` rows (tx ty tz qx qy qz qw) -> ``[T, 4, 4]``."""
    track = np.asarray(track, dtype=np.float64)
    out = np.tile(np.eye(4), (track.shape[0], 1, 1))
    for i, r in enumerate(track):
        out[i, :3, :3] = quaternion_matrix(np.array([r[6], r[3], r[4], r[5]]))
        out[i, :3, 3] = r[:3]
    return out


def umeyama(x: np.ndarray, y: np.ndarray, with_scale: bool):
    """evo.core.geometry.umeyama_alignment on ``[T, 3]`` positions (x = estimate, y = reference) -> (R, t, c, d)."""
    n = x.shape[0]
    mu_x, mu_y = x.mean(axis=0), y.mean(axis=0)
    sigma_x = (1.0 / n) * float((np.linalg.norm(x - mu_x, axis=1) ** 2).sum())
    cov = (1.0 / n) * np.einsum("ni,nj->ij", y - mu_y, x - mu_x)
    u, d, v = np.linalg.svd(cov)
    if np.count_nonzero(d > EPS) < 2:
        raise Degenerate(f"d = {d}")
    s = np.eye(3)
    if np.linalg.det(u) * np.linalg.det(v) < 0.0:
        s[2, 2] = -1.0
    r = u @ s @ v
    c = float(np.trace(np.diag(d) @ s) / sigma_x) if with_scale else 1.0
    t = mu_y - c * (r @ mu_x)
    return r, t, c, d


def singular_values(est: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """d of the centred covariance alone (the tests' conditions on their own inputs)."""
    x, y = np.asarray(est, np.float64)[:, :3], np.asarray(ref, np.float64)[:, :3]
    cov = (1.0 / x.shape[0]) * np.einsum("ni,nj->ij", y - y.mean(axis=0), x - x.mean(axis=0))
    return np.linalg.svd(cov, compute_uv=False)


def _stats(e: np.ndarray) -> dict:
    return {"mean": float(np.mean(e)), "std": float(np.std(e)), "rmse": float(np.sqrt(np.mean(np.power(e, 2))))}


def evaluate(est: np.ndarray, ref: np.ndarray, align: str = "umeyama", correct_scale: bool = False) -> dict:
    """-> {"ate": [T], "rte" / "roe" / "rpe": [T - 1], "stats": {metric: {mean, std, rmse}}, "R", "t", "c", "d"}.  Raises TooShort / NonFinite /
    Degenerate.  ``origin`` / ``none`` with ``correct_scale`` scale by Umeyama's c first (evo's ``only_scale``)."""
    est, ref = np.asarray(est, np.float64)[:, :7], np.asarray(ref, np.float64)[:, :7]
    assert est.shape == ref.shape, "time-associated tracks: one estimate row per reference row"
    T = est.shape[0]
    if T < 2:
        raise TooShort(T)
    if not (np.isfinite(est).all() and np.isfinite(ref).all()):
        raise NonFinite()
    P, Q = poses_se3(est), poses_se3(ref)
    R, t, c, d = np.eye(3), np.zeros(3), 1.0, np.full(3, np.nan)
    if align == "umeyama" or correct_scale:
        Ru, tu, c, d = umeyama(est[:, :3], ref[:, :3], correct_scale)
        P[:, :3, 3] *= c                                    # PosePath3D.scale
        if align == "umeyama":
            R, t = Ru, tu
    if align == "origin":
        A0 = Q[0] @ np.linalg.inv(P[0])                     # PosePath3D.align_origin
        R, t = A0[:3, :3], A0[:3, 3]
    elif align not in ("umeyama", "none"):
        raise ValueError(align)
    A = np.eye(4)
    A[:3, :3], A[:3, 3] = R, t
    P = np.einsum("ij,njk->nik", A, P)                      # PosePath3D.transform (left-multiplied)
    ate = np.linalg.norm(P[:, :3, 3] - Q[:, :3, 3], axis=1)
    rte, roe, rpe = np.zeros(T - 1), np.zeros(T - 1), np.zeros(T - 1)
    for i in range(T - 1):
        q_rel = np.linalg.inv(Q[i]) @ Q[i + 1]
        p_rel = np.linalg.inv(P[i]) @ P[i + 1]
        E = np.linalg.inv(q_rel) @ p_rel
        rte[i] = np.linalg.norm(E[:3, 3])
        roe[i] = np.degrees(np.linalg.norm(Rotation.from_matrix(E[:3, :3]).as_rotvec()))
        rpe[i] = np.linalg.norm(E - np.eye(4))
    out = {"ate": ate, "rte": rte, "roe": roe, "rpe": rpe, "R": R, "t": t, "c": c, "d": d}
    out["stats"] = {m: _stats(out[m]) for m in METRICS}
    return out


def status_of(est, ref, align: str = "umeyama", correct_scale: bool = False) -> str:
    try:
        evaluate(est, ref, align, correct_scale)
    except TooShort:
        return "TOO_SHORT"
    except NonFinite:
        return "NONFINITE"
    except Degenerate:
        return "DEGENERATE"
    return "OK"


def stats_row(res: dict) -> list:
    """The 12 figures in ``EvalSeq.py:60-63`` order."""
    return [res["stats"][m][s] for m in METRICS for s in STATS]


# ------------------------------------------------------------------------------------------------ the tests' track generators (seeded, CPU)
def quat_mul(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Hamilton product of (x y z w) quaternions."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def random_walk(T: int, seed: int, step: float = 0.3, rot_step: float = 0.03, planar: bool = False) -> np.ndarray:
    """``[T, 7]`` fp64: body-frame steps of about ``step`` metres forward and ``rot_step`` rad.  ``planar``: z and the roll / pitch steps are exactly 0."""
    g = np.random.default_rng(seed)
    out = np.zeros((T, 7))
    p, q = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])
    for i in range(T):
        out[i, :3], out[i, 3:] = p, q
        w = g.normal(size=3) * rot_step
        v = np.array([step, 0.0, 0.0]) + g.normal(size=3) * 0.1 * step
        if planar:
            w[0] = w[1] = 0.0
            v[2] = 0.0
        p = p + Rotation.from_quat(q).apply(v)
        if planar:
            p[2] = 0.0
        q = quat_mul(q, Rotation.from_rotvec(w).as_quat())
        q = q / np.linalg.norm(q)
        if planar:
            q[0] = q[1] = 0.0
    return out


def perturb(ref: np.ndarray, seed: int, trans: float = 0.01, rot: float = 0.002, planar: bool = False) -> np.ndarray:
    """An estimate: the reference's own relative motions, each with a seeded perturbation (metres / rad per step), chained from the first pose."""
    g = np.random.default_rng(seed)
    T = ref.shape[0]
    out = np.zeros_like(ref)
    if T == 0:
        return out
    out[0] = ref[0]
    for i in range(1, T):
        r0 = Rotation.from_quat(ref[i - 1, 3:])
        dv = r0.inv().apply(ref[i, :3] - ref[i - 1, :3]) + g.normal(size=3) * trans
        dq = (r0.inv() * Rotation.from_quat(ref[i, 3:])).as_quat()
        w = g.normal(size=3) * rot
        if planar:
            w[0] = w[1] = 0.0
            dv[2] = 0.0
        q0 = out[i - 1, 3:]
        out[i, :3] = out[i - 1, :3] + Rotation.from_quat(q0).apply(dv)
        q = quat_mul(quat_mul(q0, dq), Rotation.from_rotvec(w).as_quat())
        q = q / np.linalg.norm(q)
        if planar:
            out[i, 2] = 0.0
            q[0] = q[1] = 0.0
        out[i, 3:] = q
    return out


def rigid(track: np.ndarray, rotvec, trans) -> np.ndarray:
    """Left-multiply every pose by a fixed rigid transform."""
    r = Rotation.from_rotvec(rotvec)
    out = np.array(track, dtype=np.float64)
    out[:, :3] = r.apply(track[:, :3]) + np.asarray(trans)
    qa = r.as_quat()
    for i in range(track.shape[0]):
        out[i, 3:] = quat_mul(qa, track[i, 3:])
    return out
