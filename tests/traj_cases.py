"""TEST INFRASTRUCTURE: the input cases of the trajectory-evaluation tests (CPU twin and GPU kernel share them) and the error measure both use.

Tracks are seeded random walks (step about 0.3 m, rotation step about 0.03 rad; ``tests.traj_ref.random_walk``) with an estimate made by a seeded
per-step perturbation, plus the fixture ``tests/golden/traj_eval.npz``.  Everything is built once, on the CPU, and never modified."""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass, field

import numpy as np

from tests import traj_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKGROUP = 256                                                  # traj::THREADS (csrc/traj_math.h); test_traj_eval_host.py checks the header says so
LENGTHS = (3, 4, 63, 64, 65, 255, 256, 257, 1360)                # 255 / 257 are workgroup size -+ 1
OFFSET = 1.0e4
MODES = ("umeyama", "origin", "none")


@dataclass
class Case:
    name: str
    est: np.ndarray
    ref: np.ndarray
    align: str = "umeyama"
    correct_scale: bool = False
    status: str = "OK"
    scale: float | None = None          # the offset case: every tolerance relative to this distance
    same_as: str | None = None          # an encoding of another case that must give the IDENTICAL row
    extra: dict = field(default_factory=dict)


@functools.lru_cache(maxsize=None)
def golden() -> dict:
    g = np.load(os.path.join(ROOT, "tests", "golden", "traj_eval.npz"))
    return {k: g[k] for k in g.files}


def _pair(T: int, seed: int, planar: bool = False):
    ref = TR.random_walk(T, seed, planar=planar)
    return TR.perturb(ref, seed + 1000, planar=planar), ref


@functools.lru_cache(maxsize=None)
def cases() -> "dict[str, Case]":
    out: dict = {}

    def add(c: Case):
        assert c.name not in out
        c.est.setflags(write=False)
        c.ref.setflags(write=False)
        out[c.name] = c

    g = golden()
    # lengths
    for T in LENGTHS:
        est, ref = (g["est"].copy(), g["gt"].copy()) if T == 1360 else _pair(T, T)
        add(Case(f"len{T}", est, ref))
    # the fixture and a generic track in every mode, with and without scale
    for name, (est, ref) in (("fixture", (g["est"], g["gt"])), ("generic", _pair(200, 7))):
        for mode in MODES:
            for sc in (False, True):
                add(Case(f"{name}_{mode}_{int(sc)}", est.copy(), ref.copy(), mode, sc))
    # geometry
    est, ref = _pair(200, 11, planar=True)
    assert np.all(est[:, 2] == 0) and np.all(ref[:, 2] == 0) and np.all(est[:, 3:5] == 0) and np.all(ref[:, 3:5] == 0)
    add(Case("planar", est, ref))
    add(Case("planar_scale", est.copy(), ref.copy(), correct_scale=True))
    est, ref = _pair(200, 13)
    m = est.copy()
    m[:, 2] = -m[:, 2]
    add(Case("mirrored", m, ref))
    add(Case("mirrored_scale", m.copy(), ref.copy(), correct_scale=True))
    est, ref = _pair(200, 17)
    off = np.array([0.6, -0.64, 0.48]) * OFFSET                  # a unit direction times the offset
    eo, ro = est.copy(), ref.copy()
    eo[:, :3] += off
    ro[:, :3] += off
    for mode in MODES:
        add(Case(f"offset_{mode}", eo.copy(), ro.copy(), mode, scale=OFFSET))
    add(Case("offset_scale", eo.copy(), ro.copy(), correct_scale=True, scale=OFFSET))
    es = est.copy()
    es[:, :3] *= 0.5
    add(Case("scaled_noscale", es, ref.copy()))
    add(Case("scaled_scale", es.copy(), ref.copy(), correct_scale=True))
    # encoding
    est, ref = _pair(130, 19)
    e32, r32 = est.astype(np.float32), ref.astype(np.float32)
    add(Case("f64_f64", est, ref))
    add(Case("f32_f32", e32, r32))
    add(Case("f32_f64", e32.copy(), ref.copy()))
    add(Case("f64_f32", est.copy(), r32.copy()))
    for k, tag in ((0.5, "half"), (2.0, "double")):               # a power of two: the scaled quaternion normalises to the same bits
        e2, r2 = est.copy(), ref.copy()
        e2[:, 3:] *= k
        r2[:, 3:] *= k
        add(Case(f"quat_{tag}", e2, r2, same_as="f64_f64"))
    e2, r2 = est.copy(), ref.copy()
    e2[::2, 3:] *= -1.0
    r2[1::2, 3:] *= -1.0
    add(Case("quat_negated", e2, r2, same_as="f64_f64"))
    e9 = np.full((130, 9), 1.0e30)                                # a [T, 9] table: a row stride that is not 7; the two spare columns must not be read
    e9[:, :7] = est
    r11 = np.full((130, 11), -1.0e30, np.float32)
    r11[:, :7] = r32
    add(Case("stride", e9, r11, same_as="f64_f32"))
    # status
    est, ref = _pair(40, 23)
    add(Case("T0", est[:0].copy(), ref[:0].copy(), status="TOO_SHORT"))
    add(Case("T1", est[:1].copy(), ref[:1].copy(), status="TOO_SHORT"))
    add(Case("T2", est[:2].copy(), ref[:2].copy(), status="DEGENERATE"))
    add(Case("T2_origin", est[:2].copy(), ref[:2].copy(), "origin"))                # no Umeyama: two poses are enough
    add(Case("T2_none_scale", est[:2].copy(), ref[:2].copy(), "none", True, status="DEGENERATE"))
    line_r = np.zeros((10, 7))
    line_r[:, 0] = np.arange(10) * 0.25
    line_r[:, 6] = 1.0
    line_e = line_r.copy()
    line_e[:, 0] = np.arange(10) * 0.26 + 0.125
    add(Case("line_x", line_e, line_r, status="DEGENERATE"))
    for col, bad, tag in ((1, np.nan, "nan"), (5, np.inf, "inf"), (0, -np.inf, "ninf")):
        e2 = est.copy()
        e2[17, col] = bad
        add(Case(f"nonfinite_{tag}", e2, ref.copy(), status="NONFINITE"))
    r2 = ref.copy()
    r2[39, 6] = np.nan
    add(Case("nonfinite_ref", est.copy(), r2, status="NONFINITE"))
    return out


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """The restatement's result for a case (computed once, shared): a dict, or the status name where it raises."""
    c = cases()[name]
    try:
        return TR.evaluate(c.est, c.ref, c.align, c.correct_scale)
    except TR.TooShort:
        return "TOO_SHORT"
    except TR.NonFinite:
        return "NONFINITE"
    except TR.Degenerate:
        return "DEGENERATE"


def extent(c: Case) -> float:
    """The track's extent: the diagonal of the reference positions' bounding box."""
    p = np.asarray(c.ref, np.float64)[:, :3]
    return float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))


def worst_error(c: Case, res: dict, row: np.ndarray, err: np.ndarray | None) -> dict:
    """|got - ref| / s per group.  s: the track's extent for ATE (values and statistics) and for t; for RTE / ROE / RPE the ratio's own denominator
    max(|ref|, 1e-12); 1 for R and c (unit scale); max(d_1, 1e-12) for d; for an offset case the offset distance throughout."""
    from macvo_amd import _lib as L

    col = {n: i for i, n in enumerate(L.EVAL_TRAJ_COLS)}
    ext = c.scale if c.scale is not None else extent(c)
    out = {}

    def rel(got, ref, s=None):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        den = np.maximum(np.abs(ref), 1e-12) if s is None else s
        if c.scale is not None:
            den = c.scale
        return float(np.max(np.abs(got - ref) / den)) if got.size else 0.0

    for k, m in enumerate(TR.METRICS):
        stats = [res["stats"][m][s] for s in TR.STATS]
        out[m + "_stats"] = rel(row[3 * k:3 * k + 3], stats, ext if m == "ate" else None)
        if err is not None:
            n = len(res[m])
            out[m + "_values"] = rel(err[k, :n], res[m], ext if m == "ate" else None)
    out["R"] = rel(row[col["r00"]:col["r22"] + 1], res["R"].reshape(-1), 1.0)
    out["t"] = rel(row[col["tx"]:col["tz"] + 1], res["t"], max(ext, 1.0))
    out["c"] = rel(row[col["scale"]], res["c"], 1.0)
    if not np.isnan(res["d"]).any():
        out["d"] = rel(row[col["d1"]:col["d3"] + 1], res["d"], max(float(res["d"][0]), 1e-12))
    else:       # ORIGIN / NONE without scale: no Umeyama, no singular values on either side
        assert np.isnan(res["d"]).all() and np.isnan(row[col["d1"]:col["d3"] + 1]).all(), (c.name, row[col["d1"]:col["d3"] + 1])
    return out


EPS = float(np.finfo(np.float64).eps)


def check_conditions() -> None:
    """The conditions on the inputs, asserted with the restatement alone (a borderline track must not hide a failure): every case has the status it
    is listed with; where Umeyama must work d_2 > 1e-6, where it must not d_2 < DBL_EPSILON; the planar track has d_3 = 0 exactly; the mirrored one
    takes the S[2][2] = -1 branch with d_2 >= 2 d_3 (R is unique there); the fixture is well-posed.  No case is left out."""
    for name, c in cases().items():
        ref = reference(name)
        assert (ref if isinstance(ref, str) else "OK") == c.status, name
        if c.est.shape[0] < 2 or c.status == "NONFINITE":
            continue
        d = TR.singular_values(c.est, c.ref)
        if c.status == "DEGENERATE":
            assert d[1] < EPS, (name, d)
        elif c.align == "umeyama" or c.correct_scale:
            assert d[1] > 1e-6, (name, d)
    c = cases()["planar"]
    assert TR.singular_values(c.est, c.ref)[2] == 0.0
    c = cases()["mirrored"]
    x, y = c.est[:, :3] - c.est[:, :3].mean(0), c.ref[:, :3] - c.ref[:, :3].mean(0)
    u, d, v = np.linalg.svd(y.T @ x / len(x))
    assert np.linalg.det(u) * np.linalg.det(v) < 0 and d[1] >= 2 * d[2], d
    g = golden()
    assert g["gt"].shape == (1360, 7) and g["est"].shape == (1360, 7)
    d = TR.singular_values(g["est"], g["gt"])
    assert d[0] > 50 and d[1] > 30 and d[2] > 2, d
