"""CPU: the ground the GPU tests of tests/test_gpu_traj_eval.py stand on.

(a) tests/traj_ref.py — the restatement of evo's definition that Evaluation/MetricsSeq.py calls (UNPINNED: evo is not importable) — against things it
    did not come from: oracle.metrics.relative_errors, scipy's Kabsch (Rotation.align_vectors), invariance under a rigid transform of the estimate,
    and zero error for a rigidly moved copy of the reference;
(b) the kernel's host twin (tests/c_abi/traj_twin.cpp on the kernel's own csrc/traj_math.h, in the kernel's reduction order) against the
    restatement on every case of tests/traj_cases.py: the Jacobi SVD, the reflection branch, the degenerate rule, the status precedence;
(c) the header, the _lib table and the built library agree on the new symbol; the ABI stays 8."""
import os
import re

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from tests import traj_cases as TC
from tests import traj_ref as TR
from tests import traj_twin as TW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)
OK_CASES = [n for n, c in TC.cases().items() if c.status == "OK"]
BAD_CASES = [n for n, c in TC.cases().items() if c.status != "OK"]
# twin against restatement, |twin - ref| / s (tests/traj_cases.worst_error).  Both are fp64 throughout and differ in the SVD (Jacobi / LAPACK), the
# angle (atan2 of the antisymmetric part / scipy's quaternion route) and the order of sums: differences of a few hundred ulp of the largest
# intermediate.  The restatement's own noise — the same track moved rigidly — is up to 2e-12 on the same measure (test (a) below); 50 x that, and a
# tenth of the 1e-9 cap the GPU tests may never exceed.
TWIN_BOUND = 1e-10


# ---------------------------------------------------------------------------------------------------------------------------- conditions on the inputs
def test_cases_satisfy_their_conditions():
    """Asserted with the restatement alone: a borderline track must not hide a failure (tests/traj_cases.check_conditions; the GPU file runs it too)."""
    TC.check_conditions()


def test_golden_rows_are_the_restatement():
    g = TC.golden()
    for mode in TC.MODES:
        for sc in (0, 1):
            res = TC.reference(f"fixture_{mode}_{sc}")
            np.testing.assert_allclose(TR.stats_row(res), g[f"rows_{mode}_{sc}"], rtol=1e-12, atol=0)
    assert TC.WORKGROUP == int(re.search(r"constexpr int THREADS = (\d+);", open(os.path.join(ROOT, "mac-vo_amd", "csrc", "traj_math.h")).read()).group(1))


# ---------------------------------------------------------------------------------------------------------------------------- (a) the restatement
@pytest.mark.parametrize("name", ["generic_none_0", "fixture_none_0", "len65", "planar", "f64_f64"])
def test_ref_relative_errors_match_oracle(name):
    from oracle import metrics

    c = TC.cases()[name]
    res = TR.evaluate(c.est, c.ref, "none", False)

    def unit(track):      # the oracle takes unit quaternions as given; evo normalises (the fixture's are fp32 values, unit to 1e-7 only)
        t = np.array(track, dtype=np.float64)
        t[:, 3:] /= np.linalg.norm(t[:, 3:], axis=1, keepdims=True)
        return torch.from_numpy(t)

    rte, roe = metrics.relative_errors(unit(c.ref), unit(c.est))
    np.testing.assert_allclose(res["rte"], rte.numpy(), rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(np.radians(res["roe"]), roe.numpy(), rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize("name", [n for n in OK_CASES if TC.cases()[n].align == "umeyama"])
def test_ref_rotation_is_kabsch(name):
    c = TC.cases()[name]
    res = TC.reference(name)
    x, y = np.asarray(c.est, np.float64)[:, :3], np.asarray(c.ref, np.float64)[:, :3]
    rot, _ = Rotation.align_vectors(y - y.mean(0), x - x.mean(0))
    assert np.abs(rot.as_matrix() - res["R"]).max() <= 1e-13, name


@pytest.mark.parametrize("name", ["generic_umeyama_0", "generic_umeyama_1", "fixture_umeyama_0", "planar", "len3", "len257"])
def test_ref_invariant_under_rigid_transform_of_estimate(name):
    c = TC.cases()[name]
    base = TC.reference(name)
    moved = TR.evaluate(TR.rigid(c.est, [0.3, -1.1, 0.7], [12.0, -7.0, 3.0]), c.ref, c.align, c.correct_scale)
    # The restatement is literal: it moves every pose by the alignment and only then differences neighbours.  A coordinate of magnitude M carries a
    # rounding of eps * M, M <= the track's extent + the shift (rotation entries: M = 1, in degrees 57.3), and an error value is a short chain of such
    # differences: 64 roundings are allowed.  Against the values themselves (RTE of millimetres on a 60 m track) that is 1e-11 relative; ATE is
    # measured against the extent, where it is below 2e-12.
    reach = TC.extent(c) + float(np.linalg.norm([12.0, -7.0, 3.0]))
    worst = {m: float(np.max(np.abs(moved[m] - base[m]))) for m in TR.METRICS}
    print(name, worst, "relative:", {m: float(np.max(np.abs(moved[m] - base[m]) / np.maximum(np.abs(base[m]), 1e-12))) for m in TR.METRICS})
    assert worst["ate"] / TC.extent(c) <= 2e-12 and worst["rte"] <= 64 * EPS * reach and worst["rpe"] <= 64 * EPS * reach, (name, worst)
    assert worst["roe"] <= 64 * EPS * np.degrees(1.0), (name, worst)


@pytest.mark.parametrize("name", ["generic_umeyama_0", "fixture_umeyama_0", "planar", "len4"])
def test_ref_rigid_copy_of_reference_has_no_error(name):
    c = TC.cases()[name]
    res = TR.evaluate(TR.rigid(np.asarray(c.ref, np.float64)[:, :7], [-0.4, 0.2, 2.0], [5.0, 6.0, -7.0]), c.ref, "umeyama", False)
    worst = {m: float(np.max(res[m])) for m in TR.METRICS}          # metres, metres, degrees, unit-less: 1e-12 absolute on each
    print(name, worst)
    assert max(worst.values()) <= 1e-12, (name, worst)


# ---------------------------------------------------------------------------------------------------------------------------- (b) the twin
@pytest.mark.parametrize("name", OK_CASES)
def test_twin_matches_restatement(name):
    from macvo_amd import _lib as L

    c, res = TC.cases()[name], TC.reference(name)
    row, err = TW.lane(c.est, c.ref, c.align, c.correct_scale)
    col = {n: i for i, n in enumerate(L.EVAL_TRAJ_COLS)}
    T = c.est.shape[0]
    assert (row[col["status"]], row[col["n_poses"]], row[col["n_pairs"]]) == (L.MV_TRAJ_OK, T, T - 1)
    assert np.isnan(err[1:, T - 1]).all() and not np.isnan(err[0]).any() and not np.isnan(err[1:, :T - 1]).any()
    worst = TC.worst_error(c, res, row, err)
    print(name, {k: "%.2e" % v for k, v in worst.items()})
    assert max(worst.values()) <= TWIN_BOUND, worst
    if c.same_as is not None:
        o = TC.cases()[c.same_as]
        row2, err2 = TW.lane(o.est, o.ref, o.align, o.correct_scale)
        assert row.tobytes() == row2.tobytes() and err.tobytes() == err2.tobytes()


@pytest.mark.parametrize("name", BAD_CASES)
def test_twin_status(name):
    from macvo_amd import _lib as L

    c = TC.cases()[name]
    row, err = TW.lane(c.est, c.ref, c.align, c.correct_scale)
    col = {n: i for i, n in enumerate(L.EVAL_TRAJ_COLS)}
    T = c.est.shape[0]
    assert L.TRAJ_STATUS[int(row[col["status"]])] == c.status
    assert (row[col["n_poses"]], row[col["n_pairs"]]) == (T, max(T - 1, 0))
    assert np.isnan(row[:col["d1"]]).all() and np.isnan(err).all()
    if c.status == "DEGENERATE":
        assert row[col["d2"]] < EPS and row[col["d1"]] > 0, row[col["d1"]:col["d3"] + 1]       # the rule saw what the restatement saw


def test_twin_svd():
    """traj::svd3 on its own: factorisation, ordering, orthogonality, det(U) = +1, exact null columns, LAPACK's singular values."""
    g = np.random.default_rng(5)
    mats = [g.normal(size=(3, 3)) for _ in range(20)]
    mats += [np.diag([3.0, 2.0, 0.0]), np.diag([0.0, 5.0, 1.0]), np.zeros((3, 3)), np.diag([1.0, 0.0, 0.0]), np.eye(3), -np.eye(3)]
    a = g.normal(size=(3, 3))
    a[:, 2] = 0.0
    a[2, :] = 0.0
    mats += [a, a.T, np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]), g.normal(size=(3, 3)) * 1e-9, g.normal(size=(3, 3)) * 1e9]
    q, _ = np.linalg.qr(g.normal(size=(3, 3)))
    mats += [q @ np.diag([7.0, 7.0, 1.0]) @ q.T, q @ np.diag([4.0, 1e-9, 1e-13]) @ q.T]
    for m in mats:
        U, d, V = TW.svd3(m)
        scale = max(np.abs(m).max(), 1e-300)
        ref = np.linalg.svd(m, compute_uv=False)
        assert d[0] >= d[1] >= d[2] >= 0
        assert np.abs(d - ref).max() <= 8 * EPS * max(ref[0], 1e-300), (m, d, ref)
        assert np.abs(V.T @ V - np.eye(3)).max() <= 16 * EPS
        if d[1] > 0:
            assert np.abs(U @ np.diag(d) @ V.T - m).max() <= 16 * EPS * scale, m
            assert np.abs(U[:, :2].T @ U[:, :2] - np.eye(2)).max() <= 16 * EPS and abs(np.linalg.det(U) - 1) <= 16 * EPS
    U, d, V = TW.svd3(np.diag([3.0, 2.0, 0.0]))
    assert d[2] == 0.0                                                                            # a null column stays exactly null


# ---------------------------------------------------------------------------------------------------------------------------- (c) bindings
def test_traj_symbol_declared_and_bound():
    import ctypes as C

    import macvo_amd._lib as L

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "macvo_hip.h")).read(), flags=re.S)
    assert re.search(r"\bmv_eval_traj_lanes\s*\(", src) and "mv_eval_traj_lanes" in L.SIGNATURES
    cols = re.search(r"enum\s*\{\s*(MV_EVAL_TRAJ_ATE_MEAN.*?)\}", src, re.S).group(1)
    names = [x.split("=")[0].strip() for x in cols.split(",")]
    assert [n[len("MV_EVAL_TRAJ_"):].lower() for n in names] == list(L.EVAL_TRAJ_COLS) + ["cols"]
    for enum, vals in (("MV_TRAJ_ALIGN_UMEYAMA", [L.MV_TRAJ_ALIGN_UMEYAMA, L.MV_TRAJ_ALIGN_ORIGIN, L.MV_TRAJ_ALIGN_NONE]),
                       ("MV_TRAJ_OK", [L.MV_TRAJ_OK, L.MV_TRAJ_TOO_SHORT, L.MV_TRAJ_DEGENERATE, L.MV_TRAJ_NONFINITE]), ("MV_TRAJ_F32", [L.MV_TRAJ_F32, L.MV_TRAJ_F64])):
        body = re.search(r"enum\s*\{\s*(%s.*?)\}" % enum, src, re.S).group(1)
        assert [int(x.split("=")[1]) for x in body.split(",")] == vals, enum
    assert [s for s in L.TRAJ_STATUS] == ["OK", "TOO_SHORT", "DEGENERATE", "NONFINITE"]
    assert int(re.search(r"#define MV_EVAL_TRAJ_MAX_POSES \(1 << (\d+)\)", src).group(1)) == 20 and L.EVAL_TRAJ_MAX_POSES == 1 << 20
    assert L.ABI_VERSION == 8
    lib = L.load()
    assert lib.mv_abi_version() == 8
    # refusals that need no device: argument checks come before the launch
    one = (C.c_void_p * 1)(8)
    T = (C.c_int32 * 1)(4)
    big = (C.c_int32 * 1)((1 << 20) + 1)
    many = (C.c_void_p * 65)(*([8] * 65))
    manyT = (C.c_int32 * 65)(*([4] * 65))
    call = lib.mv_eval_traj_lanes
    assert call(1, one, one, big, 0, 0, 7, 7, 0, 0, 8, None, 0, None) == -1            # T > 2^20
    assert call(65, many, many, manyT, 0, 0, 7, 7, 0, 0, 8, None, 0, None) == -1       # lanes > MV_MAX_LANES
    assert call(0, one, one, T, 0, 0, 7, 7, 0, 0, 8, None, 0, None) == -1
    assert call(1, one, one, T, 2, 0, 7, 7, 0, 0, 8, None, 0, None) == -1              # dtype
    assert call(1, one, one, T, 0, 0, 6, 7, 0, 0, 8, None, 0, None) == -1              # stride < 7
    assert call(1, one, one, T, 0, 0, 7, 7, 3, 0, 8, None, 0, None) == -1              # align
    assert call(1, one, one, T, 0, 0, 7, 7, 0, 0, None, None, 0, None) == -1           # rows
    assert call(1, one, one, T, 0, 0, 7, 7, 0, 0, 8, 8, 3, None) == -1                 # err_stride < T


def test_sequence_table_assembly():
    """EvalSeq.py:35-83 on read-back rows: None rows, the decorator, the Average over the rows present."""
    from macvo_amd import _lib as L
    from macvo_amd import evaluation as E

    n = len(L.EVAL_TRAJ_COLS)
    a, b, bad = np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64) * 3, np.full(n, np.nan)
    a[-1] = b[-1] = L.MV_TRAJ_OK
    bad[-1] = L.MV_TRAJ_DEGENERATE
    rows = E.trajectory_rows(["s0", "s1", "s2", "s3"], [a, None, bad, b])
    assert rows[0] == ["s0"] + list(a[:12]) and rows[1] == ["s1"] + [None] * 12 and rows[2] == ["s2"] + [None] * 12
    assert rows[4] == ["Average"] + [(x + y) / 2 for x, y in zip(a[:12], b[:12])]
    with pytest.raises(ValueError):
        E.trajectory_rows(["s0"], [None])
    assert E.trajectory_header(True)[:5] == ["Trajectory", "μ_ATE[S]", "σ_ATE", "RMSE_ATE", "μ_RTE[S]"]
    assert E.trajectory_header(False) == ["Trajectory", "μ_ATE", "σ_ATE", "RMSE_ATE", "μ_RTE", "σ_RTE", "RMSE_RTE", "μ_ROE", "σ_ROE", "RMSE_ROE", "μ_RPE", "σ_RPE",
                                          "RMSE_RPE"]
