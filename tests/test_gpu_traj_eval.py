"""GPU: mv_eval_traj_lanes (csrc/traj_eval.hip) and the layers above it against tests/traj_ref.py, the numpy restatement of what
Evaluation/MetricsSeq.py asks of evo 1.x (UNPINNED: evo is not importable, no evo run stands behind the figures).

Inputs: tests/traj_cases.py (seeded random walks + the fixture tests/golden/traj_eval.npz); their conditions (d_2 > 1e-6 where the alignment must
work, d_2 < DBL_EPSILON where it must not, the reflection branch, the exactly planar track) are asserted on the CPU by a module fixture of this
file (tests/traj_cases.check_conditions, the check tests/test_traj_eval_host.py runs) and by the lanes64 fixture for the lanes this file adds.

Measure (tests/traj_cases.worst_error): |gpu - ref| / s; s = the track's extent for ATE, the value's own magnitude max(|ref|, 1e-12) for RTE / ROE /
RPE, the offset distance for the offset cases; R, t, c, d on the same scheme.  Counts and status are exact."""
import numpy as np
import pytest
import torch

from tests import traj_cases as TC
from tests import traj_ref as TR

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
# The worst |gpu - ref| / s over every case of this file, measured on the MI355X (test_worst_error_over_all_cases prints it).  The asserted bound is
# 8 x that: the margin is for the ulp-order differences between Jacobi and LAPACK singular vectors and between the device's and libm's atan2.  It
# may never exceed 1e-9: correct fp64 arithmetic sits orders of magnitude below (the restatement's own rigid-invariance noise is 1e-12 .. 1e-11), a
# wrong reflection branch, an uncentred covariance or fp32 arithmetic orders of magnitude above.
TRAJ_ERR_MEASURED = 1.011e-11
TRAJ_BOUND = 8 * TRAJ_ERR_MEASURED
assert TRAJ_BOUND <= 1e-9

OK_CASES = [n for n, c in TC.cases().items() if c.status == "OK"]
BAD_CASES = [n for n, c in TC.cases().items() if c.status != "OK"]


@pytest.fixture(scope="module")
def dev(gpu):
    return gpu


@pytest.fixture(scope="module", autouse=True)
def inputs_satisfy_their_conditions():
    """A `pytest -m gpu` run does not execute the CPU file: the conditions on the shared cases are asserted here too, once, by the restatement alone."""
    TC.check_conditions()


def _col():
    from macvo_amd import _lib as L

    return {n: i for i, n in enumerate(L.EVAL_TRAJ_COLS)}


def _gpu(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(dev)


def run_case(c, dev, errors=True):
    """One lane through ops.eval_trajectory, in place: a [T, 9] / [T, 11] case keeps its row stride."""
    from macvo_amd import ops

    res = ops.eval_trajectory([_gpu(c.est, dev)], [_gpu(c.ref, dev)], c.align, c.correct_scale, errors=errors)
    return res.rows[0].cpu().numpy(), (res.errors[0].cpu().numpy() if errors else None)


@pytest.mark.parametrize("name", OK_CASES)
def test_case_matches_restatement(name, dev):
    from macvo_amd import _lib as L

    c, res = TC.cases()[name], TC.reference(name)
    row, err = run_case(c, dev)
    col, T = _col(), c.est.shape[0]
    assert (row[col["status"]], row[col["n_poses"]], row[col["n_pairs"]]) == (L.MV_TRAJ_OK, T, T - 1)
    assert not np.isnan(err[0, :T]).any() and not np.isnan(err[1:, :T - 1]).any() and np.isnan(err[1:, T - 1:]).all()
    worst = TC.worst_error(c, res, row, err)
    print(name, {k: "%.2e" % v for k, v in worst.items()})
    assert max(worst.values()) <= TRAJ_BOUND, worst
    if c.same_as is not None:                                       # q and -q, k q, a strided table: identical rows
        o = TC.cases()[c.same_as]
        row2, err2 = run_case(o, dev)
        assert row.tobytes() == row2.tobytes() and err[:, :T].tobytes() == err2[:, :T].tobytes()


def test_worst_error_over_all_cases(dev):
    """The figure TRAJ_ERR_MEASURED records: every OK case in one batched call per 64 lanes would mix strides, so lane by lane."""
    worst, where = 0.0, None
    for name in OK_CASES:
        c = TC.cases()[name]
        row, err = run_case(c, dev)
        w = TC.worst_error(c, TC.reference(name), row, err)
        k = max(w, key=w.get)
        if w[k] > worst:
            worst, where = w[k], (name, k)
    print("worst |gpu - ref| / s over %d cases: %.3e at %s" % (len(OK_CASES), worst, where))
    assert worst <= TRAJ_BOUND, (worst, where)


@pytest.mark.parametrize("name", BAD_CASES)
def test_status(name, dev):
    from macvo_amd import _lib as L

    c = TC.cases()[name]
    row, err = run_case(c, dev)
    col, T = _col(), c.est.shape[0]
    assert L.TRAJ_STATUS[int(row[col["status"]])] == c.status
    assert (row[col["n_poses"]], row[col["n_pairs"]]) == (T, max(T - 1, 0))
    assert np.isnan(row[:col["d1"]]).all() and np.isnan(err).all()
    if c.status == "DEGENERATE":
        assert row[col["d2"]] < EPS and row[col["d1"]] > 0
    else:
        assert np.isnan(row[col["d1"]:col["d3"] + 1]).all()


def test_pose_table_of_a_device_map_in_place(dev):
    """A DeviceVisualMap's own [cap, 7] fp32 pose table, read where it lies (no copy: the same data_ptr reaches the launch), against an fp64 reference."""
    from macvo_amd import ops
    from macvo_amd.devmap import DeviceVisualMap

    c = TC.cases()["f32_f64"]
    T = c.est.shape[0]
    m = DeviceVisualMap(dev, init_size=256)
    table = m.frames["pose"]
    assert table.dtype == torch.float32 and table.shape[1] == 7 and table.shape[0] >= T
    table[:T] = _gpu(c.est, dev)
    table[T:] = float("nan")                                        # rows past T must not be read
    view = table[:T]
    assert view.data_ptr() == table.data_ptr()
    res = ops.eval_trajectory([view], [_gpu(c.ref, dev)], errors=True)
    row, err = run_case(c, dev)
    assert res.rows[0].cpu().numpy().tobytes() == row.tobytes() and res.errors[0].cpu().numpy().tobytes() == err.tobytes()
    w = TC.worst_error(c, TC.reference("f32_f64"), row, err)
    assert max(w.values()) <= TRAJ_BOUND, w


# ------------------------------------------------------------------------------------------------------------------------------------ lanes
def _lane_set(n: int):
    """n lanes, each of a different T, one degenerate and one too-short lane in the middle (n >= 3)."""
    lanes = []
    for l in range(n):
        T = 5 + 7 * l + (250 if l % 5 == 0 else 0)
        ref = TR.random_walk(T, 500 + l)
        lanes.append((TR.perturb(ref, 600 + l), ref))
    if n >= 3:
        c = TC.cases()
        lanes[n // 2] = (np.array(c["line_x"].est), np.array(c["line_x"].ref))
        lanes[n // 2 - 1] = (np.array(c["T1"].est), np.array(c["T1"].ref))
    assert len({e.shape[0] for e, _ in lanes}) == n
    return lanes


@pytest.fixture(scope="module")
def lanes64():
    lanes = _lane_set(64)
    for l, (e, r) in enumerate(lanes):                              # conditions on the inputs, by the restatement alone
        if l == 32:
            assert TR.singular_values(e, r)[1] < EPS
        elif l != 31:
            assert TR.singular_values(e, r)[1] > 1e-6, l
    return lanes


@pytest.mark.parametrize("n", [1, 3, 64])
def test_lanes_bit_equal_alone_batched_and_moved(n, dev, lanes64):
    from macvo_amd import _lib as L
    from macvo_amd import ops

    lanes = lanes64 if n == 64 else ([lanes64[40]] if n == 1 else [lanes64[3], lanes64[31], lanes64[32]])
    est = [_gpu(e, dev) for e, _ in lanes]
    ref = [_gpu(r, dev) for _, r in lanes]
    both = ops.eval_trajectory(est, ref, errors=True)
    rows, errs = both.rows.cpu().numpy(), both.errors.cpu().numpy()
    perm = [(i + 1) % n for i in range(n)] if n < 64 else [(7 * i + 13) % 64 for i in range(64)]        # every lane in another position
    moved = ops.eval_trajectory([est[i] for i in perm], [ref[i] for i in perm], errors=True)
    mrows, merrs = moved.rows.cpu().numpy(), moved.errors.cpu().numpy()
    col = _col()
    st = [int(x) for x in rows[:, col["status"]]]
    if n == 64:
        assert st[31] == L.MV_TRAJ_TOO_SHORT and st[32] == L.MV_TRAJ_DEGENERATE and all(s == L.MV_TRAJ_OK for i, s in enumerate(st) if i not in (31, 32))
    if n == 3:
        assert st == [L.MV_TRAJ_OK, L.MV_TRAJ_TOO_SHORT, L.MV_TRAJ_DEGENERATE]
    for l in range(n):
        T = lanes[l][0].shape[0]
        p = perm.index(l)
        assert rows[l].tobytes() == mrows[p].tobytes(), l
        assert errs[l, :, :T].tobytes() == merrs[p, :, :T].tobytes(), l
        alone = ops.eval_trajectory([est[l]], [ref[l]], errors=True)          # ... and every lane again on its own
        assert alone.rows[0].cpu().numpy().tobytes() == rows[l].tobytes(), l
        assert alone.errors[0, :, :T].cpu().numpy().tobytes() == errs[l, :, :T].tobytes(), l
    # ... and the batched rows are right, not only equal: two lanes against the restatement
    for l in ([0] if n < 64 else [0, 63]):
        if st[l] == L.MV_TRAJ_OK:
            c = TC.Case("lane", lanes[l][0], lanes[l][1])
            w = TC.worst_error(c, TR.evaluate(c.est, c.ref), rows[l], errs[l])
            assert max(w.values()) <= TRAJ_BOUND, (l, w)


def test_three_dim_tensor_and_refusals(dev):
    from macvo_amd import _lib as L
    from macvo_amd import ops

    c = TC.cases()
    e = torch.stack([_gpu(c["f64_f64"].est, dev), _gpu(c["quat_negated"].est, dev)])
    r = torch.stack([_gpu(c["f64_f64"].ref, dev), _gpu(c["quat_negated"].ref, dev)])
    res = ops.eval_trajectory(e, r)
    assert res.errors is None and res.rows.shape == (2, len(L.EVAL_TRAJ_COLS)) and res.rows.dtype == torch.float64 and res.rows.is_cuda
    rows = res.rows.cpu().numpy()
    assert rows[0].tobytes() == rows[1].tobytes() == run_case(c["f64_f64"], dev)[0].tobytes()
    with pytest.raises(L.MacvoHipError, match="time-associated"):
        ops.eval_trajectory([e[0]], [r[0][:-1]])
    with pytest.raises(L.MacvoHipError):
        ops.eval_trajectory([e[0]], [r[0], r[1]])
    with pytest.raises(L.MacvoHipError):
        ops.eval_trajectory([e[0].cpu()], [r[0]])
    with pytest.raises(L.MacvoHipError):
        ops.eval_trajectory([e[0]], [r[0]], align="sim3")
    with pytest.raises(L.MacvoHipError):
        ops.eval_trajectory([e[0][:, :6]], [r[0]])
    with pytest.raises(L.MacvoHipError):
        ops.eval_trajectory([e[0].half()], [r[0]])


# ------------------------------------------------------------------------------------------------------------------------------------ layers
def test_evaluate_functions_under_the_reference_names(dev):
    from macvo_amd import evaluation as E

    for name in ("fixture_umeyama_0", "scaled_scale"):
        c, res = TC.cases()[name], TC.reference(name)
        ext = TC.extent(c)
        for k, (fn, m) in enumerate(((E.evaluateATE, "ate"), (E.evaluateRTE, "rte"), (E.evaluateROE, "roe"), (E.evaluateRPE, "rpe"))):
            # gt first, as MetricsSeq.py; numpy on the host and tensors on the device are both taken
            out = fn(np.array(c.ref), _gpu(c.est, dev), correct_scale=c.correct_scale) if k % 2 else fn(_gpu(c.ref, dev), np.array(c.est), c.correct_scale)
            assert set(out.stats) == {"mean", "std", "rmse"} and out.np_arrays["error_array"].shape == res[m].shape
            s = ext if m == "ate" else np.maximum(np.abs(res[m]), 1e-12)
            assert np.max(np.abs(out.error_array - res[m]) / s) <= TRAJ_BOUND, (name, m)
            for key in TR.STATS:
                d = ext if m == "ate" else max(abs(res["stats"][m][key]), 1e-12)
                assert abs(out.stats[key] - res["stats"][m][key]) / d <= TRAJ_BOUND, (name, m, key)
    c = TC.cases()["line_x"]
    with pytest.raises(E.TrajectoryEvaluationError, match="DEGENERATE"):
        E.evaluateATE(c.ref, c.est)
    c = TC.cases()["T1"]
    with pytest.raises(E.TrajectoryEvaluationError, match="TOO_SHORT"):
        E.evaluateRTE(c.ref, c.est)


@pytest.mark.parametrize("correct_scale", [False, True])
def test_evaluate_sequences_table(correct_scale, dev):
    """Header, None rows and the Average row against the same table assembled from the restatement (EvalSeq.py:35-83)."""
    from macvo_amd import evaluation as E

    names = ["generic_umeyama_0", "line_x", "planar", "T1", "scaled_noscale", "nonfinite_nan", "len65"]
    c = TC.cases()
    tracks = [(n, np.array(c[n].ref), _gpu(c[n].est, dev) if i % 2 else np.array(c[n].est)) for i, n in enumerate(names)]
    tracks.insert(3, ("no_estimate", np.array(c["len3"].ref), None))
    header, rows = E.EvaluateSequences(tracks, correct_scale=correct_scale)
    dec = "[S]" if correct_scale else ""
    assert header == ["Trajectory", f"μ_ATE{dec}", "σ_ATE", "RMSE_ATE", f"μ_RTE{dec}", "σ_RTE", "RMSE_RTE", f"μ_ROE{dec}", "σ_ROE", "RMSE_ROE", f"μ_RPE{dec}",
                      "σ_RPE", "RMSE_RPE"]
    want = []
    for name, gt, est in tracks:
        try:
            if est is None:
                raise ValueError("no estimate")
            res = TR.evaluate(est.cpu().numpy() if isinstance(est, torch.Tensor) else est, gt, "umeyama", correct_scale)
            want.append([name] + TR.stats_row(res))
        except (ValueError, TR.TooShort, TR.Degenerate, TR.NonFinite):
            want.append([name] + [None] * 12)
    want.append(["Average"] + [sum(r[i] for r in want if r[i] is not None) / sum(1 for r in want if r[i] is not None) for i in range(1, 13)])
    assert [r[0] for r in rows] == [w[0] for w in want] and rows[-1][0] == "Average"
    assert [r[0] for r in rows if r[1] is None] == ["line_x", "no_estimate", "T1", "nonfinite_nan"]
    for r, w in zip(rows, want):
        assert [x is None for x in r[1:]] == [x is None for x in w[1:]], r[0]
        if w[1] is None:
            continue
        ext = max(TC.extent(c[n]) for n in names) if r[0] == "Average" else TC.extent(c[r[0]])
        for i in range(1, 13):
            s = ext if i <= 3 else max(abs(w[i]), 1e-12)
            assert abs(r[i] - w[i]) / s <= TRAJ_BOUND, (r[0], header[i])


def test_evaluate_sequences_mixed_dtypes(dev):
    """fp32 and fp64 tracks in one table: the side is widened to fp64, every track gets its scored row."""
    from macvo_amd import evaluation as E

    c = TC.cases()
    a, b = c["f32_f32"], c["len65"]
    _, rows = E.EvaluateSequences([("a", np.array(a.ref), np.array(a.est)), ("b", np.array(b.ref), _gpu(b.est, dev))])
    for r, case, name in ((rows[0], a, "f32_f32"), (rows[1], b, "len65")):
        w = TR.stats_row(TC.reference(name))
        ext = TC.extent(case)
        for i in range(12):
            assert abs(r[1 + i] - w[i]) / (ext if i < 3 else max(abs(w[i]), 1e-12)) <= TRAJ_BOUND, (name, i)


def test_device_maps_evaluate(dev):
    """DeviceVisualMaps.evaluate == ops.eval_trajectory on every lane's body_poses(), bit for bit, and the body poses are what was stored."""
    from macvo_amd import ops
    from macvo_amd.devmap import DeviceVisualMaps

    c = TC.cases()
    picks = [c["f32_f32"], c["len65"], c["T1"]]
    maps = DeviceVisualMaps(3, dev, init_size=256)
    refs = []
    for m, case in zip(maps, picks):
        T = case.est.shape[0]
        m.frames["pose"][:T] = _gpu(case.est, dev).float()
        m.frames["T_BS"][:T] = torch.tensor([0.1, -0.2, 0.05, 0.0, 0.0, 0.0, 1.0], device=dev)
        m.n_frames = T
        refs.append(_gpu(case.ref, dev).double())                 # one dtype per side
    got = maps.evaluate(refs, errors=True)
    body = [m.body_poses() for m in maps]
    want = ops.eval_trajectory(body, refs, errors=True)
    assert got.rows.cpu().numpy().tobytes() == want.rows.cpu().numpy().tobytes()
    assert got.errors.cpu().numpy().tobytes() == want.errors.cpu().numpy().tobytes()
    col = _col()
    assert [int(x) for x in got.rows[:, col["status"]].cpu()] == [0, 0, 1]
    # against the restatement on the same body poses (read back): the whole path from the maps to the figures
    for l in (0, 1):
        case = TC.Case("map", body[l].cpu().numpy(), np.array(picks[l].ref))
        w = TC.worst_error(case, TR.evaluate(case.est, case.ref), got.rows[l].cpu().numpy(), got.errors[l].cpu().numpy())
        assert max(w.values()) <= TRAJ_BOUND, (l, w)
    other = maps.evaluate(refs, align="origin", correct_scale=True)
    assert other.rows.cpu().numpy()[0].tobytes() != got.rows.cpu().numpy()[0].tobytes()
