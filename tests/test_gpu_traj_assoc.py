"""GPU: mv_traj_associate_lanes (csrc/traj_assoc.hip), mv_pose_interpolate(_lanes) (csrc/visual_map.hip) and the layers above them against
tests/traj_assoc_ref.py, the restatement of Trajectory.from_sandbox's association step and of PoseInterpolate (UNPINNED: PyPose and evo are not
importable).  Inputs: tests/traj_assoc_cases.py, built once on the CPU.

Measure (tests/traj_assoc_cases.pose_error): |gpu - ref64| / s, s = max(1, track extent) for positions, 1 for quaternion components, each row up to a
common sign; bound 8 x ASSOC_ERR_MEASURED (the CPU suite's measured twin error).  Flags and status are exact."""
import numpy as np
import pytest
import torch

from tests import traj_assoc_cases as AC
from tests import traj_assoc_ref as AR
from tests import traj_cases as TC
from tests import traj_ref as TR

pytestmark = pytest.mark.gpu

TRAJ_ERR_MEASURED = 1.011e-11          # tests/test_gpu_traj_eval.py: the evaluation kernel's own measured error; its bound is 8 x
TRAJ_BOUND = 8 * TRAJ_ERR_MEASURED
RAD2DEG = 57.29577951308232


@pytest.fixture(scope="module")
def dev(gpu):
    return gpu


def _gpu(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(dev)


def _run(names, dev, out_dtype=torch.float64, origin=False):
    """The named cases as the lanes of one launch -> per lane (poses, flags, status)."""
    from macvo_amd import ops

    cs = [AC.cases()[n] for n in names]
    assert len({c.rebase for c in cs}) == 1
    res = ops.associate_trajectory([_gpu(c.src, dev) for c in cs], [_gpu(c.ts, dev) for c in cs], [_gpu(c.tq, dev) for c in cs],
                                   origin_ref=[_gpu(c.origin, dev) for c in cs] if origin else None, rebase=cs[0].rebase, out_dtype=out_dtype)
    st = res.status.cpu().numpy()
    return [(p.cpu().numpy(), f.cpu().numpy(), int(s)) for p, f, s in zip(res.poses, res.extrapolated, st)]


def _check(name, got, flag, st):
    c = AC.cases()[name]
    want, wflag, wst = AC.reference(name)
    assert AR.STATUS[st] == wst == "OK" and flag.dtype == np.uint8 and flag.tobytes() == wflag.tobytes(), name
    err = AC.pose_error(got, want, AC.scale_of(c))
    print(f"{name}: |gpu - ref64| / s = {err:.3e}")
    assert err <= AC.ASSOC_BOUND, (name, err)


# ------------------------------------------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("T", AC.SHAPE_T)
def test_shapes(T, dev):
    """T x Q in {1, 2, 3, 1024, 1025} x {1, 255, 256, 257, 1000}: the five Q of one T are the lanes of one launch (different lengths per lane)."""
    names = [f"shape_T{T}_Q{Q}" for Q in AC.SHAPE_Q]
    hits = 0
    for name, (got, flag, st) in zip(names, _run(names, dev)):
        _check(name, got, flag, st)
        c = AC.cases()[name]
        assert not flag[c.interior_hits].any()                           # a query exactly on an interior stamp is interpolated (prop = 1), not copied
        hits += len(c.interior_hits)
        if T == 1:
            assert flag.all() and (got == c.src[0]).all()
    assert hits > 0 or T < 3


# ------------------------------------------------------------------------------------------------------------------------------------ 2. lanes
def test_lane_bits_alone_batched_and_moved(dev):
    """The [130, 9] lane alone, as lane 1 of 3 and as lane 63 of 64, beside [T, 9] lanes of other lengths: identical bits, read in place at stride 9."""
    from macvo_amd import ops

    c = AC.cases()["stride9"]
    lane = (_gpu(c.src, dev), _gpu(c.ts, dev), _gpu(c.tq, dev))
    assert lane[0].stride(0) == 9
    others = []
    for k, n in enumerate(("shape_T3_Q257", "shape_T1024_Q255", "shape_T1_Q1", "shape_T1025_Q1000")):
        o = AC.cases()[n]
        wide = np.full((o.src.shape[0], 9), -1.0e30)
        wide[:, :7] = o.src
        others.append((_gpu(wide, dev), _gpu(o.ts, dev), _gpu(o.tq, dev)))

    def run(lanes):
        r = ops.associate_trajectory([x[0] for x in lanes], [x[1] for x in lanes], [x[2] for x in lanes], rebase=False)
        return r

    alone = run([lane])
    three = run([others[0], lane, others[1]])
    many = run([others[i % 4] for i in range(63)] + [lane])
    ref = (alone.poses[0].cpu().numpy().tobytes(), alone.extrapolated[0].cpu().numpy().tobytes())
    assert (three.poses[1].cpu().numpy().tobytes(), three.extrapolated[1].cpu().numpy().tobytes()) == ref
    assert (many.poses[63].cpu().numpy().tobytes(), many.extrapolated[63].cpu().numpy().tobytes()) == ref
    assert not many.status.cpu().numpy().any() and many.status.shape == (64,)
    _check("stride9", alone.poses[0].cpu().numpy(), alone.extrapolated[0].cpu().numpy(), int(alone.status[0]))
    plain = _run(["stride7"], dev)[0]
    assert plain[0].tobytes() == ref[0]                                  # the spare columns (1e30) were not read


# ------------------------------------------------------------------------------------------------------------------------------------ 3. int64 stamps
def test_int64_stamps_rebased_in_integers(dev):
    from macvo_amd import ops

    c = AC.cases()["int64"]
    assert c.rebase and c.ts.dtype == np.int64 and (c.ts[1:] % 256 != 0).all() and int(c.ts[0]) == AC.EUROC_T0
    got, flag, st = _run(["int64"], dev)[0]
    _check("int64", got, flag, st)
    ts_exact = np.array([float(int(x) - int(c.ts[0])) for x in c.ts])                 # Python integers: exact
    tq_exact = np.array([float(int(x) - int(c.tq[0])) for x in c.tq])
    src = _gpu(c.src, dev)
    r = ops.associate_trajectory([src], [_gpu(ts_exact, dev)], [_gpu(tq_exact, dev)], rebase=True)
    assert r.poses[0].cpu().numpy().tobytes() == got.tobytes() and r.extrapolated[0].cpu().numpy().tobytes() == flag.tobytes()
    # converting before subtracting (the reference's astype(float)) rounds these stamps to multiples of 256 ns: another prop, other poses
    early_ts, early_tq = c.ts.astype(np.float64), c.tq.astype(np.float64)
    assert not np.array_equal(early_ts - early_ts[0], ts_exact)
    e = ops.associate_trajectory([src], [_gpu(early_ts, dev)], [_gpu(early_tq, dev)], rebase=True)
    assert e.poses[0].cpu().numpy().tobytes() != got.tobytes()


# ------------------------------------------------------------------------------------------------------------------------------------ 4. fp32
@pytest.mark.parametrize("name", ["f32_T1360", "f32_T1360_origin", "f32_T40", "f32_T40_origin"])
def test_fp32_in_fp32_out(name, dev):
    c = AC.cases()[name]
    assert c.src.dtype == np.float32
    got, flag, st = _run([name], dev, out_dtype=None, origin=c.origin is not None)[0]
    want, wflag, _ = AC.reference(name)
    assert got.dtype == np.float32 and st == 0 and flag.tobytes() == wflag.tobytes()
    w32 = want.astype(np.float32)
    assert (np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= AC.ulp32(w32.astype(np.float64))).all()      # both sides round an fp64 result once
    chain, _ = AR.ref_chain(c.src, c.ts, c.tq, c.origin, c.rebase)
    gap = AC.pose_error(got, chain, AC.scale_of(c))
    print(f"{name}: |gpu - ref_chain| / s = {gap:.3e}")
    assert gap <= AC.ASSOC_F32_CHAIN_BOUND


# ------------------------------------------------------------------------------------------------------------------------------------ 5. rotation branches
def test_rotation_branches(dev):
    names = ["rot_180", "rot_179_999", "rot_tiny", "rot_zero", "quat_alternating", "quat_plain"]
    out = _run(names, dev)
    for name, (got, flag, st) in zip(names, out):
        _check(name, got, flag, st)
    assert AC.pose_error(out[4][0], out[5][0], 1.0) <= AC.ASSOC_BOUND                  # alternating signs: the same rotations, up to sign
    c = AC.cases()["rot_180"]
    assert (c.src[1, 3:] == (1, 0, 0, 0)).all() and (c.src[0, 3:] == (0, 0, 0, 1)).all()  # q_e q_s^-1 has w == 0 exactly


# ------------------------------------------------------------------------------------------------------------------------------------ 6. status
@pytest.mark.parametrize("bad", AC.BAD_CASES)
def test_status_beside_good_lanes(bad, dev):
    from macvo_amd import _lib as L

    c = AC.cases()[bad]
    with_origin = c.origin is not None
    good = ["good_a", "good_b"]
    org = np.array([1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 1.0])

    def run(names):
        from macvo_amd import ops

        cs = [AC.cases()[n] for n in names]
        r = ops.associate_trajectory([_gpu(x.src, dev) for x in cs], [_gpu(x.ts, dev) for x in cs], [_gpu(x.tq, dev) for x in cs],
                                     origin_ref=[_gpu(x.origin if x.origin is not None else org, dev) for x in cs] if with_origin else None, rebase=False)
        return [(p.cpu().numpy(), f.cpu().numpy()) for p, f in zip(r.poses, r.extrapolated)], r.status.cpu().numpy()

    (a, b, g), st = run([good[0], bad, good[1]])
    assert [L.TRAJ_ASSOC_STATUS[s] for s in st] == ["OK", c.status, "OK"]
    assert b[0].shape == (len(c.tq), 7) and np.isnan(b[0]).all() and not b[1].any()
    (a2, g2), st2 = run(good)
    assert not st2.any()
    assert a[0].tobytes() == a2[0].tobytes() and a[1].tobytes() == a2[1].tobytes() and g[0].tobytes() == g2[0].tobytes() and g[1].tobytes() == g2[1].tobytes()
    if not with_origin:
        _check("good_a", a[0], a[1], 0)
        _check("good_b", g[0], g[1], 0)


# ------------------------------------------------------------------------------------------------------------------------------------ 7. origin
def test_origin_alignment(dev):
    (got, flag, st), (moved, mflag, mst) = _run(["origin", "origin_moved"], dev, origin=True)
    _check("origin", got, flag, st)
    _check("origin_moved", moved, mflag, mst)
    c = AC.cases()["origin"]
    want = np.array(c.origin)
    want[3:] = -want[3:] / np.linalg.norm(want[3:])                         # the reference row is given with w < 0
    assert c.tq[0] == c.ts[0] and flag[0] == 1 and got[0, 6] >= 0
    assert AC.pose_error(got[:1], want[None], AC.scale_of(c)) <= AC.ASSOC_BOUND and np.abs(got[0, 3:] - want[3:]).max() <= AC.ASSOC_BOUND
    assert (got[:, 6] >= 0).all()
    assert AC.pose_error(moved, got, AC.scale_of(c)) <= AC.ASSOC_BOUND         # a rigid left factor on the whole source is undone by the alignment


# ------------------------------------------------------------------------------------------------------------------------------------ 8. chained evaluation
def _sparse_fixture():
    g = TC.golden()
    stamps = np.arange(1360) * 0.1 + 1.0e3
    est8 = np.concatenate([stamps[::3, None], g["est"][::3]], axis=1)
    gt8 = np.concatenate([stamps[:, None], g["gt"]], axis=1)
    return est8, gt8


def _stats_bound(i: int, w: float, s: float, ext: float) -> float:
    """The sum used: TRAJ_BOUND (the evaluation kernel's own) + the association bound propagated.  A pose moved by ASSOC_BOUND * s in position and
    ASSOC_BOUND per quaternion component (2 ASSOC_BOUND rad) moves an ATE value by <= ASSOC_BOUND * s; a relative value takes two poses on either
    side of two products: <= 8 ASSOC_BOUND * max(s, RAD2DEG) in metres / degrees / matrix norm.  mean, std and rmse move by no more than their
    values do.  Relative to the figure's denominator: the extent for ATE, the figure's own magnitude otherwise."""
    den = ext if i < 3 else max(abs(w), 1e-12)
    return TRAJ_BOUND + 8 * AC.ASSOC_BOUND * max(s, RAD2DEG) / den


def test_evaluate_sequences_on_timed_rows(dev):
    """Every third estimate row with its stamp against the full-rate reference: refused without stamps (the lengths differ), scored with them."""
    from macvo_amd import _lib as L
    from macvo_amd import evaluation as E
    from macvo_amd import ops

    est8, gt8 = _sparse_fixture()
    with pytest.raises(L.MacvoHipError, match="time-associated"):
        ops.eval_trajectory([_gpu(est8[:, 1:], dev)], [_gpu(gt8[:, 1:], dev)])
    header, rows = E.EvaluateSequences([("sparse", gt8, est8), ("sparse_gpu", _gpu(gt8, dev), _gpu(est8, dev)), ("none", gt8, None)])
    assoc, flag, st = AR.ref64(est8[:, 1:], est8[:, 0], gt8[:, 0], origin=gt8[0, 1:], rebase=True)
    assert st == "OK" and flag.sum() == 2                                    # the first and the last stamp: rows 0 and 1359 are estimate rows
    want = TR.stats_row(TR.evaluate(assoc, gt8[:, 1:], "umeyama", False))
    ext, s = AC.extent(gt8[:, 1:]), max(1.0, AC.extent(assoc))
    assert rows[2][1:] == [None] * 12 and rows[3][0] == "Average"
    for r in rows[:2]:
        for i in range(12):
            rel = abs(r[1 + i] - want[i]) / (ext if i < 3 else max(abs(want[i]), 1e-12))
            print(f"{r[0]} {header[1 + i]}: {rel:.3e} (bound {_stats_bound(i, want[i], s, ext):.3e})")
            assert rel <= _stats_bound(i, want[i], s, ext), (r[0], header[1 + i])
    assert rows[0][1:] == rows[1][1:]
    # the four evaluate* functions take the same input
    m = E.evaluateATE(E.Trajectory(_gpu(gt8[:, 1:], dev), _gpu(gt8[:, 0], dev)), est8)
    assert abs(m.stats["rmse"] - want[2]) / ext <= _stats_bound(2, want[2], s, ext) and m.error_array.shape == (1360,)


def test_timed_input_with_coinciding_stamps_equals_untimed(dev):
    from macvo_amd import evaluation as E

    g = TC.golden()
    assert np.array_equal(g["est"][0], g["gt"][0])                           # coinciding origins: the alignment is the identity up to rounding
    stamps = (np.arange(1360) * 0.1 + 1.0e3)[:, None]
    _, timed = E.EvaluateSequences([("t", np.concatenate([stamps, g["gt"]], 1), np.concatenate([stamps, g["est"]], 1))])
    _, plain = E.EvaluateSequences([("t", g["gt"], g["est"])])
    ext = AC.extent(g["gt"])
    for i in range(12):
        w = plain[0][1 + i]
        assert abs(timed[0][1 + i] - w) / (ext if i < 3 else max(abs(w), 1e-12)) <= _stats_bound(i, w, max(1.0, ext), ext), i


def test_device_maps_evaluate_with_reference_clock(dev):
    """A 3-lane map of skipped-style rows of different lengths, its own int64 time_ns, against references on their own (denser, longer) clocks."""
    from macvo_amd.devmap import DeviceVisualMaps

    maps = DeviceVisualMaps(3, dev, init_size=256)
    refs, times, wants = [], [], []
    for l, (m, T) in enumerate(zip(maps, (40, 97, 130))):
        ref = TR.random_walk(3 * T + 5, 500 + l)
        t_ref = AC.EUROC_T0 + np.arange(3 * T + 5, dtype=np.int64) * 33_333_333 + 7 * l
        est = TR.perturb(ref, 600 + l)[2::3][:T]
        t_est = t_ref[2::3][:T] + 1001                                       # off the reference's stamps
        m.frames["pose"][:T] = _gpu(est, dev).float()
        m.frames["T_BS"][:T] = torch.tensor([0.1, -0.2, 0.05, 0.0, 0.0, 0.0, 1.0], device=dev)
        m.frames["time_ns"][:T] = _gpu(t_est, dev)
        m.frames["need_interp"][:T] = True
        m.n_frames = T
        refs.append(_gpu(ref, dev))
        times.append(_gpu(t_ref, dev))
        body = m.body_poses().cpu().numpy()
        assoc, _, st = AR.ref64(body, t_est, t_ref, origin=ref[0], rebase=True)
        assert st == "OK"
        wants.append((TR.stats_row(TR.evaluate(assoc, ref, "umeyama", False)), AC.extent(ref), max(1.0, AC.extent(assoc))))
    got = maps.evaluate(refs, ref_times=times)
    assert got.assoc_status.cpu().tolist() == [0, 0, 0]
    rows = got.rows.cpu().numpy()
    assert rows[:, -1].tolist() == [0, 0, 0]
    for l, (want, ext, s) in enumerate(wants):
        for i in range(12):
            assert abs(rows[l, i] - want[i]) / (ext if i < 3 else max(abs(want[i]), 1e-12)) <= _stats_bound(i, want[i], s, ext), (l, i)
    # a lane whose association fails reaches the evaluation as NaN rows
    maps[1].frames["time_ns"][5] = maps[1].frames["time_ns"][4]
    bad = maps.evaluate(refs, ref_times=times)
    assert bad.assoc_status.cpu().tolist() == [0, 4, 0] and bad.rows[:, -1].cpu().tolist() == [0, 3, 0]
    assert bad.rows[0].cpu().numpy().tobytes() == rows[0].tobytes()


def test_trajectory_class(dev, tmp_path):
    from macvo_amd import evaluation as E

    est8, gt8 = _sparse_fixture()
    np.save(tmp_path / "poses.npy", est8)
    np.save(tmp_path / "ref_poses.npy", gt8)
    gt, est = E.Trajectory.from_sandbox(str(tmp_path), device=dev)
    assert est.length == gt.length == 1360 and est.poses.dtype == torch.float32 and est.time.tolist() == gt.time.tolist() and gt.time[0] == 0
    assert est.frame_status.sum() == 2 and est.translation.shape == (1360, 3) and est.rotation.shape == (1360, 4) and est[5:9].length == 4
    assert est.crop(10, 20).length == 10 and torch.equal(est.scale(2.0).translation, est.translation * 2.0)
    # the reference's two-step chain: align_origin rounds to fp32 (from_evo(...).float()), then align_time in that dtype
    aligned = AR.ref64(est8[:, 1:], np.arange(454.0), np.arange(454.0), origin=gt8[0, 1:], rebase=False)[0].astype(np.float32)
    want = AR.ref64(aligned, est8[:, 0], gt8[:, 0], rebase=True)[0]
    got = est.poses.cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= 2 * AC.ulp32(want)).all()                  # one fp32 ulp of the first launch's store can move the second's by one more


# ------------------------------------------------------------------------------------------------------------------------------------ 9. PoseInterpolate
def _fill(m, pose, need, dev):
    T = len(need)
    m.frames["pose"][:T] = _gpu(pose, dev)
    m.frames["need_interp"][:T] = _gpu(need, dev).bool()
    m.n_frames = T


@pytest.mark.parametrize("T", AC.POSE_T)
def test_pose_interpolate(T, dev):
    from macvo_amd.devmap import DeviceVisualMap

    for pattern in AC.POSE_PATTERNS:
        pose, need, (want, want_need, want_mask) = AC.pose_case(T, pattern)
        m = DeviceVisualMap(dev, init_size=512)
        _fill(m, pose, need, dev)
        mask = m.pose_interpolate()
        assert isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype == torch.uint8
        mask = mask.cpu().numpy()
        got = m.frames["pose"][:T].cpu().numpy()
        assert mask.tobytes() == want_mask.tobytes(), pattern
        assert m.frames["need_interp"][:T].cpu().numpy().astype(np.uint8).tobytes() == want_need.tobytes(), pattern   # the edge flags are cleared in the map
        good = mask == 0
        assert got[good].tobytes() == pose[good].tobytes(), pattern                                                   # good rows: bit-untouched
        assert (np.abs(got[~good].astype(np.float64) - want[~good]) <= AC.ulp32(want[~good])).all(), pattern
        if T <= 10:
            assert not mask.any() and got.tobytes() == pose.tobytes()
        elif pattern in ("all_inner", "alternating"):
            assert mask.any()


def test_pose_interpolate_lanes_equal_single_calls(dev):
    from macvo_amd.devmap import DeviceVisualMap, DeviceVisualMaps

    picks = [(64, "alternating"), (9, "edges"), (300, "all_inner")]
    maps = DeviceVisualMaps(3, dev, init_size=512)
    singles = []
    for m, (T, pattern) in zip(maps, picks):
        pose, need, _ = AC.pose_case(T, pattern)
        _fill(m, pose, need, dev)
        one = DeviceVisualMap(dev, init_size=512)
        _fill(one, pose, need, dev)
        singles.append((one, one.pose_interpolate()))
    masks = maps.pose_interpolate()
    for m, (one, mask1), mask, (T, _) in zip(maps, singles, masks, picks):
        assert mask.shape == (T,) and mask.cpu().numpy().tobytes() == mask1.cpu().numpy().tobytes()
        assert m.frames["pose"][:T].cpu().numpy().tobytes() == one.frames["pose"][:T].cpu().numpy().tobytes()
        assert torch.equal(m.frames["need_interp"][:T], one.frames["need_interp"][:T])
    assert masks[0].any() and masks[2].sum() == 290 and not masks[1].any()


def test_write_takes_the_processor_choice(dev, tmp_path):
    from macvo_amd.devmap import DeviceVisualMaps

    pose, need, (want, _, want_mask) = AC.pose_case(64, "alternating")
    out = {}
    for how in ("pose", "motion", False):
        maps = DeviceVisualMaps(1, dev, init_size=128)
        _fill(maps[0], pose, need, dev)
        maps[0].frames["T_BS"][:64] = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=dev)
        maps.write([str(tmp_path / str(how))], interpolate=how)
        out[how] = maps[0].frames["pose"][:64].cpu().numpy()
    assert out[False].tobytes() == pose.tobytes() and out["pose"].tobytes() != pose.tobytes() and out["motion"].tobytes() != out["pose"].tobytes()
    bad = want_mask != 0
    assert (np.abs(out["pose"][bad].astype(np.float64) - want[bad]) <= AC.ulp32(want[bad])).all()
    with pytest.raises(ValueError):
        DeviceVisualMaps(1, dev, init_size=128).write([str(tmp_path / "x")], interpolate="spline")
