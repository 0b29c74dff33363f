"""CPU: stereo rectification off the GPU — the C plan (``mv_stereo_rectify_plan``) against the reference's hard-coded EuRoC baseline, against the forward camera
model alone and against the numpy restatement (``tests/rectify_ref.py``); its error paths; the remap's host twin (``csrc/remap_math.h`` replayed by
``tests/c_abi/remap_twin.cpp``) against the numpy integer formula; the ABI.

OpenCV is restated, PARITY-UNPINNED (it is no dependency): the principal point agrees with OpenCV's to about 1e-4 px (OpenCV keeps the four undistorted corners in
float32, the plan in double).  What pins the restatement to the reference is the EuRoC baseline below."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from macvo_amd import _lib as L
from macvo_amd import ops
from tests import rectify_cases as RC
from tests import rectify_ref as RR
from tests import remap_twin as TW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the largest relative difference (per array: max |C - numpy| / max |numpy|) between the C plan and tests/rectify_ref.py over RIGS, measured
# by test_c_plan_matches_numpy_restatement (which prints it); both sides are the same fp64 formulae, so it is rounding of differently ordered sums.
# Asserted at 8 x (the margin convention of TRAJ_ERR_MEASURED); beyond 1e-9 the C code has a bug, not a rounding difference.
RECT_PLAN_ERR_MEASURED = 2.191e-16
RECT_PLAN_BOUND = 8 * RECT_PLAN_ERR_MEASURED


def _rig4():
    K1, D1, K2, D2, size, R, T = RR.euroc_rig()
    return K1, D1[:4], K2, D2[:4], size, R, T


RIGS = {"euroc": RR.euroc_rig, "vertical_8_4": RR.vertical_rig, "euroc_4coef": _rig4,
        "euroc_small": lambda: RR.euroc_rig()[:4] + ((47, 30),) + RR.euroc_rig()[5:]}


def _plan_arrays(p):
    if isinstance(p, dict):
        out = {k: p[k] for k in ("R1", "R2", "P1", "P2")}
        out.update(baseline=np.array([p["baseline"]]), fc=np.array([p["fc"]]))
        for i, c in enumerate(p["cams"]):
            out[f"iR{i}"] = c["iR"]
            out[f"intr{i}"] = np.array([c["fx"], c["fy"], c["cx"], c["cy"]])
            out[f"k{i}"] = c["k"]
        return out
    out = dict(R1=p.R1.numpy(), R2=p.R2.numpy(), P1=p.P1.numpy(), P2=p.P2.numpy(), baseline=np.array([p.c.baseline]), fc=np.array([p.c.fc]))
    for i in range(2):
        c = p.c.cam[i]
        out[f"iR{i}"] = np.array(list(c.iR)).reshape(3, 3)
        out[f"intr{i}"] = np.array([c.fx, c.fy, c.cx, c.cy])
        out[f"k{i}"] = np.array(list(c.k))
    return out


def test_euroc_baseline_pin():
    """EuRoC's public calibration at (752, 480) gives the baseline the reference hard-codes, to the ten digits it prints (EuRoC.py:76)."""
    for p in (ops.stereo_rectify_plan(*RR.euroc_rig()), ):
        assert abs(p.baseline - 0.1100778422) <= 5e-11, p.baseline
        assert p.idx == 0 and float(p.P2[0, 3]) < 0
        assert p.size == (752, 480)
        assert np.array_equal(p.K.numpy(), p.P1.numpy()[:, :3].astype(np.float32))
    ref = RR.plan(*RR.euroc_rig())
    assert abs(ref["baseline"] - 0.1100778422) <= 5e-11 and ref["idx"] == 0 and ref["P2"][0, 3] < 0


@pytest.mark.parametrize("rig", ["euroc", "vertical_8_4"])
def test_plan_geometry_against_forward_model(rig):
    """Independent of the restatement: only the forward camera model.  For points X in front of the rig, a = R1 X and b = R2 (R X + T) project through P1[:, :3]
    onto one row (column for the vertical rig), fc * baseline / a_z apart along the other axis, and iR followed by the distortion formula at the left
    rectified pixel is the distorted projection of X in camera 1.  1e-6 px each: well above fp64 rounding at 1e3 px, five orders below the remap's 1/32 px."""
    K1, D1, K2, D2, size, R, T = RIGS[rig]()
    p = ops.stereo_rectify_plan(K1, D1, K2, D2, size, R, T)
    A = _plan_arrays(p)
    idx, fc, bl = p.idx, p.focal, p.baseline
    assert idx == (1 if rig.startswith("vertical") else 0)
    rng = np.random.default_rng(0)
    X = np.stack([rng.uniform(-3, 3, 2000), rng.uniform(-2, 2, 2000), rng.uniform(2, 20, 2000)], 1)
    a, b = X @ A["R1"].T, (X @ np.asarray(R).T + np.asarray(T)) @ A["R2"].T
    M = A["P1"][:, :3]
    pa, pb = a @ M.T, b @ M.T
    pa, pb = pa[:, :2] / pa[:, 2:], pb[:, :2] / pb[:, 2:]
    same, other = idx ^ 1, idx
    e_row = np.abs(pa[:, same] - pb[:, same]).max()
    e_disp = np.abs(np.abs(pa[:, other] - pb[:, other]) - fc * bl / a[:, 2]).max()
    q = np.concatenate([pa, np.ones((2000, 1))], 1) @ A["iR0"].T
    xd, yd = RR.distort(q[:, 0] / q[:, 2], q[:, 1] / q[:, 2], RR.coeffs8(D1))
    fxd, fyd = RR.distort(X[:, 0] / X[:, 2], X[:, 1] / X[:, 2], RR.coeffs8(D1))
    e_map = max(np.abs(K1[0, 0] * (xd - fxd)).max(), np.abs(K1[1, 1] * (yd - fyd)).max())
    print(f"{rig}: row {e_row:.2e} px, disparity {e_disp:.2e} px, map vs forward model {e_map:.2e} px")
    assert e_row <= 1e-6 and e_disp <= 1e-6 and e_map <= 1e-6
    # a.z == b.z: the rectified cameras share their optical axes' direction
    assert np.abs(a[:, 2] - b[:, 2] - (A["R2"] @ np.asarray(T))[2]).max() <= 1e-9


def _plan_err(name):
    rig = RIGS[name]()
    c, r = _plan_arrays(ops.stereo_rectify_plan(*rig)), _plan_arrays(RR.plan(*rig))
    return max(float(np.abs(c[k] - r[k]).max() / np.abs(r[k]).max()) for k in r)


def test_c_plan_matches_numpy_restatement():
    """The figure recorded as RECT_PLAN_ERR_MEASURED."""
    errs = {n: _plan_err(n) for n in RIGS}
    print("C plan vs numpy, relative:", {k: f"{v:.3e}" for k, v in errs.items()})
    assert RECT_PLAN_ERR_MEASURED < 1e-9
    assert max(errs.values()) <= RECT_PLAN_BOUND, errs
    for n in RIGS:
        rig = RIGS[n]()
        assert ops.stereo_rectify_plan(*rig).idx == RR.plan(*rig)["idx"]


def test_plan_coefficient_counts_agree_with_twin():
    """A 4-coefficient and an 8-coefficient rig; 5 coefficients with k3 = 0 is the 4-coefficient plan."""
    assert _plan_err("euroc_4coef") <= RECT_PLAN_BOUND and _plan_err("vertical_8_4") <= RECT_PLAN_BOUND
    a, b = _plan_arrays(ops.stereo_rectify_plan(*RIGS["euroc"]())), _plan_arrays(ops.stereo_rectify_plan(*RIGS["euroc_4coef"]()))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    K1, D1, K2, D2, size, R, T = RR.vertical_rig()
    p8 = _plan_arrays(ops.stereo_rectify_plan(K1, D1, K2, D2, size, R, T))
    assert np.array_equal(p8["k0"], D1) and np.array_equal(p8["k1"], np.concatenate([D2, np.zeros(4)]))


def _raw_plan(K1, D1, K2, D2, size, R, T):
    lib = L.load()
    arr = lambda a: (C.c_double * np.asarray(a).size)(*np.asarray(a, np.float64).reshape(-1).tolist())      # noqa: E731
    return lib.mv_stereo_rectify_plan(C.byref(L.mvRectifyPlan()), arr(K1), arr(D1), len(D1), arr(K2), arr(D2), len(D2), size[0], size[1], arr(R), arr(T))


def test_plan_error_paths():
    K1, D1, K2, D2, size, R, T = RR.euroc_rig()
    INVALID, UNSUPPORTED = -1, -2
    assert _raw_plan(K1, D1, K2, D2, size, R, T) == L.MV_OK
    assert _raw_plan(K1, D1, K2, D2, size, R, np.zeros(3)) == INVALID
    Kn = K1.copy()
    Kn[0, 0] = np.nan
    assert _raw_plan(Kn, D1, K2, D2, size, R, T) == INVALID
    assert _raw_plan(K1, D1, K2, D2, size, R, np.array([np.inf, 0, 0])) == INVALID
    assert _raw_plan(K1, np.zeros(6), K2, D2, size, R, T) == UNSUPPORTED
    assert _raw_plan(K1, D1, K2, np.zeros(6), size, R, T) == UNSUPPORTED
    for bad in ((0, 480), (752, 0), (32769, 480), (752, 40000)):
        assert _raw_plan(K1, D1, K2, D2, bad, R, T) == INVALID
    assert _raw_plan(K1, D1, K2, D2, (32768, 1), R, T) == L.MV_OK
    with pytest.raises(L.MacvoHipError):
        ops.stereo_rectify_plan(K1, np.zeros(6), K2, D2, size, R, T)


def test_rodrigues_round_trip_in_the_plan():
    """An identity rotation (a perfectly parallel rig) and a rig rotated by almost pi/2 about the optical axis both leave R2 R R1^T = I: the rectified
    cameras are parallel."""
    K1, D1, K2, D2, size, _, _ = RR.euroc_rig()
    for R, T in ((np.eye(3), np.array([-0.11, 0.0, 0.0])), (RR.rodrigues(np.array([0.0, 0.0, 1.5])), np.array([-0.1, 0.02, 0.003])),
                 (RR.rodrigues(np.array([0.3, -0.2, 0.1])), np.array([0.01, 0.15, 0.0]))):
        p = ops.stereo_rectify_plan(K1, D1, K2, D2, size, R, T)
        assert np.abs(p.R2.numpy() @ R @ p.R1.numpy().T - np.eye(3)).max() <= 1e-14
        assert _plan_arrays(p)["baseline"][0] == pytest.approx(np.linalg.norm(T), rel=1e-12)


# ------------------------------------------------------------------------------------------------------------------------- the remap's host twin
@pytest.mark.parametrize("channels,layout", [(1, "hwc"), (3, "hwc"), (3, "planar"), (4, "hwc"), (4, "planar")])
def test_remap_twin_is_the_integer_formula(channels, layout):
    """remap_math.h replayed on the host == the numpy integer formula, bit for bit, on the crafted maps (ties to even, (-1, 0), the right and lower border,
    -1.0, 1e9, +-inf, NaN)."""
    src = RC.images(channels, layout)
    for lanes in (None, RC.LANES):
        mx, my = RC.crafted_maps(lanes=lanes, seed=3)
        for rev in (False, True):
            got = TW.remap_lanes_u8(src, mx, my, layout, rev)
            for l in range(RC.LANES):
                hwc = src[l] if layout == "hwc" else np.moveaxis(src[l], 0, -1)
                if rev and channels >= 3:
                    hwc = np.concatenate([hwc[..., 2::-1], hwc[..., 3:]], -1)
                want = np.moveaxis(RR.remap_u8(hwc, mx if lanes is None else mx[l], my if lanes is None else my[l]), -1, 0)
                assert np.array_equal(got[l], want), (lanes, rev, l)


def test_remap_quantise_rounds_half_to_even_and_refuses_what_overflows():
    assert TW.quantise(4.5 / 32) == (True, 4) and TW.quantise(5.5 / 32) == (True, 6) and TW.quantise(-0.5 / 32) == (True, 0)
    assert TW.quantise(-1.5 / 32) == (True, -2) and TW.quantise(-2.5 / 32) == (True, -2) and TW.quantise(-0.25) == (True, -8)
    assert TW.quantise(2.0 ** 25) == (True, 2 ** 30) and TW.quantise(-2.0 ** 25) == (True, -2 ** 30)
    for bad in (2.0 ** 25 + 4, -2.0 ** 25 - 4, 1e9, float("inf"), float("-inf"), float("nan"), 3e38):
        assert TW.quantise(bad) == (False, 0), bad


def test_remap_weights_are_opencvs_table():
    """For fractions in 1/32 the 15-bit weight table of the fixed-point remap holds 32 x the integer weights: they sum to 32768 (no correction step), so
    (sum of w15 * p + 2^14) >> 15 == (S + 512) >> 10 for every (fx, fy) and every tap value pattern tried."""
    rng = np.random.default_rng(0)
    p = rng.integers(0, 256, (64, 4))
    p[:4] = [[255] * 4, [0] * 4, [255, 0, 0, 255], [0, 255, 255, 0]]
    for fy in range(32):
        for fx in range(32):
            w = np.array([(32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy])
            assert w.sum() == 1024
            S = p @ w
            assert np.array_equal((S * 32 + (1 << 14)) >> 15, (S + 512) >> 10)
    u = TW.unit_table()
    assert np.array_equal(u, (np.arange(256, dtype=np.float32) / np.float32(255)))


def test_remap_twin_standalone_under_sanitizers():
    out = TW.run_standalone_sanitized()
    assert out.startswith("remap_twin OK"), out


# ------------------------------------------------------------------------------------------------------------------------- ABI, fixture
def test_abi_stays_8_and_exports_the_new_symbols():
    lib = L.load()
    assert lib.mv_abi_version() == 8 == L.ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "macvo_hip.h")).read(), flags=re.S)
    for sym in ("mv_stereo_rectify_plan", "mv_rectify_maps", "mv_remap_lanes"):
        assert hasattr(lib, sym) and sym in L.SIGNATURES and f" {sym}(" in header, sym
    assert L.MV_RM_MAX_GROUPS == int(re.search(r"#define MV_RM_MAX_GROUPS (\d+)", header).group(1))
    # the ctypes records have the C records' sizes (doubles first, no hidden padding): 21 and 2 * 21 + 44 doubles + 9 floats + 3 ints, padded to 8
    assert C.sizeof(L.mvRectifyCam) == 21 * 8 and C.sizeof(L.mvRectifyPlan) == (42 + 2 * 21 + 2) * 8 + 48 and C.sizeof(L.mvRemapGroup) == 4 * 8 + 3 * 8 + 6 * 4


def test_remap_refuses_cpu_tensors_and_bad_arguments():
    import torch

    img, m = torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4)
    with pytest.raises(L.MacvoHipError):
        ops.remap(img, (m, m))
    with pytest.raises(ValueError):
        ops.remap(img, (m, m), layout="chw")
    with pytest.raises(ValueError):
        ops.remap(img, (m, m), dtype=torch.float64)
    with pytest.raises(L.MacvoHipError):
        ops.rectify_maps(ops.stereo_rectify_plan(*RR.euroc_rig()), device="cpu")


def test_from_body_frames_is_the_datasets_T_LR():
    """StereoRectifier.from_body_frames composes inv(T_BS_r) @ T_BS_l (EuRoC.py:146): checked through the plan it would build, without a GPU."""
    import json

    import torch

    cal = json.load(open(os.path.join(ROOT, "tests", "golden", "euroc_calib.json")))
    Tl, Tr = (torch.tensor(cal[c]["T_BS"], dtype=torch.float64).reshape(4, 4) for c in ("cam0", "cam1"))
    T_LR = (torch.linalg.inv(Tr) @ Tl).numpy()
    _, _, _, _, _, R, T = RR.euroc_rig()
    assert np.abs(T_LR[:3, :3] - R).max() <= 1e-15 and np.abs(T_LR[:3, 3] - T).max() <= 1e-15
    assert abs(np.linalg.norm(T) - 0.11007) < 1e-4
