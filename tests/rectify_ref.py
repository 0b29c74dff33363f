"""TEST INFRASTRUCTURE: numpy restatement of stereo rectification — Bouguet's rectifying rotations and projection matrices as OpenCV's ``stereoRectify`` does
them on its ``alpha < 0``, ``CALIB_ZERO_DISPARITY`` path, the ``initUndistortRectifyMap`` formula and the 8-bit fixed-point ``remap`` (``INTER_LINEAR``,
``BORDER_CONSTANT`` 0) — written from the formulae in ``include/macvo_hip.h``, all in fp64 / integers.

OpenCV is RESTATED, PARITY-UNPINNED (it is no dependency here).  One known difference: OpenCV keeps the four undistorted image corners in float32, this file
and the C plan keep them in double, so the principal point agrees with OpenCV's to about 1e-4 px.  One figure pins the restatement to the reference: EuRoC's
calibration gives the baseline the reference hard-codes (DataLoader/Dataset/EuRoC.py:76), tests/test_rectify_host.py."""
from __future__ import annotations

import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rodrigues(v: np.ndarray) -> np.ndarray:
    """Rotation vector -> matrix: I + sin(th) [k]x + (1 - cos(th)) [k]x^2."""
    v = np.asarray(v, np.float64)
    th = float(np.linalg.norm(v))
    if th < 1e-300:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def inv_rodrigues(R: np.ndarray) -> np.ndarray:
    """Rotation matrix -> vector (angles away from pi: every rig's cameras look the same way)."""
    R = np.asarray(R, np.float64)
    r = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.linalg.norm(r)), 0.5 * (np.trace(R) - 1.0)
    if s == 0.0:
        return np.zeros(3)
    return r * (np.arctan2(s, c) / s)


def coeffs8(D) -> np.ndarray:
    """k1 k2 p1 p2 [k3 [k4 k5 k6]] -> all eight, missing ones 0."""
    D = np.asarray(D, np.float64).reshape(-1)
    assert D.size in (4, 5, 8), D.size
    out = np.zeros(8)
    out[:D.size] = D
    return out


def distort(x, y, D8):
    """The forward camera model on normalised coordinates."""
    k1, k2, p1, p2, k3, k4, k5, k6 = D8
    r2 = x * x + y * y
    kr = (1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 * r2 + k6 * r2 ** 3)
    return x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y


def undistort_point(u, v, K, D8, iters: int = 5):
    """Five fixed-point iterations of the inverse model."""
    k1, k2, p1, p2, k3, k4, k5, k6 = D8
    x0, y0 = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    x, y = x0, y0
    for _ in range(iters):
        r2 = x * x + y * y
        ik = (1 + k4 * r2 + k5 * r2 * r2 + k6 * r2 ** 3) / (1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 ** 3)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * ik, (y0 - dy) * ik
    return x, y


def plan(K1, D1, K2, D2, size, R, T) -> dict:
    """-> dict(R1, R2, P1, P2, idx, fc, baseline, K (fp32 3 x 3), cams = [dict(iR, fx, fy, cx, cy, k)] * 2)."""
    K1, K2, R, T = (np.asarray(a, np.float64) for a in (K1, K2, R, T))
    D = [coeffs8(D1), coeffs8(D2)]
    nx, ny = size
    om = inv_rodrigues(R)
    rr = rodrigues(-0.5 * om)
    t = rr @ T
    idx = 0 if abs(t[0]) > abs(t[1]) else 1
    c, nt = t[idx], float(np.linalg.norm(t))
    uu = np.zeros(3)
    uu[idx] = 1.0 if c > 0 else -1.0
    ww = np.cross(t, uu)
    nw = float(np.linalg.norm(ww))
    if nw > 0:
        ww = ww * (np.arccos(abs(c) / nt) / nw)
    wR = rodrigues(ww)
    R1, R2 = wR @ rr.T, wR @ rr
    tn = R2 @ T
    fc = np.inf
    for K, d in ((K1, D[0]), (K2, D[1])):
        f = K[idx ^ 1, idx ^ 1]
        if d[0] < 0:
            f = f * (1 + d[0] * (nx * nx + ny * ny) / (4 * f * f))
        fc = min(fc, f)
    cc = []
    for K, d, Rk in ((K1, D[0], R1), (K2, D[1], R2)):
        acc = np.zeros(2)
        for i in range(4):
            x, y = undistort_point((i % 2) * (nx - 1.0), (i // 2) * (ny - 1.0), K, d)
            p = Rk @ np.array([x, y, 1.0])
            acc += np.array([fc * p[0] / p[2], fc * p[1] / p[2]])
        cc.append(np.array([(nx - 1) / 2.0, (ny - 1) / 2.0]) - acc / 4.0)
    ccm = 0.5 * (cc[0] + cc[1])
    P1 = np.array([[fc, 0, ccm[0], 0], [0, fc, ccm[1], 0], [0, 0, 1, 0.0]])
    P2 = P1.copy()
    P2[idx, 3] = tn[idx] * fc
    cams = []
    for K, d, Rk, P in ((K1, D[0], R1, P1), (K2, D[1], R2, P2)):
        cams.append(dict(iR=np.linalg.inv(P[:, :3] @ Rk), fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], k=d))
    return dict(R1=R1, R2=R2, P1=P1, P2=P2, idx=idx, fc=fc, baseline=abs(P2[idx, 3] / fc), K=P1[:, :3].astype(np.float32), cams=cams)


def maps(cam: dict, out_h: int, out_w: int):
    """fp64 (map_x, map_y) [out_h, out_w] of one camera of a plan."""
    v, u = np.meshgrid(np.arange(out_h, dtype=np.float64), np.arange(out_w, dtype=np.float64), indexing="ij")
    iR = cam["iR"]
    x = iR[0, 0] * u + iR[0, 1] * v + iR[0, 2]
    y = iR[1, 0] * u + iR[1, 1] * v + iR[1, 2]
    w = iR[2, 0] * u + iR[2, 1] * v + iR[2, 2]
    xd, yd = distort(x / w, y / w, cam["k"])
    return cam["fx"] * xd + cam["cx"], cam["fy"] * yd + cam["cy"]


def remap_u8(src: np.ndarray, map_x: np.ndarray, map_y: np.ndarray) -> np.ndarray:
    """The 8-bit fixed-point bilinear remap in integers.  src uint8 [H, W] or [H, W, C]; maps fp32 [h, w] -> uint8 [h, w(, C)].

    s = rndne(map * 32) in fp32; i = s >> 5 (floor), f = s & 31; a tap outside the source counts 0 on its own; out = (sum of weight * tap + 512) >> 10.
    A NaN entry, or one whose * 32 leaves [-2^30, 2^30], yields 0."""
    H, W = src.shape[:2]
    im = src.reshape(H, W, -1).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = np.asarray(map_x, np.float32) * np.float32(32), np.asarray(map_y, np.float32) * np.float32(32)
        ok = (qx >= -2.0 ** 30) & (qx <= 2.0 ** 30) & (qy >= -2.0 ** 30) & (qy <= 2.0 ** 30)       # (NaN fails every comparison)
        sx = np.rint(np.where(ok, qx, 0)).astype(np.int64)
        sy = np.rint(np.where(ok, qy, 0)).astype(np.int64)
    ix, iy, fx, fy = sx >> 5, sy >> 5, sx & 31, sy & 31

    def tap(y, x):
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return im[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)] * inside[..., None]

    wx, wy = fx[..., None], fy[..., None]
    S = (32 - wx) * (32 - wy) * tap(iy, ix) + wx * (32 - wy) * tap(iy, ix + 1) + (32 - wx) * wy * tap(iy + 1, ix) + wx * wy * tap(iy + 1, ix + 1)
    out = ((S + 512) >> 10) * ok[..., None]
    return out.astype(np.uint8).reshape(map_x.shape + src.shape[2:])


def euroc_rig():
    """EuRoC's public calibration (tests/golden/euroc_calib.json) as the arguments of ``plan``: K1, D1, K2, D2, size, R, T with T_LR = inv(T_BS_r) @ T_BS_l."""
    cal = json.load(open(os.path.join(ROOT, "tests", "golden", "euroc_calib.json")))

    def Kof(i):
        return np.array([[i[0], 0, i[2]], [0, i[1], i[3]], [0, 0, 1.0]])

    Tl, Tr = (np.array(cal[c]["T_BS"], np.float64).reshape(4, 4) for c in ("cam0", "cam1"))
    TLR = np.linalg.inv(Tr) @ Tl
    return (Kof(cal["cam0"]["intrinsics"]), np.array(cal["cam0"]["distortion"]), Kof(cal["cam1"]["intrinsics"]), np.array(cal["cam1"]["distortion"]),
            tuple(cal["resolution"]), TLR[:3, :3], TLR[:3, 3])


def vertical_rig():
    """A rig whose second camera sits below the first (idx = 1), slightly rotated, 8 coefficients on one camera and 4 on the other."""
    K1 = np.array([[410.0, 0, 322.5], [0, 395.0, 236.0], [0, 0, 1.0]])
    K2 = np.array([[405.0, 0, 318.0], [0, 401.0, 243.5], [0, 0, 1.0]])
    D1 = np.array([-0.21, 0.05, 3e-4, -2e-4, 0.01, 0.02, -0.01, 0.003])
    D2 = np.array([0.08, -0.02, -1e-4, 4e-4])
    R = rodrigues(np.array([0.012, -0.02, 0.015]))
    T = np.array([0.004, -0.2, 0.006])
    return K1, D1, K2, D2, (640, 480), R, T
