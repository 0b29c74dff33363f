"""The cameras of the intrinsics tests, defined once (a plain module: no fixtures).  Every other camera of the suite has fx == fy, almost always
fx = fy = 320 with the principal point at the image centre and a 0.25 m baseline; these do not.

``EUROC``        the EuRoC MAV cam0 calibration: 0.3 % anisotropy, a real camera
``KITTI``        the KITTI odometry (sequence 00) calibration: fx == fy, but a principal point far from the centre and baseline * fx = 388 instead of 80
``ANISO``        strongly anisotropic, so that tolerances at fp32 level still tell fx from fy
``ANISO_SMALL``  the same idea at the frame size of the driver tests (240 x 320)"""
from types import SimpleNamespace as _NS


def _cam(name, fx, fy, cx, cy, baseline, W, H):
    return _NS(name=name, fx=fx, fy=fy, cx=cx, cy=cy, baseline=baseline, W=W, H=H, K=(fx, fy, cx, cy))


EUROC = _cam("EUROC", 458.654, 457.296, 367.215, 248.375, 0.11, 752, 480)
KITTI = _cam("KITTI", 718.856, 718.856, 607.1928, 185.2157, 0.54, 1241, 376)
ANISO = _cam("ANISO", 300.0, 380.0, 290.5, 260.25, 0.25, 640, 480)
ANISO_SMALL = _cam("ANISO_SMALL", 150.0, 190.0, 151.25, 127.5, 0.4, 320, 240)

BY_NAME = {c.name: c for c in (EUROC, KITTI, ANISO, ANISO_SMALL)}


def cam_dict(c, H=None, W=None):
    """The dict form ``tools.synth.make_sequence`` / ``pipeline.Camera`` / ``OracleHotPath`` take (the keys of ``tools.synth.make_camera``)."""
    return dict(fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy, baseline=c.baseline, H=c.H if H is None else H, W=c.W if W is None else W)


def K_matrix(c):
    import torch

    return torch.tensor([[c.fx, 0, c.cx], [0, c.fy, c.cy], [0, 0, 1]], dtype=torch.float32)
