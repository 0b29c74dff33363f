"""TEST INFRASTRUCTURE: reads tests/golden/keyframe_run.npz (tests/golden/make_golden_local_keyframe.py).

Rows that do not depend on the pose — keypoints, gathered values, camera-frame covariances — are the same bits whatever the optimizer, so the
generator stores a table that equals another one as a reference (``meta["same"]``: key -> [file or "", key]); ``case`` resolves them."""
from __future__ import annotations

import json
import os

import numpy as np

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_files: dict = {}


def _file(name: str):
    if name not in _files:
        _files[name] = np.load(os.path.join(GOLD_DIR, name))
    return _files[name]


def meta() -> dict:
    return json.loads(str(_file("keyframe_run.npz")["meta"]))


def case(name: str) -> dict:
    """Every table of case ``name``, references resolved, keyed as in ``tensor_map.npz`` with the ``map/`` prefix of tests/refrun."""
    z = _file("keyframe_run.npz")
    out = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}
    for k, (f, src) in meta()["same"].items():
        if k.startswith(name + "/"):
            out[k[len(name) + 1:]] = _file(f or "keyframe_run.npz")[src]
    return out
