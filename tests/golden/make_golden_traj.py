"""Writes tests/golden/traj_eval.npz: the 1360 ground-truth poses of the reference's unit-test sequence
(``Scripts/UnitTest/assets/test_sequence/TartanAir2_abs_P000/pose_lcam_front.txt``, rows tx ty tz qx qy qz qw, 76 KB as fp64), an estimate made from
them by a seeded per-step perturbation (``tests.traj_ref.perturb``), and what ``tests/traj_ref.py`` — the restatement of evo's definition,
UNPINNED: evo is not importable, so no evo run stands behind these rows — gives for that pair in all three alignment modes, with and without scale
correction.  Build-container only (it reads the reference checkout).

    python tests/golden/make_golden_traj.py [path/to/reference]
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import traj_ref as TR  # noqa: E402

ASSET = os.path.join("Scripts", "UnitTest", "assets", "test_sequence", "TartanAir2_abs_P000", "pose_lcam_front.txt")
MODES = ("umeyama", "origin", "none")


def main() -> None:
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MACVO_REFERENCE", "/root/reference")
    gt = np.loadtxt(os.path.join(ref_root, ASSET), dtype=np.float64)
    assert gt.shape == (1360, 7), gt.shape
    est = TR.perturb(gt, seed=2024, trans=0.004, rot=0.0005)
    out = {"gt": gt, "est": est}
    for mode in MODES:
        for scale in (False, True):
            r = TR.evaluate(est, gt, mode, scale)
            tag = f"{mode}_{int(scale)}"
            out["rows_" + tag] = np.array(TR.stats_row(r))
            out["align_" + tag] = np.concatenate([r["R"].reshape(-1), r["t"], [r["c"]], r["d"]])
            print(tag, "d =", r["d"], "ATE mean %.4f m, RTE mean %.5f m, ROE mean %.5f deg" % (r["stats"]["ate"]["mean"], r["stats"]["rte"]["mean"],
                                                                                              r["stats"]["roe"]["mean"]))
    path = os.path.join(ROOT, "tests", "golden", "traj_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
