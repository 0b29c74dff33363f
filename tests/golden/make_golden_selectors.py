"""Writes tests/golden/selectors.npz: the reference's OWN RandomSelector and GridSelector classes (Module/KeypointSelector.py:103-118, 216-247) run with
``device: cpu`` under fixed ``torch.manual_seed``.  Build-container only (needs the reference checkout); imports it through
tests.golden.make_golden.import_reference.

    python tests/golden/make_golden_selectors.py

Per case (H, W, mask_width, numPoint) of tests/selectors_ref.CASES and per seed: RANDOM_CALLS successive ``select_point`` calls of the global CPU
generator, then one ``torch.randperm(RANDPERM_N)[:RANDPERM_K]`` from the same generator (the word stream continues); GridSelector's rows per case; and
for GRID_RAISES the fact that the reference raises."""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import selectors_ref as SR  # noqa: E402
from tests.golden import make_golden as MG  # noqa: E402


def main():
    KS = MG.import_reference().KS
    out = {"cases": np.array(SR.CASES, dtype=np.int64), "seeds": np.array(SR.RANDOM_SEEDS, dtype=np.int64),
           "grid_raises": np.array(SR.GRID_RAISES, dtype=np.int64)}
    for ci, (H, W, m, n) in enumerate(SR.CASES):
        frame = SimpleNamespace(height=H, width=W)
        cfg = SimpleNamespace(mask_width=m, device="cpu")
        KS.RandomSelector.is_valid_config(cfg)
        KS.GridSelector.is_valid_config(cfg)
        out[f"grid_{ci}"] = KS.GridSelector(cfg).select_point(frame, n, None, None, None)
        assert out[f"grid_{ci}"].dtype == torch.int64
        for seed in SR.RANDOM_SEEDS:
            torch.manual_seed(seed)
            sel = KS.RandomSelector(cfg)
            rows = torch.stack([sel.select_point(frame, n, None, None, None) for _ in range(SR.RANDOM_CALLS)])
            assert rows.dtype == torch.int64 and rows.shape == (SR.RANDOM_CALLS, n, 2)
            out[f"random_{ci}_{seed}"] = rows
            out[f"randperm_{ci}_{seed}"] = torch.randperm(SR.RANDPERM_N)[: SR.RANDPERM_K]
    raised = []
    for (H, W, m, n) in SR.GRID_RAISES:
        try:
            KS.GridSelector(SimpleNamespace(mask_width=m, device="cpu")).select_point(SimpleNamespace(height=H, width=W), n, None, None, None)
            raised.append(0)
        except (ZeroDivisionError, RuntimeError):
            raised.append(1)
    out["grid_raised"] = np.array(raised, dtype=np.int64)
    MG.save("selectors", **out)


if __name__ == "__main__":
    main()
