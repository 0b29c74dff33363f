"""Writes tests/golden/grad_selectors.npz: the reference's OWN GradientSelector, SparseGradienSelector and SelectorCompose classes
(Module/KeypointSelector.py:121-158, :161-213, :51-75) run on the CPU under fixed ``torch.manual_seed``.  Build-container only (needs the reference
checkout); imports it through tests.golden.make_golden.import_reference.

    python tests/golden/make_golden_grad_selectors.py

The inputs are small uint8 images (tests/grad_selectors_ref.quantised_u8), stored in the file and fed as ``k / 256`` fp32, on which every step of the
selectors is exact; the file keeps the images and the selected rows only."""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import grad_selectors_ref as GR  # noqa: E402
from tests.golden import make_golden as MG  # noqa: E402


def _frame(u8: np.ndarray):
    img = torch.from_numpy(u8.astype(np.float32)) / 256.0
    return NS(imageL=img.unsqueeze(0), height=u8.shape[1], width=u8.shape[2])


def main():
    KS = MG.import_reference().KS
    out = {}
    images = {}
    for ci, (H, W, iseed, m, gs, nms, n, seed) in enumerate(GR.GOLDEN_CASES):
        key = f"image_{H}x{W}_{iseed}"
        if key not in images:
            images[key] = GR.quantised_u8(H, W, iseed)
            out[key] = images[key]
        if nms is None:
            cfg = NS(mask_width=m, grad_std=gs)
            KS.GradientSelector.is_valid_config(cfg)
            sel = KS.GradientSelector(cfg)
        else:
            cfg = NS(mask_width=m, grad_std=gs, nms_size=nms)
            KS.SparseGradienSelector.is_valid_config(cfg)
            sel = KS.SparseGradienSelector(cfg)
        torch.manual_seed(seed)
        rows = sel.select_point(_frame(images[key]), n, None, None, None)
        assert rows.dtype == torch.int64 and rows.shape[1] == 2
        out[f"rows_{ci}"] = rows
        print(ci, (H, W, m, gs, nms, n), "->", tuple(rows.shape))
    c = GR.GOLDEN_COMPOSE
    cfg = NS(selector_args=[NS(type="GradientSelector", args=NS(mask_width=c["mask_width"], grad_std=c["grad_std"])),
                            NS(type="SparseGradienSelector", args=NS(mask_width=c["mask_width"], grad_std=c["grad_std"], nms_size=c["nms_size"]))],
             weight=list(c["weight"]))
    KS.SelectorCompose.is_valid_config(cfg)
    sel = KS.SelectorCompose(cfg)
    torch.manual_seed(c["seed"])
    out["compose_rows"] = sel.select_point(_frame(images[f"image_{c['H']}x{c['W']}_{c['image_seed']}"]), c["num_point"], None, None, None)
    print("compose ->", tuple(out["compose_rows"].shape))
    MG.save("grad_selectors", **out)


if __name__ == "__main__":
    main()
