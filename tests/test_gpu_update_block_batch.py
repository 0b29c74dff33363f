"""GPU: the update blocks with more images than a grid's y or z dimension holds (65 535): the layout kernel carries the image index in x."""
from __future__ import annotations

import pytest
import torch

from tests import update_block_twin as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", [T.COV, T.FLOW], ids=["cov", "flow"])
def test_more_images_than_a_grid_dimension_holds(gpu, kind):
    """B = 65 537 one-pixel images in one call against the same images in two calls of at most 32 769: every pixel's sum runs in a fixed order that does
    not depend on its place in the batch, so the bits are equal; and the first 35 images equal the twin's within its bar."""
    from macvo_amd import ops

    c = T.case(kind, "bf16", (1, 5, 7))
    w = ops.UpdateBlockWeights.from_module({k: v.to(gpu) for k, v in c.sd.items()}, "cov" if kind == T.COV else "flow", "bf16")
    B = 65537
    net, inp = (t.to(c.dt).to(gpu) for t in T.make_inputs((B, 1, 1), 9))
    whole = ops.update_block(net, inp, w)
    half = B // 2
    parts = [ops.update_block(net[s], inp[s], w) for s in (slice(0, half), slice(half, B))]
    torch.cuda.synchronize()
    for i, name in enumerate(T.OUTPUTS):
        assert torch.equal(whole[i].view(torch.int16), torch.cat([p[i] for p in parts]).view(torch.int16)), name
    twin, scale = T.twin_outputs(c.sd, kind, net[:35].cpu(), inp[:35].cpu(), c.dt)
    for i, name in enumerate(T.OUTPUTS):
        d = float((whole[i][:35].float().cpu() - twin[i].float()).abs().max())
        print(f"{name}: max |kernel - twin| = {d / (T.ULP['bf16'] * scale[i]):.2f} ulp(scale)")
        assert d <= 2 * T.ULP["bf16"] * scale[i], (name, d)
