"""GPU: RandomSelector / GridSelector as HIP launches (ops.kp_random, ops.kp_grid) against torch.randint on CPU generators seeded alike and the
reference classes' golden rows, bit for bit; the HIP_RandomSelector / HIP_GridSelector plugins (against the reference's own classes where its
byte-compiled tree is present)."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import selectors_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    z = np.load(os.path.join(ROOT, "tests", "golden", "selectors.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("H,W,mask,n,calls", [(480, 640, 32, 200, 10), (720, 1280, 0, 512, 4), (96, 128, 5, 1, 9), (192, 256, 16, 313, 7)])
def test_kp_random_is_torch_randint_over_calls_and_lanes(gpu, H, W, mask, n, calls):
    """One workgroup per lane, generators advanced in place: `calls` successive calls of every lane equal torch.randint of CPU generators seeded
    alike (v rows first, then u), block boundaries included (10 x 400 words; 512 rows = 1024 words per call); afterwards a lane's state continues
    as torch.randperm does (mv_randperm_head_lanes on the same state)."""
    from macvo_amd import _lib as L
    from macvo_amd import ops

    seeds = [5, 7, 99, 1234, 2 ** 33 + 5]
    state = ops.mt19937_state(seeds, gpu)
    gens = [torch.Generator().manual_seed(s) for s in seeds]
    for c in range(calls):
        out = ops.kp_random(state, n, H, W, mask)
        torch.cuda.synchronize()
        assert out.shape == (len(seeds), n, 2) and out.dtype == torch.int64
        for l, gen in enumerate(gens):
            assert torch.equal(out[l].cpu(), SR.random_select(n, H, W, mask, gen)), (c, l)
    lib = L.load()
    cnt = torch.tensor([[7000, 0, 0, 0]] * len(seeds), dtype=torch.int32, device=gpu)
    perm = torch.full((len(seeds), 200), -1, dtype=torch.int64, device=gpu)
    nsel = torch.zeros(len(seeds), dtype=torch.int32, device=gpu)
    L.check(lib.mv_randperm_head_lanes(state.data_ptr(), cnt.data_ptr(), 4, len(seeds), 200, 200, perm.data_ptr(), nsel.data_ptr(), 1, None),
            "mv_randperm_head_lanes")
    torch.cuda.synchronize()
    for l, gen in enumerate(gens):
        assert torch.equal(perm[l].cpu(), torch.randperm(7000, generator=gen)[:200]), l


def test_kp_random_golden_and_argument_checks(gpu, g):
    from macvo_amd import ops

    for ci, (H, W, m, n) in enumerate(SR.CASES):
        if n > 512:
            with pytest.raises(ValueError):
                ops.kp_random(ops.mt19937_state([1], gpu), n, H, W, m)
            continue
        state = ops.mt19937_state(list(SR.RANDOM_SEEDS), gpu)
        rows = torch.stack([ops.kp_random(state, n, H, W, m) for _ in range(SR.RANDOM_CALLS)], dim=1).cpu()
        for l, seed in enumerate(SR.RANDOM_SEEDS):
            assert torch.equal(rows[l], torch.from_numpy(g[f"random_{ci}_{seed}"])), (ci, seed)
    with pytest.raises(ValueError):
        ops.kp_random(ops.mt19937_state([1], gpu), 10, 64, 640, 32)
    with pytest.raises(ValueError):
        ops.kp_random(torch.zeros(3, 5, dtype=torch.int32, device=gpu), 10, 480, 640, 32)


def test_kp_grid_equals_golden(gpu, g):
    from macvo_amd import ops

    for ci, (H, W, m, n) in enumerate(SR.CASES):
        want = torch.from_numpy(g[f"grid_{ci}"])
        assert ops.kp_grid_count(H, W, m, n) == want.shape[0]
        got = ops.kp_grid(H, W, m, n, gpu)
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), want), SR.CASES[ci]
    for (H, W, m, n) in SR.GRID_RAISES:
        with pytest.raises(ValueError):
            ops.kp_grid(H, W, m, n, gpu)


def test_plugins_draw_the_reference_rows(gpu, g):
    """Unseeded HIP_RandomSelector = torch's global CPU generator (the reference class's golden rows, then the same randperm); seeded = a device
    generator with the bits of torch.Generator().manual_seed(seed); HIP_GridSelector = the golden grid."""
    import macvo_amd.plugins as P

    H, W, m, n = SR.CASES[0]
    frame = SimpleNamespace(height=H, width=W)
    seed = SR.RANDOM_SEEDS[0]
    sel = P.HIP_RandomSelector(SimpleNamespace(mask_width=m, device="cuda"))
    torch.manual_seed(seed)
    rows = [sel.select_point(frame, n, None, None, None) for _ in range(SR.RANDOM_CALLS)]
    assert all(r.is_cuda and r.dtype == torch.int64 for r in rows)
    assert torch.equal(torch.stack(rows).cpu(), torch.from_numpy(g[f"random_0_{seed}"]))
    assert torch.equal(torch.randperm(SR.RANDPERM_N)[: SR.RANDPERM_K], torch.from_numpy(g[f"randperm_0_{seed}"]))
    seeded = P.HIP_RandomSelector(SimpleNamespace(mask_width=m, device="cuda", seed=seed))
    before = torch.get_rng_state()
    rows = torch.stack([seeded.select_point(frame, n, None, None, None) for _ in range(SR.RANDOM_CALLS)])
    assert torch.equal(rows.cpu(), torch.from_numpy(g[f"random_0_{seed}"]))
    assert torch.equal(torch.get_rng_state(), before)        # the global generator did not move
    grid = P.HIP_GridSelector(SimpleNamespace(mask_width=m, device="cuda")).select_point(frame, n, None, None, None)
    assert grid.is_cuda and grid.shape == (231, 2) and torch.equal(grid.cpu(), torch.from_numpy(g["grid_0"]))


_REF_SCRIPT = r"""
import sys
from types import SimpleNamespace as NS
import torch
sys.path.insert(0, {root!r})
from tests import refrun
refrun.import_reference()
import Module.KeypointSelector as KS
import macvo_amd.plugins as P
for (H, W, m, n) in [(480, 640, 32, 200), (720, 1280, 32, 200), (480, 640, 0, 200), (192, 256, 16, 50)]:
    frame = NS(height=H, width=W)
    ref_r, ref_g = KS.RandomSelector(NS(mask_width=m, device="cpu")), KS.GridSelector(NS(mask_width=m, device="cpu"))
    hip_r, hip_g = P.HIP_RandomSelector(NS(mask_width=m, device="cuda")), P.HIP_GridSelector(NS(mask_width=m, device="cuda"))
    torch.manual_seed(11)
    a = [ref_r.select_point(frame, n, None, None, None) for _ in range(6)] + [torch.randperm(5000)[:100]]
    torch.manual_seed(11)
    b = [hip_r.select_point(frame, n, None, None, None).cpu() for _ in range(6)] + [torch.randperm(5000)[:100]]
    assert all(torch.equal(x, y) for x, y in zip(a, b)), (H, W, m, n)
    assert torch.equal(ref_g.select_point(frame, n, None, None, None), hip_g.select_point(frame, n, None, None, None).cpu())
print("SELECTOR_PLUGINS_OK")
"""


def test_plugins_against_the_reference_classes(gpu):
    from tests import refrun

    root = refrun.reference_root()
    if root is None or not any(os.path.exists(os.path.join(root, "Module", "KeypointSelector" + ext)) for ext in (".py", ".pyc")):
        pytest.skip("needs the byte-compiled reference tree (oracle/_ref/pyref: python oracle/build_ref.py)")
    r = subprocess.run([sys.executable, "-c", _REF_SCRIPT.format(root=ROOT)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "SELECTOR_PLUGINS_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
