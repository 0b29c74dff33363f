"""CPU: the torch restatement (tests/cov_models_ref.py) reproduces the reference's GaussianMixtureCovariance / NoCovariance /
modifier outputs recorded in tests/golden/cov_models.npz; the packing of the modifier chain and the `cov.obs` mapping of
HotPathConfig."""
import os

import numpy as np
import pytest
import torch

from tests import cov_models_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cov_models.npz")


@pytest.fixture(scope="module")
def g():
    z = np.load(GOLD)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def test_gmm_restatement_matches_reference_golden(g):
    K = tuple(float(x) for x in g["K"])
    fc = g["flow_cov_in"].clone()
    cov, w = R.gmm_covariance(g["kp_int"], g["depth"], g["dcov"], None, fc, *K, return_weights=True)
    torch.testing.assert_close(cov, g["gmm_int_flowcov"], rtol=1e-5, atol=1e-9)
    assert torch.equal(fc, g["gmm_flow_cov_after"])
    torch.testing.assert_close(w, g["gmm_weights"], rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(R.gmm_covariance(g["kp_float"], g["depth"], g["dcov"], None, g["flow_cov_in"].clone(), *K),
                               g["gmm_float_flowcov"], rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(R.gmm_covariance(g["kp_int"], g["depth"], g["dcov"], g["depth_cov_kp"], None, *K),
                               g["gmm_int_nodefault"], rtol=1e-5, atol=1e-9)
    s0 = torch.ones(48, 3) * 0.25
    s0[:, 2] = 0
    torch.testing.assert_close(R.gmm_covariance(g["kp_int"], g["depth"], g["dcov"], g["depth_cov_kp"], s0, *K),
                               g["gmm_int_default_sigma"], rtol=1e-5, atol=1e-9)
    # the broad rows put weights on both sides of the threshold, and the variance carries the /2 (no clamp)
    assert ((w[40:46] < 1e-3) & (w[40:46] > 0)).any() and (w[40:46] >= 1e-3).any()


def test_none_and_modifiers_match_reference_golden(g):
    assert torch.equal(g["none"], R.no_covariance(48)) and torch.equal(g["none_flow_cov_after"], g["flow_cov_in"])
    m = g["match_float_flowcov"]
    for key, chain in (("diag_match", ("diag",)), ("norm_match", ("normalize",)), ("norm_diag_match", ("diag", "normalize")),
                       ("diag_norm_match", ("normalize", "diag"))):
        torch.testing.assert_close(R.apply_chain(m, chain), g[key], rtol=1e-12, atol=0)
    assert not torch.allclose(g["norm_diag_match"], g["diag_norm_match"])      # order matters
    torch.testing.assert_close(R.apply_chain(g["gmm_float_flowcov"], ("diag",)), g["diag_gmm"], rtol=0, atol=0)


def test_modifier_chain_packing_and_cov_obs_mapping():
    from types import SimpleNamespace as NS

    from macvo_amd import ops
    from macvo_amd.pipeline import HotPathConfig, cov_config_fields

    assert ops.cov_modifier_chain(()) == 0
    assert ops.cov_modifier_chain(("diag", "normalize")) == 1 | (2 << 4)
    with pytest.raises(ValueError):
        ops.cov_modifier_chain(("diag",) * 5)
    with pytest.raises(ValueError):
        ops.cov_modifier_chain(("cube_root",))
    args = NS(kernel_size=31, match_cov_default=0.25, min_flow_cov=0.25, min_depth_cov=0.05, device="cuda")
    blk = NS(type="Modifier_Normalize", args=NS(type="Modifier_Diagonalize", args=NS(type="MatchCovariance", args=args)))
    f = cov_config_fields(blk)
    assert f["cov_model"] == "match" and f["cov_modifiers"] == ("diag", "normalize") and f["cov_kernel_size"] == 31
    HotPathConfig(**f)
    assert cov_config_fields({"type": "NoCovariance", "args": None}) == {"cov_model": "none", "cov_modifiers": ()}
    assert cov_config_fields(NS(type="Modifier_Diagonalize", args=NS(type="GaussianMixtureCovariance", args=args)))["cov_model"] == "gmm"
    with pytest.raises(ValueError):
        cov_config_fields(NS(type="DepthCovariance", args=NS(regularization=1e-5)))


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from tests.test_reference_abcs import REF  # noqa: E402  (the reference checkout the ABC test uses)

ABLATION_SCRIPT = r'''
import sys, glob
from pathlib import Path
sys.path.insert(0, %(root)r)
from tests.golden import make_golden as MG
MG.import_reference()
import Module
import macvo_amd.plugins as P
from macvo_amd.pipeline import cov_config_fields
from Utility.Config import load_config
for name in ("HIP_GaussianMixtureCovariance", "HIP_NoCovariance", "HIP_Modifier_Diagonalize", "HIP_Modifier_Normalize"):
    cls = Module.ICovariance2to3.get_class(name)
    assert cls is getattr(P, name) and issubclass(cls, Module.ICovariance2to3), name
seen = set()
for f in sorted(glob.glob(str(Path(%(ref)r) / "Config/Experiment/MACVO/Ablation_Study/*.yaml"))):
    cfg, _ = load_config(Path(f))
    obs = cfg.Odometry.cov.obs
    node = obs
    while True:                                   # swap only the type: strings
        if not node.type.startswith("HIP_"):
            node.type = "HIP_" + node.type
        if node.type.startswith("HIP_Modifier_"):
            node = node.args
        else:
            break
    Module.ICovariance2to3.is_valid_config(obs)
    m = Module.ICovariance2to3.instantiate(obs.type, obs.args)
    assert type(m).__name__ == obs.type, (f, type(m))
    seen.add((cov_config_fields(obs)["cov_model"], cov_config_fields(obs)["cov_modifiers"]))
assert {("match", ("diag",)), ("match", ("normalize",)), ("match", ("diag", "normalize")), ("none", ())} <= seen, seen
print("OK", sorted(seen))
'''


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "Module")), reason="needs the reference checkout (build container only)")
def test_ablation_configs_instantiate_hip_covariance_models(tmp_path):
    import subprocess
    import sys

    script = tmp_path / "ablation.py"
    script.write_text(ABLATION_SCRIPT % {"root": ROOT, "ref": REF})
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
