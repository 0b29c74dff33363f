"""Writes tests/golden/cov_update_block.npz: the reference's OWN ``CovUpdateBlock`` (Module/Network/FlowFormerCov/covhead.py:24-43) on the CPU in fp32
and fp64, for one seeded weight set and one small seeded input.  Build-container only (needs the reference checkout; the files are loaded in place).

covhead.py's first two imports point into the FlowFormer submodule, which the checkout lacks: ``MemoryDecoder`` and ``initialize_flow`` are inert
placeholders here, and ``SepConvGRU`` is the in-tree class of Module/Network/PWCNet/pwc_cov/gru.py:90 behind FlowFormer's signature — the in-tree class takes
the TOTAL input channels, FlowFormer's takes ``hidden_dim`` and ``input_dim`` and builds ``hidden_dim + input_dim`` wide convolutions.  The weights are copied
from a seeded ``tools.flowformer_host.CovUpdateBlock`` (same keys, same shapes), so the fixture holds the seed, the SHA-256 of that state dict, the input
and the three outputs; no weights are stored.

    python tests/golden/make_golden_update_block.py
"""
from __future__ import annotations

import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SEED, SHAPE = 0, (1, 5, 7)
N_PARAMS = 3075202


def state_dict_sha256(sd) -> str:
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _load(name: str, path: str):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_class(ref_root: str):
    net = os.path.join(ref_root, "Module", "Network")
    for pkg in ("_mvref", "_mvref.PWCNet", "_mvref.PWCNet.pwc_cov", "_mvref.FlowFormer", "_mvref.FlowFormer.core", "_mvref.FlowFormerCov"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    att = types.ModuleType("_mvref.PWCNet.pwc_cov.attention")
    att.AttentionLayer = object
    sys.modules[att.__name__] = att
    ref_gru = _load("_mvref.PWCNet.pwc_cov.gru", os.path.join(net, "PWCNet", "pwc_cov", "gru.py"))

    gru = types.ModuleType("_mvref.FlowFormer.core.gru")
    gru.SepConvGRU = lambda hidden_dim=128, input_dim=192 + 128: ref_gru.SepConvGRU(hidden_dim=hidden_dim, input_dim=hidden_dim + input_dim)
    dec = types.ModuleType("_mvref.FlowFormer.core.decoder")
    dec.MemoryDecoder = torch.nn.Module
    dec.initialize_flow = lambda *a, **k: None
    sys.modules[gru.__name__], sys.modules[dec.__name__] = gru, dec
    return _load("_mvref.FlowFormerCov.covhead", os.path.join(net, "FlowFormerCov", "covhead.py")).CovUpdateBlock


def main():
    from tests import update_block_twin as T
    from tests.golden.make_golden import REF

    block_cls = reference_class(REF)
    sd = T.make_block(T.COV, SEED).state_dict()
    net, inp = T.make_inputs(SHAPE, SEED)
    out = {"seed": np.array(SEED), "shape": np.array(SHAPE), "sha": np.array(state_dict_sha256(sd)), "net": net.numpy(), "inp": inp.numpy()}
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        block = block_cls(None, hidden_dim=128)
        assert list(block.state_dict()) == list(sd), "the canonical tensor order is the reference's state_dict() order"
        assert sum(p.numel() for p in block.parameters()) == N_PARAMS
        block.load_state_dict(sd, strict=True)
        block = block.to(dt).eval()
        with torch.no_grad():
            res = block(net.to(dt), inp.to(dt))
        for name, t in zip(T.OUTPUTS, res):
            out[f"{tag}_{name}"] = t.numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cov_update_block.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
