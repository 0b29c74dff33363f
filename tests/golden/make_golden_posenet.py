"""Writes tests/golden/posenet.npz: the reference's OWN PoseNet class — ``VOFlowRes(intrinsic=True, down_scale=True, config=1, stereo=True,
autoDistTarget=0.)`` of Module/Network/TartanVOStereo/FlowPoseNet.py, as StereoVO.py:21 constructs it — on CPU in fp32 and fp64, for two
seeded weight sets and a seeded 3-lane input.  Build-container only (needs the reference checkout; the file is loaded in place, it imports
nothing but torch).  Weights and input are regenerated from seeds (tools/posenet_torch.py), so the fixture holds the seeds, the SHA-256 of
each generated state dict, the ``[3,6]`` outputs and 512 sampled values of each of the six stage outputs; no weights are stored.

    python tests/golden/make_golden_posenet.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

WEIGHT_SEEDS = (11, 12)
INPUT_SEED, LANES, SAMPLE = 5, 3, 512


def main():
    from tests.golden.make_golden import REF
    from tools import posenet_torch as PT

    spec = importlib.util.spec_from_file_location("ref_flowposenet", os.path.join(REF, "Module/Network/TartanVOStereo/FlowPoseNet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    x = PT.sample_input(LANES, INPUT_SEED)
    out = {"weight_seeds": np.array(WEIGHT_SEEDS), "input_seed": np.array(INPUT_SEED), "lanes": np.array(LANES)}
    for seed in WEIGHT_SEEDS:
        sd = PT.seeded_state_dict(seed)
        out[f"s{seed}_sha"] = np.array(PT.state_dict_sha256(sd))
        for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            net = mod.VOFlowRes(intrinsic=True, down_scale=True, config=1, stereo=True, autoDistTarget=0.)
            assert [k for k in net.state_dict()] == list(sd), "the canonical tensor order is the reference's state_dict() order"
            net.load_state_dict(sd, strict=True)
            net = net.to(dt).eval()
            stages = []
            hooks = [getattr(net, n).register_forward_hook(lambda m, i, o: stages.append(o.detach().clone())) for n in PT.STAGES]
            with torch.no_grad():
                y = net(x.to(dt).clone(), scale_disp=1.0)     # (the forward scales channel 2 in place)
            for h in hooks:
                h.remove()
            out[f"s{seed}_{tag}_out"] = y.numpy()
            for name, st in zip(PT.STAGES, stages):
                assert tuple(st.shape[1:]) == PT.STAGE_SHAPES[PT.STAGES.index(name)]
                out[f"s{seed}_{tag}_{name}"] = st.reshape(-1)[PT.sample_index(st.numel(), SAMPLE)].numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "posenet.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
