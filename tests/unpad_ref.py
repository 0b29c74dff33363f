"""Frames whose sides are no multiples of 8, as the network hands them to the hot path (FlowFormerCov.inference: centred pad to multiples of 8 in front of the
encoders, `unpad` behind the upsampling): dense fields at the un-padded H x W, feature maps / coords / 1/8-resolution fields at ceil(H / 8) x ceil(W / 8)."""
import torch

from tests import synth


def pad_of(H, W):
    """(hp, pw, y0, x0): the pad the network adds and where the frame sits in the padded one (centred)."""
    hp, pw = (-H) % 8, (-W) % 8
    return hp, pw, hp // 2, pw // 2


def make_sequence(n_frames, H, W, fields8=False, mask_seed=2, **kw):
    """`synth.make_sequence` for any frame size: camera, `flow` and `logcov` of the H x W sequence, `fmap1` / `fmap2` / `coords` of the sequence at the padded
    size (same seed).  fields8: `flow` / `logcov` are replaced by `flow8` / `cov8` / `up_mask` / `cov_mask` at 1/8 of the PADDED size, built from the padded
    sequence's dense fields as tests/test_gpu_native.py::test_native_upsample_path_and_split3 builds them."""
    hp, pw, _, _ = pad_of(H, W)
    cam, frames, poses = synth.make_sequence(n_frames, H, W, **kw)
    _, padded, _ = synth.make_sequence(n_frames, H + hp, W + pw, **kw)
    h8, w8 = (H + hp) // 8, (W + pw) // 8
    g = torch.Generator().manual_seed(mask_seed)
    out = []
    for fr, pf in zip(frames, padded):
        d = dict(fmap1=pf["fmap1"], fmap2=pf["fmap2"], coords=pf["coords"], flow=fr["flow"], logcov=fr["logcov"])
        assert d["coords"].shape[-2:] == (h8, w8)
        if fields8:
            d["flow8"] = torch.nn.functional.avg_pool2d(pf["flow"], 8) / 8.0
            d["cov8"] = torch.nn.functional.avg_pool2d(pf["logcov"], 8) / 8.0
            d["up_mask"] = torch.randn(2, 576, h8, w8, generator=g)
            d["cov_mask"] = torch.randn(2, 576, h8, w8, generator=g) * 0.25
            d["flow"] = None
            d["logcov"] = None
        out.append(d)
    return cam, out, poses


def upsample_case(B, h, w, seed=0):
    """Seeded `flow8 [B,2,h,w]` and fp32 `mask [B,576,h,w]` for the convex-upsampling kernels."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 2, h, w, generator=g), torch.randn(B, 576, h, w, generator=g) * 4
