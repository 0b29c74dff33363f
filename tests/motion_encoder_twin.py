"""Host twin of csrc/motion_encoder.hip in plain torch on the CPU, and the seeded cases the motion-encoder tests share.

The twin states what csrc/motion_encoder_math.h states: weights, biases and inputs rounded to the 16-bit operand type, products accumulated in fp32 (or
fp64, to measure what the accumulation order is worth), bias and ReLU in the accumulation type, and one rounding exactly where the kernels store: C1 =
relu(convc1), the two column blocks of CF (cor = relu(convc2), flo = relu(convf2)), F1 = relu(convf1) and output channels 0..125.  flow passes through to
channels 126..127 as it is.  With ``dt=None`` nothing is rounded: the twin is then MotionEncoder.forward itself."""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from tools import flowformer_host as FH

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
ULP = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10}          # ulp(scale) / scale of the issue's bar
COR_PLANES = 145
LIVE = 126                                             # output channels the last convolution writes; 126..127 are flow
# (B, H8, W8): smaller than the 7x7 halo; partial tiles with a row and an image boundary inside one 32-pixel block; three images in one 64-pixel tile; KITTI
SHAPES = ((1, 5, 7), (2, 9, 18), (3, 5, 7), (1, 47, 98))
EDGE_SHAPES = ((1, 1, 1), (1, 1, 40), (1, 40, 1), (1, 2, 33))
STORED = ("c1", "cor", "f1", "flo", "out")            # what the kernels store, in launch order; "out" = channels 0..125
NAN_SHAPE = (2, 9, 18)                                 # the NaN cases: one NaN at the last pixel of image 0
NAN_AT = (0, 0, 8, 17)


def make_module(seed: int):
    torch.manual_seed(seed)
    return FH.MotionEncoder(COR_PLANES).eval()


def make_inputs(shape, seed: int):
    """flow in pixels at 1/8 resolution (a few pixels), corr = [64 latent | 81 window cells] features of unit scale."""
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 + seed)
    flow = 4 * torch.randn(B, 2, H, W, generator=g)
    corr = torch.randn(B, COR_PLANES, H, W, generator=g)
    return flow, corr


def stored(sd, flow, corr, dt: torch.dtype | None, acc: torch.dtype = torch.float32) -> dict:
    """The twin: every stored tensor (STORED) and "full" = the [B,128,H,W] result, as ``acc`` tensors holding ``dt`` values."""
    def rnd(t):
        return t.to(acc) if dt is None else t.to(dt).to(acc)

    def conv(x, name, pad):
        return F.conv2d(x, rnd(sd[name + ".weight"]), rnd(sd[name + ".bias"]), padding=pad)

    fl, co = rnd(flow), rnd(corr)
    c1 = rnd(torch.relu(conv(co, "convc1", 0)))
    cor = rnd(torch.relu(conv(c1, "convc2", 1)))
    f1 = rnd(torch.relu(conv(fl, "convf1", 3)))
    flo = rnd(torch.relu(conv(f1, "convf2", 1)))
    out = rnd(torch.relu(conv(torch.cat([cor, flo], dim=1), "conv", 1)))
    return {"c1": c1, "cor": cor, "f1": f1, "flo": flo, "out": out, "full": torch.cat([out, fl], dim=1)}


def forward(sd, flow, corr, dt: torch.dtype | None, acc: torch.dtype = torch.float32):
    return stored(sd, flow, corr, dt, acc)["full"]


def finite_scale(t) -> float:
    """max |t| over the finite elements of t (0 when there are none)."""
    f = t[torch.isfinite(t)]
    return float(f.abs().max()) if f.numel() else 0.0


def live_scale(full) -> float:
    """The scale of a result: over channels 0..125 only (the pass-through flow, a few pixels large, must not set it), finite elements only."""
    return finite_scale(full[:, :LIVE])


def rel_err(got, ref) -> float:
    """max |got - ref| / max |ref| over channels 0..125."""
    got, ref = got[:, :LIVE].double(), ref[:, :LIVE].double()
    return float((got - ref).abs().max() / ref.abs().max())


class Case:
    """One seeded encoder in a 16-bit type with its inputs and, computed once on the CPU: the twin's stored tensors (fp32 and fp64 accumulation), the fp64
    module on the same 16-bit weights and inputs, and the eager 16-bit module."""

    def __init__(self, dtname: str, shape, seed: int):
        self.dtname, self.dt, self.shape, self.seed = dtname, DTYPES[dtname], shape, seed
        module = make_module(seed).to(self.dt)
        self.module = module
        self.sd = {k: v.detach() for k, v in module.state_dict().items()}
        flow, corr = make_inputs(shape, seed)
        self.flow, self.corr = flow.to(self.dt), corr.to(self.dt)
        with torch.no_grad():
            self.stored = stored(self.sd, self.flow, self.corr, self.dt)
            self.stored64 = stored(self.sd, self.flow, self.corr, self.dt, torch.float64)
            m64 = make_module(seed).double()
            m64.load_state_dict({k: v.double() for k, v in self.sd.items()})
            self.f64 = m64(self.flow.double(), self.corr.double())
            self.eager = module(self.flow, self.corr)
        self.twin = self.stored["full"]
        self.scale = live_scale(self.twin)

    def twin_bar(self) -> float:
        """max |got - twin| allowed over channels 0..125: 2 ulp of the twin's largest magnitude there."""
        return 2 * ULP[self.dtname] * self.scale


@functools.lru_cache(maxsize=None)
def case(dtname: str, shape=SHAPES[0], seed: int = 0) -> Case:
    return Case(dtname, tuple(shape), seed)


@functools.lru_cache(maxsize=None)
def nan_case(dtname: str, which: str):
    """The seeded (2, 9, 18) case with one NaN in ``which`` ("flow" or "corr") at channel 0 of the last pixel of image 0: (flow, corr, twin result)."""
    c = case(dtname, NAN_SHAPE)
    flow, corr = c.flow.clone(), c.corr.clone()
    (flow if which == "flow" else corr)[NAN_AT] = float("nan")
    with torch.no_grad():
        return flow, corr, forward(c.sd, flow, corr, c.dt)


# ---------------------------------------------------------------------------------------------------------------- one-hot "selection" weights
CONVS = ("convc1", "convc2", "convf1", "convf2", "conv")
# Channel shifts of the pass-through convolutions.  `conv` has 126 rows over the 256 columns of CF = [cor 0..191 | flo 192..255], convc2 192 rows over C1's
# 256 channels, convf2 64 rows over F1's 128: one set of pass-through weights cannot show every row of the layer in front of it, so each scrambled layer runs
# under the sets that between them do.  Row o of a pass-through convolution picks the centre tap of input channel (o + shift) % cin.
_A = {"conv": 0, "convc2": 0, "convf2": 0}        # conv sees cor 0..125   <- C1 0..125
_B = {"conv": 66, "convc2": 0, "convf2": 0}       # conv sees cor 66..191  <- C1 66..191
_C = {"conv": 130, "convc2": 64, "convf2": 64}    # conv sees cor 130..191 <- C1 194..255, and flo 0..63 <- F1 64..127
_D = {"conv": 66, "convc2": 64, "convf2": 0}      # conv sees cor 66..191  <- C1 130..255
_E = {"conv": 130, "convc2": 0, "convf2": 0}      # conv sees cor 130..191 <- C1 130..191, and flo 0..63 <- F1 0..63
LAYER_VARIANTS = {"convc1": (_A, _B, _D), "convc2": (_A, _B, _C), "convf1": (_C, _E), "convf2": (_C,), "conv": (_A,)}


def selection_weights(sd, scrambled: str, seed: int, shifts: dict):
    """Every convolution picks, per output channel o, ONE input element with gain 1: the centre tap of channel (o + shifts[name]) % cin, bias 0 or 0.5 —
    except ``scrambled``, which picks a random tap of a random channel, bias 0 or +-0.5, with gain +-1 or +-0.5 where its input is signed (convc1, convf1)
    and 1 or 0.5 where it is a ReLU's output (a negative gain there is a row that the next ReLU sets to zero: nothing would be seen of it).  One non-zero
    product per output: exact whatever the summation order, so the kernel can differ from the twin only where a tap, a channel, a row or a padded border
    is wrong."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in sd.items():
        name = k.rsplit(".", 1)[0]
        if k.endswith(".bias"):
            lo = -1 if name == scrambled else 0
            out[k] = (torch.randint(lo, 2, v.shape, generator=g) * 0.5).to(v.dtype)
            continue
        cout, cin, kh, kw = v.shape
        w = torch.zeros(v.shape)
        o = torch.arange(cout)
        if name == scrambled:
            ch, ty, tx = (torch.randint(0, n, (cout,), generator=g) for n in (cin, kh, kw))
            gain = torch.tensor([1.0, 0.5, -1.0, -0.5])[torch.randint(0, 4 if name in ("convc1", "convf1") else 2, (cout,), generator=g)]
        else:
            ch, ty, tx, gain = (o + shifts.get(name, 0)) % cin, torch.full((cout,), kh // 2), torch.full((cout,), kw // 2), torch.ones(cout)
        w[o, ch, ty, tx] = gain
        out[k] = w.to(v.dtype)
    return out


def observed_rows(sd_sel, layer: str, flow, corr, dt) -> set:
    """The output rows of ``layer`` that the result depends on under the selection weights ``sd_sel``: row r counts when setting its weights and bias to
    zero changes channels 0..125 of the twin's result."""
    with torch.no_grad():
        base = stored(sd_sel, flow, corr, dt)["out"]
        rows = set()
        for r in range(sd_sel[layer + ".weight"].shape[0]):
            sd = dict(sd_sel)
            w, b = sd[layer + ".weight"].clone(), sd[layer + ".bias"].clone()
            w[r], b[r] = 0, 0
            sd[layer + ".weight"], sd[layer + ".bias"] = w, b
            if not torch.equal(stored(sd, flow, corr, dt)["out"], base):
                rows.add(r)
    return rows
