"""The resampling family of the reference's ``DataLoader/Transform.py`` (:41-209) as HIP plugins: one launch per frame.

``HIP_ScaleFrame``, ``HIP_CenterCropFrame``, ``HIP_SmartResizeFrame`` and ``HIP_CastDataType`` keep the reference's config key sets and its
``forward(frame)`` contract on ``frame.stereo`` (``imageL``, ``imageR``, ``gt_flow``, ``flow_mask``, ``gt_depth`` are replaced, ``K``, ``height`` and
``width`` updated); the planes come back as device tensors.  :func:`smart_transform` is ``DataLoader/SequenceBase.py:120-141``: the lookup by sequence type and
the list form, with every run of these four folded into ONE plan (``ops.preprocess_plan``), hence one launch; any other transform passes through unfused.

``IDataTransform`` is the reference's own ABC when the MAC-VO checkout is importable (the switch of :mod:`macvo_amd.interfaces`), a mirror on
``interfaces.ConfigurablePlugin`` otherwise.  torchvision's tensor path is restated, parity-unpinned (the reference does not pin torchvision).
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from types import SimpleNamespace

import torch

from . import ops
from .interfaces import USING_REFERENCE, ConfigurablePlugin

if USING_REFERENCE:  # pragma: no cover - only inside a full MAC-VO environment
    from DataLoader import IDataTransform  # type: ignore
else:

    class IDataTransform(ABC, ConfigurablePlugin):
        """``DataLoader/Transform.py:18-29``: a callable ``frame -> frame`` configured by a namespace (None = empty)."""

        def __init__(self, config: "SimpleNamespace | dict | None") -> None:
            if config is None:
                self.config = SimpleNamespace()
            elif isinstance(config, SimpleNamespace):
                self.config = config
            else:
                self.config = SimpleNamespace(**config)

        @abstractmethod
        def forward(self, frame): ...

        def __call__(self, frame):
            return self.forward(frame)


_PLANES = ("imageL", "imageR", "gt_flow", "flow_mask", "gt_depth")


def _is_int(v) -> bool:
    return isinstance(v, int) and v > 0


def _is_num(v) -> bool:
    return isinstance(v, (float, int)) and v > 0


def apply_plan(stereo, plan: "ops.PreprocessPlan", device=None):
    """``stereo`` (anything with the fields of the reference's ``StereoData``) through ``plan``: one launch on the current stream.  Planes that are not on a
    GPU yet are uploaded as they are (a uint8 image travels as uint8).  ``stereo`` is updated in place and returned."""
    dev = torch.device(device) if device is not None else next(
        (t.device for t in (getattr(stereo, n, None) for n in _PLANES) if isinstance(t, torch.Tensor) and t.is_cuda), torch.device("cuda"))
    src = {n: getattr(stereo, n, None) for n in _PLANES}
    src = {n: (None if t is None else t.to(dev, non_blocking=True)) for n, t in src.items()}
    res = ops.preprocess(plan, **src)
    for n in _PLANES:
        if src[n] is not None:
            setattr(stereo, n, getattr(res, n))
    K0 = getattr(stereo, "K", None)
    stereo.K = plan.K.to(K0.device) if isinstance(K0, torch.Tensor) else plan.K          # (the plan's K has the shape the frame's K had)
    stereo.height, stereo.width = plan.height, plan.width
    return stereo


class _HipFrameTransform(IDataTransform):
    """A transform that is one step of a plan: ``steps()`` names it, ``forward`` plans for the frame's size and intrinsics and launches."""

    def steps(self) -> list:
        raise NotImplementedError

    def forward(self, frame):
        return _FoldedTransform([self]).forward(frame)


class HIP_ScaleFrame(_HipFrameTransform):
    """``ScaleFrame`` (Transform.py:41-94)."""

    @classmethod
    def is_valid_config(cls, config: SimpleNamespace | None) -> None:
        cls._enforce_config_spec(config, {"scale_u": _is_num, "scale_v": _is_num, "interp": lambda v: v in {"nearest", "bilinear"}})

    def steps(self) -> list:
        return [("scale", dict(scale_u=self.config.scale_u, scale_v=self.config.scale_v, interp=self.config.interp))]


class HIP_CenterCropFrame(_HipFrameTransform):
    """``CenterCropFrame`` (Transform.py:97-133)."""

    @classmethod
    def is_valid_config(cls, config: SimpleNamespace | None) -> None:
        cls._enforce_config_spec(config, {"height": _is_int, "width": _is_int})

    def steps(self) -> list:
        return [("crop", dict(height=self.config.height, width=self.config.width))]


class HIP_SmartResizeFrame(_HipFrameTransform):
    """``SmartResizeFrame`` (Transform.py:181-209)."""

    @classmethod
    def is_valid_config(cls, config: SimpleNamespace | None) -> None:
        cls._enforce_config_spec(config, {"height": _is_int, "width": _is_int, "interp": lambda v: v in {"nearest", "bilinear"}})

    def steps(self) -> list:
        return [("smart", dict(height=self.config.height, width=self.config.width, interp=self.config.interp))]


class HIP_CastDataType(_HipFrameTransform):
    """``CastDataType`` (Transform.py:153-178)."""

    @classmethod
    def is_valid_config(cls, config: SimpleNamespace | None) -> None:
        cls._enforce_config_spec(config, {"dtype": lambda v: v in ("fp16", "fp32", "bf16")})

    def steps(self) -> list:
        return [("cast", dict(dtype=self.config.dtype))]


_FOLDABLE = {"ScaleFrame": HIP_ScaleFrame, "CenterCropFrame": HIP_CenterCropFrame, "SmartResizeFrame": HIP_SmartResizeFrame, "CastDataType": HIP_CastDataType}
_FOLDABLE.update({c.__name__: c for c in list(_FOLDABLE.values())})


def plan_steps(steps: list, H: int, W: int, K: torch.Tensor | None) -> list:
    """``[(kind, args), ...]`` -> the fewest plans that carry them in order (one, unless a step does not fold into the plan in front of it)."""
    plans, cur = [], None
    for kind, args in steps:
        if cur is None:
            cur = ops.preprocess_plan(H, W, kind, K=K, **args)
            continue
        try:
            cur = cur.then(kind, **args)
        except ops.PlanDoesNotFold:
            plans.append(cur)
            cur = ops.preprocess_plan(cur.height, cur.width, kind, K=cur.K, **args)
    return plans + [cur]


class _FoldedTransform(IDataTransform):
    """A run of the four HIP transforms as one callable: plans are made per (size, intrinsics) and kept."""

    def __init__(self, transforms: list) -> None:
        super().__init__(None)
        self.transforms = list(transforms)
        self._plans: dict = {}

    @classmethod
    def is_valid_config(cls, config: SimpleNamespace | None) -> None:
        raise KeyError("a folded run of transforms is made by smart_transform, never named in a config")

    def steps(self) -> list:
        return [s for t in self.transforms for s in t.steps()]

    def plans(self, H: int, W: int, K: torch.Tensor | None) -> list:
        key = (H, W, None if K is None else tuple(K.detach().reshape(-1).tolist()))
        if key not in self._plans:
            self._plans[key] = plan_steps(self.steps(), H, W, K)
        return self._plans[key]

    def forward(self, frame):
        st = frame.stereo
        for plan in self.plans(int(st.height), int(st.width), st.K.detach().cpu() if isinstance(st.K, torch.Tensor) else None):
            apply_plan(st, plan)
        return frame


def fold_transforms(transforms: list) -> list:
    """Neighbouring HIP transforms of a list become one :class:`_FoldedTransform`; everything else keeps its place."""
    out, run = [], []
    for t in transforms:
        if isinstance(t, _HipFrameTransform):
            run.append(t)
            continue
        if run:
            out.append(_FoldedTransform(run))
            run = []
        out.append(t)
    if run:
        out.append(_FoldedTransform(run))
    return out


def _cfg_ns(c):
    if isinstance(c, SimpleNamespace):
        return c
    return SimpleNamespace(type=c["type"], args=SimpleNamespace(**(c.get("args") or {})))


def instantiate_transforms(transform_cfg: list) -> list:
    """``[{type, args}, ...]`` -> transforms: the four resampling classes (by their reference names or their ``HIP_`` names) as HIP plugins, folded; any other
    type through ``IDataTransform.instantiate`` (the reference's registry when it is importable)."""
    made = []
    for c in transform_cfg:
        c = _cfg_ns(c)
        cls = _FOLDABLE.get(c.type)
        if cls is not None:
            cls.is_valid_config(c.args)
            made.append(cls(c.args))
        else:
            made.append(IDataTransform.instantiate(c.type, c.args))
    return fold_transforms(made)


def smart_transform(seq, trans_cfg):
    """``DataLoader/SequenceBase.py:120-141``: ``trans_cfg`` is a list of ``{type, args}``, or a mapping / namespace from sequence type (``seq.name()``) to such
    a list — a sequence type it does not name is returned unchanged.  ``seq.transform(fns)`` receives the folded callables."""
    if isinstance(trans_cfg, (list, tuple)):
        cfgs = list(trans_cfg)
    else:
        table = vars(trans_cfg) if isinstance(trans_cfg, SimpleNamespace) else dict(trans_cfg)
        seq_type = seq.name()
        if seq_type not in table:
            return seq
        cfgs = list(table[seq_type])
    return seq.transform(instantiate_transforms(cfgs))
