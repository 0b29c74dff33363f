"""The per-frame hot path in the reference's call order (``Odometry/MACVO.py:173-311``), on one GPU.

``HotPath.step`` is what ``MACVO.run_pair`` executes between "the learned layers produced feature maps /
GRU updates" and "the optimised pose is written back", with every arithmetic step in the HIP kernels:

    Frontend.estimate_pair   MACVO.py:182   corr volume (A5) -> 12 x window lookup (A6) -> epilogue (A8/A2)
    KeypointSelector         MACVO.py:197   dense selector (A10/A11) + host randperm (bit-exact indices)
    gathers / tracking       MACVO.py:198-232  kp_track (A12)
    pixel2point_NED, world   MACVO.py:240,273-281  backproject (A12/A16)
    ObsCovModel.estimate x2  MACVO.py:241-242  match_cov (A13-A16), world rotation fused
    OutlierFilter.filter     MACVO.py:269   obs_filter (validity mask instead of row compaction)
    Optimizer                MACVO.py:309-311  pgo_solve (A17-A22), pose written back in fp32 (A22)

The learned FlowFormer layers (Twins encoder, cost-token transformer, GRU) are NOT part of this module: their
outputs for a frame arrive as :class:`FrameInputs` already resident in HBM (the network "stays
PyTorch-ROCm"; its source and weights are absent from the reference checkout).

State carried between frames lives on the device: the previous frame's depth maps and the previous pose
(StaticMotionModel: the prior of frame t is the optimised pose of frame t-1, MotionModel.py:134-142).
The only host synchronisation per frame is the selector's candidate count (needed by ``torch.randperm``).
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass, field, replace
from types import SimpleNamespace

import torch

from . import ops

_RANGES = os.environ.get("MV_TRACE_RANGES", "0") not in ("", "0")


def traced(name: str):
    """Opt-in (``MV_TRACE_RANGES=1``) profiler range around a pipeline stage, named like the reference's ``Timer`` scopes
    (``Frontend.estimate``: ``Module/Frontend/Frontend.py:215-216``; ``Odom_Runtime``: ``Odometry/MACVO.py:350-351``).  On ROCm
    ``torch.cuda.nvtx`` emits roctx ranges (``rocprofv3 --marker-trace``).  Off by default: two host calls per stage per frame."""
    def deco(fn):
        if not _RANGES:
            return fn
        import functools

        @functools.wraps(fn)
        def wrapped(*a, **k):
            torch.cuda.nvtx.range_push(name)
            try:
                return fn(*a, **k)
            finally:
                torch.cuda.nvtx.range_pop()
        return wrapped
    return deco


@dataclass
class Camera:
    fx: float
    fy: float
    cx: float
    cy: float
    baseline: float
    H: int
    W: int

    @property
    def K4(self):
        return (self.fx, self.fy, self.cx, self.cy)


@dataclass
class HotPathConfig:
    """Values of ``Config/Experiment/MACVO/MACVO_Fast.yaml`` (:22-104) that touch the hot path."""
    num_point: int = 200
    edgewidth: int = 32
    match_cov_default: float = 0.25
    # CovAwareSelector_NoDepth | "full" = CovAwareSelector | "random" = RandomSelector | "grid" = GridSelector (both use kp_mask_width only) |
    # "explicit" = every frame's keypoints come from the caller (FrameInputs.keypoints / step(..., keypoints=)).  selector_config_fields() maps a
    # reference `keypoint` block onto this field and the selector's arguments.
    selector: str = "nodepth"
    kp_kernel_size: int = 7
    kp_mask_width: int = 32
    max_match_cov: float = 100.0
    max_depth_cov: float = 250.0
    max_depth: float | str = "auto"      # "auto" -> fx * baseline (KeypointSelector.py:263)
    cov_kernel_size: int = 31
    min_flow_cov: float = 0.25
    min_depth_cov: float = 0.05
    graph_type: str = "disp"
    min_num_point: int = 10              # MACVO.py:64
    filters: int = ops.FILTER_COV_SANITY  # CovarianceSanityFilter
    filter_min_depth: float = 0.05
    radius: int = 4
    feature_layout: str = "chw"
    use_graphs: bool = False             # hipGraph-replay the decoder-side segment for inputs marked `static`
    mapping: bool = False                # dense-mapping tail of run_pair (MACVO.py:313-337; `mapping: true` in MACVO_Fast)
    map_num_point: int = 2000            # :315
    map_max_depth: float = 5.0           # MappingPointSelector args (Config/Experiment/MACVO/MACVO_Fast.yaml)
    map_max_depth_cov: float = 0.005
    map_mask_width: int = 32
    # fp32 features: "f16x2" (the default everywhere, ops.default_volume_precision(): per-row power-of-two scales + two fp16 pieces,
    # three products on the 16-bit matrix pipe, error <= ~2^-21 sum |a||b|) | "bf16x3" three bf16 pieces, six products | "exact" fp32
    # MFMA (bitwise fmaf chain) | "split3" / "split2" the round-1 tile kernels over pre-split planes (layout "hwc").  Shapes the
    # streaming split kernel does not cover run the exact kernel.  16-bit features ignore it.
    volume_precision: str = field(default_factory=ops.default_volume_precision)
    # 16-bit features: "fp32" = fp32 cells (rounds 1-3) | "encoder" = the volume in the features' fp16 type, one rounding in the GEMM's epilogue —
    # what the reference's Fast mode computes (einsum of fp16 maps, flownet.py:26-27; MACVO_Fast.yaml:73-74) at half the bytes; the lookups read
    # the 2-byte cells.  fp16 features in layout "hwc" with C = 128 / 256 (native driver); anything else keeps fp32 cells.
    volume_store: str = "fp32"
    async_backend: bool | None = None    # native driver: issue a frame's backend launches from a second host thread (None: the
                                         # library's default / MV_PIPE_ASYNC_BACKEND); identical results either way
    # observation-covariance model (`cov.obs` of the experiment YAML, Project2to3.py): "match" = MatchCovariance | "gmm" =
    # GaussianMixtureCovariance | "none" = NoCovariance, then the modifiers "diag" (Modifier_Diagonalize) / "normalize"
    # (Modifier_Normalize), innermost first.  cov_config_fields() maps a reference `cov.obs` block onto these two fields.
    cov_model: str = "match"
    cov_modifiers: tuple[str, ...] = ()
    # motion model (`motion` of the experiment YAML, Module/MotionModel.py): "static" = StaticMotionModel (the prior of frame t is the
    # pose of frame t-1) | "tartan" = TartanMotionNet (prior = pose of frame t-1 @ Exp(PoseNet motion); HotPath's `pose_net` supplies the
    # network).  motion_config_fields() maps a reference `motion` block onto this field.
    motion_model: str = "static"
    # which covariances the frontend provides, (depth model, matcher) = IFrontend.provide_cov (Frontend.py:137-139).  (True, True) = FlowFormerCov;
    # (False, False) = FrontendCompose(FlowFormerDepth, FlowFormerMatcher), the paper's "no covariance at all" baseline (Ablation_Study/
    # TartanAirv2_Vanilla.yaml); the mixed composes set one.  A missing side has no covariance input, no covariance map, -1 placeholders in the stored
    # rows (MACVO.py:253-263); whatever would read it is refused (check_frontend_cov).  frontend_config_fields() maps a `frontend` block onto it.
    frontend_cov: "tuple[bool, bool]" = (True, True)
    # the covariance MODEL's own `match_cov_default` (cov.obs args; Project2to3.py:133,216): sigma of the second observation when the matcher gives no
    # covariance.  Not `match_cov_default` above (Odometry.args), which stays the sigma of the first observation and of map points (MACVO.py:228,322).
    cov_match_cov_default: float = 0.25
    # frame the LM solve runs in (`optimizer.type` of the experiment YAML): "world" = TwoFrame_PGO | "local" = Local_TwoFrame_PGO, the frame of the pose
    # stored at map index frame_idx - 1 (Optimizer.py:111-150).  optimizer_config_fields() maps an `optimizer` block onto this field and graph_type.
    solve_frame: str = "world"
    # keyframe policy (`keyframe` of the experiment YAML, Module/KeyframeSelector.py): 1 = AllKeyframe, k = UniformKeyframe(keyframe_freq=k) — frame i
    # of a run() is a keyframe when i % k == 0, the others are registered with need_interp and filled in by MotionInterpolate (MACVO.py:177-179).
    keyframe_freq: int = 1


SOLVE_FRAMES = ("world", "local")
_OPTIMIZER_TYPES = {"TwoFrame_PGO": "world", "HIP_TwoFrame_PGO": "world", "Local_TwoFrame_PGO": "local", "HIP_Local_TwoFrame_PGO": "local"}


def optimizer_config_fields(block) -> dict:
    """A reference ``optimizer`` block (``{type, args}`` as a dict or SimpleNamespace) -> ``{"solve_frame", "graph_type"}`` for
    :class:`HotPathConfig`.  ``autodiff`` / ``vectorize`` / ``parallel`` / ``device`` are ignored (see :func:`hot_path_config`)."""
    t = _ns_get(block, "type")
    if t not in _OPTIMIZER_TYPES:
        raise ValueError(f"optimizer {t!r} has no HIP form (one of {sorted(_OPTIMIZER_TYPES)})")
    g = _ns_get(_ns_get(block, "args"), "graph_type")
    if g not in ("icp", "reproj", "disp"):
        raise ValueError(f"optimizer {t!r}: graph_type {g!r} is not one of icp, reproj, disp")
    return {"solve_frame": _OPTIMIZER_TYPES[t], "graph_type": g}


def keyframe_config_fields(block) -> dict:
    """A reference ``keyframe`` block (``{type, args}``) -> ``{"keyframe_freq"}`` for :class:`HotPathConfig`: ``AllKeyframe`` -> 1,
    ``UniformKeyframe`` -> its ``keyframe_freq``."""
    t = _ns_get(block, "type")
    if t == "AllKeyframe":
        return {"keyframe_freq": 1}
    if t != "UniformKeyframe":
        raise ValueError(f"keyframe selector {t!r} has no HIP form (AllKeyframe or UniformKeyframe)")
    k = _ns_get(_ns_get(block, "args"), "keyframe_freq")
    if not (isinstance(k, int) and not isinstance(k, bool) and k >= 1):
        raise ValueError(f"UniformKeyframe: keyframe_freq must be an integer >= 1, not {k!r}")
    return {"keyframe_freq": k}


_POSTPROCESS_TYPES = {"MotionInterpolate": "motion", "PoseInterpolate": "pose"}


def postprocess_config_fields(block) -> dict:
    """A reference ``Odometry.postprocess`` block (``{type, args}``; Module/MapProcessor.py) -> ``{"interpolate"}``: the choice
    ``DeviceVisualMaps.write(..., interpolate=)`` takes — ``MotionInterpolate`` -> ``"motion"``, ``PoseInterpolate`` -> ``"pose"``."""
    t = _ns_get(block, "type")
    if t not in _POSTPROCESS_TYPES:
        raise ValueError(f"map processor {t!r} has no HIP form (one of {sorted(_POSTPROCESS_TYPES)})")
    return {"interpolate": _POSTPROCESS_TYPES[t]}


def check_keyframes(cfg: "HotPathConfig") -> None:
    if cfg.solve_frame not in SOLVE_FRAMES:
        raise ValueError(f"solve_frame must be one of {SOLVE_FRAMES}, not {cfg.solve_frame!r}")
    if not (isinstance(cfg.keyframe_freq, int) and cfg.keyframe_freq >= 1):
        raise ValueError(f"keyframe_freq must be an integer >= 1, not {cfg.keyframe_freq!r}")


def check_frontend_cov(cfg: "HotPathConfig") -> None:
    """Configuration-time refusals of a frontend without covariances (the frame driver's check_config applies the same rules).  The reference asserts
    on ``depth.cov`` in CovAwareSelector / MappingPointSelector / GaussianMixtureCovariance, reads ``match.cov`` in both CovAware selectors, and
    builds the ``reproj`` / ``disp`` weights by inverting the -1 placeholders of ``pixel2_uv_cov`` / ``pixel2_disp_cov`` (Graphs.py:54-55,97-103,133)."""
    fc = cfg.frontend_cov
    if not (isinstance(fc, (tuple, list)) and len(fc) == 2):
        raise ValueError(f"frontend_cov must be (depth provides covariance, matcher provides covariance), not {fc!r}")
    d, m = bool(fc[0]), bool(fc[1])
    no_d = "the depth model provides no covariance (frontend_cov[0] is False: no depth / disparity variance)"
    no_m = "the matcher provides no covariance (frontend_cov[1] is False: no match covariance)"
    if not d:
        if cfg.selector == "full":
            raise ValueError(f"selector 'full' (CovAwareSelector) reads depth.cov, but {no_d}")
        if cfg.mapping:
            raise ValueError(f"mapping=True (MappingPointSelector) reads depth.cov, but {no_d}")
        if cfg.cov_model == "gmm":
            raise ValueError(f"cov_model 'gmm' (GaussianMixtureCovariance) reads depth.cov, but {no_d}")
        if cfg.graph_type == "disp":
            raise ValueError(f"graph_type 'disp' weighs its residual by pixel2_disp_cov, but {no_d}")
    if not m:
        if cfg.selector in ("nodepth", "full"):
            raise ValueError(f"selector {cfg.selector!r} (CovAwareSelector{'_NoDepth' if cfg.selector == 'nodepth' else ''}) reads match.cov, but {no_m}")
        if cfg.graph_type in ("reproj", "disp"):
            raise ValueError(f"graph_type {cfg.graph_type!r} weighs its residual by pixel2_uv_cov, but {no_m}")
        if cfg.cov_model != "none" and not cfg.cov_match_cov_default > 0:
            raise ValueError(f"cov_match_cov_default must be > 0 (it is the second observation's sigma when {no_m})")


def _nocov_mask(cfg: "HotPathConfig") -> int:
    d, m = ops.frontend_cov_flags(cfg.frontend_cov)
    return (0 if d else ops.L.MV_NOCOV_DEPTH) | (0 if m else ops.L.MV_NOCOV_MATCH)


_COV_TYPES = {"MatchCovariance": "match", "GaussianMixtureCovariance": "gmm", "NoCovariance": "none",
              "HIP_MatchCovariance": "match", "HIP_GaussianMixtureCovariance": "gmm", "HIP_NoCovariance": "none"}
_COV_MODIFIER_TYPES = {"Modifier_Diagonalize": "diag", "Modifier_Normalize": "normalize",
                       "HIP_Modifier_Diagonalize": "diag", "HIP_Modifier_Normalize": "normalize"}


def _ns_get(x, key):
    return x[key] if isinstance(x, dict) else getattr(x, key)


def cov_config_fields(obs) -> dict:
    """A reference ``cov.obs`` block (``{type, args}`` as a dict or SimpleNamespace; modifiers nest their submodel in
    ``args.type`` / ``args.args``) -> ``{"cov_model", "cov_modifiers", and the model's args}`` for :class:`HotPathConfig`.
    ``Modifier_Normalize(Modifier_Diagonalize(MatchCovariance))`` -> ``cov_model="match", cov_modifiers=("diag", "normalize")``."""
    mods = []
    while _ns_get(obs, "type") in _COV_MODIFIER_TYPES:
        mods.append(_COV_MODIFIER_TYPES[_ns_get(obs, "type")])
        obs = _ns_get(obs, "args")
    t = _ns_get(obs, "type")
    if t not in _COV_TYPES:
        raise ValueError(f"covariance model {t!r} has no HIP form (one of {sorted(set(_COV_TYPES))})")
    out = {"cov_model": _COV_TYPES[t], "cov_modifiers": tuple(reversed(mods))}
    args = _ns_get(obs, "args")
    if args is not None and _COV_TYPES[t] != "none":
        # (the model's own match_cov_default stands in for an absent flow_cov — a matcher without covariance, frontend_cov[1] False — and goes to
        # cov_match_cov_default; the constant kp0 / map-point sigma is Odometry.args.match_cov_default, MACVO.py:228,322)
        for k, f in (("kernel_size", "cov_kernel_size"), ("min_flow_cov", "min_flow_cov"), ("min_depth_cov", "min_depth_cov"),
                     ("match_cov_default", "cov_match_cov_default")):
            try:
                out[f] = _ns_get(args, k)
            except (KeyError, AttributeError):
                pass
    return out


def preprocess_config_fields(block, seq_type: str, camera: "Camera") -> dict:
    """A reference ``Preprocess`` block (Config/Experiment/Common/Preprocess.yaml: a mapping from sequence type to a list of ``{type, args}``, or such a list;
    dicts or SimpleNamespaces) for a ``seq_type`` sequence whose frames arrive as ``camera`` -> ``{"plans", "camera"}``: the folded
    :class:`ops.PreprocessPlan` list (one plan = one launch per frame; empty when the block does not name ``seq_type``) and the :class:`Camera` the backend
    must use — size and intrinsics after the transforms, K through the reference's own fp32 steps.  KITTI's block turns a 376 x 1241 camera into 376 x 780."""
    from .transforms import _FOLDABLE, _cfg_ns, plan_steps

    if isinstance(block, (list, tuple)):
        cfgs = list(block)
    else:
        table = vars(block) if not isinstance(block, dict) else block
        cfgs = list(table.get(seq_type, ()))
    steps = []
    for c in cfgs:
        c = _cfg_ns(c)
        if c.type not in _FOLDABLE:
            raise ValueError(f"data transform {c.type!r} has no HIP form (one of {sorted(_FOLDABLE)})")
        _FOLDABLE[c.type].is_valid_config(c.args)
        steps += _FOLDABLE[c.type](c.args).steps()
    if not steps:
        return {"plans": [], "camera": camera}
    K = torch.tensor([[camera.fx, 0.0, camera.cx], [0.0, camera.fy, camera.cy], [0.0, 0.0, 1.0]], dtype=torch.float32)
    plans = plan_steps(steps, camera.H, camera.W, K)
    Ko = plans[-1].K
    cam = replace(camera, fx=float(Ko[0, 0]), fy=float(Ko[1, 1]), cx=float(Ko[0, 2]), cy=float(Ko[1, 2]), H=plans[-1].height, W=plans[-1].width)
    return {"plans": plans, "camera": cam}


_MOTION_TYPES = {"StaticMotionModel": "static", "TartanMotionNet": "tartan", "HIP_TartanMotionNet": "tartan",
                 "HIP_TartanMotionNet_HIPPoseNet": "tartan"}


def hip_pose_net(weight_or_state_dict, device="cuda") -> "ops.PoseNet":
    """The ``pose_net`` of :class:`HotPath` / :class:`NativeHotPath` (motion_model "tartan") in HIP: a checkpoint path (the ``weight`` of a
    ``TartanMotionNet`` block) or a state dict -> the ``[lanes,5,112,160] -> [lanes,6]`` callable :class:`ops.PoseNet`."""
    if isinstance(weight_or_state_dict, (str, os.PathLike)):
        if not str(weight_or_state_dict):
            raise ops.L.MacvoHipError("hip_pose_net needs a checkpoint path or a state dict (an empty `weight` names no network)")
        return ops.PoseNet.from_file(str(weight_or_state_dict), device)
    return ops.PoseNet.from_state_dict(weight_or_state_dict, device)


def motion_config_fields(block) -> dict:
    """A reference ``motion`` block (``{type, args}`` as a dict or SimpleNamespace) -> ``{"motion_model": ...}`` for :class:`HotPathConfig`.
    ``TartanMotionNet`` (every configuration the paper reports: Paper_Reproduce.yaml, Ablation_Study/*) -> "tartan"; its ``weight`` /
    ``device`` args belong to the PoseNet, which the caller hands to :class:`HotPath` as ``pose_net``."""
    t = _ns_get(block, "type")
    if t not in _MOTION_TYPES:
        raise ValueError(f"motion model {t!r} has no HIP form (one of {sorted(set(_MOTION_TYPES))})")
    return {"motion_model": _MOTION_TYPES[t]}


_SELECTOR_TYPES = {"CovAwareSelector_NoDepth": "nodepth", "CovAwareSelector": "full", "RandomSelector": "random", "GridSelector": "grid",
                   "HIP_CovAwareSelector_NoDepth": "nodepth", "HIP_CovAwareSelector": "full", "HIP_RandomSelector": "random", "HIP_GridSelector": "grid"}
SELECTORS = ("nodepth", "full", "random", "grid", "explicit")
MAPLESS_SELECTORS = ("random", "grid", "explicit")     # look at no map: no selector kernels, no candidate list


def selector_config_fields(block) -> dict:
    """A reference ``keypoint`` block (``{type, args}`` as a dict or SimpleNamespace) -> ``{"selector", "kp_mask_width", ...}`` for
    :class:`HotPathConfig`: ``mask_width`` for every selector, and ``kernel_size`` / ``max_depth`` / ``max_depth_cov`` / ``max_match_cov`` for the
    CovAware ones.  ``GradientSelector``, ``SparseGradienSelector`` and ``SelectorCompose`` have no HIP form inside the pipe (they look at the image,
    which the pipe never sees): their HIP kernels run in front of it — :func:`image_selector` for the two gradient selectors, the ``HIP_*`` plugins for
    all three — and hand their pixels to the pipe as explicit keypoints (``selector="explicit"``), device rows and device counts included."""
    t = _ns_get(block, "type")
    if t not in _SELECTOR_TYPES:
        hint = ("pipeline.image_selector(block, device) computes its rows on the GPU; feed them through selector='explicit'"
                if t in _IMAGE_SELECTOR_TYPES else "its pixels can be fed through selector='explicit'")
        raise ValueError(f"keypoint selector {t!r} has no HIP form as a pipe selector (one of {sorted(set(_SELECTOR_TYPES))}); {hint}")
    out = {"selector": _SELECTOR_TYPES[t]}
    args = _ns_get(block, "args")
    names = [("mask_width", "kp_mask_width")]
    if out["selector"] in ("nodepth", "full"):
        names += [("kernel_size", "kp_kernel_size"), ("max_depth", "max_depth"), ("max_depth_cov", "max_depth_cov"), ("max_match_cov", "max_match_cov")]
    for k, f in names:
        try:
            out[f] = _ns_get(args, k)
        except (KeyError, AttributeError, TypeError):
            pass
    return out


_IMAGE_SELECTOR_TYPES = {"GradientSelector": False, "SparseGradienSelector": True, "HIP_GradientSelector": False, "HIP_SparseGradienSelector": True}


def image_selector(block, device, seeds=None):
    """A reference ``keypoint`` block of type ``GradientSelector`` / ``SparseGradienSelector`` (or their ``HIP_`` names; ``{type, args}`` as a dict or
    SimpleNamespace, the reference's keys ``mask_width``, ``grad_std``, ``nms_size``) -> a callable ``(imageL [lanes, 3, H, W] fp32, num_point) ->
    (rows int64 [lanes, num_point, 2], counts int32 [lanes])``, both on ``device``, the rows zero-padded behind each lane's count: what
    ``FrameInputs.keypoints`` / ``keypoint_counts`` of a ``selector="explicit"`` pipe take.  ``seeds`` (one per lane): device-resident generators with
    the bits of ``torch.Generator().manual_seed(seed)``, advanced call by call — nothing reaches the host.  Without: ``torch.randperm`` of torch's
    global CPU generator per lane, in lane order, as the reference draws (one host read of the counts per call)."""
    from .plugins import HIP_GradientSelector, HIP_SparseGradienSelector

    t = _ns_get(block, "type")
    if t not in _IMAGE_SELECTOR_TYPES:
        raise ValueError(f"image_selector: {t!r} is not an image selector (one of {sorted(_IMAGE_SELECTOR_TYPES)})")
    args = _ns_get(block, "args")
    args = SimpleNamespace(**args) if isinstance(args, dict) else args
    sparse = _IMAGE_SELECTOR_TYPES[t]
    (HIP_SparseGradienSelector if sparse else HIP_GradientSelector).is_valid_config(args)
    if getattr(args, "seed", None) is not None and seeds is None:
        seeds = [args.seed]
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"image_selector: {device!r} is not a GPU device (the HIP selectors have no CPU fallback)")
    mask_width, grad_std, nms = args.mask_width, float(args.grad_std), (args.nms_size if sparse else None)
    state = None if seeds is None else ops.mt19937_state(list(seeds), dev)

    def select(imageL: torch.Tensor, num_point: int):
        if imageL.dim() != 4:
            raise ValueError(f"image_selector: imageL must be [lanes, 3, H, W], got {tuple(imageL.shape)}")
        lanes = imageL.shape[0]
        cands = ops.kp_gradient(imageL.to(dev), mask_width, grad_std, nms)
        if state is not None:
            if state.shape[0] != lanes:
                raise ValueError(f"image_selector: {state.shape[0]} seeds for {lanes} lanes")
            return cands.finish_device(num_point, state)
        rows = torch.zeros((lanes, num_point, 2), dtype=torch.int64, device=dev)
        live = [cands.lane(l).finish(num_point) for l in range(lanes)]
        for l, r in enumerate(live):
            rows[l, : r.shape[0]] = r
        return rows, torch.tensor([r.shape[0] for r in live], dtype=torch.int32).to(dev)

    return select


_DEPTH_TYPES = {"FlowFormerCovDepth": True, "HIP_FlowFormerCovDepth": True, "FlowFormerDepth": False, "HIP_FlowFormerDepth": False}
_MATCH_TYPES = {"FlowFormerCovMatcher": True, "HIP_FlowFormerCovMatcher": True, "FlowFormerMatcher": False, "HIP_FlowFormerMatcher": False}
_JOINT_FRONTENDS = ("FlowFormerCovFrontend", "CUDAGraph_FlowFormerCovFrontend", "HIP_FlowFormerCovFrontend", "HIP_CUDAGraph_FlowFormerCovFrontend")


def frontend_config_fields(block) -> dict:
    """A reference ``frontend`` block (``{type, args}`` as a dict or SimpleNamespace) -> ``{"frontend_cov": (depth, match)}`` for
    :class:`HotPathConfig` = the frontend's ``provide_cov``: the joint FlowFormerCov frontends give both covariances, a ``FrontendCompose`` what its
    ``depth`` (``FlowFormerCovDepth`` / ``FlowFormerDepth``) and ``match`` (``FlowFormerCovMatcher`` / ``FlowFormerMatcher``) modules give.  The
    ground-truth and TartanVO modules have no HIP form."""
    t = _ns_get(block, "type")
    if t in _JOINT_FRONTENDS:
        return {"frontend_cov": (True, True)}
    if t != "FrontendCompose":
        raise ValueError(f"frontend {t!r} has no HIP form (one of {sorted(_JOINT_FRONTENDS)} or a FrontendCompose of "
                         f"{sorted(_DEPTH_TYPES)} x {sorted(_MATCH_TYPES)})")
    args = _ns_get(block, "args")
    dt, mt = _ns_get(_ns_get(args, "depth"), "type"), _ns_get(_ns_get(args, "match"), "type")
    if dt not in _DEPTH_TYPES:
        raise ValueError(f"depth model {dt!r} has no HIP form (one of {sorted(_DEPTH_TYPES)})")
    if mt not in _MATCH_TYPES:
        raise ValueError(f"matcher {mt!r} has no HIP form (one of {sorted(_MATCH_TYPES)})")
    return {"frontend_cov": (_DEPTH_TYPES[dt], _MATCH_TYPES[mt])}


_FILTER_TYPES = {"CovarianceSanityFilter": ops.FILTER_COV_SANITY, "SimpleDepthFilter": ops.FILTER_SIMPLE_DEPTH,
                 "LikelyFrontOfCamFilter": ops.FILTER_FRONT_OF_CAM, "IdentityFilter": 0}


def filter_config_fields(block) -> dict:
    """A reference ``outlier`` block (``{type, args}``; ``FilterCompose`` nests its filters in ``args.filter_args``) -> ``{"filters", and for a
    SimpleDepthFilter "filter_min_depth" and "max_depth"}``.  The filters are a conjunction, so their order does not matter.  The pipe has ONE
    ``max_depth`` (the selector's bound and this filter's): :func:`hot_path_config` reconciles the two."""
    out = {"filters": 0}

    def one(b):
        t = _ns_get(b, "type")
        if t == "FilterCompose":
            for sub in _ns_get(_ns_get(b, "args"), "filter_args"):
                one(sub)
            return
        if t not in _FILTER_TYPES:
            raise ValueError(f"observation filter {t!r} has no HIP form (one of {sorted(_FILTER_TYPES)} or a FilterCompose of them)")
        out["filters"] |= _FILTER_TYPES[t]
        if t == "SimpleDepthFilter":
            args = _ns_get(b, "args")
            for k, f in (("min_depth", "filter_min_depth"), ("max_depth", "max_depth")):
                v = _ns_get(args, k)
                if f in out and out[f] != v:
                    raise ValueError(f"two SimpleDepthFilters with different {k} ({out[f]!r}, {v!r}): the pipe has one")
                out[f] = v
    one(block)
    return out


def hot_path_config(odometry, **overrides) -> HotPathConfig:
    """The ``Odometry`` block of a reference experiment YAML (dict or SimpleNamespace, e.g. ``load_config(...)[0].Odometry``) ->
    :class:`HotPathConfig`: ``cov.obs``, ``keypoint``, ``motion``, ``frontend``, ``outlier``, ``optimizer`` and ``keyframe`` (where the block
    exists) through their mappers, ``mappoint`` (the MappingPointSelector's bounds) and ``args.{num_point, edgewidth, match_cov_default, mapping}``.  The optimizer's
    ``autodiff`` / ``vectorize`` / ``parallel`` / ``device`` are ignored: the solver's analytic Jacobians are the same residual's, and it runs on its own
    stream.  ``overrides`` win (e.g. ``feature_layout``)."""
    f: dict = {}
    args = _ns_get(odometry, "args")
    for k in ("num_point", "edgewidth", "match_cov_default", "mapping"):
        f[k] = _ns_get(args, k)
    f.update(cov_config_fields(_ns_get(_ns_get(odometry, "cov"), "obs")))
    f.update(motion_config_fields(_ns_get(odometry, "motion")))
    f.update(frontend_config_fields(_ns_get(odometry, "frontend")))
    sel = selector_config_fields(_ns_get(odometry, "keypoint"))
    flt = filter_config_fields(_ns_get(odometry, "outlier"))
    if "max_depth" in sel and "max_depth" in flt and sel["max_depth"] != flt["max_depth"]:
        raise ValueError(f"keypoint.args.max_depth = {sel['max_depth']!r} but the SimpleDepthFilter's max_depth = {flt['max_depth']!r}: the pipe has one max_depth")
    f.update(flt)
    f.update(sel)
    try:
        mp = _ns_get(odometry, "mappoint")
    except (KeyError, AttributeError):
        mp = None                                     # (only the block's absence is tolerated: HotPathConfig's defaults are MACVO_Fast's)
    if mp is not None and _ns_get(mp, "type") in ("MappingPointSelector", "HIP_MappingPointSelector"):
        for k, name in (("max_depth", "map_max_depth"), ("max_depth_cov", "map_max_depth_cov"), ("mask_width", "map_mask_width")):
            try:
                f[name] = _ns_get(_ns_get(mp, "args"), k)
            except (KeyError, AttributeError, TypeError):
                raise ValueError(f"mappoint.args lacks {k!r} (MappingPointSelector takes max_depth, max_depth_cov, mask_width)") from None
    elif mp is not None and f["mapping"]:
        raise ValueError(f"mapping: true with mappoint {_ns_get(mp, 'type')!r}: only MappingPointSelector has a HIP form")
    f.update(optimizer_config_fields(_ns_get(odometry, "optimizer")))
    try:
        kf = _ns_get(odometry, "keyframe")
    except (KeyError, AttributeError):
        kf = None
    if kf is not None:
        f.update(keyframe_config_fields(kf))
    f.update(overrides)
    cfg = HotPathConfig(**f)
    check_frontend_cov(cfg)
    check_keyframes(cfg)
    return cfg


def check_selector(cfg: "HotPathConfig", cam: "Camera") -> None:
    """Configuration-time checks of the selector block (the frame driver's check_config applies the same rules)."""
    if cfg.selector not in SELECTORS:
        raise ValueError(f"selector must be one of {SELECTORS}, not {cfg.selector!r}")
    if cfg.selector not in MAPLESS_SELECTORS:
        k = cfg.kp_kernel_size
        if not (isinstance(k, int) and k > 0 and k % 2 == 1 and k <= 15):
            raise ValueError(f"selector {cfg.selector!r}: kp_kernel_size {k!r} must be odd and within 1..15 (the NMS kernel's halo)")
        return
    m = cfg.kp_mask_width
    if m < 0 or cam.H <= 2 * m or cam.W <= 2 * m:
        raise ValueError(f"selector {cfg.selector!r}: kp_mask_width {m} leaves no pixel of a {cam.W} x {cam.H} image")
    if cfg.selector == "grid" and ops.kp_grid_count(cam.H, cam.W, m, cfg.num_point) <= 0:
        raise ValueError(f"selector 'grid': a grid step of 0 at {cam.W} x {cam.H}, mask_width {m}, num_point {cfg.num_point} (the reference raises here)")
    if cfg.selector == "random" and cfg.num_point > ops.L.load().mv_kp_random_max_point():
        raise ValueError(f"selector 'random': num_point {cfg.num_point} > {ops.L.load().mv_kp_random_max_point()} (the draw's word buffer)")
    if table_rows(cfg, cam) > ops.L.MV_KP_TABLE_MAX:
        raise ValueError(f"selector {cfg.selector!r}: {table_rows(cfg, cam)} keypoint rows > MV_KP_TABLE_MAX = {ops.L.MV_KP_TABLE_MAX}")
    if cfg.cov_model in ("match", "gmm") and m < cfg.cov_kernel_size // 2:
        raise ValueError(
            f"selector {cfg.selector!r} with cov_model {cfg.cov_model!r}: kp_mask_width {m} < cov_kernel_size // 2 = {cfg.cov_kernel_size // 2}.  The "
            f"{cfg.cov_kernel_size} x {cfg.cov_kernel_size} covariance patch of a keypoint that close to the border leaves the image; the reference then "
            "wraps negative indices or raises while the kernel clamps, so such keypoints must not get in (raise kp_mask_width, or use cov_model='none')")


def table_rows(cfg: "HotPathConfig", cam: "Camera") -> int:
    """Rows of capacity per lane of the per-keypoint tables: ``max(num_point, grid count)`` for "grid" (GridSelector may return more rows than
    ``num_point``: 231 at 640 x 480 / 32 / 200), ``num_point`` otherwise."""
    if cfg.selector == "grid":
        return max(cfg.num_point, ops.kp_grid_count(cam.H, cam.W, cfg.kp_mask_width, cfg.num_point))
    return cfg.num_point


def check_keypoints(kp: torch.Tensor, cfg: "HotPathConfig", cam: "Camera") -> None:
    """Explicit keypoints (host tensors only): inside the image and, for the patch-based covariance models, ``cov_kernel_size // 2`` from its border."""
    if kp.numel() == 0:
        return
    hw = cfg.cov_kernel_size // 2 if cfg.cov_model in ("match", "gmm") else 0
    u, v = kp[..., 0], kp[..., 1]
    if int(u.min()) < hw or int(u.max()) >= cam.W - hw or int(v.min()) < hw or int(v.max()) >= cam.H - hw:
        raise ValueError(f"explicit keypoints must lie at least {hw} pixels inside the {cam.W} x {cam.H} image (cov_model {cfg.cov_model!r}: the covariance "
                         "patch must not leave the image)")


def _randint_rows(num_point: int, H: int, W: int, mask: int, g) -> torch.Tensor:
    """RandomSelector.select_point (KeypointSelector.py:103-118) on the CPU generator ``g`` (None: torch's global one): first the rows' v, then their u."""
    kw = {} if g is None else {"generator": g}
    h = torch.randint(mask, H - mask, (num_point, 1), **kw)
    w = torch.randint(mask, W - mask, (num_point, 1), **kw)
    return torch.cat([w, h], dim=1)


@dataclass
class FrameInputs:
    """What the learned layers hand to the hot path for one ``estimate_pair`` (all GPU-resident).

    fmap1 / fmap2 : ``[2, C, h8, w8]`` (layout "chw") or ``[2, h8, w8, C]`` ("hwc"); pair 0 = stereo
                    (L_t2 vs R_t2), pair 1 = temporal (L_t1 vs L_t2)  (Frontend.py:219-220)
    coords        : ``[iters, 2, 2, h8, w8]`` fp32 — coords1 entering each decoder iteration (covhead.py:85-92)
    flow, logcov  : ``[2, 2, H, W]`` fp32 — last upsampled flow / log-sigma predictions (covhead.py:140), un-padded as ``inference`` returns them

    ``H x W`` is the camera's frame, of any size but one: a side one above a multiple of 8 (a pad of 7) is an invalid configuration for the native driver; ``h8, w8 = ops.eighth_shape(H, W) = ceil(H / 8), ceil(W / 8)`` is the grid the network works on after
    its centred pad to multiples of 8 (``ops.input_pad``; flownet.py:37-44 — KITTI's 376 x 780 frames give 47 x 98 maps).  ``flow8`` / ``cov8`` and the masks
    live on that grid too; the hot path upsamples them straight into the un-padded ``H x W`` window.

    With ``HotPathConfig.frontend_cov`` not ``(True, True)`` only the covariance samples of a side that provides one are read (sample 0 = depth
    model, sample 1 = matcher); ``logcov`` / ``cov8`` / ``cov_mask`` are None when neither does (plain FlowFormer has no covariance head).
    """
    fmap1: torch.Tensor
    fmap2: torch.Tensor
    coords: torch.Tensor
    flow: torch.Tensor | None = None
    logcov: torch.Tensor | None = None
    # False: `logcov` already holds sigma^2 = exp(2 * log-sigma), which is what the network's `inference` returns (flownet.py:44) — the epilogue then
    # takes it as it is (mv_frontend_epilogue's cov_is_log = 0).  pipeline.HotPath only; the native driver takes log-sigma.
    cov_is_log: bool = True
    # alternative to flow/logcov: the last decoder iteration's 1/8-resolution fields and convex
    # upsampling masks (covhead.py:119-135); the hot path then runs mv_convex_upsample (+ fused exp(2*cov)) itself
    flow8: torch.Tensor | None = None        # [2, 2, h8, w8]  coords1 - coords0
    cov8: torch.Tensor | None = None         # [2, 2, h8, w8]  cov_coords1 - cov_coords0
    up_mask: torch.Tensor | None = None      # [2, 576, h8, w8] flow branch mask BEFORE the 0.25 scale (:121)
    cov_mask: torch.Tensor | None = None     # [2, 576, h8, w8] log-sigma branch mask (0.25 already applied, :41)
    # event recorded by whoever produced fmap1/fmap2 (None = already complete, e.g. resident inputs): the volume GEMM
    # runs on its own stream and must not start before its operands exist
    ready: "torch.cuda.Event | None" = None
    # previous LEFT image [1|-,3,H,W] in [0,1] for the map-point colours (MACVO.py:326-328); optional, mapping mode only
    image: torch.Tensor | None = None
    # frame timestamp (StereoData.frame_ns) — recorded in the device-resident map when one is attached
    time_ns: int = 0
    # batched step (stack_lanes): every lane's own timestamp, recorded in that lane's map (NativeHotPath.attach_maps); None: `time_ns` for every lane
    lane_time_ns: "list | None" = None
    # caller-supplied keypoints of this frame: int64 (u, v) rows [n, 2] ([lanes, n, 2] for a batched step), on the host (checked) or on the device
    # (used as given: the caller keeps them cov_kernel_size // 2 inside the image).  Required by selector "explicit"; on any other selector they
    # replace the frame's own selection.  keypoint_counts: live rows per lane (default: all n) — a list, or with device keypoints a device int32 [lanes]
    # tensor (image_selector's), which the native driver hands to the pipe as it is: no host read.
    keypoints: torch.Tensor | None = None
    keypoint_counts: "list | torch.Tensor | None" = None
    # promise that every tensor above lives at a fixed address for the lifetime of the HotPath (e.g. the static output
    # buffers of a graph-captured network, as in the reference's CUDAGraph frontend): allows hipGraph replay
    static: bool = False


def check_frame_shapes(x: "FrameInputs", cam: "Camera") -> None:
    """The 1/8-resolution inputs live on ``ops.eighth_shape(H, W)``, the full-resolution ones on the un-padded ``H x W`` frame."""
    h8, w8 = ops.eighth_shape(cam.H, cam.W)
    if tuple(x.coords.shape[-2:]) != (h8, w8):
        raise ops.L.MacvoHipError(f"coords are {tuple(x.coords.shape[-2:])} but a {cam.H} x {cam.W} frame has {h8} x {w8} maps at 1/8 resolution")
    for name in ("flow8", "cov8", "up_mask", "cov_mask"):
        t = getattr(x, name)
        if t is not None and tuple(t.shape[-2:]) != (h8, w8):
            raise ops.L.MacvoHipError(f"{name} is {tuple(t.shape[-2:])}, expected {h8} x {w8}")
    for name in ("flow", "logcov"):
        t = getattr(x, name)
        if t is not None and x.flow8 is None and tuple(t.shape[-2:]) != (cam.H, cam.W):
            raise ops.L.MacvoHipError(f"{name} is {tuple(t.shape[-2:])}, expected the un-padded {cam.H} x {cam.W} frame")


@dataclass
class FrameResult:
    pose: torch.Tensor                 # [7] fp32 GPU — optimised pose of this frame (write_graph_data)
    pose_f64: torch.Tensor | None      # [1,7] fp64 GPU
    info: torch.Tensor | None          # [1,4] fp64 GPU {loss, steps, rejects, loss0}
    kp0_uv: torch.Tensor | None        # [n,2] int64 GPU selected keypoints
    n_valid: torch.Tensor | None       # [1] int32 GPU surviving observations
    extras: dict = field(default_factory=dict)
    map_points: "ops.MapPoints | None" = None   # mapping mode: the frame's dense map points (valid after sync_pose())
    prior: torch.Tensor | None = None  # motion_model "tartan": [7] fp32 GPU — the frame's motion-model prior (the LM start)


def _check_motion(cfg: HotPathConfig) -> None:
    if cfg.motion_model not in ("static", "tartan"):
        raise ops.L.MacvoHipError(f"motion_model must be 'static' or 'tartan', not {cfg.motion_model!r}")


class HotPath:
    """``pose_net`` (motion_model "tartan"): the PoseNet of TartanMotionNet, ``[lanes, 5, 112, 160] -> [lanes, 6]`` raw network output
    (before ``pose_norm``), called on the current stream between a frame's frontend and its finish."""

    def __init__(self, cam: Camera, cfg: HotPathConfig | None = None, device: str | torch.device = "cuda",
                 keep_extras: bool = False, pose_net=None, generator: "torch.Generator | None" = None):
        self.cam, self.cfg = cam, cfg or HotPathConfig()
        _check_motion(self.cfg)
        check_selector(self.cfg, cam)
        check_frontend_cov(self.cfg)
        check_keyframes(self.cfg)
        self._fcov = ops.frontend_cov_flags(self.cfg.frontend_cov)
        self._prev_prior = None                   # the pose the previous keyframe was pushed with (= what a skipped frame's row holds)
        self._prev_prior_ev = None
        self._skipped = False                     # a frame has been skipped since the previous keyframe
        self._n_key_enq = self._n_key_fin = 0
        self._skip_queue: list = []               # (keyframes that must have finished first, time_ns)
        self._map = None
        self.pose_net = pose_net
        self.generator = generator   # CPU generator of the selector's draws (None: torch's global one, which is what the reference consumes)
        self.dev = torch.device(device)
        self.keep_extras = keep_extras
        self.lm = ops.lm_default_params()
        self.maps_prev_for_next: ops.FrontendMaps | None = None   # depth maps of the newest frontend'ed frame
        self._side = torch.cuda.Stream(device=self.dev, priority=-1)      # PGO stream
        self._back = torch.cuda.Stream(device=self.dev, priority=-1)      # pose-dependent half of a frame (tracking .. filter)
        self._perm_pinned = [torch.empty((max(self.cfg.num_point, 1),), dtype=torch.int64, pin_memory=True) for _ in range(4)]
        self._perm_slot = 0
        self._graphs: dict = {}                   # (id(inputs), slot) -> captured decoder-side segment
        self._frame_no = 0
        self._pgo_done = None
        self._pgo_keep = None
        self._map_done = None
        self._prev_image = None
        self.pose = torch.tensor([0, 0, 0, 0, 0, 0, 1], dtype=torch.float32, device=self.dev)
        c = self.cfg
        self._max_depth = cam.fx * cam.baseline if c.max_depth == "auto" else float(c.max_depth)
        self._intr = torch.tensor([cam.K4], dtype=torch.float32, device=self.dev)
        self._bl = torch.tensor([cam.baseline], dtype=torch.float32, device=self.dev)
        self._vols = [None, None]                 # double-buffered cost volumes (184 MB each @640x480, B = 2)
        self._vol_free = [None, None]             # event: the last reader (lookups) of that buffer has finished
        self._vol_idx = 0
        # the GEMM stream gets the LOWEST priority: whenever CU slots free up, the small latency-bound kernels of the other
        # streams (lookups, selector, backend, PGO) should be dispatched first and the GEMM fills whatever is left
        self._vol_stream = torch.cuda.Stream(device=self.dev, priority=0)
        self._tok = None
        self.last_tokens = None
        # offsets table: row n = [0, n] (one problem of n points) — avoids an H2D copy per frame
        m = table_rows(self.cfg, cam) + 1
        self._offs = torch.stack([torch.zeros(m, dtype=torch.int32), torch.arange(m, dtype=torch.int32)], 1).to(self.dev)

    # ------------------------------------------------------------------ frontend part of the hot path
    def _volume(self, x: FrameInputs):
        """The MFMA-bound volume GEMM of THIS frame runs on its own stream and overlaps the latency-bound decoder-side
        work (lookups, selector, backend) of the PREVIOUS frame that is still queued on the other streams — the two
        frontends are independent (Frontend.py:219-224).  Two volume buffers alternate; a buffer is rewritten only
        after the lookups that read it have finished."""
        c = self.cfg
        main = torch.cuda.current_stream()
        slot = self._frame_no % 6
        self._frame_no += 1
        k = slot & 1
        n_rows = x.fmap1.shape[0] * x.coords.shape[-1] * x.coords.shape[-2]
        if self._vols[k] is not None and self._vols[k].shape[0] != n_rows:
            self._vols[k] = None
        vs = self._vol_stream
        if x.ready is not None:
            vs.wait_event(x.ready)            # producer of the feature maps (the encoder) signals readiness
        if self._vol_free[k] is not None:
            vs.wait_event(self._vol_free[k])
        with torch.cuda.stream(vs):
            self._vols[k] = ops.corr_volume(x.fmap1, x.fmap2, layout=c.feature_layout, out=self._vols[k],
                                            precision=c.volume_precision if x.fmap1.dtype == torch.float32 else "exact")
            vol_done = torch.cuda.Event()
            vol_done.record(vs)
        main.wait_event(vol_done)
        return self._vols[k], k, slot

    def _decoder_side(self, x: FrameInputs, vol: torch.Tensor, with_selector: bool):
        """12 x window lookup + (convex upsampling) + epilogue + dense selector stage: everything between the volume and
        the host's randperm.  Pure enqueue (graph-capturable)."""
        c, cam = self.cfg, self.cam
        tok = None
        for it in range(x.coords.shape[0]):
            tok = ops.corr_lookup(vol, x.coords[it], c.radius, out=tok)
        fd, fm = self._fcov
        win = ops.unpad_window(cam.H, cam.W) if x.flow8 is not None else None   # (a frame with a pad: the un-padded window only, as the native driver does)
        if win is not None:
            check_frame_shapes(x, cam)
        if x.flow8 is not None and fd and fm:
            flow = ops.convex_upsample(x.flow8, x.up_mask, mask_scale=0.25, crop=win)
            cov = ops.convex_upsample(x.cov8, x.cov_mask, mask_scale=1.0, exp2_out=True, crop=win)     # exp(2*cov) fused
            maps = ops.frontend_epilogue(flow, cov, cam.baseline, cam.fx, cov_is_log=False)
        elif x.flow8 is not None:
            # a side without covariance: no covariance upsampling for its pair (pair 0 = the depth model's, pair 1 = the matcher's)
            flow = ops.convex_upsample(x.flow8, x.up_mask, mask_scale=0.25, crop=win)
            cov = None
            if fd or fm:
                k = 0 if fd else 1
                cov = torch.empty_like(flow)
                cov[k: k + 1] = ops.convex_upsample(x.cov8[k: k + 1], x.cov_mask[k: k + 1], mask_scale=1.0, exp2_out=True, crop=win)
            maps = ops.frontend_epilogue(flow, cov, cam.baseline, cam.fx, cov_is_log=False, provide_cov=(fd, fm))
        elif not (fd and fm):
            maps = ops.frontend_epilogue(x.flow, x.logcov if (fd or fm) else None, cam.baseline, cam.fx, cov_is_log=x.cov_is_log, provide_cov=(fd, fm))
        else:
            maps = ops.frontend_epilogue(x.flow, x.logcov, cam.baseline, cam.fx, cov_is_log=x.cov_is_log)
        cands = None
        if with_selector:
            cands = ops.kp_select("nodepth", cam.H, cam.W, flow_cov=maps.flow_cov, kernel_size=c.kp_kernel_size,
                                  mask_width=c.kp_mask_width, max_match_cov=c.max_match_cov)
        return tok, maps, cands

    def frontend(self, x: FrameInputs, with_selector: bool = False):
        """volume -> decoder side; returns (maps, cands | None, host_count | None).  With ``use_graphs`` and a ``static``
        input the decoder side is one hipGraph replay (12 lookups + epilogue + selector + count copy = 17 nodes)."""
        c = self.cfg
        vol, k, slot = self._volume(x)
        main = torch.cuda.current_stream()
        graphable = c.use_graphs and x.static and with_selector and c.selector == "nodepth"
        host_count = None
        if graphable:
            key = (id(x), slot)
            g = self._graphs.get(key)
            if g is None:
                # eager warm-up (lazy initialisations must not happen under capture), then capture
                self._decoder_side(x, vol, True)
                hc = torch.empty((4,), dtype=torch.int32, pin_memory=True)
                main.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    tok, maps, cands = self._decoder_side(x, vol, True)
                    hc.copy_(cands.count, non_blocking=True)
                g = (graph, tok, maps, cands, hc, x, vol)
                self._graphs[key] = g
            graph, tok, maps, cands, host_count = g[:5]
            graph.replay()
            cands._n = None
        else:
            tok, maps, cands = self._decoder_side(x, vol, with_selector and c.selector == "nodepth")
            if cands is not None:
                host_count = torch.empty((4,), dtype=torch.int32, pin_memory=True)
                host_count.copy_(cands.count, non_blocking=True)
        free = torch.cuda.Event()
        free.record(main)
        self._vol_free[k] = free
        self.last_tokens = tok
        return maps, cands, host_count

    def initialize(self, x: FrameInputs, init_pose: torch.Tensor | None = None) -> None:
        """Frame 0: ``MACVO.initialize`` (:158-171) — depth only, pose = prior."""
        self.maps_prev_for_next = self.frontend(x)[0]
        self._prev_image = x.image
        if init_pose is not None:
            self.pose = init_pose.to(self.dev, torch.float32).reshape(7).clone()
        self._prev_prior, self._prev_prior_ev, self._skipped = self.pose, None, False
        self._frame_index = 0

    def attach_map(self, devmap, K: torch.Tensor, T_BS: torch.Tensor | None = None) -> None:
        """The map :meth:`skip` registers non-keyframes in (only the driver knows the pose a skipped row carries).  Keyframes are registered by the
        caller from their :class:`FrameResult` (``DeviceVisualMap.push_frame`` / ``set_pose``), as before."""
        self._map = devmap
        self._map_K = K.to(self.dev, torch.float32).reshape(3, 3).contiguous()
        self._map_TBS = (torch.tensor([0, 0, 0, 0, 0, 0, 1.0]) if T_BS is None else T_BS).to(self.dev, torch.float32).reshape(7).contiguous()

    def skip(self, time_ns: int = 0) -> None:
        """A non-keyframe (MACVO.py:177-179): nothing of it is computed.  It is registered in the attached map (if any) with ``need_interp`` and the
        pose the previous keyframe was PUSHED with — that keyframe's optimised pose is not written back before the next ``run_pair`` — and the next
        local solve takes that pose as its reference frame: ``pose[frame_idx - 1]`` is this row (Optimizer.py:119-121).  Called while keyframes
        are still pending (``run``), it takes effect once they have finished."""
        if self._n_key_fin < self._n_key_enq:
            self._skip_queue.append((self._n_key_enq, int(time_ns)))
            return
        self._skip_now(time_ns)

    def _skip_now(self, time_ns: int) -> None:
        self._skipped = True
        if self._map is not None:
            if self._prev_prior_ev is not None:
                torch.cuda.current_stream().wait_event(self._prev_prior_ev)
            self._map.push_skipped(self._map_K, self._map_TBS, self.cam.baseline, int(time_ns), self._prev_prior)

    def _keyframes_of(self, frames):
        """The keyframes of ``frames`` (UniformKeyframe.isKeyframe: frame index % keyframe_freq == 0, the frame of ``initialize`` being index 0);
        the frames in between are skipped as they are passed."""
        k = self.cfg.keyframe_freq
        for x in frames:
            self._frame_index += 1
            if self._frame_index % k == 0:
                yield x
            else:
                self.skip(x.time_ns)

    def _keyframe_done(self, prior: torch.Tensor, ev) -> None:
        self._prev_prior, self._prev_prior_ev, self._skipped = prior, ev, False
        self._n_key_fin += 1

    def _flush_skips(self) -> None:
        """Deferred skips whose keyframes have finished — run() calls it once the consumer has taken that keyframe's result (and registered its row)."""
        while self._skip_queue and self._skip_queue[0][0] <= self._n_key_fin:
            self._skip_now(self._skip_queue.pop(0)[1])

    # ------------------------------------------------------------------ one run_pair, in two halves
    @traced("Frontend.estimate")
    def enqueue_frontend(self, x: FrameInputs) -> "_Pending":
        """Everything of a frame that does not depend on the previous pose: volume, lookups, epilogue and the dense
        selector stage.  Only enqueues work; the candidate count travels to a pinned host word behind an event, so a
        later ``finish`` waits for THIS frame's selector and not for whatever was queued after it."""
        c, cam = self.cfg, self.cam
        maps0 = self.maps_prev_for_next
        maps1, cands, host_count = self.frontend(x, with_selector=True)
        if c.selector in MAPLESS_SELECTORS or x.keypoints is not None:
            pass            # no candidate list: the keypoints are drawn / computed / taken from the caller in finish
        elif cands is None:   # CovAwareSelector needs the previous frame's depth maps: eager, after the frontend
            cands = ops.kp_select("full", cam.H, cam.W, flow_cov=maps1.flow_cov, depth0=maps0.depth,
                                  depth0_cov=maps0.depth_cov, depth1=maps1.depth, depth1_cov=maps1.depth_cov,
                                  kernel_size=c.kp_kernel_size, mask_width=c.kp_mask_width, max_depth=self._max_depth,
                                  max_depth_cov=c.max_depth_cov, max_match_cov=c.max_match_cov)
            host_count = torch.empty((4,), dtype=torch.int32, pin_memory=True)
            host_count.copy_(cands.count, non_blocking=True)
        cands_m = host_count_m = None
        if c.mapping:   # MappingPointSelector works on the PREVIOUS frame's depth maps (KeypointSelector.py:87-97): count travels with the other one
            cands_m = ops.kp_select("mapping", cam.H, cam.W, depth0=maps0.depth, depth0_cov=maps0.depth_cov,
                                    mask_width=c.map_mask_width, max_depth=c.map_max_depth, max_depth_cov=c.map_max_depth_cov)
            host_count_m = torch.empty((4,), dtype=torch.int32, pin_memory=True)
            host_count_m.copy_(cands_m.count, non_blocking=True)
        motion_in = None
        if c.motion_model == "tartan":   # TartanMotionNet.predict's input (MotionModel.py:112): temporal flow + depth of frame t
            motion_in = ops.motion_input(maps1.flow, maps1.depth, cam.fx, cam.fy, cam.cx, cam.cy, cam.baseline)
        ev = torch.cuda.Event()
        ev.record()
        self.maps_prev_for_next = maps1
        pend = _Pending(maps0, maps1, cands, host_count, ev)
        pend.motion_in = motion_in
        if motion_in is not None and self.pose_net is not None:
            # the PoseNet right behind the frame's frontend (between enqueue and finish, MACVO.py:194): in run() it is queued before the NEXT
            # frame's frontend, so the frame's finish does not wait for that
            pend.motion = self.pose_net(motion_in)
            pend.motion_ev = torch.cuda.Event()
            pend.motion_ev.record()
        pend.cands_m, pend.host_count_m, pend.image0 = cands_m, host_count_m, self._prev_image
        pend.keypoints, pend.keypoint_counts = x.keypoints, x.keypoint_counts
        self._prev_image = x.image
        self._n_key_enq += 1
        return pend

    def pose_motion(self, pend: "_Pending") -> torch.Tensor:
        """The raw PoseNet output ``[1, 6]`` of a pending frame (motion_model "tartan"), on the current stream."""
        if self.pose_net is None:
            raise ops.L.MacvoHipError("motion_model='tartan' needs a pose_net ([lanes,5,112,160] -> [lanes,6])")
        return self.pose_net(pend.motion_in)

    @traced("Odom_Runtime")
    def finish(self, pend: "_Pending", pose_sink: torch.Tensor | None = None, motion: torch.Tensor | None = None) -> FrameResult:
        """Host randperm (bit-exact indices) + the pose-dependent half: tracking, back-projection, covariances, filter,
        PGO.  The solve runs on a side stream (the GPU analogue of the reference's optimizer child process,
        Optimization/Interface.py:80-96): the next frame's frontend overlaps it, the next frame's back-projection
        waits for it.  motion_model "tartan": ``motion`` is the frame's raw PoseNet output (default: ``pose_net`` on the frame's
        ``motion_in``); the prior ``pose of frame t-1 @ Exp(motion * pose_norm)`` is where LM starts and what a lost-track frame keeps,
        while the world registration still uses the pose of frame t-1 (MACVO.py:193-194,273-281,303-307)."""
        c, cam = self.cfg, self.cam
        self._flush_skips()
        maps0, maps1, cands = pend.maps0, pend.maps1, pend.cands
        motion_ev = None
        if c.motion_model == "tartan":
            if motion is None and pend.motion is not None:
                motion, motion_ev = pend.motion, pend.motion_ev
            else:
                if motion is None:
                    motion = self.pose_motion(pend)
                motion_ev = torch.cuda.Event()
                motion_ev.record()
        mapless = c.selector in MAPLESS_SELECTORS or pend.keypoints is not None
        if not mapless:
            pend.event.synchronize()
            cands._n = int(pend.host_count[0])
        back, side = self._back, self._side
        # The backend runs on its own stream: it must not queue behind the NEXT frame's decoder-side work that
        # enqueue_frontend already put on the main stream (that work waits for the next volume GEMM).
        back.wait_event(pend.event)
        with torch.cuda.stream(back):
            self._perm_slot = (self._perm_slot + 1) % len(self._perm_pinned)
            if pend.keypoints is not None:
                kp0 = pend.keypoints.reshape(-1, 2)
                if pend.keypoint_counts is not None:
                    kp0 = kp0[: int(pend.keypoint_counts[0])]
                if kp0.shape[0] > table_rows(c, cam):
                    raise ValueError(f"{kp0.shape[0]} explicit keypoints > the table capacity {table_rows(c, cam)}")
                if not kp0.is_cuda:
                    check_keypoints(kp0, c, cam)
                kp0 = kp0.to(self.dev, torch.int64).contiguous()
            elif c.selector == "explicit":
                raise ValueError("selector 'explicit': the frame carries no keypoints (FrameInputs.keypoints / step(..., keypoints=))")
            elif c.selector == "random":   # torch.randint on the CPU generator, exactly as the reference (KeypointSelector.py:103-118)
                kp0 = _randint_rows(c.num_point, cam.H, cam.W, c.kp_mask_width, self.generator).to(self.dev)
            elif c.selector == "grid":
                kp0 = ops.kp_grid(cam.H, cam.W, c.kp_mask_width, c.num_point, self.dev)
            else:
                kp0 = cands.finish(c.num_point, staging=self._perm_pinned[self._perm_slot], generator=self.generator)  # CPU randperm, as the reference
            n = kp0.shape[0]
            if self._pgo_done is not None:
                back.wait_event(self._pgo_done)   # self.pose of the previous frame is produced on the PGO stream
            prev_pose = prior = self.pose

            def compose():   # the prior, behind the PoseNet: only the solve (and a frame without keypoints) needs it
                back.wait_event(motion_ev)
                return ops.pose_exp_compose(prev_pose, motion.reshape(6).to(torch.float32))
            if n == 0:
                if motion_ev is None:
                    self._keyframe_done(self.pose, self._pgo_done)
                    return FrameResult(self.pose, None, None, kp0, None)
                prior = compose()
                # nothing tracked: the frame keeps the motion-model prior (MACVO.py:303-307), and the next prior composes onto it
                done = torch.cuda.Event()
                done.record(back)
                self._pgo_done = done
                self._pgo_keep = (self._pgo_keep[1] if self._pgo_keep else None, (motion, kp0, cands, pend, prev_pose))
                self.pose = prior
                self._keyframe_done(prior, done)
                return FrameResult(prior, None, None, kp0, None, prior=prior)

            tr = ops.kp_track(kp0, maps1.flow, maps1.flow_cov, maps0, maps1, c.edgewidth, c.match_cov_default)
            pos0_Tc, pos_Tw, rot = ops.backproject(tr.kp0_uv, tr.vals[0], cam.K4, prev_pose, want_rot=True)
            # a matcher that gives no covariance: tr.sigma1 holds the -1 placeholders, the second call is the model with flow_cov=None
            no_match_cov = not self._fcov[1]
            cov0, cov0_w, cov1 = ops.obs_cov_pair(c.cov_model, maps0.depth, tr.kp0_uv, tr.sigma0, maps1.depth, tr.kp1_uv,
                                                  None if no_match_cov else tr.sigma1, *cam.K4,
                                                  depth_cov_map0=maps0.depth_cov, depth_cov_map1=maps1.depth_cov,
                                                  modifiers=c.cov_modifiers, rot=rot, kernel_size=c.cov_kernel_size,
                                                  min_flow_cov=c.min_flow_cov, min_depth_cov=c.min_depth_cov, no_match_cov=no_match_cov,
                                                  match_cov_default=c.cov_match_cov_default,
                                                  depth_cov1=tr.vals[7] if no_match_cov and self._fcov[0] else None)
            valid, n_valid = ops.obs_filter(tr.inbound, cov0, cov1, tr.vals, c.filters, c.filter_min_depth, self._max_depth)
            if motion_ev is not None:
                prior = compose()

            batch = ops.PGOBatch(
                offsets=self._offs[n], init_pose=prior.reshape(1, 7), intrinsics=self._intr, baseline=self._bl,
                pos_Tw=pos_Tw, pixel2_uv=tr.kp1_uv, cov_Tw=cov0_w, pixel2_d=tr.vals[4], pixel2_disp=tr.vals[5],
                pixel2_disp_cov=tr.vals[6], pixel2_uv_cov=tr.sigma1, obs2_covTc=cov1, valid=valid)
            ready = torch.cuda.Event()
            ready.record(back)
        side.wait_event(ready)
        with torch.cuda.stream(side):
            new_pose = torch.empty((1, 7), dtype=torch.float32, device=self.dev)
            # the local solve's frame is pose[frame_idx - 1] (Optimizer.py:119-121): the previous keyframe's row — its current pose, the one the
            # rows were registered with — or, behind a skipped frame, that frame's row, which holds the previous keyframe's prior
            ref_pose = None if c.solve_frame != "local" else (self._prev_prior if self._skipped else prev_pose).reshape(1, 7)
            pose64, info = ops.pgo_solve(batch, c.graph_type, self.lm, min_points=c.min_num_point, out_pose_f32=new_pose, ref_pose=ref_pose)
            if pose_sink is not None:
                pose_sink.copy_(new_pose.reshape(7), non_blocking=True)
            done = torch.cuda.Event()
            done.record(side)
        map_pts = None
        if c.mapping:
            # the reference maps only when tracking succeeded (:303-307) and then draws its second randperm of the frame
            ready.synchronize()
            if int(n_valid.item()) >= c.min_num_point:
                pend.cands_m._n = int(pend.host_count_m[0])
                with torch.cuda.stream(back):
                    muv = pend.cands_m.finish(c.map_num_point, generator=self.generator)
                    map_pts = ops.map_points(muv, maps0.depth, maps0.depth_cov, cam.K4, prev_pose.reshape(1, 7), image=pend.image0,
                                             match_cov_default=c.match_cov_default, kernel_size=c.cov_kernel_size,
                                             min_flow_cov=c.min_flow_cov, min_depth_cov=c.min_depth_cov, cov_model=c.cov_model,
                                             cov_modifiers=c.cov_modifiers)
                    self._map_done = torch.cuda.Event()
                    self._map_done.record(back)
        self._pgo_done = done
        self._pgo_keep = (self._pgo_keep[1] if self._pgo_keep else None, (batch, tr, cov0, cov1, maps0, maps1, kp0, pos0_Tc, cands, pend,
                                                                           prev_pose, motion))  # keep 2 frames of cross-stream tensors alive
        self.pose = new_pose.reshape(7)
        self._keyframe_done(prior, ready)
        res = FrameResult(self.pose, pose64, info, kp0, n_valid, prior=prior if motion_ev is not None else None)
        res.map_points = map_pts
        if self.keep_extras:
            res.extras = dict(tracked=tr, cov0=cov0, cov0_w=cov0_w, cov1=cov1, valid=valid, pos_Tw=pos_Tw,
                              maps1=maps1, cands=cands)
        return res

    def step(self, x: FrameInputs, keypoints: torch.Tensor | None = None) -> FrameResult:
        """One ``run_pair`` start to finish (no cross-frame overlap); results are valid on the current stream.  ``keypoints``: this frame's
        keypoints (see :class:`FrameInputs`), instead of ``x.keypoints``."""
        assert self.maps_prev_for_next is not None, "call initialize() with the first frame"
        if keypoints is not None:
            x = replace(x, keypoints=keypoints, keypoint_counts=None)
        res = self.finish(self.enqueue_frontend(x))
        self.sync_pose()
        return res

    def sync_pose(self) -> None:
        """Make the current stream wait for the in-flight solve (needed before reading ``self.pose`` there)."""
        if self._pgo_done is not None:
            torch.cuda.current_stream().wait_event(self._pgo_done)
        if getattr(self, "_map_done", None) is not None:
            torch.cuda.current_stream().wait_event(self._map_done)

    def run(self, frames, pose_sink: torch.Tensor | None = None):
        """Software-pipelined stream: frame t+1's frontend is enqueued before frame t's host-side randperm, so the GPU
        never idles on the selector's host round trip.  Yields a FrameResult per KEYFRAME (same results as ``step``).  ``keyframe_freq`` k > 1:
        frame i of ``frames`` (the frame after ``initialize``'s has index 1) is a keyframe when ``i % k == 0``; the others are not enqueued — only
        their ``time_ns`` is read (:meth:`skip`)."""
        it = self._keyframes_of(frames)
        try:
            nxt = self.enqueue_frontend(next(it))
        except StopIteration:
            return
        i = 0
        while nxt is not None:
            cur = nxt
            try:
                nxt = self.enqueue_frontend(next(it))
            except StopIteration:
                nxt = None
            yield self.finish(cur, None if pose_sink is None else pose_sink[i])
            self._flush_skips()
            i += 1
        self.sync_pose()


@dataclass
class _Pending:
    maps0: "ops.FrontendMaps"
    maps1: "ops.FrontendMaps"
    cands: "ops.KeypointCandidates"
    host_count: torch.Tensor
    event: "torch.cuda.Event"
    cands_m: "ops.KeypointCandidates | None" = None     # mapping mode
    host_count_m: torch.Tensor | None = None
    image0: torch.Tensor | None = None
    motion_in: torch.Tensor | None = None                # motion_model "tartan": the PoseNet input [1, 5, 112, 160]
    motion: torch.Tensor | None = None                   # ... the PoseNet's raw output, when HotPath.pose_net ran it behind the enqueue
    motion_ev: "torch.cuda.Event | None" = None
    keypoints: torch.Tensor | None = None                # caller-supplied keypoints of the frame (FrameInputs.keypoints)
    keypoint_counts: "list | None" = None


# ====================================================================================== native driver (default)
def stack_lanes(inputs: "list[FrameInputs]") -> FrameInputs:
    """Batch the per-sequence inputs of ``len(inputs)`` independent sequences ("lanes") along the pair axis — the
    reference's batching point (``Frontend.py:219-224``): lane l contributes pairs 2l (stereo) and 2l + 1 (temporal)."""
    # the per-lane inputs may have been produced on other streams: the concatenation below runs on the current one
    for x in inputs:
        if x.ready is not None:
            torch.cuda.current_stream().wait_event(x.ready)
    # images feed the dense-mapping tail, which is one lane per pipe, so per-lane images have no consumer in a batched step: refuse them rather than
    # drop them silently; the lanes advance in lock-step: `time_ns` stays lane 0's timestamp, `lane_time_ns` carries every lane's (one map per lane)
    assert len(inputs) == 1 or all(x.image is None for x in inputs), "stack_lanes: per-lane images are not carried"
    cat = lambda name, dim=0: (None if getattr(inputs[0], name) is None  # noqa: E731
                               else torch.cat([getattr(x, name) for x in inputs], dim=dim).contiguous())
    kps = None
    if any(x.keypoints is not None for x in inputs):   # per-lane [n_l, 2] rows -> [lanes, max n, 2] + counts
        assert all(x.keypoints is not None for x in inputs), "stack_lanes: keypoints for every lane or for none"
        rows = [x.keypoints.reshape(-1, 2) if x.keypoint_counts is None else x.keypoints.reshape(-1, 2)[: int(x.keypoint_counts[0])] for x in inputs]
        kps = rows[0].new_zeros((len(rows), max(r.shape[0] for r in rows), 2))
        for l, r in enumerate(rows):
            kps[l, : r.shape[0]] = r
    return FrameInputs(fmap1=cat("fmap1"), fmap2=cat("fmap2"), coords=cat("coords", 1), flow=cat("flow"), logcov=cat("logcov"),
                       flow8=cat("flow8"), cov8=cat("cov8"), up_mask=cat("up_mask"), cov_mask=cat("cov_mask"),
                       keypoints=kps, keypoint_counts=None if kps is None else [r.shape[0] for r in rows],
                       image=inputs[0].image if len(inputs) == 1 else None, time_ns=inputs[0].time_ns,
                       lane_time_ns=[int(x.time_ns) for x in inputs], static=all(x.static for x in inputs))


class _NativeResult:
    """Result of one natively driven frame of one lane.  Every tensor is a VIEW into the pipe's arena: valid until two
    more frames have been finished (slots rotate); clone what must live longer."""

    def __init__(self, hp: "NativeHotPath", lane: int, n_sel: "int | None", n_cand: "int | None"):
        self._hp, self.lane, self._n_sel, self._n_cand = hp, lane, n_sel, n_cand
        self._fin = hp._n_fin          # finish counter at creation: views are resolved against it
        self._extras: "dict | None" = None
        self.map_points = None          # mapping mode: ops.MapPoints views of the frame's dense map points

    # Device-driven frames (round 6): the counts never reach the host on their own — the first access reads them back from the frame's backend slot
    # (blocks until that frame's front launch has run; off the hot path).
    def _resolve(self) -> None:
        if self._n_sel is None:
            self._n_cand, self._n_sel = self._hp._finished_counts(self._fin, self._age(), self.lane)

    @property
    def n_sel(self) -> int:
        self._resolve()
        return self._n_sel

    @property
    def n_cand(self) -> int:
        self._resolve()
        return self._n_cand

    @property
    def extras(self) -> dict:
        if self._extras is None:
            self._extras = self._hp._extras_of(self) if self._hp.keep_extras else {}
        return self._extras

    def _age(self) -> int:
        age = self._hp._n_fin - self._fin
        if age > 1:
            raise ops.L.MacvoHipError("this frame's buffers were recycled (results are views; clone them earlier)")
        return age

    def _rows(self, name, dtype, tail=()):
        """[n_sel, *tail] live rows of this lane in a per-keypoint table [lanes, cap, *tail]."""
        hp = self._hp
        return hp._view(name, self._age(), dtype, (hp.lanes, hp._cap) + tuple(tail))[self.lane, : self.n_sel]

    def _per_lane(self, name, dtype, tail):
        hp = self._hp
        return hp._view(name, self._age(), dtype, (hp.lanes,) + tuple(tail))[self.lane]

    @property
    def pose(self):
        """fp32 [7]: this lane's optimised pose (valid on a stream after ``sync_pose``)."""
        return self._per_lane("POSE", torch.float32, (7,))

    @property
    def prior(self):
        """motion_model "tartan": fp32 [7], this lane's motion-model prior (the LM start); None for the static model."""
        return self._per_lane("PRIOR", torch.float32, (7,)) if self._hp.cfg.motion_model == "tartan" else None

    @property
    def kp0_uv(self):
        return self._rows("KP0", torch.int64, (2,))

    @property
    def n_valid(self):
        return self._per_lane("NVALID", torch.int32, ())[None] if self.n_sel else None

    @property
    def pose_f64(self):
        return self._per_lane("POSE64", torch.float64, (7,))[None] if self.n_sel else None

    @property
    def info(self):
        return self._per_lane("INFO", torch.float64, (4,))[None] if self.n_sel else None


class NativeHotPath:
    """Same contract as :class:`HotPath`, but the per-frame sequencing (streams, events, buffer rotation, ~30 launches)
    runs in C++ (``mv_frame_pipe_*``, csrc/frame_pipe.hip): two host calls per frame instead of ~30 Python-level ones.
    The Python loop was interpreter-bound (~370 us/frame, more than the GPU work); kernels, launch order and arguments
    are identical, so results are bit-identical to :class:`HotPath` (tests/test_gpu_native.py).

    ``lanes`` > 1 (BASELINE configs[4], "batch-32 frames per GPU"): that many INDEPENDENT sequences advance in lock-step
    through the same launches — one volume GEMM over ``2 * lanes`` pairs, lane-batched lookups / epilogue / selector /
    backend kernels, one batched LM solve.  Inputs are the per-lane :class:`FrameInputs` concatenated along the pair axis
    (:func:`stack_lanes`); ``finish`` then returns one result per lane.  Each lane draws its keypoint permutation from its
    own CPU generator (``generators[l]``; ``None`` = torch's global generator, which is what the reference consumes), in
    lane order — a lane seeded like a stand-alone run therefore selects exactly the keypoints of that stand-alone run."""

    def __init__(self, cam: Camera, cfg: HotPathConfig | None = None, device: str | torch.device = "cuda",
                 keep_extras: bool = False, lanes: int = 1, generators: "list | None" = None, pose_net=None):
        self.cam, self.cfg = cam, cfg or HotPathConfig()
        _check_motion(self.cfg)
        check_selector(self.cfg, cam)
        check_frontend_cov(self.cfg)
        check_keyframes(self.cfg)
        self._skip_queue: list = []      # (finishes that must have happened first, time_ns)
        self._frame_index = 0
        self.pose_net = pose_net   # motion_model "tartan": [lanes, 5, 112, 160] -> [lanes, 6], run right behind each tracked frame's enqueue
        if self.cfg.mapping and lanes != 1:
            raise ops.L.MacvoHipError("the dense-mapping tail (mapping=True) runs one sequence per pipe (lanes == 1), as the reference does")
        if self.cfg.use_graphs:
            raise ops.L.MacvoHipError("use_graphs belongs to the Python-sequenced pipeline.HotPath")
        if not 1 <= lanes <= ops.L.MV_MAX_LANES:
            raise ops.L.MacvoHipError(f"lanes must be in [1, {ops.L.MV_MAX_LANES}]")
        self.dev = torch.device(device)
        self.keep_extras = keep_extras
        self.lanes = int(lanes)
        self.generators = list(generators) if generators is not None else [None] * self.lanes
        assert len(self.generators) == self.lanes
        # integer entries = seeds of NATIVE per-lane generators (mv_frame_pipe_seed_lanes: MT19937 + Fisher-Yates in C++, the bits of
        # torch.Generator().manual_seed(seed) + torch.randperm at ~1/20 of the host time — what many-lane steps need)
        self._native_seeds = all(isinstance(g, int) and not isinstance(g, bool) for g in self.generators)
        if not self._native_seeds and any(isinstance(g, int) for g in self.generators):
            raise ops.L.MacvoHipError("generators: either all torch.Generator / None or all integer seeds")
        if self._native_seeds and self.cfg.mapping:
            raise ops.L.MacvoHipError("mapping=True draws its second permutation on the Python side: use torch generators")
        self._prev_image = None          # mapping: LEFT image of the previously enqueued frame (map-point colours, MACVO.py:326-328)
        self._images: list = []
        self._cap = max(table_rows(self.cfg, cam), 1)      # the driver's capacity rule (mv_frame_pipe_table_rows)
        self._frame_rows = (ops.kp_grid_count(cam.H, cam.W, self.cfg.kp_mask_width, self.cfg.num_point) if self.cfg.selector == "grid"
                            else self.cfg.num_point)
        # "grid": nothing in a frame waits for the host either (the rows are computed inside the front launch) — run() drives it like a device-driven frame
        self._hostless = self.cfg.selector == "grid" and not self.cfg.mapping
        self._kp = torch.zeros((self.lanes, self._cap, 2), dtype=torch.int64)   # host staging of keypoint rows
        self._kps: list = []             # keypoints of the enqueued, unfinished frames (FrameInputs.keypoints; None: the pipe's own selector)
        self._kp_keep: list = []         # device keypoints / counts of the newest finishes (read asynchronously by the pipe)
        self._volume_ahead = os.environ.get("MV_PIPE_VOLUME_AHEAD", "1") != "0"   # A/B knobs of run()
        # frames in flight: never more than the slot rotation the library was built with (MV_MAX_PENDING, 3 in the stock build)
        # The default follows the stream layout the driver picks (mv_frame_pipe_default_depth): 3 for the round-5 layout of one- and two-lane pipes (even /
        # odd frames' decoder sides on two streams: a third frame in flight keeps both fed) and for batched pipes, 2 for the classic one-lane layout
        # ([r4] there 3 bought nothing and cost a period of latency, profiles/r04_latency_ab.log)
        lib = ops.L.load()
        self._depth = max(1, min(int(lib.mv_frame_pipe_max_pending()), int(os.environ.get("MV_PIPE_MAX_DEPTH", "3")),
                                 int(os.environ.get("MV_PIPE_DEPTH", str(lib.mv_frame_pipe_default_depth(self.lanes, int(bool(self.cfg.mapping))))))))
        self.lm = ops.lm_default_params()
        self._pipe = None
        self._arena = None
        self._views: dict = {}
        self._n_fin = 0
        self._n_enq = 0
        self._pending: list = []
        self._init_pose = None
        self._ncand = (ops.C.c_int32 * self.lanes)()
        self._nsel = (ops.C.c_int32 * self.lanes)()
        self._perm = torch.zeros((self.lanes, self._cap), dtype=torch.int64)
        self._ptr = ops.C.c_void_p()
        self._cnt = ops.C.c_size_t()

    # ------------------------------------------------------------------ construction (needs the first input's shapes)
    def _create(self, x: FrameInputs) -> None:
        L, C = ops.L, ops.C
        c, cam = self.cfg, self.cam
        lib = L.load()
        hwc = c.feature_layout == "hwc"
        pairs = x.fmap1.shape[0]
        if pairs != 2 * self.lanes:
            raise L.MacvoHipError(f"inputs carry {pairs} pairs but the pipe has {self.lanes} lane(s) (2 pairs per lane)")
        chans = x.fmap1.shape[-1] if hwc else x.fmap1.shape[1]
        check_frame_shapes(x, cam)
        dt = {torch.float32: L.MV_F32, torch.float16: L.MV_F16, torch.bfloat16: L.MV_BF16}[x.fmap1.dtype]
        bl_fx = float(cam.baseline) * float(cam.fx)
        max_depth = cam.fx * cam.baseline if c.max_depth == "auto" else float(c.max_depth)
        pc = L.mvFramePipeConfig(
            H=cam.H, W=cam.W, C=chans, pairs=pairs, iters=x.coords.shape[0], radius=c.radius, feat_dtype=dt,
            layout=L.MV_LAYOUT_HWC if hwc else L.MV_LAYOUT_CHW, volume_split={"exact": 0, "split3": 3, "split2": 2, "bf16x3": L.MV_PACK_BF16X3, "f16x2": L.MV_PACK_F16X2}[c.volume_precision] if dt == L.MV_F32 else (L.MV_VOL_ENC16 if (c.volume_store == "encoder" and dt == L.MV_F16 and c.radius == 4) else 0),   # 16-bit features: one kernel family
            selector_mode={"nodepth": L.MV_KP_NODEPTH, "full": L.MV_KP_FULL, "random": L.MV_KP_RANDOM, "grid": L.MV_KP_GRID,
                           "explicit": L.MV_KP_EXPLICIT}[c.selector],
            kp_kernel_size=c.kp_kernel_size, kp_mask_width=c.kp_mask_width, num_point=c.num_point, edgewidth=c.edgewidth,
            min_num_point=c.min_num_point, graph_type=ops._GRAPH[c.graph_type], filters=c.filters,
            cov_kernel_size=c.cov_kernel_size, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, baseline=cam.baseline,
            bl_fx=bl_fx, bl_fx_sq=bl_fx ** 2, match_cov_default=c.match_cov_default, max_match_cov=c.max_match_cov,
            max_depth_cov=c.max_depth_cov, max_depth=max_depth, min_flow_cov_sq=c.min_flow_cov ** 2,
            min_depth_cov=c.min_depth_cov, filter_min_depth=c.filter_min_depth, mapping=int(c.mapping), map_num_point=c.map_num_point,
            map_mask_width=c.map_mask_width, async_backend=0 if c.async_backend is None else (1 if c.async_backend else -1), map_max_depth=c.map_max_depth, map_max_depth_cov=c.map_max_depth_cov, lm=self.lm,
            cov_model=ops._cov_model(c.cov_model), cov_modifiers=ops.cov_modifier_chain(c.cov_modifiers),
            motion_model=L.MV_MOTION_TARTAN if c.motion_model == "tartan" else L.MV_MOTION_STATIC,
            frontend_nocov=_nocov_mask(c), cov_match_cov_default=c.cov_match_cov_default)
        nbytes = lib.mv_frame_pipe_arena_bytes(C.byref(pc))
        if nbytes == 0:
            raise L.MacvoHipError("mv_frame_pipe_arena_bytes: invalid configuration")
        self._arena = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.dev)
        self._base = (self._arena.data_ptr() + 255) & ~255
        pipe = C.c_void_p()
        L.check(lib.mv_frame_pipe_create(C.byref(pc), self._base, nbytes, C.byref(pipe)), "mv_frame_pipe_create")
        self._pipe, self._lib, self._pc = pipe, lib, pc
        if c.solve_frame == "local":      # (a pipe on which this is never called issues exactly the world-frame launches)
            L.check(lib.mv_frame_pipe_set_solve_frame(pipe, L.MV_SOLVE_LOCAL), "mv_frame_pipe_set_solve_frame")
        self.device_driven = False
        if self._native_seeds:
            seeds = (C.c_uint64 * self.lanes)(*[int(g) & 0xFFFFFFFFFFFFFFFF for g in self.generators])
            L.check(lib.mv_frame_pipe_seed_lanes(pipe, seeds), "mv_frame_pipe_seed_lanes")
            # round 6: the generators also live in device memory and — wherever it applies — the frame is device-driven: the permutation head is drawn
            # inside the backend's front launch, `finish` never waits for the GPU (csrc/frame_pipe.hip, csrc/randperm_dev.h; MV_PIPE_DEVICE_DRAW=0 restores
            # the host draw).  Same keypoints, same poses (tests/test_gpu_lanes.py).
            self.device_driven = bool(lib.mv_frame_pipe_device_draw(pipe))
        # the volume buffers hold every query's slice in 4 x 4-cell tiles (Fast-mode pipes; MV_PIPE_TILED): read them with corr_lookup(tiled=True)
        self.volume_tiled = bool(lib.mv_frame_pipe_volume_tiled(pipe))
        self.host_threads = int(lib.mv_frame_pipe_host_threads(pipe))      # 1, or 2 with the backend launch thread
        self._counts_cache: dict = {}
        self.host_issue_s = self.host_wait_s = 0.0
        self.host_frames = 0
        if self._init_pose is not None:
            self._set_pose(self._init_pose)

    def close(self) -> None:
        """Destroy the native pipe NOW (drains its streams, frees its HIP streams / events; the arena goes back to torch's allocator).  Result objects keep a
        reference to their pipe, so dropping the last NAME of a pipe does not destroy it while any result of it is alive — and a pipe that lingers keeps its four
        HIP streams: the next pipe's streams then share hardware queues with them (measured: a 32-lane pipe at 6.3 k instead of 7.8 k frames/s behind a lingering
        one-lane pipe, profiles/probes/r6_queue_history.py).  Views handed out earlier become invalid."""
        if getattr(self, "_pipe", None):
            self._lib.mv_frame_pipe_destroy(self._pipe)
            self._pipe = None
            self._views.clear()
            self._arena = None

    def __del__(self):
        self.close()

    def _set_pose(self, pose: torch.Tensor) -> None:
        host = pose.detach().to("cpu", torch.float32).reshape(-1, 7)
        if host.shape[0] == 1 and self.lanes > 1:
            host = host.expand(self.lanes, 7)
        assert host.shape[0] == self.lanes, "pose must be [7] or [lanes, 7]"
        host = host.contiguous()
        ops.L.check(self._lib.mv_frame_pipe_set_pose(self._pipe, host.data_ptr()), "mv_frame_pipe_set_pose")

    def _view(self, name: str, age: int, dtype: torch.dtype, shape: tuple) -> torch.Tensor:
        if self._pipe is None:
            raise ops.L.MacvoHipError("this pipe has been closed (or was never created): its buffers are gone")
        ops.L.check(self._lib.mv_frame_pipe_buffer(self._pipe, ops.L.FB[name], age, ops.C.byref(self._ptr),
                                                   ops.C.byref(self._cnt)), f"mv_frame_pipe_buffer({name})")
        key = (self._ptr.value, dtype, shape)
        v = self._views.get(key)
        if v is None:
            off = self._ptr.value - self._arena.data_ptr()
            n = 1
            for s in shape:
                n *= s
            assert n <= self._cnt.value or n == 0, (name, shape, self._cnt.value)
            v = self._arena[off: off + n * torch.empty((), dtype=dtype).element_size()].view(dtype).view(shape)
            if len(self._views) > 256:
                self._views.clear()
            self._views[key] = v
        return v

    @property
    def pose(self) -> torch.Tensor:
        """fp32 ``[7]`` (``[lanes, 7]`` for lanes > 1) view of the newest solve's output (valid on a stream after
        :meth:`sync_pose`)."""
        v = self._view("POSE", 0, torch.float32, (self.lanes, 7))
        return v[0] if self.lanes == 1 else v

    @pose.setter
    def pose(self, value: torch.Tensor) -> None:
        """Override the prior of the next frame (blocking; e.g. an external motion model)."""
        if self._pipe is None:
            self._init_pose = value
        else:
            self._set_pose(value)

    @property
    def last_tokens(self) -> torch.Tensor:
        """Window-lookup output of the newest frame's last decoder iteration ``[pairs, (2r+1)^2, h8, w8]`` (``ops.eighth_shape``)."""
        k = 2 * self.cfg.radius + 1
        return self._view("TOKENS", 0, torch.float32, (self._pc.pairs, k * k) + ops.eighth_shape(self.cam.H, self.cam.W))

    def maps(self, age: int = 0, lane: int = 0) -> "ops.FrontendMaps":
        H, W = self.cam.H, self.cam.W
        v = lambda n, c: self._view(n, age, torch.float32, (self.lanes, c, H, W))[lane: lane + 1]  # noqa: E731
        fd, fm = ops.frontend_cov_flags(self.cfg.frontend_cov)    # (a covariance map the frontend does not provide does not exist in the pipe)
        return ops.FrontendMaps(v("DEPTH", 1), v("DEPTH_COV", 1) if fd else None, v("DISPARITY", 1), v("DISPARITY_COV", 1) if fd else None, None,
                                v("MATCH_FLOW", 2), v("MATCH_COV", 3) if fm else None)

    # ------------------------------------------------------------------ frame API
    def _inputs(self, x: FrameInputs):
        st = getattr(x, "_native_struct", None)
        if st is not None and x.static:
            return st
        q = lambda t, dt=torch.float32: None if t is None else ops._req(t, dt, "frame input").data_ptr()  # noqa: E731
        st = ops.L.mvFrameInputs(q(x.fmap1, x.fmap1.dtype), q(x.fmap2, x.fmap2.dtype), q(x.coords), q(x.flow), q(x.logcov),
                                 q(x.flow8), q(x.cov8), q(x.up_mask), q(x.cov_mask))
        if x.flow8 is not None:
            st.flow, st.logcov = None, None
        x._native_struct = st
        return st

    def _enqueue(self, x: FrameInputs, with_selector: bool) -> None:
        if not x.cov_is_log:
            raise ops.L.MacvoHipError("FrameInputs.cov_is_log=False (sigma^2 instead of log-sigma) is pipeline.HotPath's; the native driver takes log-sigma")
        if self._pipe is None:
            self._create(x)
        if x.ready is not None:
            torch.cuda.current_stream().wait_event(x.ready)
        ops.L.check(self._lib.mv_frame_pipe_enqueue(self._pipe, ops.C.byref(self._inputs(x)), ops._stream(),
                                                    int(with_selector)), "mv_frame_pipe_enqueue")
        self._n_enq += 1

    def attach_map(self, devmap, K: torch.Tensor, T_BS: torch.Tensor | None = None) -> None:
        """Register every finished frame in a :class:`macvo_amd.devmap.DeviceVisualMap`: the frame's
        tables go from the tracking kernels into the map's SoA stores on the pipe's own streams — no ``.cpu()`` round trip
        (the reference: Odometry/MACVO.py:235-266, ~25 device-to-host copies per frame).  lanes == 1: the one-member form of
        :meth:`attach_maps`, ``devmap`` itself is filled.  Call before :meth:`initialize`."""
        from .devmap import DeviceVisualMaps

        if self.lanes != 1:
            raise ops.L.MacvoHipError("attach_map: one map per pipe, lanes must be 1 (attach_maps takes one map per lane)")
        self._attach(DeviceVisualMaps(maps=[devmap]), K, T_BS)

    def attach_maps(self, maps, K: torch.Tensor, T_BS: torch.Tensor | None = None) -> None:
        """:meth:`attach_map` for any lane count: lane ``l``'s finished frames go into ``maps[l]`` (a :class:`macvo_amd.devmap.DeviceVisualMaps`, or a list
        of ``lanes`` :class:`DeviceVisualMap`) — what the reference's multi-sequence driver keeps per sequence (Scripts/Experiment/Experiment_MACVO.py:55-58),
        registered by one launch per frame for all lanes (mv_frame_pipe_map_append_lanes), no host wait.  ``T_BS``: ``[7]`` or ``[lanes, 7]``.  All maps must
        hold the same number of frames (the lanes advance in lock-step).  Call before :meth:`initialize`."""
        from .devmap import DeviceVisualMaps

        if self.cfg.mapping:
            raise ops.L.MacvoHipError("attach_maps: the dense-mapping tail (mapping=True) registers through attach_map (one lane, one map)")
        seq = maps.maps if isinstance(maps, DeviceVisualMaps) else list(maps)
        if len(seq) != self.lanes:
            raise ops.L.MacvoHipError(f"attach_maps: {len(seq)} map(s) for {self.lanes} lane(s)")
        if len({(m.n_frames, m.last_keyframe) for m in seq}) != 1:
            raise ops.L.MacvoHipError(f"attach_maps: every map must hold the same number of frames (the lanes advance in lock-step), got {[m.n_frames for m in seq]}")
        self._attach(maps if isinstance(maps, DeviceVisualMaps) else DeviceVisualMaps(maps=seq), K, T_BS)

    def _attach(self, maps, K: torch.Tensor, T_BS: torch.Tensor | None) -> None:
        tbs = (torch.tensor([0, 0, 0, 0, 0, 0, 1.0]) if T_BS is None else T_BS).to(self.dev, torch.float32).reshape(-1, 7)
        if tbs.shape[0] == 1:
            tbs = tbs.expand(self.lanes, 7)
        if tbs.shape[0] != self.lanes:
            raise ops.L.MacvoHipError(f"attach_maps: T_BS must be [7] or [{self.lanes}, 7]")
        self._maps = maps
        self._map_K = K.to(self.dev, torch.float32).reshape(3, 3).contiguous()
        self._map_TBS = tbs.contiguous()
        self._times = []
        if maps.stale():
            maps.upload()
        torch.cuda.synchronize()      # the descriptor array is read on the pipe's own streams

    def _lane_times(self, x: FrameInputs):
        """int64[lanes]: every lane's timestamp of a (stacked) step."""
        t = x.lane_time_ns if x.lane_time_ns is not None else [x.time_ns] * self.lanes
        if len(t) != self.lanes:
            raise ops.L.MacvoHipError(f"lane_time_ns: {len(t)} timestamps for {self.lanes} lane(s)")
        return (ops.C.c_int64 * self.lanes)(*[int(v) for v in t])

    def initialize(self, x: FrameInputs, init_pose: torch.Tensor | None = None) -> None:
        """Frame 0: ``MACVO.initialize`` (:158-171) — depth only, pose = prior."""
        self._init_pose = init_pose
        self._frame_index = 0
        self._skip_queue.clear()
        self._enqueue(x, False)
        self._prev_image = x.image
        mps = getattr(self, "_maps", None)
        if mps is not None:   # MACVO.initialize pushes the first frame at the prior (:162-169): every lane's, each at its own (once per sequence: the one-frame kernel per lane)
            pri = None if init_pose is None else init_pose.detach().to(torch.float32).reshape(-1, 7)
            times = self._lane_times(x)
            for l, m in enumerate(mps):
                m.push_frame(K=self._map_K, T_BS=self._map_TBS[l], baseline=self.cam.baseline, time_ns=times[l],
                             prior_pose=None if pri is None else pri[l if pri.shape[0] > 1 else 0])
            if mps.stale():
                mps.upload()
            torch.cuda.synchronize()   # later frames are appended on the pipe's streams: order them after this one

    def skip(self, time_ns=0) -> None:
        """A non-keyframe (MACVO.py:177-179), see :meth:`HotPath.skip` (``time_ns``: one timestamp, or one per lane with :meth:`attach_maps`): the pipe notes that the next solve's reference frame is the previous keyframe's
        prior (mv_frame_pipe_skip), and with an attached map the row is appended on the pipe's own stream with that prior copied on the device
        (mv_frame_pipe_map_skip_lanes) — no host wait.  Called while tracked frames are still pending (``run``), it takes effect once they have finished."""
        assert self._n_enq >= 1, "call initialize() with the first frame"
        time_ns = [int(v) for v in time_ns] if isinstance(time_ns, (list, tuple)) else int(time_ns)
        if self._has_pending():
            self._skip_queue.append((self._n_enq - 1, time_ns))
            return
        self._skip_now(time_ns)

    def _skip_now(self, time_ns) -> None:
        L, lib = ops.L, self._lib
        L.check(lib.mv_frame_pipe_skip(self._pipe), "mv_frame_pipe_skip")
        mps = getattr(self, "_maps", None)
        if mps is not None:   # one need_interp row per lane, each at its own prior: one launch (mv_frame_pipe_map_skip_lanes)
            t = time_ns if isinstance(time_ns, list) else [time_ns] * self.lanes
            if len(t) != self.lanes:
                raise L.MacvoHipError(f"skip: {len(t)} timestamps for {self.lanes} lane(s)")
            mps.grow(0, drain=self.synchronize)
            L.check(lib.mv_frame_pipe_map_skip_lanes(self._pipe, mps.stores_dev(), mps[0].n_frames, self._map_K.data_ptr(), self._map_TBS.data_ptr(),
                                                     float(self.cam.baseline), (ops.C.c_int64 * self.lanes)(*t)), "mv_frame_pipe_map_skip_lanes")
            for m in mps:
                m.n_frames += 1

    def _keyframes_of(self, frames):
        """:meth:`HotPath._keyframes_of`: the keyframes of ``frames``; the frames in between are skipped as they are passed."""
        k = self.cfg.keyframe_freq
        if k == 1:
            yield from frames
            return
        for x in frames:
            self._frame_index += 1
            if self._frame_index % k == 0:
                yield x
            else:
                self.skip(x.time_ns if x.lane_time_ns is None else list(x.lane_time_ns))

    @traced("Frontend.estimate")
    def enqueue_frontend(self, x: FrameInputs):
        assert self._n_enq >= 1, "call initialize() with the first frame"
        self._enqueue(x, True)
        self._kps.append((x.keypoints, x.keypoint_counts))
        if self.cfg.motion_model == "tartan":
            self._motion()
        if self.cfg.mapping:
            self._images.append(self._prev_image)
            self._prev_image = x.image
        if getattr(self, "_maps", None) is not None:
            self._times.append(self._lane_times(x))
        return x

    def _motion(self) -> None:
        """TartanMotionNet of the frame just enqueued: the PoseNet on its input (MV_FB_MOTION_IN, written behind the frame's epilogue) on the
        current stream, its raw output attached to the frame's finish (mv_frame_pipe_set_motion) — between enqueue and finish, as run_pair does."""
        if self.pose_net is None:
            raise ops.L.MacvoHipError("motion_model='tartan' needs a pose_net ([lanes,5,112,160] -> [lanes,6])")
        lib, st = self._lib, ops._stream()
        ops.L.check(lib.mv_frame_pipe_wait_motion_input(self._pipe, st), "mv_frame_pipe_wait_motion_input")
        x = self._view("MOTION_IN", 0, torch.float32, (self.lanes,) + ops.MOTION_IN_SHAPE)
        raw = self.pose_net(x).reshape(self.lanes, 6).to(torch.float32).contiguous()
        ops.L.check(lib.mv_frame_pipe_set_motion(self._pipe, raw.data_ptr(), st), "mv_frame_pipe_set_motion")

    def enqueue_volume(self, x: FrameInputs) -> None:
        """Issue only the cost-volume GEMM of the frame the NEXT :meth:`enqueue_frontend` call will complete (same ``x``).
        The GEMM needs nothing but the feature maps and a free volume buffer, so it can be queued a frame ahead — before the
        host blocks on the previous frame's candidate count — and the GEMM stream never waits for the host."""
        if x.ready is not None:
            torch.cuda.current_stream().wait_event(x.ready)
        ops.L.check(self._lib.mv_frame_pipe_enqueue_volume(self._pipe, ops.C.byref(self._inputs(x)), ops._stream()),
                    "mv_frame_pipe_enqueue_volume")

    @traced("Odom_Runtime")
    def finish(self, pend=None, pose_sink: torch.Tensor | None = None):
        """Host half of a frame: wait for the candidate counts, draw the permutations (CPU generators, lane order), enqueue
        the pose-dependent kernels.  Returns a :class:`_NativeResult` (a list of them, one per lane, for lanes > 1)."""
        L, lib = ops.L, self._lib
        sink = None if pose_sink is None else pose_sink.data_ptr()
        kp, kp_counts = self._kps[0] if self._kps else (None, None)     # (taken off the list by _finished: a finish that raises leaves the frame pending)
        sel = self.cfg.selector
        if kp is not None or sel == "explicit":
            return self._finish_keypoints(kp, kp_counts, sink)
        if sel == "grid":   # nothing to draw and nothing to wait for: the front launch computes the rows
            L.check(lib.mv_frame_pipe_release(self._pipe, ops._stream()), "mv_frame_pipe_release")
            L.check(lib.mv_frame_pipe_finish_device(self._pipe, sink), "mv_frame_pipe_finish_device")
            for l in range(self.lanes):
                self._nsel[l] = self._ncand[l] = self._frame_rows
            return self._finished(host_counts=True)
        if sel == "random" and not self._native_seeds:
            # torch generators: torch.randint per lane, in lane order, exactly as the reference (KeypointSelector.py:103-118) -> explicit rows
            c, cam = self.cfg, self.cam
            for l in range(self.lanes):
                self._kp[l, : c.num_point] = _randint_rows(c.num_point, cam.H, cam.W, c.kp_mask_width, self.generators[l])
            return self._finish_keypoints(self._kp, [c.num_point] * self.lanes, sink, checked=True)
        if self.device_driven:
            L.check(lib.mv_frame_pipe_release(self._pipe, ops._stream()), "mv_frame_pipe_release")
            L.check(lib.mv_frame_pipe_finish_device(self._pipe, None if pose_sink is None else pose_sink.data_ptr()), "mv_frame_pipe_finish_device")
            return self._finished()
        if self._native_seeds:
            L.check(lib.mv_frame_pipe_release(self._pipe, ops._stream()), "mv_frame_pipe_release")
            L.check(lib.mv_frame_pipe_finish_seeded(self._pipe, None if pose_sink is None else pose_sink.data_ptr(), self._ncand, self._nsel),
                    "mv_frame_pipe_finish_seeded")
            return self._finished()
        L.check(lib.mv_frame_pipe_wait_candidates(self._pipe, self._ncand), "mv_frame_pipe_wait_candidates")
        num = self.cfg.num_point
        if self.lanes == 1:
            n = self._ncand[0]
            g = self.generators[0]
            # global CPU generator by default, exactly as the reference (KeypointSelector.py:331,404)
            perm = (torch.randperm(n) if g is None else torch.randperm(n, generator=g))[:num]
            self._nsel[0] = perm.numel()
            perm_ptr = perm.data_ptr() if perm.numel() else None
        else:
            for l in range(self.lanes):
                n = self._ncand[l]
                g = self.generators[l]
                perm = (torch.randperm(n) if g is None else torch.randperm(n, generator=g))[:num]
                k = perm.numel()
                self._nsel[l] = k
                if k:
                    self._perm[l, :k] = perm
            perm_ptr = self._perm.data_ptr()
        # views of earlier results may still be being read on the caller's stream: the pipe recycles their buffers behind that
        L.check(lib.mv_frame_pipe_release(self._pipe, ops._stream()), "mv_frame_pipe_release")
        L.check(lib.mv_frame_pipe_finish(self._pipe, perm_ptr, self._nsel, None if pose_sink is None else pose_sink.data_ptr()),
                "mv_frame_pipe_finish")
        return self._finished()

    def _finish_keypoints(self, kp, counts, sink, checked: bool = False):
        """Finish the oldest pending frame with caller-supplied (or host-drawn) keypoint rows: mv_frame_pipe_finish_keypoints for host tensors,
        mv_frame_pipe_finish_keypoints_dev — which never waits for the host — for device tensors."""
        L, lib, C = ops.L, self._lib, ops.C
        if kp is None:
            raise ValueError("selector 'explicit': the frame carries no keypoints (FrameInputs.keypoints / step(..., keypoints=))")
        kp = kp.reshape(self.lanes, -1, 2)
        n = kp.shape[1]
        if isinstance(counts, torch.Tensor) and counts.is_cuda:
            return self._finish_keypoints_dev_counts(kp, counts, sink)
        counts = [n] * self.lanes if counts is None else [int(k) for k in counts]
        if len(counts) != self.lanes or any(k < 0 or k > n for k in counts) or max(counts) > self._cap:
            raise ValueError(f"keypoints: {counts} live rows of {n} given, table capacity {self._cap}")
        for l in range(self.lanes):
            self._nsel[l] = self._ncand[l] = counts[l]
        L.check(lib.mv_frame_pipe_release(self._pipe, ops._stream()), "mv_frame_pipe_release")
        if kp.is_cuda:
            if self.cfg.mapping:
                raise L.MacvoHipError("device keypoints do not combine with mapping=True (the mapping decision needs the host anyway): pass a host tensor")
            tab = torch.zeros((self.lanes, self._cap, 2), dtype=torch.int64, device=self.dev)
            tab[:, :n] = kp.to(torch.int64)
            cnt = torch.tensor(counts, dtype=torch.int32).to(self.dev, non_blocking=True)
            self._kp_keep = self._kp_keep[-6:] + [(tab, cnt)]     # alive until the pipe has read them (two more finishes at most)
            L.check(lib.mv_frame_pipe_finish_keypoints_dev(self._pipe, tab.data_ptr(), cnt.data_ptr(), ops._stream(), sink),
                    "mv_frame_pipe_finish_keypoints_dev")
        else:
            if kp is not self._kp:
                live = [kp[l, : counts[l]] for l in range(self.lanes)]
                if not checked:
                    for r in live:
                        check_keypoints(r, self.cfg, self.cam)
                for l, r in enumerate(live):
                    self._kp[l, : counts[l]] = r
            L.check(lib.mv_frame_pipe_finish_keypoints(self._pipe, self._kp.data_ptr(), self._nsel, sink), "mv_frame_pipe_finish_keypoints")
        return self._finished(host_counts=True)

    def _finish_keypoints_dev_counts(self, kp, counts, sink):
        """Device rows with device counts (``image_selector``): both go to mv_frame_pipe_finish_keypoints_dev as they are — the pipe clamps each count to
        the table capacity — and the frame's counts come back lazily (mv_frame_pipe_finished_counts) for whoever reads ``n_sel``."""
        L, lib = ops.L, self._lib
        n = kp.shape[1]
        if not kp.is_cuda or counts.dtype != torch.int32 or counts.shape != (self.lanes,) or n > self._cap:
            raise ValueError(f"keypoints with device counts: need device int64 rows [{self.lanes}, n <= {self._cap}, 2] and int32 counts [{self.lanes}]")
        if self.cfg.mapping:
            raise L.MacvoHipError("device keypoints do not combine with mapping=True (the mapping decision needs the host anyway): pass a host tensor")
        L.check(lib.mv_frame_pipe_release(self._pipe, ops._stream()), "mv_frame_pipe_release")
        if n == self._cap and kp.dtype == torch.int64 and kp.is_contiguous():
            tab = kp
        else:
            tab = torch.zeros((self.lanes, self._cap, 2), dtype=torch.int64, device=self.dev)
            tab[:, :n] = kp.to(torch.int64)
        cnt = counts.contiguous() if n == self._cap else counts.clamp(max=n)     # (rows behind n do not exist; on the device)
        self._kp_keep = self._kp_keep[-6:] + [(tab, cnt)]     # alive until the pipe has read them (two more finishes at most)
        L.check(lib.mv_frame_pipe_finish_keypoints_dev(self._pipe, tab.data_ptr(), cnt.data_ptr(), ops._stream(), sink),
                "mv_frame_pipe_finish_keypoints_dev")
        return self._finished(lazy_counts=True)

    def _map_tail(self, mps):
        """Dense-mapping tail of the frame just finished (Odometry/MACVO.py:303-337): the reference maps only when tracking
        succeeded — so the frame's observation count has to reach the host first (one blocking wait per frame: mapping mode gives
        up the driver's run-ahead, as the reference's own `.cpu()` calls do) — and then draws its SECOND randperm of the frame from
        the same CPU generator."""
        L, lib, c = ops.L, self._lib, self.cfg
        image0 = self._images.pop(0)
        nv, nm = ops.C.c_int32(0), ops.C.c_int32(0)
        L.check(lib.mv_frame_pipe_wait_tracked(self._pipe, ops.C.byref(nv), ops.C.byref(nm)), "mv_frame_pipe_wait_tracked")
        if nv.value < c.min_num_point:
            return None
        g = self.generators[0]
        perm = (torch.randperm(nm.value) if g is None else torch.randperm(nm.value, generator=g))[: c.map_num_point]
        n = perm.numel()
        img = None if image0 is None else ops._req(image0.reshape(3, self.cam.H, self.cam.W), torch.float32, "image")
        if mps is not None:   # (growth re-allocates the store member 0's host descriptor names, and stales the holder's device array with it)
            mps.grow(new_map_points=n, drain=self.synchronize)
            mps[0].map_rows_upper += n
        L.check(lib.mv_frame_pipe_map_points(self._pipe, perm.data_ptr() if n else None, n, None if img is None else img.data_ptr(),
                                             None if mps is None else ops.C.byref(mps[0].stores())), "mv_frame_pipe_map_points")
        self._map_keep = img
        f32 = torch.float32
        v = lambda name, dt, tail: self._view(name, 0, dt, (n,) + tail)  # noqa: E731
        return ops.MapPoints(v("MAP_UV", f32, (2,)), v("MAP_D", f32, ()), v("MAP_SDD", f32, ()), v("MAP_TC", f32, (3,)), v("MAP_TW", f32, (3,)),
                             v("MAP_COV", torch.float64, (3, 3)), None if img is None else v("MAP_COLOR", torch.uint8, (3,)))

    def _finished(self, host_counts: bool = False, lazy_counts: bool = False):
        """Bookkeeping behind a finish call: map registration, result views.  host_counts: the frame's row counts are known on the host
        (self._nsel / self._ncand) although the pipe is device-driven; lazy_counts: they exist on the device only although it is not."""
        L, lib = ops.L, self._lib
        self._n_fin += 1
        if self._kps:
            self._kps.pop(0)
        dd = (self.device_driven and not host_counts) or lazy_counts
        mps = getattr(self, "_maps", None)
        if mps is not None:   # every lane into its own map: one launch for all lanes, then the optimised poses by one more (mv_frame_pipe_map_append_lanes)
            n_rows = [self._cap if dd else int(self._nsel[l]) for l in range(self.lanes)]   # (device-driven: an upper bound; the append compacts by the `valid` mask)
            mps.grow(n_rows, drain=self.synchronize)
            L.check(lib.mv_frame_pipe_map_append_lanes(self._pipe, mps.stores_dev(), mps[0].n_frames, mps[0].last_keyframe, self._map_K.data_ptr(),
                                                       self._map_TBS.data_ptr(), float(self.cam.baseline), self._times.pop(0)),
                    "mv_frame_pipe_map_append_lanes")
            for m, n in zip(mps, n_rows):
                m.last_keyframe = m.n_frames
                m.n_frames += 1
                m.rows_upper += n
        map_pts = self._map_tail(mps) if self.cfg.mapping else None
        out = []
        for l in range(self.lanes):
            res = _NativeResult(self, l, None if dd else self._nsel[l], None if dd else self._ncand[l])
            res.map_points = map_pts
            if self.keep_extras and not dd:
                res.extras   # noqa: B018  (host-driven frames: build the views now, as before)
            out.append(res)
        while self._skip_queue and self._skip_queue[0][0] <= self._n_fin:
            self._skip_now(self._skip_queue.pop(0)[1])
        return out[0] if self.lanes == 1 else out

    def _extras_of(self, res: "_NativeResult") -> dict:
        n_sel, l = res.n_sel, res.lane
        if not n_sel:
            return {}
        f32, f64 = torch.float32, torch.float64
        vals = self._view("VALS", res._age(), f32, (11, self.lanes, self._cap))[:, l, :n_sel]
        tr = ops.TrackedKeypoints(res._rows("KP0F", f32, (2,)), res._rows("KP1", f32, (2,)),
                                  res._rows("INBOUND", torch.bool), vals,
                                  res._rows("SIGMA0", f32, (3,)), res._rows("SIGMA1", f32, (3,)))
        return dict(tracked=tr, cov0=res._rows("COV0", f64, (3, 3)), cov0_w=res._rows("COV0W", f64, (3, 3)),
                    cov1=res._rows("COV1", f64, (3, 3)), valid=res._rows("VALID", torch.bool),
                    pos_Tw=res._rows("POS_TW", f32, (3,)), n_cand=res.n_cand)

    def _finished_counts(self, fin: int, age: int, lane: int):
        """(n_cand, n_sel) of lane ``lane`` of the frame that was finish number ``fin`` (device-driven frames; blocking read-back)."""
        got = self._counts_cache.get(fin)
        if got is None:
            nc, ns = (ops.C.c_int32 * self.lanes)(), (ops.C.c_int32 * self.lanes)()
            ops.L.check(self._lib.mv_frame_pipe_finished_counts(self._pipe, age, nc, ns), "mv_frame_pipe_finished_counts")
            got = (list(nc), list(ns))
            if len(self._counts_cache) > 64:
                self._counts_cache.clear()
            self._counts_cache[fin] = got
        return got[0][lane], got[1][lane]

    def step(self, x: FrameInputs, keypoints: torch.Tensor | None = None):
        """One ``run_pair`` start to finish (no cross-frame overlap); results are valid on the current stream.  ``keypoints``: this frame's
        keypoints (see :class:`FrameInputs`), instead of ``x.keypoints``."""
        if keypoints is not None:
            x = replace(x, keypoints=keypoints, keypoint_counts=None)
        self.enqueue_frontend(x)
        res = self.finish()
        self.sync_all()
        return res

    def sync_pose(self) -> None:
        """Make the current stream wait for the newest FINISHED frame's backend and solve (its results: keypoints, covariances,
        pose) — not for the frontends of the frames :meth:`run` has already queued behind it.  Read a result right after this
        call: its buffers are recycled two finishes later."""
        if self._pipe is not None:
            ops.L.check(self._lib.mv_frame_pipe_sync(self._pipe, ops._stream(), 2), "mv_frame_pipe_sync")

    def sync_all(self) -> None:
        """Make the current stream wait for everything the pipe has enqueued (frontends of queued frames included)."""
        if self._pipe is not None:
            ops.L.check(self._lib.mv_frame_pipe_sync(self._pipe, ops._stream(), 0), "mv_frame_pipe_sync")

    def time_volume(self, max_launches: int) -> None:
        """Record a HIP-event pair around each of the next ``max_launches`` volume GEMMs (on the stream they run on)."""
        ops.L.check(self._lib.mv_frame_pipe_time_volume(self._pipe, int(max_launches)), "mv_frame_pipe_time_volume")

    def time_detail(self, on: bool) -> None:
        """``False``: timed frames record only the event pair around their GEMM (no timeline events on the other streams)."""
        ops.L.check(self._lib.mv_frame_pipe_time_detail(self._pipe, int(bool(on))), "mv_frame_pipe_time_detail")

    def volume_times_ms(self) -> list:
        cap = self._pc_timed = 1 << 16
        buf = (ops.C.c_float * cap)()
        n = ops.C.c_int(0)
        ops.L.check(self._lib.mv_frame_pipe_volume_times(self._pipe, buf, cap, ops.C.byref(n)), "mv_frame_pipe_volume_times")
        return list(buf[: n.value])

    def volume_starts_ms(self) -> list:
        """Start of each timed GEMM, ms since the first timed one."""
        cap = 1 << 16
        buf = (ops.C.c_float * cap)()
        n = ops.C.c_int(0)
        ops.L.check(self._lib.mv_frame_pipe_volume_starts(self._pipe, buf, cap, ops.C.byref(n)), "mv_frame_pipe_volume_starts")
        return list(buf[: n.value])

    def timeline_ms(self) -> list:
        """[(GEMM start, GEMM end, last lookup done, selector done)] per timed frame, ms since the first timed GEMM start."""
        cap = 1 << 14
        buf = (ops.C.c_float * (4 * cap))()
        n = ops.C.c_int(0)
        ops.L.check(self._lib.mv_frame_pipe_timeline(self._pipe, buf, cap, ops.C.byref(n)), "mv_frame_pipe_timeline")
        return [tuple(buf[4 * i: 4 * i + 4]) for i in range(n.value)]

    def timeline_backend_ms(self) -> list:
        """[(backend start, backend end, pose_apply start, solve end)] per timed frame, same time base as :meth:`timeline_ms`."""
        cap = 1 << 14
        buf = (ops.C.c_float * (4 * cap))()
        n = ops.C.c_int(0)
        ops.L.check(self._lib.mv_frame_pipe_timeline_backend(self._pipe, buf, cap, ops.C.byref(n)), "mv_frame_pipe_timeline_backend")
        return [tuple(buf[4 * i: 4 * i + 4]) for i in range(n.value)]

    def synchronize(self) -> None:
        if self._pipe is not None:
            ops.L.check(self._lib.mv_frame_pipe_sync(self._pipe, None, 1), "mv_frame_pipe_sync")

    def run(self, frames, pose_sink: torch.Tensor | None = None, depth: int | None = None):
        """Software-pipelined stream: up to ``depth`` (default 3 = the pipe's slot rotation) tracked frames are enqueued ahead
        of the frame whose candidate count the host waits for, plus the volume GEMM of the one after — the GPU-side chain
        volume -> 12 lookups -> selector of a frame takes ~2.5 frame periods when it shares the chip with the next GEMMs, so
        the host has to run that far ahead for the GEMM stream to stay busy.  ``pose_sink``: ``[steps, 7]``
        (``[steps, lanes, 7]`` for lanes > 1) device tensor receiving each step's poses."""
        depth = self._depth if depth is None else depth
        it = iter(frames) if self.cfg.keyframe_freq == 1 else self._keyframes_of(frames)
        nxt = next(it, None)
        if self._pipe is not None and (self.device_driven or self._hostless):
            # Device-driven frames: nothing in a frame waits for the host, so a frame is enqueued and finished in one go (the next frame's GEMM in between, as
            # in the host-driven order); how far the host runs ahead of the GPU is bounded by the HIP queues, the slot rotation is guarded by events.
            i = 0
            # ... and by `lag`: the host stays at most that many finished frames ahead of the GPU's front launches (flow control on an event two frames old, not a
            # wait on the critical chain).  Measured at 640x480 (profiles/r06_device_draw_ab.log): lag 0 / 1 / 2 / 3 / 4 / 6 / unbounded = 4.13 / 6.01 / 6.51 / 6.46 / 6.34 /
            # 6.24 / 4.07 k frames/s — with hundreds of frames queued the same kernels take 1.6x as long (deep queues of cross-queue barriers), so the default is 2.
            # (Also measured and dropped: flow control on the SELECTOR's event instead of the front launch's — 30 us earlier, i.e. deeper: 5.0 k instead of 5.4 k on
            # the 20-step line — and the host-drawn frame's order, a frame finished only once its selector is done: 5.0 k / 5.9-6.4 k at 300 steps.)
            lag = min(int(os.environ.get("MV_PIPE_DD_AHEAD", "2")), 6)      # (the driver keeps a ring of 8 front-launch events)
            clock = time.perf_counter
            while nxt is not None:
                t0 = clock()
                self.enqueue_frontend(nxt)
                nxt = next(it, None)
                if self._volume_ahead and nxt is not None:
                    self.enqueue_volume(nxt)
                res = self.finish(None, None if pose_sink is None else pose_sink[i])
                t1 = clock()
                i += 1
                if lag >= 0:
                    ops.L.check(self._lib.mv_frame_pipe_wait_finished(self._pipe, lag), "mv_frame_pipe_wait_finished")
                # host accounting (bench.py `host_us_per_frame`): time spent issuing a frame vs time spent in the flow-control wait (= ahead of the GPU)
                self.host_issue_s += t1 - t0
                self.host_wait_s += clock() - t1
                self.host_frames += 1
                yield res
            self.sync_all()
            return
        state = {"nxt": nxt, "vol": False, "pending": 0}

        def pump():
            while state["nxt"] is not None and state["pending"] < depth:
                self.enqueue_frontend(state["nxt"])       # completes the frame (its GEMM may already be queued)
                state["pending"] += 1
                state["nxt"], state["vol"] = next(it, None), False
            if self._volume_ahead and state["nxt"] is not None and not state["vol"]:
                self.enqueue_volume(state["nxt"])
                state["vol"] = True

        pump()
        i = 0
        while state["pending"]:
            res = self.finish(None, None if pose_sink is None else pose_sink[i])
            state["pending"] -= 1
            i += 1
            pump()                                        # refill before handing the result out: the GPU stays fed
            yield res
        self.sync_all()

    def _has_pending(self) -> bool:
        return self._n_fin < self._n_enq - 1          # frame 0 (initialize) is never finished
