"""TEST INFRASTRUCTURE: ``Local_TwoFrame_PGO`` restated in torch around ``oracle.pgo.solve``.

The two frame changes of Module/Optimization/TwoFramePGO/Optimizer.py:131-150 in the reference's precisions and order, on the PyPose restatement of
``oracle.se3`` (dtype-generic: the fp32 stages run in fp32 with one rounding per torch op, as PyPose's own ops do):

    world_to_optim   T_c2o = T_w2o @ T_c2w (fp32); pos_To = Act(T_w2o, pos_Tw) (fp32); cov_To = R_w2o @ cov_Tw @ R_w2o^T (fp64, R_w2o the fp32
                     rotation matrix widened)
    optim_to_world   NormalizeQuat(T_o2w @ float(T_c2o'))  (fp32; Utility/Math.py:124-133)
"""
from __future__ import annotations

import copy
from types import SimpleNamespace

import torch

from oracle import pgo, se3


def cross_is_fused() -> bool:
    """Whether this host's ``torch.linalg.cross`` evaluates an fp32 component as ``fmsub(a1, b2, a2 * b1)`` — ATen's FMA-capable vector dispatch, which the
    goldens were generated with and ``csrc/pgo_local_dev.h`` spells out as ``fmaf``.  On a torch build that rounds both products, the fp32 stages of this
    restatement (not of the twin or the kernel) are off the golden by an ulp or two."""
    a = torch.tensor([0.0, 1.0 + 2.0 ** -12, 1.0 + 2.0 ** -12])
    b = torch.tensor([0.0, 1.0 - 2.0 ** -12, 1.0 + 2.0 ** -12])      # x = a1 b2 - a2 b1 = (1 + e)^2 - (1 + e)(1 - e) = 2 e + 2 e^2: the 2 e^2 survives the fused form only
    x = float(torch.linalg.cross(a, b)[0])
    return x == 2.0 ** -11 + 2.0 ** -23


def rotation_matrix(q: torch.Tensor) -> torch.Tensor:
    """``LieTensor.rotation().matrix()``: the columns are SO3_Act(q, e_i), in q's dtype."""
    I = torch.eye(3, dtype=q.dtype)
    return se3.quat_act(q.unsqueeze(-2), I).transpose(-1, -2)


def normalize_quat(T: torch.Tensor) -> torch.Tensor:
    out = T.clone()
    out[..., 3:] = out[..., 3:] / out[..., 3:].norm(dim=-1, keepdim=True)
    return out


def world_to_optim(prob: pgo.PGOProblem, ref_pose: torch.Tensor) -> pgo.PGOProblem:
    """The problem moved into the frame of ``ref_pose`` (T_o2w, [7] fp32); Optimizer.py:119-123,131-143."""
    T_w2o = se3.se3_inv(ref_pose.float())
    out = copy.copy(prob)
    out.init_pose = se3.se3_mul(T_w2o, prob.init_pose.float())
    R = rotation_matrix(T_w2o[3:]).to(prob.cov_Tw)
    out.pos_Tw = se3.se3_act(T_w2o.to(prob.pos_Tw), prob.pos_Tw)
    out.cov_Tw = R @ prob.cov_Tw @ R.transpose(-1, -2)
    return out


def optim_to_world(pose_local: torch.Tensor, ref_pose: torch.Tensor) -> torch.Tensor:
    """fp64 local-frame result -> fp32 world pose; Optimizer.py:145-150."""
    return normalize_quat(se3.se3_mul(ref_pose.float(), pose_local.to(torch.float32)))


def solve(prob: pgo.PGOProblem, ref_pose: torch.Tensor, graph_type="disp", params=None, min_points: int = 0):
    """``get_graph_data`` -> ``_optimize`` -> ``write_graph_data`` of Local_TwoFrame_PGO for one problem: a namespace with the moved problem
    (``local``), the oracle's result in the local frame (``res``) and the fp32 world pose (``pose_f32``).  Fewer than ``min_points`` rows: no solve,
    the start pose stays (Odometry/MACVO.py:303-307)."""
    local = world_to_optim(prob, ref_pose)
    if prob.pos_Tw.shape[0] < min_points:
        return SimpleNamespace(local=local, res=None, pose_f32=prob.init_pose.float().clone())
    res = pgo.solve(local, graph_type, params)
    return SimpleNamespace(local=local, res=res, pose_f32=optim_to_world(res.pose, ref_pose))


def move_problem(prob: pgo.PGOProblem, move: torch.Tensor) -> pgo.PGOProblem:
    """The same problem seen from a world frame moved rigidly by ``move`` ([7] fp32): poses, points and point covariances."""
    out = copy.copy(prob)
    m = move.float()
    out.init_pose = se3.se3_mul(m, prob.init_pose.float())
    out.pos_Tw = se3.se3_act(m, prob.pos_Tw.float())
    R = rotation_matrix(m[3:]).double()
    out.cov_Tw = R @ prob.cov_Tw @ R.transpose(-1, -2)
    return out
