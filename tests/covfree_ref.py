"""Torch restatement of ``MACVO.run_pair`` (Odometry/MACVO.py:173-311) for a frontend that lacks covariances — ``provide_cov`` (d, m) with
d = the depth model gives a covariance, m = the matcher does — chained from the ``oracle/`` pieces (TEST INFRASTRUCTURE, CPU tensors).
Pinned against the reference's own loop by tests/golden/covfree.npz (tests/test_covfree_host.py); used where the reference tree is absent.

What changes without a covariance (the contract of DESIGN.md, "Covariance-free frontends"):
  * no d: ``depth.cov`` / ``depth.disparity_uncertainty`` are None -> ``pixel*_d_cov`` / ``pixel*_disp_cov`` are stored as -1;
  * no m: ``match.cov`` is None -> ``pixel2_uv_cov`` is stored as (-1, -1, -1) and the second observation's covariance is the model with
    ``flow_cov=None``: sigma (c, c, 0), c = the MODEL's ``match_cov_default``, unclamped, depth variance = ``depth.cov`` at kp1 when d holds
    (then clamped by ``min_depth_cov``), the patch variance when it does not.
"""
from __future__ import annotations

import torch

from oracle import covariance, filters, frontend, pgo, se3
from oracle.pipeline import rotation_matrix_f32
from tests import selectors_ref as SR

FILTER_COV_SANITY, FILTER_SIMPLE_DEPTH, FILTER_FRONT_OF_CAM = 1, 2, 4


def frontend_maps(flow: torch.Tensor, cov: "torch.Tensor | None", bl: float, fx: float, d: bool, m: bool) -> dict:
    """FlowFormer[Cov]Depth.estimate + FlowFormer[Cov]Matcher.forward behind the network: ``flow`` [2,2,H,W] (sample 0 = stereo pair, sample 1 =
    temporal pair), ``cov`` = exp(2 * log sigma) of the same shape (None when neither side provides one)."""
    disp = flow[0:1, 0:1].abs()
    out = dict(depth=frontend.disparity_to_depth(disp, bl, fx), disparity=disp, cov=None, disparity_uncertainty=None, flow=flow[1:2], flow_cov=None)
    if d:
        out["disparity_uncertainty"] = cov[0:1, 0:1]
        out["cov"] = frontend.disparity_to_depth_cov(disp, cov[0:1, 0:1], bl, fx)
    if m:
        out["flow_cov"] = frontend.from_partial_cov(cov[1:2])
    return out


def _gather(kp, mp):
    return None if mp is None else frontend.retrieve_pixels(kp, mp)


class CovFreeRef:
    """cfg keys: frontend_cov (d, m); selector "random" | "grid" | "explicit"; cov_model "match" | "none"; cov_match_cov_default (the model's);
    match_cov_default (Odometry's); filters (flag mask); graph_type; num_point, edgewidth, kp_mask_width, cov_kernel_size, min_flow_cov,
    min_depth_cov, filter_min_depth, min_num_point."""

    def __init__(self, cam: dict, cfg: dict, generator: "torch.Generator | None" = None):
        self.cam = cam
        c = dict(frontend_cov=(False, False), selector="random", cov_model="none", cov_match_cov_default=0.25, match_cov_default=0.25,
                 filters=FILTER_SIMPLE_DEPTH, graph_type="icp", num_point=200, edgewidth=32, kp_mask_width=32, cov_kernel_size=31,
                 min_flow_cov=0.25, min_depth_cov=0.05, filter_min_depth=0.05, min_num_point=10)
        c.update(cfg)
        self.cfg = c
        self.gen = generator
        self.pose = torch.tensor([0, 0, 0, 0, 0, 0, 1], dtype=torch.float32)
        self.maps_prev = None

    def _maps(self, x: dict) -> dict:
        d, m = self.cfg["frontend_cov"]
        return frontend_maps(x["flow"], x.get("cov_exp"), self.cam["baseline"], self.cam["fx"], bool(d), bool(m))

    def initialize(self, x: dict, init_pose=None):
        self.maps_prev = self._maps(x)
        if init_pose is not None:
            self.pose = init_pose.float().reshape(7).clone()

    def _obs_cov(self, kp, maps, depth_cov, flow_cov):
        c, cam = self.cfg, self.cam
        if c["cov_model"] == "none":
            return torch.eye(3).unsqueeze(0).repeat(kp.size(0), 1, 1).double()
        return covariance.match_covariance(kp, maps["depth"], depth_cov, flow_cov, cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                                           kernel_size=c["cov_kernel_size"], match_cov_default=c["cov_match_cov_default"],
                                           min_flow_cov=c["min_flow_cov"], min_depth_cov=c["min_depth_cov"])

    def step(self, x: dict, keypoints: "torch.Tensor | None" = None) -> dict:
        c, cam = self.cfg, self.cam
        H, W = cam["H"], cam["W"]
        Km = torch.tensor([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1]], dtype=torch.float32)
        maps0, maps1 = self.maps_prev, self._maps(x)
        if keypoints is not None:
            kp_all = keypoints
        elif c["selector"] == "random":
            kp_all = SR.random_select(c["num_point"], H, W, c["kp_mask_width"], self.gen)
        else:
            kp_all = SR.grid_select(c["num_point"], H, W, c["kp_mask_width"])
        kp1_all = kp_all + frontend.retrieve_pixels(kp_all, maps1["flow"]).T
        inb = frontend.filterPointsInRange(kp1_all, (c["edgewidth"], W - c["edgewidth"]), (c["edgewidth"], H - c["edgewidth"]))
        kp0, kp1 = kp_all[inb], kp1_all[inb]
        n = kp0.size(0)
        kp0_d, kp1_d = frontend.retrieve_pixels(kp0, maps0["depth"]).squeeze(0), frontend.retrieve_pixels(kp1, maps1["depth"]).squeeze(0)
        g = {}
        for tag, kp, mp in (("1", kp0, maps0), ("2", kp1, maps1)):
            g[f"pixel{tag}_disp"] = frontend.retrieve_pixels(kp, mp["disparity"]).T
            su, sd = _gather(kp, mp["disparity_uncertainty"]), _gather(kp, mp["cov"])
            g[f"pixel{tag}_disp_cov"] = torch.full((n, 1), -1.0) if su is None else su.T
            g[f"sdd{tag}"] = None if sd is None else sd.squeeze(0)
            g[f"pixel{tag}_d_cov"] = torch.full((n, 1), -1.0) if sd is None else sd.squeeze(0).unsqueeze(-1)
        s0 = torch.ones((n, 3)) * c["match_cov_default"]
        s0[..., 2] = 0.0
        s1 = _gather(kp0, maps1["flow_cov"])
        s1 = None if s1 is None else s1.T.contiguous()
        pos0_Tc = frontend.pixel2point_NED(kp0, kp0_d, Km)
        cov0 = self._obs_cov(kp0, maps0, g["sdd1"], s0)
        cov1 = self._obs_cov(kp1, maps1, g["sdd2"], s1)            # (clamps s1 in place when it is there, like the reference)
        g["pixel1_uv_cov"] = s0
        g["pixel2_uv_cov"] = torch.full((n, 3), -1.0) if s1 is None else s1
        mask = torch.ones(n, dtype=torch.bool)
        if c["filters"] & FILTER_COV_SANITY:
            mask &= filters.covariance_sanity(cov0, cov1)
        if c["filters"] & FILTER_SIMPLE_DEPTH:
            mask &= filters.simple_depth(kp0_d.unsqueeze(-1), kp1_d.unsqueeze(-1), c["filter_min_depth"], cam["fx"] * cam["baseline"])
        if c["filters"] & FILTER_FRONT_OF_CAM:
            mask &= filters.likely_front_of_cam(kp0_d.unsqueeze(-1), g["pixel1_d_cov"], kp1_d.unsqueeze(-1), g["pixel2_d_cov"])
        R = rotation_matrix_f32(self.pose)
        pos_Tw = se3.se3_act(self.pose, pos0_Tc)
        cov_Tw = covariance.rotate_covariance(R, cov0)
        nv = int(mask.sum())
        out = dict(kp_all=kp_all, inbound=inb, kp0=kp0, kp1=kp1, kp0_d=kp0_d, kp1_d=kp1_d, cov0=cov0, cov1=cov1, mask=mask, pos_Tw=pos_Tw,
                   cov_Tw=cov_Tw, n_valid=nv, stored=g, solved=nv >= c["min_num_point"])
        if out["solved"]:
            prob = pgo.PGOProblem(init_pose=self.pose.clone(), K=Km, baseline=cam["baseline"], pos_Tw=pos_Tw[mask], cov_Tw=cov_Tw[mask],
                                  pixel2_uv=kp1[mask], pixel2_d=kp1_d[mask].unsqueeze(-1), pixel2_disp=g["pixel2_disp"][mask],
                                  pixel2_disp_cov=g["pixel2_disp_cov"][mask], pixel2_uv_cov=g["pixel2_uv_cov"][mask], obs2_covTc=cov1[mask])
            res = pgo.solve(prob, c["graph_type"])
            self.pose = res.pose.float()
            out["pose_f64"] = res.pose
        out["pose"] = self.pose
        self.maps_prev = maps1
        return out
