"""CPU: what the covariance, solve and window-lookup entry points accept.  Every row of the table is either refused on the host before any HIP call or
returns ``MV_OK`` early on a zero count, so the expected code is the same with or without a GPU — but the module only runs without one: a row that an
entry point wrongly ACCEPTED would go on to launch a kernel on the dummy pointers below.  Without a GPU the same mistake is a failed launch
(``MV_ERR_LAUNCH``) and a failed assertion.  The codes pin each entry point's own conditions (which check comes first where two fail, "unsupported" against
"invalid"), which the one host path behind each family (``mv_obs_cov_launch``, ``mv_plain_solve`` / ``mv_posed_solve``, ``mv_lookup``) has to keep apart."""
import ctypes as C

import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("host-side argument table: its rows pass dummy pointers, and a wrongly accepted row would launch a kernel on them; it runs where no GPU is "
                "visible (there such a row fails as MV_ERR_LAUNCH)", allow_module_level=True)

from macvo_amd import _lib as L  # noqa: E402

OK, INVALID, UNSUPPORTED = L.MV_OK, -1, -2   # MV_ERR_INVALID_ARG, MV_ERR_UNSUPPORTED (include/macvo_hip.h)
P = 0x1000        # a non-null device pointer: nothing dereferences it on these paths
GMM, ICP = L.MV_COV_GMM, L.MV_GRAPH_ICP


def _i32(*v):     # host arrays (n_live) ARE read
    return (C.c_int32 * len(v))(*v)


def _cp(**kw):
    d = dict(H=48, W=64, kernel_size=5, use_patch_var=1, fx=80.0, fy=80.0, cx=32.0, cy=24.0, min_flow_cov_sq=0.0625, min_depth_cov=0.05)
    d.update(kw)
    return L.mvMatchCovParams(**d)


def _lm(**kw):
    p = L.mvLMParams()
    L.load().mv_lm_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# ---- argument names in header order; a row overrides the defaults below by name
_SET0 = ["depth_map0", "kp_uv0", "flow_cov0", "rot0", "out_cov0", "out_cov_rot0"]
_LANES = ["params", "lanes", "n_live", "cap", "stream"]
_SOLVE_TABLES = ["pixel2_uv", "pixel2_d", "pixel2_disp", "pixel2_disp_cov", "pixel2_uv_cov", "obs2_covTc"]
_PLAIN_TAIL = ["intrinsics", "baseline", "pos_Tw", "cov_Tw"] + _SOLVE_TABLES + ["valid", "min_points", "lm", "out_pose", "out_info", "out_pose_f32", "stream"]
_POSED_TAIL = ["intrinsics", "baseline", "pos_Tc", "cov_Tc", "pos_Tw", "cov_Tw", "out_rot"] + _SOLVE_TABLES + [
    "filter_flags", "filter_min_depth", "filter_max_depth", "inbound", "vals", "valid", "count_out", "min_points", "lm", "out_pose", "out_info",
    "out_pose_f32", "pose_sink", "stream"]
_HOST, _DEV = ["nprob", "offsets", "n_live", "cap", "graph_type"], ["nprob", "offsets", "n_live_dev", "n_live_stride", "cap", "graph_type"]
_LOOKUP = ["vol", "coords", "out", "B", "H1", "W1", "H2", "W2", "radius", "stream"]
NAMES = {
    "mv_match_cov": ["depth_map", "kp_uv", "flow_cov", "depth_cov", "rot", "params", "N", "out_cov", "out_cov_rot", "out_stats", "stream"],
    "mv_match_cov_pair": _SET0 + ["depth_map1", "kp_uv1", "flow_cov1", "out_cov1", "params", "N", "stream"],
    "mv_match_cov_pair_lanes": _SET0 + ["depth_map1", "kp_uv1", "flow_cov1", "out_cov1"] + _LANES,
    "mv_obs_cov": ["model", "modifiers", "depth_map", "depth_cov_map", "kp_uv", "flow_cov", "depth_cov", "rot", "params", "N", "out_cov", "out_cov_rot",
                   "out_stats", "stream"],
    "mv_obs_cov_pair_lanes": ["model", "modifiers", "depth_map0", "depth_cov_map0"] + _SET0[1:] + [
        "depth_map1", "depth_cov_map1", "kp_uv1", "flow_cov1", "out_cov1"] + _LANES,
    "mv_obs_cov_pair_nomatch_lanes": ["model", "modifiers", "depth_map0", "depth_cov_map0"] + _SET0[1:] + [
        "depth_map1", "depth_cov_map1", "kp_uv1", "depth_cov1", "model_match_cov_default", "out_cov1"] + _LANES,
    "mv_pgo_solve": ["nprob", "offsets", "graph_type", "init_pose"] + _PLAIN_TAIL,
    "mv_pgo_solve_local": ["nprob", "offsets", "graph_type", "init_pose", "ref_pose"] + _PLAIN_TAIL,
    "mv_pgo_solve_posed": _HOST + ["init_pose"] + _POSED_TAIL,
    "mv_pgo_solve_posed_dev": _DEV + ["init_pose"] + _POSED_TAIL,
    "mv_pgo_solve_posed_motion": _HOST + ["init_pose", "start_pose"] + _POSED_TAIL,
    "mv_pgo_solve_posed_motion_dev": _DEV + ["init_pose", "start_pose"] + _POSED_TAIL,
    "mv_pgo_solve_posed_local": _HOST + ["init_pose", "start_pose", "ref_pose"] + _POSED_TAIL,
    "mv_pgo_solve_posed_local_dev": _DEV + ["init_pose", "start_pose", "ref_pose"] + _POSED_TAIL,
    "mv_corr_lookup": _LOOKUP, "mv_corr_lookup_vol16": _LOOKUP, "mv_corr_lookup_tiled": _LOOKUP, "mv_corr_lookup_tiled_vol16": _LOOKUP,
}
# With nothing overridden every call is a valid one (it would launch): each row below breaks exactly what its comment names, or zeroes the count.
DEFAULTS = dict(
    stream=None, model=L.MV_COV_MATCH, modifiers=0, model_match_cov_default=0.25, N=4, lanes=2, n_live=_i32(3, 4), cap=4, params=_cp(),
    depth_cov=None, depth_cov1=None, depth_cov_map=None, depth_cov_map0=None, depth_cov_map1=None, rot=None, rot0=None, out_cov_rot=None,
    out_cov_rot0=None, out_stats=None,
    nprob=2, graph_type=L.MV_GRAPH_DISP, n_live_stride=1, filter_flags=7, filter_min_depth=0.1, filter_max_depth=80.0, min_points=0,
    B=2, H1=8, W1=8, H2=8, W2=8, radius=4)   # (every name not listed: the dummy pointer P)
Z = dict(n_live=_i32(0, 0))                  # no live row in any lane
NULLS0 = dict(depth_map0=None, kp_uv0=None, flow_cov0=None, out_cov0=None, depth_map1=None, kp_uv1=None, out_cov1=None)

TABLE = [
    # ---- mv_match_cov: the single form, N rows
    ("mv_match_cov", dict(N=0), OK),
    ("mv_match_cov", dict(N=0, depth_map=None, kp_uv=None, flow_cov=None, out_cov=None), OK),          # the zero count returns before the pointer checks
    ("mv_match_cov", dict(N=0, params=None), INVALID),                                                  # ... but behind params
    ("mv_match_cov", dict(N=-1), INVALID),
    ("mv_match_cov", dict(depth_map=None), INVALID),
    ("mv_match_cov", dict(out_cov=None), INVALID),
    ("mv_match_cov", dict(params=_cp(H=0)), INVALID),
    ("mv_match_cov", dict(params=_cp(kernel_size=4)), INVALID),                                         # even
    ("mv_match_cov", dict(params=_cp(kernel_size=0)), INVALID),
    ("mv_match_cov", dict(params=_cp(kernel_size=33)), UNSUPPORTED),                                    # oversized: unsupported, not invalid
    ("mv_match_cov", dict(params=_cp(use_patch_var=0)), INVALID),                                       # neither the patch statistic nor depth_cov
    ("mv_match_cov", dict(params=_cp(use_patch_var=0), depth_cov=P, N=0), OK),
    ("mv_match_cov", dict(params=_cp(use_patch_var=0, kernel_size=33)), UNSUPPORTED),                   # single forms: the kernel size is looked at first
    ("mv_match_cov", dict(out_cov_rot=P), INVALID),                                                     # R cov R^T without R
    # ---- mv_obs_cov: model + modifiers in front of the same
    ("mv_obs_cov", dict(N=0), OK),
    ("mv_obs_cov", dict(N=0, modifiers=0x21, model=L.MV_COV_NONE), OK),                                 # diag, then normalize
    ("mv_obs_cov", dict(N=0, model=3), INVALID),                                                        # the model is checked before the zero count
    ("mv_obs_cov", dict(model=-1), INVALID),
    ("mv_obs_cov", dict(modifiers=3), INVALID),                                                         # no such modifier
    ("mv_obs_cov", dict(modifiers=0x10), INVALID),                                                      # a step behind the end of the chain
    ("mv_obs_cov", dict(modifiers=0x11111), INVALID),                                                   # five steps
    ("mv_obs_cov", dict(N=-1), INVALID),
    ("mv_obs_cov", dict(kp_uv=None), INVALID),
    ("mv_obs_cov", dict(model=GMM), INVALID),                                                           # the mixture without the depth-variance map
    ("mv_obs_cov", dict(model=GMM, N=0), OK),
    ("mv_obs_cov", dict(params=_cp(kernel_size=6)), INVALID),
    ("mv_obs_cov", dict(params=_cp(kernel_size=33)), UNSUPPORTED),
    ("mv_obs_cov", dict(model=GMM, params=_cp(kernel_size=33)), UNSUPPORTED),                           # single forms: kernel size first
    ("mv_obs_cov", dict(params=_cp(use_patch_var=0)), INVALID),
    ("mv_obs_cov", dict(out_cov_rot=P), INVALID),
    # ---- mv_match_cov_pair: N rows in both sets, always the patch statistic
    ("mv_match_cov_pair", dict(N=0), OK),
    ("mv_match_cov_pair", dict(N=0, **NULLS0, flow_cov1=None), OK),
    ("mv_match_cov_pair", dict(N=-1), INVALID),
    ("mv_match_cov_pair", dict(N=0, params=None), INVALID),
    ("mv_match_cov_pair", dict(flow_cov1=None), INVALID),
    ("mv_match_cov_pair", dict(params=_cp(use_patch_var=0)), INVALID),
    ("mv_match_cov_pair", dict(params=_cp(kernel_size=33)), UNSUPPORTED),
    ("mv_match_cov_pair", dict(params=_cp(kernel_size=33, use_patch_var=0)), INVALID),                  # pair forms: use_patch_var first
    ("mv_match_cov_pair", dict(out_cov_rot0=P), INVALID),
    # ---- mv_match_cov_pair_lanes
    ("mv_match_cov_pair_lanes", Z, OK),
    ("mv_match_cov_pair_lanes", dict(Z, **NULLS0, flow_cov1=None), OK),
    ("mv_match_cov_pair_lanes", dict(Z, params=None), INVALID),
    ("mv_match_cov_pair_lanes", dict(lanes=0), INVALID),
    ("mv_match_cov_pair_lanes", dict(lanes=L.MV_MAX_LANES + 1), INVALID),
    ("mv_match_cov_pair_lanes", dict(n_live=None), INVALID),
    ("mv_match_cov_pair_lanes", dict(cap=-1, n_live=_i32(0, 0)), INVALID),
    ("mv_match_cov_pair_lanes", dict(n_live=_i32(3, 5)), INVALID),                                      # n_live > cap
    ("mv_match_cov_pair_lanes", dict(n_live=_i32(-1, 4)), INVALID),
    ("mv_match_cov_pair_lanes", dict(kp_uv1=None), INVALID),
    ("mv_match_cov_pair_lanes", dict(params=_cp(kernel_size=8)), INVALID),
    ("mv_match_cov_pair_lanes", dict(params=_cp(kernel_size=33)), UNSUPPORTED),
    ("mv_match_cov_pair_lanes", dict(params=_cp(use_patch_var=0)), INVALID),
    ("mv_match_cov_pair_lanes", dict(out_cov_rot0=P), INVALID),
    # ---- mv_obs_cov_pair_lanes
    ("mv_obs_cov_pair_lanes", Z, OK),
    ("mv_obs_cov_pair_lanes", dict(Z, model=GMM, modifiers=0x12), OK),
    ("mv_obs_cov_pair_lanes", dict(Z, model=3), INVALID),
    ("mv_obs_cov_pair_lanes", dict(Z, modifiers=0x100), INVALID),
    ("mv_obs_cov_pair_lanes", dict(lanes=L.MV_MAX_LANES + 1), INVALID),
    ("mv_obs_cov_pair_lanes", dict(n_live=_i32(5, 0)), INVALID),
    ("mv_obs_cov_pair_lanes", dict(out_cov1=None), INVALID),
    ("mv_obs_cov_pair_lanes", dict(model=GMM), INVALID),
    ("mv_obs_cov_pair_lanes", dict(model=GMM, depth_cov_map0=P), INVALID),                              # both maps
    ("mv_obs_cov_pair_lanes", dict(model=GMM, depth_cov_map0=P, depth_cov_map1=P, params=_cp(kernel_size=33)), UNSUPPORTED),
    ("mv_obs_cov_pair_lanes", dict(model=GMM, params=_cp(kernel_size=33)), INVALID),                    # pair forms: the maps first
    ("mv_obs_cov_pair_lanes", dict(params=_cp(use_patch_var=0)), INVALID),
    ("mv_obs_cov_pair_lanes", dict(params=_cp(kernel_size=2)), INVALID),
    ("mv_obs_cov_pair_lanes", dict(out_cov_rot0=P), INVALID),
    # ---- mv_obs_cov_pair_nomatch_lanes: set 1 has no flow_cov; the mixture also needs the depth variance at its keypoints
    ("mv_obs_cov_pair_nomatch_lanes", Z, OK),
    ("mv_obs_cov_pair_nomatch_lanes", dict(Z, **NULLS0), OK),
    ("mv_obs_cov_pair_nomatch_lanes", dict(Z, model=-1), INVALID),
    ("mv_obs_cov_pair_nomatch_lanes", dict(Z, modifiers=0x30), INVALID),
    ("mv_obs_cov_pair_nomatch_lanes", dict(lanes=0), INVALID),
    ("mv_obs_cov_pair_nomatch_lanes", dict(n_live=_i32(4, 5)), INVALID),
    ("mv_obs_cov_pair_nomatch_lanes", dict(kp_uv1=None), INVALID),
    ("mv_obs_cov_pair_nomatch_lanes", dict(flow_cov0=None), INVALID),
    ("mv_obs_cov_pair_nomatch_lanes", dict(model=GMM, depth_cov_map0=P, depth_cov_map1=P), INVALID),    # no depth_cov1
    ("mv_obs_cov_pair_nomatch_lanes", dict(model=GMM, depth_cov1=P), INVALID),                          # no maps
    ("mv_obs_cov_pair_nomatch_lanes", dict(params=_cp(kernel_size=33)), UNSUPPORTED),
    ("mv_obs_cov_pair_nomatch_lanes", dict(params=_cp(kernel_size=7, use_patch_var=0)), INVALID),
    ("mv_obs_cov_pair_nomatch_lanes", dict(out_cov_rot0=P), INVALID),
    # ---- mv_pgo_solve / mv_pgo_solve_local: the plain solve
    ("mv_pgo_solve", dict(nprob=0), OK),
    ("mv_pgo_solve", dict(nprob=0, offsets=None, init_pose=None, out_pose=None), OK),
    ("mv_pgo_solve", dict(nprob=0, lm=None), INVALID),
    ("mv_pgo_solve", dict(nprob=-1), INVALID),
    ("mv_pgo_solve", dict(offsets=None), INVALID),
    ("mv_pgo_solve", dict(out_info=None), INVALID),
    ("mv_pgo_solve", dict(lm=_lm(max_steps=0)), INVALID),
    ("mv_pgo_solve", dict(lm=_lm(huber_delta=0.0)), INVALID),
    ("mv_pgo_solve", dict(graph_type=3), INVALID),
    ("mv_pgo_solve", dict(graph_type=ICP, cov_Tw=None), INVALID),
    ("mv_pgo_solve", dict(pixel2_disp=None), INVALID),                                                  # the disparity graph's own table
    ("mv_pgo_solve_local", dict(nprob=0), OK),
    ("mv_pgo_solve_local", dict(nprob=0, ref_pose=None), INVALID),                                      # a local form without its frame
    ("mv_pgo_solve_local", dict(ref_pose=None), INVALID),
    ("mv_pgo_solve_local", dict(intrinsics=None), INVALID),
    ("mv_pgo_solve_local", dict(graph_type=-1), INVALID),
    # ---- the six posed solves
    ("mv_pgo_solve_posed", dict(nprob=0), OK),
    ("mv_pgo_solve_posed", dict(nprob=0, n_live=None), INVALID),                                        # neither n_live nor n_live_dev
    ("mv_pgo_solve_posed", dict(n_live=None), INVALID),
    ("mv_pgo_solve_posed", dict(nprob=0, pos_Tc=None), INVALID),
    ("mv_pgo_solve_posed", dict(nprob=0, cov_Tw=None), INVALID),                                        # cov_Tc without its world-frame table
    ("mv_pgo_solve_posed", dict(nprob=0, cov_Tc=None, cov_Tw=None), OK),
    ("mv_pgo_solve_posed", dict(nprob=512), INVALID),
    ("mv_pgo_solve_posed", dict(nprob=L.MV_MAX_LANES + 1), INVALID),
    ("mv_pgo_solve_posed", dict(n_live=_i32(3, 5)), INVALID),                                           # n_live > cap under the filters
    ("mv_pgo_solve_posed", dict(n_live=_i32(-1, 4)), INVALID),
    ("mv_pgo_solve_posed", dict(valid=None), INVALID),
    ("mv_pgo_solve_posed", dict(filter_flags=1, cov_Tc=None), INVALID),                                 # the covariance filter without covariances
    ("mv_pgo_solve_posed", dict(vals=None), INVALID),
    ("mv_pgo_solve_posed", dict(lm=None), INVALID),
    ("mv_pgo_solve_posed", dict(graph_type=5), INVALID),
    ("mv_pgo_solve_posed_dev", dict(nprob=0), OK),
    ("mv_pgo_solve_posed_dev", dict(nprob=0, n_live_dev=None), INVALID),
    ("mv_pgo_solve_posed_dev", dict(nprob=0, n_live_stride=0), INVALID),
    ("mv_pgo_solve_posed_dev", dict(nprob=512), INVALID),
    ("mv_pgo_solve_posed_dev", dict(count_out=None), INVALID),
    ("mv_pgo_solve_posed_dev", dict(cap=-1), INVALID),
    ("mv_pgo_solve_posed_motion", dict(nprob=0), OK),
    ("mv_pgo_solve_posed_motion", dict(nprob=0, start_pose=None), INVALID),                             # a motion form without its prior
    ("mv_pgo_solve_posed_motion", dict(nprob=0, n_live=None), INVALID),
    ("mv_pgo_solve_posed_motion", dict(nprob=512), INVALID),
    ("mv_pgo_solve_posed_motion", dict(n_live=_i32(5, 5)), INVALID),
    ("mv_pgo_solve_posed_motion", dict(pos_Tw=None), INVALID),
    ("mv_pgo_solve_posed_motion_dev", dict(nprob=0), OK),
    ("mv_pgo_solve_posed_motion_dev", dict(nprob=0, start_pose=None), INVALID),
    ("mv_pgo_solve_posed_motion_dev", dict(nprob=0, n_live_dev=None), INVALID),
    ("mv_pgo_solve_posed_motion_dev", dict(nprob=0, n_live_stride=0), INVALID),
    ("mv_pgo_solve_posed_motion_dev", dict(nprob=600), INVALID),
    ("mv_pgo_solve_posed_local", dict(nprob=0), OK),
    ("mv_pgo_solve_posed_local", dict(nprob=0, start_pose=None), OK),                                   # the prior is optional here
    ("mv_pgo_solve_posed_local", dict(nprob=0, ref_pose=None), INVALID),
    ("mv_pgo_solve_posed_local", dict(nprob=0, n_live=None), INVALID),
    ("mv_pgo_solve_posed_local", dict(nprob=512), INVALID),
    ("mv_pgo_solve_posed_local", dict(n_live=_i32(0, 9)), INVALID),
    ("mv_pgo_solve_posed_local_dev", dict(nprob=0), OK),
    ("mv_pgo_solve_posed_local_dev", dict(nprob=0, start_pose=None), OK),
    ("mv_pgo_solve_posed_local_dev", dict(nprob=0, ref_pose=None), INVALID),
    ("mv_pgo_solve_posed_local_dev", dict(nprob=0, n_live_dev=None), INVALID),
    ("mv_pgo_solve_posed_local_dev", dict(nprob=512), INVALID),
    ("mv_pgo_solve_posed_local_dev", dict(out_pose=None), INVALID),
    # ---- the window lookups: each form's own domain
    ("mv_corr_lookup", dict(vol=None), INVALID),
    ("mv_corr_lookup", dict(B=0), INVALID),
    ("mv_corr_lookup", dict(H2=1), INVALID),
    ("mv_corr_lookup", dict(radius=0), UNSUPPORTED),
    ("mv_corr_lookup", dict(radius=5), UNSUPPORTED),
    ("mv_corr_lookup", dict(B=65536), UNSUPPORTED),
    ("mv_corr_lookup", dict(radius=0, coords=None), INVALID),
    ("mv_corr_lookup_vol16", dict(coords=None), INVALID),
    ("mv_corr_lookup_vol16", dict(W1=0), INVALID),
    ("mv_corr_lookup_vol16", dict(radius=3), UNSUPPORTED),                                              # radius 4 only
    ("mv_corr_lookup_vol16", dict(radius=5), UNSUPPORTED),
    ("mv_corr_lookup_vol16", dict(B=65536), UNSUPPORTED),
    ("mv_corr_lookup_tiled", dict(out=None), INVALID),
    ("mv_corr_lookup_tiled", dict(W2=1), INVALID),
    ("mv_corr_lookup_tiled", dict(radius=1), UNSUPPORTED),
    ("mv_corr_lookup_tiled", dict(H2=10), UNSUPPORTED),                                                 # whole 4 x 4 tiles
    ("mv_corr_lookup_tiled", dict(W2=10), UNSUPPORTED),
    ("mv_corr_lookup_tiled", dict(B=65536), UNSUPPORTED),
    ("mv_corr_lookup_tiled_vol16", dict(vol=None), INVALID),
    ("mv_corr_lookup_tiled_vol16", dict(vol=P + 16), INVALID),                                          # a tile = one 32-byte sector
    ("mv_corr_lookup_tiled_vol16", dict(vol=P + 16, radius=3), INVALID),                                # ... checked before the radius
    ("mv_corr_lookup_tiled_vol16", dict(radius=3), UNSUPPORTED),
    ("mv_corr_lookup_tiled_vol16", dict(W2=6), UNSUPPORTED),
    ("mv_corr_lookup_tiled_vol16", dict(H1=0), INVALID),
]


def _call(sym, over):
    unknown = set(over) - set(NAMES[sym])
    assert not unknown, (sym, unknown)          # a row must override arguments its entry point has
    vals = {"lm": _lm(), **DEFAULTS, **over}
    args = []
    for n in NAMES[sym]:
        v = vals.get(n, P)
        args.append(C.cast(v, C.c_void_p) if isinstance(v, C.Array) else v)   # (structures go by reference through their POINTER argtypes)
    return getattr(L.load(), sym)(*args)


def test_every_touched_entry_point_is_in_the_table():
    assert {s for s, _, _ in TABLE} == set(NAMES) and len(NAMES) == 18
    for sym, names in NAMES.items():
        assert len(names) == len(L.SIGNATURES[sym][1]), sym


@pytest.mark.parametrize("sym", sorted(NAMES))
def test_entry_point_accepts_what_it_always_did(sym):
    got = [(over, _call(s, over), want) for s, over, want in TABLE if s == sym]
    bad = [(sorted(over), code, want) for over, code, want in got if code != want]
    assert not bad, f"{sym}: (overridden arguments, returned, expected) {bad}"
