"""The selector's finishing pass (second launch of mv_kp_select) off its in-register fast path, against oracle/selector.py on the CPU.

The finishing workgroup keeps records and candidate words in registers while both fit ``mv_kp_select_finish_capacity``; past either limit the same steps run
against global memory (medians re-read from the record arrays, failing bits cleared with global atomics, compaction through atomic loads).  Every case
below states, from that query and the record count the launch returned, which of the two forms it ran, so that none can drift back onto the fast path:
  a. more records than fit (window 3 on noisy maps, window 1 where every pixel is a record; NODEPTH and FULL with and without flow_cov; both variants),
  b. exactly the capacity and one record more,
  c. more candidate words than fit with fewer records than fit (769 x 1280),
  d. every supported NMS window 1 .. 15 on maps with NaN / inf / plateaus on tile seams, fused and un-fused, and window 17 refused,
  e. median populations the synthetic maps never produce (tests/kp_median_twin.py, established on the host model first), in both forms,
  f. two lanes of which one runs each form, and one workspace reused across the forms,
  g. the 512-thread variant (MV_KP_FINISH_SMALL_NT=512) against the default one, each in an interpreter of its own.
Checked per case: the candidate list, the record count, both medians and thresholds by value, and the pixels drawn under a fixed seed."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from tests import kp_median_twin as T
from tests import selector_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PICK, SEED, MW = 50, 31, 8
_dev = {}


def _lib():
    from macvo_amd import _lib as L

    return L.load(), L


def _synth_on(gpu, H, W):
    """CPU maps and their device copies, once per shape."""
    if (H, W) not in _dev:
        cpu = S.synth_maps(H, W)
        _dev[(H, W)] = (cpu, {k: v.to(gpu) for k, v in cpu.items()})
    return _dev[(H, W)]


def _oracle(mode, m, ksize, mw, max_match_cov=S.MAX_MATCH_COV):
    """oracle/selector.py on CPU maps [1, c, H, W] (masks bool) under the fixed seed -> (pixels, candidates, aux)."""
    from oracle import selector

    torch.manual_seed(SEED)
    if mode == "nodepth":
        return selector.cov_aware_selector_nodepth(m["flow_cov"].clone(), N_PICK, ksize, mw, max_match_cov, match_mask=m.get("mask_b"))
    fc = m.get("flow_cov")
    return selector.cov_aware_selector(m["depth0"], m["depth0_cov"], m["depth1"], m["depth1_cov"], None if fc is None else fc.clone(), N_PICK,
                                       S.FULL_MAX_DEPTH, ksize, mw, S.FULL_MAX_DEPTH_COV, max_match_cov, depth0_mask=m.get("mask_a"),
                                       match_mask=m.get("mask_b"))


def _same(a, b):
    return a == b or (a != a and b != b)


def _f32(x):
    return float(np.float32(x))


def _check(r, lane, ref, mode, has_flow, H, W, caps, expect):
    """One lane of a launch against the oracle's (pixels, candidates, aux), and the form it ran in (``expect``: "fast" / "global")."""
    from macvo_amd import ops

    ref_px, ref_cand, aux = ref
    c = ops.KeypointCandidates(r["cand"][lane], r["count"][lane], r["stats"][lane], W)
    count, stats = r["count"][lane].cpu(), [float(x) for x in r["stats"][lane].cpu()]
    n_rec, n_words = int(count[1]), H * ((W + 63) // 64)
    print(f"  {H}x{W} {mode} lane {lane}: records {n_rec} / capacity {caps[0]}, words {n_words} / {caps[1]}, candidates {int(count[0])}, "
          f"stats {stats} -> expected form: {expect}")
    assert n_rec == aux["n_nms"]
    assert ("fast" if (n_rec <= caps[0] and n_words <= caps[1]) else "global") == expect, (n_rec, n_words, caps)
    assert int(count[0]) == ref_cand.shape[0] and int(count[2]) == 0 and int(count[3]) == 0
    assert torch.equal(c.candidates_vu().cpu(), ref_cand)
    assert c.n == H * W or int(r["cand"][lane, c.n:].max()) == -1                   # nothing written behind the list
    if mode == "nodepth":
        want = [aux["median"], _f32(aux["thresh"]), float("nan"), float("inf")]
    else:
        want = [aux["median_flow_cov"], _f32(aux["flow_cov_thresh"])] if has_flow else [float("nan"), float("inf")]
        want += [aux["median_depth_cov"], _f32(aux["depth_cov_thresh"])]
    assert all(_same(g, w) for g, w in zip(stats, want)), (stats, want)
    torch.manual_seed(SEED)
    assert torch.equal(c.finish(N_PICK).cpu(), ref_px)
    return n_rec


def _case(gpu, mode, H, W, ksize, cpu, dev, expect, mw=MW, max_match_cov=S.MAX_MATCH_COV, caps=None):
    lib, L = _lib()
    caps = caps or S.capacity(lib, H, W)
    r = S.select(lib, L, gpu, mode, H, W, ksize, mw, dev, max_depth=S.FULL_MAX_DEPTH, max_depth_cov=S.FULL_MAX_DEPTH_COV, max_match_cov=max_match_cov)
    return _check(r, 0, _oracle(mode, cpu, ksize, mw, max_match_cov), mode, dev.get("flow_cov") is not None, H, W, caps, expect)


def _only(m, *names):
    return {k: m[k] for k in names}


_DEPTHS = ("depth0", "depth0_cov", "depth1", "depth1_cov")


# ---------------------------------------------------------------------------------------------------- a. over the record capacity
@pytest.mark.parametrize("H,W,ksize,mode,flow", [(360, 480, 3, "nodepth", True), (136, 128, 1, "nodepth", True), (136, 128, 1, "full", True),
                                                 (136, 128, 1, "full", False), (257, 1280, 3, "nodepth", True)])
def test_more_records_than_the_registers_hold(gpu, H, W, ksize, mode, flow):
    cpu, dev = _synth_on(gpu, H, W)
    lib, _ = _lib()
    caps = S.capacity(lib, H, W)
    if (H, W) == (257, 1280):
        assert H * ((W + 63) // 64) > S.capacity(lib, 480, 640)[1] and caps[0] > S.capacity(lib, 480, 640)[0]       # the large variant
    if mode == "nodepth":
        n_rec = _case(gpu, mode, H, W, ksize, _only(cpu, "flow_cov"), _only(dev, "flow_cov"), "global")
    else:
        cpu, dev = dict(cpu), dict(dev)
        d0c = cpu["depth0_cov"].clone()
        d0c[0, 0, H // 2, W // 3] = float("nan")                     # its quality is NaN: no record, and no NaN reaches the depth-variance median
        cpu["depth0_cov"], dev["depth0_cov"] = d0c, d0c.to(gpu)
        below = (cpu["depth0"] < S.FULL_MAX_DEPTH) & (cpu["depth1"] < S.FULL_MAX_DEPTH)
        assert 0.1 < below.float().mean() < 0.9                       # both outcomes of the depth test
        names = _DEPTHS + (("flow_cov",) if flow else ())
        n_rec = _case(gpu, mode, H, W, ksize, _only(cpu, *names), _only(dev, *names), "global")
    assert n_rec > caps[0]


def test_more_records_than_fit_with_a_mask_and_a_low_cap(gpu):
    """136 x 128, window 1, a validity mask and a max_match_cov below 1.5 medians: most candidate records fail and clear their bit in global memory."""
    H, W = 136, 128
    cpu, dev = _synth_on(gpu, H, W)
    g = torch.Generator().manual_seed(9)
    mask = torch.rand(1, 1, H, W, generator=g) < 0.7
    fc = cpu["flow_cov"]
    cap = float((fc[:, 0] + fc[:, 1] - 2 * fc[:, 2]).median()) * 0.75
    ref = _oracle("nodepth", {"flow_cov": fc, "mask_b": mask}, 1, MW, cap)
    assert ref[2]["thresh"] == cap and 0 < ref[1].shape[0] < 0.45 * 0.7 * (H - 2 * MW) * (W - 2 * MW)
    lib, L = _lib()
    r = S.select(lib, L, gpu, "nodepth", H, W, 1, MW, {"flow_cov": dev["flow_cov"], "mask_b": mask.to(torch.uint8).to(gpu)}, max_match_cov=cap)
    _check(r, 0, ref, "nodepth", True, H, W, S.capacity(lib, H, W), "global")


# ---------------------------------------------------------------------------------------------------- b. the exact boundary
def test_exactly_the_record_capacity_and_one_more(gpu):
    """128 x 130, window 1: NaNs planted so that the records number exactly the capacity (in registers), then one NaN fewer (global memory)."""
    H, W = 128, 130
    lib, L = _lib()
    caps = S.capacity(lib, H, W)
    n_nan = H * W - caps[0]
    assert 1 <= n_nan < H * W
    cpu, _ = _synth_on(gpu, H, W)
    at = torch.randperm(H * W, generator=torch.Generator().manual_seed(4))[:n_nan]
    n_recs = []
    for extra, expect in ((0, "fast"), (1, "global")):
        fc = cpu["flow_cov"].clone()
        fc[0, 0].view(-1)[at[extra:]] = float("nan")                  # `extra` = 1: the first planted pixel keeps its value
        n_recs.append(_case(gpu, "nodepth", H, W, 1, {"flow_cov": fc}, {"flow_cov": fc.to(gpu)}, expect, caps=caps))
    assert n_recs == [caps[0], caps[0] + 1]


# ---------------------------------------------------------------------------------------------------- c. over the word capacity only
@pytest.mark.parametrize("mode", ["nodepth", "full"])
def test_more_candidate_words_than_fit_but_fewer_records(gpu, mode):
    H, W = 769, 1280
    cpu, dev = _synth_on(gpu, H, W)
    lib, _ = _lib()
    caps = S.capacity(lib, H, W)
    assert H * ((W + 63) // 64) > caps[1] >= (H - 1) * ((W + 63) // 64)     # one row of words too many
    names = ("flow_cov",) if mode == "nodepth" else _DEPTHS + ("flow_cov",)
    n_rec = _case(gpu, mode, H, W, 7, _only(cpu, *names), _only(dev, *names), "global")
    assert 0 < n_rec <= caps[0]


# ---------------------------------------------------------------------------------------------------- d. every window size
WINDOWS = (1, 3, 5, 7, 9, 11, 13, 15)


@pytest.mark.parametrize("cov_is_log", [True, False])
@pytest.mark.parametrize("H,W", [(40, 72), (33, 130)])
def test_every_window_size_fused_and_unfused(gpu, H, W, cov_is_log):
    """NODEPTH: the fused launch is bitwise the epilogue followed by the selector, and both are the oracle on the covariance planes the launch wrote."""
    lib, L = _lib()
    caps = S.capacity(lib, H, W)
    flow, cov = S.inputs_on(gpu, H, W, 1, cov_is_log)
    strip = (min(H, W) - 2) // 2
    for ksize in WINDOWS:
        for mw in (0, strip, 3):                                      # none, a strip two or three pixels wide, nearly the whole image
            fu = S.run(lib, L, gpu, H, W, 1, True, flow, cov, cov_is_log, ksize, mw)
            un = S.run(lib, L, gpu, H, W, 1, False, flow, cov, cov_is_log, ksize, mw)
            for name in ("disparity", "disparity_cov", "depth", "depth_cov", "match_flow", "match_cov", "stats"):
                assert torch.equal(fu[name].view(torch.int32), un[name].view(torch.int32)), (name, ksize, mw)
            assert torch.equal(fu["bad_mask"], un["bad_mask"]) and torch.equal(fu["count"], un["count"]), (ksize, mw)
            n = int(fu["count"][0, 0])
            assert torch.equal(fu["cand"][0, :n], un["cand"][0, :n]), (ksize, mw)
            for res in (fu, un):                                      # mask_width 0: `border[0:-0]` of the reference is empty, no candidates
                r = {k: res[k].to(gpu) for k in ("cand", "count", "stats")}
                r["cand"][0, n:] = -1
                assert mw > 0 or n == 0
                _check(r, 0, _oracle("nodepth", {"flow_cov": res["match_cov"]}, ksize, mw), "nodepth", True, H, W, caps, "fast")


@pytest.mark.parametrize("H,W", [(40, 72), (33, 130)])
def test_every_window_size_full(gpu, H, W):
    """FULL on the maps the epilogue makes of the same inputs: lane 0 = frame 0, lane 1 = frame 1 (NaN and inf depths and variances among them)."""
    lib, L = _lib()
    caps = S.capacity(lib, H, W)
    flow, cov = S.inputs_on(gpu, H, W, 2, True)
    maps = S.run(lib, L, gpu, H, W, 2, False, flow, cov, True, 7, 1)
    cpu = {"depth0": maps["depth"][0:1], "depth0_cov": maps["depth_cov"][0:1], "depth1": maps["depth"][1:2], "depth1_cov": maps["depth_cov"][1:2],
           "flow_cov": maps["match_cov"][0:1]}
    cpu = {k: v.contiguous() for k, v in cpu.items()}
    below = (cpu["depth0"] < S.FULL_MAX_DEPTH) & (cpu["depth1"] < S.FULL_MAX_DEPTH)
    assert 0.1 < below.float().mean() < 0.9
    dev = {k: v.to(gpu) for k, v in cpu.items()}
    strip = (min(H, W) - 2) // 2
    for ksize in WINDOWS:
        for mw in (0, strip, 3):                                      # none, a strip two or three pixels wide, nearly the whole image
            _case(gpu, "full", H, W, ksize, cpu, dev, "fast", mw=mw, caps=caps)


def test_window_17_is_unsupported(gpu):
    import ctypes as C

    lib, L = _lib()
    H, W = 40, 72
    _, dev = _synth_on(gpu, H, W)
    ws = S.fresh_workspace(lib, gpu, H, W)
    cand, count, stats = torch.zeros(H * W, dtype=torch.int32, device=gpu), torch.zeros(4, dtype=torch.int32, device=gpu), torch.zeros(4, device=gpu)
    for mode in (L.MV_KP_NODEPTH, L.MV_KP_FULL):
        p = L.mvKpSelectParams(H, W, mode, 17, MW, 40.0, 250.0, 100.0)
        rc = lib.mv_kp_select(dev["flow_cov"].data_ptr(), dev["depth0"].data_ptr(), dev["depth0_cov"].data_ptr(), dev["depth1"].data_ptr(),
                              dev["depth1_cov"].data_ptr(), None, None, C.byref(p), ws.data_ptr(), ws.numel() * 8, cand.data_ptr(), count.data_ptr(),
                              stats.data_ptr(), None)
        assert rc == -2                                               # MV_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert int(ws.abs().max()) == 0 and int(count.abs().max()) == 0   # refused on the host: nothing ran


# ---------------------------------------------------------------------------------------------------- e. median populations
POP_SHAPES = [(48, 64), (136, 128)]
POP_NAMES = [name for name, _ in T.populations(48 * 64)]


@pytest.mark.parametrize("name", POP_NAMES)
@pytest.mark.parametrize("H,W", POP_SHAPES)
def test_median_populations_in_both_forms(gpu, H, W, name):
    """NODEPTH, window 1, plane 0 = the population (NaN = no record), planes 1 and 2 = 0: the quality is the value itself and the records are the
    population.  48 x 64 fills three register slots of the in-register form; 136 x 128 runs the global-memory form — except where the population has one
    or two members, which no shape can take past the capacity."""
    pop = dict(T.populations(H * W))[name]
    med, rounds = T.nanmedian_twin(pop)                               # the host model first: it ends, and says what the kernel's loop will do
    assert rounds <= T.MAX_ROUNDS
    fc = torch.zeros(1, 3, H, W)
    fc[0, 0] = torch.from_numpy(pop).view(H, W)
    lib, _ = _lib()
    caps = S.capacity(lib, H, W)
    members = int((~np.isnan(pop)).sum())
    expect = "global" if members > caps[0] else "fast"
    assert (expect == "global") == ((H, W) == (136, 128) and name not in ("single_member", "two_members"))
    print(f"  population {name}: {members} members, host model: median {float(med)!r} after {rounds} histogram round(s)")
    n_rec = _case(gpu, "nodepth", H, W, 1, {"flow_cov": fc}, {"flow_cov": fc.to(gpu)}, expect, caps=caps)
    assert n_rec == members


# ---------------------------------------------------------------------------------------------------- f. lanes and reuse
def _two_maps(gpu):
    """136 x 128: the full synthetic map (every pixel a record at window 1) and the same with a NaN block that leaves fewer records than fit."""
    H, W = 136, 128
    lib, _ = _lib()
    caps = S.capacity(lib, H, W)
    cpu, _ = _synth_on(gpu, H, W)
    full = cpu["flow_cov"]
    rows = (H * W - caps[0] + W - 1) // W + 1
    assert 0 < rows < H - 2 * MW
    holed = full.clone()
    holed[0, 0, 20:20 + rows] = float("nan")
    return H, W, caps, full, holed


def test_two_lanes_one_in_each_form(gpu):
    H, W, caps, full, holed = _two_maps(gpu)
    lib, L = _lib()
    both = torch.cat([full, holed]).contiguous()
    r = S.select(lib, L, gpu, "nodepth", H, W, 1, MW, {"flow_cov": both.to(gpu)}, lanes=2)
    n0 = _check(r, 0, _oracle("nodepth", {"flow_cov": full}, 1, MW), "nodepth", True, H, W, caps, "global")
    n1 = _check(r, 1, _oracle("nodepth", {"flow_cov": holed}, 1, MW), "nodepth", True, H, W, caps, "fast")
    assert n0 == H * W > caps[0] >= n1 > 0


def test_one_workspace_across_the_forms(gpu):
    """Global form, in-register form, global form again on ONE workspace: each call equals the same call on a freshly zeroed workspace (the counters are
    left zeroed, and nothing a form leaves in the record arrays or the candidate words reaches the next call)."""
    H, W, caps, full, holed = _two_maps(gpu)
    lib, L = _lib()
    dev = {"global": {"flow_cov": full.to(gpu)}, "fast": {"flow_cov": holed.to(gpu)}}
    fresh = {k: S.select(lib, L, gpu, "nodepth", H, W, 1, MW, m) for k, m in dev.items()}
    assert int(fresh["global"]["count"][0, 1]) > caps[0] >= int(fresh["fast"]["count"][0, 1]) > 0
    ws = S.fresh_workspace(lib, gpu, H, W)
    for step, form in enumerate(("global", "fast", "global")):
        r = S.select(lib, L, gpu, "nodepth", H, W, 1, MW, dev[form], ws=ws)
        for name in ("cand", "count", "stats"):
            assert torch.equal(r[name].view(torch.int32), fresh[form][name].view(torch.int32)), (step, form, name)
    _check(fresh["global"], 0, _oracle("nodepth", {"flow_cov": full}, 1, MW), "nodepth", True, H, W, caps, "global")
    _check(fresh["fast"], 0, _oracle("nodepth", {"flow_cov": holed}, 1, MW), "nodepth", True, H, W, caps, "fast")


# ---------------------------------------------------------------------------------------------------- g. the 512-thread variant
_CHILD = "import sys; sys.path.insert(0, sys.argv[1]); from tests.selector_cases import finish_variant_child; finish_variant_child(sys.argv[2])"


def test_the_512_thread_variant_gives_the_default_variants_bits(gpu):
    """MV_KP_FINISH_SMALL_NT is read once per process: one child interpreter per value.  360 x 480 with window 3 is past the 512-thread variant's capacity
    (and the default's), 96 x 130 with window 7 far below both; NODEPTH and FULL.  The children agree bit for bit, and with the oracle here."""
    outs = {}
    for knob in ("512", None):
        env = {k: v for k, v in os.environ.items() if k != "MV_KP_FINISH_SMALL_NT"}
        if knob:
            env["MV_KP_FINISH_SMALL_NT"] = knob
        d = tempfile.mkdtemp()
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, d], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (knob, r.stderr[-3000:])            # nothing is started after a failing child
        outs[knob] = torch.load(os.path.join(d, "variant.pt"), weights_only=False)
    small, default = outs["512"], outs[None]
    assert small.keys() == default.keys() and len(small) == 2 * len(S.VARIANT_CASES)
    lib, _ = _lib()
    for key in small:
        H, W, ksize, mode = key
        assert small[key]["caps"] == (8192, 5120) and default[key]["caps"] == S.capacity(lib, H, W) and default[key]["caps"][0] > 8192
        for name in ("cand", "count", "stats"):
            assert torch.equal(small[key][name].view(torch.int32), default[key][name].view(torch.int32)), (key, name)
        cpu, _ = _synth_on(gpu, H, W)
        names = ("flow_cov",) if mode == "nodepth" else _DEPTHS + ("flow_cov",)
        ref = _oracle(mode, _only(cpu, *names), ksize, S.VARIANT_MASK_WIDTH)
        for res in (small[key], default[key]):
            n = res["cand"].shape[0]
            r = {"cand": torch.full((1, H * W), -1, dtype=torch.int32), "count": res["count"][None], "stats": res["stats"][None]}
            r["cand"][0, :n] = res["cand"]
            _check({k: v.to(gpu) for k, v in r.items()}, 0, ref, mode, True, H, W, res["caps"], "global" if ksize == 3 else "fast")
