"""The frame driver's schedule, pinned on the CPU (no GPU needed).

``csrc/frame_pipe.hip`` holds no device code and the whole library imports 28 HIP runtime symbols.  ``tests/c_abi/fake_hip.cpp`` defines those 28 and logs instead
of executing; linked with the library's own objects and ``tests/c_abi/pipe_trace.cpp`` it prints, for a named scenario, every stream the driver creates, every
launch (kernel, stream, grid, block, LDS), every event record / wait / query (``wait_if_pending``: a query answered "not ready" and the wait behind it), every copy with arena-relative offsets, and at the end ``mv_frame_pipe_arena_bytes``
and ``mv_frame_pipe_buffer`` of every id.  Each scenario's trace must equal its section of ``tests/golden/frame_pipe_trace_<group>.txt`` byte for byte, so a
change of the schedule or of the arena layout reads as a diff of those files.

A section is ``### name`` and the whole trace, or ``### name ~ other`` and only what differs from the trace of an earlier scenario (``--write`` picks the
nearest one, usually the same scenario without the knob): ``@ i j`` = lines i .. j - 1 of the other trace (counted from 0) are replaced by the ``+`` lines that follow.  So the section of ``MV_PIPE_LEAN=0`` reads as "these records come back", and a knob without effect on the schedule has an empty one.

    python tests/test_frame_pipe_trace_host.py NAME       print one scenario's trace (--list: the names)
    python tests/test_frame_pipe_trace_host.py --write    regenerate the fixtures from the library as built

``MACVO_TRACE_OBJS=<dir>`` links the harness against the objects of another build (a parent checkout's ``csrc/build``) instead of this tree's."""
import collections
import difflib
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mac-vo_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HIPCC = os.environ.get("HIPCC", "hipcc")
SOURCES = [os.path.join(ROOT, "tests", "c_abi", f) for f in ("fake_hip.cpp", "pipe_trace.cpp")]
# the flags csrc/Makefile compiles frame_pipe.hip with
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-Wall", "-Wno-unused-function"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="needs hipcc (cross-compiles without a GPU)")


def delta(base: str, trace: str) -> str:
    """``trace`` as its difference from ``base`` (the format of the module docstring)."""
    a, b = base.splitlines(), trace.splitlines()
    out = []
    for op, i, j, k, l in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
        if op != "equal":
            out += [f"@ {i} {j}"] + ["+" + x for x in b[k:l]]
    return "".join(x + "\n" for x in out)


def patched(base: str, d: str) -> str:
    """The trace that ``delta(base, trace)`` came from."""
    a, out, at = base.splitlines(), [], 0
    for line in d.splitlines():
        if line.startswith("@ "):
            i, j = map(int, line.split()[1:])
            assert at <= i <= j <= len(a), line
            out += a[at:i]
            at = j
        else:
            assert line.startswith("+"), line
            out.append(line[1:])
    return "".join(x + "\n" for x in out + a[at:])


def fixtures() -> "collections.OrderedDict[str, tuple[str, str]]":
    """scenario -> (group, trace) of the committed fixtures."""
    raw = collections.OrderedDict()
    for path in sorted(glob.glob(os.path.join(GOLDEN, "frame_pipe_trace_*.txt"))):
        group = os.path.basename(path)[len("frame_pipe_trace_"):-len(".txt")]
        for section in open(path).read().split("### ")[1:]:
            head, _, body = section.partition("\n")
            name, _, like = head.partition(" ~ ")
            raw[name] = (group, like, body)

    def whole(name):
        _, like, body = raw[name]
        return patched(whole(like), body) if like else body

    return collections.OrderedDict((name, (raw[name][0], whole(name))) for name in raw)


FIXTURES = {} if sys.argv[1:] == ["--write"] else fixtures()   # (--write does not depend on what it replaces)


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    return r.stdout


def _out_dir() -> str:
    d = os.path.join(tempfile.gettempdir(), f"macvo_pipe_trace_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    return d


def _host_compiler() -> list:
    """clang++ of the HIP toolchain (the sanitized object needs its runtime at link time) and where <hip/hip_runtime_api.h> lives."""
    clang = os.path.join(_run(["hipconfig", "--hipclangpath"]).strip(), "clang++")
    rocm = _run(["hipconfig", "--rocmpath"]).strip()
    return [clang, "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include")]


def _objects() -> list:
    """The library's objects: this tree's (made here; nothing to do after build()), or those of the build MACVO_TRACE_OBJS names."""
    d = os.environ.get("MACVO_TRACE_OBJS")
    if not d:
        _run(["make", "-C", CSRC, "-j16"])
        d = os.path.join(CSRC, "build")
    objs = sorted(glob.glob(os.path.join(d, "*.o")))
    assert any(os.path.basename(o) == "frame_pipe.o" for o in objs), d
    return objs


def build(sanitized: bool = False) -> str:
    """Link the trace program; ``sanitized``: frame_pipe.hip compiled again with the host sanitizers, and the harness with it."""
    exe = os.path.join(_out_dir(), "pipe_trace_asan" if sanitized else "pipe_trace") + f".{os.getpid()}"
    objs = _objects()
    extra = ["-O1", "-g"]
    if sanitized:
        fp = os.path.join(_out_dir(), f"frame_pipe_asan.{os.getpid()}.o")
        host_only = [x for f in SANITIZE for x in ("-Xarch_host", f)]   # (the device side of the translation unit is not instrumented)
        _run([HIPCC] + HIP_FLAGS + ["-g"] + host_only + ["-c", os.path.join(CSRC, "frame_pipe.hip"), "-o", fp], cwd=CSRC)
        assert "__asan_report" in _run(["nm", fp]), "frame_pipe.hip was compiled without the address sanitizer"
        objs = [fp if os.path.basename(o) == "frame_pipe.o" else o for o in objs]
        extra += SANITIZE
    _run(_host_compiler() + extra + SOURCES + objs + ["-o", exe, "-lpthread"])
    return exe


@pytest.fixture(scope="module")
def tracer():
    exe = build()
    yield exe
    os.remove(exe)


def trace(exe: str, name: str, launch_thread: bool = False) -> str:
    return _run([exe, name] + (["--async"] if launch_thread else []))


def scenario_list(exe: str) -> list:
    return [tuple(line.split()) for line in _run([exe, "--list"]).splitlines()]


def test_fixtures_cover_every_scenario(tracer):
    assert [(g, n) for n, (g, _) in FIXTURES.items()] == sorted(scenario_list(tracer), key=lambda gn: gn[0]) and len(FIXTURES) >= 100
    for path in glob.glob(os.path.join(GOLDEN, "frame_pipe_trace_*.txt")):
        assert os.path.getsize(path) < 512 * 1024, path


@pytest.mark.parametrize("name", list(FIXTURES))
def test_trace_equals_fixture(tracer, name):
    got, want = trace(tracer, name), FIXTURES[name][1]
    if got != want:
        diff = "\n".join(list(difflib.unified_diff(want.splitlines(), got.splitlines(), "fixture", "trace", lineterm="", n=4))[:80])
        pytest.fail(f"the schedule of scenario {name} differs from tests/golden/frame_pipe_trace_{FIXTURES[name][0]}.txt:\n{diff}")


# the launch (or the line) that proves a scenario took the branch it is there for; "!": must not occur
# (backend_front_kernel<PM, ...>: rows from 0 a permutation in device memory, 1 one in the kernel arguments, 2 the draw inside the launch, 3 (u, v) rows,
#  4 RandomSelector drawn inside the launch, 5 GridSelector)
BRANCHES = {
    "one_device": ["# device_draw 1", "corr_volume_split_stream<2, true", "backend_front_kernel<2,", "stream_create S4 flags 1 priority -1", "!stream_create S5"],
    "one_perm": ["# device_draw 0", "backend_front_kernel<1,", "# n_cand 400 n_sel 50", "!memcpy_async S4 A+"],
    "one_perm_300": ["# n_cand 400 n_sel 300", "bytes 2400 kind 1", "backend_front_kernel<0,"],
    "one_seeded": ["# device_draw 0", "# n_cand 400 n_sel 50"],
    "one_seeds_600": ["# device_draw 0", "# n_cand 400 n_sel 400"],
    "three_device": ["# device_draw 1", "depth 3", "stream_create S3 flags 1 priority -1", "stream_create S4 flags 1 priority -1"],
    "three_seeded": ["# device_draw 0", "# n_cand 400 n_sel 50"],
    "mapping": ["kp_map_scan_kernel", "map_points_kernel", "# n_valid 400 n_cand_map 400", "obs_filter_kernel", "!map_append_points_kernel"],
    "mapping_map": ["map_append_kernel", "map_append_points_kernel"],
    "motion_device": ["motion_input_kernel", "pose_exp_compose_kernel"],
    "flow8_aligned_device": ["convex_upsample_kernel<0, 1, 2, false>", "frontend_epilogue_kernel", "kp_nms_kernel<false>"],
    "flow8_unpadded_device": ["convex_upsample_kernel<0, 1, 2, true>"],
    "unpadded_device": ["kp_nms_kernel<true>", "!convex_upsample_kernel"],
    "nocov_depth_random": ["frontend_epilogue_partial_kernel", "backend_front_kernel<4,"],
    "nocov_depth_nodepth": ["frontend_epilogue_partial_kernel", "kp_nms_kernel<false>"],
    "nocov_both_random": ["frontend_epilogue_partial_kernel", "backend_front_kernel<4,"],
    "nocov_match_grid": ["frontend_epilogue_partial_kernel", "backend_front_kernel<5,"],
    "full_device": ["kp_nms_kernel<false>", "kp_finish_kernel<1024, 16, 5, true>"],
    "random_device": ["backend_front_kernel<4,", "!kp_nms_kernel"],
    "random_host": ["backend_front_kernel<3,", "!kp_nms_kernel"],
    "grid": ["backend_front_kernel<5,", "!kp_nms_kernel"],
    "explicit_host": ["backend_front_kernel<3,", "!kp_nms_kernel"],
    "explicit_dev": ["backend_front_kernel<3,", "!kp_nms_kernel"],
    "exact_device": ["corr_volume_f32_chw", "!volume_pack_kernel"],
    "split3_hwc": ["split3_kernel", "corr_volume_bf16x3_hwc<3>"],
    "split2_hwc": ["split3_kernel", "corr_volume_bf16x3_hwc<2>"],
    "bf16x3": ["volume_pack_kernel<3, false>", "corr_volume_split_stream<3, false"],
    "f16x2_uncovered": ["corr_volume_f32_chw", "!volume_pack_kernel"],
    "f16x2_tiled": ["volume_tiled 1", "corr_lookup_tiled_kernel<2, 16, float>"],
    "enc16_tiled": ["volume_tiled 1", "fmap_tile_rows16_kernel", "corr_volume_h_stream", "corr_lookup_tiled_kernel<2, 16, half>"],
    "enc16_tiled_padded": ["volume_tiled 1", "fmap_tile_rows16_kernel", "corr_lookup_tiled_kernel<2, 16, half>"],
    "enc16_rows": ["volume_tiled 0", "corr_volume_h_stream", "corr_lookup_kernel<4, 2, 16, half>", "!fmap_tile_rows16_kernel"],
    "enc16_untileable": ["volume_tiled 0", "corr_lookup_kernel<4, 2, 16, half>"],
    "enc16_small_fp32_cells": ["volume_tiled 0", "corr_lookup_kernel<4, 2, 16, float>"],
    "map_one_device": ["map_append_kernel"],
    "map_lanes_device": ["map_append_lanes_kernel", "map_set_pose_lanes_kernel"],
    "skip_one_device": ["map_skip_kernel", "pgo_solve_kernel<1, 132>"],
    "skip_lanes_device": ["map_skip_lanes_kernel"],
    "skip_one_five_launch": ["map_skip_kernel", "pose_apply_kernel", "kp_front_kernel", "match_cov_kernel", "obs_filter_kernel"],
    "one_device_timed_detail": ["# timeline 4", "# timeline_backend 4", "# volume_times 4", "# volume_starts 4"],
    "one_device_timed_pairs": ["# timeline 0", "# timeline_backend 0", "# volume_times 4"],
    "one_device_SELECTOR_ON_own": ["stream_create S5 flags 1 priority -1", "kp_nms_kernel<true> grid(2,4) block(64,4) lds 0\nlaunch S5 kp_finish"],
    "one_device_SELECTOR_ON_vol": ["launch S1 kp_nms_kernel"],
    "one_device_SELECTOR_ON_back": ["launch S3 kp_nms_kernel", "!launch S2 kp_nms_kernel"],
    "one_device_LOOKUPS_ON_vol": ["launch S1 corr_lookup_kernel"],
    "one_device_PACK_ON_back": ["launch S4 volume_pack_kernel"],      # (the round-5 layout: backend and solve share a stream)
    "three_device_PACK_ON_back": ["launch S3 volume_pack_kernel"],
    "one_device_PACK_ON_main": ["launch S2 volume_pack_kernel"],
    "one_device_PACK_ON_side": ["launch S4 volume_pack_kernel"],
    "one_device_FREE_CUS_0": ["corr_volume_split_stream<2, true, 16, 4, true> grid(256)"],
    "one_device_FUSE_BACKEND_0": ["# device_draw 0", "kp_front_kernel", "pose_apply_kernel"],
    "one_device_DEVICE_DRAW_0": ["# device_draw 0"],
    "one_device_TILED_1": ["volume_tiled 1"],
    "one_device_LAYOUT_classic": ["depth 2", "stream_create S3 flags 1 priority -1"],
}


@pytest.mark.parametrize("name", list(BRANCHES))
def test_scenario_takes_its_branch(name):
    text = FIXTURES[name][1]
    for needle in BRANCHES[name]:
        assert (needle[1:] not in text) if needle.startswith("!") else (needle in text), (name, needle)


def _launches(text: str) -> collections.Counter:
    return collections.Counter(line.split(" ", 2)[2] for line in text.splitlines() if line.startswith("launch "))   # (kernel and geometry; not the stream)


@pytest.mark.parametrize("name", ["one_device", "one_perm", "one_seeded", "mapping", "one_perm_SELECTOR_ON_late_depth3"])
def test_launch_thread_issues_the_same_launches(tracer, name):
    """async_backend = 1: the interleaving is timing-dependent by design; the run succeeds and launches the same kernels."""
    assert _launches(trace(tracer, name, launch_thread=True)) == _launches(FIXTURES[name][1])


def test_driver_under_sanitizers():
    """frame_pipe.hip's host code with -fsanitize=address,undefined in the same stand-alone program: clean exits (no report, no leak), launch thread off and on."""
    exe = build(sanitized=True)
    try:
        for name in ("one_device", "three_seeded", "mapping_map"):
            assert trace(exe, name) == FIXTURES[name][1]
            assert _launches(trace(exe, name, launch_thread=True)) == _launches(FIXTURES[name][1])
    finally:
        os.remove(exe)
        for f in glob.glob(os.path.join(_out_dir(), f"frame_pipe_asan.{os.getpid()}.o")):
            os.remove(f)


if __name__ == "__main__":
    exe = build()
    try:
        if sys.argv[1:] == ["--write"]:
            groups, traces = collections.OrderedDict(), collections.OrderedDict()
            for group, name in scenario_list(exe):
                t = trace(exe, name)
                lines = t.splitlines()
                near = sorted(traces, key=lambda o: -difflib.SequenceMatcher(None, traces[o].splitlines(), lines, autojunk=False).quick_ratio())[:8]
                d, like = min(((delta(traces[o], t), o) for o in near), key=lambda x: len(x[0]), default=(t, None))
                if len(d) < 0.8 * len(t):   # (a trace that differs from every other in most lines reads better whole)
                    assert patched(traces[like], d) == t
                    groups.setdefault(group, []).append(f"### {name} ~ {like}\n{d}")
                else:
                    groups.setdefault(group, []).append(f"### {name}\n{t}")
                traces[name] = t
            for group, sections in groups.items():
                with open(os.path.join(GOLDEN, f"frame_pipe_trace_{group}.txt"), "w") as f:
                    f.write("".join(sections))
        elif sys.argv[1:] == ["--list"]:
            print("\n".join(" ".join(gn) for gn in scenario_list(exe)))
        else:
            sys.stdout.write(trace(exe, sys.argv[1], "--async" in sys.argv[2:]))
    finally:
        os.remove(exe)
