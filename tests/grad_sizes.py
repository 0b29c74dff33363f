"""TEST INFRASTRUCTURE: the image sizes at which the gradient-selector kernels (mac-vo_amd/csrc/kp_gradient.hip) change path, shared by the CPU and the
GPU suite, and the path each size reaches worked out from the kernels' own constants (read from the sources, so that a change of CHUNK, COMPACT_NT or
the tile size makes the tests say that they no longer cover what they name instead of silently passing beside it).

    tiles = ceil(H / TILE_H) * ceil(W / TILE_W)      kg_select_kernel adds the tile pairs in chunks of CHUNK: ceil(tiles / CHUNK) rounds of its loop
    words = H * ceil(W / 64)                         kg_compact_kernel: thread t owns per = ceil(words / COMPACT_NT) contiguous candidate words"""
from __future__ import annotations

import os
import re
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "mac-vo_amd", "csrc")


def _constant(file: str, name: str) -> int:
    with open(os.path.join(_CSRC, file)) as f:
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    assert m, f"{file}: constexpr int {name} not found"
    return int(m.group(1))


TILE_W, TILE_H = _constant("kp_grad_math.h", "TILE_W"), _constant("kp_grad_math.h", "TILE_H")
CHUNK, COMPACT_NT = _constant("kp_gradient.hip", "CHUNK"), _constant("kp_gradient.hip", "COMPACT_NT")


def paths(H: int, W: int) -> SimpleNamespace:
    """What the kernels do at H x W: tiles, chunks (rounds of the tile-sum loop), last (pairs of its last round), words, wpr (words per row), per (words
    per compaction thread), busy (compaction threads that own a word)."""
    wpr = -(-W // 64)
    tiles = -(-H // TILE_H) * -(-W // TILE_W)
    words = H * wpr
    per = -(-words // COMPACT_NT)
    chunks = -(-tiles // CHUNK)
    return SimpleNamespace(tiles=tiles, chunks=chunks, last=tiles - (chunks - 1) * CHUNK, words=words, wpr=wpr, per=per, busy=-(-words // per))


# Each the smallest size that reaches its path; `want` is asserted from H, W by check_path before a test relies on the size.
#   130 x 513    per = 2 with 9 words per row: odd, so a thread's pair straddles a row end; threads >= 585 own nothing; a row's last word holds 1 pixel
#   3840 x 65    480 tiles: one full chunk (cnt == CHUNK), no second round
#   3841 x 65    482 tiles: a second round of 2 pairs; the last tile row is 1 pixel high
#   7681 x 9     481 tiles in a single tile column (grid y = 481): a second round of 1 pair
#   376 x 1241   KITTI: 480 tiles, 7520 words, W % 64 = 25
LARGE = {(130, 513): dict(tiles=81, chunks=1, words=1170, wpr=9, per=2, busy=585), (3840, 65): dict(tiles=480, chunks=1, last=480, words=7680, per=8),
         (3841, 65): dict(tiles=482, chunks=2, last=2, words=7682, per=8), (7681, 9): dict(tiles=481, chunks=2, last=1, words=7681, wpr=1, per=8),
         (376, 1241): dict(tiles=480, chunks=1, last=480, words=7520, per=8)}
#   17 x 65: slivers of 1 row and 1 column; 16 x 64: one tile exactly; 5 x 300: lower than the NMS radius of nms_size 15
SMALL = {(17, 65): dict(tiles=4, per=1), (16, 64): dict(tiles=1, per=1), (5, 300): dict(tiles=5, per=1)}
#   smaller than any border; 1 x 1 has n - 1 = 0: a finite mean, NaN standard deviation and threshold (as torch)
TINY = {(3, 3): dict(tiles=1, words=3), (2, 2): dict(tiles=1, words=2), (1, 1): dict(tiles=1, words=1)}
TABLE = {**LARGE, **SMALL, **TINY}


def check_path(H: int, W: int) -> SimpleNamespace:
    p = paths(H, W)
    for k, v in TABLE[(H, W)].items():
        assert getattr(p, k) == v, f"{H} x {W} no longer reaches its path: {k} = {getattr(p, k)}, the table says {v} (CHUNK {CHUNK}, COMPACT_NT {COMPACT_NT}, " \
                                   f"tile {TILE_H} x {TILE_W})"
    if (H, W) == (130, 513):
        assert p.wpr % p.per == 1 and W % 64 == 1 and p.busy < COMPACT_NT       # a thread's words straddle a row end; idle tail threads; a 1-pixel word
    if p.chunks == 1 and TABLE[(H, W)].get("last") == 480:
        assert p.tiles == CHUNK                                                  # the exact fit
    return p


def mask_width_for(H: int, W: int) -> int:
    return 8 if min(H, W) >= 20 else 1
