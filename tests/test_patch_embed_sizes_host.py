"""`mv_cost_patch_embed_supported` is a host-only predicate: the slice sizes the fused cost patch embedding is instantiated for (no GPU needed)."""
import pytest


@pytest.mark.parametrize("H2,W2,want", [
    (47, 98, True), (48, 104, True),          # KITTI, 376 x 784 frames: the raw 1/8 slice and the one PatchEmbed.forward pads
    (60, 94, True), (64, 96, True),           # EuRoC, 480 x 752
    (60, 80, True), (64, 80, True), (80, 80, True), (90, 160, True), (96, 160, True),      # TartanAir: 640 x 480, 640 x 640, 1280 x 720
    (24, 32, False), (47, 104, False), (48, 98, False), (60, 96, False), (98, 47, False),  # sizes, not a run-time-shape kernel
])
def test_patch_embed_supported_sizes(H2, W2, want):
    from macvo_amd import ops

    assert ops.cost_patch_embed_supported(H2, W2) is want
