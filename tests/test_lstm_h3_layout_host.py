"""The state layout of the h = 256 step path (csrc/lstm_h3.hip: H3Layout), pinned through the ABI: uav_lstm_stepper_bytes is the
layout's total, and the same record places the sequence forward's state at the tail of the workspace.  The sizes below are
hs, cs f32 [N][256] | two ping-pong sets of h pieces [2][NP][256] fp16 | W_hh pieces [2][1024][256] | W_ih pieces [2][1024][IP] |
b_ih + b_hh [1024] f32, with NP = N rounded up to 64 and IP = I rounded up to 32, 64, 128 or 256 -- worked out by hand from that
formula, not read back from the library.  No GPU."""
import pytest


def _bytes(N, I, H=256):
    from uavppo import _lib
    return int(_lib.lib().uav_lstm_stepper_bytes(N, I, H))


@pytest.mark.parametrize("N,I,want", [
    (1, 1, 1316864),          # one env in one 64-env tile, one input slab
    (5, 6, 1325056),
    (100, 8, 1650688),        # two env tiles
    (65, 40, 1710080),        # I = 40 -> two slabs
    (130, 100, 2236416),      # three env tiles, I = 100 -> four slabs
    (64, 256, 2363392),       # a whole tile, the widest input
])
def test_stepper_bytes_are_the_layout_total(N, I, want):
    NP, IP = (N + 63) // 64 * 64, next(p for p in (32, 64, 128, 256) if I <= p)
    assert want == 2 * N * 256 * 4 + 2 * (2 * NP * 256 * 2) + 2 * 1024 * 256 * 2 + 2 * 1024 * IP * 2 + 1024 * 4     # the table itself
    assert want % 256 == 0
    assert _bytes(N, I) == want


@pytest.mark.parametrize("N,I,H", [(64, 8, 128), (64, 8, 64), (64, 8, 512), (64, 257, 256), (64, 0, 256), (64, -3, 256), (0, 8, 256),
                                   (-1, 8, 256)])
def test_stepper_bytes_are_zero_for_unsupported_shapes(N, I, H):
    assert _bytes(N, I, H) == 0
