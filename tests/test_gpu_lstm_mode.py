"""The arithmetic mode belongs to the handle, not to the thread: two handles on one device, one on the default fp16x3 and one on
f32_mfma, called alternately from one thread, each run their own kernels and report their own buffer sizes and capabilities
(include/uavppo.h: uav_set_lstm_arith, uav_set_debug_flags; csrc/lstm_forms.h: uav_lstm_mode).  -m gpu."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, I, N, T = 64, 6, 16, 8          # one workgroup (16 envs), one x chunk (8 steps) of the persistent h = 64 kernel
# include/uavppo.h, uav_lstm_dgates_bytes at N = 64, T = 2, H = 256.  DgPack(64, 2): NP = 64, RT = 4 row tiles, NS = 32 slabs of
# 1024 halves -> pieces 2 * (4 * 32 * 1024) * 2 bytes, + isc and iscm 2 * (2 * 64) floats; f32 rows: 64 * 2 * 1024 floats
PACKED_BYTES = 2 * (4 * 32 * 1024) * 2 + 2 * (2 * 64) * 4
ROWS_BYTES = 64 * 2 * 1024 * 4


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


def _inputs():
    g = torch.Generator().manual_seed(20)
    k = 1.0 / 8.0                                                   # nn.LSTM's 1 / sqrt(H)
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * k).to(DEV)
    x = torch.randn(N, T, I, generator=g).to(DEV)
    h0, c0 = (torch.randn(N, H, generator=g) * 0.5).to(DEV), (torch.randn(N, H, generator=g) * 0.5).to(DEV)
    return x, h0, c0, u(4 * H, I), u(4 * H, H), u(4 * H), u(4 * H)


def _fwd(ops, handle, x, h0, c0, w_ih, w_hh, b_ih, b_hh):
    """uav_lstm_fwd on `handle`: (y, hn, cn, stash) of this call, in fresh buffers."""
    p = lambda t: C.c_void_p(t.data_ptr())
    y, hn, cn, stash = (torch.zeros(*s, device=DEV) for s in ((N, T, H), (N, H), (N, H), (N, T, 6 * H)))
    ops.check(ops.lib().uav_lstm_fwd(handle, p(x), None, p(h0), p(c0), p(w_ih), p(w_hh), p(b_ih), p(b_hh), N, T, I, H, p(y), p(hn),
                                     p(cn), p(stash), None, None, 0, None, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "uav_lstm_fwd")
    return y, hn, cn, stash


def _bits_equal(a, b):
    return all(torch.equal(s.view(torch.int32), t.view(torch.int32)) for s, t in zip(a, b))


def test_two_handles_alternating_on_one_thread_keep_their_own_mode(ops):
    lib = ops.lib()
    A = ops.Context.get(DEV).handle                                 # the module's handle, on the default
    assert ops.get_lstm_arith(DEV) == "fp16x3"
    B = C.c_void_p()
    ops.check(lib.uav_create(C.byref(B), 0, 16 << 20), "uav_create")
    try:
        ops.check(lib.uav_set_lstm_arith(B, ops.ARITH["f32_mfma"]), "uav_set_lstm_arith")
        args = _inputs()
        # (a) A / B / A: each call runs the arithmetic of ITS handle
        a1 = _fwd(ops, A, *args)
        b1 = _fwd(ops, B, *args)
        a2 = _fwd(ops, A, *args)
        zeros = lambda: dict(y=torch.zeros(N, T, H, device=DEV), stash=torch.zeros(N, T, 6 * H, device=DEV))
        ref_a = ops.lstm_fwd(args[0], None, *args[1:], **zeros())
        with ops.lstm_arith("f32_mfma", DEV):
            ref_b = ops.lstm_fwd(args[0], None, *args[1:], **zeros())
        torch.cuda.synchronize()
        assert _bits_equal(a1, a2)
        assert _bits_equal(b1, ref_b)
        assert _bits_equal(a1, ref_a)
        assert not torch.equal(a1[0].view(torch.int32), b1[0].view(torch.int32)), "the two arithmetics agree bit for bit on y here"
        # (b), (c): nothing launched; what a handle reports follows its own mode whatever handle was used last
        assert lib.uav_lstm_dgates_bytes(A, 64, 2, 256) == PACKED_BYTES
        assert lib.uav_lstm_dgates_bytes(B, 64, 2, 256) == ROWS_BYTES
        assert lib.uav_lstm_dgates_bytes(A, 64, 2, 256) == PACKED_BYTES
        assert lib.uav_lstm_bwd_caps(A, 256, 256) == 7
        assert lib.uav_lstm_bwd_caps(B, 256, 256) == 0
        assert lib.uav_lstm_bwd_caps(A, 256, 256) == 7
        # (d) a debug flag of A is A's alone, and is gone when cleared
        try:
            ops.set_debug_flags("dg_f32", device=DEV)
            assert lib.uav_lstm_dgates_bytes(A, 64, 2, 256) == ROWS_BYTES
            assert lib.uav_lstm_bwd_caps(A, 256, 256) == 7 and lib.uav_lstm_bwd_caps(B, 256, 256) == 0
        finally:
            ops.set_debug_flags(device=DEV)
        assert lib.uav_lstm_dgates_bytes(A, 64, 2, 256) == PACKED_BYTES
    finally:
        torch.cuda.synchronize()
        lib.uav_destroy(B)
