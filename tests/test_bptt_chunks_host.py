"""CPU: the host side of truncated BPTT -- the C-ABI symbol uav_lstm_chunk_states in the header, the built library and the
ctypes table, chunk_plan's arithmetic and refusals, VecPPOTrainer(bptt_len=...) refusing before it touches a device, and the
config switch.  The kernel and the trainer's update are checked on the GPU (tests/test_gpu_bptt_chunks.py)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYMBOL = "uav_lstm_chunk_states"


def test_symbol_is_in_header_library_and_ctypes_table():
    from uavppo import _lib
    header = open(os.path.join(ROOT, "include", "uavppo.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % SYMBOL, code, flags=re.S)
    assert m, "not declared in include/uavppo.h"
    n_params = len(m.group(1).split(","))
    assert n_params == 13
    comment = " ".join(header[:header.index("int " + SYMBOL)].rsplit("/*", 1)[1].split())
    assert "Added without a change of UAV_ABI_VERSION (a symbol only)" in comment
    assert "already multiplied by keep" in comment
    assert int(re.search(r"#define UAV_ABI_VERSION (\d+)", header).group(1)) == 9
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s\b" % SYMBOL, out), "not exported by the built library"
    assert SYMBOL in _lib.SIGNATURES and len(_lib.SIGNATURES[SYMBOL][1]) == n_params
    assert _lib.lib().uav_abi_version() == 9


def test_library_refuses_a_null_handle_without_a_device():
    from uavppo import _lib
    assert _lib.lib().uav_lstm_chunk_states(None, None, None, None, None, None, 1, 4, 4, 2, None, None, None) != 0
    assert SYMBOL.encode() in _lib.lib().uav_last_error()


def test_chunk_plan_cuts_the_buffer_into_chunk_rows():
    from uavppo.trainer import chunk_plan
    assert chunk_plan(8, 24, 2, 8) == (3, 12)
    assert chunk_plan(8, 24, 1, 24) == (1, 8)             # one chunk per env: full BPTT
    assert chunk_plan(20, 32, 4, 8) == (4, 20)
    assert chunk_plan(5, 12, 4, 3) == (4, 5)              # N is no multiple of M, N * C is: allowed with bptt_len
    assert chunk_plan(7, 6, 1, 1) == (6, 42)


@pytest.mark.parametrize("args,kw,reason", [((8, 24, 2, 7), {}, "does not divide the horizon"),
                                            ((8, 24, 2, 48), {}, "longer than the horizon"),
                                            ((8, 24, 2, 0), {}, "at least 1"),
                                            ((8, 24, 2, -8), {}, "at least 1"),
                                            ((7, 24, 2, 8), {}, "not divisible by num_minibatches"),
                                            ((8, 24, 2, 8), {"policy": "mlp"}, "needs the LSTM policy"),
                                            ((8, 24, 1, 8), {"minibatch_rows": 64}, "bptt_len and minibatch_rows")])
def test_chunk_plan_refuses_with_a_reason(args, kw, reason):
    from uavppo.trainer import chunk_plan
    with pytest.raises(ValueError, match=reason):
        chunk_plan(*args, **kw)


def test_trainer_refuses_before_anything_is_built():
    """bptt_len is a named parameter now (the **hp catch-all used to swallow it): the checks run on a host without a GPU."""
    import inspect
    from uavppo.gail import GAILTrainer
    from uavppo.trainer import VecPPOTrainer
    assert inspect.signature(VecPPOTrainer.__init__).parameters["bptt_len"].default is None
    with pytest.raises(ValueError, match="does not divide the horizon"):
        VecPPOTrainer(8, 24, "lstm", hidden=64, bptt_len=7)
    with pytest.raises(ValueError, match="longer than the horizon"):
        VecPPOTrainer(8, 24, "lstm", hidden=64, bptt_len=25)
    with pytest.raises(ValueError, match="at least 1"):
        VecPPOTrainer(8, 24, "lstm", hidden=64, bptt_len=0)
    with pytest.raises(ValueError, match="not divisible by num_minibatches"):
        VecPPOTrainer(7, 24, "lstm", hidden=64, num_minibatches=2, bptt_len=8)
    with pytest.raises(ValueError, match="needs the LSTM policy"):
        VecPPOTrainer(8, 24, "mlp", bptt_len=8)
    with pytest.raises(ValueError, match="bptt_len and minibatch_rows"):
        VecPPOTrainer(8, 24, "mlp", minibatch_rows=64, bptt_len=8)
    with pytest.raises(ValueError, match="divisible by num_minibatches"):         # bptt_len = T: the whole-sequence rule holds
        VecPPOTrainer(7, 24, "lstm", hidden=64, num_minibatches=2, bptt_len=24)
    with pytest.raises(ValueError, match="does not divide the horizon"):          # GAILTrainer inherits the keyword
        GAILTrainer(8, 24, "lstm", hidden=64, bptt_len=7)


def test_config_switch_exists_and_is_off():
    import importlib
    config = importlib.import_module("config")
    assert config.BPTT_LEN is None
