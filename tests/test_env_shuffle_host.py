"""CPU: the host side of shuffled env-sequence minibatches -- VecPPOTrainer(shuffle_envs=True)'s refusals, the new C-ABI
symbol uav_gather_rows_multi in the header, the built library and the ctypes table, and the config switch.  The kernel and the
trainer's update are checked on the GPU (tests/test_gpu_env_shuffle.py)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYMBOL = "uav_gather_rows_multi"


def test_refused_combinations_are_raised_before_anything_is_built():
    """No device is touched before these checks (they run on a host without a GPU)."""
    from uavppo.trainer import VecPPOTrainer
    with pytest.raises(ValueError, match="shuffle_envs and minibatch_rows"):
        VecPPOTrainer(8, 32, "mlp", minibatch_rows=100, shuffle_envs=True)
    with pytest.raises(ValueError, match="nothing to shuffle"):
        VecPPOTrainer(8, 32, "lstm", hidden=64, shuffle_envs=True)
    with pytest.raises(ValueError, match="nothing to shuffle"):
        VecPPOTrainer(8, 32, "mlp", num_minibatches=1, shuffle_envs=True)
    with pytest.raises(ValueError, match="divisible by num_minibatches"):         # the neighbouring check still holds beside it
        VecPPOTrainer(8, 32, "lstm", hidden=64, num_minibatches=3, shuffle_envs=True)


def test_gail_trainer_inherits_the_keyword():
    from uavppo.gail import GAILTrainer
    with pytest.raises(ValueError, match="nothing to shuffle"):
        GAILTrainer(8, 32, "mlp", shuffle_envs=True)


def test_symbol_is_in_header_library_and_ctypes_table():
    from uavppo import _lib
    header = open(os.path.join(ROOT, "include", "uavppo.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % SYMBOL, code, flags=re.S)
    assert m, "not declared in include/uavppo.h"
    n_params = len(m.group(1).split(","))
    # its header comment carries the two promises: the version stays, a bad index is clamped
    comment = header[:header.index("int " + SYMBOL)].rsplit("/*", 1)[1]
    assert "Added without a change of UAV_ABI_VERSION (a symbol only)" in " ".join(comment.split())
    assert "clamped" in comment
    assert int(re.search(r"#define UAV_ABI_VERSION (\d+)", header).group(1)) == 9
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s\b" % SYMBOL, out), "not exported by the built library"
    assert SYMBOL in _lib.SIGNATURES and len(_lib.SIGNATURES[SYMBOL][1]) == n_params
    assert _lib.lib().uav_abi_version() == 9
    # struct uav_gather_spec: the ctypes mirror has the header's fields in the header's order
    body = re.search(r"typedef struct uav_gather_spec \{(.*?)\}", code, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == [f[0] for f in _lib.GatherSpec._fields_]
    assert int(re.search(r"#define UAV_GATHER_MAX_SPECS (\d+)", code).group(1)) == _lib.GATHER_MAX_SPECS == 12


def test_library_refuses_bad_arguments_without_a_device():
    """The argument checks come before the launch: NULL handle, and the wrapper's own checks need no GPU either."""
    import ctypes as C
    import torch
    from uavppo import _lib, ops
    specs = (_lib.GatherSpec * 1)()
    assert _lib.lib().uav_gather_rows_multi(None, None, 1, 1, specs, 1, None) != 0
    assert b"uav_gather_rows_multi" in _lib.lib().uav_last_error()
    assert C.sizeof(_lib.GatherSpec) == 48
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        ops.gather_rows_multi(torch.zeros(2, dtype=torch.int32), [(torch.zeros(4, 3), torch.zeros(2, 3))])


def test_config_switch_exists_and_is_off():
    import importlib
    config = importlib.import_module("config")
    assert config.SHUFFLE_ENVS is False
