"""Learning-rate and entropy schedules, the host side: the numpy definitions of uavppo/lr_control.py (adapt_rule, linear_value),
every refusal of check_lr_control, the header text and ctypes rows of the three new symbols, the config names, and the update
log's extra columns.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

from _lr_control_cases import D, F, HI, LO, TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "uavppo.h")
SLOT = {"lr": 0, "last_kl": 1, "raised": 2, "lowered": 3, "held": 4, "skipped": 5}


# ------------------------------------------------------------------------------------------------ 1: adapt_rule
@pytest.mark.parametrize("name,lr,s8,want_lr,slot", TABLE, ids=[c[0] for c in TABLE])
def test_adapt_rule_table(name, lr, s8, want_lr, slot):
    from uavppo.lr_control import adapt_rule, fresh_state
    new = adapt_rule(fresh_state(lr), s8, D, F, LO, HI)
    assert new.dtype == np.float64 and new.shape == (6,)
    assert new[0] == np.float64(want_lr), (new[0], want_lr)
    counts = {k: new[SLOT[k]] for k in ("raised", "lowered", "held", "skipped")}
    assert counts == {k: float(k == slot) for k in counts}
    if slot == "skipped":
        assert np.isnan(new[1])
    else:
        assert new[1] == s8[1] / s8[7]


def test_adapt_rule_keeps_counting_and_does_not_write_its_input():
    from uavppo.lr_control import adapt_rule
    state = np.array([3e-5, 0.5, 4.0, 3.0, 2.0, 1.0])
    before = state.copy()
    new = adapt_rule(state, TABLE[0][2], D, F, LO, HI)
    assert np.array_equal(state, before)
    assert new.tolist()[2:] == [4.0, 4.0, 2.0, 1.0] and new[1] == TABLE[0][2][1] / 1024


def test_forty_raises_end_exactly_at_lr_max_and_forty_lowerings_at_lr_min():
    from uavppo.lr_control import adapt_rule, fresh_state
    up = down = fresh_state(3e-5)
    for _ in range(40):
        up = adapt_rule(up, TABLE[1][2], D, F, LO, HI)
        down = adapt_rule(down, TABLE[0][2], D, F, LO, HI)
    assert up[0] == HI and up[SLOT["raised"]] == 40.0
    assert down[0] == LO and down[SLOT["lowered"]] == 40.0


# ------------------------------------------------------------------------------------------------ 2: linear_value
def test_linear_value():
    from uavppo.lr_control import linear_value
    assert linear_value(3e-5, 1e-6, 0, 10) == np.float64(3e-5)
    assert linear_value(3e-5, 1e-6, 10, 10) == np.float64(3e-5) + (np.float64(1e-6) - np.float64(3e-5)) * 10.0 / 10.0
    assert linear_value(3e-5, 1e-6, 25, 10) == linear_value(3e-5, 1e-6, 10, 10)
    assert abs(linear_value(3e-5, 1e-6, 10, 10) - 1e-6) < 1e-20
    v = linear_value(0.01, 0.0, 3, 4)
    assert isinstance(v, np.float64) and v == np.float64(0.01) + (np.float64(0.0) - np.float64(0.01)) * 3.0 / 4.0
    assert abs(v - 0.0025) < 1e-17
    assert linear_value(2.0, 4.0, 1, 2) == 3.0 and linear_value(4.0, 2.0, 1, 4) == 3.5


# ------------------------------------------------------------------------------------------------ 3: refusals
GOOD_ADAPTIVE = dict(lr_schedule="adaptive", desired_kl=0.01, optimiser_steps=5)
REFUSED = [
    ("unknown schedule", dict(lr_schedule="cosine")),
    ("linear without schedule_iterations", dict(lr_schedule="linear", lr_final=1e-6)),
    ("linear with schedule_iterations=0", dict(lr_schedule="linear", lr_final=1e-6, schedule_iterations=0)),
    ("linear with a fractional schedule_iterations", dict(lr_schedule="linear", lr_final=1e-6, schedule_iterations=2.5)),
    ("linear without lr_final", dict(lr_schedule="linear", schedule_iterations=10)),
    ("linear with a negative lr_final", dict(lr_schedule="linear", lr_final=-1e-6, schedule_iterations=10)),
    ("lr_final without linear", dict(lr_final=1e-6, schedule_iterations=10)),
    ("ent_beta_final without schedule_iterations", dict(ent_beta_final=0.0)),
    ("ent_beta_final with schedule_iterations=-1", dict(ent_beta_final=0.0, schedule_iterations=-1)),
    ("ent_beta_final NaN", dict(ent_beta_final=float("nan"), schedule_iterations=10)),
    ("adaptive without desired_kl", dict(lr_schedule="adaptive", optimiser_steps=5)),
    ("adaptive with desired_kl=0", dict(GOOD_ADAPTIVE, desired_kl=0.0)),
    ("adaptive with desired_kl=inf", dict(GOOD_ADAPTIVE, desired_kl=float("inf"))),
    ("adaptive with desired_kl NaN", dict(GOOD_ADAPTIVE, desired_kl=float("nan"))),
    ("adaptive with desired_kl a string", dict(GOOD_ADAPTIVE, desired_kl="0.01")),
    ("desired_kl without adaptive", dict(desired_kl=0.01)),
    ("lr_factor=1", dict(GOOD_ADAPTIVE, lr_factor=1.0)),
    ("lr_factor below 1", dict(GOOD_ADAPTIVE, lr_factor=0.5)),
    ("lr_factor NaN", dict(GOOD_ADAPTIVE, lr_factor=float("nan"))),
    ("lr_min=0", dict(GOOD_ADAPTIVE, lr_min=0.0)),
    ("lr_min negative", dict(GOOD_ADAPTIVE, lr_min=-1e-6)),
    ("lr_min above lr_max", dict(GOOD_ADAPTIVE, lr_min=1e-3, lr_max=1e-4, lr=5e-4)),
    ("lr below lr_min", dict(GOOD_ADAPTIVE, lr=1e-7)),
    ("lr above lr_max", dict(GOOD_ADAPTIVE, lr=0.1)),
    ("adaptive with one optimiser step", dict(GOOD_ADAPTIVE, optimiser_steps=1)),
]


@pytest.mark.parametrize("name,kw", REFUSED, ids=[c[0] for c in REFUSED])
def test_check_lr_control_refuses(name, kw):
    from uavppo.lr_control import check_lr_control
    with pytest.raises(ValueError):
        check_lr_control(**kw)


def test_check_lr_control_accepts_and_returns_plain_values():
    from uavppo.lr_control import check_lr_control
    c = check_lr_control()
    assert c == dict(lr_schedule="constant", lr_final=None, ent_beta_final=None, schedule_iterations=None, desired_kl=None,
                     lr_factor=1.5, lr_min=1e-6, lr_max=1e-2)
    assert check_lr_control(lr=0.5)["lr_schedule"] == "constant"            # the bounds act under "adaptive" only
    c = check_lr_control("linear", lr_final=0, schedule_iterations=np.int64(7), ent_beta_final=np.float32(0.5))
    assert c["lr_final"] == 0.0 and c["schedule_iterations"] == 7 and type(c["schedule_iterations"]) is int and c["ent_beta_final"] == 0.5
    c = check_lr_control(**dict(GOOD_ADAPTIVE, optimiser_steps=2, lr_min=3e-5, lr_max=3e-5))     # a pinned rate is allowed
    assert c["desired_kl"] == 0.01 and c["lr_min"] == c["lr_max"] == 3e-5


@pytest.mark.parametrize("kw", [dict(lr_schedule="cosine"), dict(lr_schedule="linear", lr_final=1e-6), dict(ent_beta_final=0.0),
                                dict(lr_schedule="adaptive"), dict(lr_schedule="adaptive", desired_kl=0.01, lr_factor=1.0),
                                dict(lr_schedule="adaptive", desired_kl=0.01, lr_min=0.0),
                                dict(lr_schedule="adaptive", desired_kl=0.01, lr_min=1e-3, lr_max=1e-4),
                                dict(lr_schedule="adaptive", desired_kl=0.01, lr=0.1),
                                dict(lr_schedule="adaptive", desired_kl=0.01, epochs=1),
                                dict(lr_factor=0.9), dict(lr_min=-1.0)])
def test_the_trainer_refuses_before_anything_is_allocated(kw):
    """ValueError, not the RuntimeError of a missing GPU: check_lr_control runs before the trainer touches a device."""
    from uavppo.trainer import VecPPOTrainer
    with pytest.raises(ValueError):
        VecPPOTrainer(8, 16, policy="mlp", **kw)


def test_the_keywords_are_off_by_default_and_gail_inherits_them():
    from uavppo.gail import GAILTrainer
    from uavppo.trainer import VecPPOTrainer
    p = inspect.signature(VecPPOTrainer.__init__).parameters
    want = dict(lr_schedule="constant", lr_final=None, ent_beta_final=None, schedule_iterations=None, desired_kl=None, lr_factor=1.5,
                lr_min=1e-6, lr_max=1e-2)
    assert {k: p[k].default for k in want} == want
    g = inspect.signature(GAILTrainer.__init__).parameters
    assert "lr_schedule" not in g and g["kw"].kind is inspect.Parameter.VAR_KEYWORD and "disc_lr" in g


# ------------------------------------------------------------------------------------------------ 4: header, ctypes, config
def test_header_text_and_ctypes_rows_of_the_three_symbols():
    from uavppo import _lib, ops
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, count in (("uav_clip_adam_dlr", 15), ("uav_lr_init", 5), ("uav_lr_adapt", 9)):
        m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == count == len(_lib.SIGNATURES[name][1]), name
        # the comment in front of the declaration says how the symbol arrived
        comment = text[:text.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert "Added without a change of UAV_ABI_VERSION (symbols only)." in " ".join(comment.split()), name
    assert "const float* lr_dev" in re.search(r"uav_clip_adam_dlr\s*\((.*?)\)", src, flags=re.S).group(1)
    adam = re.search(r"\buav_clip_adam\s*\((.*?)\)", src, flags=re.S).group(1)
    dlr = re.search(r"\buav_clip_adam_dlr\s*\((.*?)\)", src, flags=re.S).group(1)
    assert " ".join(adam.split()).replace("float lr,", "const float* lr_dev,") == " ".join(dlr.split())     # uav_clip_adam's list otherwise
    assert re.search(r"#define UAV_LR_STATE_N 6\b", text) and ops.LR_STATE_N == 6
    for i, nm in enumerate(ops.LR_STATE_NAMES):
        assert re.search(r"#define UAV_LR_STATE_%s %d\b" % (nm.upper(), i), text), nm
    assert re.search(r"#define UAV_ABI_VERSION 9\b", text) and _lib.lib().uav_abi_version() == 9


def test_config_names_and_defaults():
    import config
    assert config.LR_SCHEDULE == "constant" and config.LR_FINAL is None and config.ENTROPY_BETA_FINAL is None
    assert config.SCHEDULE_ITERATIONS is None and config.DESIRED_KL is None
    assert config.LR_FACTOR == 1.5 and config.LR_MIN == 1e-6 and config.LR_MAX == 1e-2
    assert config.LEARNING_RATE == 3e-5 and config.ENTROPY_BETA == 0.01
    src = open(config.__file__).read()
    for nm in ("LR_SCHEDULE", "LR_FINAL", "ENTROPY_BETA_FINAL", "SCHEDULE_ITERATIONS", "DESIRED_KL", "LR_FACTOR", "LR_MIN", "LR_MAX"):
        assert re.search(r"^%s = [^#\n]+#\s*\S" % nm, src, flags=re.M), nm        # one line, with its comment
    for script in ("train_ppo2.0.py", "train_ppo_gail.py"):
        s = open(os.path.join(os.path.dirname(config.__file__), script)).read()
        for kw in ("lr_schedule=LR_SCHEDULE", "lr_final=LR_FINAL", "ent_beta_final=ENTROPY_BETA_FINAL", "schedule_iterations=SCHEDULE_ITERATIONS",
                   "desired_kl=DESIRED_KL", "lr_factor=LR_FACTOR", "lr_min=LR_MIN", "lr_max=LR_MAX"):
            assert kw in s, (script, kw)


# ------------------------------------------------------------------------------------------------ 5: update log
DIAG = {"epochs_run": 3, "approx_kl": [0.001, 0.002, 0.0125], "approx_kl_k1": [0.0, 0.001, -0.5], "clip_fraction": [0.0, 0.1, 0.25],
        "value_clip_fraction": [0.0, 0.0, 0.5], "explained_variance": [0.1, 0.2, float("nan")]}


def test_update_log_without_extra_columns_is_byte_identical(tmp_path):
    from uavppo import update_log as ul
    assert ul.COLUMNS == ("Iteration", "Epochs_Run", "Approx_Kl", "Approx_Kl_K1", "Clip_Fraction", "Value_Clip_Fraction",
                          "Explained_Variance")
    log = ul.UpdateDiagnosticsLog(str(tmp_path / "a" / ul.FILE_NAME))
    assert log.add(1, DIAG)[:6] == [1, 3, 0.0125, -0.5, 0.25, 0.5]
    log.add(2, DIAG)
    log.close()
    want = ("Iteration,Epochs_Run,Approx_Kl,Approx_Kl_K1,Clip_Fraction,Value_Clip_Fraction,Explained_Variance\n"
            "1,3,0.0125,-0.5,0.25,0.5,nan\n2,3,0.0125,-0.5,0.25,0.5,nan\n")
    assert open(tmp_path / "a" / ul.FILE_NAME, "rb").read() == want.encode()
    with pytest.raises(ValueError):
        ul.UpdateDiagnosticsLog(None).add(1, DIAG, (3e-5, 0.01))


def test_update_log_with_extra_columns(tmp_path):
    from uavppo import update_log as ul
    assert ul.SCHEDULE_COLUMNS == ("Learning_Rate", "Entropy_Beta")
    log = ul.UpdateDiagnosticsLog(str(tmp_path / ul.FILE_NAME), extra_columns=ul.SCHEDULE_COLUMNS)
    assert log.add(1, DIAG, (3e-5, 0.01))[-2:] == [3e-5, 0.01]
    log.add(2, DIAG, (np.float64(2e-5), 0.0075))
    log.close()
    want = ("Iteration,Epochs_Run,Approx_Kl,Approx_Kl_K1,Clip_Fraction,Value_Clip_Fraction,Explained_Variance,Learning_Rate,Entropy_Beta\n"
            "1,3,0.0125,-0.5,0.25,0.5,nan,3e-05,0.01\n2,3,0.0125,-0.5,0.25,0.5,nan,2e-05,0.0075\n")
    assert open(tmp_path / ul.FILE_NAME).read() == want
    with pytest.raises(ValueError):
        ul.UpdateDiagnosticsLog(None, ul.SCHEDULE_COLUMNS).add(1, DIAG)
    mem = ul.UpdateDiagnosticsLog(None, ul.SCHEDULE_COLUMNS)
    mem.add(5, DIAG, (1e-3, 0.0))
    assert mem.rows[0][:2] == [5, 3] and mem.rows[0][-2:] == [1e-3, 0.0]
