"""CPU: the host side of the update diagnostics and the KL-target early stop -- defaults off, the ctypes row, the pure function
that turns per-epoch sums into the diagnostics dict (with its stop decision), target_kl validation, the update_diagnostics.csv
rows, and what tests/test_gpu_ppo_diag.py assumes about its inputs (tests/_ppo_diag_check.py)."""
import inspect
import math

import numpy as np
import pytest

import _ppo_diag_check as dc


def test_defaults_are_off():
    import config
    from uavppo.gail import GAILTrainer
    from uavppo.trainer import VecPPOTrainer
    assert config.PPO_DIAGNOSTICS is False and config.TARGET_KL is None
    sig = inspect.signature(VecPPOTrainer.__init__).parameters
    assert sig["diagnostics"].default is False and sig["target_kl"].default is None
    assert inspect.signature(GAILTrainer.__init__).parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD     # inherits both


def test_ctypes_row_and_constants():
    from uavppo import _lib, ops
    res, args = _lib.SIGNATURES["uav_set_ppo_diag"]
    assert len(args) == 2 and res is _lib.I32
    assert ops.PPO_DIAG_N == 8 == len(ops.PPO_DIAG_NAMES) and ops.PPO_DIAG_NAMES == dc.NAMES
    assert hasattr(_lib.lib(), "uav_set_ppo_diag")
    header = open(_lib.os.path.join(_lib._HERE, "..", "..", "include", "uavppo.h")).read()
    assert "#define UAV_PPO_DIAG_N 8" in header
    for k, name in enumerate(("KL_K1", "KL_K3", "CLIPPED", "VCLIPPED", "VERR2", "RET", "RET2", "COUNT")):
        assert f"#define UAV_PPO_DIAG_{name} {k}\n" in header


def _row(n, kl3, kl1=0.0, clipped=0, vclipped=0, ret=None, V=None):
    ret = np.linspace(-1, 1, n) if ret is None else np.asarray(ret, float)
    V = np.zeros(n) if V is None else np.asarray(V, float)
    return [kl1 * n, kl3 * n, clipped, vclipped, ((ret - V) ** 2).sum(), ret.sum(), (ret * ret).sum(), n]


def test_diagnostics_from_hand_made_sums():
    from uavppo.trainer import diagnostics_from_sums
    ret = np.array([1.0, 2.0, 3.0, 6.0])
    V = np.array([1.5, 2.0, 2.0, 5.0])
    sums = [_row(4, 0.01, kl1=-0.02, clipped=1, vclipped=3, ret=ret, V=V), _row(4, 0.04, ret=ret, V=ret), [0.0] * 8]
    d = diagnostics_from_sums(sums, epochs_run=2)
    assert d["epochs_run"] == 2 and d["stopped_early"] is True                 # 2 of 3 planned epochs
    assert d["approx_kl"] == pytest.approx([0.01, 0.04]) and d["approx_kl_k1"] == pytest.approx([-0.02, 0.0])
    assert d["clip_fraction"] == [0.25, 0.0] and d["value_clip_fraction"] == [0.75, 0.0]
    want_ev = 1.0 - ((ret - V) ** 2).sum() / ((ret - ret.mean()) ** 2).sum()
    assert d["explained_variance"] == pytest.approx([want_ev, 1.0])
    full = diagnostics_from_sums(sums[:2], epochs_run=2)
    assert full["stopped_early"] is False and full["approx_kl"] == d["approx_kl"]


def test_constant_returns_give_nan_explained_variance():
    from uavppo.trainer import diagnostics_from_sums
    for c in (0.0, 1.0, 0.1, -37.25, 1e-3):
        d = diagnostics_from_sums([_row(1000, 0.01, ret=np.full(1000, np.float32(c)), V=np.zeros(1000))], epochs_run=1)
        assert math.isnan(d["explained_variance"][0]), c
    d = diagnostics_from_sums([_row(1, 0.01, ret=[2.0], V=[0.0])], epochs_run=1)          # one sample has no variance either
    assert math.isnan(d["explained_variance"][0])


def test_the_stop_decision():
    from uavppo.trainer import diagnostics_from_sums, kl_stop
    assert kl_stop(_row(8, 0.0101), 0.01) and not kl_stop(_row(8, 0.0099), 0.01)
    assert not kl_stop([0, 0.08, 0, 0, 0, 0, 0, 8], 0.01)                     # equal is not greater: no hidden factor
    assert kl_stop([0, 0.081, 0, 0, 0, 0, 0, 8], 0.01)
    assert not kl_stop(_row(8, 1e9), None)                                     # no target: never
    assert not kl_stop([0, float("nan"), 0, 0, 0, 0, 0, 8], 0.01)              # a NaN estimate does not stop (losses() reports it)
    assert kl_stop([0, float("inf"), 0, 0, 0, 0, 0, 8], 0.01)
    # walked in order: the epochs up to and including the first one over the target
    sums = [_row(8, k) for k in (0.001, 0.004, 0.02, 0.5, 0.9)]
    d = diagnostics_from_sums(sums, target_kl=0.01)
    assert d["epochs_run"] == 3 and d["stopped_early"] and d["approx_kl"] == pytest.approx([0.001, 0.004, 0.02])
    d = diagnostics_from_sums(sums, target_kl=1e30)
    assert d["epochs_run"] == 5 and not d["stopped_early"]
    d = diagnostics_from_sums(sums[:2] + [[0.0] * 8] * 3)                     # rows without samples: epochs that did not run
    assert d["epochs_run"] == 2 and d["stopped_early"]


@pytest.mark.parametrize("bad", [0, 0.0, -0.01, float("inf"), float("-inf"), float("nan"), "0.01", True])
def test_target_kl_is_validated(bad):
    from uavppo.trainer import VecPPOTrainer, check_target_kl
    with pytest.raises(ValueError, match="target_kl"):
        check_target_kl(bad)
    with pytest.raises(ValueError, match="target_kl"):        # refused before the trainer touches a device
        VecPPOTrainer(8, 16, "mlp", device="cuda:0", target_kl=bad)


def test_target_kl_accepts_positive_finite_numbers():
    from uavppo.trainer import check_target_kl
    assert check_target_kl(None) is None
    assert check_target_kl(0.015) == 0.015 and check_target_kl(1) == 1.0 and check_target_kl(np.float32(0.5)) == 0.5
    assert check_target_kl(1e30) == 1e30


def test_update_log_rows(tmp_path):
    from uavppo import update_log as ul
    diag = {"approx_kl": [1e-9, 0.02], "approx_kl_k1": [0.0, -0.01], "clip_fraction": [0.0, 0.125], "value_clip_fraction": [0.0, 0.5],
            "explained_variance": [0.1, 0.25], "epochs_run": 2, "stopped_early": True}
    assert ul.path_beside(str(tmp_path / "sub" / "training_results2_0.csv")) == str(tmp_path / "sub" / "update_diagnostics.csv")
    assert ul.path_beside(None) is None
    log = ul.UpdateDiagnosticsLog(ul.path_beside(str(tmp_path / "training.csv")))
    assert log.add(1, diag) == [1, 2, 0.02, -0.01, 0.125, 0.5, 0.25]
    log.add(2, dict(diag, epochs_run=1, approx_kl=[0.5]))
    log.close()
    lines = open(tmp_path / "update_diagnostics.csv").read().splitlines()
    assert lines[0] == "Iteration,Epochs_Run,Approx_Kl,Approx_Kl_K1,Clip_Fraction,Value_Clip_Fraction,Explained_Variance"
    assert lines[1] == "1,2,0.02,-0.01,0.125,0.5,0.25" and lines[2].startswith("2,1,0.5,") and len(lines) == 3
    assert "kl 2.000e-02" in ul.progress_text(diag) and "epochs 2" in ul.progress_text(diag)
    assert ul.UpdateDiagnosticsLog(None).add(3, diag)[0] == 3               # no path: kept in memory only


# ---------------------------------------------------------------------------------------------- the GPU tests' inputs
@pytest.fixture(scope="module")
def cases():
    return {k: f() for k, f in dc.CASES.items()}


def test_no_sample_of_the_gpu_cases_is_near_a_clip_boundary(cases):
    """The counts are compared EXACTLY on the GPU: with every ratio and every |V - v_old| more than 1e-5 from its boundary (the
    kernels' f32 values are within ~1e-6 of these f64 ones) both sides must count the same samples."""
    for name, c in cases.items():
        assert c["margin"] > dc.MARGIN, (name, c["margin"])


def test_both_sides_of_both_clips_are_populated(cases):
    for name, c in cases.items():
        n = int(c["ref"][7])
        if n >= 4:
            assert min(c["sides"]) >= 1, (name, c["sides"])
    for name in ("heads_n1000", "from_y_h64", "from_y_h128"):
        c = cases[name]
        n = c["ref"][7]
        assert min(c["sides"]) >= 5, (name, c["sides"])
        assert 0.0 < c["ref"][1] / n < 0.01, (name, c["ref"][1] / n)         # the small-lr regime of the k3 estimator


def test_mean_abs_log_ratio_of_the_cases_is_about_0_05():
    rng = np.random.RandomState(0)
    logits, value = rng.randn(20000, 5).astype(np.float32), rng.randn(20000).astype(np.float32)
    act, lpo, _, _, _ = dc.draw_samples(rng, logits, value)
    lr = dc.logp_f64(logits, act) - lpo
    assert 0.04 < np.abs(lr).mean() < 0.06


def test_restatement_on_a_hand_made_sample():
    logits = np.log(np.array([[0.5, 0.25, 0.25]]))
    s = dc.diag_sums(logits, [1.0], [0], [math.log(0.4)], [3.0], [0.5])
    lr = math.log(0.5) - math.log(0.4)
    assert s == pytest.approx([-lr, math.expm1(lr) - lr, 1.0, 1.0, 4.0, 3.0, 9.0, 1.0], rel=1e-12)      # ratio 1.25 > 1.2; |dV| 0.5 > 0.2
    assert s[1] > 0
