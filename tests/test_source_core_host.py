"""The source estimator's solve (csrc/source_solve.h: chol_solve<N>, the two closed forms, solve_core) is code without a HIP
dependency: tests/host/source_core_check.cpp runs it on the CPU, built here with the ROCm clang++ under AddressSanitizer + UBSan
and run as a child process.  The systems are the numpy statement's states of the twelve kinds of episodes / episodes6 (every status
among them); status, the Cholesky's verdict, its smallest pivot, a, mu and the widths use + - * / sqrt alone and must equal
source_fit.solve / source_aniso.solve6 bit for bit, theta, peak and strength (atan2, exp) within the tolerance of
tests/test_gpu_source_aniso.py.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from _source_aniso_cases import episodes6
from _source_fit_cases import episodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd", "csrc")
CLANGS = ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")
# exact: fit columns that go through + - * / sqrt alone; the others: (column, rtol, atol)
MODELS = {"iso": dict(n_phi=4, shapes=((257, 64, 6), (48, 24, 6)), cfgs=((5, 1e-6), (4, 1e-3)), exact=(0, 1, 2),
                      close=((3, 1e-9, 0.0), (4, 1e-9, 0.0))),
          "aniso": dict(n_phi=6, shapes=((257, 63, 6), (48, 80, 8)), cfgs=((8, 1e-6), (6, 1e-3)), exact=(0, 1, 2, 3),
                        close=((4, 0.0, 1e-9), (5, 1e-9, 0.0), (6, 1e-9, 0.0)))}


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    clang = next((c for c in CLANGS if os.path.exists(c)), None)
    if clang is None:
        pytest.skip("no ROCm clang++")
    out = str(tmp_path_factory.mktemp("source_core") / "source_core_check")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "host", "source_core_check.cpp"), "-o", out],
                   check=True)
    return out


def _states(model):
    from uavppo import source_aniso as sa, source_fit as sf
    out = []
    for n, k, D in MODELS[model]["shapes"]:
        ep = (episodes if model == "iso" else episodes6)(n, k, D)
        moments = sf.moments_chunk if model == "iso" else sa.moments_chunk6
        out.append(moments(ep["flags"], ep["obs"], ep["pos"], ep["state"], ep["ended"]))
    return np.concatenate(out)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_the_solve_on_the_cpu_is_the_numpy_statement(exe, tmp_path, model):
    from uavppo import source_aniso as sa, source_fit as sf
    M = MODELS[model]
    N = M["n_phi"]
    state = _states(model)
    width = 3 + N * (N + 1) // 2 + N                                      # count, centre, A, g: what the solve reads
    seen = set()
    for min_samples, min_pivot in M["cfgs"]:
        path = tmp_path / f"{model}_{min_samples}.txt"
        with open(path, "w") as f:
            f.write(f"{N} {state.shape[0]} {float(min_samples).hex()} {float(min_pivot).hex()}\n")
            for row in state[:, :width]:
                f.write(" ".join(float(v).hex() for v in row) + "\n")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]      # the sanitizers report nothing
        got = np.array([[float.fromhex(w) for w in line.split()] for line in r.stdout.splitlines()])
        solve = sf.solve if model == "iso" else sa.solve6
        want_est, want_status = solve(state, min_samples=min_samples, min_pivot=min_pivot)
        assert got.shape == (state.shape[0], 3 + N + want_est.shape[1] - 3)                 # status, solved, low | a | fit
        status, solved, low, a, fit = got[:, 0], got[:, 1] != 0, got[:, 2], got[:, 3:3 + N], got[:, 3 + N:]
        want_a, bad, want_low = sf.cholesky(state, min_pivot, sf.ISO if model == "iso" else sf.ANISO)
        assert np.array_equal(status, want_status)
        assert np.array_equal(solved, ~bad)
        assert np.array_equal(bits64(low), bits64(want_low))
        assert np.array_equal(bits64(a[solved]), bits64(want_a[solved]))
        fitted = want_status == 0
        assert np.isnan(fit[~fitted]).all() and np.isfinite(fit[fitted]).all()
        assert np.array_equal(bits64(fit[fitted][:, M["exact"]]), bits64(want_est[fitted][:, M["exact"]]))
        for j, rtol, atol in M["close"]:
            assert np.allclose(fit[fitted, j], want_est[fitted, j], rtol=rtol, atol=atol), j
        seen |= set(want_status)
    assert seen == {0, 1, 2, 3}
