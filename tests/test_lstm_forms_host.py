"""The buffer-form rules of the LSTM update (csrc/lstm_forms.h: which form a dgates / stash buffer holds, who may read it, what a
failed call leaves behind) are host code without a HIP dependency: tests/host/lstm_forms_check.cpp asserts them, built here with
the ROCm clang++ under AddressSanitizer + UBSan and run as a child process.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd", "csrc")
CLANGS = ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")


def test_lstm_forms_rules_under_sanitizers(tmp_path):
    clang = next((c for c in CLANGS if os.path.exists(c)), None)
    if clang is None:
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "lstm_forms_check")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "host", "lstm_forms_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
