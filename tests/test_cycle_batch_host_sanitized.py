"""The batch entry points of the host runtime (pockit_amd/csrc/pk_batch.cpp: record copy, per-entry workspaces, error 97, the loop of
single cycles, refusals, tear-down) built with ``-fsanitize=address,undefined`` against the host-only stand-in of the HIP
runtime and driven by tests/fake_hip/batch_driver.cpp.  CPU only."""
import os
import shutil
import subprocess

import pytest

from sanitized_build import sanitized_driver


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_batch_entry_points_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = sanitized_driver("batch_driver.cpp", tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
