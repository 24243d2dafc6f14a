"""The batch entry points of the host runtime (pockit_amd/csrc/pk_batch.cpp: record copy, per-entry workspaces, error 97, the loop of
single cycles, refusals, tear-down) built with ``-fsanitize=address,undefined`` against the host-only stand-in of the HIP
runtime and driven by tests/fake_hip/batch_driver.cpp.  CPU only."""
import os
import shutil
import subprocess

import pytest

from pockit_amd.hipbuild import RUNTIME_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_hip")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_batch_entry_points_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "pk_batch_sanitized")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined", "-I", FAKE, "-I", ROOT] + RUNTIME_SOURCES + [
               os.path.join(FAKE, "fake_hip.cpp"), os.path.join(FAKE, "batch_driver.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
