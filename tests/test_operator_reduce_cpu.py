"""The runtime unit behind the row norms and weighted diagonals (pockit_amd/csrc/pk_reduce.cpp: the walk of pk_red_rows /
pk_red_long / pk_diag on the host stand-in, refusals, what drops the positions of the diagonal, tear-down) built with
``-fsanitize=address,undefined`` against the host-only stand-in of the HIP runtime and driven by tests/fake_hip/reduce_driver.cpp.
(That the unit leaves what the runtime enqueues elsewhere as tests/fake_hip/launch_trace.txt recorded it is
tests/test_runtime_sanitized.py's test of the launch shapes.)  CPU only."""
import os
import shutil
import subprocess

import pytest

from sanitized_build import sanitized_driver

ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_reduce_entry_points_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main): nothing sanitized is loaded into Python."""
    exe = sanitized_driver("reduce_driver.cpp", tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
