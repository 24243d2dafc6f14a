"""The block form of the operator entry points (pk_apply_operator_block[_dev], pockit_amd/csrc/pk_ops.cpp: the walk of
pk_op_rows_k / pk_op_long_k in chunks of columns, leading dimensions, refusals, the host form's scratch, tear-down) built with
``-fsanitize=address,undefined`` against the host-only stand-in of the HIP runtime and driven by
tests/fake_hip/ops_block_driver.cpp, and the Python surface that needs no device.  CPU only."""
import os
import shutil
import subprocess

import pytest

from pockit_amd import runtime
from pockit_amd.evaluator import Evaluator, Linearization
from sanitized_build import sanitized_driver


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_block_entry_points_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main): nothing sanitized is loaded into Python."""
    exe = sanitized_driver("ops_block_driver.cpp", tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


def test_the_python_surface_of_the_block_product():
    import ctypes as C

    assert runtime.PROTOTYPES["pk_apply_operator_block_dev"][1][3] is C.c_int32
    assert runtime.PROTOTYPES["pk_apply_operator_block_dev"][1][5] is C.c_int64 and runtime.PROTOTYPES["pk_apply_operator_block_dev"][1][8] is C.c_int64
    assert runtime.PROTOTYPES["pk_apply_operator_block"][1][2] is C.c_int32
    assert callable(Evaluator.apply_operator_block_dev)
    for name in ("jmat", "jtmat", "hmat"):
        assert callable(getattr(Linearization, name))
