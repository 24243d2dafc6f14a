"""The merit entry points (pk_set_bounds, pk_trial_points_dev, pk_merit_reduce_dev, pk_merit_batch_dev, pk_merit_scan,
pk_merit_batch; pockit_amd/csrc/pk_merit.cpp: the walk of pk_trial / pk_merit / pk_merit_fin, leading dimensions, refusals, the
partial rows and the scratch, tear-down) built with ``-fsanitize=address,undefined`` against the host-only stand-in of the HIP
runtime and driven by tests/fake_hip/merit_driver.cpp, and the Python surface that needs no device.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from pockit_amd import merit, runtime
from pockit_amd.evaluator import Evaluator
from pockit_amd.hipbuild import RUNTIME_SOURCES
from pockit_amd.model import SystemBase
from sanitized_build import sanitized_driver


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_merit_entry_points_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main): nothing sanitized is loaded into Python."""
    assert any(os.path.basename(s) == "pk_merit.cpp" for s in RUNTIME_SOURCES)
    exe = sanitized_driver("merit_driver.cpp", tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


def test_the_python_surface_of_the_merit_terms():
    P = runtime.PROTOTYPES
    assert len(P["pk_set_bounds"][1]) == 5
    assert P["pk_trial_points_dev"][1][1] is C.c_int and P["pk_trial_points_dev"][1][6] is C.c_int64
    assert [P["pk_merit_batch_dev"][1][k] for k in (4, 6, 8)] == [C.c_int64] * 3 and len(P["pk_merit_batch_dev"][1]) == 12
    assert P["pk_merit_scan"][1][1] is C.c_int64 and P["pk_merit_batch"][1][1] is C.c_int64 and P["pk_merit_batch"][1][3] is C.c_int64
    assert len(P["pk_merit_reduce_dev"][1]) == 18
    for name in ("set_bounds", "trial_points_dev", "merit_batch_dev", "merit_batch", "merit_scan"):
        assert callable(getattr(Evaluator, name))
    for name in ("merit_batch", "merit_scan"):
        assert callable(getattr(SystemBase, name)) and "viol" in SystemBase.merit_batch.__doc__


def test_merit_table_is_read_only_with_named_columns():
    assert merit.COLUMNS == ("f", "theta1", "theta_inf", "theta2_sq", "bound1", "bound_inf", "slope", "bad")
    raw = np.arange(24.0).reshape(3, 8)
    t = merit.MeritTable(raw)
    raw[0, 0] = -1.0                                   # (a copy: the caller's array is not the table)
    assert len(t) == 3 and t.table.shape == (3, 8) and t.table[0, 0] == 0.0
    for q, name in enumerate(merit.COLUMNS):
        assert np.array_equal(getattr(t, name), np.arange(3) * 8.0 + q)
    with pytest.raises(ValueError):
        t.table[0, 0] = 1.0
    with pytest.raises(ValueError):
        t.slope[0] = 1.0
    with pytest.raises(AttributeError):
        t.table = raw
    assert merit.MeritTable(np.empty((0, 8))).f.shape == (0,)
