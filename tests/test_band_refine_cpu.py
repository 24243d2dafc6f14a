"""The refinement of the band solve (pockit_amd/csrc/pk_band_refine.cpp: pk_bd_resid_k, pk_bd_refine_scalar_k, pk_bd_correct_k and the
entry points around them) built with ``-fsanitize=address,undefined`` against the host-only stand-in of the HIP runtime and driven
by tests/fake_hip/band_refine_driver.cpp: the stand-in walk of the three kernels against plain loops at the lengths 1, 2, 255,
256, 257, 2047, 2048, 2049 and 524 289, NaN at every element that is no unknown, planted NaN and infinities, the decision in its
order, the planned forms against their own composition, the freeze rule, the refusals with their codes and sentinels, what frees
the state.  With ``--dump`` the five systems of tests/band_refine_cases.py compared BIT FOR BIT with its emulator after every
step.  CPU only; a stand-alone program (its own main): nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import band_cases as bc
import band_refine_cases as br
from sanitized_build import sanitized_driver

ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
TABLE_TOL = 1.0e-14      # (tests/test_band_refine_cases_cpu.py: the bound the repaired rows are held to)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sanitized_driver("band_refine_driver.cpp", tmp_path_factory.mktemp("band_refine_driver"))


def test_refinement_entry_points_under_address_and_undefined_behaviour_sanitizers(driver):
    run = subprocess.run([driver], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


def _doubles(a, order="F"):
    a = np.asarray(a, dtype=np.float64).ravel(order=order)
    return f"{len(a)} " + " ".join(float(v).hex() for v in a)


def dump_refinement(driver, tmp_path, s, steps, tol, min_steps):
    """The driver's composition on the system ``s`` (a ``band_refine_cases.Dense``): the band record of the first solve and the
    list of ``(x, r, rec)`` after step 0 ... ``steps``."""
    path = tmp_path / "system.txt"
    path.write_text("\n".join([f"{s.nb} {s.w} {s.p} {steps} {min_steps} {float(tol).hex()}", _doubles(s.AB), _doubles(s.U), _doubles(s.C),
                               _doubles(s.rhs)]) + "\n")
    run = subprocess.run([driver, "--dump", str(path)], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
    got = np.array([float.fromhex(t) for t in run.stdout.split()])
    band, rest = got[:8], got[8:].reshape(steps + 1, 2 * s.N + 8)
    return band, [(row[: s.N], row[s.N: 2 * s.N], row[2 * s.N:]) for row in rest]


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("k", range(5))
def test_the_host_walk_matches_the_emulator_bit_for_bit(driver, tmp_path, k):
    row = br.TABLE[k]
    s = br.table_system(row)
    steps = br.MAX_STEPS if k == 4 else 3
    band, got = dump_refinement(driver, tmp_path, s, steps, TABLE_TOL, 0)
    want = s.refine(steps, tol=TABLE_TOL)
    assert _same(band, s.first()[1]) and band[bc.STATUS] == 0.0
    for t, ((x, r, rec), (w_x, w_r, w_rec)) in enumerate(zip(got, want)):
        assert _same(rec, w_rec), (t, rec, w_rec)
        assert _same(x, w_x) and _same(r, w_r), t
    final = got[-1][2]
    assert final[br.STATUS] == row[2]
    if k == 0:
        assert final[br.STEPS] == 0.0 and _same(got[-1][0], got[0][0])
    elif k < 4:
        assert final[br.STEPS] == 1.0 and final[br.RHO] <= 1.0e-14 and final[br.RHO0] >= 1.0e-12
    else:
        assert final[br.RHO] > br.SINGULAR


def test_min_steps_takes_a_correction_the_tolerance_did_not_ask_for(driver, tmp_path):
    s = br.table_system(br.TABLE[0])
    _, got = dump_refinement(driver, tmp_path, s, 2, br.TOL, 1)
    want = s.refine(2, tol=br.TOL, min_steps=1)
    for (x, r, rec), (w_x, w_r, w_rec) in zip(got, want):
        assert _same(rec, w_rec) and _same(x, w_x) and _same(r, w_r)
    assert got[0][2][br.STATUS] == br.RUNNING and got[1][2][br.STATUS] == br.CONVERGED and got[2][2][br.STEPS] == 1.0
