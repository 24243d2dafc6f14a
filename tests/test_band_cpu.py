"""The runtime unit behind the bordered band LU (pockit_amd/csrc/pk_band.cpp) built with ``-fsanitize=address,undefined`` against
the host-only stand-in of the HIP runtime and driven by tests/fake_hip/band_driver.cpp: the stand-in walk of every kernel
against plain loops at the sizes where the panels, the windows and the border change shape, the public forms against the raw
form, the host form against the device forms, the refusals with their codes and sentinels, a failed pivot leaving the solution
untouched, what frees the state; with ``--dump`` the systems of tests/band_cases.py compared BIT FOR BIT with its emulator, so the
documented order of operations is held on the CPU as well.  CPU only; a stand-alone program (its own main): nothing sanitized is
loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import band_cases as bc
from sanitized_build import sanitized_driver

ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sanitized_driver("band_driver.cpp", tmp_path_factory.mktemp("band_driver"))


def test_band_entry_points_under_address_and_undefined_behaviour_sanitizers(driver):
    run = subprocess.run([driver], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


def _doubles(a):
    a = np.asarray(a, dtype=np.float64).ravel(order="F")
    return f"{len(a)} " + " ".join(float(v).hex() for v in a)


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all(got.view(np.uint64) == want.view(np.uint64)))


def dump_case(driver, tmp_path, AB, U, C, rhs):
    """The driver's raw form on a system: (band, ipiv, x, rec)."""
    ldab, nb = AB.shape
    w, p = (ldab - 1) // 3, C.shape[0]
    path = tmp_path / "band.txt"
    path.write_text("\n".join([f"{nb} {w} {p}", _doubles(AB), _doubles(U), _doubles(C), _doubles(rhs)]) + "\n")
    run = subprocess.run([driver, "--dump", str(path)], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
    got = np.array([float.fromhex(t) for t in run.stdout.split()])
    band, ipiv, x, rec = np.split(got, np.cumsum([ldab * nb, nb, nb + p]))
    return band.reshape((ldab, nb), order="F"), ipiv.astype(np.int64), x, rec


@pytest.mark.parametrize("nb,w,p,variant", [(2 * bc.NB + 1, 7, 3, "plain"), (2 * bc.NB + 1, bc.NB + 1, 1, "tiny_diagonal"), (97, 20, bc.P_CAP, "ties"),
                                            (2 * bc.NB + 1 + bc.W_CAP, bc.W_CAP, 1, "plain"), (4500, 8, 1, "tiny_diagonal"), (40, 7, 0, "plain")])
def test_the_host_walk_matches_the_emulator_bit_for_bit(driver, tmp_path, nb, w, p, variant):
    AB, U, C, rhs = bc.system(nb, w, p, seed=3, variant=variant)
    band, ipiv, x, rec = dump_case(driver, tmp_path, AB, U, C, rhs)
    w_band, w_ipiv, w_x, w_rec = bc.solve_system(AB, U, C, rhs)
    assert w_rec[bc.STATUS] == 0.0
    assert _same(rec, w_rec), (rec, w_rec)
    assert np.array_equal(ipiv, w_ipiv)
    inside = bc.in_band(nb, w) | bc.fill_rows(nb, w)
    assert _same(band[inside], w_band[inside])
    assert _same(x, w_x)
    if variant == "tiny_diagonal":
        assert rec[bc.SWAPS] == nb - 1 if nb <= bc.EVERY else rec[bc.SWAPS] >= nb // 4


@pytest.mark.parametrize("variant,status", [("zero_column", 1.0), ("nan", 3.0)])
def test_a_failed_pivot_is_reported_and_the_solution_left_alone(driver, tmp_path, variant, status):
    nb, w, p = 3 * bc.NB + 5, 7, 1
    AB, U, C, rhs = bc.system(nb, w, p, seed=4, variant=variant)
    _, _, x, rec = dump_case(driver, tmp_path, AB, U, C, rhs)
    _, _, w_x, w_rec = bc.solve_system(AB, U, C, rhs)
    assert w_x is None and _same(rec, w_rec)
    assert rec[bc.STATUS] == status and rec[bc.COLUMN] == bc.failing_column(nb, variant)
    assert np.all(x == -77.0)
