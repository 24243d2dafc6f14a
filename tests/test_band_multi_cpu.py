"""The block solve of the bordered band LU (pockit_amd/csrc/pk_band.cpp: k right-hand sides against one factorisation, the launches
of one solve) built with ``-fsanitize=address,undefined`` against the host-only stand-in of the HIP runtime and driven by
tests/fake_hip/band_multi_driver.cpp: the stand-in walk of every generalised kernel against plain loops and against k calls of
the single raw form, bit for bit, at the shapes of tests/band_multi_cases.py; strides with NaN in the gaps; a NaN confined to its
column; failed factorisations that leave every column untouched; the elementwise stride loops taken to a second trip; the planned
and host forms against the single ones; the refusals with their codes and sentinels; what frees the state.  With ``--dump`` the
blocks of tests/band_multi_cases.py compared BIT FOR BIT with its emulator (the single solve of tests/band_cases.py column by
column).  CPU only; a stand-alone program (its own main): nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import band_cases as bc
import band_multi_cases as bm
from sanitized_build import sanitized_driver

ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sanitized_driver("band_multi_driver.cpp", tmp_path_factory.mktemp("band_multi_driver"))


def test_block_solve_entry_points_under_address_and_undefined_behaviour_sanitizers(driver):
    run = subprocess.run([driver], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


def _doubles(a, order="F"):
    a = np.asarray(a, dtype=np.float64).ravel(order=order)
    return f"{len(a)} " + " ".join(float(v).hex() for v in a)


def dump_block(driver, tmp_path, AB, U, C, R):
    """The driver's raw block form: (band, ipiv, X (k, nb + p), rec); the driver checks that the gaps of the solutions stay NaN."""
    ldab, nb = AB.shape
    w, p, (k, stride) = (ldab - 1) // 3, C.shape[0], R.shape
    path = tmp_path / "block.txt"
    path.write_text("\n".join([f"{nb} {w} {p} {k} {stride}", _doubles(AB), _doubles(U), _doubles(C), _doubles(R, "C")]) + "\n")
    run = subprocess.run([driver, "--dump", str(path)], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
    got = np.array([float.fromhex(t) for t in run.stdout.split()])
    band, ipiv, X, rec = np.split(got, np.cumsum([ldab * nb, nb, k * (nb + p)]))
    return band.reshape((ldab, nb), order="F"), ipiv.astype(np.int64), X.reshape(k, nb + p), rec


@pytest.mark.parametrize("nb,w,p,k,gap", [(2 * bc.NB + 1, 7, 3, 9, 3), (33, 33, 1, 2, 0), (97, 20, bc.P_CAP, bm.RHS_CAP, 3),
                                          (2 * bc.NB + 1 + bc.W_CAP, bc.W_CAP, 1, 2, 0), (4500, 8, 1, 3, 3), (40, 7, 0, 9, 3)])
def test_the_host_walk_matches_the_emulator_bit_for_bit(driver, tmp_path, nb, w, p, k, gap):
    AB, U, C, R = bm.block(nb, w, p, k, seed=3, gap=gap)
    band, ipiv, X, rec = dump_block(driver, tmp_path, AB, U, C, R)
    w_band, w_ipiv, w_X, w_rec = bm.solve_columns(AB, U, C, R)
    assert w_rec[bc.STATUS] == 0.0 and bm.same(rec, w_rec) and np.array_equal(ipiv, w_ipiv)
    inside = bc.in_band(nb, w) | bc.fill_rows(nb, w)
    assert bm.same(band[inside], w_band[inside])
    assert bm.same(X, w_X)


def test_a_failed_pivot_is_reported_and_no_column_is_written(driver, tmp_path):
    nb, w, p, k = 3 * bc.NB + 5, 7, 1, 4
    AB, U, C, R = bm.block(nb, w, p, k, seed=4, gap=3, variant="zero_column")
    _, _, X, rec = dump_block(driver, tmp_path, AB, U, C, R)
    _, _, w_X, w_rec = bm.solve_columns(AB, U, C, R)
    assert w_X is None and bm.same(rec, w_rec) and rec[bc.STATUS] == 1.0 and rec[bc.COLUMN] == bc.failing_column(nb, "zero_column")
    assert np.all(X == -77.0)
