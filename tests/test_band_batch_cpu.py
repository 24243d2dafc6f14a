"""The batch forms of the bordered band LU (pockit_amd/csrc/pk_band.cpp: B systems behind one plan, one launch sequence) built with
``-fsanitize=address,undefined`` against the host-only stand-in of the HIP runtime and driven by
tests/fake_hip/band_batch_driver.cpp: every entry of a batch against the single raw form at B = 1, 2, 3 and 16, strides larger
than the lengths with NaN in the gaps, failing entries among good ones, a permuted batch, shared sources, the planned forms at
B = 2, 5, 2 around a single factorisation, the host form, the refusals, what frees the state; with ``--dump`` the batches of
tests/band_batch_cases.py compared BIT FOR BIT, entry by entry, with the emulator of tests/band_cases.py.  CPU only; a stand-alone
program (its own main): nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import band_batch_cases as bb
import band_cases as bc
from sanitized_build import sanitized_driver

ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sanitized_driver("band_batch_driver.cpp", tmp_path_factory.mktemp("band_batch_driver"))


def test_band_batch_entry_points_under_address_and_undefined_behaviour_sanitizers(driver):
    run = subprocess.run([driver], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


def _doubles(a):
    a = np.asarray(a, dtype=np.float64).ravel(order="F")
    return f"{len(a)} " + " ".join(float(v).hex() for v in a)


def dump_batch(driver, tmp_path, batch):
    """The driver's raw batch form on a batch: per entry (band, ipiv, x, rec).  The driver packs the entries itself, at a stride
    larger than the lengths, NaN in the gaps, and checks that the gaps stay NaN."""
    ldab = 3 * batch.w + 1
    lines = [f"{batch.B} {batch.nb} {batch.w} {batch.p}"]
    for e in range(batch.B):
        lines += [_doubles(batch.entry("band", batch.band, e)), _doubles(batch.entries[e][1]), _doubles(batch.entries[e][2]),
                  _doubles(batch.entries[e][3])]
    path = tmp_path / "batch.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([driver, "--dump", str(path)], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
    got = np.array([float.fromhex(t) for t in run.stdout.split()])
    per = ldab * batch.nb + batch.nb + batch.nb + batch.p + 8
    assert len(got) == per * batch.B
    out = []
    for chunk in got.reshape(batch.B, per):
        band, ipiv, x, rec = np.split(chunk, np.cumsum([ldab * batch.nb, batch.nb, batch.nb + batch.p]))
        out.append((band.reshape((ldab, batch.nb), order="F"), ipiv.astype(np.int64), x, rec))
    return out


@pytest.mark.parametrize("B,nb,w,p", [(3, 2 * bc.NB + 1, 7, 8), (2, 33, 33, 1), (bb.BATCH_CAP, 2 * bc.NB + 1, 0, 8), (1, 2 * bc.NB + 1 + bc.W_CAP, bc.W_CAP, 1),
                                      (3, 4129, 8, 1)])
def test_every_entry_of_the_host_walk_matches_the_emulator_bit_for_bit(driver, tmp_path, B, nb, w, p):
    batch = bb.Batch(nb, w, p, bb.picks(B, first_seed=5))
    for e, (band, ipiv, x, rec) in enumerate(dump_batch(driver, tmp_path, batch)):
        assert batch.expected[e][3][bc.STATUS] == 0.0 or e % 2      # (plain entries solve; a tiny diagonal may leave a singular border)
        bb.check_entry(batch, e, band, ipiv, x, rec)
    assert not bb.same(batch.expected[0][2], batch.expected[-1][2]) or B == 1


def test_failed_entries_are_reported_and_do_not_stop_the_others(driver, tmp_path):
    nb, w, p = 3 * bc.NB + 5, 7, 1
    batch = bb.Batch(nb, w, p, [(variant, 4) for variant, _ in bb.MIXED])
    for e, (band, ipiv, x, rec) in enumerate(dump_batch(driver, tmp_path, batch)):
        variant, status = bb.MIXED[e]
        assert rec[bc.STATUS] == status
        if status:
            assert rec[bc.COLUMN] == bc.failing_column(nb, variant)
        bb.check_entry(batch, e, band, ipiv, x, rec)
