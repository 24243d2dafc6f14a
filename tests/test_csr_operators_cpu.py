"""The operator structures of the device-side products J v, J^T y, H v (pockit_amd/csr.py: CsrMap.operator / transposed /
symmetric) against scipy.sparse, and the runtime unit that applies them (pockit_amd/csrc/pk_ops.cpp: row blocks, the walk of
pk_op_rows / pk_op_long, refusals, tear-down) built with ``-fsanitize=address,undefined`` against the host-only stand-in of the
HIP runtime and driven by tests/fake_hip/ops_driver.cpp.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse

import models
import pockit_amd.radau as radau
from pockit_amd.csr import CsrMap, CsrOperator
from sanitized_build import sanitized_driver


def _same_matrix(a, b):
    """Exact equality as matrices (explicit zeros and the order of storage do not matter)."""
    a, b = scipy.sparse.csr_array(a), scipy.sparse.csr_array(b)
    return a.shape == b.shape and (a != b).nnz == 0


def _check_structure(op, shape):
    assert isinstance(op, CsrOperator) and op.shape == shape
    assert op.indptr.dtype == np.int32 and op.indices.dtype == np.int32 and (op.src is None or op.src.dtype == np.int32)
    assert op.indptr[0] == 0 and op.indptr[-1] == op.nnz == len(op.indices) and np.all(np.diff(op.indptr) >= 0)
    for r in range(shape[0]):                      # columns strictly ascending within a row
        assert np.all(np.diff(op.indices[op.indptr[r]: op.indptr[r + 1]]) > 0)


def _random_pattern(seed, n_rows, n_cols, n_triplets, lower=False):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_rows, n_triplets)
    cols = rng.integers(0, n_cols, n_triplets)
    rows[rows % 5 == 3] = 0                        # empty rows (and a full first one)
    cols[::7] = n_cols // 2                        # a dense column
    rows[: n_triplets // 10], cols[: n_triplets // 10] = rows[-(n_triplets // 10):].copy(), cols[-(n_triplets // 10):].copy()   # repeats
    if lower:
        rows, cols = np.maximum(rows, cols), np.minimum(rows, cols)
    return rows, cols


def _check_builders(rows, cols, shape, values_seed, lower):
    cm = CsrMap(rows, cols, shape)
    vals = np.random.default_rng(values_seed).standard_normal(cm.nnz)
    A = cm.to_scipy(vals)
    own = cm.operator()
    _check_structure(own, shape)
    assert own.src is None and _same_matrix(own.to_scipy(vals), A)
    t = cm.transposed()
    _check_structure(t, shape[::-1])
    assert _same_matrix(t.to_scipy(vals), A.T)
    assert sorted(t.src.tolist()) == list(range(cm.nnz))      # every value of A exactly once
    if lower:
        s = cm.symmetric()
        _check_structure(s, shape)
        dense = A.toarray()
        assert _same_matrix(s.to_scipy(vals), dense + dense.T - np.diag(np.diag(dense)))
        assert np.array_equal(s.to_scipy(vals).toarray(), s.to_scipy(vals).toarray().T)
        n_diag = int(np.count_nonzero(np.repeat(np.arange(shape[0]), np.diff(cm.indptr)) == cm.indices))
        assert s.nnz == 2 * cm.nnz - n_diag            # off-diagonal entries twice, diagonal entries once
        counts = np.bincount(s.src, minlength=cm.nnz)
        assert set(counts.tolist()) <= {1, 2} and int((counts == 1).sum()) == n_diag


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_builders_match_scipy_on_random_patterns(seed):
    _check_builders(*_random_pattern(seed, 37, 23, 400), (37, 23), seed + 10, lower=False)
    _check_builders(*_random_pattern(seed, 5, 301, 600), (5, 301), seed + 20, lower=False)
    _check_builders(*_random_pattern(seed, 41, 41, 500, lower=True), (41, 41), seed + 30, lower=True)


@pytest.mark.parametrize("mesh, num_point", [(3, 4), (60, 5)])
def test_builders_match_scipy_on_the_structure_of_a_plan(mesh, num_point):
    plan = models.brachistochrone(radau, mesh, num_point)[0].plan
    _check_builders(plan.jac_row, plan.jac_col, (plan.m, plan.n), 1, lower=False)
    _check_builders(plan.hess_row, plan.hess_col, (plan.n, plan.n), 2, lower=True)


def test_the_small_gpu_shapes_reach_the_long_row_path():
    """brachistochrone(radau, 60, 5), the smallest model of tests/test_gpu_csr_operators.py with a row of more than 256
    entries: the column of t_f in J^T (4 pieces) and the row of t_f in the symmetric H (3 pieces), empty rows in H."""
    plan = models.brachistochrone(radau, 60, 5)[0].plan
    jt = CsrMap(plan.jac_row, plan.jac_col, (plan.m, plan.n)).transposed()
    h = CsrMap(plan.hess_row, plan.hess_col, (plan.n, plan.n)).symmetric()
    assert -(-int(np.diff(jt.indptr).max()) // 256) == 4 and -(-int(np.diff(h.indptr).max()) // 256) == 3
    assert int((np.diff(h.indptr) == 0).sum()) > 256


def test_symmetric_refuses_an_entry_above_the_diagonal():
    with pytest.raises(ValueError, match="above the diagonal"):
        CsrMap([0, 1, 1], [0, 0, 2], (3, 3)).symmetric()
    with pytest.raises(ValueError, match="square"):
        CsrMap([0, 1], [0, 0], (2, 3)).symmetric()
    CsrMap([0, 1, 1, 2], [0, 0, 1, 0], (3, 3)).symmetric()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_operator_entry_points_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (its own main): nothing sanitized is loaded into Python."""
    exe = sanitized_driver("ops_driver.cpp", tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
