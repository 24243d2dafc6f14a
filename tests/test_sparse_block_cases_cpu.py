"""tests/sparse_block_cases.py itself: the per-column expectation accepts a block walk written in NumPy the way the kernels are
laid out (chunks of 8 columns, one plane per column, ``partial[slot, column]``) at every k the GPU file uses, and catches its
three deliberate mistakes.  The bounds are those of tests/sparse_cases.py, per (row, column).  CPU only."""
import numpy as np
import pytest

import sparse_block_cases as sbc
import sparse_cases as sc


def _case(ctx, name, op):
    return next(c for c in sc.operator_cases() if c.id == f"{ctx}-{name}-op{op}")


SMALL = [("A", "edges", 1), ("A", "no-src", 0), ("B", "long-first-and-last", 2), ("B", "equal-lengths", 1), ("B", "cut-by-rows", 0)]


@pytest.mark.parametrize("k", [1, 3, 8, 9])
@pytest.mark.parametrize("which", SMALL, ids=lambda w: f"{w[0]}-{w[1]}-op{w[2]}")
def test_the_numpy_block_walk_holds_per_column(which, k):
    case = _case(*which)
    V, Add = sbc.block_inputs(case, k, seed=10 * k + case.op)
    want = sbc.BlockExpectation(case, V, Add)
    assert want.problems(sbc.walk_block(case, V), False) == []
    assert want.problems(sbc.walk_block(case, V, Add), True) == []
    for j in range(k):      # the contract itself: column j is the single-vector emulator on column j
        assert sc.same_bits(want.emulated[True][:, j], sc.emulate_operator(sbc.column_case(case, V, Add, j), Add[:, j]))
    assert np.all(want.bound[False][case.lengths == 0] == 0.0)


def test_the_inputs_make_every_product_exact_and_each_row_of_one_scale():
    case = _case("B", "equal-lengths", 0)
    V, Add = sbc.block_inputs(case, 5, seed=3)
    assert V.shape == (case.n_cols, 5) and Add.shape == (case.n_rows, 5) and V.flags.c_contiguous and Add.flags.c_contiguous
    assert np.array_equal(np.float32(np.abs(V)).astype(np.float64), np.abs(V)) and np.all((np.abs(V) >= 1) & (np.abs(V) < 2))
    scale = np.ldexp(1.0, np.asarray(sc.BUCKETS)[np.arange(case.n_rows) % 5])[:, None]
    assert np.all((np.abs(Add) >= scale) & (np.abs(Add) < 4 * scale))
    assert len({V[:, j].tobytes() for j in range(5)}) == 5      # the columns differ: a swapped plane shows


@pytest.mark.parametrize("mutant, which, k", [("plane", ("B", "equal-lengths", 1), 8), ("plane", ("A", "edges", 1), 3),
                                              ("shared_partial", ("B", "long-first-and-last", 2), 8),
                                              ("shared_partial", ("A", "pieces", 1), 3),
                                              ("last_chunk", ("A", "edges", 0), 9)])
def test_the_checker_catches_every_mutant_of_the_block_walk(mutant, which, k):
    assert set(sbc.BLOCK_MUTANTS) == {"plane", "shared_partial", "last_chunk"}
    case = _case(*which)
    V, Add = sbc.block_inputs(case, k, seed=99)
    want = sbc.BlockExpectation(case, V, Add)
    for with_add in (False, True):
        assert want.problems(sbc.walk_block(case, V, Add if with_add else None), with_add) == []
        found = want.problems(sbc.walk_block(case, V, Add if with_add else None, mutant), with_add)
        assert found, f"{mutant} passed on {case.id}"
        if mutant == "last_chunk":
            assert any("column 8" in f and "not written" in f for f in found) and not any("column 7" in f for f in found)
