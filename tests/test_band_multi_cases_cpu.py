"""The emulator of the block solve (tests/band_multi_cases.py) held to statements that are not its own; CPU only.

* ``solve_columns`` (the single solve of tests/band_cases.py column by column) is held by the residual: every column's
  normalised residual ``|K x - b|_inf / (|K|_inf |x|_inf + |b|_inf)`` in extended precision against a dense
  ``numpy.linalg.solve`` of the bordered matrix, at most 4 times LAPACK's own on the same column (and one unit roundoff where
  LAPACK's is smaller): DESIGN.md section 23's rule.
* ``solve_block``, the restatement of the block kernels' own walk, gives ``solve_columns``' bits -- and with each of the five
  planted mistakes of ``MUTANTS`` it does not: the bit comparison catches every one."""
import numpy as np
import pytest

import band_cases as bc
import band_multi_cases as bm

U_ROUND = 2.0 ** -53
INPUTS = [(40, 5, 2, 3), (2 * bc.NB + 1, 7, 3, 9), (97, bc.NB + 1, 1, 2), (bc.W_CAP + 40, bc.W_CAP, 0, 5), (300, 20, bc.P_CAP, bm.RHS_CAP)]


def _normalised(K, x, b):
    Kl, xl, bl = K.astype(np.longdouble), x.astype(np.longdouble), b.astype(np.longdouble)
    return float(np.abs(Kl @ xl - bl).max() / (np.abs(Kl).sum(axis=1).max() * np.abs(xl).max() + np.abs(bl).max()))


@pytest.mark.parametrize("nb,w,p,k", INPUTS)
def test_every_column_of_the_emulator_is_held_by_lapacks_residual(nb, w, p, k):
    AB, U, C, R = bm.block(nb, w, p, k, seed=2, gap=3)
    _, _, X, rec = bm.solve_columns(AB, U, C, R)
    assert rec[bc.STATUS] == 0.0 and X.shape == (k, nb + p)
    K = bc.full_matrix(AB, U, C, w)
    worst = 0.0
    for c in range(k):
        b = R[c, : nb + p]
        ours, dense = _normalised(K, X[c], b), _normalised(K, np.linalg.solve(K, b), b)
        worst = max(worst, ours / max(dense, U_ROUND))
        assert ours <= 4.0 * max(dense, U_ROUND), (c, ours, dense)
    print(f"Nb {nb} w {w} p {p} k {k}: worst residual / LAPACK's {worst:.2f}")


@pytest.mark.parametrize("nb,w,p,k,gap", [(40, 5, 2, 3, 0), (40, 5, 2, 3, 3), (2 * bc.NB + 1, 7, bc.P_CAP, 9, 3), (33, 33, 1, bm.RHS_CAP, 0), (65, 0, 0, 2, 3),
                                          (1, 7, 1, 2, 0), (0, 0, 1, 2, 1), (300, 20, 3, bm.RHS_CAP, 3)])
def test_the_block_walk_gives_the_bits_of_the_single_solve_column_by_column(nb, w, p, k, gap):
    AB, U, C, R = bm.block(nb, w, p, k, seed=3, gap=gap)
    band, ipiv, X, rec = bm.solve_block(AB, U, C, R)
    w_band, w_ipiv, w_X, w_rec = bm.solve_columns(AB, U, C, R)
    assert rec[bc.STATUS] == 0.0 and bm.same(rec, w_rec) and np.array_equal(ipiv, w_ipiv) and bm.same(band, w_band)
    assert bm.same(X, w_X)


@pytest.mark.parametrize("mutant", bm.MUTANTS)
def test_every_planted_mistake_is_caught_by_the_bit_comparison(mutant):
    nb, w, p, k, gap = 40, 5, 2, 5, 3
    AB, U, C, R = bm.block(nb, w, p, k, seed=6, gap=gap)
    cap = 1 if mutant == "one_trip" else bm.GRID_CAP      # (one workgroup: the 80 + 5 * 42 elements need a second trip)
    assert nb * p + k * (nb + p) > bm.BLOCK * cap or mutant != "one_trip"
    right = bm.solve_block(AB, U, C, R, grid_cap=cap)
    assert bm.same(right[2], bm.solve_columns(AB, U, C, R)[2])
    wrong = bm.solve_block(AB, U, C, R, mutant=mutant, grid_cap=cap)
    assert wrong[2] is None or not bm.same(right[2], wrong[2]), f"the mistake {mutant!r} left every bit"
    if wrong[2] is not None and mutant in ("previous_rhs", "first_xc"):      # ... and column 0 is the one it leaves alone
        assert bm.same(right[2][0], wrong[2][0])


def test_a_failed_factorisation_gives_no_column_and_a_nan_stays_in_its_column():
    AB, U, C, R = bm.block(3 * bc.NB + 5, 7, 1, 3, seed=4, variant="zero_column")
    for solve in (bm.solve_columns, bm.solve_block):
        _, _, X, rec = solve(AB, U, C, R)
        assert X is None and rec[bc.STATUS] == 1.0 and rec[bc.COLUMN] == bc.failing_column(3 * bc.NB + 5, "zero_column")
    AB, U, C, R = bm.block(2 * bc.NB + 1, 7, 3, 5, seed=4)
    clean = bm.solve_block(AB, U, C, R)[2]
    R[2, 11] = np.nan
    X = bm.solve_block(AB, U, C, R)[2]
    assert bm.same(X, bm.solve_columns(AB, U, C, R)[2])
    assert np.isnan(X[2]).any() and all(bm.same(X[c], clean[c]) for c in (0, 1, 3, 4))


def test_the_shapes_cover_the_sizes_where_a_kernel_changes_its_path():
    shapes = bm.shapes()
    assert len(shapes) == 5 * 4 * 3 * 4 and (0, 0, 0, 1) in shapes and (2 * bc.NB + 1 + bc.W_CAP, bc.W_CAP, bc.P_CAP, bm.RHS_CAP) in shapes
    assert set(bm.GPU_NB_SHAPES) == set(bm.NB_SHAPES) - {0} and max(bm.K_SHAPES) == bm.RHS_CAP
    nb, _, _, k = bm.LONG
    assert (nb + 2047) // 2048 == 3 and k == bm.RHS_CAP
