"""The NumPy emulator of the bordered band LU (tests/band_cases.py) held to statements that are not its own; CPU only.

* ``P L U`` rebuilt in extended precision (``np.longdouble``) reproduces the matrix entrywise within the standard bound of LU by
  Gaussian elimination (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 9.3): ``|A - P L U|_ij <= gamma_T (|L||U|)_ij``
  with ``gamma_T = T u / (1 - T u)``, ``u = 2^-53`` and T the number of terms of row i's inner products (its multipliers that are
  not zero, plus one).  Without interchanges a row takes at most w multipliers, so ``T <= w + 1`` and the bound is
  ``c (w + 1) 2^-53 (|L||U|)_ij`` with ``c = 1 / (1 - (w + 1) 2^-53)`` -- asserted in that form on the inputs that do not
  interchange; a row that interchanges keeps being handed on and can take more, so there T is counted.
* its ``ipiv`` equals ``scipy.linalg.lapack.dgbtrf``'s on the inputs without ties.
* its solution is held by the residual: the normalised residual ``|K x - b|_inf / (|K|_inf |x|_inf + |b|_inf)`` in extended
  precision, of the band part against ``scipy.linalg.solve_banded`` and of the bordered system against a dense
  ``numpy.linalg.solve``, at most 4 times LAPACK's own on the same input (and one unit roundoff where LAPACK's is smaller).
  One kind of input is exempt from the bordered half and says why: the short systems in which EVERY column interchanges have
  a band part that is singular to working precision, which is the documented limit of pivoting inside the band.
* every deliberate mistake of ``MUTANTS`` is caught by the bit comparison."""
import numpy as np
import pytest
import scipy.linalg

import band_cases as bc

U_ROUND = 2.0 ** -53
INPUTS = [(nb, w, p, variant) for nb, w, p in ((40, 5, 2), (2 * bc.NB + 1, 7, 3), (97, bc.NB + 1, 1), (bc.W_CAP + 40, bc.W_CAP, 0), (300, 20, bc.P_CAP))
          for variant in ("plain", "tiny_diagonal", "ties")]


def _rebuild(F, w, ipiv):
    """``(P L U, |P L| |U|, T)`` from the factored band in extended precision; T per row."""
    nb = F.shape[1]
    Ud = np.zeros((nb, nb), dtype=np.longdouble)
    for j in range(nb):
        lo = max(0, j - 2 * w)
        Ud[lo: j + 1, j] = F[2 * w + lo - j: 2 * w + 1, j]
    M, Mabs, T = Ud.copy(), np.abs(Ud), np.ones(nb)
    for j in range(nb - 1, -1, -1):
        km = min(w, nb - 1 - j)
        l = F[2 * w + 1: 2 * w + km + 1, j].astype(np.longdouble)
        M[j + 1: j + km + 1] += l[:, None] * Ud[j][None, :]
        Mabs[j + 1: j + km + 1] += np.abs(l)[:, None] * np.abs(Ud[j])[None, :]
        T[j + 1: j + km + 1] += l != 0
        ip = int(ipiv[j])
        if ip != j:
            M[[j, ip]], Mabs[[j, ip]], T[[j, ip]] = M[[ip, j]], Mabs[[ip, j]], T[[ip, j]]
    return M, Mabs, T


@pytest.mark.parametrize("nb,w,p,variant", INPUTS)
def test_plu_reproduces_the_matrix_within_the_standard_bound(nb, w, p, variant):
    AB, _, _, _ = bc.system(nb, w, p, seed=2, variant=variant)
    F = AB.copy(order="F")
    ipiv, rec = bc.factor(F, w)
    assert rec[bc.STATUS] == 0.0
    M, Mabs, T = _rebuild(F, w, ipiv)
    A = bc.dense(AB, w).astype(np.longdouble)
    gamma = (T * U_ROUND / (1.0 - T * U_ROUND)).astype(np.longdouble)
    err = np.abs(A - M)
    worst = float(np.max(err / np.maximum(gamma[:, None] * Mabs, np.finfo(np.longdouble).tiny)))
    print(f"Nb {nb} w {w} {variant}: T up to {int(T.max())} (w + 1 = {w + 1}), interchanges {int(rec[bc.SWAPS])}, worst error / bound {worst:.3f}")
    assert np.all(err <= gamma[:, None] * Mabs)
    if rec[bc.SWAPS] == 0.0:
        c = 1.0 / (1.0 - (w + 1) * U_ROUND)
        assert T.max() <= w + 1 and np.all(err <= np.longdouble(c * (w + 1) * U_ROUND) * Mabs)


@pytest.mark.parametrize("nb,w,p,variant", [i for i in INPUTS if i[3] != "ties"])
def test_the_interchanges_are_lapacks(nb, w, p, variant):
    AB, _, _, _ = bc.system(nb, w, p, seed=2, variant=variant)
    F = AB.copy(order="F")
    ipiv, _ = bc.factor(F, w)
    _, piv, info = scipy.linalg.lapack.dgbtrf(AB.copy(order="F"), w, w)
    assert info == 0 and np.array_equal(piv, ipiv)


def _normalised(K, x, b):
    Kl, xl, bl = K.astype(np.longdouble), x.astype(np.longdouble), b.astype(np.longdouble)
    r = np.abs(Kl @ xl - bl).max() if len(b) else 0.0
    scale = np.abs(Kl).sum(axis=1).max() * np.abs(xl).max() + np.abs(bl).max() if len(b) else 1.0
    return float(r / scale)


@pytest.mark.parametrize("nb,w,p,variant", INPUTS)
def test_the_solution_is_held_by_lapacks_residual(nb, w, p, variant):
    AB, U, C, rhs = bc.system(nb, w, p, seed=2, variant=variant)
    F, ipiv, x, rec = bc.solve_system(AB, U, C, rhs)
    exempt = variant == "tiny_diagonal" and nb <= bc.EVERY and p > 0
    assert rec[bc.STATUS] == 0.0 or (exempt and rec[bc.STATUS] == 2.0)
    B, K = bc.dense(AB, w), bc.full_matrix(AB, U, C, w)
    # the band part alone: the emulator's sweeps against LAPACK's band solve
    y = rhs[:nb].copy()[:, None]
    bc.sweeps(F, w, ipiv, y)
    ours_band = _normalised(B, y[:, 0], rhs[:nb])
    lapack_band = _normalised(B, scipy.linalg.solve_banded((w, w), AB[w:], rhs[:nb]), rhs[:nb])
    # the bordered system against a dense solve
    ours, dense = (np.nan if x is None else _normalised(K, x, rhs)), _normalised(K, np.linalg.solve(K, rhs), rhs)
    print(f"Nb {nb} w {w} p {p} {variant}: band part {ours_band:.2e} (LAPACK {lapack_band:.2e}), bordered {ours:.2e} (dense solve {dense:.2e})")
    assert ours_band <= 4.0 * max(lapack_band, U_ROUND)
    if exempt:
        # every column interchanges: the row that is handed on shrinks by 2^-10 per column, so the band part alone is singular
        # to working precision (its condition number exceeds 2^(10 Nb)) while K is not -- the restricted-pivoting limit of
        # DESIGN.md section 23.  The band solve above is still backward stable; the border's Schur complement is not held (it may
        # even come out singular: status 2).
        assert np.linalg.cond(B) > 1e16
        return
    assert ours <= 4.0 * max(dense, U_ROUND)


def _bits(result):
    F, ipiv, x, rec = result
    return F.tobytes(), ipiv.tobytes(), None if x is None else x.tobytes(), rec.tobytes()


@pytest.mark.parametrize("mutant", bc.MUTANTS)
def test_every_deliberate_mistake_is_caught_by_the_bit_comparison(mutant):
    variant = {"tie_highest": "ties", "narrow_u": "tiny_diagonal", "swap_earlier_columns": "tiny_diagonal", "no_forward_swap": "tiny_diagonal"}.get(mutant, "plain")
    AB, U, C, rhs = bc.system(40, 5, 2, seed=6, variant=variant)
    right = bc.solve_system(AB, U, C, rhs)
    wrong = bc.solve_system(AB, U, C, rhs, mutant=mutant)
    assert _bits(right) == _bits(bc.solve_system(AB, U, C, rhs))            # the emulator repeats itself
    assert _bits(right) != _bits(wrong), f"the mistake {mutant!r} left every bit"
    if wrong[2] is not None and mutant in ("fma", "plain_border_dots"):      # ... though it is a sound algorithm: only the bits tell
        assert np.allclose(right[2], wrong[2], rtol=1e-9, atol=1e-12)


def test_failures_are_reported_with_their_column():
    for variant, status in (("zero_column", 1.0), ("nan", 3.0)):
        AB, U, C, rhs = bc.system(3 * bc.NB + 5, 7, 1, seed=4, variant=variant)
        _, _, x, rec = bc.solve_system(AB, U, C, rhs)
        assert x is None and rec[bc.STATUS] == status and rec[bc.COLUMN] == bc.failing_column(3 * bc.NB + 5, variant)
    AB, U, C, rhs = bc.system(8, 0, 1)
    AB[0, :], U[:, 0], C[0, 0] = 2.0, np.where(np.arange(8) < 2, 2.0, 0.0), 4.0
    _, _, x, rec = bc.solve_system(AB, U, C, rhs)
    assert x is None and rec[bc.STATUS] == 2.0 and rec[bc.COLUMN] == 8.0


def test_the_shapes_cover_the_sizes_where_a_kernel_changes_its_path():
    shapes = bc.shapes()
    assert {s[0] for s in shapes} >= set(bc.NB_SHAPES) and {s[1] for s in shapes} >= set(bc.W_SHAPES) and {s[2] for s in shapes} >= set(bc.P_SHAPES)
    assert any(nb <= w for nb, w, _ in shapes if nb > 1) and bc.LONG[0] // bc.NB + 1 == 1563 and bc.LONG[0] > 2048 * 8
