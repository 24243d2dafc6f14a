"""The emulator of the band solve's refinement (tests/band_refine_cases.py) against statements that are not its own, the five
synthetic systems it is used on, and its mutants.  CPU only.

The five systems are those of ``band_refine_cases.TABLE``: a well-conditioned one, two whose band part B has one column and row
scaled by 2^-30 and 2^-24 (cond B 1.8e9 and 3.5e7, cond K 56 and 160), and two of ``band_cases``' "tiny_diagonal" variant
(cond B 2e16, cond K 2e5 and 7e4).  The refinements run with ``tol = 1e-14``: the bound the rows 2 to 4 are held to after one
correction, so that a row counts as converged exactly when it meets that bound -- row 1 at once (rho_0 = 3.6e-16), the rows 2 to
4 (rho_0 from 2.1e-11 to 2.2e-4) after one correction.  Row 5 cannot be repaired: rho falls from 4.9e4 to 0.45 and stalls."""
import numpy as np
import pytest

import band_cases as bc
import band_refine_cases as br

LD = np.longdouble
TABLE_TOL = 1.0e-14


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def histories():
    """Per row of the table the system and its refinement of ten enqueued steps, computed once."""
    out = []
    for row in br.TABLE:
        s = br.table_system(row)
        out.append((row, s, s.refine(br.MAX_STEPS, tol=TABLE_TOL)))
    return out


# ---------------------------------------------------------------- the kernels against plain statements
@pytest.mark.parametrize("length", br.LENGTHS)
@pytest.mark.parametrize("fixed", [False, True])
def test_the_residual_against_a_plain_loop(length, fixed):
    where, b, q, x, _ = br.step_vectors(length, planted=True, fixed=fixed)
    r, (rn, xn, bn, bad) = br.resid(b, q, x, where)
    want_r, maxima, count = np.zeros(length), [0.0, 0.0, 0.0], 0
    for i in range(length):
        if where is not None and where[i] < 0:
            continue
        with np.errstate(all="ignore"):
            ri = np.float64(b[i]) - np.float64(q[i])
        want_r[i] = ri
        if np.isfinite(ri) and np.isfinite(x[i]) and np.isfinite(b[i]):
            maxima = [max(maxima[0], abs(ri)), max(maxima[1], abs(x[i])), max(maxima[2], abs(b[i]))]
        else:
            count += 1
    live = br.unknowns(length, where)
    assert np.array_equal(np.isnan(r), np.isnan(want_r)) and _same(np.nan_to_num(r, nan=7.0), np.nan_to_num(want_r, nan=7.0))
    assert np.all(r[~live] == 0.0) and not np.any(np.signbit(r[~live]))
    assert (rn, xn, bn, bad) == (maxima[0], maxima[1], maxima[2], float(count))
    planted = min(6, int(live.sum()))
    assert bad >= 1 if planted else bad == 0


def test_the_residual_is_one_rounding_of_the_exact_difference():
    _, b, q, x, _ = br.step_vectors(2049, planted=False, fixed=False)
    r, _ = br.resid(b, q, x)
    exact = b.astype(LD) - q.astype(LD)                  # (exact in extended precision: both have 53 bits, close exponents)
    assert _same(r, exact.astype(np.float64))


@pytest.mark.parametrize("rn,xn,bn", [(3.0e-7, 2.5, 0.75), (1.0, 1.0e9, 2.0), (0.0, 3.0, 1.0), (5.0e-3, 0.0, 0.0), (1.0e-300, 1.0e-3, 0.0),
                                      (2.0, 1.0e300, 1.0e300)])
def test_the_ratio_against_extended_precision(rn, xn, bn):
    rho = br.ratio(rn, xn, bn)
    if rn == 0.0:
        assert rho == 0.0
        return
    den = min(LD(xn), LD(1.0e6) * LD(bn)) + LD(bn)
    with np.errstate(all="ignore"):
        want = float(LD(rn) / den) if den != 0 else np.inf
    assert rho == want or abs(rho - want) <= 4.0 * 2.0 ** -53 * abs(want)      # three roundings: product, sum, quotient


def test_the_decision_in_its_order():
    run = np.array([br.RUNNING, 1.0, 1.0e-9, 1.0, 1.0, 1.0e-9, 1.0e-3, 1.0e-3])
    sums = lambda rho, bad=0.0: (rho * 2.0, 1.0, 1.0, bad)      # noqa: E731  (rho = rn / (min(1, 1e6) + 1))
    # 1: a non-finite count wins over everything
    assert br.scalar(sums(1.0e-16, 2.0), run, 2, 1e-10, 0)[br.STATUS] == br.NON_FINITE
    # 2: converged, though rho did not fall (rule 2 ahead of rule 3)
    rec = br.scalar(sums(1.0e-9), run, 2, 1e-8, 0)
    assert rec[br.STATUS] == br.CONVERGED and rec[br.PREV] == 1.0e-9 and rec[br.RHO] == 1.0e-9 and rec[br.STEPS] == 2.0
    # ... but not before min_steps: then the stall rule speaks
    assert br.scalar(sums(1.0e-9), run, 2, 1e-8, 3)[br.STATUS] == br.STALLED
    # 3: the improvement factor: a fall by less than 1e-9 relative is a stall, by more is none
    assert br.scalar(sums(1.0e-9 * (1.0 - 1.0e-10)), run, 2, 1e-12, 0)[br.STATUS] == br.STALLED
    assert br.scalar(sums(1.0e-9 * (1.0 - 1.0e-8)), run, 2, 1e-12, 0)[br.STATUS] == br.RUNNING
    # step 0 cannot stall, keeps no previous rho and sets rho_0
    rec = br.scalar(sums(0.5), None, 0, 1e-10, 0)
    assert rec[br.STATUS] == br.RUNNING and rec[br.RHO0] == 0.5 and rec[br.PREV] == 0.0 and rec[br.STEPS] == 0.0
    # a failed factorisation: nothing is measured
    assert _same(br.scalar(sums(0.5), None, 0, 1e-10, 0, band_status=1.0), [br.BAND_FAILED, 0, 0, 0, 0, 0, 0, 0])
    # a stopped record stays
    for status in (br.CONVERGED, br.STALLED, br.NON_FINITE, br.BAND_FAILED):
        stopped = run.copy()
        stopped[br.STATUS] = status
        assert _same(br.scalar(sums(0.25), stopped, 3, 1e-10, 0), stopped)


def test_the_correction_only_while_running_and_only_at_unknowns():
    where, _, _, x, d = br.step_vectors(257, planted=False, fixed=True)
    rec = np.zeros(8)
    got = br.correct(x, d, rec, where)
    live = where >= 0
    assert _same(got[live], x[live] + d[live]) and np.all(np.isnan(got[~live]))
    rec[br.STATUS] = br.CONVERGED
    assert _same(br.correct(x, d, rec, where)[live], x[live])


# ---------------------------------------------------------------- the five systems
def test_the_dense_product_is_the_stated_association():
    s = br.table_system(br.TABLE[1])
    x = np.random.default_rng(3).uniform(-1.0, 1.0, s.N)
    want = np.zeros(s.N)
    for i in range(s.N):
        acc = 0.0
        for j in range(s.N):
            acc = acc + float(np.float64(s.K[i, j]) * np.float64(x[j]))
        want[i] = acc
    assert _same(s.kx(x), want)
    exact = s.K.astype(LD) @ x.astype(LD)
    assert np.max(np.abs(want - exact)) <= s.N * 2.0 ** -53 * np.max(np.abs(s.K).astype(LD) @ np.abs(x).astype(LD))


def test_the_squeezed_systems_are_the_issues():
    for row, cond_b, cond_k in ((br.TABLE[1], 1.8e9, 56.0), (br.TABLE[2], 3.5e7, 160.0)):
        s = br.table_system(row)
        (nb, w, p, seed, _), (j, factor) = row[0], row[1]
        plain = br.Dense(*bc.system(nb, w, p, seed, "plain"))
        B, B0 = bc.dense(s.AB, s.w), bc.dense(plain.AB, plain.w)
        scale = np.ones((nb, nb))
        scale[j, :] = scale[:, j] = factor
        assert _same(B, B0 * scale) and _same(s.U, plain.U) and _same(s.C, plain.C) and _same(s.rhs, plain.rhs)
        assert 0.9 * cond_b <= np.linalg.cond(B) <= 1.1 * cond_b and 0.9 * cond_k <= np.linalg.cond(s.K) <= 1.1 * cond_k


@pytest.mark.parametrize("k", range(5))
def test_the_table(histories, k):
    row, s, history = histories[k]
    _, _, status, corrections = row
    final = history[-1][2]
    stop = next(t for t, (_, _, rec) in enumerate(history) if rec[br.STATUS] != br.RUNNING)
    print(f"row {k + 1}: rho by step {[float(rec[br.RHO]) for _, _, rec in history[: stop + 1]]}, status {final[br.STATUS]}")
    assert final[br.STATUS] == status
    # the freeze rule: nothing moves behind the stop
    for x, r, rec in history[stop:]:
        assert _same(x, history[stop][0]) and _same(r, history[stop][1]) and _same(rec, history[stop][2])
    x0, band = s.first()
    assert band[bc.STATUS] == 0.0 and _same(history[0][0], x0)
    if k == 0:
        assert final[br.STEPS] == 0.0 and _same(history[-1][0], x0), "row 1: no correction, x keeps its bits"
    elif k < 4:
        assert final[br.STEPS] == corrections == 1.0 and stop == 1
        assert final[br.RHO] <= 1.0e-14 and final[br.RHO0] >= 1.0e-12 and final[br.PREV] == final[br.RHO0]
    else:
        assert final[br.RHO] > br.SINGULAR and final[br.RHO] > br.IMPROVE * final[br.PREV] and final[br.STEPS] == stop
    # the record's rho against extended precision on the final x
    x, r, rec = history[-1]
    exact = s.rhs.astype(LD) - s.K.astype(LD) @ x.astype(LD)
    slack = s.N * 2.0 ** -53 * float(np.max(np.abs(s.K).astype(LD) @ np.abs(x).astype(LD)) + np.max(np.abs(s.rhs)))
    assert abs(float(np.max(np.abs(exact))) - rec[br.RNORM]) <= slack
    assert rec[br.XNORM] == np.max(np.abs(x)) and rec[br.BNORM] == np.max(np.abs(s.rhs))


def test_the_host_loop_reads_the_record_between_steps(histories):
    for k, (row, s, history) in enumerate(histories):
        x0, _ = s.first()
        x, r, rec = br.refine_host(s.solve, s.kx, s.rhs, x0, tol=TABLE_TOL, max_steps=br.MAX_STEPS)
        assert _same(x, history[-1][0]) and _same(rec, history[-1][2]) and _same(r, history[-1][1])
    row, s, history = histories[4]
    x0, _ = s.first()
    x, _, rec = br.refine_host(s.solve, s.kx, s.rhs, x0, tol=TABLE_TOL, max_steps=2)
    assert rec[br.STATUS] == br.EXHAUSTED and rec[br.STEPS] == 2.0 and _same(x, history[2][0])
    x, _, rec = br.refine_host(s.solve, s.kx, s.rhs, x0, tol=TABLE_TOL, max_steps=0)
    assert rec[br.STATUS] == br.EXHAUSTED and rec[br.STEPS] == 0.0 and _same(x, x0)


def test_a_planted_nan_ends_with_status_3_and_x_untouched(histories):
    _, s, _ = histories[1]
    x0, _ = s.first()
    b = s.rhs.copy()
    b[11] = np.nan
    history = br.refine(s.solve, s.kx, b, x0, steps=3)
    for x, _, rec in history:
        assert rec[br.STATUS] == br.NON_FINITE and rec[br.STEPS] == 0.0 and _same(x, x0)


# ---------------------------------------------------------------- the mutants
def _differs(a, b):
    return not all(_same(p[0], q[0]) and _same(np.nan_to_num(p[1], nan=7.0), np.nan_to_num(q[1], nan=7.0)) and _same(p[2], q[2])
                   for p, q in zip(a, b))


@pytest.mark.parametrize("mutant", br.MUTANTS)
def test_every_mutant_is_caught(histories, mutant):
    if mutant in ("fused_residual", "correct_behind_stop"):
        row, s, history = histories[1]
        assert _differs(history, s.refine(br.MAX_STEPS, tol=TABLE_TOL, mutant=mutant))
    elif mutant == "no_min_in_ratio":
        row, s, history = histories[4]
        assert _differs(history, s.refine(br.MAX_STEPS, tol=TABLE_TOL, mutant=mutant))
    elif mutant == "non_finite_in_maxima":
        where, b, q, x, _ = br.step_vectors(2049, planted=True, fixed=True)
        assert br.resid(b, q, x, where)[1] != br.resid(b, q, x, where, mutant)[1]
    elif mutant == "fixed_in_norms":
        where, b, q, x, _ = br.step_vectors(2049, planted=False, fixed=True)
        b, x = np.nan_to_num(b, nan=50.0), np.nan_to_num(x, nan=-60.0)      # (finite values at the fixed variables: larger than any unknown's)
        q = np.nan_to_num(q, nan=1.0)
        r, sums = br.resid(b, q, x, where)
        mr, msums = br.resid(b, q, x, where, mutant)
        assert sums != msums and not _same(r, mr)
    else:
        assert mutant == "stall_before_convergence"
        run = np.array([br.RUNNING, 1.0, 1.0e-16, 1.0, 1.0, 1.0e-16, 1.0e-9, 1.0e-9])
        sums = (2.0e-16, 1.0, 1.0, 0.0)            # rho stays at 1e-16: converged, and only the mutant calls it a stall
        assert br.scalar(sums, run, 2, 1e-10, 0)[br.STATUS] == br.CONVERGED
        assert br.scalar(sums, run, 2, 1e-10, 0, mutant=mutant)[br.STATUS] == br.STALLED
