"""tests/minres_cases.py tested on the CPU: the emulator of the device's MINRES solve converges on every synthetic KKT system to
the SciPy matrix's solution within the derived bounds, does not depend on ``check_every``, reports what it should on a
preconditioner that is not positive and on ``b = 0``, and every deliberate mistake (minres_cases.MUTANTS) is caught by the bit
comparison the GPU file makes.

The bounds.  MINRES stops at ``phibar <= tol |b|_M`` in the recurrence; the true residual ``r = b - K x`` is held to
``2 tol |b|_M`` in the M-norm (the recurrence drifts from it by rounding, orders below tol at these condition numbers; the
factor 2 is the one of the CG tests, and ``test_the_factor_two_stands`` shows the emulator's worst ratio is at most 1).  From
``|r|_2 <= |r|_M / sqrt(min minv)`` and ``e = K^-1 r`` follows, for the quasi-definite family whose eigenvalues lie outside
``(-0.05, 1)`` by construction, ``max|x - x*| <= |r|_2 / 0.05 <= 2 tol |b|_M / sqrt(min minv) / 0.05``."""
import numpy as np
import pytest
import scipy.sparse.linalg

import cg_cases as cg
import minres_cases as mr
import sparse_cases as sc

TOL, MAXITER = 1e-8, 400
SOLVES = [(ctx, family, with_h, pre) for ctx, family, with_h in mr.SYSTEMS for pre in (True, False)]
# what a plain-NumPy prototype of the iteration took (with and without x0): the emulator's counts lie within a few of these
EXPECTED = {("A", "quasi", True): ((52, 53), (73, 75)), ("A", "quasi", False): ((50, 50), (56, 60)),
            ("A", "eq", True): ((91, 91), (128, 131)), ("A", "eq", False): ((75, 75), (91, 92)),
            ("B", "quasi", True): ((93, 94), (193, 197)), ("B", "quasi", False): ((96, 97), (162, 163))}


@pytest.fixture(scope="module")
def solved():
    """{(ctx, family, with_h, pre): (inputs, minv, x, rec)} with x0: computed once."""
    out = {}
    for ctx, family, with_h, pre in SOLVES:
        kk = mr.kkt(ctx)
        inp = kk.inputs(family, with_h)
        minv = kk.precond(with_h, inp["s1"], inp["s2"]) if pre else None
        x, rec = mr.emulate_solve(kk, with_h, inp["s1"], inp["s2"], minv, inp["b"], inp["x0"], TOL, MAXITER)
        out[ctx, family, with_h, pre] = (inp, minv, x, rec)
    return out


def test_the_systems_have_the_shapes_the_walk_needs():
    a, b = mr.kkt("A"), mr.kkt("B")
    assert (a.n, a.m, b.n, b.m) == (53, 36, 1205, 900)
    assert b.sy.has_long and not a.sy.has_long


@pytest.mark.parametrize("ctx,with_h", [("A", True), ("A", False), ("B", True), ("B", False)])
def test_the_quasi_family_is_quasi_definite_by_construction(ctx, with_h):
    inp = mr.kkt(ctx).inputs("quasi", with_h)
    lam = np.linalg.eigvalsh(inp["K"].toarray())
    print(f"{ctx} H={with_h}: no eigenvalue in ({lam[lam < 0].max():.3f}, {lam[lam > 0].min():.3f})")
    assert abs(inp["K"] - inp["K"].T).max() == 0.0
    assert lam[lam < 0].max() <= -mr.LAMBDA_QUASI and lam[lam > 0].min() >= 1.0
    assert (lam < 0).sum() == mr.kkt(ctx).m            # indefinite: m negative eigenvalues


@pytest.mark.parametrize("ctx,family,with_h", mr.SYSTEMS)
def test_the_emulated_product_and_preconditioner_are_the_matrix(ctx, family, with_h):
    kk = mr.kkt(ctx)
    inp = kk.inputs(family, with_h)
    for s1, s2 in ((inp["s1"], inp["s2"]), (None, inp["s2"]), (inp["s1"], None)):
        K = inp["K"]
        if s1 is None:
            K = K - scipy.sparse.diags_array(np.concatenate((inp["s1"], np.zeros(kk.m))))
        if s2 is None and inp["s2"] is not None:
            K = K + scipy.sparse.diags_array(np.concatenate((np.zeros(kk.n), inp["s2"])))
        y, ref = kk.kv(with_h, s1, s2, inp["x0"]), K @ inp["x0"]
        assert np.max(np.abs(y - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
    minv = kk.precond(with_h, inp["s1"], inp["s2"])
    top = np.abs((kk.sy.Hm.diagonal() if with_h else 0.0) + inp["s1"])
    low = np.abs(kk.sy.Jm.multiply(kk.sy.Jm) @ (1.0 / top) + (0.0 if inp["s2"] is None else inp["s2"]))
    assert np.all(minv > 0) and np.allclose(minv, 1.0 / np.concatenate((top, low)), rtol=1e-13, atol=0.0)


@pytest.mark.parametrize("ctx,family,with_h,pre", SOLVES)
def test_the_emulator_converges_within_the_derived_bounds(ctx, family, with_h, pre, solved):
    inp, minv, x, rec = solved[ctx, family, with_h, pre]
    r = inp["b"] - inp["K"] @ x
    res, nb = mr.m_norm(r, minv), mr.m_norm(inp["b"], minv)
    lo, hi = EXPECTED[ctx, family, with_h][0 if pre else 1]
    print(f"{ctx} {family} H={with_h} pre={pre}: {int(rec[mr.ITERS])} iterations (prototype {lo}-{hi}), M-norm residual "
          f"{res / (TOL * nb):.3f} tol |b|_M, phibar / true {rec[mr.PHIBAR] / res:.4f}")
    assert rec[mr.STATUS] == 1.0 and 0 < rec[mr.ITERS] < MAXITER
    assert 0.9 * lo - 2 <= rec[mr.ITERS] <= 1.1 * hi + 2
    assert rec[mr.PHIBAR] <= rec[mr.THR] and rec[mr.FRESH] == 0.0
    b = inp["b"]
    assert rec[mr.THR] == np.float64(TOL) * np.sqrt(np.float64(cg.dot(b * (b if minv is None else minv * b))))
    assert res <= 2 * TOL * nb
    assert abs(rec[mr.PHIBAR] / res - 1.0) < 1e-2
    if family == "quasi":
        err = np.max(np.abs(x - scipy.sparse.linalg.spsolve(inp["K"], b)))
        bound = mr.residual_bound_2norm(TOL, b, minv) / mr.LAMBDA_QUASI
        print(f"    error {err:.3e}: {err / (np.linalg.norm(r) / mr.LAMBDA_QUASI):.3f} of |r|_2 / 0.05, {err / bound:.3f} of the derived bound")
        assert err <= np.linalg.norm(r) / mr.LAMBDA_QUASI and err <= bound


def test_the_factor_two_stands(solved):
    """The emulator's worst true residual is at most tol |b|_M, with and without x0: the factor 2 of the bound is kept."""
    worst = 0.0
    for (ctx, family, with_h, pre), (inp, minv, x, _) in solved.items():
        x_cold, _ = mr.emulate_solve(mr.kkt(ctx), with_h, inp["s1"], inp["s2"], minv, inp["b"], None, TOL, MAXITER)
        for sol in (x, x_cold):
            worst = max(worst, mr.m_norm(inp["b"] - inp["K"] @ sol, minv) / (TOL * mr.m_norm(inp["b"], minv)))
    print(f"worst M-norm residual: {worst:.4f} tol |b|_M")
    assert worst <= 1.0


@pytest.mark.parametrize("ctx,family,with_h,pre", [s for s in SOLVES if s[3] or s[0] == "A"])
def test_x_the_record_and_the_status_do_not_depend_on_check_every(ctx, family, with_h, pre, solved):
    inp, minv, x, rec = solved[ctx, family, with_h, pre]
    for ce in (1, 3, 8, 64):
        x2, rec2 = mr.emulate_solve(mr.kkt(ctx), with_h, inp["s1"], inp["s2"], minv, inp["b"], inp["x0"], TOL, MAXITER, check_every=ce)
        assert sc.same_bits(x, x2) and sc.same_bits(rec, rec2), ce
        assert rec2[mr.FRESH] == 0.0


def test_exhaustion_is_status_4_and_slot_15_is_0(solved):
    inp, minv, _, rec = solved["A", "quasi", True, True]
    k = int(rec[mr.ITERS]) - 2
    x3, rec3 = mr.emulate_solve(mr.kkt("A"), True, inp["s1"], inp["s2"], minv, inp["b"], inp["x0"], TOL, k, check_every=3)
    assert rec3[mr.STATUS] == 4.0 and rec3[mr.ITERS] == k and rec3[mr.FRESH] == 0.0 and np.all(np.isfinite(x3))


def test_a_negative_entry_of_the_callers_minv_ends_in_status_2(solved):
    inp, minv, _, _ = solved["A", "quasi", True, True]
    bad = minv.copy()
    bad[:] = -minv                                           # r.Mr < 0 at once
    x, rec = mr.emulate_solve(mr.kkt("A"), True, inp["s1"], inp["s2"], bad, inp["b"], None, TOL, MAXITER)
    assert rec[mr.STATUS] == 2.0 and rec[mr.ITERS] == 0.0 and np.all(x == 0.0)
    bad = minv.copy()
    bad[5] = -40.0 * minv[5]                                 # one entry: r.Mr turns negative on the way
    x, rec = mr.emulate_solve(mr.kkt("A"), True, inp["s1"], inp["s2"], bad, inp["b"], None, TOL, MAXITER)
    print(f"one negative entry: status {rec[mr.STATUS]} after {int(rec[mr.ITERS])} iterations")
    assert rec[mr.STATUS] == 2.0 and np.all(np.isfinite(x))
    for ce in (1, 64):
        x2, rec2 = mr.emulate_solve(mr.kkt("A"), True, inp["s1"], inp["s2"], bad, inp["b"], None, TOL, MAXITER, check_every=ce)
        assert sc.same_bits(x, x2) and sc.same_bits(rec, rec2)


def test_a_zero_right_hand_side_converges_at_once(solved):
    inp, minv, _, _ = solved["A", "quasi", True, True]
    for x0 in (None, np.zeros(mr.kkt("A").N)):
        x, rec = mr.emulate_solve(mr.kkt("A"), True, inp["s1"], inp["s2"], minv, np.zeros(mr.kkt("A").N), x0, TOL, MAXITER)
        assert rec[mr.STATUS] == 1.0 and rec[mr.ITERS] == 0.0 and np.all(x == 0.0)


def test_the_scalar_step_stops_on_what_it_must():
    rng = np.random.default_rng(2)
    rec = mr.running_record(rng)
    assert mr.scalar_b(rec, -1.0)[mr.STATUS] == 2.0 and mr.scalar_b(rec, np.nan)[mr.STATUS] == 3.0
    assert mr.scalar_b(rec, np.inf)[mr.STATUS] == 3.0
    for out in (mr.scalar_b(rec, -1.0), mr.scalar_b(rec, np.nan)):
        assert sc.same_bits(out[1:], rec[1:])                # nothing but the status moved
    zero = rec.copy()
    zero[mr.DBAR] = zero[mr.ALFA] = 0.0
    out = mr.scalar_b(zero, 0.0)                             # gbar = 0 and beta = 0: gamma == 0
    assert out[mr.STATUS] == 3.0 and out[mr.GAMMA] == 0.0 and out[mr.ITERS] == rec[mr.ITERS] and out[mr.FRESH] == 0.0
    good = mr.scalar_b(rec, 0.75)
    assert good[mr.STATUS] == 0.0 and good[mr.ITERS] == rec[mr.ITERS] + 1 and good[mr.FRESH] == 1.0
    assert abs(good[mr.CS] ** 2 + good[mr.SN] ** 2 - 1.0) < 1e-15
    v = np.array([np.inf])
    assert mr.step_alfa(v, v, rec)[mr.STATUS] == 3.0


# ---------------------------------------------------------------- every deliberate mistake is caught
def _differs(a, b):
    return not (sc.same_bits(a[0], b[0]) and sc.same_bits(a[1], b[1]))


def test_every_mutant_is_caught(solved):
    caught = {}
    kk = mr.kkt("B")
    inp, minv, x, rec = solved["B", "quasi", True, True]
    args = (kk, True, inp["s1"], inp["s2"], minv, inp["b"], inp["x0"], TOL, MAXITER)
    good = (x, rec)
    for mutant in ("fma_x", "s2_sign_dropped", "split_off_by_one", "r1_term_on_first_iteration", "converging_update_skipped",
                   "cs_sn_swapped", "hypot_gamma", "tree_stops_at_2"):
        caught[mutant] = _differs(good, mr.emulate_solve(*args, mutant=mutant))
    # a frozen iteration that still moves w: visible in w and w2 when iterations are enqueued behind the stop
    _, _, state = mr.emulate_solve(*args, check_every=64, full=True)
    _, _, moved = mr.emulate_solve(*args, check_every=64, full=True, mutant="frozen_moves_w")
    assert int(rec[mr.ITERS]) % 64 != 0
    caught["frozen_moves_w"] = not (sc.same_bits(state["w"], moved["w"]) and sc.same_bits(state["w2"], moved["w2"]))
    _, _, short = mr.emulate_solve(*args, check_every=1, full=True)
    assert all(sc.same_bits(state[k], short[k]) for k in state)          # (the emulator itself freezes all six vectors)
    # the second strided trip of the scalar step: more than 256 pieces
    v = mr.step_vectors(524289)
    caught["strided_first_trip"] = mr.dot(v["v"] * v["q"]) != mr.dot(v["v"] * v["q"], "strided_first_trip")
    assert set(caught) == set(mr.MUTANTS) and len(caught) >= 8
    assert all(caught.values()), caught


def test_the_hypot_mutant_differs_from_the_rounded_products():
    """hypot rounds once; the unit rounds gbar^2, beta^2 and their sum before the root."""
    rng = np.random.default_rng(8)
    a, b = rng.uniform(0.5, 2.0, 4000), rng.uniform(0.5, 2.0, 4000)
    assert np.any(np.hypot(a, b) != np.sqrt(a * a + b * b))
