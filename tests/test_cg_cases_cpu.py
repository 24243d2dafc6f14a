"""tests/cg_cases.py tested on the CPU: the emulator of the device's CG solve converges to ``spsolve`` on the same matrices within
the derived bound, does not depend on ``check_every``, stops on non-positive curvature on the indefinite family, and every
deliberate mistake (cg_cases.MUTANTS) is caught by the bit comparison the GPU file makes.

The bound: CG stops at ``|r| <= tol |b|`` in the recurrence; the true residual is held to ``2 tol |b|`` (the recurrence drifts
from ``b - K x`` by rounding, orders below tol at these condition numbers), and ``e = K^-1 r`` gives
``max|x - x*| <= |e|_2 <= 2 tol |b|_2 / lambda`` with ``lambda <= lambda_min(K)`` known by construction (cg_cases.LAMBDA)."""
import numpy as np
import pytest
import scipy.sparse.linalg

import cg_cases as cg
import sparse_cases as sc

TOL, MAXITER = 1e-8, 400
SOLVES = [(ctx, form) for ctx in ("A", "B") for form in (0, 1)]


@pytest.fixture(scope="module")
def solved():
    """{(ctx, form): (inputs, minv, x, rec)} of the pd family with x0 and the Jacobi preconditioner: computed once."""
    out = {}
    for ctx, form in SOLVES:
        sy = cg.system(ctx)
        inp = sy.inputs(form, "pd")
        minv = sy.jacobi(form, inp["with_h"], inp["d"], inp["s"])
        x, rec = cg.emulate_solve(sy, form, inp["with_h"], inp["d"], inp["s"], minv, inp["b"], inp["x0"], TOL, MAXITER)
        out[ctx, form] = (inp, minv, x, rec)
    return out


def test_the_systems_have_the_shapes_the_walk_needs():
    a, b = cg.system("A"), cg.system("B")
    assert (a.n, a.m, b.n, b.m) == (53, 36, 1205, 900)
    assert b.has_long and not a.has_long
    _, longs, _ = sc.row_blocks(b.JT.indptr)
    assert len(longs) == 1 and longs[0][2] == 2            # one column of more than 256 entries: two pieces, pk_op_long
    for sy in (a, b):
        assert sy.J.src.max() < sc.CONTEXTS[sy.ctx]["nnz_j"] and sy.H.src.max() < sc.CONTEXTS[sy.ctx]["nnz_h"]
        assert np.array_equal(sy.JT.matrix(sy.jvals).toarray(), sy.Jm.T.toarray())
        assert np.array_equal(sy.hvals[sy.diag_pos], sy.Hm.diagonal())


@pytest.mark.parametrize("ctx,form", SOLVES)
def test_the_pd_family_is_positive_definite_by_construction(ctx, form):
    inp = cg.system(ctx).inputs(form, "pd")
    lam = np.linalg.eigvalsh(inp["K"].toarray())
    print(f"{ctx} form {form}: lambda in [{lam[0]:.3f}, {lam[-1]:.3f}]")
    assert lam[0] >= cg.LAMBDA[form]


@pytest.mark.parametrize("ctx,form", SOLVES)
def test_the_emulated_product_and_diagonal_are_the_matrix(ctx, form):
    sy = cg.system(ctx)
    inp = sy.inputs(form, "pd")
    v = inp["x0"]
    y = sy.kv(form, inp["with_h"], inp["d"], inp["s"], v)
    ref = inp["K"] @ v
    assert np.max(np.abs(y - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
    minv = sy.jacobi(form, inp["with_h"], inp["d"], inp["s"])
    assert np.allclose(minv, 1.0 / np.abs(inp["K"].diagonal()), rtol=1e-13, atol=0.0)


@pytest.mark.parametrize("ctx,form", SOLVES)
def test_the_emulator_converges_to_spsolve_within_the_derived_bound(ctx, form, solved):
    inp, _, x, rec = solved[ctx, form]
    ref = scipy.sparse.linalg.spsolve(inp["K"], inp["b"])
    nb = np.linalg.norm(inp["b"])
    res = np.linalg.norm(inp["b"] - inp["K"] @ x)
    err = np.max(np.abs(x - ref))
    print(f"{ctx} form {form}: {int(rec[cg.ITERS])} iterations, residual {res:.3e} (bound {2 * TOL * nb:.3e}), "
          f"error {err:.3e} (bound {2 * TOL * nb / cg.LAMBDA[form]:.3e})")
    assert rec[cg.STATUS] == 1.0 and 0 < rec[cg.ITERS] < MAXITER
    assert rec[cg.RR] <= rec[cg.THR] and rec[cg.THR] == (TOL * TOL) * cg.dot(inp["b"] * inp["b"])
    assert res <= 2 * TOL * nb
    assert err <= 2 * TOL * nb / cg.LAMBDA[form]


@pytest.mark.parametrize("ctx,form", SOLVES)
def test_x_iterations_and_status_do_not_depend_on_check_every(ctx, form, solved):
    inp, minv, x, rec = solved[ctx, form]
    sy = cg.system(ctx)
    for ce in (1, 3, 8, 64):
        x2, rec2 = cg.emulate_solve(sy, form, inp["with_h"], inp["d"], inp["s"], minv, inp["b"], inp["x0"], TOL, MAXITER, check_every=ce)
        assert sc.same_bits(x, x2) and sc.same_bits(rec, rec2), ce


def test_exhaustion_is_status_4_and_a_prefix_of_the_longer_solve(solved):
    inp, minv, _, rec = solved["A", 0]
    sy = cg.system("A")
    k = int(rec[cg.ITERS]) - 2
    x3, rec3 = cg.emulate_solve(sy, 0, inp["with_h"], inp["d"], inp["s"], minv, inp["b"], inp["x0"], TOL, k, check_every=3)
    assert rec3[cg.STATUS] == 4.0 and rec3[cg.ITERS] == k and np.all(np.isfinite(x3))


@pytest.mark.parametrize("ctx,form", SOLVES)
def test_the_indefinite_family_ends_on_non_positive_curvature(ctx, form):
    sy = cg.system(ctx)
    inp = sy.inputs(form, "indefinite")
    lam = np.linalg.eigvalsh(inp["K"].toarray())
    assert lam[0] < 0.0
    x, rec = cg.emulate_solve(sy, form, inp["with_h"], inp["d"], inp["s"], None, inp["b"], None, TOL, MAXITER)
    print(f"{ctx} form {form}: status {rec[cg.STATUS]} after {int(rec[cg.ITERS])} iterations, pq = {rec[cg.PQ]:.3e}")
    assert rec[cg.STATUS] == 2.0 and rec[cg.PQ] <= 0.0 and np.all(np.isfinite(x))
    for ce in (1, 3, 64):
        x2, rec2 = cg.emulate_solve(sy, form, inp["with_h"], inp["d"], inp["s"], None, inp["b"], None, TOL, MAXITER, check_every=ce)
        assert sc.same_bits(x, x2) and sc.same_bits(rec, rec2)


def test_the_dot_is_the_documented_association_and_exact_on_small_integers():
    rng = np.random.default_rng(3)
    for length in (0, 1, 255, 256, 257, 2047, 2048, 2049, 524289):
        t = rng.integers(-8, 9, length).astype(np.float64)
        assert cg.dot(t) == float(t.sum())
    # thread t of piece 0 owns t, t + 256, ...: a term 2**60 at index 0 absorbs a 1.0 at 256 (the same thread's next term)
    t = np.zeros(2048)
    t[0], t[256] = 2.0 ** 60, 1.0
    assert cg.dot(t) == 2.0 ** 60
    t[256], t[1] = 0.0, 1.0
    assert cg.dot(t) == 2.0 ** 60          # (the tree adds slot 1 to slot 0 last: absorbed there too)
    t = np.zeros(2048)
    t[1], t[2], t[3] = 1.0, 2.0 ** 53, 1.0     # width 2: slot 0 += slot 2, slot 1 += slot 3 = 2.0; width 1: 2**53 + 2 is exact
    assert cg.dot(t) == 2.0 ** 53 + 2.0        # (a sequential sum would lose both ones)


# ---------------------------------------------------------------- every deliberate mistake is caught
def _differs(a, b):
    return not (sc.same_bits(a[0], b[0]) and sc.same_bits(a[1], b[1]))


def test_every_mutant_is_caught(solved):
    caught = {}
    sy = cg.system("B")
    inp, minv, x, rec = solved["B", 0]
    args = (sy, 0, inp["with_h"], inp["d"], inp["s"], minv, inp["b"], inp["x0"], TOL, MAXITER)
    good = (x, rec)
    for mutant in ("fma_x", "beta_inverted", "thr_from_r0", "tree_stops_at_2"):
        caught[mutant] = _differs(good, cg.emulate_solve(*args, mutant=mutant))
    # a frozen iteration that still moves x: visible only when iterations are enqueued behind the stop
    caught["frozen_moves_x"] = _differs(cg.emulate_solve(*args, check_every=64), cg.emulate_solve(*args, check_every=64, mutant="frozen_moves_x"))
    assert sc.same_bits(cg.emulate_solve(*args, check_every=64)[0], x)
    # minv == NULL read as 0: a solve without a preconditioner
    plain = args[:5] + (None,) + args[6:]
    caught["minv_null_zero"] = _differs(cg.emulate_solve(*plain), cg.emulate_solve(*plain, mutant="minv_null_zero"))
    # d indexed by the wrong side: the dual form, where d has n values and the system m
    inp1, minv1, x1, rec1 = solved["B", 1]
    dual = (sy, 1, False, inp1["d"], inp1["s"], minv1, inp1["b"], inp1["x0"], TOL, MAXITER)
    caught["d_wrong_side"] = _differs((x1, rec1), cg.emulate_solve(*dual, mutant="d_wrong_side"))
    # the second strided trip of the scalar step: more than 256 pieces
    v = cg.step_vectors(524289)
    caught["strided_first_trip"] = cg.dot(v["p"] * v["q"]) != cg.dot(v["p"] * v["q"], "strided_first_trip")
    assert set(caught) == set(cg.MUTANTS)
    assert all(caught.values()), caught


def test_the_fma_mutant_is_a_single_rounding():
    a, b, c = np.array([1.0 + 2.0 ** -30]), np.array([1.0 + 2.0 ** -30]), np.array([-1.0])
    assert cg._fma(a, b, c)[0] == 2.0 ** -29 + 2.0 ** -60 and (a * b + c)[0] == 2.0 ** -29
