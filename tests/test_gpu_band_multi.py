"""The block solve of the bordered band LU (pockit_amd/csrc/pk_band.cpp: k right-hand sides against one factorisation in the
launches of one solve) on the device.

Synthetic systems through ``pk_band_raw_multi_dev`` on the context of brachistochrone(radau, 3, 4): the shapes of
tests/band_multi_cases.py (Nb = 1, 33, 65, 257, w = 0, 7, 33, 192, p = 0, 1, 8, k = 1, 2, 9, 64), full-mantissa data, NaN in the
fill rows, outside the matrix and in the gaps between right-hand sides and between solutions.  Every column, the interchanges
and the record bit-equal to the emulator (the single solve of tests/band_cases.py column by column) and to k calls of
``pk_band_raw_dev`` -- the code that was there before, so a reference; the same bits from a second call; sentinels and gaps
intact; a planted NaN confined to its column; a zero pivot writes nothing; the refusals; one long case Nb = 4 500, w = 8, p = 1,
k = 64 (three pieces per dot) against 64 single device solves, and Nb = 64 000, w = 1, p = 1, k = 64, where the dot kernel's
stride loop takes a second trip.

Two models of tests/test_gpu_csr_operators.py (p = 1 and 2): ``solve_banded_multi`` with k = 5 against five ``solve_banded``,
bit-equal; 70 right-hand sides (two chunks against one factorisation); ``solve_banded``, ``solve_banded_batch``, ``solve_kkt``
and ``jv`` return the bits they returned before."""
import numpy as np
import pytest

import band_cases as bc
import band_multi_cases as bm
import sparse_cases as sc
from device_cases import Buf, _ptr, _same, _sync, _up, step_ev  # noqa: F401  (step_ev: a fixture)
from test_gpu_band import _poisoned, _raw
from test_gpu_csr_operators import Case

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]


def _raw_multi(ev, AB, U, C, R, check=True):
    """One call of the raw block form: (band, ipiv, X with its gaps (k, stride), rec) as they come down, or the error code."""
    ldab, nb = AB.shape
    w, p, (k, stride) = (ldab - 1) // 3, C.shape[0], R.shape
    band = Buf(ldab * nb, _poisoned(AB, w).ravel(order="F"))
    dU, dC = (_up(a.ravel(order="F")) if a.size else _up(np.zeros(1)) for a in (U, C))
    drhs = _up(R.ravel()) if R.size else _up(np.zeros(1))
    piv, x, rec = Buf((nb + 1) // 2 + 1), Buf(k * stride), Buf(8)
    _sync()
    rc = ev.ctx.lib.pk_band_raw_multi_dev(ev.ctx.handle, nb, w, p, k, band.ptr, _ptr(dU), _ptr(dC), _ptr(drhs), stride, piv.ptr, x.ptr, stride,
                                          rec.ptr)
    if not check:
        return rc
    ev.ctx.check(rc)
    ev.sync()
    ipiv = piv.fetch().view(np.int32)[:nb].astype(np.int64)
    return band.fetch().reshape((ldab, nb), order="F"), ipiv, x.fetch().reshape(k, stride), rec.fetch()


def _bits(a, b):
    return sc.same_bits(np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64))


@pytest.mark.parametrize("nb,w,p", [(nb, w, p) for nb in bm.GPU_NB_SHAPES for w in bm.W_SHAPES for p in bm.P_SHAPES], ids=lambda v: str(v))
def test_every_column_matches_the_emulator_and_the_single_form_bit_for_bit(step_ev, nb, w, p):
    ev, N, gap = step_ev, nb + p, 3 * ((nb + w + p) % 2)
    AB, U, C, R = bm.block(nb, w, p, bm.RHS_CAP, seed=1, gap=gap)
    w_band, w_ipiv, w_X, w_rec = bm.solve_columns(AB, U, C, R)
    assert w_rec[bc.STATUS] == 0.0
    inside = bc.in_band(nb, w) | bc.fill_rows(nb, w)
    for k in bm.K_SHAPES:
        what = f"Nb {nb} w {w} p {p} k {k} gap {gap}"
        first, second = _raw_multi(ev, AB, U, C, R[:k]), _raw_multi(ev, AB, U, C, R[:k])
        band, ipiv, X, rec = first
        for name, a, b in zip(("band", "ipiv", "X", "record"), first, second):
            assert _bits(a, b), f"{what} {name}: a second call gave other bits"
        _same(f"{what} record", rec, w_rec)
        assert np.array_equal(ipiv, w_ipiv), what
        _same(f"{what} band", np.ascontiguousarray(band[inside]), np.ascontiguousarray(w_band[inside]))
        assert np.all(np.isnan(band[~inside])), f"{what}: a slot outside the matrix was written"
        _same(f"{what} solutions", np.ascontiguousarray(X[:, :N]), w_X[:k])
        assert np.all(np.isnan(X[:, N:])), f"{what}: a gap between two solutions was written"
    for c in range(bm.RHS_CAP):            # the single device form, column by column: what the block must reproduce
        s_band, s_ipiv, s_x, s_rec = _raw(ev, AB, U, C, R[c, :N])
        assert _bits(s_x, X[c, :N]) and _bits(s_rec, rec) and np.array_equal(s_ipiv, ipiv) and _bits(s_band[inside], band[inside]), (nb, w, p, c)


def test_the_long_block_against_single_device_solves(step_ev):
    nb, w, p, k = bm.LONG
    AB, U, C, R = bm.block(nb, w, p, k, seed=1, gap=3)
    band, ipiv, X, rec = _raw_multi(step_ev, AB, U, C, R)
    assert rec[bc.STATUS] == 0.0 and rec[bc.R_NB] == nb and np.all(np.isnan(X[:, nb + p:]))
    inside = bc.in_band(nb, w) | bc.fill_rows(nb, w)
    for c in range(k):
        s_band, s_ipiv, s_x, s_rec = _raw(step_ev, AB, U, C, R[c, : nb + p])
        assert _bits(s_x, X[c, : nb + p]) and _bits(s_rec, rec) and np.array_equal(s_ipiv, ipiv), c
    assert _bits(s_band[inside], band[inside])
    _, _, again, _ = _raw_multi(step_ev, AB, U, C, R)
    assert _bits(again, X)


def test_the_dot_kernel_takes_its_stride_loop_to_a_second_trip(step_ev):
    """Nb has no cap: at Nb = 64 000, p = 1, k = 64 the dots are 65 * 32 = 2 080 work items for a grid of 2 048, so 32 workgroups go
    round again, through the barriers and the reused LDS planes; the items of the second trip are the pieces of the LAST column."""
    nb, w, p, k = 64000, 1, 1, bm.RHS_CAP
    assert (p + k) * -(-nb // 2048) > bm.GRID_CAP and (p + k - 1) * -(-nb // 2048) <= bm.GRID_CAP
    AB, U, C, R = bm.block(nb, w, p, k, seed=2, gap=0)
    band, ipiv, X, rec = _raw_multi(step_ev, AB, U, C, R)
    assert rec[bc.STATUS] == 0.0 and rec[bc.R_NB] == nb
    for c in (0, 40, k - 1):
        _, s_ipiv, s_x, s_rec = _raw(step_ev, AB, U, C, R[c])
        assert _bits(s_x, X[c]) and _bits(s_rec, rec) and np.array_equal(s_ipiv, ipiv), c
    assert _bits(_raw_multi(step_ev, AB, U, C, R)[2], X)


def test_a_planted_nan_stays_in_its_column(step_ev):
    AB, U, C, R = bm.block(2 * bc.NB + 1, 7, 3, 5, seed=4, gap=3)
    _, _, clean, _ = _raw_multi(step_ev, AB, U, C, R)
    R[2, 11] = np.nan
    _, _, X, rec = _raw_multi(step_ev, AB, U, C, R)
    want = bm.solve_columns(AB, U, C, R)[2]
    N = want.shape[1]
    assert rec[bc.STATUS] == 0.0 and np.isnan(X[2, :N]).any()
    assert all(_bits(X[c], clean[c]) for c in (0, 1, 3, 4))
    for c in (0, 1, 3, 4):
        _same(f"column {c} beside the NaN", X[c, :N].copy(), want[c])
    poisoned = np.isnan(want[2])      # (a NaN's sign and payload are not compared: which entries it reaches, and the bits of the others)
    assert np.array_equal(np.isnan(X[2, :N]), poisoned) and _bits(X[2, :N][~poisoned], want[2][~poisoned])


@pytest.mark.parametrize("nb,w,p", [(3 * bc.NB + 5, 7, 1), (2 * bc.NB + 1, bc.NB + 1, 0)])
def test_a_zero_pivot_writes_no_column(step_ev, nb, w, p):
    AB, U, C, R = bm.block(nb, w, p, 9, seed=4, gap=3, variant="zero_column")
    _, _, X, rec = _raw_multi(step_ev, AB, U, C, R)
    w_rec = bm.solve_columns(AB, U, C, R)[3]
    _same("the record", rec, w_rec)
    assert rec[bc.STATUS] == 1.0 and rec[bc.COLUMN] == bc.failing_column(nb, "zero_column") and np.all(np.isnan(X))


def test_refusals_of_the_raw_block_form(step_ev):
    ev = step_ev
    lib, h = ev.ctx.lib, ev.ctx.handle
    AB, U, C, R = bm.block(40, 7, 1, 3)
    band, dU, dC, drhs = Buf(AB.size, AB.ravel(order="F")), _up(U.ravel(order="F")), _up(C.ravel(order="F")), _up(R.ravel())
    piv, x, rec = Buf(21), Buf(3 * 41), Buf(8)
    _sync()

    def call(nb=40, w=7, p=1, k=3, s_rhs=41, s_x=41, drop=None):
        args = [band.ptr, _ptr(dU), _ptr(dC), _ptr(drhs), s_rhs, piv.ptr, x.ptr, s_x, rec.ptr]
        if drop is not None:
            args[drop] = None
        return lib.pk_band_raw_multi_dev(h, nb, w, p, k, *args)

    assert call(nb=-1) == 134 and call(w=bc.W_CAP + 1) == 134 and call(w=-1) == 134 and call(p=bc.P_CAP + 1) == 134
    assert call(k=0) == 134 and call(k=bm.RHS_CAP + 1) == 134 and call(k=-1) == 134
    assert call(s_rhs=40) == 134 and call(s_x=40) == 134 and call(s_rhs=0) == 134
    for drop in (0, 1, 2, 3, 5, 6, 8):
        assert call(drop=drop) == 110
    ev.sync()
    for b in (piv, x, rec):
        assert np.all(np.isnan(b.fetch()))
    assert sc.same_bits(band.fetch(), AB.ravel(order="F"))


# ---------------------------------------------------------------- models
MODELS = [("brachistochrone", "radau", 60, 5), ("two_stage_rocket", "radau", 6, 4)]


@pytest.fixture(scope="module", params=MODELS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def case(request):
    c = Case(*request.param)
    p = c.system.evaluator.plan
    rng = np.random.default_rng(29)
    ineq = np.asarray(p.c_lb, dtype=np.float64) != np.asarray(p.c_ub, dtype=np.float64)
    c.s1, c.s2 = rng.uniform(0.5, 1.5, c.n), np.where(ineq, rng.uniform(0.5, 1.5, c.m), 0.0)
    c.B = rng.uniform(-1.0, 1.0, (70, c.n + c.m))
    yield c
    c.system.evaluator.close()


def test_solve_banded_multi_matches_solve_banded_row_by_row(case):
    lin = case.linearize()
    singles = [lin.solve_banded(case.B[c], s1=case.s1, s2=case.s2) for c in range(5)]
    X, info = lin.solve_banded_multi(case.B[:5], s1=case.s1, s2=case.s2)
    again, _ = lin.solve_banded_multi(case.B[:5], s1=case.s1, s2=case.s2)
    assert info.status == "solved" and info.border == (1 if case.system.n_p == 1 else 2), info
    assert X.shape == (5, case.n + case.m) and _bits(X, again)
    for c, (x, one) in enumerate(singles):
        assert _bits(X[c], x) and _bits(info.record, one.record), c


def test_seventy_right_hand_sides_are_served_in_chunks_against_one_factorisation(case):
    lin = case.linearize()
    X, info = lin.solve_banded_multi(case.B, s1=case.s1, s2=case.s2)
    assert info.status == "solved" and X.shape == case.B.shape
    for c in (0, 63, 64, 69):
        x, _ = lin.solve_banded(case.B[c], s1=case.s1, s2=case.s2)
        assert _bits(X[c], x), c
    with pytest.raises(ValueError):
        lin.solve_banded_multi(case.B[0], s1=case.s1, s2=case.s2)
    with pytest.raises(ValueError):
        lin.solve_banded_multi(case.B[:0], s1=case.s1, s2=case.s2)


def test_the_other_products_of_the_handle_keep_their_bits(case):
    lin = case.linearize()
    rhs = case.B[7]

    def products():
        x, _ = lin.solve_banded(rhs, s1=case.s1, s2=case.s2)
        Xb, _ = lin.solve_banded_batch(case.B[:3], s1=case.s1, s2=case.s2)
        sol, _ = lin.solve_kkt(rhs, s1=case.s1, s2=case.s2, precond=None, tol=0.0, maxiter=6, check_every=6)
        return x, Xb, sol, lin.jv(case.v)

    before = products()
    lin.solve_banded_multi(case.B[:9], s1=case.s1, s2=case.s2)
    after = products()
    for a, b in zip(before, after):
        assert _bits(a, b)


def test_refusals_of_the_planned_block_forms(case):
    from pockit_amd import runtime

    ev = case.system.evaluator
    lib, h = ev.ctx.lib, ev.ctx.handle
    as_dp = runtime.as_dp
    N = case.n + case.m
    lin = case.linearize()
    lin.solve_banded(case.B[0], s1=case.s1, s2=case.s2)           # (planned and factored)
    rhs, sol = _up(case.B[:3].ravel()), Buf(3 * N)
    hx, hrec = np.full(3 * N, -3.0), np.full(8, -3.0)
    _sync()
    assert lib.pk_band_solve_multi_dev(h, 3, None, N, sol.ptr, N) == 110 and lib.pk_band_solve_multi_dev(h, 3, _ptr(rhs), N, None, N) == 110
    assert lib.pk_band_solve_multi_dev(h, 0, _ptr(rhs), N, sol.ptr, N) == 134 and lib.pk_band_solve_multi_dev(h, 65, _ptr(rhs), N, sol.ptr, N) == 134
    assert lib.pk_band_solve_multi_dev(h, 3, _ptr(rhs), N - 1, sol.ptr, N) == 134 and lib.pk_band_solve_multi_dev(h, 3, _ptr(rhs), N, sol.ptr, N - 1) == 134
    b3 = np.ascontiguousarray(case.B[:3])
    assert lib.pk_solve_banded_multi(h, 3, None, as_dp(case.s2), as_dp(b3), as_dp(hx), as_dp(hrec)) == 60
    assert lib.pk_solve_banded_multi(h, 3, as_dp(case.s1), as_dp(case.s2), as_dp(b3), None, as_dp(hrec)) == 60
    assert lib.pk_solve_banded_multi(h, 0, as_dp(case.s1), as_dp(case.s2), as_dp(b3), as_dp(hx), as_dp(hrec)) == 134
    assert lib.pk_solve_banded_multi(h, 65, as_dp(case.s1), as_dp(case.s2), as_dp(b3), as_dp(hx), as_dp(hrec)) == 134
    ev.sync()
    assert np.all(np.isnan(sol.fetch())) and np.all(hx == -3.0) and np.all(hrec == -3.0)
    ev.band_plan(__import__("pockit_amd.band", fromlist=["BandOrdering"]).BandOrdering(
        ev.csr_map("jac"), ev.csr_map("hess"), np.asarray(ev.plan.v_lb, dtype=np.float64) != np.asarray(ev.plan.v_ub, dtype=np.float64)))
    assert lib.pk_band_solve_multi_dev(h, 3, _ptr(rhs), N, sol.ptr, N) == 134      # a new plan: no factorisation
    ev.sync()
    assert np.all(np.isnan(sol.fetch()))
