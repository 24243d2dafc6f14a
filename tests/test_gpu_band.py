"""The bordered band LU of the step's system (pockit_amd/csrc/pk_band.cpp) on the device.

Synthetic systems through ``pk_band_raw_dev`` on the context of brachistochrone(radau, 3, 4): the shapes of the CPU driver
(band_cases.shapes(): Nb = 0, 1, 2, NB - 1, NB, NB + 1, 2 NB + 1 and w + 1, w = 0, 1, 7, NB - 1, NB, NB + 1 and the cap, p = 0,
1, 3 and the cap) and one long system Nb = 50 001, w = 8, p = 1 (1 563 panels, 25 pieces per dot).  Full-mantissa data, NaN in
the fill rows and in the slots outside the matrix (a kernel must not read either), outputs between sentinels in NaN-filled
tensors; band, interchanges, solution and record bit-equal to the emulator of tests/band_cases.py, the same bits from a second
call; the every-column-interchanges and tie variants; a zero column and a planted NaN give status 1 and 3 with the right
column and the solution untouched; the refusals.

The six models of tests/test_gpu_csr_operators.py with the plan's own row classification (section 22's: ``c_lb == c_ub`` is an
equality row with ``s2 = 0``): the device fill bit-equal to ``BandOrdering.assemble``; ``solve_banded`` bit-equal to the
emulator on the same values; its residual ``|K x - b|_inf``, computed with NumPy in extended precision from the downloaded
values, at most 16 times the residual of ``DirectKkt.solve`` (``splu``) on the same system plus a floor of
``N 2^-52 (|K|_inf |x|_inf + |b|_inf)``; ``solve_kkt``, ``jv`` and ``slack_terms`` return the bits they returned before."""
import numpy as np
import pytest

import band_cases as bc
import sparse_cases as sc
from device_cases import Buf, _ptr, _same, _sync, _up, step_ev  # noqa: F401  (step_ev: a fixture)
from test_gpu_csr_operators import CASES, Case

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]


def _poisoned(AB, w):
    """The band with NaN in the fill rows and in the slots outside the matrix."""
    nb = AB.shape[1]
    out = np.full(AB.shape, np.nan, order="F")
    keep = bc.in_band(nb, w)
    out[keep] = AB[keep]
    return out


def _raw(ev, AB, U, C, rhs):
    """One call of the raw form: (band, ipiv, x, rec) as they come down."""
    ldab, nb = AB.shape
    w, p = (ldab - 1) // 3, C.shape[0]
    band = Buf(ldab * nb, _poisoned(AB, w).ravel(order="F"))
    dU, dC = (_up(a.ravel(order="F")) if a.size else _up(np.zeros(1)) for a in (U, C))
    drhs = _up(rhs) if len(rhs) else _up(np.zeros(1))
    piv, x, rec = Buf((nb + 1) // 2 + 1), Buf(nb + p), Buf(8)
    _sync()
    rc = ev.ctx.lib.pk_band_raw_dev(ev.ctx.handle, nb, w, p, p + 1, band.ptr, _ptr(dU), _ptr(dC), _ptr(drhs), piv.ptr, x.ptr, rec.ptr)
    ev.ctx.check(rc)
    ev.sync()
    ipiv = piv.fetch().view(np.int32)[:nb].astype(np.int64)
    return band.fetch().reshape((ldab, nb), order="F"), ipiv, x.fetch(), rec.fetch()


def _check_raw(ev, nb, w, p, variant, seed=1):
    AB, U, C, rhs = bc.system(nb, w, p, seed=seed, variant=variant)
    first, second = _raw(ev, AB, U, C, rhs), _raw(ev, AB, U, C, rhs)
    w_band, w_ipiv, w_x, w_rec = bc.solve_system(AB, U, C, rhs)
    what = f"Nb {nb} w {w} p {p} {variant}"
    band, ipiv, x, rec = first
    for name, a, b in zip(("band", "ipiv", "x", "record"), first, second):
        assert sc.same_bits(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)), f"{what} {name}: a second call gave other bits"
    _same(f"{what} record", rec, w_rec)
    if w_x is None:
        assert np.all(np.isnan(x)), f"{what}: the solution was written behind a failed pivot"
        return rec
    inside = bc.in_band(nb, w) | bc.fill_rows(nb, w)
    assert np.array_equal(ipiv, w_ipiv), what
    _same(f"{what} band", np.ascontiguousarray(band[inside]), np.ascontiguousarray(w_band[inside]))
    assert np.all(np.isnan(band[~inside])), f"{what}: a slot outside the matrix was written"
    _same(f"{what} solution", x, w_x)
    return rec


@pytest.mark.parametrize("nb,w,p", bc.shapes(), ids=lambda v: str(v))
def test_the_kernels_match_the_emulator_bit_for_bit(step_ev, nb, w, p):
    rec = _check_raw(step_ev, nb, w, p, "plain")
    assert rec[bc.STATUS] == 0.0
    rec = _check_raw(step_ev, nb, w, p, "tiny_diagonal")
    assert rec[bc.STATUS] == 0.0
    if w > 0 and 1 < nb <= bc.EVERY:
        assert rec[bc.SWAPS] == nb - 1          # every column but the last interchanges


def test_the_long_system(step_ev):
    nb, w, p = bc.LONG
    rec = _check_raw(step_ev, nb, w, p, "plain")
    assert rec[bc.STATUS] == 0.0 and rec[bc.R_NB] == nb


@pytest.mark.parametrize("nb,w,p", [(2 * bc.NB + 1, 7, 1), (3 * bc.NB + 5, bc.NB + 1, 3), (5, 7, 0)])
def test_ties_go_to_the_lowest_row(step_ev, nb, w, p):
    rec = _check_raw(step_ev, nb, w, p, "ties")
    assert rec[bc.STATUS] == 0.0


@pytest.mark.parametrize("variant,status", [("zero_column", 1.0), ("nan", 3.0)])
@pytest.mark.parametrize("nb,w,p", [(3 * bc.NB + 5, 7, 1), (2 * bc.NB + 1, bc.NB + 1, 0)])
def test_a_failed_pivot_sets_the_record_and_leaves_the_solution(step_ev, nb, w, p, variant, status):
    rec = _check_raw(step_ev, nb, w, p, variant)
    assert rec[bc.STATUS] == status and rec[bc.COLUMN] == bc.failing_column(nb, variant)


def test_refusals_of_the_raw_form(step_ev):
    ev = step_ev
    lib, h = ev.ctx.lib, ev.ctx.handle
    AB, U, C, rhs = bc.system(40, 7, 1)
    band, dU, dC, drhs = Buf(AB.size, AB.ravel(order="F")), _up(U.ravel(order="F")), _up(C.ravel(order="F")), _up(rhs)
    piv, x, rec = Buf(21), Buf(41), Buf(8)
    _sync()
    args = [band.ptr, _ptr(dU), _ptr(dC), _ptr(drhs), piv.ptr, x.ptr, rec.ptr]
    assert lib.pk_band_raw_dev(h, -1, 7, 1, 2, *args) == 134
    assert lib.pk_band_raw_dev(h, 40, bc.W_CAP + 1, 1, 2, *args) == 134
    assert lib.pk_band_raw_dev(h, 40, -1, 1, 2, *args) == 134
    assert lib.pk_band_raw_dev(h, 40, 7, bc.P_CAP + 1, bc.P_CAP + 2, *args) == 134
    assert lib.pk_band_raw_dev(h, 40, 7, 1, 1, *args) == 134
    for k in range(7):
        bad = list(args)
        bad[k] = None
        assert lib.pk_band_raw_dev(h, 40, 7, 1, 2, *bad) == 110
    ev.sync()
    for b in (piv, x, rec):
        assert np.all(np.isnan(b.fetch()))
    assert sc.same_bits(band.fetch(), AB.ravel(order="F"))


# ---------------------------------------------------------------- models
class BandInputs:
    """Per model the ordering, the values of the linearization, ``s1``, ``s2`` (0.0 on the plan's equality rows) and ``b``."""

    def __init__(self, case):
        from pockit_amd.band import BandOrdering
        from pockit_amd.optimizer.interior_point import DirectKkt

        ev = case.system.evaluator
        p = ev.plan
        rng = np.random.default_rng(29)
        n, m = case.n, case.m
        self.free = np.asarray(p.v_lb, dtype=np.float64) != np.asarray(p.v_ub, dtype=np.float64)
        ineq = np.asarray(p.c_lb, dtype=np.float64) != np.asarray(p.c_ub, dtype=np.float64)
        self.s1 = rng.uniform(0.5, 1.5, n)
        self.s2 = np.where(ineq, rng.uniform(0.5, 1.5, m), 0.0)
        self.b = rng.uniform(-1.0, 1.0, n + m)
        self.jvals, self.hvals = ev.jacobian_csr(case.x), ev.hessian_csr(case.x, case.lam, case.sigma)
        self.map_j, self.map_h = ev.csr_map("jac"), ev.csr_map("hess")
        self.ordering = BandOrdering(self.map_j, self.map_h, self.free)
        self.direct = DirectKkt(self.map_j, self.map_h, self.free)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def case(request):
    c = Case(*request.param)
    c.band = BandInputs(c)
    yield c
    c.system.evaluator.close()


def _residual(q, x):
    """``|K x - b|_inf`` over the free variables and all rows in extended precision, with ``|K|_inf`` and ``|x|_inf``."""
    d = q.direct
    data = (d.select @ np.concatenate((q.hvals, q.jvals, q.s1, q.s2))).astype(np.longdouble)
    cols = np.repeat(np.arange(d.N), np.diff(d.indptr))
    rows = d.indices.astype(np.int64)
    n = d.n
    y = np.concatenate((x[:n][q.free], x[n:])).astype(np.longdouble)
    b = np.concatenate((q.b[:n][q.free], q.b[n:])).astype(np.longdouble)
    r = -b
    np.add.at(r, rows, data * y[cols])
    norm = np.zeros(d.N, dtype=np.longdouble)
    np.add.at(norm, rows, np.abs(data))
    return float(np.abs(r).max()), float(norm.max()), float(np.abs(y).max()), float(np.abs(b).max())


def test_the_device_fill_is_the_assembly_map(case):
    ev, q = case.system.evaluator, case.band
    ev.band_plan(q.ordering)
    out = Buf(q.ordering.dests)
    d = [_up(a) for a in (q.hvals, q.jvals, q.s1, q.s2)]
    _sync()
    ev.ctx.check(ev.ctx.lib.pk_band_fill_dev(ev.ctx.handle, *[_ptr(t) for t in d], out.ptr))
    ev.sync()
    band, U, Cc = q.ordering.assemble(q.hvals, q.jvals, q.s1, q.s2)
    want = np.concatenate((band.ravel(order="F"), U.ravel(order="F"), Cc.ravel(order="F")))
    _same("the filled [band | U | C]", out.fetch(), want)


def test_solve_banded_matches_the_emulator_and_the_direct_solve(case):
    q = case.band
    lin = case.linearize()
    x, info = lin.solve_banded(q.b, s1=q.s1, s2=q.s2)
    again, _ = lin.solve_banded(q.b, s1=q.s1, s2=q.s2)
    want, rec = bc.emulate(q.ordering, q.hvals, q.jvals, q.s1, q.s2, q.b)
    _same("the record", info.record, rec)
    assert info.status == "solved" and info.width == q.ordering.w and info.border == q.ordering.p, info
    _same("solve_banded", x, want)
    assert sc.same_bits(x, again), "a second call gave other bits"
    assert not x[: case.n][~q.free].any()
    dx, dlam = q.direct.solve(q.hvals, q.jvals, q.s1, q.s2, q.b)
    res, k_inf, x_inf, b_inf = _residual(q, x)
    res_direct, _, _, _ = _residual(q, np.concatenate((dx, dlam)))
    floor = q.direct.N * 2.0 ** -52 * (k_inf * x_inf + b_inf)
    print(f"N {q.direct.N} w {info.width} p {info.border} interchanges {info.interchanges} pivots [{info.min_pivot:.3e}, {info.max_pivot:.3e}]: "
          f"residual banded {res:.3e}, splu {res_direct:.3e}, floor {floor:.3e}")
    assert res <= 16.0 * res_direct + floor


def test_the_other_products_of_the_handle_keep_their_bits(case):
    ev, q = case.system.evaluator, case.band
    p = ev.plan
    rng = np.random.default_rng(31)
    lin = case.linearize()
    rhs = rng.uniform(-1.0, 1.0, case.n + case.m)
    ev.set_bounds()
    g, s, lam, sig, rbar = (rng.uniform(0.5, 1.5, case.m) for _ in range(5))

    def products():
        sol, _ = lin.solve_kkt(rhs, s1=q.s1, s2=q.s2, precond=None, tol=0.0, maxiter=6, check_every=6)
        terms = ev.slack_terms(g, s, lam, sig, rbar)
        return sol, lin.jv(case.v), terms.s2, terms.b2, terms.table

    before = products()
    lin.solve_banded(q.b, s1=q.s1, s2=q.s2)
    after = products()
    for a, b in zip(before, after):
        assert sc.same_bits(a, b)
    del p


def test_refusals_of_the_public_forms(case):
    import models
    import pockit_amd.radau as radau
    from pockit_amd import runtime

    ev, q = case.system.evaluator, case.band
    lib, h = ev.ctx.lib, ev.ctx.handle
    as_dp = runtime.as_dp
    N = case.n + case.m
    lin = case.linearize()
    lin.solve_banded(q.b, s1=q.s1, s2=q.s2)           # (planned and factored)
    d = [_up(a) for a in (q.hvals, q.jvals, q.s1, q.s2)]
    rhs, sol = _up(q.b), Buf(N)
    hx, hrec = np.full(N, -3.0), np.full(8, -3.0)
    _sync()
    ptrs = [_ptr(t) for t in d]
    for k in range(4):
        bad = list(ptrs)
        bad[k] = None
        assert lib.pk_band_factor_dev(h, *bad) == 110
    assert lib.pk_band_solve_dev(h, None, sol.ptr) == 110 and lib.pk_band_solve_dev(h, _ptr(rhs), None) == 110
    assert lib.pk_band_record(h, None) == 60
    assert lib.pk_solve_banded(h, None, as_dp(q.s2), as_dp(q.b), as_dp(hx), as_dp(hrec)) == 60
    assert lib.pk_solve_banded(h, as_dp(q.s1), as_dp(q.s2), as_dp(q.b), None, as_dp(hrec)) == 60
    o = q.ordering
    order, amap = np.ascontiguousarray(o.order), np.ascontiguousarray(o.map)
    i32 = lambda a: a.ctypes.data_as(runtime.c_int32_p)  # noqa: E731
    assert lib.pk_band_plan(h, -1, o.w, o.p, i32(order), i32(amap)) == 134
    assert lib.pk_band_plan(h, o.nb, bc.W_CAP + 1, o.p, i32(order), i32(amap)) == 134
    assert lib.pk_band_plan(h, o.nb, o.w, bc.P_CAP + 1, i32(order), i32(amap)) == 134
    assert lib.pk_band_plan(h, o.nb, o.w, o.p, None, i32(amap)) == 60
    ev.sync()
    assert np.all(np.isnan(sol.fetch())) and np.all(hx == -3.0) and np.all(hrec == -3.0)
    fresh = models.brachistochrone(radau, 3, 4)[0].evaluator
    try:
        v = np.zeros(fresh.plan.n + fresh.plan.m)
        out = np.full(len(v), -3.0)
        fh = fresh.ctx.handle
        assert fresh.ctx.lib.pk_band_record(fh, as_dp(hrec)) == 134                                   # nothing planned
        assert fresh.ctx.lib.pk_solve_banded(fh, as_dp(v), as_dp(v), as_dp(v), as_dp(out), as_dp(hrec)) == 117
        assert np.all(out == -3.0) and np.all(hrec == -3.0)
    finally:
        fresh.close()
