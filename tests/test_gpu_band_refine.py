"""The refinement of the band solve (pockit_amd/csrc/pk_band_refine.cpp: pk_bd_resid_k, pk_bd_refine_scalar_k, pk_bd_correct_k) on the
device, against the emulator of tests/band_refine_cases.py.

1. The three kernels through ``pk_band_refine_step_dev`` on the context of brachistochrone(radau, 3, 4) at the lengths 1, 2, 255,
   256, 257, 2047, 2048, 2049 and 524 289 (one element beyond 2048 work items of the correction: its stride loop takes a second
   trip): r, x and the record bit-equal to the emulator, the same bits from a second call; a NaN and an infinity planted in x, b
   and q (status 3, counted, left out of the maxima); NaN at every element that is no unknown of a classification.
2. The five synthetic systems of ``band_refine_cases.TABLE``, each step composed of ``pk_band_raw_dev``, the host's dense product
   uploaded as q, the step form, and ``pk_band_raw_dev`` on r: x, r and the record bit-equal to the emulator after every step;
   the statuses and bounds of tests/test_band_refine_cases_cpu.py.
3. The six models of tests/test_gpu_csr_operators.py with the plan's row classification: ``solve_banded(refine=2)`` bit-equal to
   the emulator in x and both records; ``refine=0``, ``solve_kkt`` and ``jv`` return the bits of a call made before any refinement.
   Slot 5 of the record against rho recomputed in ``np.longdouble`` from the downloaded values, twice:
   * at a perturbed x (the solution plus noise of its own size, so that r is no rounding error), through ``band_refine_begin_dev``:
     within ``4 N 2^-53`` RELATIVE to rho, and the record bit-equal to the emulator;
   * at the refined x, where r = b - K x is itself the rounding error of sums of size |K||x| + |b| and no bound relative to rho can
     hold for any correct code (measured on the six models: the two rho differ by 0.03 % to 11 % of rho, at rho from 1.7e-16 to
     7.5e-15): within ``4 N 2^-53 (|K||x| + |b|)inf / (min(|x|inf, 1e6 |b|inf) + |b|inf)``, the same factor relative to the summands.
4. The refusals with their codes; an advance behind a new factorisation gives 135."""
import numpy as np
import pytest

import band_refine_cases as br
import sparse_cases as sc
from device_cases import Buf, _ptr, _same, _sync, _up, step_ev  # noqa: F401  (step_ev: a fixture)
from test_gpu_band import BandInputs, _raw
from test_gpu_csr_operators import CASES, Case

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]
LD = np.longdouble
TABLE_TOL = 1.0e-14      # (tests/test_band_refine_cases_cpu.py: the bound the repaired rows are held to)


def _i32(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(torch.device("cuda", 0))


def _step(ev, which, length, where, b, q, x, d, r, rec, band_rec, tol, min_steps, t):
    ev.ctx.check(ev.ctx.lib.pk_band_refine_step_dev(ev.ctx.handle, which, length, _ptr(where), _ptr(b), _ptr(q), _ptr(x), _ptr(d), _ptr(r),
                                                    _ptr(rec), _ptr(band_rec), float(tol), int(min_steps), int(t)))


def _same_or_nan(what, got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN in other places"
    _same(what, np.nan_to_num(got, nan=7.0), np.nan_to_num(want, nan=7.0))


# ---------------------------------------------------------------- 1: the kernels
def _kernels(ev, length, fixed, planted, t, tol, min_steps, rec_in):
    where, b, q, x, d = br.step_vectors(length, planted=planted, fixed=fixed)
    w_r, sums = br.resid(b, q, x, where)
    w_rec = br.scalar(sums, rec_in, t, tol, min_steps)
    w_x = br.correct(x, d, w_rec, where)
    dw = None if where is None else _i32(where)
    db, dq, dd = _up(b), _up(q), _up(d)
    outs = []
    for _ in range(2):
        dx, dr, drec = Buf(length, x), Buf(length), Buf(8, rec_in)
        _sync()
        _step(ev, br.RESID, length, dw, db, dq, dx, None, dr, None, None, 0.0, 0, 0)
        _step(ev, br.SCALAR, length, None, None, None, None, None, None, drec, None, tol, min_steps, t)
        _step(ev, br.CORRECT, length, dw, None, None, dx, dd, None, drec, None, 0.0, 0, t)
        ev.sync()
        outs.append((dr.fetch(), drec.fetch(), dx.fetch()))
    what = f"length {length} fixed {fixed} planted {planted} step {t}"
    (r, rec, got_x), again = outs
    for a, c in zip(outs[0], again):
        assert sc.same_bits(a, c), f"{what}: a second call gave other bits"
    _same(f"{what} record", rec, w_rec)
    _same_or_nan(f"{what} r", r, w_r)
    _same_or_nan(f"{what} x", got_x, w_x)
    if where is not None:
        out = where < 0
        assert np.all(r[out] == 0.0) and not np.any(np.signbit(r[out])) and np.all(np.isnan(got_x[out]))
    return rec


@pytest.mark.parametrize("length", br.LENGTHS + (br.BEYOND_GRID,))
def test_the_kernels_match_the_emulator_bit_for_bit(step_ev, length):
    running = np.array([br.RUNNING, 1.0, 0.5, 1.0, 1.0, 0.25, 0.75, 0.75])
    tiny = np.array([br.RUNNING, 1.0, 1e-9, 1.0, 1.0, 1e-12, 0.75, 0.75])
    stopped = running.copy()
    stopped[br.STATUS] = br.STALLED
    for fixed in (False, True):
        assert _kernels(step_ev, length, fixed, False, 0, 1e-10, 0, None)[br.STATUS] == br.RUNNING
        assert _kernels(step_ev, length, fixed, True, 0, 1e-10, 0, None)[br.STATUS] == br.NON_FINITE
        if length == br.BEYOND_GRID:
            continue
        assert _kernels(step_ev, length, fixed, False, 0, 1.0, 0, None)[br.STATUS] == br.CONVERGED
        assert _kernels(step_ev, length, fixed, False, 0, 1.0, 1, None)[br.STATUS] == br.RUNNING
        assert _kernels(step_ev, length, fixed, False, 1, 1e-10, 0, running)[br.STATUS] == br.RUNNING
        assert _kernels(step_ev, length, fixed, False, 2, 1e-10, 0, tiny)[br.STATUS] == br.STALLED
        assert _kernels(step_ev, length, fixed, False, 2, 1e-3, 0, tiny)[br.STATUS] == br.CONVERGED
        assert _kernels(step_ev, length, fixed, False, 3, 1.0, 0, stopped)[br.STATUS] == br.STALLED


# ---------------------------------------------------------------- 2: the synthetic systems, step by step
@pytest.mark.parametrize("k", range(5))
def test_the_synthetic_systems_step_by_step(step_ev, k):
    ev, row = step_ev, br.TABLE[k]
    s = br.table_system(row)
    steps = br.MAX_STEPS if k == 4 else 3
    want = s.refine(steps, tol=TABLE_TOL)
    _, _, x, band_rec = _raw(ev, s.AB, s.U, s.C, s.rhs)
    _same("the band record", band_rec, s.first()[1])
    db, dband_rec, drec = _up(s.rhs), _up(band_rec), Buf(8)
    dx = Buf(s.N, x)
    r = None
    for t in range(steps + 1):
        if t >= 1:
            _, _, d, _ = _raw(ev, s.AB, s.U, s.C, r)
            dd = _up(d)
            _sync()
            _step(ev, br.CORRECT, s.N, None, None, None, dx, dd, None, drec, None, 0.0, 0, t)
            ev.sync()
        dq, dr = _up(s.kx(dx.fetch())), Buf(s.N)
        _sync()
        _step(ev, br.RESID, s.N, None, db, dq, dx, None, dr, None, None, 0.0, 0, t)
        _step(ev, br.SCALAR, s.N, None, None, None, None, None, None, drec, dband_rec, TABLE_TOL, 0, t)
        ev.sync()
        r, rec = dr.fetch(), drec.fetch()
        w_x, w_r, w_rec = want[t]
        _same(f"row {k + 1} step {t} record", rec, w_rec)
        _same(f"row {k + 1} step {t} x", dx.fetch(), w_x)
        _same(f"row {k + 1} step {t} r", r, w_r)
    print(f"row {k + 1}: status {rec[br.STATUS]}, {rec[br.STEPS]} corrections, rho_0 {rec[br.RHO0]:.3e}, rho {rec[br.RHO]:.3e}")
    assert rec[br.STATUS] == row[2]
    if k == 0:
        assert rec[br.STEPS] == 0.0 and sc.same_bits(dx.fetch(), x)
    elif k < 4:
        assert rec[br.STEPS] == 1.0 and rec[br.RHO] <= 1.0e-14 and rec[br.RHO0] >= 1.0e-12
    else:
        assert rec[br.RHO] > br.SINGULAR


# ---------------------------------------------------------------- 3: models
@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def case(request):
    c = Case(*request.param)
    c.band = BandInputs(c)
    yield c
    c.system.evaluator.close()


def _model(q):
    """The emulator's view of a case, made once (its first solve is the slow part at 192 008 unknowns)."""
    if getattr(q, "refine_model", None) is None:
        q.refine_model = br.Model(q.ordering, q.map_j, q.map_h, q.hvals, q.jvals, q.s1, q.s2)
    return q.refine_model


def _rho_extended(q, x, b):
    """rho over the free variables and all rows in extended precision from the downloaded values."""
    d = q.direct
    data = (d.select @ np.concatenate((q.hvals, q.jvals, q.s1, q.s2))).astype(LD)
    cols = np.repeat(np.arange(d.N), np.diff(d.indptr))
    rows = d.indices.astype(np.int64)
    n = d.n
    y = np.concatenate((x[:n][q.free], x[n:])).astype(LD)
    rhs = np.concatenate((b[:n][q.free], b[n:])).astype(LD)
    r = rhs.copy()
    np.subtract.at(r, rows, data * y[cols])
    size = np.zeros(d.N, dtype=LD)
    np.add.at(size, rows, np.abs(data * y[cols]))
    rn, xn, bn = np.abs(r).max(), np.abs(y).max(), np.abs(rhs).max()
    return float(rn), float(rn / (min(xn, LD(1.0e6) * bn) + bn)), float((size + np.abs(rhs)).max())


def test_solve_banded_refined_matches_the_emulator(case):
    q = case.band
    lin = case.linearize()
    plain, _ = lin.solve_banded(q.b, s1=q.s1, s2=q.s2)
    sol_kkt = lin.solve_kkt(q.b, s1=q.s1, s2=q.s2, precond=None, tol=0.0, maxiter=6, check_every=6)[0]
    jv = lin.jv(case.v)
    x, info = lin.solve_banded(q.b, s1=q.s1, s2=q.s2, refine=2)
    again, info2 = lin.solve_banded(q.b, s1=q.s1, s2=q.s2, refine=2)
    model = _model(q)
    w_x, _, w_rec, w_band = model.refine_host(q.b, 2)
    _same("the band record", info.record, w_band)
    _same("the refinement's record", info.refinement_record, w_rec)
    _same("the refined x", x, w_x)
    assert sc.same_bits(x, again) and sc.same_bits(info.refinement_record, info2.refinement_record), "a second call gave other bits"
    assert info.status == "solved" and info.refinement in ("converged", "stalled", "exhausted")
    assert info.refinement_steps == int(w_rec[br.STEPS]) <= 2 and info.residual_ratio == w_rec[br.RHO] and info.residual_ratio_start == w_rec[br.RHO0]
    assert not x[: case.n][~q.free].any()
    # slot 5 against extended precision: r = b - K x carries the rounding of N-term sums of size |K||x| + |b|
    N = case.n + case.m
    rn, rho, size = _rho_extended(q, x, q.b)
    rec = info.refinement_record
    den = min(rec[br.XNORM], 1.0e6 * rec[br.BNORM]) + rec[br.BNORM]
    print(f"N {N}: rho_0 {rec[br.RHO0]:.3e}, rho {rec[br.RHO]:.3e} after {info.refinement_steps} corrections ({info.refinement}); extended rho {rho:.3e}")
    assert abs(rec[br.RHO] - rho) <= 4.0 * N * 2.0 ** -53 * size / den
    # ... and relative to rho itself where r is no rounding error: the solution plus noise of its own size, measured by begin
    ev = case.system.evaluator
    rng = np.random.default_rng(41)
    xp = x + rng.uniform(-1.0, 1.0, N) * np.abs(x).max()
    xp[: case.n][~q.free] = 0.0
    d = [_up(a) for a in (q.hvals, q.jvals, q.s1, q.s2, q.b)]
    live = Buf(N, xp)
    _sync()
    ev.band_factor_dev(*[_ptr(t) for t in d[:4]])
    ev.band_refine_begin_dev(*[_ptr(t) for t in d], live.ptr, 0.0, 0)
    rec_p = ev.band_refine_record()
    _, rho_p, _ = _rho_extended(q, xp, q.b)
    _, sums = br.resid(q.b, model.kx(xp), xp, model.where)
    _same("the record at the perturbed x", rec_p, br.scalar(sums, None, 0, 0.0, 0))
    assert sc.same_bits(live.fetch(), xp), "begin moved x"
    rel = abs(rec_p[br.RHO] - rho_p) / rho_p
    print(f"    perturbed x: rho {rec_p[br.RHO]:.6e}, extended {rho_p:.6e}, relative difference {rel:.2e} (bound {4.0 * N * 2.0 ** -53:.2e})")
    assert rec_p[br.STATUS] == br.RUNNING and rho_p > 1.0e-3 and rel <= 4.0 * N * 2.0 ** -53
    # the unrefined call, solve_kkt and jv keep the bits they had before any refinement
    after, info0 = lin.solve_banded(q.b, s1=q.s1, s2=q.s2)
    assert sc.same_bits(plain, after) and info0.refinement is None and info0.residual_ratio is None
    assert sc.same_bits(sol_kkt, lin.solve_kkt(q.b, s1=q.s1, s2=q.s2, precond=None, tol=0.0, maxiter=6, check_every=6)[0])
    assert sc.same_bits(jv, lin.jv(case.v))


# ---------------------------------------------------------------- 4: refusals
def test_refusals_of_the_refinement(case):
    from pockit_amd import runtime

    ev, q = case.system.evaluator, case.band
    lib, h = ev.ctx.lib, ev.ctx.handle
    as_dp = runtime.as_dp
    N = case.n + case.m
    lin = case.linearize()
    lin.solve_banded(q.b, s1=q.s1, s2=q.s2)           # (planned and factored; the operators are set)
    d = [_up(a) for a in (q.hvals, q.jvals, q.s1, q.s2, q.b)]
    sol = Buf(N)
    hx, hrec, hrrec = np.full(N, -3.0), np.full(8, -3.0), np.full(8, -3.0)
    _sync()
    ptrs = [_ptr(t) for t in d] + [sol.ptr]
    for k in range(6):
        bad = list(ptrs)
        bad[k] = None
        assert lib.pk_band_refine_begin_dev(h, *bad, 1e-10, 0) == 110
    assert lib.pk_band_refine_begin_dev(h, *ptrs, -1.0, 0) == 134
    assert lib.pk_band_refine_begin_dev(h, *ptrs, float("nan"), 0) == 134
    assert lib.pk_band_refine_begin_dev(h, *ptrs, 1e-10, -1) == 134
    assert lib.pk_band_refine_begin_dev(h, *ptrs, 1e-10, 11) == 134
    assert lib.pk_band_refine_record(h, None) == 60
    host = (as_dp(q.s1), as_dp(q.s2), as_dp(q.b), as_dp(hx), as_dp(hrec), as_dp(hrrec))
    assert lib.pk_solve_banded_refined(h, *host, 1e-10, 0, 11) == 134
    assert lib.pk_solve_banded_refined(h, *host, 1e-10, 11, 2) == 134
    assert lib.pk_solve_banded_refined(h, *host, -1.0, 0, 2) == 134
    assert lib.pk_solve_banded_refined(h, *host[:5], None, 1e-10, 0, 2) == 60
    for bad in (-1, 11, 1.5, True):
        with pytest.raises(ValueError, match="refine"):
            lin.solve_banded(q.b, s1=q.s1, s2=q.s2, refine=bad)
    ev.sync()
    assert np.all(np.isnan(sol.fetch())) and np.all(hx == -3.0) and np.all(hrec == -3.0) and np.all(hrrec == -3.0)
    # the life of a refinement: begin, advance, record; a new factorisation ends it
    ev.band_factor_dev(*[_ptr(t) for t in d[:4]])
    assert lib.pk_band_refine_advance_dev(h, 1) == 135 and lib.pk_band_refine_record(h, as_dp(hrec)) == 135
    live = Buf(N, np.zeros(N))
    ev.band_solve_dev(_ptr(d[4]), live.ptr)
    ev.band_refine_begin_dev(*[_ptr(t) for t in d], live.ptr)
    assert lib.pk_band_refine_advance_dev(h, 0) == 134
    ev.band_refine_advance_dev(3)
    rec = ev.band_refine_record()
    frozen = live.fetch()
    ev.band_refine_advance_dev(2)
    assert sc.same_bits(ev.band_refine_record(), rec) and sc.same_bits(live.fetch(), frozen) and rec[br.STATUS] != br.RUNNING
    model = _model(q)
    x0 = model.first(q.b)[0]
    w_x, _, w_rec = br.refine(model.solve, model.kx, q.b, x0, model.where, steps=3)[-1]
    _same("the record behind three enqueued steps", rec, w_rec)
    _same("x behind three enqueued steps", frozen, w_x)
    ev.band_factor_dev(*[_ptr(t) for t in d[:4]])
    assert lib.pk_band_refine_advance_dev(h, 1) == 135
    assert np.all(hrec == -3.0)
