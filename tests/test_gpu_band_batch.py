"""The batch forms of the bordered band LU (pockit_amd/csrc/pk_band.cpp: B step systems behind one plan, one launch sequence with
the grid (., B)) on the device.

Synthetic batches through ``pk_band_raw_batch_dev`` on the context of brachistochrone(radau, 3, 4): the shapes and B of the CPU
driver (band_batch_cases.SHAPES, B = 1, 2, 3, 16) and one longer batch (B = 3, Nb = 4 129, w = 8, p = 1: three pieces per dot,
130 panels).  Full-mantissa data; NaN in the fill rows, outside the matrix and in the gaps between the entries (every array is
packed at a stride larger than its length); every entry's band, interchanges, solution and record bit-equal to the emulator of
tests/band_cases.py for that entry ALONE, the same bits from a second call, the gaps still NaN; failing entries among good ones;
a permuted batch; growing, shrinking and a single factorisation in between; the refusals.

Three of the models of tests/test_gpu_csr_operators.py (a border of 0, 2 and a wide band): the batch device forms at B = 3 with
per-entry values (all four strides non-zero) and with shared H, J and s2 (stride 0) bit-equal, entry by entry, to three calls of
the single device forms on the same pointers; ``solve_banded_batch`` bit-equal to ``solve_banded`` per row; ``solve_banded``,
``solve_kkt`` and ``jv`` return the bits they returned before the batch calls."""
import numpy as np
import pytest

import band_batch_cases as bb
import band_cases as bc
import sparse_cases as sc
from device_cases import Buf, _ptr, _same, _sync, _up, step_ev  # noqa: F401  (step_ev: a fixture)
from test_gpu_band import BandInputs
from test_gpu_csr_operators import Case

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]
GAP = bb.GAP


def _raw_batch(ev, batch):
    """One call of the raw batch form on the packed arrays: per entry (band, ipiv, x, rec), and the gaps of the outputs."""
    s = batch.strides
    B = batch.B
    band = Buf(B * s["band"], batch.band)
    dU, dC, drhs = _up(batch.U), _up(batch.C), _up(batch.rhs)
    piv = Buf((B * s["ipiv"] + 1) // 2 + 1)
    x, rec = Buf(B * s["x"]), Buf(B * s["rec"])
    _sync()
    ev.ctx.check(ev.ctx.lib.pk_band_raw_batch_dev(ev.ctx.handle, B, batch.nb, batch.w, batch.p, batch.p + 1, band.ptr, s["band"], _ptr(dU), s["U"],
                                                  _ptr(dC), s["C"], _ptr(drhs), s["rhs"], piv.ptr, s["ipiv"], x.ptr, s["x"], rec.ptr, s["rec"]))
    ev.sync()
    got = dict(band=band.fetch(), ipiv=piv.fetch().view(np.int32)[: B * s["ipiv"]], x=x.fetch(), rec=rec.fetch())
    for name in ("band", "x", "rec"):
        assert np.all(np.isnan(batch.gaps(name, got[name]))), f"the gaps of {name} were written"
    untouched = np.full(piv.count, np.nan).view(np.int32)[: B * s["ipiv"]]      # (the interchanges lie in a NaN-filled array of doubles)
    assert np.array_equal(batch.gaps("ipiv", got["ipiv"]), batch.gaps("ipiv", untouched)), "the gaps of the interchanges were written"
    return [(batch.entry("band", got["band"], e), batch.entry("ipiv", got["ipiv"], e).astype(np.int64), batch.entry("x", got["x"], e),
             batch.entry("rec", got["rec"], e)) for e in range(B)]


def _check_batch(ev, batch):
    first, second = _raw_batch(ev, batch), _raw_batch(ev, batch)
    for e in range(batch.B):
        band, ipiv, x, rec = first[e]
        for name, a, b in zip(("band", "ipiv", "x", "record"), first[e], second[e]):
            assert sc.same_bits(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)), f"entry {e} {name}: a second call gave other bits"
        _same(f"entry {e} record", rec, batch.expected[e][3])
        bb.check_entry(batch, e, band, ipiv, x, rec, untouched=np.nan)
        if batch.expected[e][2] is not None:
            assert np.all(np.isnan(band[~batch.inside])), f"entry {e}: a slot outside the matrix was written"
    return first


@pytest.mark.parametrize("B", bb.BATCHES)
@pytest.mark.parametrize("nb,w,p", bb.SHAPES, ids=lambda v: str(v))
def test_every_entry_matches_the_emulator_bit_for_bit(step_ev, nb, w, p, B):
    batch = bb.Batch(nb, w, p, bb.picks(B))
    _check_batch(step_ev, batch)
    assert all(batch.expected[e][3][bc.STATUS] == 0.0 for e in range(0, B, 2))      # (the plain entries solve)


def test_the_longer_batch(step_ev):
    B, nb, w, p = bb.LONG
    batch = bb.Batch(nb, w, p, [("plain", 11 + e) for e in range(B)])
    got = _check_batch(step_ev, batch)
    assert all(rec[bc.STATUS] == 0.0 and rec[bc.R_NB] == nb for _, _, _, rec in got)
    assert not sc.same_bits(got[0][2], got[1][2])


def test_failed_entries_do_not_stop_the_others_and_a_permuted_batch_is_permuted(step_ev):
    nb, w, p = 3 * bc.NB + 5, 7, 1
    chosen = [(variant, 4) for variant, _ in bb.MIXED]
    got = _check_batch(step_ev, bb.Batch(nb, w, p, chosen))
    for (variant, status), (_, _, x, rec) in zip(bb.MIXED, got):
        assert rec[bc.STATUS] == status
        if status:
            assert rec[bc.COLUMN] == bc.failing_column(nb, variant) and np.all(np.isnan(x))
        else:
            assert np.all(np.isfinite(x))
    perm = [2, 0, 3, 1]
    moved = _raw_batch(step_ev, bb.Batch(nb, w, p, [chosen[e] for e in perm]))
    for e, source in enumerate(perm):
        for name, a, b in zip(("band", "ipiv", "x", "record"), moved[e], got[source]):
            assert sc.same_bits(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)), f"entry {e} {name}"


def test_growing_shrinking_and_a_single_system_in_between(step_ev):
    from test_gpu_band import _raw

    ev = step_ev
    nb, w, p = 2 * bc.NB + 1, 7, 8
    AB, U, C, rhs = bc.system(nb, w, p, seed=21)
    single = _raw(ev, AB, U, C, rhs)
    _check_batch(ev, bb.Batch(nb, w, p, bb.picks(2, first_seed=30)))
    _check_batch(ev, bb.Batch(nb, w, p, bb.picks(5, first_seed=40)))
    again = _raw(ev, AB, U, C, rhs)
    for a, b in zip(single, again):
        assert sc.same_bits(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    _check_batch(ev, bb.Batch(nb, w, p, bb.picks(2, first_seed=30)))


def test_refusals_of_the_raw_batch_form(step_ev):
    ev = step_ev
    lib, h = ev.ctx.lib, ev.ctx.handle
    batch = bb.Batch(40, 7, 1, bb.picks(2), nan_outside=False)
    s = batch.strides
    band, dU, dC, drhs = Buf(2 * s["band"], batch.band), _up(batch.U), _up(batch.C), _up(batch.rhs)
    piv, x, rec = Buf(s["ipiv"] + 1), Buf(2 * s["x"]), Buf(2 * s["rec"])
    _sync()
    good = [band.ptr, s["band"], _ptr(dU), s["U"], _ptr(dC), s["C"], _ptr(drhs), s["rhs"], piv.ptr, s["ipiv"], x.ptr, s["x"], rec.ptr, s["rec"]]
    call = lambda B, nb, w, p, R, args: lib.pk_band_raw_batch_dev(h, B, nb, w, p, R, *args)  # noqa: E731
    assert call(0, 40, 7, 1, 2, good) == 134 and call(bb.BATCH_CAP + 1, 40, 7, 1, 2, good) == 134
    assert call(2, -1, 7, 1, 2, good) == 134 and call(2, 40, bc.W_CAP + 1, 1, 2, good) == 134
    assert call(2, 40, 7, bc.P_CAP + 1, bc.P_CAP + 2, good) == 134 and call(2, 40, 7, 1, 1, good) == 134
    L = batch.lengths
    for k, stride in ((1, L["band"] - 1), (1, 0), (3, L["U"] - 1), (5, -1), (7, L["rhs"] - 1), (9, L["ipiv"] - 1), (11, 0), (11, L["x"] - 1), (13, 7)):
        bad = list(good)
        bad[k] = stride
        assert call(2, 40, 7, 1, 2, bad) == 134, (k, stride)
    for k in range(0, 14, 2):
        bad = list(good)
        bad[k] = None
        assert call(2, 40, 7, 1, 2, bad) == 110, k
    ev.sync()
    for b in (piv, x, rec):
        assert np.all(np.isnan(b.fetch()))
    assert sc.same_bits(band.fetch(), batch.band)


# ---------------------------------------------------------------- models
MODELS = [("brachistochrone", "radau", 3, 4), ("two_stage_rocket", "radau", 6, 4), ("planar_quadrotor", "lobatto", 20, 6)]
B_MODEL = 3


@pytest.fixture(scope="module", params=MODELS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def case(request):
    c = Case(*request.param)
    c.band = BandInputs(c)
    yield c
    c.system.evaluator.close()


def _entries(q, n, m, shared):
    """Per entry (hvals, jvals, s1, s2, b): the model's values, perturbed per entry unless H, J and s2 are ``shared``."""
    rng = np.random.default_rng(47)
    out = []
    for e in range(B_MODEL):
        scale_h, scale_j = (1.0, 1.0) if shared or e == 0 else (1.0 + rng.uniform(-1e-3, 1e-3, len(q.hvals)), 1.0 + rng.uniform(-1e-3, 1e-3, len(q.jvals)))
        s2 = q.s2 if shared else q.s2 * rng.uniform(0.5, 1.5, m)
        out.append((q.hvals * scale_h, q.jvals * scale_j, q.s1 * rng.uniform(0.5, 1.5, n), s2, rng.uniform(-1.0, 1.0, n + m)))
    return out


def _packed(arrays):
    """Arrays of one length at stride length + GAP with NaN in the gaps: (device tensor, stride)."""
    length = len(arrays[0])
    host = np.full(len(arrays) * (length + GAP), np.nan)
    for e, a in enumerate(arrays):
        host[e * (length + GAP): e * (length + GAP) + length] = a
    return _up(host), length + GAP


@pytest.mark.parametrize("shared", [False, True], ids=["own_values", "shared_h_j_s2"])
def test_the_batch_device_forms_equal_three_single_calls(case, shared):
    ev, q = case.system.evaluator, case.band
    n, m = case.n, case.m
    N = n + m
    ev.band_plan(q.ordering)
    entries = _entries(q, n, m, shared)
    (dh, sh), (dj, sj), (d1, ss1), (d2, ss2), (db, sb) = (_packed([entry[k] for entry in entries]) for k in range(5))
    if shared:
        sh = sj = ss2 = 0
    sol = Buf(B_MODEL * (N + GAP))
    _sync()
    ev.band_factor_batch_dev(B_MODEL, _ptr(dh), _ptr(dj), _ptr(d1), _ptr(d2), strides=(sh, sj, ss1, ss2))
    ev.band_solve_batch_dev(B_MODEL, _ptr(db), sol.ptr, stride_rhs=sb, stride_sol=N + GAP)
    records = ev.band_record_batch(B_MODEL)
    got = sol.fetch().reshape(B_MODEL, N + GAP)
    assert np.all(np.isnan(got[:, N:])), "the gaps between the solutions were written"
    for e in range(B_MODEL):
        one = Buf(N)
        ev.band_factor_dev(_ptr(dh) + 8 * sh * e, _ptr(dj) + 8 * sj * e, _ptr(d1) + 8 * ss1 * e, _ptr(d2) + 8 * ss2 * e)
        ev.band_solve_dev(_ptr(db) + 8 * sb * e, one.ptr)
        rec = ev.band_record()
        assert rec[bc.STATUS] == 0.0
        _same(f"entry {e}: the record", records[e], rec)
        _same(f"entry {e}: the solution", got[e, :N], one.fetch())
    assert not sc.same_bits(got[0, :N], got[1, :N])
    # ... the batch survived the single calls: a second batch solve gives the same bits
    again = Buf(B_MODEL * (N + GAP))
    ev.band_solve_batch_dev(B_MODEL, _ptr(db), again.ptr, stride_rhs=sb, stride_sol=N + GAP)
    ev.sync()
    assert sc.same_bits(again.fetch().reshape(B_MODEL, N + GAP)[:, :N], got[:, :N])


def test_solve_banded_batch_equals_solve_banded_per_row_and_the_other_products_keep_their_bits(case):
    q = case.band
    lin = case.linearize()
    n, m = case.n, case.m
    rng = np.random.default_rng(53)
    rhs = rng.uniform(-1.0, 1.0, n + m)

    def products():
        x, _ = lin.solve_banded(q.b, s1=q.s1, s2=q.s2)
        sol, _ = lin.solve_kkt(rhs, s1=q.s1, s2=q.s2, precond=None, tol=0.0, maxiter=6, check_every=6)
        return x, sol, lin.jv(case.v)

    before = products()
    s1 = q.s1[None, :] * rng.uniform(0.5, 1.5, (B_MODEL, n))
    s2 = q.s2[None, :] * rng.uniform(0.5, 1.5, (B_MODEL, m))
    b = rng.uniform(-1.0, 1.0, (B_MODEL, n + m))
    s1[1, np.flatnonzero(q.free)[0]] = np.nan      # entry 1 fails (a column that is not finite): its row is NaN, the others are whole
    X, infos = lin.solve_banded_batch(b, s1=s1, s2=s2)
    assert X.shape == (B_MODEL, n + m) and len(infos) == B_MODEL
    for e in range(B_MODEL):
        x, info = lin.solve_banded(b[e], s1=s1[e], s2=s2[e])
        assert infos[e].status == info.status == ("non_finite" if e == 1 else "solved")
        _same(f"row {e}: the record", infos[e].record, info.record)
        assert np.all(np.isnan(X[e])) if e == 1 else sc.same_bits(X[e], x), e
    Y, shared_infos = lin.solve_banded_batch(b, s1=q.s1, s2=None)      # (n,) and None broadcast over the rows
    for e in range(B_MODEL):
        x, _ = lin.solve_banded(b[e], s1=q.s1, s2=None)
        assert sc.same_bits(Y[e], x) or (np.all(np.isnan(Y[e])) and np.all(np.isnan(x)))
    for a, c in zip(before, products()):
        assert sc.same_bits(a, c)
    with pytest.raises(ValueError):
        lin.solve_banded_batch(b[0])
    with pytest.raises(ValueError):
        lin.solve_banded_batch(np.zeros((17, n + m)))
    with pytest.raises(ValueError):
        lin.solve_banded_batch(b, s1=np.zeros((2, n)))


def test_refusals_of_the_public_batch_forms(case):
    from pockit_amd import runtime

    ev, q = case.system.evaluator, case.band
    lib, h = ev.ctx.lib, ev.ctx.handle
    as_dp = runtime.as_dp
    n, m = case.n, case.m
    N = n + m
    case.linearize().solve_banded(q.b, s1=q.s1, s2=q.s2)      # (operators, a linearization, a plan)
    ev.band_plan(q.ordering)                                   # (a new plan: no batch factorisation)
    d = [_up(a) for a in (q.hvals, q.jvals, q.s1, q.s2)]
    rhs, sol = _up(q.b), Buf(2 * N)
    hx, hrec = np.full(2 * N, -3.0), np.full(16, -3.0)
    _sync()
    ptrs = [_ptr(t) for t in d]
    factor = lambda B, p, strides: lib.pk_band_factor_batch_dev(h, B, p[0], strides[0], p[1], strides[1], p[2], strides[2], p[3], strides[3])  # noqa: E731
    assert lib.pk_band_solve_batch_dev(h, 2, _ptr(rhs), 0, sol.ptr, N) == 134            # planned, no batch factorisation
    assert lib.pk_band_record_batch(h, 2, as_dp(hrec)) == 134
    assert factor(0, ptrs, (0, 0, 0, 0)) == 134 and factor(bb.BATCH_CAP + 1, ptrs, (0, 0, 0, 0)) == 134
    for k, length in enumerate((len(q.hvals), len(q.jvals), n, m)):
        strides = [0, 0, 0, 0]
        strides[k] = length - 1 if length > 1 else -1
        assert factor(2, ptrs, strides) == 134, k
        bad = list(ptrs)
        bad[k] = None
        assert factor(2, bad, (0, 0, 0, 0)) == 110, k
    ev.band_factor_batch_dev(2, *ptrs, strides=(0, 0, 0, 0))
    assert lib.pk_band_solve_batch_dev(h, 3, _ptr(rhs), 0, sol.ptr, N) == 134            # the last batch had 2 entries
    assert lib.pk_band_solve_batch_dev(h, 2, _ptr(rhs), N - 1, sol.ptr, N) == 134
    assert lib.pk_band_solve_batch_dev(h, 2, _ptr(rhs), 0, sol.ptr, N - 1) == 134
    assert lib.pk_band_solve_batch_dev(h, 2, _ptr(rhs), 0, sol.ptr, 0) == 134
    assert lib.pk_band_solve_batch_dev(h, 2, None, 0, sol.ptr, N) == 110 and lib.pk_band_solve_batch_dev(h, 2, _ptr(rhs), 0, None, N) == 110
    assert lib.pk_band_record_batch(h, 2, None) == 60 and lib.pk_band_record_batch(h, 3, as_dp(hrec)) == 134
    two = lambda a: np.ascontiguousarray(np.tile(a, 2))  # noqa: E731
    assert lib.pk_solve_banded_batch(h, 2, None, as_dp(two(q.s2)), as_dp(two(q.b)), as_dp(hx), as_dp(hrec)) == 60
    assert lib.pk_solve_banded_batch(h, 2, as_dp(two(q.s1)), as_dp(two(q.s2)), as_dp(two(q.b)), None, as_dp(hrec)) == 60
    assert lib.pk_solve_banded_batch(h, 0, as_dp(two(q.s1)), as_dp(two(q.s2)), as_dp(two(q.b)), as_dp(hx), as_dp(hrec)) == 134
    ev.sync()
    assert np.all(np.isnan(sol.fetch())) and np.all(hx == -3.0) and np.all(hrec == -3.0)
    ev.band_solve_batch_dev(2, _ptr(rhs), sol.ptr)    # (no refusal invalidated the batch of 2)
    records = ev.band_record_batch(2)
    got = sol.fetch().reshape(2, N)
    assert records.shape == (2, 8) and np.all(records[:, 0] == 0.0) and sc.same_bits(got[0], got[1])
