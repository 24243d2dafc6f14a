"""pk_red_rows, pk_red_long and pk_diag (pockit_amd/csrc/pk_reduce.cpp) on the device.

Synthetic structures (tests/reduce_cases.py, tested by tests/test_reduce_cases_cpu.py) go through pk_set_csr_operator into the
contexts of tests/sparse_cases.py -- A brachistochrone(radau, 3, 4), B (radau, 60, 5), C (radau, 200, 8) only for the two
structures beyond the grid cap of 2 048 -- and pk_operator_reduce_dev runs the three modes on them: the "edges" rows, the piece
rows of 65 536 / 65 537 / 131 329 entries, "cut-by-rows", "long-first-and-last", "equal-lengths", ``src`` given and NULL, ``w``
given and NULL; every case with ``add`` NULL, given and aliasing ``y``, ``y`` between sentinels in a NaN-filled tensor.  Asserted:
bit equality with the emulator in every row, the derived bound against ``fsum`` for the sums, equality with the exact maximum
(every planted position), intact sentinels, the same bits from a second call; the full-mantissa case bit-equal to (a a) w.
NaN, zero and negative weights in mode 2: the sentence of the header.  The diagonal on a synthetic ``pos`` at n = 53 and 1 205.

On the six models of tests/test_gpu_csr_operators.py, built the same way: row_norms for each op and kind, h_diag, jdjt_diag,
jtdj_diag with and without H against the same quantities formed with SciPy from the ORACLE's matrices, 1e-11 max(1, max|ref|)
per vector for kinds "1", "inf" and h_diag and twice that for the squared kinds (a relative error delta of an entry is 2 delta
in its square; every term is non-negative for d >= 0, so nothing cancels); host forms bit-equal to the device-pointer forms;
a stale handle raises; a linearization without H raises for the H forms; jv, jtv and hv keep their bits afterwards.
"""
import numpy as np
import pytest

import reduce_cases as rc
import sparse_cases as sc
from test_gpu_csr_operators import CASES as MODELS, TOL, Case
from test_gpu_sparse_kernels import Result, _evaluator, _i32

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]


@pytest.fixture(scope="module")
def context():
    made = {}

    def get(ctx):
        if ctx not in made:
            made[ctx] = ev = _evaluator(ctx)
            c = sc.CONTEXTS[ctx]      # the operators take n_unique from the maps
            assert (ev.csr_map("jac").nnz, ev.csr_map("hess").nnz) == (c["nnz_j"], c["nnz_h"])
        return made[ctx]

    yield get
    for ev in made.values():
        ev.close()


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.device("cuda", 0))


def _run(torch, ev, case, vals, w, add):
    """(plain, again, added, alias) of one structure already uploaded: the four calls of every case."""
    lib, h, dev = ev.ctx.lib, ev.ctx.handle, torch.device("cuda", 0)
    d_vals, d_w, d_add = _up(torch, vals), None if w is None else _up(torch, w), _up(torch, add)
    plain, again, added = (Result(torch, dev, case.n_rows) for _ in range(3))
    alias = Result(torch, dev, case.n_rows, fill=add)
    torch.cuda.synchronize()            # torch's copies run on its own stream; the context uses its own
    for out, a in ((plain, None), (again, None), (added, d_add.data_ptr()), (alias, alias.ptr)):
        ev.ctx.check(lib.pk_operator_reduce_dev(h, case.op, case.mode, d_vals.data_ptr(), None if d_w is None else d_w.data_ptr(),
                                                a, out.ptr, None))
    ev.sync()
    return tuple(r.fetch(f"{case.id} {k}") for r, k in ((plain, "plain"), (again, "again"), (added, "add"), (alias, "alias")))


def _set(ev, case):
    ev.ctx.check(ev.ctx.lib.pk_set_csr_operator(ev.ctx.handle, case.op, _i32(case.indptr), _i32(case.indices), _i32(case.src),
                                                case.n_rows, case.n_cols, case.nnz))


@pytest.mark.parametrize("case", rc.reduce_cases(), ids=lambda c: c.id)
def test_reductions_match_the_exact_rows(case, context):
    import torch

    ev = context(case.ctx)
    _set(ev, case)
    plain, again, added, alias = _run(torch, ev, case, case.vals, case.w if case.with_w else None, case.add)
    assert sc.same_bits(plain, again), f"{case.id}: a second call gave other bits"
    for what, got, with_add in (("add=NULL", plain, False), ("add given", added, True), ("add aliasing y", alias, True)):
        what = f"{case.id} {what}"
        assert not np.any(np.isnan(got)), f"{what}: entries {np.flatnonzero(np.isnan(got))[:8]} were not written"
        emulated = case.emulated(with_add)
        differ = np.flatnonzero(got.view(np.uint64) != emulated.view(np.uint64))
        assert len(differ) == 0, f"{what}: {len(differ)} rows differ in bits from the documented association, first {differ[:8]}"
        if case.mode == rc.ABS_MAX:
            assert sc.same_bits(got, case.max_reference[with_add]), f"{what}: not the exact maximum"
            assert not np.any(np.signbit(got))
        else:
            ref, bound, scale = case.reference[with_add]
            print(f"{what}: worst {sc.worst_units(got, ref, scale):.3e} u*sum|t|, bound {float(sc.gamma(int(case.lengths.max()) + 1) / sc.U):.1f}")
            bad = sc.failures(got, ref, bound)
            assert len(bad) == 0, f"{what}: {len(bad)} rows miss the bound, first {bad[:8]}: {got[bad[:8]]} for {ref[bad[:8]]}"
            exact = bound == 0.0
            assert sc.same_bits(got[exact], ref[exact]), f"{what}: a row that must be exact is not"
    if case.plant is not None:
        row = case.plant[0]
        assert plain[row] == case.terms()[case.planted_entry] == added[row]
    if case.full_mantissa:
        a, w = case.values(), case.w[case.indices]
        assert sc.same_bits(plain, sc.emulate_operator(rc._Mutated(case, (a * a) * w)))
        assert not sc.same_bits(plain, sc.emulate_operator(rc._Mutated(case, a * (a * w))))
    empty = case.lengths == 0
    zero = np.zeros(int(empty.sum()))
    assert sc.same_bits(plain[empty], zero)
    assert sc.same_bits(added[empty], np.maximum(case.add[empty], 0.0) if case.mode == rc.ABS_MAX else case.add[empty])


def test_the_maximum_by_comparison_nan_zero_and_negative_weights(context):
    """"A NaN term loses, the zero padding is the identity, the result is never negative and never -0.0, a negative weight gives
    what the arithmetic gives" -- and the sums carry a NaN."""
    import torch

    case = rc.ReduceCase("A", "specials", 1, [4, 3, 2, 1, 300, 0, 2], seed=99, mode=rc.ABS_MAX)
    ev = context("A")
    _set(ev, case)
    vals, w = case.vals.copy(), case.w.copy()
    e = case.indptr.astype(np.int64)
    used = lambda k: int(case.src[k])  # noqa: E731
    vals[used(e[0] + 1)] = np.nan                                   # row 0: a NaN value among others
    vals[used(e[2])] = vals[used(e[2] + 1)] = 0.0                   # row 2: zeros under negative weights: terms of -0.0
    w[case.indices[e[2]: e[3]]] = -1.5
    vals[used(e[4] + 270)] = np.nan                                 # row 4 (two pieces): a NaN in the second piece
    w[case.indices[e[6]: e[7]]] = -2.0                              # row 6: negative terms only
    t = np.abs(vals[case.src]) * w[case.indices]
    want = np.zeros(case.n_rows)
    for r in range(case.n_rows):
        for x in t[e[r]: e[r + 1]]:
            if x > want[r]:
                want[r] = x
    with_add = np.where(case.add > want, case.add, want)
    plain, again, added, alias = _run(torch, ev, case, vals, w, case.add)
    for got, ref in ((plain, want), (again, want), (added, with_add), (alias, with_add)):
        assert sc.same_bits(got, ref) and not np.any(np.signbit(got))
    assert np.isnan(t[e[0] + 1]) and plain[0] > 0.0 and plain[2] == 0.0 and plain[6] == 0.0 and plain[4] > 0.0
    nan_add = case.add.copy()
    nan_add[3] = np.nan                                             # a NaN add loses like a NaN term
    assert sc.same_bits(_run(torch, ev, case, vals, w, nan_add)[2], np.where(nan_add > want, nan_add, want))
    case.mode = rc.ABS_SUM                                          # the same inputs summed: what the arithmetic gives
    plain = _run(torch, ev, case, vals, w, case.add)[0]
    assert np.isnan(plain[0]) and np.isnan(plain[4]) and plain[6] < 0.0 and plain[2] == 0.0


@pytest.mark.parametrize("ctx", ["A", "B"])
def test_the_diagonal_of_a_synthetic_pos(ctx, context):
    import torch

    ev = context(ctx)
    n, n_unique = sc.CONTEXTS[ctx]["n"], sc.CONTEXTS[ctx]["nnz_h"]
    assert n in (53, 1205)
    pos = rc.diagonal_positions(n, n_unique, seed=n)
    lib, h, dev = ev.ctx.lib, ev.ctx.handle, torch.device("cuda", 0)
    ev.ctx.check(lib.pk_set_operator_diagonal(h, 2, _i32(pos), n))
    rng = np.random.default_rng(n)
    vals, add = rng.standard_normal(n_unique), rng.standard_normal(n)
    d_vals, d_add = _up(torch, vals), _up(torch, add)
    plain, again, added = (Result(torch, dev, n) for _ in range(3))
    alias = Result(torch, dev, n, fill=add)
    torch.cuda.synchronize()
    for out, a in ((plain, None), (again, None), (added, d_add.data_ptr()), (alias, alias.ptr)):
        ev.ctx.check(lib.pk_operator_diagonal_dev(h, 2, d_vals.data_ptr(), a, out.ptr, None))
    ev.sync()
    plain, again, added, alias = (r.fetch(f"diagonal {ctx}") for r in (plain, again, added, alias))
    assert sc.same_bits(plain, np.where(pos >= 0, vals[np.maximum(pos, 0)], 0.0)) and sc.same_bits(plain, again)
    assert sc.same_bits(added, rc.emulate_diagonal(vals, pos, add)) and sc.same_bits(alias, added)
    assert plain[0] == 0.0 and plain[-1] == 0.0
    for bad, length in ((np.where(np.arange(n) == 5, -2, pos), n), (np.where(np.arange(n) == 5, n_unique, pos), n), (pos[:-1], n - 1)):
        assert lib.pk_set_operator_diagonal(h, 2, _i32(bad), length) == 131
    assert lib.pk_set_operator_diagonal(h, 0, _i32(pos), n) == 130
    d_y = torch.zeros(n, dtype=torch.float64, device=dev)
    assert lib.pk_operator_reduce_dev(h, 2, 3, d_vals.data_ptr(), None, None, d_y.data_ptr(), None) == 129
    assert lib.pk_operator_diagonal_dev(h, 1, d_vals.data_ptr(), None, d_y.data_ptr(), None) == 130


# ---------------------------------------------------------------- the models
@pytest.fixture(scope="module", params=MODELS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def model(request):
    c = Case(*request.param)
    rng = np.random.default_rng(11)
    c.dn, c.dm = rng.uniform(0.5, 2.0, c.n), rng.uniform(0.5, 2.0, c.m)
    yield c
    c.system.evaluator.close()


def _close(a, b, what, factor=1.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    err, bound = np.max(np.abs(a - b)), factor * TOL * max(1.0, np.max(np.abs(b)))
    print(f"{what}: err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: err {err:.3e}, bound {bound:.3e}"


def _scipy_norms(A, kind, weights=None):
    B = abs(A) if kind != "2sq" else A.multiply(A)
    if weights is not None:
        B = B.multiply(weights[None, :])
    B = B.tocsr()
    return np.asarray(B.max(axis=1).todense()).reshape(-1) if kind == "inf" else np.asarray(B.sum(axis=1)).reshape(-1)


def test_norms_and_diagonals_match_the_oracle(model):
    lin = model.linearize()
    before = (lin.jv(model.v), lin.jtv(model.y), lin.hv(model.v))
    mats = {"J": (model.J, model.dn), "JT": (model.J.T.tocsr(), model.dm), "H": (model.H, model.dn)}
    for op, (A, weights) in mats.items():
        for kind in ("1", "2sq", "inf"):
            factor = 2.0 if kind == "2sq" else 1.0
            _close(lin.row_norms(op, kind), _scipy_norms(A, kind), f"{op} {kind}", factor)
            _close(lin.row_norms(op, kind, weights), _scipy_norms(A, kind, weights), f"{op} {kind} weighted", factor)
    hd = model.H.diagonal()
    _close(lin.h_diag(), hd, "diag H")
    jdjt = _scipy_norms(model.J, "2sq", model.dn)
    jtdj = _scipy_norms(model.J.T.tocsr(), "2sq", model.dm)
    _close(lin.jdjt_diag(model.dn), jdjt, "diag J D J^T", 2.0)
    _close(lin.jtdj_diag(model.dm), jtdj, "diag J^T D J", 2.0)
    _close(lin.jtdj_diag(model.dm, with_h=True), hd + jtdj, "diag(H + J^T D J)", 2.0)      # a squared kind: twice the rule
    both = lin.jtdj_diag(model.dm, with_h=True)
    assert np.array_equal(both, lin.h_diag() + lin.jtdj_diag(model.dm))          # the same two roundings per row
    assert np.array_equal(lin.row_norms("J", "2sq", model.dn), lin.jdjt_diag(model.dn))
    after = (lin.jv(model.v), lin.jtv(model.y), lin.hv(model.v))                 # the partial-sum slots are shared
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        lin.row_norms("J", "2")
    with pytest.raises(ValueError):
        lin.row_norms("J", "1", model.dm if model.m != model.n else model.dm[:-1])


def test_host_forms_equal_the_device_pointer_forms_bit_for_bit(model):
    import torch

    ev = model.system.evaluator
    lin = model.linearize()
    host = {(op, kind, weighted): lin.row_norms(op, kind, (model.dm if op == "JT" else model.dn) if weighted else None)
            for op in ("J", "JT", "H") for kind in ("1", "2sq", "inf") for weighted in (False, True)}
    host_diag, host_both = lin.h_diag(), lin.jtdj_diag(model.dm, with_h=True)
    dev = torch.device("cuda", 0)
    dx, dlam = _up(torch, model.x), _up(torch, model.lam)
    cj = torch.zeros(ev.csr_map("jac").nnz, dtype=torch.float64, device=dev)
    ch = torch.zeros(ev.csr_map("hess").nnz, dtype=torch.float64, device=dev)
    d_n, d_m = _up(torch, model.dn), _up(torch, model.dm)
    torch.cuda.synchronize()
    ev.jacobian_csr_dev(dx.data_ptr(), cj.data_ptr())
    ev.hessian_csr_dev(dx.data_ptr(), dlam.data_ptr(), model.sigma, ch.data_ptr())
    for call in (lambda: lin.row_norms("J", "1"), lin.h_diag, lambda: lin.jdjt_diag(model.dn), lambda: lin.jtdj_diag(model.dm)):
        with pytest.raises(RuntimeError, match="stale"):      # (those calls gave the context's buffers another evaluation)
            call()
    modes = {"1": "abs_sum", "2sq": "sq_sum", "inf": "abs_max"}
    rows = {"J": model.m, "JT": model.n, "H": model.n}
    outs = {}
    for key in host:
        op, kind, weighted = key
        outs[key] = out = torch.full((rows[op],), np.nan, dtype=torch.float64, device=dev)
        d_w = (d_m if op == "JT" else d_n).data_ptr() if weighted else None
        ev.operator_reduce_dev(op, modes[kind], (ch if op == "H" else cj).data_ptr(), out.data_ptr(), d_w=d_w)
    diag = torch.full((model.n,), np.nan, dtype=torch.float64, device=dev)
    both = torch.full((model.n,), np.nan, dtype=torch.float64, device=dev)
    ev.operator_diagonal_dev("H", ch.data_ptr(), diag.data_ptr())
    ev.operator_diagonal_dev("H", ch.data_ptr(), both.data_ptr())
    ev.operator_reduce_dev("JT", "sq_sum", cj.data_ptr(), both.data_ptr(), d_w=d_m.data_ptr(), d_add=both.data_ptr())
    ev.sync()
    for key, out in outs.items():
        assert np.array_equal(out.cpu().numpy(), host[key]), key
    assert np.array_equal(diag.cpu().numpy(), host_diag) and np.array_equal(both.cpu().numpy(), host_both)
    with pytest.raises(ValueError):
        ev.operator_diagonal_dev("J", cj.data_ptr(), diag.data_ptr())
    with pytest.raises(ValueError):
        ev.operator_reduce_dev("J", "sum", cj.data_ptr(), diag.data_ptr())


def test_the_h_forms_raise_without_a_hessian_and_every_form_on_a_stale_handle(model):
    first = model.linearize()
    first.h_diag()
    no_h = model.system.linearize(model.x)                  # the context's one linearization is now this one
    for call in (first.h_diag, lambda: first.row_norms("JT", "inf"), lambda: first.jtdj_diag(model.dm, with_h=True)):
        with pytest.raises(RuntimeError, match="stale"):
            call()
    _close(no_h.row_norms("J", "1"), _scipy_norms(model.J, "1"), "J 1 without a Hessian")
    _close(no_h.jtdj_diag(model.dm), _scipy_norms(model.J.T.tocsr(), "2sq", model.dm), "diag J^T D J without a Hessian", 2.0)
    for call in (no_h.h_diag, lambda: no_h.row_norms("H", "1"), lambda: no_h.jtdj_diag(model.dm, with_h=True)):
        with pytest.raises(RuntimeError, match="no Hessian"):
            call()
