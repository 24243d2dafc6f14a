"""The slacks of a resident iterate (pockit_amd/csrc/pk_slack.cpp) on the device.

The four kernels and the scalar step through ``pk_slack_raw_dev`` on the context of brachistochrone(radau, 3, 4): row lengths 1,
255, 256, 257, 2 047, 2 048, 2 049, 524 289 (257 pieces: the second strided trip of the scalar step) and 4 194 305 (2 049 pieces:
past the grid cap, the stride loop of a workgroup runs), the variables' range beside them at most 2 049 long.  Full-mantissa data,
NaN wherever a kernel must not read, outputs between sentinels in NaN-filled tensors; every vector and every record slot but the
merit's ``log_sum`` bit-equal to the emulator of tests/slack_cases.py, the same bits from a second call.  ``log_sum``: the
device's log is not NumPy's, so it is held to ``|dev - emu| <= (2 * 2^-52 + ceil(log2 L + 1) * 2^-52) * sum |ln term|`` -- one ulp
per term on each side plus both sides' tree rounding (slack_cases.merit_log_bound, DESIGN.md section 21's bound).  Planted
defects, all-equality and all-inequality rows, an already clamped multiplier, alpha = 0.

Models (the cases of tests/test_gpu_csr_operators.py, with a mix of equality, two-sided and one-sided rows set over the plan's
bounds): the host forms bit-equal to the emulator on inputs that owe nothing to the oracle; the chain terms -> slack_reduce ->
dual_residual -> MINRES (12 iterations) -> slack_recover -> ip_step -> slack_update on device pointers with one wait against the
same chain through the host forms; the refusals; the other products of the handle unchanged."""
import ctypes as C

import numpy as np
import pytest

import ipm_cases as ip
import slack_cases as sl
import sparse_cases as sc
from device_cases import Buf, _ptr, _same, _sync, _up, step_ev  # noqa: F401  (step_ev: a fixture)
from test_gpu_csr_operators import CASES, Case

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]

MU, TAU, AP, AD, KAPPA = 0.0625 * 1.37, 0.995, 0.8125 * 0.93, 0.71, 10.0
ROW_KEYS = ("lb", "ub", "g", "s", "lam", "dlam", "sigma_s", "rbar_s", "s2", "ds", "dv", "zl", "zu", "dzl", "dzu")


def _raw(ev, kind, n, m, batch, xlb, xub, clb, cub, ptrs, out, ap=AP, ad=AD, mu=MU, kappa=KAPPA):
    table = (C.c_void_p * 10)(*([_ptr(p) for p in ptrs] + [None] * (10 - len(ptrs))))
    return ev.ctx.lib.pk_slack_raw_dev(ev.ctx.handle, kind, n, m, batch, _ptr(xlb), _ptr(xub), _ptr(clb), _ptr(cub), table, float(ap), float(ad),
                                       float(mu), float(kappa), _ptr(out), None)


def _run_all(ev, x, b, X, G, alphas, kappa=KAPPA, ap=AP, ad=AD):
    """The four kinds on one set of vectors, each twice: per run [s2, b2, rec4, ds, rec5, v, zl, zu, lam, rec4, table]."""
    n, m, batch = len(x["lb"]), len(b["lb"]), len(alphas)
    d = {k: _up(b[k]) for k in ROW_KEYS}
    dx = {k: _up(x[k]) for k in ("lb", "ub", "dx", "w", "s1")}
    dX, dG, da = _up(X), _up(G), _up(alphas)
    runs = []
    for _ in range(2):
        s2, b2, r4, ds, r5, r4b, table = Buf(m), Buf(m), Buf(4), Buf(m), Buf(5), Buf(4), Buf(4 * batch)
        v, zl, zu, lam = Buf(m, b["v"]), Buf(m, b["zl"]), Buf(m, b["zu"]), Buf(m, b["lam"])
        _sync()
        ev.ctx.check(_raw(ev, sl.REDUCE, 0, m, 1, None, None, d["lb"], d["ub"], [d["g"], d["s"], d["lam"], d["sigma_s"], d["rbar_s"], s2, b2], r4))
        ev.ctx.check(_raw(ev, sl.RECOVER, n, m, 1, dx["lb"], dx["ub"], d["lb"], d["ub"],
                          [d["dlam"], d["lam"], d["rbar_s"], d["s2"], d["sigma_s"], dx["dx"], dx["w"], dx["s1"], ds], r5))
        ev.ctx.check(_raw(ev, sl.UPDATE, 0, m, 1, None, None, d["lb"], d["ub"], [v, d["dv"], zl, d["dzl"], zu, d["dzu"], lam, d["dlam"]], r4b,
                          ap=ap, ad=ad, kappa=kappa))
        ev.ctx.check(_raw(ev, sl.MERIT, n, m, batch, dx["lb"], dx["ub"], d["lb"], d["ub"], [dX, dG, d["s"], d["ds"], da], table))
        ev.sync()
        runs.append([q.fetch() for q in (s2, b2, r4, ds, r5, v, zl, zu, lam, r4b, table)])
    return runs


NAMES = ("s2", "b2", "record of reduce", "ds", "record of recover", "v", "zl", "zu", "lam", "record of update", "merit table")


def _emulate(x, b, X, G, alphas, kappa=KAPPA, ap=AP, ad=AD):
    want = list(sl.emulate_reduce(b["lb"], b["ub"], b["g"], b["s"], b["lam"], b["sigma_s"], b["rbar_s"]))
    want += sl.emulate_recover(x["lb"], x["ub"], b["lb"], b["ub"], b["dlam"], b["lam"], b["rbar_s"], b["s2"], b["sigma_s"], x["dx"], x["w"], x["s1"])
    want += sl.emulate_update(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["dzl"], b["zu"], b["dzu"], ap, ad, MU, kappa, b["lam"], b["dlam"])
    want.append(sl.emulate_merit(x["lb"], x["ub"], b["lb"], b["ub"], X, G, b["s"], b["ds"], alphas))
    return want


def _same_but_nan(what, got, want):
    """Bit for bit, a NaN for a NaN: where a planted NaN passes through arithmetic its sign and payload are the platform's."""
    got, want = np.asarray(got), np.asarray(want)
    both = np.isnan(got) & np.isnan(want)
    _same(what, np.where(both, 0.0, got), np.where(both, 0.0, want))


def _check(ev, x, b, X, G, alphas, what, planted=False, **kw):
    first, second = _run_all(ev, x, b, X, G, alphas, **kw)
    want = _emulate(x, b, X, G, alphas, **kw)
    for name, got, again, ref in zip(NAMES, first, second, want):
        assert sc.same_bits(got, again), f"{what} {name}: a second call gave other bits"
        if name != "merit table":
            (_same_but_nan if planted else _same)(f"{what} {name}", got, ref)
    table, ref = first[-1].reshape(-1, 4), want[-1]
    keep = [q for q in range(4) if q != sl.M_LOG]
    _same(f"{what} merit table", np.ascontiguousarray(table[:, keep]), np.ascontiguousarray(ref[:, keep]))
    for k, alpha in enumerate(alphas):
        with np.errstate(invalid="ignore"):
            bound = sl.merit_log_bound(x["lb"], x["ub"], b["lb"], b["ub"], X[k], b["s"] + alpha * b["ds"])
        err = abs(table[k, sl.M_LOG] - ref[k, sl.M_LOG])
        print(f"{what} entry {k}: log_sum device {table[k, sl.M_LOG]!r}, emulator {ref[k, sl.M_LOG]!r}, |difference| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, f"{what}: log_sum of entry {k} differs by {err:.3e}, bound {bound:.3e}"
    return first, want


@pytest.mark.parametrize("length", sl.LENGTHS + (sl.LENGTH_PAST_THE_PIECE_CAP,))
def test_the_kernels_match_the_emulator_bit_for_bit(step_ev, length):
    x, b = sl.variables(min(length, 2049)), sl.rows(length)
    X, G, alphas = sl.trial_points(x, b, 2 if length > 600000 else 3)
    _, want = _check(step_ev, x, b, X, G, alphas, f"clean, length {length}")
    assert want[2][sl.RED_BAD] == 0.0 and want[4][sl.REC_BAD] == 0.0 and want[9][sl.UPD_BAD] == 0.0 and not want[10][:, sl.M_BAD].any()


def test_the_variables_range_past_one_piece(step_ev):
    """35 pieces of variables in front of one piece of rows (an empty range is the CPU driver's: a device tensor of no
    elements has no address to pass)."""
    x, b = sl.variables(70001), sl.rows(300)
    X, G, alphas = sl.trial_points(x, b, 3)
    _check(step_ev, x, b, X, G, alphas, "n 70001, m 300")


@pytest.mark.parametrize("n,m", ((300, 257), (2049, 4500)))
def test_planted_defects_are_counted_and_left_out(step_ev, n, m):
    x, b = sl.variables(n), sl.rows(m)
    X, G, alphas = sl.trial_points(x, b, 3)
    sl.plant(x, b, X, G)
    got, _ = _check(step_ev, x, b, X, G, alphas, f"planted, n {n}, m {m}", planted=True)
    s2, b2, r4, ds, r5, v, zl, zu, lam, r4b, table = got
    assert r4[sl.RED_BAD] == 3.0 and r5[sl.REC_BAD] == 3.0 and r4b[sl.UPD_BAD] == 3.0 and table.reshape(-1, 4)[:, sl.M_BAD].tolist() == [2.0, 2.0, 3.0]
    assert all(np.all(np.isfinite(a)) for a in (r4, r5, r4b[:1], table, s2, ds, np.delete(b2, 2)))
    assert s2[0] == b2[0] == s2[1] == b2[1] == ds[0] == ds[1] == 0.0 and np.isnan(b2[2]) and np.isnan(v[3]) and np.isinf(zl[4])
    assert zu[5] == b["zu"][5] + AD * b["dzu"][5]          # (a slack that is not positive: the multiplier stored as computed, not clamped)


def test_all_equality_and_all_inequality_rows(step_ev):
    x = sl.variables(300)
    for kinds, rows_counted in ((ip.FIXED, 0.0), (ip.BOTH, 2500.0), (ip.FREE, 2500.0)):
        b = sl.rows(2500, kinds=kinds)
        if kinds == ip.FREE:                       # a free slack has sigma_s = 0: every row is bad, every output 0.0
            b["sigma_s"] = np.zeros(2500)
        X, G, alphas = sl.trial_points(x, b, 2)
        got, _ = _check(step_ev, x, b, X, G, alphas, f"rows of kind {kinds}")
        s2, b2, r4, ds, r5 = got[:5]
        assert r4[sl.RED_ROWS] == rows_counted
        if kinds == ip.FIXED:
            assert not s2.any() and not ds.any() and sc.same_bits(b2, -(b["g"] - b["lb"])) and r5[sl.CURV_S] == 0.0 and r5[sl.DS_SQ] == 0.0
            for name, after, before in zip(("v", "zl", "zu"), got[5:8], (b["v"], b["zl"], b["zu"])):
                assert sc.same_bits(after, before), f"an equality row's {name} was written"
        if kinds == ip.FREE:
            assert r4[sl.RED_BAD] == 2500.0 and not s2.any() and not b2.any() and not ds.any() and r4[sl.THETA_1] == 0.0


def test_an_already_clamped_multiplier_stays_and_alpha_zero_leaves_every_bit(step_ev):
    x, b = sl.variables(300), sl.rows(3000, kinds=ip.BOTH)
    X, G, alphas = sl.trial_points(x, b, 2)
    got, _ = _check(step_ev, x, b, X, G, alphas, "alpha = 0", ap=0.0, ad=0.0, kappa=1e10)
    for name, after, before in zip(("v", "zl", "zu", "lam"), got[5:9], (b["v"], b["zl"], b["zu"], b["lam"])):
        assert sc.same_bits(after, before), f"alpha = 0 changed {name}"
    assert got[9][sl.CLAMPED] == 0.0
    b["zl"][:40], b["zu"][:40] = 1e-30, 1e30
    got, _ = _check(step_ev, x, b, X, G, alphas, "clamped from both sides", ap=0.0, ad=0.0, kappa=2.0)
    assert got[9][sl.CLAMPED] >= 80.0
    with np.errstate(invalid="ignore"):
        assert sc.same_bits(got[6][:40], MU / (2.0 * (b["v"] - b["lb"]))[:40]) and sc.same_bits(got[7][:40], ((2.0 * MU) / (b["ub"] - b["v"]))[:40])
    b["zl"], b["zu"] = got[6], got[7]
    again, _ = _check(step_ev, x, b, X, G, alphas, "already clamped", ap=0.0, ad=0.0, kappa=2.0)
    assert again[9][sl.CLAMPED] == 0.0 and sc.same_bits(again[6], got[6]) and sc.same_bits(again[7], got[7])


# ---------------------------------------------------------------- models
class SlackInputs:
    """Per model the bounds (every fourth row an equality as the plan has it, the others two-sided, lower-only and upper-only
    around the plan's), the iterate with slacks and its steps; they owe nothing to the oracle."""

    def __init__(self, case):
        p = case.system.evaluator.plan
        rng = np.random.default_rng(13)
        n, m = case.n, case.m
        k = np.arange(m) % 4
        c_lb, c_ub = np.asarray(p.c_lb, dtype=np.float64), np.asarray(p.c_ub, dtype=np.float64)
        self.c_lb = np.where(k == 0, c_lb, np.where(k == 3, -np.inf, c_lb - 1.0))
        self.c_ub = np.where(k == 0, c_ub, np.where(k == 2, np.inf, c_ub + 1.0))
        self.v_lb, self.v_ub = np.asarray(p.v_lb, dtype=np.float64), np.asarray(p.v_ub, dtype=np.float64)
        self.x = ip.inside(self.v_lb, self.v_ub, case.x)
        self.s = ip.inside(self.c_lb, self.c_ub, np.zeros(m))
        self.zl, self.zu, self.yl, self.yu = (rng.uniform(0.1, 1.0, count) for count in (n, n, m, m))
        self.g = self.s + rng.uniform(-0.5, 0.5, m)
        self.grad, self.lam = rng.standard_normal(n), rng.standard_normal(m)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def case(request):
    c = Case(*request.param)
    c.slack = q = SlackInputs(c)
    c.system.evaluator.set_bounds(q.c_lb, q.c_ub, q.v_lb, q.v_ub)
    yield c
    c.system.evaluator.close()


def _chain_host(case, iters):
    ev, q, n = case.system.evaluator, case.slack, case.n
    lin = case.linearize()
    tx = ev.barrier_terms(q.x, q.zl, q.zu, MU)
    ts = ev.barrier_terms(q.s, q.yl, q.yu, MU, which="c")
    red = ev.slack_terms(q.g, q.s, q.lam, ts.sigma, ts.rbar)
    b1, res = lin.dual_residual(q.grad, q.lam, z=tx.rbar, negate=True)
    rhs = np.concatenate((b1, red.b2))
    sol, _ = lin.solve_kkt(rhs, s1=tx.sigma, s2=red.s2, precond=None, tol=0.0, maxiter=iters, check_every=iters)
    dx, dlam = sol[:n].copy(), sol[n:].copy()
    step = ev.slack_step(dlam, q.lam, ts.rbar, red.s2, ts.sigma, dx, lin.hv(dx), tx.sigma)
    bx = ev.boundary_step(q.x, dx, q.zl, q.zu, MU, TAU)
    bs = ev.boundary_step(q.s, step.ds, q.yl, q.yu, MU, TAU, which="c")
    ux = ev.update_iterate(q.x, dx, q.zl, bx.dzl, q.zu, bx.dzu, AP, AD, MU, KAPPA)
    us = ev.update_iterate(q.s, step.ds, q.yl, bs.dzl, q.yu, bs.dzu, AP, AD, MU, KAPPA, lam=q.lam, dlam=dlam, which="c")
    return (red.s2, red.table, rhs, sol, step.ds, step.table, bx.table, bs.table, ux.v, ux.zl, ux.zu, ux.table, us.v, us.zl, us.zu, us.lam, us.table)


def _chain_device(case, iters):
    ev, q, n, m = case.system.evaluator, case.slack, case.n, case.m
    dx0, dlam0 = _up(case.x), _up(case.lam)
    x, zl, zu, s, yl, yu, lam = (Buf(len(a), a) for a in (q.x, q.zl, q.zu, q.s, q.yl, q.yu, q.lam))
    g, grad = _up(q.g), _up(q.grad)
    cj, ch = Buf(ev.csr_map("jac").nnz), Buf(ev.csr_map("hess").nnz)
    sig_x, rbar_x, sig_s, rbar_s, s2, w, ds = Buf(n), Buf(n), Buf(m), Buf(m), Buf(m), Buf(n), Buf(m)
    rhs, sol = Buf(n + m), Buf(n + m)
    dzl, dzu, dyl, dyu = Buf(n), Buf(n), Buf(m), Buf(m)
    r8x, r8s, r4, r4d, r5, r4x, r4s, r4ux, r4us = Buf(8), Buf(8), Buf(4), Buf(4), Buf(5), Buf(4), Buf(4), Buf(4), Buf(4)
    _sync()
    ev.jacobian_csr_dev(dx0.data_ptr(), cj.ptr)
    ev.hessian_csr_dev(dx0.data_ptr(), dlam0.data_ptr(), case.sigma, ch.ptr)
    ev.ip_terms_dev(x.ptr, zl.ptr, zu.ptr, MU, sig_x.ptr, rbar_x.ptr, r8x.ptr)
    ev.ip_terms_dev(s.ptr, yl.ptr, yu.ptr, MU, sig_s.ptr, rbar_s.ptr, r8s.ptr, which="c")
    ev.slack_reduce_dev(_ptr(g), s.ptr, lam.ptr, sig_s.ptr, rbar_s.ptr, s2.ptr, rhs.ptr + 8 * n, r4.ptr)
    ev.dual_residual_dev(cj.ptr, _ptr(grad), lam.ptr, rhs.ptr, r4d.ptr, d_z=rbar_x.ptr, negate=True)
    ev.minres_begin_dev(cj.ptr, rhs.ptr, sol.ptr, 0.0, d_hvals=ch.ptr, d_s1=sig_x.ptr, d_s2=s2.ptr)
    ev.minres_advance_dev(iters)
    ev.apply_operator_dev("H", ch.ptr, sol.ptr, w.ptr)
    ev.slack_recover_dev(sol.ptr + 8 * n, lam.ptr, rbar_s.ptr, s2.ptr, sig_s.ptr, sol.ptr, w.ptr, sig_x.ptr, ds.ptr, r5.ptr)
    ev.ip_step_dev(x.ptr, sol.ptr, zl.ptr, zu.ptr, MU, TAU, dzl.ptr, dzu.ptr, r4x.ptr)
    ev.ip_step_dev(s.ptr, ds.ptr, yl.ptr, yu.ptr, MU, TAU, dyl.ptr, dyu.ptr, r4s.ptr, which="c")
    ev.slack_update_dev(x.ptr, sol.ptr, zl.ptr, dzl.ptr, zu.ptr, dzu.ptr, AP, AD, MU, r4ux.ptr, kappa=KAPPA)
    ev.slack_update_dev(s.ptr, ds.ptr, yl.ptr, dyl.ptr, yu.ptr, dyu.ptr, AP, AD, MU, r4us.ptr, kappa=KAPPA, d_lam=lam.ptr, d_dlam=sol.ptr + 8 * n,
                        which="c")
    ev.sync()                                   # the one wait; everything comes down behind it
    return tuple(a.fetch() for a in (s2, r4, rhs, sol, ds, r5, r4x, r4s, x, zl, zu, r4ux, s, yl, yu, lam, r4us))


CHAIN = ("s2", "record of reduce", "b", "solution", "ds", "record of recover", "record of the step of x", "record of the step of s", "x", "zl", "zu",
         "record of the update of x", "s", "yl", "yu", "lam", "record of the update of s")


def test_the_host_forms_match_the_emulator_and_the_chains_agree(case):
    """terms -> slack_reduce -> dual_residual -> 12 MINRES iterations on [[H + Sigma_x, J^T], [J, -S2]] -> slack_recover ->
    ip_step -> slack_update, once with every array resident and one wait at the end, once through the host forms with a
    download and an upload between every stage: the same bits, so no stage depends on who owns the memory.  The host forms of
    this unit against the emulator on the chain's own intermediate vectors: bit for bit."""
    ev, q, n = case.system.evaluator, case.slack, case.n
    host = _chain_host(case, 12)
    dev = _chain_device(case, 12)
    for name, h, g in zip(CHAIN, host, dev):
        _same(f"chain {name}", g, h)
    free_rows = np.sum(~np.isfinite(q.c_lb) & ~np.isfinite(q.c_ub))      # (a slack without a side has sigma_s = 0: counted in bad)
    assert np.all(np.isfinite(host[3])) and host[1][sl.RED_ROWS] == np.sum(q.c_lb != q.c_ub) and host[1][sl.RED_BAD] == free_rows
    # the emulator on the same inputs
    ts = ev.barrier_terms(q.s, q.yl, q.yu, MU, which="c")
    tx = ev.barrier_terms(q.x, q.zl, q.zu, MU)
    s2, b2, rec = sl.emulate_reduce(q.c_lb, q.c_ub, q.g, q.s, q.lam, ts.sigma, ts.rbar)
    _same("host s2", host[0], s2)
    _same("host b2", host[2][n:], b2)
    _same("host record of reduce", host[1], rec)
    dx, dlam = host[3][:n].copy(), host[3][n:].copy()
    w = case.linearize().hv(dx)
    ds, rec5 = sl.emulate_recover(q.v_lb, q.v_ub, q.c_lb, q.c_ub, dlam, q.lam, ts.rbar, s2, ts.sigma, dx, w, tx.sigma)
    _same("host ds", host[4], ds)
    _same("host record of recover", host[5], rec5)
    bx = ev.boundary_step(q.x, dx, q.zl, q.zu, MU, TAU)
    bs = ev.boundary_step(q.s, ds, q.yl, q.yu, MU, TAU, which="c")
    ux = sl.emulate_update(q.v_lb, q.v_ub, q.x, dx, q.zl, bx.dzl, q.zu, bx.dzu, AP, AD, MU, KAPPA)
    us = sl.emulate_update(q.c_lb, q.c_ub, q.s, ds, q.yl, bs.dzl, q.yu, bs.dzu, AP, AD, MU, KAPPA, q.lam, dlam)
    for name, got, want in zip(CHAIN[8:], host[8:], (ux[0], ux[1], ux[2], ux[4], us[0], us[1], us[2], us[3], us[4])):
        _same(f"host {name}", got, want)


def test_refusals_with_their_codes_and_nothing_written(case):
    import models
    import pockit_amd.radau as radau
    from pockit_amd import runtime

    ev, q, n, m = case.system.evaluator, case.slack, case.n, case.m
    as_dp = runtime.as_dp
    lib, h = ev.ctx.lib, ev.ctx.handle
    ev.barrier_terms(q.x, q.zl, q.zu, MU)                # (the bounds are up)
    o1, o2, rec = np.full(m, -3.0), np.full(m, -3.0), np.full(8, -3.0)
    rows = [as_dp(a) for a in (q.g, q.s, q.lam, q.yl, q.yu)]
    assert lib.pk_slack_reduce(h, None, *rows[1:], as_dp(o1), as_dp(o2), as_dp(rec)) == 60
    assert lib.pk_slack_reduce(h, *rows, as_dp(o1), as_dp(o2), None) == 60
    assert lib.pk_slack_update(h, 2, as_dp(o1), rows[0], as_dp(o2), rows[1], as_dp(o2), rows[2], None, None, AP, AD, MU, KAPPA, as_dp(rec)) == 134
    assert lib.pk_slack_update(h, 1, as_dp(o1), rows[0], as_dp(o2), rows[1], as_dp(o2), rows[2], None, None, 1.5, AD, MU, KAPPA, as_dp(rec)) == 134
    assert lib.pk_slack_update(h, 1, as_dp(o1), rows[0], as_dp(o2), rows[1], as_dp(o2), rows[2], None, None, AP, AD, -MU, KAPPA, as_dp(rec)) == 134
    assert lib.pk_slack_update(h, 1, as_dp(o1), rows[0], as_dp(o2), rows[1], as_dp(o2), rows[2], None, None, AP, AD, MU, 0.5, as_dp(rec)) == 134
    assert lib.pk_slack_update(h, 1, as_dp(o1), rows[0], as_dp(o2), rows[1], as_dp(o2), rows[2], as_dp(o1), None, AP, AD, MU, KAPPA, as_dp(rec)) == 60
    dev_o, dev_rec = Buf(max(n, m)), Buf(8)
    d = {k: _up(a) for k, a in (("g", q.g), ("s", q.s), ("lam", q.lam), ("yl", q.yl), ("yu", q.yu), ("x", q.x))}
    _sync()
    p = {k: _ptr(t) for k, t in d.items()}
    assert lib.pk_slack_reduce_dev(h, None, p["s"], p["lam"], p["yl"], p["yu"], dev_o.ptr, dev_o.ptr, dev_rec.ptr, None) == 110
    assert lib.pk_slack_recover_dev(h, p["lam"], p["lam"], p["yl"], p["yl"], p["yu"], p["x"], None, p["x"], dev_o.ptr, dev_rec.ptr, None) == 110
    assert lib.pk_slack_update_dev(h, 0, dev_o.ptr, p["x"], dev_o.ptr, p["x"], dev_o.ptr, p["x"], dev_o.ptr, p["x"], AP, AD, MU, KAPPA, dev_rec.ptr, None) == 134
    assert lib.pk_slack_update_dev(h, 1, dev_o.ptr, p["s"], dev_o.ptr, p["s"], dev_o.ptr, p["s"], None, None, AP, 2.0, MU, KAPPA, dev_rec.ptr, None) == 134
    assert lib.pk_slack_merit_dev(h, 0, p["x"], p["g"], p["s"], p["s"], p["x"], dev_rec.ptr, None) == 134
    assert lib.pk_slack_merit_dev(h, 1, p["x"], None, p["s"], p["s"], p["x"], dev_rec.ptr, None) == 110
    assert _raw(ev, 4, n, m, 1, d["x"], d["x"], d["s"], d["s"], [d["g"]] * 9, dev_rec) == 134
    ev.sync()
    assert np.all(o1 == -3.0) and np.all(o2 == -3.0) and np.all(rec == -3.0)
    assert np.all(np.isnan(dev_o.fetch())) and np.all(np.isnan(dev_rec.fetch()))
    with pytest.raises(ValueError):
        ev.slack_terms(q.g[:-1], q.s, q.lam, q.yl, q.yu)
    with pytest.raises(ValueError):
        ev.update_iterate(q.x, q.x, q.zl, q.zl, q.zu, q.zu, AP, AD, MU, lam=q.lam, dlam=q.lam, which="x")
    # no bounds: a context that never had them
    fresh = models.brachistochrone(radau, 3, 4)[0].evaluator
    try:
        k = fresh.plan.m
        v, w1, w2, out4 = np.zeros(k), np.full(k, -3.0), np.full(k, -3.0), np.full(4, -3.0)
        assert fresh.ctx.lib.pk_slack_reduce(fresh.ctx.handle, as_dp(v), as_dp(v), as_dp(v), as_dp(v), as_dp(v), as_dp(w1), as_dp(w2), as_dp(out4)) == 123
        assert np.all(out4 == -3.0) and np.all(w1 == -3.0) and np.all(w2 == -3.0)
    finally:
        fresh.close()


def test_the_other_products_of_the_handle_return_the_bits_they_returned_before(case):
    ev, q = case.system.evaluator, case.slack
    rhs = np.random.default_rng(3).standard_normal(case.n + case.m)
    d = np.random.default_rng(4).standard_normal(case.n)
    scan = ev.merit_scan(case.x, d, [0.0, 0.5, 1.0])
    terms = ev.barrier_terms(q.x, q.zl, q.zu, MU)
    lin = case.linearize()               # (merit_scan gave the context another evaluation)
    others = lambda: (lin.solve_kkt(rhs, 2.0, 0.5, precond=None, tol=1e-8, maxiter=16)[0], lin.jv(case.v), lin.row_norms("J", "1"))  # noqa: E731
    before = others()
    ts = ev.barrier_terms(q.s, q.yl, q.yu, MU, which="c")
    red = ev.slack_terms(q.g, q.s, q.lam, ts.sigma, ts.rbar)
    step = ev.slack_step(q.lam, q.lam, ts.rbar, red.s2, ts.sigma, d, d, terms.sigma)
    ev.update_iterate(q.s, step.ds, q.yl, q.yl, q.yu, q.yu, AP, AD, MU, which="c", lam=q.lam, dlam=q.lam)
    for a, b in zip(before, others()):
        assert np.array_equal(a, b)
    assert np.array_equal(scan, ev.merit_scan(case.x, d, [0.0, 0.5, 1.0]))
    again = ev.barrier_terms(q.x, q.zl, q.zu, MU)
    assert sc.same_bits(again.table, terms.table) and sc.same_bits(again.sigma, terms.sigma)
