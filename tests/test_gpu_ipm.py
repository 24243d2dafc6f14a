"""Barrier terms, dual residual and boundary step of pockit_amd/csrc/pk_ipm.cpp on the device.

The three kernels and the scalar step through ``pk_ip_raw_dev`` on the context of brachistochrone(radau, 3, 4): lengths 1, 255, 256,
257, 2 047, 2 048, 2 049, 524 289 (257 pieces: the second strided trip of the scalar step) and 4 194 305 (2 049 pieces: past the
grid cap, the stride loop of a workgroup runs).  Full-mantissa data, NaN wherever a kernel must not read, outputs between
sentinels in NaN-filled tensors; every vector and every record slot but slot 4 bit-equal to the emulator of tests/ipm_cases.py
(the divisions rest on DESIGN.md section 19's finding that ``/`` is the correctly rounded one on this hardware), the same bits
from a second call.  Slot 4, the sum of logarithms: the device's log is not NumPy's, so it is held to
``|dev - emu| <= (2 * 2^-52 + ceil(log2 L + 1) * 2^-52) * sum |ln term|`` -- one ulp per term on each side plus both sides' tree
rounding (ipm_cases.log_bound).  Planted defects, the identities of vectors without a side, a tie of three indices, dv = 0.

Models (the cases of tests/test_gpu_csr_operators.py, the plan's bounds): the host forms bit-equal to the emulator on inputs that
owe nothing to the oracle; ``dual_residual`` against SciPy on the ORACLE's J at ``3 * 1e-11 * max(1, max|ref|)``, and with
``z = None`` the bits of ``jtv(lam) + grad``; the chain linearize -> terms -> residual -> MINRES -> step on device pointers with
one download against the same chain through the host forms; the refusals; the other products of the handle unchanged."""
import numpy as np
import pytest

import ipm_cases as ip
import models
import sparse_cases as sc
from device_cases import Buf, _ptr, _same, _sync, _up, step_ev  # noqa: F401  (step_ev: a fixture)
from test_gpu_csr_operators import CASES, Case

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]

MU, TAU = 0.0625 * 1.37, 0.995


def _raw(ev, kind, length, lb, ub, v=None, dv=None, zl=None, zu=None, t=None, z=None, negate=False, mu=MU, tau=TAU, o1=None, o2=None, out=None):
    return ev.ctx.lib.pk_ip_raw_dev(ev.ctx.handle, kind, length, _ptr(lb), _ptr(ub), _ptr(v), _ptr(dv), _ptr(zl), _ptr(zu), _ptr(t), _ptr(z),
                                    int(negate), float(mu), float(tau), _ptr(o1), _ptr(o2), _ptr(out), None)


def _check_record(what, got, want, b, length):
    keep = [q for q in range(8) if q != ip.LOG_SUM]
    _same(what + " record", got[keep], want[keep])
    bound = ip.log_bound(b["lb"], b["ub"], b["v"], b["zl"], b["zu"], length)
    err = abs(got[ip.LOG_SUM] - want[ip.LOG_SUM])
    print(f"{what}: log_sum device {got[ip.LOG_SUM]!r}, emulator {want[ip.LOG_SUM]!r}, |difference| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: log_sum differs by {err:.3e}, bound {bound:.3e}"


def _run_all(ev, b, length):
    """The three kinds at one length on one boxed vector, each twice: [(sigma, rbar, rec8), (r, rec4), (dzl, dzu, rec4)] per run."""
    d = {k: _up(b[k]) for k in ("lb", "ub", "v", "dv", "zl", "zu", "t", "z")}
    runs = []
    for _ in range(2):
        s, rb, r8 = Buf(length), Buf(length), Buf(8)
        r, r4 = Buf(length), Buf(4)
        dl, du, r4b = Buf(length), Buf(length), Buf(4)
        _sync()
        ev.ctx.check(_raw(ev, ip.TERMS, length, d["lb"], d["ub"], v=d["v"], zl=d["zl"], zu=d["zu"], o1=s, o2=rb, out=r8))
        ev.ctx.check(_raw(ev, ip.RESID, length, d["lb"], d["ub"], t=d["t"], z=d["z"], negate=True, o1=r, out=r4))
        ev.ctx.check(_raw(ev, ip.STEP, length, d["lb"], d["ub"], v=d["v"], dv=d["dv"], zl=d["zl"], zu=d["zu"], o1=dl, o2=du, out=r4b))
        ev.sync()
        runs.append([x.fetch() for x in (s, rb, r8, r, r4, dl, du, r4b)])
    return runs


def _check_length(ev, b, length, what):
    first, second = _run_all(ev, b, length)
    want = (ip.emulate_terms(b["lb"], b["ub"], b["v"], b["zl"], b["zu"], MU) + ip.emulate_residual(b["lb"], b["ub"], b["t"], b["z"], True)
            + ip.emulate_step(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["zu"], MU, TAU))
    names = ("sigma", "rbar", "record of the terms", "r", "record of the residual", "dzl", "dzu", "record of the step")
    for name, got, again, ref in zip(names, first, second, want):
        assert sc.same_bits(got, again), f"{what} {name}: a second call gave other bits"
        if name == "record of the terms":
            _check_record(what, got, ref, b, length)
        else:
            _same(f"{what} {name}", got, ref)
    return first, want


@pytest.mark.parametrize("length", ip.LENGTHS + (ip.LENGTH_PAST_THE_PIECE_CAP,))
def test_the_kernels_match_the_emulator_bit_for_bit(step_ev, length):
    b = ip.boxed(length)
    _, want = _check_length(step_ev, b, length, f"clean, length {length}")
    assert want[2][ip.BAD] == 0.0 and want[4][ip.R_BAD] == 0.0 and want[7][ip.STEP_BAD] == 0.0


@pytest.mark.parametrize("length", (257, 2049))
def test_planted_defects_are_counted_and_left_out(step_ev, length):
    b = ip.dirty(length)
    got, want = _check_length(step_ev, b, length, f"dirty, length {length}")
    assert got[2][ip.BAD] == 4.0 and got[4][ip.R_BAD] == 1.0 and got[7][ip.STEP_BAD] == 5.0
    sigma, rbar, dzl, dzu = got[0], got[1], got[5], got[6]
    assert all(np.all(np.isfinite(a)) for a in (sigma, rbar, dzl, dzu, got[2], got[7]))
    assert sigma[0] == b["zu"][0] / (b["ub"][0] - b["v"][0]) and sigma[2] == b["zl"][2] / (b["v"][2] - b["lb"][2])
    assert dzl[0] == 0.0 and dzl[1] == 0.0 and dzu[2] == 0.0 and dzl[3] == 0.0 and dzl[4] == 0.0 and dzu[4] == 0.0 and np.isnan(got[3][4])


def test_vectors_without_a_side_give_the_identities(step_ev):
    for kinds in (ip.FREE, ip.FIXED):
        b = ip.boxed(2500, kinds=kinds)
        got, _ = _check_length(step_ev, b, 2500, f"kind {kinds}")
        assert not got[0].any() and not got[1].any() and not got[5].any() and not got[6].any()
        assert sc.same_bits(got[2], [0.0, 0.0, 0.0, np.inf, 0.0, 0.0, 0.0, np.inf]) and sc.same_bits(got[7], [1.0, 1.0, -1.0, 0.0])
        assert not got[3].any() if kinds == ip.FIXED else sc.same_bits(got[3], -(b["t"] - b["z"]))


def test_a_tie_reports_the_smallest_index_and_no_step_gives_one(step_ev):
    length = 3000
    b = ip.boxed(length, kinds=ip.BOTH)
    b["dv"] = np.abs(b["dv"]) * np.where(b["v"] - b["lb"] < b["ub"] - b["v"], 1.0, -1.0) * 1e-6
    for i in (5, 700, 2900):
        b["lb"][i], b["ub"][i], b["v"][i], b["dv"][i] = -1.0, 3.0, 0.0, -4.0
    got, _ = _check_length(step_ev, b, length, "tie")
    assert got[7][ip.ALPHA_PRI] == TAU / 4.0 and got[7][ip.ARG_PRI] == 5.0
    b["dv"] = np.zeros(length)
    got, _ = _check_length(step_ev, b, length, "dv = 0")
    assert got[7][ip.ALPHA_PRI] == 1.0 and got[7][ip.ARG_PRI] == -1.0 and sc.same_bits(got[5], MU / (b["v"] - b["lb"]) - b["zl"])


# ---------------------------------------------------------------- models
class IpmInputs:
    """Per model the boxed vectors and their emulated results, computed once; they owe nothing to the oracle."""

    def __init__(self, case):
        p = case.system.evaluator.plan
        rng = np.random.default_rng(11)
        self.box = {}
        for which, lo, hi, start in (("x", p.v_lb, p.v_ub, case.x), ("c", p.c_lb, p.c_ub, np.zeros(case.m))):
            lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
            count = len(lo)
            self.box[which] = dict(lb=lo, ub=hi, v=ip.inside(lo, hi, start), zl=rng.uniform(0.1, 1.0, count), zu=rng.uniform(0.1, 1.0, count),
                                   dv=rng.standard_normal(count))
        self.grad, self.lam, self.z = rng.standard_normal(case.n), rng.standard_normal(case.m), rng.standard_normal(case.n)
        self.fixed = np.asarray(p.v_lb) == np.asarray(p.v_ub)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def case(request):
    c = Case(*request.param)
    c.ipm = IpmInputs(c)
    yield c
    c.system.evaluator.close()


def _close3(a, b, what):
    err, bound = np.max(np.abs(a - b)), 3 * 1e-11 * max(1.0, np.max(np.abs(b)))
    print(f"{what}: err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, what


def test_the_host_forms_match_the_emulator_bit_for_bit(case):
    ev = case.system.evaluator
    for which, b in case.ipm.box.items():
        count = len(b["lb"])
        terms = ev.barrier_terms(b["v"], b["zl"], b["zu"], MU, which=which)
        sigma, rbar, rec = ip.emulate_terms(b["lb"], b["ub"], b["v"], b["zl"], b["zu"], MU)
        _same(f"{which} sigma", terms.sigma, sigma)
        _same(f"{which} rbar", terms.rbar, rbar)
        _check_record(f"{which} terms", terms.table, rec, b, count)
        assert terms.bad == 0.0 and terms.sides == rec[ip.SIDES]
        assert terms.mean_compl == (rec[ip.COMPL_SUM] / rec[ip.SIDES] if rec[ip.SIDES] else 0.0)
        step = ev.boundary_step(b["v"], b["dv"], b["zl"], b["zu"], MU, TAU, which=which)
        dzl, dzu, rec4 = ip.emulate_step(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["zu"], MU, TAU)
        _same(f"{which} dzl", step.dzl, dzl)
        _same(f"{which} dzu", step.dzu, dzu)
        _same(f"{which} step record", step.table, rec4)
        assert (step.alpha_primal, step.alpha_dual, step.bad) == (rec4[0], rec4[1], 0.0)
        assert step.blocking == (None if rec4[2] < 0 else int(rec4[2]))
        again = ev.barrier_terms(b["v"], b["zl"], b["zu"], MU, which=which)
        assert sc.same_bits(again.table, terms.table) and sc.same_bits(again.sigma, terms.sigma)
    with pytest.raises(ValueError):
        ev.barrier_terms(case.ipm.box["x"]["v"][:-1], case.ipm.box["x"]["zl"], case.ipm.box["x"]["zu"], MU)
    with pytest.raises(ValueError):
        ev.boundary_step(case.ipm.box["x"]["v"], case.ipm.box["x"]["dv"], case.ipm.box["x"]["zl"], case.ipm.box["x"]["zu"], MU, which="g")


def test_the_dual_residual_matches_the_oracle_and_the_products(case):
    lin = case.linearize()
    q = case.ipm
    box = q.box["x"]
    for z, negate in ((q.z, False), (q.z, True), (None, False), (None, True)):
        r, res = lin.dual_residual(q.grad, q.lam, z, negate)
        ref = case.J.T @ q.lam + q.grad - (0.0 if z is None else z)
        ref = np.where(q.fixed, 0.0, -ref if negate else ref)
        _close3(r, ref, f"dual residual z={z is not None} negate={negate}")
        assert res.bad == 0.0 and abs(res.inf - np.max(np.abs(ref))) <= 3e-11 * max(1.0, np.max(np.abs(ref)))
        assert abs(res.two_sq - ref @ ref) <= 1e-10 * max(1.0, ref @ ref)
        # the kernel on the operator's own result: the emulator, bit for bit
        t = lin.jtv(q.lam) + q.grad
        want_r, want_rec = ip.emulate_residual(box["lb"], box["ub"], t, z, negate)
        _same("r", r, want_r)
        _same("record", res.table, want_rec)
    r, _ = lin.dual_residual(q.grad, q.lam)
    _same("z = None", r, np.where(q.fixed, 0.0, lin.jtv(q.lam) + q.grad))


def _chain_host(case, iters):
    ev, q = case.system.evaluator, case.ipm
    b, n = q.box["x"], case.n
    lin = case.linearize()
    terms = ev.barrier_terms(b["v"], b["zl"], b["zu"], MU)
    r, res = lin.dual_residual(q.grad, q.lam, z=terms.rbar, negate=True)
    rhs = np.concatenate((r, q.lam))
    sol, info = lin.solve_kkt(rhs, s1=terms.sigma, s2=0.5, precond=None, tol=0.0, maxiter=iters, check_every=iters)
    step = ev.boundary_step(b["v"], sol[:n], b["zl"], b["zu"], MU, TAU)
    return terms.sigma, terms.rbar, terms.table, rhs, res.table, sol, step.dzl, step.dzu, step.table


def _chain_device(case, iters):
    ev, q = case.system.evaluator, case.ipm
    b, n, m = q.box["x"], case.n, case.m
    d = {k: _up(b[k]) for k in ("v", "zl", "zu")}
    dx, dlam, dgrad, ds2 = _up(case.x), _up(case.lam), _up(q.grad), _up(np.full(m, 0.5))
    dy = _up(q.lam)
    cj, ch = Buf(ev.csr_map("jac").nnz), Buf(ev.csr_map("hess").nnz)
    sigma, rbar, rec8, rec4, rec4b, dzl, dzu = Buf(n), Buf(n), Buf(8), Buf(4), Buf(4), Buf(n), Buf(n)
    rhs, sol = Buf(n + m, np.concatenate((np.full(n, np.nan), q.lam))), Buf(n + m)
    _sync()
    ev.jacobian_csr_dev(dx.data_ptr(), cj.ptr)
    ev.hessian_csr_dev(dx.data_ptr(), dlam.data_ptr(), case.sigma, ch.ptr)
    ev.ip_terms_dev(_ptr(d["v"]), _ptr(d["zl"]), _ptr(d["zu"]), MU, sigma.ptr, rbar.ptr, rec8.ptr)
    ev.dual_residual_dev(cj.ptr, _ptr(dgrad), _ptr(dy), rhs.ptr, rec4.ptr, d_z=rbar.ptr, negate=True)
    ev.minres_begin_dev(cj.ptr, rhs.ptr, sol.ptr, 0.0, d_hvals=ch.ptr, d_s1=sigma.ptr, d_s2=_ptr(ds2))
    ev.minres_advance_dev(iters)
    ev.ip_step_dev(_ptr(d["v"]), sol.ptr, _ptr(d["zl"]), _ptr(d["zu"]), MU, TAU, dzl.ptr, dzu.ptr, rec4b.ptr)
    ev.sync()                                   # the one wait; everything comes down behind it
    return tuple(x.fetch() for x in (sigma, rbar, rec8, rhs, rec4, sol, dzl, dzu, rec4b))


def test_the_chain_on_device_pointers_equals_the_chain_through_the_host_forms(case):
    """linearize -> barrier terms -> dual residual (b1 = -(J^T lam + grad - rbar)) -> 12 MINRES iterations on
    [[H + diag(sigma), J^T], [J, -0.5 I]] -> boundary step, once with every array resident and one download at the end, once
    through the host forms with a download and an upload between every stage: the same bits, so no stage depends on who owns
    the memory.  No tolerance is needed."""
    iters = 12
    host = _chain_host(case, iters)
    dev = _chain_device(case, iters)
    names = ("sigma", "rbar", "record of the terms", "b", "record of the residual", "solution", "dzl", "dzu", "record of the step")
    for name, h, g in zip(names, host, dev):
        _same(f"chain {name}", g, h)
    assert np.all(np.isfinite(host[5])) and host[8][ip.ALPHA_PRI] > 0.0


def test_refusals_with_their_codes_and_nothing_written(case):
    import pockit_amd.radau as radau

    ev, q = case.system.evaluator, case.ipm
    b, n = q.box["x"], case.n
    from pockit_amd import runtime

    as_dp = runtime.as_dp
    lib, h = ev.ctx.lib, ev.ctx.handle
    lin = case.linearize()
    lin.dual_residual(q.grad, q.lam)                    # (bounds and operators are up)
    o1, o2, rec = np.full(n, -3.0), np.full(n, -3.0), np.full(8, -3.0)
    args = (as_dp(b["v"]), as_dp(b["zl"]), as_dp(b["zu"]))
    assert lib.pk_ip_terms(h, 0, *args, -1.0, as_dp(o1), as_dp(o2), as_dp(rec)) == 134
    assert lib.pk_ip_terms(h, 2, *args, MU, as_dp(o1), as_dp(o2), as_dp(rec)) == 134
    assert lib.pk_ip_terms(h, 0, None, args[1], args[2], MU, as_dp(o1), as_dp(o2), as_dp(rec)) == 60
    assert lib.pk_ip_step(h, 0, args[0], as_dp(b["dv"]), args[1], args[2], MU, 0.0, as_dp(o1), as_dp(o2), as_dp(rec)) == 134
    assert lib.pk_ip_step(h, 0, args[0], as_dp(b["dv"]), args[1], args[2], -MU, TAU, as_dp(o1), as_dp(o2), as_dp(rec)) == 134
    assert lib.pk_ip_step(h, 0, args[0], None, args[1], args[2], MU, TAU, as_dp(o1), as_dp(o2), as_dp(rec)) == 60
    dev_o, dev_rec = Buf(n), Buf(8)
    dv = {k: _up(b[k]) for k in ("v", "dv", "zl", "zu")}
    _sync()
    assert lib.pk_ip_terms_dev(h, 0, None, _ptr(dv["zl"]), _ptr(dv["zu"]), MU, dev_o.ptr, dev_o.ptr, dev_rec.ptr, None) == 110
    assert lib.pk_ip_terms_dev(h, 0, _ptr(dv["v"]), _ptr(dv["zl"]), _ptr(dv["zu"]), -1.0, dev_o.ptr, dev_o.ptr, dev_rec.ptr, None) == 134
    assert lib.pk_ip_step_dev(h, 0, _ptr(dv["v"]), _ptr(dv["dv"]), _ptr(dv["zl"]), _ptr(dv["zu"]), MU, 0.0, dev_o.ptr, dev_o.ptr, dev_rec.ptr, None) == 134
    assert lib.pk_ip_step_dev(h, 0, _ptr(dv["v"]), _ptr(dv["dv"]), _ptr(dv["zl"]), _ptr(dv["zu"]), MU, TAU, dev_o.ptr, None, dev_rec.ptr, None) == 110
    assert lib.pk_dual_residual_dev(h, None, _ptr(dv["v"]), _ptr(dv["v"]), None, 0, dev_o.ptr, dev_rec.ptr, None) == 110
    assert _raw(ev, 3, n, dv["v"], dv["v"], v=dv["v"], zl=dv["zl"], zu=dv["zu"], o1=dev_o, o2=dev_o, out=dev_rec) == 134
    # a stale handle; then no linearization at all for the C entry point
    case.system.linearize(case.x)
    with pytest.raises(RuntimeError, match="stale"):
        lin.dual_residual(q.grad, q.lam)
    ev.jacobian_csr(case.x)
    assert lib.pk_dual_residual(h, as_dp(q.grad), as_dp(q.lam), None, 0, as_dp(o1), as_dp(rec)) == 118
    ev.sync()
    assert np.all(o1 == -3.0) and np.all(o2 == -3.0) and np.all(rec == -3.0)
    assert np.all(np.isnan(dev_o.fetch())) and np.all(np.isnan(dev_rec.fetch()))
    # no bounds: a context that never had them
    fresh = models.brachistochrone(radau, 3, 4)[0].evaluator
    try:
        k = fresh.plan.n
        v, w1, w2, out8 = np.zeros(k), np.full(k, -3.0), np.full(k, -3.0), np.full(8, -3.0)
        assert fresh.ctx.lib.pk_ip_terms(fresh.ctx.handle, 0, as_dp(v), as_dp(v), as_dp(v), MU, as_dp(w1), as_dp(w2), as_dp(out8)) == 123
        assert fresh.ctx.lib.pk_ip_step(fresh.ctx.handle, 0, as_dp(v), as_dp(v), as_dp(v), as_dp(v), MU, TAU, as_dp(w1), as_dp(w2), as_dp(out8)) == 123
        assert np.all(out8 == -3.0) and np.all(w1 == -3.0) and np.all(w2 == -3.0)
    finally:
        fresh.close()


def test_the_other_products_of_the_handle_return_the_bits_they_returned_before(case):
    ev, q = case.system.evaluator, case.ipm
    b = q.box["x"]
    rhs = np.random.default_rng(3).standard_normal(case.n + case.m)
    d = np.random.default_rng(4).standard_normal(case.n)
    scan = ev.merit_scan(case.x, d, [0.0, 0.5, 1.0])
    lin = case.linearize()               # (merit_scan gave the context another evaluation)
    others = lambda: (lin.solve_kkt(rhs, 2.0, 0.5, precond=None, tol=1e-8, maxiter=16)[0], lin.jv(case.v), lin.row_norms("J", "1"))  # noqa: E731
    before = others()
    ev.barrier_terms(b["v"], b["zl"], b["zu"], MU)
    lin.dual_residual(q.grad, q.lam, q.z)
    ev.boundary_step(b["v"], b["dv"], b["zl"], b["zu"], MU, TAU)
    for x, y in zip(before, others()):
        assert np.array_equal(x, y)
    assert np.array_equal(scan, ev.merit_scan(case.x, d, [0.0, 0.5, 1.0]))
