"""The CG solve of pockit_amd/csrc/pk_cg.cpp on the device.

Vector steps (pk_cg_step_dev on the context of brachistochrone(radau, 3, 4)): lengths 1, 255, 256, 257, 2 047, 2 048, 2 049,
524 289 (257 pieces: the second strided trip of the scalar step; 2 049 elementwise items: past the grid cap) and, for one case,
4 194 305 (2 049 pieces: past the cap for the piece kernels).  Full-mantissa data, outputs between sentinels in NaN-filled
tensors, bit equality with the emulator of tests/cg_cases.py for every vector and every record entry, the same bits from a second
call, and a frozen record (status 1, 2, 3) leaves x, r, z, p and the record untouched.

Synthetic systems (cg_cases.System on contexts A and B, both forms, both families): x and the record bit-equal to the emulator
through begin / advance / record on device pointers; the host form bit-equal to it and to the device-pointer form, for
check_every in {1, 3, 64}.

Models (the cases of tests/test_gpu_csr_operators.py) against SciPy on the ORACLE's matrices: ``kv`` in every combination of
form, H, d and shift at that file's rule scaled by the three products composed; the solves with the inputs and the bounds the
module constants state: status 1, ``|b - K x| <= 2 tol |b|`` and ``max|x - spsolve| <= 2 tol |b| / lambda``
(``e = K^-1 r``; the factor 2 covers the 1e-11 parity of the matrices times cond(K) < 1e2, three orders below tol)."""
import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

import cg_cases as cg
import sparse_cases as sc
from device_cases import Buf, SyntheticContext, _ptr, _same, _up, step_ev  # noqa: F401  (step_ev: a fixture)
from test_gpu_csr_operators import CASES, Case

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]

TOL, MAXITER = 1e-8, 64
INIT, CURVATURE, UPDATE, DIRECTION, SCALE, JACOBI = range(6)


def _step(ev, step, length, b=None, x0=None, minv=None, s=None, x=None, r=None, z=None, p=None, q=None, rec=None, tol=0.0):
    ev.ctx.check(ev.ctx.lib.pk_cg_step_dev(ev.ctx.handle, step, length, _ptr(b), _ptr(x0), _ptr(minv), _ptr(s), _ptr(x), _ptr(r), _ptr(z),
                                           _ptr(p), _ptr(q), _ptr(rec), tol, None))


def _check_steps(ev, L, full):
    """Every vector step at length L against the emulator; ``full`` False: init, curvature and update only."""
    import torch

    v = cg.step_vectors(L)
    tol = 1e-3
    d = {k: _up(a) for k, a in v.items() if k in ("b", "x0", "minv", "s")}
    torch.cuda.synchronize()            # torch's copies run on its own stream; the context uses its own
    # ---- init with x0 (q holds K x0 on entry), minv and s; twice
    want = cg.step_init(v["b"], v["x0"], v["kx"], v["minv"], v["s"], tol)
    runs = []
    for _ in range(2):
        out = {k: Buf(L) for k in "xrzp"}
        out["q"], out["rec"] = Buf(L, v["kx"]), Buf(8)
        torch.cuda.synchronize()
        _step(ev, INIT, L, b=d["b"], x0=d["x0"], minv=d["minv"], s=d["s"], tol=tol, **out)
        ev.sync()
        runs.append([out[k].fetch() for k in ("x", "r", "z", "p", "q", "rec")])
    for name, got, again, ref in zip(("x", "r", "z", "p", "q", "rec"), runs[0], runs[1], want):
        _same(f"init {name}", got, ref)
        assert sc.same_bits(got, again), f"init {name}: a second call gave other bits"
    assert want[5][cg.STATUS] == 0.0
    # ---- init without x0, minv and s
    out = {k: Buf(L) for k in "xrzpq"}
    out["rec"] = Buf(8)
    torch.cuda.synchronize()
    _step(ev, INIT, L, b=d["b"], tol=tol, **out)
    ev.sync()
    for name, ref in zip(("x", "r", "z", "p", "q", "rec"), cg.step_init(v["b"], None, None, None, None, tol)):
        _same(f"plain init {name}", out[name].fetch(), ref)
    # ---- curvature and update on a running record, with and without minv; the update twice
    rec0 = np.array([0.0, 3.0, 1.5, 1e-30, 0.75, 0.0, 0.0, 0.25])
    for minv_key in ("minv", None):
        minv = None if minv_key is None else v[minv_key]
        rec_a = cg.step_curvature(v["p"], v["q"], rec0)
        if rec_a[cg.STATUS] != 0.0:     # (p.q of random vectors may be negative: make it the curvature of -q)
            v["q"] = -v["q"]
            rec_a = cg.step_curvature(v["p"], v["q"], rec0)
        assert rec_a[cg.STATUS] == 0.0 and rec_a[cg.ALPHA] != 0.0
        want = cg.step_update(v["x"], v["r"], v["z"], v["p"], v["q"], minv, rec_a)
        runs = []
        for _ in range(2):
            bufs = {k: Buf(L, v[k]) for k in "xrzpq"}
            bufs["rec"] = Buf(8, rec0)
            torch.cuda.synchronize()
            _step(ev, CURVATURE, L, p=bufs["p"], q=bufs["q"], rec=bufs["rec"])
            ev.sync()
            _same("curvature rec", bufs["rec"].fetch(), rec_a)
            _step(ev, UPDATE, L, minv=None if minv is None else d["minv"], **bufs)
            ev.sync()
            runs.append([bufs[k].fetch() for k in ("x", "r", "z", "rec", "p", "q")])
        for name, got, again, ref in zip(("x", "r", "z", "rec", "p", "q"), runs[0], runs[1], want + (v["p"], v["q"])):
            _same(f"update {name} (minv {minv_key})", got, ref)
            assert sc.same_bits(got, again), f"update {name}: a second call gave other bits"
        if not full:
            return
        # ---- direction on the updated state
        x1, r1, z1, rec_b = want
        assert rec_b[cg.STATUS] == 0.0
        bufs = {"z": _up(z1), "p": Buf(L, v["p"]), "q": Buf(L), "rec": Buf(8, rec_b)}
        torch.cuda.synchronize()
        _step(ev, DIRECTION, L, s=d["s"], **bufs)
        ev.sync()
        p1, q1 = cg.step_direction(z1, v["p"], v["s"], rec_b)
        _same("direction p", bufs["p"].fetch(), p1)
        _same("direction q", bufs["q"].fetch(), q1)
        _same("direction rec", bufs["rec"].fetch(), rec_b)
    # ---- a negative and a NaN curvature
    for q_bad, status in ((-v["p"], 2.0), (np.where(np.arange(L) == L // 2, np.nan, v["q"]), 3.0)):
        rec = Buf(8, rec0)
        torch.cuda.synchronize()
        _step(ev, CURVATURE, L, p=_up(v["p"]), q=_up(q_bad), rec=rec)
        ev.sync()
        with np.errstate(invalid="ignore"):
            ref = cg.step_curvature(v["p"], q_bad, rec0)
        assert ref[cg.STATUS] == status
        assert np.array_equal(rec.fetch().view(np.uint64), ref.view(np.uint64))
    # ---- scale and the Jacobi reciprocal (zeros, an infinity and a NaN among g)
    q = Buf(L, v["q"])
    torch.cuda.synchronize()
    _step(ev, SCALE, L, s=d["s"], q=q)
    ev.sync()
    _same("scale", q.fetch(), v["s"] * v["q"])
    g = v["r"].copy()
    g[:: 7] = -v["s"][:: 7]              # g + s == 0
    g[1:: 11] = np.inf
    g[2:: 13] = np.nan
    for s_key in ("s", None):
        out = Buf(L)
        torch.cuda.synchronize()
        _step(ev, JACOBI, L, b=_up(g), s=None if s_key is None else d["s"], q=out)
        ev.sync()
        with np.errstate(invalid="ignore"):
            ref = cg.step_jacobi(g, None if s_key is None else v["s"])
        got = out.fetch()
        _same(f"jacobi (s {s_key})", got, ref)
        assert np.all(np.isfinite(got)) and np.all(got > 0)
    # ---- a frozen record leaves x, r, z, p and the record untouched
    for status in (1.0, 2.0, 3.0):
        frozen = rec0.copy()
        frozen[cg.STATUS], frozen[cg.ALPHA] = status, 0.5
        bufs = {k: Buf(L, v[k]) for k in "xrzpq"}
        bufs["rec"] = Buf(8, frozen)
        torch.cuda.synchronize()
        _step(ev, CURVATURE, L, p=bufs["p"], q=bufs["q"], rec=bufs["rec"])
        _step(ev, UPDATE, L, minv=d["minv"], **bufs)
        _step(ev, DIRECTION, L, s=d["s"], z=bufs["z"], p=bufs["p"], q=bufs["q"], rec=bufs["rec"])
        ev.sync()
        for k in "xrzp":
            _same(f"frozen {status} {k}", bufs[k].fetch(), v[k])
        _same(f"frozen {status} rec", bufs["rec"].fetch(), frozen)
        _same(f"frozen {status} q", bufs["q"].fetch(), v["s"] * v["p"])


@pytest.mark.parametrize("length", cg.STEP_LENGTHS)
def test_vector_steps_match_the_emulator_bit_for_bit(length, step_ev):
    _check_steps(step_ev, length, full=True)


def test_the_piece_kernels_past_the_grid_cap(step_ev):
    _check_steps(step_ev, cg.STEP_LENGTH_PAST_THE_PIECE_CAP, full=False)


def test_step_refusals(step_ev):
    ev = step_ev
    lib, h = ev.ctx.lib, ev.ctx.handle
    t = _up(np.ones(8))
    p = t.data_ptr()
    assert lib.pk_cg_step_dev(h, 6, 8, p, p, p, p, p, p, p, p, p, p, 0.0, None) == 134
    assert lib.pk_cg_step_dev(h, 0, -1, p, p, p, p, p, p, p, p, p, p, 0.0, None) == 134
    assert lib.pk_cg_step_dev(h, 0, 8, p, p, p, p, p, p, p, p, p, p, -1.0, None) == 134
    assert lib.pk_cg_step_dev(h, 0, 8, None, p, p, p, p, p, p, p, p, p, 0.0, None) == 110
    assert lib.pk_cg_advance_dev(h, 1, None) == 135
    assert lib.pk_cg_record(h, None) == 60


# ---------------------------------------------------------------- synthetic systems on contexts A and B
class Synthetic(SyntheticContext):
    def device_solve(self, sy, inp, minv, x0, chunk):
        """begin / advance / record on device pointers: (x, rec)"""
        import torch

        ev = self.ev
        lib, h = ev.ctx.lib, ev.ctx.handle
        jv, hv = _up(sy.jvals), _up(sy.hvals)
        d, s, b = _up(inp["d"]), _up(inp["s"]), _up(inp["b"])
        dm = None if minv is None else _up(minv)
        dx0 = None if x0 is None else _up(x0)
        x = Buf(len(inp["b"]))
        torch.cuda.synchronize()
        ev.ctx.check(lib.pk_cg_begin_dev(h, inp["form"], jv.data_ptr(), hv.data_ptr() if inp["with_h"] else None, d.data_ptr(), s.data_ptr(),
                                         _ptr(dm), b.data_ptr(), _ptr(dx0), x.ptr, TOL, None))
        rec = ev.cg_record()
        done = 0
        while rec[0] == 0.0 and done < 400:
            ev.cg_advance_dev(chunk)
            rec = ev.cg_record()
            done += chunk
        return x.fetch(), rec

    def host_solve(self, inp, precond, minv, x0, maxiter, check_every):
        from pockit_amd import runtime

        ev = self.ev
        opt = lambda a: None if a is None else runtime.as_dp(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
        x, rec = np.full(len(inp["b"]), np.nan), np.full(8, np.nan)
        ev.ctx.check(ev.ctx.lib.pk_solve_condensed(ev.ctx.handle, inp["form"], int(inp["with_h"]), opt(inp["d"]), opt(inp["s"]), precond,
                                                   opt(minv), opt(inp["b"]), opt(x0), TOL, maxiter, check_every, runtime.as_dp(x),
                                                   runtime.as_dp(rec)))
        return x, rec


@pytest.fixture(scope="module", params=["A", "B"])
def synthetic(request):
    s = Synthetic(request.param)
    yield s
    s.ev.close()


@pytest.mark.parametrize("family", ["pd", "indefinite"])
@pytest.mark.parametrize("form", [0, 1])
def test_synthetic_systems_match_the_emulator_bit_for_bit(synthetic, form, family):
    sy = synthetic.random
    inp = sy.inputs(form, family)
    pd = family == "pd"
    minv = sy.jacobi(form, inp["with_h"], inp["d"], inp["s"]) if pd else None
    x0 = inp["x0"] if pd else None
    want_x, want_rec = cg.emulate_solve(sy, form, inp["with_h"], inp["d"], inp["s"], minv, inp["b"], x0, TOL, 400)
    assert want_rec[cg.STATUS] == (1.0 if pd else 2.0)
    for chunk in (1, 5):
        x, rec = synthetic.device_solve(sy, inp, minv, x0, chunk)
        print(f"{sy.ctx} form {form} {family}: status {rec[0]}, {int(rec[1])} iterations, chunks of {chunk}")
        _same("record", rec, want_rec)
        _same("x", x, want_x)


@pytest.mark.parametrize("family", ["pd", "indefinite"])
@pytest.mark.parametrize("form", [0, 1])
def test_the_host_form_matches_the_device_pointer_form_and_the_emulator(synthetic, form, family):
    """On the values pk_linearize left (the model's own), under the synthetic structures: the Jacobi build on the device, the
    uploads, the chunks of check_every."""
    sy = synthetic.real
    inp = sy.inputs(form, family)
    pd = family == "pd"
    minv = sy.jacobi(form, inp["with_h"], inp["d"], inp["s"]) if pd else None
    x0 = inp["x0"] if pd else None
    want_x, want_rec = cg.emulate_solve(sy, form, inp["with_h"], inp["d"], inp["s"], minv, inp["b"], x0, TOL, 400)
    dev_x, dev_rec = synthetic.device_solve(sy, inp, minv, x0, 8)
    _same("device-pointer record", dev_rec, want_rec)
    _same("device-pointer x", dev_x, want_x)
    for ce in (1, 3, 64):
        x, rec = synthetic.host_solve(inp, 1 if pd else 0, None, x0, 400, ce)
        _same(f"host record, check_every {ce}", rec, want_rec)
        _same(f"host x, check_every {ce}", x, want_x)
    if pd:
        x, rec = synthetic.host_solve(inp, 2, minv, x0, 400, 8)       # the caller's minv: the array the Jacobi build gives
        _same("host x, precond 2", x, want_x)
        k = int(want_rec[cg.ITERS]) - 1
        assert k >= 1
        x, rec = synthetic.host_solve(inp, 1, None, x0, k, 3)           # exhaustion: status 4 in the host copy
        ref_x, ref_rec = cg.emulate_solve(sy, form, inp["with_h"], inp["d"], inp["s"], minv, inp["b"], x0, TOL, k, check_every=3)
        assert rec[0] == 4.0 and rec[1] == k
        _same("exhausted record", rec, ref_rec)
        _same("exhausted x", x, ref_x)


def test_refusals_enqueue_nothing(synthetic):
    from pockit_amd import runtime

    ev, sy = synthetic.ev, synthetic.random
    lib, h = ev.ctx.lib, ev.ctx.handle
    inp = sy.inputs(0, "pd")
    x, rec = np.full(sy.n, -3.0), np.full(8, -3.0)
    dp = lambda a: runtime.as_dp(a)  # noqa: E731
    b, d, s = (np.ascontiguousarray(inp[k]) for k in ("b", "d", "s"))
    call = lambda form, with_h, precond, tol, maxiter, ce: lib.pk_solve_condensed(  # noqa: E731
        h, form, with_h, dp(d), dp(s), precond, None, dp(b), None, tol, maxiter, ce, dp(x), dp(rec))
    assert call(2, 0, 0, TOL, 8, 8) == 133 and call(-1, 0, 0, TOL, 8, 8) == 133 and call(1, 1, 0, TOL, 8, 8) == 133
    assert call(0, 1, 0, -1.0, 8, 8) == 134 and call(0, 1, 0, float("nan"), 8, 8) == 134 and call(0, 1, 0, float("inf"), 8, 8) == 134
    assert call(0, 1, 0, TOL, 0, 8) == 134 and call(0, 1, 0, TOL, 8, 0) == 134 and call(0, 1, 3, TOL, 8, 8) == 134
    assert call(0, 1, 2, TOL, 8, 8) == 60                                # precond 2 without minv
    assert lib.pk_cg_advance_dev(h, 0, None) == 134
    assert lib.pk_condensed_apply_dev(h, 0, None, None, None, None, None, None, None) == 110
    ev.sync()
    assert np.all(x == -3.0) and np.all(rec == -3.0)


# ---------------------------------------------------------------- models against SciPy on the oracle's matrices
def _pcg(K, b, minv, tol, maxiter, x0=None):
    """The reference PCG in NumPy: (x, iterations, status, last curvature)"""
    x = np.zeros(len(b)) if x0 is None else x0.copy()
    r = b - K @ x
    z = minv * r
    p, rz, thr = z.copy(), r @ z, tol * tol * (b @ b)
    for k in range(maxiter):
        q = K @ p
        pq = p @ q
        if not pq > 0:
            return x, k, 2, pq
        alpha = rz / pq
        x, r = x + alpha * p, r - alpha * q
        if r @ r <= thr:
            return x, k + 1, 1, pq
        z = minv * r
        rz, rz0 = r @ z, rz
        p = z + (rz / rz0) * p
    return x, maxiter, 4, pq


class Solves:
    """Per model the inputs of the primal and the dual solve and their references, computed once."""

    def __init__(self, case):
        J, H = case.J, case.H
        n, m = case.n, case.m
        self.rho = max(1.0, float(abs(H).sum(axis=1).max()))
        row2 = np.asarray(J.multiply(J).sum(axis=1)).reshape(-1)
        col2 = np.asarray(J.multiply(J).sum(axis=0)).reshape(-1)
        inv = lambda a: np.where(a > 0, 1.0 / np.where(a > 0, a, 1.0), 0.0)  # noqa: E731
        rng = np.random.default_rng(11)
        eye = scipy.sparse.eye_array
        self.primal = dict(form="primal", d=inv(row2), shift=2.0 * self.rho, lam=self.rho, b=rng.standard_normal(n))
        self.primal["K"] = scipy.sparse.csc_array(H + J.T @ scipy.sparse.diags_array(self.primal["d"]) @ J + 2.0 * self.rho * eye(n))
        self.dual = dict(form="dual", d=inv(col2), shift=0.5, lam=0.5, b=rng.standard_normal(m))
        self.dual["K"] = scipy.sparse.csc_array(J @ scipy.sparse.diags_array(self.dual["d"]) @ J.T + 0.5 * eye(m))
        for side in (self.primal, self.dual):
            K = side["K"]      # (a free final time makes J D J^T dense: the same direct solve, by LAPACK instead of SuperLU)
            dense = K.nnz > 0.2 * K.shape[0] * K.shape[1]
            side["ref"] = np.linalg.solve(K.toarray(), side["b"]) if dense else scipy.sparse.linalg.spsolve(K, side["b"])
            side["pcg"] = _pcg(side["K"], side["b"], 1.0 / np.abs(side["K"].diagonal()), TOL, MAXITER)
        self.indefinite = scipy.sparse.csr_array(H + 1.0e-3 * eye(n))


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def case(request):
    c = Case(*request.param)
    c.solves = Solves(c)
    yield c
    c.system.evaluator.close()


def _close3(a, b, what):
    err, bound = np.max(np.abs(a - b)), 3 * 1e-11 * max(1.0, np.max(np.abs(b)))
    print(f"{what}: err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, what


def test_kv_matches_the_oracle_in_every_combination(case):
    lin = case.linearize()
    rng = np.random.default_rng(13)
    n, m = case.n, case.m
    J, H = case.J, case.H
    for form, size, other in (("primal", n, m), ("dual", m, n)):
        v = rng.standard_normal(size)
        d_vec, s_vec = rng.uniform(0.5, 2.0, other), rng.uniform(0.5, 2.0, size)
        for with_h in ((True, False, None) if form == "primal" else (False,)):
            for d in (None, d_vec):
                for shift in (None, 0.75, s_vec):
                    t = (J @ v) if form == "primal" else (J.T @ v)
                    if d is not None:
                        t = d * t
                    ref = (J.T @ t) if form == "primal" else (J @ t)
                    if with_h or with_h is None:
                        ref = ref + H @ v
                    if shift is not None:
                        ref = ref + shift * v
                    got = lin.kv(v, d, shift, form=form, with_h=with_h)
                    _close3(got, ref, f"kv {form} H={with_h} d={'v' if d is not None else None} shift={type(shift).__name__}")
    op = lin.condensed_operator(d=None, shift=0.75, form="dual")
    v = rng.standard_normal(m)
    assert np.array_equal(op @ v, lin.kv(v, None, 0.75, form="dual"))


@pytest.mark.parametrize("side", ["primal", "dual"])
def test_the_solve_meets_the_residual_and_error_bounds(case, side):
    lin = case.linearize()
    inp = getattr(case.solves, side)
    b, K = inp["b"], inp["K"]
    x, info = lin.solve_condensed(b, inp["d"], inp["shift"], form=inp["form"], tol=TOL, maxiter=MAXITER)
    nb = np.linalg.norm(b)
    res, err = np.linalg.norm(b - K @ x), np.max(np.abs(x - inp["ref"]))
    print(f"{side}: device {info.iterations} iterations, reference {inp['pcg'][1]}; residual {res:.3e} (bound {2 * TOL * nb:.3e}), "
          f"error {err:.3e} (bound {2 * TOL * nb / inp['lam']:.3e}); rel_residual {info.rel_residual:.3e}")
    assert info.status == "converged"
    assert res <= 2 * TOL * nb
    assert err <= 2 * TOL * nb / inp["lam"]
    assert info.rel_residual <= TOL and info.curvature > 0
    with pytest.raises(AttributeError):
        info.status = "x"
    # the preconditioner as an array is the Jacobi build, bit for bit; none at all converges to the same solution
    minv = lin.jacobi(inp["d"], inp["shift"], form=inp["form"])
    x2, info2 = lin.solve_condensed(b, inp["d"], inp["shift"], form=inp["form"], precond=minv, tol=TOL, maxiter=MAXITER)
    assert np.array_equal(x, x2) and np.array_equal(info.record, info2.record)
    x3, info3 = lin.solve_condensed(b, inp["d"], inp["shift"], form=inp["form"], precond=None, tol=TOL, maxiter=4 * MAXITER)
    print(f"{side}: {info3.iterations} iterations without a preconditioner")
    assert info3.status == "converged" and np.max(np.abs(x3 - inp["ref"])) <= 2 * TOL * nb / inp["lam"]
    # x0 given, against x0 = None applied to b - K x0: the same solution within the bound
    x0 = np.random.default_rng(17).standard_normal(len(b))
    x4, info4 = lin.solve_condensed(b, inp["d"], inp["shift"], form=inp["form"], x0=x0, tol=TOL, maxiter=MAXITER)
    b5 = b - K @ x0
    x5, info5 = lin.solve_condensed(b5, inp["d"], inp["shift"], form=inp["form"], tol=TOL, maxiter=MAXITER)
    assert info4.status == "converged" and info5.status == "converged"
    assert np.max(np.abs(x4 - inp["ref"])) <= 2 * TOL * nb / inp["lam"]
    assert np.max(np.abs(x0 + x5 - inp["ref"])) <= 2 * TOL * np.linalg.norm(b5) / inp["lam"]


def test_the_indefinite_system_stops_on_non_positive_curvature(case):
    lin = case.linearize()
    n, m = case.n, case.m
    b = np.random.default_rng(11).standard_normal(n)
    K = case.solves.indefinite
    _, k_ref, status_ref, _ = _pcg(K, b, 1.0 / np.abs(K.diagonal()), TOL, MAXITER)
    assert status_ref == 2 and k_ref <= 3
    x, info = lin.solve_condensed(b, np.zeros(m), 1.0e-3, form="primal", tol=TOL, maxiter=MAXITER)
    print(f"indefinite: device stops after {info.iterations} iterations with curvature {info.curvature:.3e}; reference after {k_ref}")
    assert info.status == "non_positive_curvature" and info.curvature <= 0 and np.all(np.isfinite(x))
    k = info.iterations
    if k == 0:
        assert np.array_equal(x, np.zeros(n))
    else:
        xk, infok = lin.solve_condensed(b, np.zeros(m), 1.0e-3, form="primal", tol=TOL, maxiter=k)
        assert infok.status == "maxiter" and np.array_equal(x, xk)


def test_stale_handles_missing_hessians_and_the_other_products(case):
    lin = case.linearize()
    before = (lin.jv(case.v), lin.jtv(case.y), lin.hv(case.v), lin.row_norms("J", "1"), lin.jtdj_diag(np.ones(case.m)))
    inp = case.solves.primal
    lin.solve_condensed(inp["b"], inp["d"], inp["shift"], tol=TOL, maxiter=MAXITER)
    lin.solve_condensed(case.solves.dual["b"], case.solves.dual["d"], 0.5, form="dual", tol=TOL, maxiter=MAXITER)
    after = (lin.jv(case.v), lin.jtv(case.y), lin.hv(case.v), lin.row_norms("J", "1"), lin.jtdj_diag(np.ones(case.m)))
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        lin.kv(case.y, form="dual", with_h=True)
    no_h = case.system.linearize(case.x)
    with pytest.raises(RuntimeError, match="stale"):
        lin.kv(case.v)
    with pytest.raises(RuntimeError, match="stale"):
        lin.solve_condensed(inp["b"])
    with pytest.raises(RuntimeError, match="no Hessian"):
        no_h.kv(case.v, with_h=True)
    with pytest.raises(RuntimeError, match="no Hessian"):
        no_h.solve_condensed(inp["b"], with_h=True)
    x, info = no_h.solve_condensed(inp["b"], inp["d"], 1.0, tol=TOL, maxiter=MAXITER)      # Gauss-Newton: J^T D J + I
    K = scipy.sparse.csc_array(case.J.T @ scipy.sparse.diags_array(inp["d"]) @ case.J + scipy.sparse.eye_array(case.n))
    assert info.status == "converged" and np.linalg.norm(inp["b"] - K @ x) <= 2 * TOL * np.linalg.norm(inp["b"])
