"""The MINRES solve of pockit_amd/csrc/pk_minres.cpp on the device.

Vector steps (pk_minres_step_dev on the context of brachistochrone(radau, 3, 4)): lengths 1, 255, 256, 257, 2 047, 2 048, 2 049,
524 289 (257 pieces: the second strided trip of the scalar step; 2 049 elementwise items: past the grid cap) and, for begin and
the update, 4 194 305 (2 049 pieces: past the cap for the piece kernels); the split index at 0, 1, 255, 256, 257, N - 1, N where
they fit the length.  Full-mantissa data, outputs between sentinels in NaN-filled tensors, bit equality with the emulator of
tests/minres_cases.py for every vector and every record entry, the same bits from a second call.  The scalar steps on their own
(length 1: the sums are single products) on 64 full-mantissa records: this is what holds sqrt and / to the correctly rounded
ones on the hardware.  Scalar edge cases, and a frozen record (status 1, 2, 3) leaves x, r1, r2, y, w, w2 and slots 0 ... 14.

Synthetic systems (minres_cases.Kkt on contexts A and B): x and the record bit-equal to the emulator through begin / advance /
record on device pointers in chunks of 1 and 5; the host form bit-equal to it and to the device-pointer form, for check_every in
{1, 3, 64}; exhaustion; the device-built preconditioner bit-equal to ``Linearization.kkt_precond``'s arithmetic.

Models (the cases of tests/test_gpu_csr_operators.py) against SciPy on the ORACLE's matrices: ``kkt_v`` in every combination of
H, s1 and s2 at that file's rule scaled by the three products composed; the solve of K = [[H + 2 rho I, J^T], [J, -0.5 I]]
(quasi-definite: no eigenvalue in (-0.5, rho)) with status 1 within the reference count plus 10 %,
``|b - K x|_M <= 2 tol |b|_M`` and ``max|x - x*| <= 2 tol |b|_M / sqrt(min minv) / 0.5`` (``e = K^-1 r``,
``|r|_2 <= |r|_M / sqrt(min minv)``; the factor 2 is the one tests/test_minres_cases_cpu.py holds on the emulator)."""
import math

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

import cg_cases as cg
import minres_cases as mr
import sparse_cases as sc
from device_cases import Buf, SyntheticContext, _ptr, _same, _sync, _up, step_ev  # noqa: F401  (step_ev: a fixture)
from test_gpu_csr_operators import CASES, Case

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]

TOL = 1e-8
VECTORS = ("x", "r1", "r2", "y", "v", "w", "w2", "q")


def _step(ev, step, length, split=0, b=None, x0=None, minv=None, s1=None, s2=None, x=None, r1=None, r2=None, y=None, v=None, w=None, w2=None,
          q=None, rec=None, tol=0.0):
    ev.ctx.check(ev.ctx.lib.pk_minres_step_dev(ev.ctx.handle, step, length, split, _ptr(b), _ptr(x0), _ptr(minv), _ptr(s1), _ptr(s2), _ptr(x),
                                               _ptr(r1), _ptr(r2), _ptr(y), _ptr(v), _ptr(w), _ptr(w2), _ptr(q), _ptr(rec), tol, None))


def _running(length, iterations=3.0):
    return mr.running_record(np.random.default_rng(100 + length), iterations)


def _check_piece_steps(ev, L):
    """begin, alfa and the update at length L against the emulator, each twice."""
    v = mr.step_vectors(L)
    tol = 1e-3
    d = {k: _up(v[k]) for k in ("b", "x0", "minv")}
    # ---- begin with x0 (q holds K x0 on entry) and minv; then without either
    for full in (True, False):
        want = mr.step_init(v["b"], v["x0"] if full else None, v["kx"], v["minv"] if full else None, tol)
        runs = []
        for _ in range(2):
            out = {k: Buf(L) for k in ("x", "r1", "r2", "y", "w", "w2")}
            out["q"], out["rec"] = Buf(L, v["kx"]), Buf(16)
            _sync()
            _step(ev, mr.INIT, L, L // 2, b=d["b"], x0=d["x0"] if full else None, minv=d["minv"] if full else None, tol=tol, **out)
            ev.sync()
            runs.append([out[k].fetch() for k in ("x", "r1", "r2", "y", "w", "w2", "rec")])
        for name, got, again, ref in zip(("x", "r1", "r2", "y", "w", "w2", "rec"), runs[0], runs[1], want):
            _same(f"begin {name} (x0, minv {full})", got, ref)
            assert sc.same_bits(got, again), f"begin {name}: a second call gave other bits"
        assert want[6][mr.STATUS] == 0.0
    # ---- alfa and the update on a running record, with and without minv, on the first iteration and past it
    for minv_key, iterations in (("minv", 3.0), (None, 3.0), ("minv", 0.0)):
        minv = None if minv_key is None else v[minv_key]
        rec0 = _running(L, iterations)
        rec0[mr.FRESH] = 1.0
        rec_a = mr.step_alfa(v["v"], v["q"], rec0)
        assert rec_a[mr.STATUS] == 0.0 and rec_a[mr.FRESH] == 0.0
        want = mr.step_update(v["r1"], v["r2"], v["y"], v["q"], minv, rec_a)
        runs = []
        for _ in range(2):
            bufs = {k: Buf(L, v[k]) for k in ("r1", "r2", "y", "v", "q")}
            bufs["rec"] = Buf(16, rec0)
            _sync()
            _step(ev, mr.ALFA_STEP, L, v=bufs["v"], q=bufs["q"], rec=bufs["rec"])
            ev.sync()
            _same("alfa rec", bufs["rec"].fetch(), rec_a)
            _step(ev, mr.UPDATE, L, minv=None if minv is None else d["minv"], r1=bufs["r1"], r2=bufs["r2"], y=bufs["y"], q=bufs["q"], rec=bufs["rec"])
            ev.sync()
            runs.append([bufs[k].fetch() for k in ("r1", "r2", "y", "rec", "v", "q")])
        for name, got, again, ref in zip(("r1", "r2", "y", "rec", "v", "q"), runs[0], runs[1], want + (v["v"], v["q"])):
            _same(f"update {name} (minv {minv_key}, iterations {iterations})", got, ref)
            assert sc.same_bits(got, again), f"update {name}: a second call gave other bits"
        assert want[3][mr.ITERS] == iterations + 1 and want[3][mr.FRESH] == 1.0
    return v, d


def _check_steps(ev, L):
    """Every vector step at length L against the emulator."""
    v, d = _check_piece_steps(ev, L)
    d.update({k: _up(v[k]) for k in ("s1", "s2")})
    # ---- the Lanczos vector and the diagonal blocks at every split index, running and frozen, s1 / s2 present or not
    for split in mr.split_points(L):
        for s1_key, s2_key in (("s1", "s2"), ("s1", None), (None, "s2")):
            for status in (0.0, 1.0) if s1_key and s2_key else (0.0,):
                rec0 = _running(L)
                rec0[mr.STATUS] = status
                bufs = {"y": Buf(L, v["y"]), "v": Buf(L, v["v"]), "q": Buf(L), "rec": Buf(16, rec0)}
                _sync()
                _step(ev, mr.LANCZOS, L, split, s1=d.get(s1_key), s2=d.get(s2_key), **bufs)
                ev.sync()
                want_v, want_q = mr.step_lanczos(v["y"], v["v"], v.get(s1_key), v.get(s2_key), split, rec0)
                what = f"Lanczos split {split} s1 {s1_key} s2 {s2_key} status {status}"
                _same(what + " v", bufs["v"].fetch(), want_v)
                _same(what + " q", bufs["q"].fetch(), want_q)
                _same(what + " rec", bufs["rec"].fetch(), rec0)
            out = Buf(L)
            _sync()
            _step(ev, mr.DIAG, L, split, b=_up(v["v"]), s1=d.get(s1_key), s2=d.get(s2_key), q=out)
            ev.sync()
            _same(f"diagonal blocks split {split}", out.fetch(), mr.diag_terms(v["v"], v.get(s1_key), v.get(s2_key), split))
    # ---- the solution update: exactly when fresh == 1, whatever the status; twice
    for fresh in (1.0, 0.0):
        for status in (0.0, 1.0):
            rec0 = _running(L)
            rec0[mr.STATUS], rec0[mr.FRESH] = status, fresh
            want = mr.step_solution(v["x"], v["v"], v["w"], v["w2"], rec0)
            runs = []
            for _ in range(2):
                bufs = {k: Buf(L, v[k]) for k in ("x", "v", "w", "w2")}
                bufs["rec"] = Buf(16, rec0)
                _sync()
                _step(ev, mr.SOLUTION, L, **bufs)
                ev.sync()
                runs.append([bufs[k].fetch() for k in ("x", "w", "w2", "v", "rec")])
            for name, got, again, ref in zip(("x", "w", "w2", "v", "rec"), runs[0], runs[1], want + (v["v"], rec0)):
                _same(f"solution update {name} (fresh {fresh}, status {status})", got, ref)
                assert sc.same_bits(got, again)
            assert sc.same_bits(want[0], v["x"]) == (fresh == 0.0)
    # ---- the reciprocal (zeros, an infinity and a NaN among g)
    g = v["r1"].copy()
    g[:: 7] = -v["s1"][:: 7]              # g + s == 0
    g[1:: 11] = np.inf
    g[2:: 13] = np.nan
    for g_key, s_key in (("g", "s1"), ("g", None), (None, "s1")):
        out = Buf(L)
        _sync()
        _step(ev, mr.RECIP, L, b=None if g_key is None else _up(g), s1=d.get(s_key), q=out)
        ev.sync()
        with np.errstate(invalid="ignore"):
            ref = mr.step_recip(None if g_key is None else g, v.get(s_key))
        got = out.fetch()
        _same(f"reciprocal (g {g_key}, s {s_key})", got, ref)
        assert np.all(np.isfinite(got)) and np.all(got > 0)
    # ---- a frozen record: a whole iteration leaves x, r1, r2, y, w, w2 and the record's slots 0 ... 14 untouched
    for status in (1.0, 2.0, 3.0):
        for fresh in (0.0, 1.0):          # (fresh 1: the stopping iteration's own scalar step A has yet to clear it)
            frozen = _running(L)
            frozen[mr.STATUS], frozen[mr.FRESH] = status, fresh
            bufs = {k: Buf(L, v[k]) for k in VECTORS}
            bufs["rec"] = Buf(16, frozen)
            _sync()
            _step(ev, mr.LANCZOS, L, L // 2, s1=d["s1"], s2=d["s2"], y=bufs["y"], v=bufs["v"], q=bufs["q"], rec=bufs["rec"])
            _step(ev, mr.ALFA_STEP, L, v=bufs["v"], q=bufs["q"], rec=bufs["rec"])
            _step(ev, mr.UPDATE, L, minv=d["minv"], r1=bufs["r1"], r2=bufs["r2"], y=bufs["y"], q=bufs["q"], rec=bufs["rec"])
            _step(ev, mr.SOLUTION, L, x=bufs["x"], v=bufs["v"], w=bufs["w"], w2=bufs["w2"], rec=bufs["rec"])
            ev.sync()
            for k in ("x", "r1", "r2", "y", "w", "w2", "v"):
                _same(f"frozen {status} {k}", bufs[k].fetch(), v[k])
            got = bufs["rec"].fetch()
            _same(f"frozen {status} rec", got[:15], frozen[:15])
            assert got[mr.FRESH] == 0.0


@pytest.mark.parametrize("length", cg.STEP_LENGTHS)
def test_vector_steps_match_the_emulator_bit_for_bit(length, step_ev):
    _check_steps(step_ev, length)


def test_the_piece_kernels_past_the_grid_cap(step_ev):
    _check_piece_steps(step_ev, cg.STEP_LENGTH_PAST_THE_PIECE_CAP)


def _scalar_steps(ev, rec0, v, q, r1, r2, minv=None):
    """Scalar steps A and B alone: vectors of length 1, so alfa = v q and bsq = t y are single products."""
    one = lambda a: np.array([a], dtype=np.float64)  # noqa: E731
    bufs = {"v": Buf(1, one(v)), "q": Buf(1, one(q)), "r1": Buf(1, one(r1)), "r2": Buf(1, one(r2)), "y": Buf(1, one(0.0)), "rec": Buf(16, rec0)}
    dm = None if minv is None else _up(one(minv))
    _sync()
    _step(ev, mr.ALFA_STEP, 1, v=bufs["v"], q=bufs["q"], rec=bufs["rec"])
    _step(ev, mr.UPDATE, 1, minv=dm, r1=bufs["r1"], r2=bufs["r2"], y=bufs["y"], q=bufs["q"], rec=bufs["rec"])
    ev.sync()
    with np.errstate(all="ignore"):
        rec_a = mr.step_alfa(one(v), one(q), rec0)
        want = mr.step_update(one(r1), one(r2), one(0.0), one(q), None if minv is None else one(minv), rec_a)
    return bufs["rec"].fetch(), want[3], bufs["r2"].fetch(), want[1]


def test_the_scalar_steps_round_sqrt_and_division_correctly(step_ev):
    """64 full-mantissa records through scalar steps A and B: beta = sqrt(bsq), gamma = sqrt(gbar^2 + beta^2), cs, sn and the
    update's two quotients, bit for bit against NumPy's correctly rounded sqrt and /."""
    rng = np.random.default_rng(64)
    moved = 0
    for k in range(64):
        rec0 = mr.running_record(rng, float(k % 3))
        scale = 2.0 ** int(rng.integers(-30, 31))
        rec0[mr.BETA] *= scale                      # quotients and roots over a range of exponents
        v, q, r1, r2 = rng.uniform(-2, 2, 4)
        got, want, got_t, want_t = _scalar_steps(step_ev, rec0, v, q * scale, r1, r2 * scale)
        _same(f"record {k}", got, want)
        _same(f"t of record {k}", got_t, want_t)
        assert want[mr.STATUS] == 0.0 and want[mr.ITERS] == rec0[mr.ITERS] + 1 and want[mr.FRESH] == 1.0
        moved += int(want[mr.GAMMA] != np.hypot(want[mr.BETA], rec0[mr.SN] * rec0[mr.DBAR] - rec0[mr.CS] * want[mr.ALFA]))
    assert moved > 0                                # (the rounded products differ from hypot somewhere: the comparison is sharp)


def test_scalar_edge_cases(step_ev):
    rng = np.random.default_rng(65)
    rec0 = mr.running_record(rng)
    # a negative bsq (a preconditioner that is not positive), a NaN bsq (alfa finite), a non-finite alfa
    for (q, r2, minv), status in (((1.5, -0.25, -1.0), 2.0), ((1.5, np.nan, None), 3.0), ((np.inf, -0.25, None), 3.0)):
        got, want, _, _ = _scalar_steps(step_ev, rec0, 0.75, q, 0.5, r2, minv)
        assert want[mr.STATUS] == status and np.isfinite(want[mr.ALFA]) == np.isfinite(q)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
        assert got[mr.ITERS] == rec0[mr.ITERS] and got[mr.FRESH] == 0.0
    # gamma == 0: bsq = 0 and gbar = 0
    zero = rec0.copy()
    zero[mr.DBAR] = 0.0
    got, want, _, _ = _scalar_steps(step_ev, zero, 0.75, 0.0, 0.0, 0.0)
    assert want[mr.STATUS] == 3.0 and want[mr.GAMMA] == 0.0 and want[mr.ALFA] == 0.0
    _same("gamma == 0", got, want)
    # a converging step: phibar falls below the threshold, fresh stays 1 for the solution update
    conv = rec0.copy()
    conv[mr.THR] = 10.0
    got, want, _, _ = _scalar_steps(step_ev, conv, 0.75, 1.25, 0.5, -0.25)
    assert want[mr.STATUS] == 1.0 and want[mr.FRESH] == 1.0
    _same("converging", got, want)


def test_step_refusals(step_ev):
    ev = step_ev
    lib, h = ev.ctx.lib, ev.ctx.handle
    t = _up(np.ones(16))
    p = t.data_ptr()
    full = (p,) * 14
    assert lib.pk_minres_step_dev(h, 7, 8, 4, *full, 0.0, None) == 134
    assert lib.pk_minres_step_dev(h, 0, -1, 0, *full, 0.0, None) == 134
    assert lib.pk_minres_step_dev(h, 0, 8, 9, *full, 0.0, None) == 134
    assert lib.pk_minres_step_dev(h, 0, 8, 4, *full, -1.0, None) == 134
    assert lib.pk_minres_step_dev(h, 0, 8, 4, None, *full[1:], 0.0, None) == 110
    assert lib.pk_minres_advance_dev(h, 1, None) == 135
    assert lib.pk_minres_record(h, None) == 60
    ev.sync()
    assert np.all(t.cpu().numpy() == 1.0)


# ---------------------------------------------------------------- synthetic systems on contexts A and B
class Synthetic(SyntheticContext):
    """... and the KKT systems of minres_cases over the two systems."""

    def __init__(self, ctx):
        super().__init__(ctx)
        self.random, self.real = mr.Kkt(self.random), mr.Kkt(self.real)

    def device_solve(self, kk, inp, minv, x0, chunk, limit=400):
        """begin / advance / record on device pointers: (x, rec)"""
        ev = self.ev
        jv, hv = _up(kk.sy.jvals), _up(kk.sy.hvals)
        s1, b = _up(inp["s1"]), _up(inp["b"])
        s2 = None if inp["s2"] is None else _up(inp["s2"])
        dm = None if minv is None else _up(minv)
        dx0 = None if x0 is None else _up(x0)
        x = Buf(kk.N)
        _sync()
        # (the library directly: Evaluator.minres_begin_dev would first upload the model's own operators over the synthetic ones)
        ev.ctx.check(ev.ctx.lib.pk_minres_begin_dev(ev.ctx.handle, jv.data_ptr(), hv.data_ptr() if inp["with_h"] else None, s1.data_ptr(),
                                                    _ptr(s2), _ptr(dm), b.data_ptr(), _ptr(dx0), x.ptr, TOL, None))
        rec = ev.minres_record()
        done = 0
        while rec[0] == 0.0 and done < limit:
            ev.minres_advance_dev(chunk)
            rec = ev.minres_record()
            done += chunk
        return x.fetch(), rec

    def host_solve(self, inp, precond, minv, x0, maxiter, check_every):
        from pockit_amd import runtime

        ev = self.ev
        opt = lambda a: None if a is None else runtime.as_dp(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
        x, rec = np.full(len(inp["b"]), np.nan), np.full(16, np.nan)
        ev.ctx.check(ev.ctx.lib.pk_solve_kkt(ev.ctx.handle, int(inp["with_h"]), opt(inp["s1"]), opt(inp["s2"]), precond, opt(minv),
                                             opt(inp["b"]), opt(x0), TOL, maxiter, check_every, runtime.as_dp(x), runtime.as_dp(rec)))
        return x, rec


@pytest.fixture(scope="module", params=["A", "B"])
def synthetic(request):
    s = Synthetic(request.param)
    yield s
    s.ev.close()


def _synthetic_cases(ctx):
    """(family, with_h, preconditioned): A quasi and eq, with and without H, preconditioned and not; B quasi preconditioned."""
    if ctx == "A":
        return [(f, h, p) for f in ("quasi", "eq") for h in (True, False) for p in (True, False)]
    return [("quasi", True, True), ("quasi", False, True)]


def test_synthetic_systems_match_the_emulator_bit_for_bit(synthetic):
    kk = synthetic.random
    for family, with_h, pre in _synthetic_cases(kk.sy.ctx):
        inp = kk.inputs(family, with_h)
        minv = kk.precond(with_h, inp["s1"], inp["s2"]) if pre else None
        x0 = inp["x0"] if pre else None
        want_x, want_rec = mr.emulate_solve(kk, with_h, inp["s1"], inp["s2"], minv, inp["b"], x0, TOL, 400)
        assert want_rec[mr.STATUS] == 1.0
        for chunk in (1, 5):
            x, rec = synthetic.device_solve(kk, inp, minv, x0, chunk)
            print(f"{kk.sy.ctx} {family} H={with_h} pre={pre}: status {rec[0]}, {int(rec[1])} iterations, chunks of {chunk}")
            _same("record", rec, want_rec)
            _same("x", x, want_x)


def test_the_kkt_product_matches_the_emulator_bit_for_bit(synthetic):
    kk = synthetic.random
    ev = synthetic.ev
    inp = kk.inputs("quasi", True)
    jv, hv, s1, s2, v = (_up(a) for a in (kk.sy.jvals, kk.sy.hvals, inp["s1"], inp["s2"], inp["x0"]))
    for with_h in (True, False):
        for k1, k2 in ((s1, s2), (None, s2), (s1, None), (None, None)):
            y = Buf(kk.N)
            _sync()
            ev.ctx.check(ev.ctx.lib.pk_kkt_apply_dev(ev.ctx.handle, jv.data_ptr(), hv.data_ptr() if with_h else None, _ptr(k1), _ptr(k2),
                                                     v.data_ptr(), y.ptr, None))
            ev.sync()
            want = kk.kv(with_h, None if k1 is None else inp["s1"], None if k2 is None else inp["s2"], inp["x0"])
            _same(f"K v (H {with_h}, s1 {k1 is not None}, s2 {k2 is not None})", y.fetch(), want)


def test_the_host_form_matches_the_device_pointer_form_and_the_emulator(synthetic):
    """On the values pk_linearize left (the model's own), under the synthetic structures: the preconditioner built on the
    device, the uploads, the chunks of check_every."""
    kk = synthetic.real
    for family, with_h in ((("quasi", True), ("quasi", False), ("eq", True)) if kk.sy.ctx == "A" else (("quasi", True),)):
        inp = kk.inputs(family, with_h)
        minv = kk.precond(with_h, inp["s1"], inp["s2"])
        x0 = inp["x0"]
        want_x, want_rec = mr.emulate_solve(kk, with_h, inp["s1"], inp["s2"], minv, inp["b"], x0, TOL, 400)
        print(f"{kk.sy.ctx} {family} H={with_h}: status {want_rec[0]} after {int(want_rec[1])} iterations")
        dev_x, dev_rec = synthetic.device_solve(kk, inp, minv, x0, 8)
        _same("device-pointer record", dev_rec, want_rec)
        _same("device-pointer x", dev_x, want_x)
        for ce in (1, 3, 64):
            x, rec = synthetic.host_solve(inp, 1, None, x0, 400, ce)      # the device-built preconditioner
            _same(f"host record, check_every {ce}", rec, want_rec)
            _same(f"host x, check_every {ce}", x, want_x)
            assert rec[mr.FRESH] == 0.0
        x, rec = synthetic.host_solve(inp, 2, minv, x0, 400, 8)           # the caller's minv: the array the build gives
        _same("host x, precond 2", x, want_x)
        plain_x, plain_rec = mr.emulate_solve(kk, with_h, inp["s1"], inp["s2"], None, inp["b"], None, TOL, 40, check_every=3)
        x, rec = synthetic.host_solve(inp, 0, None, None, 40, 3)          # no preconditioner, no x0
        _same("host record, precond 0", rec, plain_rec)
        _same("host x, precond 0", x, plain_x)
        k = int(want_rec[mr.ITERS]) - 1
        assert k >= 1
        x, rec = synthetic.host_solve(inp, 1, None, x0, k, 3)             # exhaustion: status 4 in the host copy
        ref_x, ref_rec = mr.emulate_solve(kk, with_h, inp["s1"], inp["s2"], minv, inp["b"], x0, TOL, k, check_every=3)
        assert rec[0] == 4.0 and rec[1] == k
        _same("exhausted record", rec, ref_rec)
        _same("exhausted x", x, ref_x)
        bad = minv.copy()
        bad[3] = -40.0 * minv[3]                                          # a negative entry of the caller's minv
        x, rec = synthetic.host_solve(inp, 2, bad, None, 60, 8)
        ref_x, ref_rec = mr.emulate_solve(kk, with_h, inp["s1"], inp["s2"], bad, inp["b"], None, TOL, 60)
        _same("record with a negative preconditioner entry", rec, ref_rec)
        _same("x with a negative preconditioner entry", x, ref_x)


def test_refusals_enqueue_nothing(synthetic):
    from pockit_amd import runtime

    ev, kk = synthetic.ev, synthetic.random
    lib, h = ev.ctx.lib, ev.ctx.handle
    inp = kk.inputs("quasi", True)
    x, rec = np.full(kk.N, -3.0), np.full(16, -3.0)
    dp = lambda a: runtime.as_dp(a)  # noqa: E731
    b, s1, s2 = (np.ascontiguousarray(inp[k]) for k in ("b", "s1", "s2"))
    call = lambda precond, tol, maxiter, ce: lib.pk_solve_kkt(  # noqa: E731
        h, 1, dp(s1), dp(s2), precond, None, dp(b), None, tol, maxiter, ce, dp(x), dp(rec))
    assert call(0, -1.0, 8, 8) == 134 and call(0, float("nan"), 8, 8) == 134 and call(0, float("inf"), 8, 8) == 134
    assert call(0, TOL, 0, 8) == 134 and call(0, TOL, 8, 0) == 134 and call(3, TOL, 8, 8) == 134 and call(-1, TOL, 8, 8) == 134
    assert call(2, TOL, 8, 8) == 60                                      # precond 2 without minv
    assert lib.pk_minres_advance_dev(h, 0, None) == 134
    assert lib.pk_kkt_apply_dev(h, None, None, None, None, None, None, None) == 110
    assert lib.pk_minres_begin_dev(h, None, None, None, None, None, None, None, None, TOL, None) == 110
    ev.sync()
    assert np.all(x == -3.0) and np.all(rec == -3.0)


# ---------------------------------------------------------------- models against SciPy on the oracle's matrices
def _minres(K, b, minv, tol, maxiter, x0=None):
    """The reference preconditioned MINRES in plain NumPy, the unit's iteration with NumPy's sums: (x, iterations, status)"""
    x = np.zeros(len(b)) if x0 is None else x0.copy()
    r1 = b - K @ x
    y = minv * r1
    r2 = r1.copy()
    beta = math.sqrt(r1 @ y)
    thr = tol * math.sqrt(b @ (minv * b))
    if beta <= thr:
        return x, 0, 1
    oldb = dbar = epsln = 0.0
    phibar, cs, sn = beta, -1.0, 0.0
    w = np.zeros(len(b))
    w2 = np.zeros(len(b))
    for k in range(1, maxiter + 1):
        v = y / beta
        t = K @ v
        alfa = v @ t
        if k >= 2:
            t = t - (beta / oldb) * r1
        t = t - (alfa / beta) * r2
        r1, r2 = r2, t
        y = minv * t
        oldb, beta = beta, math.sqrt(t @ y)
        oldeps, delta, gbar = epsln, cs * dbar + sn * alfa, sn * dbar - cs * alfa
        epsln, dbar = sn * beta, -cs * beta
        gamma = math.hypot(gbar, beta)
        cs, sn = gbar / gamma, beta / gamma
        phi, phibar = cs * phibar, sn * phibar
        w2, w = w, (v - oldeps * w2 - delta * w) / gamma
        x = x + phi * w
        if phibar <= thr:
            return x, k, 1
    return x, maxiter, 4


def _recip(a):
    a = np.abs(a)
    return np.where(a > 0, 1.0 / np.where(a > 0, a, 1.0), 1.0)


class KktSolve:
    """Per model the inputs of the solve and its references, computed once."""

    def __init__(self, case):
        J, H = case.J, case.H
        n, m = case.n, case.m
        self.rho = max(1.0, float(abs(H).sum(axis=1).max()))
        self.s1, self.s2 = 2.0 * self.rho, 0.5
        self.b = np.random.default_rng(11).standard_normal(n + m)
        eye = scipy.sparse.eye_array
        self.K = scipy.sparse.csc_array(scipy.sparse.block_array([[H + self.s1 * eye(n), J.T], [J, -self.s2 * eye(m)]]))
        self.K_no_h = scipy.sparse.csc_array(scipy.sparse.block_array([[self.s1 * eye(n), J.T], [J, -self.s2 * eye(m)]]))
        self.ref = scipy.sparse.linalg.spsolve(self.K, self.b)
        minv1 = _recip(H.diagonal() + self.s1)
        self.minv = np.concatenate((minv1, _recip(J.multiply(J) @ minv1 + self.s2)))
        self.count = _minres(self.K, self.b, self.minv, TOL, 20 * (n + m))[1]
        self.count_plain = _minres(self.K, self.b, np.ones(n + m), TOL, 20 * (n + m))[1]
        self.lam = 0.5                       # no eigenvalue of K in (-0.5, rho), rho >= 1

    def bounds(self, b, minv):
        """(the M-norm residual bound, the error bound) of a solve of right-hand side b under preconditioner minv"""
        return 2 * TOL * mr.m_norm(b, minv), mr.residual_bound_2norm(TOL, b, minv) / self.lam


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def case(request):
    c = Case(*request.param)
    c.kkt = KktSolve(c)
    yield c
    c.system.evaluator.close()


def _close3(a, b, what):
    err, bound = np.max(np.abs(a - b)), 3 * 1e-11 * max(1.0, np.max(np.abs(b)))
    print(f"{what}: err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, what


def test_kkt_v_matches_the_oracle_in_every_combination(case):
    lin = case.linearize()
    rng = np.random.default_rng(13)
    n, m = case.n, case.m
    J, H = case.J, case.H
    v = rng.standard_normal(n + m)
    s1_vec, s2_vec = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, m)
    for with_h in (True, False, None):
        for s1 in (None, 0.75, s1_vec):
            for s2 in (None, 0.25, s2_vec):
                top = J.T @ v[n:] + (0.0 if s1 is None else s1 * v[:n])
                if with_h or with_h is None:
                    top = top + H @ v[:n]
                low = J @ v[:n] - (0.0 if s2 is None else s2 * v[n:])
                got = lin.kkt_v(v, s1, s2, with_h=with_h)
                _close3(got, np.concatenate((top, low)), f"kkt_v H={with_h} s1={type(s1).__name__} s2={type(s2).__name__}")
    op = lin.kkt_operator(0.75, 0.25)
    assert op.shape == (n + m, n + m) and np.array_equal(op @ v, lin.kkt_v(v, 0.75, 0.25))
    with pytest.raises(ValueError):
        lin.kkt_v(v[:n])


def test_the_solve_meets_the_residual_and_error_bounds(case):
    lin = case.linearize()
    kk = case.kkt
    b, K, n = kk.b, kk.K, case.n
    maxiter = math.ceil(1.1 * kk.count)
    minv = lin.kkt_precond(kk.s1, kk.s2)
    assert np.all(minv > 0) and np.allclose(minv, kk.minv, rtol=1e-9, atol=0.0)
    x, info = lin.solve_kkt(b, kk.s1, kk.s2, tol=TOL, maxiter=maxiter)
    res_bound, err_bound = kk.bounds(b, minv)
    res, err = mr.m_norm(b - K @ x, minv), np.max(np.abs(x - kk.ref))
    print(f"device {info.iterations} iterations, reference {kk.count} (maxiter {maxiter}); M-norm residual {res:.3e} (bound {res_bound:.3e}), "
          f"error {err:.3e} (bound {err_bound:.3e}); rel_residual {info.rel_residual:.3e}")
    assert info.status == "converged" and 0 < info.iterations <= maxiter
    assert res <= res_bound
    assert err <= err_bound
    assert info.rel_residual <= TOL and info.record[mr.FRESH] == 0.0
    assert np.shares_memory(info.primal, x) and np.array_equal(info.primal, x[:n]) and np.array_equal(info.dual, x[n:])
    with pytest.raises(AttributeError):
        info.status = "x"
    # the preconditioner as an array is the device's build, bit for bit; none at all converges to the same solution
    x2, info2 = lin.solve_kkt(b, kk.s1, kk.s2, precond=minv, tol=TOL, maxiter=maxiter)
    assert np.array_equal(x, x2) and np.array_equal(info.record, info2.record)
    plain_max = math.ceil(1.1 * kk.count_plain)
    x3, info3 = lin.solve_kkt(b, kk.s1, kk.s2, precond=None, tol=TOL, maxiter=plain_max)
    print(f"{info3.iterations} iterations without a preconditioner (reference {kk.count_plain})")
    assert info3.status == "converged"
    assert np.linalg.norm(b - K @ x3) <= 2 * TOL * np.linalg.norm(b) and np.max(np.abs(x3 - kk.ref)) <= kk.bounds(b, None)[1]
    # x0 given, against x0 = None applied to b - K x0: the same solution within the bound
    x0 = np.random.default_rng(17).standard_normal(len(b))
    x4, info4 = lin.solve_kkt(b, kk.s1, kk.s2, x0=x0, tol=TOL, maxiter=2 * maxiter)
    b5 = b - K @ x0
    x5, info5 = lin.solve_kkt(b5, kk.s1, kk.s2, tol=TOL, maxiter=2 * maxiter)
    assert info4.status == "converged" and info5.status == "converged"
    assert np.max(np.abs(x4 - kk.ref)) <= err_bound
    assert np.max(np.abs(x0 + x5 - kk.ref)) <= kk.bounds(b5, minv)[1]
    # exhaustion, and a negative entry in the caller's preconditioner
    xk, infok = lin.solve_kkt(b, kk.s1, kk.s2, tol=TOL, maxiter=2, check_every=5)
    assert infok.status == "maxiter" and infok.iterations == 2 and np.all(np.isfinite(xk))
    _, info_bad = lin.solve_kkt(b, kk.s1, kk.s2, precond=-minv, tol=TOL, maxiter=maxiter)
    assert info_bad.status == "preconditioner_not_positive" and info_bad.iterations == 0


def test_stale_handles_missing_hessians_and_the_other_products(case):
    lin = case.linearize()
    kk = case.kkt
    d, rhs = np.ones(case.m), np.random.default_rng(3).standard_normal(case.n)
    others = lambda: (lin.solve_condensed(rhs, d, kk.s1, tol=TOL, maxiter=64)[0], lin.jv(case.v), lin.jtv(case.y), lin.hv(case.v),  # noqa: E731
                      lin.row_norms("J", "1"), lin.jtdj_diag(d))
    before = others()
    lin.solve_kkt(kk.b, kk.s1, kk.s2, tol=TOL, maxiter=math.ceil(1.1 * kk.count))
    for a, b in zip(before, others()):
        assert np.array_equal(a, b)
    no_h = case.system.linearize(case.x)
    with pytest.raises(RuntimeError, match="stale"):
        lin.kkt_v(kk.b)
    with pytest.raises(RuntimeError, match="stale"):
        lin.solve_kkt(kk.b)
    with pytest.raises(RuntimeError, match="stale"):
        lin.kkt_precond(kk.s1, kk.s2)
    with pytest.raises(RuntimeError, match="no Hessian"):
        no_h.kkt_v(kk.b, with_h=True)
    with pytest.raises(RuntimeError, match="no Hessian"):
        no_h.solve_kkt(kk.b, with_h=True)
    x, info = no_h.solve_kkt(kk.b, kk.s1, kk.s2, tol=TOL, maxiter=4 * kk.count + 40)      # without H: [[s1 I, J^T], [J, -s2 I]]
    minv = no_h.kkt_precond(kk.s1, kk.s2)
    assert info.status == "converged" and mr.m_norm(kk.b - kk.K_no_h @ x, minv) <= 2 * TOL * mr.m_norm(kk.b, minv)
