"""A batch of iterates in ONE launch of the fused cycle (kernel pk_cycleb, ``Evaluator.cycle_batch``): every output of every
entry is BIT-identical to the single launch on that entry (``np.array_equal`` on the ``uint64`` patterns) and within the
tolerance of ``smoke()`` -- ``1e-11 * max(1, max|ref|)`` -- of the oracle.

Inputs: ``benchmarks.bench_inputs``; entry ``b`` is ``x * (1 + 1e-3 (b + 1))`` with a lambda and a sigma of its own, so that no
two entries can agree by accident.  The models are the smallest that reach the paths a batch can go wrong on: one tile
smaller than a wave (3 x 4), several tile blocks and partial sums from several workgroups per entry (60 x 5), two phases, LGL
and gradient slots shared by all nodes.  Single launches and oracle values are computed once per (model, entry) and shared.

The evaluator holds its batched kernel against single launches on first use and, on a difference, serves batches by a loop of
single cycles with a ``RuntimeWarning`` -- values that would pass every comparison here without pk_cycleb having run.  So every
case that is meant to be one launch asserts that the kernel served it: the runtime's count of pk_cycleb launches rises by
exactly one per chunk of at most 64 entries (``served_by_kernel``), and a ``RuntimeWarning`` is an error in this file.  The
model that takes the loop asserts the opposite."""
import contextlib
import ctypes as C
import importlib

import numpy as np
import pytest

import models

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]

TOL = 1e-11
NAMES = ("f", "grad", "g", "J", "H")

CASES = {
    "brach_3x4": ("brachistochrone", "radau", dict(mesh=3, num_point=4)),
    "brach_60x5": ("brachistochrone", "radau", dict(mesh=60, num_point=5)),
    "rocket_6x4": ("two_stage_rocket", "radau", dict(mesh=6, num_point=4)),
    "quadrotor_lgl_20x6": ("planar_quadrotor", "lobatto", dict(mesh=20, num_point=6)),
}
RANDOM_SEED = 2      # tests/random_models.py, radau: objective and system constraints nonlinear in the integrals (prepass_* all set)

_built, _single, _oracle = {}, {}, {}


def _ns(scheme, pkg):
    return importlib.import_module(f"{pkg}.{scheme}")


def case(name):
    """(system, oracle system, x, lambda) of a model, built once."""
    if name not in _built:
        if name == "random":
            import random_models as rm

            system, _ = rm.random_model(_ns("radau", "pockit_amd"), RANDOM_SEED, "radau")
            ref, _ = rm.random_model(_ns("radau", "oracle"), RANDOM_SEED, "radau")
            x, lam, _ = rm.random_inputs(system, RANDOM_SEED)
        else:
            builder, scheme, kw = CASES[name]
            system, _, guess = getattr(models, builder)(_ns(scheme, "pockit_amd"), **kw)
            ref, _, _ = getattr(models, builder)(_ns(scheme, "oracle"), **kw)
            x, lam, _ = models.bench_inputs(system, guess)
        _built[name] = (system, ref, x, lam)
    return _built[name]


def entry(name, b):
    """Inputs of batch entry ``b``: a function of the model and ``b`` alone."""
    _, _, x, lam = case(name)
    return x * (1.0 + 1.0e-3 * (b + 1)), lam + np.random.default_rng(100 + b).standard_normal(lam.shape), 1.0 - 0.125 * b


def batch(name, B):
    rows = [entry(name, b) for b in range(B)]
    return (np.array([r[0] for r in rows]).reshape(B, -1), np.array([r[1] for r in rows]).reshape(B, -1),
            np.array([r[2] for r in rows], dtype=np.float64))


def frozen(arrays):
    out = tuple(np.array(a, dtype=np.float64, ndmin=1) for a in arrays)
    for a in out:
        a.flags.writeable = False
    return out


def single(name, b):
    """The five outputs of ONE launch of the cycle on entry ``b`` (computed once, read-only)."""
    if (name, b) not in _single:
        x, lam, sigma = entry(name, b)
        _single[name, b] = frozen(case(name)[0].evaluator.cycle(x, lam, sigma))
    return _single[name, b]


def oracle(name, b):
    if (name, b) not in _oracle:
        ref = case(name)[1]
        x, lam, sigma = entry(name, b)
        _oracle[name, b] = frozen((ref.objective(x), ref.gradient(x), ref.constraints(x), ref.jacobian(x), ref.hessian(x, lam, sigma)))
    return _oracle[name, b]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).reshape(-1).view(np.uint64)


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.size == b.size, what
    assert np.array_equal(bits(a), bits(b)), f"{what}: {int(np.sum(bits(a) != bits(b)))} of {a.size} values differ"


def close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert a.shape == b.shape, what
    if a.size:
        err = np.max(np.abs(a - b))
        assert err <= TOL * max(1.0, np.max(np.abs(b))), f"{what}: err {err:.3e}"


class DeviceArrays:
    """Device buffers of doubles through the library's own allocator and copies (freed on exit)."""

    def __init__(self, ev):
        self.ev, self.lib, self.h, self.ptrs = ev, ev.ctx.lib, ev.ctx.handle, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for ptr in self.ptrs:
            self.lib.pk_device_free(self.h, ptr)

    def new(self, host):
        host = np.ascontiguousarray(host, dtype=np.float64)
        ptr = C.c_void_p()
        self.ev.ctx.check(self.lib.pk_device_alloc(self.h, max(host.nbytes, 8), 0, C.byref(ptr)))
        self.ptrs.append(ptr.value)
        self.ev.ctx.check(self.lib.pk_copy_dev(self.h, ptr.value, host.ctypes.data, host.nbytes, None))
        self.ev.sync()
        return ptr.value

    def read(self, ptr, count):
        out = np.empty(count)
        self.ev.ctx.check(self.lib.pk_copy_dev(self.h, out.ctypes.data, ptr, out.nbytes, None))
        self.ev.sync()
        return out


@contextlib.contextmanager
def served_by_kernel(ev, launches):
    """The block launches pk_cycleb exactly ``launches`` times -- and the evaluator's batched object passed its own check."""
    assert ev._ensure_batch() == ("kernel" if launches else ev._batch_state)
    before = ev.batch_launches()
    yield
    assert ev.batch_launches() - before == launches, f"{ev.batch_launches() - before} launches of pk_cycleb, expected {launches}"


def check_batch(name, got, B, entries=None, with_oracle=True):
    assert [None if a is None else a.shape[0] for a in got] == [B] * 5
    for b in (range(B) if entries is None else entries):
        for k, out in enumerate(got):
            same_bits(out[b], single(name, b)[k], f"{name} entry {b} {NAMES[k]} against its single launch")
            if with_oracle:
                close(out[b], oracle(name, b)[k], f"{name} entry {b} {NAMES[k]} against the oracle")


@pytest.mark.parametrize("B", [1, 2, 5])
def test_one_tile_smaller_than_a_wave(B):
    """3 x 4: 12 nodes in ONE tile block (one workgroup per role), every tile far smaller than a wave, and the edge and
    finalize workgroups of every entry."""
    ev = case("brach_3x4")[0].evaluator
    tiles = ev.tables.tiles
    assert len(tiles) == 4 and int(np.max(tiles["nj"] * tiles["K"])) < 64
    X, Lam, sig = batch("brach_3x4", B)
    with served_by_kernel(ev, 1):
        got = ev.cycle_batch(X, Lam, sig)
    check_batch("brach_3x4", got, B)


def test_several_tile_blocks_per_entry():
    """60 x 5 = 300 nodes: at least five tiles in at least two tile blocks (the last padded with empty tiles where the count
    is no multiple of four), partial sums from several workgroups per entry."""
    ev = case("brach_60x5")[0].evaluator
    tiles = ev.tables.tiles
    assert int(np.sum(tiles["nj"] > 0)) >= 5 and len(tiles) // 4 >= 2
    X, Lam, sig = batch("brach_60x5", 3)
    with served_by_kernel(ev, 1):
        got = ev.cycle_batch(X, Lam, sig)
    check_batch("brach_60x5", got, 3)


@pytest.mark.parametrize("name", ["rocket_6x4", "quadrotor_lgl_20x6"])
def test_two_phases_and_lgl_with_shared_gradient_slots(name):
    system = case(name)[0]
    if name == "rocket_6x4":
        assert len(system.plan.phase_plans) == 2
    X, Lam, sig = batch(name, 2)
    with served_by_kernel(system.evaluator, 1):
        got = system.evaluator.cycle_batch(X, Lam, sig)
    check_batch(name, got, 2)


def test_x_only_batch_and_untouched_hessian_buffer():
    name, B = "brach_60x5", 3
    system = case(name)[0]
    ev, p = system.evaluator, system.plan
    X, _, _ = batch(name, B)
    with served_by_kernel(ev, 1):
        f, grad, g, J, H = ev.cycle_batch(X)
    assert H is None and f.shape == (B,) and J.shape == (B, p.nnz_J)
    for b in range(B):      # the single x-only path: one x-only launch behind the first callback on a new x
        x = X[b].copy()
        want = (ev.objective(x), ev.gradient(x).copy(), ev.constraints(x).copy(), ev.jacobian(x).copy())
        for k, (a, w) in enumerate(zip((f, grad, g, J), want)):
            same_bits(a[b], w, f"x-only entry {b} {NAMES[k]}")
            close(a[b], oracle(name, b)[k], f"x-only entry {b} {NAMES[k]} against the oracle")
    with DeviceArrays(ev) as dev:
        sizes = (1, p.n, p.m, p.nnz_J)
        dX = dev.new(X)
        o = [dev.new(np.zeros(B * n)) for n in sizes]
        dH = dev.new(np.full(B * p.nnz_H, -7.25))
        with served_by_kernel(ev, 1):
            ev.cycle_batch_dev(B, dX, None, [], *o, dH)
            ev.sync()
        for k, (t, n, a) in enumerate(zip(o, sizes, (f, grad, g, J))):
            same_bits(dev.read(t, B * n), a, f"device form {NAMES[k]}")
        assert (dev.read(dH, B * p.nnz_H) == -7.25).all(), "an x-only batch must not touch d_hess"


def test_a_nan_entry_does_not_leak_into_its_neighbours():
    name = "brach_60x5"
    ev = case(name)[0].evaluator
    X, Lam, sig = batch(name, 3)
    X[1, :] = np.nan
    with np.errstate(all="ignore"), served_by_kernel(ev, 1):
        got = ev.cycle_batch(X, Lam, sig)      # (no error: a NaN of the model's own is passed through, not a failed hand-off)
    check_batch(name, got, 3, entries=(0, 2), with_oracle=False)
    assert np.isnan(got[0][1])


def test_rearming_between_batches_and_single_cycles():
    name = "brach_60x5"
    ev = case(name)[0].evaluator
    X, Lam, sig = batch(name, 3)
    X0, Lam0 = X.copy(), Lam.copy()
    with served_by_kernel(ev, 3):
        check_batch(name, ev.cycle_batch(X, Lam, sig), 3, with_oracle=False)
        check_batch(name, ev.cycle_batch(X[:2], Lam[:2], sig[:2]), 2, with_oracle=False)
        one = ev.cycle(X[0], Lam[0], sig[0])
        for k in range(5):
            same_bits(one[k], single(name, 0)[k], f"single cycle between batches: {NAMES[k]}")
        check_batch(name, ev.cycle_batch(X, Lam, sig), 3, with_oracle=False)
    same_bits(X, X0, "x on return")
    same_bits(Lam, Lam0, "lambda on return")


def test_model_nonlinear_in_the_integrals_takes_the_loop():
    """Seed 2 of tests/random_models.py (radau): every callback needs the integrals first, so the batch is a loop of single
    cycles inside the call -- the same values, and NO launch of pk_cycleb."""
    name = "random"
    ev = case(name)[0].evaluator
    md = ev.model_desc
    assert md.prepass_grad and md.prepass_g and md.prepass_jac and md.prepass_hess
    X, Lam, sig = batch(name, 3)
    with served_by_kernel(ev, 0):
        got = ev.cycle_batch(X, Lam, sig)
    assert ev._ensure_batch() == "loop" and ev.batch_launches() == 0
    check_batch(name, got, 3)


def test_refusals_and_edges():
    from pockit_amd import runtime

    name = "brach_3x4"
    system = case(name)[0]
    ev, p = system.evaluator, system.plan
    empty = ev.cycle_batch(np.zeros((0, p.n)), np.zeros((0, p.m)))
    assert [a.shape for a in empty] == [(0,), (0, p.n), (0, p.m), (0, p.nnz_J), (0, p.nnz_H)]
    assert ev.cycle_batch(np.zeros((0, p.n)))[4] is None
    # 65 entries: two launches (64 + 1)
    assert runtime.MAX_BATCH == 64
    X, Lam, sig = batch(name, 65)
    with served_by_kernel(ev, 2):
        got = ev.cycle_batch(X, Lam, sig)
    check_batch(name, got, 65, entries=(0, 63, 64))
    with served_by_kernel(ev, 1):
        five = ev.cycle_batch(X[:5], Lam[:5], sig[:5])
    for k in range(5):
        same_bits(got[k][:5], five[k], f"65 entries against 5: {NAMES[k]}")
        assert np.isfinite(got[k]).all(), NAMES[k]
        if k != 1:      # (f = t_f: the gradient of this model is the same constant vector at every x)
            assert len(np.unique(got[k].reshape(65, -1), axis=0)) == 65, NAMES[k]
    # ... and through the C ABI: error 87
    lib, h = ev.ctx.lib, ev.ctx.handle
    assert lib.pk_set_batch(h, 65) == 87 and lib.pk_set_batch(h, 0) == 87
    assert b"64" in lib.pk_last_error(h)      # (the message names the limit)
    with DeviceArrays(ev) as dev:      # (refused before any pointer is used)
        t = dev.new(np.zeros(p.n + p.m + p.nnz_J + p.nnz_H + 8))
        one = (C.c_double * 65)(*([1.0] * 65))
        rc = lib.pk_eval_cycle_batch_dev(h, 65, t, p.n, t, p.m, C.cast(one, runtime.c_double_p), t, t, t, t, t, None)
        assert rc == 87
        with pytest.raises(RuntimeError, match="87"):
            ev.cycle_batch_dev(65, t, t, [1.0] * 65, *([t] * 5))
    # wrong shapes
    for bad in (np.zeros(p.n), np.zeros((2, p.n + 1)), np.zeros((2, 2, p.n))):
        with pytest.raises(ValueError):
            ev.cycle_batch(bad)
    with pytest.raises(ValueError):
        ev.cycle_batch(X[:2], Lam[:3], 1.0)
    with pytest.raises(ValueError):
        ev.cycle_batch(X[:2], Lam[:2, :-1], 1.0)
    with pytest.raises(ValueError):
        ev.cycle_batch(X[:2], Lam[:2], np.ones(3))
    # a compact cycle layout is not offered for a batch (error 88)
    ev.set_cycle_layout(True, False)
    try:
        before = ev.batch_launches()
        with pytest.raises(RuntimeError, match="88"):
            ev.cycle_batch(X[:2], Lam[:2], sig[:2])
        assert ev.batch_launches() == before
    finally:
        ev.set_cycle_layout(False, False)
    with served_by_kernel(ev, 1):
        check_batch(name, ev.cycle_batch(X[:2], Lam[:2], sig[:2]), 2, with_oracle=False)


def test_system_evaluate_batch_is_the_evaluators():
    name = "brach_3x4"
    system = case(name)[0]
    X, Lam, sig = batch(name, 2)
    with served_by_kernel(system.evaluator, 2):
        a, b = system.evaluate_batch(X, Lam, sig), system.evaluator.cycle_batch(X, Lam, sig)
    for k in range(5):
        same_bits(a[k], b[k], NAMES[k])
    check_batch(name, a, 2)
    assert system.evaluate_batch(X)[4] is None
