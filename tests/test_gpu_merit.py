"""pk_trial, pk_merit and pk_merit_fin (pockit_amd/csrc/pk_merit.cpp) on the device.

Synthetic cases through ``pk_merit_reduce_dev`` on the context of one small model: the inputs, the ``fsum`` reference, the
bound derived from the depth of the association and the bit-for-bit emulator are described, and tested, in
tests/merit_cases.py (tests/test_merit_cases_cpu.py).  Lengths 1, 255, 256, 257, 2 047, 2 048, 2 049 on both sides with
B in {1, 3, 64}; 524 289 values with B = 9 (2 313 workgroups: past the grid cap of 2 048 into the stride loop, 257 pieces: the
second strided trip of pk_merit_fin); leading dimensions larger than the lengths with NaN in the padding; non-finite g, grad
and f values; ``d`` given and NULL; ``out`` between sentinels in a NaN-filled array.  Asserted: bit equality with the emulator,
the derived bound against ``fsum`` on the exact cases, intact sentinels, the same bits from a second call; on full-mantissa
inputs pk_trial bit-equal to NumPy's ``x + a * d`` (a fused multiply-add would differ: the CPU file shows it).

Model cases, five entries each, on the four models of tests/test_gpu_cycle_batch.py and the random model that takes the loop
of single cycles: ``merit_batch(X)`` is bit-equal to the emulator applied to what ``evaluate_batch(X, None)`` returns for the
same X -- no tolerance is involved; ``merit_scan(x, d, alphas)`` is bit-equal to ``merit_batch(x + a * d, d)``; the
device-pointer forms are bit-equal to the host forms; ``batch_launches()`` rises by exactly one per chunk where the batch is one
launch and by none for the loop model; a ``RuntimeWarning`` is an error.  Entry 0 lies inside the variable bounds (bound1 = 0),
entry 3 has three components pushed past ``v_ub`` (bound1 > 0), and no entry satisfies the defect equations (theta1 > 0 in
every entry: theta1 = 0 would need a feasible point, which none of these models has at hand) -- confirmed with the oracle's g."""
import ctypes as C
import importlib

import numpy as np
import pytest

import merit_cases as mc
import models

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]

PAD = 8
SENTINEL = -7.25e77
CASES = {
    "brach_3x4": ("brachistochrone", "radau", dict(mesh=3, num_point=4)),
    "brach_60x5": ("brachistochrone", "radau", dict(mesh=60, num_point=5)),
    "rocket_6x4": ("two_stage_rocket", "radau", dict(mesh=6, num_point=4)),
    "quadrotor_lgl_20x6": ("planar_quadrotor", "lobatto", dict(mesh=20, num_point=6)),
}
RANDOM_SEED = 2
MODELS = tuple(CASES) + ("random",)
ENTRIES = 5
ALPHAS = np.array([0.0, 1.0, 0.5, 0.25, 0.125])

_built = {}


def case(name):
    """(system, x) of a model, built once."""
    if name not in _built:
        if name == "random":
            import random_models as rm

            system, _ = rm.random_model(importlib.import_module("pockit_amd.radau"), RANDOM_SEED, "radau")
            x = rm.random_inputs(system, RANDOM_SEED)[0]
        else:
            builder, scheme, kw = CASES[name]
            system, _, guess = getattr(models, builder)(importlib.import_module(f"pockit_amd.{scheme}"), **kw)
            x = models.bench_inputs(system, guess)[0]
        _built[name] = (system, np.asarray(x, dtype=np.float64))
    return _built[name]


def model_inputs(system, x):
    """(X (5, n), d): entry b is x (1 + 1e-3 (b + 1)); entry 0 is moved into the variable bounds, three components of entry 3
    past ``v_ub`` (past ``v_lb`` downwards where no upper bound is finite)."""
    p = system.plan
    X = np.array([x * (1.0 + 1.0e-3 * (b + 1)) for b in range(ENTRIES)])
    X[0] = np.clip(X[0], p.v_lb, p.v_ub)
    up = np.flatnonzero(np.isfinite(p.v_ub))[:3]
    if len(up):
        X[3, up] = p.v_ub[up] + 1.0 + 0.5 * np.arange(len(up))
    else:
        down = np.flatnonzero(np.isfinite(p.v_lb))[:3]
        assert len(down)
        X[3, down] = p.v_lb[down] - 1.0 - 0.5 * np.arange(len(down))
    d = 1.0e-3 * np.random.default_rng(11).standard_normal(p.n)
    return X, d


def bounds(system):
    p = system.plan
    return p.c_lb, p.c_ub, p.v_lb, p.v_ub


def same_bits(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    diff = np.argwhere(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64))
    assert len(diff) == 0, f"{what}: {len(diff)} of {a.size} values differ, first at {diff[0]}: {a[tuple(diff[0])]!r} != {b[tuple(diff[0])]!r}"


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
        if host.nbytes:
            self.ev.ctx.check(self.lib.pk_copy_dev(self.h, ptr.value, host.ctypes.data, host.nbytes, None))
            self.ev.sync()
        return ptr.value

    def read(self, ptr, count):
        out = np.empty(count)
        self.ev.ctx.check(self.lib.pk_copy_dev(self.h, out.ctypes.data, ptr, out.nbytes, None))
        self.ev.sync()
        return out


@pytest.fixture(scope="module")
def small():
    system = models.brachistochrone(importlib.import_module("pockit_amd.radau"), 3, 4)[0]
    ev = system.evaluator
    yield ev
    ev.close()


def framed(count):
    """A NaN-filled result between two runs of sentinels."""
    a = np.full(count + 2 * PAD, np.nan)
    a[:PAD] = a[-PAD:] = SENTINEL
    return a


SYNTHETIC = mc.exact_cases() + (mc.full_case(), mc.no_d_case())


@pytest.mark.parametrize("c", SYNTHETIC, ids=lambda c: c.id)
def test_reduction_on_synthetic_vectors(small, c):
    ev = small
    lib, h = ev.ctx.lib, ev.ctx.handle
    want = c.emulated()
    with DeviceArrays(ev) as dev:
        g, clb, cub, X, vlb, vub, grad, f = (dev.new(a) for a in (c.g, c.clb, c.cub, c.X, c.vlb, c.vub, c.grad, c.f))
        d = None if c.d is None else dev.new(c.d)
        out = dev.new(framed(8 * c.B))
        got = []
        for _ in range(2):
            ev.ctx.check(lib.pk_merit_reduce_dev(h, c.B, c.n_g, g, c.ldg, clb, cub, c.n_x, X, c.ldx, vlb, vub, grad, c.ldgrad, d, f,
                                                 out + 8 * PAD, None))
            ev.sync()
            raw = dev.read(out, 8 * c.B + 2 * PAD)
            assert (raw[:PAD] == SENTINEL).all() and (raw[-PAD:] == SENTINEL).all(), "sentinels"
            got.append(raw[PAD:-PAD].reshape(c.B, 8))
            fresh = framed(8 * c.B)                      # (alive until the copy has been waited for)
            ev.ctx.check(lib.pk_copy_dev(h, out, fresh.ctypes.data, fresh.nbytes, None))
            ev.sync()
    same_bits(got[0], want, f"{c.id} against the emulator")
    same_bits(got[1], got[0], f"{c.id}: a second call")
    if c.kind != "full":
        bad = c.failures(got[0])
        assert len(bad) == 0, f"{c.id}: cells outside the derived bound: {bad[:5].tolist()}"
    if c.d is None:
        assert (got[0][:, 6] == 0.0).all()
    assert np.isfinite(got[0][:, 1:]).all()


@pytest.mark.parametrize("name", ["brach_3x4", "brach_60x5"])
def test_trial_points_have_the_bits_of_numpy(name):
    """Full mantissas; n = 53 (one workgroup, a quarter full) and 1 205 (five, the last one partial); B = 1, 3, 64; rows three
    doubles further apart than n, the padding untouched."""
    system, _ = case(name)
    ev, n = system.evaluator, system.plan.n
    x, d, alphas = mc.trial_case(n)
    want = mc.trial_points(x, d, alphas)
    assert np.array_equal(want, x[None, :] + alphas[:, None] * d[None, :])
    assert (want != mc.trial_points(x, d, alphas, fma=True)).any()      # a fused multiply-add would be seen
    ldx = n + 3
    with DeviceArrays(ev) as dev:
        dx, dd = dev.new(x), dev.new(d)
        for B in (1, 3, 64):
            dX = dev.new(np.full(B * ldx, SENTINEL))
            ev.trial_points_dev(B, dx, dd, alphas[:B], dX, ldx=ldx)
            ev.sync()
            got = dev.read(dX, B * ldx).reshape(B, ldx)
            same_bits(got[:, :n], want[:B], f"{name} B = {B}")
            assert (got[:, n:] == SENTINEL).all()


def launches_per_batch(ev, B):
    from pockit_amd import runtime

    return -(-B // runtime.MAX_BATCH) if ev._ensure_batch() == "kernel" else 0


@pytest.mark.parametrize("name", MODELS)
def test_merit_of_a_model_batch_is_the_emulator_on_its_outputs(name):
    system, x = case(name)
    ev = system.evaluator
    X, d = model_inputs(system, x)
    assert ev._ensure_batch() == ("loop" if name == "random" else "kernel")
    per = launches_per_batch(ev, ENTRIES)
    before = ev.batch_launches()
    f, grad, g, J, H = system.evaluate_batch(X)
    assert ev.batch_launches() - before == per
    for dd in (None, d):
        want = mc.emulate_dense(f, grad, g, X, bounds(system), dd)
        before = ev.batch_launches()
        got = system.merit_batch(X, dd)
        assert ev.batch_launches() - before == per
        same_bits(got.table, want, f"{name} merit_batch, d {'given' if dd is not None else 'None'}")
    assert (got.bad == 0).all() and np.isfinite(got.table).all()
    # the comparison is not vacuous
    assert (got.theta1 > 0).any() and got.bound1[3] > 0 and got.bound1[0] == 0 and (got.slope != 0).any()
    assert np.array_equal(got.f, f) and (got.theta_inf <= got.theta1).all() and (got.theta2_sq > 0).all()
    if name == "random":
        assert ev.batch_launches() == 0


@pytest.mark.parametrize("name", MODELS)
def test_scan_is_the_batch_on_the_trial_points_and_the_device_forms_agree(name):
    system, x = case(name)
    ev, p = system.evaluator, system.plan
    _, d = model_inputs(system, x)
    per = launches_per_batch(ev, ENTRIES)
    trial = x[None, :] + ALPHAS[:, None] * d[None, :]
    before = ev.batch_launches()
    scan = system.merit_scan(x, d, ALPHAS)
    assert ev.batch_launches() - before == per
    want = system.merit_batch(trial, d)
    same_bits(scan.table, want.table, f"{name}: merit_scan against merit_batch(x + a d)")
    assert len(np.unique(scan.table[:, 1])) == ENTRIES      # (five different points)
    B = ENTRIES
    with DeviceArrays(ev) as dev:
        dx, dd = dev.new(x), dev.new(d)
        dX = dev.new(np.full(B * p.n, np.nan))
        df, dgrad, dg, dJ = (dev.new(np.full(B * k, np.nan)) for k in (1, p.n, p.m, p.nnz_J))
        out = dev.new(framed(8 * B))
        before = ev.batch_launches()
        ev.trial_points_dev(B, dx, dd, ALPHAS, dX)
        ev.cycle_batch_dev(B, dX, None, [], df, dgrad, dg, dJ, None)
        ev.merit_batch_dev(B, df, dg, dgrad, dX, out + 8 * PAD, d_d=dd)
        ev.sync()
        assert ev.batch_launches() - before == per
        raw = dev.read(out, 8 * B + 2 * PAD)
        same_bits(dev.read(dX, B * p.n).reshape(B, p.n), trial, f"{name}: trial points on the device")
    assert (raw[:PAD] == SENTINEL).all() and (raw[-PAD:] == SENTINEL).all()
    same_bits(raw[PAD:-PAD].reshape(B, 8), scan.table, f"{name}: the device-pointer forms against the host form")


def test_more_entries_than_one_launch_holds_and_edges():
    from pockit_amd import runtime

    name = "brach_3x4"
    system, x = case(name)
    ev, p = system.evaluator, system.plan
    _, d = model_inputs(system, x)
    alphas = np.linspace(0.0, 1.0, 65)
    assert runtime.MAX_BATCH == 64 and ev._ensure_batch() == "kernel"
    before = ev.batch_launches()
    got = ev.merit_scan(x, d, alphas)
    assert ev.batch_launches() - before == 2      # 64 + 1
    assert got.shape == (65, 8)
    same_bits(got[[0, 32, 64]], ev.merit_scan(x, d, alphas[[0, 32, 64]]), "65 points against 3 of them")
    assert ev.merit_batch(np.zeros((0, p.n))).shape == (0, 8) and ev.merit_scan(x, d, []).shape == (0, 8)
    for bad in (np.zeros(p.n), np.zeros((2, p.n + 1))):
        with pytest.raises(ValueError):
            ev.merit_batch(bad)
    with pytest.raises(ValueError):
        ev.merit_scan(x, d[:-1], alphas)
    with pytest.raises(ValueError):
        ev.set_bounds(c_lb=np.zeros(p.m + 1))
    # bounds of the caller's: everything allowed, nothing is violated; the plan's again afterwards
    inf = np.inf
    ev.set_bounds(np.full(p.m, -inf), np.full(p.m, inf), np.full(p.n, -inf), np.full(p.n, inf))
    free = ev.merit_scan(x, d, alphas[:3])
    assert (free[:, 1:6] == 0).all() and (free[:, 6] != 0).any()
    ev.set_bounds(c_lb=np.full(p.m, np.nan))
    with pytest.raises(RuntimeError, match="126"):
        ev.merit_scan(x, d, alphas[:3])
    ev.set_bounds()
    same_bits(ev.merit_scan(x, d, alphas[:3]), got[:3], "the plan's bounds again")
    # a compact cycle layout is not offered (error 88), as for the batch
    ev.set_cycle_layout(True, False)
    try:
        before = ev.batch_launches()
        with pytest.raises(RuntimeError, match="88"):
            ev.merit_scan(x, d, alphas[:3])
        assert ev.batch_launches() == before
    finally:
        ev.set_cycle_layout(False, False)
    same_bits(ev.merit_scan(x, d, alphas[:3]), got[:3], "after the refusal")
