"""GPU: the generated model kernels at non-finite iterates (cases, poisons and the comparison: tests/nonfinite_cases.py).

The interior-point solver rejects a trial point whose f, grad f or J is not finite and the batched cycle passes a NaN of the
model's own through; the parity tests evaluate at finite points only.  These kernels pack several intervals into a wave, pad
lanes, stage rows in LDS and reduce with shuffles: a ``0.0 * stale`` in place of a select makes a NaN appear in a neighbouring
interval, a select where the reference multiplies makes one disappear -- neither shows at a finite point.

For every case and every poison (one slot of x or of lambda set to NaN, and to +-inf where the case allows) every route to
the five arrays is held to the reference (the oracle; the NumPy execution of the plan where an interval has more points than the
oracle can tabulate) by ``compare``: the SAME set of non-finite entries, 1e-11 on the finite ones.  Beside it:

* a slot the transcription dictates changes no bit of any output, a multiplier changes H only;
* after every poisoned evaluation the clean point is evaluated again on the same context and must give the clean bits (a stale
  hand-off slot, a stale partial sum, a cached x);
* x and lambda are not written;
* the damage of one node is local: some of g, J, H has a non-finite set that is neither empty nor everything.

Only values are non-finite; every index stays valid."""
import numpy as np
import pytest

import nonfinite_cases as nf

pytestmark = pytest.mark.gpu
X_ONLY = ("f", "grad", "g", "J", "Jc", "Jcsr")      # what a multiplier must not change
SENTINEL = -7.25e77                                   # finite: an unwritten slot cannot pass as "non-finite"


class World:
    """One case: its system and evaluator, its reference, its poisons, and the references at the poisoned points (computed
    once, shared by the routes)."""

    def __init__(self, case):
        self.case = case
        self.system, _, self.guess = nf.build(case, "pockit_amd")
        self.ev, self.plan = self.system.evaluator, self.system.plan
        self.plan.jacc  # noqa: B018  (builds the compact plans)
        self.oracle = nf.build(case, "oracle")[0] if case.reference == "oracle" else None
        if self.oracle is not None:
            self.ref_j, self.ref_h = self.oracle.jacobianstructure(), self.oracle.hessianstructure()
            for a, b in zip(self.system.jacobianstructure() + self.system.hessianstructure(), self.ref_j + self.ref_h):
                assert np.array_equal(a, b), "structure"
        self.poisons = nf.poisons(self.system, tiles=self.ev.tables.tiles, inf=case.inf)
        self._want = {}

    def want(self, poison=None, scale=None):
        key = (None if poison is None else poison.label, scale)
        if key not in self._want:
            x, lam, sigma = nf.inputs(self.system, self.guess, poison)
            if scale is not None:
                x = x * scale
            if self.oracle is not None:
                res = nf.reference(self.oracle, x, lam, sigma)
            else:
                from plan_interp import Interp

                it = Interp(self.plan, x, lam, sigma)
                res = nf.reference(lambda *_: it, x, lam, sigma)
                with np.errstate(all="ignore"):
                    res["Jc"], res["Hc"] = it.jacobian_compact(), it.hessian_compact()
            self._want[key] = res
        return self._want[key]

    def hold(self, key, got, want, tag):
        """One array of a route against the reference."""
        plan, what = self.plan, f"{tag} [{key}]"
        if key in nf.NAMES:
            nf.compare(got, want[key], what)
        elif key in ("Jcsr", "Hcsr"):
            m = self.ev.csr_map("jac" if key == "Jcsr" else "hess")
            with np.errstate(all="ignore"):
                nf.compare(got, m.gather(want[key[0]]), what)      # the host gather of the reference's values
        elif self.oracle is None:
            nf.compare(got, want[key], what)
        elif key == "Jc":
            nf.compare_matrix(got, (plan.jacc_row, plan.jacc_col), want["J"], self.ref_j, (plan.m, plan.n), what)
        else:
            nf.compare_matrix(got, (plan.hessc_row, plan.hessc_col), want["H"], self.ref_h, (plan.n, plan.n), what)


# ------------------------------------------------------------------------------------------------ the routes
def _arrays(names, vals):
    return {k: np.array(v, dtype=np.float64) for k, v in zip(names, vals)}      # (copies: the callbacks recycle their buffers)


def route_callbacks(w, x, lam, sigma):
    s = w.system
    return _arrays(nf.NAMES, (s.objective(x), s.gradient(x), s.constraints(x), s.jacobian(x), s.hessian(x, lam, sigma)))


def route_cycle(w, x, lam, sigma):
    return _arrays(nf.NAMES, w.ev.cycle(x, lam, sigma))


def route_direct(w, x, lam, sigma):
    ev = w.ev
    return _arrays(nf.NAMES, (ev.objective_direct(x), ev.gradient_direct(x), ev.constraints_direct(x), ev.jacobian_direct(x),
                              ev.hessian_direct(x, lam, sigma)))


def route_compact(w, x, lam, sigma):
    out = {}
    if w.ev.src.compact_j:
        out["Jc"] = np.array(w.ev.jacobian_compact(x))
    if w.ev.src.compact:
        out["Hc"] = np.array(w.ev.hessian_compact(x, lam, sigma))
    return out


def route_cyclec(w, x, lam, sigma):
    """pk_cyclec: the compact layouts out of the single launch, into buffers preset to a finite sentinel."""
    import torch

    ev, plan = w.ev, w.plan
    if not (ev.src.compact and ev.src.compact_j and ev._one_launch_cycle()) or ev.src.big:
        return {}      # (the compact layouts ride in the single-launch cycle only: the library answers error 69 otherwise)
    dev = torch.device("cuda", 0)
    dx, dlam = torch.from_numpy(x).to(dev), torch.from_numpy(lam).to(dev)
    sizes = (("f", 1), ("grad", plan.n), ("g", plan.m), ("Jc", plan.nnz_Jc), ("Hc", plan.nnz_Hc))
    o = {k: torch.full((max(n, 1),), SENTINEL, dtype=torch.float64, device=dev) for k, n in sizes}
    ev.set_cycle_layout(True, True)
    try:
        torch.cuda.synchronize()
        ev.cycle_dev(dx.data_ptr(), dlam.data_ptr(), sigma, *[o[k].data_ptr() for k, _ in sizes])
        ev.sync()
    finally:
        ev.set_cycle_layout(False, False)
    out = {k: o[k].cpu().numpy()[:n].copy() for k, n in sizes}
    out["f"] = out["f"][0]
    assert nf.same_bits(dx.cpu().numpy(), x) and nf.same_bits(dlam.cpu().numpy(), lam), "the device copies of x and lam must not be written"
    for k, v in out.items():
        assert not np.any(v == SENTINEL), f"pk_cyclec left entries of {k} unwritten"
    return out


def route_csr(w, x, lam, sigma):
    return {"Jcsr": np.array(w.ev.jacobian_csr(x)), "Hcsr": np.array(w.ev.hessian_csr(x, lam, sigma))}


ROUTES = {"callbacks": route_callbacks, "cycle": route_cycle, "direct": route_direct, "compact": route_compact,
          "cyclec": route_cyclec, "csr": route_csr}


@pytest.fixture(scope="module", params=nf.CASES, ids=nf.CASE_IDS)
def world(request):
    with nf.switches(request.param):      # (the switches stay set while the case's evaluator lives: its batched object compiles late)
        w = World(request.param)
        try:
            yield w
        finally:
            w.system._invalidate()


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_route_matches_the_reference_at_every_poisoned_point(world, route):
    w, run = world, ROUTES[route]
    x, lam, sigma = nf.inputs(w.system, w.guess)
    clean = run(w, x, lam, sigma)
    if not clean:
        assert route in ("compact", "cyclec"), "every other route exists for every model"
        return      # (the model has no such route: src.compact / src.compact_j / a cycle that is not one launch)
    for key, got in clean.items():
        w.hold(key, got, w.want(), f"{w.case.id}, clean point, {route}")
        assert np.isfinite(got).all()
    local = []
    for poison in w.poisons:
        px, plam, _ = nf.inputs(w.system, w.guess, poison)
        x0, lam0 = px.copy(), plam.copy()
        tag = f"{w.case.id}, {poison.label}, {route}"
        got = run(w, px, plam, sigma)
        assert nf.same_bits(px, x0) and nf.same_bits(plam, lam0), tag + ": x and lam must not be written"
        want = w.want(poison)
        for key, a in got.items():
            w.hold(key, a, want, tag)
            if poison.kind == "dictated" or (poison.kind == "lam" and key in X_ONLY):
                assert nf.same_bits(a, clean[key]), f"{tag} [{key}]: must be the clean bits"
        again = run(w, x, lam, sigma)
        for key, a in again.items():
            assert nf.same_bits(a, clean[key]), f"{tag} [{key}]: the clean point afterwards differs from the clean point before"
        if poison.kind == "node" and set(nf.NAMES) <= set(got):
            assert nf.is_local(got), f"{tag}: the damage of one node must be local, got {nf.nonfinite_counts(got)}"
            local.append(poison.label)
    if set(nf.NAMES) <= set(clean):
        assert local, "no poison of this case has a local effect: the case is vacuous"


def test_a_poisoned_entry_in_the_middle_of_a_batch(world):
    """cycle_batch with B = 3 and the poisoned point in the middle: entries 0 and 2 are bit for bit their clean single cycles,
    entry 1 is held to the reference."""
    w = world
    x, lam, sigma = nf.inputs(w.system, w.guess)
    x2 = x * (1.0 + 1.0e-3)
    single0 = route_cycle(w, x, lam, sigma)
    single2 = route_cycle(w, x2, lam, sigma)
    for key in nf.NAMES:
        w.hold(key, single2[key], w.want(None, 1.0 + 1.0e-3), f"{w.case.id}, second clean point, cycle")
    for poison in w.poisons:
        px, plam, _ = nf.inputs(w.system, w.guess, poison)
        X, Lam = np.stack([x, px, x2]), np.stack([lam, plam, lam])
        X0, Lam0 = X.copy(), Lam.copy()
        out = dict(zip(nf.NAMES, w.ev.cycle_batch(X, Lam, sigma)))
        assert nf.same_bits(X, X0) and nf.same_bits(Lam, Lam0), "X and Lam must not be written"
        tag = f"{w.case.id}, {poison.label}, cycle_batch"
        for key in nf.NAMES:
            assert nf.same_bits(out[key][0], single0[key]), f"{tag} [{key}]: entry 0 differs from its clean single cycle"
            assert nf.same_bits(out[key][2], single2[key]), f"{tag} [{key}]: entry 2 differs from its clean single cycle"
            w.hold(key, out[key][1], w.want(poison), tag + ", entry 1")
