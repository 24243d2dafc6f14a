"""Non-finite iterates (TEST INFRASTRUCTURE, no GPU): the cases, the poisoned slots, the comparison and the planted mistakes
shared by tests/test_nonfinite_cases_cpu.py (oracle against the NumPy execution of the plan) and tests/test_gpu_nonfinite.py
(every kernel route against the oracle).

The interior-point solver steers by non-finite values (a trial point whose f, grad f or J is not finite is rejected), so WHERE
a NaN of the iterate shows in f, grad f, g, J and H is part of what the kernels compute.  The rule of ``compare``: the set of
non-finite entries must be the reference's exactly; on the finite entries the project's tolerance holds
(|a - b| <= 1e-11 * max(1, max|b|)).  NaN against Inf inside the non-finite set is not compared:
fused multiply-add contraction and the fastmath reassociation may turn one into the other.

A poison is ``(label, "x" | "lam", index, value, kind)``; ``kind`` is one of "dictated" (a slot the transcription
overwrites: nothing may change), "node" (a state or control value at one node: the damage is local), "tf", "static",
"lam" (a multiplier: only H may change)."""
import importlib
import os
from collections import namedtuple

import numpy as np

import models

TOL = 1e-11
NAMES = ("f", "grad", "g", "J", "H")
Poison = namedtuple("Poison", "label which index value kind")
Case = namedtuple("Case", "id model scheme kw env inf reference slow")


def _case(id, model, scheme, kw, env=None, inf=True, reference="oracle", slow=False):
    return Case(id, model, scheme, kw, dict(env or {}), inf, reference, slow)


# The generated source does not depend on the mesh: every case reuses a code object another GPU test builds.
# "inf": +inf and -inf are poison values too (only where oracle and plan print forms that agree at infinity, measured by
# tests/test_nonfinite_cases_cpu.py).  "reference": whose values and mask the device is held to.
_BIG = dict(mesh=[0, 0.2, 0.5, 0.7, 1.0], num_point=[6, 100, 8, 65])
CASES = (
    [_case(f"brach-lgr-37x5-ipw{w}", "brachistochrone", "radau", dict(mesh=37, num_point=5), {"POCKIT_AMD_IPW": str(w)}) for w in (1, 3, 64)]
    + [_case(f"brach-lgl-23x6-ipw{w}", "brachistochrone", "lobatto", dict(mesh=23, num_point=6), {"POCKIT_AMD_IPW": str(w)}) for w in (1, 3, 64)]
    + [_case("brach-lgr-37x5-groups2", "brachistochrone", "radau", dict(mesh=37, num_point=5), {"POCKIT_AMD_GROUP_CAP": "2"}),
       _case("brach-lgr-13x12", "brachistochrone", "radau", dict(mesh=13, num_point=12)),
       _case("brach-lgr-13x12-tabcap64", "brachistochrone", "radau", dict(mesh=13, num_point=12), {"POCKIT_AMD_TAB_CAP": "64"}),
       # intervals of 100 and 65 points, a workgroup each: the oracle's np.roots tables cannot even be built at these orders
       # (numpy.linalg.LinAlgError in oracle/tables.py at K = 100), so values AND mask come from the plan interpreter
       _case("brach-lgr-workgroup-wide", "brachistochrone", "radau", _BIG, reference="interp"),
       _case("rocket-lgr-40x3-ipw64", "two_stage_rocket", "radau", dict(mesh=40, num_point=3), {"POCKIT_AMD_IPW": "64"}),
       _case("quadrotor-lgl-19x4-fastmath", "planar_quadrotor", "lobatto", dict(mesh=19, num_point=4, fastmath=True), inf=False),
       _case("humanoid-lgr-9x7", "humanoid_wbc", "radau", dict(mesh=9, num_point=7), slow=True),
       _case("func-times-lgr", "func_times_model", "radau", {}),
       _case("derivative-lgr", "derivative_model", "radau", {}),
       _case("elementary-lgr", "elementary_functions_model", "radau", {}, inf=False),      # (forms differ at infinity)
       _case("elementary-lgl", "elementary_functions_model", "lobatto", {}, inf=False),
       _case("chain52-lgr-40x4", "state_chain", "radau", dict(states=52, mesh=40, num_point=4))])
CASE_IDS = [c.id for c in CASES]


def namespace(scheme, pkg):
    return importlib.import_module(f"{pkg}.{scheme}")


def build(case, pkg):
    """(system, phases, guess) of the case in ``pkg`` ("pockit_amd" or "oracle")."""
    return getattr(models, case.model)(namespace(case.scheme, pkg), **case.kw)


def plan_key(case):
    """Cases that differ only in a device switch share one plan, one oracle and one set of CPU references."""
    return (case.model, case.scheme, repr(sorted(case.kw.items())))


# ------------------------------------------------------------------------------------------------ the comparison
def compare(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    fg, fw = np.isfinite(got), np.isfinite(want)
    if not np.array_equal(fg, fw):
        leak, hide = np.flatnonzero((~fg & fw).ravel()), np.flatnonzero((fg & ~fw).ravel())
        raise AssertionError(f"{what}: the non-finite sets differ -- {leak.size} entries non-finite only here (first {leak[:5].tolist()}), "
                             f"{hide.size} finite only here (first {hide[:5].tolist()}); the reference has {int((~fw).sum())} of {fw.size}")
    if fw.any():
        err = np.max(np.abs(got[fw] - want[fw]))
        assert err <= TOL * max(1.0, np.max(np.abs(want[fw]))), f"{what}: err {err:.3e} on the finite entries"


def coalesce(vals, rc, shape):
    """Scatter-add of triplets: (sorted linear positions, sums).  A non-finite triplet makes its position non-finite."""
    key = np.asarray(rc[0], dtype=np.int64) * int(shape[1]) + np.asarray(rc[1], dtype=np.int64)
    pos, inv = np.unique(key, return_inverse=True)
    out = np.zeros(len(pos))
    with np.errstate(invalid="ignore"):
        np.add.at(out, inv, np.asarray(vals, dtype=np.float64))
    return pos, out


def compare_matrix(got, rc, want, rc_ref, shape, what):
    """A compact layout against the reference layout: both scatter-added, positions absent on one side count as 0.0."""
    pa, a = coalesce(got, rc, shape)
    pb, b = coalesce(want, rc_ref, shape)
    pos = np.union1d(pa, pb)
    A, B = np.zeros(len(pos)), np.zeros(len(pos))
    A[np.searchsorted(pos, pa)] = a
    B[np.searchsorted(pos, pb)] = b
    compare(A, B, what)


def check_result(got, want, tag):
    """The five arrays (dicts by NAMES); the message names the array in brackets."""
    for name in NAMES:
        compare(got[name], want[name], f"{tag} [{name}]")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64).reshape(-1), np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def side_conditions(poison, got, clean, tag):
    """A dictated slot changes nothing, a multiplier only H -- bit for bit against the clean evaluation on the same route."""
    if poison.kind == "dictated":
        for name in NAMES:
            assert same_bits(got[name], clean[name]), f"{tag} [{name}]: a dictated slot ({poison.label}) changed the result"
    if poison.kind == "lam":
        for name in NAMES[:4]:
            assert same_bits(got[name], clean[name]), f"{tag} [{name}]: a multiplier ({poison.label}) changed an x-only result"


def nonfinite_counts(res):
    return {name: (int((~np.isfinite(np.asarray(res[name]))).sum()), int(np.asarray(res[name]).size)) for name in NAMES}


def is_local(res):
    """At least one of g, J, H has a non-finite set that is neither empty nor everything."""
    return any(0 < bad < size for bad, size in (nonfinite_counts(res)[name] for name in ("g", "J", "H")))


# ------------------------------------------------------------------------------------------------ the poisoned slots
def default_tiles(plan):
    """The tile records an evaluator of this plan would use (no device needed: generated source + tables)."""
    from pockit_amd.codegen import ModelSource
    from pockit_amd.evaluator import Tables

    return Tables(plan, ModelSource(plan)).tiles


def _nonlinear_first(exprs, syms):
    """Index of the first symbol some expression is nonlinear in, else of the first one any expression reads; None."""
    import sympy as sp

    reads = [i for i, s in enumerate(syms) if any(s in sp.sympify(e).free_symbols for e in exprs)]
    for i in reads:
        if any(sp.diff(sp.sympify(e), syms[i]).free_symbols for e in exprs):
            return i, True
    return (reads[0], False) if reads else (None, False)


def _nonlinear_function(exprs):
    """Index of the first expression with a second derivative that is not identically zero, else 0; None without any."""
    import sympy as sp

    for i, e in enumerate(exprs):
        e = sp.sympify(e)
        if any(sp.diff(e, s).free_symbols for s in sorted(e.free_symbols, key=str)):
            return i
    return 0 if exprs else None


def poisons(system, tiles=None, inf=True):
    """The poisons of a model, derived from the plan's layout and the tile records (``evaluator.tables.tiles``)."""
    from pockit_amd.model import FREE
    from pockit_amd.optimizer._common import dictated_slots

    plan = system.plan
    tiles = default_tiles(plan) if tiles is None else tiles
    fixed_at, _, func = dictated_slots(system)
    dictated = set(int(i) for i in fixed_at) | set(int(i) for i, _, _ in func)
    out, seen = [], set()

    def add(label, which, index, kind):
        index = int(index)
        if (which, index) in seen or (which == "x" and kind != "dictated" and index in dictated):
            return
        seen.add((which, index))
        out.append((label, which, index, kind))

    for k, pp in enumerate(plan.phase_plans):
        p, lay, base = pp.phase, pp.layout, int(plan.l_p[k])
        lo, hi = base, int(plan.r_p[k])
        mine = [int(i) for i in fixed_at if lo <= i < hi]
        if mine:
            add(f"p{k} fixed slot", "x", mine[0], "dictated")
        mine = [int(i) for i, _, _ in func if lo <= i < hi]
        if mine:
            add(f"p{k} slot dictated by the static parameters", "x", mine[0], "dictated")
        exprs = [f.expr for f in p.F_d]
        i, nonlinear = _nonlinear_first(exprs, list(p.x))
        K, lm, N = [int(v) for v in lay.K], [int(v) for v in lay.lm], int(lay.N)
        if i is not None:
            kind = "node" if nonlinear else "linear node"
            at = lambda q: base + int(lay.l_v[i]) + int(q)  # noqa: E731
            add(f"p{k} state {i} first free node", "x", at(0 if p.info_bc_0[i].t == FREE else 1), kind)
            j = min(1, N - 1)
            add(f"p{k} state {i} interior node of interval {j}", "x", at(lm[j] + K[j] // 2), kind)
            add(f"p{k} state {i} last node of interval {j}", "x", at(lm[j] + K[j] - 1), kind)
            if j + 1 < N:
                add(f"p{k} state {i} first node of interval {j + 1}", "x", at(lm[j + 1]), kind)
                add(f"p{k} state {i} second node of interval {j + 1}", "x", at(lm[j + 1] + 1), kind)
            add(f"p{k} state {i} node of the last interval", "x", at(lm[N - 1] + (K[N - 1] - 1) // 2), kind)
            pos = [t for t in range(len(tiles)) if int(tiles[t]["phase"]) == k and int(tiles[t]["nj"]) > 0]
            inner = [t for t in pos if int(tiles[t]["j0"]) > 0]
            if inner:
                t = inner[len(inner) // 2]                       # a boundary between two tiles in the middle of the phase
                q = lm[int(tiles[t]["j0"])]
                add(f"p{k} state {i} last node before tile {t}", "x", at(q - 1), kind)
                add(f"p{k} state {i} first node of tile {t}", "x", at(q), kind)
            wg = [t for t in inner if t % 4 == 0]                # a tile that opens a workgroup (4 tile records each)
            if wg:
                q = lm[int(tiles[wg[0]]["j0"])]
                add(f"p{k} state {i} last node before the workgroup of tile {wg[0]}", "x", at(q - 1), kind)
                add(f"p{k} state {i} first node of the workgroup of tile {wg[0]}", "x", at(q), kind)
        if p.n_u:
            c, nonlinear = _nonlinear_first(exprs + [f.expr for f in p.F_c] + [f.expr for f in p.F_I], list(p.u))
            if c is not None:
                j = N // 2
                add(f"p{k} control {c} in interval {j}", "x", base + int(lay.l_v[p.n_x + c]) + lm[j] + K[j] // 2,
                    "node" if nonlinear else "linear node")
        if p.info_t_f.t == FREE:
            add(f"p{k} t_f", "x", base + int(lay.L) - 1, "tf")
        j = N // 2                                               # multipliers: a defect row and a path row of a middle interval
        d = _nonlinear_function(exprs)                           # (of a state whose dynamics have second derivatives: H reads it)
        if d is not None:
            add(f"p{k} multiplier of a defect row of state {d}", "lam", int(plan.g_off[k]) + int(lay.l_d[d]) + int(lay.ld[j]), "lam")
        if p.n_c:
            add(f"p{k} multiplier of a path row", "lam", int(plan.path_off[k]) + lm[j] + K[j] // 2, "lam")
    if plan.n_s:
        add("static parameter 0", "x", plan.l_s, "static")
    if plan.n_sys:
        add("multiplier of system constraint 0", "lam", 0, "lam")
    values = (np.nan, np.inf, -np.inf) if inf else (np.nan,)
    return [Poison(f"{label} = {v}", which, index, v, kind) for v in values for label, which, index, kind in out]


def inputs(system, guess, poison=None):
    """(x, lam, sigma) of SURVEY.md section 8(d), with the poison applied to a copy."""
    x, lam, sigma = models.bench_inputs(system, guess)
    x, lam = x.copy(), lam.copy()
    if poison is not None:
        (x if poison.which == "x" else lam)[poison.index] = poison.value
    return x, lam, sigma


def reference(ref, x, lam, sigma):
    """The five arrays of an oracle system or of a plan interpreter factory (``lambda x, lam, sigma: Interp(...)``)."""
    with np.errstate(all="ignore"):
        if callable(ref):
            it = ref(x, lam, sigma)
            vals = (it.objective(), it.gradient(), it.constraints(), it.jacobian(), it.hessian())
        else:
            vals = (ref.objective(x), ref.gradient(x), ref.constraints(x), ref.jacobian(x), ref.hessian(x, lam, sigma))
    return {name: np.array(v, dtype=np.float64) for name, v in zip(NAMES, vals)}


class switches:
    """The case's environment switches, set for the construction of its evaluator and restored afterwards."""

    def __init__(self, case):
        self.env, self.keep = case.env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.keep[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------ planted mistakes
def _defect_blocks(system, res):
    """[(rows of interval j, rows of interval j + 1)] of g where the first block is non-finite throughout and the second
    finite throughout (defect rows of one state)."""
    plan, bad = system.plan, ~np.isfinite(res["g"])
    for k, pp in enumerate(plan.phase_plans):
        lay = pp.layout
        for i in range(pp.nx):
            r0 = int(plan.g_off[k]) + int(lay.l_d[i])
            for j in range(int(lay.N) - 1):
                a = r0 + int(lay.ld[j]) + np.arange(int(lay.R[j]))
                b = r0 + int(lay.ld[j + 1]) + np.arange(int(lay.R[j + 1]))
                if bad[a].all() and not bad[b].any():
                    yield a, b


def _copy(res):
    return {k: np.array(v, dtype=np.float64) for k, v in res.items()}


def _mutant_leak(system, res, clean):
    for _, b in _defect_blocks(system, res):
        out = _copy(res)
        out["g"][b[0]] = np.nan                      # NaN in a row of the neighbouring interval
        return out, "g"
    return None


def _mutant_hide(system, res, clean):
    bad = np.flatnonzero(~np.isfinite(res["J"]))
    if not bad.size:
        return None
    out = _copy(res)
    out["J"][bad[len(bad) // 2]] = 0.0
    return out, "J"


def _mutant_hide_all_but_one(system, res, clean):
    bad = np.flatnonzero(~np.isfinite(res["H"]))
    if bad.size < 2:
        return None
    out = _copy(res)
    out["H"][bad[1:]] = 0.0
    return out, "H"


def _mutant_small_wrong(system, res, clean):
    fin = np.flatnonzero(np.isfinite(res["J"]))
    if not fin.size or fin.size == res["J"].size:      # (planted at a poisoned point: beside a non-finite set)
        return None
    out = _copy(res)
    out["J"][fin[len(fin) // 2]] += 1e-9 * max(1.0, np.max(np.abs(res["J"][fin])))
    return out, "J"


def _mutant_shifted(system, res, clean):
    for a, b in _defect_blocks(system, res):
        out = _copy(res)
        out["g"][a] = clean["g"][a]                  # the non-finite block of interval j sits on interval j + 1 instead
        out["g"][b] = np.nan
        return out, "g"
    return None


#: name -> f(system, poisoned result, clean result) -> (mutated result, name of the array it touched), or None where the
#: result has nothing to plant the mistake in.  Applied to a CORRECT result; ``check_result`` must then fail and name the array.
MUTANTS = {"leak": _mutant_leak, "hide": _mutant_hide, "hide_all_but_one": _mutant_hide_all_but_one,
           "small_wrong": _mutant_small_wrong, "shifted": _mutant_shifted}
