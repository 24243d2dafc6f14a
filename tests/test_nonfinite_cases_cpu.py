"""Non-finite iterates, CPU tier: the two references of tests/test_gpu_nonfinite.py against each other, and the comparison
itself against planted mistakes (tests/nonfinite_cases.py).

For every case and every poison the oracle and the NumPy execution of the product's plan (tests/plan_interp.py) must agree by
``compare``: the same non-finite entries in f, grad f, g, J and H -- with nothing left out -- and the project's 1e-11 on the
finite ones.  The NaN mask is a property of the mathematics (a product with a NaN factor is NaN whatever form the derivative is
printed in); the mask of +-inf depends on the printed form (inf - inf, 0 * inf), so an Inf poison belongs to a case only where
both references agree on every entry:

* ``elementary_functions_model`` (both schemes) has no Inf poison: oracle and plan print different forms of the same
  derivatives and 4-5 entries of J and of H are finite in one and not in the other.
* ``planar_quadrotor`` with fastmath has none: the flags permit the device to differ at infinity.
* every other case keeps its Inf poisons and this module holds them to equality of the masks.

The workgroup-wide case (intervals of 100 and 65 points) has the plan interpreter as its only reference: the oracle's
np.roots-based tables cannot be built at that order (numpy.linalg.LinAlgError), so there is no oracle mask to compare with; the
side conditions and the locality of the damage are still asserted on the interpreter's result."""
import numpy as np
import pytest

import nonfinite_cases as nf
from plan_interp import Interp

_WORLD = {}


def _world(case):
    key = nf.plan_key(case)
    if key not in _WORLD:
        system, _, guess = nf.build(case, "pockit_amd")
        plan = system.plan
        interp = lambda x, lam, sigma: Interp(plan, x, lam, sigma)  # noqa: E731
        ref = nf.build(case, "oracle")[0] if case.reference == "oracle" else None
        x, lam, sigma = nf.inputs(system, guess)
        clean = {"interp": nf.reference(interp, x, lam, sigma)}
        if ref is not None:
            clean["oracle"] = nf.reference(ref, x, lam, sigma)
        for res in clean.values():
            assert all(np.isfinite(res[name]).all() for name in nf.NAMES), "the clean point must be finite"
        _WORLD[key] = (system, guess, ref, interp, clean)
    return _WORLD[key]


def _poisons(case, system):
    with nf.switches(case):
        return nf.poisons(system, inf=case.inf)


@pytest.mark.parametrize("case", [c for c in nf.CASES if not c.slow], ids=lambda c: c.id)
def test_oracle_and_plan_agree_at_every_poisoned_point(case):
    system, guess, ref, interp, clean = _world(case)
    poisons = _poisons(case, system)
    kinds = {p.kind for p in poisons}
    assert "node" in kinds and "lam" in kinds and any(p.which == "x" and p.kind == "dictated" for p in poisons), kinds
    for poison in poisons:
        x, lam, sigma = nf.inputs(system, guess, poison)
        x0, lam0 = x.copy(), lam.copy()
        tag = f"{case.id}, {poison.label}"
        got = nf.reference(interp, x, lam, sigma)
        if ref is not None:
            want = nf.reference(ref, x, lam, sigma)
            nf.check_result(got, want, tag + ": plan against oracle")
            nf.side_conditions(poison, want, clean["oracle"], tag + " (oracle)")
        nf.side_conditions(poison, got, clean["interp"], tag + " (plan)")
        assert nf.same_bits(x, x0) and nf.same_bits(lam, lam0), tag + ": x and lam must not be written"
        if poison.kind == "node":
            assert nf.is_local(got), f"{tag}: the damage of one node must be local, got {nf.nonfinite_counts(got)}"
        if poison.kind in ("node", "tf", "static") and np.isnan(poison.value):
            assert not all(np.isfinite(got[name]).all() for name in nf.NAMES), tag + ": the case is vacuous"


def _mutant_material():
    for case in nf.CASES:
        if case.id in ("brach-lgr-37x5-ipw3", "brach-lgl-23x6-ipw3", "rocket-lgr-40x3-ipw64"):
            system, guess, ref, _, clean = _world(case)
            for poison in _poisons(case, system):
                if poison.kind == "node" and np.isnan(poison.value):
                    x, lam, sigma = nf.inputs(system, guess, poison)
                    yield case, poison, system, nf.reference(ref, x, lam, sigma), clean["oracle"]


@pytest.mark.parametrize("name", sorted(nf.MUTANTS))
def test_every_planted_mistake_is_caught_and_the_array_named(name):
    planted = 0
    for case, poison, system, res, clean in _mutant_material():
        nf.check_result(res, res, "a correct result passes")
        made = nf.MUTANTS[name](system, res, clean)
        if made is None:
            continue
        mutated, array = made
        planted += 1
        with pytest.raises(AssertionError) as err:
            nf.check_result(mutated, res, f"{case.id}, {poison.label}, mutant {name}")
        assert f"[{array}]" in str(err.value), str(err.value)
    assert planted >= 3, f"mutant {name} found nothing to be planted in"


def test_compare_rejects_what_it_must():
    nan, inf = np.nan, np.inf
    nf.compare([1.0, nan, 3.0], [1.0, inf, 3.0], "NaN against Inf inside the non-finite set is not compared")
    nf.compare([1.0 + 5e-12, nan], [1.0, nan], "within the tolerance")
    nf.compare([1.0e6 + 5e-6, nan], [1.0e6, -inf], "the tolerance scales with the largest finite entry")
    for got, want in (([1.0, 2.0], [1.0, nan]), ([nan, 2.0], [1.0, 2.0]), ([1.0, nan], [nan, 1.0]), ([1.0 + 2e-11, nan], [1.0, nan]),
                      ([1.0, 2.0, 3.0], [1.0, 2.0]), ([0.0], [inf])):
        with pytest.raises(AssertionError):
            nf.compare(got, want, "must fail")
    # scatter-added layouts: a non-finite triplet makes its position non-finite, a missing position counts as zero
    nf.compare_matrix([1.0, 2.0, nan], ([0, 0, 1], [0, 0, 1]), [3.0, inf], ([0, 1], [0, 1]), (2, 2), "coalesced")
    nf.compare_matrix([3.0, 0.0], ([0, 1], [0, 0]), [3.0], ([0], [0]), (2, 2), "an explicit zero")
    with pytest.raises(AssertionError):
        nf.compare_matrix([1.0, 2.0, 4.0], ([0, 0, 1], [0, 0, 1]), [3.0, inf], ([0, 1], [0, 1]), (2, 2), "hidden")
    with pytest.raises(AssertionError):
        nf.compare_matrix([3.0, nan], ([0, 1], [0, 0]), [3.0], ([0], [0]), (2, 2), "leaked")


def test_the_interpreter_still_insists_on_a_complete_plan():
    """The NaN sentinel of ``Interp._run`` became a mask of written slots: a plan that misses a slot must still be refused,
    and a NaN the model produces must not be taken for a hole."""
    case = next(c for c in nf.CASES if c.id == "brach-lgr-37x5-ipw3")
    system, guess, _, interp, _ = _world(case)
    x, lam, sigma = nf.inputs(system, guess)
    it = interp(x, lam, sigma)
    with pytest.raises(AssertionError, match="does not cover every output slot"):
        it._run(system.plan.jac, system.plan.nnz_J + 1, False)
    poison = next(p for p in _poisons(case, system) if p.kind == "node")
    x, lam, sigma = nf.inputs(system, guess, poison)
    assert np.isnan(interp(x, lam, sigma).jacobian()).any()
