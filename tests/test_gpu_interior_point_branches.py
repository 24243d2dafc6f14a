"""``pockit_amd.optimizer.interior_point.solve`` on the device, held to the branches that the benchmark models never take.  The
models are those of tests/ipm_models.py; their references stand on their own in tests/test_ipm_models_cpu.py.  Every solve runs
with ``tol = 1e-8`` and ``max_iter = 200`` (the failing ones say otherwise), closes its evaluator and asserts no iteration count.

* Convex models take no regularisation: lqr(lobatto, 6, 6), the path-constrained LQR (Radau 5 x 4) and the LQR with the variable
  bound ``u >= -1`` (Lobatto 6 x 6, Radau 5 x 4), ``"direct"`` and ``"banded"``: status 0, converged by ``_converged`` of
  tests/test_gpu_interior_point.py, ``regularisations == 0``.  (A solver that leaves the dictated slots of the NLP vector free
  has an empty row and column per slot in its step matrix and regularises every iteration.)  The bounded LQR lies within 1e-6 of
  SLSQP on the oracle and more than 1e-2 above the unbounded optimum, with a control on its bound and a multiplier there.
* A saddle is left by regularising: ``double_well``, both schemes, ``"direct"`` and ``"banded"`` with ``band_attempts`` 1, 3 and 8.
  The start's Newton step has negative curvature and lands on the saddle ``x = 0`` (f = 0), a KKT point that ``_converged`` alone
  would accept; the solver must end in a well instead: ``regularisations > 0``, f < -2 and within 1e-6 of SLSQP, ``max |x| > 0.5``.
  The three banded runs are bit-equal: here the batched walk takes candidates behind the first for a numerical reason.
* A trial point outside the model's domain is rejected, not adopted: ``sqrt_well``, ``"direct"``.  The full Newton step from the
  guess is NaN and the half step lies on the edge of the domain (f finite without a decrease, grad f infinite): status 0,
  ``|f + 1| <= 1e-7``, every state positive, and ``trial_lengths`` was asked for lengths behind the first.
* The failure statuses: a start outside the domain is status -13 with zero iterations and the start in ``info["x"]``; a problem
  without a feasible point ends with -1 or -2 within 60 iterations, a finite x and ``error > tol``.  Neither raises.
"""
import functools

import numpy as np
import pytest

import ipm_models as im
import models
import sparse_cases as sc
from test_gpu_interior_point import TOL, _converged, _ns, _slsqp, constrained_lqr, dictated

pytestmark = pytest.mark.gpu


def _lqr(ns, mesh, num_point):
    system, (phase,), _ = models.lqr(ns, mesh, num_point)
    return system, [phase], [ns.constant_guess(phase, 0.0), [0.0]]


@functools.lru_cache(maxsize=None)
def _reference(builder, scheme, *args):
    """SLSQP on the oracle from the builder's guess, once per model: ``(the oracle system, f)``."""
    ref, _, guess = builder(_ns(scheme, "oracle"), *args)
    return ref, float(_slsqp(ref, models.pack_guess(ref, guess)).fun)


def _solve(system, guess, options=None, **kw):
    from pockit_amd.optimizer import interior_point

    try:
        return interior_point.solve(system, guess, {"tol": TOL, "max_iter": 200, **(options or {})}, **kw)
    finally:
        system.evaluator.close()


def _report(what, info):
    print(f"{what}: status {info['status']}, {info['iterations']} iterations, {info['regularisations']} regularisations, f = {info['obj_val']!r}, mu {info['mu']:.1e}")


CONVEX = [(_lqr, "lobatto", (6, 6)), (constrained_lqr, "radau", (5, 4)), (im.bounded_lqr, "lobatto", (6, 6)), (im.bounded_lqr, "radau", (5, 4))]


@pytest.mark.parametrize("linear_solver", ("direct", "banded"))
@pytest.mark.parametrize("builder,scheme,args", CONVEX, ids=[f"{b.__name__.strip('_')}-{s}-{'x'.join(map(str, a))}" for b, s, a in CONVEX])
def test_a_convex_model_takes_no_regularisation(builder, scheme, args, linear_solver):
    system, _, guess = builder(_ns(scheme, "pockit_amd"), *args)
    _, info = _solve(system, guess, linear_solver=linear_solver)
    _report(f"{builder.__name__.strip('_')}({scheme}, {args}), {linear_solver}", info)
    ref = builder(_ns(scheme, "oracle"), *args)[0]
    _converged(ref, info, dictated=dictated(system))
    assert info["regularisations"] == 0
    if builder is im.bounded_lqr:
        _, optimum = _reference(builder, scheme, *args)
        assert abs(optimum - im.BOUNDED_LQR_OPTIMUM[(scheme, *args)]) <= 1e-9
        print(f"interior point {info['obj_val']!r}, SLSQP {optimum!r}, difference {abs(info['obj_val'] - optimum):.2e}")
        assert abs(info["obj_val"] - optimum) <= 1e-6
        x, bounded = info["x"], np.asarray(ref.v_lb, dtype=np.float64) == -1.0
        assert int(bounded.sum()) == im.BOUNDED_LQR_ACTIVE[(scheme, *args)][1]
        active = bounded & (x + 1.0 <= 1e-6)
        assert active.any(), "no control is on its bound at the solution"
        assert np.any(info["mult_x_L"][active] > 1e-3), info["mult_x_L"][active]
        assert not info["mult_x_U"].any()
        assert info["obj_val"] - im.UNBOUNDED_LQR_OPTIMUM > 1e-2


@pytest.mark.parametrize("scheme", ("radau", "lobatto"))
def test_a_saddle_is_left_by_regularising(scheme):
    ref, optimum = _reference(im.double_well, scheme)
    assert abs(optimum - im.DOUBLE_WELL_OPTIMUM[scheme, 4, 5]) <= 1e-9
    runs = {}
    for name, kw in (("direct", dict(linear_solver="direct")), (1, dict(linear_solver="banded", band_attempts=1)),
                     (3, dict(linear_solver="banded", band_attempts=3)), (8, dict(linear_solver="banded", band_attempts=8))):
        system, _, guess = im.double_well(_ns(scheme, "pockit_amd"))
        (var,), info = _solve(system, guess, **kw)
        _report(f"double_well({scheme}), {name}", info)
        _converged(ref, info, dictated=dictated(system))
        assert info["obj_val"] < -2.0 and abs(info["obj_val"] - optimum) <= 1e-6, (info["obj_val"], optimum)
        assert np.abs(var.x[0]).max() > 0.5
        assert info["regularisations"] > 0
        runs[name] = info
    first = runs[1]
    for k in (3, 8):
        info = runs[k]
        assert (info["iterations"], info["regularisations"]) == (first["iterations"], first["regularisations"]), k
        assert np.float64(info["obj_val"]).tobytes() == np.float64(first["obj_val"]).tobytes(), (k, info["obj_val"], first["obj_val"])
        for key in ("x", "mult_g"):
            assert sc.same_bits(np.asarray(info[key], dtype=np.float64), np.asarray(first[key], dtype=np.float64)), (k, key)


@pytest.mark.parametrize("scheme", ("radau", "lobatto"))
def test_a_trial_point_outside_the_domain_is_rejected_not_adopted(scheme, monkeypatch):
    from pockit_amd.optimizer import interior_point

    asked, original = [], interior_point.trial_lengths

    def spy(alpha_max, done, *args, **kw):
        asked.append(int(done))
        return original(alpha_max, done, *args, **kw)

    monkeypatch.setattr(interior_point, "trial_lengths", spy)
    system, _, guess = im.sqrt_well(_ns(scheme, "pockit_amd"))
    (var,), info = _solve(system, guess, linear_solver="direct")
    _report(f"sqrt_well({scheme}), direct", info)
    _converged(im.sqrt_well(_ns(scheme, "oracle"))[0], info, dictated=dictated(system))
    assert abs(info["obj_val"] - im.SQRT_WELL_OPTIMUM) <= 1e-7
    assert np.all(var.x[0] > 0.0)
    assert max(asked) >= 1, "the line search never went behind its first trial point"


def test_a_start_outside_the_domain_is_status_minus_13():
    system, _, guess = im.sqrt_well(_ns("radau", "pockit_amd"), start=-1.0)
    start = models.pack_guess(system, guess)
    _, info = _solve(system, guess, linear_solver="direct")
    assert info["status"] == -13 and info["iterations"] == 0 and "non-finite" in info["status_msg"]
    assert np.array_equal(info["x"], start)


def test_a_problem_without_a_feasible_point_ends_with_a_failure_status():
    system, _, guess = im.unreachable(_ns("radau", "pockit_amd"))
    (var,), info = _solve(system, guess, {"max_iter": 60}, linear_solver="direct")
    _report("unreachable(radau), direct", info)
    assert info["status"] in (-1, -2), (info["status"], info["status_msg"])
    assert np.all(np.isfinite(info["x"])) and np.all(np.isfinite(var.data)) and info["error"] > TOL


def test_every_print_level_prints_and_changes_nothing(capsys):
    """``print_level`` 1, 2 and 3 on the double well (regularised steps and backtracking both occur): no exception, the lines they
    promise, and the bits of the silent solve."""
    runs = []
    for level in (0, 1, 2, 3):
        system, _, guess = im.double_well(_ns("radau", "pockit_amd"))
        _, info = _solve(system, guess, {"print_level": level}, linear_solver="direct")
        text = capsys.readouterr().out
        assert (" E_0 " in text) == (level >= 1) and ("step: delta_w" in text) == (level >= 2) and ("alpha " in text) == (level >= 3), (level, text[:400])
        runs.append(info)
    for info in runs[1:]:
        assert info["status"] == 0 and info["iterations"] == runs[0]["iterations"] and sc.same_bits(info["x"], runs[0]["x"])
