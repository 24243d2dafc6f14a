"""``interior_point.solve(..., sensitivity=...)`` on the device against the oracle-side references of
tests/sensitivity_models.py.

* ``param_lqr`` at Radau 4 x 4 and Lobatto 4 x 4, "banded" and "direct", the held static parameter ``s_0`` alone and together with
  the right-hand side of the row ``2 x_f = c``: ``dx`` and ``dlam`` within ``1e-8 max(1, |ref|_inf)`` of the dense solve on the
  oracle's J and H at the solver's point (K of a QP does not depend on the iterate, so the solver's own ``tol = 1e-8`` is a generous
  bound); ``|dobj - 2 obj_val / p0| <= 2e-6 |dobj|`` without the row (a quadratic value function; the bound the suite uses against
  the Riccati value), ``p0 dobj_p0 + c dobj_c`` against ``2 obj_val`` with it; ``dobj`` of the row equals ``-mult_g[i]`` exactly.
* the control-bounded variant (``u >= -1``, active on the first part of the horizon, strictly complementary): against the
  ACTIVE-SET sensitivity of the oracle -- SLSQP's point polished by Newton's method with the variables on a bound held.  The
  difference is the O(mu) effect of the barrier; the bound is BARRIER_GAP below.
* 70 row parameters in one call (two block solves against one factorisation): the columns bit-equal to those of two smaller calls.
* ``max_iter = 2``: ``"not_converged"``, arrays None.  ``sensitivity=None``: today's keys, ``x`` bit-equal to the call without the
  argument.  On the banded path no CSR value and no right-hand side block comes down."""
import importlib

import numpy as np
import pytest

import models
import sensitivity_models as sm
import sparse_cases as sc
from test_gpu_interior_point import _slsqp

pytestmark = pytest.mark.gpu

TOL, P0, C = 1e-8, 1.0, 0.5
# The barrier's O(mu) effect on the sensitivities at the final mu = 2.5e-9 of tol = 1e-8, relative to |ref|_inf: measured 4.82e-5
# (7.28e-5 absolute at |ref|_inf = 1.510; radau 5 x 4, banded and direct alike; the constant in front of mu is 1 / z^2 of the most
# weakly active bound).  The bound is 100 times that, capped at 1e-4: the cap binds.
BARRIER_GAP = min(100 * 4.82e-5, 1e-4)


def _ns(scheme, package):
    return importlib.import_module(f"{package}.{scheme}")


def _solve(build, opts=None, **kw):
    from pockit_amd.optimizer import interior_point

    system, _, guess = build
    try:
        return system, interior_point.solve(system, guess, dict({"tol": TOL, "max_iter": 200}, **(opts or {})), **kw)[1]
    finally:
        system.evaluator.close()


def _held(system, ref):
    from pockit_amd.optimizer._common import dictated_slots

    fixed_at, _, func = dictated_slots(system)
    held = np.asarray(ref.v_lb, dtype=np.float64) == np.asarray(ref.v_ub, dtype=np.float64)
    held[fixed_at] = True
    held[[slot for slot, _, _ in func]] = True
    return held


@pytest.mark.parametrize("with_row", (False, True), ids=("variable", "variable-and-row"))
@pytest.mark.parametrize("linear_solver", ("banded", "direct"))
@pytest.mark.parametrize("scheme", ("radau", "lobatto"))
def test_param_lqr_matches_the_dense_oracle_solve(scheme, linear_solver, with_row):
    c = C if with_row else None
    ref = sm.param_lqr(_ns(scheme, "oracle"), 4, 4, P0, c=c)[0]
    build = sm.param_lqr(_ns(scheme, "pockit_amd"), 4, 4, P0, c=c)
    slot = build[0].plan.l_s
    rows = [0] if with_row else []
    system, info = _solve(build, linear_solver=linear_solver, sensitivity={"variables": [slot], "rows": rows})
    s = info["sensitivity"]
    assert info["status"] == 0 and s["status"] == "ok" and s["parameters"] == [("variable", slot)] + [("row", 0)] * with_row
    assert (s["record"] is None) == (linear_solver == "direct") and (s["record"] is None or s["record"][0] == 0.0)
    n, m, k = system.plan.n, system.plan.m, 1 + with_row
    assert s["dx"].shape == (n, k) and s["dlam"].shape == (m, k) and s["dobj"].shape == (k,)
    held = _held(system, ref)
    dx, dlam, dobj = sm.active_sensitivity(ref, info["x"], info["mult_g"], held, [slot], rows)
    size = max(np.abs(dx).max(), np.abs(dlam).max())
    err = max(np.abs(s["dx"] - dx).max(), np.abs(s["dlam"] - dlam).max())
    print(f"{scheme} {linear_solver} {'with' if with_row else 'without'} the row: |S - ref|_inf {err:.3e}, |ref|_inf {size:.3f}, bound "
          f"{1e-8 * max(1.0, size):.1e}; dobj {s['dobj']!r}, 2 obj {2 * info['obj_val']!r}")
    assert err <= 1e-8 * max(1.0, size)
    assert s["dx"][slot, 0] == 1.0 and not s["dx"][held][:, 1:].any() and np.count_nonzero(s["dx"][held, 0]) == 1
    assert np.abs(s["dobj"] - dobj).max() <= 1e-8 * max(1.0, np.abs(dobj).max())
    if with_row:
        assert s["dobj"][1] == -info["mult_g"][0]
        euler = P0 * s["dobj"][0] + C * s["dobj"][1]
        assert abs(euler - 2.0 * info["obj_val"]) <= 2e-6 * abs(euler)
    else:
        assert abs(s["dobj"][0] - 2.0 * info["obj_val"] / P0) <= 2e-6 * abs(s["dobj"][0])
    also = _solve(sm.param_lqr(_ns(scheme, "pockit_amd"), 4, 4, P0, c=c), linear_solver=linear_solver, sensitivity="fixed")[1]["sensitivity"]
    assert also["parameters"] == [("variable", slot)] and sc.same_bits(also["dx"][:, 0].copy(), s["dx"][:, 0].copy())


@pytest.fixture(scope="module")
def active_set():
    """The oracle's active-set reference of the control-bounded variant at Radau 5 x 4: SLSQP's point, the variables within 1e-7
    of a bound held (what ``_polish`` of tests/test_ipm_models_cpu.py holds), Newton's method, the sensitivity."""
    ref, _, guess = sm.param_lqr(_ns("radau", "oracle"), 5, 4, P0, u_max=1.0)
    system = sm.param_lqr(_ns("radau", "pockit_amd"), 5, 4, P0, u_max=1.0)[0]
    x0 = models.pack_guess(ref, guess)
    res = _slsqp(ref, x0)
    v_lb, v_ub = np.asarray(ref.v_lb, dtype=np.float64), np.asarray(ref.v_ub, dtype=np.float64)
    x = res.x.copy()
    at_lb, at_ub = np.abs(x - v_lb) <= 1e-7, np.abs(x - v_ub) <= 1e-7
    x[at_lb], x[at_ub] = v_lb[at_lb], v_ub[at_ub]
    held = _held(system, ref) | at_lb | at_ub
    active = at_lb & (v_lb != v_ub)
    x, lam, f = sm.solve_active(ref, x, held)
    z = (ref.gradient(x) + sm.dense(ref, x, lam)[0].T @ lam)[active]
    assert int(active.sum()) >= 3 and np.all(z > 1e-3), (int(active.sum()), z)      # active and strictly complementary
    slot = int(ref.l_s)
    return ref, slot, f, sm.active_sensitivity(ref, x, lam, held, [slot], [])


@pytest.mark.parametrize("linear_solver", ("banded", "direct"))
def test_an_active_control_bound_matches_the_active_set_sensitivity(active_set, linear_solver):
    ref, slot, f, (dx, dlam, dobj) = active_set
    system, info = _solve(sm.param_lqr(_ns("radau", "pockit_amd"), 5, 4, P0, u_max=1.0), linear_solver=linear_solver, sensitivity="fixed")
    s = info["sensitivity"]
    assert info["status"] == 0 and s["status"] == "ok" and s["parameters"] == [("variable", slot)]
    assert abs(info["obj_val"] - f) <= 1e-6 and np.max(info["mult_x_L"]) > 1e-3
    size = max(np.abs(dx).max(), np.abs(dlam).max())
    err = max(np.abs(s["dx"] - dx).max(), np.abs(s["dlam"] - dlam).max())
    print(f"{linear_solver}: barrier sensitivities against the active set: {err:.3e} = {err / size:.3e} |ref|_inf (|ref|_inf {size:.3f}), mu {info['mu']:.1e}; "
          f"dobj {s['dobj'][0]!r} against {dobj[0]!r}")
    assert err <= BARRIER_GAP * size
    assert abs(s["dobj"][0] - dobj[0]) <= BARRIER_GAP * max(1.0, abs(dobj[0]))


def test_seventy_row_parameters_in_one_call_match_two_smaller_calls():
    build = lambda: sm.param_lqr(_ns("radau", "pockit_amd"), 10, 8, P0)  # noqa: E731
    rows = list(range(5, 75))
    assert build()[0].plan.m >= 75
    whole = _solve(build(), linear_solver="banded", sensitivity={"rows": rows})[1]["sensitivity"]
    assert whole["status"] == "ok" and whole["dx"].shape[1] == 70 and whole["record"][0] == 0.0
    lo = 0
    for part in (rows[:30], rows[30:]):
        s = _solve(build(), linear_solver="banded", sensitivity={"rows": part})[1]["sensitivity"]
        hi = lo + len(part)
        for name in ("dx", "dlam"):
            assert sc.same_bits(np.ascontiguousarray(whole[name][:, lo:hi]), np.ascontiguousarray(s[name])), (name, lo)
        assert sc.same_bits(whole["dobj"][lo:hi].copy(), s["dobj"])
        lo = hi
    assert np.abs(whole["dx"]).max() > 0.0 and not np.array_equal(whole["dx"][:, 0], whole["dx"][:, 69])


@pytest.mark.parametrize("linear_solver", ("banded", "direct"))
def test_an_unconverged_solve_reports_not_converged(linear_solver):
    _, info = _solve(sm.param_lqr(_ns("radau", "pockit_amd"), 5, 4, P0, u_max=1.0), opts={"max_iter": 2}, linear_solver=linear_solver,
                     sensitivity="fixed")
    s = info["sensitivity"]
    assert info["status"] == -1 and s["status"] == "not_converged" and len(s["parameters"]) == 1
    assert s["dx"] is None and s["dlam"] is None and s["dobj"] is None and s["record"] is None


@pytest.mark.parametrize("linear_solver", ("banded", "direct"))
def test_without_the_argument_nothing_changes(linear_solver):
    from pockit_amd.optimizer import interior_point

    build = lambda: sm.param_lqr(_ns("radau", "pockit_amd"), 4, 4, P0, c=C)  # noqa: E731
    _, plain = _solve(build(), linear_solver=linear_solver)                     # the call form there was before
    _, none = _solve(build(), linear_solver=linear_solver, sensitivity=None)
    _, asked = _solve(build(), linear_solver=linear_solver, sensitivity="fixed")
    assert set(plain) == set(none) == set(interior_point.INFO_KEYS) and set(asked) == set(interior_point.INFO_KEYS) | {"sensitivity"}
    for key in ("x", "mult_g", "g", "mult_x_L"):
        assert sc.same_bits(plain[key], none[key]) and sc.same_bits(plain[key], asked[key]), key
    assert plain["iterations"] == none["iterations"] == asked["iterations"] and plain["obj_val"] == asked["obj_val"]


def test_on_the_banded_path_no_matrix_value_and_no_right_hand_side_comes_down(monkeypatch):
    from pockit_amd.optimizer import interior_point

    seen, residents = [], []
    down, init = interior_point._Resident.down, interior_point._Resident.__init__

    def spy_init(self, *a, **kw):
        init(self, *a, **kw)
        residents.append(self)

    def spy_down(self, t, count=None):
        seen.append((t.data_ptr(), t.numel()))
        return down(self, t, count)

    monkeypatch.setattr(interior_point._Resident, "__init__", spy_init)
    monkeypatch.setattr(interior_point._Resident, "down", spy_down)
    build = sm.param_lqr(_ns("radau", "pockit_amd"), 4, 4, P0, c=C)
    slot = build[0].plan.l_s
    system, info = _solve(build, linear_solver="banded", sensitivity={"variables": [slot], "rows": [0, 3]})
    assert info["sensitivity"]["status"] == "ok"
    (R,) = residents
    n, m = R.n, R.m
    block = 3 * (n + m)
    matrix = {R.cj.data_ptr(), R.ch.data_ptr(), R.jt.data_ptr(), R.ht.data_ptr(), R.sig_x.data_ptr(), R.s2.data_ptr(), R.rhs.data_ptr()}
    assert not [p for p, _ in seen if p in matrix], "a matrix value or a right-hand side was downloaded"
    assert [c for _, c in seen].count(block) == 1, "the block of solutions comes down once; the block of right-hand sides never"
    assert max(c for _, c in seen) <= max(block, 64)
