"""pockit_amd.optimizer.interior_point.solve on the device, end to end, against optima known from elsewhere.

* lqr(lobatto, 6, 6), ``linear_solver`` "direct" and "minres": the Riccati value as tests/test_gpu_parity.py's LQR test computes it,
  within its bound ``2e-6 max(1, |opt|)``; ``x(1) = x_f`` to 1e-9.
* brachistochrone(radau, 10, 8) and (lobatto, 6, 6), direct: the cycloid's descent time within 1e-7 for the objective and for
  ``t_f`` (the bound of the existing trust-constr test), the end point (2, 2) to 1e-12.
* LQR with the path constraints ``x + u >= -0.5`` and ``-1.5 <= u <= 0.5`` (defined here: ``constrained_lqr``), Lobatto 6 x 6 and
  Radau 5 x 4, direct: the objective within 1e-6 of SciPy's SLSQP (``ftol = 1e-14``) on the ORACLE of the same model -- the
  bound leaves room for SLSQP's own accuracy and is four orders below the 6.5e-3 gap to the unconstrained optimum, so a solver
  that ignores the constraint fails --, an inequality row active, its multiplier non-zero.
* every converged case: ``E_0 <= tol`` recomputed here with NumPy on the oracle's f, grad f, g and J from ``info`` alone, bound
  multipliers >= 0, x inside its bounds; a slot whose value the transcription dictates is no variable of the problem: it holds
  the dictated number and has no bound multiplier.
* ``max_iter = 3`` on the brachistochrone: status -1, a finite x, no exception.

The solves cap at ``max_iter = 200`` and assert no iteration count."""
import importlib

import numpy as np
import pytest
import scipy.sparse

import models

pytestmark = pytest.mark.gpu

TOL = 1e-8


def _ns(scheme, package):
    return importlib.import_module(f"{package}.{scheme}")


def constrained_lqr(ns, mesh, num_point):
    """The LQR of ``models.lqr`` with an active path inequality and control bounds; the start is the zero guess."""
    system, (phase,), _ = models.lqr(ns, mesh, num_point)
    (x,), (u,) = phase.x, phase.u
    phase.set_phase_constraint([x + u, u], [-0.5, -1.5], [np.inf, 0.5])
    system.set_phase([phase])
    return system, [phase], [ns.constant_guess(phase, 0.0), [0.0]]


def dictated(system):
    """``(fixed_at, fixed_to, func_at)`` of a ``pockit_amd`` system: the NLP slots whose value the transcription dictates (a
    number; a function of the static parameters).  The solver fixes them; they are not variables of the problem."""
    from pockit_amd.optimizer._common import dictated_slots

    fixed_at, fixed_to, func = dictated_slots(system)
    return fixed_at, fixed_to, np.array([slot for slot, _, _ in func], dtype=np.int64)


def error_from_info(ref, info, dictated=None):
    """E_0 of the module's docstring from ``info`` alone, every function value from the oracle system ``ref``.  ``dictated``
    (what ``dictated(system)`` returns): those slots are not free, hold the dictated number where there is one, and have no bound
    multiplier."""
    x, lam = info["x"], info["mult_g"]
    zl, zu, s, yl, yu = info["mult_x_L"], info["mult_x_U"], info["slack"], info["mult_s_L"], info["mult_s_U"]
    v_lb, v_ub, c_lb, c_ub = (np.asarray(a, dtype=np.float64) for a in (ref.v_lb, ref.v_ub, ref.c_lb, ref.c_ub))
    n, m = len(x), len(lam)
    g, grad = ref.constraints(x), ref.gradient(x)
    J = scipy.sparse.coo_array((ref.jacobian(x), ref.jacobianstructure()), shape=(m, n)).tocsr()
    free, ineq = v_lb != v_ub, c_lb != c_ub
    if dictated is not None:
        fixed_at, fixed_to, func_at = dictated
        dead = np.concatenate((fixed_at, func_at))
        free[dead] = False
        assert np.array_equal(x[fixed_at], fixed_to), (x[fixed_at], fixed_to)
        assert not zl[dead].any() and not zu[dead].any(), (zl[dead], zu[dead])
    r_d = np.where(free, grad + J.T @ lam - zl + zu, 0.0)
    r_s = np.where(ineq, -lam - yl + yu, 0.0)
    theta = np.where(ineq, g - s, g - c_lb)
    compl, sides, z_sum = [0.0], 0, 0.0
    for present, slack, z in ((free & np.isfinite(v_lb), x - v_lb, zl), (free & np.isfinite(v_ub), v_ub - x, zu),
                              (ineq & np.isfinite(c_lb), s - c_lb, yl), (ineq & np.isfinite(c_ub), c_ub - s, yu)):
        assert np.all(slack[present] > 0.0) and np.all(z[present] >= 0.0) and not z[~present].any()
        compl.append(np.max(slack[present] * z[present], initial=0.0))
        sides += int(present.sum())
        z_sum += float(z[present].sum())
    s_d = max(100.0, (np.abs(lam).sum() + z_sum) / (m + sides)) / 100.0
    e_0 = max(np.abs(r_d).max() / s_d, np.abs(r_s).max() / s_d, np.abs(theta).max(), max(compl) / s_d)
    print(f"E_0 from the oracle {e_0:.3e} (r_d {np.abs(r_d).max():.2e}, r_s {np.abs(r_s).max():.2e}, theta {np.abs(theta).max():.2e}, "
          f"compl {max(compl):.2e}, s_d {s_d:.2f}); the solver's {info['error']:.3e}; {info['iterations']} iterations, "
          f"{info['linear_iterations']} linear, {info['regularisations']} regularised, mu {info['mu']:.1e}")
    return e_0


def _converged(ref, info, dictated=None):
    assert info["status"] == 0, (info["status"], info["status_msg"], info["iterations"], info["error"])
    assert info["error"] <= TOL and error_from_info(ref, info, dictated=dictated) <= TOL
    x = info["x"]
    assert np.all(x >= np.asarray(ref.v_lb)) and np.all(x <= np.asarray(ref.v_ub))
    assert np.all(info["mult_x_L"] >= 0.0) and np.all(info["mult_x_U"] >= 0.0) and np.all(info["mult_s_L"] >= 0.0) and np.all(info["mult_s_U"] >= 0.0)
    assert abs(ref.objective(x) - info["obj_val"]) <= 1e-11 * max(1.0, abs(info["obj_val"]))


def _solve(system, guess, **kw):
    from pockit_amd.optimizer import interior_point

    try:
        return interior_point.solve(system, guess, {"tol": TOL, "max_iter": 200}, **kw)
    finally:
        system.evaluator.close()


@pytest.fixture(scope="module")
def riccati():
    from scipy.integrate import solve_ivp

    a, b, q, r, sw = -1.0, 1.0, 1.0, 0.1, 1.0
    ric = solve_ivp(lambda t, P: -(2 * a * P - b * b * P * P / r + q), (1.0, 0.0), [sw / 2], rtol=1e-11, atol=1e-12)
    return ric.y[0, -1] * 1.0 ** 2


@pytest.mark.parametrize("linear_solver", ("direct", "minres"))
def test_lqr_reaches_the_riccati_value(riccati, linear_solver):
    ns = _ns("lobatto", "pockit_amd")
    system, (phase,), _ = models.lqr(ns, 6, 6)
    (var, s), info = _solve(system, [ns.constant_guess(phase, 0.0), [0.0]], linear_solver=linear_solver)
    _converged(models.lqr(_ns("lobatto", "oracle"), 6, 6)[0], info, dictated=dictated(system))
    assert abs(info["obj_val"] - riccati) <= 2e-6 * max(1.0, abs(riccati)), (info["obj_val"], riccati)
    assert abs(var.x[0][-1] - s[0]) < 1e-9 and abs(var.x[0][0] - 1.0) < 1e-12
    assert (info["linear_iterations"] > 0) == (linear_solver == "minres")


@pytest.mark.parametrize("scheme,mesh,num_point", [("radau", 10, 8), ("lobatto", 6, 6)])
def test_the_brachistochrone_reaches_the_cycloid_time(scheme, mesh, num_point):
    from scipy.optimize import brentq

    system, _, guess = models.brachistochrone(_ns(scheme, "pockit_amd"), mesh, num_point)
    (var,), info = _solve(system, guess)
    theta = brentq(lambda t: (t - np.sin(t)) / (1 - np.cos(t)) - 1.0, 0.1, 2 * np.pi - 0.1)      # x_f / y_f = 1
    optimum = theta * np.sqrt(2.0 / (1 - np.cos(theta)) / 9.81)
    _converged(models.brachistochrone(_ns(scheme, "oracle"), mesh, num_point)[0], info, dictated=dictated(system))
    assert abs(info["obj_val"] - optimum) <= 1e-7, (info["obj_val"], optimum)
    assert abs(var.t_f - optimum) <= 1e-7
    assert abs(var.x[0][-1] - 2.0) < 1e-12 and abs(var.x[1][-1] - 2.0) < 1e-12


def _slsqp(ref, x0):
    """SLSQP on the oracle: dense Jacobians, equality rows as equalities, every finite side of the others as an inequality."""
    from scipy.optimize import minimize

    c_lb, c_ub = np.asarray(ref.c_lb, dtype=np.float64), np.asarray(ref.c_ub, dtype=np.float64)
    m, n = len(c_lb), len(x0)
    eq, lo, up = c_lb == c_ub, (c_lb != c_ub) & np.isfinite(c_lb), (c_lb != c_ub) & np.isfinite(c_ub)
    jac = lambda x: scipy.sparse.coo_array((ref.jacobian(x), ref.jacobianstructure()), shape=(m, n)).toarray()  # noqa: E731
    cons = [dict(type="eq", fun=lambda x: (ref.constraints(x) - c_lb)[eq], jac=lambda x: jac(x)[eq]),
            dict(type="ineq", fun=lambda x: (ref.constraints(x) - c_lb)[lo], jac=lambda x: jac(x)[lo]),
            dict(type="ineq", fun=lambda x: (c_ub - ref.constraints(x))[up], jac=lambda x: -jac(x)[up])]
    res = minimize(ref.objective, x0, jac=ref.gradient, method="SLSQP", constraints=cons, bounds=list(zip(ref.v_lb, ref.v_ub)),
                   options=dict(ftol=1e-14, maxiter=500))
    assert res.success, res.message
    return res


@pytest.mark.parametrize("scheme,mesh,num_point,rows", [("lobatto", 6, 6, 31), ("radau", 5, 4, 20)])
def test_lqr_with_an_active_path_inequality_matches_slsqp_on_the_oracle(scheme, mesh, num_point, rows):
    system, _, guess = constrained_lqr(_ns(scheme, "pockit_amd"), mesh, num_point)
    ref, _, ref_guess = constrained_lqr(_ns(scheme, "oracle"), mesh, num_point)
    c_lb, c_ub = np.asarray(ref.c_lb), np.asarray(ref.c_ub)
    assert int(np.sum(c_lb != c_ub)) == rows
    _, info = _solve(system, guess)
    _converged(ref, info, dictated=dictated(system))
    res = _slsqp(ref, models.pack_guess(ref, ref_guess))
    print(f"interior point {info['obj_val']!r}, SLSQP {res.fun!r}, difference {abs(info['obj_val'] - res.fun):.2e}")
    assert abs(info["obj_val"] - res.fun) <= 1e-6
    g = info["g"]
    active = (c_lb != c_ub) & np.isfinite(c_lb) & (g - c_lb < 1e-6)
    assert active.any(), "no inequality row is active at the solution"
    assert np.all(info["mult_g"][active] != 0.0) and np.abs(info["mult_g"][active]).max() > 1e-3
    assert info["obj_val"] - 0.2319139745 > 1e-3          # (the unconstrained optimum lies 6.5e-3 below)


def test_max_iter_ends_with_status_minus_one_and_a_finite_x():
    system, _, guess = models.brachistochrone(_ns("radau", "pockit_amd"), 10, 8)
    from pockit_amd.optimizer import interior_point

    try:
        (var,), info = interior_point.solve(system, guess, {"max_iter": 3})
    finally:
        system.evaluator.close()
    assert info["status"] == -1 and info["iterations"] == 3 and np.all(np.isfinite(info["x"])) and np.all(np.isfinite(var.data))
    assert "maximum" in info["status_msg"]
