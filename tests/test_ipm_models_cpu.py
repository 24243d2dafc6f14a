"""The models of tests/ipm_models.py on the oracle alone: what tests/test_gpu_interior_point_branches.py compares the solver
with stands here on its own, without a GPU.

* The references.  SLSQP on the oracle (``test_gpu_interior_point._slsqp``, ``ftol = 1e-14``) from each builder's guess gives the
  recorded optimum to 1e-9 (the figures are recorded with ten decimals).  For ``double_well`` and ``bounded_lqr`` SLSQP's point is
  polished by Newton's method on the dense KKT system of its active set (the bounds it ends on held as equalities); SLSQP and the
  polished value agree to 1e-8, two orders inside the GPU file's 1e-6, and the polished multipliers of the active bounds have the
  sign of a minimum.
* ``double_well``.  The Hessian reduced to the null space of J at the guess has a negative eigenvalue; the Newton step d from the
  guess fails ``d.H d >= 1e-11 |d|^2`` and lands on the saddle ``x = 0``, where f = 0 and the KKT residual is exactly zero.
* ``sqrt_well``.  The Newton step from the guess is -8 at every state node; the full step leaves the domain (NaN), the half step
  is ``x = 0`` with f = 0 = f(guess) and a non-finite gradient, the quarter step has f = 2 - 2 sqrt(2).  The start ``x = -1`` is NaN.
* ``min_time``: SLSQP ends on ``t_f = 2`` with every control on a bound but the Lobatto node at the switch.  ``unreachable``: the
  equality rows cannot be met inside the bounds (a linear programme says so).
* The dead variables.  For every model the GPU solver tests solve, the slots of ``dictated_slots`` have no non-zero in the oracle's
  J and H at the start, and the first step's matrix ``K = [[H + Sigma_x, J^T], [J, -S2]]`` (``Sigma_x`` on the live variables, as
  the solver has it once those slots are fixed) has full rank without their rows and columns and a rank deficit equal to their
  number with them: left free they make K structurally singular.
"""
import importlib

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse

import ipm_models as im
import models
from pockit_amd.optimizer import interior_point as ipm
from pockit_amd.optimizer._common import dictated_slots
from test_gpu_interior_point import _slsqp, constrained_lqr


def _ns(scheme, package="oracle"):
    return importlib.import_module(f"{package}.{scheme}")


def _dense(ref, x, lam=None):
    """(J, H) of the oracle at x as dense arrays; H is the Lagrangian's full symmetric Hessian at ``lam`` (default 0)."""
    n, m = len(x), len(ref.c_lb)
    J = scipy.sparse.coo_array((ref.jacobian(x), ref.jacobianstructure()), shape=(m, n)).toarray()
    L = scipy.sparse.coo_array((ref.hessian(x, np.zeros(m) if lam is None else lam, 1.0), ref.hessianstructure()), shape=(n, n)).toarray()
    return J, L + L.T - np.diag(np.diag(L))


def _dead(builder, scheme, *args):
    """The indices of the dictated slots, from the product's transcription of the same model."""
    fixed_at, _, func = dictated_slots(builder(_ns(scheme, "pockit_amd"), *args)[0])
    return np.concatenate((fixed_at, np.array([slot for slot, _, _ in func], dtype=np.int64)))


def _newton_step(ref, x, live):
    """The step of Newton's method on the equality-constrained problem at ``(x, lam = 0)`` over the variables ``live``."""
    J, H = _dense(ref, x)
    m = J.shape[0]
    K = np.block([[H[live][:, live], J[:, live].T], [J[:, live], np.zeros((m, m))]])
    y = np.linalg.solve(K, -np.concatenate((ref.gradient(x)[live], ref.constraints(x) - np.asarray(ref.c_lb))))
    d = np.zeros(len(x))
    d[live] = y[: int(live.sum())]
    return d, H


def _polish(ref, x, dead):
    """Newton's method on the KKT system of the active set at SLSQP's point ``x`` (a model without inequality rows): the
    variables within 1e-7 of a bound, and the dead slots, are held; returns ``(x, f, multipliers of the held bounds, held)``."""
    v_lb, v_ub = np.asarray(ref.v_lb, dtype=np.float64), np.asarray(ref.v_ub, dtype=np.float64)
    assert np.array_equal(ref.c_lb, ref.c_ub)
    x = x.copy()
    at_lb, at_ub = np.abs(x - v_lb) <= 1e-7, np.abs(x - v_ub) <= 1e-7
    x[at_lb], x[at_ub] = v_lb[at_lb], v_ub[at_ub]
    held = at_lb | at_ub
    live = ~held
    live[dead] = False
    lam = np.zeros(len(ref.c_lb))
    for _ in range(20):
        J, H = _dense(ref, x, lam)
        m = J.shape[0]
        r = np.concatenate(((ref.gradient(x) + J.T @ lam)[live], ref.constraints(x) - np.asarray(ref.c_lb)))
        if np.abs(r).max() <= 1e-13:
            break
        y = np.linalg.solve(np.block([[H[live][:, live], J[:, live].T], [J[:, live], np.zeros((m, m))]]), -r)
        x[live] += y[: int(live.sum())]
        lam = lam + y[int(live.sum()):]
    assert np.abs(r).max() <= 1e-13, np.abs(r).max()
    z = ref.gradient(x) + J.T @ lam          # = z_L - z_U on the held variables
    return x, ref.objective(x), np.where(at_lb, z, -z)[held & (at_lb | at_ub)], held


# ---------------------------------------------------------------------------- the references
@pytest.mark.parametrize("scheme", ("radau", "lobatto"))
def test_slsqp_finds_a_well_of_the_double_well_and_newton_confirms_it(scheme):
    ref, _, guess = im.double_well(_ns(scheme))
    res = _slsqp(ref, models.pack_guess(ref, guess))
    want = im.DOUBLE_WELL_OPTIMUM[scheme, 4, 5]
    x, f, _, held = _polish(ref, res.x, _dead(im.double_well, scheme))
    print(f"SLSQP {res.fun!r}, polished {f!r}, recorded {want!r}; n {len(res.x)}, m {len(ref.c_lb)}")
    assert (len(res.x), len(ref.c_lb)) == {"radau": (43, 20), "lobatto": (36, 16)}[scheme]
    assert abs(res.fun - want) <= 1e-9 and abs(res.fun - f) <= 1e-8
    assert not held.any() and np.abs(x).max() > 0.5
    # a minimum, not the saddle: the Hessian reduced to the null space of J (live variables) is positive definite there
    live = np.ones(len(x), dtype=bool)
    live[_dead(im.double_well, scheme)] = False
    J, H = _dense(ref, x)
    Z = scipy.linalg.null_space(J[:, live])
    assert np.linalg.eigvalsh(Z.T @ H[live][:, live] @ Z).min() > 0.0


@pytest.mark.parametrize("scheme,mesh,num_point", [("lobatto", 6, 6), ("radau", 5, 4)])
def test_slsqp_ends_on_the_bound_of_the_bounded_lqr_and_newton_confirms_it(scheme, mesh, num_point):
    ref, _, guess = im.bounded_lqr(_ns(scheme), mesh, num_point)
    res = _slsqp(ref, models.pack_guess(ref, guess))
    want = im.BOUNDED_LQR_OPTIMUM[scheme, mesh, num_point]
    x, f, z, held = _polish(ref, res.x, _dead(im.bounded_lqr, scheme, mesh, num_point))
    bounded = np.isfinite(np.asarray(ref.v_lb, dtype=np.float64))
    print(f"SLSQP {res.fun!r}, polished {f!r}, recorded {want!r}; {int(held.sum())} of {int(bounded.sum())} bounds active, multipliers {z.min():.3e} ... {z.max():.3e}")
    assert abs(res.fun - want) <= 1e-9 and abs(res.fun - f) <= 1e-8
    assert (int(held.sum()), int(bounded.sum())) == im.BOUNDED_LQR_ACTIVE[scheme, mesh, num_point]
    assert np.all(x[held] == -1.0) and np.all(z > 0.0) and np.all(x[bounded] >= -1.0)
    assert f - im.UNBOUNDED_LQR_OPTIMUM > 1e-2


@pytest.mark.parametrize("scheme", ("radau", "lobatto"))
def test_slsqp_finds_the_bang_bang_control_of_the_minimum_time_model(scheme):
    ref, (phase,), guess = im.min_time(_ns(scheme))
    res = _slsqp(ref, models.pack_guess(ref, guess))
    v_lb = np.asarray(ref.v_lb, dtype=np.float64)
    u = res.x[np.isfinite(v_lb)]
    print(f"SLSQP t_f {res.x[-1]!r}, f {res.fun!r}, u {u}")
    assert abs(res.fun - im.MIN_TIME_OPTIMUM) <= 1e-12 and abs(res.x[-1] - im.MIN_TIME_OPTIMUM) <= 1e-12
    inner = np.abs(np.abs(u) - 1.0) > 1e-6
    assert int(inner.sum()) == (1 if scheme == "lobatto" else 0) and np.all(np.abs(u[inner]) <= 1e-6)
    half = len(u) // 2
    assert np.all(u[:half] > 0.0) and np.all(u[len(u) - half:] < 0.0)


def test_the_unreachable_model_has_no_feasible_point():
    """Its rows are linear in the live variables: a linear programme finds none inside the bounds."""
    from scipy.optimize import linprog

    ref, _, guess = im.unreachable(_ns("radau"))
    x0 = models.pack_guess(ref, guess)
    J, H = _dense(ref, x0)
    assert np.array_equal(J, _dense(ref, x0 + 1.0)[0])
    res = linprog(np.zeros(len(x0)), A_eq=J, b_eq=np.asarray(ref.c_lb) - (ref.constraints(x0) - J @ x0), bounds=list(zip(ref.v_lb, ref.v_ub)))
    assert res.status == 2, res.message


# ---------------------------------------------------------------------------- the double well's saddle
@pytest.mark.parametrize("scheme", ("radau", "lobatto"))
def test_the_newton_step_of_the_double_well_has_negative_curvature_and_lands_on_the_saddle(scheme):
    ref, _, guess = im.double_well(_ns(scheme))
    x0 = models.pack_guess(ref, guess)
    live = np.ones(len(x0), dtype=bool)
    live[_dead(im.double_well, scheme)] = False
    d, H = _newton_step(ref, x0, live)
    J = _dense(ref, x0)[0]
    Z = scipy.linalg.null_space(J[:, live])
    eig = np.linalg.eigvalsh(Z.T @ H[live][:, live] @ Z)
    curvature, step_sq = float(d @ H @ d), float(d @ d)
    landed = x0 + d
    print(f"reduced Hessian {eig.min():.3e} ... {eig.max():.3e}; d.H d {curvature:.4e} against {ipm.KAPPA_CURV * step_sq:.1e}; "
          f"max |x + d| {np.abs(landed[live]).max():.2e}, f(x + d) {ref.objective(landed):.3e}")
    assert eig.min() < 0.0
    assert not curvature >= ipm.KAPPA_CURV * step_sq
    assert abs(curvature - (-5.005e-3)) <= 5e-6 and 1e-13 < ipm.KAPPA_CURV * step_sq < 1e-12
    assert np.abs(landed[live]).max() <= 1.4e-4 and abs(ref.objective(landed) - (-7.05e-9)) <= 5e-11
    # the saddle itself
    saddle = np.where(live, 0.0, x0)
    assert ref.objective(saddle) == 0.0 and not ref.gradient(saddle)[live].any()
    assert not (ref.constraints(saddle) - np.asarray(ref.c_lb)).any()
    Js, Hs = _dense(ref, saddle)
    Zs = scipy.linalg.null_space(Js[:, live])
    eig_s = np.linalg.eigvalsh(Zs.T @ Hs[live][:, live] @ Zs)
    assert eig_s.min() < 0.0 < eig_s.max()


# ---------------------------------------------------------------------------- the edge of the square root's domain
@pytest.mark.parametrize("scheme", ("radau", "lobatto"))
def test_the_newton_step_of_the_sqrt_well_leaves_the_domain(scheme):
    ref, _, guess = im.sqrt_well(_ns(scheme))
    x0 = models.pack_guess(ref, guess)
    live = np.ones(len(x0), dtype=bool)
    live[_dead(im.sqrt_well, scheme)] = False
    state = x0 == 4.0
    d, _ = _newton_step(ref, x0, live)
    assert np.abs(d[state] + 8.0).max() <= 1e-12 and np.abs(d[~state]).max() <= 1e-12
    d = np.where(state, -8.0, 0.0)
    assert ref.objective(x0) == 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.isnan(ref.objective(x0 + d))
        half = x0 + 0.5 * d
        assert not half[state].any() and ref.objective(half) == 0.0 and not np.all(np.isfinite(ref.gradient(half)))
        assert abs(ref.objective(x0 + 0.25 * d) - (2.0 - 2.0 * np.sqrt(2.0))) <= 1e-13      # (a quadrature of 13 or 10 terms of size 1)
        outside = models.pack_guess(ref, im.sqrt_well(_ns(scheme), start=-1.0)[2])
        assert np.all(outside[state] == -1.0) and np.isnan(ref.objective(outside))
    optimum = np.where(state, 1.0, np.where(live, 0.0, x0))
    assert abs(ref.objective(optimum) - im.SQRT_WELL_OPTIMUM) <= 1e-13 and np.abs(ref.gradient(optimum)[live]).max() <= 1e-16
    assert not (ref.constraints(optimum) - np.asarray(ref.c_lb)).any()


# ---------------------------------------------------------------------------- the dead variables
def _lqr_zero(ns, mesh, num_point):
    system, (phase,), _ = models.lqr(ns, mesh, num_point)
    return system, [phase], [ns.constant_guess(phase, 0.0), [0.0]]


SOLVED = [(_lqr_zero, "lobatto", (6, 6), [0, 30, 62, 63]),
          (models.brachistochrone, "radau", (10, 8), [0, 80, 81, 161, 162, 323]),
          (models.brachistochrone, "lobatto", (6, 6), [0, 30, 31, 61, 62, 124]),
          (constrained_lqr, "lobatto", (6, 6), None), (constrained_lqr, "radau", (5, 4), None),
          (im.bounded_lqr, "lobatto", (6, 6), None), (im.bounded_lqr, "radau", (5, 4), None),
          (im.double_well, "radau", (), None), (im.double_well, "lobatto", (), None),
          (im.sqrt_well, "radau", (), None), (im.sqrt_well, "lobatto", (), None),
          (im.unreachable, "radau", (), None)]


@pytest.mark.parametrize("builder,scheme,args,slots", SOLVED, ids=[f"{b.__name__.strip('_')}-{s}" for b, s, _, _ in SOLVED])
def test_dictated_slots_are_empty_rows_and_columns_of_the_step_matrix(builder, scheme, args, slots):
    ref, _, guess = builder(_ns(scheme), *args)
    dead = _dead(builder, scheme, *args)
    assert len(dead) > 0 and (slots is None or sorted(dead.tolist()) == slots)
    v_lb, v_ub, c_lb, c_ub = (np.asarray(a, dtype=np.float64) for a in (ref.v_lb, ref.v_ub, ref.c_lb, ref.c_ub))
    n, m = len(v_lb), len(c_lb)
    live = np.ones(n, dtype=bool)
    live[dead] = False
    # the first step's quantities as the solver has them: the pushed start, lam = 0, bound multipliers 1
    x = ipm.push_inside(models.pack_guess(ref, guess), v_lb, v_ub)
    ineq = c_lb != c_ub
    s = np.where(ineq, ipm.push_inside(ref.constraints(x), c_lb, c_ub), 0.0)
    J, H = _dense(ref, x)
    assert not J[:, dead].any() and not H[dead].any() and not H[:, dead].any()
    with np.errstate(divide="ignore"):
        sigma_x = np.where(live & np.isfinite(v_lb), 1.0 / (x - v_lb), 0.0) + np.where(live & np.isfinite(v_ub), 1.0 / (v_ub - x), 0.0)
        sigma_s = np.where(ineq & np.isfinite(c_lb), 1.0 / (s - c_lb), 0.0) + np.where(ineq & np.isfinite(c_ub), 1.0 / (c_ub - s), 0.0)
    s2 = np.where(ineq, 1.0 / np.where(ineq, sigma_s, 1.0), 0.0)
    K = np.block([[H + np.diag(sigma_x), J.T], [J, -np.diag(s2)]])
    keep = np.concatenate((live, np.ones(m, dtype=bool)))
    rank, rank_live = np.linalg.matrix_rank(K), np.linalg.matrix_rank(K[keep][:, keep])
    print(f"K rank {rank} of {n + m}, dictated slots {sorted(dead.tolist())}, without them {rank_live} of {int(keep.sum())}")
    assert rank_live == int(keep.sum()) and rank == n + m - len(dead)
