"""Small models that drive ``pockit_amd.optimizer.interior_point.solve`` down the branches the benchmark models never take: a
saddle that only a curvature test leaves, variable bounds that are active at the optimum, a trial point outside the model's
domain, a start outside it, and a problem without a feasible point.  Plain builders with no fixtures; each takes the namespace
``ns`` (``pockit_amd.<scheme>`` or ``oracle.<scheme>``) as the builders of ``models`` do, and returns ``(system, phases, guess)``.

The reference figures (SLSQP on the oracle from the builder's guess, ``test_gpu_interior_point._slsqp``) are held by
tests/test_ipm_models_cpu.py; the GPU tests (tests/test_gpu_interior_point_branches.py) compare the solver with them.
"""
import numpy as np
import sympy as sp

import models

# what SLSQP finds on the oracle from the builder's guess, by (scheme, mesh, num_point)
DOUBLE_WELL_OPTIMUM = {("radau", 4, 5): -2.1553347912, ("lobatto", 4, 5): -2.1553347958}
BOUNDED_LQR_OPTIMUM = {("lobatto", 6, 6): 0.24983625008, ("radau", 5, 4): 0.24982912842}
BOUNDED_LQR_ACTIVE = {("lobatto", 6, 6): (11, 31), ("radau", 5, 4): (7, 20)}       # (active bounds, bounded controls)
UNBOUNDED_LQR_OPTIMUM = 0.2319139745
MIN_TIME_OPTIMUM = 2.0
SQRT_WELL_OPTIMUM = -1.0


def double_well(ns, mesh=4, num_point=5, a=6.0):
    """``x' = u``, ``x(0) = 0``, ``x(1)`` free on [0, 1], integral ``-a x^2 + x^4 + u^2``.  ``x = 0`` is a KKT point with f = 0
    and a saddle; the two optima lie in the wells at ``x = +-sqrt(a / 2)``.  The guess ``x = 0.05 t``, ``u = 0.05`` is so close
    to the saddle that the Newton step lands on it, along a direction of negative curvature."""
    system = ns.System(0)
    phase = system.new_phase(["x"], ["u"])
    (x,), (u,) = phase.x, phase.u
    phase.set_dynamics([u])
    phase.set_integral([-a * x**2 + x**4 + u**2])
    phase.set_boundary_condition([0.0], [None], 0.0, 1.0)
    phase.set_discretization(mesh, num_point)
    system.set_phase([phase])
    system.set_objective(phase.I[0])
    guess = ns.linear_guess(phase, 0.0)
    guess.x[0] = 0.05 * guess.t_x
    guess.u[0] = 0.05 + 0.0 * guess.t_u
    return system, [phase], [guess]


def bounded_lqr(ns, mesh, num_point):
    """``models.lqr`` with ``u >= -1`` given as a bare symbol, which makes it a variable bound and no path row; the zero guess.
    Convex; the bound is active on the first part of the horizon."""
    system, (phase,), _ = models.lqr(ns, mesh, num_point)
    (u,) = phase.u
    phase.set_phase_constraint([u], [-1.0], [np.inf])
    system.set_phase([phase])
    return system, [phase], [ns.constant_guess(phase, 0.0), [0.0]]


def min_time(ns, mesh=4, num_point=4):
    """The double integrator ``x' = v``, ``v' = u`` with ``-1 <= u <= 1`` (a bare symbol: variable bounds) from rest at 0 to rest
    at 1 in the shortest time.  The optimum is ``t_f = 2``, ``u = +1`` then ``-1``; with an even ``mesh`` the switch lies on a mesh
    point.  The guess: ``t_f = 3``, x linear, everything else 0."""
    system = ns.System(0)
    phase = system.new_phase(["x", "v"], ["u"])
    (u,) = phase.u
    phase.set_dynamics([phase.x[1], u])
    phase.set_integral([1.0])
    phase.set_phase_constraint([u], [-1.0], [1.0])
    phase.set_boundary_condition([0.0, 0.0], [1.0, 0.0], 0.0, None)
    phase.set_discretization(mesh, num_point)
    system.set_phase([phase])
    system.set_objective(phase.I[0])
    guess = ns.linear_guess(phase, 0.0)
    guess.t_f = 3.0
    guess.x[0] = guess.t_x / 3.0
    return system, [phase], [guess]


def sqrt_well(ns, mesh=3, num_point=4, start=4.0):
    """``x' = u`` on [0, 1] with both ends free, integral ``x - 2 sqrt(x) + u^2``: defined for ``x >= 0`` only, with an infinite
    gradient at 0.  The optimum is ``x = 1``, ``u = 0``, f = -1.  From ``start = 4`` the Newton step is ``dx = -8`` at every
    node: the full step leaves the domain (NaN), the half step lands on its edge.  ``start = -1`` is outside it."""
    system = ns.System(0)
    phase = system.new_phase(["x"], ["u"])
    (x,), (u,) = phase.x, phase.u
    phase.set_dynamics([u])
    phase.set_integral([x - 2 * sp.sqrt(x) + u**2])
    phase.set_boundary_condition([None], [None], 0.0, 1.0)
    phase.set_discretization(mesh, num_point)
    system.set_phase([phase])
    system.set_objective(phase.I[0])
    guess = ns.constant_guess(phase, float(start))
    guess.u[0] = 0.0 * guess.t_u               # (constant_guess fills the control too)
    return system, [phase], [guess]


def unreachable(ns, mesh=3, num_point=4):
    """``x' = u`` from ``x(0) = 0`` to ``x(1) = 1`` on [0, 1] with ``|u| <= 0.5`` (variable bounds), integral ``u^2``: x can reach
    0.5 at most, so no feasible point exists."""
    system = ns.System(0)
    phase = system.new_phase(["x"], ["u"])
    (u,) = phase.u
    phase.set_dynamics([u])
    phase.set_integral([u**2])
    phase.set_phase_constraint([u], [-0.5], [0.5])
    phase.set_boundary_condition([0.0], [1.0], 0.0, 1.0)
    phase.set_discretization(mesh, num_point)
    system.set_phase([phase])
    system.set_objective(phase.I[0])
    return system, [phase], [ns.constant_guess(phase, 0.0)]
