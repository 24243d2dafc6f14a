"""The model and the oracle-side references of the solution sensitivities (``interior_point.solve(..., sensitivity=...)``,
DESIGN.md section 27).  A plain helper module, shared by tests/test_sensitivity_cpu.py (oracle only) and
tests/test_gpu_sensitivity.py (the solver against these references).

``param_lqr`` is the LQR of ``models.lqr`` whose initial state is a static parameter: ``x(0) = s_0`` with ``s_0`` held at ``p0`` by
equal bounds (``set_phase_constraint([s_0], [p0], [p0])``: a bare symbol is a variable bound).  The slot of ``x(0)`` is then a FUNC
slot, dictated by the transcription and without a column; ``s_0`` has the column.  Optionally the equality system constraint
``2 x_f = c`` (a row whose right-hand side is a parameter of the second kind) and the control bound ``u >= -u_max``.

Everything else here runs on the ORACLE: Newton's method on the KKT system of an active set (``solve_active``), the sensitivity
of that system (``active_sensitivity``) and central differences of re-solves (``by_differences``)."""
import numpy as np
import scipy.sparse


def param_lqr(ns, mesh, K, p0, c=None, u_max=None):
    a, b, s_w, q, r = -1.0, 1.0, 1.0, 1.0, 0.1
    system = ns.System(["s_0", "x_f"])
    s_0, x_f = system.s
    phase = system.new_phase(["x"], ["u"])
    (x,), (u,) = phase.x, phase.u
    phase.set_dynamics([a * x + b * u])
    phase.set_integral([q * x**2 + r * u**2])
    if u_max is None:
        phase.set_phase_constraint([s_0], [p0], [p0])
    else:
        phase.set_phase_constraint([s_0, u], [p0, -float(u_max)], [p0, np.inf])
    phase.set_boundary_condition([s_0], [x_f], 0, 1)
    phase.set_discretization(mesh, K)
    system.set_phase([phase])
    system.set_objective(phase.I[0] + s_w * x_f**2 / 2)
    if c is not None:
        system.set_system_constraint([2 * x_f], [float(c)], [float(c)])
    return system, [phase], [ns.constant_guess(phase, 0.0), [float(p0), 0.0]]


def path_constrained_lqr(ns, mesh, K):
    """The LQR with an active path inequality ``x + u >= -0.5`` and control bounds as a row ``-1.5 <= u <= 0.5``: a model with
    inequality rows, which are no parameters."""
    system = ns.System(["x_f"])
    (x_f,) = system.s
    phase = system.new_phase(["x"], ["u"])
    (x,), (u,) = phase.x, phase.u
    phase.set_dynamics([-1.0 * x + 1.0 * u])
    phase.set_integral([1.0 * x**2 + 0.1 * u**2])
    phase.set_phase_constraint([x + u, u], [-0.5, -1.5], [np.inf, 0.5])
    phase.set_boundary_condition([1], [x_f], 0, 1)
    phase.set_discretization(mesh, K)
    system.set_phase([phase])
    system.set_objective(phase.I[0] + 1.0 * x_f**2 / 2)
    return system, [phase], [ns.constant_guess(phase, 0.0), [0.0]]


def dense(ref, x, lam):
    """(J, H) of the oracle at (x, lam) as dense arrays; H the Lagrangian's full symmetric Hessian."""
    n, m = len(x), len(ref.c_lb)
    J = scipy.sparse.coo_array((ref.jacobian(x), ref.jacobianstructure()), shape=(m, n)).toarray()
    L = scipy.sparse.coo_array((ref.hessian(x, lam, 1.0), ref.hessianstructure()), shape=(n, n)).toarray()
    return J, L + L.T - np.diag(np.diag(L))


def solve_active(ref, x, held, rhs=None):
    """Newton's method on the KKT system of the equality rows with the variables ``held`` (a mask) kept at ``x``; the rows'
    right-hand sides are ``rhs`` (default ``c_lb``).  A model without inequality rows.  Returns ``(x, lam, f)``."""
    assert np.array_equal(ref.c_lb, ref.c_ub)
    rhs = np.asarray(ref.c_lb, dtype=np.float64) if rhs is None else rhs
    x, live, lam = np.array(x, dtype=np.float64), ~held, np.zeros(len(ref.c_lb))
    nl = int(live.sum())
    for _ in range(20):
        J, H = dense(ref, x, lam)
        m = J.shape[0]
        r = np.concatenate(((ref.gradient(x) + J.T @ lam)[live], ref.constraints(x) - rhs))
        if np.abs(r).max() <= 1e-13:
            break
        y = np.linalg.solve(np.block([[H[live][:, live], J[:, live].T], [J[:, live], np.zeros((m, m))]]), -r)
        x[live] += y[:nl]
        lam = lam + y[nl:]
    assert np.abs(r).max() <= 1e-13, np.abs(r).max()
    return x, lam, float(ref.objective(x))


def active_sensitivity(ref, x, lam, held, variables=(), rows=()):
    """``(dx (n, k), dlam (m, k), dobj (k))`` of the KKT system with ``held`` kept: column per held variable j of ``variables``
    (its value) then per row i of ``rows`` (its right-hand side) -- the formula of DESIGN.md section 27 on dense arrays."""
    J, H = dense(ref, x, lam)
    n, m = len(x), J.shape[0]
    live = ~held
    nl = int(live.sum())
    K = np.block([[H[live][:, live], J[:, live].T], [J[:, live], np.zeros((m, m))]])
    cols, dobj = [], []
    grad_l = ref.gradient(x) + J.T @ lam
    for j in variables:
        assert held[j]
        cols.append(-np.concatenate((H[live][:, j], J[:, j])))
        dobj.append(grad_l[j])
    for i in rows:
        e = np.zeros(nl + m)
        e[nl + i] = 1.0
        cols.append(e)
        dobj.append(-lam[i])
    S = np.linalg.solve(K, np.array(cols).T) if cols else np.zeros((nl + m, 0))
    dx = np.zeros((n, len(cols)))
    dx[live] = S[:nl]
    for c, j in enumerate(variables):
        dx[j, c] = 1.0
    return dx, S[nl:], np.array(dobj)


def by_differences(ref, x, held, variable=None, row=None, h=1e-5):
    """Central differences of two re-solves: ``(dx, dlam, dobj)`` with respect to the held variable's value or the row's
    right-hand side."""
    out = []
    for sign in (1.0, -1.0):
        xs, rhs = np.array(x, dtype=np.float64), np.array(ref.c_lb, dtype=np.float64)
        if variable is not None:
            xs[variable] += sign * h
        else:
            rhs[row] += sign * h
        out.append(solve_active(ref, xs, held, rhs))
    (xp, lp, fp), (xm, lm, fm) = out
    return (xp - xm) / (2 * h), (lp - lm) / (2 * h), (fp - fm) / (2 * h)
