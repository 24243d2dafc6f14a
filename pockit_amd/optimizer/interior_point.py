"""A primal-dual interior-point solver on the device-resident units of this package: ``solve(system, guess)`` needs no
third-party optimiser.  The iterate -- x, the slacks s of the inequality rows, the multipliers lam of all rows and the bound
multipliers of x and s -- stays in HBM; per iteration only records of a few doubles come down, plus, with
``linear_solver="direct"``, the CSR values of J and H for a host sparse LU.  ``linear_solver="banded"``
factors the step's system on the device instead: no matrix value crosses PCIe.

The problem is ``min f(x)  s.t.  g_i(x) = c_i`` on equality rows (``c_lb == c_ub``), ``g_i(x) - s_i = 0`` with
``c_lb_i <= s_i <= c_ub_i`` on inequality rows, ``v_lb <= x <= v_ub``; a variable with ``v_lb == v_ub`` is fixed and out of the
system, and so is a slot of the NLP vector whose value the transcription dictates (``_common.dictated_slots``: a boundary value
or time that is a number or a function of the static parameters).  Such a slot has no entry in J or H; left free it would be an
empty row and column of the step's matrix.  For the length of a solve the evaluator's variable bounds hold ``lb == ub`` there
(``set_bounds``), and the plan's bounds are put back when ``solve`` returns or raises.  One iteration:

* ``cycle_dev`` / ``gather_csr_dev``: f, grad f, g and the CSR values of J and of the Lagrangian's Hessian;
* ``ip_terms_dev`` on x and on s: ``Sigma``, ``rbar``, complementarity; ``dual_residual_dev``: ``r_d`` and ``b1``;
  ``slack_reduce_dev``: ``S2``, ``b2``, the infeasibility;
* the step ``[[H + Sigma_x + delta_w, J^T], [J, -S2]] (dx, dlam) = (b1, b2)`` -- ``"direct"``: ``scipy.sparse.linalg.splu`` on the
  downloaded values, fixed variables' rows and columns dropped; ``"minres"``: ``minres_begin_dev`` / ``minres_advance_dev`` with
  the diagonal preconditioner, fixed variables decoupled by a unit row (below); ``"banded"``: ``band_factor_dev`` /
  ``band_solve_dev``, a bordered band LU of the same matrix where its values lie (below);
* ``slack_recover_dev``: ds and the inertia-free curvature test ``dx.(H + Sigma_x + delta_w) dx + ds.Sigma_s ds >= 1e-11 (|dx|^2 +
  |ds|^2)``, on failure ``delta_w`` grows (``Regularisation``);
* ``ip_step_dev`` on x and on s: the multiplier steps and the fraction-to-the-boundary lengths;
* a backtracking line search on the l1 merit ``phi_mu + nu theta_1``: ``trial_points_dev``, the x-only batch
  (``cycle_batch_dev``), ``slack_merit_dev``; ``4 B`` doubles and f come back; a trial point with a non-finite f, g, grad f or
  J is rejected like one outside the bounds;
* ``slack_update_dev`` on x and on (s, lam) with the multiplier safeguard ``kappa = 1e10``.

What is NOT here: a feasibility restoration phase, a filter, second-order corrections, Mehrotra steps, warm starts, sharded
contexts.  A step that no trial point of the line search accepts ends the solve with status -2.

``linear_solver="minres"``.  The step is solved where the iterate lies; nothing but records crosses PCIe.  A fixed variable
keeps its row in K; it is decoupled by ``s1_i = 1e20`` and ``b1_i = 0`` (``dual_residual_dev`` writes that zero), so ``dx_i`` is
0 to 1e-20 of the row's coupling, and is then set to 0.0.  FINDING (a CPU prototype on the KKT matrices of
brachistochrone(radau, 10, 8), 565 unknowns): MINRES with this diagonal preconditioner is NOT a usable step solver on real
barrier systems -- 700 to 3 400 iterations per step at ``rtol = 1e-8``, stopping at a true relative residual of 3e-3 ... 0.8
because the preconditioned-norm test is met long before the step is accurate once Sigma spans eight decades; a loop driven by it
stalled at 11 300 iterations per step; an interval-block Schur preconditioner cut the counts only 1.6-6x.  On pure-equality
problems it works: lqr converged in 2-3 Newton iterations with 104 (6 x 6) and 332 (Radau 10 x 10) MINRES iterations.  Use it
there; use ``"direct"`` otherwise.

``linear_solver="banded"``.  ``pockit_amd.band.BandOrdering`` orders K once per solve (the few dense unknowns -- a free final
time -- to a border, reverse Cuthill-McKee on the rest) and ``band_plan`` uploads the plan; per attempt of the regularisation
loop ``band_factor_dev`` assembles K from the resident CSR values with ``Sigma_x + delta_w`` and factors it, ``band_solve_dev``
solves into the step, and the 64-byte record comes down.  A status other than 0 (a singular pivot, a non-finite column) is a
failed attempt, as ``splu``'s ``RuntimeError`` is on the direct path.  No CSR value, ``Sigma_x``, ``S2`` or right-hand side is
downloaded.  LIMIT: pivoting is confined to the band part.  A model whose band part (K without the border's rows and
columns) is singular while K is not gets failed attempts here and should use ``"direct"``; so should a model whose
half-bandwidth exceeds 192 or whose border exceeds 8 unknowns (``BandOrdering`` raises ``ValueError``).

``band_attempts=k`` (1 ... 8, with ``"banded"`` only).  A factorisation is a long serial chain of small
launches, and the schedule of ``delta_w`` is known in advance, so the next k candidates can be factored and solved together:
``band_factor_batch_dev`` / ``band_solve_batch_dev`` take k matrices ``H + Sigma_x + delta_j`` over one J, H, ``S2`` and
right-hand side in the launches of one, the k records come down in one transfer, and the candidates are then walked in the
schedule's order with the same curvature test; the first that passes is the step.  Every entry of a batch has the bits of the
single factorisation, so the iterates, the iteration count and ``regularisations`` do not depend on k.  What it costs: up to
k - 1 factorisations and solves nobody needed (the candidates behind the accepted one), and k bands of device memory instead of
one.  1, the default, is the path without a batch.

``sensitivity``.  A converged solve already holds the matrix that says how the solution moves with a
parameter: ``K = [[H + Sigma_x, J^T], [J, -S2]]`` at ``delta_w = 0``.  A parameter is the value of a variable that equal bounds
hold (a static parameter fixed by ``v_lb == v_ub``: it has a column in J and H though it is out of the system) or the right-hand
side ``c_i`` of an equality row.  At status 0 K is factored once more at the final iterate, with ``Sigma_x`` and ``S2`` of the last
measurement, and one column per parameter is solved: ``-[H_sym[:, j]; J[:, j]]`` over the free rows for variable j,
``[0; e_i]`` for row i.  ``"banded"`` solves all columns in the launches of one solve (``band_solve_multi_dev``, 64 columns per
call) and downloads ``dx``, ``dlam`` and the record; ``"direct"`` uses one ``splu`` on the downloaded values.  The numbers are
those of the BARRIER system at the final mu: they equal the active-set sensitivities up to O(mu) under strict complementarity.
Sensitivities of the bound multipliers and of the slacks are not returned; inequality rows and bounds are not parameters."""
from __future__ import annotations

import math

import numpy as np

from ..evaluator import BAND_REFINE_MAX_STEPS, BAND_REFINE_SINGULAR, BAND_REFINE_TOL
from ._common import dictated_slots, postprocess, preprocess

DEFAULTS = {"tol": 1e-8, "max_iter": 200, "mu_init": 0.1, "print_level": 0}
KAPPA_PUSH = 1e-2            # kappa_1 = kappa_2 of the start's push inside the bounds
KAPPA_EPS = 10.0             # the barrier parameter falls while E_mu <= KAPPA_EPS * mu
KAPPA_CURV = 1e-11           # the inertia-free curvature test
KAPPA_SIGMA = 1e10           # the multiplier safeguard of slack_update_dev
ARMIJO, MAX_TRIALS, TRIAL_BATCH = 1e-8, 25, 8
MAX_REGULARISATIONS = 12
MAX_BAND_ATTEMPTS = 8        # candidates of the schedule taken together with linear_solver="banded" (the unit's cap is 16)
FIXED_S1 = 1e20              # the unit row of a fixed variable on the MINRES path
STATUS = {0: "converged", -1: "maximum number of iterations", -2: "no acceptable step (restoration is not implemented)",
          -13: "a non-finite value"}
INFO_KEYS = ("x", "g", "obj_val", "mult_g", "mult_x_L", "mult_x_U", "status", "status_msg", "iterations", "mu", "error",
             "linear_iterations", "regularisations", "slack", "mult_s_L", "mult_s_U")


# ---------------------------------------------------------------------------- the scalar logic (no device needed)
def options(given):
    """The options with their defaults; an unknown name or a value out of range is a ``ValueError``."""
    out = dict(DEFAULTS)
    for key, value in ({} if given is None else dict(given)).items():
        if key not in DEFAULTS:
            raise ValueError(f"unknown option {key!r} (known: {', '.join(sorted(DEFAULTS))})")
        out[key] = value
    out["tol"], out["mu_init"] = float(out["tol"]), float(out["mu_init"])
    out["max_iter"], out["print_level"] = int(out["max_iter"]), int(out["print_level"])
    if not (out["tol"] > 0.0 and math.isfinite(out["tol"])) or not (out["mu_init"] > 0.0 and math.isfinite(out["mu_init"])) or out["max_iter"] < 0:
        raise ValueError("tol and mu_init must be positive and finite, max_iter not negative")
    return out


def push_inside(v, lb, ub, k1=KAPPA_PUSH, k2=KAPPA_PUSH):
    """``v`` moved inside ``[lb, ub]``: at least ``min(k1 max(1, |lb|), k2 (ub - lb))`` off a finite lower bound, mirrored for the
    upper one, one-sided where only one bound is finite; an element with ``lb == ub`` sits on its bound."""
    v, lb, ub = (np.asarray(a, dtype=np.float64) for a in (v, lb, ub))
    with np.errstate(invalid="ignore"):
        width = np.where(np.isfinite(ub - lb), ub - lb, np.inf)
        pl = np.minimum(k1 * np.maximum(1.0, np.abs(lb)), k2 * width)
        pu = np.minimum(k1 * np.maximum(1.0, np.abs(ub)), k2 * width)
        out = np.where(np.isfinite(lb), np.maximum(v, lb + pl), v)
        out = np.where(np.isfinite(ub), np.minimum(out, ub - pu), out)
    return np.where(lb == ub, lb, out)


def dual_scale(lam_1, z_sum, rows, sides):
    """``s_d = max(100, (|lam|_1 + sum z) / (m + sides)) / 100``."""
    count = rows + sides
    return max(100.0, (lam_1 + z_sum) / count) / 100.0 if count > 0 else 1.0


def barrier_error(r_d_inf, r_s_inf, theta_inf, compl_inf, s_d):
    """``E_mu = max(|r_d|_inf / s_d, |r_s|_inf / s_d, theta_inf, compl_inf(mu) / s_d)``."""
    return max(r_d_inf / s_d, r_s_inf / s_d, theta_inf, compl_inf / s_d)


def next_mu(mu, tol):
    """``max(tol / 10, min(0.2 mu, mu^1.5))``."""
    return max(tol / 10.0, min(0.2 * mu, mu ** 1.5))


def barrier_falls(error_mu, mu, tol):
    """Does the barrier parameter fall at this error?"""
    return error_mu <= KAPPA_EPS * mu and mu > tol / 10.0


def fraction_to_boundary(mu):
    return max(0.99, 1.0 - mu)


def penalty(lam_trial_inf, slope, curvature, theta_1):
    """``nu = max(1, |lam + dlam|_inf, (slope + max(curvature, 0) / 2) / (0.9 theta_1))``, the smallest value the rule allows,
    taken anew in every iteration (a value carried over from an early iteration, where ``|lam + dlam|`` is large, stalls the
    line search later: DESIGN.md section 22); ``slope = grad phi_mu . d``.  Without infeasibility the quotient has no say."""
    need = max(1.0, lam_trial_inf)
    if theta_1 > 0.0:
        need = max(need, (slope + 0.5 * max(curvature, 0.0)) / (0.9 * theta_1))
    return need


def armijo(merit_trial, merit_0, alpha, slope_merit):
    """``merit(alpha) <= merit(0) + 1e-8 alpha D`` with ``D = slope - nu theta_1`` (allowing for the rounding of the two
    merits themselves: ten ulps of their size)."""
    slack = 10.0 * np.finfo(np.float64).eps * abs(merit_0)
    return bool(np.isfinite(merit_trial)) and merit_trial <= merit_0 + ARMIJO * alpha * slope_merit + slack


def trial_lengths(alpha_max, done, count=TRIAL_BATCH):
    """The next lengths of the backtracking: ``alpha_max / 2^k`` for k = done ... , at most ``count`` and MAX_TRIALS in all."""
    return [alpha_max * 0.5 ** k for k in range(done, min(done + count, MAX_TRIALS))]


class Regularisation:
    """The schedule of ``delta_w``: 0 first; on a failed curvature test ``max(1e-4, last / 3)`` (``last``: the value the last
    regularised step succeeded with), then times 8 -- times 100 while no ``last`` exists --, MAX_REGULARISATIONS attempts."""

    def __init__(self):
        self.last = None
        self.count = 0              # regularised attempts over the whole solve

    def attempts(self):
        """Yield the ``delta_w`` to try for one step; call ``accept(delta)`` for the one that passed."""
        delta = 0.0
        yield delta
        for k in range(MAX_REGULARISATIONS):
            if k == 0:
                delta = 1e-4 if self.last is None else max(1e-4, self.last / 3.0)
            else:
                delta *= 100.0 if self.last is None else 8.0
            self.count += 1
            yield delta

    def accept(self, delta):
        if delta > 0.0:
            self.last = delta

    def schedule(self):
        """The ``delta_w`` that ``attempts()`` would yield for one step, as a list, without counting any of them: the schedule
        is a function of ``last`` alone."""
        ahead = Regularisation()
        ahead.last = self.last
        return list(ahead.attempts())

    def batches(self, k):
        """The schedule of one step, k values at a time (the last batch is shorter where k does not divide), without counting.
        Whoever takes candidates together walks each batch in order, calls ``tried(delta)`` for every candidate it looks at and
        ``accept(delta)`` for the one that passed: ``last`` and ``count`` then end as ``attempts()`` leaves them."""
        values = self.schedule()
        for lo in range(0, len(values), int(k)):
            yield values[lo: lo + int(k)]

    def tried(self, delta):
        if delta > 0.0:
            self.count += 1


def derivatives_finite(grad_batch, jac_batch, k, n, nnz_j):
    """Are grad f and J finite at entry k of the line search's batch (torch tensors, dense ``[B][n]`` and ``[B][nnz_J]``)?  On
    the edge of a model's domain f and g can be finite where a derivative is not (``sqrt`` at 0): such a trial point may pass
    the Armijo test, and adopting it ends the solve with status -13 one iteration later.  It is rejected like a point outside."""
    grad, jac = grad_batch[k * n: (k + 1) * n], jac_batch[k * nnz_j: (k + 1) * nnz_j]
    return bool(grad.isfinite().all().item()) and bool(jac.isfinite().all().item())


def make_info(status, **fields):
    info = dict(fields, status=int(status), status_msg=STATUS[int(status)])
    missing = [k for k in INFO_KEYS if k not in info]
    if missing:
        raise KeyError(f"info lacks {missing}")
    return info


# ---------------------------------------------------------------------------- the direct step solver (host LU on downloaded values)
class DirectKkt:
    """The structure of ``K = [[H + diag(s1), J^T], [J, -diag(s2)]]`` over the free variables and all rows, assembled ONCE from
    the CSR maps of J and H: ``values(...)`` are the CSC data of K as one sparse product with the downloaded value arrays."""

    def __init__(self, map_j, map_h, free):
        import scipy.sparse as sp

        n, m = len(free), map_j.shape[0]
        self.n, self.m, self.free = n, m, free
        col_of = np.cumsum(free) - 1
        self.nf = nf = int(free.sum())
        N = self.N = nf + m
        hs = map_h.symmetric()
        h_rows = np.repeat(np.arange(n), np.diff(hs.indptr))
        h_cols, h_src = hs.indices.astype(np.int64), hs.src.astype(np.int64)
        keep = free[h_rows] & free[h_cols]
        j_rows = np.repeat(np.arange(m), np.diff(map_j.indptr))
        j_cols = map_j.indices.astype(np.int64)
        j_keep = free[j_cols]
        off_j, off_s1, off_s2 = map_h.nnz, map_h.nnz + map_j.nnz, map_h.nnz + map_j.nnz + n
        idx_free = np.flatnonzero(free)
        jr, jc, je = nf + j_rows[j_keep], col_of[j_cols[j_keep]], off_j + np.flatnonzero(j_keep)
        rows = np.concatenate((col_of[h_rows[keep]], col_of[idx_free], jr, jc, nf + np.arange(m)))
        cols = np.concatenate((col_of[h_cols[keep]], col_of[idx_free], jc, jr, nf + np.arange(m)))
        src = np.concatenate((h_src[keep], off_s1 + idx_free, je, je, off_s2 + np.arange(m)))
        sign = np.concatenate((np.ones(len(rows) - m), -np.ones(m)))
        keys, inverse = np.unique(cols * N + rows, return_inverse=True)
        self.indices = (keys % N).astype(np.int32)
        self.indptr = np.searchsorted(keys // N, np.arange(N + 1)).astype(np.int32)
        self.select = sp.csr_array((sign, (inverse, src)), shape=(len(keys), off_s2 + m))

    def solve(self, hvals, jvals, s1, s2, rhs):
        """``(dx (n), dlam (m))`` of ``K (dx, dlam) = rhs`` (``rhs`` of n + m values; fixed variables get 0.0).  Raises
        ``RuntimeError`` where the factorisation finds K singular."""
        import scipy.sparse as sp
        from scipy.sparse.linalg import splu

        data = self.select @ np.concatenate((hvals, jvals, s1, s2))
        K = sp.csc_matrix((data, self.indices, self.indptr), shape=(self.N, self.N))
        b = np.concatenate((rhs[: self.n][self.free], rhs[self.n:]))
        y = splu(K).solve(b)
        dx = np.zeros(self.n)
        dx[self.free] = y[: self.nf]
        return dx, y[self.nf:]

    def solve_block(self, hvals, jvals, s1, s2, rhs):
        """``solve`` for the k rows of ``rhs`` (k, n + m) against ONE factorisation: ``(dx (k, n), dlam (k, m))``."""
        import scipy.sparse as sp
        from scipy.sparse.linalg import splu

        data = self.select @ np.concatenate((hvals, jvals, s1, s2))
        K = sp.csc_matrix((data, self.indices, self.indptr), shape=(self.N, self.N))
        b = np.concatenate((rhs[:, : self.n][:, self.free], rhs[:, self.n:]), axis=1)
        y = splu(K).solve(np.asfortranarray(b.T)).T
        dx = np.zeros((len(rhs), self.n))
        dx[:, self.free] = y[:, : self.nf]
        return dx, np.ascontiguousarray(y[:, self.nf:])


# ---------------------------------------------------------------------------- the resident iterate and the loop
class _Resident:
    """The device arrays of a solve (torch tensors) and the evaluator's calls on them.  The evaluator's kernels run on the
    context's stream, torch's few vector operations on torch's: ``to_torch`` / ``to_kernels`` order the two."""

    def __init__(self, system, x0):
        import torch

        self.torch, self.ev = torch, system.evaluator
        ev, p = self.ev, system.plan
        if ev.src.sharded:
            raise NotImplementedError("the interior-point solver is not offered for a sharded evaluator")
        self.n, self.m = n, m = p.n, p.m
        self.dev = torch.device("cuda", int(getattr(ev, "device", 0)))
        self.v_lb, self.v_ub, self.c_lb, self.c_ub = (np.array(a, dtype=np.float64) for a in (p.v_lb, p.v_ub, p.c_lb, p.c_ub))
        # a slot whose value the transcription dictates is a variable of the NLP vector that nothing reads: no entry in J or H,
        # bounds (-inf, inf) or the state's.  Left free it is an empty row and column of K, so it is fixed
        # here: at the dictated value (FIXED), at the start's value (FUNC: the kernels substitute the real one)
        fixed_at, fixed_to, func = dictated_slots(system)
        func_at = np.array([slot for slot, _, _ in func], dtype=np.int64)
        x0 = np.array(x0, dtype=np.float64)
        self.v_lb[fixed_at] = self.v_ub[fixed_at] = fixed_to
        self.v_lb[func_at] = self.v_ub[func_at] = np.where(np.isfinite(x0[func_at]), x0[func_at], 0.0)
        self.free = self.v_lb != self.v_ub
        self.ineq = self.c_lb != self.c_ub
        if np.any(self.ineq & ~np.isfinite(self.c_lb) & ~np.isfinite(self.c_ub)):
            raise ValueError("a constraint row without a finite bound constrains nothing: drop it from the model")
        self.map_j, self.map_h = ev.csr_map("jac"), ev.csr_map("hess")
        for op in ("J", "JT", "H"):
            ev._operator(op)
        ev._operator_diagonal()
        z = self.zeros
        self.x, self.lam = self.up(push_inside(x0, self.v_lb, self.v_ub)), z(m)
        side = lambda present: self.up(np.where(present, 1.0, 0.0))  # noqa: E731
        self.zl, self.zu = side(self.free & np.isfinite(self.v_lb)), side(self.free & np.isfinite(self.v_ub))
        self.yl, self.yu = side(self.ineq & np.isfinite(self.c_lb)), side(self.ineq & np.isfinite(self.c_ub))
        self.s = z(m)
        self.ineq_mask, self.free_mask = self.up(self.ineq.astype(np.float64)), self.up(self.free.astype(np.float64))
        self.fixed_s1 = self.up(np.where(self.free, 0.0, FIXED_S1))
        self.f, self.grad, self.g = z(1), z(n), z(m)
        self.jt, self.ht = z(p.nnz_J), z(p.nnz_H)                       # triplet values of one cycle
        self.cj, self.ch = z(self.map_j.nnz), z(self.map_h.nnz)          # their CSR values
        self.sig_x, self.rbar_x, self.sig_s, self.rbar_s = z(n), z(n), z(m), z(m)
        self.scr_x, self.scr_x2, self.scr_s, self.scr_s2 = z(n), z(n), z(m), z(m)
        self.s1, self.s2, self.rhs, self.sol, self.w, self.ds, self.r_d = z(n), z(m), z(n + m), z(n + m), z(n), z(m), z(n)
        self.dzl, self.dzu, self.dyl, self.dyu = z(n), z(n), z(m), z(m)
        self.minv = z(n + m)
        self.rec = z(64)
        self.batch = None
        ev.set_bounds(v_lb=self.v_lb, v_ub=self.v_ub)       # (last: solve() puts the plan's back once this has been said)

    def zeros(self, count):
        return self.torch.zeros(max(int(count), 1), dtype=self.torch.float64, device=self.dev)

    def up(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        t = self.zeros(len(a))
        if len(a):
            t[: len(a)] = self.torch.from_numpy(a)
        return t

    def to_torch(self):
        self.ev.sync()

    def to_kernels(self):
        self.torch.cuda.synchronize()

    def down(self, t, count=None):
        a = t.cpu().numpy()
        return a if count is None else a[:count]

    @staticmethod
    def at(t, offset=0):
        return t.data_ptr() + 8 * int(offset)

    # ---- one evaluation at (x, lam): f, grad, g, CSR values of J and H
    def evaluate(self):
        ev, at = self.ev, self.at
        self.to_kernels()
        ev._invalidate_x()
        ev.cycle_dev(at(self.x), at(self.lam), 1.0, at(self.f), at(self.grad), at(self.g), at(self.jt), at(self.ht))
        ev.gather_csr_dev("jac", at(self.jt), at(self.cj))
        ev.gather_csr_dev("hess", at(self.ht), at(self.ch))

    # ---- the records of the iterate at mu: [terms x (8) | terms s (8) | terms x at 0 (8) | terms s at 0 (8) | r_d (4) | reduce (4)]
    def measure(self, mu):
        ev, at, rec, torch = self.ev, self.at, self.rec, self.torch
        self.to_torch()
        z = self.zl - self.zu
        r_s = ((-self.lam - self.yl + self.yu) * self.ineq_mask)[: self.m]
        r_s_inf = float(r_s.abs().max().item()) if self.m else 0.0
        lam_1 = float(self.lam[: self.m].abs().sum().item())
        self.to_kernels()
        ev.ip_terms_dev(at(self.x), at(self.zl), at(self.zu), mu, at(self.sig_x), at(self.rbar_x), at(rec, 0))
        ev.ip_terms_dev(at(self.s), at(self.yl), at(self.yu), mu, at(self.sig_s), at(self.rbar_s), at(rec, 8), which="c")
        ev.ip_terms_dev(at(self.x), at(self.zl), at(self.zu), 0.0, at(self.scr_x), at(self.scr_x2), at(rec, 16))
        ev.ip_terms_dev(at(self.s), at(self.yl), at(self.yu), 0.0, at(self.scr_s), at(self.scr_s2), at(rec, 24), which="c")
        ev.dual_residual_dev(at(self.cj), at(self.grad), at(self.lam), at(self.r_d), at(rec, 32), d_z=at(z))
        ev.slack_reduce_dev(at(self.g), at(self.s), at(self.lam), at(self.sig_s), at(self.rbar_s), at(self.s2), at(self.rhs, self.n), at(rec, 36))
        self.to_torch()
        r = self.down(rec)
        tx, ts, tx0, ts0, rd, red = r[0:8], r[8:16], r[16:24], r[24:32], r[32:36], r[36:40]
        del torch
        return dict(tx=tx, ts=ts, tx0=tx0, ts0=ts0, rd=rd, red=red, r_s_inf=r_s_inf, lam_1=lam_1, f=float(self.down(self.f)[0]))


def _errors(q, m):
    """(E_0, E_mu, bad) from the records of ``_Resident.measure``."""
    tx, ts, tx0, ts0, rd, red = q["tx"], q["ts"], q["tx0"], q["ts0"], q["rd"], q["red"]
    s_d = dual_scale(q["lam_1"], tx[6] + ts[6], m, tx[2] + ts[2])
    e_mu = barrier_error(rd[0], q["r_s_inf"], red[0], max(tx[0], ts[0]), s_d)
    e_0 = barrier_error(rd[0], q["r_s_inf"], red[0], max(tx0[0], ts0[0]), s_d)
    bad = tx[5] + ts[5] + rd[2] + red[2]
    finite = all(np.all(np.isfinite(a)) for a in (tx[:3], ts[:3], rd, red)) and math.isfinite(q["f"]) and math.isfinite(q["r_s_inf"])
    return e_0, e_mu, (bad > 0.0 or not finite)


SENSITIVITY_ROUTE = ("a slot whose value the transcription dictates has no column in J or H and cannot be a parameter: make the value a "
                     "FUNC of a static parameter and fix that parameter by equal bounds")


def sensitivity_parameters(system, sensitivity, linear_solver):
    """The parameters ``solve(..., sensitivity=...)`` asks for as a list of ``("variable", slot)`` and ``("row", row)``, or None;
    every ``ValueError`` of the argument is raised here, from the plan alone (no device needed)."""
    if sensitivity is None:
        return None
    if linear_solver == "minres":
        raise ValueError('sensitivity needs linear_solver="direct" or "banded": the "minres" path has no factorisation to reuse')
    plan = system.plan
    n, m = plan.n, plan.m
    fixed = np.asarray(plan.v_lb, dtype=np.float64) == np.asarray(plan.v_ub, dtype=np.float64)
    equality = np.asarray(plan.c_lb, dtype=np.float64) == np.asarray(plan.c_ub, dtype=np.float64)
    fixed_at, _, func = dictated_slots(system)
    dictated = set(int(j) for j in fixed_at) | set(int(slot) for slot, _, _ in func)
    if isinstance(sensitivity, str):
        if sensitivity != "fixed":
            raise ValueError('sensitivity must be None, "fixed" or a mapping with "variables" and "rows"')
        used = np.zeros(n, dtype=bool)
        for index in (plan.jac_col, plan.hess_row, plan.hess_col):
            used[np.asarray(index, dtype=np.int64)] = True
        return [("variable", int(j)) for j in np.flatnonzero(fixed & used) if int(j) not in dictated]
    try:
        unknown = set(sensitivity) - {"variables", "rows"}
        variables, rows = list(sensitivity.get("variables", ())), list(sensitivity.get("rows", ()))
    except (TypeError, AttributeError):
        raise ValueError('sensitivity must be None, "fixed" or a mapping with "variables" and "rows"') from None
    if unknown:
        raise ValueError(f'sensitivity: unknown keys {sorted(unknown)} (known: "variables", "rows")')
    out = []
    for j in variables:
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 0 <= j < n:
            raise ValueError(f"sensitivity: variable {j!r} is not an NLP slot in 0 ... {n - 1}")
        if int(j) in dictated:
            raise ValueError(f"sensitivity: variable {int(j)}: {SENSITIVITY_ROUTE}")
        if not fixed[j]:
            raise ValueError(f"sensitivity: variable {int(j)} is free (v_lb != v_ub): only a variable held by equal bounds is a parameter")
        out.append(("variable", int(j)))
    for i in rows:
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i < m:
            raise ValueError(f"sensitivity: row {i!r} is not a constraint row in 0 ... {m - 1}")
        if not equality[i]:
            raise ValueError(f"sensitivity: row {int(i)} is an inequality row (c_lb != c_ub): only the right-hand side of an equality row is a parameter")
        out.append(("row", int(i)))
    return out


SENSITIVITY_CHUNK = 64       # the right-hand sides of one band_solve_multi_dev


def _sensitivities(R, params, direct, status):
    """``info["sensitivity"]`` at the final iterate of ``R`` (``R.sig_x``, ``R.s2``, ``R.cj``, ``R.ch`` of the last measurement
    and evaluation): K at ``delta_w = 0`` factored once, one column per parameter."""
    out = {"parameters": list(params), "dx": None, "dlam": None, "dobj": None, "status": "not_converged", "record": None}
    if status != 0:
        return out
    ev, at, torch, n, m = R.ev, R.at, R.torch, R.n, R.m
    N, k = n + m, len(params)
    var_cols = [(c, j) for c, (kind, j) in enumerate(params) if kind == "variable"]
    row_cols = [(c, i) for c, (kind, i) in enumerate(params) if kind == "row"]
    # ---- dobj of a variable: grad f_j + (J^T lam)_j, the k picked entries alone come down
    dobj = np.zeros(k)
    R.to_kernels()
    ev.apply_operator_dev("JT", at(R.cj), at(R.lam), at(R.w))
    R.to_torch()
    if var_cols:
        pick = torch.tensor([j for _, j in var_cols], dtype=torch.int64, device=R.dev)
        dobj[[c for c, _ in var_cols]] = R.down((R.grad[:n] + R.w[:n])[pick])
    if row_cols:
        pick = torch.tensor([i for _, i in row_cols], dtype=torch.int64, device=R.dev)
        dobj[[c for c, _ in row_cols]] = -R.down(R.lam[:m][pick])
    out["dobj"] = dobj
    dx, dlam, record = np.zeros((k, n)), np.zeros((k, m)), None
    if k and direct is not None:
        import scipy.sparse as sp

        hvals, jvals, sig_x, s2 = (R.down(t, c).copy() for t, c in ((R.ch, R.map_h.nnz), (R.cj, R.map_j.nnz), (R.sig_x, n), (R.s2, m)))
        hs = R.map_h.symmetric()
        H = sp.csc_matrix(sp.csr_matrix((hvals[hs.src], hs.indices, hs.indptr), shape=(n, n)))
        J = sp.csc_matrix(sp.csr_matrix((jvals, R.map_j.indices, R.map_j.indptr), shape=(m, n)))
        rhs = np.zeros((k, N))
        for c, j in var_cols:
            rhs[c, :n], rhs[c, n:] = -H[:, [j]].toarray()[:, 0], -J[:, [j]].toarray()[:, 0]
        for c, i in row_cols:
            rhs[c, n + i] = 1.0
        try:
            dx, dlam = direct.solve_block(hvals, jvals, sig_x, s2, rhs)
        except RuntimeError:
            dx = None
    elif k:
        V = torch.zeros((k, max(N, 1)), dtype=torch.float64, device=R.dev)
        rhs, sol = torch.zeros_like(V), torch.zeros_like(V)
        for c, j in var_cols:
            V[c, j] = -1.0
        for c, i in row_cols:
            rhs[c, n + i] = 1.0
        R.to_kernels()
        for c, _ in var_cols:      # -[H_sym[:, j]; J[:, j]] = K (-e_j) with s1 = s2 = NULL; the gather drops the fixed rows
            ev.kkt_apply_dev(at(R.cj), at(V[c]), at(rhs[c]), d_hvals=at(R.ch))
        ev.band_factor_dev(at(R.ch), at(R.cj), at(R.sig_x), at(R.s2))
        stride = max(N, 1)
        for lo in range(0, k, SENSITIVITY_CHUNK):
            ev.band_solve_multi_dev(min(SENSITIVITY_CHUNK, k - lo), at(rhs[lo]), at(sol[lo]), stride_rhs=stride, stride_sol=stride)
        record = ev.band_record()
        R.to_torch()
        if record[0] == 0.0:
            S = R.down(sol.reshape(-1), k * stride).reshape(k, stride)
            dx, dlam = S[:, :n].copy(), S[:, n: n + m].copy()
        else:
            dx = None
    out["record"] = record
    if dx is None or not (np.all(np.isfinite(dx)) and np.all(np.isfinite(dlam))):
        out["status"] = "singular"
        out["dobj"] = None
        return out
    for c, j in var_cols:
        dx[c, j] = 1.0          # (the parameter itself; every other fixed variable stays 0.0)
    out.update(dx=np.ascontiguousarray(dx.T), dlam=np.ascontiguousarray(dlam.T), status="ok")
    return out


def solve(system, guess, optimizer_options=None, *, linear_solver="direct", band_attempts=1, sensitivity=None, band_refine=0):
    """Solve the NLP of ``system`` from ``guess`` (the shapes of ``ipopt.solve``); returns ``(solution, info)``.  ``info`` has
    cyipopt's keys ``x, g, obj_val, mult_g, mult_x_L, mult_x_U, status, status_msg`` and ``iterations``, ``mu``, ``error`` (the
    final E_0), ``linear_iterations`` (MINRES iterations in all; 0 on the direct and banded paths), ``regularisations``, and the slacks with
    their multipliers ``slack, mult_s_L, mult_s_U`` (m values; 0.0 on equality rows).  ``status``: 0 converged (``E_0 <= tol``),
    -1 maximum iterations, -2 no acceptable step, -13 a non-finite value.  Options: ``tol`` (1e-8), ``max_iter`` (200),
    ``mu_init`` (0.1), ``print_level`` (0; 1 prints a line per iteration, 2 the step's figures as well, 3 every trial point).  ``linear_solver``: "direct", "minres" or
    "banded" (module docstring: where the latter two work); with "banded" a ``ValueError`` of the ordering (band too wide, border
    too large) leaves the choice of "direct" to the caller.  ``band_attempts`` (1 ... 8, "banded" only): how many ``delta_w`` of the
    regularisation schedule are factored and solved together (module docstring); the iterates do not depend on it.
    ``band_refine`` (0 ... 10, "banded" only, not with ``band_attempts > 1``): the most corrections of the iterative refinement every
    band solve gets against the true K (``band_refine_begin_dev``: tolerance 1e-10 on the residual ratio, the device decides); an
    attempt whose final ratio exceeds 1e-5, or whose refinement met a non-finite value, counts as a failed factorisation.  Then
    ``info`` has ``refinement_steps`` (corrections in all) and ``residual_ratio`` (the largest ratio of an accepted step).  With 0 no
    call is added and neither key appears.

    ``sensitivity`` (with "direct" or "banded"): None, ``"fixed"`` -- every variable that equal bounds hold, that is not a slot the
    transcription dictates and that has a non-empty column in J or H -- or a mapping ``{"variables": [NLP slots], "rows":
    [constraint rows]}`` of variables held by equal bounds and of equality rows.  Then ``info["sensitivity"]`` is a dict:
    ``parameters`` (``("variable", slot)`` / ``("row", row)`` in column order), ``dx`` (n x k: the derivative of the solution with
    respect to the variable's value or the row's right-hand side; row j of a variable's own column is 1, other fixed rows 0),
    ``dlam`` (m x k), ``dobj`` (k: ``grad f_j + (J^T lam)_j`` for a variable, ``-lam_i`` for a row), ``status`` -- ``"ok"``,
    ``"not_converged"`` (the solve did not end with status 0) or ``"singular"`` (the factorisation at ``delta_w = 0`` failed); the
    arrays are None unless ``"ok"`` -- and ``record`` (the band record, None on the direct path).  The numbers are those of the
    barrier system at the final mu: they equal the active-set sensitivities up to O(mu) under strict complementarity.  Bound-
    multiplier and slack sensitivities are not returned.  ``ValueError`` before any device work: "minres", a free variable, a
    dictated slot (route: a FUNC of a static parameter fixed by bounds), an inequality row, an index out of range."""
    if linear_solver not in ("direct", "minres", "banded"):
        raise ValueError('linear_solver must be "direct", "minres" or "banded"')
    if isinstance(band_attempts, bool) or not isinstance(band_attempts, (int, np.integer)) or not 1 <= band_attempts <= MAX_BAND_ATTEMPTS:
        raise ValueError(f"band_attempts must be an integer in 1 ... {MAX_BAND_ATTEMPTS}")
    if band_attempts != 1 and linear_solver != "banded":
        raise ValueError('band_attempts other than 1 needs linear_solver="banded"')
    band_attempts = int(band_attempts)
    if isinstance(band_refine, bool) or not isinstance(band_refine, (int, np.integer)) or not 0 <= band_refine <= BAND_REFINE_MAX_STEPS:
        raise ValueError(f"band_refine must be an integer in 0 ... {BAND_REFINE_MAX_STEPS}")
    if band_refine and linear_solver != "banded":
        raise ValueError('band_refine other than 0 needs linear_solver="banded"')
    if band_refine and band_attempts > 1:
        raise ValueError("band_refine is not offered with band_attempts > 1: the batch form is not refined")
    band_refine = int(band_refine)
    opt = options(optimizer_options)
    params = sensitivity_parameters(system, sensitivity, linear_solver)
    x0, bare, _ = preprocess(system, guess, None)
    R = _Resident(system, x0)
    try:
        return _iterate(system, R, opt, bare, linear_solver, band_attempts, params, band_refine)
    finally:
        R.ev.set_bounds()            # the plan's bounds again: a later merit_scan measures against them, not against the fixed slots


def _iterate(system, R, opt, bare, linear_solver, band_attempts, params=None, band_refine=0):
    """The loop of ``solve`` on the resident iterate ``R``."""
    ev, at, torch, n, m = R.ev, R.at, R.torch, R.n, R.m
    tol, mu = opt["tol"], opt["mu_init"]
    direct = DirectKkt(R.map_j, R.map_h, R.free) if linear_solver == "direct" else None
    banded = linear_solver == "banded"
    if banded:
        from ..band import BandOrdering

        ev.band_plan(BandOrdering(R.map_j, R.map_h, R.free))

    # ---- the start: s = g(x) pushed inside the rows' bounds
    R.evaluate()
    R.to_torch()
    g0 = R.down(R.g, m)
    R.s = R.up(np.where(R.ineq, push_inside(g0, R.c_lb, R.c_ub), 0.0))
    reg = Regularisation()

    def passes(delta):
        """ds and the curvature test on the step in ``R.sol`` with ``R.s1 = Sigma_x + delta``: ``(curvature, delta, |step|^2)`` or
        None."""
        ev.apply_operator_dev("H", at(R.ch), at(R.sol), at(R.w))
        ev.slack_recover_dev(at(R.sol, n), at(R.lam), at(R.rbar_s), at(R.s2), at(R.sig_s), at(R.sol), at(R.w), at(R.s1), at(R.ds), at(R.rec, 44))
        R.to_torch()
        rc = R.down(R.rec)[44:49]
        curvature, step_sq = rc[0] + rc[1], rc[2] + rc[3]
        if rc[4] == 0.0 and np.all(np.isfinite(rc)) and curvature >= KAPPA_CURV * step_sq:
            reg.accept(delta)
            return curvature, delta, step_sq
        return None

    iterations = linear_iterations = refinement_steps = 0
    residual_ratio = 0.0
    status, e_0 = -1, math.inf
    while True:
        q = R.measure(mu)
        e_0, e_mu, broken = _errors(q, m)
        if opt["print_level"] > 0:
            print(f"{iterations:4d}  f {q['f']: .10e}  theta {q['red'][0]:.2e}  r_d {q['rd'][0]:.2e}  E_0 {e_0:.2e}  mu {mu:.1e}  delta_w {reg.last or 0.0:.1e}")
        if broken:
            status = -13
            break
        if e_0 <= tol:
            status = 0
            break
        if barrier_falls(e_mu, mu, tol):
            mu = next_mu(mu, tol)
            continue
        if iterations >= opt["max_iter"]:
            status = -1
            break
        tau = fraction_to_boundary(mu)
        # ---- the step
        ev.dual_residual_dev(at(R.cj), at(R.grad), at(R.lam), at(R.rhs), at(R.rec, 40), d_z=at(R.rbar_x), negate=True)
        R.to_torch()
        if direct is not None:
            hvals, jvals, sig_x, s2, rhs = (R.down(t, c).copy() for t, c in ((R.ch, R.map_h.nnz), (R.cj, R.map_j.nnz), (R.sig_x, n), (R.s2, m),
                                                                              (R.rhs, n + m)))
        step = None
        # ---- band_attempts > 1: the next candidates of the schedule factored and solved together, then walked in order
        for deltas in (reg.batches(band_attempts) if band_attempts > 1 else ()):
            k = len(deltas)
            s1_rows = torch.stack([R.sig_x[:n] + delta for delta in deltas]) if n else torch.zeros((k, 1), dtype=torch.float64, device=R.dev)
            sol_rows = torch.zeros((k, max(n + m, 1)), dtype=torch.float64, device=R.dev)
            R.to_kernels()
            ev.band_factor_batch_dev(k, at(R.ch), at(R.cj), at(s1_rows), at(R.s2), strides=(0, 0, n, 0))
            ev.band_solve_batch_dev(k, at(R.rhs), at(sol_rows), stride_rhs=0, stride_sol=n + m)
            records = ev.band_record_batch(k)
            for j, delta in enumerate(deltas):
                reg.tried(delta)
                if records[j, 0] != 0.0 or not np.all(np.isfinite(records[j])):
                    continue
                R.s1, R.sol = s1_rows[j], sol_rows[j]
                R.to_kernels()
                step = passes(delta)
                if step is not None:
                    if opt["print_level"] > 1:
                        print(f"      band batch of {k}: candidate {j} taken, delta_w {delta:.1e}")
                    break
            if step is not None:
                break
        for delta in (reg.attempts() if band_attempts == 1 else ()):
            R.s1 = R.sig_x + delta                        # (the curvature test's Sigma_x + delta_w)
            if direct is not None:
                try:
                    dx, dlam = direct.solve(hvals, jvals, sig_x + delta, s2, rhs)
                except RuntimeError:
                    continue
                if not (np.all(np.isfinite(dx)) and np.all(np.isfinite(dlam))):
                    continue
                R.sol = R.up(np.concatenate((dx, dlam)))
                R.to_kernels()
            elif banded:
                R.to_kernels()
                ev.band_factor_dev(at(R.ch), at(R.cj), at(R.s1), at(R.s2))
                ev.band_solve_dev(at(R.rhs), at(R.sol))
                if band_refine:
                    ev.band_refine_begin_dev(at(R.ch), at(R.cj), at(R.s1), at(R.s2), at(R.rhs), at(R.sol), BAND_REFINE_TOL, 0)
                br = ev.band_record()
                if br[0] != 0.0 or not np.all(np.isfinite(br)):
                    continue
                if band_refine:
                    rr = ev.band_refine_record()
                    while rr[0] == 0.0 and rr[1] < band_refine:
                        ev.band_refine_advance_dev(1)
                        rr = ev.band_refine_record()
                    refinement_steps += int(rr[1])
                    if rr[0] in (3.0, 4.0) or not rr[5] <= BAND_REFINE_SINGULAR:
                        continue
                    attempt_ratio = float(rr[5])
            else:
                k_s1 = R.s1 + R.fixed_s1
                R.to_kernels()
                ev.operator_diagonal_dev("H", at(R.ch), at(R.minv), d_add=at(k_s1))
                R.to_torch()
                m1 = R.minv[:n].abs()
                m1 = torch.where((m1 > 0) & torch.isfinite(m1), 1.0 / m1, torch.ones_like(m1))
                R.minv[:n] = m1
                R.to_kernels()
                ev.operator_reduce_dev("J", "sq_sum", at(R.cj), at(R.minv, n), d_w=at(R.minv), d_add=at(R.s2))
                R.to_torch()
                m2 = R.minv[n: n + m].abs()
                R.minv[n: n + m] = torch.where((m2 > 0) & torch.isfinite(m2), 1.0 / m2, torch.ones_like(m2))
                R.to_kernels()
                ev.minres_begin_dev(at(R.cj), at(R.rhs), at(R.sol), min(1e-8, 0.01 * e_mu), d_hvals=at(R.ch), d_s1=at(k_s1), d_s2=at(R.s2),
                                    d_minv=at(R.minv))
                cap, done, mr = 20 * (n + m) + 200, 0, None
                while done < cap:
                    ev.minres_advance_dev(64)
                    done += 64
                    mr = ev.minres_record()
                    if mr[0] != 0:
                        break
                linear_iterations += int(mr[1])
                if mr[0] in (2, 3):
                    continue
                R.to_torch()
                R.sol[:n] *= R.free_mask[:n]
                R.to_kernels()
            step = passes(delta)
            if step is not None:
                if band_refine:
                    residual_ratio = max(residual_ratio, attempt_ratio)
                break
        if step is None:
            status = -2
            break
        curvature = step[0]
        # ---- the lengths
        R.to_kernels()
        ev.ip_step_dev(at(R.x), at(R.sol), at(R.zl), at(R.zu), mu, tau, at(R.dzl), at(R.dzu), at(R.rec, 52))
        ev.ip_step_dev(at(R.s), at(R.ds), at(R.yl), at(R.yu), mu, tau, at(R.dyl), at(R.dyu), at(R.rec, 56), which="c")
        R.to_torch()
        sx, ss = R.down(R.rec)[52:56], R.down(R.rec)[56:60]
        if sx[3] + ss[3] > 0.0:
            status = -13
            break
        alpha_max, alpha_d = min(sx[0], ss[0]), min(sx[1], ss[1])
        dx_t, dlam_t = R.sol[:n], R.sol[n: n + m]
        slope = float((torch.dot(R.grad[:n] - R.rbar_x[:n], dx_t) - torch.dot(R.rbar_s[:m], R.ds[:m])).item())
        lam_trial_inf = float((R.lam[:m] + dlam_t).abs().max().item()) if m else 0.0
        theta_1 = float(q["red"][1])
        nu = penalty(lam_trial_inf, slope, curvature, theta_1)
        slope_merit = slope - nu * theta_1
        # ---- the line search: the first batch holds the full step and, as its second entry, alpha = 0 -- the merit of the
        # iterate itself through the same kernels, so that both sides of the Armijo test carry the same rounding
        accepted, done, merit_0 = None, 0, None
        while accepted is None and done < MAX_TRIALS:
            alphas = trial_lengths(alpha_max, done, 1 if done == 0 else TRIAL_BATCH)
            tried = len(alphas)
            if done == 0:
                alphas = alphas + [0.0]
            B = len(alphas)
            if R.batch is None:
                cap, p = TRIAL_BATCH, system.plan
                R.batch = (R.zeros(cap * n), R.zeros(cap), R.zeros(cap * n), R.zeros(cap * m), R.zeros(cap * p.nnz_J), R.zeros(4 * cap))
            X, fB, gradB, gB, jacB, table = R.batch
            d_alphas = R.up(alphas)
            R.to_kernels()
            ev.trial_points_dev(B, at(R.x), at(R.sol), alphas, at(X))
            ev.cycle_batch_dev(B, at(X), None, [], at(fB), at(gradB), at(gB), at(jacB), None)
            ev.slack_merit_dev(B, at(X), at(gB), at(R.s), at(R.ds), at(d_alphas), at(table))
            R.to_torch()
            f_trial, t = R.down(fB)[:B], R.down(table)[: 4 * B].reshape(B, 4)
            if done == 0:
                merit_0 = f_trial[1] - mu * t[1, 2] + nu * t[1, 0]
            if opt["print_level"] > 2:
                print(f"      merit_0 {merit_0!r} (records: f {q['f']!r} logs {q['tx'][4] + q['ts'][4]!r} theta_1 {theta_1!r}); slope_merit {slope_merit:.3e}")
                for k, alpha in enumerate(alphas):
                    print(f"        alpha {alpha:.3e}: f {f_trial[k]!r} log_sum {t[k, 2]!r} theta_1 {t[k, 0]!r} bad {t[k, 3]} merit - merit_0 "
                          f"{f_trial[k] - mu * t[k, 2] + nu * t[k, 0] - merit_0:.3e} predicted {alpha * slope_merit:.3e}")
            for k, alpha in enumerate(alphas[:tried]):
                if (t[k, 3] == 0.0 and armijo(f_trial[k] - mu * t[k, 2] + nu * t[k, 0], merit_0, alpha, slope_merit)
                        and derivatives_finite(gradB, jacB, k, n, system.plan.nnz_J)):
                    accepted = alpha
                    break
            done += tried
        if opt["print_level"] > 1:
            print(f"      step: delta_w {step[1]:.1e} curvature {curvature:.3e} step_sq {step[2]:.3e} alpha_max {alpha_max:.3e} alpha_d {alpha_d:.3e} slope {slope:.3e} "
                  f"nu {nu:.3e} theta_1 {theta_1:.3e} accepted {accepted} after {done} trial points")
        if accepted is None:
            status = -2
            break
        # ---- the update, then the new point
        R.to_kernels()
        ev.slack_update_dev(at(R.x), at(R.sol), at(R.zl), at(R.dzl), at(R.zu), at(R.dzu), accepted, alpha_d, mu, at(R.rec, 60), kappa=KAPPA_SIGMA)
        ev.slack_update_dev(at(R.s), at(R.ds), at(R.yl), at(R.dyl), at(R.yu), at(R.dyu), accepted, alpha_d, mu, at(R.rec, 60), kappa=KAPPA_SIGMA,
                            d_lam=at(R.lam), d_dlam=at(R.sol, n), which="c")
        R.to_torch()
        iterations += 1
        R.evaluate()
    R.to_torch()
    sens = None if params is None else _sensitivities(R, params, direct, status)
    R.to_torch()
    x = R.down(R.x, n).copy()
    info = make_info(status, x=x, g=R.down(R.g, m).copy(), obj_val=float(R.down(R.f)[0]), mult_g=R.down(R.lam, m).copy(),
                     mult_x_L=R.down(R.zl, n).copy(), mult_x_U=R.down(R.zu, n).copy(), iterations=iterations, mu=mu, error=float(e_0),
                     linear_iterations=linear_iterations, regularisations=reg.count, slack=R.down(R.s, m).copy(),
                     mult_s_L=R.down(R.yl, m).copy(), mult_s_U=R.down(R.yu, m).copy())
    if sens is not None:
        info["sensitivity"] = sens
    if band_refine:
        info["refinement_steps"], info["residual_ratio"] = refinement_steps, residual_ratio
    ev._invalidate_x()
    return postprocess(system, x, bare), info
