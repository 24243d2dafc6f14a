"""pockit_amd.optimizer.interior_point.solve with ``linear_solver="banded"`` on the device, end to end: the solving cases of
tests/test_gpu_interior_point.py with that file's own bounds and helpers (imported, not copied).

* lqr(lobatto, 6, 6): the Riccati value within ``2e-6 max(1, |opt|)``; ``x(1) = x_f`` to 1e-9.
* brachistochrone(radau, 10, 8) and (lobatto, 6, 6): the cycloid's descent time within 1e-7 for the objective and for ``t_f``,
  the end point (2, 2) to 1e-12.  The free final time is the border of the band LU.
* the path-constrained LQR, Lobatto 6 x 6 and Radau 5 x 4: the objective within 1e-6 of SLSQP on the oracle, an inequality row
  active with a non-zero multiplier.
* every converged case: ``E_0 <= 1e-8`` recomputed from ``info`` on the oracle (``_converged``).
* ``max_iter = 3`` on the brachistochrone: status -1, a finite x.
* every case: a spy on ``_Resident.down`` saw no transfer of an ``nnz``-sized array (the CSR values of J and H, the triplets)
  and none of n + m values (the right-hand side, the step): the step's system never crosses PCIe on this path.

No iteration count is asserted."""
import numpy as np
import pytest

import models
from test_gpu_interior_point import TOL, _converged, _ns, _slsqp, constrained_lqr, dictated, riccati  # noqa: F401  (riccati: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture
def downloads(monkeypatch):
    """The sizes of every tensor ``_Resident.down`` brought to the host."""
    from pockit_amd.optimizer import interior_point

    seen = []
    original = interior_point._Resident.down

    def spy(self, t, count=None):
        names = [k for k in MATRIX_SIDE if getattr(self, k, None) is not None and getattr(self, k).data_ptr() == t.data_ptr()]
        seen.append((names[0] if names else None, int(t.numel()) if count is None else int(count)))
        return original(self, t, count)

    monkeypatch.setattr(interior_point._Resident, "down", spy)
    return seen


# the resident arrays of the step's system: the triplet and CSR values of J and H, Sigma_x, S2, the right-hand side, the step
MATRIX_SIDE = ("jt", "ht", "cj", "ch", "sig_x", "s2", "rhs", "sol")


def _solve(system, guess, options=None):
    from pockit_amd.optimizer import interior_point

    try:
        return interior_point.solve(system, guess, options or {"tol": TOL, "max_iter": 200}, linear_solver="banded")
    finally:
        system.evaluator.close()


def _no_matrix_came_down(system, seen, iterations):
    """Nothing of the step's system came down: no value array of J or H (triplets or CSR), no Sigma_x, S2, right-hand side or
    step, and no vector of n + m values at all.  What the host sees are the records, f, g once at the start and the result."""
    p = system.plan
    assert seen, "the spy saw nothing"
    named = sorted({name for name, _ in seen if name is not None})
    assert not named, f"arrays of the step's system were downloaded: {named}"
    sizes = [size for _, size in seen]
    assert p.n + p.m not in sizes, "a vector of n + m values came down"
    assert max(sizes) <= max(p.n, p.m, 64), f"a transfer of {max(sizes)} doubles (n {p.n}, m {p.m}, nnz_J {p.nnz_J}, nnz_H {p.nnz_H})"
    print(f"{len(seen)} downloads in {iterations} iterations ({len(seen) / max(1, iterations):.1f} per iteration), the largest of {max(sizes)} doubles")


def test_lqr_reaches_the_riccati_value(riccati, downloads):
    ns = _ns("lobatto", "pockit_amd")
    system, (phase,), _ = models.lqr(ns, 6, 6)
    (var, s), info = _solve(system, [ns.constant_guess(phase, 0.0), [0.0]])
    _converged(models.lqr(_ns("lobatto", "oracle"), 6, 6)[0], info, dictated=dictated(system))
    assert abs(info["obj_val"] - riccati) <= 2e-6 * max(1.0, abs(riccati)), (info["obj_val"], riccati)
    assert abs(var.x[0][-1] - s[0]) < 1e-9 and abs(var.x[0][0] - 1.0) < 1e-12
    assert info["linear_iterations"] == 0
    _no_matrix_came_down(system, downloads, info["iterations"])


@pytest.mark.parametrize("scheme,mesh,num_point", [("radau", 10, 8), ("lobatto", 6, 6)])
def test_the_brachistochrone_reaches_the_cycloid_time(scheme, mesh, num_point, downloads):
    from scipy.optimize import brentq

    system, _, guess = models.brachistochrone(_ns(scheme, "pockit_amd"), mesh, num_point)
    (var,), info = _solve(system, guess)
    theta = brentq(lambda t: (t - np.sin(t)) / (1 - np.cos(t)) - 1.0, 0.1, 2 * np.pi - 0.1)      # x_f / y_f = 1
    optimum = theta * np.sqrt(2.0 / (1 - np.cos(theta)) / 9.81)
    _converged(models.brachistochrone(_ns(scheme, "oracle"), mesh, num_point)[0], info, dictated=dictated(system))
    assert abs(info["obj_val"] - optimum) <= 1e-7, (info["obj_val"], optimum)
    assert abs(var.t_f - optimum) <= 1e-7
    assert abs(var.x[0][-1] - 2.0) < 1e-12 and abs(var.x[1][-1] - 2.0) < 1e-12
    _no_matrix_came_down(system, downloads, info["iterations"])


@pytest.mark.parametrize("scheme,mesh,num_point,rows", [("lobatto", 6, 6, 31), ("radau", 5, 4, 20)])
def test_lqr_with_an_active_path_inequality_matches_slsqp_on_the_oracle(scheme, mesh, num_point, rows, downloads):
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
    _no_matrix_came_down(system, downloads, info["iterations"])


def test_max_iter_ends_with_status_minus_one_and_a_finite_x(downloads):
    system, _, guess = models.brachistochrone(_ns("radau", "pockit_amd"), 10, 8)
    (var,), info = _solve(system, guess, {"max_iter": 3})
    assert info["status"] == -1 and info["iterations"] == 3 and np.all(np.isfinite(info["x"])) and np.all(np.isfinite(var.data))
    assert "maximum" in info["status_msg"]
    _no_matrix_came_down(system, downloads, info["iterations"])
