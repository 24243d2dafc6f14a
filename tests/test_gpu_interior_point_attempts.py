"""``interior_point.solve(..., linear_solver="banded", band_attempts=k)`` on the device: the next k values of ``delta_w`` are
factored and solved together (one batch of the band LU) and then walked in the schedule's order.  Every entry of a batch has
the bits of the single factorisation, so a solve must not depend on k: brachistochrone(radau, 10, 8), the path-constrained LQR
(Radau 5 x 4) and lqr(lobatto, 6, 6), each with ``band_attempts`` = 1, 3 and 8 -- ``x``, ``mult_g``, ``obj_val``, ``iterations`` and
``regularisations`` bit-equal across the three runs, status 0, and converged by the checks of
tests/test_gpu_interior_point_banded.py (imported, not copied).  A spy on ``_Resident.down`` sees no array of the step's system
and no transfer above ``max(n, m, 64)`` doubles.  No iteration count is asserted."""
import numpy as np
import pytest

import models
import sparse_cases as sc
from test_gpu_interior_point import TOL, _converged, _ns, constrained_lqr, dictated
from test_gpu_interior_point_banded import _no_matrix_came_down, downloads  # noqa: F401  (downloads: a fixture)

pytestmark = pytest.mark.gpu
ATTEMPTS = (1, 3, 8)


def _brachistochrone(package):
    system, _, guess = models.brachistochrone(_ns("radau", package), 10, 8)
    return system, guess


def _constrained(package):
    system, _, guess = constrained_lqr(_ns("radau", package), 5, 4)
    return system, guess


def _lqr(package):
    ns = _ns("lobatto", package)
    system, (phase,), _ = models.lqr(ns, 6, 6)
    return system, [ns.constant_guess(phase, 0.0), [0.0]]


@pytest.mark.parametrize("build", [_brachistochrone, _constrained, _lqr], ids=["brachistochrone-radau-10x8", "constrained-lqr-radau-5x4", "lqr-lobatto-6x6"])
def test_the_solve_does_not_depend_on_band_attempts(build, downloads):
    from pockit_amd.optimizer import interior_point

    runs = []
    for k in ATTEMPTS:
        system, guess = build("pockit_amd")
        del downloads[:]
        try:
            _, info = interior_point.solve(system, guess, {"tol": TOL, "max_iter": 200}, linear_solver="banded", band_attempts=k)
        finally:
            system.evaluator.close()
        assert info["status"] == 0, (k, info["status_msg"])
        _converged(build("oracle")[0], info, dictated=dictated(system))
        _no_matrix_came_down(system, downloads, info["iterations"])
        runs.append(info)
    first = runs[0]
    print(f"{first['iterations']} iterations, {first['regularisations']} regularisations, f = {first['obj_val']!r}")
    for k, info in zip(ATTEMPTS[1:], runs[1:]):
        assert (info["iterations"], info["regularisations"]) == (first["iterations"], first["regularisations"]), k
        assert np.float64(info["obj_val"]).tobytes() == np.float64(first["obj_val"]).tobytes(), (k, info["obj_val"], first["obj_val"])
        for key in ("x", "mult_g"):
            assert sc.same_bits(np.asarray(info[key], dtype=np.float64), np.asarray(first[key], dtype=np.float64)), (k, key)
