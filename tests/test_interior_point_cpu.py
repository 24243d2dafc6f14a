"""The scalar logic of pockit_amd/optimizer/interior_point.py, which needs no device: option validation, the start's push inside
the bounds, the error and its scaling, the barrier update, the penalty rule, the Armijo test and its trial lengths, the
regularisation schedule, the keys of ``info``, the direct step's assembled matrix against SciPy's own block assembly -- on
recorded records and small synthetic systems.  Without a GPU ``solve`` fails loudly.  CPU only."""
import numpy as np
import pytest

from pockit_amd import runtime
from pockit_amd.optimizer import interior_point as ipm


def test_options_have_defaults_and_unknown_names_are_refused():
    assert ipm.options(None) == {"tol": 1e-8, "max_iter": 200, "mu_init": 0.1, "print_level": 0}
    got = ipm.options({"tol": 1e-6, "max_iter": 3})
    assert (got["tol"], got["max_iter"], got["mu_init"]) == (1e-6, 3, 0.1)
    for bad in ({"maxiter": 3}, {"tol": 0.0}, {"tol": float("nan")}, {"mu_init": -1.0}, {"max_iter": -1}):
        with pytest.raises(ValueError):
            ipm.options(bad)
    with pytest.raises(ValueError, match="linear_solver"):
        ipm.solve(None, None, linear_solver="cholesky")
    with pytest.raises(ValueError, match="unknown option"):
        ipm.solve(None, None, {"hessian_approximation": "exact"})


def test_the_start_is_pushed_inside_by_the_two_kappas():
    inf = np.inf
    lb = np.array([0.0, -inf, 0.0, 2.0, -inf, 100.0, 0.0])
    ub = np.array([1.0, 5.0, inf, 2.0, inf, 300.0, 1e-3])
    v = np.array([0.0, 9.0, -3.0, 7.0, 4.0, 250.0, 5e-4])
    got = ipm.push_inside(v, lb, ub)
    # two-sided: min(1e-2 max(1, |lb|), 1e-2 (ub - lb)); one-sided: 1e-2 max(1, |bound|); fixed: the bound; free: untouched
    assert np.array_equal(got, [0.01, 5.0 - 0.05, 0.01, 2.0, 4.0, 250.0, 5e-4])
    assert ipm.push_inside([100.0], [100.0], [300.0])[0] == 101.0 and ipm.push_inside([1.0], [0.0], [1e-3])[0] == 1e-3 - 1e-5


def test_the_error_its_scale_and_the_barrier_update():
    assert ipm.dual_scale(10.0, 20.0, 5, 5) == 1.0                      # (a mean multiplier below 100 does not scale)
    assert ipm.dual_scale(1e4, 1e4, 10, 10) == 10.0
    assert ipm.dual_scale(0.0, 0.0, 0, 0) == 1.0
    assert ipm.barrier_error(2e-3, 4e-3, 1e-3, 8e-3, 2.0) == 4e-3
    assert ipm.barrier_error(2e-3, 1e-3, 5e-3, 8e-3, 2.0) == 5e-3       # (the infeasibility is not scaled)
    # recorded: mu = 0.1 falls to 0.2 mu first, then by mu^1.5 (superlinearly), and stops at tol / 10
    mus, mu = [], 0.1
    while ipm.barrier_falls(0.0, mu, 1e-8):
        mu = ipm.next_mu(mu, 1e-8)
        mus.append(mu)
    assert mus[0] == 0.2 * 0.1 < 0.1 ** 1.5 and mus[-1] == 1e-9 and all(a > b for a, b in zip(mus, mus[1:])) and len(mus) == 6
    assert mus[1] == mus[0] ** 1.5 < 0.2 * mus[0] and abs(mus[4] - 2.5059035596800618e-09) < 1e-20 and not ipm.barrier_falls(1.01, 0.1, 1e-8) and ipm.barrier_falls(1.0, 0.1, 1e-8)
    assert not ipm.barrier_falls(0.0, 1e-9, 1e-8)
    assert ipm.fraction_to_boundary(0.1) == 0.99 and ipm.fraction_to_boundary(1e-4) == 1.0 - 1e-4


def test_the_penalty_rule():
    assert ipm.penalty(0.5, -3.0, 2.0, 0.0) == 1.0                       # feasible: max(1, |lam + dlam|)
    assert ipm.penalty(7.0, -3.0, 2.0, 0.0) == 7.0
    assert ipm.penalty(0.5, 4.0, 2.0, 0.5) == (4.0 + 1.0) / 0.45         # the quotient with half the curvature
    assert ipm.penalty(0.5, 4.0, -2.0, 0.5) == 4.0 / 0.45                # negative curvature does not lower it
    assert ipm.penalty(0.5, -4.0, 2.0, 0.5) == 1.0                       # a descent direction of phi needs no more than 1
    nu = ipm.penalty(0.0, 4.0, 2.0, 0.5)
    assert 4.0 - nu * 0.5 <= -0.5 * 2.0 + 0.1 * nu * 0.5 + 1e-12         # the merit's slope is then negative enough


def test_armijo_and_the_trial_lengths():
    assert ipm.armijo(1.0 - 1e-6, 1.0, 0.5, -1.0) and not ipm.armijo(1.0 + 1e-6, 1.0, 0.5, -1.0)
    assert not ipm.armijo(1.0 - 1e-10, 1.0, 1.0, -1.0) and ipm.armijo(1.0 - 1e-8, 1.0, 1.0, -1.0)
    assert not ipm.armijo(float("nan"), 1.0, 1.0, -1.0) and not ipm.armijo(float("inf"), 1.0, 1.0, -1.0)
    first = ipm.trial_lengths(0.8, 0, 1)
    assert first == [0.8] and ipm.trial_lengths(0.8, 1) == [0.8 * 0.5 ** k for k in range(1, 9)]
    total, done = [], 0
    while True:
        part = ipm.trial_lengths(1.0, done, 1 if done == 0 else ipm.TRIAL_BATCH)
        if not part:
            break
        total += part
        done += len(part)
    assert len(total) == 25 and total[-1] == 0.5 ** 24


def test_the_regularisation_schedule():
    reg = ipm.Regularisation()
    assert list(reg.attempts()) == [0.0] + [1e-4 * 100.0 ** k for k in range(12)] and reg.count == 12
    reg = ipm.Regularisation()
    for delta in reg.attempts():
        if delta >= 1.0:
            reg.accept(delta)
            break
    assert reg.last == 1.0 and reg.count == 3
    seq = list(reg.attempts())
    assert seq[:4] == [0.0, 1.0 / 3.0, 8.0 / 3.0, 64.0 / 3.0] and len(seq) == 13
    reg.last = 1e-4
    assert list(reg.attempts())[1] == 1e-4                               # max(1e-4, last / 3)
    gen = reg.attempts()
    assert next(gen) == 0.0
    reg.accept(0.0)
    assert reg.last == 1e-4                                              # an unregularised success keeps the last value


def test_info_has_cyipopts_keys_and_this_solvers():
    fields = dict(x=np.zeros(2), g=np.zeros(1), obj_val=1.0, mult_g=np.zeros(1), mult_x_L=np.zeros(2), mult_x_U=np.zeros(2), iterations=3, mu=1e-9,
                  error=1e-10, linear_iterations=0, regularisations=0, slack=np.zeros(1), mult_s_L=np.zeros(1), mult_s_U=np.zeros(1))
    info = ipm.make_info(0, **fields)
    assert {"x", "g", "obj_val", "mult_g", "mult_x_L", "mult_x_U", "status", "status_msg", "iterations", "mu", "error", "linear_iterations",
            "regularisations"} <= set(info)
    assert info["status"] == 0 and info["status_msg"] == "converged"
    assert [ipm.make_info(s, **fields)["status"] for s in (-1, -2, -13)] == [-1, -2, -13] and set(ipm.STATUS) == {0, -1, -2, -13}
    with pytest.raises(KeyError):
        ipm.make_info(0, x=np.zeros(2))


def test_the_errors_from_recorded_records():
    tx = np.array([3e-9, 1.0, 10.0, 0.1, -4.0, 0.0, 20.0, 1e-9])
    ts = np.array([5e-9, 1.0, 4.0, 0.2, -1.0, 0.0, 8.0, 1e-9])
    q = dict(tx=tx, ts=ts, tx0=tx * 0.5, ts0=ts * 0.5, rd=np.array([2e-9, 0.0, 0.0, 0.0]), red=np.array([1e-9, 4e-9, 0.0, 4.0]), r_s_inf=1e-9,
             lam_1=12.0, f=0.25)
    e_0, e_mu, broken = ipm._errors(q, 6)
    assert (e_0, e_mu, broken) == (2.5e-9, 5e-9, False)
    q["red"] = np.array([1e-9, 4e-9, 1.0, 4.0])
    assert ipm._errors(q, 6)[2]
    q["red"], q["f"] = np.array([1e-9, 4e-9, 0.0, 4.0]), float("nan")
    assert ipm._errors(q, 6)[2]


def test_the_direct_steps_matrix_is_the_block_matrix():
    """DirectKkt's once-assembled structure against scipy.sparse.bmat on a random lower-triangular H, a random J and a fixed
    variable: the same solution as a dense solve, 0.0 for the fixed variable."""
    import scipy.sparse as sp

    from pockit_amd.csr import CsrMap

    rng = np.random.default_rng(5)
    n, m = 9, 5
    hr, hc = np.tril_indices(n)
    pick = rng.uniform(size=len(hr)) < 0.5
    pick |= hr == hc
    map_h = CsrMap(hr[pick], hc[pick], (n, n))
    jr, jc = np.nonzero(rng.uniform(size=(m, n)) < 0.6)
    map_j = CsrMap(jr, jc, (m, n))
    hvals, jvals = rng.standard_normal(map_h.nnz), rng.standard_normal(map_j.nnz)
    free = np.ones(n, dtype=bool)
    free[4] = False
    s1, s2, rhs = rng.uniform(5.0, 6.0, n), np.where(np.arange(m) % 2, 0.0, rng.uniform(0.5, 1.0, m)), rng.standard_normal(n + m)
    dx, dlam = ipm.DirectKkt(map_j, map_h, free).solve(hvals, jvals, s1, s2, rhs)
    L = map_h.to_scipy(hvals).toarray()
    H = L + L.T - np.diag(np.diag(L)) + np.diag(s1)
    J = map_j.to_scipy(jvals).toarray()
    K = sp.bmat([[sp.csr_array(H[free][:, free]), sp.csr_array(J[:, free].T)], [sp.csr_array(J[:, free]), sp.diags(-s2)]]).toarray()
    want = np.linalg.solve(K, np.concatenate((rhs[:n][free], rhs[n:])))
    assert dx[4] == 0.0 and np.allclose(dx[free], want[: n - 1], rtol=1e-10, atol=1e-12) and np.allclose(dlam, want[n - 1:], rtol=1e-10, atol=1e-12)


def test_without_a_gpu_solve_fails_loudly():
    if runtime.load_library().pk_device_count() > 0:
        pytest.skip("a GPU is present")
    import models
    import pockit_amd.lobatto as lobatto

    system, (phase,), _ = models.lqr(lobatto, 2, 3)
    with pytest.raises(RuntimeError):
        ipm.solve(system, [lobatto.constant_guess(phase, 0.0), [0.0]])


def test_a_trial_point_with_a_non_finite_derivative_is_told_apart():
    """``derivatives_finite`` looks at entry k of the line search's dense batches and at nothing else."""
    import torch

    n, nnz = 5, 7
    grad = torch.arange(3 * n, dtype=torch.float64)
    jac = torch.arange(3 * nnz, dtype=torch.float64)
    assert all(ipm.derivatives_finite(grad, jac, k, n, nnz) for k in range(3))
    for bad in (float("inf"), float("-inf"), float("nan")):
        for at in (n, 2 * n - 1):
            g = grad.clone()
            g[at] = bad
            assert [ipm.derivatives_finite(g, jac, k, n, nnz) for k in range(3)] == [True, False, True]
        for at in (nnz, 2 * nnz - 1):
            j = jac.clone()
            j[at] = bad
            assert [ipm.derivatives_finite(grad, j, k, n, nnz) for k in range(3)] == [True, False, True]
    assert ipm.derivatives_finite(grad, jac[:0], 0, n, 0)
