"""J v, J^T y and H v on the device (pockit_amd/csrc/pk_ops.cpp through System.linearize and Evaluator.apply_operator_dev)
against scipy.sparse matrices built from the ORACLE's triplets, on identical inputs.  Tolerance: the project's rule,
|a - b| <= 1e-11 * max(1, max|b|) per result vector.  The shapes are the smallest that reach each path of the two kernels:

    brachistochrone(radau, 3, 4)        everything in one or two blocks; empty rows of H
    brachistochrone(radau, 60, 5)       one long row: J^T's t_f column (4 pieces), H's t_f row (3 pieces); J with repeated triplets
    two_stage_rocket(radau, 6, 4)       two phases
    planar_quadrotor(lobatto, 20, 6)    LGL; J with empty rows
    brachistochrone(radau, 200, 8)      a 4 800-entry row (19 pieces); ~300 blocks
    planar_quadrotor(radau, 2000, 6)    ~3 000 blocks: the grid cap and the stride loop; no long row
"""
import importlib

import numpy as np
import pytest
import scipy.sparse

import models

pytestmark = pytest.mark.gpu

TOL = 1e-11
CASES = [("brachistochrone", "radau", 3, 4), ("brachistochrone", "radau", 60, 5), ("two_stage_rocket", "radau", 6, 4),
         ("planar_quadrotor", "lobatto", 20, 6), ("brachistochrone", "radau", 200, 8), ("planar_quadrotor", "radau", 2000, 6)]


def close(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    err = np.max(np.abs(a - b))
    print(f"{what}: err {err:.3e}, bound {TOL * max(1.0, np.max(np.abs(b))):.3e}")
    assert err <= TOL * max(1.0, np.max(np.abs(b))), f"{what}: err {err:.3e}"


class Case:
    """One model: the inputs, the reference matrices from the oracle's triplets and the reference products, computed once."""

    def __init__(self, name, scheme, mesh, num_point):
        build = getattr(models, name)
        self.system, _, guess = build(importlib.import_module(f"pockit_amd.{scheme}"), mesh, num_point)
        ref, _, _ = build(importlib.import_module(f"oracle.{scheme}"), mesh, num_point)
        self.x, self.lam, self.sigma = models.bench_inputs(self.system, guess)
        n, m = len(self.x), len(self.lam)
        self.n, self.m = n, m
        self.J = scipy.sparse.coo_array((ref.jacobian(self.x), ref.jacobianstructure()), shape=(m, n)).tocsr()
        row, col = (np.asarray(a) for a in ref.hessianstructure())
        data = ref.hessian(self.x, self.lam, self.sigma)
        diag = np.nonzero(row == col)[0]      # mirrored as optimizer/scipy.py::_reflection does it
        half = scipy.sparse.coo_array((data, (row, col)), shape=(n, n))
        self.H = (half + half.T - scipy.sparse.coo_array((data[diag], (row[diag], col[diag])), shape=(n, n))).tocsr()
        rng = np.random.default_rng(7)
        self.v, self.y, self.u = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(n)
        self.Jv, self.JTy, self.Hv, self.Hu = self.J @ self.v, self.J.T @ self.y, self.H @ self.v, self.H @ self.u
        self.x_other = self.x * (1.0 + 1.0e-3 * np.random.default_rng(8).uniform(-1.0, 1.0, n))

    def linearize(self):
        return self.system.linearize(self.x, self.lam, self.sigma)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def case(request):
    c = Case(*request.param)
    yield c
    c.system.evaluator.close()


def test_host_vector_products_match_the_oracle(case):
    lin = case.linearize()
    close(lin.jv(case.v), case.Jv, "J v")
    close(lin.jtv(case.y), case.JTy, "J^T y")
    close(lin.hv(case.v), case.Hv, "H v")


def test_device_pointer_products_match_the_oracle_and_the_host_path_bit_for_bit(case):
    import torch

    ev = case.system.evaluator
    lin = case.linearize()
    host = {"J": lin.jv(case.v), "JT": lin.jtv(case.y), "H": lin.hv(case.v)}
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dx, dlam = up(case.x), up(case.lam)
    cj = torch.zeros(ev.csr_map("jac").nnz, dtype=torch.float64, device=dev)
    ch = torch.zeros(ev.csr_map("hess").nnz, dtype=torch.float64, device=dev)
    vec = {"J": (cj, up(case.v), case.m, case.Jv), "JT": (cj, up(case.y), case.n, case.JTy), "H": (ch, up(case.v), case.n, case.Hv)}
    add = {op: np.random.default_rng(9).standard_normal(rows) for op, (_, _, rows, _) in vec.items()}
    torch.cuda.synchronize()             # torch's fills and copies run on its own stream; the context uses its own
    ev.jacobian_csr_dev(dx.data_ptr(), cj.data_ptr())
    ev.hessian_csr_dev(dx.data_ptr(), dlam.data_ptr(), case.sigma, ch.data_ptr())
    with pytest.raises(RuntimeError, match="stale"):      # (those calls gave the context's buffers another evaluation)
        lin.jv(case.v)
    for op, (vals, d_v, rows, ref) in vec.items():
        plain = torch.full((rows,), -3.0, dtype=torch.float64, device=dev)
        again = torch.full((rows,), -4.0, dtype=torch.float64, device=dev)
        summed = torch.full((rows,), -5.0, dtype=torch.float64, device=dev)
        d_add, alias = up(add[op]), up(add[op])
        torch.cuda.synchronize()
        ev.apply_operator_dev(op, vals.data_ptr(), d_v.data_ptr(), plain.data_ptr())
        ev.apply_operator_dev(op, vals.data_ptr(), d_v.data_ptr(), again.data_ptr(), d_add=None)
        ev.apply_operator_dev(op, vals.data_ptr(), d_v.data_ptr(), summed.data_ptr(), d_add=d_add.data_ptr())
        ev.apply_operator_dev(op, vals.data_ptr(), d_v.data_ptr(), alias.data_ptr(), d_add=alias.data_ptr())
        ev.sync()
        plain, again, summed, alias = (t.cpu().numpy() for t in (plain, again, summed, alias))
        close(plain, ref, op)
        close(summed, ref + add[op], op + " + add")
        close(alias, ref + add[op], op + " + add aliasing y")
        assert np.array_equal(summed, alias), op
        assert np.array_equal(plain, again), f"{op}: a second call gave other bits"
        assert np.array_equal(plain, host[op]), f"{op}: device-pointer path and host path differ in bits"


def test_the_same_bits_from_run_to_run_and_after_another_iterate(case):
    lin = case.linearize()
    first = (lin.jv(case.v), lin.jtv(case.y), lin.hv(case.v))
    second = (lin.jv(case.v), lin.jtv(case.y), lin.hv(case.v))
    other = case.system.linearize(case.x_other, case.lam, case.sigma)
    moved = other.jv(case.v)
    assert np.all(np.isfinite(moved)) and not np.array_equal(moved, first[0])
    lin = case.linearize()
    third = (lin.jv(case.v), lin.jtv(case.y), lin.hv(case.v))
    for a, b, c in zip(first, second, third):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_adjoint_identities(case):
    """<y, J v> = <J^T y, v> and <u, H v> = <H u, v>.  Each inner product is bounded by the product of the norms of its
    two factors (Cauchy-Schwarz) and carries a rounding error proportional to it, so the difference is held to 1e-11 of the
    larger of the two products of norms."""
    lin = case.linearize()
    v, y, u = case.v, case.y, case.u
    jv, jty, hv, hu = lin.jv(v), lin.jtv(y), lin.hv(v), lin.hv(u)
    norm = np.linalg.norm
    for what, a, b, scale in (("J", y @ jv, jty @ v, max(norm(y) * norm(jv), norm(jty) * norm(v))),
                              ("H", u @ hv, hu @ v, max(norm(u) * norm(hv), norm(hu) * norm(v)))):
        print(f"{what}: |<a, A b> - <A^T a, b>| = {abs(a - b):.3e}, bound {TOL * scale:.3e}")
        assert abs(a - b) <= TOL * scale, what
    close(hu, case.Hu, "H u")


def test_a_stale_handle_raises_and_so_does_hv_without_multipliers(case):
    system = case.system
    first = case.linearize()
    first.jv(case.v)
    no_h = system.linearize(case.x)                      # the context's one linearization is now this one
    with pytest.raises(RuntimeError, match="stale"):
        first.jv(case.v)
    with pytest.raises(RuntimeError, match="stale"):
        first.hv(case.v)
    close(no_h.jv(case.v), case.Jv, "J v without a Hessian")
    with pytest.raises(RuntimeError, match="no Hessian"):
        no_h.hv(case.v)
    system.evaluator.jacobian_csr(case.x)                # the CSR value arrays now hold another evaluation
    with pytest.raises(RuntimeError, match="stale"):
        no_h.jv(case.v)
    with pytest.raises(ValueError):
        case.linearize().jv(case.y if case.m != case.n else case.v[:-1])


def test_linear_operators_agree_with_the_methods(case):
    lin = case.linearize()
    J, H = lin.jacobian_operator(), lin.hessian_operator()
    assert J.shape == (case.m, case.n) and H.shape == (case.n, case.n)
    assert np.array_equal(J.matvec(case.v), lin.jv(case.v))
    assert np.array_equal(J.rmatvec(case.y), lin.jtv(case.y))
    assert np.array_equal(H.matvec(case.v), lin.hv(case.v))
    assert np.array_equal(J.rmatvec(case.y.reshape(-1, 1)).reshape(-1), lin.jtv(case.y))
