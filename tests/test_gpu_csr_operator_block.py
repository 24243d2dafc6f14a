"""pk_op_rows_k / pk_op_long_k (pockit_amd/csrc/pk_ops.cpp): Y = A V (+ Add) for a block of k vectors on the device.

Synthetic structures, bit for bit against the per-column emulator of tests/sparse_block_cases.py (``sparse_cases.emulate_operator``
on column j: the contract) and within ``sparse_cases``' derived bound of the exact ``fsum`` per (row, column).  The operator
cases of tests/sparse_cases.py in contexts A -- brachistochrone(radau, 3, 4) -- and B -- brachistochrone(radau, 60, 5) -- for all
three ops, uploaded through pk_set_csr_operator: edges, pieces of 256 / 257 / 514, blocks cut by rows, long rows first and
last, equal lengths, no src.  Each at k = 8 with ld = k and at k = 3 with ldv = 5, ldy = 4 and sentinels in the padding of Y
(NaN in the padding of V: a read of it poisons the row); one case per op at k = 9 (two chunks, the second with one column) and
at k = 1; from context C -- brachistochrone(radau, 200, 8) -- the two cases past the grid cap (op 2) at k = 8, which reach the
stride loops.  Every case with Add absent and with Add aliasing Y, and a second call for the same bits.

Models, against the oracle: the first four of tests/test_gpu_csr_operators.py's CASES with k = 5 random columns; ``jmat``, ``jtmat``,
``hmat`` per column to the project's rule |a - b| <= 1e-11 * max(1, max|b|) against the SciPy matrices that file builds from the
oracle's triplets; column j equal to ``jv`` / ``jtv`` / ``hv`` of column j, also for a Fortran-ordered block; the device-pointer
form equal to the host form; the LinearOperators' ``matmat`` / ``rmatmat``; a stale handle, ``hmat`` without multipliers and a
wrong shape.
"""
import functools
import importlib

import numpy as np
import pytest

import models
import sparse_block_cases as sbc
import sparse_cases as sc
from test_gpu_csr_operators import CASES, Case, close

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]

PAD = 8                     # sentinel elements on both sides of a result
SENTINEL = -7.25e77


def _evaluator(ctx):
    name, scheme, mesh, num_point = sc.CONTEXTS[ctx]["model"]
    system = getattr(models, name)(importlib.import_module(f"pockit_amd.{scheme}"), mesh, num_point)[0]
    c, plan = sc.CONTEXTS[ctx], system.plan
    assert (plan.n, plan.m, plan.nnz_J) == (c["n"], c["m"], c["trip_j"])
    ev = system.evaluator
    assert (ev.csr_map("jac").nnz, ev.csr_map("hess").nnz) == (c["nnz_j"], c["nnz_h"])      # the operators take n_unique from the maps
    return ev


@pytest.fixture(scope="module")
def operator_context():
    made = {}

    def get(ctx):
        if ctx not in made:
            made[ctx] = _evaluator(ctx)
        return made[ctx]

    yield get
    for ev in made.values():
        ev.close()


def _i32(a):
    from pockit_amd import runtime

    return None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(runtime.c_int32_p)


@functools.lru_cache(maxsize=None)
def _expectation(case_id, k):
    case = next(c for c in sc.operator_cases() if c.id == case_id)
    V, Add = sbc.block_inputs(case, k, seed=500 + k)
    return sbc.BlockExpectation(case, V, Add)


def _padded(block, ld, pad):
    out = np.full((block.shape[0], ld), pad)
    out[:, : block.shape[1]] = block
    return out


class Result:
    """rows x k doubles with leading dimension ld in the middle of a larger device tensor: NaN (or ``fill``) where the kernel
    writes, sentinels in the padding columns and on both sides."""

    def __init__(self, torch, dev, rows, k, ld, fill=None):
        inner = _padded(np.full((rows, k), np.nan) if fill is None else fill, ld, SENTINEL)
        host = np.concatenate((np.full(PAD, SENTINEL), inner.reshape(-1), np.full(PAD, SENTINEL)))
        self.rows, self.k, self.ld, self.buf = rows, k, ld, torch.from_numpy(host).to(dev)
        self.ptr = self.buf.data_ptr() + 8 * PAD

    def fetch(self, what):
        host = self.buf.cpu().numpy()
        edge = np.full(PAD, SENTINEL)
        inner = host[PAD: PAD + self.rows * self.ld].reshape(self.rows, self.ld)
        assert sc.same_bits(host[:PAD], edge) and sc.same_bits(host[PAD + self.rows * self.ld:], edge), f"{what}: a sentinel beside Y was overwritten"
        assert sc.same_bits(inner[:, self.k:], np.full((self.rows, self.ld - self.k), SENTINEL)), f"{what}: the padding of Y was written"
        return inner[:, : self.k].copy()


AB = [c for c in sc.operator_cases() if c.ctx in "AB"]
LAYOUTS = {"k8": (8, 8, 8), "k3-padded": (3, 5, 4), "k9": (9, 9, 9), "k1": (1, 1, 1)}
RUNS = [(c, "k8") for c in AB] + [(c, "k3-padded") for c in AB]
RUNS += [(next(c for c in AB if c.id == cid), lay) for lay in ("k9", "k1")
         for cid in ("B-equal-lengths-op0", "B-long-first-and-last-op1", "A-edges-op2")]
RUNS += [(c, "k8") for c in sc.operator_cases() if c.ctx == "C" and c.name in ("blocks-past-the-cap", "longs-past-the-cap")]
assert len(RUNS) == 2 * len(AB) + 6 + 2 and {c.op for c, lay in RUNS if lay == "k9"} == {0, 1, 2}


@pytest.mark.parametrize("case, layout", RUNS, ids=lambda v: v if isinstance(v, str) else v.id)
def test_block_kernels_match_the_single_vector_association_per_column(case, layout, operator_context):
    import torch

    k, ldv, ldy = LAYOUTS[layout]
    want = _expectation(case.id, k)
    ev = operator_context(case.ctx)
    lib, h = ev.ctx.lib, ev.ctx.handle
    ev.ctx.check(lib.pk_set_csr_operator(h, case.op, _i32(case.indptr), _i32(case.indices), _i32(case.src), case.n_rows,
                                         case.n_cols, case.nnz))
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    vals, V = up(case.vals), up(_padded(want.V, ldv, np.nan))
    plain, again = (Result(torch, dev, case.n_rows, k, ldy) for _ in range(2))
    alias = Result(torch, dev, case.n_rows, k, ldy, fill=want.Add)
    torch.cuda.synchronize()            # torch's copies run on its own stream; the context uses its own
    for out, d_add in ((plain, None), (again, None), (alias, alias.ptr)):
        ev.ctx.check(lib.pk_apply_operator_block_dev(h, case.op, vals.data_ptr(), k, V.data_ptr(), ldv, d_add, out.ptr, ldy, None))
    ev.sync()
    what = f"{case.id} {layout}"
    plain, again, alias = (r.fetch(f"{what} {n}") for r, n in ((plain, "plain"), (again, "again"), (alias, "alias")))
    for got, with_add in ((plain, False), (alias, True)):
        worst = max(sc.worst_units(got[:, j], want.ref[with_add][:, j], want.scale[with_add][:, j]) for j in range(k))
        print(f"{what} add={'aliasing Y' if with_add else 'NULL'}: worst {worst:.3e} u*sum|t|, bound {float(sc.gamma(int(case.lengths.max()) + 1) / sc.U):.1f}")
        assert want.problems(got, with_add) == []
    assert sc.same_bits(plain, again), f"{what}: a second call gave other bits"
    empty = case.lengths == 0
    assert sc.same_bits(plain[empty], np.zeros((int(empty.sum()), k))) and sc.same_bits(alias[empty], want.Add[empty])


# ---------------------------------------------------------------- models, against the oracle
K_MODEL = 5


@pytest.fixture(scope="module", params=CASES[:4], ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def case(request):
    c = Case(*request.param)
    rng = np.random.default_rng(11)
    c.V, c.Y = rng.standard_normal((c.n, K_MODEL)), rng.standard_normal((c.m, K_MODEL))
    yield c
    c.system.evaluator.close()


def _columns_close(got, matrix, block, what):
    assert got.shape == (matrix.shape[0], block.shape[1]) and got.flags.c_contiguous
    for j in range(block.shape[1]):
        close(got[:, j], matrix @ block[:, j], f"{what} column {j}")


def test_host_block_products_match_the_oracle_and_the_single_products_bit_for_bit(case):
    lin = case.linearize()
    JV, JTY, HV = lin.jmat(case.V), lin.jtmat(case.Y), lin.hmat(case.V)
    _columns_close(JV, case.J, case.V, "J V")
    _columns_close(JTY, case.J.T, case.Y, "J^T Y")
    _columns_close(HV, case.H, case.V, "H V")
    for j in range(K_MODEL):
        assert np.array_equal(JV[:, j], lin.jv(case.V[:, j])), f"J V column {j}"
        assert np.array_equal(JTY[:, j], lin.jtv(case.Y[:, j])), f"J^T Y column {j}"
        assert np.array_equal(HV[:, j], lin.hv(case.V[:, j])), f"H V column {j}"
    VF, YF = np.asfortranarray(case.V), np.asfortranarray(case.Y)
    assert VF.flags.f_contiguous and not VF.flags.c_contiguous
    assert np.array_equal(lin.jmat(VF), JV) and np.array_equal(lin.jtmat(YF), JTY) and np.array_equal(lin.hmat(VF), HV)
    assert np.array_equal(lin.jmat(case.V), JV), "a second call gave other bits"
    assert np.array_equal(lin.jmat(case.V[:, :1]), JV[:, :1]) and np.array_equal(lin.hmat(case.V[:, 1:4]), HV[:, 1:4])


def test_device_pointer_block_products_equal_the_host_form_bit_for_bit(case):
    import torch

    ev = case.system.evaluator
    lin = case.linearize()
    host = {"J": lin.jmat(case.V), "JT": lin.jtmat(case.Y), "H": lin.hmat(case.V)}
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dx, dlam = up(case.x), up(case.lam)
    cj = torch.zeros(ev.csr_map("jac").nnz, dtype=torch.float64, device=dev)
    ch = torch.zeros(ev.csr_map("hess").nnz, dtype=torch.float64, device=dev)
    block = {"J": (cj, case.V, case.m), "JT": (cj, case.Y, case.n), "H": (ch, case.V, case.n)}
    torch.cuda.synchronize()             # torch's fills and copies run on its own stream; the context uses its own
    ev.jacobian_csr_dev(dx.data_ptr(), cj.data_ptr())
    ev.hessian_csr_dev(dx.data_ptr(), dlam.data_ptr(), case.sigma, ch.data_ptr())
    with pytest.raises(RuntimeError, match="stale"):      # (those calls gave the context's buffers another evaluation)
        lin.jmat(case.V)
    for op, (vals, B, rows) in block.items():
        add = np.random.default_rng(9).standard_normal((rows, K_MODEL))
        d_B, d_add = up(B), up(add)
        plain = torch.full((rows, K_MODEL), -3.0, dtype=torch.float64, device=dev)
        wide = torch.full((rows, K_MODEL + 2), -4.0, dtype=torch.float64, device=dev)
        summed = torch.full((rows, K_MODEL), -5.0, dtype=torch.float64, device=dev)
        alias = up(add)
        torch.cuda.synchronize()
        ev.apply_operator_block_dev(op, vals.data_ptr(), K_MODEL, d_B.data_ptr(), plain.data_ptr())
        ev.apply_operator_block_dev(op, vals.data_ptr(), K_MODEL - 1, d_B.data_ptr() + 8, wide.data_ptr() + 8, ldv=K_MODEL, ldy=K_MODEL + 2)
        ev.apply_operator_block_dev(op, vals.data_ptr(), K_MODEL, d_B.data_ptr(), summed.data_ptr(), d_add=d_add.data_ptr())
        ev.apply_operator_block_dev(op, vals.data_ptr(), K_MODEL, d_B.data_ptr(), alias.data_ptr(), d_add=alias.data_ptr())
        ev.sync()
        plain, wide, summed, alias = (t.cpu().numpy() for t in (plain, wide, summed, alias))
        assert np.array_equal(plain, host[op]), f"{op}: device-pointer form and host form differ in bits"
        # columns 1 .. 4 of the block addressed in place through the leading dimensions, into columns 1 .. 4 of a wider Y
        assert np.array_equal(wide[:, 1:K_MODEL], host[op][:, 1:]) and np.all(wide[:, 0] == -4.0) and np.all(wide[:, K_MODEL:] == -4.0), op
        assert np.array_equal(summed, alias), op
        for j in range(K_MODEL):
            close(summed[:, j], host[op][:, j] + add[:, j], f"{op} + Add column {j}")


def test_linear_operators_hand_blocks_to_the_block_product(case):
    lin = case.linearize()
    J, H = lin.jacobian_operator(), lin.hessian_operator()
    JV, JTY, HV = lin.jmat(case.V), lin.jtmat(case.Y), lin.hmat(case.V)
    assert np.array_equal(J.matmat(case.V), JV) and np.array_equal(J.rmatmat(case.Y), JTY)
    assert np.array_equal(H.matmat(case.V), HV) and np.array_equal(H.rmatmat(case.V), HV)
    assert np.array_equal(J @ case.V, JV) and np.array_equal(J.T @ case.Y, JTY)
    assert np.array_equal(J.matvec(case.V[:, 0]), JV[:, 0])      # (matvec is the single product, as before)


def test_a_stale_handle_hmat_without_multipliers_and_a_wrong_shape_raise(case):
    system = case.system
    first = case.linearize()
    first.jmat(case.V)
    no_h = system.linearize(case.x)                      # the context's one linearization is now this one
    for stale in (first.jmat, first.hmat):
        with pytest.raises(RuntimeError, match="stale"):
            stale(case.V)
    with pytest.raises(RuntimeError, match="stale"):
        first.jtmat(case.Y)
    _columns_close(no_h.jmat(case.V), case.J, case.V, "J V without a Hessian")
    with pytest.raises(RuntimeError, match="no Hessian"):
        no_h.hmat(case.V)
    lin = case.linearize()
    wrong_rows = case.Y if case.m != case.n else case.V[:-1]
    for bad in (wrong_rows, case.V[:, 0], case.V[:, :0], case.V.T, case.V[None]):
        with pytest.raises(ValueError):
            lin.jmat(bad)
    with pytest.raises(ValueError):
        lin.jtmat(case.V if case.m != case.n else case.Y[:-1])
    with pytest.raises(ValueError):
        lin.hmat(case.V[1:])
