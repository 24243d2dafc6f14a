"""pk_op_rows, pk_op_long (pockit_amd/csrc/pk_ops.cpp) and pk_csr (kernel_csr) on the device against the exact per-row
references of tests/sparse_cases.py: synthetic structures and maps at the shapes where these kernels can go wrong, uploaded
through the C ABI (pk_set_csr_operator / pk_apply_operator_dev, pk_set_csr_map / pk_gather_csr_dev) into the context of a small
model.  The inputs, the ``fsum`` reference, the derived per-row bound and the emulators are described, and tested, there
(tests/test_sparse_cases_cpu.py).

Operator cases (each for the ops whose row count fits; op 0 has m rows, ops 1 and 2 have n):

    A  brachistochrone(radau, 3, 4)     rows of 0, 1, 255, 256, 257, 512, 513, 0, 3, 1 entries; rows of 65 536, 65 537 and 131 329
                                        entries (256, 257 and 514 pieces, the last piece of the last row with one entry: the
                                        second and third trip of op_long_strided); src = NULL
    B  brachistochrone(radau, 60, 5)    600 one-entry rows (blocks cut by the 256-row limit: 256, 256, 88); a 300-entry first row,
                                        700 empty rows, a 257-entry last row; equal row lengths 2, 4, 8, 16, 32, 31, 33, 128 that
                                        fill whole blocks (what op_slot's padding exists for); src = NULL
    C  brachistochrone(radau, 200, 8)   op 2: 2 100 rows of 200 entries, one per block, long rows interleaved (more blocks than
                                        the grid cap of 2 048); 2 100 rows of 257 entries (pk_op_long's stride loop); src = NULL

Every operator case: ``add`` NULL, given, and aliasing ``y``; ``y`` in the middle of a larger tensor prefilled with NaN between
sentinels (all rows written, the sentinels untouched); the per-row bound against ``fsum``; bit equality with the emulator; bit
equality of a second call.

Gather cases (contexts A and B, which = 0): n_unique mod 256 in {0, 1, 255}; ragged slices whose widest run takes every value
in {1, 2, 3, 4, 5, 7, 8, 9} (the four-way unrolled loop and its remainder at every width); one run of 3 000 among runs of 1; a
slice of runs of 1 inside a map that has ``seg``; ``seg`` = NULL.  The same checks.

pk_csr past its grid cap (4 096 workgroups: a stride loop's second trip needs more than 1 048 576 CSR entries), in the context
of planar_quadrotor(radau, 2776, 6) -- the smallest uniform mesh of that model with more than 1 048 576 + 512 Jacobian triplets:
a map with ``seg`` of 1 048 577 + 255 entries (4 097 slices; slice 4 096 holds a run of 2 and, in its last entry, a run of 5;
slice 0 a wide run: workgroup 0 takes both), and ``seg`` = NULL with 1 049 253 entries (the elementwise loop).  The same checks.
tests/test_gpu_parity.py::test_device_csr_gathers_past_the_grid_cap gathers the model's real Jacobian at that size.

The operator group and the gather group have an evaluator each per context: a synthetic pk_set_csr_map drops the operators, and
after it the evaluator's cached CSR methods would describe a map the context no longer has -- they are not called here.
"""
import importlib

import numpy as np
import pytest

import models
import sparse_cases as sc

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]

PAD = 8                     # sentinel elements on both sides of a result
SENTINEL = -7.25e77


def _evaluator(ctx):
    c = sc.CAP_CONTEXT if ctx == "D" else sc.CONTEXTS[ctx]
    name, scheme, mesh, num_point = c["model"]
    system = getattr(models, name)(importlib.import_module(f"pockit_amd.{scheme}"), mesh, num_point)[0]
    plan = system.plan
    assert (plan.n, plan.m, plan.nnz_J) == (c["n"], c["m"], c["trip_j"])
    return system.evaluator


def _contexts(prepare):
    made = {}

    def get(ctx):
        if ctx not in made:
            made[ctx] = _evaluator(ctx)
            prepare(ctx, made[ctx])
        return made[ctx]

    return made, get


@pytest.fixture(scope="module")
def operator_context():
    def real_maps(ctx, ev):      # the operators take n_unique from the maps
        c = sc.CONTEXTS[ctx]
        assert (ev.csr_map("jac").nnz, ev.csr_map("hess").nnz) == (c["nnz_j"], c["nnz_h"])

    made, get = _contexts(real_maps)
    yield get
    for ev in made.values():
        ev.close()


@pytest.fixture(scope="module")
def gather_context():
    made, get = _contexts(lambda ctx, ev: None)
    yield get
    for ev in made.values():
        ev.close()


def _i32(a):
    from pockit_amd import runtime

    return None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(runtime.c_int32_p)


class Result:
    """``count`` doubles in the middle of a larger device tensor: NaN (or ``fill``) between sentinels."""

    def __init__(self, torch, dev, count, fill=None):
        host = np.full(count + 2 * PAD, np.nan)
        host[:PAD] = host[PAD + count:] = SENTINEL
        if fill is not None:
            host[PAD: PAD + count] = fill
        self.count, self.buf = count, torch.from_numpy(host).to(dev)
        self.ptr = self.buf.data_ptr() + 8 * PAD

    def fetch(self, what):
        host = self.buf.cpu().numpy()
        edge = np.full(PAD, SENTINEL)
        assert sc.same_bits(host[:PAD], edge) and sc.same_bits(host[PAD + self.count:], edge), f"{what}: a sentinel was overwritten"
        return host[PAD: PAD + self.count].copy()


def _held(what, got, ref, bound, scale, emulated, longest):
    print(f"{what}: worst {sc.worst_units(got, ref, scale):.3e} u*sum|t|, bound {float(sc.gamma(longest) / sc.U):.1f}")
    assert not np.any(np.isnan(got)), f"{what}: entries {np.flatnonzero(np.isnan(got))[:8]} were not written"
    bad = sc.failures(got, ref, bound)
    assert len(bad) == 0, f"{what}: {len(bad)} entries miss the bound, first {bad[:8]}: {got[bad[:8]]} for {ref[bad[:8]]}"
    exact = bound == 0.0
    assert sc.same_bits(got[exact], ref[exact]), f"{what}: an entry that must be exact is not"
    differ = np.flatnonzero(got.view(np.uint64) != emulated.view(np.uint64))
    assert len(differ) == 0, f"{what}: {len(differ)} entries differ in bits from the documented association, first {differ[:8]}"


@pytest.mark.parametrize("case", sc.operator_cases(), ids=lambda c: c.id)
def test_operator_kernels_match_the_exact_row_sums(case, operator_context):
    import torch

    ev = operator_context(case.ctx)
    lib, h = ev.ctx.lib, ev.ctx.handle
    ev.ctx.check(lib.pk_set_csr_operator(h, case.op, _i32(case.indptr), _i32(case.indices), _i32(case.src), case.n_rows,
                                         case.n_cols, case.nnz))
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    vals, v, add = up(case.vals), up(case.v), up(case.add)
    plain, again, added = (Result(torch, dev, case.n_rows) for _ in range(3))
    alias = Result(torch, dev, case.n_rows, fill=case.add)
    torch.cuda.synchronize()            # torch's copies run on its own stream; the context uses its own
    for out, d_add in ((plain, None), (again, None), (added, add.data_ptr()), (alias, alias.ptr)):
        ev.ctx.check(lib.pk_apply_operator_dev(h, case.op, vals.data_ptr(), v.data_ptr(), d_add, out.ptr, None))
    ev.sync()
    plain, again, added, alias = (r.fetch(f"{case.id} {k}") for r, k in ((plain, "plain"), (again, "again"), (added, "add"), (alias, "alias")))
    longest = int(case.lengths.max()) + 1
    _held(f"{case.id} add=NULL", plain, *case.reference[False], case.emulated(False), longest)
    _held(f"{case.id} add given", added, *case.reference[True], case.emulated(True), longest)
    _held(f"{case.id} add aliasing y", alias, *case.reference[True], case.emulated(True), longest)
    assert sc.same_bits(plain, again), f"{case.id}: a second call gave other bits"
    empty = case.lengths == 0
    assert sc.same_bits(plain[empty], np.zeros(int(empty.sum()))) and sc.same_bits(added[empty], case.add[empty])


@pytest.mark.parametrize("case", sc.gather_cases() + sc.gather_cap_cases(), ids=lambda c: c.id)
def test_gather_kernel_matches_the_exact_run_sums(case, gather_context):
    import torch

    ev = gather_context(case.ctx)
    lib, h = ev.ctx.lib, ev.ctx.handle
    ev.ctx.check(lib.pk_set_csr_map(h, 0, _i32(case.seg), _i32(case.perm), case.n_unique, case.n_triplets))
    dev = torch.device("cuda", 0)
    triplets = torch.from_numpy(case.triplets).to(dev)
    first, again = Result(torch, dev, case.n_unique), Result(torch, dev, case.n_unique)
    torch.cuda.synchronize()
    for out in (first, again):
        ev.ctx.check(lib.pk_gather_csr_dev(h, 0, triplets.data_ptr(), out.ptr, None))
    ev.sync()
    first, again = first.fetch(case.id), again.fetch(case.id + " again")
    _held(case.id, first, *case.reference, case.emulated(), max(int(case.runs.max()) - 1, 0))
    assert sc.same_bits(first, again), f"{case.id}: a second call gave other bits"
