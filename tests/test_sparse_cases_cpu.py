"""Tests of the test: tests/sparse_cases.py, the inputs, exact references, bounds and emulators that
tests/test_gpu_sparse_kernels.py holds pk_op_rows, pk_op_long and pk_csr to.  CPU only, numpy only.

* the emulator of the documented association stays inside the derived bound of the ``fsum`` reference, for every structure the
  GPU file uses;
* sensitivity, with zero exempt rows: removing any single term of any row, or counting it twice, moves the exact sum by at least
  2**10 times that row's bound (every term of a row is within a factor of 4 of every other, so the ratio is at least
  1 / (4 (L + 1)**2 u), 1.3e5 at the longest row used) -- asserted, not assumed;
* six deliberate mistakes in the emulator are each caught by the checker on at least one case;
* the structures are what the block cutter sees: stream and piece counts and the number of long rows match a Python
  transcription of pk_op_row_blocks;
* the gather cases past pk_csr's grid cap really exceed it (more slices, and more entries, than 4 096 workgroups take in one
  trip), and a stride loop left after its first trip is caught.
"""
import math

import numpy as np
import pytest

import sparse_cases as sc

OPERATOR_CASES, GATHER_CASES = sc.operator_cases(), sc.gather_cases()
ids = lambda c: c.id  # noqa: E731


def _caught(case, got, with_add=None):
    """What the GPU file asserts of a result: the bound against fsum and bit equality with the emulator."""
    if isinstance(case, sc.OperatorCase):
        ref, bound, _ = case.reference[with_add]
        return len(sc.failures(got, ref, bound)) > 0, not sc.same_bits(got, case.emulated(with_add))
    ref, bound, _ = case.reference
    return len(sc.failures(got, ref, bound)) > 0, not sc.same_bits(got, case.emulated())


def test_the_context_table_matches_the_plans():
    import importlib

    import models
    from pockit_amd.csr import CsrMap

    for c in sc.CONTEXTS.values():
        name, scheme, mesh, num_point = c["model"]
        plan = getattr(models, name)(importlib.import_module(f"pockit_amd.{scheme}"), mesh, num_point)[0].plan
        mj = CsrMap(plan.jac_row, plan.jac_col, (plan.m, plan.n))
        mh = CsrMap(plan.hess_row, plan.hess_col, (plan.n, plan.n))
        assert (plan.n, plan.m, mj.nnz, mh.nnz, mj.n_triplets, plan.nnz_J) == (c["n"], c["m"], c["nnz_j"], c["nnz_h"], c["trip_j"], c["trip_j"])


def test_the_inputs_are_what_the_module_promises():
    for case in OPERATOR_CASES:
        for a in (case.vals, case.v):
            assert np.array_equal(np.float32(a).astype(np.float64), a)              # 24-bit mantissas: exact products
        mag = np.abs(case.products())
        scale = np.ldexp(1.0, np.asarray(sc.BUCKETS)[case.row_of % 5])
        assert np.all((mag >= scale) & (mag < 4.0 * scale)), case.id                # a row's terms within a factor of 4
        assert case.indices.min() >= 0 and case.indices.max() < case.n_cols
        assert (case.src is None) == (case.name == "no-src")
        if case.src is not None:
            assert case.src.min() >= 0 and case.src.max() < case.n_unique
        for r in np.flatnonzero(case.lengths <= case.n_cols):                       # ascending and distinct while the row fits
            assert np.all(np.diff(case.indices[case.indptr[r]: case.indptr[r + 1]]) > 0)
    assert {c.ctx for c in OPERATOR_CASES if c.src is None} == set(sc.CONTEXTS)
    for case in GATHER_CASES:
        assert sorted(case.perm.tolist()) == list(range(case.n_triplets))
        mag = np.abs(case.triplets[case.perm])
        scale = np.ldexp(1.0, np.asarray(sc.BUCKETS)[np.repeat(np.arange(case.n_unique), case.runs) % 5])
        assert np.all((mag >= scale) & (mag < 2.0 * scale)), case.id


def test_the_gather_cases_cover_what_the_gpu_file_promises():
    widths = set()
    for case in GATHER_CASES:
        if case.seg is not None:
            widths |= set(case.slice_width.tolist())
    assert set(sc.GATHER_WIDTHS) <= widths and 3000 in widths
    assert {0, 1, 255} <= {c.n_unique % sc.BLOCK for c in GATHER_CASES}
    ragged = [c for c in GATHER_CASES if c.seg is not None and any(
        len(set(c.runs[b * sc.BLOCK: (b + 1) * sc.BLOCK].tolist())) > 1 for b in range(len(c.slice_width)))]
    assert len(ragged) >= 7
    ones = [c for c in GATHER_CASES if c.seg is not None and 1 in c.slice_width.tolist() and c.slice_width.max() > 1]
    assert ones, "a slice made entirely of runs of 1 inside a map that has seg"
    assert any(c.seg is None and c.ctx == "B" for c in GATHER_CASES)


@pytest.mark.parametrize("case", OPERATOR_CASES, ids=ids)
def test_operator_emulator_stays_inside_the_bound(case):
    for with_add in (False, True):
        ref, bound, scale = case.reference[with_add]
        got = case.emulated(with_add)
        print(f"{case.id} add={with_add}: worst {sc.worst_units(got, ref, scale):.3e} u*sum|t|, bound {float(sc.gamma(case.lengths.max() + 1) / sc.U):.1f}")
        assert len(sc.failures(got, ref, bound)) == 0
        exact = bound == 0.0
        assert sc.same_bits(got[exact], ref[exact])
    empty = case.lengths == 0
    assert sc.same_bits(case.emulated(False)[empty], np.zeros(int(empty.sum())))
    assert sc.same_bits(case.emulated(True)[empty], case.add[empty])


@pytest.mark.parametrize("case", GATHER_CASES, ids=ids)
def test_gather_emulator_stays_inside_the_bound(case):
    ref, bound, scale = case.reference
    got = case.emulated()
    print(f"{case.id}: worst {sc.worst_units(got, ref, scale):.3e} u*sum|t|, bound {float(sc.gamma(case.runs.max() - 1) / sc.U):.1f}")
    assert len(sc.failures(got, ref, bound)) == 0
    assert sc.same_bits(got[case.runs == 1], ref[case.runs == 1])


def _sensitivity(terms, bound, extra=()):
    """Every term of the row against 2**10 bounds (an exact statement: the exact sum moves by exactly |t|), and literally for
    the smallest one, which is the hardest to see: the correctly rounded sum without it, and with it twice."""
    mags = [abs(x) for x in terms]
    assert min(mags) > 0.0 and min(mags) >= 1024.0 * bound
    k = mags.index(min(mags))
    full = math.fsum(list(terms) + list(extra))
    dropped = math.fsum(list(terms[:k]) + list(terms[k + 1:]) + list(extra))
    doubled = math.fsum(list(terms) + [terms[k]] + list(extra))
    assert abs(full - dropped) >= 1024.0 * bound and abs(doubled - full) >= 1024.0 * bound
    assert abs(full - dropped) > 0.0 and abs(doubled - full) > 0.0


@pytest.mark.parametrize("case", OPERATOR_CASES, ids=ids)
def test_operator_rows_are_sensitive_to_every_single_term(case):
    p = case.products().tolist()
    checked = 0
    for r in np.flatnonzero(case.lengths > 0):                       # (a row without terms has none to lose)
        t = p[case.indptr[r]: case.indptr[r + 1]]
        _sensitivity(t, float(case.reference[False][1][r]))
        _sensitivity(t, float(case.reference[True][1][r]), extra=[float(case.add[r])])
        checked += 1
    assert checked == int((case.lengths > 0).sum())                 # zero exempt rows


@pytest.mark.parametrize("case", GATHER_CASES, ids=ids)
def test_gather_entries_are_sensitive_to_every_single_triplet(case):
    t = case.triplets[case.perm].tolist()
    bound = case.reference[1]
    for p in range(case.n_unique):
        _sensitivity(t[case.start[p]: case.start[p + 1]], float(bound[p]))


@pytest.mark.parametrize("mutant", sc.OPERATOR_MUTANTS)
def test_operator_mutants_are_caught(mutant):
    by_bound, by_bits = [], []
    for case in OPERATOR_CASES:
        for with_add in (False, True):
            bound, bits = _caught(case, sc.emulate_operator(case, case.add if with_add else None, mutant), with_add)
            assert bits or not bound                                  # (whatever misses the bound differs in bits too)
            if bound:
                by_bound.append(case.id)
            if bits:
                by_bits.append(case.id)
    print(f"{mutant}: misses the bound on {sorted(set(by_bound))}")
    assert by_bound, f"no case sees the mutant {mutant} through the bound"
    assert by_bits


@pytest.mark.parametrize("mutant", sc.GATHER_MUTANTS)
def test_gather_mutants_are_caught(mutant):
    by_bound = [case.id for case in GATHER_CASES if _caught(case, sc.emulate_gather(case, mutant))[0]]
    print(f"{mutant}: misses the bound on {by_bound}")
    assert by_bound
    # the remainder loop matters at every width that is no multiple of 4: each of them is caught by itself
    seen = set()
    for case in GATHER_CASES:
        if case.seg is None:
            continue
        ref, bound, _ = case.reference
        bad = sc.failures(sc.emulate_gather(case, mutant), ref, bound)
        seen |= set(case.slice_width[np.unique(bad // sc.BLOCK)].tolist())
    assert {w for w in sc.GATHER_WIDTHS if w % 4} <= seen


def test_the_mutant_list_is_the_six_of_the_module():
    assert len(sc.MUTANTS) == 6 and len(set(sc.MUTANTS)) == 6


@pytest.mark.parametrize("case", OPERATOR_CASES, ids=ids)
def test_structures_are_what_the_block_cutter_sees(case):
    blocks, longs, n_slots = sc.row_blocks(case.indptr)
    stream = [b for b in blocks if b[3] >= 0]
    pieces = [b for b in blocks if b[3] < 0]
    assert len(pieces) == case.expect_pieces == n_slots and len(longs) == case.expect_longs
    if case.expect_stream is not None:
        assert [b[1] for b in stream if b[1] > 0] == case.expect_stream
    # every row in exactly one work item, every entry in exactly one block, nothing beyond a workgroup
    rows = [r for b in stream for r in range(b[2], b[2] + b[3])] + [l[0] for l in longs]
    assert sorted(rows) == list(range(case.n_rows))
    assert sum(b[1] for b in blocks) == case.nnz and all(0 <= b[1] <= sc.BLOCK for b in blocks)
    assert all(0 < b[3] <= sc.BLOCK for b in stream) and all(b[1] > 0 for b in pieces)
    assert sorted(b[2] for b in pieces) == list(range(n_slots))
    for row, first, count in longs:
        assert count == -(-int(case.lengths[row]) // sc.BLOCK) and case.lengths[row] > sc.BLOCK


def test_the_cases_reach_the_paths_they_are_named_for():
    by_id = {c.id: c for c in OPERATOR_CASES}
    blocks, longs, _ = sc.row_blocks(by_id["C-blocks-past-the-cap-op2"].indptr)
    assert len(blocks) > sc.OP_GRID_CAP and 0 < len(longs) < sc.OP_GRID_CAP          # the stride loop of pk_op_rows
    blocks, longs, _ = sc.row_blocks(by_id["C-longs-past-the-cap-op2"].indptr)
    assert len(longs) > sc.OP_GRID_CAP                                               # the stride loop of pk_op_long
    _, longs, _ = sc.row_blocks(by_id["A-pieces-op0"].indptr)
    assert [l[2] for l in longs] == [256, 257, 514] and by_id["A-pieces-op0"].lengths[2] % sc.BLOCK == 1
    stream = [b for b in sc.row_blocks(by_id["B-cut-by-rows-op0"].indptr)[0]]
    assert [b[3] for b in stream[:2]] == [sc.BLOCK, sc.BLOCK]                        # cut by the 256-row limit
    for ctx in "AB":
        assert {c.op for c in OPERATOR_CASES if c.ctx == ctx and c.name != "no-src"} == {0, 1, 2}
    assert max(int(c.nnz) for c in OPERATOR_CASES) == 2100 * 257


# ---------------------------------------------------------------- pk_csr past its grid cap
def test_the_cap_context_matches_its_plan_and_is_the_smallest_mesh_past_the_cap():
    import importlib

    import models

    c = sc.CAP_CONTEXT
    name, scheme, mesh, num_point = c["model"]
    ns = importlib.import_module(f"pockit_amd.{scheme}")
    plan = getattr(models, name)(ns, mesh, num_point)[0].plan
    assert (plan.n, plan.m, plan.nnz_J) == (c["n"], c["m"], c["trip_j"])
    assert len(set(zip(plan.jac_row.tolist(), plan.jac_col.tolist()))) == c["nnz_j"] == c["trip_j"]      # J has no repeats: seg = NULL
    assert plan.nnz_J > sc.CSR_GRID_CAP * sc.BLOCK + 512
    assert getattr(models, name)(ns, mesh - 1, num_point)[0].plan.nnz_J <= sc.CSR_GRID_CAP * sc.BLOCK + 512


@pytest.mark.parametrize("case", sc.gather_cap_cases(), ids=ids)
def test_the_gather_cases_past_the_cap_take_a_second_trip(case):
    nblk = -(-case.n_unique // sc.BLOCK)
    assert sorted(case.perm.tolist()) == list(range(case.n_triplets))
    ref, bound, scale = case.reference
    got = case.emulated()
    assert len(sc.failures(got, ref, bound)) == 0 and sc.same_bits(got[case.runs == 1], ref[case.runs == 1])
    if case.seg is None:      # the elementwise loop: thread p, then p + 4 096 * 256
        assert case.n_unique > sc.CSR_GRID_CAP * sc.BLOCK + 512
    else:                     # the slice loop: workgroup b, then b + 4 096
        assert nblk > sc.CSR_GRID_CAP, "the shape must exceed the cap"
        assert case.n_unique == 1048577 + 255
        late = np.flatnonzero(case.runs[sc.CSR_GRID_CAP * sc.BLOCK:] > 1) + sc.CSR_GRID_CAP * sc.BLOCK
        assert sorted(case.runs[late].tolist()) == [2, 5] and late.max() == case.n_unique - 1      # (the last entry of the last slice)
        assert case.slice_width[sc.CSR_GRID_CAP] == 5 and case.slice_width[0] > 8                   # unrolled loop + remainder on both trips
        assert int((case.runs > 1).sum()) == 3
        for p in np.flatnonzero(case.runs > 1):
            t = case.triplets[case.perm].tolist()[case.start[p]: case.start[p + 1]]
            _sensitivity(t, float(bound[p]))
    # the mistake: a stride loop that ends after its first trip leaves what lies beyond the cap unwritten
    dropped = sc.emulate_gather(case, sc.GATHER_CAP_MUTANT)
    by_bound, by_bits = _caught(case, dropped)
    assert by_bound and by_bits, "second trip dropped: not caught"
    bad = sc.failures(dropped, ref, bound)
    assert bad.min() == sc.CSR_GRID_CAP * sc.BLOCK and len(bad) == case.n_unique - sc.CSR_GRID_CAP * sc.BLOCK
