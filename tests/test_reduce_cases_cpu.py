"""Tests of the test: tests/reduce_cases.py, the inputs, exact references, bounds and emulators that
tests/test_gpu_operator_reduce.py holds pk_red_rows, pk_red_long and pk_diag to.  CPU only, numpy only.

* the terms of every case but the full-mantissa one are exact (mantissa widths for all, rational arithmetic for the small ones);
* the emulator of the two sums -- sparse_cases.emulate_operator as it stands, fed the terms -- stays inside the derived bound of
  the ``fsum`` reference for every case, and removing any single term of any row moves the exact sum by at least 2**10 bounds
  (the threshold of tests/test_sparse_cases_cpu.py), with zero exempt rows;
* the emulator of the maximum equals the exact maximum, and every planted entry is its row's unique maximum, lies where the
  case says, and is missed once it is left out;
* the full-mantissa case tells (a a) w from a (a w);
* eight deliberate mistakes are each caught.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import reduce_cases as rc
import sparse_cases as sc

CASES = rc.reduce_cases()
SUMS = [c for c in CASES if c.mode != rc.ABS_MAX]
MAXES = [c for c in CASES if c.mode == rc.ABS_MAX]
PLANTED = [c for c in CASES if c.plant is not None]
ids = lambda c: c.id  # noqa: E731


def test_the_case_list_covers_what_the_gpu_file_promises():
    assert len({c.id for c in CASES}) == len(CASES)
    for name in ("edges", "cut-by-rows", "long-first-and-last", "equal-lengths"):
        assert {(c.op, c.mode) for c in CASES if c.name == name} == {(op, mode) for op in (0, 1, 2) for mode in rc.MODES}, name
    assert {c.mode for c in CASES if c.name == "pieces"} == set(rc.MODES)
    assert [c.lengths[:3].tolist() for c in CASES if c.name == "pieces"][0] == [65536, 65537, 131329]
    for mode in rc.MODES:
        assert {c.with_w for c in CASES if c.mode == mode} == {True, False}
        assert {c.src is None for c in CASES if c.mode == mode} == {True, False}
    past = [c for c in CASES if c.ctx == "C"]
    assert {c.name for c in past} == {"blocks-past-the-cap", "longs-past-the-cap"} and all(c.op == 2 for c in past)
    for c in past:
        blocks, longs, _ = sc.row_blocks(c.indptr)
        assert (len(blocks) if c.name.startswith("blocks") else len(longs)) > sc.OP_GRID_CAP
    assert {c.name for c in PLANTED} == {"planted-" + k for k in rc.PLANTS} and len(rc.PLANTS) == 9
    assert sum(c.full_mantissa for c in CASES) == 1
    assert sorted((c.ctx, c.op) for c in CASES if c.name == "no-src") == [(ctx, op) for ctx in "AB" for op in (0, 1, 2)]
    assert len(CASES) == 64


def test_the_inputs_are_what_the_module_promises():
    for case in CASES:
        q = case.w if not case.full_mantissa else None
        if q is not None:
            m = np.frexp(q)[0]
            assert np.all(m * 32 == np.round(m * 32)) and np.all((q >= 0.5) & (q < 4.0)), case.id      # 5-bit mantissas
            assert np.array_equal(np.float32(case.vals).astype(np.float64), case.vals)    # 24-bit mantissas (16 a is as wide as a)
        power = np.asarray(sc.BUCKETS)[case.row_of % 5] * (2 if case.mode == rc.SQ_SUM else 1)
        t = case.terms() / np.ldexp(1.0, power)
        top = 4.0 * 4.0 * 2.25 * 1.5 if case.mode == rc.SQ_SUM else 2.0 * 4.0 * 2.25
        live = np.ones(case.nnz, dtype=bool)
        if case.plant is not None:
            live[case.planted_entry] = False
        assert np.all(t[live] >= (0.5 if case.with_w else 1.0)) and np.all(t[live] < top), case.id


@pytest.mark.parametrize("case", [c for c in CASES if not c.full_mantissa], ids=ids)
def test_terms_are_exact(case):
    """53 significant bits at the most by construction; the rational product itself where the case is small."""
    a = case.values()
    t = case.terms()
    if case.nnz <= 20000:
        w = case.w[case.indices] if case.with_w else np.ones(case.nnz)
        for e in range(case.nnz):
            x = Fraction(float(a[e]))
            want = (x * x if case.mode == rc.SQ_SUM else abs(x)) * Fraction(float(w[e]))
            assert Fraction(float(t[e])) == want, (case.id, e)
    # for every size: the integer mantissas multiply without overflow of 53 bits
    ma = np.abs(np.frexp(a)[0]) * 2.0 ** 24
    assert np.array_equal(ma, np.round(ma))
    if case.with_w:
        mw = np.frexp(case.w[case.indices])[0] * 32.0
        assert np.array_equal(mw, np.round(mw))
        bits = (ma * ma if case.mode == rc.SQ_SUM else ma) * mw
        assert np.all(bits < 2.0 ** 53)


@pytest.mark.parametrize("case", SUMS, ids=ids)
def test_sum_emulator_stays_inside_the_bound(case):
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


@pytest.mark.parametrize("case", SUMS, ids=ids)
def test_sum_rows_are_sensitive_to_every_single_term(case):
    p = case.products().tolist()
    checked, least = 0, math.inf
    for r in np.flatnonzero(case.lengths > 0):
        t = p[case.indptr[r]: case.indptr[r + 1]]
        for with_add in (False, True):
            bound = float(case.reference[with_add][1][r])
            assert min(t) > 0.0 and min(t) >= 1024.0 * bound, (case.id, r)      # the exact sum moves by exactly the term
            if bound > 0.0:
                least = min(least, min(t) / bound)
        checked += 1
    assert checked == int((case.lengths > 0).sum())                 # zero exempt rows
    print(f"{case.id}: a lost term moves its row by at least 2**{math.log2(least):.1f} bounds")
    if case.name == "edges" and case.mode == rc.SQ_SUM and not case.full_mantissa:
        assert least >= 2.0 ** 30


@pytest.mark.parametrize("case", MAXES, ids=ids)
def test_max_emulator_is_the_exact_maximum(case):
    for with_add in (False, True):
        got, ref = case.emulated(with_add), case.max_reference[with_add]
        assert sc.same_bits(got, ref), case.id
        assert np.all(got >= 0.0) and not np.any(np.signbit(got))


def test_add_decides_some_rows_of_the_maximum_and_loses_others():
    """(A row of hundreds of entries has a term near the top of the range: add wins in the short rows.)"""
    deciding = 0
    for case in MAXES:
        rows = np.flatnonzero(case.lengths > 0)
        wins = case.add[rows] > case.max_reference[False][rows]
        assert not wins.all(), case.id
        deciding += bool(wins.any())
    assert deciding >= 10


@pytest.mark.parametrize("case", PLANTED, ids=ids)
def test_the_planted_entry_is_the_unique_maximum_and_lies_where_it_says(case):
    row, offset = case.plant
    e = case.planted_entry
    t = case.terms()
    lo, hi = int(case.indptr[row]), int(case.indptr[row + 1])
    others = np.delete(t[lo:hi], offset)
    assert t[e] >= 8.0 * np.ldexp(1.0, sc.BUCKETS[row % 5])
    assert len(others) == 0 or t[e] > others.max()
    assert t[e] > abs(case.add[row])
    for with_add in (False, True):
        assert case.max_reference[with_add][row] == t[e]
    # leaving the planted entry out is seen
    lost = t.copy()
    lost[e] = 0.0
    assert rc.emulate_max(case, lost, case.add)[row] != t[e]
    # ... and it lies at the place of the walk its name states
    blocks, longs, _ = sc.row_blocks(case.indptr)
    name = case.name[len("planted-"):]
    if name.startswith("stream"):
        b = [b for b in blocks if b[3] >= 0 and b[2] <= row < b[2] + b[3]][0]
        assert b[3] > 1 and b[0] < lo and hi < b[0] + b[1]               # rows in front of it and behind it in the block
        assert offset == (0 if name.endswith("first") else hi - lo - 1)
    else:
        long = [l for l in longs if l[0] == row][0]
        piece, within = divmod(offset, sc.BLOCK)
        want = {"index-0": (0, 0), "last-entry": (long[2] - 1, sc.BLOCK - 1), "offset-255-of-a-piece": (0, 255),
                "offset-0-of-the-next-piece": (1, 0), "last-piece-of-one": (long[2] - 1, 0), "piece-256": (256, 0),
                "piece-255": (255, 255)}[name]
        assert (piece, within) == want
        if name == "last-piece-of-one":
            assert (hi - lo) % sc.BLOCK == 1
        if name == "last-entry":
            assert offset == hi - lo - 1
        if name == "piece-256":
            assert long[2] > sc.BLOCK                                     # the second trip of the strided walk


def test_the_full_mantissa_case_pins_the_rounding_order():
    case = [c for c in CASES if c.full_mantissa][0]
    a, w = case.values(), case.w[case.indices]
    kernel, other = (a * a) * w, a * (a * w)
    assert sc.same_bits(case.terms(), kernel)
    assert int((kernel != other).sum()) > case.nnz // 10
    for with_add in (False, True):
        alt = sc.emulate_operator(rc._Mutated(case, other), case.add if with_add else None)
        assert not sc.same_bits(alt, case.emulated(with_add))


def _caught(case, with_add, mutant):
    got = case.emulated(with_add, mutant)
    if case.mode == rc.ABS_MAX:
        return not sc.same_bits(got, case.max_reference[with_add])
    ref, bound, _ = case.reference[with_add]
    by_bound, by_bits = len(sc.failures(got, ref, bound)) > 0, not sc.same_bits(got, case.emulated(with_add))
    assert by_bits or not by_bound
    return by_bound


@pytest.mark.parametrize("mutant", rc.TERM_MUTANTS + rc.MAX_MUTANTS + rc.WALK_MUTANTS)
def test_reduce_mutants_are_caught(mutant):
    seen = {mode: [c.id for c in CASES for with_add in (False, True) if c.mode == mode and _caught(c, with_add, mutant)]
            for mode in rc.MODES}
    print(f"{mutant}: caught on {({m: len(v) for m, v in seen.items()})}")
    if mutant in rc.MAX_MUTANTS:
        assert seen[rc.ABS_MAX]
    elif mutant == "fabs_dropped":
        assert seen[rc.ABS_SUM] and seen[rc.ABS_MAX]                 # (a square has no sign to lose)
    else:
        assert all(seen.values()), seen
    if mutant in rc.WALK_MUTANTS:                                    # the maximum sees them through the plantings
        planted = {c.name for c in PLANTED if _caught(c, False, mutant)}
        assert planted, mutant
        if mutant == "strided_first_trip":
            assert "planted-piece-256" in planted and "planted-piece-255" not in planted


def test_the_diagonal_mutant_is_caught():
    for n, n_unique in ((53, 46), (1205, 1198)):
        pos = rc.diagonal_positions(n, n_unique, seed=n)
        assert pos[0] == -1 and pos[-1] == -1 and int((pos == -1).sum()) >= 9 and pos.min() == -1 and pos.max() == n_unique - 1
        vals = np.random.default_rng(n).standard_normal(n_unique) + 3.0
        add = np.random.default_rng(n + 1).standard_normal(n)
        for a in (None, add):
            want = np.array([(vals[p] if p >= 0 else 0.0) + (0.0 if a is None else a[i]) for i, p in enumerate(pos)])
            assert sc.same_bits(rc.emulate_diagonal(vals, pos, a), want)
            assert not sc.same_bits(rc.emulate_diagonal(vals, pos, a, "pos_minus_one_as_zero"), want)


def test_the_mutant_list_is_the_eight_of_the_issue():
    assert len(rc.MUTANTS) == 8 and len(set(rc.MUTANTS)) == 8


def test_diagonal_src_of_a_lower_triangular_map():
    from pockit_amd.csr import CsrMap

    rng = np.random.default_rng(5)
    rows, cols = rng.integers(0, 40, 300), rng.integers(0, 40, 300)
    rows, cols = np.maximum(rows, cols), np.minimum(rows, cols)
    keep = ~((rows == cols) & (rows % 3 == 0))                        # rows without a diagonal entry
    keep &= rows != 7                                                 # an empty row
    m = CsrMap(rows[keep], cols[keep], (40, 40))
    pos = m.diagonal_src()
    assert pos.dtype == np.int32 and pos.shape == (40,) and pos[7] == -1 and pos[0] == -1
    vals = rng.standard_normal(m.nnz)
    assert np.array_equal(rc.emulate_diagonal(vals, pos), m.to_scipy(vals).diagonal())
    assert (pos >= 0).sum() == np.count_nonzero(m.to_scipy(np.ones(m.nnz)).diagonal())
    with pytest.raises(ValueError, match="above the diagonal"):
        CsrMap([0, 1], [1, 1], (2, 2)).diagonal_src()
    with pytest.raises(ValueError, match="square"):
        CsrMap([0, 1], [0, 0], (2, 3)).diagonal_src()
