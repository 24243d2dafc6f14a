"""tests/ipm_cases.py -- the NumPy emulator of pockit_amd/csrc/pk_ipm.cpp that the host stand-in and the kernels are held to bit
for bit -- against straightforward statements of every vector and column: the plain NumPy expressions per kind of element, Python
loops for the step lengths, ``math.fsum`` for the sums within the tree bound ceil(log2 L + 1) * 2^-53 * sum |term|; the dirty
inputs put exactly the planted sides into ``bad``; and every deliberate mistake of MUTANTS changes some bit.  CPU only."""
import math

import numpy as np
import pytest

import ipm_cases as ip
import sparse_cases as sc

LENGTHS = (1, 255, 257, 2049, 5000)
MU, TAU = 0.0625 * 1.37, 0.995


def _sides_by_loop(b):
    """[(index, slack, multiplier, is_upper)] of every present side, element by element, lower first."""
    out = []
    for i, k in enumerate(b["kind"]):
        if k in (ip.BOTH, ip.LOWER):
            out.append((i, b["v"][i] - b["lb"][i], b["zl"][i], False))
        if k in (ip.BOTH, ip.UPPER):
            out.append((i, b["ub"][i] - b["v"][i], b["zu"][i], True))
    return out


def _within_tree_bound(got, terms, length):
    exact = math.fsum(terms)
    bound = math.ceil(math.log2(max(length, 1)) + 1) * 2.0 ** -53 * math.fsum(abs(t) for t in terms)
    assert abs(got - exact) <= bound, (got, exact, bound)


@pytest.mark.parametrize("length", LENGTHS)
def test_the_terms_are_the_plain_expressions_on_clean_inputs(length):
    b = ip.boxed(length)
    sigma, rbar, rec = ip.emulate_terms(b["lb"], b["ub"], b["v"], b["zl"], b["zu"], MU)
    k, v, lb, ub, zl, zu = (b[n] for n in ("kind", "v", "lb", "ub", "zl", "zu"))
    with np.errstate(all="ignore"):
        want_sigma = np.select([k == ip.BOTH, k == ip.LOWER, k == ip.UPPER], [zl / (v - lb) + zu / (ub - v), zl / (v - lb), zu / (ub - v)], 0.0)
        want_rbar = np.select([k == ip.BOTH, k == ip.LOWER, k == ip.UPPER], [MU / (v - lb) - MU / (ub - v), MU / (v - lb), -(MU / (ub - v))], 0.0)
    assert sc.same_bits(sigma, want_sigma) and sc.same_bits(rbar, want_rbar)
    sides = _sides_by_loop(b)
    assert rec[ip.BAD] == 0.0 and rec[ip.SIDES] == len(sides)
    if not sides:
        assert rec[ip.MIN_SLACK] == np.inf and rec[ip.MIN_COMPL] == np.inf and rec[ip.COMPL_INF] == 0.0 and rec[ip.COMPL_SUM] == 0.0
        return
    assert rec[ip.COMPL_INF] == max(abs(d * z - MU) for _, d, z, _ in sides)
    assert rec[ip.MIN_SLACK] == min(d for _, d, _, _ in sides) and rec[ip.MIN_COMPL] == min(d * z for _, d, z, _ in sides)
    _within_tree_bound(rec[ip.COMPL_SUM], [d * z for _, d, z, _ in sides], length)
    _within_tree_bound(rec[ip.Z_SUM], [z for _, _, z, _ in sides], length)
    _within_tree_bound(rec[ip.LOG_SUM], [float(np.log(d)) for _, d, _, _ in sides], length)


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("with_z,negate", [(False, False), (True, False), (True, True)])
def test_the_residual_is_the_plain_expression(length, with_z, negate):
    b = ip.boxed(length)
    r, rec = ip.emulate_residual(b["lb"], b["ub"], b["t"], b["z"] if with_z else None, negate)
    want = b["t"] - b["z"] if with_z else b["t"].copy()
    want = np.where(b["kind"] == ip.FIXED, 0.0, -want if negate else want)
    assert sc.same_bits(r, want)
    assert rec[ip.R_INF] == np.max(np.abs(want)) and rec[ip.R_BAD] == 0.0 and rec[3] == 0.0
    _within_tree_bound(rec[ip.R_SQ], (want * want).tolist(), length)


@pytest.mark.parametrize("length", LENGTHS)
def test_the_step_is_the_plain_expressions_and_a_python_loop(length):
    b = ip.boxed(length)
    dzl, dzu, rec = ip.emulate_step(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["zu"], MU, TAU)
    k, v, dv, lb, ub, zl, zu = (b[n] for n in ("kind", "v", "dv", "lb", "ub", "zl", "zu"))
    with np.errstate(all="ignore"):
        want_l = np.where((k == ip.BOTH) | (k == ip.LOWER), (MU / (v - lb) - zl) - (zl / (v - lb)) * dv, 0.0)
        want_u = np.where((k == ip.BOTH) | (k == ip.UPPER), (MU / (ub - v) - zu) + (zu / (ub - v)) * dv, 0.0)
    assert sc.same_bits(dzl, want_l) and sc.same_bits(dzu, want_u)
    apri, arg, adual = 1.0, -1.0, 1.0
    for i, d, z, upper in _sides_by_loop(b):
        ds = -dv[i] if upper else dv[i]
        if ds < 0 and (TAU * d) / (-ds) < apri:
            apri, arg = (TAU * d) / (-ds), float(i)
        dz = want_u[i] if upper else want_l[i]
        if dz < 0:
            adual = min(adual, (TAU * z) / (-dz))
    assert (rec[ip.ALPHA_PRI], rec[ip.ALPHA_DUAL], rec[ip.ARG_PRI], rec[ip.STEP_BAD]) == (apri, adual, arg, 0.0)


def test_the_identities_of_a_vector_without_sides():
    for kinds in (ip.FREE, ip.FIXED):
        b = ip.boxed(300, kinds=kinds)
        sigma, rbar, rec = ip.emulate_terms(b["lb"], b["ub"], b["v"], b["zl"], b["zu"], MU)
        assert not sigma.any() and not rbar.any()
        assert sc.same_bits(rec, [0.0, 0.0, 0.0, np.inf, 0.0, 0.0, 0.0, np.inf])
        dzl, dzu, rec = ip.emulate_step(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["zu"], MU, TAU)
        assert not dzl.any() and not dzu.any() and sc.same_bits(rec, [1.0, 1.0, -1.0, 0.0])


def tie(length=3000):
    """Two-sided elements whose step stops at the same quotient at indices 5, 700 and 2900; everything else moves inward."""
    b = ip.boxed(length, kinds=ip.BOTH)
    b["dv"] = np.abs(b["dv"]) * np.where(b["v"] - b["lb"] < b["ub"] - b["v"], 1.0, -1.0) * 1e-6      # (towards the far bound, barely)
    for i in (5, 700, 2900):
        b["lb"][i], b["ub"][i], b["v"][i], b["dv"][i] = -1.0, 3.0, 0.0, -4.0      # (tau * 1) / 4
    return b


def test_a_tie_reports_the_smallest_index_and_no_step_gives_one():
    b = tie()
    _, _, rec = ip.emulate_step(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["zu"], MU, TAU)
    assert rec[ip.ALPHA_PRI] == TAU / 4.0 and rec[ip.ARG_PRI] == 5.0
    _, _, rec = ip.emulate_step(b["lb"], b["ub"], b["v"], np.zeros(len(b["v"])), b["zl"], b["zu"], MU, TAU)
    assert rec[ip.ALPHA_PRI] == 1.0 and rec[ip.ARG_PRI] == -1.0


def test_the_dirty_inputs_put_exactly_the_planted_sides_into_bad():
    b = ip.dirty(2500)
    clean = ip.boxed(2500)
    sigma, rbar, rec = ip.emulate_terms(b["lb"], b["ub"], b["v"], b["zl"], b["zu"], MU)
    assert rec[ip.BAD] == 4.0 and np.all(np.isfinite(rec[[0, 1, 2, 4, 6]])) and np.all(np.isfinite(sigma)) and np.all(np.isfinite(rbar))
    # the bad side's bracket is 0.0, the other side's is what it is alone
    assert sigma[0] == b["zu"][0] / (b["ub"][0] - b["v"][0]) and rbar[0] == -(MU / (b["ub"][0] - b["v"][0]))
    assert sigma[2] == b["zl"][2] / (b["v"][2] - b["lb"][2]) and rbar[2] == MU / (b["v"][2] - b["lb"][2])
    for name, index in ip.PLANTED.items():      # repairing one defect takes exactly one side out of bad
        fixed = {k: a.copy() for k, a in b.items()}
        for k in ("v", "zl", "zu", "dv", "t"):
            fixed[k][index] = {"v": 0.5, "zl": 0.5, "zu": 0.75, "dv": -0.5, "t": 0.25}[k]
        assert ip.emulate_terms(fixed["lb"], fixed["ub"], fixed["v"], fixed["zl"], fixed["zu"], MU)[2][ip.BAD] == (4.0 if name == "nan_step" else 3.0)
        assert ip.emulate_step(fixed["lb"], fixed["ub"], fixed["v"], fixed["dv"], fixed["zl"], fixed["zu"], MU, TAU)[2][ip.STEP_BAD] == 4.0
    dzl, dzu, rec = ip.emulate_step(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["zu"], MU, TAU)
    assert rec[ip.STEP_BAD] == 5.0 and dzl[0] == 0.0 and dzl[1] == 0.0 and dzu[2] == 0.0 and dzl[3] == 0.0 and dzl[4] == 0.0 and dzu[4] == 0.0
    assert np.all(np.isfinite(dzl)) and np.all(np.isfinite(dzu)) and np.all(np.isfinite(rec))
    r, rec = ip.emulate_residual(b["lb"], b["ub"], b["t"], b["z"], False)
    assert rec[ip.R_BAD] == 1.0 and np.isnan(r[4]) and np.all(np.isfinite(rec))
    assert ip.emulate_terms(clean["lb"], clean["ub"], clean["v"], clean["zl"], clean["zu"], MU)[2][ip.BAD] == 0.0


@pytest.mark.parametrize("length", (1, 255, 2049, 5000, 524289))
def test_a_sum_column_is_the_pieced_dot_of_the_solvers(length):
    """One association, two statements: a one-layer sum here is cg_cases.dot, bit for bit, also under the shared mistakes."""
    import cg_cases as cg

    terms = np.random.default_rng(length).uniform(-1.0, 1.0, length)
    assert ip.reduce_column([terms], "sum") == cg.dot(terms)
    assert ip.reduce_column([terms], "sum", "tree_stops_at_2") == cg.dot(terms, "tree_stops_at_2")
    assert ip.reduce_column([terms], "sum", "second_trip_dropped") == cg.dot(terms, "strided_first_trip")
    assert (ip.BLOCK, ip.PIECE) == (cg.BLOCK, cg.PIECE)


def _all_outputs(b, mutant, length):
    out = []
    out += ip.emulate_terms(b["lb"], b["ub"], b["v"], b["zl"], b["zu"], MU, mutant=mutant)
    out += ip.emulate_residual(b["lb"], b["ub"], b["t"], b["z"], True, mutant=mutant)
    out += ip.emulate_step(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["zu"], MU, TAU, mutant=mutant)
    return out


@pytest.mark.parametrize("mutant", ip.MUTANTS)
def test_every_deliberate_mistake_is_caught_by_the_bit_comparison(mutant):
    assert len(ip.MUTANTS) >= 8
    length = 524289 if mutant == "second_trip_dropped" else 3000
    b = tie() if mutant == "arg_largest" else ip.boxed(length)
    cases = [b]
    if mutant == "upper_before_lower":      # (two additions swapped within a thread: most lengths round the difference away again)
        cases = [ip.boxed(20000)]
    if mutant == "fma_dz":
        cases = [ip.boxed(300)]
    if mutant == "tau_after_quotient":      # (only the winning quotient shows it, and one quotient may round alike: six vectors)
        cases = [ip.boxed(40, seed=s) for s in range(1, 7)]
    good = [o for c in cases for o in _all_outputs(c, None, length)]
    bad = [o for c in cases for o in _all_outputs(c, mutant, length)]
    assert any(not sc.same_bits(g, m) for g, m in zip(good, bad)), mutant
