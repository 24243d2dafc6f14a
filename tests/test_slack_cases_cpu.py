"""tests/slack_cases.py, the emulator the kernels of pockit_amd/csrc/pk_slack.cpp are held to, held itself to statements that
owe nothing to it: the vectors (s2, b2, ds, the updated vectors and their clamps) bit-equal to plain NumPy expressions written
out here; the sums within ``ceil(log2 L + 1) * 2^-53 * sum |term|`` of ``math.fsum``, the maxima, minima and counts exact;
exactly the planted elements in ``bad``; and every deliberate mistake of ``slack_cases.MUTANTS`` caught by the bit comparison.
CPU only."""
import math

import numpy as np
import pytest

import slack_cases as sl
import sparse_cases as sc

MU, KAPPA, AP, AD = 0.0625 * 1.37, sl.KAPPA, 0.8125 * 0.93, 0.71
LENGTHS = (1, 255, 257, 2049, 70001)      # (70001: 35 pieces; the GPU file walks the long ones)


def _sum_ok(got, terms):
    terms = np.asarray(terms, dtype=np.float64)
    L = max(len(terms), 1)
    bound = math.ceil(math.log2(L) + 1) * 2.0 ** -53 * math.fsum(np.abs(terms))
    return abs(got - math.fsum(terms)) <= bound


def _same(a, b):
    return sc.same_bits(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


@pytest.mark.parametrize("m", LENGTHS)
def test_reduce_is_the_plain_expressions(m):
    b = sl.rows(m)
    s2, b2, rec = sl.emulate_reduce(b["lb"], b["ub"], b["g"], b["s"], b["lam"], b["sigma_s"], b["rbar_s"])
    eq = b["lb"] == b["ub"]
    with np.errstate(invalid="ignore"):
        want_s2 = np.where(eq, 0.0, 1.0 / b["sigma_s"])
        want_b2 = np.where(eq, -(b["g"] - b["lb"]), -(b["g"] - b["s"]) + want_s2 * (b["lam"] + b["rbar_s"]))
        r = np.abs(np.where(eq, b["g"] - b["lb"], b["g"] - b["s"]))
    assert _same(s2, want_s2) and _same(b2, want_b2)
    assert rec[sl.THETA_INF] == r.max() and _sum_ok(rec[sl.THETA_1], r) and rec[sl.RED_BAD] == 0.0 and rec[sl.RED_ROWS] == (~eq).sum()


@pytest.mark.parametrize("n,m", [(1, 1), (257, 255), (2049, 2047), (70001, 4500), (0, 300), (300, 0)])
def test_recover_is_the_plain_expressions(n, m):
    x, b = sl.variables(n), sl.rows(m)
    ds, rec = sl.emulate_recover(x["lb"], x["ub"], b["lb"], b["ub"], b["dlam"], b["lam"], b["rbar_s"], b["s2"], b["sigma_s"], x["dx"], x["w"],
                                 x["s1"])
    eq, free = b["lb"] == b["ub"], x["lb"] != x["ub"]
    with np.errstate(invalid="ignore"):
        want = np.where(eq, 0.0, b["s2"] * ((b["dlam"] + b["lam"]) + b["rbar_s"]))
    assert _same(ds, want)
    dx, w, s1 = x["dx"][free], x["w"][free], x["s1"][free]
    assert _sum_ok(rec[sl.CURV_X], dx * w + s1 * (dx * dx)) and _sum_ok(rec[sl.DX_SQ], dx * dx)
    assert _sum_ok(rec[sl.CURV_S], b["sigma_s"][~eq] * (want[~eq] * want[~eq])) and _sum_ok(rec[sl.DS_SQ], want[~eq] * want[~eq])
    assert rec[sl.REC_BAD] == 0.0


@pytest.mark.parametrize("m", LENGTHS)
@pytest.mark.parametrize("with_lam", (False, True))
def test_update_is_the_plain_expressions(m, with_lam):
    b = sl.rows(m)
    lam = (b["lam"], b["dlam"]) if with_lam else (None, None)
    v, zl, zu, lam_new, rec = sl.emulate_update(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["dzl"], b["zu"], b["dzu"], AP, AD, MU, KAPPA, *lam)
    boxed = b["lb"] != b["ub"]
    lo, up = boxed & np.isfinite(b["lb"]), boxed & np.isfinite(b["ub"])
    with np.errstate(invalid="ignore"):
        want_v = np.where(boxed, b["v"] + AP * b["dv"], b["v"])
        dl, du = want_v - b["lb"], b["ub"] - want_v
        want_zl = np.where(lo, np.minimum(np.maximum(b["zl"] + AD * b["dzl"], MU / (KAPPA * dl)), (KAPPA * MU) / dl), b["zl"])
        want_zu = np.where(up, np.minimum(np.maximum(b["zu"] + AD * b["dzu"], MU / (KAPPA * du)), (KAPPA * MU) / du), b["zu"])
    assert _same(v, want_v) and _same(zl, want_zl) and _same(zu, want_zu)
    assert (lam_new is None) if not with_lam else _same(lam_new, b["lam"] + AP * b["dlam"])
    slacks = np.concatenate((dl[lo], du[up]))
    assert rec[sl.MIN_SLACK] == (slacks.min() if len(slacks) else np.inf) and rec[sl.UPD_BAD] == 0.0 and rec[3] == 0.0
    with np.errstate(invalid="ignore"):
        moved = (lo & (want_zl != b["zl"] + AD * b["dzl"])).sum() + (up & (want_zu != b["zu"] + AD * b["dzu"])).sum()
    assert rec[sl.CLAMPED] == moved
    # alpha = 0 leaves every bit
    v0, zl0, zu0, lam0, _ = sl.emulate_update(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["dzl"], b["zu"], b["dzu"], 0.0, 0.0, MU, KAPPA, *lam)
    assert _same(v0, b["v"]) and _same(zl0, b["zl"]) and _same(zu0, b["zu"]) and (lam0 is None or _same(lam0, b["lam"]))


def test_the_safeguard_clamps_from_both_sides_and_counts():
    b = sl.rows(600, kinds=sl.ip.BOTH)
    b["zl"][3], b["zu"][7], b["zl"][11] = 1e-30, 1e30, MU / (b["v"][11] - b["lb"][11])
    b["dzl"][3] = b["dzu"][7] = b["dzl"][11] = 0.0
    _, zl, zu, _, rec = sl.emulate_update(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["dzl"], b["zu"], b["dzu"], 0.0, 1.0, MU, 10.0)
    assert zl[3] == MU / (10.0 * (b["v"][3] - b["lb"][3])) and zu[7] == (10.0 * MU) / (b["ub"][7] - b["v"][7]) and zl[11] == b["zl"][11]
    assert rec[sl.CLAMPED] >= 2.0
    again = sl.emulate_update(b["lb"], b["ub"], b["v"], b["dv"], zl, np.zeros(600), zu, np.zeros(600), 0.0, 1.0, MU, 10.0)
    assert again[4][sl.CLAMPED] == 0.0 and _same(again[1], zl) and _same(again[2], zu)      # (already clamped: left as it is)


@pytest.mark.parametrize("n,m,count", [(1, 1, 1), (257, 255, 3), (2049, 4500, 3), (0, 300, 2)])
def test_merit_is_the_plain_expressions(n, m, count):
    x, b = sl.variables(n), sl.rows(m)
    X, G, alphas = sl.trial_points(x, b, count)
    out = sl.emulate_merit(x["lb"], x["ub"], b["lb"], b["ub"], X, G, b["s"], b["ds"], alphas)
    eq = b["lb"] == b["ub"]
    xlo, xup = sl.ip.sides(x["lb"], x["ub"])
    rlo, rup = sl.ip.sides(b["lb"], b["ub"])
    for k in range(count):
        with np.errstate(invalid="ignore"):
            st = b["s"] + alphas[k] * b["ds"]
            r = np.abs(np.where(eq, G[k] - b["lb"], G[k] - st))
            logs = np.concatenate((np.log((X[k] - x["lb"])[xlo]), np.log((x["ub"] - X[k])[xup]), np.log((st - b["lb"])[rlo]), np.log((b["ub"] - st)[rup])))
        assert _sum_ok(out[k, sl.M_THETA_1], r) and out[k, sl.M_THETA_INF] == r.max() and out[k, sl.M_BAD] == 0.0
        L = max(n + m, 1)
        assert abs(out[k, sl.M_LOG] - math.fsum(logs)) <= math.ceil(math.log2(L) + 1) * 2.0 ** -53 * math.fsum(np.abs(logs))


def test_exactly_the_planted_elements_are_bad():
    m, n = 3000, 2500
    x, b = sl.variables(n, kinds=sl.ip.BOTH), sl.rows(m, kinds=sl.ip.BOTH)
    b["sigma_s"][[4, 2100]] = 0.0, np.inf
    b["g"][9] = np.nan
    s2, b2, rec = sl.emulate_reduce(b["lb"], b["ub"], b["g"], b["s"], b["lam"], b["sigma_s"], b["rbar_s"])
    assert rec[sl.RED_BAD] == 3.0 and s2[4] == b2[4] == s2[2100] == b2[2100] == 0.0 and np.isnan(b2[9]) and np.isfinite(rec).all()
    x["w"][17] = np.inf
    ds, rec = sl.emulate_recover(x["lb"], x["ub"], b["lb"], b["ub"], b["dlam"], b["lam"], b["rbar_s"], b["s2"], b["sigma_s"], x["dx"], x["w"],
                                 x["s1"])
    assert rec[sl.REC_BAD] == 3.0 and ds[4] == ds[2100] == 0.0 and np.isfinite(rec).all()
    b["dv"][5], b["dzl"][6], b["dv"][2500] = np.nan, np.inf, 100.0      # a NaN step, an infinite multiplier step, a step across the bound
    v, zl, zu, lam, rec = sl.emulate_update(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["dzl"], b["zu"], b["dzu"], 1.0, 1.0, MU, KAPPA,
                                            b["lam"], b["dlam"])
    assert rec[sl.UPD_BAD] == 3.0 and np.isnan(v[5]) and np.isinf(zl[6]) and np.isfinite(rec[:1]).all() and rec[sl.MIN_SLACK] > 0.0
    X, G, alphas = sl.trial_points(x, b, 3)
    X[1, 40], G[2, 50] = x["lb"][40], np.inf
    b["ds"][60] = 1e6
    out = sl.emulate_merit(x["lb"], x["ub"], b["lb"], b["ub"], X, G, b["s"], b["ds"], alphas)
    assert out[:, sl.M_BAD].tolist() == [1.0, 2.0, 2.0] and np.isfinite(out).all()


def _everything(mutant, m):
    """Every vector and record of the four kinds on inputs where each mistake shows; ``m`` rows."""
    x, b = sl.variables(5000), sl.rows(m)
    b["zl"][:2], b["zu"][:2] = 1e-30, 1e30          # (clamped from both sides, so swapped clamp bounds show)
    shared = mutant if mutant in sl._SHARED else None
    got = list(sl.emulate_reduce(b["lb"], b["ub"], b["g"], np.nan_to_num(b["s"]), b["lam"], np.nan_to_num(b["sigma_s"], nan=1.5),
                                 np.nan_to_num(b["rbar_s"]), mutant=mutant))
    got += sl.emulate_recover(x["lb"], x["ub"], b["lb"], b["ub"], b["dlam"], b["lam"], b["rbar_s"], b["s2"], b["sigma_s"], x["dx"], x["w"], x["s1"],
                              mutant=shared)
    upd = sl.emulate_update(b["lb"], b["ub"], b["v"], 100.0 * b["dv"], b["zl"], b["dzl"], b["zu"], b["dzu"], AP, AD, MU, 10.0, b["lam"], b["dlam"],
                            mutant=mutant)
    got += [a for a in upd if a is not None]
    if m < 10000:
        X, G, alphas = sl.trial_points(x, b, 2)
        got.append(sl.emulate_merit(x["lb"], x["ub"], b["lb"], b["ub"], X, G, b["s"], b["ds"], alphas, mutant=mutant))
    return got


_HONEST = {}


@pytest.mark.parametrize("mutant", sl.MUTANTS)
def test_every_deliberate_mistake_is_caught_by_the_bit_comparison(mutant):
    m = 600000 if mutant == "second_trip_dropped" else 2500      # (293 pieces: the scalar step's second strided trip)
    if m not in _HONEST:
        _HONEST[m] = _everything(None, m)
    got, want = _everything(mutant, m), _HONEST[m]
    assert len(got) == len(want)
    assert any(not sc.same_bits(np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)) for g, w in zip(got, want)), mutant
