"""A NumPy emulator of the four vector kernels and the scalar step of pockit_amd/csrc/pk_slack.cpp, bit for bit, and the vectors
it is tested on.  A plain helper module on top of tests/ipm_cases.py and tests/cg_cases.py (pieces of 2048, 8 elements per
thread, the fixed tree, the strided scalar step), shared by tests/test_slack_cases_cpu.py (which tests this module),
tests/test_slack_cpu.py (the host stand-in's walk against it) and tests/test_gpu_slack.py (the kernels against it).

The association is the unit's header's.  ``reduce`` and ``update`` walk one index range, which is ``ipm_cases.reduce_column``.
``recover`` and ``merit`` walk two: the variables' pieces first, the rows' pieces behind them, a piece wholly in one range, then
one scalar step over all pieces (``two_ranges``); a range of length 0 has no piece, and without any piece one piece of
identities stands.  An absent or bad term enters as the identity, which is bit for bit what skipping it gives.  Every product
and quotient is rounded before it is added (NumPy never fuses).  ``log`` is a parameter: the device's is not NumPy's.
``mutant`` names one deliberate mistake each (MUTANTS): the CPU test requires every one to be caught."""
import numpy as np

import ipm_cases as ip

BLOCK, PIECE, INF = ip.BLOCK, ip.PIECE, np.inf
REDUCE, RECOVER, UPDATE, MERIT = range(4)
THETA_INF, THETA_1, RED_BAD, RED_ROWS = range(4)
CURV_X, CURV_S, DX_SQ, DS_SQ, REC_BAD = range(5)
CLAMPED, MIN_SLACK, UPD_BAD = range(3)
M_THETA_1, M_THETA_INF, M_LOG, M_BAD = range(4)
MUTANTS = ("fused_s2", "equality_gets_slack", "safeguard_old_slack", "clamp_swapped", "upper_sign", "absent_written",
           "alpha_d_for_v", "tree_stops_at_2", "second_trip_dropped")
_SHARED = {"tree_stops_at_2", "second_trip_dropped"}      # (the two the association itself can make: ipm_cases' names)


def _assoc(mutant):
    return mutant if mutant in _SHARED else None


def one_range(layers, kind, mutant=None):
    return ip.reduce_column([np.asarray(a, dtype=np.float64) for a in layers], kind, _assoc(mutant))


def _pieces(layers, kind, mutant):
    """The partial of every piece of one range: thread t folds its elements' layers in order, then the tree."""
    op, identity = ip._OPS[kind]
    if len(layers[0]) == 0:
        return np.zeros(0)
    cubes = [ip._threads(np.asarray(a, dtype=np.float64), identity) for a in layers]
    acc = np.full((cubes[0].shape[0], BLOCK), identity)
    for j in range(8):
        for c in cubes:
            acc = op(acc, c[:, j, :])
    return ip._tree(acc, op, _assoc(mutant))


def two_ranges(x_layers, r_layers, kind, mutant=None):
    """One column over the variables' pieces and the rows' pieces behind them."""
    op, identity = ip._OPS[kind]
    partial = np.concatenate((_pieces(x_layers, kind, mutant), _pieces(r_layers, kind, mutant)))
    if len(partial) == 0:
        partial = np.full(1, identity)
    acc = np.full((1, BLOCK), identity)
    for row in ip._trips(partial, identity, _assoc(mutant)):
        acc = op(acc, row)
    return float(ip._tree(acc, op, _assoc(mutant))[0])


def _positive(a):
    return (a > 0) & np.isfinite(a)


def emulate_reduce(clb, cub, g, s, lam, sigma_s, rbar_s, mutant=None):
    """(s2, b2, record of 4) as pk_sl_reduce_k and pk_sl_scalar_k leave them."""
    assert mutant is None or mutant in MUTANTS
    with np.errstate(all="ignore"):
        eq = np.zeros(len(clb), dtype=bool) if mutant == "equality_gets_slack" else clb == cub
        ok = ~eq & _positive(sigma_s)
        r = np.where(eq, g - clb, np.where(ok, g - s, 0.0))
        s2 = np.where(ok, 1.0 / np.where(ok, sigma_s, 1.0), 0.0)
        z = np.where(ok, lam + rbar_s, 0.0)
        inner = ip._fms(s2, z, -r, +1) if mutant == "fused_s2" else (-r) + s2 * z
        b2 = np.where(eq, -r, np.where(ok, inner, 0.0))
        good = (eq | ok) & np.isfinite(r)
        ar = np.where(good, np.abs(r), 0.0)
        rec = np.array([one_range([ar], "max", mutant), one_range([ar], "sum", mutant), one_range([np.where(good, 0.0, 1.0)], "sum", mutant),
                        one_range([np.where(eq, 0.0, 1.0)], "sum", mutant)])
    return s2, b2, rec


def emulate_recover(xlb, xub, clb, cub, dlam, lam, rbar_s, s2, sigma_s, dx, w, s1, mutant=None):
    """(ds, record of 5) as pk_sl_recover_k and pk_sl_scalar_k leave them."""
    assert mutant is None or mutant in MUTANTS
    n, m = len(xlb), len(clb)
    with np.errstate(all="ignore"):
        free = xlb != xub
        sq_x = dx * dx
        term = dx * w + s1 * sq_x
        okx = free & np.isfinite(term)
        eq = np.zeros(m, dtype=bool) if mutant == "equality_gets_slack" else clb == cub
        sig_ok = ~eq & _positive(sigma_s)
        raw = s2 * ((dlam + lam) + rbar_s)
        ds = np.where(sig_ok, raw, 0.0)
        okr = sig_ok & np.isfinite(raw)
        sq_s = ds * ds
        zx, zr = np.zeros(n), np.zeros(m)
        rec = np.array([
            two_ranges([np.where(okx, term, 0.0)], [zr], "sum", mutant),
            two_ranges([zx], [np.where(okr, sigma_s * sq_s, 0.0)], "sum", mutant),
            two_ranges([np.where(okx, sq_x, 0.0)], [zr], "sum", mutant),
            two_ranges([zx], [np.where(okr, sq_s, 0.0)], "sum", mutant),
            two_ranges([np.where(free & ~okx, 1.0, 0.0)], [np.where(~eq & ~okr, 1.0, 0.0)], "sum", mutant)])
    return ds, rec


def emulate_update(lb, ub, v, dv, zl, dzl, zu, dzu, alpha_p, alpha_d, mu, kappa, lam=None, dlam=None, mutant=None):
    """(v, zl, zu, lam or None, record of 4) as pk_sl_update_k and pk_sl_scalar_k leave them; the inputs are not modified."""
    assert mutant is None or mutant in MUTANTS
    with np.errstate(all="ignore"):
        boxed = lb != ub
        lo, up = boxed & np.isfinite(lb), boxed & np.isfinite(ub)
        vn = np.where(boxed, v + (alpha_d if mutant == "alpha_d_for_v" else alpha_p) * dv, v)
        fin = boxed & np.isfinite(vn)
        layers_bad = [np.where(boxed & ~fin, 1.0, 0.0)]
        lam_new = None
        if lam is not None:
            lam_new = lam + alpha_p * dlam
            layers_bad.insert(0, np.where(np.isfinite(lam_new), 0.0, 1.0))
        clamped, slack, out = [], [], []
        for upper, present, z, dz in ((False, lo, zl, dzl), (True, up, zu, dzu)):
            d_new = (vn - ub if mutant == "upper_sign" else ub - vn) if upper else vn - lb
            d_old = (ub - v) if upper else v - lb
            d = d_old if mutant == "safeguard_old_slack" else d_new
            zn = z + alpha_d * dz
            low, high = mu / (kappa * d), (kappa * mu) / d
            if mutant == "clamp_swapped":
                low, high = high, low
            ok = present & fin & _positive(d_new) & np.isfinite(zn)
            zc = np.where(ok, np.minimum(np.maximum(zn, low), high), zn)
            out.append(np.where(present, zc, np.where(boxed, 0.0, z) if mutant == "absent_written" else z))
            clamped.append(np.where(ok & (zc != zn), 1.0, 0.0))
            slack.append(np.where(ok, d_new, INF))
            layers_bad.append(np.where(present & fin & ~ok, 1.0, 0.0))
        rec = np.array([one_range(clamped, "sum", mutant), one_range(slack, "min", mutant), one_range(layers_bad, "sum", mutant), 0.0])
    return vn, out[0], out[1], lam_new, rec


def emulate_merit(xlb, xub, clb, cub, X, G, s, ds, alphas, log=np.log, mutant=None):
    """The (B, 4) table as pk_sl_merit_k and pk_sl_scalar_k leave it."""
    assert mutant is None or mutant in MUTANTS
    out = np.zeros((len(alphas), 4))
    with np.errstate(all="ignore"):
        xlo, xup = ip.sides(xlb, xub)
        eq = np.zeros(len(clb), dtype=bool) if mutant == "equality_gets_slack" else clb == cub
        rlo, rup = ~eq & np.isfinite(clb), ~eq & np.isfinite(cub)
        zx = np.zeros(len(xlb))

        def side(present, d):
            ok = present & _positive(d)
            return np.where(ok, log(np.where(ok, d, 1.0)), 0.0), np.where(present & ~ok, 1.0, 0.0)

        for b, alpha in enumerate(alphas):
            st = s + alpha * ds
            r = np.where(eq, G[b] - clb, G[b] - st)
            finr = np.isfinite(r)
            ar = np.where(finr, np.abs(r), 0.0)
            lxl, bxl = side(xlo, X[b] - xlb)
            lxu, bxu = side(xup, xub - X[b])
            lrl, brl = side(rlo, st - clb)
            lru, bru = side(rup, (st - cub) if mutant == "upper_sign" else cub - st)
            out[b] = (two_ranges([zx], [ar], "sum", mutant), two_ranges([zx], [ar], "max", mutant),
                      two_ranges([lxl, lxu], [lrl, lru], "sum", mutant),
                      two_ranges([bxl, bxu], [np.where(finr, 0.0, 1.0), brl, bru], "sum", mutant))
    return out


def merit_log_bound(xlb, xub, clb, cub, x, s_trial):
    """The bound the log_sum slot of one entry is held to between two implementations of log (DESIGN.md section 21's): one ulp
    per term on each side plus both sides' tree rounding, (2 * 2^-52 + ceil(log2 L + 1) * 2^-52) * sum |ln term| with L the
    walked length n + m."""
    with np.errstate(all="ignore"):
        xlo, xup = ip.sides(xlb, xub)
        rlo, rup = ip.sides(clb, cub)
        total = 0.0
        for present, d in ((xlo, x - xlb), (xup, xub - x), (rlo, s_trial - clb), (rup, cub - s_trial)):
            ok = present & _positive(d)
            total += float(np.sum(np.abs(np.log(d[ok]))))
    return (2.0 + np.ceil(np.log2(max(len(xlb) + len(clb), 1)) + 1.0)) * 2.0 ** -52 * total


# ---------------------------------------------------------------- the vectors
LENGTHS = ip.LENGTHS
LENGTH_PAST_THE_PIECE_CAP = ip.LENGTH_PAST_THE_PIECE_CAP
KAPPA = 1e10


def rows(m, seed=5, kinds=None):
    """Constraint rows with their slack quantities: ``ipm_cases.boxed`` read as rows (FIXED: an equality row) plus g, s, lam,
    dlam, sigma_s, rbar_s, s2, the slack step and the multiplier steps, full mantissa; NaN wherever a kernel must not read (s,
    sigma_s, rbar_s, s2 of an equality row beside ipm_cases' own)."""
    b = ip.boxed(m, seed, kinds)
    rng = np.random.default_rng(seed + 1000 + m)
    eq = b["lb"] == b["ub"]
    b["s"] = np.where(eq, np.nan, np.where(np.isnan(b["v"]), rng.standard_normal(m), b["v"]))       # (a free slack has a value too)
    b["g"] = np.where(eq, b["lb"], b["s"]) + rng.uniform(-0.5, 0.5, m)
    b["lam"], b["dlam"] = rng.standard_normal(m), rng.standard_normal(m)
    b["sigma_s"] = np.where(eq, np.nan, rng.uniform(0.01, 100.0, m))
    b["rbar_s"] = np.where(eq, np.nan, rng.standard_normal(m))
    b["s2"] = np.where(eq, np.nan, 1.0 / b["sigma_s"])
    b["ds"] = np.where(eq, np.nan, 0.002 * rng.standard_normal(m))
    b["dv"] = np.where(eq, np.nan, np.where(np.isnan(b["dv"]), rng.standard_normal(m), b["dv"]) * 0.002)
    b["v"] = b["s"]
    b["dzl"] = np.where(np.isnan(b["zl"]), np.nan, 0.05 * rng.standard_normal(m))
    b["dzu"] = np.where(np.isnan(b["zu"]), np.nan, 0.05 * rng.standard_normal(m))
    return b


def variables(n, seed=9, kinds=None):
    """Variables for the curvature terms and the trial points: ``ipm_cases.boxed`` plus dx, w, s1 (NaN on a fixed variable)."""
    b = ip.boxed(n, seed, kinds)
    rng = np.random.default_rng(seed + 2000 + n)
    fixed = b["lb"] == b["ub"]
    for name in ("dx", "w"):
        b[name] = np.where(fixed, np.nan, rng.standard_normal(n))
    b["s1"] = np.where(fixed, np.nan, rng.uniform(0.0, 3.0, n))
    return b


def trial_points(xv, rw, count, seed=3):
    """(X, G, alphas) of ``count`` trial points: X strictly inside the bounds where a side is present and NaN where an element
    has none, G near the slacks."""
    rng = np.random.default_rng(seed + count)
    alphas = 0.5 ** np.arange(count) * rng.uniform(0.9, 1.0)
    n, m = len(xv["lb"]), len(rw["lb"])
    X = np.tile(xv["v"], (count, 1)) * 1.0
    has = ~np.isnan(xv["v"])
    X[:, has] += 1e-3 * rng.standard_normal((count, int(has.sum())))
    eq = rw["lb"] == rw["ub"]
    G = np.where(eq, rw["lb"], np.nan_to_num(rw["s"])) + rng.uniform(-0.5, 0.5, (count, m))
    assert X.shape == (count, n)
    return X, G, alphas


def plant(x, b, X, G):
    """Defects into the vectors of ``variables`` / ``rows`` / ``trial_points`` (>= 12 rows, >= 4 variables, >= 3 trial points),
    in place.  Rows 0 ... 11 and variables 0 ... 3 become two-sided and clean first.  Then: sigma_s of rows 0, 1 is 0 and inf and
    g of row 2 NaN (reduce: 3 bad); w of variable 1 inf (recover: 3 bad with the two sigma_s); the slack step of row 3 NaN, the
    lower multiplier step of row 4 inf, the slack step of row 5 across its bound (update: 3 bad); G of row 6 inf and the merit's
    slack step of row 7 far across its bound in every entry, variable 2 of trial point 2 on its bound (merit: 2, 2, 3 bad)."""
    for k in range(12):
        b["kind"][k] = ip.BOTH
        b["lb"][k], b["ub"][k], b["s"][k], b["g"][k] = -1.0, 2.0, 0.25 + 0.125 * k, 0.3 + 0.1 * k
        b["sigma_s"][k], b["rbar_s"][k], b["ds"][k], b["dv"][k] = 1.5, 0.7, 0.002, 0.002
        b["zl"][k], b["zu"][k], b["dzl"][k], b["dzu"][k] = 0.5, 0.75, 0.01, -0.01
        b["s2"][k] = 1.0 / 1.5
        G[:, k] = b["g"][k]
    b["v"] = b["s"]
    for k in range(4):
        x["kind"][k] = ip.BOTH
        x["lb"][k], x["ub"][k], x["v"][k], x["dx"][k], x["w"][k], x["s1"][k] = -1.0, 2.0, 0.3, 0.5, -0.25, 1.25
        X[:, k] = 0.3
    b["sigma_s"][0], b["sigma_s"][1], b["g"][2] = 0.0, INF, np.nan
    x["w"][1] = INF
    b["dv"][3], b["dzl"][4], b["dv"][5] = np.nan, INF, 100.0
    G[:, 6], b["ds"][7], X[2, 2] = INF, 1e6, x["lb"][2]
