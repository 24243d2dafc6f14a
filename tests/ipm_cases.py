"""A NumPy emulator of the three vector kernels and the scalar step of pockit_amd/csrc/pk_ipm.cpp, bit for bit, and the boxed
vectors it is tested on.  A plain helper module on the conventions of tests/cg_cases.py (pieces of 2048, 8 elements per thread,
the fixed tree, the strided scalar step), shared by tests/test_ipm_cases_cpu.py (which tests this module), tests/test_ipm_cpu.py
(the host stand-in's walk against it) and tests/test_gpu_ipm.py (the kernels against it).

A column of a record is reduced as the unit's header states it: index i belongs to piece i / 2048; thread t folds the sides of
piece * 2048 + t + 256 j, j = 0 ... 7, ascending, within an element the lower side before the upper, into the column's identity;
the tree of widths 128 ... 1; then one workgroup whose thread t folds the pieces t, t + 256, ... ascending into the identity, and
the same tree.  A side that is absent or bad enters as the identity, which is bit for bit what skipping it gives (no partial sum
here can be -0.0).  Every product and quotient is rounded before it is added (NumPy never fuses).  ``log`` is a parameter: the
device's is not NumPy's.  ``mutant`` names one deliberate mistake each (MUTANTS): the CPU test requires every one to be caught."""
from fractions import Fraction

import numpy as np

import cg_cases as cg

# The association is cg_cases.dot's with the step as a parameter: that function adds one layer of terms
# and nothing else, and this unit needs max, min, the (quotient, index) pair and two sides per element, so the walk is restated
# here with an ``op``; tests/test_ipm_cases_cpu.py holds ``reduce_column([a], "sum")`` to ``cg_cases.dot(a)`` bit for bit, with and
# without the two mistakes the modules share, so the two statements cannot drift apart unnoticed.
BLOCK, PIECE = cg.BLOCK, cg.PIECE
TERMS, RESID, STEP = 0, 1, 2
COMPL_INF, COMPL_SUM, SIDES, MIN_SLACK, LOG_SUM, BAD, Z_SUM, MIN_COMPL = range(8)
R_INF, R_SQ, R_BAD = 0, 1, 2
ALPHA_PRI, ALPHA_DUAL, ARG_PRI, STEP_BAD = range(4)
MUTANTS = ("fma_dz", "upper_sign", "fixed_takes_part", "absent_times_zero", "tau_after_quotient", "tree_stops_at_2",
           "second_trip_dropped", "arg_largest", "upper_before_lower")
INF = np.inf

_OPS = {"sum": (np.add, 0.0), "max": (np.maximum, 0.0), "min": (np.minimum, INF), "min1": (np.minimum, 1.0)}


def _threads(a, identity):
    """(n_pieces, 8, 256): element piece * 2048 + t + 256 j at [piece, j, t], the identity beyond the length."""
    n_pieces = max(1, -(-len(a) // PIECE))
    full = np.full(n_pieces * PIECE, identity, dtype=np.float64)
    full[: len(a)] = a
    return full.reshape(n_pieces, 8, BLOCK)


def _tree(a, op, mutant):
    w = BLOCK // 2
    while w >= (2 if mutant == "tree_stops_at_2" else 1):
        a[:, :w] = op(a[:, :w], a[:, w: 2 * w])
        w //= 2
    return a[:, 0].copy()


def _trips(partial, identity, mutant):
    trips = -(-len(partial) // BLOCK)
    padded = np.full(trips * BLOCK, identity)
    padded[: len(partial)] = partial
    padded = padded.reshape(trips, BLOCK)
    return padded[:1] if mutant == "second_trip_dropped" else padded


def reduce_column(layers, kind, mutant=None):
    """One column from its per-side terms ``layers`` (arrays of one length, in the order a thread folds them within an
    element), ``kind`` one of "sum", "max", "min", "min1" (a min that starts from 1.0)."""
    op, identity = _OPS[kind]
    if mutant == "upper_before_lower":
        layers = layers[::-1]
    cubes = [_threads(a, identity) for a in layers]
    acc = np.full((cubes[0].shape[0], BLOCK), identity)
    for j in range(8):
        for c in cubes:
            acc = op(acc, c[:, j, :])
    rows = _trips(_tree(acc, op, mutant), identity, mutant)
    acc = np.full((1, BLOCK), identity)
    for row in rows:
        acc = op(acc, row)
    return float(_tree(acc, op, mutant)[0])


def _pair(qa, ia, qb, ib, mutant):
    take = (qb < qa) | ((qb == qa) & ((ib > ia) if mutant == "arg_largest" else (ib < ia)))
    return np.where(take, qb, qa), np.where(take, ib, ia)


def _pair_tree(q, i, mutant):
    w = BLOCK // 2
    while w >= (2 if mutant == "tree_stops_at_2" else 1):
        q[:, :w], i[:, :w] = _pair(q[:, :w], i[:, :w], q[:, w: 2 * w], i[:, w: 2 * w], mutant)
        w //= 2
    return q[:, 0].copy(), i[:, 0].copy()


def reduce_pair(layers, mutant=None):
    """(alpha, index): the lexicographic min of the (quotient, index) pairs ``layers`` from (1.0, +inf) -- the smaller
    quotient, among equal quotients the smaller index."""
    if mutant == "upper_before_lower":
        layers = layers[::-1]
    none = -INF if mutant == "arg_largest" else INF
    cubes = [(_threads(q, 1.0), _threads(i, none)) for q, i in layers]
    n_pieces = cubes[0][0].shape[0]
    q, i = np.full((n_pieces, BLOCK), 1.0), np.full((n_pieces, BLOCK), none)
    for j in range(8):
        for cq, ci in cubes:
            q, i = _pair(q, i, cq[:, j, :], ci[:, j, :], mutant)
    pq, pi = _pair_tree(q, i, mutant)
    rq, ri = _trips(pq, 1.0, mutant), _trips(pi, none, mutant)
    q, i = np.full((1, BLOCK), 1.0), np.full((1, BLOCK), none)
    for a, b in zip(rq, ri):
        q, i = _pair(q, i, a, b, mutant)
    q, i = _pair_tree(q, i, mutant)
    return float(q[0]), float(i[0])


# ---------------------------------------------------------------- the sides of a boxed vector
def sides(lb, ub, mutant=None):
    """(lower present, upper present): none for a fixed element."""
    boxed = np.ones(len(lb), dtype=bool) if mutant == "fixed_takes_part" else lb != ub
    return boxed & np.isfinite(lb), boxed & np.isfinite(ub)


def _side(present, slack, z):
    """(good, slack, z) with 1.0 in place of whatever a side that is absent or bad holds."""
    slack, z = np.where(present, slack, 1.0), np.where(present, z, 1.0)
    good = present & (slack > 0) & np.isfinite(slack) & (z >= 0) & np.isfinite(z)
    return good, np.where(good, slack, 1.0), np.where(good, z, 1.0)


def _fms(a, b, c, sign):
    """c - a * b (sign -1) or c + a * b (sign +1) with ONE rounding: the mistake of the 'fma_dz' mutant."""
    return np.array([float(Fraction(z) + sign * Fraction(x) * Fraction(y)) if np.isfinite(x) and np.isfinite(y) and np.isfinite(z) else z + sign * x * y
                     for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())])


def emulate_terms(lb, ub, v, zl, zu, mu, log=np.log, mutant=None):
    """(sigma, rbar, record of 8) as pk_ip_terms_k and pk_ip_scalar_k leave them."""
    assert mutant is None or mutant in MUTANTS
    with np.errstate(all="ignore"):
        lo, up = sides(lb, ub, mutant)
        okl, dl, sl = _side(lo, v - lb, zl)
        oku, du, su = _side(up, ub - v, zu)
        if mutant == "absent_times_zero":
            sigma = lo * (zl / (v - lb)) + up * (zu / (ub - v))
            rbar = lo * (mu / (v - lb)) - up * (mu / (ub - v))
        else:
            ql, qu = np.where(okl, sl / dl, 0.0), np.where(oku, su / du, 0.0)
            ml, mu_u = np.where(okl, mu / dl, 0.0), np.where(oku, mu / du, 0.0)
            sigma = np.where(lo & up, ql + qu, np.where(lo, ql, np.where(up, qu, 0.0)))
            rbar = np.where(lo & up, ml - mu_u, np.where(lo, ml, np.where(up & oku, -mu_u, 0.0)))
        cl, cu = dl * sl, du * su
        rec = np.zeros(8)
        both = lambda a, b, fill: [np.where(okl, a, fill), np.where(oku, b, fill)]  # noqa: E731
        rec[COMPL_INF] = reduce_column(both(np.abs(cl - mu), np.abs(cu - mu), 0.0), "max", mutant)
        rec[COMPL_SUM] = reduce_column(both(cl, cu, 0.0), "sum", mutant)
        rec[SIDES] = reduce_column(both(1.0, 1.0, 0.0), "sum", mutant)
        rec[MIN_SLACK] = reduce_column(both(dl, du, INF), "min", mutant)
        rec[LOG_SUM] = reduce_column(both(log(dl), log(du), 0.0), "sum", mutant)
        rec[BAD] = reduce_column([np.where(lo & ~okl, 1.0, 0.0), np.where(up & ~oku, 1.0, 0.0)], "sum", mutant)
        rec[Z_SUM] = reduce_column(both(sl, su, 0.0), "sum", mutant)
        rec[MIN_COMPL] = reduce_column(both(cl, cu, INF), "min", mutant)
    return sigma, rbar, rec


def emulate_residual(lb, ub, t, z=None, negate=False, mutant=None):
    """(r, record of 4) as pk_ip_resid_k and pk_ip_scalar_k leave them; ``t`` = J^T lam + grad."""
    assert mutant is None or mutant in MUTANTS
    with np.errstate(all="ignore"):
        boxed = np.ones(len(lb), dtype=bool) if mutant == "fixed_takes_part" else lb != ub
        r = t if z is None else t - z
        if negate:
            r = -r
        r = np.where(boxed, r, 0.0)
        fin = boxed & np.isfinite(r)
        safe = np.where(fin, r, 0.0)
        rec = np.zeros(4)
        rec[R_INF] = reduce_column([np.abs(safe)], "max", mutant)
        rec[R_SQ] = reduce_column([safe * safe], "sum", mutant)
        rec[R_BAD] = reduce_column([np.where(boxed & ~fin, 1.0, 0.0)], "sum", mutant)
    return r, rec


def emulate_step(lb, ub, v, dv, zl, zu, mu, tau, mutant=None):
    """(dzl, dzu, record of 4) as pk_ip_step_k and pk_ip_scalar_k leave them."""
    assert mutant is None or mutant in MUTANTS
    with np.errstate(all="ignore"):
        lo, up = sides(lb, ub, mutant)
        live = np.isfinite(np.where(lo | up, dv, 0.0))
        okl, dl, sl = _side(lo & live, v - lb, zl)
        oku, du, su = _side(up & live, ub - v, zu)
        d = np.where(lo | up, np.where(live, dv, 0.0), 0.0)
        bl, bu = mu / dl - sl, mu / du - su
        if mutant == "fma_dz":
            dzl, dzu = _fms(sl / dl, d, bl, -1), _fms(su / du, d, bu, +1)
        else:
            dzl, dzu = bl - (sl / dl) * d, (bu - (su / du) * d) if mutant == "upper_sign" else bu + (su / du) * d
        dzl, dzu = np.where(okl, dzl, 0.0), np.where(oku, dzu, 0.0)
        if mutant == "absent_times_zero":
            dzl, dzu = lo * ((mu / (v - lb) - zl) - (zl / (v - lb)) * dv), up * ((mu / (ub - v) - zu) + (zu / (ub - v)) * dv)

        def cand(mask, s, neg):
            neg = np.where(mask, neg, 1.0)
            q = tau * (s / neg) if mutant == "tau_after_quotient" else (tau * s) / neg
            return np.where(mask & (q < 1.0), q, 1.0), mask & (q < 1.0)

        idx = np.arange(len(lb), dtype=np.float64)
        none = -INF if mutant == "arg_largest" else INF
        ql, hl = cand(okl & (d < 0), dl, -d)
        qu, hu = cand(oku & (d > 0), du, d)
        apri, arg = reduce_pair([(ql, np.where(hl, idx, none)), (qu, np.where(hu, idx, none))], mutant)
        adual = reduce_column([cand(okl & (dzl < 0), sl, -dzl)[0], cand(oku & (dzu < 0), su, -dzu)[0]], "min1", mutant)
        bad = reduce_column([np.where((lo | up) & ~live, 1.0, 0.0), np.where(lo & live & ~okl, 1.0, 0.0), np.where(up & live & ~oku, 1.0, 0.0)],
                            "sum", mutant)
    return dzl, dzu, np.array([apri, adual, arg if apri < 1.0 else -1.0, bad])


# ---------------------------------------------------------------- boxed vectors
LENGTHS = (1, 255, 256, 257, 2047, 2048, 2049, 524289)
LENGTH_PAST_THE_PIECE_CAP = 4194305      # 2049 pieces: past PK_LIB_GRID_CAP, the stride loop of a workgroup runs
BOTH, LOWER, UPPER, FREE, FIXED = range(5)


def boxed(length, seed=7, kinds=None):
    """A clean boxed vector of full-mantissa doubles: dict(lb, ub, v, dv, zl, zu, t, z, kind).  Elements mix two-sided,
    one-sided, free and fixed bounds; v lies strictly inside, multipliers in (0.1, 1); whatever a kernel must not read is NaN:
    the multiplier of an absent side, and v and dv of an element without a side."""
    rng = np.random.default_rng(seed + length)
    kind = rng.choice(5, size=length, p=(0.4, 0.2, 0.2, 0.1, 0.1)) if kinds is None else np.broadcast_to(np.asarray(kinds), (length,)).copy()
    base, width = rng.uniform(-2.0, 1.0, length), rng.uniform(0.5, 3.0, length)
    lb = np.where((kind == BOTH) | (kind == LOWER) | (kind == FIXED), base, -INF)
    ub = np.where(kind == BOTH, base + width, np.where(kind == UPPER, base, np.where(kind == FIXED, base, INF)))
    inside = rng.uniform(0.05, 0.95, length)
    v = np.where(kind == BOTH, base + width * inside, np.where(kind == LOWER, base + 2.0 * inside + 0.1, np.where(kind == UPPER, base - 2.0 * inside - 0.1, np.nan)))
    has_l, has_u = (kind == BOTH) | (kind == LOWER), (kind == BOTH) | (kind == UPPER)
    zl = np.where(has_l, rng.uniform(0.1, 1.0, length), np.nan)
    zu = np.where(has_u, rng.uniform(0.1, 1.0, length), np.nan)
    dv = np.where(has_l | has_u, rng.standard_normal(length), np.nan)
    return dict(lb=lb, ub=ub, v=v, dv=dv, zl=zl, zu=zu, t=rng.uniform(-1.0, 1.0, length), z=rng.uniform(-1.0, 1.0, length), kind=kind)


def inside(lo, hi, start):
    """``start`` moved strictly inside [lo, hi]: a tenth of the width (at most 0.1) off every finite bound; a fixed element
    stays on its bound.  For the bounds of a model (tests/test_gpu_ipm.py, tools/ipm_probe.py)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        margin = np.where(np.isfinite(hi - lo), np.minimum(0.1, 0.1 * (hi - lo)), 0.1)
    return np.where(lo == hi, lo, np.minimum(np.maximum(start, lo + margin), hi - margin))


PLANTED = {"zero_slack": 0, "negative_multiplier": 1, "inf_multiplier": 2, "nan_multiplier": 3, "nan_step": 4}


def dirty(length, seed=7):
    """``boxed`` with elements 0 ... 4 two-sided and one defect each (PLANTED): a zero lower slack, a negative zl, an infinite
    zu, a NaN zl, a NaN dv (the step alone reads it; the residual's t is NaN there too).  ``length`` >= 5."""
    assert length >= 5
    b = boxed(length, seed)
    for k in range(5):
        b["kind"][k] = BOTH
        b["lb"][k], b["ub"][k], b["v"][k], b["dv"][k], b["zl"][k], b["zu"][k] = -1.0, 2.0, 0.25 + 0.125 * k, -0.5, 0.5, 0.75
    b["v"][0] = -1.0
    b["zl"][1] = -0.5
    b["zu"][2] = INF
    b["zl"][3] = np.nan
    b["dv"][4] = np.nan
    b["t"][4] = np.nan
    return b


def log_bound(lb, ub, v, zl, zu, length):
    """The bound tests/test_gpu_ipm.py and tests/test_ipm_cpu.py hold column 4 to between two implementations of log: one ulp
    per term on each side plus both sides' tree rounding, (2 * 2^-52 + ceil(log2 L + 1) * 2^-52) * sum |ln term| over the
    good sides."""
    with np.errstate(all="ignore"):
        lo, up = sides(lb, ub)
        okl, dl, _ = _side(lo, v - lb, zl)
        oku, du, _ = _side(up, ub - v, zu)
        total = float(np.sum(np.abs(np.log(dl[okl]))) + np.sum(np.abs(np.log(du[oku]))))
    return (2.0 + np.ceil(np.log2(max(length, 1)) + 1.0)) * 2.0 ** -52 * total
