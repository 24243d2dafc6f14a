"""A NumPy emulator of the whole MINRES solve of pockit_amd/csrc/pk_minres.cpp, bit for bit, and the synthetic KKT systems it is
tested on.  A plain helper module on top of tests/cg_cases.py and tests/sparse_cases.py, shared by
tests/test_minres_cases_cpu.py (which tests this module), tests/test_minres_cpu.py (the host stand-in's walk against it) and
tests/test_gpu_minres.py (the kernels against it).

The matrix is K = [[H + diag(s1), J^T], [J, -diag(s2)]] of size N = n + m on the structures of ``cg_cases.system``.  One
application runs in the unit's fixed order: q = (s1 o v1 | -(s2 o v2)) (or 0.0), q1 = H v1 + q1, q1 = J^T v2 + q1,
q2 = J v1 + q2, the products ``sparse_cases.emulate_operator`` (the association of pk_op_rows / pk_op_long).  A dot is
``cg_cases.dot`` (pieces of 2048, 8 strided terms per thread, the tree 128 ... 1, then one workgroup over the pieces).  Every
product is rounded before it is added (NumPy never fuses); sqrt and / are NumPy's, correctly rounded.  ``mutant`` names one
deliberate mistake each (MUTANTS): the CPU test requires every one of them to be caught.

Family "quasi": s1_i = sum_j |H_ij| + 1 + U(0, 0.5) (1 + U without H), so H + diag(s1) has its eigenvalues >= 1 by Gershgorin,
and s2 in U(0.05, 0.5): K is quasi-definite, its eigenvalues lie outside (-LAMBDA_QUASI, 1), and
max|x - x*| <= |K^-1 r|_2 <= |b - K x|_2 / LAMBDA_QUASI.  Family "eq": the same s1, s2 = None (pure equality constraints)."""
import functools

import numpy as np
import scipy.sparse

import cg_cases as cg
import sparse_cases as sc

(STATUS, ITERS, PHIBAR, THR, BETA, OLDB, ALFA, DBAR, EPSLN, CS, SN, PHI, OLDEPS, DELTA, GAMMA, FRESH) = range(16)
INIT, LANCZOS, ALFA_STEP, UPDATE, SOLUTION, DIAG, RECIP = range(7)      # the steps of pk_minres_step_dev
MUTANTS = ("fma_x", "s2_sign_dropped", "split_off_by_one", "r1_term_on_first_iteration", "converging_update_skipped",
           "frozen_moves_w", "cs_sn_swapped", "hypot_gamma", "tree_stops_at_2", "strided_first_trip")
LAMBDA_QUASI = 0.05
F = np.float64


def dot(terms, mutant=None):
    return cg.dot(terms, mutant if mutant in ("tree_stops_at_2", "strided_first_trip") else None)


# ---------------------------------------------------------------- the vector steps on plain arrays and a record of 16 doubles
def diag_terms(v, s1, s2, split, mutant=None):
    """Step 1 of one application: s1 o v below the split index, -(s2 o v) from it on; 0.0 where the vector is None."""
    if mutant == "split_off_by_one":
        split = min(split + 1, len(v))
    q = np.zeros(len(v))
    if s1 is not None:
        k = min(split, len(s1))
        q[:k] = s1[:k] * v[:k]
        if split > k:                                    # (the mutant reads one value of s1 that is not there: the first of s2's)
            q[k:split] = (s2[0] if s2 is not None else 0.0) * v[k:split]
    if s2 is not None:
        p = s2[: len(v) - split] * v[split:]
        q[split:] = p if mutant == "s2_sign_dropped" else -p
    return q


def step_init(b, x0, kx, minv, tol, mutant=None):
    """begin: (x, r1, r2, y, w, w2, rec).  ``kx`` = K x0 (ignored without x0)."""
    b = np.asarray(b, dtype=F)
    x = np.zeros(len(b)) if x0 is None else np.array(x0, dtype=F)
    r1 = b.copy() if x0 is None else b - kx
    y = r1.copy() if minv is None else minv * r1
    mb = b if minv is None else minv * b
    bmb, ry = F(dot(b * mb, mutant)), F(dot(r1 * y, mutant))
    rec = np.zeros(16)
    with np.errstate(all="ignore"):
        thr = F(tol) * np.sqrt(bmb)
        beta = F(0.0)
        if not np.isfinite(ry):
            status = 3.0
        elif ry < 0.0:
            status = 2.0
        else:
            beta = np.sqrt(ry)
            status = 1.0 if beta <= thr else 0.0
    rec[STATUS], rec[PHIBAR], rec[THR], rec[BETA], rec[CS] = status, beta, thr, beta, -1.0
    return x, r1, r1.copy(), y, np.zeros(len(b)), np.zeros(len(b)), rec


def step_lanczos(y, v, s1, s2, split, rec, mutant=None):
    """(v, q): v = (1 / beta) y only while the status is 0; q = the diagonal blocks' terms of v always."""
    if rec[STATUS] == 0.0:
        with np.errstate(all="ignore"):
            v = (F(1.0) / F(rec[BETA])) * y
    else:
        v = v.copy()
    with np.errstate(all="ignore"):
        return v, diag_terms(v, s1, s2, split, mutant)


def step_alfa(v, q, rec, mutant=None):
    """alfa = v.q and scalar step A, on a copy of the record."""
    rec = rec.copy()
    rec[FRESH] = 0.0
    if rec[STATUS] != 0.0:
        return rec
    with np.errstate(all="ignore"):
        alfa = dot(v * q, mutant)
    rec[ALFA] = alfa
    if not np.isfinite(alfa):
        rec[STATUS] = 3.0
    return rec


def scalar_b(rec, bsq, mutant=None):
    """Scalar step B on a copy of a running record."""
    rec = rec.copy()
    bsq = F(bsq)
    if not np.isfinite(bsq):
        rec[STATUS] = 3.0
        return rec
    if bsq < 0.0:
        rec[STATUS] = 2.0
        return rec
    cs, sn, dbar, alfa, phibar = (F(rec[k]) for k in (CS, SN, DBAR, ALFA, PHIBAR))
    if mutant == "cs_sn_swapped":
        cs, sn = sn, cs
    with np.errstate(all="ignore"):
        beta = np.sqrt(bsq)
        rec[OLDB], rec[BETA], rec[OLDEPS] = rec[BETA], beta, rec[EPSLN]
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        rec[DELTA], rec[EPSLN], rec[DBAR] = delta, sn * beta, -(cs * beta)
        gamma = F(np.hypot(gbar, beta)) if mutant == "hypot_gamma" else np.sqrt(gbar * gbar + beta * beta)
        rec[GAMMA] = gamma
        if not gamma > 0.0 or not np.isfinite(gamma):
            rec[STATUS] = 3.0
            return rec
        cs1, sn1 = gbar / gamma, beta / gamma
        rec[CS], rec[SN], rec[PHI], rec[PHIBAR] = cs1, sn1, cs1 * phibar, sn1 * phibar
    rec[ITERS] += 1.0
    rec[FRESH] = 1.0
    if rec[PHIBAR] <= rec[THR]:
        rec[STATUS] = 1.0
    return rec


def step_update(r1, r2, y, q, minv, rec, mutant=None):
    """The update and scalar step B: (r1, r2, y, rec), the inputs untouched."""
    if rec[STATUS] != 0.0:
        return r1.copy(), r2.copy(), y.copy(), rec.copy()
    with np.errstate(all="ignore"):
        t = q.copy()
        if rec[ITERS] >= 1.0 or mutant == "r1_term_on_first_iteration":
            t = t - (F(rec[BETA]) / F(rec[OLDB])) * r1
        t = t - (F(rec[ALFA]) / F(rec[BETA])) * r2
        y = t.copy() if minv is None else minv * t
        bsq = dot(t * y, mutant)
    return r2.copy(), t, y, scalar_b(rec, bsq, mutant)


def step_solution(x, v, w, w2, rec, mutant=None):
    """(x, w, w2): the solution update, exactly when the record's slot 15 is 1."""
    due = rec[FRESH] == 1.0 and not (mutant == "converging_update_skipped" and rec[STATUS] != 0.0)
    if not due and not (mutant == "frozen_moves_w" and rec[STATUS] != 0.0):
        return x.copy(), w.copy(), w2.copy()
    with np.errstate(all="ignore"):
        wn = ((v - F(rec[OLDEPS]) * w2) - F(rec[DELTA]) * w) / F(rec[GAMMA])
        if not due:
            return x.copy(), wn, w.copy()
        phi = np.full(len(x), rec[PHI])
        xn = cg._fma(phi, wn, x) if mutant == "fma_x" else x + phi * wn
    return xn, wn, w.copy()


def step_recip(g, s):
    """recip |g + s|: g None is 0.0, s None no term; 1.0 where the denominator is zero or not finite."""
    if g is None and s is None:
        raise ValueError("a length is needed")
    a = np.abs((np.zeros(len(s)) if g is None else g) + s) if s is not None else np.abs(g)
    good = (a > 0) & np.isfinite(a)
    return np.where(good, 1.0 / np.where(good, a, 1.0), 1.0)


# ---------------------------------------------------------------- synthetic KKT systems
class Kkt:
    """The augmented system on one ``cg_cases.System``: per (family, with_h) the inputs of a solve, K and its preconditioner
    as the device computes them."""

    def __init__(self, sy):
        self.sy, self.n, self.m, self.N = sy, sy.n, sy.m, sy.n + sy.m

    def inputs(self, family, with_h):
        """dict(with_h, s1, s2, b, x0, K): K the scipy matrix of the same numbers."""
        sy, n, m = self.sy, self.n, self.m
        rng = np.random.default_rng(sy.rng_seed + 100 + (0 if family == "quasi" else 10) + (1 if with_h else 0))
        b, x0 = cg._full(rng, n + m), cg._full(rng, n + m)
        s1 = (np.asarray(abs(sy.Hm).sum(axis=1)).reshape(-1) if with_h else np.zeros(n)) + 1.0 + cg._full(rng, n, 0.0, 0.5)
        s2 = cg._full(rng, m, 0.05, 0.5) if family == "quasi" else None
        top = scipy.sparse.diags_array(s1)
        if with_h:
            top = top + sy.Hm
        low = scipy.sparse.csr_array((m, m)) if s2 is None else scipy.sparse.diags_array(-s2)
        K = scipy.sparse.block_array([[top, sy.Jm.T], [sy.Jm, low]])
        return dict(with_h=bool(with_h), s1=s1, s2=s2, b=b, x0=x0, K=scipy.sparse.csc_array(K))

    def products(self, with_h, v, q):
        """Steps 2 ... 4 of one application: q already holds the diagonal blocks' terms."""
        sy, n = self.sy, self.n
        q1, q2 = q[:n], q[n:]
        if with_h:
            q1 = cg.apply_structure(sy.H, sy.hvals, v[:n], q1)
        q1 = cg.apply_structure(sy.JT, sy.jvals, v[n:], q1)
        q2 = cg.apply_structure(sy.J, sy.jvals, v[:n], q2)
        return np.concatenate((q1, q2))

    def kv(self, with_h, s1, s2, v, mutant=None):
        return self.products(with_h, v, diag_terms(v, s1, s2, self.n, mutant))

    def precond(self, with_h, s1, s2):
        """The diagonal preconditioner of pk_solve_kkt's precond 1."""
        sy = self.sy
        g1 = sy.hvals[sy.diag_pos] if with_h else None
        minv1 = np.ones(self.n) if (g1 is None and s1 is None) else step_recip(g1, s1)
        minv2 = step_recip(cg.sq_sum(sy.J, sy.jvals, minv1), s2)
        return np.concatenate((minv1, minv2))


@functools.lru_cache(maxsize=None)
def kkt(ctx):
    return Kkt(cg.system(ctx))


def emulate_solve(kk, with_h, s1, s2, minv, b, x0, tol, maxiter, check_every=8, mutant=None, full=False):
    """(x, rec) as pk_solve_kkt returns them: chunks of min(check_every, remaining) iterations, the iterations behind the stop
    enqueued and frozen; exhaustion is status 4 and slot 15 is 0 in the returned record.  ``full``: also the dict of the
    vectors x, r1, r2, y, w, w2 behind the last enqueued iteration."""
    assert mutant is None or mutant in MUTANTS
    kx = None if x0 is None else kk.kv(with_h, s1, s2, x0, mutant)
    x, r1, r2, y, w, w2, rec = step_init(b, x0, kx, minv, tol, mutant)
    v = np.zeros(len(x))
    done = 0
    while rec[STATUS] == 0.0 and done < maxiter:
        chunk = min(check_every, maxiter - done)
        for _ in range(chunk):
            v, q = step_lanczos(y, v, s1, s2, kk.n, rec, mutant)
            if rec[STATUS] == 0.0:              # (behind the stop q is scratch nobody reads)
                q = kk.products(with_h, v, q)
            rec = step_alfa(v, q, rec, mutant)
            r1, r2, y, rec = step_update(r1, r2, y, q, minv, rec, mutant)
            x, w, w2 = step_solution(x, v, w, w2, rec, mutant)
        done += chunk
    rec = rec.copy()
    rec[FRESH] = 0.0
    if rec[STATUS] == 0.0:
        rec[STATUS] = 4.0
    if full:
        return x, rec, dict(x=x, r1=r1, r2=r2, y=y, w=w, w2=w2)
    return x, rec


# ---------------------------------------------------------------- the cases of the synthetic solves, and what bounds them
# (context, family, with_h): B "eq" is no test input -- the synthetic J is numerically rank-deficient there
SYSTEMS = [("A", "quasi", True), ("A", "quasi", False), ("A", "eq", True), ("A", "eq", False), ("B", "quasi", True), ("B", "quasi", False)]


def m_norm(r, minv):
    return float(np.sqrt(np.dot(r, r if minv is None else minv * r)))


def residual_bound_2norm(tol, b, minv, factor=2.0):
    """|b - K x|_2 of a solve whose M-norm residual is held to ``factor tol |b|_M``: |r|_2 <= |r|_M / sqrt(min minv)."""
    return factor * tol * m_norm(b, minv) / (1.0 if minv is None else float(np.sqrt(minv.min())))


# ---------------------------------------------------------------- inputs of the vector-step tests
def split_points(length):
    """The split indices 0, 1, 255, 256, 257, N - 1, N that fit a length."""
    return sorted({s for s in (0, 1, 255, 256, 257, length - 1, length) if 0 <= s <= length})


def step_vectors(length, seed=7):
    """Full-mantissa vectors b, x0, kx, minv, s1, s2, x, r1, r2, y, v, w, w2, q of one length (s1 and s2 of the whole length:
    a step reads s1 below the split index and s2 from its start)."""
    rng = np.random.default_rng(seed + length)
    names = ("b", "x0", "kx", "minv", "s1", "s2", "x", "r1", "r2", "y", "v", "w", "w2", "q")
    vec = {k: cg._full(rng, length) for k in names}
    vec["minv"] = np.abs(vec["minv"]) + 0.25
    return vec


def running_record(rng, iterations=3.0):
    """A running record of full-mantissa scalars (status 0) as an iteration past the first might find it."""
    rec = np.zeros(16)
    c = rng.uniform(-1.0, 1.0)
    rec[ITERS], rec[PHIBAR], rec[THR] = iterations, rng.uniform(0.5, 2.0), 1e-30
    rec[BETA], rec[OLDB], rec[ALFA], rec[DBAR], rec[EPSLN] = rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0), rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-1, 1)
    rec[CS], rec[SN] = c, np.sqrt(1.0 - c * c)
    rec[PHI], rec[OLDEPS], rec[DELTA], rec[GAMMA] = rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-2, 2), rng.uniform(0.5, 2.0)
    return rec
