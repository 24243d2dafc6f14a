"""A NumPy emulator of the refinement of the band solve (pockit_amd/csrc/pk_band_refine.cpp: pk_bd_resid_k, pk_bd_refine_scalar_k,
pk_bd_correct_k around the family's solve), bit for bit, and the synthetic systems it is tested on.  A plain helper module on top
of tests/band_cases.py (``solve_system`` / ``emulate``: the solve with the factors in place) and tests/minres_cases.py
(``Kkt.kv``: one application of K in the unit's fixed order), shared by tests/test_band_refine_cases_cpu.py (which tests this
module), tests/test_band_refine_cpu.py (the host stand-in's walk against it) and tests/test_gpu_band_refine.py (the kernels).

``resid``: at an unknown (``where[i] >= 0``; ``where`` None: everywhere) ``r_i = b_i - q_i``, one rounding; the largest ``|r_i|``,
``|x_i|``, ``|b_i|`` over the unknowns at which all three are finite and the count of the others; ``r_i = 0.0`` elsewhere.  A
maximum and an exact count do not depend on the order in which pieces and threads are reduced, so none is stated here.
``scalar``: the record of 8 doubles and the decision behind step t.  ``correct``: ``x_i + d_i`` at the unknowns while the status is
0.  ``refine``: begin and any number of enqueued steps, with the freeze rule; ``refine_host``: the host form's loop.

The synthetic systems are those of ``band_cases.system`` with K = [[B, U], [U^T, C]] dense; their product ``q = K x`` is
``Dense.kx``: the products ``K_ij x_j`` rounded one by one and added to 0.0 in ascending j.  ``mutant`` names one deliberate
mistake each (MUTANTS): the CPU test requires every one to be caught."""
from fractions import Fraction

import numpy as np

import band_cases as bc
import cg_cases as cg
import minres_cases as mc

STATUS, STEPS, RNORM, XNORM, BNORM, RHO, RHO0, PREV = range(8)
RUNNING, CONVERGED, STALLED, NON_FINITE, BAND_FAILED, EXHAUSTED = (float(k) for k in range(6))
RESID, SCALAR, CORRECT = range(3)                  # the steps of pk_band_refine_step_dev
TOL, SINGULAR, MAX_STEPS = 1.0e-10, 1.0e-5, 10     # PK_BAND_REFINE_TOL, PK_BAND_REFINE_SINGULAR, PK_BAND_REFINE_MAX_STEPS
IMPROVE, XCAP = 1.0 - 1.0e-9, 1.0e6                # PK_BR_IMPROVE, PK_BR_XCAP
MUTANTS = ("fused_residual", "non_finite_in_maxima", "fixed_in_norms", "stall_before_convergence", "correct_behind_stop",
           "no_min_in_ratio")
LENGTHS = (1, 2, 255, 256, 257, 2047, 2048, 2049)  # around the workgroup and the piece
BEYOND_GRID = 524289                               # one element beyond 2048 work items of 256: the correction's stride loop
F = np.float64
# the five systems of the CPU and GPU tests: (nb, w, p, seed, variant), the squeezed (j, factor) or None, and what is asserted:
# the final status, the corrections, and whether rho_0 is already below the tolerance
TABLE = (
    ((65, 7, 3, 1, "plain"), None, CONVERGED, 0),
    ((65, 7, 3, 1, "plain"), (32, 2.0 ** -30), CONVERGED, 1),
    ((101, 20, 8, 2, "plain"), (50, 2.0 ** -24), CONVERGED, 1),
    ((40, 7, 1, 3, "tiny_diagonal"), None, CONVERGED, 1),
    ((65, 7, 3, 1, "tiny_diagonal"), None, STALLED, None),
)


# ---------------------------------------------------------------- the three kernels
def unknowns(length, where):
    return np.ones(length, dtype=bool) if where is None else np.asarray(where) >= 0


def resid(b, q, x, where=None, mutant=None, fused=None):
    """``(r, sums)``: sums = (max |r|, max |x|, max |b|, non-finite count).  ``fused``: with the mutant "fused_residual" the pair
    ``(q_before, last)`` of ``Dense.kx_parts`` -- the last product is subtracted together with the sum in one rounding."""
    b, q, x = (np.asarray(a, dtype=F) for a in (b, q, x))
    u = unknowns(len(b), where)
    if mutant == "fixed_in_norms":
        u = np.ones(len(b), dtype=bool)
    with np.errstate(all="ignore"):
        if mutant == "fused_residual" and fused is not None:
            full = np.array([float(Fraction(bi) - Fraction(a) - Fraction(c)) if np.isfinite([bi, a, c]).all() else bi - (a + c)
                             for bi, a, c in zip(b.tolist(), fused[0].tolist(), fused[1].tolist())])
        else:
            full = b - q
    r = np.where(u, full, 0.0)
    fin = np.isfinite(r) & np.isfinite(x) & np.isfinite(b)
    keep = u & fin
    if mutant == "non_finite_in_maxima":      # (an infinity enters; a NaN loses every comparison as it would in the kernel)
        keep = u
    sums = []
    for a in (r, x, b):
        v = np.abs(a[keep])
        v = v[~np.isnan(v)]
        sums.append(float(v.max()) if len(v) else 0.0)
    sums.append(float(np.count_nonzero(u & ~fin)))
    return r, tuple(sums)


def ratio(rn, xn, bn, mutant=None):
    """rho = |r| / (min(|x|, 1e6 |b|) + |b|), 0.0 when |r| is 0: the product, the minimum, the sum and the quotient each rounded."""
    if rn == 0.0:
        return 0.0
    with np.errstate(all="ignore"):
        cap = F(XCAP) * F(bn)
        small = F(xn) if (mutant == "no_min_in_ratio" or xn < cap) else cap
        return float(F(rn) / (small + F(bn)))


def scalar(sums, rec, t, tol, min_steps, band_status=0.0, mutant=None):
    """The record behind step t on a copy (``rec`` is ignored at t == 0)."""
    if t == 0:
        rec = np.zeros(8)
        if band_status != 0.0:
            rec[STATUS] = BAND_FAILED
            return rec
    else:
        rec = np.array(rec, dtype=F)
        if rec[STATUS] != RUNNING:
            return rec
    rn, xn, bn, bad = sums
    prev = 0.0 if t == 0 else float(rec[RHO])
    rho = ratio(rn, xn, bn, mutant)
    rec[STEPS], rec[RNORM], rec[XNORM], rec[BNORM], rec[RHO], rec[PREV] = float(t), rn, xn, bn, rho, prev
    if t == 0:
        rec[RHO0] = rho
    converged = t >= min_steps and rho <= tol
    stalled = t >= 1 and rho > F(IMPROVE) * F(prev)
    if bad > 0.0:
        rec[STATUS] = NON_FINITE
    elif mutant == "stall_before_convergence" and stalled:
        rec[STATUS] = STALLED
    elif converged:
        rec[STATUS] = CONVERGED
    elif stalled:
        rec[STATUS] = STALLED
    else:
        rec[STATUS] = RUNNING
    return rec


def correct(x, d, rec, where=None, mutant=None):
    x = np.array(x, dtype=F)
    if rec[STATUS] != RUNNING and mutant != "correct_behind_stop":
        return x
    u = unknowns(len(x), where)
    with np.errstate(all="ignore"):
        x[u] = x[u] + np.asarray(d, dtype=F)[u]
    return x


# ---------------------------------------------------------------- a whole refinement
def refine(solve, kx, b, x, where=None, tol=TOL, min_steps=0, steps=0, band_status=0.0, mutant=None, kx_parts=None):
    """Begin and ``steps`` enqueued steps: a list of ``(x, r, rec)`` after step 0, 1 ... ``steps``.  ``solve(r)``: d = K^-1 r with
    the factors in place (0.0 at the fixed variables), ``kx(x)``: q = K x.  Behind a stop a step runs its solve and changes nothing
    else.  ``kx_parts`` (for the mutant "fused_residual"): x -> (the sum without its last product, the last product)."""
    x = np.array(x, dtype=F)

    def measure(x, rec, t):
        fused = kx_parts(x) if (mutant == "fused_residual" and kx_parts is not None) else None
        r, sums = resid(b, kx(x), x, where, mutant, fused)
        return r, scalar(sums, rec, t, tol, min_steps, band_status, mutant)

    r, rec = measure(x, None, 0)
    out = [(x.copy(), r, rec)]
    for t in range(1, steps + 1):
        running = rec[STATUS] == RUNNING
        if running or (mutant == "correct_behind_stop" and band_status == 0.0):
            x = correct(x, solve(r), rec, where, mutant)
        r, rec = measure(x, rec, t)
        out.append((x.copy(), r, rec))
    return out


def refine_host(solve, kx, b, x, where=None, tol=TOL, min_steps=0, max_steps=MAX_STEPS, band_status=0.0, mutant=None, kx_parts=None):
    """What ``pk_solve_banded_refined`` leaves: ``(x, r, rec)``, one step at a time behind a read of the record until the status is
    not 0 or ``max_steps`` are done -- then status 5 in this copy."""
    history = refine(solve, kx, b, x, where, tol, min_steps, max_steps, band_status, mutant, kx_parts)
    done = next((k for k, (_, _, rec) in enumerate(history) if rec[STATUS] != RUNNING), max_steps)
    x, r, rec = history[done]
    rec = rec.copy()
    if rec[STATUS] == RUNNING:
        rec[STATUS] = EXHAUSTED
    return x, r, rec


# ---------------------------------------------------------------- synthetic systems
def squeezed(nb, w, p, seed, j, factor):
    """``band_cases.system(nb, w, p, seed, "plain")`` with column j and row j of B scaled by ``factor`` (the diagonal entry once):
    B becomes ill-conditioned, K = [[B, U], [U^T, C]] does not -- U's row j is as it was."""
    AB, U, C, rhs = bc.system(nb, w, p, seed, "plain")
    AB[w: 3 * w + 1, j] *= factor                                 # column j: the rows j - w ... j + w
    for c in range(max(0, j - w), min(nb, j + w + 1)):
        if c != j:
            AB[2 * w + j - c, c] *= factor                        # row j
    return AB, U, C, rhs


class Dense:
    """One synthetic system: its solve with the factors in place and the product with the true K, in permuted order (the order
    of ``pk_band_raw_dev``: every element an unknown)."""

    def __init__(self, AB, U, C, rhs):
        self.AB, self.U, self.C, self.rhs = AB, U, C, np.asarray(rhs, dtype=F)
        self.w = (AB.shape[0] - 1) // 3
        self.nb, self.p = AB.shape[1], C.shape[0]
        self.K = bc.full_matrix(AB, U, C, self.w)
        self.N = self.nb + self.p

    def kx_parts(self, x):
        """``(q_before, last)``: q = K x is ``q_before + last`` -- the products K_ij x_j, each rounded, added to 0.0 in ascending
        j; ``last`` is the product of the last column."""
        with np.errstate(all="ignore"):
            P = self.K * np.asarray(x, dtype=F)[None, :]
            q = np.zeros(self.N)
            for j in range(self.N - 1):
                q = q + P[:, j]
            return q, (P[:, self.N - 1] if self.N else np.zeros(0))

    def kx(self, x):
        q, last = self.kx_parts(x)
        with np.errstate(all="ignore"):
            return q + last if self.N else q

    def solve(self, r):
        """d = K^-1 r as ``pk_band_raw_dev`` computes it (it factors again: the same bits every time); None after a failure."""
        return bc.solve_system(self.AB, self.U, self.C, r)[2]

    def first(self):
        """The solve of the system's own right-hand side: ``(x or None, band record)``."""
        _, _, x, rec = bc.solve_system(self.AB, self.U, self.C, self.rhs)
        return x, rec

    def refine(self, steps, tol=TOL, min_steps=0, mutant=None):
        x, _ = self.first()
        return refine(self.solve, self.kx, self.rhs, x, None, tol, min_steps, steps, 0.0, mutant, self.kx_parts)


def table_system(row):
    (nb, w, p, seed, variant), squeeze, _, _ = row
    if squeeze is None:
        return Dense(*bc.system(nb, w, p, seed, variant))
    return Dense(*squeezed(nb, w, p, seed, *squeeze))


# ---------------------------------------------------------------- a model's K from its CSR maps
class _MapSystem:
    """What ``minres_cases.Kkt`` reads of a system, built from an evaluator's two CSR maps and their values: the structures
    ``pk_set_csr_operator`` was handed (``CsrMap.operator`` / ``transposed`` / ``symmetric``)."""

    def __init__(self, map_j, map_h, jvals, hvals):
        self.m, self.n = map_j.shape

        def structure(op):
            src = np.arange(op.nnz) if op.src is None else op.src
            return cg.Structure(op.indptr, op.indices, src, op.shape[1])

        self.J, self.JT, self.H = structure(map_j.operator()), structure(map_j.transposed()), structure(map_h.symmetric())
        self.jvals, self.hvals = np.asarray(jvals, dtype=F), np.asarray(hvals, dtype=F)


class Model:
    """The planned system of a model: ``where`` of the plan, the solve of ``band_cases.emulate`` and the product of
    ``minres_cases.Kkt.kv`` on the same values."""

    def __init__(self, ordering, map_j, map_h, hvals, jvals, s1, s2):
        self.ordering, self.hvals, self.jvals, self.s1, self.s2 = ordering, hvals, jvals, s1, s2
        self.kkt = mc.Kkt(_MapSystem(map_j, map_h, jvals, hvals))
        size = self.kkt.N
        self.where = np.full(size, -1, dtype=np.int32)
        order = np.asarray(ordering.order)
        self.where[order] = np.arange(len(order), dtype=np.int32)

    def kx(self, x):
        with np.errstate(all="ignore"):
            return self.kkt.kv(True, self.s1, self.s2, x)

    def solve(self, r):
        return bc.emulate(self.ordering, self.hvals, self.jvals, self.s1, self.s2, r)[0]

    def first(self, b):
        """The unrefined solve ``(x or None, band record)``, computed once per right-hand side object."""
        if getattr(self, "_first_of", None) is not b:
            self._first_of, self._first = b, bc.emulate(self.ordering, self.hvals, self.jvals, self.s1, self.s2, b)
        return self._first

    def refine_host(self, b, max_steps, tol=TOL, min_steps=0):
        """``(x, r, rec, band record)`` as ``pk_solve_banded_refined`` leaves them (x None after a failed factorisation)."""
        x, band = self.first(b)
        if x is None:
            return None, None, scalar(None, None, 0, tol, min_steps, band[bc.STATUS]), band
        x, r, rec = refine_host(self.solve, self.kx, b, x, self.where, tol, min_steps, max_steps)
        return x, r, rec, band


# ---------------------------------------------------------------- vectors of the step-form tests
def step_vectors(length, seed=5, planted=True, fixed=True):
    """``(where, b, q, x, d)`` of full-mantissa values.  ``fixed``: every seventh element (and the last but one) is no unknown
    and holds NaN in b, q, x and d -- nothing may read it.  ``planted``: one NaN and one infinity at unknowns of x, b and q."""
    rng = np.random.default_rng(1000 * seed + length)
    b, q, x, d = (rng.uniform(-1.0, 1.0, length) for _ in range(4))
    q = b + 2.0 ** -20 * q                       # a residual of size 1e-6 with full-mantissa bits
    where = None
    if fixed:
        where = np.arange(length, dtype=np.int32)
        out = np.zeros(length, dtype=bool)
        out[3::7] = True
        if length >= 2:
            out[length - 2] = True
        where[out] = -1
        for a in (b, q, x, d):
            a[out] = np.nan
    if planted:
        live = np.flatnonzero(unknowns(length, where))
        spots = live[np.linspace(0, len(live) - 1, 6).astype(int)] if len(live) else []
        for k, (a, v) in enumerate(((x, np.nan), (x, np.inf), (b, np.nan), (b, -np.inf), (q, np.nan), (q, np.inf))):
            if len(spots) > k:
                a[spots[k]] = v
    return where, b, q, x, d
