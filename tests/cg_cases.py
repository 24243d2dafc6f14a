"""A NumPy emulator of the whole CG solve of pockit_amd/csrc/pk_cg.cpp, bit for bit, and the synthetic systems it is tested on.
A plain helper module on top of tests/sparse_cases.py, shared by tests/test_cg_cases_cpu.py (which tests this module),
tests/test_cg_cpu.py (the host stand-in's walk against it) and tests/test_gpu_cg.py (the kernels against it).

The products are ``sparse_cases.emulate_operator`` (the association of pk_op_rows / pk_op_long); one application of K runs in
the unit's fixed order q = s o v, t = A1 v, t = d o t, q = H v + q, q = A2 t + q.  A dot follows the unit's header: index i
belongs to piece i / 2048; thread t adds the terms at piece * 2048 + t + 256 j, j = 0 ... 7, ascending, to 0.0; the tree of
widths 128 ... 1; then one workgroup whose thread t adds the pieces t, t + 256, ... ascending, and the same tree.  Every product
is rounded before it is added (NumPy never fuses).  ``mutant`` names one deliberate mistake each (MUTANTS): the CPU test requires
every one of them to be caught.

The systems live on the sizes of contexts A and B of sparse_cases.CONTEXTS: J as a structure with ``src`` into the context's
Jacobian value array, J^T as its transpose with the transposed ``src`` (on B one column of 300 entries, so that pk_op_long is
in the loop; A has only 36 rows, so no column of J can be long there), a symmetric H with ``src`` into the Hessian value array
(its values repeat: the array is shorter than n).  Family "pd": d >= 0 and s chosen by Gershgorin, s_i = sum_j |H_ij| + 1
(primal; 1 without H) or 0.5 (dual), so lambda_min(K) >= LAMBDA[form] by construction.  Family "indefinite": the primal K is
H + 1e-3 I (d = 0) with H's mixed signs, the dual K is -J J^T + 1e-3 I (d = -1)."""
import functools
from fractions import Fraction

import numpy as np
import scipy.sparse

import sparse_cases as sc

BLOCK, PIECE = sc.BLOCK, 8 * sc.BLOCK
STATUS, ITERS, RR, THR, RZ, PQ, ALPHA, BETA = range(8)
MUTANTS = ("fma_x", "beta_inverted", "thr_from_r0", "frozen_moves_x", "tree_stops_at_2", "strided_first_trip", "minv_null_zero",
           "d_wrong_side")
LAMBDA = {0: 1.0, 1: 0.5}       # lower bounds of lambda_min(K) of family "pd", by construction


# ---------------------------------------------------------------- dots
def dot(terms, mutant=None):
    """The sum of ``terms`` (already rounded products) as a piece kernel and the scalar step associate it."""
    terms = np.asarray(terms, dtype=np.float64)
    n_pieces = max(1, -(-len(terms) // PIECE))
    a = np.zeros(n_pieces * PIECE)
    a[: len(terms)] = terms
    a = a.reshape(n_pieces, 8, BLOCK)
    th = np.zeros((n_pieces, BLOCK))
    for j in range(8):
        th = th + a[:, j, :]
    partial = sc._tree(th, "tree_stops_at_2" if mutant == "tree_stops_at_2" else None)
    trips = -(-n_pieces // BLOCK)
    padded = np.zeros(trips * BLOCK)
    padded[:n_pieces] = partial
    padded = padded.reshape(trips, BLOCK)
    acc = np.zeros((1, BLOCK))
    for j in range(1 if mutant == "strided_first_trip" else trips):
        acc = acc + padded[j]
    return float(sc._tree(acc, "tree_stops_at_2" if mutant == "tree_stops_at_2" else None)[0])


def _fma(a, b, c):
    """a * b + c with one rounding, exactly (the mistake the 'fma_x' mutant makes)."""
    return np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())])


# ---------------------------------------------------------------- the vector steps on plain arrays and a record of 8 doubles
def step_init(b, x0, kx, minv, s, tol, mutant=None):
    """begin's init: (x, r, z, p, q, rec).  ``kx`` = K x0 (ignored without x0)."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros(len(b)) if x0 is None else np.array(x0, dtype=np.float64)
    r = b.copy() if x0 is None else b - kx
    if minv is None:
        z = np.zeros(len(b)) if mutant == "minv_null_zero" else r.copy()
    else:
        z = minv * r
    p = z.copy()
    q = np.zeros(len(b)) if s is None else s * p
    bb, rz, rr = dot(b * b, mutant), dot(r * z, mutant), dot(r * r, mutant)
    thr = (tol * tol) * (rr if mutant == "thr_from_r0" else bb)
    rec = np.array([1.0 if rr <= thr else 0.0, 0.0, rr, thr, rz, 0.0, 0.0, 0.0])
    return x, r, z, p, q, rec


def step_curvature(p, q, rec, mutant=None):
    """pq = p.q and scalar step A, on a copy of the record."""
    rec = rec.copy()
    if rec[STATUS] != 0.0:
        return rec
    pq = dot(p * q, mutant)
    rec[PQ] = pq
    if not np.isfinite(pq):
        rec[STATUS] = 3.0
    elif not pq > 0.0:
        rec[STATUS] = 2.0
    else:
        rec[ALPHA] = rec[RZ] / pq
    return rec


def step_update(x, r, z, p, q, minv, rec, mutant=None):
    """The update and scalar step B: (x, r, z, rec), the inputs untouched."""
    if rec[STATUS] != 0.0:
        if mutant == "frozen_moves_x":
            return x + rec[ALPHA] * p, r, z, rec.copy()
        return x.copy(), r.copy(), z.copy(), rec.copy()
    rec = rec.copy()
    alpha = rec[ALPHA]
    x = _fma(np.full(len(p), alpha), p, x) if mutant == "fma_x" else x + alpha * p
    r = r - alpha * q
    if minv is None:
        z = np.zeros(len(r)) if mutant == "minv_null_zero" else r.copy()
    else:
        z = minv * r
    rz, rr = dot(r * z, mutant), dot(r * r, mutant)
    rec[ITERS] += 1.0
    rec[RR] = rr
    if not (np.isfinite(rr) and np.isfinite(rz)):
        rec[STATUS] = 3.0
    elif rr <= rec[THR]:
        rec[STATUS] = 1.0
    else:
        with np.errstate(all="ignore"):
            rec[BETA] = rec[RZ] / rz if mutant == "beta_inverted" else rz / rec[RZ]
        rec[RZ] = rz
    return x, r, z, rec


def step_direction(z, p, s, rec):
    """(p, q): p = z + beta p only while the status is 0; q = s o p (or 0.0) always."""
    if rec[STATUS] == 0.0:
        p = z + rec[BETA] * p
    else:
        p = p.copy()
    return p, (np.zeros(len(p)) if s is None else s * p)


def step_jacobi(g, s):
    a = np.abs(g if s is None else g + s)
    good = (a > 0) & np.isfinite(a)
    return np.where(good, 1.0 / np.where(good, a, 1.0), 1.0)


# ---------------------------------------------------------------- synthetic systems
class Structure:
    """A CSR structure whose entry e takes vals[src[e]]: what pk_set_csr_operator is handed, and what
    ``sparse_cases.emulate_operator`` reads of a case (indptr, n_rows, products())."""

    def __init__(self, indptr, indices, src, n_cols):
        self.indptr = np.asarray(indptr, dtype=np.int32)
        self.indices = np.asarray(indices, dtype=np.int32)
        self.src = np.asarray(src, dtype=np.int32)
        self.n_rows, self.n_cols, self.nnz = len(self.indptr) - 1, n_cols, len(self.indices)

    def matrix(self, vals):
        return scipy.sparse.csr_array((vals[self.src], self.indices.astype(np.int64), self.indptr.astype(np.int64)),
                                      shape=(self.n_rows, self.n_cols))

    def transposed(self):
        t = scipy.sparse.csr_array((np.arange(1, self.nnz + 1), self.indices.astype(np.int64), self.indptr.astype(np.int64)),
                                   shape=(self.n_rows, self.n_cols)).T.tocsr()
        t.sort_indices()
        return Structure(t.indptr, t.indices, self.src[t.data - 1], self.n_rows)


class _Terms:
    def __init__(self, structure, terms):
        self.indptr, self.n_rows, self._terms = structure.indptr, structure.n_rows, terms

    def products(self):
        return self._terms


def apply_structure(structure, vals, v, add=None):
    """y = A(vals) v (+ add) with the association of pk_op_rows / pk_op_long."""
    return sc.emulate_operator(_Terms(structure, vals[structure.src] * v[structure.indices]), add)


def sq_sum(structure, vals, w=None, add=None):
    """pk_operator_reduce_dev's mode 1: the square rounded first, then the product with the weight."""
    a = vals[structure.src]
    t = a * a
    if w is not None:
        t = t * w[structure.indices]
    return sc.emulate_operator(_Terms(structure, t), add)


def _full(rng, size, lo=-1.0, hi=1.0):
    """Full-mantissa doubles."""
    return rng.uniform(lo, hi, size)


class System:
    """One synthetic system on a context's sizes: structures, values, and per (form, family) the inputs of a solve."""

    def __init__(self, ctx, seed, values=None):
        """``values``: (jvals, hvals) of the context's two value arrays in place of the random ones (same structures)."""
        c = sc.CONTEXTS[ctx]
        self.ctx, self.n, self.m = ctx, c["n"], c["m"]
        n, m = self.n, self.m
        rng = np.random.default_rng(seed)
        rows = []
        long_col = 7 if m > 300 else None
        for r in range(m):
            cols = set(rng.choice(n, int(rng.integers(2, 6)), replace=False).tolist())
            if long_col is not None and r % 3 == 0:      # 300 of B's 900 rows hold column 7: J^T's row 7 has 300 entries
                cols.add(long_col)
            rows.append(sorted(cols))
        indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows])))
        nnz = int(indptr[-1])
        assert nnz <= c["nnz_j"]
        self.J = Structure(indptr, np.concatenate(rows), rng.permutation(c["nnz_j"])[:nnz], n)
        self.JT = self.J.transposed()
        self.has_long = bool(np.diff(self.JT.indptr).max() > BLOCK)
        assert self.has_long == (long_col is not None)
        # H: the lower triangle L has a diagonal and two sub-diagonals with gaps; the symmetric structure lists L's row, then
        # the mirrored entries (pockit_amd/csr.py's CsrMap.symmetric); entry e of L takes hvals[e mod nnz_h]
        l_rows, l_cols = [], []
        for i in range(n):
            for jc in (i - 3, i - 1):
                if jc >= 0 and (i + jc) % 4 != 0:
                    l_rows.append(i); l_cols.append(jc)
            l_rows.append(i); l_cols.append(i)
        l_rows, l_cols = np.array(l_rows), np.array(l_cols)
        l_src = np.arange(len(l_rows)) % c["nnz_h"]
        self.diag_pos = l_src[l_rows == l_cols].astype(np.int32)
        assert len(self.diag_pos) == n
        off = l_rows != l_cols
        order = np.lexsort((np.concatenate((np.zeros(len(l_rows)), np.ones(off.sum()))), np.concatenate((l_rows, l_cols[off]))))
        all_rows = np.concatenate((l_rows, l_cols[off]))[order]
        all_cols = np.concatenate((l_cols, l_rows[off]))[order]
        all_src = np.concatenate((l_src, l_src[off]))[order]
        self.H = Structure(np.concatenate(([0], np.cumsum(np.bincount(all_rows, minlength=n)))), all_cols, all_src, n)
        self.jvals = _full(rng, c["nnz_j"])
        self.hvals = _full(rng, c["nnz_h"])
        if values is not None:
            self.jvals, self.hvals = (np.ascontiguousarray(v, dtype=np.float64) for v in values)
            assert self.jvals.shape == (c["nnz_j"],) and self.hvals.shape == (c["nnz_h"],)
        self.Jm, self.Hm = self.J.matrix(self.jvals), self.H.matrix(self.hvals)
        assert abs(self.Hm - self.Hm.T).max() == 0.0
        self.rng_seed = seed

    def inputs(self, form, family, with_h=None):
        """dict(form, with_h, d, s, b, x0, K): K the scipy matrix of the same numbers."""
        n, m = self.n, self.m
        size, other = (n, m) if form == 0 else (m, n)
        rng = np.random.default_rng(self.rng_seed + 10 * form + (1 if family == "pd" else 2))
        if with_h is None:
            with_h = form == 0
        b, x0 = _full(rng, size), _full(rng, size)
        if family == "pd":
            d = _full(rng, other, 0.25, 1.0)
            if form == 0:
                s = (np.asarray(abs(self.Hm).sum(axis=1)).reshape(-1) if with_h else np.zeros(n)) + 1.0 + _full(rng, n, 0.0, 0.5)
            else:
                s = 0.5 + _full(rng, m, 0.0, 0.5)
        else:
            d = np.zeros(other) if form == 0 else -np.ones(other)
            s = np.full(size, 1.0e-3)
        D = scipy.sparse.diags_array(d)
        if form == 0:
            K = self.Jm.T @ D @ self.Jm + scipy.sparse.diags_array(s)
            if with_h:
                K = K + self.Hm
        else:
            K = self.Jm @ D @ self.Jm.T + scipy.sparse.diags_array(s)
        return dict(form=form, with_h=bool(with_h), d=d, s=s, b=b, x0=x0, K=scipy.sparse.csc_array(K))

    # ---- K and its diagonal as the device computes them
    def products(self, form, with_h, d, v, q, mutant=None):
        """Steps 2 ... 5 of one application: q already holds s o v (or 0.0)."""
        a1, a2 = (self.J, self.JT) if form == 0 else (self.JT, self.J)
        t = apply_structure(a1, self.jvals, v)
        if d is not None:
            t = d[np.arange(len(t)) % len(v)] * t if (mutant == "d_wrong_side" and form == 1) else d * t
        if with_h:
            q = apply_structure(self.H, self.hvals, v, q)
        return apply_structure(a2, self.jvals, t, q)

    def kv(self, form, with_h, d, s, v, mutant=None):
        return self.products(form, with_h, d, v, np.zeros(len(v)) if s is None else s * v, mutant)

    def jacobi(self, form, with_h, d, s):
        if form == 0:
            g = sq_sum(self.JT, self.jvals, d, self.hvals[self.diag_pos] if with_h else None)
        else:
            g = sq_sum(self.J, self.jvals, d)
        return step_jacobi(g, s)


SEEDS = {"A": 41, "B": 42}


@functools.lru_cache(maxsize=None)
def system(ctx):
    return System(ctx, SEEDS[ctx])


def emulate_solve(sy, form, with_h, d, s, minv, b, x0, tol, maxiter, check_every=8, mutant=None):
    """(x, rec) as pk_solve_condensed returns them: chunks of min(check_every, remaining) iterations, the iterations behind
    the stop enqueued and frozen; exhaustion is status 4 in the returned record."""
    assert mutant is None or mutant in MUTANTS
    kx = None if x0 is None else sy.kv(form, with_h, d, s, x0, mutant)
    x, r, z, p, q, rec = step_init(b, x0, kx, minv, s, tol, mutant)
    done = 0
    while rec[STATUS] == 0.0 and done < maxiter:
        chunk = min(check_every, maxiter - done)
        for _ in range(chunk):
            if rec[STATUS] == 0.0:
                q = sy.products(form, with_h, d, p, q, mutant)
            rec = step_curvature(p, q, rec, mutant)
            x, r, z, rec = step_update(x, r, z, p, q, minv, rec, mutant)
            p, q = step_direction(z, p, s, rec)
        done += chunk
    if rec[STATUS] == 0.0:
        rec = rec.copy()
        rec[STATUS] = 4.0
    return x, rec


# ---------------------------------------------------------------- inputs of the vector-step tests
STEP_LENGTHS = (1, 255, 256, 257, 2047, 2048, 2049, 524289)
STEP_LENGTH_PAST_THE_PIECE_CAP = 4194305


def step_vectors(length, seed=5):
    """Full-mantissa vectors b, x0, kx, minv, s, x, r, z, p, q of one length."""
    rng = np.random.default_rng(seed + length)
    names = ("b", "x0", "kx", "minv", "s", "x", "r", "z", "p", "q")
    v = {k: _full(rng, length) for k in names}
    v["minv"] = np.abs(v["minv"]) + 0.25
    return v
