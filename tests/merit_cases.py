"""Inputs, exact references and a bit-for-bit NumPy emulator for the merit kernels ``pk_trial``, ``pk_merit`` and ``pk_merit_fin``
(pockit_amd/csrc/pk_merit.cpp).  A plain helper module, shared by tests/test_merit_cases_cpu.py (which tests this module) and
tests/test_gpu_merit.py (which tests the kernels).

The emulator follows the association the code documents.  Index i of entry b belongs to piece p = i // 2048; thread t of the
piece adds the terms of p * 2048 + t + 256 j, j = 0 ... 7, in ascending j to 0.0 (an index beyond the vector's length adds
nothing); the 256 thread values are reduced by the tree of widths 128, 64 ... 1 (slot t += slot t + w); per entry, thread t
adds the pieces t, t + 256, ... in ascending order to 0.0 and the same tree follows.  Columns 2 and 5 walk the same way with
max.  Squares and products are rounded before they are added (``fma=True`` fuses them instead: what the kernels must NOT do).
n_pieces = max(1, ceil(max(n_g, n_x) / 2048)).

Exact cases, built the way tests/sparse_cases.py builds its inputs: 24-bit mantissas and ONE power-of-two scale per entry b
from {-40, -20, 0, 20, 40}, so entries differ by up to 2**80 while the terms of an entry lie within a factor of 16 of each
other.  The bounds are shared by the entries, so in these cases they are 0 or infinite by index (i % 3: equality at 0, upper
bound 0, lower bound 0): lo - v is then -v, every square and every product (grad 24-bit at the entry's scale, d 24-bit at
scale 0) is exact, and ``math.fsum`` over the exact terms is the correctly rounded reference.  A second family ("bounded") keeps
every entry at scale 0 and gives finite bounds -[1/4, 1/2) and +[1/4, 1/2) with 24-bit mantissas under values in +-[1, 2): every
value violates one of them by (1/2, 7/4], a multiple of 2**-25 -- exact in 26 bits, its square in 52.  Every entry also holds a few non-finite g and grad values, which must be counted and left out.

The bound is derived, not measured: a term takes part in at most D = 8 + 8 + trips + 8 additions (its thread's eight, the
tree, ``trips = ceil(n_pieces / 256)`` strided additions of pk_merit_fin, the tree again), so the sum errs by at most
gamma_D * sum|t| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); the reference's own rounding is one
more u, hence gamma_{D+1} * sum|t| -- the form of sparse_cases' gamma_{L+1} * sum|t|, with the depth of this association in
place of the row length.  The max columns, the copied f and the count must be exact.

``MUTANTS`` names one deliberate mistake each: the CPU test requires the checker to catch every one of them."""
import functools
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
BLOCK = 256                 # PK_BLOCK
PER_THREAD = 8              # PK_MERIT_PER_THREAD
PIECE = BLOCK * PER_THREAD  # PK_MERIT_PIECE
GRID_CAP = 2048             # PK_LIB_GRID_CAP of csrc/pk_libkernel.h
COLUMNS = ("f", "theta1", "theta_inf", "theta2_sq", "bound1", "bound_inf", "slope", "bad")
SUM_COLUMNS, MAX_COLUMNS = (1, 3, 4, 6), (2, 5)
SCALES = (-40, -20, 0, 20, 40)
MUTANTS = ("tail_not_zeroed", "second_trip_dropped", "bounds_swapped", "nonfinite_added", "ld_is_length", "max_as_sum")


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def n_pieces(n_g, n_x):
    return max(1, -(-max(n_g, n_x) // PIECE))


def depth(n_g, n_x):
    """Additions a term takes part in at most: thread, tree, strided trips of pk_merit_fin, tree."""
    return PER_THREAD + 8 + -(-n_pieces(n_g, n_x) // BLOCK) + 8


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def _fma(a, b, c):
    """Elementwise a * b + c with ONE rounding (exact rational arithmetic; non-finite operands go the plain way)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    out = np.empty(a.shape)
    fa, fb, fc, fo = a.reshape(-1), b.reshape(-1), c.reshape(-1), out.reshape(-1)
    for k in range(fa.size):
        x, y, z = float(fa[k]), float(fb[k]), float(fc[k])
        if x == 0.0 or y == 0.0 or not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
            fo[k] = x * y + z
        else:
            fo[k] = float(Fraction(x) * Fraction(y) + Fraction(z))
    return out


def trial_points(x, d, alphas, fma=False):
    """(B, n): x + a * d, the product rounded first -- or fused."""
    a = np.asarray(alphas, dtype=np.float64)[:, None]
    return _fma(a, d[None, :], x[None, :]) if fma else x[None, :] + a * d[None, :]


def _viol(v, lo, hi):
    """max(lo - v, v - hi, 0) by comparisons: a NaN difference loses."""
    with np.errstate(invalid="ignore"):
        a, b = lo - v, v - hi
        r = np.where(a > 0.0, a, 0.0)
        return np.where(b > r, b, r)


def _rows(flat, B, length, ld, mutant):
    """(B, length) rows of a flat array with leading dimension ld."""
    flat = np.asarray(flat, dtype=np.float64).reshape(-1)
    if mutant == "ld_is_length":
        ld = length
    idx = np.arange(B)[:, None] * ld + np.arange(length)[None, :]
    return flat[idx] if length else np.zeros((B, 0))


def _pieces(a, P, fill=0.0):
    """(B, L) -> (B, P, 8, 256): [b, p, j, t] is index p * 2048 + j * 256 + t, ``fill`` beyond L."""
    B, L = a.shape
    out = np.full((B, P * PIECE), fill)
    out[:, :L] = a
    return out.reshape(B, P, PER_THREAD, BLOCK)


def _tree(a, is_max):
    a = a.copy()
    w = BLOCK // 2
    while w >= 1:
        a[..., :w] = np.maximum(a[..., :w], a[..., w: 2 * w]) if is_max else a[..., :w] + a[..., w: 2 * w]
        w //= 2
    return a[..., 0]


def _thread_walk(x, y, is_max, fma):
    """Eight terms x[..., j, :] (* y[..., j, :]) per thread in ascending j, then the tree: (B, P)."""
    acc = np.zeros(x.shape[:2] + (BLOCK,))
    for j in range(PER_THREAD):
        if is_max:
            acc = np.where(x[:, :, j] > acc, x[:, :, j], acc)
        elif y is None:
            acc = acc + x[:, :, j]
        elif fma:
            acc = _fma(x[:, :, j], y[:, :, j], acc)
        else:
            acc = acc + x[:, :, j] * y[:, :, j]
    return _tree(acc, is_max)


def _fin(partial, is_max, mutant):
    """(B, P) -> (B,): thread t takes the pieces t, t + 256, ...; the tree."""
    B, P = partial.shape
    trips = -(-P // BLOCK)
    padded = np.zeros((B, trips * BLOCK))
    padded[:, :P] = partial
    padded = padded.reshape(B, trips, BLOCK)
    acc = np.zeros((B, BLOCK))
    for k in range(1 if mutant == "second_trip_dropped" else trips):
        acc = np.maximum(acc, padded[:, k]) if is_max else acc + padded[:, k]
    return _tree(acc, is_max)


def emulate(B, n_g, g, ldg, clb, cub, n_x, X, ldx, vlb, vub, grad, ldgrad, d, f, fma=False, mutant=None):
    """``out`` (B, 8) as pk_merit and pk_merit_fin compute it, bit for bit, from the arguments of ``pk_merit_reduce_dev``."""
    assert mutant is None or mutant in MUTANTS
    P = n_pieces(n_g, n_x)
    g, X, grad = _rows(g, B, n_g, ldg, mutant), _rows(X, B, n_x, ldx, mutant), _rows(grad, B, n_x, ldgrad, mutant)
    f = np.asarray(f, dtype=np.float64).reshape(B)
    clb, cub, vlb, vub = (np.asarray(a, dtype=np.float64) for a in (clb, cub, vlb, vub))
    if mutant == "bounds_swapped":
        clb, cub, vlb, vub = cub, clb, vub, vlb
    with np.errstate(invalid="ignore", over="ignore"):
        g_ok, grad_ok = np.isfinite(g), np.isfinite(grad)
        if mutant == "nonfinite_added":
            wg, gr = _viol(g, clb[None, :], cub[None, :]) + np.where(g_ok, 0.0, np.nan), grad
        else:
            wg, gr = np.where(g_ok, _viol(np.where(g_ok, g, 0.0), clb[None, :], cub[None, :]), 0.0), np.where(grad_ok, grad, 0.0)
        wx = _viol(X, vlb[None, :], vub[None, :])
        bad = [(~g_ok).astype(np.float64), (~grad_ok).astype(np.float64)]
        tail = 0.0
        if mutant == "tail_not_zeroed":      # the last piece reads on behind the vector's end: whatever lies there
            tail = np.nan
        wgp, wxp, grp = _pieces(wg, P, tail), _pieces(wx, P, tail), _pieces(gr, P, tail)
        dp = None if d is None else _pieces(np.broadcast_to(np.asarray(d, dtype=np.float64), (B, n_x)), P, tail)
        out = np.zeros((B, 8))
        out[:, 0] = f
        mx = "max_as_sum" != mutant
        out[:, 1] = _fin(_thread_walk(wgp, None, False, fma), False, mutant)
        out[:, 2] = _fin(_thread_walk(wgp, None, mx, fma), mx, mutant)
        out[:, 3] = _fin(_thread_walk(wgp, wgp, False, fma), False, mutant)
        out[:, 4] = _fin(_thread_walk(wxp, None, False, fma), False, mutant)
        out[:, 5] = _fin(_thread_walk(wxp, None, mx, fma), mx, mutant)
        if d is not None:
            out[:, 6] = _fin(_thread_walk(grp, dp, False, fma), False, mutant)
        count = _fin(_thread_walk(_pieces(bad[0], P), None, False, False) + _thread_walk(_pieces(bad[1], P), None, False, False), False, mutant)
        out[:, 7] = count + (~np.isfinite(f)).astype(np.float64)
    return out


def emulate_dense(f, grad, g, X, bounds, d=None):
    """The emulator on what ``evaluate_batch(X, None)`` returns (dense rows) and the four bound vectors."""
    c_lb, c_ub, v_lb, v_ub = bounds
    B, m, n = len(f), g.shape[1], X.shape[1]
    return emulate(B, m, g, m, c_lb, c_ub, n, X, n, v_lb, v_ub, grad, n, d, f)


# ---------------------------------------------------------------- cases
def _unit(rng, size):
    """+-[1, 2) with a 24-bit mantissa."""
    x = rng.integers(2 ** 23, 2 ** 24, size).astype(np.float64) / 2.0 ** 23
    return x * rng.choice([-1.0, 1.0], size)


def _padded(rows, ld):
    """(B, L) -> flat (B * ld) with NaN in the padding."""
    B, L = rows.shape
    out = np.full((B, ld), np.nan)
    out[:, :L] = rows
    return out.reshape(-1)


class MeritCase:
    """One call of ``pk_merit_reduce_dev``: B entries, g of n_g values, X and grad of n_x, rows padded with NaN to leading
    dimensions larger than the lengths.  ``kind``: "scaled" and "bounded" are exact (see the module docstring), "full" draws
    53-bit inputs and finite bounds (emulator bits only)."""

    def __init__(self, name, kind, B, n_g, n_x, seed, with_d=True):
        self.name, self.kind, self.B, self.n_g, self.n_x = name, kind, B, n_g, n_x
        self.id = f"{kind}-{name}-B{B}"
        rng = np.random.default_rng(seed)
        self.ldg, self.ldx, self.ldgrad = n_g + 3, n_x + 1, n_x + 5
        inf = np.inf
        if kind == "scaled":
            scale = np.ldexp(1.0, np.asarray(SCALES)[(np.arange(B) + seed) % 5])[:, None]
            pat = lambda n: (np.where(np.arange(n) % 3 == 1, -inf, 0.0), np.where(np.arange(n) % 3 == 2, inf, 0.0))  # noqa: E731
            (self.clb, self.cub), (self.vlb, self.vub) = pat(n_g), pat(n_x)
            g, X, grad = (_unit(rng, (B, k)) * scale for k in (n_g, n_x, n_x))
            self.d = _unit(rng, n_x)
            self.f = _unit(rng, B) * scale[:, 0]
        elif kind == "bounded":
            def pair(n):
                return -np.abs(_unit(rng, n)) / 4.0, np.abs(_unit(rng, n)) / 4.0
            (self.clb, self.cub), (self.vlb, self.vub) = pair(n_g), pair(n_x)
            g, X, grad = (_unit(rng, (B, k)) for k in (n_g, n_x, n_x))
            self.d = _unit(rng, n_x)
            self.f = _unit(rng, B)
        else:
            assert kind == "full"
            def pair(n):
                a, b = rng.standard_normal(n), rng.standard_normal(n)
                return np.minimum(a, b), np.maximum(a, b)
            (self.clb, self.cub), (self.vlb, self.vub) = pair(n_g), pair(n_x)
            g, X, grad = (3.0 * rng.standard_normal((B, k)) for k in (n_g, n_x, n_x))
            self.d = rng.standard_normal(n_x)
            self.f = rng.standard_normal(B)
        if not with_d:
            self.d = None
        # non-finite values, counted and left out: never index 0, so that every entry keeps a term in every column
        self.poisoned = 0
        for b in range(B):
            for rows, n, vals in ((g, n_g, (np.nan, inf)), (grad, n_x, (-inf, np.nan))):
                for k, v in enumerate(vals):
                    if n >= 4:
                        rows[b, 1 + (7 * b + 2 * k) % (n - 1)] = v
        if B > 1:
            self.f = self.f.copy()
            self.f[B - 1] = np.nan
        self.g_rows, self.X_rows, self.grad_rows = g, X, grad
        self.g, self.X, self.grad = _padded(g, self.ldg), _padded(X, self.ldx), _padded(grad, self.ldgrad)
        self.workgroups = B * n_pieces(n_g, n_x)

    def args(self):
        """The arguments of ``emulate`` (and, as device arrays, of ``pk_merit_reduce_dev``)."""
        return (self.B, self.n_g, self.g, self.ldg, self.clb, self.cub, self.n_x, self.X, self.ldx, self.vlb, self.vub, self.grad,
                self.ldgrad, self.d, self.f)

    def emulated(self, fma=False, mutant=None):
        return emulate(*self.args(), fma=fma, mutant=mutant)

    @functools.cached_property
    def terms(self):
        """Per column of SUM_COLUMNS and MAX_COLUMNS the exact terms of every entry, (B, length), 0.0 where an entry is left out."""
        assert self.kind != "full"
        with np.errstate(invalid="ignore"):
            g_ok, grad_ok = np.isfinite(self.g_rows), np.isfinite(self.grad_rows)
            wg = np.where(g_ok, _viol(np.where(g_ok, self.g_rows, 0.0), self.clb[None, :], self.cub[None, :]), 0.0)
            wx = _viol(self.X_rows, self.vlb[None, :], self.vub[None, :])
            slope = np.where(grad_ok, self.grad_rows, 0.0) * (0.0 if self.d is None else self.d[None, :])
        return {1: wg, 2: wg, 3: wg * wg, 4: wx, 5: wx, 6: slope}

    @functools.cached_property
    def reference(self):
        """(ref, bound, sensitivity), each (B, 8).  ref: fsum / max / copy / count; bound: gamma_{D+1} * sum|t| for the sum
        columns, 0 elsewhere; sensitivity: what one lost (or, for a sum, doubled) term changes at least -- the smallest nonzero
        |t| of a sum column, the distance between the two largest terms of a max column, 1 for the count, |f| for f."""
        B = self.B
        ref, bound, sens = np.zeros((B, 8)), np.zeros((B, 8)), np.zeros((B, 8))
        g_bad = (~np.isfinite(self.g_rows)).sum(axis=1)
        grad_bad = (~np.isfinite(self.grad_rows)).sum(axis=1)
        ref[:, 0], ref[:, 7] = self.f, g_bad + grad_bad + ~np.isfinite(self.f)
        sens[:, 0], sens[:, 7] = np.where(np.isfinite(self.f), np.abs(self.f), 1.0), 1.0
        D = depth(self.n_g, self.n_x)
        for q, t in self.terms.items():
            for b in range(B):
                row = t[b]
                if q in SUM_COLUMNS:
                    ref[b, q] = math.fsum(row.tolist())
                    bound[b, q] = float(gamma(D + 1)) * math.fsum(np.abs(row).tolist())
                    live = np.abs(row[row != 0.0])
                    sens[b, q] = live.min() if live.size else 0.0
                else:
                    top = np.sort(row)[-2:] if row.size > 1 else np.array([0.0, row[0] if row.size else 0.0])
                    ref[b, q], sens[b, q] = top[-1], top[-1] - top[-2]
        return ref, bound, sens

    def failures(self, got):
        """(entry, column) cells of ``got`` outside the bound around the exact reference (a NaN where none is due fails)."""
        ref, bound, _ = self.reference
        got = np.asarray(got, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            ok = np.abs(got - ref) <= bound
        ok |= np.isnan(got) & np.isnan(ref)
        return np.argwhere(~ok)


LENGTHS = (1, 255, 256, 257, 2047, 2048, 2049)
BIG = 524289                # 257 pieces: pk_merit_fin's second strided trip; with B = 9, 2 313 workgroups: past the grid cap


@functools.lru_cache(maxsize=None)
def exact_cases():
    cases, seed = [], 500
    for k, L in enumerate(LENGTHS):
        for B in (1, 3, 64):
            seed += 1
            n_x = LENGTHS[(k + 2) % 7]
            kind = "bounded" if (k + B) % 2 and min(L, n_x) >= 255 else "scaled"      # (a lone bounded term may be feasible: no term)
            cases.append(MeritCase(f"{L}x{n_x}", kind, B, L, n_x, seed))
    cases.append(MeritCase(f"{BIG}x2049", "scaled", 9, BIG, 2049, 601))
    cases.append(MeritCase(f"255x{BIG}", "bounded", 2, 255, BIG, 602))
    return tuple(cases)


FULL_SEED = 7


@functools.lru_cache(maxsize=None)
def full_case():
    """Random 53-bit inputs: exact products cannot tell a contracted FMA from multiply-then-add, these can."""
    return MeritCase("2047x2049", "full", 3, 2047, 2049, FULL_SEED)


@functools.lru_cache(maxsize=None)
def no_d_case():
    return MeritCase("257x2049", "bounded", 3, 257, 2049, 603, with_d=False)


@functools.lru_cache(maxsize=None)
def trial_case(n=2049):
    """(x, d, alphas) with full mantissas for pk_trial: 64 step lengths, 0 and 1 among them."""
    rng = np.random.default_rng(FULL_SEED)
    return rng.standard_normal(n), rng.standard_normal(n), np.concatenate(([0.0, 1.0], rng.uniform(1e-3, 1.0, 62)))
