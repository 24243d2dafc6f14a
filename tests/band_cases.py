"""A NumPy emulator of the bordered band LU of pockit_amd/csrc/pk_band.cpp -- fill, factor, solve, border, scatter -- bit for bit,
and the synthetic systems it is tested on.  A plain helper module, shared by tests/test_band_cases_cpu.py (which tests this
module), tests/test_band_cpu.py (the host stand-in's walk against it) and tests/test_gpu_band.py (the kernels against it).

The factorisation is the UNBLOCKED loop of the unit's header: every entry receives its updates in ascending pivot order
whatever the panel width is, so the blocked kernels must give these bits.  Every product is rounded before it is subtracted
(NumPy never fuses); a quotient is the correctly rounded one.  The border's dots are ``cg_cases.dot`` (the pieced dot of
pk_libkernel.h).  ``mutant`` names one deliberate mistake each (MUTANTS): the CPU test requires every one to be caught.

Band storage is LAPACK's: ``AB`` of shape ``(3 w + 1, nb)``, Fortran order, ``B(i, j) = AB[2 w + i - j, j]``.

After a failed pivot the kernels leave the band as the last complete panel left it; the emulator does not state those bits (it
returns the band as its loop left it) -- a failure is held by the record and by ``sol`` staying untouched.  The record's
extremes and interchanges are the ones committed by the last complete panel."""
import numpy as np

import cg_cases as cg

NB, W_CAP, P_CAP = 32, 192, 8          # PK_BD_NB, PK_BD_W_CAP, PK_BD_P_CAP
STATUS, COLUMN, MIN_PIVOT, MAX_PIVOT, R_NB, R_W, R_P, SWAPS = range(8)
MUTANTS = ("fma", "tie_highest", "swap_earlier_columns", "narrow_u", "no_forward_swap", "border_sign", "plain_border_dots")
VARIANTS = ("plain", "tiny_diagonal", "ties", "zero_column", "nan")
# the shapes of the CPU driver and of the GPU test: Nb around the panel width and around w, w around the panel width and at the cap
NB_SHAPES = (0, 1, 2, NB - 1, NB, NB + 1, 2 * NB + 1)
W_SHAPES = (0, 1, 7, NB - 1, NB, NB + 1, W_CAP)
P_SHAPES = (0, 1, 3, P_CAP)
EVERY = 70                             # up to this Nb "tiny_diagonal" makes every column interchange (the row handed on shrinks by
                                       # 2^-10 per column: a long system of that kind is singular in fp64); beyond it most columns do
LONG = (50001, 8, 1)                   # 1 563 panels; 25 pieces per dot


def shapes():
    """(nb, w, p) of every synthetic case but the long one: every Nb with a few widths and borders, every w and p once more."""
    out = []
    for k, nb in enumerate(NB_SHAPES):
        out.append((nb, W_SHAPES[k % len(W_SHAPES)], P_SHAPES[k % len(P_SHAPES)]))
        out.append((nb, 7, P_SHAPES[(k + 1) % len(P_SHAPES)]))
    for k, w in enumerate(W_SHAPES):
        out.append((w + 1, w, P_SHAPES[(k + 2) % len(P_SHAPES)]))           # Nb <= w + 1: one window holds the matrix
        out.append((2 * NB + 1 + w, w, P_SHAPES[(k + 3) % len(P_SHAPES)]))
    out.append((3 * NB + 5, 20, P_CAP))
    return sorted(set(out))


def new_band(nb, w):
    return np.zeros((3 * w + 1, nb), order="F")


def in_band(nb, w):
    """Mask of the slots of ``AB`` that are entries of B (|i - j| <= w, 0 <= i < nb)."""
    r = np.arange(3 * w + 1)[:, None]
    j = np.arange(nb)[None, :]
    i = r - 2 * w + j
    return (r >= w) & (i >= 0) & (i < nb)


def fill_rows(nb, w):
    """Mask of the slots of ``AB`` above the band that take the fill of pivoting (w < j - i <= 2 w, i >= 0)."""
    r = np.arange(3 * w + 1)[:, None]
    j = np.arange(nb)[None, :]
    return (r < w) & (r - 2 * w + j >= 0)


def system(nb, w, p, seed=0, variant="plain"):
    """``(AB, U, C, rhs)`` of full-mantissa values; ``rhs`` in permuted order ``[band part | border]``.  The fill rows of AB
    and its slots outside the matrix are 0.0 (a caller may overwrite them: nothing reads them before it writes them)."""
    rng = np.random.default_rng(1000 * seed + 17 * nb + 3 * w + p)
    AB = new_band(nb, w)
    mask = in_band(nb, w)
    AB[mask] = rng.uniform(-1.0, 1.0, int(mask.sum()))
    if nb:
        d = rng.uniform(1.0, 2.0, nb) * np.where(rng.random(nb) < 0.5, -1.0, 1.0) * (0.25 * w + 1.0)
        AB[2 * w, :] = d * (2.0 ** -26 if variant == "tiny_diagonal" else 1.0)
        if variant == "tiny_diagonal" and w > 0 and nb <= EVERY:      # ... and a dominant subdiagonal: EVERY column but the last interchanges
            sub = AB[2 * w + 1, : nb - 1]
            AB[2 * w + 1, : nb - 1] = sub * 1024.0 + np.where(sub < 0.0, -1024.0, 1024.0)
    if variant == "ties" and nb:
        km = min(w, nb - 1)
        v = AB[2 * w, 0]
        AB[2 * w: 2 * w + km + 1, 0] = v * np.where(np.arange(km + 1) % 2 == 0, 1.0, -1.0)
    if variant == "zero_column" and nb:
        j = (2 * nb) // 3
        AB[:, j] = 0.0
    if variant == "nan" and nb:
        AB[2 * w, nb // 2] = np.nan
    U = np.asfortranarray(rng.uniform(-1.0, 1.0, (nb, p)))
    C = np.asfortranarray(rng.uniform(-1.0, 1.0, (p, p)) + np.diag(np.full(p, 4.0 + p)))
    rhs = rng.uniform(-1.0, 1.0, nb + p)
    return AB, U, C, rhs


def failing_column(nb, variant):
    return {"zero_column": (2 * nb) // 3, "nan": nb // 2}[variant]


def dense(AB, w):
    """B as a dense array."""
    nb = AB.shape[1]
    B = np.zeros((nb, nb))
    for j in range(nb):
        lo, hi = max(0, j - w), min(nb, j + w + 1)
        B[lo:hi, j] = AB[2 * w + lo - j: 2 * w + hi - j, j]
    return B


def full_matrix(AB, U, C, w):
    nb, p = AB.shape[1], C.shape[0]
    K = np.zeros((nb + p, nb + p))
    K[:nb, :nb] = dense(AB, w)
    K[:nb, nb:], K[nb:, :nb], K[nb:, nb:] = U, U.T, C
    return K


# ---------------------------------------------------------------- the factorisation
def _row(flat, ldab, w, i, c0, c1):
    """Row i of B over the columns c0 ... c1 as a strided view of the flat band storage."""
    start = 2 * w + i + c0 * (ldab - 1)
    return flat[start: start + (c1 - c0) * (ldab - 1) + 1: ldab - 1]


def factor(AB, w, mutant=None):
    """dgbtf2's arithmetic in place on ``AB``: ``(ipiv, rec)``; ``rec[STATUS]`` 0, 1 (a zero pivot) or 3 (a column with an
    entry that is not finite), ``rec[COLUMN]`` the failing column."""
    ldab, nb = AB.shape
    assert ldab == 3 * w + 1 and AB.flags.f_contiguous
    flat = AB.reshape(-1, order="F")
    assert nb == 0 or np.shares_memory(flat, AB)
    ipiv = np.zeros(nb, dtype=np.int32)
    rec = np.array([0.0, -1.0, np.inf, 0.0, nb, w, 0.0, 0.0])
    pmin, pmax, swaps = np.inf, 0.0, 0.0
    reach = w if mutant == "narrow_u" else 2 * w
    for j in range(nb):
        km = min(w, nb - 1 - j)
        col = AB[2 * w: 2 * w + km + 1, j]
        if not np.all(np.isfinite(col)):
            rec[STATUS], rec[COLUMN] = 3.0, j
            return ipiv, rec
        mag = np.abs(col)
        jp = int(np.argmax(mag))
        if mutant == "tie_highest":
            jp = km - int(np.argmax(mag[::-1]))
        big = float(mag[jp])
        if big == 0.0:
            rec[STATUS], rec[COLUMN] = 1.0, j
            return ipiv, rec
        ipiv[j] = j + jp
        pmin, pmax = min(pmin, big), max(pmax, big)
        ju = min(j + reach, nb - 1)
        if jp:
            swaps += 1.0
            c0 = max(0, j + jp - w) if mutant == "swap_earlier_columns" else j
            a, b = _row(flat, ldab, w, j, c0, ju), _row(flat, ldab, w, j + jp, c0, ju)
            t = a.copy()
            a[:] = b
            b[:] = t
        if km:
            col = AB[2 * w + 1: 2 * w + km + 1, j]
            col[:] = col / AB[2 * w, j]
            if ju > j:
                u = _row(flat, ldab, w, j, j + 1, ju).copy()
                start = 2 * w + (j + 1) + (j + 1) * (ldab - 1)
                block = np.lib.stride_tricks.as_strided(flat[start:], shape=(km, ju - j), strides=(8, 8 * (ldab - 1)))
                if mutant == "fma":
                    for k in range(ju - j):
                        block[:, k] = cg._fma(-col, np.full(km, u[k]), block[:, k])
                else:
                    block -= np.outer(col, u)
        if (j + 1) % NB == 0 or j == nb - 1:      # the panel is complete: its extremes are committed
            rec[MIN_PIVOT], rec[MAX_PIVOT], rec[SWAPS] = pmin, pmax, swaps
    return ipiv, rec


def sweeps(AB, w, ipiv, Y, mutant=None):
    """The forward and backward sweeps in place on the columns of ``Y`` (nb, R)."""
    nb = AB.shape[1]
    for j in range(nb):
        km = min(w, nb - 1 - j)
        ip = int(ipiv[j])
        if ip != j and mutant != "no_forward_swap":
            Y[[j, ip]] = Y[[ip, j]]
        if km:
            Y[j + 1: j + km + 1] -= AB[2 * w + 1: 2 * w + km + 1, j][:, None] * Y[j][None, :]
    for k in range(nb - 1, -1, -1):
        Y[k] = Y[k] / AB[2 * w, k]
        lo = max(0, k - 2 * w)
        if k > lo:
            Y[lo:k] -= AB[2 * w + lo - k: 2 * w, k][:, None] * Y[k][None, :]


def border(U, C, Y, b_c, mutant=None):
    """``(x_C, status, k)``: the Schur complement of the border from the dots, its LU with partial pivoting, the solve."""
    nb, p = U.shape
    dots = np.zeros((p + 1, p))
    for r in range(p + 1):
        for a in range(p):
            terms = U[:, a] * Y[:, r]
            if mutant == "plain_border_dots":
                acc = 0.0
                for t in terms.tolist():
                    acc = acc + t
                dots[r, a] = acc
            else:
                dots[r, a] = cg.dot(terms)
    S = [[float(C[a, b] + dots[b, a]) if mutant == "border_sign" else float(C[a, b] - dots[b, a]) for b in range(p)] for a in range(p)]
    v = [float(b_c[a] - dots[p, a]) for a in range(p)]
    for k in range(p):
        mags = [abs(S[r][k]) if np.isfinite(S[r][k]) else np.inf for r in range(k, p)]
        big = max(mags)
        ip = k + mags.index(big)
        if not np.isfinite(big) or big == 0.0:
            return None, (2.0 if np.isfinite(big) else 3.0), k
        if ip != k:
            S[k], S[ip] = S[ip], S[k]
            v[k], v[ip] = v[ip], v[k]
        for r in range(k + 1, p):
            l = S[r][k] / S[k][k]
            S[r][k] = l
            for c in range(k + 1, p):
                pr = l * S[k][c]
                S[r][c] = S[r][c] - pr
            pr = l * v[k]
            v[r] = v[r] - pr
    for k in range(p - 1, -1, -1):
        e = v[k]
        for c in range(k + 1, p):
            pr = S[k][c] * v[c]
            e = e - pr
        v[k] = e / S[k][k]
    return np.array(v, dtype=np.float64), 0.0, -1


def solve_system(AB, U, C, rhs, mutant=None):
    """What ``pk_band_raw_dev`` computes: ``(AB factored, ipiv, x or None, rec)`` on copies; ``x`` in permuted order."""
    AB = np.array(AB, order="F")
    ldab, nb = AB.shape
    w, p = (ldab - 1) // 3, C.shape[0]
    ipiv, rec = factor(AB, w, mutant)
    rec[R_P] = p
    if rec[STATUS] != 0.0:
        return AB, ipiv, None, rec
    Y = np.empty((nb, p + 1), order="F")
    Y[:, :p], Y[:, p] = U, rhs[:nb]
    sweeps(AB, w, ipiv, Y, mutant)
    if p == 0:
        return AB, ipiv, Y[:, 0].copy(), rec
    x_c, status, k = border(U, C, Y, rhs[nb:], mutant)
    if status != 0.0:
        rec[STATUS], rec[COLUMN] = status, nb + k
        return AB, ipiv, None, rec
    x_b = Y[:, p].copy()
    for q in range(p):
        x_b = x_b - Y[:, q] * x_c[q]
    return AB, ipiv, np.concatenate((x_b, x_c)), rec


def emulate(ordering, hvals, jvals, s1, s2, rhs, mutant=None):
    """What ``pk_band_factor_dev`` and ``pk_band_solve_dev`` compute for a ``pockit_amd.band.BandOrdering``: ``(sol or None,
    rec)``, ``sol`` of n + m values in the caller's order."""
    band, U, C = ordering.assemble(hvals, jvals, s1, s2)
    _, _, x, rec = solve_system(band, U, C, ordering.permute_rhs(rhs), mutant)
    return (None if x is None else ordering.scatter(x)), rec
