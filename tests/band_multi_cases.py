"""The block solve of pockit_amd/csrc/pk_band.cpp -- k right-hand sides against one factorisation -- as NumPy, and the shapes it is
tested at.  A plain helper module, shared by tests/test_band_multi_cases_cpu.py (which tests this module),
tests/test_band_multi_cpu.py (the host stand-in's walk) and tests/test_gpu_band_multi.py (the kernels).

THE EMULATOR is ``solve_columns``: the single solve of tests/band_cases.py (``solve_system``, imported, not restated) applied
column by column.  That is the contract: column c of a block has the bits the single solve gives for column c alone.

``solve_block`` restates the block kernels' own walk -- one factorisation, p + k sweep vectors in one array, the (p + k) p dots
in one flat array, S formed and factored once with the interchanges and multipliers replayed per column, x_B per column, the
right-hand sides read at a stride -- so that the mistakes such a walk can make (MUTANTS) can be planted in it.  Without a mutant
it must give ``solve_columns``' bits; with each of them it must not."""
import numpy as np

import band_cases as bc
import cg_cases as cg

RHS_CAP = 64                                   # PK_BD_RHS_CAP
BLOCK, GRID_CAP = 256, 2048                    # PK_BLOCK, PK_LIB_GRID_CAP
NB_SHAPES = (0, 1, 33, 65, 2 * bc.NB + 1 + bc.W_CAP)
W_SHAPES = (0, 7, 33, bc.W_CAP)
P_SHAPES = (0, 1, bc.P_CAP)
K_SHAPES = (1, 2, 9, RHS_CAP)
GPU_NB_SHAPES = (1, 33, 65, 2 * bc.NB + 1 + bc.W_CAP)
LONG = (4500, 8, 1, RHS_CAP)                   # three pieces per dot
MUTANTS = ("previous_rhs", "dots_stride", "packed_stride", "first_xc", "one_trip")


def shapes(nbs=NB_SHAPES):
    return [(nb, w, p, k) for nb in nbs for w in W_SHAPES for p in P_SHAPES for k in K_SHAPES]


def block(nb, w, p, k, seed=0, gap=0, variant="plain"):
    """``(AB, U, C, R)``: ``bc.system``'s matrix and ``R`` of shape ``(k, nb + p + gap)``, full-mantissa right-hand sides in
    permuted order with NaN in the ``gap`` columns behind each."""
    AB, U, C, _ = bc.system(nb, w, p, seed, variant)
    rng = np.random.default_rng(7000 * seed + 31 * nb + 5 * w + 3 * p + k)
    R = np.full((k, nb + p + gap), np.nan)
    R[:, : nb + p] = rng.uniform(-1.0, 1.0, (k, nb + p))
    return AB, U, C, R


def solve_columns(AB, U, C, R):
    """THE EMULATOR: ``(AB factored, ipiv, X or None, rec)``; row c of ``X`` is ``bc.solve_system`` on right-hand side c alone
    (``R`` may carry a gap behind each row: only the first nb + p entries of a row are a right-hand side)."""
    N = AB.shape[1] + C.shape[0]
    out = [bc.solve_system(AB, U, C, R[c, :N]) for c in range(R.shape[0])]
    band, ipiv, x0, rec = out[0]
    if x0 is None:
        return band, ipiv, None, rec
    return band, ipiv, np.array([x for _, _, x, _ in out]).reshape(R.shape[0], N), rec


def solve_block(AB, U, C, R, mutant=None, grid_cap=GRID_CAP):
    """The block kernels' walk (module docstring): ``(AB factored, ipiv, X or None, rec)``."""
    AB = np.array(AB, order="F")
    ldab, nb = AB.shape
    w, p, k = (ldab - 1) // 3, C.shape[0], R.shape[0]
    N, stride = nb + p, R.shape[1]
    ipiv, rec = bc.factor(AB, w)
    rec[bc.R_P] = p
    if rec[bc.STATUS] != 0.0:
        return AB, ipiv, None, rec
    # prep: element e of [U | the k right-hand sides], PK_BLOCK elements per work item, the items in a stride loop
    flat = R.reshape(-1)
    read = N if mutant == "packed_stride" else stride
    Y = np.full((p + k) * nb, -77.0)
    b_c = np.full(k * p, -77.0)
    length = nb * p + k * N
    items = -(-length // BLOCK)
    done = min(items, grid_cap) if mutant == "one_trip" else items      # (the loop left after its first trip)
    for e in range(min(length, done * BLOCK)):
        if e < nb * p:
            Y[e] = U.reshape(-1, order="F")[e]
            continue
        c, pos = divmod(e - nb * p, N)
        src = c - 1 if mutant == "previous_rhs" and c > 0 else c
        v = flat[src * read + pos]
        if pos < nb:
            Y[nb * p + c * nb + pos] = v
        else:
            b_c[c * p + pos - nb] = v
    Ys = np.asfortranarray(Y.reshape((nb, p + k), order="F"))
    bc.sweeps(AB, w, ipiv, Ys)
    if p == 0:
        return AB, ipiv, np.ascontiguousarray(Ys.T), rec
    # the (p + k) p dots in one flat array
    dots = np.zeros((p + k + 1) * (p + 1))
    for r in range(p + k):
        for a in range(p):
            dots[r * p + a] = cg.dot(U[:, a] * Ys[:, r])
    ld = p + 1 if mutant == "dots_stride" else p
    # S and its LU once: the interchanges, the multipliers as they are formed
    S = [[float(C[a, b] - dots[b * ld + a]) for b in range(p)] for a in range(p)]
    piv, L = [0] * p, [[0.0] * p for _ in range(p)]
    for j in range(p):
        mags = [abs(S[r][j]) if np.isfinite(S[r][j]) else np.inf for r in range(j, p)]
        big = max(mags)
        if not np.isfinite(big) or big == 0.0:
            rec[bc.STATUS], rec[bc.COLUMN] = (2.0 if np.isfinite(big) else 3.0), nb + j
            return AB, ipiv, None, rec
        piv[j] = j + mags.index(big)
        if piv[j] != j:
            S[j], S[piv[j]] = S[piv[j]], S[j]
        for r in range(j + 1, p):
            l = S[r][j] / S[j][j]
            S[r][j] = L[r][j] = l
            for c in range(j + 1, p):
                pr = l * S[j][c]
                S[r][c] = S[r][c] - pr
    X = np.empty((k, N))
    for c in range(k):
        v = [float(b_c[c * p + a] - dots[(p + c) * ld + a]) for a in range(p)]
        for j in range(p):
            if piv[j] != j:
                v[j], v[piv[j]] = v[piv[j]], v[j]
            for r in range(j + 1, p):
                pr = L[r][j] * v[j]
                v[r] = v[r] - pr
        for j in range(p - 1, -1, -1):
            e = v[j]
            for q in range(j + 1, p):
                pr = S[j][q] * v[q]
                e = e - pr
            v[j] = e / S[j][j]
        X[c, nb:] = v
    for c in range(k):
        x_b = Ys[:, p + c].copy()
        x_c = X[0 if mutant == "first_xc" else c, nb:]
        for q in range(p):
            x_b = x_b - Ys[:, q] * x_c[q]
        X[c, :nb] = x_b
    return AB, ipiv, X, rec


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))
