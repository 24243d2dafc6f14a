"""The ordering and the assembly map of the bordered band LU on the device (``csrc/pk_band.cpp``).  Host
side, once per solve, no GPU needed.

``K = [[H + diag(s1), J^T], [J, -diag(s2)]]`` over the free variables (``v_lb != v_ub``) and all rows has ``N = nf + m`` unknowns:
the free variables in ascending order, then the rows.  ``BandOrdering`` permutes it symmetrically to ``[[B, U], [U^T, C]]``:

* THE BORDER RULE.  The degree of an unknown is the number of off-diagonal entries of its row of K's pattern.  An unknown whose
  degree exceeds ``max(64, N / 8)`` goes to the border (a free final time couples to every dynamic row); the border unknowns
  keep their ascending order and come last.  Deterministic: a function of the pattern alone.
* The other ``Nb = N - p`` unknowns are ordered by SciPy's ``reverse_cuthill_mckee`` (symmetric mode) on the pattern without the
  border; ``w`` is the largest ``|pos(i) - pos(j)|`` over its entries.
* ``w`` above ``max_width`` (default ``W_CAP`` = 192) or ``p`` above ``max_border`` (default ``P_CAP`` = 8) is a ``ValueError``:
  the caps are those of the kernels' static LDS.

Storage.  B in LAPACK's ``dgbtrf`` layout: ``kl = ku = w``, leading dimension ``ldab = 3 w + 1``, column-major, ``B(i, j)`` at
``AB[2 w + i - j, j]`` (the first w rows take the fill of pivoting); U is ``Nb x p`` and C is ``p x p``, column-major; only U
is stored, the block below the band part is its transpose.

THE ASSEMBLY MAP lists, destination by destination over ``[band | U | C]`` (in that storage order), at most two sources:
``map[2 d + k]`` is 0 (none), ``+(e + 1)`` (plus entry e) or ``-(e + 1)`` (minus entry e) of ``[hvals | jvals | s1 (n) | s2 (m)]``.
The sources of a slot are listed by ascending e -- the Hessian entry of a diagonal before its ``s1``.  A slot's value is
``0.0`` plus or minus its sources in that order (so a slot without a source is 0.0 and no slot is -0.0): what
``assemble`` states in NumPy and ``pk_bd_fill_k`` computes."""
from __future__ import annotations

import numpy as np

W_CAP, P_CAP = 192, 8      # PK_BD_W_CAP, PK_BD_P_CAP of csrc/pk_band.cpp


class BandOrdering:
    """Border, permutation, half-bandwidth and assembly map of K for the CSR maps ``map_j`` (m x n) and ``map_h`` (lower triangle,
    n x n) and the mask ``free`` of the variables that are not fixed.

    ``N, nb, p, w, ldab``; ``pos[u]``: the permuted position of unknown u; ``order[k]``: the index in a caller's vector of n + m
    values (variables, then rows) of the unknown at permuted position k; ``map``: int32, two codes per stored slot; ``dests``."""

    def __init__(self, map_j, map_h, free, *, max_width=None, max_border=None):
        import scipy.sparse as sp
        from scipy.sparse.csgraph import reverse_cuthill_mckee

        free = np.asarray(free, dtype=bool)
        n, m = len(free), map_j.shape[0]
        if map_j.shape[1] != n or map_h.shape != (n, n):
            raise ValueError("the maps do not fit the mask of free variables")
        max_width = W_CAP if max_width is None else int(max_width)
        max_border = P_CAP if max_border is None else int(max_border)
        self.n, self.m = n, m
        col_of = np.cumsum(free) - 1
        idx_free = np.flatnonzero(free)
        nf = len(idx_free)
        N = self.N = nf + m
        # ---- the entries of K with their sources, as DirectKkt lists them
        hs = map_h.symmetric()
        h_rows = np.repeat(np.arange(n), np.diff(hs.indptr))
        h_cols, h_src = hs.indices.astype(np.int64), hs.src.astype(np.int64)
        keep = free[h_rows] & free[h_cols]
        j_rows = np.repeat(np.arange(m), np.diff(map_j.indptr))
        j_cols = map_j.indices.astype(np.int64)
        j_keep = free[j_cols]
        off_j, off_s1, off_s2 = map_h.nnz, map_h.nnz + map_j.nnz, map_h.nnz + map_j.nnz + n
        self.sources = off_s2 + m
        jr, jc, je = nf + j_rows[j_keep], col_of[j_cols[j_keep]], off_j + np.flatnonzero(j_keep)
        rows = np.concatenate((col_of[h_rows[keep]], col_of[idx_free], jr, jc, nf + np.arange(m))).astype(np.int64)
        cols = np.concatenate((col_of[h_cols[keep]], col_of[idx_free], jc, jr, nf + np.arange(m))).astype(np.int64)
        src = np.concatenate((h_src[keep], off_s1 + idx_free, je, je, off_s2 + np.arange(m))).astype(np.int64)
        sign = np.concatenate((np.ones(len(rows) - m, dtype=np.int64), -np.ones(m, dtype=np.int64)))
        # ---- the border: degree above max(64, N / 8)
        pattern = sp.csr_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(N, N))
        pattern.sum_duplicates()
        offdiag = pattern.copy()
        offdiag.setdiag(0)
        offdiag.eliminate_zeros()
        degree = np.diff(offdiag.indptr)
        border = np.flatnonzero(degree > max(64.0, N / 8.0))
        p = self.p = len(border)
        if p > max_border:
            raise ValueError(f"{p} dense unknowns exceed the border's cap of {max_border}: use linear_solver=\"direct\" for this model")
        inner = np.setdiff1d(np.arange(N), border)
        nb = self.nb = len(inner)
        # ---- RCM on the band part
        sub = offdiag[inner][:, inner].tocsr()
        rcm = np.asarray(reverse_cuthill_mckee(sub, symmetric_mode=True), dtype=np.int64) if nb else np.zeros(0, dtype=np.int64)
        inv = np.concatenate((inner[rcm], border)).astype(np.int64)      # the unknown at permuted position k
        pos = np.empty(N, dtype=np.int64)
        pos[inv] = np.arange(N)
        self.pos, self.inv = pos, inv
        pr, pc = pos[rows], pos[cols]
        in_band = (pr < nb) & (pc < nb)
        w = self.w = int(np.abs(pr[in_band] - pc[in_band]).max()) if in_band.any() else 0
        if w > max_width:
            raise ValueError(f"half-bandwidth {w} exceeds the cap of {max_width}: use linear_solver=\"direct\" for this model")
        caller = np.concatenate((idx_free, n + np.arange(m)))
        self.order = caller[inv].astype(np.int32)
        # ---- the assembly map, destination by destination
        ldab = self.ldab = 3 * w + 1
        base_u, base_c = ldab * nb, ldab * nb + nb * p
        self.dests = base_c + p * p
        if 2 * self.dests > np.iinfo(np.int32).max:
            raise ValueError("the band storage does not fit 32-bit positions: use linear_solver=\"direct\" for this model")
        dest = np.full(len(rows), -1, dtype=np.int64)
        dest[in_band] = (2 * w + pr[in_band] - pc[in_band]) + pc[in_band] * ldab
        in_u = (pr < nb) & (pc >= nb)
        dest[in_u] = base_u + (pc[in_u] - nb) * nb + pr[in_u]
        in_c = (pr >= nb) & (pc >= nb)
        dest[in_c] = base_c + (pr[in_c] - nb) + (pc[in_c] - nb) * p
        live = dest >= 0                                   # (the block below the band part is U's transpose: not stored)
        dest, code = dest[live], (sign * (src + 1))[live]
        by = np.lexsort((src[live], dest))
        dest, code = dest[by], code[by]
        first = np.concatenate(([True], dest[1:] != dest[:-1])) if len(dest) else np.zeros(0, dtype=bool)
        rank = np.arange(len(dest)) - np.maximum.accumulate(np.where(first, np.arange(len(dest)), 0)) if len(dest) else np.zeros(0, dtype=np.int64)
        if len(rank) and rank.max() > 1:
            raise ValueError("a slot of K with more than two sources")
        self.map = np.zeros(2 * self.dests, dtype=np.int32)
        self.map[2 * dest + rank] = code

    # ---- the NumPy statement of the map
    def assemble(self, hvals, jvals, s1, s2):
        """``(band, U, C)``: band storage ``(ldab, nb)``, U ``(nb, p)`` and C ``(p, p)``, all Fortran-ordered."""
        vals = np.concatenate([np.asarray(a, dtype=np.float64) for a in (hvals, jvals, s1, s2)])
        if len(vals) != self.sources:
            raise ValueError(f"[hvals | jvals | s1 | s2] must have {self.sources} values")
        acc = np.zeros(self.dests)
        for k in range(2):
            code = self.map[k::2].astype(np.int64)
            plus, minus = code > 0, code < 0
            acc[plus] = acc[plus] + vals[code[plus] - 1]
            acc[minus] = acc[minus] - vals[-code[minus] - 1]
        nb, p, ldab = self.nb, self.p, self.ldab
        band = acc[: ldab * nb].reshape((ldab, nb), order="F")
        U = acc[ldab * nb: ldab * nb + nb * p].reshape((nb, p), order="F")
        C = acc[ldab * nb + nb * p:].reshape((p, p), order="F")
        return band, U, C

    def to_dense(self, band, U, C):
        """The permuted K as a dense (N, N) array (for tests)."""
        nb, p, w = self.nb, self.p, self.w
        K = np.zeros((self.N, self.N))
        for j in range(nb):
            lo, hi = max(0, j - w), min(nb, j + w + 1)
            K[lo:hi, j] = band[2 * w + lo - j: 2 * w + hi - j, j]
        K[:nb, nb:] = U
        K[nb:, :nb] = U.T
        K[nb:, nb:] = C
        return K

    def permute_rhs(self, rhs):
        """The caller's vector of n + m values in permuted order."""
        return np.asarray(rhs, dtype=np.float64)[self.order]

    def scatter(self, x):
        """The permuted solution in the caller's order; fixed variables get 0.0."""
        out = np.zeros(self.n + self.m)
        out[self.order] = x
        return out
