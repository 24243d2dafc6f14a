"""Triplet list -> CSR map (host side of the device-resident CSR hand-off).

The NLP callbacks return values in the reference's triplet order (duplicates included, systembase.py:671-693,
811-835).  A GPU linear solver wants CSR.  The (row, col) sort is a property of the mesh, so it is done once
here; per iterate the device only gathers (``pk_csr``): ``csr[p] = sum(triplets[perm[seg[p]:seg[p+1]]])``.

``CsrOperator``: the structures of the products ``J v``, ``J^T y``, ``H v`` on those values where they lie
(``csrc/pk_ops.cpp``), built from a map: the matrix itself, its transpose and the symmetric completion of a lower triangle.
The reductions over their entries (``csrc/pk_reduce.cpp``: row norms, weighted diagonals) walk the same structures; the diagonal
of H reads ``CsrMap.diagonal_src``.
"""
from __future__ import annotations

import numpy as np


class CsrMap:
    """CSR structure of a triplet pattern plus the gather map that fills its values.

    ``indptr`` (n_rows + 1), ``indices`` (nnz): the CSR structure, columns ascending within a row;
    ``perm`` (n_triplets): triplet indices in (row, col) order, ties in triplet order (stable: repeated
    entries are summed in the order the reference lists them); ``seg`` (nnz + 1): runs of ``perm`` per CSR
    entry, ``None`` when no entry repeats."""

    def __init__(self, rows, cols, shape):
        rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        n_rows, n_cols = (int(v) for v in shape)
        if rows.shape != cols.shape or rows.ndim != 1:
            raise ValueError("rows and cols must be one-dimensional arrays of the same length")
        if len(rows) == 0:
            raise ValueError("empty pattern")
        if len(rows) > np.iinfo(np.int32).max:
            raise ValueError("pattern too large for 32-bit indices")
        if rows.min() < 0 or rows.max() >= n_rows or cols.min() < 0 or cols.max() >= n_cols:
            raise ValueError("triplet index outside the matrix")
        key = rows * n_cols + cols
        order = np.argsort(key, kind="stable")
        sorted_key = key[order]
        first = np.concatenate(([True], sorted_key[1:] != sorted_key[:-1]))
        starts = np.flatnonzero(first)
        unique_key = sorted_key[starts]
        self.shape = (n_rows, n_cols)
        self.n_triplets = len(rows)
        self.nnz = len(starts)
        self.perm = order.astype(np.int32)
        self.seg = None if self.nnz == self.n_triplets else np.concatenate((starts, [len(rows)])).astype(np.int32)
        self.indices = (unique_key % n_cols).astype(np.int32)
        self.indptr = np.searchsorted(unique_key // n_cols, np.arange(n_rows + 1)).astype(np.int32)

    def gather(self, triplet_values):
        """Host execution of the gather (what ``pk_csr`` does on the device, up to the association of the sums
        inside a run); used by the tests."""
        v = np.asarray(triplet_values, dtype=np.float64)[self.perm]
        if self.seg is None:
            return v
        out = np.zeros(self.nnz)
        return np.add.reduceat(v, self.seg[:-1], out=out) if len(v) else out

    def to_scipy(self, values):
        import scipy.sparse

        return scipy.sparse.csr_array((np.asarray(values), self.indices, self.indptr), shape=self.shape)

    # ---- operator structures of the device-side products (csrc/pk_ops.cpp): J . v, J^T . y, H . v
    def operator(self):
        """The matrix itself as a ``CsrOperator``: entry ``e`` takes ``values[e]``."""
        return CsrOperator(self.shape, self.indptr, self.indices, None)

    def transposed(self):
        """CSR of the transpose; ``src`` points into this map's values (nothing is copied per iterate)."""
        n_rows, n_cols = self.shape
        rows = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(self.indptr))
        order = np.argsort(self.indices, kind="stable")      # by column; rows stay ascending within one
        indptr = np.searchsorted(self.indices[order], np.arange(n_cols + 1))
        return CsrOperator((n_cols, n_rows), indptr, rows[order], order)

    def symmetric(self):
        """For a lower-triangular map: the full symmetric pattern ``L + L^T - diag(L)``.  An off-diagonal entry is
        listed twice with the same ``src``, a diagonal entry once."""
        n_rows, n_cols = self.shape
        if n_rows != n_cols:
            raise ValueError("symmetric(): the map is not square")
        rows = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(self.indptr))
        cols = self.indices.astype(np.int64)
        if np.any(cols > rows):
            raise ValueError("symmetric(): the map has an entry above the diagonal")
        off = np.flatnonzero(cols < rows)
        r, c = np.concatenate((rows, cols[off])), np.concatenate((cols, rows[off]))
        src = np.concatenate((np.arange(self.nnz, dtype=np.int64), off))
        order = np.argsort(r * n_cols + c, kind="stable")      # (no position repeats: L has one entry per position)
        indptr = np.searchsorted(r[order], np.arange(n_rows + 1))
        return CsrOperator(self.shape, indptr, c[order], src[order])

    def diagonal_src(self):
        """For a lower-triangular map: per row the position of its diagonal entry in this map's values, -1 where the row has
        none (int32, ``n`` entries).  Columns ascend and never exceed the row, so the diagonal entry is the last entry of a row
        whose column equals the row.  What ``pk_set_operator_diagonal`` takes."""
        n_rows, n_cols = self.shape
        if n_rows != n_cols:
            raise ValueError("diagonal_src(): the map is not square")
        rows = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(self.indptr))
        if np.any(self.indices > rows):
            raise ValueError("diagonal_src(): the map has an entry above the diagonal")
        pos = np.full(n_rows, -1, dtype=np.int32)
        last = self.indptr[1:].astype(np.int64) - 1
        live = np.flatnonzero(np.diff(self.indptr) > 0)
        hit = live[self.indices[last[live]] == live]
        pos[hit] = last[hit]
        return pos


class CsrOperator:
    """CSR structure of a matrix whose entries are taken from the CSR value array of a ``CsrMap``: entry ``e`` has the value
    ``values[src[e]]`` (``src`` None: ``values[e]``).  ``indptr`` (rows + 1), ``indices`` and ``src`` are int32, columns
    ascending within a row.  What ``pk_set_csr_operator`` takes."""

    def __init__(self, shape, indptr, indices, src):
        self.shape = (int(shape[0]), int(shape[1]))
        if len(indices) > np.iinfo(np.int32).max:
            raise ValueError("pattern too large for 32-bit indices")
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int32)
        self.indices = np.ascontiguousarray(indices, dtype=np.int32)
        self.src = None if src is None else np.ascontiguousarray(src, dtype=np.int32)
        self.nnz = len(self.indices)

    def to_scipy(self, values):
        import scipy.sparse

        v = np.asarray(values)
        return scipy.sparse.csr_array((v if self.src is None else v[self.src], self.indices, self.indptr), shape=self.shape)
