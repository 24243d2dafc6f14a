"""Inputs, references and the checker for the BLOCK form of the operator kernels (``pk_op_rows_k`` / ``pk_op_long_k``,
pockit_amd/csrc/pk_ops.cpp), built on tests/sparse_cases.py, which stays as it is.  A plain helper module, shared by
tests/test_sparse_block_cases_cpu.py (which tests this module) and tests/test_gpu_csr_operator_block.py (which tests the kernels).

The contract of a block product is per column: column j of ``Y = A V (+ Add)`` has exactly the bits of the single-vector
product with column j of ``V`` (and of ``Add``).  So the emulator is ``sparse_cases.emulate_operator`` applied per column, the
exact reference is its ``math.fsum`` per (row, column), and the bound is its derived bound gamma(L + 1) * (sum|t| + |add|) per
(row, column): nothing new is transcribed and no new number appears.

Inputs: for an ``OperatorCase`` k columns drawn with ``sparse_cases._unit`` (24-bit mantissas: every product exact) and k
``add`` columns of each row's own scale, +-[1, 4) * 2**s.

``walk_block`` is a block walk written in NumPy the way the kernels are laid out -- chunks of at most KMAX columns, one plane of
products per column, ``partial[slot, column]`` -- with one deliberate mistake per name in BLOCK_MUTANTS; the CPU test requires the
checker to catch each.
"""
import copy

import numpy as np

import sparse_cases as sc

KMAX = 8                    # PK_OP_KMAX
BLOCK_MUTANTS = ("plane", "shared_partial", "last_chunk")


def block_inputs(case, k, seed):
    """(V, Add): (n_cols, k) and (n_rows, k), C order."""
    rng = np.random.default_rng(seed)
    V = sc._unit(rng, case.n_cols * k).reshape(case.n_cols, k)
    rows5 = np.arange(case.n_rows) % 5
    scale = np.ldexp(1.0, np.asarray(sc.BUCKETS)[rows5])[:, None]
    Add = rng.uniform(1.0, 4.0, (case.n_rows, k)) * rng.choice([-1.0, 1.0], (case.n_rows, k)) * scale
    return np.ascontiguousarray(V), np.ascontiguousarray(Add)


def column_case(case, V, Add, j):
    """The single-vector case of column j: ``case`` with v = V[:, j] and add = Add[:, j] (its cached reference dropped)."""
    c = copy.copy(case)
    c.__dict__.pop("reference", None)
    c.v, c.add = np.ascontiguousarray(V[:, j]), np.ascontiguousarray(Add[:, j])
    return c


class BlockExpectation:
    """Per (row, column) of one (case, V, Add): the emulated bits and (ref, bound, scale), with and without Add.  Computed once."""

    def __init__(self, case, V, Add):
        self.case, self.V, self.Add, self.k = case, V, Add, V.shape[1]
        cols = [column_case(case, V, Add, j) for j in range(self.k)]
        self.emulated, self.ref, self.bound, self.scale = {}, {}, {}, {}
        for with_add in (False, True):
            self.emulated[with_add] = np.stack([c.emulated(with_add) for c in cols], axis=1)
            ref, bound, scale = zip(*(c.reference[with_add] for c in cols))
            self.ref[with_add], self.bound[with_add], self.scale[with_add] = (np.stack(x, axis=1) for x in (ref, bound, scale))

    def problems(self, got, with_add):
        """What is wrong with ``got`` (n_rows, k): a list of strings, empty when every column holds."""
        out = []
        got = np.asarray(got, dtype=np.float64)
        if got.shape != (self.case.n_rows, self.k):
            return [f"shape {got.shape}"]
        ref, bound, emulated = self.ref[with_add], self.bound[with_add], self.emulated[with_add]
        for j in range(self.k):
            col = np.ascontiguousarray(got[:, j])
            unwritten = np.flatnonzero(np.isnan(col))
            if len(unwritten):
                out.append(f"column {j}: rows {unwritten[:8]} were not written")
                continue
            bad = sc.failures(col, ref[:, j], bound[:, j])
            if len(bad):
                out.append(f"column {j}: {len(bad)} rows miss the bound, first {bad[:8]}")
            exact = bound[:, j] == 0.0
            if not sc.same_bits(col[exact], ref[exact, j]):
                out.append(f"column {j}: a row that must be exact is not")
            if not sc.same_bits(col, emulated[:, j]):
                differ = np.flatnonzero(col.view(np.uint64) != np.ascontiguousarray(emulated[:, j]).view(np.uint64))
                out.append(f"column {j}: {len(differ)} rows differ in bits from the single-vector association, first {differ[:8]}")
        return out


def walk_block(case, V, Add=None, mutant=None):
    """Y as the block kernels compute it, laid out as they are: NaN where no thread writes."""
    assert mutant is None or mutant in BLOCK_MUTANTS
    k = V.shape[1]
    indptr = case.indptr.astype(np.int64)
    blocks, longs, n_slots = sc.row_blocks(case.indptr)
    vals = case.vals[np.arange(case.nnz) if case.src is None else case.src]
    Y = np.full((case.n_rows, k), np.nan)
    stream = [b for b in blocks if b[3] >= 0]
    pieces = [b for b in blocks if b[3] < 0]
    chunks = [(c0, min(KMAX, k - c0)) for c0 in range(0, k, KMAX)]
    if mutant == "last_chunk" and len(chunks) > 1:
        chunks = chunks[:-1]
    for c0, kc in chunks:
        planes = vals[:, None] * V[case.indices, c0: c0 + kc]            # plane c: the products with column c0 + c
        read = (np.arange(kc) + 1) % kc if mutant == "plane" else np.arange(kc)
        if stream:
            rows = np.concatenate([np.arange(b[2], b[2] + b[3]) for b in stream])
            lo, hi = indptr[rows], indptr[rows + 1]
            s = np.zeros((len(rows), kc))
            for i in range(int((hi - lo).max())):
                m = lo + i < hi
                s[m] = s[m] + planes[lo[m] + i][:, read]
            Y[rows, c0: c0 + kc] = s if Add is None else s + Add[rows, c0: c0 + kc]
        if pieces:
            a = np.zeros((len(pieces), sc.BLOCK, kc))
            for j, (e, cnt, _, _) in enumerate(pieces):
                a[j, :cnt] = planes[e: e + cnt]
            sums = sc._tree(a, None)                                        # (pieces, kc)
            slots = [b[2] for b in pieces]
            partial = np.full((n_slots, kc), np.nan)
            partial[slots] = sums[:, [kc - 1] * kc] if mutant == "shared_partial" else sums      # (one slot: the last writer's)
            row, first, cnt = (np.array(x, dtype=np.int64) for x in zip(*longs))
            a = np.zeros((len(longs), sc.BLOCK, kc))
            t = np.arange(sc.BLOCK)
            for j in range(-(-int(cnt.max()) // sc.BLOCK)):
                at = t[None, :] + sc.BLOCK * j
                held = at < cnt[:, None]
                a = a + np.where(held[:, :, None], partial[np.minimum(first[:, None] + at, n_slots - 1)], 0.0)
            total = sc._tree(a, None)
            Y[row, c0: c0 + kc] = total if Add is None else total + Add[row, c0: c0 + kc]
    return Y
