"""Inputs, exact references and bit-for-bit emulators for the three model-independent sparse kernels: ``pk_op_rows`` and
``pk_op_long`` (pockit_amd/csrc/pk_ops.cpp) and ``pk_csr`` (``kernel_csr`` in pk_kernels.hip.h).  A plain helper module, shared
by tests/test_sparse_cases_cpu.py (which tests this module) and tests/test_gpu_sparse_kernels.py (which tests the kernels).

Inputs that make a lost term visible.  ``vals[i] = +-[1, 2) * 2**s`` with ``s`` from the five buckets {-40, -20, 0, 20, 40},
``v[j] = +-[1, 2)``, both with 24-bit mantissas, so every product is exact in fp64.  Row ``r`` takes its values only from
bucket ``r mod 5``: every term of a row is within a factor of 4 of every other (|t| in [1, 4) * 2**s), while rows differ by
up to 2**80.  ``add[r]`` is a full-precision double of the row's own scale, +-[1, 4) * 2**s.

The exact reference is ``math.fsum`` over a row's exact products (and ``add[row]``): the correctly rounded sum.

The bound is derived, not measured.  Any order of L - 1 additions of L exact terms plus one more addition for ``add`` errs by
at most gamma_L * (sum|t| + |add|), gamma_k = k u / (1 - k u), u = 2**-53 (Higham, Accuracy and Stability of Numerical
Algorithms, section 4.2); the reference's own rounding is one more u, hence gamma_{L+1}.  An empty row must equal ``add[row]``
(or 0.0) exactly, a one-entry row without ``add`` its term exactly.  For the gather a run of ``len`` triplets is ``len - 1``
additions: gamma_{len-1} * sum|t| per entry, runs of one exact.

The emulators follow the association the code documents: a stream row's products added sequentially in entry order; a piece
block's 256 zero-padded slots reduced by the tree of widths 128, 64 ... 1; a long row's thread t adding partial[first + t],
partial[first + t + 256] ... in ascending order, the same tree, then + add; a run's triplets added sequentially in run order.
None of the kernels can contract to an FMA (the products go to LDS before any addition; the gather only adds), so the device
must match the emulator in every bit.  ``mutant`` names one deliberate mistake each (MUTANTS): the CPU test requires the
checker to catch every one of them.
"""
import functools
import math

import numpy as np

U = 2.0 ** -53
BLOCK = 256                 # PK_BLOCK
OP_GRID_CAP = 2048          # PK_LIB_GRID_CAP of csrc/pk_libkernel.h
CSR_GRID_CAP = 4096         # the workgroups pk_csr is launched with at most (K_CSR in csrc/pk_launch.h)
BUCKETS = (-40, -20, 0, 20, 40)

# context -> model and the sizes the cases are built for (both test files assert them against the plan)
CONTEXTS = {
    "A": dict(model=("brachistochrone", "radau", 3, 4), n=53, m=36, nnz_j=329, nnz_h=46, trip_j=437),
    "B": dict(model=("brachistochrone", "radau", 60, 5), n=1205, m=900, nnz_j=10177, nnz_h=1198, trip_j=13777),
    "C": dict(model=("brachistochrone", "radau", 200, 8), n=6405, m=4800, nnz_j=78365, nnz_h=6398, trip_j=111965),
}
# The context of the gather cases past pk_csr's grid cap: the smallest uniform mesh of the full-size CSR test's model whose
# Jacobian has more than CSR_GRID_CAP * BLOCK + 512 triplets (2 775 intervals give 1 048 875).  Kept out of CONTEXTS: it has
# no operator cases.
CAP_CONTEXT = dict(model=("planar_quadrotor", "radau", 2776, 6), n=133256, m=133248, nnz_j=1049253, trip_j=1049253)
GATHER_CAP_MUTANT = "second_trip_dropped"      # the stride loops of pk_csr left after their first trip
OPERATOR_MUTANTS = ("slot", "row_boundary", "tree_stops_at_2", "strided_first_trip", "long_first_2048")
GATHER_MUTANTS = ("remainder",)
MUTANTS = OPERATOR_MUTANTS + GATHER_MUTANTS


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def op_shape(ctx, op):
    """(n_rows, n_cols, n_unique) of operator ``op`` (0: J, 1: J^T, 2: H symmetric) in a context."""
    c = CONTEXTS[ctx]
    return {0: (c["m"], c["n"], c["nnz_j"]), 1: (c["n"], c["m"], c["nnz_j"]), 2: (c["n"], c["n"], c["nnz_h"])}[op]


def _unit(rng, size):
    """+-[1, 2) with a 24-bit mantissa."""
    x = rng.integers(2 ** 23, 2 ** 24, size).astype(np.float64) / 2.0 ** 23
    x = np.float32(x).astype(np.float64)
    assert np.all((x >= 1.0) & (x < 2.0))
    return x * rng.choice([-1.0, 1.0], size)


def _scaled(rng, bucket):
    bucket = np.asarray(bucket)
    return np.ldexp(_unit(rng, len(bucket)), np.asarray(BUCKETS)[bucket])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def failures(got, ref, bound):
    """Indices that miss |got - ref| <= bound (a NaN misses it)."""
    return np.flatnonzero(~(np.abs(np.asarray(got, dtype=np.float64) - ref) <= bound))


def worst_units(got, ref, scale):
    """max |got - ref| in units of u * scale over the entries with a scale; 0.0 when there is none."""
    live = scale > 0
    return float(np.max(np.abs(np.asarray(got)[live] - ref[live]) / (U * scale[live]))) if np.any(live) else 0.0


# ---------------------------------------------------------------- the block cutter, transcribed from pk_op_row_blocks
def row_blocks(indptr):
    """(blocks, longs, n_slots): blocks are (e0, count, row0, n_rows) with n_rows = -1 for a piece block (row0 = its slot);
    longs are (row, first slot, pieces)."""
    indptr = [int(x) for x in indptr]
    n_rows = len(indptr) - 1
    blocks, longs, slots, r = [], [], 0, 0
    while r < n_rows:
        e0, length = indptr[r], indptr[r + 1] - indptr[r]
        if length > BLOCK:
            pieces = (length + BLOCK - 1) // BLOCK
            longs.append((r, slots, pieces))
            for p in range(pieces):
                blocks.append((e0 + p * BLOCK, min(BLOCK, length - p * BLOCK), slots + p, -1))
            slots += pieces
            r += 1
        else:
            r0 = r
            while r < n_rows and r - r0 < BLOCK and indptr[r + 1] - indptr[r] <= BLOCK and indptr[r + 1] - e0 <= BLOCK:
                r += 1
            blocks.append((e0, indptr[r] - e0, r0, r - r0))
    return blocks, longs, slots


# ---------------------------------------------------------------- operator cases
class OperatorCase:
    """A CSR structure for operator ``op`` of a context from a list of row lengths (padded with empty rows), with inputs,
    exact reference and bounds.  Columns ascend and are distinct while a row fits n_cols and cycle when it is longer (the
    product is then the sum over the listed entries).  ``expect_stream``: the entry counts of the non-empty stream blocks in
    order, where they are stated by hand; pieces and long rows follow from the lengths."""

    def __init__(self, ctx, name, op, lengths, seed, with_src=True, expect_stream=None):
        self.ctx, self.name, self.op = ctx, name, op
        self.id = f"{ctx}-{name}-op{op}"
        self.n_rows, self.n_cols, self.n_unique = op_shape(ctx, op)
        assert len(lengths) <= self.n_rows, self.id
        rng = np.random.default_rng(seed)
        self.lengths = np.zeros(self.n_rows, dtype=np.int64)
        self.lengths[: len(lengths)] = lengths
        self.nnz = int(self.lengths.sum())
        assert 0 < self.nnz < 2 ** 31
        self.indptr = np.concatenate(([0], np.cumsum(self.lengths))).astype(np.int32)
        cols = []
        for length in self.lengths[self.lengths > 0]:
            if length <= self.n_cols:
                cols.append(np.sort(rng.choice(self.n_cols, int(length), replace=False)))
            else:
                cols.append((int(rng.integers(self.n_cols)) + np.arange(length)) % self.n_cols)
        self.indices = np.concatenate(cols).astype(np.int32)
        self.row_of = np.repeat(np.arange(self.n_rows), self.lengths)
        if with_src:
            bucket = np.arange(self.n_unique) % 5                      # value i lies in bucket i mod 5
            want = self.row_of % 5
            count = (self.n_unique - want + 4) // 5                    # values of bucket b: b, b + 5, ...
            self.src = (want + 5 * rng.integers(0, count)).astype(np.int32)
            assert self.src.max() < self.n_unique and np.array_equal(bucket[self.src], want)
        else:
            assert self.nnz == self.n_unique, self.id                 # entry e takes vals[e]
            bucket, self.src = self.row_of % 5, None
        self.vals = _scaled(rng, bucket)
        self.v = _unit(rng, self.n_cols)
        rows5 = np.arange(self.n_rows) % 5
        self.add = rng.uniform(1.0, 4.0, self.n_rows) * rng.choice([-1.0, 1.0], self.n_rows) * np.ldexp(1.0, np.asarray(BUCKETS)[rows5])
        self.expect_stream = expect_stream
        self.expect_pieces = int(sum(-(-int(n) // BLOCK) for n in self.lengths if n > BLOCK))
        self.expect_longs = int((self.lengths > BLOCK).sum())

    def products(self):
        """The exact products, in entry order (24-bit by 24-bit mantissas: no rounding)."""
        return self.vals[np.arange(self.nnz) if self.src is None else self.src] * self.v[self.indices]

    @functools.cached_property
    def reference(self):
        """{with_add: (ref, bound, scale)} per row: ref the correctly rounded sum, scale = sum|t| (+ |add|)."""
        p = self.products().tolist()
        ref = {False: np.zeros(self.n_rows), True: np.zeros(self.n_rows)}
        sabs = np.zeros(self.n_rows)
        for r in range(self.n_rows):
            t = p[self.indptr[r]: self.indptr[r + 1]]
            ref[False][r] = math.fsum(t)
            ref[True][r] = math.fsum(t + [float(self.add[r])])
            sabs[r] = math.fsum(abs(x) for x in t)
        out = {}
        for with_add in (False, True):
            scale = sabs + np.abs(self.add) if with_add else sabs
            bound = gamma(self.lengths + 1) * scale
            bound[self.lengths == 0] = 0.0                             # add[row], or 0.0, exactly
            if not with_add:
                bound[self.lengths == 1] = 0.0                         # the term exactly
            out[with_add] = (ref[with_add], bound, scale)
        return out

    def emulated(self, with_add, mutant=None):
        return emulate_operator(self, self.add if with_add else None, mutant)


def _tree(a, mutant):
    """The fixed tree over the 256 slots of every row of ``a``: s[t] += s[t + w] for t < w, w = 128, 64 ... 1."""
    w = BLOCK // 2
    while w >= (2 if mutant == "tree_stops_at_2" else 1):
        a[:, :w] += a[:, w: 2 * w]
        w //= 2
    return a[:, 0].copy()


def emulate_operator(case, add=None, mutant=None):
    """y as pk_op_rows and pk_op_long compute it, bit for bit; NaN where no thread writes."""
    assert mutant is None or mutant in OPERATOR_MUTANTS
    indptr, p = case.indptr.astype(np.int64), case.products()
    blocks, longs, n_slots = row_blocks(case.indptr)
    y = np.full(case.n_rows, np.nan)
    stream = [b for b in blocks if b[3] >= 0]
    rows = np.concatenate([np.arange(b[2], b[2] + b[3]) for b in stream]) if stream else np.zeros(0, dtype=np.int64)
    if len(rows):
        e0 = np.repeat([b[0] for b in stream], [b[3] for b in stream])
        count = np.repeat([b[1] for b in stream], [b[3] for b in stream])
        lo, hi = indptr[rows] - e0, indptr[rows + 1] - e0
        if mutant == "row_boundary":
            hi = hi + 1
        s = np.zeros(len(rows))
        for k in range(int((hi - lo).max())):
            m = lo + k < hi
            slot = lo[m] + k                    # the slot thread r reads; it holds product i (0.0 beyond the block's count)
            if mutant == "slot":                # written at i + i / 32, read unpadded: the layouts alias
                i, held = slot - slot // 33, slot % 33 != 32
            else:
                i, held = slot, np.ones(len(slot), dtype=bool)
            held &= i < count[m]
            s[m] = s[m] + np.where(held, p[np.minimum(e0[m] + i, len(p) - 1)], 0.0)
        y[rows] = s if add is None else s + add[rows]
    pieces = [b for b in blocks if b[3] < 0]
    if pieces:
        a = np.zeros((len(pieces), BLOCK))
        for j, (e, cnt, _, _) in enumerate(pieces):
            a[j, :cnt] = p[e: e + cnt]
        partial = np.full(n_slots, np.nan)
        partial[[b[2] for b in pieces]] = _tree(a, mutant)
        served = longs[:OP_GRID_CAP] if mutant == "long_first_2048" else longs
        row, first, cnt = (np.array(x, dtype=np.int64) for x in zip(*served))
        a = np.zeros((len(served), BLOCK))
        t = np.arange(BLOCK)
        for j in range(1 if mutant == "strided_first_trip" else -(-int(cnt.max()) // BLOCK)):
            k = t[None, :] + BLOCK * j
            held = k < cnt[:, None]
            a = a + np.where(held, partial[np.minimum(first[:, None] + k, n_slots - 1)], 0.0)
        total = _tree(a, mutant)
        y[row] = total if add is None else total + add[row]
    return y


def _random_lengths(rng, total, n_rows, cap):
    lengths = np.zeros(n_rows, dtype=np.int64)
    for _ in range(total):
        while True:
            r = int(rng.integers(n_rows))
            if lengths[r] < cap:
                lengths[r] += 1
                break
    return lengths


@functools.lru_cache(maxsize=None)
def operator_cases():
    """Every operator case of the GPU file, for the ops whose row count fits."""
    cases = []

    def put(ctx, name, lengths, ops=(0, 1, 2), **kw):
        for op in ops:
            if len(lengths) <= op_shape(ctx, op)[0]:
                cases.append(OperatorCase(ctx, name, op, lengths, seed=1000 + len(cases), **kw))

    # context A
    put("A", "edges", [0, 1, 255, 256, 257, 512, 513, 0, 3, 1], expect_stream=[256, 256, 4])
    put("A", "pieces", [65536, 65537, 131329], expect_stream=[])       # 256 pieces, 257 pieces, 514 with a last piece of one
    # context B
    put("B", "cut-by-rows", [1] * 600, expect_stream=[256, 256, 88])
    put("B", "long-first-and-last", [300] + [0] * 700 + [257], expect_stream=[])
    equal = [2] * 128 + [4] * 64 + [8] * 32 + [16] * 16 + [32] * 8 + [31] * 8 + [33] * 7 + [128] * 2
    put("B", "equal-lengths", equal, expect_stream=[256] * 5 + [248, 231, 256])
    # context C, op 2
    many = []
    for i in range(2100):                                              # one row per block; a long row behind every hundredth
        many.append(200)
        if i % 100 == 99:
            many.append((300, 513, 1000)[(i // 100) % 3])
    put("C", "blocks-past-the-cap", many, ops=(2,), expect_stream=[200] * 2100)
    put("C", "longs-past-the-cap", [257] * 2100, ops=(2,), expect_stream=[])
    # one case per context and op without src: nnz == n_unique
    for ctx, ops in (("A", (0, 1, 2)), ("B", (0, 1, 2)), ("C", (2,))):
        for op in ops:
            n_rows, n_cols, n_unique = op_shape(ctx, op)
            rng = np.random.default_rng(77 + op)
            cases.append(OperatorCase(ctx, "no-src", op, _random_lengths(rng, n_unique, n_rows, min(n_cols, BLOCK)).tolist(),
                                      seed=2000 + len(cases), with_src=False))
    return tuple(cases)


# ---------------------------------------------------------------- gather cases
class GatherCase:
    """A synthetic pk_csr map of a context's Jacobian triplets: run lengths summing to n_triplets and a random permutation.
    The value of each triplet is assigned after ``perm`` is drawn, from the bucket of the CSR entry whose run it falls in
    (entry p: bucket p mod 5)."""

    def __init__(self, ctx, name, runs, seed, with_seg=True, context=None):
        self.ctx, self.name, self.id = ctx, name, f"{ctx}-{name}"
        self.context = CONTEXTS[ctx] if context is None else context
        rng = np.random.default_rng(seed)
        self.runs = np.asarray(runs, dtype=np.int64)
        self.n_unique, self.n_triplets = len(self.runs), int(self.runs.sum())
        assert self.n_triplets == self.context["trip_j"] and self.runs.min() >= 1, self.id
        self.start = np.concatenate(([0], np.cumsum(self.runs)))
        self.perm = rng.permutation(self.n_triplets).astype(np.int32)
        if with_seg:
            self.seg = self.start.astype(np.int32)
        else:
            assert self.n_unique == self.n_triplets
            self.seg = None
        entry = np.repeat(np.arange(self.n_unique), self.runs)
        self.triplets = np.zeros(self.n_triplets)
        self.triplets[self.perm] = _scaled(rng, entry % 5)
        n_slices = -(-self.n_unique // BLOCK)
        self.slice_width = np.array([self.runs[b * BLOCK: (b + 1) * BLOCK].max() for b in range(n_slices)])

    @functools.cached_property
    def reference(self):
        """(ref, bound, scale) per CSR entry."""
        t = self.triplets[self.perm]
        ref, sabs = t[self.start[:-1]].copy(), np.abs(t[self.start[:-1]])      # a run of one: the triplet itself, exactly
        t = t.tolist()
        for p in np.flatnonzero(self.runs > 1).tolist():
            run = t[self.start[p]: self.start[p + 1]]
            ref[p] = math.fsum(run)
            sabs[p] = math.fsum(abs(x) for x in run)
        return ref, gamma(self.runs - 1) * sabs, sabs

    def emulated(self, mutant=None):
        return emulate_gather(self, mutant)


def emulate_gather(case, mutant=None):
    """The CSR values as pk_csr computes them: the triplets of a run added sequentially in run order."""
    assert mutant is None or mutant in GATHER_MUTANTS + (GATHER_CAP_MUTANT,)
    t = case.triplets[case.perm]
    if case.seg is None:
        out = t.copy()
    else:
        width = np.repeat(case.slice_width, BLOCK)[: case.n_unique]        # the padded width of the entry's slice
        trips = width - width % 4 if mutant == "remainder" else width      # (the unrolled loop without its remainder loop)
        out = np.zeros(case.n_unique)
        live = np.arange(case.n_unique)
        for k in range(int(case.runs.max())):
            live = live[case.runs[live] > k]                               # (the entries whose run has a k-th triplet)
            m = live[k < trips[live]]
            out[m] = out[m] + t[case.start[:-1][m] + k]
    if mutant == GATHER_CAP_MUTANT:      # a workgroup serves slice b only, not b + 4096 ...: what it skips is never written
        out[CSR_GRID_CAP * BLOCK:] = np.nan
    return out


def _runs(rng, n_triplets, n_unique, widths):
    """Run lengths: slice b's widest run is exactly widths[b], the others ragged below it, n_triplets in all."""
    n_slices = -(-n_unique // BLOCK)
    assert len(widths) == n_slices
    runs = np.ones(n_unique, dtype=np.int64)
    cap = np.repeat(widths, BLOCK)[:n_unique]
    for b, w in enumerate(widths):
        runs[int(rng.integers(b * BLOCK, min((b + 1) * BLOCK, n_unique)))] = w
    extra = n_triplets - int(runs.sum())
    assert 0 <= extra <= int((cap - runs).sum()), (extra, int((cap - runs).sum()))
    while extra:
        p = int(rng.integers(n_unique))
        if runs[p] < cap[p]:
            runs[p] += 1
            extra -= 1
    return runs


GATHER_WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9)       # the widest run of a slice takes every one of these


@functools.lru_cache(maxsize=None)
def gather_cases():
    rng = np.random.default_rng(4242)
    ta, tb = CONTEXTS["A"]["trip_j"], CONTEXTS["B"]["trip_j"]
    cyc = list(GATHER_WIDTHS)
    cases = [
        GatherCase("A", "255-entries", _runs(rng, ta, 255, [5]), 1),
        GatherCase("A", "256-entries", _runs(rng, ta, 256, [7]), 2),
        GatherCase("A", "257-entries", _runs(rng, ta, 257, [3, 2]), 3),
        GatherCase("A", "a-slice-of-ones", _runs(rng, ta, 300, [1, 9]), 4),            # inside a map that has seg
        GatherCase("B", "every-width-mod-255", _runs(rng, tb, 17 * BLOCK - 1, cyc + cyc + [4]), 5),
        GatherCase("B", "every-width-mod-0", _runs(rng, tb, 17 * BLOCK, cyc[::-1] + cyc + [6]), 6),
        GatherCase("B", "every-width-mod-1", _runs(rng, tb, 17 * BLOCK + 1, cyc + cyc[::-1] + [5, 8]), 7),
    ]
    runs = np.ones(tb - 2999, dtype=np.int64)
    runs[800] = 3000                                                                  # one run of 3 000 among runs of 1
    cases.append(GatherCase("B", "a-run-of-3000", runs, 8))
    cases.append(GatherCase("B", "no-seg", np.ones(tb, dtype=np.int64), 9, with_seg=False))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def gather_cap_cases():
    """pk_csr past its grid cap of 4 096 workgroups, on CAP_CONTEXT: the second trip of the slice loop (a map with ``seg``)
    and of the elementwise loop (``seg`` = NULL).  With ``seg``: n_unique = 1 048 577 + 255 = 4 097 whole slices, so slice
    4 096 -- the one a workgroup reaches only on its second trip -- is also the last one; it holds a run of 2 and, in its last
    entry, a run of 5 (the unrolled loop and its remainder on that trip).  Every other run is 1, except the one in slice 0
    that takes up the triplets of the context the map must account for beyond that (pk_set_csr_map requires n_triplets =
    nnz_J): workgroup 0 walks a wide slice and then takes its second trip."""
    trip = CAP_CONTEXT["trip_j"]
    n_unique = 1048577 + 255
    runs = np.ones(n_unique, dtype=np.int64)
    runs[CSR_GRID_CAP * BLOCK + 3], runs[n_unique - 1] = 2, 5
    runs[7] += trip - int(runs.sum())
    assert runs[7] > 1
    return (GatherCase("D", "slices-past-the-cap", runs, 10, context=CAP_CONTEXT),
            GatherCase("D", "no-seg-past-the-cap", np.ones(trip, dtype=np.int64), 11, with_seg=False, context=CAP_CONTEXT))
