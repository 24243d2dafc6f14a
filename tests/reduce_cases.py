"""Inputs, exact references and bit-for-bit emulators for the reductions over the rows of an operator: ``pk_red_rows``,
``pk_red_long`` and ``pk_diag`` (pockit_amd/csrc/pk_reduce.cpp).  A plain helper module on top of tests/sparse_cases.py, shared by
tests/test_reduce_cases_cpu.py (which tests this module) and tests/test_gpu_operator_reduce.py (which tests the kernels).

A ``ReduceCase`` is an ``OperatorCase`` whose ``products()`` are the terms of a mode:

    0 abs_sum   |a_e| * w[c_e]            1 sq_sum   (a_e * a_e) * w[c_e]           2 abs_max   |a_e| * w[c_e], y = max(0, t, add)

Inputs.  The values are sparse_cases' (24-bit mantissas, row r from bucket r mod 5).  A weight is ``q/16 * 2**k`` with integer
q in [16, 31] and k in {-1, 0, 1}: a 5-bit mantissa.  ``(a a) w`` then has at most 24 + 24 + 5 = 53 significant bits and
``|a| w`` 29: every term is exact, so the two sums are held to what the products are held to -- ``math.fsum`` over a row's
terms, the derived bound gamma_{L+1} (sum|t| + |add|) of sparse_cases, and bit equality with ``sparse_cases.emulate_operator``
as it stands, fed these terms.  ``add[r]`` is a full-precision double of the scale of the row's TERMS (2**(2 s) for the
squares), so the bound stays a small multiple of every term and a lost one shows.

The maximum is exact whatever the order, so a lost term must show by position: a PLANTED case scales one value of a row by 16
(still exact) and gives it a ``src`` no other entry shares, which makes that entry the row's unique maximum (|a| w lies in
[1/2, 8) 2**s for every other entry and in [8, 128) 2**s for the planted one; add stays below 4 * 2**s).  ``emulate_max`` walks
the blocks the way the kernels do -- stream rows sequentially, the tree over a piece, the strided trips of a long row -- so the
structural mistakes drop the entries they would drop on the device.

One full-mantissa case (53-bit values and weights, mode 1) pins the rounding order: its terms are ``(a * a) * w`` with both
roundings, and ``a * (a * w)`` differs.

``mutant`` names one deliberate mistake each (MUTANTS); the CPU test requires every one to be caught.
"""
import functools

import numpy as np

import sparse_cases as sc

ABS_SUM, SQ_SUM, ABS_MAX = 0, 1, 2
MODES = (ABS_SUM, SQ_SUM, ABS_MAX)
TERM_MUTANTS = ("weight_by_row", "fabs_dropped", "null_weight_as_zero")
MAX_MUTANTS = ("max_as_sum", "add_ignored_in_max")
WALK_MUTANTS = ("tree_stops_at_2", "strided_first_trip")
DIAGONAL_MUTANTS = ("pos_minus_one_as_zero",)
MUTANTS = TERM_MUTANTS + MAX_MUTANTS + WALK_MUTANTS + DIAGONAL_MUTANTS


def _weights(rng, size):
    """q/16 * 2**k, q in [16, 31], k in {-1, 0, 1}: positive, 5-bit mantissas, in [1/2, 4)."""
    return np.ldexp(rng.integers(16, 32, size).astype(np.float64) / 16.0, rng.integers(-1, 2, size))


class ReduceCase(sc.OperatorCase):
    """``OperatorCase`` with a mode, weights (``with_w`` False: the kernel gets NULL) and an ``add`` of the terms' scale.
    ``plant``: (row, offset within the row) of the entry made the row's unique maximum.  ``full_mantissa``: 53-bit values and
    weights, whose terms round."""

    def __init__(self, ctx, name, op, lengths, seed, mode, with_w=True, with_src=True, plant=None, full_mantissa=False):
        super().__init__(ctx, name, op, lengths, seed, with_src=with_src)
        self.mode, self.with_w, self.plant, self.full_mantissa = mode, with_w, plant, full_mantissa
        self.id = f"{ctx}-{name}-op{op}-mode{mode}-{'w' if with_w else 'now'}"
        rng = np.random.default_rng(seed + 50000)
        self.w = _weights(rng, self.n_cols)
        power = np.asarray(sc.BUCKETS)[np.arange(self.n_rows) % 5] * (2 if mode == SQ_SUM else 1)
        self.add = rng.uniform(1.0, 4.0, self.n_rows) * rng.choice([-1.0, 1.0], self.n_rows) * np.ldexp(1.0, power)
        if full_mantissa:
            self.vals = self.vals * rng.uniform(1.0, 1.5, len(self.vals))
            self.w = self.w * rng.uniform(1.0, 1.5, len(self.w))
        if plant is not None:
            assert self.src is not None and mode == ABS_MAX
            row, offset = plant
            assert 0 <= offset < self.lengths[row], self.id
            e = int(self.indptr[row]) + offset
            own = int(self.src[e])
            for other in np.flatnonzero(self.src == own):      # nobody else reads the planted value
                if other != e:
                    self.src[other] = own + 5 if own + 5 < self.n_unique else own - 5
            assert int((self.src == own).sum()) == 1 and np.all(self.src >= 0) and np.all(self.src < self.n_unique)
            self.vals[own] *= 16.0
            self.planted_entry = e

    def values(self):
        return self.vals[np.arange(self.nnz) if self.src is None else self.src]

    def terms(self, mutant=None):
        """The terms in entry order, as the kernel forms them (abs_max: before the comparison with 0)."""
        a = self.values()
        t = a * a if self.mode == SQ_SUM else (a if mutant == "fabs_dropped" else np.abs(a))
        if self.with_w:
            t = t * (self.w[self.row_of % self.n_cols] if mutant == "weight_by_row" else self.w[self.indices])
        elif mutant == "null_weight_as_zero":
            t = t * 0.0
        return t

    def products(self):
        """What ``sparse_cases`` sums: the terms (exact but for the full-mantissa case)."""
        return self.terms()

    @functools.cached_property
    def max_reference(self):
        """{with_add: exact y of mode 2}: max(0, max_e t_e, add[row])."""
        t = self.terms()
        top = np.zeros(self.n_rows)
        np.maximum.at(top, self.row_of, t)
        return {False: top, True: np.maximum(top, self.add)}

    def emulated(self, with_add, mutant=None):
        return emulate_reduce(self, self.add if with_add else None, mutant)


class _Mutated:
    """A case seen through a mutant of its terms: what ``sparse_cases.emulate_operator`` reads of a case."""

    def __init__(self, case, terms):
        self.indptr, self.n_rows, self._terms = case.indptr, case.n_rows, terms

    def products(self):
        return self._terms


def _greater(a, b):
    """b where b > a, else a: the comparison of the kernels (a NaN b loses)."""
    return np.where(b > a, b, a)


def _max_tree(a, mutant):
    w = sc.BLOCK // 2
    while w >= (2 if mutant == "tree_stops_at_2" else 1):
        a[:, :w] = _greater(a[:, :w], a[:, w: 2 * w])
        w //= 2
    return a[:, 0].copy()


def emulate_max(case, terms, add=None, mutant=None):
    """y of mode 2 over the row blocks, as pk_red_rows and pk_red_long walk them; NaN where no thread writes."""
    p = _greater(np.zeros(len(terms)), terms)                 # what reaches a slot: never below 0, never NaN
    indptr = case.indptr.astype(np.int64)
    blocks, longs, n_slots = sc.row_blocks(case.indptr)
    y = np.full(case.n_rows, np.nan)
    stream = [np.arange(b[2], b[2] + b[3]) for b in blocks if b[3] >= 0]
    if stream:                                                # a stream row: its slots one after the other (no slot is NaN or
        rows = np.concatenate(stream)                         # below 0, so the order of the comparisons does not show)
        top = np.zeros(case.n_rows)
        np.maximum.at(top, np.repeat(np.arange(case.n_rows), np.diff(indptr)), p)
        y[rows] = top[rows]
    pieces = [b for b in blocks if b[3] < 0]
    if pieces:
        a = np.zeros((len(pieces), sc.BLOCK))
        for j, (e, cnt, _, _) in enumerate(pieces):
            a[j, :cnt] = p[e: e + cnt]
        partial = np.full(n_slots, np.nan)
        partial[[b[2] for b in pieces]] = _max_tree(a, mutant)
        for row, first, cnt in longs:
            a = np.zeros((1, sc.BLOCK))
            for j in range(1 if mutant == "strided_first_trip" else -(-cnt // sc.BLOCK)):
                part = partial[first + sc.BLOCK * j: first + min(cnt, sc.BLOCK * (j + 1))]
                a[0, : len(part)] = _greater(a[0, : len(part)], part)
            y[row] = _max_tree(a, mutant)[0]
    if add is not None and mutant != "add_ignored_in_max":
        y = _greater(y, add)
    return y


def emulate_reduce(case, add=None, mutant=None):
    """y as pk_red_rows and pk_red_long compute it, bit for bit."""
    assert mutant is None or mutant in MUTANTS
    terms = case.terms(mutant if mutant in TERM_MUTANTS else None)
    walk = mutant if mutant in WALK_MUTANTS else None
    if case.mode == ABS_MAX and mutant != "max_as_sum":
        return emulate_max(case, terms, add, mutant)
    if case.mode == ABS_MAX:
        terms = _greater(np.zeros(len(terms)), terms)
    return sc.emulate_operator(_Mutated(case, terms), add, walk)


def emulate_diagonal(vals, pos, add=None, mutant=None):
    """y[i] = pos[i] >= 0 ? vals[pos[i]] : 0.0 (+ add[i])"""
    pos = np.asarray(pos, dtype=np.int64)
    if mutant == "pos_minus_one_as_zero":
        d = vals[np.maximum(pos, 0)]
    else:
        d = np.where(pos >= 0, vals[np.maximum(pos, 0)], 0.0)
    return d if add is None else d + add


def diagonal_positions(n, n_unique, seed):
    """A synthetic ``pos``: -1 in the first row, the last row and a run of rows, the others anywhere in [0, n_unique)."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, n_unique, n).astype(np.int32)
    pos[0] = pos[n - 1] = -1
    pos[n // 3: n // 3 + 7] = -1
    pos[1], pos[2] = 0, n_unique - 1
    return pos


# the plantings: name -> (row, offset) in the rows PLANT_LENGTHS
PLANT_LENGTHS = [3, 5, 1, 512, 513, 0, 65537]
PLANTS = {
    "index-0": (4, 0),                       # the entry at index 0 of a row
    "last-entry": (3, 511),                  # the last entry of a row
    "offset-255-of-a-piece": (4, 255),
    "offset-0-of-the-next-piece": (4, 256),
    "last-piece-of-one": (4, 512),           # the single entry of a last piece of one
    "piece-256": (6, 256 * 256),             # a piece beyond index 255: the second trip of the strided walk (and a piece of one)
    "piece-255": (6, 255 * 256 + 255),       # ... and the last piece of the first trip
    "stream-row-first": (1, 0),              # a row's first and last entry inside a stream block shared with other rows
    "stream-row-last": (1, 4),
}


@functools.lru_cache(maxsize=None)
def reduce_cases():
    """Every case of the GPU file."""
    cases = []

    def put(ctx, name, lengths, op, mode, **kw):
        assert len(lengths) <= sc.op_shape(ctx, op)[0], (ctx, name, op)      # (every structure fits every op it is listed for)
        cases.append(ReduceCase(ctx, name, op, lengths, seed=3000 + len(cases), mode=mode, **kw))

    edges = [0, 1, 255, 256, 257, 512, 513, 0, 3, 1]
    for mode in MODES:
        for op in (0, 1, 2):
            put("A", "edges", edges, op, mode)
        put("A", "edges", edges, 1, mode, with_w=False)
    for op, mode in ((0, 0), (0, 1), (1, 1), (2, 1), (2, 2)):
        put("A", "pieces", [65536, 65537, 131329], op, mode, with_w=(op, mode) != (1, 1))
    equal = [2] * 128 + [4] * 64 + [8] * 32 + [16] * 16 + [32] * 8 + [31] * 8 + [33] * 7 + [128] * 2
    for name, lengths in (("cut-by-rows", [1] * 600), ("long-first-and-last", [300] + [0] * 700 + [257]), ("equal-lengths", equal)):
        for mode in MODES:
            for op in (0, 1, 2):
                put("B", name, lengths, op, mode, with_w=(mode + op) % 2 == 0)
    many = []
    for i in range(2100):                                              # one row per block; a long row behind every hundredth
        many.append(200)
        if i % 100 == 99:
            many.append((300, 513, 1000)[(i // 100) % 3])
    put("C", "blocks-past-the-cap", many, 2, SQ_SUM)
    put("C", "blocks-past-the-cap", many, 2, ABS_MAX)
    put("C", "longs-past-the-cap", [257] * 2100, 2, ABS_SUM, with_w=False)
    put("C", "longs-past-the-cap", [257] * 2100, 2, ABS_MAX)
    for ctx in "AB":
        for op in (0, 1, 2):
            n_rows, n_cols, n_unique = sc.op_shape(ctx, op)
            rng = np.random.default_rng(177 + op)
            lengths = sc._random_lengths(rng, n_unique, n_rows, min(n_cols, sc.BLOCK)).tolist()
            put(ctx, "no-src", lengths, op, (op + (ctx == "B")) % 3, with_src=False, with_w=op != 1)
    for k, (name, where) in enumerate(PLANTS.items()):
        put("A", "planted-" + name, PLANT_LENGTHS, k % 3, ABS_MAX, plant=where, with_w=k % 4 != 3)
    put("A", "full-mantissa", edges, 0, SQ_SUM, full_mantissa=True)
    return tuple(cases)
