"""Batches of the synthetic systems of tests/band_cases.py for the batch forms of pockit_amd/csrc/pk_band.cpp: B systems of one
shape, every array packed at a stride LARGER than its length with NaN in the gaps, and per entry what ``band_cases.solve_system``
gives for that entry alone -- the contract of the batch forms is exactly that.  A plain helper module, shared by
tests/test_band_batch_cpu.py (the host stand-in's walk) and tests/test_gpu_band_batch.py (the kernels).  No arithmetic of its own:
the emulator is the existing one."""
import numpy as np

import band_cases as bc

BATCH_CAP = 16                         # PK_BD_BATCH_CAP
GAP = 3                                # doubles (or 32-bit integers) between two entries of a packed array
BATCHES = (1, 2, 3, BATCH_CAP)
# the issue's table (Nb 0, 1, 33, 65; w 0, 7, 33, 192; p 0, 1, 8) within band_cases.shapes(), then Nb = 1 and the cap of w from there
_TABLE = [s for s in bc.shapes() if s[0] in (0, 1, 33, 65) and s[1] in (0, 7, 33, 192) and s[2] in (0, 1, 8)]
SHAPES = _TABLE + [(1, 1, 1), (bc.W_CAP + 1, bc.W_CAP, 0), (2 * bc.NB + 1 + bc.W_CAP, bc.W_CAP, 1)]
LONG = (3, 4129, 8, 1)                 # B, Nb, w, p: three pieces per dot, 130 panels
MIXED = (("plain", 0.0), ("zero_column", 1.0), ("tiny_diagonal", 0.0), ("nan", 3.0))


class Batch:
    """``entries``: the ``(AB, U, C, rhs)`` of each system; ``band``, ``U``, ``C``, ``rhs``: the packed arrays (NaN in the gaps,
    and NaN in the fill rows and outside the matrix of every band); ``strides``: by name; ``expected``: per entry
    ``(band, ipiv, x or None, rec)`` of the emulator."""

    def __init__(self, nb, w, p, picks, nan_outside=True):
        self.B, self.nb, self.w, self.p = len(picks), nb, w, p
        self.entries = [bc.system(nb, w, p, seed=seed, variant=variant) for variant, seed in picks]
        self.lengths = dict(band=(3 * w + 1) * nb, U=nb * p, C=p * p, rhs=nb + p, x=nb + p, ipiv=nb, rec=8)
        self.strides = {k: v + GAP for k, v in self.lengths.items()}
        self.inside = bc.in_band(nb, w) | bc.fill_rows(nb, w)      # the slots of a band the kernels own
        packed = {k: np.full(self.B * self.strides[k], np.nan) for k in ("band", "U", "C", "rhs")}
        for e, (AB, U, C, rhs) in enumerate(self.entries):
            given = AB.copy(order="F")
            if nan_outside:
                given[~bc.in_band(nb, w)] = np.nan      # the fill rows and the slots outside the matrix: never read
            for k, a in (("band", given), ("U", U), ("C", C), ("rhs", rhs)):
                packed[k][e * self.strides[k]: e * self.strides[k] + self.lengths[k]] = np.asarray(a).ravel(order="F")
        self.band, self.U, self.C, self.rhs = (packed[k] for k in ("band", "U", "C", "rhs"))
        self.expected = [bc.solve_system(*entry) for entry in self.entries]

    def entry(self, name, packed, e):
        """Entry e's slice of a packed array ``name`` (the band as ``(3 w + 1, nb)``)."""
        a = np.asarray(packed)[e * self.strides[name]: e * self.strides[name] + self.lengths[name]]
        return a.reshape((3 * self.w + 1, self.nb), order="F") if name == "band" else a

    def gaps(self, name, packed):
        """The slots of a packed array ``name`` that belong to no entry."""
        a = np.asarray(packed).reshape(self.B, self.strides[name])
        return a[:, self.lengths[name]:]


def same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all(got.view(np.uint64) == want.view(np.uint64)))


def picks(B, first_seed=0):
    """B entries, plain and tiny-diagonal alternating, each with its own seed."""
    return [("tiny_diagonal" if e % 2 else "plain", first_seed + e) for e in range(B)]


def check_entry(batch, e, band, ipiv, x, rec, untouched=-77.0):
    """Entry e's results against the emulator's: the record; with status 0 the interchanges, the band's own slots and the
    solution, otherwise the solution still as the caller left it (``untouched``; NaN allowed)."""
    w_band, w_ipiv, w_x, w_rec = batch.expected[e]
    assert same(rec, w_rec), (e, rec, w_rec)
    if w_rec[bc.STATUS] == 0.0:
        assert np.array_equal(np.asarray(ipiv, dtype=np.int64), w_ipiv), e
        assert same(np.asarray(band)[batch.inside], w_band[batch.inside]), e
        assert same(x, w_x), e
    else:
        x = np.asarray(x)
        assert w_x is None and np.all(np.isnan(x) if np.isnan(untouched) else x == untouched), e
