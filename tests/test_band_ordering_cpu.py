"""pockit_amd.band.BandOrdering on the plans of DESIGN.md section 23's table, without a GPU: the permutation is one, the border
and the half-bandwidth are within the table, ``assemble`` scattered to dense equals ``DirectKkt``'s K under the permutation bit
for bit, the caps raise ``ValueError`` with a sentence that points to the direct solver, and a structure with two dense
unknowns puts both in the border.  The 200-interval plans are left to a single case."""
import importlib

import numpy as np
import pytest

import models
from pockit_amd.band import P_CAP, W_CAP, BandOrdering
from pockit_amd.csr import CsrMap
from pockit_amd.optimizer.interior_point import DirectKkt

# (model, scheme, mesh, points): (border, the half-bandwidth the table gives)
TABLE = {("lqr", "radau", 6, 6): (0, 17), ("lqr", "radau", 40, 6): (0, 29), ("lqr", "lobatto", 6, 6): (0, 14), ("lqr", "lobatto", 40, 6): (0, 24),
         ("brachistochrone", "radau", 10, 8): (1, 46), ("brachistochrone", "radau", 40, 8): (1, 78),
         ("brachistochrone", "lobatto", 10, 8): (1, 54), ("brachistochrone", "lobatto", 40, 8): (1, 77),
         ("planar_quadrotor", "radau", 14, 6): (0, 130), ("planar_quadrotor", "radau", 60, 6): (0, 130),
         ("planar_quadrotor", "lobatto", 14, 6): (0, 73), ("planar_quadrotor", "lobatto", 60, 6): (0, 132)}
LARGE = {("brachistochrone", "radau", 200, 8): (1, 72)}


def _maps(key):
    name, scheme, mesh, k = key
    plan = getattr(models, name)(importlib.import_module(f"pockit_amd.{scheme}"), mesh, k)[0].plan
    map_j = CsrMap(plan.jac_row, plan.jac_col, (plan.m, plan.n))
    map_h = CsrMap(plan.hess_row, plan.hess_col, (plan.n, plan.n))
    free = np.asarray(plan.v_lb, dtype=np.float64) != np.asarray(plan.v_ub, dtype=np.float64)
    return plan, map_j, map_h, free


def _check_structure(o, plan, free, border, width):
    assert o.N == int(free.sum()) + plan.m == o.nb + o.p
    assert np.array_equal(np.sort(o.pos), np.arange(o.N)) and np.array_equal(o.pos[o.inv], np.arange(o.N))
    caller = np.concatenate((np.flatnonzero(free), plan.n + np.arange(plan.m)))
    assert np.array_equal(np.sort(o.order), caller)                      # every free variable and every row once, no fixed variable
    assert o.p <= max(border, 1) and o.p <= 1 and o.w <= width, (o.p, o.w)
    assert o.ldab == 3 * o.w + 1 and o.dests == o.ldab * o.nb + o.nb * o.p + o.p * o.p and o.map.shape == (2 * o.dests,)
    assert np.all(np.sort(o.pos[o.inv[o.nb:]]) == np.arange(o.nb, o.N))     # the border comes last


def _check_values(o, map_j, map_h, free, seed=5):
    rng = np.random.default_rng(seed)
    n, m = len(free), map_j.shape[0]
    hvals, jvals = rng.uniform(-1.0, 1.0, map_h.nnz), rng.uniform(-1.0, 1.0, map_j.nnz)
    s1, s2 = rng.uniform(0.5, 1.5, n), np.where(np.arange(m) % 3 == 0, 0.0, rng.uniform(0.5, 1.5, m))
    band, U, C = o.assemble(hvals, jvals, s1, s2)
    assert band.shape == (o.ldab, o.nb) and U.shape == (o.nb, o.p) and C.shape == (o.p, o.p)
    d = DirectKkt(map_j, map_h, free)
    import scipy.sparse as sp

    data = d.select @ np.concatenate((hvals, jvals, s1, s2))
    K = sp.csc_matrix((data, d.indices, d.indptr), shape=(d.N, d.N)).toarray()
    want = K[np.ix_(o.inv, o.inv)]
    got = o.to_dense(band, U, C)
    assert got.tobytes() == want.tobytes()                                 # bit for bit: no entry is -0.0 on either side
    assert not np.any(band[: o.w])                                        # the fill rows start as zeros
    b = rng.uniform(-1.0, 1.0, n + m)
    assert np.array_equal(o.scatter(o.permute_rhs(b))[o.order], b[o.order]) and not o.scatter(o.permute_rhs(b))[:n][~free].any()


@pytest.mark.parametrize("key", sorted(TABLE), ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}x{k[3]}")
def test_the_ordering_of_the_table(key):
    plan, map_j, map_h, free = _maps(key)
    o = BandOrdering(map_j, map_h, free)
    border, width = TABLE[key]
    _check_structure(o, plan, free, border, width)
    assert o.p == border
    if plan.n + plan.m <= 2500:
        _check_values(o, map_j, map_h, free)
    again = BandOrdering(map_j, map_h, free)
    assert np.array_equal(again.order, o.order) and np.array_equal(again.map, o.map)      # deterministic


def test_a_200_interval_plan():
    (key, (border, width)), = LARGE.items()
    plan, map_j, map_h, free = _maps(key)
    o = BandOrdering(map_j, map_h, free)
    _check_structure(o, plan, free, border, width)
    assert o.p == border == 1 and o.N == 11205


def test_the_caps_raise_and_point_to_the_direct_solver():
    plan, map_j, map_h, free = _maps(("brachistochrone", "radau", 10, 8))
    with pytest.raises(ValueError, match='linear_solver="direct"'):
        BandOrdering(map_j, map_h, free, max_width=45)
    with pytest.raises(ValueError, match='linear_solver="direct"'):
        BandOrdering(map_j, map_h, free, max_border=0)
    assert BandOrdering(map_j, map_h, free, max_width=46, max_border=1).w == 46
    assert W_CAP >= 160 and P_CAP >= 8
    with pytest.raises(ValueError):
        BandOrdering(map_j, map_h, free[:-1])


def test_two_dense_unknowns_both_go_to_the_border():
    """A chain of 600 variables and 598 rows, each row on three neighbours and on the LAST TWO variables."""
    n, m = 600, 598
    rows = np.repeat(np.arange(m), 5)
    cols = np.stack([np.arange(m), np.arange(m) + 1, np.minimum(np.arange(m) + 2, n - 3), np.full(m, n - 2), np.full(m, n - 1)], axis=1)
    cols[:, 2] = np.where(cols[:, 2] == cols[:, 1], cols[:, 0], cols[:, 2])
    keep = np.ones(cols.shape, dtype=bool)
    keep[:, 2] = cols[:, 2] != cols[:, 0]
    map_j = CsrMap(rows[keep.ravel()], cols.ravel()[keep.ravel()], (m, n))
    map_h = CsrMap(np.arange(n), np.arange(n), (n, n))
    free = np.ones(n, dtype=bool)
    free[7] = False
    o = BandOrdering(map_j, map_h, free)
    assert o.p == 2 and sorted(o.order[o.nb:].tolist()) == [n - 2, n - 1] and o.w <= 8
    _check_values(o, map_j, map_h, free)
    with pytest.raises(ValueError, match='linear_solver="direct"'):
        BandOrdering(map_j, map_h, free, max_border=1)
