"""tests/merit_cases.py held to its own claims, on the CPU: the NumPy emulator of pk_merit / pk_merit_fin stays inside the
bound derived from the depth of the documented association around the ``math.fsum`` reference on the exact cases; every
(entry, column) cell is sensitive to one lost or doubled term by at least 2**10 bounds, no cell exempt; on the full-mantissa
case an emulator that fuses multiply and add differs, so the GPU file's bit comparison can tell a contracted FMA; every
mutant is caught."""
import numpy as np
import pytest

import merit_cases as mc

EXACT = mc.exact_cases()
SMALL = [c for c in EXACT if max(c.n_g, c.n_x) < mc.BIG]
BIG = [c for c in EXACT if max(c.n_g, c.n_x) >= mc.BIG]


def test_the_case_list_is_what_the_gpu_file_expects():
    assert {c.n_g for c in SMALL} == set(mc.LENGTHS) and {c.n_x for c in SMALL} == set(mc.LENGTHS)
    assert {c.B for c in SMALL} == {1, 3, 64}
    assert [(c.B, c.n_g, c.workgroups) for c in BIG][0] == (9, 524289, 2313) and BIG[0].workgroups > mc.GRID_CAP
    assert mc.n_pieces(524289, 0) == 257 and mc.n_pieces(0, 0) == 1 and mc.n_pieces(2048, 2049) == 2
    assert {c.kind for c in EXACT} == {"scaled", "bounded"}
    for c in EXACT:
        assert c.ldg > c.n_g and c.ldx > c.n_x and c.ldgrad > c.n_x
        assert np.isnan(c.g.reshape(c.B, c.ldg)[:, c.n_g:]).all() and np.isnan(c.X.reshape(c.B, c.ldx)[:, c.n_x:]).all()
    scaled = [c for c in EXACT if c.kind == "scaled" and c.B == 64]
    ratio = [np.abs(c.g_rows[:, 0]).max() / np.abs(c.g_rows[:, 0]).min() for c in scaled]
    assert min(ratio) >= 2.0 ** 79      # the entries of one call differ by 2**80 in scale


@pytest.mark.parametrize("case", EXACT, ids=lambda c: c.id)
def test_emulator_inside_the_derived_bound_and_every_cell_sensitive(case):
    ref, bound, sens = case.reference
    got = case.emulated()
    assert len(case.failures(got)) == 0
    for q in mc.MAX_COLUMNS + (0, 7):
        assert np.array_equal(got[:, q], ref[:, q], equal_nan=True)      # exact columns
    assert (bound[:, mc.SUM_COLUMNS] > 0).all() and (bound[:, mc.MAX_COLUMNS + (0, 7)] == 0).all()
    assert np.isfinite(got[:, 1:]).all()
    # one lost or doubled term moves every cell by at least 2**10 bounds: no exempt cell
    assert (sens > 0).all(), np.argwhere(~(sens > 0))
    assert (sens >= 2.0 ** 10 * bound).all()
    if min(case.n_g, case.n_x) >= 4:
        assert (got[:, 7] >= 4).all()      # every entry holds non-finite values that were counted


def test_fused_multiply_add_is_visible_on_the_full_mantissa_case():
    case = mc.full_case()
    plain, fused = case.emulated(), case.emulated(fma=True)
    assert np.isfinite(plain[:, 1:]).all()
    for q in (3, 6):
        assert (plain[:, q] != fused[:, q]).any(), mc.COLUMNS[q]
    for q in (0, 1, 2, 4, 5, 7):
        assert np.array_equal(plain[:, q], fused[:, q], equal_nan=True)
    x, d, alphas = mc.trial_case()
    a, b = mc.trial_points(x, d, alphas), mc.trial_points(x, d, alphas, fma=True)
    assert (a != b).any() and np.array_equal(a, x[None, :] + alphas[:, None] * d[None, :])
    assert np.array_equal(a[0], x) and np.array_equal(a[1], x + d)


def test_without_d_the_slope_is_zero():
    out = mc.no_d_case().emulated()
    assert (out[:, 6] == 0.0).all() and not np.signbit(out[:, 6]).any()


def test_dense_form_is_the_padded_form():
    case = mc.full_case()
    dense = mc.emulate_dense(case.f, case.grad_rows, case.g_rows, case.X_rows, (case.clb, case.cub, case.vlb, case.vub), case.d)
    assert mc.same_bits(dense, case.emulated())


def _caught(case, mutant):
    got = case.emulated(mutant=mutant)
    if case.kind != "full" and len(case.failures(got)):
        return True
    return not mc.same_bits(got, case.emulated())


@pytest.mark.parametrize("mutant", mc.MUTANTS)
def test_every_mutant_is_caught(mutant):
    cases = BIG[:1] if mutant == "second_trip_dropped" else [c for c in SMALL if c.B == 3] + [mc.full_case()]
    hits = [c.id for c in cases if _caught(c, mutant)]
    assert hits, mutant
    if mutant in ("bounds_swapped", "nonfinite_added", "ld_is_length", "max_as_sum"):
        assert mc.full_case().id in hits      # ... by the bit comparison alone, too
    if mutant == "second_trip_dropped":       # and only where there is a second trip
        assert not any(_caught(c, mutant) for c in SMALL if c.B == 3)
