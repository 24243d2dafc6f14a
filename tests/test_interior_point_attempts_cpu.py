"""``band_attempts`` of pockit_amd.optimizer.interior_point without a GPU: the candidate logic of the batched walk
(``Regularisation.schedule`` / ``batches`` / ``tried``) picks the same ``delta_w`` and leaves the same ``last`` and ``count`` as
the sequential ``attempts()`` / ``accept()`` for any pattern of passing and failing candidates; the ``ValueError``s of the
keyword; ``solve`` still fails loudly for want of a GPU; the prototypes and the Python layer of the batch forms."""
import itertools

import numpy as np
import pytest

import models
from pockit_amd.optimizer.interior_point import MAX_BAND_ATTEMPTS, MAX_REGULARISATIONS, Regularisation

ATTEMPTS = 1 + MAX_REGULARISATIONS


def sequential(reg, passing):
    """What the solver does with ``band_attempts = 1``: the accepted delta_w or None; ``passing[i]``: does candidate i pass?"""
    for i, delta in enumerate(reg.attempts()):
        if passing[i]:
            reg.accept(delta)
            return delta
    return None


def batched(reg, passing, k):
    """What the solver does with ``band_attempts = k``: every batch is taken whole, then walked in order."""
    i = 0
    for deltas in reg.batches(k):
        assert 1 <= len(deltas) <= k
        for delta in deltas:
            reg.tried(delta)
            if passing[i]:
                reg.accept(delta)
                return delta
            i += 1
    assert i == ATTEMPTS
    return None


def patterns():
    rng = np.random.default_rng(5)
    yield [True] + [False] * (ATTEMPTS - 1)                     # the first candidate (delta_w = 0) passes
    yield [False] * ATTEMPTS                                    # no candidate passes
    for first in range(1, ATTEMPTS):                            # exactly the candidate `first` is the first to pass
        yield [False] * first + [True] + list(rng.random(ATTEMPTS - first - 1) < 0.5)
    for _ in range(40):
        yield list(rng.random(ATTEMPTS) < 0.3)


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_the_batched_walk_picks_what_the_sequential_loop_picks(k):
    for last in (None, 1e-4, 0.0512, 7.0):                      # before any regularised step succeeded, and once `last` is set
        for passing in patterns():
            a, b = Regularisation(), Regularisation()
            a.last = b.last = last
            a.count = b.count = 17
            picked = (sequential(a, passing), batched(b, passing, k))
            assert picked[0] == picked[1] or (picked[0] is None and picked[1] is None), (k, last, passing, picked)
            assert (a.last, a.count) == (b.last, b.count), (k, last, passing)
            if not any(passing):
                assert picked == (None, None) and a.count == 17 + MAX_REGULARISATIONS and a.last == last


def test_steps_in_a_row_keep_the_two_walks_together():
    rng = np.random.default_rng(9)
    for k in (2, 3, 8):
        a, b = Regularisation(), Regularisation()
        for _ in range(30):
            passing = list(rng.random(ATTEMPTS) < 0.4)
            assert sequential(a, passing) == batched(b, passing, k)
            assert (a.last, a.count) == (b.last, b.count)


def test_the_schedule_is_listed_without_counting():
    reg = Regularisation()
    for last in (None, 3e-3):
        reg.last = last
        values = reg.schedule()
        assert reg.count == 0 and reg.last == last
        assert values == list(Regularisation.attempts(_with_last(last))) and len(values) == ATTEMPTS and values[0] == 0.0
        assert list(itertools.chain.from_iterable(reg.batches(5))) == values and [len(b) for b in reg.batches(5)] == [5, 5, 3]
        assert reg.count == 0
    assert values[1] == max(1e-4, 3e-3 / 3.0) and values[2] == values[1] * 8.0


def _with_last(last):
    reg = Regularisation()
    reg.last = last
    return reg


def _lqr():
    import pockit_amd.lobatto as lobatto

    system, (phase,), _ = models.lqr(lobatto, 6, 6)
    return system, [lobatto.constant_guess(phase, 0.0), [0.0]]


@pytest.mark.parametrize("value", [0, -1, MAX_BAND_ATTEMPTS + 1, 2.0, "2", None, True])
def test_band_attempts_outside_its_range_is_a_value_error(value):
    from pockit_amd.optimizer import interior_point

    system, guess = _lqr()
    with pytest.raises(ValueError, match="band_attempts"):
        interior_point.solve(system, guess, linear_solver="banded", band_attempts=value)


@pytest.mark.parametrize("linear_solver", ["direct", "minres"])
def test_band_attempts_needs_the_banded_solver(linear_solver):
    from pockit_amd.optimizer import interior_point

    system, guess = _lqr()
    with pytest.raises(ValueError, match="band_attempts"):
        interior_point.solve(system, guess, linear_solver=linear_solver, band_attempts=2)
    with pytest.raises(ValueError, match="band_attempts"):
        interior_point.solve(system, guess, band_attempts=3)


def test_solve_still_fails_loudly_without_a_gpu():
    from pockit_amd.optimizer import interior_point

    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except ImportError:
        has_gpu = False
    if not has_gpu:
        system, guess = _lqr()
        with pytest.raises(Exception) as raised:                # loud: no quiet fall-back to the host
            interior_point.solve(system, guess, linear_solver="banded", band_attempts=4)
        assert not isinstance(raised.value, ValueError), raised.value
    assert "band_attempts" in interior_point.solve.__doc__ and "band_attempts" in interior_point.__doc__


def test_the_batch_forms_are_part_of_the_binding_and_of_the_python_layer():
    from pockit_amd import runtime
    from pockit_amd.evaluator import Evaluator, Linearization

    for name, count in (("pk_band_factor_batch_dev", 10), ("pk_band_solve_batch_dev", 6), ("pk_band_record_batch", 3), ("pk_solve_banded_batch", 7),
                        ("pk_band_raw_batch_dev", 20)):
        assert len(runtime.PROTOTYPES[name][1]) == count and name in runtime.EXPORTS
    for method in ("band_factor_batch_dev", "band_solve_batch_dev", "band_record_batch"):
        assert getattr(Evaluator, method).__doc__
    assert Linearization.solve_banded_batch.__doc__
