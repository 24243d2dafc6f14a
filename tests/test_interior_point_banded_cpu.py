"""The banded step solver of pockit_amd.optimizer.interior_point without a GPU: ``solve`` accepts ``"banded"`` up to the point
where it fails loudly for want of a GPU and still refuses an unknown name; the prototypes of the new entry points; the Python
layer's names; ``BandInfo`` is read-only."""
import os

import numpy as np
import pytest

import models


def test_solve_accepts_banded_and_refuses_an_unknown_name():
    import pockit_amd.lobatto as lobatto
    from pockit_amd.optimizer import interior_point

    system, (phase,), _ = models.lqr(lobatto, 6, 6)
    guess = [lobatto.constant_guess(phase, 0.0), [0.0]]
    with pytest.raises(ValueError, match="banded"):
        interior_point.solve(system, guess, linear_solver="cholesky")
    with pytest.raises(ValueError, match="unknown option"):
        interior_point.solve(system, guess, {"colour": 1}, linear_solver="banded")      # past the name, at the options
    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except ImportError:
        has_gpu = False
    if not has_gpu:
        with pytest.raises(Exception) as raised:                                          # loud: no quiet fall-back to the host
            interior_point.solve(system, guess, linear_solver="banded")
        assert not isinstance(raised.value, ValueError), raised.value
    assert '"banded"' in interior_point.solve.__doc__ and "banded" in interior_point.__doc__


def test_the_unit_is_part_of_the_library_and_of_the_binding():
    from pockit_amd import runtime
    from pockit_amd.hipbuild import RUNTIME_SOURCES

    assert any(os.path.basename(s) == "pk_band.cpp" for s in RUNTIME_SOURCES)
    for name, count in (("pk_band_plan", 6), ("pk_band_factor_dev", 5), ("pk_band_solve_dev", 3), ("pk_band_record", 2), ("pk_solve_banded", 6),
                        ("pk_band_raw_dev", 12), ("pk_band_fill_dev", 6)):
        assert len(runtime.PROTOTYPES[name][1]) == count


def test_the_python_layer_offers_the_capabilities():
    from pockit_amd.band import BandOrdering
    from pockit_amd.evaluator import BandInfo, Evaluator, Linearization

    for name in ("band_plan", "band_factor_dev", "band_solve_dev", "band_record"):
        assert callable(getattr(Evaluator, name))
    assert callable(Linearization.solve_banded) and callable(BandOrdering.assemble) and callable(BandOrdering.to_dense)
    x = np.arange(5.0)
    info = BandInfo([0.0, -1.0, 0.25, 8.0, 4.0, 2.0, 1.0, 3.0], x, 3)
    assert (info.status, info.column, info.min_pivot, info.max_pivot, info.width, info.border, info.interchanges) == ("solved", -1, 0.25, 8.0, 2, 1, 3)
    assert info.primal.tolist() == [0.0, 1.0, 2.0] and info.dual.tolist() == [3.0, 4.0]
    assert BandInfo([1.0, 7.0, 0, 0, 0, 0, 0, 0], x, 3).status == "singular_band_pivot" and BandInfo([2.0] + [0] * 7, x, 3).status == "singular_border"
    assert BandInfo([3.0] + [0] * 7, x, 3).status == "non_finite"
    with pytest.raises(AttributeError):
        info.status = "solved"
    with pytest.raises(ValueError):
        info.record[0] = 1.0
