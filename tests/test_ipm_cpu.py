"""The runtime unit behind the barrier terms, the dual residual and the boundary step (pockit_amd/csrc/pk_ipm.cpp) built with
``-fsanitize=address,undefined`` against the host-only stand-in of the HIP runtime and driven by tests/fake_hip/ipm_driver.cpp: the
stand-in walk of every kernel against plain loops at the lengths where the pieces and the strided scalar step change shape, clean
and with planted defects, the public forms against the raw form, the refusals with their codes and sentinels, what frees the
state; with ``--dump`` two boxed vectors compared BIT FOR BIT with the emulator of tests/ipm_cases.py (column 4, the sum of
logarithms, within the bound of two implementations of log), so the documented association is held on the CPU as well.  CPU
only; a stand-alone program (its own main): nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ipm_cases as ip
from sanitized_build import sanitized_driver

ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sanitized_driver("ipm_driver.cpp", tmp_path_factory.mktemp("ipm_driver"))


def test_the_unit_is_part_of_the_library_and_of_the_binding():
    from pockit_amd import runtime
    from pockit_amd.hipbuild import RUNTIME_SOURCES

    assert any(os.path.basename(s) == "pk_ipm.cpp" for s in RUNTIME_SOURCES)
    for name, count in (("pk_ip_terms_dev", 10), ("pk_dual_residual_dev", 9), ("pk_ip_step_dev", 12), ("pk_ip_terms", 9),
                        ("pk_dual_residual", 7), ("pk_ip_step", 11), ("pk_ip_raw_dev", 18)):
        assert len(runtime.PROTOTYPES[name][1]) == count


def test_the_python_layer_offers_the_three_capabilities():
    from pockit_amd.evaluator import BarrierTerms, BoundaryStep, DualResidual, Evaluator, Linearization

    for name in ("ip_terms_dev", "dual_residual_dev", "ip_step_dev", "barrier_terms", "boundary_step"):
        assert callable(getattr(Evaluator, name))
    assert callable(Linearization.dual_residual)
    terms = BarrierTerms(np.arange(3.0), -np.arange(3.0), [0.5, 6.0, 4.0, 0.25, -1.0, 0.0, 3.0, 0.125])
    assert (terms.compl_inf, terms.compl_sum, terms.sides, terms.min_slack, terms.log_sum, terms.bad, terms.z_sum, terms.min_compl) == (
        0.5, 6.0, 4.0, 0.25, -1.0, 0.0, 3.0, 0.125)
    assert terms.mean_compl == 1.5 and terms.table.shape == (8,) and terms.sigma[2] == 2.0 and terms.rbar[2] == -2.0
    with pytest.raises(AttributeError):
        terms.bad = 1.0
    with pytest.raises(ValueError):
        terms.sigma[0] = 1.0
    step = BoundaryStep(np.zeros(2), np.ones(2), [0.25, 1.0, 7.0, 0.0])
    assert (step.alpha_primal, step.alpha_dual, step.blocking, step.bad) == (0.25, 1.0, 7, 0.0) and step.dzu[1] == 1.0
    assert BoundaryStep(np.zeros(2), np.ones(2), [1.0, 1.0, -1.0, 0.0]).blocking is None
    res = DualResidual([2.0, 9.0, 0.0, 0.0])
    assert (res.inf, res.two_sq, res.bad) == (2.0, 9.0, 0.0)


def test_ipm_entry_points_under_address_and_undefined_behaviour_sanitizers(driver):
    run = subprocess.run([driver], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


def _doubles(a):
    return f"{len(a)} " + " ".join(float(v).hex() for v in a)


def _same(got, want):
    """Bit for bit; a NaN for a NaN (the text form does not carry a NaN's sign and payload)."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(got) & np.isnan(want)
    return got.shape == want.shape and bool(np.all(nan | (got.view(np.uint64) == want.view(np.uint64))))


@pytest.mark.parametrize("length,planted", [(2500, False), (4500, True)])
def test_the_host_walk_matches_the_emulator_bit_for_bit(driver, tmp_path, length, planted):
    b = ip.dirty(length) if planted else ip.boxed(length)
    mu, tau, negate = 0.0625 * 1.37, 0.995, True
    lines = [f"{length} {int(negate)} {float(mu).hex()} {float(tau).hex()}"]
    lines += [_doubles(b[k]) for k in ("lb", "ub", "v", "dv", "zl", "zu", "t", "z")]
    path = tmp_path / "boxed.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([driver, "--dump", str(path)], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
    got = np.array([float.fromhex(t) for t in run.stdout.split()])
    L = length
    cut = np.cumsum([L, L, 8, L, 4, L, L, 4])
    sigma, rbar, rec8, r, rec4, dzl, dzu, rec4b = np.split(got, cut[:-1])
    w_sigma, w_rbar, w_rec8 = ip.emulate_terms(b["lb"], b["ub"], b["v"], b["zl"], b["zu"], mu)
    w_r, w_rec4 = ip.emulate_residual(b["lb"], b["ub"], b["t"], b["z"], negate)
    w_dzl, w_dzu, w_rec4b = ip.emulate_step(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["zu"], mu, tau)
    assert _same(sigma, w_sigma) and _same(rbar, w_rbar) and _same(r, w_r) and _same(dzl, w_dzl) and _same(dzu, w_dzu)
    keep = [q for q in range(8) if q != ip.LOG_SUM]
    assert _same(rec8[keep], w_rec8[keep]), (rec8, w_rec8)
    assert abs(rec8[ip.LOG_SUM] - w_rec8[ip.LOG_SUM]) <= ip.log_bound(b["lb"], b["ub"], b["v"], b["zl"], b["zu"], L)
    assert _same(rec4, w_rec4) and _same(rec4b, w_rec4b), (rec4, w_rec4, rec4b, w_rec4b)
    assert w_rec8[ip.BAD] == (4.0 if planted else 0.0) and w_rec4b[ip.STEP_BAD] == (5.0 if planted else 0.0)
