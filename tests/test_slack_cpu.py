"""The runtime unit behind the slacks of a resident iterate (pockit_amd/csrc/pk_slack.cpp) built with
``-fsanitize=address,undefined`` against the host-only stand-in of the HIP runtime and driven by tests/fake_hip/slack_driver.cpp:
the stand-in walk of every kernel against plain loops at the lengths where the pieces and the strided scalar step change shape,
clean and with planted defects, batches of 1, 3 and 64 trial points, the public forms against the raw form, the host forms
against the device forms, the refusals with their codes and sentinels, what frees the state; with ``--dump`` the vectors of
tests/slack_cases.py compared BIT FOR BIT with its emulator (the sum of logarithms within the bound of two implementations of
log), so the documented association is held on the CPU as well.  CPU only; a stand-alone program (its own main): nothing
sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import slack_cases as sl
from sanitized_build import sanitized_driver

ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sanitized_driver("slack_driver.cpp", tmp_path_factory.mktemp("slack_driver"))


def test_the_unit_is_part_of_the_library_and_of_the_binding():
    from pockit_amd import runtime
    from pockit_amd.hipbuild import RUNTIME_SOURCES

    assert any(os.path.basename(s) == "pk_slack.cpp" for s in RUNTIME_SOURCES)
    for name, count in (("pk_slack_reduce_dev", 10), ("pk_slack_recover_dev", 12), ("pk_slack_update_dev", 16), ("pk_slack_merit_dev", 9),
                        ("pk_slack_reduce", 9), ("pk_slack_recover", 11), ("pk_slack_update", 15), ("pk_slack_raw_dev", 16)):
        assert len(runtime.PROTOTYPES[name][1]) == count


def test_the_python_layer_offers_the_capabilities():
    from pockit_amd.evaluator import Evaluator, IterateUpdate, SlackStep, SlackTerms

    for name in ("slack_reduce_dev", "slack_recover_dev", "slack_update_dev", "slack_merit_dev", "slack_terms", "slack_step", "update_iterate"):
        assert callable(getattr(Evaluator, name))
    terms = SlackTerms(np.arange(3.0), -np.arange(3.0), [0.5, 6.0, 0.0, 2.0])
    assert (terms.theta_inf, terms.theta_1, terms.bad, terms.inequalities) == (0.5, 6.0, 0.0, 2.0) and terms.s2[2] == 2.0 and terms.b2[2] == -2.0
    with pytest.raises(AttributeError):
        terms.bad = 1.0
    with pytest.raises(ValueError):
        terms.s2[0] = 1.0
    step = SlackStep(np.ones(2), [3.0, 1.0, 2.0, 0.5, 0.0])
    assert (step.curvature, step.step_sq, step.bad) == (4.0, 2.5, 0.0) and step.ds[1] == 1.0 and step.accepts(1.0) and not step.accepts(2.0)
    upd = IterateUpdate(np.zeros(2), np.ones(2), np.ones(2), None, [1.0, 0.25, 0.0, 0.0])
    assert (upd.clamped, upd.min_slack, upd.bad) == (1.0, 0.25, 0.0) and upd.lam is None and upd.zu[1] == 1.0


def test_slack_entry_points_under_address_and_undefined_behaviour_sanitizers(driver):
    run = subprocess.run([driver], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


def _doubles(a):
    a = np.asarray(a, dtype=np.float64).ravel()
    return f"{len(a)} " + " ".join(float(v).hex() for v in a)


def _same(got, want):
    """Bit for bit; a NaN for a NaN (the text form does not carry a NaN's sign and payload)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(got) & np.isnan(want)
    return got.shape == want.shape and bool(np.all(nan | (got.view(np.uint64) == want.view(np.uint64))))


@pytest.mark.parametrize("n,m,planted", [(2500, 4500, False), (4500, 2500, True)])
def test_the_host_walk_matches_the_emulator_bit_for_bit(driver, tmp_path, n, m, planted):
    x, b = sl.variables(n), sl.rows(m)
    batch, ap, ad, mu, kappa = 3, 0.8125 * 0.93, 0.71, 0.0625 * 1.37, 10.0
    X, G, alphas = sl.trial_points(x, b, batch)
    if planted:
        sl.plant(x, b, X, G)
    lines = [f"{n} {m} {batch} " + " ".join(float(v).hex() for v in (ap, ad, mu, kappa))]
    lines += [_doubles(a) for a in (x["lb"], x["ub"], b["lb"], b["ub"])]
    lines += [_doubles(b[k]) for k in ("g", "s", "lam", "dlam", "sigma_s", "rbar_s", "s2", "ds", "dv", "zl", "zu", "dzl", "dzu")]
    lines += [_doubles(x[k]) for k in ("dx", "w", "s1")] + [_doubles(X), _doubles(G), _doubles(alphas)]
    path = tmp_path / "slack.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([driver, "--dump", str(path)], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
    got = np.array([float.fromhex(t) for t in run.stdout.split()])
    cut = np.cumsum([m, m, 4, m, 5, m, m, m, m, 4, 4 * batch])
    s2, b2, rec4, ds, rec5, v, zl, zu, lam, rec4b, table = np.split(got, cut[:-1])
    w_s2, w_b2, w_rec4 = sl.emulate_reduce(b["lb"], b["ub"], b["g"], b["s"], b["lam"], b["sigma_s"], b["rbar_s"])
    w_ds, w_rec5 = sl.emulate_recover(x["lb"], x["ub"], b["lb"], b["ub"], b["dlam"], b["lam"], b["rbar_s"], b["s2"], b["sigma_s"], x["dx"], x["w"],
                                      x["s1"])
    w_v, w_zl, w_zu, w_lam, w_rec4b = sl.emulate_update(b["lb"], b["ub"], b["v"], b["dv"], b["zl"], b["dzl"], b["zu"], b["dzu"], ap, ad, mu, kappa,
                                                        b["lam"], b["dlam"])
    w_table = sl.emulate_merit(x["lb"], x["ub"], b["lb"], b["ub"], X, G, b["s"], b["ds"], alphas)
    for name, g, w in (("s2", s2, w_s2), ("b2", b2, w_b2), ("reduce record", rec4, w_rec4), ("ds", ds, w_ds), ("recover record", rec5, w_rec5),
                       ("v", v, w_v), ("zl", zl, w_zl), ("zu", zu, w_zu), ("lam", lam, w_lam), ("update record", rec4b, w_rec4b)):
        assert _same(g, w), (name, g, w)
    table = table.reshape(batch, 4)
    keep = [q for q in range(4) if q != sl.M_LOG]
    assert _same(table[:, keep], w_table[:, keep]), (table, w_table)
    for k in range(batch):
        bound = sl.merit_log_bound(x["lb"], x["ub"], b["lb"], b["ub"], X[k], b["s"] + alphas[k] * b["ds"])
        assert abs(table[k, sl.M_LOG] - w_table[k, sl.M_LOG]) <= bound
    if planted:
        assert (w_rec4[sl.RED_BAD], w_rec5[sl.REC_BAD], w_rec4b[sl.UPD_BAD]) == (3.0, 3.0, 3.0) and w_table[:, sl.M_BAD].tolist() == [2.0, 2.0, 3.0]
    else:
        assert w_rec4[sl.RED_BAD] == w_rec5[sl.REC_BAD] == w_rec4b[sl.UPD_BAD] == 0.0 and not w_table[:, sl.M_BAD].any()
