"""The runtime unit behind the MINRES solve (pockit_amd/csrc/pk_minres.cpp) built with ``-fsanitize=address,undefined`` against the
host-only stand-in of the HIP runtime and driven by tests/fake_hip/minres_driver.cpp: the stand-in walk of every vector step
against plain loops, the split index at its boundary values, K with and without H, s1 and s2, the refusals, the host form against
begin / advance / record, what frees and forgets the state; with ``--dump`` two synthetic solves compared BIT FOR BIT with the
emulator of tests/minres_cases.py, so the documented association is held on the CPU as well.  (That the unit leaves what the
runtime enqueues elsewhere as tests/fake_hip/launch_trace.txt recorded it is tests/test_runtime_sanitized.py's test of the
launch shapes.)  CPU only; a stand-alone program (its own main): nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import minres_cases as mr
import sparse_cases as sc
from sanitized_build import sanitized_driver

ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sanitized_driver("minres_driver.cpp", tmp_path_factory.mktemp("minres_driver"))


def test_the_unit_is_part_of_the_library_and_of_the_binding():
    from pockit_amd import runtime
    from pockit_amd.hipbuild import RUNTIME_SOURCES

    assert any(os.path.basename(s) == "pk_minres.cpp" for s in RUNTIME_SOURCES)
    for name, count in (("pk_kkt_apply_dev", 8), ("pk_kkt_apply", 6), ("pk_minres_begin_dev", 11), ("pk_minres_advance_dev", 3),
                        ("pk_minres_record", 2), ("pk_solve_kkt", 13), ("pk_minres_step_dev", 20)):
        assert len(runtime.PROTOTYPES[name][1]) == count


def test_the_python_layer_offers_the_solve():
    from pockit_amd.evaluator import Evaluator, Linearization, MinresInfo

    for name in ("kkt_v", "kkt_operator", "kkt_precond", "solve_kkt"):
        assert callable(getattr(Linearization, name))
    for name in ("kkt_apply_dev", "minres_begin_dev", "minres_advance_dev", "minres_record"):
        assert callable(getattr(Evaluator, name))
    rec = np.zeros(16)
    rec[:4] = 1.0, 7.0, 2.0e-9, 4.0e-8
    x = np.arange(5.0)
    info = MinresInfo(rec, 1e-8, x, 3)
    assert (info.status, info.iterations) == ("converged", 7) and info.rel_residual == 2.0e-9 / 4.0e-8 * 1e-8
    assert np.shares_memory(info.primal, x) and info.primal.shape == (3,) and info.dual.shape == (2,)
    assert [MinresInfo.STATUS[k] for k in (1, 2, 3, 4)] == ["converged", "preconditioner_not_positive", "non_finite", "maxiter"]
    with pytest.raises(AttributeError):
        info.status = "x"


def test_minres_entry_points_under_address_and_undefined_behaviour_sanitizers(driver):
    run = subprocess.run([driver], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


def _ints(a):
    return f"{len(a)} " + " ".join(str(int(v)) for v in a)


def _doubles(a):
    return f"{len(a)} " + " ".join(float(v).hex() for v in a)


@pytest.mark.parametrize("ctx,family,with_h,pre", [("A", "eq", True, True), ("B", "quasi", True, True), ("A", "quasi", False, False)])
def test_the_host_walk_matches_the_emulator_bit_for_bit(driver, tmp_path, ctx, family, with_h, pre):
    kk = mr.kkt(ctx)
    sy, c = kk.sy, sc.CONTEXTS[ctx]
    inp = kk.inputs(family, with_h)
    minv = kk.precond(with_h, inp["s1"], inp["s2"]) if pre else np.zeros(0)
    x0 = inp["x0"] if pre else np.zeros(0)
    s2 = np.zeros(0) if inp["s2"] is None else inp["s2"]
    tol, maxiter, chunk = 1e-8, 400, 5
    lines = [f"{sy.n} {sy.m} {c['nnz_j']} {c['nnz_h']} {int(with_h)} {int(inp['s2'] is not None)} {int(pre)} {int(pre)} {maxiter} {chunk} "
             f"{float(tol).hex()}"]
    for st in (sy.J, sy.JT, sy.H):
        lines += [_ints(st.indptr), _ints(st.indices), _ints(st.src)]
    lines += [_doubles(a) for a in (sy.jvals, sy.hvals, inp["s1"], s2, minv, inp["b"], x0)]
    path = tmp_path / "solve.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([driver, "--dump", str(path)], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
    got = np.array([float.fromhex(t) for t in run.stdout.split()])
    rec, x = got[:16], got[16:]
    want_x, want_rec = mr.emulate_solve(kk, with_h, inp["s1"], inp["s2"], minv if pre else None, inp["b"], x0 if pre else None, tol, maxiter,
                                        check_every=chunk)
    assert want_rec[mr.STATUS] == 1.0
    assert sc.same_bits(rec, want_rec), (rec, want_rec)
    assert sc.same_bits(x, want_x)
