"""The runtime unit behind the CG solve (pockit_amd/csrc/pk_cg.cpp) built with ``-fsanitize=address,undefined`` against the
host-only stand-in of the HIP runtime and driven by tests/fake_hip/cg_driver.cpp: the stand-in walk of every vector step against
plain loops, K in both forms, the refusals, the host form against begin / advance / record, what frees and forgets the state; with
``--dump`` one synthetic solve compared BIT FOR BIT with the emulator of tests/cg_cases.py, so the documented association is held
on the CPU as well.  (That the unit leaves what the runtime enqueues elsewhere as tests/fake_hip/launch_trace.txt recorded it is
tests/test_runtime_sanitized.py's test of the launch shapes.)  CPU only; a stand-alone program (its own main): nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cg_cases as cg
import sparse_cases as sc
from sanitized_build import sanitized_driver

ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sanitized_driver("cg_driver.cpp", tmp_path_factory.mktemp("cg_driver"))


def test_the_unit_is_part_of_the_library_and_of_the_binding():
    from pockit_amd import runtime
    from pockit_amd.hipbuild import RUNTIME_SOURCES

    assert any(os.path.basename(s) == "pk_cg.cpp" for s in RUNTIME_SOURCES)
    for name, count in (("pk_condensed_apply_dev", 9), ("pk_condensed_apply", 7), ("pk_cg_begin_dev", 12), ("pk_cg_advance_dev", 3),
                        ("pk_cg_record", 2), ("pk_solve_condensed", 14), ("pk_cg_step_dev", 15)):
        assert len(runtime.PROTOTYPES[name][1]) == count


def test_cg_entry_points_under_address_and_undefined_behaviour_sanitizers(driver):
    run = subprocess.run([driver], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


def _ints(a):
    return f"{len(a)} " + " ".join(str(int(v)) for v in a)


def _doubles(a):
    return f"{len(a)} " + " ".join(float(v).hex() for v in a)


@pytest.mark.parametrize("ctx,form,family", [("A", 0, "pd"), ("B", 0, "pd"), ("B", 1, "pd"), ("B", 0, "indefinite")])
def test_the_host_walk_matches_the_emulator_bit_for_bit(driver, tmp_path, ctx, form, family):
    sy = cg.system(ctx)
    c = sc.CONTEXTS[ctx]
    inp = sy.inputs(form, family)
    pd = family == "pd"
    minv = sy.jacobi(form, inp["with_h"], inp["d"], inp["s"]) if pd else np.zeros(0)
    x0 = inp["x0"] if pd else np.zeros(0)
    tol, maxiter, chunk = 1e-8, 400, 5
    lines = [f"{sy.n} {sy.m} {c['nnz_j']} {c['nnz_h']} {form} {int(inp['with_h'])} {int(pd)} {int(pd)} {maxiter} {chunk} {float(tol).hex()}"]
    for st in (sy.J, sy.JT, sy.H):
        lines += [_ints(st.indptr), _ints(st.indices), _ints(st.src)]
    lines += [_doubles(a) for a in (sy.jvals, sy.hvals, inp["d"], inp["s"], minv, inp["b"], x0)]
    path = tmp_path / "solve.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([driver, "--dump", str(path)], capture_output=True, text=True, env=dict(os.environ, **ENV), timeout=900)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
    got = np.array([float.fromhex(t) for t in run.stdout.split()])
    rec, x = got[:8], got[8:]
    want_x, want_rec = cg.emulate_solve(sy, form, inp["with_h"], inp["d"], inp["s"], minv if pd else None, inp["b"], x0 if pd else None,
                                        tol, maxiter, check_every=chunk)
    assert want_rec[cg.STATUS] == (1.0 if pd else 2.0)
    assert sc.same_bits(rec, want_rec), (rec, want_rec)
    assert sc.same_bits(x, want_x)
