"""The host runtime behind the C ABI (the units of pockit_amd.hipbuild.RUNTIME_SOURCES: pinned landing blocks, double-buffered staging,
prepared-x protocol, copy batching, polling waits, speculative Hessian, constant Jacobian runs, CSR run tables) built with
``-fsanitize=address,undefined`` against a host-only stand-in of the HIP runtime (tests/fake_hip: deferred streams, "kernels"
that write recomputable values) and driven through its protocols by tests/fake_hip/driver.cpp.  CPU only -- GPU sanitizers are
not available on this pool.  SURVEY.md section 5 "race detection / sanitizers"."""
import os
import shutil
import subprocess

import pytest

from pockit_amd.hipbuild import POOL_SOURCES
from sanitized_build import sanitized_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_hip")


SANITIZER_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def driver_exe(tmp_path_factory):
    """tests/fake_hip/driver.cpp + the runtime + the stand-in, built once with the address and undefined-behaviour sanitizers."""
    return sanitized_driver("driver.cpp", tmp_path_factory.mktemp("runtime"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_runtime_under_address_and_undefined_behaviour_sanitizers(driver_exe):
    env = dict(os.environ, **SANITIZER_ENV)
    run = subprocess.run([driver_exe], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_launch_shapes_are_those_of_the_recorded_trace(driver_exe):
    """Grid, dynamic LDS bytes and kernel-argument bytes of every launch, and the order of copies and kernels of every entry
    point, over the driver's scenarios and over descriptors that reach every row of csrc/pk_launch.h: byte for byte what
    tests/fake_hip/launch_trace.txt recorded from the runtime BEFORE the launch shapes moved into that table (its first
    line names the commit).  The file is a recording of that commit, never regenerated from the code under test."""
    with open(os.path.join(FAKE, "launch_trace.txt")) as fh:
        head, recorded = fh.read().split("\n", 1)
    assert head.startswith("# ")
    env = dict(os.environ, **SANITIZER_ENV)
    run = subprocess.run([driver_exe, "--launch-trace"], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
    assert run.stdout == recorded


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_host_helper_threads_under_sanitizers(tmp_path, sanitizer):
    """pk_host_threads / pk_same_bits / pk_copy_bits (the helper threads that take slices of rank 0's passes over x and
    lambda in the host-landed sharded cycle): ThreadSanitizer and AddressSanitizer builds of the same source, driven by
    tests/fake_hip/pool_driver.cpp through hot and cold helpers, every pass length class, differences at either end."""
    exe = str(tmp_path / "pk_pool_sanitized")
    cmd = ["g++", "-std=c++17", "-g", "-O1", f"-fsanitize={sanitizer}", "-fno-omit-frame-pointer", "-pthread", "-I", ROOT] + POOL_SOURCES + [
               os.path.join(FAKE, "pool_driver.cpp"), "-o", exe]      # (the pool's two units alone: no stand-in of HIP needed)
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    if sanitizer == "thread" and run.returncode != 0 and "unexpected memory mapping" in run.stderr:
        # (ThreadSanitizer cannot place its shadow under this kernel's address-space randomisation: once more without it)
        if shutil.which("setarch") is None:
            pytest.skip("ThreadSanitizer cannot start on this kernel (unexpected memory mapping) and setarch is missing")
        run = subprocess.run(["setarch", "-R", exe], capture_output=True, text=True, env=env, timeout=600)
        if run.returncode != 0 and ("unexpected memory mapping" in run.stderr or "setarch" in run.stderr):
            pytest.skip("ThreadSanitizer cannot start on this kernel (unexpected memory mapping)")
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-6000:])
    assert "checks passed" in run.stdout and "WARNING: ThreadSanitizer" not in run.stderr and "ERROR" not in run.stderr
