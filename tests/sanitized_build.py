"""One place that builds a driver program of tests/fake_hip with ``-fsanitize=address,undefined``: the host runtime (the units of
pockit_amd.hipbuild.RUNTIME_SOURCES) and the host-only stand-in of the HIP runtime are compiled to object files once per
process, a driver is compiled and linked against them per request.  Every result is a stand-alone program with its own main:
nothing sanitized is loaded into Python.  A plain helper module, imported by the tests that run such a driver."""
import atexit
import os
import shutil
import subprocess
import tempfile

from pockit_amd.hipbuild import RUNTIME_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_hip")
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
         "-fno-sanitize-recover=undefined", "-I", FAKE, "-I", ROOT]

_objects = None      # the runtime's and the stand-in's object files, once they are built


def _compile(args):
    build = subprocess.run(["g++"] + FLAGS + args, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]


def _runtime_objects():
    global _objects
    if _objects is None:
        work = tempfile.mkdtemp(prefix="pk_sanitized_")
        atexit.register(shutil.rmtree, work, ignore_errors=True)
        sources = RUNTIME_SOURCES + [os.path.join(FAKE, "fake_hip.cpp")]
        objects = [os.path.join(work, os.path.basename(s)[:-len(".cpp")] + ".o") for s in sources]
        for source, obj in zip(sources, objects):
            _compile(["-c", source, "-o", obj])
        _objects = objects
    return _objects


def sanitized_driver(driver, directory):
    """Path of tests/fake_hip/<driver> (a file name, e.g. ``"ops_driver.cpp"``) built into ``directory`` against the
    sanitized runtime and stand-in."""
    exe = os.path.join(str(directory), os.path.splitext(driver)[0] + "_sanitized")
    _compile([os.path.join(FAKE, driver)] + _runtime_objects() + ["-o", exe])
    return exe
