"""Parallel compilation of the GPU suite's code objects, beside the suite itself.

The GPU tests are sized for a warm code-object cache (pockit_amd/_cache); in a fresh checkout every model is cold and the
suite would spend hours in hipcc, one model after the other.  tests/conftest.py therefore starts, at the beginning of a GPU
session, a second pytest process over the same tests with this plugin (``-p tools.compile_only``) and several xdist
workers.  There the tests run only as far as compiling their models: the library's loader and torch's device
initialisation raise, so nothing reaches a device and every test stops with an error once its evaluator has compiled (or
found) its model; tests that build several models warm the first one.  The session in front finds the objects in the
cache when it gets to them.

``guarded_compile`` keeps the two sessions from compiling one model twice: whoever compiles a model first holds
``<key>.busy`` (its pid) in the cache; another process that needs the same object waits for it (the GPU session) or
leaves it (the compile-only one)."""
import os
import time

import pytest


class CompileOnly(RuntimeError):
    pass


def _refuse(*args, **kwargs):
    raise CompileOnly("compile-only session: no device is used")


def _alive(marker):
    try:
        with open(marker) as fh:
            pid = int(fh.read().strip() or 0)
        os.kill(pid, 0)
        return True
    except (OSError, ValueError):
        return False


def guarded_compile(compile_model, wait, max_wait_s=1800.0):
    """``hipbuild.compile_model`` behind the ``<key>.busy`` marker.  ``wait``: when another live process compiles the same
    object, wait for it (True) or raise CompileOnly (False)."""
    from pockit_amd import hipbuild

    def compile_guarded(source, fastmath=False, keep_source=None, extra_flags=()):
        key = hipbuild._key(source, fastmath, extra_flags)
        obj = os.path.join(hipbuild.CACHE_DIR, key + ".hsacoz")
        busy = os.path.join(hipbuild.CACHE_DIR, key + ".busy")
        t0 = time.monotonic()
        while not os.path.exists(obj):
            try:
                os.makedirs(hipbuild.CACHE_DIR, exist_ok=True)
                fd = os.open(busy, os.O_CREAT | os.O_EXCL | os.O_WRONLY)
            except FileExistsError:
                if not _alive(busy):            # (left by a process that ended while compiling)
                    try:
                        os.remove(busy)
                    except OSError:
                        pass
                    continue
                if not wait:
                    raise CompileOnly("another process compiles this model") from None
                if time.monotonic() - t0 > max_wait_s:
                    break
                time.sleep(0.2)
                continue
            with os.fdopen(fd, "w") as fh:
                fh.write(str(os.getpid()))
            try:
                return compile_model(source, fastmath, keep_source, extra_flags)
            finally:
                try:
                    os.remove(busy)
                except OSError:
                    pass
        return compile_model(source, fastmath, keep_source, extra_flags)

    return compile_guarded


def remove_stale_markers():
    from pockit_amd import hipbuild

    if os.path.isdir(hipbuild.CACHE_DIR):
        for name in os.listdir(hipbuild.CACHE_DIR):
            path = os.path.join(hipbuild.CACHE_DIR, name)
            if name.endswith(".busy") and not _alive(path):
                try:
                    os.remove(path)
                except OSError:
                    pass


def pytest_configure(config):
    import torch

    from pockit_amd import hipbuild, runtime

    hipbuild.compile_model = guarded_compile(hipbuild.compile_model, wait=False)
    runtime.load_library = _refuse
    runtime.Context.__init__ = _refuse
    torch.cuda._lazy_init = _refuse
    torch.cuda.is_available = lambda: False
    torch.cuda.device_count = lambda: 0


@pytest.hookimpl(tryfirst=True)
def pytest_collection_modifyitems(config, items):
    # tests that start processes of their own would open the device in them
    items[:] = [it for it in items if "two_process" not in it.nodeid]
