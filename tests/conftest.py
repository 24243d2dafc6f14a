import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_sessionstart(session):
    # a session on a GPU box (gpurun_out/ exists): log every code object that had to be compiled, in this process or a child
    out = os.path.join(ROOT, "gpurun_out")
    if os.environ.get("GRAFT_REPO_ROOT") and os.path.isdir(out) and "POCKIT_AMD_COMPILE_LOG" not in os.environ:
        os.environ["POCKIT_AMD_COMPILE_LOG"] = os.path.join(out, "compiled_keys.txt")
        os.environ.setdefault("POCKIT_AMD_USED_LOG", os.path.join(out, "used_keys.txt"))      # every object the suite was served
        for name in ("POCKIT_AMD_COMPILE_LOG", "POCKIT_AMD_USED_LOG"):
            try:
                os.remove(os.environ[name])
            except OSError:
                pass


@pytest.hookimpl(trylast=True)
def pytest_collection_modifyitems(config, items):
    """A GPU session on a machine with a device: compile the selected tests' models in a second process with several
    workers while the tests run (tools/compile_only.py) -- a fresh checkout has none of them in pockit_amd/_cache.
    POCKIT_AMD_PREFETCH=0 turns this off."""
    gpu = [it.nodeid for it in items if it.get_closest_marker("gpu")]
    if (not gpu or os.environ.get("POCKIT_AMD_COMPILE_ONLY") or os.environ.get("PYTEST_XDIST_WORKER")
            or os.environ.get("POCKIT_AMD_PREFETCH", "1") == "0" or not os.path.exists("/dev/kfd")):
        return
    import subprocess
    import tempfile

    from pockit_amd import hipbuild
    from tools import compile_only

    compile_only.remove_stale_markers()
    hipbuild.compile_model = compile_only.guarded_compile(hipbuild.compile_model, wait=True)
    fd, ids = tempfile.mkstemp(prefix="pockit_amd_gpu_tests_", suffix=".txt")
    with os.fdopen(fd, "w") as fh:
        fh.write("\n".join(gpu) + "\n")
    cpus = min(16, int(os.environ.get("MAX_JOBS") or 0) or len(os.sched_getaffinity(0)))
    jobs = []
    try:
        import xdist  # noqa: F401

        if cpus > 3:
            jobs = ["-n", str(cpus - 2)]        # (two CPUs stay with the session that drives the GPU)
    except ImportError:
        pass
    env = dict(os.environ, POCKIT_AMD_COMPILE_ONLY="1", POCKIT_AMD_COMPILE_LOG=os.devnull, POCKIT_AMD_USED_LOG=os.devnull,
               PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    proc = subprocess.Popen([sys.executable, "-m", "pytest", "@" + ids, "-q", "-p", "no:cacheprovider", "-p", "tools.compile_only",
                             "--tb=no", "--no-header", "--disable-warnings", "-rN"] + jobs,
                            cwd=str(config.rootpath), env=env, stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL,
                            stderr=subprocess.DEVNULL, start_new_session=True)
    config._pockit_prefetch = (proc, ids)


def pytest_unconfigure(config):
    prefetch = getattr(config, "_pockit_prefetch", None)
    if prefetch is None:
        return
    import signal
    import subprocess

    proc, ids = prefetch
    if proc.poll() is None:
        try:
            os.killpg(proc.pid, signal.SIGTERM)
            proc.wait(timeout=20)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)
            proc.wait()
        except OSError:
            pass
    try:
        os.remove(ids)
    except OSError:
        pass
    from tools import compile_only

    compile_only.remove_stale_markers()


def pytest_terminal_summary(terminalreporter):
    """How much of the session went into hipcc: the GPU suite is sized for a warm code-object cache (pockit_amd/_cache, filled
    without a GPU by tools/warm_cache.sh and shipped with the tree).  Objects compiled here mean the cache was cold for them
    (tests that build several models stop at the first one when warmed without a GPU).  On a GPU box they are copied to
    gpurun_out/cache_new/ (<= 48 MB), from where ``cp gpurun_out/cache_new/* pockit_amd/_cache/`` completes the local cache."""
    log = os.environ.get("POCKIT_AMD_COMPILE_LOG")
    if not log or not os.path.exists(log):
        return
    rows = [ln.split() for ln in open(log) if ln.strip()]
    if not rows:
        return
    total = sum(float(r[1]) for r in rows if len(r) > 1)
    terminalreporter.write_line(f"[pockit_amd] {len(rows)} code object(s) were compiled in this session ({total:.0f} s of hipcc): "
                                f"cold cache entries")
    try:
        import shutil

        from pockit_amd import hipbuild

        dst = os.path.join(os.path.dirname(log), "cache_new")
        os.makedirs(dst, exist_ok=True)
        used = 0
        for key in dict.fromkeys(r[0] for r in rows):
            for ext in (".hsacoz", ".gen", ".res.json"):
                src = os.path.join(hipbuild.CACHE_DIR, key + ext)
                if os.path.exists(src) and used + os.path.getsize(src) < 48 * 2**20:
                    shutil.copy(src, dst)
                    used += os.path.getsize(src)
        terminalreporter.write_line(f"[pockit_amd] copied {used / 2**20:.1f} MB of new objects to {dst}")
    except Exception as exc:  # noqa: BLE001
        terminalreporter.write_line(f"[pockit_amd] could not export the new objects: {exc!r}")
