"""The C-ABI library builds, loads and exports every symbol its two headers (include/pockit_hip.h, the stable surface, and
pockit_amd/csrc/pockit_hip_internal.h) declare, and the ctypes prototypes agree with them; without a
GPU the product fails loudly (no CPU fallback).  No compute calls are made here."""
import ctypes as C
import os
import re

import pytest

from pockit_amd import hipbuild, runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


HEADERS = [os.path.join(ROOT, "include", "pockit_hip.h"), os.path.join(ROOT, "pockit_amd", "csrc", "pockit_hip_internal.h")]


def _declarations(path):
    """{name: (return type, [parameter declarations])} of the functions a C header declares (comments removed first)."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    found = {}
    for ret, name, params in re.findall(r"^\s*((?:const\s+)?\w+\s*\**)\s*\b(pk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        params = " ".join(params.split())
        found[name] = (" ".join(ret.split()).replace(" *", "*"), [] if params in ("", "void") else [q.strip() for q in params.split(",")])
    return found


def test_library_exports_every_declared_symbol():
    hipbuild.build_runtime()
    lib = runtime.load_library()
    stable, internal = (set(_declarations(path)) for path in HEADERS)
    assert stable and internal, "no declarations parsed"
    assert not stable & internal, "a function is declared in both headers"
    assert stable | internal == set(runtime.EXPORTS)
    assert len(runtime.EXPORTS) == len(set(runtime.EXPORTS))
    for name in stable | internal:
        assert getattr(lib, name) is not None


def test_prototype_table_agrees_with_the_headers():
    """runtime.PROTOTYPES against the declarations of both headers: the number of parameters, c_double exactly where the
    header passes a double by value, and the return type (int; two const char*, one void, one long)."""
    declared = {}
    for path in HEADERS:
        declared.update(_declarations(path))
    assert set(declared) == set(runtime.PROTOTYPES)
    returns = {"int": C.c_int, "const char*": C.c_char_p, "void": None, "long": C.c_long}
    seen = []
    for name, (ret, params) in declared.items():
        restype, argtypes = runtime.PROTOTYPES[name]
        assert len(argtypes) == len(params), name
        by_value_double = [bool(re.match(r"^double\s+\w+$", q)) for q in params]
        assert [t is C.c_double for t in argtypes] == by_value_double, name
        assert ret in returns and restype is returns[ret], name
        seen.append(ret)
    assert (seen.count("const char*"), seen.count("void"), seen.count("long")) == (2, 1, 1)
    lib = runtime.load_library()
    for name, (restype, argtypes) in runtime.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_struct_sizes_match_the_c_abi():
    # csrc/pk_abi.h: PkPhase 30 ints, PkTile 22 ints, PkKind 8 ints, PkItem {int64, double, int32, int32}
    assert runtime.PHASE_DTYPE.itemsize == 30 * 4
    assert runtime.TILE_DTYPE.itemsize == 22 * 4
    assert runtime.KIND_DTYPE.itemsize == 8 * 4
    assert runtime.ITEM_DTYPE.itemsize == 24
    assert runtime.OUTER_DTYPE.itemsize == 40
    assert runtime.ERRIV_DTYPE.itemsize == 48
    assert C.sizeof(runtime.ModelDesc) == 29 * 4


def test_numpy_mirrors_agree_with_the_compiled_structs(tmp_path):
    """sizeof / offsetof of csrc/pk_abi.h and include/pockit_hip.h as g++ lays them out."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sizes.cpp"
    src.write_text(
        '#include <cstdio>\n#include <cstddef>\n#include "pockit_amd/csrc/pk_abi.h"\n#include "include/pockit_hip.h"\n'
        'int main() { std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(PkPhase), sizeof(PkTile), '
        "sizeof(PkKind), sizeof(PkItem), sizeof(PkOuter), sizeof(PkErrIv), offsetof(PkErrIv, out_off), "
        "offsetof(PkErrIv, width), sizeof(pk_model_desc), sizeof(pk_problem_desc)); }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["g++", "-I", root, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [runtime.PHASE_DTYPE.itemsize, runtime.TILE_DTYPE.itemsize, runtime.KIND_DTYPE.itemsize,
            runtime.ITEM_DTYPE.itemsize, runtime.OUTER_DTYPE.itemsize, runtime.ERRIV_DTYPE.itemsize,
            runtime.ERRIV_DTYPE.fields["out_off"][1], runtime.ERRIV_DTYPE.fields["width"][1],
            C.sizeof(runtime.ModelDesc), C.sizeof(runtime.ProblemDesc)]
    assert got == want


LAUNCH_TABLE_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "pockit_amd/csrc/pk_launch.h"
int main(int argc, char** argv) {      // the int32 fields of pk_model_desc in order, then n_tiles, split_xall, exchange, layout
  const int nf = (int)(sizeof(pk_model_desc) / sizeof(int32_t));
  if (argc != 1 + nf + 4) return 2;
  pk_model_desc md;
  for (int i = 0; i < nf; ++i) reinterpret_cast<int32_t*>(&md)[i] = std::atoi(argv[1 + i]);
  PkLaunchFacts p;
  p.n_tiles = std::atoi(argv[1 + nf]); p.split_xall = std::atoi(argv[2 + nf]) != 0;
  p.exchange = std::atoi(argv[3 + nf]) != 0; p.layout = std::atoi(argv[4 + nf]);
  for (int k = 0; k < K_COUNT; ++k) {
    const PkLaunchShape s = pk_launch_shape(k, md, p);
    std::printf("%s %u %zu\n", kKernelNames[k], s.grid, s.lds_bytes);
  }
}
"""


@pytest.fixture(scope="module")
def launch_table(tmp_path_factory):
    """csrc/pk_launch.h as a program: (model descriptor, tiles, split, exchange, layout) -> {kernel: (grid, LDS bytes)}."""
    import subprocess

    d = tmp_path_factory.mktemp("launch_table")
    (d / "table.cpp").write_text(LAUNCH_TABLE_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-I", ROOT, str(d / "table.cpp"), "-o", str(d / "table")], check=True)

    def ask(md, n_tiles=0, split=False, exchange=False, layout=0):
        fields = [str(getattr(md, name)) for name, _ in md._fields_]
        out = subprocess.run([str(d / "table")] + fields + [str(int(v)) for v in (n_tiles, split, exchange, layout)],
                             check=True, capture_output=True, text=True).stdout
        return {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in out.splitlines()}

    return ask


def _launch_sources():
    """(name, plan, ModelSource arguments): a small example, two_stage_rocket, a model evaluated in groups, wide models with
    both table capacities (the models of tests/test_codegen_groups.py)."""
    import models
    import pockit_amd.radau as radau
    from pockit_amd import benchmarks

    yield "brachistochrone", models.brachistochrone(radau, 2, 3)[0].plan, {}
    yield "two_stage_rocket", models.two_stage_rocket(radau, 3, 2)[0].plan, {}
    yield "humanoid_wbc in groups of 16", benchmarks.humanoid_wbc(radau, mesh=25, num_point=8)[0].plan, {"group_cap": 16}
    yield "state_chain 24 states", benchmarks.state_chain(radau, states=24, mesh=40, num_point=4)[0].plan, {}
    yield "state_chain 52 states, 12 points", benchmarks.state_chain(radau, states=52, mesh=7, num_point=12)[0].plan, {"group_cap": 16}


def test_the_code_generator_counts_lds_bytes_as_the_launch_table_does(launch_table, monkeypatch):
    """ModelSource.launch_lds_bytes (what compile_plan chooses the group size with) against csrc/pk_launch.h (what the library
    launches with and pk_load_model checks): equal for every kernel of a single-GPU code object; for a sharded one Python
    counts the exchange vectors of pk_cycle / pk_cyclec in front of the table block instead of under it, so it may only be
    larger there.  Python's pk_cyclec is the layout with every compact role the model has."""
    from pockit_amd.codegen import ModelSource
    from pockit_amd.evaluator import model_desc

    for key in ("POCKIT_AMD_GROUP_CAP", "POCKIT_AMD_PASS_PARALLEL", "POCKIT_AMD_IPW", "POCKIT_AMD_TAB_CAP"):
        monkeypatch.delenv(key, raising=False)
    seen = {"grouped": False, "wide": False, 64: False, 256: False}
    for name, plan, kw in _launch_sources():
        for sharded in (False, True):
            src = ModelSource(plan, sharded=sharded, **kw)
            seen["grouped"] |= bool(src.cycle_subs)
            seen["wide"] |= any(src.wide)
            seen[src.tab_cap] = True
            table = launch_table(model_desc(src), exchange=sharded, layout=1 | (2 if src.compact else 0))
            mirror = src.launch_lds_bytes()
            assert {"pk_g", "pk_jac", "pk_hess", "pk_xall", "pk_cycle", "pk_jacc", "pk_cyclec"} <= set(mirror)
            for kernel, nbytes in mirror.items():
                if sharded and kernel in ("pk_cycle", "pk_cyclec"):
                    assert nbytes >= table[kernel][1], (name, kernel)
                else:
                    assert nbytes == table[kernel][1], (name, kernel, sharded)
    assert all(seen.values()), seen


@pytest.mark.parametrize("tiles", [4, 1024, 1028, 4000])
@pytest.mark.parametrize("subs", [0, 7])
def test_the_tiling_rule_counts_the_workgroups_of_the_cycle_as_the_launch_table_does(launch_table, tiles, subs):
    """evaluator._intervals_per_wave weighs a tiling by ``roles * tiles // WAVES_PER_BLOCK + 3`` workgroups with 3 roles up to
    1024 tiles (where pk_set_problem splits the x-part), 2 beyond, or the model's cycle_subs: the grid of pk_cycle."""
    from pockit_amd import runtime

    md = runtime.ModelDesc()
    md.tab_cap, md.cycle_subs, md.hess_subs = 64, subs, (3 if subs else 0)
    roles = subs or (3 if tiles <= 1024 else 2)
    assert tiles % runtime.WAVES_PER_BLOCK == 0      # (the rule pads every phase to whole tile blocks)
    grid = launch_table(md, n_tiles=tiles, split=tiles <= 1024)["pk_cycle"][0]
    assert grid == roles * tiles // runtime.WAVES_PER_BLOCK + 3


def test_no_gpu_means_loud_failure():
    lib = runtime.load_library()
    if lib.pk_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no HIP device|pk_create failed"):
        runtime.Context(0)
    import models
    import pockit_amd.radau as radau

    system, _, guess = models.brachistochrone(radau, 2, 3)
    x = models.pack_guess(system, guess)
    with pytest.raises(RuntimeError):
        system.objective(x)


def test_generated_code_cross_compiles_for_gfx950():
    import models
    import pockit_amd.radau as radau
    from pockit_amd.codegen import ModelSource

    system, _, _ = models.two_stage_rocket(radau, 3, 2)
    src = ModelSource(system.plan)
    code = hipbuild.compile_model(src.source)
    assert (code[:4] == b"\x7fELF" or code.startswith(b"__CLANG_OFFLOAD_BUNDLE__")) and len(code) > 1000
    for k in runtime.KERNELS:
        assert k.encode() in code
