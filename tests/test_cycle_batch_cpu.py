"""The batched code object (kernel pk_cycleb) and its host plumbing, without a GPU: the source variant and what the compiler
says about it, the launch table's K_CYCLEB row, the three exports."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import pytest

import models
import pockit_amd.radau as radau
from pockit_amd import hipbuild, runtime
from pockit_amd.codegen import ModelSource

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# brachistochrone(radau, 3, 4) on the commit BEFORE the batched kernel existed: sha256 of the generated (non-batched) source,
# the hash of the two kernel headers it was compiled against and the cache key hipbuild._key gave it
PARENT_SOURCE_SHA256 = "629630f95aebaf5eec5500bdefc35222daa783d4c6b28e722b0e8d063e8cdfc8"
PARENT_HEADER_HASH = "b79fd7143ab0"
PARENT_KEY = "f9461d949896671a7b8e8b459e1860e9"

# VGPRs pk_cycleb may need beyond pk_cycle of the same model: the build shows 70 and 70 (the record pointer lives in SGPRs)
VGPR_MARGIN = 0


@pytest.fixture(scope="module")
def plan():
    return models.brachistochrone(radau, 3, 4)[0].plan


def test_batched_source_compiles_to_the_one_kernel_without_spills(plan):
    plain, batched = ModelSource(plan), ModelSource(plan, batched=True)
    assert batched.source != plain.source and "PK_DEFINE_CYCLE_BATCH(pkgen::Gen)" in batched.source
    code = hipbuild.compile_model(batched.source)
    assert (code[:4] == b"\x7fELF" or code.startswith(b"__CLANG_OFFLOAD_BUNDLE__")) and b"pk_cycleb" in code
    usage = hipbuild.resource_usage(batched.source)
    assert list(usage) == [runtime.BATCH_KERNEL] == ["pk_cycleb"]
    mine = usage["pk_cycleb"]
    assert mine["vgpr_spill"] == 0 and mine["scratch"] == 0
    hipbuild.compile_model(plain.source)
    theirs = hipbuild.resource_usage(plain.source)["pk_cycle"]
    assert mine["vgpr"] <= theirs["vgpr"] + VGPR_MARGIN, (mine, theirs)
    assert mine["lds"] == theirs["lds"]
    for name in runtime.KERNELS:      # (no kernel of the model's own object rides along)
        assert name.encode() + b"\x00" not in code, name


def test_the_model_objects_of_every_evaluator_are_what_they_were(plan):
    """The non-batched source is byte for byte the parent's; its cache key too, unless the kernel headers were edited (they
    are part of the key) -- then the kernel list of the object is held instead."""
    src = ModelSource(plan)
    assert "pk_cycleb" not in src.source and "PK_DEFINE_CYCLE_BATCH" not in src.source
    assert hashlib.sha256(src.source.encode()).hexdigest() == PARENT_SOURCE_SHA256
    if hipbuild._kernel_header_hash() == PARENT_HEADER_HASH:
        assert hipbuild._key(src.source, False) == PARENT_KEY
    else:
        hipbuild.compile_model(src.source)
        assert sorted(hipbuild.resource_usage(src.source)) == sorted(runtime.KERNELS)
        assert runtime.BATCH_KERNEL not in runtime.KERNELS
    with pytest.raises(ValueError):
        ModelSource(plan, sharded=True, batched=True)


SHAPE_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "pockit_amd/csrc/pk_launch.h"
int main(int argc, char** argv) {      // tab_cap lds_x lds_h ne_j ne_h cycle_subs hess_subs n_tiles split
  if (argc != 10) return 2;
  pk_model_desc md{};
  md.tab_cap = std::atoi(argv[1]); md.lds_x = std::atoi(argv[2]); md.lds_h = std::atoi(argv[3]); md.ne_j = std::atoi(argv[4]);
  md.ne_h = std::atoi(argv[5]); md.cycle_subs = std::atoi(argv[6]); md.hess_subs = std::atoi(argv[7]);
  PkLaunchFacts p;
  p.n_tiles = std::atoi(argv[8]); p.split_xall = std::atoi(argv[9]) != 0;
  const PkLaunchShape a = pk_launch_shape(K_CYCLE, md, p), b = pk_launch_shape(K_CYCLEB, md, p);
  std::printf("%s %u %zu %u %s %u %zu %u %d\n", kKernelNames[K_CYCLE], a.grid, a.lds_bytes, a.batch, kKernelNames[K_CYCLEB], b.grid,
              b.lds_bytes, b.batch, (int)PK_MAX_BATCH);
}
"""


@pytest.mark.parametrize("desc", [
    pytest.param((64, 640, 512, 40, 60, 0, 0, 8, 0), id="plain"),
    pytest.param((64, 640, 512, 40, 60, 0, 0, 8, 1), id="split"),
    pytest.param((256, 2048, 4096, 300, 900, 7, 3, 1028, 0), id="grouped"),
])
def test_the_launch_table_gives_the_batched_kernel_the_cycles_shape(tmp_path, desc):
    """csrc/pk_launch.h compiled with the plain C++ compiler: K_CYCLEB has K_CYCLE's x-grid and LDS bytes."""
    (tmp_path / "shape.cpp").write_text(SHAPE_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-I", ROOT, str(tmp_path / "shape.cpp"), "-o", str(tmp_path / "shape")], check=True)
    out = subprocess.run([str(tmp_path / "shape")] + [str(v) for v in desc], check=True, capture_output=True, text=True).stdout.split()
    assert out[0] == "pk_cycle" and out[4] == "pk_cycleb"
    assert out[1:3] == out[5:7] and int(out[1]) > 3 and int(out[2]) > 0
    assert out[3] == out[7] == "1"      # (the y-extent is the launch's: the table knows one entry)
    tiles, split, subs = desc[7], desc[8], desc[5]
    assert int(out[1]) == (subs or (3 if split else 2)) * tiles // 4 + 3
    assert int(out[8]) == runtime.MAX_BATCH == 64


def test_the_three_exports_are_declared_and_prototyped():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "pockit_hip.h")).read(), flags=re.S)
    internal = open(os.path.join(ROOT, "pockit_amd", "csrc", "pockit_hip_internal.h")).read()
    for name, arity in (("pk_load_batch_model", 3), ("pk_set_batch", 2), ("pk_eval_cycle_batch_dev", 13)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^()]*)\)\s*;", text)
        assert m, f"{name} is not declared in the stable header"
        assert len(m.group(1).split(",")) == arity
        assert name not in internal
        restype, argtypes = runtime.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == arity
    assert "pk_batch.cpp" in [os.path.basename(p) for p in hipbuild.RUNTIME_SOURCES]
    hipbuild.build_runtime()
    lib = runtime.load_library()
    for name in ("pk_load_batch_model", "pk_set_batch", "pk_eval_cycle_batch_dev"):
        assert getattr(lib, name) is not None
    assert lib.pk_set_batch(None, 4) == 1 and lib.pk_load_batch_model(None, None, 0) == 1      # (null context: error 1, no crash)
