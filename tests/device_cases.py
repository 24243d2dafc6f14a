"""What the GPU tests of the solvers on the device (tests/test_gpu_cg.py, tests/test_gpu_minres.py) share: device buffers between
sentinels, uploads through torch, bit comparison with an emulator, the evaluator the vector steps run on, and the context of a
synthetic system.  A plain helper module: imported by name, no fixtures of its own beyond ``step_ev``."""
import importlib

import numpy as np
import pytest

import cg_cases as cg
import models
import sparse_cases as sc

PAD, SENTINEL = 8, -7.25e77


def _i32(a):
    from pockit_amd import runtime

    return np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(runtime.c_int32_p)


class Buf:
    """``count`` doubles in the middle of a larger device tensor, between sentinels: NaN, or ``content``."""

    def __init__(self, count, content=None):
        import torch

        host = np.full(count + 2 * PAD, np.nan)
        host[:PAD] = host[PAD + count:] = SENTINEL
        if content is not None:
            host[PAD: PAD + count] = content
        self.count, self.t = count, torch.from_numpy(host).to(torch.device("cuda", 0))
        self.ptr = self.t.data_ptr() + 8 * PAD

    def fetch(self):
        host = self.t.cpu().numpy()
        edge = np.full(PAD, SENTINEL)
        assert sc.same_bits(host[:PAD], edge) and sc.same_bits(host[PAD + self.count:], edge), "a sentinel was overwritten"
        return host[PAD: PAD + self.count].copy()


def _up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.device("cuda", 0))


def _ptr(t):
    return None if t is None else t.ptr if isinstance(t, Buf) else t.data_ptr()


def _sync():
    import torch

    torch.cuda.synchronize()            # torch's copies run on its own stream; the context uses its own


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    differ = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert len(differ) == 0, f"{what}: {len(differ)} entries differ in bits from the emulator, first {differ[:6]}: {got[differ[:6]]} for {want[differ[:6]]}"


@pytest.fixture(scope="module")
def step_ev():
    import pockit_amd.radau as radau

    ev = models.brachistochrone(radau, 3, 4)[0].evaluator
    yield ev
    ev.close()


class SyntheticContext:
    """The evaluator ``ev`` of a context of sparse_cases.CONTEXTS with the structures of cg_cases.System as its operators and the
    model's own values linearized: ``random`` is the system of full-mantissa values, ``real`` the same structures over the
    values pk_linearize leaves (what the host forms read)."""

    def __init__(self, ctx):
        from pockit_amd import runtime

        name, scheme, mesh, num_point = sc.CONTEXTS[ctx]["model"]
        system, _, guess = getattr(models, name)(importlib.import_module(f"pockit_amd.{scheme}"), mesh, num_point)
        self.ev = ev = system.evaluator
        x, lam, sigma = models.bench_inputs(system, guess)
        c = sc.CONTEXTS[ctx]
        assert (ev.csr_map("jac").nnz, ev.csr_map("hess").nnz) == (c["nnz_j"], c["nnz_h"])
        vals_j, vals_h = ev.jacobian_csr(x), ev.hessian_csr(x, lam, sigma)
        self.random = sy = cg.system(ctx)
        self.real = cg.System(ctx, cg.SEEDS[ctx], values=(vals_j, vals_h))
        lib, h = ev.ctx.lib, ev.ctx.handle
        for op, st in ((0, sy.J), (1, sy.JT), (2, sy.H)):
            ev.ctx.check(lib.pk_set_csr_operator(h, op, _i32(st.indptr), _i32(st.indices), _i32(st.src), st.n_rows, st.n_cols, st.nnz))
        ev.ctx.check(lib.pk_set_operator_diagonal(h, 2, _i32(sy.diag_pos), sy.n))
        ev.ctx.check(lib.pk_linearize(h, runtime.as_dp(np.ascontiguousarray(x)), runtime.as_dp(np.ascontiguousarray(lam)), float(sigma)))
