"""Host-landed time of one round ``barrier_terms`` + ``dual_residual`` + ``boundary_step`` (csrc/pk_ipm.cpp) against the same
quantities in NumPy on host arrays with J^T lam through the SAME handle's ``jtv`` -- what a user writes without the unit -- and
the bytes each moves over PCIe.  Needs an MI355X; prints a table.

    python tools/ipm_probe.py [--runs 5] [--out profiles/ipm_probe_mi355x.txt]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODELS = [("planar_quadrotor", "radau", 2000, 6), ("brachistochrone", "radau", 200, 8)]
MU, TAU = 0.1, 0.995


def spread(samples):
    return f"{statistics.median(samples):9.1f} [{min(samples):.1f}, {max(samples):.1f}]"


def device_round(ev, lin, q):
    terms = ev.barrier_terms(q["v"], q["zl"], q["zu"], MU)
    r, res = lin.dual_residual(q["grad"], q["lam"], z=terms.rbar, negate=True)
    step = ev.boundary_step(q["v"], q["dv"], q["zl"], q["zu"], MU, TAU)
    return terms, r, res, step


class Resident:
    """The round on vectors that already lie on the device (torch tensors): six launches and J^T lam enqueued, one wait, the
    three records (16 doubles) down."""

    def __init__(self, ev, lin, q, point):
        import torch

        self.torch, self.ev = torch, ev
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
        n = lin.n
        self.d = {k: up(q[k]) for k in ("v", "dv", "zl", "zu", "grad", "lam")}
        self.cj = torch.zeros(ev.csr_map("jac").nnz, dtype=torch.float64, device=dev)
        self.out = {k: torch.zeros(n, dtype=torch.float64, device=dev) for k in ("sigma", "rbar", "r", "dzl", "dzu")}
        self.rec = torch.zeros(16, dtype=torch.float64, device=dev)
        self.sol = up(np.concatenate((q["dv"], q["lam"])))
        dx = up(point)
        torch.cuda.synchronize()
        ev.jacobian_csr_dev(dx.data_ptr(), self.cj.data_ptr())
        ev.sync()

    def round(self):
        ev, d, o, p = self.ev, self.d, self.out, self.rec.data_ptr()
        ev.ip_terms_dev(d["v"].data_ptr(), d["zl"].data_ptr(), d["zu"].data_ptr(), MU, o["sigma"].data_ptr(), o["rbar"].data_ptr(), p)
        ev.dual_residual_dev(self.cj.data_ptr(), d["grad"].data_ptr(), d["lam"].data_ptr(), o["r"].data_ptr(), p + 64, d_z=o["rbar"].data_ptr(),
                             negate=True)
        ev.ip_step_dev(d["v"].data_ptr(), d["dv"].data_ptr(), d["zl"].data_ptr(), d["zu"].data_ptr(), MU, TAU, o["dzl"].data_ptr(),
                       o["dzu"].data_ptr(), p + 96)
        ev.sync()
        return self.rec.cpu().numpy()

    def host_side_round(self, lin, q):
        """What a caller does without the unit when the step lies on the device: the step (n + m doubles) down, the NumPy
        round, sigma and b1 (2 n doubles) up again for the next solve."""
        torch = self.torch
        sol = self.sol.cpu().numpy()
        res = numpy_round(lin, dict(q, dv=sol[: lin.n]))
        self.out["sigma"].copy_(torch.from_numpy(res[0]))
        self.out["r"].copy_(torch.from_numpy(res[3]))
        torch.cuda.synchronize()
        return res


def numpy_round(lin, q):
    """The same quantities by elementwise passes and reductions over host arrays; one product through PCIe."""
    lb, ub, v, dv, zl, zu = (q[k] for k in ("lb", "ub", "v", "dv", "zl", "zu"))
    with np.errstate(all="ignore"):
        boxed = lb != ub
        lo, up = boxed & np.isfinite(lb), boxed & np.isfinite(ub)
        dl, du = np.where(lo, v - lb, 1.0), np.where(up, ub - v, 1.0)
        sl, su = np.where(lo, zl, 0.0), np.where(up, zu, 0.0)
        sigma = np.where(lo, sl / dl, 0.0) + np.where(up, su / du, 0.0)
        rbar = np.where(lo, MU / dl, 0.0) - np.where(up, MU / du, 0.0)
        cl, cu = dl * sl, du * su
        rec = (max(np.max(np.abs(cl - MU), where=lo, initial=0.0), np.max(np.abs(cu - MU), where=up, initial=0.0)),
               np.sum(cl, where=lo) + np.sum(cu, where=up), lo.sum() + up.sum(),
               min(np.min(dl, where=lo, initial=np.inf), np.min(du, where=up, initial=np.inf)),
               np.sum(np.log(dl), where=lo) + np.sum(np.log(du), where=up),
               np.sum(lo & ~((dl > 0) & (sl >= 0))) + np.sum(up & ~((du > 0) & (su >= 0))), np.sum(sl) + np.sum(su),
               min(np.min(cl, where=lo, initial=np.inf), np.min(cu, where=up, initial=np.inf)))
        r = np.where(boxed, -(lin.jtv(q["lam"]) + q["grad"] - rbar), 0.0)
        res = (np.max(np.abs(r)), r @ r)
        dzl = np.where(lo, (MU / dl - sl) - (sl / dl) * dv, 0.0)
        dzu = np.where(up, (MU / du - su) + (su / du) * dv, 0.0)
        cand = np.concatenate(((TAU * dl)[lo & (dv < 0)] / -dv[lo & (dv < 0)], (TAU * du)[up & (dv > 0)] / dv[up & (dv > 0)]))
        cand_z = np.concatenate(((TAU * sl)[lo & (dzl < 0)] / -dzl[lo & (dzl < 0)], (TAU * su)[up & (dzu < 0)] / -dzu[up & (dzu < 0)]))
        alpha = (min(1.0, cand.min(initial=1.0)), min(1.0, cand_z.min(initial=1.0)))
    return sigma, rbar, rec, r, res, dzl, dzu, alpha


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import models
    from ipm_cases import inside      # (tests/: x moved strictly inside the plan's bounds, as the GPU tests do it)

    lines = [f"ipm_probe: one round barrier_terms + dual_residual (z = rbar, negated) + boundary_step on the variables, mu {MU}, tau {TAU}; "
             f"median [min, max] of {args.runs} alternating runs; host-landed microseconds (perf_counter around calls that end in a synchronisation)"]
    for name, scheme, mesh, num_point in MODELS:
        system, _, guess = getattr(models, name)(importlib.import_module(f"pockit_amd.{scheme}"), mesh, num_point)
        x, lam, sigma = models.bench_inputs(system, guess)
        ev = system.evaluator
        p = ev.plan
        lin = system.linearize(x, lam, sigma)
        n, m = lin.n, lin.m
        rng = np.random.default_rng(11)
        lb, ub = np.asarray(p.v_lb, dtype=np.float64), np.asarray(p.v_ub, dtype=np.float64)
        q = dict(lb=lb, ub=ub, v=inside(lb, ub, x), zl=rng.uniform(0.1, 1.0, n), zu=rng.uniform(0.1, 1.0, n), dv=rng.standard_normal(n),
                 grad=rng.standard_normal(n), lam=rng.standard_normal(m))
        terms, r, res, step = device_round(ev, lin, q)          # warm-up, and the comparison
        ref = numpy_round(lin, q)
        worst = max(np.max(np.abs(terms.sigma - ref[0])), np.max(np.abs(terms.rbar - ref[1])), np.max(np.abs(r - ref[3])),
                    np.max(np.abs(step.dzl - ref[5])), np.max(np.abs(step.dzu - ref[6])), abs(step.alpha_primal - ref[7][0]),
                    abs(step.alpha_dual - ref[7][1]))
        dev_bytes = 8 * (3 * n + 2 * n + 8) + 8 * (2 * n + m + n + 4) + 8 * (4 * n + 2 * n + 4)
        np_bytes = 8 * (m + n)                                   # jtv: lam up, J^T lam down; everything else is on the host already
        t_dev, t_np, t_res, t_side = [], [], [], []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            device_round(ev, lin, q)
            t1 = time.perf_counter()
            numpy_round(lin, q)
            t2 = time.perf_counter()
            t_dev.append(1e6 * (t1 - t0))
            t_np.append(1e6 * (t2 - t1))
        resident = Resident(ev, lin, q, x)                       # (its own CSR values: the handle is stale from here on)
        lin = system.linearize(x, lam, sigma)
        rec = resident.round()
        resident.host_side_round(lin, q)
        same = np.array_equal(rec, np.concatenate((terms.table, res.table, step.table)))      # (all sixteen slots)
        for _ in range(args.runs):
            t0 = time.perf_counter()
            resident.round()
            t1 = time.perf_counter()
            resident.host_side_round(lin, q)
            t2 = time.perf_counter()
            t_res.append(1e6 * (t1 - t0))
            t_side.append(1e6 * (t2 - t1))
        lines.append(f"{name}({scheme}, {mesh}, {num_point}): n {n}, m {m}; sides {terms.sides:.0f}, bad {terms.bad:.0f}, alpha_primal "
                     f"{step.alpha_primal:.3e}, alpha_dual {step.alpha_dual:.3e}; max |device - NumPy| over the vectors and step lengths {worst:.2e}")
        lines.append(f"    host forms (6 launches + J^T lam) {spread(t_dev)} us per round, {dev_bytes} bytes over PCIe")
        lines.append(f"    NumPy on host arrays + jtv         {spread(t_np)} us per round, {np_bytes} bytes over PCIe")
        lines.append(f"    ratio of medians NumPy / host forms {statistics.median(t_np) / statistics.median(t_dev):.2f}x "
                     f"(the host forms move every vector both ways)")
        lines.append(f"    _dev forms on resident vectors      {spread(t_res)} us per round, 128 bytes over PCIe (the three records); records "
                     f"{'equal' if same else 'DIFFER from'} the host forms'")
        lines.append(f"    step down, NumPy, sigma and b1 up   {spread(t_side)} us per round, {8 * (n + m) + 8 * (m + n) + 8 * 2 * n} bytes over PCIe")
        lines.append(f"    ratio of medians {statistics.median(t_side) / statistics.median(t_res):.2f}x; the slowest resident round lies "
                     f"{'BELOW' if max(t_res) < min(t_side) else 'NOT below'} the fastest host-side round")
        ev.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
