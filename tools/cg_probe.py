"""Host-landed time of ``Linearization.solve_condensed`` (the CG loop on the device, csrc/pk_cg.cpp) against
``scipy.sparse.linalg.cg`` over ``LinearOperator``s composed from the SAME handle's ``jv`` / ``jtv`` / ``hv`` -- what a user writes
without it -- with the same tol, the same Jacobi vector and the same iteration count; and the event-timed cost of one device
iteration, split into the products and the vector steps.  Needs an MI355X; prints a table.

    python tools/cg_probe.py [--runs 5] [--out profiles/cg_probe_mi355x.txt]
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
TOL, MAXITER = 1e-8, 64


def spread(samples):
    return f"{statistics.median(samples):9.1f} [{min(samples):.1f}, {max(samples):.1f}]"


def inputs(lin, form):
    inv = lambda a: np.where(a > 0, 1.0 / np.where(a > 0, a, 1.0), 0.0)  # noqa: E731
    rng = np.random.default_rng(11)
    if form == "primal":
        rho = max(1.0, float(lin.row_norms("H", "1").max()))
        return inv(lin.row_norms("J", "2sq")), 2.0 * rho, rng.standard_normal(lin.n)
    return inv(lin.row_norms("JT", "2sq")), 0.5, rng.standard_normal(lin.m)


def scipy_solve(lin, form, d, shift, b, minv, maxiter):
    """(x, iterations, products): SciPy's CG over the handle's products, one host round trip each."""
    from scipy.sparse.linalg import LinearOperator, cg

    count = [0, 0]
    if form == "primal":
        def mv(v):
            count[1] += 3
            v = np.asarray(v).reshape(-1)
            return lin.hv(v) + lin.jtv(d * lin.jv(v)) + shift * v
    else:
        def mv(v):
            count[1] += 2
            v = np.asarray(v).reshape(-1)
            return lin.jv(d * lin.jtv(v)) + shift * v
    size = len(b)
    K = LinearOperator((size, size), matvec=mv, dtype=np.float64)
    M = LinearOperator((size, size), matvec=lambda v: minv * np.asarray(v).reshape(-1), dtype=np.float64)

    def cb(_):
        count[0] += 1

    x, _ = cg(K, b, rtol=TOL, atol=0.0, maxiter=maxiter, M=M, callback=cb)
    return x, count[0], count[1]


def device_iteration(ev, point, form, d, shift, b, minv, lines):
    """Event-timed microseconds of one iteration on torch's stream: whole, products alone, vector steps alone."""
    import torch

    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    x, lam, sigma = point      # (the probe evaluates the CSR values into tensors of its own, on torch's stream)
    size = len(b)
    cj = torch.zeros(ev.csr_map("jac").nnz, dtype=torch.float64, device=dev)
    ch = torch.zeros(ev.csr_map("hess").nnz, dtype=torch.float64, device=dev)
    dx, dlam = up(x), up(lam)
    ts = torch.cuda.Stream()      # (a stream of torch's own: its events then bracket what the library enqueues on it)
    st = ts.cuda_stream
    torch.cuda.synchronize()
    ev.jacobian_csr_dev(dx.data_ptr(), cj.data_ptr(), stream=st)
    ev.hessian_csr_dev(dx.data_ptr(), dlam.data_ptr(), sigma, ch.data_ptr(), stream=st)
    dd, ds, dm, db = up(d), up(np.full(size, shift)), up(minv), up(b)
    sol, v, y = torch.zeros(size, dtype=torch.float64, device=dev), up(b), torch.zeros(size, dtype=torch.float64, device=dev)
    hv = ch.data_ptr() if form == "primal" else None
    torch.cuda.synchronize()
    K = 16
    whole, prod, vec = [], [], []
    work = [torch.zeros(size, dtype=torch.float64, device=dev) for _ in range(5)]
    rec = torch.zeros(8, dtype=torch.float64, device=dev)
    lib, h = ev.ctx.lib, ev.ctx.handle
    for rep in range(12):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev.cg_begin_dev(form, cj.data_ptr(), db.data_ptr(), sol.data_ptr(), 0.0, d_hvals=hv, d_d=dd.data_ptr(), d_s=ds.data_ptr(),
                        d_minv=dm.data_ptr(), stream=st)
        e[0].record(ts)
        ev.cg_advance_dev(K, stream=st)
        e[1].record(ts)
        e[2].record(ts)
        for _ in range(K):
            ev.condensed_apply_dev(form, cj.data_ptr(), v.data_ptr(), y.data_ptr(), d_hvals=hv, d_d=dd.data_ptr(), d_s=ds.data_ptr(), stream=st)
        e[3].record(ts)
        xx, r, z, p, q = (w.data_ptr() for w in work)
        ev.ctx.check(lib.pk_cg_step_dev(h, 0, size, db.data_ptr(), None, dm.data_ptr(), ds.data_ptr(), xx, r, z, p, q, rec.data_ptr(), 0.0, st))
        e[4].record(ts)
        for _ in range(K):
            for step in (1, 2, 3):
                ev.ctx.check(lib.pk_cg_step_dev(h, step, size, None, None, dm.data_ptr(), ds.data_ptr(), xx, r, z, p, q, rec.data_ptr(), 0.0, st))
        e[5].record(ts)
        torch.cuda.synchronize()
        if rep >= 2:      # (two warm-up rounds)
            whole.append(1e3 * e[0].elapsed_time(e[1]) / K)
            prod.append(1e3 * e[2].elapsed_time(e[3]) / K)
            vec.append(1e3 * e[4].elapsed_time(e[5]) / K)
    status = (ev.cg_record()[0], float(rec.cpu()[0]))      # (both must still be 0: a frozen iteration skips its update)
    lines.append(f"    device iteration, event-timed over {K} back-to-back iterations (us): whole {spread(whole)}   products (with q = s o v) "
                 f"{spread(prod)}   vector steps (p.q, update, direction, two scalar steps) {spread(vec)}   [status {status[0]:.0f} / {status[1]:.0f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import models

    lines = [f"cg_probe: tol {TOL}, Jacobi preconditioner, b standard normal (seed 11); median [min, max] of {args.runs} alternating runs; "
             "host-landed microseconds (perf_counter around calls that end in a synchronisation)"]
    slower = []
    for name, scheme, mesh, num_point in MODELS:
        system, _, guess = getattr(models, name)(importlib.import_module(f"pockit_amd.{scheme}"), mesh, num_point)
        x, lam, sigma = models.bench_inputs(system, guess)
        ev = system.evaluator
        for form in ("primal", "dual"):
            lin = system.linearize(x, lam, sigma)
            d, shift, b = inputs(lin, form)
            minv = lin.jacobi(d, shift, form=form)
            xd, info = lin.solve_condensed(b, d, shift, form=form, tol=TOL, maxiter=MAXITER)           # warm-up, and the count
            k = info.iterations
            xs, ks, products = scipy_solve(lin, form, d, shift, b, minv, k)
            n, m = lin.n, lin.m
            size, other = (n, m) if form == "primal" else (m, n)
            chunks = -(-k // 8) + 1
            dev_bytes = 8 * (2 * size + other) + 8 * size + 64 * chunks                       # b, s and d up; x down; the records
            per_product = 8 * ((n + m) * 2 + (2 * n if form == "primal" else 0))              # every product: a vector up, a vector down
            sci_bytes = per_product * (products // (3 if form == "primal" else 2))
            t_dev, t_sci = [], []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                lin.solve_condensed(b, d, shift, form=form, tol=TOL, maxiter=MAXITER)
                t1 = time.perf_counter()
                scipy_solve(lin, form, d, shift, b, minv, k)
                t2 = time.perf_counter()
                t_dev.append(1e6 * (t1 - t0))
                t_sci.append(1e6 * (t2 - t1))
            below = max(t_dev) < min(t_sci)
            slower.append(below)
            lines.append(f"{name}({scheme}, {mesh}, {num_point}) {form}: n {n}, m {m}; device {k} iterations ({info.status}), SciPy {ks} "
                         f"iterations, {products} products; max|x_dev - x_scipy| {np.max(np.abs(xd - xs)):.2e}")
            lines.append(f"    solve_condensed  {spread(t_dev)} us per solve, {statistics.median(t_dev) / max(k, 1):8.1f} us per iteration, "
                         f"{dev_bytes} bytes over PCIe")
            lines.append(f"    scipy cg         {spread(t_sci)} us per solve, {statistics.median(t_sci) / max(ks, 1):8.1f} us per iteration, "
                         f"{sci_bytes} bytes over PCIe")
            lines.append(f"    the slowest device run lies {'BELOW' if below else 'NOT below'} the fastest SciPy run "
                         f"(ratio of medians {statistics.median(t_sci) / statistics.median(t_dev):.1f}x)")
            device_iteration(ev, (x, lam, sigma), form, d, shift, b, minv, lines)
        ev.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
