"""Host-landed time of ``Linearization.solve_kkt`` (the MINRES loop on the device, csrc/pk_minres.cpp) against
``scipy.sparse.linalg.minres`` over a ``LinearOperator`` composed from the SAME handle's ``jv`` / ``jtv`` / ``hv`` -- what a user
writes without it -- with the same diagonal preconditioner and SciPy stopped by ``maxiter`` at the device's iteration count; and the
event-timed cost of one device iteration, split into the products and the vector steps.  Needs an MI355X; prints a table
(DESIGN.md section 19).

    python tools/minres_probe.py [--runs 5] [--out profiles/minres_probe_mi355x.txt]
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
TOL, MAXITER = 1e-8, 400


def spread(samples):
    return f"{statistics.median(samples):9.1f} [{min(samples):.1f}, {max(samples):.1f}]"


def inputs(lin):
    """s1 = 2 rho, s2 = 0.5, b standard normal: the quasi-definite system of tests/test_gpu_minres.py"""
    rho = max(1.0, float(lin.row_norms("H", "1").max()))
    return 2.0 * rho, 0.5, np.random.default_rng(11).standard_normal(lin.n + lin.m)


def scipy_solve(lin, s1, s2, b, minv, maxiter):
    """(x, iterations, applications): SciPy's MINRES over the handle's products, one host round trip each."""
    from scipy.sparse.linalg import LinearOperator, minres

    n = lin.n
    count = [0, 0]

    def mv(v):
        count[1] += 1
        v = np.asarray(v).reshape(-1)
        v1, v2 = v[:n], v[n:]
        return np.concatenate((lin.hv(v1) + lin.jtv(v2) + s1 * v1, lin.jv(v1) - s2 * v2))

    size = len(b)
    K = LinearOperator((size, size), matvec=mv, dtype=np.float64)
    M = LinearOperator((size, size), matvec=lambda v: minv * np.asarray(v).reshape(-1), dtype=np.float64)

    def cb(_):
        count[0] += 1

    x, _ = minres(K, b, rtol=0.0, maxiter=maxiter, M=M, callback=cb)      # (its own stopping rule is another one: maxiter alone stops it)
    return x, count[0], count[1]


def device_iteration(ev, point, s1, s2, b, minv, n, lines):
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
    d1, d2, dm, db = up(np.full(n, s1)), up(np.full(size - n, s2)), up(minv), up(b)
    sol, v, y = torch.zeros(size, dtype=torch.float64, device=dev), up(b), torch.zeros(size, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    K = 16
    whole, prod, vec = [], [], []
    work = [torch.zeros(size, dtype=torch.float64, device=dev) for _ in range(8)]
    rec = torch.zeros(16, dtype=torch.float64, device=dev)
    lib, h = ev.ctx.lib, ev.ctx.handle
    for rep in range(12):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev.minres_begin_dev(cj.data_ptr(), db.data_ptr(), sol.data_ptr(), 0.0, d_hvals=ch.data_ptr(), d_s1=d1.data_ptr(), d_s2=d2.data_ptr(),
                            d_minv=dm.data_ptr(), stream=st)
        e[0].record(ts)
        ev.minres_advance_dev(K, stream=st)
        e[1].record(ts)
        e[2].record(ts)
        for _ in range(K):
            ev.kkt_apply_dev(cj.data_ptr(), v.data_ptr(), y.data_ptr(), d_hvals=ch.data_ptr(), d_s1=d1.data_ptr(), d_s2=d2.data_ptr(), stream=st)
        e[3].record(ts)
        p = [w.data_ptr() for w in work]      # x, r1, r2, y, v, w, w2, q
        step = lambda which: ev.ctx.check(lib.pk_minres_step_dev(  # noqa: E731
            h, which, size, n, db.data_ptr(), None, dm.data_ptr(), d1.data_ptr(), d2.data_ptr(), *p, rec.data_ptr(), 0.0, st))
        step(0)
        e[4].record(ts)
        for _ in range(K):
            for which in (1, 2, 3, 4):
                step(which)
        e[5].record(ts)
        torch.cuda.synchronize()
        if rep >= 2:      # (two warm-up rounds)
            whole.append(1e3 * e[0].elapsed_time(e[1]) / K)
            prod.append(1e3 * e[2].elapsed_time(e[3]) / K)
            vec.append(1e3 * e[4].elapsed_time(e[5]) / K)
    status = (ev.minres_record()[0], float(rec.cpu()[0]))      # (the first must still be 0: a frozen iteration skips its update)
    lines.append(f"    device iteration, event-timed over {K} back-to-back iterations (us): whole {spread(whole)}   products (with the diagonal "
                 f"blocks' launch) {spread(prod)}   vector steps (Lanczos vector, v.q, update, solution update, two scalar steps) {spread(vec)}   "
                 f"[status {status[0]:.0f} / {status[1]:.0f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import models

    lines = [f"minres_probe: K = [[H + 2 rho I, J^T], [J, -0.5 I]], tol {TOL}, diagonal preconditioner, b standard normal (seed 11); median "
             f"[min, max] of {args.runs} alternating runs; host-landed microseconds (perf_counter around calls that end in a synchronisation)"]
    for name, scheme, mesh, num_point in MODELS:
        system, _, guess = getattr(models, name)(importlib.import_module(f"pockit_amd.{scheme}"), mesh, num_point)
        x, lam, sigma = models.bench_inputs(system, guess)
        ev = system.evaluator
        lin = system.linearize(x, lam, sigma)
        s1, s2, b = inputs(lin)
        minv = lin.kkt_precond(s1, s2)
        xd, info = lin.solve_kkt(b, s1, s2, tol=TOL, maxiter=MAXITER)           # warm-up, and the count
        k = info.iterations
        xs, ks, applications = scipy_solve(lin, s1, s2, b, minv, k)
        n, m = lin.n, lin.m
        size = n + m
        chunks = -(-k // 8) + 1
        dev_bytes = 8 * (2 * size) + 8 * size + 128 * chunks                   # b, s1 and s2 up; x down; the records
        sci_bytes = applications * 8 * (2 * (n + n) + 2 * (n + m))             # hv, jtv and jv: a vector up, a vector down each
        t_dev, t_sci = [], []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            lin.solve_kkt(b, s1, s2, tol=TOL, maxiter=MAXITER)
            t1 = time.perf_counter()
            scipy_solve(lin, s1, s2, b, minv, k)
            t2 = time.perf_counter()
            t_dev.append(1e6 * (t1 - t0))
            t_sci.append(1e6 * (t2 - t1))
        below = max(t_dev) < min(t_sci)
        lines.append(f"{name}({scheme}, {mesh}, {num_point}): n {n}, m {m}; device {k} iterations ({info.status}, rel_residual "
                     f"{info.rel_residual:.2e}), SciPy {ks} iterations, {applications} applications of K (3 products each); "
                     f"max|x_dev - x_scipy| {np.max(np.abs(xd - xs)):.2e}")
        lines.append(f"    solve_kkt        {spread(t_dev)} us per solve, {statistics.median(t_dev) / max(k, 1):8.1f} us per iteration, "
                     f"{dev_bytes} bytes over PCIe")
        lines.append(f"    scipy minres     {spread(t_sci)} us per solve, {statistics.median(t_sci) / max(ks, 1):8.1f} us per iteration, "
                     f"{sci_bytes} bytes over PCIe")
        lines.append(f"    the slowest device run lies {'BELOW' if below else 'NOT below'} the fastest SciPy run "
                     f"(ratio of medians {statistics.median(t_sci) / statistics.median(t_dev):.1f}x)")
        device_iteration(ev, (x, lam, sigma), s1, s2, b, minv, n, lines)
        ev.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
