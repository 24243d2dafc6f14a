"""What a product with J, J^T or the symmetric H costs on the device (pk_op_rows / pk_op_long), next to what a caller pays
today to get the matrix itself.

    python tools/operator_probe.py [--runs 5] [--inner 200] [--out FILE]
    python tools/operator_probe.py --block [--runs 5] [--inner 50] [--out FILE]

Per model -- c2 = brachistochrone(radau, 200, 8), c3 = planar_quadrotor(radau, 2000, 6) -- microseconds as [median, min, max]
of ``--runs`` ALTERNATING runs (every figure once per run, run after run):

* J v, J^T y, H v: ``inner`` back-to-back ``apply_operator_dev`` on one stream between two HIP events, per product;
* pk_csr J / H: the gather of the triplets into the CSR values (``gather_csr_dev``), timed the same way;
* jacobian_csr / hessian_csr: wall time of the host-landed calls of the same tree (evaluate, gather, bring the values down):
  what a caller pays per iterate to hold the matrix on the host.

bytes = what a product moves at least: 12 per entry (value, column), 4 more with src, 8 per row and per column.

``--block``: the block product (pk_op_rows_k / pk_op_long_k) instead.  Per model and operator, for k = 1, 2, 4, 8, 16: event-timed
microseconds PER COLUMN of one ``apply_operator_block_dev`` with k columns, next to k ``apply_operator_dev`` calls of the same
tree on the columns' own vectors, and the wall time per column of the host-landed ``jmat`` next to k calls of ``jv``; the same
[median, min, max] of alternating runs.  bytes = 12 per entry (+ 4 with src) + 8 k per row and per column for the block, k
times the single product's bytes for the k single products."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--host-inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--block", action="store_true", help="the block product against k single products")
    a = ap.parse_args()
    if a.block:
        return block_main(a)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from pockit_amd import benchmarks as models
    import pockit_amd.radau as radau

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    stat = lambda v: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)]  # noqa: E731
    results, lines = [], []
    for tag, build in (("c2 brachistochrone(radau, 200, 8)", lambda: models.brachistochrone(radau, 200, 8)),
                       ("c3 planar_quadrotor(radau, 2000, 6)", lambda: models.planar_quadrotor(radau, 2000, 6))):
        system, _, guess = build()
        ev, p = system.evaluator, system.plan
        x, lam, sigma = models.bench_inputs(system, guess)
        mj, mh = ev.csr_map("jac"), ev.csr_map("hess")
        up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)  # noqa: E731
        zeros = lambda n: torch.zeros(max(n, 1), dtype=torch.float64, device=dev)  # noqa: E731
        dx, dlam = up(x), up(lam)
        cj, ch, tj, th = zeros(mj.nnz), zeros(mh.nnz), zeros(p.nnz_J), zeros(p.nnz_H)
        rng = np.random.default_rng(0)
        vn, vm, yn, ym = up(rng.standard_normal(p.n)), up(rng.standard_normal(p.m)), zeros(p.n), zeros(p.m)
        torch.cuda.synchronize()
        ev.jacobian_csr_dev(dx.data_ptr(), cj.data_ptr(), st)
        ev.hessian_csr_dev(dx.data_ptr(), dlam.data_ptr(), sigma, ch.data_ptr(), st)
        stream.synchronize()
        device_items = {
            "J v": lambda: ev.apply_operator_dev("J", cj.data_ptr(), vn.data_ptr(), ym.data_ptr(), stream=st),
            "J^T y": lambda: ev.apply_operator_dev("JT", cj.data_ptr(), vm.data_ptr(), yn.data_ptr(), stream=st),
            "H v": lambda: ev.apply_operator_dev("H", ch.data_ptr(), vn.data_ptr(), yn.data_ptr(), stream=st),
            "pk_csr J": lambda: ev.gather_csr_dev("jac", tj.data_ptr(), cj.data_ptr(), st),
            "pk_csr H": lambda: ev.gather_csr_dev("hess", th.data_ptr(), ch.data_ptr(), st),
        }
        host_items = {"jacobian_csr (host-landed)": lambda: system.jacobian_csr(x),
                      "hessian_csr (host-landed)": lambda: system.hessian_csr(x, lam, sigma)}
        for fn in list(device_items.values()) + list(host_items.values()):      # operators uploaded, caches warm
            fn()
        stream.synchronize()
        us = {name: [] for name in list(device_items) + list(host_items)}
        for _ in range(a.runs):
            for name, fn in device_items.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fn()
                e0.record(stream)
                for _ in range(a.inner):
                    fn()
                e1.record(stream)
                stream.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / a.inner)
            for name, fn in host_items.items():
                fn()
                t0 = time.perf_counter()
                for _ in range(a.host_inner):
                    fn()
                us[name].append((time.perf_counter() - t0) * 1e6 / a.host_inner)
        ops = {"J v": ev._ops["J"], "J^T y": ev._ops["JT"], "H v": ev._ops["H"]}
        nbytes = {k: 12 * o.nnz + (4 * o.nnz if o.src is not None else 0) + 8 * sum(o.shape) for k, o in ops.items()}
        rows = {name: {"us": stat(v), "bytes": nbytes.get(name)} for name, v in us.items()}
        results.append({"model": tag, "n": p.n, "m": p.m, "nnz_J_csr": mj.nnz, "nnz_H_csr": mh.nnz,
                        "nnz_H_symmetric": ops["H v"].nnz, "rows": rows})
        lines.append(f"# {tag}: n {p.n}, m {p.m}, J {mj.nnz} entries, H {mh.nnz} (lower) / {ops['H v'].nnz} (symmetric)")
        lines.append(f"# {'':<28} {'us [median, min, max]':>28} {'MB moved':>10} {'GB/s':>8}")
        for name, r in rows.items():
            mb = "" if r["bytes"] is None else f"{r['bytes'] / 1e6:.2f}"
            rate = "" if r["bytes"] is None else f"{r['bytes'] / r['us'][0] / 1e3:.0f}"
            lines.append(f"  {name:<28} {str(r['us']):>28} {mb:>10} {rate:>8}")
        ev.close()
    res = {"runs": a.runs, "inner": a.inner, "host_inner": a.host_inner, "figures": "[median, min, max] in us", "models": results}
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n" + json.dumps(res) + "\n")


BLOCK_KS = (1, 2, 4, 8, 16)


def block_main(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from pockit_amd import benchmarks as models
    import pockit_amd.radau as radau

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    stat = lambda v: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)]  # noqa: E731
    results, lines = [], []
    for tag, build in (("c2 brachistochrone(radau, 200, 8)", lambda: models.brachistochrone(radau, 200, 8)),
                       ("c3 planar_quadrotor(radau, 2000, 6)", lambda: models.planar_quadrotor(radau, 2000, 6))):
        system, _, guess = build()
        ev, p = system.evaluator, system.plan
        x, lam, sigma = models.bench_inputs(system, guess)
        mj, mh = ev.csr_map("jac"), ev.csr_map("hess")
        up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)  # noqa: E731
        dx, dlam = up(x), up(lam)
        cj = torch.zeros(mj.nnz, dtype=torch.float64, device=dev)
        ch = torch.zeros(mh.nnz, dtype=torch.float64, device=dev)
        rng = np.random.default_rng(0)
        kmax = max(BLOCK_KS)
        hVn, hVm = rng.standard_normal((p.n, kmax)), rng.standard_normal((p.m, kmax))
        torch.cuda.synchronize()
        ev.jacobian_csr_dev(dx.data_ptr(), cj.data_ptr(), st)
        ev.hessian_csr_dev(dx.data_ptr(), dlam.data_ptr(), sigma, ch.data_ptr(), st)
        stream.synchronize()
        shapes = {"J": (cj, hVn, p.m), "JT": (cj, hVm, p.n), "H": (ch, hVn, p.n)}
        items = {}      # name -> (callable, columns per call)
        for op, (vals, hV, rows) in shapes.items():
            for k in BLOCK_KS:
                V = up(hV[:, :k])
                Y = torch.zeros((rows, k), dtype=torch.float64, device=dev)
                cols = [up(hV[:, j]) for j in range(k)]
                ys = [torch.zeros(rows, dtype=torch.float64, device=dev) for _ in range(k)]

                def block(op=op, vals=vals, k=k, V=V, Y=Y):
                    ev.apply_operator_block_dev(op, vals.data_ptr(), k, V.data_ptr(), Y.data_ptr(), stream=st)

                def singles(op=op, vals=vals, cols=cols, ys=ys):
                    for v, y in zip(cols, ys):
                        ev.apply_operator_dev(op, vals.data_ptr(), v.data_ptr(), y.data_ptr(), stream=st)

                items[f"{op} block k={k}"] = (block, k)
                items[f"{op} {k} singles"] = (singles, k)
        lin = system.linearize(x, lam, sigma)
        host_items = {}
        for k in BLOCK_KS:
            Vk = np.ascontiguousarray(hVn[:, :k])
            host_items[f"jmat k={k} (host-landed)"] = (lambda Vk=Vk: lin.jmat(Vk), k)
            host_items[f"{k} x jv (host-landed)"] = (lambda Vk=Vk: [lin.jv(Vk[:, j]) for j in range(Vk.shape[1])], k)
        torch.cuda.synchronize()
        for fn, _ in items.values():      # operators uploaded, partial sums allocated
            fn()
        stream.synchronize()
        us = {name: [] for name in list(items) + list(host_items)}
        for _ in range(a.runs):
            for name, (fn, k) in items.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fn()
                e0.record(stream)
                for _ in range(a.inner):
                    fn()
                e1.record(stream)
                stream.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / a.inner / k)
        lin = system.linearize(x, lam, sigma)      # (the device-pointer evaluations above did not touch it; a fresh handle all the same)
        for fn, _ in host_items.values():
            fn()
        for _ in range(a.runs):
            for name, (fn, k) in host_items.items():
                t0 = time.perf_counter()
                for _ in range(a.host_inner):
                    fn()
                us[name].append((time.perf_counter() - t0) * 1e6 / a.host_inner / k)
        ops = {"J": ev._ops["J"], "JT": ev._ops["JT"], "H": ev._ops["H"]}
        fixed = {op: 12 * o.nnz + (4 * o.nnz if o.src is not None else 0) for op, o in ops.items()}

        def model_bytes(name):
            op = name.split()[0]
            if op not in ops:
                return None
            k = int(name.split("k=")[1]) if "block" in name else int(name.split()[1])
            return fixed[op] + 8 * k * sum(ops[op].shape) if "block" in name else k * (fixed[op] + 8 * sum(ops[op].shape))

        rows = {name: {"us_per_column": stat(v), "bytes": model_bytes(name)} for name, v in us.items()}
        results.append({"model": tag, "n": p.n, "m": p.m, "nnz_J_csr": mj.nnz, "nnz_H_symmetric": ops["H"].nnz, "rows": rows})
        lines.append(f"# {tag}: n {p.n}, m {p.m}, J {mj.nnz} entries, H {ops['H'].nnz} (symmetric)")
        lines.append(f"# {'':<28} {'us per column [median, min, max]':>34} {'MB moved (model)':>18}")
        for name, r in rows.items():
            mb = "" if r["bytes"] is None else f"{r['bytes'] / 1e6:.2f}"
            lines.append(f"  {name:<28} {str(r['us_per_column']):>34} {mb:>18}")
        ev.close()
    res = {"block": True, "runs": a.runs, "inner": a.inner, "host_inner": a.host_inner,
           "figures": "[median, min, max] in us per column", "models": results}
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
