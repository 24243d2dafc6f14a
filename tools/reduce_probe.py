"""What a reduction over the rows of J, J^T or the symmetric H costs on the device (pk_red_rows / pk_red_long, pk_diag), next to
the product with the same operator in the same process and next to what a caller pays today for the same vector.

    python tools/reduce_probe.py [--runs 5] [--inner 200] [--out FILE]

Per model -- c2 = brachistochrone(radau, 200, 8), c3 = planar_quadrotor(radau, 2000, 6) -- microseconds as [median, min, max]
of ``--runs`` ALTERNATING runs (every figure once per run, run after run):

* each mode (abs_sum, sq_sum, abs_max) on J, J^T and H, with and without ``w``: ``inner`` back-to-back ``operator_reduce_dev``
  on one stream between two HIP events, per call; diag H (``operator_diagonal_dev``) the same way;
* the product: ``apply_operator_dev`` with the same operator, timed the same way in the same run -- the yardstick, its kernels
  being those of the parent commit;
* today: wall time of the host-landed ``jacobian_csr`` / ``hessian_csr`` plus the NumPy reduction a user would write
  (``np.add.reduceat`` / ``np.maximum.reduceat`` over the CSR values of J; for J^T ``np.add.at`` by column), per call;
* the host forms of a ``Linearization`` (``row_norms``, ``jtdj_diag(d, with_h=True)``): wall time per call, one round trip each.

bytes = what a reduction moves at least: 12 per entry (value, column), 4 more with src, 8 per row, 8 per column with ``w``
(the product: 8 per row and per column)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("abs_sum", "sq_sum", "abs_max")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--host-inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
        cj, ch = zeros(mj.nnz), zeros(mh.nnz)
        rng = np.random.default_rng(0)
        hn, hm = rng.uniform(0.5, 2.0, p.n), rng.uniform(0.5, 2.0, p.m)
        wn, wm, yn, ym = up(hn), up(hm), zeros(p.n), zeros(p.m)
        torch.cuda.synchronize()
        ev.jacobian_csr_dev(dx.data_ptr(), cj.data_ptr(), st)
        ev.hessian_csr_dev(dx.data_ptr(), dlam.data_ptr(), sigma, ch.data_ptr(), st)
        stream.synchronize()
        shapes = {"J": (cj, wn, ym), "JT": (cj, wm, yn), "H": (ch, wn, yn)}      # values, a vector of n_cols, a result of n_rows
        device_items = {}
        for op, (vals, w, y) in shapes.items():
            device_items[f"{op} product"] = lambda op=op, vals=vals, w=w, y=y: ev.apply_operator_dev(
                op, vals.data_ptr(), w.data_ptr(), y.data_ptr(), stream=st)
            for mode in MODES:
                device_items[f"{op} {mode}"] = lambda op=op, mode=mode, vals=vals, y=y: ev.operator_reduce_dev(
                    op, mode, vals.data_ptr(), y.data_ptr(), stream=st)
                device_items[f"{op} {mode} w"] = lambda op=op, mode=mode, vals=vals, w=w, y=y: ev.operator_reduce_dev(
                    op, mode, vals.data_ptr(), y.data_ptr(), d_w=w.data_ptr(), stream=st)
        device_items["H diagonal"] = lambda: ev.operator_diagonal_dev("H", ch.data_ptr(), yn.data_ptr(), stream=st)
        rows_of_j = np.repeat(np.arange(p.m), np.diff(mj.indptr))
        live = np.flatnonzero(np.diff(mj.indptr) > 0)

        def today_rows(kind):
            v = system.jacobian_csr(x).data      # (a csr_array in the structure of the map)
            t = v * v if kind == "sq_sum" else np.abs(v)
            out = np.zeros(p.m)
            out[live] = (np.maximum if kind == "abs_max" else np.add).reduceat(t, mj.indptr[:-1][live])
            return out

        def today_columns():
            v = system.jacobian_csr(x).data      # (a csr_array in the structure of the map)
            out = np.zeros(p.n)
            np.add.at(out, mj.indices, v * v * hm[rows_of_j])
            return out

        def today_h_diagonal():
            return system.hessian_csr(x, lam, sigma).diagonal()

        host_items = {"today: jacobian_csr + NumPy row sums of |J|": lambda: today_rows("abs_sum"),
                      "today: jacobian_csr + NumPy row maxima of |J|": lambda: today_rows("abs_max"),
                      "today: jacobian_csr + NumPy diag(J^T D J)": today_columns,
                      "today: hessian_csr + SciPy diagonal": today_h_diagonal}
        for fn in list(device_items.values()) + list(host_items.values()):      # operators uploaded, caches warm
            fn()
        stream.synchronize()
        us = {name: [] for name in list(device_items) + list(host_items)}
        lin_items = {"row_norms('J', '1') (host form)": lambda lin: lin.row_norms("J", "1"),
                     "row_norms('JT', 'inf') (host form)": lambda lin: lin.row_norms("JT", "inf"),
                     "jdjt_diag(d) (host form)": lambda lin: lin.jdjt_diag(hn),
                     "jtdj_diag(d, with_h=True) (host form)": lambda lin: lin.jtdj_diag(hm, with_h=True),
                     "h_diag() (host form)": lambda lin: lin.h_diag()}
        us.update({name: [] for name in lin_items})
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
            lin = system.linearize(x, lam, sigma)      # (the host-landed calls above ended the one before)
            for name, fn in lin_items.items():
                fn(lin)
                t0 = time.perf_counter()
                for _ in range(a.host_inner):
                    fn(lin)
                us[name].append((time.perf_counter() - t0) * 1e6 / a.host_inner)
        ops = {op: ev._ops[op] for op in ("J", "JT", "H")}
        fixed = {op: 12 * o.nnz + (4 * o.nnz if o.src is not None else 0) for op, o in ops.items()}

        def model_bytes(name):
            op = name.split()[0]
            if name == "H diagonal":
                return 4 * p.n + 8 * p.n + 8 * p.n
            if op not in ops or "host form" in name:
                return None
            n_rows, n_cols = ops[op].shape
            return fixed[op] + 8 * n_rows + (8 * n_cols if name.endswith(" w") or name.endswith("product") else 0)

        rows = {name: {"us": stat(v), "bytes": model_bytes(name)} for name, v in us.items()}
        for op in ops:      # a reduction against the product with the same operator, and the spread of the product's own runs
            prod = rows[f"{op} product"]["us"]
            for mode in MODES:
                for suffix in ("", " w"):
                    r = rows[f"{op} {mode}{suffix}"]
                    r["minus_product_us"] = round(r["us"][0] - prod[0], 2)
                    r["product_spread_us"] = round(prod[2] - prod[1], 2)
        results.append({"model": tag, "n": p.n, "m": p.m, "nnz_J_csr": mj.nnz, "nnz_H_csr": mh.nnz,
                        "nnz_H_symmetric": ops["H"].nnz, "rows": rows})
        lines.append(f"# {tag}: n {p.n}, m {p.m}, J {mj.nnz} entries, H {mh.nnz} (lower) / {ops['H'].nnz} (symmetric)")
        lines.append(f"# {'':<46} {'us [median, min, max]':>28} {'MB moved':>10} {'GB/s':>8} {'- product':>10} {'its spread':>11}")
        for name, r in rows.items():
            mb = "" if r["bytes"] is None else f"{r['bytes'] / 1e6:.2f}"
            rate = "" if r["bytes"] is None else f"{r['bytes'] / r['us'][0] / 1e3:.0f}"
            diff = "" if "minus_product_us" not in r else f"{r['minus_product_us']:+.2f}"
            spread = "" if "product_spread_us" not in r else f"{r['product_spread_us']:.2f}"
            lines.append(f"  {name:<46} {str(r['us']):>28} {mb:>10} {rate:>8} {diff:>10} {spread:>11}")
        ev.close()
    res = {"runs": a.runs, "inner": a.inner, "host_inner": a.host_inner, "figures": "[median, min, max] in us", "models": results}
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
