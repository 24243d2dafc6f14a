"""What a merit scan costs per trial point as the HOST sees it, against the x-only batch that brings grad f, g and J home.

    python tools/merit_probe.py [--batches 1,2,4,8,16] [--runs 5] [--inner 20] [--out FILE]

Both sides are host-array calls of the same build that end in their own synchronize, timed with the host clock around
``inner`` calls: ``System.merit_scan(x, d, alphas)`` (x and d go up, the trial points are formed on the device, 8 B doubles come
back) against ``System.evaluate_batch(X, None)`` at the same B on the same trial points (X goes up; f, grad f, g and J of every
entry come back).  The comparison is "merit_scan against evaluate_batch x-only at the same B, same build"; a difference counts
only where it exceeds the spread of the runs.  Per B and model: [median, min, max] microseconds per trial point over ``runs``
ALTERNATING runs (scan, batch, scan, ...), every shape warmed up first, and beside each figure the bytes the call moves over
PCIe per trial point, computed from the shapes.

Models: brachistochrone(radau, 200, 8) (launch-bound) and planar_quadrotor(radau, 2000, 6) (12 000 nodes, the benchmark's).
Needs a GPU: there is no CPU path to time."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np

    from pockit_amd import benchmarks as models
    import pockit_amd.radau as radau

    batches = [int(v) for v in a.batches.split(",")]
    stat = lambda v: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)]  # noqa: E731
    results = []
    for label, build in (("brachistochrone(radau, 200, 8)", lambda: models.brachistochrone(radau, 200, 8)),
                         ("planar_quadrotor(radau, 2000, 6)", lambda: models.planar_quadrotor(radau, 2000, 6))):
        system, _, guess = build()
        p = system.plan
        x = np.asarray(models.bench_inputs(system, guess)[0], dtype=np.float64)
        d = 1.0e-3 * np.random.default_rng(11).standard_normal(p.n)
        served = system.evaluator._ensure_batch()

        def timed(fn):
            t0 = time.perf_counter()
            for _ in range(a.inner):
                fn()
            return (time.perf_counter() - t0) * 1e6 / a.inner

        rows = []
        for B in batches:
            alphas = np.ldexp(1.0, -np.arange(B))
            X = x[None, :] + alphas[:, None] * d[None, :]
            scan = lambda: system.merit_scan(x, d, alphas)  # noqa: E731
            full = lambda: system.evaluate_batch(X)  # noqa: E731
            want = system.merit_batch(X, d).table      # (warm-up of every shape, and the two sides agree on what they compute)
            assert np.array_equal(scan().table, want, equal_nan=True)
            full()
            ts, tf = [], []
            for _ in range(a.runs):
                ts.append(timed(scan) / B)
                tf.append(timed(full) / B)
            rows.append({"B": B, "merit_scan_us_per_point": stat(ts), "evaluate_batch_us_per_point": stat(tf),
                         "merit_scan_pcie_bytes_per_point": 8 * (2 * p.n + B + 8 * B) // B,
                         "evaluate_batch_pcie_bytes_per_point": 8 * (p.n + 1 + p.n + p.m + p.nnz_J)})
        results.append({"model": label, "n": p.n, "m": p.m, "nnz_J": p.nnz_J, "batch_served_by": served, "rows": rows})
        print(f"# {label}: n = {p.n}, m = {p.m}, nnz_J = {p.nnz_J}; batch served by the {served}; host-landed us per trial point, "
              f"[median, min, max] of {a.runs} alternating runs of {a.inner} calls; bytes over PCIe per trial point")
        print(f"# {'B':>2} {'merit_scan':>28} {'bytes':>10} {'evaluate_batch x-only':>28} {'bytes':>10}")
        for r in rows:
            print(f"  {r['B']:>2} {str(r['merit_scan_us_per_point']):>28} {r['merit_scan_pcie_bytes_per_point']:>10} "
                  f"{str(r['evaluate_batch_us_per_point']):>28} {r['evaluate_batch_pcie_bytes_per_point']:>10}")
        system.evaluator.close()
    res = {"runs": a.runs, "inner": a.inner, "figures": "[median, min, max] in us per trial point", "models": results}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
