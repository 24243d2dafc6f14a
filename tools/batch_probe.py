"""What a batch of iterates per launch (pk_cycleb) costs per entry, against the same number of single launches (pk_cycle).

    python tools/batch_probe.py [--model c3|c2] [--batches 1,2,4,8] [--runs 5] [--inner 200] [--out FILE]

Two figures per batch size B, each the median of ``--runs`` ALTERNATING runs (batch, singles, batch, ...) with min and max:

* kernel: the library's event-timed launches (pk_profile: hipExtModuleLaunchKernel events on the dispatch itself) -- the time of
  ONE pk_cycleb launch divided by B, against the time of one pk_cycle launch.  It holds the latency prefix and the store drain
  of a launch, NOT the gap between two launches: the single launches look better here than they are back to back.
* stream: wall time of ``inner`` back-to-back enqueues and one wait, per entry -- B singles from C (pk_eval_cycle_dev_repeat) against
  one pk_cycleb enqueued from this script.  It holds the launch gaps, and the host's pace where the host is slower than the GPU.

c3 = planar_quadrotor(radau, 2000, 6), 12 000 nodes, the benchmark's model; c2 = brachistochrone(radau, 200, 8), launch-bound.
On a tree without the batched kernel (an older commit) the single-launch columns are printed alone."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="c3", choices=["c3", "c2"])
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=ROOT, help="the tree whose pockit_amd is measured")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import numpy as np
    import torch

    from pockit_amd import benchmarks as models
    from pockit_amd import runtime
    import pockit_amd.radau as radau

    system, _, guess = models.planar_quadrotor(radau, 2000, 6) if a.model == "c3" else models.brachistochrone(radau, 200, 8)
    ev, p = system.evaluator, system.plan
    lib, h = ev.ctx.lib, ev.ctx.handle
    has_batch = hasattr(ev, "cycle_batch_dev")
    x, lam, _ = models.bench_inputs(system, guess)
    batches = [int(v) for v in a.batches.split(",")]
    Bmax = max(batches)
    dev = torch.device("cuda", 0)
    X = np.array([x * (1.0 + 1.0e-3 * (b + 1)) for b in range(Bmax)])
    Lam = np.array([lam + 0.01 * b for b in range(Bmax)])
    dX, dLam = torch.from_numpy(X).to(dev), torch.from_numpy(Lam).to(dev)
    out = [torch.zeros(Bmax * n, dtype=torch.float64, device=dev) for n in (1, p.n, p.m, p.nnz_J, p.nnz_H)]
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    k_cycle = runtime.KERNELS.index("pk_cycle")
    k_batch = len(runtime.KERNELS)      # K_CYCLEB follows the kernels of the model's own object (csrc/pk_launch.h)

    def read(k):
        n, ms = C.c_int64(), C.c_double()
        ev.ctx.check(lib.pk_profile_read(h, k, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def singles(count):
        ev.ctx.check(lib.pk_eval_cycle_dev_repeat(h, ptr(dX), ptr(dLam), C.c_double(1.0), *[ptr(t) for t in out], None, count, 0, None))

    def batch(B, sig):
        ev.cycle_batch_dev(B, dX.data_ptr(), dLam.data_ptr(), sig, *[t.data_ptr() for t in out])

    def timed(fn, k):
        """(event-timed us per launch of kernel k, wall us of the whole of fn)"""
        ev.profile(0)
        fn()
        ev.sync()
        t0 = time.perf_counter()
        fn()
        ev.sync()
        wall = (time.perf_counter() - t0) * 1e6
        n0, ms0 = read(k)
        ev.profile(1 << k)
        fn()
        ev.sync()
        ev.profile(0)
        n1, ms1 = read(k)
        return (ms1 - ms0) * 1e3 / max(n1 - n0, 1), wall

    rows = []
    for B in batches:
        sig = [1.0] * B
        kb, wb, ks, ws = [], [], [], []
        for _ in range(a.runs):
            if has_batch:
                kern, wall = timed(lambda: [batch(B, sig) for _ in range(a.inner)], k_batch)
                kb.append(kern / B)
                wb.append(wall / a.inner / B)
            kern, wall = timed(lambda: singles(B * a.inner), k_cycle)
            ks.append(kern)
            ws.append(wall / a.inner / B)
        stat = lambda v: None if not v else [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]  # noqa: E731
        rows.append({"B": B, "batch_kernel_us_per_entry": stat(kb), "single_kernel_us": stat(ks),
                     "batch_stream_us_per_entry": stat(wb), "singles_stream_us_per_entry": stat(ws)})
    bytes_per_entry = 8 * (1 + p.n + p.m + p.nnz_J + p.nnz_H) + 8 * (p.n + p.m)
    res = {"model": a.model, "nodes": int(sum(int(pp.layout.L_m) for pp in p.phase_plans)), "runs": a.runs, "inner": a.inner,
           "has_batch_kernel": has_batch, "bytes_per_entry": bytes_per_entry, "rows": rows, "figures": "[median, min, max] in us"}
    print(f"# {a.model}: {res['nodes']} nodes, {bytes_per_entry / 1e6:.2f} MB per entry; [median, min, max] us of {a.runs} alternating runs")
    print(f"# {'B':>2} {'pk_cycleb kernel/entry':>26} {'pk_cycle kernel':>26} {'batch stream/entry':>26} {'singles stream/entry':>26}")
    for r in rows:
        print(f"  {r['B']:>2} {str(r['batch_kernel_us_per_entry']):>26} {str(r['single_kernel_us']):>26} "
              f"{str(r['batch_stream_us_per_entry']):>26} {str(r['singles_stream_us_per_entry']):>26}")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
