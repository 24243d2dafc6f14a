"""Host-landed time of ``interior_point.solve`` (direct) against ``optimizer.scipy.solve`` (trust-constr) on the brachistochrone,
and of one resident round of the interior-point iteration (everything but the linear solve) against the same quantities in NumPy
on downloaded vectors -- what a caller writes without the units.  Needs an MI355X; prints a table.

    python tools/ip_solve_probe.py [--runs 5] [--out profiles/ip_solve_probe_mi355x.txt] [--quadrotor]

``--banded`` runs the rows of DESIGN.md section 23 instead: ``linear_solver="banded"`` alternating with ``"direct"`` on both
sizes, and the host-landed time of one factorisation and of one solve of the band LU with their launches (``--append`` adds the
rows to ``--out`` instead of replacing it).  ``--banded-batch`` runs the rows of section 24: the batch forms of the band LU at
B = 1, 2, 4, 8 against B single factorisations and solves in a row, and whole solves with ``band_attempts`` = 1, 2, 4.
``--multi`` runs the rows of section 27: after one factorisation one block solve at k = 1, 8, 64 against k calls of
``band_solve_dev``, and a whole solve of the parametrised LQR with ``sensitivity="fixed"`` against the same solve without it.
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

MODELS = [("brachistochrone", "radau", 10, 8), ("brachistochrone", "radau", 200, 8)]
MU, TAU = 0.1, 0.99


def spread(samples, scale=1.0, fmt="9.1f"):
    return f"{statistics.median(samples) * scale:{fmt}} [{min(samples) * scale:.1f}, {max(samples) * scale:.1f}]"


def resident_round(R, ipm):
    """measure (terms of x and s at mu and at 0, r_d, slack_reduce) + b1 + H dx + slack_recover + ip_step of x and s + the merit of
    two trial points' slacks; the updates are left out so that the round can be repeated on the same iterate.  Records down."""
    ev, at, n = R.ev, R.at, R.n
    q = R.measure(MU)
    ev.dual_residual_dev(at(R.cj), at(R.grad), at(R.lam), at(R.rhs), at(R.rec, 40), d_z=at(R.rbar_x), negate=True)
    ev.apply_operator_dev("H", at(R.ch), at(R.sol), at(R.w))
    ev.slack_recover_dev(at(R.sol, n), at(R.lam), at(R.rbar_s), at(R.s2), at(R.sig_s), at(R.sol), at(R.w), at(R.sig_x), at(R.ds), at(R.rec, 44))
    ev.ip_step_dev(at(R.x), at(R.sol), at(R.zl), at(R.zu), MU, TAU, at(R.dzl), at(R.dzu), at(R.rec, 52))
    ev.ip_step_dev(at(R.s), at(R.ds), at(R.yl), at(R.yu), MU, TAU, at(R.dyl), at(R.dyu), at(R.rec, 56), which="c")
    R.to_torch()
    return q, R.down(R.rec)


def numpy_round(R, J, H):
    """The same quantities on downloaded vectors: x, s, lam, the four multipliers, g, grad and the step come down (J and H lie
    on the host as SciPy matrices already), sigma_x, s2 and the right-hand side go up again."""
    n, m = R.n, R.m
    x, s, lam, zl, zu, yl, yu, g, grad = (R.down(t, c).copy() for t, c in ((R.x, n), (R.s, m), (R.lam, m), (R.zl, n), (R.zu, n), (R.yl, m),
                                                                            (R.yu, m), (R.g, m), (R.grad, n)))
    sol = R.down(R.sol, n + m).copy()
    dx, dlam = sol[:n], sol[n:]
    out = {}
    with np.errstate(all="ignore"):
        for name, v, lb, ub, a, b, dv in (("x", x, R.v_lb, R.v_ub, zl, zu, dx), ("s", s, R.c_lb, R.c_ub, yl, yu, None)):
            boxed = lb != ub
            lo, up = boxed & np.isfinite(lb), boxed & np.isfinite(ub)
            dl, du = np.where(lo, v - lb, 1.0), np.where(up, ub - v, 1.0)
            sigma = np.where(lo, a / dl, 0.0) + np.where(up, b / du, 0.0)
            rbar = np.where(lo, MU / dl, 0.0) - np.where(up, MU / du, 0.0)
            compl = max(np.max(np.abs(dl * a - MU), where=lo, initial=0.0), np.max(np.abs(du * b - MU), where=up, initial=0.0))
            compl0 = max(np.max(dl * a, where=lo, initial=0.0), np.max(du * b, where=up, initial=0.0))
            logs = np.sum(np.log(dl), where=lo) + np.sum(np.log(du), where=up)
            out[name] = dict(lo=lo, up=up, dl=dl, du=du, sigma=sigma, rbar=rbar, compl=compl, compl0=compl0, logs=logs, z_sum=a[lo].sum() + b[up].sum())
        ineq = R.c_lb != R.c_ub
        r_d = np.where(R.free, J.T @ lam + grad - zl + zu, 0.0)
        r_s = np.where(ineq, -lam - yl + yu, 0.0)
        s2 = np.where(ineq, 1.0 / out["s"]["sigma"], 0.0)
        res = np.where(ineq, g - s, g - R.c_lb)
        b2 = -res + s2 * np.where(ineq, lam + out["s"]["rbar"], 0.0)
        b1 = np.where(R.free, -(J.T @ lam + grad - out["x"]["rbar"]), 0.0)
        ds = s2 * np.where(ineq, dlam + lam + out["s"]["rbar"], 0.0)
        curv = dx @ (H @ dx) + out["x"]["sigma"] @ (dx * dx) + np.where(ineq, out["s"]["sigma"], 0.0) @ (ds * ds)
        alphas = []
        for name, dv, a, b in (("x", dx, zl, zu), ("s", ds, yl, yu)):
            o = out[name]
            dza = np.where(o["lo"], (MU / o["dl"] - a) - (a / o["dl"]) * dv, 0.0)
            dzb = np.where(o["up"], (MU / o["du"] - b) + (b / o["du"]) * dv, 0.0)
            cand = np.concatenate(((TAU * o["dl"])[o["lo"] & (dv < 0)] / -dv[o["lo"] & (dv < 0)], (TAU * o["du"])[o["up"] & (dv > 0)] / dv[o["up"] & (dv > 0)]))
            cz = np.concatenate(((TAU * a)[o["lo"] & (dza < 0)] / -dza[o["lo"] & (dza < 0)], (TAU * b)[o["up"] & (dzb < 0)] / -dzb[o["up"] & (dzb < 0)]))
            alphas.append((min(1.0, cand.min(initial=1.0)), min(1.0, cz.min(initial=1.0))))
    R.s1 = R.up(out["x"]["sigma"])
    R.s2 = R.up(s2)
    R.rhs = R.up(np.concatenate((b1, b2)))
    R.to_kernels()
    return dict(r_d=np.abs(r_d).max(), r_s=np.abs(r_s).max(), theta=np.abs(res).max(), theta_1=np.abs(res).sum(), curv=curv, alphas=alphas,
                compl=max(out["x"]["compl"], out["s"]["compl"]), compl0=max(out["x"]["compl0"], out["s"]["compl0"]))


def banded_rows(args, models, ipm):
    """``"banded"`` alternating with ``"direct"``: whole solves, then one factorisation and one solve of the band LU at the
    start point (enqueue and wait, host-landed), with the launches they take."""
    from pockit_amd.band import BandOrdering

    lines = [f"ip_solve_probe --banded: interior_point.solve, linear_solver \"banded\" alternating with \"direct\" (tol 1e-8); median [min, max] of "
             f"{args.runs} runs each, host-landed (perf_counter around whole solves and around enqueue + wait)"]
    for name, scheme, mesh, num_point in MODELS:
        ns = importlib.import_module(f"pockit_amd.{scheme}")
        system, _, guess = getattr(models, name)(ns, mesh, num_point)
        times, infos = {"direct": [], "banded": []}, {}
        ipm.solve(system, guess, linear_solver="banded")                    # warm-up: code objects, the batch's self-check
        for _ in range(args.runs):
            for solver in ("direct", "banded"):
                t0 = time.perf_counter()
                _, infos[solver] = ipm.solve(system, guess, linear_solver=solver)
                times[solver].append(time.perf_counter() - t0)
        lines.append(f"{name}({scheme}, {mesh}, {num_point}): n {system.plan.n}, m {system.plan.m}")
        for solver in ("direct", "banded"):
            info = infos[solver]
            per = [t / max(1, info["iterations"]) for t in times[solver]]
            lines.append(f"    {solver:7s} {spread(times[solver], 1e3)} ms per solve, {spread(per, 1e3, '9.2f')} ms per iteration; status {info['status']}, "
                         f"{info['iterations']} Newton iterations, {info['regularisations']} regularised, f = {info['obj_val']:.10f}, E_0 {info['error']:.2e}")
        R = ipm._Resident(system, ipm.preprocess(system, guess, None)[0])
        R.evaluate()
        R.to_torch()
        t0 = time.perf_counter()
        o = BandOrdering(R.map_j, R.map_h, R.free)
        t_order = time.perf_counter() - t0
        t0 = time.perf_counter()
        R.ev.band_plan(o)
        t_plan = time.perf_counter() - t0
        R.s1 = R.up(np.ones(R.n))
        R.s2 = R.up(np.where(R.ineq, 1.0, 0.0))
        R.rhs = R.up(np.random.default_rng(3).standard_normal(R.n + R.m))
        R.to_kernels()
        at, ev = R.at, R.ev
        t_f, t_s = [], []
        for _ in range(args.runs + 1):
            t0 = time.perf_counter()
            ev.band_factor_dev(at(R.ch), at(R.cj), at(R.s1), at(R.s2))
            ev.sync()
            t1 = time.perf_counter()
            ev.band_solve_dev(at(R.rhs), at(R.sol))
            ev.sync()
            t2 = time.perf_counter()
            t_f.append(t1 - t0)
            t_s.append(t2 - t1)
        rec = ev.band_record()
        panels = -(-o.nb // 32)
        lines.append(f"    ordering N {o.N}, Nb {o.nb}, w {o.w}, p {o.p}: {t_order * 1e3:.1f} ms on the host once per solve; plan upload ({8 * o.dests} bytes of map) "
                     f"{t_plan * 1e3:.1f} ms")
        lines.append(f"    factor  {spread(t_f[1:], 1e3, '9.3f')} ms: {2 + 2 * panels} launches at most (init, fill, {panels} panels with their updates), "
                     f"{8 * o.dests} bytes of [band | U | C] written; status {int(rec[0])}, {int(rec[7])} interchanges, pivots [{rec[2]:.2e}, {rec[3]:.2e}]")
        lines.append(f"    solve   {spread(t_s[1:], 1e3, '9.3f')} ms: {6 if o.p else 3} launches (right-hand sides, sweeps"
                     f"{', dots, border, x_B' if o.p else ''}, scatter), {o.p + 1} right-hand side{'s' if o.p else ''} of {o.nb} in one workgroup each")
        system.evaluator.close()
    return lines


def refine_rows(args, models, ipm):
    """``--banded --refine R``: whole solves with ``band_refine`` = R alternating with 0, what the refinement
    saw over a solve (the largest and the median rho_0, the corrections), and one begin and one step at the start point (enqueue
    and wait, host-landed)."""
    from pockit_amd.band import BandOrdering

    r = args.refine
    lines = [f"ip_solve_probe --banded --refine {r}: interior_point.solve, linear_solver \"banded\", band_refine {r} alternating with 0 (tol 1e-8); "
             f"median [min, max] of {args.runs} runs each, host-landed"]
    for name, scheme, mesh, num_point in MODELS:
        ns = importlib.import_module(f"pockit_amd.{scheme}")
        system, _, guess = getattr(models, name)(ns, mesh, num_point)
        ev = system.evaluator
        seen = []
        record = ev.band_refine_record

        def spy():
            rec = record()
            seen.append(rec.copy())
            return rec

        times, infos = {0: [], r: []}, {}
        ipm.solve(system, guess, linear_solver="banded", band_refine=r)                    # warm-up
        ev.band_refine_record = spy
        for _ in range(args.runs):
            for k in (0, r):
                del seen[:]
                t0 = time.perf_counter()
                _, infos[k] = ipm.solve(system, guess, linear_solver="banded", band_refine=k)
                times[k].append(time.perf_counter() - t0)
        del ev.band_refine_record
        lines.append(f"{name}({scheme}, {mesh}, {num_point}): n {system.plan.n}, m {system.plan.m}")
        for k in (0, r):
            info = infos[k]
            per = [t / max(1, info["iterations"]) for t in times[k]]
            lines.append(f"    band_refine {k}: {spread(times[k], 1e3)} ms per solve, {spread(per, 1e3, '9.2f')} ms per iteration; status {info['status']}, "
                         f"{info['iterations']} Newton iterations, {info['regularisations']} regularised, f = {info['obj_val']:.10f}, E_0 {info['error']:.2e}")
        first = np.array([rec[6] for rec in seen if rec[0] != 4.0])
        if len(first):
            lines.append(f"    rho_0 over the last solve ({len(first)} records read): largest {first.max():.2e}, median {np.median(first):.2e}; "
                         f"{infos[r]['refinement_steps']} corrections, the largest accepted rho {infos[r]['residual_ratio']:.2e}")
        R = ipm._Resident(system, ipm.preprocess(system, guess, None)[0])
        R.evaluate()
        R.to_torch()
        R.ev.band_plan(BandOrdering(R.map_j, R.map_h, R.free))
        R.s1 = R.up(np.ones(R.n))
        R.s2 = R.up(np.where(R.ineq, 1.0, 0.0))
        R.rhs = R.up(np.random.default_rng(3).standard_normal(R.n + R.m))
        R.to_kernels()
        at = R.at
        ev.band_factor_dev(at(R.ch), at(R.cj), at(R.s1), at(R.s2))
        t_b, t_s = [], []
        for _ in range(args.runs + 1):
            ev.band_solve_dev(at(R.rhs), at(R.sol))
            ev.sync()
            t0 = time.perf_counter()
            ev.band_refine_begin_dev(at(R.ch), at(R.cj), at(R.s1), at(R.s2), at(R.rhs), at(R.sol), 0.0, 0)
            ev.sync()
            t1 = time.perf_counter()
            ev.band_refine_advance_dev(1)
            ev.sync()
            t2 = time.perf_counter()
            t_b.append(t1 - t0)
            t_s.append(t2 - t1)
        rec = ev.band_refine_record()
        lines.append(f"    begin   {spread(t_b[1:], 1e3, '9.3f')} ms (the product with K, the residual, the record)")
        lines.append(f"    step    {spread(t_s[1:], 1e3, '9.3f')} ms (one solve, the correction, the product, the residual, the record); at the start point "
                     f"rho_0 {rec[6]:.2e}, rho_1 {rec[5]:.2e}, status {int(rec[0])}")
        ev.close()
    return lines


def banded_batch_rows(args, models, ipm):
    """one batched factorisation and one batched solve at B = 1, 2, 4, 8 against B single ones in a row on
    the same values (enqueue and wait, host-landed, alternating), then whole solves with ``band_attempts`` = 1, 2, 4."""
    from pockit_amd.band import BandOrdering

    lines = [f"ip_solve_probe --banded-batch: the batch forms of the band LU against the single forms; median [min, max] of {args.runs} runs each, "
             f"alternating, host-landed (perf_counter around enqueue + wait and around whole solves)"]
    for name, scheme, mesh, num_point in MODELS:
        ns = importlib.import_module(f"pockit_amd.{scheme}")
        system, _, guess = getattr(models, name)(ns, mesh, num_point)
        lines.append(f"{name}({scheme}, {mesh}, {num_point}): n {system.plan.n}, m {system.plan.m}")
        R = ipm._Resident(system, ipm.preprocess(system, guess, None)[0])
        R.evaluate()
        R.to_torch()
        o = BandOrdering(R.map_j, R.map_h, R.free)
        R.ev.band_plan(o)
        n, m, torch = R.n, R.m, R.torch
        R.s2 = R.up(np.where(R.ineq, 1.0, 0.0))
        R.rhs = R.up(np.random.default_rng(3).standard_normal(n + m))
        at, ev = R.at, R.ev
        for B in (1, 2, 4, 8):
            s1 = torch.stack([torch.ones(n, dtype=torch.float64, device=R.dev) * (1.0 + 0.25 * e) for e in range(B)])
            sol, one = torch.zeros((B, n + m), dtype=torch.float64, device=R.dev), torch.zeros(n + m, dtype=torch.float64, device=R.dev)
            R.to_kernels()
            t = {"factor batch": [], "solve batch": [], "factor singles": [], "solve singles": []}
            for _ in range(args.runs + 1):
                t0 = time.perf_counter()
                ev.band_factor_batch_dev(B, at(R.ch), at(R.cj), at(s1), at(R.s2))
                ev.sync()
                t1 = time.perf_counter()
                ev.band_solve_batch_dev(B, at(R.rhs), at(sol))
                ev.sync()
                t2 = time.perf_counter()
                t["factor batch"].append(t1 - t0)
                t["solve batch"].append(t2 - t1)
                tf = ts = 0.0
                for e in range(B):
                    t0 = time.perf_counter()
                    ev.band_factor_dev(at(R.ch), at(R.cj), at(s1[e]), at(R.s2))
                    ev.sync()
                    t1 = time.perf_counter()
                    ev.band_solve_dev(at(R.rhs), at(one))
                    ev.sync()
                    tf, ts = tf + (t1 - t0), ts + (time.perf_counter() - t1)
                t["factor singles"].append(tf)
                t["solve singles"].append(ts)
            records = ev.band_record_batch(B)
            R.to_torch()
            same = bool(torch.equal(sol[B - 1], one))
            med = {k: statistics.median(v[1:]) for k, v in t.items()}
            lines.append(f"    B {B}: factor batch {spread(t['factor batch'][1:], 1e3, '9.3f')} ms, {B} singles {spread(t['factor singles'][1:], 1e3, '9.3f')} ms, "
                         f"ratio t_batch / (B t_single) {med['factor batch'] / med['factor singles']:.3f}; solve batch {spread(t['solve batch'][1:], 1e3, '9.3f')} ms, "
                         f"{B} singles {spread(t['solve singles'][1:], 1e3, '9.3f')} ms, ratio {med['solve batch'] / med['solve singles']:.3f}; "
                         f"statuses {[int(s) for s in records[:, 0]]}, last entry bit-equal to the single solve: {same}")
        system.evaluator.close()
        system, _, guess = getattr(models, name)(ns, mesh, num_point)
        attempts = (1, 2, 4)
        times, infos = {k: [] for k in attempts}, {}
        ipm.solve(system, guess, linear_solver="banded")                    # warm-up
        for _ in range(args.runs):
            for k in attempts:
                t0 = time.perf_counter()
                _, infos[k] = ipm.solve(system, guess, linear_solver="banded", band_attempts=k)
                times[k].append(time.perf_counter() - t0)
        for k in attempts:
            info = infos[k]
            per = [x / max(1, info["iterations"]) for x in times[k]]
            lines.append(f"    band_attempts {k}: {spread(times[k], 1e3)} ms per solve, {spread(per, 1e3, '9.2f')} ms per iteration; status {info['status']}, "
                         f"{info['iterations']} Newton iterations, {info['regularisations']} regularised, f = {info['obj_val']:.10f}")
        system.evaluator.close()
    return lines


def multi_rows(args, models, ipm):
    """after one factorisation, one block solve of k right-hand sides against k single solves in a row
    (enqueue and wait, host-landed, alternating), then a whole solve with ``sensitivity="fixed"`` against one without."""
    from pockit_amd.band import BandOrdering

    lines = [f"ip_solve_probe --multi: band_solve_multi_dev (k right-hand sides, the launches of one solve) against k calls of band_solve_dev after one "
             f"factorisation; median [min, max] of {args.runs} runs each, alternating, host-landed (perf_counter around enqueue + wait)"]
    for name, scheme, mesh, num_point in reversed(MODELS):
        ns = importlib.import_module(f"pockit_amd.{scheme}")
        system, _, guess = getattr(models, name)(ns, mesh, num_point)
        R = ipm._Resident(system, ipm.preprocess(system, guess, None)[0])
        R.evaluate()
        R.to_torch()
        o = BandOrdering(R.map_j, R.map_h, R.free)
        R.ev.band_plan(o)
        n, m, torch = R.n, R.m, R.torch
        lines.append(f"{name}({scheme}, {mesh}, {num_point}): n {n}, m {m}, Nb {o.nb}, w {o.w}, p {o.p}")
        R.s1 = R.up(np.ones(n))
        R.s2 = R.up(np.where(R.ineq, 1.0, 0.0))
        rhs = torch.from_numpy(np.random.default_rng(3).standard_normal((64, n + m))).to(R.dev)
        R.to_kernels()
        at, ev = R.at, R.ev
        ev.band_factor_dev(at(R.ch), at(R.cj), at(R.s1), at(R.s2))
        ev.sync()
        for k in (1, 8, 64):
            sol, one = torch.zeros((k, n + m), dtype=torch.float64, device=R.dev), torch.zeros((k, n + m), dtype=torch.float64, device=R.dev)
            R.to_kernels()
            t_block, t_singles = [], []
            for _ in range(args.runs + 1):
                t0 = time.perf_counter()
                ev.band_solve_multi_dev(k, at(rhs), at(sol))
                ev.sync()
                t1 = time.perf_counter()
                for c in range(k):
                    ev.band_solve_dev(at(rhs[c]), at(one[c]))
                ev.sync()
                t_block.append(t1 - t0)
                t_singles.append(time.perf_counter() - t1)
            R.to_torch()
            same = bool(torch.equal(sol, one))
            ratio = statistics.median(t_block[1:]) / statistics.median(t_singles[1:])
            lines.append(f"    k {k:2d}: block {spread(t_block[1:], 1e3, '9.3f')} ms ({o.p + k} workgroups in the sweeps), {k} singles in a row (one wait) "
                         f"{spread(t_singles[1:], 1e3, '9.3f')} ms, ratio {ratio:.3f}, block / one single {statistics.median(t_block[1:]) * k / statistics.median(t_singles[1:]):.2f}; "
                         f"bit-equal: {same}; status {int(ev.band_record()[0])}")
        system.evaluator.close()
    import sensitivity_models as sm

    for solver in ("banded", "direct"):
        ns = importlib.import_module("pockit_amd.radau")
        system, _, guess = sm.param_lqr(ns, 200, 8, 1.0)
        times, infos = {None: [], "fixed": []}, {}
        ipm.solve(system, guess, linear_solver=solver)                         # warm-up
        for _ in range(args.runs):
            for sens in (None, "fixed"):
                t0 = time.perf_counter()
                _, infos[sens] = ipm.solve(system, guess, linear_solver=solver, sensitivity=sens)
                times[sens].append(time.perf_counter() - t0)
        s = infos["fixed"]["sensitivity"]
        lines.append(f"param_lqr(radau, 200, 8), {solver}: n {system.plan.n}, m {system.plan.m}; without sensitivity {spread(times[None], 1e3)} ms, with "
                     f"sensitivity=\"fixed\" ({len(s['parameters'])} parameter) {spread(times['fixed'], 1e3)} ms; {infos['fixed']['iterations']} iterations, "
                     f"status {s['status']}, dobj {s['dobj'][0]:.10f}, 2 f {2 * infos['fixed']['obj_val']:.10f}")
        system.evaluator.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--multi", action="store_true", help="the rows of the block solve and the sensitivities instead (DESIGN.md section 27)")
    ap.add_argument("--banded-batch", action="store_true", help="the rows of the batched band LU instead (DESIGN.md section 24)")
    ap.add_argument("--banded", action="store_true", help="the rows of the banded step solver instead (DESIGN.md section 23)")
    ap.add_argument("--refine", type=int, default=0, help="with --banded: band_refine R alternating with 0 instead (DESIGN.md section 29)")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quadrotor", action="store_true", help="also run planar_quadrotor(radau, 14, 6) once and report what happens")
    ap.add_argument("--trust-constr-large", type=int, default=1, help="trust-constr runs on the large model (each takes minutes)")
    ap.add_argument("--large-maxiter", type=int, default=400, help="trust-constr's maxiter on the large model")
    args = ap.parse_args()
    if args.refine and not args.banded:
        ap.error("--refine needs --banded")
    if not 0 <= args.refine <= 10:
        ap.error("--refine takes 0 ... 10")
    import models
    from pockit_amd.optimizer import interior_point as ipm
    from pockit_amd.optimizer import scipy as scipy_solver

    if args.banded or args.banded_batch or args.multi:
        text = "\n".join((multi_rows if args.multi else banded_batch_rows if args.banded_batch else refine_rows if args.refine else banded_rows)(args, models, ipm)) + "\n"
        print(text, end="")
        if args.out:
            with open(args.out, "a" if args.append else "w") as fh:
                fh.write(text)
        return
    lines = [f"ip_solve_probe: interior_point.solve (direct, tol 1e-8) against optimizer.scipy.solve (trust-constr, gtol 1e-9, xtol 1e-11); "
             f"median [min, max] of {args.runs} alternating runs, host-landed (perf_counter around whole solves and around rounds that end in a wait)"]
    for name, scheme, mesh, num_point in MODELS:
        ns = importlib.import_module(f"pockit_amd.{scheme}")
        system, _, guess = getattr(models, name)(ns, mesh, num_point)
        large = system.plan.n > 2000
        _, info = ipm.solve(system, guess)                                    # warm-up: code objects, the batch's self-check
        t_ip, t_tc, its, tc_its, tc_f = [], [], [], [], []
        for k in range(args.runs):
            t0 = time.perf_counter()
            _, info = ipm.solve(system, guess)
            t1 = time.perf_counter()
            t_ip.append(t1 - t0)
            its.append(info["iterations"])
            if not large or k < args.trust_constr_large:
                t0 = time.perf_counter()
                _, res = scipy_solver.solve(system, guess, {"maxiter": args.large_maxiter if large else 400, "gtol": 1e-9, "xtol": 1e-11})
                t_tc.append(time.perf_counter() - t0)
                tc_its.append(int(res.nit))
                tc_f.append(float(res.fun))
        lines.append(f"{name}({scheme}, {mesh}, {num_point}): n {system.plan.n}, m {system.plan.m}")
        lines.append(f"    interior_point.solve (direct)   {spread(t_ip, 1e3)} ms, status {info['status']}, {its[-1]} Newton iterations, "
                     f"{info['regularisations']} regularised, f = {info['obj_val']:.10f}, E_0 {info['error']:.2e}")
        lines.append(f"    scipy trust-constr ({len(t_tc)} run{'s' if len(t_tc) != 1 else ''})    {spread(t_tc, 1e3)} ms, {tc_its[-1]} iterations (status {int(res.status)}: "
                     f"0 is trust-constr's maxiter), f = {tc_f[-1]:.10f}")
        # ---- one resident round against NumPy on downloaded vectors, at the start point with a unit step direction
        R = ipm._Resident(system, ipm.preprocess(system, guess, None)[0])
        R.evaluate()
        R.to_torch()
        R.s = R.up(np.where(R.ineq, ipm.push_inside(R.down(R.g, R.m), R.c_lb, R.c_ub), 0.0))
        rng = np.random.default_rng(3)
        R.sol = R.up(1e-3 * rng.standard_normal(R.n + R.m) * np.concatenate((R.free, np.ones(R.m))))
        R.to_kernels()
        J = R.map_j.to_scipy(R.down(R.cj, R.map_j.nnz).copy())
        L = R.map_h.to_scipy(R.down(R.ch, R.map_h.nnz).copy())
        import scipy.sparse as sp

        H = (L + L.T - sp.diags(L.diagonal())).tocsr()
        q, rec = resident_round(R, ipm)
        ref = numpy_round(R, J, H)
        agree = max(abs(q["rd"][0] - ref["r_d"]), abs(q["red"][0] - ref["theta"]), abs(rec[44] + rec[45] - ref["curv"]) / max(1.0, abs(ref["curv"])),
                    abs(min(rec[52], rec[56]) - min(ref["alphas"][0][0], ref["alphas"][1][0])))
        t_res, t_np = [], []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            resident_round(R, ipm)
            t1 = time.perf_counter()
            numpy_round(R, J, H)
            t2 = time.perf_counter()
            t_res.append(1e6 * (t1 - t0))
            t_np.append(1e6 * (t2 - t1))
        n, m = R.n, R.m
        lines.append(f"    one round but the linear solve, resident (16 launches + 2 products, 3 waits, 512 bytes of records down) {spread(t_res)} us")
        lines.append(f"    the same in NumPy: {8 * (3 * n + 6 * m + n + m)} bytes down, {8 * (2 * n + 2 * m)} bytes up    {spread(t_np)} us; "
                     f"max difference of r_d, theta, curvature (relative), alpha_primal {agree:.2e}")
        system.evaluator.close()
    if args.quadrotor:
        ns = importlib.import_module("pockit_amd.radau")
        system, _, guess = models.planar_quadrotor(ns, 14, 6)
        t0 = time.perf_counter()
        _, info = ipm.solve(system, guess)
        lines.append(f"planar_quadrotor(radau, 14, 6), direct, once: status {info['status']} ({info['status_msg']}), {info['iterations']} iterations, "
                     f"{info['regularisations']} regularised, final E_0 {info['error']:.3e}, mu {info['mu']:.1e}, {time.perf_counter() - t0:.1f} s")
        system.evaluator.close()
        ns = importlib.import_module("pockit_amd.radau")
        system, _, guess = models.brachistochrone(ns, 10, 8)
        _, info = ipm.solve(system, guess, {"max_iter": 30}, linear_solver="minres")
        lines.append(f"brachistochrone(radau, 10, 8), minres, max_iter 30, once: status {info['status']} ({info['status_msg']}), {info['iterations']} "
                     f"Newton iterations, {info['linear_iterations']} MINRES iterations in all, final E_0 {info['error']:.3e}")
        system.evaluator.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
