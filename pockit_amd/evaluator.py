"""GPU evaluator of one transcribed system: plan -> code object + device tables -> callbacks.

``Evaluator(plan)`` generates the model's HIP source, compiles (or fetches from cache) its gfx950
code object, flattens the mesh-dependent tables into the blobs of csrc/pk_abi.h, uploads
everything through the C ABI and then serves the five NLP callbacks with host NumPy arrays
(pk_eval_*), or with device pointers and a stream for callers that keep data resident (pk_eval_*_dev).

Mirrors the callback semantics of /root/reference/pockit/base/systembase.py:602-835: callbacks
return freshly allocated float64 arrays; ``x`` is borrowed and never written.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import hipbuild, runtime
from .codegen import ModelSource
from .transcription import SystemPlan

N_CU = 256      # compute units of an MI355X (one workgroup of the cycle per CU is the sweet spot, see _intervals_per_wave)


def _intervals_per_wave(plan, override=None, shards=1, subs=0, want_workgroups=False):
    """Intervals per wavefront, up to 64 nodes per wave (Layout.tiles caps it).  Measured on MI355X with pk_cycle
    (tools/ipw_sweep.sh): at 12k nodes the cycle is bound by the number of vector-memory
    instructions a CU has to issue and by the time the dispatcher needs to start the waves, so fuller waves
    (18-42 nodes: 126-133k cycles/s) beat many small ones (12 nodes: 114k, 6 nodes: 81k) as long as every CU
    still gets work; the 40k-node humanoid runs best with full 64-node waves."""
    forced = override or os.environ.get("POCKIT_AMD_IPW")        # (tests / sweeps: tools/ipw_sweep.sh)
    if forced and not want_workgroups:
        return int(forced)
    # Candidates from ~16 nodes per wave (on small meshes a wave of 6-8 nodes pays its fixed work -- tile record, table
    # staging, one streaming iteration per segment -- for a quarter of the entries: tools/ipw_small_sweep.sh, humanoid
    # 100 x 8 10.7 -> 8.2 us per cycle, quadrotor 100 x 6 4.79 -> 4.14) up to full waves; the choice minimizes the work of
    # the busiest CU.  A launch is as slow as its most loaded CU: with 303 workgroups on 256 CUs 47 CUs hold two and the
    # launch takes as long as with 504 (tools/mid_size_sweep.sh: quadrotor 3000 x 6 with 380 tiles 6.09 us, with 304 tiles
    # 5.21 us).  Cost of a candidate = workgroups per CU x (intervals per wave [x 1.5 where one wave does the Jacobian and
    # the values] + 4 for a workgroup's fixed work); ties go to the fuller waves.  The model reproduces the optimum of the
    # sweeps at 100 ... 10 000 intervals (profiles/r02_g_ipw_small.txt, r02_g_mid_size.txt, r02_z2_tile_sweep.txt).
    shards = max(1, int(shards))
    best = None
    caps = []
    for pp in plan.phase_plans:
        lay = pp.layout
        kmed = max(1, int(np.median(np.asarray(lay.K, dtype=np.int64))))
        nodes = kmed if lay.scheme == "lgr" else max(kmed - 1, 1)
        caps.append((int(lay.N), max(1, (runtime.WAVE if lay.scheme == "lgr" else runtime.WAVE - 1) // nodes), kmed))
    if not caps:
        return 1
    lo = max(1, math.ceil(16 / max(1, int(np.median([k for _, _, k in caps])))))
    hi = max(lo, max(c for _, c, _ in caps))
    if forced:      # (the workgroups of the forced tiling, not the model's choice)
        lo = hi = int(forced)
    for ipw in range(lo, hi + 1):
        tiles = 0
        for n_p, cap, _ in caps:
            t = math.ceil(max(n_p / shards - 1, 0) / min(ipw, cap)) + 1        # (the first interval is a kind of its own)
            tiles += -(-t // runtime.WAVES_PER_BLOCK) * runtime.WAVES_PER_BLOCK
        # (the grid of pk_cycle in csrc/pk_launch.h: per tile block 3 workgroups while pk_set_problem splits the x-part, up to
        #  1024 tiles, else 2, or the model's cycle_subs; + 3.  tests/test_cabi.py holds this formula against the table)
        roles = 3 if tiles <= 1024 else 2
        if subs:
            roles = int(subs)
        per_cu = math.ceil((roles * tiles // runtime.WAVES_PER_BLOCK + 3) / N_CU)
        cost = per_cu * (ipw * (1.5 if roles == 2 else 1.0) + 4.0)      # (+4: a workgroup's fixed work, in intervals)
        if best is None or cost <= best[0]:
            best = (cost, ipw, roles * tiles // runtime.WAVES_PER_BLOCK + 3)
    return best[2] if want_workgroups else best[1]


def _launch_underfills_the_chip(plan, shards=1):
    """True when the one-launch cycle of this mesh, tiled by default, has no more workgroups than the GPU has CUs: the
    cycle's time is then one wave's chain, not throughput (see compile_plan)."""
    return bool(plan.phase_plans) and _intervals_per_wave(plan, shards=shards, want_workgroups=True) <= N_CU


def model_desc(src):
    """The pk_model_desc of a generated model: what the library sizes its launches from (csrc/pk_launch.h)."""
    plan = src.plan
    md = runtime.ModelDesc()
    md.n_phase, md.n_I, md.nred = src.nphase, max(len(plan.I_syms), 1), src.nred
    md.lds_g, md.lds_j, md.lds_h, md.lds_x = src.lds_g, src.lds_j, src.lds_h, src.lds_x
    md.ne_j, md.ne_h = src.list_off["jac"]["total"], src.list_off["hess"]["total"]
    md.ne_a = src.list_off["aux"]["total"]
    md.ne_hc = src.list_off["hessc"]["total"] if src.compact else 0
    md.lds_e = src.lds_e
    md.lds_jc = src.lds_jc
    md.ne_jc = src.list_off["jacc"]["total"] if src.compact_j else 0
    md.tab_cap = src.tab_cap
    md.sharded = int(src.sharded)
    md.max_phases = src.max_phases
    md.cycle_subs = src.cycle_subs
    md.hess_subs = src.h_ngmax if src.cycle_subs else 0
    # (the stand-alone compact kernels of such a model: a workgroup per pass too)
    md.hessc_subs = src.hc_ngmax if (src.cycle_subs and src.hc_ngmax > 1) else 0
    md.jacc_subs = src.jc_ngmax if (src.cycle_subs and src.jc_ngmax > 1) else 0
    md.big_global, md.big_rows = int(src.big_global), int(src.big_rows)
    md.wide = int(any(src.wide))      # (the library then refuses pk_xall: _refuse_sequential_values_role)
    md.prepass_f = 1
    md.prepass_grad = int(plan.needs_I_grad)
    md.prepass_g = int(plan.needs_I_con)
    md.prepass_jac = int(plan.jac.needs_I)
    md.prepass_hess = int(plan.hess.needs_I)
    return md


def magic_number(d: int) -> int:
    """32-bit magic of the divisor ``d`` for the kernels' ``magic_div`` (pk_kernels.hip.h):
    ``p // d == (p * magic) >> 32`` for ``p < 2**16`` with ``magic = ceil(2**32 / d)``.  ``d == 1`` has no 32-bit magic
    (2**32): it is encoded as 0 and the kernel returns ``p`` itself; ``d == 0`` (nothing to divide) is 0 as well."""
    if d <= 1:
        return 0
    return (0xFFFFFFFF // d + 1) & 0xFFFFFFFF


def magic_div(p: int, magic: int) -> int:
    """Host model of the device function of the same name (used by the tests)."""
    return p if magic == 0 else (p * magic) >> 32


class Tables:
    """Mesh-dependent tables of a plan in the layout of csrc/pk_abi.h (host NumPy arrays).

    ``tile_filter(phase_index, tiles) -> tiles`` lets a rank keep only its shard of the tiles."""

    def __init__(self, plan: SystemPlan, src: ModelSource, intervals_per_wave=None, tile_filter=None, shards=1):
        ib, db, lb = [], [], []

        def put(store, arr, dtype):
            arr = np.asarray(arr, dtype=dtype).ravel()
            off = sum(len(a) for a in store)
            store.append(arr)
            return off

        nP = len(plan.phase_plans)
        phases = np.zeros(nP, dtype=runtime.PHASE_DTYPE)
        kinds, tiles = [], []
        ipw = _intervals_per_wave(plan, intervals_per_wave, shards=shards, subs=getattr(src, "cycle_subs", 0))
        for k, pp in enumerate(plan.phase_plans):
            lay = pp.layout
            kind0 = len(kinds)
            for kd in lay.kinds:
                rec = np.zeros((), dtype=runtime.KIND_DTYPE)
                rec["K"], rec["R"], rec["nnzI"], rec["nnzT"] = kd.K, kd.R, kd.nnzI, kd.nnzT
                rec["irc_off"] = put(ib, np.stack([kd.I_r, kd.I_c], axis=1) if kd.nnzI else np.zeros((0, 2)), np.int32)
                rec["iv_off"] = put(db, kd.I_v, np.float64)
                rec["tv_off"] = put(db, kd.T_v, np.float64)
                rec["full_off"] = put(db, kd.full, np.float64)
                kinds.append(rec)
            tl = lay.tiles(ipw)
            if tile_filter is not None:
                tl = tile_filter(k, tl)
            ph = phases[k]
            ph["scheme"] = 0 if lay.scheme == "lgr" else 1
            ph["n_x"], ph["n_u"], ph["n_c"] = pp.nx, pp.nu, pp.phase.n_c
            ph["L_m"], ph["L_d"], ph["state_len"], ph["L"] = lay.L_m, lay.L_d, lay.state_len, lay.L
            ph["x_off"], ph["g_off"], ph["path_off"] = plan.l_p[k], plan.g_off[k], plan.path_off[k]
            ph["mid_lo"], ph["mid_hi"] = lay.mid_lo, lay.mid_hi
            ph["tile_lo"], ph["tile_hi"] = len(tiles), len(tiles) + len(tl)
            ph["tau_off"] = put(db, lay.tau, np.float64)
            ph["w_off"] = put(db, lay.w, np.float64)
            ph["width_off"] = put(db, lay.width, np.float64)
            ph["n_int"] = lay.N
            ph["ivK_off"] = put(ib, lay.K, np.int32)
            ph["ivld_off"] = put(ib, lay.ld, np.int32)
            full_pos = [int(kinds[kind0 + int(kf)]["full_off"]) for kf in lay.kid_full]
            ph["ivfull_off"] = put(ib, full_pos, np.int32)
            cbs = [("jac", "jseg_off"), ("hess", "hseg_off"), ("aux", "aseg_off")]
            if src.compact:
                cbs.append(("hessc", "hcseg_off"))
            if src.compact_j:
                cbs.append(("jacc", "jcseg_off"))
            for cbname, field in cbs:
                segs = getattr(plan, cbname).segs[k]
                bases = [s.base for s in segs if s.kind == "I"] + [s.base for s in segs if s.kind == "D"] + \
                        [s.base for s in segs if s.kind == "N"]
                ph[field] = put(lb, bases, np.int64)
            ph["jt_off"] = put(lb, plan.jac.tconst[k], np.int64)
            if src.compact_j:
                ph["jct_off"] = put(lb, plan.jacc.tconst[k], np.int64)
            red = [plan.l_p[k] + s if s >= 0 else plan.r_s + s for s in plan.grad_red_slots[k]]
            ph["red_off"] = put(ib, red, np.int32)
            def empty_tile():
                e = np.zeros((), dtype=runtime.TILE_DTYPE)
                e["phase"], e["K"] = k, 1
                return e

            for row in tl:
                j0, nj, kid, kidf, q0, r0, offI, offT = (int(v) for v in row)
                big = int(lay.K[j0]) > runtime.WAVE       # more points than a wave has lanes: the interval takes a whole
                while big and len(tiles) % runtime.WAVES_PER_BLOCK:       # workgroup (first slot of a tile block)
                    tiles.append(empty_tile())
                rec = np.zeros((), dtype=runtime.TILE_DTYPE)
                rec["phase"], rec["j0"], rec["nj"] = k, j0, nj
                rec["kid"], rec["kidf"] = kind0 + kid, kind0 + kidf
                rec["q0"], rec["r0"], rec["offI"], rec["offT"] = q0, r0, offI, offT
                rec["K"] = int(lay.K[j0])
                rec["last"] = 1 if j0 + nj == lay.N else 0
                for f in ("nnzI", "nnzT", "irc_off", "iv_off", "tv_off"):
                    rec[f] = kinds[kind0 + kid][f]
                rec["full_off"] = kinds[kind0 + kidf]["full_off"]
                R = int(kinds[kind0 + kidf]["R"])
                for field, d in (("magicI", int(rec["nnzI"])), ("magicR", R), ("magicT", int(rec["nnzT"]))):
                    rec[field] = magic_number(d)
                tiles.append(rec)
                if big:
                    tiles.extend(empty_tile() for _ in range(runtime.WAVES_PER_BLOCK - 1))
            while len(tiles) % runtime.WAVES_PER_BLOCK:      # a workgroup never mixes phases: pad with empty tiles
                rec = np.zeros((), dtype=runtime.TILE_DTYPE)
                rec["phase"], rec["K"] = k, 1
                tiles.append(rec)
            ph["tile_hi"] = len(tiles)
        # gradient slots no tile writes: state end slots (LGR), t0/tf, static parameters
        gz = []
        for k, pp in enumerate(plan.phase_plans):
            lay = pp.layout
            if lay.scheme == "lgr":
                gz += [plan.l_p[k] + lay.l_v[i] + lay.L_m for i in range(pp.nx)]
            gz += [plan.l_p[k] + lay.L - 2, plan.l_p[k] + lay.L - 1]
        gz += list(range(plan.l_s, plan.r_s))
        self.gz_off, self.n_gz = put(ib, gz, np.int32), len(gz)

        def items(cbname):
            cb = getattr(plan, cbname)
            off = src.list_off[cbname]
            arr = np.zeros(len(cb.items), dtype=runtime.ITEM_DTYPE)
            for i, it in enumerate(cb.items):
                arr[i] = (it.pos, it.coef, off[it.lst] + it.eid, it.lam)
            return arr

        self.items_jac, self.items_hess, self.items_aux = items("jac"), items("hess"), items("aux")
        self.items_hessc = items("hessc") if src.compact else np.zeros(0, dtype=runtime.ITEM_DTYPE)
        self.items_jacc = items("jacc") if src.compact_j else np.zeros(0, dtype=runtime.ITEM_DTYPE)
        self.outer = np.zeros(len(plan.outer), dtype=runtime.OUTER_DTYPE)
        for i, b in enumerate(plan.outer):
            flags = (1 if b.tril else 0) | (2 if b.collapseA else 0) | (4 if b.collapseB else 0) | (8 if b.second else 0)
            self.outer[i] = (b.pos, b.offA, b.lenA, b.offB, b.lenB, b.offM, flags, b.count, 0)
        self.phases = phases
        self.kinds = np.array(kinds, dtype=runtime.KIND_DTYPE) if kinds else np.zeros(0, runtime.KIND_DTYPE)
        self.tiles = np.array(tiles, dtype=runtime.TILE_DTYPE) if tiles else np.zeros(0, runtime.TILE_DTYPE)
        cat = lambda store, dt: np.concatenate(store).astype(dt) if store else np.zeros(0, dt)  # noqa: E731
        self.ib, self.db, self.lb = cat(ib, np.int32), cat(db, np.float64), cat(lb, np.int64)
        self.intervals_per_wave = ipw


def compile_plan(plan: SystemPlan, sharded=False, output_share=1.0, extra_flags=(), fixed=None):
    """Generated source + gfx950 code object of a plan.  The group size (codegen.split_groups: how many derivative entries a
    pass evaluates, stages and streams) is searched under two criteria, in this order:

    * **LDS** -- every launch of the code object must fit the 160 KiB of a workgroup *including* the table blocks the
      runtime adds (``ModelSource.launch_lds_bytes``, the bytes of ``csrc/pk_launch.h``): the size is halved
      until it does.  Nothing a wave stages grows with the number of states (WIDE phases, codegen.py), so a fitting size
      exists for every model; if none did, this raises instead of handing the library a model it must reject.
    * **registers** -- a model whose kernels would spill vector registers to scratch memory is generated again with smaller
      groups (every size down to 4, the fewest spilled registers win).  What is left is reported: ``ModelSource.spilling_kernels``
      and a ``RuntimeWarning`` (the kernels are correct, a spilling one is slow).

    Every size tried stays cached, so a model pays its extra compiles once.  Returns (ModelSource, code object)."""
    fast = plan.system._fastmath

    generated = {}

    def generate(cap, wide_nx=None):
        if (cap, wide_nx) not in generated:
            generated[(cap, wide_nx)] = ModelSource(plan, sharded=sharded, output_share=output_share, group_cap=cap, wide_nx=wide_nx)
        return generated[(cap, wide_nx)]

    def build(cap, src=None):
        src = src or generate(cap)
        code = hipbuild.compile_model(src.source, fastmath=fast, extra_flags=extra_flags)
        src.spilling_kernels = hipbuild.spills(hipbuild.resource_usage(src.source, fastmath=fast, extra_flags=extra_flags))
        return src, code, sum(v[0] for v in src.spilling_kernels.values())

    if fixed is not None:      # (Evaluator.checked's rebuild: the group size and wide threshold of the build it replaces, ONE compile
        best = build(int(fixed[0]), generate(int(fixed[0]), fixed[1]))      #  instead of the search -- with the flags of that rebuild
        return best[0], best[1]                                              #  the search took more than half an hour on a two-phase model)
    fixed_cap = bool(os.environ.get("POCKIT_AMD_GROUP_CAP"))
    cap0 = generate(None).group_cap
    while not fixed_cap and cap0 > 1 and not generate(cap0).fits_lds():
        cap0 //= 2
    if not generate(cap0).fits_lds():
        worst = max(generate(cap0).launch_lds_bytes().items(), key=lambda kv: kv[1])
        raise ValueError(f"the model does not fit a workgroup's LDS at any group size: {worst[0]} needs {worst[1]} bytes with "
                         f"groups of {cap0} (limit {ModelSource.LDS_LIMIT})")

    # A launch that underfills the chip (small and medium meshes: what the reference's example programs use) is as slow as
    # one wave's chain of evaluation, staging and streaming: groups of 16 instead of 32 split the roles of a moderately
    # large model into passes that run as workgroups of their own (humanoid 25 ... 500 x 8: 8.3 -> 7.3 ... 6.6 us per cycle);
    # with the chip full (humanoid 5000 x 8) the single pass is 4 % faster (profiles/r04_ze_*.txt).  The choice is a fact of
    # the mesh like PK_TAB_CAP: a refinement that crosses the line costs one more (cached) compile.
    free = not fixed_cap and os.environ.get("POCKIT_AMD_PASS_PARALLEL", "auto") == "auto"
    settled = None                    # (the underfill rule's choice: the group-size searches below are skipped, not the rest)
    if free and cap0 > ModelSource.GROUP_CAP // 2 and _launch_underfills_the_chip(plan, max(1, int(round(1.0 / output_share)))):
        probe = generate(ModelSource.GROUP_CAP // 2)
        if probe.grouped and probe.cycle_subs and probe.fits_lds():
            trial = build(probe.group_cap, probe)
            if trial[2] == 0:
                settled = trial
    best = settled or build(cap0)
    if settled is None and best[0].grouped and not fixed_cap:
        cap = best[0].group_cap      # (every size down to 4 while registers still spill: the count is not monotonic in the size.
        while best[2] > 0 and cap > 4:      # Some models keep spills at EVERY size -- DESIGN.md section 11 lists the measured ones)
            cap //= 2
            trial = build(cap)
            if trial[2] < best[2]:
                best = trial
    # The cycle of a model evaluated in groups is fastest with every pass as a workgroup of its own (ModelSource.cycle_subs,
    # DESIGN.md section 3c), which needs two workgroups of the launch on a CU: when the groups need too much LDS for that,
    # half the size is tried (rocket_powered_descent at 2000 x 4: 22.6 -> 11.3 us per cycle, drone_stabilization 15.2 -> 13.6;
    # profiles/r04_y_fat_pp_sweep.txt) -- unless it brings spills back.
    src = best[0]
    if free and src.grouped and not src.cycle_subs:
        cap = src.group_cap
        while cap > 8:
            cap //= 2
            probe = generate(cap)
            if not probe.cycle_subs:
                continue                     # (generated only: the rows of this size still leave no room for two workgroups)
            trial = build(cap, probe)
            if trial[2] <= best[2]:
                best = trial
            break
    # A pass-parallel model whose cycle kernel leaves room for ONE wave per SIMD runs its workgroups in two rounds (one
    # workgroup per CU at a time): the values workgroups of the second round publish their partial sums late and the launch
    # ends with the finalize workgroup (drone_stabilization at 2000 x 4: 480 workgroups, values waves entering up to 5.4 us
    # into a 13.3 us launch, profiles/r05_m_drone_wave_timeline.txt).  The register hog is the values role of a phase with
    # 9 ... 16 states (all states' node values, end slots and row sums at once: 250 VGPRs); evaluated the WIDE way -- chunks of
    # 8 states -- it needs far fewer.  Tried only there, kept only if it raises the occupancy without spills.
    src = best[0]
    if free and src.cycle_subs and best[2] == 0 and src.wide_nx == ModelSource.WIDE_NX and \
            any(ModelSource.WIDE_NX_LOW < pp.nx <= ModelSource.WIDE_NX for pp in plan.phase_plans):
        occ = lambda s_: ((hipbuild.resource_usage(s_.source, fastmath=fast, extra_flags=extra_flags) or {}).get("pk_cycle") or {}).get("occupancy", 0)  # noqa: E731
        if occ(src) == 1:
            probe = generate(src.group_cap, ModelSource.WIDE_NX_LOW)
            if probe.cycle_subs and probe.fits_lds():
                trial = build(src.group_cap, probe)
                if trial[2] == 0 and occ(trial[0]) > 1:
                    best = trial
    if best[2] > 0:
        import warnings

        warnings.warn("pockit_amd: kernels of this model spill vector registers to scratch memory at the best group size found "
                      f"({best[0].group_cap}): " + ", ".join(f"{k} {v[0]} VGPRs / {v[1]} B" for k, v in best[0].spilling_kernels.items()),
                      RuntimeWarning, stacklevel=2)
    return best[0], best[1]


def batched_source(plan, src, output_share=1.0):
    """The source of the BATCHED code object that goes with ``src`` (what ``compile_plan`` chose for the plan): the same model
    code -- group size, wide threshold, store policy -- with ``pk_cycleb`` as its only kernel."""
    return ModelSource(plan, output_share=output_share, group_cap=src.group_cap, wide_nx=src.wide_nx, batched=True)


def compile_batched(plan, src, output_share=1.0, extra_flags=()):
    """Code object of ``batched_source``; compiled and cached like any other the first time a batch is asked for."""
    return hipbuild.compile_model(batched_source(plan, src, output_share).source, fastmath=plan.system._fastmath, extra_flags=extra_flags)


# The refinement of the band solve (PK_BAND_REFINE_* of include/pockit_hip.h): the tolerance on the residual ratio, the ratio
# above which a system counts as singular for the solve that asked, the most steps of one refinement.
BAND_REFINE_TOL, BAND_REFINE_SINGULAR, BAND_REFINE_MAX_STEPS = 1.0e-10, 1.0e-5, 10


class Evaluator:
    #: the one build change with evidence behind it for the round-5 defect: SGPR spills to scratch memory
    SGPR_TO_SCRATCH = ("-mllvm", "-amdgpu-spill-sgpr-to-vgpr=0")

    @classmethod
    def checked(cls, plan: SystemPlan, **kw):
        """An evaluator whose FUSED kernel (pk_cycle: the x-callbacks and the one-launch cycle) has been verified against its
        own stand-alone kernels at a probe point (``self_check``).  Round 5 found code objects -- models wide in several
        directions, four cases, cause open -- whose fused kernel returned wrong f / grad / g while
        every stand-alone kernel was exact, with no error.  On a mismatch the model is built once more with the compiler's SGPR
        spills sent to scratch memory (the change that made every affected build tested exact) and checked again; if that
        fails too, this raises instead of handing out an evaluator that answers wrongly.  POCKIT_AMD_SELF_CHECK=0 skips it."""
        ev = cls(plan, **kw)
        if os.environ.get("POCKIT_AMD_SELF_CHECK", "1") == "0":
            return ev
        ok, worst = ev.self_check()
        if ok:
            return ev
        import warnings

        warnings.warn(f"pockit_amd: the fused kernel of this model's code object failed its self-check against the stand-alone "
                      f"kernels ({worst}); rebuilding with SGPR spills in scratch memory (DESIGN.md section 11)", RuntimeWarning, stacklevel=3)
        fixed = (ev.src.group_cap, ev.src.wide_nx)
        ev.close()
        ev = cls(plan, hipcc_flags=cls.SGPR_TO_SCRATCH, _fixed=fixed, **kw)
        ok, worst2 = ev.self_check()
        if ok:
            return ev
        # Both builds disagree with their own stand-alone kernels, which have been exact in every case seen: serve the model
        # through THEM (five launches per iterate instead of one -- what a model that needs the integrals first gets anyway).
        ev.close()
        ev = cls(plan, **kw)
        if ev.src.big:      # (a mesh with intervals of more than 64 points has the fused x-kernel only)
            ev.close()
            raise RuntimeError("pockit_amd: the fused kernel of this model's code object fails its self-check against the stand-alone "
                               f"kernels in both builds tried ({worst}; with SGPR spills in scratch memory: {worst2}) -- an open defect "
                               "(DESIGN.md section 11) -- and this mesh (an interval of more than 64 points) has no stand-alone "
                               "path.  No evaluator is handed out rather than one that answers wrongly")
        ev.ctx.check(ev.ctx.lib.pk_set_host_option(ev.ctx.handle, b"separate_x", 1))
        ev.separate_x = True
        warnings.warn(f"pockit_amd: both builds of this model fail the self-check of their fused kernel ({worst}; {worst2}): the "
                      "callbacks are served by the stand-alone kernels, one launch each (slower, exact in every case seen; DESIGN.md "
                      "section 11)", RuntimeWarning, stacklevel=3)
        return ev

    def self_check(self, tol=1.0e-9):
        """(ok, description of the worst disagreement).  One probe point -- x in [0.7, 1.3], lambda ~ N(0, 1), sigma 1 -- through
        the fused launch and through pk_int + pk_fin, pk_grad, pk_g, pk_jac, pk_hess; entries that are not finite must be so in
        both.  A consistency check, not a physical point.  (Meshes with intervals of more than 64 points and models that need
        the integrals first serve both sides from the same kernels: the check is vacuous there.)"""
        rng = np.random.default_rng(20240531)
        x = 0.7 + 0.6 * rng.uniform(size=self.plan.n)
        lam = rng.standard_normal(self.plan.m)
        with np.errstate(all="ignore"):
            fused = [np.array(v, dtype=np.float64, ndmin=1) for v in self.cycle(x, lam, 1.0)]
            alone = [np.array(v, dtype=np.float64, ndmin=1) for v in (self.objective_direct(x), self.gradient_direct(x), self.constraints_direct(x),
                                                                       self.jacobian_direct(x), self.hessian_direct(x, lam, 1.0))]
        self._invalidate_x()
        worst, ok = "", True
        for name, a, b in zip(("f", "grad f", "g", "J", "H"), fused, alone):
            fa, fb = np.isfinite(a), np.isfinite(b)
            if a.shape != b.shape or not np.array_equal(fa, fb):
                ok, worst = False, f"{name}: shapes / finite entries differ"
                break
            if fa.any():
                err = float(np.max(np.abs(a[fa] - b[fa]))) / max(1.0, float(np.max(np.abs(b[fb]))))
                if err > tol:
                    ok, worst = False, f"{name}: relative difference {err:.2e}"
                    break
        return ok, worst

    def __init__(self, plan: SystemPlan, device: int = 0, intervals_per_wave=None, tile_filter=None, sharded=False,
                 output_share=1.0, host_helpers=True, hipcc_flags=(), _fixed=None):
        self.plan = plan
        self.hipcc_flags = tuple(hipcc_flags)
        self.separate_x = False      # (True: Evaluator.checked switched this context to the stand-alone kernels)
        self._want_host_helpers = bool(host_helpers) and tile_filter is None
        self._output_share = float(output_share)
        self._batch_state = None     # None: not decided; "kernel": pk_cycleb loaded and verified; "loop": single cycles (see _ensure_batch)
        self._batch_bufs = (0, None)
        self._bounds = None          # what set_bounds was given (None: the plan's); _bounds_up: they are on the device
        self._bounds_up = False
        # (compiled before the context is created: a box without a GPU -- the build container -- can still fill the
        # code-object cache by constructing evaluators, tools/warm_cache.sh)
        self.src, code = compile_plan(plan, sharded=sharded, output_share=output_share, extra_flags=self.hipcc_flags, fixed=_fixed)
        self.ctx = runtime.Context(device)            # raises RuntimeError without a GPU
        lib, h = self.ctx.lib, self.ctx.handle
        md = model_desc(self.src)
        self._err_views = None
        self._csr = {}
        self._ops = {}               # operators uploaded to the context (pk_set_csr_operator): "J", "JT", "H"
        self._diag_pos = None        # positions of the diagonal of H uploaded to the context (pk_set_operator_diagonal)
        self._lin_gen = 0            # generation of the context's ONE linearization (Linearization handles compare with it)
        self._code = code
        self._views = {}
        self.zero_copy = False   # True: callbacks return views of pinned buffers (set by the IPOPT adapter)
        self.writable_results = os.environ.get("POCKIT_AMD_WRITABLE_RESULTS", "0") == "1"    # (see _result)
        if (md.prepass_grad or md.prepass_g or md.prepass_jac or md.prepass_hess) and self.src.big:
            # (integrals first AND an interval of more than 64 points: the x-callbacks then run pk_xall behind the prepass)
            self._refuse_sequential_values_role("a model that needs the integrals first, on a mesh with an interval of more than 64 points,")
        self.ctx.check(lib.pk_load_model(h, code, len(code), C.byref(md)))
        self.model_desc = md
        # (the tiling is sized for ONE shard's share of the mesh: output_share = 1 / number of shards)
        self.set_tables(Tables(plan, self.src, intervals_per_wave, tile_filter, shards=max(1, int(round(1.0 / output_share)))))

    def set_tables(self, tb: Tables):
        plan, lib, h = self.plan, self.ctx.lib, self.ctx.handle
        self.tables = tb
        self._views = {}
        self._csr, self._ops, self._diag_pos = {}, {}, None      # (pk_set_problem frees the maps and the operators of the context)
        self._bounds, self._bounds_up = None, False      # (... and the uploaded bounds of the merit terms)
        self._lin_gen += 1
        pd = runtime.ProblemDesc()
        pd.n, pd.m, pd.n_sys, pd.n_s, pd.l_s = plan.n, plan.m, plan.n_sys, plan.n_s, plan.l_s
        pd.n_phase, pd.n_tiles, pd.n_kinds = len(tb.phases), len(tb.tiles), len(tb.kinds)
        pd.nnz_J, pd.nnz_H = plan.nnz_J, plan.nnz_H
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        pd.phases, pd.tiles, pd.kinds = vp(tb.phases), vp(tb.tiles), vp(tb.kinds)
        pd.items_jac, pd.n_items_jac = vp(tb.items_jac), len(tb.items_jac)
        pd.items_hess, pd.n_items_hess = vp(tb.items_hess), len(tb.items_hess)
        pd.ib, pd.n_ib = tb.ib.ctypes.data_as(runtime.c_int32_p), len(tb.ib)
        pd.db, pd.n_db = tb.db.ctypes.data_as(runtime.c_double_p), len(tb.db)
        pd.lb, pd.n_lb = tb.lb.ctypes.data_as(C.POINTER(C.c_int64)), len(tb.lb)
        pd.gz_off, pd.n_gz = tb.gz_off, tb.n_gz
        pd.items_aux, pd.n_items_aux = vp(tb.items_aux), len(tb.items_aux)
        pd.outer, pd.n_outer, pd.n_aux = vp(tb.outer), len(tb.outer), plan.n_aux
        pd.items_hessc, pd.n_items_hessc = vp(tb.items_hessc), len(tb.items_hessc)
        pd.nnz_Hc = plan.nnz_Hc if self.src.compact else 0
        pd.items_jacc, pd.n_items_jacc = vp(tb.items_jacc), len(tb.items_jacc)
        pd.nnz_Jc = plan.nnz_Jc if self.src.compact_j else 0
        self._struct = [np.ascontiguousarray(a, dtype=np.int32) for a in
                        (plan.jac_row, plan.jac_col, plan.hess_row, plan.hess_col)]
        pd.jac_row, pd.jac_col, pd.hess_row, pd.hess_col = (a.ctypes.data_as(runtime.c_int32_p) for a in self._struct)
        self.ctx.check(lib.pk_set_problem(h, C.byref(pd)))
        # (pk_set_problem starts every problem in the reference layouts: what set_cycle_layout chose is applied again, so that
        #  a caller's compact-sized buffers never receive reference-layout writes after a change of tables)
        jc, hc = getattr(self, "_cycle_layout", (False, False))
        if jc or hc:
            self.set_cycle_layout(jc, hc)
        self._host_setup()

    def close(self):
        if self.ctx is not None:
            self._free_batch_buffers()
            self.ctx.close()
            self.ctx = None

    # ------------------------------------------------------------------ host-array callbacks
    def _x(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.plan.n,):
            raise ValueError(f"x must have shape ({self.plan.n},)")
        return x

    # IPOPT calls objective / gradient / constraints / jacobian one after the other on the same iterate and then
    # hessian with new multipliers (the five methods optimizer/ipopt.py hands to cyipopt; reference ipopt.py:41-53).
    # Every callback is ONE call into the library (pk_callback_x / pk_callback_hess): a bitwise compare decides whether x is
    # the prepared iterate; a new x is staged, uploaded, evaluated by the fused x-kernel and all of its results are on their
    # way to pinned host memory behind it; the callback then only waits for its own result.
    #
    # Where results land: ``zero_copy`` (set by the IPOPT adapter: cyipopt copies a result at once) hands out views of
    # the context's pinned buffers, valid until the next iterate.  Otherwise the callbacks return arrays the caller
    # owns, as the reference's do -- but over pinned memory the DMA writes directly (runtime.PinnedRing): J, grad f and g of
    # one iterate are three views of ONE block laid out like the device's buffer, [J | grad f | g], so that they arrive in a
    # single DMA; the x-independent entries of J (the translation part, ``SystemPlan.jac_constant_runs``) were put into the
    # block when it was allocated and never cross PCIe again.  A block is recycled only when the caller no longer refers
    # to any of its arrays.
    HEAD_RUN_MIN = 1024         # constant runs worth leaving out of the copy: at the head of J (the copy just starts later)
    INNER_RUN_MIN = 80_000      # ... and inside it (the copy splits in two: ~10 us per extra DMA = 0.5 MB of link time)

    def _host_setup(self):
        p = self.plan
        self._jac_compact = False
        self._nj = p.nnz_J          # Jacobian values of a landing block (the layout the Jacobian callback serves)
        self._blocks = runtime.PinnedRing(p.nnz_J + p.n + p.m)
        self._blocks_ref = self._blocks
        self._ring_h = runtime.PinnedRing(p.nnz_H)
        self._ring_hc = None
        self._next = self._cur = None
        self._cur_views, self._handed = {}, set()
        self._c_f, self._c_fresh = C.c_double(), C.c_int()
        self._a_f, self._a_fresh = C.addressof(self._c_f), C.addressof(self._c_fresh)
        self._const_runs = {}
        self.jac_constant_runs = self._register_constant_runs(False)
        # large systems: the solver thread's passes over x and lambda (a compare per callback, the staging copies) get helpers
        self.host_helper_threads = runtime.host_helpers(self.ctx.lib, p.n) if self._want_host_helpers else 0

    def _register_constant_runs(self, compact):
        """The x-independent runs of the Jacobian (in the layout the shim serves right now) worth leaving out of the copy."""
        if compact not in self._const_runs:
            runs = [(a, b) for a, b in self.plan.jac_constant_runs(compact)
                    if b - a >= (self.HEAD_RUN_MIN if a == 0 else self.INNER_RUN_MIN)]
            if runs:
                lo = (C.c_int64 * len(runs))(*[a for a, _ in runs])
                hi = (C.c_int64 * len(runs))(*[b for _, b in runs])
                self.ctx.check(self.ctx.lib.pk_set_jac_constant_runs(self.ctx.handle, len(runs), lo, hi))
            self._const_runs[compact] = runs
        return self._const_runs[compact]

    def set_jacobian_layout(self, compact):
        """The layout ``jacobian()`` and the J part of the landing blocks have: the reference's triplets or the compact
        layout (``plan.jacc_row/col``; an extra launch of pk_jacc behind the fused x-kernel, fewer values over PCIe)."""
        compact = bool(compact)
        if compact == self._jac_compact:
            return
        self.ctx.check(self.ctx.lib.pk_set_jacobian_layout(self.ctx.handle, int(compact)))
        p = self.plan
        self._jac_compact = compact
        self._nj = p.nnz_Jc if compact else p.nnz_J
        if compact:
            if getattr(self, "_blocks_compact", None) is None:
                self._blocks_compact = runtime.PinnedRing(p.nnz_Jc + p.n + p.m)
            self._blocks = self._blocks_compact
        else:
            self._blocks = self._blocks_ref
        self.jac_constant_runs = self._register_constant_runs(compact)
        self._next = self._cur = None
        self._cur_views, self._handed = {}, set()

    def _next_block(self):
        """The landing block [J | grad f | g] of the next new iterate (None: zero-copy mode, or the caller holds on to every
        block of the ring -- the results then land in the context's buffers and are copied)."""
        if self.zero_copy:
            return None
        it = self._next
        if it is None:
            it = self._blocks.take_item()
            if it is None:
                return None
            if not it.ready:
                if self.jac_constant_runs:
                    self.ctx.check(self.ctx.lib.pk_fill_jac_constants(self.ctx.handle, it.address))
                it.ready = True
            self._next = it
        return it

    def _became_current(self, it):
        """A new iterate was prepared; its x-results land in ``it`` (None: in the context's buffers)."""
        self._cur, self._next, self._handed = it, None, set()
        if it is None:
            self._cur_views = {}
        else:
            p, root, nj = self.plan, it.root, self._nj
            self._cur_views = {3: root[: nj], 1: root[nj: nj + p.n], 2: root[nj + p.n: nj + p.n + p.m]}

    def _callback_x(self, what, x):
        x = self._x(x)
        it = self._next_block()
        rc = self.ctx.lib.pk_callback_x(self.ctx.handle, what, x.ctypes.data, it.address if it is not None else None,
                                        self._a_f, self._a_fresh)
        if rc:
            self.ctx.check(rc)
        if self._c_fresh.value:
            self._became_current(it)

    def _invalidate_x(self):
        """The context's x / result buffers are about to be used by an entry point outside the prepared-x protocol."""
        self._lin_gen += 1      # (... and a Linearization handed out before is stale)
        if self.ctx is not None:
            self.ctx.lib.pk_invalidate_x(self.ctx.handle)

    def _pinned(self, what):
        """NumPy view of the context's pinned result buffer ``what`` (0 f, 1 grad, 2 g, 3 jac, 4 hess)."""
        if what not in self._views:
            ptr, cnt = runtime.c_double_p(), C.c_int64()
            self.ctx.check(self.ctx.lib.pk_host_buffer(self.ctx.handle, what, C.byref(ptr), C.byref(cnt)))
            self._views[what] = np.ctypeslib.as_array(ptr, shape=(max(cnt.value, 1),))[: cnt.value]
        return self._views[what]

    def _result(self, what, count):
        """The array result ``what`` of the current iterate landed in, as the callback's return value."""
        own = self._cur_views.get(what)
        if own is None:                      # landed in the context's buffer: zero-copy mode, or the ring is exhausted
            view = self._pinned(what)[:count]           # (the caller keeps many results): plain array + host copy
            return view if self.zero_copy else view.copy()
        if self.zero_copy:
            return own
        if what in self._handed:             # asked twice for the same iterate: the first array is the caller's
            return own.copy()
        self._handed.add(what)
        if what == 3 and self.jac_constant_runs:
            # The landing block keeps the x-independent entries of J (the +-1 translation part) from iterate to iterate: they
            # were filled in once and never cross PCIe again.  A caller that scaled this array in place would corrupt them for
            # every later Jacobian served from the block, so by default the array is handed out READ-ONLY (the reference
            # returns a fresh writable array; ``.copy()`` gives one).  ``writable_results = True`` (System.writable_results):
            # the array is writable and its block is marked to have the constant entries filled in again before it is
            # reused -- the reference's semantics at the price of one host pass over those entries per iterate.
            if self.writable_results:
                if self._cur is not None:
                    self._cur.ready = False
            else:
                own.flags.writeable = False
        return own

    def objective(self, x):
        self._callback_x(0, x)
        return np.float64(self._c_f.value)

    def gradient(self, x):
        self._callback_x(1, x)
        return self._result(1, self.plan.n)

    def constraints(self, x):
        self._callback_x(2, x)
        return self._result(2, self.plan.m)

    def jacobian(self, x):
        self._callback_x(3, x)
        return self._result(3, self._nj)

    def _lam(self, lagrange):
        lam = np.ascontiguousarray(lagrange, dtype=np.float64)
        if lam.shape != (self.plan.m,):
            raise ValueError(f"lagrange must have shape ({self.plan.m},)")
        return lam

    def _callback_hess(self, x, lam, obj_factor, target, compact):
        x = self._x(x)
        it = self._next_block()
        rc = self.ctx.lib.pk_callback_hess(self.ctx.handle, x.ctypes.data, lam.ctypes.data, float(obj_factor),
                                           it.address if it is not None else None, target, compact, self._a_fresh)
        if rc:
            self.ctx.check(rc)
        if self._c_fresh.value:
            self._became_current(it)

    def hessian(self, x, lagrange, obj_factor):
        lam = self._lam(lagrange)
        hit = None if self.zero_copy else self._ring_h.take_item()
        self._callback_hess(x, lam, obj_factor, hit.address if hit is not None else None, 0)
        if hit is None:                      # the context's buffer: zero-copy mode, or the caller keeps every Hessian
            view = self._pinned(4)[: self.plan.nnz_H]
            return view if self.zero_copy else view.copy()
        return hit.array

    def set_host_mode(self, prefetch=True, host_direct=False):
        """``prefetch`` (default True): all four x-results are copied to the host right behind the kernel; False: f and
        g always, grad f and J when first asked for.  ``host_direct``: the kernels store into pinned host memory
        themselves instead of device memory + DMA (A/B switch)."""
        self.ctx.check(self.ctx.lib.pk_set_host_mode(self.ctx.handle, int(bool(prefetch)), int(bool(host_direct))))

    # one-shot variants without the x cache (each uploads x and runs only its own kernels)
    def objective_direct(self, x):
        x = self._x(x)
        self._invalidate_x()        # the context's x / result buffers are about to hold another iterate
        out = np.empty(1)
        self.ctx.check(self.ctx.lib.pk_eval_f(self.ctx.handle, runtime.as_dp(x), runtime.as_dp(out)))
        return np.float64(out[0])

    def gradient_direct(self, x):
        x = self._x(x)
        self._invalidate_x()        # the context's x / result buffers are about to hold another iterate
        out = np.empty(self.plan.n)
        self.ctx.check(self.ctx.lib.pk_eval_grad(self.ctx.handle, runtime.as_dp(x), runtime.as_dp(out)))
        return out

    def constraints_direct(self, x):
        x = self._x(x)
        self._invalidate_x()        # the context's x / result buffers are about to hold another iterate
        out = np.empty(self.plan.m)
        self.ctx.check(self.ctx.lib.pk_eval_g(self.ctx.handle, runtime.as_dp(x), runtime.as_dp(out)))
        return out

    def jacobian_direct(self, x):
        x = self._x(x)
        self._invalidate_x()        # the context's x / result buffers are about to hold another iterate
        out = np.empty(self.plan.nnz_J)
        self.ctx.check(self.ctx.lib.pk_eval_jac(self.ctx.handle, runtime.as_dp(x), runtime.as_dp(out)))
        return out

    def hessian_direct(self, x, lagrange, obj_factor):
        x = self._x(x)
        self._invalidate_x()        # the context's x / result buffers are about to hold another iterate
        lam = np.ascontiguousarray(lagrange, dtype=np.float64)
        out = np.empty(self.plan.nnz_H)
        self.ctx.check(self.ctx.lib.pk_eval_hess(self.ctx.handle, runtime.as_dp(x), runtime.as_dp(lam),
                                                 float(obj_factor), runtime.as_dp(out)))
        return out

    def hessian_compact(self, x, lagrange, obj_factor):
        """Values of the compact (coalesced) Hessian layout ``plan.hessc_row/col``."""
        if not self.src.compact:
            raise NotImplementedError("compact Hessian layout is not available for this model")
        lam = self._lam(lagrange)
        # the prepared-x protocol, like hessian(): the x of the iterate is already on the device (objective ... jacobian ran
        # on it), the values come back by DMA into a pinned array of the caller's
        if self._ring_hc is None:
            self._ring_hc = runtime.PinnedRing(self.plan.nnz_Hc)
        hit = self._ring_hc.take_item()
        if hit is not None:
            self._callback_hess(x, lam, obj_factor, hit.address, 1)
            return hit.array
        # (the caller keeps every array of the ring: a plain array, filled through the context's pinned buffer)
        lib, h = self.ctx.lib, self.ctx.handle
        self._callback_x(2, x)
        out = np.empty(self.plan.nnz_Hc)
        self.ctx.check(lib.pk_eval_hessc_prepared(h, runtime.as_dp(lam), float(obj_factor), runtime.as_dp(out), 0))
        return out

    def jacobian_compact(self, x):
        """Values of the compact (coalesced) Jacobian layout ``plan.jacc_row/col`` (one pk_jacc launch; the one-shot entry
        point -- a solver loop uses ``set_jacobian_layout(True)`` and ``jacobian()``)."""
        x = self._x(x)
        self._invalidate_x()        # the context's x buffer is about to hold another iterate
        out = np.empty(self.plan.nnz_Jc)
        self.ctx.check(self.ctx.lib.pk_eval_jacc(self.ctx.handle, runtime.as_dp(x), runtime.as_dp(out)))
        return out

    def mesh_error(self, x):
        """Mesh error estimation data of every phase at the NLP point ``x`` (one pk_err launch): a list of
        ``(T, I)`` with shape (n_x, rows) each -- the two sides of the collocation equation on every interval
        re-collocated with one more point (reference: phasebase.py:1339-1372)."""
        from . import refine

        lib, h = self.ctx.lib, self.ctx.handle
        if self._err_views is None:
            recs, tables, n_out, views, groups = refine.error_tables(self.plan)
            self.ctx.check(lib.pk_set_mesh_error_tables(h, recs.ctypes.data, len(recs), groups.ctypes.data, len(groups),
                                                        runtime.as_dp(tables),
                                                        len(tables), n_out))
            self._err_views, self._err_len = views, n_out
        x = self._x(x)
        self._invalidate_x()        # the context's x / result buffers are about to hold another iterate
        T, I = np.empty(self._err_len), np.empty(self._err_len)
        self.ctx.check(lib.pk_eval_mesh_error(h, runtime.as_dp(x), runtime.as_dp(T), runtime.as_dp(I)))
        return [(T[o: o + nx * rows].reshape(nx, rows), I[o: o + nx * rows].reshape(nx, rows))
                for o, nx, rows in self._err_views]

    # ------------------------------------------------------------------ device-resident CSR hand-off
    def csr_map(self, which):
        """``CsrMap`` of the Jacobian (``"jac"``) or of the lower triangle of the Hessian of the Lagrangian
        (``"hess"``, reference layout); built and uploaded on first use."""
        from .csr import CsrMap

        if which not in ("jac", "hess"):
            raise ValueError('which must be "jac" or "hess"')
        if which not in self._csr:
            plan = self.plan
            if which == "jac":
                m = CsrMap(plan.jac_row, plan.jac_col, (plan.m, plan.n))
            else:
                m = CsrMap(plan.hess_row, plan.hess_col, (plan.n, plan.n))
            seg = None if m.seg is None else m.seg.ctypes.data_as(runtime.c_int32_p)
            self._ops, self._diag_pos = {}, None      # pk_set_csr_map drops the context's operators and its linearization
            self._lin_gen += 1
            self.ctx.check(self.ctx.lib.pk_set_csr_map(self.ctx.handle, 0 if which == "jac" else 1, seg,
                                                       m.perm.ctypes.data_as(runtime.c_int32_p), m.nnz, m.n_triplets))
            self._csr[which] = m
            if which == "jac" and self.src.compact_j:
                # the CSR values of J from the compact evaluation: its few repeated positions are summed by the gather
                plan.jacc  # noqa: B018  (builds the compact plan)
                mc = CsrMap(plan.jacc_row, plan.jacc_col, (plan.m, plan.n))
                if mc.n_triplets < m.n_triplets and mc.nnz == m.nnz and np.array_equal(mc.indices, m.indices) \
                        and np.array_equal(mc.indptr, m.indptr):      # (only where the compact layout writes fewer values)
                    segc = None if mc.seg is None else mc.seg.ctypes.data_as(runtime.c_int32_p)
                    self.ctx.check(self.ctx.lib.pk_set_csr_map(self.ctx.handle, 3, segc,
                                                               mc.perm.ctypes.data_as(runtime.c_int32_p), mc.nnz, mc.n_triplets))
                    self._csr["jacc"] = mc
            if which == "hess" and self.src.compact:
                # the compact Hessian has one value per distinct (row, col): if its pattern is the full pattern's set of
                # entries, the CSR values are a permutation of it (pk_eval_hess_csr then never writes the repeats)
                mc = CsrMap(plan.hessc_row, plan.hessc_col, (plan.n, plan.n))
                if mc.seg is None and mc.nnz == m.nnz and np.array_equal(mc.indices, m.indices) \
                        and np.array_equal(mc.indptr, m.indptr):
                    self.ctx.check(self.ctx.lib.pk_set_csr_map(self.ctx.handle, 2, None,
                                                               mc.perm.ctypes.data_as(runtime.c_int32_p), mc.nnz, mc.n_triplets))
                    self._csr["hessc"] = mc
        return self._csr[which]

    def jacobian_csr(self, x):
        """CSR values of the constraint Jacobian (structure: ``csr_map("jac")``), gathered on the device."""
        m = self.csr_map("jac")
        x = self._x(x)
        self._invalidate_x()        # the context's x / result buffers are about to hold another iterate
        out = np.empty(m.nnz)
        self.ctx.check(self.ctx.lib.pk_eval_jac_csr(self.ctx.handle, runtime.as_dp(x), runtime.as_dp(out)))
        return out

    def hessian_csr(self, x, lagrange, obj_factor):
        """CSR values of the lower triangle of the Hessian of the Lagrangian (``csr_map("hess")``)."""
        m = self.csr_map("hess")
        x = self._x(x)
        self._invalidate_x()        # the context's x / result buffers are about to hold another iterate
        lam = np.ascontiguousarray(lagrange, dtype=np.float64)
        out = np.empty(m.nnz)
        self.ctx.check(self.ctx.lib.pk_eval_hess_csr(self.ctx.handle, runtime.as_dp(x), runtime.as_dp(lam),
                                                     float(obj_factor), runtime.as_dp(out)))
        return out

    def jacobian_csr_dev(self, d_x, d_out, stream=None):
        self.csr_map("jac")
        self._invalidate_x()        # (the triplets pass through the context's J buffer)
        self.ctx.check(self.ctx.lib.pk_eval_jac_csr_dev(self.ctx.handle, d_x, d_out, stream))

    def hessian_csr_dev(self, d_x, d_lam, sigma, d_out, stream=None):
        self.csr_map("hess")
        self._invalidate_x()
        self.ctx.check(self.ctx.lib.pk_eval_hess_csr_dev(self.ctx.handle, d_x, d_lam, float(sigma), d_out, stream))

    def gather_csr_dev(self, which, d_triplets, d_out, stream=None):
        """Triplet values already on the device (e.g. from ``cycle_dev``) -> CSR values."""
        self.csr_map(which)
        self.ctx.check(self.ctx.lib.pk_gather_csr_dev(self.ctx.handle, 0 if which == "jac" else 1, d_triplets, d_out,
                                                      stream))

    # ------------------------------------------------------------------ J, J^T and H applied to vectors on the device
    OPERATORS = {"J": 0, "JT": 1, "H": 2}

    def _operator(self, op):
        """Number of the operator ``op`` for the C ABI; its structure (csr.CsrOperator, from the maps) is built and uploaded
        on first use, like ``csr_map``."""
        if op not in self.OPERATORS:
            raise ValueError('op must be "J", "JT" or "H"')
        if self.src.sharded:
            raise NotImplementedError("the device-side operators are not offered for a sharded evaluator")
        m = self.csr_map("hess" if op == "H" else "jac")      # (first: a new map drops the operators)
        if op not in self._ops:
            o = m.operator() if op == "J" else m.transposed() if op == "JT" else m.symmetric()
            i32 = lambda a: None if a is None else a.ctypes.data_as(runtime.c_int32_p)  # noqa: E731
            self.ctx.check(self.ctx.lib.pk_set_csr_operator(self.ctx.handle, self.OPERATORS[op], i32(o.indptr), i32(o.indices),
                                                            i32(o.src), o.shape[0], o.shape[1], o.nnz))
            self._ops[op] = o
        return self.OPERATORS[op]

    def apply_operator_dev(self, op, d_vals, d_v, d_y, d_add=None, stream=None):
        """``y = A(vals) v (+ add)`` on device pointers, ``op`` one of "J", "JT", "H"; ``d_vals``: a CSR value array as
        ``jacobian_csr_dev`` / ``hessian_csr_dev`` / ``gather_csr_dev`` fill it.  ``d_add`` may alias ``d_y``.  Enqueued on
        ``stream``, not waited for."""
        k = self._operator(op)
        self.ctx.check(self.ctx.lib.pk_apply_operator_dev(self.ctx.handle, k, d_vals, d_v, d_add, d_y, stream))

    def apply_operator_block_dev(self, op, d_vals, k, d_V, d_Y, ldv=None, ldy=None, d_add=None, stream=None):
        """``Y = A(vals) V (+ Add)`` on device pointers for a block of ``k`` vectors, row-major: ``V[i * ldv + j]``,
        ``Y[r * ldy + j]`` (and ``Add`` like ``Y``), ``ldv`` / ``ldy`` defaulting to ``k`` -- the C order of an ``(n, k)``
        tensor.  Only the first ``k`` entries of a row of ``Y`` are written.  Column ``j`` has the bits ``apply_operator_dev``
        gives for column ``j`` alone.  ``d_add`` may alias ``d_Y``.  Enqueued on ``stream``, not waited for."""
        num = self._operator(op)
        k = int(k)
        self.ctx.check(self.ctx.lib.pk_apply_operator_block_dev(self.ctx.handle, num, d_vals, k, d_V, k if ldv is None else int(ldv),
                                                                d_add, d_Y, k if ldy is None else int(ldy), stream))

    REDUCE_MODES = {"abs_sum": 0, "sq_sum": 1, "abs_max": 2}

    def _reduce_mode(self, mode):
        if mode not in self.REDUCE_MODES:
            raise ValueError('mode must be "abs_sum", "sq_sum" or "abs_max"')
        return self.REDUCE_MODES[mode]

    def _operator_diagonal(self):
        """The positions of the diagonal of H in the Hessian map's values (csr.CsrMap.diagonal_src), uploaded on first use
        like an operator and dropped with the operators."""
        if self.src.sharded:
            raise NotImplementedError("the device-side operators are not offered for a sharded evaluator")
        m = self.csr_map("hess")      # (first: a new map drops the operators and the positions)
        if self._diag_pos is None:
            pos = m.diagonal_src()
            self.ctx.check(self.ctx.lib.pk_set_operator_diagonal(self.ctx.handle, self.OPERATORS["H"],
                                                                 pos.ctypes.data_as(runtime.c_int32_p), len(pos)))
            self._diag_pos = pos
        return self.OPERATORS["H"]

    def operator_reduce_dev(self, op, mode, d_vals, d_y, d_w=None, d_add=None, stream=None):
        """A reduction over the rows of ``op`` ("J", "JT", "H") on device pointers, ``mode`` one of "abs_sum"
        (``y[r] = sum_e |a_e| w[c_e]``), "sq_sum" (``sum_e (a_e a_e) w[c_e]``) and "abs_max" (``max(0, max_e |a_e| w[c_e])``);
        ``d_w`` (one weight per column) may be None: no weight.  ``d_add`` (added to the sums, a further candidate of the
        maximum) may alias ``d_y``.  The association is that of ``apply_operator_dev``; enqueued on ``stream``, not waited for."""
        k = self._operator(op)
        self.ctx.check(self.ctx.lib.pk_operator_reduce_dev(self.ctx.handle, k, self._reduce_mode(mode), d_vals, d_w, d_add, d_y, stream))

    def operator_diagonal_dev(self, op, d_vals, d_y, d_add=None, stream=None):
        """``y = diag(H(vals)) (+ add)`` on device pointers; ``op`` must be "H", ``d_vals`` a CSR value array of the Hessian map.
        ``d_add`` may alias ``d_y``.  Enqueued on ``stream``, not waited for."""
        if op not in self.OPERATORS:
            raise ValueError('op must be "J", "JT" or "H"')
        if op != "H":
            raise ValueError('only "H" is square: J and JT have no diagonal')
        self.ctx.check(self.ctx.lib.pk_operator_diagonal_dev(self.ctx.handle, self._operator_diagonal(), d_vals, d_add, d_y, stream))

    # ------------------------------------------------------------------ the condensed KKT matrix / the normal equations (csrc/pk_cg.cpp)
    FORMS = {"primal": 0, "dual": 1}

    def _condensed(self, form, with_h):
        """Number of ``form`` for the C ABI, with the operators (and the map of H) it needs uploaded."""
        if form not in self.FORMS:
            raise ValueError('form must be "primal" or "dual"')
        if self.src.sharded:
            raise NotImplementedError("the condensed operator and its CG solve are not offered for a sharded evaluator")
        if with_h and form == "dual":
            raise ValueError("the dual form has no Hessian term")
        for op in ("J", "JT") + (("H",) if with_h else ()):
            self._operator(op)
        return self.FORMS[form]

    def condensed_apply_dev(self, form, d_jvals, d_v, d_y, d_hvals=None, d_d=None, d_s=None, stream=None):
        """``y = K v`` on device pointers: ``form`` "primal" (``[H v] + J^T (d o (J v)) + s o v``, size n) or "dual"
        (``J (d o (J^T v)) + s o v``, size m); ``d_hvals``, ``d_d`` and ``d_s`` may be None.  Enqueued, not waited for."""
        k = self._condensed(form, d_hvals is not None)
        self.ctx.check(self.ctx.lib.pk_condensed_apply_dev(self.ctx.handle, k, d_jvals, d_hvals, d_d, d_s, d_v, d_y, stream))

    def cg_begin_dev(self, form, d_jvals, d_b, d_x, tol, d_hvals=None, d_d=None, d_s=None, d_minv=None, d_x0=None, stream=None):
        """Begin a preconditioned CG solve of ``K x = b`` on device pointers (``pk_cg_begin_dev``): the arrays stay the
        caller's and must stay valid until the solve ends.  Enqueued, not waited for."""
        k = self._condensed(form, d_hvals is not None)
        self.ctx.check(self.ctx.lib.pk_cg_begin_dev(self.ctx.handle, k, d_jvals, d_hvals, d_d, d_s, d_minv, d_b, d_x0, d_x, float(tol),
                                                    stream))

    def cg_advance_dev(self, iters, stream=None):
        """Enqueue ``iters`` iterations of the solve in progress, without a synchronisation."""
        self.ctx.check(self.ctx.lib.pk_cg_advance_dev(self.ctx.handle, int(iters), stream))

    def cg_record(self):
        """The record of the solve in progress (8 doubles: status, iterations, rr, thr, rz, pq, alpha, beta), waited for."""
        rec = np.empty(8)
        self.ctx.check(self.ctx.lib.pk_cg_record(self.ctx.handle, runtime.as_dp(rec)))
        return rec

    # ------------------------------------------------------------------ the augmented KKT system (csrc/pk_minres.cpp)
    def _kkt(self, with_h):
        """The operators (and the map of H) the augmented system needs, uploaded."""
        if self.src.sharded:
            raise NotImplementedError("the augmented KKT operator and its MINRES solve are not offered for a sharded evaluator")
        for op in ("J", "JT") + (("H",) if with_h else ()):
            self._operator(op)

    def kkt_apply_dev(self, d_jvals, d_v, d_y, d_hvals=None, d_s1=None, d_s2=None, stream=None):
        """``y = K v`` on device pointers, ``K = [[H + diag(s1), J^T], [J, -diag(s2)]]`` of size n + m, vectors
        ``[primal | dual]``; ``d_hvals``, ``d_s1`` and ``d_s2`` may be None.  Enqueued, not waited for."""
        self._kkt(d_hvals is not None)
        self.ctx.check(self.ctx.lib.pk_kkt_apply_dev(self.ctx.handle, d_jvals, d_hvals, d_s1, d_s2, d_v, d_y, stream))

    def minres_begin_dev(self, d_jvals, d_b, d_x, tol, d_hvals=None, d_s1=None, d_s2=None, d_minv=None, d_x0=None, stream=None):
        """Begin a preconditioned MINRES solve of ``K x = b`` on device pointers (``pk_minres_begin_dev``): the arrays stay the
        caller's and must stay valid until the solve ends.  Enqueued, not waited for."""
        self._kkt(d_hvals is not None)
        self.ctx.check(self.ctx.lib.pk_minres_begin_dev(self.ctx.handle, d_jvals, d_hvals, d_s1, d_s2, d_minv, d_b, d_x0, d_x,
                                                        float(tol), stream))

    def minres_advance_dev(self, iters, stream=None):
        """Enqueue ``iters`` iterations of the MINRES solve in progress, without a synchronisation."""
        self.ctx.check(self.ctx.lib.pk_minres_advance_dev(self.ctx.handle, int(iters), stream))

    def minres_record(self):
        """The record of the MINRES solve in progress (16 doubles: status, iterations, phibar, thr, beta, oldb, alfa, dbar,
        epsln, cs, sn, phi, oldeps, delta, gamma, 0), waited for."""
        rec = np.empty(16)
        self.ctx.check(self.ctx.lib.pk_minres_record(self.ctx.handle, runtime.as_dp(rec)))
        return rec

    def linearize(self, x, lagrange=None, obj_factor=1.0):
        """Evaluate J at ``x`` -- and the Hessian of the Lagrangian with ``(lagrange, obj_factor)`` unless ``lagrange`` is
        None -- into the context's CSR value arrays and leave them on the device: the ``Linearization`` returned multiplies
        with them, one vector each way per product.  A context holds ONE linearization: the handle is stale after the next
        ``linearize`` and after any call that gives the context's buffers another evaluation (``jacobian_csr``, ``cycle``, the
        ``*_direct`` and ``*_dev`` entry points ...); the callbacks of the prepared-x protocol leave it alone."""
        x = self._x(x)
        lam = None if lagrange is None else self._lam(lagrange)
        self.csr_map("jac")         # (both maps before any operator: a new map drops the operators)
        if lam is not None:
            self.csr_map("hess")
        for op in ("J", "JT") + (("H",) if lam is not None else ()):
            self._operator(op)
        self._invalidate_x()        # the context's x buffer is about to hold another iterate; earlier handles are stale
        self.ctx.check(self.ctx.lib.pk_linearize(self.ctx.handle, runtime.as_dp(x), None if lam is None else runtime.as_dp(lam),
                                                 float(obj_factor)))
        return Linearization(self, self._lin_gen, lam is not None)

    def cycle(self, x, lagrange, obj_factor):
        """All five outputs on the same x from ONE call and ONE launch (pk_cycle): returns (f, grad, g, J, H).  Staging and
        landing are the callbacks' (pk_callback_cycle): x and lambda through the pinned staging buffers, [J | grad f | g] into a
        landing block whose x-independent entries are already there, H into a pinned array of the Hessian ring.  Afterwards
        the iterate is the prepared one: the callbacks on the same x are served from what has landed."""
        x = self._x(x)
        lam = self._lam(lagrange)
        p = self.plan
        it = None if self._jac_compact else self._next_block()      # (the one-launch cycle writes the reference layout)
        hit = None if self.zero_copy else self._ring_h.take_item()
        if it is not None and hit is not None:
            rc = self.ctx.lib.pk_callback_cycle(self.ctx.handle, x.ctypes.data, lam.ctypes.data, float(obj_factor), it.address,
                                                hit.address, self._a_f)
            if rc:
                self.ctx.check(rc)
            self._became_current(it)
            v = self._cur_views
            self._handed = {1, 2, 3}
            return np.float64(self._c_f.value), v[1], v[2], v[3], hit.array
        # no landing block to be had (zero-copy mode, the caller holds on to every block, compact Jacobian layout): plain
        # arrays, one copy per output
        self._invalidate_x()        # the context's x / result buffers are about to hold another iterate
        J, grad, g, H = np.empty(p.nnz_J), np.empty(p.n), np.empty(p.m), np.empty(p.nnz_H)
        f = np.empty(1)
        dp = runtime.as_dp
        self.ctx.check(self.ctx.lib.pk_eval_cycle(self.ctx.handle, dp(x), dp(lam), float(obj_factor), dp(f), dp(grad),
                                                  dp(g), dp(J), dp(H)))
        return np.float64(f[0]), grad, g, J, H

    # ------------------------------------------------------------------ device-pointer API
    def cycle_dev(self, d_x, d_lam, sigma, d_f, d_grad, d_g, d_jac, d_hess, stream=None):
        """Enqueue one full callback cycle on device pointers (ints); no synchronization."""
        self.ctx.check(self.ctx.lib.pk_eval_cycle_dev(self.ctx.handle, d_x, d_lam, float(sigma), d_f, d_grad, d_g,
                                                      d_jac, d_hess, stream))

    def sync(self, stream=None):
        self.ctx.check(self.ctx.lib.pk_sync(self.ctx.handle, stream))

    # ------------------------------------------------------------------ a batch of iterates per launch (pk_cycleb)
    def batched_source(self):
        """The source of this model's batched code object: the model code of ``self.src``, ``pk_cycleb`` its only kernel."""
        return batched_source(self.plan, self.src, self._output_share)

    def _one_launch_cycle(self):
        """Is this context's cycle the one-launch cycle (what a batch can be one launch of)?"""
        md = self.model_desc
        return not (md.prepass_grad or md.prepass_g or md.prepass_jac or md.prepass_hess or self.separate_x or self.src.sharded)

    def _ensure_batch(self):
        """First batch of this evaluator: compile (or fetch) and load the batched code object, then hold it against this
        context's own single launches.  The batched object is a new build of the fused kernel, so the set-up check of
        ``pk_cycle`` (``Evaluator.checked``) says nothing about it: a batch of two -- the self-check's
        probe point and a second point -- must agree BIT FOR BIT with two single cycles, and the x-only batch of the same points
        with the single x-only path.  On any difference the object is dropped: batches are then served by the library's loop of
        single cycles (the same values, no gain) and a ``RuntimeWarning`` names the model.  ``POCKIT_AMD_SELF_CHECK=0`` skips the
        check (the object is used unchecked).  Models whose cycle is not the one-launch cycle take the loop from the start."""
        if self._batch_state is not None:
            return self._batch_state
        if not self._one_launch_cycle():
            self._batch_state = "loop"
            return self._batch_state
        lib, h = self.ctx.lib, self.ctx.handle
        code = compile_batched(self.plan, self.src, self._output_share, self.hipcc_flags)
        self.ctx.check(lib.pk_load_batch_model(h, code, len(code)))
        self._batch_state = "kernel"
        if os.environ.get("POCKIT_AMD_SELF_CHECK", "1") == "0":
            return self._batch_state
        rng = np.random.default_rng(20240531)                      # (entry 0: self_check's x and lambda, drawn in its order)
        X, Lam = np.empty((2, self.plan.n)), np.empty((2, self.plan.m))
        for e in range(2):
            X[e] = 0.7 + 0.6 * rng.uniform(size=self.plan.n)
            Lam[e] = rng.standard_normal(self.plan.m)
        sig = np.array([1.0, 0.75])
        names = ("f", "grad f", "g", "J", "H")
        same = lambda a, b: np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint64),  # noqa: E731
                                           np.ascontiguousarray(b, dtype=np.float64).reshape(-1).view(np.uint64))
        worst = ""
        try:
            with np.errstate(all="ignore"):
                got = self._cycle_batch_chunk(X, Lam, sig)
                got_x = self._cycle_batch_chunk(X, None, sig)      # (the x-only records: no Hessian role)
                for e in range(2):
                    want = self._cycle_plain(X[e], Lam[e], sig[e])
                    for name, a, b in zip(names, got, want):
                        if not same(a[e], b):
                            worst = worst or f"{name} of entry {e}"
                    self._invalidate_x()
                    x = X[e].copy()      # (the single x-only path: what the first callback on a new x launches)
                    want_x = (self.objective(x), self.gradient(x), self.constraints(x), self.jacobian(x))
                    for name, a, b in zip(names, got_x, want_x):
                        if not same(a[e], b):
                            worst = worst or f"{name} of entry {e} of the x-only batch"
        finally:
            self._invalidate_x()
            self._free_batch_buffers()
        if worst:
            import warnings

            self.ctx.check(lib.pk_load_batch_model(h, None, 0))
            self._batch_state = "loop"
            p = self.plan
            warnings.warn(f"pockit_amd: the batched kernel (pk_cycleb) of model {self.src.hash} ({len(p.phase_plans)} phases, n = {p.n}, "
                          f"m = {p.m}) differs from the single-launch cycle of the same context ({worst}): its code object is dropped, "
                          "batches are served by a loop of single cycles (DESIGN.md sections 11 and 14)", RuntimeWarning, stacklevel=3)
        return self._batch_state

    def _cycle_plain(self, x, lam, sigma):
        """One cycle through pk_eval_cycle into plain arrays: (f (1,), grad, g, J, H)."""
        p, dp = self.plan, runtime.as_dp
        x, lam = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(lam, dtype=np.float64)
        f, grad, g, J, H = np.empty(1), np.empty(p.n), np.empty(p.m), np.empty(p.nnz_J), np.empty(p.nnz_H)
        self.ctx.check(self.ctx.lib.pk_eval_cycle(self.ctx.handle, dp(x), dp(lam), float(sigma), dp(f), dp(grad), dp(g), dp(J), dp(H)))
        return f, grad, g, J, H

    def _free_batch_buffers(self):
        cap, bufs = self._batch_bufs
        if bufs and self.ctx is not None and self.ctx.handle:
            for ptr in bufs.values():
                self.ctx.lib.pk_device_free(self.ctx.handle, ptr)
        self._batch_bufs = (0, None)

    def _batch_buffers(self, B):
        """Device arrays [B][...] of the host-array form: x, lambda and the five outputs -- kept from chunk to chunk of one
        ``cycle_batch``, freed before it returns (64 entries of a large model are of the order of a gigabyte)."""
        cap, bufs = self._batch_bufs
        if bufs is not None and B <= cap:
            return bufs
        self._free_batch_buffers()
        p, bufs = self.plan, {}
        for name, count in (("x", p.n), ("lam", p.m), ("f", 1), ("grad", p.n), ("g", p.m), ("jac", p.nnz_J), ("hess", p.nnz_H)):
            ptr = C.c_void_p()
            self.ctx.check(self.ctx.lib.pk_device_alloc(self.ctx.handle, 8 * B * max(int(count), 1), 0, C.byref(ptr)))
            bufs[name] = ptr.value
        self._batch_bufs = (B, bufs)
        return bufs

    def _cycle_batch_chunk(self, X, Lam, sig):
        """At most MAX_BATCH iterates: upload, ONE call of the library, download, wait."""
        p, lib, h = self.plan, self.ctx.lib, self.ctx.handle
        B = len(X)
        d = self._batch_buffers(B)
        self.ctx.check(lib.pk_copy_dev(h, d["x"], X.ctypes.data, X.nbytes, None))
        if Lam is not None:
            self.ctx.check(lib.pk_copy_dev(h, d["lam"], Lam.ctypes.data, Lam.nbytes, None))
        self.ctx.check(lib.pk_eval_cycle_batch_dev(h, B, d["x"], p.n, d["lam"] if Lam is not None else None, p.m,
                                                   runtime.as_dp(sig), d["f"], d["grad"], d["g"], d["jac"], d["hess"], None))
        out = [np.empty(B), np.empty((B, p.n)), np.empty((B, p.m)), np.empty((B, p.nnz_J)),
               np.empty((B, p.nnz_H)) if Lam is not None else None]
        for name, a in zip(("f", "grad", "g", "jac", "hess"), out):
            if a is not None:
                self.ctx.check(lib.pk_copy_dev(h, a.ctypes.data, d[name], a.nbytes, None))
        self.sync()
        return out

    def cycle_batch_dev(self, B, d_x, d_lam, sigmas, d_f, d_grad, d_g, d_jac, d_hess, stream=None):
        """Enqueue the cycles of ``B`` iterates (at most ``runtime.MAX_BATCH``) on device pointers (ints) as ONE launch of
        ``pk_cycleb``, without waiting for it.  (The FIRST batch of an evaluator loads the batched code object and holds it against
        single launches -- ``_ensure_batch`` -- which compiles, evaluates and waits.)  The arrays are dense ``[B][...]``; ``sigmas``: B host values; ``d_lam = None``: an
        x-only batch (``d_hess`` is not touched)."""
        self._ensure_batch()
        sig = np.ascontiguousarray(sigmas, dtype=np.float64).reshape(-1)
        if d_lam is not None and len(sig) != int(B):
            raise ValueError(f"sigmas must have {int(B)} values")
        p = self.plan
        self._invalidate_x()
        self.ctx.check(self.ctx.lib.pk_eval_cycle_batch_dev(self.ctx.handle, int(B), d_x, p.n, d_lam, p.m, runtime.as_dp(sig) if len(sig) else None,
                                                            d_f, d_grad, d_g, d_jac, d_hess, stream))

    def cycle_batch(self, X, Lam=None, sigma=1.0):
        """The cycles of the ``B`` iterates ``X[b], Lam[b], sigma[b]`` -- one launch per ``runtime.MAX_BATCH`` of them, every
        entry bit for bit what ``cycle`` returns for it.  ``X``: (B, n); ``Lam``: (B, m), or None for the x-only outputs;
        ``sigma``: a scalar or (B,).  Returns new arrays ``(f (B,), grad (B, n), g (B, m), J (B, nnz_J), H (B, nnz_H) or None)``.
        Afterwards no iterate is the prepared one (as after ``cycle`` on plain arrays)."""
        p = self.plan
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] != p.n:
            raise ValueError(f"X must have shape (B, {p.n})")
        B = X.shape[0]
        if Lam is not None:
            Lam = np.ascontiguousarray(Lam, dtype=np.float64)
            if Lam.shape != (B, p.m):
                raise ValueError(f"Lam must have shape ({B}, {p.m})")
        sig = np.asarray(sigma, dtype=np.float64)
        if sig.ndim == 0:
            sig = np.full(B, float(sig))
        if sig.shape != (B,):
            raise ValueError(f"sigma must be a scalar or have shape ({B},)")
        sig = np.ascontiguousarray(sig)
        out = [np.empty(B), np.empty((B, p.n)), np.empty((B, p.m)), np.empty((B, p.nnz_J)),
               np.empty((B, p.nnz_H)) if Lam is not None else None]
        if B == 0:
            return tuple(out)
        self._ensure_batch()
        self._invalidate_x()        # the context's x / result buffers may hold other iterates afterwards
        try:
            for lo in range(0, B, runtime.MAX_BATCH):
                hi = min(B, lo + runtime.MAX_BATCH)
                part = self._cycle_batch_chunk(X[lo:hi], None if Lam is None else Lam[lo:hi], sig[lo:hi])
                for a, b in zip(out, part):
                    if a is not None:
                        a[lo:hi] = b
        finally:
            self._free_batch_buffers()
        return tuple(out)

    # ------------------------------------------------------------------ merit terms of a batch of trial points (csrc/pk_merit.cpp)
    def set_bounds(self, c_lb=None, c_ub=None, v_lb=None, v_ub=None):
        """The bounds the merit terms are measured against: ``(m,), (m,), (n,), (n,)``, each defaulting to the plan's.  They are
        validated (no NaN, ``lb <= ub``) and uploaded on first use; ``set_tables`` forgets them."""
        p = self.plan
        given = (c_lb, c_ub, v_lb, v_ub)
        out = []
        for a, default, count in zip(given, (p.c_lb, p.c_ub, p.v_lb, p.v_ub), (p.m, p.m, p.n, p.n)):
            a = np.ascontiguousarray(default if a is None else a, dtype=np.float64)
            if a.shape != (count,):
                raise ValueError(f"bounds must have shapes ({p.m},), ({p.m},), ({p.n},), ({p.n},)")
            out.append(a.copy())
        self._bounds, self._bounds_up = tuple(out), False

    def _ensure_merit(self):
        """What every merit entry point needs first: an unsharded evaluator, the batched code object decided
        (``_ensure_batch``), the bounds on the device."""
        if self.src.sharded:
            raise NotImplementedError("the merit terms of a batch are not offered for a sharded evaluator")
        self._ensure_batch()
        self._ensure_bounds()

    def _ensure_bounds(self):
        """The bounds on the device (the plan's unless ``set_bounds`` said otherwise), uploaded on first use."""
        if not self._bounds_up:
            if self._bounds is None:
                self.set_bounds()
            self.ctx.check(self.ctx.lib.pk_set_bounds(self.ctx.handle, *(runtime.as_dp(a) for a in self._bounds)))
            self._bounds_up = True

    def trial_points_dev(self, B, d_x, d_d, alphas, d_X, ldx=None, stream=None):
        """Enqueue ``X[b] = x + alphas[b] * d`` for ``B`` (at most ``runtime.MAX_BATCH``) host values ``alphas`` on device
        pointers (ints): the product rounded, then the sum -- the bits of NumPy's ``x + a * d``.  Rows of ``X`` are ``ldx``
        (default n) doubles apart.  Not waited for."""
        self._ensure_merit()
        a = np.ascontiguousarray(alphas, dtype=np.float64).reshape(-1)
        if len(a) != int(B):
            raise ValueError(f"alphas must have {int(B)} values")
        self._invalidate_x()
        self.ctx.check(self.ctx.lib.pk_trial_points_dev(self.ctx.handle, int(B), d_x, d_d, runtime.as_dp(a) if len(a) else None, d_X,
                                                        self.plan.n if ldx is None else int(ldx), stream))

    def merit_batch_dev(self, B, d_f, d_g, d_grad, d_X, d_out, d_d=None, ldg=None, ldgrad=None, ldx=None, stream=None):
        """Enqueue the reduction of ``B`` entries as ``cycle_batch_dev`` leaves them (device pointers, dense unless a leading
        dimension says otherwise) to ``(B, 8)`` merit terms at ``d_out`` (columns: ``merit.COLUMNS``); ``d_d``: the direction
        of the slope column, or None.  Two launches, not waited for."""
        self._ensure_merit()
        p = self.plan
        self._invalidate_x()
        self.ctx.check(self.ctx.lib.pk_merit_batch_dev(self.ctx.handle, int(B), d_f, d_g, p.m if ldg is None else int(ldg), d_grad,
                                                       p.n if ldgrad is None else int(ldgrad), d_X, p.n if ldx is None else int(ldx),
                                                       d_d, d_out, stream))

    def _direction(self, d):
        d = np.ascontiguousarray(d, dtype=np.float64)
        if d.shape != (self.plan.n,):
            raise ValueError(f"d must have shape ({self.plan.n},)")
        return d

    def merit_batch(self, X, d=None):
        """The ``(B, 8)`` merit terms (columns: ``merit.COLUMNS``) of the iterates ``X[b]``: the x-only batch and the
        reduction stay on the device, ``8 B`` doubles come back.  ``d``: the direction of the slope column (0.0 without)."""
        p = self.plan
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] != p.n:
            raise ValueError(f"X must have shape (B, {p.n})")
        d = None if d is None else self._direction(d)
        out = np.empty((X.shape[0], 8))
        if X.shape[0] == 0:
            return out
        self._ensure_merit()
        self._invalidate_x()
        self.ctx.check(self.ctx.lib.pk_merit_batch(self.ctx.handle, X.shape[0], runtime.as_dp(X), p.n, None if d is None else runtime.as_dp(d),
                                                   runtime.as_dp(out)))
        return out

    def merit_scan(self, x, d, alphas):
        """The ``(B, 8)`` merit terms of the trial points ``x + alphas[b] * d``, formed on the device: one upload of ``x`` and
        ``d``, one batch launch and two reduction launches per ``runtime.MAX_BATCH`` points, ``8 B`` doubles back."""
        x, d = self._x(x), self._direction(d)
        a = np.ascontiguousarray(alphas, dtype=np.float64).reshape(-1)
        out = np.empty((len(a), 8))
        if len(a) == 0:
            return out
        self._ensure_merit()
        self._invalidate_x()
        dp = runtime.as_dp
        self.ctx.check(self.ctx.lib.pk_merit_scan(self.ctx.handle, len(a), dp(x), dp(d), dp(a), dp(out)))
        return out

    # ------------------------------------------------------------------ barrier terms, dual residual, boundary step (csrc/pk_ipm.cpp)
    WHICH = {"x": 0, "c": 1}      # the boxed vectors: the variables with v_lb, v_ub; the constraint rows' slacks with c_lb, c_ub

    def _ensure_ipm(self):
        """What every entry point of pk_ipm.cpp needs first: an unsharded evaluator and the bounds on the device (the plan's
        unless ``set_bounds`` said otherwise).  The batched code object is not needed."""
        if self.src.sharded:
            raise NotImplementedError("the barrier terms, the dual residual and the boundary step are not offered for a sharded evaluator")
        self._ensure_bounds()

    def _which(self, which):
        if which not in self.WHICH:
            raise ValueError('which must be "x" (the variables) or "c" (the constraint rows)')
        return self.WHICH[which], self.plan.n if which == "x" else self.plan.m

    def ip_terms_dev(self, d_v, d_zl, d_zu, mu, d_sigma, d_rbar, d_out, which="x", stream=None):
        """Enqueue ``sigma`` and ``rbar`` of the boxed vector at ``d_v`` with multipliers ``d_zl, d_zu`` and the record of 8
        doubles at ``d_out`` (``BarrierTerms.COLUMNS``) on device pointers: two launches, not waited for."""
        self._ensure_ipm()
        self.ctx.check(self.ctx.lib.pk_ip_terms_dev(self.ctx.handle, self._which(which)[0], d_v, d_zl, d_zu, float(mu), d_sigma, d_rbar,
                                                    d_out, stream))

    def dual_residual_dev(self, d_jvals, d_grad, d_lam, d_r, d_out, d_z=None, negate=False, stream=None):
        """Enqueue ``r = J^T lam + grad - z`` (negated with ``negate``; ``d_z`` None: no term; 0.0 for a fixed variable) and
        the record of 4 doubles at ``d_out`` (``r_inf, r_sq, bad, 0``) on device pointers; ``d_jvals``: the CSR values of the
        Jacobian map.  Not waited for."""
        self._ensure_ipm()
        self._operator("JT")
        self.ctx.check(self.ctx.lib.pk_dual_residual_dev(self.ctx.handle, d_jvals, d_grad, d_lam, d_z, int(bool(negate)), d_r, d_out,
                                                         stream))

    def ip_step_dev(self, d_v, d_dv, d_zl, d_zu, mu, tau, d_dzl, d_dzu, d_out, which="x", stream=None):
        """Enqueue the multiplier steps ``dzl, dzu`` of the step ``d_dv`` and the record of 4 doubles at ``d_out``
        (``alpha_pri, alpha_dual, arg_pri, bad``) on device pointers: two launches, not waited for."""
        self._ensure_ipm()
        self.ctx.check(self.ctx.lib.pk_ip_step_dev(self.ctx.handle, self._which(which)[0], d_v, d_dv, d_zl, d_zu, float(mu), float(tau),
                                                   d_dzl, d_dzu, d_out, stream))

    def _boxed(self, count, **arrays):
        out = []
        for name, a in arrays.items():
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != (count,):
                raise ValueError(f"{name} must have shape ({count},)")
            out.append(a)
        return out

    def barrier_terms(self, v, zl, zu, mu, which="x"):
        """``BarrierTerms`` of the boxed vector ``v`` (``which``: "x" the variables, "c" the constraint rows' slacks) with the
        multipliers ``zl, zu`` of its lower and upper sides and the barrier parameter ``mu``: one round trip."""
        w, count = self._which(which)
        v, zl, zu = self._boxed(count, v=v, zl=zl, zu=zu)
        self._ensure_ipm()
        sigma, rbar, rec = np.empty(count), np.empty(count), np.empty(8)
        dp = runtime.as_dp
        self.ctx.check(self.ctx.lib.pk_ip_terms(self.ctx.handle, w, dp(v), dp(zl), dp(zu), float(mu), dp(sigma), dp(rbar), dp(rec)))
        return BarrierTerms(sigma, rbar, rec)

    def boundary_step(self, v, dv, zl, zu, mu, tau=0.99, which="x"):
        """``BoundaryStep`` of the step ``dv`` from ``v``: the multiplier steps and the fraction-to-the-boundary step lengths
        with parameter ``tau`` in (0, 1].  One round trip."""
        w, count = self._which(which)
        v, dv, zl, zu = self._boxed(count, v=v, dv=dv, zl=zl, zu=zu)
        self._ensure_ipm()
        dzl, dzu, rec = np.empty(count), np.empty(count), np.empty(4)
        dp = runtime.as_dp
        self.ctx.check(self.ctx.lib.pk_ip_step(self.ctx.handle, w, dp(v), dp(dv), dp(zl), dp(zu), float(mu), float(tau), dp(dzl), dp(dzu),
                                               dp(rec)))
        return BoundaryStep(dzl, dzu, rec)

    # ------------------------------------------------------------------ the step's system factored on the device (csrc/pk_band.cpp)
    def band_plan(self, ordering):
        """Upload the plan of the bordered band LU once: the permutation, the border, the half-bandwidth and the assembly map of
        a ``pockit_amd.band.BandOrdering`` built from this evaluator's CSR maps.  It replaces an earlier plan."""
        if self.src.sharded:
            raise NotImplementedError("the band factorisation is not offered for a sharded evaluator")
        self.csr_map("jac")
        self.csr_map("hess")
        order = np.ascontiguousarray(ordering.order, dtype=np.int32)
        amap = np.ascontiguousarray(ordering.map, dtype=np.int32)
        self.ctx.check(self.ctx.lib.pk_band_plan(self.ctx.handle, int(ordering.nb), int(ordering.w), int(ordering.p),
                                                 order.ctypes.data_as(runtime.c_int32_p), amap.ctypes.data_as(runtime.c_int32_p)))

    def band_factor_dev(self, d_hvals, d_jvals, d_s1, d_s2):
        """Enqueue the assembly of ``K = [[H + diag(s1), J^T], [J, -diag(s2)]]`` from the resident CSR values and ``s1`` (n),
        ``s2`` (m) on device pointers, and its band LU with partial pivoting inside the band.  Not waited for."""
        self.ctx.check(self.ctx.lib.pk_band_factor_dev(self.ctx.handle, d_hvals, d_jvals, d_s1, d_s2))

    def band_solve_dev(self, d_rhs, d_sol):
        """Enqueue the solve ``K sol = rhs`` with the factors of ``band_factor_dev`` on device vectors of n + m values (fixed
        variables get 0.0).  Not waited for; after a failed factorisation ``d_sol`` is left untouched."""
        self.ctx.check(self.ctx.lib.pk_band_solve_dev(self.ctx.handle, d_rhs, d_sol))

    def band_solve_multi_dev(self, k, d_rhs, d_sol, stride_rhs=None, stride_sol=None):
        """Enqueue the k solves ``K sol_c = rhs_c`` (1 ... 64) with the factors of ``band_factor_dev`` in the launches of ONE
        solve: right-hand side c is the n + m doubles ``stride_rhs`` c behind ``d_rhs``, its solution ``stride_sol`` c behind
        ``d_sol`` (None: n + m; at least n + m).  Column c has the bits ``band_solve_dev`` gives for it alone; the record is
        ``band_record``'s.  Not waited for; after a failed factorisation no column of ``d_sol`` is written."""
        size = self.plan.n + self.plan.m
        stride_rhs = size if stride_rhs is None else stride_rhs
        stride_sol = size if stride_sol is None else stride_sol
        self.ctx.check(self.ctx.lib.pk_band_solve_multi_dev(self.ctx.handle, int(k), d_rhs, int(stride_rhs), d_sol, int(stride_sol)))

    def band_record(self):
        """The record of the last factorisation and solve (8 doubles: status, failing column, smallest and largest |pivot|,
        Nb, w, p, interchanges), waited for."""
        rec = np.empty(8)
        self.ctx.check(self.ctx.lib.pk_band_record(self.ctx.handle, runtime.as_dp(rec)))
        return rec

    def band_refine_begin_dev(self, d_hvals, d_jvals, d_s1, d_s2, d_rhs, d_sol, tol=BAND_REFINE_TOL, min_steps=0):
        """Enqueue step 0 of the refinement of ``d_sol``, a solution of ``band_solve_dev`` for ``d_rhs`` with the factors of
        ``band_factor_dev`` on the same four arrays: ``q = K sol`` by ``kkt_apply_dev``'s fixed-order application of the TRUE K
        (the CSR values, not the assembled band), the residual at the plan's unknowns and the record.  The six arrays must stay
        valid and unchanged until the refinement ends; ``d_sol`` is refined in place.  Not waited for."""
        for op in ("J", "JT", "H"):
            self._operator(op)
        self.ctx.check(self.ctx.lib.pk_band_refine_begin_dev(self.ctx.handle, d_hvals, d_jvals, d_s1, d_s2, d_rhs, d_sol, float(tol),
                                                             int(min_steps)))

    def band_refine_advance_dev(self, steps=1):
        """Enqueue ``steps`` steps of the refinement: ``d = K^-1 r`` with the factors in place (the launches of one solve), ``sol
        += d`` while the record's status is 0, then the product, the residual and the record again.  The device decides: a step
        behind a stop runs its solve and changes nothing else, so the result does not depend on how many steps were enqueued
        beyond the stop.  Not waited for."""
        self.ctx.check(self.ctx.lib.pk_band_refine_advance_dev(self.ctx.handle, int(steps)))

    def band_refine_record(self):
        """The refinement's record (8 doubles: status -- 0 running, 1 converged, 2 stalled, 3 non-finite, 4 the factorisation
        failed --, corrections applied, ``|r|inf``, ``|x|inf``, ``|b|inf``, rho, rho of step 0, the rho before), waited for."""
        rec = np.empty(8)
        self.ctx.check(self.ctx.lib.pk_band_refine_record(self.ctx.handle, runtime.as_dp(rec)))
        return rec

    def band_factor_batch_dev(self, B, d_hvals, d_jvals, d_s1, d_s2, strides=None):
        """Enqueue ``band_factor_dev`` for B systems (1 ... 16) behind the one plan in one launch sequence: entry e reads its
        arrays e strides behind the pointers.  ``strides``: the doubles between two entries of ``(hvals, jvals, s1, s2)``,
        0 for an array all entries share (otherwise at least its length); None: ``(0, 0, n, 0)``, one H, J and ``s2`` under B
        different ``s1``.  Every entry gets the bits ``band_factor_dev`` gives for its inputs alone.  The batch has its own
        arrays: the factors of ``band_factor_dev`` stay.  Not waited for."""
        sh, sj, s1, s2 = (0, 0, self.plan.n, 0) if strides is None else strides
        self.ctx.check(self.ctx.lib.pk_band_factor_batch_dev(self.ctx.handle, int(B), d_hvals, int(sh), d_jvals, int(sj), d_s1, int(s1), d_s2,
                                                             int(s2)))

    def band_solve_batch_dev(self, B, d_rhs, d_sol, stride_rhs=0, stride_sol=None):
        """Enqueue the B solves ``K_e sol_e = rhs_e`` with the factors of ``band_factor_batch_dev`` (the same B) on device
        vectors of n + m values, ``stride_rhs`` doubles apart (0: one right-hand side for all) and ``stride_sol`` apart (None:
        n + m).  Not waited for; an entry whose factorisation failed leaves its slice of ``d_sol`` untouched and does not stop
        the others."""
        stride_sol = self.plan.n + self.plan.m if stride_sol is None else stride_sol
        self.ctx.check(self.ctx.lib.pk_band_solve_batch_dev(self.ctx.handle, int(B), d_rhs, int(stride_rhs), d_sol, int(stride_sol)))

    def band_record_batch(self, B):
        """The records of the last batch factorisation and solve, ``(B, 8)`` (row e: ``band_record``'s 8 doubles of entry e),
        waited for, in one transfer."""
        rec = np.empty((int(B), 8))
        self.ctx.check(self.ctx.lib.pk_band_record_batch(self.ctx.handle, int(B), runtime.as_dp(rec)))
        return rec

    # ------------------------------------------------------------------ the slacks of a resident iterate (csrc/pk_slack.cpp)
    def slack_reduce_dev(self, d_g, d_s, d_lam, d_sigma_s, d_rbar_s, d_s2, d_b2, d_out, stream=None):
        """Enqueue the elimination of the slacks on device pointers: ``s2`` and ``b2`` of the step's system
        ``[[H + Sigma_x, J^T], [J, -S2]]`` from the constraint values ``d_g``, the slacks, the multipliers and the slacks'
        ``sigma_s, rbar_s`` (``ip_terms_dev(..., which="c")``), and the record of 4 doubles at ``d_out``
        (``SlackTerms.COLUMNS``): two launches, not waited for."""
        self._ensure_ipm()
        self.ctx.check(self.ctx.lib.pk_slack_reduce_dev(self.ctx.handle, d_g, d_s, d_lam, d_sigma_s, d_rbar_s, d_s2, d_b2, d_out, stream))

    def slack_recover_dev(self, d_dlam, d_lam, d_rbar_s, d_s2, d_sigma_s, d_dx, d_w, d_s1, d_ds, d_out, stream=None):
        """Enqueue the slacks' step ``ds = s2 ((dlam + lam) + rbar_s)`` and the record of 5 doubles at ``d_out``
        (``SlackStep.COLUMNS``; ``d_w = H dx``, ``d_s1 = Sigma_x``) on device pointers: two launches, not waited for."""
        self._ensure_ipm()
        self.ctx.check(self.ctx.lib.pk_slack_recover_dev(self.ctx.handle, d_dlam, d_lam, d_rbar_s, d_s2, d_sigma_s, d_dx, d_w, d_s1, d_ds,
                                                         d_out, stream))

    def slack_update_dev(self, d_v, d_dv, d_zl, d_dzl, d_zu, d_dzu, alpha_p, alpha_d, mu, d_out, kappa=1e10, d_lam=None, d_dlam=None,
                         which="x", stream=None):
        """Enqueue the update IN PLACE of a boxed vector and its multipliers on device pointers: ``v += alpha_p dv``,
        ``z += alpha_d dz`` and the safeguard ``z = min(max(z, mu / (kappa d)), kappa mu / d)`` with the new slacks; with
        ``d_lam, d_dlam`` (``which="c"`` only) also ``lam += alpha_p dlam``.  The record of 4 doubles at ``d_out``:
        ``IterateUpdate.COLUMNS``.  Two launches, not waited for."""
        self._ensure_ipm()
        self.ctx.check(self.ctx.lib.pk_slack_update_dev(self.ctx.handle, self._which(which)[0], d_v, d_dv, d_zl, d_dzl, d_zu, d_dzu, d_lam,
                                                        d_dlam, float(alpha_p), float(alpha_d), float(mu), float(kappa), d_out, stream))

    def slack_merit_dev(self, count, d_X, d_G, d_s, d_ds, d_alphas, d_out, stream=None):
        """Enqueue the merit terms of ``count`` trial points with slacks on device pointers: per entry ``theta_1, theta_inf,
        log_sum, bad`` at ``d_out`` (4 * count doubles) from the points ``d_X`` (count x n), their constraint values ``d_G``
        (count x m) and the slacks ``s + alphas[b] ds``.  Two launches, not waited for."""
        self._ensure_ipm()
        self.ctx.check(self.ctx.lib.pk_slack_merit_dev(self.ctx.handle, int(count), d_X, d_G, d_s, d_ds, d_alphas, d_out, stream))

    def slack_terms(self, g, s, lam, sigma_s, rbar_s):
        """``SlackTerms`` of the constraint values ``g``, the slacks ``s``, the multipliers ``lam`` and the slacks' barrier terms
        ``sigma_s, rbar_s`` (``barrier_terms(s, yl, yu, mu, which="c")``).  One round trip."""
        m = self.plan.m
        g, s, lam, sigma_s, rbar_s = self._boxed(m, g=g, s=s, lam=lam, sigma_s=sigma_s, rbar_s=rbar_s)
        self._ensure_ipm()
        s2, b2, rec = np.empty(m), np.empty(m), np.empty(4)
        dp = runtime.as_dp
        self.ctx.check(self.ctx.lib.pk_slack_reduce(self.ctx.handle, dp(g), dp(s), dp(lam), dp(sigma_s), dp(rbar_s), dp(s2), dp(b2), dp(rec)))
        return SlackTerms(s2, b2, rec)

    def slack_step(self, dlam, lam, rbar_s, s2, sigma_s, dx, w, s1):
        """``SlackStep`` of the solve's ``dx, dlam``: the slacks' step and the terms of the curvature test; ``w = H dx``
        (``Linearization.hv``), ``s1 = Sigma_x``.  One round trip."""
        n, m = self.plan.n, self.plan.m
        dlam, lam, rbar_s, s2, sigma_s = self._boxed(m, dlam=dlam, lam=lam, rbar_s=rbar_s, s2=s2, sigma_s=sigma_s)
        dx, w, s1 = self._boxed(n, dx=dx, w=w, s1=s1)
        self._ensure_ipm()
        ds, rec = np.empty(m), np.empty(5)
        dp = runtime.as_dp
        self.ctx.check(self.ctx.lib.pk_slack_recover(self.ctx.handle, dp(dlam), dp(lam), dp(rbar_s), dp(s2), dp(sigma_s), dp(dx), dp(w), dp(s1),
                                                     dp(ds), dp(rec)))
        return SlackStep(ds, rec)

    def update_iterate(self, v, dv, zl, dzl, zu, dzu, alpha_p, alpha_d, mu, kappa=1e10, lam=None, dlam=None, which="x"):
        """``IterateUpdate``: copies of ``v, zl, zu`` (and ``lam``, with ``which="c"``) moved by the steps with the lengths
        ``alpha_p`` (v, lam) and ``alpha_d`` (zl, zu), the multipliers safeguarded with the new slacks.  One round trip."""
        w, count = self._which(which)
        v, dv, zl, dzl, zu, dzu = self._boxed(count, v=v, dv=dv, zl=zl, dzl=dzl, zu=zu, dzu=dzu)
        if (lam is None) != (dlam is None):
            raise ValueError("lam and dlam go together")
        if lam is not None:
            if which != "c":
                raise ValueError('lam goes with which="c" only')
            lam, dlam = self._boxed(count, lam=lam, dlam=dlam)
            lam = lam.copy()
        self._ensure_ipm()
        v, zl, zu, rec = v.copy(), zl.copy(), zu.copy(), np.empty(4)
        dp = runtime.as_dp
        opt = lambda a: None if a is None else dp(a)  # noqa: E731
        self.ctx.check(self.ctx.lib.pk_slack_update(self.ctx.handle, w, dp(v), dp(dv), dp(zl), dp(dzl), dp(zu), dp(dzu), opt(lam), opt(dlam),
                                                    float(alpha_p), float(alpha_d), float(mu), float(kappa), dp(rec)))
        return IterateUpdate(v, zl, zu, lam, rec)

    def batch_launches(self):
        """Launches of ``pk_cycleb`` by this evaluator so far: a batch served by the loop of single cycles adds none."""
        n = C.c_int64()
        self.ctx.check(self.ctx.lib.pk_batch_launches(self.ctx.handle, C.byref(n)))
        return n.value

    def profile(self, enable=True, period=1):
        """Time the kernels whose bit is set in ``enable`` with HIP events; only every ``period``-th launch."""
        # (the x-CALLBACKS of a profiled context run pk_xall, which the library refuses for a model with a wide phase -- error 27,
        #  DESIGN.md section 11; profiling around device-resident cycles, what bench.py does, never reaches that kernel)
        self.ctx.check(self.ctx.lib.pk_profile_sampling(self.ctx.handle, int(period)))
        self.ctx.check(self.ctx.lib.pk_profile(self.ctx.handle, int(enable)))

    def set_cycle_graph(self, enable=True):
        """Replay the fused cycle from a cached hipGraph (measured slower than plain launches on MI355X /
        ROCm 7.2 -- DESIGN.md section 5 -- so it is off by default)."""
        self.ctx.check(self.ctx.lib.pk_set_cycle_graph(self.ctx.handle, int(bool(enable))))

    #: what the guarded entry points say (the reason in full: DESIGN.md section 11; the library's own guard is error 27)
    _WIDE_SEQUENTIAL = ("is not available for a model with a wide phase (more than {nx} states): it runs the values role of such a "
                        "phase with its dynamics passes inside one wave (pk_xall), a form that returned wrong f / grad / g for "
                        "some models and raised GPU memory faults -- an open defect (DESIGN.md section 11).  The default "
                        "one-launch cycle and the five callbacks do not use it")

    def _refuse_sequential_values_role(self, what):
        if any(self.src.wide):
            raise NotImplementedError(f"pockit_amd: {what} " + self._WIDE_SEQUENTIAL.format(nx=self.src.wide_nx))

    def set_cycle_mode(self, single_launch=True):
        """True (default): one cycle = one launch (pk_cycle).  False: pk_xall, then pk_hess with the reductions."""
        if not single_launch:
            self._refuse_sequential_values_role("the two-launch form of the cycle")
        self.ctx.check(self.ctx.lib.pk_set_cycle_mode(self.ctx.handle, int(bool(single_launch))))

    def set_cycle_layout(self, jacobian_compact=False, hessian_compact=False):
        """What ``cycle_dev`` writes into its J / H buffers: the reference's triplet lists (default) or the compact layouts
        (``plan.nnz_Jc`` / ``plan.nnz_Hc`` values) -- from the same single launch."""
        if hessian_compact and not self.src.compact:
            raise NotImplementedError("compact Hessian layout is not available for this model")
        if jacobian_compact:
            self.plan.jacc  # noqa: B018
        self.ctx.check(self.ctx.lib.pk_set_cycle_layout(self.ctx.handle, int(bool(jacobian_compact)), int(bool(hessian_compact))))
        self._cycle_layout = (bool(jacobian_compact), bool(hessian_compact))

    def profile_read(self):
        """{kernel name: (launches, total_ms)} accumulated while profiling was enabled."""
        out = {}
        for k, name in enumerate(runtime.KERNELS):
            n, ms = C.c_int64(), C.c_double()
            self.ctx.check(self.ctx.lib.pk_profile_read(self.ctx.handle, k, C.byref(n), C.byref(ms)))
            out[name] = (n.value, ms.value)
        return out


class CgInfo:
    """What a CG solve on the device reports (read-only): ``status`` by name, ``iterations``, ``rel_residual`` (of the
    recurrence: ``sqrt(rr / bb)``), ``curvature`` (the last ``p^T K p``), ``alpha``, ``beta`` and the raw ``record``."""
    STATUS = {0: "running", 1: "converged", 2: "non_positive_curvature", 3: "non_finite", 4: "maxiter"}
    __slots__ = ("_rec", "_tol")

    def __init__(self, rec, tol):
        rec = np.array(rec, dtype=np.float64)
        rec.setflags(write=False)
        object.__setattr__(self, "_rec", rec)
        object.__setattr__(self, "_tol", float(tol))

    def __setattr__(self, name, value):
        raise AttributeError("CgInfo is read-only")

    record = property(lambda self: self._rec)
    status = property(lambda self: self.STATUS[int(self._rec[0])])
    iterations = property(lambda self: int(self._rec[1]))
    curvature = property(lambda self: float(self._rec[5]))
    alpha = property(lambda self: float(self._rec[6]))
    beta = property(lambda self: float(self._rec[7]))

    @property
    def rel_residual(self):
        rr, thr = float(self._rec[2]), float(self._rec[3])      # thr = tol^2 b.b
        if thr > 0.0:
            return float(np.sqrt(rr / thr)) * self._tol
        return 0.0 if rr == 0.0 else float("nan")      # (b = 0, or tol = 0: the record does not hold b.b itself)

    def __repr__(self):
        return f"CgInfo(status={self.status!r}, iterations={self.iterations}, curvature={self.curvature:.3e})"


class MinresInfo:
    """What a MINRES solve on the device reports (read-only): ``status`` by name, ``iterations``, ``rel_residual`` (of the
    recurrence, in the preconditioner's norm: ``phibar / sqrt(b.M b)``), ``primal`` and ``dual`` (views of the solution's two
    blocks) and the raw ``record`` of 16 doubles."""
    STATUS = {0: "running", 1: "converged", 2: "preconditioner_not_positive", 3: "non_finite", 4: "maxiter"}
    __slots__ = ("_rec", "_tol", "_x", "_n")

    def __init__(self, rec, tol, x, n):
        rec = np.array(rec, dtype=np.float64)
        rec.setflags(write=False)
        for name, value in (("_rec", rec), ("_tol", float(tol)), ("_x", x), ("_n", int(n))):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError("MinresInfo is read-only")

    record = property(lambda self: self._rec)
    status = property(lambda self: self.STATUS[int(self._rec[0])])
    iterations = property(lambda self: int(self._rec[1]))
    primal = property(lambda self: self._x[: self._n])
    dual = property(lambda self: self._x[self._n:])

    @property
    def rel_residual(self):
        phibar, thr = float(self._rec[2]), float(self._rec[3])      # thr = tol sqrt(b.M b)
        if thr > 0.0:
            return phibar / thr * self._tol
        return 0.0 if phibar == 0.0 else float("nan")      # (b = 0, or tol = 0: the record does not hold b.M b itself)

    def __repr__(self):
        return f"MinresInfo(status={self.status!r}, iterations={self.iterations}, rel_residual={self.rel_residual:.3e})"


class BandInfo:
    """What a band factorisation and solve on the device reports (read-only): ``status`` by name, ``column`` (the failing
    column in permuted numbering, -1 without one), ``min_pivot`` and ``max_pivot`` (of the band part), ``width``, ``border``,
    ``interchanges`` (columns whose pivot moved a row), ``primal`` and ``dual`` (views of the solution's two blocks) and the raw
    ``record`` of 8 doubles.  After a refined solve (``solve_banded(refine=r)``, r > 0) also ``residual_ratio`` (rho of the
    returned x), ``residual_ratio_start`` (rho of the unrefined solve), ``refinement_steps`` (corrections applied),
    ``refinement`` ("converged", "stalled", "non_finite", "exhausted"; "failed" behind a failed factorisation) and the raw
    ``refinement_record``; all None without one."""
    STATUS = {0: "solved", 1: "singular_band_pivot", 2: "singular_border", 3: "non_finite"}
    REFINEMENT = {1: "converged", 2: "stalled", 3: "non_finite", 4: "failed", 5: "exhausted"}
    __slots__ = ("_rec", "_x", "_n", "_rrec")

    def __init__(self, rec, x, n, rrec=None):
        rec = np.array(rec, dtype=np.float64)
        rec.setflags(write=False)
        if rrec is not None:
            rrec = np.array(rrec, dtype=np.float64)
            rrec.setflags(write=False)
        for name, value in (("_rec", rec), ("_x", x), ("_n", int(n)), ("_rrec", rrec)):
            object.__setattr__(self, name, value)

    refinement_record = property(lambda self: self._rrec)
    refinement = property(lambda self: None if self._rrec is None else self.REFINEMENT[int(self._rrec[0])])
    refinement_steps = property(lambda self: None if self._rrec is None else int(self._rrec[1]))
    residual_ratio = property(lambda self: None if self._rrec is None else float(self._rrec[5]))
    residual_ratio_start = property(lambda self: None if self._rrec is None else float(self._rrec[6]))

    def __setattr__(self, name, value):
        raise AttributeError("BandInfo is read-only")

    record = property(lambda self: self._rec)
    status = property(lambda self: self.STATUS[int(self._rec[0])])
    column = property(lambda self: int(self._rec[1]))
    min_pivot = property(lambda self: float(self._rec[2]))
    max_pivot = property(lambda self: float(self._rec[3]))
    unknowns = property(lambda self: int(self._rec[4]))
    width = property(lambda self: int(self._rec[5]))
    border = property(lambda self: int(self._rec[6]))
    interchanges = property(lambda self: int(self._rec[7]))
    primal = property(lambda self: self._x[: self._n])
    dual = property(lambda self: self._x[self._n:])

    def __repr__(self):
        return (f"BandInfo(status={self.status!r}, width={self.width}, border={self.border}, interchanges={self.interchanges}, "
                f"min_pivot={self.min_pivot:.3e}, max_pivot={self.max_pivot:.3e})")


class _Record:
    """A read-only result: named views of a record of doubles (``COLUMNS``) beside its vectors."""
    COLUMNS = ()
    __slots__ = ("_rec", "_vectors")

    def __init__(self, rec, **vectors):
        rec = np.array(rec, dtype=np.float64)
        rec.setflags(write=False)
        for v in vectors.values():
            v.setflags(write=False)
        object.__setattr__(self, "_rec", rec)
        object.__setattr__(self, "_vectors", vectors)

    def __setattr__(self, name, value):
        raise AttributeError(f"{type(self).__name__} is read-only")

    def __getattr__(self, name):
        if name in type(self).COLUMNS:
            return float(self._rec[type(self).COLUMNS.index(name)])
        vectors = object.__getattribute__(self, "_vectors")
        if name in vectors:
            return vectors[name]
        raise AttributeError(name)

    table = property(lambda self: self._rec)

    def __repr__(self):
        return f"{type(self).__name__}(" + ", ".join(f"{k}={getattr(self, k):.6g}" for k in type(self).COLUMNS if not k.startswith("_")) + ")"


class BarrierTerms(_Record):
    """What ``Evaluator.barrier_terms`` reports (read-only): the vectors ``sigma`` and ``rbar``, the columns of the record by
    name (``COLUMNS``; ``bad`` > 0: some side has a slack that is not positive or a multiplier that is negative or not finite
    and was left out), ``table`` the record itself, ``mean_compl = compl_sum / sides``."""
    COLUMNS = ("compl_inf", "compl_sum", "sides", "min_slack", "log_sum", "bad", "z_sum", "min_compl")
    __slots__ = ()

    def __init__(self, sigma, rbar, rec):
        super().__init__(rec, sigma=sigma, rbar=rbar)

    @property
    def mean_compl(self):
        return float(self._rec[1] / self._rec[2]) if self._rec[2] > 0 else 0.0


class BoundaryStep(_Record):
    """What ``Evaluator.boundary_step`` reports (read-only): the multiplier steps ``dzl, dzu``, the step lengths
    ``alpha_primal`` and ``alpha_dual`` in (0, 1], ``blocking`` (the smallest index that limits the primal step, None when the
    step is 1) and ``bad``; ``table`` is the record."""
    COLUMNS = ("alpha_primal", "alpha_dual", "_arg", "bad")
    __slots__ = ()

    def __init__(self, dzl, dzu, rec):
        super().__init__(rec, dzl=dzl, dzu=dzu)

    @property
    def blocking(self):
        return None if self._rec[2] < 0 else int(self._rec[2])


class DualResidual(_Record):
    """What ``Linearization.dual_residual`` reports beside ``r`` (read-only): ``inf = max |r_i|``, ``two_sq = sum r_i^2`` and
    ``bad`` (non-finite entries of r, left out of the other two); ``table`` is the record."""
    COLUMNS = ("inf", "two_sq", "bad", "_zero")
    __slots__ = ()


class SlackTerms(_Record):
    """What ``Evaluator.slack_terms`` reports (read-only): the vectors ``s2`` and ``b2`` of the step's system with the slacks
    eliminated, ``theta_inf`` and ``theta_1`` (the norms of ``g - c`` on equality rows and ``g - s`` on inequality rows), ``bad``
    (a ``sigma_s`` that is not positive or a residual that is not finite, left out) and ``inequalities``, their count."""
    COLUMNS = ("theta_inf", "theta_1", "bad", "inequalities")
    __slots__ = ()

    def __init__(self, s2, b2, rec):
        super().__init__(rec, s2=s2, b2=b2)


class SlackStep(_Record):
    """What ``Evaluator.slack_step`` reports (read-only): the slacks' step ``ds`` and the terms of the inertia-free curvature
    test -- ``curv_x = sum dx.w + s1.dx^2``, ``curv_s = sum sigma_s.ds^2``, ``dx_sq``, ``ds_sq`` and ``bad``;
    ``curvature = curv_x + curv_s``, ``step_sq = dx_sq + ds_sq``, ``accepts(kappa)`` the test itself."""
    COLUMNS = ("curv_x", "curv_s", "dx_sq", "ds_sq", "bad")
    __slots__ = ()

    def __init__(self, ds, rec):
        super().__init__(rec, ds=ds)

    curvature = property(lambda self: float(self._rec[0] + self._rec[1]))
    step_sq = property(lambda self: float(self._rec[2] + self._rec[3]))

    def accepts(self, kappa=1e-11):
        return self.bad == 0.0 and self.curvature >= kappa * self.step_sq


class IterateUpdate(_Record):
    """What ``Evaluator.update_iterate`` reports (read-only): the updated ``v``, ``zl``, ``zu`` and ``lam`` (None when none was
    given), ``clamped`` (multipliers the safeguard moved), ``min_slack`` (the smallest new slack) and ``bad``."""
    COLUMNS = ("clamped", "min_slack", "bad", "_zero")
    __slots__ = ()

    def __init__(self, v, zl, zu, lam, rec):
        vectors = dict(v=v, zl=zl, zu=zu)
        if lam is not None:
            vectors["lam"] = lam
        super().__init__(rec, **vectors)

    @property
    def lam(self):
        return self._vectors.get("lam")


class Linearization:
    """J (and H) of one iterate, resident on the device (``Evaluator.linearize``): products with host vectors."""

    def __init__(self, evaluator, generation, has_hessian):
        self._ev, self._gen, self.has_hessian = evaluator, generation, has_hessian
        self.m, self.n = evaluator.plan.m, evaluator.plan.n

    def _apply(self, op, v, n_in, n_out):
        ev = self._ev
        if ev.ctx is None or self._gen != ev._lin_gen:
            raise RuntimeError("stale linearization: the evaluator has been given another evaluation since (one linearization per context)")
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.shape != (n_in,):
            raise ValueError(f"the vector must have shape ({n_in},)")
        y = np.empty(n_out)
        ev.ctx.check(ev.ctx.lib.pk_apply_operator(ev.ctx.handle, ev.OPERATORS[op], runtime.as_dp(v), runtime.as_dp(y)))
        return y

    def _apply_block(self, op, V, n_in, n_out):
        ev = self._ev
        if ev.ctx is None or self._gen != ev._lin_gen:
            raise RuntimeError("stale linearization: the evaluator has been given another evaluation since (one linearization per context)")
        V = np.asarray(V, dtype=np.float64)
        if V.ndim != 2 or V.shape[0] != n_in or V.shape[1] < 1:
            raise ValueError(f"the block must have shape ({n_in}, k) with k >= 1")
        V = np.ascontiguousarray(V)
        Y = np.empty((n_out, V.shape[1]))
        ev.ctx.check(ev.ctx.lib.pk_apply_operator_block(ev.ctx.handle, ev.OPERATORS[op], V.shape[1], runtime.as_dp(V), runtime.as_dp(Y)))
        return Y

    def jmat(self, V):
        """``J V`` for a block ``V`` of shape (n, k), any memory order: (m, k), column j with the bits of ``jv(V[:, j])``"""
        return self._apply_block("J", V, self.n, self.m)

    def jtmat(self, Y):
        """``J^T Y`` for a block ``Y`` of shape (m, k): (n, k)"""
        return self._apply_block("JT", Y, self.m, self.n)

    def hmat(self, V):
        """``H V`` with the full symmetric Hessian of the Lagrangian for a block ``V`` of shape (n, k): (n, k)"""
        if not self.has_hessian:
            raise RuntimeError("this linearization has no Hessian: linearize(x, lagrange, obj_factor)")
        return self._apply_block("H", V, self.n, self.n)

    def jv(self, v):
        """``J v``"""
        return self._apply("J", v, self.n, self.m)

    def jtv(self, y):
        """``J^T y``"""
        return self._apply("JT", y, self.m, self.n)

    def hv(self, v):
        """``H v`` with the full symmetric Hessian of the Lagrangian"""
        if not self.has_hessian:
            raise RuntimeError("this linearization has no Hessian: linearize(x, lagrange, obj_factor)")
        return self._apply("H", v, self.n, self.n)

    # ---- about the entries, not about a product: row norms and weighted diagonals (csrc/pk_reduce.cpp)
    KINDS = {"1": "abs_sum", "2sq": "sq_sum", "inf": "abs_max"}

    def _check_live(self, need_h):
        """The evaluator of a handle that is still the context's linearization (and has a Hessian where one is needed)."""
        ev = self._ev
        if ev.ctx is None or self._gen != ev._lin_gen:
            raise RuntimeError("stale linearization: the evaluator has been given another evaluation since (one linearization per context)")
        if need_h and not self.has_hessian:
            raise RuntimeError("this linearization has no Hessian: linearize(x, lagrange, obj_factor)")
        return ev

    def _reduce(self, op, mode, weights, with_h=False):
        ev = self._check_live(op == "H" or with_h)
        if op not in ev.OPERATORS:
            raise ValueError('op must be "J", "JT" or "H"')
        n_rows, n_cols = {"J": (self.m, self.n), "JT": (self.n, self.m), "H": (self.n, self.n)}[op]
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64)
            if w.shape != (n_cols,):
                raise ValueError(f"the weights must have shape ({n_cols},)")
        k = ev._operator(op)
        if with_h:
            ev._operator_diagonal()
        y = np.empty(n_rows)
        ev.ctx.check(ev.ctx.lib.pk_operator_reduce(ev.ctx.handle, k, ev._reduce_mode(mode), None if w is None else runtime.as_dp(w),
                                                   int(with_h), runtime.as_dp(y)))
        return y

    def row_norms(self, op, kind, weights=None):
        """Per row of ``op`` ("J", "JT", "H") the norm ``kind`` of its entries: "1" ``sum |a|``, "2sq" ``sum a^2`` (the SQUARE
        of the 2-norm), "inf" ``max |a|``; with ``weights`` (one per column) every term is multiplied by its column's weight.
        The column norms of J are ``row_norms("JT", ...)``."""
        if kind not in self.KINDS:
            raise ValueError('kind must be "1", "2sq" or "inf"')
        return self._reduce(op, self.KINDS[kind], weights)

    def h_diag(self):
        """The diagonal of the Hessian of the Lagrangian (0.0 where the pattern has no diagonal entry)"""
        ev = self._check_live(True)
        y = np.empty(self.n)
        ev.ctx.check(ev.ctx.lib.pk_operator_diagonal(ev.ctx.handle, ev._operator_diagonal(), runtime.as_dp(y)))
        return y

    def jdjt_diag(self, d):
        """The diagonal of ``J diag(d) J^T`` (length m): what preconditions the normal equations"""
        return self._reduce("J", "sq_sum", d)

    def jtdj_diag(self, d, with_h=False):
        """The diagonal of ``J^T diag(d) J`` (length n); ``with_h``: of ``H + J^T diag(d) J``, the condensed KKT matrix -- the
        diagonal of H is formed on the device and the sums are added to it there, one round trip."""
        return self._reduce("JT", "sq_sum", d, with_h=with_h)

    # ---- the condensed KKT matrix and the normal equations: products and the CG solve on the device (csrc/pk_cg.cpp)
    def _condensed_args(self, d, shift, form, with_h):
        if form not in Evaluator.FORMS:
            raise ValueError('form must be "primal" or "dual"')
        if with_h is None:
            with_h = self.has_hessian and form == "primal"
        ev = self._check_live(bool(with_h))
        size, other = (self.n, self.m) if form == "primal" else (self.m, self.n)
        k = ev._condensed(form, bool(with_h))
        if d is not None:
            d = np.ascontiguousarray(d, dtype=np.float64)
            if d.shape != (other,):
                raise ValueError(f"d must have shape ({other},)")
        if shift is not None:
            shift = np.ascontiguousarray(np.broadcast_to(np.asarray(shift, dtype=np.float64), (size,)))
        return ev, k, bool(with_h), size, d, shift

    @staticmethod
    def _opt(a):
        return None if a is None else runtime.as_dp(a)

    def kv(self, v, d=None, shift=None, form="primal", with_h=None):
        """``K v``: ``form`` "primal" gives ``[H v] + J^T (d o (J v)) + shift o v`` (size n, ``d`` of m values), "dual"
        ``J (d o (J^T v)) + shift o v`` (size m, ``d`` of n values).  ``d`` None: the identity; ``shift`` a scalar, a vector or
        None; ``with_h`` None: H where the linearization has one.  One round trip."""
        ev, k, with_h, size, d, shift = self._condensed_args(d, shift, form, with_h)
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.shape != (size,):
            raise ValueError(f"the vector must have shape ({size},)")
        y = np.empty(size)
        ev.ctx.check(ev.ctx.lib.pk_condensed_apply(ev.ctx.handle, k, int(with_h), self._opt(d), self._opt(shift), runtime.as_dp(v),
                                                   runtime.as_dp(y)))
        return y

    def condensed_operator(self, d=None, shift=None, form="primal", with_h=None):
        """``kv`` with these arguments as a symmetric ``scipy.sparse.linalg.LinearOperator``."""
        from scipy.sparse.linalg import LinearOperator

        size = self.n if form == "primal" else self.m
        mv = lambda v: self.kv(np.asarray(v).reshape(-1), d, shift, form, with_h)  # noqa: E731
        return LinearOperator((size, size), matvec=mv, rmatvec=mv, dtype=np.float64)

    def jacobi(self, d=None, shift=None, form="primal", with_h=None):
        """The Jacobi preconditioner of ``K`` as ``solve_condensed(precond="jacobi")`` builds it on the device, bit for bit:
        ``1 / |diag K|``, 1.0 where that is zero or not finite."""
        _, _, with_h, _, d, shift = self._condensed_args(d, shift, form, with_h)
        g = self.jtdj_diag(d, with_h=with_h) if form == "primal" else self.jdjt_diag(d)
        a = np.abs(g if shift is None else g + shift)
        good = (a > 0) & np.isfinite(a)
        return np.where(good, 1.0 / np.where(good, a, 1.0), 1.0)

    def solve_condensed(self, b, d=None, shift=None, *, form="primal", with_h=None, precond="jacobi", x0=None, tol=1e-8, maxiter=None,
                        check_every=8):
        """Solve ``K x = b`` (``kv``'s matrix) by preconditioned CG on the device: one call uploads ``b`` and downloads ``x``;
        the iterations are launches with no synchronisation inside a chunk of ``check_every``.  ``precond``: "jacobi" (built on
        the device), None, or an array ``minv`` applied as ``z = minv o r``.  Convergence is ``|r| <= tol |b|`` in the
        recurrence.  Returns ``(x, info)``, ``info`` a ``CgInfo``."""
        ev, k, with_h, size, d, shift = self._condensed_args(d, shift, form, with_h)
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.shape != (size,):
            raise ValueError(f"b must have shape ({size},)")
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            if x0.shape != (size,):
                raise ValueError(f"x0 must have shape ({size},)")
        minv = None
        if precond is None:
            mode = 0
        elif isinstance(precond, str):
            if precond != "jacobi":
                raise ValueError('precond must be "jacobi", None or an array')
            mode = 1
            if with_h:
                ev._operator_diagonal()
        else:
            mode, minv = 2, np.ascontiguousarray(precond, dtype=np.float64)
            if minv.shape != (size,):
                raise ValueError(f"the preconditioner must have shape ({size},)")
        x, rec = np.empty(size), np.empty(8)
        ev.ctx.check(ev.ctx.lib.pk_solve_condensed(ev.ctx.handle, k, int(with_h), self._opt(d), self._opt(shift), mode, self._opt(minv),
                                                   runtime.as_dp(b), self._opt(x0), float(tol), int(size if maxiter is None else maxiter),
                                                   int(check_every), runtime.as_dp(x), runtime.as_dp(rec)))
        return x, CgInfo(rec, tol)

    # ---- the augmented (indefinite) KKT system: products and the MINRES solve on the device (csrc/pk_minres.cpp)
    def _kkt_args(self, s1, s2, with_h):
        if with_h is None:
            with_h = self.has_hessian
        ev = self._check_live(bool(with_h))
        ev._kkt(bool(with_h))
        if s1 is not None:
            s1 = np.ascontiguousarray(np.broadcast_to(np.asarray(s1, dtype=np.float64), (self.n,)))
        if s2 is not None:
            s2 = np.ascontiguousarray(np.broadcast_to(np.asarray(s2, dtype=np.float64), (self.m,)))
        return ev, bool(with_h), s1, s2

    def kkt_v(self, v, s1=None, s2=None, with_h=None):
        """``K v`` for ``K = [[H + diag(s1), J^T], [J, -diag(s2)]]`` and ``v = [primal (n) | dual (m)]``.  ``s1`` and ``s2``: a
        scalar, a vector or None (no term; ``s2`` None: equality constraints); ``with_h`` None: H where the linearization has
        one.  One round trip."""
        ev, with_h, s1, s2 = self._kkt_args(s1, s2, with_h)
        size = self.n + self.m
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.shape != (size,):
            raise ValueError(f"the vector must have shape ({size},)")
        y = np.empty(size)
        ev.ctx.check(ev.ctx.lib.pk_kkt_apply(ev.ctx.handle, int(with_h), self._opt(s1), self._opt(s2), runtime.as_dp(v), runtime.as_dp(y)))
        return y

    def kkt_operator(self, s1=None, s2=None, with_h=None):
        """``kkt_v`` with these arguments as a symmetric ``scipy.sparse.linalg.LinearOperator``."""
        from scipy.sparse.linalg import LinearOperator

        size = self.n + self.m
        mv = lambda v: self.kkt_v(np.asarray(v).reshape(-1), s1, s2, with_h)  # noqa: E731
        return LinearOperator((size, size), matvec=mv, rmatvec=mv, dtype=np.float64)

    @staticmethod
    def _recip(a):
        a = np.abs(a)
        good = (a > 0) & np.isfinite(a)
        return np.where(good, 1.0 / np.where(good, a, 1.0), 1.0)

    def kkt_precond(self, s1=None, s2=None, with_h=None):
        """The diagonal preconditioner of ``K`` as ``solve_kkt(precond="diagonal")`` builds it on the device, bit for bit:
        ``minv1 = 1 / |diag H + s1|``, ``minv2_i = 1 / |sum_j J_ij^2 minv1_j + s2_i|``, 1.0 where a denominator is zero or not
        finite (length n + m, positive)."""
        _, with_h, s1, s2 = self._kkt_args(s1, s2, with_h)
        g1 = self.h_diag() if with_h else None
        if g1 is None:
            minv1 = np.ones(self.n) if s1 is None else self._recip(s1)
        else:
            minv1 = self._recip(g1 if s1 is None else g1 + s1)
        g2 = self._reduce("J", "sq_sum", minv1)
        return np.concatenate((minv1, self._recip(g2 if s2 is None else g2 + s2)))

    def solve_kkt(self, b, s1=None, s2=None, *, with_h=None, precond="diagonal", x0=None, tol=1e-8, maxiter=None, check_every=8):
        """Solve ``K x = b`` (``kkt_v``'s symmetric indefinite matrix) by preconditioned MINRES on the device: one call uploads
        ``b`` and downloads ``x``; the iterations are launches with no synchronisation inside a chunk of ``check_every``.
        ``precond``: "diagonal" (built on the device, ``kkt_precond``), None, or a positive array ``minv`` of n + m values
        applied as ``y = minv o r``.  Convergence is ``|r|_M <= tol |b|_M`` in the recurrence.  Returns ``(x, info)``,
        ``info`` a ``MinresInfo``."""
        ev, with_h, s1, s2 = self._kkt_args(s1, s2, with_h)
        size = self.n + self.m
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.shape != (size,):
            raise ValueError(f"b must have shape ({size},)")
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            if x0.shape != (size,):
                raise ValueError(f"x0 must have shape ({size},)")
        minv = None
        if precond is None:
            mode = 0
        elif isinstance(precond, str):
            if precond != "diagonal":
                raise ValueError('precond must be "diagonal", None or an array')
            mode = 1
            if with_h:
                ev._operator_diagonal()
        else:
            mode, minv = 2, np.ascontiguousarray(precond, dtype=np.float64)
            if minv.shape != (size,):
                raise ValueError(f"the preconditioner must have shape ({size},)")
        x, rec = np.empty(size), np.empty(16)
        ev.ctx.check(ev.ctx.lib.pk_solve_kkt(ev.ctx.handle, int(with_h), self._opt(s1), self._opt(s2), mode, self._opt(minv),
                                             runtime.as_dp(b), self._opt(x0), float(tol), int(2 * size if maxiter is None else maxiter),
                                             int(check_every), runtime.as_dp(x), runtime.as_dp(rec)))
        return x, MinresInfo(rec, tol, x, self.n)

    def solve_banded(self, b, s1=None, s2=None, refine=0):
        """Solve ``K x = b`` (``kkt_v``'s matrix with the Hessian) by the bordered band LU on the device (csrc/pk_band.cpp):
        the ordering is built from the CSR maps and the bounds' fixed variables (``pockit_amd.band.BandOrdering``; a
        ``ValueError`` where the band is too wide), one call uploads ``b``, ``s1``, ``s2`` and downloads ``x`` and the record.
        ``s1`` and ``s2``: a scalar, a vector or None (zeros).  Returns ``(x, info)``, ``info`` a ``BandInfo``; ``x`` is all
        NaN unless ``info.status == "solved"``.  Fixed variables (``v_lb == v_ub``) are out of the system: their ``x`` is 0.0.
        Pivoting never leaves the band part: a K whose band part is singular reports ``"singular_band_pivot"``.

        ``refine`` (0 ... 10): the most corrections of an iterative refinement against the true K (the CSR values), decided on the
        device: the residual ratio ``rho = |b - K x|inf / (min(|x|inf, 1e6 |b|inf) + |b|inf)`` over the unknowns is measured, and
        while it exceeds 1e-10 and keeps falling ``x += K^-1 (b - K x)`` with the factors in place.  ``info`` then has
        ``residual_ratio``, ``residual_ratio_start``, ``refinement_steps`` and ``refinement``.  0 is the unrefined call."""
        from .band import BandOrdering

        if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or not 0 <= refine <= BAND_REFINE_MAX_STEPS:
            raise ValueError(f"refine must be an integer in 0 ... {BAND_REFINE_MAX_STEPS}")

        ev, _, s1, s2 = self._kkt_args(s1, s2, True)
        size = self.n + self.m
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.shape != (size,):
            raise ValueError(f"b must have shape ({size},)")
        s1 = np.zeros(self.n) if s1 is None else s1
        s2 = np.zeros(self.m) if s2 is None else s2
        free = np.asarray(ev.plan.v_lb, dtype=np.float64) != np.asarray(ev.plan.v_ub, dtype=np.float64)
        ordering = BandOrdering(ev.csr_map("jac"), ev.csr_map("hess"), free)
        ev.band_plan(ordering)
        x, rec = np.full(size, np.nan), np.empty(8)
        dp = runtime.as_dp
        if refine:
            rrec = np.empty(8)
            ev.ctx.check(ev.ctx.lib.pk_solve_banded_refined(ev.ctx.handle, dp(s1), dp(s2), dp(b), dp(x), dp(rec), dp(rrec), BAND_REFINE_TOL, 0,
                                                            int(refine)))
            return x, BandInfo(rec, x, self.n, rrec)
        ev.ctx.check(ev.ctx.lib.pk_solve_banded(ev.ctx.handle, dp(s1), dp(s2), dp(b), dp(x), dp(rec)))
        return x, BandInfo(rec, x, self.n)

    def solve_banded_batch(self, b, s1=None, s2=None):
        """``solve_banded`` for B systems (1 ... 16) that share this linearization's J and H and differ in ``s1``, ``s2`` and
        ``b``, factored and solved in ONE launch sequence (the launches of one system, B times the workgroups each).  ``b``:
        ``(B, n + m)``; ``s1``: None, a scalar, ``(n,)`` or ``(B, n)``; ``s2`` the same with m.  Returns ``(X, infos)``: ``X`` of
        shape ``(B, n + m)`` and a list of B ``BandInfo``; row e has the bits ``solve_banded(b[e], s1[e], s2[e])`` returns, and is
        all NaN unless ``infos[e].status == "solved"`` -- an entry that fails does not stop the others.  The ordering and its
        ``ValueError``s are ``solve_banded``'s."""
        from .band import BandOrdering

        ev = self._check_live(True)
        ev._kkt(True)
        size = self.n + self.m
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.ndim != 2 or b.shape[1] != size or not 1 <= b.shape[0] <= 16:
            raise ValueError(f"b must have shape (B, {size}) with B in 1 ... 16")
        B = b.shape[0]

        def rows(s, length, name):
            s = np.zeros(length) if s is None else np.asarray(s, dtype=np.float64)
            if s.ndim == 2 and s.shape != (B, length):
                raise ValueError(f"{name} must be a scalar, ({length},) or ({B}, {length})")
            return np.ascontiguousarray(np.broadcast_to(s, (B, length)))

        s1, s2 = rows(s1, self.n, "s1"), rows(s2, self.m, "s2")
        free = np.asarray(ev.plan.v_lb, dtype=np.float64) != np.asarray(ev.plan.v_ub, dtype=np.float64)
        ordering = BandOrdering(ev.csr_map("jac"), ev.csr_map("hess"), free)
        ev.band_plan(ordering)
        X, rec = np.full((B, size), np.nan), np.empty((B, 8))
        dp = runtime.as_dp
        ev.ctx.check(ev.ctx.lib.pk_solve_banded_batch(ev.ctx.handle, B, dp(s1), dp(s2), dp(b), dp(X), dp(rec)))
        return X, [BandInfo(rec[e], X[e], self.n) for e in range(B)]

    MULTI_CAP = 64      # PK_BD_RHS_CAP: the right-hand sides of one block solve

    def solve_banded_multi(self, B, s1=None, s2=None):
        """``solve_banded`` for k right-hand sides against ONE factorisation: ``B`` of shape ``(k, n + m)``, any k >= 1, ``s1``
        and ``s2`` as ``solve_banded`` takes them (one matrix).  Up to 64 right-hand sides are one call -- one upload, the
        factorisation, a block solve in the launches of one solve, one download; beyond that the rows are served in chunks of
        64 against the same factors.  Returns ``(X, info)``: ``X`` of shape ``(k, n + m)``, row c with the bits
        ``solve_banded(B[c], s1, s2)`` returns, all NaN unless ``info.status == "solved"``; ``info`` a ``BandInfo`` (on row
        0).  The ordering and its ``ValueError``s are ``solve_banded``'s."""
        from .band import BandOrdering

        ev, _, s1, s2 = self._kkt_args(s1, s2, True)
        size = self.n + self.m
        B = np.ascontiguousarray(B, dtype=np.float64)
        if B.ndim != 2 or B.shape[1] != size or B.shape[0] < 1:
            raise ValueError(f"B must have shape (k, {size}) with k >= 1")
        k = B.shape[0]
        s1 = np.zeros(self.n) if s1 is None else s1
        s2 = np.zeros(self.m) if s2 is None else s2
        free = np.asarray(ev.plan.v_lb, dtype=np.float64) != np.asarray(ev.plan.v_ub, dtype=np.float64)
        ordering = BandOrdering(ev.csr_map("jac"), ev.csr_map("hess"), free)
        ev.band_plan(ordering)
        X, rec = np.full((k, size), np.nan), np.empty(8)
        dp = runtime.as_dp
        first = min(k, self.MULTI_CAP)
        head = np.full((first, size), np.nan)
        ev.ctx.check(ev.ctx.lib.pk_solve_banded_multi(ev.ctx.handle, first, dp(s1), dp(s2), dp(np.ascontiguousarray(B[:first])), dp(head), dp(rec)))
        X[:first] = head
        if k > first and rec[0] == 0.0:      # the later chunks go against the factors that call left, through device arrays of the context
            lib, h = ev.ctx.lib, ev.ctx.handle
            nbytes = 8 * self.MULTI_CAP * max(size, 1)
            d_b, d_x = C.c_void_p(), C.c_void_p()
            ev.ctx.check(lib.pk_device_alloc(h, nbytes, 0, C.byref(d_b)))
            try:
                ev.ctx.check(lib.pk_device_alloc(h, nbytes, 0, C.byref(d_x)))
                for lo in range(first, k, self.MULTI_CAP):
                    rows = min(self.MULTI_CAP, k - lo)
                    chunk, out = np.ascontiguousarray(B[lo: lo + rows]), np.empty((rows, size))
                    if size:
                        ev.ctx.check(lib.pk_copy_dev(h, d_b.value, chunk.ctypes.data, chunk.nbytes, None))
                    ev.band_solve_multi_dev(rows, d_b.value, d_x.value, stride_rhs=size, stride_sol=size)
                    if size:
                        ev.ctx.check(lib.pk_copy_dev(h, out.ctypes.data, d_x.value, out.nbytes, None))
                    ev.sync()
                    X[lo: lo + rows] = out
                rec = ev.band_record()
            finally:
                for ptr in (d_b, d_x):
                    if ptr.value:
                        lib.pk_device_free(h, ptr.value)
        return X, BandInfo(rec, X[0], self.n)

    # ---- the dual side of optimality, and the first block of the KKT right-hand side (csrc/pk_ipm.cpp)
    def dual_residual(self, grad, lam, z=None, negate=False):
        """``r = J^T lam + grad - z`` on the device, negated with ``negate``; ``z`` None: no term; ``r_i = 0.0`` for a fixed
        variable.  ``z = zl - zu`` gives the optimality test, ``z = rbar`` with ``negate`` the KKT step's ``b1``.  Returns
        ``(r, DualResidual)``.  One round trip."""
        ev = self._check_live(False)
        grad, = ev._boxed(self.n, grad=grad)
        lam, = ev._boxed(self.m, lam=lam)
        if z is not None:
            z, = ev._boxed(self.n, z=z)
        ev._ensure_ipm()
        ev._operator("JT")
        r, rec = np.empty(self.n), np.empty(4)
        dp = runtime.as_dp
        ev.ctx.check(ev.ctx.lib.pk_dual_residual(ev.ctx.handle, dp(grad), dp(lam), self._opt(z), int(bool(negate)), dp(r), dp(rec)))
        return r, DualResidual(rec)

    def jacobian_operator(self):
        from scipy.sparse.linalg import LinearOperator

        flat = lambda f: lambda v: f(np.asarray(v).reshape(-1))  # noqa: E731  (SciPy also passes columns)
        return LinearOperator((self.m, self.n), matvec=flat(self.jv), rmatvec=flat(self.jtv), matmat=self.jmat, rmatmat=self.jtmat,
                              dtype=np.float64)

    def hessian_operator(self):
        from scipy.sparse.linalg import LinearOperator

        hv = lambda v: self.hv(np.asarray(v).reshape(-1))  # noqa: E731
        return LinearOperator((self.n, self.n), matvec=hv, rmatvec=hv, matmat=self.hmat, rmatmat=self.hmat, dtype=np.float64)
