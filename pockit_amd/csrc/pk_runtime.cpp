// pk_runtime.cpp -- host runtime behind the C ABI of include/pockit_hip.h.
//
// This file is the CORE unit: context, model and problem set-up, the launch machinery, the device-pointer entry points, the
// one-shot host-buffer entry points and the cycle.  Its siblings (pk_runtime.h lists them): pk_shim.cpp (host shim),
// pk_pool.cpp (helper threads), pk_shard.cpp (sharding), pk_extras.cpp (CSR, mesh error, profiling), pk_ops.cpp (J, J^T, H times a vector), pk_reduce.cpp (reductions over their rows), pk_merit.cpp (merit terms), pk_cg.cpp (CG on the condensed matrices), pk_minres.cpp (MINRES on the augmented KKT system), pk_ipm.cpp (barrier terms, dual residual, boundary step), pk_slack.cpp (slack elimination, slack step, iterate update, merit terms with slacks), pk_solve.cpp (what the two solves share on the host), pk_error.cpp.
//
// Owns: the HIP context objects of one GPU (stream, loaded code object, kernel handles), the
// device copies of the per-(model, mesh) tables, and device work buffers (x, lambda, outputs,
// integrals, per-tile partial sums).  It launches the kernels of the generated code object
// (pockit_amd/codegen.py + csrc/pk_kernels.hip.h) in the order each NLP callback needs:
//
//   eval_f     pk_int, pk_fin(integrals, f)
//   eval_grad  [pk_int, pk_fin(integrals)]?  pk_grad, pk_fin(gradient slots)
//   eval_g     [pk_int, pk_fin(integrals)]?  pk_g
//   eval_jac   [pk_int, pk_fin(integrals)]?  pk_jac
//   eval_hess  [pk_int, pk_fin(integrals)]?  pk_hess
//   batch      pk_cycleb: B cycles in ONE launch, a code object of its own (pk_batch.cpp)
//   cycle      pk_cycle: ONE launch holding pk_xall's workgroups (f partials, grad f, g, J from one node
//              evaluation), pk_hess's workgroups and a finalize workgroup that receives the partial sums of
//              the same launch through hand-off slots (integrals, f, shared gradient slots);
//              pk_set_cycle_mode(0) selects the older two-launch form pk_xall, pk_hess(+ reductions)
// ("?" = only when a system-level function is nonlinear in the integrals, pk_model_desc.prepass_*).
//
// There is no CPU evaluation path: every entry point fails with an error code when no device /
// code object / problem is present.
#include "pk_runtime.h"

void drop_cycle_graph(pk_ctx* c) {
  if (c->graph.cyc_exec) { (void)hipGraphExecDestroy(c->graph.cyc_exec); c->graph.cyc_exec = nullptr; }
  if (c->graph.rep_exec) { (void)hipGraphExecDestroy(c->graph.rep_exec); c->graph.rep_exec = nullptr; }
}

namespace {

// every area frees what it owns (free_shim: pk_shim.cpp; free_mesh_error, free_csr, free_trace: pk_extras.cpp; free_operators: pk_ops.cpp; free_merit: pk_merit.cpp; free_ipm: pk_ipm.cpp; free_slack: pk_slack.cpp; free_band: pk_band.cpp; solve_free: pk_runtime.h)
void free_problem(pk_ctx* c) {
  release(c->d_items_jacc); release(c->d_Jc);
  release(c->d_phases); release(c->d_tiles); release(c->d_kinds); release(c->d_items_jac); release(c->d_items_hess); release(c->d_items_aux); release(c->d_outer); release(c->d_aux); release(c->d_items_hessc); release(c->d_Hc);
  free_mesh_error(c);
  release(c->d_big_stage);
  drop_cycle_graph(c);
  free_trace(c);
  free_operators(c);
  free_csr(c);
  release(c->d_ib); release(c->d_db); release(c->d_lb);
  c->d_g = c->d_grad = nullptr;   // (interior pointers of the d_J allocation: one block [J | grad f | g])
  release(c->d_x); release(c->d_lam); release(c->d_f); release(c->d_J);
  release(c->d_H); release(c->d_I); release(c->d_partial); release(c->d_partial2);
  release(c->d_cpart); release(c->d_cpart2);
  free_batch(c);
  free_merit(c);
  solve_free(c->cg);
  solve_free(c->minres);
  free_ipm(c);
  free_slack(c);
  free_band(c);
  free_shim(c);
  c->have_problem = false;
}

}  // namespace

PkArgs base_args(pk_ctx* c, const double* d_x, const double* d_lam, double sigma) {
  PkArgs A;      // (only the bytes the code object declares are filled and launched: the head and its phase records)
  std::memset(static_cast<void*>(&A), 0, args_bytes(c));
  A.x = d_x; A.lam = d_lam; A.sigma = sigma;
  A.phase = (const PkPhase*)c->d_phases; A.tile = (const PkTile*)c->d_tiles; A.kind = (const PkKind*)c->d_kinds;
  A.items = nullptr; A.ib = c->d_ib; A.db = c->d_db; A.lb = c->d_lb;
  A.Ibuf = c->shard.ext_I ? c->shard.ext_I : c->d_I; A.partial = c->d_partial; A.partial2 = c->d_partial2;
  A.cpart = c->d_cpart; A.cpart2 = c->d_cpart2; A.o_aux = c->d_aux; A.outer = (const PkOuter*)c->d_outer; A.n_outer = c->n_outer;
  A.n_tiles = c->n_tiles; A.n_items = 0; A.n_phase = c->n_phase; A.n = c->n;
  A.l_s = c->l_s; A.n_s = c->n_s; A.n_sys = c->n_sys; A.m = c->m;
  A.gz_off = c->gz_off; A.n_gz = c->n_gz; A.flags = c->shard.flags | c->debug_flags;
  for (size_t k = 0; k < c->h_phases.size(); ++k) A.ph[k] = c->h_phases[k];
  A.trace = c->profile.d_trace;
  A.o_gshared = c->shard.gshared;
  A.big_stage = c->d_big_stage; A.big_row = c->big_row; A.big_slot = c->big_slot;
  A.status = c->shim.res[0].h_out ? reinterpret_cast<unsigned long long*>(c->shim.res[0].h_out + 6) : nullptr;
  A.poll_limit = c->shim.poll_limit;
  return A;
}

// pk_launch_shape with the facts of the context's problem (n_flat: entries of pk_csr / chunks of pk_runs; layout: pk_cyclec's)
PkLaunchShape shape_of(const pk_ctx* c, int k, int64_t n_flat, int layout) {
  return pk_launch_shape(k, c->md, {c->n_tiles, c->split_xall, c->exchange.in_launch && c->exchange.world > 1, layout, c->n_outer, c->mesh_error.n_groups, n_flat});
}

int launch_raw(pk_ctx* c, int k, void* args, size_t sz, const PkLaunchShape& shape, hipStream_t st) {
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
  EventPair ev{};
  const unsigned grid = shape.grid;
  if (grid == 0) return 0;
  if (shape.lds_bytes > PK_LDS_LIMIT)
    return fail(c, 22, "%s needs %zu bytes of LDS per workgroup (> 160 KiB)", kKernelNames[k], shape.lds_bytes);
  // every `profile_period`-th launch of a selected kernel is timed (the timed launch path costs ~2-3 us of host
  // and command-processor work, so timing all of them would slow the loop being measured)
  const bool timed = c->profile.on && ((c->profile.mask >> k) & 1u) && (c->profile.seen[k]++ % c->profile.period == 0);
  if (timed) {
    // Timed launch: hipExtModuleLaunchKernel attaches the events to the dispatch packet itself, so
    // elapsed(a, b) is the kernel's own start->end on this stream (what rocprofv3 reports), without
    // the command-processor gaps a hipEventRecord pair around the launch would add.
    if (!c->profile.free_events.empty()) {
      ev = c->profile.free_events.back();
      c->profile.free_events.pop_back();
    } else {
      PK_HIP(c, hipEventCreate(&ev.a));
      PK_HIP(c, hipEventCreate(&ev.b));
    }
    PK_HIP(c, hipExtModuleLaunchKernel(c->fn[k], grid * PK_BLOCK, shape.batch, 1, PK_BLOCK, 1, 1, shape.lds_bytes, st, nullptr, config,
                                       ev.a, ev.b, 0));
    c->profile.pending[k].push_back(ev);
    return 0;
  }
  PK_HIP(c, hipModuleLaunchKernel(c->fn[k], grid, shape.batch, 1, PK_BLOCK, 1, 1, (unsigned)shape.lds_bytes, st, nullptr, config));
  return 0;
}

int launch(pk_ctx* c, int k, PkArgs& A, hipStream_t st, int64_t n_flat) {
  // pk_xall runs the values role of a WIDE phase with its dynamics passes inside the values wave: wrong f / grad / g for
  // some models and GPU memory faults (round 5, an open defect on that kernel's SGPR-spill path).
  // Every route to it -- the two-launch cycle, a profiled context, pk_set_option("xpart_single", 0), the x-part of a
  // sharded context with the in-launch exchange, integrals-first models with intervals of more than 64 points -- ends here.
  if (k == K_XALL && c->md.wide)
    return fail(c, 27, "pk_xall is not offered for a model with a wide phase (open defect of its sequential values role, DESIGN.md "
                       "section 11): use the one-launch cycle / the callbacks of an unprofiled context (the default)");
  return launch_raw(c, k, &A, args_bytes(c), shape_of(c, k, n_flat), st);
}

int prepass(pk_ctx* c, const double* d_x, const double* d_lam, double sigma, double* d_f, bool write_f, hipStream_t st) {
  PkArgs A = base_args(c, d_x, d_lam, sigma);
  A.o_f = d_f;
  int rc = launch(c, K_INT, A, st);
  if (rc) return rc;
  A.flags |= F_FIN_INT | (write_f ? F_WRITE_F : 0);
  return launch(c, K_FIN, A, st);
}

// The integral pre-pass in front of a callback whose system functions are nonlinear in the integrals (`needed`: the callback's
// pk_model_desc.prepass_*), unless the caller reduces the integrals itself (a shard, pk_set_shard).
static int prepass_if(pk_ctx* c, int32_t needed, const double* d_x, const double* d_lam, double sigma, hipStream_t st) {
  return (needed && !c->shard.external_prepass) ? prepass(c, d_x, d_lam, sigma, c->d_f, false, st) : 0;
}

// the cycle as ONE launch (pk_cycle): [edge J | edge H | finalize | tile slots: x block(s) + Hessian block per group]
// (d_lam == NULL: the x-part alone -- the Hessian workgroups of the grid leave at once)
// layout: bit 0 -- d_jac receives the COMPACT Jacobian (the Jacobian role of the launch runs pk_jacc's tile code), bit 1 --
// d_hess receives the COMPACT Hessian (the Hessian workgroups run pk_hessc's); -1: what pk_set_cycle_layout chose
PkArgs cycle_args(pk_ctx* c, const double* d_x, const double* d_lam, double sigma, double* d_f, double* d_grad, double* d_g,
                  double* d_jac, double* d_hess, int layout) {
  PkArgs A = base_args(c, d_x, d_lam, sigma);
  if (!d_lam) A.flags |= F_NO_HESS;
  A.o_f = d_f; A.o_grad = d_grad; A.o_g = d_g; A.o_jac = d_jac; A.o_hess = d_hess;
  A.items = (const PkItem*)((layout & 1) ? c->d_items_jacc : c->d_items_jac);
  A.n_items = (layout & 1) ? c->n_items_jacc : c->n_items_jac;
  A.items2 = (const PkItem*)((layout & 2) ? c->d_items_hessc : c->d_items_hess);
  A.n_items2 = (layout & 2) ? c->n_items_hessc : c->n_items_hess;
  if (layout & 1) A.flags |= F_COMPACT_J;
  if (layout & 2) A.flags |= F_COMPACT_H;
  A.flags |= F_FIN_INT | F_WRITE_F | F_FIN_GRAD | (c->split_xall ? F_SPLIT : 0);
  if (c->exchange.in_launch && c->exchange.world > 1) {      // sharded: the sums over the ranks are exchanged inside this launch
    A.flags |= F_XCHG;
    A.xc_box = (unsigned long long* const*)c->exchange.box; A.xc_idx = c->exchange.idx;
    A.xc_world = c->exchange.world; A.xc_rank = c->exchange.rank; A.xc_epoch = 0; A.xc_nsh = c->exchange.nsh; A.xc_stride = c->exchange.stride;
  }      // (xc_epoch = 0: the cycle number is kept in device memory, so these arguments never change -> graph-replayable)
  return A;
}

int enqueue_single_launch_cycle(pk_ctx* c, const double* d_x, const double* d_lam, double sigma, double* d_f,
                                double* d_grad, double* d_g, double* d_jac, double* d_hess, hipStream_t st, int layout) {
  if (layout < 0) layout = c->cycle_layout;
  const PkArgs A = cycle_args(c, d_x, d_lam, sigma, d_f, d_grad, d_g, d_jac, d_hess, layout);
  // (the compact layouts: pk_cyclec, the same launch compiled with their roles -- a kernel of its own so that pk_cycle's
  //  register count stays what the reference layouts need)
  const int k = layout ? K_CYCLEC : K_CYCLE;
  const PkLaunchShape shape = shape_of(c, k, 0, layout);
  // pk_cycle's kernarg segment: the scalars a tile wave needs first (preloaded into SGPRs), then the PkArgs
  struct CycleArgs {
    const PkTile* tile;
    int32_t n_tiles, flags, grid, pad;
    PkArgs A;
  } K;
  static_assert(offsetof(CycleArgs, A) == PK_CYCLE_ARGS_OFFSET, "layout of pk_cycle's kernel arguments");
  K.tile = A.tile; K.n_tiles = A.n_tiles; K.flags = A.flags; K.grid = (int32_t)shape.grid; K.pad = 0;
  std::memcpy(static_cast<void*>(&K.A), &A, args_bytes(c));
  return launch_raw(c, k, &K, offsetof(CycleArgs, A) + args_bytes(c), shape, st);
}

namespace {
int enqueue_fused_cycle(pk_ctx* c, const double* d_x, const double* d_lam, double sigma, double* d_f, double* d_grad,
                        double* d_g, double* d_jac, double* d_hess, hipStream_t st) {
  int rc;
  if (c->cycle_mode == 1) return enqueue_single_launch_cycle(c, d_x, d_lam, sigma, d_f, d_grad, d_g, d_jac, d_hess, st);
  if (c->cycle_layout) return fail(c, 69, "the two-launch cycle (pk_set_cycle_mode 0) writes the reference layouts only");
  PkArgs A = base_args(c, d_x, nullptr, 0.0);
  A.o_f = d_f; A.o_grad = d_grad; A.o_g = d_g; A.o_jac = d_jac;
  A.items = (const PkItem*)c->d_items_jac;
  A.n_items = c->n_items_jac;
  A.flags |= (c->split_xall ? F_SPLIT : 0);
  if ((rc = launch(c, K_XALL, A, st))) return rc;
  // pk_hess's boundary workgroup also performs pk_fin's reductions (f, shared gradient slots)
  PkArgs H = base_args(c, d_x, d_lam, sigma);
  H.o_f = d_f; H.o_grad = d_grad; H.o_hess = d_hess;
  H.items = (const PkItem*)c->d_items_hess;
  H.n_items = c->n_items_hess;
  H.flags |= F_FIN_INT | F_WRITE_F | F_FIN_GRAD | (c->split_xall ? F_SPLIT : 0);
  return launch(c, K_HESS, H, st);
}

// Meshes with big intervals (more than 64 points) are served by the fused x-kernel only: a single callback on device
// pointers runs it with the context's own buffers for the outputs nobody asked for.
int eval_one_via_xpart(pk_ctx* c, const double* d_x, int which, double* d_out, void* stream) {
  c->shim.x_valid = false;
  double* o[4] = {c->d_f, c->d_grad, c->d_g, c->d_J};
  o[which] = d_out;
  return pk_eval_xpart_dev(c, d_x, o[0], o[1], o[2], o[3], stream);
}
}  // namespace

// can the x-part of an iterate come from ONE pk_cycle launch without its Hessian role?
bool xpart_is_one_launch(const pk_ctx* c) {
  const bool needs_I = c->md.prepass_grad || c->md.prepass_g || c->md.prepass_jac || c->md.prepass_hess || c->separate_x;
  return c->xpart_single && c->cycle_mode == 1 && !needs_I && c->profile.mask == 0 && !(c->exchange.in_launch && c->exchange.world > 1);
}

extern "C" {

int pk_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int pk_create(pk_ctx** out, int device_id) {
  if (!out) return fail(nullptr, 1, "pk_create: null output pointer");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(nullptr, 10, "pk_create: no HIP device available (%s); the evaluator has no CPU path",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, 11, "pk_create: device %d out of range [0,%d)", device_id, ndev);
  pk_ctx* c = new pk_ctx();
  c->device = device_id;
  if (const char* dbg = getenv("POCKIT_AMD_DEBUG_FLAGS")) c->debug_flags = atoi(dbg) & (256 | 512 | 1024 | 2048 | 4096 | 8192 | 16384 | 32768 | 65536 | 131072);
  if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
    int rc = fail(nullptr, 12, "pk_create: %s", hipGetErrorString(e));
    delete c;
    return rc;
  }
  *out = c;
  return 0;
}

void pk_destroy(pk_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (int k = 0; k < K_COUNT; ++k)
    for (auto& ev : c->profile.pending[k]) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
  for (auto& ev : c->profile.free_events) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
  free_problem(c);
  unload_batch_model(c);
  if (c->module) (void)hipModuleUnload(c->module);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* pk_last_error(pk_ctx* c) { return c ? c->error.c_str() : last_contextless_error(); }

int pk_load_model(pk_ctx* c, const void* code_object, size_t len, const pk_model_desc* md) {
  if (!c) return fail(nullptr, 1, "null context");
  if (!code_object || len == 0 || !md) return fail(c, 20, "pk_load_model: empty code object or descriptor");
  PK_HIP(c, hipSetDevice(c->device));
  unload_batch_model(c);      // (a batched object belongs to the model it was generated from)
  if (c->module) { (void)hipModuleUnload(c->module); c->module = nullptr; c->have_model = false; }
  PK_HIP(c, hipModuleLoadData(&c->module, code_object));
  for (int k = 0; k < K_COUNT; ++k)
    if (!pk_kernel_of_batched_object(k)) PK_HIP(c, hipModuleGetFunction(&c->fn[k], c->module, kKernelNames[k]));
  c->md = *md;
  if (md->tab_cap != 64 && md->tab_cap != 256) return fail(c, 23, "pk_load_model: table capacity %d (64 or 256)", md->tab_cap);
  if (md->cycle_subs < 0 || md->cycle_subs > 4096) return fail(c, 25, "pk_load_model: cycle_subs %d", md->cycle_subs);
  if (md->hess_subs < 0 || md->hess_subs > 4096 || (md->hess_subs > 0) != (md->cycle_subs > 0))
    return fail(c, 25, "pk_load_model: hess_subs %d with cycle_subs %d", md->hess_subs, md->cycle_subs);
  if (md->wide < 0 || md->wide > 1) return fail(c, 25, "pk_load_model: wide %d", md->wide);
  if (md->big_global < 0 || md->big_global > 1 || md->big_rows < 0 || md->big_rows > (1 << 20))
    return fail(c, 25, "pk_load_model: big_global %d / big_rows %d", md->big_global, md->big_rows);
  if (md->hessc_subs < 0 || md->hessc_subs > 4096 || md->jacc_subs < 0 || md->jacc_subs > 4096 ||
      ((md->hessc_subs > 0 || md->jacc_subs > 0) && md->cycle_subs == 0))
    return fail(c, 25, "pk_load_model: hessc_subs %d / jacc_subs %d with cycle_subs %d", md->hessc_subs, md->jacc_subs, md->cycle_subs);
  if (md->max_phases < 0 || md->max_phases > PK_HOST_MAX_PHASES || md->n_phase > (md->max_phases > 0 ? md->max_phases : 8))
    return fail(c, 24, "pk_load_model: %d phases, code object compiled for %d (the library passes at most %d phase records in "
                       "the kernel arguments)", md->n_phase, md->max_phases > 0 ? md->max_phases : 8, PK_HOST_MAX_PHASES);
  // what the launches will ask for (pk_launch.h); pk_cyclec with every compact role the descriptor has expressions for, which
  // needs no less than any other layout.  Not pk_aux and pk_err: a model without outer-product blocks / a caller without mesh
  // error tables never launches them (errors 22, 72).
  PkLaunchFacts p;
  p.layout = (md->ne_jc > 0 ? 1 : 0) | (md->ne_hc > 0 ? 2 : 0);
  for (int k = 0; k < K_COUNT; ++k) {
    const size_t lds = pk_launch_shape(k, *md, p).lds_bytes;
    if (k != K_AUX && k != K_ERR && lds > PK_LDS_LIMIT)
      return fail(c, 21, "pk_load_model: model needs %zu bytes of LDS per workgroup (> 160 KiB)", lds);
  }
  c->have_model = true;
  return 0;
}

int pk_set_problem(pk_ctx* c, const pk_problem_desc* pd) {
  if (!c) return fail(nullptr, 1, "null context");
  if (!c->have_model) return fail(c, 2, "pk_set_problem: load a model first");
  if (!pd) return fail(c, 30, "pk_set_problem: null descriptor");
  if (pd->n_phase > (c->md.max_phases > 0 ? c->md.max_phases : 8))
    return fail(c, 32, "pk_set_problem: %d phases, but the code object was generated for at most %d", pd->n_phase,
                c->md.max_phases > 0 ? c->md.max_phases : 8);
  if (pd->n_phase != c->md.n_phase) return fail(c, 31, "pk_set_problem: %d phases but the model was generated for %d", pd->n_phase, c->md.n_phase);
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  free_problem(c);
  c->n = pd->n; c->m = pd->m; c->n_sys = pd->n_sys; c->n_s = pd->n_s; c->l_s = pd->l_s;
  c->n_phase = pd->n_phase; c->n_tiles = pd->n_tiles; c->nnz_J = pd->nnz_J; c->nnz_H = pd->nnz_H;
  c->n_items_jac = pd->n_items_jac; c->n_items_hess = pd->n_items_hess; c->gz_off = pd->gz_off; c->n_gz = pd->n_gz;
  c->n_items_aux = pd->n_items_aux; c->n_outer = pd->n_outer; c->n_aux = pd->n_aux;
  c->cycle_layout = 0;
  c->n_items_hessc = pd->n_items_hessc; c->nnz_Hc = pd->nnz_Hc;
  c->n_items_jacc = pd->n_items_jacc; c->nnz_Jc = pd->nnz_Jc;
  // Small meshes are bound by the serial chain of one wave, not by throughput: let two waves share a tile in
  // pk_xall as long as that still leaves at most two waves per SIMD (POCKIT_AMD_SPLIT=0/1 overrides).
  {
    const char* env = getenv("POCKIT_AMD_SPLIT");
    c->split_xall = env ? atoi(env) != 0 : (pd->n_tiles > 0 && pd->n_tiles <= 1024);
  }
  int rc;
  if ((rc = upload(c, &c->d_phases, pd->phases, sizeof(PkPhase) * (size_t)pd->n_phase))) return rc;
  c->h_phases.assign((const PkPhase*)pd->phases, (const PkPhase*)pd->phases + pd->n_phase);

  {   // intervals with more than 256 points stage their rows in device memory: slot numbers into the tile records
    std::vector<PkTile> tiles((const PkTile*)pd->tiles, (const PkTile*)pd->tiles + pd->n_tiles);
    int32_t n_stage = 0, kmax = 0;
    for (PkTile& t : tiles) {
      t.stage = 0;
      if (t.nj > 0 && t.K > (c->md.big_global ? PK_WAVE : 256)) {
        t.stage = n_stage++;
        if (t.K > kmax) kmax = t.K;
      }
    }
    release(c->d_big_stage);
    c->big_row = c->big_slot = 0;
    c->big_stage_doubles = 0;
    if (n_stage) {
      size_t rows = (size_t)(c->md.lds_x > c->md.lds_h ? c->md.lds_x : c->md.lds_h) / PK_WAVE;
      if ((size_t)c->md.lds_jc / PK_WAVE > rows) rows = (size_t)c->md.lds_jc / PK_WAVE;
      if ((size_t)c->md.big_rows > rows) rows = (size_t)c->md.big_rows;      // (big_global: lds_x is sized for ordinary tiles only)
      c->big_row = (kmax + 7) & ~7;
      const size_t slot = rows * (size_t)c->big_row;
      if (slot > (size_t)INT32_MAX) return fail(c, 33, "pk_set_problem: an interval with %d points is too long for the staging buffer", kmax);
      c->big_slot = (int32_t)slot;
      c->big_stage_doubles = slot * 4 * (size_t)n_stage;
      PK_HIP(c, hipMalloc((void**)&c->d_big_stage, sizeof(double) * c->big_stage_doubles));
    }
    if ((rc = upload(c, &c->d_tiles, tiles.data(), sizeof(PkTile) * tiles.size()))) return rc;
  }
  if ((rc = upload(c, &c->d_kinds, pd->kinds, sizeof(PkKind) * (size_t)pd->n_kinds))) return rc;
  if ((rc = upload(c, &c->d_items_jac, pd->items_jac, sizeof(PkItem) * (size_t)pd->n_items_jac))) return rc;
  if ((rc = upload(c, &c->d_items_hess, pd->items_hess, sizeof(PkItem) * (size_t)pd->n_items_hess))) return rc;
  if ((rc = upload(c, &c->d_items_aux, pd->items_aux, sizeof(PkItem) * (size_t)pd->n_items_aux))) return rc;
  if ((rc = upload(c, &c->d_outer, pd->outer, sizeof(PkOuter) * (size_t)pd->n_outer))) return rc;
  if ((rc = upload(c, &c->d_items_hessc, pd->items_hessc, sizeof(PkItem) * (size_t)pd->n_items_hessc))) return rc;
  if ((rc = upload(c, &c->d_items_jacc, pd->items_jacc, sizeof(PkItem) * (size_t)pd->n_items_jacc))) return rc;
  if ((rc = upload(c, (void**)&c->d_ib, pd->ib, sizeof(int32_t) * (size_t)pd->n_ib))) return rc;
  if ((rc = upload(c, (void**)&c->d_db, pd->db, sizeof(double) * (size_t)pd->n_db))) return rc;
  if ((rc = upload(c, (void**)&c->d_lb, pd->lb, sizeof(int64_t) * (size_t)pd->n_lb))) return rc;
  auto dalloc = [&](double** p, size_t count) -> int {
    PK_HIP(c, hipMalloc((void**)p, sizeof(double) * (count ? count : 1)));
    PK_HIP(c, hipMemset(*p, 0, sizeof(double) * (count ? count : 1)));
    return 0;
  };
  // J, grad f and g of the host shim share ONE allocation in this order, on the device and in pinned host memory: the
  // pieces of J that change with x, grad f and g then leave in one DMA (every extra DMA costs ~10 us on this link)
  if ((rc = dalloc(&c->d_x, c->n)) || (rc = dalloc(&c->d_lam, c->m)) || (rc = dalloc(&c->d_f, 1)) ||
      (rc = dalloc(&c->d_J, (size_t)c->nnz_J + (size_t)c->n + (size_t)c->m)) ||
      (rc = dalloc(&c->d_H, (size_t)c->nnz_H)) || (rc = dalloc(&c->d_aux, (size_t)c->n_aux)) || (rc = dalloc(&c->d_Hc, (size_t)c->nnz_Hc)) || (rc = dalloc(&c->d_Jc, (size_t)c->nnz_Jc)) || (rc = dalloc(&c->d_I, c->md.n_I)) ||
      (rc = dalloc(&c->d_partial, (2 * (size_t)c->n_tiles / PK_WAVES_PER_BLOCK + 2) * (size_t)c->md.nred)) ||
      (rc = dalloc(&c->d_partial2, (2 * (size_t)c->n_tiles / PK_WAVES_PER_BLOCK + 2) * (size_t)c->md.nred)))
    return rc;
  c->has_big = false;
  {
    const PkTile* tl = (const PkTile*)pd->tiles;
    for (int32_t t = 0; t < pd->n_tiles; ++t)
      if (tl[t].nj > 0 && tl[t].K > PK_WAVE) {
        c->has_big = true;
        if (t % PK_WAVES_PER_BLOCK || tl[t].nj != 1)
          return fail(c, 33, "pk_set_problem: tile %d: an interval with more than %d points must be alone in the first slot of a tile block", t, PK_WAVE);
        for (int32_t u = 1; u < PK_WAVES_PER_BLOCK && t + u < pd->n_tiles; ++u)
          if (tl[t + u].nj != 0) return fail(c, 33, "pk_set_problem: tile %d shares a block with a big interval", t + u);
      }
  }
  c->d_grad = c->d_J + c->nnz_J;
  c->d_g = c->d_grad + c->n;
  {   // hand-off slots of pk_cycle: one per x-kernel workgroup and reduction row, PK_EMPTY between launches
    const size_t slots = (2 * (size_t)c->n_tiles / PK_WAVES_PER_BLOCK + 2) * (size_t)c->md.nred;
    const std::vector<unsigned long long> empty(slots, (unsigned long long)PK_EMPTY);
    if ((rc = upload(c, (void**)&c->d_cpart, empty.data(), sizeof(unsigned long long) * slots))) return rc;
    if ((rc = upload(c, (void**)&c->d_cpart2, empty.data(), sizeof(unsigned long long) * slots))) return rc;
    c->cpart_slots = slots;
  }
  if ((rc = alloc_shim(c))) return rc;
  auto keep = [](std::vector<int32_t>& v, const int32_t* src, int64_t cnt) {
    v.clear();
    if (src) v.assign(src, src + cnt);
  };
  keep(c->jac_row, pd->jac_row, pd->nnz_J); keep(c->jac_col, pd->jac_col, pd->nnz_J);
  keep(c->hess_row, pd->hess_row, pd->nnz_H); keep(c->hess_col, pd->hess_col, pd->nnz_H);
  c->have_problem = true;
  return 0;
}

int pk_get_structure(pk_ctx* c, int32_t* jr, int32_t* jc, int32_t* hr, int32_t* hc) {
  int rc = ready(c);
  if (rc) return rc;
  if (c->jac_row.empty() && c->nnz_J) return fail(c, 40, "pk_get_structure: no structure was supplied to pk_set_problem");
  if (jr) std::memcpy(jr, c->jac_row.data(), sizeof(int32_t) * c->jac_row.size());
  if (jc) std::memcpy(jc, c->jac_col.data(), sizeof(int32_t) * c->jac_col.size());
  if (hr) std::memcpy(hr, c->hess_row.data(), sizeof(int32_t) * c->hess_row.size());
  if (hc) std::memcpy(hc, c->hess_col.data(), sizeof(int32_t) * c->hess_col.size());
  return 0;
}

// ---------------------------------------------------------------- device-pointer API
int pk_eval_f_dev(pk_ctx* c, const double* d_x, double* d_f, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  return prepass(c, d_x, nullptr, 0.0, d_f, true, pick(c, stream));
}

int pk_eval_grad_dev(pk_ctx* c, const double* d_x, double* d_grad, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (c->has_big) return eval_one_via_xpart(c, d_x, 1, d_grad, stream);
  hipStream_t st = pick(c, stream);
  if ((rc = prepass_if(c, c->md.prepass_grad, d_x, nullptr, 0.0, st))) return rc;
  PkArgs A = base_args(c, d_x, nullptr, 0.0);
  A.o_grad = d_grad;
  if ((rc = launch(c, K_GRAD, A, st))) return rc;
  A.flags |= F_FIN_GRAD;
  return launch(c, K_FIN, A, st);
}

int pk_eval_g_dev(pk_ctx* c, const double* d_x, double* d_g, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (c->has_big) return eval_one_via_xpart(c, d_x, 2, d_g, stream);
  hipStream_t st = pick(c, stream);
  if ((rc = prepass_if(c, c->md.prepass_g, d_x, nullptr, 0.0, st))) return rc;
  PkArgs A = base_args(c, d_x, nullptr, 0.0);
  A.o_g = d_g;
  return launch(c, K_G, A, st);
}

int pk_eval_jac_dev(pk_ctx* c, const double* d_x, double* d_vals, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (c->has_big) return eval_one_via_xpart(c, d_x, 3, d_vals, stream);
  hipStream_t st = pick(c, stream);
  if ((rc = prepass_if(c, c->md.prepass_jac, d_x, nullptr, 0.0, st))) return rc;
  PkArgs A = base_args(c, d_x, nullptr, 0.0);
  A.o_jac = d_vals;
  A.items = (const PkItem*)c->d_items_jac;
  A.n_items = c->n_items_jac;
  return launch(c, K_JAC, A, st);
}

int pk_eval_hess_dev(pk_ctx* c, const double* d_x, const double* d_lam, double sigma, double* d_vals, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (!d_lam) return fail(c, 50, "pk_eval_hess: lambda is required");
  hipStream_t st = pick(c, stream);
  if ((rc = prepass_if(c, c->md.prepass_hess, d_x, d_lam, sigma, st))) return rc;
  PkArgs A = base_args(c, d_x, d_lam, sigma);
  A.o_hess = d_vals;
  A.items = (const PkItem*)c->d_items_hess;
  A.n_items = c->n_items_hess;
  if ((rc = launch(c, K_HESS, A, st))) return rc;
  if (c->n_outer > 0) {   // objective / system constraints nonlinear in the integrals: outer-product blocks
    PkArgs X = base_args(c, d_x, d_lam, sigma);
    X.o_hess = d_vals;
    X.items = (const PkItem*)c->d_items_aux;
    X.n_items = c->n_items_aux;
    if ((rc = launch(c, K_AUX, X, st))) return rc;
    // a shard stops here: its auxiliary buffer holds the entries of ITS nodes, the caller sums the buffers over the
    // ranks and has the primary rank form the blocks (pk_eval_outer_dev)
    if (c->shard.external_prepass) return 0;
    return launch(c, K_OUTER, X, st);
  }
  return 0;
}

// compact (coalesced) Hessian of the Lagrangian: one value per distinct (row, col) class of a node
int pk_eval_hessc_dev(pk_ctx* c, const double* d_x, const double* d_lam, double sigma, double* d_vals, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (!d_lam) return fail(c, 50, "pk_eval_hessc: lambda is required");
  if (c->nnz_Hc <= 0) return fail(c, 51, "pk_eval_hessc: no compact Hessian layout was supplied to pk_set_problem");
  hipStream_t st = pick(c, stream);
  if ((rc = prepass_if(c, c->md.prepass_hess, d_x, d_lam, sigma, st))) return rc;
  PkArgs A = base_args(c, d_x, d_lam, sigma);
  A.o_hess = d_vals;
  A.items = (const PkItem*)c->d_items_hessc;
  A.n_items = c->n_items_hessc;
  return launch(c, K_HESSC, A, st);
}

// compact (coalesced) Jacobian: dense-column entries of the dynamics contracted with the integration block first
int pk_eval_jacc_dev(pk_ctx* c, const double* d_x, double* d_vals, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (c->nnz_Jc <= 0) return fail(c, 52, "pk_eval_jacc: no compact Jacobian layout was supplied to pk_set_problem");
  hipStream_t st = pick(c, stream);
  if ((rc = prepass_if(c, c->md.prepass_jac, d_x, nullptr, 0.0, st))) return rc;
  PkArgs A = base_args(c, d_x, nullptr, 0.0);
  A.o_jac = d_vals;
  A.items = (const PkItem*)c->d_items_jacc;
  A.n_items = c->n_items_jacc;
  return launch(c, K_JACC, A, st);
}

int pk_eval_jacc(pk_ctx* c, const double* x, double* vals) {
  const int rc = host_ready(c, x && vals);
  return rc ? rc : host_eval(c, x, nullptr, {{vals, c->d_Jc, (size_t)c->nnz_Jc}}, false, [&] { return pk_eval_jacc_dev(c, c->d_x, c->d_Jc, nullptr); });
}

int pk_eval_hessc(pk_ctx* c, const double* x, const double* lambda, double sigma, double* vals) {
  const int rc = host_ready(c, x && lambda && vals);
  return rc ? rc : host_eval(c, x, lambda, {{vals, c->d_Hc, (size_t)c->nnz_Hc}}, false, [&] { return pk_eval_hessc_dev(c, c->d_x, c->d_lam, sigma, c->d_Hc, nullptr); });
}

int pk_eval_cycle_dev(pk_ctx* c, const double* d_x, const double* d_lam, double sigma, double* d_f, double* d_grad,
                      double* d_g, double* d_jac, double* d_hess, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (!d_lam) return fail(c, 50, "pk_eval_cycle: lambda is required");
  hipStream_t st = pick(c, stream);
  const bool needs_I = c->md.prepass_grad || c->md.prepass_g || c->md.prepass_jac || c->md.prepass_hess || c->separate_x;
  // general path: the five callbacks one after the other.  A shard (pk_set_shard) may take the single launch too: its
  // finalize workgroup then leaves THIS shard's share of the integrals and of the shared gradient slots for the
  // caller's all-reduce, and f is the caller's to recompute (pk_eval_f_from_integrals_dev).
  if (c->cycle_layout && (needs_I || c->has_big || c->cycle_mode != 1))
    return fail(c, 69, "pk_eval_cycle: the compact layouts ride in the single-launch cycle only");
  if (needs_I && c->has_big) {       // (big intervals: the fused x-kernel behind the integral prepass, then H)
    if ((rc = pk_eval_xpart_dev(c, d_x, d_f, d_grad, d_g, d_jac, stream))) return rc;
    return pk_eval_hess_dev(c, d_x, d_lam, sigma, d_hess, stream);
  }
  if (needs_I || ((c->shard.external_prepass || c->shard.flags) && c->cycle_mode != 1)) {
    if (!c->shard.external_prepass && (rc = pk_eval_f_dev(c, d_x, d_f, stream))) return rc;
    if ((rc = pk_eval_grad_dev(c, d_x, d_grad, stream))) return rc;
    if ((rc = pk_eval_g_dev(c, d_x, d_g, stream))) return rc;
    if ((rc = pk_eval_jac_dev(c, d_x, d_jac, stream))) return rc;
    return pk_eval_hess_dev(c, d_x, d_lam, sigma, d_hess, stream);
  }
  // fused path: every x-only output from one evaluation of each node, then H (whose boundary workgroup also
  // performs the reductions).  With pk_set_cycle_graph the two launches are replayed from a cached hipGraph as
  // long as the pointers, sigma and the stream stay the same (an NLP solver's steady state).
  const PkCycleKey key{d_x, d_lam, d_f, d_grad, d_g, d_jac, d_hess, sigma, st};
  // (a sharded cycle replays too: its exchange counts the cycles in device memory, and every pk_set_* call that changes
  //  a launch argument -- shard flags, shared-slot target, integral buffer, exchange form -- drops the captured graph)
  const bool graph = c->graph.use && c->profile.mask == 0;
  if (graph && c->graph.cyc_exec && c->graph.cyc_key == key) {
    PK_HIP(c, hipGraphLaunch(c->graph.cyc_exec, st));
    return 0;
  }
  if (graph) {
    drop_cycle_graph(c);
    PK_HIP(c, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  }
  rc = enqueue_fused_cycle(c, d_x, d_lam, sigma, d_f, d_grad, d_g, d_jac, d_hess, st);
  if (!graph) return rc;
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(st, &g);
  if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
  if (e != hipSuccess) return fail(c, 3, "pk_eval_cycle: graph capture failed: %s", hipGetErrorString(e));
  e = hipGraphInstantiate(&c->graph.cyc_exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) { c->graph.cyc_exec = nullptr; return fail(c, 3, "pk_eval_cycle: graph instantiation failed: %s", hipGetErrorString(e)); }
  c->graph.cyc_key = key;
  PK_HIP(c, hipGraphLaunch(c->graph.cyc_exec, st));
  return 0;
}

// `count` back-to-back cycles on the same buffers, enqueued from here (a solver written against the C ABI launches from
// compiled code; bench.py's timed batches use this so that a Python loop does not pace the stream).  xchg = 1: every cycle
// is followed by pk_exchange_sums_dev(d_x, d_xgrad, d_f) -- the two-launch form of a sharded cycle.
int pk_eval_cycle_dev_repeat(pk_ctx* c, const double* d_x, const double* d_lam, double sigma, double* d_f, double* d_grad,
                             double* d_g, double* d_jac, double* d_hess, void* stream, int count, int xchg, double* d_xgrad) {
  int rc = ready(c);
  if (rc) return rc;
  if (count < 0 || (xchg && !d_xgrad)) return fail(c, 50, "pk_eval_cycle_dev_repeat: bad count, or xchg without the gradient buffer of the exchange");
  // pk_set_cycle_graph(1): the whole batch is ONE hipGraph of `count` kernel nodes, captured once and replayed while
  // pointers, sigma, stream and count stay the same -- the host then pays one graph launch per batch instead of `count`
  // kernel launches.  Sharded cycles with the in-launch exchange included (the cycle number lives in device memory).
  const bool needs_I = c->md.prepass_grad || c->md.prepass_g || c->md.prepass_jac || c->md.prepass_hess || c->separate_x;
  const bool graph = c->graph.use && c->profile.mask == 0 && !xchg && !needs_I && count > 1 && c->cycle_mode == 1 &&
                     !c->shard.external_prepass && d_lam;
  if (graph) {
    hipStream_t st = pick(c, stream);
    const PkCycleKey key{d_x, d_lam, d_f, d_grad, d_g, d_jac, d_hess, sigma, st};
    if (!(c->graph.rep_exec && c->graph.rep_key == key && c->graph.rep_count == count)) {
      if (c->graph.rep_exec) { (void)hipGraphExecDestroy(c->graph.rep_exec); c->graph.rep_exec = nullptr; }
      PK_HIP(c, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
      for (int k = 0; k < count && !rc; ++k) rc = enqueue_single_launch_cycle(c, d_x, d_lam, sigma, d_f, d_grad, d_g, d_jac, d_hess, st);
      hipGraph_t g = nullptr;
      hipError_t e = hipStreamEndCapture(st, &g);
      if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
      if (e != hipSuccess) return fail(c, 3, "pk_eval_cycle_dev_repeat: graph capture failed: %s", hipGetErrorString(e));
      e = hipGraphInstantiate(&c->graph.rep_exec, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      if (e != hipSuccess) { c->graph.rep_exec = nullptr; return fail(c, 3, "pk_eval_cycle_dev_repeat: graph instantiation failed: %s", hipGetErrorString(e)); }
      c->graph.rep_key = key;
      c->graph.rep_count = count;
    }
    PK_HIP(c, hipGraphLaunch(c->graph.rep_exec, st));
    return 0;
  }
  for (int k = 0; k < count; ++k) {
    rc = pk_eval_cycle_dev(c, d_x, d_lam, sigma, d_f, d_grad, d_g, d_jac, d_hess, stream);
    if (!rc && xchg) rc = pk_exchange_sums_dev(c, d_x, d_xgrad, d_f, 0, 1, stream);
    if (rc) return rc;
  }
  return 0;
}

// The four x-only outputs (f, grad f, g, J) of one iterate on device pointers: the fused x-kernel (every node evaluated
// once, one joint CSE) + the one-workgroup reduction -- what a line search's trial point needs, and what the host shim
// runs on a new x.  A shard (pk_set_shard) leaves ITS share of the integrals in the integral buffer and its partial sums
// in the shared gradient slots; its f is not meaningful (the caller adds the integrals over the shards first).  Models
// whose system functions are nonlinear in the integrals run the callbacks one after the other.
int pk_eval_xpart_dev(pk_ctx* c, const double* d_x, double* d_f, double* d_grad, double* d_g, double* d_jac, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  hipStream_t st = pick(c, stream);
  const bool needs_I = c->md.prepass_grad || c->md.prepass_g || c->md.prepass_jac || c->md.prepass_hess || c->separate_x;
  if (needs_I && !c->has_big) {
    if (!c->shard.external_prepass && (rc = pk_eval_f_dev(c, d_x, d_f, stream))) return rc;
    if ((rc = pk_eval_grad_dev(c, d_x, d_grad, stream))) return rc;
    if ((rc = pk_eval_g_dev(c, d_x, d_g, stream))) return rc;
    return pk_eval_jac_dev(c, d_x, d_jac, stream);
  }
  // (a mesh with intervals of more than 64 points has the fused x-kernel only: the integrals it needs come from the
  //  integral prepass in front of it)
  if (needs_I && !c->shard.external_prepass && (rc = prepass(c, d_x, nullptr, 0.0, d_f, true, st))) return rc;
  // ONE launch instead of pk_xall + pk_fin: pk_cycle's grid without its Hessian role -- the partial sums reach the finalize
  // workgroup inside the launch (host shim at 12k nodes: f is in pinned memory ~5 us earlier, and so is everything behind it)
  // (a shard takes it too, like pk_eval_cycle_dev: its finalize workgroup leaves THIS shard's share of the integrals and of
  //  the shared gradient slots for the caller to add up; never with the in-launch exchange, which belongs to whole cycles)
  if (xpart_is_one_launch(c))
    return enqueue_single_launch_cycle(c, d_x, nullptr, 0.0, d_f, d_grad, d_g, d_jac, nullptr, st, 0);
  PkArgs A = base_args(c, d_x, nullptr, 0.0);
  A.o_f = d_f; A.o_grad = d_grad; A.o_g = d_g; A.o_jac = d_jac;
  A.items = (const PkItem*)c->d_items_jac;
  A.n_items = c->n_items_jac;
  A.flags |= (c->split_xall ? F_SPLIT : 0);
  if ((rc = launch(c, K_XALL, A, st))) return rc;
  // (a shard of a model nonlinear in the integrals: the caller has summed the integrals over the ranks, they stay as they are)
  A.flags |= ((needs_I && c->shard.external_prepass) ? 0 : (F_FIN_INT | F_WRITE_F)) | F_FIN_GRAD;
  return launch(c, K_FIN, A, st);
}

// Which layouts pk_eval_cycle_dev writes into d_jac / d_hess: 0 the reference's triplets (default), 1 the compact layout
// (nnz_Jc / nnz_Hc values, the structures of pk_set_problem).  The compact layouts ride in the SAME single launch: the
// Jacobian role runs pk_jacc's tile code, the Hessian workgroups pk_hessc's -- a compact cycle is one launch too.
int pk_set_cycle_layout(pk_ctx* c, int jac_compact, int hess_compact) {
  int rc = ready(c);
  if (rc) return rc;
  if (jac_compact && c->nnz_Jc <= 0) return fail(c, 52, "pk_set_cycle_layout: no compact Jacobian layout was supplied to pk_set_problem");
  if (hess_compact && c->nnz_Hc <= 0) return fail(c, 51, "pk_set_cycle_layout: no compact Hessian layout was supplied to pk_set_problem");
  const bool needs_I = c->md.prepass_grad || c->md.prepass_g || c->md.prepass_jac || c->md.prepass_hess || c->separate_x;
  if ((jac_compact || hess_compact) && (needs_I || c->has_big))
    return fail(c, 69, "pk_set_cycle_layout: the compact layouts ride in the single-launch cycle, which this model / mesh does not "
                       "use (system functions nonlinear in the integrals, or an interval with more than 64 points)");
  c->cycle_layout = (jac_compact ? 1 : 0) | (hess_compact ? 2 : 0);
  drop_cycle_graph(c);
  if (c->graph.rep_exec) { (void)hipGraphExecDestroy(c->graph.rep_exec); c->graph.rep_exec = nullptr; }
  return 0;
}

// 1 (default): the cycle is ONE launch (pk_cycle); 0: two launches (pk_xall, then pk_hess with the reductions)
int pk_set_cycle_mode(pk_ctx* c, int single_launch) {
  if (!c) return fail(nullptr, 1, "null context");
  c->cycle_mode = single_launch ? 1 : 0;
  drop_cycle_graph(c);
  return 0;
}

int pk_set_cycle_graph(pk_ctx* c, int enable) {
  if (!c) return fail(nullptr, 1, "null context");
  c->graph.use = enable != 0;
  if (!c->graph.use) drop_cycle_graph(c);
  return 0;
}

int pk_sync(pk_ctx* c, void* stream) {
  if (!c) return fail(nullptr, 1, "null context");
  PK_HIP(c, hipStreamSynchronize(pick(c, stream)));
  return handoff_check(c);
}

// the same by polling the stream's state: the host learns ~8 us earlier than through hipStreamSynchronize that a copy has
// landed (tools/dma_probe.cpp); for callers on a latency path (the host-landed sharded cycle)
int pk_wait_idle(pk_ctx* c, void* stream) {
  if (!c) return fail(nullptr, 1, "null context");
  hipStream_t st = pick(c, stream);
  hipError_t e;
  while ((e = hipStreamQuery(st)) == hipErrorNotReady) { }
  if (e != hipSuccess) return fail(c, 100 + (int)e, "hipStreamQuery failed: %s", hipGetErrorString(e));
  return handoff_check(c);
}

// ---------------------------------------------------------------- host-buffer API
int pk_eval_f(pk_ctx* c, const double* x, double* f) {
  const int rc = host_ready(c, x && f);
  return rc ? rc : host_eval(c, x, nullptr, {{f, c->d_f, 1}}, true, [&] { return pk_eval_f_dev(c, c->d_x, c->d_f, nullptr); });
}

int pk_eval_grad(pk_ctx* c, const double* x, double* grad) {
  const int rc = host_ready(c, x && grad);
  return rc ? rc : host_eval(c, x, nullptr, {{grad, c->d_grad, (size_t)c->n}}, true, [&] { return pk_eval_grad_dev(c, c->d_x, c->d_grad, nullptr); });
}

int pk_eval_g(pk_ctx* c, const double* x, double* g) {
  const int rc = host_ready(c, x && g);
  return rc ? rc : host_eval(c, x, nullptr, {{g, c->d_g, (size_t)c->m}}, true, [&] { return pk_eval_g_dev(c, c->d_x, c->d_g, nullptr); });
}

int pk_eval_jac(pk_ctx* c, const double* x, double* vals) {
  const int rc = host_ready(c, x && vals);
  return rc ? rc : host_eval(c, x, nullptr, {{vals, c->d_J, (size_t)c->nnz_J}}, true, [&] { return pk_eval_jac_dev(c, c->d_x, c->d_J, nullptr); });
}

int pk_eval_hess(pk_ctx* c, const double* x, const double* lambda, double sigma, double* vals) {
  if (c && !lambda) return fail(c, 50, "pk_eval_hess: lambda is required");
  const int rc = host_ready(c, x && vals);
  return rc ? rc : host_eval(c, x, lambda, {{vals, c->d_H, (size_t)c->nnz_H}}, true, [&] { return pk_eval_hess_dev(c, c->d_x, c->d_lam, sigma, c->d_H, nullptr); });
}

int pk_eval_cycle(pk_ctx* c, const double* x, const double* lambda, double sigma, double* f, double* grad, double* g,
                  double* jac, double* hess) {
  if (const int rc = host_ready(c, x && lambda && f && grad && g && jac && hess)) return rc;
  return host_eval(c, x, lambda, {{f, c->d_f, 1}, {grad, c->d_grad, (size_t)c->n}, {g, c->d_g, (size_t)c->m},
                                  {jac, c->d_J, (size_t)c->nnz_J}, {hess, c->d_H, (size_t)c->nnz_H}}, true,
                   [&] { return pk_eval_cycle_dev(c, c->d_x, c->d_lam, sigma, c->d_f, c->d_grad, c->d_g, c->d_J, c->d_H, nullptr); },
                   /*staged=*/true);
}

}  // extern "C"
