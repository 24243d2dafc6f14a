// pk_batch.cpp -- a batch of iterates in ONE launch of the fused cycle (pk_cycleb).
//
// A launch of pk_cycle costs a launch gap and a latency prefix whatever it computes; a caller that
// holds B iterates -- multi-start, a merit scan over trial points, a lock-step ensemble -- pays them once per batch here
// instead of once per iterate.  pk_cycleb is pk_cycle's body with blockIdx.y as the batch entry: the four preloaded scalars
// stay in the kernarg segment, the PkArgs of entry b is record b of a device array written ahead of the launch.
//
//   pk_load_batch_model      attaches the batched code object (codegen.ModelSource(plan, batched=True)) to the context
//   pk_set_batch             per-entry workspaces: integrals, partial sums, hand-off slots, auxiliary buffer, staging rows
//   pk_eval_cycle_batch_dev  records -> device (the caller's stream), then ONE launch with gridDim.y = B
//
// Nothing a launch writes is shared between its entries; the tables of the problem and the status words are.  A time-out
// of the hand-off in any entry is therefore error 97 for the whole call (handoff_check).  Contexts whose cycle is not the
// one-launch cycle (models that need the integrals first, separate_x, a shard, pk_set_cycle_mode(0), no batched object) are
// served by a loop of single cycles inside the same call: the same values, no speed claim.
#include "pk_runtime.h"

namespace {

bool needs_integrals_first(const pk_ctx* c) {
  return c->md.prepass_grad || c->md.prepass_g || c->md.prepass_jac || c->md.prepass_hess || c->separate_x;
}

// is a batch of this context ONE launch of pk_cycleb?  (x_only: the x-part alone, under pk_eval_xpart_dev's own conditions)
bool batch_is_one_launch(const pk_ctx* c, bool x_only) {
  if (!c->fn[K_CYCLEB] || c->cycle_mode != 1 || needs_integrals_first(c)) return false;
  if (c->shard.external_prepass || c->shard.flags || c->shard.ext_I || c->shard.gshared) return false;
  return x_only ? xpart_is_one_launch(c) : true;
}

}  // namespace

void free_batch(pk_ctx* c) {
  PkBatch& b = c->batch;
  release(b.d_ws); release(b.d_cp); release(b.d_big); release(b.d_args);
  if (b.h_args) (void)hipHostFree(b.h_args);
  b.h_args = nullptr;
  if (b.ev_copied) (void)hipEventDestroy(b.ev_copied);
  b.ev_copied = nullptr;
  b.copy_pending = false;
  b.B = b.cap = 0;
}

void unload_batch_model(pk_ctx* c) {
  if (c->batch.module) (void)hipModuleUnload(c->batch.module);
  c->batch.module = nullptr;
  c->fn[K_CYCLEB] = nullptr;
}

extern "C" {

// code_object == NULL (len 0): the batched object is dropped -- batches are then served by the loop of single cycles
int pk_load_batch_model(pk_ctx* c, const void* code_object, size_t len) {
  if (!c) return fail(nullptr, 1, "null context");
  if (!c->have_model) return fail(c, 2, "pk_load_batch_model: load the model first (pk_load_model)");
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  unload_batch_model(c);
  if (!code_object || len == 0) return 0;
  PK_HIP(c, hipModuleLoadData(&c->batch.module, code_object));
  if (hipModuleGetFunction(&c->fn[K_CYCLEB], c->batch.module, kKernelNames[K_CYCLEB]) != hipSuccess || !c->fn[K_CYCLEB]) {
    unload_batch_model(c);
    return fail(c, 86, "pk_load_batch_model: the code object has no kernel %s (generate it with batched=True)", kKernelNames[K_CYCLEB]);
  }
  return 0;
}

int pk_set_batch(pk_ctx* c, int B) {
  int rc = ready(c);
  if (rc) return rc;
  if (B < 1 || B > PK_MAX_BATCH) return fail(c, 87, "pk_set_batch: %d entries (1 ... %d)", B, PK_MAX_BATCH);
  PkBatch& b = c->batch;
  if (B <= b.cap) {      // (the workspaces of a larger batch serve a smaller one: every entry's slots are armed)
    b.B = B;
    return 0;
  }
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipDeviceSynchronize());      // (nothing may still run on the workspaces about to be replaced)
  free_batch(c);
  const size_t D = sizeof(double);
  b.n_partial = (2 * (size_t)c->n_tiles / PK_WAVES_PER_BLOCK + 2) * (size_t)c->md.nred;      // (= pk_set_problem's)
  const size_t n_I = (size_t)(c->md.n_I > 0 ? c->md.n_I : 1), n_aux = (size_t)(c->n_aux > 0 ? c->n_aux : 1);
  b.ws_stride = n_I + 2 * b.n_partial + n_aux;
  b.big_stride = c->big_stage_doubles;
  PK_HIP(c, hipMalloc((void**)&b.d_ws, D * b.ws_stride * (size_t)B));
  PK_HIP(c, hipMemset(b.d_ws, 0, D * b.ws_stride * (size_t)B));
  if (b.big_stride) PK_HIP(c, hipMalloc((void**)&b.d_big, D * b.big_stride * (size_t)B));
  {
    const std::vector<unsigned long long> empty(2 * b.n_partial * (size_t)B, (unsigned long long)PK_EMPTY);
    if ((rc = upload(c, (void**)&b.d_cp, empty.data(), sizeof(unsigned long long) * empty.size()))) return rc;
  }
  const size_t bytes = args_bytes(c) * (size_t)B;
  PK_HIP(c, hipMalloc((void**)&b.d_args, bytes));
  PK_HIP(c, hipHostMalloc((void**)&b.h_args, bytes, hipHostMallocDefault));
  PK_HIP(c, hipEventCreateWithFlags(&b.ev_copied, hipEventDisableTiming));
  b.B = b.cap = B;
  return 0;
}

int pk_eval_cycle_batch_dev(pk_ctx* c, int B, const double* d_x, int64_t ldx, const double* d_lam, int64_t ldlam,
                            const double* sigma, double* d_f, double* d_grad, double* d_g, double* d_jac, double* d_hess,
                            void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (B < 1 || B > PK_MAX_BATCH) return fail(c, 87, "pk_eval_cycle_batch: %d entries (1 ... %d)", B, PK_MAX_BATCH);
  if (!d_x || !d_f || !d_grad || !d_g || !d_jac || (d_lam && (!d_hess || !sigma)))
    return fail(c, 89, "pk_eval_cycle_batch: null pointer (only lambda, and with it sigma and the Hessian, may be NULL)");
  if (ldx < c->n || (d_lam && ldlam < c->m))
    return fail(c, 89, "pk_eval_cycle_batch: leading dimensions %lld / %lld of x / lambda (at least %d / %d)", (long long)ldx,
                (long long)ldlam, c->n, c->m);
  if (c->cycle_layout)
    return fail(c, 88, "pk_eval_cycle_batch: the compact layouts (pk_set_cycle_layout) are not offered for a batch");
  if (c->exchange.in_launch && c->exchange.world > 1)
    return fail(c, 88, "pk_eval_cycle_batch: a sharded context with the in-launch exchange is not offered for a batch");
  hipStream_t st = pick(c, stream);
  const size_t n = (size_t)c->n, m = (size_t)c->m, nj = (size_t)c->nnz_J, nh = (size_t)c->nnz_H;
  const bool x_only = d_lam == nullptr;
  if (!batch_is_one_launch(c, x_only)) {
    // the same values from B single cycles, one after the other on the caller's stream (the context's own workspaces)
    for (int e = 0; e < B; ++e) {
      const size_t u = (size_t)e;
      if (x_only) rc = pk_eval_xpart_dev(c, d_x + u * (size_t)ldx, d_f + u, d_grad + u * n, d_g + u * m, d_jac + u * nj, stream);
      else rc = pk_eval_cycle_dev(c, d_x + u * (size_t)ldx, d_lam + u * (size_t)ldlam, sigma[e], d_f + u, d_grad + u * n, d_g + u * m,
                                  d_jac + u * nj, d_hess + u * nh, stream);
      if (rc) return rc;
    }
    return 0;
  }
  PK_HIP(c, hipSetDevice(c->device));
  if (B > c->batch.cap) {
    if ((rc = pk_set_batch(c, B))) return rc;
  } else {
    c->batch.B = B;
  }
  PkBatch& b = c->batch;
  const size_t stride = args_bytes(c);      // (= sizeof(PkArgs) as the code object declares it: argv[b] on the device)
  const size_t bytes = stride * (size_t)B;
  // the records are written into pinned memory once the copy of the previous batch has left it
  if (b.copy_pending) {
    PK_HIP(c, hipEventSynchronize(b.ev_copied));
    b.copy_pending = false;
  }
  char* rec = b.h_args;
  int32_t flags = 0;
  for (int e = 0; e < B; ++e) {
    const size_t u = (size_t)e;
    PkArgs A = cycle_args(c, d_x + u * (size_t)ldx, x_only ? nullptr : d_lam + u * (size_t)ldlam, x_only ? 0.0 : sigma[e], d_f + u,
                          d_grad + u * n, d_g + u * m, d_jac + u * nj, x_only ? nullptr : d_hess + u * nh, 0);
    double* ws = b.d_ws + u * b.ws_stride;
    A.Ibuf = ws;
    A.partial = ws + (c->md.n_I > 0 ? c->md.n_I : 1);
    A.partial2 = A.partial + b.n_partial;
    A.o_aux = A.partial2 + b.n_partial;
    A.cpart = b.d_cp + u * 2 * b.n_partial;
    A.cpart2 = A.cpart + b.n_partial;
    A.big_stage = b.d_big ? b.d_big + u * b.big_stride : nullptr;
    A.trace = nullptr;      // (the developer trace holds the records of ONE cycle)
    flags = A.flags;
    std::memcpy(rec + u * stride, static_cast<const void*>(&A), stride);
  }
  PK_HIP(c, hipMemcpyAsync(b.d_args, rec, bytes, hipMemcpyHostToDevice, st));
  PK_HIP(c, hipEventRecord(b.ev_copied, st));
  b.copy_pending = true;
  // pk_cycleb's kernarg segment: pk_cycle's four leading scalars (the same for every entry), then the record array
  PkLaunchShape shape = shape_of(c, K_CYCLEB);
  shape.batch = (unsigned)B;
  struct BatchArgs {
    const PkTile* tile;
    int32_t n_tiles, flags, grid, pad;
    const void* argv;
  } K;
  static_assert(offsetof(BatchArgs, argv) == PK_CYCLE_ARGS_OFFSET, "pk_cycleb's leading kernel arguments are pk_cycle's");
  K.tile = (const PkTile*)c->d_tiles; K.n_tiles = c->n_tiles; K.flags = flags; K.grid = (int32_t)shape.grid; K.pad = 0;
  K.argv = b.d_args;
  if ((rc = launch_raw(c, K_CYCLEB, &K, sizeof K, shape, st))) return rc;
  ++b.launches;
  return 0;
}

int pk_batch_launches(pk_ctx* c, int64_t* launches) {
  if (!c || !launches) return fail(c, 1, "pk_batch_launches: null argument");
  *launches = c->batch.launches;
  return 0;
}

}  // extern "C"
