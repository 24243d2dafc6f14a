// pk_shard.cpp -- mesh-interval sharding across GPUs: the shard switches of a context, the split callbacks around the
// caller's reductions, peer / IPC / registered memory of the mailboxes, the exchange of the partial sums, run copies and
// progress marks (pockit_hip_internal.h, "Sharding").
#include "pk_runtime.h"

extern "C" {

// sharded mode, step 1: this shard's contribution to every integral -> integral buffer
int pk_eval_integrals_dev(pk_ctx* c, const double* d_x, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  return prepass(c, d_x, nullptr, 0.0, c->d_f, false, pick(c, stream));
}

// sharded mode, step 2 (after the caller all-reduced the integral buffer): f = F_o(I, s)
int pk_eval_f_from_integrals_dev(pk_ctx* c, const double* d_x, double* d_f, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  PkArgs A = base_args(c, d_x, nullptr, 0.0);
  A.o_f = d_f;
  A.flags |= F_WRITE_F;
  return launch(c, K_FIN, A, pick(c, stream));
}

int pk_set_shard(pk_ctx* c, int secondary, int external_prepass, double* d_integrals) {
  if (!c) return fail(nullptr, 1, "null context");
  c->shard.flags = secondary ? F_SECONDARY : 0;
  c->shard.external_prepass = external_prepass != 0;
  c->shard.ext_I = d_integrals;
  drop_cycle_graph(c);            // (a captured cycle holds the old flags / integral buffer)
  return 0;
}

// sharded mode, models nonlinear in the integrals: the auxiliary buffer pk_eval_hess_dev fills on a shard (NULL / 0 for
// models without outer-product blocks) ...
int pk_aux_buffer(pk_ctx* c, double** ptr, int64_t* count) {
  int rc = ready(c);
  if (rc) return rc;
  if (ptr) *ptr = c->n_outer > 0 ? c->d_aux : nullptr;
  if (count) *count = c->n_outer > 0 ? (int64_t)c->n_aux : 0;
  return 0;
}

// ... and the outer-product blocks of the Hessian from the buffer summed over the ranks (d_aux_sum: n_aux doubles, device)
int pk_eval_outer_dev(pk_ctx* c, const double* d_aux_sum, double* d_vals, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (c->n_outer <= 0) return 0;
  if (!d_aux_sum || !d_vals) return fail(c, 50, "pk_eval_outer: null device buffer");
  PkArgs X = base_args(c, nullptr, nullptr, 0.0);
  X.o_hess = d_vals;
  X.o_aux = const_cast<double*>(d_aux_sum);
  return launch(c, K_OUTER, X, pick(c, stream));
}

// ---------------------------------------------------------------- sharded cycles: peer memory + the exchange of the sums
// Device memory of the caller's own (a mailbox, a reassembly buffer).  finegrained = 1: coherent with other GPUs and the
// host WHILE kernels run (flags polled across devices); 0: ordinary device memory.
int pk_device_alloc(pk_ctx* c, size_t bytes, int finegrained, void** out) {
  if (!c) return fail(nullptr, 1, "null context");
  if (!out) return fail(c, 60, "null output pointer");
  PK_HIP(c, hipSetDevice(c->device));
  if (finegrained) PK_HIP(c, hipExtMallocWithFlags(out, bytes ? bytes : 8, hipDeviceMallocFinegrained));
  else PK_HIP(c, hipMalloc(out, bytes ? bytes : 8));
  PK_HIP(c, hipMemset(*out, 0, bytes ? bytes : 8));
  PK_HIP(c, hipDeviceSynchronize());
  return 0;
}

int pk_device_free(pk_ctx* c, void* p) {
  if (!c) return fail(nullptr, 1, "null context");
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipDeviceSynchronize());
  if (p) PK_HIP(c, hipFree(p));
  return 0;
}

// Inter-process handle (64 bytes) of a pk_device_alloc allocation, and its mapping in another process (one per GPU).
int pk_ipc_export(pk_ctx* c, void* dptr, void* handle64) {
  if (!c) return fail(nullptr, 1, "null context");
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "handle size of the C ABI");
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipIpcGetMemHandle((hipIpcMemHandle_t*)handle64, dptr));
  return 0;
}

int pk_ipc_open(pk_ctx* c, const void* handle64, void** out) {
  if (!c) return fail(nullptr, 1, "null context");
  hipIpcMemHandle_t h;
  std::memcpy(&h, handle64, sizeof h);
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipIpcOpenMemHandle(out, h, hipIpcMemLazyEnablePeerAccess));
  return 0;
}

int pk_ipc_close(pk_ctx* c, void* p) {
  if (!c) return fail(nullptr, 1, "null context");
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipDeviceSynchronize());
  PK_HIP(c, hipIpcCloseMemHandle(p));
  return 0;
}

// Host memory of the caller's own (e.g. a shared-memory segment several processes map) made a DMA / kernel target:
// page-locks [p, p + bytes) and returns the address the device sees it at.  pk_host_unregister before it is unmapped.
int pk_host_register(pk_ctx* c, void* p, size_t bytes, void** dev_ptr) {
  if (!c) return fail(nullptr, 1, "null context");
  if (!p || !bytes || !dev_ptr) return fail(c, 60, "null host buffer");
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipHostRegister(p, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
  PK_HIP(c, hipHostGetDevicePointer(dev_ptr, p, 0));
  return 0;
}

int pk_host_unregister(pk_ctx* c, void* p) {
  if (!c) return fail(nullptr, 1, "null context");
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipDeviceSynchronize());
  PK_HIP(c, hipHostUnregister(p));
  return 0;
}

// Asynchronous copy between any two addresses the device can see (device memory, registered / pinned host memory)
int pk_copy_dev(pk_ctx* c, void* dst, const void* src, size_t bytes, void* stream) {
  if (!c) return fail(nullptr, 1, "null context");
  if (!bytes) return 0;
  PK_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, pick(c, stream)));
  return 0;
}

// A shard whose gradient output is another GPU's buffer keeps the slots shared by all nodes (partial sums) local.
int pk_set_shared_grad_target(pk_ctx* c, double* d_grad_shared) {
  if (!c) return fail(nullptr, 1, "null context");
  c->shard.gshared = d_grad_shared;
  drop_cycle_graph(c);
  return 0;
}

// d_boxes: device array of `world` pointers, entry r = rank r's mailbox as mapped in this process; d_idx: device array
// of the NLP indices of the n_sh shared gradient slots; stride: words per sender slot (>= 1 + n_I + n_sh).
int pk_set_exchange(pk_ctx* c, int world, int rank, const void* d_boxes, const int32_t* d_idx, int n_sh, int stride) {
  int rc = ready(c);
  if (rc) return rc;
  // everything is checked before anything is stored: a refused call leaves the context as it was
  if (world < 1 || world > PK_MAX_RANKS || rank < 0 || rank >= world)
    return fail(c, 90, "pk_set_exchange: %d ranks (at most %d), rank %d", world, PK_MAX_RANKS, rank);
  if (c->md.n_I + n_sh > 512 || stride < 1 + c->md.n_I + n_sh)
    return fail(c, 91, "pk_set_exchange: partial vector of %d doubles (at most 512), slot of %d words", c->md.n_I + n_sh, stride);
  if (n_sh != c->n_gz) return fail(c, 94, "pk_set_exchange: %d shared gradient slots, the problem has %d", n_sh, c->n_gz);
  if (!d_boxes) return fail(c, 93, "pk_set_exchange: no mailbox table");
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  std::vector<unsigned long long*> boxes((size_t)world, nullptr);
  PK_HIP(c, hipMemcpy(boxes.data(), d_boxes, sizeof(void*) * (size_t)world, hipMemcpyDeviceToHost));
  if (!boxes[(size_t)rank]) return fail(c, 93, "pk_set_exchange: this rank's own mailbox is missing from the table");
  // this rank's mailbox starts empty and its cycle count at zero (stale flags of an earlier set-up cannot match: every rank
  // resets here, and the caller's barrier behind the set-up comes before the first flag is raised)
  const size_t words = 2 * (size_t)world * (size_t)stride + PK_XC_STATE;
  PK_HIP(c, hipMemset(boxes[(size_t)rank], 0, sizeof(unsigned long long) * words));
  PK_HIP(c, hipDeviceSynchronize());
  c->exchange.box = (const unsigned long long* const*)d_boxes;
  c->exchange.own = boxes[(size_t)rank];
  c->exchange.idx = d_idx;
  c->exchange.world = world; c->exchange.rank = rank; c->exchange.nsh = n_sh; c->exchange.stride = stride;
  drop_cycle_graph(c);
  return 0;
}

// cycles exchanged so far and how many of them gave up waiting for a peer (their sums read NaN on THIS rank, while a late
// peer still got finite ones: a caller checks this before it trusts f across the ranks).  Synchronizes the stream.
int pk_exchange_status(pk_ctx* c, void* stream, int64_t* cycles, int64_t* timed_out) {
  int rc = ready(c);
  if (rc) return rc;
  if (!c->exchange.own) return fail(c, 92, "pk_exchange_status: call pk_set_exchange first");
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipStreamSynchronize(pick(c, stream)));
  unsigned long long st[2] = {0, 0};
  PK_HIP(c, hipMemcpy(st, c->exchange.own + 2 * (size_t)c->exchange.world * (size_t)c->exchange.stride, sizeof st, hipMemcpyDeviceToHost));
  if (cycles) *cycles = (int64_t)st[0];
  if (timed_out) *timed_out = (int64_t)st[1];
  return 0;
}

// 1: pk_eval_cycle_dev's single launch exchanges the partial sums itself (its finalize workgroup posts, waits and adds:
// a sharded cycle is ONE launch per GPU); 0: the caller runs pk_exchange_sums_dev behind it (a second launch).
int pk_set_exchange_inline(pk_ctx* c, int enable) {
  if (!c) return fail(nullptr, 1, "null context");
  if (enable && !c->exchange.box) return fail(c, 92, "pk_set_exchange_inline: call pk_set_exchange first");
  if (enable && !c->md.sharded)
    return fail(c, 95, "pk_set_exchange_inline: the code object was generated for a single GPU (no exchange code in pk_cycle)");
  c->exchange.in_launch = enable != 0;
  drop_cycle_graph(c);
  return 0;
}

// After the shard's pk_eval_cycle_dev on the same stream: post this rank's partial sums to every peer, take theirs, leave
// the global integrals, the summed shared gradient slots (in d_grad, or the shared-slot target) and -- write_f -- f.
int pk_exchange_sums_dev(pk_ctx* c, const double* d_x, double* d_grad, double* d_f, int epoch, int write_f, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (!c->exchange.box) return fail(c, 92, "pk_exchange_sums: call pk_set_exchange first");
  if (epoch < 0) epoch = 0;                   // (0: the exchange counts the cycles itself, in device memory)
  PkArgs A = base_args(c, d_x, nullptr, 0.0);
  A.o_grad = d_grad; A.o_f = d_f;
  A.xc_box = (unsigned long long* const*)c->exchange.box; A.xc_idx = c->exchange.idx;
  A.xc_world = c->exchange.world; A.xc_rank = c->exchange.rank; A.xc_epoch = epoch; A.xc_nsh = c->exchange.nsh; A.xc_stride = c->exchange.stride;
  A.flags = (A.flags & ~F_WRITE_F) | (write_f ? F_WRITE_F : 0);
  return launch(c, K_XCHG, A, pick(c, stream));
}

// dst[dst_off + i] = src[src_off + i] over a device table of n_chunks (src_off, dst_off, len) int64 triples
int pk_copy_runs_dev(pk_ctx* c, const int64_t* d_table, int n_chunks, const double* d_src, double* d_dst, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (n_chunks <= 0) return 0;
  PkArgs A = base_args(c, nullptr, nullptr, 0.0);
  A.rc_table = d_table; A.rc_n = n_chunks; A.rc_src = d_src; A.rc_dst = d_dst;
  return launch(c, K_RUNS, A, pick(c, stream), n_chunks);
}

// *d_dst = value, in stream order (d_dst: device address of a 64-bit word, typically of a registered host segment)
int pk_store_word_dev(pk_ctx* c, void* d_dst, int64_t value, void* stream) {
  if (!c) return fail(nullptr, 1, "null context");
  if (!d_dst || ((uintptr_t)d_dst & 7)) return fail(c, 60, "pk_store_word: destination must be an 8-byte aligned device address");
  PK_HIP(c, hipSetDevice(c->device));
  return launch_store_word(c, (unsigned long long*)d_dst, (unsigned long long)value, pick(c, stream));
}

}  // extern "C"
