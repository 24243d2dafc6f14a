// pk_shim.cpp -- the host shim of the runtime: the "new x" protocol of a solver's callbacks (prepared x, landing blocks, copy
// batching, polling waits, speculative Hessian, constant Jacobian runs) and its A/B options; declared in pockit_hip_internal.h.
// Everything on the per-callback path is defined in this unit: the two copy / mark kernels,
// copy_async, stage_upload, enqueue_result_copies, the waits.  What it launches for an iterate are the core's entry points.
#include "pk_runtime.h"

// Copy kernel of the host shim: n doubles between pinned host memory and device memory, 16 bytes per lane.  src and dst
// are congruent modulo 16 bytes (the caller checks), so at most one leading and one trailing double go alone.
__global__ void __launch_bounds__(256) pk_copy_kernel(const double* __restrict__ src, double* __restrict__ dst, size_t n) {
  size_t head = ((uintptr_t)src >> 3) & 1;
  if (head > n) head = n;
  const size_t pairs = (n - head) >> 1;
  const double2* __restrict__ s2 = reinterpret_cast<const double2*>(src + head);
  double2* __restrict__ d2 = reinterpret_cast<double2*>(dst + head);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < pairs; i += (size_t)gridDim.x * blockDim.x) d2[i] = s2[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (head) dst[0] = src[0];
    if (head + 2 * pairs < n) dst[n - 1] = src[n - 1];
  }
}

// One 64-bit word stored behind everything enqueued before it on the stream (a progress mark in pinned host memory that
// the host, or another process mapping the same segment, polls: seen a few microseconds before an event would report).
__global__ void __launch_bounds__(64) pk_store_word_kernel(unsigned long long* dst, unsigned long long value) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *(volatile unsigned long long*)dst = value;
}

// dst[0 .. n) = src[0 .. n) on the context's stream: the copy kernel when asked for and possible, else the DMA engine
int copy_async(pk_ctx* c, double* dst, const double* src, size_t n, hipMemcpyKind kind, bool by_kernel) {
  if (!n) return 0;
  if (by_kernel && !(((uintptr_t)dst ^ (uintptr_t)src) & 8)) {
    // (tools/copy_kernel_probe.cpp: device -> host does not care about the grid, 49-50 GB/s from 32 to 2048 workgroups;
    //  host -> device prefers FEW workgroups: 0.77 MB 28 us with 64, 32 us with 1024; 4.8 MB 101 vs 123 us)
    const size_t pairs = n / 2 + 1;
    unsigned grid = (unsigned)((pairs + 255) / 256);
    const unsigned cap = kind == hipMemcpyHostToDevice ? 64u : 512u;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(pk_copy_kernel, dim3(grid), dim3(256), 0, c->stream, src, dst, n);
    PK_HIP(c, hipGetLastError());
    return 0;
  }
  PK_HIP(c, hipMemcpyAsync(dst, src, sizeof(double) * n, kind, c->stream));
  return 0;
}

namespace {

size_t result_count(const pk_ctx* c, int what) {
  const size_t cnt[5] = {1, (size_t)c->n, (size_t)c->m, (size_t)(c->shim.jac_compact ? c->nnz_Jc : c->nnz_J), (size_t)c->nnz_H};
  return cnt[what];
}

double* device_result(pk_ctx* c, int what) {
  double* src[5] = {c->d_f, c->d_grad, c->d_g, c->shim.jac_compact ? c->d_Jc : c->d_J, c->d_H};
  return src[what];
}

int enqueue_mark(pk_ctx* c) {
  if (!c->shim.mark_wait || !c->shim.spin_wait || !c->shim.res[0].h_out) return 0;
  unsigned long long* word = reinterpret_cast<unsigned long long*>(c->shim.res[0].h_out + 4);
  const unsigned long long value = ++c->shim.mark_val;      // (a copy: the launch takes its arguments by value, now)
  c->shim.mark_op_seq = c->shim.op_seq;
  hipStream_t st = c->stream;
  hipLaunchKernelGGL(pk_store_word_kernel, dim3(1), dim3(64), 0, st, word, value);
  PK_HIP(c, hipGetLastError());
  c->shim.mark_pending = true;
  return 0;
}

}  // namespace

// A hand-off that gave up waiting (pk_cycle's finalize workgroup for the partial sums of its own launch; the exchange of the
// sums between the ranks) leaves NaN in f and in the gradient entries shared by all nodes -- indistinguishable, for a solver,
// from a model that evaluates to NaN (which the reference passes on unchecked, examples/_plotting.py:58-63, and so do we).
// The kernels count such events in two status words in pinned memory (PkArgs.status); every waiting entry point compares
// them with what it saw last and turns a change into error 97: the hand-off slots are put back to PK_EMPTY (a publisher that
// arrived after the give-up left its value behind), the staged iterate is dropped, the message says what happened.
int handoff_check(pk_ctx* c) {
  if (!c->shim.res[0].h_out) return 0;
  const volatile unsigned long long* st = reinterpret_cast<const volatile unsigned long long*>(c->shim.res[0].h_out + 6);
  const unsigned long long a = st[0], b = st[1];
  if (a == c->shim.status_seen[0] && b == c->shim.status_seen[1]) return 0;
  const unsigned long long da = a - c->shim.status_seen[0], db = b - c->shim.status_seen[1];
  // (rare path: the device, not only the context's stream -- pk_sync / pk_wait_idle come here for a caller's stream too, and
  //  cycles still in flight on it must not race with the reset of the hand-off slots below)
  (void)hipDeviceSynchronize();
  if (c->d_cpart && c->cpart_slots) {
    const std::vector<unsigned long long> empty(c->cpart_slots, (unsigned long long)PK_EMPTY);
    (void)hipMemcpy(c->d_cpart, empty.data(), sizeof(unsigned long long) * c->cpart_slots, hipMemcpyHostToDevice);
    (void)hipMemcpy(c->d_cpart2, empty.data(), sizeof(unsigned long long) * c->cpart_slots, hipMemcpyHostToDevice);
  }
  if (c->batch.d_cp && c->batch.cap) {      // (the slots of every entry of a batch: the status words do not say which entry gave up)
    const std::vector<unsigned long long> empty(2 * c->batch.n_partial * (size_t)c->batch.cap, (unsigned long long)PK_EMPTY);
    (void)hipMemcpy(c->batch.d_cp, empty.data(), sizeof(unsigned long long) * empty.size(), hipMemcpyHostToDevice);
  }
  c->shim.status_seen[0] = st[0];
  c->shim.status_seen[1] = st[1];
  c->shim.x_valid = false;
  c->shim.lam_staged = false;
  if (da)
    return fail(c, 97, "pk_cycle: the finalize workgroup gave up waiting for %llu partial sum(s) of its own launch; f and the "
                       "gradient entries shared by all nodes of this iterate are NaN (hand-off slots reset)", da);
  return fail(c, 97, "%llu exchange(s) of the partial sums between the ranks gave up waiting for a peer; f and the shared "
                     "gradient entries of this iterate are NaN on this rank", db);
}

namespace {

// everything enqueued for the results has finished: the pending mark has been stored, or (no mark) the stream is idle
int wait_results_landed_raw(pk_ctx* c) {
  hipError_t e;
  if (c->shim.mark_pending) {
    const volatile unsigned long long* word = reinterpret_cast<const volatile unsigned long long*>(c->shim.res[0].h_out + 4);
    const unsigned long long want = c->shim.mark_val;
    for (long spins = 1; *word < want; ++spins) {
      if ((spins & 0x3FFF) == 0) {          // now and then: has the stream finished (or failed) without storing the mark?
        e = hipStreamQuery(c->stream);
        if (e == hipSuccess) {
          if (*word < want) return fail(c, 65, "the progress mark was not stored by its kernel");
          break;
        }
        if (e != hipErrorNotReady) return fail(c, 100 + (int)e, "waiting for the results: %s", hipGetErrorString(e));
      }
    }
    c->shim.mark_pending = false;
    if (c->shim.mark_op_seq > c->shim.idle_seq) c->shim.idle_seq = c->shim.mark_op_seq;
    return 0;
  }
  const uint64_t seen = c->shim.op_seq;
  while ((e = hipStreamQuery(c->stream)) == hipErrorNotReady) { }
  if (e != hipSuccess) return fail(c, 100 + (int)e, "hipStreamQuery failed: %s", hipGetErrorString(e));
  c->shim.idle_seq = seen;
  return 0;
}

int wait_results_landed(pk_ctx* c) {
  const int rc = wait_results_landed_raw(c);
  return rc ? rc : handoff_check(c);
}

// Queue the copies of the results in `mask` (bit k: result k; 0 f, 1 grad f, 2 g, 3 J, 4 H) of the current iterate that are
// not on their way yet, and -- unless results are awaited by polling the stream, see wait_result -- ONE event behind them.  J, grad f and g are neighbours on the device ([J | grad | g], one
// allocation); where their landing places are neighbours in the same order (the context's own block, or one block of the
// caller's) the pieces are merged: the changing part of J, grad f and g leave in one DMA.  The pieces of J that never
// change (pk_set_jac_constant_runs) are not copied at all.  f needs no copy when the kernel stored it into its pinned
// landing place itself (a DMA of 8 bytes costs as much as one of 100 KB).
int enqueue_result_copies(pk_ctx* c, unsigned mask) {
  struct Piece { const double* src; double* dst; size_t count; bool pinned; };
  std::vector<Piece> pcs;
  pcs.reserve(8);
  int first = -1;
  auto add = [&](const double* src, double* dst, size_t count, bool pinned) {
    if (!count) return;
    if (!pcs.empty() && pcs.back().src + pcs.back().count == src && pcs.back().dst + pcs.back().count == dst &&
        pcs.back().pinned == pinned) {
      pcs.back().count += count;
      return;
    }
    pcs.push_back(Piece{src, dst, count, pinned});
  };
  // device order of the x-results is [J | grad f | g]: one piece when nothing is left out; split_copy sends grad f | g first
  const int joined[5] = {0, 3, 1, 2, 4}, split[5] = {0, 1, 2, 3, 4};
  const int* order = c->shim.split_copy ? split : joined;
  size_t early_pieces = 0;
  bool early = false;
  for (int o = 0; o < 5; ++o) {
    const int k = order[o];
    if (!((mask >> k) & 1u) || c->shim.res[k].enq) continue;
    if (first < 0) first = k;
    if (c->shim.res[k].stored_direct) continue;
    const bool pinned = !c->shim.res[k].target || c->shim.res[k].target_pinned;
    if (k == 3 && c->shim.jac_filled) {
      const double* dj = device_result(c, 3);
      for (const auto& r : c->shim.jruns) add(dj + r.first, c->shim.res[3].landed + r.first, (size_t)(r.second - r.first), pinned);
    } else {
      add(device_result(c, k), c->shim.res[k].landed, result_count(c, k), pinned);
    }
    if (c->shim.split_copy && (k == 1 || k == 2)) { early = true; early_pieces = pcs.size(); }
  }
  if (first < 0) return 0;
  // an event behind grad f | g only when something (J) follows them in this batch: otherwise the stream's state tells
  const bool want_early = early && c->shim.spin_wait && ((mask >> 3) & 1u) && !c->shim.res[3].enq && !c->shim.res[3].stored_direct && pcs.size() > early_pieces;
  int rc;
  bool any_dma = false;
  for (size_t i = 0; i < pcs.size(); ++i) {
    const bool by_kernel = pcs[i].pinned && sizeof(double) * pcs[i].count <= ((size_t)c->shim.kernel_download << 20);
    any_dma |= !by_kernel || (((uintptr_t)pcs[i].dst ^ (uintptr_t)pcs[i].src) & 8) != 0;
    if ((rc = copy_async(c, pcs[i].dst, pcs[i].src, pcs[i].count, hipMemcpyDeviceToHost, by_kernel))) return rc;
    if (want_early && i + 1 == early_pieces) {
      PK_HIP(c, hipEventRecord(c->shim.ev_early, c->stream));
      c->shim.early_valid = true;
    }
  }
  ++c->shim.op_seq;
  // (a mark kernel behind a DMA would wait for the hand-off between the two engines, ~10 us: large copies keep the stream poll)
  c->shim.mark_pending = false;
  if (!any_dma && (rc = enqueue_mark(c))) return rc;
  if (!c->shim.spin_wait) PK_HIP(c, hipEventRecord(c->shim.res[first].ev_out, c->stream));      // (see wait_result)
  for (int k = 0; k < 5; ++k)
    if (((mask >> k) & 1u) && !c->shim.res[k].enq) { c->shim.res[k].enq = true; c->shim.res[k].ev_of = first; }
  return 0;
}

// Wait for result k of the current iterate.  Measured on MI355X (tools/dma_probe.cpp, profiles/r03_b_dma_probe.txt): a
// hipEventRecord behind a copy plus hipEventSynchronize (or polling hipEventQuery) returns ~8 us after polling
// hipStreamQuery alone does, and a word the kernel itself stores into pinned memory is seen ~4 us before its event.  So
// (spin_wait, the default) no event is recorded for the results at all: f, which the finalize kernel stores into its
// pinned landing place, is awaited on its own word (PK_EMPTY until the system-scope store lands), every copied result by
// polling the stream -- the result copies are the last thing an iterate enqueues, and an idle stream means every result
// enqueued so far has landed.
int wait_result_raw(pk_ctx* c, int k) {
  if (c->shim.res[k].done) return 0;
  if (k == 0 && c->shim.res[0].stored_direct && c->shim.spin_wait) {
    const volatile unsigned long long* word = (const volatile unsigned long long*)c->shim.res[0].landed;
    for (long spins = 1; *word == (unsigned long long)PK_EMPTY; ++spins) {
      if ((spins & 0x3FFF) == 0) {          // now and then: has the stream finished (or failed) without storing f?
        const uint64_t seen = c->shim.op_seq;
        const hipError_t e = hipStreamQuery(c->stream);
        if (e == hipSuccess) {
          c->shim.idle_seq = seen;
          if (*word == (unsigned long long)PK_EMPTY) {
            // (an f computed from a hand-off that gave up carries the sentinel's own NaN payload: say what happened)
            const int hc = handoff_check(c);
            return hc ? hc : fail(c, 65, "the objective was not stored by its kernel");
          }
          break;
        }
        if (e != hipErrorNotReady) return fail(c, 100 + (int)e, "waiting for f: %s", hipGetErrorString(e));
      }
    }
    c->shim.res[0].done = true;
    return 0;
  }
  if (c->shim.spin_wait) {
    hipError_t e;
    if ((k == 1 || k == 2) && c->shim.early_valid) {       // grad f | g went ahead of J with an event of their own (split_copy)
      while ((e = hipEventQuery(c->shim.ev_early)) == hipErrorNotReady) { }
      if (e != hipSuccess) return fail(c, 100 + (int)e, "hipEventQuery failed: %s", hipGetErrorString(e));
      c->shim.res[1].done = c->shim.res[2].done = true;
      return 0;
    }
    int rc = wait_results_landed_raw(c);
    if (rc) return rc;
    for (int j = 0; j < 5; ++j)
      if (c->shim.res[j].enq) c->shim.res[j].done = true;
    return 0;
  }
  PK_HIP(c, hipEventSynchronize(c->shim.res[c->shim.res[k].ev_of].ev_out));
  c->shim.res[k].done = true;
  return 0;
}

int wait_result(pk_ctx* c, int k) {
  const int rc = wait_result_raw(c, k);
  return rc ? rc : handoff_check(c);
}

}  // namespace

// stage `count` doubles in the next staging buffer of a double-buffered pair and queue their upload (dst == nullptr: stage
// only -- the consumer kernel reads the pinned buffer itself).  Large inputs are staged and uploaded in a few chunks so that
// the host's memcpy of chunk i + 1 runs while chunk i is on the link (4.8 MB: 202 -> 157 us; every extra DMA costs ~10 us,
// so small inputs go in one piece).
int stage_upload(pk_ctx* c, double* const bufs[2], hipEvent_t const evs[2], uint64_t seqs[2], int& cur, const double* src,
                 double* dst, size_t count, double** staged) {
  cur ^= 1;
  // the buffer was last read two iterates ago -- by an upload whose completion an idle stream seen since then implies
  // (polling waits), or whose event says so (event waits)
  if (seqs[cur] > c->shim.idle_seq) {
    if (c->shim.spin_wait || !dst) {          // (no upload, no event: the kernels that read the buffer in place are awaited on the stream)
      const uint64_t seen = c->shim.op_seq;
      PK_HIP(c, hipStreamSynchronize(c->stream));
      c->shim.idle_seq = seen;
    } else {
      PK_HIP(c, hipEventSynchronize(evs[cur]));
    }
  }
  const size_t bytes = sizeof(double) * count;
  const int chunks = (dst && c->shim.chunk_upload && bytes >= ((size_t)2 << 20)) ? (c->shim.kernel_upload ? 4 : 3) : 1;
  const size_t step = ((count + chunks - 1) / chunks + 7) & ~(size_t)7;
  int rc;
  for (size_t lo = 0; lo < count; lo += step) {
    const size_t len = count - lo < step ? count - lo : step;
    (void)pk_copy_bits(bufs[cur] + lo, src + lo, len);      // (memcpy; with the helper threads of pk_host_threads from 1 MB on)
    if (dst && (rc = copy_async(c, dst + lo, bufs[cur] + lo, len, hipMemcpyHostToDevice, c->shim.kernel_upload != 0))) return rc;
  }
  seqs[cur] = ++c->shim.op_seq;          // (a consumer kernel reading the buffer itself is enqueued right behind: same number)
  if (dst && !c->shim.spin_wait) PK_HIP(c, hipEventRecord(evs[cur], c->stream));
  if (staged) *staged = bufs[cur];
  return 0;
}

// pk_set_problem: the pinned staging buffers of x and lambda, the landing places of the five results and their events
int alloc_shim(pk_ctx* c) {
  c->shim.jruns.assign(1, std::make_pair((int64_t)0, (int64_t)c->nnz_J));
  c->shim.jconst.clear();
  c->shim.jruns_other.assign(1, std::make_pair((int64_t)0, (int64_t)c->nnz_Jc));
  c->shim.jconst_other.clear();
  const size_t cnt[5] = {1, (size_t)c->n, (size_t)c->m, (size_t)c->nnz_J, (size_t)c->nnz_H};
  for (int b = 0; b < 2; ++b) {
    PK_HIP(c, hipHostMalloc((void**)&c->shim.h_xs[b], sizeof(double) * (size_t)(c->n ? c->n : 1), hipHostMallocDefault));
    PK_HIP(c, hipHostMalloc((void**)&c->shim.h_lams[b], sizeof(double) * (size_t)(c->m ? c->m : 1), hipHostMallocDefault));
    PK_HIP(c, hipEventCreateWithFlags(&c->shim.ev_xs[b], hipEventDisableTiming));
    PK_HIP(c, hipEventCreateWithFlags(&c->shim.ev_lams[b], hipEventDisableTiming));
  }
  PK_HIP(c, hipHostMalloc((void**)&c->shim.res[0].h_out, sizeof(double) * 8, hipHostMallocDefault));
  std::memset(c->shim.res[0].h_out, 0, sizeof(double) * 8);      // ([0] f, [4] the progress mark of mark_wait, [6] [7] PkArgs.status)
  c->shim.status_seen[0] = c->shim.status_seen[1] = 0;
  c->shim.mark_val = 0; c->shim.mark_op_seq = 0; c->shim.mark_pending = false;
  PK_HIP(c, hipHostMalloc((void**)&c->shim.res[3].h_out, sizeof(double) * (cnt[3] + cnt[1] + cnt[2] + 1), hipHostMallocDefault));
  PK_HIP(c, hipHostMalloc((void**)&c->shim.res[4].h_out, sizeof(double) * (cnt[4] + 1), hipHostMallocDefault));
  c->shim.res[1].h_out = c->shim.res[3].h_out + cnt[3];                      // (one block [J | grad f | g], like the device's)
  c->shim.res[2].h_out = c->shim.res[1].h_out + cnt[1];
  for (int k = 0; k < 5; ++k) PK_HIP(c, hipEventCreateWithFlags(&c->shim.res[k].ev_out, hipEventDisableTiming));
  PK_HIP(c, hipEventCreateWithFlags(&c->shim.ev_early, hipEventDisableTiming));
  c->shim.xbuf = c->shim.lambuf = 0;
  return 0;
}

void free_shim(pk_ctx* c) {
  c->shim.jruns.clear(); c->shim.jconst.clear(); c->shim.jruns_other.clear(); c->shim.jconst_other.clear();
  c->shim.jac_compact = false;
  c->shim.lam_src = nullptr;
  if (c->shim.h_Hc) { (void)hipHostFree(c->shim.h_Hc); c->shim.h_Hc = nullptr; }
  for (int b = 0; b < 2; ++b) {
    if (c->shim.h_xs[b]) (void)hipHostFree(c->shim.h_xs[b]);
    if (c->shim.h_lams[b]) (void)hipHostFree(c->shim.h_lams[b]);
    if (c->shim.ev_xs[b]) (void)hipEventDestroy(c->shim.ev_xs[b]);
    if (c->shim.ev_lams[b]) (void)hipEventDestroy(c->shim.ev_lams[b]);
    c->shim.h_xs[b] = c->shim.h_lams[b] = nullptr;
    c->shim.ev_xs[b] = c->shim.ev_lams[b] = nullptr;
    c->shim.xs_seq[b] = c->shim.lams_seq[b] = 0;
  }
  if (c->shim.ev_early) { (void)hipEventDestroy(c->shim.ev_early); c->shim.ev_early = nullptr; }
  c->shim.early_valid = false;
  c->shim.h_x = nullptr;
  c->shim.x_valid = false;
  for (int k = 0; k < 5; ++k) {
    if (c->shim.res[k].h_out && k != 1 && k != 2) (void)hipHostFree(c->shim.res[k].h_out);      // (h_out[1], h_out[2] live inside h_out[3]'s block)
    if (c->shim.res[k].ev_out) (void)hipEventDestroy(c->shim.res[k].ev_out);
    c->shim.res[k].h_out = c->shim.res[k].target = c->shim.res[k].landed = nullptr;
    c->shim.res[k].ev_out = nullptr;
    c->shim.res[k].enq = false;
  }
}

int launch_store_word(pk_ctx* c, unsigned long long* dst, unsigned long long value, hipStream_t st) {
  hipLaunchKernelGGL(pk_store_word_kernel, dim3(1), dim3(64), 0, st, dst, value);
  PK_HIP(c, hipGetLastError());
  return 0;
}

extern "C" {

// ---------------------------------------------------------------- host shim: the "new x" protocol
// IPOPT evaluates f, grad f, g, J separately but on the same iterate (ipopt.py:41-53 hands the five methods of the
// problem object to cyipopt): pk_prepare_x uploads a new x ONCE, runs the fused x-kernel and -- prefetch mode -- queues
// the copy of every result into pinned host memory right behind it, in the order a solver asks for them; pk_fetch then
// only waits for the event of its result.  Nothing in here synchronizes the stream: the staging buffers of x and lambda
// are double-buffered and guarded by events, the results by one event each.
// 1 if x equals the x of the last pk_prepare_x bit for bit (the results held for it are still valid), else 0
int pk_same_x(pk_ctx* c, const double* x) {
  if (!c || !c->have_problem || !x || !c->shim.x_valid || !c->shim.h_x) return 0;
  return pk_same_bits(c->shim.h_x, x, (size_t)c->n);      // (with the helper threads of pk_host_threads, if the caller started any)
}

// the context's x / result buffers were used for something else (mesh error, one-shot evals, the cycle call)
int pk_invalidate_x(pk_ctx* c) {
  if (!c) return fail(nullptr, 1, "null context");
  c->shim.x_valid = false;
  return 0;
}

// Where the results of the NEXT pk_prepare_x / pk_eval_hess_prepared land: pinned host memory of the caller (from
// pk_host_alloc), NULL = the context's own pinned buffer of that output (pk_host_buffer).
int pk_set_result_targets(pk_ctx* c, double* f, double* grad, double* g, double* jac, double* hess) {
  int rc = ready(c);
  if (rc) return rc;
  double* t[5] = {f, grad, g, jac, hess};
  c->shim.target_filled = false;       // (an arbitrary array of the caller's: the whole Jacobian is copied into it)
  for (int k = 0; k < 5; ++k) {
    c->shim.res[k].target = t[k];
    c->shim.res[k].target_pinned = false;
    // A kernel may store into a target only if the device can see it (pinned / registered host memory); a pageable
    // target still works as the destination of a copy.
    c->shim.res[k].target_visible = true;
    if (t[k]) {
      hipPointerAttribute_t attr;
      std::memset(&attr, 0, sizeof attr);
      const hipError_t e = hipPointerGetAttributes(&attr, t[k]);
      if (e != hipSuccess) (void)hipGetLastError();
      c->shim.res[k].target_visible = e == hipSuccess && (attr.type == hipMemoryTypeHost || attr.type == hipMemoryTypeDevice ||
                                                 attr.type == hipMemoryTypeManaged);
    }
  }
  return 0;
}

// prefetch = 1 (default): every x-only result is copied to the host right behind the kernel; 0: a result is copied
// when it is first asked for (a request for the gradient also queues the Jacobian -- a solver wants both at an accepted
// point, and neither at a rejected trial point).  host_direct = 1: the kernels store f / grad / g / J (and H) straight
// into the pinned host targets over PCIe, no device-side staging and no DMA (A/B switch).
int pk_set_host_mode(pk_ctx* c, int prefetch, int host_direct) {
  if (!c) return fail(nullptr, 1, "null context");
  c->shim.prefetch = prefetch ? 1 : 0;
  c->shim.host_direct = host_direct ? 1 : 0;
  c->shim.x_valid = false;
  return 0;
}

// Pinned (page-locked, device-visible) host memory for result arrays that outlive a call: process-wide, not tied to a
// context (a host array handed to the solver may outlive the evaluator that filled it).
int pk_host_alloc(size_t bytes, void** out) {
  if (!out) return fail(nullptr, 60, "null host buffer");
  *out = nullptr;
  hipError_t e = hipHostMalloc(out, bytes ? bytes : 8, hipHostMallocDefault);
  if (e != hipSuccess) return fail(nullptr, 100 + (int)e, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  return 0;
}

int pk_host_free(void* p) {
  if (!p) return 0;
  // (a landing block may still be the target of copies nobody asked for -- every result of a new x is on its way into it:
  //  nothing may be in flight when the memory goes; found by the sanitized build, tests/fake_hip)
  (void)hipDeviceSynchronize();
  hipError_t e = hipHostFree(p);
  if (e != hipSuccess) return fail(nullptr, 100 + (int)e, "hipHostFree failed: %s", hipGetErrorString(e));
  return 0;
}

namespace {
bool small_x(const pk_ctx* c) { return c->shim.small_direct && sizeof(double) * (size_t)c->n <= ((size_t)c->shim.small_x_kb << 10); }
bool small_results(const pk_ctx* c) {
  const size_t nj = (size_t)(c->shim.jac_compact ? c->nnz_Jc : c->nnz_J);
  return c->shim.small_direct && sizeof(double) * (nj + (size_t)c->n + (size_t)c->m) <= ((size_t)1 << 20);
}
bool hess_goes_direct(const pk_ctx* c) {
  return c->shim.hess_direct && sizeof(double) * (size_t)c->nnz_H <= ((size_t)c->shim.kernel_download << 20);
}

// multipliers of the next Hessian: staged in pinned memory; uploaded by DMA, or -- lambda_direct -- left there for the
// Hessian kernel to read over PCIe itself (0.77 MB: DMA + kernel 34 us, kernel reading pinned memory 26 us)
int stage_lambda(pk_ctx* c, const double* lambda) {
  double* staged = nullptr;
  const bool direct = c->shim.lambda_direct != 0 && sizeof(double) * (size_t)c->m <= ((size_t)2 << 20);
  int rc = stage_upload(c, c->shim.h_lams, c->shim.ev_lams, c->shim.lams_seq, c->shim.lambuf, lambda, direct ? nullptr : c->d_lam, (size_t)c->m, &staged);
  if (rc) return rc;
  c->shim.lam_src = direct ? staged : c->d_lam;
  c->shim.lam_staged = true;
  return 0;
}

// a landing block of the caller's for the x-results of the next new iterate: [J (nnz_J) | grad f (n) | g (m)]
void take_block(pk_ctx* c, double* block) {
  const int64_t nj = c->shim.jac_compact ? c->nnz_Jc : c->nnz_J;      // (a block follows the layout the Jacobian callback serves)
  c->shim.res[3].target = block;
  c->shim.res[1].target = block ? block + nj : nullptr;
  c->shim.res[2].target = block ? block + nj + c->n : nullptr;
  c->shim.res[1].target_visible = c->shim.res[2].target_visible = c->shim.res[3].target_visible = !c->shim.host_direct;   // (copy targets; see pk_set_result_targets)
  c->shim.target_filled = block != nullptr;      // (the contract of pk_callback_x: blocks were filled by pk_fill_jac_constants)
  c->shim.res[1].target_pinned = c->shim.res[2].target_pinned = c->shim.res[3].target_pinned = block != nullptr;      // (... and are pinned memory)
}
}  // namespace

int pk_prepare_x(pk_ctx* c, const double* x) {
  int rc = ready(c);
  if (rc) return rc;
  if (!x) return fail(c, 60, "null host buffer");
  PK_HIP(c, hipSetDevice(c->device));
  c->shim.x_valid = false;
  const bool sx = small_x(c), sr = small_results(c);
  if ((rc = stage_upload(c, c->shim.h_xs, c->shim.ev_xs, c->shim.xs_seq, c->shim.xbuf, x, sx ? nullptr : c->d_x, (size_t)c->n, &c->shim.h_x))) return rc;
  // (small x: every kernel of this iterate -- the x-part now, the Hessian later -- reads the staging buffer in place.  The
  //  buffer is written again two stagings from now; every kernel of this iterate has been awaited by then: a callback returns
  //  only when its result has landed, a discarded speculative launch is synchronized, and stage_upload waits for the stream
  //  if nothing since the buffer's staging has been seen idle)
  c->shim.x_src = sx ? c->shim.h_x : c->d_x;
  for (int k = 0; k < 5; ++k) {
    c->shim.res[k].landed = c->shim.res[k].target ? c->shim.res[k].target : c->shim.res[k].h_out;
    c->shim.res[k].enq = c->shim.res[k].done = false;
  }
  c->shim.jac_filled = !c->shim.jconst.empty() && (c->shim.res[3].target ? c->shim.target_filled : true) && !c->shim.host_direct && !sr;
  c->shim.early_valid = false;
  double* o[4];
  for (int k = 0; k < 4; ++k) {     // (f: stored by the kernel itself whenever its landing place is device-visible)
    c->shim.res[k].stored_direct = (c->shim.host_direct || sr || k == 0) && (!c->shim.res[k].target || c->shim.res[k].target_visible);
    o[k] = c->shim.res[k].stored_direct ? c->shim.res[k].landed : device_result(c, k);
  }
  if (c->shim.res[0].stored_direct) *(volatile unsigned long long*)c->shim.res[0].landed = (unsigned long long)PK_EMPTY;     // (see wait_result)
  if (c->shim.jac_compact && !c->has_big && xpart_is_one_launch(c)) {
    // the compact layout of the Jacobian from the SAME launch: its Jacobian role runs pk_jacc's tile code (no reference-layout
    // J is written, no second kernel)
    if ((rc = enqueue_single_launch_cycle(c, c->shim.x_src, nullptr, 0.0, o[0], o[1], o[2], o[3], nullptr, c->stream, 1))) return rc;
  } else {
    if ((rc = pk_eval_xpart_dev(c, c->shim.x_src, o[0], o[1], o[2], c->shim.jac_compact ? c->d_J : o[3], nullptr))) return rc;
    // the compact layout of the Jacobian: its own kernel behind the fused x-kernel (whose reference-layout J stays on the device)
    if (c->shim.jac_compact && (rc = pk_eval_jacc_dev(c, c->shim.x_src, o[3], nullptr))) return rc;
  }
  // f and g are what a line search asks for at every trial point: always on their way; grad f and J in prefetch mode
  const bool ahead = c->shim.prefetch && (!c->shim.adaptive_prefetch || c->shim.cur_J_asked);
  c->shim.cur_J_asked = false;
  if ((rc = enqueue_result_copies(c, ahead ? 0xFu : 0x5u))) return rc;
  c->shim.x_valid = true;
  return 0;
}

// result `what` (0 f, 1 grad, 2 g, 3 jac) of the last pk_prepare_x: waits for its copy.  out == NULL: the result stays
// where it landed (pk_result_location); otherwise it is copied on to `out` (a second host copy).
int pk_fetch(pk_ctx* c, int what, double* out) {
  int rc = ready(c);
  if (rc) return rc;
  if (what < 0 || what > 3) return fail(c, 61, "pk_fetch: what must be 0 (f), 1 (grad), 2 (g) or 3 (jac)");
  if (!c->shim.x_valid) return fail(c, 64, "pk_fetch: no prepared x (pk_prepare_x)");
  if (what == 1 || what == 3) c->shim.cur_J_asked = true;
  if (!c->shim.res[what].enq && (rc = enqueue_result_copies(c, (1u << what) | (what == 1 ? 8u : 0u)))) return rc;   // (an accepted point: J follows grad f)
  if ((rc = wait_result(c, what))) return rc;
  if (out && out != c->shim.res[what].landed) std::memcpy(out, c->shim.res[what].landed, sizeof(double) * result_count(c, what));
  return 0;
}

// ONE call per x-callback of a host shim (objective / gradient / constraints / jacobian of the cyipopt protocol,
// ipopt.py:41-53): if `x` is not the prepared iterate it becomes it -- its results landing in `block`, pinned memory of the
// caller's holding [J (nnz_J) | grad f (n) | g (m)] (NULL: the context's own buffers; f always lands in the context's
// pinned word) and *fresh = 1 -- then result `what` is waited for; f_out (may be NULL) receives f when what == 0.
int pk_callback_x(pk_ctx* c, int what, const double* x, double* block, double* f_out, int* fresh) {
  int rc = ready(c);
  if (rc) return rc;
  if (!x) return fail(c, 60, "null host buffer");
  if (what < 0 || what > 3) return fail(c, 61, "pk_callback_x: what must be 0 (f), 1 (grad), 2 (g) or 3 (jac)");
  const bool same = pk_same_x(c, x) != 0;
  if (fresh) *fresh = same ? 0 : 1;
  if (!same) {
    c->shim.res[0].target = nullptr;
    take_block(c, block);
    if ((rc = pk_prepare_x(c, x))) return rc;
  }
  if ((rc = pk_fetch(c, what, nullptr))) return rc;
  if (what == 0 && f_out) *f_out = c->shim.res[0].landed[0];
  return 0;
}

// ONE call for all five results of an iterate whose multipliers are known together with x (a solver written against the C
// ABI; Evaluator.cycle): x and lambda are staged like in the callbacks, the whole cycle is ONE launch (pk_cycle), the results
// land like the callbacks' -- [J (changing part) | grad f | g] in `block` (pinned, [J | grad f | g], constants filled in by
// pk_fill_jac_constants), H in `hess` (pinned), f in the context's pinned word -- and the call returns when all of it is
// there.  Reference layout of the Jacobian only.
int pk_callback_cycle(pk_ctx* c, const double* x, const double* lambda, double sigma, double* block, double* hess, double* f_out) {
  int rc = ready(c);
  if (rc) return rc;
  if (!x || !lambda || !block || !hess) return fail(c, 60, "null host buffer");
  if (c->shim.jac_compact) return fail(c, 68, "pk_callback_cycle: the one-launch cycle writes the reference layout of the Jacobian");
  PK_HIP(c, hipSetDevice(c->device));
  c->shim.x_valid = false;
  if ((rc = stage_lambda(c, lambda))) return rc;
  c->shim.res[0].target = nullptr;
  take_block(c, block);
  c->shim.res[4].target = hess;
  c->shim.res[4].target_visible = !c->shim.host_direct;
  c->shim.res[4].target_pinned = true;
  const bool sx = small_x(c), sr = small_results(c) && !c->shim.host_direct;
  if ((rc = stage_upload(c, c->shim.h_xs, c->shim.ev_xs, c->shim.xs_seq, c->shim.xbuf, x, sx ? nullptr : c->d_x, (size_t)c->n, &c->shim.h_x))) return rc;
  c->shim.x_src = sx ? c->shim.h_x : c->d_x;
  for (int k = 0; k < 5; ++k) {
    c->shim.res[k].landed = c->shim.res[k].target ? c->shim.res[k].target : c->shim.res[k].h_out;
    c->shim.res[k].enq = c->shim.res[k].done = false;
  }
  c->shim.jac_filled = !c->shim.jconst.empty() && c->shim.target_filled && !c->shim.host_direct && !sr;
  c->shim.early_valid = false;
  double* o[5];
  for (int k = 0; k < 5; ++k) {
    c->shim.res[k].stored_direct = k == 0 || (k == 4 && hess_goes_direct(c) && c->shim.res[4].target_visible) || (k >= 1 && k <= 3 && sr);
    o[k] = c->shim.res[k].stored_direct ? c->shim.res[k].landed : (k == 4 ? c->d_H : device_result(c, k));
  }
  *(volatile unsigned long long*)c->shim.res[0].landed = (unsigned long long)PK_EMPTY;
  if ((rc = pk_eval_cycle_dev(c, c->shim.x_src, c->shim.lam_src, sigma, o[0], o[1], o[2], o[3], o[4], nullptr))) return rc;
  c->shim.lam_staged = false;
  if ((rc = enqueue_result_copies(c, 0x1Fu))) return rc;
  c->shim.x_valid = true;
  c->shim.cur_J_asked = true;
  if ((rc = wait_result(c, 4)) || (rc = wait_result(c, 3)) || (rc = wait_result(c, 0))) return rc;
  c->shim.res[1].done = c->shim.res[2].done = true;
  if (f_out) *f_out = c->shim.res[0].landed[0];
  return 0;
}

// Queue the upload of the multipliers of the next pk_eval_hess_prepared and return: the caller's check of x
// (pk_same_x, a pass over n doubles) then runs while the DMA is in flight.
int pk_stage_lambda(pk_ctx* c, const double* lambda) {
  int rc = ready(c);
  if (rc) return rc;
  if (!lambda) return fail(c, 60, "null host buffer");
  PK_HIP(c, hipSetDevice(c->device));
  return stage_lambda(c, lambda);
}

// Hessian on the x of the last pk_prepare_x (no re-upload of x); vals == NULL: the result stays where it landed;
// lambda == NULL: the multipliers staged by pk_stage_lambda
int pk_eval_hess_prepared(pk_ctx* c, const double* lambda, double sigma, double* vals) {
  int rc = ready(c);
  if (rc) return rc;
  if (!lambda && !c->shim.lam_staged) return fail(c, 60, "null host buffer (no multipliers staged either)");
  if (!c->shim.x_valid) return fail(c, 64, "pk_eval_hess_prepared: no prepared x (pk_prepare_x)");
  PK_HIP(c, hipSetDevice(c->device));
  if (lambda && (rc = stage_lambda(c, lambda))) return rc;
  c->shim.lam_staged = false;
  c->shim.res[4].landed = c->shim.res[4].target ? c->shim.res[4].target : c->shim.res[4].h_out;
  c->shim.res[4].enq = c->shim.res[4].done = false;
  c->shim.res[4].stored_direct = (c->shim.host_direct || hess_goes_direct(c)) && (!c->shim.res[4].target || c->shim.res[4].target_visible);
  if ((rc = pk_eval_hess_dev(c, c->shim.x_src, c->shim.lam_src, sigma, c->shim.res[4].stored_direct ? c->shim.res[4].landed : c->d_H, nullptr))) return rc;
  if ((rc = enqueue_result_copies(c, 1u << 4))) return rc;
  if ((rc = wait_result(c, 4))) return rc;
  if (vals && vals != c->shim.res[4].landed) std::memcpy(vals, c->shim.res[4].landed, sizeof(double) * (size_t)c->nnz_H);
  return 0;
}

// The compact Hessian layout on the x of the last pk_prepare_x: what a solver that was handed the compact structure calls
// instead of pk_eval_hess_prepared -- 6 ... 10 x fewer values over PCIe.  lambda == NULL: the
// multipliers staged by pk_stage_lambda.  vals_pinned = 1: `vals` is device-visible host memory (pk_host_alloc) and the
// DMA writes it directly; 0: the values land in a pinned buffer of the context and are copied on.
int pk_eval_hessc_prepared(pk_ctx* c, const double* lambda, double sigma, double* vals, int vals_pinned) {
  int rc = ready(c);
  if (rc) return rc;
  if (!vals) return fail(c, 60, "null host buffer");
  if (!lambda && !c->shim.lam_staged) return fail(c, 60, "null host buffer (no multipliers staged either)");
  if (!c->shim.x_valid) return fail(c, 64, "pk_eval_hessc_prepared: no prepared x (pk_prepare_x)");
  if (c->nnz_Hc <= 0) return fail(c, 51, "pk_eval_hessc: no compact Hessian layout was supplied to pk_set_problem");
  PK_HIP(c, hipSetDevice(c->device));
  if (lambda && (rc = stage_lambda(c, lambda))) return rc;
  c->shim.lam_staged = false;
  if ((rc = pk_eval_hessc_dev(c, c->shim.x_src, c->shim.lam_src, sigma, c->d_Hc, nullptr))) return rc;
  const size_t bytes = sizeof(double) * (size_t)c->nnz_Hc;
  double* dst = vals;
  if (!vals_pinned) {
    if (!c->shim.h_Hc) PK_HIP(c, hipHostMalloc((void**)&c->shim.h_Hc, bytes, hipHostMallocDefault));
    dst = c->shim.h_Hc;
  }
  const bool hc_by_kernel = bytes <= ((size_t)c->shim.kernel_download << 20) && !(((uintptr_t)dst ^ (uintptr_t)c->d_Hc) & 8);
  if ((rc = copy_async(c, dst, c->d_Hc, (size_t)c->nnz_Hc, hipMemcpyDeviceToHost, hc_by_kernel))) return rc;
  ++c->shim.op_seq;
  c->shim.mark_pending = false;
  if (hc_by_kernel && (rc = enqueue_mark(c))) return rc;
  if (c->shim.spin_wait) {      // (every earlier copy of this iterate has been waited for by its callback)
    if ((rc = wait_results_landed(c))) return rc;
  } else {
    PK_HIP(c, hipStreamSynchronize(c->stream));
  }
  if (!vals_pinned) std::memcpy(vals, c->shim.h_Hc, bytes);
  return 0;
}

// ONE call for the Hessian callback of a host shim (SystemBase.hessian, systembase.py:820-835): the multipliers are staged
// first (their upload, if any, runs while x is compared), a new x is prepared like in pk_callback_x (landing block
// `block`), then the Hessian of the Lagrangian is evaluated on the prepared x and waited for.  compact = 0: reference
// layout, `hess` = pinned landing place of nnz_H values (NULL: the context's buffer); compact = 1: the compact layout
// (pk_eval_hessc), `hess` = pinned landing place of nnz_Hc values (required).
int pk_callback_hess(pk_ctx* c, const double* x, const double* lambda, double sigma, double* block, double* hess, int compact,
                     int* fresh) {
  int rc = ready(c);
  if (rc) return rc;
  if (!x || !lambda) return fail(c, 60, "null host buffer");
  if (compact && !hess) return fail(c, 60, "pk_callback_hess: the compact layout needs a landing array");
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = stage_lambda(c, lambda))) return rc;
  if (!compact) {
    c->shim.res[4].target = hess;
    c->shim.res[4].target_visible = !c->shim.host_direct;      // (by contract `hess` is pinned memory the device can address)
    c->shim.res[4].target_pinned = hess != nullptr;
  }
  if (fresh) *fresh = 0;
  // The solver's Hessian callback comes on the iterate the x-callbacks just ran on: launch on the prepared x at once and
  // compare x with it WHILE the GPU works (the compare is a pass over n doubles: 10 us at 12k nodes, 90 us at 40k).  A
  // different x discards the launch (its values are overwritten below) and takes the ordinary route.
  if (c->shim.speculative_hess && c->shim.x_valid && c->shim.h_x) {
    const size_t bytes = sizeof(double) * (size_t)c->nnz_Hc;
    if (compact) {
      if ((rc = pk_eval_hessc_dev(c, c->shim.x_src, c->shim.lam_src, sigma, c->d_Hc, nullptr))) return rc;
      const bool hc_by_kernel = bytes <= ((size_t)c->shim.kernel_download << 20) && !(((uintptr_t)hess ^ (uintptr_t)c->d_Hc) & 8);
      if ((rc = copy_async(c, hess, c->d_Hc, (size_t)c->nnz_Hc, hipMemcpyDeviceToHost, hc_by_kernel))) return rc;
      ++c->shim.op_seq;
      c->shim.mark_pending = false;
      if (hc_by_kernel && (rc = enqueue_mark(c))) return rc;
    } else {
      c->shim.res[4].landed = c->shim.res[4].target ? c->shim.res[4].target : c->shim.res[4].h_out;
      c->shim.res[4].enq = c->shim.res[4].done = false;
      c->shim.res[4].stored_direct = (c->shim.host_direct || hess_goes_direct(c)) && (!c->shim.res[4].target || c->shim.res[4].target_visible);
      if ((rc = pk_eval_hess_dev(c, c->shim.x_src, c->shim.lam_src, sigma, c->shim.res[4].stored_direct ? c->shim.res[4].landed : c->d_H, nullptr))) return rc;
      if ((rc = enqueue_result_copies(c, 1u << 4))) return rc;
    }
    const bool same = pk_same_bits(c->shim.h_x, x, (size_t)c->n) != 0;
    const uint64_t seen = c->shim.op_seq;
    if (same) {
      c->shim.lam_staged = false;
      if (!compact) return wait_result(c, 4);
      return wait_results_landed(c);
    }
    PK_HIP(c, hipStreamSynchronize(c->stream));       // (the discarded launch must not write behind the one that follows)
    c->shim.mark_pending = false;
    c->shim.idle_seq = seen;
    c->shim.x_valid = false;
  }
  const bool same = pk_same_x(c, x) != 0;
  if (fresh) *fresh = same ? 0 : 1;
  if (!same) {
    c->shim.res[0].target = nullptr;
    take_block(c, block);
    if ((rc = pk_prepare_x(c, x))) return rc;
  }
  if (compact) return pk_eval_hessc_prepared(c, nullptr, sigma, hess, 1);
  return pk_eval_hess_prepared(c, nullptr, sigma, nullptr);
}

// Runs [start[i], stop[i]) of the Jacobian values -- in the layout the shim serves, pk_set_jacobian_layout; every layout keeps
// its own -- that never change with x (ascending, disjoint): the x-results' copy to the
// host skips them from now on.  The landing arrays must hold those values already: pk_fill_jac_constants writes them into
// an array once (the context's own landing buffer is filled here).  n_runs = 0 restores the full copy.
// Reference: the translation part of the Jacobian, phasebase.py:1071-1081, is recomputed and returned by every call there.
int pk_set_jac_constant_runs(pk_ctx* c, int n_runs, const int64_t* start, const int64_t* stop) {
  int rc = ready(c);
  if (rc) return rc;
  if (n_runs < 0 || (n_runs > 0 && (!start || !stop))) return fail(c, 66, "pk_set_jac_constant_runs: bad arguments");
  int64_t at = 0;
  for (int i = 0; i < n_runs; ++i) {
    if (start[i] < at || stop[i] <= start[i] || stop[i] > (int64_t)result_count(c, 3))
      return fail(c, 66, "pk_set_jac_constant_runs: run %d [%lld, %lld) is out of order or out of range", i, (long long)start[i], (long long)stop[i]);
    at = stop[i];
  }
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  c->shim.x_valid = false;
  c->shim.jconst.clear();
  c->shim.jruns.clear();
  at = 0;
  for (int i = 0; i < n_runs; ++i) {
    if (start[i] > at) c->shim.jruns.emplace_back(at, start[i]);
    c->shim.jconst.emplace_back(start[i], stop[i]);
    at = stop[i];
  }
  if (at < (int64_t)result_count(c, 3) || c->shim.jruns.empty()) c->shim.jruns.emplace_back(at, (int64_t)result_count(c, 3));
  if (n_runs == 0) return 0;
  // one evaluation of J (in the layout the shim serves) into the context's device buffer, whatever x it holds -- the
  // constant entries do not depend on it --, from which the constants are taken
  if ((rc = c->shim.jac_compact ? pk_eval_jacc_dev(c, c->d_x, c->d_Jc, nullptr) : pk_eval_jac_dev(c, c->d_x, c->d_J, nullptr))) return rc;
  return pk_fill_jac_constants(c, c->shim.res[3].h_out);
}

// the x-independent runs of J (pk_set_jac_constant_runs) -> jac[...]; the other entries of `jac` are not touched
int pk_fill_jac_constants(pk_ctx* c, double* jac) {
  int rc = ready(c);
  if (rc) return rc;
  if (!jac) return fail(c, 60, "null host buffer");
  PK_HIP(c, hipSetDevice(c->device));
  const double* dj = device_result(c, 3);
  for (const auto& r : c->shim.jconst)
    PK_HIP(c, hipMemcpyAsync(jac + r.first, dj + r.first, sizeof(double) * (size_t)(r.second - r.first), hipMemcpyDeviceToHost, c->stream));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

// Which layout the Jacobian of the host shim (pk_prepare_x / pk_fetch(3) / pk_callback_x(3), the J part of a landing block)
// has: 0 the reference's triplets (default), 1 the compact layout of pk_eval_jacc.
int pk_set_jacobian_layout(pk_ctx* c, int compact) {
  int rc = ready(c);
  if (rc) return rc;
  if (compact && c->nnz_Jc <= 0) return fail(c, 52, "pk_set_jacobian_layout: no compact Jacobian layout was supplied to pk_set_problem");
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  if ((compact != 0) != c->shim.jac_compact) {      // every layout has constant runs of its own
    c->shim.jruns.swap(c->shim.jruns_other);
    c->shim.jconst.swap(c->shim.jconst_other);
  }
  c->shim.jac_compact = compact != 0;
  c->shim.x_valid = false;
  for (int k = 0; k < 5; ++k) c->shim.res[k].target = nullptr;
  return 0;
}

// A/B switches of the host shim (defaults: what measured fastest): "spin_wait" (1: results are awaited
// by polling, 0: hipEventSynchronize), "lambda_direct" (1: the Hessian kernel reads the staged multipliers from pinned
// memory itself, 0: they are uploaded first), "chunk_upload" (1: large inputs are staged and uploaded in chunks),
// "kernel_upload" / "kernel_download" (copy kernels instead of the DMA engine), "split_copy" (grad f | g ahead of J),
// "speculative_hess" (the Hessian is launched before x has been compared with the prepared iterate).
int pk_set_host_option(pk_ctx* c, const char* name, int value) {
  if (!c) return fail(nullptr, 1, "null context");
  if (!name) return fail(c, 67, "pk_set_host_option: null name");
  if (c->have_problem) {
    PK_HIP(c, hipSetDevice(c->device));
    PK_HIP(c, hipStreamSynchronize(c->stream));
  }
  c->shim.x_valid = false;
  c->shim.lam_staged = false;
  if (!std::strcmp(name, "spin_wait")) c->shim.spin_wait = value != 0;
  else if (!std::strcmp(name, "lambda_direct")) c->shim.lambda_direct = value != 0;
  else if (!std::strcmp(name, "chunk_upload")) c->shim.chunk_upload = value != 0;
  else if (!std::strcmp(name, "kernel_upload")) c->shim.kernel_upload = value != 0;
  else if (!std::strcmp(name, "kernel_download")) c->shim.kernel_download = value < 0 ? 0 : (value > 4096 ? 4096 : value);
  else if (!std::strcmp(name, "split_copy")) c->shim.split_copy = value != 0;
  else if (!std::strcmp(name, "speculative_hess")) c->shim.speculative_hess = value != 0;
  else if (!std::strcmp(name, "hess_direct")) c->shim.hess_direct = value != 0;
  else if (!std::strcmp(name, "xpart_single")) c->xpart_single = value != 0;
  else if (!std::strcmp(name, "separate_x")) {
    if (value && c->has_big) return fail(c, 67, "pk_set_host_option: separate_x needs a mesh without intervals of more than 64 points "
                                                "(such a mesh has the fused x-kernel only)");
    c->separate_x = value != 0;
    drop_cycle_graph(c);
  }
  else if (!std::strcmp(name, "small_direct")) c->shim.small_direct = value != 0;
  else if (!std::strcmp(name, "small_x_kb")) c->shim.small_x_kb = value < 0 ? 0 : (value > (1 << 20) ? (1 << 20) : value);
  else if (!std::strcmp(name, "adaptive_prefetch")) { c->shim.adaptive_prefetch = value != 0; c->shim.cur_J_asked = true; }
  else if (!std::strcmp(name, "mark_wait")) { c->shim.mark_wait = value != 0; c->shim.mark_pending = false; }
  else if (!std::strcmp(name, "poll_limit")) { c->shim.poll_limit = value < 0 ? 0 : value; drop_cycle_graph(c); }
  else return fail(c, 67, "pk_set_host_option: unknown option \"%s\"", name);
  return 0;
}

// where result `what` (0..4) of the current iterate landed (valid after its pk_fetch / pk_eval_hess_prepared)
int pk_result_location(pk_ctx* c, int what, double** ptr) {
  int rc = ready(c);
  if (rc) return rc;
  if (what < 0 || what > 4 || !ptr) return fail(c, 62, "pk_result_location: bad arguments");
  *ptr = c->shim.res[what].landed ? c->shim.res[what].landed : c->shim.res[what].h_out;
  return 0;
}

// pinned host result buffers of the context: what = 0 f, 1 grad, 2 g, 3 jac, 4 hess
int pk_host_buffer(pk_ctx* c, int what, double** ptr, int64_t* count) {
  int rc = ready(c);
  if (rc) return rc;
  if (what < 0 || what > 4 || !ptr) return fail(c, 62, "pk_host_buffer: bad arguments");
  const int64_t cnt[5] = {1, c->n, c->m, c->nnz_J, c->nnz_H};
  *ptr = c->shim.res[what].h_out;
  if (count) *count = cnt[what];
  return 0;
}

}  // extern "C"
