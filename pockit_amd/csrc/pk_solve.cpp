// pk_solve.cpp -- the host scaffolding of a solve that lives on the device, stated once for pk_cg.cpp and pk_minres.cpp (and, for
// the growing arrays, pk_merit.cpp): the arrays of the context that grow on demand, the checks every entry point of a solver
// makes, and the skeletons of record / advance / the host form's loop.  No kernels and no arithmetic: a method brings its
// record, its steps and its iteration (a plain function); nothing here knows which method it serves.
#include "pk_libkernel.h"      // (lib_dot_pieces: how many partial sums a dot of a length leaves)

// work enqueued earlier may still use the old array, so the device is waited for before it is freed
int lib_reserve(pk_ctx* c, double*& p, size_t& cap, size_t want, int code, const char* who, const char* what) {
  if (want <= cap) return 0;
  PK_HIP(c, hipSetDevice(c->device));
  double* q = nullptr;
  if (hipMalloc((void**)&q, sizeof(double) * want) != hipSuccess || !q)
    return fail(c, code, "%s: no device memory for %zu doubles of %s", who, want, what);
  const hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    release(q);
    return fail(c, 100 + (int)e, "hipDeviceSynchronize failed: %s", hipGetErrorString(e));
  }
  release(p);
  p = q;
  cap = want;
  return 0;
}

int lib_upload(pk_ctx* c, double* dst, const double* src, size_t count) {
  if (src && count) PK_HIP(c, hipMemcpyAsync(dst, src, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
  return 0;
}

int solve_state(pk_ctx* c, PkSolveState& s, size_t work, size_t rec, const char* who) {
  if (const int rc = lib_reserve(c, s.d_work, s.work_cap, work, 136, who, "work vectors")) return rc;
  return lib_reserve(c, s.d_rec, s.rec_cap, rec, 136, who, "the record");
}

int solve_partial(pk_ctx* c, PkSolveState& s, int planes, int64_t len, const char* who) {
  return lib_reserve(c, s.d_partial, s.partial_cap, (size_t)planes * (size_t)lib_dot_pieces(len), 136, who, "partial sums");
}

int solve_ops_ready(pk_ctx* c, bool with_h, bool pointers, const char* who) {
  int rc;
  if (c->shard.flags || c->exchange.world > 1) return fail(c, 119, "%s: not offered for a sharded context", who);
  if ((rc = op_ready(c, 0, pointers, who)) || (rc = op_ready(c, 1, pointers, who))) return rc;
  return with_h ? op_ready(c, 2, pointers, who) : 0;
}

int solve_host_checks(pk_ctx* c, bool with_h, double tol, int maxiter, int check_every, int precond, const double*& jvals,
                      const double*& hvals, const char* who) {
  int rc;
  if (!solve_tol_ok(tol) || maxiter < 1 || check_every < 1 || precond < 0 || precond > 2)
    return fail(c, 134, "%s: tol %g (finite, not negative), maxiter %d and check_every %d (at least 1), precond %d (0, 1 or 2)", who, tol,
                maxiter, check_every, precond);
  if ((rc = solve_linearized(c, with_h, jvals, hvals, who))) return rc;
  if (precond == 1 && with_h && !c->ops.d_diag_pos) return fail(c, 132, "%s: call pk_set_operator_diagonal(2) first", who);
  return 0;
}

int solve_linearized(pk_ctx* c, bool with_h, const double*& jvals, const double*& hvals, const char* who) {
  hvals = nullptr;
  if (const int rc = op_linearized(c, 0, jvals, who)) return rc;
  return with_h ? op_linearized(c, 2, hvals, who) : 0;
}

int solve_record(pk_ctx* c, const PkSolveState& s, double* rec, size_t count, const char* who, const char* begin) {
  if (!rec) return fail(c, 60, "null host buffer");
  if (!s.active) return fail(c, 135, "%s: no solve in progress (%s)", who, begin);
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipMemcpyAsync(rec, s.d_rec, sizeof(double) * count, hipMemcpyDeviceToHost, s.stream));
  PK_HIP(c, hipStreamSynchronize(s.stream));
  return 0;
}

int solve_advance(pk_ctx* c, PkSolveState& s, int iters, void* stream, int (*iteration)(pk_ctx*, hipStream_t), const char* who,
                  const char* begin) {
  if (iters < 1) return fail(c, 134, "%s: iters = %d, at least one iteration", who, iters);
  if (!s.active) return fail(c, 135, "%s: no solve in progress (%s)", who, begin);
  hipStream_t st = pick(c, stream);
  s.stream = st;
  for (int k = 0; k < iters; ++k)
    if (const int rc = iteration(c, st)) return rc;
  return 0;
}

int solve_host_loop(pk_ctx* c, int maxiter, int check_every, int (*advance)(pk_ctx*, int, void*), int (*record)(pk_ctx*, double*),
                    double* rec, double* x, const double* d_x, size_t count) {
  int rc;
  if ((rc = record(c, rec))) return rc;
  for (int done = 0; rec[0] == 0.0 && done < maxiter;) {
    const int chunk = std::min(check_every, maxiter - done);
    if ((rc = advance(c, chunk, nullptr)) || (rc = record(c, rec))) return rc;
    done += chunk;
  }
  if (rec[0] == 0.0) rec[0] = 4.0;      // exhausted: in the host copy only
  if (count) PK_HIP(c, hipMemcpyAsync(x, d_x, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}
