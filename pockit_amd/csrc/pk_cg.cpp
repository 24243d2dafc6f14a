// pk_cg.cpp -- the condensed KKT matrix and the normal equations applied and SOLVED where the linearization lies: preconditioned
// conjugate gradients whose iterations are launches on one stream, with the scalars, the stopping test and the curvature test
// decided on the device.  One call uploads the right-hand side and downloads the solution.
//
// The operator.  form 0 (primal, size n): K v = [H v] + J^T (d o (J v)) + s o v, d of m values, s of n -- H + Sigma + delta I +
// J^T D J, or Gauss-Newton without H.  form 1 (dual, size m): K v = J (d o (J^T v)) + s o v, d of n values, s of m -- the normal
// equations; no H.  d NULL: D = I, no scaling launch (not a multiplication by 1.0); s NULL: no diagonal term.  The products are
// pk_op_rows / pk_op_long (pk_apply_operator_dev) with their association; one application is, in this order,
//
//   1  q = s o v (or 0.0)      2  t = A1 v      3  t = d o t      4  q = H v + q (form 0 with H)      5  q = A2 t + q
//
// A1 = J, A2 = J^T in form 0 and the other way round in form 1; add aliases y in 4 and 5, which the products allow.
//
// The iteration: standard preconditioned CG with a diagonal preconditioner minv (NULL: none).  x, r, z, p, q have the system's
// size, t the other one.  A record of 8 doubles lives on the device:
//
//   0 status      0 running, 1 converged, 2 non-positive curvature, 3 non-finite scalar     4 rz     r.z
//   1 iterations  completed iterations                                                      5 pq     the last p^T K p
//   2 rr          r.r of the recurrence                                                     6 alpha  last step length
//   3 thr         (tol tol) (b.b)                                                           7 beta   last direction factor
//
//   begin      x = x0 or 0.0; r = b - K x0 (r = b without x0); z = minv o r; p = z; q = s o p; b.b, r.z, r.r;
//              thr = (tol tol)(b.b), status = rr <= thr ? 1 : 0, iterations = pq = alpha = beta = 0                [pk_cg_init]
//   iteration  1 the products of p into q (steps 2 ... 5 above: q already holds s o p)
//              2 pq = p.q                                                                       [pk_cg_dot, pk_cg_scalar]
//              3 scalar step A, if status == 0: pq is stored; pq non-finite: status = 3; !(pq > 0): status = 2;
//                otherwise alpha = rz / pq
//              4 update, skipped entirely unless status == 0: x = x + alpha p, r = r - alpha q,
//                z = minv ? minv r : r, and the terms r z and r r of the updated values                           [pk_cg_update]
//              5 scalar step B, skipped unless status == 0: iterations += 1, rr stored; rr or the new r.z
//                non-finite: status = 3; rr <= thr: status = 1; otherwise beta = rz_new / rz, rz = rz_new
//              6 direction: p = z + beta p only when status == 0; q = s o p (or 0.0) always                       [pk_cg_elem]
//
// Once status != 0 further enqueued iterations leave x, r, z, p and the record untouched (q and t are scratch): x, iterations
// and status do not depend on how many iterations were enqueued beyond the stop.
//
// Every product is rounded before its sum: nothing here contracts to a fused multiply-add.  The dots are the pieced dots of
// pk_libkernel.h (pieces of 2048, 8 terms per thread, the fixed tree, the one-workgroup scalar step), one LDS plane per
// simultaneous dot: three in begin (b.b, r.z, r.r), one in the curvature, two in the update (r.z, r.r).  The update's work item
// is a piece (it updates and reduces in one pass); the purely elementwise kernels (direction, t = d o t, the Jacobi reciprocal,
// q = s o v) take 256 elements per item; the grid rule is lib_grid.  The host side of a solve -- the context's arrays, the
// checks, the skeletons of record / advance and of the host form's loop -- is pk_solve.cpp's.
//
// Jacobi: g = diag(K) from pk_operator_reduce_dev (sq_sum, w = d, add = diag H), then a = |g + s|,
// minv = (a > 0 && finite(a)) ? 1 / a : 1.0                                                                          [pk_cg_elem]
#include "pk_runtime.h"

// Nothing in this unit may contract a * b + c into a fused multiply-add: every product is rounded before it is added.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#include "pk_libkernel.h"      // (behind the pragma: what its templates are instantiated with is this unit's arithmetic)

enum { PK_CG_PLANES = 3, PK_CG_REC = 8 };
enum { CG_STATUS = 0, CG_ITERS = 1, CG_RR = 2, CG_THR = 3, CG_RZ = 4, CG_PQ = 5, CG_ALPHA = 6, CG_BETA = 7 };
enum { PK_CG_INIT = 0, PK_CG_CURVATURE = 1, PK_CG_UPDATE = 2, PK_CG_DIRECTION = 3, PK_CG_SCALE = 4, PK_CG_JACOBI = 5,
       PK_CG_DIAG = 6 };      // (PK_CG_DIAG: step 1 of an application, used inside the unit only)

struct PkCgArgs {
  const double *b, *x0, *minv, *s;      // x0, minv and s may be NULL
  double *x, *r, *z, *p, *q;
  double *rec, *partial;
  int64_t len, n_pieces;
  double tol;
  int32_t kind, planes;                 // of the scalar step: PK_CG_INIT, PK_CG_CURVATURE, PK_CG_UPDATE, and the dots it adds
};

// ---------------------------------------------------------------- thread t of piece pc: its elements, its terms into the planes
PK_LIB_FN void cg_init_thread(const PkCgArgs& a, int64_t pc, int t, double* s) {
  double bb = 0.0, rz = 0.0, rr = 0.0;
  for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
    const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
    if (i < a.len) {
      const double bi = a.b[i];
      const double ri = a.x0 ? bi - a.q[i] : bi;      // (with x0 the products left K x0 in q)
      const double zi = a.minv ? a.minv[i] * ri : ri;
      a.x[i] = a.x0 ? a.x0[i] : 0.0;
      a.r[i] = ri;
      a.z[i] = zi;
      a.p[i] = zi;
      a.q[i] = a.s ? a.s[i] * zi : 0.0;
      const double t0 = bi * bi, t1 = ri * zi, t2 = ri * ri;
      bb = bb + t0;
      rz = rz + t1;
      rr = rr + t2;
    }
  }
  s[0 * PK_BLOCK + t] = bb; s[1 * PK_BLOCK + t] = rz; s[2 * PK_BLOCK + t] = rr;
}

PK_LIB_FN void cg_dot_thread(const PkCgArgs& a, int64_t pc, int t, double* s) {
  double pq = 0.0;
  for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
    const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
    if (i < a.len) {
      const double term = a.p[i] * a.q[i];
      pq = pq + term;
    }
  }
  s[t] = pq;
}

PK_LIB_FN void cg_update_thread(const PkCgArgs& a, int64_t pc, int t, double alpha, double* s) {
  double rz = 0.0, rr = 0.0;
  for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
    const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
    if (i < a.len) {
      const double ap = alpha * a.p[i], aq = alpha * a.q[i];
      const double xi = a.x[i] + ap, ri = a.r[i] - aq;
      const double zi = a.minv ? a.minv[i] * ri : ri;
      a.x[i] = xi;
      a.r[i] = ri;
      a.z[i] = zi;
      const double t1 = ri * zi, t2 = ri * ri;
      rz = rz + t1;
      rr = rr + t2;
    }
  }
  s[0 * PK_BLOCK + t] = rz; s[1 * PK_BLOCK + t] = rr;
}

// thread 0 of the scalar step behind the trees: plane q ended in s[q * PK_BLOCK]
PK_LIB_FN void cg_scalar_decide(const PkCgArgs& a, const double* s) {
  double* rec = a.rec;
  if (a.kind == PK_CG_INIT) {
    const double bb = s[0], rz = s[PK_BLOCK], rr = s[2 * PK_BLOCK];
    const double thr = (a.tol * a.tol) * bb;
    rec[CG_STATUS] = rr <= thr ? 1.0 : 0.0;
    rec[CG_ITERS] = 0.0; rec[CG_RR] = rr; rec[CG_THR] = thr; rec[CG_RZ] = rz; rec[CG_PQ] = 0.0; rec[CG_ALPHA] = 0.0; rec[CG_BETA] = 0.0;
    return;
  }
  if (rec[CG_STATUS] != 0.0) return;
  if (a.kind == PK_CG_CURVATURE) {      // scalar step A
    const double pq = s[0];
    rec[CG_PQ] = pq;
    if (!__builtin_isfinite(pq)) rec[CG_STATUS] = 3.0;
    else if (!(pq > 0.0)) rec[CG_STATUS] = 2.0;
    else rec[CG_ALPHA] = rec[CG_RZ] / pq;
  } else {                              // scalar step B
    const double rz = s[0], rr = s[PK_BLOCK];
    rec[CG_ITERS] = rec[CG_ITERS] + 1.0;
    rec[CG_RR] = rr;
    if (!__builtin_isfinite(rr) || !__builtin_isfinite(rz)) rec[CG_STATUS] = 3.0;
    else if (rr <= rec[CG_THR]) rec[CG_STATUS] = 1.0;
    else { rec[CG_BETA] = rz / rec[CG_RZ]; rec[CG_RZ] = rz; }
  }
}

// ---------------------------------------------------------------- the elementwise steps, element i
PK_LIB_FN void cg_dir_element(const PkCgArgs& a, int64_t i, bool running, double beta) {
  double pi = a.p[i];
  if (running) {
    const double bp = beta * pi;
    pi = a.z[i] + bp;
    a.p[i] = pi;
  }
  a.q[i] = a.s ? a.s[i] * pi : 0.0;
}
PK_LIB_FN void cg_scale_element(const PkCgArgs& a, int64_t i) { a.q[i] = a.s[i] * a.q[i]; }
PK_LIB_FN void cg_jacobi_element(const PkCgArgs& a, int64_t i) {
  const double g = a.s ? a.b[i] + a.s[i] : a.b[i];
  const double m = __builtin_fabs(g);
  a.q[i] = (m > 0.0 && __builtin_isfinite(m)) ? 1.0 / m : 1.0;
}
PK_LIB_FN void cg_diag_element(const PkCgArgs& a, int64_t i) { a.q[i] = a.s ? a.s[i] * a.b[i] : 0.0; }

PK_LIB_FN void cg_element(const PkCgArgs& a, int64_t i, bool running, double beta) {
  switch (a.kind) {
    case PK_CG_DIRECTION: cg_dir_element(a, i, running, beta); break;
    case PK_CG_SCALE: cg_scale_element(a, i); break;
    case PK_CG_JACOBI: cg_jacobi_element(a, i); break;
    default: cg_diag_element(a, i); break;
  }
}

#ifdef __HIPCC__
// ---------------------------------------------------------------- kernels (gfx950)
__global__ void __launch_bounds__(PK_BLOCK) pk_cg_init(PkCgArgs a) {
  __shared__ double s[PK_CG_PLANES * PK_BLOCK];
  const int t = (int)threadIdx.x;
  for (int64_t pc = (int64_t)blockIdx.x; pc < a.n_pieces; pc += (int64_t)gridDim.x) {
    cg_init_thread(a, pc, t, s);
    __syncthreads();
    lib_tree(lib_planes_step, s, t, 3);
    if (t < 3) lib_store_partial(a, pc, t, s);
    __syncthreads();          // the next piece of this workgroup's stride overwrites the planes
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_cg_dot(PkCgArgs a) {
  __shared__ double s[PK_BLOCK];
  const int t = (int)threadIdx.x;
  for (int64_t pc = (int64_t)blockIdx.x; pc < a.n_pieces; pc += (int64_t)gridDim.x) {
    cg_dot_thread(a, pc, t, s);
    __syncthreads();
    lib_tree(lib_planes_step, s, t, 1);
    if (t < 1) lib_store_partial(a, pc, t, s);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_cg_update(PkCgArgs a) {
  __shared__ double s[2 * PK_BLOCK];
  const int t = (int)threadIdx.x;
  if (a.rec[CG_STATUS] != 0.0) return;      // (uniform over the launch: nobody writes the record while it runs)
  const double alpha = a.rec[CG_ALPHA];
  for (int64_t pc = (int64_t)blockIdx.x; pc < a.n_pieces; pc += (int64_t)gridDim.x) {
    cg_update_thread(a, pc, t, alpha, s);
    __syncthreads();
    lib_tree(lib_planes_step, s, t, 2);
    if (t < 2) lib_store_partial(a, pc, t, s);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_cg_scalar(PkCgArgs a) {
  __shared__ double s[PK_CG_PLANES * PK_BLOCK];
  const int t = (int)threadIdx.x;
  lib_scalar_thread(a, t, s);
  __syncthreads();
  lib_tree(lib_planes_step, s, t, a.planes);
  if (t == 0) cg_scalar_decide(a, s);
}

__global__ void __launch_bounds__(PK_BLOCK) pk_cg_elem(PkCgArgs a) {
  const bool running = a.kind == PK_CG_DIRECTION && a.rec[CG_STATUS] == 0.0;
  const double beta = running ? a.rec[CG_BETA] : 0.0;
  for (int64_t i = (int64_t)blockIdx.x * PK_BLOCK + threadIdx.x; i < a.len; i += (int64_t)gridDim.x * PK_BLOCK)
    cg_element(a, i, running, beta);
}
#else
// ---------------------------------------------------------------- host stand-in: the identical walk
static void cg_init_host(const PkCgArgs& a, unsigned grid) {
  lib_pieces_host<PK_CG_PLANES>(a, grid, 3, [&](int64_t pc, int t, double* s) { cg_init_thread(a, pc, t, s); });
}
static void cg_dot_host(const PkCgArgs& a, unsigned grid) {
  lib_pieces_host<PK_CG_PLANES>(a, grid, 1, [&](int64_t pc, int t, double* s) { cg_dot_thread(a, pc, t, s); });
}
static void cg_update_host(const PkCgArgs& a, unsigned grid) {
  if (a.rec[CG_STATUS] != 0.0) return;
  const double alpha = a.rec[CG_ALPHA];
  lib_pieces_host<PK_CG_PLANES>(a, grid, 2, [&](int64_t pc, int t, double* s) { cg_update_thread(a, pc, t, alpha, s); });
}
static void cg_scalar_host(const PkCgArgs& a, unsigned) { lib_scalar_host<PK_CG_PLANES>(a, cg_scalar_decide); }
static void cg_elem_host(const PkCgArgs& a, unsigned grid) {
  const bool running = a.kind == PK_CG_DIRECTION && a.rec[CG_STATUS] == 0.0;
  const double beta = running ? a.rec[CG_BETA] : 0.0;
  lib_elements_host(grid, a.len, [&](int64_t i) { cg_element(a, i, running, beta); });
}
#endif

namespace {

size_t cg_len(const pk_ctx* c) { return (size_t)std::max(std::max(c->n, c->m), 1); }

// the context's work vectors and the record, on first use
struct CgWork {
  double *r, *z, *p, *q, *t;
};
int cg_state(pk_ctx* c, const char* who) { return solve_state(c, c->cg, sizeof(CgWork) / sizeof(double*) * cg_len(c), PK_CG_REC, who); }
CgWork cg_work(const pk_ctx* c) { return lib_slices<CgWork>(c->cg.d_work, cg_len(c)); }

// what every entry point that applies K checks before anything is enqueued
int cg_form_ready(pk_ctx* c, int form, bool with_h, bool pointers, const char* who) {
  if (form < 0 || form > 1) return fail(c, 133, "%s: form must be 0 (primal) or 1 (dual)", who);
  if (form == 1 && with_h) return fail(c, 133, "%s: the dual form (1) has no Hessian term", who);
  return solve_ops_ready(c, with_h, pointers, who);
}

int cg_size(const pk_ctx* c, int form) { return form == 0 ? c->n : c->m; }

int cg_launch_elem(pk_ctx* c, const PkCgArgs& a, hipStream_t st) {
  if (a.len > 0) PK_LIB_LAUNCH(c, pk_cg_elem, cg_elem_host, lib_grid(lib_elem_items(a.len)), st, a);
  return 0;
}

int cg_launch_scalar(pk_ctx* c, PkCgArgs a, int kind, int planes, hipStream_t st) {
  a.kind = kind; a.planes = planes;
  PK_LIB_LAUNCH(c, pk_cg_scalar, cg_scalar_host, 1u, st, a);
  return 0;
}

// one vector step on explicit pointers; the partials are reserved by the caller
int cg_step(pk_ctx* c, int step, const PkCgArgs& in, hipStream_t st) {
  PkCgArgs a = in;
  a.n_pieces = lib_dot_pieces(a.len);
  a.partial = c->cg.d_partial;
  a.kind = step;
  const unsigned grid = lib_grid(a.n_pieces);
  switch (step) {
    case PK_CG_INIT:
      PK_LIB_LAUNCH(c, pk_cg_init, cg_init_host, grid, st, a);
      return cg_launch_scalar(c, a, PK_CG_INIT, 3, st);
    case PK_CG_CURVATURE:
      PK_LIB_LAUNCH(c, pk_cg_dot, cg_dot_host, grid, st, a);
      return cg_launch_scalar(c, a, PK_CG_CURVATURE, 1, st);
    case PK_CG_UPDATE:
      PK_LIB_LAUNCH(c, pk_cg_update, cg_update_host, grid, st, a);
      return cg_launch_scalar(c, a, PK_CG_UPDATE, 2, st);
    default:
      return cg_launch_elem(c, a, st);
  }
}

int cg_reserve_partial(pk_ctx* c, int64_t len, const char* who) { return solve_partial(c, c->cg, PK_CG_PLANES, len, who); }

// steps 2 ... 5 of one application: q already holds s o v (or 0.0).  Checked by the caller: nothing here refuses.
int cg_products(pk_ctx* c, int form, const double* jvals, const double* hvals, const double* d, const double* v, double* q, double* t,
                hipStream_t st) {
  int rc;
  const int a1 = form == 0 ? 0 : 1, a2 = 1 - a1;
  if ((rc = pk_apply_operator_dev(c, a1, jvals, v, nullptr, t, st))) return rc;
  if (d) {
    PkCgArgs a{};
    a.s = d; a.q = t; a.len = form == 0 ? c->m : c->n; a.kind = PK_CG_SCALE;
    if ((rc = cg_launch_elem(c, a, st))) return rc;
  }
  if (hvals && (rc = pk_apply_operator_dev(c, 2, hvals, v, q, q, st))) return rc;
  return pk_apply_operator_dev(c, a2, jvals, t, q, q, st);
}

int cg_apply(pk_ctx* c, int form, const double* jvals, const double* hvals, const double* d, const double* s, const double* v,
             double* y, hipStream_t st) {
  PkCgArgs a{};
  a.b = v; a.s = s; a.q = y; a.len = cg_size(c, form); a.kind = PK_CG_DIAG;
  if (const int rc = cg_launch_elem(c, a, st)) return rc;
  return cg_products(c, form, jvals, hvals, d, v, y, cg_work(c).t, st);
}

int cg_iteration(pk_ctx* c, hipStream_t st) {
  const PkCg& g = c->cg;
  const CgWork w = cg_work(c);
  int rc;
  PkCgArgs a{};
  a.minv = g.minv; a.s = g.s; a.x = g.x; a.r = w.r; a.z = w.z; a.p = w.p; a.q = w.q; a.rec = g.d_rec; a.len = cg_size(c, g.form);
  if ((rc = cg_products(c, g.form, g.jvals, g.hvals, g.d, w.p, w.q, w.t, st))) return rc;
  if ((rc = cg_step(c, PK_CG_CURVATURE, a, st)) || (rc = cg_step(c, PK_CG_UPDATE, a, st))) return rc;
  return cg_step(c, PK_CG_DIRECTION, a, st);
}

// the host forms' scratch, max(n, m) doubles each
struct CgScratch {
  double *b, *x0, *x, *d, *s, *minv, *v;
};

}  // namespace

extern "C" {

int pk_cg_step_dev(pk_ctx* c, int step, int64_t len, const double* d_b, const double* d_x0, const double* d_minv, const double* d_s,
                   double* d_x, double* d_r, double* d_z, double* d_p, double* d_q, double* d_rec, double tol, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  const char* who = "pk_cg_step";
  if (step < PK_CG_INIT || step > PK_CG_JACOBI) return fail(c, 134, "%s: step must be 0 ... 5", who);
  if (len < 0) return fail(c, 134, "%s: length %lld", who, (long long)len);
  if (step == PK_CG_INIT && !solve_tol_ok(tol)) return fail(c, 134, "%s: tol must be finite and not negative", who);
  bool ok = true;
  switch (step) {
    case PK_CG_INIT: ok = d_b && d_x && d_r && d_z && d_p && d_q && d_rec; break;
    case PK_CG_CURVATURE: ok = d_p && d_q && d_rec; break;
    case PK_CG_UPDATE: ok = d_x && d_r && d_z && d_p && d_q && d_rec; break;
    case PK_CG_DIRECTION: ok = d_z && d_p && d_q && d_rec; break;
    case PK_CG_SCALE: ok = d_s && d_q; break;
    case PK_CG_JACOBI: ok = d_b && d_q; break;
  }
  if (!ok) return fail(c, 110, "%s: null device pointer", who);
  if (step <= PK_CG_UPDATE && (rc = cg_reserve_partial(c, len, who))) return rc;
  PkCgArgs a{};
  a.b = d_b; a.x0 = d_x0; a.minv = d_minv; a.s = d_s; a.x = d_x; a.r = d_r; a.z = d_z; a.p = d_p; a.q = d_q; a.rec = d_rec;
  a.len = len; a.tol = tol;
  return cg_step(c, step, a, pick(c, stream));
}

int pk_condensed_apply_dev(pk_ctx* c, int form, const double* d_jvals, const double* d_hvals, const double* d_d, const double* d_s,
                           const double* d_v, double* d_y, void* stream) {
  int rc = ready(c);
  if (rc || (rc = cg_form_ready(c, form, d_hvals != nullptr, d_jvals && d_v && d_y, "pk_condensed_apply"))) return rc;
  if ((rc = cg_state(c, "pk_condensed_apply"))) return rc;
  return cg_apply(c, form, d_jvals, d_hvals, d_d, d_s, d_v, d_y, pick(c, stream));
}

int pk_condensed_apply(pk_ctx* c, int form, int with_h, const double* d, const double* s, const double* v, double* y) {
  const char* who = "pk_condensed_apply";
  const double *jvals = nullptr, *hvals = nullptr;
  CgScratch w;
  int rc = host_ready(c, v && y);
  if (rc || (rc = cg_form_ready(c, form, with_h != 0, true, who)) || (rc = solve_linearized(c, with_h != 0, jvals, hvals, who))) return rc;
  if ((rc = cg_state(c, who)) || (rc = solve_scratch(c, c->cg, cg_len(c), w, who))) return rc;
  const size_t N = (size_t)cg_size(c, form), M = (size_t)cg_size(c, 1 - form);
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_upload(c, w.v, v, N)) || (rc = lib_upload(c, w.d, d, M)) || (rc = lib_upload(c, w.s, s, N))) return rc;
  if ((rc = cg_apply(c, form, jvals, hvals, d ? w.d : nullptr, s ? w.s : nullptr, w.v, w.x, c->stream))) return rc;
  if (N) PK_HIP(c, hipMemcpyAsync(y, w.x, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int pk_cg_begin_dev(pk_ctx* c, int form, const double* d_jvals, const double* d_hvals, const double* d_d, const double* d_s,
                    const double* d_minv, const double* d_b, const double* d_x0, double* d_x, double tol, void* stream) {
  const char* who = "pk_cg_begin";
  int rc = ready(c);
  if (rc || (rc = cg_form_ready(c, form, d_hvals != nullptr, d_jvals && d_b && d_x, who))) return rc;
  if (!solve_tol_ok(tol)) return fail(c, 134, "%s: tol must be finite and not negative", who);
  const int64_t N = cg_size(c, form);
  if ((rc = cg_state(c, who)) || (rc = cg_reserve_partial(c, N, who))) return rc;
  hipStream_t st = pick(c, stream);
  const CgWork w = cg_work(c);
  PkCg& g = c->cg;
  solve_forget(g);
  if (d_x0 && (rc = cg_apply(c, form, d_jvals, d_hvals, d_d, d_s, d_x0, w.q, st))) return rc;
  PkCgArgs a{};
  a.b = d_b; a.x0 = d_x0; a.minv = d_minv; a.s = d_s; a.x = d_x; a.r = w.r; a.z = w.z; a.p = w.p; a.q = w.q; a.rec = g.d_rec;
  a.len = N; a.tol = tol;
  if ((rc = cg_step(c, PK_CG_INIT, a, st))) return rc;
  g.active = true; g.form = form; g.jvals = d_jvals; g.hvals = d_hvals; g.d = d_d; g.s = d_s; g.minv = d_minv; g.x = d_x;
  g.stream = st;
  return 0;
}

int pk_cg_advance_dev(pk_ctx* c, int iters, void* stream) {
  if (const int rc = ready(c)) return rc;
  return solve_advance(c, c->cg, iters, stream, cg_iteration, "pk_cg_advance", "pk_cg_begin_dev");
}

int pk_cg_record(pk_ctx* c, double* rec) {
  if (const int rc = ready(c)) return rc;
  return solve_record(c, c->cg, rec, PK_CG_REC, "pk_cg_record", "pk_cg_begin_dev");
}

int pk_solve_condensed(pk_ctx* c, int form, int with_h, const double* d, const double* s, int precond, const double* minv,
                       const double* b, const double* x0, double tol, int maxiter, int check_every, double* x, double* rec) {
  const char* who = "pk_solve_condensed";
  const double *jvals = nullptr, *hvals = nullptr;
  CgScratch w;
  int rc = host_ready(c, b && x && rec && (precond != 2 || minv));
  if (rc || (rc = cg_form_ready(c, form, with_h != 0, true, who))) return rc;
  if ((rc = solve_host_checks(c, with_h != 0, tol, maxiter, check_every, precond, jvals, hvals, who))) return rc;
  const size_t N = (size_t)cg_size(c, form), M = (size_t)cg_size(c, 1 - form);
  if ((rc = cg_state(c, who)) || (rc = solve_scratch(c, c->cg, cg_len(c), w, who)) || (rc = cg_reserve_partial(c, (int64_t)N, who))) return rc;
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_upload(c, w.b, b, N)) || (rc = lib_upload(c, w.x0, x0, N)) || (rc = lib_upload(c, w.d, d, M)) || (rc = lib_upload(c, w.s, s, N))) return rc;
  const double *dd = d ? w.d : nullptr, *ds = s ? w.s : nullptr, *dm = nullptr;
  if (precond == 2) {
    if ((rc = lib_upload(c, w.minv, minv, N))) return rc;
    dm = w.minv;
  } else if (precond == 1) {      // g = diag(K) without s, then minv = 1 / |g + s|
    if (with_h && (rc = pk_operator_diagonal_dev(c, 2, hvals, nullptr, w.minv, nullptr))) return rc;
    if ((rc = pk_operator_reduce_dev(c, form == 0 ? 1 : 0, 1, jvals, dd, with_h ? w.minv : nullptr, w.minv, nullptr))) return rc;
    PkCgArgs a{};
    a.b = w.minv; a.s = ds; a.q = w.minv; a.len = (int64_t)N;
    if ((rc = cg_step(c, PK_CG_JACOBI, a, c->stream))) return rc;
    dm = w.minv;
  }
  if ((rc = pk_cg_begin_dev(c, form, jvals, hvals, dd, ds, dm, w.b, x0 ? w.x0 : nullptr, w.x, tol, nullptr))) return rc;
  return solve_host_loop(c, maxiter, check_every, pk_cg_advance_dev, pk_cg_record, rec, x, w.x, N);
}

}  // extern "C"
