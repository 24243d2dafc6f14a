// pk_minres.cpp -- the augmented KKT system applied and SOLVED where the linearization lies: preconditioned MINRES (Paige and
// Saunders) whose iterations are launches on one stream, with the Lanczos and Givens scalars, the stopping test and the breakdown
// tests decided on the device.  One call uploads the right-hand side and downloads the solution.
//
// The operator, symmetric and indefinite, of size N = n + m:
//
//   K = [ H + diag(s1)     J^T     ]      s1 of n values (NULL: no term), s2 of m values (NULL: no term, pure equalities),
//       [      J       -diag(s2)   ]      H only with its value array
//
// For v = [v1 | v2] and q = [q1 | q2] contiguous one application is, in this order,
//
//   1  q_i = s1 ? s1_i v_i : 0.0 (i < n),  q_i = s2 ? -(s2_(i-n) v_i) : 0.0 (i >= n)      one elementwise launch
//   2  q1 = H v1 + q1 (with H)        3  q1 = J^T v2 + q1        4  q2 = J v1 + q2
//
// 2 ... 4 are pk_op_rows / pk_op_long (pk_apply_operator_dev) with their association; add aliases y, which the products allow.
//
// The iteration.  x, r1, r2, y, v, w, w2, q have length N; minv is a diagonal, positive preconditioner of N values (NULL:
// none).  A record of 16 doubles lives on the device:
//
//   0 status      0 running, 1 converged, 2 preconditioner not positive (r.Mr < 0),     8 epsln
//                 3 non-finite scalar or gamma == 0                                      9 cs
//   1 iterations  completed iterations                                                  10 sn
//   2 phibar      the recurrence's |b - K x| in the M-norm                              11 phi
//   3 thr         tol sqrt(b.(minv o b))                                                12 oldeps
//   4 beta        5 oldb        6 alfa        7 dbar                                    13 delta     14 gamma
//   15 fresh      1 between the scalar step B of a completed iteration and the next scalar step A: the solution update is due
//
//   begin      x = x0 or 0.0; r1 = b - K x0 (r1 = b without x0); r2 = r1; y = minv ? minv o r1 : r1; w = w2 = 0.0; the dots
//              b.(minv o b) and r1.y [pk_mr_init]; then thr = tol sqrt(b.Mb); r1.y non-finite: status 3; r1.y < 0: status 2
//              (beta = phibar = 0.0 in both); otherwise beta = phibar = sqrt(r1.y), status = phibar <= thr ? 1 : 0;
//              oldb = alfa = dbar = epsln = sn = phi = oldeps = delta = gamma = iterations = fresh = 0, cs = -1   [pk_mr_scalar]
//   iteration  1 Lanczos vector: while status == 0, v = (1 / beta) y, the quotient formed by every thread from the record;
//                always step 1 of the application of v into q                                                      [pk_mr_elem]
//              2 the products of v into q (steps 2 ... 4 above)
//              3 alfa = v.q                                                                          [pk_mr_dot, pk_mr_scalar]
//                scalar step A: fresh = 0 whatever the status; if status == 0: alfa stored, alfa non-finite: status 3
//              4 update, skipped entirely unless status == 0: t = q; if iterations >= 1: t = t - (beta / oldb) r1 (the
//                term is skipped on the first iteration, not multiplied by zero); t = t - (alfa / beta) r2; r1 = r2; r2 = t;
//                y = minv ? minv t : t; the term t y into one plane                                              [pk_mr_update]
//              5 scalar step B, skipped unless status == 0, bsq the sum: bsq non-finite: status 3; bsq < 0: status 2;
//                otherwise oldb = beta, beta = sqrt(bsq), oldeps = epsln, delta = cs dbar + sn alfa,
//                gbar = sn dbar - cs alfa, epsln = sn beta, dbar = -(cs beta), gamma = sqrt(gbar gbar + beta beta);
//                !(gamma > 0) or gamma non-finite: status 3; otherwise cs = gbar / gamma, sn = beta / gamma,
//                phi = cs phibar, phibar = sn phibar, iterations += 1, fresh = 1, phibar <= thr: status 1          [pk_mr_scalar]
//              6 solution update, exactly when fresh == 1 (the converging iteration included):
//                wn = ((v - oldeps w2) - delta w) / gamma; w2 = w; w = wn; x = x + phi wn                          [pk_mr_elem]
//
// Freeze rule.  Once status != 0 and the solution update of the stopping iteration has run, further enqueued iterations leave
// x, r1, r2, y, w, w2 and the record's slots 0 ... 14 untouched (v and q are scratch; slot 15 is set to 0 by the next scalar
// step A, which is what keeps the solution update from running twice): x, iterations and status do not depend on how many
// iterations were enqueued beyond the stop.
//
// Every product is rounded before its sum: nothing here contracts to a fused multiply-add.  sqrt and / are the correctly
// rounded ones.  The dots are the pieced dots of pk_libkernel.h (pieces of 2048, 8 terms per thread, the fixed tree, the
// one-workgroup scalar step), one LDS plane per simultaneous dot: two in begin (b.Mb, r1.y), one in the dot and in the update.
// The work item of begin, the dot and the update is a piece; the elementwise kernels take 256 elements per item; the grid rule
// is lib_grid.  The host side of a solve -- the context's arrays, the checks, the skeletons of record / advance and of the
// host form's loop -- is pk_solve.cpp's.
//
// The diagonal preconditioner built on the device (pk_solve_kkt, precond 1): g1 = diag H (pk_operator_diagonal_dev; 0.0 without
// H), minv1 = recip |g1 + s1|; g2_i = sum_j J_ij^2 minv1_j (pk_operator_reduce_dev, sq_sum, w = minv1), minv2 = recip |g2 + s2|;
// recip a = (a > 0 && finite(a)) ? 1 / a : 1.0                                                                      [pk_mr_elem]
#include "pk_runtime.h"

// Nothing in this unit may contract a * b + c into a fused multiply-add: every product is rounded before it is added.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#include "pk_libkernel.h"      // (behind the pragma: what its templates are instantiated with is this unit's arithmetic)

enum { PK_MR_PLANES = 2, PK_MR_REC = 16 };
enum { MR_STATUS = 0, MR_ITERS = 1, MR_PHIBAR = 2, MR_THR = 3, MR_BETA = 4, MR_OLDB = 5, MR_ALFA = 6, MR_DBAR = 7, MR_EPSLN = 8,
       MR_CS = 9, MR_SN = 10, MR_PHI = 11, MR_OLDEPS = 12, MR_DELTA = 13, MR_GAMMA = 14, MR_FRESH = 15 };
enum { PK_MR_INIT = 0, PK_MR_LANCZOS = 1, PK_MR_ALFA = 2, PK_MR_UPDATE = 3, PK_MR_SOLUTION = 4, PK_MR_DIAG = 5, PK_MR_RECIP = 6 };

struct PkMrArgs {
  const double *b, *x0, *minv, *s1, *s2;      // x0, minv, s1 and s2 may be NULL
  double *x, *r1, *r2, *y, *v, *w, *w2, *q;
  double *rec, *partial;
  int64_t len, split, n_pieces;               // split: the first index of the second block (n)
  double tol;
  int32_t kind, planes;                       // of the scalar step: PK_MR_INIT, PK_MR_ALFA, PK_MR_UPDATE, and the dots it adds
};

// what the threads of an elementwise or update launch read from the record, the same in every thread
struct PkMrScalars {
  bool on;
  double c0, c1, c2, c3;
};

// ---------------------------------------------------------------- thread t of piece pc: its elements, its terms into the planes
PK_LIB_FN void mr_init_thread(const PkMrArgs& a, int64_t pc, int t, double* s) {
  double bmb = 0.0, ry = 0.0;
  for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
    const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
    if (i < a.len) {
      const double bi = a.b[i];
      const double ri = a.x0 ? bi - a.q[i] : bi;      // (with x0 the application left K x0 in q)
      const double yi = a.minv ? a.minv[i] * ri : ri;
      const double mb = a.minv ? a.minv[i] * bi : bi;
      a.x[i] = a.x0 ? a.x0[i] : 0.0;
      a.r1[i] = ri;
      a.r2[i] = ri;
      a.y[i] = yi;
      a.w[i] = 0.0;
      a.w2[i] = 0.0;
      const double t0 = bi * mb, t1 = ri * yi;
      bmb = bmb + t0;
      ry = ry + t1;
    }
  }
  s[0 * PK_BLOCK + t] = bmb; s[1 * PK_BLOCK + t] = ry;
}

PK_LIB_FN void mr_dot_thread(const PkMrArgs& a, int64_t pc, int t, double* s) {
  double vq = 0.0;
  for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
    const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
    if (i < a.len) {
      const double term = a.v[i] * a.q[i];
      vq = vq + term;
    }
  }
  s[t] = vq;
}

// the update's scalars: on = past the first iteration, c1 = beta / oldb (then), c2 = alfa / beta
PK_LIB_FN PkMrScalars mr_update_scalars(const double* rec) {
  PkMrScalars k{};
  k.on = rec[MR_ITERS] >= 1.0;
  k.c1 = k.on ? rec[MR_BETA] / rec[MR_OLDB] : 0.0;
  k.c2 = rec[MR_ALFA] / rec[MR_BETA];
  return k;
}

PK_LIB_FN void mr_update_thread(const PkMrArgs& a, int64_t pc, int t, const PkMrScalars& k, double* s) {
  double ty = 0.0;
  for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
    const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
    if (i < a.len) {
      const double r2 = a.r2[i];
      double ti = a.q[i];
      if (k.on) {
        const double p1 = k.c1 * a.r1[i];
        ti = ti - p1;
      }
      const double p2 = k.c2 * r2;
      ti = ti - p2;
      const double yi = a.minv ? a.minv[i] * ti : ti;
      a.r1[i] = r2;
      a.r2[i] = ti;
      a.y[i] = yi;
      const double term = ti * yi;
      ty = ty + term;
    }
  }
  s[t] = ty;
}

// thread 0 of the scalar step behind the trees: plane q ended in s[q * PK_BLOCK]
PK_LIB_FN void mr_scalar_decide(const PkMrArgs& a, const double* s) {
  double* rec = a.rec;
  if (a.kind == PK_MR_INIT) {
    const double bmb = s[0], ry = s[PK_BLOCK];
    const double thr = a.tol * __builtin_sqrt(bmb);
    double status = 0.0, beta = 0.0;
    if (!__builtin_isfinite(ry)) status = 3.0;
    else if (ry < 0.0) status = 2.0;
    else {
      beta = __builtin_sqrt(ry);
      status = beta <= thr ? 1.0 : 0.0;
    }
    for (int k = 0; k < PK_MR_REC; ++k) rec[k] = 0.0;
    rec[MR_STATUS] = status; rec[MR_PHIBAR] = beta; rec[MR_THR] = thr; rec[MR_BETA] = beta; rec[MR_CS] = -1.0;
    return;
  }
  if (a.kind == PK_MR_ALFA) {      // scalar step A
    rec[MR_FRESH] = 0.0;
    if (rec[MR_STATUS] != 0.0) return;
    const double alfa = s[0];
    rec[MR_ALFA] = alfa;
    if (!__builtin_isfinite(alfa)) rec[MR_STATUS] = 3.0;
    return;
  }
  if (rec[MR_STATUS] != 0.0) return;      // scalar step B
  const double bsq = s[0];
  if (!__builtin_isfinite(bsq)) { rec[MR_STATUS] = 3.0; return; }
  if (bsq < 0.0) { rec[MR_STATUS] = 2.0; return; }
  const double cs = rec[MR_CS], sn = rec[MR_SN], dbar = rec[MR_DBAR], alfa = rec[MR_ALFA], phibar = rec[MR_PHIBAR];
  const double beta = __builtin_sqrt(bsq);
  rec[MR_OLDB] = rec[MR_BETA];
  rec[MR_BETA] = beta;
  rec[MR_OLDEPS] = rec[MR_EPSLN];
  const double p0 = cs * dbar, p1 = sn * alfa, p2 = sn * dbar, p3 = cs * alfa, p4 = cs * beta;
  const double delta = p0 + p1, gbar = p2 - p3;
  rec[MR_DELTA] = delta;
  rec[MR_EPSLN] = sn * beta;
  rec[MR_DBAR] = -p4;
  const double g0 = gbar * gbar, g1 = beta * beta;
  const double gamma = __builtin_sqrt(g0 + g1);
  rec[MR_GAMMA] = gamma;
  if (!(gamma > 0.0) || !__builtin_isfinite(gamma)) { rec[MR_STATUS] = 3.0; return; }
  const double cs1 = gbar / gamma, sn1 = beta / gamma;
  const double phibar1 = sn1 * phibar;
  rec[MR_CS] = cs1;
  rec[MR_SN] = sn1;
  rec[MR_PHI] = cs1 * phibar;
  rec[MR_PHIBAR] = phibar1;
  rec[MR_ITERS] = rec[MR_ITERS] + 1.0;
  rec[MR_FRESH] = 1.0;
  if (phibar1 <= rec[MR_THR]) rec[MR_STATUS] = 1.0;
}

// ---------------------------------------------------------------- the elementwise steps, element i
// step 1 of one application of K: the diagonal blocks
PK_LIB_FN double mr_diag_term(const PkMrArgs& a, int64_t i, double vi) {
  if (i < a.split) return a.s1 ? a.s1[i] * vi : 0.0;
  if (!a.s2) return 0.0;
  const double p = a.s2[i - a.split] * vi;
  return -p;
}

PK_LIB_FN PkMrScalars mr_elem_scalars(const PkMrArgs& a) {
  PkMrScalars k{};
  if (a.kind == PK_MR_LANCZOS) {
    k.on = a.rec[MR_STATUS] == 0.0;
    k.c0 = k.on ? 1.0 / a.rec[MR_BETA] : 0.0;
  } else if (a.kind == PK_MR_SOLUTION) {
    k.on = a.rec[MR_FRESH] == 1.0;
    k.c0 = a.rec[MR_OLDEPS]; k.c1 = a.rec[MR_DELTA]; k.c2 = a.rec[MR_GAMMA]; k.c3 = a.rec[MR_PHI];
  }
  return k;
}

PK_LIB_FN void mr_element(const PkMrArgs& a, int64_t i, const PkMrScalars& k) {
  switch (a.kind) {
    case PK_MR_LANCZOS: {
      double vi = a.v[i];
      if (k.on) {
        vi = k.c0 * a.y[i];
        a.v[i] = vi;
      }
      a.q[i] = mr_diag_term(a, i, vi);
      break;
    }
    case PK_MR_SOLUTION: {      // (launched work returns at once unless k.on)
      const double w = a.w[i];
      const double p0 = k.c0 * a.w2[i], p1 = k.c1 * w;
      const double d0 = a.v[i] - p0;
      const double d1 = d0 - p1;
      const double wn = d1 / k.c2;
      const double p2 = k.c3 * wn;
      a.w2[i] = w;
      a.w[i] = wn;
      a.x[i] = a.x[i] + p2;
      break;
    }
    case PK_MR_DIAG: a.q[i] = mr_diag_term(a, i, a.b[i]); break;
    default: {                  // PK_MR_RECIP: q = recip |b + s1| (b NULL: 0.0; s1 NULL: no term)
      double g = a.b ? a.b[i] : 0.0;
      if (a.s1) g = g + a.s1[i];
      const double m = __builtin_fabs(g);
      a.q[i] = (m > 0.0 && __builtin_isfinite(m)) ? 1.0 / m : 1.0;
      break;
    }
  }
}

#ifdef __HIPCC__
// ---------------------------------------------------------------- kernels (gfx950)
__global__ void __launch_bounds__(PK_BLOCK) pk_mr_init(PkMrArgs a) {
  __shared__ double s[PK_MR_PLANES * PK_BLOCK];
  const int t = (int)threadIdx.x;
  for (int64_t pc = (int64_t)blockIdx.x; pc < a.n_pieces; pc += (int64_t)gridDim.x) {
    mr_init_thread(a, pc, t, s);
    __syncthreads();
    lib_tree(lib_planes_step, s, t, 2);
    if (t < 2) lib_store_partial(a, pc, t, s);
    __syncthreads();          // the next piece of this workgroup's stride overwrites the planes
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_mr_dot(PkMrArgs a) {
  __shared__ double s[PK_BLOCK];
  const int t = (int)threadIdx.x;
  for (int64_t pc = (int64_t)blockIdx.x; pc < a.n_pieces; pc += (int64_t)gridDim.x) {
    mr_dot_thread(a, pc, t, s);
    __syncthreads();
    lib_tree(lib_planes_step, s, t, 1);
    if (t < 1) lib_store_partial(a, pc, t, s);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_mr_update(PkMrArgs a) {
  __shared__ double s[PK_BLOCK];
  const int t = (int)threadIdx.x;
  if (a.rec[MR_STATUS] != 0.0) return;      // (uniform over the launch: nobody writes the record while it runs)
  const PkMrScalars k = mr_update_scalars(a.rec);
  for (int64_t pc = (int64_t)blockIdx.x; pc < a.n_pieces; pc += (int64_t)gridDim.x) {
    mr_update_thread(a, pc, t, k, s);
    __syncthreads();
    lib_tree(lib_planes_step, s, t, 1);
    if (t < 1) lib_store_partial(a, pc, t, s);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_mr_scalar(PkMrArgs a) {
  __shared__ double s[PK_MR_PLANES * PK_BLOCK];
  const int t = (int)threadIdx.x;
  lib_scalar_thread(a, t, s);
  __syncthreads();
  lib_tree(lib_planes_step, s, t, a.planes);
  if (t == 0) mr_scalar_decide(a, s);
}

__global__ void __launch_bounds__(PK_BLOCK) pk_mr_elem(PkMrArgs a) {
  const PkMrScalars k = mr_elem_scalars(a);
  if (a.kind == PK_MR_SOLUTION && !k.on) return;
  for (int64_t i = (int64_t)blockIdx.x * PK_BLOCK + threadIdx.x; i < a.len; i += (int64_t)gridDim.x * PK_BLOCK)
    mr_element(a, i, k);
}
#else
// ---------------------------------------------------------------- host stand-in: the identical walk
static void mr_init_host(const PkMrArgs& a, unsigned grid) {
  lib_pieces_host<PK_MR_PLANES>(a, grid, 2, [&](int64_t pc, int t, double* s) { mr_init_thread(a, pc, t, s); });
}
static void mr_dot_host(const PkMrArgs& a, unsigned grid) {
  lib_pieces_host<PK_MR_PLANES>(a, grid, 1, [&](int64_t pc, int t, double* s) { mr_dot_thread(a, pc, t, s); });
}
static void mr_update_host(const PkMrArgs& a, unsigned grid) {
  if (a.rec[MR_STATUS] != 0.0) return;
  const PkMrScalars k = mr_update_scalars(a.rec);
  lib_pieces_host<PK_MR_PLANES>(a, grid, 1, [&](int64_t pc, int t, double* s) { mr_update_thread(a, pc, t, k, s); });
}
static void mr_scalar_host(const PkMrArgs& a, unsigned) { lib_scalar_host<PK_MR_PLANES>(a, mr_scalar_decide); }
static void mr_elem_host(const PkMrArgs& a, unsigned grid) {
  const PkMrScalars k = mr_elem_scalars(a);
  if (a.kind == PK_MR_SOLUTION && !k.on) return;
  lib_elements_host(grid, a.len, [&](int64_t i) { mr_element(a, i, k); });
}
#endif

namespace {

size_t mr_len(const pk_ctx* c) { return (size_t)std::max(c->n + c->m, 1); }

// the context's work vectors and the record, on first use
struct MrWork {
  double *r1, *r2, *y, *v, *w, *w2, *q;
};
int mr_state(pk_ctx* c, const char* who) { return solve_state(c, c->minres, sizeof(MrWork) / sizeof(double*) * mr_len(c), PK_MR_REC, who); }
MrWork mr_work(const pk_ctx* c) { return lib_slices<MrWork>(c->minres.d_work, mr_len(c)); }

int mr_launch_elem(pk_ctx* c, const PkMrArgs& a, hipStream_t st) {
  if (a.len > 0) PK_LIB_LAUNCH(c, pk_mr_elem, mr_elem_host, lib_grid(lib_elem_items(a.len)), st, a);
  return 0;
}

int mr_launch_scalar(pk_ctx* c, PkMrArgs a, int kind, int planes, hipStream_t st) {
  a.kind = kind; a.planes = planes;
  PK_LIB_LAUNCH(c, pk_mr_scalar, mr_scalar_host, 1u, st, a);
  return 0;
}

// one vector step on explicit pointers; the partials are reserved by the caller
int mr_step(pk_ctx* c, int step, const PkMrArgs& in, hipStream_t st) {
  PkMrArgs a = in;
  a.n_pieces = lib_dot_pieces(a.len);
  a.partial = c->minres.d_partial;
  a.kind = step;
  const unsigned grid = lib_grid(a.n_pieces);
  switch (step) {
    case PK_MR_INIT:
      PK_LIB_LAUNCH(c, pk_mr_init, mr_init_host, grid, st, a);
      return mr_launch_scalar(c, a, PK_MR_INIT, 2, st);
    case PK_MR_ALFA:
      PK_LIB_LAUNCH(c, pk_mr_dot, mr_dot_host, grid, st, a);
      return mr_launch_scalar(c, a, PK_MR_ALFA, 1, st);
    case PK_MR_UPDATE:
      PK_LIB_LAUNCH(c, pk_mr_update, mr_update_host, grid, st, a);
      return mr_launch_scalar(c, a, PK_MR_UPDATE, 1, st);
    default:
      return mr_launch_elem(c, a, st);
  }
}

int mr_reserve_partial(pk_ctx* c, int64_t len, const char* who) { return solve_partial(c, c->minres, PK_MR_PLANES, len, who); }

// steps 2 ... 4 of one application: q already holds the diagonal blocks' terms.  Checked by the caller: nothing here refuses.
int mr_products(pk_ctx* c, const double* jvals, const double* hvals, const double* v, double* q, hipStream_t st) {
  int rc;
  const double* v2 = v + c->n;
  double* q2 = q + c->n;
  if (hvals && (rc = pk_apply_operator_dev(c, 2, hvals, v, q, q, st))) return rc;
  if ((rc = pk_apply_operator_dev(c, 1, jvals, v2, q, q, st))) return rc;
  return pk_apply_operator_dev(c, 0, jvals, v, q2, q2, st);
}

int mr_apply(pk_ctx* c, const double* jvals, const double* hvals, const double* s1, const double* s2, const double* v, double* y,
             hipStream_t st) {
  PkMrArgs a{};
  a.b = v; a.s1 = s1; a.s2 = s2; a.q = y; a.len = (int64_t)c->n + c->m; a.split = c->n;
  if (const int rc = mr_step(c, PK_MR_DIAG, a, st)) return rc;
  return mr_products(c, jvals, hvals, v, y, st);
}

int mr_iteration(pk_ctx* c, hipStream_t st) {
  const PkMinres& g = c->minres;
  const MrWork w = mr_work(c);
  int rc;
  PkMrArgs a{};
  a.minv = g.minv; a.s1 = g.s1; a.s2 = g.s2; a.x = g.x; a.r1 = w.r1; a.r2 = w.r2; a.y = w.y; a.v = w.v; a.w = w.w; a.w2 = w.w2; a.q = w.q;
  a.rec = g.d_rec; a.len = (int64_t)c->n + c->m; a.split = c->n;
  if ((rc = mr_step(c, PK_MR_LANCZOS, a, st)) || (rc = mr_products(c, g.jvals, g.hvals, w.v, w.q, st))) return rc;
  if ((rc = mr_step(c, PK_MR_ALFA, a, st)) || (rc = mr_step(c, PK_MR_UPDATE, a, st))) return rc;
  return mr_step(c, PK_MR_SOLUTION, a, st);
}

// the host forms' scratch, n + m doubles each (s: s1 | s2)
struct MrScratch {
  double *b, *x0, *x, *s, *minv, *v;
};

}  // namespace

extern "C" {

int pk_minres_step_dev(pk_ctx* c, int step, int64_t len, int64_t split, const double* d_b, const double* d_x0, const double* d_minv,
                       const double* d_s1, const double* d_s2, double* d_x, double* d_r1, double* d_r2, double* d_y, double* d_v, double* d_w,
                       double* d_w2, double* d_q, double* d_rec, double tol, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  const char* who = "pk_minres_step";
  if (step < PK_MR_INIT || step > PK_MR_RECIP) return fail(c, 134, "%s: step must be 0 ... 6", who);
  if (len < 0 || split < 0 || split > len) return fail(c, 134, "%s: length %lld, split %lld", who, (long long)len, (long long)split);
  if (step == PK_MR_INIT && !solve_tol_ok(tol)) return fail(c, 134, "%s: tol must be finite and not negative", who);
  bool ok = true;
  switch (step) {
    case PK_MR_INIT: ok = d_b && d_x && d_r1 && d_r2 && d_y && d_w && d_w2 && d_rec && (!d_x0 || d_q); break;
    case PK_MR_LANCZOS: ok = d_y && d_v && d_q && d_rec; break;
    case PK_MR_ALFA: ok = d_v && d_q && d_rec; break;
    case PK_MR_UPDATE: ok = d_r1 && d_r2 && d_y && d_q && d_rec; break;
    case PK_MR_SOLUTION: ok = d_x && d_v && d_w && d_w2 && d_rec; break;
    case PK_MR_DIAG: ok = d_b && d_q; break;
    case PK_MR_RECIP: ok = d_q != nullptr; break;
  }
  if (!ok) return fail(c, 110, "%s: null device pointer", who);
  if ((step == PK_MR_INIT || step == PK_MR_ALFA || step == PK_MR_UPDATE) && (rc = mr_reserve_partial(c, len, who))) return rc;
  PkMrArgs a{};
  a.b = d_b; a.x0 = d_x0; a.minv = d_minv; a.s1 = d_s1; a.s2 = d_s2; a.x = d_x; a.r1 = d_r1; a.r2 = d_r2; a.y = d_y; a.v = d_v; a.w = d_w;
  a.w2 = d_w2; a.q = d_q; a.rec = d_rec; a.len = len; a.split = split; a.tol = tol;
  return mr_step(c, step, a, pick(c, stream));
}

int pk_kkt_apply_dev(pk_ctx* c, const double* d_jvals, const double* d_hvals, const double* d_s1, const double* d_s2, const double* d_v,
                     double* d_y, void* stream) {
  int rc = ready(c);
  if (rc || (rc = solve_ops_ready(c, d_hvals != nullptr, d_jvals && d_v && d_y, "pk_kkt_apply"))) return rc;
  return mr_apply(c, d_jvals, d_hvals, d_s1, d_s2, d_v, d_y, pick(c, stream));
}

int pk_kkt_apply(pk_ctx* c, int with_h, const double* s1, const double* s2, const double* v, double* y) {
  const char* who = "pk_kkt_apply";
  const double *jvals = nullptr, *hvals = nullptr;
  MrScratch w;
  int rc = host_ready(c, v && y);
  if (rc || (rc = solve_ops_ready(c, with_h != 0, true, who)) || (rc = solve_linearized(c, with_h != 0, jvals, hvals, who))) return rc;
  if ((rc = solve_scratch(c, c->minres, mr_len(c), w, who))) return rc;
  const size_t n = (size_t)c->n, m = (size_t)c->m, N = n + m;
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_upload(c, w.v, v, N)) || (rc = lib_upload(c, w.s, s1, n)) || (rc = lib_upload(c, w.s + n, s2, m))) return rc;
  if ((rc = mr_apply(c, jvals, hvals, s1 ? w.s : nullptr, s2 ? w.s + n : nullptr, w.v, w.x, c->stream))) return rc;
  if (N) PK_HIP(c, hipMemcpyAsync(y, w.x, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int pk_minres_begin_dev(pk_ctx* c, const double* d_jvals, const double* d_hvals, const double* d_s1, const double* d_s2,
                        const double* d_minv, const double* d_b, const double* d_x0, double* d_x, double tol, void* stream) {
  const char* who = "pk_minres_begin";
  int rc = ready(c);
  if (rc || (rc = solve_ops_ready(c, d_hvals != nullptr, d_jvals && d_b && d_x, who))) return rc;
  if (!solve_tol_ok(tol)) return fail(c, 134, "%s: tol must be finite and not negative", who);
  const int64_t N = (int64_t)c->n + c->m;
  if ((rc = mr_state(c, who)) || (rc = mr_reserve_partial(c, N, who))) return rc;
  hipStream_t st = pick(c, stream);
  const MrWork w = mr_work(c);
  PkMinres& g = c->minres;
  solve_forget(g);
  if (d_x0 && (rc = mr_apply(c, d_jvals, d_hvals, d_s1, d_s2, d_x0, w.q, st))) return rc;
  PkMrArgs a{};
  a.b = d_b; a.x0 = d_x0; a.minv = d_minv; a.x = d_x; a.r1 = w.r1; a.r2 = w.r2; a.y = w.y; a.v = w.v; a.w = w.w; a.w2 = w.w2; a.q = w.q;
  a.rec = g.d_rec; a.len = N; a.split = c->n; a.tol = tol;
  if ((rc = mr_step(c, PK_MR_INIT, a, st))) return rc;
  g.active = true; g.jvals = d_jvals; g.hvals = d_hvals; g.s1 = d_s1; g.s2 = d_s2; g.minv = d_minv; g.x = d_x;
  g.stream = st;
  return 0;
}

int pk_minres_advance_dev(pk_ctx* c, int iters, void* stream) {
  if (const int rc = ready(c)) return rc;
  return solve_advance(c, c->minres, iters, stream, mr_iteration, "pk_minres_advance", "pk_minres_begin_dev");
}

int pk_minres_record(pk_ctx* c, double* rec) {
  int rc = ready(c);
  if (rc || (rc = solve_record(c, c->minres, rec, PK_MR_REC, "pk_minres_record", "pk_minres_begin_dev"))) return rc;
  rec[MR_FRESH] = 0.0;      // internal: between two iterations the solution update has always run
  return 0;
}

int pk_solve_kkt(pk_ctx* c, int with_h, const double* s1, const double* s2, int precond, const double* minv, const double* b,
                 const double* x0, double tol, int maxiter, int check_every, double* x, double* rec) {
  const char* who = "pk_solve_kkt";
  const double *jvals = nullptr, *hvals = nullptr;
  MrScratch w;
  int rc = host_ready(c, b && x && rec && (precond != 2 || minv));
  if (rc || (rc = solve_ops_ready(c, with_h != 0, true, who))) return rc;
  if ((rc = solve_host_checks(c, with_h != 0, tol, maxiter, check_every, precond, jvals, hvals, who))) return rc;
  const size_t n = (size_t)c->n, m = (size_t)c->m, N = n + m;
  if ((rc = mr_state(c, who)) || (rc = solve_scratch(c, c->minres, mr_len(c), w, who)) || (rc = mr_reserve_partial(c, (int64_t)N, who))) return rc;
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_upload(c, w.b, b, N)) || (rc = lib_upload(c, w.x0, x0, N)) || (rc = lib_upload(c, w.s, s1, n)) || (rc = lib_upload(c, w.s + n, s2, m))) return rc;
  const double *d1 = s1 ? w.s : nullptr, *d2 = s2 ? w.s + n : nullptr, *dm = nullptr;
  if (precond == 2) {
    if ((rc = lib_upload(c, w.minv, minv, N))) return rc;
    dm = w.minv;
  } else if (precond == 1) {      // minv1 = recip |diag H + s1|, then minv2 = recip |sum_j J_ij^2 minv1_j + s2|
    if (with_h && (rc = pk_operator_diagonal_dev(c, 2, hvals, nullptr, w.minv, nullptr))) return rc;
    PkMrArgs a{};
    a.b = with_h ? w.minv : nullptr; a.s1 = d1; a.q = w.minv; a.len = (int64_t)n;
    if ((rc = mr_step(c, PK_MR_RECIP, a, c->stream))) return rc;
    if ((rc = pk_operator_reduce_dev(c, 0, 1, jvals, w.minv, nullptr, w.minv + n, nullptr))) return rc;
    a.b = w.minv + n; a.s1 = d2; a.q = w.minv + n; a.len = (int64_t)m;
    if ((rc = mr_step(c, PK_MR_RECIP, a, c->stream))) return rc;
    dm = w.minv;
  }
  if ((rc = pk_minres_begin_dev(c, jvals, hvals, d1, d2, dm, w.b, x0 ? w.x0 : nullptr, w.x, tol, nullptr))) return rc;
  return solve_host_loop(c, maxiter, check_every, pk_minres_advance_dev, pk_minres_record, rec, x, w.x, N);
}

}  // extern "C"
