// pk_band_refine.cpp -- a solution of the band solve (pk_band.cpp) measured against the TRUE K and refined with the factors in
// place, where the values lie; the device decides when to stop.  A unit of its own beside pk_band.cpp: the ten kernels of the
// family are held to the resources of DESIGN.md section 28, and kernels added to their unit move the panel kernel's registers.
// What this unit needs of the planned system -- its checks, its solve, its record -- it gets through pk_runtime.h.
#include <cmath>

#include "pk_runtime.h"

// Nothing in this unit may contract a * b + c into a fused multiply-add: every product is rounded before it is added.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#include "pk_libkernel.h"      // (behind the pragma: what its templates are instantiated with is this unit's arithmetic)

// A solution x of the planned solve is measured against K as the CSR values state it (q = K x by pk_kkt_apply_dev's fixed-order
// application, not the assembled band) and corrected with the factors in place.  Three kernels beside the family's ten:
//
//   resid     pieced like pk_mr_dot (pieces of 2048, 8 elements per thread).  At an unknown of the plan (where[i] >= 0; where NULL:
//             every element) r_i = b_i - q_i, one rounding.  Four planes per piece: max |r_i|, max |x_i|, max |b_i| and the count
//             of unknowns at which one of r_i, x_i, b_i is not finite; such an element is counted and none of its three values
//             enters a maximum.  Elsewhere r_i = 0.0 and b_i, q_i, x_i are not read.                              [pk_bd_resid_k]
//   scalar    one workgroup reduces the partials (a maximum and an exact count have the same bits in any order), then thread 0
//             writes the record and decides.                                                               [pk_bd_refine_scalar_k]
//   correct   x_i = x_i + d_i at the unknowns, only while the record's status is 0.                            [pk_bd_correct_k]
//
// Step 0 (begin) is q = K x, resid, scalar.  Step t >= 1 is d = K^-1 r by the family's solve (band_planned_solve, not gated by the
// refinement's record), correct, q = K x, resid, scalar.
//
// The record of 8 doubles: 0 status (0 running, 1 converged, 2 stalled, 3 non-finite, 4 the factorisation's own record is not 0:
// nothing is measured and x is untouched); 1 corrections applied; 2 |r|inf; 3 |x|inf; 4 |b|inf; 5 rho now; 6 rho of step 0; 7 the
// rho before this one (0.0 at step 0).  rho = |r|inf / (min(|x|inf, 1e6 |b|inf) + |b|inf), and 0.0 when |r|inf == 0.
// The decision behind step t, in this order: a non-finite count above 0: status 3; t >= min_steps and rho <= tol: status 1; t >= 1
// and rho > (1 - 1e-9) rho_prev: status 2 (the correction that did not help stays in x); otherwise 0.
//
// Freeze rule (MINRES's, pk_minres.cpp).  Once the status is not 0 a further enqueued step runs its solve -- the family's kernels
// are not gated by this record -- and changes nothing else: the correction returns at once, q and r are recomputed to the bits they had, the
// scalar step leaves the record.  x, the record and the status do not depend on how many steps were enqueued beyond the stop; a
// surplus step costs one solve and one application of K.
enum { PK_BR_PLANES = 4, PK_BR_REC = 8, PK_BR_MAX_STEPS = PK_BAND_REFINE_MAX_STEPS };
enum { BR_STATUS = 0, BR_STEPS = 1, BR_RNORM = 2, BR_XNORM = 3, BR_BNORM = 4, BR_RHO = 5, BR_RHO0 = 6, BR_PREV = 7 };
enum { PK_BR_RESID = 0, PK_BR_SCALAR = 1, PK_BR_CORRECT = 2 };
// a step must shrink rho below this factor of the previous one to count as an improvement; |x|inf enters the ratio up to this
// multiple of |b|inf
#define PK_BR_IMPROVE (1.0 - 1.0e-9)
#define PK_BR_XCAP 1.0e6

struct PkBrArgs {
  const int32_t* where;                  // NULL: every element is an unknown
  const double *b, *q, *d, *band_rec;    // band_rec NULL: no factorisation to ask (the raw step form)
  double *x, *r, *rec, *partial;
  int64_t len, n_pieces;
  double tol;
  int32_t min_steps, t, planes;
};

PK_LIB_FN void br_resid_thread(const PkBrArgs& a, int64_t pc, int t, double* s) {
  double mr = 0.0, mx = 0.0, mb = 0.0, bad = 0.0;
  for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
    const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
    if (i < a.len) {
      if (!a.where || a.where[i] >= 0) {
        const double bi = a.b[i], xi = a.x[i];
        const double ri = bi - a.q[i];
        a.r[i] = ri;
        if (__builtin_isfinite(ri) && __builtin_isfinite(xi) && __builtin_isfinite(bi)) {
          const double ar = __builtin_fabs(ri), ax = __builtin_fabs(xi), ab = __builtin_fabs(bi);
          mr = ar > mr ? ar : mr;
          mx = ax > mx ? ax : mx;
          mb = ab > mb ? ab : mb;
        } else {
          bad = bad + 1.0;
        }
      } else {
        a.r[i] = 0.0;
      }
    }
  }
  s[0 * PK_BLOCK + t] = mr; s[1 * PK_BLOCK + t] = mx; s[2 * PK_BLOCK + t] = mb; s[3 * PK_BLOCK + t] = bad;
}

// one level of the four trees: three maxima and the count (a sum of small integers: exact)
PK_LIB_FN void br_planes_step(double* s, int w, int t) {
  if (t >= w) return;
  for (int q = 0; q < 3; ++q) {
    const double u = s[q * PK_BLOCK + t], v = s[q * PK_BLOCK + t + w];
    s[q * PK_BLOCK + t] = v > u ? v : u;
  }
  s[3 * PK_BLOCK + t] = s[3 * PK_BLOCK + t] + s[3 * PK_BLOCK + t + w];
}

// thread t of the scalar step: per plane the pieces t, t + 256, ...
PK_LIB_FN void br_scalar_thread(const PkBrArgs& a, int t, double* s) {
  for (int q = 0; q < PK_BR_PLANES; ++q) {
    double acc = 0.0;
    for (int64_t pc = t; pc < a.n_pieces; pc += PK_BLOCK) {
      const double v = a.partial[(int64_t)q * a.n_pieces + pc];
      if (q < 3) acc = v > acc ? v : acc;
      else acc = acc + v;
    }
    s[q * PK_BLOCK + t] = acc;
  }
}

// thread 0 behind the trees: plane q ended in s[q * PK_BLOCK]
PK_LIB_FN void br_scalar_decide(const PkBrArgs& a, const double* s) {
  double* rec = a.rec;
  if (a.t == 0) {
    for (int k = 0; k < PK_BR_REC; ++k) rec[k] = 0.0;
    if (a.band_rec && a.band_rec[0] != 0.0) { rec[BR_STATUS] = 4.0; return; }
  } else if (rec[BR_STATUS] != 0.0) {
    return;
  }
  const double rn = s[0], xn = s[PK_BLOCK], bn = s[2 * PK_BLOCK], bad = s[3 * PK_BLOCK];
  const double prev = a.t == 0 ? 0.0 : rec[BR_RHO];
  const double cap = PK_BR_XCAP * bn;
  const double den = (xn < cap ? xn : cap) + bn;
  const double rho = rn == 0.0 ? 0.0 : rn / den;
  rec[BR_STEPS] = (double)a.t; rec[BR_RNORM] = rn; rec[BR_XNORM] = xn; rec[BR_BNORM] = bn;
  rec[BR_RHO] = rho; rec[BR_PREV] = prev;
  if (a.t == 0) rec[BR_RHO0] = rho;
  if (bad > 0.0) rec[BR_STATUS] = 3.0;
  else if (a.t >= a.min_steps && rho <= a.tol) rec[BR_STATUS] = 1.0;
  else if (a.t >= 1 && rho > PK_BR_IMPROVE * prev) rec[BR_STATUS] = 2.0;
  else rec[BR_STATUS] = 0.0;
}

PK_LIB_FN void br_correct_element(const PkBrArgs& a, int64_t i) {
  if (!a.where || a.where[i] >= 0) a.x[i] = a.x[i] + a.d[i];
}

#ifdef __HIPCC__
__global__ void __launch_bounds__(PK_BLOCK) pk_bd_resid_k(PkBrArgs a) {
  __shared__ double s[PK_BR_PLANES * PK_BLOCK];
  const int t = (int)threadIdx.x;
  for (int64_t pc = (int64_t)blockIdx.x; pc < a.n_pieces; pc += (int64_t)gridDim.x) {
    br_resid_thread(a, pc, t, s);
    __syncthreads();
    lib_tree(br_planes_step, s, t);
    if (t < PK_BR_PLANES) lib_store_partial(a, pc, t, s);
    __syncthreads();          // the next piece of this workgroup's stride overwrites the planes
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_bd_refine_scalar_k(PkBrArgs a) {
  __shared__ double s[PK_BR_PLANES * PK_BLOCK];
  const int t = (int)threadIdx.x;
  br_scalar_thread(a, t, s);
  __syncthreads();
  lib_tree(br_planes_step, s, t);
  if (t == 0) br_scalar_decide(a, s);
}

__global__ void __launch_bounds__(PK_BLOCK) pk_bd_correct_k(PkBrArgs a) {
  if (a.rec[BR_STATUS] != 0.0) return;      // (uniform over the launch: nobody writes the record while it runs)
  for (int64_t i = (int64_t)blockIdx.x * PK_BLOCK + threadIdx.x; i < a.len; i += (int64_t)gridDim.x * PK_BLOCK) br_correct_element(a, i);
}
#else
static void br_resid_host(const PkBrArgs& a, unsigned grid) {
  double s[PK_BR_PLANES * PK_BLOCK];
  lib_walk_host(grid, a.n_pieces, [&](int64_t pc) {
    for (int t = 0; t < PK_BLOCK; ++t) br_resid_thread(a, pc, t, s);
    lib_tree_host(br_planes_step, s);
    for (int q = 0; q < PK_BR_PLANES; ++q) lib_store_partial(a, pc, q, s);
  });
}
static void br_scalar_host(const PkBrArgs& a, unsigned) {
  double s[PK_BR_PLANES * PK_BLOCK];
  for (int t = 0; t < PK_BLOCK; ++t) br_scalar_thread(a, t, s);
  lib_tree_host(br_planes_step, s);
  br_scalar_decide(a, s);
}
static void br_correct_host(const PkBrArgs& a, unsigned grid) {
  if (a.rec[BR_STATUS] != 0.0) return;
  lib_elements_host(grid, a.len, [&](int64_t i) { br_correct_element(a, i); });
}
#endif

namespace {

// ---------------------------------------------------------------- launches and the context's work
// one of the three kernels on explicit pointers; a.partial holds 4 n_pieces doubles
int br_launch(pk_ctx* c, int step, PkBrArgs a, hipStream_t st) {
  a.n_pieces = lib_dot_pieces(a.len);
  a.planes = PK_BR_PLANES;
  switch (step) {
    case PK_BR_RESID: PK_LIB_LAUNCH(c, pk_bd_resid_k, br_resid_host, lib_grid(a.n_pieces), st, a); break;
    case PK_BR_SCALAR: PK_LIB_LAUNCH(c, pk_bd_refine_scalar_k, br_scalar_host, 1u, st, a); break;
    default:
      if (a.len > 0) PK_LIB_LAUNCH(c, pk_bd_correct_k, br_correct_host, lib_grid(lib_elem_items(a.len)), st, a);
  }
  return 0;
}

bool br_params_ok(double tol, int32_t min_steps) { return solve_tol_ok(tol) && min_steps >= 0 && min_steps <= PK_BR_MAX_STEPS; }

// the slices of the context's work and the arguments of the refinement in progress
struct BrWork {
  double *r, *d, *q, *partial, *rec;
};
BrWork br_work(const pk_ctx* c) {
  const size_t N = (size_t)std::max(c->n + c->m, 1);
  double* w = c->band.d_refine;
  return BrWork{w, w + N, w + 2 * N, w + 3 * N, w + 3 * N + PK_BR_PLANES * (size_t)lib_dot_pieces((int64_t)N)};
}
int br_reserve(pk_ctx* c, const char* who) {
  const size_t N = (size_t)std::max(c->n + c->m, 1);
  return lib_reserve(c, c->band.d_refine, c->band.refine_cap, 3 * N + PK_BR_PLANES * (size_t)lib_dot_pieces((int64_t)N) + PK_BR_REC, 136, who,
                     "the refinement's residual, correction, product, partials and record");
}
PkBrArgs br_args(const pk_ctx* c, int32_t t) {
  const PkBand& b = c->band;
  const BrWork w = br_work(c);
  PkBrArgs a{};
  a.where = b.d_where; a.b = b.rf_rhs; a.q = w.q; a.d = w.d; a.band_rec = band_planned_record(const_cast<pk_ctx*>(c));
  a.x = b.rf_sol; a.r = w.r; a.rec = w.rec; a.partial = w.partial;
  a.len = (int64_t)c->n + c->m; a.tol = b.rf_tol; a.min_steps = b.rf_min_steps; a.t = t;
  return a;
}

// q = K x, the residual and the scalar step t
int br_measure(pk_ctx* c, int32_t t) {
  const PkBand& b = c->band;
  const PkBrArgs a = br_args(c, t);
  int rc;
  if ((rc = pk_kkt_apply_dev(c, b.rf_jvals, b.rf_hvals, b.rf_s1, b.rf_s2, b.rf_sol, const_cast<double*>(a.q), c->stream))) return rc;
  if ((rc = br_launch(c, PK_BR_RESID, a, c->stream))) return rc;
  return br_launch(c, PK_BR_SCALAR, a, c->stream);
}

int br_context(pk_ctx* c, const char* who) {
  if (c->shard.flags || c->exchange.world > 1) return fail(c, 119, "%s: not offered for a sharded context", who);
  return 0;
}

// step t >= 1: d = K^-1 r with the factors in place, the correction, then the measurement
int br_step(pk_ctx* c, int32_t t, const char* who) {
  const BrWork w = br_work(c);
  int rc;
  if ((rc = band_planned_solve(c, w.r, w.d, who)) || (rc = br_launch(c, PK_BR_CORRECT, br_args(c, t), c->stream))) return rc;
  return br_measure(c, t);
}

}  // namespace

extern "C" {

int pk_band_refine_begin_dev(pk_ctx* c, const double* d_hvals, const double* d_jvals, const double* d_s1, const double* d_s2,
                             const double* d_rhs, double* d_sol, double tol, int32_t min_steps) {
  const char* who = "pk_band_refine_begin";
  int rc = ready(c);
  if (rc) return rc;
  if (!d_hvals || !d_jvals || !d_s1 || !d_s2 || !d_rhs || !d_sol) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = solve_ops_ready(c, true, true, who))) return rc;
  if (!br_params_ok(tol, min_steps))
    return fail(c, 134, "%s: tol %g (finite, not negative), min_steps %d (0 ... %d)", who, tol, (int)min_steps, (int)PK_BR_MAX_STEPS);
  if ((rc = band_planned_ready(c, true, who))) return rc;
  if ((rc = br_reserve(c, who)) || (rc = band_planned_partial(c, who))) return rc;
  PkBand& b = c->band;
  b.refining = false;
  b.rf_hvals = d_hvals; b.rf_jvals = d_jvals; b.rf_s1 = d_s1; b.rf_s2 = d_s2; b.rf_rhs = d_rhs; b.rf_sol = d_sol;
  b.rf_tol = tol; b.rf_min_steps = min_steps; b.refine_t = 0;
  if ((rc = br_measure(c, 0))) return rc;
  b.refining = true;
  return 0;
}

int pk_band_refine_advance_dev(pk_ctx* c, int32_t steps) {
  const char* who = "pk_band_refine_advance";
  int rc = ready(c);
  if (rc || (rc = br_context(c, who))) return rc;
  if (steps < 1) return fail(c, 134, "%s: steps = %d, at least one step", who, (int)steps);
  if (!c->band.planned || !c->band.factored || !c->band.refining)
    return fail(c, 135, "%s: no refinement in progress (pk_band_refine_begin_dev)", who);
  for (int32_t k = 0; k < steps; ++k) {
    const int32_t t = c->band.refine_t < INT32_MAX ? c->band.refine_t + 1 : INT32_MAX;      // (reaches the record only while the status is 0)
    if ((rc = br_step(c, t, who))) return rc;
    c->band.refine_t = t;
  }
  return 0;
}

int pk_band_refine_record(pk_ctx* c, double* rec) {
  const char* who = "pk_band_refine_record";
  int rc = ready(c);
  if (rc) return rc;
  if (!rec) return fail(c, 60, "null host buffer");
  if (!c->band.planned || !c->band.factored || !c->band.refining)
    return fail(c, 135, "%s: no refinement in progress (pk_band_refine_begin_dev)", who);
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipMemcpyAsync(rec, br_work(c).rec, sizeof(double) * PK_BR_REC, hipMemcpyDeviceToHost, c->stream));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int pk_solve_banded_refined(pk_ctx* c, const double* s1, const double* s2, const double* b, double* x, double* rec, double* rrec, double tol,
                            int32_t min_steps, int32_t max_steps) {
  const char* who = "pk_solve_banded_refined";
  const double *jvals = nullptr, *hvals = nullptr;
  int rc = host_ready(c, s1 && s2 && b && x && rec && rrec);
  if (rc || (rc = solve_ops_ready(c, true, true, who))) return rc;
  if (!br_params_ok(tol, min_steps) || max_steps < 0 || max_steps > PK_BR_MAX_STEPS)
    return fail(c, 134, "%s: tol %g (finite, not negative), min_steps %d and max_steps %d (0 ... %d)", who, tol, (int)min_steps, (int)max_steps,
                (int)PK_BR_MAX_STEPS);
  if ((rc = band_planned_ready(c, false, who)) || (rc = solve_linearized(c, true, jvals, hvals, who))) return rc;
  const size_t n = (size_t)c->n, m = (size_t)c->m, N = n + m;
  if ((rc = lib_reserve(c, c->band.d_scratch, c->band.scratch_cap, 3 * N + 1, 136, who, "host-form scratch")) || (rc = br_reserve(c, who))) return rc;
  double *d_b = c->band.d_scratch, *d_s = d_b + N, *d_x = d_s + N;
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_upload(c, d_b, b, N)) || (rc = lib_upload(c, d_s, s1, n)) || (rc = lib_upload(c, d_s + n, s2, m))) return rc;
  if ((rc = pk_band_factor_dev(c, hvals, jvals, d_s, d_s + n)) || (rc = pk_band_solve_dev(c, d_b, d_x))) return rc;
  if ((rc = pk_band_refine_begin_dev(c, hvals, jvals, d_s, d_s + n, d_b, d_x, tol, min_steps)) || (rc = pk_band_refine_record(c, rrec))) return rc;
  for (int32_t done = 0; rrec[BR_STATUS] == 0.0 && done < max_steps; ++done)
    if ((rc = pk_band_refine_advance_dev(c, 1)) || (rc = pk_band_refine_record(c, rrec))) return rc;
  if (rrec[BR_STATUS] == 0.0) rrec[BR_STATUS] = 5.0;      // exhausted: in the host copy only
  std::vector<double> got(N + 1);
  if (N) PK_HIP(c, hipMemcpyAsync(got.data(), d_x, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
  if ((rc = pk_band_record(c, rec))) return rc;      // (synchronises)
  if (rec[0] == 0.0) std::copy(got.begin(), got.begin() + (long)N, x);
  return 0;
}

int pk_band_refine_step_dev(pk_ctx* c, int step, int64_t len, const int32_t* d_where, const double* d_b, const double* d_q, double* d_x,
                            const double* d_d, double* d_r, double* d_rec, const double* d_band_rec, double tol, int32_t min_steps, int32_t t) {
  const char* who = "pk_band_refine_step";
  int rc = ready(c);
  if (rc) return rc;
  if (step < PK_BR_RESID || step > PK_BR_CORRECT) return fail(c, 134, "%s: step must be 0 ... 2", who);
  if (len < 0 || t < 0) return fail(c, 134, "%s: length %lld, step number %d", who, (long long)len, (int)t);
  if (step == PK_BR_SCALAR && !br_params_ok(tol, min_steps))
    return fail(c, 134, "%s: tol %g (finite, not negative), min_steps %d (0 ... %d)", who, tol, (int)min_steps, (int)PK_BR_MAX_STEPS);
  const bool ok = step == PK_BR_RESID ? d_b && d_q && d_x && d_r : step == PK_BR_SCALAR ? d_rec != nullptr : d_x && d_d && d_rec;
  if (!ok) return fail(c, 110, "%s: null device pointer", who);
  if (step != PK_BR_CORRECT &&
      (rc = lib_reserve(c, c->band.d_rpartial, c->band.rpartial_cap, PK_BR_PLANES * (size_t)lib_dot_pieces(len), 136, who, "the partials of the residual")))
    return rc;
  PkBrArgs a{};
  a.where = d_where; a.b = d_b; a.q = d_q; a.d = d_d; a.band_rec = d_band_rec; a.x = d_x; a.r = d_r; a.rec = d_rec; a.partial = c->band.d_rpartial;
  a.len = len; a.tol = tol; a.min_steps = min_steps; a.t = t;
  return br_launch(c, step, a, c->stream);
}

}  // extern "C"
