// pk_ipm.cpp -- what a primal-dual interior-point iteration needs around its solve, computed where x, J and H lie: the barrier
// terms of a boxed vector, the dual residual J^T lambda + grad - z, and the multiplier steps with the step to the boundary.
// Vectors stay on the device; a record of a few doubles comes back.
//
// The boxed vector.  v of length L with bounds lb, ub (which = 0: the n variables with v_lb, v_ub; which = 1: the m slacks of the
// constraint rows with c_lb, c_ub -- the bounds of pk_set_bounds).  Per element: lb == ub is FIXED and has no side; otherwise the
// lower side is present when lb is finite, the upper when ub is.  dl = v - lb, du = ub - v.  An absent side contributes no term:
// nothing of it is read, nothing is multiplied by zero.  A present side is BAD when its slack is not > 0 or not finite, or its
// multiplier is negative or not finite: it is counted, left out of every other column, and its bracket below is 0.0.
//
//   terms     sigma_i = [zl_i / dl] + [zu_i / du],  rbar_i = [mu / dl] - [mu / du]; a single present bracket is stored as it is
//             (the upper one of rbar negated; 0.0 when that side is bad), 0.0 without a side.  The record of 8:
//               0 compl_inf  max |dl zl - mu|, |du zu - mu|        4 log_sum    sum ln dl + sum ln du
//               1 compl_sum  sum dl zl + sum du zu                 5 bad        bad sides
//               2 sides      good sides, counted                   6 z_sum      sum zl + sum zu
//               3 min_slack  min dl, du (+inf without a side)      7 min_compl  min dl zl, du zu (+inf without a side)
//   residual  r_i = t_i - z_i (z NULL: t_i), negated when `negate`; 0.0 for a fixed variable, which reads nothing.  t is what
//             pk_apply_operator_dev (op 1, add = grad) left in r.  The record of 4: 0 r_inf = max |r_i|, 1 r_sq = sum r_i r_i,
//             2 bad (non-finite r_i: stored, left out of 0 and 1), 3 0.0
//   step      dzl_i = (mu / dl - zl_i) - (zl_i / dl) dv_i,  dzu_i = (mu / du - zu_i) + (zu_i / du) dv_i; 0.0 on an absent or bad
//             side.  A candidate is (tau s) / (-ds) for a slack s that decreases (ds < 0): primal dl with ds = dv_i, du with
//             ds = -dv_i; dual zl with ds = dzl_i, zu with ds = dzu_i.  Only candidates < 1 count.  The record of 4:
//               0 alpha_pri = min(1, primal candidates)    2 arg_pri: the smallest index attaining alpha_pri, -1.0 when it is 1
//               1 alpha_dual = min(1, dual candidates)     3 bad: bad sides, plus the elements with a side whose dv_i is not
//                                                            finite (counted once; both steps 0.0, no candidate)
//
// Every product and every quotient is rounded before it is added or subtracted: nothing here contracts to a fused multiply-add.
// / is the correctly rounded one; ln is the platform's (the only column that is not the same bits on the host stand-in).
//
// The association is the pieced one of pk_libkernel.h with this unit's step: index i belongs to piece i / 2048; thread t of
// the piece walks piece * 2048 + t + 256 j, j = 0 ... 7, ascending, within an element the lower side before the upper, from
// the column's identity (0.0 for a sum and for compl_inf, +inf for a min, 1.0 / +inf for a step length and its index); one LDS
// plane per column, the fixed tree of widths 128 ... 1 (slot t = slot t o slot t + w), partial[q * n_pieces + piece]; the scalar
// step is one workgroup: per plane thread t folds the pieces t, t + 256, ... ascending into the identity, the same tree,
// thread 0 fills the record.  o is + for a sum, max / min by comparison, and for (alpha_pri, arg_pri) the pair's
// lexicographic min: the smaller quotient, among equal quotients the smaller index.  No atomics, the same bits from run to run.
// The partial columns are ONE array of the context whatever the stream a call names: the calls of one context must be
// stream-ordered (one stream, or streams ordered by events), as for the other library units.
#include <cmath>

#include "pk_runtime.h"

// Nothing in this unit may contract a * b + c into a fused multiply-add: every product is rounded before it is added.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#include "pk_libkernel.h"      // (behind the pragma: what its templates are instantiated with is this unit's arithmetic)

enum { PK_IP_TERMS = 0, PK_IP_RESID = 1, PK_IP_STEP = 2 };
enum { PK_IP_PLANES = 8, PK_IP_TERMS_REC = 8, PK_IP_REC = 4 };
enum { IP_CINF = 0, IP_CSUM = 1, IP_SIDES = 2, IP_MSLACK = 3, IP_LOG = 4, IP_BAD = 5, IP_ZSUM = 6, IP_MCOMPL = 7 };
enum { IP_RINF = 0, IP_RSQ = 1, IP_RBAD = 2 };
enum { IP_APRI = 0, IP_ADUAL = 1, IP_ARG = 2, IP_SBAD = 3 };

struct PkIpArgs {
  const double *lb, *ub;                  // len values each
  const double *v, *dv, *zl, *zu;         // terms and step
  const double *t, *z;                    // residual: t may alias o1; z may be NULL
  double *o1, *o2;                        // sigma | rbar, r, dzl | dzu
  double *partial, *out;
  int64_t len, n_pieces;
  double mu, tau;
  int32_t kind, planes, negate;
};

PK_LIB_FN int ip_planes(int kind) { return kind == PK_IP_TERMS ? 8 : kind == PK_IP_RESID ? 3 : 4; }
PK_LIB_FN double ip_inf() { return __builtin_inf(); }

PK_LIB_FN double ip_max(double a, double b) { return b > a ? b : a; }
PK_LIB_FN double ip_min(double a, double b) { return b < a ? b : a; }

// the identity of every column of a kind: what a thread without elements, and the scalar step, start from
PK_LIB_FN void ip_identity(int kind, double* a, int64_t stride) {
  if (kind == PK_IP_TERMS) {
    a[IP_CINF * stride] = 0.0; a[IP_CSUM * stride] = 0.0; a[IP_SIDES * stride] = 0.0; a[IP_MSLACK * stride] = ip_inf();
    a[IP_LOG * stride] = 0.0; a[IP_BAD * stride] = 0.0; a[IP_ZSUM * stride] = 0.0; a[IP_MCOMPL * stride] = ip_inf();
  } else if (kind == PK_IP_RESID) {
    a[IP_RINF * stride] = 0.0; a[IP_RSQ * stride] = 0.0; a[IP_RBAD * stride] = 0.0;
  } else {
    a[IP_APRI * stride] = 1.0; a[IP_ADUAL * stride] = 1.0; a[IP_ARG * stride] = ip_inf(); a[IP_SBAD * stride] = 0.0;
  }
}

// a = a o b, column by column (columns `sa` and `sb` doubles apart): the one step of the trees and of the scalar step's trips
PK_LIB_FN void ip_combine(int kind, double* a, int64_t sa, const double* b, int64_t sb) {
  if (kind == PK_IP_TERMS) {
    a[IP_CINF * sa] = ip_max(a[IP_CINF * sa], b[IP_CINF * sb]);
    a[IP_CSUM * sa] = a[IP_CSUM * sa] + b[IP_CSUM * sb];
    a[IP_SIDES * sa] = a[IP_SIDES * sa] + b[IP_SIDES * sb];
    a[IP_MSLACK * sa] = ip_min(a[IP_MSLACK * sa], b[IP_MSLACK * sb]);
    a[IP_LOG * sa] = a[IP_LOG * sa] + b[IP_LOG * sb];
    a[IP_BAD * sa] = a[IP_BAD * sa] + b[IP_BAD * sb];
    a[IP_ZSUM * sa] = a[IP_ZSUM * sa] + b[IP_ZSUM * sb];
    a[IP_MCOMPL * sa] = ip_min(a[IP_MCOMPL * sa], b[IP_MCOMPL * sb]);
  } else if (kind == PK_IP_RESID) {
    a[IP_RINF * sa] = ip_max(a[IP_RINF * sa], b[IP_RINF * sb]);
    a[IP_RSQ * sa] = a[IP_RSQ * sa] + b[IP_RSQ * sb];
    a[IP_RBAD * sa] = a[IP_RBAD * sa] + b[IP_RBAD * sb];
  } else {
    const double qa = a[IP_APRI * sa], qb = b[IP_APRI * sb], ia = a[IP_ARG * sa], ib = b[IP_ARG * sb];
    if (qb < qa || (qb == qa && ib < ia)) {
      a[IP_APRI * sa] = qb;
      a[IP_ARG * sa] = ib;
    }
    a[IP_ADUAL * sa] = ip_min(a[IP_ADUAL * sa], b[IP_ADUAL * sb]);
    a[IP_SBAD * sa] = a[IP_SBAD * sa] + b[IP_SBAD * sb];
  }
}

// one step of the trees of a kind's planes, which share the barrier of the level
PK_LIB_FN void ip_tree_step(double* s, int w, int t, int kind) {
  if (t >= w) return;
  ip_combine(kind, s + t, PK_BLOCK, s + t + w, PK_BLOCK);
}

PK_LIB_FN void ip_sides(double lb, double ub, bool& lo, bool& up) {
  const bool boxed = !(lb == ub);
  lo = boxed && __builtin_isfinite(lb);
  up = boxed && __builtin_isfinite(ub);
}
PK_LIB_FN bool ip_side_ok(double slack, double z) {
  return slack > 0.0 && __builtin_isfinite(slack) && z >= 0.0 && __builtin_isfinite(z);
}

// one good side of the terms into the thread's columns
PK_LIB_FN void ip_terms_side(double d, double z, double mu, double* acc) {
  const double cp = d * z;
  const double off = __builtin_fabs(cp - mu);
  acc[IP_CINF] = ip_max(acc[IP_CINF], off);
  acc[IP_CSUM] = acc[IP_CSUM] + cp;
  acc[IP_SIDES] = acc[IP_SIDES] + 1.0;
  acc[IP_MSLACK] = ip_min(acc[IP_MSLACK], d);
  acc[IP_LOG] = acc[IP_LOG] + log(d);      // (the device library's on the device, libm's in the stand-in)
  acc[IP_ZSUM] = acc[IP_ZSUM] + z;
  acc[IP_MCOMPL] = ip_min(acc[IP_MCOMPL], cp);
}

// ---------------------------------------------------------------- thread t of piece pc: its elements, its columns into the planes
PK_LIB_FN void ip_terms_thread(const PkIpArgs& a, int64_t pc, int t, double* s) {
  double acc[PK_IP_PLANES];
  ip_identity(PK_IP_TERMS, acc, 1);
  for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
    const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
    if (i < a.len) {
      const double lb = a.lb[i], ub = a.ub[i];
      bool lo, up;
      ip_sides(lb, ub, lo, up);
      double sig = 0.0, rb = 0.0;
      if (lo || up) {
        const double v = a.v[i];
        double ql = 0.0, ml = 0.0, qu = 0.0, mu_u = 0.0;
        bool oku = false;
        if (lo) {
          const double d = v - lb, z = a.zl[i];
          if (ip_side_ok(d, z)) {
            ql = z / d;
            ml = a.mu / d;
            ip_terms_side(d, z, a.mu, acc);
          } else {
            acc[IP_BAD] = acc[IP_BAD] + 1.0;
          }
        }
        if (up) {
          const double d = ub - v, z = a.zu[i];
          if (ip_side_ok(d, z)) {
            oku = true;
            qu = z / d;
            mu_u = a.mu / d;
            ip_terms_side(d, z, a.mu, acc);
          } else {
            acc[IP_BAD] = acc[IP_BAD] + 1.0;
          }
        }
        if (lo && up) {
          sig = ql + qu;
          rb = ml - mu_u;
        } else if (lo) {
          sig = ql;
          rb = ml;
        } else {
          sig = qu;
          rb = oku ? -mu_u : 0.0;
        }
      }
      a.o1[i] = sig;
      a.o2[i] = rb;
    }
  }
  for (int q = 0; q < PK_IP_PLANES; ++q) s[q * PK_BLOCK + t] = acc[q];
}

PK_LIB_FN void ip_resid_thread(const PkIpArgs& a, int64_t pc, int t, double* s) {
  double rinf = 0.0, rsq = 0.0, bad = 0.0;
  for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
    const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
    if (i < a.len) {
      double r = 0.0;
      if (!(a.lb[i] == a.ub[i])) {
        r = a.t[i];
        if (a.z) r = r - a.z[i];
        if (a.negate) r = -r;
        if (__builtin_isfinite(r)) {
          const double sq = r * r;
          rinf = ip_max(rinf, __builtin_fabs(r));
          rsq = rsq + sq;
        } else {
          bad = bad + 1.0;
        }
      }
      a.o1[i] = r;
    }
  }
  s[IP_RINF * PK_BLOCK + t] = rinf; s[IP_RSQ * PK_BLOCK + t] = rsq; s[IP_RBAD * PK_BLOCK + t] = bad;
}

// a step length's candidate (tau s) / (-ds) of a slack s that decreases by ds < 0; `neg` = -ds > 0
PK_LIB_FN double ip_candidate(double tau, double s, double neg) {
  const double num = tau * s;
  return num / neg;
}

PK_LIB_FN void ip_step_thread(const PkIpArgs& a, int64_t pc, int t, double* s) {
  double apri = 1.0, adual = 1.0, arg = ip_inf(), bad = 0.0;
  for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
    const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
    if (i < a.len) {
      const double lb = a.lb[i], ub = a.ub[i];
      bool lo, up;
      ip_sides(lb, ub, lo, up);
      double dzl = 0.0, dzu = 0.0;
      if (lo || up) {
        const double v = a.v[i], dv = a.dv[i];
        if (!__builtin_isfinite(dv)) {
          bad = bad + 1.0;
        } else {
          if (lo) {
            const double d = v - lb, z = a.zl[i];
            if (ip_side_ok(d, z)) {
              const double m = a.mu / d, q = z / d;
              const double b = m - z, p = q * dv;
              dzl = b - p;
              if (dv < 0.0) {
                const double cand = ip_candidate(a.tau, d, -dv);
                if (cand < 1.0 && (cand < apri || (cand == apri && (double)i < arg))) {
                  apri = cand;
                  arg = (double)i;
                }
              }
              if (dzl < 0.0) {
                const double cand = ip_candidate(a.tau, z, -dzl);
                if (cand < 1.0) adual = ip_min(adual, cand);
              }
            } else {
              bad = bad + 1.0;
            }
          }
          if (up) {
            const double d = ub - v, z = a.zu[i];
            if (ip_side_ok(d, z)) {
              const double m = a.mu / d, q = z / d;
              const double b = m - z, p = q * dv;
              dzu = b + p;
              if (dv > 0.0) {
                const double cand = ip_candidate(a.tau, d, dv);
                if (cand < 1.0 && (cand < apri || (cand == apri && (double)i < arg))) {
                  apri = cand;
                  arg = (double)i;
                }
              }
              if (dzu < 0.0) {
                const double cand = ip_candidate(a.tau, z, -dzu);
                if (cand < 1.0) adual = ip_min(adual, cand);
              }
            } else {
              bad = bad + 1.0;
            }
          }
        }
      }
      a.o1[i] = dzl;
      a.o2[i] = dzu;
    }
  }
  s[IP_APRI * PK_BLOCK + t] = apri; s[IP_ADUAL * PK_BLOCK + t] = adual; s[IP_ARG * PK_BLOCK + t] = arg; s[IP_SBAD * PK_BLOCK + t] = bad;
}

// thread t of the scalar step: per plane the pieces t, t + 256, ... in ascending order into the identity
PK_LIB_FN void ip_scalar_thread(const PkIpArgs& a, int t, double* s) {
  ip_identity(a.kind, s + t, PK_BLOCK);
  for (int64_t pc = t; pc < a.n_pieces; pc += PK_BLOCK) ip_combine(a.kind, s + t, PK_BLOCK, a.partial + pc, a.n_pieces);
}

// thread 0 of the scalar step behind the trees: plane q ended in s[q * PK_BLOCK]
PK_LIB_FN void ip_scalar_decide(const PkIpArgs& a, const double* s) {
  if (a.kind == PK_IP_TERMS) {
    for (int q = 0; q < PK_IP_TERMS_REC; ++q) a.out[q] = s[q * PK_BLOCK];
  } else if (a.kind == PK_IP_RESID) {
    a.out[0] = s[IP_RINF * PK_BLOCK]; a.out[1] = s[IP_RSQ * PK_BLOCK]; a.out[2] = s[IP_RBAD * PK_BLOCK]; a.out[3] = 0.0;
  } else {
    const double apri = s[IP_APRI * PK_BLOCK];
    a.out[0] = apri; a.out[1] = s[IP_ADUAL * PK_BLOCK]; a.out[2] = apri < 1.0 ? s[IP_ARG * PK_BLOCK] : -1.0;
    a.out[3] = s[IP_SBAD * PK_BLOCK];
  }
}

#ifdef __HIPCC__
// ---------------------------------------------------------------- kernels (gfx950)
__global__ void __launch_bounds__(PK_BLOCK) pk_ip_terms_k(PkIpArgs a) {
  __shared__ double s[PK_IP_PLANES * PK_BLOCK];
  const int t = (int)threadIdx.x;
  for (int64_t pc = (int64_t)blockIdx.x; pc < a.n_pieces; pc += (int64_t)gridDim.x) {
    ip_terms_thread(a, pc, t, s);
    __syncthreads();
    lib_tree(ip_tree_step, s, t, (int)PK_IP_TERMS);
    if (t < 8) lib_store_partial(a, pc, t, s);
    __syncthreads();          // the next piece of this workgroup's stride overwrites the planes
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_ip_resid_k(PkIpArgs a) {
  __shared__ double s[3 * PK_BLOCK];
  const int t = (int)threadIdx.x;
  for (int64_t pc = (int64_t)blockIdx.x; pc < a.n_pieces; pc += (int64_t)gridDim.x) {
    ip_resid_thread(a, pc, t, s);
    __syncthreads();
    lib_tree(ip_tree_step, s, t, (int)PK_IP_RESID);
    if (t < 3) lib_store_partial(a, pc, t, s);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_ip_step_k(PkIpArgs a) {
  __shared__ double s[4 * PK_BLOCK];
  const int t = (int)threadIdx.x;
  for (int64_t pc = (int64_t)blockIdx.x; pc < a.n_pieces; pc += (int64_t)gridDim.x) {
    ip_step_thread(a, pc, t, s);
    __syncthreads();
    lib_tree(ip_tree_step, s, t, (int)PK_IP_STEP);
    if (t < 4) lib_store_partial(a, pc, t, s);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_ip_scalar_k(PkIpArgs a) {
  __shared__ double s[PK_IP_PLANES * PK_BLOCK];
  const int t = (int)threadIdx.x;
  ip_scalar_thread(a, t, s);
  __syncthreads();
  lib_tree(ip_tree_step, s, t, (int)a.kind);
  if (t == 0) ip_scalar_decide(a, s);
}
#else
// ---------------------------------------------------------------- host stand-in: the identical walk
template <class Thread>
static void ip_pieces_host(const PkIpArgs& a, unsigned grid, Thread thread) {
  double s[PK_IP_PLANES * PK_BLOCK];
  lib_walk_host(grid, a.n_pieces, [&](int64_t pc) {
    for (int t = 0; t < PK_BLOCK; ++t) thread(a, pc, t, s);
    lib_tree_host(ip_tree_step, s, (int)a.kind);
    for (int q = 0; q < a.planes; ++q) lib_store_partial(a, pc, q, s);
  });
}
static void ip_terms_host(const PkIpArgs& a, unsigned grid) { ip_pieces_host(a, grid, ip_terms_thread); }
static void ip_resid_host(const PkIpArgs& a, unsigned grid) { ip_pieces_host(a, grid, ip_resid_thread); }
static void ip_step_host(const PkIpArgs& a, unsigned grid) { ip_pieces_host(a, grid, ip_step_thread); }
static void ip_scalar_host(const PkIpArgs& a, unsigned) {
  double s[PK_IP_PLANES * PK_BLOCK];
  for (int t = 0; t < PK_BLOCK; ++t) ip_scalar_thread(a, t, s);
  lib_tree_host(ip_tree_step, s, (int)a.kind);
  ip_scalar_decide(a, s);
}
#endif

void free_ipm(pk_ctx* c) {
  release(c->ipm.d_partial); release(c->ipm.d_scratch);
  c->ipm = PkIpm{};
}

namespace {

// the pieced launch of a kind and the scalar launch behind it; checked by the caller: nothing here refuses but the allocation
int ip_run(pk_ctx* c, PkIpArgs a, int kind, const char* who, void* stream) {
  a.kind = kind; a.planes = ip_planes(kind); a.n_pieces = lib_dot_pieces(a.len);
  if (const int rc = lib_reserve(c, c->ipm.d_partial, c->ipm.partial_cap, (size_t)PK_IP_PLANES * (size_t)a.n_pieces, 136, who, "partial columns"))
    return rc;
  a.partial = c->ipm.d_partial;
  hipStream_t st = pick(c, stream);
  const unsigned grid = lib_grid(a.n_pieces);
  if (kind == PK_IP_TERMS) PK_LIB_LAUNCH(c, pk_ip_terms_k, ip_terms_host, grid, st, a);
  else if (kind == PK_IP_RESID) PK_LIB_LAUNCH(c, pk_ip_resid_k, ip_resid_host, grid, st, a);
  else PK_LIB_LAUNCH(c, pk_ip_step_k, ip_step_host, grid, st, a);
  PK_LIB_LAUNCH(c, pk_ip_scalar_k, ip_scalar_host, 1u, st, a);
  return 0;
}

int ip_not_sharded(pk_ctx* c, const char* who) {
  return (c->shard.flags || c->exchange.world > 1) ? fail(c, 119, "%s: not offered for a sharded context", who) : 0;
}
bool ip_mu_ok(double mu) { return mu >= 0.0 && __builtin_isfinite(mu); }
bool ip_tau_ok(double tau) { return tau > 0.0 && tau <= 1.0; }

// the boxed vector `which` of the context: its length and its bounds (123 without them)
int ip_boxed(pk_ctx* c, int which, PkIpArgs& a, const char* who) {
  if (which != 0 && which != 1) return fail(c, 134, "%s: which = %d (0: the variables, 1: the constraint rows)", who, which);
  if (!c->merit.d_bounds) return fail(c, 123, "%s: no bounds (pk_set_bounds)", who);
  const double* b = c->merit.d_bounds;
  const size_t n = (size_t)c->n, m = (size_t)c->m;
  a.len = which ? c->m : c->n;
  a.lb = which ? b : b + 2 * m;
  a.ub = which ? b + m : b + 2 * m + n;
  return 0;
}

// the host forms' scratch: slices of max(n, m) doubles, the record behind them
struct IpScratch {
  double *a0, *a1, *a2, *a3, *a4, *a5;
};
int ip_scratch(pk_ctx* c, IpScratch& w, double*& rec, const char* who) {
  const size_t L = (size_t)std::max(std::max(c->n, c->m), 1);
  if (const int rc = lib_reserve(c, c->ipm.d_scratch, c->ipm.scratch_cap, 6 * L + PK_IP_TERMS_REC, 136, who, "host-form scratch")) return rc;
  w = lib_slices<IpScratch>(c->ipm.d_scratch, L);
  rec = c->ipm.d_scratch + 6 * L;
  return 0;
}
int ip_download(pk_ctx* c, double* dst, const double* src, size_t count) {
  if (count) PK_HIP(c, hipMemcpyAsync(dst, src, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
  return 0;
}

}  // namespace

extern "C" {

int pk_ip_terms_dev(pk_ctx* c, int which, const double* d_v, const double* d_zl, const double* d_zu, double mu, double* d_sigma,
                    double* d_rbar, double* d_out, void* stream) {
  const char* who = "pk_ip_terms";
  int rc = ready(c);
  if (rc) return rc;
  if (!d_v || !d_zl || !d_zu || !d_sigma || !d_rbar || !d_out) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = ip_not_sharded(c, who))) return rc;
  if (!ip_mu_ok(mu)) return fail(c, 134, "%s: mu = %g (finite, not negative)", who, mu);
  PkIpArgs a{};
  if ((rc = ip_boxed(c, which, a, who))) return rc;
  a.v = d_v; a.zl = d_zl; a.zu = d_zu; a.mu = mu; a.o1 = d_sigma; a.o2 = d_rbar; a.out = d_out;
  return ip_run(c, a, PK_IP_TERMS, who, stream);
}

int pk_dual_residual_dev(pk_ctx* c, const double* d_jvals, const double* d_grad, const double* d_lam, const double* d_z, int negate,
                         double* d_r, double* d_out, void* stream) {
  const char* who = "pk_dual_residual";
  int rc = ready(c);
  if (rc || (rc = ip_not_sharded(c, who)) || (rc = op_ready(c, 1, d_jvals && d_grad && d_lam && d_r && d_out, who))) return rc;
  PkIpArgs a{};
  if ((rc = ip_boxed(c, 0, a, who))) return rc;
  a.t = d_r; a.z = d_z; a.negate = negate != 0; a.o1 = d_r; a.out = d_out;
  // (the partial columns first: nothing is enqueued behind a refusal)
  if ((rc = lib_reserve(c, c->ipm.d_partial, c->ipm.partial_cap, (size_t)PK_IP_PLANES * (size_t)lib_dot_pieces(a.len), 136, who, "partial columns")))
    return rc;
  if ((rc = pk_apply_operator_dev(c, 1, d_jvals, d_lam, d_grad, d_r, stream))) return rc;
  return ip_run(c, a, PK_IP_RESID, who, stream);
}

int pk_ip_step_dev(pk_ctx* c, int which, const double* d_v, const double* d_dv, const double* d_zl, const double* d_zu, double mu,
                   double tau, double* d_dzl, double* d_dzu, double* d_out, void* stream) {
  const char* who = "pk_ip_step";
  int rc = ready(c);
  if (rc) return rc;
  if (!d_v || !d_dv || !d_zl || !d_zu || !d_dzl || !d_dzu || !d_out) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = ip_not_sharded(c, who))) return rc;
  if (!ip_mu_ok(mu) || !ip_tau_ok(tau)) return fail(c, 134, "%s: mu = %g (finite, not negative), tau = %g (in (0, 1])", who, mu, tau);
  PkIpArgs a{};
  if ((rc = ip_boxed(c, which, a, who))) return rc;
  a.v = d_v; a.dv = d_dv; a.zl = d_zl; a.zu = d_zu; a.mu = mu; a.tau = tau; a.o1 = d_dzl; a.o2 = d_dzu; a.out = d_out;
  return ip_run(c, a, PK_IP_STEP, who, stream);
}

int pk_ip_raw_dev(pk_ctx* c, int kind, int64_t len, const double* d_lb, const double* d_ub, const double* d_v, const double* d_dv,
                  const double* d_zl, const double* d_zu, const double* d_t, const double* d_z, int negate, double mu, double tau,
                  double* d_o1, double* d_o2, double* d_out, void* stream) {
  const char* who = "pk_ip_raw";
  int rc = ready(c);
  if (rc) return rc;
  if (kind < PK_IP_TERMS || kind > PK_IP_STEP || len < 0) return fail(c, 134, "%s: kind %d (0, 1 or 2), length %lld", who, kind, (long long)len);
  bool ok = d_lb && d_ub && d_o1 && d_out;
  if (kind == PK_IP_RESID) ok = ok && d_t;
  else ok = ok && d_v && d_zl && d_zu && d_o2 && (kind == PK_IP_TERMS || d_dv);
  if (!ok) return fail(c, 110, "%s: null device pointer", who);
  if (kind != PK_IP_RESID && (!ip_mu_ok(mu) || (kind == PK_IP_STEP && !ip_tau_ok(tau))))
    return fail(c, 134, "%s: mu = %g (finite, not negative), tau = %g (in (0, 1])", who, mu, tau);
  PkIpArgs a{};
  a.lb = d_lb; a.ub = d_ub; a.v = d_v; a.dv = d_dv; a.zl = d_zl; a.zu = d_zu; a.t = d_t; a.z = d_z; a.negate = negate != 0;
  a.mu = mu; a.tau = tau; a.o1 = d_o1; a.o2 = d_o2; a.out = d_out; a.len = len;
  return ip_run(c, a, kind, who, stream);
}

int pk_ip_terms(pk_ctx* c, int which, const double* v, const double* zl, const double* zu, double mu, double* sigma, double* rbar,
                double* out) {
  const char* who = "pk_ip_terms";
  IpScratch w;
  double* rec = nullptr;
  PkIpArgs a{};
  int rc = host_ready(c, v && zl && zu && sigma && rbar && out);
  if (rc || (rc = ip_not_sharded(c, who))) return rc;
  if (!ip_mu_ok(mu)) return fail(c, 134, "%s: mu = %g (finite, not negative)", who, mu);
  if ((rc = ip_boxed(c, which, a, who)) || (rc = ip_scratch(c, w, rec, who))) return rc;
  const size_t L = (size_t)a.len;
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_upload(c, w.a0, v, L)) || (rc = lib_upload(c, w.a1, zl, L)) || (rc = lib_upload(c, w.a2, zu, L))) return rc;
  if ((rc = pk_ip_terms_dev(c, which, w.a0, w.a1, w.a2, mu, w.a3, w.a4, rec, nullptr))) return rc;
  if ((rc = ip_download(c, sigma, w.a3, L)) || (rc = ip_download(c, rbar, w.a4, L)) || (rc = ip_download(c, out, rec, PK_IP_TERMS_REC))) return rc;
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int pk_dual_residual(pk_ctx* c, const double* grad, const double* lam, const double* z, int negate, double* r, double* out) {
  const char* who = "pk_dual_residual";
  const double* jvals = nullptr;
  IpScratch w;
  double* rec = nullptr;
  PkIpArgs a{};
  int rc = host_ready(c, grad && lam && r && out);
  if (rc || (rc = ip_not_sharded(c, who)) || (rc = op_ready(c, 1, true, who)) || (rc = ip_boxed(c, 0, a, who))) return rc;
  if ((rc = op_linearized(c, 1, jvals, who)) || (rc = ip_scratch(c, w, rec, who))) return rc;
  const size_t n = (size_t)c->n, m = (size_t)c->m;
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_upload(c, w.a0, grad, n)) || (rc = lib_upload(c, w.a1, lam, m)) || (rc = lib_upload(c, w.a2, z, n))) return rc;
  if ((rc = pk_dual_residual_dev(c, jvals, w.a0, w.a1, z ? w.a2 : nullptr, negate, w.a3, rec, nullptr))) return rc;
  if ((rc = ip_download(c, r, w.a3, n)) || (rc = ip_download(c, out, rec, PK_IP_REC))) return rc;
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int pk_ip_step(pk_ctx* c, int which, const double* v, const double* dv, const double* zl, const double* zu, double mu, double tau,
               double* dzl, double* dzu, double* out) {
  const char* who = "pk_ip_step";
  IpScratch w;
  double* rec = nullptr;
  PkIpArgs a{};
  int rc = host_ready(c, v && dv && zl && zu && dzl && dzu && out);
  if (rc || (rc = ip_not_sharded(c, who))) return rc;
  if (!ip_mu_ok(mu) || !ip_tau_ok(tau)) return fail(c, 134, "%s: mu = %g (finite, not negative), tau = %g (in (0, 1])", who, mu, tau);
  if ((rc = ip_boxed(c, which, a, who)) || (rc = ip_scratch(c, w, rec, who))) return rc;
  const size_t L = (size_t)a.len;
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_upload(c, w.a0, v, L)) || (rc = lib_upload(c, w.a1, dv, L)) || (rc = lib_upload(c, w.a2, zl, L)) || (rc = lib_upload(c, w.a3, zu, L)))
    return rc;
  if ((rc = pk_ip_step_dev(c, which, w.a0, w.a1, w.a2, w.a3, mu, tau, w.a4, w.a5, rec, nullptr))) return rc;
  if ((rc = ip_download(c, dzl, w.a4, L)) || (rc = ip_download(c, dzu, w.a5, L)) || (rc = ip_download(c, out, rec, PK_IP_REC))) return rc;
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
