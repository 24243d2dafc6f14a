// pk_slack.cpp -- what a resident primal-dual iterate with slacks needs beside pk_ipm.cpp, computed where the vectors lie: the
// elimination of the slacks from the step's system, the recovery of their step with the terms of the curvature test, the update
// of a boxed vector and its multipliers with the multiplier safeguard, and the barrier merit terms of trial points that carry
// slacks.  Vectors stay on the device; a record of a few doubles comes back.
//
// Rows are classified as pk_ipm.cpp classifies the boxed vector which = 1: c_lb == c_ub is an EQUALITY row (no slack, nothing
// of s, lam's barrier terms or the slack's multipliers is read there); any other row is an INEQUALITY row g_i - s_i = 0 whose
// slack s_i is boxed by the finite ones of c_lb_i, c_ub_i.  A variable with v_lb == v_ub is FIXED and takes part in nothing:
// nothing of it is read or written.  A side is present as in pk_ipm.cpp.
//
//   reduce    equality:   s2_i = 0.0,          b2_i = -(g_i - c_lb_i)
//             inequality: s2_i = 1 / sigma_s_i, b2_i = (-(g_i - s_i)) + s2_i (lam_i + rbar_s_i)
//             A sigma_s_i that is not > 0 or not finite is BAD: counted, s2_i = b2_i = 0.0, out of the other columns.  A residual
//             that is not finite is counted in bad as well and left out of the two norms (s2_i, b2_i stored as computed).
//             The record of 4: 0 theta_inf = max |g - c|, |g - s|; 1 theta_1, the sum of the same; 2 bad; 3 inequality rows
//   recover   ds_i = s2_i ((dlam_i + lam_i) + rbar_s_i) on inequality rows (0.0 on a bad sigma_s_i, counted), 0.0 on equality
//             rows.  The record of 5 over the free variables and the inequality rows:
//               0 sum (dx_i w_i + s1_i dx_i^2)   1 sum sigma_s_i ds_i^2   2 sum dx_i^2   3 sum ds_i^2
//               4 bad: bad sigma_s_i, non-finite ds_i (stored), non-finite dx_i w_i + s1_i dx_i^2; each left out of 0 ... 3
//   update    in place, on a boxed vector of length L with its bounds: v_i += alpha_p dv_i on every element that is not fixed;
//             on a present side z_i += alpha_d dz_i, then with the NEW slack d (v_i - lb_i or ub_i - v_i)
//             z_i = min(max(z_i, mu / (kappa d)), (kappa mu) / d).  With lam (a length L = m, which = 1 only):
//             lam_i += alpha_p dlam_i on EVERY row, equality rows included.  The record of 4: 0 clamped multipliers; 1 the
//             smallest new slack (+inf without a side); 2 bad: a new v_i or lam_i that is not finite (the element's
//             multipliers then stored unclamped), a new slack that is not > 0, a new multiplier that is not finite (stored
//             as computed, unclamped, out of 0 and 1); 3 0.0
//   merit     per entry b of a batch, trial point X[b] (n), its constraint values G[b] (m), the slacks st = s + alpha_b ds:
//               0 theta_1 = sum_eq |g - c| + sum_ineq |g - st|   1 theta_inf, the max of the same
//               2 log_sum = sum ln over the present sides of X[b] and of st
//               3 bad: a side whose slack is not > 0 or not finite, a residual that is not finite; left out of 0, 1, 2
//
// Every product and every quotient is rounded before it is added or subtracted: nothing here contracts to a fused multiply-add.
// / is the correctly rounded one; ln is the platform's (the only column that is not the same bits on the host stand-in).
//
// The association is the pieced one of pk_libkernel.h.  reduce and update walk one index range: index i belongs to piece
// i / 2048.  recover and merit walk two: the variables' pieces first (ceil(n / 2048) of them), the rows' pieces behind them
// (ceil(m / 2048)); a piece lies wholly in one range.  Thread t of a piece walks its base + t + 256 j, j = 0 ... 7, ascending,
// within a variable or a row the residual before the sides and the lower side before the upper, from the column's identity
// (0.0 for a sum and a max, +inf for a min); one LDS plane per column, the fixed tree of widths 128 ... 1, the partial
// [(entry * planes + q) * n_pieces + piece] (entry 0 outside a batch).  The scalar step is one workgroup per entry: per plane
// thread t folds the pieces t, t + 256, ... ascending into the identity, the same tree, thread 0 fills the entry's record.  The
// entries of a batch never meet.  No atomics, the same bits from run to run.  The partial columns are ONE array of the context
// whatever the stream a call names: the calls of one context must be stream-ordered, as for the other library units.
#include <cmath>

#include "pk_runtime.h"

// Nothing in this unit may contract a * b + c into a fused multiply-add: every product is rounded before it is added.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#include "pk_libkernel.h"      // (behind the pragma: what its templates are instantiated with is this unit's arithmetic)

enum { PK_SL_REDUCE = 0, PK_SL_RECOVER = 1, PK_SL_UPDATE = 2, PK_SL_MERIT = 3 };
enum { PK_SL_PLANES = 5, PK_SL_SLOTS = 10 };
enum { SL_SUM = 0, SL_MAX = 1, SL_MIN = 2 };

// the pointers of a kind, in the order of pk_slack_raw_dev:
//   reduce   0 g, 1 s, 2 lam, 3 sigma_s, 4 rbar_s, 5 s2 (out), 6 b2 (out)
//   recover  0 dlam, 1 lam, 2 rbar_s, 3 s2, 4 sigma_s, 5 dx, 6 w, 7 s1, 8 ds (out)
//   update   0 v, 1 dv, 2 zl, 3 dzl, 4 zu, 5 dzu, 6 lam or NULL, 7 dlam or NULL     (0, 2, 4, 6 in place)
//   merit    0 X, 1 G, 2 s, 3 ds, 4 alphas
struct PkSlackArgs {
  const double *xlb, *xub;                // the variables' bounds (n): recover, merit
  const double *clb, *cub;                // the rows' bounds (m); update: the boxed vector's (m is its length)
  double* p[PK_SL_SLOTS];
  double *partial, *out;
  int64_t n, m, x_pieces, n_pieces, batch;
  double alpha_p, alpha_d, mu, kappa;
  int32_t kind, planes;
};

PK_LIB_FN int sl_planes(int kind) { return kind == PK_SL_RECOVER ? 5 : kind == PK_SL_UPDATE ? 3 : 4; }
PK_LIB_FN int sl_record(int kind) { return kind == PK_SL_RECOVER ? 5 : 4; }
PK_LIB_FN double sl_inf() { return __builtin_inf(); }
PK_LIB_FN double sl_max(double a, double b) { return b > a ? b : a; }
PK_LIB_FN double sl_min(double a, double b) { return b < a ? b : a; }

// how column q of a kind is folded
PK_LIB_FN int sl_op(int kind, int q) {
  if (kind == PK_SL_REDUCE) return q == 0 ? SL_MAX : SL_SUM;
  if (kind == PK_SL_UPDATE) return q == 1 ? SL_MIN : SL_SUM;
  if (kind == PK_SL_MERIT) return q == 1 ? SL_MAX : SL_SUM;
  return SL_SUM;
}
PK_LIB_FN double sl_identity(int op) { return op == SL_MIN ? sl_inf() : 0.0; }
PK_LIB_FN double sl_fold(int op, double a, double b) { return op == SL_SUM ? a + b : op == SL_MAX ? sl_max(a, b) : sl_min(a, b); }

// one step of the trees of a kind's planes, which share the barrier of the level
PK_LIB_FN void sl_tree_step(double* s, int w, int t, int kind) {
  if (t >= w) return;
  const int planes = sl_planes(kind);
  for (int q = 0; q < planes; ++q) s[q * PK_BLOCK + t] = sl_fold(sl_op(kind, q), s[q * PK_BLOCK + t], s[q * PK_BLOCK + t + w]);
}

PK_LIB_FN void sl_sides(double lb, double ub, bool& lo, bool& up) {
  const bool boxed = !(lb == ub);
  lo = boxed && __builtin_isfinite(lb);
  up = boxed && __builtin_isfinite(ub);
}
PK_LIB_FN bool sl_positive(double d) { return d > 0.0 && __builtin_isfinite(d); }

// ---------------------------------------------------------------- thread t of piece pc: its elements, its columns into the planes
PK_LIB_FN void sl_reduce_thread(const PkSlackArgs& a, int64_t pc, int t, double* s) {
  double tinf = 0.0, t1 = 0.0, bad = 0.0, rows = 0.0;
  for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
    const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
    if (i < a.m) {
      const double lb = a.clb[i], ub = a.cub[i];
      double s2 = 0.0, b2 = 0.0, r = 0.0;
      bool good = true;
      if (lb == ub) {
        r = a.p[0][i] - lb;
        b2 = -r;
      } else {
        rows = rows + 1.0;
        const double sig = a.p[3][i];
        if (sl_positive(sig)) {
          s2 = 1.0 / sig;
          r = a.p[0][i] - a.p[1][i];
          const double z = a.p[2][i] + a.p[4][i];
          const double q = s2 * z;
          b2 = (-r) + q;
        } else {
          good = false;
        }
      }
      if (good && __builtin_isfinite(r)) {
        const double ar = __builtin_fabs(r);
        tinf = sl_max(tinf, ar);
        t1 = t1 + ar;
      } else {
        bad = bad + 1.0;
      }
      a.p[5][i] = s2;
      a.p[6][i] = b2;
    }
  }
  s[0 * PK_BLOCK + t] = tinf; s[1 * PK_BLOCK + t] = t1; s[2 * PK_BLOCK + t] = bad; s[3 * PK_BLOCK + t] = rows;
}

PK_LIB_FN void sl_recover_thread(const PkSlackArgs& a, int64_t pc, int t, double* s) {
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0, bad = 0.0;
  if (pc < a.x_pieces) {
    for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
      const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
      if (i < a.n && !(a.xlb[i] == a.xub[i])) {
        const double dx = a.p[5][i];
        const double pw = dx * a.p[6][i], sq = dx * dx;
        const double e = a.p[7][i] * sq;
        const double term = pw + e;
        if (__builtin_isfinite(term)) {
          c0 = c0 + term;
          c2 = c2 + sq;
        } else {
          bad = bad + 1.0;
        }
      }
    }
  } else {
    for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
      const int64_t i = (pc - a.x_pieces) * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
      if (i < a.m) {
        double ds = 0.0;
        if (!(a.clb[i] == a.cub[i])) {
          const double sig = a.p[4][i];
          if (sl_positive(sig)) {
            const double u = a.p[0][i] + a.p[1][i];
            const double z = u + a.p[2][i];
            ds = a.p[3][i] * z;
            if (__builtin_isfinite(ds)) {
              const double sq = ds * ds;
              const double e = sig * sq;
              c1 = c1 + e;
              c3 = c3 + sq;
            } else {
              bad = bad + 1.0;
            }
          } else {
            bad = bad + 1.0;
          }
        }
        a.p[8][i] = ds;
      }
    }
  }
  s[0 * PK_BLOCK + t] = c0; s[1 * PK_BLOCK + t] = c1; s[2 * PK_BLOCK + t] = c2; s[3 * PK_BLOCK + t] = c3; s[4 * PK_BLOCK + t] = bad;
}

// one present side behind the update of its element: the multiplier's step, then the safeguard with the new slack d
PK_LIB_FN void sl_update_side(const PkSlackArgs& a, double* z, const double* dz, int64_t i, double d, bool fin, double& clamped,
                              double& mins, double& bad) {
  const double pz = a.alpha_d * dz[i];
  const double zn = z[i] + pz;
  double zc = zn;
  if (fin) {
    if (!sl_positive(d) || !__builtin_isfinite(zn)) {
      bad = bad + 1.0;
    } else {
      const double kd = a.kappa * d, km = a.kappa * a.mu;
      const double low = a.mu / kd, high = km / d;
      if (zc < low) zc = low;
      if (zc > high) zc = high;
      if (!(zc == zn)) clamped = clamped + 1.0;
      mins = sl_min(mins, d);
    }
  }
  z[i] = zc;
}

PK_LIB_FN void sl_update_thread(const PkSlackArgs& a, int64_t pc, int t, double* s) {
  double clamped = 0.0, mins = sl_inf(), bad = 0.0;
  for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
    const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
    if (i < a.m) {
      if (a.p[6]) {
        const double pl = a.alpha_p * a.p[7][i];
        const double ln = a.p[6][i] + pl;
        if (!__builtin_isfinite(ln)) bad = bad + 1.0;
        a.p[6][i] = ln;
      }
      const double lb = a.clb[i], ub = a.cub[i];
      if (!(lb == ub)) {
        const double pv = a.alpha_p * a.p[1][i];
        const double vn = a.p[0][i] + pv;
        const bool fin = __builtin_isfinite(vn);
        if (!fin) bad = bad + 1.0;
        a.p[0][i] = vn;
        if (__builtin_isfinite(lb)) sl_update_side(a, a.p[2], a.p[3], i, vn - lb, fin, clamped, mins, bad);
        if (__builtin_isfinite(ub)) sl_update_side(a, a.p[4], a.p[5], i, ub - vn, fin, clamped, mins, bad);
      }
    }
  }
  s[0 * PK_BLOCK + t] = clamped; s[1 * PK_BLOCK + t] = mins; s[2 * PK_BLOCK + t] = bad;
}

// a present side of a trial point: its logarithm, or bad
PK_LIB_FN void sl_merit_side(double d, double& lsum, double& bad) {
  if (sl_positive(d)) lsum = lsum + log(d);      // (the device library's on the device, libm's in the stand-in)
  else bad = bad + 1.0;
}

PK_LIB_FN void sl_merit_thread(const PkSlackArgs& a, int64_t entry, int64_t pc, int t, double* s) {
  double t1 = 0.0, tinf = 0.0, lsum = 0.0, bad = 0.0;
  if (pc < a.x_pieces) {
    const double* x = a.p[0] + entry * a.n;
    for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
      const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
      if (i < a.n) {
        const double lb = a.xlb[i], ub = a.xub[i];
        bool lo, up;
        sl_sides(lb, ub, lo, up);
        if (lo || up) {
          const double v = x[i];
          if (lo) sl_merit_side(v - lb, lsum, bad);
          if (up) sl_merit_side(ub - v, lsum, bad);
        }
      }
    }
  } else {
    const double* g = a.p[1] + entry * a.m;
    const double alpha = a.p[4][entry];
    for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
      const int64_t i = (pc - a.x_pieces) * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
      if (i < a.m) {
        const double lb = a.clb[i], ub = a.cub[i];
        double r, st = 0.0;
        const bool eq = lb == ub;
        if (eq) {
          r = g[i] - lb;
        } else {
          const double step = alpha * a.p[3][i];
          st = a.p[2][i] + step;
          r = g[i] - st;
        }
        if (__builtin_isfinite(r)) {
          const double ar = __builtin_fabs(r);
          t1 = t1 + ar;
          tinf = sl_max(tinf, ar);
        } else {
          bad = bad + 1.0;
        }
        if (!eq) {
          if (__builtin_isfinite(lb)) sl_merit_side(st - lb, lsum, bad);
          if (__builtin_isfinite(ub)) sl_merit_side(ub - st, lsum, bad);
        }
      }
    }
  }
  s[0 * PK_BLOCK + t] = t1; s[1 * PK_BLOCK + t] = tinf; s[2 * PK_BLOCK + t] = lsum; s[3 * PK_BLOCK + t] = bad;
}

// thread q < planes behind the trees of piece pc of an entry
PK_LIB_FN void sl_store_partial(const PkSlackArgs& a, int64_t entry, int64_t pc, int q, const double* s) {
  a.partial[(entry * a.planes + q) * a.n_pieces + pc] = s[q * PK_BLOCK];
}

// thread t of the scalar step of an entry: per plane the pieces t, t + 256, ... in ascending order into the identity
PK_LIB_FN void sl_scalar_thread(const PkSlackArgs& a, int64_t entry, int t, double* s) {
  for (int q = 0; q < a.planes; ++q) {
    const int op = sl_op(a.kind, q);
    double acc = sl_identity(op);
    for (int64_t pc = t; pc < a.n_pieces; pc += PK_BLOCK) acc = sl_fold(op, acc, a.partial[(entry * a.planes + q) * a.n_pieces + pc]);
    s[q * PK_BLOCK + t] = acc;
  }
}

// thread 0 of the scalar step behind the trees: plane q ended in s[q * PK_BLOCK]
PK_LIB_FN void sl_scalar_decide(const PkSlackArgs& a, int64_t entry, const double* s) {
  const int rec = sl_record(a.kind);
  for (int q = 0; q < rec; ++q) a.out[entry * rec + q] = q < a.planes ? s[q * PK_BLOCK] : 0.0;
}

#ifdef __HIPCC__
// ---------------------------------------------------------------- kernels (gfx950)
__global__ void __launch_bounds__(PK_BLOCK) pk_sl_reduce_k(PkSlackArgs a) {
  __shared__ double s[4 * PK_BLOCK];
  const int t = (int)threadIdx.x;
  for (int64_t pc = (int64_t)blockIdx.x; pc < a.n_pieces; pc += (int64_t)gridDim.x) {
    sl_reduce_thread(a, pc, t, s);
    __syncthreads();
    lib_tree(sl_tree_step, s, t, (int)PK_SL_REDUCE);
    if (t < 4) sl_store_partial(a, 0, pc, t, s);
    __syncthreads();          // the next piece of this workgroup's stride overwrites the planes
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_sl_recover_k(PkSlackArgs a) {
  __shared__ double s[5 * PK_BLOCK];
  const int t = (int)threadIdx.x;
  for (int64_t pc = (int64_t)blockIdx.x; pc < a.n_pieces; pc += (int64_t)gridDim.x) {
    sl_recover_thread(a, pc, t, s);
    __syncthreads();
    lib_tree(sl_tree_step, s, t, (int)PK_SL_RECOVER);
    if (t < 5) sl_store_partial(a, 0, pc, t, s);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_sl_update_k(PkSlackArgs a) {
  __shared__ double s[3 * PK_BLOCK];
  const int t = (int)threadIdx.x;
  for (int64_t pc = (int64_t)blockIdx.x; pc < a.n_pieces; pc += (int64_t)gridDim.x) {
    sl_update_thread(a, pc, t, s);
    __syncthreads();
    lib_tree(sl_tree_step, s, t, (int)PK_SL_UPDATE);
    if (t < 3) sl_store_partial(a, 0, pc, t, s);
    __syncthreads();
  }
}

// work item = entry * n_pieces + piece
__global__ void __launch_bounds__(PK_BLOCK) pk_sl_merit_k(PkSlackArgs a) {
  __shared__ double s[4 * PK_BLOCK];
  const int t = (int)threadIdx.x;
  const int64_t items = a.batch * a.n_pieces;
  for (int64_t item = (int64_t)blockIdx.x; item < items; item += (int64_t)gridDim.x) {
    const int64_t entry = item / a.n_pieces, pc = item % a.n_pieces;
    sl_merit_thread(a, entry, pc, t, s);
    __syncthreads();
    lib_tree(sl_tree_step, s, t, (int)PK_SL_MERIT);
    if (t < 4) sl_store_partial(a, entry, pc, t, s);
    __syncthreads();
  }
}

// one workgroup per entry (one entry outside a batch)
__global__ void __launch_bounds__(PK_BLOCK) pk_sl_scalar_k(PkSlackArgs a) {
  __shared__ double s[PK_SL_PLANES * PK_BLOCK];
  const int t = (int)threadIdx.x;
  for (int64_t entry = (int64_t)blockIdx.x; entry < a.batch; entry += (int64_t)gridDim.x) {
    sl_scalar_thread(a, entry, t, s);
    __syncthreads();
    lib_tree(sl_tree_step, s, t, (int)a.kind);
    if (t == 0) sl_scalar_decide(a, entry, s);
    __syncthreads();
  }
}
#else
// ---------------------------------------------------------------- host stand-in: the identical walk
static void sl_pieces_host(const PkSlackArgs& a, unsigned grid) {
  double s[PK_SL_PLANES * PK_BLOCK];
  lib_walk_host(grid, a.batch * a.n_pieces, [&](int64_t item) {
    const int64_t entry = item / a.n_pieces, pc = item % a.n_pieces;
    for (int t = 0; t < PK_BLOCK; ++t) {
      if (a.kind == PK_SL_REDUCE) sl_reduce_thread(a, pc, t, s);
      else if (a.kind == PK_SL_RECOVER) sl_recover_thread(a, pc, t, s);
      else if (a.kind == PK_SL_UPDATE) sl_update_thread(a, pc, t, s);
      else sl_merit_thread(a, entry, pc, t, s);
    }
    lib_tree_host(sl_tree_step, s, (int)a.kind);
    for (int q = 0; q < a.planes; ++q) sl_store_partial(a, entry, pc, q, s);
  });
}
static void sl_scalar_host(const PkSlackArgs& a, unsigned grid) {
  double s[PK_SL_PLANES * PK_BLOCK];
  lib_walk_host(grid, a.batch, [&](int64_t entry) {
    for (int t = 0; t < PK_BLOCK; ++t) sl_scalar_thread(a, entry, t, s);
    lib_tree_host(sl_tree_step, s, (int)a.kind);
    sl_scalar_decide(a, entry, s);
  });
}
#endif

void free_slack(pk_ctx* c) {
  release(c->slack.d_partial); release(c->slack.d_scratch);
  c->slack = PkSlack{};
}

namespace {

int64_t sl_pieces_of(int64_t len) { return (len + PK_LIB_PIECE - 1) / PK_LIB_PIECE; }

// the pointers a kind needs, all of them given?
bool sl_pointers(int kind, double* const* p) {
  const int need = kind == PK_SL_REDUCE ? 7 : kind == PK_SL_RECOVER ? 9 : kind == PK_SL_UPDATE ? 6 : 5;
  for (int k = 0; k < need; ++k)
    if (!p[k]) return false;
  return true;
}
bool sl_unit(double v) { return v >= 0.0 && v <= 1.0; }

// the checks every form shares behind its own, the pieced launch of a kind and the scalar launch behind it
int sl_run(pk_ctx* c, PkSlackArgs a, int kind, const char* who, void* stream) {
  if (!sl_pointers(kind, a.p) || !a.out || !a.clb || !a.cub || ((kind == PK_SL_RECOVER || kind == PK_SL_MERIT) && (!a.xlb || !a.xub)))
    return fail(c, 110, "%s: null device pointer", who);
  if (kind == PK_SL_UPDATE) {
    if (!a.p[6] != !a.p[7]) return fail(c, 110, "%s: lam and dlam go together", who);
    if (!sl_unit(a.alpha_p) || !sl_unit(a.alpha_d) || !(a.mu >= 0.0) || !__builtin_isfinite(a.mu) || !(a.kappa >= 1.0) || !__builtin_isfinite(a.kappa))
      return fail(c, 134, "%s: alpha_p = %g, alpha_d = %g (in [0, 1]), mu = %g (finite, not negative), kappa = %g (finite, at least 1)", who,
                  a.alpha_p, a.alpha_d, a.mu, a.kappa);
  }
  if (kind == PK_SL_MERIT) {
    if (a.batch < 1) return fail(c, 134, "%s: a batch of %lld trial points", who, (long long)a.batch);
  } else {
    a.batch = 1;
  }
  a.kind = kind; a.planes = sl_planes(kind);
  const bool two = kind == PK_SL_RECOVER || kind == PK_SL_MERIT;
  a.x_pieces = two ? sl_pieces_of(a.n) : 0;
  a.n_pieces = std::max<int64_t>(1, a.x_pieces + sl_pieces_of(a.m));
  if (const int rc = lib_reserve(c, c->slack.d_partial, c->slack.partial_cap, (size_t)a.planes * (size_t)a.n_pieces * (size_t)a.batch, 136, who,
                                 "partial columns"))
    return rc;
  a.partial = c->slack.d_partial;
  hipStream_t st = pick(c, stream);
  const unsigned grid = lib_grid(a.batch * a.n_pieces);
  if (kind == PK_SL_REDUCE) PK_LIB_LAUNCH(c, pk_sl_reduce_k, sl_pieces_host, grid, st, a);
  else if (kind == PK_SL_RECOVER) PK_LIB_LAUNCH(c, pk_sl_recover_k, sl_pieces_host, grid, st, a);
  else if (kind == PK_SL_UPDATE) PK_LIB_LAUNCH(c, pk_sl_update_k, sl_pieces_host, grid, st, a);
  else PK_LIB_LAUNCH(c, pk_sl_merit_k, sl_pieces_host, grid, st, a);
  PK_LIB_LAUNCH(c, pk_sl_scalar_k, sl_scalar_host, lib_grid(a.batch), st, a);
  return 0;
}

// the public forms' start: a context that is ready, not sharded, with bounds; the bounds and lengths into the arguments
int sl_context(pk_ctx* c, PkSlackArgs& a, const char* who) {
  if (c->shard.flags || c->exchange.world > 1) return fail(c, 119, "%s: not offered for a sharded context", who);
  if (!c->merit.d_bounds) return fail(c, 123, "%s: no bounds (pk_set_bounds)", who);
  const double* b = c->merit.d_bounds;
  const size_t n = (size_t)c->n, m = (size_t)c->m;
  a.n = c->n; a.m = c->m;
  a.clb = b; a.cub = b + m; a.xlb = b + 2 * m; a.xub = b + 2 * m + n;
  return 0;
}
int sl_which(pk_ctx* c, int which, bool with_lam, PkSlackArgs& a, const char* who) {
  if (which != 0 && which != 1) return fail(c, 134, "%s: which = %d (0: the variables, 1: the constraint rows)", who, which);
  if (with_lam && which != 1) return fail(c, 134, "%s: lam goes with which = 1 (the constraint rows) only", who);
  if (which == 0) { a.clb = a.xlb; a.cub = a.xub; a.m = a.n; }
  return 0;
}

// the host forms' scratch: slices of max(n, m) doubles, the record behind them
struct SlackScratch {
  double *a0, *a1, *a2, *a3, *a4, *a5, *a6, *a7, *a8;
};
int sl_scratch(pk_ctx* c, SlackScratch& w, double*& rec, const char* who) {
  const size_t L = (size_t)std::max(std::max(c->n, c->m), 1);
  if (const int rc = lib_reserve(c, c->slack.d_scratch, c->slack.scratch_cap, 9 * L + 8, 136, who, "host-form scratch")) return rc;
  w = lib_slices<SlackScratch>(c->slack.d_scratch, L);
  rec = c->slack.d_scratch + 9 * L;
  return 0;
}
int sl_download(pk_ctx* c, double* dst, const double* src, size_t count) {
  if (count) PK_HIP(c, hipMemcpyAsync(dst, src, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
  return 0;
}
double* sl_in(const double* p) { return const_cast<double*>(p); }      // (an input's slot: the kernels read it only)

}  // namespace

extern "C" {

int pk_slack_reduce_dev(pk_ctx* c, const double* d_g, const double* d_s, const double* d_lam, const double* d_sigma_s,
                        const double* d_rbar_s, double* d_s2, double* d_b2, double* d_out, void* stream) {
  const char* who = "pk_slack_reduce";
  PkSlackArgs a{};
  int rc = ready(c);
  if (rc) return rc;
  if (!d_g || !d_s || !d_lam || !d_sigma_s || !d_rbar_s || !d_s2 || !d_b2 || !d_out) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = sl_context(c, a, who))) return rc;
  a.p[0] = sl_in(d_g); a.p[1] = sl_in(d_s); a.p[2] = sl_in(d_lam); a.p[3] = sl_in(d_sigma_s); a.p[4] = sl_in(d_rbar_s);
  a.p[5] = d_s2; a.p[6] = d_b2; a.out = d_out;
  return sl_run(c, a, PK_SL_REDUCE, who, stream);
}

int pk_slack_recover_dev(pk_ctx* c, const double* d_dlam, const double* d_lam, const double* d_rbar_s, const double* d_s2,
                         const double* d_sigma_s, const double* d_dx, const double* d_w, const double* d_s1, double* d_ds, double* d_out,
                         void* stream) {
  const char* who = "pk_slack_recover";
  PkSlackArgs a{};
  int rc = ready(c);
  if (rc) return rc;
  if (!d_dlam || !d_lam || !d_rbar_s || !d_s2 || !d_sigma_s || !d_dx || !d_w || !d_s1 || !d_ds || !d_out)
    return fail(c, 110, "%s: null device pointer", who);
  if ((rc = sl_context(c, a, who))) return rc;
  a.p[0] = sl_in(d_dlam); a.p[1] = sl_in(d_lam); a.p[2] = sl_in(d_rbar_s); a.p[3] = sl_in(d_s2); a.p[4] = sl_in(d_sigma_s);
  a.p[5] = sl_in(d_dx); a.p[6] = sl_in(d_w); a.p[7] = sl_in(d_s1); a.p[8] = d_ds; a.out = d_out;
  return sl_run(c, a, PK_SL_RECOVER, who, stream);
}

int pk_slack_update_dev(pk_ctx* c, int which, double* d_v, const double* d_dv, double* d_zl, const double* d_dzl, double* d_zu,
                        const double* d_dzu, double* d_lam, const double* d_dlam, double alpha_p, double alpha_d, double mu, double kappa,
                        double* d_out, void* stream) {
  const char* who = "pk_slack_update";
  PkSlackArgs a{};
  int rc = ready(c);
  if (rc) return rc;
  if (!d_v || !d_dv || !d_zl || !d_dzl || !d_zu || !d_dzu || !d_out || (!d_lam != !d_dlam)) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = sl_context(c, a, who)) || (rc = sl_which(c, which, d_lam != nullptr, a, who))) return rc;
  a.p[0] = d_v; a.p[1] = sl_in(d_dv); a.p[2] = d_zl; a.p[3] = sl_in(d_dzl); a.p[4] = d_zu; a.p[5] = sl_in(d_dzu);
  a.p[6] = d_lam; a.p[7] = sl_in(d_dlam);
  a.alpha_p = alpha_p; a.alpha_d = alpha_d; a.mu = mu; a.kappa = kappa; a.out = d_out;
  return sl_run(c, a, PK_SL_UPDATE, who, stream);
}

int pk_slack_merit_dev(pk_ctx* c, int32_t count, const double* d_X, const double* d_G, const double* d_s, const double* d_ds,
                       const double* d_alphas, double* d_out, void* stream) {
  const char* who = "pk_slack_merit";
  PkSlackArgs a{};
  int rc = ready(c);
  if (rc) return rc;
  if (!d_X || !d_G || !d_s || !d_ds || !d_alphas || !d_out) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = sl_context(c, a, who))) return rc;
  a.p[0] = sl_in(d_X); a.p[1] = sl_in(d_G); a.p[2] = sl_in(d_s); a.p[3] = sl_in(d_ds); a.p[4] = sl_in(d_alphas);
  a.batch = count; a.out = d_out;
  return sl_run(c, a, PK_SL_MERIT, who, stream);
}

int pk_slack_raw_dev(pk_ctx* c, int kind, int64_t n, int64_t m, int64_t batch, const double* d_xlb, const double* d_xub, const double* d_clb,
                     const double* d_cub, double* const* d_p, double alpha_p, double alpha_d, double mu, double kappa, double* d_out,
                     void* stream) {
  const char* who = "pk_slack_raw";
  const int rc = ready(c);
  if (rc) return rc;
  if (kind < PK_SL_REDUCE || kind > PK_SL_MERIT || n < 0 || m < 0)
    return fail(c, 134, "%s: kind %d (0 ... 3), lengths %lld and %lld", who, kind, (long long)n, (long long)m);
  if (!d_p) return fail(c, 110, "%s: null pointer table", who);
  PkSlackArgs a{};
  a.xlb = d_xlb; a.xub = d_xub; a.clb = d_clb; a.cub = d_cub; a.n = n; a.m = m; a.batch = batch;
  for (int k = 0; k < PK_SL_SLOTS; ++k) a.p[k] = d_p[k];
  a.alpha_p = alpha_p; a.alpha_d = alpha_d; a.mu = mu; a.kappa = kappa; a.out = d_out;
  return sl_run(c, a, kind, who, stream);
}

int pk_slack_reduce(pk_ctx* c, const double* g, const double* s, const double* lam, const double* sigma_s, const double* rbar_s, double* s2,
                    double* b2, double* out) {
  const char* who = "pk_slack_reduce";
  SlackScratch w;
  double* rec = nullptr;
  PkSlackArgs a{};
  int rc = host_ready(c, g && s && lam && sigma_s && rbar_s && s2 && b2 && out);
  if (rc || (rc = sl_context(c, a, who)) || (rc = sl_scratch(c, w, rec, who))) return rc;
  const size_t m = (size_t)c->m;
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_upload(c, w.a0, g, m)) || (rc = lib_upload(c, w.a1, s, m)) || (rc = lib_upload(c, w.a2, lam, m)) ||
      (rc = lib_upload(c, w.a3, sigma_s, m)) || (rc = lib_upload(c, w.a4, rbar_s, m)))
    return rc;
  if ((rc = pk_slack_reduce_dev(c, w.a0, w.a1, w.a2, w.a3, w.a4, w.a5, w.a6, rec, nullptr))) return rc;
  if ((rc = sl_download(c, s2, w.a5, m)) || (rc = sl_download(c, b2, w.a6, m)) || (rc = sl_download(c, out, rec, 4))) return rc;
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int pk_slack_recover(pk_ctx* c, const double* dlam, const double* lam, const double* rbar_s, const double* s2, const double* sigma_s,
                     const double* dx, const double* w_hdx, const double* s1, double* ds, double* out) {
  const char* who = "pk_slack_recover";
  SlackScratch w;
  double* rec = nullptr;
  PkSlackArgs a{};
  int rc = host_ready(c, dlam && lam && rbar_s && s2 && sigma_s && dx && w_hdx && s1 && ds && out);
  if (rc || (rc = sl_context(c, a, who)) || (rc = sl_scratch(c, w, rec, who))) return rc;
  const size_t n = (size_t)c->n, m = (size_t)c->m;
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_upload(c, w.a0, dlam, m)) || (rc = lib_upload(c, w.a1, lam, m)) || (rc = lib_upload(c, w.a2, rbar_s, m)) ||
      (rc = lib_upload(c, w.a3, s2, m)) || (rc = lib_upload(c, w.a4, sigma_s, m)) || (rc = lib_upload(c, w.a5, dx, n)) ||
      (rc = lib_upload(c, w.a6, w_hdx, n)) || (rc = lib_upload(c, w.a7, s1, n)))
    return rc;
  if ((rc = pk_slack_recover_dev(c, w.a0, w.a1, w.a2, w.a3, w.a4, w.a5, w.a6, w.a7, w.a8, rec, nullptr))) return rc;
  if ((rc = sl_download(c, ds, w.a8, m)) || (rc = sl_download(c, out, rec, 5))) return rc;
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int pk_slack_update(pk_ctx* c, int which, double* v, const double* dv, double* zl, const double* dzl, double* zu, const double* dzu,
                    double* lam, const double* dlam, double alpha_p, double alpha_d, double mu, double kappa, double* out) {
  const char* who = "pk_slack_update";
  SlackScratch w;
  double* rec = nullptr;
  PkSlackArgs a{};
  int rc = host_ready(c, v && dv && zl && dzl && zu && dzu && out && (!lam == !dlam));
  if (rc || (rc = sl_context(c, a, who)) || (rc = sl_which(c, which, lam != nullptr, a, who))) return rc;
  if (!sl_unit(alpha_p) || !sl_unit(alpha_d) || !(mu >= 0.0) || !__builtin_isfinite(mu) || !(kappa >= 1.0) || !__builtin_isfinite(kappa))
    return fail(c, 134, "%s: alpha_p = %g, alpha_d = %g (in [0, 1]), mu = %g (finite, not negative), kappa = %g (finite, at least 1)", who,
                alpha_p, alpha_d, mu, kappa);
  if ((rc = sl_scratch(c, w, rec, who))) return rc;
  const size_t L = (size_t)a.m;
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_upload(c, w.a0, v, L)) || (rc = lib_upload(c, w.a1, dv, L)) || (rc = lib_upload(c, w.a2, zl, L)) ||
      (rc = lib_upload(c, w.a3, dzl, L)) || (rc = lib_upload(c, w.a4, zu, L)) || (rc = lib_upload(c, w.a5, dzu, L)) ||
      (rc = lib_upload(c, w.a6, lam, L)) || (rc = lib_upload(c, w.a7, dlam, L)))
    return rc;
  if ((rc = pk_slack_update_dev(c, which, w.a0, w.a1, w.a2, w.a3, w.a4, w.a5, lam ? w.a6 : nullptr, lam ? w.a7 : nullptr, alpha_p, alpha_d, mu,
                                kappa, rec, nullptr)))
    return rc;
  if ((rc = sl_download(c, v, w.a0, L)) || (rc = sl_download(c, zl, w.a2, L)) || (rc = sl_download(c, zu, w.a4, L)) ||
      (rc = sl_download(c, lam, w.a6, lam ? L : 0)) || (rc = sl_download(c, out, rec, 4)))
    return rc;
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
