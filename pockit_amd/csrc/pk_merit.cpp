// pk_merit.cpp -- a batch of trial points scored where the batch launch left its results: per entry b a row of 8 doubles
//
//   0 f            f[b], copied                                   4 bound1      sum_i viol(X[b,i], v_lb[i], v_ub[i])
//   1 theta1       sum_i viol(g[b,i], c_lb[i], c_ub[i])           5 bound_inf   max_i of the same
//   2 theta_inf    max_i of the same                              6 slope       sum_i grad[b,i] * d[i]   (0.0 without d)
//   3 theta2_sq    sum_i viol^2                                   7 bad         non-finite values among f[b], g[b,:], grad[b,:]
//
// viol(v, lo, hi) = max(lo - v, v - hi, 0), taken by comparisons: a NaN difference (inf - inf) loses like -inf does.  A
// non-finite g or grad entry is counted in column 7 and adds nothing to any other column, so those stay finite and the caller
// rejects the point on bad > 0.  (X is not screened: a NaN in X adds nothing, an infinite one an infinite bound violation.)
// Model-independent, so the three kernels live in the library like pk_ops.cpp's, not in the generated code object.
//
//   pk_trial      X[b * ldx + i] = x[i] + alpha[b] * d[i]: the product rounded, then the sum -- no fused multiply-add, the
//                 bits of NumPy's x + a * d.  alpha: B <= PK_MAX_BATCH host values that travel in the kernel arguments
//   pk_merit      one workgroup per (entry, piece of 2048 = 256 threads x 8 indices): partial[(b * n_pieces + p) * 8 + q]
//   pk_merit_fin  one workgroup per entry: the pieces' rows -> out[b * 8 + q]
//
// The association is fixed: it depends neither on the grid nor on the run, and there are no atomics.  Index i of entry b
// belongs to piece p = i / 2048; thread t of the piece adds the terms of p * 2048 + t + 256 j for j = 0 ... 7 in ascending j
// to 0.0 (coalesced reads; an index beyond a vector's length adds nothing), every square and every product rounded before it
// is added.  The 256 thread values meet in LDS and are reduced by the tree of widths 128, 64 ... 1 (slot t += slot t + w)
// of pk_libkernel.h.  pk_merit_fin: thread t adds the rows of the pieces t, t + 256, ... in ascending order to 0.0, the
// same tree follows, thread q < 8 stores column q.  Columns 2 and 5 walk the same way with max in place of +; column 7 counts.
// n_pieces = max(1, ceil(max(len g, len X) / 2048)): g, X and grad share the pieces, the shorter vector ends earlier.
#include "pk_runtime.h"

// Nothing in this unit may contract a * b + c into a fused multiply-add (hipcc's default is to contract; __dmul_rn and
// __dadd_rn are plain operators in its headers and contract with their neighbours once inlined).
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#include "pk_libkernel.h"      // (behind the pragma: what its templates are instantiated with is this unit's arithmetic)

enum { PK_MERIT_PER_THREAD = 8, PK_MERIT_PIECE = PK_BLOCK * PK_MERIT_PER_THREAD, PK_MERIT_COLS = 8, PK_MERIT_PLANES = 7 };

struct PkMeritArgs {
  const double *g, *clb, *cub;      // n_g values per entry, rows ldg apart; the bounds are shared by the entries
  const double *X, *vlb, *vub;      // n_x values per entry, rows ldx apart
  const double *grad, *d;           // n_x values per entry, rows ldgrad apart; d (n_x values, shared) may be NULL
  const double* f;                  // one value per entry
  double *partial, *out;
  int64_t ldg, ldx, ldgrad, n_g, n_x, n_pieces;
  int32_t B;
};

struct PkTrialArgs {
  const double *x, *d;
  double* X;
  int64_t ldx;
  int32_t n, B;
  double alpha[PK_MAX_BATCH];
};

PK_LIB_FN double merit_viol(double v, double lo, double hi) {
  const double a = lo - v, b = v - hi;
  double r = 0.0;
  if (a > r) r = a;
  if (b > r) r = b;
  return r;
}

PK_LIB_FN bool merit_is_max(int q) { return q == 2 || q == 5; }
PK_LIB_FN double merit_combine(int q, double a, double b) { return merit_is_max(q) ? (b > a ? b : a) : a + b; }

// thread t of piece p of entry b: its seven values (columns 1 ... 7) into the planes, plane q - 1 for column q
PK_LIB_FN void merit_thread(const PkMeritArgs& a, int32_t b, int64_t p, int t, double* s) {
  const double* g = a.g + (int64_t)b * a.ldg;
  const double* X = a.X + (int64_t)b * a.ldx;
  const double* grad = a.grad + (int64_t)b * a.ldgrad;
  double th1 = 0.0, thinf = 0.0, th2 = 0.0, b1 = 0.0, binf = 0.0, slope = 0.0, bad = 0.0;
  for (int j = 0; j < PK_MERIT_PER_THREAD; ++j) {
    const int64_t i = p * PK_MERIT_PIECE + t + (int64_t)PK_BLOCK * j;
    if (i < a.n_g) {
      const double v = g[i];
      if (__builtin_isfinite(v)) {
        const double w = merit_viol(v, a.clb[i], a.cub[i]);
        const double sq = w * w;
        th1 = th1 + w;
        if (w > thinf) thinf = w;
        th2 = th2 + sq;
      } else {
        bad = bad + 1.0;
      }
    }
    if (i < a.n_x) {
      const double w = merit_viol(X[i], a.vlb[i], a.vub[i]);
      b1 = b1 + w;
      if (w > binf) binf = w;
      const double gr = grad[i];
      if (!__builtin_isfinite(gr)) {
        bad = bad + 1.0;
      } else if (a.d) {
        const double pr = gr * a.d[i];
        slope = slope + pr;
      }
    }
  }
  s[0 * PK_BLOCK + t] = th1; s[1 * PK_BLOCK + t] = thinf; s[2 * PK_BLOCK + t] = th2; s[3 * PK_BLOCK + t] = b1;
  s[4 * PK_BLOCK + t] = binf; s[5 * PK_BLOCK + t] = slope; s[6 * PK_BLOCK + t] = bad;
}

// thread t of entry b in pk_merit_fin: per column the rows of the pieces t, t + 256, ... in ascending order
PK_LIB_FN void merit_fin_thread(const PkMeritArgs& a, int32_t b, int t, double* s) {
  const double* rows = a.partial + (int64_t)b * a.n_pieces * PK_MERIT_COLS;
  for (int q = 1; q < PK_MERIT_COLS; ++q) {
    double acc = 0.0;
    for (int64_t p = t; p < a.n_pieces; p += PK_BLOCK) acc = merit_combine(q, acc, rows[p * PK_MERIT_COLS + q]);
    s[(q - 1) * PK_BLOCK + t] = acc;
  }
}

// one step of the seven trees, which share the barrier of the level: widths 128, 64 ... 1.  The lanes of a wave work on
// consecutive doubles of one plane at a time: no bank is asked twice by a half-wave.
PK_LIB_FN void merit_tree_step(double* s, int w, int t) {
  if (t >= w) return;
  for (int q = 1; q < PK_MERIT_COLS; ++q) {
    double* p = s + (q - 1) * PK_BLOCK;
    p[t] = merit_combine(q, p[t], p[t + w]);
  }
}

// thread q < 8 behind the trees
PK_LIB_FN void merit_store_partial(const PkMeritArgs& a, int64_t item, int q, const double* s) {
  a.partial[item * PK_MERIT_COLS + q] = q == 0 ? 0.0 : s[(q - 1) * PK_BLOCK];
}
PK_LIB_FN void merit_store_out(const PkMeritArgs& a, int32_t b, int q, const double* s) {
  const double f = a.f[b];
  double v = q == 0 ? f : s[(q - 1) * PK_BLOCK];
  if (q == 7 && !__builtin_isfinite(f)) v = v + 1.0;
  a.out[(int64_t)b * PK_MERIT_COLS + q] = v;
}

static int64_t trial_items(int64_t n) { return (n + PK_BLOCK - 1) / PK_BLOCK; }

// element i of every trial point: x[i] and d[i] are read once
PK_LIB_FN void trial_element(const PkTrialArgs& a, int32_t i) {
  const double xi = a.x[i], di = a.d[i];
  for (int32_t b = 0; b < a.B; ++b) {
    const double step = a.alpha[b] * di;
    a.X[(int64_t)b * a.ldx + i] = xi + step;
  }
}

#ifdef __HIPCC__
// ---------------------------------------------------------------- kernels (gfx950)
__global__ void __launch_bounds__(PK_BLOCK) pk_merit(PkMeritArgs a) {
  __shared__ double s[PK_MERIT_PLANES * PK_BLOCK];
  const int t = (int)threadIdx.x;
  const int64_t items = (int64_t)a.B * a.n_pieces;
  for (int64_t item = (int64_t)blockIdx.x; item < items; item += (int64_t)gridDim.x) {
    const int32_t b = (int32_t)(item / a.n_pieces);
    merit_thread(a, b, item - (int64_t)b * a.n_pieces, t, s);
    __syncthreads();
    lib_tree(merit_tree_step, s, t);
    if (t < PK_MERIT_COLS) merit_store_partial(a, item, t, s);
    __syncthreads();          // the next item of this workgroup's stride overwrites the planes
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_merit_fin(PkMeritArgs a) {
  __shared__ double s[PK_MERIT_PLANES * PK_BLOCK];
  const int t = (int)threadIdx.x;
  for (int32_t b = (int32_t)blockIdx.x; b < a.B; b += (int32_t)gridDim.x) {
    merit_fin_thread(a, b, t, s);
    __syncthreads();
    lib_tree(merit_tree_step, s, t);
    if (t < PK_MERIT_COLS) merit_store_out(a, b, t, s);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_trial(PkTrialArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * PK_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * PK_BLOCK)
    trial_element(a, (int32_t)i);
}
#else
// ---------------------------------------------------------------- host stand-in: the identical walk
static void merit_host(const PkMeritArgs& a, unsigned grid) {
  double s[PK_MERIT_PLANES * PK_BLOCK];
  lib_walk_host(grid, (int64_t)a.B * a.n_pieces, [&](int64_t item) {
    const int32_t b = (int32_t)(item / a.n_pieces);
    for (int t = 0; t < PK_BLOCK; ++t) merit_thread(a, b, item - (int64_t)b * a.n_pieces, t, s);
    lib_tree_host(merit_tree_step, s);
    for (int q = 0; q < PK_MERIT_COLS; ++q) merit_store_partial(a, item, q, s);
  });
}

static void merit_fin_host(const PkMeritArgs& a, unsigned grid) {
  double s[PK_MERIT_PLANES * PK_BLOCK];
  lib_walk_host(grid, a.B, [&](int64_t b) {
    for (int t = 0; t < PK_BLOCK; ++t) merit_fin_thread(a, (int32_t)b, t, s);
    lib_tree_host(merit_tree_step, s);
    for (int q = 0; q < PK_MERIT_COLS; ++q) merit_store_out(a, (int32_t)b, q, s);
  });
}

static void trial_host(const PkTrialArgs& a, unsigned grid) {
  lib_walk_host(grid, trial_items(a.n), [&](int64_t item) {
    for (int64_t i = item * PK_BLOCK; i < std::min<int64_t>(a.n, (item + 1) * PK_BLOCK); ++i) trial_element(a, (int32_t)i);
  });
}
#endif

// The work items of the grid rule (lib_grid, pk_libkernel.h): a piece of an entry (pk_merit), an entry (pk_merit_fin), 256
// elements of x (pk_trial).

static int64_t merit_pieces(int64_t n_g, int64_t n_x) {
  return std::max<int64_t>(1, (std::max(n_g, n_x) + PK_MERIT_PIECE - 1) / PK_MERIT_PIECE);
}

void free_merit(pk_ctx* c) {
  release(c->merit.d_bounds); release(c->merit.d_partial); release(c->merit.d_scratch);
  c->merit = PkMerit{};
}

namespace {

// entries of one chunk of the host forms: what bounds their scratch
int64_t merit_chunk(const pk_ctx* c) {
  const int64_t per_entry = 8 * (c->nnz_J + (int64_t)c->n + c->m + 1);
  return std::min<int64_t>(PK_MAX_BATCH, std::max<int64_t>(1, (256ll << 20) / per_entry));
}

int merit_refused_for(pk_ctx* c, const char* who) {
  if (c->cycle_layout) return fail(c, 88, "%s: the compact layouts (pk_set_cycle_layout) are not offered for a batch", who);
  if (c->exchange.in_launch && c->exchange.world > 1)
    return fail(c, 88, "%s: a sharded context with the in-launch exchange is not offered for a batch", who);
  return 0;
}

struct MeritScratch {
  double *x, *d, *X, *f, *grad, *g, *J, *out;
};

// the host forms: scan (x, d, alpha given, X NULL) and batch (X given; d may be NULL)
int merit_host_form(pk_ctx* c, int64_t B, const double* x, const double* d, const double* alpha, const double* X, int64_t ldx,
                    double* out, const char* who) {
  int rc;
  if (B < 1) return fail(c, 124, "%s: B = %lld, a batch has at least one entry", who, (long long)B);
  if (X && ldx < c->n) return fail(c, 125, "%s: leading dimension %lld of X is smaller than n = %d", who, (long long)ldx, c->n);
  if (!c->merit.d_bounds) return fail(c, 123, "%s: no bounds (pk_set_bounds)", who);
  if ((rc = merit_refused_for(c, who))) return rc;
  const size_t n = (size_t)c->n, m = (size_t)c->m, nj = (size_t)c->nnz_J;
  const size_t cap = (size_t)std::min<int64_t>(B, merit_chunk(c));
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_reserve(c, c->merit.d_scratch, c->merit.scratch_cap, 2 * n + cap * (2 * n + m + nj + 1 + PK_MERIT_COLS), 127, who,
                        "scratch")))
    return rc;
  if ((rc = lib_reserve(c, c->merit.d_partial, c->merit.partial_cap, cap * (size_t)merit_pieces(c->m, c->n) * PK_MERIT_COLS, 127, who,
                        "partial rows")))
    return rc;
  MeritScratch s;
  s.x = c->merit.d_scratch; s.d = s.x + n; s.X = s.d + n; s.f = s.X + cap * n; s.grad = s.f + cap; s.g = s.grad + cap * n;
  s.J = s.g + cap * m; s.out = s.J + cap * nj;
  c->shim.x_valid = false;      // the context's workspaces now hold other evaluations (the loop of single cycles uses them)
  if (x) PK_HIP(c, hipMemcpyAsync(s.x, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  if (d) PK_HIP(c, hipMemcpyAsync(s.d, d, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  for (int64_t lo = 0; lo < B; lo += (int64_t)cap) {
    const int cnt = (int)std::min<int64_t>((int64_t)cap, B - lo);
    if (X) {
      if (ldx == c->n) {
        PK_HIP(c, hipMemcpyAsync(s.X, X + (size_t)lo * n, sizeof(double) * n * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
      } else {
        for (int e = 0; e < cnt; ++e)
          PK_HIP(c, hipMemcpyAsync(s.X + (size_t)e * n, X + (size_t)(lo + e) * (size_t)ldx, sizeof(double) * n, hipMemcpyHostToDevice,
                                   c->stream));
      }
    } else if ((rc = pk_trial_points_dev(c, cnt, s.x, s.d, alpha + lo, s.X, c->n, nullptr))) {
      return rc;
    }
    if ((rc = pk_eval_cycle_batch_dev(c, cnt, s.X, c->n, nullptr, 0, nullptr, s.f, s.grad, s.g, s.J, nullptr, nullptr))) return rc;
    if ((rc = pk_merit_batch_dev(c, cnt, s.f, s.g, c->m, s.grad, c->n, s.X, c->n, d ? s.d : nullptr, s.out, nullptr))) return rc;
    PK_HIP(c, hipMemcpyAsync(out + (size_t)lo * PK_MERIT_COLS, s.out, sizeof(double) * PK_MERIT_COLS * (size_t)cnt,
                             hipMemcpyDeviceToHost, c->stream));
  }
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return handoff_check(c);
}

}  // namespace

extern "C" {

int pk_set_bounds(pk_ctx* c, const double* c_lb, const double* c_ub, const double* v_lb, const double* v_ub) {
  int rc = ready(c);
  if (rc) return rc;
  if (!c_lb || !c_ub || !v_lb || !v_ub) return fail(c, 126, "pk_set_bounds: null pointer");
  const size_t n = (size_t)c->n, m = (size_t)c->m;
  const struct { const double *lo, *hi; size_t count; const char* name; } sets[2] = {{c_lb, c_ub, m, "c"}, {v_lb, v_ub, n, "v"}};
  for (const auto& s : sets)
    for (size_t i = 0; i < s.count; ++i)
      if (!(s.lo[i] <= s.hi[i]))      // (a NaN on either side fails the comparison too)
        return fail(c, 126, "pk_set_bounds: %s_lb[%zu] = %g, %s_ub[%zu] = %g (NaN, or lower above upper)", s.name, i, s.lo[i], s.name, i,
                    s.hi[i]);
  std::vector<double> all;
  all.reserve(2 * (n + m));
  all.insert(all.end(), c_lb, c_lb + m); all.insert(all.end(), c_ub, c_ub + m);
  all.insert(all.end(), v_lb, v_lb + n); all.insert(all.end(), v_ub, v_ub + n);
  PK_HIP(c, hipSetDevice(c->device));
  double* fresh = nullptr;
  if (hipMalloc((void**)&fresh, sizeof(double) * std::max<size_t>(all.size(), 1)) != hipSuccess || !fresh)
    return fail(c, 127, "pk_set_bounds: no device memory for %zu doubles", all.size());
  hipError_t e = hipDeviceSynchronize();      // (a reduction enqueued earlier may still read the old bounds)
  if (e == hipSuccess && !all.empty()) e = hipMemcpy(fresh, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    release(fresh);
    return fail(c, 100 + (int)e, "pk_set_bounds: the upload failed: %s", hipGetErrorString(e));
  }
  release(c->merit.d_bounds);
  c->merit.d_bounds = fresh;
  return 0;
}

int pk_trial_points_dev(pk_ctx* c, int B, const double* d_x, const double* d_d, const double* alpha, double* d_X, int64_t ldx,
                        void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (B < 1 || B > PK_MAX_BATCH) return fail(c, 124, "pk_trial_points: %d entries (1 ... %d)", B, PK_MAX_BATCH);
  if (!d_x || !d_d || !alpha || !d_X) return fail(c, 128, "pk_trial_points: null pointer");
  if (ldx < c->n) return fail(c, 125, "pk_trial_points: leading dimension %lld is smaller than n = %d", (long long)ldx, c->n);
  PkTrialArgs a{};
  a.x = d_x; a.d = d_d; a.X = d_X; a.ldx = ldx; a.n = c->n; a.B = B;
  std::copy(alpha, alpha + B, a.alpha);
  hipStream_t st = pick(c, stream);
  if (c->n > 0) PK_LIB_LAUNCH(c, pk_trial, trial_host, lib_grid(trial_items(c->n)), st, a);
  return 0;
}

int pk_merit_reduce_dev(pk_ctx* c, int B, int64_t n_g, const double* d_g, int64_t ldg, const double* d_clb, const double* d_cub,
                        int64_t n_x, const double* d_X, int64_t ldx, const double* d_vlb, const double* d_vub, const double* d_grad,
                        int64_t ldgrad, const double* d_d, const double* d_f, double* d_out, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (B < 1 || B > PK_MAX_BATCH) return fail(c, 124, "pk_merit_reduce: %d entries (1 ... %d)", B, PK_MAX_BATCH);
  if (n_g < 0 || n_x < 0 || ldg < n_g || ldx < n_x || ldgrad < n_x)
    return fail(c, 125, "pk_merit_reduce: leading dimensions %lld / %lld / %lld of g / X / grad (lengths %lld / %lld / %lld)",
                (long long)ldg, (long long)ldx, (long long)ldgrad, (long long)n_g, (long long)n_x, (long long)n_x);
  if (!d_f || !d_out || (n_g > 0 && (!d_g || !d_clb || !d_cub)) || (n_x > 0 && (!d_X || !d_vlb || !d_vub || !d_grad)))
    return fail(c, 128, "pk_merit_reduce: null pointer (only d may be NULL)");
  PkMeritArgs a{};
  a.g = d_g; a.clb = d_clb; a.cub = d_cub; a.X = d_X; a.vlb = d_vlb; a.vub = d_vub; a.grad = d_grad; a.d = d_d; a.f = d_f;
  a.out = d_out; a.ldg = ldg; a.ldx = ldx; a.ldgrad = ldgrad; a.n_g = n_g; a.n_x = n_x; a.n_pieces = merit_pieces(n_g, n_x); a.B = B;
  if ((rc = lib_reserve(c, c->merit.d_partial, c->merit.partial_cap, (size_t)B * (size_t)a.n_pieces * PK_MERIT_COLS, 127,
                        "pk_merit_reduce", "partial rows")))
    return rc;
  a.partial = c->merit.d_partial;
  hipStream_t st = pick(c, stream);
  PK_LIB_LAUNCH(c, pk_merit, merit_host, lib_grid((int64_t)B * a.n_pieces), st, a);
  PK_LIB_LAUNCH(c, pk_merit_fin, merit_fin_host, lib_grid(B), st, a);
  return 0;
}

int pk_merit_batch_dev(pk_ctx* c, int B, const double* d_f, const double* d_g, int64_t ldg, const double* d_grad, int64_t ldgrad,
                       const double* d_X, int64_t ldx, const double* d_d, double* d_out, void* stream) {
  const int rc = ready(c);
  if (rc) return rc;
  if (B < 1 || B > PK_MAX_BATCH) return fail(c, 124, "pk_merit_batch: %d entries (1 ... %d)", B, PK_MAX_BATCH);
  if (!c->merit.d_bounds) return fail(c, 123, "pk_merit_batch: no bounds (pk_set_bounds)");
  const double* b = c->merit.d_bounds;
  const size_t n = (size_t)c->n, m = (size_t)c->m;
  return pk_merit_reduce_dev(c, B, c->m, d_g, ldg, b, b + m, c->n, d_X, ldx, b + 2 * m, b + 2 * m + n, d_grad, ldgrad, d_d, d_f, d_out,
                             stream);
}

int pk_merit_scan(pk_ctx* c, int64_t B, const double* x, const double* d, const double* alpha, double* out) {
  if (const int rc = host_ready(c, x && d && alpha && out)) return rc;
  return merit_host_form(c, B, x, d, alpha, nullptr, 0, out, "pk_merit_scan");
}

int pk_merit_batch(pk_ctx* c, int64_t B, const double* X, int64_t ldx, const double* d, double* out) {
  if (const int rc = host_ready(c, X && out)) return rc;
  return merit_host_form(c, B, nullptr, d, nullptr, X, ldx, out, "pk_merit_batch");
}

}  // extern "C"
