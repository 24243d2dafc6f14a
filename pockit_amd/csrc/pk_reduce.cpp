// pk_reduce.cpp -- what a matrix-free solver needs about the ENTRIES of J, J^T and the symmetric H, computed where their values
// lie: row norms (scaling, equilibration), the diagonals of J D J^T and J^T D J (preconditioners of the normal equations and of
// the condensed KKT matrix), the diagonal of H.  None is a product with a vector; all of them walk an operator's rows.
//
// A reduction over the rows of operator op (pk_set_csr_operator: 0 J, 1 J^T, 2 H symmetric), a_e = vals[src ? src[e] : e],
// c_e = indices[e], an optional weight w (n_cols values; NULL: the weight is left out, not multiplied by 1.0), an optional add
// (n_rows values, may alias y):
//
//   mode 0  abs_sum   t_e = fabs(a_e) * w[c_e]                                         y[row] = sum_e t_e (+ add[row])
//   mode 1  sq_sum    t_e = (a_e * a_e) * w[c_e]: the square is rounded first, then    y[row] = sum_e t_e (+ add[row])
//                     the product with the weight
//   mode 2  abs_max   t_e = fabs(a_e) * w[c_e]                                         y[row] = max(0, max_e t_e, add[row])
//
// The kernels walk the operator's own row blocks, long rows and partial slots (pk_ops.cpp) under the grid rule lib_grid, and the
// two sums have exactly the association of pk_op_rows / pk_op_long: the terms go to the padded LDS slots (op_slot); a stream row
// is added sequentially in ascending entry order; a piece block runs the fixed tree of widths 128 ... 1; thread t of a long row
// adds partial[first + t], partial[first + t + 256], ... in ascending order, the same tree follows, then + add.  No atomics,
// no dependence on the grid, the same bits from run to run.  The partial slots are the products': the stream orders the two.
//
// Mode 2 walks the same way but takes maxima by comparison (m = 0.0; if (t > m) m = t;), the term itself included before it
// reaches its slot: a NaN term loses, the zero padding is the identity, the result is never negative and never -0.0, and a
// negative weight gives what the arithmetic gives.  NaN is not screened for.
//
// The diagonal of H: y[i] = pos[i] >= 0 ? vals[pos[i]] : 0.0 (+ add[i]), one thread per row, pos (pk_set_operator_diagonal)
// pointing into the Hessian map's CSR values.
#include "pk_runtime.h"

// Nothing in this unit may contract a * b + c into a fused multiply-add: every term is rounded before it is added.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#include "pk_oprows.h"      // (behind the pragma: what its templates are instantiated with is this unit's arithmetic)

enum { PK_RED_ABS_SUM = 0, PK_RED_SQ_SUM = 1, PK_RED_ABS_MAX = 2 };

struct PkRedArgs {
  const PkOpBlock* blocks;
  const PkOpLong* longs;
  const int32_t *indptr, *indices, *src;
  const double *vals, *w, *add;      // w and add may be NULL; add may alias y
  double *y, *partial;
  int32_t n_blocks, n_longs, mode;
};

// a (+) b: the sum, or for abs_max the larger by comparison -- a NaN b loses, and so does -0.0 against 0.0
PK_LIB_FN double red_combine(bool is_max, double a, double b) { return is_max ? (b > a ? b : a) : a + b; }

// thread t of a block: its term (0 beyond the block's count; abs_max: never below 0, never NaN)
PK_LIB_FN double red_term(const PkRedArgs& a, const PkOpBlock& b, int t) {
  if (t >= b.count) return 0.0;
  const int32_t e = b.e0 + t;
  const double v = a.vals[a.src ? a.src[e] : e];
  double x = a.mode == PK_RED_SQ_SUM ? v * v : __builtin_fabs(v);
  if (a.w) x = x * a.w[a.indices[e]];
  return a.mode == PK_RED_ABS_MAX ? red_combine(true, 0.0, x) : x;
}

// what is stored for a row: (+) add where there is one
PK_LIB_FN void red_store(const PkRedArgs& a, int32_t row, double acc) {
  a.y[row] = a.add ? red_combine(a.mode == PK_RED_ABS_MAX, acc, a.add[row]) : acc;
}

// thread r < n_rows of a stream block: the terms of its row in ascending entry order
PK_LIB_FN void red_row(const PkRedArgs& a, const PkOpBlock& b, int r, const double* s) {
  const int32_t row = b.row0 + r;
  const int lo = a.indptr[row] - b.e0, hi = a.indptr[row + 1] - b.e0;
  const bool is_max = a.mode == PK_RED_ABS_MAX;
  double acc = 0.0;
  for (int k = lo; k < hi; ++k) acc = red_combine(is_max, acc, s[op_slot(k)]);
  red_store(a, row, acc);
}

// thread t of a long row: its partial results first + t, first + t + 256, ... in ascending order
PK_LIB_FN double red_long_strided(const PkRedArgs& a, const PkOpLong& l, int t) {
  const bool is_max = a.mode == PK_RED_ABS_MAX;
  double acc = 0.0;
  for (int32_t k = t; k < l.pieces; k += PK_BLOCK) acc = red_combine(is_max, acc, a.partial[l.first + k]);
  return acc;
}

// one step of the fixed tree over the 256 slots (lib_tree: widths 128, 64 ... 1; the result ends in s[0])
PK_LIB_FN void red_tree_step(double* s, int w, int t, bool is_max) {
  if (t < w) s[op_slot(t)] = red_combine(is_max, s[op_slot(t)], s[op_slot(t + w)]);
}

struct PkDiagArgs {
  const int32_t* pos;
  const double *vals, *add;      // add may be NULL, and may alias y
  double* y;
  int32_t n;
};

static int64_t diag_items(int64_t n) { return (n + PK_BLOCK - 1) / PK_BLOCK; }

PK_LIB_FN void diag_element(const PkDiagArgs& a, int32_t i) {
  const int32_t p = a.pos[i];
  const double d = p >= 0 ? a.vals[p] : 0.0;
  a.y[i] = a.add ? d + a.add[i] : d;
}

#ifdef __HIPCC__
// ---------------------------------------------------------------- kernels (gfx950)
__global__ void __launch_bounds__(PK_BLOCK) pk_red_rows(PkRedArgs a) {
  __shared__ double s[PK_OP_LDS];
  const int t = (int)threadIdx.x;
  for (int32_t i = (int32_t)blockIdx.x; i < a.n_blocks; i += (int32_t)gridDim.x) {
    const PkOpBlock b = a.blocks[i];
    s[op_slot(t)] = red_term(a, b, t);
    __syncthreads();
    if (b.n_rows >= 0) {      // (uniform over the workgroup)
      if (t < b.n_rows) red_row(a, b, t, s);
    } else {
      lib_tree(red_tree_step, s, t, a.mode == PK_RED_ABS_MAX);
      if (t == 0) a.partial[b.row0] = s[0];
    }
    __syncthreads();          // the next block of this workgroup's stride overwrites the slots
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_red_long(PkRedArgs a) {
  __shared__ double s[PK_OP_LDS];
  const int t = (int)threadIdx.x;
  for (int32_t i = (int32_t)blockIdx.x; i < a.n_longs; i += (int32_t)gridDim.x) {
    const PkOpLong l = a.longs[i];
    s[op_slot(t)] = red_long_strided(a, l, t);
    __syncthreads();
    lib_tree(red_tree_step, s, t, a.mode == PK_RED_ABS_MAX);
    if (t == 0) red_store(a, l.row, s[0]);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_diag(PkDiagArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * PK_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * PK_BLOCK)
    diag_element(a, (int32_t)i);
}
#else
// ---------------------------------------------------------------- host stand-in: the identical walk over the same tables
static void red_rows_host(const PkRedArgs& a, unsigned grid) {
  double s[PK_OP_LDS];
  lib_walk_host(grid, a.n_blocks, [&](int64_t i) {
    const PkOpBlock b = a.blocks[i];
    for (int t = 0; t < PK_BLOCK; ++t) s[op_slot(t)] = red_term(a, b, t);
    if (b.n_rows >= 0) {
      for (int t = 0; t < b.n_rows; ++t) red_row(a, b, t, s);
    } else {
      lib_tree_host(red_tree_step, s, a.mode == PK_RED_ABS_MAX);
      a.partial[b.row0] = s[0];
    }
  });
}

static void red_long_host(const PkRedArgs& a, unsigned grid) {
  double s[PK_OP_LDS];
  lib_walk_host(grid, a.n_longs, [&](int64_t i) {
    const PkOpLong l = a.longs[i];
    for (int t = 0; t < PK_BLOCK; ++t) s[op_slot(t)] = red_long_strided(a, l, t);
    lib_tree_host(red_tree_step, s, a.mode == PK_RED_ABS_MAX);
    red_store(a, l.row, s[0]);
  });
}

static void diag_host(const PkDiagArgs& a, unsigned grid) {
  lib_walk_host(grid, diag_items(a.n), [&](int64_t item) {
    for (int64_t i = item * PK_BLOCK; i < std::min<int64_t>(a.n, (item + 1) * PK_BLOCK); ++i) diag_element(a, (int32_t)i);
  });
}
#endif

namespace {

// The entry checks of the two diagonal forms, in the order they fire.
int diag_ready(pk_ctx* c, int op, bool pointers, const char* who) {
  if (op < 0 || op > 2) return fail(c, 110, "%s: op must be 0 (J), 1 (J^T) or 2 (H symmetric)", who);
  if (op != 2) return fail(c, 130, "%s: operator %d is not square, only H (op 2) has a diagonal", who, op);
  if (!c->ops.d_diag_pos) return fail(c, 132, "%s: call pk_set_operator_diagonal(2) first", who);
  if (!pointers) return fail(c, 110, "%s: null device pointer", who);
  return 0;
}

int bad_mode(pk_ctx* c, int mode, const char* who) {
  return mode < 0 || mode > 2 ? fail(c, 129, "%s: mode must be 0 (abs_sum), 1 (sq_sum) or 2 (abs_max)", who) : 0;
}

// the scratch vectors of the host forms (pk_set_csr_operator allocates the same two with an operator)
int host_scratch(pk_ctx* c) {
  if (c->ops.d_v) return 0;
  const size_t len = (size_t)std::max(c->n, c->m);
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipMalloc((void**)&c->ops.d_v, sizeof(double) * len));
  PK_HIP(c, hipMalloc((void**)&c->ops.d_y, sizeof(double) * len));
  c->ops.scratch_k = 1;
  return 0;
}

}  // namespace

extern "C" {

int pk_operator_reduce_dev(pk_ctx* c, int op, int mode, const double* d_vals, const double* d_w, const double* d_add, double* d_y,
                           void* stream) {
  int rc = ready(c);
  if (rc || (rc = op_ready(c, op, d_vals && d_y, "pk_operator_reduce")) || (rc = bad_mode(c, mode, "pk_operator_reduce"))) return rc;
  const PkOperator& o = c->ops.op[op];
  PkRedArgs a{};
  a.blocks = o.d_blocks; a.longs = o.d_longs; a.indptr = o.d_indptr; a.indices = o.d_indices; a.src = o.d_src;
  a.vals = d_vals; a.w = d_w; a.add = d_add; a.y = d_y; a.partial = o.d_partial;
  a.n_blocks = o.n_blocks; a.n_longs = o.n_longs; a.mode = mode;
  hipStream_t st = pick(c, stream);
  PK_LIB_LAUNCH(c, pk_red_rows, red_rows_host, lib_grid(o.n_blocks), st, a);
  if (o.n_longs) PK_LIB_LAUNCH(c, pk_red_long, red_long_host, lib_grid(o.n_longs), st, a);
  return 0;
}

int pk_set_operator_diagonal(pk_ctx* c, int op, const int32_t* pos, int32_t n) {
  int rc = ready(c);
  if (rc) return rc;
  if (op < 0 || op > 2) return fail(c, 110, "pk_set_operator_diagonal: op must be 0 (J), 1 (J^T) or 2 (H symmetric)");
  if (!pos) return fail(c, 110, "pk_set_operator_diagonal: null positions");
  if (c->shard.flags || c->exchange.world > 1) return fail(c, 119, "pk_set_operator_diagonal: not offered for a sharded context");
  if (op != 2) return fail(c, 130, "pk_set_operator_diagonal: operator %d is not square, only H (op 2) has a diagonal", op);
  const int64_t n_unique = c->csr[1].n_unique;
  if (n_unique == 0)
    return fail(c, 111, "pk_set_operator_diagonal: call pk_set_csr_map(1) first (the positions point into that map's CSR array)");
  if (n != c->n) return fail(c, 131, "pk_set_operator_diagonal: %d positions for %d rows", n, c->n);
  for (int32_t i = 0; i < n; ++i)
    if (pos[i] < -1 || pos[i] >= n_unique)
      return fail(c, 131, "pk_set_operator_diagonal: pos[%d] = %d is neither -1 nor below %lld", i, pos[i], (long long)n_unique);
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipDeviceSynchronize());      // (a diagonal enqueued earlier, on any stream, may still read the old positions)
  release(c->ops.d_diag_pos);
  return upload(c, (void**)&c->ops.d_diag_pos, pos, sizeof(int32_t) * (size_t)n);
}

int pk_operator_diagonal_dev(pk_ctx* c, int op, const double* d_vals, const double* d_add, double* d_y, void* stream) {
  int rc = ready(c);
  if (rc || (rc = diag_ready(c, op, d_vals && d_y, "pk_operator_diagonal"))) return rc;
  PkDiagArgs a{};
  a.pos = c->ops.d_diag_pos; a.vals = d_vals; a.add = d_add; a.y = d_y; a.n = c->n;
  hipStream_t st = pick(c, stream);
  if (c->n > 0) PK_LIB_LAUNCH(c, pk_diag, diag_host, lib_grid(diag_items(c->n)), st, a);
  return 0;
}

int pk_operator_reduce(pk_ctx* c, int op, int mode, const double* w, int add_diagonal, double* y) {
  const double *vals = nullptr, *hvals = nullptr;
  const char* who = "pk_operator_reduce";
  int rc = host_ready(c, y != nullptr);
  if (rc || (rc = op_ready(c, op, true, who)) || (rc = bad_mode(c, mode, who)) || (rc = op_linearized(c, op, vals, who))) return rc;
  const PkOperator& o = c->ops.op[op];
  if (add_diagonal) {      // diag(H) under the rows: they must be H's
    if (o.n_rows != c->n || op == 0) return fail(c, 130, "%s: the diagonal of H cannot be added to the %d rows of operator %d", who, o.n_rows, op);
    if ((rc = diag_ready(c, 2, true, who)) || (rc = op_linearized(c, 2, hvals, who))) return rc;
  }
  if ((rc = host_scratch(c))) return rc;
  PK_HIP(c, hipSetDevice(c->device));
  if (w) PK_HIP(c, hipMemcpyAsync(c->ops.d_v, w, sizeof(double) * (size_t)o.n_cols, hipMemcpyHostToDevice, c->stream));
  if (add_diagonal && (rc = pk_operator_diagonal_dev(c, 2, hvals, nullptr, c->ops.d_y, nullptr))) return rc;
  if ((rc = pk_operator_reduce_dev(c, op, mode, vals, w ? c->ops.d_v : nullptr, add_diagonal ? c->ops.d_y : nullptr, c->ops.d_y, nullptr)))
    return rc;
  PK_HIP(c, hipMemcpyAsync(y, c->ops.d_y, sizeof(double) * (size_t)o.n_rows, hipMemcpyDeviceToHost, c->stream));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int pk_operator_diagonal(pk_ctx* c, int op, double* y) {
  const double* vals = nullptr;
  int rc = host_ready(c, y != nullptr);
  if (rc || (rc = diag_ready(c, op, true, "pk_operator_diagonal")) || (rc = op_linearized(c, 2, vals, "pk_operator_diagonal"))) return rc;
  if ((rc = host_scratch(c))) return rc;
  if ((rc = pk_operator_diagonal_dev(c, 2, vals, nullptr, c->ops.d_y, nullptr))) return rc;
  PK_HIP(c, hipMemcpyAsync(y, c->ops.d_y, sizeof(double) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
