// pk_ops.cpp -- the matrices of the CSR hand-off applied to vectors where their values lie: y = J v, y = J^T v and
// y = H v (H symmetric, stored as its lower triangle) on the device, from the CSR value arrays pk_csr fills (pk_extras.cpp).
// Model-independent, so the two kernels live in the library like the shim's copy kernel, not in the generated code object.
//
// An operator is a CSR structure (indptr, indices) whose entry e takes its value from vals[src[e]] (src NULL: vals[e]): J^T
// and the mirrored half of H point into the values of the map they were built from (pockit_amd/csr.py), nothing is copied or
// transposed per iterate.  Its rows are cut ONCE, on the host, into work items of one 256-thread workgroup (pk_op_row_blocks):
//
//   stream block  consecutive whole rows with at most 256 entries (and 256 rows) together: one entry per thread, the products
//                 meet in LDS, thread r adds the products of row r in ascending entry order
//   piece block   256 consecutive entries of a row with more than 256 of them (the column of t_f in J^T): a fixed tree over
//                 the 256 LDS slots leaves one partial sum; pk_op_long, one workgroup per long row, adds a row's partial sums
//
// Every y[row] is a fixed expression of the inputs: no atomics, no dependence on the grid, the same bits from run to run.
//
// A BLOCK of k vectors (pk_apply_operator_block[_dev]: Y = A V (+ Add), V and Y row-major with leading dimensions) walks the
// same row blocks in chunks of at most PK_OP_KMAX columns: pk_op_rows_k / pk_op_long_k read the structure and the values once
// per chunk and keep one LDS plane of products per column.  Column j of Y has exactly the bits of the single product with
// column j of V: the association per (row, column) is the one above.
#include "pk_oprows.h"

// ---------------------------------------------------------------- row blocks (host, once per operator)
int pk_op_row_blocks(const int32_t* indptr, int32_t n_rows, std::vector<PkOpBlock>& blocks, std::vector<PkOpLong>& longs,
                     int32_t& n_slots) {
  blocks.clear();
  longs.clear();
  int64_t slots = 0;
  for (int32_t r = 0; r < n_rows;) {
    const int32_t e0 = indptr[r], len = indptr[r + 1] - e0;
    if (len > PK_BLOCK) {
      const int32_t pieces = (len + PK_BLOCK - 1) / PK_BLOCK;
      if (slots + pieces > INT32_MAX) return 1;
      longs.push_back({r, (int32_t)slots, pieces});
      for (int32_t p = 0; p < pieces; ++p)
        blocks.push_back({e0 + p * PK_BLOCK, std::min<int32_t>(PK_BLOCK, len - p * PK_BLOCK), (int32_t)slots + p, -1});
      slots += pieces;
      ++r;
    } else {
      const int32_t r0 = r;
      while (r < n_rows && r - r0 < PK_BLOCK && indptr[r + 1] - indptr[r] <= PK_BLOCK && indptr[r + 1] - e0 <= PK_BLOCK) ++r;
      blocks.push_back({e0, indptr[r] - e0, r0, r - r0});
    }
    if (blocks.size() > (size_t)INT32_MAX) return 1;
  }
  n_slots = (int32_t)slots;
  return 0;
}

// ---------------------------------------------------------------- the walk of one block, shared by the kernels and the host stand-in
// (the function macro, the tree's driver, the grid rule, the host walk and the launch are pk_libkernel.h's; the padded LDS
// slots, PK_OP_LDS and op_slot, are pk_oprows.h's, shared with the reductions of pk_reduce.cpp)
struct PkOpArgs {
  const PkOpBlock* blocks;
  const PkOpLong* longs;
  const int32_t *indptr, *indices, *src;
  const double *vals, *v, *add;      // add may be NULL, and may alias y
  double *y, *partial;
  int32_t n_blocks, n_longs;
};

// thread t of a block: its product (0 beyond the block's count)
PK_LIB_FN double op_product(const PkOpArgs& a, const PkOpBlock& b, int t) {
  if (t >= b.count) return 0.0;
  const int32_t e = b.e0 + t;
  return a.vals[a.src ? a.src[e] : e] * a.v[a.indices[e]];
}

// thread r < n_rows of a stream block: the products of its row in ascending entry order
PK_LIB_FN void op_row_sum(const PkOpArgs& a, const PkOpBlock& b, int r, const double* s) {
  const int32_t row = b.row0 + r;
  const int lo = a.indptr[row] - b.e0, hi = a.indptr[row + 1] - b.e0;
  double sum = 0.0;
  for (int k = lo; k < hi; ++k) sum += s[op_slot(k)];
  a.y[row] = a.add ? sum + a.add[row] : sum;
}

// thread t of a long row: its partial sums first + t, first + t + 256, ... in ascending order
PK_LIB_FN double op_long_strided(const PkOpArgs& a, const PkOpLong& l, int t) {
  double sum = 0.0;
  for (int32_t k = t; k < l.pieces; k += PK_BLOCK) sum += a.partial[l.first + k];
  return sum;
}

// one step of the fixed tree over the 256 slots (lib_tree: widths 128, 64 ... 1; the sum ends in s[0])
PK_LIB_FN void op_tree_step(double* s, int w, int t) {
  if (t < w) s[op_slot(t)] += s[op_slot(t + w)];
}

// ---------------------------------------------------------------- the same walk for a chunk of kc <= PK_OP_KMAX columns
// One LDS plane of PK_OP_LDS slots per column, the planes behind one another: product (i, c) lies at c * PK_OP_LDS + op_slot(i).
// The lanes of a half-wave work on consecutive i of ONE plane wherever the workgroup is full (the stores of the products, the
// row sums of a block with 32 rows or more, the wide levels of the tree), so the bank reasoning of op_slot carries over plane
// by plane; a plane's 264 doubles shift the next one by 8 doubles = 16 banks, which matters only where a half-wave crosses
// planes (blocks of fewer than 32 rows, tree levels below 32).  Not measured.
struct PkOpArgsK {
  PkOpArgs a;            // v, add and y point at the chunk's first column; partial holds PK_OP_KMAX doubles per slot
  int64_t ldv, ldy;      // doubles between two rows of V, and of Y and Add
  int32_t kc;            // columns of this chunk
};

// two doubles from a 16-byte aligned address: one 16-byte load
PK_LIB_FN void op_load_pair(const double* p, double& x, double& y) {
  double q[2];
  __builtin_memcpy(q, __builtin_assume_aligned(p, 16), sizeof q);
  x = q[0];
  y = q[1];
}

// thread t of a block: its kc products into the planes (0 beyond the block's count); value, column and src are read once
PK_LIB_FN void op_products_k(const PkOpArgsK& k, const PkOpBlock& b, int t, double* s) {
  const PkOpArgs& a = k.a;
  double* p = s + op_slot(t);
  if (t >= b.count) {
    for (int c = 0; c < k.kc; ++c) p[c * PK_OP_LDS] = 0.0;
    return;
  }
  const int32_t e = b.e0 + t;
  const double val = a.vals[a.src ? a.src[e] : e];
  const double* v = a.v + (int64_t)a.indices[e] * k.ldv;
  int c = 0;
  if (((((uintptr_t)a.v) | ((uintptr_t)k.ldv << 3)) & 15) == 0)      // (uniform over the launch) every row of the chunk is 16-byte aligned
    for (; c + 1 < k.kc; c += 2) {
      double x, y;
      op_load_pair(v + c, x, y);
      p[c * PK_OP_LDS] = val * x;
      p[(c + 1) * PK_OP_LDS] = val * y;
    }
  for (; c < k.kc; ++c) p[c * PK_OP_LDS] = val * v[c];
}

// thread t of a stream block: the n_rows x kc sums are spread over the workgroup, PK_BLOCK / n_rows columns side by side --
// thread q * n_rows + r takes row r in the columns q, q + PK_BLOCK / n_rows, ... -- each the products of its row in its plane
// in ascending entry order.  Every (row, column) has one writer, which reads add first.
PK_LIB_FN void op_row_sums_k(const PkOpArgsK& k, const PkOpBlock& b, int t, const double* s) {
  const PkOpArgs& a = k.a;
  if (b.n_rows <= 0) return;
  const int step = PK_BLOCK / b.n_rows, q = t / b.n_rows, r = t - q * b.n_rows;
  if (q >= step) return;      // (the threads behind the last whole group of n_rows)
  const int32_t row = b.row0 + r;
  const int lo = a.indptr[row] - b.e0, hi = a.indptr[row + 1] - b.e0;
  for (int c = q; c < k.kc; c += step) {
    const double* p = s + c * PK_OP_LDS;
    double sum = 0.0;
    for (int i = lo; i < hi; ++i) sum += p[op_slot(i)];
    const int64_t at = (int64_t)row * k.ldy + c;
    a.y[at] = a.add ? sum + a.add[at] : sum;
  }
}

// thread t of a long row: per column its partial sums first + t, first + t + 256, ... in ascending order
PK_LIB_FN void op_long_strided_k(const PkOpArgsK& k, const PkOpLong& l, int t, double* s) {
  for (int c = 0; c < k.kc; ++c) {
    double sum = 0.0;
    for (int32_t j = t; j < l.pieces; j += PK_BLOCK) sum += k.a.partial[(int64_t)(l.first + j) * PK_OP_KMAX + c];
    s[c * PK_OP_LDS + op_slot(t)] = sum;
  }
}

// one step of the kc trees, which share the barrier of the level: the PK_BLOCK / w groups of w threads take a column each
PK_LIB_FN void op_tree_step_k(double* s, int w, int t, int kc) {
  const int i = t & (w - 1);
  for (int c = t / w; c < kc; c += PK_BLOCK / w) {
    double* p = s + c * PK_OP_LDS;
    p[op_slot(i)] += p[op_slot(i + w)];
  }
}

// thread t < kc behind the trees: the sum of column t
PK_LIB_FN void op_store_partial_k(const PkOpArgsK& k, const PkOpBlock& b, int t, const double* s) {
  k.a.partial[(int64_t)b.row0 * PK_OP_KMAX + t] = s[t * PK_OP_LDS];
}
PK_LIB_FN void op_store_long_k(const PkOpArgsK& k, const PkOpLong& l, int t, const double* s) {
  const int64_t at = (int64_t)l.row * k.ldy + t;
  const double sum = s[t * PK_OP_LDS];
  k.a.y[at] = k.a.add ? sum + k.a.add[at] : sum;
}

#ifdef __HIPCC__
// ---------------------------------------------------------------- kernels (gfx950)
__global__ void __launch_bounds__(PK_BLOCK) pk_op_rows(PkOpArgs a) {
  __shared__ double s[PK_OP_LDS];
  const int t = (int)threadIdx.x;
  for (int32_t i = (int32_t)blockIdx.x; i < a.n_blocks; i += (int32_t)gridDim.x) {
    const PkOpBlock b = a.blocks[i];
    s[op_slot(t)] = op_product(a, b, t);
    __syncthreads();
    if (b.n_rows >= 0) {      // (uniform over the workgroup)
      if (t < b.n_rows) op_row_sum(a, b, t, s);
    } else {
      lib_tree(op_tree_step, s, t);
      if (t == 0) a.partial[b.row0] = s[0];
    }
    __syncthreads();          // the next block of this workgroup's stride overwrites the slots
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_op_long(PkOpArgs a) {
  __shared__ double s[PK_OP_LDS];
  const int t = (int)threadIdx.x;
  for (int32_t i = (int32_t)blockIdx.x; i < a.n_longs; i += (int32_t)gridDim.x) {
    const PkOpLong l = a.longs[i];
    s[op_slot(t)] = op_long_strided(a, l, t);
    __syncthreads();
    lib_tree(op_tree_step, s, t);
    if (t == 0) a.y[l.row] = a.add ? s[0] + a.add[l.row] : s[0];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_op_rows_k(PkOpArgsK k) {
  __shared__ double s[PK_OP_KMAX * PK_OP_LDS];
  const int t = (int)threadIdx.x;
  for (int32_t i = (int32_t)blockIdx.x; i < k.a.n_blocks; i += (int32_t)gridDim.x) {
    const PkOpBlock b = k.a.blocks[i];
    op_products_k(k, b, t, s);
    __syncthreads();
    if (b.n_rows >= 0) {      // (uniform over the workgroup)
      op_row_sums_k(k, b, t, s);
    } else {
      lib_tree(op_tree_step_k, s, t, k.kc);      // (column c ends in s[c * PK_OP_LDS])
      if (t < k.kc) op_store_partial_k(k, b, t, s);
    }
    __syncthreads();          // the next block of this workgroup's stride overwrites the planes
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_op_long_k(PkOpArgsK k) {
  __shared__ double s[PK_OP_KMAX * PK_OP_LDS];
  const int t = (int)threadIdx.x;
  for (int32_t i = (int32_t)blockIdx.x; i < k.a.n_longs; i += (int32_t)gridDim.x) {
    const PkOpLong l = k.a.longs[i];
    op_long_strided_k(k, l, t, s);
    __syncthreads();
    lib_tree(op_tree_step_k, s, t, k.kc);      // (column c ends in s[c * PK_OP_LDS])
    if (t < k.kc) op_store_long_k(k, l, t, s);
    __syncthreads();
  }
}
#else
// ---------------------------------------------------------------- host stand-in: the identical walk over the same tables
static void op_rows_host(const PkOpArgs& a, unsigned grid) {
  double s[PK_OP_LDS];
  lib_walk_host(grid, a.n_blocks, [&](int64_t i) {
    const PkOpBlock b = a.blocks[i];
    for (int t = 0; t < PK_BLOCK; ++t) s[op_slot(t)] = op_product(a, b, t);
    if (b.n_rows >= 0) {
      for (int t = 0; t < b.n_rows; ++t) op_row_sum(a, b, t, s);
    } else {
      lib_tree_host(op_tree_step, s);
      a.partial[b.row0] = s[0];
    }
  });
}

static void op_long_host(const PkOpArgs& a, unsigned grid) {
  double s[PK_OP_LDS];
  lib_walk_host(grid, a.n_longs, [&](int64_t i) {
    const PkOpLong l = a.longs[i];
    for (int t = 0; t < PK_BLOCK; ++t) s[op_slot(t)] = op_long_strided(a, l, t);
    lib_tree_host(op_tree_step, s);
    a.y[l.row] = a.add ? s[0] + a.add[l.row] : s[0];
  });
}

static void op_rows_k_host(const PkOpArgsK& k, unsigned grid) {
  std::vector<double> planes((size_t)PK_OP_KMAX * PK_OP_LDS);
  double* s = planes.data();
  lib_walk_host(grid, k.a.n_blocks, [&](int64_t i) {
    const PkOpBlock b = k.a.blocks[i];
    for (int t = 0; t < PK_BLOCK; ++t) op_products_k(k, b, t, s);
    if (b.n_rows >= 0) {
      for (int t = 0; t < PK_BLOCK; ++t) op_row_sums_k(k, b, t, s);
    } else {
      lib_tree_host(op_tree_step_k, s, k.kc);
      for (int t = 0; t < k.kc; ++t) op_store_partial_k(k, b, t, s);
    }
  });
}

static void op_long_k_host(const PkOpArgsK& k, unsigned grid) {
  std::vector<double> planes((size_t)PK_OP_KMAX * PK_OP_LDS);
  double* s = planes.data();
  lib_walk_host(grid, k.a.n_longs, [&](int64_t i) {
    const PkOpLong l = k.a.longs[i];
    for (int t = 0; t < PK_BLOCK; ++t) op_long_strided_k(k, l, t, s);
    lib_tree_host(op_tree_step_k, s, k.kc);
    for (int t = 0; t < k.kc; ++t) op_store_long_k(k, l, t, s);
  });
}
#endif

static void free_operator(PkOperator& o) {
  release(o.d_indptr); release(o.d_indices); release(o.d_src); release(o.d_blocks); release(o.d_longs); release(o.d_partial);
  release(o.d_partial_k);
  o = PkOperator{};
}

void free_operators(pk_ctx* c) {
  for (auto& o : c->ops.op) free_operator(o);
  release(c->ops.d_v); release(c->ops.d_y); release(c->ops.d_diag_pos);
  c->ops.scratch_k = 0;
  c->ops.lin_J = c->ops.lin_H = nullptr;
  solve_forget(c->cg);      // (a solve in progress holds pointers into what the operators were built from)
  solve_forget(c->minres);
}

void drop_linearization(pk_ctx* c) { c->ops.lin_J = c->ops.lin_H = nullptr; }

// The entry checks of the pk_apply_operator* and pk_operator_reduce* entry points, in the order they fire; ``who`` is the name
// in the message.
int op_ready(pk_ctx* c, int op, bool pointers, const char* who) {
  if (op < 0 || op > 2) return fail(c, 110, "%s: op must be 0 (J), 1 (J^T) or 2 (H symmetric)", who);
  if (c->ops.op[op].n_blocks == 0) return fail(c, 117, "%s: call pk_set_csr_operator(%d) first", who, op);
  if (!pointers) return fail(c, 110, "%s: null device pointer", who);
  return 0;
}

// ... and of the host forms behind it: the value array pk_linearize left for this operator
int op_linearized(pk_ctx* c, int op, const double*& vals, const char* who) {
  vals = op == 2 ? c->ops.lin_H : c->ops.lin_J;
  if (!vals && op == 2 && c->ops.lin_J) return fail(c, 118, "%s: the linearization has no Hessian (pk_linearize without lambda)", who);
  if (!vals) return fail(c, 118, "%s: no linearization (pk_linearize)", who);
  return 0;
}

extern "C" {

int pk_set_csr_operator(pk_ctx* c, int op, const int32_t* indptr, const int32_t* indices, const int32_t* src, int32_t n_rows,
                        int32_t n_cols, int64_t nnz) {
  int rc = ready(c);
  if (rc) return rc;
  if (op < 0 || op > 2) return fail(c, 110, "pk_set_csr_operator: op must be 0 (J), 1 (J^T) or 2 (H symmetric)");
  if (!indptr || !indices) return fail(c, 110, "pk_set_csr_operator: null structure");
  if (c->shard.flags || c->exchange.world > 1) return fail(c, 119, "pk_set_csr_operator: not offered for a sharded context");
  const int64_t n_unique = c->csr[op == 2 ? 1 : 0].n_unique;
  if (n_unique == 0)
    return fail(c, 111, "pk_set_csr_operator: call pk_set_csr_map(%d) first (the operator takes its values from that map's CSR array)", op == 2 ? 1 : 0);
  const int32_t want_rows = op == 0 ? c->m : c->n, want_cols = op == 1 ? c->m : c->n;
  if (n_rows != want_rows || n_cols != want_cols || nnz <= 0 || (!src && nnz != n_unique))
    return fail(c, 112, "pk_set_csr_operator: %d x %d with %lld entries does not match the problem (%d x %d%s)", n_rows, n_cols,
                (long long)nnz, want_rows, want_cols, src ? "" : ", one entry per CSR value without src");
  if (nnz > INT32_MAX) return fail(c, 116, "pk_set_csr_operator: %lld entries do not fit 32-bit indices", (long long)nnz);
  // validate on the host everything a kernel indexes with
  if (indptr[0] != 0 || indptr[n_rows] != nnz) return fail(c, 113, "pk_set_csr_operator: indptr does not cover the entries");
  for (int32_t r = 0; r < n_rows; ++r)
    if (indptr[r + 1] < indptr[r]) return fail(c, 113, "pk_set_csr_operator: indptr decreases at row %d", r);
  for (int64_t e = 0; e < nnz; ++e)
    if (indices[e] < 0 || indices[e] >= n_cols) return fail(c, 114, "pk_set_csr_operator: indices[%lld] out of range", (long long)e);
  if (src)
    for (int64_t e = 0; e < nnz; ++e)
      if (src[e] < 0 || src[e] >= n_unique) return fail(c, 115, "pk_set_csr_operator: src[%lld] out of range", (long long)e);
  std::vector<PkOpBlock> blocks;
  std::vector<PkOpLong> longs;
  int32_t n_slots = 0;
  if (pk_op_row_blocks(indptr, n_rows, blocks, longs, n_slots))
    return fail(c, 116, "pk_set_csr_operator: the row blocks do not fit 32-bit counts");
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  PkOperator& o = c->ops.op[op];
  free_operator(o);
  solve_forget(c->cg);
  solve_forget(c->minres);
  if ((rc = upload(c, (void**)&o.d_indptr, indptr, sizeof(int32_t) * ((size_t)n_rows + 1)))) return rc;
  if ((rc = upload(c, (void**)&o.d_indices, indices, sizeof(int32_t) * (size_t)nnz))) return rc;
  if (src && (rc = upload(c, (void**)&o.d_src, src, sizeof(int32_t) * (size_t)nnz))) return rc;
  if ((rc = upload(c, (void**)&o.d_blocks, blocks.data(), sizeof(PkOpBlock) * blocks.size()))) return rc;
  if (!longs.empty()) {
    if ((rc = upload(c, (void**)&o.d_longs, longs.data(), sizeof(PkOpLong) * longs.size()))) return rc;
    PK_HIP(c, hipMalloc((void**)&o.d_partial, sizeof(double) * (size_t)n_slots));
  }
  if (!c->ops.d_v) {      // scratch vectors of the host form (pk_apply_operator): every operator's v and y fit
    const size_t len = (size_t)std::max(c->n, c->m);
    PK_HIP(c, hipMalloc((void**)&c->ops.d_v, sizeof(double) * len));
    PK_HIP(c, hipMalloc((void**)&c->ops.d_y, sizeof(double) * len));
    c->ops.scratch_k = 1;
  }
  o.n_rows = n_rows; o.n_cols = n_cols; o.nnz = nnz; o.n_slots = n_slots;
  o.n_blocks = (int32_t)blocks.size(); o.n_longs = (int32_t)longs.size();
  return 0;
}

int pk_apply_operator_dev(pk_ctx* c, int op, const double* d_vals, const double* d_v, const double* d_add, double* d_y,
                          void* stream) {
  int rc = ready(c);
  if (rc || (rc = op_ready(c, op, d_vals && d_v && d_y, "pk_apply_operator"))) return rc;
  const PkOperator& o = c->ops.op[op];
  PkOpArgs a{};
  a.blocks = o.d_blocks; a.longs = o.d_longs; a.indptr = o.d_indptr; a.indices = o.d_indices; a.src = o.d_src;
  a.vals = d_vals; a.v = d_v; a.add = d_add; a.y = d_y; a.partial = o.d_partial;
  a.n_blocks = o.n_blocks; a.n_longs = o.n_longs;
  hipStream_t st = pick(c, stream);
  PK_LIB_LAUNCH(c, pk_op_rows, op_rows_host, lib_grid(o.n_blocks), st, a);
  if (o.n_longs) PK_LIB_LAUNCH(c, pk_op_long, op_long_host, lib_grid(o.n_longs), st, a);
  return 0;
}

int pk_apply_operator_block_dev(pk_ctx* c, int op, const double* d_vals, int32_t k, const double* d_V, int64_t ldv,
                                const double* d_Add, double* d_Y, int64_t ldy, void* stream) {
  int rc = ready(c);
  if (rc || (rc = op_ready(c, op, d_vals && d_V && d_Y, "pk_apply_operator_block"))) return rc;
  PkOperator& o = c->ops.op[op];
  if (k < 1) return fail(c, 120, "pk_apply_operator_block: k = %d, a block has at least one column", k);
  if (ldv < k || ldy < k)
    return fail(c, 121, "pk_apply_operator_block: leading dimensions %lld / %lld are smaller than k = %d", (long long)ldv, (long long)ldy, k);
  if (o.n_longs && !o.d_partial_k) {      // the first block product of an operator with long rows
    PK_HIP(c, hipSetDevice(c->device));
    if (hipMalloc((void**)&o.d_partial_k, sizeof(double) * (size_t)o.n_slots * PK_OP_KMAX) != hipSuccess) {
      o.d_partial_k = nullptr;
      return fail(c, 122, "pk_apply_operator_block: no device memory for %d x %d partial sums", o.n_slots, (int)PK_OP_KMAX);
    }
  }
  PkOpArgsK a{};
  a.a.blocks = o.d_blocks; a.a.longs = o.d_longs; a.a.indptr = o.d_indptr; a.a.indices = o.d_indices; a.a.src = o.d_src;
  a.a.vals = d_vals; a.a.partial = o.d_partial_k;
  a.a.n_blocks = o.n_blocks; a.a.n_longs = o.n_longs;
  a.ldv = ldv; a.ldy = ldy;
  hipStream_t st = pick(c, stream);
  // chunks of PK_OP_KMAX columns, the last one narrower; the launches are ordered by the stream, so they share the partial sums
  for (int32_t c0 = 0; c0 < k; c0 += PK_OP_KMAX) {
    a.kc = std::min<int32_t>(PK_OP_KMAX, k - c0);
    a.a.v = d_V + c0; a.a.add = d_Add ? d_Add + c0 : nullptr; a.a.y = d_Y + c0;
    PK_LIB_LAUNCH(c, pk_op_rows_k, op_rows_k_host, lib_grid(o.n_blocks), st, a);
    if (o.n_longs) PK_LIB_LAUNCH(c, pk_op_long_k, op_long_k_host, lib_grid(o.n_longs), st, a);
  }
  return 0;
}

int pk_linearize(pk_ctx* c, const double* x, const double* lambda, double sigma) {
  if (const int rc = host_ready(c, x != nullptr)) return rc;
  const PkCsrMap& mj = c->csr[c->csr[3].n_unique > 0 ? 3 : 0];      // (the value arrays pk_eval_jac_csr / pk_eval_hess_csr choose)
  const PkCsrMap& mh = c->csr[c->csr[2].n_unique > 0 ? 2 : 1];
  if (mj.n_unique == 0 || (lambda && mh.n_unique == 0))
    return fail(c, 111, "pk_linearize: call pk_set_csr_map first (0%s)", lambda ? " and 1" : "");
  drop_linearization(c);
  const int rc = host_eval(c, x, lambda, {}, false, [&] {
    const int rj = pk_eval_jac_csr_dev(c, c->d_x, mj.d_vals, nullptr);
    return rj || !lambda ? rj : pk_eval_hess_csr_dev(c, c->d_x, c->d_lam, sigma, mh.d_vals, nullptr);
  });
  if (rc) return rc;
  c->ops.lin_J = mj.d_vals;
  c->ops.lin_H = lambda ? mh.d_vals : nullptr;
  return 0;
}

int pk_apply_operator(pk_ctx* c, int op, const double* v, double* y) {
  const double* vals = nullptr;
  int rc = host_ready(c, v && y);
  if (rc || (rc = op_ready(c, op, true, "pk_apply_operator")) || (rc = op_linearized(c, op, vals, "pk_apply_operator"))) return rc;
  const PkOperator& o = c->ops.op[op];
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipMemcpyAsync(c->ops.d_v, v, sizeof(double) * (size_t)o.n_cols, hipMemcpyHostToDevice, c->stream));
  if ((rc = pk_apply_operator_dev(c, op, vals, c->ops.d_v, nullptr, c->ops.d_y, nullptr))) return rc;
  PK_HIP(c, hipMemcpyAsync(y, c->ops.d_y, sizeof(double) * (size_t)o.n_rows, hipMemcpyDeviceToHost, c->stream));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int pk_apply_operator_block(pk_ctx* c, int op, int32_t k, const double* V, double* Y) {
  const double* vals = nullptr;
  int rc = host_ready(c, V && Y);
  if (rc || (rc = op_ready(c, op, true, "pk_apply_operator_block")) || (rc = op_linearized(c, op, vals, "pk_apply_operator_block"))) return rc;
  const PkOperator& o = c->ops.op[op];
  if (k < 1) return fail(c, 120, "pk_apply_operator_block: k = %d, a block has at least one column", k);
  PK_HIP(c, hipSetDevice(c->device));
  if (k > c->ops.scratch_k) {      // the scratch grows to the widest block seen and never shrinks short of free_operators
    const size_t len = (size_t)std::max(c->n, c->m) * (size_t)k;
    double *v = nullptr, *y = nullptr;
    if (hipMalloc((void**)&v, sizeof(double) * len) != hipSuccess || hipMalloc((void**)&y, sizeof(double) * len) != hipSuccess) {
      release(v);
      return fail(c, 122, "pk_apply_operator_block: no device memory for two scratch blocks of %zu doubles", len);
    }
    const hipError_t e = hipStreamSynchronize(c->stream);      // (a product enqueued earlier may still read the old ones)
    if (e != hipSuccess) {
      release(v); release(y);
      return fail(c, 100 + (int)e, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    }
    release(c->ops.d_v); release(c->ops.d_y);
    c->ops.d_v = v; c->ops.d_y = y; c->ops.scratch_k = k;
  }
  PK_HIP(c, hipMemcpyAsync(c->ops.d_v, V, sizeof(double) * (size_t)o.n_cols * (size_t)k, hipMemcpyHostToDevice, c->stream));
  if ((rc = pk_apply_operator_block_dev(c, op, vals, k, c->ops.d_v, k, nullptr, c->ops.d_y, k, nullptr))) return rc;
  PK_HIP(c, hipMemcpyAsync(Y, c->ops.d_y, sizeof(double) * (size_t)o.n_rows * (size_t)k, hipMemcpyDeviceToHost, c->stream));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
