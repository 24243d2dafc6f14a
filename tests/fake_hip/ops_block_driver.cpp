// ops_block_driver.cpp -- TEST INFRASTRUCTURE: drives the BLOCK form of the operator entry points (pk_apply_operator_block[_dev],
// pockit_amd/csrc/pk_ops.cpp) against the host-only HIP stand-in of this directory, built with -fsanitize=address,undefined
// (tests/test_csr_operator_block_cpu.py).  The host walk of pk_op_rows_k / pk_op_long_k over the block tables the kernels read,
// on matrices and blocks of small integers: every sum is exact in fp64, so Y must EQUAL a plain triple loop, and column j must
// equal the single-vector stand-in on column j.  Leading dimensions larger than k with sentinels in the padding, Add absent,
// separate and aliasing Y, every refusal, the host form's scratch growing, what drops everything, tear-down without a live
// allocation.  (Error 122, a failed allocation, is not reached: the stand-in's hipMalloc never fails.)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "driver_common.h"
#include "../../pockit_amd/csrc/pk_runtime.h"      // (the context's operator tables: d_partial_k, scratch_k)


// a row-major block: rows x k in a buffer of leading dimension ld, the padding filled with ``pad``
struct Block {
  int32_t rows, k;
  int64_t ld;
  std::vector<double> data;
  Block(int32_t rows_, int32_t k_, int64_t ld_, double pad) : rows(rows_), k(k_), ld(ld_), data((size_t)rows_ * (size_t)ld_, pad) {}
  double& at(int32_t r, int32_t j) { return data[(size_t)r * (size_t)ld + (size_t)j]; }
  double at(int32_t r, int32_t j) const { return data[(size_t)r * (size_t)ld + (size_t)j]; }
  bool padding_is(double pad) const {
    for (int32_t r = 0; r < rows; ++r)
      for (int64_t j = k; j < ld; ++j)
        if (data[(size_t)r * (size_t)ld + (size_t)j] != pad) return false;
    return true;
  }
  std::vector<double> column(int32_t j) const {
    std::vector<double> c((size_t)rows);
    for (int32_t r = 0; r < rows; ++r) c[(size_t)r] = at(r, j);
    return c;
  }
};

// the reference: a plain triple loop over rows, columns of the block and entries, dense rows x k
static std::vector<double> reference(const Csr& A, const std::vector<double>& vals, const Block& V, const Block* add) {
  std::vector<double> y((size_t)A.rows * (size_t)V.k);
  for (int32_t r = 0; r < A.rows; ++r)
    for (int32_t j = 0; j < V.k; ++j) {
      double sum = 0.0;
      for (int32_t e = A.indptr[(size_t)r]; e < A.indptr[(size_t)r + 1]; ++e)
        sum += vals[(size_t)(A.src.empty() ? e : A.src[(size_t)e])] * V.at(A.indices[(size_t)e], j);
      y[(size_t)r * (size_t)V.k + (size_t)j] = sum + (add ? add->at(r, j) : 0.0);
    }
  return y;
}

static bool equals(const Block& Y, const std::vector<double>& want) {
  for (int32_t r = 0; r < Y.rows; ++r)
    for (int32_t j = 0; j < Y.k; ++j)
      if (Y.at(r, j) != want[(size_t)r * (size_t)Y.k + (size_t)j]) return false;
  return true;
}

static const int32_t KS[] = {1, 2, 3, 7, 8, 9, 17};

// Y = A V for every k, with ld = k and with padded leading dimensions; Add absent, separate and aliasing Y; against the
// triple loop and, column by column, against the single-vector walk
static void check_block_products(int op, const Csr& A, const std::vector<double>& vals) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (const int32_t k : KS)
    for (const int padded : {0, 1}) {
      const int64_t ldv = k + (padded ? 2 : 0), ldy = k + (padded ? 3 : 0);
      Block V(A.cols, k, ldv, nan), add(A.rows, k, ldy, nan);      // (a NaN read from the padding would poison the row)
      for (int32_t i = 0; i < A.cols; ++i)
        for (int32_t j = 0; j < k; ++j) V.at(i, j) = small_vec(3 * i + 5 * j + op);
      for (int32_t r = 0; r < A.rows; ++r)
        for (int32_t j = 0; j < k; ++j) add.at(r, j) = small_vec(7 * r + 2 * j + 1);
      const std::vector<double> plain = reference(A, vals, V, nullptr), summed = reference(A, vals, V, &add);
      // the padded block lies one double behind a 16-byte boundary: with an even ldv its rows are 8-byte aligned only
      std::vector<double> shifted(V.data.size() + 3, nan);
      const size_t lead = ((uintptr_t)shifted.data() & 15) == 0 ? 1 : 2;
      std::copy(V.data.begin(), V.data.end(), shifted.begin() + (std::ptrdiff_t)lead);
      const double* d_V = padded ? shifted.data() + lead : V.data.data();
      CHECK(!padded || ((uintptr_t)d_V & 15) == 8);

      Block Y(A.rows, k, ldy, SENTINEL);
      OK(pk_apply_operator_block_dev(ctx, op, vals.data(), k, d_V, ldv, nullptr, Y.data.data(), ldy, nullptr));
      OK(pk_sync(ctx, nullptr));
      CHECK(equals(Y, plain) && Y.padding_is(SENTINEL));

      Block Z(A.rows, k, ldy, SENTINEL);
      OK(pk_apply_operator_block_dev(ctx, op, vals.data(), k, d_V, ldv, add.data.data(), Z.data.data(), ldy, nullptr));
      OK(pk_sync(ctx, nullptr));
      CHECK(equals(Z, summed) && Z.padding_is(SENTINEL));

      Block W(A.rows, k, ldy, SENTINEL);                             // Add aliases Y
      for (int32_t r = 0; r < A.rows; ++r)
        for (int32_t j = 0; j < k; ++j) W.at(r, j) = add.at(r, j);
      OK(pk_apply_operator_block_dev(ctx, op, vals.data(), k, d_V, ldv, W.data.data(), W.data.data(), ldy, nullptr));
      OK(pk_sync(ctx, nullptr));
      CHECK(equals(W, summed) && W.padding_is(SENTINEL));

      for (int32_t j = 0; j < k; ++j) {                              // column j against the single-vector walk on column j
        const std::vector<double> v = V.column(j), a = add.column(j);
        std::vector<double> y((size_t)A.rows, SENTINEL);
        OK(pk_apply_operator_dev(ctx, op, vals.data(), v.data(), nullptr, y.data(), nullptr));
        OK(pk_sync(ctx, nullptr));
        CHECK(y == Y.column(j));
        OK(pk_apply_operator_dev(ctx, op, vals.data(), v.data(), a.data(), y.data(), nullptr));
        OK(pk_sync(ctx, nullptr));
        CHECK(y == Z.column(j));
      }
    }
}

// one synthetic J (rows of the given lengths): J V with src NULL, J^T Y with src; the partial sums of the block form appear
// with an operator's first block product, and only where it has long rows
static void jacobian_case(const std::vector<int32_t>& lens, int32_t cols) {
  const Csr A = from_lengths(lens, cols), T = transposed(A);
  set_problem(cols, A.rows, A.nnz(), 5);
  set_identity_map(0, A.nnz());
  OK(set_operator(0, A));
  OK(set_operator(1, T));
  std::vector<double> vals((size_t)A.nnz());
  for (int64_t e = 0; e < A.nnz(); ++e) vals[(size_t)e] = small_val(e);
  for (int op = 0; op < 2; ++op) CHECK(ctx->ops.op[op].d_partial_k == nullptr);
  check_block_products(0, A, vals);
  check_block_products(1, T, vals);
  for (int op = 0; op < 2; ++op) CHECK((ctx->ops.op[op].d_partial_k != nullptr) == (ctx->ops.op[op].n_longs > 0));
}

int main() {
  load_model();

  // ---- the row lengths at which the walk changes, mixed; 600 consecutive empty rows; a long row first and last, and alone
  jacobian_case({0, 1, 255, 256, 257, 512, 513, 0, 3, 1, 0}, 600);
  {
    std::vector<int32_t> lens = {700, 2, 3};
    lens.insert(lens.end(), 600, 0);
    lens.insert(lens.end(), {4, 0, 0, 5, 300});
    jacobian_case(lens, 701);
  }
  jacobian_case({300}, 300);                                       // a long row alone (its transpose: 300 one-entry rows)
  jacobian_case({257, 600, 256 * 3, 1000}, 1000);                  // only long rows
  jacobian_case(std::vector<int32_t>(500, 3), 40);                 // many short rows: every group size of the row sums; a dense transpose
  jacobian_case(std::vector<int32_t>(2100, 200), 256);             // one row per block: more blocks than the grid cap, the stride loop
  {
    // ---- 65 537 entries in one row: 257 pieces, more than one round of the long row's strided sums
    std::vector<int32_t> lens(600, 2);
    lens[17] = 65537;
    lens[599] = 256;
    jacobian_case(lens, 65600);
  }

  // ---- every refusal: its code, nothing enqueued, nothing written; then the host form
  {
    const Csr A = from_lengths({3, 0, 300, 2}, 400), T = transposed(A);
    set_problem(400, 4, A.nnz(), 9);
    set_identity_map(0, A.nnz());
    std::vector<double> vals((size_t)A.nnz(), 1.0), x(400);
    Block V(400, 17, 17, 0.0), Y(4, 17, 17, SENTINEL), U(4, 17, 17, 0.0), Z(400, 17, 17, SENTINEL);
    for (int i = 0; i < 400; ++i) {
      x[(size_t)i] = 2.0 * (double)(i % 7 - 3);
      for (int j = 0; j < 17; ++j) V.at(i, j) = small_vec(i + 3 * j);
    }
    for (int r = 0; r < 4; ++r)
      for (int j = 0; j < 17; ++j) U.at(r, j) = (double)(r - 2 + j % 3);
    double *v = V.data.data(), *y = Y.data.data();
    CHECK(pk_apply_operator_block_dev(ctx, 0, vals.data(), 2, v, 2, nullptr, y, 2, nullptr) == 117);      // no operator yet
    CHECK(pk_apply_operator_block(ctx, 0, 2, v, y) == 117);
    OK(set_operator(0, A));
    OK(set_operator(1, T));
    const size_t mark = fake_hip_log().size(), launches = fake_hip_launches().size();
    CHECK(pk_apply_operator_block(ctx, 0, 2, v, y) == 118);                                                // no linearization
    CHECK(pk_apply_operator_block_dev(ctx, 3, vals.data(), 2, v, 2, nullptr, y, 2, nullptr) == 110);      // op
    CHECK(pk_apply_operator_block_dev(ctx, -1, vals.data(), 2, v, 2, nullptr, y, 2, nullptr) == 110);
    CHECK(pk_apply_operator_block_dev(ctx, 2, vals.data(), 2, v, 2, nullptr, y, 2, nullptr) == 117);      // H was never set
    CHECK(pk_apply_operator_block_dev(ctx, 0, nullptr, 2, v, 2, nullptr, y, 2, nullptr) == 110);          // null pointers
    CHECK(pk_apply_operator_block_dev(ctx, 0, vals.data(), 2, nullptr, 2, nullptr, y, 2, nullptr) == 110);
    CHECK(pk_apply_operator_block_dev(ctx, 0, vals.data(), 2, v, 2, nullptr, nullptr, 2, nullptr) == 110);
    CHECK(pk_apply_operator_block_dev(ctx, 0, vals.data(), 0, v, 2, nullptr, y, 2, nullptr) == 120);      // k < 1
    CHECK(pk_apply_operator_block_dev(ctx, 0, vals.data(), -4, v, 2, nullptr, y, 2, nullptr) == 120);
    CHECK(pk_apply_operator_block_dev(ctx, 0, vals.data(), 3, v, 2, nullptr, y, 3, nullptr) == 121);      // ldv < k
    CHECK(pk_apply_operator_block_dev(ctx, 0, vals.data(), 3, v, 3, nullptr, y, 2, nullptr) == 121);      // ldy < k
    CHECK(pk_apply_operator_block_dev(ctx, 0, vals.data(), 3, v, 3, nullptr, y, -1, nullptr) == 121);
    CHECK(pk_apply_operator_block(ctx, 5, 2, v, y) == 110);
    CHECK(pk_apply_operator_block(ctx, 0, 2, nullptr, y) == 60 && pk_apply_operator_block(ctx, 0, 2, v, nullptr) == 60);
    CHECK(fake_hip_log().size() == mark && fake_hip_launches().size() == launches);
    OK(pk_linearize(ctx, x.data(), nullptr, 1.0));
    const size_t mark2 = fake_hip_log().size(), launches2 = fake_hip_launches().size();
    CHECK(pk_apply_operator_block(ctx, 0, 0, v, y) == 120);
    CHECK(pk_apply_operator_block(ctx, 2, 2, v, y) == 117);
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark2 && fake_hip_launches().size() == launches2);
    CHECK(Y.padding_is(SENTINEL) && Y.column(0) == std::vector<double>(4, SENTINEL));
    CHECK(ctx->ops.op[0].d_partial_k == nullptr && ctx->ops.scratch_k == 1);      // a refused call allocates nothing

    // ---- the host form: the scratch grows from one column to 2, to 17, and stays there for a narrower block
    for (int64_t e = 0; e < A.nnz(); ++e) vals[(size_t)e] = fake_jac(x.data(), 400, e, false);
    const size_t live = fake_hip_live_allocations();
    for (const int32_t k : {2, 17, 2, 1, 9}) {
      Block Vk(400, k, k, 0.0), Yk(4, k, k, SENTINEL), Uk(4, k, k, 0.0), Zk(400, k, k, SENTINEL);
      for (int i = 0; i < 400; ++i)
        for (int j = 0; j < k; ++j) Vk.at(i, j) = V.at(i, j);
      for (int r = 0; r < 4; ++r)
        for (int j = 0; j < k; ++j) Uk.at(r, j) = U.at(r, j);
      const double* before = ctx->ops.d_v;
      const int64_t had = ctx->ops.scratch_k;
      OK(pk_apply_operator_block(ctx, 0, k, Vk.data.data(), Yk.data.data()));
      CHECK(ctx->ops.scratch_k == std::max<int64_t>(had, k) && (k > had || ctx->ops.d_v == before));
      OK(pk_apply_operator_block(ctx, 1, k, Uk.data.data(), Zk.data.data()));
      CHECK(equals(Yk, reference(A, vals, Vk, nullptr)) && equals(Zk, reference(T, vals, Uk, nullptr)));
      // (J has a long row, J^T has none: one more allocation, the partial sums, from the first block product on; the scratch
      //  is replaced, not added to)
      CHECK(fake_hip_live_allocations() == live + 1);
      for (int32_t j = 0; j < k; ++j) {                              // the single-vector host form on column j
        std::vector<double> yj(4, SENTINEL);
        OK(pk_apply_operator(ctx, 0, Vk.column(j).data(), yj.data()));
        CHECK(yj == Yk.column(j));
      }
    }
    CHECK(ctx->ops.scratch_k == 17 && ctx->ops.op[0].d_partial_k != nullptr && ctx->ops.op[1].d_partial_k == nullptr);

    // ---- a linearization without H, and another evaluation of the value arrays
    Csr L;
    L.rows = L.cols = 400;
    L.indptr.push_back(0);
    for (int32_t r = 0; r < 400; ++r) {
      if (r < 9) L.indices.push_back(r);
      L.indptr.push_back((int32_t)L.indices.size());
    }
    set_identity_map(1, 9);                                            // a new map drops everything of the operators
    for (int op = 0; op < 3; ++op) CHECK(ctx->ops.op[op].n_blocks == 0 && ctx->ops.op[op].d_partial_k == nullptr);
    CHECK(ctx->ops.d_v == nullptr && ctx->ops.d_y == nullptr && ctx->ops.scratch_k == 0);
    CHECK(pk_apply_operator_block(ctx, 0, 2, v, y) == 117);
    OK(set_operator(0, A));
    OK(set_operator(2, L));
    CHECK(ctx->ops.scratch_k == 1);
    CHECK(pk_apply_operator_block(ctx, 0, 2, v, y) == 118);
    OK(pk_linearize(ctx, x.data(), nullptr, 1.0));
    CHECK(pk_apply_operator_block(ctx, 2, 2, v, Z.data.data()) == 118);      // a linearization without H
    OK(pk_apply_operator_block(ctx, 0, 17, v, y));
    CHECK(equals(Y, reference(A, vals, V, nullptr)));
    std::vector<double> jvals((size_t)A.nnz());
    OK(pk_eval_jac_csr(ctx, x.data(), jvals.data()));                  // the value arrays now hold another evaluation
    CHECK(pk_apply_operator_block(ctx, 0, 2, v, y) == 118);
    set_problem(400, 4, A.nnz(), 9);                                   // a new problem drops everything
    CHECK(pk_apply_operator_block_dev(ctx, 0, vals.data(), 2, v, 2, nullptr, y, 2, nullptr) == 117);
    set_identity_map(0, A.nnz());
    OK(set_operator(0, A));
    OK(pk_apply_operator_block_dev(ctx, 0, vals.data(), 2, v, 17, nullptr, y, 17, nullptr));      // torn down with a live partial array
    OK(pk_sync(ctx, nullptr));
    CHECK(ctx->ops.op[0].d_partial_k != nullptr);
  }
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return checks_passed();
}
