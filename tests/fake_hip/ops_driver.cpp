// ops_driver.cpp -- TEST INFRASTRUCTURE: drives the operator entry points of the host runtime (pockit_amd/csrc/pk_ops.cpp) against
// the host-only HIP stand-in of this directory, built with -fsanitize=address,undefined (tests/test_csr_operators_cpu.py): the
// row-block function and the host walk of pk_op_rows / pk_op_long over the same block tables the kernels read, on synthetic
// matrices of small integers (every sum is exact in fp64, so the products must EQUAL a plain loop over the entries), the
// refusals, what drops the operators and the linearization, tear-down without a live allocation.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "driver_common.h"
#include "../../pockit_amd/csrc/pk_runtime.h"      // (pk_op_row_blocks and the context's operator tables)

// the reference: a plain loop over rows, entries and the optional addend
static std::vector<double> reference(const Csr& A, const std::vector<double>& vals, const std::vector<double>& v, const double* add) {
  std::vector<double> y((size_t)A.rows);
  for (int32_t r = 0; r < A.rows; ++r) {
    double sum = 0.0;
    for (int32_t e = A.indptr[(size_t)r]; e < A.indptr[(size_t)r + 1]; ++e)
      sum += vals[(size_t)(A.src.empty() ? e : A.src[(size_t)e])] * v[(size_t)A.indices[(size_t)e]];
    y[(size_t)r] = sum + (add ? add[r] : 0.0);
  }
  return y;
}

// what pk_op_row_blocks promises about a structure
static void check_blocks(const Csr& A) {
  std::vector<PkOpBlock> blocks;
  std::vector<PkOpLong> longs;
  int32_t n_slots = -1;
  OK(pk_op_row_blocks(A.indptr.data(), A.rows, blocks, longs, n_slots));
  int32_t row = 0, entry = 0, slot = 0;
  size_t li = 0;
  for (size_t i = 0; i < blocks.size();) {
    const PkOpBlock& b = blocks[i];
    CHECK(b.e0 == entry && b.count >= 0 && b.count <= PK_BLOCK);
    if (b.n_rows >= 0) {
      CHECK(b.row0 == row && b.n_rows >= 1 && b.n_rows <= PK_BLOCK);
      CHECK(A.indptr[(size_t)row] == b.e0 && A.indptr[(size_t)(row + b.n_rows)] == b.e0 + b.count);
      // greedy: the next row would not have fitted (or is a long one, or there is none)
      if (row + b.n_rows < A.rows && b.n_rows < PK_BLOCK) CHECK(A.indptr[(size_t)(row + b.n_rows + 1)] - b.e0 > PK_BLOCK);
      row += b.n_rows; entry += b.count;
      ++i;
    } else {
      const int32_t len = A.indptr[(size_t)row + 1] - A.indptr[(size_t)row], pieces = (len + PK_BLOCK - 1) / PK_BLOCK;
      CHECK(len > PK_BLOCK && li < longs.size());
      CHECK(longs[li].row == row && longs[li].first == slot && longs[li].pieces == pieces);
      for (int32_t p = 0; p < pieces; ++p, ++i) {
        CHECK(i < blocks.size() && blocks[i].n_rows == -1 && blocks[i].row0 == slot + p && blocks[i].e0 == entry);
        CHECK(blocks[i].count == (p + 1 < pieces ? PK_BLOCK : len - p * PK_BLOCK));
        entry += blocks[i].count;
      }
      slot += pieces; ++row; ++li;
    }
  }
  CHECK(row == A.rows && entry == A.nnz() && li == longs.size() && slot == n_slots);
}

// y = A v, with an addend, and with the addend aliasing y, against the plain loop
static void check_products(int op, const Csr& A, const std::vector<double>& vals) {
  std::vector<double> v((size_t)A.cols), add((size_t)A.rows), y((size_t)A.rows, -77.0);
  for (int32_t j = 0; j < A.cols; ++j) v[(size_t)j] = small_vec(j + op);
  for (int32_t r = 0; r < A.rows; ++r) add[(size_t)r] = small_vec(3 * r + 1);
  OK(pk_apply_operator_dev(ctx, op, vals.data(), v.data(), nullptr, y.data(), nullptr));
  OK(pk_sync(ctx, nullptr));
  CHECK(y == reference(A, vals, v, nullptr));
  OK(pk_apply_operator_dev(ctx, op, vals.data(), v.data(), add.data(), y.data(), nullptr));
  OK(pk_sync(ctx, nullptr));
  const std::vector<double> want = reference(A, vals, v, add.data());
  CHECK(y == want);
  y = add;
  OK(pk_apply_operator_dev(ctx, op, vals.data(), v.data(), y.data(), y.data(), nullptr));      // add aliases y
  OK(pk_sync(ctx, nullptr));
  CHECK(y == want);
}

// one synthetic J (rows of the given lengths): its row blocks, J v with src NULL, J^T y with src, both grids' strides
static void jacobian_case(const std::vector<int32_t>& lens, int32_t cols) {
  const Csr A = from_lengths(lens, cols), T = transposed(A);
  check_blocks(A);
  check_blocks(T);
  set_problem(cols, A.rows, A.nnz(), 5);
  set_identity_map(0, A.nnz());
  OK(set_operator(0, A));
  OK(set_operator(1, T));
  std::vector<double> vals((size_t)A.nnz());
  for (int64_t e = 0; e < A.nnz(); ++e) vals[(size_t)e] = small_val(e);
  check_products(0, A, vals);
  check_products(1, T, vals);
}

int main() {
  load_model();

  // ---- the row lengths at which the walk changes, mixed; 600 consecutive empty rows; a long row first and last
  jacobian_case({0, 1, 255, 256, 257, 512, 513, 0, 3, 1, 0}, 600);
  {
    std::vector<int32_t> lens = {700, 2, 3};
    lens.insert(lens.end(), 600, 0);
    lens.insert(lens.end(), {4, 0, 0, 5, 300});
    jacobian_case(lens, 701);
  }
  jacobian_case({257, 600, 256 * 3, 1000}, 1000);                  // only long rows
  jacobian_case(std::vector<int32_t>(1000, 3), 40);                // many short rows: blocks bounded by entries; a dense transpose
  jacobian_case(std::vector<int32_t>(2100, 200), 256);             // one row per block: more blocks than the grid cap, the stride loop
  {
    // ---- 65 537 entries in one row: 257 pieces, more than one round of pk_op_long's loop
    std::vector<int32_t> lens(3000, 2);
    lens[17] = 65537;
    lens[2999] = 256;
    jacobian_case(lens, 65600);
  }

  // ---- H symmetric from its lower triangle: diagonal, a sub-diagonal band and a dense last row (the row of t_f)
  {
    const int32_t n = 2000;
    Csr L;
    L.rows = L.cols = n;
    L.indptr.push_back(0);
    for (int32_t r = 0; r < n; ++r) {
      if (r == n - 1) {
        for (int32_t c = 0; c < n; ++c) L.indices.push_back(c);
      } else if (r % 5 != 4) {                     // (every fifth row is empty in L)
        if (r >= 2) L.indices.push_back(r - 2);
        L.indices.push_back(r);
      }
      L.indptr.push_back((int32_t)L.indices.size());
    }
    const Csr S = symmetric(L);
    check_blocks(S);
    set_problem(n, 7, 11, L.nnz());
    CHECK(set_operator(2, S) == 111);              // operator before its map
    set_identity_map(1, L.nnz());
    OK(set_operator(2, S));
    std::vector<double> vals((size_t)L.nnz());
    for (int64_t e = 0; e < L.nnz(); ++e) vals[(size_t)e] = small_val(e + 5);
    check_products(2, S, vals);
    CHECK(pk_apply_operator_dev(ctx, 0, vals.data(), vals.data(), nullptr, vals.data(), nullptr) == 117);      // J was never set here

    // ---- the host form: pk_linearize downloads nothing, pk_apply_operator multiplies with what it left
    std::vector<double> x((size_t)n), lam(7), v((size_t)n), y((size_t)n, -3.0);
    for (int32_t i = 0; i < n; ++i) { x[(size_t)i] = 2.0 * (double)(i % 9 - 4); v[(size_t)i] = small_vec(i); }
    for (int j = 0; j < 7; ++j) lam[(size_t)j] = (double)(j - 3);
    CHECK(pk_apply_operator(ctx, 2, v.data(), y.data()) == 118);      // apply before linearize
    CHECK(pk_linearize(ctx, x.data(), nullptr, 1.0) == 111);          // J's map is missing
    set_identity_map(0, 11);                                           // (drops the operators: their src refers to a map)
    CHECK(pk_apply_operator_dev(ctx, 2, vals.data(), v.data(), nullptr, y.data(), nullptr) == 117);
    OK(set_operator(2, S));
    size_t mark = fake_hip_log().size();
    OK(pk_linearize(ctx, x.data(), nullptr, 1.0));
    for (size_t i = mark; i < fake_hip_log().size(); ++i) CHECK(fake_hip_log()[i] != "d2h");
    CHECK(pk_apply_operator(ctx, 2, v.data(), y.data()) == 118);      // a linearization without H
    mark = fake_hip_log().size();
    OK(pk_linearize(ctx, x.data(), lam.data(), 2.0));
    for (size_t i = mark; i < fake_hip_log().size(); ++i) CHECK(fake_hip_log()[i] != "d2h");
    OK(pk_apply_operator(ctx, 2, v.data(), y.data()));
    for (int64_t e = 0; e < L.nnz(); ++e) vals[(size_t)e] = fake_hess(x.data(), lam.data(), 2.0, n, 7, e);
    CHECK(y == reference(S, vals, v, nullptr));
    std::vector<double> hvals((size_t)L.nnz());
    OK(pk_eval_hess_csr(ctx, x.data(), lam.data(), 2.0, hvals.data()));      // the value arrays now hold another evaluation
    CHECK(pk_apply_operator(ctx, 2, v.data(), y.data()) == 118);
  }

  // ---- J through the host form, and every refusal: its code, nothing enqueued, nothing written
  {
    const Csr A = from_lengths({3, 0, 300, 2}, 400), T = transposed(A);
    set_problem(400, 4, A.nnz(), 9);
    CHECK(set_operator(0, A) == 111);                                  // pk_set_problem dropped the maps
    set_identity_map(0, A.nnz());
    OK(set_operator(0, A));
    OK(set_operator(1, T));
    std::vector<double> x(400), v(400), y(4, -5.0), u(4), z(400, -5.0), vals((size_t)A.nnz());
    for (int i = 0; i < 400; ++i) { x[(size_t)i] = 2.0 * (double)(i % 7 - 3); v[(size_t)i] = small_vec(i); }
    for (int j = 0; j < 4; ++j) u[(size_t)j] = (double)(j - 2);
    CHECK(pk_apply_operator(ctx, 0, v.data(), y.data()) == 118);
    OK(pk_linearize(ctx, x.data(), nullptr, 1.0));
    OK(pk_apply_operator(ctx, 0, v.data(), y.data()));
    OK(pk_apply_operator(ctx, 1, u.data(), z.data()));
    for (int64_t e = 0; e < A.nnz(); ++e) vals[(size_t)e] = fake_jac(x.data(), 400, e, false);
    CHECK(y == reference(A, vals, v, nullptr));
    CHECK(z == reference(T, vals, u, nullptr));
    CHECK(pk_apply_operator(ctx, 2, v.data(), z.data()) == 117);

    const size_t mark = fake_hip_log().size();
    const std::vector<double> y0 = y;
    Csr B = A;
    B.indices[5] = 400;
    CHECK(set_operator(0, B) == 114);                                  // index out of range
    B = A; B.indices[0] = -1;
    CHECK(set_operator(0, B) == 114);
    B = A; B.indptr[2] = 1;
    CHECK(set_operator(0, B) == 113);                                  // non-monotone indptr
    B = A; B.indptr[4] -= 1;
    CHECK(set_operator(0, B) == 113);                                  // ... or one that does not cover the entries
    B = T; B.src[7] = (int32_t)A.nnz();
    CHECK(set_operator(1, B) == 115);                                  // src out of range
    B = T; B.src[0] = -1;
    CHECK(set_operator(1, B) == 115);
    CHECK(set_operator(0, T) == 112 && set_operator(1, A) == 112);     // the shape of the other operator
    CHECK(pk_set_csr_operator(ctx, 0, A.indptr.data(), A.indices.data(), nullptr, A.rows, A.cols, A.nnz() - 1) == 112);
    CHECK(set_operator(3, A) == 110 && set_operator(-1, A) == 110);
    CHECK(pk_set_csr_operator(ctx, 0, nullptr, A.indices.data(), nullptr, A.rows, A.cols, A.nnz()) == 110);
    CHECK(pk_apply_operator_dev(ctx, 0, vals.data(), nullptr, nullptr, y.data(), nullptr) == 110);
    CHECK(pk_apply_operator_dev(ctx, 5, vals.data(), v.data(), nullptr, y.data(), nullptr) == 110);
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark && y == y0);
    // (a refused structure leaves the operator that was there in place)
    OK(pk_apply_operator(ctx, 0, v.data(), y.data()));
    CHECK(y == y0);

    set_identity_map(0, A.nnz());                                      // a new map drops the operators and the linearization
    CHECK(pk_apply_operator(ctx, 0, v.data(), y.data()) == 117);
    OK(set_operator(0, A));
    CHECK(pk_apply_operator(ctx, 0, v.data(), y.data()) == 118);
    OK(pk_linearize(ctx, x.data(), nullptr, 1.0));
    OK(pk_apply_operator(ctx, 0, v.data(), y.data()));
    CHECK(y == y0);
    set_problem(400, 4, A.nnz(), 9);                                   // a new problem drops everything
    CHECK(pk_apply_operator_dev(ctx, 0, vals.data(), v.data(), nullptr, y.data(), nullptr) == 117);
    CHECK(pk_apply_operator(ctx, 0, v.data(), y.data()) == 117);
    set_identity_map(0, A.nnz());
    OK(set_operator(0, A));
    OK(set_operator(1, T));
  }
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return checks_passed();
}
