// reduce_driver.cpp -- TEST INFRASTRUCTURE: drives the reductions over an operator's rows and the diagonal of H
// (pockit_amd/csrc/pk_reduce.cpp) against the host-only HIP stand-in of this directory, built with -fsanitize=address,undefined
// (tests/test_operator_reduce_cpu.py): the host walk of pk_red_rows / pk_red_long / pk_diag over the block tables the kernels
// read, on synthetic matrices of small integers (every term and every sum is exact in fp64, so a result must EQUAL a plain loop
// over the entries), the refusals with their codes, what drops the positions of the diagonal, tear-down without a live allocation.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "driver_common.h"

// the reference: a plain loop over rows and entries; w and add may be NULL
static std::vector<double> reference(const Csr& A, int mode, const std::vector<double>& vals, const double* w, const double* add) {
  std::vector<double> y((size_t)A.rows);
  for (int32_t r = 0; r < A.rows; ++r) {
    double acc = 0.0;
    for (int32_t e = A.indptr[(size_t)r]; e < A.indptr[(size_t)r + 1]; ++e) {
      const double a = vals[(size_t)(A.src.empty() ? e : A.src[(size_t)e])];
      double t = mode == 1 ? a * a : std::fabs(a);
      if (w) t = t * w[A.indices[(size_t)e]];
      if (mode == 2) { if (t > acc) acc = t; } else acc += t;
    }
    if (add) { if (mode == 2) { if (add[r] > acc) acc = add[r]; } else acc += add[r]; }
    y[(size_t)r] = acc;
  }
  return y;
}

static void check_nonnegative(const std::vector<double>& y) {
  for (double v : y) CHECK(v >= 0.0 && !std::signbit(v));
}

// the three modes of one operator: w given and NULL; add NULL, given and aliasing y
static void check_reductions(int op, const Csr& A, const std::vector<double>& vals) {
  std::vector<double> w((size_t)A.cols), add((size_t)A.rows);
  for (int32_t j = 0; j < A.cols; ++j) w[(size_t)j] = small_vec(j + op);             // (negative and zero weights among them)
  for (int32_t r = 0; r < A.rows; ++r) add[(size_t)r] = 40.0 * small_vec(3 * r + 1);
  for (int mode = 0; mode < 3; ++mode)
    for (const double* wp : {(const double*)w.data(), (const double*)nullptr}) {
      Guarded plain((size_t)A.rows), added((size_t)A.rows), alias((size_t)A.rows);
      OK(pk_operator_reduce_dev(ctx, op, mode, vals.data(), wp, nullptr, plain.ptr(), nullptr));
      OK(pk_operator_reduce_dev(ctx, op, mode, vals.data(), wp, add.data(), added.ptr(), nullptr));
      for (int32_t r = 0; r < A.rows; ++r) alias.ptr()[r] = add[(size_t)r];
      OK(pk_operator_reduce_dev(ctx, op, mode, vals.data(), wp, alias.ptr(), alias.ptr(), nullptr));      // add aliases y
      OK(pk_sync(ctx, nullptr));
      const std::vector<double> want = reference(A, mode, vals, wp, add.data());
      CHECK(plain.fetch() == reference(A, mode, vals, wp, nullptr));
      CHECK(added.fetch() == want);
      CHECK(alias.fetch() == want);
      if (mode == 2) { check_nonnegative(plain.fetch()); check_nonnegative(added.fetch()); }
    }
}

// one synthetic J (rows of the given lengths): J with src NULL, J^T with src
static void jacobian_case(const std::vector<int32_t>& lens, int32_t cols) {
  const Csr A = from_lengths(lens, cols), T = transposed(A);
  set_problem(cols, A.rows, A.nnz(), 5);
  set_identity_map(0, A.nnz());
  OK(set_operator(0, A));
  OK(set_operator(1, T));
  std::vector<double> vals((size_t)A.nnz());
  for (int64_t e = 0; e < A.nnz(); ++e) vals[(size_t)e] = small_val(e);
  check_reductions(0, A, vals);
  check_reductions(1, T, vals);
}

// CsrMap.diagonal_src: the last entry of a row whose column equals the row, -1 where there is none
static std::vector<int32_t> diagonal_src(const Csr& L) {
  std::vector<int32_t> pos((size_t)L.rows, -1);
  for (int32_t r = 0; r < L.rows; ++r) {
    const int32_t last = L.indptr[(size_t)r + 1] - 1;
    if (last >= L.indptr[(size_t)r] && L.indices[(size_t)last] == r) pos[(size_t)r] = last;
  }
  return pos;
}

static std::vector<double> diagonal(const std::vector<int32_t>& pos, const std::vector<double>& vals, const double* add) {
  std::vector<double> y(pos.size());
  for (size_t i = 0; i < pos.size(); ++i) y[i] = (pos[i] >= 0 ? vals[(size_t)pos[i]] : 0.0) + (add ? add[i] : 0.0);
  return y;
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
  jacobian_case(std::vector<int32_t>(2100, 200), 256);             // one row per block: more blocks than the grid cap, the stride loop
  jacobian_case(std::vector<int32_t>(2100, 257), 300);             // ... and more long rows than the cap
  {
    // ---- 65 537 entries in one row: 257 pieces, more than one round of pk_red_long's strided loop
    std::vector<int32_t> lens(3000, 2);
    lens[17] = 65537;
    lens[2999] = 256;
    jacobian_case(lens, 65600);
  }

  // ---- H symmetric from its lower triangle: diagonal, a sub-diagonal band, empty rows and a dense last row; its diagonal
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
        if (r % 7 != 3) L.indices.push_back(r);    // (... and some rows have no diagonal entry)
      }
      L.indptr.push_back((int32_t)L.indices.size());
    }
    const Csr S = symmetric(L);
    std::vector<int32_t> pos = diagonal_src(L);
    CHECK(pos[0] == 0 && pos[3] == -1 && pos[4] == -1 && pos[(size_t)n - 1] == (int32_t)L.nnz() - 1);
    set_problem(n, 7, 11, L.nnz());
    CHECK(pk_set_operator_diagonal(ctx, 2, pos.data(), n) == 111);              // positions before their map
    set_identity_map(1, L.nnz());
    OK(set_operator(2, S));
    std::vector<double> vals((size_t)L.nnz()), add((size_t)n);
    for (int64_t e = 0; e < L.nnz(); ++e) vals[(size_t)e] = small_val(e + 5);
    for (int32_t i = 0; i < n; ++i) add[(size_t)i] = small_vec(i + 2);
    check_reductions(2, S, vals);

    Guarded y((size_t)n);
    size_t mark = fake_hip_log().size();
    CHECK(pk_operator_diagonal_dev(ctx, 2, vals.data(), nullptr, y.ptr(), nullptr) == 132);      // before pk_set_operator_diagonal
    // ---- pos rejected: a wrong length, -2, n_unique; a refused pos leaves none behind
    CHECK(pk_set_operator_diagonal(ctx, 2, pos.data(), n - 1) == 131);
    std::vector<int32_t> bad = pos;
    bad[10] = -2;
    CHECK(pk_set_operator_diagonal(ctx, 2, bad.data(), n) == 131);
    bad = pos; bad[(size_t)n - 1] = (int32_t)L.nnz();
    CHECK(pk_set_operator_diagonal(ctx, 2, bad.data(), n) == 131);
    CHECK(pk_set_operator_diagonal(ctx, 0, pos.data(), n) == 130 && pk_set_operator_diagonal(ctx, 1, pos.data(), n) == 130);
    CHECK(pk_set_operator_diagonal(ctx, 3, pos.data(), n) == 110 && pk_set_operator_diagonal(ctx, 2, nullptr, n) == 110);
    CHECK(pk_operator_diagonal_dev(ctx, 2, vals.data(), nullptr, y.ptr(), nullptr) == 132);
    OK(pk_set_shard(ctx, 1, 0, nullptr));                                         // a shard is refused the positions
    CHECK(pk_set_operator_diagonal(ctx, 2, pos.data(), n) == 119);
    OK(pk_set_shard(ctx, 0, 0, nullptr));
    CHECK(pk_operator_diagonal_dev(ctx, 2, vals.data(), nullptr, y.ptr(), nullptr) == 132);
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark);
    for (double v : y.fetch()) CHECK(v == -77.0);

    OK(pk_set_operator_diagonal(ctx, 2, pos.data(), n));
    Guarded plain((size_t)n), added((size_t)n), alias((size_t)n);
    OK(pk_operator_diagonal_dev(ctx, 2, vals.data(), nullptr, plain.ptr(), nullptr));
    OK(pk_operator_diagonal_dev(ctx, 2, vals.data(), add.data(), added.ptr(), nullptr));
    for (int32_t i = 0; i < n; ++i) alias.ptr()[i] = add[(size_t)i];
    OK(pk_operator_diagonal_dev(ctx, 2, vals.data(), alias.ptr(), alias.ptr(), nullptr));
    OK(pk_sync(ctx, nullptr));
    CHECK(plain.fetch() == diagonal(pos, vals, nullptr));
    CHECK(added.fetch() == diagonal(pos, vals, add.data()) && alias.fetch() == added.fetch());
    OK(pk_set_operator_diagonal(ctx, 2, pos.data(), n));                          // a second upload replaces the first

    // ---- refusals of the device forms: the code, nothing enqueued, nothing written
    mark = fake_hip_log().size();
    Guarded z((size_t)n);
    CHECK(pk_operator_reduce_dev(ctx, 3, 0, vals.data(), nullptr, nullptr, z.ptr(), nullptr) == 110);
    CHECK(pk_operator_reduce_dev(ctx, -1, 0, vals.data(), nullptr, nullptr, z.ptr(), nullptr) == 110);
    CHECK(pk_operator_reduce_dev(ctx, 0, 0, vals.data(), nullptr, nullptr, z.ptr(), nullptr) == 117);      // J was never set here
    CHECK(pk_operator_reduce_dev(ctx, 2, 0, nullptr, nullptr, nullptr, z.ptr(), nullptr) == 110);
    CHECK(pk_operator_reduce_dev(ctx, 2, 0, vals.data(), nullptr, nullptr, nullptr, nullptr) == 110);
    CHECK(pk_operator_reduce_dev(ctx, 2, 3, vals.data(), nullptr, nullptr, z.ptr(), nullptr) == 129);
    CHECK(pk_operator_reduce_dev(ctx, 2, -1, vals.data(), nullptr, nullptr, z.ptr(), nullptr) == 129);
    CHECK(pk_operator_diagonal_dev(ctx, 0, vals.data(), nullptr, z.ptr(), nullptr) == 130);
    CHECK(pk_operator_diagonal_dev(ctx, 1, vals.data(), nullptr, z.ptr(), nullptr) == 130);
    CHECK(pk_operator_diagonal_dev(ctx, 7, vals.data(), nullptr, z.ptr(), nullptr) == 110);
    CHECK(pk_operator_diagonal_dev(ctx, 2, nullptr, nullptr, z.ptr(), nullptr) == 110);
    CHECK(pk_operator_diagonal_dev(ctx, 2, vals.data(), nullptr, nullptr, nullptr) == 110);
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark);
    for (double v : z.fetch()) CHECK(v == -77.0);

    // ---- the host forms against the context's linearization
    std::vector<double> x((size_t)n), lam(7), w((size_t)n), h((size_t)n, -3.0), hd((size_t)n, -3.0);
    for (int32_t i = 0; i < n; ++i) { x[(size_t)i] = 2.0 * (double)(i % 9 - 4); w[(size_t)i] = small_vec(i) + 6.0; }
    for (int j = 0; j < 7; ++j) lam[(size_t)j] = (double)(j - 3);
    mark = fake_hip_log().size();
    CHECK(pk_operator_reduce(ctx, 2, 0, nullptr, 0, h.data()) == 118);           // before pk_linearize
    CHECK(pk_operator_diagonal(ctx, 2, hd.data()) == 118);
    CHECK(pk_operator_reduce(ctx, 2, 0, nullptr, 0, nullptr) == 60);
    CHECK(fake_hip_log().size() == mark);
    set_identity_map(0, 11);                                                      // (drops the operators and the positions)
    CHECK(pk_operator_diagonal_dev(ctx, 2, vals.data(), nullptr, z.ptr(), nullptr) == 132);
    CHECK(pk_operator_reduce_dev(ctx, 2, 0, vals.data(), nullptr, nullptr, z.ptr(), nullptr) == 117);
    OK(set_operator(2, S));
    OK(pk_set_operator_diagonal(ctx, 2, pos.data(), n));
    OK(pk_linearize(ctx, x.data(), nullptr, 1.0));
    mark = fake_hip_log().size();
    CHECK(pk_operator_reduce(ctx, 2, 1, w.data(), 0, h.data()) == 118);           // a linearization without H
    CHECK(pk_operator_diagonal(ctx, 2, hd.data()) == 118);
    CHECK(fake_hip_log().size() == mark);
    OK(pk_linearize(ctx, x.data(), lam.data(), 2.0));
    for (int64_t e = 0; e < L.nnz(); ++e) vals[(size_t)e] = fake_hess(x.data(), lam.data(), 2.0, n, 7, e);
    for (int mode = 0; mode < 3; ++mode) {
      OK(pk_operator_reduce(ctx, 2, mode, w.data(), 0, h.data()));
      CHECK(h == reference(S, mode, vals, w.data(), nullptr));
      OK(pk_operator_reduce(ctx, 2, mode, nullptr, 0, h.data()));
      CHECK(h == reference(S, mode, vals, nullptr, nullptr));
    }
    OK(pk_operator_diagonal(ctx, 2, hd.data()));
    CHECK(hd == diagonal(pos, vals, nullptr));
    OK(pk_operator_reduce(ctx, 2, 1, w.data(), 1, h.data()));                     // diag(H) under the sums, one round trip
    CHECK(h == reference(S, 1, vals, w.data(), hd.data()));
    mark = fake_hip_log().size();
    CHECK(pk_operator_reduce(ctx, 2, 4, w.data(), 0, h.data()) == 129);
    CHECK(pk_operator_reduce(ctx, 0, 1, w.data(), 0, h.data()) == 117);
    CHECK(pk_operator_diagonal(ctx, 1, hd.data()) == 130);
    CHECK(fake_hip_log().size() == mark);
    std::vector<double> hvals((size_t)L.nnz());
    OK(pk_eval_hess_csr(ctx, x.data(), lam.data(), 2.0, hvals.data()));           // the value arrays now hold another evaluation
    CHECK(pk_operator_reduce(ctx, 2, 0, nullptr, 0, h.data()) == 118 && pk_operator_diagonal(ctx, 2, hd.data()) == 118);
  }

  // ---- J and J^T through the host form; diag(H + J^T D J); what drops the positions
  {
    const Csr A = from_lengths({3, 0, 300, 2}, 400), T = transposed(A);
    Csr L;                                                                         // H: a diagonal without its rows 5 k
    L.rows = L.cols = 400;
    L.indptr.push_back(0);
    for (int32_t r = 0; r < 400; ++r) {
      if (r % 5) L.indices.push_back(r);
      L.indptr.push_back((int32_t)L.indices.size());
    }
    const Csr S = symmetric(L);
    const std::vector<int32_t> pos = diagonal_src(L);
    set_problem(400, 4, A.nnz(), L.nnz());
    CHECK(pk_set_operator_diagonal(ctx, 2, pos.data(), 400) == 111);               // pk_set_problem dropped the maps
    set_identity_map(0, A.nnz());
    set_identity_map(1, L.nnz());
    OK(set_operator(0, A));
    OK(set_operator(1, T));
    std::vector<double> x(400), lam(4), d(4), dn(400), y(4, -5.0), z(400, -5.0), hd(400), jv((size_t)A.nnz()), hv((size_t)L.nnz());
    for (int i = 0; i < 400; ++i) { x[(size_t)i] = 2.0 * (double)(i % 7 - 3); dn[(size_t)i] = small_vec(i) + 6.0; }
    for (int j = 0; j < 4; ++j) { lam[(size_t)j] = (double)(j - 2); d[(size_t)j] = (double)(j + 1); }
    OK(pk_linearize(ctx, x.data(), lam.data(), 1.0));
    for (int64_t e = 0; e < A.nnz(); ++e) jv[(size_t)e] = fake_jac(x.data(), 400, e, false);
    for (int64_t e = 0; e < L.nnz(); ++e) hv[(size_t)e] = fake_hess(x.data(), lam.data(), 1.0, 400, 4, e);
    for (int mode = 0; mode < 3; ++mode) {
      OK(pk_operator_reduce(ctx, 0, mode, dn.data(), 0, y.data()));
      CHECK(y == reference(A, mode, jv, dn.data(), nullptr));
      OK(pk_operator_reduce(ctx, 1, mode, d.data(), 0, z.data()));
      CHECK(z == reference(T, mode, jv, d.data(), nullptr));
    }
    size_t mark = fake_hip_log().size();
    CHECK(pk_operator_reduce(ctx, 1, 1, d.data(), 1, z.data()) == 132);            // the diagonal was never set
    CHECK(pk_operator_diagonal(ctx, 2, hd.data()) == 132);
    CHECK(fake_hip_log().size() == mark);
    OK(pk_set_operator_diagonal(ctx, 2, pos.data(), 400));                         // (needs the map, not the operator)
    OK(pk_operator_diagonal(ctx, 2, hd.data()));
    CHECK(hd == diagonal(pos, hv, nullptr));
    OK(pk_operator_reduce(ctx, 1, 1, d.data(), 1, z.data()));
    CHECK(z == reference(T, 1, jv, d.data(), hd.data()));
    mark = fake_hip_log().size();
    CHECK(pk_operator_reduce(ctx, 0, 1, dn.data(), 1, y.data()) == 130);           // J's rows are not H's
    CHECK(fake_hip_log().size() == mark);
    OK(set_operator(2, S));                                                        // pk_set_csr_operator leaves the positions alone
    OK(pk_operator_diagonal(ctx, 2, hd.data()));
    CHECK(hd == diagonal(pos, hv, nullptr));

    set_identity_map(1, L.nnz());                                                  // a new map drops the operators and the positions
    CHECK(pk_operator_diagonal_dev(ctx, 2, hv.data(), nullptr, hd.data(), nullptr) == 132);
    CHECK(pk_operator_reduce_dev(ctx, 0, 0, jv.data(), nullptr, nullptr, y.data(), nullptr) == 117);
    OK(pk_set_operator_diagonal(ctx, 2, pos.data(), 400));
    set_problem(400, 4, A.nnz(), L.nnz());                                         // a new problem drops everything
    CHECK(pk_operator_diagonal_dev(ctx, 2, hv.data(), nullptr, hd.data(), nullptr) == 132);
    set_identity_map(1, L.nnz());
    OK(pk_set_operator_diagonal(ctx, 2, pos.data(), 400));                         // ... and pk_destroy frees what is left
  }
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return checks_passed();
}
