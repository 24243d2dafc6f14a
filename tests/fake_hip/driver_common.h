// driver_common.h -- TEST INFRASTRUCTURE: what the driver programs of this directory share (header-only; every driver is a
// program of its own, so everything here is inline).  The counted checks, the context, the smallest problem the runtime
// accepts, synthetic CSR structures of small integers for the drivers of the operators, and for the drivers of the units built on
// them (reductions, CG, MINRES): results between sentinels, vectors of small integers, plain-loop products, the reader of --dump.
#ifndef FAKE_HIP_DRIVER_COMMON_H
#define FAKE_HIP_DRIVER_COMMON_H

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/pockit_hip.h"
#include "../../pockit_amd/csrc/pockit_hip_internal.h"
#include "../../pockit_amd/csrc/pk_abi.h"
#include "fake_hip.h"

inline int g_checks = 0;
inline pk_ctx* ctx = nullptr;

// A driver may define CHECK_CONTEXT() before it includes this header: what it prints behind the line of a failed check.
#ifndef CHECK_CONTEXT
#define CHECK_CONTEXT() ((void)0)
#endif
#define CHECK(cond)                                                                                              \
  do {                                                                                                           \
    ++g_checks;                                                                                                  \
    if (!(cond)) {                                                                                               \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s (%s)\n", __FILE__, __LINE__, #cond, pk_last_error(ctx));     \
      CHECK_CONTEXT();                                                                                           \
      std::exit(1);                                                                                              \
    }                                                                                                            \
  } while (0)
#define OK(call) CHECK((call) == 0)

// the last line of a driver that got this far
inline int checks_passed() {
  std::printf("%d checks passed\n", g_checks);
  return 0;
}

// ---------------------------------------------------------------- the smallest problem: one phase, two blocks of empty tiles
inline const char image[16] = "fake code";
inline PkPhase g_phase{};
inline PkTile g_tiles[2 * PK_WAVES_PER_BLOCK] = {};
inline const double SENTINEL = -77.5;

inline void set_problem(int32_t n, int32_t m, int64_t nnz_J, int64_t nnz_H) {
  FakeSizes S;
  S.n = n; S.m = m; S.nnz_J = nnz_J; S.nnz_H = nnz_H;
  fake_hip_set_sizes(S);
  for (auto& t : g_tiles) t.K = 1;
  g_phase.tile_hi = 2 * PK_WAVES_PER_BLOCK;
  pk_problem_desc pd{};
  pd.n = n; pd.m = m; pd.n_phase = 1; pd.nnz_J = nnz_J; pd.nnz_H = nnz_H;
  pd.phases = &g_phase; pd.tiles = g_tiles; pd.n_tiles = 2 * PK_WAVES_PER_BLOCK;
  OK(pk_set_problem(ctx, &pd));
}

inline void set_identity_map(int which, int64_t count) {
  std::vector<int32_t> perm((size_t)count);
  for (int64_t q = 0; q < count; ++q) perm[(size_t)q] = (int32_t)q;
  OK(pk_set_csr_map(ctx, which, nullptr, perm.data(), count, count));
}

// ---------------------------------------------------------------- CSR structures for the operator drivers
struct Csr {
  int32_t rows = 0, cols = 0;
  std::vector<int32_t> indptr, indices, src;      // src empty: the identity
  int64_t nnz() const { return (int64_t)indices.size(); }
  const int32_t* srcp() const { return src.empty() ? nullptr : src.data(); }
};

// rows of the given lengths, columns ascending and distinct within a row
inline Csr from_lengths(const std::vector<int32_t>& lens, int32_t cols) {
  Csr A;
  A.rows = (int32_t)lens.size(); A.cols = cols;
  A.indptr.push_back(0);
  for (int32_t r = 0; r < A.rows; ++r) {
    const int32_t L = lens[(size_t)r], off = L < cols ? (r * 7) % (cols - L + 1) : 0;
    if (L > cols) std::exit(2);
    for (int32_t k = 0; k < L; ++k) A.indices.push_back(off + k);
    A.indptr.push_back((int32_t)A.indices.size());
  }
  return A;
}

// CSR of the transpose, src pointing into A's values (what pockit_amd/csr.py's CsrMap.transposed builds)
inline Csr transposed(const Csr& A) {
  Csr T;
  T.rows = A.cols; T.cols = A.rows;
  T.indptr.assign((size_t)T.rows + 1, 0);
  for (int32_t j : A.indices) ++T.indptr[(size_t)j + 1];
  for (int32_t j = 0; j < T.rows; ++j) T.indptr[(size_t)j + 1] += T.indptr[(size_t)j];
  T.indices.resize(A.indices.size()); T.src.resize(A.indices.size());
  std::vector<int32_t> at(T.indptr.begin(), T.indptr.end() - 1);
  for (int32_t r = 0; r < A.rows; ++r)
    for (int32_t e = A.indptr[(size_t)r]; e < A.indptr[(size_t)r + 1]; ++e) {
      const int32_t q = at[(size_t)A.indices[(size_t)e]]++;
      T.indices[(size_t)q] = r; T.src[(size_t)q] = e;
    }
  return T;
}

inline int set_operator(int op, const Csr& A) {
  return pk_set_csr_operator(ctx, op, A.indptr.data(), A.indices.data(), A.srcp(), A.rows, A.cols, A.nnz());
}

inline double small_val(int64_t e) { return (double)((e * 31) % 17 - 8); }
inline double small_vec(int64_t j) { return (double)((j * 13) % 11 - 5); }

// ---------------------------------------------------------------- vectors between sentinels, small integers, exact comparisons
typedef std::vector<double> Vec;
inline const int PAD = 5;

// a result between sentinels: what was written, nothing beside it
struct Guarded {
  Vec buf;
  size_t count;
  explicit Guarded(size_t n, double fill = -77.0) : buf(n + 2 * PAD, fill), count(n) {
    for (int i = 0; i < PAD; ++i) buf[(size_t)i] = buf[n + PAD + (size_t)i] = SENTINEL;
  }
  explicit Guarded(const Vec& v) : Guarded(v.size()) { std::copy(v.begin(), v.end(), buf.begin() + PAD); }
  double* ptr() { return buf.data() + PAD; }
  Vec fetch() const {
    for (int i = 0; i < PAD; ++i) CHECK(buf[(size_t)i] == SENTINEL && buf[count + PAD + (size_t)i] == SENTINEL);
    return Vec(buf.begin() + PAD, buf.begin() + PAD + (long)count);
  }
};

// n doubles whose data() is never NULL (a length of 0 is a valid step; a null pointer is refused)
inline Vec made(size_t n) {
  Vec v;
  v.reserve(n + 1);
  v.resize(n);
  return v;
}

inline Vec ints(size_t n, int64_t salt, bool positive = false) {
  Vec v = made(n);
  for (size_t i = 0; i < n; ++i) v[i] = positive ? (double)(((int64_t)i * 7 + salt) % 4 + 1) : small_vec((int64_t)i * 3 + salt);
  return v;
}

inline double dotp(const Vec& a, const Vec& b) {
  double s = 0.0;
  for (size_t i = 0; i < a.size(); ++i) s += a[i] * b[i];
  return s;
}

inline bool same_bits(const Vec& a, const Vec& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), 8 * a.size()) == 0; }

// L + L^T - diag(L) of a lower-triangular L, each off-diagonal entry twice with one src (CsrMap.symmetric)
inline Csr symmetric(const Csr& L) {
  struct E { int32_t c, s; };
  std::vector<std::vector<E>> mirrored((size_t)L.rows);
  for (int32_t r = 0; r < L.rows; ++r)
    for (int32_t e = L.indptr[(size_t)r]; e < L.indptr[(size_t)r + 1]; ++e) {
      const int32_t c = L.indices[(size_t)e];
      if (c > r) std::exit(2);
      if (c < r) mirrored[(size_t)c].push_back({r, e});      // rows ascend, so the mirrored entries of a row arrive in column order
    }
  Csr S;
  S.rows = S.cols = L.rows;
  S.indptr.push_back(0);
  for (int32_t r = 0; r < L.rows; ++r) {
    for (int32_t e = L.indptr[(size_t)r]; e < L.indptr[(size_t)r + 1]; ++e) { S.indices.push_back(L.indices[(size_t)e]); S.src.push_back(e); }
    for (const E& m : mirrored[(size_t)r]) { S.indices.push_back(m.c); S.src.push_back(m.s); }
    S.indptr.push_back((int32_t)S.indices.size());
  }
  return S;
}

inline Vec matvec(const Csr& A, const Vec& vals, const double* v) {
  Vec y((size_t)A.rows, 0.0);
  for (int32_t r = 0; r < A.rows; ++r)
    for (int32_t e = A.indptr[(size_t)r]; e < A.indptr[(size_t)r + 1]; ++e)
      y[(size_t)r] += vals[(size_t)(A.src.empty() ? e : A.src[(size_t)e])] * v[(size_t)A.indices[(size_t)e]];
  return y;
}

// the context with the smallest model the runtime accepts
inline void load_model() {
  OK(pk_create(&ctx, 0));
  pk_model_desc md{};
  md.n_phase = 1; md.n_I = 1; md.nred = 1; md.lds_g = md.lds_j = md.lds_h = md.lds_x = md.lds_e = md.lds_jc = 64;
  md.ne_j = md.ne_h = md.ne_a = 1; md.tab_cap = 64;
  OK(pk_load_model(ctx, image, sizeof image, &md));
}

// ---------------------------------------------------------------- --dump: reading the solve a file describes
inline std::vector<int32_t> read_ints(FILE* f) {
  size_t n = 0;
  if (std::fscanf(f, "%zu", &n) != 1) std::exit(3);
  std::vector<int32_t> v(n);
  for (auto& e : v) if (std::fscanf(f, "%d", &e) != 1) std::exit(3);
  return v;
}
inline Vec read_doubles(FILE* f) {
  size_t n = 0;
  if (std::fscanf(f, "%zu", &n) != 1) std::exit(3);
  Vec v(n);
  for (auto& e : v) if (std::fscanf(f, "%la", &e) != 1) std::exit(3);
  return v;
}
inline Csr read_csr(FILE* f, int32_t cols) {
  Csr A;
  A.indptr = read_ints(f); A.indices = read_ints(f); A.src = read_ints(f);
  A.rows = (int32_t)A.indptr.size() - 1; A.cols = cols;
  return A;
}

#endif  // FAKE_HIP_DRIVER_COMMON_H
