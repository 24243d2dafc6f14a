// minres_driver.cpp -- TEST INFRASTRUCTURE: drives the MINRES entry points (pockit_amd/csrc/pk_minres.cpp) against the host-only HIP
// stand-in of this directory, built with -fsanitize=address,undefined (tests/test_minres_cpu.py): the stand-in walk of every vector
// step against plain loops on small integers and powers of two (every product, sum and quotient of the vectors is exact in fp64,
// so a result must EQUAL the loop; the scalar steps against the same formulas in plain C++), the split index at its boundary
// values, one application of K with and without H, s1 and s2 against plain loops, the host form against begin / advance /
// record, every refusal with its code and nothing enqueued behind it, sentinels around x and the record, what frees and forgets
// the state, and tear-down without a live allocation.  With --dump FILE: the solve FILE describes (tests/test_minres_cpu.py
// writes it from tests/minres_cases.py) through begin / advance / record, the record and x printed as hex doubles.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <set>

#include "driver_common.h"

enum { INIT = 0, LANCZOS = 1, ALFA = 2, UPDATE = 3, SOLUTION = 4, DIAG = 5, RECIP = 6 };
enum { STATUS = 0, ITERS, PHIBAR, THR, BETA, OLDB, ALFA_, DBAR, EPSLN, CS, SN, PHI, OLDEPS, DELTA, GAMMA, FRESH };

struct StepArgs {
  const double *b = nullptr, *x0 = nullptr, *minv = nullptr, *s1 = nullptr, *s2 = nullptr;
  double *x = nullptr, *r1 = nullptr, *r2 = nullptr, *y = nullptr, *v = nullptr, *w = nullptr, *w2 = nullptr, *q = nullptr, *rec = nullptr;
  double tol = 0.0;
};
static int step(int which, int64_t len, int64_t split, const StepArgs& a) {
  return pk_minres_step_dev(ctx, which, len, split, a.b, a.x0, a.minv, a.s1, a.s2, a.x, a.r1, a.r2, a.y, a.v, a.w, a.w2, a.q, a.rec, a.tol, nullptr);
}

// scalar step B as the unit's header states it, in plain C++
static Vec reference_b(Vec rec, double bsq) {
  if (rec[STATUS] != 0.0) return rec;
  if (!std::isfinite(bsq)) { rec[STATUS] = 3.0; return rec; }
  if (bsq < 0.0) { rec[STATUS] = 2.0; return rec; }
  const double cs = rec[CS], sn = rec[SN], dbar = rec[DBAR], alfa = rec[ALFA_], phibar = rec[PHIBAR];
  const double beta = std::sqrt(bsq);
  rec[OLDB] = rec[BETA]; rec[BETA] = beta; rec[OLDEPS] = rec[EPSLN];
  const double p0 = cs * dbar, p1 = sn * alfa, p2 = sn * dbar, p3 = cs * alfa, p4 = cs * beta;
  const double gbar = p2 - p3;
  rec[DELTA] = p0 + p1; rec[EPSLN] = sn * beta; rec[DBAR] = -p4;
  const double g0 = gbar * gbar, g1 = beta * beta;
  const double gamma = std::sqrt(g0 + g1);
  rec[GAMMA] = gamma;
  if (!(gamma > 0.0) || !std::isfinite(gamma)) { rec[STATUS] = 3.0; return rec; }
  rec[CS] = gbar / gamma; rec[SN] = beta / gamma; rec[PHI] = rec[CS] * phibar; rec[PHIBAR] = rec[SN] * phibar;
  rec[ITERS] += 1.0; rec[FRESH] = 1.0;
  if (rec[PHIBAR] <= rec[THR]) rec[STATUS] = 1.0;
  return rec;
}

// a running record whose quotients are powers of two: 1 / beta = 2, beta / oldb = 2, alfa / beta = 3, / gamma = * 2
static Vec running(double iterations) {
  Vec rec(16, 0.0);
  rec[ITERS] = iterations; rec[PHIBAR] = 3.0; rec[THR] = 0.125; rec[BETA] = 0.5; rec[OLDB] = 0.25; rec[ALFA_] = 1.5; rec[DBAR] = -2.0;
  rec[EPSLN] = 0.75; rec[CS] = 0.6; rec[SN] = 0.8; rec[PHI] = 2.0; rec[OLDEPS] = 3.0; rec[DELTA] = -2.0; rec[GAMMA] = 0.5;
  return rec;
}

static std::vector<int64_t> splits_of(size_t L) {
  std::set<int64_t> s;
  for (int64_t v : {(int64_t)0, (int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)L - 1, (int64_t)L})
    if (v >= 0 && v <= (int64_t)L) s.insert(v);
  return std::vector<int64_t>(s.begin(), s.end());
}

static Vec diag_reference(const Vec& v, const Vec* s1, const Vec* s2, int64_t split) {
  Vec q = made(v.size());
  for (size_t i = 0; i < v.size(); ++i)
    q[i] = (int64_t)i < split ? (s1 ? (*s1)[i] * v[i] : 0.0) : (s2 ? -((*s2)[i - (size_t)split] * v[i]) : 0.0);
  return q;
}

// every vector step at one length against plain loops
static void check_steps(size_t L) {
  const int64_t N = (int64_t)L;
  const Vec b = ints(L, 1), x0 = ints(L, 2), kx = ints(L, 3), minv = ints(L, 4, true), s1 = ints(L, 5), s2 = ints(L, 6);
  const Vec x = ints(L, 7), r1 = ints(L, 8), r2 = ints(L, 9), y = ints(L, 10), v = ints(L, 11), w = ints(L, 12), w2 = ints(L, 13), q = ints(L, 14);
  for (int variant = 0; variant < 2; ++variant) {      // ---- begin.  0: x0 and minv given; 1: neither
    const bool full = variant == 0;
    Guarded gx(L), g1(L), g2(L), gy(L), gw(L), gw2(L), gq(full ? Guarded(kx) : Guarded(L)), rec(16);
    StepArgs a;
    a.b = b.data(); a.x0 = full ? x0.data() : nullptr; a.minv = full ? minv.data() : nullptr;
    a.x = gx.ptr(); a.r1 = g1.ptr(); a.r2 = g2.ptr(); a.y = gy.ptr(); a.w = gw.ptr(); a.w2 = gw2.ptr(); a.q = gq.ptr(); a.rec = rec.ptr(); a.tol = 0.5;
    OK(step(INIT, N, N / 2, a));
    OK(pk_sync(ctx, nullptr));
    Vec wx = made(L), wr = made(L), wy = made(L), mb = made(L);
    for (size_t i = 0; i < L; ++i) {
      wx[i] = full ? x0[i] : 0.0;
      wr[i] = full ? b[i] - kx[i] : b[i];
      wy[i] = full ? minv[i] * wr[i] : wr[i];
      mb[i] = full ? minv[i] * b[i] : b[i];
    }
    CHECK(gx.fetch() == wx && g1.fetch() == wr && g2.fetch() == wr && gy.fetch() == wy && gw.fetch() == Vec(L, 0.0) && gw2.fetch() == Vec(L, 0.0));
    const double bmb = dotp(b, mb), ry = dotp(wr, wy), thr = 0.5 * std::sqrt(bmb);
    Vec want(16, 0.0);
    want[CS] = -1.0; want[THR] = thr;
    if (ry < 0.0) want[STATUS] = 2.0;
    else {
      want[BETA] = want[PHIBAR] = std::sqrt(ry);
      want[STATUS] = want[BETA] <= thr ? 1.0 : 0.0;
    }
    CHECK(same_bits(rec.fetch(), want));
  }
  for (int64_t split : splits_of(L))      // ---- the Lanczos vector and the diagonal blocks at every split index
    for (int variant = 0; variant < 3; ++variant) {      // 0: s1 and s2; 1: s1 alone; 2: s2 alone
      const Vec* p1 = variant != 2 ? &s1 : nullptr;
      const Vec* p2 = variant != 1 ? &s2 : nullptr;
      for (double status : {0.0, 1.0}) {
        Vec state = running(3.0);
        state[STATUS] = status;
        Guarded gy(y), gv(v), gq(L), rec(state);
        StepArgs a;
        a.s1 = p1 ? p1->data() : nullptr; a.s2 = p2 ? p2->data() : nullptr; a.y = gy.ptr(); a.v = gv.ptr(); a.q = gq.ptr(); a.rec = rec.ptr();
        OK(step(LANCZOS, N, split, a));
        OK(pk_sync(ctx, nullptr));
        Vec wv = made(L);
        for (size_t i = 0; i < L; ++i) wv[i] = status == 0.0 ? 2.0 * y[i] : v[i];
        CHECK(gv.fetch() == wv && gy.fetch() == y && gq.fetch() == diag_reference(wv, p1, p2, split) && same_bits(rec.fetch(), state));
      }
      Guarded gq(L);
      StepArgs a;
      a.b = v.data(); a.s1 = p1 ? p1->data() : nullptr; a.s2 = p2 ? p2->data() : nullptr; a.q = gq.ptr();
      OK(step(DIAG, N, split, a));
      OK(pk_sync(ctx, nullptr));
      CHECK(gq.fetch() == diag_reference(v, p1, p2, split));
    }
  for (double status : {0.0, 2.0}) {      // ---- alfa: fresh is cleared whatever the status
    Vec state = running(3.0);
    state[STATUS] = status; state[FRESH] = 1.0;
    Guarded gv(v), gq(q), rec(state);
    StepArgs a;
    a.v = gv.ptr(); a.q = gq.ptr(); a.rec = rec.ptr();
    OK(step(ALFA, N, 0, a));
    OK(pk_sync(ctx, nullptr));
    state[FRESH] = 0.0;
    if (status == 0.0) state[ALFA_] = dotp(v, q);
    CHECK(same_bits(rec.fetch(), state) && gv.fetch() == v && gq.fetch() == q);
  }
  for (int with_minv = 0; with_minv < 2; ++with_minv)      // ---- update: the first iteration skips the r1 term
    for (double iterations : {0.0, 1.0, 3.0}) {
      const Vec state = running(iterations);
      Guarded g1(r1), g2(r2), gy(y), gq(q), rec(state);
      StepArgs a;
      a.minv = with_minv ? minv.data() : nullptr; a.r1 = g1.ptr(); a.r2 = g2.ptr(); a.y = gy.ptr(); a.q = gq.ptr(); a.rec = rec.ptr();
      OK(step(UPDATE, N, 0, a));
      OK(pk_sync(ctx, nullptr));
      Vec t = made(L), wy = made(L);
      for (size_t i = 0; i < L; ++i) {
        t[i] = q[i];
        if (iterations >= 1.0) t[i] -= 2.0 * r1[i];
        t[i] -= 3.0 * r2[i];
        wy[i] = with_minv ? minv[i] * t[i] : t[i];
      }
      CHECK(g1.fetch() == r2 && g2.fetch() == t && gy.fetch() == wy && gq.fetch() == q);
      CHECK(same_bits(rec.fetch(), reference_b(state, dotp(t, wy))));
    }
  for (double fresh : {1.0, 0.0})      // ---- the solution update runs exactly when fresh == 1, whatever the status
    for (double status : {0.0, 1.0}) {
      Vec state = running(3.0);
      state[STATUS] = status; state[FRESH] = fresh;
      Guarded gx(x), gv(v), gw(w), gw2(w2), rec(state);
      StepArgs a;
      a.x = gx.ptr(); a.v = gv.ptr(); a.w = gw.ptr(); a.w2 = gw2.ptr(); a.rec = rec.ptr();
      OK(step(SOLUTION, N, 0, a));
      OK(pk_sync(ctx, nullptr));
      Vec wn = made(L), wx = made(L);
      for (size_t i = 0; i < L; ++i) {
        wn[i] = ((v[i] - 3.0 * w2[i]) - (-2.0) * w[i]) / 0.5;
        wx[i] = x[i] + 2.0 * wn[i];
      }
      if (fresh == 1.0) CHECK(gx.fetch() == wx && gw.fetch() == wn && gw2.fetch() == w && gv.fetch() == v);
      else CHECK(gx.fetch() == x && gw.fetch() == w && gw2.fetch() == w2 && gv.fetch() == v);
      CHECK(same_bits(rec.fetch(), state));
    }
  for (double status : {1.0, 2.0, 3.0}) {      // ---- a frozen record: a whole iteration leaves x, r1, r2, y, w, w2 and slots 0 ... 14
    Vec state = running(3.0);
    state[STATUS] = status;
    Guarded gx(x), g1(r1), g2(r2), gy(y), gv(v), gw(w), gw2(w2), gq(q), rec(state);
    StepArgs a;
    a.minv = minv.data(); a.s1 = s1.data(); a.s2 = s2.data(); a.x = gx.ptr(); a.r1 = g1.ptr(); a.r2 = g2.ptr(); a.y = gy.ptr(); a.v = gv.ptr();
    a.w = gw.ptr(); a.w2 = gw2.ptr(); a.q = gq.ptr(); a.rec = rec.ptr();
    OK(step(LANCZOS, N, N / 2, a));
    OK(step(ALFA, N, N / 2, a));
    OK(step(UPDATE, N, N / 2, a));
    OK(step(SOLUTION, N, N / 2, a));
    OK(pk_sync(ctx, nullptr));
    CHECK(gx.fetch() == x && g1.fetch() == r1 && g2.fetch() == r2 && gy.fetch() == y && gw.fetch() == w && gw2.fetch() == w2 && gv.fetch() == v);
    CHECK(same_bits(rec.fetch(), state));
  }
  {  // ---- the reciprocal
    Vec g = made(L);
    std::copy(r1.begin(), r1.end(), g.begin());
    if (L > 2) { g[1] = INFINITY; g[2] = NAN; }
    Guarded out(L), out2(L), out3(L);
    StepArgs a;
    a.b = g.data(); a.s1 = s1.data(); a.q = out.ptr();
    OK(step(RECIP, N, 0, a));
    a.s1 = nullptr; a.q = out2.ptr();
    OK(step(RECIP, N, 0, a));
    a.b = nullptr; a.s1 = s1.data(); a.q = out3.ptr();
    OK(step(RECIP, N, 0, a));
    OK(pk_sync(ctx, nullptr));
    const Vec m1 = out.fetch(), m2 = out2.fetch(), m3 = out3.fetch();
    for (size_t i = 0; i < L; ++i) {
      const double a1 = std::fabs(g[i] + s1[i]), a2 = std::fabs(g[i]), a3 = std::fabs(s1[i]);
      CHECK(m1[i] == ((a1 > 0.0 && std::isfinite(a1)) ? 1.0 / a1 : 1.0));
      CHECK(m2[i] == ((a2 > 0.0 && std::isfinite(a2)) ? 1.0 / a2 : 1.0));
      CHECK(m3[i] == (a3 > 0.0 ? 1.0 / a3 : 1.0));
    }
  }
}

// K v by plain loops; s1, s2, hvals may be NULL
static Vec reference_kv(const Csr& A, const Csr& T, const Csr& S, const Vec& jv, const Vec* hv, const Vec* s1, const Vec* s2, const Vec& v) {
  const size_t n = (size_t)A.cols, m = (size_t)A.rows;
  Vec y(n + m, 0.0);
  const Vec jt = matvec(T, jv, v.data() + n), j = matvec(A, jv, v.data());
  for (size_t i = 0; i < n; ++i) y[i] = jt[i] + (s1 ? (*s1)[i] * v[i] : 0.0);
  if (hv) { const Vec h = matvec(S, *hv, v.data()); for (size_t i = 0; i < n; ++i) y[i] += h[i]; }
  for (size_t i = 0; i < m; ++i) y[n + i] = j[i] - (s2 ? (*s2)[i] * v[n + i] : 0.0);
  return y;
}

// begin / advance in chunks / record on "device" pointers
static void device_solve(const double* jv, const double* hv, const double* s1, const double* s2, const double* minv, const double* b,
                         const double* x0, double* x, double tol, int maxiter, int chunk, double* rec) {
  OK(pk_minres_begin_dev(ctx, jv, hv, s1, s2, minv, b, x0, x, tol, nullptr));
  OK(pk_minres_record(ctx, rec));
  for (int done = 0; rec[0] == 0.0 && done < maxiter; done += chunk) {
    OK(pk_minres_advance_dev(ctx, std::min(chunk, maxiter - done), nullptr));
    OK(pk_minres_record(ctx, rec));
  }
}

static int dump(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 3;
  int n, m, nnz_j, nnz_h, with_h, has_s2, has_minv, has_x0, maxiter, chunk;
  double tol;
  if (std::fscanf(f, "%d %d %d %d %d %d %d %d %d %d %la", &n, &m, &nnz_j, &nnz_h, &with_h, &has_s2, &has_minv, &has_x0, &maxiter, &chunk, &tol) != 11)
    return 3;
  const Csr A = read_csr(f, n), T = read_csr(f, m), S = read_csr(f, n);
  const Vec jv = read_doubles(f), hv = read_doubles(f), s1 = read_doubles(f), s2 = read_doubles(f), minv = read_doubles(f), b = read_doubles(f),
            x0 = read_doubles(f);
  std::fclose(f);
  load_model();
  set_problem(n, m, nnz_j, nnz_h);
  set_identity_map(0, nnz_j);
  set_identity_map(1, nnz_h);
  OK(set_operator(0, A));
  OK(set_operator(1, T));
  OK(set_operator(2, S));
  Guarded x((size_t)(n + m));
  Vec rec(16);
  device_solve(jv.data(), with_h ? hv.data() : nullptr, s1.data(), has_s2 ? s2.data() : nullptr, has_minv ? minv.data() : nullptr, b.data(),
               has_x0 ? x0.data() : nullptr, x.ptr(), tol, maxiter, chunk, rec.data());
  for (double v : rec) std::printf("%a\n", v);
  for (double v : x.fetch()) std::printf("%a\n", v);
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "--dump")) return dump(argv[2]);
  load_model();
  set_problem(400, 6, 11, 7);

  // ---- the vector steps; the partial sums grow from one piece to 257
  for (size_t L : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)2047, (size_t)2048, (size_t)2049, (size_t)524289, (size_t)2049})
    check_steps(L);
  {  // refusals of the step form: the code, nothing written
    Guarded q(8), rec(16);
    Vec b(8, 1.0);
    StepArgs a;
    a.b = b.data(); a.x = a.r1 = a.r2 = a.y = a.v = a.w = a.w2 = a.q = q.ptr(); a.rec = rec.ptr(); a.tol = 0.5;
    CHECK(step(7, 8, 4, a) == 134);
    CHECK(step(-1, 8, 4, a) == 134);
    CHECK(step(INIT, -1, 0, a) == 134);
    CHECK(step(INIT, 8, 9, a) == 134);
    CHECK(step(INIT, 8, -1, a) == 134);
    a.tol = -0.5;
    CHECK(step(INIT, 8, 4, a) == 134);
    a.tol = NAN;
    CHECK(step(INIT, 8, 4, a) == 134);
    a.tol = 0.5; a.b = nullptr;
    CHECK(step(INIT, 8, 4, a) == 110);
    CHECK(step(DIAG, 8, 4, a) == 110);
    a.b = b.data(); a.rec = nullptr;
    CHECK(step(UPDATE, 8, 4, a) == 110);
    CHECK(step(LANCZOS, 8, 4, a) == 110);
    CHECK(step(ALFA, 8, 4, a) == 110);
    CHECK(step(SOLUTION, 8, 4, a) == 110);
    a.q = nullptr;
    CHECK(step(RECIP, 8, 4, a) == 110);
    OK(pk_sync(ctx, nullptr));
    for (double v : q.fetch()) CHECK(v == -77.0);
    for (double v : rec.fetch()) CHECK(v == -77.0);
  }

  // ---- K on small integers: J with a long row and, transposed, a long column; H symmetric with gaps
  std::vector<int32_t> lens = {3, 0, 300, 2, 5, 1};
  lens.insert(lens.end(), 290, 1);
  for (size_t r = 6; r < lens.size(); ++r) lens[r] = 2;
  Csr A = from_lengths(lens, 400);
  for (int32_t r = 0; r < A.rows; ++r)      // every row past the sixth also holds column 399 last: J^T's row 399 is long
    if (r >= 6) A.indices[(size_t)A.indptr[(size_t)r + 1] - 1] = 399;
  const Csr T = transposed(A);
  CHECK(T.indptr[400] - T.indptr[399] > 256);
  Csr Lo;
  Lo.rows = Lo.cols = 400;
  Lo.indptr.push_back(0);
  for (int32_t r = 0; r < 400; ++r) {
    if (r >= 2 && r % 5 != 4) Lo.indices.push_back(r - 2);
    if (r % 7 != 3) Lo.indices.push_back(r);
    Lo.indptr.push_back((int32_t)Lo.indices.size());
  }
  const Csr S = symmetric(Lo);
  std::vector<int32_t> pos(400, -1);
  for (int32_t r = 0; r < 400; ++r) {
    const int32_t last = Lo.indptr[(size_t)r + 1] - 1;
    if (last >= Lo.indptr[(size_t)r] && Lo.indices[(size_t)last] == r) pos[(size_t)r] = last;
  }
  const int32_t n = 400, m = A.rows;
  const size_t N = (size_t)(n + m);
  set_problem(n, m, A.nnz(), Lo.nnz());
  Vec jv((size_t)A.nnz()), hv((size_t)Lo.nnz());
  for (size_t e = 0; e < jv.size(); ++e) jv[e] = small_val((int64_t)e);
  for (size_t e = 0; e < hv.size(); ++e) hv[e] = small_val((int64_t)e + 5);
  const Vec vN = ints(N, 11), s1 = ints((size_t)n, 15), s2 = ints((size_t)m, 16);
  {
    Guarded y(N);
    CHECK(pk_kkt_apply_dev(ctx, jv.data(), nullptr, nullptr, nullptr, vN.data(), y.ptr(), nullptr) == 117);      // no operator yet
    set_identity_map(0, A.nnz());
    set_identity_map(1, Lo.nnz());
    OK(set_operator(0, A));
    CHECK(pk_kkt_apply_dev(ctx, jv.data(), nullptr, nullptr, nullptr, vN.data(), y.ptr(), nullptr) == 117);      // J^T is missing
    OK(set_operator(1, T));
    CHECK(pk_kkt_apply_dev(ctx, jv.data(), hv.data(), nullptr, nullptr, vN.data(), y.ptr(), nullptr) == 117);     // H is missing
    OK(set_operator(2, S));
    OK(pk_sync(ctx, nullptr));
    for (double v : y.fetch()) CHECK(v == -77.0);
  }
  for (int with_h = 0; with_h < 2; ++with_h)
    for (int with_s1 = 0; with_s1 < 2; ++with_s1)
      for (int with_s2 = 0; with_s2 < 2; ++with_s2) {
        Guarded y(N);
        OK(pk_kkt_apply_dev(ctx, jv.data(), with_h ? hv.data() : nullptr, with_s1 ? s1.data() : nullptr, with_s2 ? s2.data() : nullptr, vN.data(),
                            y.ptr(), nullptr));
        OK(pk_sync(ctx, nullptr));
        CHECK(y.fetch() == reference_kv(A, T, S, jv, with_h ? &hv : nullptr, with_s1 ? &s1 : nullptr, with_s2 ? &s2 : nullptr, vN));
      }

  // ---- refusals of the device forms: the code, nothing written
  {
    Guarded y(N), x(N);
    Vec host_rec(16, -3.0);
    const size_t mark = fake_hip_log().size();
    CHECK(pk_kkt_apply_dev(ctx, nullptr, nullptr, nullptr, nullptr, vN.data(), y.ptr(), nullptr) == 110);
    CHECK(pk_kkt_apply_dev(ctx, jv.data(), nullptr, nullptr, nullptr, nullptr, y.ptr(), nullptr) == 110);
    CHECK(pk_kkt_apply_dev(ctx, jv.data(), nullptr, nullptr, nullptr, vN.data(), nullptr, nullptr) == 110);
    CHECK(pk_minres_begin_dev(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, vN.data(), nullptr, x.ptr(), 1e-8, nullptr) == 110);
    CHECK(pk_minres_begin_dev(ctx, jv.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, x.ptr(), 1e-8, nullptr) == 110);
    CHECK(pk_minres_begin_dev(ctx, jv.data(), nullptr, nullptr, nullptr, nullptr, vN.data(), nullptr, nullptr, 1e-8, nullptr) == 110);
    CHECK(pk_minres_begin_dev(ctx, jv.data(), nullptr, nullptr, nullptr, nullptr, vN.data(), nullptr, x.ptr(), -1.0, nullptr) == 134);
    CHECK(pk_minres_begin_dev(ctx, jv.data(), nullptr, nullptr, nullptr, nullptr, vN.data(), nullptr, x.ptr(), NAN, nullptr) == 134);
    CHECK(pk_minres_begin_dev(ctx, jv.data(), nullptr, nullptr, nullptr, nullptr, vN.data(), nullptr, x.ptr(), INFINITY, nullptr) == 134);
    CHECK(pk_minres_advance_dev(ctx, 1, nullptr) == 135);                       // no begin yet
    CHECK(pk_minres_record(ctx, host_rec.data()) == 135);
    CHECK(pk_minres_record(ctx, nullptr) == 60);
    OK(pk_set_shard(ctx, 1, 0, nullptr));                                        // a shard is refused
    CHECK(pk_kkt_apply_dev(ctx, jv.data(), nullptr, nullptr, nullptr, vN.data(), y.ptr(), nullptr) == 119);
    CHECK(pk_minres_begin_dev(ctx, jv.data(), nullptr, nullptr, nullptr, nullptr, vN.data(), nullptr, x.ptr(), 1e-8, nullptr) == 119);
    OK(pk_set_shard(ctx, 0, 0, nullptr));
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark);
    for (double v : y.fetch()) CHECK(v == -77.0);
    for (double v : x.fetch()) CHECK(v == -77.0);
    for (double v : host_rec) CHECK(v == -3.0);
  }

  // ---- a solve on device pointers: the diagonal blocks dominate (quasi-definite); what forgets it
  Vec big1((size_t)n), big2((size_t)m);
  for (int i = 0; i < n; ++i) big1[(size_t)i] = 4.0e5 + 1000.0 * (i % 7);
  for (int j = 0; j < m; ++j) big2[(size_t)j] = 3.0e5 + 1000.0 * (j % 5);
  {
    Guarded x(N);
    Vec rec(16), rec2(16);
    device_solve(jv.data(), hv.data(), big1.data(), big2.data(), nullptr, vN.data(), nullptr, x.ptr(), 1e-10, 200, 7, rec.data());
    CHECK(rec[STATUS] == 1.0 && rec[ITERS] > 0.0 && rec[PHIBAR] <= rec[THR] && rec[FRESH] == 0.0);
    const Vec sol = x.fetch();
    const Vec back = reference_kv(A, T, S, jv, &hv, &big1, &big2, sol);
    double worst = 0.0;
    for (size_t i = 0; i < N; ++i) worst = std::max(worst, std::fabs(back[i] - vN[i]));
    CHECK(worst < 1e-6);
    CHECK(pk_minres_advance_dev(ctx, 0, nullptr) == 134);
    OK(pk_minres_advance_dev(ctx, 5, nullptr));                                  // behind the stop: frozen
    OK(pk_minres_record(ctx, rec2.data()));
    CHECK(same_bits(rec, rec2) && same_bits(sol, x.fetch()));
    Guarded x2(N);                                                                // other chunks, the same bits
    device_solve(jv.data(), hv.data(), big1.data(), big2.data(), nullptr, vN.data(), nullptr, x2.ptr(), 1e-10, 200, 1, rec2.data());
    CHECK(same_bits(rec, rec2) && same_bits(sol, x2.fetch()));
    OK(set_operator(1, T));                                                       // pk_set_csr_operator forgets the solve
    CHECK(pk_minres_advance_dev(ctx, 1, nullptr) == 135 && pk_minres_record(ctx, rec2.data()) == 135);
    device_solve(jv.data(), hv.data(), big1.data(), big2.data(), nullptr, vN.data(), nullptr, x2.ptr(), 0.0, 3, 3, rec2.data());
    CHECK(rec2[STATUS] == 0.0 && rec2[ITERS] == 3.0);                             // (still running: exhaustion is the host form's word)
    set_identity_map(0, A.nnz());                                                 // pk_set_csr_map forgets it, and drops the operators
    CHECK(pk_minres_advance_dev(ctx, 1, nullptr) == 135);
    OK(set_operator(0, A));
    OK(set_operator(1, T));
    OK(set_operator(2, S));
    // a caller's preconditioner with negative entries: status 2 at once, x = 0
    Vec neg(N, -1.0);
    Guarded x3(N);
    device_solve(jv.data(), hv.data(), big1.data(), big2.data(), neg.data(), vN.data(), nullptr, x3.ptr(), 1e-10, 10, 4, rec2.data());
    CHECK(rec2[STATUS] == 2.0 && rec2[ITERS] == 0.0);
    for (double v : x3.fetch()) CHECK(v == 0.0);
    // b = 0: converged at once
    Vec zero(N, 0.0);
    device_solve(jv.data(), hv.data(), big1.data(), big2.data(), nullptr, zero.data(), nullptr, x3.ptr(), 1e-10, 10, 4, rec2.data());
    CHECK(rec2[STATUS] == 1.0 && rec2[ITERS] == 0.0);
    for (double v : x3.fetch()) CHECK(v == 0.0);
  }

  // ---- the host forms on the context's linearization against the device-pointer forms on the same values
  {
    Vec x((size_t)n), lam((size_t)m), y(N, -3.0), sol(N, -3.0), rec(16, -3.0);
    for (int i = 0; i < n; ++i) x[(size_t)i] = 2.0 * (double)(i % 9 - 4);
    for (int j = 0; j < m; ++j) lam[(size_t)j] = (double)(j % 5 - 2);
    size_t mark = fake_hip_log().size();
    CHECK(pk_kkt_apply(ctx, 0, nullptr, nullptr, vN.data(), y.data()) == 118);                                    // before pk_linearize
    CHECK(pk_solve_kkt(ctx, 0, big1.data(), big2.data(), 0, nullptr, vN.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 118);
    CHECK(pk_kkt_apply(ctx, 0, nullptr, nullptr, nullptr, y.data()) == 60);
    CHECK(pk_solve_kkt(ctx, 0, big1.data(), big2.data(), 0, nullptr, nullptr, nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 60);
    CHECK(pk_solve_kkt(ctx, 0, big1.data(), big2.data(), 2, nullptr, vN.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 60);
    OK(pk_linearize(ctx, x.data(), nullptr, 1.0));
    CHECK(pk_kkt_apply(ctx, 1, nullptr, nullptr, vN.data(), y.data()) == 118);                                    // a linearization without H
    CHECK(pk_solve_kkt(ctx, 1, big1.data(), big2.data(), 0, nullptr, vN.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 118);
    OK(pk_linearize(ctx, x.data(), lam.data(), 2.0));
    mark = fake_hip_log().size();
    CHECK(pk_solve_kkt(ctx, 1, big1.data(), big2.data(), 0, nullptr, vN.data(), nullptr, -1e-8, 50, 8, sol.data(), rec.data()) == 134);
    CHECK(pk_solve_kkt(ctx, 1, big1.data(), big2.data(), 0, nullptr, vN.data(), nullptr, 1e-8, 0, 8, sol.data(), rec.data()) == 134);
    CHECK(pk_solve_kkt(ctx, 1, big1.data(), big2.data(), 0, nullptr, vN.data(), nullptr, 1e-8, 50, 0, sol.data(), rec.data()) == 134);
    CHECK(pk_solve_kkt(ctx, 1, big1.data(), big2.data(), 3, nullptr, vN.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 134);
    CHECK(pk_solve_kkt(ctx, 1, big1.data(), big2.data(), -1, nullptr, vN.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 134);
    CHECK(pk_solve_kkt(ctx, 1, big1.data(), big2.data(), 1, nullptr, vN.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 132);   // diagonal with H, no positions
    OK(pk_set_shard(ctx, 1, 0, nullptr));
    CHECK(pk_solve_kkt(ctx, 1, big1.data(), big2.data(), 0, nullptr, vN.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 119);
    CHECK(pk_kkt_apply(ctx, 1, nullptr, nullptr, vN.data(), y.data()) == 119);
    OK(pk_set_shard(ctx, 0, 0, nullptr));
    CHECK(fake_hip_log().size() == mark);
    for (double v : sol) CHECK(v == -3.0);
    for (double v : rec) CHECK(v == -3.0);
    for (double v : y) CHECK(v == -3.0);
    OK(pk_set_operator_diagonal(ctx, 2, pos.data(), n));
    Vec lj((size_t)A.nnz()), lh((size_t)Lo.nnz());
    for (int64_t e = 0; e < A.nnz(); ++e) lj[(size_t)e] = fake_jac(x.data(), n, e, false);
    for (int64_t e = 0; e < Lo.nnz(); ++e) lh[(size_t)e] = fake_hess(x.data(), lam.data(), 2.0, n, m, e);
    Vec huge1((size_t)n), huge2((size_t)m);
    for (int i = 0; i < n; ++i) huge1[(size_t)i] = 1.0e9 + 1.0e6 * (i % 5);
    for (int j = 0; j < m; ++j) huge2[(size_t)j] = 1.0e9 + 1.0e6 * (j % 3);
    const Vec x0 = ints(N, 21);
    for (int with_h = 0; with_h < 2; ++with_h)
      for (int variant = 0; variant < 3; ++variant) {      // 0: the device-built diagonal, x0; 1: no preconditioner, no x0; 2: the caller's minv
        const double* x0p = variant == 0 ? x0.data() : nullptr;
        const double* lhp = with_h ? lh.data() : nullptr;
        // K v: host form against the device form on the same values, and against plain loops
        Vec hy(N, -3.0);
        Guarded dy(N);
        OK(pk_kkt_apply(ctx, with_h, huge1.data(), variant == 1 ? nullptr : huge2.data(), vN.data(), hy.data()));
        OK(pk_kkt_apply_dev(ctx, lj.data(), lhp, huge1.data(), variant == 1 ? nullptr : huge2.data(), vN.data(), dy.ptr(), nullptr));
        OK(pk_sync(ctx, nullptr));
        CHECK(same_bits(hy, dy.fetch()));
        // the diagonal preconditioner by plain arithmetic on the reductions' results
        Vec g1((size_t)n, 0.0), g2((size_t)m), minv(N);
        if (with_h) OK(pk_operator_diagonal(ctx, 2, g1.data()));
        for (int i = 0; i < n; ++i) minv[(size_t)i] = 1.0 / std::fabs(g1[(size_t)i] + huge1[(size_t)i]);
        OK(pk_operator_reduce(ctx, 0, 1, minv.data(), 0, g2.data()));
        for (int j = 0; j < m; ++j) minv[(size_t)(n + j)] = 1.0 / std::fabs(g2[(size_t)j] + huge2[(size_t)j]);
        const int precond = variant == 0 ? 1 : variant == 1 ? 0 : 2;
        for (int ce : {1, 3, 64}) {
          Guarded hx(N), hrec(16);
          OK(pk_solve_kkt(ctx, with_h, huge1.data(), huge2.data(), precond, precond == 2 ? minv.data() : nullptr, vN.data(), x0p, 1e-9, 40, ce,
                          hx.ptr(), hrec.ptr()));
          Guarded dx(N);
          Vec drec(16);
          device_solve(lj.data(), lhp, huge1.data(), huge2.data(), precond ? minv.data() : nullptr, vN.data(), x0p, dx.ptr(), 1e-9, 40, ce,
                       drec.data());
          if (drec[STATUS] == 0.0) drec[STATUS] = 4.0;
          CHECK(hrec.fetch()[STATUS] == 1.0 && hrec.fetch()[FRESH] == 0.0);
          CHECK(same_bits(hrec.fetch(), drec) && same_bits(hx.fetch(), dx.fetch()));
        }
      }
    // exhaustion is status 4 in the host copy, and a result: the call returns 0
    OK(pk_solve_kkt(ctx, 1, huge1.data(), huge2.data(), 0, nullptr, vN.data(), nullptr, 0.0, 2, 8, sol.data(), rec.data()));
    CHECK(rec[STATUS] == 4.0 && rec[ITERS] == 2.0 && rec[FRESH] == 0.0);
    std::vector<double> hvals((size_t)Lo.nnz());
    OK(pk_eval_hess_csr(ctx, x.data(), lam.data(), 2.0, hvals.data()));           // the value arrays now hold another evaluation
    CHECK(pk_kkt_apply(ctx, 0, nullptr, nullptr, vN.data(), y.data()) == 118);
  }

  // ---- what frees the state: a new problem, and pk_destroy leaves no live allocation
  CHECK(fake_hip_live_allocations() > 0);
  set_problem(400, 6, 11, 7);
  {
    Vec rec(16);
    CHECK(pk_minres_record(ctx, rec.data()) == 135);
  }
  check_steps(2049);                                                           // (allocated again on first use)
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return checks_passed();
}
