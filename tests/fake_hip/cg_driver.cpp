// cg_driver.cpp -- TEST INFRASTRUCTURE: drives the CG entry points (pockit_amd/csrc/pk_cg.cpp) against the host-only HIP stand-in of
// this directory, built with -fsanitize=address,undefined (tests/test_cg_cpu.py): the stand-in walk of every vector step against
// plain loops on small integers (every product and every sum is exact in fp64, so a result must EQUAL the loop), one application
// of K in both forms with and without H, d and s against plain loops, the host form against begin / advance / record, every
// refusal with its code and nothing enqueued behind it, sentinels around x and the record, what frees and forgets the state, and
// tear-down without a live allocation.  With --dump FILE: the solve FILE describes (tests/test_cg_cpu.py writes it from
// tests/cg_cases.py) through begin / advance / record, x and the record printed as hex doubles.
#include <cmath>
#include <cstring>

#include "driver_common.h"

enum { INIT = 0, CURVATURE = 1, UPDATE = 2, DIRECTION = 3, SCALE = 4, JACOBI = 5 };

static int step(int which, int64_t len, const double* b, const double* x0, const double* minv, const double* s, double* x, double* r,
                double* z, double* p, double* q, double* rec, double tol) {
  return pk_cg_step_dev(ctx, which, len, b, x0, minv, s, x, r, z, p, q, rec, tol, nullptr);
}

// every vector step at one length against plain loops
static void check_steps(size_t L) {
  const Vec b = ints(L, 1), x0 = ints(L, 2), kx = ints(L, 3), minv = ints(L, 4, true), s = ints(L, 5);
  for (int variant = 0; variant < 2; ++variant) {      // 0: x0, minv and s given; 1: none of them
    const bool full = variant == 0;
    Guarded x(L), r(L), z(L), p(L), q(full ? Guarded(kx) : Guarded(L)), rec(8);
    OK(step(INIT, (int64_t)L, b.data(), full ? x0.data() : nullptr, full ? minv.data() : nullptr, full ? s.data() : nullptr, x.ptr(), r.ptr(),
            z.ptr(), p.ptr(), q.ptr(), rec.ptr(), 0.5));
    OK(pk_sync(ctx, nullptr));
    Vec wr = made(L), wz = made(L), wq = made(L), wx = made(L);
    for (size_t i = 0; i < L; ++i) {
      wx[i] = full ? x0[i] : 0.0;
      wr[i] = full ? b[i] - kx[i] : b[i];
      wz[i] = full ? minv[i] * wr[i] : wr[i];
      wq[i] = full ? s[i] * wz[i] : 0.0;
    }
    CHECK(x.fetch() == wx && r.fetch() == wr && z.fetch() == wz && p.fetch() == wz && q.fetch() == wq);
    const double bb = dotp(b, b), rz = dotp(wr, wz), rr = dotp(wr, wr), thr = 0.25 * bb;
    CHECK(rec.fetch() == (Vec{rr <= thr ? 1.0 : 0.0, 0.0, rr, thr, rz, 0.0, 0.0, 0.0}));
  }
  const Vec x = ints(L, 6), r = ints(L, 7), z = ints(L, 8), p = ints(L, 9), q = ints(L, 10);
  {  // ---- curvature: a positive, a negative (p . -q... ) and a zero one
    for (int sign = -1; sign <= 1; ++sign) {
      Vec qq = made(L);
      for (size_t i = 0; i < L; ++i) qq[i] = sign == 0 ? 0.0 : sign * p[i];
      Guarded rec(Vec{0.0, 3.0, 9.0, 1.0, 6.0, -1.0, -2.0, -3.0});
      OK(step(CURVATURE, (int64_t)L, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, const_cast<double*>(p.data()), qq.data(),
              rec.ptr(), 0.0));
      OK(pk_sync(ctx, nullptr));
      const double pq = dotp(p, qq);
      const Vec got = rec.fetch();
      if (pq > 0.0) CHECK(got == (Vec{0.0, 3.0, 9.0, 1.0, 6.0, pq, 6.0 / pq, -3.0}));
      else CHECK(got == (Vec{2.0, 3.0, 9.0, 1.0, 6.0, pq, -2.0, -3.0}));
    }
  }
  for (int with_minv = 0; with_minv < 2; ++with_minv) {  // ---- update (alpha = 2) and direction (beta = 0.5)
    Guarded gx(x), gr(r), gz(z), gp(p), gq(q), rec(Vec{0.0, 3.0, 9.0, 1.0, 6.0, 5.0, 2.0, -3.0});
    OK(step(UPDATE, (int64_t)L, nullptr, nullptr, with_minv ? minv.data() : nullptr, nullptr, gx.ptr(), gr.ptr(), gz.ptr(), gp.ptr(), gq.ptr(),
            rec.ptr(), 0.0));
    OK(pk_sync(ctx, nullptr));
    Vec wx(L), wr(L), wz(L);
    for (size_t i = 0; i < L; ++i) {
      wx[i] = x[i] + 2.0 * p[i];
      wr[i] = r[i] - 2.0 * q[i];
      wz[i] = with_minv ? minv[i] * wr[i] : wr[i];
    }
    CHECK(gx.fetch() == wx && gr.fetch() == wr && gz.fetch() == wz && gp.fetch() == p && gq.fetch() == q);
    const double rz = dotp(wr, wz), rr = dotp(wr, wr);
    Vec want = rr <= 1.0 ? Vec{1.0, 4.0, rr, 1.0, 6.0, 5.0, 2.0, -3.0} : Vec{0.0, 4.0, rr, 1.0, rz, 5.0, 2.0, rz / 6.0};
    CHECK(rec.fetch() == want);
    Vec state = rec.fetch();
    state[7] = 0.5;
    Guarded rec2(state);
    OK(step(DIRECTION, (int64_t)L, nullptr, nullptr, nullptr, s.data(), nullptr, nullptr, gz.ptr(), gp.ptr(), gq.ptr(), rec2.ptr(), 0.0));
    OK(pk_sync(ctx, nullptr));
    Vec wp(L), wq(L);
    for (size_t i = 0; i < L; ++i) {
      wp[i] = state[0] == 0.0 ? wz[i] + 0.5 * p[i] : p[i];
      wq[i] = s[i] * wp[i];
    }
    CHECK(gp.fetch() == wp && gq.fetch() == wq && rec2.fetch() == state);
  }
  for (double status : {1.0, 2.0, 3.0}) {  // ---- a frozen record: x, r, z, p and the record stay; q = s o p
    Guarded gx(x), gr(r), gz(z), gp(p), gq(q), rec(Vec{status, 3.0, 9.0, 1.0, 6.0, 5.0, 2.0, 0.5});
    OK(step(CURVATURE, (int64_t)L, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, gp.ptr(), gq.ptr(), rec.ptr(), 0.0));
    OK(step(UPDATE, (int64_t)L, nullptr, nullptr, minv.data(), nullptr, gx.ptr(), gr.ptr(), gz.ptr(), gp.ptr(), gq.ptr(), rec.ptr(), 0.0));
    OK(step(DIRECTION, (int64_t)L, nullptr, nullptr, nullptr, s.data(), nullptr, nullptr, gz.ptr(), gp.ptr(), gq.ptr(), rec.ptr(), 0.0));
    OK(pk_sync(ctx, nullptr));
    Vec wq(L);
    for (size_t i = 0; i < L; ++i) wq[i] = s[i] * p[i];
    CHECK(gx.fetch() == x && gr.fetch() == r && gz.fetch() == z && gp.fetch() == p && gq.fetch() == wq);
    CHECK(rec.fetch() == (Vec{status, 3.0, 9.0, 1.0, 6.0, 5.0, 2.0, 0.5}));
  }
  {  // ---- scale and the Jacobi reciprocal
    Guarded gq(q), out(L), out2(L);
    OK(step(SCALE, (int64_t)L, nullptr, nullptr, nullptr, s.data(), nullptr, nullptr, nullptr, nullptr, gq.ptr(), nullptr, 0.0));
    Vec g = made(L);
    std::copy(r.begin(), r.end(), g.begin());
    if (L > 2) { g[1] = INFINITY; g[2] = NAN; }
    OK(step(JACOBI, (int64_t)L, g.data(), nullptr, nullptr, s.data(), nullptr, nullptr, nullptr, nullptr, out.ptr(), nullptr, 0.0));
    OK(step(JACOBI, (int64_t)L, g.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out2.ptr(), nullptr, 0.0));
    OK(pk_sync(ctx, nullptr));
    const Vec sq = gq.fetch(), m1 = out.fetch(), m2 = out2.fetch();
    for (size_t i = 0; i < L; ++i) {
      CHECK(sq[i] == s[i] * q[i]);
      const double a = std::fabs(g[i] + s[i]), a2 = std::fabs(g[i]);
      CHECK(m1[i] == ((a > 0.0 && std::isfinite(a)) ? 1.0 / a : 1.0));
      CHECK(m2[i] == ((a2 > 0.0 && std::isfinite(a2)) ? 1.0 / a2 : 1.0));
    }
  }
}

// K v by plain loops; d, s, hvals may be NULL
static Vec reference_kv(int form, const Csr& A, const Csr& T, const Csr& S, const Vec& jv, const Vec* hv, const Vec* d, const Vec* s, const Vec& v) {
  Vec t = matvec(form == 0 ? A : T, jv, v.data());
  if (d) for (size_t i = 0; i < t.size(); ++i) t[i] = (*d)[i] * t[i];
  Vec y = matvec(form == 0 ? T : A, jv, t.data());
  if (hv) { const Vec h = matvec(S, *hv, v.data()); for (size_t i = 0; i < y.size(); ++i) y[i] += h[i]; }
  if (s) for (size_t i = 0; i < y.size(); ++i) y[i] += (*s)[i] * v[i];
  return y;
}

// begin / advance in chunks / record on "device" pointers
static void device_solve(int form, const double* jv, const double* hv, const double* d, const double* s, const double* minv, const double* b,
                         const double* x0, double* x, double tol, int maxiter, int chunk, double* rec) {
  OK(pk_cg_begin_dev(ctx, form, jv, hv, d, s, minv, b, x0, x, tol, nullptr));
  OK(pk_cg_record(ctx, rec));
  for (int done = 0; rec[0] == 0.0 && done < maxiter; done += chunk) {
    OK(pk_cg_advance_dev(ctx, std::min(chunk, maxiter - done), nullptr));
    OK(pk_cg_record(ctx, rec));
  }
}

// ---------------------------------------------------------------- --dump: the solve a file describes
static int dump(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 3;
  int n, m, nnz_j, nnz_h, form, with_h, has_minv, has_x0, maxiter, chunk;
  double tol;
  if (std::fscanf(f, "%d %d %d %d %d %d %d %d %d %d %la", &n, &m, &nnz_j, &nnz_h, &form, &with_h, &has_minv, &has_x0, &maxiter, &chunk, &tol) != 11)
    return 3;
  const Csr A = read_csr(f, n), T = read_csr(f, m), S = read_csr(f, n);
  const Vec jv = read_doubles(f), hv = read_doubles(f), d = read_doubles(f), s = read_doubles(f), minv = read_doubles(f), b = read_doubles(f),
            x0 = read_doubles(f);
  std::fclose(f);
  load_model();
  set_problem(n, m, nnz_j, nnz_h);
  set_identity_map(0, nnz_j);
  set_identity_map(1, nnz_h);
  OK(set_operator(0, A));
  OK(set_operator(1, T));
  OK(set_operator(2, S));
  Guarded x((size_t)(form == 0 ? n : m));
  Vec rec(8);
  device_solve(form, jv.data(), with_h ? hv.data() : nullptr, d.data(), s.data(), has_minv ? minv.data() : nullptr, b.data(),
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
    Guarded q(8), rec(8);
    Vec b(8, 1.0);
    CHECK(step(6, 8, b.data(), nullptr, nullptr, nullptr, q.ptr(), q.ptr(), q.ptr(), q.ptr(), q.ptr(), rec.ptr(), 0.5) == 134);
    CHECK(step(-1, 8, b.data(), nullptr, nullptr, nullptr, q.ptr(), q.ptr(), q.ptr(), q.ptr(), q.ptr(), rec.ptr(), 0.5) == 134);
    CHECK(step(INIT, -1, b.data(), nullptr, nullptr, nullptr, q.ptr(), q.ptr(), q.ptr(), q.ptr(), q.ptr(), rec.ptr(), 0.5) == 134);
    CHECK(step(INIT, 8, b.data(), nullptr, nullptr, nullptr, q.ptr(), q.ptr(), q.ptr(), q.ptr(), q.ptr(), rec.ptr(), -0.5) == 134);
    CHECK(step(INIT, 8, b.data(), nullptr, nullptr, nullptr, q.ptr(), q.ptr(), q.ptr(), q.ptr(), q.ptr(), rec.ptr(), NAN) == 134);
    CHECK(step(INIT, 8, nullptr, nullptr, nullptr, nullptr, q.ptr(), q.ptr(), q.ptr(), q.ptr(), q.ptr(), rec.ptr(), 0.5) == 110);
    CHECK(step(UPDATE, 8, nullptr, nullptr, nullptr, nullptr, q.ptr(), q.ptr(), q.ptr(), q.ptr(), q.ptr(), nullptr, 0.5) == 110);
    CHECK(step(SCALE, 8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, q.ptr(), nullptr, 0.5) == 110);
    OK(pk_sync(ctx, nullptr));
    for (double v : q.fetch()) CHECK(v == -77.0);
    for (double v : rec.fetch()) CHECK(v == -77.0);
  }

  // ---- K in both forms on small integers: J with a long row and, transposed, a long column; H symmetric with gaps
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
  set_problem(n, m, A.nnz(), Lo.nnz());
  CHECK(fake_hip_live_allocations() > 0);
  Vec jv((size_t)A.nnz()), hv((size_t)Lo.nnz());
  for (size_t e = 0; e < jv.size(); ++e) jv[e] = small_val((int64_t)e);
  for (size_t e = 0; e < hv.size(); ++e) hv[e] = small_val((int64_t)e + 5);
  const Vec vn = ints((size_t)n, 11), vm = ints((size_t)m, 12), dn = ints((size_t)n, 13), dm = ints((size_t)m, 14), sn = ints((size_t)n, 15),
            sm = ints((size_t)m, 16);
  {
    Guarded y((size_t)n);
    CHECK(pk_condensed_apply_dev(ctx, 0, jv.data(), nullptr, nullptr, nullptr, vn.data(), y.ptr(), nullptr) == 117);      // no operator yet
    set_identity_map(0, A.nnz());
    set_identity_map(1, Lo.nnz());
    OK(set_operator(0, A));
    CHECK(pk_condensed_apply_dev(ctx, 0, jv.data(), nullptr, nullptr, nullptr, vn.data(), y.ptr(), nullptr) == 117);      // J^T is missing
    OK(set_operator(1, T));
    CHECK(pk_condensed_apply_dev(ctx, 0, jv.data(), hv.data(), nullptr, nullptr, vn.data(), y.ptr(), nullptr) == 117);     // H is missing
    OK(set_operator(2, S));
    OK(pk_sync(ctx, nullptr));
    for (double v : y.fetch()) CHECK(v == -77.0);
  }
  for (int form = 0; form < 2; ++form)
    for (int with_h = 0; with_h <= (form == 0 ? 1 : 0); ++with_h)
      for (int with_d = 0; with_d < 2; ++with_d)
        for (int with_s = 0; with_s < 2; ++with_s) {
          const Vec& v = form == 0 ? vn : vm;
          const Vec& d = form == 0 ? dm : dn;
          const Vec& s = form == 0 ? sn : sm;
          Guarded y(v.size());
          OK(pk_condensed_apply_dev(ctx, form, jv.data(), with_h ? hv.data() : nullptr, with_d ? d.data() : nullptr, with_s ? s.data() : nullptr,
                                    v.data(), y.ptr(), nullptr));
          OK(pk_sync(ctx, nullptr));
          CHECK(y.fetch() == reference_kv(form, A, T, S, jv, with_h ? &hv : nullptr, with_d ? &d : nullptr, with_s ? &s : nullptr, v));
        }

  // ---- refusals of the device forms: the code, nothing written
  {
    Guarded y((size_t)n), rec(8);
    Vec host_rec(8, -3.0);
    const size_t mark = fake_hip_log().size();
    CHECK(pk_condensed_apply_dev(ctx, 2, jv.data(), nullptr, nullptr, nullptr, vn.data(), y.ptr(), nullptr) == 133);
    CHECK(pk_condensed_apply_dev(ctx, -1, jv.data(), nullptr, nullptr, nullptr, vn.data(), y.ptr(), nullptr) == 133);
    CHECK(pk_condensed_apply_dev(ctx, 1, jv.data(), hv.data(), nullptr, nullptr, vm.data(), y.ptr(), nullptr) == 133);      // H with the dual form
    CHECK(pk_condensed_apply_dev(ctx, 0, nullptr, nullptr, nullptr, nullptr, vn.data(), y.ptr(), nullptr) == 110);
    CHECK(pk_condensed_apply_dev(ctx, 0, jv.data(), nullptr, nullptr, nullptr, nullptr, y.ptr(), nullptr) == 110);
    CHECK(pk_condensed_apply_dev(ctx, 0, jv.data(), nullptr, nullptr, nullptr, vn.data(), nullptr, nullptr) == 110);
    CHECK(pk_cg_begin_dev(ctx, 3, jv.data(), nullptr, nullptr, nullptr, nullptr, vn.data(), nullptr, y.ptr(), 1e-8, nullptr) == 133);
    CHECK(pk_cg_begin_dev(ctx, 1, jv.data(), hv.data(), nullptr, nullptr, nullptr, vm.data(), nullptr, y.ptr(), 1e-8, nullptr) == 133);
    CHECK(pk_cg_begin_dev(ctx, 0, jv.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, y.ptr(), 1e-8, nullptr) == 110);
    CHECK(pk_cg_begin_dev(ctx, 0, jv.data(), nullptr, nullptr, nullptr, nullptr, vn.data(), nullptr, nullptr, 1e-8, nullptr) == 110);
    CHECK(pk_cg_begin_dev(ctx, 0, jv.data(), nullptr, nullptr, nullptr, nullptr, vn.data(), nullptr, y.ptr(), -1.0, nullptr) == 134);
    CHECK(pk_cg_begin_dev(ctx, 0, jv.data(), nullptr, nullptr, nullptr, nullptr, vn.data(), nullptr, y.ptr(), NAN, nullptr) == 134);
    CHECK(pk_cg_begin_dev(ctx, 0, jv.data(), nullptr, nullptr, nullptr, nullptr, vn.data(), nullptr, y.ptr(), INFINITY, nullptr) == 134);
    CHECK(pk_cg_advance_dev(ctx, 1, nullptr) == 135);                       // no begin yet
    CHECK(pk_cg_record(ctx, host_rec.data()) == 135);
    CHECK(pk_cg_record(ctx, nullptr) == 60);
    OK(pk_set_shard(ctx, 1, 0, nullptr));                                    // a shard is refused
    CHECK(pk_condensed_apply_dev(ctx, 0, jv.data(), nullptr, nullptr, nullptr, vn.data(), y.ptr(), nullptr) == 119);
    CHECK(pk_cg_begin_dev(ctx, 0, jv.data(), nullptr, nullptr, nullptr, nullptr, vn.data(), nullptr, y.ptr(), 1e-8, nullptr) == 119);
    OK(pk_set_shard(ctx, 0, 0, nullptr));
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark);
    for (double v : y.fetch()) CHECK(v == -77.0);
    for (double v : host_rec) CHECK(v == -3.0);
  }

  // ---- a solve on device pointers: K = J^T J + H + S with S large (positive definite); what forgets it
  Vec big((size_t)n);
  for (int i = 0; i < n; ++i) big[(size_t)i] = 4.0e5 + 1000.0 * (i % 7);
  {
    Guarded x((size_t)n);
    Vec rec(8), rec2(8);
    device_solve(0, jv.data(), hv.data(), nullptr, big.data(), nullptr, vn.data(), nullptr, x.ptr(), 1e-10, 200, 7, rec.data());
    CHECK(rec[0] == 1.0 && rec[1] > 0.0 && rec[2] <= rec[3]);
    const Vec sol = x.fetch();
    const Vec back = reference_kv(0, A, T, S, jv, &hv, nullptr, &big, sol);
    double worst = 0.0;
    for (int i = 0; i < n; ++i) worst = std::max(worst, std::fabs(back[(size_t)i] - vn[(size_t)i]));
    CHECK(worst < 1e-6);
    CHECK(pk_cg_advance_dev(ctx, 0, nullptr) == 134);
    OK(pk_cg_advance_dev(ctx, 5, nullptr));                                  // behind the stop: frozen
    OK(pk_cg_record(ctx, rec2.data()));
    CHECK(same_bits(rec, rec2) && same_bits(sol, x.fetch()));
    Guarded x2((size_t)n);                                                    // other chunks, the same bits
    device_solve(0, jv.data(), hv.data(), nullptr, big.data(), nullptr, vn.data(), nullptr, x2.ptr(), 1e-10, 200, 1, rec2.data());
    CHECK(same_bits(rec, rec2) && same_bits(sol, x2.fetch()));
    OK(set_operator(1, T));                                                   // pk_set_csr_operator forgets the solve
    CHECK(pk_cg_advance_dev(ctx, 1, nullptr) == 135 && pk_cg_record(ctx, rec2.data()) == 135);
    device_solve(0, jv.data(), hv.data(), nullptr, big.data(), nullptr, vn.data(), nullptr, x2.ptr(), 1e-10, 3, 3, rec2.data());
    CHECK(rec2[0] == 0.0 && rec2[1] == 3.0);                                  // (still running: exhaustion is the host form's word)
    set_identity_map(0, A.nnz());                                             // pk_set_csr_map forgets it, and drops the operators
    CHECK(pk_cg_advance_dev(ctx, 1, nullptr) == 135);
    OK(set_operator(0, A));
    OK(set_operator(1, T));
    OK(set_operator(2, S));
  }

  // ---- the host forms on the context's linearization against the device-pointer forms on the same values
  {
    Vec x((size_t)n), lam((size_t)m), y((size_t)n, -3.0), sol((size_t)n, -3.0), rec(8, -3.0);
    for (int i = 0; i < n; ++i) x[(size_t)i] = 2.0 * (double)(i % 9 - 4);
    for (int j = 0; j < m; ++j) lam[(size_t)j] = (double)(j % 5 - 2);
    size_t mark = fake_hip_log().size();
    CHECK(pk_condensed_apply(ctx, 0, 0, nullptr, nullptr, vn.data(), y.data()) == 118);                                 // before pk_linearize
    CHECK(pk_solve_condensed(ctx, 0, 0, nullptr, big.data(), 0, nullptr, vn.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 118);
    CHECK(pk_condensed_apply(ctx, 0, 0, nullptr, nullptr, nullptr, y.data()) == 60);
    CHECK(pk_solve_condensed(ctx, 0, 0, nullptr, big.data(), 0, nullptr, nullptr, nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 60);
    CHECK(pk_solve_condensed(ctx, 0, 0, nullptr, big.data(), 2, nullptr, vn.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 60);
    OK(pk_linearize(ctx, x.data(), nullptr, 1.0));
    CHECK(pk_condensed_apply(ctx, 0, 1, nullptr, nullptr, vn.data(), y.data()) == 118);                                 // a linearization without H
    CHECK(pk_solve_condensed(ctx, 0, 1, nullptr, big.data(), 0, nullptr, vn.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 118);
    OK(pk_linearize(ctx, x.data(), lam.data(), 2.0));
    mark = fake_hip_log().size();
    CHECK(pk_solve_condensed(ctx, 2, 0, nullptr, big.data(), 0, nullptr, vn.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 133);
    CHECK(pk_solve_condensed(ctx, 1, 1, nullptr, big.data(), 0, nullptr, vm.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 133);
    CHECK(pk_solve_condensed(ctx, 0, 1, nullptr, big.data(), 0, nullptr, vn.data(), nullptr, -1e-8, 50, 8, sol.data(), rec.data()) == 134);
    CHECK(pk_solve_condensed(ctx, 0, 1, nullptr, big.data(), 0, nullptr, vn.data(), nullptr, 1e-8, 0, 8, sol.data(), rec.data()) == 134);
    CHECK(pk_solve_condensed(ctx, 0, 1, nullptr, big.data(), 0, nullptr, vn.data(), nullptr, 1e-8, 50, 0, sol.data(), rec.data()) == 134);
    CHECK(pk_solve_condensed(ctx, 0, 1, nullptr, big.data(), 3, nullptr, vn.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 134);
    CHECK(pk_solve_condensed(ctx, 0, 1, nullptr, big.data(), -1, nullptr, vn.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 134);
    CHECK(pk_solve_condensed(ctx, 0, 1, nullptr, big.data(), 1, nullptr, vn.data(), nullptr, 1e-8, 50, 8, sol.data(), rec.data()) == 132);   // Jacobi with H, no positions
    CHECK(fake_hip_log().size() == mark);
    for (double v : sol) CHECK(v == -3.0);
    for (double v : rec) CHECK(v == -3.0);
    OK(pk_set_operator_diagonal(ctx, 2, pos.data(), n));
    Vec lj((size_t)A.nnz()), lh((size_t)Lo.nnz());
    for (int64_t e = 0; e < A.nnz(); ++e) lj[(size_t)e] = fake_jac(x.data(), n, e, false);
    for (int64_t e = 0; e < Lo.nnz(); ++e) lh[(size_t)e] = fake_hess(x.data(), lam.data(), 2.0, n, m, e);
    Vec huge((size_t)n), hm((size_t)m);
    for (int i = 0; i < n; ++i) huge[(size_t)i] = 1.0e9 + 1.0e6 * (i % 5);
    for (int j = 0; j < m; ++j) hm[(size_t)j] = 1.0e9 + 1.0e6 * (j % 3);
    Vec dpos_m((size_t)m), dpos_n((size_t)n), x0n = ints((size_t)n, 21), x0m = ints((size_t)m, 22);
    for (int j = 0; j < m; ++j) dpos_m[(size_t)j] = 1.0 + j % 3;
    for (int i = 0; i < n; ++i) dpos_n[(size_t)i] = 1.0 + i % 4;
    for (int form = 0; form < 2; ++form)
      for (int with_h = 0; with_h <= (form == 0 ? 1 : 0); ++with_h)
        for (int variant = 0; variant < 3; ++variant) {      // 0: d, Jacobi, x0; 1: no d, no preconditioner, no x0; 2: the caller's minv
          const size_t N = form == 0 ? (size_t)n : (size_t)m;
          const Vec& b = form == 0 ? vn : vm;
          const Vec& s = form == 0 ? huge : hm;
          const Vec& d = form == 0 ? dpos_m : dpos_n;
          const Vec& x0 = form == 0 ? x0n : x0m;
          const double* dp = variant == 1 ? nullptr : d.data();
          const double* x0p = variant == 0 ? x0.data() : nullptr;
          // K v: host form against the device form on the same values
          Vec hy(N, -3.0);
          Guarded dy(N);
          OK(pk_condensed_apply(ctx, form, with_h, dp, s.data(), b.data(), hy.data()));
          OK(pk_condensed_apply_dev(ctx, form, lj.data(), with_h ? lh.data() : nullptr, dp, s.data(), b.data(), dy.ptr(), nullptr));
          OK(pk_sync(ctx, nullptr));
          CHECK(same_bits(hy, dy.fetch()));
          // the Jacobi vector by plain arithmetic on the reductions' results
          Vec g(N), minv(N);
          if (form == 0) {
            OK(pk_operator_reduce(ctx, 1, 1, dp, with_h, g.data()));
          } else {
            OK(pk_operator_reduce(ctx, 0, 1, dp, 0, g.data()));
          }
          for (size_t i = 0; i < N; ++i) minv[i] = 1.0 / std::fabs(g[i] + s[i]);
          const int precond = variant == 0 ? 1 : variant == 1 ? 0 : 2;
          for (int ce : {1, 3, 64}) {
            Guarded hx(N), hrec(8);
            OK(pk_solve_condensed(ctx, form, with_h, dp, s.data(), precond, precond == 2 ? minv.data() : nullptr, b.data(), x0p, 1e-9, 40, ce,
                                  hx.ptr(), hrec.ptr()));
            Guarded dx(N);
            Vec drec(8);
            device_solve(form, lj.data(), with_h ? lh.data() : nullptr, dp, s.data(), precond ? minv.data() : nullptr, b.data(), x0p, dx.ptr(), 1e-9,
                         40, ce, drec.data());
            if (drec[0] == 0.0) drec[0] = 4.0;
            CHECK(hrec.fetch()[0] == 1.0);
            CHECK(same_bits(hrec.fetch(), drec) && same_bits(hx.fetch(), dx.fetch()));
          }
        }
    // exhaustion is status 4 in the host copy, and a result: the call returns 0
    OK(pk_solve_condensed(ctx, 0, 1, nullptr, huge.data(), 0, nullptr, vn.data(), nullptr, 0.0, 2, 8, sol.data(), rec.data()));
    CHECK(rec[0] == 4.0 && rec[1] == 2.0);
    std::vector<double> hvals((size_t)Lo.nnz());
    OK(pk_eval_hess_csr(ctx, x.data(), lam.data(), 2.0, hvals.data()));           // the value arrays now hold another evaluation
    CHECK(pk_condensed_apply(ctx, 0, 0, nullptr, nullptr, vn.data(), y.data()) == 118);
  }

  // ---- what frees the state: a new problem, and pk_destroy leaves no live allocation
  set_problem(400, 6, 11, 7);
  {
    Vec rec(8);
    CHECK(pk_cg_record(ctx, rec.data()) == 135);
  }
  check_steps(2049);                                                           // (allocated again on first use)
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return checks_passed();
}
