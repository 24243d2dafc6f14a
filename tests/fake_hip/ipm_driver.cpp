// ipm_driver.cpp -- TEST INFRASTRUCTURE: drives the entry points of pockit_amd/csrc/pk_ipm.cpp (barrier terms, dual residual,
// boundary step) against the host-only HIP stand-in of this directory, built with -fsanitize=address,undefined
// (tests/test_ipm_cpu.py): the stand-in walk of every kernel against plain loops on small integers and powers of two (every
// product, quotient and sum but the logarithms' is exact in fp64, so a result must EQUAL the loop; column 4 is held to a bound),
// clean and with planted defects, the public forms against the raw form and the host forms against the device forms, every
// refusal with its code and nothing enqueued or written behind it, sentinels around every output, and tear-down without a live
// allocation.  With --dump FILE: the boxed vector FILE describes (tests/test_ipm_cpu.py writes it from tests/ipm_cases.py)
// through the raw form, every vector and record printed as hex doubles.
#include <cmath>
#include <cstring>

#include "driver_common.h"

enum { TERMS = 0, RESID = 1, STEP = 2 };

struct Box {
  Vec lb, ub, v, dv, zl, zu, t, z;
};

// small integers and powers of two; NaN wherever a kernel must not read
static Box box(size_t L, bool planted) {
  Box b;
  for (Vec* p : {&b.lb, &b.ub, &b.v, &b.dv, &b.zl, &b.zu, &b.t, &b.z}) *p = made(L);
  for (size_t i = 0; i < L; ++i) {
    const int kind = (int)((i * 7 + 3) % 5);
    const double base = (double)((i * 3) % 5) - 2.0, dl = (double)(1 << (i % 3)), du = (double)(1 << ((i / 3) % 3));
    const bool lo = kind == 0 || kind == 1, up = kind == 0 || kind == 2;
    b.lb[i] = (lo || kind == 4) ? base : -INFINITY;
    b.ub[i] = kind == 0 ? base + dl + du : (kind == 2 || kind == 4) ? base : INFINITY;
    b.v[i] = lo ? base + dl : up ? base - du : NAN;
    b.zl[i] = lo ? (double)((i * 5 + 1) % 4 + 1) : NAN;
    b.zu[i] = up ? (double)((i * 3 + 2) % 4 + 1) : NAN;
    b.dv[i] = (lo || up) ? small_vec((int64_t)i) : NAN;
    b.t[i] = small_vec((int64_t)i * 3 + 1);
    b.z[i] = small_vec((int64_t)i + 2);
  }
  if (planted && L >= 5) {
    for (size_t i = 0; i < 5; ++i) { b.lb[i] = -1.0; b.ub[i] = 3.0; b.v[i] = 1.0; b.dv[i] = -3.0; b.zl[i] = 2.0; b.zu[i] = 3.0; }
    b.v[0] = -1.0; b.zl[1] = -2.0; b.zu[2] = INFINITY; b.zl[3] = NAN; b.dv[4] = NAN; b.t[4] = NAN;
  }
  return b;
}

static bool side_ok(double s, double z) { return s > 0.0 && std::isfinite(s) && z >= 0.0 && std::isfinite(z); }

struct Want {
  Vec o1, o2, rec;
};

static Want terms_loop(const Box& b, double mu) {
  const size_t L = b.lb.size();
  Want w{made(L), made(L), {0.0, 0.0, 0.0, INFINITY, 0.0, 0.0, 0.0, INFINITY}};
  for (size_t i = 0; i < L; ++i) {
    const bool boxed = b.lb[i] != b.ub[i], lo = boxed && std::isfinite(b.lb[i]), up = boxed && std::isfinite(b.ub[i]);
    double br[2] = {0.0, 0.0}, mr[2] = {0.0, 0.0};
    for (int s = 0; s < 2; ++s) {
      if (!(s ? up : lo)) continue;
      const double d = s ? b.ub[i] - b.v[i] : b.v[i] - b.lb[i], z = s ? b.zu[i] : b.zl[i];
      if (!side_ok(d, z)) { w.rec[5] += 1.0; continue; }
      br[s] = z / d; mr[s] = mu / d;
      w.rec[0] = std::max(w.rec[0], std::fabs(d * z - mu)); w.rec[1] += d * z; w.rec[2] += 1.0; w.rec[3] = std::min(w.rec[3], d);
      w.rec[4] += std::log(d); w.rec[6] += z; w.rec[7] = std::min(w.rec[7], d * z);
    }
    w.o1[i] = br[0] + br[1];
    w.o2[i] = mr[0] - mr[1];
  }
  return w;
}

static Want resid_loop(const Box& b, bool with_z, bool negate) {
  const size_t L = b.lb.size();
  Want w{made(L), {}, {0.0, 0.0, 0.0, 0.0}};
  for (size_t i = 0; i < L; ++i) {
    double r = 0.0;
    if (b.lb[i] != b.ub[i]) {
      r = with_z ? b.t[i] - b.z[i] : b.t[i];
      if (negate) r = -r;
      if (std::isfinite(r)) { w.rec[0] = std::max(w.rec[0], std::fabs(r)); w.rec[1] += r * r; }
      else w.rec[2] += 1.0;
    }
    w.o1[i] = r;
  }
  return w;
}

static Want step_loop(const Box& b, double mu, double tau) {
  const size_t L = b.lb.size();
  Want w{made(L), made(L), {1.0, 1.0, -1.0, 0.0}};
  for (size_t i = 0; i < L; ++i) {
    const bool boxed = b.lb[i] != b.ub[i], lo = boxed && std::isfinite(b.lb[i]), up = boxed && std::isfinite(b.ub[i]);
    double dz[2] = {0.0, 0.0};
    if ((lo || up) && !std::isfinite(b.dv[i])) w.rec[3] += 1.0;
    else
      for (int s = 0; s < 2; ++s) {
        if (!(s ? up : lo)) continue;
        const double d = s ? b.ub[i] - b.v[i] : b.v[i] - b.lb[i], z = s ? b.zu[i] : b.zl[i], ds = s ? -b.dv[i] : b.dv[i];
        if (!side_ok(d, z)) { w.rec[3] += 1.0; continue; }
        dz[s] = s ? (mu / d - z) + (z / d) * b.dv[i] : (mu / d - z) - (z / d) * b.dv[i];
        if (ds < 0.0 && (tau * d) / (-ds) < w.rec[0]) { w.rec[0] = (tau * d) / (-ds); w.rec[2] = (double)i; }
        if (dz[s] < 0.0) w.rec[1] = std::min(w.rec[1], (tau * z) / (-dz[s]));
      }
    w.o1[i] = dz[0];
    w.o2[i] = dz[1];
  }
  return w;
}

static int raw(int kind, int64_t len, const Box& b, const double* t, const double* z, int negate, double mu, double tau, double* o1,
               double* o2, double* out) {
  return pk_ip_raw_dev(ctx, kind, len, b.lb.data(), b.ub.data(), b.v.data(), b.dv.data(), b.zl.data(), b.zu.data(), t, z, negate, mu, tau, o1,
                       o2, out, nullptr);
}

// the same vector is equal but for signed zeros of a lone bad upper bracket, which the loop writes as 0.0 - 0.0
static bool equal(const Vec& a, const Vec& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (!(a[i] == b[i]) && !(std::isnan(a[i]) && std::isnan(b[i]))) return false;
  return true;
}
// a record against the loop's: column 4 of the terms within the rounding of its tree, the rest equal
static bool record_ok(const Vec& got, const Vec& want, size_t L) {
  for (size_t q = 0; q < want.size(); ++q) {
    if (want.size() == 8 && q == 4) {
      if (!(std::fabs(got[q] - want[q]) <= (double)(2 * L + 2) * 0x1p-52 * 1.5 * (double)(2 * L + 2))) return false;      // |ln d| <= ln 4 < 1.5
    } else if (!(got[q] == want[q])) {
      return false;
    }
  }
  return true;
}

static void check_kernels(size_t L, bool planted) {
  const int64_t N = (int64_t)L;
  const Box b = box(L, planted);
  const double mu = 0.5, tau = 0.5;
  {
    Guarded s(L), r(L), rec(8);
    OK(raw(TERMS, N, b, nullptr, nullptr, 0, mu, tau, s.ptr(), r.ptr(), rec.ptr()));
    OK(pk_sync(ctx, nullptr));
    const Want w = terms_loop(b, mu);
    CHECK(equal(s.fetch(), w.o1) && equal(r.fetch(), w.o2) && record_ok(rec.fetch(), w.rec, L));
    if (planted && L >= 5) CHECK(rec.fetch()[5] == 4.0);
    if (!planted) CHECK(rec.fetch()[5] == 0.0);
  }
  for (int variant = 0; variant < 3; ++variant) {      // 0: no z; 1: z; 2: z, negated, in place
    Guarded r(variant == 2 ? Guarded(b.t) : Guarded(L)), rec(4);
    OK(raw(RESID, N, b, variant == 2 ? r.ptr() : b.t.data(), variant ? b.z.data() : nullptr, variant == 2, mu, tau, r.ptr(), nullptr, rec.ptr()));
    OK(pk_sync(ctx, nullptr));
    const Want w = resid_loop(b, variant != 0, variant == 2);
    CHECK(equal(r.fetch(), w.o1) && record_ok(rec.fetch(), w.rec, L));
    if (planted && L >= 5) CHECK(rec.fetch()[2] == 1.0);
  }
  {
    Guarded dl(L), du(L), rec(4);
    OK(raw(STEP, N, b, nullptr, nullptr, 0, mu, tau, dl.ptr(), du.ptr(), rec.ptr()));
    OK(pk_sync(ctx, nullptr));
    const Want w = step_loop(b, mu, tau);
    CHECK(equal(dl.fetch(), w.o1) && equal(du.fetch(), w.o2) && record_ok(rec.fetch(), w.rec, L));
    if (planted && L >= 5) CHECK(rec.fetch()[3] == 5.0);
  }
}

static void print(const Vec& v) {
  for (double x : v) std::printf("%a\n", x);
}

static int dump(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 3;
  long long L;
  int negate;
  double mu, tau;
  if (std::fscanf(f, "%lld %d %la %la", &L, &negate, &mu, &tau) != 4) return 3;
  Box b;
  for (Vec* p : {&b.lb, &b.ub, &b.v, &b.dv, &b.zl, &b.zu, &b.t, &b.z}) *p = read_doubles(f);
  std::fclose(f);
  load_model();
  set_problem(400, 6, 11, 7);
  const size_t n = (size_t)L;
  Guarded s(n), rb(n), rec8(8), r(n), rec4(4), dl(n), du(n), rec4b(4);
  OK(raw(TERMS, L, b, nullptr, nullptr, 0, mu, tau, s.ptr(), rb.ptr(), rec8.ptr()));
  OK(raw(RESID, L, b, b.t.data(), b.z.data(), negate, mu, tau, r.ptr(), nullptr, rec4.ptr()));
  OK(raw(STEP, L, b, nullptr, nullptr, 0, mu, tau, dl.ptr(), du.ptr(), rec4b.ptr()));
  OK(pk_sync(ctx, nullptr));
  for (const Guarded* g : {&s, &rb, &rec8, &r, &rec4, &dl, &du, &rec4b}) print(g->fetch());
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "--dump")) return dump(argv[2]);
  load_model();
  set_problem(400, 6, 11, 7);

  // ---- the three kernels and the scalar step through the raw form; the partial columns grow from one piece to 257
  for (size_t L : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)2047, (size_t)2048, (size_t)2049, (size_t)524289, (size_t)2049}) {
    check_kernels(L, false);
    check_kernels(L, true);
  }
  {  // the identities of a vector without a side, and a tie of three indices
    Box b = box(600, false);
    for (size_t i = 0; i < 600; ++i) { b.lb[i] = i % 2 ? -INFINITY : 1.0; b.ub[i] = i % 2 ? INFINITY : 1.0; b.v[i] = b.dv[i] = b.zl[i] = b.zu[i] = NAN; }
    Guarded s(600), r(600), rec(8), rec4(4);
    OK(raw(TERMS, 600, b, nullptr, nullptr, 0, 0.5, 0.5, s.ptr(), r.ptr(), rec.ptr()));
    OK(pk_sync(ctx, nullptr));
    CHECK(s.fetch() == Vec(600, 0.0) && r.fetch() == Vec(600, 0.0) && rec.fetch() == Vec({0.0, 0.0, 0.0, INFINITY, 0.0, 0.0, 0.0, INFINITY}));
    Guarded s2(600), r2(600);
    OK(raw(STEP, 600, b, nullptr, nullptr, 0, 0.5, 0.5, s2.ptr(), r2.ptr(), rec4.ptr()));
    OK(pk_sync(ctx, nullptr));
    CHECK(s2.fetch() == Vec(600, 0.0) && r2.fetch() == Vec(600, 0.0) && rec4.fetch() == Vec({1.0, 1.0, -1.0, 0.0}));
    Box t = box(3000, false);
    for (size_t i = 0; i < 3000; ++i) { t.lb[i] = -1.0; t.ub[i] = 3.0; t.v[i] = 1.0; t.dv[i] = 0.0; t.zl[i] = 1.0; t.zu[i] = 1.0; }
    for (size_t i : {(size_t)2900, (size_t)700, (size_t)5}) t.dv[i] = -8.0;
    Guarded a(3000), c(3000), rec4b(4);
    OK(raw(STEP, 3000, t, nullptr, nullptr, 0, 0.5, 0.5, a.ptr(), c.ptr(), rec4b.ptr()));
    OK(pk_sync(ctx, nullptr));
    CHECK(rec4b.fetch()[0] == 0.125 && rec4b.fetch()[2] == 5.0);
  }
  {  // refusals of the raw form: the code, nothing enqueued, nothing written
    const Box b = box(8, false);
    Guarded o(8), rec(8);
    const size_t mark = fake_hip_log().size();
    CHECK(raw(3, 8, b, nullptr, nullptr, 0, 0.5, 0.5, o.ptr(), o.ptr(), rec.ptr()) == 134);
    CHECK(raw(-1, 8, b, nullptr, nullptr, 0, 0.5, 0.5, o.ptr(), o.ptr(), rec.ptr()) == 134);
    CHECK(raw(TERMS, -1, b, nullptr, nullptr, 0, 0.5, 0.5, o.ptr(), o.ptr(), rec.ptr()) == 134);
    CHECK(raw(TERMS, 8, b, nullptr, nullptr, 0, -0.5, 0.5, o.ptr(), o.ptr(), rec.ptr()) == 134);
    CHECK(raw(TERMS, 8, b, nullptr, nullptr, 0, NAN, 0.5, o.ptr(), o.ptr(), rec.ptr()) == 134);
    CHECK(raw(STEP, 8, b, nullptr, nullptr, 0, 0.5, 0.0, o.ptr(), o.ptr(), rec.ptr()) == 134);
    CHECK(raw(STEP, 8, b, nullptr, nullptr, 0, 0.5, 1.5, o.ptr(), o.ptr(), rec.ptr()) == 134);
    CHECK(raw(STEP, 8, b, nullptr, nullptr, 0, 0.5, NAN, o.ptr(), o.ptr(), rec.ptr()) == 134);
    CHECK(raw(TERMS, 8, b, nullptr, nullptr, 0, 0.5, 0.5, nullptr, o.ptr(), rec.ptr()) == 110);
    CHECK(raw(TERMS, 8, b, nullptr, nullptr, 0, 0.5, 0.5, o.ptr(), nullptr, rec.ptr()) == 110);
    CHECK(raw(TERMS, 8, b, nullptr, nullptr, 0, 0.5, 0.5, o.ptr(), o.ptr(), nullptr) == 110);
    CHECK(raw(RESID, 8, b, nullptr, nullptr, 0, 0.5, 0.5, o.ptr(), nullptr, rec.ptr()) == 110);
    CHECK(pk_ip_raw_dev(ctx, STEP, 8, b.lb.data(), b.ub.data(), b.v.data(), nullptr, b.zl.data(), b.zu.data(), nullptr, nullptr, 0, 0.5, 0.5, o.ptr(),
                        o.ptr(), rec.ptr(), nullptr) == 110);
    CHECK(pk_ip_raw_dev(ctx, TERMS, 8, nullptr, b.ub.data(), b.v.data(), nullptr, b.zl.data(), b.zu.data(), nullptr, nullptr, 0, 0.5, 0.5, o.ptr(),
                        o.ptr(), rec.ptr(), nullptr) == 110);
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark);
    for (double v : o.fetch()) CHECK(v == -77.0);
    for (double v : rec.fetch()) CHECK(v == -77.0);
  }

  // ---- the public forms on a problem with bounds, J and J^T: n = 400, m rows
  std::vector<int32_t> lens = {3, 0, 300, 2, 5, 1};
  lens.insert(lens.end(), 290, 2);
  const Csr A = from_lengths(lens, 400);
  const Csr T = transposed(A);
  const int32_t n = 400, m = A.rows;
  set_problem(n, m, A.nnz(), 7);
  const Box bx = box((size_t)n, true), bc = box((size_t)m, false);
  Vec grad = ints((size_t)n, 3), lam = ints((size_t)m, 4), jv((size_t)A.nnz());
  for (size_t e = 0; e < jv.size(); ++e) jv[e] = small_val((int64_t)e);
  const double mu = 0.5, tau = 0.5;
  {  // before the bounds, the operator and the linearization: 123, 117, 118; null pointers, bad arguments, a shard
    Guarded o1((size_t)n), o2((size_t)n), rec(8);
    Vec h1((size_t)n, -3.0), h2((size_t)n, -3.0), hrec(8, -3.0);
    const size_t mark = fake_hip_log().size();
    CHECK(pk_ip_terms_dev(ctx, 0, bx.v.data(), bx.zl.data(), bx.zu.data(), mu, o1.ptr(), o2.ptr(), rec.ptr(), nullptr) == 123);
    CHECK(pk_ip_step_dev(ctx, 0, bx.v.data(), bx.dv.data(), bx.zl.data(), bx.zu.data(), mu, tau, o1.ptr(), o2.ptr(), rec.ptr(), nullptr) == 123);
    CHECK(pk_ip_terms(ctx, 0, bx.v.data(), bx.zl.data(), bx.zu.data(), mu, h1.data(), h2.data(), hrec.data()) == 123);
    CHECK(pk_ip_step(ctx, 1, bc.v.data(), bc.dv.data(), bc.zl.data(), bc.zu.data(), mu, tau, h1.data(), h2.data(), hrec.data()) == 123);
    CHECK(pk_dual_residual_dev(ctx, jv.data(), grad.data(), lam.data(), nullptr, 0, o1.ptr(), rec.ptr(), nullptr) == 117);
    set_identity_map(0, A.nnz());
    OK(set_operator(0, A));
    OK(set_operator(1, T));
    CHECK(pk_dual_residual_dev(ctx, jv.data(), grad.data(), lam.data(), nullptr, 0, o1.ptr(), rec.ptr(), nullptr) == 123);
    CHECK(pk_dual_residual(ctx, grad.data(), lam.data(), nullptr, 0, h1.data(), hrec.data()) == 123);
    OK(pk_set_bounds(ctx, bc.lb.data(), bc.ub.data(), bx.lb.data(), bx.ub.data()));
    const size_t mark2 = fake_hip_log().size();
    CHECK(pk_dual_residual(ctx, grad.data(), lam.data(), nullptr, 0, h1.data(), hrec.data()) == 118);
    CHECK(pk_dual_residual(ctx, nullptr, lam.data(), nullptr, 0, h1.data(), hrec.data()) == 60);
    CHECK(pk_dual_residual(ctx, grad.data(), lam.data(), nullptr, 0, nullptr, hrec.data()) == 60);
    CHECK(pk_ip_terms(ctx, 0, nullptr, bx.zl.data(), bx.zu.data(), mu, h1.data(), h2.data(), hrec.data()) == 60);
    CHECK(pk_ip_terms(ctx, 0, bx.v.data(), bx.zl.data(), bx.zu.data(), mu, h1.data(), h2.data(), nullptr) == 60);
    CHECK(pk_ip_step(ctx, 0, bx.v.data(), nullptr, bx.zl.data(), bx.zu.data(), mu, tau, h1.data(), h2.data(), hrec.data()) == 60);
    CHECK(pk_ip_terms(ctx, 2, bx.v.data(), bx.zl.data(), bx.zu.data(), mu, h1.data(), h2.data(), hrec.data()) == 134);
    CHECK(pk_ip_terms(ctx, -1, bx.v.data(), bx.zl.data(), bx.zu.data(), mu, h1.data(), h2.data(), hrec.data()) == 134);
    CHECK(pk_ip_terms(ctx, 0, bx.v.data(), bx.zl.data(), bx.zu.data(), -1.0, h1.data(), h2.data(), hrec.data()) == 134);
    CHECK(pk_ip_step(ctx, 0, bx.v.data(), bx.dv.data(), bx.zl.data(), bx.zu.data(), mu, 0.0, h1.data(), h2.data(), hrec.data()) == 134);
    CHECK(pk_ip_step(ctx, 0, bx.v.data(), bx.dv.data(), bx.zl.data(), bx.zu.data(), INFINITY, tau, h1.data(), h2.data(), hrec.data()) == 134);
    CHECK(pk_ip_terms_dev(ctx, 0, nullptr, bx.zl.data(), bx.zu.data(), mu, o1.ptr(), o2.ptr(), rec.ptr(), nullptr) == 110);
    CHECK(pk_ip_terms_dev(ctx, 0, bx.v.data(), bx.zl.data(), bx.zu.data(), mu, o1.ptr(), o2.ptr(), nullptr, nullptr) == 110);
    CHECK(pk_ip_terms_dev(ctx, 5, bx.v.data(), bx.zl.data(), bx.zu.data(), mu, o1.ptr(), o2.ptr(), rec.ptr(), nullptr) == 134);
    CHECK(pk_ip_terms_dev(ctx, 0, bx.v.data(), bx.zl.data(), bx.zu.data(), NAN, o1.ptr(), o2.ptr(), rec.ptr(), nullptr) == 134);
    CHECK(pk_ip_step_dev(ctx, 0, bx.v.data(), bx.dv.data(), bx.zl.data(), bx.zu.data(), mu, tau, o1.ptr(), nullptr, rec.ptr(), nullptr) == 110);
    CHECK(pk_ip_step_dev(ctx, 0, bx.v.data(), bx.dv.data(), bx.zl.data(), bx.zu.data(), mu, -0.5, o1.ptr(), o2.ptr(), rec.ptr(), nullptr) == 134);
    CHECK(pk_ip_step_dev(ctx, 0, bx.v.data(), bx.dv.data(), bx.zl.data(), bx.zu.data(), -mu, tau, o1.ptr(), o2.ptr(), rec.ptr(), nullptr) == 134);
    CHECK(pk_dual_residual_dev(ctx, nullptr, grad.data(), lam.data(), nullptr, 0, o1.ptr(), rec.ptr(), nullptr) == 110);
    CHECK(pk_dual_residual_dev(ctx, jv.data(), grad.data(), lam.data(), nullptr, 0, nullptr, rec.ptr(), nullptr) == 110);
    CHECK(pk_dual_residual_dev(ctx, jv.data(), grad.data(), lam.data(), nullptr, 0, o1.ptr(), nullptr, nullptr) == 110);
    OK(pk_set_shard(ctx, 1, 0, nullptr));                                        // a shard is refused
    CHECK(pk_ip_terms_dev(ctx, 0, bx.v.data(), bx.zl.data(), bx.zu.data(), mu, o1.ptr(), o2.ptr(), rec.ptr(), nullptr) == 119);
    CHECK(pk_ip_step_dev(ctx, 0, bx.v.data(), bx.dv.data(), bx.zl.data(), bx.zu.data(), mu, tau, o1.ptr(), o2.ptr(), rec.ptr(), nullptr) == 119);
    CHECK(pk_dual_residual_dev(ctx, jv.data(), grad.data(), lam.data(), nullptr, 0, o1.ptr(), rec.ptr(), nullptr) == 119);
    CHECK(pk_ip_terms(ctx, 0, bx.v.data(), bx.zl.data(), bx.zu.data(), mu, h1.data(), h2.data(), hrec.data()) == 119);
    OK(pk_set_shard(ctx, 0, 0, nullptr));
    OK(pk_sync(ctx, nullptr));
    CHECK(mark2 >= mark && fake_hip_log().size() == mark2);
    for (const Guarded* g : {&o1, &o2, &rec}) for (double v : g->fetch()) CHECK(v == -77.0);
    for (const Vec* h : {&h1, &h2, &hrec}) for (double v : *h) CHECK(v == -3.0);
  }
  for (int which = 0; which < 2; ++which) {      // the device forms on the context's bounds against the raw form, the host forms against both
    const Box& b = which ? bc : bx;
    const size_t L = b.lb.size();
    Guarded s(L), r(L), rec(8), s2(L), r2(L), rec2(8), hs(L), hr(L), hrec(8);
    OK(pk_ip_terms_dev(ctx, which, b.v.data(), b.zl.data(), b.zu.data(), mu, s.ptr(), r.ptr(), rec.ptr(), nullptr));
    OK(raw(TERMS, (int64_t)L, b, nullptr, nullptr, 0, mu, tau, s2.ptr(), r2.ptr(), rec2.ptr()));
    OK(pk_ip_terms(ctx, which, b.v.data(), b.zl.data(), b.zu.data(), mu, hs.ptr(), hr.ptr(), hrec.ptr()));
    CHECK(same_bits(s.fetch(), s2.fetch()) && same_bits(r.fetch(), r2.fetch()) && same_bits(rec.fetch(), rec2.fetch()));
    CHECK(same_bits(s.fetch(), hs.fetch()) && same_bits(r.fetch(), hr.fetch()) && same_bits(rec.fetch(), hrec.fetch()));
    CHECK(rec.fetch()[5] == (which ? 0.0 : 4.0));
    Guarded d(L), u(L), rec4(4), d2(L), u2(L), rec42(4), hd(L), hu(L), hrec4(4);
    OK(pk_ip_step_dev(ctx, which, b.v.data(), b.dv.data(), b.zl.data(), b.zu.data(), mu, tau, d.ptr(), u.ptr(), rec4.ptr(), nullptr));
    OK(raw(STEP, (int64_t)L, b, nullptr, nullptr, 0, mu, tau, d2.ptr(), u2.ptr(), rec42.ptr()));
    OK(pk_ip_step(ctx, which, b.v.data(), b.dv.data(), b.zl.data(), b.zu.data(), mu, tau, hd.ptr(), hu.ptr(), hrec4.ptr()));
    CHECK(same_bits(d.fetch(), d2.fetch()) && same_bits(u.fetch(), u2.fetch()) && same_bits(rec4.fetch(), rec42.fetch()));
    CHECK(same_bits(d.fetch(), hd.fetch()) && same_bits(u.fetch(), hu.fetch()) && same_bits(rec4.fetch(), hrec4.fetch()));
  }
  {  // the dual residual: J^T lam + grad by the operator, then the kernel; the host form on pk_linearize's values
    Vec x((size_t)n);
    for (int i = 0; i < n; ++i) x[(size_t)i] = 2.0 * (double)(i % 9 - 4);
    Guarded t((size_t)n);
    OK(pk_apply_operator_dev(ctx, 1, jv.data(), lam.data(), grad.data(), t.ptr(), nullptr));
    OK(pk_sync(ctx, nullptr));
    Box b = bx;
    b.t = t.fetch();
    for (int variant = 0; variant < 3; ++variant) {
      Guarded r((size_t)n), rec(4);
      OK(pk_dual_residual_dev(ctx, jv.data(), grad.data(), lam.data(), variant ? b.z.data() : nullptr, variant == 2, r.ptr(), rec.ptr(), nullptr));
      OK(pk_sync(ctx, nullptr));
      const Want w = resid_loop(b, variant != 0, variant == 2);
      CHECK(equal(r.fetch(), w.o1) && record_ok(rec.fetch(), w.rec, (size_t)n));
    }
    OK(pk_linearize(ctx, x.data(), nullptr, 1.0));
    Vec lj((size_t)A.nnz());
    for (int64_t e = 0; e < A.nnz(); ++e) lj[(size_t)e] = fake_jac(x.data(), n, e, false);
    Guarded r((size_t)n), rec(4), hr((size_t)n), hrec(4);
    OK(pk_dual_residual_dev(ctx, lj.data(), grad.data(), lam.data(), b.z.data(), 1, r.ptr(), rec.ptr(), nullptr));
    OK(pk_dual_residual(ctx, grad.data(), lam.data(), b.z.data(), 1, hr.ptr(), hrec.ptr()));
    CHECK(same_bits(r.fetch(), hr.fetch()) && same_bits(rec.fetch(), hrec.fetch()) && hrec.fetch()[3] == 0.0);
  }

  // ---- what frees the state: a new problem forgets the bounds, and pk_destroy leaves no live allocation
  CHECK(fake_hip_live_allocations() > 0);
  set_problem(400, 6, 11, 7);
  {
    Guarded o1(400), o2(400), rec(8);
    CHECK(pk_ip_terms_dev(ctx, 0, bx.v.data(), bx.zl.data(), bx.zu.data(), mu, o1.ptr(), o2.ptr(), rec.ptr(), nullptr) == 123);
  }
  check_kernels(2049, true);                                                   // (allocated again on first use)
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return checks_passed();
}
