// slack_driver.cpp -- TEST INFRASTRUCTURE: drives the entry points of pockit_amd/csrc/pk_slack.cpp (slack elimination, slack step
// with the curvature terms, iterate update with the multiplier safeguard, merit terms of trial points with slacks) against the
// host-only HIP stand-in of this directory, built with -fsanitize=address,undefined (tests/test_slack_cpu.py): the stand-in walk
// of every kernel against plain loops on small integers and powers of two (every product, quotient and sum but the logarithms'
// is exact in fp64 or a single rounding, so a result must EQUAL the loop; the sum of logarithms is held to a bound), clean and
// with planted defects, batches of 1, 3 and 64 trial points, the public forms against the raw form and the host forms against
// the device forms, every refusal with its code and nothing enqueued or written behind it, sentinels around every output, and
// tear-down without a live allocation.  With --dump FILE: the vectors FILE describes (tests/test_slack_cpu.py writes them from
// tests/slack_cases.py) through the raw form, every vector and record printed as hex doubles.
#include <cmath>
#include <cstring>

#include "driver_common.h"

enum { REDUCE = 0, RECOVER = 1, UPDATE = 2, MERIT = 3 };

struct Rows {
  Vec lb, ub, g, s, lam, dlam, sig, rbar, s2, ds, dv, zl, zu, dzl, dzu;
};
struct Vars {
  Vec lb, ub, x, dx, w, s1;
};

static bool positive(double d) { return d > 0.0 && std::isfinite(d); }

// small integers and powers of two; NaN wherever a kernel must not read
static Rows rows(size_t m, bool planted) {
  Rows b;
  for (Vec* p : {&b.lb, &b.ub, &b.g, &b.s, &b.lam, &b.dlam, &b.sig, &b.rbar, &b.s2, &b.ds, &b.dv, &b.zl, &b.zu, &b.dzl, &b.dzu}) *p = made(m);
  for (size_t i = 0; i < m; ++i) {
    const int kind = (int)((i * 7 + 3) % 5);      // 0 both sides, 1 lower, 2 upper, 3 a free slack, 4 an equality row
    const double base = (double)((i * 3) % 5) - 2.0, dl = (double)(1 << (i % 3)), du = (double)(1 << ((i / 3) % 3));
    const bool lo = kind == 0 || kind == 1, up = kind == 0 || kind == 2, eq = kind == 4;
    b.lb[i] = (lo || eq) ? base : -INFINITY;
    b.ub[i] = kind == 0 ? base + dl + du : (kind == 2 || eq) ? base : INFINITY;
    b.s[i] = eq ? NAN : lo ? base + dl : up ? base - du : small_vec((int64_t)i);
    b.g[i] = (eq ? base : b.s[i]) + small_vec((int64_t)i * 5 + 2);
    b.lam[i] = small_vec((int64_t)i * 3 + 1);
    b.dlam[i] = small_vec((int64_t)i + 4);
    b.sig[i] = eq ? NAN : (double)(1 << ((i / 5) % 3));
    b.rbar[i] = eq ? NAN : small_vec((int64_t)i * 2 + 3);
    b.s2[i] = eq ? NAN : 1.0 / b.sig[i];
    b.ds[i] = eq ? NAN : 0.125 * (double)((int)(i % 3) - 1);
    b.dv[i] = eq ? NAN : 0.5 * (double)((int)(i % 3) - 1);
    b.zl[i] = lo ? (double)((i * 5 + 1) % 4 + 1) : NAN;
    b.zu[i] = up ? (double)((i * 3 + 2) % 4 + 1) : NAN;
    b.dzl[i] = lo ? small_vec((int64_t)i + 1) : NAN;
    b.dzu[i] = up ? small_vec((int64_t)i + 6) : NAN;
  }
  if (planted && m >= 8) {
    for (size_t i = 0; i < 8; ++i) {
      b.lb[i] = -1.0; b.ub[i] = 3.0; b.s[i] = 1.0; b.g[i] = 2.0; b.sig[i] = 2.0; b.s2[i] = 0.5; b.rbar[i] = 1.0; b.ds[i] = 0.25; b.dv[i] = 0.5;
      b.zl[i] = 2.0; b.zu[i] = 3.0; b.dzl[i] = 1.0; b.dzu[i] = -1.0;
    }
    b.sig[0] = 0.0; b.sig[1] = INFINITY; b.sig[2] = NAN; b.g[3] = NAN;      // reduce, recover: three bad sigma_s; reduce, merit: a residual
    b.dv[4] = NAN; b.dv[5] = 16.0; b.dzl[6] = INFINITY; b.ds[7] = 64.0;     // update: a NaN step, across the bound, a multiplier; merit: a slack
  }
  return b;
}

static Vars vars(size_t n, bool planted) {
  Vars v;
  for (Vec* p : {&v.lb, &v.ub, &v.x, &v.dx, &v.w, &v.s1}) *p = made(n);
  for (size_t i = 0; i < n; ++i) {
    const int kind = (int)((i * 3 + 1) % 5);
    const double base = (double)((i * 2) % 5) - 2.0, dl = (double)(1 << (i % 3)), du = (double)(1 << ((i / 3) % 3));
    const bool lo = kind == 0 || kind == 1, up = kind == 0 || kind == 2, fixed = kind == 4;
    v.lb[i] = (lo || fixed) ? base : -INFINITY;
    v.ub[i] = kind == 0 ? base + dl + du : (kind == 2 || fixed) ? base : INFINITY;
    v.x[i] = lo ? base + dl : up ? base - du : NAN;
    v.dx[i] = fixed ? NAN : small_vec((int64_t)i);
    v.w[i] = fixed ? NAN : small_vec((int64_t)i * 3 + 2);
    v.s1[i] = fixed ? NAN : (double)(i % 4);
  }
  if (planted && n >= 3) {
    for (size_t i = 0; i < 3; ++i) { v.lb[i] = -1.0; v.ub[i] = 3.0; v.x[i] = 1.0; v.dx[i] = 1.0; v.w[i] = 1.0; v.s1[i] = 1.0; }
    v.w[1] = INFINITY;      // recover: a term that is not finite
    v.x[2] = -1.0;          // merit: a zero slack
  }
  return v;
}

// ---------------------------------------------------------------- the plain loops
struct Want {
  Vec o1, o2, o3, o4, rec;
};

static Want reduce_loop(const Rows& b) {
  const size_t m = b.lb.size();
  Want w{made(m), made(m), {}, {}, {0.0, 0.0, 0.0, 0.0}};
  for (size_t i = 0; i < m; ++i) {
    double s2 = 0.0, b2 = 0.0, r = NAN;
    if (b.lb[i] == b.ub[i]) {
      r = b.g[i] - b.lb[i];
      b2 = -r;
    } else {
      w.rec[3] += 1.0;
      if (positive(b.sig[i])) {
        s2 = 1.0 / b.sig[i];
        r = b.g[i] - b.s[i];
        b2 = -r + s2 * (b.lam[i] + b.rbar[i]);
      }
    }
    if (std::isfinite(r)) { w.rec[0] = std::max(w.rec[0], std::fabs(r)); w.rec[1] += std::fabs(r); }
    else w.rec[2] += 1.0;
    w.o1[i] = s2; w.o2[i] = b2;
  }
  return w;
}

static Want recover_loop(const Vars& v, const Rows& b) {
  const size_t n = v.lb.size(), m = b.lb.size();
  Want w{made(m), {}, {}, {}, {0.0, 0.0, 0.0, 0.0, 0.0}};
  for (size_t i = 0; i < n; ++i) {
    if (v.lb[i] == v.ub[i]) continue;
    const double term = v.dx[i] * v.w[i] + v.s1[i] * (v.dx[i] * v.dx[i]);
    if (std::isfinite(term)) { w.rec[0] += term; w.rec[2] += v.dx[i] * v.dx[i]; }
    else w.rec[4] += 1.0;
  }
  for (size_t i = 0; i < m; ++i) {
    double ds = 0.0;
    if (b.lb[i] != b.ub[i]) {
      if (positive(b.sig[i])) ds = b.s2[i] * ((b.dlam[i] + b.lam[i]) + b.rbar[i]);
      if (positive(b.sig[i]) && std::isfinite(ds)) { w.rec[1] += b.sig[i] * (ds * ds); w.rec[3] += ds * ds; }
      else w.rec[4] += 1.0;
    }
    w.o1[i] = ds;
  }
  return w;
}

static Want update_loop(const Rows& b, bool with_lam, double ap, double ad, double mu, double kappa) {
  const size_t m = b.lb.size();
  Want w{b.s, b.zl, b.zu, b.lam, {0.0, INFINITY, 0.0, 0.0}};
  for (size_t i = 0; i < m; ++i) {
    if (with_lam) {
      w.o4[i] = b.lam[i] + ap * b.dlam[i];
      if (!std::isfinite(w.o4[i])) w.rec[2] += 1.0;
    }
    if (b.lb[i] == b.ub[i]) continue;
    const double vn = b.s[i] + ap * b.dv[i];
    w.o1[i] = vn;
    if (!std::isfinite(vn)) w.rec[2] += 1.0;
    for (int side = 0; side < 2; ++side) {
      if (!std::isfinite(side ? b.ub[i] : b.lb[i])) continue;
      const double d = side ? b.ub[i] - vn : vn - b.lb[i], zn = side ? b.zu[i] + ad * b.dzu[i] : b.zl[i] + ad * b.dzl[i];
      double z = zn;
      if (std::isfinite(vn)) {
        if (!positive(d) || !std::isfinite(zn)) {
          w.rec[2] += 1.0;
        } else {
          z = std::min(std::max(zn, mu / (kappa * d)), (kappa * mu) / d);
          if (z != zn) w.rec[0] += 1.0;
          w.rec[1] = std::min(w.rec[1], d);
        }
      }
      (side ? w.o3 : w.o2)[i] = z;
    }
  }
  return w;
}

// the record of entry e; sum_abs_log: what the bound of column 2 scales with
static Vec merit_loop(const Vars& v, const Rows& b, const Vec& X, const Vec& G, double alpha, size_t e, double& sum_abs_log) {
  const size_t n = v.lb.size(), m = b.lb.size();
  Vec rec = {0.0, 0.0, 0.0, 0.0};
  sum_abs_log = 0.0;
  auto side = [&](double d) {
    if (positive(d)) { rec[2] += std::log(d); sum_abs_log += std::fabs(std::log(d)); }
    else rec[3] += 1.0;
  };
  for (size_t i = 0; i < n; ++i) {
    if (v.lb[i] == v.ub[i]) continue;
    if (std::isfinite(v.lb[i])) side(X[e * n + i] - v.lb[i]);
    if (std::isfinite(v.ub[i])) side(v.ub[i] - X[e * n + i]);
  }
  for (size_t i = 0; i < m; ++i) {
    const bool eq = b.lb[i] == b.ub[i];
    const double st = eq ? 0.0 : b.s[i] + alpha * b.ds[i], r = eq ? G[e * m + i] - b.lb[i] : G[e * m + i] - st;
    if (std::isfinite(r)) { rec[0] += std::fabs(r); rec[1] = std::max(rec[1], std::fabs(r)); }
    else rec[3] += 1.0;
    if (eq) continue;
    if (std::isfinite(b.lb[i])) side(st - b.lb[i]);
    if (std::isfinite(b.ub[i])) side(b.ub[i] - st);
  }
  return rec;
}

// ---------------------------------------------------------------- the raw form
static double* in(const Vec& v) { return const_cast<double*>(v.data()); }

static int raw(int kind, int64_t n, int64_t m, int64_t batch, const Vars* v, const Rows& b, std::vector<double*> p, double ap, double ad, double mu,
               double kappa, double* out) {
  p.resize(10, nullptr);
  return pk_slack_raw_dev(ctx, kind, n, m, batch, v ? v->lb.data() : nullptr, v ? v->ub.data() : nullptr, b.lb.data(), b.ub.data(), p.data(), ap,
                          ad, mu, kappa, out, nullptr);
}

// equal, a NaN for a NaN
static bool equal(const Vec& a, const Vec& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (!(a[i] == b[i]) && !(std::isnan(a[i]) && std::isnan(b[i]))) return false;
  return true;
}

static const double AP = 0.5, AD = 0.25, MU = 0.5, KAPPA = 4.0;

static Vec trial_x(const Vars& v, size_t batch) {
  const size_t n = v.lb.size();
  Vec X = made(batch * n);
  for (size_t e = 0; e < batch; ++e)
    for (size_t i = 0; i < n; ++i) X[e * n + i] = v.x[i];      // (NaN where the element has no side)
  return X;
}
static Vec trial_g(const Rows& b, size_t batch) {
  const size_t m = b.lb.size();
  Vec G = made(batch * m);
  for (size_t e = 0; e < batch; ++e)
    for (size_t i = 0; i < m; ++i) G[e * m + i] = b.g[i] + (double)(e % 3);
  return G;
}

static void check_merit(const Vars& v, const Rows& b, size_t batch) {
  const size_t n = v.lb.size(), m = b.lb.size();
  const Vec X = trial_x(v, batch), G = trial_g(b, batch);
  Vec alphas = made(batch);
  for (size_t e = 0; e < batch; ++e) alphas[e] = 1.0 / (double)(1 << (e % 4));
  Guarded out(4 * batch);
  OK(raw(MERIT, (int64_t)n, (int64_t)m, (int64_t)batch, &v, b, {in(X), in(G), in(b.s), in(b.ds), in(alphas)}, AP, AD, MU, KAPPA, out.ptr()));
  OK(pk_sync(ctx, nullptr));
  const Vec got = out.fetch();
  for (size_t e = 0; e < batch; ++e) {
    double scale = 0.0;
    const Vec want = merit_loop(v, b, X, G, alphas[e], e, scale);
    CHECK(got[4 * e] == want[0] && got[4 * e + 1] == want[1] && got[4 * e + 3] == want[3]);
    CHECK(std::fabs(got[4 * e + 2] - want[2]) <= (double)(n + m + 2) * 0x1p-52 * scale);
  }
}

static void check_kernels(size_t n, size_t m, bool planted) {
  const Rows b = rows(m, planted);
  const Vars v = vars(n, planted);
  {
    Guarded s2(m), b2(m), rec(4);
    OK(raw(REDUCE, 0, (int64_t)m, 1, nullptr, b, {in(b.g), in(b.s), in(b.lam), in(b.sig), in(b.rbar), s2.ptr(), b2.ptr()}, AP, AD, MU, KAPPA, rec.ptr()));
    OK(pk_sync(ctx, nullptr));
    const Want w = reduce_loop(b);
    CHECK(equal(s2.fetch(), w.o1) && equal(b2.fetch(), w.o2) && rec.fetch() == w.rec);
    CHECK(rec.fetch()[2] == (planted && m >= 8 ? 4.0 : 0.0));
  }
  {
    Guarded ds(m), rec(5);
    OK(raw(RECOVER, (int64_t)n, (int64_t)m, 1, &v, b,
           {in(b.dlam), in(b.lam), in(b.rbar), in(b.s2), in(b.sig), in(v.dx), in(v.w), in(v.s1), ds.ptr()}, AP, AD, MU, KAPPA, rec.ptr()));
    OK(pk_sync(ctx, nullptr));
    const Want w = recover_loop(v, b);
    CHECK(equal(ds.fetch(), w.o1) && rec.fetch() == w.rec);
    CHECK(rec.fetch()[4] == (planted && m >= 8 ? 3.0 : 0.0) + (planted && n >= 3 ? 1.0 : 0.0));
  }
  for (int with_lam = 0; with_lam < 2; ++with_lam) {
    Guarded s(b.s), zl(b.zl), zu(b.zu), lam(b.lam), rec(4);
    OK(raw(UPDATE, 0, (int64_t)m, 1, nullptr, b,
           {s.ptr(), in(b.dv), zl.ptr(), in(b.dzl), zu.ptr(), in(b.dzu), with_lam ? lam.ptr() : nullptr, with_lam ? in(b.dlam) : nullptr}, AP, AD, MU,
           KAPPA, rec.ptr()));
    OK(pk_sync(ctx, nullptr));
    const Want w = update_loop(b, with_lam != 0, AP, AD, MU, KAPPA);
    CHECK(equal(s.fetch(), w.o1) && equal(zl.fetch(), w.o2) && equal(zu.fetch(), w.o3) && equal(lam.fetch(), w.o4) && rec.fetch() == w.rec);
    if (planted && m >= 8) CHECK(rec.fetch()[2] == 3.0);      // the NaN step once, the upper side of the step across the bound, the multiplier
  }
  check_merit(v, b, 1);
}

static void print(const Vec& v) {
  for (double x : v) std::printf("%a\n", x);
}

// FILE: "n m batch alpha_p alpha_d mu kappa", then xlb xub clb cub, the rows' g s lam dlam sigma_s rbar_s s2 ds dv zl zu dzl dzu,
// the variables' dx w s1, X G alphas
static int dump(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 3;
  long long n, m, batch;
  double ap, ad, mu, kappa;
  if (std::fscanf(f, "%lld %lld %lld %la %la %la %la", &n, &m, &batch, &ap, &ad, &mu, &kappa) != 7) return 3;
  Vars v;
  Rows b;
  v.lb = read_doubles(f); v.ub = read_doubles(f); b.lb = read_doubles(f); b.ub = read_doubles(f);
  for (Vec* p : {&b.g, &b.s, &b.lam, &b.dlam, &b.sig, &b.rbar, &b.s2, &b.ds, &b.dv, &b.zl, &b.zu, &b.dzl, &b.dzu, &v.dx, &v.w, &v.s1}) *p = read_doubles(f);
  const Vec X = read_doubles(f), G = read_doubles(f), alphas = read_doubles(f);
  std::fclose(f);
  load_model();
  set_problem(400, 6, 11, 7);
  const size_t M = (size_t)m;
  Guarded s2(M), b2(M), rec4(4), ds(M), rec5(5), s(b.s), zl(b.zl), zu(b.zu), lam(b.lam), rec4b(4), table(4 * (size_t)batch);
  OK(raw(REDUCE, 0, m, 1, nullptr, b, {in(b.g), in(b.s), in(b.lam), in(b.sig), in(b.rbar), s2.ptr(), b2.ptr()}, ap, ad, mu, kappa, rec4.ptr()));
  OK(raw(RECOVER, n, m, 1, &v, b, {in(b.dlam), in(b.lam), in(b.rbar), in(b.s2), in(b.sig), in(v.dx), in(v.w), in(v.s1), ds.ptr()}, ap, ad, mu, kappa,
         rec5.ptr()));
  OK(raw(UPDATE, 0, m, 1, nullptr, b, {s.ptr(), in(b.dv), zl.ptr(), in(b.dzl), zu.ptr(), in(b.dzu), lam.ptr(), in(b.dlam)}, ap, ad, mu, kappa,
         rec4b.ptr()));
  OK(raw(MERIT, n, m, batch, &v, b, {in(X), in(G), in(b.s), in(b.ds), in(alphas)}, ap, ad, mu, kappa, table.ptr()));
  OK(pk_sync(ctx, nullptr));
  for (const Guarded* g : {&s2, &b2, &rec4, &ds, &rec5, &s, &zl, &zu, &lam, &rec4b, &table}) print(g->fetch());
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "--dump")) return dump(argv[2]);
  load_model();
  set_problem(400, 6, 11, 7);

  // ---- the four kernels and the scalar step through the raw form; the partial columns grow from one piece to 257 and more
  for (size_t L : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)2047, (size_t)2048, (size_t)2049, (size_t)524289, (size_t)2049}) {
    const size_t n = L == 524289 ? 2049 : L;      // (the two-range kinds: 2 + 257 pieces there)
    check_kernels(n, L, false);
    check_kernels(n, L, true);
  }
  check_kernels(524289, 300, false);
  check_kernels(0, 300, true);
  check_kernels(300, 0, true);
  for (size_t batch : {(size_t)1, (size_t)3, (size_t)64}) {
    check_merit(vars(2500, false), rows(4500, false), batch);
    check_merit(vars(2500, true), rows(4500, true), batch);
  }
  {  // alpha = 0 leaves every bit; an already clamped multiplier is left as it is
    const Rows b = rows(3000, false);
    Guarded s(b.s), zl(b.zl), zu(b.zu), lam(b.lam), rec(4);
    OK(raw(UPDATE, 0, 3000, 1, nullptr, b, {s.ptr(), in(b.dv), zl.ptr(), in(b.dzl), zu.ptr(), in(b.dzu), lam.ptr(), in(b.dlam)}, 0.0, 0.0, MU, 1e10,
           rec.ptr()));
    OK(pk_sync(ctx, nullptr));
    CHECK(equal(s.fetch(), b.s) && equal(zl.fetch(), b.zl) && equal(zu.fetch(), b.zu) && equal(lam.fetch(), b.lam) && rec.fetch()[0] == 0.0);
    Rows c = rows(3000, false);
    for (size_t i = 0; i < 3000; ++i) { c.zl[i] *= 1024.0; c.zu[i] /= 1024.0; }
    Guarded s1(c.s), zl1(c.zl), zu1(c.zu), rec1(4);
    OK(raw(UPDATE, 0, 3000, 1, nullptr, c, {s1.ptr(), in(c.dv), zl1.ptr(), in(c.dzl), zu1.ptr(), in(c.dzu)}, 0.0, 0.0, MU, 2.0, rec1.ptr()));
    OK(pk_sync(ctx, nullptr));
    CHECK(rec1.fetch()[0] > 1000.0);
    Rows d = c;
    d.zl = zl1.fetch(); d.zu = zu1.fetch();
    Guarded s3(d.s), zl3(d.zl), zu3(d.zu), rec3(4);
    OK(raw(UPDATE, 0, 3000, 1, nullptr, d, {s3.ptr(), in(d.dv), zl3.ptr(), in(d.dzl), zu3.ptr(), in(d.dzu)}, 0.0, 0.0, MU, 2.0, rec3.ptr()));
    OK(pk_sync(ctx, nullptr));
    CHECK(rec3.fetch()[0] == 0.0 && equal(zl3.fetch(), d.zl) && equal(zu3.fetch(), d.zu));
  }
  {  // refusals of the raw form: the code, nothing enqueued, nothing written
    const Rows b = rows(8, false);
    const Vars v = vars(8, false);
    Guarded o(8), o2(8), rec(8);
    const std::vector<double*> red = {in(b.g), in(b.s), in(b.lam), in(b.sig), in(b.rbar), o.ptr(), o2.ptr()};
    const std::vector<double*> upd = {o.ptr(), in(b.dv), o2.ptr(), in(b.dzl), o2.ptr(), in(b.dzu)};
    const size_t mark = fake_hip_log().size();
    CHECK(raw(4, 8, 8, 1, &v, b, red, AP, AD, MU, KAPPA, rec.ptr()) == 134);
    CHECK(raw(-1, 8, 8, 1, &v, b, red, AP, AD, MU, KAPPA, rec.ptr()) == 134);
    CHECK(raw(REDUCE, 8, -1, 1, &v, b, red, AP, AD, MU, KAPPA, rec.ptr()) == 134);
    CHECK(raw(REDUCE, -1, 8, 1, &v, b, red, AP, AD, MU, KAPPA, rec.ptr()) == 134);
    CHECK(raw(REDUCE, 8, 8, 1, &v, b, red, AP, AD, MU, KAPPA, nullptr) == 110);
    for (size_t k = 0; k < 7; ++k) {
      std::vector<double*> p = red;
      p[k] = nullptr;
      CHECK(raw(REDUCE, 8, 8, 1, &v, b, p, AP, AD, MU, KAPPA, rec.ptr()) == 110);
    }
    CHECK(raw(RECOVER, 8, 8, 1, nullptr, b, {in(b.dlam), in(b.lam), in(b.rbar), in(b.s2), in(b.sig), in(v.dx), in(v.w), in(v.s1), o.ptr()}, AP, AD, MU,
              KAPPA, rec.ptr()) == 110);
    CHECK(raw(RECOVER, 8, 8, 1, &v, b, {in(b.dlam), in(b.lam), in(b.rbar), in(b.s2), in(b.sig), in(v.dx), in(v.w), in(v.s1), nullptr}, AP, AD, MU,
              KAPPA, rec.ptr()) == 110);
    CHECK(pk_slack_raw_dev(ctx, REDUCE, 8, 8, 1, nullptr, nullptr, b.lb.data(), b.ub.data(), nullptr, AP, AD, MU, KAPPA, rec.ptr(), nullptr) == 110);
    for (double bad : {-0.25, 1.5, (double)NAN}) {
      CHECK(raw(UPDATE, 0, 8, 1, nullptr, b, upd, bad, AD, MU, KAPPA, rec.ptr()) == 134);
      CHECK(raw(UPDATE, 0, 8, 1, nullptr, b, upd, AP, bad, MU, KAPPA, rec.ptr()) == 134);
    }
    CHECK(raw(UPDATE, 0, 8, 1, nullptr, b, upd, AP, AD, -1.0, KAPPA, rec.ptr()) == 134);
    CHECK(raw(UPDATE, 0, 8, 1, nullptr, b, upd, AP, AD, INFINITY, KAPPA, rec.ptr()) == 134);
    CHECK(raw(UPDATE, 0, 8, 1, nullptr, b, upd, AP, AD, MU, 0.5, rec.ptr()) == 134);
    CHECK(raw(UPDATE, 0, 8, 1, nullptr, b, upd, AP, AD, MU, NAN, rec.ptr()) == 134);
    {
      std::vector<double*> p = upd;
      p.resize(8, nullptr);
      p[6] = o.ptr();                                  // lam without dlam
      CHECK(raw(UPDATE, 0, 8, 1, nullptr, b, p, AP, AD, MU, KAPPA, rec.ptr()) == 110);
    }
    const Vec X = trial_x(v, 1), G = trial_g(b, 1), alphas = {1.0};
    CHECK(raw(MERIT, 8, 8, 0, &v, b, {in(X), in(G), in(b.s), in(b.ds), in(alphas)}, AP, AD, MU, KAPPA, rec.ptr()) == 134);
    CHECK(raw(MERIT, 8, 8, 1, &v, b, {in(X), in(G), in(b.s), in(b.ds), nullptr}, AP, AD, MU, KAPPA, rec.ptr()) == 110);
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark);
    for (const Guarded* g : {&o, &o2, &rec}) for (double x : g->fetch()) CHECK(x == -77.0);
  }

  // ---- the public forms on a problem with bounds: n = 400 variables, m = 296 rows
  const int32_t n = 400, m = 296;
  set_problem(n, m, 11, 7);
  const Rows b = rows((size_t)m, true);
  const Vars v = vars((size_t)n, true);
  const Rows bx = rows((size_t)n, false);      // (a boxed vector of the variables' length for which = 0)
  {  // before the bounds: 123; null pointers, bad arguments, a shard; nothing enqueued, nothing written
    Guarded o1((size_t)n), o2((size_t)n), rec(8);
    Vec h1((size_t)n, -3.0), h2((size_t)n, -3.0), hrec(8, -3.0);
    const Vec X = trial_x(v, 2), G = trial_g(b, 2), alphas = {1.0, 0.5};
    const size_t mark = fake_hip_log().size();
    CHECK(pk_slack_reduce_dev(ctx, b.g.data(), b.s.data(), b.lam.data(), b.sig.data(), b.rbar.data(), o1.ptr(), o2.ptr(), rec.ptr(), nullptr) == 123);
    CHECK(pk_slack_recover_dev(ctx, b.dlam.data(), b.lam.data(), b.rbar.data(), b.s2.data(), b.sig.data(), v.dx.data(), v.w.data(), v.s1.data(), o1.ptr(),
                               rec.ptr(), nullptr) == 123);
    CHECK(pk_slack_update_dev(ctx, 1, o1.ptr(), b.dv.data(), o2.ptr(), b.dzl.data(), o2.ptr(), b.dzu.data(), nullptr, nullptr, AP, AD, MU, KAPPA, rec.ptr(),
                              nullptr) == 123);
    CHECK(pk_slack_merit_dev(ctx, 2, X.data(), G.data(), b.s.data(), b.ds.data(), alphas.data(), rec.ptr(), nullptr) == 123);
    CHECK(pk_slack_reduce(ctx, b.g.data(), b.s.data(), b.lam.data(), b.sig.data(), b.rbar.data(), h1.data(), h2.data(), hrec.data()) == 123);
    CHECK(pk_slack_recover(ctx, b.dlam.data(), b.lam.data(), b.rbar.data(), b.s2.data(), b.sig.data(), v.dx.data(), v.w.data(), v.s1.data(), h1.data(),
                           hrec.data()) == 123);
    OK(pk_set_bounds(ctx, b.lb.data(), b.ub.data(), v.lb.data(), v.ub.data()));
    const size_t mark2 = fake_hip_log().size();
    CHECK(pk_slack_reduce_dev(ctx, nullptr, b.s.data(), b.lam.data(), b.sig.data(), b.rbar.data(), o1.ptr(), o2.ptr(), rec.ptr(), nullptr) == 110);
    CHECK(pk_slack_reduce_dev(ctx, b.g.data(), b.s.data(), b.lam.data(), b.sig.data(), b.rbar.data(), o1.ptr(), o2.ptr(), nullptr, nullptr) == 110);
    CHECK(pk_slack_recover_dev(ctx, b.dlam.data(), b.lam.data(), b.rbar.data(), b.s2.data(), b.sig.data(), v.dx.data(), nullptr, v.s1.data(), o1.ptr(),
                               rec.ptr(), nullptr) == 110);
    CHECK(pk_slack_update_dev(ctx, 1, o1.ptr(), b.dv.data(), nullptr, b.dzl.data(), o2.ptr(), b.dzu.data(), nullptr, nullptr, AP, AD, MU, KAPPA, rec.ptr(),
                              nullptr) == 110);
    CHECK(pk_slack_update_dev(ctx, 1, o1.ptr(), b.dv.data(), o2.ptr(), b.dzl.data(), o2.ptr(), b.dzu.data(), o1.ptr(), nullptr, AP, AD, MU, KAPPA, rec.ptr(),
                              nullptr) == 110);
    CHECK(pk_slack_update_dev(ctx, 2, o1.ptr(), b.dv.data(), o2.ptr(), b.dzl.data(), o2.ptr(), b.dzu.data(), nullptr, nullptr, AP, AD, MU, KAPPA, rec.ptr(),
                              nullptr) == 134);
    CHECK(pk_slack_update_dev(ctx, 0, o1.ptr(), bx.dv.data(), o2.ptr(), bx.dzl.data(), o2.ptr(), bx.dzu.data(), o1.ptr(), bx.dlam.data(), AP, AD, MU, KAPPA,
                              rec.ptr(), nullptr) == 134);
    CHECK(pk_slack_update_dev(ctx, 1, o1.ptr(), b.dv.data(), o2.ptr(), b.dzl.data(), o2.ptr(), b.dzu.data(), nullptr, nullptr, 2.0, AD, MU, KAPPA, rec.ptr(),
                              nullptr) == 134);
    CHECK(pk_slack_update_dev(ctx, 1, o1.ptr(), b.dv.data(), o2.ptr(), b.dzl.data(), o2.ptr(), b.dzu.data(), nullptr, nullptr, AP, AD, MU, 0.0, rec.ptr(),
                              nullptr) == 134);
    CHECK(pk_slack_merit_dev(ctx, 0, X.data(), G.data(), b.s.data(), b.ds.data(), alphas.data(), rec.ptr(), nullptr) == 134);
    CHECK(pk_slack_merit_dev(ctx, 2, X.data(), nullptr, b.s.data(), b.ds.data(), alphas.data(), rec.ptr(), nullptr) == 110);
    CHECK(pk_slack_reduce(ctx, nullptr, b.s.data(), b.lam.data(), b.sig.data(), b.rbar.data(), h1.data(), h2.data(), hrec.data()) == 60);
    CHECK(pk_slack_reduce(ctx, b.g.data(), b.s.data(), b.lam.data(), b.sig.data(), b.rbar.data(), h1.data(), h2.data(), nullptr) == 60);
    CHECK(pk_slack_recover(ctx, b.dlam.data(), b.lam.data(), b.rbar.data(), b.s2.data(), b.sig.data(), v.dx.data(), v.w.data(), v.s1.data(), nullptr,
                           hrec.data()) == 60);
    CHECK(pk_slack_update(ctx, 1, h1.data(), b.dv.data(), h2.data(), b.dzl.data(), h2.data(), b.dzu.data(), h1.data(), nullptr, AP, AD, MU, KAPPA,
                          hrec.data()) == 60);
    CHECK(pk_slack_update(ctx, 1, h1.data(), b.dv.data(), h2.data(), b.dzl.data(), h2.data(), b.dzu.data(), nullptr, nullptr, AP, AD, -MU, KAPPA,
                          hrec.data()) == 134);
    CHECK(pk_slack_update(ctx, 3, h1.data(), b.dv.data(), h2.data(), b.dzl.data(), h2.data(), b.dzu.data(), nullptr, nullptr, AP, AD, MU, KAPPA,
                          hrec.data()) == 134);
    OK(pk_set_shard(ctx, 1, 0, nullptr));                                        // a shard is refused
    CHECK(pk_slack_reduce_dev(ctx, b.g.data(), b.s.data(), b.lam.data(), b.sig.data(), b.rbar.data(), o1.ptr(), o2.ptr(), rec.ptr(), nullptr) == 119);
    CHECK(pk_slack_merit_dev(ctx, 2, X.data(), G.data(), b.s.data(), b.ds.data(), alphas.data(), rec.ptr(), nullptr) == 119);
    CHECK(pk_slack_update(ctx, 1, h1.data(), b.dv.data(), h2.data(), b.dzl.data(), h2.data(), b.dzu.data(), nullptr, nullptr, AP, AD, MU, KAPPA,
                          hrec.data()) == 119);
    OK(pk_set_shard(ctx, 0, 0, nullptr));
    OK(pk_sync(ctx, nullptr));
    CHECK(mark2 >= mark && fake_hip_log().size() == mark2);
    for (const Guarded* g : {&o1, &o2, &rec}) for (double x : g->fetch()) CHECK(x == -77.0);
    for (const Vec* h : {&h1, &h2, &hrec}) for (double x : *h) CHECK(x == -3.0);
  }
  {  // the device forms on the context's bounds against the raw form, the host forms against both
    const size_t M = (size_t)m;
    Guarded s2(M), b2(M), rec(4), s2r(M), b2r(M), recr(4), hs2(M), hb2(M), hrec(4);
    OK(pk_slack_reduce_dev(ctx, b.g.data(), b.s.data(), b.lam.data(), b.sig.data(), b.rbar.data(), s2.ptr(), b2.ptr(), rec.ptr(), nullptr));
    OK(raw(REDUCE, 0, m, 1, nullptr, b, {in(b.g), in(b.s), in(b.lam), in(b.sig), in(b.rbar), s2r.ptr(), b2r.ptr()}, AP, AD, MU, KAPPA, recr.ptr()));
    OK(pk_slack_reduce(ctx, b.g.data(), b.s.data(), b.lam.data(), b.sig.data(), b.rbar.data(), hs2.ptr(), hb2.ptr(), hrec.ptr()));
    CHECK(same_bits(s2.fetch(), s2r.fetch()) && same_bits(b2.fetch(), b2r.fetch()) && same_bits(rec.fetch(), recr.fetch()));
    CHECK(same_bits(s2.fetch(), hs2.fetch()) && same_bits(b2.fetch(), hb2.fetch()) && same_bits(rec.fetch(), hrec.fetch()));
    CHECK(rec.fetch()[2] == 4.0);
    Guarded ds(M), rec5(5), dsr(M), rec5r(5), hds(M), hrec5(5);
    OK(pk_slack_recover_dev(ctx, b.dlam.data(), b.lam.data(), b.rbar.data(), b.s2.data(), b.sig.data(), v.dx.data(), v.w.data(), v.s1.data(), ds.ptr(),
                            rec5.ptr(), nullptr));
    OK(raw(RECOVER, n, m, 1, &v, b, {in(b.dlam), in(b.lam), in(b.rbar), in(b.s2), in(b.sig), in(v.dx), in(v.w), in(v.s1), dsr.ptr()}, AP, AD, MU, KAPPA,
           rec5r.ptr()));
    OK(pk_slack_recover(ctx, b.dlam.data(), b.lam.data(), b.rbar.data(), b.s2.data(), b.sig.data(), v.dx.data(), v.w.data(), v.s1.data(), hds.ptr(),
                        hrec5.ptr()));
    CHECK(same_bits(ds.fetch(), dsr.fetch()) && same_bits(rec5.fetch(), rec5r.fetch()));
    CHECK(same_bits(ds.fetch(), hds.fetch()) && same_bits(rec5.fetch(), hrec5.fetch()) && rec5.fetch()[4] == 4.0);
    for (int which = 0; which < 2; ++which) {
      const Rows& u = which ? b : bx;
      Rows ub = u;                                       // (which = 0: the raw form on the variables' bounds)
      if (!which) { ub.lb = v.lb; ub.ub = v.ub; }
      const bool with_lam = which == 1;
      Guarded a(u.s), zl(u.zl), zu(u.zu), lam(u.lam), rec4(4), ar(u.s), zlr(u.zl), zur(u.zu), lamr(u.lam), rec4r(4);
      Guarded ha(u.s), hzl(u.zl), hzu(u.zu), hlam(u.lam), hrec4(4);
      OK(pk_slack_update_dev(ctx, which, a.ptr(), u.dv.data(), zl.ptr(), u.dzl.data(), zu.ptr(), u.dzu.data(), with_lam ? lam.ptr() : nullptr,
                             with_lam ? u.dlam.data() : nullptr, AP, AD, MU, KAPPA, rec4.ptr(), nullptr));
      OK(raw(UPDATE, 0, (int64_t)u.lb.size(), 1, nullptr, ub,
             {ar.ptr(), in(u.dv), zlr.ptr(), in(u.dzl), zur.ptr(), in(u.dzu), with_lam ? lamr.ptr() : nullptr, with_lam ? in(u.dlam) : nullptr}, AP, AD, MU,
             KAPPA, rec4r.ptr()));
      OK(pk_slack_update(ctx, which, ha.ptr(), u.dv.data(), hzl.ptr(), u.dzl.data(), hzu.ptr(), u.dzu.data(), with_lam ? hlam.ptr() : nullptr,
                         with_lam ? u.dlam.data() : nullptr, AP, AD, MU, KAPPA, hrec4.ptr()));
      OK(pk_sync(ctx, nullptr));
      CHECK(same_bits(a.fetch(), ar.fetch()) && same_bits(zl.fetch(), zlr.fetch()) && same_bits(zu.fetch(), zur.fetch()) &&
            same_bits(lam.fetch(), lamr.fetch()) && same_bits(rec4.fetch(), rec4r.fetch()));
      CHECK(same_bits(a.fetch(), ha.fetch()) && same_bits(zl.fetch(), hzl.fetch()) && same_bits(zu.fetch(), hzu.fetch()) &&
            same_bits(lam.fetch(), hlam.fetch()) && same_bits(rec4.fetch(), hrec4.fetch()));
    }
    const Vec X = trial_x(v, 3), G = trial_g(b, 3), alphas = {1.0, 0.5, 0.25};
    Guarded t(12), tr(12);
    OK(pk_slack_merit_dev(ctx, 3, X.data(), G.data(), b.s.data(), b.ds.data(), alphas.data(), t.ptr(), nullptr));
    OK(raw(MERIT, n, m, 3, &v, b, {in(X), in(G), in(b.s), in(b.ds), in(alphas)}, AP, AD, MU, KAPPA, tr.ptr()));
    OK(pk_sync(ctx, nullptr));
    CHECK(same_bits(t.fetch(), tr.fetch()));
  }

  // ---- what frees the state: pk_destroy leaves no live allocation
  CHECK(fake_hip_live_allocations() > 0);
  set_problem(400, 6, 11, 7);
  check_kernels(2049, 2049, true);                                             // (allocated again on first use)
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return checks_passed();
}
