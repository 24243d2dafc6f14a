// band_refine_driver.cpp -- TEST INFRASTRUCTURE: drives the refinement of the band solve, pockit_amd/csrc/pk_band_refine.cpp
// (pk_band_refine_step_dev, pk_band_refine_begin_dev, pk_band_refine_advance_dev, pk_band_refine_record, pk_solve_banded_refined)
// against the host-only HIP stand-in of this directory, built with -fsanitize=address,undefined (tests/test_band_refine_cpu.py).
// The stand-in walk of the three kernels through the step form against PLAIN LOOPS at the lengths 1, 2, 255, 256, 257, 2047,
// 2048, 2049 (and 524 289, where the correction's stride loop takes a second trip), with and without a classification, with NaN
// at every element that is no unknown (r is 0.0 there, the maxima and the count are those of the unknowns, x keeps its NaN) and
// with a NaN and an infinity planted in x, b and q; the decision in its order; the planned forms against their own composition
// from pk_band_solve_dev, pk_kkt_apply_dev and the step form, bit for bit, the freeze rule, status 4 behind a failed
// factorisation, 135 behind a new factorisation or a new plan; the host form; every refusal with its code, nothing enqueued and
// nothing written; tear-down without a live allocation.  With --dump FILE: the refinement of the synthetic system FILE describes
// (tests/test_band_refine_cpu.py writes it from tests/band_refine_cases.py), composed of pk_band_raw_dev, the dense product of K
// in plain loops and the step form; x, r and the record after every step.
#include "band_driver_common.h"

enum { R_STATUS = 0, R_STEPS = 1, R_RNORM = 2, R_XNORM = 3, R_BNORM = 4, R_RHO = 5, R_RHO0 = 6, R_PREV = 7 };
enum { S_RESID = 0, S_SCALAR = 1, S_CORRECT = 2 };
static const int LENGTHS[] = {1, 2, 255, 256, 257, 2047, 2048, 2049};

// ---------------------------------------------------------------- the plain loops
struct Sums {
  double r = 0.0, x = 0.0, b = 0.0, bad = 0.0;
};

static Sums plain_resid(const int32_t* where, const Vec& b, const Vec& q, const Vec& x, Vec& r) {
  Sums s;
  for (size_t i = 0; i < b.size(); ++i) {
    if (where && where[i] < 0) { r[i] = 0.0; continue; }
    const double ri = b[i] - q[i];
    r[i] = ri;
    if (std::isfinite(ri) && std::isfinite(x[i]) && std::isfinite(b[i])) {
      s.r = std::max(s.r, std::fabs(ri)); s.x = std::max(s.x, std::fabs(x[i])); s.b = std::max(s.b, std::fabs(b[i]));
    } else {
      s.bad += 1.0;
    }
  }
  return s;
}

static void plain_scalar(const Sums& s, Vec& rec, int t, double tol, int min_steps, const double* band_rec) {
  if (t == 0) {
    rec.assign(8, 0.0);
    if (band_rec && band_rec[0] != 0.0) { rec[R_STATUS] = 4.0; return; }
  } else if (rec[R_STATUS] != 0.0) {
    return;
  }
  const double prev = t == 0 ? 0.0 : rec[R_RHO];
  const double cap = 1.0e6 * s.b;
  const double den = std::min(s.x, cap) + s.b;
  const double rho = s.r == 0.0 ? 0.0 : s.r / den;
  rec[R_STEPS] = t; rec[R_RNORM] = s.r; rec[R_XNORM] = s.x; rec[R_BNORM] = s.b; rec[R_RHO] = rho; rec[R_PREV] = prev;
  if (t == 0) rec[R_RHO0] = rho;
  const double bar = (1.0 - 1.0e-9) * prev;
  rec[R_STATUS] = s.bad > 0.0 ? 3.0 : (t >= min_steps && rho <= tol) ? 1.0 : (t >= 1 && rho > bar) ? 2.0 : 0.0;
}

static void plain_correct(const int32_t* where, const Vec& d, const Vec& rec, Vec& x) {
  if (rec[R_STATUS] != 0.0) return;
  for (size_t i = 0; i < x.size(); ++i)
    if (!where || where[i] >= 0) x[i] = x[i] + d[i];
}

// ---------------------------------------------------------------- the step form between sentinels
struct Vectors {
  std::vector<int32_t> where;      // empty: none
  Vec b, q, x, d;
  const int32_t* wp() const { return where.empty() ? nullptr : where.data(); }
};

// full-mantissa vectors with a residual of size 2^-20; `fixed`: every seventh element and the last but one are no unknowns and
// hold NaN; `planted`: a NaN and an infinity at unknowns of x, b and q
static Vectors vectors(size_t len, bool fixed, bool planted) {
  g_state = 977 * len + (fixed ? 5 : 0) + (planted ? 3 : 0) + 1;
  Vectors v;
  v.b = made(len); v.q = made(len); v.x = made(len); v.d = made(len);
  for (size_t i = 0; i < len; ++i) {
    v.b[i] = unit(); v.x[i] = unit(); v.d[i] = unit();
    v.q[i] = v.b[i] + 0x1p-20 * unit();
  }
  if (fixed) {
    v.where.assign(len + 1, 0);
    for (size_t i = 0; i < len; ++i) {
      const bool out = i % 7 == 3 || (len >= 2 && i == len - 2);
      v.where[i] = out ? -1 : (int32_t)i;
      if (out) v.b[i] = v.q[i] = v.x[i] = v.d[i] = NAN;
    }
  }
  if (planted) {
    std::vector<size_t> live;
    for (size_t i = 0; i < len; ++i) if (!fixed || v.where[i] >= 0) live.push_back(i);
    const double plant[6] = {NAN, INFINITY, NAN, -INFINITY, NAN, INFINITY};
    Vec* into[6] = {&v.x, &v.x, &v.b, &v.b, &v.q, &v.q};
    for (size_t k = 0; k < 6 && k < live.size(); ++k) (*into[k])[live[k * (live.size() - 1) / 5]] = plant[k];
  }
  return v;
}

static int step(int which, int64_t len, const int32_t* where, const double* b, const double* q, double* x, const double* d, double* r,
                double* rec, const double* band_rec, double tol, int min_steps, int t) {
  return pk_band_refine_step_dev(ctx, which, len, where, b, q, x, d, r, rec, band_rec, tol, min_steps, t);
}

// resid and the scalar step t, then the correction, against the plain loops; rec_in: the record the scalar step finds (t >= 1)
static void check_kernels(size_t len, bool fixed, bool planted, int t, double tol, int min_steps, const Vec& rec_in) {
  const Vectors v = vectors(len, fixed, planted);
  Vec want_r = made(len), want_rec = rec_in, want_x = v.x;
  const Sums sums = plain_resid(v.wp(), v.b, v.q, v.x, want_r);
  plain_scalar(sums, want_rec, t, tol, min_steps, nullptr);
  plain_correct(v.wp(), v.d, want_rec, want_x);
  for (int round = 0; round < 2; ++round) {      // (twice: the same bits)
    Guarded r(len), rec = rec_in.empty() ? Guarded(8) : Guarded(rec_in), x(v.x);
    OK(step(S_RESID, (int64_t)len, v.wp(), v.b.data(), v.q.data(), x.ptr(), nullptr, r.ptr(), nullptr, nullptr, 0.0, 0, 0));
    OK(step(S_SCALAR, (int64_t)len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rec.ptr(), nullptr, tol, min_steps, t));
    OK(step(S_CORRECT, (int64_t)len, v.wp(), nullptr, nullptr, x.ptr(), v.d.data(), nullptr, rec.ptr(), nullptr, 0.0, 0, t));
    OK(pk_sync(ctx, nullptr));
    const bool ok = same_or_nan(r.fetch(), want_r) && same_bits(rec.fetch(), want_rec) && same_or_nan(x.fetch(), want_x);
    if (!ok) std::fprintf(stderr, "  (len %zu fixed %d planted %d t %d)\n", len, (int)fixed, (int)planted, t);
    CHECK(ok);
    const Vec got = r.fetch(), got_x = x.fetch();
    bool untouched = true;
    if (fixed)
      for (size_t i = 0; i < len; ++i)
        if (v.where[i] < 0) untouched = untouched && got[i] == 0.0 && !std::signbit(got[i]) && std::isnan(got_x[i]);
    CHECK(untouched);
  }
  if (!planted) CHECK(sums.bad == 0.0 && std::isfinite(sums.r) && sums.r > 0.0);
  else CHECK(want_rec[R_STATUS] == 3.0 || !rec_in.empty());
}

// ---------------------------------------------------------------- --dump: a synthetic system refined through the raw forms
// K = [[B, U], [U^T, C]] dense, row-major
static Vec dense_k(const Sys& s) {
  const int64_t N = s.N(), nb = s.nb;
  Vec K((size_t)(N * N), 0.0);
  Sys t = s;
  for (int64_t j = 0; j < nb; ++j)
    for (int64_t i = std::max<int64_t>(0, j - s.w); i <= std::min<int64_t>(nb - 1, j + s.w); ++i) K[(size_t)(i * N + j)] = t.at(i, j);
  for (int q = 0; q < s.p; ++q)
    for (int64_t i = 0; i < nb; ++i) K[(size_t)(i * N + nb + q)] = K[(size_t)((nb + q) * N + i)] = s.U[(size_t)(q * nb + i)];
  for (int a = 0; a < s.p; ++a)
    for (int c = 0; c < s.p; ++c) K[(size_t)((nb + a) * N + nb + c)] = s.C[(size_t)(a + c * s.p)];
  return K;
}
// q = K x: the products rounded one by one, added to 0.0 in ascending j
static Vec dense_kx(const Vec& K, const Vec& x) {
  const size_t N = x.size();
  Vec q = made(N);
  for (size_t i = 0; i < N; ++i) {
    double acc = 0.0;
    for (size_t j = 0; j < N; ++j) { const double pr = K[i * N + j] * x[j]; acc = acc + pr; }
    q[i] = acc;
  }
  return q;
}

// FILE: "nb w p steps min_steps tol", then band, U, C, rhs
static int dump(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 3;
  long long nb;
  int w, p, steps, min_steps;
  double tol;
  if (std::fscanf(f, "%lld %d %d %d %d %la", &nb, &w, &p, &steps, &min_steps, &tol) != 6) return 3;
  Sys s = shaped(nb, w, p);
  s.band = read_doubles(f); s.U = read_doubles(f); s.C = read_doubles(f); s.rhs = read_doubles(f);
  std::fclose(f);
  s.band.reserve(s.band.size() + 1); s.U.reserve(s.U.size() + 1); s.C.reserve(s.C.size() + 1); s.rhs.reserve(s.rhs.size() + 1);
  load_model();
  set_problem(400, 6, 11, 7);
  const Vec K = dense_k(s);
  const size_t N = (size_t)s.N();
  Got first;
  OK(raw_single(s, 0, first));
  print(first.rec);
  Vec x = first.x, r = made(N), d = made(N), rec(8, -3.0), band_rec = first.rec;
  for (int t = 0; t <= steps; ++t) {
    if (t >= 1) {
      Sys c = s;
      c.rhs = r;
      c.stride = (int64_t)N;
      Got corr;
      OK(raw_single(c, 0, corr));
      d = corr.x;
      OK(step(S_CORRECT, (int64_t)N, nullptr, nullptr, nullptr, x.data(), d.data(), nullptr, rec.data(), nullptr, 0.0, 0, t));
      OK(pk_sync(ctx, nullptr));
    }
    const Vec q = dense_kx(K, x);
    OK(step(S_RESID, (int64_t)N, nullptr, s.rhs.data(), q.data(), x.data(), nullptr, r.data(), nullptr, nullptr, 0.0, 0, t));
    OK(step(S_SCALAR, (int64_t)N, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rec.data(), band_rec.data(), tol, min_steps, t));
    OK(pk_sync(ctx, nullptr));
    print(x); print(r); print(rec);
  }
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return 0;
}

// ---------------------------------------------------------------- the planned forms
static Planned planned() {
  return planned_kkt(14, 8, 3, [](int32_t r) { return r % 5 != 4; }, [](int32_t) { return true; });
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "--dump")) return dump(argv[2]);
  load_model();
  set_problem(400, 6, 11, 7);

  // ---- the three kernels against the plain loops
  const Vec none, running = {0.0, 1.0, 0.5, 1.0, 1.0, 0.25, 0.75, 0.75}, tiny = {0.0, 1.0, 1e-9, 1.0, 1.0, 1e-12, 0.75, 0.75};
  Vec stopped = running;
  stopped[R_STATUS] = 2.0;
  for (int len : LENGTHS)
    for (int fixed = 0; fixed < 2; ++fixed) {
      check_kernels((size_t)len, fixed, false, 0, 1.0e-10, 0, none);      // step 0: running (rho about 1e-6)
      check_kernels((size_t)len, fixed, false, 0, 1.0, 0, none);          // step 0: converged at once, the correction is withheld
      check_kernels((size_t)len, fixed, false, 0, 1.0, 1, none);          // ... but not before min_steps
      check_kernels((size_t)len, fixed, true, 0, 1.0e-10, 0, none);       // planted: status 3
      check_kernels((size_t)len, fixed, false, 1, 1.0e-10, 0, running);   // step 1 behind rho 0.25: running on
      check_kernels((size_t)len, fixed, false, 2, 1.0e-10, 0, tiny);      // step 2 behind rho 1e-12: no improvement, stalled
      check_kernels((size_t)len, fixed, false, 2, 1.0e-3, 0, tiny);       // ... converged goes first
      check_kernels((size_t)len, fixed, false, 3, 1.0, 0, stopped);       // a stopped record stays, nothing is corrected
    }
  CHECK((524289 + 255) / 256 > 2048);
  check_kernels(524289, true, false, 0, 1.0e-10, 0, none);                // the correction's stride loop takes a second trip
  {  // a length of 0: the record of an empty system is converged
    Guarded rec(8);
    Vec e = made(0);
    OK(step(S_RESID, 0, nullptr, e.data(), e.data(), e.data(), nullptr, e.data(), nullptr, nullptr, 0.0, 0, 0));
    OK(step(S_SCALAR, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rec.ptr(), nullptr, 0.0, 0, 0));
    OK(step(S_CORRECT, 0, nullptr, nullptr, nullptr, e.data(), e.data(), nullptr, rec.ptr(), nullptr, 0.0, 0, 0));
    OK(pk_sync(ctx, nullptr));
    CHECK(same_bits(rec.fetch(), Vec({1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0})));
  }
  {  // a band record that is not 0: status 4, nothing measured
    const Vectors v = vectors(300, true, false);
    Guarded r(300), rec(8);
    Vec x = v.x, band_rec = {1.0, 5.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    OK(step(S_RESID, 300, v.wp(), v.b.data(), v.q.data(), x.data(), nullptr, r.ptr(), nullptr, nullptr, 0.0, 0, 0));
    OK(step(S_SCALAR, 300, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rec.ptr(), band_rec.data(), 1.0e-10, 0, 0));
    OK(step(S_CORRECT, 300, v.wp(), nullptr, nullptr, x.data(), v.d.data(), nullptr, rec.ptr(), nullptr, 0.0, 0, 1));
    OK(pk_sync(ctx, nullptr));
    CHECK(same_bits(rec.fetch(), Vec({4.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0})) && same_or_nan(x, v.x));
  }
  {  // refusals of the step form: the code, nothing enqueued, nothing written
    const Vectors v = vectors(40, false, false);
    Guarded r(40), rec(8), x(40);
    const size_t mark = fake_hip_log().size();
    const double *b = v.b.data(), *q = v.q.data(), *d = v.d.data();
    CHECK(step(-1, 40, nullptr, b, q, x.ptr(), d, r.ptr(), rec.ptr(), nullptr, 1e-10, 0, 0) == 134);
    CHECK(step(3, 40, nullptr, b, q, x.ptr(), d, r.ptr(), rec.ptr(), nullptr, 1e-10, 0, 0) == 134);
    CHECK(step(S_RESID, -1, nullptr, b, q, x.ptr(), d, r.ptr(), rec.ptr(), nullptr, 1e-10, 0, 0) == 134);
    CHECK(step(S_SCALAR, 40, nullptr, b, q, x.ptr(), d, r.ptr(), rec.ptr(), nullptr, 1e-10, 0, -1) == 134);
    CHECK(step(S_SCALAR, 40, nullptr, b, q, x.ptr(), d, r.ptr(), rec.ptr(), nullptr, -1.0, 0, 0) == 134);
    CHECK(step(S_SCALAR, 40, nullptr, b, q, x.ptr(), d, r.ptr(), rec.ptr(), nullptr, NAN, 0, 0) == 134);
    CHECK(step(S_SCALAR, 40, nullptr, b, q, x.ptr(), d, r.ptr(), rec.ptr(), nullptr, INFINITY, 0, 0) == 134);
    CHECK(step(S_SCALAR, 40, nullptr, b, q, x.ptr(), d, r.ptr(), rec.ptr(), nullptr, 1e-10, -1, 0) == 134);
    CHECK(step(S_SCALAR, 40, nullptr, b, q, x.ptr(), d, r.ptr(), rec.ptr(), nullptr, 1e-10, 11, 0) == 134);
    CHECK(step(S_RESID, 40, nullptr, nullptr, q, x.ptr(), d, r.ptr(), rec.ptr(), nullptr, 1e-10, 0, 0) == 110);
    CHECK(step(S_RESID, 40, nullptr, b, nullptr, x.ptr(), d, r.ptr(), rec.ptr(), nullptr, 1e-10, 0, 0) == 110);
    CHECK(step(S_RESID, 40, nullptr, b, q, nullptr, d, r.ptr(), rec.ptr(), nullptr, 1e-10, 0, 0) == 110);
    CHECK(step(S_RESID, 40, nullptr, b, q, x.ptr(), d, nullptr, rec.ptr(), nullptr, 1e-10, 0, 0) == 110);
    CHECK(step(S_SCALAR, 40, nullptr, b, q, x.ptr(), d, r.ptr(), nullptr, nullptr, 1e-10, 0, 0) == 110);
    CHECK(step(S_CORRECT, 40, nullptr, b, q, nullptr, d, r.ptr(), rec.ptr(), nullptr, 1e-10, 0, 0) == 110);
    CHECK(step(S_CORRECT, 40, nullptr, b, q, x.ptr(), nullptr, r.ptr(), rec.ptr(), nullptr, 1e-10, 0, 0) == 110);
    CHECK(step(S_CORRECT, 40, nullptr, b, q, x.ptr(), d, r.ptr(), nullptr, nullptr, 1e-10, 0, 0) == 110);
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark);
    for (const Guarded* g : {&r, &rec, &x}) for (double e : g->fetch()) CHECK(e == -77.0);
  }

  // ---- the planned forms: n = 14 variables (one fixed), m = 8 rows, the last variable in the border
  const Planned q = planned();
  const int32_t n = q.n, m = q.m;
  const size_t N = (size_t)(n + m);
  set_problem(n, m, q.A.nnz(), q.Lo.nnz());
  Vec hv((size_t)q.Lo.nnz()), jv((size_t)q.A.nnz()), s1((size_t)n), s2((size_t)m), b = made(N);
  g_state = 99;
  for (Vec* v : {&hv, &jv}) for (double& e : *v) e = unit();
  for (double& e : s1) e = 3.0 + unit();
  for (double& e : s2) e = 2.0 + unit();
  for (double& e : b) e = unit();
  b[3] = NAN;      // (the fixed variable's entry is not read)
  set_identity_map(0, q.A.nnz());
  set_identity_map(1, q.Lo.nnz());
  std::vector<int32_t> where(N + 1, -1);
  for (size_t k = 0; k < q.order.size(); ++k) where[(size_t)q.order[k]] = (int32_t)k;
  {  // without operators, a plan or a factorisation, null pointers, parameters, a shard: the codes, nothing enqueued or written
    Guarded sol(N);
    Vec hx(N, -3.0), hrec(8, -3.0), hrrec(8, -3.0);
    const size_t mark = fake_hip_log().size();
    CHECK(pk_band_refine_begin_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data(), b.data(), sol.ptr(), 1e-10, 0) == 117);
    CHECK(pk_solve_banded_refined(ctx, s1.data(), s2.data(), b.data(), hx.data(), hrec.data(), hrrec.data(), 1e-10, 0, 2) == 117);
    OK(set_operator(0, q.A));
    OK(set_operator(1, q.T));
    OK(set_operator(2, q.S));
    CHECK(pk_band_refine_begin_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data(), b.data(), sol.ptr(), 1e-10, 0) == 134);      // no plan
    CHECK(pk_band_refine_advance_dev(ctx, 1) == 135);
    CHECK(pk_band_refine_record(ctx, hrec.data()) == 135);
    CHECK(pk_solve_banded_refined(ctx, s1.data(), s2.data(), b.data(), hx.data(), hrec.data(), hrrec.data(), 1e-10, 0, 2) == 134);
    CHECK(fake_hip_log().size() == mark);
    OK(pk_band_plan(ctx, q.nb, q.w, q.p, q.order.data(), q.map.data()));
    const size_t mark2 = fake_hip_log().size();
    CHECK(pk_band_refine_begin_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data(), b.data(), sol.ptr(), 1e-10, 0) == 134);      // not factored
    CHECK(pk_solve_banded_refined(ctx, s1.data(), s2.data(), b.data(), hx.data(), hrec.data(), hrrec.data(), 1e-10, 0, 2) == 118);
    CHECK(pk_solve_banded_refined(ctx, s1.data(), s2.data(), b.data(), hx.data(), hrec.data(), hrrec.data(), -1.0, 0, 2) == 134);
    CHECK(pk_solve_banded_refined(ctx, s1.data(), s2.data(), b.data(), hx.data(), hrec.data(), hrrec.data(), 1e-10, 11, 2) == 134);
    CHECK(pk_solve_banded_refined(ctx, s1.data(), s2.data(), b.data(), hx.data(), hrec.data(), hrrec.data(), 1e-10, 0, 11) == 134);
    CHECK(pk_solve_banded_refined(ctx, s1.data(), s2.data(), b.data(), hx.data(), hrec.data(), hrrec.data(), 1e-10, 0, -1) == 134);
    CHECK(pk_solve_banded_refined(ctx, nullptr, s2.data(), b.data(), hx.data(), hrec.data(), hrrec.data(), 1e-10, 0, 2) == 60);
    CHECK(pk_solve_banded_refined(ctx, s1.data(), s2.data(), b.data(), nullptr, hrec.data(), hrrec.data(), 1e-10, 0, 2) == 60);
    CHECK(pk_solve_banded_refined(ctx, s1.data(), s2.data(), b.data(), hx.data(), hrec.data(), nullptr, 1e-10, 0, 2) == 60);
    OK(pk_band_factor_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data()));
    OK(pk_sync(ctx, nullptr));
    const size_t mark3 = fake_hip_log().size();
    const double* args[5] = {hv.data(), jv.data(), s1.data(), s2.data(), b.data()};
    for (int k = 0; k < 5; ++k) {
      const double* a[5] = {args[0], args[1], args[2], args[3], args[4]};
      a[k] = nullptr;
      CHECK(pk_band_refine_begin_dev(ctx, a[0], a[1], a[2], a[3], a[4], sol.ptr(), 1e-10, 0) == 110);
    }
    CHECK(pk_band_refine_begin_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data(), b.data(), nullptr, 1e-10, 0) == 110);
    CHECK(pk_band_refine_begin_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data(), b.data(), sol.ptr(), -1e-10, 0) == 134);
    CHECK(pk_band_refine_begin_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data(), b.data(), sol.ptr(), NAN, 0) == 134);
    CHECK(pk_band_refine_begin_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data(), b.data(), sol.ptr(), 1e-10, -1) == 134);
    CHECK(pk_band_refine_begin_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data(), b.data(), sol.ptr(), 1e-10, 11) == 134);
    CHECK(pk_band_refine_advance_dev(ctx, 1) == 135);
    CHECK(pk_band_refine_record(ctx, hrec.data()) == 135);
    CHECK(pk_band_refine_record(ctx, nullptr) == 60);
    OK(pk_set_shard(ctx, 1, 0, nullptr));
    CHECK(pk_band_refine_begin_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data(), b.data(), sol.ptr(), 1e-10, 0) == 119);
    CHECK(pk_band_refine_advance_dev(ctx, 1) == 119);
    CHECK(pk_solve_banded_refined(ctx, s1.data(), s2.data(), b.data(), hx.data(), hrec.data(), hrrec.data(), 1e-10, 0, 2) == 119);
    OK(pk_set_shard(ctx, 0, 0, nullptr));
    OK(pk_sync(ctx, nullptr));
    CHECK(mark2 >= mark && fake_hip_log().size() == mark3);
    for (double v : sol.fetch()) CHECK(v == -77.0);
    for (const Vec* h : {&hx, &hrec, &hrrec}) for (double v : *h) CHECK(v == -3.0);
  }
  Vec first_x, first_rec;
  {  // begin and advance against their own composition from the solve, the product and the step form, step by step
    Guarded sol(N);
    OK(pk_band_solve_dev(ctx, b.data(), sol.ptr()));
    OK(pk_sync(ctx, nullptr));
    first_x = sol.fetch();
    Vec band_rec(8);
    OK(pk_band_record(ctx, band_rec.data()));
    CHECK(band_rec[STATUS] == 0.0 && first_x[3] == 0.0);
    // the composition (tol 0: it runs until it stalls)
    std::vector<Vec> xs, rs, recs;
    Vec x = first_x, r = made(N), d = made(N), kx = made(N), rec(8, -3.0);
    const int steps = 6;
    for (int t = 0; t <= steps; ++t) {
      if (t >= 1) {
        OK(pk_band_solve_dev(ctx, r.data(), d.data()));
        OK(step(S_CORRECT, (int64_t)N, where.data(), nullptr, nullptr, x.data(), d.data(), nullptr, rec.data(), nullptr, 0.0, 0, t));
      }
      OK(pk_kkt_apply_dev(ctx, jv.data(), hv.data(), s1.data(), s2.data(), x.data(), kx.data(), nullptr));
      OK(step(S_RESID, (int64_t)N, where.data(), b.data(), kx.data(), x.data(), nullptr, r.data(), nullptr, nullptr, 0.0, 0, t));
      OK(step(S_SCALAR, (int64_t)N, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rec.data(), band_rec.data(), 0.0, 0, t));
      OK(pk_sync(ctx, nullptr));
      xs.push_back(x); rs.push_back(r); recs.push_back(rec);
    }
    CHECK(recs[0][R_STATUS] == 0.0 && recs[0][R_RHO0] > 0.0 && recs[0][R_RHO0] < 1.0e-12 && rs[0][3] == 0.0);
    CHECK((recs[steps][R_STATUS] == 2.0 || (recs[steps][R_STATUS] == 1.0 && recs[steps][R_RNORM] == 0.0)) && recs[steps][R_STEPS] >= 1.0);
    for (int round = 0; round < 2; ++round) {      // (twice: the same bits; the second begin replaces the first)
      Guarded live(first_x);
      Vec got(8);
      OK(pk_band_refine_begin_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data(), b.data(), live.ptr(), 0.0, 0));
      OK(pk_band_refine_record(ctx, got.data()));
      CHECK(same_bits(got, recs[0]) && same_bits(live.fetch(), xs[0]));
      for (int t = 1; t <= steps; ++t) {
        OK(pk_band_refine_advance_dev(ctx, 1));
        OK(pk_band_refine_record(ctx, got.data()));
        CHECK(same_bits(got, recs[(size_t)t]) && same_bits(live.fetch(), xs[(size_t)t]));
      }
      // the freeze rule: steps behind the stop change neither x nor the record; and all steps enqueued at once give the same
      OK(pk_band_refine_advance_dev(ctx, 3));
      OK(pk_band_refine_record(ctx, got.data()));
      CHECK(same_bits(got, recs[steps]) && same_bits(live.fetch(), xs[steps]));
      Guarded at_once(first_x);
      OK(pk_band_refine_begin_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data(), b.data(), at_once.ptr(), 0.0, 0));
      OK(pk_band_refine_advance_dev(ctx, steps + 5));
      OK(pk_band_refine_record(ctx, got.data()));
      CHECK(same_bits(got, recs[steps]) && same_bits(at_once.fetch(), xs[steps]));
    }
    first_rec = recs[0];
    // a tolerance rho_0 meets: converged with no correction, x keeps its bits; min_steps 1 takes one
    Guarded kept(first_x), one(first_x);
    Vec got(8);
    OK(pk_band_refine_begin_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data(), b.data(), kept.ptr(), 1.0e-10, 0));
    OK(pk_band_refine_advance_dev(ctx, 2));
    OK(pk_band_refine_record(ctx, got.data()));
    CHECK(got[R_STATUS] == 1.0 && got[R_STEPS] == 0.0 && same_bits(kept.fetch(), first_x));
    OK(pk_band_refine_begin_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data(), b.data(), one.ptr(), 1.0e-10, 1));
    OK(pk_band_refine_advance_dev(ctx, 2));
    OK(pk_band_refine_record(ctx, got.data()));
    CHECK(got[R_STATUS] == 1.0 && got[R_STEPS] == 1.0 && same_bits(one.fetch(), xs[1]));
    // a new factorisation ends the refinement
    OK(pk_band_factor_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data()));
    CHECK(pk_band_refine_advance_dev(ctx, 1) == 135 && pk_band_refine_record(ctx, got.data()) == 135);
    // a singular band part: status 4, x untouched, whatever is enqueued
    Vec hz = hv, jz = jv, s1z = s1;
    std::fill(hz.begin(), hz.end(), 0.0); std::fill(jz.begin(), jz.end(), 0.0); std::fill(s1z.begin(), s1z.end(), 0.0);
    OK(pk_band_factor_dev(ctx, hz.data(), jz.data(), s1z.data(), s2.data()));
    Guarded none(N);
    OK(pk_band_solve_dev(ctx, b.data(), none.ptr()));
    for (size_t i = 0; i < N; ++i) none.ptr()[i] = 0.5;      // (finite: the product reads it)
    OK(pk_band_refine_begin_dev(ctx, hz.data(), jz.data(), s1z.data(), s2.data(), b.data(), none.ptr(), 1.0e-10, 0));
    OK(pk_band_refine_advance_dev(ctx, 2));
    OK(pk_band_refine_record(ctx, got.data()));
    CHECK(same_bits(got, Vec({4.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0})));
    for (double v : none.fetch()) CHECK(v == 0.5);
    // a new plan ends it too
    OK(pk_band_plan(ctx, q.nb, q.w, q.p, q.order.data(), q.map.data()));
    CHECK(pk_band_refine_advance_dev(ctx, 1) == 135);
  }
  {  // the host form on the context's linearization
    Vec x((size_t)n), lam((size_t)m), big1((size_t)n), big2((size_t)m);
    for (int i = 0; i < n; ++i) x[(size_t)i] = 2.0 * (double)(i % 9 - 4);
    for (int j = 0; j < m; ++j) lam[(size_t)j] = (double)(j % 5 - 2);
    for (int i = 0; i < n; ++i) big1[(size_t)i] = 1.0e9 + 1.0e6 * (i % 5);
    for (int j = 0; j < m; ++j) big2[(size_t)j] = 1.0e9 + 1.0e6 * (j % 3);
    OK(pk_linearize(ctx, x.data(), lam.data(), 2.0));
    Guarded plain(N), prec(8);
    OK(pk_solve_banded(ctx, big1.data(), big2.data(), b.data(), plain.ptr(), prec.ptr()));
    CHECK(prec.fetch()[STATUS] == 0.0);
    // no step allowed: the plain solve's bits, measured
    Guarded h0(N), r0(8), rr0(8);
    OK(pk_solve_banded_refined(ctx, big1.data(), big2.data(), b.data(), h0.ptr(), r0.ptr(), rr0.ptr(), 0.0, 0, 0));
    CHECK(same_bits(h0.fetch(), plain.fetch()) && same_bits(r0.fetch(), prec.fetch()));
    const Vec m0 = rr0.fetch();
    CHECK((m0[R_STATUS] == 5.0 || (m0[R_STATUS] == 1.0 && m0[R_RNORM] == 0.0)) && m0[R_STEPS] == 0.0 && m0[R_RHO] == m0[R_RHO0]);
    CHECK(std::isfinite(m0[R_RHO]) && m0[R_XNORM] > 0.0 && m0[R_BNORM] > 0.0 && m0[R_RHO] < 1.0e-10);
    // a tolerance it meets at once: converged, the same bits
    Guarded h1(N), r1(8), rr1(8);
    OK(pk_solve_banded_refined(ctx, big1.data(), big2.data(), b.data(), h1.ptr(), r1.ptr(), rr1.ptr(), 1.0e-10, 0, 10));
    CHECK(rr1.fetch()[R_STATUS] == 1.0 && rr1.fetch()[R_STEPS] == 0.0 && same_bits(h1.fetch(), plain.fetch()));
    // tol 0: until it stalls or the steps run out, twice the same bits
    Guarded h2(N), r2(8), rr2(8), h3(N), r3(8), rr3(8);
    OK(pk_solve_banded_refined(ctx, big1.data(), big2.data(), b.data(), h2.ptr(), r2.ptr(), rr2.ptr(), 0.0, 0, 10));
    OK(pk_solve_banded_refined(ctx, big1.data(), big2.data(), b.data(), h3.ptr(), r3.ptr(), rr3.ptr(), 0.0, 0, 10));
    const Vec m2 = rr2.fetch();
    CHECK(same_bits(h2.fetch(), h3.fetch()) && same_bits(m2, rr3.fetch()) && same_bits(r2.fetch(), prec.fetch()));
    CHECK((m2[R_STATUS] == 2.0 && m2[R_STEPS] >= 1.0) || (m2[R_STATUS] == 1.0 && m2[R_RNORM] == 0.0) || (m2[R_STATUS] == 5.0 && m2[R_STEPS] == 10.0));
    CHECK(same_bits(Vec(1, m2[R_RHO0]), Vec(1, m0[R_RHO0])));
  }

  // ---- what frees the state: a new problem, and pk_destroy leaves no live allocation
  CHECK(fake_hip_live_allocations() > 0);
  set_problem(400, 6, 11, 7);
  check_kernels(2049, true, false, 0, 1.0e-10, 0, none);      // (allocated again on first use)
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  (void)first_rec;
  return checks_passed();
}
