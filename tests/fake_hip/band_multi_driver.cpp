// band_multi_driver.cpp -- TEST INFRASTRUCTURE: drives the block solve of pockit_amd/csrc/pk_band.cpp (k right-hand sides against
// one factorisation: pk_band_raw_multi_dev, pk_band_solve_multi_dev, pk_solve_banded_multi) against the host-only HIP stand-in of
// this directory, built with -fsanitize=address,undefined (tests/test_band_multi_cpu.py).  The stand-in walk of every
// kernel through the raw form against the PLAIN LOOPS of band_driver_common.h (one unblocked band LU, then per column the sweeps,
// the pieced dots, the border's LU with the column's t eliminated beside it, x_B) and against k calls of the single raw form,
// bit for bit, at Nb = 0, 1, 33, 65, 2 NB + 1 + 192, w = 0, 7, 33, 192, p = 0, 1, 8, k = 1, 2, 9, 64 (the k single calls at the cap
// of w only up to k = 9 and for the first and last column of 64: each of them factors again); strides n + m and n + m + 3 with
// NaN in the gaps of the right-hand sides and of the solutions, still NaN afterwards; a NaN planted in one column; a failed
// pivot leaving every column untouched; (8 200, 1, 1) with k = 64, whose elementwise kernels (prep, x_B, scatter) take their
// stride loops to a second trip, and (64 000, 1, 1) with k = 64, whose 65 * 32 dot items take the dot kernel's (the sweeps' grid
// holds p + k <= 72 workgroups: its loop cannot); the planned forms against pk_band_solve_dev column by column, the host form against the single host form;
// every refusal with its code, nothing enqueued and nothing written; tear-down without a live allocation.  With --dump FILE: the
// block FILE describes (tests/test_band_multi_cpu.py writes it from tests/band_multi_cases.py) through the raw form.
#include "band_driver_common.h"

static Sys make(int64_t nb, int w, int p, int k, int gap, bool zero_column = false) {
  return make_system(nb, w, p, zero_column ? ZERO : PLAIN, (uint64_t)k, 0, k, gap);
}

// ---------------------------------------------------------------- the raw block form between sentinels
// (Got's x: k rows `stride` apart, -77 in the slots and NaN in the gaps before the call)
static int raw_multi(const Sys& s, Got& g) {
  Guarded band(s.band), x((size_t)(s.stride * s.k), NAN), rec(8), piv((size_t)(s.nb + 1) / 2 + 1);
  for (int c = 0; c < s.k; ++c)
    for (int64_t i = 0; i < s.N(); ++i) x.ptr()[c * s.stride + i] = -77.0;
  const int rc = pk_band_raw_multi_dev(ctx, s.nb, s.w, s.p, s.k, band.ptr(), s.U.data(), s.C.data(), s.rhs.data(), s.stride, (int32_t*)piv.ptr(),
                                       x.ptr(), s.stride, rec.ptr());
  if (rc) return rc;
  OK(pk_sync(ctx, nullptr));
  g.band = band.fetch(); g.x = x.fetch(); g.rec = rec.fetch(); g.ipiv = ipiv_of(piv.fetch(), s.nb);
  return 0;
}

static Vec column(const Sys& s, const Vec& x, int c) { return Vec(x.begin() + (long)(c * s.stride), x.begin() + (long)(c * s.stride + s.N())); }
static bool gaps_nan(const Sys& s, const Vec& x) {
  for (int c = 0; c < s.k; ++c)
    for (int64_t i = s.N(); i < s.stride; ++i)
      if (!std::isnan(x[(size_t)(c * s.stride + i)])) return false;
  return true;
}
static int g_case[5];
static void say_case() { std::fprintf(stderr, "  (case nb %d w %d p %d k %d gap %d)\n", g_case[0], g_case[1], g_case[2], g_case[3], g_case[4]); }

static void check_case(int64_t nb, int w, int p, int k, int gap, bool singles_all) {
  g_case[0] = (int)nb; g_case[1] = w; g_case[2] = p; g_case[3] = k; g_case[4] = gap;
  const Sys s = make(nb, w, p, k, gap);
  const Ref want = reference(s);
  Got got;
  OK(raw_multi(s, got));
  const bool ok = want.rec[STATUS] == 0.0 && bits(got.rec, want.rec) && band_matches(s, got.band, want.band) && gaps_nan(s, got.x);
  if (!ok) say_case();
  CHECK(ok);
  for (int64_t j = 0; j < nb; ++j) CHECK(got.ipiv[(size_t)j] == (double)want.ipiv[(size_t)j]);
  for (int c = 0; c < k; ++c) {
    if (!bits(column(s, got.x, c), want.x[(size_t)c])) { say_case(); std::fprintf(stderr, "  column %d against the plain loops\n", c); }
    CHECK(bits(column(s, got.x, c), want.x[(size_t)c]));
  }
  for (int c = 0; c < k; ++c) {
    if (!singles_all && c != 0 && c != k - 1) continue;
    Got one;
    OK(raw_single(s, c, one));
    const bool same = bits(one.rec, got.rec) && bits(one.ipiv, got.ipiv) && bits(one.x, column(s, got.x, c)) && band_matches(s, one.band, got.band);
    if (!same) { say_case(); std::fprintf(stderr, "  column %d against the single form\n", c); }
    CHECK(same);
  }
}

// FILE: "nb w p k stride", then band (ldab x nb, column-major), U, C, rhs (k x stride, row-major, "nan" in the gaps)
static int dump(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 3;
  long long nb, stride;
  int w, p, k;
  if (std::fscanf(f, "%lld %d %d %d %lld", &nb, &w, &p, &k, &stride) != 5) return 3;
  Sys s = shaped(nb, w, p, k, stride);
  s.band = read_doubles(f); s.U = read_doubles(f); s.C = read_doubles(f); s.rhs = read_doubles(f);
  std::fclose(f);
  s.band.reserve(s.band.size() + 1); s.U.reserve(s.U.size() + 1); s.C.reserve(s.C.size() + 1); s.rhs.reserve(s.rhs.size() + 1);
  load_model();
  set_problem(400, 6, 11, 7);
  Got got;
  OK(raw_multi(s, got));
  CHECK(gaps_nan(s, got.x));
  print(got.band); print(got.ipiv);
  for (int c = 0; c < k; ++c) print(column(s, got.x, c));
  print(got.rec);
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return 0;
}

// ---------------------------------------------------------------- a small K with its plan: n = 14 variables (variable 3 fixed),
// m = 8 rows; H: a diagonal and one subdiagonal
static Planned planned() {
  return planned_kkt(14, 8, 3, [](int32_t r) { return r % 5 != 4; }, [](int32_t) { return true; });
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "--dump")) return dump(argv[2]);
  load_model();
  set_problem(400, 6, 11, 7);

  // ---- every generalised kernel through the raw form against the plain loops and the single form
  for (int64_t nb : {(int64_t)0, (int64_t)1, (int64_t)33, (int64_t)65, (int64_t)2 * NB + 1 + W_CAP})
    for (int w : {0, 7, 33, (int)W_CAP})
      for (int p : {0, 1, (int)P_CAP})
        for (int k : {1, 2, 9, (int)K_CAP}) check_case(nb, w, p, k, (k + p) % 2 ? 3 : 0, w < W_CAP || k <= 9);
  check_case(4500, 8, 1, 9, 3, false);           // three pieces per dot
  // prep, x_B and the scatter beyond 2048 work items of 256 elements: their stride loops take a second trip
  CHECK((8200 + 64 * 8201 + 255) / 256 > 2048 && (64 * 8200 + 255) / 256 > 2048 && (64 * 8201 + 255) / 256 > 2048);
  check_case(8200, 1, 1, K_CAP, 0, false);
  // the dots beyond 2048 work items ((p + k) pieces: 65 * 32): the stride loop of the dot kernel, with its barriers and its reused
  // LDS planes, takes a second trip.  Nb has no cap; the sweeps' loop holds p + k <= 72 items and cannot.
  CHECK((1 + K_CAP) * ((64000 + 2047) / 2048) > 2048);
  check_case(64000, 1, 1, K_CAP, 0, false);
  {  // a NaN planted in one column harms that column only
    Sys s = make(65, 7, 3, 5, 3);
    Got clean, got;
    OK(raw_multi(s, clean));
    s.rhs[(size_t)(2 * s.stride + 11)] = NAN;
    OK(raw_multi(s, got));
    CHECK(got.rec[STATUS] == 0.0 && gaps_nan(s, got.x));
    bool any = false;
    for (double v : column(s, got.x, 2)) any = any || std::isnan(v);
    CHECK(any);
    for (int c : {0, 1, 3, 4}) CHECK(bits(column(s, got.x, c), column(s, clean.x, c)));
    Got one;
    OK(raw_single(s, 2, one));
    CHECK(one.x.size() == (size_t)s.N());
    for (int64_t i = 0; i < s.N(); ++i) {
      const double a = one.x[(size_t)i], b = column(s, got.x, 2)[(size_t)i];
      CHECK((std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, 8) == 0);
    }
  }
  {  // a failed pivot (status 1) and a singular border (status 2): every column of the solutions untouched
    const Sys z = make(3 * NB + 5, 7, 1, 5, 3, true);
    Got got;
    OK(raw_multi(z, got));
    CHECK(got.rec[STATUS] == 1.0 && got.rec[COLUMN] == (double)(2 * (3 * NB + 5) / 3) && gaps_nan(z, got.x));
    for (int c = 0; c < z.k; ++c) for (double v : column(z, got.x, c)) CHECK(v == -77.0);
    Sys s = make(8, 0, 1, 3, 0);
    for (int64_t i = 0; i < 8; ++i) { s.at(i, i) = 2.0; s.U[(size_t)i] = i < 2 ? 2.0 : 0.0; }
    s.C[0] = 4.0;
    OK(raw_multi(s, got));
    CHECK(got.rec[STATUS] == 2.0 && got.rec[COLUMN] == 8.0);
    for (double v : got.x) CHECK(v == -77.0);
  }
  {  // refusals of the raw form: the code, nothing enqueued, nothing written
    const Sys s = make(40, 7, 1, 3, 0);
    Guarded band(s.band), x((size_t)(3 * 41)), rec(8), piv(21);
    const size_t mark = fake_hip_log().size();
    int32_t* pv = (int32_t*)piv.ptr();
    const double *U = s.U.data(), *C = s.C.data(), *b = s.rhs.data();
    CHECK(pk_band_raw_multi_dev(ctx, -1, 7, 1, 3, band.ptr(), U, C, b, 41, pv, x.ptr(), 41, rec.ptr()) == 134);
    CHECK(pk_band_raw_multi_dev(ctx, 40, W_CAP + 1, 1, 3, band.ptr(), U, C, b, 41, pv, x.ptr(), 41, rec.ptr()) == 134);
    CHECK(pk_band_raw_multi_dev(ctx, 40, 7, P_CAP + 1, 3, band.ptr(), U, C, b, 41, pv, x.ptr(), 41, rec.ptr()) == 134);
    CHECK(pk_band_raw_multi_dev(ctx, 40, 7, 1, 0, band.ptr(), U, C, b, 41, pv, x.ptr(), 41, rec.ptr()) == 134);
    CHECK(pk_band_raw_multi_dev(ctx, 40, 7, 1, K_CAP + 1, band.ptr(), U, C, b, 41, pv, x.ptr(), 41, rec.ptr()) == 134);
    CHECK(pk_band_raw_multi_dev(ctx, 40, 7, 1, 3, band.ptr(), U, C, b, 40, pv, x.ptr(), 41, rec.ptr()) == 134);
    CHECK(pk_band_raw_multi_dev(ctx, 40, 7, 1, 3, band.ptr(), U, C, b, 41, pv, x.ptr(), 40, rec.ptr()) == 134);
    CHECK(pk_band_raw_multi_dev(ctx, 40, 7, 1, 3, band.ptr(), U, C, b, 0, pv, x.ptr(), 41, rec.ptr()) == 134);
    CHECK(pk_band_raw_multi_dev(ctx, 40, 7, 1, 3, nullptr, U, C, b, 41, pv, x.ptr(), 41, rec.ptr()) == 110);
    CHECK(pk_band_raw_multi_dev(ctx, 40, 7, 1, 3, band.ptr(), nullptr, C, b, 41, pv, x.ptr(), 41, rec.ptr()) == 110);
    CHECK(pk_band_raw_multi_dev(ctx, 40, 7, 1, 3, band.ptr(), U, nullptr, b, 41, pv, x.ptr(), 41, rec.ptr()) == 110);
    CHECK(pk_band_raw_multi_dev(ctx, 40, 7, 1, 3, band.ptr(), U, C, nullptr, 41, pv, x.ptr(), 41, rec.ptr()) == 110);
    CHECK(pk_band_raw_multi_dev(ctx, 40, 7, 1, 3, band.ptr(), U, C, b, 41, nullptr, x.ptr(), 41, rec.ptr()) == 110);
    CHECK(pk_band_raw_multi_dev(ctx, 40, 7, 1, 3, band.ptr(), U, C, b, 41, pv, nullptr, 41, rec.ptr()) == 110);
    CHECK(pk_band_raw_multi_dev(ctx, 40, 7, 1, 3, band.ptr(), U, C, b, 41, pv, x.ptr(), 41, nullptr) == 110);
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark);
    for (const Guarded* g : {&x, &rec, &piv}) for (double v : g->fetch()) CHECK(v == -77.0);
  }

  // ---- the planned forms: n = 14 variables (one fixed), m = 8 rows, the last variable in the border
  const Planned q = planned();
  const int32_t n = q.n, m = q.m;
  const size_t N = (size_t)(n + m);
  CHECK(q.p == 1 && q.w > 0 && q.nb == (int64_t)N - 2);
  set_problem(n, m, q.A.nnz(), q.Lo.nnz());
  Vec hv((size_t)q.Lo.nnz()), jv((size_t)q.A.nnz()), s1((size_t)n), s2((size_t)m);
  g_state = 99;
  for (Vec* v : {&hv, &jv}) for (double& e : *v) e = unit();
  for (double& e : s1) e = 3.0 + unit();
  for (double& e : s2) e = 2.0 + unit();
  const int k = 5;
  const size_t wide = N + 3;
  Vec packed(k * N), strided(k * wide, NAN);
  for (int c = 0; c < k; ++c)
    for (size_t i = 0; i < N; ++i) packed[c * N + i] = strided[c * wide + i] = unit();
  for (int c = 0; c < k; ++c) packed[c * N + 3] = strided[c * wide + 3] = NAN;      // (the fixed variable's entry is not read)
  set_identity_map(0, q.A.nnz());
  set_identity_map(1, q.Lo.nnz());
  OK(set_operator(0, q.A));
  OK(set_operator(1, q.T));
  OK(set_operator(2, q.S));
  {  // without a plan, without a factorisation, null pointers, counts, strides, a shard: the codes, nothing enqueued or written
    Guarded sol(k * N);
    Vec hx(k * N, -3.0), hrec(8, -3.0);
    const size_t mark = fake_hip_log().size();
    CHECK(pk_band_solve_multi_dev(ctx, k, packed.data(), (int64_t)N, sol.ptr(), (int64_t)N) == 134);                 // no plan
    CHECK(pk_solve_banded_multi(ctx, k, s1.data(), s2.data(), packed.data(), hx.data(), hrec.data()) == 134);         // no plan
    CHECK(fake_hip_log().size() == mark);
    OK(pk_band_plan(ctx, q.nb, q.w, q.p, q.order.data(), q.map.data()));
    const size_t mark2 = fake_hip_log().size();
    CHECK(pk_band_solve_multi_dev(ctx, k, packed.data(), (int64_t)N, sol.ptr(), (int64_t)N) == 134);                 // planned, not factored
    CHECK(pk_solve_banded_multi(ctx, k, s1.data(), s2.data(), packed.data(), hx.data(), hrec.data()) == 118);         // no linearization
    CHECK(pk_solve_banded_multi(ctx, 0, s1.data(), s2.data(), packed.data(), hx.data(), hrec.data()) == 134);
    CHECK(pk_solve_banded_multi(ctx, K_CAP + 1, s1.data(), s2.data(), packed.data(), hx.data(), hrec.data()) == 134);
    CHECK(pk_solve_banded_multi(ctx, k, nullptr, s2.data(), packed.data(), hx.data(), hrec.data()) == 60);
    CHECK(pk_solve_banded_multi(ctx, k, s1.data(), s2.data(), nullptr, hx.data(), hrec.data()) == 60);
    CHECK(pk_solve_banded_multi(ctx, k, s1.data(), s2.data(), packed.data(), nullptr, hrec.data()) == 60);
    CHECK(pk_solve_banded_multi(ctx, k, s1.data(), s2.data(), packed.data(), hx.data(), nullptr) == 60);
    OK(pk_band_factor_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data()));
    OK(pk_sync(ctx, nullptr));
    const size_t mark3 = fake_hip_log().size();
    CHECK(pk_band_solve_multi_dev(ctx, k, nullptr, (int64_t)N, sol.ptr(), (int64_t)N) == 110);
    CHECK(pk_band_solve_multi_dev(ctx, k, packed.data(), (int64_t)N, nullptr, (int64_t)N) == 110);
    CHECK(pk_band_solve_multi_dev(ctx, 0, packed.data(), (int64_t)N, sol.ptr(), (int64_t)N) == 134);
    CHECK(pk_band_solve_multi_dev(ctx, K_CAP + 1, packed.data(), (int64_t)N, sol.ptr(), (int64_t)N) == 134);
    CHECK(pk_band_solve_multi_dev(ctx, k, packed.data(), (int64_t)N - 1, sol.ptr(), (int64_t)N) == 134);
    CHECK(pk_band_solve_multi_dev(ctx, k, packed.data(), 0, sol.ptr(), (int64_t)N) == 134);
    CHECK(pk_band_solve_multi_dev(ctx, k, packed.data(), (int64_t)N, sol.ptr(), (int64_t)N - 1) == 134);
    OK(pk_set_shard(ctx, 1, 0, nullptr));
    CHECK(pk_band_solve_multi_dev(ctx, k, packed.data(), (int64_t)N, sol.ptr(), (int64_t)N) == 119);
    CHECK(pk_solve_banded_multi(ctx, k, s1.data(), s2.data(), packed.data(), hx.data(), hrec.data()) == 119);
    OK(pk_set_shard(ctx, 0, 0, nullptr));
    OK(pk_sync(ctx, nullptr));
    CHECK(mark2 >= mark && fake_hip_log().size() == mark3);
    for (double v : sol.fetch()) CHECK(v == -77.0);
    for (const Vec* h : {&hx, &hrec}) for (double v : *h) CHECK(v == -3.0);
  }
  {  // the block against pk_band_solve_dev column by column: packed, then strided with NaN gaps; twice (the same bits); the record
    Vec single(k * N), rec1(8);
    for (int c = 0; c < k; ++c) {
      Guarded sol(N);
      OK(pk_band_solve_dev(ctx, packed.data() + c * N, sol.ptr()));
      OK(pk_band_record(ctx, rec1.data()));
      const Vec got = sol.fetch();
      std::copy(got.begin(), got.end(), single.begin() + (long)(c * N));
      CHECK(rec1[STATUS] == 0.0 && got[3] == 0.0);
    }
    for (int round = 0; round < 2; ++round) {
      Guarded sol(k * N);
      Vec rec(8);
      OK(pk_band_solve_multi_dev(ctx, k, packed.data(), (int64_t)N, sol.ptr(), (int64_t)N));
      OK(pk_band_record(ctx, rec.data()));
      CHECK(same_bits(sol.fetch(), single) && same_bits(rec, rec1));
    }
    Guarded sol(k * wide, NAN);
    for (int c = 0; c < k; ++c) for (size_t i = 0; i < N; ++i) sol.ptr()[c * wide + i] = -77.0;
    OK(pk_band_solve_multi_dev(ctx, k, strided.data(), (int64_t)wide, sol.ptr(), (int64_t)wide));
    OK(pk_sync(ctx, nullptr));
    const Vec got = sol.fetch();
    for (int c = 0; c < k; ++c) {
      CHECK(std::memcmp(got.data() + c * wide, single.data() + c * N, 8 * N) == 0);
      for (size_t i = N; i < wide; ++i) CHECK(std::isnan(got[c * wide + i]));
    }
    // k = 1 and k = 64 against the same factors (the arrays grow)
    Vec many(K_CAP * N);
    for (double& e : many) e = unit();
    Guarded big(K_CAP * N), one(N), first(N);
    OK(pk_band_solve_multi_dev(ctx, K_CAP, many.data(), (int64_t)N, big.ptr(), (int64_t)N));
    OK(pk_band_solve_multi_dev(ctx, 1, many.data() + 63 * N, (int64_t)N, one.ptr(), (int64_t)N));
    OK(pk_band_solve_dev(ctx, many.data() + 63 * N, first.ptr()));
    OK(pk_sync(ctx, nullptr));
    CHECK(same_bits(one.fetch(), first.fetch()) && std::memcmp(big.fetch().data() + 63 * N, first.fetch().data(), 8 * N) == 0);
    // a singular band part: status 1, no column written
    Vec hz = hv, jz = jv, s1z = s1;
    std::fill(hz.begin(), hz.end(), 0.0); std::fill(jz.begin(), jz.end(), 0.0); std::fill(s1z.begin(), s1z.end(), 0.0);
    OK(pk_band_factor_dev(ctx, hz.data(), jz.data(), s1z.data(), s2.data()));
    Guarded none(k * N);
    Vec rec3(8);
    OK(pk_band_solve_multi_dev(ctx, k, packed.data(), (int64_t)N, none.ptr(), (int64_t)N));
    OK(pk_band_record(ctx, rec3.data()));
    CHECK(rec3[STATUS] == 1.0);
    for (double v : none.fetch()) CHECK(v == -77.0);
  }
  {  // the host form on the context's linearization against the single host form row by row
    Vec x((size_t)n), lam((size_t)m), big1((size_t)n), big2((size_t)m);
    for (int i = 0; i < n; ++i) x[(size_t)i] = 2.0 * (double)(i % 9 - 4);
    for (int j = 0; j < m; ++j) lam[(size_t)j] = (double)(j % 5 - 2);
    for (int i = 0; i < n; ++i) big1[(size_t)i] = 1.0e9 + 1.0e6 * (i % 5);
    for (int j = 0; j < m; ++j) big2[(size_t)j] = 1.0e9 + 1.0e6 * (j % 3);
    OK(pk_linearize(ctx, x.data(), lam.data(), 2.0));
    Guarded hx(k * N), hrec(8);
    OK(pk_solve_banded_multi(ctx, k, big1.data(), big2.data(), packed.data(), hx.ptr(), hrec.ptr()));
    CHECK(hrec.fetch()[STATUS] == 0.0);
    for (int c = 0; c < k; ++c) {
      Guarded one(N), rec(8);
      OK(pk_solve_banded(ctx, big1.data(), big2.data(), packed.data() + c * N, one.ptr(), rec.ptr()));
      CHECK(same_bits(rec.fetch(), hrec.fetch()) && std::memcmp(hx.fetch().data() + c * N, one.fetch().data(), 8 * N) == 0);
    }
    OK(pk_band_plan(ctx, q.nb, q.w, q.p, q.order.data(), q.map.data()));      // a plan replaces a plan: its factorisation is gone
    Guarded later(k * N);
    CHECK(pk_band_solve_multi_dev(ctx, k, packed.data(), (int64_t)N, later.ptr(), (int64_t)N) == 134);
    for (double v : later.fetch()) CHECK(v == -77.0);
  }

  // ---- what frees the state: a new problem, and pk_destroy leaves no live allocation
  CHECK(fake_hip_live_allocations() > 0);
  set_problem(400, 6, 11, 7);
  check_case(65, 7, 8, 9, 3, true);                                           // (allocated again on first use)
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return checks_passed();
}
