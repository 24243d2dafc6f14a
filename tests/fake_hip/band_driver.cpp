// band_driver.cpp -- TEST INFRASTRUCTURE: drives the entry points of pockit_amd/csrc/pk_band.cpp (the bordered band LU of the
// step's system) against the host-only HIP stand-in of this directory, built with -fsanitize=address,undefined
// (tests/test_band_cpu.py): the stand-in walk of every kernel through the raw form against the PLAIN LOOPS of
// band_driver_common.h (an unblocked band LU, the sweeps, the pieced dots, the border) on full-mantissa data -- the arithmetic is the same, so a result must have
// the loops' BITS -- at Nb = 0, 1, 2, NB - 1, NB, NB + 1, 2 NB + 1 and w + 1, w = 0, 1, 7, NB - 1, NB, NB + 1 and the cap,
// p = 0, 1, 3 and the cap; NaN in the fill rows and outside the matrix (never read), every-column-interchanges, ties, a zero
// column, a planted NaN; the public forms against the raw form, the host form against the device forms, every refusal with its
// code and nothing enqueued or written behind it, a failed pivot leaving sol between its sentinels, and tear-down without a
// live allocation.  With --dump FILE: the system FILE describes (tests/test_band_cpu.py writes it from tests/band_cases.py)
// through the raw form, band, interchanges, solution and record printed as hex doubles.
#include "band_driver_common.h"

static Sys make(int64_t nb, int w, int p, Variant variant) { return make_system(nb, w, p, variant, (uint64_t)variant, 0, 1, 0); }
static int raw(const Sys& s, Got& g) { return raw_single(s, 0, g); }

static int g_nb, g_w, g_p, g_variant;
static void check_case(int64_t nb, int w, int p, Variant variant) {
  g_nb = (int)nb; g_w = w; g_p = p; g_variant = variant;
  const Sys s = make(nb, w, p, variant);
  const Ref want = reference(s);
  Got got;
  OK(raw(s, got));
  if (!bits(got.rec, want.rec)) std::fprintf(stderr, "case nb %d w %d p %d variant %d: record %g %g %g %g %g for %g %g %g %g %g\n", g_nb, g_w, g_p,
                                                   g_variant, got.rec[0], got.rec[1], got.rec[2], got.rec[3], got.rec[7], want.rec[0], want.rec[1],
                                                   want.rec[2], want.rec[3], want.rec[7]);
  CHECK(bits(got.rec, want.rec));
  if (want.rec[STATUS] == 0.0) {
    if (!band_matches(s, got.band, want.band)) std::fprintf(stderr, "case nb %d w %d p %d variant %d: band\n", g_nb, g_w, g_p, g_variant);
    CHECK(band_matches(s, got.band, want.band));
    for (int64_t j = 0; j < nb; ++j) CHECK(got.ipiv[(size_t)j] == (double)want.ipiv[(size_t)j]);
    if (!bits(got.x, want.x[0])) std::fprintf(stderr, "case nb %d w %d p %d variant %d: solution\n", g_nb, g_w, g_p, g_variant);
    CHECK(bits(got.x, want.x[0]));
  } else {
    for (double v : got.x) CHECK(v == -77.0);      // a failed pivot leaves the solution untouched
  }
  if (variant == TINY && nb > 1 && w > 0) CHECK(nb <= EVERY ? got.rec[SWAPS] == (double)(nb - 1) : got.rec[SWAPS] >= (double)(nb / 4));
  if (variant == ZERO && nb) CHECK(got.rec[STATUS] == 1.0 && got.rec[COLUMN] == (double)(2 * nb / 3));
  if (variant == PLANT && nb) CHECK(got.rec[STATUS] == 3.0 && got.rec[COLUMN] == (double)(nb / 2));
}

// FILE: "nb w p", then band (ldab x nb, column-major), U, C, rhs
static int dump(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 3;
  long long nb;
  int w, p;
  if (std::fscanf(f, "%lld %d %d", &nb, &w, &p) != 3) return 3;
  Sys s = shaped(nb, w, p);
  s.band = read_doubles(f); s.U = read_doubles(f); s.C = read_doubles(f); s.rhs = read_doubles(f);
  std::fclose(f);
  s.band.reserve(s.band.size() + 1); s.U.reserve(s.U.size() + 1); s.C.reserve(s.C.size() + 1);
  load_model();
  set_problem(400, 6, 11, 7);
  Got got;
  OK(raw(s, got));
  print(got.band); print(got.ipiv); print(got.x); print(got.rec);
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return 0;
}

// ---------------------------------------------------------------- a small K with its plan: n = 30 variables (variable 3 fixed),
// m = 20 rows
static Planned planned() {
  return planned_kkt(30, 20, 3, [](int32_t r) { return r % 6 != 5; }, [](int32_t r) { return r % 7 != 3; });
}

// the system the plan's map assembles from the four arrays, by plain loops
static Sys assembled(const Planned& q, const Vec& hv, const Vec& jv, const Vec& s1, const Vec& s2, const Vec& rhs) {
  Sys s = shaped(q.nb, q.w, q.p);
  Vec vals;
  for (const Vec* v : {&hv, &jv, &s1, &s2}) vals.insert(vals.end(), v->begin(), v->end());
  Vec all(q.map.size() / 2);
  for (size_t d = 0; d < all.size(); ++d) {
    double acc = 0.0;
    for (int k = 0; k < 2; ++k) {
      const int32_t code = q.map[2 * d + (size_t)k];
      if (code > 0) acc = acc + vals[(size_t)code - 1];
      else if (code < 0) acc = acc - vals[(size_t)(-code) - 1];
    }
    all[d] = acc;
  }
  const size_t nband = (size_t)(s.ldab * s.nb), nu = (size_t)(s.nb * s.p);
  s.band.assign(all.begin(), all.begin() + (long)nband);
  s.U.assign(all.begin() + (long)nband, all.begin() + (long)(nband + nu));
  s.C.assign(all.begin() + (long)(nband + nu), all.end());
  s.rhs = made(q.order.size());
  for (size_t k = 0; k < q.order.size(); ++k) s.rhs[k] = rhs[(size_t)q.order[k]];
  return s;
}

static Vec scattered(const Planned& q, const Vec& x) {
  Vec sol((size_t)(q.n + q.m), 0.0);
  for (size_t k = 0; k < q.order.size(); ++k) sol[(size_t)q.order[k]] = x[k];
  return sol;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "--dump")) return dump(argv[2]);
  load_model();
  set_problem(400, 6, 11, 7);

  // ---- every kernel through the raw form against the plain loops
  const int widths[] = {0, 1, 7, NB - 1, NB, NB + 1, W_CAP};
  const int borders[] = {0, 1, 3, P_CAP};
  for (int w : widths)
    for (int p : borders)
      for (int64_t nb : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)NB - 1, (int64_t)NB, (int64_t)NB + 1, (int64_t)2 * NB + 1, (int64_t)w + 1}) {
        check_case(nb, w, p, PLAIN);
        check_case(nb, w, p, TINY);
      }
  for (Variant variant : {TIES, ZERO, PLANT}) {
    check_case(2 * NB + 1, 7, 1, variant);
    check_case(3 * NB + 5, NB + 1, 3, variant);
    check_case(5, 7, 0, variant);
  }
  check_case(2 * NB + 1 + W_CAP, W_CAP, 1, PLAIN);
  check_case(4500, 8, 1, PLAIN);                 // three pieces per dot, 141 panels
  {  // a singular border: C = U^T B^-1 U on a diagonal B
    Sys s = make(8, 0, 1, PLAIN);
    for (int64_t i = 0; i < 8; ++i) { s.at(i, i) = 2.0; s.U[(size_t)i] = i < 2 ? 2.0 : 0.0; }
    s.C[0] = 4.0;
    Got got;
    OK(raw(s, got));
    CHECK(got.rec[STATUS] == 2.0 && got.rec[COLUMN] == 8.0);
    for (double v : got.x) CHECK(v == -77.0);
  }
  {  // refusals of the raw form: the code, nothing enqueued, nothing written
    const Sys s = make(40, 7, 1, PLAIN);
    Guarded band(s.band), x(41), rec(8), piv(21);
    const size_t mark = fake_hip_log().size();
    int32_t* pv = (int32_t*)piv.ptr();
    CHECK(pk_band_raw_dev(ctx, -1, 7, 1, 2, band.ptr(), s.U.data(), s.C.data(), s.rhs.data(), pv, x.ptr(), rec.ptr()) == 134);
    CHECK(pk_band_raw_dev(ctx, 40, -1, 1, 2, band.ptr(), s.U.data(), s.C.data(), s.rhs.data(), pv, x.ptr(), rec.ptr()) == 134);
    CHECK(pk_band_raw_dev(ctx, 40, W_CAP + 1, 1, 2, band.ptr(), s.U.data(), s.C.data(), s.rhs.data(), pv, x.ptr(), rec.ptr()) == 134);
    CHECK(pk_band_raw_dev(ctx, 40, 7, P_CAP + 1, P_CAP + 2, band.ptr(), s.U.data(), s.C.data(), s.rhs.data(), pv, x.ptr(), rec.ptr()) == 134);
    CHECK(pk_band_raw_dev(ctx, 40, 7, -1, 0, band.ptr(), s.U.data(), s.C.data(), s.rhs.data(), pv, x.ptr(), rec.ptr()) == 134);
    CHECK(pk_band_raw_dev(ctx, 40, 7, 1, 1, band.ptr(), s.U.data(), s.C.data(), s.rhs.data(), pv, x.ptr(), rec.ptr()) == 134);
    CHECK(pk_band_raw_dev(ctx, 40, 7, 1, 2, nullptr, s.U.data(), s.C.data(), s.rhs.data(), pv, x.ptr(), rec.ptr()) == 110);
    CHECK(pk_band_raw_dev(ctx, 40, 7, 1, 2, band.ptr(), nullptr, s.C.data(), s.rhs.data(), pv, x.ptr(), rec.ptr()) == 110);
    CHECK(pk_band_raw_dev(ctx, 40, 7, 1, 2, band.ptr(), s.U.data(), nullptr, s.rhs.data(), pv, x.ptr(), rec.ptr()) == 110);
    CHECK(pk_band_raw_dev(ctx, 40, 7, 1, 2, band.ptr(), s.U.data(), s.C.data(), nullptr, pv, x.ptr(), rec.ptr()) == 110);
    CHECK(pk_band_raw_dev(ctx, 40, 7, 1, 2, band.ptr(), s.U.data(), s.C.data(), s.rhs.data(), nullptr, x.ptr(), rec.ptr()) == 110);
    CHECK(pk_band_raw_dev(ctx, 40, 7, 1, 2, band.ptr(), s.U.data(), s.C.data(), s.rhs.data(), pv, nullptr, rec.ptr()) == 110);
    CHECK(pk_band_raw_dev(ctx, 40, 7, 1, 2, band.ptr(), s.U.data(), s.C.data(), s.rhs.data(), pv, x.ptr(), nullptr) == 110);
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark);
    CHECK(same_or_nan(band.fetch(), s.band));
    for (const Guarded* g : {&x, &rec, &piv}) for (double v : g->fetch()) CHECK(v == -77.0);
  }

  // ---- the public forms on a planned system: n = 30 variables (one fixed), m = 20 rows, the last variable in the border
  const Planned q = planned();
  const int32_t n = q.n, m = q.m;
  const size_t N = (size_t)(n + m);
  CHECK(q.p == 1 && q.w > 0 && q.w <= W_CAP && q.nb == (int64_t)N - 2);
  set_problem(n, m, q.A.nnz(), q.Lo.nnz());
  Vec hv((size_t)q.Lo.nnz()), jv((size_t)q.A.nnz()), s1((size_t)n), s2((size_t)m), rhs(N);
  g_state = 99;
  for (Vec* v : {&hv, &jv, &rhs}) for (double& e : *v) e = unit();
  for (double& e : s1) e = 3.0 + unit();
  for (double& e : s2) e = 2.0 + unit();
  rhs[3] = NAN;                                   // (the fixed variable's entry is not read)
  {  // before the plan, with bad plans, null pointers, a shard: the codes, nothing enqueued, nothing written
    Guarded sol(N), rec(8);
    Vec hsol(N, -3.0), hrec(8, -3.0);
    const size_t mark = fake_hip_log().size();
    CHECK(pk_band_factor_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data()) == 134);
    CHECK(pk_band_solve_dev(ctx, rhs.data(), sol.ptr()) == 134);
    CHECK(pk_band_record(ctx, hrec.data()) == 134);
    CHECK(pk_band_plan(ctx, q.nb, q.w, q.p, q.order.data(), q.map.data()) == 134);      // no CSR maps yet: the sources are out of range
    set_identity_map(0, q.A.nnz());
    set_identity_map(1, q.Lo.nnz());
    const size_t mark2 = fake_hip_log().size();
    CHECK(pk_band_plan(ctx, q.nb, q.w, q.p, nullptr, q.map.data()) == 60);
    CHECK(pk_band_plan(ctx, q.nb, q.w, q.p, q.order.data(), nullptr) == 60);
    CHECK(pk_band_plan(ctx, -1, q.w, q.p, q.order.data(), q.map.data()) == 134);
    CHECK(pk_band_plan(ctx, q.nb, W_CAP + 1, q.p, q.order.data(), q.map.data()) == 134);
    CHECK(pk_band_plan(ctx, q.nb, q.w, P_CAP + 1, q.order.data(), q.map.data()) == 134);
    CHECK(pk_band_plan(ctx, (int64_t)N, q.w, q.p, q.order.data(), q.map.data()) == 134);      // more unknowns than the system has
    {
      std::vector<int32_t> twice = q.order;
      twice[1] = twice[0];
      CHECK(pk_band_plan(ctx, q.nb, q.w, q.p, twice.data(), q.map.data()) == 134);
      twice[1] = (int32_t)N;
      CHECK(pk_band_plan(ctx, q.nb, q.w, q.p, twice.data(), q.map.data()) == 134);
      std::vector<int32_t> far = q.map;
      far[0] = (int32_t)(q.Lo.nnz() + q.A.nnz() + (int64_t)N + 1);
      CHECK(pk_band_plan(ctx, q.nb, q.w, q.p, q.order.data(), far.data()) == 134);
    }
    CHECK(pk_solve_banded(ctx, s1.data(), s2.data(), rhs.data(), hsol.data(), hrec.data()) == 117);      // no operators
    OK(set_operator(0, q.A));
    OK(set_operator(1, q.T));
    OK(set_operator(2, q.S));
    const size_t mark3 = fake_hip_log().size();
    CHECK(pk_solve_banded(ctx, s1.data(), s2.data(), rhs.data(), hsol.data(), hrec.data()) == 134);      // no plan
    OK(pk_set_shard(ctx, 1, 0, nullptr));
    CHECK(pk_band_plan(ctx, q.nb, q.w, q.p, q.order.data(), q.map.data()) == 119);
    OK(pk_set_shard(ctx, 0, 0, nullptr));
    OK(pk_band_plan(ctx, q.nb, q.w, q.p, q.order.data(), q.map.data()));
    const size_t mark4 = fake_hip_log().size();
    CHECK(pk_band_solve_dev(ctx, rhs.data(), sol.ptr()) == 134);                                          // planned, not factored
    CHECK(pk_band_record(ctx, hrec.data()) == 134);
    CHECK(pk_band_factor_dev(ctx, nullptr, jv.data(), s1.data(), s2.data()) == 110);
    CHECK(pk_band_factor_dev(ctx, hv.data(), nullptr, s1.data(), s2.data()) == 110);
    CHECK(pk_band_factor_dev(ctx, hv.data(), jv.data(), nullptr, s2.data()) == 110);
    CHECK(pk_band_factor_dev(ctx, hv.data(), jv.data(), s1.data(), nullptr) == 110);
    CHECK(pk_solve_banded(ctx, s1.data(), s2.data(), rhs.data(), hsol.data(), hrec.data()) == 118);      // no linearization
    CHECK(pk_solve_banded(ctx, nullptr, s2.data(), rhs.data(), hsol.data(), hrec.data()) == 60);
    CHECK(pk_solve_banded(ctx, s1.data(), s2.data(), rhs.data(), nullptr, hrec.data()) == 60);
    CHECK(pk_solve_banded(ctx, s1.data(), s2.data(), rhs.data(), hsol.data(), nullptr) == 60);
    OK(pk_set_shard(ctx, 1, 0, nullptr));
    CHECK(pk_band_factor_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data()) == 119);
    CHECK(pk_band_solve_dev(ctx, rhs.data(), sol.ptr()) == 119);
    CHECK(pk_solve_banded(ctx, s1.data(), s2.data(), rhs.data(), hsol.data(), hrec.data()) == 119);
    OK(pk_set_shard(ctx, 0, 0, nullptr));
    OK(pk_sync(ctx, nullptr));
    CHECK(mark2 >= mark && mark3 >= mark2 && mark4 >= mark3 && fake_hip_log().size() == mark4);
    for (const Guarded* g : {&sol, &rec}) for (double v : g->fetch()) CHECK(v == -77.0);
    for (const Vec* h : {&hsol, &hrec}) for (double v : *h) CHECK(v == -3.0);
  }
  {  // factor and solve on the plan against the raw form on the system assembled by plain loops, twice (a second right-hand side)
    const Sys s = assembled(q, hv, jv, s1, s2, rhs);
    const Ref want = reference(s);
    CHECK(want.rec[STATUS] == 0.0);
    OK(pk_band_factor_dev(ctx, hv.data(), jv.data(), s1.data(), s2.data()));
    for (int round = 0; round < 2; ++round) {
      Guarded sol(N);
      Vec rec(8);
      OK(pk_band_solve_dev(ctx, rhs.data(), sol.ptr()));
      OK(pk_band_record(ctx, rec.data()));
      CHECK(same_bits(rec, want.rec) && same_bits(sol.fetch(), scattered(q, want.x[0])) && sol.fetch()[3] == 0.0);
    }
    Vec other = rhs;
    for (double& e : other) e = e * 0.5 + 0.125;
    const Ref want2 = reference(assembled(q, hv, jv, s1, s2, other));
    Guarded sol2(N);
    OK(pk_band_solve_dev(ctx, other.data(), sol2.ptr()));
    OK(pk_sync(ctx, nullptr));
    CHECK(same_bits(sol2.fetch(), scattered(q, want2.x[0])));
    // a singular band part: s1 = 0 and no Hessian entry on the diagonal of a variable no row reaches -- status 1, sol untouched
    Vec hz = hv, jz = jv, s1z = s1;
    std::fill(hz.begin(), hz.end(), 0.0); std::fill(jz.begin(), jz.end(), 0.0); std::fill(s1z.begin(), s1z.end(), 0.0);
    OK(pk_band_factor_dev(ctx, hz.data(), jz.data(), s1z.data(), s2.data()));
    Guarded sol3(N);
    Vec rec3(8);
    OK(pk_band_solve_dev(ctx, rhs.data(), sol3.ptr()));
    OK(pk_band_record(ctx, rec3.data()));
    CHECK(rec3[STATUS] == 1.0 && rec3[COLUMN] >= 0.0);
    for (double v : sol3.fetch()) CHECK(v == -77.0);
  }
  {  // the host form on the context's linearization against the device forms on the same values
    Vec x((size_t)n), lam((size_t)m);
    for (int i = 0; i < n; ++i) x[(size_t)i] = 2.0 * (double)(i % 9 - 4);
    for (int j = 0; j < m; ++j) lam[(size_t)j] = (double)(j % 5 - 2);
    OK(pk_linearize(ctx, x.data(), lam.data(), 2.0));
    Vec lj((size_t)q.A.nnz()), lh((size_t)q.Lo.nnz()), huge1((size_t)n), huge2((size_t)m);
    for (int64_t e = 0; e < q.A.nnz(); ++e) lj[(size_t)e] = fake_jac(x.data(), n, e, false);
    for (int64_t e = 0; e < q.Lo.nnz(); ++e) lh[(size_t)e] = fake_hess(x.data(), lam.data(), 2.0, n, m, e);
    for (int i = 0; i < n; ++i) huge1[(size_t)i] = 1.0e9 + 1.0e6 * (i % 5);
    for (int j = 0; j < m; ++j) huge2[(size_t)j] = 1.0e9 + 1.0e6 * (j % 3);
    Guarded hx(N), hrec(8), dx(N);
    Vec drec(8);
    OK(pk_solve_banded(ctx, huge1.data(), huge2.data(), rhs.data(), hx.ptr(), hrec.ptr()));
    OK(pk_band_factor_dev(ctx, lh.data(), lj.data(), huge1.data(), huge2.data()));
    OK(pk_band_solve_dev(ctx, rhs.data(), dx.ptr()));
    OK(pk_band_record(ctx, drec.data()));
    CHECK(drec[STATUS] == 0.0 && same_bits(hrec.fetch(), drec) && same_bits(hx.fetch(), dx.fetch()));
    const Ref want = reference(assembled(q, lh, lj, huge1, huge2, rhs));
    CHECK(same_bits(dx.fetch(), scattered(q, want.x[0])));
    // a factorisation that fails (every value zero but s2: a zero pivot) leaves the host form's x untouched and reports status 1
    OK(pk_linearize(ctx, x.data(), lam.data(), 0.0));
    Vec zero1((size_t)n, 0.0), lh0((size_t)q.Lo.nnz());
    for (int64_t e = 0; e < q.Lo.nnz(); ++e) lh0[(size_t)e] = fake_hess(x.data(), lam.data(), 0.0, n, m, e);
    Guarded fx(N), frec(8);
    bool all_zero = true;
    for (double v : lh0) all_zero = all_zero && v == 0.0;
    if (all_zero) {      // (sigma = 0 and these multipliers: only where the stand-in's Hessian vanishes with them)
      std::vector<double> jz((size_t)q.A.nnz(), 0.0);
      OK(pk_band_factor_dev(ctx, lh0.data(), jz.data(), zero1.data(), huge2.data()));
      Guarded sx(N);
      Vec srec(8);
      OK(pk_band_solve_dev(ctx, rhs.data(), sx.ptr()));
      OK(pk_band_record(ctx, srec.data()));
      CHECK(srec[STATUS] == 1.0);
      for (double v : sx.fetch()) CHECK(v == -77.0);
    }
    OK(pk_band_plan(ctx, q.nb, q.w, q.p, q.order.data(), q.map.data()));      // a plan replaces a plan
    Guarded later(N);
    CHECK(pk_band_solve_dev(ctx, rhs.data(), later.ptr()) == 134);            // ... and its factorisation is gone
    for (double v : later.fetch()) CHECK(v == -77.0);
    for (double v : fx.fetch()) CHECK(v == -77.0);
    for (double v : frec.fetch()) CHECK(v == -77.0);
  }

  // ---- what frees the state: a new problem, and pk_destroy leaves no live allocation
  CHECK(fake_hip_live_allocations() > 0);
  set_problem(400, 6, 11, 7);
  {
    Vec rec(8);
    CHECK(pk_band_record(ctx, rec.data()) == 134);
  }
  check_case(2 * NB + 1, 7, 3, PLAIN);                                        // (allocated again on first use)
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return checks_passed();
}
