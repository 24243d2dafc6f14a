// merit_driver.cpp -- TEST INFRASTRUCTURE: drives the merit entry points (pk_set_bounds, pk_trial_points_dev, pk_merit_reduce_dev,
// pk_merit_batch_dev, pk_merit_scan, pk_merit_batch; pockit_amd/csrc/pk_merit.cpp) against the host-only HIP stand-in of this
// directory, built with -fsanitize=address,undefined (tests/test_merit_cpu.py).  The host walk of pk_trial / pk_merit /
// pk_merit_fin on small-integer data: every difference, square, product and sum is exact in fp64, so a row must EQUAL a plain
// loop.  Lengths around the piece size and 524 289 (257 pieces: the second strided trip of pk_merit_fin), B up to 64, leading
// dimensions larger than the lengths with NaN in the padding, infinite bounds, non-finite g / grad / f entries counted and
// left out, d absent, trial points against volatile temporaries, sentinels around out, every refusal, the partial rows and the
// scratch growing, tear-down by pk_set_problem and pk_destroy.  (Error 127, a failed allocation, is not reached: the
// stand-in's hipMalloc never fails.)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "driver_common.h"
#include "../../pockit_amd/csrc/pk_runtime.h"      // (the context's merit area: d_bounds, partial_cap, scratch_cap)

static const double INF = std::numeric_limits<double>::infinity();
static const double NAN_ = std::numeric_limits<double>::quiet_NaN();

static double viol(double v, double lo, double hi) { return std::max(std::max(lo - v, v - hi), 0.0); }

// the reference: one plain loop per column
static void plain_row(int64_t n_g, const double* g, const double* clb, const double* cub, int64_t n_x, const double* X,
                      const double* vlb, const double* vub, const double* grad, const double* d, double f, double* row) {
  for (int q = 0; q < 8; ++q) row[q] = 0.0;
  row[0] = f;
  if (!std::isfinite(f)) row[7] += 1.0;
  for (int64_t i = 0; i < n_g; ++i) {
    if (!std::isfinite(g[i])) { row[7] += 1.0; continue; }
    const double w = viol(g[i], clb[i], cub[i]);
    row[1] += w; row[2] = std::max(row[2], w); row[3] += w * w;
  }
  for (int64_t i = 0; i < n_x; ++i) {
    const double w = viol(X[i], vlb[i], vub[i]);
    row[4] += w; row[5] = std::max(row[5], w);
    if (!std::isfinite(grad[i])) row[7] += 1.0;
    else if (d) row[6] += grad[i] * d[i];
  }
}

static bool same_row(const double* a, const double* b) {
  for (int q = 0; q < 8; ++q)
    if (!(a[q] == b[q] || (std::isnan(a[q]) && std::isnan(b[q])))) return false;
  return true;
}

static double small(int64_t k, int mod, int shift) { return (double)((k * 31 + 7) % mod - shift); }

// lower / upper bounds of small integers, every seventh lower and every fifth upper one infinite (every 35th both)
static void make_bounds(int64_t len, int salt, std::vector<double>& lo, std::vector<double>& hi) {
  lo.resize((size_t)len); hi.resize((size_t)len);
  for (int64_t i = 0; i < len; ++i) {
    lo[(size_t)i] = (i + salt) % 7 == 0 ? -INF : small(i + salt, 5, 4);       // -4 ... 0
    hi[(size_t)i] = (i + salt) % 5 == 0 ? INF : small(i + 3 * salt, 4, 0);    //  0 ... 3
  }
}

// one synthetic reduction through pk_merit_reduce_dev: g of n_g values, X and grad of n_x, B entries, rows padded with NaN
static void reduce_case(int B, int64_t n_g, int64_t n_x, bool with_d, bool poison) {
  const int64_t ldg = n_g + 3, ldx = n_x + 2, ldgrad = n_x + 5;
  std::vector<double> g((size_t)(B * ldg), NAN_), X((size_t)(B * ldx), NAN_), grad((size_t)(B * ldgrad), NAN_), f((size_t)B), d((size_t)n_x);
  std::vector<double> clb, cub, vlb, vub;
  make_bounds(n_g, 1, clb, cub);
  make_bounds(n_x, 4, vlb, vub);
  for (int64_t i = 0; i < n_x; ++i) d[(size_t)i] = small(i, 9, 4);
  for (int b = 0; b < B; ++b) {
    f[(size_t)b] = (double)(3 * b - 5);
    for (int64_t i = 0; i < n_g; ++i) g[(size_t)(b * ldg + i)] = small(i + 11 * b, 17, 8);
    for (int64_t i = 0; i < n_x; ++i) {
      X[(size_t)(b * ldx + i)] = small(i + 5 * b, 13, 6);
      grad[(size_t)(b * ldgrad + i)] = small(i + 3 * b, 11, 5);
    }
  }
  if (poison) {      // non-finite entries: counted, and left out of every other column
    const int b = B - 1;
    if (n_g > 0) { g[(size_t)(b * ldg)] = NAN_; g[(size_t)(b * ldg + n_g - 1)] = INF; g[(size_t)(b * ldg + n_g / 2)] = -INF; }
    if (n_x > 0) { grad[(size_t)(b * ldgrad + n_x - 1)] = NAN_; grad[(size_t)(b * ldgrad + n_x / 3)] = -INF; }
    f[0] = NAN_;
    if (B > 1) f[(size_t)b] = INF;
  }
  std::vector<double> out((size_t)(B * 8 + 8), SENTINEL), want(8);
  double* o = out.data() + 4;
  OK(pk_merit_reduce_dev(ctx, B, n_g, g.data(), ldg, clb.data(), cub.data(), n_x, X.data(), ldx, vlb.data(), vub.data(), grad.data(),
                         ldgrad, with_d ? d.data() : nullptr, f.data(), o, nullptr));
  OK(pk_sync(ctx, nullptr));
  for (int k = 0; k < 4; ++k) CHECK(out[(size_t)k] == SENTINEL && out[(size_t)(B * 8 + 4 + k)] == SENTINEL);
  double bad_total = 0.0;
  for (int b = 0; b < B; ++b) {
    plain_row(n_g, g.data() + b * ldg, clb.data(), cub.data(), n_x, X.data() + b * ldx, vlb.data(), vub.data(),
              grad.data() + b * ldgrad, with_d ? d.data() : nullptr, f[(size_t)b], want.data());
    CHECK(same_row(o + 8 * b, want.data()));
    for (int q = 1; q < 7; ++q) CHECK(std::isfinite(o[8 * b + q]));
    if (!with_d) CHECK(o[8 * b + 6] == 0.0);
    bad_total += o[8 * b + 7];
  }
  if (poison) CHECK(bad_total >= 1.0);      // (f[0] at least; the rows themselves were compared above)
  else CHECK(bad_total == 0.0);
  CHECK(ctx->merit.partial_cap >= (size_t)B * (size_t)std::max<int64_t>(1, (std::max(n_g, n_x) + 2047) / 2048) * 8);
}

int main() {
  load_model();
  const int32_t n = 40, m = 30;
  const int64_t nnz_J = 200;
  {
    double one = 1.0;
    CHECK(pk_set_bounds(ctx, &one, &one, &one, &one) == 3);      // no problem yet
  }
  set_problem(n, m, nnz_J, 150);

  // ---- the reduction on synthetic vectors: every length at which the walk changes, on both sides; the partial rows grow
  //      with the largest (entries x pieces) seen and never shrink
  CHECK(ctx->merit.d_partial == nullptr && ctx->merit.partial_cap == 0);
  const int64_t LENS[] = {0, 1, 255, 256, 257, 2047, 2048, 2049};
  const int BS[] = {1, 2, 3, 64};
  size_t cap_seen = 0;
  for (int k = 0; k < 8; ++k)
    for (const int B : BS) {
      reduce_case(B, LENS[k], LENS[(k + 3) % 8], (k + B) % 2 == 0, (k + B) % 3 == 0);
      CHECK(ctx->merit.partial_cap >= cap_seen);
      cap_seen = ctx->merit.partial_cap;
    }
  reduce_case(3, 2049, 2049, true, true);
  CHECK(ctx->merit.partial_cap == cap_seen);                       // 3 x 2 rows fit what 64 x 2 rows left
  {
    const double* before = ctx->merit.d_partial;
    reduce_case(2, 524289, 2049, true, true);                      // 257 pieces: pk_merit_fin's second strided trip
    CHECK(ctx->merit.partial_cap == 2u * 257u * 8u && ctx->merit.d_partial != before);
    reduce_case(1, 255, 524289, false, true);                      // ... with X and grad the long side
    reduce_case(3, 524289, 524289, true, false);
    CHECK(ctx->merit.partial_cap == 3u * 257u * 8u);
    reduce_case(64, 1, 1, true, false);
    CHECK(ctx->merit.partial_cap == 3u * 257u * 8u);
  }

  // ---- trial points: x + alpha d with the product rounded first, against volatile temporaries; padding untouched
  {
    const int64_t ldx = n + 3;
    std::vector<double> x((size_t)n), d((size_t)n), alpha(64);
    for (int i = 0; i < n; ++i) {
      x[(size_t)i] = 1.0 / 3.0 + 0.1 * i;
      d[(size_t)i] = std::sqrt(2.0 + i) * (i % 2 ? -1.0 : 1.0);
    }
    for (int b = 0; b < 64; ++b) alpha[(size_t)b] = std::ldexp(1.0 / 7.0 + b, -b / 4);
    for (const int B : BS) {
      std::vector<double> X((size_t)(B * ldx), SENTINEL);
      OK(pk_trial_points_dev(ctx, B, x.data(), d.data(), alpha.data(), X.data(), ldx, nullptr));
      OK(pk_sync(ctx, nullptr));
      for (int b = 0; b < B; ++b) {
        for (int i = 0; i < n; ++i) {
          volatile double prod = alpha[(size_t)b] * d[(size_t)i];
          volatile double sum = x[(size_t)i] + prod;
          CHECK(X[(size_t)(b * ldx + i)] == sum);
        }
        for (int64_t i = n; i < ldx; ++i) CHECK(X[(size_t)(b * ldx + i)] == SENTINEL);
      }
    }
  }

  // ---- every refusal: its code, nothing enqueued, nothing written
  std::vector<double> x((size_t)n), d((size_t)n), alpha(200), clb, cub, vlb, vub;
  for (int i = 0; i < n; ++i) { x[(size_t)i] = (double)(i % 5 - 2); d[(size_t)i] = (double)(i % 3 - 1); }
  for (int b = 0; b < 200; ++b) alpha[(size_t)b] = (double)(b % 9 - 3);
  make_bounds(m, 2, clb, cub);
  make_bounds(n, 3, vlb, vub);
  {
    std::vector<double> f(2, 0.0), g((size_t)(2 * m), 0.0), grad((size_t)(2 * n), 0.0), X((size_t)(2 * n), 0.0), out(16, SENTINEL);
    double *pf = f.data(), *pg = g.data(), *pgr = grad.data(), *pX = X.data(), *po = out.data();
    const size_t mark = fake_hip_log().size(), launches = fake_hip_launches().size(), live = fake_hip_live_allocations();
    CHECK(pk_merit_batch_dev(ctx, 2, pf, pg, m, pgr, n, pX, n, nullptr, po, nullptr) == 123);      // bounds not set
    CHECK(pk_merit_scan(ctx, 2, x.data(), d.data(), alpha.data(), po) == 123);
    CHECK(pk_merit_batch(ctx, 2, pX, n, nullptr, po) == 123);
    CHECK(pk_set_bounds(ctx, nullptr, cub.data(), vlb.data(), vub.data()) == 126);                  // bounds rejected
    CHECK(pk_set_bounds(ctx, clb.data(), cub.data(), vlb.data(), nullptr) == 126);
    {
      std::vector<double> bad = clb;
      bad[3] = NAN_;
      CHECK(pk_set_bounds(ctx, bad.data(), cub.data(), vlb.data(), vub.data()) == 126);
      CHECK(pk_set_bounds(ctx, clb.data(), bad.data(), vlb.data(), vub.data()) == 126);
      bad = vlb;
      bad[(size_t)n - 1] = 100.0;
      CHECK(pk_set_bounds(ctx, clb.data(), cub.data(), bad.data(), vub.data()) == 126);            // lower above upper
    }
    CHECK(ctx->merit.d_bounds == nullptr && fake_hip_live_allocations() == live);
    OK(pk_set_bounds(ctx, clb.data(), cub.data(), vlb.data(), vub.data()));
    CHECK(fake_hip_live_allocations() == live + 1);
    OK(pk_set_bounds(ctx, clb.data(), cub.data(), vlb.data(), vub.data()));                        // replaced, not added to
    CHECK(fake_hip_live_allocations() == live + 1);
    const size_t mark2 = fake_hip_log().size();
    CHECK(pk_merit_batch_dev(ctx, 0, pf, pg, m, pgr, n, pX, n, nullptr, po, nullptr) == 124);      // B
    CHECK(pk_merit_batch_dev(ctx, PK_MAX_BATCH + 1, pf, pg, m, pgr, n, pX, n, nullptr, po, nullptr) == 124);
    CHECK(pk_trial_points_dev(ctx, 0, x.data(), d.data(), alpha.data(), pX, n, nullptr) == 124);
    CHECK(pk_trial_points_dev(ctx, PK_MAX_BATCH + 1, x.data(), d.data(), alpha.data(), pX, n, nullptr) == 124);
    CHECK(pk_merit_reduce_dev(ctx, -1, m, pg, m, clb.data(), cub.data(), n, pX, n, vlb.data(), vub.data(), pgr, n, nullptr, pf, po, nullptr) == 124);
    CHECK(pk_merit_scan(ctx, 0, x.data(), d.data(), alpha.data(), po) == 124);
    CHECK(pk_merit_batch(ctx, -3, pX, n, nullptr, po) == 124);
    CHECK(pk_merit_batch_dev(ctx, 2, pf, pg, m - 1, pgr, n, pX, n, nullptr, po, nullptr) == 125);  // leading dimensions
    CHECK(pk_merit_batch_dev(ctx, 2, pf, pg, m, pgr, n - 1, pX, n, nullptr, po, nullptr) == 125);
    CHECK(pk_merit_batch_dev(ctx, 2, pf, pg, m, pgr, n, pX, n - 1, nullptr, po, nullptr) == 125);
    CHECK(pk_trial_points_dev(ctx, 2, x.data(), d.data(), alpha.data(), pX, n - 1, nullptr) == 125);
    CHECK(pk_merit_batch(ctx, 2, pX, n - 1, nullptr, po) == 125);
    CHECK(pk_merit_reduce_dev(ctx, 2, -1, pg, m, clb.data(), cub.data(), n, pX, n, vlb.data(), vub.data(), pgr, n, nullptr, pf, po, nullptr) == 125);
    CHECK(pk_merit_batch_dev(ctx, 2, nullptr, pg, m, pgr, n, pX, n, nullptr, po, nullptr) == 128);  // null device pointers
    CHECK(pk_merit_batch_dev(ctx, 2, pf, nullptr, m, pgr, n, pX, n, nullptr, po, nullptr) == 128);
    CHECK(pk_merit_batch_dev(ctx, 2, pf, pg, m, nullptr, n, pX, n, nullptr, po, nullptr) == 128);
    CHECK(pk_merit_batch_dev(ctx, 2, pf, pg, m, pgr, n, nullptr, n, nullptr, po, nullptr) == 128);
    CHECK(pk_merit_batch_dev(ctx, 2, pf, pg, m, pgr, n, pX, n, nullptr, nullptr, nullptr) == 128);
    CHECK(pk_trial_points_dev(ctx, 2, nullptr, d.data(), alpha.data(), pX, n, nullptr) == 128);
    CHECK(pk_trial_points_dev(ctx, 2, x.data(), d.data(), nullptr, pX, n, nullptr) == 128);
    CHECK(pk_trial_points_dev(ctx, 2, x.data(), d.data(), alpha.data(), nullptr, n, nullptr) == 128);
    CHECK(pk_merit_scan(ctx, 2, nullptr, d.data(), alpha.data(), po) == 60);                       // null host buffers
    CHECK(pk_merit_scan(ctx, 2, x.data(), nullptr, alpha.data(), po) == 60);
    CHECK(pk_merit_scan(ctx, 2, x.data(), d.data(), nullptr, po) == 60);
    CHECK(pk_merit_scan(ctx, 2, x.data(), d.data(), alpha.data(), nullptr) == 60);
    CHECK(pk_merit_batch(ctx, 2, nullptr, n, nullptr, po) == 60 && pk_merit_batch(ctx, 2, pX, n, nullptr, nullptr) == 60);
    OK(pk_set_cycle_layout(ctx, 0, 0));
    ctx->cycle_layout = 1;                                                                          // a compact cycle layout
    CHECK(pk_merit_scan(ctx, 2, x.data(), d.data(), alpha.data(), po) == 88);
    CHECK(pk_merit_batch(ctx, 2, pX, n, nullptr, po) == 88);
    ctx->cycle_layout = 0;
    ctx->exchange.in_launch = true; ctx->exchange.world = 2;                                        // the in-launch exchange
    CHECK(pk_merit_scan(ctx, 2, x.data(), d.data(), alpha.data(), po) == 88);
    CHECK(pk_merit_batch(ctx, 2, pX, n, nullptr, po) == 88);
    ctx->exchange.in_launch = false; ctx->exchange.world = 0;
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark2 && fake_hip_launches().size() == launches && mark2 >= mark);
    for (double v : out) CHECK(v == SENTINEL);
    CHECK(ctx->merit.d_scratch == nullptr && ctx->merit.scratch_cap == 0);      // a refused call allocates nothing
  }

  // ---- the host forms, served by the loop of single cycles (no batched object: the stand-in's kernels write recomputable
  //      values): the scan against the plain loop on x + a d, the batch form on the same points, leading dimension with NaN
  //      padding, d absent; 130 entries walk three chunks; the scratch grows with the chunk and stays
  auto expect = [&](const double* xb, const double* dd, double* row) {
    std::vector<double> g((size_t)m), grad((size_t)n);
    for (int j = 0; j < m; ++j) g[(size_t)j] = fake_g(xb, n, j);
    for (int i = 0; i < n; ++i) grad[(size_t)i] = fake_grad(xb, n, i);
    plain_row(m, g.data(), clb.data(), cub.data(), n, xb, vlb.data(), vub.data(), grad.data(), dd, fake_f(xb, n), row);
  };
  size_t scratch_seen = 0;
  for (const int64_t B : {2, 1, 64, 130, 3}) {
    const int64_t ldx = n + 2;
    std::vector<double> out((size_t)(8 * B + 8), SENTINEL), out_b((size_t)(8 * B), SENTINEL), out_n((size_t)(8 * B), SENTINEL);
    std::vector<double> X((size_t)(B * ldx), NAN_), want(8);
    OK(pk_merit_scan(ctx, B, x.data(), d.data(), alpha.data(), out.data() + 4));
    for (int k = 0; k < 4; ++k) CHECK(out[(size_t)k] == SENTINEL && out[(size_t)(8 * B + 4 + k)] == SENTINEL);
    for (int64_t b = 0; b < B; ++b)
      for (int i = 0; i < n; ++i) X[(size_t)(b * ldx + i)] = x[(size_t)i] + alpha[(size_t)b] * d[(size_t)i];
    OK(pk_merit_batch(ctx, B, X.data(), ldx, d.data(), out_b.data()));
    OK(pk_merit_batch(ctx, B, X.data(), ldx, nullptr, out_n.data()));
    bool some_theta = false, some_bound = false;
    for (int64_t b = 0; b < B; ++b) {
      expect(X.data() + b * ldx, d.data(), want.data());
      CHECK(same_row(out.data() + 4 + 8 * b, want.data()) && same_row(out_b.data() + 8 * b, want.data()));
      expect(X.data() + b * ldx, nullptr, want.data());
      CHECK(same_row(out_n.data() + 8 * b, want.data()) && out_n[(size_t)(8 * b + 6)] == 0.0);
      some_theta |= want[1] > 0.0;
      some_bound |= want[4] > 0.0;
    }
    CHECK(some_theta && some_bound);
    CHECK(ctx->merit.scratch_cap >= scratch_seen && ctx->merit.scratch_cap > 0);
    scratch_seen = ctx->merit.scratch_cap;
  }
  {
    const size_t cnt = 64, per = 2 * (size_t)n + (size_t)m + (size_t)nnz_J + 1 + 8;
    CHECK(ctx->merit.scratch_cap == 2 * (size_t)n + cnt * per);     // the chunk of this problem is PK_MAX_BATCH
  }

  // ---- with the batched object: ONE launch of pk_cycleb per chunk, one synchronize for the call
  {
    OK(pk_load_batch_model(ctx, image, sizeof image));
    std::vector<double> out(8 * 130);
    int64_t before = 0, after = 0;
    OK(pk_batch_launches(ctx, &before));
    size_t launches = fake_hip_launches().size();
    OK(pk_merit_scan(ctx, 130, x.data(), d.data(), alpha.data(), out.data()));
    OK(pk_batch_launches(ctx, &after));
    CHECK(after - before == 3 && fake_hip_launches().size() == launches + 3 && fake_hip_launches().back().kernel == "pk_cycleb");
    OK(pk_merit_batch(ctx, 5, out.data(), n, nullptr, out.data() + 500));
    OK(pk_batch_launches(ctx, &before));
    CHECK(before - after == 1);
    OK(pk_load_batch_model(ctx, nullptr, 0));
  }

  // ---- a problem whose Jacobian bounds the chunk: 256 MiB / (8 (nnz_J + n + m + 1)) = 8 entries, 9 entries walk two chunks
  {
    const int64_t big = 4000000;
    set_problem(n, m, big, 150);
    CHECK(ctx->merit.d_bounds == nullptr && ctx->merit.d_partial == nullptr && ctx->merit.d_scratch == nullptr);      // torn down
    CHECK(ctx->merit.partial_cap == 0 && ctx->merit.scratch_cap == 0);
    std::vector<double> out(8 * 9, SENTINEL), want(8), xb((size_t)n);
    CHECK(pk_merit_scan(ctx, 9, x.data(), d.data(), alpha.data(), out.data()) == 123);                              // ... the bounds too
    OK(pk_set_bounds(ctx, clb.data(), cub.data(), vlb.data(), vub.data()));
    OK(pk_merit_scan(ctx, 9, x.data(), d.data(), alpha.data(), out.data()));
    CHECK((256ll << 20) / (8 * (big + n + m + 1)) == 8);
    CHECK(ctx->merit.scratch_cap == 2 * (size_t)n + 8 * (2 * (size_t)n + (size_t)m + (size_t)big + 1 + 8));
    for (int b = 0; b < 9; ++b) {
      for (int i = 0; i < n; ++i) xb[(size_t)i] = x[(size_t)i] + alpha[(size_t)b] * d[(size_t)i];
      expect(xb.data(), d.data(), want.data());
      CHECK(same_row(out.data() + 8 * b, want.data()));
    }
  }
  // ---- torn down with live bounds, partial rows and scratch
  CHECK(ctx->merit.d_bounds && ctx->merit.d_partial && ctx->merit.d_scratch);
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return checks_passed();
}
