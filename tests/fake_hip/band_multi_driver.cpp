// band_multi_driver.cpp -- TEST INFRASTRUCTURE: drives the block solve of pockit_amd/csrc/pk_band.cpp (k right-hand sides against
// one factorisation: pk_band_raw_multi_dev, pk_band_solve_multi_dev, pk_solve_banded_multi) against the host-only HIP stand-in of
// this directory, built with -fsanitize=address,undefined (tests/test_band_multi_cpu.py).  The stand-in walk of every
// generalised kernel through the raw form against PLAIN LOOPS written here (one unblocked band LU, then per column the sweeps,
// the pieced dots, the border's LU with the column's t eliminated beside it, x_B) and against k calls of the single raw form,
// bit for bit, at Nb = 0, 1, 33, 65, 2 NB + 1 + 192, w = 0, 7, 33, 192, p = 0, 1, 8, k = 1, 2, 9, 64 (the k single calls at the cap
// of w only up to k = 9 and for the first and last column of 64: each of them factors again); strides n + m and n + m + 3 with
// NaN in the gaps of the right-hand sides and of the solutions, still NaN afterwards; a NaN planted in one column; a failed
// pivot leaving every column untouched; (8 200, 1, 1) with k = 64, whose elementwise kernels (prep, x_B, scatter) take their
// stride loops to a second trip, and (64 000, 1, 1) with k = 64, whose 65 * 32 dot items take the dot kernel's (the sweeps' grid
// holds p + k <= 72 workgroups: its loop cannot); the planned forms against pk_band_solve_dev column by column, the host form against the single host form;
// every refusal with its code, nothing enqueued and nothing written; tear-down without a live allocation.  With --dump FILE: the
// block FILE describes (tests/test_band_multi_cpu.py writes it from tests/band_multi_cases.py) through the raw form.
#include <cmath>
#include <cstring>
#include <map>

#include "driver_common.h"

enum { NB = 32, W_CAP = 192, P_CAP = 8, K_CAP = 64 };
enum { STATUS = 0, COLUMN = 1, PMIN = 2, PMAX = 3, R_NB = 4, R_W = 5, R_P = 6, SWAPS = 7 };

static uint64_t g_state = 1;
static double unit() {      // in (-1, 1), 53 random bits
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return 2.0 * ((double)(g_state >> 11) * 0x1p-53) - 1.0;
}

struct Sys {
  int64_t nb = 0, ldab = 1, stride = 0;
  int w = 0, p = 0, k = 1;
  Vec band, U, C, rhs;      // band: NaN in the fill rows and outside the matrix; rhs: k rows `stride` apart, NaN in the gaps
  double& at(int64_t i, int64_t j) { return band[(size_t)((2 * (int64_t)w + i - j) + j * ldab)]; }
  int64_t N() const { return nb + p; }
};

static Sys make(int64_t nb, int w, int p, int k, int gap, bool zero_column = false) {
  g_state = 1000003ull * (uint64_t)nb + 7919ull * (uint64_t)w + 31ull * (uint64_t)p + (uint64_t)k;
  Sys s;
  s.nb = nb; s.w = w; s.p = p; s.k = k; s.ldab = 3 * (int64_t)w + 1; s.stride = nb + p + gap;
  s.band = made((size_t)(s.ldab * nb));
  std::fill(s.band.begin(), s.band.end(), NAN);
  for (int64_t j = 0; j < nb; ++j)
    for (int64_t i = std::max<int64_t>(0, j - w); i <= std::min<int64_t>(nb - 1, j + w); ++i) s.at(i, j) = unit();
  for (int64_t j = 0; j < nb; ++j) s.at(j, j) = (1.5 + 0.5 * unit()) * (unit() < 0.0 ? -1.0 : 1.0) * (0.25 * w + 1.0);
  if (zero_column && nb) {
    const int64_t j = 2 * nb / 3;
    for (int64_t i = std::max<int64_t>(0, j - w); i <= std::min<int64_t>(nb - 1, j + w); ++i) s.at(i, j) = 0.0;
  }
  s.U = made((size_t)(nb * p)); s.C = made((size_t)(p * p));
  for (double& v : s.U) v = unit();
  for (double& v : s.C) v = unit();
  for (int q = 0; q < p; ++q) s.C[(size_t)(q + q * p)] += 4.0 + p;
  s.rhs = made((size_t)(s.stride * k));
  std::fill(s.rhs.begin(), s.rhs.end(), NAN);
  for (int c = 0; c < k; ++c)
    for (int64_t i = 0; i < s.N(); ++i) s.rhs[(size_t)(c * s.stride + i)] = unit();
  return s;
}

// ---------------------------------------------------------------- the plain loops
struct Ref {
  Vec band, rec;
  std::vector<Vec> x;      // per column; empty after a failure
  std::vector<int32_t> ipiv;
};

static double tree(double* s) {
  for (int w = 128; w >= 1; w >>= 1)
    for (int t = 0; t < w; ++t) s[t] = s[t] + s[t + w];
  return s[0];
}

static double pieced_dot(const double* u, const double* y, int64_t len) {
  const int64_t pieces = std::max<int64_t>(1, (len + 2047) / 2048);
  Vec partial((size_t)pieces);
  double s[256];
  for (int64_t pc = 0; pc < pieces; ++pc) {
    for (int t = 0; t < 256; ++t) {
      double acc = 0.0;
      for (int j = 0; j < 8; ++j) {
        const int64_t i = pc * 2048 + t + 256 * j;
        if (i < len) { const double pr = u[i] * y[i]; acc = acc + pr; }
      }
      s[t] = acc;
    }
    partial[(size_t)pc] = tree(s);
  }
  for (int t = 0; t < 256; ++t) {
    double acc = 0.0;
    for (int64_t pc = t; pc < pieces; pc += 256) acc = acc + partial[(size_t)pc];
    s[t] = acc;
  }
  return tree(s);
}

static void sweep(Sys& s, const std::vector<int32_t>& ipiv, double* y) {
  const int64_t nb = s.nb;
  const int w = s.w;
  for (int64_t j = 0; j < nb; ++j) {
    const int64_t km = std::min<int64_t>(w, nb - 1 - j);
    std::swap(y[j], y[ipiv[(size_t)j]]);
    for (int64_t i = j + 1; i <= j + km; ++i) { const double pr = s.at(i, j) * y[j]; y[i] = y[i] - pr; }
  }
  for (int64_t k = nb - 1; k >= 0; --k) {
    y[k] = y[k] / s.at(k, k);
    for (int64_t i = std::max<int64_t>(0, k - 2 * w); i < k; ++i) { const double pr = s.at(i, k) * y[k]; y[i] = y[i] - pr; }
  }
}

static Ref reference(Sys s) {
  const int64_t nb = s.nb;
  const int w = s.w, p = s.p;
  Ref r;
  r.rec = {0.0, -1.0, INFINITY, 0.0, (double)nb, (double)w, (double)p, 0.0};
  r.ipiv.assign((size_t)nb, 0);
  for (int64_t j = 0; j < nb; ++j)
    for (int64_t i = std::max<int64_t>(0, j - 2 * w); i < j - w; ++i) s.at(i, j) = 0.0;
  double pmin = INFINITY, pmax = 0.0, swaps = 0.0;
  for (int64_t j = 0; j < nb; ++j) {
    const int64_t km = std::min<int64_t>(w, nb - 1 - j), ju = std::min<int64_t>(j + 2 * w, nb - 1);
    int64_t ip = j;
    double big = -1.0;
    bool finite = true;
    for (int64_t i = j; i <= j + km; ++i) {
      const double e = s.at(i, j);
      if (!std::isfinite(e)) finite = false;
      if (std::fabs(e) > big) { big = std::fabs(e); ip = i; }
    }
    if (!finite || big == 0.0) {
      r.rec[STATUS] = finite ? 1.0 : 3.0; r.rec[COLUMN] = (double)j;
      return r;
    }
    r.ipiv[(size_t)j] = (int32_t)ip;
    pmin = std::min(pmin, big); pmax = std::max(pmax, big);
    if (ip != j) {
      swaps += 1.0;
      for (int64_t c = j; c <= ju; ++c) std::swap(s.at(j, c), s.at(ip, c));
    }
    for (int64_t i = j + 1; i <= j + km; ++i) s.at(i, j) = s.at(i, j) / s.at(j, j);
    for (int64_t c = j + 1; c <= ju; ++c)
      for (int64_t i = j + 1; i <= j + km; ++i) { const double pr = s.at(i, j) * s.at(j, c); s.at(i, c) = s.at(i, c) - pr; }
    if ((j + 1) % NB == 0 || j == nb - 1) { r.rec[PMIN] = pmin; r.rec[PMAX] = pmax; r.rec[SWAPS] = swaps; }
  }
  r.band = s.band;
  Vec YU = s.U;      // the border's columns, swept
  for (int q = 0; q < p; ++q) sweep(s, r.ipiv, YU.data() + (int64_t)q * nb);
  Vec S0((size_t)(p * p));
  for (int c = 0; c < p; ++c)
    for (int a = 0; a < p; ++a) S0[(size_t)(a + c * p)] = s.C[(size_t)(a + c * p)] - pieced_dot(s.U.data() + (int64_t)a * nb, YU.data() + (int64_t)c * nb, nb);
  for (int col = 0; col < s.k; ++col) {      // every column on its own: the border's LU again, with the column's t beside it
    const double* b = s.rhs.data() + (int64_t)col * s.stride;
    Vec y(b, b + nb), x((size_t)(nb + p), 0.0), S = S0, v((size_t)p);
    y.reserve((size_t)nb + 1);
    sweep(s, r.ipiv, y.data());
    for (int a = 0; a < p; ++a) v[(size_t)a] = b[nb + a] - pieced_dot(s.U.data() + (int64_t)a * nb, y.data(), nb);
    auto at = [&](int a, int c) -> double& { return S[(size_t)(a + c * p)]; };
    for (int k = 0; k < p; ++k) {
      int ip = k;
      double big = -1.0;
      for (int a = k; a < p; ++a) {
        const double mag = std::isfinite(at(a, k)) ? std::fabs(at(a, k)) : INFINITY;
        if (mag > big) { big = mag; ip = a; }
      }
      if (!std::isfinite(big) || big == 0.0) {
        r.rec[STATUS] = std::isfinite(big) ? 2.0 : 3.0; r.rec[COLUMN] = (double)(nb + k);
        r.x.clear();
        return r;
      }
      if (ip != k) {
        for (int c = 0; c < p; ++c) std::swap(at(k, c), at(ip, c));
        std::swap(v[(size_t)k], v[(size_t)ip]);
      }
      for (int a = k + 1; a < p; ++a) {
        const double l = at(a, k) / at(k, k);
        at(a, k) = l;
        for (int c = k + 1; c < p; ++c) { const double pr = l * at(k, c); at(a, c) = at(a, c) - pr; }
        const double pr = l * v[(size_t)k];
        v[(size_t)a] = v[(size_t)a] - pr;
      }
    }
    for (int k = p - 1; k >= 0; --k) {
      double e = v[(size_t)k];
      for (int c = k + 1; c < p; ++c) { const double pr = at(k, c) * v[(size_t)c]; e = e - pr; }
      v[(size_t)k] = e / at(k, k);
    }
    for (int64_t i = 0; i < nb; ++i) {
      double e = y[(size_t)i];
      for (int q = 0; q < p; ++q) { const double pr = YU[(size_t)(q * nb + i)] * v[(size_t)q]; e = e - pr; }
      x[(size_t)i] = e;
    }
    for (int q = 0; q < p; ++q) x[(size_t)(nb + q)] = v[(size_t)q];
    r.x.push_back(x);
  }
  return r;
}

// ---------------------------------------------------------------- the raw forms between sentinels
struct Got {
  Vec band, x, rec, ipiv;      // x: k rows `stride` apart, -77 in the slots and NaN in the gaps before the call
};

static Vec ipiv_of(const Vec& pv, int64_t nb) {
  Vec out((size_t)nb);
  for (int64_t j = 0; j < nb; ++j) out[(size_t)j] = (double)((const int32_t*)pv.data())[j];
  return out;
}

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

// column c alone through the single raw form
static void raw_single(const Sys& s, int c, Got& g) {
  Guarded band(s.band), x((size_t)s.N()), rec(8), piv((size_t)(s.nb + 1) / 2 + 1);
  OK(pk_band_raw_dev(ctx, s.nb, s.w, s.p, s.p + 1, band.ptr(), s.U.data(), s.C.data(), s.rhs.data() + (int64_t)c * s.stride, (int32_t*)piv.ptr(), x.ptr(),
                     rec.ptr()));
  OK(pk_sync(ctx, nullptr));
  g.band = band.fetch(); g.x = x.fetch(); g.rec = rec.fetch(); g.ipiv = ipiv_of(piv.fetch(), s.nb);
}

static bool bits(const Vec& a, const Vec& b) { return a.size() == b.size() && (a.empty() || same_bits(a, b)); }
static Vec column(const Sys& s, const Vec& x, int c) { return Vec(x.begin() + (long)(c * s.stride), x.begin() + (long)(c * s.stride + s.N())); }
static bool gaps_nan(const Sys& s, const Vec& x) {
  for (int c = 0; c < s.k; ++c)
    for (int64_t i = s.N(); i < s.stride; ++i)
      if (!std::isnan(x[(size_t)(c * s.stride + i)])) return false;
  return true;
}
static bool band_matches(const Sys& s, const Vec& got, const Vec& want) {
  for (int64_t j = 0; j < s.nb; ++j)
    for (int64_t r = 0; r < s.ldab; ++r) {
      const int64_t i = r - 2 * (int64_t)s.w + j;
      const size_t e = (size_t)(r + j * s.ldab);
      if (i < 0 || i >= s.nb) { if (!std::isnan(got[e])) return false; }
      else if (std::memcmp(&got[e], &want[e], 8) != 0) return false;
    }
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
    raw_single(s, c, one);
    const bool same = bits(one.rec, got.rec) && bits(one.ipiv, got.ipiv) && bits(one.x, column(s, got.x, c)) && band_matches(s, one.band, got.band);
    if (!same) { say_case(); std::fprintf(stderr, "  column %d against the single form\n", c); }
    CHECK(same);
  }
}

static void print(const Vec& v) {
  for (double x : v) std::printf("%a\n", x);
}

// FILE: "nb w p k stride", then band (ldab x nb, column-major), U, C, rhs (k x stride, row-major, "nan" in the gaps)
static int dump(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 3;
  long long nb, stride;
  int w, p, k;
  if (std::fscanf(f, "%lld %d %d %d %lld", &nb, &w, &p, &k, &stride) != 5) return 3;
  Sys s;
  s.nb = nb; s.w = w; s.p = p; s.k = k; s.stride = stride; s.ldab = 3 * (int64_t)w + 1;
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

// ---------------------------------------------------------------- a small K with its plan: n variables (one fixed), m rows, the
// last variable in every row (the border); H: a diagonal and one subdiagonal
struct Planned {
  int32_t n = 14, m = 8;
  Csr A, T, Lo, S;
  std::vector<int32_t> order, map;
  int64_t nb = 0;
  int w = 0, p = 1;
};

static Planned planned() {
  Planned q;
  const int32_t n = q.n, m = q.m, fixed = 3;
  q.A.rows = m; q.A.cols = n;
  q.A.indptr.push_back(0);
  for (int32_t r = 0; r < m; ++r) {
    for (int32_t c : {r, r + 1, r + 4}) q.A.indices.push_back(c);
    q.A.indices.push_back(n - 1);
    q.A.indptr.push_back((int32_t)q.A.indices.size());
  }
  q.T = transposed(q.A);
  q.Lo.rows = q.Lo.cols = n;
  q.Lo.indptr.push_back(0);
  for (int32_t r = 0; r < n; ++r) {
    if (r >= 1 && r % 5 != 4) q.Lo.indices.push_back(r - 1);
    q.Lo.indices.push_back(r);
    q.Lo.indptr.push_back((int32_t)q.Lo.indices.size());
  }
  q.S = symmetric(q.Lo);
  std::vector<int32_t> pos((size_t)(n + m), -1);
  for (int32_t i = 0; i < n - 1; ++i) {
    if (i != fixed) { pos[(size_t)i] = (int32_t)q.order.size(); q.order.push_back(i); }
    if (i < m) { pos[(size_t)(n + i)] = (int32_t)q.order.size(); q.order.push_back(n + i); }
  }
  q.nb = (int64_t)q.order.size();
  pos[(size_t)(n - 1)] = (int32_t)q.order.size();
  q.order.push_back(n - 1);
  struct Entry { int32_t r, c, code; };
  std::vector<Entry> entries;
  const int32_t nh = (int32_t)q.Lo.nnz(), nj = (int32_t)q.A.nnz();
  for (int32_t r = 0; r < n; ++r)
    for (int32_t e = q.Lo.indptr[(size_t)r]; e < q.Lo.indptr[(size_t)r + 1]; ++e) {
      const int32_t c = q.Lo.indices[(size_t)e];
      entries.push_back({r, c, e + 1});
      if (c != r) entries.push_back({c, r, e + 1});
    }
  for (int32_t i = 0; i < n; ++i) entries.push_back({i, i, nh + nj + i + 1});
  for (int32_t r = 0; r < m; ++r) {
    for (int32_t e = q.A.indptr[(size_t)r]; e < q.A.indptr[(size_t)r + 1]; ++e) {
      const int32_t c = q.A.indices[(size_t)e];
      entries.push_back({n + r, c, nh + e + 1});
      entries.push_back({c, n + r, nh + e + 1});
    }
    entries.push_back({n + r, n + r, -(nh + nj + n + r + 1)});
  }
  for (const Entry& e : entries) {
    const int32_t a = pos[(size_t)e.r], b = pos[(size_t)e.c];
    if (a >= 0 && b >= 0 && a < q.nb && b < q.nb) q.w = std::max(q.w, std::abs(a - b));
  }
  const int64_t ldab = 3 * (int64_t)q.w + 1, dests = ldab * q.nb + q.nb * q.p + q.p * q.p;
  std::map<int64_t, std::vector<int32_t>> slots;
  for (const Entry& e : entries) {
    const int64_t a = pos[(size_t)e.r], b = pos[(size_t)e.c];
    if (a < 0 || b < 0) continue;
    int64_t d = -1;
    if (a < q.nb && b < q.nb) d = (2 * q.w + a - b) + b * ldab;
    else if (a < q.nb) d = ldab * q.nb + (b - q.nb) * q.nb + a;
    else if (b >= q.nb) d = ldab * q.nb + q.nb * q.p + (a - q.nb) + (b - q.nb) * q.p;
    if (d >= 0) slots[d].push_back(e.code);
  }
  q.map.assign((size_t)(2 * dests), 0);
  for (auto& kv : slots) {
    std::sort(kv.second.begin(), kv.second.end(), [](int32_t x, int32_t y) { return std::abs(x) < std::abs(y); });
    if (kv.second.size() > 2) std::exit(2);
    for (size_t k = 0; k < kv.second.size(); ++k) q.map[(size_t)(2 * kv.first) + k] = kv.second[k];
  }
  return q;
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
    raw_single(s, 2, one);
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
