// band_driver.cpp -- TEST INFRASTRUCTURE: drives the entry points of pockit_amd/csrc/pk_band.cpp (the bordered band LU of the
// step's system) against the host-only HIP stand-in of this directory, built with -fsanitize=address,undefined
// (tests/test_band_cpu.py): the stand-in walk of every kernel through the raw form against PLAIN LOOPS written here (an unblocked
// band LU, the sweeps, the pieced dots, the border) on full-mantissa data -- the arithmetic is the same, so a result must have
// the loops' BITS -- at Nb = 0, 1, 2, NB - 1, NB, NB + 1, 2 NB + 1 and w + 1, w = 0, 1, 7, NB - 1, NB, NB + 1 and the cap,
// p = 0, 1, 3 and the cap; NaN in the fill rows and outside the matrix (never read), every-column-interchanges, ties, a zero
// column, a planted NaN; the public forms against the raw form, the host form against the device forms, every refusal with its
// code and nothing enqueued or written behind it, a failed pivot leaving sol between its sentinels, and tear-down without a
// live allocation.  With --dump FILE: the system FILE describes (tests/test_band_cpu.py writes it from tests/band_cases.py)
// through the raw form, band, interchanges, solution and record printed as hex doubles.
#include <cmath>
#include <cstring>
#include <map>

#include "driver_common.h"

enum { NB = 32, W_CAP = 192, P_CAP = 8 };
enum { STATUS = 0, COLUMN = 1, PMIN = 2, PMAX = 3, R_NB = 4, R_W = 5, R_P = 6, SWAPS = 7 };
enum { PLAIN = 0, TINY = 1, TIES = 2, ZERO = 3, PLANT = 4 };
enum { EVERY = 70 };      // up to this Nb the tiny diagonal comes with a dominant subdiagonal: every column but the last interchanges
                          // (the row that is handed on shrinks by 2^-10 per column, so a long system of this kind is singular in fp64)

// ---------------------------------------------------------------- synthetic systems of full-mantissa values
static uint64_t g_state = 1;
static double unit() {      // in (-1, 1), 53 random bits
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  const double v = (double)(g_state >> 11) * 0x1p-53;
  return 2.0 * v - 1.0;
}

struct Sys {
  int64_t nb = 0;
  int w = 0, p = 0;
  int64_t ldab = 1;
  Vec band, U, C, rhs;      // band: NaN in the fill rows and outside the matrix
  double& at(int64_t i, int64_t j) { return band[(size_t)((2 * (int64_t)w + i - j) + j * ldab)]; }
};

static Sys make(int64_t nb, int w, int p, int variant) {
  g_state = 1000003ull * (uint64_t)nb + 7919ull * (uint64_t)w + 31ull * (uint64_t)p + (uint64_t)variant;
  Sys s;
  s.nb = nb; s.w = w; s.p = p; s.ldab = 3 * (int64_t)w + 1;
  s.band = made((size_t)(s.ldab * nb));
  std::fill(s.band.begin(), s.band.end(), NAN);
  for (int64_t j = 0; j < nb; ++j)
    for (int64_t i = std::max<int64_t>(0, j - w); i <= std::min<int64_t>(nb - 1, j + w); ++i) s.at(i, j) = unit();
  for (int64_t j = 0; j < nb; ++j) {
    const double d = (1.5 + 0.5 * unit()) * (unit() < 0.0 ? -1.0 : 1.0) * (0.25 * w + 1.0);
    s.at(j, j) = variant == TINY ? d * 0x1p-26 : d;
    if (variant == TINY && w > 0 && nb <= EVERY && j + 1 < nb) s.at(j + 1, j) = s.at(j + 1, j) * 1024.0 + (s.at(j + 1, j) < 0.0 ? -1024.0 : 1024.0);
  }
  if (variant == TIES && nb) {
    const double v = s.at(0, 0);
    for (int64_t i = 0; i <= std::min<int64_t>(w, nb - 1); ++i) s.at(i, 0) = i % 2 ? -v : v;
  }
  if (variant == ZERO && nb) {
    const int64_t j = 2 * nb / 3;
    for (int64_t i = std::max<int64_t>(0, j - w); i <= std::min<int64_t>(nb - 1, j + w); ++i) s.at(i, j) = 0.0;
  }
  if (variant == PLANT && nb) s.at(nb / 2, nb / 2) = NAN;
  s.U = made((size_t)(nb * p)); s.C = made((size_t)(p * p)); s.rhs = made((size_t)(nb + p));
  for (double& v : s.U) v = unit();
  for (double& v : s.C) v = unit();
  for (int k = 0; k < p; ++k) s.C[(size_t)(k + k * p)] += 4.0 + p;
  for (double& v : s.rhs) v = unit();
  return s;
}

// ---------------------------------------------------------------- the plain loops
struct Ref {
  Vec band, x, rec;
  std::vector<int32_t> ipiv;
};

static double tree(double* s) {
  for (int w = 128; w >= 1; w >>= 1)
    for (int t = 0; t < w; ++t) s[t] = s[t] + s[t + w];
  return s[0];
}

// u . y as the pieces and the scalar step associate it
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

static Ref reference(Sys s) {
  const int64_t nb = s.nb;
  const int w = s.w, p = s.p;
  Ref r;
  r.rec = {0.0, -1.0, INFINITY, 0.0, (double)nb, (double)w, (double)p, 0.0};
  r.ipiv.assign((size_t)nb, 0);
  for (int64_t j = 0; j < nb; ++j)      // the fill rows start as zeros
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
      r.band = s.band;
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
      for (int64_t i = j + 1; i <= j + km; ++i) {
        const double pr = s.at(i, j) * s.at(j, c);
        s.at(i, c) = s.at(i, c) - pr;
      }
    if ((j + 1) % NB == 0 || j == nb - 1) { r.rec[PMIN] = pmin; r.rec[PMAX] = pmax; r.rec[SWAPS] = swaps; }
  }
  r.band = s.band;
  Vec Y((size_t)(nb * (p + 1)));
  for (int64_t e = 0; e < nb * p; ++e) Y[(size_t)e] = s.U[(size_t)e];
  for (int64_t i = 0; i < nb; ++i) Y[(size_t)(nb * p + i)] = s.rhs[(size_t)i];
  for (int q = 0; q <= p; ++q) {
    double* y = Y.data() + (int64_t)q * nb;
    for (int64_t j = 0; j < nb; ++j) {
      const int64_t km = std::min<int64_t>(w, nb - 1 - j);
      std::swap(y[j], y[r.ipiv[(size_t)j]]);
      for (int64_t i = j + 1; i <= j + km; ++i) { const double pr = s.at(i, j) * y[j]; y[i] = y[i] - pr; }
    }
    for (int64_t k = nb - 1; k >= 0; --k) {
      y[k] = y[k] / s.at(k, k);
      for (int64_t i = std::max<int64_t>(0, k - 2 * w); i < k; ++i) { const double pr = s.at(i, k) * y[k]; y[i] = y[i] - pr; }
    }
  }
  r.x.assign((size_t)(nb + p), 0.0);
  if (p == 0) {
    for (int64_t i = 0; i < nb; ++i) r.x[(size_t)i] = Y[(size_t)i];
    return r;
  }
  Vec S((size_t)(p * p)), v((size_t)p);
  for (int c = 0; c < p; ++c)
    for (int a = 0; a < p; ++a) S[(size_t)(a + c * p)] = s.C[(size_t)(a + c * p)] - pieced_dot(s.U.data() + (int64_t)a * nb, Y.data() + (int64_t)c * nb, nb);
  for (int a = 0; a < p; ++a) v[(size_t)a] = s.rhs[(size_t)(nb + a)] - pieced_dot(s.U.data() + (int64_t)a * nb, Y.data() + (int64_t)p * nb, nb);
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
    double e = Y[(size_t)(nb * p + i)];
    for (int q = 0; q < p; ++q) { const double pr = Y[(size_t)(q * nb + i)] * v[(size_t)q]; e = e - pr; }
    r.x[(size_t)i] = e;
  }
  for (int q = 0; q < p; ++q) r.x[(size_t)(nb + q)] = v[(size_t)q];
  return r;
}

// ---------------------------------------------------------------- the raw form between sentinels
struct Got {
  Vec band, x, rec, ipiv;
};

static int raw(const Sys& s, Got& g) {
  Guarded band(s.band), x((size_t)(s.nb + s.p)), rec(8), piv((size_t)(s.nb + 1) / 2 + 1);      // (the interchanges: 32-bit, in a guarded array of doubles)
  const int rc = pk_band_raw_dev(ctx, s.nb, s.w, s.p, s.p + 1, band.ptr(), s.U.data(), s.C.data(), s.rhs.data(), (int32_t*)piv.ptr(), x.ptr(), rec.ptr());
  if (rc) return rc;
  OK(pk_sync(ctx, nullptr));
  g.band = band.fetch(); g.x = x.fetch(); g.rec = rec.fetch();
  const Vec pv = piv.fetch();
  g.ipiv.assign((size_t)s.nb, 0.0);
  for (int64_t j = 0; j < s.nb; ++j) g.ipiv[(size_t)j] = (double)((const int32_t*)pv.data())[j];
  return 0;
}

// same_bits, for vectors that may be empty
static bool bits(const Vec& a, const Vec& b) { return a.size() == b.size() && (a.empty() || same_bits(a, b)); }

static bool same_or_nan(const Vec& a, const Vec& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (std::memcmp(&a[i], &b[i], 8) != 0 && !(std::isnan(a[i]) && std::isnan(b[i]))) return false;
  return true;
}

// the slots outside the matrix still hold the caller's NaN; every slot of the matrix has the loops' bits
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

static int g_nb, g_w, g_p, g_variant;
static void check_case(int64_t nb, int w, int p, int variant) {
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
    if (!bits(got.x, want.x)) std::fprintf(stderr, "case nb %d w %d p %d variant %d: solution\n", g_nb, g_w, g_p, g_variant);
    CHECK(bits(got.x, want.x));
  } else {
    for (double v : got.x) CHECK(v == -77.0);      // a failed pivot leaves the solution untouched
  }
  if (variant == TINY && nb > 1 && w > 0) CHECK(nb <= EVERY ? got.rec[SWAPS] == (double)(nb - 1) : got.rec[SWAPS] >= (double)(nb / 4));
  if (variant == ZERO && nb) CHECK(got.rec[STATUS] == 1.0 && got.rec[COLUMN] == (double)(2 * nb / 3));
  if (variant == PLANT && nb) CHECK(got.rec[STATUS] == 3.0 && got.rec[COLUMN] == (double)(nb / 2));
}

static void print(const Vec& v) {
  for (double x : v) std::printf("%a\n", x);
}

// FILE: "nb w p", then band (ldab x nb, column-major), U, C, rhs
static int dump(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 3;
  long long nb;
  int w, p;
  if (std::fscanf(f, "%lld %d %d", &nb, &w, &p) != 3) return 3;
  Sys s;
  s.nb = nb; s.w = w; s.p = p; s.ldab = 3 * (int64_t)w + 1;
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

// ---------------------------------------------------------------- a small K with its plan, built by plain loops
struct Planned {
  int32_t n = 0, m = 0;
  Csr A, T, Lo, S;
  std::vector<int32_t> order, map;
  int64_t nb = 0;
  int w = 0, p = 0;
  std::vector<bool> fixed;
};

static Planned planned() {
  Planned q;
  const int32_t n = q.n = 30, m = q.m = 20;
  q.fixed.assign((size_t)n, false);
  q.fixed[3] = true;
  q.A.rows = m; q.A.cols = n;
  q.A.indptr.push_back(0);
  for (int32_t r = 0; r < m; ++r) {
    for (int32_t c : {r, r + 1, r + 4}) q.A.indices.push_back(c);
    q.A.indices.push_back(n - 1);      // the last variable is in every row: the border
    q.A.indptr.push_back((int32_t)q.A.indices.size());
  }
  q.T = transposed(q.A);
  q.Lo.rows = q.Lo.cols = n;
  q.Lo.indptr.push_back(0);
  for (int32_t r = 0; r < n; ++r) {
    if (r >= 1 && r % 6 != 5) q.Lo.indices.push_back(r - 1);
    if (r % 7 != 3) q.Lo.indices.push_back(r);
    q.Lo.indptr.push_back((int32_t)q.Lo.indices.size());
  }
  q.S = symmetric(q.Lo);
  // the permuted positions: variable i, row i, variable i + 1 ...; the last variable behind everything
  std::vector<int32_t> pos((size_t)(n + m), -1);
  for (int32_t i = 0; i < n - 1; ++i) {
    if (!q.fixed[(size_t)i]) { pos[(size_t)i] = (int32_t)q.order.size(); q.order.push_back(i); }
    if (i < m) { pos[(size_t)(n + i)] = (int32_t)q.order.size(); q.order.push_back(n + i); }
  }
  q.nb = (int64_t)q.order.size();
  q.p = 1;
  pos[(size_t)(n - 1)] = (int32_t)q.order.size();
  q.order.push_back(n - 1);
  // the entries of K: (caller row, caller column, signed source)
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

// the system the plan's map assembles from the four arrays, by plain loops
static Sys assembled(const Planned& q, const Vec& hv, const Vec& jv, const Vec& s1, const Vec& s2, const Vec& rhs) {
  Sys s;
  s.nb = q.nb; s.w = q.w; s.p = q.p; s.ldab = 3 * (int64_t)q.w + 1;
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
  for (int variant : {TIES, ZERO, PLANT}) {
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
      CHECK(same_bits(rec, want.rec) && same_bits(sol.fetch(), scattered(q, want.x)) && sol.fetch()[3] == 0.0);
    }
    Vec other = rhs;
    for (double& e : other) e = e * 0.5 + 0.125;
    const Ref want2 = reference(assembled(q, hv, jv, s1, s2, other));
    Guarded sol2(N);
    OK(pk_band_solve_dev(ctx, other.data(), sol2.ptr()));
    OK(pk_sync(ctx, nullptr));
    CHECK(same_bits(sol2.fetch(), scattered(q, want2.x)));
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
    CHECK(same_bits(dx.fetch(), scattered(q, want.x)));
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
