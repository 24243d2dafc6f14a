// band_driver_common.h -- TEST INFRASTRUCTURE: what the three drivers of pockit_amd/csrc/pk_band.cpp share (band_driver.cpp,
// band_batch_driver.cpp, band_multi_driver.cpp; header-only, beside driver_common.h): the generator of full-mantissa systems, the
// PLAIN LOOPS every form is held to (one unblocked band LU, then per right-hand side the sweeps, the pieced dots, the border's
// LU with the column's t eliminated beside it, x_B), the single raw form between sentinels, the bitwise comparisons, the hex
// print of --dump and the small planned K.  Each driver keeps its own cases, checks and refusals.
#ifndef FAKE_HIP_BAND_DRIVER_COMMON_H
#define FAKE_HIP_BAND_DRIVER_COMMON_H

#include <cmath>
#include <cstring>
#include <map>

#include "driver_common.h"

enum { NB = 32, W_CAP = 192, P_CAP = 8, BATCH_CAP = 16, K_CAP = 64, REC = 8 };
enum { STATUS = 0, COLUMN = 1, PMIN = 2, PMAX = 3, R_NB = 4, R_W = 5, R_P = 6, SWAPS = 7 };
enum Variant { PLAIN, TINY, TIES, ZERO, PLANT };
enum { EVERY = 70 };      // up to this Nb the tiny diagonal comes with a dominant subdiagonal: every column but the last interchanges
                          // (the row that is handed on shrinks by 2^-10 per column, so a long system of this kind is singular in fp64)

// ---------------------------------------------------------------- synthetic systems of full-mantissa values
inline uint64_t g_state = 1;
inline double unit() {      // in (-1, 1), 53 random bits
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  const double v = (double)(g_state >> 11) * 0x1p-53;
  return 2.0 * v - 1.0;
}

struct Sys {
  int64_t nb = 0, ldab = 1, stride = 0;
  int w = 0, p = 0, k = 1;
  Vec band, U, C, rhs;      // band: NaN in the fill rows and outside the matrix; rhs: k rows `stride` apart, NaN in the gaps
  double& at(int64_t i, int64_t j) { return band[(size_t)((2 * (int64_t)w + i - j) + j * ldab)]; }
  int64_t N() const { return nb + p; }
};

// a system a driver read or assembled itself: one right-hand side behind the matrix
inline Sys shaped(int64_t nb, int w, int p, int k = 1, int64_t stride = -1) {
  Sys s;
  s.nb = nb; s.w = w; s.p = p; s.k = k; s.ldab = 3 * (int64_t)w + 1; s.stride = stride < 0 ? nb + p : stride;
  return s;
}

// The seed is 1000003 Nb + 7919 w + 31 p + code + 104729 salt: `code` is the term a driver adds for its own case (its number of
// the variant, or k), so that every driver's cases are the systems they always were.  k right-hand sides at stride Nb + p + gap.
inline Sys make_system(int64_t nb, int w, int p, Variant variant, uint64_t code, uint64_t salt, int k, int gap) {
  g_state = 1000003ull * (uint64_t)nb + 7919ull * (uint64_t)w + 31ull * (uint64_t)p + code + 104729ull * salt;
  Sys s = shaped(nb, w, p, k, nb + p + gap);
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
  Vec band, rec;           // band: after the LU (as far as it got, after a failed pivot)
  std::vector<Vec> x;      // per column; empty after a failure
  std::vector<int32_t> ipiv;
};

inline double tree(double* s) {
  for (int w = 128; w >= 1; w >>= 1)
    for (int t = 0; t < w; ++t) s[t] = s[t] + s[t + w];
  return s[0];
}

// u . y as the pieces and the scalar step associate it
inline double pieced_dot(const double* u, const double* y, int64_t len) {
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

inline void sweep(Sys& s, const std::vector<int32_t>& ipiv, double* y) {
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

inline Ref reference(Sys s) {
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

// ---------------------------------------------------------------- the single raw form between sentinels
struct Got {
  Vec band, x, rec, ipiv;      // ipiv: the 32-bit interchanges as doubles
};

inline Vec ipiv_of(const Vec& pv, int64_t nb) {      // (the interchanges: 32-bit, in a guarded array of doubles)
  Vec out((size_t)nb);
  for (int64_t j = 0; j < nb; ++j) out[(size_t)j] = (double)((const int32_t*)pv.data())[j];
  return out;
}

// right-hand side c of the system alone; an interchange the call did not write reads -7
inline int raw_single(const Sys& s, int c, Got& g) {
  Guarded band(s.band), x((size_t)s.N()), rec(REC), piv((size_t)(s.nb + 1) / 2 + 1);
  for (size_t j = 0; j < 2 * piv.count; ++j) ((int32_t*)piv.ptr())[j] = -7;
  const int rc = pk_band_raw_dev(ctx, s.nb, s.w, s.p, s.p + 1, band.ptr(), s.U.data(), s.C.data(), s.rhs.data() + (int64_t)c * s.stride,
                                 (int32_t*)piv.ptr(), x.ptr(), rec.ptr());
  if (rc) return rc;
  OK(pk_sync(ctx, nullptr));
  g.band = band.fetch(); g.x = x.fetch(); g.rec = rec.fetch(); g.ipiv = ipiv_of(piv.fetch(), s.nb);
  return 0;
}

// ---------------------------------------------------------------- comparisons and the print of --dump
// same_bits, for vectors that may be empty
inline bool bits(const Vec& a, const Vec& b) { return a.size() == b.size() && (a.empty() || same_bits(a, b)); }

inline bool same_or_nan(const double* a, const double* b, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (std::memcmp(a + i, b + i, 8) != 0 && !(std::isnan(a[i]) && std::isnan(b[i]))) return false;
  return true;
}
inline bool same_or_nan(const Vec& a, const Vec& b) { return a.size() == b.size() && same_or_nan(a.data(), b.data(), a.size()); }

// the slots outside the matrix still hold the caller's NaN; every slot of the matrix (the fill rows too) has the loops' bits
inline bool band_matches(const Sys& s, const double* got, const Vec& want) {
  for (int64_t j = 0; j < s.nb; ++j)
    for (int64_t r = 0; r < s.ldab; ++r) {
      const int64_t i = r - 2 * (int64_t)s.w + j;
      const size_t e = (size_t)(r + j * s.ldab);
      if (i < 0 || i >= s.nb) { if (!std::isnan(got[e])) return false; }
      else if (std::memcmp(&got[e], &want[e], 8) != 0) return false;
    }
  return true;
}
inline bool band_matches(const Sys& s, const Vec& got, const Vec& want) { return band_matches(s, got.data(), want); }

inline void print(const double* v, int64_t count) {
  for (int64_t i = 0; i < count; ++i) std::printf("%a\n", v[i]);
}
inline void print(const Vec& v) { print(v.data(), (int64_t)v.size()); }

// ---------------------------------------------------------------- a small K with its plan, built by plain loops
// n variables (one fixed), m rows; row r of J reaches the variables r, r + 1, r + 4 and the last variable, which is the border;
// H is lower triangular with the subdiagonal and the diagonal entries sub(r) and diag(r) keep.  The permuted positions are
// variable i, row i, variable i + 1 ...; the last variable behind everything.
struct Planned {
  int32_t n = 0, m = 0;
  Csr A, T, Lo, S;
  std::vector<int32_t> order, map;
  int64_t nb = 0;
  int w = 0, p = 1;
};

template <class Sub, class Diag>
inline Planned planned_kkt(int32_t n, int32_t m, int32_t fixed, Sub sub, Diag diag) {
  Planned q;
  q.n = n; q.m = m;
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
    if (r >= 1 && sub(r)) q.Lo.indices.push_back(r - 1);
    if (diag(r)) q.Lo.indices.push_back(r);
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

#endif  // FAKE_HIP_BAND_DRIVER_COMMON_H
