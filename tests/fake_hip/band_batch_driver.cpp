// band_batch_driver.cpp -- TEST INFRASTRUCTURE: drives the BATCH forms of pockit_amd/csrc/pk_band.cpp (B step systems behind one
// plan, factored and solved in one launch sequence) against the host-only HIP stand-in of this directory, built with
// -fsanitize=address,undefined (tests/test_band_batch_cpu.py).  The contract is that entry e of a batch has, bit for bit, what the
// single form gives for entry e's inputs alone.  The single raw form runs the same kernels as a batch of one, so every entry of
// a shape is held twice: to the SINGLE raw form (entry e of B equals entry 0 of 1) and to the PLAIN LOOPS of band_driver_common.h
// (band inside the matrix and fill rows, interchanges, solution, record): the raw batch form at B = 1, 2, 3, 16 on full-mantissa data, every array packed at a stride larger
// than its length with NaN in the gaps (still NaN afterwards); a batch with a zero column and a planted NaN among good entries;
// a batch against itself permuted; shared sources (stride 0) against the same array repeated; the planned forms at B = 2, 5, 2
// with a single factorisation in between that keeps its bits; the host form against the device forms; every refusal with its
// code and nothing enqueued or written; tear-down without a live allocation.  With --dump FILE: the batch FILE describes
// (tests/test_band_batch_cpu.py writes it from tests/band_batch_cases.py) through the raw batch form, per entry band,
// interchanges, solution and record printed as hex doubles.
#include "band_driver_common.h"

enum { GAP = 3 };

// (the seed's term for a variant is this driver's own number of it: zero column 2, planted NaN 3)
static Sys make(int64_t nb, int w, int p, Variant variant, int salt) {
  const uint64_t code = variant == ZERO ? 2 : variant == PLANT ? 3 : (uint64_t)variant;
  return make_system(nb, w, p, variant, code, (uint64_t)salt, 1, 0);
}

static bool all_nan(const double* a, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!std::isnan(a[i])) return false;
  return true;
}

// one system through the single raw form
static Got single(const Sys& s) {
  Got g;
  OK(raw_single(s, 0, g));
  return g;
}

// ---------------------------------------------------------------- a batch: every array at stride = length + GAP, NaN in the gaps
struct Batch {
  int B = 0;
  int64_t nb = 0;
  int w = 0, p = 0;
  int64_t l_band = 0, l_U = 0, l_C = 0, l_v = 0;      // the lengths: band, U, C, and rhs / x (nb + p)
  Vec band, U, C, rhs, x, rec;                          // x and rec: -77.0 in the entries
  std::vector<int32_t> ipiv;                            // -7 in the entries, -9 in the gaps
  int64_t stride(int64_t len) const { return len + GAP; }
};

static Batch pack(const std::vector<Sys>& entries) {
  Batch b;
  const Sys& s0 = entries[0];
  b.B = (int)entries.size(); b.nb = s0.nb; b.w = s0.w; b.p = s0.p;
  b.l_band = s0.ldab * s0.nb; b.l_U = s0.nb * s0.p; b.l_C = (int64_t)s0.p * s0.p; b.l_v = s0.nb + s0.p;
  const auto filled = [&](int64_t len) {
    Vec v = made((size_t)(b.stride(len) * b.B));
    std::fill(v.begin(), v.end(), NAN);
    return v;
  };
  b.band = filled(b.l_band); b.U = filled(b.l_U); b.C = filled(b.l_C); b.rhs = filled(b.l_v); b.x = filled(b.l_v); b.rec = filled(REC);
  b.ipiv.assign((size_t)(b.stride(b.nb) * b.B) + 1, -9);
  for (int e = 0; e < b.B; ++e) {
    const Sys& s = entries[(size_t)e];
    CHECK(s.nb == b.nb && s.w == b.w && s.p == b.p);
    std::copy(s.band.begin(), s.band.end(), b.band.begin() + (long)(b.stride(b.l_band) * e));
    std::copy(s.U.begin(), s.U.end(), b.U.begin() + (long)(b.stride(b.l_U) * e));
    std::copy(s.C.begin(), s.C.end(), b.C.begin() + (long)(b.stride(b.l_C) * e));
    std::copy(s.rhs.begin(), s.rhs.end(), b.rhs.begin() + (long)(b.stride(b.l_v) * e));
    std::fill_n(b.x.begin() + (long)(b.stride(b.l_v) * e), b.l_v, -77.0);
    std::fill_n(b.rec.begin() + (long)(b.stride(REC) * e), (long)REC, -77.0);
    std::fill_n(b.ipiv.begin() + (long)(b.stride(b.nb) * e), b.nb, -7);
  }
  return b;
}

static int run(Batch& b) {
  const int rc = pk_band_raw_batch_dev(ctx, b.B, b.nb, b.w, b.p, b.p + 1, b.band.data(), b.stride(b.l_band), b.U.data(), b.stride(b.l_U), b.C.data(),
                                       b.stride(b.l_C), b.rhs.data(), b.stride(b.l_v), b.ipiv.data(), b.stride(b.nb), b.x.data(), b.stride(b.l_v),
                                       b.rec.data(), b.stride(REC));
  if (rc) return rc;
  OK(pk_sync(ctx, nullptr));
  return 0;
}

// entry e of the batch has the single form's bits in band, interchanges, solution and record
static bool entry_matches(const Batch& b, int e, const Got& g) {
  if (!same_or_nan(b.band.data() + b.stride(b.l_band) * e, g.band.data(), (size_t)b.l_band)) return false;
  for (int64_t j = 0; j < b.nb; ++j)
    if ((double)b.ipiv[(size_t)(b.stride(b.nb) * e + j)] != g.ipiv[(size_t)j]) return false;
  if (b.l_v && std::memcmp(b.x.data() + b.stride(b.l_v) * e, g.x.data(), 8 * (size_t)b.l_v) != 0) return false;
  return std::memcmp(b.rec.data() + b.stride(REC) * e, g.rec.data(), 8 * REC) == 0;
}

// the gaps between the entries are what the caller left there, in every array
static bool gaps_intact(const Batch& b) {
  for (int e = 0; e < b.B; ++e) {
    const struct { const Vec* v; int64_t len; } arrays[] = {{&b.band, b.l_band}, {&b.U, b.l_U}, {&b.C, b.l_C}, {&b.rhs, b.l_v}, {&b.x, b.l_v}, {&b.rec, REC}};
    for (const auto& a : arrays)
      if (!all_nan(a.v->data() + b.stride(a.len) * e + a.len, GAP)) return false;
    for (int k = 0; k < GAP; ++k)
      if (b.ipiv[(size_t)(b.stride(b.nb) * e + b.nb + k)] != -9) return false;
  }
  return true;
}

// entry e of the batch has the bits of the plain loops: the record; behind a solve the band inside the matrix and in the fill
// rows, the interchanges and the solution; behind a failure the solution untouched
static bool entry_is_reference(const Batch& b, int e, const Sys& s, const Ref& want) {
  if (std::memcmp(b.rec.data() + b.stride(REC) * e, want.rec.data(), 8 * REC) != 0) return false;
  const double* x = b.x.data() + b.stride(b.l_v) * e;
  if (want.rec[STATUS] != 0.0) {
    for (int64_t i = 0; i < b.l_v; ++i)
      if (x[i] != -77.0) return false;
    return true;
  }
  if (!band_matches(s, b.band.data() + b.stride(b.l_band) * e, want.band)) return false;
  for (int64_t j = 0; j < b.nb; ++j)
    if (b.ipiv[(size_t)(b.stride(b.nb) * e + j)] != want.ipiv[(size_t)j]) return false;
  return b.l_v == 0 || std::memcmp(x, want.x[0].data(), 8 * (size_t)b.l_v) == 0;
}

static double status_of(const Batch& b, int e) { return b.rec[(size_t)(b.stride(REC) * e + STATUS)]; }
static bool x_untouched(const Batch& b, int e) {
  for (int64_t i = 0; i < b.l_v; ++i)
    if (b.x[(size_t)(b.stride(b.l_v) * e + i)] != -77.0) return false;
  return true;
}

static int g_B, g_nb, g_w, g_p;
static void check_shape(int B, int64_t nb, int w, int p) {
  g_B = B; g_nb = (int)nb; g_w = w; g_p = p;
  std::vector<Sys> entries;
  for (int e = 0; e < B; ++e) entries.push_back(make(nb, w, p, e % 2 ? TINY : PLAIN, e));
  Batch b = pack(entries);
  OK(run(b));
  for (int e = 0; e < B; ++e) {
    const Got g = single(entries[(size_t)e]);      // entry e of B equals entry 0 of 1 ...
    if (!entry_matches(b, e, g)) std::fprintf(stderr, "B %d nb %d w %d p %d: entry %d\n", g_B, g_nb, g_w, g_p, e);
    CHECK(entry_matches(b, e, g));
    const Ref want = reference(entries[(size_t)e]);      // ... and both are the plain loops
    if (!entry_is_reference(b, e, entries[(size_t)e], want)) std::fprintf(stderr, "B %d nb %d w %d p %d: entry %d against the plain loops\n", g_B, g_nb, g_w, g_p, e);
    CHECK(entry_is_reference(b, e, entries[(size_t)e], want));
    if (e % 2 == 0) CHECK(status_of(b, e) == 0.0);      // (a tiny diagonal may leave a border that is singular in fp64: the bits still agree)
  }
  CHECK(gaps_intact(b));
}

// FILE: "B nb w p", then per entry band (ldab x nb, column-major), U, C, rhs
static int dump(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return 3;
  int B, w, p;
  long long nb;
  if (std::fscanf(f, "%d %lld %d %d", &B, &nb, &w, &p) != 4) return 3;
  std::vector<Sys> entries((size_t)B);
  for (Sys& s : entries) {
    s = shaped(nb, w, p);
    s.band = read_doubles(f); s.U = read_doubles(f); s.C = read_doubles(f); s.rhs = read_doubles(f);
  }
  std::fclose(f);
  load_model();
  set_problem(400, 6, 11, 7);
  Batch b = pack(entries);
  OK(run(b));
  CHECK(gaps_intact(b));
  for (int e = 0; e < B; ++e) {
    print(b.band.data() + b.stride(b.l_band) * e, b.l_band);
    for (int64_t j = 0; j < nb; ++j) std::printf("%a\n", (double)b.ipiv[(size_t)(b.stride(b.nb) * e + j)]);
    print(b.x.data() + b.stride(b.l_v) * e, b.l_v);
    print(b.rec.data() + b.stride(REC) * e, REC);
  }
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return 0;
}

// ---------------------------------------------------------------- a planned system: n = 30 variables (one fixed), m = 20 rows
// The unit assembles what the map says; the map here is a band of half-width 5 around a dominant diagonal and one border
// column, each slot from one or two sources of [hvals | jvals | s1 | s2] -- no K of a model, which the unit does not need.
struct PlannedMap {
  int32_t n = 30, m = 20;
  Csr A, T, Lo, S;
  std::vector<int32_t> order, map;
  int64_t nb = 0, nh = 0, nj = 0;
  int w = 5, p = 1;
};

static PlannedMap planned() {
  PlannedMap q;
  q.A = from_lengths(std::vector<int32_t>((size_t)q.m, 3), q.n);
  q.T = transposed(q.A);
  q.Lo.rows = q.Lo.cols = q.n;
  q.Lo.indptr.push_back(0);
  for (int32_t r = 0; r < q.n; ++r) {
    if (r >= 1) q.Lo.indices.push_back(r - 1);
    q.Lo.indices.push_back(r);
    q.Lo.indptr.push_back((int32_t)q.Lo.indices.size());
  }
  q.S = symmetric(q.Lo);
  q.nh = q.Lo.nnz(); q.nj = q.A.nnz();
  for (int32_t i = 0; i < q.n + q.m; ++i)
    if (i != 3 && i != q.n - 1) q.order.push_back(i);      // variable 3 is fixed, the last variable is the border
  q.nb = (int64_t)q.order.size();
  q.order.push_back(q.n - 1);
  const int64_t ldab = 3 * (int64_t)q.w + 1, dests = ldab * q.nb + q.nb * q.p + q.p * q.p;
  q.map.assign((size_t)(2 * dests), 0);
  const int32_t values = (int32_t)(q.nh + q.nj);
  for (int64_t j = 0; j < q.nb; ++j)
    for (int64_t i = std::max<int64_t>(0, j - q.w); i <= std::min<int64_t>(q.nb - 1, j + q.w); ++i) {
      const size_t d = (size_t)((2 * q.w + i - j) + j * ldab);
      const int32_t e = (int32_t)((i * 7 + j * 3) % values) + 1;
      q.map[2 * d] = (i + j) % 3 ? e : -e;
      if (i == j) q.map[2 * d + 1] = values + q.order[(size_t)i] + 1;      // ... plus its entry of [s1 | s2]
    }
  for (int64_t i = 0; i < q.nb; ++i) q.map[(size_t)(2 * (ldab * q.nb + i))] = (int32_t)(q.nh + i % q.nj) + 1;
  q.map[(size_t)(2 * (dests - 1))] = 1;
  q.map[(size_t)(2 * (dests - 1)) + 1] = values + q.n;      // C: hvals[0] + s1[n - 1]
  return q;
}

// B arrays of a length at stride length + GAP, NaN in the gaps; entry e filled by value(e, i)
template <class Value>
static Vec strided(int B, int64_t len, Value value) {
  Vec v = made((size_t)((len + GAP) * B));
  std::fill(v.begin(), v.end(), NAN);
  for (int e = 0; e < B; ++e)
    for (int64_t i = 0; i < len; ++i) v[(size_t)((len + GAP) * e + i)] = value(e, i);
  return v;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "--dump")) return dump(argv[2]);
  load_model();
  set_problem(400, 6, 11, 7);

  // ---- the raw batch form against the single raw form, entry by entry
  const struct { int64_t nb; int w, p; } shapes[] = {{0, 0, 0}, {0, 7, 1}, {33, 33, 1}, {65, 7, 8}, {65, 0, 8},      // (the issue's table within band_cases.shapes())
                                                     {1, 1, 1}, {193, 192, 0}, {257, 192, 1}};                       // (and Nb = 1, the cap of w)
  for (const auto& s : shapes)
    for (int B : {1, 2, 3, (int)BATCH_CAP}) check_shape(B, s.nb, s.w, s.p);
  check_shape(3, 4500, 8, 1);      // three pieces per dot, 141 panels

  {  // good and failing entries in one batch: statuses 0, 1, 0, 3; the failed entries' solutions untouched, the others complete
    std::vector<Sys> entries;
    for (Variant variant : {PLAIN, ZERO, TINY, PLANT}) entries.push_back(make(65, 7, 1, variant, 9));
    Batch b = pack(entries);
    OK(run(b));
    const double statuses[] = {0.0, 1.0, 0.0, 3.0};
    for (int e = 0; e < 4; ++e) {
      CHECK(status_of(b, e) == statuses[e]);
      CHECK(entry_matches(b, e, single(entries[(size_t)e])));
      CHECK(x_untouched(b, e) == (statuses[e] != 0.0));
    }
    CHECK(b.rec[(size_t)(b.stride(REC) * 1 + COLUMN)] == (double)(2 * 65 / 3) && b.rec[(size_t)(b.stride(REC) * 3 + COLUMN)] == (double)(65 / 2));
    CHECK(gaps_intact(b));
    // ... and the same batch with its entries permuted: the results are permuted, bit for bit
    const int perm[] = {2, 0, 3, 1};
    std::vector<Sys> moved;
    for (int e : perm) moved.push_back(entries[(size_t)e]);
    Batch c = pack(moved);
    OK(run(c));
    for (int e = 0; e < 4; ++e) {
      const int from = perm[e];
      CHECK(same_or_nan(c.band.data() + c.stride(c.l_band) * e, b.band.data() + b.stride(b.l_band) * from, (size_t)b.l_band));
      CHECK(std::memcmp(c.ipiv.data() + c.stride(c.nb) * e, b.ipiv.data() + b.stride(b.nb) * from, 4 * (size_t)b.nb) == 0);
      CHECK(std::memcmp(c.x.data() + c.stride(c.l_v) * e, b.x.data() + b.stride(b.l_v) * from, 8 * (size_t)b.l_v) == 0);
      CHECK(std::memcmp(c.rec.data() + c.stride(REC) * e, b.rec.data() + b.stride(REC) * from, 8 * REC) == 0);
    }
  }
  {  // shared sources: U, C and the right-hand side at stride 0 against the same arrays repeated
    std::vector<Sys> entries;
    for (int e = 0; e < 3; ++e) {
      entries.push_back(make(65, 7, 8, PLAIN, 20 + e));
      entries.back().U = entries[0].U; entries.back().C = entries[0].C; entries.back().rhs = entries[0].rhs;
    }
    Batch repeated = pack(entries), shared = pack(entries);
    OK(run(repeated));
    const Sys& s0 = entries[0];
    OK(pk_band_raw_batch_dev(ctx, 3, s0.nb, s0.w, s0.p, s0.p + 1, shared.band.data(), shared.stride(shared.l_band), s0.U.data(), 0, s0.C.data(), 0,
                             s0.rhs.data(), 0, shared.ipiv.data(), shared.stride(shared.nb), shared.x.data(), shared.stride(shared.l_v),
                             shared.rec.data(), shared.stride(REC)));
    OK(pk_sync(ctx, nullptr));
    CHECK(same_or_nan(shared.band.data(), repeated.band.data(), shared.band.size()) && shared.ipiv == repeated.ipiv);
    CHECK(same_or_nan(shared.x.data(), repeated.x.data(), shared.x.size()) && same_or_nan(shared.rec.data(), repeated.rec.data(), shared.rec.size()));
    for (int e = 0; e < 3; ++e) CHECK(status_of(shared, e) == 0.0 && !x_untouched(shared, e));
  }
  {  // refusals of the raw batch form: the code, nothing enqueued, nothing written
    std::vector<Sys> entries;
    for (int e = 0; e < 2; ++e) entries.push_back(make(40, 7, 1, PLAIN, e));
    Batch b = pack(entries);
    const Batch before = b;
    const size_t mark = fake_hip_log().size();
    const int64_t sb = b.stride(b.l_band), su = b.stride(b.l_U), sc = b.stride(b.l_C), sv = b.stride(b.l_v), sp = b.stride(b.nb), sr = b.stride(REC);
    double *band = b.band.data(), *U = b.U.data(), *C = b.C.data(), *rhs = b.rhs.data(), *x = b.x.data(), *rec = b.rec.data();
    int32_t* pv = b.ipiv.data();
    CHECK(pk_band_raw_batch_dev(ctx, 0, 40, 7, 1, 2, band, sb, U, su, C, sc, rhs, sv, pv, sp, x, sv, rec, sr) == 134);
    CHECK(pk_band_raw_batch_dev(ctx, BATCH_CAP + 1, 40, 7, 1, 2, band, sb, U, su, C, sc, rhs, sv, pv, sp, x, sv, rec, sr) == 134);
    CHECK(pk_band_raw_batch_dev(ctx, 2, -1, 7, 1, 2, band, sb, U, su, C, sc, rhs, sv, pv, sp, x, sv, rec, sr) == 134);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, W_CAP + 1, 1, 2, band, sb, U, su, C, sc, rhs, sv, pv, sp, x, sv, rec, sr) == 134);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, P_CAP + 1, P_CAP + 2, band, sb, U, su, C, sc, rhs, sv, pv, sp, x, sv, rec, sr) == 134);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 1, band, sb, U, su, C, sc, rhs, sv, pv, sp, x, sv, rec, sr) == 134);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, b.l_band - 1, U, su, C, sc, rhs, sv, pv, sp, x, sv, rec, sr) == 134);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, 0, U, su, C, sc, rhs, sv, pv, sp, x, sv, rec, sr) == 134);      // (the bands are written)
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, sb, U, b.l_U - 1, C, sc, rhs, sv, pv, sp, x, sv, rec, sr) == 134);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, sb, U, su, C, -1, rhs, sv, pv, sp, x, sv, rec, sr) == 134);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, sb, U, su, C, sc, rhs, b.l_v - 1, pv, sp, x, sv, rec, sr) == 134);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, sb, U, su, C, sc, rhs, sv, pv, b.nb - 1, x, sv, rec, sr) == 134);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, sb, U, su, C, sc, rhs, sv, pv, sp, x, 0, rec, sr) == 134);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, sb, U, su, C, sc, rhs, sv, pv, sp, x, sv, rec, REC - 1) == 134);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, nullptr, sb, U, su, C, sc, rhs, sv, pv, sp, x, sv, rec, sr) == 110);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, sb, nullptr, su, C, sc, rhs, sv, pv, sp, x, sv, rec, sr) == 110);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, sb, U, su, nullptr, sc, rhs, sv, pv, sp, x, sv, rec, sr) == 110);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, sb, U, su, C, sc, nullptr, sv, pv, sp, x, sv, rec, sr) == 110);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, sb, U, su, C, sc, rhs, sv, nullptr, sp, x, sv, rec, sr) == 110);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, sb, U, su, C, sc, rhs, sv, pv, sp, nullptr, sv, rec, sr) == 110);
    CHECK(pk_band_raw_batch_dev(ctx, 2, 40, 7, 1, 2, band, sb, U, su, C, sc, rhs, sv, pv, sp, x, sv, nullptr, sr) == 110);
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark);
    CHECK(same_or_nan(b.band.data(), before.band.data(), b.band.size()) && same_or_nan(b.x.data(), before.x.data(), b.x.size()));
    CHECK(same_or_nan(b.rec.data(), before.rec.data(), b.rec.size()) && b.ipiv == before.ipiv);
  }

  // ---- the planned forms
  const PlannedMap q = planned();
  const int32_t n = q.n, m = q.m;
  const int64_t N = n + m, nh = q.nh, nj = q.nj;
  set_problem(n, m, nj, nh);
  g_state = 4242;
  const int BMAX = 5;
  // per-entry values, every array at stride length + GAP: the diagonal (s1, s2) dominates each row of the band
  const Vec hv = strided(BMAX, nh, [](int, int64_t) { return unit(); }), jv = strided(BMAX, nj, [](int, int64_t) { return unit(); });
  const Vec s1 = strided(BMAX, n, [](int e, int64_t) { return 30.0 + e + unit(); }), s2 = strided(BMAX, m, [](int e, int64_t) { return 20.0 + e + unit(); });
  Vec rhs = strided(BMAX, N, [](int, int64_t) { return unit(); });
  for (int e = 0; e < BMAX; ++e) rhs[(size_t)((N + GAP) * e + 3)] = NAN;      // (the fixed variable's entry is not read)
  const int64_t sh = nh + GAP, sj = nj + GAP, ss1 = n + GAP, ss2 = m + GAP, sN = N + GAP;
  const auto fresh_sol = [&](int B) { return strided(B, N, [](int, int64_t) { return -77.0; }); };
  {  // before the plan
    Vec sol = fresh_sol(2), rec(2 * REC, -3.0);
    const size_t mark = fake_hip_log().size();
    CHECK(pk_band_factor_batch_dev(ctx, 2, hv.data(), sh, jv.data(), sj, s1.data(), ss1, s2.data(), ss2) == 134);
    CHECK(pk_band_solve_batch_dev(ctx, 2, rhs.data(), sN, sol.data(), sN) == 134);
    CHECK(pk_band_record_batch(ctx, 2, rec.data()) == 134);
    CHECK(fake_hip_log().size() == mark);
  }
  set_identity_map(0, nj);
  set_identity_map(1, nh);
  OK(pk_band_plan(ctx, q.nb, q.w, q.p, q.order.data(), q.map.data()));
  // the single forms on entry e's arrays: (sol, rec)
  const auto single_planned = [&](int e) {
    Vec sol((size_t)N, -77.0), rec(REC);
    OK(pk_band_factor_dev(ctx, hv.data() + sh * e, jv.data() + sj * e, s1.data() + ss1 * e, s2.data() + ss2 * e));
    OK(pk_band_solve_dev(ctx, rhs.data() + sN * e, sol.data()));
    OK(pk_band_record(ctx, rec.data()));
    return std::make_pair(sol, rec);
  };
  std::vector<std::pair<Vec, Vec>> want;
  for (int e = 0; e < BMAX; ++e) {
    want.push_back(single_planned(e));
    CHECK(want.back().second[STATUS] == 0.0 && want.back().first[3] == 0.0);
    if (e) CHECK(!same_bits(want[(size_t)e].first, want[0].first));
  }
  const auto batch_planned = [&](int B) {
    Vec sol = fresh_sol(B), rec((size_t)(B * REC), -3.0);
    OK(pk_band_factor_batch_dev(ctx, B, hv.data(), sh, jv.data(), sj, s1.data(), ss1, s2.data(), ss2));
    OK(pk_band_solve_batch_dev(ctx, B, rhs.data(), sN, sol.data(), sN));
    OK(pk_band_record_batch(ctx, B, rec.data()));
    for (int e = 0; e < B; ++e) {
      CHECK(std::memcmp(sol.data() + sN * e, want[(size_t)e].first.data(), 8 * (size_t)N) == 0);
      CHECK(std::memcmp(rec.data() + REC * e, want[(size_t)e].second.data(), 8 * REC) == 0);
      CHECK(all_nan(sol.data() + sN * e + N, GAP));
    }
  };
  {  // B = 2, 5, 2 on one context; a single factorisation made in between keeps its bits, and solves again after the batches
    OK(pk_band_factor_dev(ctx, hv.data() + sh * 4, jv.data() + sj * 4, s1.data() + ss1 * 4, s2.data() + ss2 * 4));
    batch_planned(2);
    Vec sol((size_t)N, -77.0), rec(REC);
    OK(pk_band_solve_dev(ctx, rhs.data() + sN * 4, sol.data()));      // (the single factors of entry 4 survived the batch)
    OK(pk_band_record(ctx, rec.data()));
    CHECK(same_bits(sol, want[4].first) && same_bits(rec, want[4].second));
    batch_planned(5);
    const auto again = single_planned(1);
    CHECK(same_bits(again.first, want[1].first) && same_bits(again.second, want[1].second));
    {  // ... and the batch of 5 survived the single call: a second solve with it
      Vec bsol = fresh_sol(5);
      OK(pk_band_solve_batch_dev(ctx, 5, rhs.data(), sN, bsol.data(), sN));
      OK(pk_sync(ctx, nullptr));
      for (int e = 0; e < 5; ++e) CHECK(std::memcmp(bsol.data() + sN * e, want[(size_t)e].first.data(), 8 * (size_t)N) == 0);
    }
    batch_planned(2);
    batch_planned(1);
  }
  {  // shared sources: H, J, s2 and the right-hand side at stride 0 equal the same arrays repeated
    const int B = 3;
    const Vec hrep = strided(B, nh, [&](int, int64_t i) { return hv[(size_t)i]; }), jrep = strided(B, nj, [&](int, int64_t i) { return jv[(size_t)i]; });
    const Vec s2rep = strided(B, m, [&](int, int64_t i) { return s2[(size_t)i]; }), rrep = strided(B, N, [&](int, int64_t i) { return rhs[(size_t)i]; });
    Vec a = fresh_sol(B), b = fresh_sol(B), ra((size_t)(B * REC)), rb((size_t)(B * REC));
    OK(pk_band_factor_batch_dev(ctx, B, hrep.data(), sh, jrep.data(), sj, s1.data(), ss1, s2rep.data(), ss2));
    OK(pk_band_solve_batch_dev(ctx, B, rrep.data(), sN, a.data(), sN));
    OK(pk_band_record_batch(ctx, B, ra.data()));
    OK(pk_band_factor_batch_dev(ctx, B, hv.data(), 0, jv.data(), 0, s1.data(), ss1, s2.data(), 0));
    OK(pk_band_solve_batch_dev(ctx, B, rhs.data(), 0, b.data(), sN));
    OK(pk_band_record_batch(ctx, B, rb.data()));
    CHECK(same_or_nan(a.data(), b.data(), a.size()) && same_bits(ra, rb) && ra[STATUS] == 0.0);
    CHECK(std::memcmp(a.data() + sN, a.data(), 8 * (size_t)N) != 0);      // (s1 differs: so do the solutions)
  }
  {  // a failing entry among good ones on the plan: entry 1 with every source zero -- status 1, its sol untouched, the others whole
    Vec h0 = hv, j0 = jv, z1 = s1, z2 = s2;
    for (Vec* v : {&h0, &j0, &z1, &z2}) {
      const int64_t stride = v == &h0 ? sh : v == &j0 ? sj : v == &z1 ? ss1 : ss2;
      std::fill_n(v->begin() + (long)stride, (long)(stride - GAP), 0.0);
    }
    Vec sol = fresh_sol(3), rec(3 * REC);
    OK(pk_band_factor_batch_dev(ctx, 3, h0.data(), sh, j0.data(), sj, z1.data(), ss1, z2.data(), ss2));
    OK(pk_band_solve_batch_dev(ctx, 3, rhs.data(), sN, sol.data(), sN));
    OK(pk_band_record_batch(ctx, 3, rec.data()));
    CHECK(rec[STATUS] == 0.0 && rec[REC + STATUS] == 1.0 && rec[REC + COLUMN] == 0.0 && rec[2 * REC + STATUS] == 0.0);
    for (int e : {0, 2}) CHECK(std::memcmp(sol.data() + sN * e, want[(size_t)e].first.data(), 8 * (size_t)N) == 0);
    for (int64_t i = 0; i < N; ++i) CHECK(sol[(size_t)(sN + i)] == -77.0);
  }
  {  // refusals of the planned forms: the code, nothing enqueued, nothing written; the last batch (3 entries) stays usable
    Vec sol = fresh_sol(3), rec(3 * REC, -3.0);
    const Vec sol0 = sol;
    const size_t mark = fake_hip_log().size();
    const double *h = hv.data(), *j = jv.data(), *a1 = s1.data(), *a2 = s2.data();
    CHECK(pk_band_factor_batch_dev(ctx, 0, h, sh, j, sj, a1, ss1, a2, ss2) == 134);
    CHECK(pk_band_factor_batch_dev(ctx, BATCH_CAP + 1, h, sh, j, sj, a1, ss1, a2, ss2) == 134);
    CHECK(pk_band_factor_batch_dev(ctx, 3, h, nh - 1, j, sj, a1, ss1, a2, ss2) == 134);
    CHECK(pk_band_factor_batch_dev(ctx, 3, h, sh, j, -sj, a1, ss1, a2, ss2) == 134);
    CHECK(pk_band_factor_batch_dev(ctx, 3, h, sh, j, sj, a1, n - 1, a2, ss2) == 134);
    CHECK(pk_band_factor_batch_dev(ctx, 3, h, sh, j, sj, a1, ss1, a2, 1) == 134);
    CHECK(pk_band_factor_batch_dev(ctx, 3, nullptr, sh, j, sj, a1, ss1, a2, ss2) == 110);
    CHECK(pk_band_factor_batch_dev(ctx, 3, h, sh, nullptr, sj, a1, ss1, a2, ss2) == 110);
    CHECK(pk_band_factor_batch_dev(ctx, 3, h, sh, j, sj, nullptr, ss1, a2, ss2) == 110);
    CHECK(pk_band_factor_batch_dev(ctx, 3, h, sh, j, sj, a1, ss1, nullptr, ss2) == 110);
    CHECK(pk_band_solve_batch_dev(ctx, 2, rhs.data(), sN, sol.data(), sN) == 134);      // (the last batch had 3 entries)
    CHECK(pk_band_solve_batch_dev(ctx, 0, rhs.data(), sN, sol.data(), sN) == 134);
    CHECK(pk_band_solve_batch_dev(ctx, 3, rhs.data(), N - 1, sol.data(), sN) == 134);
    CHECK(pk_band_solve_batch_dev(ctx, 3, rhs.data(), sN, sol.data(), 0) == 134);      // (the solutions are written)
    CHECK(pk_band_solve_batch_dev(ctx, 3, rhs.data(), sN, sol.data(), N - 1) == 134);
    CHECK(pk_band_solve_batch_dev(ctx, 3, nullptr, sN, sol.data(), sN) == 110);
    CHECK(pk_band_solve_batch_dev(ctx, 3, rhs.data(), sN, nullptr, sN) == 110);
    CHECK(pk_band_record_batch(ctx, 2, rec.data()) == 134);
    CHECK(pk_band_record_batch(ctx, BATCH_CAP + 1, rec.data()) == 134);
    CHECK(pk_band_record_batch(ctx, 3, nullptr) == 60);
    OK(pk_set_shard(ctx, 1, 0, nullptr));
    CHECK(pk_band_factor_batch_dev(ctx, 3, h, sh, j, sj, a1, ss1, a2, ss2) == 119);
    CHECK(pk_band_solve_batch_dev(ctx, 3, rhs.data(), sN, sol.data(), sN) == 119);
    OK(pk_set_shard(ctx, 0, 0, nullptr));
    OK(pk_sync(ctx, nullptr));
    CHECK(fake_hip_log().size() == mark);
    CHECK(same_or_nan(sol.data(), sol0.data(), sol.size()));
    for (double v : rec) CHECK(v == -3.0);
    OK(pk_band_solve_batch_dev(ctx, 3, rhs.data(), sN, sol.data(), sN));      // (no refusal invalidated the batch of 3)
    OK(pk_sync(ctx, nullptr));
    for (int e : {0, 2}) CHECK(std::memcmp(sol.data() + sN * e, want[(size_t)e].first.data(), 8 * (size_t)N) == 0);
  }
  {  // the host form on the context's linearization against the device batch forms on the same values
    OK(set_operator(0, q.A));
    OK(set_operator(1, q.T));
    OK(set_operator(2, q.S));
    Vec x((size_t)n), lam((size_t)m);
    for (int i = 0; i < n; ++i) x[(size_t)i] = 2.0 * (double)(i % 9 - 4);
    for (int k = 0; k < m; ++k) lam[(size_t)k] = (double)(k % 5 - 2);
    const int B = 3;
    Vec t1((size_t)(B * n)), t2((size_t)(B * m)), tb((size_t)(B * N));
    for (int e = 0; e < B; ++e) {
      for (int i = 0; i < n; ++i) t1[(size_t)(e * n + i)] = 1.0e9 + 1.0e6 * (i % 5) + 1.0e5 * e;
      for (int k = 0; k < m; ++k) t2[(size_t)(e * m + k)] = 1.0e9 + 1.0e6 * (k % 3) + 1.0e5 * e;
      for (int64_t i = 0; i < N; ++i) tb[(size_t)(e * N + i)] = rhs[(size_t)(sN * e + i)];
    }
    Guarded hx((size_t)(B * N)), hrec((size_t)(B * REC));
    const size_t mark = fake_hip_log().size();
    CHECK(pk_solve_banded_batch(ctx, B, t1.data(), t2.data(), tb.data(), hx.ptr(), hrec.ptr()) == 118);      // no linearization
    OK(pk_linearize(ctx, x.data(), lam.data(), 2.0));
    const size_t mark2 = fake_hip_log().size();
    CHECK(pk_solve_banded_batch(ctx, B, nullptr, t2.data(), tb.data(), hx.ptr(), hrec.ptr()) == 60);
    CHECK(pk_solve_banded_batch(ctx, B, t1.data(), nullptr, tb.data(), hx.ptr(), hrec.ptr()) == 60);
    CHECK(pk_solve_banded_batch(ctx, B, t1.data(), t2.data(), nullptr, hx.ptr(), hrec.ptr()) == 60);
    CHECK(pk_solve_banded_batch(ctx, B, t1.data(), t2.data(), tb.data(), nullptr, hrec.ptr()) == 60);
    CHECK(pk_solve_banded_batch(ctx, B, t1.data(), t2.data(), tb.data(), hx.ptr(), nullptr) == 60);
    CHECK(pk_solve_banded_batch(ctx, 0, t1.data(), t2.data(), tb.data(), hx.ptr(), hrec.ptr()) == 134);
    CHECK(pk_solve_banded_batch(ctx, BATCH_CAP + 1, t1.data(), t2.data(), tb.data(), hx.ptr(), hrec.ptr()) == 134);
    OK(pk_set_shard(ctx, 1, 0, nullptr));
    CHECK(pk_solve_banded_batch(ctx, B, t1.data(), t2.data(), tb.data(), hx.ptr(), hrec.ptr()) == 119);
    OK(pk_set_shard(ctx, 0, 0, nullptr));
    CHECK(fake_hip_log().size() == mark2 && mark2 >= mark);
    for (const Guarded* g : {&hx, &hrec}) for (double v : g->fetch()) CHECK(v == -77.0);
    OK(pk_solve_banded_batch(ctx, B, t1.data(), t2.data(), tb.data(), hx.ptr(), hrec.ptr()));
    Vec lj((size_t)nj), lh((size_t)nh);
    for (int64_t e = 0; e < nj; ++e) lj[(size_t)e] = fake_jac(x.data(), n, e, false);
    for (int64_t e = 0; e < nh; ++e) lh[(size_t)e] = fake_hess(x.data(), lam.data(), 2.0, n, m, e);
    Guarded dx((size_t)(B * N));
    Vec drec((size_t)(B * REC));
    OK(pk_band_factor_batch_dev(ctx, B, lh.data(), 0, lj.data(), 0, t1.data(), n, t2.data(), m));
    OK(pk_band_solve_batch_dev(ctx, B, tb.data(), N, dx.ptr(), N));
    OK(pk_band_record_batch(ctx, B, drec.data()));
    CHECK(same_bits(hrec.fetch(), drec) && same_bits(hx.fetch(), dx.fetch()));
    for (int e = 0; e < B; ++e) {      // ... and each row against the single host form
      Vec sx((size_t)N, -77.0), srec(REC);
      OK(pk_solve_banded(ctx, t1.data() + e * n, t2.data() + e * m, tb.data() + e * N, sx.data(), srec.data()));
      CHECK(srec[STATUS] == 0.0 && std::memcmp(sx.data(), hx.ptr() + e * N, 8 * (size_t)N) == 0 && std::memcmp(srec.data(), hrec.ptr() + e * REC, 8 * REC) == 0);
    }
    // a row whose entry fails is left as the caller gave it: a NaN in entry 1's s1
    t1[(size_t)(n + 7)] = NAN;
    Guarded fx((size_t)(B * N)), frec((size_t)(B * REC));
    OK(pk_solve_banded_batch(ctx, B, t1.data(), t2.data(), tb.data(), fx.ptr(), frec.ptr()));
    const Vec got = fx.fetch(), grec = frec.fetch(), good = hx.fetch();
    CHECK(grec[STATUS] == 0.0 && grec[REC + STATUS] == 3.0 && grec[2 * REC + STATUS] == 0.0);
    for (int64_t i = 0; i < N; ++i) CHECK(got[(size_t)(N + i)] == -77.0);
    for (int e : {0, 2}) CHECK(std::memcmp(got.data() + e * N, good.data() + e * N, 8 * (size_t)N) == 0);
  }
  {  // the CSR maps changed since the plan: refused; then a new plan invalidates the batch (and the single factors)
    std::vector<int32_t> seg((size_t)nj), perm((size_t)nj);
    for (int64_t k = 0; k < nj; ++k) { seg[(size_t)k] = (int32_t)(k < nj - 1 ? k : nj); perm[(size_t)k] = (int32_t)k; }
    OK(pk_set_csr_map(ctx, 0, seg.data(), perm.data(), nj - 1, nj));
    CHECK(pk_band_factor_batch_dev(ctx, 2, hv.data(), sh, jv.data(), sj, s1.data(), ss1, s2.data(), ss2) == 134);
    set_identity_map(0, nj);
    OK(pk_band_factor_batch_dev(ctx, 2, hv.data(), sh, jv.data(), sj, s1.data(), ss1, s2.data(), ss2));
    OK(pk_band_plan(ctx, q.nb, q.w, q.p, q.order.data(), q.map.data()));
    Vec sol = fresh_sol(2), rec(2 * REC, -3.0);
    CHECK(pk_band_solve_batch_dev(ctx, 2, rhs.data(), sN, sol.data(), sN) == 134);
    CHECK(pk_band_record_batch(ctx, 2, rec.data()) == 134);
    CHECK(pk_band_solve_dev(ctx, rhs.data(), sol.data()) == 134);
    for (int64_t i = 0; i < N; ++i) CHECK(sol[(size_t)i] == -77.0);
    batch_planned(2);      // (reserved again on first use)
  }

  // ---- what frees the state: a new problem, and pk_destroy leaves no live allocation
  CHECK(fake_hip_live_allocations() > 0);
  set_problem(400, 6, 11, 7);
  {
    Vec rec(2 * REC);
    CHECK(pk_band_record_batch(ctx, 2, rec.data()) == 134);
  }
  check_shape(3, 65, 7, 8);
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return checks_passed();
}
