// pk_band.cpp -- the step's system K = [[H + diag(s1), J^T], [J, -diag(s2)]] over the free variables and all rows, assembled,
// FACTORED and solved where the CSR values lie: a band LU with partial pivoting inside the band, bordered by the few dense
// unknowns the ordering set aside (pockit_amd/band.py).  No matrix value leaves the device; a record of 8
// doubles comes back.
//
// The permuted matrix is [[B, U], [U^T, C]]: B (Nb x Nb) has half-bandwidth w, U is Nb x p, C is p x p, p <= PK_BD_P_CAP,
// w <= PK_BD_W_CAP.  B lies in LAPACK's dgbtrf storage: kl = ku = w, leading dimension ldab = 3 w + 1, column-major,
// B(i, j) at AB[(2 w + i - j) + j ldab] for j - 2 w <= i <= j + w (the rows 0 ... w - 1 of AB hold the fill of pivoting: they are
// never read before they are written, whatever a caller left there; the slots outside the matrix are neither read nor written).
// U is column-major (U[q Nb + i]), C is column-major (C[a + b p]).
//
//   fill      destination d of [band | U | C] takes acc = 0.0, then acc = acc + v or acc = acc - v for its (at most two)
//             sources in the map's order; v is an entry of [hvals | jvals | s1 | s2].  A slot without a source is 0.0 and no slot
//             is -0.0.                                                                                           [pk_bd_fill_k]
//   factor    the record is initialised [pk_bd_init_k]; then dgbtf2's arithmetic, column by column j = 0 ... Nb - 1 with
//             km = min(w, Nb - 1 - j):
//               the pivot is the largest |B(i, j)|, i = j ... j + km, ties to the lowest i; a column with an entry that is not
//               finite ends the factorisation with status 3, a pivot of 0.0 with status 1, both with the column;
//               rows j and ipiv[j] are exchanged in the columns j ... min(j + 2 w, Nb - 1) (never in earlier columns);
//               l_i = B(i, j) / B(j, j), the correctly rounded quotient, i = j + 1 ... j + km;
//               B(i, c) = B(i, c) - (l_i B(j, c)) for c = j + 1 ... min(j + 2 w, Nb - 1), the product rounded before the
//               subtraction.
//             Panels of PK_BD_NB columns: one workgroup factors a panel in LDS [pk_bd_panel_k], then one workgroup per
//             trailing column c (up to NB - 1 + 2 w of them) applies the panel's interchanges and updates to it, pivot by pivot
//             in ascending order [pk_bd_update_k].  Every entry receives its updates in ascending pivot order whatever NB is,
//             so the bits are those of the unblocked loop above.  A launch that finds status != 0 returns at once; the panel
//             that fails writes nothing but the record.
//   solve     R = p + k sweep vectors (k = 1 for one right-hand side): the p columns of U, then each b gathered through order[]
//             (its b_C aside) [pk_bd_prep_k]; one workgroup each [pk_bd_solve_k].  Forward, j ascending:
//             y_j <-> y_ipiv[j], then y_i = y_i - (l_i y_j), i = j + 1 ... j + km.  Backward, k descending: y_k = y_k / B(k, k),
//             then y_i = y_i - (B(i, k) y_k), i = max(0, k - 2 w) ... k - 1.  Elementwise: no sum is reduced across threads.
//             The active window lives in an LDS ring, the factor's columns come in chunks of PK_BD_CH columns.
//   border    (p > 0) the (p + k) p dots d[r p + a] = U_a . Y_r by the pieced dot of pk_libkernel.h, products rounded before
//             they are added [pk_bd_dot_k]; one workgroup: S(a, b) = C(a, b) - d[b p + a], t_a = b_C,a - d[(p + c) p + a], LU of S
//             with partial pivoting (largest |.|, ties lowest) in plain loops, x_C by forward and back substitution, a pivot of
//             0.0 gives status 2, one that is not finite status 3, column Nb + k [pk_bd_border_k]; then elementwise
//             x_B,i = y_b,i - (Y_0,i x_C,0) - (Y_1,i x_C,1) ... in ascending q [pk_bd_xb_k].
//   scatter   sol[i] = x[where[i]], 0.0 where where[i] < 0 (a fixed variable)                                   [pk_bd_scatter_k]
//
// The record of 8 doubles: 0 status (0 solved, 1 singular band pivot, 2 singular border, 3 non-finite); 1 the failing column in
// permuted numbering or -1; 2 the smallest |pivot| of the band (+inf without one); 3 the largest (0.0 without one); 4 Nb; 5 w;
// 6 p; 7 the interchanges that moved a row.  After status != 0 sol is left untouched.
//
//   forms     ONE family of ten kernels serves a single system, a batch and a block.  The grid is (work items, entries): a
//             kernel takes its entry from blockIdx.y (bd_entry moves the pointers) and walks blockIdx.x; the single form is one
//             entry with one column.  A batch is B <= PK_BD_BATCH_CAP systems behind one plan, each entry in its own slices.  A
//             block is k <= PK_BD_RHS_CAP right-hand sides against one factorisation in the launches of one solve: the p columns
//             of U are swept once per call, S is formed and factored ONCE by thread 0 of the border workgroup and thread c
//             substitutes for column c (the interchanges and multipliers are replayed on its own t in the order the LU applied
//             them to S), x_B and the scatter run over k Nb and k (n + m) elements.  Column c has the bits the solve gives for
//             it alone, and entry e the bits of a batch of one.
//
// Pivoting is confined to the band part: a K whose band part B is singular while K is not fails here (status 1).
// No atomics, no fused multiply-add, no workgroup waits for another: every dependency is a kernel boundary on the stream.
#include <cmath>

#include "pk_runtime.h"

// Nothing in this unit may contract a * b + c into a fused multiply-add: every product is rounded before it is added.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#include "pk_libkernel.h"      // (behind the pragma: what its templates are instantiated with is this unit's arithmetic)

// The caps follow from the kernels' static LDS: the panel's tile is (W_CAP + NB + 1) x NB doubles (57 600 bytes) beside the two
// planes of the pivot search; the solve's chunk of factor columns is CH x (2 W_CAP + 1) doubles (49 280 bytes) beside the ring;
// the border's dots take one plane per border unknown.
enum { PK_BD_NB = 32, PK_BD_W_CAP = 192, PK_BD_P_CAP = 8, PK_BD_CH = 16, PK_BD_RING = 512, PK_BD_REC = 8 };
enum { BD_LD = PK_BD_W_CAP + PK_BD_NB + 1, BD_LW = 2 * PK_BD_W_CAP + 1 };      // (BD_LD odd: a row of the tile walks all banks)
enum { BD_STATUS = 0, BD_COLUMN = 1, BD_MIN = 2, BD_MAX = 3, BD_NB = 4, BD_W = 5, BD_P = 6, BD_SWAPS = 7 };
static_assert(PK_BD_W_CAP + 1 <= PK_BLOCK && PK_BD_W_CAP + PK_BD_NB <= PK_BLOCK, "one thread per row of a column's window");
static_assert(2 * PK_BD_W_CAP + PK_BD_CH <= PK_BD_RING && (PK_BD_RING & (PK_BD_RING - 1)) == 0, "the ring holds the active window");

struct PkBandArgs {
  const double *hvals, *jvals, *s1, *s2;      // fill: the four source arrays and where each begins in [hvals | jvals | s1 | s2]
  int64_t nh, nj, ns1, dests;
  const int32_t *map, *order, *where;         // map: 2 codes per destination (0 none, +(k + 1) plus, -(k + 1) minus)
  double *band, *U, *C;
  int32_t* ipiv;
  double *Y, *x, *bc, *rec, *partial, *sol;
  const double* rhs;
  int64_t nb, ldab, j0, n_pieces, nsol;
  int32_t w, p, planes;
};

// What every kernel takes: B <= PK_BD_BATCH_CAP entries behind ONE plan (shape, map, order, where and j0 are shared), each with
// k <= PK_BD_RHS_CAP right-hand sides against its ONE factorisation.  The single form is B = 1, k = 1.
//   entries   `a` holds entry 0; entry e's arrays begin e strides s_* behind it, in elements of each array.  A stride of 0
//             (sources only) makes every entry read the same array.  Y, x and b_C are slices of one work array per entry and
//             move together.  No entry reads or writes another's slices.
//   columns   a.Y has p + k sweep vectors (U's columns, then the k right-hand sides), a.x k slices of nb + p, a.bc k slices of
//             p, a.partial (p + k) p planes.  Column c reads a.rhs + c c_rhs and writes a.sol + c c_sol; the scatter reads
//             slice c at a.x + c c_from.  At k = 1 these are the slices of one right-hand side.
//   columns_j the trailing columns behind the panel at a.j0: the work items of the update launch.
enum { PK_BD_BATCH_CAP = 16, PK_BD_RHS_CAP = 64 };
struct PkBandFamilyArgs {
  PkBandArgs a;
  int64_t s_h, s_j, s_s1, s_s2, s_band, s_U, s_C, s_ipiv, s_work, s_rec, s_partial, s_rhs, s_sol;
  int64_t c_rhs, c_sol, c_from, columns_j;
  int32_t k;
};
static_assert(PK_BD_RHS_CAP <= PK_BLOCK, "one thread of the border workgroup per right-hand side");

#ifdef __HIPCC__
#define BD_BODY __device__ __forceinline__
#define BD_PHASE(call)                    \
  do {                                    \
    {                                     \
      const int t = (int)threadIdx.x;     \
      call;                               \
    }                                     \
    __syncthreads();                      \
  } while (0)
#define BD_TREE(step, s, ...) lib_tree(step, s, (int)threadIdx.x, ##__VA_ARGS__)
// The code behind this point begins on a 64-byte line of the instruction cache, whatever the length of the kernel's prologue
// in front of it (the padding is s_nop, passed once).  The one-workgroup panel is a chain of ~200 barrier phases per panel, and
// where its column loop falls against those lines is worth 2 us of its 74: measured, DESIGN.md section 28.
#ifdef __HIP_DEVICE_COMPILE__
#define BD_ALIGN_CODE() asm volatile(".p2align 6")
#else
#define BD_ALIGN_CODE() do {} while (0)
#endif
#else
#define BD_BODY inline
#define BD_PHASE(call)                                  \
  do {                                                  \
    for (int t = 0; t < PK_BLOCK; ++t) { call; }        \
  } while (0)
#define BD_TREE(step, s, ...) lib_tree_host(step, s, ##__VA_ARGS__)
#define BD_ALIGN_CODE() do {} while (0)
#endif

PK_LIB_FN int64_t bd_min(int64_t a, int64_t b) { return a < b ? a : b; }
PK_LIB_FN int64_t bd_max(int64_t a, int64_t b) { return a > b ? a : b; }
PK_LIB_FN int64_t bd_items(int64_t len) { return (len + PK_BLOCK - 1) / PK_BLOCK; }      // (lib_elem_items, for a kernel)
PK_LIB_FN double* bd_at(const PkBandArgs& a, int64_t i, int64_t j) { return a.band + ((2 * (int64_t)a.w + i - j) + j * a.ldab); }
// is B(i, j) a slot of the storage?  And is it a slot of the fill rows (j - i > w) that no pivot in front of the panel at j0 has
// touched yet -- read as 0.0 whatever the memory holds: the kernels never read the fill rows a caller hands over
PK_LIB_FN bool bd_stored(const PkBandArgs& a, int64_t i, int64_t j) { return i - j <= a.w && j - i <= 2 * (int64_t)a.w; }
PK_LIB_FN bool bd_fresh(const PkBandArgs& a, int64_t i, int64_t j) { return j - i > a.w && (a.j0 == 0 || j >= a.j0 + 2 * (int64_t)a.w); }

// the arguments of entry e: every pointer moved by the entry's stride (an array the form does not use is null and its stride
// 0), everything else as it is.  The only place that moves a pointer by an entry.
PK_LIB_FN PkBandArgs bd_entry(const PkBandFamilyArgs& g, int64_t e) {
  PkBandArgs a = g.a;
  a.hvals += e * g.s_h; a.jvals += e * g.s_j; a.s1 += e * g.s_s1; a.s2 += e * g.s_s2;
  a.band += e * g.s_band; a.U += e * g.s_U; a.C += e * g.s_C;
  a.ipiv += e * g.s_ipiv;
  a.Y += e * g.s_work; a.x += e * g.s_work; a.bc += e * g.s_work;
  a.rec += e * g.s_rec; a.partial += e * g.s_partial;
  a.rhs += e * g.s_rhs; a.sol += e * g.s_sol;
  return a;
}

// ---------------------------------------------------------------- elementwise work
PK_LIB_FN void bd_init_thread(const PkBandArgs& a, int t) {
  if (t != 0) return;
  a.rec[BD_STATUS] = 0.0; a.rec[BD_COLUMN] = -1.0; a.rec[BD_MIN] = __builtin_inf(); a.rec[BD_MAX] = 0.0;
  a.rec[BD_NB] = (double)a.nb; a.rec[BD_W] = (double)a.w; a.rec[BD_P] = (double)a.p; a.rec[BD_SWAPS] = 0.0;
}

PK_LIB_FN double bd_source(const PkBandArgs& a, int64_t k) {
  if (k < a.nh) return a.hvals[k];
  if (k < a.nh + a.nj) return a.jvals[k - a.nh];
  if (k < a.nh + a.nj + a.ns1) return a.s1[k - a.nh - a.nj];
  return a.s2[k - a.nh - a.nj - a.ns1];
}

PK_LIB_FN void bd_fill_element(const PkBandArgs& a, int64_t d) {
  double acc = 0.0;
  for (int k = 0; k < 2; ++k) {
    const int32_t code = a.map[2 * d + k];
    if (code > 0) acc = acc + bd_source(a, (int64_t)code - 1);
    else if (code < 0) acc = acc - bd_source(a, -(int64_t)code - 1);
  }
  a.band[d] = acc;      // (band, U and C are one array)
}

// In the three elements below `a` is the entry's (bd_entry) and g gives the columns: k and the strides c_*.
// [Y_0 ... Y_{p-1} | y_b of column 0 ... k - 1] and the k slices of b_C from U and the right-hand sides
PK_LIB_FN void bd_prep_element(const PkBandArgs& a, const PkBandFamilyArgs& g, int64_t e) {
  const int64_t nu = a.nb * a.p, N = a.nb + a.p;
  if (e < nu) { a.Y[e] = a.U[e]; return; }
  const int64_t c = (e - nu) / N, k = (e - nu) % N;      // the column and the permuted position
  const double v = a.rhs[c * g.c_rhs + (a.order ? (int64_t)a.order[k] : k)];
  if (k < a.nb) a.Y[nu + c * a.nb + k] = v;
  else a.bc[c * a.p + (k - a.nb)] = v;
}

PK_LIB_FN void bd_xb_element(const PkBandArgs& a, int64_t e) {
  const int64_t c = e / a.nb, i = e % a.nb, N = a.nb + a.p;
  double v = a.Y[((int64_t)a.p + c) * a.nb + i];
  for (int q = 0; q < a.p; ++q) {
    const double pr = a.Y[(int64_t)q * a.nb + i] * a.x[c * N + a.nb + q];
    v = v - pr;
  }
  a.x[c * N + i] = v;
}

// (a.x is the scatter's source: x, or the swept right-hand sides without a border)
PK_LIB_FN void bd_scatter_element(const PkBandArgs& a, const PkBandFamilyArgs& g, int64_t e) {
  const int64_t c = e / a.nsol, i = e % a.nsol;
  const int64_t k = a.where ? (int64_t)a.where[i] : i;
  a.sol[c * g.c_sol + i] = k < 0 ? 0.0 : a.x[c * g.c_from + k];
}

// ---------------------------------------------------------------- the panel: threads of the one workgroup
// tile T: column c of the panel at T[c * BD_LD + r], row r = i - j0
PK_LIB_FN void bd_panel_load(const PkBandArgs& a, double* T, int t, int nbp, int rows) {
  for (int e = t; e < nbp * rows; e += PK_BLOCK) {
    const int c = e / rows, r = e % rows;
    T[c * BD_LD + r] = bd_stored(a, a.j0 + r, a.j0 + c) && !bd_fresh(a, a.j0 + r, a.j0 + c) ? *bd_at(a, a.j0 + r, a.j0 + c) : 0.0;
  }
}
PK_LIB_FN void bd_panel_store(const PkBandArgs& a, const double* T, const int* piv, int t, int nbp, int rows) {
  for (int e = t; e < nbp * rows; e += PK_BLOCK) {
    const int c = e / rows, r = e % rows;
    if (bd_stored(a, a.j0 + r, a.j0 + c)) *bd_at(a, a.j0 + r, a.j0 + c) = T[c * BD_LD + r];
  }
  if (t < nbp) a.ipiv[a.j0 + t] = (int32_t)(a.j0 + t + piv[t]);
}
// the pivot search of column jj: |.| of the rows jj ... jj + km into plane 0 (an entry that is not finite counts as +inf), the
// row's offset into plane 1
PK_LIB_FN void bd_amax_load(const double* T, double* s, int t, int jj, int km) {
  double v = -1.0;
  if (t <= km) {
    const double e = T[jj * BD_LD + jj + t];
    v = __builtin_isfinite(e) ? __builtin_fabs(e) : __builtin_inf();
  }
  s[t] = v;
  s[PK_BLOCK + t] = (double)t;
}
PK_LIB_FN void bd_amax_step(double* s, int w, int t) {
  if (t >= w) return;
  const double va = s[t], vb = s[t + w], ia = s[PK_BLOCK + t], ib = s[PK_BLOCK + t + w];
  if (vb > va || (vb == va && ib < ia)) { s[t] = vb; s[PK_BLOCK + t] = ib; }
}
PK_LIB_FN void bd_panel_swap(double* T, int* piv, int t, int jj, int jp, int nbp, int w) {
  if (t == 0) piv[jj] = jp;
  const int c = jj + t;
  if (jp != 0 && c < nbp && t <= 2 * w) {
    const double u = T[c * BD_LD + jj];
    T[c * BD_LD + jj] = T[c * BD_LD + jj + jp];
    T[c * BD_LD + jj + jp] = u;
  }
}
PK_LIB_FN void bd_panel_scale(double* T, int t, int jj, int km) {
  if (t < km) T[jj * BD_LD + jj + 1 + t] = T[jj * BD_LD + jj + 1 + t] / T[jj * BD_LD + jj];
}
PK_LIB_FN void bd_panel_update(double* T, int t, int jj, int km, int nbp, int w) {
  const int count = km * (int)bd_min(nbp - 1 - jj, 2 * w);
  for (int e = t; e < count; e += PK_BLOCK) {
    const int r = jj + 1 + e % km, c = jj + 1 + e / km;
    const double pr = T[jj * BD_LD + r] * T[c * BD_LD + jj];
    T[c * BD_LD + r] = T[c * BD_LD + r] - pr;
  }
}
PK_LIB_FN void bd_fail(const PkBandArgs& a, int t, double status, double column) {
  if (t == 0) { a.rec[BD_STATUS] = status; a.rec[BD_COLUMN] = column; }
}
PK_LIB_FN void bd_panel_record(const PkBandArgs& a, int t, double pmin, double pmax, double swaps) {
  if (t == 0) { a.rec[BD_MIN] = pmin; a.rec[BD_MAX] = pmax; a.rec[BD_SWAPS] = swaps; }
}

BD_BODY void bd_panel_body(const PkBandArgs& a, double* T, double* s, int* piv) {
  if (a.rec[BD_STATUS] != 0.0) return;
  const int nbp = (int)bd_min(PK_BD_NB, a.nb - a.j0), rows = (int)bd_min((int64_t)a.w + nbp, a.nb - a.j0);
  double pmin = a.rec[BD_MIN], pmax = a.rec[BD_MAX], swaps = a.rec[BD_SWAPS];
  BD_PHASE(bd_panel_load(a, T, t, nbp, rows));
  BD_ALIGN_CODE();
  for (int jj = 0; jj < nbp; ++jj) {
    const int km = (int)bd_min(a.w, a.nb - 1 - (a.j0 + jj));
    BD_PHASE(bd_amax_load(T, s, t, jj, km));
    BD_TREE(bd_amax_step, s);
    const double big = s[0];
    const int jp = (int)s[PK_BLOCK];
    if (!__builtin_isfinite(big) || big == 0.0) {      // (the same for every thread)
      BD_PHASE(bd_fail(a, t, __builtin_isfinite(big) ? 1.0 : 3.0, (double)(a.j0 + jj)));
      return;
    }
    pmin = big < pmin ? big : pmin;
    pmax = big > pmax ? big : pmax;
    if (jp != 0) swaps = swaps + 1.0;
    BD_PHASE(bd_panel_swap(T, piv, t, jj, jp, nbp, (int)a.w));
    BD_PHASE(bd_panel_scale(T, t, jj, km));
    BD_PHASE(bd_panel_update(T, t, jj, km, nbp, (int)a.w));
  }
  BD_PHASE(bd_panel_store(a, T, piv, t, nbp, rows));
  BD_PHASE(bd_panel_record(a, t, pmin, pmax, swaps));
}

// ---------------------------------------------------------------- a trailing column c behind the panel at j0: one workgroup
// thread t owns row j0 + t of the column's window (the rows the panel's pivots can touch)
PK_LIB_FN void bd_col_load(const PkBandArgs& a, double* col, int t, int64_t c, int rows) {
  if (t < rows) {
    const int64_t i = a.j0 + t;
    col[t] = i >= c - 2 * (int64_t)a.w && !bd_fresh(a, i, c) ? *bd_at(a, i, c) : 0.0;
  }
}
PK_LIB_FN void bd_col_store(const PkBandArgs& a, const double* col, int t, int64_t c, int rows) {
  if (t < rows) {
    const int64_t i = a.j0 + t;
    if (i >= c - 2 * (int64_t)a.w) *bd_at(a, i, c) = col[t];
  }
}
PK_LIB_FN void bd_col_swap(double* col, int t, int jj, int ip) {
  if (t == 0 && ip != jj) {
    const double u = col[jj];
    col[jj] = col[ip];
    col[ip] = u;
  }
}
PK_LIB_FN void bd_col_update(const PkBandArgs& a, double* col, int t, int jj, int km) {
  if (t < km) {
    const int64_t j = a.j0 + jj;
    const double pr = *bd_at(a, j + 1 + t, j) * col[jj];
    col[jj + 1 + t] = col[jj + 1 + t] - pr;
  }
}

BD_BODY void bd_update_body(const PkBandArgs& a, int64_t item, double* col) {
  if (a.rec[BD_STATUS] != 0.0) return;
  const int nbp = (int)bd_min(PK_BD_NB, a.nb - a.j0), rows = (int)bd_min((int64_t)a.w + nbp, a.nb - a.j0);
  const int64_t c = a.j0 + nbp + item;
  BD_PHASE(bd_col_load(a, col, t, c, rows));
  for (int jj = 0; jj < nbp; ++jj) {
    const int64_t j = a.j0 + jj;
    if (c > j + 2 * (int64_t)a.w) continue;
    const int km = (int)bd_min(a.w, a.nb - 1 - j), ip = (int)(a.ipiv[j] - a.j0);
    BD_PHASE(bd_col_swap(col, t, jj, ip));
    BD_PHASE(bd_col_update(a, col, t, jj, km));
  }
  BD_PHASE(bd_col_store(a, col, t, c, rows));
}

// ---------------------------------------------------------------- the sweeps of one right-hand side: one workgroup
// F: the chunk's columns of the factor (column jj at F[jj * BD_LW + ...]), ring: y_i at ring[i & (RING - 1)], ipl: the chunk's pivots
PK_LIB_FN void bd_fwd_load(const PkBandArgs& a, const double* y, double* F, double* ring, int* ipl, int t, int64_t j0, int cn) {
  const int64_t lo = j0 == 0 ? 0 : j0 + a.w, hi = bd_min(a.nb, j0 + PK_BD_CH + a.w);
  for (int64_t i = lo + t; i < hi; i += PK_BLOCK) ring[i & (PK_BD_RING - 1)] = y[i];
  for (int e = t; e < cn * a.w; e += PK_BLOCK) {
    const int jj = e / a.w, r = e % a.w;
    const int64_t j = j0 + jj;
    if (j + 1 + r < a.nb) F[jj * BD_LW + r] = *bd_at(a, j + 1 + r, j);
  }
  if (t < cn) ipl[t] = (int)a.ipiv[j0 + t];
}
PK_LIB_FN void bd_ring_swap(double* ring, int t, int64_t j, int64_t ip) {
  if (t == 0 && ip != j) {
    const double u = ring[j & (PK_BD_RING - 1)];
    ring[j & (PK_BD_RING - 1)] = ring[ip & (PK_BD_RING - 1)];
    ring[ip & (PK_BD_RING - 1)] = u;
  }
}
PK_LIB_FN void bd_fwd_axpy(const double* F, double* ring, int t, int64_t j, int jj, int km) {
  if (t < km) {
    const double pr = F[jj * BD_LW + t] * ring[j & (PK_BD_RING - 1)];
    ring[(j + 1 + t) & (PK_BD_RING - 1)] = ring[(j + 1 + t) & (PK_BD_RING - 1)] - pr;
  }
}
PK_LIB_FN void bd_ring_store(double* y, const double* ring, int t, int64_t j0, int cn) {
  if (t < cn) y[j0 + t] = ring[(j0 + t) & (PK_BD_RING - 1)];
}
PK_LIB_FN void bd_bwd_load(const PkBandArgs& a, const double* y, double* F, double* ring, int t, int64_t k0, int cn, bool first) {
  const int64_t w2 = 2 * (int64_t)a.w;
  const int64_t lo = bd_max(0, k0 - w2), hi = first ? a.nb : bd_max(0, k0 + PK_BD_CH - w2);
  for (int64_t i = lo + t; i < hi; i += PK_BLOCK) ring[i & (PK_BD_RING - 1)] = y[i];
  for (int e = t; e < cn * (int)(w2 + 1); e += PK_BLOCK) {
    const int kk = e / (int)(w2 + 1), r = e % (int)(w2 + 1);
    const int64_t k = k0 + kk, i = k - w2 + r;
    if (i >= 0) F[kk * BD_LW + r] = *bd_at(a, i, k);
  }
}
PK_LIB_FN void bd_bwd_div(const PkBandArgs& a, const double* F, double* ring, int t, int64_t k, int kk) {
  if (t == 0) ring[k & (PK_BD_RING - 1)] = ring[k & (PK_BD_RING - 1)] / F[kk * BD_LW + 2 * a.w];
}
PK_LIB_FN void bd_bwd_axpy(const PkBandArgs& a, const double* F, double* ring, int t, int64_t k, int kk, int cnt) {
  for (int r = t; r < cnt; r += PK_BLOCK) {      // row i = k - 1 - r
    const double pr = F[kk * BD_LW + 2 * a.w - 1 - r] * ring[k & (PK_BD_RING - 1)];
    ring[(k - 1 - r) & (PK_BD_RING - 1)] = ring[(k - 1 - r) & (PK_BD_RING - 1)] - pr;
  }
}

BD_BODY void bd_solve_body(const PkBandArgs& a, int64_t q, double* F, double* ring, int* ipl) {
  if (a.rec[BD_STATUS] != 0.0) return;
  double* y = a.Y + q * a.nb;
  for (int64_t j0 = 0; j0 < a.nb; j0 += PK_BD_CH) {
    const int cn = (int)bd_min(PK_BD_CH, a.nb - j0);
    BD_PHASE(bd_fwd_load(a, y, F, ring, ipl, t, j0, cn));
    for (int jj = 0; jj < cn; ++jj) {
      const int64_t j = j0 + jj;
      const int km = (int)bd_min(a.w, a.nb - 1 - j);
      BD_PHASE(bd_ring_swap(ring, t, j, (int64_t)ipl[jj]));
      BD_PHASE(bd_fwd_axpy(F, ring, t, j, jj, km));
    }
    BD_PHASE(bd_ring_store(y, ring, t, j0, cn));
  }
  bool first = true;
  for (int64_t k0 = a.nb > 0 ? ((a.nb - 1) / PK_BD_CH) * PK_BD_CH : -1; k0 >= 0; k0 -= PK_BD_CH) {
    const int cn = (int)bd_min(PK_BD_CH, a.nb - k0);
    BD_PHASE(bd_bwd_load(a, y, F, ring, t, k0, cn, first));
    first = false;
    for (int kk = cn - 1; kk >= 0; --kk) {
      const int64_t k = k0 + kk;
      const int cnt = (int)bd_min(2 * (int64_t)a.w, k);
      BD_PHASE(bd_bwd_div(a, F, ring, t, k, kk));
      BD_PHASE(bd_bwd_axpy(a, F, ring, t, k, kk, cnt));
    }
    BD_PHASE(bd_ring_store(y, ring, t, k0, cn));
  }
}

// ---------------------------------------------------------------- the border
// thread t of piece pc of right-hand side r: the p dots U_a . Y_r, one plane each
PK_LIB_FN void bd_dot_thread(const PkBandArgs& a, int64_t r, int64_t pc, int t, double* s) {
  const double* y = a.Y + r * a.nb;
  for (int q = 0; q < a.p; ++q) {
    const double* u = a.U + (int64_t)q * a.nb;
    double acc = 0.0;
    for (int j = 0; j < PK_LIB_PER_THREAD; ++j) {
      const int64_t i = pc * PK_LIB_PIECE + t + (int64_t)PK_BLOCK * j;
      if (i < a.nb) {
        const double pr = u[i] * y[i];
        acc = acc + pr;
      }
    }
    s[q * PK_BLOCK + t] = acc;
  }
}
PK_LIB_FN void bd_dot_store(const PkBandArgs& a, int64_t r, int64_t pc, int q, const double* s) {
  a.partial[(r * a.p + q) * a.n_pieces + pc] = s[q * PK_BLOCK];
}
PK_LIB_FN void bd_dots_keep(double* dots, const double* s, int t, int r, int p) {
  if (t < p) dots[r * p + t] = s[t * PK_BLOCK];
}
// thread 0: S = C - U^T Y_U and its LU with partial pivoting, ONCE for the k columns.  The multipliers are kept as they are
// formed (L[r + k p], never exchanged afterwards) beside the interchanges piv[k], so that a column can replay on its own t
// exactly what an LU of [S | t] would do to t, step by step; piv[p] is 1 after a failed pivot.
PK_LIB_FN void bd_border_factor(const PkBandArgs& a, int t, const double* dots, double* S, double* L, int* piv) {
  if (t != 0) return;
  const int p = a.p;
  piv[p] = 0;
  for (int c = 0; c < p; ++c)
    for (int r = 0; r < p; ++r) S[r + c * p] = a.C[r + c * p] - dots[c * p + r];
  for (int k = 0; k < p; ++k) {
    int ip = k;
    double big = -1.0;
    for (int r = k; r < p; ++r) {
      const double e = S[r + k * p];
      const double m = __builtin_isfinite(e) ? __builtin_fabs(e) : __builtin_inf();
      if (m > big) { big = m; ip = r; }
    }
    if (!__builtin_isfinite(big) || big == 0.0) {
      a.rec[BD_STATUS] = __builtin_isfinite(big) ? 2.0 : 3.0;
      a.rec[BD_COLUMN] = (double)(a.nb + k);
      piv[p] = 1;
      return;
    }
    piv[k] = ip;
    if (ip != k)
      for (int c = 0; c < p; ++c) { const double u = S[k + c * p]; S[k + c * p] = S[ip + c * p]; S[ip + c * p] = u; }
    for (int r = k + 1; r < p; ++r) {
      const double l = S[r + k * p] / S[k + k * p];
      S[r + k * p] = l;
      L[r + k * p] = l;
      for (int c = k + 1; c < p; ++c) { const double pr = l * S[k + c * p]; S[r + c * p] = S[r + c * p] - pr; }
    }
  }
}
// thread c < k: t = b_C - U^T y_b of column c, the interchanges and multipliers replayed, the back substitution; v is the
// column's own slice of P_CAP doubles
PK_LIB_FN void bd_border_column(const PkBandArgs& a, int k_rhs, int c, const double* dots, const double* S, const double* L, const int* piv,
                                double* vs) {
  const int p = a.p;
  if (c >= k_rhs || piv[p] != 0) return;
  double* v = vs + c * PK_BD_P_CAP;
  for (int r = 0; r < p; ++r) v[r] = a.bc[(int64_t)c * p + r] - dots[(p + c) * p + r];
  for (int k = 0; k < p; ++k) {
    const int ip = piv[k];
    if (ip != k) { const double u = v[k]; v[k] = v[ip]; v[ip] = u; }
    for (int r = k + 1; r < p; ++r) {
      const double pr = L[r + k * p] * v[k];
      v[r] = v[r] - pr;
    }
  }
  for (int k = p - 1; k >= 0; --k) {
    double e = v[k];
    for (int q = k + 1; q < p; ++q) { const double pr = S[k + q * p] * v[q]; e = e - pr; }
    v[k] = e / S[k + k * p];
  }
  for (int k = 0; k < p; ++k) a.x[(int64_t)c * (a.nb + p) + a.nb + k] = v[k];
}

BD_BODY void bd_border_body(const PkBandArgs& a, int k_rhs, double* s, double* dots, double* S, double* L, int* piv, double* vs) {
  if (a.rec[BD_STATUS] != 0.0) return;
  for (int r = 0; r < a.p + k_rhs; ++r) {
    PkBandArgs b = a;
    b.partial = a.partial + (int64_t)r * a.p * a.n_pieces;
    b.planes = a.p;
    BD_PHASE(lib_scalar_thread(b, t, s));
    BD_TREE(lib_planes_step, s, (int)a.p);
    BD_PHASE(bd_dots_keep(dots, s, t, r, a.p));
  }
  BD_PHASE(bd_border_factor(a, t, dots, S, L, piv));
  BD_PHASE(bd_border_column(a, k_rhs, t, dots, S, L, piv, vs));
}

#ifdef __HIPCC__
// ---------------------------------------------------------------- kernels (gfx950): grid (work items, entries)
// Entry blockIdx.y's arguments, then the walk of blockIdx.x over the body.
__global__ void __launch_bounds__(PK_BLOCK) pk_bd_init_k(PkBandFamilyArgs g) {
  const PkBandArgs a = bd_entry(g, (int64_t)blockIdx.y);
  bd_init_thread(a, (int)threadIdx.x);
}

__global__ void __launch_bounds__(PK_BLOCK) pk_bd_fill_k(PkBandFamilyArgs g) {
  const PkBandArgs a = bd_entry(g, (int64_t)blockIdx.y);
  const int64_t items = bd_items(a.dests);
  for (int64_t item = (int64_t)blockIdx.x; item < items; item += (int64_t)gridDim.x) {
    const int64_t d = item * PK_BLOCK + (int64_t)threadIdx.x;
    if (d < a.dests) bd_fill_element(a, d);
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_bd_panel_k(PkBandFamilyArgs g) {
  __shared__ double T[BD_LD * PK_BD_NB];
  __shared__ double s[2 * PK_BLOCK];
  __shared__ int piv[PK_BD_NB];
  const PkBandArgs a = bd_entry(g, (int64_t)blockIdx.y);
  bd_panel_body(a, T, s, piv);
}

// work item = a trailing column
__global__ void __launch_bounds__(PK_BLOCK) pk_bd_update_k(PkBandFamilyArgs g) {
  __shared__ double col[PK_BLOCK];
  const PkBandArgs a = bd_entry(g, (int64_t)blockIdx.y);
  for (int64_t item = (int64_t)blockIdx.x; item < g.columns_j; item += (int64_t)gridDim.x) bd_update_body(a, item, col);
}

__global__ void __launch_bounds__(PK_BLOCK) pk_bd_prep_k(PkBandFamilyArgs g) {
  const PkBandArgs a = bd_entry(g, (int64_t)blockIdx.y);
  const int64_t len = a.nb * a.p + (int64_t)g.k * (a.nb + a.p), items = bd_items(len);
  for (int64_t item = (int64_t)blockIdx.x; item < items; item += (int64_t)gridDim.x) {
    const int64_t e = item * PK_BLOCK + (int64_t)threadIdx.x;
    if (e < len) bd_prep_element(a, g, e);
  }
}

// work item = a sweep vector: a column of U or a right-hand side
__global__ void __launch_bounds__(PK_BLOCK) pk_bd_solve_k(PkBandFamilyArgs g) {
  __shared__ double F[PK_BD_CH * BD_LW];
  __shared__ double ring[PK_BD_RING];
  __shared__ int ipl[PK_BD_CH];
  const PkBandArgs a = bd_entry(g, (int64_t)blockIdx.y);
  const int64_t R = (int64_t)a.p + g.k;
  for (int64_t q = (int64_t)blockIdx.x; q < R; q += (int64_t)gridDim.x) bd_solve_body(a, q, F, ring, ipl);
}

// work item = sweep vector * n_pieces + piece
__global__ void __launch_bounds__(PK_BLOCK) pk_bd_dot_k(PkBandFamilyArgs g) {
  __shared__ double s[PK_BD_P_CAP * PK_BLOCK];
  const PkBandArgs a = bd_entry(g, (int64_t)blockIdx.y);
  const int t = (int)threadIdx.x;
  const int64_t items = ((int64_t)a.p + g.k) * a.n_pieces;
  for (int64_t item = (int64_t)blockIdx.x; item < items; item += (int64_t)gridDim.x) {
    const int64_t r = item / a.n_pieces, pc = item % a.n_pieces;
    bd_dot_thread(a, r, pc, t, s);
    __syncthreads();
    lib_tree(lib_planes_step, s, t, (int)a.p);
    if (t < a.p) bd_dot_store(a, r, pc, t, s);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_bd_border_k(PkBandFamilyArgs g) {
  __shared__ double s[PK_BD_P_CAP * PK_BLOCK];
  __shared__ double dots[(PK_BD_P_CAP + PK_BD_RHS_CAP) * PK_BD_P_CAP], S[PK_BD_P_CAP * PK_BD_P_CAP], L[PK_BD_P_CAP * PK_BD_P_CAP];
  __shared__ double vs[PK_BD_RHS_CAP * PK_BD_P_CAP];
  __shared__ int piv[PK_BD_P_CAP + 1];
  const PkBandArgs a = bd_entry(g, (int64_t)blockIdx.y);
  bd_border_body(a, (int)g.k, s, dots, S, L, piv, vs);
}

__global__ void __launch_bounds__(PK_BLOCK) pk_bd_xb_k(PkBandFamilyArgs g) {
  const PkBandArgs a = bd_entry(g, (int64_t)blockIdx.y);
  if (a.rec[BD_STATUS] != 0.0) return;
  const int64_t len = (int64_t)g.k * a.nb, items = bd_items(len);
  for (int64_t item = (int64_t)blockIdx.x; item < items; item += (int64_t)gridDim.x) {
    const int64_t e = item * PK_BLOCK + (int64_t)threadIdx.x;
    if (e < len) bd_xb_element(a, e);
  }
}

__global__ void __launch_bounds__(PK_BLOCK) pk_bd_scatter_k(PkBandFamilyArgs g) {
  const PkBandArgs a = bd_entry(g, (int64_t)blockIdx.y);
  if (a.rec[BD_STATUS] != 0.0) return;
  const int64_t len = (int64_t)g.k * a.nsol, items = bd_items(len);
  for (int64_t item = (int64_t)blockIdx.x; item < items; item += (int64_t)gridDim.x) {
    const int64_t e = item * PK_BLOCK + (int64_t)threadIdx.x;
    if (e < len) bd_scatter_element(a, g, e);
  }
}
#else
// ---------------------------------------------------------------- host stand-in: the identical walk of entry y
// (PK_LIB_LAUNCH_Y walks the entries outermost)
static void bd_init_host(const PkBandFamilyArgs& g, unsigned, unsigned y) { bd_init_thread(bd_entry(g, y), 0); }
static void bd_fill_host(const PkBandFamilyArgs& g, unsigned grid, unsigned y) {
  const PkBandArgs a = bd_entry(g, y);
  lib_elements_host(grid, a.dests, [&](int64_t d) { bd_fill_element(a, d); });
}
static void bd_panel_host(const PkBandFamilyArgs& g, unsigned, unsigned y) {
  static double T[BD_LD * PK_BD_NB];
  double s[2 * PK_BLOCK];
  int piv[PK_BD_NB];
  bd_panel_body(bd_entry(g, y), T, s, piv);
}
static void bd_update_host(const PkBandFamilyArgs& g, unsigned grid, unsigned y) {
  const PkBandArgs a = bd_entry(g, y);
  double col[PK_BLOCK];
  lib_walk_host(grid, g.columns_j, [&](int64_t item) { bd_update_body(a, item, col); });
}
static void bd_prep_host(const PkBandFamilyArgs& g, unsigned grid, unsigned y) {
  const PkBandArgs a = bd_entry(g, y);
  lib_elements_host(grid, a.nb * a.p + (int64_t)g.k * (a.nb + a.p), [&](int64_t e) { bd_prep_element(a, g, e); });
}
static void bd_solve_host(const PkBandFamilyArgs& g, unsigned grid, unsigned y) {
  static double F[PK_BD_CH * BD_LW];
  double ring[PK_BD_RING];
  int ipl[PK_BD_CH];
  const PkBandArgs a = bd_entry(g, y);
  lib_walk_host(grid, (int64_t)a.p + g.k, [&](int64_t q) { bd_solve_body(a, q, F, ring, ipl); });
}
static void bd_dot_host(const PkBandFamilyArgs& g, unsigned grid, unsigned y) {
  static double s[PK_BD_P_CAP * PK_BLOCK];
  const PkBandArgs a = bd_entry(g, y);
  lib_walk_host(grid, ((int64_t)a.p + g.k) * a.n_pieces, [&](int64_t item) {
    const int64_t r = item / a.n_pieces, pc = item % a.n_pieces;
    for (int t = 0; t < PK_BLOCK; ++t) bd_dot_thread(a, r, pc, t, s);
    lib_tree_host(lib_planes_step, s, (int)a.p);
    for (int q = 0; q < a.p; ++q) bd_dot_store(a, r, pc, q, s);
  });
}
static void bd_border_host(const PkBandFamilyArgs& g, unsigned, unsigned y) {
  static double s[PK_BD_P_CAP * PK_BLOCK];
  double dots[(PK_BD_P_CAP + PK_BD_RHS_CAP) * PK_BD_P_CAP], S[PK_BD_P_CAP * PK_BD_P_CAP], L[PK_BD_P_CAP * PK_BD_P_CAP];
  double vs[PK_BD_RHS_CAP * PK_BD_P_CAP];
  int piv[PK_BD_P_CAP + 1];
  bd_border_body(bd_entry(g, y), (int)g.k, s, dots, S, L, piv, vs);
}
static void bd_xb_host(const PkBandFamilyArgs& g, unsigned grid, unsigned y) {
  const PkBandArgs a = bd_entry(g, y);
  if (a.rec[BD_STATUS] != 0.0) return;
  lib_elements_host(grid, (int64_t)g.k * a.nb, [&](int64_t e) { bd_xb_element(a, e); });
}
static void bd_scatter_host(const PkBandFamilyArgs& g, unsigned grid, unsigned y) {
  const PkBandArgs a = bd_entry(g, y);
  if (a.rec[BD_STATUS] != 0.0) return;
  lib_elements_host(grid, (int64_t)g.k * a.nsol, [&](int64_t e) { bd_scatter_element(a, g, e); });
}
#endif

void free_band(pk_ctx* c) {
  PkBand& b = c->band;
  release(b.d_refine); release(b.d_rpartial);
  release(b.d_map); release(b.d_order); release(b.d_where);
  release(b.d_work); release(b.d_ipiv); release(b.d_partial); release(b.d_scratch); release(b.d_raw);
  release(b.d_bwork); release(b.d_bipiv); release(b.d_bpartial); release(b.d_bscratch); release(b.d_braw);
  release(b.d_mwork); release(b.d_mpartial); release(b.d_mscratch);
  b = PkBand{};
}

namespace {

int64_t bd_ldab(int64_t w) { return 3 * w + 1; }
// doubles of [band | U | C] and of the rest of a solve's work [Y | x | b_C | record]
size_t bd_matrix_doubles(int64_t nb, int64_t w, int64_t p) { return (size_t)(bd_ldab(w) * nb + nb * p + p * p); }
size_t bd_solve_doubles(int64_t nb, int64_t p) { return (size_t)(nb * (p + 1) + (nb + p) + p + PK_BD_REC); }

int bd_shape(pk_ctx* c, int64_t nb, int64_t w, int64_t p, const char* who) {
  if (nb < 0 || w < 0 || w > PK_BD_W_CAP || p < 0 || p > PK_BD_P_CAP || nb > (int64_t)INT32_MAX - PK_BD_P_CAP)
    return fail(c, 134, "%s: Nb = %lld (not negative), w = %lld (0 ... %d), p = %lld (0 ... %d)", who, (long long)nb, (long long)w,
                (int)PK_BD_W_CAP, (long long)p, (int)PK_BD_P_CAP);
  return 0;
}

// the slices of a solve's work for k right-hand sides, into the arguments: [Y | x | b_C]
void bd_solve_slices(PkBandArgs& a, int64_t k, double* work) {
  a.Y = work;
  a.x = a.Y + a.nb * (a.p + k);
  a.bc = a.x + k * (a.nb + a.p);
}

// init, the panels and the updates behind them for B entries: the arguments hold band, ipiv, rec and the shape
int bd_enqueue_factor(pk_ctx* c, PkBandFamilyArgs g, int32_t B, bool fill, hipStream_t st) {
  const PkBandArgs& a = g.a;
  PK_LIB_LAUNCH_Y(c, pk_bd_init_k, bd_init_host, 1u, B, st, g);
  if (fill && a.dests > 0) PK_LIB_LAUNCH_Y(c, pk_bd_fill_k, bd_fill_host, lib_grid(lib_elem_items(a.dests)), B, st, g);
  for (int64_t j0 = 0; j0 < a.nb; j0 += PK_BD_NB) {
    g.a.j0 = j0;
    PK_LIB_LAUNCH_Y(c, pk_bd_panel_k, bd_panel_host, 1u, B, st, g);
    const int64_t j1 = std::min<int64_t>(j0 + PK_BD_NB, a.nb);
    g.columns_j = std::min<int64_t>(j1 - 1 + 2 * (int64_t)a.w, a.nb - 1) - j1 + 1;
    if (g.columns_j > 0) PK_LIB_LAUNCH_Y(c, pk_bd_update_k, bd_update_host, lib_grid(g.columns_j), B, st, g);
  }
  return 0;
}

// right-hand sides, sweeps, border and scatter for B entries of k columns, in the launches of ONE solve (3 without a border, 6
// with one): the arguments hold everything but the scatter's source
int bd_enqueue_solve(pk_ctx* c, PkBandFamilyArgs g, int32_t B, hipStream_t st) {
  const PkBandArgs& a = g.a;
  const int64_t k = g.k, N = a.nb + a.p;
  if (N > 0) PK_LIB_LAUNCH_Y(c, pk_bd_prep_k, bd_prep_host, lib_grid(lib_elem_items(a.nb * a.p + k * N)), B, st, g);
  if (a.nb > 0) PK_LIB_LAUNCH_Y(c, pk_bd_solve_k, bd_solve_host, lib_grid((int64_t)a.p + k), B, st, g);
  double* from = a.Y;      // (without a border the solutions are the swept right-hand sides themselves; Y and x move by the same stride)
  g.c_from = a.nb;
  if (a.p > 0) {
    PK_LIB_LAUNCH_Y(c, pk_bd_dot_k, bd_dot_host, lib_grid(((int64_t)a.p + k) * a.n_pieces), B, st, g);
    PK_LIB_LAUNCH_Y(c, pk_bd_border_k, bd_border_host, 1u, B, st, g);
    if (a.nb > 0) PK_LIB_LAUNCH_Y(c, pk_bd_xb_k, bd_xb_host, lib_grid(lib_elem_items(k * a.nb)), B, st, g);
    from = a.x;
    g.c_from = N;
  }
  g.a.x = from;
  if (a.nsol > 0) PK_LIB_LAUNCH_Y(c, pk_bd_scatter_k, bd_scatter_host, lib_grid(lib_elem_items(k * a.nsol)), B, st, g);
  return 0;
}

int bd_partial(pk_ctx* c, PkBandArgs& a, const char* who) {
  a.n_pieces = lib_dot_pieces(a.nb);
  if (a.p > 0) {
    if (const int rc = lib_reserve(c, c->band.d_partial, c->band.partial_cap, (size_t)(a.p + 1) * (size_t)a.p * (size_t)a.n_pieces, 136, who,
                                   "partial sums"))
      return rc;
  }
  a.partial = c->band.d_partial;
  return 0;
}

int bd_context(pk_ctx* c, const char* who) {
  if (c->shard.flags || c->exchange.world > 1) return fail(c, 119, "%s: not offered for a sharded context", who);
  return 0;
}

// is there a plan, and do the CSR maps still have the sources it was made for?
int bd_plan_current(pk_ctx* c, const char* who) {
  if (!c->band.planned) return fail(c, 134, "%s: no plan (pk_band_plan)", who);
  if (c->band.sources != c->csr[1].n_unique + c->csr[0].n_unique + (int64_t)c->n + c->m)
    return fail(c, 134, "%s: the CSR maps changed since pk_band_plan", who);
  return 0;
}

// the arguments of the planned system, one entry with one column: the matrix, ipiv and the record in the context's arrays
PkBandFamilyArgs bd_planned(pk_ctx* c) {
  const PkBand& b = c->band;
  PkBandFamilyArgs g{};
  PkBandArgs& a = g.a;
  g.k = 1;
  a.nb = b.nb; a.w = (int32_t)b.w; a.p = (int32_t)b.p; a.ldab = bd_ldab(b.w);
  a.band = b.d_work; a.U = a.band + a.ldab * a.nb; a.C = a.U + a.nb * a.p;
  a.dests = (int64_t)bd_matrix_doubles(b.nb, b.w, b.p);
  bd_solve_slices(a, 1, b.d_work + a.dests);
  a.rec = a.bc + a.p;
  a.ipiv = (int32_t*)b.d_ipiv;
  a.map = b.d_map; a.order = b.d_order; a.where = b.d_where;
  a.nh = c->csr[1].n_unique; a.nj = c->csr[0].n_unique; a.ns1 = c->n;
  a.nsol = (int64_t)c->n + c->m;
  return g;
}

// the arguments of a raw form, one entry with one column: the caller's arrays and the shape (no fill: the kernels only read U
// and C)
PkBandFamilyArgs bd_raw(int64_t nb, int32_t w, int32_t p, double* d_band, const double* d_U, const double* d_C, const double* d_rhs,
                        int32_t* d_ipiv, double* d_x, double* d_rec) {
  PkBandFamilyArgs g{};
  PkBandArgs& a = g.a;
  g.k = 1;
  a.nb = nb; a.w = w; a.p = p; a.ldab = bd_ldab(w);
  a.band = d_band; a.U = const_cast<double*>(d_U); a.C = const_cast<double*>(d_C);
  a.ipiv = d_ipiv; a.rec = d_rec; a.rhs = d_rhs; a.sol = d_x; a.nsol = nb + p;
  return g;
}

// ---------------------------------------------------------------- the batch
int bd_batch_size(pk_ctx* c, int32_t B, const char* who) {
  if (B < 1 || B > PK_BD_BATCH_CAP) return fail(c, 134, "%s: a batch of %d (1 ... %d)", who, B, (int)PK_BD_BATCH_CAP);
  return 0;
}

// a source may be shared (stride 0) or its entries lie at least a length apart; an output's entries always do
int bd_stride(pk_ctx* c, int64_t stride, int64_t len, bool source, const char* who, const char* what) {
  if ((source && stride == 0) || stride >= std::max<int64_t>(len, source ? 1 : 0)) return 0;
  return fail(c, 134, "%s: a stride of %lld doubles for %s of %lld (%sat least the length)", who, (long long)stride, what, (long long)len,
              source ? "0, or " : "");
}

// an array of the batch for B entries; what it was reserved for goes into the message
int bd_batch_reserve(pk_ctx* c, double*& p, size_t& cap, size_t per, int32_t B, bool factors, const char* who, const char* what) {
  if (per * (size_t)B <= cap) return 0;
  char named[160];
  std::snprintf(named, sizeof named, "%s of a batch of %d (%zu doubles each)", what, (int)B, per);
  const int rc = lib_reserve(c, p, cap, per * (size_t)B, 136, who, named);
  if (!rc && factors) c->band.batch = 0;      // (the array that went held the last batch factorisation)
  return rc;
}

// doubles of one entry of the planned batch, [band | U | C | Y | x | b_C]; the B records lie behind the B entries
size_t bd_entry_doubles(int64_t nb, int64_t w, int64_t p) { return bd_matrix_doubles(nb, w, p) + bd_solve_doubles(nb, p) - PK_BD_REC; }
size_t bd_ipiv_doubles(int64_t nb) { return (size_t)nb / 2 + 1; }

// the arguments of B planned systems in the batch's arrays (reserved for at least B)
PkBandFamilyArgs bd_planned_batch(pk_ctx* c, int32_t B) {
  const PkBand& b = c->band;
  PkBandFamilyArgs g = bd_planned(c);
  PkBandArgs& a = g.a;
  const int64_t per = (int64_t)bd_entry_doubles(b.nb, b.w, b.p);
  a.band = b.d_bwork; a.U = a.band + a.ldab * a.nb; a.C = a.U + a.nb * a.p;
  bd_solve_slices(a, 1, b.d_bwork + a.dests);
  a.rec = b.d_bwork + per * B;
  a.ipiv = (int32_t*)b.d_bipiv;
  g.s_band = g.s_U = g.s_C = g.s_work = per;
  g.s_rec = PK_BD_REC;
  g.s_ipiv = 2 * (int64_t)bd_ipiv_doubles(b.nb);
  return g;
}

int bd_partial_batch(pk_ctx* c, PkBandFamilyArgs& g, int32_t B, const char* who) {
  PkBandArgs& a = g.a;
  a.n_pieces = lib_dot_pieces(a.nb);
  const size_t per = (size_t)(a.p + 1) * (size_t)a.p * (size_t)a.n_pieces;
  if (a.p > 0) {
    if (const int rc = bd_batch_reserve(c, c->band.d_bpartial, c->band.bpartial_cap, per, B, false, who, "the partial sums")) return rc;
  }
  a.partial = a.p > 0 ? c->band.d_bpartial : nullptr;
  g.s_partial = a.p > 0 ? (int64_t)per : 0;
  return 0;
}

// ---------------------------------------------------------------- the block: k right-hand sides behind one factorisation
int bd_rhs_count(pk_ctx* c, int32_t k, const char* who) {
  if (k < 1 || k > PK_BD_RHS_CAP) return fail(c, 134, "%s: a block of %d right-hand sides (1 ... %d)", who, k, (int)PK_BD_RHS_CAP);
  return 0;
}

// the block's work arrays for g.k right-hand sides of the shape in g.a, and its slices into the arguments
int bd_multi_work(pk_ctx* c, PkBandFamilyArgs& g, const char* who) {
  PkBandArgs& a = g.a;
  PkBand& b = c->band;
  const size_t k = (size_t)g.k, nb = (size_t)a.nb, p = (size_t)a.p;
  char named[160];
  std::snprintf(named, sizeof named, "the sweep vectors and solutions of a block of %d right-hand sides", (int)g.k);
  int rc = lib_reserve(c, b.d_mwork, b.mwork_cap, (p + k) * nb + k * (nb + p) + k * p + 1, 136, who, named);
  if (rc) return rc;
  a.n_pieces = lib_dot_pieces(a.nb);
  if (p > 0) {
    std::snprintf(named, sizeof named, "the partial sums of a block of %d right-hand sides", (int)g.k);
    if ((rc = lib_reserve(c, b.d_mpartial, b.mpartial_cap, (p + k) * p * (size_t)a.n_pieces, 136, who, named))) return rc;
  }
  a.partial = p > 0 ? b.d_mpartial : nullptr;
  bd_solve_slices(a, g.k, b.d_mwork);
  return 0;
}

// ---------------------------------------------------------------- the host forms of one system: k right-hand sides
// Behind the caller's own refusals: the plan, the linearization, then b and [s1 | s2] up into `scratch` ([b | s1 | s2 | x], named
// `what` in error 136), the factorisation, solve(d_b, d_x), and x back where the record says solved.  The batch's host form
// is not folded in: it has B rows of s1 and s2 at strides of their own, B records and a copy-back per entry's status.
template <class Solve>
int bd_host_form(pk_ctx* c, const char* who, size_t k, double*& scratch, size_t& cap, const char* what, const double* s1, const double* s2,
                 const double* b, double* x, double* rec, Solve solve) {
  const double *jvals = nullptr, *hvals = nullptr;
  int rc;
  if (!c->band.planned) return fail(c, 134, "%s: no plan (pk_band_plan)", who);
  if ((rc = solve_linearized(c, true, jvals, hvals, who))) return rc;
  const size_t n = (size_t)c->n, m = (size_t)c->m, N = n + m;
  if ((rc = lib_reserve(c, scratch, cap, (2 * k + 1) * N + 1, 136, who, what))) return rc;
  double *d_b = scratch, *d_s = d_b + N * k, *d_x = d_s + N;
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_upload(c, d_b, b, N * k)) || (rc = lib_upload(c, d_s, s1, n)) || (rc = lib_upload(c, d_s + n, s2, m))) return rc;
  if ((rc = pk_band_factor_dev(c, hvals, jvals, d_s, d_s + n)) || (rc = solve(d_b, d_x))) return rc;
  std::vector<double> got(N * k + 1);
  if (N) PK_HIP(c, hipMemcpyAsync(got.data(), d_x, sizeof(double) * N * k, hipMemcpyDeviceToHost, c->stream));
  if ((rc = pk_band_record(c, rec))) return rc;      // (synchronises)
  if (rec[BD_STATUS] == 0.0) std::copy(got.begin(), got.begin() + (long)(N * k), x);
  return 0;
}

}  // namespace

// ---------------------------------------------------------------- for pk_band_refine.cpp (pk_runtime.h)
int band_planned_ready(pk_ctx* c, bool factored, const char* who) {
  if (const int rc = bd_plan_current(c, who)) return rc;
  if (factored && !c->band.factored) return fail(c, 134, "%s: no factorisation (pk_band_plan, pk_band_factor_dev)", who);
  return 0;
}
int band_planned_partial(pk_ctx* c, const char* who) {
  PkBandArgs a = bd_planned(c).a;
  return bd_partial(c, a, who);
}
int band_planned_solve(pk_ctx* c, const double* d_rhs, double* d_sol, const char* who) {
  PkBandFamilyArgs g = bd_planned(c);
  if (const int rc = bd_partial(c, g.a, who)) return rc;
  g.a.rhs = d_rhs; g.a.sol = d_sol;
  return bd_enqueue_solve(c, g, 1, c->stream);
}
const double* band_planned_record(pk_ctx* c) { return bd_planned(c).a.rec; }

extern "C" {

int pk_band_plan(pk_ctx* c, int64_t nb, int32_t w, int32_t p, const int32_t* order, const int32_t* map) {
  const char* who = "pk_band_plan";
  int rc = ready(c);
  if (rc || (rc = bd_context(c, who))) return rc;
  if (!order || !map) return fail(c, 60, "null host buffer");
  if ((rc = bd_shape(c, nb, w, p, who))) return rc;
  const int64_t N = nb + p, total = (int64_t)c->n + c->m;
  const int64_t sources = c->csr[1].n_unique + c->csr[0].n_unique + total;
  if (N > total) return fail(c, 134, "%s: %lld unknowns for a system of %lld", who, (long long)N, (long long)total);
  std::vector<int32_t> where((size_t)total + 1, -1);
  for (int64_t k = 0; k < N; ++k) {
    if (order[k] < 0 || order[k] >= total || where[(size_t)order[k]] >= 0)
      return fail(c, 134, "%s: order[%lld] = %d is outside the system or repeated", who, (long long)k, order[k]);
    where[(size_t)order[k]] = (int32_t)k;
  }
  const size_t dests = bd_matrix_doubles(nb, w, p);
  if (2 * dests > (size_t)INT32_MAX * 2) return fail(c, 134, "%s: %zu stored slots do not fit 32-bit positions", who, dests);
  for (size_t d = 0; d < 2 * dests; ++d) {
    const int64_t k = map[d] < 0 ? -(int64_t)map[d] : (int64_t)map[d];
    if (k > sources) return fail(c, 134, "%s: a source beyond [hvals | jvals | s1 | s2] (%lld of %lld; set the CSR maps first)", who, (long long)k,
                                 (long long)sources);
  }
  PK_HIP(c, hipSetDevice(c->device));
  PkBand fresh{};
  fresh.nb = nb; fresh.w = w; fresh.p = p; fresh.sources = sources;
  const auto drop = [&](int code, const char* what) {
    release(fresh.d_map); release(fresh.d_order); release(fresh.d_where); release(fresh.d_work); release(fresh.d_ipiv);
    return fail(c, code, "%s: no device memory for %s", who, what);
  };
  if (upload(c, (void**)&fresh.d_map, map, sizeof(int32_t) * 2 * dests) || upload(c, (void**)&fresh.d_order, order, sizeof(int32_t) * (size_t)N) ||
      upload(c, (void**)&fresh.d_where, where.data(), sizeof(int32_t) * (size_t)total))
    return drop(136, "the plan");
  size_t cap = 0;
  if (lib_reserve(c, fresh.d_work, cap, dests + bd_solve_doubles(nb, p), 136, who, "the band, the border and the right-hand sides"))
    return drop(136, "the band, the border and the right-hand sides");
  cap = 0;
  if (lib_reserve(c, fresh.d_ipiv, cap, (size_t)nb / 2 + 1, 136, who, "the interchanges")) return drop(136, "the interchanges");
  PK_HIP(c, hipDeviceSynchronize());      // work enqueued earlier may still use the plan that goes
  fresh.d_partial = c->band.d_partial; fresh.partial_cap = c->band.partial_cap;
  fresh.d_scratch = c->band.d_scratch; fresh.scratch_cap = c->band.scratch_cap;
  fresh.d_raw = c->band.d_raw; fresh.raw_cap = c->band.raw_cap;
  fresh.d_refine = c->band.d_refine; fresh.refine_cap = c->band.refine_cap;      // (sized by n + m, not by the plan)
  fresh.d_rpartial = c->band.d_rpartial; fresh.rpartial_cap = c->band.rpartial_cap;
  c->band.d_partial = nullptr; c->band.d_scratch = nullptr; c->band.d_raw = nullptr; c->band.d_refine = nullptr; c->band.d_rpartial = nullptr;
  free_band(c);
  c->band = fresh;
  c->band.planned = true;
  return 0;
}

int pk_band_factor_dev(pk_ctx* c, const double* d_hvals, const double* d_jvals, const double* d_s1, const double* d_s2) {
  const char* who = "pk_band_factor";
  int rc = ready(c);
  if (rc) return rc;
  if (!d_hvals || !d_jvals || !d_s1 || !d_s2) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = bd_context(c, who)) || (rc = bd_plan_current(c, who))) return rc;
  PkBandFamilyArgs g = bd_planned(c);
  g.a.hvals = d_hvals; g.a.jvals = d_jvals; g.a.s1 = d_s1; g.a.s2 = d_s2;
  c->band.refining = false;      // (a refinement in progress measured the factors that go)
  if ((rc = bd_enqueue_factor(c, g, 1, true, c->stream))) return rc;
  c->band.factored = true;
  return 0;
}

int pk_band_solve_dev(pk_ctx* c, const double* d_rhs, double* d_sol) {
  const char* who = "pk_band_solve";
  int rc = ready(c);
  if (rc) return rc;
  if (!d_rhs || !d_sol) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = bd_context(c, who))) return rc;
  if (!c->band.planned || !c->band.factored) return fail(c, 134, "%s: no factorisation (pk_band_plan, pk_band_factor_dev)", who);
  PkBandFamilyArgs g = bd_planned(c);
  if ((rc = bd_partial(c, g.a, who))) return rc;
  g.a.rhs = d_rhs; g.a.sol = d_sol;
  return bd_enqueue_solve(c, g, 1, c->stream);
}

int pk_band_solve_multi_dev(pk_ctx* c, int32_t k, const double* d_rhs, int64_t stride_rhs, double* d_sol, int64_t stride_sol) {
  const char* who = "pk_band_solve_multi";
  int rc = ready(c);
  if (rc) return rc;
  if (!d_rhs || !d_sol) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = bd_context(c, who)) || (rc = bd_rhs_count(c, k, who))) return rc;
  if (!c->band.planned || !c->band.factored) return fail(c, 134, "%s: no factorisation (pk_band_plan, pk_band_factor_dev)", who);
  const int64_t N = (int64_t)c->n + c->m;
  if ((rc = bd_stride(c, stride_rhs, N, false, who, "the right-hand sides")) || (rc = bd_stride(c, stride_sol, N, false, who, "the solutions")))
    return rc;
  PkBandFamilyArgs g = bd_planned(c);      // (the matrix, ipiv, order, where and the record; the work slices are the block's own)
  g.k = k; g.c_rhs = stride_rhs; g.c_sol = stride_sol;
  if ((rc = bd_multi_work(c, g, who))) return rc;
  g.a.rhs = d_rhs; g.a.sol = d_sol;
  return bd_enqueue_solve(c, g, 1, c->stream);
}

int pk_band_record(pk_ctx* c, double* rec) {
  const char* who = "pk_band_record";
  int rc = ready(c);
  if (rc) return rc;
  if (!rec) return fail(c, 60, "null host buffer");
  if (!c->band.planned || !c->band.factored) return fail(c, 134, "%s: no factorisation (pk_band_plan, pk_band_factor_dev)", who);
  const PkBandArgs a = bd_planned(c).a;
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipMemcpyAsync(rec, a.rec, sizeof(double) * PK_BD_REC, hipMemcpyDeviceToHost, c->stream));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int pk_solve_banded(pk_ctx* c, const double* s1, const double* s2, const double* b, double* x, double* rec) {
  const char* who = "pk_solve_banded";
  int rc = host_ready(c, s1 && s2 && b && x && rec);
  if (rc || (rc = solve_ops_ready(c, true, true, who))) return rc;
  return bd_host_form(c, who, 1, c->band.d_scratch, c->band.scratch_cap, "host-form scratch", s1, s2, b, x, rec,
                      [&](const double* d_b, double* d_x) { return pk_band_solve_dev(c, d_b, d_x); });
}

int pk_solve_banded_multi(pk_ctx* c, int32_t k, const double* s1, const double* s2, const double* b, double* x, double* rec) {
  const char* who = "pk_solve_banded_multi";
  int rc = host_ready(c, s1 && s2 && b && x && rec);
  if (rc || (rc = solve_ops_ready(c, true, true, who)) || (rc = bd_rhs_count(c, k, who))) return rc;
  const int64_t N = (int64_t)c->n + c->m;
  return bd_host_form(c, who, (size_t)k, c->band.d_mscratch, c->band.mscratch_cap, "host-form scratch of the block", s1, s2, b, x, rec,
                      [&](const double* d_b, double* d_x) { return pk_band_solve_multi_dev(c, k, d_b, N, d_x, N); });
}

int pk_band_factor_batch_dev(pk_ctx* c, int32_t B, const double* d_hvals, int64_t stride_h, const double* d_jvals, int64_t stride_j,
                             const double* d_s1, int64_t stride_s1, const double* d_s2, int64_t stride_s2) {
  const char* who = "pk_band_factor_batch";
  int rc = ready(c);
  if (rc) return rc;
  if (!d_hvals || !d_jvals || !d_s1 || !d_s2) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = bd_context(c, who)) || (rc = bd_batch_size(c, B, who)) || (rc = bd_plan_current(c, who))) return rc;
  if ((rc = bd_stride(c, stride_h, c->csr[1].n_unique, true, who, "the Hessian's values")) ||
      (rc = bd_stride(c, stride_j, c->csr[0].n_unique, true, who, "the Jacobian's values")) ||
      (rc = bd_stride(c, stride_s1, c->n, true, who, "s1")) || (rc = bd_stride(c, stride_s2, c->m, true, who, "s2")))
    return rc;
  PkBand& b = c->band;
  if ((rc = bd_batch_reserve(c, b.d_bwork, b.bwork_cap, bd_entry_doubles(b.nb, b.w, b.p) + PK_BD_REC, B, true, who,
                             "the bands, the borders and the right-hand sides")) ||
      (rc = bd_batch_reserve(c, b.d_bipiv, b.bipiv_cap, bd_ipiv_doubles(b.nb), B, true, who, "the interchanges")))
    return rc;
  PkBandFamilyArgs g = bd_planned_batch(c, B);
  g.a.hvals = d_hvals; g.a.jvals = d_jvals; g.a.s1 = d_s1; g.a.s2 = d_s2;
  g.s_h = stride_h; g.s_j = stride_j; g.s_s1 = stride_s1; g.s_s2 = stride_s2;
  b.batch = 0;      // (the factors of an earlier batch are overwritten from here on)
  if ((rc = bd_enqueue_factor(c, g, B, true, c->stream))) return rc;
  b.batch = B;
  return 0;
}

int pk_band_solve_batch_dev(pk_ctx* c, int32_t B, const double* d_rhs, int64_t stride_rhs, double* d_sol, int64_t stride_sol) {
  const char* who = "pk_band_solve_batch";
  int rc = ready(c);
  if (rc) return rc;
  if (!d_rhs || !d_sol) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = bd_context(c, who)) || (rc = bd_batch_size(c, B, who))) return rc;
  if (!c->band.planned || c->band.batch != B)
    return fail(c, 134, "%s: no batch factorisation of %d entries (pk_band_plan, pk_band_factor_batch_dev; the last one had %d)", who, B,
                (int)c->band.batch);
  const int64_t N = (int64_t)c->n + c->m;
  if ((rc = bd_stride(c, stride_rhs, N, true, who, "the right-hand sides")) || (rc = bd_stride(c, stride_sol, N, false, who, "the solutions")))
    return rc;
  PkBandFamilyArgs g = bd_planned_batch(c, B);
  if ((rc = bd_partial_batch(c, g, B, who))) return rc;
  g.a.rhs = d_rhs; g.a.sol = d_sol;
  g.s_rhs = stride_rhs; g.s_sol = stride_sol;
  return bd_enqueue_solve(c, g, B, c->stream);
}

int pk_band_record_batch(pk_ctx* c, int32_t B, double* rec) {
  const char* who = "pk_band_record_batch";
  int rc = ready(c);
  if (rc) return rc;
  if (!rec) return fail(c, 60, "null host buffer");
  if ((rc = bd_batch_size(c, B, who))) return rc;
  if (!c->band.planned || c->band.batch != B)
    return fail(c, 134, "%s: no batch factorisation of %d entries (pk_band_plan, pk_band_factor_batch_dev; the last one had %d)", who, B,
                (int)c->band.batch);
  const PkBandFamilyArgs g = bd_planned_batch(c, B);
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipMemcpyAsync(rec, g.a.rec, sizeof(double) * PK_BD_REC * (size_t)B, hipMemcpyDeviceToHost, c->stream));      // (the records are one array)
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int pk_solve_banded_batch(pk_ctx* c, int32_t B, const double* s1, const double* s2, const double* b, double* x, double* rec) {
  const char* who = "pk_solve_banded_batch";
  const double *jvals = nullptr, *hvals = nullptr;
  int rc = host_ready(c, s1 && s2 && b && x && rec);
  if (rc || (rc = solve_ops_ready(c, true, true, who))) return rc;
  if ((rc = bd_context(c, who)) || (rc = bd_batch_size(c, B, who))) return rc;
  if (!c->band.planned) return fail(c, 134, "%s: no plan (pk_band_plan)", who);
  if ((rc = solve_linearized(c, true, jvals, hvals, who))) return rc;
  const size_t n = (size_t)c->n, m = (size_t)c->m, N = n + m, nB = (size_t)B;
  if ((rc = lib_reserve(c, c->band.d_bscratch, c->band.bscratch_cap, 3 * N * nB + 1, 136, who, "host-form scratch of the batch"))) return rc;
  double *d_b = c->band.d_bscratch, *d_s1 = d_b + N * nB, *d_s2 = d_s1 + n * nB, *d_x = d_s2 + m * nB;
  PK_HIP(c, hipSetDevice(c->device));
  if ((rc = lib_upload(c, d_b, b, N * nB)) || (rc = lib_upload(c, d_s1, s1, n * nB)) || (rc = lib_upload(c, d_s2, s2, m * nB))) return rc;
  // (an array of length 0 has nothing to tell apart: its stride is 0)
  if ((rc = pk_band_factor_batch_dev(c, B, hvals, 0, jvals, 0, d_s1, (int64_t)n, d_s2, (int64_t)m)) ||
      (rc = pk_band_solve_batch_dev(c, B, d_b, (int64_t)N, d_x, (int64_t)N)))
    return rc;
  std::vector<double> got(N * nB + 1);
  if (N) PK_HIP(c, hipMemcpyAsync(got.data(), d_x, sizeof(double) * N * nB, hipMemcpyDeviceToHost, c->stream));
  if ((rc = pk_band_record_batch(c, B, rec))) return rc;      // (synchronises)
  for (size_t e = 0; e < nB; ++e)
    if (rec[PK_BD_REC * e + BD_STATUS] == 0.0) std::copy(got.begin() + (long)(N * e), got.begin() + (long)(N * (e + 1)), x + N * e);
  return 0;
}

int pk_band_fill_dev(pk_ctx* c, const double* d_hvals, const double* d_jvals, const double* d_s1, const double* d_s2, double* d_out) {
  const char* who = "pk_band_fill";
  int rc = ready(c);
  if (rc) return rc;
  if (!d_hvals || !d_jvals || !d_s1 || !d_s2 || !d_out) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = bd_context(c, who)) || (rc = bd_plan_current(c, who))) return rc;
  PkBandFamilyArgs g = bd_planned(c);
  g.a.hvals = d_hvals; g.a.jvals = d_jvals; g.a.s1 = d_s1; g.a.s2 = d_s2;
  g.a.band = d_out;      // (band, U and C are one array: the caller's)
  if (g.a.dests > 0) PK_LIB_LAUNCH_Y(c, pk_bd_fill_k, bd_fill_host, lib_grid(lib_elem_items(g.a.dests)), 1, c->stream, g);
  return 0;
}

int pk_band_raw_dev(pk_ctx* c, int64_t nb, int32_t w, int32_t p, int32_t R, double* d_band, const double* d_U, const double* d_C,
                    const double* d_rhs, int32_t* d_ipiv, double* d_x, double* d_rec) {
  const char* who = "pk_band_raw";
  int rc = ready(c);
  if (rc) return rc;
  if (!d_band || !d_rhs || !d_ipiv || !d_x || !d_rec || (p > 0 && (!d_U || !d_C))) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = bd_shape(c, nb, w, p, who))) return rc;
  if (R != p + 1) return fail(c, 134, "%s: R = %d right-hand sides for a border of %d (p + 1: the border's columns and b)", who, R, p);
  PkBandFamilyArgs g = bd_raw(nb, w, p, d_band, d_U, d_C, d_rhs, d_ipiv, d_x, d_rec);
  if ((rc = lib_reserve(c, c->band.d_raw, c->band.raw_cap, bd_solve_doubles(nb, p), 136, who, "the right-hand sides")) || (rc = bd_partial(c, g.a, who)))
    return rc;
  bd_solve_slices(g.a, 1, c->band.d_raw);
  if ((rc = bd_enqueue_factor(c, g, 1, false, c->stream))) return rc;
  return bd_enqueue_solve(c, g, 1, c->stream);
}

int pk_band_raw_multi_dev(pk_ctx* c, int64_t nb, int32_t w, int32_t p, int32_t k, double* d_band, const double* d_U, const double* d_C,
                          const double* d_rhs, int64_t stride_rhs, int32_t* d_ipiv, double* d_x, int64_t stride_x, double* d_rec) {
  const char* who = "pk_band_raw_multi";
  int rc = ready(c);
  if (rc) return rc;
  if (!d_band || !d_rhs || !d_ipiv || !d_x || !d_rec || (p > 0 && (!d_U || !d_C))) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = bd_shape(c, nb, w, p, who)) || (rc = bd_rhs_count(c, k, who))) return rc;
  if ((rc = bd_stride(c, stride_rhs, nb + p, false, who, "the right-hand sides")) || (rc = bd_stride(c, stride_x, nb + p, false, who, "the solutions")))
    return rc;
  PkBandFamilyArgs g = bd_raw(nb, w, p, d_band, d_U, d_C, d_rhs, d_ipiv, d_x, d_rec);
  g.k = k; g.c_rhs = stride_rhs; g.c_sol = stride_x;
  if ((rc = bd_multi_work(c, g, who))) return rc;
  if ((rc = bd_enqueue_factor(c, g, 1, false, c->stream))) return rc;
  return bd_enqueue_solve(c, g, 1, c->stream);
}

int pk_band_raw_batch_dev(pk_ctx* c, int32_t B, int64_t nb, int32_t w, int32_t p, int32_t R, double* d_band, int64_t stride_band,
                          const double* d_U, int64_t stride_U, const double* d_C, int64_t stride_C, const double* d_rhs, int64_t stride_rhs,
                          int32_t* d_ipiv, int64_t stride_ipiv, double* d_x, int64_t stride_x, double* d_rec, int64_t stride_rec) {
  const char* who = "pk_band_raw_batch";
  int rc = ready(c);
  if (rc) return rc;
  if (!d_band || !d_rhs || !d_ipiv || !d_x || !d_rec || (p > 0 && (!d_U || !d_C))) return fail(c, 110, "%s: null device pointer", who);
  if ((rc = bd_batch_size(c, B, who)) || (rc = bd_shape(c, nb, w, p, who))) return rc;
  if (R != p + 1) return fail(c, 134, "%s: R = %d right-hand sides for a border of %d (p + 1: the border's columns and b)", who, R, p);
  if ((rc = bd_stride(c, stride_band, bd_ldab(w) * nb, false, who, "the bands")) || (rc = bd_stride(c, stride_U, nb * p, true, who, "U")) ||
      (rc = bd_stride(c, stride_C, (int64_t)p * p, true, who, "C")) || (rc = bd_stride(c, stride_rhs, nb + p, true, who, "the right-hand sides")) ||
      (rc = bd_stride(c, stride_ipiv, nb, false, who, "the interchanges")) || (rc = bd_stride(c, stride_x, nb + p, false, who, "the solutions")) ||
      (rc = bd_stride(c, stride_rec, PK_BD_REC, false, who, "the records")))
    return rc;
  PkBandFamilyArgs g = bd_raw(nb, w, p, d_band, d_U, d_C, d_rhs, d_ipiv, d_x, d_rec);
  g.s_band = stride_band; g.s_U = d_U ? stride_U : 0; g.s_C = d_C ? stride_C : 0; g.s_rhs = stride_rhs;
  g.s_ipiv = stride_ipiv; g.s_sol = stride_x; g.s_rec = stride_rec;
  g.s_work = (int64_t)bd_solve_doubles(nb, p);
  if ((rc = bd_batch_reserve(c, c->band.d_braw, c->band.braw_cap, (size_t)g.s_work, B, false, who, "the right-hand sides")) ||
      (rc = bd_partial_batch(c, g, B, who)))
    return rc;
  bd_solve_slices(g.a, 1, c->band.d_braw);
  if ((rc = bd_enqueue_factor(c, g, B, false, c->stream))) return rc;
  return bd_enqueue_solve(c, g, B, c->stream);
}

}  // extern "C"
