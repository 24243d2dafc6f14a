// pk_extras.cpp -- what sits beside the callbacks: the device-resident CSR hand-off, mesh error estimation, HIP-event profiling
// of the kernels and developer tracing.
#include "pk_runtime.h"

void free_csr(pk_ctx* c) {
  for (auto& m : c->csr) { release(m.d_seg); release(m.d_perm); release(m.d_vals); m.n_unique = m.n_triplets = 0; }
}

void free_mesh_error(pk_ctx* c) {
  release(c->mesh_error.d_iv); release(c->mesh_error.d_grp); release(c->mesh_error.d_db); release(c->mesh_error.d_T); release(c->mesh_error.d_I); release(c->mesh_error.d_stage);
  c->mesh_error.n_groups = 0; c->mesh_error.n_out = 0; c->mesh_error.row = c->mesh_error.slot = 0;
}

void free_trace(pk_ctx* c) {
  release(c->profile.d_trace);
}

extern "C" {

const char* pk_kernel_name(int k) { return (k >= 0 && k < K_COUNT) ? kKernelNames[k] : ""; }

// ---------------------------------------------------------------- device-resident CSR hand-off
int pk_set_csr_map(pk_ctx* c, int which, const int32_t* seg, const int32_t* perm, int64_t n_unique, int64_t n_triplets) {
  int rc = ready(c);
  if (rc) return rc;
  if (which < 0 || which > 3)
    return fail(c, 80, "pk_set_csr_map: which must be 0 (Jacobian), 1 (Hessian), 2 (compact Hessian) or 3 (compact Jacobian)");
  const int64_t expect = which == 0 ? c->nnz_J : which == 1 ? c->nnz_H : which == 2 ? c->nnz_Hc : c->nnz_Jc;
  if (!perm || n_unique <= 0 || n_unique > n_triplets || n_triplets != expect || n_triplets > INT32_MAX)
    return fail(c, 81, "pk_set_csr_map: map does not match the problem (%lld triplets expected)", (long long)expect);
  // validate on the host: the kernel indexes with these
  for (int64_t q = 0; q < n_triplets; ++q)
    if (perm[q] < 0 || perm[q] >= n_triplets) return fail(c, 82, "pk_set_csr_map: perm[%lld] out of range", (long long)q);
  if (seg) {
    if (seg[0] != 0 || seg[n_unique] != n_triplets) return fail(c, 83, "pk_set_csr_map: segment table does not cover the triplets");
    for (int64_t p = 0; p < n_unique; ++p)
      if (seg[p + 1] <= seg[p]) return fail(c, 83, "pk_set_csr_map: empty or decreasing segment %lld", (long long)p);
  } else if (n_unique != n_triplets) {
    return fail(c, 83, "pk_set_csr_map: a segment table is required when entries repeat");
  }
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  free_operators(c);      // (their src refers to a map, the linearization lies in the maps' value arrays)
  auto& m = c->csr[which];
  release(m.d_seg); release(m.d_perm); release(m.d_vals);
  m.n_unique = m.n_triplets = 0;
  if (seg) {
    // repeated entries: the device gets the runs per slice of 256 consecutive CSR entries, transposed and padded to the
    // slice's longest run (see kernel_csr)
    const int64_t nblk = (n_unique + PK_BLOCK - 1) / PK_BLOCK;
    std::vector<int32_t> off((size_t)nblk + 1, 0);
    int64_t total = 0;
    for (int64_t b = 0; b < nblk; ++b) {
      int32_t width = 0;
      for (int64_t p = b * PK_BLOCK; p < n_unique && p < (b + 1) * PK_BLOCK; ++p) width = std::max(width, seg[p + 1] - seg[p]);
      off[(size_t)b] = (int32_t)total;
      total += (int64_t)width * PK_BLOCK;
      if (total > INT32_MAX) return fail(c, 85, "pk_set_csr_map: the padded run table does not fit 32-bit offsets");
    }
    off[(size_t)nblk] = (int32_t)total;
    std::vector<int32_t> sell((size_t)total, -1);
    for (int64_t p = 0; p < n_unique; ++p) {
      const int64_t b = p / PK_BLOCK, t = p % PK_BLOCK;
      for (int32_t k = 0; k < seg[p + 1] - seg[p]; ++k) sell[(size_t)(off[(size_t)b] + (int64_t)k * PK_BLOCK + t)] = perm[seg[p] + k];
    }
    if ((rc = upload(c, (void**)&m.d_seg, off.data(), sizeof(int32_t) * off.size()))) return rc;
    if ((rc = upload(c, (void**)&m.d_perm, sell.data(), sizeof(int32_t) * sell.size()))) return rc;
  } else if ((rc = upload(c, (void**)&m.d_perm, perm, sizeof(int32_t) * (size_t)n_triplets))) {
    return rc;
  }
  PK_HIP(c, hipMalloc((void**)&m.d_vals, sizeof(double) * (size_t)n_unique));
  m.n_unique = n_unique;
  m.n_triplets = n_triplets;
  return 0;
}

int pk_gather_csr_dev(pk_ctx* c, int which, const double* d_triplets, double* d_csr, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (which < 0 || which > 3 || c->csr[which].n_unique == 0) return fail(c, 84, "pk_gather_csr: call pk_set_csr_map first");
  const auto& m = c->csr[which];
  PkArgs A = base_args(c, nullptr, nullptr, 0.0);
  A.csr_in = d_triplets; A.csr_seg = m.d_seg; A.csr_perm = m.d_perm; A.csr_out = d_csr; A.n_csr = (int32_t)m.n_unique;
  return launch(c, K_CSR, A, pick(c, stream), m.n_unique);
}

int pk_eval_jac_csr_dev(pk_ctx* c, const double* d_x, double* d_csr, void* stream) {
  if (c) c->shim.x_valid = false;      // (the triplets pass through the context's J buffer)
  if (c && c->have_problem && c->csr[3].n_unique > 0 && c->nnz_Jc > 0) {      // from the compact evaluation, like the Hessian's
    int rc = pk_eval_jacc_dev(c, d_x, c->d_Jc, stream);
    return rc ? rc : pk_gather_csr_dev(c, 3, c->d_Jc, d_csr, stream);
  }
  int rc = pk_eval_jac_dev(c, d_x, c ? c->d_J : nullptr, stream);
  return rc ? rc : pk_gather_csr_dev(c, 0, c->d_J, d_csr, stream);
}

// The CSR values of the Hessian come from the COMPACT evaluation when its map is set (which = 2): pk_hessc writes one value
// per distinct (row, col) -- the multipliers contracted with the integration block first -- and the gather is a pure
// permutation of nnz_Hc values; the route through the reference layout writes every repeated triplet (6.6 per entry at the
// humanoid's size) and adds them up again (40k nodes: 17 + 52 us vs 8 + 6 us).
int pk_eval_hess_csr_dev(pk_ctx* c, const double* d_x, const double* d_lam, double sigma, double* d_csr, void* stream) {
  if (c && c->have_problem && c->csr[2].n_unique > 0 && c->nnz_Hc > 0) {
    int rc = pk_eval_hessc_dev(c, d_x, d_lam, sigma, c->d_Hc, stream);
    return rc ? rc : pk_gather_csr_dev(c, 2, c->d_Hc, d_csr, stream);
  }
  int rc = pk_eval_hess_dev(c, d_x, d_lam, sigma, c ? c->d_H : nullptr, stream);
  return rc ? rc : pk_gather_csr_dev(c, 1, c->d_H, d_csr, stream);
}

int pk_eval_jac_csr(pk_ctx* c, const double* x, double* vals) {
  if (const int rc = host_ready(c, x && vals)) return rc;
  const PkCsrMap& m = c->csr[c->csr[3].n_unique > 0 ? 3 : 0];      // (both maps fill the same CSR entries)
  if (m.n_unique == 0) return fail(c, 84, "pk_eval_jac_csr: call pk_set_csr_map first");
  drop_linearization(c);      // (m.d_vals is where pk_linearize leaves J)
  return host_eval(c, x, nullptr, {{vals, m.d_vals, (size_t)m.n_unique}}, false,
                   [&] { return pk_eval_jac_csr_dev(c, c->d_x, m.d_vals, nullptr); });
}

int pk_eval_hess_csr(pk_ctx* c, const double* x, const double* lambda, double sigma, double* vals) {
  if (const int rc = host_ready(c, x && lambda && vals)) return rc;
  const PkCsrMap& m = c->csr[c->csr[2].n_unique > 0 ? 2 : 1];      // (both maps fill the same CSR entries)
  if (m.n_unique == 0) return fail(c, 84, "pk_eval_hess_csr: call pk_set_csr_map first");
  drop_linearization(c);
  return host_eval(c, x, lambda, {{vals, m.d_vals, (size_t)m.n_unique}}, false,
                   [&] { return pk_eval_hess_csr_dev(c, c->d_x, c->d_lam, sigma, m.d_vals, nullptr); });
}

// ---------------------------------------------------------------- mesh error estimation
int pk_set_mesh_error_tables(pk_ctx* c, const void* intervals, int32_t n_intervals, const int32_t* groups,
                             int32_t n_groups, const double* tables, int64_t n_tables, int64_t n_out) {
  int rc = ready(c);
  if (rc) return rc;
  if (!intervals || n_intervals <= 0 || !groups || n_groups <= 0 || !tables || n_tables <= 0 || n_out <= 0)
    return fail(c, 70, "pk_set_mesh_error_tables: empty tables");
  if (n_groups % PK_WAVES_PER_BLOCK)
    return fail(c, 71, "pk_set_mesh_error_tables: wave groups must be padded to a multiple of %d per phase", PK_WAVES_PER_BLOCK);
  if (shape_of(c, K_ERR).lds_bytes > PK_LDS_LIMIT)
    return fail(c, 72, "pk_set_mesh_error_tables: model needs more than 160 KiB of LDS per workgroup");
  // host-side validation of everything the kernel indexes with (a faulting kernel can take the node down)
  const PkErrIv* iv = (const PkErrIv*)intervals;
  for (int32_t g = 0; g < n_intervals; ++g) {
    const PkErrIv& r = iv[g];
    if (r.phase < 0 || r.phase >= c->n_phase) return fail(c, 73, "pk_set_mesh_error_tables: record %d: bad phase", g);
    const PkPhase& ph = c->h_phases[r.phase];
    const int na = r.K + 1, ncx = r.K + 1 - ph.scheme, nr = ncx;
    const int64_t tab = (int64_t)na * ncx + (int64_t)na * r.K + (int64_t)nr * ncx + (int64_t)nr * na;
    if (r.K < 1 || r.lm < 0 || r.lm + ncx > ph.state_len || r.lm + r.K > ph.L_m || r.tab_off < 0 ||
        r.tab_off + tab > n_tables || r.tau_off < 0 || r.tau_off + na > n_tables || r.row0 < 0 || r.row0 + nr > r.rows ||
        r.out_off < 0 || r.out_off + (int64_t)ph.n_x * r.rows > n_out)
      return fail(c, 74, "pk_set_mesh_error_tables: record %d is inconsistent with the problem", g);
  }
  for (int32_t g = 0; g < n_groups; ++g) {     // a wave's intervals: in range, one phase, one K, K + 1 lanes each
    const int32_t first = groups[2 * g], cnt = groups[2 * g + 1];
    if (first < 0 || first >= n_intervals)
      return fail(c, 76, "pk_set_mesh_error_tables: wave group %d is out of range", g);
    if (cnt == 1 && iv[first].K + 1 > PK_WAVE) {     // K + 1 > 64: a workgroup of its own (first group of the block, count 1;
      if (g % PK_WAVES_PER_BLOCK)                    //  the block's other groups carry count -1)
        return fail(c, 76, "pk_set_mesh_error_tables: wave group %d: an interval with K + 1 > %d must start a block", g, PK_WAVE);
      for (int32_t u = 1; u < PK_WAVES_PER_BLOCK; ++u)
        if (groups[2 * (g + u) + 1] != -1)
          return fail(c, 76, "pk_set_mesh_error_tables: wave group %d shares its block with a workgroup-wide interval", g + u);
      g += PK_WAVES_PER_BLOCK - 1;
      continue;
    }
    if (cnt < 0 || first + cnt > n_intervals || cnt * (iv[first].K + 1) > PK_WAVE)
      return fail(c, 76, "pk_set_mesh_error_tables: wave group %d is out of range", g);
    for (int32_t j = 1; j < cnt; ++j)
      if (iv[first + j].K != iv[first].K || iv[first + j].phase != iv[first].phase)
        return fail(c, 76, "pk_set_mesh_error_tables: wave group %d mixes phases or orders", g);
  }
  PK_HIP(c, hipSetDevice(c->device));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  free_mesh_error(c);
  {   // intervals whose K + 1 augmented nodes do not fit the LDS rows of 264 doubles: slots of a staging buffer
    std::vector<PkErrIv> ivs(iv, iv + n_intervals);
    int32_t n_stage = 0, namax = 0;
    for (PkErrIv& r : ivs) {
      r.stage = 0;
      if (r.K + 1 > 264) {
        r.stage = n_stage++;
        if (r.K + 1 > namax) namax = r.K + 1;
      }
    }
    if (n_stage) {
      c->mesh_error.row = (namax + 7) & ~7;
      const size_t slot = ((size_t)c->md.lds_e / PK_WAVE) * (size_t)c->mesh_error.row;
      if (slot > (size_t)INT32_MAX) return fail(c, 72, "pk_set_mesh_error_tables: an interval with %d points is too long for the staging buffer", namax - 1);
      c->mesh_error.slot = (int32_t)slot;
      PK_HIP(c, hipMalloc((void**)&c->mesh_error.d_stage, sizeof(double) * slot * (size_t)n_stage));
    }
    if ((rc = upload(c, &c->mesh_error.d_iv, ivs.data(), sizeof(PkErrIv) * ivs.size()))) return rc;
  }
  if ((rc = upload(c, (void**)&c->mesh_error.d_grp, groups, sizeof(int32_t) * 2 * (size_t)n_groups))) return rc;
  if ((rc = upload(c, (void**)&c->mesh_error.d_db, tables, sizeof(double) * (size_t)n_tables))) return rc;
  PK_HIP(c, hipMalloc((void**)&c->mesh_error.d_T, sizeof(double) * (size_t)n_out));
  PK_HIP(c, hipMalloc((void**)&c->mesh_error.d_I, sizeof(double) * (size_t)n_out));
  PK_HIP(c, hipMemset(c->mesh_error.d_T, 0, sizeof(double) * (size_t)n_out));
  PK_HIP(c, hipMemset(c->mesh_error.d_I, 0, sizeof(double) * (size_t)n_out));
  c->mesh_error.n_groups = n_groups;
  c->mesh_error.n_out = n_out;
  return 0;
}

int pk_eval_mesh_error_dev(pk_ctx* c, const double* d_x, double* d_T, double* d_I, void* stream) {
  int rc = ready(c);
  if (rc) return rc;
  if (c->mesh_error.n_groups <= 0) return fail(c, 75, "pk_eval_mesh_error: call pk_set_mesh_error_tables first");
  PkArgs A = base_args(c, d_x, nullptr, 0.0);
  A.erriv = (const PkErrIv*)c->mesh_error.d_iv;
  A.errgrp = c->mesh_error.d_grp;
  A.errdb = c->mesh_error.d_db;
  A.n_erriv = c->mesh_error.n_groups;
  A.o_errT = d_T;
  A.o_errI = d_I;
  A.big_stage = c->mesh_error.d_stage; A.big_row = c->mesh_error.row; A.big_slot = c->mesh_error.slot;
  return launch(c, K_ERR, A, pick(c, stream));
}

int pk_eval_mesh_error(pk_ctx* c, const double* x, double* T, double* I) {
  const int rc = host_ready(c, x && T && I);
  return rc ? rc : host_eval(c, x, nullptr, {{T, c->mesh_error.d_T, (size_t)c->mesh_error.n_out}, {I, c->mesh_error.d_I, (size_t)c->mesh_error.n_out}}, false,
                             [&] { return pk_eval_mesh_error_dev(c, c->d_x, c->mesh_error.d_T, c->mesh_error.d_I, nullptr); });
}

// ---------------------------------------------------------------- profiling
int pk_profile(pk_ctx* c, int enable) {
  if (!c) return fail(nullptr, 1, "null context");
  c->profile.on = enable != 0;
  c->profile.mask = (unsigned)enable;   /* bit k set: time kernel id k */
  return 0;
}

// developer tracing (models generated with POCKIT_AMD_TRACE=1): per-tile s_memtime marks of the last launch
int pk_trace_read(pk_ctx* c, uint64_t* out, int64_t count) {
  int rc = ready(c);
  if (rc) return rc;
  const int64_t need = ((int64_t)c->n_tiles * 3 + 3) * 16;   // [tile][role] records + pk_cycle's three special workgroups
  PK_HIP(c, hipSetDevice(c->device));
  if (!c->profile.d_trace) {
    PK_HIP(c, hipStreamSynchronize(c->stream));
    PK_HIP(c, hipMalloc((void**)&c->profile.d_trace, sizeof(uint64_t) * (size_t)(need ? need : 1)));
    PK_HIP(c, hipMemset(c->profile.d_trace, 0, sizeof(uint64_t) * (size_t)(need ? need : 1)));
    drop_cycle_graph(c);
    return 0;          // first call only arms the buffer
  }
  if (!out || count < need) return fail(c, 72, "pk_trace_read: need room for %lld marks", (long long)need);
  PK_HIP(c, hipDeviceSynchronize());
  PK_HIP(c, hipMemcpy(out, c->profile.d_trace, sizeof(uint64_t) * (size_t)need, hipMemcpyDeviceToHost));
  PK_HIP(c, hipMemset(c->profile.d_trace, 0, sizeof(uint64_t) * (size_t)need));
  return 0;
}

int pk_profile_sampling(pk_ctx* c, int period) {
  if (!c) return fail(nullptr, 1, "null context");
  if (period < 1) return fail(c, 71, "pk_profile_sampling: period must be >= 1");
  c->profile.period = (unsigned)period;
  for (auto& v : c->profile.seen) v = 0;
  return 0;
}

int pk_profile_read(pk_ctx* c, int k, int64_t* launches, double* total_ms) {
  if (!c) return fail(nullptr, 1, "null context");
  if (k < 0 || k >= K_COUNT) return fail(c, 70, "pk_profile_read: bad kernel id %d", k);
  for (auto& ev : c->profile.pending[k]) {
    float ms = 0.f;
    PK_HIP(c, hipEventSynchronize(ev.b));
    PK_HIP(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    c->profile.total_ms[k] += ms;
    c->profile.launches[k] += 1;
    c->profile.free_events.push_back(ev);
  }
  c->profile.pending[k].clear();
  if (launches) *launches = c->profile.launches[k];
  if (total_ms) *total_ms = c->profile.total_ms[k];
  return 0;
}

}  // extern "C"
