// pk_launch.h -- the launch shape of every kernel of a generated code object: workgroups and dynamic LDS bytes per workgroup
// as a function of the model descriptor and a few facts of the problem.  This is the one place where they are written
// down: the host runtime (pk_runtime.cpp) launches with it and pk_load_model refuses a descriptor with it; the code generator's
// ModelSource.launch_lds_bytes (codegen.py) is held against it by tests/test_cabi.py, the runtime's launches by
// tests/fake_hip/launch_trace.txt.  Host-only, no HIP: the tests compile it with a plain C++ compiler.
#pragma once
#include <algorithm>

#include "../../include/pockit_hip.h"
#include "pk_abi.h"

enum { K_INT = 0, K_FIN, K_G, K_GRAD, K_JAC, K_HESS, K_XALL, K_AUX, K_OUTER, K_HESSC, K_ERR, K_CSR, K_CYCLE, K_XCHG, K_RUNS, K_JACC,
       K_CYCLEC, K_CYCLEB, K_COUNT };
static const char* const kKernelNames[K_COUNT] = {"pk_int", "pk_fin", "pk_g", "pk_grad", "pk_jac", "pk_hess", "pk_xall",
                                                  "pk_aux", "pk_outer", "pk_hessc", "pk_err", "pk_csr", "pk_cycle", "pk_xchg",
                                                  "pk_runs", "pk_jacc", "pk_cyclec", "pk_cycleb"};
// pk_cycleb lives in a code object of its own (codegen.ModelSource(plan, batched=True), pk_load_batch_model): every other
// kernel is looked up in the model's object by pk_load_model, this one never is
inline bool pk_kernel_of_batched_object(int k) { return k == K_CYCLEB; }

#define PK_LDS_LIMIT ((size_t)160 * 1024)      // LDS a workgroup may ask for on gfx950

// what a launch shape depends on beside the model descriptor (pk_runtime.cpp fills it by position: keep the order)
struct PkLaunchFacts {
  int32_t n_tiles = 0;
  bool split_xall = false;   // the x-part runs as two waves (of two workgroups) per tile: pk_xall, pk_cycle, pk_cyclec
  bool exchange = false;     // pk_cycle / pk_cyclec: the finalize workgroup exchanges the partial sums between the ranks
  int layout = 0;            // pk_cyclec: bit 0 compact Jacobian, bit 1 compact Hessian
  int32_t n_outer = 0;       // pk_outer: outer-product blocks
  int32_t n_erriv = 0;       // pk_err: wave groups
  int64_t n_flat = 0;        // pk_csr: CSR entries; pk_runs: chunks
};

// workgroups of PK_BLOCK threads, dynamic LDS per workgroup; batch: the y-extent of the grid (pk_cycleb: the batch entries, set
// by the launch -- the table knows the shape of ONE entry)
struct PkLaunchShape { unsigned grid; size_t lds_bytes; unsigned batch = 1; };

inline PkLaunchShape pk_launch_shape(int k, const pk_model_desc& md, const PkLaunchFacts& p) {
  const size_t D = sizeof(double), W = PK_WAVES_PER_BLOCK;
  const unsigned blocks = (unsigned)((p.n_tiles + PK_WAVES_PER_BLOCK - 1) / PK_WAVES_PER_BLOCK);
  // a model evaluated in groups runs the passes of a role as workgroups of their own (md.*_subs, codegen.py)
  auto subs = [](int32_t s) { return s > 0 ? (unsigned)s : 1u; };
  auto most = [](size_t a, size_t b) { return std::max(a, b); };
  // a tile kernel's LDS: one table block per wave in front of the staging area, which holds the rows of the workgroup's
  // waves or, in a boundary / system workgroup, the scalar expressions of the callback
  const size_t tab = D * W * (size_t)(2 * md.tab_cap + 2 * PK_WAVE + md.tab_cap / 2);
  auto tile = [&](int32_t rows, int32_t ne) { return D * most(W * (size_t)rows, (size_t)ne) + tab; };
  switch (k) {
    case K_INT: case K_GRAD: return {blocks, 0};
    case K_FIN: case K_XCHG: return {1u, 0};
    case K_G: return {blocks + 1, tile(md.lds_g, 0)};
    case K_JAC: return {blocks + 1, tile(md.lds_j, md.ne_j)};
    // pk_hess: edge and reduction workgroups + one workgroup per tile block (and pass)
    case K_HESS: return {blocks * subs(md.hess_subs) + 2, tile(md.lds_h, md.ne_h)};
    case K_HESSC: return {blocks * subs(md.hessc_subs) + 1, tile(md.lds_g, md.ne_hc)};      // (rows: the tile's multipliers)
    case K_JACC: return {blocks * subs(md.jacc_subs) + 1, tile(md.lds_jc, md.ne_jc)};
    case K_XALL: return {(p.split_xall ? 2u : 1u) * blocks + 1, tile(md.lds_x, md.ne_j)};
    case K_CYCLE: case K_CYCLEC: case K_CYCLEB: {      // (pk_cycleb: pk_cycle's x-grid and LDS, once per batch entry)
      // [edge J | edge H | finalize | per tile block: Jacobian, values, Hessian (x-part split) or x-part, Hessian; a model
      // evaluated in groups: the values workgroup and one per pass of the Jacobian / Hessian role (md.cycle_subs)]
      const unsigned per_block = md.cycle_subs > 0 ? (unsigned)md.cycle_subs : (p.split_xall ? 3u : 2u);
      const int layout = k == K_CYCLEC ? p.layout : 0;
      size_t lds = most(tile(md.lds_x > md.lds_h ? md.lds_x : md.lds_h, md.ne_j), tile(0, md.ne_h));
      // (the compact Jacobian role stages in the x-part's rows: lds_x >= lds_jc by construction, codegen.py)
      if (layout & 1) lds = most(lds, tile(0, md.ne_jc));
      if (layout & 2) lds = most(lds, tile(md.lds_g, md.ne_hc));
      // the finalize workgroup's exchange vectors, 2 x PK_XC_CAP doubles (pk_kernels.hip.h relies on this floor; the table
      // block alone, at least 9216 bytes, exceeds it, so it never decides)
      if (p.exchange) lds = most(lds, D * 2 * 512);
      return {blocks * per_block + 3, lds};
    }
    case K_AUX: return {blocks + 1, D * (size_t)(md.ne_a > 0 ? md.ne_a : 1)};
    case K_OUTER: return {(unsigned)std::min(p.n_outer, 4096), 0};
    // (lds_e = 64 (2 n_x + n_u) doubles per wave; a workgroup-wide interval stages rows of 264 doubles)
    case K_ERR: return {(unsigned)(p.n_erriv / PK_WAVES_PER_BLOCK), D * ((size_t)md.lds_e / PK_WAVE) * 264};
    case K_CSR: return {(unsigned)std::min<int64_t>((p.n_flat + PK_BLOCK - 1) / PK_BLOCK, 4096), 0};
    case K_RUNS: return {(unsigned)std::min<int64_t>(p.n_flat, 8192), 0};
  }
  return {0u, 0};
}
