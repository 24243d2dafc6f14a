// pk_runtime.h -- private to the translation units of the host runtime (libpockit_hip.so):
//
//   pk_runtime.cpp  core: context, model, problem, the launch machinery, device-pointer and one-shot host evaluation, cycle
//   pk_shim.cpp     host shim: prepared-x protocol, landing blocks, copy batching, polling waits, its A/B options
//   pk_pool.cpp     helper threads of the host's passes over x and lambda (no HIP, no pk_ctx: includes pk_error.h only)
//   pk_shard.cpp    sharding: shard flags, peer / IPC / registered memory, the exchange of the partial sums, run copies
//   pk_batch.cpp    a batch of iterates in one launch of the fused cycle (pk_cycleb): batched object, per-entry workspaces
//   pk_extras.cpp   CSR hand-off, mesh error estimation, profiling and developer tracing
//   pk_ops.cpp      J, J^T and the symmetric H applied to vectors and blocks of vectors on the device (pk_op_rows, pk_op_long,
//                   pk_op_rows_k, pk_op_long_k: the library's own kernels)
//   pk_reduce.cpp   row norms and weighted diagonals of J, J^T and H over the same row blocks, the diagonal of H (pk_red_rows,
//                   pk_red_long, pk_diag: the library's own kernels)
//   pk_merit.cpp    merit terms of a batch of trial points reduced on the device (pk_trial, pk_merit, pk_merit_fin: the library's
//                   own kernels), the bounds they are measured against, the scratch of the host forms
//   pk_cg.cpp       the condensed KKT matrix and the normal equations applied and solved by preconditioned CG on the device
//                   (pk_cg_init, pk_cg_dot, pk_cg_update, pk_cg_scalar, pk_cg_elem: the library's own kernels)
//   pk_minres.cpp   the augmented (indefinite) KKT system applied and solved by preconditioned MINRES on the device
//                   (pk_mr_init, pk_mr_dot, pk_mr_update, pk_mr_scalar, pk_mr_elem: the library's own kernels)
//   pk_ipm.cpp      barrier terms, dual residual and the step to the boundary of a boxed vector, around that solve (pk_ip_terms_k,
//                   pk_ip_resid_k, pk_ip_step_k, pk_ip_scalar_k: the library's own kernels)
//   pk_slack.cpp    the slacks of a resident iterate: their elimination, their step with the curvature terms, the update with the
//                   multiplier safeguard, the merit terms of trial points with slacks (pk_sl_reduce_k, pk_sl_recover_k,
//                   pk_sl_update_k, pk_sl_merit_k, pk_sl_scalar_k: the library's own kernels)
//   pk_band.cpp     the step's system assembled, factored and solved on the device: a band LU with partial pivoting inside the
//                   band, bordered by the few dense unknowns (pk_bd_init_k, pk_bd_fill_k, pk_bd_panel_k, pk_bd_update_k,
//                   pk_bd_prep_k, pk_bd_solve_k, pk_bd_dot_k, pk_bd_border_k, pk_bd_xb_k, pk_bd_scatter_k: the library's own kernels, one
//                   family for a single system, a batch of entries and a block of right-hand sides)
//   pk_band_refine.cpp  a solution of that solve measured against the true K (the CSR values) and refined with the factors in
//                   place, the stop decided on the device (pk_bd_resid_k, pk_bd_refine_scalar_k, pk_bd_correct_k: the library's
//                   own kernels)
//   pk_solve.cpp    the host scaffolding of a device-resident solve, shared by pk_cg.cpp and pk_minres.cpp: the context's growing
//                   arrays (lib_reserve, also pk_merit.cpp's, pk_ipm.cpp's, pk_slack.cpp's and pk_band.cpp's), the common checks, the skeletons of record / advance / the host loop
//   pk_error.cpp    fail(): where an error message is kept
//
// pk_libkernel.h, on top of this header, is what pk_ops.cpp, pk_reduce.cpp, pk_merit.cpp, pk_cg.cpp, pk_minres.cpp, pk_ipm.cpp, pk_slack.cpp and pk_band.cpp share
// beyond it: the scaffolding of kernels that are compiled into the library (function macro, tree driver, grid rule, host walk,
// launch) and the pieced dot of the two solvers (piece size, tree step, partial store, scalar trip, their host stand-ins).
//
// Holds what they share: pk_ctx (one member per area, each with ONE reset function in the unit that owns it), PK_HIP, and the
// few helpers that cross a unit boundary.  The helpers of the per-callback path are either defined in
// pk_shim.cpp, beside the callbacks, or inline here.
#ifndef PK_RUNTIME_H
#define PK_RUNTIME_H

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pockit_hip.h"
#include "pockit_hip_internal.h"
#include "pk_error.h"
#define PK_MAX_PHASES 128     // (= PK_HOST_MAX_PHASES: the host-side PkArgs holds the most a code object may ask for)
#include "pk_abi.h"
#include "pk_launch.h"        // kernel ids and names; grid and LDS bytes of every launch

enum { F_WRITE_F = 1, F_SECONDARY = 2, F_FIN_INT = 8, F_FIN_GRAD = 16, F_SPLIT = 32, F_XCHG = 64, F_NO_HESS = 128,
       F_COMPACT_H = 256, F_COMPACT_J = 512 };

struct EventPair {
  hipEvent_t a, b;
};

// ---- sharding (pk_shard.cpp): pk_set_shard, pk_set_shared_grad_target
struct PkShard {
  int flags = 0;                 // OR-ed into PkArgs.flags (bit 1: secondary shard)
  bool external_prepass = false; // sharded mode: the caller all-reduces the integrals itself
  double* ext_I = nullptr;       // caller-owned integral buffer (sharded mode)
  double* gshared = nullptr;     // pk_set_shared_grad_target: where the shared gradient slots go (NULL: the gradient itself)
};

// ---- pk_set_exchange (pk_shard.cpp): peer-mapped mailboxes of the partial-sum exchange (pk_xchg)
struct PkExchange {
  const unsigned long long* const* box = nullptr;
  const int32_t* idx = nullptr;
  int32_t world = 0, rank = 0, nsh = 0, stride = 0;
  unsigned long long* own = nullptr;   // this rank's own mailbox (host copy of the pointer: state block, pk_exchange_status)
  bool in_launch = false;       // pk_cycle's finalize workgroup exchanges the partial sums itself (pk_set_exchange_inline)
};

// ---- cached hipGraph of the fused callback cycle (pk_set_cycle_graph; pk_runtime.cpp: drop_cycle_graph)
struct PkCycleKey {
  const void *x, *lam, *f, *grad, *g, *jac, *hess;
  double sigma;
  hipStream_t st;
  bool operator==(const PkCycleKey& o) const {
    return x == o.x && lam == o.lam && f == o.f && grad == o.grad && g == o.g && jac == o.jac && hess == o.hess &&
           sigma == o.sigma && st == o.st;
  }
};
struct PkGraph {
  bool use = false;
  hipGraphExec_t cyc_exec = nullptr;
  hipGraphExec_t rep_exec = nullptr;      // pk_eval_cycle_dev_repeat: a batch of rep_count cycles as one graph
  int rep_count = 0;
  PkCycleKey cyc_key{}, rep_key{};
};

// ---- a batch of iterates per launch (pk_batch.cpp: pk_load_batch_model, pk_set_batch, pk_eval_cycle_batch_dev; free_batch)
// Everything a launch of pk_cycleb writes beside the caller's outputs exists once per batch entry: nothing is shared between
// the entries of a launch but the read-only tables and the status words.
struct PkBatch {
  hipModule_t module = nullptr;          // the batched code object (its only kernel: pk_cycleb = pk_ctx.fn[K_CYCLEB])
  int B = 0, cap = 0;                    // entries armed by pk_set_batch; entries the workspaces were allocated for
  double* d_ws = nullptr;                // per entry [integrals | partial | partial2 | auxiliary buffer], ws_stride doubles
  unsigned long long* d_cp = nullptr;    // per entry [cpart | cpart2] hand-off slots (PK_EMPTY between launches)
  double* d_big = nullptr;               // per entry the staging rows of intervals with more than 256 points
  char* d_args = nullptr;                // the PkArgs records of the entries: what pk_cycleb's fifth argument points to
  size_t ws_stride = 0, n_partial = 0, big_stride = 0;
  char* h_args = nullptr;                // pinned: the records as filled on the host, copied to d_args ahead of every launch
  hipEvent_t ev_copied = nullptr;        // ... recorded behind that copy: the next batch waits for it before it refills h_args
  bool copy_pending = false;
  int64_t launches = 0;                  // launches of pk_cycleb by this context (pk_batch_launches): the loop of single cycles adds none
};

// ---- profiling and developer tracing (pk_extras.cpp: free_trace; the timed launch itself is launch_raw's)
struct PkProfile {
  bool on = false;
  unsigned mask = 0;
  unsigned period = 1;          // time every n-th launch of a selected kernel
  unsigned seen[K_COUNT] = {};
  std::vector<EventPair> pending[K_COUNT];
  std::vector<EventPair> free_events;
  int64_t launches[K_COUNT] = {};
  double total_ms[K_COUNT] = {};
  unsigned long long* d_trace = nullptr;   // developer tracing buffer, [n_tiles][16]
};

// ---- triplet -> CSR map (pk_set_csr_map; pk_extras.cpp: free_csr)
struct PkCsrMap {
  int32_t *d_seg = nullptr, *d_perm = nullptr;
  double* d_vals = nullptr;
  int64_t n_unique = 0, n_triplets = 0;
};

// ---- operators over the CSR values (pk_set_csr_operator; pk_ops.cpp: free_operators)
// A work item of one workgroup of pk_op_rows.  n_rows >= 0: a stream block, the whole rows [row0, row0 + n_rows) = the entries
// [e0, e0 + count); n_rows = -1: a piece block, count consecutive entries of a long row, row0 = its slot in the partial sums.
struct PkOpBlock {
  int32_t e0, count, row0, n_rows;
};
enum { PK_OP_KMAX = 8 };      // columns of a block product one workgroup handles: a wider block goes in chunks of launches
struct PkOpLong {      // a row with more than PK_BLOCK entries: its partial sums are the slots [first, first + pieces)
  int32_t row, first, pieces;
};
struct PkOperator {
  int32_t *d_indptr = nullptr, *d_indices = nullptr, *d_src = nullptr;   // d_src NULL: entry e takes vals[e]
  PkOpBlock* d_blocks = nullptr;
  PkOpLong* d_longs = nullptr;
  double* d_partial = nullptr;
  double* d_partial_k = nullptr;      // the block product's partial sums, n_slots x PK_OP_KMAX: allocated on its first use
  int32_t n_rows = 0, n_cols = 0, n_blocks = 0, n_longs = 0;             // n_blocks = 0: not set
  int32_t n_slots = 0;
  int64_t nnz = 0;
};
struct PkOps {
  PkOperator op[3];                          // 0 J, 1 J^T, 2 H symmetric
  double *d_v = nullptr, *d_y = nullptr;     // scratch of pk_apply_operator[_block], max(n, m) * scratch_k doubles each
  int64_t scratch_k = 0;                     // columns they hold (1 from pk_set_csr_operator; pk_apply_operator_block grows them)
  const double *lin_J = nullptr, *lin_H = nullptr;   // the linearization of pk_linearize: CSR value arrays of the maps (NULL: none)
  int32_t* d_diag_pos = nullptr;             // pk_set_operator_diagonal: per row of H its diagonal entry in the Hessian map's CSR
                                             // values, -1 where there is none (n entries; NULL: not set; pk_reduce.cpp)
};

// ---- merit terms of a batch of trial points (pk_merit.cpp: pk_set_bounds, pk_merit_batch_dev, pk_merit_scan ...; free_merit)
struct PkMerit {
  double* d_bounds = nullptr;       // pk_set_bounds: [c_lb (m) | c_ub (m) | v_lb (n) | v_ub (n)], NULL: not set
  double* d_partial = nullptr;      // the pieces' partial rows of pk_merit, 8 doubles each: grows when needed, never shrinks
  size_t partial_cap = 0;           // ... in doubles
  double* d_scratch = nullptr;      // the host forms' [x | d | X | f | grad | g | J | out] for one chunk of entries: likewise
  size_t scratch_cap = 0;
};

// ---- what a device-resident iterative solve keeps in the context, whichever the method (pk_solve.cpp; solve_free, solve_forget)
// Allocated on first use; every array grows when needed and never shrinks short of pk_set_problem.
struct PkSolveState {
  double* d_work = nullptr;         // the method's work vectors, slices of one length
  size_t work_cap = 0;
  double* d_partial = nullptr;      // the pieces' partial sums, planes x n_pieces doubles (pk_libkernel.h)
  size_t partial_cap = 0;
  double* d_rec = nullptr;          // the method's record
  size_t rec_cap = 0;
  double* d_scratch = nullptr;      // the host forms' copies of the caller's arrays, slices of the same length
  size_t scratch_cap = 0;
  bool active = false;              // a solve is in progress (begin): forgotten by pk_set_csr_operator and pk_set_csr_map
  hipStream_t stream = nullptr;     // where the last begin / advance was enqueued: the record is copied behind it
};

// ---- CG on the condensed KKT matrix / the normal equations (pk_cg.cpp: pk_cg_begin_dev, pk_solve_condensed ...)
// work [r | z | p | q | t] and scratch [b | x0 | x | d | s | minv | v] of max(n, m) doubles each, 3 planes, a record of 8 doubles
struct PkCg : PkSolveState {
  int form = 0;                     // the solve in progress: the caller's arrays
  const double *jvals = nullptr, *hvals = nullptr, *d = nullptr, *s = nullptr, *minv = nullptr;
  double* x = nullptr;
};

// ---- MINRES on the augmented KKT system (pk_minres.cpp: pk_minres_begin_dev, pk_solve_kkt ...)
// work [r1 | r2 | y | v | w | w2 | q] and scratch [b | x0 | x | s1 s2 | minv | v] of n + m doubles each, 2 planes, a record of 16
struct PkMinres : PkSolveState {
  const double *jvals = nullptr, *hvals = nullptr, *s1 = nullptr, *s2 = nullptr, *minv = nullptr;
  double* x = nullptr;
};

// ---- barrier terms, dual residual and boundary step of a boxed vector (pk_ipm.cpp: pk_ip_terms_dev ...; free_ipm)
// Allocated on first use; both arrays grow when needed and never shrink short of pk_set_problem.
struct PkIpm {
  double* d_partial = nullptr;      // the pieces' partial columns, 8 planes x n_pieces doubles (pk_libkernel.h)
  size_t partial_cap = 0;
  double* d_scratch = nullptr;      // the host forms' six slices of max(n, m) doubles and the record of 8 behind them
  size_t scratch_cap = 0;
};

// ---- slack elimination, slack step, iterate update and merit terms with slacks (pk_slack.cpp: pk_slack_reduce_dev ...; free_slack)
// Allocated on first use; both arrays grow when needed and never shrink short of pk_set_problem.
struct PkSlack {
  double* d_partial = nullptr;      // the pieces' partial columns, planes x n_pieces doubles per entry of a batch (pk_libkernel.h)
  size_t partial_cap = 0;
  double* d_scratch = nullptr;      // the host forms' nine slices of max(n, m) doubles and the record of 8 behind them
  size_t scratch_cap = 0;
};

// ---- the bordered band LU of the step's system (pk_band.cpp: pk_band_plan, pk_band_factor_dev, pk_band_solve_dev ...; free_band)
// The plan's arrays are replaced by the next plan; the others grow when needed and never shrink short of pk_set_problem.
struct PkBand {
  int32_t *d_map = nullptr, *d_order = nullptr, *d_where = nullptr;   // pk_band_plan: two source codes per stored slot, the caller's
                                                                      // index of a permuted position, and its inverse (n + m)
  double* d_work = nullptr;         // [band | U | C | Y | x | b_C | record] of the planned system
  double* d_ipiv = nullptr;         // the interchanges (Nb 32-bit integers)
  double* d_partial = nullptr;      // the pieces' partial sums of the border's dots, (p + 1) p planes x n_pieces doubles
  size_t partial_cap = 0;
  double* d_scratch = nullptr;      // the host form's [b | s1 s2 | x]
  size_t scratch_cap = 0;
  double* d_raw = nullptr;          // pk_band_raw_dev's [Y | x | b_C | record]
  size_t raw_cap = 0;
  int64_t nb = 0, w = 0, p = 0;
  int64_t sources = 0;              // entries of [hvals | jvals | s1 | s2] the plan was checked against
  bool planned = false, factored = false;
  // the batch forms (pk_band_factor_batch_dev ...): B systems behind the one plan, reserved by the first batch call, grown by a
  // larger B, released with the plan
  double* d_bwork = nullptr;        // B x [band | U | C | Y | x | b_C], then the B records of 8
  size_t bwork_cap = 0;
  double* d_bipiv = nullptr;        // B x the interchanges
  size_t bipiv_cap = 0;
  double* d_bpartial = nullptr;     // B x the partial sums of the border's dots
  size_t bpartial_cap = 0;
  double* d_bscratch = nullptr;     // the host batch form's [b | s1 | s2 | x], B of each
  size_t bscratch_cap = 0;
  double* d_braw = nullptr;         // pk_band_raw_batch_dev's B x [Y | x | b_C]
  size_t braw_cap = 0;
  int32_t batch = 0;                // the entries of the last batch factorisation (0: none)
  // the block solve (pk_band_solve_multi_dev ...): k right-hand sides against one factorisation, reserved by the first call,
  // grown by a larger k, released with the plan
  double* d_mwork = nullptr;        // [Y: p + k sweep vectors of Nb | x: k slices of Nb + p | b_C: k slices of p]
  size_t mwork_cap = 0;
  double* d_mpartial = nullptr;     // the partial sums of the (p + k) p dots
  size_t mpartial_cap = 0;
  double* d_mscratch = nullptr;     // the host block form's [b (k rows) | s1 s2 | x (k rows)]
  size_t mscratch_cap = 0;
  // the refinement (pk_band_refine.cpp: pk_band_refine_begin_dev ...): reserved by the first begin, kept across plans, released
  // with the band's state
  double* d_refine = nullptr;       // [r | d | q] of n + m doubles each, the 4 planes of partials, the record of 8
  size_t refine_cap = 0;
  double* d_rpartial = nullptr;     // pk_band_refine_step_dev's partials (its other arrays are the caller's)
  size_t rpartial_cap = 0;
  bool refining = false;            // between a begin and the next plan or factorisation
  int32_t refine_t = 0;             // steps enqueued since the begin
  const double *rf_hvals = nullptr, *rf_jvals = nullptr, *rf_s1 = nullptr, *rf_s2 = nullptr, *rf_rhs = nullptr;   // the caller's arrays
  double* rf_sol = nullptr;
  double rf_tol = 0.0;
  int32_t rf_min_steps = 0;
};

// ---- mesh error estimation (pk_set_mesh_error_tables; pk_extras.cpp: free_mesh_error)
struct PkMeshError {
  void* d_iv = nullptr;
  int32_t* d_grp = nullptr;     // (first record, count) per wavefront of pk_err
  double *d_db = nullptr, *d_T = nullptr, *d_I = nullptr;
  int32_t n_groups = 0;
  int64_t n_out = 0;
  double* d_stage = nullptr;    // staging rows of intervals with more than 264 augmented nodes
  int32_t row = 0, slot = 0;
};

// ---- host shim (pk_shim.cpp: alloc_shim, free_shim)
// one result of the current iterate: 0 f, 1 grad f, 2 g, 3 J, 4 H
struct PkResult {
  double* h_out = nullptr;       // the context's own pinned landing place
  double* target = nullptr;      // pk_set_result_targets (NULL: h_out)
  bool target_visible = true;    // the device can store into target itself
  bool target_pinned = false;    // target is pinned memory by contract (landing blocks)
  double* landed = nullptr;      // where the result of the current iterate went
  hipEvent_t ev_out = nullptr;
  bool enq = false;              // copy of the result is enqueued
  bool done = false;             // ... and known to have landed
  bool stored_direct = false;    // the kernel stored the result into its landing place
  int ev_of = 0;                 // the event that covers the result (one event per batch of copies); default: its own, see PkShim()
};

struct PkShim {
  PkShim() { for (int k = 0; k < 5; ++k) res[k].ev_of = k; }
  double* h_Hc = nullptr;      // pinned landing place of the compact Hessian (pk_eval_hessc_prepared), allocated on first use
  // pinned host staging: x and lambda are double-buffered (the upload of iterate k + 1 does not wait for anything of
  // iterate k), results land in res[k].h_out (f, grad, g, J, H) or in caller-supplied pinned targets
  double *h_xs[2] = {nullptr, nullptr}, *h_lams[2] = {nullptr, nullptr};
  hipEvent_t ev_xs[2] = {nullptr, nullptr}, ev_lams[2] = {nullptr, nullptr};   // upload k of the buffer has left it
  int xbuf = 0, lambuf = 0;
  double* h_x = nullptr;                   // the staging buffer holding the x of the last pk_prepare_x (pk_same_x)
  bool x_valid = false;
  bool lam_staged = false;                 // pk_stage_lambda ran, pk_eval_hess_prepared has not consumed it yet
  PkResult res[5];
  unsigned long long status_seen[2] = {0, 0};   // PkArgs.status as of the last check (handoff_check)
  int poll_limit = 0;                           // > 0: poll rounds before a hand-off gives up ("poll_limit" host option; tests)
  int prefetch = 1;            // 1: every x-only result is copied out right behind the kernel; 0: on first request
  int adaptive_prefetch = 1;   // ... but grad f and J only while the solver keeps asking for them: an iterate whose Jacobian was
                               // never asked for was a rejected trial point of a line search (f and g only), and the copy of
                               // its J (122 us of link time at 12k nodes) stood in the way of the next trial point's upload;
                               // the new x behind such an iterate gets grad f / J on request
  bool cur_J_asked = true;     // grad f or J of the prepared iterate has been asked for
  int host_direct = 0;         // 1: the kernels store into the (pinned, device-visible) host targets themselves
  // Host-shim tuning (pk_set_host_option; defaults = what measured fastest on MI355X, tools/dma_probe.cpp):
  int spin_wait = 1;           // results are awaited by polling (the event's state / f's own pinned word), not hipEventSynchronize
  int lambda_direct = 1;       // the Hessian kernel of the prepared protocol reads the multipliers from the pinned staging
                               // buffer itself (one pass over PCIe inside the kernel) instead of an upload in front of it;
                               // applied up to 2 MB of multipliers (12k nodes: -8 us; at 3.2 MB the chunk-pipelined upload
                               // wins by 16 us: the staging memcpy then overlaps the link)
  int chunk_upload = 1;        // staging of large inputs is pipelined with their upload in a few chunks
  int kernel_upload = 1;       // x (and lambda) go up through a copy kernel on the compute queue instead of the DMA engine: the
                               // kernel behind it then starts without a cross-engine hand-off (~10 us on the path to f)
  int kernel_download = 8;     // results of up to this many MiB per piece come down through a copy kernel instead of the DMA
                               // engine (0: never): no cross-engine hand-off behind the kernel that produced them (~10 us per
                               // copy), but 51 instead of 56 GB/s on the link -- the DMA engine wins from ~5 MB on
  int split_copy = 1;          // grad f | g leave in a copy of their own in front of J (+1 DMA), with an event behind it: the
                               // gradient and constraints callbacks return while J is still on the link, and the bitwise
                               // compares of x they and the Jacobian callback start with are hidden behind that copy
  int small_direct = 1;        // small systems are bound by the number of launches, not by bytes: a kernel reads an x of at most
                               // 128 KB from its pinned staging buffer (no upload launch) and stores x-results of at most 1 MB
                               // straight into their pinned landing places (no copy launches) -- LQR 10x10: 53 -> us per iterate
  int small_x_kb = 128;            // (the x threshold of small_direct, in KB: an A/B knob)
  const double* x_src = nullptr;   // where the kernels read the prepared x: d_x, or (small_direct) the pinned staging buffer
  int hess_direct = 1;         // the Hessian kernel stores into the pinned landing place itself when H is small enough for the
                               // copy kernel (kernel_download): no launch behind it, its reads of lambda and its stores share
                               // the link in both directions (12k nodes: 97 -> 93 us; at 83 MB the copy is faster)
  int speculative_hess = 1;    // pk_callback_hess launches on the prepared x BEFORE comparing x with it (the compare then runs
                               // while the GPU works; a different x -- rare -- discards the launch and starts over)
  // reuse guard of the staging buffers without events: every enqueue takes a sequence number; an idle stream seen by the host
  // (wait_result) retires all numbers issued so far
  uint64_t op_seq = 0, idle_seq = 0;
  // mark_wait: behind the last result copy of a batch a one-word kernel stores a counter into pinned memory (res[0].h_out[4])
  // and the waiting callback polls that word instead of the stream's state (the runtime's query answers several microseconds
  // after the word is there; the stream is still asked now and then, so a failed launch does not hang the caller)
  int mark_wait = 1;
  unsigned long long mark_val = 0;     // value of the last mark enqueued
  uint64_t mark_op_seq = 0;            // op_seq when it was enqueued: everything up to it has finished once the mark is seen
  bool mark_pending = false;           // the last thing enqueued for the results is a mark nobody has waited for yet
  uint64_t xs_seq[2] = {0, 0}, lams_seq[2] = {0, 0};
  hipEvent_t ev_early = nullptr;     // behind the grad f | g copy of the current iterate (split_copy)
  bool early_valid = false;
  const double* lam_src = nullptr;   // where the staged multipliers are read from (d_lam, or the pinned staging buffer)
  // Pieces [start, stop) of the Jacobian values that CHANGE with x.  Default: everything.  pk_set_jac_constant_runs takes
  // x-independent runs (the +-1 translation entries of phasebase.py:1071-1081 are 19 % of J at 12k nodes) out of the
  // per-iterate copy: they are put into a landing array once (pk_fill_jac_constants) and never cross PCIe again.
  std::vector<std::pair<int64_t, int64_t>> jruns, jconst;      // (of the layout the shim serves; the other layout's are parked)
  std::vector<std::pair<int64_t, int64_t>> jruns_other, jconst_other;
  bool jac_compact = false;    // the host shim's Jacobian callback serves the compact layout (pk_set_jacobian_layout)
  bool target_filled = false;  // the caller's J landing array (res[3].target) already holds the constant runs (pk_callback_x blocks)
  bool jac_filled = false;     // ... and so does the landing place of the CURRENT iterate: its copy skips them
};

struct pk_ctx : pk_error_state {
  // ---- core (pk_runtime.cpp: free_problem)
  int device = 0;
  hipStream_t stream = nullptr;
  hipModule_t module = nullptr;
  hipFunction_t fn[K_COUNT] = {};
  bool have_model = false, have_problem = false;
  bool split_xall = false;      // pk_xall with two waves per tile (values / Jacobian), see pk_set_problem
  int cycle_mode = 1;           // 1: single-launch pk_cycle; 0: pk_xall + pk_hess (pk_set_cycle_mode)
  int cycle_layout = 0;         // what pk_eval_cycle_dev writes: bit 0 compact Jacobian, bit 1 compact Hessian (pk_set_cycle_layout)
  // (two switches of pk_set_host_option that choose among the core's launches)
  int xpart_single = 1;        // pk_eval_xpart_dev as ONE launch (pk_cycle without its Hessian role) instead of pk_xall + pk_fin
  bool separate_x = false;     // the five callbacks one after the other through the STAND-ALONE kernels (pk_int + pk_fin, pk_grad, pk_g,
                               // pk_jac, pk_hess), as for a model that needs the integrals first: what pockit_amd.Evaluator.checked falls back
                               // to when a code object's fused kernel fails its self-check (round 5)
  bool has_big = false;         // the mesh has intervals with more than 64 points (one workgroup each, PK_BIG code objects)
  // staging rows of intervals with more than 256 points (they do not fit the workgroup's LDS rows): slots in device memory
  double* d_big_stage = nullptr;
  int32_t big_row = 0, big_slot = 0;
  size_t big_stage_doubles = 0; // size of d_big_stage (pk_set_batch gives every batch entry a slice of its own)
  unsigned long long *d_cpart = nullptr, *d_cpart2 = nullptr;   // pk_cycle's hand-off slots (PK_EMPTY between launches)
  size_t cpart_slots = 0;
  int debug_flags = 0;          // diagnostic kernel switches (POCKIT_AMD_DEBUG_FLAGS), never set in production
  pk_model_desc md{};
  // problem
  int32_t n = 0, m = 0, n_sys = 0, n_s = 0, l_s = 0, n_phase = 0, n_tiles = 0;
  int64_t nnz_J = 0, nnz_H = 0;
  int32_t n_items_jac = 0, n_items_hess = 0, n_items_aux = 0, n_outer = 0, n_aux = 0, gz_off = 0, n_gz = 0;
  int32_t n_items_hessc = 0, n_items_jacc = 0;
  int64_t nnz_Hc = 0, nnz_Jc = 0;
  void* d_items_jacc = nullptr;
  double* d_Jc = nullptr;
  void *d_phases = nullptr, *d_tiles = nullptr, *d_kinds = nullptr, *d_items_jac = nullptr, *d_items_hess = nullptr,
       *d_items_aux = nullptr, *d_outer = nullptr, *d_items_hessc = nullptr;
  double *d_aux = nullptr, *d_Hc = nullptr;
  int32_t* d_ib = nullptr;
  double* d_db = nullptr;
  int64_t* d_lb = nullptr;
  // work buffers
  double *d_x = nullptr, *d_lam = nullptr, *d_f = nullptr, *d_grad = nullptr, *d_g = nullptr, *d_J = nullptr,
         *d_H = nullptr, *d_I = nullptr, *d_partial = nullptr, *d_partial2 = nullptr;
  std::vector<PkPhase> h_phases;
  std::vector<int32_t> jac_row, jac_col, hess_row, hess_col;
  // ---- the other areas
  PkShard shard;
  PkExchange exchange;
  PkGraph graph;
  PkBatch batch;
  PkProfile profile;
  PkCsrMap csr[4];   // [0] Jacobian, [1] Hessian of the Lagrangian (lower triangle)
                     // + [2]: compact Hessian values -> the same CSR entries (a pure permutation: one value per entry)
                     // + [3]: compact Jacobian values -> the CSR entries of J (the few repeated positions summed)
  PkOps ops;
  PkMerit merit;
  PkCg cg;
  PkMinres minres;
  PkMeshError mesh_error;
  PkShim shim;
  PkIpm ipm;         // (last: the members the cycle's host path reads keep the offsets they had)
  PkSlack slack;     // (behind it, for the same reason)
  PkBand band;       // (and behind that)
};

#pragma GCC visibility push(hidden)      // (no function declared here leaves the library: its exports are the two C headers')

#define PK_HIP(c, call)                                                                                  \
  do {                                                                                                   \
    hipError_t e_ = (call);                                                                              \
    if (e_ != hipSuccess) return fail((c), 100 + (int)e_, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// ---- small helpers, inline in every unit
template <class T>
inline void release(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

inline int upload(pk_ctx* c, void** dst, const void* src, size_t bytes) {
  *dst = nullptr;
  const size_t alloc = bytes ? bytes : 8;
  PK_HIP(c, hipMalloc(dst, alloc));
  if (bytes) PK_HIP(c, hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return 0;
}

inline int ready(pk_ctx* c) {
  if (!c) return fail(nullptr, 1, "null context");
  if (!c->have_model) return fail(c, 2, "no model loaded (pk_load_model)");
  if (!c->have_problem) return fail(c, 3, "no problem set (pk_set_problem)");
  return 0;
}

inline hipStream_t pick(pk_ctx* c, void* stream) { return stream ? (hipStream_t)stream : c->stream; }

// bytes of PkArgs the loaded code object declares: the head and as many phase records as it was compiled for
inline size_t args_bytes(const pk_ctx* c) {
  return offsetof(PkArgs, ph) + sizeof(PkPhase) * (size_t)(c->md.max_phases > 0 ? c->md.max_phases : 8);
}

// ---- pk_runtime.cpp: the launch machinery
void drop_cycle_graph(pk_ctx* c);
PkArgs base_args(pk_ctx* c, const double* d_x, const double* d_lam, double sigma);
// pk_launch_shape with the facts of the context's problem (n_flat: entries of pk_csr / chunks of pk_runs; layout: pk_cyclec's)
PkLaunchShape shape_of(const pk_ctx* c, int k, int64_t n_flat = 0, int layout = 0);
int launch_raw(pk_ctx* c, int k, void* args, size_t sz, const PkLaunchShape& shape, hipStream_t st);
int launch(pk_ctx* c, int k, PkArgs& A, hipStream_t st, int64_t n_flat = 0);
int prepass(pk_ctx* c, const double* d_x, const double* d_lam, double sigma, double* d_f, bool write_f, hipStream_t st);
// the PkArgs of one single-launch cycle (flags, items of the layout, exchange): what pk_cycle / pk_cyclec take by value and
// pk_cycleb reads from the record of a batch entry
PkArgs cycle_args(pk_ctx* c, const double* d_x, const double* d_lam, double sigma, double* d_f, double* d_grad, double* d_g,
                  double* d_jac, double* d_hess, int layout);
int enqueue_single_launch_cycle(pk_ctx* c, const double* d_x, const double* d_lam, double sigma, double* d_f,
                                double* d_grad, double* d_g, double* d_jac, double* d_hess, hipStream_t st, int layout = -1);
bool xpart_is_one_launch(const pk_ctx* c);

// ---- pk_shim.cpp: the per-callback path lives there; the core's one-shot host evaluation borrows these
int alloc_shim(pk_ctx* c);      // pk_set_problem: staging buffers, landing places, events
void free_shim(pk_ctx* c);
int copy_async(pk_ctx* c, double* dst, const double* src, size_t n, hipMemcpyKind kind, bool by_kernel);
int stage_upload(pk_ctx* c, double* const bufs[2], hipEvent_t const evs[2], uint64_t seqs[2], int& cur, const double* src,
                 double* dst, size_t count, double** staged);
int handoff_check(pk_ctx* c);
int launch_store_word(pk_ctx* c, unsigned long long* dst, unsigned long long value, hipStream_t st);   // pk_store_word_kernel

// ---- pk_batch.cpp
void free_batch(pk_ctx* c);         // the per-entry workspaces (with the problem)
void unload_batch_model(pk_ctx* c); // the batched code object (with the model)

// ---- pk_extras.cpp
void free_csr(pk_ctx* c);
void free_mesh_error(pk_ctx* c);
void free_trace(pk_ctx* c);

// ---- pk_ops.cpp
void free_operators(pk_ctx* c);      // with the problem, and with every pk_set_csr_map: an operator's src refers to a map
void drop_linearization(pk_ctx* c);  // the CSR value arrays of the maps are about to hold something else
// The rows of a CSR structure (indptr validated: monotone from 0) cut in order into the work items of pk_op_rows: stream blocks
// of whole rows (empty ones included) with at most PK_BLOCK entries and PK_BLOCK rows, ceil(len / PK_BLOCK) piece blocks for a
// row with more than PK_BLOCK entries, and the list of those long rows.  Pure; nonzero: a count does not fit 32 bits.
int pk_op_row_blocks(const int32_t* indptr, int32_t n_rows, std::vector<PkOpBlock>& blocks, std::vector<PkOpLong>& longs,
                     int32_t& n_slots);
// The entry checks the operator entry points of pk_ops.cpp and pk_reduce.cpp share (errors 110, 117; 118 and the value array
// pk_linearize left for the operator): nothing is enqueued behind a nonzero return.
int op_ready(pk_ctx* c, int op, bool pointers, const char* who);
int op_linearized(pk_ctx* c, int op, const double*& vals, const char* who);

// ---- pk_merit.cpp
void free_merit(pk_ctx* c);          // bounds, partial rows and scratch (with the problem)

// ---- pk_ipm.cpp
void free_ipm(pk_ctx* c);            // partial columns and scratch (with the problem)

// ---- pk_slack.cpp
void free_slack(pk_ctx* c);          // partial columns and scratch (with the problem)

// ---- pk_band.cpp
void free_band(pk_ctx* c);           // the plan and every array of the unit (with the problem), the refinement's too
// what pk_band_refine.cpp asks of the planned system: is there a plan the CSR maps still fit (and a factorisation)?  (134); the
// border's partial sums reserved ahead of a solve (136); K sol = rhs with the factors in place, in the launches of
// pk_band_solve_dev on the context's stream; the device address of the factorisation's record
int band_planned_ready(pk_ctx* c, bool factored, const char* who);
int band_planned_partial(pk_ctx* c, const char* who);
int band_planned_solve(pk_ctx* c, const double* d_rhs, double* d_sol, const char* who);
const double* band_planned_record(pk_ctx* c);

// ---- pk_solve.cpp: the host scaffolding of a device-resident solve, shared by pk_cg.cpp and pk_minres.cpp (no kernels)
// An array of the context that grows when needed and never shrinks: the new one first, so the error (code: 127 for the merit
// terms, 136 for the solves) enqueues nothing and leaves what was there.  And the upload of an optional host array (src NULL:
// nothing) on the context's stream.
int lib_reserve(pk_ctx* c, double*& p, size_t& cap, size_t want, int code, const char* who, const char* what);
int lib_upload(pk_ctx* c, double* dst, const double* src, size_t count);
int solve_state(pk_ctx* c, PkSolveState& s, size_t work, size_t rec, const char* who);           // work vectors and record, on first use
int solve_partial(pk_ctx* c, PkSolveState& s, int planes, int64_t len, const char* who);         // partial sums of `planes` dots of len
inline bool solve_tol_ok(double tol) { return tol >= 0.0 && __builtin_isfinite(tol); }
// what every entry point that applies K checks before anything is enqueued: no sharded context (119); J, J^T [, H] ready
int solve_ops_ready(pk_ctx* c, bool with_h, bool pointers, const char* who);
// the values pk_linearize left, for the host forms (118)
int solve_linearized(pk_ctx* c, bool with_h, const double*& jvals, const double*& hvals, const char* who);
// a host form's checks behind that, in this order: its parameters (134), the values pk_linearize left (118), the positions of
// H's diagonal for the preconditioner built on the device (132)
int solve_host_checks(pk_ctx* c, bool with_h, double tol, int maxiter, int check_every, int precond, const double*& jvals,
                      const double*& hvals, const char* who);
// The skeletons of the entry points behind ready(c) (theirs: the state is a member of the context it vouches for).  who names
// the entry point in the messages, begin the one that starts a solve.  record: 60, 135, the copy behind the solve's stream,
// synchronised.  advance: 134, 135, the stream, `iters` times the method's iteration.
int solve_record(pk_ctx* c, const PkSolveState& s, double* rec, size_t count, const char* who, const char* begin);
int solve_advance(pk_ctx* c, PkSolveState& s, int iters, void* stream, int (*iteration)(pk_ctx*, hipStream_t), const char* who,
                  const char* begin);
// The tail of a host form behind its begin: the record, then chunks of check_every iterations and the record again until the
// status (slot 0) leaves 0 or maxiter is reached -- status 4 then, in the host copy only -- and the download of x.
int solve_host_loop(pk_ctx* c, int maxiter, int check_every, int (*advance)(pk_ctx*, int, void*), int (*record)(pk_ctx*, double*),
                    double* rec, double* x, const double* d_x, size_t count);

// an array cut into the slices [0, L), [L, 2 L) ...: one per double* member of Slices, in their order
template <class Slices, size_t... K>
inline Slices lib_slices_of(double* w, size_t L, std::index_sequence<K...>) { return Slices{(w + K * L)...}; }
template <class Slices>
inline Slices lib_slices(double* w, size_t L) { return lib_slices_of<Slices>(w, L, std::make_index_sequence<sizeof(Slices) / sizeof(double*)>{}); }
// the host forms' scratch: one slice of L doubles per member of Slices
template <class Slices>
inline int solve_scratch(pk_ctx* c, PkSolveState& s, size_t L, Slices& out, const char* who) {
  if (const int rc = lib_reserve(c, s.d_scratch, s.scratch_cap, sizeof(Slices) / sizeof(double*) * L, 136, who, "host-form scratch")) return rc;
  out = lib_slices<Slices>(s.d_scratch, L);
  return 0;
}
// with the problem: the arrays go, the state is a fresh one
template <class Solver>
inline void solve_free(Solver& s) {
  release(s.d_work); release(s.d_partial); release(s.d_rec); release(s.d_scratch);
  s = Solver{};
}
// the operators or a map are about to change: a solve in progress and the caller's pointers it holds are forgotten, the arrays stay
template <class Solver>
inline void solve_forget(Solver& s) {
  PkSolveState arrays = s;
  arrays.active = false;
  s = Solver{};
  static_cast<PkSolveState&>(s) = arrays;
}

// ---- the host-buffer form of an entry point: upload x (and lambda), the device-pointer entry point, download, synchronize
inline int host_ready(pk_ctx* c, bool buffers) {
  const int rc = ready(c);
  return rc ? rc : buffers ? 0 : fail(c, 60, "null host buffer");
}
struct Download { double* host; const double* dev; size_t count; };

// lambda == NULL: x alone goes up.  staged: the inputs go through the double-buffered pinned staging buffers of the host shim
// (pk_eval_cycle) instead of a copy from the caller's arrays.  handoff: errors 97 of the fused cycle are reported.
template <class Eval>
int host_eval(pk_ctx* c, const double* x, const double* lambda, std::initializer_list<Download> results, bool handoff, Eval eval,
              bool staged = false) {
  int rc;
  PK_HIP(c, hipSetDevice(c->device));
  c->shim.x_valid = false;      // the context's x and result buffers now hold another evaluation
  if (staged) {
    if ((rc = stage_upload(c, c->shim.h_xs, c->shim.ev_xs, c->shim.xs_seq, c->shim.xbuf, x, c->d_x, (size_t)c->n, nullptr))) return rc;
    if ((rc = stage_upload(c, c->shim.h_lams, c->shim.ev_lams, c->shim.lams_seq, c->shim.lambuf, lambda, c->d_lam, (size_t)c->m, nullptr))) return rc;
  } else {
    PK_HIP(c, hipMemcpyAsync(c->d_x, x, sizeof(double) * (size_t)c->n, hipMemcpyHostToDevice, c->stream));
    if (lambda) PK_HIP(c, hipMemcpyAsync(c->d_lam, lambda, sizeof(double) * (size_t)c->m, hipMemcpyHostToDevice, c->stream));
  }
  if ((rc = eval())) return rc;
  for (const Download& r : results)
    PK_HIP(c, hipMemcpyAsync(r.host, r.dev, sizeof(double) * r.count, hipMemcpyDeviceToHost, c->stream));
  PK_HIP(c, hipStreamSynchronize(c->stream));
  return handoff ? handoff_check(c) : 0;
}

#pragma GCC visibility pop
#endif  // PK_RUNTIME_H
