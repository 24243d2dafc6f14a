/* pockit_hip_internal.h -- the entry points of libpockit_hip.so that are NOT part of its stable surface
 * (include/pockit_hip.h): 55 functions in four sections.  All of them are exported like the stable ones and follow the same
 * conventions (0 or an error code, pk_last_error); they serve this project's own binding (pockit_amd/runtime.py), its sharding
 * transport, its tools and tests, and change with them.  No function crossed the line in either direction when the header was
 * split: the stable header holds exactly the list of a foreign binding's needs.
 */
#ifndef POCKIT_HIP_INTERNAL_H
#define POCKIT_HIP_INTERNAL_H

#include "../../include/pockit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ================================================================================================ Host shim (20) */
/* "new x" protocol for host shims.  cyipopt calls objective / gradient / constraints / jacobian separately but on the
 * same iterate, then hessian with fresh multipliers (the five methods ipopt.py:41-53 hands over as ``problem_obj``).
 *   pk_same_x      1 if ``x`` equals the x of the last pk_prepare_x bit for bit (its results are still held)
 *   pk_prepare_x   stages x in pinned memory, uploads it, runs the fused x-kernel (every node evaluated once for f,
 *                  grad f, g, J) and queues the copies of the results into pinned host memory right behind it, in the
 *                  order a solver asks for them -- nothing waits; x and lambda staging is double-buffered
 *   pk_fetch       waits for ONE result (what: 0 f, 1 grad[n], 2 g[m], 3 jac[nnz_J]); out == NULL leaves it where it
 *                  landed (pk_result_location), otherwise it is copied on to ``out``
 *   pk_eval_hess_prepared   Hessian of the Lagrangian on the prepared x (x is not uploaded again)
 *   pk_set_result_targets   where the results of the NEXT prepare / Hessian land: pinned memory of the caller
 *                  (pk_host_alloc; a solver-side array that outlives the call), NULL = the context's own buffers
 *   pk_set_host_mode        prefetch 1 (default): all four x-results are copied out behind the kernel; 0: f and g
 *                  always, grad f and J on first request (a line search's rejected trial points never ask);
 *                  host_direct 1: the kernels store into the pinned host targets themselves (no DMA; A/B switch)
 *   pk_invalidate_x         forget the prepared x (the context's buffers were used by another entry point) */
/* the compact Hessian layout (pk_eval_hessc: one value per distinct position of a node) on the x of the last pk_prepare_x,
 * multipliers given or staged by pk_stage_lambda; vals_pinned = 1: `vals` is pk_host_alloc memory the DMA writes directly.
 * What SystemBase.hessian (systembase.py:820-835) becomes for a solver that was handed the compact structure. */
int pk_eval_hessc_prepared(pk_ctx* ctx, const double* lambda, double sigma, double* vals, int vals_pinned);
int pk_same_x(pk_ctx* ctx, const double* x);
int pk_prepare_x(pk_ctx* ctx, const double* x);
int pk_fetch(pk_ctx* ctx, int what, double* out);
int pk_eval_hess_prepared(pk_ctx* ctx, const double* lambda /* NULL: staged */, double sigma, double* vals);
/* queue the upload of the next Hessian's multipliers and return (the x check then overlaps the DMA) */
int pk_stage_lambda(pk_ctx* ctx, const double* lambda);
int pk_set_result_targets(pk_ctx* ctx, double* f, double* grad, double* g, double* jac, double* hess);
/* ONE call per callback of a host shim (what a cyipopt binding makes of the five methods it is handed, ipopt.py:41-53):
 *   pk_callback_x     what = 0 objective (systembase.py:602), 1 gradient (:646), 2 constraints (:613), 3 jacobian (:676).
 *                     If `x` is not the prepared iterate it becomes it (pk_prepare_x) and *fresh = 1; its results then land
 *                     in `block`, pinned memory of the caller's laid out like the library's own buffers,
 *                     [J (nnz_J) | grad f (n) | g (m)] (NULL: the context's buffers, pk_host_buffer) -- the pieces of J that
 *                     change with x, grad f and g leave the device in ONE copy.  Then result `what` is waited for; f_out
 *                     receives f for what = 0.  A block must stay allocated until every result of its iterate has been
 *                     fetched or the context's stream has been synchronized (pk_sync, pk_destroy): all results of a new x
 *                     are on their way into it whether or not they are asked for.
 *   pk_callback_hess  SystemBase.hessian (systembase.py:820-835): stages the multipliers, prepares a new x as above, evaluates
 *                     the Hessian of the Lagrangian into `hess` (pinned memory of the caller's or NULL = the context's
 *                     buffer; compact = 1: the compact layout of pk_eval_hessc, `hess` required) and waits for it.
 *   pk_set_jac_constant_runs   runs [start, stop) of the Jacobian values that do not depend on x (the +-1 translation entries
 *                     of phasebase.py:1071-1081 and constant boundary items: 19 % of J at 12k quadrotor nodes): the copy to the
 *                     host skips them from then on; every landing array must have been filled once with
 *   pk_fill_jac_constants      (the context's own buffer is filled by pk_set_jac_constant_runs itself).
 *   pk_set_host_option         A/B switches of the shim, one per name (default in brackets):
 *                     "spin_wait"         (1) results are awaited by polling; 0: hipEventSynchronize
 *                     "lambda_direct"     (1) the Hessian kernel reads the staged multipliers (up to 2 MB) from pinned memory
 *                                         itself; 0: they are uploaded first
 *                     "chunk_upload"      (1) inputs of 2 MB and more are staged and uploaded in a few chunks
 *                     "kernel_upload"     (1) x and lambda go up through a copy kernel; 0: the DMA engine
 *                     "kernel_download"   (8) results of up to that many MiB per copy come down through a copy kernel; 0: never
 *                     "split_copy"        (1) grad f | g leave in a copy of their own ahead of J
 *                     "speculative_hess"  (1) the Hessian is launched before x has been compared with the prepared iterate
 *                     "hess_direct"       (1) a Hessian of at most "kernel_download" MiB is stored into its pinned landing array
 *                                         by the kernel itself
 *                     "xpart_single"      (1) the x-results of a new iterate come from ONE launch, pk_cycle without its
 *                                         Hessian role
 *                     "separate_x"        (0) 1: the five callbacks and the cycle through the stand-alone kernels one after the
 *                                         other, never the fused kernel -- the fallback of a code object whose fused kernel
 *                                         fails its self-check
 *                     "small_direct"      (1) an x of <= "small_x_kb" KB is read by the kernels from its pinned staging buffer,
 *                                         x-results of <= 1 MB are stored by the kernel straight into the landing block: no
 *                                         upload / copy launches
 *                     "small_x_kb"        (128) the x threshold of small_direct in KB, an A/B knob
 *                     "adaptive_prefetch" (1) grad f and J of a new iterate are copied ahead only if they were asked for at the
 *                                         previous one -- a line search's rejected trial points ask for f and g only
 *                     "mark_wait"         (1) the callbacks wait on a word a one-thread kernel stores behind the result copies
 *                                         instead of on the stream's state
 *                     "poll_limit"        (0) > 0: poll rounds before a hand-off inside a launch gives up (error 97; tests)
 *                     -- see pk_shim.cpp (PkShim in pk_runtime.h holds the measurements behind the defaults). */
int pk_callback_x(pk_ctx* ctx, int what, const double* x, double* block, double* f_out, int* fresh);
int pk_callback_hess(pk_ctx* ctx, const double* x, const double* lambda, double sigma, double* block, double* hess,
                     int compact, int* fresh);
/* all five results of one iterate in ONE call and ONE launch, for a caller that has the multipliers together with x
 * (Evaluator.cycle; SystemBase's five callbacks evaluated at once): same staging and landing as the two callbacks above --
 * `block` = [J | grad f | g] pinned with its constant entries filled in, `hess` = nnz_H pinned values -- returns when
 * everything has landed; the iterate is then the prepared one (pk_callback_x on the same x is served from the block). */
int pk_callback_cycle(pk_ctx* ctx, const double* x, const double* lambda, double sigma, double* block, double* hess,
                      double* f_out);
int pk_set_jac_constant_runs(pk_ctx* ctx, int n_runs, const int64_t* start, const int64_t* stop);
int pk_fill_jac_constants(pk_ctx* ctx, double* jac /* nnz_J */);
int pk_set_host_option(pk_ctx* ctx, const char* name, int value);
/* layout of the Jacobian the host shim serves (pk_fetch(3), pk_callback_x(3), the J part of a landing block): 0 the reference's
 * triplets (default), 1 the compact layout of pk_eval_jacc (a landing block is then [J compact (nnz_Jc) | grad f | g]) */
int pk_set_jacobian_layout(pk_ctx* ctx, int compact);
int pk_result_location(pk_ctx* ctx, int what /* 0..4 */, double** ptr);
int pk_set_host_mode(pk_ctx* ctx, int prefetch, int host_direct);
int pk_invalidate_x(pk_ctx* ctx);
/* Pinned (page-locked) result buffers owned by the context: what = 0 f, 1 grad, 2 g, 3 jac, 4 hess.  The default
 * landing place of the results; reused by the next iterate. */
int pk_host_buffer(pk_ctx* ctx, int what, double** ptr, int64_t* count);
/* Pinned, device-visible host memory that is NOT tied to a context (result arrays handed to a solver may outlive the
 * evaluator): DMA targets at full PCIe rate.  pk_last_error(NULL) holds the message of a failure. */
int pk_host_alloc(size_t bytes, void** out);
int pk_host_free(void* p);

/* ================================================================================================ Helper threads (5) */
int pk_same_bits(const double* a, const double* b, size_t n);   /* 1 if equal bit for bit (memcmp), for host shims */
int pk_copy_bits(double* dst, const double* src, size_t n);      /* dst = src (non-overlapping), for host shims */
/* k helper threads (0 = none, the default; <= 16) that take slices of pk_same_bits / pk_copy_bits passes of 256 KB and more:
 * rank 0 of the host-landed sharded cycle stages and compares an x that is N times as long as one GPU's.
 * Process-wide; helpers spin for 1 ms after the last pass, otherwise they sleep in 20 us steps. */
int pk_host_threads(int k);
long pk_host_threads_jobs(void); /* slices of passes the helpers have executed so far (diagnostics) */
int pk_host_threads_hot(void);   /* how many of them are spinning right now (diagnostics); -1: the pool gave up -- the caller waited
                                  * more than 1 ms for a helper three times (a host whose CPUs are time slices of fewer cores) */

/* ================================================================================================ Sharding (20) */
/* Mesh-interval sharding across GPUs (one context per GPU, each holding its shard of the tiles):
 * ``secondary`` shards skip the boundary-node / system-level work (done once, on the primary);
 * with ``external_prepass`` the callbacks do not run the integral pre-pass themselves: the caller
 * runs pk_eval_integrals_dev, sums ``d_integrals`` (n_I doubles, caller-owned) across shards
 * (RCCL all-reduce) and only then calls the callbacks / pk_eval_f_from_integrals_dev. */
int pk_set_shard(pk_ctx* ctx, int secondary, int external_prepass, double* d_integrals);
int pk_eval_integrals_dev(pk_ctx* ctx, const double* d_x, void* stream);
/* models nonlinear in the integrals (outer-product Hessian blocks, easyderiv.py:323-459) as shards: pk_eval_hess_dev leaves
 * the quadrature-weighted gradient entries of the integrals of THIS shard's nodes in the auxiliary buffer (pk_aux_buffer;
 * entries of other shards' nodes stay zero); the caller sums the buffers over the ranks into a buffer of its own and the
 * primary rank forms the blocks from the sum with pk_eval_outer_dev (into the Hessian values, reference positions). */
int pk_aux_buffer(pk_ctx* ctx, double** d_ptr, int64_t* count);
int pk_eval_outer_dev(pk_ctx* ctx, const double* d_aux_sum, double* d_vals /* nnz_H */, void* stream);
int pk_eval_f_from_integrals_dev(pk_ctx* ctx, const double* d_x, double* d_f, void* stream);

/* Sharded cycles without a collective in the data path.  Every rank leaves its shard's slices of grad f / g / J / H in
 * its own HBM (pk_eval_cycle_dev on its tiles); what couples the shards is the handful of sums over all nodes -- the
 * integrals (-> f) and the gradient entries of t0 / tf / static parameters.  pk_exchange_sums_dev posts this rank's
 * partial vector into every peer's mailbox (peer-mapped fine-grained device memory: pk_device_alloc + pk_ipc_export on
 * the owner, pk_ipc_open on the peers), waits for theirs and adds them in rank order inside ONE one-workgroup launch.
 * pk_set_shared_grad_target redirects a shard's partial sums of the shared gradient slots (used when its gradient
 * output points at another GPU's buffer: the reassembly of the triplets on one GPU by direct peer stores).
 * pk_copy_runs_dev is the pack / unpack pass of the RCCL gather / all-gather forms of the reassembly (A/B). */
int pk_device_alloc(pk_ctx* ctx, size_t bytes, int finegrained, void** out);
int pk_device_free(pk_ctx* ctx, void* p);
int pk_ipc_export(pk_ctx* ctx, void* dptr, void* handle64 /* 64 bytes out */);
int pk_ipc_open(pk_ctx* ctx, const void* handle64, void** out);
int pk_ipc_close(pk_ctx* ctx, void* p);
int pk_set_shared_grad_target(pk_ctx* ctx, double* d_grad_shared);
/* Host-landed sharded cycle (every GPU lands its slices in ONE host array over its own PCIe link): a host
 * region several processes map (shared memory) is page-locked and made device-visible in every process
 * (pk_host_register), the ranks' run-copy kernels (pk_copy_runs_dev) store their owned runs straight into it;
 * pk_copy_dev is an asynchronous copy between any two device-visible addresses. */
int pk_host_register(pk_ctx* ctx, void* p, size_t bytes, void** dev_ptr);
int pk_host_unregister(pk_ctx* ctx, void* p);
int pk_copy_dev(pk_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);
int pk_set_exchange(pk_ctx* ctx, int world, int rank, const void* d_boxes, const int32_t* d_idx, int n_sh, int stride);
/* pk_set_exchange: every rank's mailbox holds 2 * world * stride words + 16 state words (zeroed here on this rank: the caller
 * puts a barrier between the set-up and the first cycle).  pk_exchange_status: cycles exchanged so far and how many of them
 * timed out waiting for a peer (then this rank's sums read NaN). */
int pk_exchange_status(pk_ctx* ctx, void* stream, int64_t* cycles, int64_t* timed_out);
int pk_exchange_sums_dev(pk_ctx* ctx, const double* d_x, double* d_grad, double* d_f, int epoch /* <= 0: counted on the device */,
                         int write_f, void* stream);
/* 1: the finalize workgroup of pk_eval_cycle_dev's launch exchanges the partial sums itself -- a sharded cycle is ONE
 * launch per GPU; 0 (default): pk_exchange_sums_dev is a launch of its own behind it. */
int pk_set_exchange_inline(pk_ctx* ctx, int enable);
int pk_copy_runs_dev(pk_ctx* ctx, const int64_t* d_table, int n_chunks, const double* d_src, double* d_dst, void* stream);
/* a progress mark: *d_dst = value once everything enqueued before it on the stream has finished (d_dst: device address of an
 * 8-byte aligned word, e.g. inside a segment registered with pk_host_register -- the host-landed sharded cycle lets rank 0
 * poll such words instead of waiting for the other processes to notice that their GPU has finished) */
int pk_store_word_dev(pk_ctx* ctx, void* d_dst, int64_t value, void* stream);

/* ================================================================================================ Tuning and diagnostics (12) */
/* `count` back-to-back cycles on the same buffers, enqueued by the library (a solver written against the C ABI launches from
 * compiled code; bench.py's timed batches go through this so that no interpreter loop paces the stream).  xchg = 1: every
 * cycle is followed by pk_exchange_sums_dev(d_x, d_xgrad, d_f) -- the two-launch form of a sharded cycle.  No reference
 * counterpart (the reference's callbacks are synchronous NumPy calls, systembase.py:602-835). */
int pk_eval_cycle_dev_repeat(pk_ctx* ctx, const double* d_x, const double* d_lambda, double sigma, double* d_f, double* d_grad,
                             double* d_g, double* d_jac, double* d_hess, void* stream, int count, int xchg, double* d_xgrad);
/* Replay the fused cycle from a cached hipGraph while its pointers, sigma and stream do not change (a solver's
 * steady state); any change re-captures.  Off by default. */
int pk_set_cycle_graph(pk_ctx* ctx, int enable);
/* single_launch = 1 (default): pk_cycle; 0: the two-launch form, pk_xall then pk_hess, which also reduces */
int pk_set_cycle_mode(pk_ctx* ctx, int single_launch);
int pk_wait_idle(pk_ctx* ctx, void* stream);   /* the same by polling the stream (returns a few microseconds earlier) */

/* HIP-event timing of the individual kernels on the launch stream.
 * kernel ids: 0 pk_int, 1 pk_fin, 2 pk_g, 3 pk_grad, 4 pk_jac, 5 pk_hess, 6 pk_xall, 7 pk_aux, 8 pk_outer,
 * 9 pk_hessc, 10 pk_err, 11 pk_csr, 12 pk_cycle, 13 pk_xchg, 14 pk_runs, 15 pk_jacc.  pk_profile_sampling(n): only every n-th launch of a selected kernel is timed (a timed
 * launch costs ~2-3 us more than a plain one, so timing every launch slows the loop being measured). */
int pk_profile(pk_ctx* ctx, int kernel_mask /* bit k: time kernel k; 0 = off */);
int pk_profile_sampling(pk_ctx* ctx, int period);
/* Developer tracing: with a model generated under POCKIT_AMD_TRACE=1 the waves of pk_cycle / pk_xall store the
 * constant-rate device clock (s_memrealtime) at up to 16 checkpoints of their record.  The first call arms the
 * buffer; later calls copy the [3 n_tiles + 3][16] marks out (records: [tile][values, Jacobian, Hessian wave], then
 * pk_cycle's boundary-J, boundary-H and finalize workgroups) and clear the buffer. */
int pk_trace_read(pk_ctx* ctx, uint64_t* out, int64_t count);
int pk_profile_read(pk_ctx* ctx, int kernel_id, int64_t* launches, double* total_ms);
const char* pk_kernel_name(int kernel_id);
/* launches of pk_cycleb by this context so far (counted with or without profiling): a batch served by the loop of single
 * cycles adds none, a batch served by the kernel adds exactly one */
int pk_batch_launches(pk_ctx* ctx, int64_t* launches);
/* pk_merit_batch_dev's reduction with EXPLICIT lengths and device bound pointers (the public form calls it with the context's
 * n, m and uploaded bounds): g has n_g values per entry, X and grad n_x; so that tests can drive lengths a small model does
 * not have.  Lengths may be 0.  Errors 124, 125, 127, 128 as there. */
int pk_merit_reduce_dev(pk_ctx* ctx, int B, int64_t n_g, const double* d_g, int64_t ldg, const double* d_clb, const double* d_cub,
                        int64_t n_x, const double* d_X, int64_t ldx, const double* d_vlb, const double* d_vub, const double* d_grad,
                        int64_t ldgrad, const double* d_d /* or NULL */, const double* d_f, double* d_out, void* stream);
/* ONE vector step of the CG of pk_cg.cpp on an EXPLICIT length with caller-owned device vectors and record (the public forms call
 * it with the context's vectors): so that tests can drive lengths a small model does not have.  The partial sums are the
 * context's.  step: 0 init -- d_b, d_x0 or NULL (then d_q holds K x0 on entry), d_minv or NULL, d_s or NULL; writes x, r, z, p,
 * q = s o p and the whole record from b.b, r.z, r.r and tol; 1 curvature -- pq = p.q and scalar step A; 2 update -- x, r, z,
 * r.z, r.r and scalar step B, d_minv or NULL; 3 direction -- p = z + beta p while the status is 0, q = s o p always; 4 scale --
 * q = s o q in place; 5 Jacobi -- q = 1 / |b + s| or 1.0, d_s or NULL.  Pointers a step does not use may be NULL.  Errors 110,
 * 134 for step, len or tol, 136. */
int pk_cg_step_dev(pk_ctx* ctx, int step, int64_t len, const double* d_b, const double* d_x0, const double* d_minv,
                   const double* d_s, double* d_x, double* d_r, double* d_z, double* d_p, double* d_q, double* d_rec, double tol,
                   void* stream);
/* ONE vector step of the MINRES of pk_minres.cpp on an EXPLICIT length and an EXPLICIT split index (the first index of the second
 * diagonal block, 0 <= split <= len) with caller-owned device vectors and record of 16 doubles (the public forms call it with
 * the context's vectors, len = n + m, split = n).  The partial sums are the context's.  step: 0 begin -- d_b, d_x0 or NULL (then
 * d_q holds K x0 on entry), d_minv or NULL; writes x, r1, r2, y, w = w2 = 0 and the whole record from b.(minv o b), r1.y and
 * tol; 1 Lanczos vector -- v = (1 / beta) y while the status is 0, q = the diagonal blocks' terms of v always (d_s1, d_s2 or
 * NULL); 2 alfa -- v.q and scalar step A; 3 update -- r1, r2, y, the sum of t y and scalar step B, d_minv or NULL; 4 solution
 * update -- w2, w, x when the record's slot 15 is 1; 5 diagonal blocks -- q = the terms of b (d_s1, d_s2 or NULL); 6 reciprocal
 * -- q = 1 / |b + s1| or 1.0 (d_b NULL: 0.0, d_s1 or NULL).  Pointers a step does not use may be NULL.  Errors 110, 134 for
 * step, len, split or tol, 136. */
int pk_minres_step_dev(pk_ctx* ctx, int step, int64_t len, int64_t split, const double* d_b, const double* d_x0, const double* d_minv,
                       const double* d_s1, const double* d_s2, double* d_x, double* d_r1, double* d_r2, double* d_y, double* d_v,
                       double* d_w, double* d_w2, double* d_q, double* d_rec, double tol, void* stream);
/* ONE of the three vector kernels of pk_ipm.cpp and the scalar launch behind it on an EXPLICIT length with caller-owned device
 * bounds d_lb, d_ub (the public forms call them with the context's bounds and n or m).  The partial columns are the context's.
 * kind: 0 terms -- d_v, d_zl, d_zu, mu; writes sigma to d_o1, rbar to d_o2, the record of 8 to d_out; 1 residual -- d_t (may be
 * d_o1 itself), d_z or NULL, negate; writes r to d_o1, the record of 4; 2 step -- d_v, d_dv, d_zl, d_zu, mu, tau; writes dzl to
 * d_o1, dzu to d_o2, the record of 4.  Pointers a kind does not use may be NULL.  Errors 110, 134 for kind, len, mu or tau, 136. */
int pk_ip_raw_dev(pk_ctx* ctx, int kind, int64_t len, const double* d_lb, const double* d_ub, const double* d_v, const double* d_dv,
                  const double* d_zl, const double* d_zu, const double* d_t, const double* d_z, int negate, double mu, double tau,
                  double* d_o1, double* d_o2, double* d_out, void* stream);
/* ONE of the four vector kernels of pk_slack.cpp and the scalar launch behind it on EXPLICIT lengths n, m with caller-owned device
 * bounds (the public forms call them with the context's).  The partial columns are the context's.  d_p: a HOST array of 10
 * device pointers, by kind: 0 reduce -- g, s, lam, sigma_s, rbar_s, s2 (out), b2 (out); 1 recover -- dlam, lam, rbar_s, s2,
 * sigma_s, dx, w, s1, ds (out); 2 update -- v, dv, zl, dzl, zu, dzu, lam or NULL, dlam or NULL, on the boxed vector of length m
 * with bounds d_clb, d_cub; 3 merit -- X, G, s, ds, alphas, with `batch` entries.  Slots a kind does not use may be NULL, and so
 * may d_xlb, d_xub for kinds 0 and 2.  Errors 110, 134 for kind, lengths, batch, alpha_p, alpha_d, mu or kappa, 136. */
int pk_slack_raw_dev(pk_ctx* ctx, int kind, int64_t n, int64_t m, int64_t batch, const double* d_xlb, const double* d_xub,
                     const double* d_clb, const double* d_cub, double* const* d_p, double alpha_p, double alpha_d, double mu, double kappa,
                     double* d_out, void* stream);
/* The factorisation and the solve of pk_band.cpp on a CALLER-GIVEN matrix already in band storage: d_band (ldab x nb, ldab =
 * 3 w + 1, factored in place), d_U (nb x p) and d_C (p x p) column-major (NULL allowed for p = 0), d_rhs and d_x of nb + p values in
 * permuted order ([band part | border]), d_ipiv nb 32-bit integers, d_rec the record of 8.  R, the right-hand sides of the
 * band solve, is p + 1.  The work arrays are the context's; enqueued on its stream.  Errors 110, 134, 136. */
/* The fill of the planned system alone (pk_bd_fill_k) into a caller's array of as many doubles as the plan has stored slots,
 * [band | U | C]: what pk_band_factor_dev factors.  Errors 110, 119, 134 without a plan. */
int pk_band_fill_dev(pk_ctx* ctx, const double* d_hvals, const double* d_jvals, const double* d_s1, const double* d_s2, double* d_out);
int pk_band_raw_dev(pk_ctx* ctx, int64_t nb, int32_t w, int32_t p, int32_t R, double* d_band, const double* d_U, const double* d_C,
                    const double* d_rhs, int32_t* d_ipiv, double* d_x, double* d_rec);
/* The batch of pk_band_raw_dev: B systems of one shape (1 <= B <= 16), entry e of every array e strides behind entry 0 (strides
 * in elements of the array; 0 allowed for d_U, d_C and d_rhs, which are only read: all entries share the array; every other
 * stride at least the array's length).  No fill happens.  Entry e gets the bits pk_band_raw_dev gives for its arrays alone; a
 * failed entry does not stop the others.  Errors 110, 134, 136. */
int pk_band_raw_batch_dev(pk_ctx* ctx, int32_t B, int64_t nb, int32_t w, int32_t p, int32_t R, double* d_band, int64_t stride_band,
                          const double* d_U, int64_t stride_U, const double* d_C, int64_t stride_C, const double* d_rhs, int64_t stride_rhs,
                          int32_t* d_ipiv, int64_t stride_ipiv, double* d_x, int64_t stride_x, double* d_rec, int64_t stride_rec);
/* pk_band_raw_dev with k right-hand sides (1 <= k <= 64) in place of R == p + 1: one factorisation of the caller's matrix, then
 * the block solve of pk_band_solve_multi_dev.  Right-hand side c is the nb + p values at d_rhs + c stride_rhs in permuted order,
 * its solution at d_x + c stride_x (both strides at least nb + p); one d_ipiv, one record.  Column c gets the bits pk_band_raw_dev
 * gives for it alone.  Errors 110, 134, 136. */
int pk_band_raw_multi_dev(pk_ctx* ctx, int64_t nb, int32_t w, int32_t p, int32_t k, double* d_band, const double* d_U, const double* d_C,
                          const double* d_rhs, int64_t stride_rhs, int32_t* d_ipiv, double* d_x, int64_t stride_x, double* d_rec);
/* ONE of the three kernels of the band solve's refinement (pk_band_refine.cpp) on an EXPLICIT length with caller-owned device arrays
 * (the public forms call them with the context's work, len = n + m and the plan's classification).  step: 0 residual -- d_where
 * or NULL (every element an unknown), d_b, d_q, d_x; writes r and the context's partials; 1 scalar -- reduces those partials,
 * writes the record of 8 at d_rec for step number t (0: begin; d_band_rec or NULL: a band record whose status is asked first);
 * 2 correct -- x = x + d at the unknowns while the record's status is 0.  Pointers a step does not use may be NULL.  Errors
 * 110, 134 for step, len, t, tol or min_steps, 136. */
int pk_band_refine_step_dev(pk_ctx* ctx, int step, int64_t len, const int32_t* d_where, const double* d_b, const double* d_q,
                            double* d_x, const double* d_d, double* d_r, double* d_rec, const double* d_band_rec, double tol,
                            int32_t min_steps, int32_t t);

#ifdef __cplusplus
}
#endif
#endif /* POCKIT_HIP_INTERNAL_H */
