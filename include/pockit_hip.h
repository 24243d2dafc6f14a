/* pockit_hip.h -- C ABI of the MI355X NLP-callback evaluator (libpockit_hip.so).
 *
 * STABLE SURFACE.  The 66 entry points declared here are the contract of the library: what a second host binding for
 * pockit's evaluator path needs -- life cycle, evaluation on host buffers and on device pointers, the compact layouts, the CSR
 * hand-off with its operators, reductions, the CG solve and the MINRES solve on them, batches with their merit terms, and mesh error estimation.  Everything else libpockit_hip.so exports (the plumbing of this project's own Python
 * shim, the sharding transport, the helper threads, tuning switches and diagnostics) is declared in
 * pockit_amd/csrc/pockit_hip_internal.h and may change with the project.
 *
 * Drop-in boundary: these entry points are what a host binding for pockit's evaluator path
 * binds.  Each eval function replaces one method of the reference's cyipopt ``problem_obj``
 * (class SystemBase in /root/reference/pockit/base/systembase.py):
 *
 *   pk_eval_f     <-  SystemBase.objective(x)                     systembase.py:602-605
 *   pk_eval_grad  <-  SystemBase.gradient(x)                      systembase.py:646-657
 *   pk_eval_g     <-  SystemBase.constraints(x)                   systembase.py:613-623
 *   pk_eval_jac   <-  SystemBase.jacobian(x)                      systembase.py:676-693
 *   pk_eval_hess  <-  SystemBase.hessian(x, lagrange, obj_factor) systembase.py:820-835
 *   pk_get_structure <- jacobianstructure()/hessianstructure()    systembase.py:671-674,811-818
 * and the caller they serve is cyipopt.Problem(...) built in
 * /root/reference/pockit/optimizer/ipopt.py:41-53.
 *
 * Conventions: every function returns 0 on success and a non-zero code on error, with a message
 * retrievable through pk_last_error(); the caller owns all host buffers; the library owns device
 * memory, its stream and the loaded code object; ``x`` is never written (the reference mutates
 * boundary slots in place, phasebase.py:840-847 -- we evaluate as if, without touching x); one
 * context per GPU, calls on one context are serialized by the caller (as IPOPT does).
 * No function falls back to the CPU: without a GPU / code object every eval returns an error.
 *
 * The *_dev variants take device pointers (e.g. torch tensors' data_ptr()) and a hipStream_t
 * (NULL = the context's stream); they enqueue only and do not synchronize.
 */
#ifndef POCKIT_HIP_H
#define POCKIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pk_ctx pk_ctx;

/* Compile-time facts of a generated model (pockit_amd/codegen.py) the runtime needs to launch it. */
typedef struct pk_model_desc {
  int32_t n_phase;
  int32_t n_I;          /* number of integral symbols (length of the device I buffer)            */
  int32_t nred;         /* PK_NRED the code object was compiled with                             */
  int32_t lds_g;        /* LDS doubles per wave for eval_g / eval_jac / eval_hess                */
  int32_t lds_j;
  int32_t lds_h;
  int32_t ne_j;         /* number of boundary/system scalar expressions of eval_jac / eval_hess  */
  int32_t ne_h;
  int32_t prepass_f;    /* 1 if the callback needs the integral pre-pass (pk_int)                 */
  int32_t prepass_grad;
  int32_t prepass_g;
  int32_t prepass_jac;
  int32_t prepass_hess;
  int32_t lds_x;        /* LDS doubles per wave of the fused x-kernel (pk_xall)                   */
  int32_t ne_a;         /* scalar expressions of the auxiliary pass (outer-product Hessian path)  */
  int32_t ne_hc;        /* scalar expressions of the compact Hessian                              */
  int32_t lds_e;        /* LDS doubles per wave of the mesh error estimation kernel (pk_err)      */
  int32_t tab_cap;      /* PK_TAB_CAP the code object was compiled with: entries of a staged pattern table, 64 or 256 */
  int32_t sharded;      /* 1 if the code object was generated with PK_SHARDED (in-launch exchange between GPUs)       */
  int32_t lds_jc;       /* LDS doubles per wave of the compact Jacobian kernel (pk_jacc)                                */
  int32_t ne_jc;        /* scalar expressions of the compact Jacobian                                                   */
  int32_t max_phases;   /* PK_MAX_PHASES the code object was compiled with (0: 8): phase records in its kernel arguments */
  int32_t cycle_subs;   /* workgroups per tile block of pk_cycle for a model evaluated in groups (1 + passes of J + passes of H); 0: 3 / 2 */
  int32_t hess_subs;    /* workgroups per tile block of pk_hess for such a model (passes of H); 0: 1 */
  int32_t hessc_subs;   /* ... of the compact Hessian kernel for such a model (its passes); 0: 1 */
  int32_t jacc_subs;    /* ... of the compact Jacobian kernel for such a model (its passes); 0: 1 */
  int32_t big_global;   /* 1: intervals with more than 64 points stage their rows in the device staging buffer whatever their
                           length (PK_BIG_GLOBAL: the rows of every state do not fit a workgroup's LDS); 0: only beyond 256 */
  int32_t big_rows;     /* rows one such interval stages per sub-slot (0: derived from lds_x / lds_h / lds_jc) */
  int32_t wide;         /* 1: the model has a WIDE phase (its states are evaluated in passes over chunks).  The library then refuses
                           every launch of the kernel pk_xall with error 27: the sequential values role of such a phase has an open defect
                           (round 5); the one-launch cycle and the five callbacks do not use that kernel */
} pk_model_desc;

/* One (model, mesh) instance: sizes plus the table blobs built by pockit_amd/evaluator.py.
 * ``phases``/``tiles``/``kinds``/``items_*`` are arrays of the PkPhase/PkTile/PkKind/PkItem
 * structs of pockit_amd/csrc/pk_abi.h passed as raw bytes. */
typedef struct pk_problem_desc {
  int32_t n, m, n_sys, n_s, l_s;
  int32_t n_phase, n_tiles, n_kinds;
  int64_t nnz_J, nnz_H;
  const void* phases;
  const void* tiles;
  const void* kinds;
  const void* items_jac;
  int32_t n_items_jac;
  const void* items_hess;
  int32_t n_items_hess;
  const int32_t* ib;
  int64_t n_ib;
  const double* db;
  int64_t n_db;
  const int64_t* lb;
  int64_t n_lb;
  int32_t gz_off, n_gz;
  /* outer-product path (objective / system constraints nonlinear in the integrals); all may be empty */
  const void* items_aux;
  int32_t n_items_aux;
  const void* outer;      /* PkOuter[n_outer] */
  int32_t n_outer;
  int32_t n_aux;          /* length of the auxiliary buffer */
  /* compact (coalesced) Hessian layout, optional (nnz_Hc = 0: not available) */
  const void* items_hessc;
  int32_t n_items_hessc;
  int64_t nnz_Hc;
  /* optional COO structure in the reference's order (copied; may be NULL) */
  const int32_t* jac_row;
  const int32_t* jac_col;
  const int32_t* hess_row;
  const int32_t* hess_col;
  /* compact (coalesced) Jacobian layout, optional (nnz_Jc = 0: not available) */
  const void* items_jacc;
  int32_t n_items_jacc;
  int64_t nnz_Jc;
} pk_problem_desc;

int pk_create(pk_ctx** out, int device_id);
void pk_destroy(pk_ctx* ctx);
const char* pk_last_error(pk_ctx* ctx); /* ctx may be NULL: last error of a failed pk_create */
int pk_device_count(void);

/* Loads the code object and checks the descriptor.  Error 21: a kernel every model launches (pockit_amd/csrc/pk_launch.h;
 * pk_cyclec with every compact role the descriptor has expressions for) would ask for more than 160 KiB of LDS per workgroup
 * -- expression counts, the cycle's larger staging area and the compact roles included, so a descriptor no launch could
 * serve is refused here and not by its first launch (error 22).  Code objects of pockit_amd.evaluator.compile_plan pass
 * by construction (ModelSource.fits_lds counts the same bytes). */
int pk_load_model(pk_ctx* ctx, const void* code_object, size_t len, const pk_model_desc* md);
int pk_set_problem(pk_ctx* ctx, const pk_problem_desc* pd);
int pk_get_structure(pk_ctx* ctx, int32_t* jac_row, int32_t* jac_col, int32_t* hess_row, int32_t* hess_col);

/* host-buffer API (what the cyipopt shim calls): H2D, launch, D2H, synchronize */
int pk_eval_f(pk_ctx* ctx, const double* x, double* f);
int pk_eval_grad(pk_ctx* ctx, const double* x, double* grad /* n */);
int pk_eval_g(pk_ctx* ctx, const double* x, double* g /* m */);
int pk_eval_jac(pk_ctx* ctx, const double* x, double* vals /* nnz_J */);
int pk_eval_hess(pk_ctx* ctx, const double* x, const double* lambda, double sigma, double* vals /* nnz_H */);

/* all five outputs of one cycle on the same x (fused x-kernel + Hessian), host buffers */
int pk_eval_cycle(pk_ctx* ctx, const double* x, const double* lambda, double sigma, double* f, double* grad,
                  double* g, double* jac, double* hess);

/* Compact Hessian of the Lagrangian: the reference repeats every dynamics entry for
 * each nonzero of the integration matrix (phasebase.py:923-928,1280-1285; 10-20x duplication); here lambda is
 * contracted first (mu = I^T lambda) and entries of a node with equal (row, col) are summed, so one value per
 * distinct position is produced.  Layout: pockit_amd.transcription.SystemPlan.hessc_row/col. */
int pk_eval_hessc(pk_ctx* ctx, const double* x, const double* lambda, double sigma, double* vals /* nnz_Hc */);
/* Compact Jacobian (the other half of SURVEY.md 8(f) rank 1): the reference repeats every derivative entry of a dynamics
 * function for each nonzero of the integration matrix (phasebase.py:885-887,1120-1124); where the entry's column is the
 * same on every node (t_0, t_f, a static parameter) that is K triplets on one (row, column).  pk_jacc contracts such
 * entries with the integration block first -- one value per defect row -- and sums scalar items that meet on one
 * position; entries with a per-node column keep the reference's form.  Layout: SystemPlan.jacc_row/col; scatter-added, the
 * triplets give the matrix SystemBase.jacobian (systembase.py:676-693) assembles to. */
int pk_eval_jacc(pk_ctx* ctx, const double* x, double* vals /* nnz_Jc */);
int pk_eval_jacc_dev(pk_ctx* ctx, const double* d_x, double* d_vals, void* stream);
int pk_eval_hessc_dev(pk_ctx* ctx, const double* d_x, const double* d_lambda, double sigma, double* d_vals,
                      void* stream);

/* Mesh error estimation (reference: phasebase.py:1339-1372
 * _error_estimation_data_continuous, called by check_continuous / refine_continuous, phasebase.py:1374-1437,
 * 1522-1617): every mesh interval is re-collocated with one more point; the kernel (pk_err, one wavefront per
 * group of intervals) interpolates states/controls to the augmented nodes, evaluates the dynamics there and returns both
 * sides of the integral-form collocation equation,  T = T_aug x  and  I = dt (I_aug d/2) f, per phase as
 * [n_x][rows] (rows = sum_j (K_j + 1) for LGR, sum_j K_j for LGL).  The per-interval comparison and the
 * hp-refinement decision are host logic (pockit_amd/refine.py).
 * ``intervals``: one PkErrIv (csrc/pk_abi.h) per mesh interval; ``groups``: (first record, count) pairs -- the run of
 * consecutive intervals of one phase and one K that ONE wavefront handles (K + 1 lanes per interval), padded per phase to a
 * multiple of 4 groups with count 0;
 * ``tables``: the interpolation / translation / integration blocks they index; ``n_out``: doubles per output. */
int pk_set_mesh_error_tables(pk_ctx* ctx, const void* intervals, int32_t n_intervals, const int32_t* groups,
                             int32_t n_groups, const double* tables, int64_t n_tables, int64_t n_out);
int pk_eval_mesh_error(pk_ctx* ctx, const double* x, double* T /* n_out */, double* I /* n_out */);
int pk_eval_mesh_error_dev(pk_ctx* ctx, const double* d_x, double* d_T, double* d_I, void* stream);

/* Device-resident CSR hand-off (the reference hands host triplets to IPOPT,
 * optimizer/ipopt.py:41-53).  The triplet values of J (which = 0) or H (which = 1, lower triangle) are gathered
 * into CSR order on the device, repeated (row, col) entries summed in triplet order: the matrices can feed a
 * GPU KKT solve without crossing PCIe.  ``perm[q]``: triplet index of the q-th entry in (row, col) order;
 * ``seg[p] .. seg[p+1]``: the run of q belonging to CSR entry p (NULL when no entry repeats).  The CSR
 * structure itself (indptr, indices) is host data: pockit_amd/csr.py.  which = 2 maps the COMPACT Hessian values
 * (pk_eval_hessc, one value per distinct entry) onto the same CSR entries: when it is set, pk_eval_hess_csr(_dev) evaluate
 * the compact form and permute instead of writing and re-adding every repeated triplet.  which = 3 does the same for the
 * Jacobian with the compact values of pk_eval_jacc (its few repeated positions are summed by the gather). */
int pk_set_csr_map(pk_ctx* ctx, int which, const int32_t* seg /* n_unique + 1 or NULL */, const int32_t* perm,
                   int64_t n_unique, int64_t n_triplets);
int pk_gather_csr_dev(pk_ctx* ctx, int which, const double* d_triplets, double* d_csr, void* stream);
int pk_eval_jac_csr_dev(pk_ctx* ctx, const double* d_x, double* d_csr, void* stream);
int pk_eval_hess_csr_dev(pk_ctx* ctx, const double* d_x, const double* d_lambda, double sigma, double* d_csr,
                         void* stream);
int pk_eval_jac_csr(pk_ctx* ctx, const double* x, double* vals /* n_unique */);
int pk_eval_hess_csr(pk_ctx* ctx, const double* x, const double* lambda, double sigma, double* vals);

/* The matrices of the CSR hand-off applied to vectors on the device: y = A v (+ add) with A = J (op 0), J^T (op 1) or the
 * symmetric H (op 2, from its lower triangle), the values read where pk_eval_*_csr_dev / pk_gather_csr_dev left them.
 * An operator is a CSR structure (indptr, indices; int32) whose entry e takes its value from vals[src[e]] of the CSR value
 * array of a map (src NULL: vals[e]): pockit_amd/csr.py builds the three from the maps (J itself; the transpose; L + L^T -
 * diag(L), each off-diagonal entry twice with one src).  pk_set_csr_operator needs the matching pk_set_csr_map (which = 0 for
 * op 0 / 1, which = 1 for op 2), checks everything a kernel will index with (errors 110-116, 119) and cuts the rows into
 * the kernels' work items; pk_set_csr_map and pk_set_problem drop every operator.  indices and src are only range-checked: a
 * row may list a column more than once, in any order, and y[row] is then the sum over the listed entries.  Every y[row] is
 * a fixed expression of the inputs (no atomics): the same bits from run to run.  ``d_add`` may be NULL and may alias ``d_y``.
 * pk_linearize evaluates the CSR values of J at x -- and of H with (lambda, sigma) unless lambda is NULL -- into the
 * context's own value arrays (the ones pk_eval_jac_csr / pk_eval_hess_csr use) and downloads nothing; pk_apply_operator
 * sends v up, multiplies with that linearization and brings y down (error 118: no linearization, or none of H for op 2;
 * 117: no operator).  A context holds one linearization: pk_eval_jac_csr / pk_eval_hess_csr and pk_set_csr_map end it. */
int pk_set_csr_operator(pk_ctx* ctx, int op, const int32_t* indptr /* n_rows + 1 */, const int32_t* indices,
                        const int32_t* src /* nnz or NULL */, int32_t n_rows, int32_t n_cols, int64_t nnz);
int pk_apply_operator_dev(pk_ctx* ctx, int op, const double* d_vals, const double* d_v, const double* d_add, double* d_y,
                          void* stream);
int pk_linearize(pk_ctx* ctx, const double* x, const double* lambda /* or NULL */, double sigma);
int pk_apply_operator(pk_ctx* ctx, int op, const double* v, double* y);
/* The same operators applied to a BLOCK of k >= 1 vectors in one call: Y = A V (+ Add).  Device layout row-major with leading
 * dimensions: V[i * ldv + j] (row i < n_cols, column j < k, ldv >= k), Y[r * ldy + j] (ldy >= k), Add NULL or laid out like Y
 * with the same ldy, and it may alias Y -- NumPy's C order for an (n, k) array when ld = k; ld > k addresses a column range of
 * a wider block in place.  Only entries of Y with a column index below k are written.  A workgroup handles up to 8 columns of
 * one row block and reads the structure and the values once for them; k > 8 runs ceil(k / 8) chunks of launches on the stream.
 * Column j of Y has exactly the bits pk_apply_operator_dev gives for column j of V (and of Add).  Errors as for the single
 * form (110, 117, 118), and 120: k < 1; 121: ldv < k or ldy < k; 122: no device memory for the block's partial sums (allocated
 * on an operator's first block product) or for the host form's scratch (grown to max(n, m) * k doubles when k exceeds what it
 * holds).  The host form takes C-contiguous V (n_cols x k) and Y (n_rows x k) and multiplies with the context's linearization. */
int pk_apply_operator_block_dev(pk_ctx* ctx, int op, const double* d_vals, int32_t k, const double* d_V, int64_t ldv,
                                const double* d_Add, double* d_Y, int64_t ldy, void* stream);
int pk_apply_operator_block(pk_ctx* ctx, int op, int32_t k, const double* V, double* Y);
/* What a solver needs about the ENTRIES of the same operators, not about a product (kernels pk_red_rows, pk_red_long, pk_diag of
 * the library): a reduction over the rows of operator op with a_e = vals[src ? src[e] : e], c_e = indices[e], an optional
 * weight d_w (n_cols values; NULL: the weight is left out, not multiplied by 1.0) and an optional d_add (n_rows values, may
 * alias d_y):
 *   mode 0 abs_sum   t_e = fabs(a_e) * w[c_e]                                     y[row] = sum_e t_e (+ add[row])
 *   mode 1 sq_sum    t_e = (a_e * a_e) * w[c_e], the square rounded first         y[row] = sum_e t_e (+ add[row])
 *   mode 2 abs_max   t_e = fabs(a_e) * w[c_e]                                     y[row] = max(0, max_e t_e, add[row])
 * Row norms of J: op 0; column norms of J: op 1; diag(J D J^T): op 0, mode 1, w = d; diag(J^T D J): op 1, mode 1, w = d.  The
 * two sums have exactly the association of pk_apply_operator_dev over the same row blocks (no atomics, no dependence on the
 * grid, the same bits from run to run) and share its partial-sum slots, ordered by the stream.  Mode 2 walks the same way
 * but takes maxima by comparison (m = 0.0; if (t > m) m = t;): a NaN term loses, the zero padding is the identity, the
 * result is never negative and never -0.0, and a negative weight gives what the arithmetic gives.  NaN is not screened for.
 * The diagonal of H: y[i] = pos[i] >= 0 ? vals[pos[i]] : 0.0 (+ add[i]); pk_set_operator_diagonal (op must be 2) uploads pos
 * once -- n int32 entries pointing into the CSR value array of the Hessian map (pk_set_csr_map(1)), -1 for a row without a
 * diagonal entry -- after checking it on the host and waiting for the device (a diagonal enqueued earlier on any stream may
 * still read the old positions); pk_set_csr_map and pk_set_problem drop it with the operators.
 * The host forms work on the context's linearization (pk_linearize): pk_operator_reduce sends w up (NULL: none) and brings y
 * down; add_diagonal != 0 (op 1 or 2) computes diag(H) on the device first and reduces with add aliasing y, one round trip
 * for diag(H + J^T D J).  Errors: 110 op out of range or a null pointer; 117 no operator; 118 no linearization, or none of
 * H; 119 a sharded context; 111 no Hessian map; 129 mode out of range; 130 a diagonal asked of an operator that is not
 * square (op 0 or 1), or added to rows that are not H's; 131 pos of the wrong length or with an entry that is neither -1
 * nor in [0, n_unique); 132 a diagonal before pk_set_operator_diagonal.  Nothing is enqueued after a refusal. */
int pk_operator_reduce_dev(pk_ctx* ctx, int op, int mode, const double* d_vals, const double* d_w /* or NULL */,
                           const double* d_add /* or NULL */, double* d_y, void* stream);
int pk_operator_reduce(pk_ctx* ctx, int op, int mode, const double* w /* or NULL */, int add_diagonal, double* y);
int pk_set_operator_diagonal(pk_ctx* ctx, int op, const int32_t* pos, int32_t n);
int pk_operator_diagonal_dev(pk_ctx* ctx, int op, const double* d_vals, const double* d_add /* or NULL */, double* d_y,
                             void* stream);
int pk_operator_diagonal(pk_ctx* ctx, int op, double* y);

/* device-pointer API: enqueue on ``stream`` (hipStream_t, NULL = context stream), no sync */
int pk_eval_f_dev(pk_ctx* ctx, const double* d_x, double* d_f, void* stream);
int pk_eval_grad_dev(pk_ctx* ctx, const double* d_x, double* d_grad, void* stream);
int pk_eval_g_dev(pk_ctx* ctx, const double* d_x, double* d_g, void* stream);
int pk_eval_jac_dev(pk_ctx* ctx, const double* d_x, double* d_vals, void* stream);
int pk_eval_hess_dev(pk_ctx* ctx, const double* d_x, const double* d_lambda, double sigma, double* d_vals,
                     void* stream);
/* the four x-only outputs of one iterate (what a line search's trial point needs, what the host shim runs on a new x):
 * the fused x-kernel + the one-workgroup reduction, two launches */
int pk_eval_xpart_dev(pk_ctx* ctx, const double* d_x, double* d_f, double* d_grad, double* d_g, double* d_jac, void* stream);
/* one NLP-callback cycle f, grad f, g, J, H on the same x (IPOPT's per-iteration pattern), as ONE launch
 * (pk_cycle: the workgroups of the fused x-kernel -- each node evaluated once for f, grad f, g, J -- and of the
 * Hessian kernel side by side, plus a finalize workgroup fed by the same launch).  One cycle may be in flight
 * per context at a time (the launch owns the context's hand-off slots). */
int pk_eval_cycle_dev(pk_ctx* ctx, const double* d_x, const double* d_lambda, double sigma, double* d_f,
                      double* d_grad, double* d_g, double* d_jac, double* d_hess, void* stream);
/* Which layouts pk_eval_cycle_dev[_repeat] writes: 0 = the reference's triplet lists (systembase.py:676-693, 820-835), 1 = the
 * compact layouts of pk_set_problem (nnz_Jc / nnz_Hc values: pk_eval_jacc / pk_eval_hessc).  A compact
 * cycle stays ONE launch: the compact kernels' tile code runs in the Jacobian / Hessian roles of pk_cycle.  Error 69 for a
 * model whose system functions are nonlinear in the integrals or a mesh with an interval of more than 64 points. */
int pk_set_cycle_layout(pk_ctx* ctx, int jac_compact, int hess_compact);

/* A BATCH of iterates in one launch of the fused cycle (kernel pk_cycleb, blockIdx.y = batch entry): a caller that holds B
 * iterates -- multi-start, a merit scan over trial points, a lock-step ensemble -- pays the fixed cost of a launch once per
 * batch.  Entry b computes exactly what pk_eval_cycle_dev computes on (x_b, lambda_b, sigma_b), bit for bit.
 *
 * pk_load_batch_model attaches the model's BATCHED code object (pockit_amd.codegen.ModelSource(plan, batched=True): the same
 * model code, pk_cycleb its only kernel) to a context that has its model; the descriptor is the model's.  Error 86: the object
 * has no pk_cycleb.  code_object = NULL drops the batched object again.
 * pk_set_batch allocates what a launch writes beside the caller's outputs once per entry (integrals, partial sums, hand-off
 * slots, auxiliary buffer, staging rows) and the device array of B argument records; idempotent for the same B; a smaller B keeps the
 * workspaces of the larger one (a context never shrinks them short of a new problem); freed with the problem.  Error 87: B outside 1 ... PK_MAX_BATCH.  pk_eval_cycle_batch_dev calls it where needed.
 * pk_eval_cycle_batch_dev: all arrays are [B][...] row-major in device memory, rows of d_x / d_lambda ldx >= n / ldlambda >= m
 * doubles apart, the outputs dense ([B], [B][n], [B][m], [B][nnz_J], [B][nnz_H]); ``sigma``: B values in HOST memory.
 * d_lambda = NULL: an x-only batch (f, grad f, g, J; d_hess and sigma are not touched).  The argument records are written on
 * the host (pinned memory of the context) and copied on ``stream`` ahead of the ONE launch, every call; a call waits for the
 * record copy of the call before it, not for its kernel.  One batch or one single cycle may be in flight per context at a
 * time; a hand-off that gives up in any entry is error 97 for the whole call (pk_sync), which puts the hand-off slots of
 * every entry back to empty.
 * Contexts whose cycle is not the one-launch cycle -- a model that needs the integrals first, the stand-alone kernels
 * (separate_x), a shard, pk_set_cycle_mode(0), no batched object loaded -- are served by a loop of single cycles inside the
 * call: the same values, no speed claim.  Error 88: a compact cycle layout, or a sharded context with the in-launch exchange.
 * Error 89: a null pointer or a leading dimension that is too small. */
#define PK_MAX_BATCH 64
int pk_load_batch_model(pk_ctx* ctx, const void* code_object, size_t len);
int pk_set_batch(pk_ctx* ctx, int B);
int pk_eval_cycle_batch_dev(pk_ctx* ctx, int B, const double* d_x, int64_t ldx, const double* d_lambda, int64_t ldlambda,
                            const double* sigma /* host, B values */, double* d_f, double* d_grad, double* d_g,
                            double* d_jac, double* d_hess, void* stream);
int pk_sync(pk_ctx* ctx, void* stream);

/* MERIT TERMS of a batch of trial points, reduced on the device (kernels pk_trial, pk_merit, pk_merit_fin of the library): what
 * a line search or a multi-start ranking wants back from a batch is a handful of scalars per point, not J.  Per entry b a row
 * of 8 doubles out[b * 8 + q]:
 *   0 f[b]                                              4 bound1     sum_i viol(X[b,i], v_lb[i], v_ub[i])
 *   1 theta1     sum_i viol(g[b,i], c_lb[i], c_ub[i])   5 bound_inf  max_i of the same
 *   2 theta_inf  max_i of the same                      6 slope      sum_i grad[b,i] * d[i], 0.0 when d is NULL
 *   3 theta2_sq  sum_i viol^2                           7 bad        non-finite values among f[b], g[b,:], grad[b,:]
 * viol(v, lo, hi) = max(lo - v, v - hi, 0); bounds may be infinite.  A non-finite g or grad entry is counted in column 7 and
 * adds nothing elsewhere: the other columns stay finite and the caller rejects the point on out[b * 8 + 7] > 0.  Every square
 * and product is rounded before it is added (no fused multiply-add); the association of the sums is fixed (pk_merit.cpp,
 * DESIGN.md section 16) and depends neither on the grid nor on the run: no atomics, the same bits every time.
 *
 * pk_set_bounds: host arrays of m, m, n, n doubles, validated and uploaded (error 126: a null pointer, a NaN, lb > ub);
 * pk_set_problem drops them.
 * pk_trial_points_dev: X[b * ldx + i] = x[i] + alpha[b] * d[i] for b < B <= PK_MAX_BATCH, with exactly the bits of the
 * rounded product added to x[i]; ``alpha``: B values in HOST memory, read before the call returns (they travel in the kernel
 * arguments).
 * pk_merit_batch_dev: the rows of B <= PK_MAX_BATCH entries from device arrays as pk_eval_cycle_batch_dev leaves them (rows of
 * g / grad / X ldg >= m / ldgrad >= n / ldx >= n doubles apart, f dense), measured against the uploaded bounds; d_d (n values)
 * may be NULL.  Two launches on ``stream``, not waited for.  The partial results lie in an array of the context that grows when
 * needed: one reduction may be in flight per context at a time.
 * pk_merit_scan / pk_merit_batch: the host forms.  They upload (x, d and form the trial points; or the rows of X, ldx >= n
 * doubles apart), run the x-only batch (pk_eval_cycle_batch_dev without lambda) into scratch the context owns -- one slice
 * per entry -- and the two reduction launches, download 8 * B doubles into ``out`` and synchronize once.  B has no upper
 * limit: they walk it in chunks of min(PK_MAX_BATCH, max(1, 256 MiB / (8 (nnz_J + n + m + 1)))) entries, which bounds the
 * scratch; it grows when needed, never shrinks, and is freed by pk_set_problem.  A context whose batch is served by the loop
 * of single cycles gives the same values.
 * Errors: 123 no bounds set; 124 B < 1, or above PK_MAX_BATCH in a _dev form; 125 a leading dimension below its length;
 * 126 bounds rejected; 127 no device memory (nothing is enqueued, what was there stays); 128 a null device pointer; 60 a null
 * host buffer; 88 (host forms) a compact cycle layout or a sharded context with the in-launch exchange, as for the batch. */
int pk_set_bounds(pk_ctx* ctx, const double* c_lb /* m */, const double* c_ub /* m */, const double* v_lb /* n */,
                  const double* v_ub /* n */);
int pk_trial_points_dev(pk_ctx* ctx, int B, const double* d_x, const double* d_d, const double* alpha /* host, B values */,
                        double* d_X, int64_t ldx, void* stream);
int pk_merit_batch_dev(pk_ctx* ctx, int B, const double* d_f, const double* d_g, int64_t ldg, const double* d_grad,
                       int64_t ldgrad, const double* d_X, int64_t ldx, const double* d_d /* or NULL */, double* d_out /* B x 8 */,
                       void* stream);
int pk_merit_scan(pk_ctx* ctx, int64_t B, const double* x, const double* d, const double* alpha /* B */, double* out /* B x 8 */);
int pk_merit_batch(pk_ctx* ctx, int64_t B, const double* X, int64_t ldx, const double* d /* or NULL */, double* out /* B x 8 */);

/* THE CONDENSED KKT MATRIX AND THE NORMAL EQUATIONS, applied and solved by preconditioned CG where the linearization lies
 * (kernels pk_cg_init, pk_cg_dot, pk_cg_update, pk_cg_scalar, pk_cg_elem of the library; pk_cg.cpp).
 *   form 0, primal, size n:  K v = [H v] + J^T (d o (J v)) + s o v     d: m values, s: n values
 *   form 1, dual, size m:    K v = J (d o (J^T v)) + s o v             d: n values, s: m values; no H
 * d NULL: D = I, no scaling launch; s NULL: no diagonal term; d_hvals NULL: no H.  The products are pk_apply_operator_dev's with
 * their association, in the fixed order q = s o v, t = A1 v, t = d o t, q = H v + q, q = A2 t + q; no product is fused with a sum.
 * pk_condensed_apply_dev enqueues one application y = K v; pk_condensed_apply does it on the values of pk_linearize, one round
 * trip.  The solve keeps a record of 8 doubles on the device: 0 status (0 running, 1 converged, 2 non-positive curvature,
 * 3 non-finite scalar), 1 completed iterations, 2 r.r of the recurrence, 3 the threshold tol^2 b.b, 4 r.z, 5 the last p^T K p,
 * 6 the last alpha, 7 the last beta.  pk_cg_begin_dev takes caller-owned device arrays that stay valid and unchanged until the
 * solve ends -- d_d, d_s, d_minv -- (a diagonal preconditioner z = minv o r, NULL: none) and d_x0 may be NULL; x is written to
 * d_x; convergence is r.r <= tol^2 b.b.  pk_cg_advance_dev enqueues iters iterations with no synchronisation; once the status
 * is not 0 an iteration leaves x and the record untouched, so x, iterations and status do not depend on how many were enqueued
 * beyond the stop.  pk_cg_record copies the record and synchronises.  One solve per context at a time; pk_set_csr_operator,
 * pk_set_csr_map and pk_set_problem forget it.  The sums are associated in a fixed way: no atomics, the same bits every run.
 * pk_solve_condensed is the host form on pk_linearize's values: uploads, the preconditioner -- precond 0 none, 1 Jacobi built
 * on the device, minv = 1 / |diag K| or 1.0 where that is zero or not finite, 2 the caller's minv -- begin, chunks of
 * min check_every, remaining iterations each followed by a read of the record until the status is not 0 or maxiter iterations
 * are done, x down.  Exhaustion is status 4 in the host copy rec.  A status is a result, not an error: the call returns 0.
 * Errors: those of the products -- 110, 117, 118, 119 -- and 132 Jacobi with H before pk_set_operator_diagonal; 133 form out of
 * range, or H with form 1; 134 tol negative or not finite, iters, maxiter or check_every below 1, precond out of range;
 * 135 advance or record without a begin; 136 no device memory; 60 a null host buffer.  Nothing is enqueued after a refusal. */
int pk_condensed_apply_dev(pk_ctx* ctx, int form, const double* d_jvals, const double* d_hvals /* or NULL */,
                           const double* d_d /* or NULL */, const double* d_s /* or NULL */, const double* d_v, double* d_y,
                           void* stream);
int pk_condensed_apply(pk_ctx* ctx, int form, int with_h, const double* d /* or NULL */, const double* s /* or NULL */,
                       const double* v, double* y);
int pk_cg_begin_dev(pk_ctx* ctx, int form, const double* d_jvals, const double* d_hvals /* or NULL */, const double* d_d,
                    const double* d_s, const double* d_minv /* or NULL */, const double* d_b, const double* d_x0 /* or NULL */,
                    double* d_x, double tol, void* stream);
int pk_cg_advance_dev(pk_ctx* ctx, int iters, void* stream);
int pk_cg_record(pk_ctx* ctx, double* rec /* 8 */);
int pk_solve_condensed(pk_ctx* ctx, int form, int with_h, const double* d, const double* s, int precond,
                       const double* minv /* precond 2 */, const double* b, const double* x0 /* or NULL */, double tol, int maxiter,
                       int check_every, double* x, double* rec /* 8 */);

/* THE AUGMENTED KKT SYSTEM, applied and solved by preconditioned MINRES where the linearization lies (kernels pk_mr_init,
 * pk_mr_dot, pk_mr_update, pk_mr_scalar, pk_mr_elem of the library; pk_minres.cpp).  Symmetric and
 * INDEFINITE, of size N = n + m, vectors [primal (n) | dual (m)] contiguous:
 *   K = [ H + diag(s1)    J^T     ]     s1: n values or NULL (no term); s2: m values or NULL (no term: equality constraints);
 *       [     J       -diag(s2)   ]     d_hvals NULL: no H
 * One application runs in the fixed order q = (s1 o v1 | -(s2 o v2)) (or 0.0), q1 = H v1 + q1, q1 = J^T v2 + q1,
 * q2 = J v1 + q2, the products pk_apply_operator_dev's with their association; no product is fused with a sum.
 * pk_kkt_apply_dev enqueues one application y = K v; pk_kkt_apply does it on the values of pk_linearize, one round trip.
 * The solve keeps a record of 16 doubles on the device: 0 status (0 running, 1 converged, 2 preconditioner not positive --
 * r.Mr < 0 --, 3 non-finite scalar or gamma == 0), 1 completed iterations, 2 phibar (the recurrence's |b - K x| in the
 * M-norm), 3 the threshold tol sqrt(b.(minv o b)), 4 beta, 5 oldb, 6 alfa, 7 dbar, 8 epsln, 9 cs, 10 sn, 11 phi, 12 oldeps,
 * 13 delta, 14 gamma (Paige and Saunders' names), 15 internal (0 in every host copy).  pk_minres_begin_dev takes caller-owned
 * device arrays that stay valid and unchanged until the solve ends -- d_s1, d_s2, d_minv (a diagonal POSITIVE preconditioner
 * y = minv o r of N values, NULL: none) -- and d_x0 may be NULL; x (N values) is written to d_x; convergence is
 * phibar <= tol sqrt(b.(minv o b)).  pk_minres_advance_dev enqueues iters iterations with no synchronisation; once the status is
 * not 0 an iteration leaves x and the record untouched, so x, iterations and status do not depend on how many were enqueued
 * beyond the stop.  pk_minres_record copies the record and synchronises.  One solve per context at a time; pk_set_csr_operator,
 * pk_set_csr_map and pk_set_problem forget it.  The sums are associated in a fixed way: no atomics, the same bits every run.
 * pk_solve_kkt is the host form on pk_linearize's values: uploads, the preconditioner -- precond 0 none, 1 diagonal, built on
 * the device: minv1 = 1 / |diag H + s1|, minv2_i = 1 / |sum_j J_ij^2 minv1_j + s2_i|, 1.0 where the denominator is zero or not
 * finite, 2 the caller's minv of N values -- begin, chunks of min(check_every, remaining) iterations each followed by a read of
 * the record until the status is not 0 or maxiter iterations are done, then x (N values) comes down; exhaustion is status 4 in
 * the host copy only, and a result: the call returns 0.
 * Errors: 110 a null device pointer; 117 an operator is not set; 118 no (matching) linearization; 119 a sharded context;
 * 132 precond 1 with H before pk_set_operator_diagonal; 134 tol negative or not finite, iters, maxiter or check_every below 1,
 * precond out of range; 135 advance or record without a begin; 136 no device memory; 60 a null host buffer.  Nothing is
 * enqueued after a refusal. */
int pk_kkt_apply_dev(pk_ctx* ctx, const double* d_jvals, const double* d_hvals /* or NULL */, const double* d_s1 /* or NULL */,
                     const double* d_s2 /* or NULL */, const double* d_v, double* d_y, void* stream);
int pk_kkt_apply(pk_ctx* ctx, int with_h, const double* s1 /* or NULL */, const double* s2 /* or NULL */, const double* v,
                 double* y);
int pk_minres_begin_dev(pk_ctx* ctx, const double* d_jvals, const double* d_hvals /* or NULL */, const double* d_s1,
                        const double* d_s2, const double* d_minv /* or NULL */, const double* d_b, const double* d_x0 /* or NULL */,
                        double* d_x, double tol, void* stream);
int pk_minres_advance_dev(pk_ctx* ctx, int iters, void* stream);
int pk_minres_record(pk_ctx* ctx, double* rec /* 16 */);
int pk_solve_kkt(pk_ctx* ctx, int with_h, const double* s1, const double* s2, int precond, const double* minv /* precond 2 */,
                 const double* b, const double* x0 /* or NULL */, double tol, int maxiter, int check_every, double* x,
                 double* rec /* 16 */);

/* WHAT A PRIMAL-DUAL INTERIOR-POINT ITERATION NEEDS AROUND ITS SOLVE, where the vectors lie (kernels pk_ip_terms_k, pk_ip_resid_k,
 * pk_ip_step_k, pk_ip_scalar_k of the library; pk_ipm.cpp).  A BOXED VECTOR is v of length L with the bounds
 * of pk_set_bounds: which = 0 the n variables (v_lb, v_ub), which = 1 the m slacks of the constraint rows (c_lb, c_ub).  Per
 * element lb == ub is fixed and has no side; otherwise a side is present when its bound is finite; dl = v - lb, du = ub - v.  An
 * absent side contributes no term and nothing of it is read.  A present side is BAD when its slack is not > 0 or not finite or its
 * multiplier is negative or not finite: counted, left out of every other column, 0.0 in its bracket.
 * pk_ip_terms_dev: sigma_i = [zl_i / dl] + [zu_i / du] and rbar_i = [mu / dl] - [mu / du] (a single present bracket stored as it
 * is, 0.0 without a side) and a record of 8: 0 compl_inf = max |dl zl - mu|, |du zu - mu|; 1 compl_sum = sum dl zl + sum du zu;
 * 2 sides (good ones, counted); 3 min_slack (+inf without a side); 4 log_sum = sum ln dl + sum ln du; 5 bad; 6 z_sum; 7 min_compl
 * = min dl zl, du zu (+inf without a side).
 * pk_dual_residual_dev: t = J^T lambda + grad by pk_apply_operator_dev (op 1, add = grad; d_jvals the CSR values of the Jacobian
 * map, as pk_kkt_apply_dev takes them), then r_i = t_i - z_i (d_z NULL: no term), negated when negate != 0, 0.0 for a fixed
 * variable; a record of 4: 0 r_inf = max |r_i|, 1 r_sq = sum r_i^2, 2 bad (non-finite r_i, left out of 0 and 1), 3 0.0.
 * z = zl - zu gives the optimality test, z = rbar with negate the right-hand side b1 of the KKT step.
 * pk_ip_step_dev: dzl_i = (mu / dl - zl_i) - (zl_i / dl) dv_i, dzu_i = (mu / du - zu_i) + (zu_i / du) dv_i (0.0 on an absent or
 * bad side) and a record of 4: 0 alpha_pri = min(1, (tau dl) / (-dv_i) over lower sides with dv_i < 0, (tau du) / dv_i over upper
 * sides with dv_i > 0); 1 alpha_dual likewise from (tau zl) / (-dzl_i), dzl_i < 0, and (tau zu) / (-dzu_i), dzu_i < 0;
 * 2 arg_pri, the smallest index that attains alpha_pri, -1.0 when alpha_pri is 1; 3 bad: bad sides, plus the elements with a
 * side whose dv_i is not finite (counted once, left out).
 * Every product and quotient is rounded before its sum (no fused multiply-add); the sums, maxima and minima are associated in
 * a fixed way (pieces of 2048, the fixed tree, one scalar launch): no atomics, the same bits every run.  The _dev forms enqueue
 * on `stream` (NULL: the context's) and do not synchronise; d_out is a device array.  They share the context's one array of partial
 * columns whatever the stream, so the calls of one context must be stream-ordered: enqueue them on one stream, or order the
 * streams with events.  pk_ip_terms, pk_dual_residual (on
 * pk_linearize's values) and pk_ip_step are the host forms: upload, the _dev form, download, one synchronisation.
 * Errors: 110 a null device pointer; 117 J^T is not set; 118 no linearization; 119 a sharded context; 123 no bounds
 * (pk_set_bounds); 134 which not 0 or 1, mu negative or not finite, tau outside (0, 1]; 136 no device memory; 60 a null host
 * buffer.  Nothing is enqueued or written after a refusal. */
int pk_ip_terms_dev(pk_ctx* ctx, int which, const double* d_v, const double* d_zl, const double* d_zu, double mu, double* d_sigma,
                    double* d_rbar, double* d_out /* 8 */, void* stream);
int pk_dual_residual_dev(pk_ctx* ctx, const double* d_jvals, const double* d_grad, const double* d_lam, const double* d_z /* or NULL */,
                         int negate, double* d_r, double* d_out /* 4 */, void* stream);
int pk_ip_step_dev(pk_ctx* ctx, int which, const double* d_v, const double* d_dv, const double* d_zl, const double* d_zu, double mu,
                   double tau, double* d_dzl, double* d_dzu, double* d_out /* 4 */, void* stream);
int pk_ip_terms(pk_ctx* ctx, int which, const double* v, const double* zl, const double* zu, double mu, double* sigma, double* rbar,
                double* out /* 8 */);
int pk_dual_residual(pk_ctx* ctx, const double* grad, const double* lam, const double* z /* or NULL */, int negate, double* r,
                     double* out /* 4 */);
int pk_ip_step(pk_ctx* ctx, int which, const double* v, const double* dv, const double* zl, const double* zu, double mu, double tau,
               double* dzl, double* dzu, double* out /* 4 */);

/* THE SLACKS OF A RESIDENT PRIMAL-DUAL ITERATE (kernels pk_sl_reduce_k, pk_sl_recover_k, pk_sl_update_k, pk_sl_merit_k,
 * pk_sl_scalar_k of the library; pk_slack.cpp).  Rows are classified as the boxed vector which = 1 above:
 * c_lb == c_ub is an EQUALITY row (no slack; nothing of s, of the slack's barrier terms or of its multipliers is read there), any
 * other row an INEQUALITY row g_i - s_i = 0 whose slack s_i is boxed by the finite ones of c_lb_i, c_ub_i.  A fixed variable
 * (v_lb == v_ub) takes part in nothing.  sigma_s, rbar_s are what pk_ip_terms_dev (which = 1) wrote for the slacks.
 * pk_slack_reduce_dev: the slacks out of the step's system [[H + Sigma_x, J^T], [J, -S2]] (dx, dlam) = (b1, b2).  Equality row:
 * s2_i = 0.0, b2_i = -(g_i - c_lb_i); inequality row: s2_i = 1 / sigma_s_i, b2_i = (-(g_i - s_i)) + s2_i (lam_i + rbar_s_i).
 * A sigma_s_i that is not > 0 or not finite is bad: counted, s2_i = b2_i = 0.0.  A record of 4: 0 theta_inf = max |g - c|,
 * |g - s|; 1 theta_1, their sum; 2 bad (bad sigma_s_i and residuals that are not finite, both left out of 0 and 1); 3 the
 * inequality rows, counted.  s2 and b2 feed pk_minres_begin_dev / pk_solve_kkt as they are.
 * pk_slack_recover_dev: ds_i = s2_i ((dlam_i + lam_i) + rbar_s_i) on inequality rows, 0.0 on equality rows and on a bad
 * sigma_s_i, and the terms of the inertia-free curvature test with w = H dx (pk_apply_operator_dev) and s1 = Sigma_x: a record of
 * 5 over the free variables and the inequality rows: 0 sum (dx_i w_i + s1_i dx_i^2); 1 sum sigma_s_i ds_i^2; 2 sum dx_i^2;
 * 3 sum ds_i^2; 4 bad (bad sigma_s_i, terms that are not finite; left out).  The test is rec0 + rec1 >= kappa (rec2 + rec3).
 * pk_slack_update_dev, IN PLACE on a boxed vector (which as above): v_i += alpha_p dv_i where not fixed; on a present side
 * z_i += alpha_d dz_i, then with the NEW slack d the safeguard z_i = min(max(z_i, mu / (kappa d)), (kappa mu) / d); an absent
 * side is neither read nor written.  With d_lam, d_dlam (both or neither; which = 1 only, else 134): lam_i += alpha_p dlam_i on
 * every row.  A record of 4: 0 clamped multipliers; 1 the smallest new slack (+inf without a side); 2 bad: a new v_i or lam_i
 * that is not finite, a new slack that is not > 0, a new multiplier that is not finite -- stored as computed, not clamped;
 * 3 0.0.
 * pk_slack_merit_dev: count trial points X (count x n, as pk_trial_points_dev wrote them) with their constraint values G
 * (count x m) and the slacks s + alphas[b] ds; per entry 4 doubles: 0 theta_1 = sum_eq |g - c| + sum_ineq |g - (s + alpha ds)|;
 * 1 theta_inf; 2 log_sum over the present sides of X[b] and of the slacks; 3 bad (a side whose slack is not > 0 or not finite, a
 * residual that is not finite; left out).
 * Arithmetic, association, streams and synchronisation as for pk_ip_terms_dev above: every product and quotient rounded on its
 * own, pieces of 2048, the fixed tree, one scalar launch (one workgroup per entry of a batch); no atomics, the same bits every
 * run; the calls of one context must be stream-ordered.  pk_slack_reduce, pk_slack_recover and pk_slack_update are the host
 * forms (pk_slack_update works in place on the host arrays; lam, dlam NULL or both).
 * Errors: 110 a null device pointer; 119 a sharded context; 123 no bounds (pk_set_bounds); 134 which not 0 or 1, lam without
 * which = 1, alpha_p or alpha_d outside [0, 1], mu negative or not finite, kappa below 1 or not finite, count < 1; 136 no device
 * memory; 60 a null host buffer.  Nothing is enqueued or written after a refusal. */
int pk_slack_reduce_dev(pk_ctx* ctx, const double* d_g, const double* d_s, const double* d_lam, const double* d_sigma_s,
                        const double* d_rbar_s, double* d_s2, double* d_b2, double* d_out /* 4 */, void* stream);
int pk_slack_recover_dev(pk_ctx* ctx, const double* d_dlam, const double* d_lam, const double* d_rbar_s, const double* d_s2,
                         const double* d_sigma_s, const double* d_dx, const double* d_w, const double* d_s1, double* d_ds,
                         double* d_out /* 5 */, void* stream);
int pk_slack_update_dev(pk_ctx* ctx, int which, double* d_v, const double* d_dv, double* d_zl, const double* d_dzl, double* d_zu,
                        const double* d_dzu, double* d_lam /* or NULL */, const double* d_dlam /* or NULL */, double alpha_p,
                        double alpha_d, double mu, double kappa, double* d_out /* 4 */, void* stream);
int pk_slack_merit_dev(pk_ctx* ctx, int32_t count, const double* d_X, const double* d_G, const double* d_s, const double* d_ds,
                       const double* d_alphas, double* d_out /* 4 * count */, void* stream);
int pk_slack_reduce(pk_ctx* ctx, const double* g, const double* s, const double* lam, const double* sigma_s, const double* rbar_s,
                    double* s2, double* b2, double* out /* 4 */);
int pk_slack_recover(pk_ctx* ctx, const double* dlam, const double* lam, const double* rbar_s, const double* s2,
                     const double* sigma_s, const double* dx, const double* w, const double* s1, double* ds, double* out /* 5 */);
int pk_slack_update(pk_ctx* ctx, int which, double* v, const double* dv, double* zl, const double* dzl, double* zu, const double* dzu,
                    double* lam /* or NULL */, const double* dlam /* or NULL */, double alpha_p, double alpha_d, double mu,
                    double kappa, double* out /* 4 */);

/* THE STEP'S SYSTEM FACTORED ON THE DEVICE: A BORDERED BAND LU (kernels pk_bd_init_k, pk_bd_fill_k, pk_bd_panel_k, pk_bd_update_k,
 * pk_bd_prep_k, pk_bd_solve_k, pk_bd_dot_k, pk_bd_border_k, pk_bd_xb_k, pk_bd_scatter_k of the library: one family that also serves
 * the batch and the block forms below; pk_band.cpp, DESIGN.md sections 23 and 28).  K = [[H + diag(s1), J^T], [J, -diag(s2)]]
 * over the free variables and all rows, permuted to [[B, U], [U^T, C]]: B (nb x nb) with half-bandwidth w in LAPACK's dgbtrf
 * storage (kl = ku = w, leading dimension 3 w + 1), U nb x p and C p x p column-major, w <= 192, p <= 8.
 * pk_band_plan uploads the plan once (it replaces an earlier one): order[k], k < nb + p, is the position in the caller's vectors
 * of n + m values of the unknown at permuted position k (the border last); map holds two source codes per stored slot of
 * [band | U | C] (0: none, +(e + 1): plus entry e of [hvals | jvals | s1 (n) | s2 (m)], -(e + 1): minus it; a slot is 0.0 plus its
 * sources in this order).  The CSR maps must be set: the sources are checked against their sizes.
 * pk_band_factor_dev fills the matrix from the resident arrays and factors B with partial pivoting inside the band (dgbtf2's
 * arithmetic, every product rounded before it is subtracted; the same bits every run).  pk_band_solve_dev solves K sol = rhs on
 * vectors of n + m values in the caller's order (fixed variables: rhs not read, sol 0.0).  Both enqueue on the context's stream
 * and wait for nothing.  pk_band_record copies the record of 8 doubles and synchronises: 0 status (0 solved, 1 singular band
 * pivot, 2 singular border, 3 non-finite); 1 the failing column in permuted numbering or -1; 2, 3 the smallest and largest
 * |pivot|; 4 nb; 5 w; 6 p; 7 the interchanges that moved a row.  After status != 0 sol is left untouched.  Pivoting never leaves
 * the band part: a K whose B is singular fails here though K is not.
 * pk_solve_banded is the host form on pk_linearize's values: one upload of b, s1 and s2, factor, solve, one download of x (left
 * untouched unless status is 0) and the record.
 * Errors: 110 a null device pointer; 119 a sharded context; 136 no device memory; 60 a null host buffer; 134 nb < 0, w or p beyond
 * the cap, an order or a map outside the system, factor or solve without a plan, solve or record without a factorisation; 117 an
 * operator of the host form that is not set; 118 no linearization with a Hessian.  Nothing is enqueued or written after a refusal. */
int pk_band_plan(pk_ctx* ctx, int64_t nb, int32_t w, int32_t p, const int32_t* order /* nb + p */, const int32_t* map /* 2 per slot */);
int pk_band_factor_dev(pk_ctx* ctx, const double* d_hvals, const double* d_jvals, const double* d_s1, const double* d_s2);
int pk_band_solve_dev(pk_ctx* ctx, const double* d_rhs, double* d_sol);
int pk_band_record(pk_ctx* ctx, double* rec /* 8 */);
int pk_solve_banded(pk_ctx* ctx, const double* s1, const double* s2, const double* b, double* x, double* rec /* 8 */);

/* A BATCH OF STEP SYSTEMS BEHIND ONE PLAN (the same ten kernels pk_bd_init_k ... pk_bd_scatter_k: the entry from the grid's second
 * dimension; DESIGN.md sections 24 and 28).  B systems, 1 <= B <= 16, share pk_band_plan's ordering, w, p and assembly map; each
 * has its own values.  Entry e is assembled, factored and solved exactly as the single forms do it: its solution and its record
 * are, bit for bit, those of pk_band_factor_dev / pk_band_solve_dev on entry e's inputs alone.  A batch costs the launches of one
 * system, each with B times the workgroups.  Strides are in doubles: entry e of an array begins e strides behind entry 0.  A
 * source stride of 0 means that all entries read the same array; otherwise it is at least the array's length (hvals and jvals: the
 * CSR value counts, s1: n, s2: m, rhs and sol: n + m).  An entry that fails (status != 0) does not stop the others: its slice of
 * sol is left untouched, theirs are complete.  The batch has its own arrays, reserved by the first call and grown by a larger B: a
 * batch call leaves the factors of pk_band_factor_dev in place and the other way round; a new plan invalidates both.
 * pk_band_solve_batch_dev and pk_band_record_batch take the B of the last pk_band_factor_batch_dev; the record of entry e is at
 * rec + 8 e.  pk_solve_banded_batch is the host form on pk_linearize's values (J and H shared by the entries): one upload of b,
 * s1, s2 (B rows each), one download of x and the records; the rows of x whose entry failed are left as the caller gave them.
 * Errors: 134 B outside 1 ... 16, a stride that is neither 0 nor at least the length, an output stride below the length, no
 * plan, CSR maps changed since the plan, a solve or a record without a batch factorisation of that B; 110 a null device pointer;
 * 60 a null host buffer; 119 a sharded context; 136 no device memory (the message names the array and B); the host form also 117
 * and 118 as pk_solve_banded.  Nothing is enqueued or written after a refusal. */
int pk_band_factor_batch_dev(pk_ctx* ctx, int32_t B, const double* d_hvals, int64_t stride_h, const double* d_jvals, int64_t stride_j,
                             const double* d_s1, int64_t stride_s1, const double* d_s2, int64_t stride_s2);
int pk_band_solve_batch_dev(pk_ctx* ctx, int32_t B, const double* d_rhs, int64_t stride_rhs /* 0 or >= n + m */, double* d_sol,
                            int64_t stride_sol /* >= n + m */);
int pk_band_record_batch(pk_ctx* ctx, int32_t B, double* rec /* 8 B: entry e at rec + 8 e */);
int pk_solve_banded_batch(pk_ctx* ctx, int32_t B, const double* s1 /* B x n */, const double* s2 /* B x m */,
                          const double* b /* B x (n + m) */, double* x /* B x (n + m) */, double* rec /* 8 B */);

/* MANY RIGHT-HAND SIDES AGAINST ONE FACTORISATION (the solve's six kernels pk_bd_prep_k, pk_bd_solve_k, pk_bd_dot_k,
 * pk_bd_border_k, pk_bd_xb_k, pk_bd_scatter_k with a column count of k; DESIGN.md sections 27 and 28).
 * pk_band_solve_multi_dev solves K sol_c = rhs_c for k right-hand sides,
 * 1 <= k <= 64, with the factors of the last pk_band_factor_dev, in the launches of ONE solve: right-hand side c is the n + m
 * doubles at d_rhs + c stride_rhs, its solution at d_sol + c stride_sol, both strides at least n + m.  The sweeps take one
 * workgroup per right-hand side; the border's columns of U are swept once per call and its Schur complement is formed and
 * factored once.  Column c has, bit for bit, the solution pk_band_solve_dev gives for column c alone, and the record is that
 * call's record; after a failed factorisation (status != 0) no column of d_sol is written; a column with an entry that is not
 * finite harms that column only.  Enqueued on the context's stream, not waited for.  pk_solve_banded_multi is the host form on
 * pk_linearize's values: one upload of b (k rows), s1 and s2, factor, the block solve, one download of x (left untouched unless
 * status is 0) and the record.
 * Errors: 110 a null device pointer; 119 a sharded context; 134 k outside 1 ... 64, a stride below n + m, no plan, no
 * factorisation; 136 no device memory (the message names the array and k); 60 a null host buffer; the host form also 117 and 118
 * as pk_solve_banded.  Nothing is enqueued or written after a refusal. */
int pk_band_solve_multi_dev(pk_ctx* ctx, int32_t k, const double* d_rhs, int64_t stride_rhs /* >= n + m */, double* d_sol,
                            int64_t stride_sol /* >= n + m */);
int pk_solve_banded_multi(pk_ctx* ctx, int32_t k, const double* s1, const double* s2, const double* b /* k x (n + m) */,
                          double* x /* k x (n + m) */, double* rec /* 8 */);

/* THE BAND SOLVE REFINED AGAINST THE TRUE K (kernels pk_bd_resid_k, pk_bd_refine_scalar_k, pk_bd_correct_k of the library;
 * pk_band_refine.cpp).  A solution of pk_band_solve_dev is measured against K as the CSR values state it -- q = K x
 * by pk_kkt_apply_dev's fixed-order application, r = b - q at the unknowns of the plan -- and corrected with the factors in place:
 * d = K^-1 r by the launches of one solve, x = x + d.  The device decides when to stop.
 * pk_band_refine_begin_dev is step 0: the product, the residual and the record.  The caller's six arrays must stay valid and
 * unchanged (d_sol: by the caller) until the refinement ends; d_sol is refined in place.  pk_band_refine_advance_dev enqueues
 * `steps` steps (solve, correction, product, residual, record).  Both enqueue on the context's stream and wait for nothing.
 * pk_band_refine_record copies the record of 8 doubles and synchronises: 0 status (0 running, 1 converged, 2 stalled, 3 a value
 * of r, x or b at an unknown is not finite, 4 the factorisation's own record is not 0: nothing is measured and d_sol is
 * untouched); 1 corrections applied; 2 |r|inf; 3 |x|inf; 4 |b|inf; 5 rho = |r|inf / (min(|x|inf, 1e6 |b|inf) + |b|inf), 0.0
 * when |r|inf is 0; 6 rho of step 0; 7 the rho before this one.  Behind step t: converged when t >= min_steps and rho <= tol;
 * otherwise stalled when t >= 1 and rho > (1 - 1e-9) rho_prev (the correction that did not help stays in d_sol).  Once the
 * status is not 0 further steps change neither d_sol nor the record: the result does not depend on how many steps were enqueued
 * beyond the stop (each surplus step still costs its solve and its product).  A new plan or a new pk_band_factor_dev ends the
 * refinement.  pk_solve_banded_refined is the host form on pk_linearize's values: uploads, factor, solve, begin, then one step
 * at a time behind a read of the record until the status is not 0 or max_steps are done (status 5, exhausted, in the host copy
 * rrec only); x comes down unless the band's status (rec) is not 0.
 * Errors: 110 a null device pointer; 117 a CSR operator of J, J^T or H is not set; 119 a sharded context; 134 no plan or no
 * factorisation, tol negative or not finite, min_steps or max_steps outside 0 ... 10, steps < 1; 135 advance or record without
 * a begin; 136 no device memory (the message names the array); 60 a null host buffer; the host form also 118.  Nothing is
 * enqueued or written after a refusal. */
#define PK_BAND_REFINE_TOL 1.0e-10          /* the tolerance on rho the solver's loop passes */
#define PK_BAND_REFINE_SINGULAR 1.0e-5      /* a final rho above this: the system counts as singular for this solve */
#define PK_BAND_REFINE_MAX_STEPS 10         /* the most steps of one refinement */
int pk_band_refine_begin_dev(pk_ctx* ctx, const double* d_hvals, const double* d_jvals, const double* d_s1, const double* d_s2,
                             const double* d_rhs, double* d_sol, double tol, int32_t min_steps);
int pk_band_refine_advance_dev(pk_ctx* ctx, int32_t steps);
int pk_band_refine_record(pk_ctx* ctx, double* rec /* 8 */);
int pk_solve_banded_refined(pk_ctx* ctx, const double* s1, const double* s2, const double* b, double* x, double* rec /* 8 */,
                            double* rrec /* 8 */, double tol, int32_t min_steps, int32_t max_steps);

#ifdef __cplusplus
}
#endif
#endif /* POCKIT_HIP_H */
