/* blsq.h — C-ABI of the MI355X trust-region step solver (libblsq_hip.so).
 *
 * Drop-in boundary for ONE path of nmayorov/bounded-lsq: the per-iteration
 * linear algebra its `trf` and `dogbox` drivers run between two fun/jac
 * callbacks.  The reference is pure Python; what a maintainer would bind is
 * this library through ctypes.  Each entry point cites
 * the reference code it replaces (paths under the reference repo).
 *
 * Conventions
 *   - all arrays float64, C-contiguous, batch-major: J is B x m x n exactly as
 *     numpy hands it over, vectors are B x n (or B x m for f), masks int64;
 *   - the caller owns every buffer passed in; outputs are caller-allocated;
 *     the library owns device memory and the factor state inside a plan;
 *   - return value: 0 ok; <0 invalid argument (-(index of the argument),
 *     1-based); >0 a hipError_t.  blsq_last_error() gives the text.  Nothing
 *     throws across the ABI.  Per-problem numerical conditions the reference
 *     signals with ValueError (trust_region.py:28-29,34-35) are reported in
 *     status[b] (BLSQ_STATUS_*);
 *   - a ctx is bound to one device and one HIP stream and is NOT thread-safe;
 *     calls taking host pointers are blocking, `_dev` calls are asynchronous
 *     on the ctx stream (blsq_sync to wait).
 */
#ifndef BLSQ_H
#define BLSQ_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct blsq_ctx blsq_ctx;
typedef struct blsq_trf_plan blsq_trf_plan;
typedef struct blsq_dogbox_plan blsq_dogbox_plan;
typedef struct blsq_cov_plan blsq_cov_plan;

enum {
  BLSQ_STATUS_OK = 0,
  BLSQ_STATUS_ZERO_DIRECTION = 1,  /* intersect_trust_region: "`s` is zero."  (trust_region.py:28-29) */
  BLSQ_STATUS_OUTSIDE_TR = 2       /* "`x` is not within the trust region."  (trust_region.py:34-35) */
};
enum {                     /* how `scale` is treated by *_factor */
  BLSQ_SCALE_GIVEN = 0,    /* numeric `scaling`: scale = 1/scaling, unchanged          */
  BLSQ_SCALE_JAC_INIT = 1, /* scale = 1/||J[:,j]||, zero norm -> 1   (trf.py:216-219, dogbox.py:141-144) */
  BLSQ_SCALE_JAC_UPDATE = 2/* scale = min(scale, 1/||J[:,j]||)        (trf.py:239-242, dogbox.py:165-168) */
};

int blsq_version(void);
int blsq_device_count(void);

int blsq_ctx_create(int device_id, blsq_ctx** out);
int blsq_ctx_destroy(blsq_ctx* ctx);
const char* blsq_last_error(const blsq_ctx* ctx);
int blsq_sync(blsq_ctx* ctx);

/* Run-time switches: ONE table inside the library (csrc/blsq_options.cpp; INTEGRATION.md lists it).  A ctx reads every
 * switch ONCE, at blsq_ctx_create, from the environment variable the table names; afterwards only blsq_ctx_set_option
 * changes it, for that ctx alone.  Route switches (gram, cqr2, csne, optimistic, no_svdfree, svdfree_min_n, gram_k2_max)
 * take effect for plans created afterwards, the others at the next call.  `name` is the table's key or its environment
 * variable's name.  No switch loosens a proven gate (gram_k2_max can only tighten).  blsq_option_info: i in
 * [0, blsq_option_count()). */
int blsq_option_count(void);
int blsq_option_info(int i, const char** name, const char** env, double* default_value, const char** doc);
int blsq_ctx_set_option(blsq_ctx* ctx, const char* name, double value);
int blsq_ctx_get_option(const blsq_ctx* ctx, const char* name, double* value);

/* device memory helpers (so hosts need not bind the HIP runtime themselves) */
int blsq_dev_malloc(blsq_ctx* ctx, size_t bytes, void** dptr);
int blsq_dev_free(blsq_ctx* ctx, void* dptr);
int blsq_memcpy_h2d(blsq_ctx* ctx, void* dst, const void* src, size_t bytes);
/* Page-locked host memory for the buffers handed to the host-pointer calls (blsq_trf_factor, blsq_dogbox_factor):
 * a `jac` callback (least_squares.py:367-371) that writes J into such a buffer has it DMA'd to the GPU at link
 * speed, in sub-batches of problems overlapped with the Gram of the previous sub-batch; pageable buffers work too
 * (the runtime stages them). */
int blsq_host_alloc(blsq_ctx* ctx, size_t bytes, void** hptr);
int blsq_host_free(blsq_ctx* ctx, void* hptr);
int blsq_memcpy_d2h(blsq_ctx* ctx, void* dst, const void* src, size_t bytes);

/* per-kernel device timing (HIP events on the ctx stream, for bench.py).  on: 0 off; 1 every kernel slot (two events
 * around every launch: they cost the step they measure about 2 %); 2 + s: slot s only (its index in blsq_timing_get) */
int blsq_timing_enable(blsq_ctx* ctx, int on);
int blsq_timing_reset(blsq_ctx* ctx);
int blsq_timing_count(const blsq_ctx* ctx);                    /* number of kernel slots */
int blsq_timing_get(blsq_ctx* ctx, int slot, const char** name, double* total_ms,
                    int64_t* launches);

/* ------------------------------------------------------------------ TRF --
 * blsq_trf_factor  replaces trf.py:244-277 (+ :216-219 / :239-242 for 'jac'):
 *   g = J^T f, Coleman-Li v/d/g_h/diag_h, g_norm, theta, and the factorisation
 *   the reference gets from svd(J_augmented) (trf.py:264-274).  Once per outer
 *   iteration.
 * blsq_trf_step    replaces trf.py:284-308 (+ the norm/correction terms of
 *   :318-331 the driver needs): solve_lsq_trust_region, feasibility test,
 *   reflected / gradient steps, model evaluation and selection, x_new.  Once
 *   per inner iteration with a new Delta / alpha, WITHOUT refactorising.
 */
int blsq_trf_plan_create(blsq_ctx* ctx, int B, int m, int n, blsq_trf_plan** out);
int blsq_trf_plan_destroy(blsq_trf_plan* plan);

int blsq_trf_factor(blsq_trf_plan* plan, const double* J, const double* f, const double* x,
                    const double* lb, const double* ub, double* scale_io, int scale_mode,
                    double* g /*B*n*/, double* g_norm /*B*/, double* theta /*B*/);
int blsq_trf_step(blsq_trf_plan* plan, const double* Delta /*B*/, double* alpha_io /*B*/,
                  double active_rtol, double* step_h /*B*n*/, double* step /*B*n*/,
                  double* x_new /*B*n*/, int64_t* hits /*B*n*/, int64_t* active_new /*B*n*/,
                  double* predicted_reduction /*B*/, double* step_h_norm /*B*/,
                  double* correction /*B*/, int32_t* n_iter /*B*/, int32_t* branch /*B*/,
                  int32_t* status /*B*/);

/* device-pointer variants: inputs already resident in HBM, results stay in
 * plan-owned device buffers until fetched.
 * blsq_trf_factor_dev (and blsq_dogbox_factor_dev, with blsq_dogbox_step_dev) is asynchronous all the way: it does not wait for the per-problem verdict of the
 * conditioning certificate (which problems must take the Householder route) but assumes the common one
 * — "none" — and the NEXT call on the plan reads the verdict: blsq_trf_step_dev enqueues its kernels
 * first and, should the guess have been wrong, runs the Householder stage and the step once more
 * (same results either way).  LIFETIME RULE for the caller: dJ / df / dscale_io must stay valid AND
 * unmodified until the verdict has been read — by the next blsq_*_step_dev / blsq_*_fetch_* call on the
 * plan, or by blsq_sync(ctx), which resolves every pending verdict of the ctx (so does blsq_dev_free and
 * blsq_memcpy_h2d: memory handed back to, or overwritten through, the library is never read afterwards).
 * After blsq_sync nothing of the caller's J / f is read again — EXCEPT by blsq_trf_step_dev while the plan holds problems
 * on the CSNE tier (ill-conditioned TRF problems of 80 <= n <= 256; blsq_debug_csne_stats below): their steps are
 * corrected against J itself, so dJ / df must then stay valid and unmodified until the next factor call on the plan
 * (option `csne` = 0 restores the unconditional rule).  A second *_factor_dev on the plan drops
 * the first one's verdict (it is still read for the path statistics).  Option `optimistic` = 0 (environment
 * BLSQ_OPTIMISTIC=0 at blsq_ctx_create): the factor call waits itself and the rule is void. */
int blsq_trf_factor_dev(blsq_trf_plan* plan, const double* dJ, const double* df,
                        const double* dx, const double* dlb, const double* dub,
                        double* dscale_io, int scale_mode);
int blsq_trf_step_dev(blsq_trf_plan* plan, const double* dDelta, const double* dalpha_in,
                      double active_rtol);
int blsq_trf_fetch_factor(blsq_trf_plan* plan, double* g, double* g_norm, double* theta,
                          double* scale, double* sing /*B*n, unsorted, may be NULL*/);
int blsq_trf_fetch_step(blsq_trf_plan* plan, double* alpha_out, double* step_h, double* step,
                        double* x_new, int64_t* hits, int64_t* active_new,
                        double* predicted_reduction, double* step_h_norm, double* correction,
                        int32_t* n_iter, int32_t* branch, int32_t* status,
                        double* p_h_tr /*may be NULL*/, double* to_bound /*may be NULL*/,
                        int32_t* choice /*may be NULL*/);

/* diagnostics: in-kernel phase stamps of the QR kernel (only a -DBLSQ_QR_STAMPS
 * build writes them): 8 doubles per workgroup into the given device buffer */
int blsq_debug_qr_stamps(void* dbuf);

/* diagnostics: 1 where the last factor call chose the SVD-free trust-region path
 * (full-rank gate passed), 0 where it went through the Jacobi SVD */
int blsq_trf_debug_fast(blsq_trf_plan* plan, int32_t* fast /*B*/);
int blsq_dogbox_debug_fast(blsq_dogbox_plan* plan, int32_t* fast /*B*/);

/* diagnostics: the conditioning certificate of the last factor call, per problem: the PROVEN upper
 * bound K2 >= kappa_2 of the equilibrated system the step is solved from on the normal-equations
 * path (0 where no bound was computed: front end off, or a Cholesky pivot failed before).  A
 * problem stays on that path iff K2 <= 2.5e5. */
int blsq_trf_debug_cond(blsq_trf_plan* plan, double* k2 /*B*/);
int blsq_dogbox_debug_cond(blsq_dogbox_plan* plan, double* k2 /*B*/);

/* diagnostics: Jacobi sweeps used by the last factor call, per problem (dogbox: meaningful where
 * blsq_dogbox_debug_fast gives 0; the kernel writes 0 for a problem it does not decompose) */
int blsq_trf_debug_sweeps(blsq_trf_plan* plan, int32_t* sweeps /*B*/);
int blsq_dogbox_debug_sweeps(blsq_dogbox_plan* plan, int32_t* sweeps /*B*/);

/* --------------------------------------------------------------- dogbox --
 * blsq_dogbox_factor replaces dogbox.py:165-199: gradient, active/free split,
 *   gtol quantity, Gauss-Newton step lstsq(J_free,-f) and the Cauchy step.
 * blsq_dogbox_step   replaces dogbox.py:203-220 (+ :235): dogleg_step /
 *   constrained_cauchy_step, predicted reduction (with the reference's
 *   not-recomputed-Js quirk, :216), scatter to x_new, new on_bound.
 */
int blsq_dogbox_plan_create(blsq_ctx* ctx, int B, int m, int n, blsq_dogbox_plan** out);
int blsq_dogbox_plan_destroy(blsq_dogbox_plan* plan);

int blsq_dogbox_factor(blsq_dogbox_plan* plan, const double* J, const double* f,
                       const double* x, const double* lb, const double* ub, double* scale_io,
                       int scale_mode, const int64_t* on_bound, double* g /*B*n*/,
                       uint8_t* active_set /*B*n*/, double* g_norm /*B*/,
                       int32_t* all_active /*B*/);
int blsq_dogbox_step(blsq_dogbox_plan* plan, const double* Delta /*B*/, double* step /*B*n*/,
                     double* x_new /*B*n*/, int64_t* on_bound_new /*B*n*/, uint8_t* tr_hit /*B*/,
                     double* predicted_reduction /*B*/, double* step_scaled_norm /*B*/,
                     uint8_t* fallback /*B*/, int32_t* status /*B*/);

int blsq_dogbox_factor_dev(blsq_dogbox_plan* plan, const double* dJ, const double* df,
                           const double* dx, const double* dlb, const double* dub,
                           double* dscale_io, int scale_mode, const int64_t* don_bound);
int blsq_dogbox_step_dev(blsq_dogbox_plan* plan, const double* dDelta);
int blsq_dogbox_fetch_factor(blsq_dogbox_plan* plan, double* g, uint8_t* active_set,
                             double* g_norm, int32_t* all_active, double* scale,
                             double* newton_full /*B*n, may be NULL*/,
                             double* cauchy_full /*B*n, may be NULL*/);
int blsq_dogbox_fetch_step(blsq_dogbox_plan* plan, double* step, double* x_new,
                           int64_t* on_bound_new, uint8_t* tr_hit,
                           double* predicted_reduction, double* step_scaled_norm,
                           uint8_t* fallback, int32_t* status);

/* ------------------------------------------------------ tall problem / comm --
 * Row-block partition of ONE very tall problem across the GPUs of a node, one process (rank) per
 * GPU (the reference has no counterpart — it would call svd on the whole matrix,
 * trf.py:272).  The collective is the library's own: RCCL over xGMI, bound at run time (dlopen),
 * enqueued on the ctx stream between the local and the replicated kernels.
 *
 *   blsq_comm_get_id   rank 0 makes the rendezvous id (ncclUniqueId, blsq_comm_id_bytes() bytes);
 *                      the HOST distributes it to the other ranks (any channel: a TCP socket,
 *                      MPI, a file, torch.distributed — bounded_lsq._multi has a socket helper)
 *   blsq_comm_init     every rank, collectively: communicator of `nranks` ranks on the ctx device
 *   blsq_tsqr_plan_create / blsq_tsqr_factor_dev / blsq_trf_step_dev / blsq_trf_fetch_step
 *
 * blsq_tsqr_factor_dev takes THIS rank's row block [J_r f_r] and leaves the same factor state on
 * every rank (so every rank computes the same step, redundantly):
 *   - normal-equations front end: local Gram, ONE ncclAllReduce(sum) of the (n+1)^2 Gram (n = 128:
 *     166 KB: "all-reduce of R" in north_star's words), replicated Cholesky + conditioning gate;
 *   - a problem the gate rejects: local Householder TSQR, ONE ncclAllGather of the (n+1)^2
 *     triangles, every rank merges the stack.
 * m_total (all ranks' rows) enters the reference's rank test eps * m * s[0] (trust_region.py:109).
 * blsq_tsqr_local_dev / blsq_tsqr_combine_dev expose the two halves of the Householder route for
 * hosts that exchange the triangles themselves (`tri` buffers: dense row-major
 * blsq_tsqr_tri_ld(n)^2 doubles, stack in rank order).
 * Every rank takes the SAME route: the gate's verdict is compared over the ranks (one 16-byte
 * ncclAllReduce(max) behind the Gram's) and the call fails with BLSQ_ERR_RANKS_DISAGREE on every rank
 * if they differ (x / bounds / scale / scale_mode / BLSQ_* environment must be identical everywhere).
 * Return codes of failed RCCL calls: 10000 + ncclResult_t.
 * The collective library is resolved at the first blsq_comm_* call: $BLSQ_RCCL_PATH if set (a full
 * path to a librccl-compatible shared object; tests/ use it for a socket-based stand-in that lets two
 * processes share ONE GPU, which RCCL itself refuses), otherwise librccl.so.1 next to the HIP runtime
 * the process already uses, then the loader's search path.  blsq_comm_library() reports the choice.
 */
#define BLSQ_ERR_RANKS_DISAGREE 20001
/* path of the collective library in use ("" before the first blsq_comm_* call) and its
 * ncclGetVersion() code (0 if the library has no such entry) */
const char* blsq_comm_library(int* version_out);
int blsq_comm_id_bytes(void);
int blsq_comm_get_id(blsq_ctx* ctx, void* id_out, size_t bytes);
int blsq_comm_init(blsq_ctx* ctx, int nranks, int rank, const void* id, size_t bytes);
int blsq_comm_destroy(blsq_ctx* ctx);
int blsq_comm_size(const blsq_ctx* ctx);
int blsq_comm_rank(const blsq_ctx* ctx);
/* max over the ranks of n <= 64 host doubles, in place; doubles as a barrier (bench timing) */
int blsq_comm_allreduce_max(blsq_ctx* ctx, double* host_io, int n);

int blsq_tsqr_tri_ld(int n);
int blsq_tsqr_plan_create(blsq_ctx* ctx, int m_local, long long m_total, int n, int nranks,
                          blsq_trf_plan** out);
int blsq_tsqr_factor_dev(blsq_trf_plan* plan, const double* dJ_block, const double* df_block,
                         const double* dx, const double* dlb, const double* dub,
                         double* dscale_io, int scale_mode);
int blsq_tsqr_local_dev(blsq_trf_plan* plan, const double* dJ_block, const double* df_block,
                        double* dtri_out);
int blsq_tsqr_combine_dev(blsq_trf_plan* plan, const double* dtri_stack /*nranks tris*/,
                          const double* dx, const double* dlb, const double* dub,
                          double* dscale_io, int scale_mode);

/* diagnostics: number of 16-column QR panels factored by the Cholesky-QR + Householder-
 * reconstruction fast path (out[0]) and by the exact Householder column loop (out[1]: partial
 * last panels and panels whose scaled Gram has a small pivot) since the last reset. */
int blsq_debug_cqr_stats(blsq_ctx* ctx, uint64_t out[2], int reset);
/* Diagnostics: of the problems the gate handed on (out[1] of blsq_debug_gram_stats), how many the CholeskyQR2
 * middle tier factored (second pass over J through the MFMA pipe, proven acceptance test)
 * instead of the Householder tree, since the last reset.  Synchronises the ctx stream. */
int blsq_debug_cqr2_stats(blsq_ctx* ctx, uint64_t* out1, int reset);
/* Diagnostics of the CSNE tier (corrected semi-normal equations, DESIGN.md 3.0d: a rejected problem of 80 <= n <= 256
 * keeps its Gram-Cholesky factor as a preconditioner and every step-solve corrects the trust-region solution against J
 * itself in ONE streaming pass; replaces what the reference gets from svd(J_augmented), trf.py:272-274 +
 * trust_region.py:111-150, for such a problem): out[0] = problems factor calls routed to the tier, out[1] = step-solves
 * it delivered, out[2] = step-solves it declined (measured correction above its bound: the problem went on to
 * CholeskyQR2 / the Householder tree in that step call), since the last reset.
 * LIFETIME RULE of the tier: while a plan holds problems on it (blsq_debug_csne_stats out[0] grows), blsq_trf_step_dev
 * READS the dJ / df of the last blsq_trf_factor_dev: they must stay valid and unmodified until the next factor call on
 * the plan (the reference's drivers keep J for exactly that long, trf.py:283-352).  BLSQ_CSNE=0 switches the tier off. */
int blsq_debug_csne_stats(blsq_ctx* ctx, uint64_t out[3], int reset);
/* ... per problem: on_tier[b] = 1 while problem b is on the tier; eta[b] = the largest first-order correction the last
 * step call measured for it (the quantity its acceptance bounds: <= 1e-7), -1 where the tier declined.  Either may be NULL. */
int blsq_trf_debug_csne(blsq_trf_plan* plan, int32_t* on_tier /*B*/, double* eta /*B*/);
/* Diagnostics: on != 0 makes every later launch of this ctx run the blocked triangular solves of the trust-region tail
 * (n > 80) in their three-barrier reference schedule instead of the look-ahead schedule; 0 (the state of a new ctx)
 * switches back.  Both give the same bits; the tests compare them. */
int blsq_debug_tri_reference(blsq_ctx* ctx, int on);
/* Diagnostics: on != 0 makes every later 16-tile Gram launch of this ctx (n = 256) stage its rows through registers even
 * where it qualifies for the LDS-DMA staging (16-byte aligned J and f, even strides and row count); 0 (the state of a
 * new ctx) switches back.  Both give the same bits; the tests compare them. */
int blsq_debug_gram_regstage(blsq_ctx* ctx, int on);
/* Diagnostics of the factorisation front end: out[0] = problems factored by the
 * normal-equations fast path (Gram + equilibrated Cholesky, conditioning-gated), out[1] =
 * problems the gate handed to the Householder TSQR tree, since the last reset. */
int blsq_debug_gram_stats(blsq_ctx* ctx, uint64_t out[2], int reset);
/* Diagnostics: what the Gram launch of a batch of B problems of m x n does — decided on the host before anything is
 * launched, so this needs no device (ctx: whose switches to read; NULL: the table's defaults).  has_final: the caller
 * offers the final slot (a launch may then fuse the reduction of two row chunks).  out[0] family (0 direct, 1 gram8,
 * 2 gram1, 3 gram16, 4 generic), out[1..3] its template key (direct: NTT, RHS, NWD; gram8: RHS; gram16: RHS, PAIR;
 * generic: SLOTS, NCB), out[4..6] grid, out[7] block, out[8] dynamic LDS bytes, out[9] rhs_valu, out[10]
 * rows_per_chunk, out[11] tile groups, out[12] reduction fused, out[13] row chunks; out[14..15] zero.  A problem's
 * summation order follows from the family, the key, rhs_valu and rows_per_chunk: none of them depends on B.
 * Returns non-zero for a shape the Gram front end does not take. */
int blsq_debug_gram_route(const blsq_ctx* ctx, int m, int n, int B, int has_final, int32_t out[16]);

/* Diagnostics: measured peaks of the device the ctx is bound to ("confirm on the
 * box with a copy kernel and an MFMA-f64 probe").
 *   kind 0: FP64 MFMA probe — every SIMD issues independent v_mfma_f64_16x16x4_f64 back to back on
 *           register operands (`arg` waves per SIMD, 1 or 2); out[0] = TFLOP/s, out[1] = number of
 *           MFMA wave-instructions executed, out[2] = milliseconds (HIP events).  The same launch
 *           calibrates the SQ MFMA counters (tools/pmc_mfma.py).
 *   kind 1: streaming copy of `arg` MiB (device to device, 16 B per lane); out[0] = GB/s counting
 *           bytes read + bytes written, out[1] = bytes moved, out[2] = milliseconds. */
int blsq_debug_probe(blsq_ctx* ctx, int kind, int arg, double out[3]);

/* ---- batched outer trust-region drivers, device-resident ------------------
 * Replaces, for B problems of one shape advancing in lock-step, the Python loops around the
 * step path: trf.py:173-237 (initialisation), :238-261 (top of the outer loop: nfev / gtol
 * checks), :309-358 (ratio test, Delta / alpha update, ftol / xtol tests, accept) and
 * dogbox.py:100-163, :164-194, :221-272.  x, f, J and every per-problem scalar stay on the
 * device; only the callbacks' inputs/outputs (device buffers owned by the driver) and ONE
 * integer per call (active / accepted problems) are visible to the host.
 *
 *   create -> buffers -> start(x0,lb,ub,scale,...)
 *   caller:  f  <- fun(x),  J <- jac(x)            (into the driver's buffers)
 *   begin                                          first factorisation, Delta_0
 *   loop:  propose(&n_active)   if n_active == 0: stop
 *          caller: f_trial <- fun(x_trial)
 *          judge(&n_accepted)
 *          caller: J[b] <- jac(x[b]) for the problems with accepted[b] != 0   (if n_accepted)
 *   fetch(...)
 * Per-problem results (x, nfev, njev, status, ...) are what the reference's driver returns for
 * that problem alone; a terminated problem is frozen.  A problem whose step reports a
 * BLSQ_STATUS_* condition (where the reference raises ValueError and aborts the solve,
 * trust_region.py:28-29,34-35) is frozen at its current x with status = -BLSQ_STATUS_*.
 * method: 0 = 'trf', 1 = 'dogbox'. */
typedef struct blsq_outer blsq_outer;
int blsq_outer_create(blsq_ctx* ctx, int method, int B, int m, int n, blsq_outer** out);
int blsq_outer_destroy(blsq_outer* o);
/* Device buffers read / written by the callbacks (any pointer argument may be NULL):
 * x [B][n] current points, x_trial [B][n], f [B][m] residuals at x, f_trial [B][m],
 * J [B][m][n] Jacobians at x, accepted [B] int32 flags set by blsq_outer_judge. */
int blsq_outer_buffers(blsq_outer* o, double** x, double** x_trial, double** f, double** f_trial,
                       double** J, int32_t** accepted);
/* Host inputs, all [B][n]: x0 (as given by the user), x_start (x0 moved strictly inside the
 * bounds for 'trf', trf.py:201; == x0 for 'dogbox'), lb, ub, scale (= 1/scaling, or ones with
 * jac_scaling != 0).  max_nfev > 0.  Uploads and resets the state; afterwards buffer `x` holds
 * x_start. */
int blsq_outer_start(blsq_outer* o, const double* x0, const double* x_start, const double* lb,
                     const double* ub, const double* scale, int jac_scaling, double ftol,
                     double xtol, double gtol, int max_nfev);
int blsq_outer_begin(blsq_outer* o);
int blsq_outer_propose(blsq_outer* o, int32_t* n_active);
int blsq_outer_judge(blsq_outer* o, int32_t* n_accepted);
/* Host outputs (any may be NULL): x [B][n], f [B][m], obj [B], optimality [B], on_bound [B][n]
 * (dogbox's final mask; zeros for 'trf' whose mask the caller derives from x, trf.py:257),
 * nfev, njev, status [B]. */
int blsq_outer_fetch(blsq_outer* o, double* x, double* f, double* obj, double* optimality,
                     int64_t* on_bound, int32_t* nfev, int32_t* njev, int32_t* status);

/* ---- finite-difference Jacobians for the batched drivers, on the device ----
 * jac='2-point' / '3-point' of the reference is the THIRD-PARTY call
 * scipy.optimize._numdiff.approx_derivative(fun, x, rel_step=diff_step, method=jac, f0=f,
 * bounds=bounds) (least_squares.py:357-365; restated against scipy 1.15.3: _compute_absolute_step,
 * _adjust_scheme_to_bounds, _dense_difference).  For B problems at once:
 *   blsq_fd_points_dev    steps h [B][n], one-sided flags [B][n] and the perturbed points
 *                         X [B][P][n] (P = n for method 2, 2n for method 3) which the caller's
 *                         `fun` evaluates in one batched call into F [B][P][m];
 *   blsq_fd_assemble_dev  J [B][m][n] from f0 [B][m] and F (problems with mask[b] == 0 are left
 *                         untouched when mask != NULL).
 * All pointers are device pointers; rel_step is NULL (scipy's default step) or [n].
 * method: 2 = '2-point', 3 = '3-point'. */
int blsq_fd_points_dev(blsq_ctx* ctx, int B, int n, int method, const double* dx,
                       const double* dlb, const double* dub, const double* drel_step, double* dX,
                       double* dh, uint8_t* done_sided);
int blsq_fd_assemble_dev(blsq_ctx* ctx, int B, int m, int n, int method, const double* dx,
                         const double* dh, const uint8_t* done_sided, const double* df0,
                         const double* dF, double* dJ, const int32_t* dmask);

/* ---- robust loss functions (scipy.optimize.least_squares `loss=`, `f_scale=`) ----------------------------------
 * The reference minimises sum f^2 only.  Its successor, scipy.optimize.least_squares (1.15.3), adds a robust loss on
 * top of the same trf / dogbox drivers by transforming the INPUTS of each step; the step path itself is unchanged.
 * Losses in scipy's IMPLEMENTED_LOSSES order (_lsq/least_squares.py: huber, soft_l1, cauchy, arctan); append only. */
enum { BLSQ_LOSS_LINEAR = 0, BLSQ_LOSS_HUBER, BLSQ_LOSS_SOFT_L1, BLSQ_LOSS_CAUCHY, BLSQ_LOSS_ARCTAN };
/* obj[b] = f_scale[b]^2 * sum_i rho0((f[b][i] / f_scale[b])^2): the objective of problem b (scipy
 * _lsq/least_squares.py construct_loss_function, cost_only, WITHOUT its factor 1/2: 'linear' with f_scale = 1 is
 * ||f||^2, the convention of every `obj` here).  Fixed summation order: a problem's bits do not depend on B or on
 * its batch mates.  Problems with dmask[b] == 0 are skipped (dmask may be NULL).  Device pointers; f_scale [B] > 0. */
int blsq_loss_cost_dev(blsq_ctx* ctx, int B, int m, int loss, const double* df_scale, const double* df,
                       double* dobj, const int32_t* dmask);
/* For the problems with dmask[b] != 0 (dmask may be NULL: all), scipy _lsq/common.py
 * scale_for_robust_loss_function: w_i = sqrt(max(rho1 + 2 rho2 f_i^2, EPS)) (rho of construct_loss_function, with
 * rho2 /= f_scale^2), J[b] <- diag(w) J[b] IN PLACE (dJ_io [B][m][n]) and df_scaled[b][i] = f_i * (rho1 / w_i)
 * ([B][m]; df itself is not written).  Applying it twice scales J twice: call it once per fresh Jacobian. */
int blsq_loss_scale_dev(blsq_ctx* ctx, int B, int m, int n, int loss, const double* df_scale, const double* df,
                        double* dJ_io, double* df_scaled, const int32_t* dmask);
/* Robust loss of a device-resident outer driver (scipy _lsq/trf.py trf_bounds / trf_no_bounds and _lsq/dogbox.py:
 * the loss cost in the ratio test, scale_for_robust_loss_function after every Jacobian).  Call before
 * blsq_outer_start (any other order is an argument error); the default after create is BLSQ_LOSS_LINEAR, for which
 * nothing is launched.  f_scale: [B] host, each > 0 (may be NULL for BLSQ_LOSS_LINEAR).  With another loss:
 *   - blsq_outer_begin scales every J, blsq_outer_propose scales the J of the problems with accepted[b] != 0 (the
 *     jac callback after a judge writes J[b] of THOSE problems only: the others hold their scaled Jacobian);
 *   - buffer `f` keeps the true residuals (callbacks write them, blsq_outer_fetch returns them); the scaled ones
 *     live in a driver-owned buffer; buffer `J` holds diag(w) J (scipy's result `jac`);
 *   - `obj` is f_scale^2 * sum rho0, as blsq_loss_cost_dev.
 * Both the scaled J and the scaled f stay unmodified from a factor call to the next one, as the CSNE tier's
 * lifetime rule asks. */
int blsq_outer_set_loss(blsq_outer* o, int loss, const double* f_scale);

/* ---- built-in fit models, evaluated on the device ---------------------------------------------------------------
 * The callbacks of a curve fit (blsq_outer_*: f <- fun(x), J <- jac(x)) for five closed-form model families, so that a
 * whole batched fit stays on the GPU.  Parameter order is fixed; a constant offset c is always last:
 *   POLY         sum_{k<n} p_k t^k                                              any n >= 1      coords 1
 *   EXP_SUM      sum_k a_k exp(-r_k t) + c          (a_1, r_1, ..., c)          n = 2K + 1      coords 1
 *   GAUSS_SUM    sum_k a_k exp(-z_k^2 / 2) + c      z_k = (t - mu_k) / s_k      n = 3K + 1      coords 1
 *                                                   (a_1, mu_1, s_1, ..., c)
 *   LORENTZ_SUM  sum_k a_k / (1 + z_k^2) + c        same parameters             n = 3K + 1      coords 1
 *   GAUSS2D      a exp(-((u-u0)^2 + (v-v0)^2) / (2 s^2)) + c   (a, u0, v0, s, c)   n = 5        coords 2, t is [2][m]
 * Append only.  n <= BLSQ_MODEL_MAX_N.
 * blsq_model_info: the name and the rule for n (n_per_term == 0: n == n_base; otherwise n = n_base + K n_per_term,
 * K >= 1); any output may be NULL; needs no device.  Non-zero for an unknown model. */
enum { BLSQ_MODEL_POLY = 0, BLSQ_MODEL_EXP_SUM, BLSQ_MODEL_GAUSS_SUM, BLSQ_MODEL_LORENTZ_SUM, BLSQ_MODEL_GAUSS2D };
#define BLSQ_MODEL_MAX_N 64
int blsq_model_count(void);
int blsq_model_info(int model, const char** name, int* coords, int* n_base, int* n_per_term);
/* For the points P [B * reps][n] (the points of problem b are rows b * reps .. b * reps + reps - 1; reps > 1 serves the
 * finite-difference points of blsq_fd_points_dev):
 *   f[q][i]    = w[b][i] * (model(t[b][.., i]; P[q]) - y[b][i])        df [B * reps][m], or NULL
 *   J[q][i][j] = w[b][i] * d model / d p_j                             dJ [B][m][n], or NULL; reps must be 1
 * dt: [coords][m] shared by all problems (t_stride 0) or [B][coords][m] (t_stride coords * m); dy: [B][m] or NULL (0:
 * plain prediction); dw: NULL (1), [m] (w_stride 0) or [B][m] (w_stride m); dmask: int32 [B] or NULL: a problem with
 * dmask[b] == 0 is left untouched in both outputs (the jac callback under a robust loss, blsq_outer_set_loss).
 * Nothing is checked on the device: non-finite values (s = 0) pass through as IEEE arithmetic gives them.  All pointers
 * are device pointers; asynchronous on the ctx stream.  A negative return is the index of the bad argument. */
int blsq_model_eval_dev(blsq_ctx* ctx, int model, int B, int reps, int m, int n, const double* dt, long t_stride,
                        const double* dy, const double* dw, long w_stride, const double* dP, double* df, double* dJ,
                        const int32_t* dmask);
/* The same model through a parameter map (fixed and tied parameters of a curve fit): the n parameters of the model are a
 * function of nf <= n solver variables X [B * reps][nf] and a per-problem template Pfix [B][n],
 *   P_full[q][j] = X[q][pmap[j]]   if pmap[j] >= 0,      Pfix[b][j]   if pmap[j] == -1            (q = b * reps + r)
 *   f[q][i]    = the f of blsq_model_eval_dev at P_full[q], bit for bit                            df [B * reps][m]
 *   J[q][i][k] = sum over {j : pmap[j] == k}, in ascending j, of the J[q][i][j] of blsq_model_eval_dev at P_full[q]:
 *                the first column of a slot is stored and the later ones are added to it, a sequential float64 sum;
 *                columns with pmap[j] == -1 are dropped                                            dJ [B][m][nf]
 * pmap: HOST pointer, int32 [n], read during the call (it travels in the kernel arguments: no device buffer); every
 * entry in -1 .. nf - 1 and every k < nf used by at least one j.  The identity (nf == n, pmap[j] == j) is accepted.
 * dPfix may be NULL when no entry is -1; where pmap[j] >= 0 its column j is not read.  Everything else as
 * blsq_model_eval_dev.  A negative return is the index of the bad argument (ctx = 1, model, B, reps, m, n, nf = 7,
 * pmap = 8, t, t_stride, y, w, w_stride, X = 14, Pfix = 15, f = 16, J = 17, mask), and for the contents of pmap -19 (an
 * entry outside -1 .. nf - 1) and -20 (a k < nf that no entry names). */
int blsq_model_eval_map_dev(blsq_ctx* ctx, int model, int B, int reps, int m, int n, int nf, const int32_t* pmap,
                            const double* dt, long t_stride, const double* dy, const double* dw, long w_stride,
                            const double* dX, const double* dPfix, double* df, double* dJ, const int32_t* dmask);
/* Composite models: a sum of up to BLSQ_MODEL_MAX_COMP components chosen at run time, each `cnt` terms of one family
 * (coords 1; there is no implicit offset: a constant is POLY with cnt 1):
 *   GAUSS    a exp(-z^2 / 2),  z = (t - mu) / s                               (a, mu, s)        3 per term
 *   LORENTZ  a / (1 + z^2)                                                    (a, mu, s)        3 per term
 *   PVOIGT   a [G + eta (L - G)],  G = exp(-ln2 z^2),  L = 1 / (1 + z^2)      (a, mu, s, eta)   4 per term
 *            (s: the half width at half maximum of both parts)
 *   EXP      a exp(-r t)                                                      (a, r)            2 per term
 *   POLY     sum_{k<cnt} p_k t^k by Horner: cnt coefficients                                    1 per term
 * The parameters (and the columns of J) are the concatenation of the components' slices in table order; a component's
 * value is the sum of its terms in ascending order, the model the sequential sum of the component values.  The term
 * formulas are those of the five closed models: {GAUSS K, POLY 1} gives the bits of GAUSS_SUM, and so on.  Append only.
 * blsq_term_info: the family's name and its parameters per term; any output may be NULL; needs no device.  Non-zero
 * for an unknown term. */
enum { BLSQ_TERM_GAUSS = 0, BLSQ_TERM_LORENTZ, BLSQ_TERM_PVOIGT, BLSQ_TERM_EXP, BLSQ_TERM_POLY };
#define BLSQ_MODEL_MAX_COMP 8
int blsq_term_count(void);
int blsq_term_info(int term, const char** name, int* n_per_term);
/* f and J of the composite {fam[c], cnt[c]}, c < ncomp, as blsq_model_eval_dev (pmap == NULL: dX is P [B * reps][n] and
 * nf must equal n) or through a parameter map as blsq_model_eval_map_dev (pmap, nf, dPfix: its rules).  fam, cnt and
 * pmap are HOST pointers read during the call: the table travels in the kernel arguments.  ncomp in
 * 1 .. BLSQ_MODEL_MAX_COMP, every fam[c] a BLSQ_TERM_*, every cnt[c] >= 1, sum cnt[c] * n_per_term(fam[c]) == n <=
 * BLSQ_MODEL_MAX_N; t_stride 0 or m.  A negative return is the index of the bad argument (ctx = 1, ncomp = 2, fam = 3,
 * cnt = 4, B, reps, m, n = 8, nf = 9, pmap = 10, t = 11, t_stride, y, w, w_stride = 15, X = 16, Pfix = 17, f = 18,
 * J = 19, mask), and for the contents of pmap -21 (an entry outside -1 .. nf - 1) and -22 (a k < nf that no entry
 * names); nothing is launched then. */
int blsq_model_eval_comp_dev(blsq_ctx* ctx, int ncomp, const int32_t* fam, const int32_t* cnt, int B, int reps, int m,
                             int n, int nf, const int32_t* pmap, const double* dt, long t_stride, const double* dy,
                             const double* dw, long w_stride, const double* dX, const double* dPfix, double* df,
                             double* dJ, const int32_t* dmask);
/* The estimator of a fit: what the residual of the models above is.  Append only.
 *   LSE      f = w (model - y): least squares, the three entries above.
 *   POISSON  maximum likelihood for counts y >= 0 under a model value mu > 0, through the deviance residual
 *              r = sign(mu - y) sqrt(D),   D = 2 [mu - y + y ln(y / mu)]   (the y ln term is 0 at y == 0)
 *            so that sum_i r_i^2 is the Poisson deviance 2 (NLL - NLL_saturated) and its minimiser the MLE:
 *              f[q][i]    = r(mu[q][i], y[b][i])
 *              J[q][i][k] = c * d mu / d p_k,   c = dr / dmu = (1 - y / mu) / r   (1 / sqrt(mu) at mu == y)
 *            with a parameter map the columns are summed first and the slot is multiplied by c.  r and c are evaluated
 *            in a form that neither cancels nor divides 0 by 0 at mu == y (the numpy definition is
 *            bounded_lsq.models.poisson_transform).  dy is required and dw must be NULL.  Nothing is checked on the
 *            device: mu <= 0 passes through as IEEE arithmetic gives it (the bounds of the fit must keep the model
 *            positive). */
enum { BLSQ_EST_LSE = 0, BLSQ_EST_POISSON };
/* One entry for every model instance, with the estimator.  model >= 0: the named model BLSQ_MODEL_* (ncomp must be 0;
 * fam and cnt are not read); model == -1: the composite {fam[c], cnt[c]}, c < ncomp, by the rules of
 * blsq_model_eval_comp_dev.  pmap == NULL: dX is P [B * reps][n] and nf must equal n; otherwise the parameter map of
 * blsq_model_eval_map_dev (pmap, nf, dPfix: its rules).  With BLSQ_EST_LSE the outputs are those of the entry this one
 * stands in for (blsq_model_eval_dev, _map_dev or _comp_dev), bit for bit.  Everything else as blsq_model_eval_dev.  A
 * negative return is the index of the bad argument (ctx = 1, est = 2, model = 3, ncomp = 4, fam = 5, cnt = 6, B = 7,
 * reps, m, n = 10, nf = 11, pmap = 12, t = 13, t_stride, y = 15, w = 16, w_stride, X = 18, Pfix = 19, f = 20, J = 21,
 * mask), and for the contents of pmap -23 (an entry outside -1 .. nf - 1) and -24 (a k < nf that no entry names); with
 * BLSQ_EST_POISSON dy == NULL is -15 and dw != NULL is -16.  Nothing is launched then. */
int blsq_model_eval_est_dev(blsq_ctx* ctx, int est, int model, int ncomp, const int32_t* fam, const int32_t* cnt, int B,
                            int reps, int m, int n, int nf, const int32_t* pmap, const double* dt, long t_stride,
                            const double* dy, const double* dw, long w_stride, const double* dX, const double* dPfix,
                            double* df, double* dJ, const int32_t* dmask);

/* The sampling of a model: what the value of row i is.  Append only.
 *   POINT  the model at the point t[b][.., i]: the entries above.
 *   BIN    the integral of the model over the bin [lo_i, hi_i] (the expected content of a histogram channel for a model
 *          read as a density); J holds the integrals of the point-sampled columns, a constant c contributes
 *          c (hi - lo).  dt then holds the edges as rows: [2][m] = lo, hi per problem (coords 1), and for GAUSS2D
 *          [4][m] = ulo, uhi, vlo, vhi, the pixel [ulo, uhi] x [vlo, vhi]; t_stride is 0 or 2 * coords * m.  Closed
 *          forms per term (erf by erfc of the magnitudes where both edges lie in one tail, atan2, expm1 with a series
 *          through r = 0, powers: DESIGN.md 7n; the numpy definition is bounded_lsq.models.binned).  The edges are not
 *          checked on the device: lo < hi and finite is the caller's to see to. */
enum { BLSQ_SAMPLE_POINT = 0, BLSQ_SAMPLE_BIN };
/* blsq_model_eval_est_dev with the sampling: one entry for every model instance, estimator and sampling.  With
 * BLSQ_SAMPLE_POINT the outputs are those of blsq_model_eval_est_dev, bit for bit; with BLSQ_SAMPLE_BIN dt and
 * t_stride are as described above and everything else is unchanged (estimator, parameter map, weights, reps, mask).
 * A negative return is the index of the bad argument (ctx = 1, est = 2, sampling = 3, model = 4, ncomp = 5, fam = 6,
 * cnt = 7, B = 8, reps, m, n = 11, nf = 12, pmap = 13, t = 14, t_stride = 15, y = 16, w = 17, w_stride, X = 19,
 * Pfix = 20, f = 21, J = 22, mask), and for the contents of pmap -24 (an entry outside -1 .. nf - 1) and -25 (a k < nf
 * that no entry names); with BLSQ_EST_POISSON dy == NULL is -16 and dw != NULL is -17.  Nothing is launched then. */
int blsq_model_eval_bin_dev(blsq_ctx* ctx, int est, int sampling, int model, int ncomp, const int32_t* fam,
                            const int32_t* cnt, int B, int reps, int m, int n, int nf, const int32_t* pmap,
                            const double* dt, long t_stride, const double* dy, const double* dw, long w_stride,
                            const double* dX, const double* dPfix, double* df, double* dJ, const int32_t* dmask);

/* What a NaN in y means.  Append only.
 *   PROPAGATE  nothing special: the NaN passes through the residual as IEEE arithmetic gives it (the entries above).
 *   OMIT       point i of problem b is left out of the fit iff y[b][i] is NaN: f[q][i] = +0.0 and row i of
 *              J is +0.0 in every column, for every rep.  Its t, w (and bin edges) are never read and may hold anything,
 *              NaN included; the row costs no arithmetic.  +-inf in y is not missing data and passes through.  A row of
 *              zeros changes no singular value of J, so the solvers, the losses and the covariance run unchanged; only
 *              the degrees of freedom differ per problem (blsq_outer_covariance_pinv_nobs).  dy is required. */
enum { BLSQ_NAN_PROPAGATE = 0, BLSQ_NAN_OMIT };
/* blsq_model_eval_bin_dev with the NaN policy: one entry for every model instance, estimator, sampling and policy.
 * With BLSQ_NAN_PROPAGATE the outputs are those of blsq_model_eval_bin_dev, bit for bit; with BLSQ_NAN_OMIT the kept rows
 * are, and the omitted ones are zeros.  A negative return is the index of the bad argument (ctx = 1, est = 2,
 * sampling = 3, nan_policy = 4, model = 5, ncomp = 6, fam = 7, cnt = 8, B = 9, reps, m, n = 12, nf = 13, pmap = 14,
 * t = 15, t_stride = 16, y = 17, w = 18, w_stride, X = 20, Pfix = 21, f = 22, J = 23, mask), and for the contents of
 * pmap -25 (an entry outside -1 .. nf - 1) and -26 (a k < nf that no entry names); with BLSQ_EST_POISSON or
 * BLSQ_NAN_OMIT dy == NULL is -17, with BLSQ_EST_POISSON dw != NULL is -18.  Nothing is launched then. */
int blsq_model_eval_nan_dev(blsq_ctx* ctx, int est, int sampling, int nan_policy, int model, int ncomp,
                            const int32_t* fam, const int32_t* cnt, int B, int reps, int m, int n, int nf,
                            const int32_t* pmap, const double* dt, long t_stride, const double* dy, const double* dw,
                            long w_stride, const double* dX, const double* dPfix, double* df, double* dJ,
                            const int32_t* dmask);

/* Global fits: G groups of S data sets of one model, m points each.  Every data set has the n parameters
 * of the model over the nf slots of pmap (the rules of blsq_model_eval_map_dev; pmap is required, the identity for a
 * model without fixed or tied parameters).  A slot k with shared[k] == 1 is ONE variable of the group; a slot with
 * shared[k] == 0 is one variable per data set.  With ns shared slots and nl = nf - ns local ones the group is one dense
 * problem of S m rows and nv = ns + S nl <= BLSQ_GLOBAL_MAX_NV variables, ordered: the shared slots in ascending slot
 * order, then the local slots of data set 0 in ascending slot order, then those of data set 1, ...  For the points
 * X [G * reps][nv] (q = g * reps + r) and the template Pfix [G][S][n]:
 *   f[q][s m + i]      = the f of blsq_model_eval_nan_dev for data set s at the parameters its variables give, bit for bit
 *   J[g][s m + i][col] = its mapped J[i][k] where col is the variable of slot k in data set s, +0.0 (every bit zero) in
 *                        every other column, under either estimator                               dJ [G][S m][nv]
 * dy: [G][S m] or NULL; dt: data set s of group g reads dt + g * t_stride + s * t_sstride, with t_sstride 0 or m and
 * t_stride 0 or the doubles of one group (S m with t_sstride == m, otherwise m); dw: NULL, [m] (w_stride 0) or [G][S m]
 * (w_stride S m); dmask: int32 [G] or NULL, a group with dmask[g] == 0 is left untouched.  shared: HOST pointer,
 * int32 [nf] of 0 / 1, read during the call as fam, cnt and pmap are.  sampling must be BLSQ_SAMPLE_POINT (-3) and the
 * model one of a single coordinate (GAUSS2D: -5).  S == 1 with every slot shared gives the outputs of
 * blsq_model_eval_nan_dev.  A negative return is the index of the bad argument (ctx = 1, est = 2, sampling = 3,
 * nan_policy = 4, model = 5, ncomp = 6, fam = 7, cnt = 8, S = 9, shared = 10, t_sstride = 11, G = 12, reps, m, n = 15,
 * nf = 16, pmap = 17, t = 18, t_stride = 19, y = 20, w = 21, w_stride, X = 23, Pfix = 24, f = 25, J = 26, mask); more
 * than BLSQ_GLOBAL_MAX_NV variables is -9, and for the contents of pmap -28 and -29 as above.  Nothing is launched then.
 * BLSQ_GLOBAL_MAX_NV is an interface limit that keeps a group inside the normal-equations front end (n + 1 <= 272,
 * DESIGN.md 9); it is not a measured figure. */
#define BLSQ_GLOBAL_MAX_NV 256
int blsq_model_eval_global_dev(blsq_ctx* ctx, int est, int sampling, int nan_policy, int model, int ncomp,
                               const int32_t* fam, const int32_t* cnt, int S, const int32_t* shared, long t_sstride,
                               int G, int reps, int m, int n, int nf, const int32_t* pmap, const double* dt,
                               long t_stride, const double* dy, const double* dw, long w_stride, const double* dX,
                               const double* dPfix, double* df, double* dJ, const int32_t* dmask);

/* Affine ties: a tied parameter that follows its slot by a ratio and an offset,
 *   P_full[q][j] = tie_ratio[j] * X[q][.] + tie_offset[j]   where pmap[j] >= 0 (X[q][.]: the variable of slot pmap[j], as
 *                  in the entry this one extends; the product first, then the sum; where the pair is (1, 0) the plain
 *                  copy, so a -0.0 stays -0.0),            Pfix[b][j] where pmap[j] == -1
 *   f            = the f of blsq_model_eval_nan_dev at P_full, bit for bit
 *   J[..][i][k]  = sum over {j : pmap[j] == k}, in ascending j, of tie_ratio[j] * (the J[i][j] of blsq_model_eval_nan_dev
 *                  at P_full): the model's weighted column first, then the ratio; the first column of a slot is stored
 *                  after its multiply and the later ones are added to it.  Under BLSQ_EST_POISSON the slot is multiplied
 *                  by c after its sum, as without ties.
 * The signature is that of blsq_model_eval_global_dev with tie_ratio and tie_offset directly behind pmap: HOST pointers,
 * double [n] each, read during the call (they travel in the kernel arguments, as pmap does); entries at fixed parameters
 * (pmap[j] == -1) are not read.  Both NULL: the plain map.  S >= 1: a global evaluation by the rules of
 * blsq_model_eval_global_dev (and with both NULL its outputs, bit for bit).  S == 0: a plain batch of G problems by the
 * rules of blsq_model_eval_nan_dev with a pmap (and with both NULL its outputs): shared is ignored, t_sstride must be
 * 0, and BLSQ_SAMPLE_BIN and GAUSS2D are taken.  pmap is required.  A negative return is the index of the bad argument
 * (ctx = 1, est = 2, sampling = 3, nan_policy = 4, model = 5, ncomp = 6, fam = 7, cnt = 8, S = 9, shared = 10,
 * t_sstride = 11, G = 12, reps, m, n = 15, nf = 16, pmap = 17, tie_ratio = 18, tie_offset = 19, t = 20, t_stride = 21,
 * y = 22, w = 23, w_stride, X = 25, Pfix = 26, f = 27, J = 28, mask); exactly one of tie_ratio / tie_offset NULL is the
 * number of the NULL one; for the contents of pmap -30 and -31 as above, and for a j with pmap[j] >= 0 -32 (a ratio that
 * is 0 or not finite) and -33 (an offset that is not finite).  Nothing is launched then. */
int blsq_model_eval_tie_dev(blsq_ctx* ctx, int est, int sampling, int nan_policy, int model, int ncomp,
                            const int32_t* fam, const int32_t* cnt, int S, const int32_t* shared, long t_sstride, int G,
                            int reps, int m, int n, int nf, const int32_t* pmap, const double* tie_ratio,
                            const double* tie_offset, const double* dt, long t_stride, const double* dy,
                            const double* dw, long w_stride, const double* dX, const double* dPfix, double* df,
                            double* dJ, const int32_t* dmask);

/* ---- linear residuals, evaluated on the device -----------------------------------------------------
 * The callbacks of a bounded linear least-squares solve, min 1/2 |A x - y|^2 with lb <= x <= ub (blsq_outer_*:
 * f <- fun(x), J <- jac(x)), so that the whole batched solve stays on the GPU.  For the points X [B * reps][n] (the
 * points of problem b are rows b * reps .. b * reps + reps - 1, as blsq_model_eval_dev):
 *   f[q][i] = w[b][i] * (sum_j A[b][i][j] * X[q][j] - y[b][i])          df [B * reps][m], or NULL
 *   J[b]    = diag(w[b]) * A[b]                                         dJ [B][m][n], or NULL; reps must be 1
 * dA: row-major [m][n], the layout of J: ONE matrix shared by all problems (A_stride 0) or [B][m][n] (A_stride m * n);
 * dy: [B][m] or NULL (0: a plain product); dw: NULL (1), [m] (w_stride 0) or [B][m] (w_stride m); dmask: int32 [B] or
 * NULL: J[b] of a problem with dmask[b] == 0 is not touched at all (f takes no mask).  The sum is a chain of fma() per
 * lane and a fixed tree over the lanes, a function of n alone: a problem's f does not depend on B, reps, the strides or
 * its batch mates, and f for a shared A equals, bit for bit, f for that matrix replicated.  With dw == NULL J[b] is A[b]
 * bit for bit; with dw every element is multiplied once.  Nothing is checked on the device: non-finite values pass
 * through as IEEE arithmetic gives them.  1 <= n <= BLSQ_LINEAR_MAX_N (the widest plan), m >= 1.  All pointers are device
 * pointers; asynchronous on the ctx stream; timed in the `model_eval` slot.  A negative return is the index of the bad
 * argument (ctx = 1, B = 2, reps = 3, m = 4, n = 5, A = 6, A_stride = 7, y, w = 9, w_stride = 10, X = 11, f = 12: f and
 * J both NULL, J = 13: reps != 1, mask); nothing is launched then. */
#define BLSQ_LINEAR_MAX_N 1023
int blsq_linear_eval_dev(blsq_ctx* ctx, int B, int reps, int m, int n, const double* dA, long A_stride,
                         const double* dy, const double* dw, long w_stride, const double* dX, double* df, double* dJ,
                         const int32_t* dmask);

/* ---- instrument response: a model convolved with a measured kernel -----------------------------------
 * The second stage of a fit whose model passes through an instrument before it meets the data (a decay through the
 * response of a detector, a line through the resolution of a spectrometer).  The first stage is any blsq_model_eval*_dev
 * entry called with y = NULL, w = NULL, no estimator and no omission: it writes the raw model values dg [B * reps][m]
 * and the raw Jacobian dG [B][m][nc] (nc: n, or nf of a map).  This entry convolves both along the rows,
 *   mu[q][i]    = sum_{k < L} h[b][k] * g[q][i + origin - k]               q = b * reps + r, r < reps
 *   HG[b][i][j] = sum_{k < L} h[b][k] * G[b][i + origin - k][j]
 * where a term whose index i + origin - k lies outside [0, m) is dropped (zeros past both ends; origin 0: the causal
 * convolution, origin L / 2 with odd L: a centred kernel), and applies what the first stage was not given:
 *   BLSQ_EST_LSE:      f = w (mu - y),  J = w HG            (dy NULL: 0; dw NULL: 1)
 *   BLSQ_EST_POISSON:  (r, c) of the deviance residual at (mu, y):  f = r,  J = c HG   (dy required, dw must be NULL;
 *                      dg is then needed for J as well)
 *   BLSQ_NAN_OMIT:     f and the row of J are +0.0 where y is NaN (dy required); the model is still evaluated there
 * into df [B * reps][m] and / or dJ [B][m][nc] (reps must be 1).  dh: [L] shared by all problems (h_stride 0) or [B][L]
 * (h_stride L); dw: NULL, [m] (w_stride 0) or [B][m] (w_stride m); dmask: int32 [B] or NULL: dJ[b] of a problem with
 * dmask[b] == 0 is not touched and nothing of the problem is read (f takes no mask).  The convolution is over the
 * sample index: a uniform grid, and h sampled at its spacing, are the caller's business.  The sum of row i takes its
 * taps in ascending k, the first as a product and the others by fma(): a function of (L, origin, i, m) alone, not of B,
 * reps, nc, the strides or the batch mates; with h = [1.0] the stage is the identity in every bit.  Nothing is checked
 * on the device.  1 <= L <= BLSQ_RESPONSE_MAX_L, 0 <= origin < L, 1 <= m <= BLSQ_RESPONSE_MAX_M, nc >= 1 (L may exceed
 * m).  All pointers are device pointers; asynchronous on the ctx stream; f and J of one call are one unit of the
 * `model_eval` slot.  A negative return is the index of the bad argument (ctx = 1, est = 2, nan_policy = 3, B = 4,
 * reps = 5, m = 6, nc = 7, L = 8, origin = 9, h = 10, h_stride = 11, g = 12, G = 13, y = 14, w = 15, w_stride = 16,
 * f = 17: f and J both NULL, J = 18: reps != 1, mask); nothing is launched then. */
#define BLSQ_RESPONSE_MAX_L 1024
#define BLSQ_RESPONSE_MAX_M 0x7fff0000
int blsq_response_apply_dev(blsq_ctx* ctx, int est, int nan_policy, int B, int reps, int m, int nc, int L, int origin,
                            const double* dh, long h_stride, const double* dg, const double* dG, const double* dy,
                            const double* dw, long w_stride, double* df, double* dJ, const int32_t* dmask);

/* ---- BVLS and NNLS: an exact active-set solver, a batch in two calls ---------------------------------
 * min 1/2 |W (A x - y)|^2 with lb <= x <= ub is a strictly convex quadratic programme in the moments G = A^T W^2 A and
 * c = A^T W^2 y.  blsq_bvls_moments_dev forms them; blsq_bvls_solve_dev runs the active-set iteration of Stark and
 * Parker (Lawson and Hanson's NNLS for bounds (0, inf)) for every problem in a workgroup of its own, to the exact
 * minimiser and the exact active set: a variable on a bound holds lb or ub bit for bit.  The first call launches one or
 * two kernels (G and c apart for a shared A), the second one; no host round trip inside or between them.
 *
 * Moments.  dA: row-major [m][n], ONE matrix (A_stride 0) or [B][m][n] (A_stride m * n); dy: [B][m]; dw: NULL (1), [m]
 * (w_stride 0) or [B][m] (w_stride m).  dG: [n][n] for the whole batch (G_stride 0; only with A_stride 0 and w not per
 * problem) or [B][n][n] (G_stride n * n); dc: [B][n].  FP64 MFMA; the summation order is a function of m alone, a
 * problem's c does not depend on its batch mates, and G is symmetric in every bit.
 *
 * Solve.  dG / G_stride / dc as above (G symmetric positive definite: both triangles are read); dlb, dub: [B][n],
 * lb < ub, infinities allowed; a variable on a bound leaves it when the gradient pushes it inwards by more than tol;
 * max_pass: the most release passes per problem.  Outputs: dx [B][n]; don_bound int32 [B][n] in {-1, 0, 1}; dgrad
 * [B][n]; doptimality [B][2]: max(max over free |g_j|, max over bound g_j on_bound_j, 0), and the cost 1/2 sum fun^2
 * (0 without A); dstat int32 [B][3]: status, release passes, factorisations.  Status 1: the optimality conditions hold;
 * 0: max_pass passes used (a variable barred against cycling is asked again before 1 is returned); -1: a pivot of a free block was <= 0 or not finite, or a value was not finite (x is then the
 * last feasible iterate).  Every loop on the device has a structural bound.
 * dA == NULL: the solve on (G, c) alone: g = G x - c; m, dy, dw and the strides are not read and dfun must be NULL.
 * dA != NULL (with dy, dw and the strides of the moments call): after the iteration x_F is corrected once against A,
 * x_F += (G_FF)^-1 A_F^T W^2 (y - A x), and clamped; then dfun [B][m] = w (A x - y) (or NULL: not written) and
 * g = A^T w fun come from A itself.  The status is that of the iteration.
 * 1 <= n <= BLSQ_BVLS_MAX_N.  All pointers are device pointers; asynchronous on the ctx stream; each call is one unit of
 * the `model_eval` slot.  A negative return is the index of the bad argument, checked in this order (moments: ctx = 1,
 * B = 2, m = 3, n = 4, A = 5, A_stride = 6, y = 7, w, w_stride = 9, G = 10, G_stride = 11, c = 12; solve: ctx = 1,
 * B = 2, m = 3, n = 4, G = 5, G_stride = 6, c = 7, lb = 8, ub = 9, tol = 10: not a number, max_pass = 11, A,
 * A_stride = 13, y = 14, w, w_stride = 16, x = 17, on_bound = 18, fun = 19: given without A, grad = 20,
 * optimality = 21, stat = 22); nothing is launched then.
 *
 * Solve under a sum constraint.  blsq_bvls_solve_eq_dev is the solve above with one linear equality per
 * problem, e^T x = d: the arguments of blsq_bvls_solve_dev in their order and with their checks and numbers, then de:
 * [n] for the whole batch (e_stride 0) or [B][n] (e_stride n), every e_j finite and not zero; dd: [B]; dmultiplier:
 * [B], out: the multiplier lambda of the equality, so that g + lambda e vanishes on the free variables and
 * (g_j + lambda e_j) on_bound_j <= 0 on the others (least squares over the free set, -e_F^T g_F / e_F^T e_F; with no
 * free variable the midpoint of the admissible interval, or its finite end).  The iteration starts from a feasible
 * point (x = clip(0, lb, ub), the gap d - e^T x walked off in ascending j), solves G_FF z + lambda e_F = c_F - G_FB x_B,
 * e_F^T z = d - e_B^T x_B on the free set from ONE factorisation, and releases on the reduced gradient g + lambda e;
 * with dA the correction against A is projected, x_F += s - mu v, so that the sum is restored as well.  doptimality[b][0]
 * is max(max over free |g_j + lambda e_j|, max over bound (g_j + lambda e_j) on_bound_j, 0); dgrad stays the plain
 * gradient.  Status as above, and for THIS entry alone -2: the equality cannot be met inside the bounds (x is then
 * clip(0, lb, ub)); an e_j that is zero or not finite, a d that is not finite, or e_F^T (G_FF)^-1 e_F not positive is
 * status -1.  One kernel, one unit of the `model_eval` slot.  Bad arguments: 1 .. 22 as blsq_bvls_solve_dev, then
 * e = 23, e_stride = 24, d = 25, multiplier = 26. */
#define BLSQ_BVLS_MAX_N 128
int blsq_bvls_moments_dev(blsq_ctx* ctx, int B, int m, int n, const double* dA, long A_stride, const double* dy,
                          const double* dw, long w_stride, double* dG, long G_stride, double* dc);
int blsq_bvls_solve_dev(blsq_ctx* ctx, int B, int m, int n, const double* dG, long G_stride, const double* dc,
                        const double* dlb, const double* dub, double tol, int max_pass, const double* dA,
                        long A_stride, const double* dy, const double* dw, long w_stride, double* dx,
                        int32_t* don_bound, double* dfun, double* dgrad, double* doptimality, int32_t* dstat);
int blsq_bvls_solve_eq_dev(blsq_ctx* ctx, int B, int m, int n, const double* dG, long G_stride, const double* dc,
                           const double* dlb, const double* dub, double tol, int max_pass, const double* dA,
                           long A_stride, const double* dy, const double* dw, long w_stride, double* dx,
                           int32_t* don_bound, double* dfun, double* dgrad, double* doptimality, int32_t* dstat,
                           const double* de, long e_stride, const double* dd, double* dmultiplier);

/* ---- expression models: a formula interpreted on the device -----------------------------------------
 * A model that is none of the built-in ones, given as a short straight-line program (compiled on the host from the
 * user's formula; bounded_lsq/_expr.py has the language and IS the definition of every value below).  A program is
 * (ops[nops], consts[nconst], root), 0 <= nops <= BLSQ_EXPR_MAX_OPS, 0 <= nconst <= BLSQ_EXPR_MAX_CONST.
 * An operand is 16 bits, its kind in the high byte and an index in the low one:
 *   TAPE k   the result of the earlier op k          PFIX j   model parameter j, held per problem: Pfix[b][j]
 *   VAR k    solver variable k: X[q][k]              CONST i  consts[i]             COORD r  coordinate r: t[b][r][i]
 * An op is one 64-bit word: the opcode in bits 0-7, operand a in bits 8-23, operand b in bits 24-39 (ADD SUB MUL DIV
 * and POWC take two operands, the others one: b is then not read; the b of POWC, the exponent, is a CONST).  root is an
 * operand and may be a leaf.
 * Forward: val[k] for k ascending; the model value v is the value of root.  Reverse, for the row of J: adjoints and row
 * start at +0.0, 1 is pushed to root, then k descending with g = adj[k], a pushed before b; a push is dst = dst +
 * contribution, dst being adj[.] of a TAPE operand whose op depends on a variable and column k of the row for VAR k; a
 * push to anything else is dropped and an op that depends on no variable is skipped.  Contributions to a and b:
 *   ADD g, g    SUB g, -g    MUL g*vb, g*va    DIV g/vb, -((g*v)/vb)    NEG -g    EXP g*v    LOG g/va    SQRT (0.5*g)/v
 *   SIN g*cos(va)    COS -(g*sin(va))    ATAN g/(1+va*va)    ERF g*(C*exp(-(va*va))), C = 1.1283791670955126
 *   ERFC the negative of ERF's    POWC g*(c*pow(va, c-1))
 * Then f = w (v - y) (y NULL: v) and the row is multiplied by w as a whole; under BLSQ_EST_POISSON f = r and the row is
 * multiplied by c of the deviance residual (blsq_model_eval_est_dev).  Compiled without contraction: the device differs
 * from the definition in the last bits of exp, log, sin, cos, atan, erf, erfc and pow only.
 *
 * blsq_expr_check: takes no context and no device.  0, or minus the position of the first bad argument, looked at in
 * this order: nops (1: outside 0 .. BLSQ_EXPR_MAX_OPS), ops (2: NULL with nops > 0), nconst (4: outside
 * 0 .. BLSQ_EXPR_MAX_CONST), nf (5: outside 1 .. BLSQ_MODEL_MAX_N), npfix (6: outside 0 .. BLSQ_MODEL_MAX_N), ncoord
 * (7: outside 1 .. BLSQ_EXPR_MAX_COORD), then the contents of ops (2: an unknown opcode, a TAPE operand that does not
 * name a strictly earlier op, VAR >= nf, PFIX >= npfix, CONST >= nconst, COORD >= ncoord, an unknown kind, a POWC whose
 * b is not a CONST), then root (3: not a valid operand, TAPE >= nops).
 *
 * blsq_expr_eval_dev: f [B * reps][m] and / or J [B][m][nf] (reps must be 1) at X [B * reps][nf], as blsq_model_eval_dev
 * and with its rules: dt [ncoord][m] shared (t_stride 0) or [B][ncoord][m] (t_stride ncoord * m); dy [B][m] or NULL; dw
 * NULL, [m] (w_stride 0) or [B][m] (w_stride m); dPfix [B][npfix], read for PFIX operands only (NULL without one);
 * dmask int32 [B] or NULL: a problem with dmask[b] == 0 is left untouched.  est: BLSQ_EST_*; POISSON needs dy and takes no
 * dw.  nan_policy: BLSQ_NAN_*; OMIT needs dy: a row whose y is NaN is +0.0 in f and in every slot of J and nothing of
 * it is evaluated.  ops and consts are HOST pointers read during the call: the program travels in the kernel arguments.
 * All other pointers are device pointers; asynchronous on the ctx stream; timed in the `model_eval` slot.  A negative
 * return is the index of the bad argument (ctx = 1, est = 2, nan_policy = 3, B = 4, reps = 5, m = 6, nf = 7, npfix = 8,
 * ncoord = 9, nops = 10, ops = 11, root = 12, nconst = 13, consts = 14: NULL with nconst > 0, t = 15, t_stride = 16,
 * y = 17, w = 18, w_stride = 19, X = 20, Pfix = 21, f = 22: f and J both NULL, J = 23: reps != 1, mask); the program is
 * checked as blsq_expr_check checks it, behind est, nan_policy, B, reps and m; nothing is launched then. */
#define BLSQ_EXPR_MAX_OPS 64
#define BLSQ_EXPR_MAX_CONST 32
#define BLSQ_EXPR_MAX_COORD 4
enum {
  BLSQ_EXPR_ADD = 0, BLSQ_EXPR_SUB, BLSQ_EXPR_MUL, BLSQ_EXPR_DIV, BLSQ_EXPR_NEG, BLSQ_EXPR_EXP, BLSQ_EXPR_LOG,
  BLSQ_EXPR_SQRT, BLSQ_EXPR_SIN, BLSQ_EXPR_COS, BLSQ_EXPR_ATAN, BLSQ_EXPR_ERF, BLSQ_EXPR_ERFC, BLSQ_EXPR_POWC
};
enum { BLSQ_EXPR_TAPE = 0, BLSQ_EXPR_VAR, BLSQ_EXPR_PFIX, BLSQ_EXPR_CONST, BLSQ_EXPR_COORD };
int blsq_expr_check(int nops, const uint64_t* ops, int root, int nconst, int nf, int npfix, int ncoord);
int blsq_expr_eval_dev(blsq_ctx* ctx, int est, int nan_policy, int B, int reps, int m, int nf, int npfix, int ncoord,
                       int nops, const uint64_t* ops, int root, int nconst, const double* consts, const double* dt,
                       long t_stride, const double* dy, const double* dw, long w_stride, const double* dX,
                       const double* dPfix, double* df, double* dJ, const int32_t* dmask);

/* ---- separable fits: variable projection of the linear parameters -----------------------------------
 * A model sum_k c_k phi_k(t; alpha) is linear in nl of its n parameters (amplitudes, polynomial coefficients, offsets).
 * For given alpha the best c solves a small linear least-squares problem, so the solver sees the na = n - nl others
 * alone (Golub and Pereyra), with Kaufman's Jacobian.  Three calls per evaluation: blsq_varpro_expand_dev, any
 * blsq_model_eval*_dev entry called for J with y = NULL, w = NULL, no estimator and no omission, and
 * blsq_varpro_reduce_dev.
 *
 * lin: HOST int32 [nl], the ascending indices of the linear parameters.  owner: HOST int32 [n], -1 on lin and, for
 * every other parameter, the position in lin of the amplitude its column scales with (mu, s and eta of a pvoigt term:
 * its a).  Both are read during the call and travel in the kernel arguments.  bounded_lsq/_varpro.py (linear_params,
 * varpro_expand, varpro_reduce) IS the definition.
 *
 * blsq_varpro_expand_dev: dP [B][n] = 1.0 in the slots lin and dX [B][na] in the others, in ascending order: bit-exact.
 *
 * blsq_varpro_reduce_dev: dG [B][m][n] is the raw Jacobian at dP, so dG[:, lin] = Phi.  With Phi_w = w Phi,
 * A_w = [w G[:, non] | w y] and S = Phi_w^T Phi_w:
 *   T  = S^-1 Phi_w^T A_w     E  = A_w - Phi_w T
 *   T2 = S^-1 Phi_w^T E       E <- E - Phi_w T2,  T <- T + T2          (one correction against Phi_w itself)
 *   dc = T[:, last]   df = -E[:, last] = w (Phi c - y)   dJ[:, i] = c[owner[non[i]]] E[:, i]
 * dJ^T df is the exact gradient of 1/2 |df|^2.  The correction keeps the error of every output at a small multiple of
 * kappa(Phi_w) eps; without it the error is kappa^2 eps.  S is scaled to unit diagonal before its Cholesky factor;
 * a diagonal entry of S that is not positive and finite, or a pivot of the scaled matrix that is not above 64 eps, marks
 * Phi as rank deficient: dinfo[b] = 1 and every output of problem b is NaN; dinfo[b] = 0 otherwise.
 * dy: [B][m]; dw: NULL (1), [m] (w_stride 0) or [B][m] (w_stride m); df [B][m], dJ [B][m][na], dc [B][nl], dinfo [B]:
 * each may be NULL (not all of df, dJ, dc).  dmask: int32 [B] or NULL: a problem with dmask[b] == 0 is left untouched
 * and nothing of it is read.  One workgroup per problem; the moments and both projections run on the FP64 MFMA pipe.
 * The summation order is a function of m and the layout (lin, owner) alone: a problem's bits do not depend on B or on
 * its position in the batch.  1 <= nl <= BLSQ_VARPRO_MAX_NL, na >= 1, n <= BLSQ_MODEL_MAX_N, m > nl.
 * All other pointers are device pointers; asynchronous on the ctx stream; each call is one unit of the `model_eval`
 * slot.  A negative return is the index of the bad argument (expand: ctx = 1, B = 2, n = 3, nl = 4, lin = 5: NULL, not
 * ascending or out of range, X = 6, P = 7; reduce: ctx = 1, B = 2, m = 3: not positive or m <= nl, n = 4, nl = 5:
 * outside 1 .. BLSQ_VARPRO_MAX_NL or nl >= n, lin = 6, owner = 7: NULL or inconsistent with lin, G = 8, y = 9, w,
 * w_stride = 11, f = 12: f, J and c all NULL, J, c, info, mask); nothing is launched then. */
#define BLSQ_VARPRO_MAX_NL 16
int blsq_varpro_expand_dev(blsq_ctx* ctx, int B, int n, int nl, const int32_t* lin, const double* dX, double* dP);
int blsq_varpro_reduce_dev(blsq_ctx* ctx, int B, int m, int n, int nl, const int32_t* lin, const int32_t* owner,
                           const double* dG, const double* dy, const double* dw, long w_stride, double* df, double* dJ,
                           double* dc, int32_t* dinfo, const int32_t* dmask);

/* ---- separable global fits: shared non-linear parameters, projected linear ones ---------------------
 * G groups of S data sets of one model.  Some NON-LINEAR parameters are shared by the data sets of a group; the linear
 * ones are projected out per data set as above.  shared: HOST int32 [n], 1 for a shared parameter and 0 elsewhere
 * (a flag that is neither, or one set on a linear parameter, is an error).  With nsh shared and nloc local non-linear
 * parameters the group has nv = nsh + S nloc <= BLSQ_GLOBAL_MAX_NV solver variables: the shared ones in ascending
 * order, then the nloc local ones of data set 0, 1, ... (bounded_lsq.GlobalMap over the non-linear parameters;
 * bounded_lsq/_varpro.py: separable_global_map, separable_global_residual / _jacobian / _cov ARE the definition).
 * The full count nv + S nl has no limit.  Data set s of group g is problem b = g S + s.
 *
 * blsq_varpro_expand_global_dev: dX [G][nv] -> dP [G S][n]: 1.0 in the slots lin, the shared variables and the window
 * of data set s in the others.  Bit-exact.
 *
 * blsq_varpro_reduce_global_dev: the arithmetic of blsq_varpro_reduce_dev, bit for bit, on the G S data sets of
 * dG [G S][m][n] (the raw Jacobian at dP).  dy and df are [G][S m]; dw is NULL, [m] (w_stride 0) or [G][S m]
 * (w_stride S m); dJ is [G][S m][nv], the group's layout: Kaufman's columns of data set s in its rows s m .. s m + m - 1
 * at its variables, and the literal +0.0 in every other column of those rows, stored by the same workgroup: every
 * element of a group's J is written exactly once per call and no memset is relied on.  dc [G S][nl], dinfo [G S].
 * dSinv [G S][nl][nl] = (Phi_w^T Phi_w)^-1 (from the factor: D Ri Ri^T D, exactly symmetric) and dTD [G S][nl][na],
 * TD[:, i] = c[owner[non[i]]] (T + T2)[:, i], are what the covariance below needs; TD is formed from T after one more
 * correction whose residual is computed in double-double arithmetic (a column of T solves for a column of G with a
 * residual as large as the column: kappa eps |T| would not do), at a cost that only a call asking for dTD pays.  Each output may be NULL (not all).
 * dmask: int32 [G] or NULL: a group with dmask[g] == 0 is neither read nor written.  A rank-deficient data set gets
 * dinfo = 1 and NaN in its rows of f, its own columns of those rows of J, its c, Sinv and TD; its other columns are
 * still +0.0 and its group mates are unaffected.
 *
 * blsq_varpro_cov_blocks_dev: Kaufman's J_K^T J_K is the Schur complement of the full Gauss-Newton matrix onto the
 * non-linear variables, so the covariance dC [G][nv][nv] of the reduced group is the exact alpha-alpha block of the full
 * covariance.  With C_s its rows and columns of data set s (the upper triangle of dC is read), per data set:
 *   alpha-alpha = C_s     c-alpha = -TD_s C_s     c-c = Sinv_s + TD_s C_s TD_s^T
 * placed at the model's parameter indices in dcov [G S][n][n], exactly symmetric, times dscale[g] (NULL: 1); sums in
 * ascending order.  NaN for a data set with dinfo[b] != 0 (NULL: none) or a group with dstatus[g] != 0 (NULL: none).
 * Nothing of the full size nv + S nl is ever formed.
 *
 * One workgroup per data set; asynchronous on the ctx stream; each call is one unit of the `model_eval` slot.  A
 * negative return is the index of the bad argument, nothing is launched then (expand_global: ctx = 1, G = 2, S = 3:
 * below 1, G S above 2^31 - 1 or nv above BLSQ_GLOBAL_MAX_NV, n = 4, nl = 5, lin = 6, shared = 7, X = 8, P = 9;
 * reduce_global: ctx = 1, G = 2, S = 3, m = 4: not positive or m <= nl, n = 5, nl = 6, lin = 7, owner = 8, shared = 9,
 * G = 10, y = 11, w, w_stride = 13: neither 0 nor S m, f = 14: every output NULL, J, c, info, Sinv, TD, mask;
 * cov_blocks: ctx = 1, G = 2, S = 3, n = 4, nl = 5, lin = 6, shared = 7, C = 8, Sinv = 9, TD = 10, scale, info, status,
 * cov = 14). */
int blsq_varpro_expand_global_dev(blsq_ctx* ctx, int G, int S, int n, int nl, const int32_t* lin, const int32_t* shared,
                                  const double* dX, double* dP);
int blsq_varpro_reduce_global_dev(blsq_ctx* ctx, int G, int S, int m, int n, int nl, const int32_t* lin,
                                  const int32_t* owner, const int32_t* shared, const double* dG, const double* dy,
                                  const double* dw, long w_stride, double* df, double* dJ, double* dc, int32_t* dinfo,
                                  double* dSinv, double* dTD, const int32_t* dmask);
int blsq_varpro_cov_blocks_dev(blsq_ctx* ctx, int G, int S, int n, int nl, const int32_t* lin, const int32_t* shared,
                               const double* dC, const double* dSinv, const double* dTD, const double* dscale,
                               const int32_t* dinfo, const int32_t* dstatus, double* dcov);

/* ---- parameter covariance from the final Jacobian --------------------------------------------------------------
 * The reference documents `x_covariance` as the inverse of J^T J at the solution (least_squares.py:248-252) and fills
 * it only through its MINPACK bridge (method='lm').  Here, per problem, from a Householder triangle R of J (the TSQR
 * tree: a Gram-Cholesky triangle would square the conditioning):
 *   active == NULL:  C = (J^T J)^-1 = R^-1 R^-T over all n variables;
 *   active != NULL:  int64 [B][n]; F = {j : active[j] == 0}; C[F,F] = (J_F^T J_F)^-1, every row and column of an
 *                    active variable exactly 0.0 (the covariance with the variables on a bound held fixed).
 * rcond[b] = 1 / (||R||_1 ||R^-1||_1) from the explicit inverse.  status[b] = 1 (singular) when a pivot of R is zero
 * or not finite (rcond = 0) or rcond < eps * max(m, |F|): cov[b] is then NaN everywhere; 0 otherwise.  A Jacobian
 * with fewer rows than free columns is singular, not an error.  No residual-variance scaling is applied.  cov is the
 * full symmetric matrix [B][n][n], exactly symmetric; a problem's bits do not depend on B or on its batch mates.
 * Shapes: n + 1 <= 1024 as the TSQR tree; m > 1024 with n > 512, past the tree's merge capacity, is factored by folding
 * the rows in sequentially (1024 at a time under the triangle) and needs n + 1 <= 1008.  B <= 65535.
 * blsq_cov_dev: device pointers, asynchronous on the ctx stream; J is not modified.  blsq_cov: host pointers, blocking. */
int blsq_cov_plan_create(blsq_ctx* ctx, int B, int m, int n, blsq_cov_plan** out);
int blsq_cov_plan_destroy(blsq_cov_plan* plan);
int blsq_cov_dev(blsq_cov_plan* plan, const double* dJ, const int64_t* dactive /*[B][n] or NULL = all variables*/,
                 double* dcov /*[B][n][n]*/, double* drcond /*[B]*/, int32_t* dstatus /*[B]: 0 ok, 1 singular*/);
int blsq_cov(blsq_cov_plan* plan, const double* J, const int64_t* active, double* cov, double* rcond,
             int32_t* status);
/* The same for every problem of a device-resident outer driver, from its resident J (under a robust loss: diag(w) J,
 * scipy's `jac`); after blsq_outer_begin, normally once the loop has ended.  free_only != 0: the active variables are
 * dogbox's on_bound, and for 'trf' find_active_constraints(x, lb, ub, rtol = xtol) (trf.py:257) of the x that
 * blsq_outer_fetch returns.  Host outputs: only B n^2 + 2 B numbers leave the GPU. */
int blsq_outer_covariance(blsq_outer* o, int free_only, double* cov, double* rcond, int32_t* status);

/* ---- pseudo-inverse covariance (rank-deficient Jacobians, curve_fit's pcov) --------------------------------------
 * scipy.optimize.curve_fit (scipy 1.15.3 _minpack_py.py) takes the covariance from an SVD of the final Jacobian:
 *     _, s, VT = svd(res.jac, full_matrices=False)
 *     threshold = np.finfo(float).eps * max(res.jac.shape) * s[0]
 *     s = s[s > threshold];  VT = VT[:s.size]
 *     pcov = np.dot(VT.T / s**2, VT)
 * the Moore-Penrose inverse of J^T J over the singular values above the threshold.  Here, per problem: the Householder
 * triangle of J (or of J_F, as blsq_cov_dev) is rotated by the one-sided Jacobi SVD into rows s_i v_i^T, then
 *     rank[b]       = #{i : s_i > eps * max(m, |F|) * s_max};
 *     cov[b][F,F]   = scale[b] * sum_{kept i} v_i v_i^T / s_i^2, rows and columns of active variables exactly 0.0;
 *     rcond[b]      = s_min / s_max over all |F| values (not the 1-norm figure of blsq_cov_dev);
 *     kept_rcond[b] = (smallest kept s) / s_max.
 * status[b] = 0; 1 when a singular value or an entry of the triangle is not finite (scipy's svd raises there): cov[b]
 * is NaN everywhere, rank 0, rcond 0; 2 when the Jacobi SVD used all its sweeps without converging (cov[b] NaN as well).
 * J = 0 gives rank 0 and cov = 0, as the recipe does (rcond = kept_rcond = 0); |F| = 0 gives cov = 0, rank 0, rcond 1.
 * A Jacobian with fewer rows than columns is an ordinary rank-deficient input.  scale (dscale): [B] or NULL = 1; the
 * residual variance of curve_fit's absolute_sigma=False ("s_sq = cost / (ysize - p0.size); pcov = pcov * s_sq") goes
 * in here.  cov is exactly symmetric; a problem's bits do not depend on B or on its batch mates.  Shape limits and the
 * plan are those of blsq_cov_plan_create; a plan serves both kinds of call.
 * blsq_cov_pinv_dev: device pointers, asynchronous on the ctx stream, J is not modified.  blsq_cov_pinv: host pointers,
 * blocking. */
int blsq_cov_pinv_dev(blsq_cov_plan* plan, const double* dJ, const int64_t* dactive /*[B][n] or NULL*/,
                      const double* dscale /*[B] or NULL*/, double* dcov /*[B][n][n]*/, int32_t* drank /*[B]*/,
                      double* drcond /*[B]*/, double* dkept_rcond /*[B]*/, int32_t* dstatus /*[B]*/);
int blsq_cov_pinv(blsq_cov_plan* plan, const double* J, const int64_t* active, const double* scale, double* cov,
                  int32_t* rank, double* rcond, double* kept_rcond, int32_t* status);
/* The same on the resident J of an outer driver, under the rules of blsq_outer_covariance (robust loss: diag(w) J,
 * scaled once; free_only: dogbox's on_bound or the TRF mask of x).  variance_scale != 0: problem b is multiplied by
 * obj[b] / (m - n), obj the resident objective that blsq_outer_fetch returns (under a robust loss the loss objective,
 * scipy's 2 * cost; curve_fit: "cost = 2 * res.cost ... s_sq = cost / (ysize - p0.size)"); it needs m > n (argument
 * error otherwise: curve_fit fills pcov with inf there, which the caller does).  Host outputs: B n^2 + 4 B numbers. */
int blsq_outer_covariance_pinv(blsq_outer* o, int free_only, int variance_scale, double* cov, int32_t* rank,
                               double* rcond, double* kept_rcond, int32_t* status);
/* blsq_outer_covariance_pinv with the degrees of freedom of every problem (BLSQ_NAN_OMIT): problem b is
 * multiplied by obj[b] / (nobs[b] - n), nobs[b] the number of points it kept, and by +inf where nobs[b] <= n (its
 * covariance cannot be estimated: the caller fills it with inf; the batch mates are not affected).  nobs: host [B], each
 * in 0 .. m (argument error otherwise, as is NULL), uploaded once per call.  The rank tolerance keeps using the
 * allocated m.  Everything else as blsq_outer_covariance_pinv. */
int blsq_outer_covariance_pinv_nobs(blsq_outer* o, int free_only, const int32_t* nobs /*host [B]*/, double* cov,
                                    int32_t* rank, double* rcond, double* kept_rcond, int32_t* status);

/* ---- row forms through the covariance factor: leverages and prediction variances ---------------------------------
 * For every row a_i of a row-major matrix A [B][rows][n]:  out[b][i] = scale[b] * a_i C_b a_i^T  with C_b the (unscaled)
 * covariance the plan's LAST blsq_cov* / blsq_cov_pinv* call computed for problem b — evaluated through the factor
 * that call left in the plan, not through C: ||a_i[F] R^-1||^2 after blsq_cov*, sum_kept (v_k . a_i[F])^2 / s_k^2
 * after blsq_cov_pinv* (a dropped singular direction contributes exactly nothing).  With A = J these are the leverages
 * h_i = (J C J^T)_ii; with A a Jacobian at new points, times the residual variance, the variance of the fitted curve.
 * Columns of active variables (the mask of that covariance call) are never read.  scale NULL means 1; the scale of a
 * blsq_cov_pinv* call is NOT applied.  out[b][:] is NaN where that call's status[b] != 0 (the plan keeps its own copy
 * of the status) and exactly 0.0 where no variable is free.  `rows` is independent of the plan's m.  A row's bits
 * depend on that row, the problem's factor, and nothing else (not on B, the batch mates or rows).
 * Before any covariance call on the plan: a negative (bad argument) return, message "no covariance factor yet".
 * blsq_cov_rows_dev: device pointers, asynchronous on the ctx stream.  blsq_cov_rows: host pointers, blocking; A = NULL
 * means the J the last HOST-pointer covariance call staged (rows must then be the plan's m; an error if the last
 * covariance call was a device-pointer one). */
int blsq_cov_rows_dev(blsq_cov_plan* plan, int rows, const double* dA /*[B][rows][n]*/,
                      const double* dscale /*[B] or NULL*/, double* dout /*[B][rows]*/);
int blsq_cov_rows(blsq_cov_plan* plan, int rows, const double* A /*host, or NULL*/,
                  const double* scale /*host [B] or NULL*/, double* out /*host [B][rows]*/);
/* Leverages of the resident J of an outer driver through the factor of its last blsq_outer_covariance / _pinv call.
 * blsq_outer_start, _begin, _propose and _judge invalidate that factor: a stale or missing one is a bad-argument error,
 * nothing is recomputed silently.  status: the status that covariance call reported.  No scale is applied, even if that
 * call used variance_scale.  Host outputs: B m + B numbers. */
int blsq_outer_leverage(blsq_outer* o, double* h /*host [B][m]*/, int32_t* status /*host [B]*/);

#ifdef __cplusplus
}
#endif
#endif /* BLSQ_H */
