/* lasso_hip.h -- C ABI of the MI355X-native ISTA/FISTA sparse-encode engine.
 *
 * Drop-in boundary for the hot path of rfeinman/pytorch-lasso.
 * The reference has no FFI: its boundary is two Python call sites,
 *   lasso/linear/sparse_encode.py:62-63   ista(x, z0, weight, alpha, **kwargs)
 *   lasso/linear/dict_learning.py:38,39,45,47   E-step, objective, M-step
 * Each entry point below names the reference function it replaces.
 *
 * Conventions
 *   - every pointer named *_dev is DEVICE memory (HBM) owned by the caller; the
 *     library allocates nothing persistent and never frees caller memory;
 *   - matrices are row-major with an explicit leading dimension in ELEMENTS:
 *       X [n][d] (ldx), W [d][k] (ldw, atoms are columns), Z [n][k] (ldz);
 *   - layout contract, for every matrix that carries a leading dimension (ldx, ldw, ldz, ldz0, ldd, ldv, ldo, ldab,
 *     pool_ld, the ld of the patch calls, the ld*_in / ld*_out of lasso_fista_run, ldzt): ANY leading dimension >= the
 *     row length is accepted (a smaller one is LASSO_ERR_BAD_ARG before anything is enqueued), and a base pointer
 *     aligned to the ELEMENT is enough -- a sub-matrix of the caller's own allocation is a valid operand.  The kernels
 *     choose 16-byte vector loads / stores or LDS-DMA at run time, per operand, from the pitch AND the pointer; the
 *     result does not depend on that choice (same products, same order) except where a function says so.  The elements
 *     between the rows (ld - row length per row) are never read into a result -- they may hold NaN -- and never
 *     written.  Two functions ask for more and refuse, with a status and a text, before the first launch:
 *     lasso_fista_solve_sharded (ldz == k) and the lasso_mstep_pipe_* calls (16-byte aligned bases, pitches that are
 *     multiples of 4 floats); stated there;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); work is
 *     enqueued on it; a call only blocks the host where a host-visible result
 *     (iteration count, stop decision) is produced -- stated per function;
 *   - scratch and stream contract, for every function that takes (workspace_dev, workspace_bytes, stream):
 *       * the CONTENTS of the workspace on entry are unspecified.  Every word a call waits on, counts with, indexes
 *         with or accumulates into is written by that call, on `stream`, before it is read (a memset, or a launch in
 *         front that clears it); the bytes may be NaN patterns, another solver's state or this function's own last
 *         state, and the result -- tensors and every reported value -- is bit for bit the same;
 *       * workspace_bytes equal to what the function's *_workspace_bytes answers for the same shape is sufficient, and a
 *         larger buffer changes nothing: every region is placed from the shape, never from workspace_bytes;
 *       * nothing outside [workspace_dev, workspace_dev + the size function's answer) and the outputs named in the
 *         signature is written;
 *       * every launch, memset and copy of a call is enqueued on `stream`, and only there: a call made behind other work
 *         of that stream sees that work's results, whatever the null stream or any other stream is doing.  (The calls
 *         that name a second stream's word -- started_word, gate_word, lasso_stream_wait_word, the lasso_mstep_pipe_*
 *         family -- say so themselves.)
 *     Two kinds of workspace are exceptions, by name:
 *       * the lasso_mstep_pipe_* workspace is zeroed ONCE by the caller when it is allocated (its tickets and sequence
 *         words count up over the steps of a loop) and carries them from call to call;
 *       * the multi-call protocols keep state in their workspace between their calls, so its contents are unspecified
 *         only before the FIRST call and must be left alone until the last: lasso_fista_prepare -> lasso_fista_run
 *         (the packed dictionary and the momentum table); lasso_cd_prepare -> lasso_cd_run -> lasso_cd_finish (S, W^T,
 *         b, the tracked code, the rows' flags and counts); an asynchronous lasso_fista_solve (LASSO_PENDING*) ->
 *         lasso_fista_solve_deltas / _collect / _verdict / _verdict_mapped / _verdict_deferred / _finish (the
 *         per-iteration sums and the four result words); lasso_dict_sweep_async* -> lasso_dict_sweep_count.
 *     (tests/test_workspace_gpu.py holds every Python entry point to this on scratch filled with 0x00, 0xFF and 0x55,
 *     with 1 MiB + 4 bytes of room, between guard bands, and on a side stream whose operands arrive late.)
 *   - return value: lasso_status (0 = ok).  No exceptions cross the boundary;
 *     lasso_hip_last_error() gives the detail string for the calling thread;
 *   - dtype: LASSO_F32; LASSO_BF16 (x, W, z0, z_out all bf16, leading dimensions in bf16
 *     elements) is accepted by lasso_fista_solve on the fused shapes (bf16-MFMA kernels,
 *     fp32 accumulation and state; fixed step or line search) and LASSO_ERR_UNSUPPORTED
 *     elsewhere; LASSO_F64 (all tensors double, leading dimensions in doubles) is accepted by
 *     lasso_fista_workspace_bytes / _kernel_name / _solve (any d, k: fp64-MFMA general-GEMM path, csrc/gemm_f64.hip;
 *     every value, sum and comparison in IEEE double), lasso_lipschitz, lasso_objective(_throttled) and
 *     lasso_init_transpose, and LASSO_ERR_UNSUPPORTED elsewhere; results that an fp32 signature carries as
 *     float have double siblings (lasso_fista_solve_f64, lasso_objective_f64);
 *   - shapes: d <= 256 and k <= 1024 run the fused kernels; beyond that lasso_fista_solve
 *     (fixed step, and the line search on fp32 tensors), lasso_objective and
 *     lasso_gram_accumulate take any d, k (unfused MFMA GEMM paths), lasso_dict_sweep
 *     d <= 1024 and k <= 4096, lasso_cd_* k <= 4096; lasso_fista_prepare/_run take any
 *     d, k too (unfused: state in HBM, kernel_hint ignored); lasso_fista_solve_sharded takes
 *     any d, k on fp32 tensors (bf16: fused shapes only);
 *   - GPSR-Basic has two entry points on one driver: lasso_gpsr_solve (the dictionary as the operator) and
 *     lasso_conv_gpsr_solve (conv_transpose2d / conv2d as the operator, contiguous NCHW tensors); both LASSO_F32 only.
 *   - the orthant-wise Newton solver is lasso_own_solve: LASSO_F32, any n, d, any pitch, k <= 4096.
 *   - the OWL-QN solver is lasso_owlqn_solve: LASSO_F32, any n, d, k, any pitch, at most 1535 held pairs;
 *     lasso_owlqn_glm_solve is the same solver on the logistic loss (LASSO_GLM_BERNOULLI), same limits and workspace.
 *   - ISTA / FISTA through a one-layer decoder act(z W^T + b) is lasso_ista_nl_solve: LASSO_F32, any n, d, k, any pitch,
 *     identity / sigmoid / tanh / ReLU, a fixed step or the per-row power-iteration step.
 *   - the BFGS iterated-ridge solver is lasso_irbfgs_solve: LASSO_F32, any d, any pitch, k <= 1024, a workspace of
 *     2 n k^2 floats (lasso_irbfgs_update is its per-row update kernel on packed operands).
 *   - the iterated-ridge solver is lasso_iter_ridge_solve: LASSO_F32, any n, d, any pitch, k <= 1024.
 *   - the interior-point solver is lasso_interior_point_solve: LASSO_F32, any n, any pitch, d <= 256, k <= 4096.
 *   - the Split Bregman solver is lasso_split_bregman_solve: LASSO_F32, any n, d, any pitch, k <= 4096.
 *   - conjugate gradients are lasso_cg_solve (dense; LASSO_F32 or LASSO_F64, any n, k, any pitch) and
 *     lasso_conv_cg_solve (conv2d o conv_transpose2d + tik I; LASSO_F32, contiguous NCHW tensors).
 *   - one dense system per batch entry: lasso_batch_chol_solve and lasso_batch_lu_solve; LASSO_F32 (d <= 1024) or
 *     LASSO_F64 (d <= 512), any batch, any pitch.
 */
#ifndef LASSO_HIP_H_
#define LASSO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LASSO_HIP_ABI_VERSION 7

typedef enum {
  LASSO_OK = 0,
  LASSO_ERR_BAD_ARG = 1,      /* reference raises ValueError / AssertionError          */
  LASSO_ERR_UNSUPPORTED = 2,  /* shape or dtype outside what the HIP path implements   */
  LASSO_ERR_WORKSPACE = 3,    /* workspace missing or too small                        */
  LASSO_ERR_HIP = 4,          /* HIP runtime error (no device, launch failure, ...)    */
  LASSO_WARN_LINESEARCH = 5,  /* backtracking failed, reverted to lr0 (ista.py:48-52)  */
  LASSO_PENDING = 6,          /* LASSO_SOLVE_ASYNC: enqueued; call lasso_fista_solve_finish */
  LASSO_WARN_ABORTED = 7,     /* lasso_fista_solve_finish: the asynchronous solve must be repeated
                                 with LASSO_STOP_GLOBAL_CHUNKED -- the in-kernel stop rule gave up
                                 (a workgroup was not resident; z_out untouched), or the rule fired
                                 before the end of an asynchronously enqueued chunk (z_out holds a
                                 later iterate)                                            */
  LASSO_PENDING_DEFERRED = 9, /* LASSO_SOLVE_DEFER_VERDICT: enqueued WITHOUT the verdict's launch (lasso_fista_solve_verdict_deferred) */
  LASSO_PENDING_MAPPED = 8    /* LASSO_SOLVE_ASYNC | LASSO_SOLVE_STATUS_MAPPED: enqueued, and the verdict's
                                 four words will be written to the caller's mapped host buffer by the
                                 verdict kernel itself -- no lasso_fista_solve_collect needed          */
} lasso_status;

typedef enum { LASSO_F32 = 0, LASSO_BF16 = 1, LASSO_F64 = 2 } lasso_dtype;

/* How the global stopping rule of ista.py:93 is evaluated. */
typedef enum {
  LASSO_STOP_GLOBAL = 0,  /* exact reference rule: sum over the whole batch <= n*k*tol */
  LASSO_STOP_NONE = 1,    /* run exactly maxiter iterations (same as tol = 0)          */
  LASSO_STOP_GLOBAL_CHUNKED = 2  /* the same exact rule, but always evaluated by the
                             chunked speculate-and-replay path (no in-kernel handshake
                             between workgroups): for callers that share the GPU with
                             other streams / processes; LASSO_STOP_GLOBAL falls back to
                             it by itself when its workgroups are not all resident      */
} lasso_stop_mode;

/* Kernel-selection hint for the fused shapes: OR it into `stop_mode` of lasso_fista_solve, pass
 * it as `kernel_hint` to lasso_fista_run.  AUTO picks by batch size: the tile kernel (one
 * workgroup per 16-row tile, no traffic between workgroups) fills the chip from n ~ 16 x #CUs
 * rows; below that the split-k kernel shares each tile among Kpad/128 workgroups.  Both give
 * bitwise the same code for a row.  SPLITK is a request, not a guarantee (in-place calls,
 * d <= 128 tall tiles and lock-step stop-rule launches with more tiles than groups keep the
 * tile kernel). */
#define LASSO_KERNEL_AUTO 0
#define LASSO_KERNEL_TILE 0x100
#define LASSO_KERNEL_SPLITK 0x200
#define LASSO_KERNEL_UNFUSED 0x300   /* fixed-step fp32 solves: the general-GEMM path (state in HBM) also on the fused shapes */
/* tuning knob: split-k with exactly T = 1, 2 or 4 tiles per workgroup group (default: by cost model) */
#define LASSO_KERNEL_SPLITK_TILES(T) (0x200 | ((T) == 1 ? 0x1000 : (T) == 2 ? 0x2000 : 0x3000))
/* tuning knob (A/B measurements): split-k with the register-gather exchange for every T (the default streams the
 * partials of T >= 2 tiles through an LDS-DMA ring, csrc/fista_splitk.hip) */
#define LASSO_KERNEL_SPLITK_GATHER (0x200 | 0x400)
#define LASSO_KERNEL_MASK 0x3F00
/* OR into stop_mode of lasso_fista_solve (fp32, fixed step): do not wait for the stop rule's
 * outcome.  Returns LASSO_PENDING when the solve was enqueued without a wait -- the single
 * persistent launch with the in-kernel rule, or, with more tiles than resident workgroups, one
 * chunk of maxiter <= 64 iterations whose deltas are judged on the device -- (then iters_out /
 * last_delta_out are not written and lasso_fista_solve_finish / _collect fetch them), or
 * LASSO_OK when the solve completed inside the call (stop rule off, longer chunked solves). */
#define LASSO_SOLVE_ASYNC 0x4000
/* OR into stop_mode together with LASSO_SOLVE_ASYNC when the batch is a ROW SHARD of a larger one
 * (one process per GPU): the stop rule of ista.py:93 sums over the rows of ALL shards, so nothing
 * on this device can judge it alone.  The solve is enqueued as one chunk of maxiter <= 64 iterations
 * (LASSO_ERR_UNSUPPORTED beyond) that leaves this shard's per-iteration sums |z - z_next| in the
 * workspace and returns LASSO_PENDING; the caller all-reduces the `maxiter` floats at
 * lasso_fista_solve_deltas() across the ranks ON THE STREAM (RCCL), enqueues
 * lasso_fista_solve_verdict(n_global, ...) -- the one-thread kernel that applies the rule to the
 * summed vector -- and then lasso_fista_solve_collect() as for any other asynchronous solve.  No
 * host wait anywhere: every rank reads the same verdict ("redo" when the rule fired before the last
 * iteration) at its one synchronisation per EM step. */
#define LASSO_SOLVE_SHARDED 0x8000
/* OR into stop_mode together with LASSO_SOLVE_ASYNC when the rule is NOT expected to fire before `maxiter`
 * (<= 64) iterations -- the E-step of an EM loop: the solve is then always enqueued as one chunk on the plain
 * kernels and judged on the device (the in-kernel rule costs a cross-workgroup exchange per iteration that only
 * pays when it stops a long solve early).  Same words from lasso_fista_solve_finish / _collect; when the rule
 * does fire early they say "redo" (LASSO_WARN_ABORTED) exactly as for any other one-chunk solve. */
#define LASSO_SOLVE_ONE_CHUNK 0x10000
/* OR into stop_mode together with LASSO_SOLVE_ASYNC: `iters_out` is not a plain host int but FOUR int32 words of
 * device-writable host memory (pinned and mapped, e.g. hipHostMalloc / torch pin_memory()).  When the solve is
 * enqueued as one chunk judged on the device (always with LASSO_SOLVE_ONE_CHUNK; otherwise when the batch has more
 * tiles than resident workgroups) the verdict kernel writes {iterations, last delta (float bits), redo, 0} there
 * itself -- the fourth word, "valid" = 1, last and released -- and the call returns LASSO_PENDING_MAPPED: a host that
 * zeroed word 3 before the call POLLS it (or waits for an event recorded behind the call).  No copy launch, no
 * collect call and no event record on the step's dependent chain (round 6: copy + event cost ~10 us of every EM step;
 * an event record between two kernels of a stream is ~5 us by itself).  A solve that takes the in-kernel rule returns LASSO_PENDING as before
 * (the buffer is then not written; collect as usual). */
#define LASSO_SOLVE_STATUS_MAPPED 0x20000
#define LASSO_SOLVE_DEFER_VERDICT 0x40000 /* with STATUS_MAPPED | ONE_CHUNK: see lasso_fista_solve_verdict_deferred */
/* lr: the reference's lr='auto' (ista.py:72-73): 1 / lambda_max(W^T W) computed by the library on
 * the stream (csrc/lipschitz.hip).  The fp32 fixed-step kernels read the step from device
 * memory -- no host round trip; other paths synchronise once to fetch it. */
#define LASSO_LR_AUTO (-1.0)

int lasso_hip_abi_version(void);
const char* lasso_hip_status_string(int status);
const char* lasso_hip_last_error(void);

/* Number of compute units of the current HIP device (0 and LASSO_ERR_HIP if none). */
int lasso_hip_device_cus(int* cus_out);

/* Test hook.  The atom sweep (lasso_dict_sweep) and the Lipschitz squarings (lasso_lipschitz, LASSO_LR_AUTO) are
 * single launches of co-operating workgroups, each followed by a stand-by launch that redoes the work in ONE
 * workgroup when the grid could not get all its workgroups resident (and returns at once otherwise).  on != 0 makes
 * the library enqueue the stand-by form alone, so that a test can hold it against the co-operative one bit for bit
 * without having to saturate the GPU.  Returns the previous setting.  Process-wide; not for production use. */
int lasso_debug_force_standby(int on);

/* ---- FISTA / ISTA solve: replaces lasso/linear/solvers/ista.py:57-104 ------------
 *   min_z 0.5*||z W^T - x||^2 + alpha*||z||_1,  fixed step `lr`.
 *   z0_dev == NULL means zero initialisation (sparse_encode.py:22-23).
 *   fast != 0 -> FISTA (Nesterov momentum, ista.py:98-101), else ISTA.
 *   tol is the reference's RELATIVE tolerance; the absolute budget n*k*tol is
 *   formed inside (ista.py:64).  tol == 0 or stop_mode == LASSO_STOP_NONE runs
 *   exactly `maxiter` iterations with no host synchronisation.
 *   Otherwise the call synchronises `stream` once per chunk of iterations to
 *   evaluate the global stop rule exactly (speculate-and-replay).
 *   iters_out / last_delta_out (HOST pointers, nullable): iterations executed and
 *   the last evaluated sum|z - z_next| (only when the stop rule is active).
 *   trials_out / accepted_lr_out (HOST arrays of `maxiter` entries, nullable; written
 *   for the executed iterations when backtrack != 0): the number of line-search trials
 *   evaluated up to and including the accepted one, and the step size the iteration
 *   used -- the quantities ista.py:43-47 prints with verbose=True.  accepted_f_out (same
 *   shape): F(z_next) = 0.5*||z_next W^T - x||^2 + alpha*||z_next||_1 of the accepted trial
 *   (:28) -- divided by n it is the objective ista() prints for the NEXT iteration
 *   with verbose=True (:66-69,80-81), obtained without an extra pass over the data.
 *   objective_out (HOST float, nullable): mean objective (0.5*||x - z W^T||^2 +
 *   alpha*||z||_1)/n of the returned code, evaluated in fp32 (dict_learning.py:10-13,
 *   ista.py:66-69); synchronises `stream`.
 *   x, W, z0 are never written; z_out may alias z0.
 *   backtrack != 0: Beck-Teboulle backtracking line search (ista.py:17-54) from lr
 *   every outer iteration (the accepted step is discarded, ista.py:87), eta_backtrack
 *   > 1 (else LASSO_ERR_BAD_ARG, the reference's ValueError :18-19).  Line search and
 *   stop rule are global over the batch; the call synchronises `stream` once per outer
 *   iteration.  If no step is accepted within 1000 trials the iteration falls back to lr
 *   and the call returns LASSO_WARN_LINESEARCH after completing (ista.py:48-52).
 */
size_t lasso_fista_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype,
                                   int maxiter, double tol, int stop_mode, int backtrack);
/* Name of the device kernel lasso_fista_solve dispatches this problem to on the current
 * device (the name rocprofv3 --kernel-trace reports; for benchmark / profile bookkeeping). */
const char* lasso_fista_kernel_name(int64_t n, int64_t d, int64_t k, int dtype, int backtrack);

int lasso_fista_solve(const void* x_dev, int64_t ldx,
                      const void* w_dev, int64_t ldw,
                      const void* z0_dev, int64_t ldz0,
                      void* z_out_dev, int64_t ldz,
                      int64_t n, int64_t d, int64_t k, int dtype,
                      double alpha, double lr, int fast, int maxiter,
                      double tol, int stop_mode,
                      int backtrack, double eta_backtrack,
                      int32_t* iters_out, float* last_delta_out,
                      int32_t* trials_out, float* accepted_lr_out, float* accepted_f_out,
                      float* objective_out,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* lasso_fista_solve on float64 tensors (dtype LASSO_F64 is implied) with the host results as doubles: the last sum
 * |z - z_next|, the accepted step and F(z_next) per outer iteration, the mean objective.  lasso_fista_solve itself
 * accepts LASSO_F64 and runs the same solve, rounding these to its float slots.  Fixed step or line search, fast on /
 * off, z0 or NULL, tol > 0 (the stop rule compares double sums, once per chunk of speculated iterations),
 * lr = LASSO_LR_AUTO (one host round trip), any d, k.  stop_mode: LASSO_STOP_* only -- the asynchronous / sharded flags
 * and the LASSO_KERNEL_TILE / _SPLITK hints answer LASSO_ERR_UNSUPPORTED.  Two solves of the same arguments give
 * bitwise the same code.  Workspace: lasso_fista_workspace_bytes(..., LASSO_F64, ...). */
int lasso_fista_solve_f64(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw,
                          const void* z0_dev, int64_t ldz0, void* z_out_dev, int64_t ldz,
                          int64_t n, int64_t d, int64_t k,
                          double alpha, double lr, int fast, int maxiter, double tol, int stop_mode,
                          int backtrack, double eta_backtrack,
                          int32_t* iters_out, double* last_delta_out,
                          int32_t* trials_out, double* accepted_lr_out, double* accepted_f_out,
                          double* objective_out,
                          void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- building blocks for multi-GPU / custom drivers ---------------------------------
 * lasso_fista_prepare packs W into the padded layouts the kernels stream
 * (W [256][Kp] and W^T [Kp][256]) at the start of `workspace_dev` and builds the
 * momentum table of iterations 0 .. maxiter-1 (ista.py:98-99) behind them; the
 * workspace is sized by lasso_fista_workspace_bytes(n, d, k, dtype, maxiter, 0,
 * LASSO_STOP_NONE, 0) with n = the largest batch it will be used with.
 * lasso_fista_run executes `iters` iterations numbered it0 .. it0+iters-1 (< maxiter, the
 * value given to prepare) of the
 * momentum schedule from state (z_in, y_in) to (z_out, y_out) and writes
 * delta_dev[i] = sum over THIS shard of |z - z_next| for each executed iteration
 * (device array of `iters` floats, nullable).  No host synchronisation.
 * y_in_dev == NULL means y = z_in (start of a solve); y_out_dev may be NULL.
 */
int lasso_fista_prepare(const void* w_dev, int64_t ldw, int64_t d, int64_t k, int dtype, int maxiter,
                        void* workspace_dev, size_t workspace_bytes, void* stream);

int lasso_fista_run(const void* x_dev, int64_t ldx,
                    const void* z_in_dev, int64_t ldz_in,
                    const void* y_in_dev, int64_t ldy_in,
                    void* z_out_dev, int64_t ldz_out,
                    void* y_out_dev, int64_t ldy_out,
                    int64_t n, int64_t d, int64_t k, int dtype,
                    double alpha, double lr, int fast, int it0, int iters, int maxiter,
                    int kernel_hint, float* delta_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Lipschitz constant: replaces _lipschitz_constant, ista.py:8-14 -----------------
 * L = lambda_max(W^T W) of an fp32 or float64 (LASSO_F64) dictionary, deterministic, fp64, computed on the device (Gram of the
 * smaller side + repeated squaring; see csrc/lipschitz.hip).  Synchronises `stream`
 * to return the value through the HOST pointer l_out (the reference returns a python
 * float the same way).  ((double*)workspace_dev)[0] also holds the value on the device.
 */
size_t lasso_lipschitz_workspace_bytes(int64_t d, int64_t k);
int lasso_lipschitz(const void* w_dev, int64_t ldw, int64_t d, int64_t k, int dtype,
                    double* l_out, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- objective: replaces lasso_loss, dict_learning.py:10-13 ------------------------
 * loss = (0.5*||X - Z W^T||^2 + alpha*||Z||_1) / n.  No host synchronisation:
 * loss_dev (device float, nullable) receives the scalar for THIS shard's n;
 * sums_dev (device double[2], nullable) receives {sum r^2, sum |z|} of the shard so a
 * multi-GPU driver can all-reduce them and normalise by the global n.
 */
size_t lasso_objective_workspace_bytes(int64_t n, int64_t d, int64_t k);
int lasso_objective(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw,
                    const void* z_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype,
                    double alpha, float* loss_dev, double* sums_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);
/* lasso_objective on at most `max_workgroups` workgroups of the fused kernel (0 = no cap): for callers that run it
 * beside latency-bound work of another stream (ABI 7; the EM loop's objective beside the atom sweep). */
int lasso_objective_throttled(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw,
                              const void* z_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype,
                              double alpha, float* loss_dev, double* sums_dev, int max_workgroups,
                              void* workspace_dev, size_t workspace_bytes, void* stream);

/* float64 tensors: lasso_objective / _throttled accept LASSO_F64 with a workspace of
 * lasso_objective_f64_workspace_bytes and round the loss to the float at loss_dev (max_workgroups does not apply);
 * lasso_objective_f64 leaves it as a device double.  The residual, both sums and the loss are computed in double. */
size_t lasso_objective_f64_workspace_bytes(int64_t n, int64_t d, int64_t k);
int lasso_objective_f64(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw,
                        const void* z_dev, int64_t ldz, int64_t n, int64_t d, int64_t k,
                        double alpha, double* loss_dev, double* sums_dev,
                        void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- constrained M-step in Gram form: replaces update_dict, dict_learning.py:56-103 --
 * lasso_gram_accumulate: A = Z^T Z [k][k] (ld k), B = Z^T X [k][d] (ld d) of this row
 *   shard (fp32 MFMA).  The caller all-reduces A and B across GPUs (they may be two
 *   slices of one buffer).  The workspace (optional, may be NULL) holds the partial
 *   products of the sample splits that keep all CUs busy; they are summed in a fixed
 *   order, so the result is deterministic either way.
 * lasso_dict_sweep: Gauss-Seidel sweep over the atoms on (A, B), updating the
 *   dictionary D [d][k] (ldd) IN PLACE like the reference (:86,:100).  Atoms with
 *   ||u|| < eps (:92) are replaced by the next unused row of `pool_dev`
 *   [pool_rows][d] (ld pool_ld) normalised to unit length -- the reference draws that
 *   direction from torch's RNG (:93) -- or, if pool_dev is NULL, by a counter-based
 *   N(0,1) vector keyed by (seed, atom).  degenerate_dev [k] (int32, device) is set to
 *   1 for those atoms; ndeg_out (HOST, nullable) receives their count and, when
 *   non-NULL, makes the call synchronise `stream`.
 * lasso_dict_sweep_count: device address (inside the sweep's workspace) of that count, for callers that pass
 *   ndeg_out = NULL and read it at their own synchronisation (4 bytes instead of a reduction over the k flags);
 *   NULL for arguments lasso_dict_sweep would reject.
 * lasso_dict_fill_degenerate: deferred form of that replacement for drivers that want to
 *   draw directions only when an atom actually degenerated (the sweep never READS a
 *   replacement -- the degenerate atom leaves the model): call lasso_dict_sweep with
 *   pool_dev == NULL, and if ndeg > 0 draw ndeg directions [ndeg][d] and pass them here;
 *   the i-th flagged atom (atom order) becomes pool row i, clamped at 0 if `positive`,
 *   normalised (:93-96).
 * lasso_zero_columns: Z[:, j] = 0 where degenerate_dev[j] != 0 (:98).
 * Layout: lasso_gram_accumulate runs its 256- and 128-wide block kernels when z_dev and x_dev are 16-byte aligned with
 *   pitches that are multiples of 4 floats, and 32-wide blocks with scalar loads otherwise: other sample splits, so A
 *   and B differ in the last bits between the two (each is deterministic, A exactly symmetric, either way).  The sweep's
 *   dictionary does not depend on ldd / ldo / pool_ld or on the alignment of d_dev.
 */
size_t lasso_gram_workspace_bytes(int64_t n, int64_t d, int64_t k);
int lasso_gram_accumulate(const void* z_dev, int64_t ldz, const void* x_dev, int64_t ldx,
                          int64_t n, int64_t d, int64_t k, int dtype,
                          float* a_dev, float* b_dev,
                          void* workspace_dev, size_t workspace_bytes, void* stream);
/* lasso_gram_accumulate whose first launch writes *started_word = started_value (device memory) as it STARTS: everything
 * enqueued on `stream` before the call has completed by then.  A start signal for work on ANOTHER stream
 * (lasso_stream_wait_word polls the word) that costs this stream nothing -- an event record between two kernels is ~5 us. */
int lasso_gram_accumulate_signal(const void* z_dev, int64_t ldz, const void* x_dev, int64_t ldx,
                                 int64_t n, int64_t d, int64_t k, int dtype, float* a_dev, float* b_dev,
                                 void* workspace_dev, size_t workspace_bytes, int32_t* started_word,
                                 int32_t started_value, void* stream);
size_t lasso_dict_sweep_workspace_bytes(int64_t d, int64_t k);
int lasso_dict_sweep(const float* a_dev, const float* b_dev, void* d_dev, int64_t ldd,
                     int64_t d, int64_t k, int dtype, double eps, int positive,
                     const float* pool_dev, int64_t pool_rows, int64_t pool_ld, uint64_t seed,
                     int32_t* degenerate_dev, int32_t* ndeg_out,
                     void* workspace_dev, size_t workspace_bytes, void* stream);
int32_t* lasso_dict_sweep_count(int64_t d, int64_t k, void* workspace_dev, size_t workspace_bytes);

/* lasso_dict_sweep without a host wait (ABI 7): the count of degenerate atoms is written by the sweep's last kernel to
 * `ndeg_mapped`, TWO int32 words of device-writable host memory (pinned, mapped): {count, 1}, the second written last
 * and released -- a host that zeroed it before the call polls it (or waits for an event recorded behind the call).  Replaces the copy of lasso_dict_sweep_count()'s word on the EM step's dependent chain. */
int lasso_dict_sweep_async(const float* a_dev, const float* b_dev, void* d_dev, int64_t ldd,
                           int64_t d, int64_t k, int dtype, double eps, int positive,
                           const float* pool_dev, int64_t pool_rows, int64_t pool_ld, uint64_t seed,
                           int32_t* degenerate_dev, int32_t* ndeg_mapped, void* workspace_dev,
                           size_t workspace_bytes, void* stream);

/* lasso_dict_sweep_async with the new dictionary written to ANOTHER buffer (d_out_dev, pitch ldo >= k, not overlapping
 * d_dev): d_dev is only read.  The call may then be enqueued BEFORE the host knows whether the EM step it belongs to
 * stands (the E-step's verdict, the previous sweep's count of degenerate atoms) -- a step that is repeated keeps d_dev
 * and ignores d_out_dev, degenerate_dev and ndeg_mapped -- and launches on another stream may keep reading d_dev beside
 * it (the objective of dict_learning.py:39).  started_word (nullable, device memory): set to started_value by a launch
 * in front of the sweep itself -- "the sweep starts now" for a wave of another stream (lasso_stream_wait_word) whose work
 * should run beside it.  Same kernels, same arithmetic: bitwise the dictionary of lasso_dict_sweep.
 * Replaces the in-place update of dict_learning.py:83-91 where the caller double-buffers the dictionary. */
int lasso_dict_sweep_async_to(const float* a_dev, const float* b_dev, const void* d_dev, int64_t ldd,
                              void* d_out_dev, int64_t ldo, int64_t d, int64_t k, int dtype, double eps, int positive,
                              const float* pool_dev, int64_t pool_rows, int64_t pool_ld, uint64_t seed,
                              int32_t* degenerate_dev, int32_t* ndeg_mapped, int32_t* started_word,
                              int32_t started_value, void* workspace_dev, size_t workspace_bytes, void* stream);

/* One wave on `stream` that returns when a word of device memory has reached `value` (*word >= value: such words count
 * up) -- or, host_memory != 0, when a word of pinned host memory (e.g. the "valid" word of a LASSO_SOLVE_STATUS_MAPPED
 * buffer) equals `value` -- or after ~20 s (host memory: ~0.1 s): "after that kernel of ANOTHER stream" for the
 * launches behind it without an event record on the other stream.  A scheduling tool: a launch behind it whose DATA
 * depend on the order must check the word itself (lasso_fista_solve_verdict_deferred's gate).  Polling host memory
 * slows kernels running beside the wave (measured: an E-step by 12-19 %); polling device memory does not. */
int lasso_stream_wait_word(const int32_t* word, int32_t value, int host_memory, void* stream);

/* ---- Pipelined constrained M-step (ABI 7; dict_learning.py:44-45,82-101 in Gram form) -------------
 * The sweep of atom block b needs rows b of A = Z^T Z and of U = B - A D^T only, and walks the blocks far slower
 * than the chip produces them.  For d == 256, k a multiple of 256 (512 ... 4096) the M-step therefore exists in a
 * form that overlaps the two: [A | B] is produced in STAGES of whole block rows (256 atoms each) into ONE matrix
 * ab [k][k + d] (A in columns 0 .. k-1, B behind it, row pitch ldab >= k + d); stage 0 (the head: the first half of
 * the block rows) before the sweep starts, the others on a SECOND stream while the sweep runs -- its workgroups wait,
 * block by block, for the rows they need.  Per EM step, with `stages = lasso_mstep_pipe_stages(n, d, k)` (0: no
 * pipelined form, use lasso_gram_accumulate + lasso_dict_sweep) and stage s covering rows
 * lasso_mstep_pipe_stage_rows(s) of ab:
 *     stream M:  pipe_gram(0) [all-reduce the head's rows of ab] pipe_rows(0, seq)                pipe_sweep ... pipe_finish
 *     stream S:  pipe_wait(seq)   for s = 1 .. stages-1: pipe_gram(s) [all-reduce stage s' rows] pipe_rows(s)
 * with everything of stream S ENQUEUED before pipe_sweep (if the two streams ever share a hardware queue the sweep
 * then simply runs behind its producers) and pipe_finish -- the only call that changes the dictionary -- after
 * whatever still reads the old one.  A stage's rows of ab are contiguous: one collective per stage, the first on the
 * critical chain, the others hidden behind the sweep.  All calls of one step take the SAME workspace
 * (lasso_mstep_pipe_workspace_bytes; caller-owned, shared by both streams, ZEROED once before its first use).
 * Results: the dictionary of lasso_dict_sweep on the same (A, B) bit for bit -- the same products in the same order --;
 * A and B themselves differ from lasso_gram_accumulate's in the last bits (other sample splits, hence another
 * summation order).
 * Layout (stricter than the library's general contract -- these kernels have 16-byte vector forms only): ab_dev, and in
 * lasso_mstep_pipe_gram z_dev and x_dev (n > 0), in lasso_mstep_pipe_rows and _sweep d_dev, must be 16-byte aligned with
 * pitches (ldab, ldz, ldx, ldd) that are multiples of 4 floats; lasso_mstep_pipe_sweep reads ab_dev element-wise (any ldab >=
 * k + d, any alignment) and lasso_mstep_pipe_finish writes d_dev element-wise (any ldd >= k).  Anything else answers
 * LASSO_ERR_BAD_ARG with the rule in the text, before the shape is looked at and before anything is enqueued. */
int lasso_mstep_pipe_stages(int64_t n, int64_t d, int64_t k);
int lasso_mstep_pipe_stage_rows(int64_t n, int64_t d, int64_t k, int stage, int64_t* row_lo, int64_t* row_hi);
size_t lasso_mstep_pipe_workspace_bytes(int64_t n, int64_t d, int64_t k);
/* the stage's rows of [A | B] from this process's n samples: per block row R the columns >= 256 R computed and folded,
 * the blocks right of the diagonal also written transposed into the rows below (after the stages 0 .. s the rows of
 * stage s are complete).  Stage 0 also resets the sweep's flag words.  n == 0 (a rank without rows, which still runs the
 * identical sweep on the all-reduced matrix): the stage's rows are zeroed, the flag words reset all the same. */
int lasso_mstep_pipe_gram(const void* z_dev, int64_t ldz, const void* x_dev, int64_t ldx, int64_t n, int64_t d,
                          int64_t k, int dtype, float* ab_dev, int64_t ldab, int stage, void* workspace_dev,
                          size_t workspace_bytes, void* stream);
/* "after the head" for stream S without an event record on stream M (an event between two kernels of a stream costs
 * ~5 us there): pipe_rows(0, seq) leaves `seq` (any value that differs from the previous step's) in a word of the
 * workspace when its last workgroup finishes; this call enqueues ONE wave that returns when it reads `seq` there (or
 * after ~0.1 s: the ordering is a scheduling matter -- launches of the later stages in front of the head's would only
 * take compute units from it -- no data depends on it). */
int lasso_mstep_pipe_wait(int64_t n, int64_t d, int64_t k, int seq, void* workspace_dev, size_t workspace_bytes,
                          void* stream);
/* the word lasso_mstep_pipe_wait polls (device memory inside the workspace; NULL if the shape has no pipelined M-step):
 * for launches behind that wait which must re-check it (the gate of lasso_fista_solve_verdict_deferred) */
const int32_t* lasso_mstep_pipe_head_word(int64_t n, int64_t d, int64_t k, void* workspace_dev, size_t workspace_bytes);
/* U rows of the stage (B - A D^T with the dictionary as it is BEFORE the sweep); its last workgroup raises the
 * "complete" words of the stage's block rows for the running sweep (stage 0: writes `seq` for lasso_mstep_pipe_wait). */
int lasso_mstep_pipe_rows(const float* ab_dev, int64_t ldab, const void* d_dev, int64_t ldd, int64_t n, int64_t d,
                          int64_t k, int dtype, int stage, int seq, void* workspace_dev, size_t workspace_bytes,
                          void* stream);
/* the sweep (one launch of co-operating workgroups + its stand-by); new atoms stay in the workspace, d_dev is only read */
int lasso_mstep_pipe_sweep(const float* ab_dev, int64_t ldab, const void* d_dev, int64_t ldd, int64_t n, int64_t d,
                           int64_t k, int dtype, double eps, int positive, int32_t* degenerate_dev, void* workspace_dev,
                           size_t workspace_bytes, void* stream);
/* (on stream S, behind its last launch that reads the old dictionary) one thread that writes `seq` to the workspace
 * word lasso_mstep_pipe_finish(wait_seq = seq) waits for */
int lasso_mstep_pipe_signal(int64_t n, int64_t d, int64_t k, int seq, void* workspace_dev, size_t workspace_bytes,
                            void* stream);
/* writes the new dictionary (degenerate atoms re-drawn from the counter-based generator, flagged in degenerate_dev as
 * by lasso_dict_sweep); `ndeg_mapped` (nullable): {count, valid} in device-writable host memory, as
 * lasso_dict_sweep_async.  wait_seq != 0: the kernel itself waits (up to ~0.3 s) for lasso_mstep_pipe_signal(wait_seq)
 * before it touches the dictionary -- instead of a cross-stream event wait in front of the launch (6-10 us on the
 * step's chain); if the word never arrives the count comes back as -1 and the caller must treat the step as failed.
 * wait_seq == 0: the caller has ordered the launch behind stream S itself. */
int lasso_mstep_pipe_finish(void* d_dev, int64_t ldd, int64_t n, int64_t d, int64_t k, int dtype, double eps, int positive,
                            int32_t* degenerate_dev, int32_t* ndeg_mapped, int wait_seq, void* workspace_dev,
                            size_t workspace_bytes, void* stream);
int lasso_dict_fill_degenerate(void* d_dev, int64_t ldd, int64_t d, int64_t k, int dtype,
                               const int32_t* degenerate_dev, const float* pool_dev, int64_t pool_rows,
                               int64_t pool_ld, int positive, void* stream);
int lasso_zero_columns(void* z_dev, int64_t ldz, int64_t n, int64_t k, int dtype,
                       const int32_t* degenerate_dev, void* stream);

/* Second half of a LASSO_SOLVE_ASYNC solve that returned LASSO_PENDING (same n, d, k, dtype,
 * maxiter, tol, workspace, stream): synchronises the stream, writes iters_out / last_delta_out
 * (HOST, nullable).  LASSO_OK, or LASSO_WARN_ABORTED (see above).  Work enqueued between the
 * two calls (lasso_objective, lasso_gram_accumulate on z_out ...) overlaps the wait. */
/* ---- line search on a ROW SHARD (one process per GPU): replaces the global reductions of
 * ista.py:23,28,32-35 (F <= Q of each trial) and :93 (stop rule) -------------------------
 * Same arguments as lasso_fista_solve with backtrack = 1 on the n rows this process holds
 * (n_global = rows of the whole batch, for the stop budget).  Wherever the reference reduces over
 * the batch the library hands `reduce` a small array of this rank's sums (doubles, HOST memory)
 * to be replaced IN PLACE by their sum over all ranks (return 0; anything else aborts the solve
 * with LASSO_ERR_HIP) -- e.g. an MPI_Allreduce / torch.distributed.all_reduce of `count`
 * doubles.  Every rank must call with the same lr, eta, maxiter, tol: the callback is then
 * invoked the same number of times with the same counts on every rank, and all ranks take the
 * same decisions (trials_out / accepted_lr_out / accepted_f_out are identical everywhere).
 * Workspace: lasso_fista_workspace_bytes(n, d, k, dtype, maxiter, tol, LASSO_STOP_GLOBAL, 1).
 * Requires ldz == k (z_out is the line search's flat [n][k] state; x, W, z0 take any layout): any other ldz answers
 * LASSO_ERR_UNSUPPORTED "row-sharded line search needs ldz == k" before the first launch, z_out untouched. */
typedef int (*lasso_allreduce_fn)(void* ctx, double* sums, int count);
int lasso_fista_solve_sharded(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw,
                              const void* z0_dev, int64_t ldz0, void* z_out_dev, int64_t ldz,
                              int64_t n, int64_t n_global, int64_t d, int64_t k, int dtype,
                              double alpha, double lr, int fast, int maxiter, double tol,
                              double eta_backtrack, lasso_allreduce_fn reduce, void* reduce_ctx,
                              int32_t* iters_out, float* last_delta_out, int32_t* trials_out,
                              float* accepted_lr_out, float* accepted_f_out, void* workspace_dev,
                              size_t workspace_bytes, void* stream);

/* The asynchronous form: only ENQUEUES the copy of {iterations, last delta (float bits), aborted
 * != 0, 0} into out4_host (HOST; pinned memory keeps the copy asynchronous).  The caller waits
 * on the stream -- or on an event recorded right behind this call, so that work enqueued after
 * it keeps the GPU busy during the wait -- and decodes the four words itself. */
int lasso_fista_solve_collect(int64_t n, int64_t d, int64_t k, int dtype, int maxiter, double tol,
                              int32_t* out4_host, void* workspace_dev, size_t workspace_bytes,
                              void* stream);
/* LASSO_SOLVE_SHARDED: the device address (inside the workspace) of the pending solve's `maxiter`
 * per-iteration sums, to be all-reduced in place; NULL when the arguments describe no such solve. */
float* lasso_fista_solve_deltas(int64_t n, int64_t d, int64_t k, int dtype, int maxiter, double tol,
                                void* workspace_dev, size_t workspace_bytes);
/* LASSO_SOLVE_SHARDED: enqueue the stop rule over the (all-reduced) sums with the budget
 * n_global * k * tol of the whole batch (ista.py:64); lasso_fista_solve_collect fetches its words.
 * sums_dev: the `maxiter` all-reduced sums, or NULL when they were reduced in place at
 * lasso_fista_solve_deltas() (a driver may carry them in the tail of its M-step message instead: the
 * EM step then has ONE collective). */
int lasso_fista_solve_verdict(int64_t n, int64_t n_global, int64_t d, int64_t k, int dtype, int maxiter,
                              double tol, const float* sums_dev, void* workspace_dev, size_t workspace_bytes,
                              void* stream);
/* lasso_fista_solve_verdict + the four words written to `status_mapped` (device-writable host memory, as
 * LASSO_SOLVE_STATUS_MAPPED) by the verdict kernel: no lasso_fista_solve_collect behind it (ABI 7). */
int lasso_fista_solve_verdict_mapped(int64_t n, int64_t n_global, int64_t d, int64_t k, int dtype, int maxiter,
                                     double tol, const float* sums_dev, int32_t* status_mapped, void* workspace_dev,
                                     size_t workspace_bytes, void* stream);
/* LASSO_SOLVE_DEFER_VERDICT (with LASSO_SOLVE_ASYNC | LASSO_SOLVE_ONE_CHUNK | LASSO_SOLVE_STATUS_MAPPED, not with
 * LASSO_SOLVE_SHARDED): the solve enqueues its kernels but NOT the launch that reduces the per-iteration sums and judges
 * the stop rule (ista.py:93-95), and returns LASSO_PENDING_DEFERRED; this call enqueues that launch on `stream`, which the
 * caller has ordered behind the solve's kernels without touching the solve's stream -- e.g. behind lasso_stream_wait_word
 * on the word lasso_gram_accumulate_signal raises.  An EM step's dependent chain (E-step -> Gram product -> sweep) is
 * then one launch shorter; same kernel, same sums, same four words in `status_mapped`.  The arguments are kept per host
 * thread, one solve at a time: call it from the thread that enqueued the solve, with that solve's workspace, before the
 * thread's next LASSO_SOLVE_ASYNC solve.  A solve that cannot defer (maxiter > 64) returns LASSO_PENDING_MAPPED as
 * without the flag.  gate_word (nullable, device memory): the word the stream's wait polled -- the launch re-checks
 * *gate_word == gate_value and, if the wait ran into its bound instead, reports "repeat the solve" (status word 2 = 1)
 * rather than judging sums of kernels that may still be running. */
int lasso_fista_solve_verdict_deferred(void* workspace_dev, int32_t* status_mapped, const int32_t* gate_word,
                                       int32_t gate_value, void* stream);
int lasso_fista_solve_finish(int64_t n, int64_t d, int64_t k, int dtype, int maxiter, double tol,
                             int32_t* iters_out, float* last_delta_out, void* workspace_dev,
                             size_t workspace_bytes, void* stream);

/* ---- init='transpose': replaces torch.matmul(x, weight), sparse_encode.py:24-25 ---------
 * z0 [n][k] (ldz) = x [n][d] W [d][k] on the library's fp32-MFMA NT GEMM (csrc/gemm.hip); LASSO_F64: on the
 * fp64-MFMA GEMM (csrc/gemm_f64.hip).
 */
size_t lasso_init_transpose_workspace_bytes(int64_t d, int64_t k);
int lasso_init_transpose(int64_t n, int64_t d, int64_t k, int dtype, const void* x_dev, int64_t ldx,
                         const void* w_dev, int64_t ldw, void* z0_dev, int64_t ldz,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- unconstrained M-step: replaces update_dict_ridge, dict_learning.py:106-123 ----------
 * V [d][k] (ldv) = ((A + lambda_n I)^-1 B)^T with A = Z^T Z, B = Z^T X from
 * lasso_gram_accumulate (all-reduced by the caller across GPUs) and lambda_n = lambd * n
 * (:119).  Blocked Cholesky + the two triangular solves on the library's own fp32-MFMA
 * kernels (csrc/ridge.hip); k <= 4096 (lasso_ridge_workspace_bytes returns 0 beyond).  A and B are not modified.  info_out (HOST, nullable):
 * 0, or 1 + the index of the first non-positive pivot (then LASSO_ERR_BAD_ARG; torch raises
 * in linalg.cholesky there); a non-NULL info_out makes the call synchronise `stream`.
 */
size_t lasso_ridge_workspace_bytes(int64_t d, int64_t k);
int lasso_ridge_solve(const float* a_dev, const float* b_dev, void* v_dev, int64_t ldv,
                      int64_t d, int64_t k, int dtype, double lambda_n, int32_t* info_out,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- float64 M-step: update_dict / update_dict_ridge (dict_learning.py:56-123) on float64 tensors ----------------
 * The M-step entry points above keep answering LASSO_ERR_UNSUPPORTED to LASSO_F64 (their A and B are float*); these
 * are their siblings with double matrices and no dtype argument (csrc/mstep_f64.hip).  Every product runs on the
 * fp64 MFMA, every value, norm, pivot and comparison is an IEEE double, no sum uses atomics: two calls with the same
 * arguments give the same bits.  Null pointers and non-positive sizes answer LASSO_ERR_BAD_ARG before any HIP call.
 * lasso_gram_accumulate_f64: A = Z^T Z [k][k] (ld k, symmetric bit for bit), B = Z^T X [k][d] (ld d) of the n >= 1
 *   rows; any d, k, ldz >= k, ldx >= d.  The workspace (optional, may be NULL) holds the partial products of the row
 *   slabs a large n is split into; they are summed in slab order.
 * lasso_dict_sweep_f64: the Gauss-Seidel atom sweep of lasso_dict_sweep on (A, B), D [d][k] (ldd) updated in place;
 *   d <= 1024, k <= 4096 (LASSO_ERR_UNSUPPORTED beyond, the workspace query returns 0).  An atom with ||u|| < eps is
 *   flagged in degenerate_dev [k] (int32, every word written) and leaves the model (its column of D is zero until
 *   lasso_dict_fill_degenerate_f64 replaces it -- the deferred form only: there is no pool argument).  ndeg_out
 *   (HOST, nullable) receives the count of flagged atoms and, when non-NULL, makes the call synchronise `stream`.
 * lasso_dict_fill_degenerate_f64: the i-th flagged atom (atom order) becomes row i of pool_dev [pool_rows][d]
 *   (ld pool_ld, double), clamped at 0 if `positive`, divided by its norm (:93-96).
 * lasso_zero_columns_f64: Z[:, j] = 0 where degenerate_dev[j] != 0 (:98).
 * lasso_ridge_solve_f64: V [d][k] (ldv) = ((A + lambda_n I)^-1 B)^T by a blocked Cholesky factorisation with B^T
 *   carried along and a back substitution; k <= 4096 (lasso_ridge_f64_workspace_bytes returns 0 beyond).  A and B are
 *   not modified.  info_out (HOST, nullable): 0, or 1 + the index of the first pivot that is not positive (then
 *   LASSO_ERR_BAD_ARG); a non-NULL info_out makes the call synchronise `stream`. */
size_t lasso_gram_f64_workspace_bytes(int64_t n, int64_t d, int64_t k);
int lasso_gram_accumulate_f64(const double* z_dev, int64_t ldz, const double* x_dev, int64_t ldx,
                              int64_t n, int64_t d, int64_t k, double* a_dev, double* b_dev,
                              void* workspace_dev, size_t workspace_bytes, void* stream);
size_t lasso_dict_sweep_f64_workspace_bytes(int64_t d, int64_t k);
int lasso_dict_sweep_f64(const double* a_dev, const double* b_dev, double* d_dev, int64_t ldd,
                         int64_t d, int64_t k, double eps, int positive,
                         int32_t* degenerate_dev, int32_t* ndeg_out,
                         void* workspace_dev, size_t workspace_bytes, void* stream);
int lasso_dict_fill_degenerate_f64(double* d_dev, int64_t ldd, int64_t d, int64_t k,
                                   const int32_t* degenerate_dev, const double* pool_dev, int64_t pool_rows,
                                   int64_t pool_ld, int positive, void* stream);
int lasso_zero_columns_f64(double* z_dev, int64_t ldz, int64_t n, int64_t k,
                           const int32_t* degenerate_dev, void* stream);
size_t lasso_ridge_f64_workspace_bytes(int64_t d, int64_t k);
int lasso_ridge_solve_f64(const double* a_dev, const double* b_dev, double* v_dev, int64_t ldv,
                          int64_t d, int64_t k, double lambda_n, int32_t* info_out,
                          void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- greedy coordinate descent: replaces coord_descent(),
 *      lasso/linear/solvers/coordinate_descent.py:5-54 (sparse_encode.py:54-55) --------
 * Per row: b = x W (:19, independent of z0), tracked z = z0 or 0 (:10-14); per step
 * propose S_alpha(b), commit the coordinate with the largest |proposal - z| (first index
 * on ties), b += (I - W^T W)[:, j] * change (:31-39); the row stops once its committed
 * change is <= tol*k (:9,45-48) or after maxiter steps.  z_out = S_alpha(b) (:52).
 *   lasso_cd_prepare : S, b and the per-row state into the workspace.
 *   lasso_cd_run     : up to `iters` further steps for every still-active row
 *                      (tol_abs is already tol*k).  n_active_out / max_steps_out are HOST
 *                      pointers (nullable); when either is given the call synchronises.
 *   lasso_cd_finish  : z_out = S_alpha(b); z_track_out (nullable) receives the tracked z
 *                      (the reference updates a caller-supplied z0 IN PLACE, :14,47).
 *   lasso_cd_solve   : prepare + run(maxiter) + finish; z0_inout may be NULL (zero init),
 *                      otherwise it is overwritten with the tracked z like the reference.
 * The workspace carries the state between the calls and must not be touched in between.
 * k <= 4096; any d.  Rows are independent: a row shard needs no collective.
 */
size_t lasso_cd_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype);
int lasso_cd_prepare(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw,
                     const void* z0_dev, int64_t ldz0, int64_t n, int64_t d, int64_t k, int dtype,
                     void* workspace_dev, size_t workspace_bytes, void* stream);
int lasso_cd_run(int64_t n, int64_t d, int64_t k, double alpha, double tol_abs, int iters,
                 int32_t* n_active_out, int32_t* max_steps_out,
                 void* workspace_dev, size_t workspace_bytes, void* stream);
int lasso_cd_finish(void* z_out_dev, int64_t ldz, void* z_track_out_dev, int64_t ldzt,
                    int64_t n, int64_t d, int64_t k, double alpha,
                    void* workspace_dev, size_t workspace_bytes, void* stream);
int lasso_cd_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw,
                   void* z0_inout_dev, int64_t ldz0, void* z_out_dev, int64_t ldz,
                   int64_t n, int64_t d, int64_t k, int dtype, double alpha, int maxiter, double tol,
                   int32_t* n_active_out, int32_t* max_steps_out,
                   void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- cyclic coordinate descent with a duality-gap stop: replaces coord_descent_mod(),
 *      lasso/linear/solvers/coordinate_descent.py:57-139 (after sklearn's enet_coordinate_descent) ----
 * Per row, sweeps over the atoms in order: z_i <- S_alpha(R . w_i + ||w_i||^2 z_i) / ||w_i||^2 with the residual
 * R = x - z W^T kept current (:110-129); an atom of zero norm is skipped, its coordinate keeps its start value (:111).
 * After a sweep the row is checked (:132) when max|z| == 0, when max|change| / max|z| < tol, or on sweep max_iter; a
 * checked row gets the duality gap (:87-99), and stops once gap < tol * ||x_row||^2.  The whole solve of all rows is
 * ONE launch behind two products (G = W^T W, b0 = x W): a wave keeps a row's z and q = b0 - G z in registers and visits
 * only the coordinates that can change (csrc/cd_mod.hip).  No atomics: two calls give the same bits.
 *   z_inout [n][k] (ldz): with z_has_start != 0 the start, updated IN PLACE like the reference's z0 (:76,139); with
 *     z_has_start == 0 it is only written (zero start).
 *   gap_out [n] (device): the last evaluated gap of each row; tol + 1 for a row never checked (max_iter == 0, :78).
 *   sweeps_out [n] int32 / converged_out [n] bytes (device, nullable): sweeps run and gap < tol * ||x_row||^2.  A row
 *     whose sweep changed nothing and did not converge reports max_iter: the remaining sweeps would repeat it.
 *   n_unconverged_out / committed_out (HOST, nullable): rows not converged, and coordinate updates with a nonzero
 *     change summed over rows and sweeps; when either is given the call synchronises `stream`, else nothing blocks.
 * The layout contract above applies to x, W and z (padding is never written).  Null pointers, negative sizes and too
 * small leading dimensions answer LASSO_ERR_BAD_ARG with nothing enqueued; dtypes other than LASSO_F32 and k > 4096
 * LASSO_ERR_UNSUPPORTED.  Any d.  Rows are independent: a row shard needs no collective.
 */
size_t lasso_cd_mod_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype);
int lasso_cd_mod_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw,
                       void* z_inout_dev, int64_t ldz, int z_has_start,
                       float* gap_out_dev, int32_t* sweeps_out_dev, uint8_t* converged_out_dev,
                       int64_t n, int64_t d, int64_t k, int dtype, double alpha, int max_iter, double tol,
                       int32_t* n_unconverged_out, int64_t* committed_out,
                       void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- convolutional ISTA/FISTA: replaces ista_conv2d(), lasso/conv2d/ista.py:7-49, and
 *      lip_bound_conv2d(), lasso/conv2d/lip_const.py:96-135 ---------------------------------
 * All tensors are contiguous NCHW fp32: x [N][C][H][W], weight [K][C][kh][kw] (the layout
 * F.conv2d takes: K code channels out, C image channels in), code z [N][K][Hz][Wz] with
 * H == (Hz-1)*sh - 2*ph + kh (the size conv_transpose2d gives the code; else
 * LASSO_ERR_BAD_ARG, the reference's shape RuntimeError at ista.py:19).
 *   lasso_conv_ista_solve: min_z 0.5*||conv_transpose2d(z, W) - x||^2 + alpha*||z||_1 by
 *     (F)ISTA with the fixed step lr; z0_dev == NULL means zero init; the stop rule
 *     sum|z - z_next| <= numel(z)*tol is global (ista.py:16,44) and, when tol > 0, is read
 *     once per chunk of speculated iterations (the stopping iteration is replayed bitwise
 *     from the chunk's head: the codes, the count and the last sum are those of a solve
 *     that checked after every iteration); tol == 0 runs exactly maxiter iterations without
 *     a synchronisation.  iters_out / last_delta_out: HOST, nullable.
 *   lasso_conv_objective: (0.5*||x - x_hat||^2 + alpha*||z||_1)/N -> loss_dev (ista.py:23-26).
 *   lasso_conv_lip_bound: the Toeplitz bound on lambda_max of the stride-1 operator on a
 *     sample x sample frequency grid (sqrt != 0: its square root); ksize odd (else
 *     LASSO_ERR_BAD_ARG, the reference's ValueError :101-102).  l_out: HOST (synchronises).
 */
size_t lasso_conv_ista_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K,
                                       int64_t Hz, int64_t Wz, int kh, int kw,
                                       int sh, int sw, int ph, int pw);
/* Name of the device kernel(s) lasso_conv_ista_solve dispatches this geometry to on the current device (the names
 * rocprofv3 --kernel-trace reports): "lasso::conv_fused_kernel<..>" when whole iterations run as one kernel with a
 * workgroup per image -- up to 64 iterations per launch -- or per band of an image (stride 1, fewer than 8 channels,
 * K <= 128, small images; at least a third as many images as CUs, or K <= 64 and bands whose halo is cheap), else the
 * synthesis kernel +
 * the gradient/prox kernel of the two-launch form. */
const char* lasso_conv_ista_kernel_name(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K,
                                        int64_t Hz, int64_t Wz, int kh, int kw, int sh, int sw, int ph, int pw);
int lasso_conv_ista_solve(const void* x_dev, const void* w_dev, const void* z0_dev, void* z_out_dev,
                          int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz,
                          int kh, int kw, int sh, int sw, int ph, int pw, int dtype,
                          double alpha, double lr, int fast, int maxiter, double tol,
                          int32_t* iters_out, float* last_delta_out,
                          void* workspace_dev, size_t workspace_bytes, void* stream);
int lasso_conv_objective(const void* x_dev, const void* w_dev, const void* z_dev,
                         int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz,
                         int kh, int kw, int sh, int sw, int ph, int pw, int dtype,
                         double alpha, float* loss_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream);
size_t lasso_conv_lip_workspace_bytes(int64_t K, int64_t C, int ksize, int sample);
int lasso_conv_lip_bound(const void* w_dev, int64_t K, int64_t C, int ksize, int padding, int sample,
                         int take_sqrt, double* l_out,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- reverse-mode derivative of the unrolled convolutional solve ---------------------
 * The reference's ista_conv2d (lasso/conv2d/ista.py:7-49) is plain torch code: torch.autograd
 * differentiates it with respect to x, weight and z0.  Same geometry arguments as above.
 *   lasso_conv_ista_run_traced: exactly `iterations` iterations (no stop rule) of the solve with
 *       the fixed step lr, bitwise those of lasso_conv_ista_solve; z_out_dev [N][K][Hz][Wz] = z_T
 *       and trace_dev = the iterates z_0 .. z_T in the solver's layout ([T+1][N*Hz*Wz][K], an
 *       opaque buffer of lasso_conv_ista_trace_bytes bytes; only lasso_conv_ista_backward reads
 *       it).  Workspace: lasso_conv_ista_workspace_bytes.
 *   lasso_conv_ista_backward: given the trace of such a run and dL/dz_T (grad_z_dev, NCHW),
 *       writes dL/dx [N][C][H][W], dL/dW [K][C][kh][kw], dL/dz0 [N][K][Hz][Wz] (each nullable,
 *       contiguous; a null grad_w_dev skips the weight-gradient kernel).  Same derivative as
 *       torch.autograd through the reference loop: softshrink passes the gradient where
 *       |u| > alpha*lr, the step and the momentum schedule are constants.  dL/dW is bitwise
 *       reproducible (no float atomics).  No host synchronisation.
 */
size_t lasso_conv_ista_trace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K,
                                   int64_t Hz, int64_t Wz, int kh, int kw, int sh, int sw, int ph, int pw,
                                   int iterations);
int lasso_conv_ista_run_traced(const void* x_dev, const void* w_dev, const void* z0_dev, void* z_out_dev,
                               int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz,
                               int kh, int kw, int sh, int sw, int ph, int pw, int dtype,
                               double alpha, double lr, int fast, int iterations, void* trace_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream);
size_t lasso_conv_ista_backward_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K,
                                                int64_t Hz, int64_t Wz, int kh, int kw, int sh, int sw,
                                                int ph, int pw);
int lasso_conv_ista_backward(const void* x_dev, const void* w_dev, const void* trace_dev, const void* grad_z_dev,
                             int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz,
                             int kh, int kw, int sh, int sw, int ph, int pw, int dtype,
                             double lr, int fast, int iterations,
                             void* grad_x_dev, void* grad_w_dev, void* grad_z0_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- float64 tensors on the convolutional path ---------------------------------------
 * lasso_conv_ista_solve, lasso_conv_objective, lasso_conv_ista_run_traced and lasso_conv_ista_backward accept
 * dtype == LASSO_F64: every tensor (x, weight, codes, trace, gradients) is then contiguous NCHW double, every value,
 * sum, threshold, momentum step and stop-rule comparison an IEEE double (fp64 MFMA, csrc/conv_f64.hip), and the
 * workspace / trace sizes are those of the _f64 byte-count functions below (the functions without the suffix take no
 * dtype and describe fp32).  Their float slots (last_delta_out, the float at loss_dev) receive the double rounded once;
 * the entry points below keep the doubles.  Same reach as the fp32 explicit path: any N >= 0, C, K, kernel size, stride
 * and padding.  A geometry mismatch or a null required pointer is LASSO_ERR_BAD_ARG, a short workspace
 * LASSO_ERR_WORKSPACE; both are decided on the host before any HIP call.  Two calls with the same arguments give the
 * same bits.  lasso_conv_ista_kernel_name describes the fp32 dispatch only.
 *   lasso_conv_lip_bound_f64: the Toeplitz bound with the phases, sin / cos and all sums in double on the frequency
 *     grid 2*pi*i/(sample-1) (an extension: the reference multiplies a double kernel by its float32 phase table and
 *     raises).  l_out: HOST (synchronises). */
size_t lasso_conv_ista_workspace_bytes_f64(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K,
                                           int64_t Hz, int64_t Wz, int kh, int kw,
                                           int sh, int sw, int ph, int pw);
size_t lasso_conv_ista_trace_bytes_f64(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K,
                                       int64_t Hz, int64_t Wz, int kh, int kw, int sh, int sw, int ph, int pw,
                                       int iterations);
size_t lasso_conv_ista_backward_workspace_bytes_f64(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K,
                                                    int64_t Hz, int64_t Wz, int kh, int kw, int sh, int sw,
                                                    int ph, int pw);
size_t lasso_conv_lip_workspace_bytes_f64(int64_t K, int64_t C, int ksize, int sample);
int lasso_conv_ista_solve_f64(const void* x_dev, const void* w_dev, const void* z0_dev, void* z_out_dev,
                              int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz,
                              int kh, int kw, int sh, int sw, int ph, int pw,
                              double alpha, double lr, int fast, int maxiter, double tol,
                              int32_t* iters_out, double* last_delta_out,
                              void* workspace_dev, size_t workspace_bytes, void* stream);
int lasso_conv_objective_f64(const void* x_dev, const void* w_dev, const void* z_dev,
                             int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz,
                             int kh, int kw, int sh, int sw, int ph, int pw,
                             double alpha, double* loss_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream);
int lasso_conv_lip_bound_f64(const void* w_dev, int64_t K, int64_t C, int ksize, int padding, int sample,
                             int take_sqrt, double* l_out,
                             void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- reverse-mode derivative of the unrolled fixed-step solve ------------------------
 * The reference's ista() is ordinary autograd-traceable torch code (ista.py:57-104; the
 * README advertises back-propagation through the solver).  Given the iterates
 * z_0 .. z_T of a fixed-step run (trace_dev: [T+1][n][k] contiguous, T = iterations;
 * produce it with lasso_fista_run, one iteration per call) and dL/dz_T (grad_z_dev
 * [n][k]), writes dL/dx [n][d], dL/dW [d][k], dL/dz0 [n][k] (each nullable, contiguous).
 * Same derivative as torch.autograd through the reference loop: softshrink passes the
 * gradient where |u| > alpha*lr, the step size and the momentum schedule are constants.
 * Any d, k.  No host synchronisation.
 */
size_t lasso_fista_backward_workspace_bytes(int64_t n, int64_t d, int64_t k);
int lasso_fista_backward(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw,
                         const void* trace_dev, const void* grad_z_dev,
                         int64_t n, int64_t d, int64_t k, int dtype, double lr, int fast, int iterations,
                         void* grad_x_dev, void* grad_w_dev, void* grad_z0_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream);
/* The same with one step size per iteration: lr_steps_host[i] (HOST array, `iterations` entries) is the
 * step iteration i was taken with -- the derivative of a line-search solve (ista.py:17-54: the accepted
 * step is a python float, i.e. a constant of the autograd graph; lasso_fista_solve reports the steps in
 * accepted_lr_out[], lasso_fista_run replays them one iteration per call to produce the trace).
 * lr_steps_host == NULL: every iteration used `lr`. */
int lasso_fista_backward_steps(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw,
                               const void* trace_dev, const void* grad_z_dev,
                               int64_t n, int64_t d, int64_t k, int dtype, double lr,
                               const float* lr_steps_host, int fast, int iterations,
                               void* grad_x_dev, void* grad_w_dev, void* grad_z0_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- patch front end: image -> patches -> centre -> dict_learning ->
 * reconstruct.  The reference's notebook that did this (examples/dict_learning_omniglot.ipynb)
 * is absent from its checkout, so there is no reference code to mirror: the layout is that of
 * torch.nn.functional.unfold -- images [N][C][H][W]; patch row m = (n, u, v) with
 * u < (H-ph)/sh+1, v < (W-pw)/sw+1; column (c, a, b).
 *   lasso_patches_extract     : patches [M][C*ph*pw] (ld); center != 0 subtracts each patch's
 *                               mean (stored in means_dev [M] when non-NULL).
 *   lasso_patches_reconstruct : overlap-AVERAGE of (patch + its mean) back into images.
 */
int lasso_patches_extract(const void* img_dev, void* patches_dev, int64_t ld, float* means_dev,
                          int64_t N, int64_t C, int64_t H, int64_t W, int ph, int pw, int sh, int sw,
                          int center, void* stream);
int lasso_patches_reconstruct(const void* patches_dev, int64_t ld, const float* means_dev, void* img_out_dev,
                              int64_t N, int64_t C, int64_t H, int64_t W, int ph, int pw, int sh, int sw,
                              void* stream);

/* ---- GPSR-Basic: replaces gpsr_basic(), lasso/linear/solvers/gpsr.py:209-365 (sparse_encode.py:56-59) --------
 * Gradient projection on the split z = u - v, u, v >= 0 (Figueiredo, Nowak, Wright 2007) over the whole batch: every
 * inner product is a sum over all n rows, so the step size, the line search and the stop criterion are one decision per
 * iteration (csrc/gpsr.hip).  The dictionary W [d][k] takes the place of the reference's A / AT callables.
 *   options : the reference's arguments; stop_criterion 0..4 (else LASSO_ERR_BAD_ARG), init 0 (zeros) or 2 (x W) when
 *             z0_dev is NULL (init 1, a random start, is the caller's to draw and pass as z0_dev: LASSO_ERR_UNSUPPORTED);
 *             first_tau_factor <= 0 means "not given".
 *   result  : n_iter (debias steps included, like the reference's counter), the final objective, flags (below),
 *             the figures of the reference's verbose summaries, and -- trace non-NULL -- per-iteration host arrays of
 *             the caller (capacity entries are written at most; every array of a non-NULL trace must be non-NULL).
 * Continuation and debias run inside the call.  One extension: a line search whose objective is not finite, or that
 * has reduced lambda 100 times, ends the solve (LASSO_GPSR_LINESEARCH_FAILED) with the last accepted z -- the
 * reference would loop for ever.  z0_dev is only read; z_out_dev may not alias x or W.
 * The call blocks: the host reads the control block once per outer iteration.  LASSO_F32 only (else
 * LASSO_ERR_UNSUPPORTED); any n >= 0, d, k >= 1; n = 0 writes nothing.
 * options->reserved: LASSO_FORCE_BLOCKS_128 is the one defined bit; any other is LASSO_ERR_BAD_ARG with nothing written. */
/* A bit of options.reserved that the solvers on the shared fp32 GEMM shell take (lasso_gpsr_solve, lasso_conv_gpsr_solve,
 * the dense lasso_cg_solve, lasso_iter_ridge_solve, lasso_interior_point_solve, lasso_irbfgs_solve): every product of the
 * solve runs on 128 x 128 blocks, also below the size at which the solver would choose them (tests; the codes are those
 * of a solve that chose them itself).  A row pitch of 2^22 elements or more keeps 64 x 64 blocks.
 * lasso_solver_block_side(m, nn, ldmax) is the side -- 64 or 128 -- an unforced solve on the current device gives a
 * product [m, nn] whose widest row pitch (operands, output, contraction) is ldmax elements; 0 for a bad shape. */
#define LASSO_FORCE_BLOCKS_128 8
int lasso_solver_block_side(int64_t m, int64_t nn, int64_t ldmax);
typedef struct lasso_gpsr_options {
  int32_t stop_criterion, maxiter, miniter, init;
  int32_t continuation, debias, cont_steps, maxiter_debias, miniter_debias, reserved;
  double tol, mu, lambda_backtrack, first_tau_factor, tol_debias;
} lasso_gpsr_options;
typedef struct lasso_gpsr_trace {
  int32_t capacity;                       /* iterations of the main phase the arrays below hold */
  float* lambda; float* lambda0;          /* accepted step, first guess */
  int32_t* trials; float* objective; float* criterion; int32_t* nz;
  int32_t step_capacity;                  /* continuation steps */
  double* step_tau; float* step_f0; int32_t* step_nz0; int32_t* step_end;   /* tau, start objective / nonzeros, n_iter at its end */
  int32_t db_capacity;                    /* debias steps */
  float* db_rr; float* db_conv;           /* |resid|^2, rTr / threshold */
} lasso_gpsr_trace;
#define LASSO_GPSR_ZERO_SOLUTION 1        /* tau >= max|x W|: z_out = 0 ("tau is too small; solution is zero vector") */
#define LASSO_GPSR_TAU_FACTOR_CHANGED 2   /* "parameter FirstTauFactor too large; changing" */
#define LASSO_GPSR_LINESEARCH_FAILED 4
#define LASSO_GPSR_DEBIAS_NO_NONZEROS 8   /* "Debiasing requested but not performed. x has no nonzeros." */
#define LASSO_GPSR_DEBIAS_TOO_MANY 16     /* "... There are too many nonzeros in x." */
typedef struct lasso_gpsr_result {
  int32_t n_iter, flags, steps, db_iters;
  double objective;                       /* the final objective (after debias when it ran) */
  double main_objective; float main_rr, main_l1; int32_t main_nz;   /* main phase: objective, |z W^T - x|^2, |z|_1, nonzeros */
  float db_rr, db_l1; int32_t db_nz;      /* after debias */
  lasso_gpsr_trace* trace;                /* nullable */
} lasso_gpsr_result;
size_t lasso_gpsr_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype);
int lasso_gpsr_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev, int64_t ldz0,
                     void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                     const lasso_gpsr_options* options, lasso_gpsr_result* result,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- convolutional GPSR-Basic: gpsr_basic(y, A, tau, AT, ...) of gpsr.py:209-365 with the closures
 *        A  = lambda v: conv_transpose2d(v, W, stride, padding)      AT = lambda v: conv2d(v, W, stride, padding)
 * min_z 0.5 |x - conv_transpose2d(z, W)|^2 + tau |z|_1 over the whole batch (csrc/conv_gpsr.hip): the loop, the decision
 * kernels, options, result, trace and flag bits of lasso_gpsr_solve, on the convolutional operator.  Tensors are
 * contiguous NCHW like the other lasso_conv_* entry points: x [N][C][H][W], W [K][C][kh][kw], z0 (nullable; only read)
 * and z_out [N][K][Hz][Wz]; z_out may not alias an input.  The debias test "too many nonzeros" compares against the
 * elements of x.  options->init: 0 (zeros) or 2 (conv2d(x, W)) when z0_dev is NULL; init 1 is the caller's to draw and
 * pass as z0_dev (LASSO_ERR_UNSUPPORTED).
 * Status: a geometry with (Hz-1) sh - 2 ph + kh != H (or the same for the width), a null pointer or a stop_criterion
 * outside 0..4 is LASSO_ERR_BAD_ARG with nothing enqueued; a dtype other than LASSO_F32 is LASSO_ERR_UNSUPPORTED;
 * N = 0 writes nothing.  The call blocks like lasso_gpsr_solve.  A problem whose code pixels N Hz Wz, K or
 * C kh kw exceed 2^23 (32-bit offsets of a 64-row GEMM block) is LASSO_ERR_UNSUPPORTED.  _workspace_bytes returns 0 for
 * every geometry the solve refuses.
 * Two kernel families (csrc/conv_gpsr.hip): "implicit" where the implicit-GEMM kernels of lasso_conv_ista_solve cover
 * the geometry (the rule of lasso_conv_ista_kernel_name: stride 1, few channels, 3/5/7 kernels, K a multiple of 4),
 * "patches" (patch matrix + GEMM, GEMM + overlap-add) everywhere else.  Bit 0 of options->reserved forces "patches";
 * lasso_conv_gpsr_form says which one a solve of that geometry with that `reserved` takes ("" for a refused geometry).
 * LASSO_FORCE_BLOCKS_128 in options->reserved gives the GEMMs of "patches" 128 x 128 blocks (tests; the form is
 * unaffected); every other bit is LASSO_ERR_BAD_ARG. */
size_t lasso_conv_gpsr_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz,
                                       int kh, int kw, int sh, int sw, int ph, int pw);
const char* lasso_conv_gpsr_form(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz, int kh,
                                 int kw, int sh, int sw, int ph, int pw, int reserved);
int lasso_conv_gpsr_solve(const void* x_dev, const void* w_dev, const void* z0_dev, void* z_out_dev, int64_t N,
                          int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz, int kh, int kw, int sh,
                          int sw, int ph, int pw, int dtype, double tau, const lasso_gpsr_options* options,
                          lasso_gpsr_result* result, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- orthant-wise Newton: replaces orthant_wise_newton(), lasso/linear/solvers/orthant_wise_newton.py:33-160 ----
 * min_z 0.5 |z W^T - x|^2 + alpha |z|_1 over the whole batch (csrc/own.hip).  Once per solve Hinv = (W^T W + 1e-4 I)^-1
 * (lasso_gram_accumulate_f64 + lasso_ridge_solve_f64 on W in double, rounded once to fp32); per iteration v = -pseudo
 * gradient, d = project(v Hinv^T, v), a batch-wide line search for t, z+ = project(z + t d, eta), stop once
 * |z+ - z|_2 <= xtol.  Every sum is folded in double in a fixed order: two solves of the same arguments give the same
 * bits.
 *   options : maxiter >= 0; line_search 0 'brent' (bounded Brent on (0, 10), csrc/brent_host.hpp; lr unused),
 *             1 'backtrack' (t = lr, lr ls_decay, ...: the first with f+ <= f - ls_tol <v, z+ - z> in the reference's
 *             fp32 order, at most ls_maxiter trials, then the next rung unexamined), 2 'none' (t = lr); bit 0 of
 *             reserved forces 128 x 128 GEMM blocks (tests).  The Brent objective is the double the fold produced, not
 *             rounded to fp32.
 *   result  : n_iter, flags, the objective of z0 and of z_out, cholesky_info (0, or 1 + the index of the first
 *             non-positive pivot of W^T W + 1e-4 I: then LASSO_ERR_BAD_ARG), and -- trace non-NULL -- host arrays of the
 *             caller: per iteration (capacity) the step t, the line-search evaluations, the objective and |dz|_2 of the
 *             new z; per line-search evaluation (eval_capacity; eval_count is written) the iteration (1-based), t and f.
 * Refusals before any HIP call: null pointers, n < 0, d or k < 1, a leading dimension below the row length, alpha < 0,
 * maxiter < 0, ls_maxiter < 1 or an unknown line_search are LASSO_ERR_BAD_ARG; a dtype other than LASSO_F32 and
 * k > 4096 LASSO_ERR_UNSUPPORTED (the workspace query returns 0); a short workspace LASSO_ERR_WORKSPACE.  n = 0 writes
 * nothing.  z0_dev is only read; z_out_dev may not alias x or W.  The call blocks: the host reads the control block once
 * per Brent evaluation / per batch of 8 backtracking rungs. */
typedef struct lasso_own_options {
  int32_t maxiter, line_search, ls_maxiter, reserved;
  double lr, xtol, ls_tol, ls_decay;
} lasso_own_options;
typedef struct lasso_own_trace {
  int32_t capacity;                       /* iterations the arrays below hold */
  int32_t eval_capacity;                  /* line-search evaluations eval_* hold */
  double* t; int32_t* ls_iters; double* f; double* delta_z;
  int32_t* eval_iter; double* eval_t; double* eval_f;
  int64_t eval_count;                     /* out: evaluations the solve made (may exceed eval_capacity) */
} lasso_own_trace;
#define LASSO_OWN_LS_NOT_CONVERGED 1      /* a backtracking ran out of trials ('line search did not converge.') */
#define LASSO_OWN_NONFINITE 2             /* a non-finite objective ended the solve with the last accepted z */
typedef struct lasso_own_result {
  int32_t n_iter, flags;
  double f0, f_final;
  int32_t cholesky_info;
  int32_t ls_failures;                    /* iterations whose backtracking ran out */
  lasso_own_trace* trace;                 /* nullable */
} lasso_own_result;
size_t lasso_own_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype);
int lasso_own_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev, int64_t ldz0,
                    void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                    const lasso_own_options* options, lasso_own_result* result,
                    void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- OWL-QN: replaces owlqn(), lasso/nonlinear/owlqn.py:80-199, for fun(z) = 0.5 |z W^T - x|^2 ----
 * min_z 0.5 |z W^T - x|^2 + alpha |z|_1 over the whole batch by orthant-wise L-BFGS (csrc/owlqn.hip): no k x k matrix
 * and no cap on k.  Per iteration v = -pseudo gradient, d = project(H v, v) with H the L-BFGS operator of the held pairs
 * (s, y) = (z - z_prev, g - g_prev), a batch-wide line search for t, z+ = project(z + t d, eta), stop once
 * |z+ - z|_2 <= xtol; then the pair of the step is held if y.s > 1e-10 (the oldest leaves once history_size are held)
 * and H's scaling becomes y.s / y.y.  H v is taken in the vector-free form of the two-loop recursion: one pass over the
 * held vectors for the dots of {v, s_new, y_new} against them (fixed segments of n k, partials in double), ONE workgroup
 * that keeps S^T Y and Y^T Y in double and runs both loops on the small vectors, one pass for
 * d = project(gamma v + S c + Y e, v), accumulated in double and rounded once.  Every sum is folded in double in a fixed
 * order: two solves of the same arguments give the same bits.
 *   pairs   : the workspace holds min(history_size, maxiter - 1) pairs (never negative) and one spare slot; pass that
 *             number to lasso_owlqn_workspace_bytes (a larger one is accepted).  The query grows with `pairs`.
 *   options : maxiter >= 0, history_size >= 1; line_search 0 'brent' (bounded Brent on (0, 10)), 1 'backtrack' (from
 *             the current t: ls_decay per trial, the first with f+ <= f - ls_tol <v, z+ - z> in the reference's fp32
 *             order, at most ls_maxiter trials, then the next rung unexamined), 2 'none'.  The first iteration's t is
 *             min(lr / |pg|_1, lr) as a float32 (and decays as one), later ones start from lr; Brent ignores it.  Bit 0
 *             of reserved forces 128 x 128 GEMM blocks (tests); bit 1 times the three launches of the direction with
 *             events, summed over the iterations into result->direction_ms, and counts the bytes they read and write
 *             into result->direction_bytes (tools/bench_owlqn.py) -- both are 0 without it.
 *   result  : n_iter, flags (LASSO_OWN_LS_NOT_CONVERGED, LASSO_OWN_NONFINITE), the objective of z0 and of z_out, and --
 *             trace non-NULL -- host arrays of the caller: per iteration (capacity) the step t, the line-search
 *             evaluations, the objective and |dz|_2 of the new z, the pairs held after the iteration's update, whether
 *             that update was dropped, and H's scaling; per line-search evaluation (eval_capacity; eval_count is
 *             written) the iteration (1-based), t and f.
 * Refusals before any HIP call: null pointers, n < 0, d or k < 1, a leading dimension below the row length, alpha < 0,
 * maxiter < 0, history_size < 1, ls_maxiter < 1 or an unknown line_search are LASSO_ERR_BAD_ARG; a dtype other than
 * LASSO_F32 is LASSO_ERR_UNSUPPORTED (the workspace query returns 0); a short workspace LASSO_ERR_WORKSPACE.  n = 0
 * writes nothing.  z0_dev is only read; z_out_dev may not alias x or W.  The call blocks: the host reads one control
 * record per Brent evaluation, one per batch of 8 backtracking rungs and one per iteration. */
typedef struct lasso_owlqn_options {
  int32_t maxiter, line_search, ls_maxiter, history_size;
  double lr, xtol, ls_tol, ls_decay;
  int64_t reserved;
} lasso_owlqn_options;
typedef struct lasso_owlqn_trace {
  int32_t capacity;                       /* iterations the arrays below hold */
  int32_t eval_capacity;                  /* line-search evaluations eval_* hold */
  double* t; int32_t* ls_iters; double* f; double* delta_x;
  int32_t* pairs; int32_t* skipped; double* h_diag;
  int32_t* eval_iter; double* eval_t; double* eval_f;
  int64_t eval_count;                     /* out: evaluations the solve made (may exceed eval_capacity) */
} lasso_owlqn_trace;
typedef struct lasso_owlqn_result {
  int32_t n_iter, flags;
  double f0, f_final;
  int32_t ls_failures;                    /* iterations whose backtracking ran out */
  int32_t reserved;
  lasso_owlqn_trace* trace;               /* nullable */
  double direction_ms, direction_bytes;   /* bit 1 of options.reserved: device time of, and bytes moved by, the direction */
} lasso_owlqn_result;
size_t lasso_owlqn_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype, int64_t pairs);
int lasso_owlqn_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev, int64_t ldz0,
                      void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                      const lasso_owlqn_options* options, lasso_owlqn_result* result,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- OWL-QN on a generalised-linear objective: owlqn() with fun(z) = sum loss(u, x), u = z W^T ----
 * lasso_owlqn_solve with the objective's family as one more argument; everything else -- the arguments, the options,
 * result and trace structs, the refusals, the direction, the ring, the line searches, the one control record per
 * decision -- is lasso_owlqn_solve's.  The workspace comes from lasso_owlqn_workspace_bytes: the layout is identical
 * (the buffer that holds the residual holds r = d loss / d u).
 *   LASSO_GLM_BERNOULLI  loss = softplus(u) - x u, torch's binary_cross_entropy_with_logits(u, x, reduction='sum'); x is
 *                        any real target (0/1 or soft), not validated.  Evaluated without exp(+|u|):
 *                          e = expf(-|u|), loss = max(u, 0) - x u + log1pf(e), r = (u >= 0 ? 1 : e) / (1 + e) - x,
 *                        finite for every finite u.  The objective is the double fold of the per-element float32 losses
 *                        plus alpha |z|_1; the backtracking test sees it rounded to float32, as the reference computes it.
 * Any other family is LASSO_ERR_UNSUPPORTED (before any HIP call). */
#define LASSO_GLM_BERNOULLI 1             /* family: logistic loss of logits u against targets x */
int lasso_owlqn_glm_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev, int64_t ldz0,
                          void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                          int family, const lasso_owlqn_options* options, lasso_owlqn_result* result,
                          void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- ISTA / FISTA through a one-layer decoder: replaces ista_nl(), lasso/nonlinear/ista.py:55-128, for
 * decoder(z) = act(z W^T + b) ----
 * min_z 0.5 |act(z W^T + b) - x|^2 + alpha |z|_1 by (fast) iterative shrinkage (csrc/ista_nl.hip).  What the reference
 * takes from autograd has a closed form for this family; with u = y W^T + b and a = act(u), per iteration
 *   product 1  y W^T; its epilogue stores r = (a - x) act'(u) -- and, lr_auto, c = act'(u)^2 + (a - x) act''(u)
 *   product 2  r W = the gradient; its epilogue does z_next = softshrink(y - t g, alpha t), the momentum point
 *              y_next = z_next + ((t_k - 1) / t_{k+1}) (z_next - z) when `fast`, and the block partials of sum |z - z_next|
 * and u, a and the gradient never exist in memory.  Sigmoid and tanh are evaluated from exp(-|u|) / exp(-2 |u|) alone (no
 * logit overflows); ReLU's derivative is (u > 0), torch's subgradient.
 *   bias_dev   : [d], nullable.  W is [d][k] (ldw), torch.nn.Linear's own layout.
 *   activation : LASSO_ACT_IDENTITY / _SIGMOID / _TANH / _RELU; anything else is LASSO_ERR_UNSUPPORTED before any HIP call.
 *   options    : maxiter >= 0; fast; lr (the fixed step) or lr_auto != 0: every iteration takes the per-row step
 *                t_i = 0.98 / L_i, L_i from the reference's power iteration (hessian_2norm, ista.py:26-52) on the row's
 *                Hessian H_i = W^T diag(c_i) W at the step's point: u <- u0, power_iters times v = normalise(H u),
 *                u = normalise(H v), then L = v . H u -- 2 power_iters + 1 applications of H, each the same two products
 *                (the first multiplies by c, the second emits the rows' sums of squares, last the rows' dots; the
 *                normalisation v / max(|v|, 1e-8) is a per-row scale in the next epilogue, not a pass).  u0_dev [n][k]
 *                (ldu0) is the start vector, the same at every step (the reference draws a new one at every step);
 *                required with lr_auto (else LASSO_ERR_BAD_ARG), ignored without.  t_i is torch's `0.98 / L`: the
 *                reciprocal times 0.98f; a row with H_i = 0 gets inf / NaN, nothing is checked or repaired.  tol: the
 *                reference's batch-wide rule, sum |z - z_next| <= n k tol in float32, ends the solve with that iteration's
 *                z_next; tol <= 0 (or NaN) runs maxiter iterations.  Bit 0 of reserved forces 128 x 128 GEMM blocks, as in
 *                lasso_owlqn_solve (tests); any other bit is LASSO_ERR_BAD_ARG.
 *   result     : n_iter, stopped (the rule fired), last_delta (the last sum the host read; NaN without one), f0 / f_final
 *                (the objective of z0 and of z_out; NaN unless trace->loss > 0).  l_dev (IN, nullable, device [n]): with
 *                lr_auto and n_iter > 0 it receives the L_i of the last step.
 *   trace      : nullable; host arrays of the caller, `capacity` iterations: deltas (nullable) the sums |z - z_next|;
 *                loss 0: no objective is computed; 1: f0 and f_final (one more decoder product each); 2: also f[i] =
 *                the objective of the i-th z_next (one more decoder product per iteration).
 * The host reads one record per chunk of speculated iterations (csrc/stoprule_host.hpp; a stop inside a chunk is
 * replayed from the chunk's head, bitwise the state the reference stops in), one per 64 iterations when tol <= 0 with a
 * trace, none when tol <= 0 without.  The call blocks.  Every sum is folded in double in a fixed order: two solves of
 * the same arguments give the same bits.  Refusals before any HIP call: null pointers, n < 0, d or k < 1, a leading
 * dimension below the row length, maxiter < 0, power_iters < 1 with lr_auto are LASSO_ERR_BAD_ARG; a dtype other than
 * LASSO_F32 is LASSO_ERR_UNSUPPORTED (the workspace query returns 0); a short workspace LASSO_ERR_WORKSPACE.  n = 0 writes
 * nothing.  The inputs are only read; z_out_dev may not alias one. */
#define LASSO_ACT_IDENTITY 0
#define LASSO_ACT_SIGMOID 1
#define LASSO_ACT_TANH 2
#define LASSO_ACT_RELU 3
typedef struct lasso_ista_nl_options {
  int32_t maxiter, fast, lr_auto, power_iters;
  double lr, tol;
  int64_t reserved;
} lasso_ista_nl_options;
typedef struct lasso_ista_nl_trace {
  int32_t capacity;                       /* iterations the arrays below hold */
  int32_t loss;                           /* 0, 1 or 2: see above */
  double* deltas;                         /* nullable */
  double* f;                              /* required with loss == 2 */
} lasso_ista_nl_trace;
typedef struct lasso_ista_nl_result {
  int32_t n_iter, stopped;
  double last_delta, f0, f_final;
  void* l_dev;                            /* in: device [n] floats or NULL */
} lasso_ista_nl_result;
size_t lasso_ista_nl_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype, int auto_lr);
int lasso_ista_nl_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* bias_dev,
                        const void* z0_dev, int64_t ldz0, void* z_out_dev, int64_t ldz, const void* u0_dev, int64_t ldu0,
                        int64_t n, int64_t d, int64_t k, int dtype, double alpha, int activation,
                        const lasso_ista_nl_options* options, lasso_ista_nl_result* result, lasso_ista_nl_trace* trace,
                        void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- BFGS iterated ridge: replaces iterative_ridge_bfgs(), lasso/nonlinear/iterative_ridge_bfgs.py:45-140, for
 * f(z) = 0.5 |z W^T - x|^2 ----
 * min_z 0.5 |z W^T - x|^2 + alpha |z|_1 over the whole batch (csrc/irbfgs.hip).  Every row i keeps its own BFGS Hessian
 * estimate B_i [k][k] (the identity at the start).  Per iteration, with g = (z W^T - x) W and mask = |z| < eps:
 *   diag = alpha / |z|, rhs = g + diag z (both 0 where masked); the system is B_i with the masked rows and columns
 *   zeroed and diag + tikhonov added to its diagonal; d = the batch's solutions by lasso_batch_chol_solve's kernels --
 *   if ANY row's factorisation fails, the upper triangles are filled and the WHOLE batch is solved by the LU kernels
 *   (the reference's 'Cholesky factorization failed. Reverting to LU decomposition...'); a singular system there is
 *   LASSO_ERR_BAD_ARG with result.bad_row -- judged by the lowest row with a zero pivot: if its solution is finite
 *   the system was singular; if not, a NaN operand reached it and the row stays NaN, as from the reference (that row
 *   is read back, one more host read on this route);
 *   t: line_search 1 = the bounded-Brent minimiser on (0, 10) of f(z - t d) + alpha |z - t d|_1 (one t for the batch;
 *   an evaluation is one pass over [n,k], no product), 0 = min(lr / |g(z0)|_1, lr) as a float32 in iteration 1, lr later;
 *   z+ = where(mask, z, z - t d); stop once |z+ - z|_2 <= xtol (absolute, compared as float32) or the objective is not
 *   finite; otherwise every row's update with s = z+ - z, y = g+ - g:  valid = |y.s| > 1e-10, rho = 1 / y.s (1000 where
 *   invalid), on the first update B *= rho (y.y) for every row, then where valid
 *   B <- (B + rho y y^T) - (B s)(B s)^T / (s^T B s).  No update follows the iteration that stops or the last one.
 * The update and the next iteration's system come from ONE launch per iteration (lasso_irbfgs_update is that launch
 * on its own): B is read twice, written once, and half a matrix is written for the system.  y.s, y.y, B s and s^T B s
 * are summed in double and rounded once; element (i, j) of the update is a symmetric function of (i, j), so B is
 * bitwise symmetric (the reference's baddbmm(B, rho y, y^T) is not).  Every sum is folded in a fixed order: the same
 * arguments give the same bits.
 *   workspace: lasso_irbfgs_workspace_bytes = TWO [n][k][k] float regions (B, which the reference holds too, and the
 *             emitted systems), six [n][k] and two [n][d] ones, W^T, the partial sums and
 *             lasso_batch_solve_workspace_bytes(n, k).  It grows with n k^2: the caller splits a large batch.
 *   options : maxiter >= 0, line_search 0 / 1, lr, xtol, tikhonov, eps >= 0.  Bit 1 of reserved times the update launches
 *             with events (result.row_ms), counts the bytes of their k x k traffic (result.row_bytes) and times the
 *             solves of the systems (result.solve_ms) -- all 0 without it (tools/bench_irbfgs.py); LASSO_FORCE_BLOCKS_128
 *             forces 128 x 128 GEMM blocks (tests); every other bit must be 0.
 *   result  : n_iter, flags (LASSO_IRBFGS_*), the objective of z0 and of z_out, lu_count = iterations that took the
 *             LU route, and -- trace non-NULL -- host arrays of the caller: per iteration (capacity) t, the Brent
 *             evaluations, the objective and |dz|_2 of the new z, the rows whose update was invalid (-1: no update
 *             followed), whether the LU route ran; per Brent evaluation (eval_capacity; eval_count is written) the
 *             iteration (1-based), t and f.
 * Refusals before any HIP call: null pointers, n < 0, d or k < 1, a leading dimension below the row length, alpha < 0,
 * a negative maxiter, lr, xtol, tikhonov or eps, an unknown line_search or reserved bit are LASSO_ERR_BAD_ARG; a dtype
 * other than LASSO_F32 and k > lasso_batch_solve_tier_cap(LASSO_F32, LASSO_BATCH_TIER_GENERAL) = 1024 are
 * LASSO_ERR_UNSUPPORTED (the workspace query returns 0); a short workspace LASSO_ERR_WORKSPACE.  n = 0 writes nothing.
 * z0_dev is only read; z_out_dev may not alias x or W.  The call enqueues on `stream` only and blocks: the host reads
 * one record per solve of the systems (two on the LU route), one per Brent evaluation and one per iteration.
 *
 * lasso_irbfgs_update: the row kernel alone, on packed operands: b_dev [n][k][k], x_dev / g_dev [n][k] (the new iterate
 * and its gradient, read), x_prev_dev / g_prev_dev [n][k] (read, then overwritten with x and g), system_dev [n][k][k]
 * (out: the lower triangles and diagonals of the masked, loaded systems of x; the strict upper triangles are not
 * defined), rhs_dev [n][k] and valid_dev [n] int32 (out).  mode 0: B = I is written, no update; 1: the update (with
 * `first` != 0 the first update's scaling); 2: B is used as it is.  max_workgroups > 0 bounds the launch's grid (rows are
 * strided over it), 0 = the default.  Needs no workspace; blocks until the launch has finished.  Refusals as above
 * (mode outside 0..2 is LASSO_ERR_BAD_ARG). */
#define LASSO_IRBFGS_CONVERGED 1
#define LASSO_IRBFGS_NONFINITE 2
typedef struct lasso_irbfgs_options {
  int32_t maxiter, line_search;
  double lr, xtol, tikhonov, eps;
  int64_t reserved;
} lasso_irbfgs_options;
typedef struct lasso_irbfgs_trace {
  int32_t capacity;                       /* iterations the arrays below hold */
  int32_t eval_capacity;                  /* Brent evaluations eval_* hold */
  double* t; int32_t* ls_iters; double* f; double* delta_x;
  int32_t* invalid_rows; int32_t* lu;
  int32_t* eval_iter; double* eval_t; double* eval_f;
  int64_t eval_count;                     /* out: evaluations the solve made (may exceed eval_capacity) */
} lasso_irbfgs_trace;
typedef struct lasso_irbfgs_result {
  int32_t n_iter, flags;
  double f0, f_final;
  int32_t lu_count, reserved;
  int64_t bad_row;                        /* -1, or the lowest row whose system was singular on the LU route */
  lasso_irbfgs_trace* trace;              /* nullable */
  double row_ms, row_bytes;               /* bit 1 of options.reserved: device time and k x k bytes of the update launches */
  double solve_ms;                        /* ... and the time in the solves of the systems, their host reads included */
} lasso_irbfgs_result;
size_t lasso_irbfgs_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype);
int lasso_irbfgs_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev, int64_t ldz0,
                       void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype, double alpha,
                       const lasso_irbfgs_options* options, lasso_irbfgs_result* result,
                       void* workspace_dev, size_t workspace_bytes, void* stream);
int lasso_irbfgs_update(void* b_dev, const void* x_dev, const void* g_dev, void* x_prev_dev, void* g_prev_dev,
                        void* system_dev, void* rhs_dev, int32_t* valid_dev, int64_t n, int64_t k, int dtype, double alpha,
                        double tikhonov, double eps, int mode, int first, int max_workgroups, void* stream);

/* ---- iterated ridge: replaces iterative_ridge(), lasso/linear/solvers/iterative_ridge.py:11-141 (cg=False) ----
 * min_z 0.5 |z W^T - x|^2 + alpha |z|_1 over the whole batch by iterated ridge regression (csrc/iter_ridge.hip).  Once
 * per solve G = W^T W and rhs = x W; per iteration every row solves
 *   (G[S,S] + diag(alpha / |z_S| + tikhonov)) z_S = rhs_S on its own support S = {j : |z_j| >= eps}
 * with a blocked Cholesky in LDS (supports up to 256) or in a fixed scratch of the workspace (up to 1024); entries off
 * the support keep their value.  line_search != 0: p = z_sol - z, t from a bounded Brent search on (0, 10)
 * (csrc/brent_host.hpp) of f(z + t p), evaluated from three sums of the residual and p W^T plus one pass over [n,k] per
 * trial and handed to the search as an un-rounded double; z += t p on the support.  The solve stops once
 * sum |update| <= n k tol (converged), on a NaN objective or update, or after maxiter iterations.  Every sum is folded
 * in double in a fixed order: two solves of the same arguments give the same bits.
 *   options : maxiter >= 0, line_search 0 / 1, tol >= 0 (per element), tikhonov >= 0, eps >= 0; reserved = 0 or
 *             LASSO_FORCE_BLOCKS_128 (128 x 128 GEMM blocks, tests).
 *   result  : n_iter, status, the objective of z0 and the last fval, bad_row / bad_minor (-1 / 0, or the lowest row whose
 *             system had a non-positive or NaN pivot and 1 + that pivot's index in the compacted system: then
 *             LASSO_ERR_BAD_ARG and z_out is not written), and -- trace non-NULL -- host arrays of the caller: per iteration
 *             (capacity) fval, sum |update|, t, the Brent evaluations, the largest and the mean support of the new z; per
 *             Brent evaluation (eval_capacity; eval_count is written) the iteration (1-based), t and f.
 * lasso_iter_ridge_rows is one masked per-row solve on its own: z_sol [n][k] from G [k][k], rhs [n][k] and z [n][k]
 * (masked entries of z_sol are 0); its workspace is lasso_iter_ridge_workspace_bytes(n, 1, k, dtype); support_max_out is
 * nullable.  z_sol may not alias z.
 * Refusals before any HIP call: null pointers, n < 0, d or k < 1, a leading dimension below the row length, alpha < 0,
 * negative options or an undefined bit of reserved are LASSO_ERR_BAD_ARG; a dtype other than LASSO_F32 and k > 1024
 * LASSO_ERR_UNSUPPORTED (the workspace query returns 0); a short workspace LASSO_ERR_WORKSPACE.  n = 0 writes nothing.
 * The workspace grows linearly in n: the general tier's scratch is at most 256 triangles and 256 MiB.  The calls block. */
typedef struct lasso_iter_ridge_options {
  int32_t maxiter, line_search;
  double tol, tikhonov, eps;
  int64_t reserved;                       /* 0 or LASSO_FORCE_BLOCKS_128 */
} lasso_iter_ridge_options;
typedef struct lasso_iter_ridge_trace {
  int32_t capacity;                       /* iterations the arrays below hold */
  int32_t eval_capacity;                  /* Brent evaluations eval_* hold */
  double* f; double* update; double* t; int32_t* ls_evals; int32_t* support_max; double* support_mean;
  int32_t* eval_iter; double* eval_t; double* eval_f;
  int64_t eval_count;                     /* out: evaluations the solve made (may exceed eval_capacity) */
} lasso_iter_ridge_trace;
#define LASSO_ITER_RIDGE_CONVERGED 0      /* sum |update| <= n k tol */
#define LASSO_ITER_RIDGE_NAN 1            /* NaN objective or update */
#define LASSO_ITER_RIDGE_MAXITER 2
typedef struct lasso_iter_ridge_result {
  int32_t n_iter, status;
  double f0, f_final;
  int64_t bad_row;
  int32_t bad_minor, pad_;
  lasso_iter_ridge_trace* trace;          /* nullable */
} lasso_iter_ridge_result;
size_t lasso_iter_ridge_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype);
int lasso_iter_ridge_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev,
                           int64_t ldz0, void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype,
                           double alpha, const lasso_iter_ridge_options* options, lasso_iter_ridge_result* result,
                           void* workspace_dev, size_t workspace_bytes, void* stream);
int lasso_iter_ridge_rows(const void* g_dev, int64_t ldg, const void* rhs_dev, int64_t ldr, const void* z_dev,
                          int64_t ldz, void* z_sol_dev, int64_t ldzs, int64_t n, int64_t k, int dtype, double alpha,
                          double tikhonov, double eps, int64_t* bad_row_out, int32_t* bad_minor_out,
                          int32_t* support_max_out, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Split Bregman: replaces split_bregman(), lasso/linear/solvers/split_bregman.py:5-86 ----
 * The reference's A is w_dev [d][k], its y is x_dev [n][d], its x0 is x0_dev [n][k] (nullable: zeros) and its x is
 * z_out_dev [n][k] (csrc/split_bregman.hip).  Once per solve Hinv = (W^T W / alpha + lambd I)^-1
 * (lasso_gram_accumulate_f64 + lasso_ridge_solve_f64 on W in double, rounded once to fp32) and Aty = (x W) / alpha; B = D = 0.
 * An outer iteration is niter_inner launches of one product X = (Aty + lambd (D - B)) Hinv^T with
 * D = softshrink(X + B, 1 / lambd) in its epilogue, the last of them also B += tau (X - D) and the partials of
 * update = |X - Xold|_F.  The loop ends at the top of an iteration once update <= tol (compared as floats; update starts
 * at +inf, a NaN never ends it) or after maxiter iterations.  Every sum is folded in double in a fixed order: two solves
 * of the same arguments give the same bits.  z_out is the linear solve's X, not the shrunk D.
 *   options : maxiter >= 1, niter_inner >= 1, lambd > 0, tol (negative: never stop), tau; bit 0 of reserved forces
 *             128 x 128 GEMM blocks (tests), every other bit must be 0.
 *   result  : n_iter (outer iterations executed), itn (the reference's return value: the index of the iteration at whose
 *             top the stop fired, maxiter - 1 if it never did), stopped, cholesky_info (0, or 1 + the index of the first
 *             pivot of W^T W / alpha + lambd I that is not positive: then LASSO_ERR_BAD_ARG and z_out is not written), and
 *             -- trace non-NULL -- host arrays of the caller: per executed iteration (capacity) update and, where cost is
 *             non-NULL, cost = 0.5 |X W^T - x|^2 + alpha |X|_1 (the cost product runs only then).
 * Refusals before any HIP call: null pointers (x0_dev excepted), n < 0, d or k < 1, a leading dimension below the row
 * length, alpha <= 0, lambd <= 0, maxiter < 1, niter_inner < 1, an undefined bit of reserved or a NaN among alpha,
 * lambd, tol, tau are LASSO_ERR_BAD_ARG; a dtype other than LASSO_F32 and k > 4096 LASSO_ERR_UNSUPPORTED (the workspace
 * query returns 0); a short workspace LASSO_ERR_WORKSPACE.  n = 0 writes nothing.  x0_dev is only read; z_out_dev may not
 * alias an input.  The call blocks; the host reads the device once per outer iteration (the update, and with the first
 * one the pivots' verdict), and with tol < 0 only once per 1024 outer iterations and at the end. */
typedef struct lasso_split_bregman_options {
  int32_t maxiter, niter_inner, reserved, pad_;
  double lambd, tol, tau;
} lasso_split_bregman_options;
typedef struct lasso_split_bregman_trace {
  int32_t capacity, pad_;                 /* iterations the arrays below hold */
  double* update;                         /* nullable */
  double* cost;                           /* nullable: NULL skips the cost product */
} lasso_split_bregman_trace;
typedef struct lasso_split_bregman_result {
  int32_t n_iter, itn, stopped, cholesky_info;
  lasso_split_bregman_trace* trace;       /* nullable */
} lasso_split_bregman_result;
size_t lasso_split_bregman_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype);
int lasso_split_bregman_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* x0_dev,
                              int64_t ldx0, void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype,
                              double alpha, const lasso_split_bregman_options* options,
                              lasso_split_bregman_result* result, void* workspace_dev, size_t workspace_bytes,
                              void* stream);

/* ---- interior point: replaces interior_point(), lasso/linear/solvers/interior_point.py:93-225 ----
 * min_z 0.5 |z W^T - x|^2 + alpha |z|_1 over the whole batch by the primal-dual log-barrier method on the split
 * z = z+ - z-, z+, z- >= 0 (csrc/interior_point.hip).  The start is the reference's: z+- = relu(+-z0) + 0.1,
 * lambda = alpha y / omega with y = sign(z0) W^T and omega = 1.1 max_j |y W|_j per row, s+- = alpha -+ lambda W; it must
 * be interior (z > 0, s > 0, -alpha < lambda W < alpha everywhere), otherwise the solve returns LASSO_ERR_BAD_ARG with
 * status LASSO_INTERIOR_POINT_BAD_START and z_out is not written (an all-zero row of z0 gives omega = 0 and a NaN
 * lambda).  Per iteration: the KKT residuals, per row the d x d system (I + W diag(c) W^T) dlambda = rhs with
 * c = z+ / s+ + z- / s- (1 / s is 0 where |s| < eps) by a blocked Cholesky in LDS, the directions, damped steps
 * 0.99 min(1, smallest ratio), mu *= 1 - min(beta_z, beta_s, 0.99), and z, s clamped at 0.  The solve stops once the
 * means over rows of the three ratios prim_feas, dual_feas and gap are all < tol, or after maxiter iterations; a NaN
 * mean never stops it, and with tol <= 0 the host reads nothing between the start's flag and the end.  A pivot that is
 * not positive is not repaired: that row's codes are NaN.  Every sum is folded in double in a fixed order: two solves
 * of the same arguments give the same bits.
 *   options : maxiter >= 0, barrier_init, tol, eps >= 0; reserved = 0 or LASSO_FORCE_BLOCKS_128 (128 x 128 GEMM blocks,
 *             tests).
 *   result  : n_iter, status, obj0 = alpha sum z + 0.5 sum lambda^2 of the start, and -- trace non-NULL -- host arrays
 *             of the caller: per iteration (capacity) that objective and the three means.
 * lasso_interior_point_rows is the per-row Newton system on its own: y [n][d] with (I + W diag(c_i) W^T) y_i = b_i from
 * W [d][k], c [n][k] >= 0 and b [n][d].  y may alias b.  It needs no workspace.
 * Refusals before any HIP call: null pointers, n < 0, d or k < 1, a leading dimension below the row length, alpha < 0
 * or NaN, maxiter < 0, eps < 0, a NaN option or an undefined bit of reserved are LASSO_ERR_BAD_ARG; a dtype other than
 * LASSO_F32, d > 256 and k > 4096 LASSO_ERR_UNSUPPORTED (the workspace query returns 0); a short workspace LASSO_ERR_WORKSPACE.
 * n = 0 writes nothing.  The workspace grows linearly in n: the state z, s [n][2k], lambda [n][d], five [n][k] and four
 * [n][d] temporaries, 64 bytes per row of ratios; there is no n d^2 term.  The calls block. */
typedef struct lasso_interior_point_options {
  int32_t maxiter, pad_;
  double barrier_init, tol, eps;
  int64_t reserved;                       /* 0 or LASSO_FORCE_BLOCKS_128 */
} lasso_interior_point_options;
typedef struct lasso_interior_point_trace {
  int32_t capacity, pad_;                 /* iterations the arrays below hold */
  double* obj; double* prim_feas; double* dual_feas; double* gap;
} lasso_interior_point_trace;
#define LASSO_INTERIOR_POINT_CONVERGED 0  /* the three means < tol */
#define LASSO_INTERIOR_POINT_MAXITER 1
#define LASSO_INTERIOR_POINT_BAD_START 2  /* the start is not interior */
typedef struct lasso_interior_point_result {
  int32_t n_iter, status;
  double obj0;
  lasso_interior_point_trace* trace;      /* nullable */
} lasso_interior_point_result;
size_t lasso_interior_point_workspace_bytes(int64_t n, int64_t d, int64_t k, int dtype);
int lasso_interior_point_solve(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* z0_dev,
                               int64_t ldz0, void* z_out_dev, int64_t ldz, int64_t n, int64_t d, int64_t k, int dtype,
                               double alpha, const lasso_interior_point_options* options,
                               lasso_interior_point_result* result, void* workspace_dev, size_t workspace_bytes,
                               void* stream);
int lasso_interior_point_rows(const void* w_dev, int64_t ldw, const void* c_dev, int64_t ldc, const void* b_dev,
                              int64_t ldb, void* y_dev, int64_t ldy, int64_t n, int64_t d, int64_t k, int dtype,
                              void* stream);

/* ---- conjugate gradients: replace cg(), batch_cg(), batch_cg_conv2d(), lasso/conjgrad.py:13-107 ----
 * x with Adot(x) = b for a whole batch of right-hand sides by the reference's conjgrad() (csrc/conjgrad.hip): x = 0,
 * r = -b, p = b; alpha = rs_old / curv and rs_new / rs_old are one number per row (per image), the exits test sums over
 * the whole batch, in the reference's order inside iteration i:
 *   status 1  sum |r| <= termcond = rtol |b|_1 min(sqrt(|b|_1), 0.5), before the product
 *   status 2  0 <= curv_sum <= 3 eps,  status 3  curv_sum < 0 (at i = 0 with x = -(rs_old / curv) b), before x moves
 *   status 0  sqrt(sum rs_new) < tol, after x and r moved;  status 4  maxiter iterations ran
 * Nothing is checked or repaired: a row whose curv is 0 gets 0 / 0, and with a NaN in the batch no exit fires.  The
 * sums are folded in double in a fixed order and rounded once to the dtype, in which termcond and the comparisons are
 * evaluated: two solves of the same arguments give the same bits.
 * lasso_cg_solve: the dense operator Adot(v) = v A^T with a_dev [k][k] (not assumed symmetric), b_dev [n][k], x_dev
 * [n][k], any pitch; LASSO_F32 (one fp32-MFMA product per iteration whose epilogue takes the per-row curv) or LASSO_F64
 * (all three matrices double, leading dimensions in doubles; the fp64-MFMA product).  tik must be 0.
 * lasso_conv_cg_solve: Adot(v) = conv2d(conv_transpose2d(v, w), w) + tik v (the tik term only where tik > 0) with w_dev
 * [K][C][kh][kw], b_dev and z_out_dev [N][K][Hz][Wz], contiguous; the geometry as lasso_conv_gpsr_solve takes it
 * (H = (Hz - 1) sh - 2 ph + kh, likewise W); LASSO_F32 only.
 *   options : maxiter >= 0, tol >= 0, rtol >= 0, tik >= 0.  Bit 0 of reserved takes the plain forms -- dense: the
 *             product stores Ap and a pass of its own takes curv; convolutional: conv_transpose2d as GEMM + overlap-add
 *             also where an implicit kernel covers the geometry.  Dense only: LASSO_FORCE_BLOCKS_128 forces 128 x 128
 *             GEMM blocks (tests; the float64 product has one block side and ignores it).  Every other bit must be 0.
 *   result  : n_iter (the index i of the iteration an exit fired in; maxiter for status 4), status, host_reads (waits
 *             of the host for the device's control record: one per chunk of iterations; with rtol = 0 and tol = 0 one
 *             at the end), form (LASSO_CG_FORM_*: what ran), termcond, and -- trace non-NULL -- host arrays of the
 *             caller with, per iteration (capacity), sum |r| at its top, curv_sum and sqrt(sum rs_new), as the dtype
 *             holds them.  Iteration i has its r_abs once exit 1 was tested, its curv_sum once the product ran, its rs
 *             once x moved; entries beyond those are unspecified.
 * Refusals before any HIP call: null pointers, n < 0, k < 1, a leading dimension below the row length, a bad geometry,
 * maxiter < 0, a negative or NaN tol, rtol or tik, tik != 0 in the dense form or an undefined bit of reserved are
 * LASSO_ERR_BAD_ARG; any other dtype LASSO_ERR_UNSUPPORTED (the workspace query returns 0); a short workspace
 * LASSO_ERR_WORKSPACE.  n = 0 writes nothing.  The inputs are only read; the output may not alias one.  The calls block. */
typedef struct lasso_cg_options {
  int32_t maxiter, reserved;
  double tol, rtol, tik;
} lasso_cg_options;
typedef struct lasso_cg_trace {
  int32_t capacity, pad_;                 /* iterations the arrays below hold */
  double* r_abs; double* curv_sum; double* rs;      /* each nullable */
} lasso_cg_trace;
#define LASSO_CG_ABS_TOL 0
#define LASSO_CG_REL_TOL 1
#define LASSO_CG_CURV_CONVERGED 2
#define LASSO_CG_CURV_NEGATIVE 3
#define LASSO_CG_MAXITER 4
#define LASSO_CG_FORM_FUSED 0             /* dense fp32: curv in the product's epilogue */
#define LASSO_CG_FORM_UNFUSED 1           /* dense: product, then a pass that takes curv (fp64 always) */
#define LASSO_CG_FORM_CONV_IMPLICIT 2     /* conv_transpose2d by an implicit-GEMM kernel; conv2d as patches + GEMM */
#define LASSO_CG_FORM_CONV_PATCHES 3      /* both convolutions as GEMMs around patch matrices */
typedef struct lasso_cg_result {
  int32_t n_iter, status, host_reads, form;
  double termcond;
  lasso_cg_trace* trace;                  /* nullable */
} lasso_cg_result;
size_t lasso_cg_workspace_bytes(int64_t n, int64_t k, int dtype);
int lasso_cg_solve(const void* a_dev, int64_t lda, const void* b_dev, int64_t ldb, void* x_dev, int64_t ldx, int64_t n,
                   int64_t k, int dtype, const lasso_cg_options* options, lasso_cg_result* result, void* workspace_dev,
                   size_t workspace_bytes, void* stream);
size_t lasso_conv_cg_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t Hz, int64_t Wz, int kh,
                                     int kw, int sh, int sw, int ph, int pw);
int lasso_conv_cg_solve(const void* w_dev, const void* b_dev, void* z_out_dev, int64_t N, int64_t C, int64_t H, int64_t W,
                        int64_t K, int64_t Hz, int64_t Wz, int kh, int kw, int sh, int sw, int ph, int pw, int dtype,
                        const lasso_cg_options* options, lasso_cg_result* result, void* workspace_dev,
                        size_t workspace_bytes, void* stream);

/* ---- exact Lipschitz constant of a convolutional dictionary: replace lip_constant(), lasso/conv2d/lip_const.py:8-31 ----
 * The largest eigenvalue of conv_transpose2d o conv2d (equally of conv2d o conv_transpose2d: the nonzero spectra
 * coincide) for w_dev [K][C][kh][kw], contiguous, by Lanczos with full reorthogonalisation on the device
 * (csrc/conv_lanczos.hip); LASSO_F32 or LASSO_F64, the value is computed in that dtype.
 * (H, W) is the reference's imsize: with transpose == 0 the size of the IMAGE (C x H x W vectors; it must round-trip,
 * (H + 2 ph - kh) % sh == 0 and likewise the width), with transpose != 0 the size of the CODE (K x H x W vectors).  The
 * iteration runs in whichever of the two spaces is smaller (result.space); the start vector is a fixed counter-based
 * pseudo-random vector, every sum is folded in double in a fixed order: the same arguments give the same bits.
 *   options : maxiter >= 1 Lanczos steps at most; tol >= 0, relative: the first step j with
 *             beta_j |s_j| <= tol theta_j stops (theta_j the largest Ritz value, s_j the last component of its vector);
 *             tol = 0 runs to maxiter or to breakdown.  reserved must be 0.
 *   result  : theta (the value; NaN for a non-finite kernel, 0 for a zero one), residual = beta_j |s_j| (some eigenvalue
 *             lies within it of theta), steps (Lanczos steps the value rests on), matvecs (operator applications
 *             launched), host_reads (waits of the host for the device: one per chunk of 8, 16, 32, 32, ... steps),
 *             space (LASSO_LIP_SPACE_*), dim (of that space), status (LASSO_LIP_*), restarts (times the basis was full
 *             and the iteration went on from the Ritz vector: more than 512 steps, or a basis beyond 1 GiB), and --
 *             history non-NULL -- theta_1 .. theta_steps in a host array of the caller (history_capacity entries).
 * Refusals before any HIP call: null pointers, a bad or non-round-tripping geometry, maxiter < 1, a negative or NaN
 * tol or reserved != 0 are LASSO_ERR_BAD_ARG; any other dtype and geometries beyond the 32-bit block offsets of the
 * convolution kernels LASSO_ERR_UNSUPPORTED (the workspace query returns 0); a short workspace LASSO_ERR_WORKSPACE.
 * The call blocks. */
typedef struct lasso_conv_lip_options {
  int32_t maxiter, reserved;
  double tol;
} lasso_conv_lip_options;
#define LASSO_LIP_CONVERGED 0
#define LASSO_LIP_BREAKDOWN 1             /* an invariant subspace was found (or the basis spans the space): exact */
#define LASSO_LIP_MAXITER 2
#define LASSO_LIP_NONFINITE 3             /* a NaN or Inf reached the recurrence: theta is NaN */
#define LASSO_LIP_SPACE_IMAGE 0
#define LASSO_LIP_SPACE_CODE 1
typedef struct lasso_conv_lip_result {
  double theta, residual;
  int64_t dim;
  int32_t steps, matvecs, host_reads, space, status, restarts;
  int32_t history_capacity, pad_;
  double* history;                        /* nullable */
} lasso_conv_lip_result;
size_t lasso_conv_lip_constant_workspace_bytes(int64_t K, int64_t C, int kh, int kw, int64_t H, int64_t W, int sh, int sw,
                                               int ph, int pw, int transpose, int dtype, int maxiter);
int lasso_conv_lip_constant(const void* w_dev, int64_t K, int64_t C, int kh, int kw, int64_t H, int64_t W, int sh, int sw,
                            int ph, int pw, int transpose, int dtype, const lasso_conv_lip_options* options,
                            lasso_conv_lip_result* result, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- one dense system per batch entry: replace batch_cholesky_solve(), lasso/linear/utils.py:43-58 ----
 * x_i with A_i x_i = b_i for a_dev [nbatch][d][d] (system i at a_dev + i batch_stride, rows lda apart), b_dev [nbatch][d]
 * (rows ldb apart) and x_dev [nbatch][d] (rows ldx apart); strides and leading dimensions in elements; LASSO_F32 or
 * LASSO_F64 (csrc/batch_solve.hip).  batch_stride may be 0: one matrix for every system.  Any lda, ldb, ldx >= d and any
 * element-aligned base pointers are taken as they are.
 * lasso_batch_chol_solve: by Cholesky.  Only the LOWER triangle of each A_i is read (the strict upper triangle may hold
 * anything).  A pivot that is not positive (or NaN) is replaced by 1 and recorded: result.bad_system is the lowest
 * system that met one (-1: none, x_dev holds every solution) and result.bad_minor 1 + the index of its first such pivot;
 * with a bad system x_dev is not a solution for it -- the reference then solves the WHOLE batch by
 * lasso_batch_lu_solve: LU with partial pivoting (the first entry of largest magnitude) on a copy of the full matrix.  A
 * pivot that is exactly zero is recorded the same way (the system is singular) and replaced by 1; a NaN pivot is no
 * error: that system's x is NaN.
 * result.tier (LASSO_BATCH_TIER_*) is the Cholesky kernel that d selects: one wave per system (d <= 32), one workgroup
 * with the packed triangle in LDS (float d <= 256, double d <= 160), or a fixed number of workgroups with their
 * triangles in the workspace (float d <= 1024, double d <= 512): lasso_batch_solve_tier_cap(dtype, tier) is the largest d
 * of a tier, lasso_batch_solve_workgroups(...) the workgroups of the last one (0 for the other two).
 * Every system is solved on its own and in a fixed order of operations: the same arguments give the same bits, and a
 * system's solution does not depend on the rest of the batch.  The calls enqueue on `stream` only, read one record
 * back and block for it.  lasso_batch_solve_workspace_bytes covers both routes.
 * Refusals before any HIP call: null pointers, nbatch < 1, d < 1, a negative batch_stride or a leading dimension below
 * d are LASSO_ERR_BAD_ARG; any other dtype and d beyond the last tier LASSO_ERR_UNSUPPORTED (the workspace query
 * returns 0); a short workspace LASSO_ERR_WORKSPACE.  The inputs are only read; x_dev may not alias one. */
#define LASSO_BATCH_TIER_WAVE 0
#define LASSO_BATCH_TIER_LDS 1
#define LASSO_BATCH_TIER_GENERAL 2
typedef struct lasso_batch_solve_result {
  int64_t bad_system;                     /* -1: none */
  int32_t bad_minor, tier;
} lasso_batch_solve_result;
int lasso_batch_solve_tier_cap(int dtype, int tier);
int lasso_batch_solve_workgroups(int64_t nbatch, int64_t d, int dtype);
size_t lasso_batch_solve_workspace_bytes(int64_t nbatch, int64_t d, int dtype);
int lasso_batch_chol_solve(const void* a_dev, int64_t batch_stride, int64_t lda, const void* b_dev, int64_t ldb, void* x_dev,
                           int64_t ldx, int64_t nbatch, int64_t d, int dtype, lasso_batch_solve_result* result,
                           void* workspace_dev, size_t workspace_bytes, void* stream);
int lasso_batch_lu_solve(const void* a_dev, int64_t batch_stride, int64_t lda, const void* b_dev, int64_t ldb, void* x_dev,
                         int64_t ldx, int64_t nbatch, int64_t d, int dtype, lasso_batch_solve_result* result,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LASSO_HIP_H_ */
