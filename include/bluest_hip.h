/*
 * bluest_hip.h -- C-ABI of libbluest_hip.so: the MI355X (gfx950) implementation of BLUEST's sample-allocation
 * hot path (Phi(m) assembly, V = e0^T Phi^-1 e0, grad V, simplex projection for the SPG solver).
 *
 * This is the drop-in boundary.  Part 1 mirrors, one entry point per function, the reference's only native
 * module `_cmisc_bluest` (/root/reference/bluest/cmisc.cpp:99-110): the same arguments in the same order and
 * the same in-place accumulation contract, as plain pointers and sizes.  Part 2 is the device-resident "plan"
 * that the Python operators SAP / MOSAP (bluest/sap.py:131-143, bluest/mosap.py:86-100) sit on: group tables
 * and per-group inverse covariances stay in HBM, one call evaluates V and grad V for every output.
 *
 * Conventions
 *   - every function returns BLUEST_OK (0) or a BLUEST_ERR_* code; bluest_last_error() gives the message
 *     of the last failure on the calling thread.  Nothing throws, nothing takes ownership of caller memory.
 *   - "hd" pointers (Part 1) may be HOST or DEVICE pointers (detected with hipPointerGetAttributes); host
 *     buffers are staged through HBM and the call is synchronous.  "dev" pointers (Part 2) must be device
 *     pointers; those calls are asynchronous on `stream` (a hipStream_t passed as void*, NULL = default).
 *   - arithmetic is IEEE float64, indices int64, exactly as the reference (cmisc.cpp uses `long int`).
 *   - there is NO CPU fallback: without a usable GPU every compute entry point fails with BLUEST_ERR_NOGPU.
 */
#ifndef BLUEST_HIP_H
#define BLUEST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLUEST_ABI_VERSION 1

#define BLUEST_OK          0
#define BLUEST_ERR_ARG     1   /* bad argument (null pointer, size out of range) */
#define BLUEST_ERR_HIP     2   /* a HIP runtime call failed */
#define BLUEST_ERR_NOGPU   3   /* no gfx950 device visible */
#define BLUEST_ERR_STATE   4   /* plan not finalized / already finalized */

#define BLUEST_MAX_MODELS  64  /* n  (Phi is n x n) */
#define BLUEST_MAX_GROUP   32  /* k_max: largest group a plan or bluest_group_pinv takes */

/* per-(candidate,output) evaluation status written by bluest_plan_solve / bluest_plan_eval */
#define BLUEST_EVAL_OK         0
#define BLUEST_EVAL_INF        1  /* max|m| < 0.05  -> V = +inf, grad = +inf   (bluest/misc.py:464,484)      */
#define BLUEST_EVAL_NO_MODEL0  2  /* model 0 not sampled -> reference asserts   (bluest/misc.py:470)          */
#define BLUEST_EVAL_SINGULAR   3  /* restricted Phi not positive definite       (bluest/misc.py:473-474)      */

int         bluest_abi_version(void);
const char *bluest_last_error(void);
int         bluest_device_count(int *count);
int         bluest_device_name(char *buf, int buflen);

/* ------------------------------------------------------------------------------------------------------
 * Part 1 -- stateless mirrors of _cmisc_bluest (reference: bluest/cmisc.cpp)
 * ---------------------------------------------------------------------------------------------------- */

/* replaces assemble_psi_c (cmisc.cpp:10-23): psi[(N*g_j+g_l), i] += invcov_i[j,l];
 * psi is C-order (N*N, Lk), zero-filled by the caller (bluest/misc.py:601). */
int bluest_assemble_psi(double *psi_hd, int N, int k, int64_t Lk, const int64_t *groupsk_hd,
                        const double *invcovsk_hd);

/* replaces objectiveK_c<double> (cmisc.cpp:25-40, overload :104): PHI[N*g_j+g_l] += m_i*invcov_i[j,l] */
int bluest_objectiveK_f64(double *PHI_hd, int N, int k, int64_t Lk, const double *mk_hd,
                          const int64_t *groupsk_hd, const double *invcovsk_hd);

/* replaces objectiveK_c<long int> (cmisc.cpp:25-40, overload :105): integer sample counts */
int bluest_objectiveK_i64(double *PHI_hd, int N, int k, int64_t Lk, const int64_t *mk_hd,
                          const int64_t *groupsk_hd, const double *invcovsk_hd);

/* replaces gradK_c (cmisc.cpp:58-72): grad_i += v[g]^T invcov_i v[g], v = invPHI[0] (length >= max(g)+1) */
int bluest_gradK(double *grad_hd, int k, int64_t Lk, const int64_t *groupsk_hd, const double *invcovsk_hd,
                 const double *invPHI_0_hd, int n_models);

/* replaces cleanupK_c (cmisc.cpp:42-56), INCLUDING its `=` (not `+=`) at line 51: only the l=k-1 term
 * survives, X[g_j, i] = invcov_i[j,k-1]*v[g_{k-1}].  X is C-order (N, Lk). */
int bluest_cleanupK(double *X_hd, int k, int64_t Lk, const int64_t *groupsk_hd, const double *invcovsk_hd,
                    const double *invPHI_0_hd, int n_models);

/* replaces hessKQ_c (cmisc.cpp:74-97): hess[ik,iq] += a_k(ik)^T invPHI[g^k,g^q] a_q(iq),
 * a_k(ik)_j = sum_l v[g^k_l] invcov^k[l,j]; hess is C-order (Lk, Lq); invPHI is C-order (N, N). */
int bluest_hessKQ(double *hess_hd, int N, int k, int q, int64_t Lk, int64_t Lq, const int64_t *groupsk_hd,
                  const int64_t *groupsq_hd, const double *invcovsk_hd, const double *invcovsq_hd,
                  const double *invPHI_hd);

/* replaces the per-group numpy.linalg.pinv(C[g,g]) loop of SAP.__init__ (bluest/sap.py:69-79):
 * invcov_i = pinv(C[g_i,g_i]) (symmetric eigen-decomposition, cut-off 1e-15*max|lambda| as numpy's default
 * rcond), flattened C-order (Lk*k*k).  1 <= k <= BLUEST_MAX_GROUP: one thread per group up to 16 models, one wavefront per group
 * (block and eigenvectors in LDS) for 17..32; BLUEST_ERR_STATE if a group's Jacobi sweeps do not converge. */
int bluest_group_pinv(const double *C_hd, int N, int k, int64_t Lk, const int64_t *groupsk_hd,
                      double *invcovsk_hd);

/* ------------------------------------------------------------------------------------------------------
 * Part 2 -- device-resident plan (operator level: bluest/sap.py:131-143, bluest/mosap.py:86-100)
 *
 * A plan holds, for each output o, the groups and inverse covariances of SAP_o re-laid out in HBM for the two
 * streaming passes (destination-major symmetric CSR for the Phi pass, group-major 64-wide tiles for the
 * gradient pass), plus the map from SAP_o's local group numbering to the global allocation vector m
 * (`mappings[o]` of bluest/mosap.py:54-67).
 * ---------------------------------------------------------------------------------------------------- */
typedef struct bluest_plan_s *bluest_plan_t;

/* n_models = N (<= BLUEST_MAX_MODELS); L_global = length of the global allocation vector m */
int bluest_plan_create(bluest_plan_t *plan, int n_models, int64_t L_global);
int bluest_plan_destroy(bluest_plan_t plan);

/* Plan lifetime vs hipGraph capture.  Releasing a plan frees device memory, and a free issued while some stream of the
 * process is being captured invalidates that capture.  Callers whose host language may drop a plan at any time (garbage
 * collection, reference counting) bracket their captures: bluest_capture_guard(1) before hipStreamBeginCapture,
 * bluest_capture_guard(0) after hipStreamEndCapture.  While a guard is open bluest_plan_destroy only parks the plan; the
 * closing call releases everything parked.  Guards nest.  bluest_deferred_plans reports how many plans are parked. */
int bluest_capture_guard(int on);
int bluest_deferred_plans(int *count);

/* Add output o (call once per output, in order).  K = max group size of this output (1..BLUEST_MAX_GROUP); sizes[k-1] = L_k for
 * k = 1..K; groups = concat_k (L_k*k) model indices; invcovs = concat_k (L_k*k*k) (HOST pointers, copied);
 * mapping = L_o global indices (m_o = m[mapping]) or NULL for the identity (requires L_o == L_global). */
int bluest_plan_add_output(bluest_plan_t plan, int K, const int64_t *sizes, const int64_t *groups,
                           const double *invcovs, const int64_t *mapping);

/* Same, but the per-group pseudo-inverses are computed on the GPU from the n x n covariance C (host pointer);
 * if invcovs_out (host) is non-NULL the inverses are also returned in the reference layout. */
int bluest_plan_add_output_cov(bluest_plan_t plan, const double *C, int K, const int64_t *sizes,
                               const int64_t *groups, const int64_t *mapping, double *invcovs_out);

/* Reference-layout pseudo-inverses of output o (concat_k L_k*k*k doubles) back to a host buffer: they stay on the device
 * after bluest_plan_add_output_cov (the plan is built from them there) and are only fetched when the host asks, e.g. for the
 * `invcovs` attribute of SAP (bluest/sap.py:69-79).  bluest_plan_gather_invcovs fetches the k x k blocks of SOME groups of
 * output o (local indices, any order, blocks written one after the other) -- what a restricted plan needs. */
int bluest_plan_get_invcovs(bluest_plan_t plan, int output, double *invcovs_out);
int bluest_plan_gather_invcovs(bluest_plan_t plan, int output, const int64_t *local_idx, int64_t n, double *out);

/* A NEW finalized plan over the sub-list `keep` (n_keep strictly ascending global group indices) of a finalized plan's groups:
 * allocation vectors of the new plan have length n_keep (entry i = group keep[i]); every output keeps the groups whose global
 * index is in `keep`, with the parent's pseudo-inverses gathered on the device (no host round trip).  This is the operator of
 * bluest/sap.py:53-79 built on a subset of the groups -- the working set of the solver.  Fails with BLUEST_ERR_ARG if some
 * output would be left without a group containing model 0 (its variance would be infinite whatever the allocation).
 * bluest_plan_output_layout returns what the host mirror needs of one output: K, the sizes L_k (K entries) and, if `mapping`
 * is non-NULL, the global indices of its groups (sum L_k entries); pass sizes = NULL to query K alone. */
int bluest_plan_restrict(bluest_plan_t parent, const int64_t *keep, int64_t n_keep, int max_candidates, bluest_plan_t *restricted);
int bluest_plan_output_layout(bluest_plan_t plan, int output, int *K, int64_t *sizes, int64_t *mapping);

/* Build the HBM layouts.  max_candidates = largest number of allocation vectors evaluated per call. */
int bluest_plan_finalize(bluest_plan_t plan, int max_candidates);

int bluest_plan_n_outputs(bluest_plan_t plan, int *n_outputs);
/* total length of the concatenated per-output gradient (sum_o L_o) and the offset of output o inside it */
int bluest_plan_grad_layout(bluest_plan_t plan, int64_t *grad_len, int64_t *offsets /* n_outputs */);
/* HBM bytes the Phi pass / gradient pass stream per candidate (actual layout, for roofline accounting) */
int bluest_plan_traffic(bluest_plan_t plan, int64_t *phi_bytes, int64_t *grad_bytes);
/* MATRIX-FREE evaluation (csrc/matfree.hip; the form BASELINE.json's north star names): the inverse of every group's covariance
 * block (bluest/sap.py:69-79) is recomputed in registers where bluest/cmisc.cpp:25-40,58-72 read the stored one, so an evaluation
 * reads the groups' model indices and m only.  Chosen at bluest_plan_finalize for plans that qualify (outputs given by their
 * covariance, group sizes <= 8 (MF_KMAX), <= 48 models, every block safely positive definite; a plan with any wider group, up to
 * BLUEST_MAX_GROUP, always evaluates on stored inverses, whatever their size) when BLUEST_MATFREE=1, or on its own when the
 * stored streams exceed 64 MB; single-candidate bluest_plan_eval / bluest_plan_phi / bluest_plan_solve_grad then take it.
 * The GRADIENT pass alone is matrix-free on every plan that qualifies (BLUEST_MATFREE=2 forces exactly that, 0 forbids everything): the
 * stored Phi pass is then followed by one kernel that folds its partials, solves and recomputes the group factors for the gradient.
 * *matfree = 1: Phi and gradient matrix-free, 2: the gradient only, 0: stored inverses everywhere; *mf_bytes = bytes a fully
 * matrix-free evaluation reads and writes per candidate. */
int bluest_plan_matfree(bluest_plan_t plan, int *matfree, int64_t *mf_bytes);
/* size in doubles of one candidate's Phi-pass result: n_outputs * (N*N + 2*N + 1), see bluest_plan_phi */
int bluest_plan_phi_len(bluest_plan_t plan, int64_t *len);

/* Phase A (a4/a5/a6 of SURVEY.md 8a): for every candidate c and output o write into phi_dev[c][o] a record of
 * N*N + 2*N + 1 doubles: Phi_o(m_c) WITHOUT the delta*I term (N*N); then for each model a, 1.0 if some group
 * containing a has |m_i| > 1e-6 else 0.0 (N doubles: the `idx` of bluest/misc.py:453-457); then for each model
 * a, 1.0 if some group containing a has m_i != 0 (N doubles: the support of Phi); then 1.0 if max|m| >= 0.05
 * (1 double, bluest/misc.py:464).  All fields are sums/indicators, so partial records from several GPUs (each
 * holding a shard of the groups) combine with one all-reduce(SUM) and are then tested with `> 0`.
 * m_dev: n_cand vectors of length L_global, m_stride doubles apart. */
int bluest_plan_phi(bluest_plan_t plan, const double *m_dev, int n_cand, int64_t m_stride, double *phi_dev,
                    void *stream);

/* Diagnostics: launch ONLY the Phi chunk kernel (partials stay in the plan's workspace); lets bench.py time
 * the streaming kernel alone with HIP events. */
int bluest_plan_phi_chunks(bluest_plan_t plan, const double *m_dev, int n_cand, int64_t m_stride, void *stream);

/* Phase B (a7/a8): from the (all-reduced) records, V = (Phi[idx,idx]^-1)_00 on the sampled models
 * (bluest/misc.py:467-472,490), v = row 0 of pinv(Phi + delta I) (bluest/misc.py:487), status codes above.
 * var_dev: n_cand*n_outputs, v_dev: n_cand*n_outputs*N, status_dev: n_cand*n_outputs int32. */
int bluest_plan_solve(bluest_plan_t plan, const double *phi_dev, int n_cand, double delta, double *var_dev,
                      double *v_dev, int32_t *status_dev, void *stream);

/* Phase B for a RANK-DEFICIENT restricted Phi (status BLUEST_EVAL_SINGULAR from bluest_plan_solve / _eval): what the
 * reference's variance_GH returns there -- V = pinv(Phi[idx,idx])[0,0] (bluest/misc.py:490) and v = row 0 of pinv(Phi)
 * (bluest/misc.py:487) with numpy's cut-off (eigenvalues <= 1e-15 * max|lambda| dropped), by a cyclic Jacobi
 * eigen-decomposition.  Same arguments as bluest_plan_solve; the status is never BLUEST_EVAL_SINGULAR.  Rare path:
 * one wavefront per (candidate, output), ~ms. */
int bluest_plan_solve_pinv(bluest_plan_t plan, const double *phi_dev, int n_cand, double delta, double *var_dev,
                           double *v_dev, int32_t *status_dev, void *stream);

/* Phase C (a9): grad_o,i = -v[g_i]^T invcov_i v[g_i] for every group of every output (this GPU's shard);
 * grad_dev: n_cand rows of grad_len doubles (row stride grad_stride); +inf where status == BLUEST_EVAL_INF. */
int bluest_plan_grad(bluest_plan_t plan, const double *v_dev, const int32_t *status_dev, int n_cand,
                     double *grad_dev, int64_t grad_stride, void *stream);

/* A + B (+ C if grad_dev != NULL) back to back on one stream, single GPU (MOSAP.variances / variance_GH). */
int bluest_plan_eval(bluest_plan_t plan, const double *m_dev, int n_cand, int64_t m_stride, double delta,
                     double *var_dev, double *grad_dev, int64_t grad_stride, int32_t *status_dev, void *stream);

/* Fold the per-output gradients back onto the global allocation vector:
 * out[c][j] = scale[j] * sum_o coef[c][o] * grad_o[c][local_o(j)]   (0 where output o has no group j).
 * coef_dev: n_cand*n_outputs; scale_dev: L_global or NULL (=1). */
int bluest_plan_combine_grad(bluest_plan_t plan, const double *grad_dev, int64_t grad_stride,
                             const double *coef_dev, const double *scale_dev, int n_cand, double *out_dev,
                             int64_t out_stride, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Part 3 -- SPG building block (NEW solver="spg"; algorithm of bluest/spg.py:39-132 with proj = simplex)
 *
 * p = argmin sum_i (p_i - u_i)^2 / s_i  over {p >= 0, sum p = z},  u = x - lambda * s * g,  d = p - x.
 *   floor == 0 : s = 1, the plain Euclidean projection P_simplex(x - lambda*g) (reference-style SPG step);
 *   floor  > 0 : s_i = max(x_i, floor), the variable-metric ("entropic") SPG step used by solver="spg" by default.
 * stats_dev[0] = g.d, stats_dev[1] = max|d|, stats_dev[2] = tau (threshold on the ratios, after shifting by their
 * max), stats_dev[3] = number of positive entries of p.  g_dev may be NULL (then lambda is ignored: p = P(x)).
 * d_dev or p_dev may be NULL.
 * work_dev: NULL, or bluest_simplex_workspace_doubles(L) doubles of scratch, ZERO-FILLED once (hipMemset) before its
 * first use and then left alone between calls: with it, vectors longer than 4096 are projected by ONE launch of up to 64
 * workgroups (one workgroup alone moves only ~25-60 GB/s) that exchange their partial sums through tagged mailboxes in
 * the scratch, and the threshold search is warm-started from the previous call on the same scratch (typically 3 passes
 * instead of 10-15).  The result does not depend on the hint.  Keep one scratch per stream: two projections running
 * concurrently on the same scratch would read each other's mailboxes.
 */
int bluest_simplex_workspace_doubles(int64_t L, int64_t *n_doubles);
int bluest_simplex_project(const double *x_dev, const double *g_dev, double lambda, double z, double floor, int64_t L,
                           double *p_dev, double *d_dev, double *stats_dev, double *work_dev, void *stream);

/* Device-resident SPG iteration (bluest/spg.py:68-106 with the control flow on the GPU).  The solver state is an
 * array of BLUEST_SPG_STATE_DOUBLES doubles in HBM (layout: csrc/spg.hip SPG_*, bluest_amd/spg_device.py);
 * every kernel below reads its scalars (lambda, alpha, f, history ...) from it and is a no-op once state[DONE] or
 * state[FAIL] is set, so the loop is a fixed launch sequence of identical STEPS -- direction, T predicated line-search slots,
 * (gradient,) Barzilai-Borwein update -- that needs no host round trip (plain stream launches, or captured in a hipGraph).
 * A trial rejected in the last slot of a step sets state[PENDING]: the next direction launch then forms the next trial point
 * x + alpha*d instead of a new direction and the update stays gated off, i.e. the line search of spg.py:9-35 simply continues
 * in the next step; a step length below 1e-300 or state[MAXFEV] evaluations set state[FAIL].
 *   bluest_plan_set_gate   : the plan's kernels (Phi chunks, solve, gradient, combine) skip when *enable_dev == 0;
 *                            always_v != 0 makes every solve also produce v (kept in the plan workspace)
 *   bluest_spg_direction   : d = P_s(x - lambda*s*g) - x with lambda = state[LAMBDA]; g.d -> state (the multi-workgroup kernel
 *                            leaves per-workgroup partials that bluest_spg_decide folds); optionally also the first trial
 *                            point (alpha = 1): xnew = x + d, m = scale*xnew, *enable = 1.  While state[PENDING]: no new
 *                            direction, xnew = x + alpha*d, m = scale*xnew instead
 *   bluest_spg_trial       : xnew = x + alpha*d, m = scale*xnew, *enable = 1 -- unless the iteration already accepted
 *   bluest_spg_decide      : F(trial) from the per-output variances (p-norm / max), nonmonotone Armijo test
 *                            (spg.py:17,32), safeguarded quadratic interpolation of alpha (spg.py:18-26)
 *                            on the last slot of an iteration also *enable = accepted (gates gradient + combine)
 *   bluest_spg_update      : s, y, Barzilai-Borwein lambda (spg.py:91-106), x <- xnew, g <- gnew, history
 *                            (work_dev: 1024 doubles of scratch for the per-block partial sums)
 *   bluest_spg_converged   : gpmax = max|P_s(x - s*g) - x| -> state; sets state[DONE] when gpmax <= state[EPS] (spg.py:68,99-101)
 */
#define BLUEST_SPG_STATE_DOUBLES 256
int bluest_plan_set_gate(bluest_plan_t plan, const int32_t *enable_dev, int always_v);
/* One line-search slot in two launches instead of three: bluest_plan_eval (value only, single candidate) with
 * bluest_spg_decide fused into the tail of the solve kernel -- the output workgroup that finishes last evaluates the decision. */
int bluest_plan_eval_decide(bluest_plan_t plan, const double *m_dev, double delta, double *var_dev, int32_t *status_dev,
                            double *state_dev, int last_slot, int32_t *enable_dev, void *stream);
/* The same with the gradient of the trial point (bluest_plan_eval's fused solve + gradient launch, decision in its tail): the
 * gradient of a rejected trial is wasted work (~2 us), the gradient of the accepted one is what the update needs -- no separate
 * gradient launch after the line search.  grad_dev: grad_len doubles (bluest_plan_grad_layout). */
int bluest_plan_eval_grad_decide(bluest_plan_t plan, const double *m_dev, double delta, double *var_dev, double *grad_dev,
                                 int32_t *status_dev, double *state_dev, int last_slot, int32_t *enable_dev, void *stream);
/* Group-sharded plans: solve + gradient of this GPU's shard FROM the all-reduced Phi record (bluest_plan_phi, summed over the
 * ranks) in one launch; state_dev != NULL adds the line-search decision in its tail (as bluest_plan_eval_grad_decide). */
int bluest_plan_solve_grad(bluest_plan_t plan, const double *rec_dev, double delta, double *var_dev, double *grad_dev,
                           int32_t *status_dev, double *state_dev, int last_slot, int32_t *enable_dev, void *stream);
int bluest_plan_v_workspace(bluest_plan_t plan, const double **v_dev, const int32_t **status_dev);
int bluest_spg_direction(const double *x_dev, const double *g_dev, double *state_dev, double z, double floor, int64_t L,
                         double *d_dev, const double *scale_dev, double *xnew_dev, double *m_dev, int32_t *enable_dev,
                         double *work_dev, void *stream);
int bluest_spg_converged(const double *x_dev, const double *g_dev, double *state_dev, double z, double floor, int64_t L,
                         double *work_dev, void *stream);
int bluest_spg_trial(const double *x_dev, const double *d_dev, const double *scale_dev, const double *state_dev,
                     double *xnew_dev, double *m_dev, int32_t *enable_dev, int64_t L, void *stream);
int bluest_spg_decide(double *state_dev, const double *var_dev, const int32_t *status_dev, int n_out, int last_slot,
                      int32_t *enable_dev, void *stream);
int bluest_spg_update(double *x_dev, double *g_dev, const double *xnew_dev, const double *gnew_dev, double *state_dev,
                      double floor, int64_t L, double *work_dev, void *stream);
/* the same with the gradient fold of bluest_plan_combine_grad fused in (coefficients from state[COEF..]): gnew is formed on
 * the fly from the per-output gradients grad_dev (single candidate) */
int bluest_spg_update_fused(bluest_plan_t plan, double *x_dev, double *g_dev, const double *xnew_dev, const double *grad_dev,
                            const double *scale_dev, double *state_dev, double floor, double *work_dev, void *stream);
/* gradient of the accepted trial point + bluest_spg_update_fused in one call: bluest_plan_grad followed by the fused update, or --
 * for small plans (K_tot <= 4096: the solver's working set) -- ONE single-workgroup kernel that does both.  v_dev / status_dev as
 * handed out by bluest_plan_v_workspace. */
int bluest_spg_finish(bluest_plan_t plan, const double *v_dev, const int32_t *status_dev, double *x_dev, double *g_dev,
                      const double *xnew_dev, double *grad_dev, const double *scale_dev, double *state_dev, double floor,
                      double *work_dev, void *stream);

/* n_iterations steps of the loop (bluest_spg_direction, `slots` x [bluest_spg_trial,] bluest_plan_eval_grad_decide,
 * bluest_spg_update_fused; on plans with K_tot <= 4096: bluest_plan_eval_decide and bluest_spg_finish), then
 * bluest_spg_converged if check_last: one host call enqueues the launch sequence of a whole window on `stream`.  Arguments as in the calls it is made of; v_ws_dev from bluest_plan_v_workspace; proj_work_dev as work_dev of
 * bluest_simplex_project (may be NULL for L <= 4096). */
int bluest_spg_window(bluest_plan_t plan, double *x_dev, double *g_dev, double *d_dev, double *xnew_dev, double *m_dev,
                      const double *scale_dev, double *state_dev, double *var_dev, int32_t *status_dev, double *grad_dev,
                      int32_t *enable_dev, double *work_dev, double *proj_work_dev, const double *v_ws_dev, double floor, int slots,
                      int n_iterations, int check_last, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Part 4 -- integer projection batch (bluest/misc.py:228-311 multi, :313-382 single)
 *
 * The reference forms phis = basephi + psi[:, idx] @ ms for up to 2^LL integer candidates and takes
 * pinv(phis)[:,0,0] (misc.py:293-294, 368-369).  Here: base_dev = n_out x (N*N) base information matrices,
 * cols_dev = n_out x LL x (N*N) columns of psi for the LL free groups (zero where an output lacks the group),
 * ms_dev = n_cand x LL candidate values (row-major), V_dev = n_cand x n_out variances (+inf where the candidate's
 * information matrix is singular on its support or does not sample model 0).
 * ---------------------------------------------------------------------------------------------------- */
int bluest_intproj_eval(int N, int n_out, int LL, const double *base_dev, const double *cols_dev, const double *ms_dev,
                        int64_t n_cand, double *V_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Part 5 -- one-shot all-reduce of the Phi records between the GPUs of ONE node
 *
 * NEW (the reference's optimiser runs on one MPI rank, bluest/blue_models.py:508-526).  One process per GPU.  Each rank
 * creates its mailboxes, the ranks swap the 64-byte handles by any means (torch.distributed all_gather in bluest_amd/dist.py),
 * connect, and then every bluest_xchg_allreduce_sum call -- issued by ALL ranks, in the same order -- replaces buf by the sum over
 * ranks in ONE kernel launch per rank: direct peer writes of tagged 8-byte granules into fine-grained memory shared with
 * hipIpc (csrc/xchg.hip).  The sum is formed in rank order, so all ranks hold identical bits.  Asynchronous on `stream`;
 * bluest_xchg_status reports the number of completed calls and whether a wait ever timed out (the result is then NaN).
 * ---------------------------------------------------------------------------------------------------- */
#define BLUEST_XCHG_HANDLE_BYTES 64
typedef struct bluest_xchg_s *bluest_xchg_t;
int bluest_xchg_create(bluest_xchg_t *xchg, int world, int rank, int64_t max_doubles, void *handle_out /* 64 bytes */);
int bluest_xchg_connect(bluest_xchg_t xchg, const void *all_handles /* world * 64 bytes, rank order */);
int bluest_xchg_allreduce_sum(bluest_xchg_t xchg, double *buf_dev, int64_t n_doubles, void *stream);
int bluest_xchg_status(bluest_xchg_t xchg, int64_t *calls, int *timed_out);
int bluest_xchg_destroy(bluest_xchg_t xchg);

/* ------------------------------------------------------------------------------------------------------
 * Part 6 -- second-order finish of solver="spg" (NEW; csrc/newton.hip, restated in numpy in oracle/master_newton.py)
 *
 * The reference hands  min_m max_o V_o(m)/s_o  s.t.  cost.m = B, m >= 0  to third-party NLP solvers together with the Hessian
 * of bluest/misc.py:497-503 / bluest/cmisc.cpp:74-97 (bluest/sap.py:387-456, bluest/mosap.py:578-673).  Here, in the scaled
 * variable x_i = cost_i m_i / B on the unit simplex:
 *   phase 1  bluest_ma_update       multiplicative algorithm on ALL groups (one evaluation + one elementwise kernel per step)
 *   phase 2  bluest_master_newton   Levenberg-Marquardt damped active-set Newton (SQP) on a support of <= 64 groups, one launch of
 *                                   one workgroup per master problem;
 *            bluest_support_point   support vector -> allocation of the full problem (+ uniform background of weight eps);
 *            bluest_price           reduced costs c_i = (B/cost_i) sum_o (mu_o/s_o) v_{o,g_i}^T C_{i,o}^-1 v_{o,g_i} of all groups
 *                                   from the gradient at that point: candidates to enter the support, and max_i c_i, which gives
 *                                   the certified bound  F* >= A^2 / (4 max_i c_i),  A = 2 sum_o (mu_o/s_o) V_o  (weak duality).
 * ---------------------------------------------------------------------------------------------------- */
/* largest support the single-workgroup master can hold for this plan (LDS budget); 0: does not fit */
int bluest_master_max_support(bluest_plan_t plan, int *s_max);
/* support_host: S strictly ascending GLOBAL group indices (host); cc_host: B / cost_j (host, S); s_dev: output scales (n_out);
 * bg_dev: n_out x N x N matrices eps_bg * Phi_o(uniform allocation) (device; may be NULL when eps_bg == 0);
 * x_dev (S): start in, solution out; mu_dev (n_out): multipliers in (any, e.g. 1/n_out) / out;
 * out_dev (16 + n_out doubles): F, lam, kkt residual, spread, iterations, evaluations, linear solves, status (0 converged,
 * 1 stalled, 2 start not evaluable), damping, lam at x, ..., then r_o = V_o/s_o at the solution.  Asynchronous on `stream`
 * after one small synchronous descriptor upload. */
int bluest_master_newton(bluest_plan_t plan, int S, const int64_t *support_host, const double *cc_host, const double *s_dev,
                         const double *bg_dev, double eps_bg, double *x_dev, double *mu_dev, double tol, int maxit,
                         double *out_dev, void *stream);
/* the same master problem with per-model sample caps (max_model_samples, bluest/sap.py:222-240, bluest/mosap.py:326-344):
 * sum over the support groups j containing model cap_model[c] of (1 - eps_bg) cc_j x_j <= cap_b[c]  (ncap <= 64; host arrays;
 * the start x must satisfy them).  Caps at their bound are equality rows of the SQP step, a cap whose multiplier comes out
 * negative leaves, trial points are repaired / pulled back onto the feasible set.  nu_dev (ncap): cap multipliers out. */
int bluest_master_newton_capped(bluest_plan_t plan, int S, const int64_t *support_host, const double *cc_host, const double *s_dev,
                                const double *bg_dev, double eps_bg, double *x_dev, double *mu_dev, double tol, int maxit,
                                double *out_dev, int ncap, const int32_t *cap_model_host, const double *cap_b_host, double *nu_dev,
                                void *stream);
/* x_i <- x_i * cc_i * sum_o wgt_o q_{o,i}/s_o / sum_o wgt_o r_o,  m_i = cc_i x_i;  var/status/grad as bluest_plan_eval left them
 * for the allocation m; wgt_o ~ r_o^(p-1) (p-norm surrogate of the max) */
int bluest_ma_update(bluest_plan_t plan, const double *var_dev, const int32_t *status_dev, const double *grad_dev,
                     const double *s_dev, const double *cc_dev, double p, double *x_dev, double *m_dev, void *stream);
/* single-output plans on all groups (identity mapping): one step of phase 1 in TWO launches -- the evaluation of m_dev, whose fused
 * solve + gradient kernel applies the update above to x_dev / m_dev in its tile wavefronts instead of writing the gradient.  Same
 * iterates as bluest_plan_eval + bluest_ma_update, bit for bit.  BLUEST_ERR_STATE for any other plan. */
int bluest_plan_is_identity(bluest_plan_t plan, int *yes);      /* every output on all groups, local index = global index */
int bluest_plan_eval_ma(bluest_plan_t plan, double *m_dev, double *var_dev, int32_t *status_dev, const double *s_dev,
                        const double *cc_dev, double *x_dev, void *stream);
/* *kmax = the widest group bluest_plan_eval_ma accepts on this plan: 12 on stored inverses, 8 under matrix-free evaluation, 0 when
 * the plan does not qualify at all (more than one output, not the identity mapping, or gated).  A plan whose widest group exceeds
 * it (a finalized plan's widest group: bluest_plan_kmax) steps phase 1 with bluest_plan_eval + bluest_ma_update instead. */
int bluest_plan_eval_ma_kmax(bluest_plan_t plan, int *kmax);
/* *kmax = the widest group over all outputs of a finalized plan (<= BLUEST_MAX_GROUP) */
int bluest_plan_kmax(bluest_plan_t plan, int *kmax);
/* Launch configuration (read-only, host only): the kernel instantiation each family of an evaluation of n_cand candidates takes on
 * this plan, decided by the same helpers the launchers call.  cfg receives BLUEST_LC_COUNT entries, indexed by BLUEST_LC_*: */
#define BLUEST_LC_PATH           0   /* bluest_plan_eval: 0 Phi pass + fold/solve + k_grad_tiles, 1 Phi pass + fused k_solve_grad,
                                        2 k_phi_matfree + k_solve_grad_mf, 3 stored Phi pass + k_solve_grad_mf */
#define BLUEST_LC_PHI_OB         1   /* stored Phi pass: 0 plain k_phi_chunks, else OB of k_phi_chunks_shared */
#define BLUEST_LC_COLS16         2   /* 1: uint16 column indices, 0: int32 */
#define BLUEST_LC_NT             3   /* NT of the fold + solve kernels */
#define BLUEST_LC_FOLD_THREADS   4   /* their workgroup size */
#define BLUEST_LC_SOLVE_GRAD_KU  5   /* KU of k_solve_grad */
#define BLUEST_LC_FUSED_TPB      6   /* tile wavefronts per workgroup of that instantiation */
#define BLUEST_LC_TILES_PER_WG   7   /* tiles per workgroup the plan launches it with (follows the device's compute units) */
#define BLUEST_LC_GRAD_TILES_KU  8   /* KU of k_grad_tiles */
#define BLUEST_LC_MATFREE        9   /* as bluest_plan_matfree */
#define BLUEST_LC_MF_NW         10   /* NW of k_phi_matfree (0: no matrix-free state) */
#define BLUEST_LC_MF_NT         11   /* NT of k_solve_grad_mf */
#define BLUEST_LC_MF_KU         12   /* KU of k_solve_grad_mf */
#define BLUEST_LC_ITERS         13   /* 256-entry blocks per chunk of the stored Phi pass */
#define BLUEST_LC_KMAX          14
#define BLUEST_LC_COUNT         15
int bluest_plan_launch_config(bluest_plan_t plan, int n_cand, int32_t *cfg);
/* the instantiation set the library is built with along one axis (BLUEST_LC_PHI_OB, _NT, _FOLD_THREADS, _SOLVE_GRAD_KU, _FUSED_TPB,
 * _GRAD_TILES_KU, _MF_NW, _MF_NT, _MF_KU; the matrix-free ones within what a matrix-free plan may have): *n values, the first
 * min(*n, cap) of them into values */
int bluest_launch_set(int axis, int32_t *values, int cap, int *n);
/* Diagnostic: the cross-lane reductions of csrc/common.hpp that do not use the LDS crossbar, seen lane by lane.  One wavefront per
 * row of 64 doubles of in_dev (n_rows x 64); every output is n_rows x 64 and holds what EACH lane ends with: sum_dev the wave sum,
 * max_dev the wave maximum, quad_dev the sum over the lane's quad in the fold's order ((l^1) first, then (l^2)), isum_dev
 * (int64) the integer wave sum of the rows' bit patterns shifted right by 8 (so that nothing overflows). */
int bluest_wave_reduce_probe(const double *in_dev, int64_t n_rows, double *sum_dev, double *max_dev, double *quad_dev,
                             int64_t *isum_dev, void *stream);
/* Diagnostic: wave_sum_multi of csrc/common.hpp, the reduction of ob = 2, 4 or 8 sums at once in the tail of k_phi_chunks_shared.
 * in_dev is n_rows x ob x 64 doubles, one wavefront per row; out_dev (n_rows x ob) receives each vector's wave sum, written by the
 * lane that kernel stores it from. */
int bluest_wave_reduce_multi_probe(const double *in_dev, int64_t n_rows, int ob, double *out_dev, void *stream);
/* m_i = cc_i ((1 - eps) x_S[i in S] + eps / L); sup_dev ascending */
int bluest_support_point(int64_t L, int S, const int64_t *sup_dev, const double *xs_dev, const double *cc_dev, double eps,
                         double *m_dev, void *stream);
/* after bluest_plan_eval (with gradient) of the priced allocation on the same stream.  c_sup_dev (S): c_i of the support
 * entries; top_val_dev / top_idx_dev (64 * 16): per workgroup the 16 largest (c_i, i); y0_dev (n_out): component 0 of the
 * vectors v_o the quadratic forms were taken with -- the bound's A = 2 sum_o (mu_o/s_o) y0_o.  S <= 0: BLUEST_ERR_ARG */
#define BLUEST_PRICE_CANDIDATES 1024
int bluest_price(bluest_plan_t plan, const double *grad_dev, const double *mu_dev, const double *s_dev, const double *cc_dev,
                 int S, const int64_t *sup_dev, double *c_sup_dev, double *top_val_dev, int64_t *top_idx_dev, double *y0_dev,
                 void *stream);

/* bluest_price with sample caps: capmask_dev (L_global x uint64, bit c: the model of cap c is in the group), nu_dev (cap
 * multipliers of bluest_master_newton_capped), master_out_dev (its result record: F at [0]); the reduced costs become
 * c_i - (B/cost_i) F^2 sum_{c in mask_i} nu_c */
int bluest_price_capped(bluest_plan_t plan, const double *grad_dev, const double *mu_dev, const double *s_dev, const double *cc_dev,
                        int S, const int64_t *sup_dev, double *c_sup_dev, double *top_val_dev, int64_t *top_idx_dev, double *y0_dev,
                        const uint64_t *capmask_dev, const double *nu_dev, const double *master_out_dev, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Part 7 -- MFMC model-subset search (bluest/blue_models.py:795-865; allocation misc.py:78-130, rounding misc.py:384-413,
 * low-budget scheme misc.py:416-449).  Local model index 0 is model 0, p = 1..nb the neighbours of model 0 in the intersection of
 * the coupling graphs.  Host arrays: w (nb+1) costs; s, rho (n_out x (nb+1)) standard deviations and correlations with model 0;
 * eps2 / epsm2 (n_out) eps**2 and eps**-2 (eps mode only); perm (n_out x (nb+1)) local indices by decreasing |rho|, model 0
 * first; adj (nb) bit q-1 set when neighbours p and q are coupled.  Searches every clique through model 0 (2^nb bitmasks) and
 * returns the reference's argmin (enumeration order on ties): best_mask (bit p-1 = neighbour p), best_combo (n_out: the index
 * of the floor/ceil combination the rounding chose, bit j = ub of the j-th entry of get_feasible_integer_bounds; 0 when no
 * rounding), best_obj, status.  Synchronous on `stream`; allocates and frees its own device memory.
 * --------------------------------------------------------------------------------------------------------- */
#define BLUEST_MFMC_MAX_NEIGHBOURS 30
#define BLUEST_MFMC_MAX_ROUND      24   /* 'Too many dimensions to brute-force it' above this clique size */
#define BLUEST_MFMC_MAX_OUTPUTS    64
#define BLUEST_MFMC_BUDGET         1    /* flags */
#define BLUEST_MFMC_CONTINUOUS     2
#define BLUEST_MFMC_SMALL_BUDGET   4
#define BLUEST_MFMC_OK             0    /* status */
#define BLUEST_MFMC_NONE           1    /* no clique admits an MFMC estimator */
#define BLUEST_MFMC_TOO_BIG        2    /* a feasible clique has more than BLUEST_MFMC_MAX_ROUND models to round */
int bluest_mfmc_search(int nb, int n_out, int flags, double budget, const double *eps2, const double *epsm2, const double *w,
                       const double *s, const double *rho, const int32_t *perm, const uint32_t *adj, uint32_t *best_mask,
                       uint32_t *best_combo, double *best_obj, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Part 8 -- projection of the covariances onto the SPD matrices (bluest/blue_models.py:348-433, SPG of bluest/spg.py:39-132)
 * Host arrays, n_out outputs of M x M row-major float64: C (NaN allowed where mask is 0), mask (1 = entry known, 0 = not
 * coupled).  A mask entry may be any finite weight m, of either sign; two thresholds apply to it, as in the reference:
 *   |m| < 1e-14   the entry is unknown: C is read as 0 there (NaN and Inf allowed), and one such entry selects SPG;
 *   m^2 < 1e-15   the entry weighs nothing in f and in the gradient (m = 1e-8 is known AND weighs nothing).
 * Per output, one workgroup of ONE launch:
 *   - every mask entry nonzero: X = V max(l, spd_threshold) V^T with (l, V) = eigh of the lower triangle of C, f = ||C - X||_F,
 *     gpmax = it = count = 0 (the reference's single clip);
 *   - otherwise SPG on f(X) = 1/2 ||mask^2 o (X - C)||^2 with proj(X) = the clip of (X + X^T)/2, started at proj(mask o C),
 *     stopping when max|proj(x - g) - x| <= eps, after maxit iterations or max_fevals evaluations; nonmonotone line search over
 *     the last hlength values, Barzilai-Borwein step clamped to [lmbda_min, lmbda_max].  X, f, gpmax, it, count as spg() returns
 *     them.
 * info: BLUEST_COVPROJ_* below (the reference's solver_info 0 / 1 / 2, then this build's own).  M outside 1..BLUEST_MAX_MODELS,
 * n_out outside 1..BLUEST_COVPROJ_MAX_OUTPUTS or hlength outside 1..BLUEST_COVPROJ_MAX_HISTORY return BLUEST_ERR_ARG.
 * Synchronous on `stream`; allocates and frees its own device memory.
 * --------------------------------------------------------------------------------------------------------- */
#define BLUEST_COVPROJ_OK          0   /* converged (SPG) / clipped (all entries known) */
#define BLUEST_COVPROJ_MAXIT       1   /* maxit iterations reached */
#define BLUEST_COVPROJ_MAXFEV      2   /* evaluation budget spent (X = the last accepted point) */
#define BLUEST_COVPROJ_NONFINITE   3   /* a known entry of C, or an entry of mask, is not finite: X = C, nothing computed */
#define BLUEST_COVPROJ_NOEIG       4   /* a Jacobi eigendecomposition did not converge in its sweep budget */
#define BLUEST_COVPROJ_MAX_OUTPUTS 1024
#define BLUEST_COVPROJ_MAX_HISTORY 64
int bluest_cov_project(int M, int n_out, const double *C, const double *mask, double spd_threshold, double eps, double lmbda_min,
                       double lmbda_max, int64_t maxit, int64_t max_fevals, int hlength, double *X_out, double *f_out,
                       double *gpmax_out, int64_t *it_out, int64_t *count_out, int32_t *info_out, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Part 9 -- MLMC model-subset search (bluest/blue_models.py:642-741; allocation misc.py:15-46, rounding misc.py:141-167,
 * 384-413).  Positions 0..nb are the models in decreasing cost order, model 0 at position 0 (the host orders them and drops
 * the models dearer than model 0).  Host arrays: w (nb+1) model costs by position; lv (n_out x (nb+1) x (nb+1)) level variances:
 * lv[n][p][q], p < q, the variance of the difference of the models at p and q (C[p,p] + (C[q,q] - 2 C[p,q]), or the user's
 * mlmc_variances entry where finite), lv[n][p][p] = C[p,p] the last level of a group ending at p, q < p unused; eps2 (n_out)
 * eps**2 (eps mode only); adj (nb+1) bit q set when positions p and q are coupled in the intersection of the coupling graphs.
 * A group is a bitmask over positions 1..nb (bit p-1 = position p kept): position 0, then the kept positions in increasing
 * order, admissible when every consecutive pair is coupled (a path, not a clique; mask 0 always is).  Its levels are
 * (g_i, g_i+1) with cost w[g_i] + w[g_i+1], and g_L-1 alone.  Searches all 2^nb masks and returns the reference's argmin of
 *   budget mode: the largest error over outputs;
 *   eps mode:    sum_i (max over outputs of the samples of level i) * w[g_i] -- the MODEL costs, not the level costs: the
 *                reference's choice (blue_models.py:718), kept;
 * ties going to the reference's enumeration order (mask 0, then by decreasing size, then the removed positions in lexicographic
 * order): best_mask, best_combo (n_out: the index of the floor/ceil combination the rounding chose, bit j = ub of the j-th
 * entry of get_feasible_integer_bounds; 0 in continuous mode), best_obj, status.  On BLUEST_MLMC_TOO_BIG only status is
 * written.  nb outside 0..BLUEST_MLMC_MAX_CANDIDATES, n_out outside 1..BLUEST_MLMC_MAX_OUTPUTS, a null pointer, or eps mode
 * without eps2 return BLUEST_ERR_ARG.  Synchronous on `stream`; allocates and frees its own device memory.
 * --------------------------------------------------------------------------------------------------------- */
#define BLUEST_MLMC_MAX_CANDIDATES 30   /* models below model 0 in cost order */
#define BLUEST_MLMC_MAX_ROUND      24   /* 'Too many dimensions to brute-force it' above this group size */
#define BLUEST_MLMC_MAX_OUTPUTS    64
#define BLUEST_MLMC_BUDGET         1    /* flags */
#define BLUEST_MLMC_CONTINUOUS     2
#define BLUEST_MLMC_OK             0    /* status */
#define BLUEST_MLMC_NONE           1    /* no group admits an MLMC estimator */
#define BLUEST_MLMC_TOO_BIG        2    /* an admissible group with finite level variances has more than BLUEST_MLMC_MAX_ROUND models */
int bluest_mlmc_search(int nb, int n_out, int flags, double budget, const double *eps2, const double *w, const double *lv,
                       const uint32_t *adj, uint32_t *best_mask, uint32_t *best_combo, double *best_obj, int32_t *status,
                       void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Part 10 -- sums over pilot samples for the covariance / MLMC-variance estimates (bluest/blue_models.py:326-346; what
 * bluest/blue_fn.py:147-167 accumulates with compute_mlmc_differences=True, for scalar outputs and the default inner product
 * a * b).  values "hd" (host or device pointer, detected with hipPointerGetAttributes): n_out x N x L row-major float64,
 * values[n][s][i] = output n of model i on joint sample s.  Host outputs, float64:
 *   sumse  (n_out x L)       sum_s y_i
 *   sumsc  (n_out x L x L)   sum_s y_i y_j, full and symmetric
 *   sumsd1 (n_out x L x L)   i < j: sum_s (y_i - y_j), every other entry 0
 *   sumsd2 (n_out x L x L)   i < j: sum_s (y_i - y_j)^2 from the explicit differences (C_ii + C_jj - 2 C_ij of two nearly equal
 *                            models has no correct digit left), every other entry 0
 * sumsd1 and sumsd2 may BOTH be null: no difference sums.  Two launches.  Stage 1, grid (chunk, output): a workgroup stages
 * BLUEST_PILOT_CHUNK consecutive samples in LDS, every thread owns a fixed set of pairs i <= j and walks the chunk's samples
 * in ascending order, accumulating in f64 registers; the partial sums go to [output][chunk][pair].  Stage 2 adds the chunks
 * in ascending order per (output, pair), writes the outputs and mirrors sumsc.  No atomics, and nothing depends on the number of
 * compute units: THE RESULT IS A FUNCTION OF `values` AND OF BLUEST_PILOT_CHUNK ONLY, bit-identical from run to run and
 * from machine to machine.  NaN / Inf in `values` propagate.  L outside 1..BLUEST_MAX_MODELS, n_out outside
 * 1..BLUEST_PILOT_MAX_OUTPUTS, N < 1 (or more than 2^31 - 1 chunks), a null pointer, or exactly one of sumsd1 / sumsd2 null
 * return BLUEST_ERR_ARG.  Synchronous on `stream`; allocates and frees its own device memory.
 * --------------------------------------------------------------------------------------------------------- */
#define BLUEST_PILOT_CHUNK         128   /* samples per workgroup: 64 KB of LDS at L = 64 */
#define BLUEST_PILOT_MAX_OUTPUTS   1024
int bluest_pilot_stats(int64_t N, int L, int n_out, const double *values, double *sumse, double *sumsc, double *sumsd1,
                       double *sumsd2, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Part 11 -- column sums over many ragged segments in one call, and the BLUE estimators they imply (what bluest/blue_fn.py:159-167
 * accumulates per sample, bluest/blue_models.py:555-571 per group and :963-968 per estimator of a variance test).
 * A SEGMENT is one (repeat, model group): counts[s] joint samples of sizes[s] models, laid out like Part 10's values,
 * values[s][n][i][j] = output n of the group's model j on sample i (n_out x counts[s] x sizes[s], row-major float64, 8-byte
 * aligned).  Each values[s] is a host OR a device pointer, detected per segment; it may be null where counts[s] == 0.  Every
 * other argument is host memory.  Host segments are copied into one device buffer in slabs of whole chunks (the slab size is
 * set with bluest_group_sums_slab); device segments are read in place.
 *   sums (n_out x T, T = sum of sizes)  sums[n][c0(s) + j] = sum_i values[s][n][i][j], c0(s) = sizes[0] + .. + sizes[s-1]
 *   mu   (R x n_out), with weights (n_out x T) and repeat_of ([S], non-decreasing, 0..R-1):
 *        mu[r][n] = sum over the segments s of repeat r and their columns j of weights[n][c0(s) + j] * sums[n][c0(s) + j];
 *        a repeat without segments gives 0.  weights and mu are both given or both null; R and repeat_of are read only with them.
 * THE ORDER OF EVERY SUMMATION IS FIXED.  Per segment, output and column:
 *   1. the samples are cut into chunks of BLUEST_GSUM_CHUNK = 128 consecutive samples (the last one may be shorter);
 *   2. inside a chunk, class k = 0..7 holds the samples 16 k .. 16 k + 15 of the chunk; q_k = the class's values added one by
 *      one in ascending sample order, starting from +0.0 (an empty class stays +0.0); the chunk's sum is
 *      ((q_0 + q_1) + (q_2 + q_3)) + ((q_4 + q_5) + (q_6 + q_7));
 *   3. lane l = 0..63 adds the sums of the chunks l, l + 64, l + 128, ... in ascending order, starting from +0.0; then for
 *      off = 32, 16, 8, 4, 2, 1 in that order, lane l < off takes p_l = p_l + p_(l + off); the segment's sum is p_0.
 *   mu[r][n] starts from +0.0 and takes m = fma(weights[n][c], sums[n][c], m) over the columns c of repeat r in ascending order
 *   (ascending segment, then ascending column of the segment).
 * So sums of segment s is a function of that segment's values and of BLUEST_GSUM_CHUNK only: not of the device, of the other
 * segments of the call, of the segment's position, of host or device memory, of the alignment of its base, or of where a slab
 * ends.  No atomics, nothing sized by the number of compute units.  A segment with counts[s] == 0 gives +0.0.  NaN / Inf propagate.
 * BLUEST_ERR_ARG: a null counts / sizes / values / sums, a null or misaligned values[s] with counts[s] > 0, S < 1, a size
 * outside 1..BLUEST_MAX_MODELS, n_out outside 1..BLUEST_GSUM_MAX_OUTPUTS, a negative count, exactly one of weights / mu, with
 * weights R < 1, a null, decreasing or out-of-range repeat_of, or more than 2^31 - 1 columns or chunks.  Synchronous on `stream`;
 * allocates and frees its own device memory.
 * bluest_group_sums_slab(bytes, previous): the staging budget for host segments of the calls that follow (process-wide; default
 * BLUEST_GSUM_SLAB_BYTES; at least one chunk is always staged); bytes == 0 only reads it; `previous` may be null.
 * --------------------------------------------------------------------------------------------------------- */
#define BLUEST_GSUM_CHUNK          128
#define BLUEST_GSUM_MAX_OUTPUTS    1024
#define BLUEST_GSUM_SLAB_BYTES     (256LL << 20)
int bluest_group_sums(int64_t S, int n_out, const int64_t *counts, const int32_t *sizes, const double *const *values,
                      const double *weights, int R, const int64_t *repeat_of, double *sums, double *mu, void *stream);
int bluest_group_sums_slab(int64_t bytes, int64_t *previous);

/* ---------------------------------------------------------------------------------------------------------
 * Part 12 -- Parts 10 and 11 for ONE output that is a vector of d components ("field") with a diagonal inner product
 * <a, b> = sum_c w_c a_c b_c (what bluest/blue_fn.py:147-167 accumulates with the Python inner products of
 * get_models_inner_products).  One output per call: outputs may differ in d.
 *
 * bluest_field_stats.  values "hd" (host or device, detected as in Part 10): N x L x d row-major float64, values[s][i][c] =
 * component c of model i on joint sample s.  w: host, d weights, finite and >= 0.  Host outputs, float64:
 *   sumse  (L x d)   sum_s y_i[c]
 *   sumsc  (L x L)   sum_s sum_c w_c y_i[c] y_j[c], full and symmetric
 *   sumsd1 (P x d)   P = L (L - 1) / 2, the pairs i < j in row-major order: sum_s (y_i[c] - y_j[c]) from the explicit differences
 *   sumsd2 (L x L)   i < j: sum_s sum_c w_c (y_i[c] - y_j[c])^2 from the explicit differences, every other entry 0
 * sumsd1 and sumsd2 may BOTH be null: no difference sums (sumse and sumsc keep their bits).
 * THE ORDER OF EVERY SUMMATION IS FIXED.  The samples are cut into chunks of BLUEST_PILOT_CHUNK consecutive samples, the
 * components into tiles of BLUEST_FIELD_TILE = 8 consecutive components (the last of either may be shorter).
 *   sumse, sumsd1: per (model or pair, component) and chunk, e = e + y_i[c] resp. r = r + (y_i[c] - y_j[c]) over the chunk's
 *     samples in ascending order from +0.0; the chunks' values are added in ascending order from +0.0.
 *   sumsc, sumsd2: per pair i <= j, chunk and tile, over the chunk's samples s in ascending order and inside a sample over the
 *     tile's components c in ascending order, from +0.0:  p = fma(w_c * a, b, p);  dd = a - b;  q = fma(w_c * dd, dd, q)
 *     with a = y_i[c], b = y_j[c] (w_c * a and w_c * dd rounded to float64).  Per pair and chunk the tiles are joined as the
 *     chunks of Part 11, step 3: lane l = 0..63 adds the values of the tiles l, l + 64, ... in ascending order from +0.0, then
 *     for off = 32, 16, 8, 4, 2, 1 lane l < off takes p_l = p_l + p_(l + off); the chunk's value is p_0.  The chunks' values are
 *     added in ascending order from +0.0.
 * With d = 1 and w = {1.0} these are the bits of bluest_pilot_stats (n_out = 1).  How many tiles a workgroup takes side by side
 * (a power of two that follows L and d) and how many samples it stages in LDS at a time shape the launch, not the order.  No
 * atomics, nothing sized by the number of compute units: the result is a function of `values`, `w`, BLUEST_PILOT_CHUNK and
 * BLUEST_FIELD_TILE only, the same bits from host or device memory and wherever a slab of staged host data ends.  NaN / Inf in
 * `values` propagate.  BLUEST_ERR_ARG: L outside 1..BLUEST_MAX_MODELS, d < 1, N < 1, a null values / w / sumse / sumsc,
 * exactly one of sumsd1 / sumsd2 null, a weight that is not finite or negative, or more than 2^31 - 1 (pair, component) sums
 * (L (L + 1) / 2 * d) or (chunk, block of tiles) workgroups.  Host input is staged in slabs of whole chunks under the budget of
 * bluest_group_sums_slab (at least one chunk).  Synchronous on `stream`; allocates and frees its own device memory.
 *
 * bluest_field_sums: Part 11 for a field.  Segment s is counts[s] x sizes[s] x d row-major float64 (8-byte aligned), a host OR
 * a device pointer per segment; it may be null where counts[s] == 0.  Every other argument is host memory.
 *   sums (T x d, T = sum of sizes)  sums[c0(s) + j][c] = sum_i values[s][i][j][c]
 *   mu   (R x d), with weights ([T]: the BLUE weight of a (group, model) column is a scalar also for a field, only the inner
 *        product enters the covariance) and repeat_of ([S], non-decreasing, 0..R-1): mu[r][c] starts from +0.0 and takes
 *        m = fma(weights[col], sums[col][c], m) over the columns of repeat r in ascending order; a repeat without segments
 *        gives +0.0.  weights and mu are both given or both null; R and repeat_of are read only with them.
 * Per (segment, column, component) the samples are added by steps 1-3 of Part 11: with d = 1 these are the bits of
 * bluest_group_sums (n_out = 1), and the sums of a segment do not depend on the other segments, on its position, on host or
 * device memory or on where a slab ends.  BLUEST_ERR_ARG as in Part 11 (d < 1 in place of n_out), and more than 2^31 - 1
 * column-components T d.  Staging budget: bluest_group_sums_slab.  Synchronous on `stream`; allocates and frees its own memory.
 * --------------------------------------------------------------------------------------------------------- */
#define BLUEST_FIELD_TILE          8
int bluest_field_stats(int64_t N, int L, int64_t d, const double *values, const double *w, double *sumse, double *sumsc,
                       double *sumsd1, double *sumsd2, void *stream);
int bluest_field_sums(int64_t S, int64_t d, const int64_t *counts, const int32_t *sizes, const double *const *values,
                      const double *weights, int R, const int64_t *repeat_of, double *sums, double *mu, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Part 13 -- first and second moments of many ragged segments in one call: what the sample covariance of every drawn model
 * group is made of.  Segments, counts, sizes, values[s] (host OR device per segment, 8-byte aligned, null allowed where
 * counts[s] == 0) and the staging budget (bluest_group_sums_slab) are exactly those of Part 11.  Host outputs, float64.
 * THE SHIFT.  Per (segment s, output n) every value enters as d_ij = values[s][n][i][j] - a_j with a_j = values[s][n][0][j], the
 * segment's first sample: one rounding.  The sums below keep their meaning when |mean| >> std, in one pass over the data.
 *   first  (n_out x T, T = sum of sizes)   first[n][c0(s) + j] = sum_i d_ij, c0(s) as in Part 11
 *   second (n_out x P, P = sum of sizes[s] (sizes[s] + 1) / 2): per segment the upper triangle j <= k, packed row-major (L = sizes[s]):
 *          second[n][p0(s) + j L - j (j - 1) / 2 + (k - j)] = sum_i d_ij d_ik, p0(s) = the triangle sizes of the segments before s.
 * The unbiased sample covariance of segment s is (second - first first^T / N) / (N - 1), N = counts[s]: the shift drops out.
 * THE ORDER OF EVERY OPERATION IS FIXED.
 *   first:  steps 1-3 of Part 11 applied to d.
 *   second: the same three steps per pair j <= k; inside a class of step 2 the accumulation is q = fma(d_ij, d_ik, q) over the
 *           class's samples in ascending order from +0.0 (one rounding per term); the classes join as
 *           ((q_0 + q_1) + (q_2 + q_3)) + ((q_4 + q_5) + (q_6 + q_7)); the chunks fold as in step 3.
 * So the results of segment s are a function of that segment's values and of BLUEST_GSUM_CHUNK only: not of the device, of the
 * other segments of the call, of the segment's position, of host or device memory, of the alignment of its base, or of where a
 * slab ends (the first samples of the host segments travel apart from the slabs).  No atomics, nothing sized by the number of
 * compute units, no matrix instructions.  counts[s] == 0 and counts[s] == 1 give +0.0 everywhere (for one sample d is exactly
 * 0).  NaN / Inf propagate (Inf - Inf is NaN).  BLUEST_ERR_ARG as in Part 11 (without the weights), and for a null first or
 * second, and for more than 2^31 - 1 packed pairs P.  Without a device BLUEST_ERR_NOGPU: there is no CPU path.  Synchronous on
 * `stream`; allocates and frees its own device memory.
 * --------------------------------------------------------------------------------------------------------- */
int bluest_group_moments(int64_t S, int n_out, const int64_t *counts, const int32_t *sizes, const double *const *values,
                         double *first, double *second, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Part 14 -- sums over pilot samples up to the fourth order: what the standard errors of Part 10's covariance and
 * MLMC-variance estimates are made of (the reference has no counterpart: its pilot size is a guess nothing checks).
 * values: exactly Part 10's array, "hd" (host or device, detected as there), n_out x N x L row-major float64.
 * THE SHIFT.  shift: a HOST array n_out x L, or null = the first sample, a_i = values[n][0][i].  Every value enters as
 * d_i = y_i - a_i (one rounding), so the sums keep their meaning when |mean| >> std; an explicit shift lets a host array go
 * in slabs that share the shift of the first.  Host outputs, float64:
 *   first (n_out x L)           sum_s d_i
 *   s11   (n_out x L x L)       sum_s d_i d_j, full and symmetric
 *   s21   (n_out x L x L)       s21[i][j] = sum_s d_i^2 d_j, full and NOT symmetric; the diagonal holds sum_s d_i^3
 *   s22   (n_out x L x L)       sum_s d_i^2 d_j^2, full and symmetric; the diagonal holds sum_s d_i^4
 *   tpow  (n_out x 4 x L x L)   may be null.  Slot k - 1 (k = 1..4) holds sum_s t^k at i < j, every other entry +0.0, with
 *                               t = (y_i - y_j) - (a_i - a_j): each inner subtraction rounded once, then the outer one.  t comes
 *                               from the explicit differences for the reason Part 10 gives.  With tpow null the other outputs
 *                               keep their bits.
 * THE ORDER OF EVERY OPERATION IS FIXED.  The samples are cut into chunks of BLUEST_PILOT_CHUNK consecutive samples (the last
 * may be shorter).  Inside a chunk the samples go in ascending order, every sum starting from +0.0:
 *   first: e = e + d_i.
 *   per pair lo <= hi, with a = d_lo, b = d_hi and p = a * b rounded to float64:
 *     S11 = fma(a, b, S11);  S21[lo][hi] = fma(a, p, S21[lo][hi]);  S21[hi][lo] = fma(b, p, S21[hi][lo]);  S22 = fma(p, p, S22);
 *     on the diagonal the two S21 updates are the same value, written once.
 *   per pair lo < hi, with t as above and q = t * t rounded to float64:
 *     T1 = T1 + t;  T2 = fma(t, t, T2);  T3 = fma(q, t, T3);  T4 = fma(q, q, T4).
 * The chunks' values are then added in ascending order from +0.0.  So the result is a function of `values`, `shift` and
 * BLUEST_PILOT_CHUNK only: the same bits from host or device memory, from run to run and from machine to machine, for one
 * output alone or inside a batch.  No atomics, nothing sized by the number of compute units, no matrix instructions.  N == 1
 * with a null shift gives +0.0 everywhere.  NaN / Inf propagate.  Two launches as in Part 10 (partial sums per (chunk, output),
 * then the fold over the chunks).  The staged chunk fills the default 64 KB of LDS at L = 64, so the shift never lives there:
 * without tpow it is subtracted while the chunk is staged; with tpow the chunk is staged as it lies (t needs the values
 * themselves), a thread holds a_lo and a_hi of its pairs in registers, and all eight sums come from the same two LDS reads.
 * BLUEST_ERR_ARG, returned before anything is written: L outside 1..BLUEST_MAX_MODELS, n_out outside
 * 1..BLUEST_PILOT_MAX_OUTPUTS, N < 1, more than 2^31 - 1 chunks, or a null values / first / s11 / s21 / s22.  Without a device
 * BLUEST_ERR_NOGPU: there is no CPU path.  Synchronous on `stream`; allocates and frees its own device memory.
 * --------------------------------------------------------------------------------------------------------- */
int bluest_pilot_moments4(int64_t N, int L, int n_out, const double *values, const double *shift, double *first, double *s11,
                          double *s21, double *s22, double *tpow, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Part 15 -- sums and sums of squares of a weighted combination of a field's models, per component, over many ragged segments
 * in one call: what the sampled variance of every component of a BLUE field estimate is made of (the reference has no
 * counterpart).  Segments, counts, sizes, values[s] (counts[s] x sizes[s] x d row-major float64, a host OR a device pointer per
 * segment, 8-byte aligned, null allowed where counts[s] == 0) and the staging budget (bluest_group_sums_slab) are exactly those of
 * bluest_field_sums.  coef: host, T = sum of sizes entries, one finite scalar per column (the BLUE weight of a (group, model)
 * column is a scalar also for a field); 0 is allowed.  Host outputs, float64, both S x d.
 * THE SHIFT.  Every value enters as d_ij[c] = values[s][i][j][c] - values[s][0][j][c], the segment's first sample subtracted: one
 * rounding, as in Part 13.  A mean far above the standard deviation costs no digit, in one pass over the data.
 *   z_i[c]      the combination of sample i: starts from +0.0 and takes z = fma(coef[c0(s) + j], d_ij[c], z) over the columns
 *               j = 0 .. sizes[s] - 1 of the segment in ascending order, c0(s) as in Part 11
 *   zsum[s][c] = sum_i z_i[c]
 *   zsq[s][c]  = sum_i z_i[c]^2
 * The unbiased variance of z over segment s is (zsq - zsum^2 / N) / (N - 1), N = counts[s]: the shift drops out.
 * THE ORDER OF EVERY OPERATION IS FIXED.  Per (segment, component) the samples are added by steps 1-3 of Part 11: chunks of
 * BLUEST_GSUM_CHUNK consecutive samples; inside a chunk eight classes of sixteen consecutive samples, each from +0.0 in ascending
 * order with q = q + z for zsum and q = fma(z, z, q) for zsq (one rounding per term); the classes join as
 * ((q_0 + q_1) + (q_2 + q_3)) + ((q_4 + q_5) + (q_6 + q_7)); lane l = 0..63 adds the chunks l, l + 64, ... in ascending order from
 * +0.0, and for off = 32, 16, 8, 4, 2, 1 lane l < off takes p_l = p_l + p_(l + off); the result is p_0.
 * So the results of segment s are a function of that segment's values, of its coefficients and of BLUEST_GSUM_CHUNK only: not of
 * the device, of the other segments of the call, of the segment's position, of host or device memory, of the alignment of its
 * base, of where a slab ends (the first samples of the host segments travel apart from the slabs), or of the launch shape (which
 * follows sizes[s] and d: a thread per component reading memory along c where d >= 64, sub-blocks of samples staged in LDS
 * below).  No atomics, nothing sized by the number of compute units, no matrix instructions.
 * TWO ANCHORS.  For a segment with sizes[s] == 1 and coef == 1.0, z = d, so for d <= BLUEST_MAX_MODELS zsum[s] is bit for bit
 * `first` of bluest_group_moments on the same counts[s] x d values read as [n_out = 1, N = counts[s], L = d], and zsq[s] is bit
 * for bit the diagonal of its `second`.
 * counts[s] == 0 and counts[s] == 1 give +0.0 everywhere (for one sample d is exactly 0).  NaN / Inf propagate (Inf - Inf is
 * NaN).  BLUEST_ERR_ARG, returned before anything is written: the cases of bluest_field_sums (S < 1, d < 1, a null counts / sizes
 * / values, a size outside 1..BLUEST_MAX_MODELS, a negative count, a null or misaligned values[s] with counts[s] > 0, more than
 * 2^31 - 1 columns, chunks or column-components T d), a null coef, zsum or zsq, a coefficient that is not finite, more than
 * 2^31 - 1 values S d, or more than 2^31 - 1 (chunk, block of 64 components, class) workgroups.  Without a device BLUEST_ERR_NOGPU:
 * there is no CPU path.  Synchronous on `stream`; allocates and frees its own device memory.
 * --------------------------------------------------------------------------------------------------------- */
int bluest_field_weighted_moments(int64_t S, int64_t d, const int64_t *counts, const int32_t *sizes, const double *const *values,
                                  const double *coef, double *zsum, double *zsq, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Part 16 -- second moments of a field's models in the inner product <a, b> = sum_c w_c a_c b_c, over many ragged segments in
 * one call: Part 13 for a field, what the unbiased covariance of every drawn model group of a field output is made of (the
 * reference has no counterpart).  Segments, counts, sizes, values[s] (counts[s] x sizes[s] x d row-major float64, a host OR a
 * device pointer per segment, 8-byte aligned, null allowed where counts[s] == 0) and the staging budget
 * (bluest_group_sums_slab) are exactly those of bluest_field_sums and Part 15.  w: host, d weights, finite and >= 0, as in Part
 * 12.  Host outputs, float64.
 * THE SHIFT.  Every value enters as d_ij[c] = values[s][i][j][c] - values[s][0][j][c], the segment's first sample subtracted: one
 * rounding, as in Parts 13 and 15.
 *   second (P = sum of sizes[s] (sizes[s] + 1) / 2, packed per segment as in Part 13):  pair j <= k:  sum_i sum_c w_c d_ij[c] d_ik[c]
 *   cross  (P, the same packing):                      pair j <= k:  sum_c w_c f_j[c] f_k[c]  with  f_j[c] = sum_i d_ij[c]
 *   first  (T x d, T = sum of sizes; MAY BE NULL):     first[c0(s) + j][c] = f_j[c], c0(s) as in Part 11.  With first null,
 *          second and cross keep their bits: f is formed on the device either way, and only its copy to the host is left out.
 * The unbiased covariance of segment s in the inner product is (second - cross / N) / (N - 1), N = counts[s]: the shift drops
 * out.  cross is formed on the device because the copy of T d per-component sums to the host is most of a field_sums call;
 * here L (L + 1) doubles per segment travel, and T d only where the caller asks for first.
 * THE ORDER OF EVERY OPERATION IS FIXED.
 *   f:      per (segment, column, component) steps 1-3 of Part 11 applied to d.
 *   second: per pair j <= k.  The samples are cut into chunks of BLUEST_GSUM_CHUNK, the components into tiles of
 *           BLUEST_FIELD_TILE = 8 (the last may be shorter).  Per (chunk, tile) and class k = 0..7 of sixteen samples, q_k starts
 *           from +0.0 and takes q = fma(w_c * a, b, q) with a = d_ij[c], b = d_ik[c] and w_c * a rounded to float64, over the
 *           class's samples in ascending order and inside a sample over the tile's components in ascending order.  The classes
 *           join as ((q_0 + q_1) + (q_2 + q_3)) + ((q_4 + q_5) + (q_6 + q_7)) (a class without samples is +0.0).  Per chunk the
 *           tiles join as in Part 12: lane l = 0..63 adds the tiles l, l + 64, ... in ascending order from +0.0, then for off =
 *           32, 16, 8, 4, 2, 1 lane l < off takes p_l = p_l + p_(l + off); the chunk's value is p_0.  The chunks fold as in step
 *           3 of Part 11.
 *   cross:  per pair j <= k and tile, x = fma(w_c * f_j[c], f_k[c], x) over the tile's components in ascending order from +0.0
 *           (w_c * f_j[c] rounded to float64); the tiles join by the same lane sums and tree.
 * ANCHORS.
 *   - With d == 1 and w == {1.0}, second and first are bit for bit those of bluest_group_moments (n_out = 1) on the same
 *     values: there is one tile of one component, 1.0 * a is a, so q_k is Part 13's class sum; the tile join adds it to +0.0
 *     (a sum that starts from +0.0 is never -0.0) and the other lanes hold +0.0, so the chunk's value is the class tree's.
 *   - With sizes[s] == 1 and w one-hot at component c, second[s] is bit for bit zsq[s][c] of Part 15 with coefficient 1.0:
 *     there z = fma(1.0, d, +0.0) = d (and -0.0 squares like +0.0), here the terms fma(+0.0 * a, b, q) of the other components
 *     leave q alone for finite values, the other tiles give +0.0, and the joins add +0.0.  For such a segment f is bit for bit
 *     zsum of Part 15 with coefficient 1.0, and at d == 1 it is bit for bit first of Part 13, for the same reason.
 *   - For identical j and k, cross is sum_c w_c f_j[c]^2 in the order above.
 * So the results of segment s are a function of that segment's values, of w, of BLUEST_GSUM_CHUNK and of BLUEST_FIELD_TILE only:
 * not of the device, of the other segments of the call, of the segment's position, of host or device memory, of the alignment of
 * its base, of where a slab ends (the first samples of the host segments travel apart from the slabs), or of the launch shape
 * (how many tiles a workgroup takes side by side and how many samples it stages in LDS at a time follow sizes[s] and d).  No
 * atomics, nothing sized by the number of compute units, no matrix instructions.  counts[s] == 0 and counts[s] == 1 give +0.0
 * everywhere.  NaN / Inf propagate (Inf - Inf is NaN).
 * BLUEST_ERR_ARG, returned before anything is written: the cases of bluest_field_sums (S < 1, d < 1, a null counts / sizes /
 * values, a size outside 1..BLUEST_MAX_MODELS, a negative count, a null or misaligned values[s] with counts[s] > 0, more than
 * 2^31 - 1 columns, chunks or column-components T d), a null w, second or cross, a weight that is not finite or is negative,
 * more than 2^31 - 1 packed pairs P, partial sums ((pair, chunk, tile) or (chunk, column, component)) or (chunk, block of
 * tiles) workgroups.  Without a device BLUEST_ERR_NOGPU: there is no CPU path.  Synchronous on `stream`; allocates one arena of
 * device memory and frees it.
 * --------------------------------------------------------------------------------------------------------- */
int bluest_field_group_moments(int64_t S, int64_t d, const int64_t *counts, const int32_t *sizes, const double *const *values,
                               const double *w, double *second, double *cross, double *first, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Part 17 -- what the standard errors of Part 12's pilot estimates are made of: per pair of models the sums, over the pilot
 * samples, of the PER-SAMPLE centred inner product and of its square (the reference has no counterpart).  One output per call.
 * values "hd" (host or device, detected as in Part 10; 8-byte aligned): N x L x d row-major float64 as in Part 12.  w: host, d
 * weights, finite and >= 0.  centre: host, L x d: the point the samples are centred at, for the standard errors the
 * per-component mean sumse / N of Part 12.  Host outputs, float64, L x L each:
 *   q_s(i, j) = sum_c w_c a b,   a = y_i[c] - centre_i[c], b = y_j[c] - centre_j[c]           (sample s, pair i <= j)
 *   r_s(i, j) = sum_c w_c t t,   t = (y_i[c] - y_j[c]) - (centre_i[c] - centre_j[c])           (from the explicit differences, i < j)
 *   qfirst = q_0,   qs1 = sum_s (q_s - q_0),   qs2 = sum_s (q_s - q_0)^2      full and symmetric: a pair i <= j is computed once
 *                                                                              and mirrored (fma(w a, b, .) is not symmetric)
 *   rfirst = r_0,   rs1 = sum_s (r_s - r_0),   rs2 = sum_s (r_s - r_0)^2      at i < j, every other entry 0
 * rfirst, rs1 and rs2 may ALL be null: no difference sums (the q outputs keep their bits).  The shift by the first sample keeps
 * the digits of qs2 - qs1^2 / N when the mean of q_s is far above its spread.  The standard error of the mean of q_s is
 * sqrt(max(qs2 - qs1^2 / N, 0) / (N (N - 1))): the first-order (delta-method) error of the covariance estimate mean_s q_s.
 * THE ORDER OF EVERY OPERATION IS FIXED.  The components are cut into strips of BLUEST_FIELD_STRIP = 512 consecutive components,
 * the samples into chunks of BLUEST_PILOT_CHUNK consecutive samples (the last of either may be shorter).
 *   per (sample, pair, strip), over the strip's components c in ascending order from +0.0:
 *       p = fma(w_c * a, b, p);   p' = fma(w_c * t, t, p')      (a, b, t as above, each difference and w_c * a, w_c * t rounded
 *                                                                 to float64; a thread walks the whole chain, nothing is joined)
 *   per (sample, pair): q_s = the strips' values added in ascending order from +0.0; r_s likewise.
 *   per (pair, chunk), over the chunk's samples in ascending order from +0.0:  u = q_s - q_0;  s1 = s1 + u;  s2 = fma(u, u, s2)
 *   per pair: the chunks' s1 and s2 added in ascending order from +0.0.
 * So the result is a function of `values`, `w`, `centre`, BLUEST_FIELD_STRIP and BLUEST_PILOT_CHUNK only: the same bits from host
 * or device memory, at any 8-byte alignment of the base, under any staging budget (bluest_group_sums_slab) and any scratch limit,
 * and whatever shape the launch takes -- how many samples a workgroup stages in LDS and how wide its column blocks are follow L
 * and d.  No atomics, nothing sized by the number of compute units.  With w one-hot at component c the results are those of the
 * d = 1 call on that component (fma(+0.0 * a, b, p) leaves p alone for finite values).  NaN / Inf propagate: a NaN in model i
 * reaches the pairs of model i and no other.  N == 1 gives +0.0 in the four sums.
 * The per-sample values pass through device scratch, (d / BLUEST_FIELD_STRIP rounded up, + 1 where that is above 1) x L (L + 1)
 * doubles per sample with the r outputs, half of it without.  The samples are processed in runs of whole chunks so that the
 * scratch stays under bluest_field_pilot_scratch's limit (at least one chunk) and, for host input, the staged values under the
 * budget of bluest_group_sums_slab; every run is read once.
 * bluest_field_pilot_scratch(bytes, previous): that limit for the calls that follow (process-wide; default
 * BLUEST_FIELD_PILOT_SCRATCH_BYTES); bytes == 0 only reads it; `previous` may be null.
 * BLUEST_ERR_ARG, returned before anything is launched: the cases of bluest_field_stats (L outside 1..BLUEST_MAX_MODELS, d < 1,
 * N < 1, a null values / w, a weight that is not finite or is negative), a null centre, qfirst, qs1 or qs2, some but not all of
 * rfirst / rs1 / rs2 null, values not 8-byte aligned, more than 2^31 - 1 values L d per sample or chunks.  Without a device
 * BLUEST_ERR_NOGPU.  Synchronous on `stream`; allocates one arena of device memory and frees it.
 * --------------------------------------------------------------------------------------------------------- */
#define BLUEST_FIELD_STRIP         512
#define BLUEST_FIELD_PILOT_SCRATCH_BYTES (256LL << 20)
int bluest_field_pilot_moments(int64_t N, int L, int64_t d, const double *values, const double *w, const double *centre,
                               double *qfirst, double *qs1, double *qs2, double *rfirst, double *rs1, double *rs2, void *stream);
int bluest_field_pilot_scratch(int64_t bytes, int64_t *previous);

/* ---------------------------------------------------------------------------------------------------------
 * Part 19 (it stands here, next to the parts whose bits it returns; Part 18 closes the header) -- a resumable accumulator for ONE
 * segment of one field output: the rows arrive over many calls, in pieces of any sizes, and are never all held.  finish returns
 *   sums (L x d)            the bits of bluest_field_sums on the concatenated rows as one segment of sizes = L;
 *   zsum, zsq (d each)      with coef (host, L finite scalars) given at creation: the bits of bluest_field_weighted_moments on
 *                           the same segment with the same coefficients.  Without coef both must be null, and the moment
 *                           kernels are never launched;
 *   count                   the number of rows taken.
 * update: values rows x L x d row-major float64, a host OR a device pointer per call (detected as in Part 10), 8-byte aligned;
 * rows may be 0.  Host outputs, float64.
 * THE STATE, on the device, owned by the handle, about 192 rows' worth of the segment whatever its length: the 64 lane partials
 * of step 3 of Part 11 per column-component ([64][L d]) and, with coef, per sum of Part 15 ([64][2 d]); the segment's first row
 * ([L d], Part 15's shift); the rows of the unfinished chunk (at most BLUEST_GSUM_CHUNK - 1 wait there between calls); and a
 * scratch for one update -- the per-chunk partials, the chunk tables, the staging buffer of a host batch -- that only grows, so
 * a steady run of equal batches does not allocate.
 * THE ORDER.  The rows of the segment are cut into the chunks of Part 11 whatever the pieces are: a chunk that straddles two
 * updates is completed inside the tail buffer and read from there, the whole chunks of a device batch are read where they lie,
 * those of a host batch pass through the staging buffer in slabs of whole chunks under the budget of bluest_group_sums_slab, and
 * the rows left over wait in the tail; finish takes them as the last, short chunk.  A chunk's value is formed by the kernels of
 * Parts 12 and 15 from its own rows (and the first row): steps 1 and 2.  The chunks of an update have the global numbers c0 ..
 * c0 + nc - 1; lane l takes its partial, adds the values of the chunks c = l (mod 64) among them in ascending c, and stores it.
 * finish runs the tree of step 3 (off = 32, 16, 8, 4, 2, 1) over the 64 lane partials.
 * WHY THE BITS ARE THOSE OF THE ONE-SHOT CALLS.  There, lane l starts from +0.0 and adds the values of the chunks l, l + 64, ...
 * in ascending order, then the tree runs.  Here the lane partial starts at +0.0 and continues the same additions of the same
 * values in the same order, call after call, and the same tree follows.  Nothing else enters: not the sizes of the pieces, not
 * host or device memory, not the alignment, not the staging budget.  No update at all gives count 0 and +0.0 everywhere; one row
 * gives +0.0 in zsum and zsq.  NaN / Inf propagate as in the one-shot calls.  No atomics, nothing sized by the number of
 * compute units.
 * Every call synchronises on `stream` before it returns: a batch may be freed right after update.
 * BLUEST_ERR_ARG, returned before anything changes: L outside 1..BLUEST_MAX_MODELS, d < 1, more than 2^31 - 1 column-components
 * L d, a coefficient that is not finite, a null handle or out-pointer, rows < 0, null or misaligned values with rows > 0,
 * exactly one of zsum / zsq, zsum given without coef or the reverse.  BLUEST_ERR_STATE: update or finish after finish.  Without a
 * device BLUEST_ERR_NOGPU: there is no CPU path.  destroy takes a null handle.
 * bluest_field_accum_info, for tests and tuning: info[0..7] = rows taken, chunks carried, rows waiting in the tail, device
 * allocations made so far, launches of the sum kernel, launches of a moment kernel, device bytes held, finished.
 * --------------------------------------------------------------------------------------------------------- */
typedef struct bluest_field_accum bluest_field_accum;
int bluest_field_accum_create(int L, int64_t d, const double *coef, bluest_field_accum **out, void *stream);
int bluest_field_accum_update(bluest_field_accum *a, int64_t rows, const double *values, void *stream);
int bluest_field_accum_finish(bluest_field_accum *a, int64_t *count, double *sums, double *zsum, double *zsq, void *stream);
int bluest_field_accum_info(const bluest_field_accum *a, int64_t *info);
int bluest_field_accum_destroy(bluest_field_accum *a);

/* ---------------------------------------------------------------------------------------------------------
 * Part 18 -- fields on per-model meshes: sparse maps B_l (q x d_l) that take the d_l components of model l into a space of q
 * components all models of an output share -- point evaluation, prolongation to the finest mesh, restriction to an observation
 * grid, evaluation at quadrature points.  After the map, Parts 12 and 15 to 17 apply as they are to the array [N, L, q].  (The
 * reference has no counterpart: its field example reduces every solution to two point values on the host.)
 * AN OPERATOR is given once as a host CSR matrix -- indptr (q + 1), indices and data (nnz = indptr[q] each) -- and is checked,
 * re-laid out for the device and uploaded by bluest_field_op_create; the handle owns its device memory until
 * bluest_field_op_destroy, and the caller's arrays are not kept.  bluest_field_op_shape reads q, d and nnz back (each pointer
 * may be null).  BLUEST_ERR_ARG from create, before anything is allocated: q < 1 or d < 1, q, d or nnz above 2^31 - 1, a null
 * indptr / op (or indices / data with nnz > 0), indptr[0] != 0, indptr decreasing, an index outside 0..d-1, a coefficient that
 * is not finite.  Without a device BLUEST_ERR_NOGPU.
 * THE CALL.  ops: L handles, or null = all identity; a null ENTRY is the identity and needs d_l == q.  values: L pointers,
 * values[l] N x d_l row-major float64, each a host OR a device pointer (detected as in Part 10), 8-byte aligned.  out: N x L x q
 * row-major float64, host or device, 8-byte aligned.
 *   out[s][l][r] = row r of ops[l] applied to sample s of values[l].
 * THE ORDER OF EVERY OPERATION IS FIXED.  The entries k = indptr[r] .. indptr[r + 1] - 1 of a row are taken in their STORED
 * order: they are neither sorted nor merged, and a column may occur twice.  They are cut into strips of BLUEST_FIELD_MAP_STRIP =
 * 512 consecutive entries (the last may be shorter).
 *   per strip, from +0.0, in ascending k:   p = fma(data[k], y[s][indices[k]], p)
 *   per row: the strips' values added in ascending order from +0.0.
 * A row of at most one strip is that one chain (a chain that starts from +0.0 never ends in -0.0, so adding it to +0.0 changes
 * no bit): every finite-element prolongation.  An empty row gives +0.0.  An identity entry copies the value's 64 bits, -0.0 and
 * the payload of a NaN included.
 * So the result is a function of the operator, of the values and of BLUEST_FIELD_MAP_STRIP only: the same bits from host or
 * device memory (the inputs mixed freely, the output on either side), at any 8-byte alignment, under any staging budget
 * (bluest_group_sums_slab), for a model alone or among 64, and whatever shape the launch takes -- rows of at most one strip run
 * with a lane per row over a sliced-ELL copy of the operator, longer rows with a lane per sample that walks the strips in order;
 * which of the two a row gets follows from its length only.  No atomics, nothing sized by the number of compute units, no
 * matrix instructions.
 * NaN / Inf propagate: a NaN at y[s][c] reaches exactly the rows that name column c, on that sample and in that model, whatever
 * their coefficient (0 * NaN is NaN; a row padded for the device layout never executes its padding).  A coefficient 0 on a
 * finite value leaves the chain as it is.
 * Host values and a host `out` pass through one arena of device memory in runs of whole samples under the budget of
 * bluest_group_sums_slab (at least one sample per run); an output element depends on one sample only, so a run's end never
 * shows.  Device values are read where they lie, a device `out` is written where it lies.
 * BLUEST_ERR_ARG, returned before anything is launched or allocated: L outside 1..BLUEST_MAX_MODELS, N < 0, q < 1, a null values,
 * a null values[l] or out with N > 0, an entry of ops that is not a live handle or whose q differs from the call's, values[l]
 * or out not 8-byte aligned.  N == 0 returns BLUEST_OK and writes nothing.  Without a device BLUEST_ERR_NOGPU: there is no CPU
 * path.  Synchronous on `stream`.
 * --------------------------------------------------------------------------------------------------------- */
typedef struct bluest_field_op *bluest_field_op_t;
#define BLUEST_FIELD_MAP_STRIP     512
int bluest_field_op_create(int64_t q, int64_t d, const int64_t *indptr, const int32_t *indices, const double *data,
                           bluest_field_op_t *op);
int bluest_field_op_shape(bluest_field_op_t op, int64_t *q, int64_t *d, int64_t *nnz);
int bluest_field_op_destroy(bluest_field_op_t op);
int bluest_field_map(int64_t N, int L, int64_t q, const bluest_field_op_t *ops, const double *const *values, double *out,
                     void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BLUEST_HIP_H */
