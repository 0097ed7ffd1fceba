/*
 * smc_hip.h -- C ABI of libsmchip.so: the MI355X (gfx950) particle-filter hot path.
 *
 * Drop-in boundary for charlesknipp/sequential_monte_carlo (reference @ v1).  The reference has
 * no FFI: its filters call Julia model methods per particle (src/particles.jl:97-98,123-124).
 * A GPU cannot call Julia closures, so the boundary is "enumerated model family + parameter
 * rows"; a Julia wrapper adds methods of the SAME generic functions for these model types and
 * `ccall`s the entry points below (INTEGRATION.md shows the stub).  Each entry point names the
 * reference function it replaces.
 *
 * Conventions: plain pointers and sizes only.  Host arrays are caller-owned and borrowed for
 * the duration of the call; device state is owned by the opaque handle.  Every function
 * returns 0 on success, a negative SMC_E* code otherwise; smc_last_error() returns a
 * thread-local message.  Never aborts.  Indices are 0-based int32 (the Julia wrapper adds 1).
 * Layouts: params [n_theta][n_raw] row-major; x [d][n_theta][n_x]; w, anc [n_theta][n_x].
 * A handle is used from one host thread at a time; different handles are independent.
 * (The threading contract as tested: DESIGN.md, "Host threads".)
 */
#ifndef SMC_HIP_H
#define SMC_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* model families (src/state_space_models.jl) */
#define SMC_MODEL_LG1D 1   /* UnivariateLinearGaussian :74-109  raw = (A,B,Q,R,x0,sigma0), Q R sigma0 variances */
#define SMC_MODEL_SV1D 2   /* stochastic volatility (SURVEY A7') raw = (mu,rho,sigma)                            */
#define SMC_MODEL_UCSV3D 3 /* UCSV :215-263                     raw = (gamma_eps,gamma_eta,x0,log_s_eps0,log_s_eta0) */
#define SMC_MODEL_UCSV_RB 4 /* UCSV with the trend integrated out (Rao-Blackwellised); the same raw row: "marginal UCSV" below */

#define SMC_OK 0
#define SMC_EINVAL (-1)
#define SMC_EHIP (-2)
#define SMC_ESTATE (-3)
#define SMC_ENOMEM (-4)

/* flags of smc_create */
#define SMC_FLAG_ANCESTORS 1u /* keep the ancestor vector `a` of the last step (particles.jl:117)      */
#define SMC_FLAG_NO_RESIDENT 2u /* never use the LDS-resident whole-series kernel (testing)            */
#define SMC_FLAG_SYSTEMATIC 4u /* OPT-IN: systematic resampling instead of the reference's multinomial
                                * resample (particles.jl:17-19 draws iid): one uniform per step, child j takes
                                * the point (j + u)/N of the weight CDF.  Same expectation N w_i of every
                                * particle's children, lower variance, a different law - never the default. */
#define SMC_FLAG_NAN_MISSING 8u /* OPT-IN: a NaN observation is a MISSING one ("missing observations" below): its step moves
                                 * the cloud by the transition and weighs nothing.  Without the flag a NaN kills its step. */
#define SMC_FLAG_CONDITIONAL 16u /* OPT-IN: the conditional particle filter ("the conditional particle filter" below): one slot of every
                                 * step is pinned to a reference trajectory.  Without the flag nothing changes. */
#define SMC_FLAG_ANCESTOR_SAMPLING 32u /* OPT-IN, with SMC_FLAG_CONDITIONAL only (else SMC_EINVAL): particle Gibbs with ancestor sampling
                                 * ("ancestor sampling" below).  Implies SMC_FLAG_ANCESTORS (smc_get_flags reports both); the record
                                 * keeps the ancestor vectors.  The steps are those of a handle with CONDITIONAL | ANCESTORS, bit for bit. */

typedef struct smc_filter_s* smc_handle;

/* ---- lifetime ------------------------------------------------------------------------------ */
/* n_theta independent bootstrap filters of n_x particles each (the batched callers
 * src/smc_samplers.jl:112-121,223-229,289-295,325-335 become ONE handle with n_theta > 1).
 * seg: particles per segment (power of two in [256,8192]); 0 = automatic (smc_auto_seg). It is part of the
 * random-number contract like the seed.  A filter has at most 16384 segments (n_x <= 2^27 with seg = 8192; the automatic
 * choice keeps segments of 2048 up to 2^25 particles).  Filter m uses Philox stream id m until smc_set_streams says otherwise. */
int smc_create(int model_id, int64_t n_theta, int64_t n_x, int seg, uint64_t seed, int device, uint32_t flags,
               smc_handle* out);
/* waits for the handle's stream, then releases it.  The device slab, the stream, the events and the pinned mirrors of up to 8
 * destroyed handles (512 MB of device memory at most) are kept for the next smc_create that fits them: creating and destroying
 * a handle per call costs 0.02 ms instead of 0.6 ms. */
int smc_destroy(smc_handle h);

/* smc.model(theta[m]) for every m (src/smc_samplers.jl:120,178,227,293,330): raw parameter rows.
 * NON-FINITE INPUTS.  Neither this call nor smc_init / smc_step / smc_step_window / smc_log_likelihood refuses a value: a row is
 * derived as it stands (sqrt(Q), 1 / sqrt(R), sigma / sqrt(1 - rho^2)) and any y is taken.  What follows is defined, the same on
 * the device and in the CPU oracle bit for bit (NaN positions included), and pinned by tests/test_gpu_nonfinite.py:
 *   - a particle whose log-weight is NaN, infinite or beyond 7e8 in magnitude takes no part in the normalisation.  A step that
 *     leaves no particle alive is DEAD: logmu = -inf, ess = 0, every weight 0, logZ = -inf from then on, weighted summaries NaN,
 *     and the next step's ancestors are the identity.  Nothing faults; the states may hold NaN or +-inf.
 *   - an observation that is NaN, +inf or -inf kills the step it arrives at, in every family.  The bootstrap families (LG1D,
 *     SV1D, UCSV3D) keep finite states through it and weigh again at the next finite observation (logZ stays -inf).  The guided
 *     filters (LG1D AFFINE - also with c2 = 0, since 0 * y is NaN - LG1D OPTIMAL, UCSV OPTIMAL) and SMC_MODEL_UCSV_RB carry y
 *     into the state (the proposal mean; the Kalman mean m): dead from that step on.  The first step of a guided filter is the
 *     bootstrap first step, so a bad y_1 costs a guided filter that step alone; SMC_MODEL_UCSV_RB is dead from it on.
 *     This holds on a handle WITHOUT SMC_FLAG_NAN_MISSING and is not a missing-data rule; with the flag a NaN is a gap
 *     ("missing observations" below; +-inf still kill the step).  (Looking past the END of the series is smc_forecast,
 *     "forecasts" below: it propagates the cloud without observations.)
 *   - a row outside its family's domain makes its filter dead: LG1D R <= 0 or a NaN B, SV1D |rho| >= 1 or a NaN sigma, UCSV a NaN
 *     x0, lse0 = +inf (and for the bootstrap filter lsn0 = -inf) from the first step; LG1D Q < 0, Q = +inf or a NaN A from the
 *     second (the first step does not move the particles).  LG1D sigma0 = 0 is valid (x_1 = x0).  A NEGATIVE UCSV gamma is a live
 *     filter: the sign only flips a normal.  lsn0 = -inf (observation noise 0) is a live SMC_MODEL_UCSV_RB filter, and under UCSV
 *     OPTIMAL dead at the first step alone.
 *   - the other filters of the batch are untouched bit for bit, and a later smc_set_params with valid rows leaves nothing of the
 *     dead filter behind on the handle.
 *   - the samplers never accept such a filter: the accept test of the PMMH move requires logZ' + log prior' > -inf
 *     (src/smc_samplers.jl:129), which a dead filter's logZ = -inf fails.  With a prior that puts mass outside a parameter's
 *     domain (PRIOR_NORMAL on a variance) such parameter particles enter with weight 0 and are resampled away.  The Python model
 *     constructors do refuse such parameters (ValueError); only rows built on the device from theta (ThetaMap) get this far.
 *   - smc_smooth and smc_sample_paths refuse a row whose transition scale is not a positive finite number (below); a filter that
 *     was dead at a recorded step reads NaN / -1 at every step. */
int smc_set_params(smc_handle h, const double* raw /*[n_theta][n_raw]*/);
/* Philox stream id per filter (e.g. the GLOBAL theta index when theta is sharded over GPUs). */
int smc_set_streams(smc_handle h, const uint32_t* stream /*[n_theta]*/);
int smc_reseed(smc_handle h, uint64_t seed);
/* Diagnostic.  *by_value = 1 when the step launches of the next smc_step / smc_log_likelihood take the filter's stream id, parameter
 * row and observation BY VALUE in the kernel arguments (one filter per handle, no skip mask, the host's copies of row 0 current:
 * set through smc_set_params / smc_set_streams and not since rewritten on the device by the PMMH kernels, smc_permute,
 * smc_copy_from, smc_unpack_slots or the exchange); 0 when they read them through device pointers.  Results never depend on it.
 * SMC_STEP_BY_VALUE=0 in the environment at smc_create: always 0. */
int smc_step_by_value(smc_handle h, int* by_value);
/* Diagnostic.  The workgroup geometry of the handle's launches (any pointer may be NULL).  *threads, *np: threads per workgroup and
 * particle pairs per thread of the one-launch-per-step kernels (init, step, forecast), seg = 2 * np * threads: the default of the
 * segment length, or what SMC_NP (1, 2 or 4) in the environment at smc_create selected; a value the segment length has no kernels
 * for leaves the default.  *resident_np: the pairs per thread the LDS-resident whole-series and window kernels would be asked for
 * if launched now - SMC_RES_NP (1, 2 or 4) as the environment holds it at THIS call (the launches read it at every call), else 1
 * for segments of 1024 with at most 512 filters, else 0 = the kernels' own choice for the segment length; a value without a kernel
 * at the segment length runs the neighbour its table documents.  Results never depend on either knob. */
int smc_get_launch_geometry(smc_handle h, int* threads, int* np, int* resident_np);

/* ---- proposals: the guided particle filter ----------------------------------------------------
 * particle_filter(N, y, model, proposal) / particle_filter!(x, w, y, model, proposal)          src/particles.jl:28-84
 * A handle has a proposal.  SMC_PROP_NONE (the default of a fresh or recycled handle) is the bootstrap filter.  With a proposal
 * every step after the first draws x from it instead of the transition and weights it as particles.jl:72-80 does,
 *     logw = logpdf(observation(x), y) + logpdf(transition(xp), x) - logpdf(proposal(xp, y), x),
 * with the normals of the bootstrap step (one per state coordinate, the same Philox slots).  Resampling, normalisation, logZ,
 * ESS, summaries, skip masks, windows, slot moves and PMMH are as without a proposal.
 *   SMC_PROP_AFFINE   LG1D only.  Row (c0, c1, c2, s2) per filter, s2 > 0 a variance:  m = c0 + c1 xp + c2 y,
 *                     x = m + sqrt(s2) z,  logw = logobs(x, y) + [logN(x; A xp, Q) - logN(x; m, s2)].
 *                     The row (0, A, 0, Q) IS the bootstrap filter, bit for bit (the bracket evaluates to +0.0).
 *   SMC_PROP_OPTIMAL  LG1D: the AFFINE row derived from the model row, with D = B B Q + R: (0, A R / D, B Q / D, Q R / D)
 *                     (smc_host_optimal_proposal; an AFFINE handle given exactly these doubles computes the same bits).
 *                     UCSV3D: the log-volatilities move by the transition; with Q = exp(xp[1]), R = exp(x[2]), K = Q / (Q + R):
 *                     x[0] = xp[0] + K (y - xp[0]) + sqrt(K R) z[0],  logw = logN(y; xp[0], Q + R)  (the closed form of the
 *                     three terms; it does not depend on x[0]).
 *   Every other pair (SV1D with a proposal, UCSV3D with AFFINE), an unknown kind, rows with AFFINE missing or given with another
 *   kind, a row that is not finite or has s2 <= 0: SMC_EINVAL, and the handle is unchanged.
 * Deviation from the reference, on purpose: the FIRST step is the bootstrap first step (draw from initial_dist, weight by the
 * observation density).  particle_filter adds logpdf(initial_dist, x) there (:41-44), a slip: its own commented line :43 shows
 * the intended correction, which is zero for a draw from initial_dist.
 * The call may be made between steps; it applies from the next smc_step, smc_step_window or smc_log_likelihood (a pending window
 * is dropped).  smc_set_params after SMC_PROP_OPTIMAL derives the proposal of the new rows; AFFINE rows stay as given.  Like
 * parameters and stream ids a proposal stays with its slot under smc_permute, smc_copy_from, smc_pack_slots / smc_unpack_slots
 * and smc_comm_exchange_slots: only the state travels.  smc_pmmh_rejuvenate on a handle with SMC_PROP_OPTIMAL derives the
 * proposal of every theta' on the device; AFFINE rows stay as set. */
#define SMC_PROP_NONE 0
#define SMC_PROP_AFFINE 1
#define SMC_PROP_OPTIMAL 2
#define SMC_PROP_NPAR 4
int smc_set_proposal(smc_handle h, int kind, const double* par /*[n_theta][SMC_PROP_NPAR], AFFINE only; else NULL*/);
int smc_host_optimal_proposal(int model_id, const double* raw, double* par /*[SMC_PROP_NPAR]*/);   /* LG1D */
/* one particle, one step, on the host: the specification's guided draw and log-weight (tests, Julia-side checks) */
int smc_host_guided_step(int model_id, const double* raw, int kind, const double* par, const double* xp /*[d]*/,
                         const double* z /*[d]*/, double y, double* x /*[d]*/, double* logw);
/* the same for n particles, xp z x [d][n], in a loop on the host: one call per step of a filter instead of one per particle */
int smc_host_guided_steps(int model_id, const double* raw, int kind, const double* par, const double* xp,
                          const double* z, double y, int64_t n, double* x, double* logw);
/* the same for n particles on the device, xp z x [d][n] (parity tests; the twin of smc_device_math) */
int smc_device_guided_step(int model_id, const double* raw, int kind, const double* par, const double* xp,
                           const double* z, double y, int64_t n, double* x, double* logw, int device);

/* ---- marginal UCSV: the Rao-Blackwellised filter ----------------------------------------------------
 * SMC_MODEL_UCSV_RB is a filter family for the UCSV model (src/state_space_models.jl:215-263): given the two log-volatility
 * paths (x, y) is linear-Gaussian, so a particle samples only the volatilities and carries the exact scalar Kalman filter of
 * the trend (src/kalman_filter.jl:29-53 with A = B = 1).  State rows (m, lse, lsn, P), smc_model_dim = 4: rows 1, 2 as UCSV3D,
 * row 0 the filtered mean of the trend, row 3 its filtered variance - always the posterior after the step's observation.
 * The parameter row is UCSV3D's (smc_model_nraw = 5), with the reference's conventions.  One step, the first included:
 *     P- = P + exp(lse_prev)                    (t = 1: m = x0, P- = exp(lse0), and the volatilities start from lse0, lsn0)
 *     lse = lse_prev + g_eps z0,  lsn = lsn_prev + g_eta z1
 *     R = exp(lsn),  S = P- + R,  e = y - m,    logw = -(log 2pi + log S + e e / S) / 2
 *     K = P- / S,  m' = m + K e,  P' = P- R / S (product form: 0 < P' <= min(P-, R))
 * logZ estimates the same p(y) as a UCSV3D filter, without bias; the trend adds no Monte-Carlo variance.  Two normals per particle
 * and step (Philox slots 1 and 2: lse, lsn).  Everything a handle offers applies (every launch path, ESS, summaries of all four
 * rows, skip masks, windows, slot moves, PMMH, exchange) except proposals: smc_set_proposal with a kind other than SMC_PROP_NONE
 * is SMC_EINVAL.  LDS-resident up to 2048 particles.  The observation moments are UCSV3D's with row 0 for the trend; the trend's
 * filtered variance is var(row 0) + mean(row 3).  smc_simulate with this id simulates UCSV3D (x [3][T]). */
/* one particle, one step, on the host: sp (m, lse, lsn, P) of the ancestor (not read when first != 0), z the two normals */
int smc_host_rb_step(const double* raw /*[5]*/, const double* sp /*[4]*/, const double* z /*[2]*/, double y, int first,
                     double* s /*[4]*/, double* logw);
/* the same for n particles, sp s [4][n], z [2][n], in a loop on the host */
int smc_host_rb_steps(const double* raw, const double* sp, const double* z, double y, int first, int64_t n, double* s,
                      double* logw);
/* the same for n particles on the device, sp s [4][n], z [2][n] (parity tests) */
int smc_device_rb_step(const double* raw, const double* sp, const double* z, double y, int first, int64_t n, double* s,
                       double* logw, int device);

/* ---- missing observations -------------------------------------------------------------------------
 * A handle created with SMC_FLAG_NAN_MISSING reads a NaN observation - in smc_init, smc_step, smc_step_window / smc_step_commit,
 * smc_log_likelihood and smc_pmmh_rejuvenate - as a period WITHOUT an observation.  The missing step is the ordinary step with
 * the observation's part left out: the same resampling from the current weights (either resampler, the same random numbers), the
 * same state normals, the time index advances by one; every particle moves by the TRANSITION (the initial distribution at the
 * first step; a guided handle too: a proposal has no role without y) and takes the log-weight +0.0, so logmu = +0.0, ess = n_x
 * and w = 1 / n_x exactly and the step adds nothing to logZ.  SMC_MODEL_UCSV_RB: the volatilities move as ever, row 0 (the mean
 * of the trend) stays, row 3 becomes P- = P + exp(lse_prev): after a gap rows 0 and 3 are the PREDICTIVE moments.  A filter that
 * is collapsed when it meets a gap leaves it with uniform weights; its logZ stays -inf (a running sum).  This is not the same
 * model as leaving the period out, which applies the transition once where the model applies it twice.  +-inf observations
 * still kill their step.  A flagged handle launches the same kernels as an unflagged one at every observed step, and for a
 * whole series or window without a NaN.  Per-step summaries, smc_forecast, the record of a step-by-step run, smc_smooth and
 * smc_sample_paths read clouds and weights and need no rule of their own (the smoothed state at a gap is the interpolation).
 * NOT covered: smc_rb_sample_paths (its Kalman / RTS pass along each path reads y: SMC_EINVAL on a flagged handle when y holds a
 * NaN) and smc_time_step_kernel (the same refusal).  The exact-Kalman entry points have the rule as well, opt-in in the same
 * way: "missing observations of the exact Kalman filter" below (smc_ibis_set_flags and the *_flags calls). */
/* the flags the handle was created with */
int smc_get_flags(smc_handle h, uint32_t* flags);
/* The whole step of n particles on the host, for every family and proposal: xp x [d][n], z [nz][n] (nz = d; 2 for
 * SMC_MODEL_UCSV_RB), logw [n].  kind / par as smc_host_guided_steps (SMC_PROP_NONE: the bootstrap step; SMC_MODEL_UCSV_RB takes
 * SMC_PROP_NONE only).  first != 0: the first step (xp is not read; a guided filter's first step is the bootstrap one).  With
 * nan_missing != 0 and a NaN y: the missing step (logw = +0.0). */
int smc_host_filter_steps(int model_id, const double* raw, int kind, const double* par, const double* xp, const double* z,
                          double y, int first, int nan_missing, int64_t n, double* x, double* logw);
/* the same on the device in one launch (parity tests; the twin of smc_device_guided_step) */
int smc_device_filter_steps(int model_id, const double* raw, int kind, const double* par, const double* xp, const double* z,
                            double y, int first, int nan_missing, int64_t n, double* x, double* logw, int device);
/* Device and pinned host bytes that the handles, communicators and bundles of this process hold right now (allocated and not yet
 * freed; process-wide, every device; the cache of destroyed handles' bundles included, the per-thread scratch of the calls
 * without a handle not).  A probe for tests: a leak shows as a difference that grows.  Either pointer may be NULL. */
int smc_live_bytes(int64_t* device_bytes, int64_t* pinned_bytes);

/* ---- the hot path ----------------------------------------------------------------------------*/
/* (all of these: a NaN observation on a handle with SMC_FLAG_NAN_MISSING is a missing step, "missing observations" above) */
/* bootstrap_filter(N, y, model) -> (x, w, logmu)            src/particles.jl:87-105 */
int smc_init(smc_handle h, double y1, double* logmu /*[n_theta]*/);
/* bootstrap_filter!(x, w, y, model) -> (logmu, w, ess)      src/particles.jl:107-129 */
int smc_step(smc_handle h, double y_t, double* logmu /*[n_theta]*/, double* ess /*[n_theta] or NULL*/);
/* k consecutive bootstrap_filter! calls (the loop `for t in 2:T smc²!(smc,y,t)` of the online sampler,
 * src/smc_samplers.jl:325-335, between two resample-move decisions) in ONE launch with the clouds resident in LDS:
 * returns (logmu, ess) of every step, [k][n_theta] each, but does NOT advance the filters - the caller looks at the
 * k outer ESS values and then keeps the first j steps with smc_step_commit(h, j) (j < k re-runs those j steps: the
 * random numbers are counter based, the bits are the same; j = 0 keeps nothing).  Bit-identical to k (or j) smc_step
 * calls.  Needs single-segment filters that fit the LDS-resident kernel (n_x <= 8192); k <= 64.
 * THE PENDING WINDOW.  Between a successful smc_step_window and the next smc_step_commit the window is pending: the (logmu, ess)
 * it reported describe steps from the filters as they stand, under the rows, seed, stream ids and proposal in force.  ONE rule:
 * a call that changes rows, seed, stream ids, proposal or the filters DROPS the window; a call that only reads, or that fails,
 * KEEPS it.  smc_step_commit without a pending window is SMC_ESTATE ("no window pending"), with j outside [0, k] SMC_EINVAL (the
 * window stays pending).  A second smc_step_window replaces the pending one.
 *   drop  smc_set_params, smc_set_streams, smc_reseed, smc_set_proposal, smc_init, smc_step, smc_log_likelihood, smc_permute,
 *         smc_copy_from (the destination; the source only reads), smc_unpack_slots, smc_comm_exchange_slots (it unpacks),
 *         smc_pmmh_rejuvenate (the proposal handle and main), smc_step_commit itself, smc_time_step_kernel (it runs a series).
 *   keep  smc_get_state, smc_get_weights_raw, smc_get_logZ, smc_get_moments, smc_get_quantiles, smc_get_predictive, smc_forecast,
 *         smc_forecast_cloud, smc_pack_slots, smc_slot_bytes, smc_get_geometry, smc_get_launch_geometry, smc_get_flags,
 *         smc_step_by_value, smc_last_elapsed_ms, smc_event_overhead_ms, smc_synchronize, smc_set_skip, smc_set_summaries,
 *         smc_get_summaries, smc_set_summary_mode, smc_pmmh_configure (they change what later calls compute, not the filters).
 *   n/a   the record and the smoothers (smc_history_*, smc_smooth*, smc_sample_paths, smc_rb_sample_paths, smc_predictive) and
 *         the conditional calls (smc_set_reference, smc_reference_from_paths, smc_get_reference, smc_ancestor_sweep): an armed or
 *         conditional handle refuses smc_step_window, so none of them meets a window opened on such a handle.  A window opened
 *         BEFORE smc_history_begin stays pending on the armed handle (smc_history_begin keeps it); smc_step_commit is refused
 *         (SMC_ESTATE) until smc_history_end, after which the window can still be committed, unless a recorded smc_init /
 *         smc_step has dropped it meanwhile.  smc_destroy ends a window with the handle.
 * REFUSED CALLS.  A call on a handle that returns SMC_EINVAL or SMC_ESTATE leaves the handle as it was: filters, logZ, time
 * index, a pending window and the host's by-value copies of row 0 (smc_step_by_value) included. */
int smc_step_window(smc_handle h, const double* y /*[k]*/, int k, double* logmu /*[k][n_theta]*/, double* ess /*[k][n_theta] or NULL*/);
int smc_step_commit(smc_handle h, int j);
/* log_likelihood(N, y, model) -> (x, w, logZ)               src/particles.jl:132-147
 * logmu_trace / ess_trace: [T][n_theta] or NULL. */
int smc_log_likelihood(smc_handle h, const double* y, int64_t T, double* logZ /*[n_theta]*/,
                       double* logmu_trace, double* ess_trace);
/* Per-step filtered summaries INSIDE the multi-step calls: what README.md:33-61 and examples/inflation_example.jl:39-55 compute
 * on the host after every bootstrap_filter! - quantile(x, weights(w), p), the weighted mean and variance - recorded at every
 * step of the following smc_log_likelihood / smc_step_window calls of the handle, on the device, without a host round trip per
 * observation (the README loop becomes ONE call).  component: state coordinate of the quantiles; p [np], np <= 8 (0: no
 * quantiles); moments != 0: mean and variance of every coordinate.  np = 0 and moments = 0 switch it off again.
 * Quantile definition: that of smc_get_quantiles (inverse of the weighted empirical CDF in the filter's integer weights).
 * Moments: those of smc_get_moments (NaN at a step after which every weight is 0).  Both in the handle's summary mode
 * (smc_set_summary_mode below): SMC_SUMM_UNWEIGHTED gives the README loop's own quantile(x, p) and var(x).
 * smc_get_summaries hands over the first T steps of the last such call: q [T][n_theta][np], mean / var [T][d][n_theta]
 * (NULL: not wanted).  Single-segment filters compute them inside the LDS-resident kernel; larger ones by trailing kernels
 * on the handle's stream after every step. */
int smc_set_summaries(smc_handle h, int component, const double* p /*[np]*/, int np, int moments);
int smc_get_summaries(smc_handle h, int64_t T, double* q /*[T][n_theta][np]*/, double* mean /*[T][d][n_theta]*/, double* var /*[T][d][n_theta]*/);
/* Summary modes.  SMC_SUMM_WEIGHTED (the default of a fresh or recycled handle): the definitions stated at smc_get_quantiles and
 * smc_get_moments.  SMC_SUMM_UNWEIGHTED: the statistics README.md:33-61 and examples/inflation_example.jl:165-171,241-252,341-348
 * compute on the cloud as bootstrap_filter! leaves it, Statistics.quantile(x, p) (unweighted, Hyndman-Fan type 7, interpolating;
 * numpy's default "linear" method) and Statistics.var(x) (unweighted, corrected):
 *   cloud      the n particles of state coordinate `component` of the current state (the x of smc_get_state), ALL of them, whatever
 *              their weights; padding slots beyond n never enter.  Order: the IEEE total order of the bits (-0.0 < +0.0).
 *   quantile   at level p (clamped to [0, 1]), in doubles and in exactly this order of operations:
 *                  h = n*p + (1 - p)
 *                  j = clamp(trunc(h), 1, n-1)          1-based rank
 *                  g = clamp(h - j, 0, 1)
 *                  a = x_(j),  b = x_(j+1)              n == 1: a = b = x_(1)
 *                  q = a + g*(b - a)                    a, b finite; otherwise (1-g)*a + g*b
 *              without a fused multiply-add: a pure function of the cloud, bit for bit.  The interpolation runs on the device.
 *   moments    mean = (1/n) sum x, var = sum (x - mean)^2 / (n - 1), centred second pass, sums in a fixed order; accuracy as stated
 *              at smc_get_moments with weights 1/n.  n == 1: var is NaN (as Julia).
 * A collapsed filter (every weight 0) has ordinary, finite unweighted summaries; a skipped filter keeps its NaN rows (smc_set_skip).
 * smc_set_summary_mode applies to the following smc_get_quantiles, smc_get_moments, and to the per-step summaries of
 * smc_log_likelihood / smc_step_window armed by smc_set_summaries; rows recorded before it are no longer handed out.  Unknown
 * mode: SMC_EINVAL, handle unchanged.
 * NOT offered: StatsBase's weighted INTERPOLATING quantile(x, weights(w), p) of get_quantiles_uc (examples/inflation_example.jl:45);
 * StatsBase is not vendored by the reference, so that variant cannot be pinned.  The weighted mode does not interpolate. */
#define SMC_SUMM_WEIGHTED 0
#define SMC_SUMM_UNWEIGHTED 1
int smc_set_summary_mode(smc_handle h, int mode);
/* the (x, w) the reference returns / mutates; any pointer may be NULL. w is the normalised
 * weight vector of normalize() (particles.jl:11); anc needs SMC_FLAG_ANCESTORS. */
int smc_get_state(smc_handle h, double* x /*[d][n_theta][n_x]*/, double* w /*[n_theta][n_x]*/,
                  int32_t* anc /*[n_theta][n_x]*/);
/* accumulated log-likelihood so far and ESS of the current weights */
int smc_get_logZ(smc_handle h, double* logZ /*[n_theta]*/, double* ess /*[n_theta] or NULL*/);
/* resample!(smc) of the OUTER sampler (src/smc_samplers.jl:74-84): filter slot m <- slot a[m]
 * (value copy of x cloud, weights and logZ; stream ids stay with the slot).  The indices are copied before the call returns;
 * the device work is enqueued on the handle's stream and NOT waited for (every later call on the handle is ordered behind it). */
int smc_permute(smc_handle h, const int32_t* a /*[n_theta]*/);
/* PMMH accept step of rejuvenate! (src/smc_samplers.jl:129-136): for every m with mask[m] != 0 the
 * filter state of slot m (x cloud, weights, logZ) is overwritten by slot m of `src` (the proposal
 * filters, same geometry).  Value copy on the device; streams and parameters are not copied.
 * A handle has ONE time index (the step number the next smc_step draws its random numbers under): after the call dst's is src's,
 * for every filter of dst and whatever the mask - callers copy between handles that have seen the same observations.  A packed
 * slot (smc_pack_slots) carries no time index: smc_unpack_slots leaves the receiver's as it is.
 * dst == src, handles that differ in model, geometry or device: SMC_EINVAL; either one without weights: SMC_ESTATE. */
int smc_copy_from(smc_handle dst, smc_handle src, const uint8_t* mask /*[n_theta]*/);

/* Proposals outside the prior's support: the reference never filters them (src/smc_samplers.jl:116).  Filters m with
 * skip[m] != 0 are left out by the following smc_log_likelihood calls; NULL runs every filter again.  What such a call
 * leaves for a skipped filter m, on every launch path:
 *   logZ[m] (returned and smc_get_logZ)         -inf;
 *   logmu_trace / ess_trace column m            NaN at every step;
 *   smc_get_summaries rows of m (q, mean, var)  NaN at every step;
 *   x, w, ancestors and raw weights of slot m   what they were before the call, bit for bit.
 * The mask applies to smc_log_likelihood only: the step API and smc_step_window run every filter. */
int smc_set_skip(smc_handle h, const uint8_t* skip /*[n_theta] or NULL*/);

/* ---- rejuvenate!(smc, y, xi) on the device: src/smc_samplers.jl:103-146 -------------------------
 * The handle `prop` holds the proposal filters of this rank's parameter particles (same geometry as the online
 * filters `main`, if any).  smc_pmmh_configure describes what a GPU cannot call as closures:
 *   prior  = product_distribution of d_theta enumerated components (smc.prior; README.md:81-85,
 *            examples/inflation_example.jl:33-37,234-239), par rows of SMC_PRIOR_NPAR doubles;
 *   model  = smc.model(theta): raw parameter row k is theta[raw_from[k]] (raw_from[k] >= 0) or raw_const[k].
 * smc_pmmh_rejuvenate then runs the whole `for c in 1:chain` loop (:113-137) for every parameter particle without
 * a host round trip: theta' ~ MvNormal(theta, scales[c] * L L') (:114; L = lower Cholesky factor of the random-walk
 * covariance :95-100, row-major [d][d]), insupport (:116), log_likelihood(N, y, model(theta')) with Philox seed
 * filter_seeds[c] for the in-support proposals only (:117-121), the accept test log(rand()) < xi (logZ' - logZ) +
 * logprior(theta') - logprior(theta) (:123-129), and theta / logZ / x / w of the accepted particles (:130-133;
 * x, w are copied into `main` when it is not NULL).  Proposal normals and accept uniforms are Philox draws keyed by
 * (move_seed, stream id of the filter = global theta index, chain position): independent of the sharding.
 * theta [n_theta][d_theta] and logZ [n_theta] are read and updated in place; accepted[m] = 1 if particle m moved at
 * least once (acc_array :135); *filters_run = number of proposal filters actually executed. */
#define SMC_PRIOR_UNIFORM 1     /* par = (lo, hi)                                                     */
#define SMC_PRIOR_NORMAL 2      /* par = (mu, sigma)                                                  */
#define SMC_PRIOR_TRUNCNORMAL 3 /* par = (mu, sigma, lo, hi, log(Phi((hi-mu)/sigma) - Phi((lo-mu)/sigma))) */
#define SMC_PRIOR_LOGNORMAL 4   /* par = (mu, sigma) of log x                                          */
#define SMC_PRIOR_NPAR 5
#define SMC_MAX_DTHETA 8
int smc_pmmh_configure(smc_handle prop, int d_theta, const int32_t* prior_family /*[d_theta]*/,
                       const double* prior_par /*[d_theta][SMC_PRIOR_NPAR]*/, const int32_t* raw_from /*[n_raw]*/,
                       const double* raw_const /*[n_raw]*/);
int smc_pmmh_rejuvenate(smc_handle prop, smc_handle main /*or NULL*/, const double* y, int64_t T, double xi,
                        const double* chol /*[d_theta][d_theta]*/, const double* scales /*[chain]*/, int chain,
                        const uint64_t* filter_seeds /*[chain]*/, uint64_t move_seed, double* theta /*[n_theta][d_theta]*/,
                        double* logZ /*[n_theta]*/, uint8_t* accepted /*[n_theta] or NULL*/, int64_t* filters_run /*or NULL*/);
/* ---- the OUTER level of the samplers: one integer, order-free, shardable specification (host code, no GPU needed) --------
 * reweight (undefined in the reference's tree; == normalize, src/particles.jl:5-15) is the inner filter's normalize with
 * segments of SMC_OUTER_SEG consecutive entries: per segment the record (kb, S, S2hi, S2lo) = (largest binary exponent, sum
 * and sum of squares of the 48-bit fixed-point weights relative to it), combined by shifts against the largest kb.  Integer
 * sums only: the same bits for any order of evaluation and for any dealing of whole segments to ranks (a rank computes the
 * records of the segments it holds, the ranks exchange records, every rank combines them).  The online sampler carries the
 * UN-NORMALISED outer log-weights logw: smc²!'s `log.(omega) .+ lik` (:324) of re-normalised weights (:338) is the same
 * weight vector up to a common factor, which reweight removes. */
#define SMC_OUTER_SEG 8
int smc_outer_seg(void);
/* reweight(logw) -> (logmu, w, ess)   src/smc_samplers.jl:232,249,265,298,338; w [n] or NULL */
int smc_host_reweight(const double* logw, int64_t n, double* w, double* logmu, double* ess);
/* the records of the whole segments a rank holds (n_local entries beginning at a multiple of SMC_OUTER_SEG; the last segment
 * of the whole vector may be short): rec [ceil(n_local / SMC_OUTER_SEG)][4] 8-byte words (bits of kb, S, S2hi, S2lo) */
int smc_host_outer_records(const double* logw_local, int64_t n_local, uint64_t* rec);
/* (logmu, ess) of a vector of n_total entries from the records of ALL its segments, in segment order */
int smc_host_outer_combine(const uint64_t* rec, int64_t nseg, int64_t n_total, double* logmu, double* ess);
/* the host half of up to k consecutive smc²! steps (src/smc_samplers.jl:323-338) over the log-likelihood increments
 * lik [k][n_local] of a window of inner-filter steps, in three pieces so that only records cross the ranks:
 *   smc_host_outer_window   records of logw + lik_1, logw + lik_1 + lik_2, ... (nothing modified): rec [k][nseg_local][4]
 *   smc_host_outer_walk     ess of every step from the records of ALL segments, rec [k][nseg][4]; stops after the first step with
 *                           ess < ess_min: *j_out = steps walked, ess_out [k]
 *   smc_host_outer_advance  keep the first j steps: logw .+= lik_t, logZ .+= lik_t, t = 1..j in step order (:333-334) */
int smc_host_outer_window(const double* logw_local, const double* lik /*[k][n_local]*/, int k, int64_t n_local, uint64_t* rec);
int smc_host_outer_walk(const uint64_t* rec, int k, int64_t nseg, int64_t n_total, double ess_min, double* ess_out /*[k]*/, int* j_out);
int smc_host_outer_advance(double* logw, double* logZ, const double* lik /*[k][n]*/, int j, int64_t n);
/* the bisection for the next tempering exponent of density_tempered (src/smc_samplers.jl:240-266) in one call: *xi_new, the
 * ESS of reweight((xi_new - xi) .* logZ), *resample_flag = 0 at the corner solution xi_new = 1 (:261-266); logw_out [n] or
 * NULL = (xi_new - xi) .* logZ */
int smc_host_outer_temper(const double* logZ, int64_t n, double xi, double ess_min, double* xi_new, double* ess, int* resample_flag,
                          double* logw_out);
/* the index draw of resample!(smc) (src/smc_samplers.jl:74-84: sample(1:n, Weights(w), m)) for the weights exp(logw): m iid
 * draws through the inverse of the integer weight CDF, pick numbers = 64-bit Philox draws keyed by `seed`; ancestors in ASCENDING
 * order, 0-based (the order of a resampled population carries no information; ascending keeps most filter copies of a sharded
 * online sampler on their rank).  All weights zero: the identity. */
int smc_host_outer_resample(const double* logw, int64_t n, int64_t m, uint64_t seed, int32_t* a /*[m]*/);
/* random_walk_kernel(theta) (src/smc_samplers.jl:87-101): lower Cholesky factor L [d][d] (row-major) of the PMMH proposal
 * covariance 2.83^2/d cov(theta) + 1e-10 I (1e-2 I when norm(cov) < 1e-8) from the cloud theta [n][d], fixed order of
 * operations; d = 1: L = [[2.83^2 var + 1e-10]] handed to Normal() as a standard deviation (:87-92), *univariate = 1 */
int smc_host_rw_factor(const double* theta, int64_t n, int d, double* L /*[d][d]*/, int* univariate);
/* the tail of smc_host_rw_factor from a covariance cov [d][d] (symmetric): Frobenius norm and collapse rule, the 2.83^2/d
 * scaling, the 1e-10 jitter, the Cholesky factorisation column by column.  smc_host_rw_factor is its serial index-order
 * covariance followed by this call; the IBIS sampler with device_moves hands it the covariance of smc_ibis_theta_moments.
 * An error (not an abort) when the scaled covariance is not positive definite. */
int smc_host_rw_factor_cov(const double* cov /*[d][d]*/, int d, double* L /*[d][d]*/, int* univariate);
/* the spec's PMMH pieces on the host (parity tests): proposal, log prior (NaN-free; -inf outside the support) */
int smc_host_pmmh_propose(int d_theta, uint64_t move_seed, uint32_t stream, uint32_t c, const double* theta,
                          const double* chol, double scale, double* prop);
double smc_host_pmmh_log_uniform(uint64_t move_seed, uint32_t stream, uint32_t c);
double smc_host_prior_logpdf(int family, const double* par /*[SMC_PRIOR_NPAR]*/, double x);

/* Moving whole filters between handles / GPUs (outer resample! of the online sampler when theta is
 * sharded, src/smc_samplers.jl:74-84 + SURVEY 8e/8f.2): pack k slots (x cloud, weights, segment records,
 * logZ) into / out of a caller-provided DEVICE buffer of k * smc_slot_bytes() bytes (e.g. a torch tensor
 * that is then exchanged with an RCCL all-to-all).  idx: local slot indices, host array. */
int smc_slot_bytes(smc_handle h, int64_t* bytes);
int smc_pack_slots(smc_handle h, const int32_t* idx, int64_t k, void* device_buf);
int smc_unpack_slots(smc_handle h, const int32_t* idx, int64_t k, const void* device_buf);

/* ---- theta sharded over the GPUs of one node, for hosts without torch.distributed ---------------------
 * One process per GPU.  Rank 0 calls smc_comm_unique_id and hands the SMC_COMM_ID_BYTES bytes to the other ranks by
 * whatever means the host has (a file, a socket, Julia's Distributed); every rank then calls smc_comm_create.  RCCL
 * (xGMI) underneath, opened with dlopen at the first call.  The collectives are the ones the samplers have:
 *   smc_outer_reweight       reweight(logZ) / reweight(logw) of src/smc_samplers.jl:232,249,265,298,338 with the
 *                            entries sharded over the ranks: the SAME function as smc_host_reweight on the concatenated
 *                            vector, bit for bit, for any number of ranks.  w_all and logw_all NULL and n_local a multiple of
 *                            SMC_OUTER_SEG: the ranks exchange segment records only; otherwise one all-gather of the slices
 *   smc_comm_all_gather      n doubles per rank -> [world][n] on every rank (theta / logZ / accepted after rejuvenate!)
 *   smc_comm_exchange_slots  resample!(smc) of the online sampler (src/smc_samplers.jl:74-84) when the filters of `h`
 *                            are sharded: a[m] is the GLOBAL ancestor of GLOBAL slot m (same vector on every rank, rank r
 *                            holds slots [r M/world, (r+1) M/world)); whole filters travel device to device */
#define SMC_COMM_ID_BYTES 128
typedef struct smc_comm_s* smc_comm;
int smc_comm_unique_id(void* id /*[SMC_COMM_ID_BYTES] out*/);
int smc_comm_create(const void* id, int rank, int world, int device, smc_comm* out);
int smc_comm_destroy(smc_comm c);
int smc_comm_rank(smc_comm c, int* rank, int* world);
int smc_comm_all_gather(smc_comm c, const double* local /*[n]*/, int64_t n, double* all /*[world][n]*/);
int smc_outer_reweight(smc_comm c, const double* logw_local /*[n_local]*/, int64_t n_local, double* logw_all /*or NULL*/,
                       double* w_all /*[n_local*world] or NULL*/, double* logmu, double* ess);
int smc_comm_exchange_slots(smc_comm c, smc_handle h, const int32_t* a /*[M]*/, int64_t M);
/* the plan smc_comm_exchange_slots follows, as pure host arithmetic (no GPU; tested on CPU against the Python twin):
 * send_idx [<= M] local slots to pack, grouped by destination rank (send_cnt [world], *n_send in total); dest_idx [M/world]
 * local slots to unpack into, grouped by source rank (recv_cnt [world]) */
int smc_comm_plan_exchange(const int32_t* a /*[M]*/, int64_t M, int rank, int world, int32_t* send_idx, int64_t* send_cnt /*[world]*/,
                           int64_t* n_send, int32_t* dest_idx, int64_t* recv_cnt /*[world]*/);

/* raw fixed-point weight state (tests): C [n_theta][nseg*seg], m/S/S2hi/S2lo [n_theta][nseg] */
int smc_get_weights_raw(smc_handle h, uint64_t* C, double* m, uint64_t* S, uint64_t* S2hi, uint64_t* S2lo);
int smc_get_geometry(smc_handle h, int* seg, int* nseg, int* d, int* resident);
/* device time (HIP events on the handle's stream) of the last log_likelihood / step_window call; after smc_init / smc_step (which
 * place no events on the stream: their results arrive through a ticket in pinned host memory) the host time spent waiting */
int smc_last_elapsed_ms(smc_handle h, double* ms);
int smc_synchronize(smc_handle h);
/* roofline measurement: runs log_likelihood through the one-launch-per-step path and brackets
 * `nsample` evenly spaced runs of 32 consecutive k_step launches (8 when T < 513, one when T < 65) with HIP events
 * on the handle's stream; returns the average / minimum bracketed duration PER k_step launch in ms. */
int smc_time_step_kernel(smc_handle h, const double* y, int64_t T, int nsample, double* avg_ms, double* min_ms);
/* what an EMPTY HIP-event bracket measures on the handle's stream (average of nsample brackets with a
 * trivial kernel before them): the fixed cost contained in every bracketed figure above. */
int smc_event_overhead_ms(smc_handle h, int nsample, double* avg_ms);

/* ---- stand-alone A1 / A2 ---------------------------------------------------------------------*/
/* normalize(logw) -> (logmu, w, ess)                        src/particles.jl:5-15
 * (also the samplers' `reweight`, src/smc_samplers.jl:232,249,265,298,338) */
int smc_normalize(const double* logw, int64_t n, double* w, double* logmu, double* ess, int device);
/* resample(w, N) -> N iid Categorical(w) indices, unsorted  src/particles.jl:17-19 */
int smc_resample(const double* w, int64_t n, int64_t ndraw, uint64_t seed, uint32_t stream, uint32_t t, int32_t* a,
                 int device);

/* ---- SURVEY 8(f) "next" rows --------------------------------------------------------------------*/
/* log_likelihood(y, model::LinearModel) -> (x_T, Sigma_T, logZ): exact scalar Kalman filter,
 * src/kalman_filter.jl:29-70, for n_theta parameter rows at once (the inner "filter" of the IBIS
 * sampler src/ibis.jl:134-189, and a self-check of linear-Gaussian particle runs).
 * raw [n_theta][6] = (A,B,Q,R,x0,sigma0); out [n_theta][3]. predict_first != 0 is the literal
 * reference loop; 0 starts at x_1 ~ N(x0, sigma0) like bootstrap_filter. */
int smc_kalman_log_likelihood(const double* raw, int64_t n_theta, const double* y, int64_t T, int predict_first,
                              double* out /*[n_theta][3]*/, int device);
/* ---- missing observations of the exact Kalman filter ---------------------------------------------------------------
 * Opt-in, as for the particle filters: with SMC_FLAG_NAN_MISSING - set on an IBIS handle by smc_ibis_set_flags, or passed as
 * the trailing `flags` of the *_flags calls, whose unsuffixed names are their flags = 0 call - a NaN observation is a period
 * WITHOUT an observation.  The missing Kalman step (csrc/smc_spec.h, beside kalman_step) is kalman_step with the observation's
 * part left out: the prediction x <- A x, Sigma <- A^2 Sigma + Q as kalman_step forms it (none at the first step of a filter
 * with predict_first = 0: the state stays (x0, sigma0)), no update, and the value +0.0.  So logZ and logw gain +0.0 and keep
 * their bits, the outer weights and hence the ESS of a missing step are the previous step's (a gap never triggers a
 * resample-move by itself), the filtered record at a gap is the predictive pair, the RTS backward pass and the backward-sampled
 * paths run over that record unchanged (the smoothed state at a gap is the interpolation), and a summary row at a gap is, at
 * ahead = 0, the predictive law of the unobserved y_t.  Only NaN is missing: +-inf takes the ordinary step.  A NaN WITHOUT the flag
 * behaves as it always did (it poisons x, Sigma, logZ and logw of every particle).  Every call that runs kalman_step takes the
 * rule: smc_ibis_window / _window_ess / _commit / _filter / _rejuvenate (so the online logZ and a re-filter of the same
 * observations stay the same number) / _smooth / _sample_paths on a flagged handle, and the calls below.  The kernels with the
 * test (a compile-time twin; the test is uniform over a wave) are launched only when the flag is set AND the observations of the
 * launch hold a NaN: every other launch is the kernel an unflagged handle runs.  Cost: profiles/ibis_missing_cost.log.
 * NOT covered: smc_rb_sample_paths (above).
 *   smc_ibis_set_flags   flags = 0 or SMC_FLAG_NAN_MISSING (anything else: SMC_EINVAL).  Only while the handle is at t = 0 with no
 *                        window pending (else SMC_ESTATE): a series is filtered under one rule from its first step
 *   smc_ibis_get_flags   the flags of the handle
 *   smc_host_kalman_steps  the step loop of ONE row on the host (no GPU): row [6], y [T] -> xf, Sf, lik [T] (each or NULL), the
 *                        filtered record and the value of every step - the host array for every device array of these calls */
int smc_ibis_set_flags(void* h, uint32_t flags);
int smc_ibis_get_flags(void* h, uint32_t* flags);
int smc_kalman_log_likelihood_flags(const double* raw, int64_t n_theta, const double* y, int64_t T, int predict_first,
                                    double* out /*[n_theta][3]*/, int device, uint32_t flags);
int smc_kalman_smooth_flags(const double* raw /*[n_theta][6]*/, int64_t n_theta, const double* y, int64_t T, int predict_first,
                            double* xs /*[T][n_theta]*/, double* Ps /*[T][n_theta]*/, int device, uint32_t flags);
int smc_host_ibis_smooth_flags(const double* rows /*[M][6]*/, const double* logw /*[M]*/, int64_t M, const double* y, int64_t T,
                               int predict_first, double* out /*[T][8]*/, double* xs /*or NULL*/, double* Ps /*or NULL*/,
                               double* xf /*or NULL*/, double* Sf /*or NULL*/, uint32_t flags);
int smc_host_ibis_sample_paths_flags(const double* rows, int64_t M, const double* y, int64_t T, int predict_first, int64_t Mp,
                                     uint64_t path_seed, const int32_t* which, double* paths /*[T][Mp]*/, double* z /*[T][Mp] or NULL*/,
                                     uint32_t flags);
int smc_host_kalman_steps(const double* row /*[6]*/, const double* y, int64_t T, int predict_first, uint32_t flags,
                          double* xf /*[T] or NULL*/, double* Sf /*[T] or NULL*/, double* lik /*[T] or NULL*/);
/* ---- the IBIS sampler: src/ibis.jl (SMC^2 with the exact Kalman filter inside) ------------------------------------
 * A handle of its own (opaque; `void*` at this boundary) keeps M parameter particles on the device for its whole life:
 * theta, the LinearModel row smc.model(theta) = (A,B,Q,R,x0,sigma0), the Kalman state (x, Sigma), logZ and the
 * un-normalised outer log-weight logw (see "the OUTER level" above).  One lane per particle; the only random numbers are
 * the PMMH proposal normals and accept uniforms of smc_pmmh_rejuvenate's contract, keyed by (move_seed, particle index,
 * chain position): results do not depend on launch geometry, window length or device.
 *   smc_ibis_create      IBIS(M, model, prior, chain, ess_threshold)      :26-58 (the device half: storage).  predict_first as
 *                        in smc_kalman_log_likelihood: 0 starts at x_1 ~ N(x0, sigma0); != 0 is the reference's literal
 *                        kalman_filter on y[1] (:136-140).  It applies to t = 1 online AND to every re-filter of
 *                        smc_ibis_rejuvenate / smc_ibis_filter, so that an online logZ and a re-filter of the same
 *                        observations are the same number.  `out` receives the handle (the address of a void*).
 *   smc_ibis_configure   the prior and smc.model(theta), the arguments of smc_pmmh_configure (the family is LG1D: 6 row entries)
 *   smc_ibis_set_theta   theta [n_theta][d_theta] (:35); rows, (x, Sigma) = (x0, sigma0) (:38-40), logZ = logw = 0, t = 0
 *   smc_ibis_window      smc²! :166-187 for k <= 64 observations in ONE launch (smc², :134-147, is k = 1 on a fresh state):
 *                        per step (x, Sigma) <- kalman_filter(row, x, Sigma, y_t), logw += lik, logZ += lik, and the
 *                        segment records of reweight(logw) (:187) computed on the device - rec [k][nseg][4] 8-byte words,
 *                        bit for bit what smc_host_outer_window gives for the same lik; lik [k][n_theta] or NULL.
 *                        The host walks the records (smc_host_outer_walk).  Nothing is advanced until
 *   smc_ibis_commit      keeps the first j <= k steps of the pending window (the same bits whatever k was)
 *   smc_ibis_filter      log_likelihood(y, model(theta[m])) for every m from (x0, sigma0) (density_tempered's first pass):
 *                        (x, Sigma, logZ) of the whole series, logw = logZ, t = T
 *   smc_ibis_permute     resample! :73-84: particle m <- particle a[m] (theta, row, x, Sigma, logZ, logw), a value copy
 *   smc_ibis_set_logw    the outer log-weights as given (the tempered weights of density_tempered)
 *   smc_ibis_rejuvenate  rejuvenate! :86-125 in ONE launch: for every particle the whole `for c in 1:chain` loop - proposal
 *                        theta + sqrt(scales[c]) L z (:97), insupport (:99), the Kalman filter over y[0:T) (:100), the accept
 *                        test log(rand()) < xi (logZ' - logZ) + logprior(theta') - logprior(theta) with logZ' + logprior(theta')
 *                        > -inf (:102-108), the overwrite of theta, logZ, x, Sigma (:109-112) - then logw = 0 (:118).
 *                        *accepted = number of particles that moved at least once (sum(acc_array), :121); moved [n_theta] or NULL.
 *   smc_ibis_get         any of theta [n_theta][d_theta], x, S, logZ, logw [n_theta]; NULL: not wanted */
int smc_ibis_create(int64_t n_theta, uint64_t seed, int device, int predict_first, void* out);
int smc_ibis_destroy(void* h);
int smc_ibis_configure(void* h, int d_theta, const int32_t* prior_family /*[d_theta]*/, const double* prior_par /*[d_theta][SMC_PRIOR_NPAR]*/,
                       const int32_t* raw_from /*[6]; [15] on a two-state handle*/, const double* raw_const /*likewise*/);
int smc_ibis_set_theta(void* h, const double* theta /*[n_theta][d_theta]*/);
int smc_ibis_window(void* h, const double* y /*[k]*/, int k, double* lik /*[k][n_theta] or NULL*/, uint64_t* rec /*[k][nseg][4]*/);
int smc_ibis_commit(void* h, int j);
int smc_ibis_filter(void* h, const double* y, int64_t T);
int smc_ibis_permute(void* h, const int32_t* a /*[n_theta]*/);
int smc_ibis_set_logw(void* h, const double* logw /*[n_theta]*/);
int smc_ibis_rejuvenate(void* h, const double* y, int64_t T, double xi, const double* chol /*[d_theta][d_theta]*/,
                        const double* scales /*[chain]*/, int chain, uint64_t move_seed, int64_t* accepted /*or NULL*/,
                        uint8_t* moved /*[n_theta] or NULL*/);
int smc_ibis_get(void* h, double* theta, double* x, double* S, double* logZ, double* logw);
/* ---- two-state linear models: the exact Kalman side (src/state_space_models.jl:137-202, src/kalman_filter.jl:3-27) -----
 * MultivariateLinearGaussian with a 2 x 2 transition and a scalar observation, hodrick_prescott among them:
 *   x_t ~ N(A x_{t-1}, Q),  y_t ~ N(B x_t, R),  x_1 ~ N(x0, Sigma0)
 * as a row of 15 doubles (A11,A12,A21,A22, B1,B2, Q11,Q21,Q22, R, x01,x02, S11,S21,S22).  Q and Sigma0 are symmetric, stored
 * as their lower triangle, and may be singular (hodrick_prescott: Q = [1/lambda 0; 0 0]).  The row's id, SMC_MODEL_LG2D, is no
 * particle-filter family - a singular Q has no transition density - so smc_create, smc_simulate, smc_model_dim and
 * smc_model_nraw refuse it; these models run through the exact filter below.  One order of operations on host and device
 * (csrc/smc_spec.h kalman2_step, rts2_step).  predict_first as in smc_kalman_log_likelihood.  A step whose innovation variance
 * is not a positive finite number poisons logZ (NaN) as the scalar step does; nothing faults.
 *   smc_kalman2_log_likelihood  log_likelihood(y, model) (:55-70) for n rows, one lane each: out [n][6] = (x1, x2, S11, S21, S22, logZ)
 *   smc_kalman2_smooth          the RTS smoother of every row: xs [T][n][2], Ps [T][n][3] (lower triangle).  A period whose
 *                               predicted covariance has a determinant that is <= 0 or not finite has no smoothed state: it
 *                               and every earlier period are NaN; the last period is the filtered state.  That cannot happen
 *                               when A is invertible and Sigma0 positive definite, or Q is positive definite.
 *   smc_host_kalman2_steps      the step loop of ONE row on the host (no GPU): xf [T][2], Sf [T][3], lik [T], each or NULL.
 *                               Every device array of the two-state calls has the bits of a composition of this call.
 *   smc_host_kalman2_smooth     the backward walk of ONE row on the host: xs [T][2], Ps [T][3], the bits of smc_kalman2_smooth
 *   smc_simulate_lg2            simulate(rng, model, T) on the host: x [2][T] (or NULL), y [T].  The factor of a singular
 *                               covariance C is l11 = sqrt(C11), l21 = C21 / l11 (0 when C11 = 0), l22 = sqrt(max(C22 - l21^2, 0));
 *                               the normals are the Philox slots smc_simulate uses
 * SMC_EINVAL: a NULL array, n outside [1, 2^30], T outside [1, 2^31], a bad device.  SMC_ENOMEM: the device arrays of the call.
 *
 * The IBIS sampler over such rows is the same handle type, created with
 *   smc_ibis_create_rows        smc_ibis_create with the row id of the particles: SMC_MODEL_LG1D (what smc_ibis_create makes) or
 *                               SMC_MODEL_LG2D.  Every smc_ibis_* signature is as it is.  On a two-state handle
 *                               smc_ibis_configure reads 15 raw_from / raw_const entries, smc_ibis_get gives x [n_theta][2] and
 *                               S [n_theta][3], and smc_ibis_set_theta, _window, _window_ess, _commit, _filter, _rejuvenate,
 *                               _permute, _resample run kalman2_step in place of the scalar step; smc_ibis_set_logw,
 *                               _theta_moments, _theta_quantiles, _theta_histogram, _get_moved are the same code for both.
 *                               Refused on a two-state handle with
 *                               SMC_EINVAL, the handle unchanged (follow-ups): smc_ibis_set_flags with SMC_FLAG_NAN_MISSING,
 *                               smc_ibis_summary, smc_ibis_set_summaries, smc_ibis_get_summaries, smc_ibis_smooth,
 *                               smc_ibis_sample_paths. */
#define SMC_MODEL_LG2D 16
int smc_kalman2_log_likelihood(const double* raw /*[n][15]*/, int64_t n, const double* y, int64_t T, int predict_first, double* out /*[n][6]*/,
                               int device);
int smc_kalman2_smooth(const double* raw /*[n][15]*/, int64_t n, const double* y, int64_t T, int predict_first, double* xs /*[T][n][2]*/,
                       double* Ps /*[T][n][3]*/, int device);
int smc_host_kalman2_steps(const double* row /*[15]*/, const double* y, int64_t T, int predict_first, double* xf /*[T][2] or NULL*/,
                           double* Sf /*[T][3] or NULL*/, double* lik /*[T] or NULL*/);
int smc_host_kalman2_smooth(const double* row /*[15]*/, const double* y, int64_t T, int predict_first, double* xs /*[T][2]*/, double* Ps /*[T][3]*/);
int smc_simulate_lg2(const double* row /*[15]*/, int64_t T, uint64_t seed, double* x /*[2][T] or NULL*/, double* y /*[T]*/);
int smc_ibis_create_rows(int64_t n_theta, uint64_t seed, int device, int predict_first, int row_id, void* out);
/* Summaries of an IBIS cloud, on the device (src/plotting_utils.jl:94-137: observation_dist, estimated_trend, quantile).  With
 * omega the normalised weights of logw and, per particle, ym = B x, vm = B^2 Sigma + R (ahead = 0) or the same after one
 * Kalman prediction x <- A x, Sigma <- A^2 Sigma + Q (ahead = 1, the one-step forecast the comment at :126-127 asks for):
 *   out [8] = (y, Sigma, between, xbar, Sbar, between_x, K, D)
 *   y = sum omega ym, Sigma = sum omega vm                     observation_dist literally at ahead = 0 (:107-108)
 *   between = sum omega (ym - y)^2                             what the reference's Sigma leaves out: Sigma + between is the
 *                                                              variance of the mixture sum omega N(ym, vm)
 *   xbar = sum omega x, Sbar = sum omega Sigma_m, between_x    the filtered state, whatever `ahead`
 *   K, D                                                       logsumexp(logw) = K ln 2 + log D
 * The order of every operation is fixed by csrc/smc_spec.h ("summaries of an IBIS cloud": chunks of 64 particles, a tree
 * within the chunk, chunks left to right; one pass with a shift per chunk), so the result is a function of the arrays alone: no
 * atomics, the same bits from the stand-alone call, from a window's recording and from the host twin.  A particle whose logw
 * is -inf or NaN contributes nothing, whatever its x.  NaN (K = -inf, D = 0) when no particle is alive.
 *   smc_ibis_summary        the committed cloud, two small launches, 64 bytes read back
 *   smc_ibis_set_summaries  on != 0: every later smc_ibis_window also records the row of summaries after each of its k steps
 *                           (a template flag of the window kernel; off: the kernel of before)
 *   smc_ibis_get_summaries  the first j <= k rows of the last recorded window, out [j][8]: bit for bit smc_ibis_summary after
 *                           the same steps taken one at a time - also for the j steps kept of a window that smc_ibis_commit cuts
 *   smc_host_ibis_summary   the same specification on the host (no GPU): rows [M][6] = (A,B,Q,R,x0,sigma0), x, S, logw [M] */
int smc_ibis_summary(void* h, int ahead, double* out /*[8]*/);
int smc_ibis_set_summaries(void* h, int on, int ahead);
int smc_ibis_get_summaries(void* h, int j, double* out /*[j][8]*/);
int smc_host_ibis_summary(const double* rows, const double* x, const double* S, const double* logw, int64_t M, int ahead, double* out /*[8]*/);
/* The resample-move loop of the IBIS sampler without a read of the cloud (IBIS(..., device_moves=True)): what the host does
 * on O(M) numbers after smc_ibis_window, smc_ibis_get and smc_ibis_rejuvenate, as reductions, scans and searches on the
 * device.  The integer parts give the bits of their host functions; the moments have a specification of their own.
 *   smc_ibis_window_ess     smc_ibis_window, but the records stay on the device: per step the three integers of the segment
 *                           combine (K = max kb, D = sum seg_Q, R = sum seg_R: integer maxima and sums, any order) are
 *                           reduced there, k x 20 bytes come back, and the walk stops at the first step with ess < ess_min.
 *                           ess_out [k] (the first *j_out are set), *j_out: bit for bit smc_host_outer_walk on the records
 *                           smc_ibis_window returns for the same state and y.  smc_ibis_commit and the recording of the
 *                           summaries behave as after smc_ibis_window.
 *   smc_ibis_resample       the index draw of resample! (:73-84) for the committed logw and its gather: the ancestors of
 *                           smc_host_outer_resample(logw, M, M, seed), bit for bit and in ascending order (fixed-point weights
 *                           and segment sums, an integer scan of the segment table, per draw a binary search for the segment
 *                           and a count inside it, an integer histogram, its scan, its expansion), then smc_ibis_permute's
 *                           value copy with the ancestors left on the device.  a_out [n_theta] or NULL: nothing else crosses
 *                           the bus.  No live particle: the identity.
 *   smc_ibis_theta_moments  mean [d] and cov [d][d] of the theta cloud.  weighted = 0: the sample mean and the corrected
 *                           covariance (divisor M - 1), what random_walk_kernel (smc_samplers.jl:87-101) takes of the
 *                           resampled cloud; weighted = 1: mean = sum omega theta, cov = sum omega (theta - mean)(theta - mean)'
 *                           (uncorrected, the convention of smc_get_moments) with omega the normalised weights of logw - a
 *                           dead particle contributes nothing whatever its theta; NaN when none is alive.  Order of operations:
 *                           csrc/smc_spec.h "moments of the theta cloud" (chunks of 64, a tree within the chunk, chunks left to
 *                           right, a centred second pass): a function of the arrays alone, no atomics on floats.  This is NOT
 *                           the serial index-order sum of smc_host_rw_factor.  Accuracy: the bounds of smc_get_moments below.
 *   smc_host_theta_moments  the same specification on the host (no GPU), the same bits: theta [M][d], logw [M] (NULL when
 *                           weighted = 0)
 *   smc_ibis_get_moved      the moved mask [n_theta] of the last smc_ibis_rejuvenate (which accepts moved = NULL) */
int smc_ibis_window_ess(void* h, const double* y /*[k]*/, int k, double ess_min, double* ess_out /*[k]*/, int* j_out);
int smc_ibis_resample(void* h, uint64_t seed, int32_t* a_out /*[n_theta] or NULL*/);
int smc_ibis_theta_moments(void* h, int weighted, double* mean /*[d_theta]*/, double* cov /*[d_theta][d_theta]*/);
int smc_host_theta_moments(const double* theta, const double* logw, int64_t M, int d, int weighted, double* mean, double* cov);
int smc_ibis_get_moved(void* h, uint8_t* moved /*[n_theta]*/);
/* Quantiles and histograms of the theta cloud, on the device: what construct_histograms (src/plotting_utils.jl:5-37) and the
 * README figures of examples/inflation_example.jl make from smc.theta and smc.omega - the median, a credible interval and the
 * marginal histogram of every parameter - without a read of the cloud.  Integer arithmetic throughout (csrc/smc_spec.h
 * "quantiles and histograms of the theta cloud"): particle m weighs q_m = rint(p_m 2^(32 + k_m - K)) with exp(logw_m) =
 * p_m 2^k_m and K the largest k_m of a live particle, a dead particle (logw -inf, NaN or beyond 7e8 in magnitude) weighs 0
 * whatever its theta, and W = sum q_m < 2^63.  Values are ordered by the IEEE total order of their bits (-0.0 below +0.0, a
 * NaN that carries weight by its sign).  The result is a function of the arrays alone: no float atomics, the same bits from
 * any launch geometry and from the host twins.
 *   smc_ibis_theta_quantiles  out [d_theta][np]: for coordinate i and level p the smallest v among theta[.][i] with
 *                             sum{q_m : theta_mi <= v} > floor(p 2^64) W / 2^64 (smc_get_quantiles' definition, its conversion of
 *                             the level): p = 0 the smallest value that carries weight, p = 1 the largest, no interpolation; NaN
 *                             at every level when no particle is alive.  A radix select over the 64-bit keys, 8 bits a pass, all
 *                             coordinates and levels of the call together; d_theta np doubles come back.  1 <= np <= 8.
 *   smc_ibis_theta_histogram  counts [nbins + 3] of one coordinate over [lo, hi) in nbins equal bins: the sums of q_m in the
 *                             order under (theta < lo) | bins (min((int)((theta - lo) scale), nbins - 1), scale = nbins /
 *                             (hi - lo) computed once) | over (theta >= hi) | nan.  They add up to *W exactly; normalising is
 *                             the caller's division.  1 <= nbins <= 4096.
 *   smc_host_theta_weights    q [M], *K and *W of logw [M] on the host (no GPU): the integers an independent reference starts
 *                             from.  *K = -2^30 when no particle is alive.
 *   smc_host_theta_quantiles, smc_host_theta_histogram   the same specification on the host (a sort), the same bits: theta [M][d]
 * SMC_EINVAL: a NULL array, np or nbins out of range, a level outside [0, 1] or NaN, component outside [0, d), lo or hi not
 * finite, hi <= lo (or hi - lo not finite).  SMC_ESTATE: before smc_ibis_set_theta, and while a window is pending
 * (smc_ibis_commit first).  The handle is read and never written; both kinds of row (smc_ibis_create_rows).  The device scratch
 * (8 n_theta bytes of weights, 0.2 MB of state) lives in the handle, grown at the first call and kept. */
int smc_ibis_theta_quantiles(void* h, const double* p /*[np]*/, int np, double* out /*[d_theta][np]*/);
int smc_ibis_theta_histogram(void* h, int component, double lo, double hi, int nbins, uint64_t* counts /*[nbins + 3]*/, uint64_t* W);
int smc_host_theta_weights(const double* logw, int64_t M, uint64_t* q /*[M]*/, int32_t* K, uint64_t* W);
int smc_host_theta_quantiles(const double* theta /*[M][d]*/, const double* logw, int64_t M, int d, const double* p, int np, double* out /*[d][np]*/);
int smc_host_theta_histogram(const double* theta, const double* logw, int64_t M, int d, int component, double lo, double hi, int nbins,
                             uint64_t* counts, uint64_t* W);
/* The RTS smoother of an IBIS cloud and its backward-sampled paths (Rauch, Tung and Striebel 1965).  smc_ibis_summary gives
 * the filtered state p(x_t | y_1:t) integrated over the cloud; for a linear-Gaussian row the smoothed state p(x_t | y_1:T)
 * is exact as well: one backward recursion per parameter particle over its own filtered record, O(T) per particle, nothing
 * is a Monte-Carlo estimate.  Per particle, with (xf_t, Sf_t) the state kalman_filter leaves after step t from (x0, sigma0)
 * under the handle's predict_first:
 *     xs_T = xf_T, Ps_T = Sf_T;   Sp = A^2 Sf_t + Q,  G = Sf_t A / Sp,  V = Sf_t Q / Sp  (Sp = 0: G = 0, V = Sf_t),
 *     xs_t = xf_t + G (xs_{t+1} - A xf_t),   Ps_t = V + G^2 Ps_{t+1}    (a sum of non-negative terms)
 * and per period the cloud is integrated exactly as smc_ibis_summary does at ahead = 0, with (xs_t, Ps_t) in the place of
 * (x, Sigma) and the particle's own logw: the order of every operation is fixed by csrc/smc_spec.h ("the RTS smoother of an
 * IBIS cloud"), so the device, the host twin and any launch geometry give the same bits.  The handle is read and never
 * written; the device memory of a call (the record, 16 T n_theta bytes, and 128 T ceil(n_theta / 64) bytes of chunk records)
 * is allocated by the call and freed before it returns.  Cost: profiles/ibis_smoother_cost.log.
 *   smc_ibis_smooth        re-filters y[0:T) for every particle of the committed cloud, walks back, and reduces every period:
 *                          out [T][8] = rows of (y, Sigma, between, xbar, Sbar, between_x, K, D) as smc_ibis_summary names
 *                          them - the smoothed fitted observation and the smoothed state; row T-1 is the filtered cloud after
 *                          y[0:T).  xs, Ps [T][n_theta]: the smoothed mean and variance per particle, or NULL.  A particle
 *                          whose logw is -inf or NaN contributes nothing whatever its row; NaN rows when none is alive.
 *                          SMC_EINVAL: T < 1.  SMC_ESTATE: no theta yet, or a window is pending (smc_ibis_commit first).
 *                          SMC_ENOMEM: the record cannot be allocated; the handle is as it was
 *   smc_ibis_sample_paths  Mp trajectories from p(x_1:T | y_1:T, theta), path p under the row of parameter particle which[p]
 *                          (the caller draws `which` from the outer weights, smc_host_outer_resample): x_T = xf_T +
 *                          sqrt(Sf_T) z, x_t = xf_t + G (x_{t+1} - A xf_t) + sqrt(V) z, with z the Box-Muller normal of the
 *                          Philox draw keyed by (path_seed, p >> 1, stream which[p], t, a slot no other draw uses), z0 for an
 *                          even p and z1 for an odd one.  paths [T][Mp].  Path p is a function of (row, y, path_seed, p,
 *                          which[p]) alone.  SMC_EINVAL: T < 1, Mp < 1, a which entry outside [0, n_theta).  SMC_ESTATE and
 *                          SMC_ENOMEM as above
 *   smc_kalman_smooth      the per-row half without a handle, the counterpart of smc_kalman_log_likelihood: raw [n_theta][6]
 *                          = (A,B,Q,R,x0,sigma0) -> xs, Ps [T][n_theta], bit for bit the xs, Ps of smc_ibis_smooth for a cloud
 *                          of these rows
 *   smc_host_ibis_smooth   the same specification on the host (no GPU), the same bits: rows [M][6], logw [M] -> out [T][8];
 *                          xs, Ps [T][M] or NULL; xf, Sf [T][M] or NULL: the filtered record the backward pass ran over
 *   smc_host_ibis_sample_paths  likewise for the paths; z [T][Mp] or NULL: the normal every entry used
 *   smc_ibis_last_elapsed_ms  what the kernels of the last completed smc_ibis_smooth / smc_ibis_sample_paths call of this handle
 *                          took, by device events on its stream (allocation and copies excluded): the measurement behind
 *                          profiles/ibis_smoother_cost.log, as smc_last_elapsed_ms is for a filter handle.  SMC_ESTATE: no such call */
int smc_ibis_smooth(void* h, const double* y, int64_t T, double* out /*[T][8]*/, double* xs /*[T][n_theta] or NULL*/,
                    double* Ps /*[T][n_theta] or NULL*/);
int smc_ibis_sample_paths(void* h, const double* y, int64_t T, int64_t Mp, uint64_t path_seed, const int32_t* which /*[Mp]*/,
                          double* paths /*[T][Mp]*/);
int smc_ibis_last_elapsed_ms(void* h, double* ms);
int smc_kalman_smooth(const double* raw /*[n_theta][6]*/, int64_t n_theta, const double* y, int64_t T, int predict_first,
                      double* xs /*[T][n_theta]*/, double* Ps /*[T][n_theta]*/, int device);
int smc_host_ibis_smooth(const double* rows /*[M][6]*/, const double* logw /*[M]*/, int64_t M, const double* y, int64_t T, int predict_first,
                         double* out /*[T][8]*/, double* xs /*or NULL*/, double* Ps /*or NULL*/, double* xf /*or NULL*/, double* Sf /*or NULL*/);
int smc_host_ibis_sample_paths(const double* rows, int64_t M, const double* y, int64_t T, int predict_first, int64_t Mp, uint64_t path_seed,
                               const int32_t* which, double* paths /*[T][Mp]*/, double* z /*[T][Mp] or NULL*/);
/* filtered mean and variance of every state coordinate under the current weights, on the device
 * (README.md:41,51 summaries; src/plotting_utils.jl:116-124 estimated_trend). mean, var: [d][n_theta].
 * Definition: StatsBase's uncorrected weighted moments with the dense weights w of smc_get_state, mean = sum w x and
 * var = sum w (x - mean)^2 (centred: no cancellation for a state with a level).  Accuracy: against the
 * exactly rounded sums, |mean - m| <= 1e-11 |m| + 1e-12 sqrt(v) and |var - v| <= 1e-9 v + (1e-11 m)^2; var >= 0.
 * NaN mean and var for a collapsed filter (every weight 0), as its quantiles.
 * In SMC_SUMM_UNWEIGHTED mode (smc_set_summary_mode): the sample mean and the corrected sample variance of the cloud. */
int smc_get_moments(smc_handle h, double* mean, double* var);

/* weighted quantiles of state coordinate `component` under the current weights, per filter, on the
 * device: what quantile(smc.x[i], weights(smc.w[i]), [0.25,0.5,0.75]) computes per theta-particle in
 * examples/inflation_example.jl:45-46 (and README.md:41,51 for an unweighted cloud).  Definition: the
 * inverse of the weighted empirical CDF in the filter's integer weights - the smallest particle value v
 * with sum{W_i : x_i <= v} > floor(p * sum W) - no interpolation between particles.  np <= 8;
 * out [n_theta][np]; NaN for a collapsed filter.  The README's unweighted, interpolating quantile(x, p) is
 * the SMC_SUMM_UNWEIGHTED mode (smc_set_summary_mode, which also names the one variant not offered). */
int smc_get_quantiles(smc_handle h, int component, const double* p, int np, double* out);

/* ---- forecasts: the cloud propagated past the last observation ---------------------------------------------------------------
 * p(x_{T+k} | y_1:T) and p(y_{T+k} | y_1:T), k = 1..H, from the current state of the handle (the x, w of smc_get_state) without a
 * copy of the cloud to the host.  Without an observation there is nothing to weigh: no resampling, no normalisation.  Every
 * particle is a chain of its own - its states over the H horizons are ONE coherent trajectory - and keeps its weight.
 * Specification (csrc/smc_spec.h "forecasts"), one step of one particle:
 *   LG1D, SV1D, UCSV3D   x_k = rand(transition(x_{k-1}));  (ym, sd) = mean and standard deviation of observation(x_k);
 *                        yv = sd sd;  yf = fma(sd, e, ym)
 *   UCSV_RB              the marginal step with the measurement update left out.  With (m, a, b, P) = x_{k-1}:
 *                        P- = P + exp(a);  lse = fma(g_eps, z0, a);  lsn = fma(g_eta, z1, b);  x_k = (m, lse, lsn, P-);
 *                        ym = m;  yv = P- + exp(lsn);  yf = fma(sqrt(yv), e, ym)
 * A handle with a proposal (smc_set_proposal) forecasts by the TRANSITION law like any other: a proposal has no role without y.
 * Random numbers: particle i of filter m at horizon k (1-based) takes element i & 1 of the Box-Muller pair of
 * Philox(key = forecast_seed; pair i >> 1, stream[m], k, slot 1 + c) for state normal c, and of slot 8 for e: the convention
 * of the filter's own steps under a seed of the caller's (use one that is not the filter's).  Trajectory i is a function of
 * (parameter row, x_T[i], forecast_seed, stream, i) alone: it does not depend on H, on the launch geometry or on how the
 * horizons are blocked (below), and smc_host_forecast reproduces it bit for bit.
 *
 * smc_forecast: per horizon and filter, under the handle's CURRENT weights (emitted first, as smc_get_moments does) and always
 * by the WEIGHTED definitions - the handle's summary mode is neither consulted nor changed:
 *   mean, var   [H][d][n_theta]   smc_get_moments' definition and accuracy, of every state row of the propagated cloud
 *   q           [H][n_theta][np]  smc_get_quantiles' definition (inverse of the weighted empirical CDF in the integer weights, no
 *                                 interpolation) of state row `component`
 *   obs_q       [H][n_theta][np]  the same definition applied to the predictive draws yf
 *   obs_mean    [H][n_theta]      sum w ym
 *   obs_var     [H][n_theta]      sum w yv + sum w (ym - obs_mean)^2: the variance of the mixture, within plus between,
 *                                 Rao-Blackwellised over the observation noise (each term with smc_get_moments' accuracy)
 * Any output may be NULL; p [np], np <= 8 (0: no quantiles).  A collapsed filter (every weight 0) reads NaN in every row, like its
 * filtered summaries.  For UCSV_RB the forecast trend is a mixture as well: mean = mean of row 0, variance = var of row 0 + mean of
 * row 3.  SMC_ESTATE before smc_init; SMC_EINVAL for H < 1, np outside 0..8, and with np > 0 for a component outside [0, d) or p
 * NULL.  An error leaves the state of the handle, and the results of a following call, as they were.
 * smc_forecast_cloud: the propagated clouds themselves, xf [H][d][n_theta][n_x] and the predictive draws yf [H][n_theta][n_x], dense
 * (no padding); either may be NULL.  With the w of smc_get_state these are weighted trajectories: fan charts, x_{T+k} - x_T,
 * functionals of the whole path.
 * Both READ the handle: x, the weights and their records, logZ, the ancestors, a pending window (smc_step_window) and the record
 * of an armed handle (smc_history_begin) are untouched, and the steps that follow give the bits they would have given.
 * Memory: the clouds of a BLOCK of horizons (8, fewer while a block would exceed 512 MiB; [block][d + 3][n_theta][n_pad] doubles),
 * the scratch of the summaries and the results of the H horizons live in ONE device block owned by the handle: grown on demand,
 * kept between calls, freed by smc_destroy and never handed to the pool of recycled handles.  A block is summarised (or copied
 * out) before the next overwrites it, so the block bounds the memory whatever H.  SMC_ENOMEM leaves the handle usable and without
 * that block.  The environment variable SMC_FORECAST_BLOCK, read at the call, overrides the block length (tuning / tests): the
 * results are the same bits for every block length.
 * smc_host_forecast: the same specification for n particles x [d][n] of ONE filter (parameter row raw, Philox stream `stream`) on
 * the host, no GPU needed: xf [H][d][n], yf, ym, yv [H][n] (NULL: not wanted).  The device clouds equal it bit for bit. */
int smc_forecast(smc_handle h, int64_t H, uint64_t forecast_seed, int component, const double* p /*[np]*/, int np,
                 double* mean, double* var /*[H][d][n_theta]*/, double* q /*[H][n_theta][np]*/,
                 double* obs_mean, double* obs_var /*[H][n_theta]*/, double* obs_q /*[H][n_theta][np]*/);
int smc_forecast_cloud(smc_handle h, int64_t H, uint64_t forecast_seed, double* xf /*[H][d][n_theta][n_x]*/, double* yf /*[H][n_theta][n_x]*/);
int smc_host_forecast(int model_id, const double* raw, const double* x /*[d][n]*/, int64_t n, int64_t H, uint64_t forecast_seed, uint32_t stream,
                      double* xf /*[H][d][n]*/, double* yf /*[H][n]*/, double* ym /*[H][n]*/, double* yv /*[H][n]*/);

/* ---- the smoother: forward filtering, backward smoothing (FFBS; Kitagawa 1996, Doucet, Godsill and Andrieu 2000) -------------
 * Everything above describes p(x_t | y_1:t).  The reference has no smoother: examples/inflation_example.jl:153-176 draws a
 * "filtered trend".  The smoothed weights ws_t of p(x_t | y_1:T) on the clouds of a step-by-step run are
 *     ws_T = w_T,    ws_t^i = w_t^i sum_j ws_{t+1}^j f(x_{t+1}^j | x_t^i) / sum_l w_t^l f(x_{t+1}^j | x_t^l),    t = T-1 .. 1,
 * with w the dense weights of smc_get_state and f the model's transition density, evaluated in the log domain with the row
 * maximum; no renormalisation.  Particles with w = 0 (sources) or ws = 0 (targets) are left out of every sum whatever their
 * states.  The order of every sum is fixed (csrc/smc_spec.h "the smoother": chunks of 128 consecutive particles summed in
 * ascending order with plain adds, chunk partials in ascending order), so the weights are a function of the recorded clouds and
 * the parameter row alone: the same bits from the device, from the host twin, for a filter alone and inside a batch.
 * A filter that collapsed at a recorded step (every weight 0 there) has NaN smoothed weights and moments at every step.
 *   smc_history_begin  arms the record: T_cap slabs of x [d][n_theta][n_x] and w [n_theta][n_x] on the device (SMC_ENOMEM when
 *                      they cannot be allocated: the handle is unchanged).  Every following smc_init / smc_step appends the
 *                      state it leaves (a device-to-device copy and the dense weights, on the handle's stream, no host
 *                      synchronisation); smc_init restarts the record.  Arming an armed handle replaces its record by an empty
 *                      one.  While armed, the calls that would change the state without a recordable step return SMC_ESTATE and
 *                      change nothing: smc_log_likelihood, smc_step_window, smc_step_commit, smc_permute, smc_copy_from (into
 *                      the handle), smc_unpack_slots, smc_comm_exchange_slots, smc_pmmh_rejuvenate (either handle),
 *                      smc_time_step_kernel, and smc_step beyond T_cap.
 *   smc_history_len    steps recorded so far (0 for a handle that is not armed)
 *   smc_history_get    the recorded state of step t (0-based): bit for bit what smc_get_state gave after that step.  x [d][n_theta][n_x],
 *                      w [n_theta][n_x]; either may be NULL.  SMC_ESTATE when not armed, SMC_EINVAL for t outside the record
 *   smc_history_put    overwrites recorded step t of an armed handle with the caller's clouds, in smc_history_get's layouts; NULL
 *                      leaves that part alone (both NULL: nothing happens).  It exists so that the backward pass can be run on
 *                      clouds that a filter would not produce (states that are not finite on zero-weight particles, a step at which
 *                      every weight is 0, subnormal weights: tests/smoother_planted.py), as smc_device_math, smc_device_guided_step
 *                      and smc_device_rb_step exist for the step's arithmetic.  It waits for the handle's stream, then copies; the
 *                      length of the record, the filter state and everything else of the handle stay as they are.  SMC_ESTATE when
 *                      not armed, SMC_EINVAL for t outside the record
 *   smc_history_end    frees the record and disarms; the handle then runs exactly the code of a handle that was never armed.  A
 *                      fresh handle, and one that smc_create recycles from destroyed ones, is disarmed
 *   smc_smooth         the backward pass over the recorded steps, T = smc_history_len: ws [T][n_theta][n_x], mean and var
 *                      [T][d][n_theta] (any may be NULL).  The moments are those of smc_get_moments applied to (x_t, ws_t): mean =
 *                      sum ws x, var = sum ws (x - mean)^2 (centred second pass, the fixed order above, the accuracy stated there;
 *                      NaN when every ws is 0).  The handle's parameter rows must be those the steps ran with.  Any proposal and
 *                      either resampler: the backward pass uses the transition only.  May be called again after more steps.
 *                      SMC_EINVAL: SMC_MODEL_UCSV_RB (its rows m and P are functions of the whole path: no transition density);
 *                      a parameter row whose transition scale (Q; sigma; gamma_eps, gamma_eta) is not a positive finite number.
 *                      SMC_ESTATE: nothing recorded.  Cost: 2 n_x^2 (T - 1) n_theta transition densities, measured in
 *                      profiles/smoother_cost.log (DESIGN.md 2e "Cost"); at most 65535 chunks of 128 particles per filter
 *   smc_host_transition_logpdf  logpdf(transition(model, xp), x) by the specification on the host (no GPU): xp, x [d]
 *   smc_host_smooth    the same specification for ONE filter on the host (no GPU), the same bits: x [T][d][n], w [T][n] ->
 *                      ws [T][n], mean / var [T][d] (both or neither NULL) */
int smc_history_begin(smc_handle h, int64_t T_cap);
int smc_history_len(smc_handle h, int64_t* len);
int smc_history_get(smc_handle h, int64_t t, double* x /*[d][n_theta][n_x]*/, double* w /*[n_theta][n_x]*/);
int smc_history_put(smc_handle h, int64_t t, const double* x /*[d][n_theta][n_x] or NULL*/, const double* w /*[n_theta][n_x] or NULL*/);
int smc_history_end(smc_handle h);
int smc_smooth(smc_handle h, double* ws /*[T][n_theta][n_x] or NULL*/, double* mean /*[T][d][n_theta] or NULL*/, double* var /*[T][d][n_theta] or NULL*/);
int smc_host_transition_logpdf(int model_id, const double* raw, const double* xp /*[d]*/, const double* x /*[d]*/, double* out);
int smc_host_smooth(int model_id, const double* raw, int64_t T, int64_t n, const double* x /*[T][d][n]*/, const double* w /*[T][n]*/,
                    double* ws /*[T][n]*/, double* mean /*[T][d] or NULL*/, double* var /*[T][d] or NULL*/);

/* ---- the smoother: lag-one pair moments (csrc/smc_spec.h "lag-one pair moments") -------------------------------
 * The backward pass forms every pair probability p_ij = P(particle i at t, particle j at t+1 | y_1:T) on its way to ws_t and keeps
 * only the row sums.  smc_smooth_pairs keeps two moments of the pairs as well, at the precision of the marginals and without paths:
 *     cross[t][a][c] = sum_ij p_ij x_t^{i,a} x_{t+1}^{j,c}            = E[x_t^a x_{t+1}^c | y_1:T]
 *     resid2[t][c]   = sum_ij p_ij (x_{t+1}^{j,c} - m_c(x_t^i))^2     = E[(x_{t+1}^c - m_c(x_t))^2 | y_1:T]
 * for t = 0 .. T-2, m the centre of the transition (LG1D: A x; SV1D: mu + rho (x - mu); UCSV3D: x): the E-step of a state-space
 * EM, and with the marginal means the lag-one smoothed covariance cross - mean_t mean_{t+1}.
 *   smc_smooth_pairs       smc_smooth (its refusals, its state rules, its results: ws, mean, var are bit for bit smc_smooth's) with
 *                          cross [T-1][d][d][n_theta] and resid2 [T-1][d][n_theta]; either may be NULL, with both NULL the call IS
 *                          smc_smooth.  Particles of weight 0 are left out whatever their states; no renormalisation; NaN everywhere
 *                          for a filter that collapsed at a recorded step; T = 1: nothing is written.  Any record: guided, systematic,
 *                          with gaps, conditional, or planted (smc_history_put).  May be repeated, also after more steps.  The
 *                          chunk partials, (1 + 2 d) n_chunks n_theta n_x doubles, live in a block of their own that the first
 *                          such call allocates: handles that never ask for pairs allocate and launch what they always did.
 *                          Cost: profiles/pairs_cost.log (DESIGN.md 2m "Cost")
 *   smc_host_smooth_pairs  the same specification for ONE filter on the host (no GPU), the same bits: cross [T-1][d][d], resid2
 *                          [T-1][d] (NULL only when T = 1); ws, mean, var as smc_host_smooth */
int smc_smooth_pairs(smc_handle h, double* ws /*[T][n_theta][n_x] or NULL*/, double* mean /*[T][d][n_theta] or NULL*/, double* var /*[T][d][n_theta] or NULL*/,
                     double* cross /*[T-1][d][d][n_theta] or NULL*/, double* resid2 /*[T-1][d][n_theta] or NULL*/);
int smc_host_smooth_pairs(int model_id, const double* raw, int64_t T, int64_t n, const double* x /*[T][d][n]*/, const double* w /*[T][n]*/,
                          double* ws /*[T][n]*/, double* mean /*[T][d] or NULL*/, double* var /*[T][d] or NULL*/,
                          double* cross /*[T-1][d][d]*/, double* resid2 /*[T-1][d]*/);

/* ---- the smoother: weighted quantiles of the smoothed state (csrc/smc_spec.h "quantiles of the smoothed state") ------
 * smc_smooth describes p(x_t | y_1:T) by a mean and a variance.  The 25 / 50 / 75 % band of a skewed state (a log-volatility, the SV
 * state after a large return) needs the quantiles of (x_t, ws_t), and the smoothed weights are on the device when the backward pass
 * ends: smc_smooth_quantiles selects them there, for every recorded step and filter in one launch, instead of a copy of every weight
 * and cloud to the host and a sort.  The quantile of a cloud is a function of its two arrays alone, in integer arithmetic: particle i
 * takes part iff 0 < ws_i < +inf, whatever its state; ws_i = f_i 2^(e_i) with f_i in [0.5, 1), K = max e_i, q_i = rint(ws_i 2^(40 - K))
 * (ties to even); the states in the IEEE total order of their bits (-NaN < -inf < .. < -0.0 < +0.0 < .. < +inf < +NaN); level p in
 * [0, 1]: the smallest state v with sum{q_i : x_i <= v} > floor(p 2^64) W / 2^64 (rounded down), W = sum q_i - smc_get_quantiles'
 * definition, no interpolation, p = 0 the smallest state that carries weight and p = 1 the largest.  A cloud in which nobody takes part,
 * or with a NaN weight (a filter that collapsed at a recorded step), has NaN at every level.
 *   smc_smooth_quantiles       smc_smooth_pairs (its refusals, its state rules, its results: ws, mean, var, cross, resid2 are bit for
 *                              bit smc_smooth_pairs', each may be NULL; ONE backward pass) with q [T][n_theta][np]: the quantiles of
 *                              state coordinate `component` at the levels p [np].  SMC_EINVAL, the handle unchanged: np outside
 *                              [1, 8], component outside [0, d), a level outside [0, 1] (or NaN), p or q NULL.  Any record: guided,
 *                              systematic, with gaps, conditional, or planted (smc_history_put).  May be repeated, also after more
 *                              steps.  The results, 8 n_theta doubles per step of the record, live in a block of their own that the
 *                              first such call allocates: handles that never ask for quantiles allocate and launch what they always
 *                              did.  Cost: profiles/smooth_quantiles_cost.log (DESIGN.md 2q "Cost")
 *   smc_host_smooth_quantiles  the same specification for ONE coordinate of ONE filter on the host (no GPU), the same bits: x, ws
 *                              [T][n] -> q [T][np].  SMC_EINVAL: a NULL argument, T or n < 1, np or a level as above
 *   smc_smooth_quantiles_info  the constants of the specification and of the kernel, and what a handle holds: scratch_bytes = the bytes
 *                              of h's quantile block (0: it never asked for quantiles; h NULL: 0), q_bits = 40, lds_max = the largest
 *                              n_x whose cloud the kernel stages in LDS (beyond it the same kernel reads global memory in every
 *                              pass).  Any pointer may be NULL */
int smc_smooth_quantiles(smc_handle h, double* ws /*[T][n_theta][n_x] or NULL*/, double* mean /*[T][d][n_theta] or NULL*/, double* var /*[T][d][n_theta] or NULL*/,
                         double* cross /*[T-1][d][d][n_theta] or NULL*/, double* resid2 /*[T-1][d][n_theta] or NULL*/, int component,
                         const double* p /*[np]*/, int np, double* q /*[T][n_theta][np]*/);
int smc_host_smooth_quantiles(int64_t T, int64_t n, const double* x /*[T][n], one coordinate*/, const double* ws /*[T][n]*/, const double* p /*[np]*/,
                              int np, double* q /*[T][np]*/);
int smc_smooth_quantiles_info(smc_handle h /*or NULL*/, int64_t* scratch_bytes, int32_t* q_bits, int64_t* lds_max);

/* ---- predictive checks: PIT and one-step forecast moments (csrc/smc_spec.h "predictive checks") ----------------------
 * logZ ranks models against each other; whether ONE model fits the series is read off the probability integral transform of its
 * one-step-ahead predictive law, u_t = P(Y_t <= y_t | y_1:t-1): iid uniform under a correct model.  A bootstrap filter resamples at
 * every step, so the cloud x_t a step leaves, taken whatever its weights, is a sample of p(x_t | y_1:t-1).  For one filter at one
 * step, n particles in the order of smc_get_state, (ym_i, sd_i) the observation law at x_i and z_i = (y - ym_i) / sd_i as the step
 * forms it:
 *     pit = sum Phi(z_i) / n,   obs_mean = sum ym_i / n,   obs_var = sum sd_i^2 / n + sum (ym_i - obs_mean)^2 / n
 * Phi = smc_host_normcdf; the sums run in chunks of 128, level by level (pred_sum).  A pure function of (cloud, y, parameter row):
 * no weight is read, and nothing is special-cased - a NaN y gives a NaN pit beside the ordinary moments (the forecast of the
 * unobserved y_t, also at a gap of an SMC_FLAG_NAN_MISSING handle), an infinite y gives 0 or 1, a NaN state or a zero sd does what
 * IEEE arithmetic does, a cloud after a dead step gives what the formula gives.
 *   smc_get_predictive    the rows of the CURRENT state for the observation y_t the last step assimilated: [n_theta] each, any NULL.
 *                         State rules of smc_get_moments (SMC_ESTATE before smc_init).  Reads the handle and changes nothing: the
 *                         steps that follow give the bits they would have given.
 *   smc_predictive        the rows of every step of the record of an armed handle (smc_history_begin) in one launch: [T][n_theta]
 *                         each, any NULL; row t is bit for bit what smc_get_predictive(h, y[t]) gave after step t.  SMC_ESTATE
 *                         without a record, SMC_EINVAL when T != smc_history_len.
 *   Both refuse, with SMC_EINVAL and the handle unchanged: a handle with a proposal (its cloud is drawn from the proposal),
 *   SMC_FLAG_CONDITIONAL, and SMC_MODEL_UCSV_RB (its rows hold the updated m, P: the predictive pair is gone).  Scratch: a block of
 *   its own, allocated at the first such call and freed by smc_destroy.
 *   smc_host_predictive   the same specification for ONE cloud x [d][n] on the host (no GPU), the same bits: out = (pit, obs_mean,
 *                         obs_var).  LG1D, SV1D, UCSV3D.
 *   smc_host_normcdf / smc_device_normcdf   Phi in f64, the same bits on both sides: absolute error at most 1e-15 over the whole
 *                         line (measured: csrc/smc_spec.h), 0 <= Phi <= 1, Phi(-inf) = +0, Phi(+inf) = 1, NaN gives NaN.
 *   smc_predictive_info   small_max: clouds of at most this many particles are finished by one workgroup each, larger ones by one
 *                         launch per level of the sums (the same bits; 4096, chosen by measurement: profiles/predictive_cost.log;
 *                         SMC_PRED_SMALL_MAX in the environment moves it within [0, 128^2]); chunk = 128.
 * The exact Kalman side (LinearModel rows (A, B, Q, R, x0, sigma0)): from the predicted pair (x-, S-) of each step,
 *     ym = B x-,  yv = B^2 S- + R,  pit = Phi((y - ym) / sqrt(yv));
 * with SMC_FLAG_NAN_MISSING a NaN y is a gap: the row is (NaN, ym, yv) and the filter takes the missing step.
 *   smc_kalman_predictive_flags   [T][n_theta] each, any NULL, on `device`;   smc_host_kalman_predictive   one row on the host, the same bits. */
int smc_get_predictive(smc_handle h, double y_t, double* pit, double* obs_mean, double* obs_var /*[n_theta] each, any NULL*/);
int smc_predictive(smc_handle h, const double* y /*[T]*/, int64_t T, double* pit, double* obs_mean, double* obs_var /*[T][n_theta]*/);
int smc_host_predictive(int model_id, const double* raw, const double* x /*[d][n]*/, int64_t n, double y, double* out /*[3]*/);
double smc_host_normcdf(double z);
int smc_device_normcdf(const double* z, int64_t n, double* out, int device);
int smc_predictive_info(int64_t* small_max, int* chunk);
int smc_kalman_predictive_flags(const double* raw /*[n_theta][6]*/, int64_t n_theta, const double* y, int64_t T, int predict_first,
                                double* pit, double* ym, double* yv /*[T][n_theta], any NULL*/, int device, uint32_t flags);
int smc_host_kalman_predictive(const double* row /*[6]*/, const double* y, int64_t T, int predict_first, uint32_t flags,
                               double* pit, double* ym, double* yv /*[T]*/);

/* ---- backward simulation: joint smoothing paths (FFBSi; Godsill, Doucet and West 2004) --------------------------------------
 * smc_smooth gives the marginals p(x_t | y_1:T).  Whatever depends on two or more times at once (the smoothed change of the
 * trend, the cycle as a path, lag covariances, the complete-data sums of a particle EM or Gibbs step) needs whole trajectories
 * from p(x_1:T | y_1:T).  Backward simulation draws them by walking back through the recorded clouds: the index of path p at
 * the last step is a draw from w_T, and the index at step t given the state x_{t+1} it chose is a draw from the weights
 * proportional to w_t^l f(x_{t+1} | x_t^l).  Every step is an exact integer computation on the log-weights the smoother forms
 * (csrc/smc_spec.h "backward simulation": the log-weights minus their maximum become integers on a 2^-40 grid, their integer
 * sum S and ONE counter-based 64-bit uniform u per path and step select the smallest index whose running sum exceeds
 * floor(u S / 2^64)), so path p is a function of the recorded clouds, the parameter row, the path seed and the filter's Philox
 * stream id (smc_set_streams; its index by default) alone: the same bits from the device and from the host twin, for any
 * number of paths, for a filter alone and inside a batch.  The marginal law of a path's index at step t, given the clouds, is
 * the smoothed weight ws_t of smc_smooth (up to the 2^-40 grid).  Particles of weight 0 are never chosen, whatever their states.
 *   smc_sample_paths   M paths per filter over the record of an armed handle, T = smc_history_len, with the parameter rows the
 *                      device holds (they must be those the steps ran with).  idx [T][n_theta][M]: the particle of recorded step t
 *                      that path p of filter th passes through; xs [T][d][n_theta][M]: its state, copied bit for bit from the
 *                      record (either may be NULL).  counts [n_theta] (NULL: M everywhere): only the first counts[th] paths of
 *                      filter th are drawn, the slots behind them read -1 and NaN; the drawn ones are those of a call with M
 *                      everywhere.  A filter that collapsed at a recorded step (every weight 0 there) has -1 / NaN everywhere; a
 *                      path whose target no live source reaches (every log-weight -inf) reads -1 / NaN from that step back.  Any
 *                      proposal and either resampler.  It may be called again with other seeds and after more steps, and neither
 *                      needs smc_smooth nor disturbs it (its scratch is its own).  Memory: idx and xs are T n_theta M entries on
 *                      the device as well, so a batch wants a small M.  Cost: 2 M n_x T n_theta pair evaluations (two passes over M x n_x pairs
 *                      at every recorded step; the last step, whose weights need no pair, runs the same kernels), measured
 *                      in profiles/paths_cost.log.
 *                      SMC_EINVAL: SMC_MODEL_UCSV_RB; a transition scale that is not a positive finite number; M outside
 *                      [1, 2^30]; a count outside [0, M]; n_x > 2^20 (the integer sum of a step must stay below 2^61).
 *                      SMC_ESTATE: the handle is not armed or nothing is recorded.  SMC_ENOMEM: the paths and the scratch cannot be
 *                      allocated; the handle is as it was
 *   smc_host_sample_paths  the same specification for ONE filter on the host (no GPU), the same bits: x [T][d][n], w [T][n],
 *                      the filter's Philox stream id -> idx [T][M], xs [T][d][M] (or NULL).  SMC_EINVAL as smc_host_smooth, and
 *                      for M < 1 and n > 2^20 */
int smc_sample_paths(smc_handle h, int64_t M, uint64_t path_seed, const int32_t* counts /*[n_theta] or NULL*/,
                     int32_t* idx /*[T][n_theta][M] or NULL*/, double* xs /*[T][d][n_theta][M] or NULL*/);
int smc_host_sample_paths(int model_id, const double* raw, int64_t T, int64_t n, const double* x /*[T][d][n]*/, const double* w /*[T][n]*/,
                          int64_t M, uint64_t path_seed, uint32_t stream, int32_t* idx /*[T][M]*/, double* xs /*[T][d][M] or NULL*/);

/* ---- the conditional particle filter: particle Gibbs with backward simulation (Andrieu, Doucet and Holenstein 2010) -------------
 * A handle created with SMC_FLAG_CONDITIONAL holds a reference trajectory xref [T][d][n_theta] on the device.  smc_init and every
 * smc_step are the ordinary bootstrap step with ONE slot overridden: slot k*_t = mulhi64(u, n_x), u the first 64-bit word of the
 * Philox draw (seed, pair 0, stream, t, slot 38) - smc_host_conditional_slot - takes the state xref[t] bit for bit, the log-weight
 * logpdf(observation(xref[t]), y_t) - smc_host_logobs - and, with SMC_FLAG_ANCESTORS, the ancestor k*_{t-1} (k*_0 at the first
 * step).  Everything else is the ordinary step's, with the same random numbers.  The slot is random because the multinomial
 * resampler sorts its uniforms: see csrc/smc_spec.h.  Run with the record armed (smc_history_begin), then ONE path of
 * smc_sample_paths adopted with smc_reference_from_paths: together a Markov kernel that leaves p(x_1:T | y_1:T, theta) invariant
 * for any n_x >= 2.  Reseed between sweeps (smc_reseed, and another path seed): a sweep must not reuse its counters.
 * Refused: at smc_create the flag with SMC_FLAG_SYSTEMATIC, SMC_FLAG_NAN_MISSING, SMC_MODEL_UCSV_RB or n_x > 2^20 (SMC_EINVAL);
 * smc_set_proposal with a kind other than SMC_PROP_NONE (SMC_EINVAL); smc_log_likelihood, smc_step_window, smc_step_commit,
 * smc_pmmh_rejuvenate (either role) and smc_time_step_kernel (SMC_ESTATE: they would launch kernels without the override, and the
 * logZ of a conditional run is not a likelihood estimate); smc_init without a reference and smc_step at a time index >= T
 * (SMC_ESTATE).  A conditional handle runs one launch per step, for every segment geometry smc_create accepts. */
/* host -> device; a non-finite entry is refused (SMC_EINVAL); replaces any earlier reference */
int smc_set_reference(smc_handle h, const double* xref /*[T][d][n_theta]*/, int64_t T);
/* path p of the last smc_sample_paths walk over the handle's current record becomes the reference: a device gather from the record
 * through the walk's indices into the reference's own buffer (the next sweep overwrites the record).  A filter whose path p is
 * dead (index -1) keeps its reference; *kept (may be NULL): the number of such filters.  SMC_ESTATE without such a walk, or when a
 * dead path has no reference of that length to keep. */
int smc_reference_from_paths(smc_handle h, int64_t p, int64_t* kept);
/* the reference read back: *T its length (either may be NULL) */
int smc_get_reference(smc_handle h, double* xref /*[T][d][n_theta]*/, int64_t* T);
/* the slot rule and the log-weight of a reference row on the host, no GPU (LG1D, SV1D, UCSV3D) */
int smc_host_conditional_slot(uint64_t seed, uint32_t stream, uint32_t t, int64_t n_x, int64_t* k);
int smc_host_logobs(int model_id, const double* raw, const double* x /*[d]*/, double y, double* out);

/* ---- ancestor sampling: particle Gibbs without the backward walk (Lindsten, Jordan and Schoen 2014) -----------------------------
 * Backward simulation walks the record from the last step to the first, every step waiting for the one behind it.  A handle created
 * with SMC_FLAG_CONDITIONAL | SMC_FLAG_ANCESTOR_SAMPLING draws its next reference without that chain (csrc/smc_spec.h "ancestor
 * sampling"): at every step t >= 1 the pinned particle redraws its ancestor J_t from the weights proportional to
 * w_{t-1}^l f(xref[t] | x_{t-1}^l) - one step of backward simulation with xref[t] as its target, the same integers - and the new
 * path is the ancestor lineage of ONE particle drawn from the last weights, followed through the recorded ancestor vectors, with
 * J_t in the place of the retained slot's ancestor.  The reference is fixed while the draws are made, so they are independent
 * given the record: ONE launch over (t, filter), then one thread per filter for the T lookups and the gather.  It leaves
 * p(x_1:T | y_1:T, theta) invariant for any n_x >= 2, as smc_sample_paths + smc_reference_from_paths do.
 *   the record         smc_history_begin on such a handle also arms an ancestor plane int32 [T_cap][n_theta][n_x]; every smc_step
 *                      appends the ancestor vector it leaves (what smc_get_state gives), row 0 reads -1
 *   smc_history_get_ancestors   row t of the plane.  smc_history_put_ancestors overwrites it (the planted cases of the tests); an
 *                      entry outside [0, n_x) is SMC_EINVAL.  Both: SMC_ESTATE on a handle without the flag or without an armed
 *                      record, SMC_EINVAL for t outside the record
 *   smc_ancestor_sweep the sweep over the handle's record, under its current filter seed (smc_reseed) and stream ids, with the
 *                      parameter rows the device holds: J [T][n_theta] the ancestor draws (J[0] = -1), idx [T][n_theta] the
 *                      particles the new path passes through, *kept the number of dead filters (every last weight 0: idx = -1
 *                      at every step, the reference kept); any may be NULL.  idx[T-1] is idx[T-1][th][0] of
 *                      smc_sample_paths(h, 1, path_seed) on a record without a collapsed step.  The new reference:
 *                      smc_get_reference.  It reads the parameter rows back first (a wait for the steps before it, as in
 *                      smc_sample_paths) and then does not wait for its own two launches unless J, idx or kept is asked for.
 *                      SMC_ESTATE, nothing changed: a handle without the flag, no armed record, no reference, a record whose
 *                      length is not the reference's.  SMC_EINVAL: a transition scale that is not a positive finite number
 *   smc_host_ancestor_sweep  the same specification for ONE filter on the host (no GPU), the same bits: a [T][n] the ancestor
 *                      vectors (row 0 is not read; an entry of a later row outside [0, n): SMC_EINVAL), xref [T][d] the reference
 *                      the steps ran with, the filter seed and stream id -> J [T], idx [T], xref_out [T][d] */
int smc_history_get_ancestors(smc_handle h, int64_t t, int32_t* a /*[n_theta][n_x]*/);
int smc_history_put_ancestors(smc_handle h, int64_t t, const int32_t* a /*[n_theta][n_x]*/);
int smc_ancestor_sweep(smc_handle h, uint64_t path_seed, int32_t* J /*[T][n_theta] or NULL*/, int32_t* idx /*[T][n_theta] or NULL*/, int64_t* kept /*or NULL*/);
int smc_host_ancestor_sweep(int model_id, const double* raw, int64_t T, int64_t n, const double* x /*[T][d][n]*/, const double* w /*[T][n]*/,
                            const int32_t* a /*[T][n]*/, const double* xref /*[T][d]*/, uint64_t seed, uint64_t path_seed, uint32_t stream,
                            int32_t* J /*[T]*/, int32_t* idx /*[T]*/, double* xref_out /*[T][d]*/);

/* ---- Rao-Blackwellised backward simulation: smoothing the marginal UCSV filter (Lindsten et al. 2016) ---------------------------
 * SMC_MODEL_UCSV_RB carries the Kalman mean and variance of the trend inside every particle, and those two rows are functions of
 * the whole volatility path: smc_smooth and smc_sample_paths refuse the family.  But the two log-volatilities are an autonomous
 * Markov chain, and given their path the trend is linear-Gaussian.  So the backward walk runs over the VOLATILITIES alone: the
 * weight of source l at step t is w_t^l f(lse+, lsn+ | lse_l, lsn_l) times the Gaussian density of everything the later
 * observations say about the trend, N(mu; m_l, P_l + exp(lse_l) + tau), where (mu, tau) is one scalar information pair per path
 * updated after every pick (csrc/smc_spec.h "Rao-Blackwellised backward simulation": one log and one division per pair on top
 * of backward simulation's chain; the integers, the uniform and the selection are backward simulation's).  The paths are draws
 * from p(lse_1:T, lsn_1:T | y_1:T); the trend then comes EXACTLY given each path, from a Kalman filter and an RTS pass along
 * it - no Monte-Carlo noise in the trend given the volatilities.  Path p is a function of the record, the parameter row, y, the
 * path seed and the filter's Philox stream id alone: the same bits from the device and the host twin, for any M, alone or in a batch.
 *   smc_rb_sample_paths  M paths per filter over the record of an armed SMC_MODEL_UCSV_RB handle; y [T] are the observations the
 *                      recorded steps saw, T = smc_history_len.  idx [T][n_theta][M]: the particle of step t the path passes
 *                      through; vol [T][2][n_theta][M]: its (lse, lsn); tmean, tvar [T][n_theta][M]: mean and variance of
 *                      p(x_t | the path's volatilities, y_1:T); tdraw: one joint draw of the trend path given the volatilities
 *                      (backward sampling, Philox slot 37); out [T][n_theta][8]: per filter and step, over the complete paths
 *                      among the first counts[th], (trend mean, within = mean of tvar, between = population variance of tmean,
 *                      mean and variance of lse, mean and variance of lsn, the number of complete paths) - the smoothed trend
 *                      has mean out[0] and variance out[1] + out[2].  Every output may be NULL.  counts as in smc_sample_paths.
 *                      A collapsed filter reads -1 / NaN everywhere; a path no live source reaches reads -1 / NaN in idx / vol
 *                      from that step back and NaN in tmean, tvar, tdraw at every step, and is left out of `out`; no complete
 *                      path: NaN and the count 0.  Either resampler.  It may be called again with other seeds and after more
 *                      steps, and disturbs nothing on the handle (its scratch is its own).  Cost: 2 M n_x T n_theta pair
 *                      evaluations plus O(M T n_theta) for the trend (profiles/rb_paths_cost.log).
 *                      SMC_EINVAL: a handle that is not SMC_MODEL_UCSV_RB; T != smc_history_len; a y that is not finite; a gamma
 *                      that is not a positive finite number; M outside [1, 2^30]; a count outside [0, M]; n_x > 2^20.
 *                      SMC_ESTATE: the handle is not armed or nothing is recorded.  SMC_ENOMEM: the paths and the scratch cannot
 *                      be allocated; the handle is as it was
 *   smc_host_rb_sample_paths  the same specification for ONE filter on the host (no GPU), the same bits: raw [5] UCSV's row,
 *                      x [T][4][n], w [T][n], y [T], the filter's Philox stream id -> idx [T][M], vol [T][2][M], tmean, tvar
 *                      [T][M], tdraw [T][M] or NULL, out [T][8] or NULL */
int smc_rb_sample_paths(smc_handle h, const double* y /*[T]*/, int64_t T, int64_t M, uint64_t path_seed, const int32_t* counts /*[n_theta] or NULL*/,
                        int32_t* idx /*[T][n_theta][M]*/, double* vol /*[T][2][n_theta][M]*/, double* tmean /*[T][n_theta][M]*/,
                        double* tvar /*[T][n_theta][M]*/, double* tdraw /*[T][n_theta][M] or NULL*/, double* out /*[T][n_theta][8] or NULL*/);
int smc_host_rb_sample_paths(const double* raw /*[5]*/, int64_t T, int64_t n, const double* x /*[T][4][n]*/, const double* w /*[T][n]*/,
                             const double* y /*[T]*/, int64_t M, uint64_t path_seed, uint32_t stream, int32_t* idx /*[T][M]*/,
                             double* vol /*[T][2][M]*/, double* tmean /*[T][M]*/, double* tvar /*[T][M]*/, double* tdraw /*[T][M] or NULL*/,
                             double* out /*[T][8] or NULL*/);

/* ---- host-side helpers (no GPU needed) ---------------------------------------------------------*/
/* simulate(rng, model, T) -> (x, y)                         src/state_space_models.jl:11-26 */
int smc_simulate(int model_id, const double* raw, int64_t T, uint64_t seed, double* x /*[smc_simulate_dim][T] or NULL*/, double* y /*[T]*/);
/* rows of smc_simulate's x: smc_model_dim(model_id), except for SMC_MODEL_UCSV_RB, whose data-generating model is UCSV3D (3 rows:
 * x, log s_eps, log s_eta - not the 4 rows of the filter's state); -1 for an unknown id */
int smc_simulate_dim(int model_id);
int smc_model_dim(int model_id);
int smc_model_nraw(int model_id);
/* the segment length smc_create picks for seg = 0: a function of the model family (its state dimension) and n_x alone */
int smc_auto_seg(int model_id, int64_t n_x);
int smc_device_count(void);
/* the SMC_SUMM_UNWEIGHTED definitions (smc_set_summary_mode) on the host, by sorting: the type-7 quantiles of x [n] at the levels
 * p [np] in [0, 1] (else SMC_EINVAL), and the sample mean and corrected variance (n == 1: var NaN).  Values that are not numbers:
 * the quantiles order by the IEEE total order of the bits, so a NaN sorts by its sign bit (below -inf when it is set, above +inf
 * when it is not) - a cloud of NaNs has NaN quantiles, a cloud with some has numbers at the levels whose neighbours are numbers
 * (np.quantile would return NaN at every level); mean and variance are NaN as soon as one value is NaN, and a cloud with
 * infinities of one sign has that infinity as its mean and a NaN variance, as mean(x) and var(x).  The device's unweighted
 * summaries order the same way (tests/test_gpu_nonfinite.py). */
int smc_host_quantile7(const double* x, int64_t n, const double* p, int np, double* out);
int smc_host_sample_moments(const double* x, int64_t n, double* mean, double* var);
/* the spec's elementary functions on the host (parity tests of the host build) */
double smc_host_exp(double x);
double smc_host_log(double x);
void smc_host_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
void smc_host_box_muller(const uint32_t w[4], double* z0, double* z1);
/* systematic-resampling targets T_{j0+k} = floor(((j0+k) Dtot + mulhi64(u, Dtot)) / n), k < nk <= 8192, by the
 * division-free evaluation of the kernels; device < 0 evaluates on the host (exactness tests) */
int smc_sys_targets(uint64_t Dtot, uint32_t n, uint64_t u, uint64_t j0, int nk, uint64_t* out, int device);
/* the same functions evaluated on the device for n inputs (math parity tests) */
int smc_device_math(int which /*0 exp,1 log,2 sqrt,3 box-muller z0,4 z1,5 div a/b*/, const double* a, const double* b,
                    int64_t n, double* out, int device);

const char* smc_last_error(void);
const char* smc_version(void);

#ifdef __cplusplus
}
#endif
#endif
