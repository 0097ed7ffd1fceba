// smc_host.h -- what the host-side translation units of libsmchip.so share: the error string behind smc_last_error(), HIPCHK,
// the filter handle, and the few helpers that cross files.  Internal: not installed, not part of the ABI (include/smc_hip.h).
// Which kernel variant a launch of a handle means: pick_variant, here.
// The entry points on a handle: smc_capi.hip (core), smc_capi_series.hip, smc_capi_summ.hip, smc_capi_pmmh.hip,
// smc_capi_slots.hip, smc_capi_smooth.hip, smc_capi_forecast.hip; without one: smc_util.hip, and the exact-Kalman row calls of
// smc_kalman2.hip and smc_ibis.hip - all of them through DeviceCall, here.
#pragma once
#include "../../include/smc_hip.h"
#include "smc_launch.h"

#include <atomic>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

// ---- errors --------------------------------------------------------------------------------------
// stores msg as the calling thread's smc_last_error() and returns code (smc_capi.hip)
int fail(int code, const std::string& msg);
#define HIPCHK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess)                                                                                 \
            return fail(SMC_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ ":" +      \
                                      std::to_string(__LINE__) + ")");                                        \
    } while (0)
// the refusal of a call whose own allocation failed with e
inline int alloc_fail(const char* who, hipError_t e) {
    return fail(e == hipErrorOutOfMemory ? SMC_ENOMEM : SMC_EHIP, std::string(who) + ": " + hipGetErrorString(e));
}

// ---- memory ----------------------------------------------------------------------------------------
// Every device and pinned allocation of the library is a Block: it owns one pointer and its size in bytes, moves (the source is
// left empty), does not copy, and frees in its destructor.  The only calls of hipMalloc / hipHostMalloc / hipFree / hipHostFree
// outside the one per-thread scratch of the calls without a handle (DeviceCall::use_scratch) and the SMC_ABLATE stamps.  A block never synchronises and never selects a
// device: whoever replaces a block the stream may still read waits for the stream first, and whoever lets a handle go selects
// its device first.  Two ways to grow, both no-ops (no runtime call) when the block already holds `need` bytes, both returning
// HIP's error with the sticky error cleared; 0 bytes are allocated as 16.  Kernels only ever see views: plain pointers into blocks.
inline std::atomic<int64_t> g_live_bytes[2];   // [0] device, [1] pinned: allocated and not yet freed (smc_live_bytes)
template <bool PINNED>
class Block {
    void* p_ = nullptr;
    size_t bytes_ = 0;
    hipError_t adopt_new(size_t need) {   // a fresh allocation in place of whatever the block holds; on failure the block is untouched
        void* q = nullptr;
        need = need ? need : 16;
        const hipError_t e = PINNED ? hipHostMalloc(&q, need, hipHostMallocDefault) : hipMalloc(&q, need);
        if (e != hipSuccess) {
            (void)hipGetLastError();   // (the failed allocation is this call's result, not the next call's)
            return e;
        }
        reset();
        p_ = q; bytes_ = need;
        g_live_bytes[PINNED].fetch_add((int64_t)need, std::memory_order_relaxed);
        return hipSuccess;
    }

public:
    Block() = default;
    Block(Block&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    Block& operator=(Block&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
    ~Block() { reset(); }
    void reset() {
        if (!p_) return;
        (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        g_live_bytes[PINNED].fetch_sub((int64_t)bytes_, std::memory_order_relaxed);
        p_ = nullptr; bytes_ = 0;
    }
    // old block first: the old allocation is freed before the new one is made (the peak is one block); on failure the block is empty
    hipError_t grow(size_t need) {
        if (p_ && bytes_ >= need) return hipSuccess;
        reset();
        return adopt_new(need);
    }
    // new block first: the old allocation is freed only once the new one exists; on failure the block is as it was
    hipError_t grow_keep(size_t need) { return p_ && bytes_ >= need ? hipSuccess : adopt_new(need); }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
    template <class T> T* as() const { return (T*)p_; }
};
using DevBlock = Block<false>;   // hipMalloc / hipFree
using PinBlock = Block<true>;    // hipHostMalloc(hipHostMallocDefault) / hipHostFree: coherent, device-visible

// the offsets of the arrays that share ONE allocation: take(n) is where the next n bytes start (256-byte aligned), bytes the total
struct OffsetPlan {
    size_t bytes = 0;
    size_t take(size_t n) { const size_t o = bytes; bytes += (n + 255) & ~(size_t)255; return o; }
};

// The scope of an entry point that runs on the device WITHOUT a handle: after its own argument checks it opens one of these,
// take()s the offsets of all its arrays, asks ONCE for the memory, and then copies, launches (plain hipLaunchKernelGGL on
// `stream`) and waits.  Nothing is planned after the allocation, so no array of a call can move or alias another.
//   begin       device checked against hipGetDeviceCount (SMC_EHIP "<who>: no HIP device", SMC_EINVAL "<who>: bad device"), then
//               selected; stream = the calling thread's hipStreamNonBlocking stream of that device (a table of 16 per thread,
//               created on first use; a device index >= 16 falls back to the null stream).  The streams are never destroyed,
//               not at thread exit either.
//   use_scratch the plan lies in the calling thread's ONE cached allocation: grown when the plan needs more or the device
//               changed, freed at thread exit, NOT counted by smc_live_bytes - the one raw hipMalloc / hipFree outside Block
//               (a hipMalloc / hipFree of a whole cloud's worth per call cost 30 ms per normalize at 2^20 entries, ten times the work)
//   use_own     the plan lies in a block of this scope: counted while the call runs, freed when the scope dies
//               (failure: SMC_ENOMEM / SMC_EHIP "<who>: <hip string>")
// Defined in smc_util.hip.
class DeviceCall {
    const char* who_ = "";
    OffsetPlan plan_;
    DevBlock own_;
    char* base_ = nullptr;
    int device_ = -1;

public:
    hipStream_t stream = nullptr;
    int begin(const char* who, int device);
    size_t take(size_t bytes) { return plan_.take(bytes); }
    int use_scratch();
    int use_own();
    template <class T> T* at(size_t off) const { return (T*)(base_ + off); }
    hipError_t upload(size_t off, const void* host, size_t bytes) { return hipMemcpyAsync(base_ + off, host, bytes, hipMemcpyHostToDevice, stream); }
    hipError_t download(void* host, size_t off, size_t bytes) { return hipMemcpyAsync(host, base_ + off, bytes, hipMemcpyDeviceToHost, stream); }
    hipError_t finish() { return hipStreamSynchronize(stream); }
};

// ---- the filter handle ---------------------------------------------------------------------------
namespace smc {
// device block of the PMMH rejuvenation (smc_pmmh_kernels.h); the handle of the proposal filters owns it
struct PmmhDev {
    double* theta;        // [ntheta][MAX_DTHETA] current parameter particles
    double* prop;         // [ntheta][MAX_DTHETA] proposals of this chain position
    double* logZ;         // [ntheta] log-likelihood estimates of the current particles
    double* lp;           // [ntheta][2] log prior of (proposal, current)
    unsigned char* skip;  // [ntheta] proposal outside the support: its filter is not run
    unsigned char* mask;  // [ntheta] accepted at this chain position
    unsigned char* any;   // [ntheta] accepted at least once in this rejuvenation (acc_array, :135)
    unsigned long long* nrun;   // [1] proposal filters executed so far
    double* chol;         // [d][d] lower Cholesky factor of the random-walk covariance (:95-100)
    int32_t* order;       // [ntheta] the filters of this chain position, those to run first (FilterView::order)
    int32_t* counts;      // [2] how many are to run / skipped (filled by k_pmmh_propose, cleared by k_pmmh_accept)
};
}  // namespace smc

struct smc_filter_s {
    int model = 0, d = 0, device = 0;
    uint32_t flags = 0;
    smc::FilterView v{};
    // Memory (DESIGN.md "Memory of a handle"): every allocation is a block, freed when the handle is deleted; plain pointers are views
    DevBlock d_slab;                           // ONE allocation behind x, C, the segment records, the per-filter scalars, params / streams / perm
    smc::Params* d_params = nullptr;           //   views into the slab
    uint32_t* d_stream = nullptr;
    int32_t* d_perm = nullptr;
    double* d_logZ_tmp = nullptr;
    DevBlock d_y;                              // double [T]: the series of the whole-series calls and the windows (ensure_y)
    DevBlock d_tr_logmu, d_tr_ess;             // double [T][ntheta] each: the traces of smc_log_likelihood
    DevBlock d_wdense;                         // double [ntheta][n] dense weights | [2][d][ntheta] moments (ensure_wdense)
    DevBlock d_recs;                           // smc::StepRec [T][ntheta]: the per-step records of the resident kernels (ensure_recs)
    PinBlock h_pin;                            // pinned host mirror double [4][ntheta]: logZ | last_logmu | last_ess | ticket of the step API
    uint32_t seq = 0;                          // last ticket handed to a step-API launch
    DevBlock d_brk;                            // uint64_t: break points of the steps [v.brk_t0, v.brk_t0 + brk_count)
    uint32_t brk_cap = 0, brk_count = 0;
    PinBlock h_perm;                           // pinned copy of smc_permute's index vector (the call does not wait for the device)
    std::vector<double> prop_par;              // smc_set_proposal(AFFINE): the rows [ntheta][SMC_PROP_NPAR] as given (v.prop_kind: the kind)
    DevBlock d_prop;                           // smc::PropRow [ntheta]: the proposal rows of a guided handle (v.prop) ...
    PinBlock h_prop;                           //   ... and their pinned twin; bootstrap: none
    PinBlock h_params;                         // smc::Params [ntheta]: pinned twin of d_params (smc_set_params does not wait either)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int cur = 0;
    uint32_t t = 0;        // index of the next observation
    const double* gap_y = nullptr;   // SMC_FLAG_NAN_MISSING: the host's copy of the series a whole-series call is enqueueing, when it holds a
                                     //    NaN (GapScope; indexed by t) - its launches take the MISS kernels; nullptr: today's kernels
    bool inited = false;   // weights exist
    bool emitted = false;  // logmu/ess of the current weights already produced
    bool have_params = false;
    bool resident_ok = false;
    smc::Geo geo{0, 0};
    double last_ms = 0.0;
    struct {   // single-filter step launches take filter 0's parameter row and stream id BY VALUE (StepHot, smc_kernels.h): the host's copies
        smc::Params prm0{};
        uint32_t stream0 = 0;
        bool prm_ok = false, stream_ok = false;   // the copy equals the device row; hot_invalidate() after anything the device wrote
        bool allow = true;                        // SMC_STEP_BY_VALUE=0 at smc_create: always through the pointers (tests, measurements)
    } hot;

    struct {   // smc_set_skip: filters log_likelihood leaves out
        DevBlock d_mask;                       // unsigned char [ntheta]
        DevBlock d_order;                      // int32_t: the order the one-workgroup-per-filter kernel takes them in: [ntheta] | n_active
        bool on = false;
        std::vector<uint8_t> h_mask;           // host copy of the mask: the skipped filters' trace columns and summary rows are set to NaN on the host
    } skip;
    struct {   // summaries (smc_capi_summ.hip): per step inside the multi-step calls (smc_set_summaries / smc_get_summaries), and one-shot
        int np = 0, comp = 0, mom = 0;
        uint64_t p64[smc::QMAX] = {};
        double p[smc::QMAX] = {};              // the same levels as doubles in [0, 1]: what the unweighted mode reads
        int mode = SMC_SUMM_WEIGHTED;          // smc_set_summary_mode (v.sum_unw mirrors it)
        DevBlock d_q, d_m;                     // double [T][ntheta][QMAX] | [T][2][d][ntheta]
        int64_t cap = 0, T = 0;                // steps the traces hold / steps the last call recorded
        std::vector<uint8_t> skip;             // the skip mask of the call whose summaries smc_get_summaries hands over (empty: none)
        DevBlock d_ms;                         // uint64_t: scratch of the summaries of multi-segment filters (smc_summ_kernels.h) + [ntheta][QMAX] results
        PinBlock h_once;                       // double [QMAX + 2 d][ntheta]: quantiles / moments of the current state (k_summ_once)
    } summ;
    struct {   // smc_step_window / smc_step_commit
        PinBlock h_out;                        // double [2][WIN_MAX][ntheta]: (logmu, ess) of the steps of a window
        int k = 0;                             // steps of the pending window, 0 = none
        bool gap = false;                      // SMC_FLAG_NAN_MISSING: the pending window's observations hold a NaN (the MISS window kernel)
    } win;
    struct {   // the record of a step-by-step run and the smoother over it (smc_capi_smooth.hip); a fresh handle is disarmed
        bool armed = false;
        int64_t cap = 0, len = 0;              // steps the slabs hold / steps recorded so far
        DevBlock rec;                          // the record, ONE allocation (new block first): d_x | d_w | d_a
        double *d_x = nullptr, *d_w = nullptr; //   its views [cap][d][ntheta][n] | [cap][ntheta][n]
        int32_t* d_a = nullptr;                //   SMC_FLAG_ANCESTOR_SAMPLING: the ancestor plane [cap][ntheta][n], dense like d_w, row 0 reads -1;
                                               //   nullptr (and no bytes) on every other handle
        DevBlock d_ws;                         // the smoother's results (old block first): ws [ws_cap][ntheta][n] | mean, var [len][2][d][ntheta]
        int64_t ws_cap = 0;                    //   steps d_ws was laid out for
        DevBlock d_tmp;                        // its scratch (old block first): chunk maxima and chunk partials [2][nchunk][ntheta][n] | logD [ntheta][n] |
                                               //   partials of the moments [len][ntheta][nchunk] | rows [ntheta] | dead [ntheta]
        DevBlock d_pair;                       // the pair moments (smc_smooth_pairs), a block of their own (old block first): chunk partials
                                               //   [1 + 2 d][nchunk][ntheta][n] | cross [cap - 1][d][d][ntheta] | resid2 [cap - 1][d][ntheta]; empty until the first such call
        DevBlock d_quant;                      // the quantiles of the smoothed state (smc_smooth_quantiles), a block of their own (old block
                                               //   first): q [cap][ntheta][QMAX]; empty until the first such call
        DevBlock d_path;                       // the backward walk (smc_sample_paths, or smc_rb_sample_paths on a MODEL_UCSV_RB handle), its own block
                                               //   (new block first): cur | pmax | psum | rmax | rows | dead | counts | idx [T][ntheta][M] | the caller's tail
        int64_t walk_M = 0, walk_T = 0;        // the last smc_sample_paths walk over this record (0: none): paths per filter, steps, and where
        size_t walk_idx = 0;                   //   its index block starts in d_path (smc_reference_from_paths gathers through it)
    } hist;
    struct {   // the conditional particle filter (SMC_FLAG_CONDITIONAL; smc_capi_cond.hip): the reference, an allocation of its own
        DevBlock d_xref;                       // double [T][d][ntheta] (new block first); empty: none yet (a recycled bundle never carries one)
        int64_t T = 0;
        DevBlock d_sweep;                      // smc_ancestor_sweep (new block first): J [T][ntheta] | idx [T][ntheta] | last [ntheta] | dead [ntheta] |
                                               //   rows [ntheta]; empty until the first sweep
    } cond;
    struct {   // forecasts (smc_capi_forecast.hip): ONE block, grown on demand (old block first)
        DevBlock d_buf;                        // clouds [block][d + 3][ntheta][npad] | summary scratch | results of every horizon
    } fc;
    struct {   // predictive checks (smc_get_predictive / smc_predictive; predictive_run, smc_capi_summ.hip): ONE block of their own,
        DevBlock d_buf;                        // empty until the first such call (old block first): y [T] | pit, obs_mean, obs_var [3][T][ntheta] |
                                               //   large clouds: the partials of the levels of pred_sum
        PinBlock h_out;                        // smc_get_predictive: its rows [3][ntheta], written by the kernel that finishes them
    } pred;
    struct {   // PMMH rejuvenation (smc_capi_pmmh.hip): this handle holds the proposal filters
        smc::PmmhSpec spec{};
        bool cfg = false;
        smc::PmmhDev dev{};                    // views into the blocks below, as the kernels take them
        PinBlock h_out;                        // pinned mirror double: theta [ntheta][d] | logZ [ntheta] | any [ntheta] | nrun
        DevBlock d_in;                         // ONE device block: dev.theta | dev.logZ | dev.chol | dev.nrun | dev.counts | dev.any -
        PinBlock h_in;                         //   a rejuvenation call fills its pinned twin (the same bytes) and uploads it in one copy
        DevBlock d_prop, d_lp, d_skip, d_mask, d_order;   // dev.prop, dev.lp, dev.skip, dev.mask, dev.order
    } pm;
};

// the parameter row of a known family from the caller's: raw [model_nraw_rt(model)] copied, the tail zero, der derived
inline void params_from_raw(int model, const double* raw, smc::Params& P) {
    const int nraw = smc::model_nraw_rt(model);
    for (int k = 0; k < smc::NPARAM; ++k) P.raw[k] = k < nraw ? raw[k] : 0.0;
    smc::derive_params(model, P.raw, P.der);
}
// a row of smc_set_proposal(AFFINE) is usable (smc_capi.hip, and the guided probes of smc_util.hip)
inline bool affine_row_ok(const double* par) {
    for (int k = 0; k < smc::PROP_NPAR; ++k)
        if (!smc::finite_d(par[k])) return false;
    return par[3] > 0.0;
}

// ---- helpers that cross files ----------------------------------------------------------------------
// smc_capi.hip: the launches of one particle step on the handle's stream, and what they need
hipError_t do_init(smc_filter_s* h, double y);
// y: the observation of the step API (v.y == nullptr); y_host: the host's copy of the series v.y points at, or nullptr - with it a
// single-filter launch passes y_host[t] by value as well
hipError_t do_step(smc_filter_s* h, uint32_t t, int emit_prev, double y, const double* y_host = nullptr);
// The host copies of row 0 (hot) no longer describe the device rows: whoever writes parameters, streams or filter slots on the
// device calls this; the next smc_set_params / smc_set_streams makes its half valid again
inline void hot_invalidate(smc_filter_s* h) { h->hot.prm_ok = h->hot.stream_ok = false; }
// a step launch of this handle may take row 0 by value: one filter, both host copies valid (the launch also wants no skip mask)
inline bool hot_legal(const smc_filter_s* h) { return h->hot.allow && h->hot.prm_ok && h->hot.stream_ok && h->v.ntheta == 1; }
// missing observations (include/smc_hip.h): the handle reads NaN as a gap; the series y[0..T) holds one
inline bool nan_missing(const smc_filter_s* h) { return (h->flags & SMC_FLAG_NAN_MISSING) != 0; }
inline bool series_has_gap(const smc_filter_s* h, const double* y, int64_t T) {
    if (!nan_missing(h)) return false;
    for (int64_t t = 0; t < T; ++t)
        if (y[t] != y[t]) return true;
    return false;
}
// the same decision for the exact-Kalman calls (an IBIS handle's flags, or the `flags` argument of a call without a handle)
inline bool kalman_has_gap(uint32_t flags, const double* y, int64_t T) {
    if (!(flags & SMC_FLAG_NAN_MISSING)) return false;
    for (int64_t t = 0; t < T; ++t)
        if (y[t] != y[t]) return true;
    return false;
}
// names the series of a whole-series call for its launches (h->gap_y) when the handle is flagged and the series holds a NaN
struct GapScope {
    smc_filter_s* h;
    GapScope(smc_filter_s* hh, const double* y, int64_t T) : h(hh) { h->gap_y = series_has_gap(h, y, T) ? y : nullptr; }
    ~GapScope() { h->gap_y = nullptr; }
};
// the conditional particle filter (include/smc_hip.h): the handle runs the COND kernels, one launch per step
inline bool conditional(const smc_filter_s* h) { return (h->flags & SMC_FLAG_CONDITIONAL) != 0; }
// ... and draws its next reference by ancestor sampling: the record keeps the ancestor vectors (smc_capi_smooth.hip)
inline bool ancestor_sampling(const smc_filter_s* h) { return (h->flags & SMC_FLAG_ANCESTOR_SAMPLING) != 0; }
// The ONE place that decides which kernels a launch of this handle means: the variant whose object serves entry (LAUNCH_OBJECT,
// smc_launch.h; NO_OBJECT: the handle has no such launch).  gap: this launch covers a missing observation - the step's own is
// NaN, or the series / window of a resident launch holds one (the caller knows from where); false for every unflagged handle.
// Conditional wins; a gap step is the missing step, with a proposal too (LAUNCH_OBJECT says so).
inline int pick_variant(const smc_filter_s* h, int entry, bool gap) {
    using namespace smc;
    const bool guided = h->v.prop_kind != 0;   // (smc_set_proposal: the families of by_guided_model)
    const int variant = conditional(h) ? VARIANT_COND : gap ? (guided ? VARIANT_MISSING_GUIDED : VARIANT_MISSING) : guided ? VARIANT_GUIDED : VARIANT_PLAIN;
    return LAUNCH_OBJECT[variant][entry];
}
// the refusal of the calls that would launch kernels without the override (or read a conditional logZ as a likelihood)
int cond_refuse(const char* who);
hipError_t do_finalize(smc_filter_s* h, int first_emit, uint32_t t_emit);
hipError_t ensure_breaks(smc_filter_s* h, uint32_t t, uint32_t t_end);
int ensure_y(smc_handle h, int64_t T);
int ensure_recs(smc_handle h, int64_t T);
int emit_if_needed(smc_handle h);
// closes the timed region opened at ev0 (records ev1, waits for the stream, stores the elapsed time in last_ms) and hands the
// requested per-filter vectors over from the pinned mirror
int finish_elapsed(smc_handle h, double* logZ = nullptr, double* logmu = nullptr, double* ess = nullptr);
// smc_capi_series.hip
// (y_host: the host copy of the series in h->d_y, alive until the launches are enqueued, or nullptr)
int enqueue_log_likelihood(smc_handle h, double y0, int64_t T, bool want_trace, bool summ = false, const double* y_host = nullptr);
// smc_capi_summ.hip: the per-step summaries of the multi-step calls
inline bool summaries_on(const smc_filter_s* h) { return h->summ.np > 0 || h->summ.mom != 0; }
bool summaries_fit_lds(const smc_filter_s* h);
int ensure_summaries(smc_handle h, int64_t T);
void view_summaries(smc_handle h);
int enqueue_step_summaries(smc_handle h, int64_t row);
// ... and the weighted summaries of another cloud [rows][ntheta][npad] under the handle's current weights (forecasts)
size_t cloud_summary_words(const smc_filter_s* h, int rows);
int enqueue_cloud_summaries(smc_handle h, const double* cloud, int rows, uint64_t* scratch, int scratch_rows, int component, const double* p, int np,
                            bool mom, double* q_out, double* mean, double* var);
// smc_capi_summ.hip: predictive checks (smc_spec.h "predictive checks").  predictive_refuse: the handles whose cloud is no predictive
// sample (SMC_EINVAL with the reason; SMC_OK otherwise).  predictive_run: the rows of T clouds read through the strides (st_t, st_c,
// st_f; smc_pred_kernels.h) with the observations y [T] on the host (nullptr: T = 1 and y0), on the handle's stream, waited for and
// handed over as pit, obs_mean, obs_var [T][ntheta] (any NULL).  It reads the handle's parameter rows and touches nothing else.
int predictive_refuse(const smc_filter_s* h, const char* who);
int predictive_run(smc_handle h, const char* who, const double* x, int64_t st_t, int64_t st_c, int64_t st_f, int64_t T, const double* y, double y0,
                   double* pit, double* obs_mean, double* obs_var);
// smc_capi_slots.hip: the dense weights of the current state into w [ntheta][n], on the handle's stream (k_dense_weights)
hipError_t enqueue_dense_weights(smc_filter_s* h, double* w);
// ... and the block smc_get_state and smc_get_moments put them (and the moments behind them) in: h->d_wdense, allocated once
int ensure_wdense(smc_handle h);
// smc_capi_smooth.hip: appends the state smc_init / smc_step leave to the record of an armed handle (no host synchronisation);
// the calls that would change the state of an armed handle without a recordable step refuse with history_refuse()
int history_append(smc_handle h);
void history_free(smc_filter_s* h);   // (frees the record and every block over it: the handle is disarmed)
inline bool history_armed(const smc_filter_s* h) { return h->hist.armed; }
int history_refuse(const char* who);
// smc_capi_smooth.hip: the two launches of smc_ancestor_sweep (smc_anc_kernels.h) over the record, on the handle's stream; its
// refusals are the caller's (smc_capi_cond.hip).  Where the results lie in h->cond.d_sweep: J, idx [T][ntheta], dead [ntheta]
int ancestor_sweep_enqueue(smc_handle h, uint64_t path_seed, const int32_t** d_J, const int32_t** d_idx, const int** d_dead);
// smc_capi_slots.hip: k_copy_slots on stream s (slot th of dst <- slot th of src where mask[th])
hipError_t copy_slots(const smc::FilterView& dst, int dcur, const smc::FilterView& src, int scur, int d, const unsigned char* mask, hipStream_t s);

#pragma GCC visibility pop
