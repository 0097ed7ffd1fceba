// smc_capi_summ.hip -- summaries of the particle clouds: quantiles and moments per step inside the multi-step calls
// (smc_set_summaries / smc_get_summaries) and of the current state (smc_get_moments / smc_get_quantiles).
// The only translation unit that includes smc_summ_kernels.h.  Predictive checks of the clouds (smc_get_predictive, and predictive_run
// behind smc_predictive): the kernels of smc_pred_kernels.h over the handle's clouds.
#include "smc_host.h"
#include "smc_summ_kernels.h"
#include "smc_pred_kernels.h"

#include <cstdlib>
#include <cstring>
#include <limits>

using namespace smc;

// ---- per-step summaries inside the multi-step calls ------------------------------------------------------------------
// whether the LDS-resident kernels have room for the summaries' histograms next to the filter's state (160 KiB per workgroup)
bool summaries_fit_lds(const smc_filter_s* h) {
    return (size_t)lds_padded_len(h->v.seg) * 8 * (size_t)(1 + h->d) + scr_words(1024, 4) * 8 + summary_lds_words(h->summ.np, h->d) * 8 <= (size_t)160 * 1024;
}
int ensure_summaries(smc_handle h, int64_t T) {
    if (T > h->summ.cap) {   // (the two traces grow together: old blocks first)
        HIPCHK(hipStreamSynchronize(h->stream));
        h->summ.d_q.reset(); h->summ.d_m.reset();
        h->summ.cap = 0;
        HIPCHK(h->summ.d_q.grow((size_t)T * h->v.ntheta * QMAX * 8));
        HIPCHK(h->summ.d_m.grow((size_t)T * 2 * h->d * h->v.ntheta * 8));
        h->summ.cap = T;
    }
    return SMC_OK;
}
// what the launches of a multi-step call need to know about the summaries (the scope of the call resets it)
void view_summaries(smc_handle h) {
    FilterView& v = h->v;
    v.sum_np = h->summ.np; v.sum_comp = h->summ.comp; v.sum_mom = h->summ.mom;
    for (int j = 0; j < QMAX; ++j) v.sum_p64[j] = h->summ.mode == SMC_SUMM_UNWEIGHTED ? d2bits(h->summ.p[j]) : h->summ.p64[j];
    v.sum_q = h->summ.d_q.as<double>(); v.sum_m = h->summ.d_m.as<double>();
}
// the levels of a request in the form the kernels of the handle's mode read (FilterView::sum_p64)
static void level_words(const smc_filter_s* h, const double* p, int np, uint64_t* out) {
    for (int j = 0; j < QMAX; ++j) out[j] = j >= np ? 0 : h->summ.mode == SMC_SUMM_UNWEIGHTED ? d2bits(q7_level(p[j])) : prob_to_u64(p[j]);
}
// The summaries of the CURRENT weights of filters of any size, enqueued on the handle's stream behind the launch that produced
// them (no host synchronisation): smc_summ_kernels.h.  q_out [ntheta][np], mean / var [d][ntheta] are device pointers.  The
// weights must have been emitted (last_K, last_D describe them).
static int ensure_ms(smc_handle h) {
    const size_t nth = (size_t)h->v.ntheta, words = ms_words(nth, (size_t)h->v.nseg, (size_t)h->d);
    if (!h->summ.d_ms) {
        HIPCHK(h->summ.d_ms.grow((words + nth * QMAX) * 8));
        HIPCHK(hipMemsetAsync(h->summ.d_ms.as<uint64_t>(), 0, (words + nth * QMAX) * 8, h->stream));
    }
    return SMC_OK;
}
// v: the view whose sum_* fields name the request and whose x[cur] points at the cloud, `rows` state rows [rows][ntheta][npad] under
// the handle's current weights; ms: scratch carved for `rows` rows
template <bool UNW>
static int enqueue_ms_view(smc_handle h, const FilterView& v, int rows, const MsScratch& ms, double* q_out, double* mean, double* var) {
    const int np = v.sum_np;
    const bool mom = v.sum_mom != 0;
    // streaming kernels: workgroups of 1024 threads over consecutive segments - about 256 workgroups in all for the passes that
    // only read, about 64 for the histogram (every workgroup flushes its occupied bins with device-scope atomics)
    auto groups = [&](int want) {
        int g = want / h->v.ntheta;
        g = g < 1 ? 1 : g;
        return g > h->v.nseg ? h->v.nseg : g;
    };
    const int g_read = groups(256), g_hist = groups(64);
    hipLaunchKernelGGL(k_ms_range<UNW>, dim3(g_read, h->v.ntheta), dim3(MS_STREAM), 0, h->stream, v, h->cur, rows, ms);
    if (np > 0) hipLaunchKernelGGL(k_ms_hist<UNW>, dim3(g_hist, h->v.ntheta), dim3(MS_STREAM), 0, h->stream, v, h->cur, g_read, ms);
    hipLaunchKernelGGL(k_ms_pick<UNW>, dim3(h->v.ntheta), dim3(MS_THREADS), 0, h->stream, v, rows, g_read, ms, q_out, mean);
    if (mom) {   // the variance centred on that mean: a second read of the cloud
        hipLaunchKernelGGL(k_ms_center<UNW>, dim3(g_read, h->v.ntheta), dim3(MS_STREAM), 0, h->stream, v, h->cur, rows, ms, (const double*)mean);
        hipLaunchKernelGGL(k_ms_var<UNW>, dim3(h->v.ntheta), dim3(MS_THREADS), 0, h->stream, v, rows, g_read, ms, var);
    }
    int64_t two_level = MS_TWO_LEVEL;
    if (const char* e = getenv("SMC_MS_TWO_LEVEL")) two_level = atoll(e);   // tuning / test knob: results do not depend on it
    if (np > 0 && h->v.n > two_level) {   // big filters: the chosen bins cut a second time before the candidates are collected
        hipLaunchKernelGGL(k_ms_hist2<UNW>, dim3(g_read, h->v.ntheta), dim3(MS_STREAM), 0, h->stream, v, h->cur, ms);
        hipLaunchKernelGGL(k_ms_pick2, dim3(np, h->v.ntheta), dim3(MS_THREADS), 0, h->stream, v, ms);
        hipLaunchKernelGGL((k_ms_collect<true, UNW>), dim3(g_read, h->v.ntheta), dim3(MS_STREAM), 0, h->stream, v, h->cur, ms);
    } else if (np > 0) {
        hipLaunchKernelGGL((k_ms_collect<false, UNW>), dim3(g_read, h->v.ntheta), dim3(MS_STREAM), 0, h->stream, v, h->cur, ms);
    }
    if (np > 0) {
        hipLaunchKernelGGL(k_ms_select<UNW>, dim3(np, h->v.ntheta), dim3(MS_SEL_THREADS), 0, h->stream, v, h->cur, ms, q_out);
        if (UNW) {   // the neighbour x_(j+1) of every level, then the interpolation
            hipLaunchKernelGGL(k_ms_succ, dim3(g_read, h->v.ntheta), dim3(MS_STREAM), 0, h->stream, v, h->cur, ms);
            hipLaunchKernelGGL(k_ms_interp, dim3(h->v.ntheta), dim3(WAVE), 0, h->stream, v, ms, q_out);
        }
    }
    HIPCHK(hipGetLastError());
    return SMC_OK;
}
// the request as a view of the handle: levels p64 of `component`, moments or not
static FilterView summary_view(const smc_filter_s* h, int component, int np, const uint64_t* p64, bool mom) {
    FilterView v = h->v;
    v.sum_np = np; v.sum_comp = np > 0 ? component : 0; v.sum_mom = mom ? 1 : 0;
    for (int j = 0; j < QMAX; ++j) v.sum_p64[j] = j < np ? p64[j] : 0;
    return v;
}
template <bool UNW>
static int enqueue_ms_t(smc_handle h, int component, int np, const uint64_t* p64, bool mom, double* q_out, double* mean, double* var) {
    const size_t nth = (size_t)h->v.ntheta;
    int rc = ensure_ms(h);
    if (rc) return rc;
    const MsScratch ms = ms_carve(h->summ.d_ms.as<uint64_t>(), nth, (size_t)h->v.nseg, (size_t)h->d);
    return enqueue_ms_view<UNW>(h, summary_view(h, component, np, p64, mom), h->d, ms, q_out, mean, var);
}
// The WEIGHTED summaries (whatever the handle's summary mode) of another cloud under the handle's current weights: `rows` <= MAX_DIM
// rows [rows][ntheta][npad] on the device, e.g. one horizon of a forecast (smc_capi_forecast.hip).  scratch: cloud_summary_words(h,
// scratch_rows) words, scratch_rows >= rows, zeroed once by the caller and always carved for scratch_rows (the kernels leave their
// histograms and counters zeroed for the next request only where THIS carving keeps them); results as enqueue_ms leaves them
// (device pointers; q_out [ntheta][np], mean / var [rows][ntheta]).
size_t cloud_summary_words(const smc_filter_s* h, int rows) { return ms_words((size_t)h->v.ntheta, (size_t)h->v.nseg, (size_t)rows); }
int enqueue_cloud_summaries(smc_handle h, const double* cloud, int rows, uint64_t* scratch, int scratch_rows, int component, const double* p, int np,
                            bool mom, double* q_out, double* mean, double* var) {
    if (rows < 1 || rows > MAX_DIM || rows > scratch_rows || np < 0 || np > QMAX) return fail(SMC_EINVAL, "cloud summaries: rows / levels out of range");
    uint64_t pw[QMAX];
    for (int j = 0; j < QMAX; ++j) pw[j] = j < np ? prob_to_u64(p[j]) : 0;
    FilterView v = summary_view(h, component, np, pw, mom);
    v.sum_unw = 0;
    v.x[h->cur] = const_cast<double*>(cloud);   // (the summary kernels only read it)
    const MsScratch ms = ms_carve(scratch, (size_t)h->v.ntheta, (size_t)h->v.nseg, (size_t)scratch_rows);
    return enqueue_ms_view<false>(h, v, rows, ms, q_out, mean, var);
}
static int enqueue_ms(smc_handle h, int component, int np, const uint64_t* p64, bool mom, double* q_out, double* mean, double* var) {
    return h->summ.mode == SMC_SUMM_UNWEIGHTED ? enqueue_ms_t<true>(h, component, np, p64, mom, q_out, mean, var)
                                              : enqueue_ms_t<false>(h, component, np, p64, mom, q_out, mean, var);
}
// ... into row `row` of the traces of a multi-step call
int enqueue_step_summaries(smc_handle h, int64_t row) {
    const size_t nth = (size_t)h->v.ntheta, nout = (size_t)h->d * nth;
    double* mbase = h->summ.d_m.as<double>() + (size_t)row * 2 * nout;
    uint64_t pw[QMAX];
    level_words(h, h->summ.p, h->summ.np, pw);
    return enqueue_ms(h, h->summ.comp, h->summ.np, pw, h->summ.mom != 0, h->summ.d_q.as<double>() + (size_t)row * nth * h->summ.np, mbase, mbase + nout);
}

extern "C" int smc_set_summaries(smc_handle h, int component, const double* p, int np, int moments) {
    if (!h) return fail(SMC_EINVAL, "smc_set_summaries: NULL handle");
    if (np < 0 || np > QMAX || (np > 0 && !p)) return fail(SMC_EINVAL, "smc_set_summaries: 0 <= np <= 8");
    if (np > 0 && (component < 0 || component >= h->d)) return fail(SMC_EINVAL, "smc_set_summaries: component out of range");
    h->summ.np = np; h->summ.comp = np > 0 ? component : 0; h->summ.mom = moments ? 1 : 0;
    for (int j = 0; j < QMAX; ++j) { h->summ.p64[j] = j < np ? prob_to_u64(p[j]) : 0; h->summ.p[j] = j < np ? q7_level(p[j]) : 0.0; }
    h->summ.T = 0;
    return SMC_OK;
}

extern "C" int smc_set_summary_mode(smc_handle h, int mode) {
    if (!h) return fail(SMC_EINVAL, "smc_set_summary_mode: NULL handle");
    if (mode != SMC_SUMM_WEIGHTED && mode != SMC_SUMM_UNWEIGHTED) return fail(SMC_EINVAL, "smc_set_summary_mode: unknown mode");
    h->summ.mode = mode;
    h->v.sum_unw = mode == SMC_SUMM_UNWEIGHTED ? 1 : 0;
    h->summ.T = 0;   // (rows recorded in the other mode are not handed out as this one's)
    return SMC_OK;
}

extern "C" int smc_get_summaries(smc_handle h, int64_t T, double* q, double* mean, double* var) {
    if (!h) return fail(SMC_EINVAL, "smc_get_summaries: NULL handle");
    if (T < 1 || T > h->summ.T) return fail(SMC_ESTATE, "smc_get_summaries: more steps than the last multi-step call recorded");
    if ((q && h->summ.np == 0) || ((mean || var) && !h->summ.mom)) return fail(SMC_ESTATE, "smc_get_summaries: not recorded (smc_set_summaries)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t nth = (size_t)h->v.ntheta, nout = (size_t)h->d * nth;
    if (q) HIPCHK(hipMemcpy(q, h->summ.d_q.as<double>(), (size_t)T * nth * h->summ.np * 8, hipMemcpyDeviceToHost));
    if (mean) HIPCHK(hipMemcpy2D(mean, nout * 8, h->summ.d_m.as<double>(), 2 * nout * 8, nout * 8, (size_t)T, hipMemcpyDeviceToHost));
    if (var) HIPCHK(hipMemcpy2D(var, nout * 8, h->summ.d_m.as<double>() + nout, 2 * nout * 8, nout * 8, (size_t)T, hipMemcpyDeviceToHost));
    if (!h->summ.skip.empty()) {   // filters the call left out have no summaries: NaN (the device rows hold whatever was there)
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (size_t m = 0; m < nth; ++m) {
            if (!h->summ.skip[m]) continue;
            for (int64_t t = 0; t < T; ++t) {
                if (q) for (int j = 0; j < h->summ.np; ++j) q[((size_t)t * nth + m) * h->summ.np + j] = nan;
                for (int c = 0; c < h->d; ++c) {
                    if (mean) mean[(size_t)t * nout + (size_t)c * nth + m] = nan;
                    if (var) var[(size_t)t * nout + (size_t)c * nth + m] = nan;
                }
            }
        }
    }
    return SMC_OK;
}

// Quantiles and / or moments of the CURRENT state of single-segment filters in ONE launch that writes to pinned host memory
// (the README loop asks for them after every bootstrap_filter!: one launch and one synchronisation per request instead of
// sixteen launches and a copy).  done = false: no such kernel for this handle (several segments, or the state does not fit LDS).
static int summaries_once(smc_handle h, int component, const double* p, int np, bool mom, double* q_out, double* mean, double* var, bool& done) {
    done = false;
    if (h->v.nseg != 1) return SMC_OK;
    const size_t nth = (size_t)h->v.ntheta, nout = (size_t)h->d * nth;
    HIPCHK(h->summ.h_once.grow(((size_t)QMAX * nth + 2 * nout) * 8));
    double* once = h->summ.h_once.as<double>();
    FilterView v = h->v;
    v.sum_np = np; v.sum_comp = component; v.sum_mom = mom ? 1 : 0;
    level_words(h, p, np, v.sum_p64);
    v.sum_q = once; v.sum_m = once + (size_t)QMAX * nth;
    const hipError_t e = by_variant<ENTRY_SUMM_ONCE>(h->model, VARIANT_PLAIN, [&](auto L) { return L.summ_once(v, h->cur, h->stream); });
    if (e == hipErrorInvalidValue) return SMC_OK;
    HIPCHK(e);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (q_out) memcpy(q_out, once, nth * np * 8);
    if (mean) memcpy(mean, once + (size_t)QMAX * nth, nout * 8);
    if (var) memcpy(var, once + (size_t)QMAX * nth + nout, nout * 8);
    done = true;
    return SMC_OK;
}

extern "C" int smc_get_moments(smc_handle h, double* mean, double* var) {
    if (!h || !mean || !var) return fail(SMC_EINVAL, "smc_get_moments: NULL argument");
    if (!h->inited) return fail(SMC_ESTATE, "smc_get_moments: filter not initialised");
    HIPCHK(hipSetDevice(h->device));
    int rc = emit_if_needed(h);
    if (rc) return rc;
    bool done = false;
    if ((rc = summaries_once(h, 0, nullptr, 0, true, nullptr, mean, var, done)) || done) return rc;
    const size_t nout = (size_t)h->d * h->v.ntheta;
    if ((rc = ensure_wdense(h))) return rc;
    double *d_mean = h->d_wdense.as<double>(), *d_var = d_mean + nout;
    if ((rc = enqueue_ms(h, 0, 0, nullptr, true, nullptr, d_mean, d_var))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(mean, d_mean, nout * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(var, d_var, nout * 8, hipMemcpyDeviceToHost));
    return SMC_OK;
}

// ---- predictive checks (smc_spec.h "predictive checks"; kernels and their order of summation: smc_pred_kernels.h) ----------------
// The size at which the launches change: clouds of at most this many particles are finished by one workgroup each (k_predictive),
// larger ones by tiles and one launch per level.  PRED_SMALL_MAX = 128^2 is the most the one-workgroup kernel can hold.  Measured
// (profiles/predictive_cost.log, smc_get_predictive of 1 and of 64 clouds): one workgroup wins up to 2048 particles (13 against 18 us),
// the two meet at 4096 (21 against 20 to 22 us), the launches per level win from 8192 on (36 to 38 against 24 to 33 us): the switch
// is 4096.  SMC_PRED_SMALL_MAX in the environment moves it within [0, 128^2] (tests and measurements: the same bits either way).
constexpr int64_t PRED_SWITCH = 4096;
static int64_t pred_small_max() {
    const char* e = getenv("SMC_PRED_SMALL_MAX");
    if (!e || !*e) return PRED_SWITCH;
    const long long v = atoll(e);
    return v < 0 ? 0 : v > PRED_SMALL_MAX ? PRED_SMALL_MAX : (int64_t)v;
}
extern "C" int smc_predictive_info(int64_t* small_max, int* chunk) {
    if (small_max) *small_max = pred_small_max();
    if (chunk) *chunk = SMOOTH_CH;
    return SMC_OK;
}

int predictive_refuse(const smc_filter_s* h, const char* who) {
    const std::string w = std::string(who) + ": ";
    if (h->v.prop_kind != 0)
        return fail(SMC_EINVAL, w + "the handle has a proposal (smc_set_proposal): its cloud is drawn from the proposal and is not a sample of the "
                                    "predictive law of the state");
    if (conditional(h))
        return fail(SMC_EINVAL, w + "the handle is conditional (SMC_FLAG_CONDITIONAL): its cloud holds the pinned reference and is not a predictive sample");
    if (!has_density(h->model))
        return fail(SMC_EINVAL, w + "SMC_MODEL_UCSV_RB keeps the UPDATED m and P in its rows: the predictive pair of the trend is gone when the step "
                                    "ends; use a UCSV3D filter");
    return SMC_OK;
}

int predictive_run(smc_handle h, const char* who, const double* x, int64_t st_t, int64_t st_c, int64_t st_f, int64_t T, const double* y, double y0,
                   double* pit, double* obs_mean, double* obs_var) {
    const std::string w = std::string(who) + ": ";
    const int64_t n = h->v.n, nt = h->v.ntheta, rows = T * nt;
    const int64_t nch = (n + SMOOTH_CH - 1) / SMOOTH_CH, ntiles = (n + PRED_THREADS - 1) / PRED_THREADS;
    const bool small = n <= pred_small_max();
    if (small ? (nt > 65535 || T > 0x7fffffff) : ((double)ntiles * (double)rows > 2147483647.0))
        return fail(SMC_EINVAL, w + "too many clouds for one launch");
    // the block: y | out [3][rows] | large clouds: the partials of level 0 [4][rows][nch] and of the level above [4][rows][ceil(nch / CH)]
    const int64_t m1 = (nch + SMOOTH_CH - 1) / SMOOTH_CH;
    OffsetPlan o;
    const size_t o_y = o.take((size_t)T * 8), o_out = o.take(3 * (size_t)rows * 8);
    const size_t o_a = small ? 0 : o.take(4 * (size_t)rows * (size_t)nch * 8), o_b = small ? 0 : o.take(4 * (size_t)rows * (size_t)m1 * 8);
    if (h->pred.d_buf.bytes() < o.bytes) {
        if (h->pred.d_buf) HIPCHK(hipStreamSynchronize(h->stream));   // (the old block first; the stream may still read it)
        if (h->pred.d_buf.grow(o.bytes) != hipSuccess) return fail(SMC_ENOMEM, w + "hipMalloc of the block of the predictive checks");
    }
    char* buf = h->pred.d_buf.as<char>();
    double *d_y = (double*)(buf + o_y), *d_out = (double*)(buf + o_out), *A = (double*)(buf + o_a), *B = (double*)(buf + o_b);
    // one step (smc_get_predictive, once per step of a filter loop): the rows go straight into pinned host memory, as the one-launch
    // summaries of the current state do - no copy behind the synchronisation
    const bool pinned = T == 1;
    if (pinned) {
        HIPCHK(h->pred.h_out.grow(3 * (size_t)rows * 8));
        d_out = h->pred.h_out.as<double>();
    }
    hipStream_t s = h->stream;
    HIPCHK(hipEventRecord(h->ev0, s));   // (smc_last_elapsed_ms: the launches of this call)
    if (y) HIPCHK(hipMemcpyAsync(d_y, y, (size_t)T * 8, hipMemcpyHostToDevice, s));
    PredArgs a{};
    a.x = x; a.st_t = st_t; a.st_c = st_c; a.st_f = st_f; a.n = n; a.ntheta = (int)nt; a.ntiles = ntiles;
    a.params = h->d_params; a.y = y ? d_y : nullptr; a.y0 = y0; a.out = d_out;
    HIPCHK(by_density_model(h->model, [&](auto Mt) {
        constexpr int M = decltype(Mt)::value;
        if (small) {
            hipLaunchKernelGGL(k_predictive<M>, dim3((unsigned)T, (unsigned)nt), dim3(PRED_THREADS), 0, s, a);
            return hipGetLastError();
        }
        // `planes` lines of sums, from the partials of level 0 at `from` down to one number a line; where they end up
        auto levels = [&](double* from, double* other, int64_t planes, const double** done) {
            int64_t m = nch;
            while (m > 1) {
                const int64_t mo = (m + SMOOTH_CH - 1) / SMOOTH_CH, lines = planes * rows;
                hipLaunchKernelGGL(k_pred_level<SMOOTH_CH>, dim3((unsigned)((lines * mo + 255) / 256)), dim3(256), 0, s, (const double*)from, m, other, mo, lines);
                const hipError_t e = hipGetLastError();
                if (e != hipSuccess) return e;
                double* tswap = from; from = other; other = tswap;
                m = mo;
            }
            *done = from;
            return hipSuccess;
        };
        hipError_t e;
        const dim3 grid((unsigned)(ntiles * rows));
        a.part = A;
        hipLaunchKernelGGL((k_predictive_tiles<M, 0>), grid, dim3(PRED_THREADS), 0, s, a, rows);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = levels(A, B, 3, &a.sums)) != hipSuccess) return e;
        // the centred pass: plane 3 of both buffers (the first-pass sums stay where they are)
        double *A3 = A + 3 * rows * nch, *B3 = B + 3 * rows * m1;
        a.part = A3;
        hipLaunchKernelGGL((k_predictive_tiles<M, 1>), grid, dim3(PRED_THREADS), 0, s, a, rows);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = levels(A3, B3, 1, &a.sum_c)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_pred_finish<0>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, a, rows);
        return hipGetLastError();
    }));
    int rc = finish_elapsed(h);
    if (rc) return rc;
    std::vector<double> res;
    const double* r = d_out;
    if (!pinned) {   // (one copy for the three planes)
        res.resize(3 * (size_t)rows);
        HIPCHK(hipMemcpy(res.data(), d_out, res.size() * 8, hipMemcpyDeviceToHost));
        r = res.data();
    }
    if (pit) memcpy(pit, r, (size_t)rows * 8);
    if (obs_mean) memcpy(obs_mean, r + rows, (size_t)rows * 8);
    if (obs_var) memcpy(obs_var, r + 2 * rows, (size_t)rows * 8);
    return SMC_OK;
}

// the row of the CURRENT cloud of every filter for the observation y_t the last step assimilated: read-only on the handle (no weight
// is read, so nothing is emitted either: the steps that follow give the bits they would have given)
extern "C" int smc_get_predictive(smc_handle h, double y_t, double* pit, double* obs_mean, double* obs_var) {
    if (!h) return fail(SMC_EINVAL, "smc_get_predictive: NULL handle");
    int rc = predictive_refuse(h, "smc_get_predictive");
    if (rc) return rc;
    if (!h->inited) return fail(SMC_ESTATE, "smc_get_predictive: filter not initialised");
    HIPCHK(hipSetDevice(h->device));
    const FilterView& v = h->v;
    return predictive_run(h, "smc_get_predictive", v.x[h->cur], 0, (int64_t)v.ntheta * v.npad, v.npad, 1, nullptr, y_t, pit, obs_mean, obs_var);
}

extern "C" int smc_get_quantiles(smc_handle h, int component, const double* p, int np, double* out) {
    if (!h || !p || !out) return fail(SMC_EINVAL, "smc_get_quantiles: NULL argument");
    if (!h->inited) return fail(SMC_ESTATE, "smc_get_quantiles: filter not initialised");
    if (component < 0 || component >= h->d) return fail(SMC_EINVAL, "smc_get_quantiles: component out of range");
    if (np < 1 || np > QMAX) return fail(SMC_EINVAL, "smc_get_quantiles: 1 <= np <= 8");
    HIPCHK(hipSetDevice(h->device));
    int rc = emit_if_needed(h);
    if (rc) return rc;
    bool done = false;
    if ((rc = summaries_once(h, component, p, np, false, out, nullptr, nullptr, done)) || done) return rc;
    const size_t nth = (size_t)h->v.ntheta, nst = nth * np;
    uint64_t hp[QMAX];
    level_words(h, p, np, hp);
    if ((rc = ensure_ms(h))) return rc;
    double* d_out = (double*)(h->summ.d_ms.as<uint64_t>() + ms_words(nth, (size_t)h->v.nseg, (size_t)h->d));
    if ((rc = enqueue_ms(h, component, np, hp, false, d_out, nullptr, nullptr))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, d_out, nst * 8, hipMemcpyDeviceToHost));
    return SMC_OK;
}
