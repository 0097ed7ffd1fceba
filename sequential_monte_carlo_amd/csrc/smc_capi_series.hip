// smc_capi_series.hip -- the whole-series driver: log_likelihood(N, y, model) for every filter of a handle (smc_log_likelihood;
// its launches, enqueue_log_likelihood, also serve the PMMH rejuvenation), and the timing probes of those launches.
#include "smc_host.h"

#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

using namespace smc;

static int ensure_trace(smc_handle h, int64_t T) {   // (the two traces grow together: old blocks first)
    const size_t bytes = (size_t)T * (size_t)h->v.ntheta * 8;
    if (bytes > h->d_tr_logmu.bytes() || bytes > h->d_tr_ess.bytes()) {
        HIPCHK(hipStreamSynchronize(h->stream));
        h->d_tr_logmu.reset(); h->d_tr_ess.reset();
        HIPCHK(h->d_tr_logmu.grow(bytes));
        HIPCHK(h->d_tr_ess.grow(bytes));
    }
    return SMC_OK;
}

// Restores the fields of the view that a whole-series call sets for its launches, on every exit path (an early HIPCHK return
// must not leave the handle accumulating no sum of squares, or pointing at the series)
struct SeriesScope {
    FilterView& v;
    explicit SeriesScope(FilterView& view) : v(view) {}
    ~SeriesScope() { v.want_s2 = 1; v.y = nullptr; v.trace_logmu = nullptr; v.trace_ess = nullptr; v.sum_np = v.sum_mom = 0; v.sum_q = v.sum_m = nullptr; }
};

static hipError_t do_resident(smc_filter_s* h, int T) {   // (gap_y: a flagged handle's series with a NaN in it, GapScope)
    return by_variant<ENTRY_RESIDENT>(h->model, pick_variant(h, ENTRY_RESIDENT, h->gap_y != nullptr),
                                      [&](auto L) { return L.resident(h->v, T, h->d_recs.as<StepRec>(), h->stream); });
}
// The launches of log_likelihood(N, y, model) (particles.jl:132-147) for every filter of the handle, enqueued on
// its stream: nothing here waits for the device.  y must already be in h->d_y (ensure_y + copy by the caller).
int enqueue_log_likelihood(smc_handle h, double y0, int64_t T, bool want_trace, bool summ, const double* y_host) {
    // (systematic resampling with per-step summaries: the LDS-resident summary kernels exist for the default law only)
    const bool resident = h->resident_ok && resident_supported(h->model, h->v.seg) && !(summ && (h->v.systematic || !summaries_fit_lds(h)));
    SeriesScope scope(h->v);
    h->v.y = h->d_y.as<double>();
    h->v.trace_logmu = want_trace ? h->d_tr_logmu.as<double>() : nullptr;
    h->v.trace_ess = want_trace ? h->d_tr_ess.as<double>() : nullptr;
    h->cur = 0;
    h->v.want_s2 = want_trace ? 1 : 0;   // ess_t is read only through the traces; the last step always has it
    int rc = SMC_OK;
    if (summ && resident) view_summaries(h);
    if (summ && !resident) {
        // one launch per step, every step followed by the emission of its (logmu, ess) and by the summary kernels - all on the
        // handle's stream, nothing waits for the device
        h->v.want_s2 = 1;
        HIPCHK(do_init(h, y0));
        h->t = 1; h->inited = true; h->emitted = false;
        if ((rc = emit_if_needed(h))) return rc;
        if ((rc = enqueue_step_summaries(h, 0))) return rc;
        for (int64_t t = 1; t < T; ++t) {
            HIPCHK(ensure_breaks(h, (uint32_t)t, (uint32_t)T));
            HIPCHK(do_step(h, (uint32_t)t, 0, 0.0, y_host));
            h->cur ^= 1; h->t += 1; h->emitted = false;
            if ((rc = emit_if_needed(h))) return rc;
            if ((rc = enqueue_step_summaries(h, t))) return rc;
        }
        return SMC_OK;
    }
    if (resident) {
        HIPCHK(do_resident(h, (int)T));
        h->cur = 0; h->t = (uint32_t)T; h->inited = true; h->emitted = true;
    } else {
        if (T == 1) h->v.want_s2 = 1;
        HIPCHK(do_init(h, y0));
        h->t = 1; h->inited = true; h->emitted = false;
        for (int64_t t = 1; t < T; ++t) {
            const int emit = h->v.want_s2 ? 1 : 2;   // 2: the records of step t-1 carry no sum of squares - (logmu, 0) from the totals alone
            if (t == T - 1) h->v.want_s2 = 1;
            HIPCHK(ensure_breaks(h, (uint32_t)t, (uint32_t)T));
            HIPCHK(do_step(h, (uint32_t)t, emit, 0.0, y_host));
            h->cur ^= 1; h->t += 1;
        }
        h->v.want_s2 = 1;
        rc = emit_if_needed(h);
    }
    return rc;
}

// log_likelihood(N, y, model)   particles.jl:132-147
extern "C" int smc_log_likelihood(smc_handle h, const double* y, int64_t T, double* logZ, double* logmu_trace,
                                  double* ess_trace) {
    if (!h || !y) return fail(SMC_EINVAL, "smc_log_likelihood: NULL argument");
    if (T <= 0) return fail(SMC_EINVAL, "smc_log_likelihood: T must be positive");
    if (conditional(h)) return cond_refuse("smc_log_likelihood");
    if (!h->have_params) return fail(SMC_ESTATE, "smc_log_likelihood: smc_set_params has not been called");
    if (history_armed(h)) return history_refuse("smc_log_likelihood");
    h->win.k = 0;   // an uncommitted window is dropped
    HIPCHK(hipSetDevice(h->device));
    int rc = ensure_y(h, T);
    if (rc) return rc;
    const bool want_trace = logmu_trace || ess_trace;
    if (want_trace && (rc = ensure_trace(h, T))) return rc;
    const bool resident = h->resident_ok && resident_supported(h->model, h->v.seg);
    if (resident && (rc = ensure_recs(h, T))) return rc;
    const bool summ = summaries_on(h);
    if (summ && (rc = ensure_summaries(h, T))) return rc;
    h->summ.T = 0;
    h->summ.skip.clear();
    HIPCHK(hipMemcpyAsync(h->d_y.as<double>(), y, (size_t)T * 8, hipMemcpyHostToDevice, h->stream));
    if (h->skip.on) { h->v.skip = h->skip.d_mask.as<unsigned char>(); h->v.order = h->skip.d_order.as<int32_t>(); h->v.n_active = h->v.order + h->v.ntheta; }
    const int cur0 = h->cur;   // where the state of the filters the call leaves out stays
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    {
        GapScope gaps(h, y, T);
        rc = enqueue_log_likelihood(h, y[0], T, want_trace, summ, y);
    }
    h->v.skip = nullptr; h->v.order = nullptr; h->v.n_active = nullptr;
    if (rc) return rc;
    // the call ends in the other buffer: the skipped filters' untouched state goes with it
    if (h->skip.on && h->cur != cur0) HIPCHK(copy_slots(h->v, h->cur, h->v, cur0, h->d, h->skip.d_mask.as<unsigned char>(), h->stream));
    if (summ) {
        h->summ.T = T;
        if (h->skip.on) h->summ.skip = h->skip.h_mask;
    }
    rc = finish_elapsed(h, logZ);
    if (rc) return rc;
    if (logmu_trace) HIPCHK(hipMemcpy(logmu_trace, h->d_tr_logmu.as<double>(), (size_t)T * h->v.ntheta * 8, hipMemcpyDeviceToHost));
    if (ess_trace) HIPCHK(hipMemcpy(ess_trace, h->d_tr_ess.as<double>(), (size_t)T * h->v.ntheta * 8, hipMemcpyDeviceToHost));
    if (h->skip.on && want_trace) {   // filters the call left out have no steps: NaN in their trace columns
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const size_t nt = (size_t)h->v.ntheta;
        for (size_t m = 0; m < nt; ++m) {
            if (!h->skip.h_mask[m]) continue;
            for (int64_t t = 0; t < T; ++t) {
                if (logmu_trace) logmu_trace[(size_t)t * nt + m] = nan;
                if (ess_trace) ess_trace[(size_t)t * nt + m] = nan;
            }
        }
    }
    return SMC_OK;
}

extern "C" int smc_time_step_kernel(smc_handle h, const double* y, int64_t T, int nsample, double* avg_ms,
                                    double* min_ms) {
    if (!h || !y || T < 2 || nsample < 1) return fail(SMC_EINVAL, "smc_time_step_kernel: bad argument");
    if (conditional(h)) return cond_refuse("smc_time_step_kernel");
    if (!h->have_params) return fail(SMC_ESTATE, "smc_time_step_kernel: smc_set_params has not been called");
    if (history_armed(h)) return history_refuse("smc_time_step_kernel");
    if (series_has_gap(h, y, T)) return fail(SMC_EINVAL, "smc_time_step_kernel: the series holds a NaN and the handle reads NaN as missing (SMC_FLAG_NAN_MISSING); it times the ordinary step");
    h->win.k = 0;   // an uncommitted window is dropped: the call runs a series of its own over the filters and the window's observations
    HIPCHK(hipSetDevice(h->device));
    int rc = ensure_y(h, T);
    if (rc) return rc;
    // a bracket spans G consecutive k_step launches (a step IS one launch): the ~5 us an event pair costs on
    // this stack is amortised over the G launches instead of being charged to one
    const int G = T - 1 >= 512 ? 32 : (T - 1 >= 64 ? 8 : 1);
    if ((int64_t)nsample * G > T - 1) nsample = (int)((T - 1) / G);
    std::vector<hipEvent_t> e0((size_t)nsample), e1((size_t)nsample);
    for (int i = 0; i < nsample; ++i) { HIPCHK(hipEventCreate(&e0[i])); HIPCHK(hipEventCreate(&e1[i])); }
    HIPCHK(hipMemcpyAsync(h->d_y.as<double>(), y, (size_t)T * 8, hipMemcpyHostToDevice, h->stream));
    SeriesScope scope(h->v);
    h->v.y = h->d_y.as<double>(); h->v.trace_logmu = nullptr; h->v.trace_ess = nullptr;
    h->cur = 0;
    h->v.want_s2 = 0;   // exactly the launches of log_likelihood without traces (enqueue_log_likelihood)
    HIPCHK(do_init(h, y[0]));
    h->t = 1; h->inited = true; h->emitted = false;
    const int64_t stride = (T - 1) / nsample;   // >= G
    int k = 0, open_left = 0;
    for (int64_t t = 1; t < T; ++t) {
        const int emit = h->v.want_s2 ? 1 : 2;
        if (t == T - 1) h->v.want_s2 = 1;
        HIPCHK(ensure_breaks(h, (uint32_t)t, (uint32_t)T));
        if (!open_left && k < nsample && ((t - 1) % stride) == (stride - G) / 2) {
            HIPCHK(hipEventRecord(e0[k], h->stream));
            open_left = G;
        }
        HIPCHK(do_step(h, (uint32_t)t, emit, 0.0, y));
        if (open_left && --open_left == 0) { HIPCHK(hipEventRecord(e1[k], h->stream)); ++k; }
        h->cur ^= 1; h->t += 1;
    }
    if (open_left) { HIPCHK(hipEventRecord(e1[k], h->stream)); }   // (cannot happen: every bracket fits its stride)
    h->v.want_s2 = 1;
    rc = emit_if_needed(h);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    double sum = 0.0, mn = 1e30;
    for (int i = 0; i < k; ++i) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0[i], e1[i]));
        sum += ms / G;
        mn = ms / G < mn ? ms / G : mn;
    }
    for (int i = 0; i < nsample; ++i) { (void)hipEventDestroy(e0[i]); (void)hipEventDestroy(e1[i]); }
    if (avg_ms) *avg_ms = k ? sum / k : 0.0;
    if (min_ms) *min_ms = k ? mn : 0.0;
    return SMC_OK;
}

__global__ void k_nop() {}

extern "C" int smc_event_overhead_ms(smc_handle h, int nsample, double* avg_ms) {
    if (!h || !avg_ms || nsample < 1) return fail(SMC_EINVAL, "smc_event_overhead_ms: bad argument");
    HIPCHK(hipSetDevice(h->device));
    std::vector<hipEvent_t> e0((size_t)nsample), e1((size_t)nsample);
    for (int i = 0; i < nsample; ++i) { HIPCHK(hipEventCreate(&e0[i])); HIPCHK(hipEventCreate(&e1[i])); }
    for (int i = 0; i < nsample; ++i) {
        hipLaunchKernelGGL(k_nop, dim3(1), dim3(64), 0, h->stream);   // keeps the stream busy like the real loop does
        HIPCHK(hipEventRecord(e0[i], h->stream));
        HIPCHK(hipEventRecord(e1[i], h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    double sum = 0.0;
    for (int i = 0; i < nsample; ++i) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0[i], e1[i]));
        sum += ms;
        (void)hipEventDestroy(e0[i]); (void)hipEventDestroy(e1[i]);
    }
    *avg_ms = sum / nsample;
    return SMC_OK;
}
