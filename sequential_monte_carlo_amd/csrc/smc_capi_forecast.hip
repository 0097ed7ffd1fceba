// smc_capi_forecast.hip -- forecasts: the filtered cloud propagated H steps past the last observation (smc_spec.h "forecasts").
// smc_forecast summarises every horizon on the device under the handle's current weights (the streaming summary kernels of
// smc_capi_summ.hip, pointed at one horizon of the propagated cloud); smc_forecast_cloud hands the clouds themselves over.
// The kernel: smc_forecast_kernels.h, instantiated per family by smc_model.hip (the plain objects) and reached through by_variant.
#include "smc_host.h"

#include <cstdlib>
#include <cstring>
#include <vector>

using namespace smc;

// horizons propagated per launch: the clouds of one block are summarised (or copied out) before the next block overwrites them,
// so the scratch stays bounded whatever H.  Shorter for big batches (FORECAST_BYTES of clouds at most, one horizon at least);
// SMC_FORECAST_BLOCK overrides it at the call (tuning / test knob: results do not depend on it).
constexpr int FORECAST_BLOCK = 8;
constexpr size_t FORECAST_BYTES = (size_t)512 << 20;

namespace {
struct Plan {
    int rows = 0, block = 0;   // d + 3 | horizons per launch
    int ms_rows = 0;           // rows the summary scratch is carved for: the state rows or the three observation rows, whichever is more
    size_t plane = 0;          // doubles of one row of every filter: ntheta * npad
    size_t res_per = 0;        // doubles of one horizon's results: q [ntheta][QMAX] | mean, var [d][ntheta] | obs q | obs mean, var [3][ntheta]
    size_t off_ms = 0, off_res = 0, bytes = 0;
};
Plan make_plan(const smc_filter_s* h, int64_t H, bool summaries) {
    Plan p;
    const size_t nth = (size_t)h->v.ntheta;
    p.rows = h->d + 3;
    p.ms_rows = h->d > 3 ? h->d : 3;
    p.plane = nth * (size_t)h->v.npad;
    const size_t per = (size_t)p.rows * p.plane * 8;
    int64_t b = FORECAST_BLOCK;
    while (b > 1 && (size_t)b * per > FORECAST_BYTES) --b;
    if (const char* e = getenv("SMC_FORECAST_BLOCK")) {
        const long long want = atoll(e);
        if (want >= 1) b = want;
    }
    p.block = (int)(b < H ? b : H);
    OffsetPlan o;
    (void)o.take((size_t)p.block * per);
    p.res_per = nth * (size_t)(2 * QMAX + 2 * h->d + 6);
    if (summaries) {
        p.off_ms = o.take(cloud_summary_words(h, p.ms_rows) * 8);
        p.off_res = o.take((size_t)H * p.res_per * 8);
    }
    p.bytes = o.bytes;
    return p;
}
}  // namespace

// the handle's forecast block holds `bytes`: grown on demand (old block first); SMC_ENOMEM leaves the handle without one, otherwise as it was
static int ensure_forecast(smc_handle h, size_t bytes) {
    if (bytes <= h->fc.d_buf.bytes()) return SMC_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->fc.d_buf.grow(bytes) != hipSuccess)
        return fail(SMC_ENOMEM, "forecast: out of device memory for the propagated clouds (" + std::to_string(bytes) + " bytes); a smaller SMC_FORECAST_BLOCK needs less");
    return SMC_OK;
}

// horizons k0 .. k0 + nk - 1 (1-based) into the block's clouds, from the handle's state (k0 == 1) or from the last horizon of the
// block before
static int enqueue_forecast_block(smc_handle h, const Plan& p, uint64_t seed, int64_t k0, int nk, int nk_prev) {
    double* out = h->fc.d_buf.as<double>();
    const double* src = k0 == 1 ? h->v.x[h->cur] : out + (size_t)(nk_prev - 1) * p.rows * p.plane;
    HIPCHK(by_variant<ENTRY_FORECAST>(h->model, VARIANT_PLAIN, [&](auto L) { return L.forecast(h->v, h->geo, src, seed, (uint32_t)k0, nk, out, h->stream); }));
    return SMC_OK;
}

extern "C" int smc_forecast(smc_handle h, int64_t H, uint64_t forecast_seed, int component, const double* p, int np, double* mean, double* var,
                            double* q, double* obs_mean, double* obs_var, double* obs_q) {
    if (!h) return fail(SMC_EINVAL, "smc_forecast: NULL handle");
    if (!h->inited) return fail(SMC_ESTATE, "smc_forecast: filter not initialised");
    if (H < 1 || H > 0x7fffffff) return fail(SMC_EINVAL, "smc_forecast: H >= 1");
    if (np < 0 || np > QMAX) return fail(SMC_EINVAL, "smc_forecast: 0 <= np <= 8");
    if (np > 0 && !p) return fail(SMC_EINVAL, "smc_forecast: np > 0 needs the levels p");
    if (np > 0 && (component < 0 || component >= h->d)) return fail(SMC_EINVAL, "smc_forecast: component out of range");
    HIPCHK(hipSetDevice(h->device));
    int rc = emit_if_needed(h);
    if (rc) return rc;
    const Plan pl = make_plan(h, H, true);
    if ((rc = ensure_forecast(h, pl.bytes))) return rc;
    const size_t nth = (size_t)h->v.ntheta, d = (size_t)h->d;
    const bool want_q = np > 0 && q, want_oq = np > 0 && obs_q, want_m = mean || var, want_om = obs_mean || obs_var;
    uint64_t* ms = (uint64_t*)(h->fc.d_buf.as<char>() + pl.off_ms);
    double* res = (double*)(h->fc.d_buf.as<char>() + pl.off_res);
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    // (the summary kernels want their histograms and counters zero and leave them so: once per call is enough, and cheap)
    HIPCHK(hipMemsetAsync(ms, 0, pl.off_res - pl.off_ms, h->stream));
    int nk_prev = 0;
    for (int64_t k0 = 1; k0 <= H; k0 += pl.block) {
        const int nk = (int)(H - k0 + 1 < pl.block ? H - k0 + 1 : pl.block);
        if ((rc = enqueue_forecast_block(h, pl, forecast_seed, k0, nk, nk_prev))) return rc;
        nk_prev = nk;
        for (int j = 0; j < nk; ++j) {
            const double* cloud = h->fc.d_buf.as<double>() + (size_t)j * pl.rows * pl.plane;
            double* r = res + (size_t)(k0 - 1 + j) * pl.res_per;
            double *r_q = r, *r_m = r_q + nth * QMAX, *r_v = r_m + d * nth, *r_oq = r_v + d * nth, *r_om = r_oq + nth * QMAX, *r_ov = r_om + 3 * nth;
            if ((want_q || want_m) && (rc = enqueue_cloud_summaries(h, cloud, h->d, ms, pl.ms_rows, component, p, want_q ? np : 0, want_m, r_q, r_m, r_v))) return rc;
            // the observation rows (yf, ym, yv): quantiles of the draws yf; mean of ym, and variance of ym + mean of yv
            if ((want_oq || want_om) && (rc = enqueue_cloud_summaries(h, cloud + d * pl.plane, 3, ms, pl.ms_rows, 0, p, want_oq ? np : 0, want_om, r_oq, r_om, r_ov))) return rc;
        }
    }
    if ((rc = finish_elapsed(h))) return rc;
    std::vector<double> host((size_t)H * pl.res_per);
    HIPCHK(hipMemcpy(host.data(), res, host.size() * 8, hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < H; ++k) {
        const double* r = host.data() + (size_t)k * pl.res_per;
        const double *r_q = r, *r_m = r_q + nth * QMAX, *r_v = r_m + d * nth, *r_oq = r_v + d * nth, *r_om = r_oq + nth * QMAX, *r_ov = r_om + 3 * nth;
        if (want_q) memcpy(q + (size_t)k * nth * np, r_q, nth * np * 8);
        if (want_oq) memcpy(obs_q + (size_t)k * nth * np, r_oq, nth * np * 8);
        if (mean) memcpy(mean + (size_t)k * d * nth, r_m, d * nth * 8);
        if (var) memcpy(var + (size_t)k * d * nth, r_v, d * nth * 8);
        for (size_t m = 0; m < nth; ++m) {
            if (obs_mean) obs_mean[(size_t)k * nth + m] = r_om[nth + m];                         // sum w ym
            if (obs_var) obs_var[(size_t)k * nth + m] = r_om[2 * nth + m] + r_ov[nth + m];       // within (sum w yv) + between
        }
    }
    return SMC_OK;
}

extern "C" int smc_forecast_cloud(smc_handle h, int64_t H, uint64_t forecast_seed, double* xf, double* yf) {
    if (!h) return fail(SMC_EINVAL, "smc_forecast_cloud: NULL handle");
    if (!h->inited) return fail(SMC_ESTATE, "smc_forecast_cloud: filter not initialised");
    if (H < 1 || H > 0x7fffffff) return fail(SMC_EINVAL, "smc_forecast_cloud: H >= 1");
    HIPCHK(hipSetDevice(h->device));
    const Plan pl = make_plan(h, H, false);
    int rc = ensure_forecast(h, pl.bytes);
    if (rc) return rc;
    const FilterView& v = h->v;
    const size_t nth = (size_t)v.ntheta, d = (size_t)h->d, n = (size_t)v.n;
    double total_ms = 0.0;
    int nk_prev = 0;
    for (int64_t k0 = 1; k0 <= H; k0 += pl.block) {
        const int nk = (int)(H - k0 + 1 < pl.block ? H - k0 + 1 : pl.block);
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        if ((rc = enqueue_forecast_block(h, pl, forecast_seed, k0, nk, nk_prev))) return rc;
        nk_prev = nk;
        if ((rc = finish_elapsed(h))) return rc;
        total_ms += h->last_ms;
        for (int j = 0; j < nk; ++j) {   // dense rows out of the padded ones, as smc_get_state copies x
            const double* cloud = h->fc.d_buf.as<double>() + (size_t)j * pl.rows * pl.plane;
            const size_t k = (size_t)(k0 - 1 + j);
            if (xf) HIPCHK(hipMemcpy2D(xf + k * d * nth * n, n * 8, cloud, (size_t)v.npad * 8, n * 8, d * nth, hipMemcpyDeviceToHost));
            if (yf) HIPCHK(hipMemcpy2D(yf + k * nth * n, n * 8, cloud + d * pl.plane, (size_t)v.npad * 8, n * 8, nth, hipMemcpyDeviceToHost));
        }
    }
    h->last_ms = total_ms;
    return SMC_OK;
}
