// smc_util.hip -- the entry points that take no filter handle: the scope they all open (DeviceCall, smc_host.h: device, stream,
// memory), stand-alone normalize / resample / Kalman, simulation, and the host (smc_host_*) and device (smc_device_*) probes of
// the numerical spec that the tests use.  Kernels in smc_util_kernels.h and below.
#include "smc_host.h"
#include "smc_util_kernels.h"
#include "smc_pred_kernels.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace smc;

// ---- DeviceCall (smc_host.h): the scope of every call without a handle ---------------------------
int DeviceCall::begin(const char* who, int device) {
    static thread_local hipStream_t streams[16] = {};   // (never destroyed: see smc_host.h)
    who_ = who;
    device_ = device;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(SMC_EHIP, std::string(who) + ": no HIP device");
    if (device < 0 || device >= ndev) return fail(SMC_EINVAL, std::string(who) + ": bad device");
    HIPCHK(hipSetDevice(device));
    if (device < 16 && !streams[device]) HIPCHK(hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking));
    stream = device < 16 ? streams[device] : nullptr;
    return SMC_OK;
}
int DeviceCall::use_scratch() {
    static thread_local struct Scratch {
        void* p = nullptr;
        size_t cap = 0;
        int device = -1;
        ~Scratch() { if (p) (void)hipFree(p); }
    } c;
    const size_t need = plan_.bytes ? plan_.bytes : 16;
    if (c.cap < need || c.device != device_) {
        if (c.p) { (void)hipFree(c.p); c.p = nullptr; c.cap = 0; }
        void* q = nullptr;
        HIPCHK(hipMalloc(&q, need));
        c.p = q; c.cap = need; c.device = device_;
    }
    base_ = (char*)c.p;
    return SMC_OK;
}
int DeviceCall::use_own() {
    const hipError_t e = own_.grow(plan_.bytes);
    if (e != hipSuccess) return alloc_fail(who_, e);
    base_ = own_.as<char>();
    return SMC_OK;
}

// ---- stand-alone normalize / resample ------------------------------------------------------------
static int fix_bits_for(int64_t n) {
    const int k = 61 - ceil_log2_i64(n);
    return k > FIX_BITS ? FIX_BITS : k;
}

extern "C" int smc_normalize(const double* logw, int64_t n, double* w, double* logmu, double* ess, int device) {
    if (!logw || !w || n <= 0) return fail(SMC_EINVAL, "smc_normalize: bad argument");
    DeviceCall c;
    if (const int rc = c.begin("smc_normalize", device)) return rc;
    const size_t b_n = (size_t)n * 8;
    const size_t o_in = c.take(b_n), o_w = c.take(b_n), o_o = c.take(16), o_acc = c.take(5 * 8);   // (acc: the grid-wide branch only)
    if (const int rc = c.use_scratch()) return rc;
    const hipStream_t st = c.stream;
    double *d_in = c.at<double>(o_in), *d_w = c.at<double>(o_w), *d_o = c.at<double>(o_o);
    HIPCHK(c.upload(o_in, logw, b_n));
    if (n <= 16384) {
        // one workgroup: the outer reweight works on n_theta-vectors (a few thousand entries)
        hipLaunchKernelGGL((k_normalize<1024>), dim3(1), dim3(1024), 0, st, d_in, n, fix_bits_for(n), d_w, d_o);
        HIPCHK(hipGetLastError());
    } else {
        // a whole cloud's log-weights: three grid-wide passes, every cross-workgroup combination an integer one (same bits)
        unsigned long long* acc = c.at<unsigned long long>(o_acc);
        int* kmax_i = reinterpret_cast<int*>(acc + 4);
        HIPCHK(hipMemsetAsync(acc, 0, 32, st));
        HIPCHK(hipMemsetD32Async(kmax_i, NORM_DEAD, 1, st));
        int64_t nb = (n + 4 * 256 - 1) / (4 * 256);
        nb = nb > 2048 ? 2048 : nb;
        const int K = fix_bits_for(n);
        hipLaunchKernelGGL((k_normalize_max<256>), dim3((unsigned)nb), dim3(256), 0, st, d_in, n, kmax_i);
        hipLaunchKernelGGL((k_normalize_sum<256>), dim3((unsigned)nb), dim3(256), 0, st, d_in, n, K, kmax_i, acc);
        hipLaunchKernelGGL((k_normalize_write<256>), dim3((unsigned)nb), dim3(256), 0, st, d_in, n, K, kmax_i, acc, d_w, d_o);
        HIPCHK(hipGetLastError());
    }
    double o[2];
    HIPCHK(c.download(w, o_w, b_n));
    HIPCHK(c.download(o, o_o, 16));
    HIPCHK(c.finish());
    if (logmu) *logmu = o[0];
    if (ess) *ess = o[1];
    return SMC_OK;
}

extern "C" int smc_resample(const double* w, int64_t n, int64_t ndraw, uint64_t seed, uint32_t stream, uint32_t t,
                            int32_t* a, int device) {
    if (!w || !a || n <= 0 || ndraw < 0) return fail(SMC_EINVAL, "smc_resample: bad argument");
    if (n > ((int64_t)1 << 31)) return fail(SMC_EINVAL, "smc_resample: n > 2^31");
    if (ndraw == 0) return SMC_OK;
    // the chunks of the grid-wide branch (a whole cloud's weights): contiguous, a multiple of the workgroup
    constexpr int TH = 256;
    int nb = (int)((n + 4 * TH - 1) / (4 * TH));
    nb = nb > 2048 ? 2048 : nb;
    const int64_t chunk = ((n + nb - 1) / nb + TH - 1) / TH * TH;
    nb = (int)((n + chunk - 1) / chunk);
    DeviceCall c;
    if (const int rc = c.begin("smc_resample", device)) return rc;
    const size_t o_w = c.take((size_t)n * 8), o_C = c.take((size_t)n * 8), o_a = c.take((size_t)ndraw * 4), o_st = c.take(4);
    const size_t o_bs = c.take(((size_t)nb + 1) * 8);   // (the chunk sums and the maximum: the grid-wide branch only)
    if (const int rc = c.use_scratch()) return rc;
    const hipStream_t st = c.stream;
    double* d_w = c.at<double>(o_w);
    uint64_t *d_C = c.at<uint64_t>(o_C), *d_bs = c.at<uint64_t>(o_bs);
    int* d_st = c.at<int>(o_st);
    HIPCHK(c.upload(o_w, w, (size_t)n * 8));
    if (n <= 65536) {
        hipLaunchKernelGGL((k_resample_cdf<1024>), dim3(1), dim3(1024), 0, st, d_w, n, fix_bits_for(n), d_C, d_st);
    } else {   // the inclusive sums grid-wide (the same integers)
        unsigned long long* mbits = c.at<unsigned long long>(o_bs) + nb;
        HIPCHK(hipMemsetAsync(mbits, 0, 8, st));
        hipLaunchKernelGGL((k_rs_max<TH>), dim3((unsigned)nb), dim3(TH), 0, st, d_w, n, mbits);
        hipLaunchKernelGGL((k_rs_chunk_sums<TH>), dim3((unsigned)nb), dim3(TH), 0, st, d_w, n, fix_bits_for(n), mbits, chunk, d_bs);
        hipLaunchKernelGGL((k_rs_scan_chunks<1024>), dim3(1), dim3(1024), 0, st, mbits, nb, d_bs, d_st);
        hipLaunchKernelGGL((k_rs_write<TH>), dim3((unsigned)nb), dim3(TH), 0, st, d_w, n, fix_bits_for(n), mbits, chunk, d_bs, d_C);
    }
    HIPCHK(hipGetLastError());
    int status = 0;
    HIPCHK(c.download(&status, o_st, 4));
    HIPCHK(c.finish());
    if (status != 0) return fail(SMC_EINVAL, "smc_resample: weights must be finite with a positive maximum");
    hipLaunchKernelGGL(k_resample_draw, dim3((unsigned)((ndraw + 255) / 256)), dim3(256), 0, st, d_C, n, ndraw, seed, stream, t,
                       c.at<int32_t>(o_a));
    HIPCHK(hipGetLastError());
    HIPCHK(c.download(a, o_a, (size_t)ndraw * 4));
    HIPCHK(c.finish());
    return SMC_OK;
}

extern "C" int smc_kalman_log_likelihood_flags(const double* raw, int64_t n_theta, const double* y, int64_t T, int predict_first,
                                               double* out, int device, uint32_t flags) {
    if (flags & ~SMC_FLAG_NAN_MISSING) return fail(SMC_EINVAL, "smc_kalman_log_likelihood: flags is 0 or SMC_FLAG_NAN_MISSING");
    if (!raw || !y || !out || n_theta <= 0 || T <= 0) return fail(SMC_EINVAL, "smc_kalman_log_likelihood: bad argument");
    DeviceCall c;
    if (const int rc = c.begin("smc_kalman_log_likelihood", device)) return rc;
    const size_t o_raw = c.take((size_t)n_theta * 48), o_y = c.take((size_t)T * 8), o_out = c.take((size_t)n_theta * 24);
    if (const int rc = c.use_scratch()) return rc;
    HIPCHK(c.upload(o_raw, raw, (size_t)n_theta * 48));
    HIPCHK(c.upload(o_y, y, (size_t)T * 8));
    const dim3 grid((unsigned)((n_theta + KALMAN_THREADS - 1) / KALMAN_THREADS));
    if (kalman_has_gap(flags, y, T))   // the MISS twin only for a flagged call whose series holds a NaN
        hipLaunchKernelGGL((k_kalman_loglik<Lg1Row, true>), grid, dim3(KALMAN_THREADS), 0, c.stream, c.at<double>(o_raw), n_theta, c.at<double>(o_y), T,
                           predict_first, c.at<double>(o_out));
    else
        hipLaunchKernelGGL((k_kalman_loglik<Lg1Row, false>), grid, dim3(KALMAN_THREADS), 0, c.stream, c.at<double>(o_raw), n_theta, c.at<double>(o_y), T,
                           predict_first, c.at<double>(o_out));
    HIPCHK(hipGetLastError());
    HIPCHK(c.download(out, o_out, (size_t)n_theta * 24));
    HIPCHK(c.finish());
    return SMC_OK;
}
extern "C" int smc_kalman_log_likelihood(const double* raw, int64_t n_theta, const double* y, int64_t T, int predict_first,
                                         double* out, int device) {
    return smc_kalman_log_likelihood_flags(raw, n_theta, y, T, predict_first, out, device, 0);
}

// ---- predictive checks (smc_spec.h "predictive checks") without a handle -------------------------------------------------------
// the exact Kalman rows of a series under every parameter row: pit, ym, yv [T][n_theta] (any NULL)
extern "C" int smc_kalman_predictive_flags(const double* raw, int64_t n_theta, const double* y, int64_t T, int predict_first, double* pit, double* ym,
                                           double* yv, int device, uint32_t flags) {
    if (flags & ~SMC_FLAG_NAN_MISSING) return fail(SMC_EINVAL, "smc_kalman_predictive: flags is 0 or SMC_FLAG_NAN_MISSING");
    if (!raw || !y || n_theta <= 0 || T <= 0) return fail(SMC_EINVAL, "smc_kalman_predictive: bad argument");
    DeviceCall c;
    if (const int rc = c.begin("smc_kalman_predictive", device)) return rc;
    const size_t plane = (size_t)T * (size_t)n_theta * 8;
    const size_t o_raw = c.take((size_t)n_theta * 48), o_y = c.take((size_t)T * 8);
    const size_t o_pit = c.take(plane), o_ym = c.take(plane), o_yv = c.take(plane);   // (the planes stay in the thread's scratch)
    if (const int rc = c.use_scratch()) return rc;
    HIPCHK(c.upload(o_raw, raw, (size_t)n_theta * 48));
    HIPCHK(c.upload(o_y, y, (size_t)T * 8));
    double *d_pit = pit ? c.at<double>(o_pit) : nullptr, *d_ym = ym ? c.at<double>(o_ym) : nullptr, *d_yv = yv ? c.at<double>(o_yv) : nullptr;
    const dim3 grid((unsigned)((n_theta + KALMAN_THREADS - 1) / KALMAN_THREADS));
    if (kalman_has_gap(flags, y, T))   // the MISS twin only for a flagged call whose series holds a NaN
        hipLaunchKernelGGL((k_kalman_predictive<Lg1Row, true>), grid, dim3(KALMAN_THREADS), 0, c.stream, c.at<double>(o_raw), n_theta, c.at<double>(o_y), T,
                           predict_first, d_pit, d_ym, d_yv);
    else
        hipLaunchKernelGGL((k_kalman_predictive<Lg1Row, false>), grid, dim3(KALMAN_THREADS), 0, c.stream, c.at<double>(o_raw), n_theta, c.at<double>(o_y), T,
                           predict_first, d_pit, d_ym, d_yv);
    HIPCHK(hipGetLastError());
    if (pit) HIPCHK(c.download(pit, o_pit, plane));
    if (ym) HIPCHK(c.download(ym, o_ym, plane));
    if (yv) HIPCHK(c.download(yv, o_yv, plane));
    HIPCHK(c.finish());
    return SMC_OK;
}
// ... and their host twin for one row: pit, ym, yv [T] (any NULL)
extern "C" int smc_host_kalman_predictive(const double* row, const double* y, int64_t T, int predict_first, uint32_t flags, double* pit, double* ym,
                                          double* yv) {
    if (flags & ~SMC_FLAG_NAN_MISSING) return fail(SMC_EINVAL, "smc_host_kalman_predictive: flags is 0 or SMC_FLAG_NAN_MISSING");
    if (!row || !y || T <= 0) return fail(SMC_EINVAL, "smc_host_kalman_predictive: bad argument");
    const bool miss = kalman_has_gap(flags, y, T);
    double x = row[4], S = row[5];
    for (int64_t t = 0; t < T; ++t) {
        double p, mu, v;
        const bool predict = predict_first != 0 || t > 0;
        if (miss) kalman_predictive_step<true>(row[0], row[1], row[2], row[3], predict, y[t], x, S, p, mu, v);
        else kalman_predictive_step<false>(row[0], row[1], row[2], row[3], predict, y[t], x, S, p, mu, v);
        if (pit) pit[t] = p;
        if (ym) ym[t] = mu;
        if (yv) yv[t] = v;
    }
    return SMC_OK;
}
extern "C" double smc_host_normcdf(double z) { return sp_normcdf(z); }
extern "C" int smc_device_normcdf(const double* z, int64_t n, double* out, int device) {
    if (!z || !out || n <= 0) return fail(SMC_EINVAL, "smc_device_normcdf: bad argument");
    DeviceCall c;
    if (const int rc = c.begin("smc_device_normcdf", device)) return rc;
    const size_t o_z = c.take((size_t)n * 8), o_out = c.take((size_t)n * 8);
    if (const int rc = c.use_scratch()) return rc;
    HIPCHK(c.upload(o_z, z, (size_t)n * 8));
    hipLaunchKernelGGL(k_normcdf<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, c.at<double>(o_z), n, c.at<double>(o_out));
    HIPCHK(hipGetLastError());
    HIPCHK(c.download(out, o_out, (size_t)n * 8));
    HIPCHK(c.finish());
    return SMC_OK;
}
// the row of ONE cloud x [d][n] (the order of smc_get_state) for the observation y: out = (pit, obs_mean, obs_var), the statement of
// the specification in its own order (pred_sum over pred_terms, then the centred pass)
extern "C" int smc_host_predictive(int model_id, const double* raw, const double* x, int64_t n, double y, double* out) {
    if (!raw || !x || !out || n < 1) return fail(SMC_EINVAL, "smc_host_predictive: bad argument");
    if (!has_density(model_id))
        return fail(SMC_EINVAL, "smc_host_predictive: the families whose rows are a sample of the state: LG1D, SV1D, UCSV3D");
    Params P;
    params_from_raw(model_id, raw, P);
    std::vector<double> cdf((size_t)n), ymv((size_t)n), s2((size_t)n), part((size_t)((n + SMOOTH_CH - 1) / SMOOTH_CH));
    (void)by_density_model(model_id, [&](auto Mt) {
        constexpr int M = decltype(Mt)::value;
        for (int64_t i = 0; i < n; ++i) {
            double xi[3] = {x[i], 0.0, 0.0};
            if constexpr (pred_rows<M>::count == 2) xi[pred_rows<M>::second] = x[(size_t)pred_rows<M>::second * n + i];
            pred_terms<M>(P, xi, y, cdf[i], ymv[i], s2[i]);
        }
        return hipSuccess;
    });
    const double pit = pred_mean_of(pred_sum(n, [&](int64_t i) { return cdf[i]; }, part.data()), n);
    const double mean = pred_mean_of(pred_sum(n, [&](int64_t i) { return ymv[i]; }, part.data()), n);
    const double sum_s2 = pred_sum(n, [&](int64_t i) { return s2[i]; }, part.data());
    const double sum_c = pred_sum(n, [&](int64_t i) { return pred_centred_term(ymv[i], mean); }, part.data());
    out[0] = pit; out[1] = mean; out[2] = pred_var_of(sum_s2, sum_c, n);
    return SMC_OK;
}

// ---- host-side helpers ---------------------------------------------------------------------------
// The unweighted summaries' definition on the host, by sorting (include/smc_hip.h "summary modes"): the spec's twin of the UNW kernels.
extern "C" int smc_host_quantile7(const double* x, int64_t n, const double* p, int np, double* out) {
    if (!x || !p || !out || n < 1 || np < 0) return fail(SMC_EINVAL, "smc_host_quantile7: bad argument");
    for (int j = 0; j < np; ++j)
        if (!(p[j] >= 0.0 && p[j] <= 1.0)) return fail(SMC_EINVAL, "smc_host_quantile7: levels must lie in [0, 1]");
    std::vector<uint64_t> k((size_t)n);
    for (int64_t i = 0; i < n; ++i) k[(size_t)i] = order_key(x[i]);
    std::sort(k.begin(), k.end());
    for (int j = 0; j < np; ++j) {
        const Q7Rank r = q7_rank(n, p[j]);
        const uint64_t ka = k[(size_t)(r.j > 1 ? r.j - 1 : 0)], kb = n == 1 ? ka : k[(size_t)r.j];
        out[j] = q7_interp(key_value(ka), key_value(kb), r.g);
    }
    return SMC_OK;
}
extern "C" int smc_host_sample_moments(const double* x, int64_t n, double* mean, double* var) {
    if (!x || !mean || !var || n < 1) return fail(SMC_EINVAL, "smc_host_sample_moments: bad argument");
    double s = 0.0, s2 = 0.0;
    for (int64_t i = 0; i < n; ++i) s += x[i];
    double m = s / (double)n, r = 0.0;
    for (int64_t i = 0; i < n; ++i) r += x[i] - m;   // (the rounding of the first sum, taken back)
    if (r - r == 0.0) m += r / (double)n;   // (a cloud that holds +inf or -inf: inf - inf here; its mean stays the +-inf of the sum, as mean(x))
    for (int64_t i = 0; i < n; ++i) { const double e = x[i] - m; s2 += e * e; }
    *mean = m;
    *var = s2 / (double)(n - 1);   // (n == 1: 0 / 0, NaN as Statistics.var)
    return SMC_OK;
}
template <int MODEL>
static void simulate_t(const Params& p, int64_t T, uint64_t seed, double* x, double* y) {
    constexpr int D = model_dim<MODEL>::value;
    double xc[D], xn[D], z[D], z1, mean, sd;
    for (int64_t t = 0; t < T; ++t) {
        for (int c = 0; c < D; ++c) box_muller(draw(seed, 0u, SIM_STREAM, (uint32_t)t, SLOT_NORMAL0 + c), z[c], z1);
        if (t == 0) model_initial<MODEL>(p, z, xn); else model_transition<MODEL>(p, xc, z, xn);
        model_obs_moments<MODEL>(p, xn, mean, sd);
        double e;
        box_muller(draw(seed, 0u, SIM_STREAM, (uint32_t)t, SLOT_OBS), e, z1);
        y[t] = fma(sd, e, mean);
        for (int c = 0; c < D; ++c) { xc[c] = xn[c]; if (x) x[(size_t)c * T + t] = xn[c]; }
    }
}

extern "C" int smc_simulate_dim(int model_id) { return model_id == MODEL_UCSV_RB ? model_dim_rt(MODEL_UCSV3D) : model_dim_rt(model_id); }
extern "C" int smc_simulate(int model_id, const double* raw, int64_t T, uint64_t seed, double* x, double* y) {
    if (model_nraw_rt(model_id) < 0 || !raw || !y || T <= 0) return fail(SMC_EINVAL, "smc_simulate: bad argument");
    Params p;
    params_from_raw(model_id, raw, p);
    (void)by_model(model_id, [&](auto M) {
        // the data-generating model of the marginal family is UCSV: x is [3][T] (smc_simulate_dim)
        constexpr int SIM = decltype(M)::value == MODEL_UCSV_RB ? MODEL_UCSV3D : decltype(M)::value;
        simulate_t<SIM>(p, T, seed, x, y);
        return hipSuccess;
    });
    return SMC_OK;
}

// the forecast specification on the host (smc_spec.h "forecasts"): the twin of k_forecast, particle pairs sharing their Box-Muller pairs
template <int MODEL>
static void host_forecast_t(const Params& p, const double* x, int64_t n, int64_t H, uint64_t seed, uint32_t stream, double* xf, double* yf,
                            double* ym, double* yv) {
    constexpr int D = model_dim<MODEL>::value, NZ = model_nz<MODEL>::value;
    for (int64_t i0 = 0; i0 < n; i0 += 2) {
        const int np = i0 + 1 < n ? 2 : 1;
        double xs[2][D] = {};
        for (int q = 0; q < np; ++q)
            for (int c = 0; c < D; ++c) xs[q][c] = x[(size_t)c * n + i0 + q];
        for (int64_t k = 1; k <= H; ++k) {
            double z[NZ][2], e[2];
            for (int c = 0; c < NZ; ++c) box_muller(draw(seed, (uint32_t)(i0 >> 1), stream, (uint32_t)k, SLOT_NORMAL0 + c), z[c][0], z[c][1]);
            box_muller(draw(seed, (uint32_t)(i0 >> 1), stream, (uint32_t)k, SLOT_OBS), e[0], e[1]);
            for (int q = 0; q < np; ++q) {
                double zz[NZ], xn[D], f, m, v;
                for (int c = 0; c < NZ; ++c) zz[c] = z[c][q];
                model_forecast_step<MODEL>(p, xs[q], zz, e[q], xn, f, m, v);
                const size_t at = (size_t)(k - 1) * n + i0 + q;
                for (int c = 0; c < D; ++c) {
                    xs[q][c] = xn[c];
                    if (xf) xf[((size_t)(k - 1) * D + c) * n + i0 + q] = xn[c];
                }
                if (yf) yf[at] = f;
                if (ym) ym[at] = m;
                if (yv) yv[at] = v;
            }
        }
    }
}
extern "C" int smc_host_forecast(int model_id, const double* raw, const double* x, int64_t n, int64_t H, uint64_t forecast_seed, uint32_t stream,
                                 double* xf, double* yf, double* ym, double* yv) {
    if (model_nraw_rt(model_id) < 0 || !raw || !x || n < 1 || n > ((int64_t)1 << 31) || H < 1 || H > 0x7fffffff)
        return fail(SMC_EINVAL, "smc_host_forecast: bad argument");
    Params p;
    params_from_raw(model_id, raw, p);
    (void)by_model(model_id, [&](auto M) {
        host_forecast_t<decltype(M)::value>(p, x, n, H, forecast_seed, stream, xf, yf, ym, yv);
        return hipSuccess;
    });
    return SMC_OK;
}

extern "C" double smc_host_exp(double x) { return sp_exp(x); }
extern "C" double smc_host_log(double x) { return sp_log(x); }
extern "C" void smc_host_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    const u32x4 r = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    for (int i = 0; i < 4; ++i) out[i] = r.v[i];
}
extern "C" void smc_host_box_muller(const uint32_t w[4], double* z0, double* z1) {
    box_muller(u32x4{{w[0], w[1], w[2], w[3]}}, *z0, *z1);
}

extern "C" int smc_host_pmmh_propose(int d_theta, uint64_t move_seed, uint32_t stream, uint32_t c, const double* theta,
                                     const double* chol, double scale, double* prop) {
    if (d_theta < 1 || d_theta > MAX_DTHETA || !theta || !chol || !prop) return fail(SMC_EINVAL, "smc_host_pmmh_propose: bad argument");
    PmmhSpec sp{};
    sp.d = d_theta;
    pmmh_propose(sp, move_seed, stream, c, theta, chol, sqrt(scale), prop);
    return SMC_OK;
}
extern "C" double smc_host_pmmh_log_uniform(uint64_t move_seed, uint32_t stream, uint32_t c) { return pmmh_log_uniform(move_seed, stream, c); }
extern "C" double smc_host_prior_logpdf(int family, const double* par, double x) {
    return prior_insupport(family, par, x) ? prior_logpdf(family, par, x) : -inf();
}

__global__ void k_device_math(int which, const double* a, const double* b, int64_t n, double* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i];
    double r = 0.0;
    if (which == 0) r = sp_exp(x);
    else if (which == 1) r = sp_log(x);
    else if (which == 2) r = sqrt(x);
    else if (which == 3 || which == 4) {
        const uint64_t ua = d2bits(x), ub = d2bits(b[i]);
        double z0, z1;
        box_muller(u32x4{{(uint32_t)ua, (uint32_t)(ua >> 32), (uint32_t)ub, (uint32_t)(ub >> 32)}}, z0, z1);
        r = which == 3 ? z0 : z1;
    } else if (which == 5) r = x / b[i];
    out[i] = r;
}

__global__ void k_sys_targets(uint64_t Dtot, uint32_t n, uint64_t u, uint64_t j0, int nk, uint64_t* out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nk) out[k] = sys_target(sys_base(Dtot, n, 1.0 / (double)n, u, j0), (uint32_t)k);
}
// T_{j0+k} = floor(((j0+k) Dtot + mulhi64(u, Dtot)) / n), k < nk <= 8192: the division-free evaluation the
// systematic kernels use, on the host (device < 0) or on a device - tests compare both with exact integers
extern "C" int smc_sys_targets(uint64_t Dtot, uint32_t n, uint64_t u, uint64_t j0, int nk, uint64_t* out, int device) {
    if (!out || nk < 1 || nk > 8192 || n < 1 || n >= (1u << 31) || Dtot >= (1ull << 63) || j0 + (uint64_t)nk > n)
        return fail(SMC_EINVAL, "smc_sys_targets: bad argument");
    if (device < 0) {
        const SysBase sb = sys_base(Dtot, n, 1.0 / (double)n, u, j0);
        for (int k = 0; k < nk; ++k) out[k] = sys_target(sb, (uint32_t)k);
        return SMC_OK;
    }
    DeviceCall c;
    if (const int rc = c.begin("smc_sys_targets", device)) return rc;
    const size_t o_out = c.take((size_t)nk * 8);
    if (const int rc = c.use_scratch()) return rc;
    hipLaunchKernelGGL(k_sys_targets, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, c.stream, Dtot, n, u, j0, nk, c.at<uint64_t>(o_out));
    HIPCHK(hipGetLastError());
    HIPCHK(c.download(out, o_out, (size_t)nk * 8));
    HIPCHK(c.finish());
    return SMC_OK;
}

// the proposals (smc_spec.h "proposals"), one particle on the host / n particles on a device
extern "C" int smc_host_optimal_proposal(int model_id, const double* raw, double* par) {
    if (!raw || !par) return fail(SMC_EINVAL, "smc_host_optimal_proposal: NULL argument");
    if (model_id != MODEL_LG1D) return fail(SMC_EINVAL, "smc_host_optimal_proposal: LG1D only (the UCSV proposal has no parameters)");
    optimal_proposal_lg(raw, par);
    return SMC_OK;
}
// the parameter and proposal rows of one guided particle step from (raw, kind, par); false: refused
static bool guided_params(int model_id, const double* raw, int kind, const double* par, Params& P, PropRow& R) {
    if (model_nraw_rt(model_id) < 0 || !raw || kind == PROP_NONE || !proposal_supported(model_id, kind)) return false;
    if ((kind == PROP_AFFINE) != (par != nullptr)) return false;
    if (kind == PROP_AFFINE && !affine_row_ok(par)) return false;
    params_from_raw(model_id, raw, P);
    R = PropRow{};
    if (kind == PROP_AFFINE)
        for (int k = 0; k < PROP_NPAR; ++k) R.p[k] = par[k];
    derive_proposal(model_id, kind, P.raw, P.der, R.p);
    return true;
}
// ... and of any particle step: kind == PROP_NONE is the bootstrap (or marginal) step, whose proposal row is zeros
static bool filter_step_params(int model_id, const double* raw, int kind, const double* par, Params& P, PropRow& R) {
    if (kind != PROP_NONE) return guided_params(model_id, raw, kind, par, P, R);
    if (model_nraw_rt(model_id) < 0 || !raw || par) return false;
    params_from_raw(model_id, raw, P);
    R = PropRow{};
    return true;
}

// The whole step of a filter (include/smc_hip.h "missing observations"): every family and proposal, the first step and the missing
// step included - what k_init, k_step and k_resident do to one particle.  The ONE gather / step / scatter loop of the probes below:
// for n particles on the host (host_steps) / on a device (k_filter_steps, device_steps); xp [d][n] (not read at the first step),
// z [nz][n] -> x [d][n], logw [n]
template <int MODEL>
SMC_HD double filter_step_one(const Params& P, const PropRow& R, bool guided, bool first, bool miss, const double* xp, const double* z, double y,
                              double* x) {
    if (miss) {
        model_missing_step<MODEL>(P, first, xp, z, x);
        return 0.0;
    }
    if constexpr (model_marginal<MODEL>::value) {
        return model_marginal_step<MODEL>(P, first, xp, z, y, x);
    } else {
        if (first) model_initial<MODEL>(P, z, x);
        else if (guided) return model_guided<MODEL>(P, R, xp, z, y, x);
        else model_transition<MODEL>(P, xp, z, x);
        return model_logobs<MODEL>(P, x, y);
    }
}
static void host_steps(int model_id, const Params& P, const PropRow& R, bool guided, bool first, bool miss, const double* xp, const double* z, double y,
                       int64_t n, double* x, double* logw) {
    (void)by_model(model_id, [&](auto M) {
        constexpr int MODEL = decltype(M)::value, D = model_dim<MODEL>::value, NZ = model_nz<MODEL>::value;
        for (int64_t i = 0; i < n; ++i) {
            double a[D] = {}, zz[NZ], xn[D];
            for (int c = 0; c < D && !first; ++c) a[c] = xp[(size_t)c * n + i];
            for (int c = 0; c < NZ; ++c) zz[c] = z[(size_t)c * n + i];
            logw[i] = filter_step_one<MODEL>(P, R, guided, first, miss, a, zz, y, xn);
            for (int c = 0; c < D; ++c) x[(size_t)c * n + i] = xn[c];
        }
        return hipSuccess;
    });
}
template <int MODEL>
__global__ void k_filter_steps(Params P, PropRow R, int guided, int first, int miss, const double* xp, const double* z, double y, int64_t n, double* x,
                               double* logw) {
    constexpr int D = model_dim<MODEL>::value, NZ = model_nz<MODEL>::value;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a[D] = {}, zz[NZ], xn[D];
    for (int c = 0; c < D; ++c) a[c] = first ? 0.0 : xp[(size_t)c * n + i];
    for (int c = 0; c < NZ; ++c) zz[c] = z[(size_t)c * n + i];
    logw[i] = filter_step_one<MODEL>(P, R, guided != 0, first != 0, miss != 0, a, zz, y, xn);
    for (int c = 0; c < D; ++c) x[(size_t)c * n + i] = xn[c];
}
static int device_steps(const char* who, int model_id, const Params& P, const PropRow& R, bool guided, bool first, bool miss, const double* xp,
                        const double* z, double y, int64_t n, double* x, double* logw, int device) {
    const size_t b_x = (size_t)model_dim_rt(model_id) * n * 8, b_z = (size_t)(model_id == MODEL_UCSV_RB ? 2 : model_dim_rt(model_id)) * n * 8;
    DeviceCall c;
    if (const int rc = c.begin(who, device)) return rc;
    const size_t o_xp = c.take(b_x), o_z = c.take(b_z), o_x = c.take(b_x), o_lw = c.take((size_t)n * 8);
    if (const int rc = c.use_scratch()) return rc;
    if (!first) HIPCHK(c.upload(o_xp, xp, b_x));
    HIPCHK(c.upload(o_z, z, b_z));
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    HIPCHK(by_model(model_id, [&](auto M) {
        hipLaunchKernelGGL(k_filter_steps<decltype(M)::value>, grid, block, 0, c.stream, P, R, guided ? 1 : 0, first ? 1 : 0, miss ? 1 : 0,
                           c.at<double>(o_xp), c.at<double>(o_z), y, n, c.at<double>(o_x), c.at<double>(o_lw));
        return hipGetLastError();
    }));
    HIPCHK(c.download(x, o_x, b_x));
    HIPCHK(c.download(logw, o_lw, (size_t)n * 8));
    HIPCHK(c.finish());
    return SMC_OK;
}
extern "C" int smc_host_guided_step(int model_id, const double* raw, int kind, const double* par, const double* xp, const double* z,
                                    double y, double* x, double* logw) {
    if (!xp || !z || !x || !logw) return fail(SMC_EINVAL, "smc_host_guided_step: NULL argument");
    Params P;
    PropRow R;
    if (!guided_params(model_id, raw, kind, par, P, R)) return fail(SMC_EINVAL, "smc_host_guided_step: bad model, kind or row");
    (void)by_guided_model(model_id, [&](auto M) {   // (guided_params has refused every other family)
        *logw = model_guided<decltype(M)::value>(P, R, xp, z, y, x);
        return hipSuccess;
    });
    return SMC_OK;
}
// the same for n particles in the device twin's layouts, a plain loop on the host (the composed references of the tests)
extern "C" int smc_host_guided_steps(int model_id, const double* raw, int kind, const double* par, const double* xp, const double* z,
                                     double y, int64_t n, double* x, double* logw) {
    if (!xp || !z || !x || !logw || n <= 0) return fail(SMC_EINVAL, "smc_host_guided_steps: bad argument");
    Params P;
    PropRow R;
    if (!guided_params(model_id, raw, kind, par, P, R)) return fail(SMC_EINVAL, "smc_host_guided_steps: bad model, kind or row");
    host_steps(model_id, P, R, true, false, false, xp, z, y, n, x, logw);
    return SMC_OK;
}
extern "C" int smc_device_guided_step(int model_id, const double* raw, int kind, const double* par, const double* xp, const double* z,
                                      double y, int64_t n, double* x, double* logw, int device) {
    if (!xp || !z || !x || !logw || n <= 0) return fail(SMC_EINVAL, "smc_device_guided_step: bad argument");
    Params P;
    PropRow R;
    if (!guided_params(model_id, raw, kind, par, P, R)) return fail(SMC_EINVAL, "smc_device_guided_step: bad model, kind or row");
    return device_steps("smc_device_guided_step", model_id, P, R, true, false, false, xp, z, y, n, x, logw, device);
}

// what the blocks of smc_host.h hold right now, process-wide (include/smc_hip.h)
extern "C" int smc_live_bytes(int64_t* device_bytes, int64_t* pinned_bytes) {
    if (device_bytes) *device_bytes = g_live_bytes[0].load(std::memory_order_relaxed);
    if (pinned_bytes) *pinned_bytes = g_live_bytes[1].load(std::memory_order_relaxed);
    return SMC_OK;
}

// the marginal step (smc_spec.h "marginal families"), one particle on the host / n particles on a device
extern "C" int smc_host_rb_step(const double* raw, const double* sp, const double* z, double y, int first, double* s, double* logw) {
    if (!raw || !sp || !z || !s || !logw) return fail(SMC_EINVAL, "smc_host_rb_step: NULL argument");
    Params P;
    params_from_raw(MODEL_UCSV_RB, raw, P);
    double a[4] = {sp[0], sp[1], sp[2], sp[3]}, o[4];
    *logw = model_marginal_step<MODEL_UCSV_RB>(P, first != 0, a, z, y, o);
    for (int c = 0; c < 4; ++c) s[c] = o[c];
    return SMC_OK;
}
// the same for n particles in the device twin's layouts, a plain loop on the host (the composed references of the tests)
extern "C" int smc_host_rb_steps(const double* raw, const double* sp, const double* z, double y, int first, int64_t n, double* s,
                                 double* logw) {
    if (!raw || !sp || !z || !s || !logw || n <= 0) return fail(SMC_EINVAL, "smc_host_rb_steps: bad argument");
    Params P;
    params_from_raw(MODEL_UCSV_RB, raw, P);
    host_steps(MODEL_UCSV_RB, P, PropRow{}, false, first != 0, false, sp, z, y, n, s, logw);
    return SMC_OK;
}
extern "C" int smc_device_rb_step(const double* raw, const double* sp, const double* z, double y, int first, int64_t n, double* s, double* logw,
                                  int device) {
    if (!raw || !sp || !z || !s || !logw || n <= 0) return fail(SMC_EINVAL, "smc_device_rb_step: bad argument");
    Params P;
    params_from_raw(MODEL_UCSV_RB, raw, P);
    return device_steps("smc_device_rb_step", MODEL_UCSV_RB, P, PropRow{}, false, first != 0, false, sp, z, y, n, s, logw, device);
}

// the whole step for n particles, every family and proposal (filter_step_one above)
extern "C" int smc_host_filter_steps(int model_id, const double* raw, int kind, const double* par, const double* xp, const double* z, double y,
                                     int first, int nan_missing, int64_t n, double* x, double* logw) {
    if (!z || !x || !logw || n <= 0 || (!first && !xp)) return fail(SMC_EINVAL, "smc_host_filter_steps: bad argument");
    Params P;
    PropRow R;
    if (!filter_step_params(model_id, raw, kind, par, P, R)) return fail(SMC_EINVAL, "smc_host_filter_steps: bad model, kind or row");
    host_steps(model_id, P, R, kind != PROP_NONE, first != 0, nan_missing && y != y, xp, z, y, n, x, logw);
    return SMC_OK;
}
// the conditional particle filter (include/smc_hip.h): the retained slot and the log-weight of the reference row on the host
extern "C" int smc_host_conditional_slot(uint64_t seed, uint32_t stream, uint32_t t, int64_t n_x, int64_t* k) {
    if (!k || n_x < 1 || n_x > ((int64_t)1 << 31)) return fail(SMC_EINVAL, "smc_host_conditional_slot: bad argument");
    *k = (int64_t)cond_slot(seed, stream, t, (uint32_t)n_x);
    return SMC_OK;
}
extern "C" int smc_host_logobs(int model_id, const double* raw, const double* x, double y, double* out) {
    if (!x || !out) return fail(SMC_EINVAL, "smc_host_logobs: NULL argument");
    Params P;
    PropRow R;
    if (!has_density(model_id) || !filter_step_params(model_id, raw, PROP_NONE, nullptr, P, R))
        return fail(SMC_EINVAL, "smc_host_logobs: bad model or row (the families with an observation density of the state: LG1D, SV1D, UCSV3D)");
    (void)by_density_model(model_id, [&](auto M) {
        *out = model_logobs<decltype(M)::value>(P, x, y);
        return hipSuccess;
    });
    return SMC_OK;
}
extern "C" int smc_device_filter_steps(int model_id, const double* raw, int kind, const double* par, const double* xp, const double* z, double y,
                                       int first, int nan_missing, int64_t n, double* x, double* logw, int device) {
    if (!z || !x || !logw || n <= 0 || (!first && !xp)) return fail(SMC_EINVAL, "smc_device_filter_steps: bad argument");
    Params P;
    PropRow R;
    if (!filter_step_params(model_id, raw, kind, par, P, R)) return fail(SMC_EINVAL, "smc_device_filter_steps: bad model, kind or row");
    return device_steps("smc_device_filter_steps", model_id, P, R, kind != PROP_NONE, first != 0, nan_missing && y != y, xp, z, y, n, x, logw, device);
}

extern "C" int smc_device_math(int which, const double* a, const double* b, int64_t n, double* out, int device) {
    if (!a || !out || n <= 0 || which < 0 || which > 5) return fail(SMC_EINVAL, "smc_device_math: bad argument");
    if (which >= 3 && !b) return fail(SMC_EINVAL, "smc_device_math: b required");
    DeviceCall c;
    if (const int rc = c.begin("smc_device_math", device)) return rc;
    const size_t o_a = c.take((size_t)n * 8), o_b = c.take((size_t)n * 8), o_out = c.take((size_t)n * 8);
    if (const int rc = c.use_scratch()) return rc;
    HIPCHK(c.upload(o_a, a, (size_t)n * 8));
    if (b) HIPCHK(c.upload(o_b, b, (size_t)n * 8));
    hipLaunchKernelGGL(k_device_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, which, c.at<double>(o_a), c.at<double>(o_b), n,
                       c.at<double>(o_out));
    HIPCHK(hipGetLastError());
    HIPCHK(c.download(out, o_out, (size_t)n * 8));
    HIPCHK(c.finish());
    return SMC_OK;
}

// ---- the smoother on the host (smc_spec.h "the smoother"): the twin the device is compared with, statement by statement ------
extern "C" int smc_host_transition_logpdf(int model_id, const double* raw, const double* xp, const double* x, double* out) {
    if (!raw || !xp || !x || !out) return fail(SMC_EINVAL, "smc_host_transition_logpdf: NULL argument");
    SmoothRow k;
    if (!smooth_row(model_id, raw, k))
        return fail(SMC_EINVAL, "smc_host_transition_logpdf: no transition density for this family, or a transition scale that is not positive and finite");
    (void)by_density_model(model_id, [&](auto Mt) { *out = model_logf<decltype(Mt)::value>(k, xp, x); return hipSuccess; });
    return SMC_OK;
}

// a filter that collapsed at a recorded step (all of its weights 0 there): the smoother answers NaN, the walks draw no path
static bool host_dead(int64_t T, int64_t n, const double* w /*[T][n]*/) {
    for (int64_t t = 0; t < T; ++t) {
        bool any = false;
        for (int64_t i = 0; i < n; ++i) any = any || w[(size_t)t * n + i] > 0.0;
        if (!any) return true;
    }
    return false;
}

// the selection of backward simulation (smc_spec.h): the integer weights q_l = path_weight(b[l], Mx) of the sources of positive
// weight wt[l], their sum S, r = mulhi64(u, S) for the 64-bit uniform u of the draw, and the first source at which the running sum
// passes r; -1 when S == 0
static int64_t host_path_pick_u(int64_t n, const double* wt, const double* b, double Mx, uint64_t u) {
    uint64_t S = 0;
    for (int64_t l = 0; l < n; ++l)
        if (wt[l] > 0.0) S += path_weight(b[l], Mx);
    if (!S) return -1;
    const uint64_t r = mulhi64(u, S);
    uint64_t C = 0;
    for (int64_t l = 0; l < n; ++l) {
        if (!(wt[l] > 0.0)) continue;
        C += path_weight(b[l], Mx);
        if (C > r) return l;
    }
    return -1;
}
// ... with the uniform of path p at step t (backward simulation)
static int64_t host_path_pick(int64_t n, const double* wt, const double* b, double Mx, uint64_t seed, int64_t p, uint32_t stream, int64_t t) {
    return host_path_pick_u(n, wt, b, Mx, path_uniform(seed, p, stream, (uint32_t)t));
}

// smoothed moments of one step: smc_get_moments' definitions on (x, ws) in the smoother's order of summation
static void host_smooth_moments(int d, int64_t n, const double* x /*[d][n]*/, const double* ws, bool dead, double* mean /*[d]*/, double* var) {
    const double nan = bits2d(0x7ff8000000000000ULL);
    bool any = false;
    for (int64_t i = 0; i < n; ++i) any = any || ws[i] > 0.0;
    for (int r = 0; r < d; ++r) {
        const double* xr = x + (size_t)r * n;
        const double m = smooth_sum(n, [&](int64_t i) { return ws[i] > 0.0 ? ws[i] * xr[i] : 0.0; });
        const double v = smooth_sum(n, [&](int64_t i) {
            const double e = xr[i] - m;
            return ws[i] > 0.0 ? ws[i] * (e * e) : 0.0;
        });
        mean[r] = (dead || !any) ? nan : m;
        var[r] = (dead || !any) ? nan : v;
    }
}

// cross [T-1][D][D] and resid2 [T-1][D] (both or neither): the lag-one pair moments (smc_spec.h "lag-one pair moments")
template <int MODEL>
static void host_smooth_t(const SmoothRow& k, int64_t T, int64_t n, const double* x, const double* w, double* ws, double* cross = nullptr,
                          double* resid2 = nullptr) {
    constexpr int D = model_dim<MODEL>::value;
    const size_t sx = (size_t)D * n;
    std::vector<double> X(cross ? (size_t)D * n : 0), Rs(cross ? (size_t)D * n : 0), pj(cross ? (size_t)n : 0);
    for (int64_t i = 0; i < n; ++i) ws[(size_t)(T - 1) * n + i] = w[(size_t)(T - 1) * n + i];
    std::vector<double> m((size_t)D * n), s((size_t)n), c((size_t)n), g((size_t)n), logD((size_t)n);
    for (int64_t t = T - 2; t >= 0; --t) {
        const double *xs = x + (size_t)t * sx, *xt = x + (size_t)(t + 1) * sx;   // sources (step t), targets (step t + 1)
        const double *wt = w + (size_t)t * n, *wn = ws + (size_t)(t + 1) * n;
        double* out = ws + (size_t)t * n;
        for (int64_t l = 0; l < n; ++l) {
            double xp[D], ml[D];
            for (int r = 0; r < D; ++r) xp[r] = xs[(size_t)r * n + l];
            if (!(wt[l] > 0.0)) { g[l] = -inf(); continue; }
            logf_source<MODEL>(k, xp, ml, s[l], c[l]);
            for (int r = 0; r < D; ++r) m[(size_t)r * n + l] = ml[r];
            g[l] = sp_log(wt[l]) + c[l];
        }
        auto pair = [&](int64_t l, int64_t j, double gl) {
            double ml[D], xj[D];
            for (int r = 0; r < D; ++r) { ml[r] = m[(size_t)r * n + l]; xj[r] = xt[(size_t)r * n + j]; }
            return logf_pair<MODEL>(k, ml, s[l], gl, xj);
        };
        for (int64_t j = 0; j < n; ++j) {
            if (!(wn[j] > 0.0)) continue;
            double M = -inf();
            for (int64_t l = 0; l < n; ++l) {
                if (!(wt[l] > 0.0)) continue;
                const double a = pair(l, j, g[l]);
                M = a > M ? a : M;
            }
            const double S = smooth_sum(n, [&](int64_t l) { return wt[l] > 0.0 ? sp_exp(pair(l, j, g[l]) - M) : 0.0; });
            logD[j] = M + sp_log(S);
        }
        for (int64_t i = 0; i < n; ++i) {
            if (!(wt[i] > 0.0)) { out[i] = 0.0; continue; }
            const double S = smooth_sum(n, [&](int64_t j) { return wn[j] > 0.0 ? wn[j] * sp_exp(pair(i, j, c[i]) - logD[j]) : 0.0; });
            out[i] = wt[i] * S;
        }
        if (!cross) continue;
        for (int64_t i = 0; i < n; ++i) {
            if (!(wt[i] > 0.0)) continue;   // (left out below by the select on w)
            double mi[D];
            for (int r = 0; r < D; ++r) mi[r] = m[(size_t)r * n + i];
            for (int64_t j = 0; j < n; ++j) {   // p_ij, once per pair
                if (!(wn[j] > 0.0)) continue;
                double xj[D];
                for (int r = 0; r < D; ++r) xj[r] = xt[(size_t)r * n + j];
                pj[j] = pair_prob<MODEL>(k, mi, s[i], c[i], xj, wn[j], logD[j]);
            }
            for (int r = 0; r < D; ++r) {
                const double* xr = xt + (size_t)r * n;
                X[(size_t)r * n + i] = smooth_sum(n, [&](int64_t j) { return wn[j] > 0.0 ? pair_x_term(pj[j], xr[j]) : 0.0; });
                Rs[(size_t)r * n + i] = smooth_sum(n, [&](int64_t j) { return wn[j] > 0.0 ? pair_r_term(pj[j], xr[j], mi[r]) : 0.0; });
            }
        }
        for (int a = 0; a < D; ++a)
            for (int r = 0; r < D; ++r)
                cross[((size_t)t * D + a) * D + r] =
                    smooth_sum(n, [&](int64_t i) { return wt[i] > 0.0 ? pair_cross_term(wt[i], xs[(size_t)a * n + i], X[(size_t)r * n + i]) : 0.0; });
        for (int r = 0; r < D; ++r)
            resid2[(size_t)t * D + r] = smooth_sum(n, [&](int64_t i) { return wt[i] > 0.0 ? pair_resid_term(wt[i], Rs[(size_t)r * n + i]) : 0.0; });
    }
}

extern "C" int smc_host_smooth(int model_id, const double* raw, int64_t T, int64_t n, const double* x, const double* w, double* ws,
                               double* mean, double* var) {
    if (!raw || !x || !w || !ws) return fail(SMC_EINVAL, "smc_host_smooth: NULL argument");
    if (T < 1 || n < 1) return fail(SMC_EINVAL, "smc_host_smooth: T and n must be positive");
    SmoothRow k;
    if (!smooth_row(model_id, raw, k))
        return fail(SMC_EINVAL, "smc_host_smooth: no transition density for this family, or a transition scale that is not positive and finite");
    const int d = model_dim_rt(model_id);
    (void)by_density_model(model_id, [&](auto Mt) { host_smooth_t<decltype(Mt)::value>(k, T, n, x, w, ws); return hipSuccess; });
    const bool dead = host_dead(T, n, w);   // NaN everywhere
    if (dead)
        for (size_t q = 0; q < (size_t)T * n; ++q) ws[q] = bits2d(0x7ff8000000000000ULL);
    if (mean && var)
        for (int64_t t = 0; t < T; ++t)
            host_smooth_moments(d, n, x + (size_t)t * d * n, ws + (size_t)t * n, dead, mean + (size_t)t * d, var + (size_t)t * d);
    return SMC_OK;
}

extern "C" int smc_host_smooth_pairs(int model_id, const double* raw, int64_t T, int64_t n, const double* x, const double* w, double* ws,
                                     double* mean, double* var, double* cross, double* resid2) {
    if (!raw || !x || !w || !ws || (T > 1 && (!cross || !resid2))) return fail(SMC_EINVAL, "smc_host_smooth_pairs: NULL argument");
    if (T < 1 || n < 1) return fail(SMC_EINVAL, "smc_host_smooth_pairs: T and n must be positive");
    if (T == 1) return smc_host_smooth(model_id, raw, T, n, x, w, ws, mean, var);   // no pair: cross and resid2 are empty
    SmoothRow k;
    if (!smooth_row(model_id, raw, k))
        return fail(SMC_EINVAL, "smc_host_smooth_pairs: no transition density for this family, or a transition scale that is not positive and finite");
    const int d = model_dim_rt(model_id);
    (void)by_density_model(model_id, [&](auto Mt) { host_smooth_t<decltype(Mt)::value>(k, T, n, x, w, ws, cross, resid2); return hipSuccess; });
    const bool dead = host_dead(T, n, w);   // NaN everywhere
    if (dead) {
        const double nan = bits2d(0x7ff8000000000000ULL);
        for (size_t q = 0; q < (size_t)T * n; ++q) ws[q] = nan;
        for (size_t q = 0; q < (size_t)(T - 1) * d * d; ++q) cross[q] = nan;
        for (size_t q = 0; q < (size_t)(T - 1) * d; ++q) resid2[q] = nan;
    }
    if (mean && var)
        for (int64_t t = 0; t < T; ++t)
            host_smooth_moments(d, n, x + (size_t)t * d * n, ws + (size_t)t * n, dead, mean + (size_t)t * d, var + (size_t)t * d);
    return SMC_OK;
}

// ---- quantiles of the smoothed state on the host (smc_spec.h "quantiles of the smoothed state"): the twin of k_smooth_quantiles ----
// One coordinate of one filter: x, ws [T][n] -> q [T][np].  The same integers by a sort where the device selects by radix.
extern "C" int smc_host_smooth_quantiles(int64_t T, int64_t n, const double* x, const double* ws, const double* p, int np, double* q) {
    if (!x || !ws || !p || !q) return fail(SMC_EINVAL, "smc_host_smooth_quantiles: NULL argument");
    if (T < 1 || n < 1) return fail(SMC_EINVAL, "smc_host_smooth_quantiles: T and n must be positive");
    if ((n + SMOOTH_CH - 1) / SMOOTH_CH > 65535) return fail(SMC_EINVAL, "smc_host_smooth_quantiles: more than 65535 chunks of particles");
    if (np < 1 || np > QMAX) return fail(SMC_EINVAL, "smc_host_smooth_quantiles: 1 <= np <= 8");
    for (int j = 0; j < np; ++j)
        if (!(p[j] >= 0.0 && p[j] <= 1.0)) return fail(SMC_EINVAL, "smc_host_smooth_quantiles: levels must lie in [0, 1]");
    std::vector<std::pair<uint64_t, uint64_t>> kv;   // (key, weight) of the particles that carry weight
    for (int64_t t = 0; t < T; ++t) {
        const double *xt = x + (size_t)t * n, *wt = ws + (size_t)t * n;
        double* out = q + (size_t)t * np;
        int K = SMOOTH_Q_NOBODY;
        bool bad = false;
        for (int64_t i = 0; i < n; ++i) {
            const int e = smooth_q_exponent(wt[i]);
            bad = bad || wt[i] != wt[i];
            K = e > K ? e : K;
        }
        if (bad || K == SMOOTH_Q_NOBODY) {
            for (int j = 0; j < np; ++j) out[j] = bits2d(0x7ff8000000000000ULL);
            continue;
        }
        kv.clear();
        for (int64_t i = 0; i < n; ++i) {
            const uint64_t qi = smooth_q_weight(wt[i], K);
            if (qi) kv.emplace_back(order_key(xt[i]), qi);
        }
        std::sort(kv.begin(), kv.end());
        for (size_t a = 1; a < kv.size(); ++a) kv[a].second += kv[a - 1].second;   // inclusive sums: kv.back().second = W > 0
        const uint64_t W = kv.back().second;
        for (int j = 0; j < np; ++j) {
            const uint64_t Tj = mulhi64(prob_to_u64(p[j]), W);
            // the first entry with a sum above Tj (Tj < W: there is one); equal keys are adjacent and the last of them has the sum
            // of all of them, so the entry's key is the smallest value with the weight at or below it above Tj
            size_t a = 0, b = kv.size() - 1;
            while (a < b) {
                const size_t mid = (a + b) >> 1;
                if (kv[mid].second > Tj) b = mid;
                else a = mid + 1;
            }
            out[j] = key_value(kv[a].first);
        }
    }
    return SMC_OK;
}

// ---- backward simulation on the host (smc_spec.h "backward simulation"): the specification as plain loops, one filter --------
template <int MODEL>
static void host_paths_t(const SmoothRow& k, int64_t T, int64_t n, const double* x, const double* w, int64_t M, uint64_t seed, uint32_t stream,
                         int32_t* idx, double* xs) {
    constexpr int D = model_dim<MODEL>::value;
    const size_t sx = (size_t)D * n;
    const double nan = bits2d(0x7ff8000000000000ULL);
    const bool dead = host_dead(T, n, w);   // no path
    std::vector<double> m((size_t)D * n), s((size_t)n), g((size_t)n), b((size_t)n);
    for (int64_t t = T - 1; t >= 0; --t) {
        const bool last = t == T - 1;
        const double *xt = x + (size_t)t * sx, *xn = xt + sx, *wt = w + (size_t)t * n;
        for (int64_t l = 0; l < n; ++l) {
            if (!(wt[l] > 0.0)) continue;
            if (last) { g[l] = sp_log(wt[l]); continue; }
            double xp[D], ml[D], c;
            for (int r = 0; r < D; ++r) xp[r] = xt[(size_t)r * n + l];
            logf_source<MODEL>(k, xp, ml, s[l], c);
            for (int r = 0; r < D; ++r) m[(size_t)r * n + l] = ml[r];
            g[l] = sp_log(wt[l]) + c;
        }
        for (int64_t p = 0; p < M; ++p) {
            int64_t pick = -1;
            const int64_t j = last ? 0 : idx[(size_t)(t + 1) * M + p];
            if (!dead && j >= 0) {
                double Mx = -inf();
                for (int64_t l = 0; l < n; ++l) {
                    if (!(wt[l] > 0.0)) continue;
                    if (last) b[l] = g[l];
                    else {
                        double ml[D], xj[D];
                        for (int r = 0; r < D; ++r) { ml[r] = m[(size_t)r * n + l]; xj[r] = xn[(size_t)r * n + j]; }
                        b[l] = logf_pair<MODEL>(k, ml, s[l], g[l], xj);
                    }
                    Mx = b[l] > Mx ? b[l] : Mx;
                }
                pick = host_path_pick(n, wt, b.data(), Mx, seed, p, stream, t);
            }
            idx[(size_t)t * M + p] = (int32_t)pick;
            if (xs)
                for (int r = 0; r < D; ++r) xs[((size_t)t * D + r) * M + p] = pick >= 0 ? xt[(size_t)r * n + pick] : nan;
        }
    }
}

extern "C" int smc_host_sample_paths(int model_id, const double* raw, int64_t T, int64_t n, const double* x, const double* w, int64_t M,
                                     uint64_t path_seed, uint32_t stream, int32_t* idx, double* xs) {
    if (!raw || !x || !w || !idx) return fail(SMC_EINVAL, "smc_host_sample_paths: NULL argument");
    if (T < 1 || n < 1) return fail(SMC_EINVAL, "smc_host_sample_paths: T and n must be positive");
    if (M < 1) return fail(SMC_EINVAL, "smc_host_sample_paths: M must be positive");
    if (n > PATH_MAX_N) return fail(SMC_EINVAL, "smc_host_sample_paths: more than 2^20 particles");
    SmoothRow k;
    if (!smooth_row(model_id, raw, k))
        return fail(SMC_EINVAL, "smc_host_sample_paths: no transition density for this family, or a transition scale that is not positive and finite");
    (void)by_density_model(model_id, [&](auto Mt) { host_paths_t<decltype(Mt)::value>(k, T, n, x, w, M, path_seed, stream, idx, xs); return hipSuccess; });
    return SMC_OK;
}

// ---- ancestor sampling on the host (smc_spec.h "ancestor sampling"): the twin of smc_ancestor_sweep for ONE filter ----------------
template <int MODEL>
static void host_ancestor_sweep_t(const SmoothRow& k, int64_t T, int64_t n, const double* x, const double* w, const int32_t* a, const double* xref,
                                  uint64_t seed, uint64_t path_seed, uint32_t stream, int32_t* J, int32_t* idx, double* xref_out) {
    constexpr int D = model_dim<MODEL>::value;
    const size_t sx = (size_t)D * n;
    std::vector<double> b((size_t)n);
    // the ancestor draws, every one from the OLD reference
    J[0] = -1;
    for (int64_t t = 1; t < T; ++t) {
        const double *xs = x + (size_t)(t - 1) * sx, *ws = w + (size_t)(t - 1) * n, *xr = xref + (size_t)t * D;
        double Mx = -inf();
        for (int64_t l = 0; l < n; ++l) {
            if (!(ws[l] > 0.0)) continue;
            double xp[D], ml[D], s, c;
            for (int r = 0; r < D; ++r) xp[r] = xs[(size_t)r * n + l];
            logf_source<MODEL>(k, xp, ml, s, c);
            b[l] = logf_pair<MODEL>(k, ml, s, sp_log(ws[l]) + c, xr);
            Mx = b[l] > Mx ? b[l] : Mx;
        }
        const int64_t pick = host_path_pick_u(n, ws, b.data(), Mx, anc_uniform(seed, stream, (uint32_t)t));
        J[t] = pick >= 0 ? (int32_t)pick : (int32_t)cond_slot(seed, stream, (uint32_t)(t - 1), (uint32_t)n);
    }
    // the last index: backward simulation's last step for path 0
    const double* wl = w + (size_t)(T - 1) * n;
    double Mx = -inf();
    for (int64_t l = 0; l < n; ++l) {
        if (!(wl[l] > 0.0)) continue;
        b[l] = sp_log(wl[l]);
        Mx = b[l] > Mx ? b[l] : Mx;
    }
    int32_t i = (int32_t)host_path_pick_u(n, wl, b.data(), Mx, path_uniform(path_seed, 0, stream, (uint32_t)(T - 1)));
    for (size_t q = 0; q < (size_t)T * D; ++q) xref_out[q] = xref[q];
    if (i < 0) {   // dead: the filter keeps its reference
        for (int64_t t = 0; t < T; ++t) idx[t] = -1;
        return;
    }
    idx[T - 1] = i;
    for (int64_t t = T - 1; t >= 1; --t) idx[t - 1] = i = anc_trace(i, cond_slot(seed, stream, (uint32_t)t, (uint32_t)n), J[t], a + (size_t)t * n);
    for (int64_t t = 0; t < T; ++t)
        for (int r = 0; r < D; ++r) xref_out[(size_t)t * D + r] = x[(size_t)t * sx + (size_t)r * n + idx[t]];
}

extern "C" int smc_host_ancestor_sweep(int model_id, const double* raw, int64_t T, int64_t n, const double* x, const double* w, const int32_t* a,
                                       const double* xref, uint64_t seed, uint64_t path_seed, uint32_t stream, int32_t* J, int32_t* idx,
                                       double* xref_out) {
    if (!raw || !x || !w || !a || !xref || !J || !idx || !xref_out) return fail(SMC_EINVAL, "smc_host_ancestor_sweep: NULL argument");
    if (T < 1 || n < 1) return fail(SMC_EINVAL, "smc_host_ancestor_sweep: T and n must be positive");
    if (n > PATH_MAX_N) return fail(SMC_EINVAL, "smc_host_ancestor_sweep: more than 2^20 particles");
    SmoothRow k;
    if (!smooth_row(model_id, raw, k))
        return fail(SMC_EINVAL, "smc_host_ancestor_sweep: no transition density for this family, or a transition scale that is not positive and finite");
    for (size_t q = (size_t)n; q < (size_t)T * n; ++q)
        if (a[q] < 0 || (int64_t)a[q] >= n) return fail(SMC_EINVAL, "smc_host_ancestor_sweep: a[" + std::to_string(q / n) + "] holds an entry outside [0, n)");
    (void)by_density_model(model_id, [&](auto Mt) {
        host_ancestor_sweep_t<decltype(Mt)::value>(k, T, n, x, w, a, xref, seed, path_seed, stream, J, idx, xref_out);
        return hipSuccess;
    });
    return SMC_OK;
}

// ---- Rao-Blackwellised backward simulation on the host (smc_spec.h; the twin of smc_rb_sample_paths for ONE filter) -------------
extern "C" int smc_host_rb_sample_paths(const double* raw, int64_t T, int64_t n, const double* x, const double* w, const double* y, int64_t M,
                                        uint64_t path_seed, uint32_t stream, int32_t* idx, double* vol, double* tmean, double* tvar, double* tdraw,
                                        double* out) {
    if (!raw || !x || !w || !y || !idx || !vol || !tmean || !tvar) return fail(SMC_EINVAL, "smc_host_rb_sample_paths: NULL argument");
    if (T < 1 || n < 1) return fail(SMC_EINVAL, "smc_host_rb_sample_paths: T and n must be positive");
    if (M < 1 || M > ((int64_t)1 << 30)) return fail(SMC_EINVAL, "smc_host_rb_sample_paths: M must be in [1, 2^30]");
    if (n > PATH_MAX_N) return fail(SMC_EINVAL, "smc_host_rb_sample_paths: more than 2^20 particles");
    for (int64_t t = 0; t < T; ++t)
        if (!(y[t] - y[t] == 0.0)) return fail(SMC_EINVAL, "smc_host_rb_sample_paths: y is not finite");
    SmoothRow k;
    if (!smooth_row(MODEL_UCSV3D, raw, k)) return fail(SMC_EINVAL, "smc_host_rb_sample_paths: a gamma is not a positive finite number");
    const size_t sx = (size_t)4 * n;
    const double nan = bits2d(0x7ff8000000000000ULL);
    const bool dead = host_dead(T, n, w);   // no path
    std::vector<double> sv((size_t)RB_NV * n), b((size_t)n), own((size_t)4 * M, 0.0);
    for (int64_t t = T - 1; t >= 0; --t) {
        const bool last = t == T - 1;
        const double *xt = x + (size_t)t * sx, *wt = w + (size_t)t * n;
        for (int64_t l = 0; l < n; ++l) {
            if (!(wt[l] > 0.0)) continue;
            const double xs[4] = {xt[l], xt[(size_t)n + l], xt[(size_t)2 * n + l], xt[(size_t)3 * n + l]};
            rb_source(last, xs, wt[l], &sv[(size_t)RB_NV * l]);
        }
        for (int64_t p = 0; p < M; ++p) {
            int64_t pick = -1;
            double* o = &own[(size_t)4 * p];
            if (!dead && (last || idx[(size_t)(t + 1) * M + p] >= 0)) {
                const double first[4] = {0.0, 0.0, 0.0, 1.0};
                const double* oo = last ? first : o;
                double Mx = -inf();
                for (int64_t l = 0; l < n; ++l) {
                    if (!(wt[l] > 0.0)) continue;
                    b[l] = rb_pair(k, &sv[(size_t)RB_NV * l], oo);
                    Mx = b[l] > Mx ? b[l] : Mx;
                }
                pick = host_path_pick(n, wt, b.data(), Mx, path_seed, p, stream, t);
            }
            idx[(size_t)t * M + p] = (int32_t)pick;
            double lse = nan, lsn = nan;
            if (pick >= 0) {
                lse = xt[(size_t)n + pick];
                lsn = xt[(size_t)2 * n + pick];
                double mu = last ? 0.0 : o[2], tau = last ? 0.0 : o[3];
                rb_info(last, lse, lsn, y[t], mu, tau);
                o[0] = lse; o[1] = lsn; o[2] = mu; o[3] = tau;
            }
            vol[((size_t)t * 2) * M + p] = lse;
            vol[((size_t)t * 2 + 1) * M + p] = lsn;
        }
    }
    // the trend pass
    for (int64_t p = 0; p < M; ++p) {
        if (idx[p] < 0) {
            for (int64_t t = 0; t < T; ++t) {
                tmean[(size_t)t * M + p] = tvar[(size_t)t * M + p] = nan;
                if (tdraw) tdraw[(size_t)t * M + p] = nan;
            }
            continue;
        }
        double m = 0.0, P = 0.0, lse_prev = 0.0;
        for (int64_t t = 0; t < T; ++t) {
            rb_trend_step(raw, t == 0, lse_prev, vol[((size_t)t * 2 + 1) * M + p], y[t], m, P);
            tmean[(size_t)t * M + p] = m;
            tvar[(size_t)t * M + p] = P;
            lse_prev = vol[((size_t)t * 2) * M + p];
        }
        double xs = m, Ps = P, xd = 0.0;
        if (tdraw) tdraw[(size_t)(T - 1) * M + p] = xd = rts_path_last(m, P, rb_trend_normal(path_seed, p, stream, (uint32_t)(T - 1)));
        for (int64_t t = T - 2; t >= 0; --t) {
            const double Q = sp_exp(vol[((size_t)t * 2) * M + p]);
            const double mf = tmean[(size_t)t * M + p], Pf = tvar[(size_t)t * M + p];
            rts_back(1.0, Q, mf, Pf, xs, Ps);
            tmean[(size_t)t * M + p] = xs;
            tvar[(size_t)t * M + p] = Ps;
            if (tdraw) tdraw[(size_t)t * M + p] = xd = rts_path_back(1.0, Q, mf, Pf, xd, rb_trend_normal(path_seed, p, stream, (uint32_t)t));
        }
    }
    // the summary over the complete paths
    if (out) {
        int64_t cnt = 0;
        for (int64_t p = 0; p < M; ++p) cnt += idx[p] >= 0 ? 1 : 0;
        const double dcnt = (double)cnt;
        for (int64_t t = 0; t < T; ++t) {
            const double* series[4] = {tmean + (size_t)t * M, tvar + (size_t)t * M, vol + ((size_t)t * 2) * M, vol + ((size_t)t * 2 + 1) * M};
            const int col_mean[4] = {0, 1, 3, 5}, col_var[4] = {2, -1, 4, 6};
            double* o = out + (size_t)t * 8;
            for (int r = 0; r < 4; ++r) {
                const double* v = series[r];
                const double mean = smooth_sum(M, [&](int64_t p) { return idx[p] >= 0 ? v[p] : 0.0; }) / dcnt;
                o[col_mean[r]] = cnt ? mean : nan;
                if (col_var[r] >= 0) {
                    const double var = smooth_sum(M, [&](int64_t p) { const double e = v[p] - mean; return idx[p] >= 0 ? e * e : 0.0; }) / dcnt;
                    o[col_var[r]] = cnt ? var : nan;
                }
            }
            o[7] = dcnt;
        }
    }
    return SMC_OK;
}
