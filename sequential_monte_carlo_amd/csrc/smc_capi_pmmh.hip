// smc_capi_pmmh.hip -- PMMH rejuvenation on the device (rejuvenate!, smc_samplers.jl:103-146): smc_pmmh_configure,
// smc_pmmh_rejuvenate and their kernels (smc_pmmh_kernels.h).
#include "smc_host.h"
#include "smc_pmmh_kernels.h"

#include <cmath>
#include <cstring>

using namespace smc;

extern "C" int smc_pmmh_configure(smc_handle h, int d_theta, const int32_t* prior_family, const double* prior_par,
                                  const int32_t* raw_from, const double* raw_const) {
    if (!h || !prior_family || !prior_par || !raw_from || !raw_const) return fail(SMC_EINVAL, "smc_pmmh_configure: NULL argument");
    if (d_theta < 1 || d_theta > MAX_DTHETA) return fail(SMC_EINVAL, "smc_pmmh_configure: 1 <= d_theta <= 8");
    PmmhSpec sp{};
    sp.d = d_theta;
    for (int i = 0; i < d_theta; ++i) {
        if (prior_family[i] < PRIOR_UNIFORM || prior_family[i] > PRIOR_LOGNORMAL)
            return fail(SMC_EINVAL, "smc_pmmh_configure: unknown prior family " + std::to_string(prior_family[i]));
        sp.family[i] = prior_family[i];
        for (int k = 0; k < PRIOR_NPAR; ++k) sp.par[i][k] = prior_par[(size_t)i * PRIOR_NPAR + k];
    }
    sp.nraw = model_nraw_rt(h->model);
    for (int k = 0; k < sp.nraw; ++k) {
        if (raw_from[k] >= d_theta) return fail(SMC_EINVAL, "smc_pmmh_configure: raw_from index out of range");
        sp.raw_from[k] = raw_from[k];
        sp.raw_const[k] = raw_const[k];
    }
    HIPCHK(hipSetDevice(h->device));
    const size_t nt = (size_t)h->v.ntheta;
    if (!h->pm.d_in) {
        // what a rejuvenation call uploads or clears sits in ONE block (8-byte words): theta | logZ | chol | nrun | counts | any
        const size_t w_theta = nt * MAX_DTHETA, w_chol = (size_t)MAX_DTHETA * MAX_DTHETA, w_any = (nt + 7) / 8;
        const size_t in_bytes = (w_theta + nt + w_chol + 2 + w_any) * 8;
        HIPCHK(h->pm.d_in.grow(in_bytes));
        HIPCHK(h->pm.h_in.grow(in_bytes));
        h->pm.dev.theta = h->pm.d_in.as<double>();
        h->pm.dev.logZ = h->pm.dev.theta + w_theta;
        h->pm.dev.chol = h->pm.dev.logZ + nt;
        h->pm.dev.nrun = (unsigned long long*)(h->pm.dev.chol + w_chol);
        h->pm.dev.counts = (int32_t*)(h->pm.dev.nrun + 1);
        h->pm.dev.any = (unsigned char*)(h->pm.dev.nrun + 2);
        HIPCHK(h->pm.d_prop.grow(nt * MAX_DTHETA * 8));
        HIPCHK(h->pm.d_lp.grow(nt * 2 * 8));
        HIPCHK(h->pm.d_skip.grow(nt));
        HIPCHK(h->pm.d_mask.grow(nt));
        HIPCHK(h->pm.d_order.grow(nt * 4));
        h->pm.dev.prop = h->pm.d_prop.as<double>(); h->pm.dev.lp = h->pm.d_lp.as<double>();
        h->pm.dev.skip = h->pm.d_skip.as<unsigned char>(); h->pm.dev.mask = h->pm.d_mask.as<unsigned char>();
        h->pm.dev.order = h->pm.d_order.as<int32_t>();
        HIPCHK(h->pm.h_out.grow((nt * (MAX_DTHETA + 2) + 1) * 8));
    }
    h->pm.spec = sp;
    h->pm.cfg = true;
    return SMC_OK;
}

__global__ void k_pmmh_export(int ntheta, int d, PmmhDev p, double* out) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= ntheta) return;
    for (int i = 0; i < d; ++i) out[(size_t)m * d + i] = p.theta[(size_t)m * MAX_DTHETA + i];
    out[(size_t)ntheta * d + m] = p.logZ[m];
    out[(size_t)ntheta * (d + 1) + m] = p.any[m] ? 1.0 : 0.0;
    if (m == 0) out[(size_t)ntheta * (d + 2)] = (double)*p.nrun;
}

extern "C" int smc_pmmh_rejuvenate(smc_handle h, smc_handle main, const double* y, int64_t T, double xi, const double* chol,
                                   const double* scales, int chain, const uint64_t* filter_seeds, uint64_t move_seed,
                                   double* theta, double* logZ, uint8_t* accepted, int64_t* filters_run) {
    if (!h || !y || !chol || !scales || !filter_seeds || !theta || !logZ) return fail(SMC_EINVAL, "smc_pmmh_rejuvenate: NULL argument");
    if (conditional(h) || (main && conditional(main))) return cond_refuse("smc_pmmh_rejuvenate");
    if (!h->pm.cfg) return fail(SMC_ESTATE, "smc_pmmh_rejuvenate: smc_pmmh_configure has not been called");
    if (T <= 0 || chain < 0) return fail(SMC_EINVAL, "smc_pmmh_rejuvenate: bad T or chain");
    if (history_armed(h) || (main && history_armed(main))) return history_refuse("smc_pmmh_rejuvenate");
    if (main) {
        if (main == h) return fail(SMC_EINVAL, "smc_pmmh_rejuvenate: main and proposal handles are the same");
        const FilterView &a = main->v, &b = h->v;
        if (main->model != h->model || a.n != b.n || a.seg != b.seg || a.ntheta != b.ntheta || main->device != h->device)
            return fail(SMC_EINVAL, "smc_pmmh_rejuvenate: handles differ in model, geometry or device");
        if (!main->inited) return fail(SMC_ESTATE, "smc_pmmh_rejuvenate: main filters not initialised");
        main->win.k = 0;
    }
    h->win.k = 0;
    HIPCHK(hipSetDevice(h->device));
    const PmmhSpec& sp = h->pm.spec;
    const int nt = h->v.ntheta, d = sp.d;
    int rc = ensure_y(h, T);
    if (rc) return rc;
    const bool resident = h->resident_ok && resident_supported(h->model, h->v.seg);
    if (resident && (rc = ensure_recs(h, T))) return rc;
    if (main) {   // its pending emission, then an idle stream: the accept copies below run on the proposal handle's stream
        if ((rc = emit_if_needed(main))) return rc;
        HIPCHK(hipStreamSynchronize(main->stream));
    }
    {   // theta (rows padded to MAX_DTHETA), logZ, the Cholesky factor and the zeros of nrun / counts / any: one pinned block, one copy
        // (the previous call's copy has completed: every call ends with a stream synchronisation)
        double* in = h->pm.h_in.as<double>();
        memset(in, 0, h->pm.h_in.bytes());
        for (int m = 0; m < nt; ++m)
            for (int i = 0; i < d; ++i) in[(size_t)m * MAX_DTHETA + i] = theta[(size_t)m * d + i];
        double* in_logZ = in + (size_t)nt * MAX_DTHETA;
        memcpy(in_logZ, logZ, (size_t)nt * 8);
        double* in_chol = in_logZ + nt;
        for (int i = 0; i < d * d; ++i) in_chol[i] = chol[i];
    }
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_y.as<double>(), y, (size_t)T * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->pm.d_in.as<double>(), h->pm.h_in.as<double>(), h->pm.h_in.bytes(), hipMemcpyHostToDevice, h->stream));
    const dim3 grid((unsigned)((nt + 127) / 128)), block(128);
    GapScope gaps(h, y, T);   // (a flagged handle: the proposal filters read a NaN as a gap, like smc_log_likelihood)
    for (int c = 0; c < chain; ++c) {
        hipLaunchKernelGGL(k_pmmh_propose, grid, block, 0, h->stream, h->v, sp, h->pm.dev, h->model, move_seed, (uint32_t)c,
                           sqrt(scales[c]), h->d_params);   // (derives the proposal rows of a guided handle too)
        HIPCHK(hipGetLastError());
        h->have_params = true;
        hot_invalidate(h);                     // the rows were written on the device
        h->v.seed = filter_seeds[c];
        h->brk_count = 0;                      // cached break points belong to the previous seed
        h->v.skip = h->pm.dev.skip; h->v.order = h->pm.dev.order; h->v.n_active = h->pm.dev.counts;
        rc = enqueue_log_likelihood(h, y[0], T, false);
        h->v.skip = nullptr; h->v.order = nullptr; h->v.n_active = nullptr;
        if (rc) return rc;
        hipLaunchKernelGGL(k_pmmh_accept, grid, block, 0, h->stream, h->v, h->pm.dev, d, move_seed, (uint32_t)c, xi);
        HIPCHK(hipGetLastError());
        // smc.x[m], smc.w[m] <- x_prop, w_prop of the accepted particles (smc_samplers.jl:132-133)
        if (main) {
            HIPCHK(copy_slots(main->v, main->cur, h->v, h->cur, main->d, h->pm.dev.mask, h->stream));
            hot_invalidate(main);
        }
    }
    hipLaunchKernelGGL(k_pmmh_export, grid, block, 0, h->stream, nt, d, h->pm.dev, h->pm.h_out.as<double>());
    HIPCHK(hipGetLastError());
    if ((rc = finish_elapsed(h))) return rc;
    if (main && chain > 0) main->t = h->t;
    const double* res = h->pm.h_out.as<double>();
    memcpy(theta, res, (size_t)nt * d * 8);
    memcpy(logZ, res + (size_t)nt * d, (size_t)nt * 8);
    if (accepted)
        for (int m = 0; m < nt; ++m) accepted[m] = res[(size_t)nt * (d + 1) + m] != 0.0 ? 1 : 0;
    if (filters_run) *filters_run = (int64_t)res[(size_t)nt * (d + 2)];
    return SMC_OK;
}
