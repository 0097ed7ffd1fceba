// smc_rb_kernels.h -- what follows the backward walk of a MODEL_UCSV_RB record (smc_spec.h "Rao-Blackwellised backward
// simulation"): the exact trend of every drawn volatility path, and the summary over the paths of a filter.
// The walk itself is the pair policy of MODEL_UCSV_RB in smc_path_kernels.h.  wave64, f64.  Included by smc_capi_smooth.hip only.
#pragma once
#include "smc_path_kernels.h"

namespace smc {

struct RbTrendArgs {
    int64_t T, M;
    int ntheta;
    uint64_t seed;           // path seed
    const Params* params;    // [ntheta] the rows the steps ran with
    const uint32_t* stream;  // [ntheta] Philox stream ids
    const double* y;         // [T]
    const int32_t* idx0;     // [ntheta][M] idx[0]: a path is complete iff it is >= 0
    const double* vol;       // [T][2][ntheta][M] the chosen (lse, lsn)
    double* tmean;           // [T][ntheta][M]
    double* tvar;            // [T][ntheta][M]
    double* tdraw;           // [T][ntheta][M] or nullptr
};

// One thread per path, serial in t: the forward Kalman pass leaves (m_t, P_t) in tmean / tvar, the backward pass replaces
// them in place by the RTS moments and draws the joint trend path.  Consecutive threads touch consecutive words at every t.
__global__ void k_rb_trend(RbTrendArgs a) {
    const int th = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.M) return;
    const size_t pw = (size_t)a.ntheta * a.M, o = (size_t)th * a.M + p;
    if (a.idx0[o] < 0) {
        const double nan = bits2d(0x7ff8000000000000ULL);
        for (int64_t t = 0; t < a.T; ++t) {
            a.tmean[(size_t)t * pw + o] = nan;
            a.tvar[(size_t)t * pw + o] = nan;
            if (a.tdraw) a.tdraw[(size_t)t * pw + o] = nan;
        }
        return;
    }
    const double* raw = a.params[th].raw;
    const uint32_t stream = a.stream[th];
    double m = 0.0, P = 0.0, lse_prev = 0.0;
    for (int64_t t = 0; t < a.T; ++t) {
        const double lse = a.vol[((size_t)t * 2) * pw + o], lsn = a.vol[((size_t)t * 2 + 1) * pw + o];
        rb_trend_step(raw, t == 0, lse_prev, lsn, a.y[t], m, P);
        a.tmean[(size_t)t * pw + o] = m;
        a.tvar[(size_t)t * pw + o] = P;
        lse_prev = lse;
    }
    double xs = m, Ps = P, xd = 0.0;
    if (a.tdraw) {
        xd = rts_path_last(m, P, rb_trend_normal(a.seed, p, stream, (uint32_t)(a.T - 1)));
        a.tdraw[(size_t)(a.T - 1) * pw + o] = xd;
    }
    for (int64_t t = a.T - 2; t >= 0; --t) {
        const double Q = sp_exp(a.vol[((size_t)t * 2) * pw + o]);
        const double mf = a.tmean[(size_t)t * pw + o], Pf = a.tvar[(size_t)t * pw + o];
        rts_back(1.0, Q, mf, Pf, xs, Ps);
        a.tmean[(size_t)t * pw + o] = xs;
        a.tvar[(size_t)t * pw + o] = Ps;
        if (a.tdraw) {
            xd = rts_path_back(1.0, Q, mf, Pf, xd, rb_trend_normal(a.seed, p, stream, (uint32_t)t));
            a.tdraw[(size_t)t * pw + o] = xd;
        }
    }
}

// The summary over the complete paths among the first counts[th] of filter th at step t: grid (T, ntheta), one workgroup per
// (step, filter), in the order of k_smooth_moments (chunks of SMOOTH_CH paths, plain adds, the partials in ascending order,
// centred second pass).  tmp [T][ntheta][nchunk] holds the chunk partials, nchunk = chunks of M.  out [T][ntheta][8]
__global__ void k_rb_summary(int64_t M, int ntheta, int nchunk, const int32_t* idx0 /*[ntheta][M]*/, const int32_t* counts,
                             const double* tmean, const double* tvar, const double* vol, double* tmp, double* out) {
    __shared__ double s_mean;
    __shared__ int s_cnt;
    const int t = blockIdx.x, th = blockIdx.y;
    const size_t pw = (size_t)ntheta * M;
    const int64_t cnt_th = counts[th];
    const int32_t* i0 = idx0 + (size_t)th * M;
    double* part = tmp + ((size_t)t * ntheta + th) * nchunk;
    double* o = out + ((size_t)t * ntheta + th) * 8;
    const double nan = bits2d(0x7ff8000000000000ULL);
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int64_t p = threadIdx.x; p < cnt_th; p += blockDim.x) mine += i0[p] >= 0 ? 1 : 0;
    if (mine) atomicAdd(&s_cnt, mine);   // (an integer count: exact in any order)
    __syncthreads();
    const int cnt = s_cnt;
    const double dcnt = (double)cnt;
    // the four series and where their moments go: (mean column, variance column or -1)
    const double* series[4] = {tmean + (size_t)t * pw, tvar + (size_t)t * pw, vol + ((size_t)t * 2) * pw, vol + ((size_t)t * 2 + 1) * pw};
    const int col_mean[4] = {0, 1, 3, 5}, col_var[4] = {2, -1, 4, 6};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double* v = series[r] + (size_t)th * M;
        for (int pass = 0; pass < (col_var[r] < 0 ? 1 : 2); ++pass) {
            const double mean = pass ? s_mean : 0.0;
            for (int c = threadIdx.x; c < nchunk; c += blockDim.x) {
                const int64_t p0 = (int64_t)c * SMOOTH_CH, p1 = p0 + SMOOTH_CH < cnt_th ? p0 + SMOOTH_CH : cnt_th;
                double s = 0.0;
                for (int64_t p = p0; p < p1; ++p) {
                    const double e = v[p] - mean;
                    s += i0[p] >= 0 ? (pass ? e * e : v[p]) : 0.0;
                }
                part[c] = s;
            }
            __syncthreads();   // (the partials a workgroup wrote to global memory are visible to its own threads after the barrier)
            if (threadIdx.x == 0) {
                double tot = 0.0;
                for (int c = 0; c < nchunk; ++c) tot += part[c];
                const double res = tot / dcnt;
                if (!pass) s_mean = res;
                o[pass ? col_var[r] : col_mean[r]] = cnt ? res : nan;
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) o[7] = dcnt;
}

}  // namespace smc
