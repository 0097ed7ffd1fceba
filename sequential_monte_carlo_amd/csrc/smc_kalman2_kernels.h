// smc_kalman2_kernels.h -- the exact Kalman filter and RTS smoother of two-state linear models with a scalar observation
// (smc_spec.h "the exact Kalman filter of a TWO-STATE linear model"; src/kalman_filter.jl:3-27, 55-70), batched over parameter
// rows.  Included by smc_kalman2.hip only.
//
//   k_kalman2_loglik   the whole series per row: (x_T [2], Sigma_T [3], logZ)
//   k_kalman2_smooth   the filter writes its record, then the backward walk over it: xs [T][n][2], Ps [T][n][3]
// and the IBIS sampler over such rows, the twins of smc_ibis_kernels.h on the same IbisView (x [M][2], S [M][3], raw [M][15]):
//   k_ibis2_init, k_ibis2_reset, k_ibis2_window, k_ibis2_rejuvenate, k_ibis2_permute
// Everything else a handle launches (the ESS records' reductions, the resampler, the moments of the theta cloud) reads theta,
// logw and M alone and serves both kinds of handle.
//
// One lane per row or parameter particle, one wave per workgroup, f64.  The row (15 doubles) and the state (5) live in registers;
// y[t] is the same address in every lane (the compiler reads it through the scalar cache).  No LDS, no float atomics; every
// store is a plain vector store of the lane's own entries.
#pragma once
#include "smc_ibis_view.h"

namespace smc {

constexpr int KALMAN2_THREADS = 64;

__global__ __launch_bounds__(KALMAN2_THREADS) void k_kalman2_loglik(const double* raw /*[n][LG2_NRAW]*/, int64_t n, const double* y, int64_t T,
                                                                    int predict_first, double* out /*[n][6]*/) {
    const int64_t m = (int64_t)blockIdx.x * KALMAN2_THREADS + threadIdx.x;
    if (m >= n) return;
    double r[LG2_NRAW];
#pragma unroll
    for (int k = 0; k < LG2_NRAW; ++k) r[k] = raw[m * LG2_NRAW + k];
    double x1 = r[LG2_X1], x2 = r[LG2_X2], S11 = r[LG2_S11], S21 = r[LG2_S21], S22 = r[LG2_S22], logZ = 0.0;
    for (int64_t t = 0; t < T; ++t) logZ += kalman2_step(r, predict_first != 0 || t > 0, y[t], x1, x2, S11, S21, S22);
    double* o = out + m * 6;
    o[0] = x1; o[1] = x2; o[2] = S11; o[3] = S21; o[4] = S22; o[5] = logZ;
}

// xs, Ps hold the filtered record after the forward loop; the backward walk overwrites entry t with the smoothed one after it
// has read it.  A lane reads back only what it stored itself.
__global__ __launch_bounds__(KALMAN2_THREADS) void k_kalman2_smooth(const double* raw /*[n][LG2_NRAW]*/, int64_t n, const double* y, int64_t T,
                                                                    int predict_first, double* xs /*[T][n][2]*/, double* Ps /*[T][n][3]*/) {
    const int64_t m = (int64_t)blockIdx.x * KALMAN2_THREADS + threadIdx.x;
    if (m >= n) return;
    double r[LG2_NRAW];
#pragma unroll
    for (int k = 0; k < LG2_NRAW; ++k) r[k] = raw[m * LG2_NRAW + k];
    double x1 = r[LG2_X1], x2 = r[LG2_X2], S11 = r[LG2_S11], S21 = r[LG2_S21], S22 = r[LG2_S22];
    const size_t sn = (size_t)n, sm = (size_t)m;
    for (int64_t t = 0; t < T; ++t) {
        (void)kalman2_step(r, predict_first != 0 || t > 0, y[t], x1, x2, S11, S21, S22);
        double* a = xs + ((size_t)t * sn + sm) * 2;
        double* P = Ps + ((size_t)t * sn + sm) * 3;
        a[0] = x1; a[1] = x2;
        P[0] = S11; P[1] = S21; P[2] = S22;
    }
    for (int64_t t = T - 2; t >= 0; --t) {
        double* a = xs + ((size_t)t * sn + sm) * 2;
        double* P = Ps + ((size_t)t * sn + sm) * 3;
        rts2_step(r, a[0], a[1], P[0], P[1], P[2], x1, x2, S11, S21, S22);
        a[0] = x1; a[1] = x2;
        P[0] = S11; P[1] = S21; P[2] = S22;
    }
}

// ---- the IBIS sampler over two-state rows ---------------------------------------------------------------------------------------
// smc.model(theta) as a gather without a run-time index into registers: row[k] = theta[raw_from[k]] or raw_const[k]
template <int D>
__device__ __forceinline__ void ibis2_row(const Lg2Map& s, const double* th, double* row) {
#pragma unroll
    for (int k = 0; k < LG2_NRAW; ++k) {
        double v = s.raw_const[k];
        const int from = s.raw_from[k];
#pragma unroll
        for (int i = 0; i < D; ++i) v = from == i ? th[i] : v;
        row[k] = v;
    }
}

// theta -> rows and the initial state of every particle   ibis.jl:38-43
template <int D>
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis2_init(IbisView v, int cp, int cs, Lg2Map s) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    if (m >= v.M) return;
    double th[D], row[LG2_NRAW];
#pragma unroll
    for (int i = 0; i < D; ++i) th[i] = v.theta[cp][m * MAX_DTHETA + i];
    ibis2_row<D>(s, th, row);
#pragma unroll
    for (int k = 0; k < LG2_NRAW; ++k) v.raw[cp][m * LG2_NRAW + k] = row[k];
    v.x[cs][m * 2] = row[LG2_X1]; v.x[cs][m * 2 + 1] = row[LG2_X2];
    v.S[cs][m * 3] = row[LG2_S11]; v.S[cs][m * 3 + 1] = row[LG2_S21]; v.S[cs][m * 3 + 2] = row[LG2_S22];
    v.logZ[cs][m] = 0.0;
    v.logw[cs][m] = 0.0;
}

// The same state from the rows alone: the beginning of a whole-series filter (density_tempered's first pass)
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis2_reset(IbisView v, int cp, int cs) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    if (m >= v.M) return;
    const double* row = v.raw[cp] + m * LG2_NRAW;
    v.x[cs][m * 2] = row[LG2_X1]; v.x[cs][m * 2 + 1] = row[LG2_X2];
    v.S[cs][m * 3] = row[LG2_S11]; v.S[cs][m * 3 + 1] = row[LG2_S21]; v.S[cs][m * 3 + 2] = row[LG2_S22];
    v.logZ[cs][m] = 0.0;
    v.logw[cs][m] = 0.0;
}

// k steps of smc²! (ibis.jl:166-187) from the committed state (set cs), as k_ibis_window: kalman2_step per step, logw and logZ
// gain its value, and with RECORD lik [k][M] (optional) and the segment records of reweight(logw) after every step.  The end
// state goes to the set `dst`.  Lanes beyond the cloud compute on the last particle and store nothing.
template <bool RECORD>
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis2_window(IbisView v, int cp, int cs, int dst, const double* y, int k, int predict0,
                                                              double* lik /*[k][M] or null*/, uint64_t* rec /*[k][nseg][4]*/) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    const bool valid = m < v.M;
    const int64_t mm = valid ? m : v.M - 1;
    double r[LG2_R + 1];
#pragma unroll
    for (int i = 0; i <= LG2_R; ++i) r[i] = v.raw[cp][mm * LG2_NRAW + i];
    double x1 = v.x[cs][mm * 2], x2 = v.x[cs][mm * 2 + 1];
    double S11 = v.S[cs][mm * 3], S21 = v.S[cs][mm * 3 + 1], S22 = v.S[cs][mm * 3 + 2];
    double logZ = v.logZ[cs][mm], logw = v.logw[cs][mm];
    const int64_t nseg = (v.M + IBIS_OSEG - 1) / IBIS_OSEG;
    for (int j = 0; j < k; ++j) {
        const double l = kalman2_step(r, j > 0 || predict0 != 0, y[j], x1, x2, S11, S21, S22);
        logw = logw + l;
        logZ = logZ + l;
        if (RECORD) {
            if (lik && valid) lik[(size_t)j * (size_t)v.M + (size_t)m] = l;
            ibis_outer_record(logw, valid, m, rec + (size_t)j * (size_t)nseg * 4);
        }
    }
    if (valid) {
        v.x[dst][m * 2] = x1; v.x[dst][m * 2 + 1] = x2;
        v.S[dst][m * 3] = S11; v.S[dst][m * 3 + 1] = S21; v.S[dst][m * 3 + 2] = S22;
        v.logZ[dst][m] = logZ;
        v.logw[dst][m] = logw;
    }
}

// rejuvenate!(ibis, y, xi) (ibis.jl:86-125) in one launch, one lane per parameter particle: k_ibis_rejuvenate statement by
// statement with the two-state row and kalman2_step.  A wave none of whose lanes proposed inside the support leaves the
// re-filter of that chain position out (the ballot is uniform over the wave; a lane outside the support never accepts, so what
// its filter would have returned is not read).
template <int D>
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis2_rejuvenate(IbisView v, int cp, int cs, PmmhSpec s, Lg2Map map, const double* y, int64_t T,
                                                                  int predict_first, double xi, const double* chol, const double* sq,
                                                                  int chain, uint64_t move_seed, unsigned char* moved,
                                                                  unsigned long long* n_moved) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    const bool valid = m < v.M;
    const int64_t mm = valid ? m : v.M - 1;
    const uint32_t stream = (uint32_t)mm;
    double th[D], row[LG2_NRAW];
#pragma unroll
    for (int i = 0; i < D; ++i) th[i] = v.theta[cp][mm * MAX_DTHETA + i];
#pragma unroll
    for (int k = 0; k < LG2_NRAW; ++k) row[k] = v.raw[cp][mm * LG2_NRAW + k];
    double x1 = v.x[cs][mm * 2], x2 = v.x[cs][mm * 2 + 1];
    double S11 = v.S[cs][mm * 3], S21 = v.S[cs][mm * 3 + 1], S22 = v.S[cs][mm * 3 + 2], logZ = v.logZ[cs][mm];
    bool any = false;
    for (int c = 0; c < chain; ++c) {
        double pr[D], prow[LG2_NRAW];
        pmmh_propose<D>(s, move_seed, stream, (uint32_t)c, th, chol, sq[c], pr);
        const bool ok = pmmh_insupport<D>(s, pr);
        ibis2_row<D>(map, pr, prow);
        const double lpp = pmmh_logprior<D>(s, pr), lpc = pmmh_logprior<D>(s, th);
        double xp1 = prow[LG2_X1], xp2 = prow[LG2_X2], Sp11 = prow[LG2_S11], Sp21 = prow[LG2_S21], Sp22 = prow[LG2_S22], logZp = 0.0;
        if (__ballot(ok) != 0)
            for (int64_t t = 0; t < T; ++t) logZp += kalman2_step(prow, predict_first != 0 || t > 0, y[t], xp1, xp2, Sp11, Sp21, Sp22);
        const double likelihood_ratio = xi * (logZp - logZ), prior_ratio = lpp - lpc;
        const double acc_ratio = likelihood_ratio + prior_ratio, log_post_prop = logZp + lpp;
        const bool acc = ok && log_post_prop > -inf() && pmmh_log_uniform(move_seed, stream, (uint32_t)c) < acc_ratio;
#pragma unroll
        for (int i = 0; i < D; ++i) th[i] = acc ? pr[i] : th[i];
#pragma unroll
        for (int k = 0; k < LG2_NRAW; ++k) row[k] = acc ? prow[k] : row[k];
        logZ = acc ? logZp : logZ;
        x1 = acc ? xp1 : x1; x2 = acc ? xp2 : x2;
        S11 = acc ? Sp11 : S11; S21 = acc ? Sp21 : S21; S22 = acc ? Sp22 : S22;
        any = any || acc;
    }
    any = any && valid;
    if (valid) {
#pragma unroll
        for (int i = 0; i < D; ++i) v.theta[cp][m * MAX_DTHETA + i] = th[i];
#pragma unroll
        for (int k = 0; k < LG2_NRAW; ++k) v.raw[cp][m * LG2_NRAW + k] = row[k];
        v.x[cs][m * 2] = x1; v.x[cs][m * 2 + 1] = x2;
        v.S[cs][m * 3] = S11; v.S[cs][m * 3 + 1] = S21; v.S[cs][m * 3 + 2] = S22;
        v.logZ[cs][m] = logZ;
        v.logw[cs][m] = 0.0;
        moved[m] = any ? 1 : 0;
    }
    const unsigned long long cnt = (unsigned long long)__popcll(__ballot(any));   // one integer add per wave: order-free
    if (threadIdx.x == 0 && cnt) atomicAdd(n_moved, cnt);
}

// resample!(ibis) (ibis.jl:73-84): particle m <- particle a[m], a value copy of everything it owns, into the other buffers
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis2_permute(IbisView v, int cp, int cs, const int32_t* a) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    if (m >= v.M) return;
    const int64_t src = a[m];
#pragma unroll
    for (int i = 0; i < MAX_DTHETA; ++i) v.theta[cp ^ 1][m * MAX_DTHETA + i] = v.theta[cp][src * MAX_DTHETA + i];
#pragma unroll
    for (int k = 0; k < LG2_NRAW; ++k) v.raw[cp ^ 1][m * LG2_NRAW + k] = v.raw[cp][src * LG2_NRAW + k];
#pragma unroll
    for (int i = 0; i < 2; ++i) v.x[cs ^ 1][m * 2 + i] = v.x[cs][src * 2 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) v.S[cs ^ 1][m * 3 + i] = v.S[cs][src * 3 + i];
    v.logZ[cs ^ 1][m] = v.logZ[cs][src];
    v.logw[cs ^ 1][m] = v.logw[cs][src];
}

}  // namespace smc
