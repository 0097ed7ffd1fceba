// smc_kalman_rows.h -- the two kinds of parameter row the exact-Kalman side filters, as one trait: what a kernel has to know about
// a row to hold it in registers and to advance its state.  Depends on smc_spec.h only; nothing of the specification is restated
// here - step() forwards to kalman_step_gaps / kalman2_step, the same operations in the same order.
//
//   NRAW    doubles per row                                 Lg1Row: (A, B, Q, R, x0, sigma0)        Lg2Row: the LG2_* entries
//   NX, NS  doubles of the state and of its stored covariance (the lower triangle for two states)
//   NSTEP   leading row entries a step reads
//   X0, S0  where the initial state and covariance sit in the row: NX entries from X0, NS entries from S0
//   SKIP_IDLE_WAVE  whether the rejuvenation tests, per chain position, that some lane of the wave proposed inside the support
//           before it re-filters (the same results either way; a matter of speed, decided by measurement per kind of row)
//
// Loops over these lengths are unrolled and every index is a constant, so x [NX], S [NS] and the row stay in registers.
#pragma once
#include "smc_spec.h"

namespace smc {

struct Lg1Row {   // MODEL_LG1D: the univariate LinearModel
    static constexpr int NRAW = 6, NX = 1, NS = 1, NSTEP = 4, X0 = 4, S0 = 5;
    static constexpr bool SKIP_IDLE_WAVE = false;   // measured: with the test the scalar rejuvenation is 3 % slower at M <= 2^16
    // MISS: a NaN y is the missing Kalman step (smc_spec.h); MISS = false is kalman_step
    template <bool MISS>
    static SMC_HD double step(const double* r /*[NSTEP]*/, bool predict, double y, double* x, double* S) {
        return kalman_step_gaps<MISS>(r[0], r[1], r[2], r[3], predict, y, x[0], S[0]);
    }
};

struct Lg2Row {   // MODEL_LG2D: two states, a scalar observation
    static constexpr int NRAW = LG2_NRAW, NX = 2, NS = 3, NSTEP = LG2_R + 1, X0 = LG2_X1, S0 = LG2_S11;
    static constexpr bool SKIP_IDLE_WAVE = true;
    template <bool MISS>
    static SMC_HD double step(const double* r /*[NSTEP]*/, bool predict, double y, double* x, double* S) {
        static_assert(!MISS, "two-state rows have no missing Kalman step");
        return kalman2_step(r, predict, y, x[0], x[1], S[0], S[1], S[2]);
    }
};
static_assert(LG2_X2 == LG2_X1 + 1 && LG2_S21 == LG2_S11 + 1 && LG2_S22 == LG2_S11 + 2, "the initial state of a row is contiguous");

// The exact Kalman filter over a whole series, batched over rows, one lane per row (kalman_filter.jl:29-70 / :3-27):
// out [n][NX + NS + 1] = the state, then its covariance, then logZ - the step values summed in step order from 0.0.
// MISS (SMC_FLAG_NAN_MISSING and a NaN in y; scalar rows only): a NaN y[t] is the missing Kalman step.
// Instantiated where it is launched: Lg1Row in smc_util.hip (smc_kalman_log_likelihood), Lg2Row in smc_kalman2.hip.
constexpr int KALMAN_THREADS = 64;
template <class Row, bool MISS = false>
__global__ __launch_bounds__(KALMAN_THREADS) void k_kalman_loglik(const double* raw /*[n][NRAW]*/, int64_t n, const double* y, int64_t T,
                                                                 int predict_first, double* out) {
    const int64_t m = (int64_t)blockIdx.x * KALMAN_THREADS + threadIdx.x;
    if (m >= n) return;
    double r[Row::NRAW], x[Row::NX], S[Row::NS], logZ = 0.0;
#pragma unroll
    for (int k = 0; k < Row::NRAW; ++k) r[k] = raw[m * Row::NRAW + k];
#pragma unroll
    for (int i = 0; i < Row::NX; ++i) x[i] = r[Row::X0 + i];
#pragma unroll
    for (int i = 0; i < Row::NS; ++i) S[i] = r[Row::S0 + i];
    for (int64_t t = 0; t < T; ++t) logZ += Row::template step<MISS>(r, predict_first != 0 || t > 0, y[t], x, S);
    double* o = out + m * (Row::NX + Row::NS + 1);
#pragma unroll
    for (int i = 0; i < Row::NX; ++i) o[i] = x[i];
#pragma unroll
    for (int i = 0; i < Row::NS; ++i) o[Row::NX + i] = S[i];
    o[Row::NX + Row::NS] = logZ;
}

}  // namespace smc
