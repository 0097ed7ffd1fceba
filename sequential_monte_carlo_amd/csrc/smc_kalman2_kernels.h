// smc_kalman2_kernels.h -- the exact Kalman filter and RTS smoother of two-state linear models with a scalar observation
// (smc_spec.h "the exact Kalman filter of a TWO-STATE linear model"; src/kalman_filter.jl:3-27, 55-70), batched over parameter
// rows.  Included by smc_kalman2.hip only.
//
//   k_kalman_loglik<Lg2Row> (smc_kalman_rows.h)   the whole series per row: (x_T [2], Sigma_T [3], logZ)
//   k_kalman2_smooth   the filter writes its record, then the backward walk over it: xs [T][n][2], Ps [T][n][3]
// (The IBIS sampler over such rows is smc_ibis_kernels.h with Row = Lg2Row.)
//
// One lane per row, one wave per workgroup, f64.  The row (15 doubles) and the state (5) live in registers; y[t] is the same
// address in every lane (the compiler reads it through the scalar cache).  No LDS, no float atomics; every store is a plain
// vector store of the lane's own entries.
#pragma once
#include "smc_kalman_rows.h"
#include "smc_kernels.h"

namespace smc {

// xs, Ps hold the filtered record after the forward loop; the backward walk overwrites entry t with the smoothed one after it
// has read it.  A lane reads back only what it stored itself.
__global__ __launch_bounds__(KALMAN_THREADS) void k_kalman2_smooth(const double* raw /*[n][LG2_NRAW]*/, int64_t n, const double* y, int64_t T,
                                                                    int predict_first, double* xs /*[T][n][2]*/, double* Ps /*[T][n][3]*/) {
    const int64_t m = (int64_t)blockIdx.x * KALMAN_THREADS + threadIdx.x;
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

}  // namespace smc
