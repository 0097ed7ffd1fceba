// smc_ibis_smooth_kernels.h -- the RTS smoother of an IBIS cloud and its backward-sampled paths (smc_spec.h "the RTS smoother of
// an IBIS cloud").  One lane per parameter particle (per path in k_ibis_rts_paths), one wave per workgroup, f64.
// Included by smc_ibis.hip only.
//
//   k_ibis_rts_forward   the Kalman filter over y[0:T) from (x0, sigma0) in registers; the filtered record xf, Sf [T][M]
//   k_ibis_rts_backward  t = T-1 .. 0 over the record: (xs_t, Ps_t) in registers, the chunk record of the summaries into row t of
//                        part (SUMM), and (xs_t, Ps_t) written over (xf_t, Sf_t) (STORE) - a lane reads its own entry of the
//                        record before it overwrites it, and no other lane touches that entry
//   k_ibis_rts_paths     one lane per path: the filter of its own particle which[p] into a record [T][Mp], then the walk back
//                        with one normal per step
//
// The rows, log-weights and y are read and never written; every store is a plain vector store; no atomics.  Entry t of lane m
// sits at t M + m: consecutive lanes, consecutive addresses.  The loops stream 32 T M bytes over the two passes (16 T M
// written, 16 T M read; STORE adds 16 T M written); the record loads of step t-1 are issued before the dependent chain of step
// t, in source order, so nothing depends on the compiler moving a load over a store it cannot tell apart.
#pragma once
#include "smc_ibis_kernels.h"

namespace smc {

// MISS (both filters of this file; launched only for a flagged call whose series holds a NaN): the missing Kalman step of
// smc_spec.h at a NaN y[t] - the record at a gap is the predictive pair, and the backward passes run over it as they are
template <bool MISS = false>
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_rts_forward(const double* raw /*[M][IBIS_NRAW]*/, int64_t M, const double* y,
                                                                  int64_t T, int predict_first, double* xf, double* Sf) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    if (m >= M) return;
    const double* row = raw + m * IBIS_NRAW;
    const double A = row[0], B = row[1], Q = row[2], R = row[3];
    double x = row[4], S = row[5];
    for (int64_t t = 0; t < T; ++t) {
        (void)kalman_step_gaps<MISS>(A, B, Q, R, t > 0 || predict_first != 0, y[t], x, S);
        xf[(size_t)t * (size_t)M + (size_t)m] = x;
        Sf[(size_t)t * (size_t)M + (size_t)m] = S;
    }
}

// logw: [M], or null with SUMM false.  part: [T][IBIS_SUM_NCOL][nchunk], nchunk = gridDim.x
template <bool SUMM, bool STORE>
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_rts_backward(const double* raw, const double* logw, int64_t M, int64_t T,
                                                                   double* xf, double* Sf, double* part) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    const bool valid = m < M;
    const int64_t mm = valid ? m : M - 1;              // lanes beyond the cloud compute on the last particle and store nothing
    const double* row = raw + mm * IBIS_NRAW;
    const double A = row[0], B = row[1], Q = row[2], R = row[3];
    const double lw = SUMM ? logw[mm] : 0.0;
    const size_t sM = (size_t)M, smm = (size_t)mm;
    double xn = xf[(size_t)(T - 1) * sM + smm], Sn = Sf[(size_t)(T - 1) * sM + smm];
    double xs = 0.0, Ps = 0.0;
    for (int64_t t = T - 1; t >= 0; --t) {
        const double xft = xn, Sft = Sn;
        if (t > 0) {                                   // the loads of step t-1, ahead of the chain and of the stores of step t
            xn = xf[(size_t)(t - 1) * sM + smm];
            Sn = Sf[(size_t)(t - 1) * sM + smm];
        }
        if (t == T - 1) { xs = xft; Ps = Sft; }
        else rts_back(A, Q, xft, Sft, xs, Ps);
        if (SUMM)
            ibis_chunk_record(A, B, Q, R, xs, Ps, lw, valid, 0, part + (size_t)t * IBIS_SUM_NCOL * (size_t)gridDim.x, gridDim.x, blockIdx.x);
        if (STORE && valid) {
            xf[(size_t)t * sM + smm] = xs;
            Sf[(size_t)t * sM + smm] = Ps;
        }
    }
}

// paths [T][Mp]: holds xf of the path's particle on the way forward, the path on the way back; Sf [T][Mp] scratch
template <bool MISS = false>
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_rts_paths(const double* raw, const int32_t* which, int64_t Mp, const double* y,
                                                                int64_t T, int predict_first, uint64_t path_seed, double* paths,
                                                                double* Sf) {
    const int64_t p = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    if (p >= Mp) return;
    const int64_t m = which[p];
    const uint32_t stream = (uint32_t)m;
    const double* row = raw + m * IBIS_NRAW;
    const double A = row[0], B = row[1], Q = row[2], R = row[3];
    const size_t sM = (size_t)Mp, sp = (size_t)p;
    double x = row[4], S = row[5];
    for (int64_t t = 0; t < T; ++t) {
        (void)kalman_step_gaps<MISS>(A, B, Q, R, t > 0 || predict_first != 0, y[t], x, S);
        if (t < T - 1) {                               // (the last entry stays in registers)
            paths[(size_t)t * sM + sp] = x;
            Sf[(size_t)t * sM + sp] = S;
        }
    }
    double xp = rts_path_last(x, S, rts_normal(path_seed, p, stream, (uint32_t)(T - 1)));
    paths[(size_t)(T - 1) * sM + sp] = xp;
    if (T < 2) return;
    double xn = paths[(size_t)(T - 2) * sM + sp], Sn = Sf[(size_t)(T - 2) * sM + sp];
    for (int64_t t = T - 2; t >= 0; --t) {
        const double xft = xn, Sft = Sn;
        if (t > 0) {
            xn = paths[(size_t)(t - 1) * sM + sp];
            Sn = Sf[(size_t)(t - 1) * sM + sp];
        }
        xp = rts_path_back(A, Q, xft, Sft, xp, rts_normal(path_seed, p, stream, (uint32_t)t));
        paths[(size_t)t * sM + sp] = xp;
    }
}

}  // namespace smc
