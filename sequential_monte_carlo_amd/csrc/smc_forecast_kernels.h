// smc_forecast_kernels.h -- forecasts: the filtered cloud propagated past the last observation (smc_spec.h "forecasts";
// smc_forecast / smc_forecast_cloud, smc_capi_forecast.hip).  Instantiated per model family by smc_model.hip.
//
//   k_forecast   grid (nseg, ntheta), the geometry of k_init: one lane owns particle PAIRS (the Box-Muller pairs of the
//                specification).  It loads the pair's state rows once, keeps them in registers and walks a BLOCK of horizons
//                k0 .. k0 + nk - 1: per horizon model_forecast_step for both particles, then d + 3 sixteen-byte streaming stores
//                (the d state rows, then yf, ym, yv) into out, laid out [horizon][d + 3][ntheta][npad] - consecutive lanes write
//                consecutive 16 bytes of every row.  Padding slots beyond n are written as 0.0, as k_init writes them.
// No resampling, no normalisation, no LDS, no barrier: the kernel reads src (the handle's x[cur], or the state rows of the last
// horizon of the previous block - same row pitch) and writes out alone; a lane reads and writes only its own pairs, so a block
// may restart from rows of the buffer it overwrites.  Store bound: (d + 3) * 8 bytes per particle and horizon against one step's
// worth of Philox / Box-Muller issue (nz + 1 pairs of normals per pair of particles).
#pragma once
#include "smc_kernels.h"

namespace smc {

template <int MODEL, int THREADS, int NP>
__global__ __launch_bounds__(THREADS) void k_forecast(FilterView v, const double* src, uint64_t fseed, uint32_t k0, int nk,
                                                      double* out) {
    constexpr int D = model_dim<MODEL>::value, NZ = model_nz<MODEL>::value, ROWS = D + 3;
    const int sb = logical_segment(blockIdx.x, v.nseg), th = blockIdx.y, tid = (int)threadIdx.x;
    const Params prm = v.params[th];
    const uint32_t stream = v.stream[th];
    const int64_t seg0 = (int64_t)sb * v.seg;
    const size_t plane = (size_t)v.ntheta * (size_t)v.npad;   // one row of every filter
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int pl = tid + k * THREADS;            // pair within segment
        const int64_t i0 = seg0 + 2 * pl;            // first particle of the pair (i0 + 1 < npad: segments are even)
        const uint32_t pg = (uint32_t)(i0 >> 1);     // pair index within the filter
        const size_t at = (size_t)th * (size_t)v.npad + (size_t)i0;
        const bool ok0 = i0 < v.n, ok1 = i0 + 1 < v.n;
        double xs[2][D];
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const double2 in = *reinterpret_cast<const double2*>(src + (size_t)c * plane + at);
            xs[0][c] = in.x;
            xs[1][c] = in.y;
        }
        double* o = out + at;
        for (int j = 0; j < nk; ++j, o += (size_t)ROWS * plane) {
            const uint32_t hz = k0 + (uint32_t)j;    // the horizon, 1-based: the Philox step index
            double z[NZ][2], e[2], xn[2][D], yf[2], ym[2], yv[2];
#pragma unroll
            for (int c = 0; c < NZ; ++c) box_muller(draw(fseed, pg, stream, hz, SLOT_NORMAL0 + c), z[c][0], z[c][1]);
            box_muller(draw(fseed, pg, stream, hz, SLOT_OBS), e[0], e[1]);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                double zz[NZ];
#pragma unroll
                for (int c = 0; c < NZ; ++c) zz[c] = z[c][q];
                model_forecast_step<MODEL>(prm, xs[q], zz, e[q], xn[q], yf[q], ym[q], yv[q]);
#pragma unroll
                for (int c = 0; c < D; ++c) xs[q][c] = xn[q][c];
            }
#pragma unroll
            for (int c = 0; c < D; ++c) {
                double2 w;
                w.x = ok0 ? xs[0][c] : 0.0;
                w.y = ok1 ? xs[1][c] : 0.0;
                store_out(reinterpret_cast<double2*>(o + (size_t)c * plane), w);
            }
            double2 w;
            w.x = ok0 ? yf[0] : 0.0; w.y = ok1 ? yf[1] : 0.0;
            store_out(reinterpret_cast<double2*>(o + (size_t)D * plane), w);
            w.x = ok0 ? ym[0] : 0.0; w.y = ok1 ? ym[1] : 0.0;
            store_out(reinterpret_cast<double2*>(o + (size_t)(D + 1) * plane), w);
            w.x = ok0 ? yv[0] : 0.0; w.y = ok1 ? yv[1] : 0.0;
            store_out(reinterpret_cast<double2*>(o + (size_t)(D + 2) * plane), w);
        }
    }
}

}  // namespace smc
