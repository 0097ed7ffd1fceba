// smc_aux_kernels.h -- kernels of the handle core off the hot path: the break points of the resampling steps, and the
// commit of a window.  Included by smc_capi.hip only.
#pragma once
#include "smc_kernels.h"
#include "smc_resident.h"

namespace smc {

// ---------------------------------------------------------------------------------------------
// k_breaks: the break points of the resampling steps t0 .. t0+gridDim.x-1 of every filter (smc_spec.h
// "break points"): F[(tt * ntheta + th) * (nseg + 1) + w], 2^-64 fixed point, F[..][0] = 0.  They depend
// on (seed, stream, t, block sizes) only - never on the particles - so this runs ahead of the steps, off
// the critical path.  grid (steps, ntheta); one Gamma variate per block, an integer scan, one long division.
// ---------------------------------------------------------------------------------------------
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_breaks(FilterView v, uint32_t t0, uint64_t* F) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* g = (uint64_t*)smem;               // [nseg + 1]
    uint64_t* wt = g + v.nseg + 1;               // [THREADS / WAVE]
    constexpr int NW = THREADS / WAVE;
    const int tt = blockIdx.x, th = blockIdx.y, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const uint32_t t = t0 + (uint32_t)tt, stream = v.stream[th];
    const int B = v.nseg;
    for (int w = tid; w < B; w += THREADS) {
        int64_t m = v.n - (int64_t)w * v.seg;
        m = m > v.seg ? v.seg : m;
        g[w] = gamma_fix(v.seed, (uint32_t)w, stream, t, m);
    }
    if (tid == 0) g[B] = exp1_fix(v.seed, (uint32_t)B, stream, t);
    __syncthreads();
    const int E = (B + THREADS - 1) / THREADS;   // consecutive entries per thread
    uint64_t run = 0;
    for (int e = 0; e < E; ++e) {
        const int i = tid * E + e;
        if (i < B) { run += g[i]; g[i] = run; }
    }
    const uint64_t incl = wave_incl_scan(run, lane);
    if (lane == WAVE - 1) wt[wave] = incl;
    __syncthreads();
    uint64_t off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { off += w < wave ? wt[w] : 0; tot += wt[w]; }
    const uint64_t excl = off + incl - run, S = tot + g[B];
    uint64_t* out = F + ((size_t)tt * v.ntheta + th) * ((size_t)B + 1);
    if (tid == 0) out[0] = 0;
    for (int e = 0; e < E; ++e) {
        const int i = tid * E + e;
        if (i < B) out[i + 1] = div_frac64(g[i] + excl, S);
    }
}

// Keeps the first j steps of a window whose k_resident<WIN> launch ran exactly j steps: logZ += logmu_1 + .. + logmu_j in
// step order (the same additions smc_step makes), and the "last emitted" values become those of step j.  grid over theta.
__global__ void k_commit(FilterView v, int j, const StepRec* recs /*[ntheta][j]*/) {
    const int th = blockIdx.x * blockDim.x + threadIdx.x;
    if (th >= v.ntheta) return;
    double z = v.logZ[th], logmu = 0.0, ess = 0.0;
    StepRec o{};
    for (int t = 0; t < j; ++t) {
        o = recs[(size_t)th * j + t];
        combine_outputs(o.kb, o.S, seg_R(o.hi, o.lo, 0, 0), 0, v.n, logmu, ess);
        z = z + logmu;
    }
    v.logZ[th] = z;
    v.last_logmu[th] = logmu;
    v.last_ess[th] = ess;
    v.last_K[th] = o.kb;
    v.last_D[th] = o.S;
    host_emit(v, th, z, logmu, ess);
}

}  // namespace smc
