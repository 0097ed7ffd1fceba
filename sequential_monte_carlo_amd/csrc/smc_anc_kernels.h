// smc_anc_kernels.h -- ancestor sampling (smc_spec.h "ancestor sampling"): the sweep of a conditional handle over its
// record without the backward walk, wave64, f64, no MFMA.  Included by smc_capi_smooth.hip only, behind smc_path_kernels.h: the pair
// policy (path_source, path_pair), path_weight and the wave scan are backward simulation's, shared and not copied.
//
// k_cond_ancestors  ONE launch, grid (T, ntheta): workgroup (c, th) with c < T - 1 draws J_{c+1} of filter th - the sources are the
//                   cloud of step c, the target is xref[c + 1] - and workgroup (T - 1, th) makes the last pick, staged as the path
//                   kernels stage the last step (m = 0, s = 0, g = sp_log(w), target 0: the chain returns g).  Three passes over the
//                   n sources, the source side recomputed in each as k_path_select does, nothing of size n stored:
//                     1  the maximum M of b_l            (per thread, wave, workgroup: exact in any order)
//                     2  the INTEGER sum S of q_l        (exact in any order)
//                     3  tiles of blockDim.x consecutive sources in ascending order; the running sums are integer prefix sums over
//                        the wave and then over the waves, so the index is the one of a serial scan on any geometry
//                   The target, the uniform and the stream id are uniform over the workgroup.  A workgroup of one wave when the
//                   cloud is small (ANC_WAVE_N), of four otherwise: the same J.  No floating-point atomics, no spinning; thread 0
//                   stores the workgroup's one result.
// k_cond_trace      behind it on the handle's stream, one thread per filter: the T - 1 lookups of the trace from the last pick,
//                   idx, the dead flag, and the gather of the new reference - after every J was drawn from the old one.
#pragma once
#include "smc_path_kernels.h"

namespace smc {

constexpr int64_t ANC_WAVE_N = 256;   // at most this many particles: one wave per (step, filter)

struct AncArgs {
    int64_t n, T;          // particles per filter, recorded steps (= the length of the reference)
    int ntheta, d;
    uint64_t seed;         // the filter seed the steps ran with (cond_slot, anc_uniform)
    uint64_t path_seed;    // the seed of the last pick (path_uniform, path 0)
    const double* hx;      // [T][d][ntheta][n] the record: states ...
    const double* hw;      // [T][ntheta][n]    ... dense weights ...
    const int32_t* ha;     // [T][ntheta][n]    ... and ancestor vectors (row 0 is not read)
    double* xref;          // [T][d][ntheta] the reference: read by k_cond_ancestors, replaced by k_cond_trace
    const SmoothRow* rows; // [ntheta]
    const uint32_t* stream;// [ntheta] Philox stream ids
    int32_t* J;            // [T][ntheta] the ancestor draws; row 0 reads -1
    int32_t* last;         // [ntheta] the last pick, -1: no live particle at the last step
    int32_t* idx;          // [T][ntheta] the particles the new path passes through, -1 for a dead filter
    int* dead;             // [ntheta]
};

template <int MODEL>
__global__ __launch_bounds__(256) void k_cond_ancestors(AncArgs a) {
    constexpr int D = model_dim<MODEL>::value;
    constexpr int NV = path_nv<MODEL>::value;
    __shared__ double s_max[4];
    __shared__ unsigned long long s_sum[4];
    __shared__ long long s_pick;
    const int th = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const bool last = (int64_t)blockIdx.x == a.T - 1;
    const size_t ts = blockIdx.x;                            // the step of the sources
    const uint32_t t = last ? blockIdx.x : blockIdx.x + 1u;  // the step of the draw
    const size_t nt = (size_t)a.ntheta, plane = nt * (size_t)a.n, row = (size_t)th * (size_t)a.n;
    PathArgs p{};   // what path_source reads
    p.n = a.n; p.last = last;
    p.x_t = a.hx + ts * plane * (size_t)D; p.w_t = a.hw + ts * plane;
    const SmoothRow k = a.rows[th];
    double xo[D];
    for (int r = 0; r < D; ++r) xo[r] = last ? 0.0 : a.xref[((size_t)t * D + r) * nt + th];
    // pass 1: the maximum
    double M = -inf();
    for (int64_t l = threadIdx.x; l < a.n; l += blockDim.x) {
        double v[NV];
        if (path_source<MODEL>(p, k, row, plane, l, v)) {
            const double b = path_pair<MODEL>(k, v, xo);
            M = b > M ? b : M;
        }
    }
#pragma unroll
    for (int s = 32; s; s >>= 1) {
        const double om = __shfl_xor(M, s, 64);
        M = om > M ? om : M;
    }
    if (lane == 0) s_max[wave] = M;
    __syncthreads();
    M = s_max[0];
    for (int w = 1; w < nwave; ++w) M = s_max[w] > M ? s_max[w] : M;
    // pass 2: the integer sum
    uint64_t S = 0;
    for (int64_t l = threadIdx.x; l < a.n; l += blockDim.x) {
        double v[NV];
        if (path_source<MODEL>(p, k, row, plane, l, v)) S += path_weight(path_pair<MODEL>(k, v, xo), M);
    }
#pragma unroll
    for (int s = 32; s; s >>= 1) S += __shfl_xor((unsigned long long)S, s, 64);
    if (lane == 0) s_sum[wave] = S;
    __syncthreads();
    S = 0;
    for (int w = 0; w < nwave; ++w) S += s_sum[w];
    // pass 3: the smallest i with C_i > r
    const uint32_t st = a.stream[th];
    int64_t pick = -1;
    if (S) {   // (uniform over the workgroup, as every branch around a barrier or a cross-lane operation below)
        const uint64_t u = last ? path_uniform(a.path_seed, 0, st, t) : anc_uniform(a.seed, st, t);
        const uint64_t r = mulhi64(u, S);   // r < S: some tile holds it
        uint64_t C = 0;                     // the sum of every tile before this one
        for (int64_t l0 = 0; l0 < a.n && pick < 0; l0 += blockDim.x) {
            const int64_t l = l0 + threadIdx.x;
            double v[NV];
            uint64_t q = 0;
            if (path_source<MODEL>(p, k, row, plane, l, v)) q = path_weight(path_pair<MODEL>(k, v, xo), M);
            const uint64_t inc = wave_scan_u64(q, lane);
            __syncthreads();   // (everybody has read s_sum and s_pick of the round before)
            if (lane == 63) s_sum[wave] = inc;
            if (threadIdx.x == 0) s_pick = -1;
            __syncthreads();
            uint64_t before = C, tile = 0;
            for (int w = 0; w < nwave; ++w) {
                before += w < wave ? s_sum[w] : 0;
                tile += s_sum[w];
            }
            const uint64_t Ci = before + inc;
            if (Ci > r && Ci - q <= r) s_pick = l;   // the one source at which the running sum passes r
            __syncthreads();
            pick = s_pick;
            C += tile;
        }
    }
    if (threadIdx.x == 0) {
        if (last) a.last[th] = (int32_t)pick;
        else a.J[(size_t)t * nt + th] = pick >= 0 ? (int32_t)pick : (int32_t)cond_slot(a.seed, st, t - 1u, (uint32_t)a.n);
    }
}

// grid ceil(ntheta / 64), one thread per filter
__global__ __launch_bounds__(64) void k_cond_trace(AncArgs a) {
    const int th = (int)(blockIdx.x * 64u + threadIdx.x);
    if (th >= a.ntheta) return;
    const size_t nt = (size_t)a.ntheta, n = (size_t)a.n, T = (size_t)a.T, d = (size_t)a.d;
    const uint32_t st = a.stream[th];
    a.J[th] = -1;   // J_0
    int32_t i = a.last[th];
    bool ok = i >= 0;
    if (ok) a.idx[(T - 1) * nt + th] = i;
    for (size_t t = T - 1; ok && t >= 1; --t) {
        i = anc_trace(i, cond_slot(a.seed, st, (uint32_t)t, (uint32_t)a.n), a.J[t * nt + th], a.ha + (t * nt + th) * n);
        ok = i >= 0 && (size_t)i < n;   // (never false: the steps record particles, smc_history_put_ancestors checks its rows)
        if (ok) a.idx[(t - 1) * nt + th] = i;
    }
    a.dead[th] = ok ? 0 : 1;
    if (!ok) {   // the filter keeps its reference
        for (size_t t = 0; t < T; ++t) a.idx[t * nt + th] = -1;
        return;
    }
    for (size_t t = 0; t < T; ++t) {
        const size_t it = (size_t)a.idx[t * nt + th];
        for (size_t c = 0; c < d; ++c) a.xref[(t * d + c) * nt + th] = a.hx[((t * d + c) * nt + th) * n + it];
    }
}

}  // namespace smc
