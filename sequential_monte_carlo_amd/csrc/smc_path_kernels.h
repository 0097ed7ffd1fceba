// smc_path_kernels.h -- backward simulation (smc_spec.h "backward simulation"): whole trajectories drawn from
// p(x_1:T | y_1:T) by walking back through the recorded clouds, wave64, f64, no MFMA.  Included by smc_capi_smooth.hip only.
//
// The smoother's shape with PATHS as owners: one thread owns one path of one filter, a workgroup owns blockDim.x consecutive
// paths and ONE chunk of SMOOTH_CH source particles, staged in LDS as (m[D], s, g) exactly as the smoother's passes 0 and 1 stage
// them; every lane reads the same LDS address in the inner loop (a broadcast).  grid = (path tiles, ntheta, chunks).  Per
// backward step t, with the owner's state x_{t+1}^{idx[t+1][p]} kept in cur [d][ntheta][M]:
//   PASS 0  chunk maximum of b_l (no exp)                                                              -> pmax [chunk][th][p]
//   k_smooth_rowmax (more than SMOOTH_MAX_DIRECT chunks): M_p once per path                            -> rmax [th][p]
//   PASS 1  M_p from the chunk maxima (or rmax), chunk INTEGER sum of q_l = path_weight(b_l, M_p)      -> psum [chunk][th][p]
//   k_path_select  per path: S = the chunk sums in order, r = mulhi64(u, S), the chunk that holds r, that one chunk's q_l again
//           in ascending order until C > r; writes idx[t][p], the new cur and xs[t].  One thread per path, or one wave per path
//           (k_path_select_wave) when the launch has few paths: integer sums, the same index either way
// The last recorded step is the same machinery: its sources are staged as (m = 0, s = 0, g = sp_log(w)) and the owners read the
// state 0, so that the chain over the pair returns g itself (0 * 0 + g, exact).  No floating-point atomics, no spinning: the
// kernels follow each other on the handle's stream.  Tiles beyond a filter's path count, and those of a collapsed filter, leave.
#pragma once
#include "smc_smooth_kernels.h"

namespace smc {

struct PathArgs {
    int64_t n, M;          // particles per filter, path slots per filter
    int ntheta, nchunk;
    int last;              // the last recorded step: b_l = sp_log(w_l)
    uint32_t t;            // the step (the Philox counter of its draws)
    uint64_t seed;         // path seed
    const double* x_t;     // [d][ntheta][n] the sources: recorded states of step t
    const double* w_t;     // [ntheta][n] their dense weights
    double* cur;           // [d][ntheta][M] the state of every path at step t + 1 (k_path_select replaces it by that of step t)
    double* pmax;          // [nchunk][ntheta][M]
    const double* rmax;    // [nmax][ntheta][M]: pmax with nmax = nchunk, or the row maxima with nmax = 1
    int nmax;
    uint64_t* psum;        // [nchunk][ntheta][M]
    const SmoothRow* rows; // [ntheta]
    const int* dead;       // [ntheta] collapsed filters (k_smooth_dead)
    const int32_t* counts; // [ntheta] paths drawn per filter (<= M)
    const uint32_t* stream;// [ntheta] Philox stream ids
    const int32_t* idx_n;  // [ntheta][M] idx[t + 1] (unused at the last step)
    int32_t* idx_t;        // [ntheta][M] idx[t]
    double* xs_t;          // [d][ntheta][M] the paths' states at step t, or nullptr (MODEL_UCSV_RB: [2][ntheta][M], the chosen lse, lsn)
    double y;              // MODEL_UCSV_RB: the observation of step t
};

// The pair policy of a family.  The three families with a transition density stage (m[D], s, g) and own the state x_{t+1}
// (logf_source / logf_pair); MODEL_UCSV_RB (smc_spec.h "Rao-Blackwellised backward simulation") stages
// (m, V, lse, lsn, g) and owns (a+, b+, mu, tau): the same passes and the same selection over another chain.
template <int MODEL> struct path_nv { static constexpr int value = MODEL == MODEL_UCSV_RB ? RB_NV : model_dim<MODEL>::value + 2; };

// (m[D], s, g) of source l as the pair chain wants them; false: not live
template <int MODEL>
__device__ __forceinline__ bool path_source(const PathArgs& a, const SmoothRow& k, size_t row, size_t plane, int64_t l, double* v) {
    constexpr int D = model_dim<MODEL>::value;
    const double wl = l < a.n ? a.w_t[row + l] : 0.0;
    if (!(wl > 0.0)) return false;
    if constexpr (MODEL == MODEL_UCSV_RB) {
        double xs[D];
        for (int r = 0; r < D; ++r) xs[r] = a.last ? 0.0 : a.x_t[(size_t)r * plane + row + l];
        rb_source(a.last, xs, wl, v);
    } else if (a.last) {
        for (int r = 0; r < D + 1; ++r) v[r] = 0.0;
        v[D + 1] = sp_log(wl);
    } else {
        double xs[D], c;
        for (int r = 0; r < D; ++r) xs[r] = a.x_t[(size_t)r * plane + row + l];
        logf_source<MODEL>(k, xs, v, v[D], c);
        v[D + 1] = sp_log(wl) + c;
    }
    return true;
}
// a source that is left out: never the maximum, q = 0
template <int MODEL>
__device__ __forceinline__ void path_no_source(double* v) {
    constexpr int NV = path_nv<MODEL>::value;
    for (int r = 0; r < NV - 1; ++r) v[r] = 0.0;
    v[NV - 1] = -inf();
}
// what the owner holds of step t + 1; at the last step the values with which the chain returns g
template <int MODEL>
__device__ __forceinline__ void path_owner(const PathArgs& a, size_t pplane, size_t prow, int64_t p, double* xo) {
    constexpr int D = model_dim<MODEL>::value;
    for (int r = 0; r < D; ++r) xo[r] = a.last ? (MODEL == MODEL_UCSV_RB && r == 3 ? 1.0 : 0.0) : a.cur[(size_t)r * pplane + prow + p];
}
template <int MODEL>
__device__ __forceinline__ double path_pair(const SmoothRow& k, const double* v, const double* xo) {
    constexpr int D = model_dim<MODEL>::value;
    if constexpr (MODEL == MODEL_UCSV_RB) return rb_pair(k, v, xo);
    else return logf_pair<MODEL>(k, v, v[D], v[D + 1], xo);
}
// MODEL_UCSV_RB, after the pick: the information update of the owner and the chosen volatilities (one thread per path)
__device__ __forceinline__ void rb_commit(const PathArgs& a, size_t row, size_t plane, size_t prow, size_t pplane, int64_t p, int64_t pick) {
    const double nan = bits2d(0x7ff8000000000000ULL);
    double lse = nan, lsn = nan, mu = nan, tau = nan;
    if (pick >= 0) {
        lse = a.x_t[plane + row + pick];
        lsn = a.x_t[2 * plane + row + pick];
        mu = a.last ? 0.0 : a.cur[2 * pplane + prow + p];
        tau = a.last ? 0.0 : a.cur[3 * pplane + prow + p];
        rb_info(a.last, lse, lsn, a.y, mu, tau);
    }
    a.cur[prow + p] = lse;
    a.cur[pplane + prow + p] = lsn;
    a.cur[2 * pplane + prow + p] = mu;
    a.cur[3 * pplane + prow + p] = tau;
    if (a.xs_t) {
        a.xs_t[prow + p] = lse;
        a.xs_t[pplane + prow + p] = lsn;
    }
}

template <int MODEL, int PASS>
__global__ void k_path_pairs(PathArgs a) {
    constexpr int D = model_dim<MODEL>::value;
    constexpr int NV = path_nv<MODEL>::value;
    __shared__ double sm[SMOOTH_CH][NV];
    const int th = blockIdx.y, ch = blockIdx.z;
    // (uniform over the workgroup: nobody waits at the barrier below)
    if (a.dead[th] || (int64_t)blockIdx.x * blockDim.x >= (int64_t)a.counts[th]) return;
    const size_t row = (size_t)th * a.n, plane = (size_t)a.ntheta * a.n;
    const size_t prow = (size_t)th * a.M, pplane = (size_t)a.ntheta * a.M;
    const SmoothRow k = a.rows[th];
    for (int q = threadIdx.x; q < SMOOTH_CH; q += blockDim.x) {
        double v[NV];
        if (!path_source<MODEL>(a, k, row, plane, (int64_t)ch * SMOOTH_CH + q, v)) path_no_source<MODEL>(v);
        for (int r = 0; r < NV; ++r) sm[q][r] = v[r];
    }
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.M) return;
    double xo[D];
    path_owner<MODEL>(a, pplane, prow, p, xo);
    const size_t o = ((size_t)ch * a.ntheta + th) * a.M + p;
    if constexpr (PASS == 0) {
        double M = -inf();
#pragma unroll 8
        for (int q = 0; q < SMOOTH_CH; ++q) {
            const double b = path_pair<MODEL>(k, sm[q], xo);
            M = b > M ? b : M;
        }
        a.pmax[o] = M;
    } else {
        double M = -inf();
        for (int c = 0; c < a.nmax; ++c) {
            const double pm = a.rmax[((size_t)c * a.ntheta + th) * a.M + p];
            M = pm > M ? pm : M;
        }
        uint64_t S = 0;
#pragma unroll 4
        for (int q = 0; q < SMOOTH_CH; ++q) {
            const double b = path_pair<MODEL>(k, sm[q], xo);
            S += path_weight(b, M);
        }
        a.psum[o] = S;
    }
}

// The selection has two shapes with the same result.  ONE THREAD per path: S and r, the chunk that holds r, then that chunk's
// sources one after the other (per-lane gathers, the source side recomputed per lane) - the fewest instructions per path, but a
// serial chain of up to SMOOTH_CH dependent evaluations: 25 us per step when there are too few paths to hide it.
template <int MODEL>
__global__ void k_path_select(PathArgs a) {
    constexpr int D = model_dim<MODEL>::value;
    const int th = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.M) return;
    const size_t row = (size_t)th * a.n, plane = (size_t)a.ntheta * a.n;
    const size_t prow = (size_t)th * a.M, pplane = (size_t)a.ntheta * a.M;
    const SmoothRow k = a.rows[th];
    int64_t pick = -1;
    const bool alive = !a.dead[th] && p < (int64_t)a.counts[th] && (a.last || a.idx_n[prow + p] >= 0);
    if (alive) {
        double M = -inf();
        for (int c = 0; c < a.nmax; ++c) {
            const double pm = a.rmax[((size_t)c * a.ntheta + th) * a.M + p];
            M = pm > M ? pm : M;
        }
        uint64_t S = 0;
        for (int c = 0; c < a.nchunk; ++c) S += a.psum[((size_t)c * a.ntheta + th) * a.M + p];
        if (S) {
            const uint64_t r = mulhi64(path_uniform(a.seed, p, a.stream[th], a.t), S);   // r < S
            uint64_t C = 0;
            int ch = 0;
            for (; ch < a.nchunk - 1; ++ch) {
                const uint64_t s = a.psum[((size_t)ch * a.ntheta + th) * a.M + p];
                if (C + s > r) break;
                C += s;
            }
            double xo[D];
            path_owner<MODEL>(a, pplane, prow, p, xo);
            const int64_t l0 = (int64_t)ch * SMOOTH_CH, l1 = l0 + SMOOTH_CH < a.n ? l0 + SMOOTH_CH : a.n;
            for (int64_t l = l0; l < l1; ++l) {
                double v[path_nv<MODEL>::value];
                if (!path_source<MODEL>(a, k, row, plane, l, v)) continue;
                C += path_weight(path_pair<MODEL>(k, v, xo), M);
                if (C > r) { pick = l; break; }
            }
        }
    }
    a.idx_t[prow + p] = (int32_t)pick;
    if constexpr (MODEL == MODEL_UCSV_RB) {
        rb_commit(a, row, plane, prow, pplane, p, pick);
    } else {
        for (int r = 0; r < D; ++r) {
            const double xv = pick >= 0 ? a.x_t[(size_t)r * plane + row + pick] : bits2d(0x7ff8000000000000ULL);
            a.cur[(size_t)r * pplane + prow + p] = xv;
            if (a.xs_t) a.xs_t[(size_t)r * pplane + prow + p] = xv;
        }
    }
}

// ONE WAVE per path, for launches of few paths (PATH_WAVE_SELECT): about three times the instructions per path (the draw and
// the prefix sums are paid per wave), a fifth of the latency.  Measured (profiles/paths_cost.log, n_theta x 1024 particles, M = 1024):
// the wave shape is ahead up to 65536 paths, level at 131072, 6 - 11 % behind at 262144, 11 - 21 % at 524288.
#ifndef SMC_PATH_WAVE_SELECT
#define SMC_PATH_WAVE_SELECT 262144
#endif
// n_theta M below this: one wave per path (DESIGN.md 2f "Cost").  The same indices either way; the timing builds of
// scripts/dbg/paths_cost.py (`make pathsel SEL=...`) force one shape at every size with 0 and 1 << 62
constexpr int64_t PATH_WAVE_SELECT = SMC_PATH_WAVE_SELECT;

// inclusive prefix sum over the 64 lanes of a wave (integers: exact)
__device__ __forceinline__ uint64_t wave_scan_u64(uint64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up((unsigned long long)v, d, 64);
        v += lane >= d ? o : 0;
    }
    return v;
}

// blockDim.x / 64 paths per workgroup.  The lanes share the chunk sums and then the sources of the chunk that holds r, 64 at a
// time in ascending order; the running sums are integer prefix sums over the wave, so the index is the one
// of a serial scan.  Every branch around a cross-lane operation is uniform over the wave.
template <int MODEL>
__global__ void k_path_select_wave(PathArgs a) {
    constexpr int D = model_dim<MODEL>::value;
    const int th = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= a.M) return;
    const size_t row = (size_t)th * a.n, plane = (size_t)a.ntheta * a.n;
    const size_t prow = (size_t)th * a.M, pplane = (size_t)a.ntheta * a.M;
    const SmoothRow k = a.rows[th];
    int64_t pick = -1;
    const bool alive = !a.dead[th] && p < (int64_t)a.counts[th] && (a.last || a.idx_n[prow + p] >= 0);
    if (alive) {
        double M = -inf();
        for (int c = lane; c < a.nmax; c += 64) {
            const double pm = a.rmax[((size_t)c * a.ntheta + th) * a.M + p];
            M = pm > M ? pm : M;
        }
        uint64_t S = 0;
        for (int c = lane; c < a.nchunk; c += 64) S += a.psum[((size_t)c * a.ntheta + th) * a.M + p];
#pragma unroll
        for (int d = 32; d; d >>= 1) {
            const double om = __shfl_xor(M, d, 64);
            M = om > M ? om : M;
            S += __shfl_xor((unsigned long long)S, d, 64);
        }
        if (S) {
            const uint64_t r = mulhi64(path_uniform(a.seed, p, a.stream[th], a.t), S);   // r < S: some chunk holds it
            uint64_t C = 0;   // the sum of everything before what the wave looks at
            int ch = -1;
            for (int c0 = 0; c0 < a.nchunk && ch < 0; c0 += 64) {
                const int c = c0 + lane;
                const uint64_t s = c < a.nchunk ? a.psum[((size_t)c * a.ntheta + th) * a.M + p] : 0;
                const uint64_t inc = wave_scan_u64(s, lane);
                const unsigned long long hit = __ballot(C + inc > r);
                if (hit) {
                    const int f = __ffsll((long long)hit) - 1;
                    ch = c0 + f;
                    C += __shfl((unsigned long long)(inc - s), f, 64);
                } else {
                    C += __shfl((unsigned long long)inc, 63, 64);
                }
            }
            double xo[D];
            path_owner<MODEL>(a, pplane, prow, p, xo);
            for (int b = 0; b < SMOOTH_CH / 64 && ch >= 0 && pick < 0; ++b) {
                const int64_t l0 = (int64_t)ch * SMOOTH_CH + b * 64;
                double v[path_nv<MODEL>::value];
                uint64_t q = 0;
                if (path_source<MODEL>(a, k, row, plane, l0 + lane, v)) q = path_weight(path_pair<MODEL>(k, v, xo), M);
                const uint64_t inc = wave_scan_u64(q, lane);
                const unsigned long long hit = __ballot(C + inc > r);
                if (hit) pick = l0 + (__ffsll((long long)hit) - 1);
                else C += __shfl((unsigned long long)inc, 63, 64);
            }
        }
    }
    if (lane == 0) a.idx_t[prow + p] = (int32_t)pick;
    if constexpr (MODEL == MODEL_UCSV_RB) {
        if (lane == 0) rb_commit(a, row, plane, prow, pplane, p, pick);
    } else if (lane < D) {
        const double xv = pick >= 0 ? a.x_t[(size_t)lane * plane + row + pick] : bits2d(0x7ff8000000000000ULL);
        a.cur[(size_t)lane * pplane + prow + p] = xv;
        if (a.xs_t) a.xs_t[(size_t)lane * pplane + prow + p] = xv;
    }
}

}  // namespace smc
