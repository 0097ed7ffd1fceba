// smc_smooth_kernels.h -- the backward pass of the FFBS smoother (smc_spec.h "the smoother"): all-pairs transition
// densities between the recorded clouds of two consecutive steps, wave64, f64, no MFMA.  Included by smc_capi_smooth.hip only.
//
// One thread owns one particle of the OWNER side; a workgroup owns blockDim.x consecutive owners of one filter and ONE chunk of
// SMOOTH_CH particles of the STAGED side, which it puts into LDS with everything that depends on the staged particle alone
// hoisted.  Every lane reads the same LDS address in the inner loop (a broadcast).  grid = (owner tiles, ntheta, chunks): a chunk
// is the unit of the summation order, so the bits depend neither on the tile length nor on the batch.
//   PASS 0  owners = targets j (step t+1), staged = sources l (step t):  chunk maximum of a_lj            -> pmax [chunk][th][j]
//   k_smooth_rowmax (filters of more than SMOOTH_MAX_DIRECT chunks): M_j = max over the chunk maxima, once per target      -> rmax [th][j]
//   PASS 1  the same roles: M_j (from rmax, or the maximum over the few chunk maxima), chunk partial of sum_l sp_exp(a_lj - M_j)
//                                                                                                            -> part [chunk][th][j]
//   k_smooth_logd: logD_j = M_j + sp_log(sum of the partials in ascending order)
//   PASS 2  owners = sources i (step t), staged = targets j (step t+1): chunk partial of sum_j ws_j sp_exp(logf_ij - logD_j)
//   k_smooth_finish: ws_t^i = w_t^i > 0 ? w_t^i * (sum of the partials in ascending order) : 0;  NaN for a collapsed filter
//   PASS 3  (smc_smooth_pairs only, in PASS 2's place) PASS 2 with 2 d accumulators more: the chunk partials of
//           p_ij, p_ij x_j^c and p_ij d_c^2                                                        -> part [1 + 2 d][chunk][th][i]
//   k_smooth_pair_moments: cross[t], resid2[t] from those partials, one workgroup per filter (plane 0 goes through k_smooth_finish)
// No floating-point atomics, no spinning: the partials go through scratch owned by the handle, the kernels follow each other on
// the handle's stream.
#pragma once
#include "smc_spec.h"
#include "smc_kernels.h"   // order_key, key_value, prob_to_u64, QMAX (k_smooth_quantiles)

namespace smc {

struct SmoothArgs {
    int64_t n;             // particles per filter
    int ntheta, nchunk;    // filters, chunks of SMOOTH_CH particles
    const double* x_own;   // [d][ntheta][n] states of the owner side
    const double* x_st;    // [d][ntheta][n] states of the staged side
    const double* w_st;    // [ntheta][n] PASS 0, 1: filter weights of the sources; PASS 2, 3: smoothed weights of the targets
    const double* logD;    // [ntheta][n] PASS 2, 3
    double* pmax;          // [nchunk][ntheta][n] chunk maxima (PASS 0 writes them)
    const double* rmax;    // [nmax][ntheta][n] what PASS 1 takes M_j from: pmax with nmax = nchunk, or the row maxima with nmax = 1
    int nmax;
    double* part;          // [nchunk][ntheta][n];  PASS 3: [1 + 2 d][nchunk][ntheta][n], plane 0 what PASS 2 writes, then the chunk
    const SmoothRow* rows; // [ntheta]                                                     partials of X^c and of R^c
};

template <int MODEL, int PASS>
__global__ void k_smooth_pairs(SmoothArgs a) {
    constexpr int D = model_dim<MODEL>::value;
    constexpr int NV = D + 2;
    __shared__ double sm[SMOOTH_CH][NV];   // PASS 0, 1: (m[D], s, g);  PASS 2, 3: (x[D], ws, logD)
    const int th = blockIdx.y, ch = blockIdx.z;
    const int64_t n = a.n;
    const size_t row = (size_t)th * n, plane = (size_t)a.ntheta * n;
    const SmoothRow k = a.rows[th];
    for (int q = threadIdx.x; q < SMOOTH_CH; q += blockDim.x) {
        const int64_t l = (int64_t)ch * SMOOTH_CH + q;
        double v[NV];
        const double wl = l < n ? a.w_st[row + l] : 0.0;
        if (wl > 0.0) {   // (false for a NaN weight as well)
            double xs[D];
            for (int r = 0; r < D; ++r) xs[r] = a.x_st[(size_t)r * plane + row + l];
            if constexpr (PASS < 2) {
                double c;
                logf_source<MODEL>(k, xs, v, v[D], c);
                v[D + 1] = sp_log(wl) + c;
            } else {
                for (int r = 0; r < D; ++r) v[r] = xs[r];
                v[D] = wl;
                v[D + 1] = a.logD[row + l];
            }
        } else {          // left out: every term it enters is exactly +0.0, and it never is the maximum
            for (int r = 0; r < D + 1; ++r) v[r] = 0.0;
            v[D + 1] = PASS < 2 ? -inf() : inf();
        }
        for (int r = 0; r < NV; ++r) sm[q][r] = v[r];
    }
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double xo[D];
    for (int r = 0; r < D; ++r) xo[r] = a.x_own[(size_t)r * plane + row + j];
    const size_t o = ((size_t)ch * a.ntheta + th) * n + j;
    if constexpr (PASS == 0) {
        double M = -inf();
#pragma unroll 8
        for (int q = 0; q < SMOOTH_CH; ++q) {
            const double al = logf_pair<MODEL>(k, sm[q], sm[q][D], sm[q][D + 1], xo);
            M = al > M ? al : M;
        }
        a.pmax[o] = M;
    } else if constexpr (PASS == 1) {
        double M = -inf();
        for (int c = 0; c < a.nmax; ++c) {
            const double pm = a.rmax[((size_t)c * a.ntheta + th) * n + j];
            M = pm > M ? pm : M;
        }
        double S = 0.0;
#pragma unroll 4
        for (int q = 0; q < SMOOTH_CH; ++q) {
            const double al = logf_pair<MODEL>(k, sm[q], sm[q][D], sm[q][D + 1], xo);
            S += sp_exp(al - M);
        }
        a.part[o] = S;
    } else if constexpr (PASS == 2) {
        double m[D], s, c;
        logf_source<MODEL>(k, xo, m, s, c);
        double S = 0.0;
#pragma unroll 4
        for (int q = 0; q < SMOOTH_CH; ++q) {
            const double lf = logf_pair<MODEL>(k, m, s, c, sm[q]);
            S += sm[q][D] * sp_exp(lf - sm[q][D + 1]);
        }
        a.part[o] = S;
    } else {   // PASS 3: PASS 2 with the pair moments (smc_spec.h "lag-one pair moments"); acc[0] is PASS 2's S, bit for bit
        double m[D], s, c;
        logf_source<MODEL>(k, xo, m, s, c);
        double acc[1 + 2 * D];
        for (int v = 0; v < 1 + 2 * D; ++v) acc[v] = 0.0;
#pragma unroll 4
        for (int q = 0; q < SMOOTH_CH; ++q) {
            const double p = pair_prob<MODEL>(k, m, s, c, sm[q], sm[q][D], sm[q][D + 1]);
            acc[0] += p;
            for (int r = 0; r < D; ++r) {
                acc[1 + r] += pair_x_term(p, sm[q][r]);
                acc[1 + D + r] += pair_r_term(p, sm[q][r], m[r]);
            }
        }
        const size_t vplane = (size_t)a.nchunk * plane;
        for (int v = 0; v < 1 + 2 * D; ++v) a.part[(size_t)v * vplane + o] = acc[v];
    }
}

// Every PASS 1 workgroup of a target needs M_j; with many chunks each of them would read all the chunk maxima again (n_x nchunk^2
// doubles per step and filter: 268 MB at 8192 particles).  Beyond this many chunks the maximum is taken once per target instead
// (one more small launch per step; a maximum is exact in any order, so the bits do not depend on the choice).
constexpr int SMOOTH_MAX_DIRECT = 8;
__global__ void k_smooth_rowmax(int64_t n, int ntheta, int nchunk, const double* pmax, double* rmax) {
    const int th = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double M = -inf();
    for (int c = 0; c < nchunk; ++c) {
        const double pm = pmax[((size_t)c * ntheta + th) * n + j];
        M = pm > M ? pm : M;
    }
    rmax[(size_t)th * n + j] = M;
}

// logD_j = M_j + sp_log(S_j): the maximum (as PASS 1 took it) and the chunk partials of target j in ascending chunk order
__global__ void k_smooth_logd(int64_t n, int ntheta, int nchunk, const double* rmax, int nmax, const double* part, double* logD) {
    const int th = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double M = -inf(), S = 0.0;
    for (int c = 0; c < nmax; ++c) {
        const double pm = rmax[((size_t)c * ntheta + th) * n + j];
        M = pm > M ? pm : M;
    }
    for (int c = 0; c < nchunk; ++c) S += part[((size_t)c * ntheta + th) * n + j];
    logD[(size_t)th * n + j] = M + sp_log(S);
}

// ws_t^i from the chunk partials of source i; part == nullptr: the last recorded step, ws = w.  dead[th] != 0: NaN
__global__ void k_smooth_finish(int64_t n, int ntheta, int nchunk, const double* part, const double* w, const int* dead, double* ws) {
    const int th = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double wi = w[(size_t)th * n + i];
    double r = wi;
    if (part) {
        double S = 0.0;
        for (int c = 0; c < nchunk; ++c) S += part[((size_t)c * ntheta + th) * n + i];
        r = wi > 0.0 ? wi * S : 0.0;
    }
    ws[(size_t)th * n + i] = dead[th] ? bits2d(0x7ff8000000000000ULL) : r;
}

// dead[th] = 1 when filter th has a recorded step at which every weight is 0 (a collapsed filter).  grid (T, ntheta); an
// integer flag, set by whoever finds such a step (dead is cleared before the launch)
__global__ void k_smooth_dead(int64_t n, int ntheta, const double* w /*[T][ntheta][n]*/, int* dead) {
    __shared__ int any;
    const int t = blockIdx.x, th = blockIdx.y;
    if (threadIdx.x == 0) any = 0;
    __syncthreads();
    const double* wt = w + ((size_t)t * ntheta + th) * n;
    int mine = 0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) mine |= wt[i] > 0.0 ? 1 : 0;
    if (mine) any = 1;   // (every writer stores the same value)
    __syncthreads();
    if (threadIdx.x == 0 && !any) atomicOr(dead + th, 1);
}

// smoothed mean and variance of every coordinate at every step: smc_get_moments' definitions on (x_t, ws_t) in the smoother's
// order of summation (smooth_sum: chunks of SMOOTH_CH, plain adds, partials in ascending order).  grid (T, ntheta), one
// workgroup per cloud; tmp [T][ntheta][nchunk] holds the chunk partials.  out [T][2][d][ntheta]
__global__ void k_smooth_moments(int64_t n, int ntheta, int nchunk, int d, const double* x /*[T][d][ntheta][n]*/,
                                 const double* ws /*[T][ntheta][n]*/, const int* dead, double* tmp, double* out) {
    __shared__ double s_mean;
    __shared__ int s_any;
    const int t = blockIdx.x, th = blockIdx.y;
    const double* wt = ws + ((size_t)t * ntheta + th) * n;
    double* part = tmp + ((size_t)t * ntheta + th) * nchunk;
    const double nan = bits2d(0x7ff8000000000000ULL);
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    int mine = 0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) mine |= wt[i] > 0.0 ? 1 : 0;
    if (mine) s_any = 1;
    __syncthreads();
    const bool none = dead[th] || !s_any;
    for (int r = 0; r < d; ++r) {
        const double* xr = x + (((size_t)t * d + r) * ntheta + th) * n;
        for (int pass = 0; pass < 2; ++pass) {
            const double mean = pass ? s_mean : 0.0;
            for (int c = threadIdx.x; c < nchunk; c += blockDim.x) {
                const int64_t i0 = (int64_t)c * SMOOTH_CH, i1 = i0 + SMOOTH_CH < n ? i0 + SMOOTH_CH : n;
                double s = 0.0;
                for (int64_t i = i0; i < i1; ++i) {
                    const double e = xr[i] - mean;
                    s += wt[i] > 0.0 ? (pass ? wt[i] * (e * e) : wt[i] * xr[i]) : 0.0;
                }
                part[c] = s;
            }
            __syncthreads();   // (the partials a workgroup wrote to global memory are visible to its own threads after the barrier)
            if (threadIdx.x == 0) {
                double tot = 0.0;
                for (int c = 0; c < nchunk; ++c) tot += part[c];
                if (!pass) s_mean = tot;
                out[(((size_t)t * 2 + pass) * d + r) * ntheta + th] = none ? nan : tot;
            }
            __syncthreads();
        }
    }
}

// cross[a][c] and resid2[c] of one backward step from the chunk partials PASS 3 left (planes 1 .. 2 D of pair): X_i^c and R_i^c
// are the partials of source i in ascending chunk order, the sums over i run in smooth_sum's order.  One workgroup per filter,
// PAIR_GROUP chunks of sources at a time: every thread forms the D D + D terms of its source (the loads of its partials are
// independent: unrolled, many in flight), thread (g, k) sums term k of chunk g in ascending order, and thread k adds the chunk
// sums, in ascending order again, to the total it keeps.  dead[th] != 0: NaN.  cross [D][D][ntheta], resid2 [D][ntheta]
constexpr int PAIR_GROUP = 512 / SMOOTH_CH;   // a workgroup of 512 threads whatever the chunk length (48 KB of LDS for three rows)
template <int D>
__global__ void __launch_bounds__(PAIR_GROUP * SMOOTH_CH)
k_smooth_pair_moments(int64_t n, int ntheta, int nchunk, const double* pair, const double* x /*[D][ntheta][n]*/,
                      const double* w /*[ntheta][n]*/, const int* dead, double* cross, double* resid2) {
    constexpr int NT = D * D + D;
    __shared__ double sm[PAIR_GROUP * SMOOTH_CH][NT];
    __shared__ double cs[PAIR_GROUP][NT];
    const int th = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)th * n, plane = (size_t)ntheta * n, vplane = (size_t)nchunk * plane;
    double tot = 0.0;
    for (int c0 = 0; c0 < nchunk; c0 += PAIR_GROUP) {
        const int64_t i = (int64_t)c0 * SMOOTH_CH + tid;
        double term[NT];
        for (int q = 0; q < NT; ++q) term[q] = 0.0;
        const double wi = i < n ? w[row + i] : 0.0;
        if (wi > 0.0) {   // (a source that is left out, or past the end: +0.0 whatever its partials hold)
            double X[D], R[D];
            for (int c = 0; c < D; ++c) X[c] = R[c] = 0.0;
            const double* pi = pair + vplane + row + i;
#pragma unroll 4
            for (int cc = 0; cc < nchunk; ++cc)
                for (int c = 0; c < D; ++c) {
                    X[c] += pi[(size_t)c * vplane + (size_t)cc * plane];
                    R[c] += pi[(size_t)(D + c) * vplane + (size_t)cc * plane];
                }
            for (int r = 0; r < D; ++r) {
                const double xr = x[(size_t)r * plane + row + i];
                for (int c = 0; c < D; ++c) term[r * D + c] = pair_cross_term(wi, xr, X[c]);
            }
            for (int c = 0; c < D; ++c) term[D * D + c] = pair_resid_term(wi, R[c]);
        }
        for (int q = 0; q < NT; ++q) sm[tid][q] = term[q];
        __syncthreads();
        if (tid < PAIR_GROUP * NT) {
            const int g = tid / NT, q = tid % NT;
            double s = 0.0;
#pragma unroll 8
            for (int p = 0; p < SMOOTH_CH; ++p) s += sm[g * SMOOTH_CH + p][q];
            cs[g][q] = s;
        }
        __syncthreads();   // (cs is written again only behind the next iteration's first barrier, which its readers below have passed)
        if (tid < NT)
            for (int g = 0; g < PAIR_GROUP && c0 + g < nchunk; ++g) tot += cs[g][tid];
    }
    if (tid < NT) {
        const double r = dead[th] ? bits2d(0x7ff8000000000000ULL) : tot;
        if (tid < D * D) cross[(size_t)tid * ntheta + th] = r;
        else resid2[(size_t)(tid - D * D) * ntheta + th] = r;
    }
}

// ---- quantiles of the smoothed state (smc_spec.h "quantiles of the smoothed state") --------------------------------
// Weighted quantiles of one state coordinate under the smoothed weights, at up to QMAX levels, for every recorded step and filter
// in ONE launch: grid (T, ntheta) like k_smooth_moments, one workgroup per cloud.
//   1. a pass over ws_t: K (integer LDS maximum) and the NaN test.  A NaN weight, or nobody who takes part: NaN at every level.
//   2. a pass that forms q_i and, when the cloud fits (n <= SMOOTH_Q_LDS_MAX), stages (order_key(x_i), q_i) in dynamic LDS; W =
//      sum q_i by 64-bit integer LDS atomics.  T_j = mulhi64(p64_j, W).
//   3. an MSB-first radix select on the 64-bit keys, 8 bits a pass: a level keeps (prefix, weight below the prefix); levels
//      with the same prefix share ONE 256-bin histogram of integer weights in LDS (its leader's: the first such level), filled
//      with integer LDS atomics from the staged pairs - or, above SMOOTH_Q_LDS_MAX, from keys and weights derived again from
//      global memory, the same integers.  Wave j mod 4 then finds the bin of level j by a wave scan over 4 bins per lane.  A
//      level whose candidates are one distinct key (the leader's integer minimum and maximum agree) is finished at once; the
//      loop ends when every level is.
// Integer sums only: no floating-point atomics, the order of the additions is immaterial.  Every store is a plain vector store.
constexpr int SMOOTH_Q_THREADS = 256;
constexpr int SMOOTH_Q_BINS = 256, SMOOTH_Q_PASSES = 8;
// the largest cloud that is staged: 16 bytes per particle, 128 KiB, beside the 16 KiB of histograms in the 160 KiB of a CU
constexpr int64_t SMOOTH_Q_LDS_MAX = 8192;
static_assert(QMAX == 8, "k_smooth_quantiles lays its per-level state out for 8 levels");
constexpr size_t SMOOTH_Q_FIXED_LDS = (size_t)QMAX * SMOOTH_Q_BINS * 8 + 64 * 8;   // the histograms and the per-level state
struct SmoothQArgs {
    int64_t n;
    int ntheta, d, component, np;
    const double* x;    // [T][d][ntheta][n] the recorded clouds
    const double* ws;   // [T][ntheta][n] the smoothed weights
    double* out;        // [T][ntheta][np]
    uint64_t p64[QMAX]; // the levels, 2^-64 fixed point (prob_to_u64)
};
__global__ void __launch_bounds__(SMOOTH_Q_THREADS) k_smooth_quantiles(SmoothQArgs a) {
    // all of the kernel's LDS is dynamic (the raised limit is the whole 160 KiB: static LDS on top of it is refused):
    // hist [QMAX][BINS] | W, kmin, kmax, prefix, below, target | K, nan, lead, fin | staged: key [n] | q [n]
    extern __shared__ __attribute__((aligned(16))) unsigned long long sq_lds[];
    unsigned long long(*hist)[SMOOTH_Q_BINS] = (unsigned long long(*)[SMOOTH_Q_BINS])sq_lds;
    unsigned long long* u = sq_lds + QMAX * SMOOTH_Q_BINS;
    unsigned long long &s_W = u[0], *kmin = u + 8, *kmax = u + 16, *prefix = u + 24, *below = u + 32, *target = u + 40;
    int* iv = (int*)(u + 48);
    int &s_K = iv[0], &s_nan = iv[1], *lead = iv + 8, *fin = iv + 16;
    unsigned long long* sq_stage = sq_lds + SMOOTH_Q_FIXED_LDS / 8;
    const int t = blockIdx.x, th = blockIdx.y, tid = threadIdx.x;
    const int64_t n = a.n;
    const double* wt = a.ws + ((size_t)t * a.ntheta + th) * n;
    const double* xt = a.x + (((size_t)t * a.d + a.component) * a.ntheta + th) * n;
    double* out = a.out + ((size_t)t * a.ntheta + th) * a.np;
    const bool staged = n <= SMOOTH_Q_LDS_MAX;
    if (tid == 0) { s_K = SMOOTH_Q_NOBODY; s_nan = 0; s_W = 0; }
    __syncthreads();
    int K = SMOOTH_Q_NOBODY, bad = 0;
    for (int64_t i = tid; i < n; i += SMOOTH_Q_THREADS) {
        const double w = wt[i];
        const int e = smooth_q_exponent(w);
        bad |= w != w ? 1 : 0;
        K = e > K ? e : K;
    }
    if (K != SMOOTH_Q_NOBODY) atomicMax(&s_K, K);
    if (bad) s_nan = 1;   // (every writer stores the same value)
    __syncthreads();
    K = s_K;
    if (s_nan || K == SMOOTH_Q_NOBODY) {   // (the same for every thread)
        if (tid < a.np) out[tid] = bits2d(0x7ff8000000000000ULL);
        return;
    }
    unsigned long long W = 0;
    for (int64_t i = tid; i < n; i += SMOOTH_Q_THREADS) {
        const uint64_t q = smooth_q_weight(wt[i], K);
        W += q;
        if (staged) {
            sq_stage[i] = q ? order_key(xt[i]) : 0;
            sq_stage[n + i] = q;
        }
    }
    if (W) atomicAdd(&s_W, W);
    __syncthreads();
    if (tid < QMAX) {   // every level starts with the empty prefix: one histogram, level 0's
        prefix[tid] = 0;
        below[tid] = 0;
        target[tid] = tid < a.np ? mulhi64(a.p64[tid], s_W) : 0;
        fin[tid] = tid < a.np ? 0 : 1;
        lead[tid] = tid < a.np ? 0 : -1;
    }
    __syncthreads();
    for (int pass = 0; pass < SMOOTH_Q_PASSES; ++pass) {
        const int shift = 56 - 8 * pass;
        const uint64_t above = pass ? ~(uint64_t)0 << (shift + 8) : 0;   // the bits of the key that the prefix has fixed
        unsigned own = 0;   // the levels that lead a histogram in this pass
        uint64_t pre[QMAX];
#pragma unroll
        for (int j = 0; j < QMAX; ++j) {
            own |= lead[j] == j ? 1u << j : 0u;
            pre[j] = prefix[j];
        }
        if (!own) break;   // (every level is finished; the same for every thread)
        for (int b = tid; b < QMAX * SMOOTH_Q_BINS; b += SMOOTH_Q_THREADS)
            if ((own >> (b / SMOOTH_Q_BINS)) & 1u) hist[b / SMOOTH_Q_BINS][b % SMOOTH_Q_BINS] = 0;
        if (tid < QMAX) { kmin[tid] = ~0ULL; kmax[tid] = 0; }
        __syncthreads();
        uint64_t lmin[QMAX], lmax[QMAX];
#pragma unroll
        for (int j = 0; j < QMAX; ++j) { lmin[j] = ~(uint64_t)0; lmax[j] = 0; }
        for (int64_t i = tid; i < n; i += SMOOTH_Q_THREADS) {
            const uint64_t q = staged ? (uint64_t)sq_stage[n + i] : smooth_q_weight(wt[i], K);
            if (!q) continue;
            const uint64_t key = staged ? (uint64_t)sq_stage[i] : order_key(xt[i]);
            const int bin = (int)(key >> shift) & (SMOOTH_Q_BINS - 1);
#pragma unroll
            for (int j = 0; j < QMAX; ++j)
                if (((own >> j) & 1u) && (key & above) == pre[j]) {
                    atomicAdd(&hist[j][bin], (unsigned long long)q);
                    lmin[j] = key < lmin[j] ? key : lmin[j];
                    lmax[j] = key > lmax[j] ? key : lmax[j];
                }
        }
#pragma unroll
        for (int j = 0; j < QMAX; ++j)
            if (lmin[j] <= lmax[j]) {   // (this thread met a candidate of leader j)
                atomicMin(&kmin[j], (unsigned long long)lmin[j]);
                atomicMax(&kmax[j], (unsigned long long)lmax[j]);
            }
        __syncthreads();
        // the bin of every unfinished level: below <= T < below + (the weight of its candidates), so a bin is found
        const int wave = tid >> 6, lane = tid & 63;
        for (int j = wave; j < QMAX; j += SMOOTH_Q_THREADS / 64) {   // (the same for every lane of the wave)
            const int L = lead[j];
            if (L < 0) continue;
            if (kmin[L] == kmax[L]) {   // one distinct candidate
                if (lane == 0) { out[j] = key_value(kmin[L]); fin[j] = 1; }
                continue;
            }
            const unsigned long long* h = &hist[L][4 * lane];
            const unsigned long long h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], s = h0 + h1 + h2 + h3;
            unsigned long long incl = s;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long v = __shfl_up(incl, o);
                incl += lane >= o ? v : 0;
            }
            const unsigned long long b0 = below[j], T = target[j];
            const unsigned long long over = __ballot(b0 + incl > T);
            if (over && lane == __ffsll((long long)over) - 1) {
                unsigned long long c = b0 + incl - s;
                int b = 4 * lane;
                if (c + h0 <= T) {
                    c += h0; ++b;
                    if (c + h1 <= T) {
                        c += h1; ++b;
                        if (c + h2 <= T) { c += h2; ++b; }
                    }
                }
                const unsigned long long np_ = prefix[j] | ((unsigned long long)b << shift);
                below[j] = c;
                prefix[j] = np_;
                if (pass == SMOOTH_Q_PASSES - 1) { out[j] = key_value(np_); fin[j] = 1; }   // (all 64 bits chosen)
            }
        }
        __syncthreads();
        int L = -1;   // the leader of level tid in the next pass: the first unfinished level with its prefix
        if (tid < QMAX && !fin[tid])
            for (int jj = tid; jj >= 0; --jj) L = (!fin[jj] && prefix[jj] == prefix[tid]) ? jj : L;
        if (tid < QMAX) lead[tid] = L;
        __syncthreads();
    }
}

}  // namespace smc
