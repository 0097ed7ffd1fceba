// smc_util_kernels.h -- kernels of the stand-alone entry points (normalize, resample; the batched scalar Kalman filter is
// k_kalman_loglik<Lg1Row> of smc_kalman_rows.h).  Included by smc_util.hip only.
#pragma once
#include "smc_kalman_rows.h"
#include "smc_kernels.h"

namespace smc {

// ---------------------------------------------------------------------------------------------
// stand-alone A1 / A2 (outer theta-level reweight / resample; n <= a few thousand): one
// workgroup, single level, all integer sums.
// ---------------------------------------------------------------------------------------------
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_normalize(const double* logw, int64_t n, int K, double* w, double* out2) {
    constexpr int NW = THREADS / WAVE;
    __shared__ double red[NW];
    __shared__ uint64_t acc[3][NW];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    double kmax = -inf();
    for (int64_t i = tid; i < n; i += THREADS) {
        const double l = logw[i];
        if (lw_alive(l)) { double k; (void)sp_exp_parts(l, k); kmax = k > kmax ? k : kmax; }
    }
    kmax = block_max<THREADS>(kmax, red);
    uint64_t S = 0;
    U128 s2{0, 0};
    for (int64_t i = tid; i < n; i += THREADS) {
        const double l = logw[i];
        uint64_t q = 0;
        if (lw_alive(l)) { double k; const double p = sp_exp_parts(l, k); q = fix_weight(p, k - kmax, K); }
        S += q;
        s2 = add128(s2, sq128(q));
    }
    S = wave_sum(S);
    s2 = wave_sum128(s2);
    if (lane == 0) { acc[0][wave] = S; acc[1][wave] = s2.lo; acc[2][wave] = s2.hi; }
    __syncthreads();
    uint64_t St = 0;
    U128 t2{0, 0};
#pragma unroll
    for (int k = 0; k < NW; ++k) { St += acc[0][k]; t2 = add128(t2, U128{acc[1][k], acc[2][k]}); }
    const double Sd = (double)St;
    for (int64_t i = tid; i < n; i += THREADS) {
        const double l = logw[i];
        uint64_t q = 0;
        if (lw_alive(l)) { double k; const double p = sp_exp_parts(l, k); q = fix_weight(p, k - kmax, K); }
        w[i] = St ? (double)q / Sd : 0.0;
    }
    if (tid == 0) {
        out2[0] = St ? fma(kmax, LN2_HI, fma(kmax, LN2_LO, sp_log(Sd * pow2i(-K)))) - sp_log((double)n) : -inf();
        out2[1] = St ? (Sd * Sd) / u128_to_double(t2.hi, t2.lo) : 0.0;
    }
}

// The same normalize() for long vectors (a whole particle cloud's log-weights): three grid-wide passes.  Every
// cross-workgroup combination is an integer operation (max of the integer exponents, sums of the fixed-point weights, sums
// of the three 32-bit limbs of their squares), so the order the workgroups arrive in cannot change a bit: the results are
// those of the one-workgroup kernel above.  acc: [0] sum q  [1..3] sums of the limbs of q^2; kmax_i: exponent maximum.
constexpr int NORM_DEAD = (int)0x80000000;
__device__ __forceinline__ uint64_t norm_q(double l, int kmax_i, int K) {
    if (!lw_alive(l) || kmax_i == NORM_DEAD) return 0;
    double k;
    const double p = sp_exp_parts(l, k);
    return fix_weight(p, k - (double)kmax_i, K);
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_normalize_max(const double* logw, int64_t n, int* kmax_i) {
    __shared__ int red[THREADS / WAVE];
    int km = NORM_DEAD;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const double l = logw[i];
        if (lw_alive(l)) { double k; (void)sp_exp_parts(l, k); const int ki = (int)k; km = ki > km ? ki : km; }
    }
    km = block_max_i32<THREADS>(km, red);
    if (threadIdx.x == 0 && km != NORM_DEAD) atomicMax(kmax_i, km);
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_normalize_sum(const double* logw, int64_t n, int K, const int* kmax_i,
                                                          unsigned long long* acc) {
    constexpr int NW = THREADS / WAVE;
    __shared__ uint64_t part[4][NW];
    const int km = *kmax_i, lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    uint64_t s[4] = {0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const uint64_t q = norm_q(logw[i], km, K);
        const U128 q2 = sq128(q);
        s[0] += q;
        s[1] += q2.lo & 0xffffffffULL;
        s[2] += q2.lo >> 32;
        s[3] += q2.hi;                     // q < 2^48: q^2 < 2^96, the top limb is below 2^32
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t t = wave_sum(s[j]);
        if (lane == 0) part[j][wave] = t;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint64_t t = 0;
        for (int w = 0; w < NW; ++w) t += part[threadIdx.x][w];
        if (t) atomicAdd(&acc[threadIdx.x], (unsigned long long)t);
    }
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_normalize_write(const double* logw, int64_t n, int K, const int* kmax_i,
                                                            const unsigned long long* acc, double* w, double* out2) {
    const int km = *kmax_i;
    const uint64_t St = acc[0];
    const double Sd = (double)St;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const uint64_t q = norm_q(logw[i], km, K);
        w[i] = St ? (double)q / Sd : 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // sum q^2 = l0 + l1 2^32 + l2 2^64 as a 128-bit integer
        const uint64_t l0 = acc[1], l1 = acc[2], l2 = acc[3];
        const uint64_t lo = l0 + (l1 << 32);
        const uint64_t hi = l2 + (l1 >> 32) + (lo < l0 ? 1u : 0u);
        const double kmax = km == NORM_DEAD ? -inf() : (double)km;
        out2[0] = St ? fma(kmax, LN2_HI, fma(kmax, LN2_LO, sp_log(Sd * pow2i(-K)))) - sp_log((double)n) : -inf();
        out2[1] = St ? (Sd * Sd) / u128_to_double(hi, lo) : 0.0;
    }
}

// q_i = rint(w_i / wmax * 2^K) ; C = inclusive scan (single workgroup, chunked)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_resample_cdf(const double* w, int64_t n, int K, uint64_t* C, int* status) {
    constexpr int NW = THREADS / WAVE;
    __shared__ double red[NW];
    __shared__ uint64_t wt[NW];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    double m = 0.0;
    for (int64_t i = tid; i < n; i += THREADS) { const double x = w[i]; m = x > m ? x : m; }
    m = block_max<THREADS>(m, red);
    if (!(m > 0.0) || m == inf()) { if (tid == 0) *status = -2; return; }
    const double scale = pow2i(K);
    uint64_t carry = 0;
    for (int64_t base = 0; base < n; base += THREADS) {
        const int64_t i = base + tid;
        uint64_t q = 0;
        if (i < n) { const double r = w[i] / m; q = (r == r && r > 0.0) ? (uint64_t)rne_pos(r * scale) : 0; }
        const uint64_t incl = wave_incl_scan(q, lane);
        if (lane == WAVE - 1) wt[wave] = incl;
        __syncthreads();
        uint64_t off = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) { off += (k < wave) ? wt[k] : 0; tot += wt[k]; }
        if (i < n) C[i] = carry + off + incl;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) *status = 0;
}

// The same inclusive sums for a long vector, grid-wide (every cross-workgroup combination an integer sum or a maximum: the same
// bits as the single workgroup): the maximum; the sum of every workgroup's contiguous chunk; their exclusive scan (one workgroup);
// the chunk's inclusive sums on top of its offset.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_rs_max(const double* w, int64_t n, unsigned long long* mbits) {
    __shared__ double red[THREADS / WAVE];
    double m = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) { const double x = w[i]; m = x > m ? x : m; }
    m = block_max<THREADS>(m, red);
    if (threadIdx.x == 0) atomicMax(mbits, (unsigned long long)d2bits(m));   // (non-negative doubles order like their bits; +inf included)
}
__device__ __forceinline__ uint64_t rs_q(double w, double m, double scale) {
    const double r = w / m;
    return (r == r && r > 0.0) ? (uint64_t)rne_pos(r * scale) : 0;
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_rs_chunk_sums(const double* w, int64_t n, int K, const unsigned long long* mbits, int64_t chunk, uint64_t* bs) {
    __shared__ uint64_t wt[THREADS / WAVE];
    const double m = bits2d(*mbits);
    if (!(m > 0.0) || m == inf()) return;
    const double scale = pow2i(K);
    const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
    uint64_t s = 0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += THREADS) s += rs_q(w[i], m, scale);
    s = wave_sum(s);
    if ((threadIdx.x & (WAVE - 1)) == 0) wt[threadIdx.x / WAVE] = s;
    __syncthreads();
    if (threadIdx.x == 0) { uint64_t t = 0; for (int k = 0; k < THREADS / WAVE; ++k) t += wt[k]; bs[blockIdx.x] = t; }
}
// one workgroup: exclusive scan of the nb chunk sums in place; status = -2 for an unusable maximum
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_rs_scan_chunks(const unsigned long long* mbits, int nb, uint64_t* bs, int* status) {
    constexpr int NW = THREADS / WAVE;
    __shared__ uint64_t wt[NW];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const double m = bits2d(*mbits);
    if (!(m > 0.0) || m == inf()) { if (tid == 0) *status = -2; return; }
    uint64_t carry = 0;
    for (int base = 0; base < nb; base += THREADS) {
        const int i = base + tid;
        const uint64_t v = i < nb ? bs[i] : 0;
        const uint64_t incl = wave_incl_scan(v, lane);
        if (lane == WAVE - 1) wt[wave] = incl;
        __syncthreads();
        uint64_t off = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) { off += (k < wave) ? wt[k] : 0; tot += wt[k]; }
        if (i < nb) bs[i] = carry + off + incl - v;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) *status = 0;
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_rs_write(const double* w, int64_t n, int K, const unsigned long long* mbits, int64_t chunk, const uint64_t* bs,
                                                      uint64_t* C) {
    constexpr int NW = THREADS / WAVE;
    __shared__ uint64_t wt[NW];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const double m = bits2d(*mbits);
    if (!(m > 0.0) || m == inf()) return;
    const double scale = pow2i(K);
    const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
    uint64_t carry = bs[blockIdx.x];
    for (int64_t base = i0; base < i1; base += THREADS) {
        const int64_t i = base + tid;
        const uint64_t q = i < i1 ? rs_q(w[i], m, scale) : 0;
        const uint64_t incl = wave_incl_scan(q, lane);
        if (lane == WAVE - 1) wt[wave] = incl;
        __syncthreads();
        uint64_t off = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) { off += (k < wave) ? wt[k] : 0; tot += wt[k]; }
        if (i < i1) C[i] = carry + off + incl;
        carry += tot;
        __syncthreads();
    }
}

__global__ void k_resample_draw(const uint64_t* C, int64_t n, int64_t ndraw, uint64_t seed, uint32_t stream, uint32_t t,
                                int32_t* a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ndraw) return;
    const u32x4 rw = draw(seed, (uint32_t)(i >> 1), stream, t, SLOT_RESAMPLE);
    const int j = (int)(i & 1);
    const uint64_t r = ((uint64_t)rw.v[2 * j + 1] << 32) | rw.v[2 * j];
    const uint64_t S = C[n - 1];
    uint64_t T, lo;
    mul64wide(r, S, T, lo);
    int64_t l = 0, h = n;
    while (l < h) {
        const int64_t mid = (l + h) >> 1;
        if (C[mid] > T) h = mid; else l = mid + 1;
    }
    a[i] = (int32_t)(l < n ? l : n - 1);
}

}  // namespace smc
