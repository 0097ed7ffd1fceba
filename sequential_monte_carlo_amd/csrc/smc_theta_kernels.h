// smc_theta_kernels.h -- quantiles and histograms of the theta cloud of an IBIS handle on the device (smc_spec.h "quantiles and
// histograms of the theta cloud").  Included by smc_ibis.hip behind smc_ibis_kernels.h.
// Every value that crosses a workgroup is an INTEGER (fixed-point weights, their sums, exponent maxima, keys): sums, minima and
// maxima in any order give the same bits, so no result depends on the grid.  No float atomics.
//   k_theta_weights   q [M] (plain stores) and W = sum q of the committed logw against the cloud's K (k_ibis_kmax)
//   k_theta_digits    one pass of the radix select, most significant digit first, for all d coordinates and all np levels of a
//                     call: per (coordinate, level) the weight per digit among the keys that match the level's prefix - its
//                     candidates - in LDS, flushed with one 64-bit integer atomic per occupied bin and workgroup; and the
//                     smallest and the largest candidate key.  Levels of a coordinate that still share a prefix share a
//                     histogram (that of the lowest such level, their leader).
//   k_theta_pick      one workgroup between the passes (the k_ms_pick pattern): every level's digit and the weight below it;
//                     a level whose candidates are ONE distinct key is finished with it; then the leaders of the next pass.
//                     pass = -1 sets a call up; the last pass finishes what is left.
//   k_theta_hist      the histogram call: one pass of the same shape with the value slots of theta_hist_slot in place of digits
// The state between the passes stays on the device (ThetaSel); a call reads back d np doubles and synchronises once.  The host
// enqueues all passes; once every level is finished the remaining launches return at their first instruction.
#pragma once
#include "smc_ibis_kernels.h"

namespace smc {

constexpr int THETA_SEL_BITS = 8;                                  // digit width: 8 passes over a 64-bit key
constexpr int THETA_SEL_BINS = 1 << THETA_SEL_BITS;
constexpr int THETA_SEL_PASSES = 64 / THETA_SEL_BITS;
constexpr int THETA_SEL_SLOTS = MAX_DTHETA * QMAX;                 // slot of (coordinate c, level j): c QMAX + j
constexpr int THETA_MAX_GROUPS = 512;                              // workgroups of a streaming pass at most (each flushes its bins): two per CU, measured
constexpr int THETA_AGG_MIN = 8;                                   // lanes of a wave on ONE bin from which they are summed before the LDS atomic
static_assert(IBIS_RED_THREADS == THETA_SEL_BINS && THETA_SEL_SLOTS == 64, "k_theta_pick: four bins per lane, one lane per slot");

// the levels of a call, 2^-64 fixed point (prob_to_u64)
struct ThetaLevels { uint64_t p64[QMAX]; };
// views into the handle's scratch block (smc_ibis.hip carves it)
struct ThetaSel {
    unsigned long long* W;       // [1] sum of q
    uint32_t* active;            // [1] slots that still select; 0: the passes return at once
    uint64_t* prefix;            // [SLOTS] the digits chosen so far, in place
    uint64_t* T;                 // [SLOTS] the target among the candidates
    double* out;                 // [SLOTS]
    unsigned long long* kmin;    // [SLOTS] the smallest and the largest candidate key of a leader's pass (all-ones / 0 between
    unsigned long long* kmax;    // [SLOTS]   the passes)
    int32_t* lead;               // [SLOTS] the slot whose histogram this slot reads; -1: unused or finished
    unsigned long long* hist;    // [SLOTS][BINS], zero between the passes
};
constexpr size_t THETA_SEL_WORDS = 2 + 5 * THETA_SEL_SLOTS + THETA_SEL_SLOTS / 2 + (size_t)THETA_SEL_SLOTS * THETA_SEL_BINS;
__host__ __device__ inline ThetaSel theta_sel_carve(uint64_t* w) {
    ThetaSel s;
    s.W = (unsigned long long*)w;
    s.active = (uint32_t*)(w + 1);
    s.prefix = w + 2;
    s.T = s.prefix + THETA_SEL_SLOTS;
    s.out = (double*)(s.T + THETA_SEL_SLOTS);
    s.kmin = (unsigned long long*)(s.T + 2 * THETA_SEL_SLOTS);
    s.kmax = s.kmin + THETA_SEL_SLOTS;
    s.lead = (int32_t*)(s.kmax + THETA_SEL_SLOTS);
    s.hist = s.kmax + THETA_SEL_SLOTS + THETA_SEL_SLOTS / 2;
    return s;
}

// Kb: the cloud's biased K (k_ibis_kmax); W zeroed by the caller
__global__ __launch_bounds__(IBIS_RED_THREADS) void k_theta_weights(IbisView v, int cs, const uint32_t* Kb, uint64_t* q, unsigned long long* W) {
    const int K = ibis_unbias_ki(*Kb);
    uint64_t s = 0;
    for (int64_t m = (int64_t)blockIdx.x * IBIS_RED_THREADS + threadIdx.x; m < v.M; m += (int64_t)gridDim.x * IBIS_RED_THREADS) {
        int k;
        const double p = ibis_sum_parts(v.logw[cs][m], true, k);
        const uint64_t qi = theta_q(p, k, K);
        q[m] = qi;
        s += qi;
    }
    __shared__ unsigned long long wg;      // (one atomic per workgroup, as k_ibis_kmax)
    if (threadIdx.x == 0) wg = 0;
    __syncthreads();
    s = wave_sum_u64(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&wg, (unsigned long long)s);
    __syncthreads();
    if (threadIdx.x == 0 && wg) atomicAdd(W, wg);
}

// v of lane `lane` (wave-uniform) in every lane
__device__ __forceinline__ uint64_t wave_read_u64(uint64_t v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

// dynamic LDS: D np histograms of THETA_SEL_BINS words.  Every lane of a wave walks the loops together (ballots and shuffles).
template <int D>
__global__ __launch_bounds__(IBIS_RED_THREADS) void k_theta_digits(const double* theta /*[M][MAX_DTHETA]*/, const uint64_t* q, int64_t M, int np, int pass,
                                                                  ThetaSel st) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long* lh = (unsigned long long*)smem;
    __shared__ uint64_t pre[D * QMAX];                   // the prefix above this pass's digit
    __shared__ int own[D * QMAX];                        // the slot is a leader: it has a histogram in this pass
    __shared__ unsigned long long lmin[D * QMAX], lmax[D * QMAX];
    if (*st.active == 0) return;                         // (uniform over the grid: k_theta_pick wrote it before this launch)
    const int tid = threadIdx.x, lane = tid & 63, shift = 64 - THETA_SEL_BITS * (pass + 1);
    for (int i = tid; i < D * np * THETA_SEL_BINS; i += IBIS_RED_THREADS) lh[i] = 0;
    if (tid < D * QMAX) {
        own[tid] = st.lead[tid] == tid;
        pre[tid] = pass ? st.prefix[tid] >> (shift + THETA_SEL_BITS) : 0;
        lmin[tid] = ~0ULL;
        lmax[tid] = 0;
    }
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * IBIS_RED_THREADS; base < M; base += (int64_t)gridDim.x * IBIS_RED_THREADS) {
        const int64_t m = base + tid;
        const bool valid = m < M;
        const uint64_t w = valid ? q[m] : 0;
        if (!__ballot(w != 0)) continue;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const uint64_t key = order_key(theta[(valid ? m : M - 1) * MAX_DTHETA + c]);
            const uint64_t above = pass ? key >> (shift + THETA_SEL_BITS) : 0;
            const int digit = (int)((key >> shift) & (THETA_SEL_BINS - 1));
            for (int j = 0; j < np; ++j) {
                const int s = c * QMAX + j;
                if (!own[s]) continue;
                const bool hit = w != 0 && pre[s] == above;
                const unsigned long long mask = __ballot(hit);
                if (!mask) continue;
                unsigned long long* bins = lh + (size_t)(c * np + j) * THETA_SEL_BINS;
                const int first = __ffsll(mask) - 1, nhit = __popcll(mask);
                const uint64_t k0 = wave_read_u64(key, first);
                const int d0 = (int)((k0 >> shift) & (THETA_SEL_BINS - 1));
                // the candidate keys of this wave: one distinct key adds itself to the slot's range, several open the range wide
                const bool one_key = !__ballot(hit && key != k0);
                if (lane == first) {
                    atomicMin(&lmin[s], one_key ? (unsigned long long)k0 : 0ULL);
                    atomicMax(&lmax[s], one_key ? (unsigned long long)k0 : ~0ULL);
                }
                if (nhit >= THETA_AGG_MIN && !__ballot(hit && digit != d0)) {   // many lanes on one bin: one LDS atomic, not nhit serial ones
                    const uint64_t sum = wave_sum_u64(hit ? w : 0);
                    if (lane == first) atomicAdd(&bins[d0], (unsigned long long)sum);
                } else if (hit) {
                    atomicAdd(&bins[digit], (unsigned long long)w);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < D * np * THETA_SEL_BINS; i += IBIS_RED_THREADS)
        if (lh[i]) {
            const int cj = i / THETA_SEL_BINS, c = cj / np, j = cj - c * np;
            atomicAdd(&st.hist[(size_t)(c * QMAX + j) * THETA_SEL_BINS + (i & (THETA_SEL_BINS - 1))], lh[i]);
        }
    if (tid < D * QMAX && own[tid] && lmin[tid] <= lmax[tid]) {
        atomicMin(&st.kmin[tid], lmin[tid]);
        atomicMax(&st.kmax[tid], lmax[tid]);
    }
}

// one workgroup.  pass = -1: the set-up of a call (every level of a coordinate behind its level 0, the histograms zero);
// pass 0 .. PASSES - 1: behind k_theta_digits of that pass
__global__ __launch_bounds__(IBIS_RED_THREADS) void k_theta_pick(int d, int np, int pass, ThetaLevels lv, ThetaSel st) {
    __shared__ int fin[THETA_SEL_SLOTS];   // the slot selects no further (unused, or finished in this pass or before)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = (tid & 63) / QMAX, j = tid & (QMAX - 1);     // the slot of lane `tid` of wave 0
    const bool used = tid < THETA_SEL_SLOTS && c < d && j < np;
    const uint64_t nan = 0x7ff8000000000000ULL;
    if (pass >= 0) {
        if (*st.active == 0) return;
        const uint64_t W = *st.W;
        const int shift = 64 - THETA_SEL_BITS * (pass + 1);
        // a wave per slot, four bins per lane: the bin with  below <= T < below + h  (T < the histogram's total: one lane has it)
        for (int s = wave; s < THETA_SEL_SLOTS; s += IBIS_RED_THREADS / 64) {
            const int L = st.lead[s];
            if (L < 0) continue;           // (wave-uniform)
            const uint64_t T = pass ? st.T[s] : __umul64hi(lv.p64[s & (QMAX - 1)], W);
            const unsigned long long* hb = st.hist + (size_t)L * THETA_SEL_BINS + lane * 4;
            uint64_t hq[4], sum = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) { hq[t] = hb[t]; sum += hq[t]; }
            uint64_t incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint64_t up = (uint64_t)__shfl_up((unsigned long long)incl, o, 64);
                incl += lane >= o ? up : 0;
            }
            uint64_t run = incl - sum;
            if (sum && run <= T && T < run + sum) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (hq[t] && run <= T && T < run + hq[t]) {
                        st.T[s] = T - run;
                        st.prefix[s] = (pass ? st.prefix[s] : 0) | ((uint64_t)(lane * 4 + t) << shift);
                    }
                    run += hq[t];
                }
            }
        }
        __syncthreads();                   // the prefixes of every slot are written, every histogram has been read
        int L = tid < THETA_SEL_SLOTS ? st.lead[tid] : -1;
        if (tid < THETA_SEL_SLOTS) {
            if (used && W == 0) { st.out[tid] = bits2d(nan); L = -1; }
            else if (L >= 0 && st.kmin[L] == st.kmax[L]) { st.out[tid] = key_value(st.kmin[L]); L = -1; }           // one distinct candidate
            else if (L >= 0 && pass == THETA_SEL_PASSES - 1) { st.out[tid] = key_value(st.prefix[tid]); L = -1; }   // (all 64 bits chosen)
            fin[tid] = L < 0;
        }
        __syncthreads();                   // (every slot has read its old leader's range)
        if (tid < THETA_SEL_SLOTS) {
            if (L >= 0) {                  // the lowest level of the coordinate that still selects and has this prefix
                const uint64_t mine = st.prefix[tid];
                for (int jj = j; jj >= 0; --jj) L = (!fin[c * QMAX + jj] && st.prefix[c * QMAX + jj] == mine) ? c * QMAX + jj : L;
            }
            st.lead[tid] = L;
            st.kmin[tid] = ~0ULL;
            st.kmax[tid] = 0;
            const unsigned long long on = __ballot(L >= 0);
            if (tid == 0) *st.active = (uint32_t)__popcll(on);
        }
    } else if (tid < THETA_SEL_SLOTS) {
        st.lead[tid] = used ? c * QMAX : -1;
        st.out[tid] = bits2d(nan);
        st.kmin[tid] = ~0ULL;
        st.kmax[tid] = 0;
        if (tid == 0) *st.active = (uint32_t)(d * np);
    }
    for (int i = tid; i < d * QMAX * THETA_SEL_BINS; i += IBIS_RED_THREADS) st.hist[i] = 0;     // (the coordinates in use)
}

// counts [nbins + 3] zeroed by the caller
__global__ __launch_bounds__(IBIS_RED_THREADS) void k_theta_hist(const double* theta, const uint64_t* q, int64_t M, int comp, double lo, double hi, double scale,
                                                                int nbins, unsigned long long* counts) {
    __shared__ unsigned long long lh[THETA_HIST_MAXBINS + 3];
    const int tid = threadIdx.x;
    for (int i = tid; i < nbins + 3; i += IBIS_RED_THREADS) lh[i] = 0;
    __syncthreads();
    for (int64_t m = (int64_t)blockIdx.x * IBIS_RED_THREADS + tid; m < M; m += (int64_t)gridDim.x * IBIS_RED_THREADS) {
        const uint64_t w = q[m];
        if (w) atomicAdd(&lh[theta_hist_slot(theta[m * MAX_DTHETA + comp], lo, hi, scale, nbins)], (unsigned long long)w);
    }
    __syncthreads();
    for (int i = tid; i < nbins + 3; i += IBIS_RED_THREADS)
        if (lh[i]) atomicAdd(&counts[i], lh[i]);
}

}  // namespace smc
