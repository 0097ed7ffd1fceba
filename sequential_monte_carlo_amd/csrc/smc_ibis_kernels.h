// smc_ibis_kernels.h -- the IBIS sampler (src/ibis.jl): SMC^2 whose inner "filter" is an exact Kalman filter, of the univariate
// LinearModel (Lg1Row) or of a two-state linear model (Lg2Row).  One lane per parameter particle; the whole state of a particle is
// (theta, row, x, Sigma, logZ, logw), resident on the device for the life of the handle.  Included by smc_ibis.hip only.
//
// The five kernels that touch a row or a state are templates on the row kind (smc_kalman_rows.h): one text for both kinds, the
// lengths and the step function from the trait.  Everything else (summaries, ESS records, resampling, moments of theta) reads
// theta, logw and M alone - or is for scalar rows only, which the handle enforces.
//
//   k_ibis_init        theta -> model rows, (x, Sigma) = the row's initial state, logZ = logw = 0          ibis.jl:35-43
//   k_ibis_reset       the same state from the rows alone
//   k_ibis_window      k online steps smc²! (:166-187; smc², :134-147, is k = 1 from the initial state) and the segment
//                      records of the outer reweight after every step
//   k_ibis_rejuvenate  rejuvenate! (:86-125): the whole chain of PMMH moves of a particle, Kalman re-filters included
//   k_ibis_permute     resample! (:73-84): gather through the ancestor vector
//
// Random numbers: pmmh_propose / pmmh_log_uniform keyed by (move_seed, stream = index of the parameter particle, chain
// position) and nothing else, so no result depends on the launch geometry.  Every store is a plain vector store.
#pragma once
#include "smc_ibis_view.h"

namespace smc {

// smc.model(theta) as a gather without a run-time index into registers: row[k] = theta[from[k]] or cst[k]
template <class Row, int D>
__device__ __forceinline__ void ibis_row(const IbisRowMap& s, const double* th, double* row) {
#pragma unroll
    for (int k = 0; k < Row::NRAW; ++k) {
        double v = s.cst[k];
        const int from = s.from[k];
#pragma unroll
        for (int i = 0; i < D; ++i) v = from == i ? th[i] : v;
        row[k] = v;
    }
}

// (x, S) of particle m of a set of the view <-> the registers of its lane
template <class Row>
__device__ __forceinline__ void ibis_load_state(const IbisView& v, int cs, int64_t m, double* x, double* S) {
#pragma unroll
    for (int i = 0; i < Row::NX; ++i) x[i] = v.x[cs][m * Row::NX + i];
#pragma unroll
    for (int i = 0; i < Row::NS; ++i) S[i] = v.S[cs][m * Row::NS + i];
}
template <class Row>
__device__ __forceinline__ void ibis_store_state(const IbisView& v, int cs, int64_t m, const double* x, const double* S) {
#pragma unroll
    for (int i = 0; i < Row::NX; ++i) v.x[cs][m * Row::NX + i] = x[i];
#pragma unroll
    for (int i = 0; i < Row::NS; ++i) v.S[cs][m * Row::NS + i] = S[i];
}

// theta -> rows and the initial state of every particle   ibis.jl:38-43
template <class Row, int D>
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_init(IbisView v, int cp, int cs, IbisRowMap s) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    if (m >= v.M) return;
    double th[D], row[Row::NRAW];
#pragma unroll
    for (int i = 0; i < D; ++i) th[i] = v.theta[cp][m * MAX_DTHETA + i];
    ibis_row<Row, D>(s, th, row);
#pragma unroll
    for (int k = 0; k < Row::NRAW; ++k) v.raw[cp][m * Row::NRAW + k] = row[k];
    ibis_store_state<Row>(v, cs, m, row + Row::X0, row + Row::S0);
    v.logZ[cs][m] = 0.0;
    v.logw[cs][m] = 0.0;
}

// The same state from the rows alone: the beginning of a whole-series filter (density_tempered's first pass)
template <class Row>
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_reset(IbisView v, int cp, int cs) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    if (m >= v.M) return;
    const double* row = v.raw[cp] + m * Row::NRAW;
    ibis_store_state<Row>(v, cs, m, row + Row::X0, row + Row::S0);
    v.logZ[cs][m] = 0.0;
    v.logw[cs][m] = 0.0;
}

// ---- summaries of the cloud (smc_spec.h "summaries of an IBIS cloud"; plotting_utils.jl:94-137) ------------------------------
// A workgroup is one wave and owns one chunk.  part: [IBIS_SUM_NCOL][nchunk] doubles per row of summaries (one row per step of
// a window), column-major so that the combine's left-to-right sums read consecutive addresses: columns 0..9 the chunk record,
// the rest scratch of k_ibis_sum_combine.
static_assert(IBIS_THREADS == IBIS_SUM_CHUNK, "one wave per chunk of the summaries");
constexpr int IBIS_SUM_NCOL = 16;
constexpr int IBIS_SUM_CTHREADS = 256;

__device__ __forceinline__ double wave_tree_sum(double v) {   // a[i] += a[i ^ s], s = 1, 2, .., 32: the same bits in every lane
#pragma unroll
    for (int s = 1; s < IBIS_SUM_CHUNK; s <<= 1) v = v + __shfl_xor(v, s, IBIS_SUM_CHUNK);
    return v;
}

// the record of the chunk this wave holds, from the registers of its lanes; lane 0 stores it (vector stores)
__device__ __forceinline__ void ibis_chunk_record(double A, double B, double Q, double R, double x, double S, double logw, bool valid,
                                                  int ahead, double* part, int64_t nchunk, int64_t c) {
    int k;
    const double p = ibis_sum_parts(logw, valid, k);
    int kc = k;
#pragma unroll
    for (int s = 1; s < IBIS_SUM_CHUNK; s <<= 1) { const int o = __shfl_xor(kc, s, IBIS_SUM_CHUNK); kc = o > kc ? o : kc; }
    const double u = ibis_sum_u(p, k, kc);
    double um = u;
#pragma unroll
    for (int s = 1; s < IBIS_SUM_CHUNK; s <<= 1) { const double o = __shfl_xor(um, s, IBIS_SUM_CHUNK); um = o > um ? o : um; }
    const unsigned long long top = __ballot(u > 0.0 && u == um);
    const int ls = top ? __ffsll(top) - 1 : 0;
    double ym, vm;
    ibis_obs_moments(A, B, Q, R, x, S, ahead != 0, ym, vm);
    const double cy = top ? __shfl(ym, ls, IBIS_SUM_CHUNK) : 0.0, cx = top ? __shfl(x, ls, IBIS_SUM_CHUNK) : 0.0;
    double t[7];
    ibis_sum_terms(u, ym, vm, x, S, cy, cx, t);
#pragma unroll
    for (int i = 0; i < 7; ++i) t[i] = wave_tree_sum(t[i]);
    if (threadIdx.x == 0) {
        part[ISF_KC * nchunk + c] = kc == IBIS_SUM_DEADK ? -inf() : (double)kc;
        part[ISF_W * nchunk + c] = t[0];
        part[ISF_CY * nchunk + c] = cy;
        part[ISF_DY * nchunk + c] = t[1];
        part[ISF_V * nchunk + c] = t[2];
        part[ISF_MY * nchunk + c] = t[3];
        part[ISF_CX * nchunk + c] = cx;
        part[ISF_DX * nchunk + c] = t[4];
        part[ISF_SX * nchunk + c] = t[5];
        part[ISF_MX * nchunk + c] = t[6];
    }
}

// the chunk records of the resident cloud (one row)
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_sum_chunks(IbisView v, int cp, int cs, int ahead, double* part) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    const bool valid = m < v.M;
    const int64_t mm = valid ? m : v.M - 1;
    const double* row = v.raw[cp] + mm * IBIS_NRAW;
    ibis_chunk_record(row[0], row[1], row[2], row[3], v.x[cs][mm], v.S[cs][mm], v.logw[cs][mm], valid, ahead, part, gridDim.x, blockIdx.x);
}

// sum of a [n] from 0.0, left to right, by the calling lane (loads of 8 addends ahead of their additions)
__device__ __forceinline__ double left_to_right_sum(const double* a, int64_t n) {
    double acc = 0.0;
    int64_t c = 0;
    for (; c + 8 <= n; c += 8) {
        double w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = a[c + i];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = acc + w[i];
    }
    for (; c < n; ++c) acc = acc + a[c];
    return acc;
}

// chunk records -> the row of summaries; workgroup r combines row r.  The addends of every chunk are computed by all lanes, the
// sums are taken by one lane each, in chunk order.
__global__ __launch_bounds__(IBIS_SUM_CTHREADS) void k_ibis_sum_combine(double* part_all, int64_t nchunk, double* out /*[rows][IBIS_SUM_NOUT]*/) {
    __shared__ double red[IBIS_SUM_CTHREADS];
    __shared__ double bc[8];
    double* part = part_all + (size_t)blockIdx.x * IBIS_SUM_NCOL * (size_t)nchunk;
    const int tid = threadIdx.x;
    double K = -inf();
    for (int64_t c = tid; c < nchunk; c += IBIS_SUM_CTHREADS) { const double kc = part[ISF_KC * nchunk + c]; K = kc > K ? kc : K; }
    red[tid] = K;
    __syncthreads();
    for (int s = IBIS_SUM_CTHREADS / 2; s > 0; s >>= 1) {      // a maximum: any order
        if (tid < s) red[tid] = red[tid + s] > red[tid] ? red[tid + s] : red[tid];
        __syncthreads();
    }
    K = red[0];
    double* g = part + 10 * nchunk;
    for (int64_t c = tid; c < nchunk; c += IBIS_SUM_CTHREADS) {
        const double W = part[ISF_W * nchunk + c];
        g[c] = ibis_sum_factor(K, part[ISF_KC * nchunk + c], W) * W;
    }
    __syncthreads();
    if (tid == 0) bc[0] = left_to_right_sum(g, nchunk);
    __syncthreads();
    const double D = bc[0];
    for (int64_t c = tid; c < nchunk; c += IBIS_SUM_CTHREADS) {
        double r[IBIS_SUM_NF], a[4];
#pragma unroll
        for (int i = 0; i < IBIS_SUM_NF; ++i) r[i] = part[i * nchunk + c];
        ibis_sum_first(r, ibis_sum_factor(K, r[ISF_KC], r[ISF_W]), D, a);
#pragma unroll
        for (int i = 0; i < 4; ++i) part[(11 + i) * nchunk + c] = a[i];
    }
    __syncthreads();
    if (tid < 4) bc[1 + tid] = left_to_right_sum(part + (11 + tid) * nchunk, nchunk);
    __syncthreads();
    const double y = bc[1], xbar = bc[3];
    for (int64_t c = tid; c < nchunk; c += IBIS_SUM_CTHREADS) {
        double r[IBIS_SUM_NF], b[2];
#pragma unroll
        for (int i = 0; i < IBIS_SUM_NF; ++i) r[i] = part[i * nchunk + c];
        ibis_sum_second(r, ibis_sum_factor(K, r[ISF_KC], r[ISF_W]), D, y, xbar, b);
        part[10 * nchunk + c] = b[0];
        part[15 * nchunk + c] = b[1];
    }
    __syncthreads();
    if (tid < 2) bc[5 + tid] = left_to_right_sum(part + (tid == 0 ? 10 : 15) * nchunk, nchunk);
    __syncthreads();
    if (tid == 0) {
        double* o = out + (size_t)blockIdx.x * IBIS_SUM_NOUT;
        const bool live = D > 0.0;
        const double nan = bits2d(0x7ff8000000000000ULL);
        o[0] = live ? bc[1] : nan;
        o[1] = live ? bc[2] : nan;
        o[2] = live ? bc[5] : nan;
        o[3] = live ? bc[3] : nan;
        o[4] = live ? bc[4] : nan;
        o[5] = live ? bc[6] : nan;
        o[6] = K;
        o[7] = D;
    }
}

// k steps of smc²! (ibis.jl:166-187) from the committed state (set cs), one lane per parameter particle:
//   (x, S) <- kalman_filter(row, x, S, y[j]);  logw += lik;  logZ += lik          (:171-181)
// RECORD: lik [k][M] (optional) and, after every step, the record (kb, S, S2hi, S2lo) of each segment of 8 consecutive
// particles of reweight(logw) (:187) - the integers smc_host_outer_window computes from the same logw, so the host only
// walks k x nseg records.  The end state goes to the set `dst` (== cs: the steps are committed in place).
// predict0: whether the first of the k steps predicts (false only at t = 1 of a sampler with predict_first = 0).
// SUMM: also the chunk record of the summaries after every step (row j of part), from the registers the step left: the
// operands the stand-alone k_ibis_sum_chunks reads back after the same steps, so the same bits.
// MISS (handles with SMC_FLAG_NAN_MISSING, launched only when the window holds a NaN): a NaN y[j] is the missing Kalman step of
// smc_spec.h - y[j] is one address for all lanes, so the test is uniform over the wave.  logw gains +0.0, so the record of
// such a step is the previous step's.  MISS = false is the kernel as it always was.
// SUMM and MISS exist for scalar rows only (a handle of two-state rows refuses summaries and the flag).
template <class Row, bool RECORD, bool SUMM = false, bool MISS = false>
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_window(IbisView v, int cp, int cs, int dst, const double* y, int k, int predict0,
                                                             double* lik /*[k][M] or null*/, uint64_t* rec /*[k][nseg][4]*/,
                                                             double* part /*[k][IBIS_SUM_NCOL][nchunk]*/, int ahead) {
    static_assert(!SUMM || Row::NX == 1, "the summaries of the cloud are those of scalar rows");
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    const bool valid = m < v.M;
    const int64_t mm = valid ? m : v.M - 1;            // lanes beyond the cloud compute on the last particle and store nothing
    double r[Row::NSTEP], x[Row::NX], S[Row::NS];
#pragma unroll
    for (int i = 0; i < Row::NSTEP; ++i) r[i] = v.raw[cp][mm * Row::NRAW + i];
    ibis_load_state<Row>(v, cs, mm, x, S);
    double logZ = v.logZ[cs][mm], logw = v.logw[cs][mm];
    const int64_t nseg = (v.M + IBIS_OSEG - 1) / IBIS_OSEG;
    for (int j = 0; j < k; ++j) {
        const double l = Row::template step<MISS>(r, j > 0 || predict0 != 0, y[j], x, S);
        logw = logw + l;
        logZ = logZ + l;
        if (RECORD) {
            if (lik && valid) lik[(size_t)j * (size_t)v.M + (size_t)m] = l;
            ibis_outer_record(logw, valid, m, rec + (size_t)j * (size_t)nseg * 4);
        }
        if constexpr (SUMM)
            ibis_chunk_record(r[0], r[1], r[2], r[3], x[0], S[0], logw, valid, ahead, part + (size_t)j * IBIS_SUM_NCOL * (size_t)gridDim.x,
                              gridDim.x, blockIdx.x);
    }
    if (valid) {
        ibis_store_state<Row>(v, dst, m, x, S);
        v.logZ[dst][m] = logZ;
        v.logw[dst][m] = logw;
    }
}

// rejuvenate!(ibis, y, xi) (ibis.jl:86-125) in one launch, one lane per parameter particle m:
//   for c in 1:chain                                                                  :96
//       theta' = rand(kernel(theta[m], scales[c]))       pmmh_propose                 :97
//       if insupport(prior, theta')                      (a lane outside is predicated off for this c)   :99
//           x', S', logZ' = log_likelihood(y, model(theta'))   the Kalman filter over y[0:T) in registers  :100
//           accept iff logZ' + logprior(theta') > -inf and log(rand()) < xi (logZ' - logZ) + logprior(theta') - logprior(theta)
//           then theta, logZ, x, S <- theta', logZ', x', S'; acc_array[m] = 1          :102-115
//   omega[m] = 1                                          logw[m] = 0                  :118
// y[t] is the same address in every lane (the compiler reads it through the scalar cache); chol [D][D] and sq [chain] likewise.
// Row::SKIP_IDLE_WAVE (two-state rows): a wave none of whose lanes proposed inside the support leaves the re-filter of that
// chain position out: the ballot is uniform over the wave, and a lane outside the support never accepts, so what its filter
// would have returned is not read.  The results are the same with and without; scalar rows measured slower with it.
// MISS: as in k_ibis_window - the re-filter skips the update at a NaN y[t], the same steps the online logZ took.
template <class Row, int D, bool MISS = false>
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_rejuvenate(IbisView v, int cp, int cs, PmmhSpec s, IbisRowMap map, const double* y,
                                                                 int64_t T, int predict_first, double xi, const double* chol,
                                                                 const double* sq, int chain, uint64_t move_seed, unsigned char* moved,
                                                                 unsigned long long* n_moved) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    const bool valid = m < v.M;
    const int64_t mm = valid ? m : v.M - 1;
    const uint32_t stream = (uint32_t)mm;
    double th[D], row[Row::NRAW], x[Row::NX], S[Row::NS];
#pragma unroll
    for (int i = 0; i < D; ++i) th[i] = v.theta[cp][mm * MAX_DTHETA + i];
#pragma unroll
    for (int k = 0; k < Row::NRAW; ++k) row[k] = v.raw[cp][mm * Row::NRAW + k];
    ibis_load_state<Row>(v, cs, mm, x, S);
    double logZ = v.logZ[cs][mm];
    bool any = false;
    for (int c = 0; c < chain; ++c) {
        double pr[D], prow[Row::NRAW], xp[Row::NX], Sp[Row::NS];
        pmmh_propose<D>(s, move_seed, stream, (uint32_t)c, th, chol, sq[c], pr);
        const bool ok = pmmh_insupport<D>(s, pr);
        ibis_row<Row, D>(map, pr, prow);
        const double lpp = pmmh_logprior<D>(s, pr), lpc = pmmh_logprior<D>(s, th);
#pragma unroll
        for (int i = 0; i < Row::NX; ++i) xp[i] = prow[Row::X0 + i];
#pragma unroll
        for (int i = 0; i < Row::NS; ++i) Sp[i] = prow[Row::S0 + i];
        double logZp = 0.0;
        if (!Row::SKIP_IDLE_WAVE || __ballot(ok) != 0)
            for (int64_t t = 0; t < T; ++t) logZp += Row::template step<MISS>(prow, predict_first != 0 || t > 0, y[t], xp, Sp);
        const double likelihood_ratio = xi * (logZp - logZ), prior_ratio = lpp - lpc;
        const double acc_ratio = likelihood_ratio + prior_ratio, log_post_prop = logZp + lpp;
        const bool acc = ok && log_post_prop > -inf() && pmmh_log_uniform(move_seed, stream, (uint32_t)c) < acc_ratio;
#pragma unroll
        for (int i = 0; i < D; ++i) th[i] = acc ? pr[i] : th[i];
#pragma unroll
        for (int k = 0; k < Row::NRAW; ++k) row[k] = acc ? prow[k] : row[k];
        logZ = acc ? logZp : logZ;
#pragma unroll
        for (int i = 0; i < Row::NX; ++i) x[i] = acc ? xp[i] : x[i];
#pragma unroll
        for (int i = 0; i < Row::NS; ++i) S[i] = acc ? Sp[i] : S[i];
        any = any || acc;
    }
    any = any && valid;
    if (valid) {
#pragma unroll
        for (int i = 0; i < D; ++i) v.theta[cp][m * MAX_DTHETA + i] = th[i];
#pragma unroll
        for (int k = 0; k < Row::NRAW; ++k) v.raw[cp][m * Row::NRAW + k] = row[k];
        ibis_store_state<Row>(v, cs, m, x, S);
        v.logZ[cs][m] = logZ;
        v.logw[cs][m] = 0.0;
        moved[m] = any ? 1 : 0;
    }
    const unsigned long long cnt = (unsigned long long)__popcll(__ballot(any));   // one integer add per wave: order-free
    if (threadIdx.x == 0 && cnt) atomicAdd(n_moved, cnt);
}

// resample!(ibis) (ibis.jl:73-84): particle m <- particle a[m], a value copy of everything it owns, into the other buffers
template <class Row>
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_permute(IbisView v, int cp, int cs, const int32_t* a) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    if (m >= v.M) return;
    const int64_t src = a[m];
#pragma unroll
    for (int i = 0; i < MAX_DTHETA; ++i) v.theta[cp ^ 1][m * MAX_DTHETA + i] = v.theta[cp][src * MAX_DTHETA + i];
#pragma unroll
    for (int k = 0; k < Row::NRAW; ++k) v.raw[cp ^ 1][m * Row::NRAW + k] = v.raw[cp][src * Row::NRAW + k];
    ibis_store_state<Row>(v, cs ^ 1, m, v.x[cs] + src * Row::NX, v.S[cs] + src * Row::NS);
    v.logZ[cs ^ 1][m] = v.logZ[cs][src];
    v.logw[cs ^ 1][m] = v.logw[cs][src];
}

// ---- the resample-move loop without a read of the cloud (IBIS(..., device_moves=True)) ---------------------------------------
// Everything here is a reduction, a scan or a search over the cloud in INTEGER arithmetic (any order gives the same bits), or the
// chunk / tree / left-to-right sums of smc_spec.h "moments of the theta cloud".  No float atomics.
constexpr int IBIS_RED_THREADS = 256;
constexpr uint32_t IBIS_KBIAS = 1u << 30;   // an exponent k, |k| < 2^30, travels as the unsigned k + 2^30 >= 1; 0: no live entry

SMC_HD uint32_t ibis_bias_k(int k) { return k == IBIS_SUM_DEADK ? 0u : (uint32_t)k + IBIS_KBIAS; }
SMC_HD int ibis_unbias_ki(uint32_t kb) { return kb ? (int)(kb - IBIS_KBIAS) : IBIS_SUM_DEADK; }
SMC_HD double ibis_unbias_k(uint32_t kb) { return kb ? (double)(int)(kb - IBIS_KBIAS) : -inf(); }

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, s, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, s, 64); v = o > v ? o : v; }
    return v;
}

// K = max kb of every step's records (smc_outer.hip combine()); rec [k][nseg][4], Kb [k] zeroed by the caller.  grid (x, k)
__global__ __launch_bounds__(IBIS_RED_THREADS) void k_ibis_rec_kmax(const uint64_t* rec, int64_t nseg, uint32_t* Kb) {
    const uint64_t* r = rec + (size_t)blockIdx.y * (size_t)nseg * 4;
    uint32_t v = 0;
    for (int64_t b = (int64_t)blockIdx.x * IBIS_RED_THREADS + threadIdx.x; b < nseg; b += (int64_t)gridDim.x * IBIS_RED_THREADS) {
        const double kb = bits2d(r[b * 4]);
        const uint32_t o = kb > -inf() ? ibis_bias_k((int)kb) : 0u;
        v = o > v ? o : v;
    }
    v = wave_max_u32(v);
    if ((threadIdx.x & 63) == 0 && v) atomicMax(&Kb[blockIdx.y], v);
}
// D = sum seg_Q(S_b, sh_b), R = sum seg_R(hi_b, lo_b, sh_b, SH) of every step; DR [k][2] zeroed by the caller
__global__ __launch_bounds__(IBIS_RED_THREADS) void k_ibis_rec_sums(const uint64_t* rec, int64_t nseg, int SH, const uint32_t* Kb,
                                                                   unsigned long long* DR) {
    const uint64_t* r = rec + (size_t)blockIdx.y * (size_t)nseg * 4;
    const double K = ibis_unbias_k(Kb[blockIdx.y]);
    uint64_t D = 0, R = 0;
    for (int64_t b = (int64_t)blockIdx.x * IBIS_RED_THREADS + threadIdx.x; b < nseg; b += (int64_t)gridDim.x * IBIS_RED_THREADS) {
        const int sh = seg_shift(K, bits2d(r[b * 4]), SH);
        D += seg_Q(r[b * 4 + 1], sh);
        R += seg_R(r[b * 4 + 2], r[b * 4 + 3], sh, SH);
    }
    D = wave_sum_u64(D);
    R = wave_sum_u64(R);
    if ((threadIdx.x & 63) == 0) {
        if (D) atomicAdd(&DR[2 * blockIdx.y], (unsigned long long)D);
        if (R) atomicAdd(&DR[2 * blockIdx.y + 1], (unsigned long long)R);
    }
}

// resample!(ibis), step 1 (smc_host_outer_resample): the fixed-point weight q of every particle of the committed logw, the
// (kb, S) of every segment of 8, and the cloud's K (Kb zeroed by the caller)
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_rs_weights(IbisView v, int cs, uint64_t* q, uint32_t* skb, uint64_t* sS, uint32_t* Kb) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    const bool valid = m < v.M;
    const int64_t mm = valid ? m : v.M - 1;
    const double logw = v.logw[cs][mm];
    const bool alive = valid && lw_alive(logw);
    double kd = 0.0;
    const double p = sp_exp_parts(alive ? logw : 0.0, kd);
    const int ki = alive ? (int)kd : IBIS_SUM_DEADK;
    const int kb = seg8_max(ki);
    const uint64_t qi = alive ? fix_weight_i(p, ki - kb, FIX_BITS) : 0;
    const uint64_t Ssum = seg8_sum(qi);
    if (valid) q[m] = qi;
    if (valid && (threadIdx.x & (IBIS_OSEG - 1)) == 0) {
        skb[m / IBIS_OSEG] = ibis_bias_k(kb);
        sS[m / IBIS_OSEG] = kb == IBIS_SUM_DEADK ? 0 : Ssum;
    }
    const uint32_t K = wave_max_u32(ibis_bias_k(kb));
    if (threadIdx.x == 0 && K) atomicMax(Kb, K);
}

// the addends of the two scans: seg_Q(S_b, sh_b) of segment b, and the number of draws that fell on particle i
struct IbisSegQ {
    const uint32_t* skb; const uint64_t* sS; const uint32_t* Kb; int SH;
    __device__ __forceinline__ uint64_t operator()(int64_t b) const { return seg_Q(sS[b], seg_shift(ibis_unbias_k(*Kb), ibis_unbias_k(skb[b]), SH)); }
};
struct IbisCount {
    const int32_t* cnt;
    __device__ __forceinline__ uint64_t operator()(int64_t i) const { return (uint64_t)cnt[i]; }
};

// inclusive scan over the workgroup (IBIS_RED_THREADS lanes); total: the sum of all of them.  Integers: the order is free.
__device__ __forceinline__ uint64_t block_scan_u64(uint64_t v, uint64_t* wsum /*[IBIS_RED_THREADS / 64] in LDS*/, uint64_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((unsigned long long)v, s, 64);
        v += lane >= s ? o : 0;
    }
    __syncthreads();                    // (a caller in a loop: the sums of the last round have been read)
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    uint64_t off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < IBIS_RED_THREADS / 64; ++i) { off += i < w ? wsum[i] : 0; tot += wsum[i]; }
    total = tot;
    return v + off;
}
// reduce-then-scan of f(0..n): tile sums, their exclusive scan by one workgroup, then the scan of every tile on top of its offset
template <class F>
__global__ __launch_bounds__(IBIS_RED_THREADS) void k_ibis_scan_sums(F f, int64_t n, uint64_t* tsum) {
    __shared__ uint64_t wsum[IBIS_RED_THREADS / 64];
    const int64_t i = (int64_t)blockIdx.x * IBIS_RED_THREADS + threadIdx.x;
    uint64_t total;
    block_scan_u64(i < n ? f(i) : 0, wsum, total);
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}
__global__ __launch_bounds__(IBIS_RED_THREADS) void k_ibis_scan_offsets(uint64_t* tsum, int64_t ntile) {
    __shared__ uint64_t wsum[IBIS_RED_THREADS / 64];
    uint64_t carry = 0;
    for (int64_t base = 0; base < ntile; base += IBIS_RED_THREADS) {
        const int64_t i = base + threadIdx.x;
        const uint64_t v = i < ntile ? tsum[i] : 0;
        uint64_t total;
        const uint64_t incl = block_scan_u64(v, wsum, total);
        if (i < ntile) tsum[i] = carry + incl - v;
        carry += total;
    }
}
template <class F>
__global__ __launch_bounds__(IBIS_RED_THREADS) void k_ibis_scan_tiles(F f, int64_t n, const uint64_t* tsum, uint64_t* out) {
    __shared__ uint64_t wsum[IBIS_RED_THREADS / 64];
    const int64_t i = (int64_t)blockIdx.x * IBIS_RED_THREADS + threadIdx.x;
    uint64_t total;
    const uint64_t incl = block_scan_u64(i < n ? f(i) : 0, wsum, total);
    if (i < n) out[i] = tsum[blockIdx.x] + incl;
}

// first index with c[i] > T in the non-decreasing c [n]; the caller guarantees T < c[n - 1], so the result is in [0, n)
__device__ __forceinline__ int64_t first_greater(const uint64_t* c, int64_t n, uint64_t T) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (c[mid] > T) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// step 5: lane p takes the draws 2p and 2p + 1 (the two 64-bit halves of one Philox call); cnt [M] zeroed by the caller.
// Dtot = 0 (no live particle): every particle is drawn once, the identity.
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_rs_draw(int64_t M, uint64_t seed, const uint64_t* q, const uint32_t* skb,
                                                              const uint32_t* Kb, int SH, const uint64_t* Dcum, int64_t nseg, int32_t* cnt) {
    const int64_t pr = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x, j0 = 2 * pr;
    if (j0 >= M) return;
    const uint64_t Dtot = Dcum[nseg - 1];
    if (Dtot == 0) {
        cnt[j0] = 1;
        if (j0 + 1 < M) cnt[j0 + 1] = 1;
        return;
    }
    const double K = ibis_unbias_k(*Kb);
    const u32x4 w = draw(seed, (uint32_t)pr, OUTER_STREAM, 0u, SLOT_OUTER);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (j0 + h >= M) break;
        const uint64_t pick = ((uint64_t)w.v[2 * h + 1] << 32) | w.v[2 * h];
        uint64_t T, lo;
        mul64wide(pick, Dtot, T, lo);
        const int64_t b = first_greater(Dcum, nseg, T);                       // T < Dtot = Dcum[nseg - 1]
        const uint64_t thr = sys_threshold(T - (b ? Dcum[b - 1] : 0), seg_shift(K, ibis_unbias_k(skb[b]), SH));
        const int64_t i0 = b * IBIS_OSEG;
        const int cn = (int)(M - i0 < IBIS_OSEG ? M - i0 : IBIS_OSEG);
        uint64_t C = 0;
        int i = 0;
#pragma unroll
        for (int t = 0; t < IBIS_OSEG; ++t)
            if (t < cn) { C += q[i0 + t]; i += C <= thr ? 1 : 0; }
        atomicAdd(&cnt[i0 + (i < cn ? i : cn - 1)], 1);
    }
}
// step 6: a = the expansion of cnt in index order; cincl [M] the inclusive scan of cnt (cincl[M - 1] = M)
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_rs_expand(int64_t M, const uint64_t* cincl, int32_t* a) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    if (m >= M) return;
    a[m] = (int32_t)first_greater(cincl, M, (uint64_t)m);
}

// ---- moments of the theta cloud (smc_spec.h) -----------------------------------------------------------------------------------
// mom: [0] W | [1 .. 8] mean | [9 .. 9 + 36) cov, lower triangle row by row.  part: [column][nchunk].  One wave per chunk.
constexpr int IBIS_MOM_MEAN = 1, IBIS_MOM_COV = 1 + MAX_DTHETA, IBIS_MOM_N = 1 + MAX_DTHETA + THETA_MOM_NTRI;

// any grid of workgroups of whole waves: the particles are strided over it, every workgroup publishes its maximum (an integer: any order)
__global__ __launch_bounds__(IBIS_RED_THREADS) void k_ibis_kmax(IbisView v, int cs, uint32_t* Kb) {
    uint32_t K = 0;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < v.M; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = base + threadIdx.x;
        const bool valid = m < v.M;
        int k;
        (void)ibis_sum_parts(v.logw[cs][valid ? m : v.M - 1], valid, k);
        const uint32_t kb = ibis_bias_k(k);
        K = kb > K ? kb : K;
    }
    // one atomic per workgroup: thousands of them on one word are served one after the other (~12 ns each)
    __shared__ uint32_t wg;
    if (threadIdx.x == 0) wg = 0;
    __syncthreads();
    K = wave_max_u32(K);
    if ((threadIdx.x & 63) == 0 && K) atomicMax(&wg, K);
    __syncthreads();
    if (threadIdx.x == 0 && wg) atomicMax(Kb, wg);
}
// u of the calling lane (weighted mode)
__device__ __forceinline__ double ibis_mom_u(const IbisView& v, int cs, int64_t mm, bool valid, const uint32_t* Kb) {
    int k;
    const double p = ibis_sum_parts(v.logw[cs][mm], valid, k);
    return theta_mom_u(p, k, ibis_unbias_ki(*Kb));
}
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_mom_w(IbisView v, int cs, const uint32_t* Kb, double* part) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x;
    const bool valid = m < v.M;
    const double t = wave_tree_sum(ibis_mom_u(v, cs, valid ? m : v.M - 1, valid, Kb));
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}
// PASS 1: the sums of c theta_i; PASS 2: the sums of c (d_i d_j), j <= i, about the means in mom
template <int D, int PASS>
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_mom_chunks(IbisView v, int cp, int cs, int weighted, const uint32_t* Kb, const double* mom,
                                                                 double* part) {
    const int64_t m = (int64_t)blockIdx.x * IBIS_THREADS + threadIdx.x, nchunk = gridDim.x;
    const bool valid = m < v.M;
    const int64_t mm = valid ? m : v.M - 1;
    double c = valid ? 1.0 : 0.0;
    if (weighted) {
        const double u = ibis_mom_u(v, cs, mm, valid, Kb);
        c = u > 0.0 ? u / mom[0] : 0.0;
    }
    const bool on = c > 0.0;
    double th[D];
#pragma unroll
    for (int i = 0; i < D; ++i) th[i] = v.theta[cp][mm * MAX_DTHETA + i];
    if (PASS == 1) {
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double t = wave_tree_sum(theta_mom_term(on, c, th[i]));
            if (threadIdx.x == 0) part[i * nchunk + blockIdx.x] = t;
        }
    } else {
#pragma unroll
        for (int i = 0; i < D; ++i) th[i] = th[i] - mom[IBIS_MOM_MEAN + i];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                const double t = wave_tree_sum(theta_mom_term(on, c, th[i] * th[j]));
                if (threadIdx.x == 0) part[(i * (i + 1) / 2 + j) * nchunk + blockIdx.x] = t;
            }
    }
}
// lane t sums column t of part over the chunks, left to right, and finishes it (theta_mom_finish) into out[t]
__global__ __launch_bounds__(IBIS_THREADS) void k_ibis_mom_combine(const double* part, int ncol, int64_t nchunk, double* out, int div_on, double div,
                                                                  int weighted, const double* W) {
    const int t = threadIdx.x;
    if (t >= ncol) return;
    const double s = left_to_right_sum(part + (size_t)t * (size_t)nchunk, nchunk);
    out[t] = theta_mom_finish(s, div_on != 0, div, weighted != 0, weighted ? *W : 1.0);
}

}  // namespace smc
