// smc_pred_kernels.h -- predictive checks (smc_spec.h "predictive checks"): the PIT and the one-step forecast
// moments of the clouds of bootstrap filters, and the exact Kalman rows.  wave64, f64, read-only on the clouds.
//
// Every kernel here is a template, so the header may be included where its kernels are launched: k_predictive and its finishing
// kernels in smc_capi_summ.hip (enqueue_predictive: smc_get_predictive, and smc_predictive of smc_capi_smooth.hip through it),
// k_kalman_predictive and k_normcdf in smc_util.hip.
//
// A cloud is read through three strides (in doubles): element (step t, state row c, filter th, particle i) is
// x[t * st_t + c * st_c + th * st_f + i].  The dense record [T][d][n_theta][n] and the padded state [d][n_theta][npad] run the
// same code.  One lane per particle: consecutive lanes read consecutive doubles of the rows the family reads (pred_rows).
//
// Order of the sums (pred_sum): a tile is PRED_THREADS consecutive particles = PRED_TILE_CH chunks of SMOOTH_CH.  Every lane puts
// its terms into an LDS tile; lane (q, c) of the first 3 * PRED_TILE_CH then adds the SMOOTH_CH terms of chunk c of quantity q in
// ascending order from +0.0.  The tile's rows are padded by one double: with a stride of SMOOTH_CH doubles all the chunk readers
// would sit on one bank; with SMOOTH_CH + 1, reader c starts two banks after reader c - 1, and at SMOOTH_CH = 128 the planes of the
// three quantities are 16 banks apart (8 * 129 * 2 mod 64), so the 24 readers never collide.
//   small clouds (the host's switch, smc_capi_summ.hip: 4096 by measurement; at most PRED_SMALL_MAX = SMOOTH_CH^2, what the LDS
//       partials hold): k_predictive, ONE workgroup per (step, filter), grid (T, n_theta): the chunk partials stay in LDS, lane q
//       adds them (level 1), the centred pass re-reads the cloud (it is in L2), lane 0 writes the row.
//   large clouds: k_predictive_tiles<PASS 0> over (tile, step, filter) writes the level-0 partials of the three first-pass sums,
//       k_pred_level sums SMOOTH_CH consecutive partials per lane, once per level, until one is left; k_predictive_tiles<PASS 1>
//       forms the mean from those sums and writes the partials of the centred terms; levels again; k_pred_finish writes the rows.
// No float atomics, no spinning: whoever adds, adds in the order of the specification.
#pragma once
#include "smc_kalman_rows.h"
#include "smc_spec.h"

namespace smc {

constexpr int PRED_THREADS = 1024;
constexpr int PRED_TILE_CH = PRED_THREADS / SMOOTH_CH;
constexpr int PRED_STRIDE = SMOOTH_CH + 1;
constexpr int PRED_PLANE = PRED_TILE_CH * PRED_STRIDE;
constexpr int64_t PRED_SMALL_MAX = (int64_t)SMOOTH_CH * SMOOTH_CH;   // the most one workgroup finishes: one level above the chunks
static_assert(PRED_THREADS % SMOOTH_CH == 0, "a tile is a whole number of chunks");

struct PredArgs {
    const double* x;            // the clouds
    int64_t st_t, st_c, st_f;   // strides in doubles: step, state row, filter
    int64_t n;                  // particles per filter
    int ntheta;
    int64_t ntiles;             // tiles per cloud (k_predictive_tiles: the grid is ntiles * T * ntheta workgroups)
    const Params* params;       // [ntheta]
    const double* y;            // [T] on the device, or nullptr: y0 for every step (smc_get_predictive)
    double y0;
    double* part;               // k_predictive_tiles: level-0 partials [planes][T * ntheta][nch], nch = ceil(n / SMOOTH_CH)
    const double* sums;         // k_predictive_tiles<1>, k_pred_finish: the finished first-pass sums [3][T * ntheta]
    const double* sum_c;        // k_pred_finish: the finished centred sums [T * ntheta]
    double* out;                // pit | obs_mean | obs_var, [T * ntheta] each
};

// one tile of one cloud: the terms of pass PASS (0: Phi(z), ym, sd^2;  1: (ym - mean)^2) into the LDS tile, then the chunk sums into
// dst[q * dst_plane + (chunk index within the cloud)].  xf: the cloud's row 0, base: the tile's first particle.  Two barriers.
template <int MODEL, int PASS>
__device__ __forceinline__ void pred_tile(const PredArgs& a, const Params& prm, const double* xf, double y, double mean, int64_t base, double* tile,
                                          double* dst, int64_t dst_plane) {
    constexpr int NQ = PASS == 0 ? 3 : 1;
    const int tid = (int)threadIdx.x;
    const int64_t i = base + tid;
    if (i < a.n) {
        double x[3] = {xf[i], 0.0, 0.0};
        if constexpr (pred_rows<MODEL>::count == 2) x[pred_rows<MODEL>::second] = xf[(int64_t)pred_rows<MODEL>::second * a.st_c + i];
        const int slot = (tid / SMOOTH_CH) * PRED_STRIDE + tid % SMOOTH_CH;
        if constexpr (PASS == 0) {
            double cdf, ym, s2;
            pred_terms<MODEL>(prm, x, y, cdf, ym, s2);
            tile[slot] = cdf;
            tile[PRED_PLANE + slot] = ym;
            tile[2 * PRED_PLANE + slot] = s2;
        } else {
            double ym, sd;
            model_obs_moments<MODEL>(prm, x, ym, sd);
            tile[slot] = pred_centred_term(ym, mean);
        }
    }
    __syncthreads();
    if (tid < NQ * PRED_TILE_CH) {
        const int q = tid / PRED_TILE_CH, c = tid % PRED_TILE_CH;
        const int64_t c0 = base + (int64_t)c * SMOOTH_CH;
        if (c0 < a.n) {
            const int len = a.n - c0 < SMOOTH_CH ? (int)(a.n - c0) : SMOOTH_CH;
            const double* src = tile + q * PRED_PLANE + c * PRED_STRIDE;
            double s = 0.0;
            for (int k = 0; k < len; ++k) s += src[k];
            dst[(int64_t)q * dst_plane + c0 / SMOOTH_CH] = s;
        }
    }
    __syncthreads();
}

// SMOOTH_CH-or-fewer partials to one number, as a level of pred_sum does (one partial: that partial)
__device__ __forceinline__ double pred_level_one(const double* p, int m) {
    if (m == 1) return p[0];
    double s = 0.0;
    for (int j = 0; j < m; ++j) s += p[j];
    return s;
}

// small clouds: one workgroup per (step, filter)
template <int MODEL>
__global__ __launch_bounds__(PRED_THREADS) void k_predictive(PredArgs a) {
    __shared__ double tile[3 * PRED_PLANE];
    __shared__ double part[3 * SMOOTH_CH];
    __shared__ double res[3];
    if (a.n > PRED_SMALL_MAX) return;   // (never launched so: `part` holds SMOOTH_CH chunk partials a quantity)
    const int64_t t = blockIdx.x;
    const int th = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int64_t row = t * a.ntheta + th, rows = (int64_t)gridDim.x * a.ntheta;
    const Params prm = a.params[th];
    const double y = a.y ? a.y[t] : a.y0;
    const double* xf = a.x + t * a.st_t + (int64_t)th * a.st_f;
    const int nch = (int)((a.n + SMOOTH_CH - 1) / SMOOTH_CH);   // <= SMOOTH_CH (the host's choice of kernel)
    for (int64_t base = 0; base < a.n; base += PRED_THREADS) pred_tile<MODEL, 0>(a, prm, xf, y, 0.0, base, tile, part, SMOOTH_CH);
    if (tid < 3) res[tid] = pred_level_one(part + tid * SMOOTH_CH, nch);
    __syncthreads();
    const double mean = pred_mean_of(res[1], a.n);
    for (int64_t base = 0; base < a.n; base += PRED_THREADS) pred_tile<MODEL, 1>(a, prm, xf, y, mean, base, tile, part, SMOOTH_CH);
    if (tid == 0) {
        a.out[row] = pred_mean_of(res[0], a.n);
        a.out[rows + row] = mean;
        a.out[2 * rows + row] = pred_var_of(res[2], pred_level_one(part, nch), a.n);
    }
}

// large clouds: one workgroup per (tile, step, filter), blockIdx.x = (t * ntheta + th) * ntiles + tile
template <int MODEL, int PASS>
__global__ __launch_bounds__(PRED_THREADS) void k_predictive_tiles(PredArgs a, int64_t rows) {
    __shared__ double tile[(PASS == 0 ? 3 : 1) * PRED_PLANE];
    const int64_t row = blockIdx.x / a.ntiles, tl = blockIdx.x % a.ntiles;
    const int64_t t = row / a.ntheta;
    const int th = (int)(row % a.ntheta);
    const Params prm = a.params[th];
    const double y = a.y ? a.y[t] : a.y0;
    const double* xf = a.x + t * a.st_t + (int64_t)th * a.st_f;
    const int64_t nch = (a.n + SMOOTH_CH - 1) / SMOOTH_CH;
    const double mean = PASS == 1 ? pred_mean_of(a.sums[rows + row], a.n) : 0.0;
    pred_tile<MODEL, PASS>(a, prm, xf, y, mean, tl * PRED_THREADS, tile, a.part + row * nch, rows * nch);
}

// one level of pred_sum over `lines` independent lines: in [lines][m_in] -> out [lines][m_out], m_out = ceil(m_in / CH); one lane per
// number written
template <int CH = SMOOTH_CH>
__global__ __launch_bounds__(256) void k_pred_level(const double* in, int64_t m_in, double* out, int64_t m_out, int64_t lines) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= lines * m_out) return;
    const int64_t r = id / m_out, j = id % m_out;
    const int64_t c0 = j * CH, c1 = c0 + CH < m_in ? c0 + CH : m_in;
    const double* p = in + r * m_in;
    double s = 0.0;
    for (int64_t i = c0; i < c1; ++i) s += p[i];
    out[id] = s;
}

// the rows from their finished sums
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_pred_finish(PredArgs a, int64_t rows) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    a.out[row] = pred_mean_of(a.sums[row], a.n);
    a.out[rows + row] = pred_mean_of(a.sums[rows + row], a.n);
    a.out[2 * rows + row] = pred_var_of(a.sums[2 * rows + row], a.sum_c[row], a.n);
}

// sp_normcdf on the device, one lane per value (smc_device_normcdf: the test of "the device value equals the host value")
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_normcdf(const double* z, int64_t n, double* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = sp_normcdf(z[i]);
}

// The exact Kalman rows of a whole series, batched over parameter rows, one lane per row: the loop of k_kalman_loglik writing
// pit, ym, yv [T][n] (any nullptr: not written; consecutive lanes write consecutive doubles).  MISS as there.
template <class Row, bool MISS = false>
__global__ __launch_bounds__(KALMAN_THREADS) void k_kalman_predictive(const double* raw /*[n][NRAW]*/, int64_t n, const double* y, int64_t T,
                                                                     int predict_first, double* pit, double* ym, double* yv) {
    static_assert(Row::NX == 1 && Row::NS == 1, "scalar rows");
    const int64_t m = (int64_t)blockIdx.x * KALMAN_THREADS + threadIdx.x;
    if (m >= n) return;
    double r[Row::NRAW];
#pragma unroll
    for (int k = 0; k < Row::NRAW; ++k) r[k] = raw[m * Row::NRAW + k];
    double x = r[Row::X0], S = r[Row::S0];
    for (int64_t t = 0; t < T; ++t) {
        double p, mu, v;
        kalman_predictive_step<MISS>(r[0], r[1], r[2], r[3], predict_first != 0 || t > 0, y[t], x, S, p, mu, v);
        if (pit) pit[t * n + m] = p;
        if (ym) ym[t * n + m] = mu;
        if (yv) yv[t * n + m] = v;
    }
}

}  // namespace smc
