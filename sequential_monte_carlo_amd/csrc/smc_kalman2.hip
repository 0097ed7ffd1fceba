// smc_kalman2.hip -- C ABI of the two-state exact Kalman side (include/smc_hip.h "two-state linear models"): the batched filter
// and RTS smoother on the device (smc_kalman2_kernels.h), their host twins, and the simulation of such a row.
#include "smc_host.h"
#include "smc_kalman2_kernels.h"

#include <string>
#include <vector>

using namespace smc;

namespace {
constexpr int64_t K2_MAX_N = (int64_t)1 << 30, K2_MAX_T = (int64_t)1 << 31;
unsigned k2_grid(int64_t n) { return (unsigned)((n + KALMAN_THREADS - 1) / KALMAN_THREADS); }
// the sizes every device call of this file accepts
bool k2_sizes_ok(int64_t n, int64_t T) { return n >= 1 && n <= K2_MAX_N && T >= 1 && T <= K2_MAX_T; }
}  // namespace

// Both device calls own their memory for the call (DeviceCall::use_own: counted while it runs, freed when it returns)
extern "C" int smc_kalman2_log_likelihood(const double* raw, int64_t n, const double* y, int64_t T, int predict_first, double* out, int device) {
    if (!raw || !y || !out) return fail(SMC_EINVAL, "smc_kalman2_log_likelihood: bad argument");
    if (!k2_sizes_ok(n, T)) return fail(SMC_EINVAL, "smc_kalman2_log_likelihood: 1 <= n <= 2^30, 1 <= T <= 2^31");
    DeviceCall c;
    if (const int rc = c.begin("smc_kalman2_log_likelihood", device)) return rc;
    const size_t b_y = (size_t)T * 8, b_raw = (size_t)n * LG2_NRAW * 8, b_out = (size_t)n * 6 * 8;
    const size_t o_y = c.take(b_y), o_raw = c.take(b_raw), o_out = c.take(b_out);
    if (const int rc = c.use_own()) return rc;
    HIPCHK(c.upload(o_y, y, b_y));
    HIPCHK(c.upload(o_raw, raw, b_raw));
    hipLaunchKernelGGL((k_kalman_loglik<Lg2Row>), dim3(k2_grid(n)), dim3(KALMAN_THREADS), 0, c.stream, c.at<const double>(o_raw), n,
                       c.at<const double>(o_y), T, predict_first ? 1 : 0, c.at<double>(o_out));
    HIPCHK(hipGetLastError());
    HIPCHK(c.download(out, o_out, b_out));
    HIPCHK(c.finish());
    return SMC_OK;
}

extern "C" int smc_kalman2_smooth(const double* raw, int64_t n, const double* y, int64_t T, int predict_first, double* xs, double* Ps, int device) {
    if (!raw || !y || !xs || !Ps) return fail(SMC_EINVAL, "smc_kalman2_smooth: bad argument");
    if (!k2_sizes_ok(n, T)) return fail(SMC_EINVAL, "smc_kalman2_smooth: 1 <= n <= 2^30, 1 <= T <= 2^31");
    DeviceCall c;
    if (const int rc = c.begin("smc_kalman2_smooth", device)) return rc;
    const size_t b_y = (size_t)T * 8, b_raw = (size_t)n * LG2_NRAW * 8, b_xs = (size_t)T * n * 2 * 8, b_Ps = (size_t)T * n * 3 * 8;
    const size_t o_y = c.take(b_y), o_raw = c.take(b_raw), o_xs = c.take(b_xs), o_Ps = c.take(b_Ps);
    if (const int rc = c.use_own()) return rc;
    HIPCHK(c.upload(o_y, y, b_y));
    HIPCHK(c.upload(o_raw, raw, b_raw));
    hipLaunchKernelGGL(k_kalman2_smooth, dim3(k2_grid(n)), dim3(KALMAN_THREADS), 0, c.stream, c.at<const double>(o_raw), n, c.at<const double>(o_y), T,
                       predict_first ? 1 : 0, c.at<double>(o_xs), c.at<double>(o_Ps));
    HIPCHK(hipGetLastError());
    HIPCHK(c.download(xs, o_xs, b_xs));
    HIPCHK(c.download(Ps, o_Ps, b_Ps));
    HIPCHK(c.finish());
    return SMC_OK;
}

// The step loop of ONE row on the host (no GPU): the filtered record and the value of every step.  Every device array of the
// two-state calls has the bits of a composition of this call.
extern "C" int smc_host_kalman2_steps(const double* row, const double* y, int64_t T, int predict_first, double* xf, double* Sf, double* lik) {
    if (!row || !y || T < 1) return fail(SMC_EINVAL, "smc_host_kalman2_steps: bad argument");
    double x1 = row[LG2_X1], x2 = row[LG2_X2], S11 = row[LG2_S11], S21 = row[LG2_S21], S22 = row[LG2_S22];
    for (int64_t t = 0; t < T; ++t) {
        const double l = kalman2_step(row, t > 0 || predict_first != 0, y[t], x1, x2, S11, S21, S22);
        if (xf) { xf[2 * t] = x1; xf[2 * t + 1] = x2; }
        if (Sf) { Sf[3 * t] = S11; Sf[3 * t + 1] = S21; Sf[3 * t + 2] = S22; }
        if (lik) lik[t] = l;
    }
    return SMC_OK;
}

// The backward walk of ONE row on the host: the filter's record, then rts2_step from the last period down
extern "C" int smc_host_kalman2_smooth(const double* row, const double* y, int64_t T, int predict_first, double* xs, double* Ps) {
    if (!row || !y || !xs || !Ps || T < 1) return fail(SMC_EINVAL, "smc_host_kalman2_smooth: bad argument");
    if (const int rc = smc_host_kalman2_steps(row, y, T, predict_first, xs, Ps, nullptr)) return rc;
    double a1 = xs[2 * (T - 1)], a2 = xs[2 * (T - 1) + 1], P11 = Ps[3 * (T - 1)], P21 = Ps[3 * (T - 1) + 1], P22 = Ps[3 * (T - 1) + 2];
    for (int64_t t = T - 2; t >= 0; --t) {
        rts2_step(row, xs[2 * t], xs[2 * t + 1], Ps[3 * t], Ps[3 * t + 1], Ps[3 * t + 2], a1, a2, P11, P21, P22);
        xs[2 * t] = a1; xs[2 * t + 1] = a2;
        Ps[3 * t] = P11; Ps[3 * t + 1] = P21; Ps[3 * t + 2] = P22;
    }
    return SMC_OK;
}

// simulate(rng, model, T) for a two-state row, on the host: x [2][T] (or NULL), y [T]
extern "C" int smc_simulate_lg2(const double* row, int64_t T, uint64_t seed, double* x, double* y) {
    if (!row || !y || T < 1 || T > K2_MAX_T) return fail(SMC_EINVAL, "smc_simulate_lg2: bad argument");
    double x1 = 0.0, x2 = 0.0;
    for (int64_t t = 0; t < T; ++t) {
        double z0, z1, e, spare;
        box_muller(draw(seed, 0u, SIM_STREAM, (uint32_t)t, SLOT_NORMAL0), z0, spare);
        box_muller(draw(seed, 0u, SIM_STREAM, (uint32_t)t, SLOT_NORMAL0 + 1), z1, spare);
        box_muller(draw(seed, 0u, SIM_STREAM, (uint32_t)t, SLOT_OBS), e, spare);
        lg2_sim_step(row, t == 0, z0, z1, e, x1, x2, y[t]);
        if (x) { x[t] = x1; x[(size_t)T + (size_t)t] = x2; }
    }
    return SMC_OK;
}
