"""TEST INFRASTRUCTURE: src/plotting_utils.jl:94-137 (observation_dist, estimated_trend, quantile of an IBIS sampler) restated
with numpy and exactly rounded sums (math.fsum), independent of the library's order of operations.  Also the two extensions the
library documents: `ahead` (one Kalman prediction first, kalman_filter.jl:39-42) and `between` (the spread of the component
means).  Never imported by the product."""
import math
import statistics

import numpy as np


def weights(logw):
    """omega = exp(logw) / sum exp(logw) over the finite entries (max-shifted); -inf and NaN entries get weight 0"""
    logw = np.asarray(logw, dtype=np.float64)
    ok = np.isfinite(logw)
    w = np.zeros(logw.size)
    if ok.any():
        e = np.exp(logw[ok] - logw[ok].max())
        w[ok] = e / math.fsum(e)
    return w


def components(rows, x, S, ahead=0):
    """(ym, vm) per particle: B x and B S B' + R (:104-105), after x <- A x, S <- A S A' + Q when ahead = 1"""
    rows = np.asarray(rows, dtype=np.float64)
    A, B, Q, R = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    x, S = np.asarray(x, dtype=np.float64), np.asarray(S, dtype=np.float64)
    if ahead:
        x, S = A * x, A * A * S + Q
    return B * x, B * B * S + R


def wsum(w, v):
    """sum_m w_m v_m over the particles with w_m > 0 (a zero weight takes its particle out, whatever v_m is), exactly rounded"""
    on = w > 0.0
    return math.fsum(w[on] * v[on])


def summary(rows, x, S, logw, ahead=0):
    """dict of y, Sigma, between, xbar, Sbar, between_x and of the magnitudes the error bounds are stated in"""
    w = weights(logw)
    ym, vm = components(rows, x, S, ahead)
    x, S = np.asarray(x, dtype=np.float64), np.asarray(S, dtype=np.float64)
    y, xbar = wsum(w, ym), wsum(w, x)
    return {
        "y": y, "Sigma": wsum(w, vm), "between": wsum(w, (ym - y) ** 2),
        "xbar": xbar, "Sbar": wsum(w, S), "between_x": wsum(w, (x - xbar) ** 2),
        "abs_y": wsum(w, np.abs(ym)), "abs_Sigma": wsum(w, np.abs(vm)), "abs_xbar": wsum(w, np.abs(x)), "abs_Sbar": wsum(w, np.abs(S)),
        "dev_y": wsum(w, np.abs(ym - y)), "dev_x": wsum(w, np.abs(x - xbar)),
    }


def observation_dist(rows, x, S, logw):
    """plotting_utils.jl:94-112"""
    s = summary(rows, x, S, logw, 0)
    return s["y"], s["Sigma"]


def quantile(rows, x, S, logw, p):
    """plotting_utils.jl:128-137 on a sorted COPY of p"""
    y, Sigma = observation_dist(rows, x, S, logw)
    return np.array([statistics.NormalDist(y, math.sqrt(Sigma)).inv_cdf(v) for v in sorted(p)])


def grid_predictive_mean(y, n=4001):
    """E[y_{T+1} | y_1..T] of case_one_parameter (theta = A; B = 1, Q = 0.9, R = 0.8, prior N(0, 1) cut to [-1, 1]) by the
    quadrature of ibis_reference.grid_posterior_A - the same grid, log-posterior and trapezoid weights - with the integrand
    A x_T(A), x_T(A) the Kalman filtered mean.  Returns (predictive mean, posterior mean of A): the second is
    grid_posterior_A(y)[0], which ties the two quadratures together."""
    from oracle import kalman
    grid = np.linspace(-1.0, 1.0, n)
    xT, lp = np.zeros(n), np.zeros(n)
    for i, a in enumerate(grid):
        xf, _, z = kalman.log_likelihood(y, a, 1.0, 0.9, 0.8, 0.0, 1.0, predict_first=False)
        xT[i], lp[i] = xf, z - 0.5 * a * a
    w = np.exp(lp - lp.max())
    w[0] *= 0.5
    w[-1] *= 0.5
    w /= w.sum()
    return float(w @ (grid * xT)), float(w @ grid)


# ---- the clouds the summary tests share (host and GPU) -----------------------------------------------------------------------
SIZES = (1, 7, 8, 9, 512, 4099, 2 ** 16)


def random_cloud(M, seed):
    """rows (A, B, Q, R, x0, sigma0) with x0 = x and sigma0 = S (so that a device handle can be loaded with it through a
    ThetaMap that copies theta to the row), and log-weights spread over a few e-folds; the state has a level (mean 3)"""
    rng = np.random.default_rng(seed)
    x, S = rng.normal(3.0, 1.0, M), rng.lognormal(0.0, 0.5, M)
    rows = np.column_stack([rng.uniform(-1.0, 1.0, M), rng.uniform(0.5, 2.0, M), rng.lognormal(0.0, 0.5, M), rng.lognormal(0.0, 0.5, M), x, S])
    return rows, x.copy(), S.copy(), rng.normal(0.0, 3.0, M)


def resample_move_cloud(M, seed):
    """the shape a resample-move leaves a few steps later: many exact duplicates of a few ancestors, and a handful of particles
    holding nearly all the weight (log-weights hundreds of units apart)"""
    rows, x, S, _ = random_cloud(M, seed)
    rng = np.random.default_rng(seed + 1000)
    a = np.sort(rng.integers(0, max(1, M // 16), M))
    rows, x, S = rows[a], x[a], S[a]
    logw = rng.normal(-400.0, 60.0, M)
    logw[rng.integers(0, M, min(M, 5))] = rng.normal(0.0, 1.0, min(M, 5))
    return rows, x, S, logw


CLOUDS = {"random": random_cloud, "resample_move": resample_move_cloud}
