"""References of the backward-simulation tests (smc_sample_paths, smc_host_sample_paths), independent of the
library's arithmetic: the densities come from smoother_reference.logf_ref in np.longdouble, the sums are exact.

    path_uniform     the 64-bit uniform of path p at step t, rebuilt from smc_host_philox4x32_10 alone: counter (p >> 1, stream,
                     t, SLOT_PATH), key = the two halves of the seed, the low pair of words for an even p, the high pair for an odd
    step_cdf         the CDF F_i of the backward kernel of one step: proportional to w_t^i (last step) or w_t^i f(x_next | x_t^i)
    check_indices    every index of every path against its CDF: F_{i-1} - tol <= u / 2^64 < F_i + tol
    rts_lag_one      C_t = Cov(x_t, x_{t+1} | y_1:T) = G_t Ps_{t+1} of the linear-Gaussian model (Rauch-Tung-Striebel)
    chi2_cells / chi2_bound   Pearson's statistic with small cells pooled, and the 1 - 1e-6 quantile of chi-square
    recorded_clouds  (x [T][d][n], w [T][n]) of the oracle's bootstrap filter, state() after every step
"""
import ctypes as C
import math

import numpy as np

import smoother_reference as R

LD = np.longdouble
SLOT_PATH = 35
PATH_BITS = 40
EPS = 2.0 ** -52


def path_uniform(L, seed, p, stream, t):
    out = (C.c_uint32 * 4)()
    ctr = (C.c_uint32 * 4)(p >> 1, stream & 0xFFFFFFFF, t, SLOT_PATH)
    key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    L.lib().smc_host_philox4x32_10(ctr, key, out)
    return (out[3] << 32 | out[2]) if p & 1 else (out[1] << 32 | out[0])


def step_cdf(model, raw, x_t, w_t, x_next=None):
    """F [n] (np.longdouble), F_i = sum_{l <= i} P_l; x_t [d][n], w_t [n]; x_next [d] the state the path holds at the next step,
    None at the last step.  Sources of weight 0 have probability 0 whatever their states."""
    d = R.DIM[model]
    live = np.flatnonzero(w_t > 0)
    a = np.log(w_t[live].astype(LD))
    if x_next is not None:
        a = a + R.logf_ref(model, raw, [x_t[r, live] for r in range(d)], [LD(x_next[r]) for r in range(d)])
    e = np.exp(a - a.max())
    P = np.zeros(w_t.size, dtype=LD)
    P[live] = e / R.exact_sum(e, 0)
    return np.cumsum(P)


def check_indices(L, model, raw, x, w, idx, seed, stream):
    """asserts the bound for every path and step; returns the largest distance by which a u lies OUTSIDE [F_{i-1}, F_i) (0 when
    every index is the one the exact CDF picks)"""
    T, n = w.shape
    M = idx.shape[1]
    tol = LD((n + 1) * 2.0 ** -PATH_BITS + 1000 * EPS)
    worst = LD(0)
    assert np.all(idx >= 0) and np.all(idx < n)
    for t in range(T - 1, -1, -1):
        cdfs = {}
        for p in range(M):
            j = None if t == T - 1 else int(idx[t + 1, p])
            if j not in cdfs:
                cdfs[j] = step_cdf(model, raw, x[t], w[t], None if j is None else x[t + 1, :, j])
            F = cdfs[j]
            i = int(idx[t, p])
            U = LD(path_uniform(L, seed, p, stream, t)) / LD(2) ** 64
            lo = F[i - 1] if i > 0 else LD(0)
            assert lo - tol <= U < F[i] + tol, (model, n, t, p, i, float(lo), float(U), float(F[i]))
            worst = max(worst, lo - U, U - F[i])
    return float(worst)


def rts_lag_one(raw, y):
    """C [T - 1]: Cov(x_t, x_{t+1} | y_1:T) = G_t Ps_{t+1}, G_t = Pf_t A / Pp_{t+1} (the smoother gain of rts_smoother)"""
    A, B, Q, Rr, x0, s0 = [float(v) for v in raw]
    T = len(y)
    Pp, Pf = np.zeros(T), np.zeros(T)
    for t in range(T):
        Pp[t] = s0 if t == 0 else A * A * Pf[t - 1] + Q
        Pf[t] = (1.0 - Pp[t] * B / (B * B * Pp[t] + Rr) * B) * Pp[t]
    _, Ps = R.rts_smoother(raw, y)
    return np.array([Pf[t] * A / Pp[t + 1] * Ps[t + 1] for t in range(T - 1)])


def chi2_bound(df, z=4.753424):
    """the 1 - 1e-6 quantile of chi-square with df degrees of freedom (z: that quantile of the standard normal); scipy's when it
    is there, else the Wilson-Hilferty approximation"""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1 - 1e-6, df))
    except ImportError:
        c = 2.0 / (9.0 * df)
        return df * (1.0 - c + z * math.sqrt(c)) ** 3


def chi2_cells(counts, expected):
    """(statistic, cells): one cell per category of expectation >= 5, the others pooled into one cell; a pooled cell of expectation
    below 5 is merged into the smallest other cell"""
    counts, expected = np.asarray(counts, dtype=float), np.asarray(expected, dtype=float)
    big = expected >= 5
    o, e = list(counts[big]), list(expected[big])
    po, pe = counts[~big].sum(), expected[~big].sum()
    assert np.all(counts[expected <= 0] == 0), "a category of expectation 0 was drawn"
    if pe >= 5 or not e:
        if pe > 0 or po > 0:
            o.append(po)
            e.append(pe)
    else:
        k = int(np.argmin(e))
        o[k] += po
        e[k] += pe
    o, e = np.array(o), np.array(e)
    return float(((o - e) ** 2 / e).sum()), len(e)


def path_moments(xs):
    """per-filter path mean of x_t [T] and sample covariance of (x_t, x_{t+1}) [T - 1] over the paths; xs [T][M]"""
    mean = xs.mean(axis=1)
    dev = xs - mean[:, None]
    cov = (dev[:-1] * dev[1:]).sum(axis=1) / (xs.shape[1] - 1)
    return mean, cov


def z_scores(per_filter, exact):
    """|average over the filters - exact| / (sd over the filters / sqrt(K)); per_filter [K][...]"""
    K = per_filter.shape[0]
    return np.abs(per_filter.mean(axis=0) - exact) / (per_filter.std(axis=0, ddof=1) / np.sqrt(K))


_CLOUDS = {}


def recorded_clouds(L, ob, model, raw, n, T, seed=5, stream=0):
    key = (model, tuple(raw), n, T, seed, stream)
    if key not in _CLOUDS:
        _, y = L.simulate(model, raw, max(T, 2), 1998)
        f = ob.Filter(model, raw, n, seed=seed, stream=stream)
        xs, wsv = [], []
        for t in range(T):
            f.bootstrap_filter(float(y[0])) if t == 0 else f.step(float(y[t]))
            x, w, _, _ = f.state()
            xs.append(x.copy())
            wsv.append(w.copy())
        _CLOUDS[key] = (np.array(xs), np.array(wsv))
    return _CLOUDS[key]
