"""References of the smoother tests, independent of the library: no step arithmetic of the library's is used here.

    logf_ref      the log transition densities of the three families in np.longdouble, from the textbook formulas
    ffbs_ref      the FFBS recursion in np.longdouble, log domain with the row maximum, with exact sums
                  (exact_sum: math.fsum over the long doubles split into pairs of doubles)
    rts_smoother  the scalar Kalman filter and Rauch-Tung-Striebel smoother of a linear-Gaussian model (textbook; the filter starts
                  at x_1 ~ N(x0, sigma0), as bootstrap_filter does)
    exact_moments mean = sum w x, var = sum w (x - mean)^2 with math.fsum
"""
import math

import numpy as np

LD = np.longdouble
LG1D, SV1D, UCSV3D = 1, 2, 3
DIM = {LG1D: 1, SV1D: 1, UCSV3D: 3}
_HALF_LOG_2PI = LD(0.5) * np.log(LD(8) * np.arctan(LD(1)))   # 2 pi = 8 atan(1), in long double


def _lognormal(x, mean, sd):
    z = (x - mean) / sd
    return -LD(0.5) * z * z - np.log(sd) - _HALF_LOG_2PI


def logf_ref(model, raw, xp, x):
    """log f(x | xp), broadcasting over xp [d][...] and x [d][...] (np.longdouble)"""
    raw = [LD(v) for v in np.asarray(raw, dtype=np.float64)]
    xp = [np.asarray(v, dtype=LD) for v in xp]
    x = [np.asarray(v, dtype=LD) for v in x]
    if model == LG1D:      # x ~ N(A xp, sqrt(Q)), Q a variance
        return _lognormal(x[0], raw[0] * xp[0], np.sqrt(raw[2]))
    if model == SV1D:      # x ~ N(mu + rho (xp - mu), sigma)
        return _lognormal(x[0], raw[0] + raw[1] * (xp[0] - raw[0]), raw[2])
    if model == UCSV3D:    # the trend moves with the PREVIOUS log-volatility; the gammas are standard deviations
        return (_lognormal(x[0], xp[0], np.exp(LD(0.5) * xp[1])) + _lognormal(x[1], xp[1], raw[0]) + _lognormal(x[2], xp[2], raw[1]))
    raise ValueError(model)


def exact_sum(a, axis):
    """sums of long doubles along `axis` without rounding error, math.fsum style: a long double (64 mantissa bits) is the exact
    sum of two doubles, hi = the nearest double and lo = the remainder; math.fsum adds all of them exactly and rounds once; a
    second pass with -s added gives what that rounding lost, so the result hi + lo is exact to about 2^-105"""
    a = np.moveaxis(np.asarray(a, dtype=LD), axis, -1)
    hi = a.astype(np.float64)
    lo = (a - hi.astype(LD)).astype(np.float64)
    out = np.zeros(a.shape[:-1], dtype=LD)
    for idx in np.ndindex(*a.shape[:-1]):
        parts = hi[idx].tolist() + lo[idx].tolist()
        s1 = math.fsum(parts)
        out[idx] = LD(s1) + LD(math.fsum(parts + [-s1]))
    return out


def ffbs_ref(model, raw, x, w):
    """smoothed weights [T][n] (np.longdouble) of the clouds x [T][d][n], w [T][n]; NaN everywhere for a filter with a step
    at which every weight is 0"""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    T, n = w.shape
    ws = np.zeros((T, n), dtype=LD)
    if not np.all((w > 0).any(axis=1)):
        ws[:] = np.nan
        return ws
    ws[T - 1] = w[T - 1]
    for t in range(T - 2, -1, -1):
        src = np.flatnonzero(w[t] > 0)
        tgt = np.flatnonzero(ws[t + 1] > 0)
        F = logf_ref(model, raw, [x[t, r, src][:, None] for r in range(DIM[model])], [x[t + 1, r, tgt][None, :] for r in range(DIM[model])])
        A = np.log(w[t, src].astype(LD))[:, None] + F
        M = A.max(axis=0)
        logD = M + np.log(exact_sum(np.exp(A - M[None, :]), 0))
        ws[t, src] = w[t, src].astype(LD) * exact_sum(ws[t + 1, tgt][None, :] * np.exp(F - logD[None, :]), 1)
    return ws


def rts_smoother(raw, y):
    """(m [T], P [T]) of p(x_t | y_1:T) for the LG1D row raw = (A, B, Q, R, x0, sigma0), x_1 ~ N(x0, sigma0) (variances)"""
    A, B, Q, R, x0, s0 = [float(v) for v in raw]
    T = len(y)
    mp, Pp, mf, Pf = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T)
    for t in range(T):
        mp[t], Pp[t] = (x0, s0) if t == 0 else (A * mf[t - 1], A * A * Pf[t - 1] + Q)
        S = B * B * Pp[t] + R
        K = Pp[t] * B / S
        mf[t] = mp[t] + K * (y[t] - B * mp[t])
        Pf[t] = (1.0 - K * B) * Pp[t]
    ms, Ps = mf.copy(), Pf.copy()
    for t in range(T - 2, -1, -1):
        G = Pf[t] * A / Pp[t + 1]
        ms[t] = mf[t] + G * (ms[t + 1] - mp[t + 1])
        Ps[t] = Pf[t] + G * G * (Ps[t + 1] - Pp[t + 1])
    return ms, Ps


def exact_moments(x, ws):
    """(mean, var) of one coordinate x [n] under the weights ws [n], exactly rounded sums of the double products
    (zero-weight particles left out)"""
    keep = ws > 0
    x, ws = np.asarray(x, dtype=np.float64)[keep], np.asarray(ws, dtype=np.float64)[keep]
    m = math.fsum((ws.astype(LD) * x.astype(LD)).astype(np.float64))
    e = x.astype(LD) - LD(m)
    v = math.fsum((ws.astype(LD) * e * e).astype(np.float64))
    return m, v
