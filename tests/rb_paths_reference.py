"""References of the Rao-Blackwellised backward-simulation tests (smc_rb_sample_paths, smc_host_rb_sample_paths),
independent of the library's arithmetic and of its backward recursion: everything here is np.longdouble and runs FORWARD.

    rb_clouds        (x [T][4][n], w [T][n]) of a small numpy particle filter around smc_host_rb_steps (multinomial resampling by
                     numpy at every step): clouds of the marginal UCSV filter without a GPU
    step_cdf         the CDF of the backward kernel of one step WITHOUT any backward information recursion: the weight of
                     candidate i is w_i f(u_{t+1} | u_i) times the product of the forward Kalman predictive densities of y_{t+1:T},
                     the Kalman filter started at (m_i, P_i) and run through the path's own later volatilities
    check_indices    every index of every path against its CDF and the path's own uniform
    trend            forward Kalman and RTS along one volatility path: (mean, var, filtered m, filtered P, predicted P-)
    summary          the eight columns in the chunked order of the specification, restated in Python
"""
import numpy as np

import paths_reference as PR

LD = np.longdouble
EPS = 2.0 ** -52
CH = 128                                  # SMOOTH_CH
SLOT_RB_TREND = 37

_CLOUDS = {}


def rb_clouds(L, raw, n, T, y, seed=5):
    key = (tuple(raw), n, T, tuple(np.asarray(y, dtype=float)[:T]), seed)
    if key not in _CLOUDS:
        r = np.random.default_rng(seed)
        xs, ws = [], []
        s = np.zeros((4, n))
        for t in range(T):
            s, lw = L.host_rb_steps(raw, s, r.normal(size=(2, n)), float(y[t]), t == 0)
            w = np.exp(lw - lw.max())
            w /= w.sum()
            xs.append(s.copy())
            ws.append(w.copy())
            s = s[:, r.choice(n, size=n, p=w)]
        _CLOUDS[key] = (np.array(xs), np.array(ws))
    return _CLOUDS[key]


def step_cdf(raw, x_t, w_t, y, t, lse_path, lsn_path):
    """F [n] (np.longdouble).  x_t [4][n], w_t [n]: the cloud of step t; lse_path, lsn_path [T]: the volatilities the path holds
    (read at steps t+1 .. T-1 only).  Sources of weight 0 have probability 0 whatever their states."""
    T = len(y)
    ge, gn = LD(raw[0]), LD(raw[1])
    live = np.flatnonzero(w_t > 0)
    a = np.log(w_t[live].astype(LD))
    if t < T - 1:
        m, lse, lsn, P = (x_t[r, live].astype(LD) for r in range(4))
        d1, d2 = (LD(lse_path[t + 1]) - lse) / ge, (LD(lsn_path[t + 1]) - lsn) / gn
        a = a - LD(0.5) * d1 * d1 - LD(0.5) * d2 * d2
        q = np.exp(lse)                                               # the trend moves with the PREVIOUS lse
        for s in range(t + 1, T):
            Pm = P + q
            R = np.exp(LD(lsn_path[s]))
            S = Pm + R
            e = LD(y[s]) - m
            a = a - LD(0.5) * (np.log(S) + e * e / S)
            K = Pm / S
            m, P = m + K * e, Pm * R / S
            q = np.exp(LD(lse_path[s]))
    e = np.exp(a - a.max())
    pr = np.zeros(w_t.size, dtype=LD)
    pr[live] = e / PR.R.exact_sum(e, 0)
    return np.cumsum(pr)


def check_indices(L, raw, x, w, y, idx, vol, seed, stream, tol_scale=1.0):
    """asserts F_{i-1} - tol <= u / 2^64 < F_i + tol for every path and step, tol = tol_scale ((n + 1) 2^-40 + 1000 eps); returns the
    largest distance by which a u lies OUTSIDE [F_{i-1}, F_i) (0: every index is the one the exact CDF picks)"""
    T, n = w.shape
    M = idx.shape[1]
    tol = LD(tol_scale) * LD((n + 1) * 2.0 ** -PR.PATH_BITS + 1000 * EPS)
    worst = LD(0)
    assert np.all(idx >= 0) and np.all(idx < n)
    for p in range(M):
        for t in range(T - 1, -1, -1):
            F = step_cdf(raw, x[t], w[t], y, t, vol[:, 0, p], vol[:, 1, p])
            i = int(idx[t, p])
            U = LD(PR.path_uniform(L, seed, p, stream, t)) / LD(2) ** 64
            lo = F[i - 1] if i > 0 else LD(0)
            assert lo - tol <= U < F[i] + tol, (n, t, p, i, float(lo), float(U), float(F[i]))
            worst = max(worst, lo - U, U - F[i])
    return float(worst)


def trend(raw, y, lse, lsn):
    """(mean [T], var [T], mf [T], Pf [T], Pm [T]) in long double for one volatility path: the Kalman filter of
    x_t = x_{t-1} + N(0, exp(lse_{t-1})), x_0 ~ N(x0, exp(lse0)), y_t = x_t + N(0, exp(lsn_t)), and the RTS pass over it"""
    T = len(y)
    mf, Pf, Pm = np.zeros(T, dtype=LD), np.zeros(T, dtype=LD), np.zeros(T, dtype=LD)
    m, P = LD(raw[2]), LD(0)
    for t in range(T):
        Pm[t] = P + np.exp(LD(raw[3]) if t == 0 else LD(lse[t - 1]))
        R = np.exp(LD(lsn[t]))
        S = Pm[t] + R
        K = Pm[t] / S
        m, P = m + K * (LD(y[t]) - m), Pm[t] * R / S
        mf[t], Pf[t] = m, P
    mean, var = mf.copy(), Pf.copy()
    for t in range(T - 2, -1, -1):
        G = Pf[t] / Pm[t + 1]
        mean[t] = mf[t] + G * (mean[t + 1] - mf[t])
        var[t] = Pf[t] + G * G * (var[t + 1] - Pm[t + 1])
    return mean, var, mf, Pf, Pm


def trend_normal(L, seed, p, stream, t):
    import rts_reference
    return rts_reference.normal(L, seed, p, stream, t, slot=SLOT_RB_TREND)


def chunked(terms):
    """the specification's order of summation in doubles: chunks of CH in ascending order, plain adds from +0.0"""
    tot = 0.0
    for c0 in range(0, len(terms), CH):
        s = 0.0
        for v in terms[c0:c0 + CH]:
            s += float(v)
        tot += s
    return tot


def summary(idx0, tmean_t, tvar_t, lse_t, lsn_t):
    """out[t] [8] restated: complete paths only (idx0 >= 0), an incomplete path adds +0.0"""
    on = np.asarray(idx0) >= 0
    cnt = float(on.sum())
    out = np.full(8, np.nan)
    out[7] = cnt
    if cnt == 0:
        return out
    for v, cm, cv in ((tmean_t, 0, 2), (tvar_t, 1, -1), (lse_t, 3, 4), (lsn_t, 5, 6)):
        mean = chunked([v[p] if on[p] else 0.0 for p in range(len(v))]) / cnt
        out[cm] = mean
        if cv >= 0:
            out[cv] = chunked([(v[p] - mean) * (v[p] - mean) if on[p] else 0.0 for p in range(len(v))]) / cnt
    return out
