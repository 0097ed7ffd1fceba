"""References of the pair-moment tests, independent of the library, in the style of smoother_reference.py.

    pairs_ref      the FFBS recursion in np.longdouble with exact sums, and from its pair probabilities
                   P_ij = w_t^i f_ij ws_{t+1}^j / D_j the lag-one moments  cross[t][a][c] = sum_ij P_ij x_t^{i,a} x_{t+1}^{j,c}  and
                   resid2[t][c] = sum_ij P_ij (x_{t+1}^{j,c} - m_c(x_t^i))^2,  each with the sum of the absolute terms
                   sum_ij P_ij |h_ij| that the bound of the host twin is stated against
    centre_ref     the transition's centre m(x) of the three families, in long double from the textbook formulas
    kalman_em_step one EM step of (A, Q, R) of a linear-Gaussian model from the exact Kalman / RTS moments, in plain numpy
"""
import numpy as np

import smoother_reference as R

LD = R.LD


def centre_ref(model, raw, xp):
    """m_c(xp) for xp [d][...] -> a list of d long-double arrays"""
    raw = [LD(v) for v in np.asarray(raw, dtype=np.float64)]
    xp = [np.asarray(v, dtype=LD) for v in xp]
    if model == R.LG1D:
        return [raw[0] * xp[0]]
    if model == R.SV1D:
        return [raw[0] + raw[1] * (xp[0] - raw[0])]
    return list(xp)


def pairs_ref(model, raw, x, w):
    """(cross [T-1][d][d], resid2 [T-1][d], |cross|, |resid2|, cond cross, cond resid2) in np.longdouble for the clouds x [T][d][n],
    w [T][n]: the moments, the sums of their absolute terms sum_ij P_ij |h_ij|, and the same sums with every term weighted by
    |logf_ij| + |logD_j|, the magnitudes in the exponent of its pair probability.  Particles of weight 0 are left out whatever
    their states; NaN everywhere for a filter with a step at which every weight is 0"""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    T, n = w.shape
    d = R.DIM[model]
    out = [np.zeros((T - 1, d, d), dtype=LD), np.zeros((T - 1, d), dtype=LD), np.zeros((T - 1, d, d), dtype=LD), np.zeros((T - 1, d), dtype=LD),
           np.zeros((T - 1, d, d), dtype=LD), np.zeros((T - 1, d), dtype=LD)]
    if not np.all((w > 0).any(axis=1)):
        for a in out:
            a[:] = np.nan
        return out
    ws = w[T - 1].astype(LD)
    for t in range(T - 2, -1, -1):
        src = np.flatnonzero(w[t] > 0)
        tgt = np.flatnonzero(ws > 0)
        xs = [x[t, r, src].astype(LD)[:, None] for r in range(d)]
        xt = [x[t + 1, r, tgt].astype(LD)[None, :] for r in range(d)]
        F = R.logf_ref(model, raw, xs, xt)
        A = np.log(w[t, src].astype(LD))[:, None] + F
        M = A.max(axis=0)
        logD = M + np.log(R.exact_sum(np.exp(A - M[None, :]), 0))
        P = w[t, src].astype(LD)[:, None] * ws[tgt][None, :] * np.exp(F - logD[None, :])
        m = centre_ref(model, raw, xs)
        E = np.abs(F) + np.abs(logD)[None, :]                            # the magnitudes in the exponent of p_ij
        for c in range(d):
            h = (xt[c] - m[c]) ** 2
            out[1][t, c] = R.exact_sum((P * h).ravel(), 0)
            out[3][t, c] = out[1][t, c]                                  # (h >= 0)
            out[5][t, c] = R.exact_sum((P * h * E).ravel(), 0)
            for a in range(d):
                h = xs[a] * xt[c]
                out[0][t, a, c] = R.exact_sum((P * h).ravel(), 0)
                out[2][t, a, c] = R.exact_sum((P * np.abs(h)).ravel(), 0)
                out[4][t, a, c] = R.exact_sum((P * np.abs(h) * E).ravel(), 0)
        nxt = np.zeros(n, dtype=LD)
        nxt[src] = R.exact_sum(P, 1)
        ws = nxt
    return out


def kalman_em_moments(raw, y):
    """(mean [T], var [T], cross [T-1]) of p(x_1:T | y_1:T) of the LG1D row raw: the scalar Kalman filter and RTS smoother with
    the lag-one covariance C_t = G_t Ps_{t+1}; cross = C + mean_t mean_{t+1}"""
    A, B, Q, Rr, x0, s0 = [float(v) for v in raw]
    T = len(y)
    mp, Pp, mf, Pf = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T)
    for t in range(T):
        mp[t], Pp[t] = (x0, s0) if t == 0 else (A * mf[t - 1], A * A * Pf[t - 1] + Q)
        K = Pp[t] * B / (B * B * Pp[t] + Rr)
        mf[t] = mp[t] + K * (y[t] - B * mp[t])
        Pf[t] = Pp[t] - K * B * Pp[t]
    ms, Ps, Cs = mf.copy(), Pf.copy(), np.zeros(T - 1)
    for t in range(T - 2, -1, -1):
        G = Pf[t] * A / Pp[t + 1]
        ms[t] = mf[t] + G * (ms[t + 1] - mp[t + 1])
        Ps[t] = Pf[t] + G * G * (Ps[t + 1] - Pp[t + 1])
        Cs[t] = G * Ps[t + 1]
    return ms, Ps, Cs + ms[:-1] * ms[1:]


def kalman_em_step(raw, y):
    """(A, Q, R) after one exact EM step from the LG1D row raw (Shumway and Stoffer 1982, scalar case, x0 and sigma0 held)"""
    B = float(raw[1])
    y = np.asarray(y, dtype=np.float64)
    T = y.size
    ms, Ps, cr = kalman_em_moments(raw, y)
    e2 = Ps + ms ** 2
    S00, S11, S10 = e2[:-1].sum(), e2[1:].sum(), cr.sum()
    a = S10 / S00
    q = (S11 - 2 * a * S10 + a * a * S00) / (T - 1)
    r = ((y - B * ms) ** 2 + B * B * Ps).mean()
    return np.array([a, q, r])
