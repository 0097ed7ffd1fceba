"""References for the RTS smoother of an IBIS cloud (csrc/smc_spec.h "the RTS smoother of an IBIS cloud"), in numpy long double:

    backward(rows, xf, Sf)        (a) the backward recursion over a GIVEN filtered record [T][M]: xs, Ps, and the gain G and the
                                  conditional variance V of every step.  It starts from the record under test's own forward pass,
                                  so it measures the backward pass alone
    dense(row, y, predict_first)  (b) Gaussian conditioning without any recursion: the joint covariance of (x_1:T, y_1:T) built
                                  from the row entry by entry, then E[x | y], Var[x | y] and the lag-one covariances by one
                                  Cholesky solve
    paths(rows, which, xf, Sf, z) every entry of the backward-sampled paths from the normals z the twin reports
    normal(L, seed, p, stream, t) the normal of path p at step t rebuilt from the library's Philox and Box-Muller probes alone:
                                  the counter layout (p >> 1, stream, t, slot), the half, the slot

Rows are (A, B, Q, R, x0, sigma0) with sigma0 a variance, as kalman_step reads them.
"""
import ctypes as C

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
SLOT_RTS = 36
OTHER_SLOTS = tuple(range(0, 36))          # the step's, PMMH's, the outer level's (.. 34) and backward simulation's (35)


def gain(A, Q, Sf):
    """(G, V) of a step in long double (arrays broadcast): Sp = A^2 Sf + Q; G = Sf A / Sp, V = Sf Q / Sp; Sp = 0: (0, Sf)"""
    A, Q, Sf = np.broadcast_arrays(np.asarray(A, dtype=LD), np.asarray(Q, dtype=LD), np.asarray(Sf, dtype=LD))
    Sp = A * A * Sf + Q
    on = Sp > 0
    safe = np.where(on, Sp, LD(1))
    return np.where(on, Sf * A / safe, LD(0)), np.where(on, Sf * Q / safe, Sf)


def backward(rows, xf, Sf):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
    xf, Sf = np.asarray(xf, dtype=LD), np.asarray(Sf, dtype=LD)
    T = xf.shape[0]
    A, Q = rows[:, 0].astype(LD), rows[:, 2].astype(LD)
    xs, Ps = xf.copy(), Sf.copy()
    G, V = np.zeros_like(xf), Sf.copy()
    for t in range(T - 2, -1, -1):
        G[t], V[t] = gain(A, Q, Sf[t])
        xs[t] = xf[t] + G[t] * (xs[t + 1] - A * xf[t])
        Ps[t] = V[t] + G[t] * G[t] * Ps[t + 1]
    return xs, Ps, G, V


def _cholesky_solve(S, Bm):
    """S^-1 Bm for a symmetric positive definite S, long double throughout"""
    n = S.shape[0]
    Lc = np.zeros((n, n), dtype=LD)
    for i in range(n):
        for j in range(i + 1):
            s = S[i, j] - (Lc[i, :j] * Lc[j, :j]).sum()
            Lc[i, j] = np.sqrt(s) if i == j else s / Lc[j, j]
    Y = np.zeros(Bm.shape, dtype=LD)
    for i in range(n):
        Y[i] = (Bm[i] - (Lc[i, :i, None] * Y[:i]).sum(axis=0)) / Lc[i, i]
    X = np.zeros(Bm.shape, dtype=LD)
    for i in range(n - 1, -1, -1):
        X[i] = (Y[i] - (Lc[i + 1:, i, None] * X[i + 1:]).sum(axis=0)) / Lc[i, i]
    return X


def dense(row, y, predict_first):
    """(mean [T], var [T], lag-one covariances [T-1]) of x | y for one row"""
    A, B, Q, R, x0, s0 = (LD(v) for v in row)
    y = np.asarray(y, dtype=LD)
    T = y.size
    mu, v = np.zeros(T, dtype=LD), np.zeros(T, dtype=LD)
    mu[0], v[0] = (A * x0, A * A * s0 + Q) if predict_first else (x0, s0)
    for t in range(1, T):
        mu[t], v[t] = A * mu[t - 1], A * A * v[t - 1] + Q
    Cx = np.zeros((T, T), dtype=LD)
    for s in range(T):
        for t in range(s, T):
            Cx[s, t] = Cx[t, s] = A ** (t - s) * v[s]
    Syy = B * B * Cx + R * np.eye(T, dtype=LD)
    Cxy = B * Cx
    rhs = np.concatenate([(y - B * mu)[:, None], Cxy.T], axis=1)
    sol = _cholesky_solve(Syy, rhs)
    mean = mu + Cxy @ sol[:, 0]
    cov = Cx - Cxy @ sol[:, 1:]
    return mean, np.diag(cov).copy(), np.array([cov[t, t + 1] for t in range(T - 1)], dtype=LD)


def paths(rows, which, xf, Sf, z):
    """the paths [T][Mp] in long double: xf, Sf [T][M] the filtered record, z [T][Mp] the normals"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
    which = np.asarray(which, dtype=np.int64)
    A, Q = rows[which, 0].astype(LD), rows[which, 2].astype(LD)
    xfp, Sfp, z = np.asarray(xf, dtype=LD)[:, which], np.asarray(Sf, dtype=LD)[:, which], np.asarray(z, dtype=LD)
    T = z.shape[0]
    out = np.zeros(z.shape, dtype=LD)
    out[T - 1] = xfp[T - 1] + np.sqrt(np.maximum(Sfp[T - 1], 0)) * z[T - 1]
    for t in range(T - 2, -1, -1):
        G, V = gain(A, Q, Sfp[t])
        out[t] = (xfp[t] + G * (out[t + 1] - A * xfp[t])) + np.sqrt(np.maximum(V, 0)) * z[t]
    return out


def normal(L, seed, p, stream, t, slot=SLOT_RTS):
    """z of path p at step t: Box-Muller of Philox(counter (p >> 1, stream, t, slot), key (seed lo, seed hi)), z0 for an even p"""
    u32 = C.c_uint32 * 4
    out = u32()
    L.lib().smc_host_philox4x32_10(u32(p >> 1, stream, t, slot), (C.c_uint32 * 2)(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), out)
    z0, z1 = C.c_double(), C.c_double()
    L.lib().smc_host_box_muller(out, C.byref(z0), C.byref(z1))
    return z1.value if p & 1 else z0.value
