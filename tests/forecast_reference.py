"""The forecast specification (include/smc_hip.h "forecasts", csrc/smc_spec.h "forecasts") restated in numpy's longdouble, with the
error bounds the binary64 specification is allowed against it, and the closed-form laws of the propagated clouds.  TEST
INFRASTRUCTURE (no GPU): nothing here is used by the library.

One step of one particle, given its normals z (state) and e (observation):
  LG1D     x' = sqrt(Q) z + A x;  ym = B x';  yv = R;  yf = ym + sqrt(R) e
  SV1D     x' = sigma z + (rho (x - mu) + mu);  ym = 0;  sd = exp(x' / 2);  yv = sd^2;  yf = sd e
  UCSV3D   x0' = exp(lse / 2) z0 + x0;  lse' = g_eps z1 + lse;  lsn' = g_eta z2 + lsn;  ym = x0';  sd = exp(lsn' / 2);  yv = sd^2
  UCSV_RB  (m, a, b, P):  P' = P + exp(a);  a' = g_eps z0 + a;  b' = g_eta z1 + b;  m' = m;  ym = m;  yv = P' + exp(b');
           yf = ym + sqrt(yv) e

Error bounds, as tests/guided_reference.py derives them: u = 2^-52 is charged for every rounded operation (twice its half-ulp) and
2 ulp of the result for every sp_exp; an error dx of an argument of exp costs exp(x) (e^dx - 1).  The bounds are CARRIED through
the H steps: the error of a state row at horizon k enters the step to k + 1 through the derivative of the step (|A|, |rho|, 1 for the
random walks, exp for the volatilities).  They are derived from the order of operations smc_spec.h states, not fitted.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -52
LG1D, SV1D, UCSV3D, UCSV_RB = 1, 2, 3, 4
DIM = {LG1D: 1, SV1D: 1, UCSV3D: 3, UCSV_RB: 4}
NZ = {LG1D: 1, SV1D: 1, UCSV3D: 3, UCSV_RB: 2}
SLOT_NORMAL0, SLOT_OBS = 1, 8


def normals(ob, model, seed, stream, H, n):
    """(z [H][nz][n], e [H][n]): the normals of the forecast of n particles, from the oracle's pair-keyed draws"""
    z = np.array([[ob.state_normals(seed, stream, k + 1, SLOT_NORMAL0 + c, n) for c in range(NZ[model])] for k in range(H)])
    e = np.array([ob.state_normals(seed, stream, k + 1, SLOT_OBS, n) for k in range(H)])
    return z, e


def _exp_err(v, dv):
    """bound on |sp_exp(v~) - exp(v)| for |v~ - v| <= dv, v~ the double at hand: the argument's error and 2 ulp of the result"""
    ev = np.exp(v)
    return ev * np.expm1(dv) + 2 * U * ev * np.exp(dv)


def step(model, raw, x, z, e):
    """one step in longdouble: x [d][n] (longdouble), z [nz][n], e [n] doubles -> (x' [d][n], yf, ym, yv)"""
    z, e = np.asarray(z, dtype=LD), np.asarray(e, dtype=LD)
    r = [LD(v) for v in raw]
    half = LD(0.5)
    if model == LG1D:
        A, B, Q, R = r[:4]
        xn = np.stack([np.sqrt(Q) * z[0] + A * x[0]])
        ym, yv = B * xn[0], R + 0 * xn[0]
        return xn, ym + np.sqrt(R) * e, ym, yv
    if model == SV1D:
        mu, rho, sg = r[:3]
        xn = np.stack([sg * z[0] + (rho * (x[0] - mu) + mu)])
        sd = np.exp(half * xn[0])
        return xn, sd * e, 0 * sd, sd * sd
    if model == UCSV3D:
        xn = np.stack([np.exp(half * x[1]) * z[0] + x[0], r[0] * z[1] + x[1], r[1] * z[2] + x[2]])
        sd = np.exp(half * xn[2])
        return xn, xn[0] + sd * e, xn[0], sd * sd
    xn = np.stack([x[0], r[0] * z[0] + x[1], r[1] * z[1] + x[2], x[3] + np.exp(x[1])])
    yv = xn[3] + np.exp(xn[2])
    return xn, xn[0] + np.sqrt(yv) * e, xn[0], yv


def step_bounds(model, raw, x, dx, z, e, xn):
    """bounds on the errors of one binary64 step whose input rows x (doubles, [d][n]) are off by at most dx: (dx' [d][n], dyf, dym,
    dyv), evaluated at the doubles the specification works with (xn: its new state)"""
    a = np.abs
    if model == LG1D:
        A, B, Q, R = raw[:4]
        sQ, sR = np.sqrt(Q), np.sqrt(R)
        # sQ = sqrt: u; A x: u; the fma: u
        dxn = np.stack([a(A) * dx[0] + U * (a(sQ * z[0]) + a(A * x[0]) + a(xn[0]))])
        ym = B * xn[0]
        dym = a(B) * dxn[0] + U * a(ym)
        dyv = 3 * U * R + 0 * dym                         # sd = sqrt(R): u; sd sd: 2u + u
        dyf = dym + U * a(sR * e) + U * a(ym + sR * e)    # sd: u; the fma: u
        return dxn, dyf, dym, dyv
    if model == SV1D:
        mu, rho, sg = raw[:3]
        t = x[0] - mu
        inner = rho * t + mu
        dinner = a(rho) * (dx[0] + U * a(t)) + U * a(inner)
        dxn = np.stack([dinner + U * a(xn[0])])
        sd = np.exp(0.5 * xn[0])
        dsd = _exp_err(0.5 * xn[0], 0.5 * dxn[0])
        dyv = 2 * sd * dsd + dsd * dsd + U * sd * sd
        dyf = dsd * a(e) + U * a(sd * e)
        return dxn, dyf, 0 * dsd, dyv
    if model == UCSV3D:
        s = np.exp(0.5 * x[1])
        ds = _exp_err(0.5 * x[1], 0.5 * dx[1])
        dxn = np.stack([dx[0] + ds * a(z[0]) + U * a(xn[0]), dx[1] + U * a(xn[1]), dx[2] + U * a(xn[2])])
        sd = np.exp(0.5 * xn[2])
        dsd = _exp_err(0.5 * xn[2], 0.5 * dxn[2])
        dyv = 2 * sd * dsd + dsd * dsd + U * sd * sd
        dyf = dxn[0] + dsd * a(e) + U * a(xn[0] + sd * e)
        return dxn, dyf, dxn[0], dyv
    dQ = _exp_err(x[1], dx[1])
    dxn = np.stack([dx[0], dx[1] + U * a(xn[1]), dx[2] + U * a(xn[2]), dx[3] + dQ + U * a(xn[3])])
    yv = xn[3] + np.exp(xn[2])
    dyv = dxn[3] + _exp_err(xn[2], dxn[2]) + U * yv
    s = np.sqrt(yv)
    ds = dyv / (s + np.sqrt(np.maximum(yv - dyv, 0.0))) + U * s     # |sqrt(v + d) - sqrt(v)| <= d / (sqrt(v) + sqrt(v - d)); the sqrt: u
    dyf = dxn[0] + ds * a(e) + U * a(xn[0] + s * e)
    return dxn, dyf, dxn[0], dyv


def trajectory(model, raw, x0, z, e):
    """the longdouble trajectory from x0 [d][n]: (xf [H][d][n], yf, ym, yv [H][n])"""
    x = np.asarray(x0, dtype=LD)
    out = [], [], [], []
    for k in range(z.shape[0]):
        x, yf, ym, yv = step(model, raw, x, z[k], e[k])
        for o, v in zip(out, (x, yf, ym, yv)):
            o.append(v)
    return tuple(np.array(o) for o in out)


def trajectory_bounds(model, raw, x0, z, e, xf):
    """the carried bounds along the binary64 trajectory xf [H][d][n] that started at x0 (exact: dx = 0)"""
    x, dx = np.asarray(x0, dtype=np.float64), np.zeros_like(np.asarray(x0, dtype=np.float64))
    out = [], [], [], []
    for k in range(z.shape[0]):
        dx, dyf, dym, dyv = step_bounds(model, raw, x, dx, z[k], e[k], xf[k])
        x = xf[k]
        for o, v in zip(out, (dx, dyf, dym, dyv)):
            o.append(v)
    return tuple(np.array(o) for o in out)


# ---- closed-form laws (equal weights, iid starting cloud) ----------------------------------------------------------------------
def lg_law(raw, m0, P0, k):
    """(mean, variance) of x_{T+k} for x_T ~ N(m0, P0) under the LG1D row"""
    A, _, Q = raw[:3]
    return A ** k * m0, A ** (2 * k) * P0 + Q * sum(A ** (2 * j) for j in range(k))


def within_se(stat, expect, se, nse=5.0):
    """|stat - expect| in units of nse standard errors: <= 1 passes"""
    return abs(stat - expect) / (nse * se)
