"""The guided particle step (include/smc_hip.h "proposals") restated in numpy's longdouble, and the error bounds the binary64
specification is allowed against it.  TEST INFRASTRUCTURE: nothing here is used by the library.

Definitions (src/particles.jl:72-80 of the reference):
    logw = logpdf(observation(x), y) + logpdf(transition(xp), x) - logpdf(proposal(xp, y), x)
  LG1D   row (c0, c1, c2, s2):  m = c0 + c1 xp + c2 y,  x = m + sqrt(s2) z
         OPTIMAL: D = B^2 Q + R, (0, A R / D, B Q / D, Q R / D)
  UCSV   x[1], x[2] by the transition;  Q = exp(xp[1]), R = exp(x[2]), K = Q / (Q + R)
         x[0] = xp[0] + K (y - xp[0]) + sqrt(K R) z[0],  logw = logN(y; xp[0], Q + R)

Error bounds.  u = 2^-52 is charged for every rounded operation (twice its half-ulp), 2 ulp of the result for every sp_exp and
sp_log (tests/test_oracle.py grants them one ulp against libm, which is itself within one ulp of the truth;
tests/test_host.py pins the host twins to the oracle bit for bit).  The bounds below propagate these through the order of
operations smc_spec.h states; they are derived, not fitted.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -52
HALF_LOG2PI = LD(0.5) * np.log(LD(8) * np.arctan(LD(1)))   # 2 pi = 8 atan 1, in longdouble


def ld(a):
    return np.asarray(a, dtype=LD)


def logn(x, mean, var):
    """log N(x; mean, var) in longdouble"""
    x, mean, var = ld(x), ld(mean), ld(var)
    return -HALF_LOG2PI - LD(0.5) * np.log(var) - LD(0.5) * (x - mean) ** 2 / var


# ---- LG1D ------------------------------------------------------------------------------------
def lg_optimal_row(raw):
    A, B, Q, R = (LD(v) for v in raw[:4])
    D = B * B * Q + R
    return np.array([LD(0), A * R / D, B * Q / D, Q * R / D], dtype=LD)


def lg_mean(par, xp, y):
    c0, c1, c2, _ = (LD(v) for v in par)
    return c0 + c1 * ld(xp) + c2 * ld(y)


def lg_draw(par, xp, z, y):
    return lg_mean(par, xp, y) + np.sqrt(LD(par[3])) * ld(z)


def lg_logw(raw, par, xp, x, y):
    """the three-term log-weight at a given new state x"""
    A, B, Q, R = (LD(v) for v in raw[:4])
    return logn(y, B * ld(x), R) + logn(x, A * ld(xp), Q) - logn(x, lg_mean(par, xp, y), par[3])


def lg_bounds(raw, par, xp, z, y, x):
    """(bound on |x - lg_draw|, bound on |logw - lg_logw(at the x the specification returned)|)"""
    A, B, Q, R = (float(v) for v in raw[:4])
    c0, c1, c2, s2 = (float(v) for v in par)
    xp, z, y, x = (np.asarray(v, dtype=float) for v in (xp, z, y, x))
    ss, sQ, sR = np.sqrt(s2), np.sqrt(Q), np.sqrt(R)
    k = c2 * y + c0
    m = c1 * xp + k
    # k = fma, m = fma: one rounding each; ss = sqrt: one; x = fma: one
    dm = U * (np.abs(k) + np.abs(m))
    bx = dm + U * (np.abs(ss * z) + np.abs(x))
    # z_o = (y - B x) / sR: product B x, difference, reciprocal of a square root (2 roundings), product
    zo = (y - B * x) / sR
    dzo = U * (np.abs(B * x) / sR + 4 * np.abs(zo))
    c_obs = np.abs(0.5 * np.log(2 * np.pi)) + np.abs(np.log(sR))
    lobs = 0.5 * zo * zo + c_obs
    d_lobs = np.abs(zo) * dzo + U * zo * zo + U * (2 * np.abs(np.log(sR)) + 2 * c_obs) + U * lobs
    # zt = (x - A xp) / sQ, zp = (x - m) / ss with the m of the specification (off by dm)
    zt = (x - A * xp) / sQ
    dzt = U * (np.abs(A * xp) / sQ + 4 * np.abs(zt))
    zp = (x - m) / ss
    dzp = dm / ss + 4 * U * np.abs(zp)
    # ((0.5 zp) zp - (0.5 zt) zt) + (log ss - log sQ): products, difference, two sp_log, their difference, the sum
    dc = np.abs(np.log(ss)) + np.abs(np.log(sQ))
    br = 0.5 * zp * zp + 0.5 * zt * zt + dc
    d_br = np.abs(zp) * dzp + np.abs(zt) * dzt + 2 * U * (0.5 * zp * zp + 0.5 * zt * zt) + 2 * U * dc + U * dc + 2 * U * br
    blw = d_lobs + d_br + U * (lobs + br)
    return bx, blw


# ---- UCSV --------------------------------------------------------------------------------------
def ucsv_vols(raw, xp, z):
    g0, g1 = LD(raw[0]), LD(raw[1])
    return g0 * ld(z[1]) + ld(xp[1]), g1 * ld(z[2]) + ld(xp[2])


def ucsv_draw_logw(xp, z0, y, x2):
    """(x[0], logw) given the new log-volatility x2 (the closed form)"""
    Q, R = np.exp(ld(xp[1])), np.exp(ld(x2))
    K = Q / (Q + R)
    x0 = ld(xp[0]) + K * (ld(y) - ld(xp[0])) + np.sqrt(K * R) * ld(z0)
    return x0, logn(y, xp[0], Q + R)


def ucsv_logw_three_terms(xp, x, y):
    """logpdf(observation(x), y) + logpdf(transition(xp), x) - logpdf(proposal(xp, y), x): the volatility factors cancel"""
    Q, R = np.exp(ld(xp[1])), np.exp(ld(x[2]))
    K = Q / (Q + R)
    m = ld(xp[0]) + K * (ld(y) - ld(xp[0]))
    return logn(y, x[0], R) + logn(x[0], xp[0], Q) - logn(x[0], m, K * R)


def ucsv_bounds(raw, xp, z, y, x):
    """(bounds on |x[c] - reference| [3], bound on |logw - reference|), the reference taken at the x[2] returned"""
    xp, z, x = (np.asarray(v, dtype=float) for v in (xp, z, x))
    y = np.asarray(y, dtype=float)
    Q, R = np.exp(xp[1]), np.exp(x[2])
    D = Q + R
    K = Q / D
    e = y - xp[0]
    s = np.sqrt(K * R)
    # Q, R: 2u each; D: +u = 3u; 1/D: 4u; K: 7u; K R: 10u; sqrt: 6u; e: u; K e: 8u (+ the fma's rounding of the sum)
    b0 = 8 * U * np.abs(K * e) + 6 * U * np.abs(s * z[0]) + 2 * U * np.abs(x[0])
    bx = np.array([b0, U * np.abs(x[1]), U * np.abs(x[2])])
    quad = 0.5 * e * e / D
    logD = np.abs(np.log(D))
    c = 0.5 * logD + 0.5 * np.log(2 * np.pi)
    blw = 9 * U * quad + 0.5 * (3 * U + 2 * U * logD) + U * c + U * (quad + c)
    return bx, blw
