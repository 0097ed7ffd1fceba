"""The step of the marginal (Rao-Blackwellised) UCSV family (include/smc_hip.h "marginal UCSV") restated in numpy's longdouble,
and the error bounds the binary64 specification is allowed against it.  TEST INFRASTRUCTURE: nothing here is used by the library.

State (m, lse, lsn, P), parameter row (g_eps, g_eta, x0, lse0, lsn0), two normals (z0, z1), observation y:
    (m, a, b, P-) = first ? (x0, lse0, lsn0, exp(lse0)) : (m, lse, lsn, P + exp(lse))
    lse' = a + g_eps z0,  lsn' = b + g_eta z1,  R = exp(lsn'),  S = P- + R,  e = y - m
    logw = log N(y; m, S),  K = P- / S,  m' = m + K e,  P' = P- R / S
(kalman_filter.jl:39-51 with A = B = 1, Q = exp(a), R = exp(lsn'); ssm.jl:233-259 for the volatilities and the first step.)

Error bounds, in the manner of guided_reference.py: u = 2^-52 is charged for every rounded operation, 2u relative for every sp_exp,
2 ulp of the result for sp_log; propagated through the order of operations smc_spec.h states (model_marginal_step); derived, not
fitted.  The reference is taken at the lsn' the specification returned (R depends on it), as guided_reference.ucsv_bounds does.
"""
import numpy as np

from guided_reference import LD, U, ld, logn


def vols(raw, sp, z, first):
    """(lse', lsn') in longdouble"""
    a, b = (raw[3], raw[4]) if first else (sp[1], sp[2])
    return LD(raw[0]) * ld(z[0]) + ld(a), LD(raw[1]) * ld(z[1]) + ld(b)


def predict(raw, sp, first):
    """(m, P-) in longdouble"""
    if first:
        return ld(raw[2]), np.exp(ld(raw[3]))
    return ld(sp[0]), ld(sp[3]) + np.exp(ld(sp[1]))


def step(raw, sp, y, first, lsn_new):
    """(m', P', logw) given the new log-volatility of the observation noise"""
    m, Pm = predict(raw, sp, first)
    R = np.exp(ld(lsn_new))
    S = Pm + R
    K = Pm / S
    return m + K * (ld(y) - m), Pm * R / S, logn(y, m, S)


def bounds(raw, sp, z, y, first, s):
    """(bounds on |s[c] - reference| [4], bound on |logw - reference|) for the state s the specification returned"""
    raw, sp, z, s = (np.asarray(v, dtype=float) for v in (raw, sp, z, s))
    m, Pm = (float(v) for v in predict(raw, sp, first))
    Q = float(np.exp(ld(raw[3] if first else sp[1])))
    R = float(np.exp(ld(s[2])))
    S = Pm + R
    K = Pm / S
    e = float(y) - m
    # Q: 2u; P- = P + Q: + one rounding (first step: Q itself)
    dPm = 2 * U * Q + (0.0 if first else U * Pm)
    # R: 2u; S: the two operands' errors and one rounding; 1 / S: one more
    rS = (dPm + 2 * U * R) / S + U
    # K = P- (1 / S): P-, 1 / S (rS + u), the product
    rK = dPm / Pm + rS + 2 * U
    # m' = fma(K, e, m): e = y - m rounded (u), K (rK), one rounding of the sum
    bm = abs(K * e) * (rK + U) + U * abs(s[0])
    # P' = min(K R, P-): K (rK), R (2u), the product; the minimum with P- moves it by no more than P-'s own error
    bP = abs(s[3]) * (rK + 3 * U) + dPm
    # logw = fma(-0.5 (e / S), e, fma(-0.5, log S, -c0)): e twice (2u), 1 / S (rS + u), two products (2u); log S: the error of S and
    # 2 ulp of sp_log; the inner fma rounds c, the outer the sum
    quad = 0.5 * e * e / S
    logS = abs(np.log(S))
    c = 0.5 * logS + 0.5 * np.log(2 * np.pi)
    blw = quad * (rS + 5 * U) + 0.5 * (rS + 2 * U * logS) + U * c + U * (quad + c)
    return np.array([bm, U * abs(s[1]), U * abs(s[2]), bP]), blw
