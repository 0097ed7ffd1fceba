"""Exact references of the filtered summaries (test helper, no GPU): StatsBase's uncorrected weighted mean and variance with
exactly rounded sums (math.fsum), and a check of a weighted quantile that does not sort.  Both take the (x, w) doubles
smc_get_state returns - the dense weights the kernels use.

Tolerances (independent of mean^2 / var, which is what the naive sum w x^2 - mean^2 loses):
  mean  |mean - m| <= 1e-11 |m| + 1e-12 sqrt(v)
  var   |var - v|  <= 1e-9 v + (1e-11 |m|)^2       (the second term: a mean off by its own tolerance)
        var >= 0, and finite for a filter that carries weight; NaN mean and var for a collapsed filter (every weight 0)."""
import math

import numpy as np

MEAN_REL, MEAN_SD, VAR_REL, VAR_LEVEL = 1e-11, 1e-12, 1e-9, 1e-11


def ref_moments(x, w):
    """(m, v): m = fsum(w x) / fsum(w), v = fsum(w (x - m)^2) / fsum(w); particles without weight do not enter; NaN without weight"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    k = w != 0
    x, w = x[k], w[k]
    W = math.fsum(w)
    if W == 0:
        return math.nan, math.nan
    m = math.fsum(w * x) / W
    e = x - m
    return m, math.fsum(w * (e * e)) / W


def moment_errors(mean, var, x, w):
    """(|mean - m| / its bound, |var - v| / its bound) - both <= 1 when the moments are right"""
    m, v = ref_moments(x, w)
    return abs(mean - m) / (MEAN_REL * abs(m) + MEAN_SD * math.sqrt(v)), abs(var - v) / (VAR_REL * v + (VAR_LEVEL * m) ** 2)


def check_moments(mean, var, x, w, ctx=()):
    """mean, var of one coordinate of one filter against ref_moments(x, w), within the bounds above"""
    m, v = ref_moments(x, w)
    if math.isnan(m):
        assert math.isnan(mean) and math.isnan(var), ("collapsed filter: NaN moments", mean, var) + tuple(ctx)
        return
    assert math.isfinite(mean) and math.isfinite(var) and var >= 0, (mean, var) + tuple(ctx)
    em, ev = moment_errors(mean, var, x, w)
    assert em <= 1, ("mean", mean, m, abs(mean - m)) + tuple(ctx)
    assert ev <= 1, ("var", var, v, abs(var - v) / max(v, 1e-300)) + tuple(ctx)


def total_order_key(a):
    """IEEE total order of doubles as unsigned integers (-0.0 < +0.0)"""
    b = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def quantile_delta(n, nseg, seg, W):
    """How far the dense-weight masses may stray from the integer weights the quantile is defined in: a
    particle's weight in the segment table, q >> sh, loses less than one table unit, and one unit is below 2^(SH-47) of the total
    (the heaviest particle of the heaviest segment weighs at least 2^(47-SH) units); the target floor(p D) sits within one unit of
    p D; every dense weight carries a rounding of 2^-53.  SH = max(0, ceil(log2(padded n)) - 14)."""
    SH = max(0, int(math.ceil(math.log2(nseg * seg))) - 14)
    return (n + 2) * (2.0 ** (SH - 47) + 2.0 ** -52) * W


def check_quantiles(q, ps, x, w, delta, ctx=()):
    """q[j] is a particle value, the weighted mass strictly below it is <= p W + delta, the mass at or below it >= p W - delta"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    W = math.fsum(w)
    if W == 0:
        assert np.all(np.isnan(q)), ("collapsed filter: NaN quantiles", q) + tuple(ctx)
        return
    k, kq = total_order_key(x), total_order_key(q)
    for j, p in enumerate(ps):
        assert np.any(k == kq[j]), ("not a particle value", p, q[j]) + tuple(ctx)
        below, upto = math.fsum(w[k < kq[j]]), math.fsum(w[k <= kq[j]])
        assert below <= p * W + delta and upto >= p * W - delta, (p, q[j], below, upto, W, delta) + tuple(ctx)
