"""The unweighted summaries' definition in numpy (test helper, no GPU): Statistics.quantile with its defaults (Hyndman-Fan type 7,
numpy's "linear" method) and the corrected sample variance, as include/smc_hip.h "summary modes" states them.

    h = n*p + (1 - p);  j = clamp(trunc(h), 1, n-1);  g = clamp(h - j, 0, 1);  a = x_(j), b = x_(j+1)  (n == 1: a = b = x_(1))
    q = a + g*(b - a)   (a, b finite; otherwise (1-g)*a + g*b)

in float64, one rounding per operation (numpy scalars do not fuse), on the values sorted by the IEEE total order of their bits.
The result is a pure function of the cloud: the library's numbers are compared with it BIT FOR BIT.

np.quantile is the independent cross-check.  It evaluates the same statistic by another formula (virtual index (n-1) p, lerp), so
the two differ by roundings: cross_bound is  2 n eps |b - a| + 4 eps max(|a|, |b|),  eps = 2^-52 - the rounding of h (of size n)
carried into g, and the two roundings of the last line.

Moments: mean = fsum(x) / n and var = fsum((x - mean)^2) / (n - 1), exactly rounded sums; the tolerances are those of
tests/summary_reference.py with every weight 1/n and the variance rescaled by n / (n - 1)."""
import math

import numpy as np

from summary_reference import check_moments, total_order_key

EPS = 2.0 ** -52


def sort_total(x):
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    return x[np.argsort(total_order_key(x), kind="stable")]


def rank7(n, p):
    """(j, g) of level p among n values: the 1-based rank of a, and the weight of b"""
    n, p = np.float64(n), np.float64(p)
    h = n * p + (np.float64(1.0) - p)
    j = int(np.trunc(h))
    hi = int(n) - 1
    j = hi if j > hi else (1 if j < 1 else j)           # Julia's clamp(x, lo, hi): hi wins (n == 1: j = 0)
    g = h - np.float64(j)
    g = np.float64(1.0) if g > 1.0 else (np.float64(0.0) if g < 0.0 else g)
    return j, g


def neighbours(xs, p):
    """(a, b, g) of level p in the sorted values xs"""
    n = xs.size
    j, g = rank7(n, p)
    if n == 1:
        return xs[0], xs[0], g
    return xs[j - 1], xs[j], g


def quantile7(x, ps):
    """the type-7 quantiles of x at the levels ps, float64 [len(ps)]"""
    xs = sort_total(x)
    out = np.empty(len(ps))
    for i, p in enumerate(ps):
        a, b, g = neighbours(xs, p)
        if np.isfinite(a) and np.isfinite(b):
            out[i] = a + g * (b - a)
        else:
            out[i] = (np.float64(1.0) - g) * a + g * b
    return out


def cross_bound(x, p):
    """the bound of |quantile7 - np.quantile| at level p"""
    xs = sort_total(x)
    a, b, _ = neighbours(xs, p)
    return 2 * xs.size * EPS * abs(b - a) + 4 * EPS * max(abs(a), abs(b))


def sample_moments(x):
    """(mean, corrected variance) with exactly rounded sums; NaN variance for n == 1"""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    n = x.size
    m = math.fsum(x) / n
    e = x - m
    return m, (math.fsum(e * e) / (n - 1) if n > 1 else math.nan)


def check_sample_moments(mean, var, x, ctx=()):
    """mean / corrected variance of the cloud x within the bounds of summary_reference (weights 1/n; variance rescaled)"""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    n = x.size
    if n == 1:
        assert mean == x[0] and math.isnan(var), (mean, var) + tuple(ctx)
        return
    check_moments(mean, var * (n - 1) / n, x, np.full(n, 1.0 / n), ctx)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))
