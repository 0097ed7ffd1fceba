"""The unweighted summaries' host twins (smc_host_quantile7, smc_host_sample_moments; no GPU): bit for bit against the published
definition in numpy (tests/quantile7_reference.py), and the definition itself against np.quantile, which computes the same
statistic independently."""
import math

import numpy as np
import pytest

from quantile7_reference import check_sample_moments, cross_bound, quantile7, same_bits

SIZES = [1, 2, 3, 1000, 1024, 70000]
LEVELS = [0.0, 0.05, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.999, 1.0]


def cloud(kind, n, seed=11):
    r = np.random.default_rng(seed + n)
    if kind.startswith("lg"):                       # an LG-like cloud at a level
        return float(kind[2:]) + r.standard_normal(n)
    if kind == "clusters":                          # a few values, many times each (a cloud after resampling)
        return r.choice(1e8 + np.array([0.0, 1.5e-8, 3e-8, 1.0, 7.0]), size=n)
    if kind == "equal":
        return np.full(n, 0.3)
    if kind == "zeros":                             # -0.0 next to +0.0: the total order tells them apart
        return r.choice(np.array([-0.0, 0.0, -1.0, 1.0]), size=n)
    raise KeyError(kind)


KINDS = ["lg0", "lg1e4", "lg1e8", "lg-1e6", "clusters", "equal", "zeros"]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_host_quantile7_is_the_definition(L, kind, n):
    x = cloud(kind, n)
    q = L.host_quantile7(x, LEVELS)
    ref = quantile7(x, LEVELS)
    assert same_bits(q, ref), (kind, n, q, ref)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_host_quantile7_against_numpy(L, kind, n):
    """np.quantile(x, p), method "linear": |q - np| <= 2 n eps |b - a| + 4 eps max(|a|, |b|)"""
    x = cloud(kind, n)
    q = L.host_quantile7(x, LEVELS)
    ref = np.quantile(x, LEVELS)
    for j, p in enumerate(LEVELS):
        bound = cross_bound(x, p)
        assert abs(q[j] - ref[j]) <= bound, (kind, n, p, q[j], ref[j], abs(q[j] - ref[j]), bound)


def test_host_quantile7_orders_signed_zeros(L):
    """-0.0 sorts below +0.0 (the total order of the bits); the results are those of the definition on that order"""
    for x in ([-1.0, 0.0, -0.0], [-1.0, 0.0, 0.0], [0.0, -0.0, -0.0, 0.0]):
        q = L.host_quantile7(np.array(x), [0.0, 0.5, 1.0])
        assert same_bits(q, quantile7(np.array(x), [0.0, 0.5, 1.0]))
    x = np.array([-1.0, -0.0, 0.0, 5.0])
    q = L.host_quantile7(x, [1.0 / 3.0, 2.0 / 3.0])
    assert same_bits(q, quantile7(x, [1.0 / 3.0, 2.0 / 3.0]))


def test_host_quantile7_rejects_bad_levels(L):
    for p in (-0.1, 1.5, math.nan):
        with pytest.raises(L.SmcError):
            L.host_quantile7([1.0, 2.0], [p])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_host_sample_moments(L, kind, n):
    x = cloud(kind, n)
    m, v = L.host_sample_moments(x)
    check_sample_moments(m, v, x, (kind, n))
