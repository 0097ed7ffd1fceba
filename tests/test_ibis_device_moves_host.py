"""CPU tests of the host halves of the IBIS sampler's device moves: smc_host_rw_factor_cov (the tail split off
smc_host_rw_factor) and smc_host_theta_moments (the host twin of smc_ibis_theta_moments) against restatements in plain Python
floats, compared with ==, and the twin against exactly rounded sums within the bounds stated for smc_get_moments."""
import math
from fractions import Fraction

import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from ibis_reference import case_readme

MEAN_REL, MEAN_SD, VAR_REL, VAR_LEVEL = 1e-11, 1e-12, 1e-9, 1e-11      # include/smc_hip.h, smc_get_moments
COV_REL, COV_LEVEL = 1e-9, 1e-22                                       # off-diagonal: 1e-9 sqrt(v_i v_j) + 1e-22 |m_i m_j|
CHUNK = 64
INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
RNE = 1.5 * 2.0 ** 52                                                  # (v + RNE) - RNE: round to the nearest integer


# ---- smc_host_rw_factor_cov -------------------------------------------------------------------------------------------------
def py_rw_factor_cov(cov):
    """the operation order of smc_host_rw_factor_cov in Python floats (no fused operation anywhere) -> (L or None, univariate)"""
    d = len(cov)
    fro = 0.0
    for i in range(d):
        for j in range(d):
            fro = fro + cov[i][j] * cov[i][j]
    collapsed = math.sqrt(fro) < 1e-8
    dth = 2.83 * 2.83
    if d == 1:
        return [[1e-2 if collapsed else dth * cov[0][0] + 1e-10]], True
    S = [[((1e-2 if i == j else 0.0) if collapsed else (dth / float(d)) * cov[i][j] + (1e-10 if i == j else 0.0)) for j in range(d)]
         for i in range(d)]
    Lm = [[0.0] * d for _ in range(d)]
    for j in range(d):
        s = S[j][j]
        for k in range(j):
            s = s - Lm[j][k] * Lm[j][k]
        if not s > 0.0:
            return None, False
        ljj = math.sqrt(s)
        Lm[j][j] = ljj
        for i in range(j + 1, d):
            t = S[i][j]
            for k in range(j):
                t = t - Lm[i][k] * Lm[j][k]
            Lm[i][j] = t / ljj
    return Lm, False


def _spd(d, seed, scale=1.0):
    g = np.random.default_rng(seed).normal(size=(d + 3, d))
    return scale * (g.T @ g) / (d + 3)


@pytest.mark.parametrize("d", [1, 2, 3, 8])
@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e-12])          # the last one: a collapsed cloud, norm(cov) < 1e-8
def test_rw_factor_cov_equals_restatement(L, d, scale):
    cov = _spd(d, 10 + d, scale)
    if scale == 1e-12:
        assert math.sqrt(float((cov * cov).sum())) < 1e-8
    got, uni = L.host_rw_factor_cov(cov)
    ref, runi = py_rw_factor_cov(cov.tolist())
    assert uni == runi == (d == 1)
    assert got.tolist() == ref
    if scale == 1e-12:
        assert got.tolist() == (np.eye(d) * (1e-2 if d == 1 else 0.1)).tolist()      # 1e-2 I, or its factor


def test_rw_factor_cov_not_positive_definite_is_an_error(L):
    cov = np.array([[1.0, 2.0], [2.0, 1.0]])
    assert py_rw_factor_cov(cov.tolist())[0] is None
    with pytest.raises(L.SmcError, match="positive definite"):
        L.host_rw_factor_cov(cov)
    assert L.host_rw_factor_cov(np.eye(2))[0].tolist() == py_rw_factor_cov(np.eye(2).tolist())[0]      # the library goes on


def _serial_cov(theta):
    """the covariance smc_host_rw_factor takes: means and centred products summed in index order, in Python floats"""
    n, d = len(theta), len(theta[0])
    mean = []
    for i in range(d):
        s = 0.0
        for m in range(n):
            s = s + theta[m][i]
        mean.append(s / float(n))
    cov = [[0.0] * d for _ in range(d)]
    for i in range(d):
        for j in range(i + 1):
            s = 0.0
            for m in range(n):
                s = s + (theta[m][i] - mean[i]) * (theta[m][j] - mean[j])
            cov[i][j] = cov[j][i] = s / float(n - 1)
    return cov


@pytest.mark.parametrize("n,d,seed", [(2, 1, 1), (77, 1, 2), (100, 2, 3), (513, 3, 4), (64, 8, 5)])
def test_rw_factor_is_the_serial_covariance_through_the_tail(L, n, d, seed):
    """smc_host_rw_factor returns what it returned before the split: its index-order covariance, then the tail"""
    theta = np.random.default_rng(seed).normal(0.3, 2.0, size=(n, d))
    got, uni = L.host_rw_factor(theta)
    ref, runi = py_rw_factor_cov(_serial_cov(theta.tolist()))
    assert uni == runi and got.tolist() == ref
    via, _ = L.host_rw_factor_cov(np.array(_serial_cov(theta.tolist())))
    assert via.tolist() == ref
    same = np.tile(theta[:1], (n, 1))                                   # a cloud of copies: the collapse rule
    assert L.host_rw_factor(same)[0].tolist() == py_rw_factor_cov(_serial_cov(same.tolist()))[0]


# ---- smc_host_theta_moments -------------------------------------------------------------------------------------------------
def _alive(l):
    return l == l and abs(l) <= 7e8


def _cloud_sum(vals):
    """chunks of 64 (padded with +0.0), the butterfly tree within the chunk, the chunks left to right from 0.0"""
    acc = 0.0
    for c in range(0, len(vals), CHUNK):
        t = list(vals[c:c + CHUNK]) + [0.0] * (CHUNK - len(vals[c:c + CHUNK]))
        s = 1
        while s < CHUNK:
            for l in range(0, CHUNK, 2 * s):
                t[l] = t[l] + t[l + s]
            s *= 2
        acc = acc + t[0]
    return acc


def py_theta_moments(L, theta, logw, weighted):
    """smc_spec.h "moments of the theta cloud" in Python floats.  exp(logw) = p 2^k comes from the library's sp_exp (an exact
    scaling of p by 2^k), with k = rint(logw / ln 2) restated here: u = p 2^(k - K) = ldexp(sp_exp(logw), -K)."""
    M, d = len(theta), len(theta[0])
    nan = math.nan
    if weighted:
        k = [int((l * INV_LN2 + RNE) - RNE) if _alive(l) else None for l in logw]
        live = [v for v in k if v is not None]
        K = max(live) if live else 0
        u = [math.ldexp(L.lib().smc_host_exp(l), -K) if (kk is not None and kk - K > -960) else 0.0 for l, kk in zip(logw, k)]
        W = _cloud_sum(u)
        c = [v / W if v > 0.0 else 0.0 for v in u]
    else:
        W, c = 1.0, [1.0] * M

    def finish(s, div):
        if not weighted:
            s = s / div if div > 0.0 else nan
        else:
            s = s if W > 0.0 else nan
        return s
    mean = [finish(_cloud_sum([c[m] * theta[m][i] if c[m] > 0.0 else 0.0 for m in range(M)]), float(M)) for i in range(d)]
    cov = [[0.0] * d for _ in range(d)]
    for i in range(d):
        for j in range(i + 1):
            s = _cloud_sum([c[m] * ((theta[m][i] - mean[i]) * (theta[m][j] - mean[j])) if c[m] > 0.0 else 0.0 for m in range(M)])
            cov[i][j] = cov[j][i] = finish(s, float(M - 1))
    return mean, cov


def exact_moments(theta, logw, weighted):
    """exactly rounded moments: rational arithmetic on the doubles, weights exp(logw) taken by math.exp as exact rationals
    (their relative error, 1e-16, is far inside every bound below)"""
    M, d = len(theta), len(theta[0])
    if weighted:
        top = max(l for l in logw if _alive(l))
        w = [Fraction(math.exp(l - top)) if _alive(l) else Fraction(0) for l in logw]
        tot = sum(w)
        w = [v / tot for v in w]
        div = Fraction(1)
    else:
        w = [Fraction(1, M)] * M
        div = Fraction(M - 1, M)
    th = [[Fraction(v) if ww else Fraction(0) for v in row] for row, ww in zip(theta, w)]
    mean = [sum(w[m] * th[m][i] for m in range(M)) for i in range(d)]
    cov = [[sum(w[m] * (th[m][i] - mean[i]) * (th[m][j] - mean[j]) for m in range(M)) / div for j in range(d)] for i in range(d)]
    return [float(v) for v in mean], [[float(v) for v in r] for r in cov]


def _check_bounds(mean, cov, em, ec):
    d = len(em)
    for i in range(d):
        assert abs(mean[i] - em[i]) <= MEAN_REL * abs(em[i]) + MEAN_SD * math.sqrt(ec[i][i]), ("mean", i, mean[i], em[i])
        assert abs(cov[i][i] - ec[i][i]) <= VAR_REL * ec[i][i] + (VAR_LEVEL * em[i]) ** 2, ("var", i, cov[i][i], ec[i][i])
        for j in range(i):
            bound = COV_REL * math.sqrt(ec[i][i] * ec[j][j]) + COV_LEVEL * abs(em[i] * em[j])
            assert abs(cov[i][j] - ec[i][j]) <= bound and cov[i][j] == cov[j][i], ("cov", i, j, cov[i][j], ec[i][j])


def _clouds(M, d, seed):
    rng = np.random.default_rng(seed)
    yield "unit", rng.normal(size=(M, d))
    yield "level", 1e6 + 1e-3 * rng.normal(size=(M, d))            # a level of 1e6 with a spread of 1e-3


@pytest.mark.parametrize("M", [2, 63, 64, 65, 1000])
@pytest.mark.parametrize("d", [1, 3])
def test_theta_moments_unweighted(L, M, d):
    for name, theta in _clouds(M, d, 100 + M + d):
        mean, cov = L.host_theta_moments(theta)
        pm, pc = py_theta_moments(L, theta.tolist(), None, False)
        assert mean.tolist() == pm and cov.tolist() == pc, name
        _check_bounds(mean.tolist(), cov.tolist(), *exact_moments(theta.tolist(), None, False))


@pytest.mark.parametrize("M", [2, 63, 64, 65, 1000])
@pytest.mark.parametrize("d", [1, 3])
def test_theta_moments_weighted(L, M, d):
    rng = np.random.default_rng(200 + M + d)
    for name, theta in _clouds(M, d, 300 + M + d):
        for logw in (np.zeros(M), 30.0 * rng.normal(size=M), rng.normal(size=M) - 600.0):        # (|logw| < 700: the restatement takes p 2^k from sp_exp)
            mean, cov = L.host_theta_moments(theta, logw, weighted=True)
            pm, pc = py_theta_moments(L, theta.tolist(), logw.tolist(), True)
            assert mean.tolist() == pm and cov.tolist() == pc, name
            _check_bounds(mean.tolist(), cov.tolist(), *exact_moments(theta.tolist(), logw.tolist(), True))


@pytest.mark.parametrize("M", [2, 65, 1000])
def test_theta_moments_weighted_edges(L, M):
    """one live particle: mean is its theta exactly and cov exactly 0; dead particles may hold NaN; all dead: NaN"""
    rng = np.random.default_rng(M)
    theta = 1e6 + 1e-3 * rng.normal(size=(M, 3))
    live = M // 2
    logw = np.full(M, -np.inf)
    logw[live] = -3.25
    keep = theta[live].copy()
    theta[np.arange(M) != live] = np.nan
    mean, cov = L.host_theta_moments(theta, logw, weighted=True)
    assert mean.tolist() == keep.tolist() and cov.tolist() == np.zeros((3, 3)).tolist()
    pm, pc = py_theta_moments(L, theta.tolist(), logw.tolist(), True)
    assert mean.tolist() == pm and cov.tolist() == pc
    # a mix: dead entries of every kind hold NaN, the live ones decide
    theta = rng.normal(size=(M, 3))
    logw = rng.normal(size=M)
    dead = np.arange(M) % 3 == 1
    logw[dead] = np.resize([-np.inf, np.nan, 8e8, -8e8], int(dead.sum()))
    theta[dead] = np.nan
    mean, cov = L.host_theta_moments(theta, logw, weighted=True)
    pm, pc = py_theta_moments(L, theta.tolist(), logw.tolist(), True)
    assert mean.tolist() == pm and cov.tolist() == pc and np.isfinite(mean).all()
    _check_bounds(mean.tolist(), cov.tolist(), *exact_moments(np.where(dead[:, None], 0.0, theta).tolist(), logw.tolist(), True))
    mean, cov = L.host_theta_moments(theta, np.full(M, -np.inf), weighted=True)
    assert np.isnan(mean).all() and np.isnan(cov).all()


def test_posterior_moments_before_the_first_sampler_call():
    """no device call: the host twin over the initial cloud with equal weights; device_moves is off unless asked for"""
    tmap, prior, model = case_readme(smc)
    ib = smc.IBIS(77, model, prior, 3, 0.5, seed=7, theta_map=tmap)
    assert ib.device_moves is False and smc.IBIS(8, model, prior, 3, 0.5, theta_map=tmap, device_moves=True).device_moves is True
    mean, cov = smc.posterior_moments(ib)
    assert ib._h is None and mean.shape == (3,) and cov.shape == (3, 3)
    th = ib.theta
    assert np.allclose(mean, th.mean(axis=0), rtol=1e-13) and np.allclose(cov, np.cov(th.T, bias=True), rtol=1e-12)
    assert np.allclose(mean, smc.expected_parameters(ib), rtol=1e-12)
    assert not ib.accepted.any() and ib.accepted.shape == (77,)
    with pytest.raises(TypeError):
        smc.posterior_moments(object())
