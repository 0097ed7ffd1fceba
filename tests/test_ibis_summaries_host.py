"""CPU tests of the IBIS summaries (observation_dist, estimated_trend, quantile, filtered_state; plotting_utils.jl:94-137): the
host twin of the device reduction (smc_host_ibis_summary, csrc/smc_spec.h "summaries of an IBIS cloud") against an exactly
rounded restatement (tests/ibis_summary_reference.py), and the Python surface before any device call."""
import math
import statistics

import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
import ibis_summary_reference as ref
from ibis_reference import case_one_parameter, case_readme

EPS = 2.0 ** -52


def _check(got, s):
    """the bounds of test_host_twin_against_exact_sums"""
    for name, i, mag in (("y", 0, "abs_y"), ("Sigma", 1, "abs_Sigma"), ("xbar", 3, "abs_xbar"), ("Sbar", 4, "abs_Sbar")):
        err, tol = abs(got[i] - s[name]), 64 * EPS * s[mag]
        print("%-9s %.17g  exact %.17g  err %.3g  tol %.3g" % (name, got[i], s[name], err, tol))
        assert err <= tol, name
    for name, i, mean, dev in (("between", 2, "y", "dev_y"), ("between_x", 5, "xbar", "dev_x")):
        err, tol = abs(got[i] - s[name]), 64 * EPS * (s[name] + 2.0 * abs(s[mean]) * s[dev])
        print("%-9s %.17g  exact %.17g  err %.3g  tol %.3g" % (name, got[i], s[name], err, tol))
        assert err <= tol, name


@pytest.mark.parametrize("ahead", [0, 1])
@pytest.mark.parametrize("M", ref.SIZES)
@pytest.mark.parametrize("shape", sorted(ref.CLOUDS))
def test_host_twin_against_exact_sums(shape, M, ahead):
    """smc_host_ibis_summary against math.fsum over the same cloud.  The tolerance is derived, not tuned: a fixed-order tree
    sum of M terms has relative error at most about (log2 M + c) eps of sum |terms| (the chunks' trees are 6 levels deep; the
    left-to-right pass over the M / 64 chunk sums adds errors that grow like the square root of their number); the weights
    carry a few ulp from exp and the normalisation.
    So for y, Sigma, xbar, Sbar:  |host - fsum| <= 64 eps sum omega_m |term_m|.
    between = sum omega (ym - y)^2 inherits the error of y twice - d/dy of it is -2 sum omega (ym - y), term by term of
    magnitude 2 |ym - y| times the error eps |y| of y - so it is allowed
    64 eps (sum omega (ym - y)^2 + 2 |y| sum omega |ym - y|), and between_x likewise in x."""
    rows, x, S, logw = ref.CLOUDS[shape](M, 11 * M + ahead)
    _check(L.host_ibis_summary(rows, x, S, logw, ahead), ref.summary(rows, x, S, logw, ahead))


@pytest.mark.parametrize("ahead", [0, 1])
def test_equal_weights(ahead):
    """all logw equal (to any common value): the plain means"""
    rows, x, S, _ = ref.random_cloud(4099, 5)
    for c in (0.0, -731.25, 1e6):
        logw = np.full(4099, c)
        got = L.host_ibis_summary(rows, x, S, logw, ahead)
        _check(got, ref.summary(rows, x, S, logw, ahead))
        assert np.isfinite(got).all()
    ym, vm = ref.components(rows, x, S, ahead)
    assert got[0] == pytest.approx(ym.mean(), rel=1e-13) and got[1] == pytest.approx(vm.mean(), rel=1e-13)


@pytest.mark.parametrize("others", [-np.inf, -5000.0])
@pytest.mark.parametrize("M,at", [(1, 0), (9, 8), (4099, 77), (4099, 4098)])
def test_one_particle_holds_all_the_weight(M, at, others):
    """one particle with all the weight (the others at -inf, or so far below that exp underflows): y and Sigma are that
    particle's ym and vm, and between is exactly 0"""
    rows, x, S, _ = ref.random_cloud(M, 3)
    logw = np.full(M, others)
    logw[at] = 2.5
    for ahead in (0, 1):
        got = L.host_ibis_summary(rows, x, S, logw, ahead)
        ym, vm = ref.components(rows, x, S, ahead)
        assert got[0] == ym[at] and got[2] == 0.0 and got[3] == x[at] and got[5] == 0.0
        assert got[1] == pytest.approx(vm[at], rel=4 * EPS) and got[4] == pytest.approx(S[at], rel=4 * EPS)


def test_out_of_support_particles_contribute_nothing():
    """logw = -inf (or NaN) takes a particle out even when its x is NaN or infinite - the rule of _integrate of SMC; the result
    is, bit for bit, that of the cloud with those particles' state replaced by anything else"""
    rows, x, S, logw = ref.random_cloud(4099, 8)
    dead = np.random.default_rng(1).choice(4099, 700, replace=False)
    logw[dead[:600]] = -np.inf
    logw[dead[600:]] = np.nan
    x2, S2 = x.copy(), S.copy()
    x2[dead[::2]], S2[dead[::3]] = np.nan, np.inf
    for ahead in (0, 1):
        a, b = L.host_ibis_summary(rows, x, S, logw, ahead), L.host_ibis_summary(rows, x2, S2, logw, ahead)
        assert np.isfinite(b[:6]).all() and np.array_equal(a, b)
        _check(b, ref.summary(rows, x, S, logw, ahead))
    # a cloud without a live particle has no summary: NaN, not an exception
    none = L.host_ibis_summary(rows, x, S, np.full(4099, -np.inf), 0)
    assert np.isnan(none[:6]).all() and none[6] == -np.inf and none[7] == 0.0


def test_result_does_not_depend_on_the_common_level_of_logw():
    """shifting every logw by a multiple of ln 2 that is exact in binary64 changes K and nothing else"""
    rows, x, S, logw = ref.random_cloud(512, 2)
    logw = np.round(logw * 8) / 8
    a, b = L.host_ibis_summary(rows, x, S, logw, 1), L.host_ibis_summary(rows, x, S, logw + 0.0, 1)
    assert np.array_equal(a, b)


def _initial(case, M=512, seed=7):
    tmap, prior, model = case(smc)
    return smc.IBIS(M, model, prior, 3, 0.5, seed=seed, theta_map=tmap), tmap


def test_api_before_any_device_call():
    """on the initial cloud every summary comes from the host twin: no handle is created"""
    ib, tmap = _initial(case_readme)
    rows = tmap.rows(ib.theta)
    for ahead in (0, 1):
        s = ref.summary(rows, rows[:, 4], rows[:, 5], np.zeros(512), ahead)
        y, Sig, btw = smc.observation_dist(ib, ahead=ahead, between=True)
        assert (y, Sig) == smc.observation_dist(ib, ahead=ahead)
        got = np.array([y, Sig, btw, *smc.filtered_state(ib)])
        _check(got, s)
    assert smc.filtered_state(ib) == (0.0, 1.0, 0.0)          # x0 = 0, sigma0 = 1 for every particle
    assert ib._h is None and ib.summary_trace == []
    with pytest.raises(ValueError):
        smc.observation_dist(ib, ahead=2)


def test_estimated_trend_dispatch():
    ib, _ = _initial(case_one_parameter)
    ib._theta0[:, 0] = np.linspace(-0.9, 0.9, 512)
    ib.theta_map = smc.ThetaMap(1, [0, -1, -1, -1, -1, -1], [0.0, 1.0, 0.9, 0.8, 2.0, 1.0])     # x0 = 2: a trend to report
    assert smc.estimated_trend(ib) == smc.observation_dist(ib)[0] == 2.0
    assert smc.observation_dist(ib, ahead=1)[0] == pytest.approx(0.0, abs=1e-15)                 # E[A] = 0 on this grid
    for f in (smc.observation_dist, smc.filtered_state, lambda s: smc.quantile(s, [0.5])):
        with pytest.raises(TypeError):
            f(object())
    assert ib._h is None


def test_quantile_is_the_normal_quantile_and_leaves_p_alone():
    ib, tmap = _initial(case_readme)
    p = [0.9, 0.1, 0.5]
    for ahead in (0, 1):
        y, Sig, btw = smc.observation_dist(ib, ahead=ahead, between=True)
        q = smc.quantile(ib, p, ahead=ahead)
        assert p == [0.9, 0.1, 0.5]
        assert np.array_equal(q, [statistics.NormalDist(y, math.sqrt(Sig)).inv_cdf(v) for v in (0.1, 0.5, 0.9)])
        qt = smc.quantile(ib, np.array(p), ahead=ahead, total=True)
        assert np.array_equal(qt, [statistics.NormalDist(y, math.sqrt(Sig + btw)).inv_cdf(v) for v in (0.1, 0.5, 0.9)])
    rows = tmap.rows(ib.theta)
    assert smc.quantile(ib, p) == pytest.approx(ref.quantile(rows, rows[:, 4], rows[:, 5], np.zeros(512), p), rel=1e-13)
    assert isinstance(smc.quantile(ib, 0.5), float) and smc.quantile(ib, 0.5) == smc.observation_dist(ib)[0]
    assert smc.quantile(ib, [0.0, 1.0]).tolist() == [-math.inf, math.inf]
    with pytest.raises(ValueError):
        smc.quantile(ib, [1.5])
    assert ib._h is None
