"""CPU tests of the host twins of the theta cloud's quantiles and histograms (smc_host_theta_weights, smc_host_theta_quantiles,
smc_host_theta_histogram; csrc/smc_spec.h "quantiles and histograms of the theta cloud") against the numpy restatement of
tests/theta_quantiles_reference.py, compared with ==, and of posterior_quantiles / posterior_histogram where they need no device."""
import math

import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
import theta_quantiles_reference as ref
from ibis_reference import case_readme

SIZES = [1, 2, 63, 64, 65, 515]
DIMS = [1, 3, 8]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def levels_of(theta, logw):
    lo, hi = ref.boundary_levels(L, theta, logw)
    return np.array([0.0, 1.0, 0.5, 0.05, 0.95, lo, hi, 0.25])


def test_weights_are_the_specification():
    """q = rint(p 2^(32 + k - K)) against exact integer arithmetic on exp(logw) to 1 unit (sp_exp_parts is an approximation of
    exp good to a few ulp; the rounding itself is exact), K and W as stated, dead particles 0, W < 2^63 at the largest p"""
    logw = np.array([0.0, -1.0, 3.0, -40.0, -np.inf, np.nan, 8e8, -8e8, 7e8, -25.0, 0.34657359027997264])
    q, K, W = L.host_theta_weights(logw)
    assert q.dtype == np.uint64 and int(q.sum()) == W
    assert K == round(7e8 / math.log(2.0))
    assert [int(v) for v in q[[0, 1, 2, 3, 4, 5, 6, 7, 9, 10]]] == [0] * 10 and int(q[8]) >= 0.707 * 2 ** 32
    q, K, W = L.host_theta_weights(logw[[0, 1, 2, 3, 4, 5, 6, 7, 9, 10]])
    assert K == 4 and [int(q[i]) for i in (4, 5, 6, 7)] == [0, 0, 0, 0]
    for i, l in ((0, 0.0), (1, -1.0), (2, 3.0), (8, -25.0), (9, 0.34657359027997264)):
        assert abs(int(q[i]) - math.exp(l) * 2.0 ** (32 - 4)) <= 1.0 + 1e-14 * 2.0 ** 32, i
    assert int(q[3]) == 0                                    # 2^(32 - 4) exp(-40) < 1 / 2
    # the range of p: logw = (k +- 1/2) ln 2 gives p = 2^(+-1/2), so q <= 1.415 2^32 and 2^30 of them stay below 2^63
    q, K, W = L.host_theta_weights(np.array([0.34657359027997264]))
    assert K == 0 and 1.4142 * 2 ** 32 < int(q[0]) < 1.4143 * 2 ** 32
    assert 1.4143 * 2 ** 32 * 2 ** 30 < 2 ** 63
    q, K, W = L.host_theta_weights(np.array([-np.inf, np.nan]))
    assert K == -(1 << 30) and W == 0 and not q.any()


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("M", SIZES)
def test_quantiles_equal_the_restatement(M, d):
    """every family, eight levels (0, 1, and a pair around a cumulative boundary among them): the twin == sort and cumsum; the
    float-only bound holds; a cloud with one live particle returns its theta at every level, one without any NaN"""
    for name, (theta, logw) in ref.families(M, d, 1000 * M + d).items():
        p = levels_of(theta, logw)
        out = L.host_theta_quantiles(theta, logw, p)
        want = ref.quantiles(L, theta, logw, p)
        assert same(out, want), name
        q, _, W = L.host_theta_weights(logw)
        if name == "none":
            assert W == 0 and np.isnan(out).all()
            continue
        live = q > 0
        for i in range(d):
            assert np.isin(ref.order_key(out[i]), ref.order_key(theta[live, i])).all(), name      # a value of a particle that carries weight
            assert np.all(np.diff(ref.order_key(out[i][[0, 3, 7, 2, 4, 1]]).astype(object)) >= 0)       # monotone in p
            for j in range(p.size):
                ok, what = ref.float_bounds(theta[:, i], logw, p[j], out[i, j])
                assert ok, (name, i, j, what)
        if name == "one":
            assert same(out, np.repeat(theta[M // 2][:, None], p.size, axis=1))
        # one level at a time gives the same column
        assert same(L.host_theta_quantiles(theta, logw, p[5:6]), out[:, 5:6])


@pytest.mark.parametrize("nbins", [1, 7, 256, 4096])
@pytest.mark.parametrize("M", SIZES)
def test_histogram_equals_the_restatement(M, nbins):
    d = 3
    for name, (theta, logw) in ref.families(M, d, 77 * M + nbins).items():
        for comp, (lo, hi) in ((0, (-1.0, 1.5)), (2, (-60.0, 90.0)), (1, (0.9995, 1.0005))):
            theta = theta.copy()
            theta[0, comp], theta[M // 3, comp], theta[M - 1, comp] = lo, lo + (hi - lo) * 3.0 / 7.0, hi      # on lo, on an edge, on hi
            counts, W = L.host_theta_histogram(theta, logw, comp, lo, hi, nbins)
            want, wW = ref.histogram(L, theta, logw, comp, lo, hi, nbins)
            assert W == wW and np.array_equal(counts, want), (name, comp)
            assert sum(int(c) for c in counts) == W
            if name == "one":
                assert sorted(int(c) for c in counts)[-1] == W and np.count_nonzero(counts) == 1
            if name == "none":
                assert W == 0 and not counts.any()
    # the edge rules on their own: lo is inside, hi is over, NaN has its slot, -0.0 at lo = 0.0 is inside
    theta = np.array([[0.0], [-0.0], [1.0], [np.nextafter(1.0, 0.0)], [np.nan], [-1e-300], [np.inf], [-np.inf]])
    counts, W = L.host_theta_histogram(theta, np.zeros(8), 0, 0.0, 1.0, 4)
    u = W // 8
    assert [int(c) for c in counts] == [2 * u, 2 * u, 0, 0, u, 2 * u, u]


def test_invalid_arguments():
    theta, logw = np.zeros((4, 2)), np.zeros(4)
    for bad in ([], [0.5] * 9, [-1e-9], [1.0000001], [np.nan]):
        with pytest.raises(L.SmcError):
            L.host_theta_quantiles(theta, logw, bad)
    for comp, lo, hi, nbins in ((-1, 0.0, 1.0, 4), (2, 0.0, 1.0, 4), (0, 0.0, 1.0, 0), (0, 0.0, 1.0, 4097), (0, 1.0, 1.0, 4), (0, 2.0, 1.0, 4),
                                (0, -np.inf, 1.0, 4), (0, 0.0, np.inf, 4), (0, np.nan, 1.0, 4), (0, 0.0, np.nan, 4), (0, -1e308, 1e308, 4)):
        with pytest.raises(L.SmcError):
            L.host_theta_histogram(theta, logw, comp, lo, hi, nbins)
    lib = L.lib()
    assert lib.smc_host_theta_quantiles(None, None, 4, 2, None, 1, None) != 0
    assert lib.smc_host_theta_histogram(None, None, 4, 2, 0, 0.0, 1.0, 4, None, None) != 0
    assert lib.smc_host_theta_weights(None, 4, None, None, None) != 0
    assert lib.smc_ibis_theta_quantiles(None, None, 1, None) != 0 and lib.smc_ibis_theta_histogram(None, 0, 0.0, 1.0, 4, None, None) != 0


def test_python_functions_without_a_device():
    """an IBIS before its first sampler call: the host twin over the initial cloud with equal weights; shapes of the results"""
    tmap, prior, model = case_readme(smc)
    ib = smc.IBIS(77, model, prior, 3, 0.5, seed=7, theta_map=tmap)
    med = smc.posterior_quantiles(ib, 0.5)
    assert ib._h is None and med.shape == (3,)
    q = smc.posterior_quantiles(ib, [0.05, 0.5, 0.95])
    assert q.shape == (3, 3) and np.array_equal(q[:, 1], med)
    assert same(q, ref.quantiles(L, ib.theta, np.zeros(77), [0.05, 0.5, 0.95]))
    # equal weights: the value of rank floor(77 p) of the sorted column
    assert np.array_equal(med, np.sort(ib.theta, axis=0)[38])
    many = smc.posterior_quantiles(ib, np.linspace(0.0, 1.0, 11))
    assert many.shape == (3, 11) and np.array_equal(many[:, 0], ib.theta.min(axis=0)) and np.array_equal(many[:, -1], ib.theta.max(axis=0))
    hists = smc.posterior_histogram(ib)
    assert len(hists) == 3
    for c, (mass, edges) in enumerate(hists):
        lo, hi = ib.theta[:, c].min(), np.nextafter(ib.theta[:, c].max(), np.inf)
        assert mass.shape == (50,) and np.array_equal(edges, np.linspace(lo, hi, 51))
        assert abs(mass.sum() - 1.0) < 1e-12 and mass[0] > 0.0 and mass[-1] > 0.0
    mass, edges, (under, over, nan) = smc.posterior_histogram(ib, 1, bins=7, range=(0.5, 2.0), outside=True)
    col = ib.theta[:, 1]
    assert np.array_equal(edges, np.linspace(0.5, 2.0, 8)) and abs(mass.sum() + under + over + nan - 1.0) < 1e-12
    assert abs(under - np.mean(col < 0.5)) < 1e-9 and abs(over - np.mean(col >= 2.0)) < 1e-9 and nan == 0.0
    want = np.histogram(col, bins=7, range=(0.5, 2.0))[0] / 77.0
    assert np.allclose(mass, want, atol=2.0 / 77.0)         # (numpy closes the last bin on the right; the bins' arithmetic differs in the last bit)
    with pytest.raises(TypeError):
        smc.posterior_quantiles(object(), 0.5)
    with pytest.raises(ValueError):
        smc.posterior_histogram(ib, 3)


def test_single_value_cloud_and_host_sampler():
    """all the weight on one value: range = (v - 0.5, v + 0.5) and one bin holds everything; an SMC built on the host: the twin
    over smc.theta and log(smc.omega)"""

    class Cloud:                                             # what the functions read of an SMC sampler
        def __init__(self, theta, omega):
            self.theta, self.omega = theta, omega

    theta = np.array([[1.0, 5.0], [2.2, 5.0], [3.0, 5.0], [4.0, 5.0]])
    omega = np.array([0.1, 0.2, 0.0, 0.7])
    from sequential_monte_carlo_amd import smc_samplers
    calls = smc_samplers._host_cloud_calls(Cloud(theta, omega))
    from sequential_monte_carlo_amd import ibis as _ibis
    q = _ibis.quantiles_from(calls[0], [0.0, 0.09, 0.11, 0.31, 1.0])
    assert np.array_equal(q[0], [1.0, 1.0, 2.2, 4.0, 4.0]) and np.array_equal(q[1], [5.0] * 5)       # the particle of weight 0 never appears
    mass, edges = _ibis.histogram_from(*calls, component=1, bins=4)
    assert np.array_equal(edges, np.linspace(4.5, 5.5, 5)) and np.array_equal(mass, [0.0, 0.0, 1.0, 0.0])
    mass, edges = _ibis.histogram_from(*calls, component=0, bins=3)
    assert np.array_equal(edges, np.linspace(1.0, np.nextafter(4.0, np.inf), 4)) and np.allclose(mass, [0.1, 0.2, 0.7], atol=1e-9)
    with pytest.raises(ValueError):
        _ibis.histogram_from(*smc_samplers._host_cloud_calls(Cloud(theta, np.zeros(4))), component=0)
    # a real SMC sampler over the CPU oracle backend (no device): weighted after one smc2 call
    from oracle_backend import OracleBackend
    from ibis_reference import LG_TRUE, Y_SEED
    tmap, prior, model = case_readme(smc)
    y = smc.simulate(smc.UnivariateLinearGaussian(**LG_TRUE), 8, seed=Y_SEED)[1]
    s = smc.SMC(16, 16, model, prior, 2, 0.6, seed=22, backend=OracleBackend(), theta_map=tmap)
    smc.smc2(s, y)
    assert np.unique(s.omega).size > 8
    with np.errstate(divide="ignore"):
        logw = np.log(s.omega)
    p = [0.1, 0.5, 0.9]
    assert same(smc.posterior_quantiles(s, p), ref.quantiles(L, s.theta, logw, p))
    assert same(smc.posterior_quantiles(s, 0.5), ref.quantiles(L, s.theta, logw, [0.5])[:, 0])
    mass, edges = smc.posterior_histogram(s, 0, bins=4)
    counts, W = ref.histogram(L, s.theta, logw, 0, edges[0], edges[-1], 4)
    assert edges[0] == s.theta[:, 0].min() and edges[-1] == np.nextafter(s.theta[:, 0].max(), np.inf)
    assert np.array_equal(mass, counts[1:-2] / float(W)) and abs(mass.sum() - 1.0) < 1e-12
