"""GPU tests of the quantiles and histograms of the theta cloud (smc_ibis_theta_quantiles, smc_ibis_theta_histogram;
csrc/smc_theta_kernels.h) against their host twins and the numpy restatement of tests/theta_quantiles_reference.py: every array
compared bit for bit.  The handles are filled through smc_ibis_set_theta and smc_ibis_set_logw, so theta and logw are arbitrary.
Shapes: a lone lane, a wave of 64 partial, full and crossed, more than one workgroup, and 773 = 3 x 256 + 5: three workgroups of
the streaming kernels (IBIS_RED_THREADS = 256 particles each) and a ragged tail of 5 in a fourth."""
import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
import ibis2_reference as r2
import theta_quantiles_reference as ref
from ibis_reference import LG_TRUE, Y_SEED, case_readme

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 130, 515, 773]
DIMS = [1, 3, 8]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def scalar_handle(M, d, theta):
    fam = np.full(d, L.PRIOR_NORMAL, dtype=np.int32)
    par = np.tile([0.0, 1.0, 0.0, 0.0, 0.0], (d, 1))
    h = L.IbisHandle(M, d, fam, par, [0, -1, -1, -1, -1, -1], [0.0, 1.0, 0.9, 0.8, 0.0, 1.0])
    h.set_theta(theta)
    return h


def two_state_handle(M, theta):
    """the one-parameter Hodrick-Prescott case of test_gpu_ibis2 (theta = 1 / lambda)"""
    tmap, prior, _ = r2.case_hp_one(smc)
    fam, par = prior.spec()
    h = L.IbisHandle(M, 1, np.atleast_1d(fam), np.atleast_2d(par), tmap.raw_from, tmap.raw_const, seed=7, row_id=L.MODEL_LG2D)
    h.set_theta(theta)
    return h


def levels_of(theta, logw):
    lo, hi = ref.boundary_levels(L, theta, logw)
    return np.array([0.0, 1.0, 0.5, 0.05, 0.95, lo, hi, 0.25])


def check_cloud(h, theta, logw, name):
    """np = 8, 3 and 1 levels of one cloud: the device == the host twin == the restatement"""
    h.set_theta(theta)
    h.set_logw(logw)
    p = levels_of(theta, logw)
    twin = L.host_theta_quantiles(theta, logw, p)
    assert same(twin, ref.quantiles(L, theta, logw, p)), name
    out = h.theta_quantiles(p)
    assert same(out, twin), name
    assert same(h.theta_quantiles(p[[4, 5, 6]]), twin[:, [4, 5, 6]]), name
    assert same(h.theta_quantiles(p[2:3]), twin[:, 2:3]), name
    return out


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("M", SIZES)
def test_quantiles_equal_host_twin(M, d):
    fams = ref.families(M, d, 1000 * M + d)
    h = scalar_handle(M, d, fams["random"][0])
    for name, (theta, logw) in fams.items():
        out = check_cloud(h, theta, logw, name)
        if name == "one":
            assert same(out, np.repeat(theta[M // 2][:, None], 8, axis=1))
        if name == "none":
            assert np.isnan(out).all()
    h.close()


@pytest.mark.parametrize("M", SIZES)
def test_two_state_handle(M):
    fams = ref.families(M, 1, 31 * M)
    h = two_state_handle(M, fams["random"][0])
    for name, (theta, logw) in fams.items():
        check_cloud(h, theta, logw, name)
        counts, W = h.theta_histogram(0, -1.0, 1.5, 7)
        wc, wW = L.host_theta_histogram(theta, logw, 0, -1.0, 1.5, 7)
        assert W == wW and np.array_equal(counts, wc), name
    h.close()


@pytest.mark.parametrize("nbins", [1, 7, 256, 4096])
@pytest.mark.parametrize("M", [1, 65, 773])
def test_histogram_equals_host_twin(M, nbins):
    d = 3
    fams = ref.families(M, d, 77 * M + nbins)
    h = scalar_handle(M, d, fams["random"][0])
    for name, (theta, logw) in fams.items():
        theta = theta.copy()
        ranges = ((0, (-1.0, 1.5)), (2, (-60.0, 90.0)), (1, (0.9995, 1.0005)))
        for comp, (lo, hi) in ranges:
            theta[0, comp], theta[M // 3, comp], theta[M - 1, comp] = lo, lo + (hi - lo) * 3.0 / 7.0, hi      # on lo, on an edge, on hi
        h.set_theta(theta)
        h.set_logw(logw)
        for comp, (lo, hi) in ranges:
            counts, W = h.theta_histogram(comp, lo, hi, nbins)
            wc, wW = L.host_theta_histogram(theta, logw, comp, lo, hi, nbins)
            assert W == wW and np.array_equal(counts, wc), (name, comp)
            rc, rW = ref.histogram(L, theta, logw, comp, lo, hi, nbins)
            assert W == rW and np.array_equal(counts, rc) and sum(int(c) for c in counts) == W, (name, comp)
    h.close()


def test_state_rules_and_handle_untouched():
    """SMC_ESTATE while a window is pending (the message names smc_ibis_commit); after the commit the twin's values for the
    committed logw; a following window gives the bits of a handle that never made the calls"""
    M, d = 515, 3
    theta = ref.families(M, d, 5)["random"][0]
    theta[:, 0] = np.tanh(theta[:, 0])
    theta[:, 1:] = np.exp(0.3 * theta[:, 1:])
    y = smc.simulate(smc.UnivariateLinearGaussian(**LG_TRUE), 12, seed=Y_SEED)[1]
    tmap, prior, _ = case_readme(smc)
    fam, par = prior.spec()
    hs = [L.IbisHandle(M, d, fam, par, tmap.raw_from, tmap.raw_const) for _ in range(2)]
    h, g = hs
    with pytest.raises(L.SmcError, match="smc_ibis_set_theta"):
        h.theta_quantiles([0.5])
    with pytest.raises(L.SmcError, match="smc_ibis_set_theta"):
        h.theta_histogram(0, 0.0, 1.0, 4)
    for hh in hs:
        hh.set_theta(theta)
        hh.window(y[:6])
    for call in (lambda: h.theta_quantiles([0.5]), lambda: h.theta_histogram(0, 0.0, 1.0, 4)):
        with pytest.raises(L.SmcError, match="smc_ibis_commit"):
            call()
    for hh in hs:
        hh.commit(6)
    logw = h.get(logw=True)["logw"]
    assert np.unique(logw).size > M // 2
    p = [0.05, 0.5, 0.95]
    assert same(h.theta_quantiles(p), L.host_theta_quantiles(theta, logw, p))
    counts, W = h.theta_histogram(1, 0.5, 2.0, 50)
    wc, wW = L.host_theta_histogram(theta, logw, 1, 0.5, 2.0, 50)
    assert W == wW and np.array_equal(counts, wc)
    for bad in ([], [0.5] * 9, [-0.1], [np.nan]):
        with pytest.raises(L.SmcError):
            h.theta_quantiles(bad)
    for comp, lo, hi, nbins in ((-1, 0.0, 1.0, 4), (3, 0.0, 1.0, 4), (0, 0.0, 1.0, 0), (0, 0.0, 1.0, 4097), (0, 1.0, 1.0, 4), (0, 0.0, np.inf, 4),
                                (0, np.nan, 1.0, 4)):
        with pytest.raises(L.SmcError):
            h.theta_histogram(comp, lo, hi, nbins)
    ra, rb = h.window(y[6:12], want_lik=True), g.window(y[6:12], want_lik=True)
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
    for hh in hs:
        hh.commit(6)
    sa, sb = (hh.get(theta=True, x=True, S=True, logZ=True, logw=True) for hh in hs)
    for name in sa:
        assert np.array_equal(sa[name], sb[name]), name
    for hh in hs:
        hh.close()


def test_sampler_run_then_resample():
    """the README case with device moves: after resample_ the cloud is uniform with heavy ties; the quantiles equal the restatement
    on ib.theta, and the median lies within the span of the cloud"""
    y = smc.simulate(smc.UnivariateLinearGaussian(**LG_TRUE), 60, seed=Y_SEED)[1]
    tmap, prior, model = case_readme(smc)
    ib = smc.IBIS(512, model, prior, 3, 0.5, seed=5, theta_map=tmap, device_moves=True)
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, len(y), verbose=False)
    p = [0.0, 0.05, 0.5, 0.95, 1.0]
    q = smc.posterior_quantiles(ib, p)
    assert same(q, ref.quantiles(L, ib.theta, ib.logw, p))
    smc.resample_(ib)
    # resample! (ibis.jl:73-84) gathers logw with the particles; the move that follows it is what makes the weights equal.  Both
    # clouds: the gathered one, and the uniform one over the same (heavily tied) theta
    theta, logw = ib.theta, ib._h.get(logw=True)["logw"]
    assert np.unique(theta[:, 0]).size < 512
    assert same(smc.posterior_quantiles(ib, p), ref.quantiles(L, theta, logw, p))
    ib._h.set_logw(np.zeros(512))
    logw = np.zeros(512)
    q = smc.posterior_quantiles(ib, p)
    assert same(q, ref.quantiles(L, theta, logw, p))
    assert np.array_equal(q[:, 2], np.sort(theta, axis=0)[256])          # equal weights: the value of rank floor(512 p)
    assert np.array_equal(q[:, 0], theta.min(axis=0)) and np.array_equal(q[:, -1], theta.max(axis=0))
    med = smc.posterior_quantiles(ib, 0.5)
    assert med.shape == (3,) and np.all(q[:, 0] <= med) and np.all(med <= q[:, -1]) and np.array_equal(med, q[:, 2])
    for c, (mass, edges) in enumerate(smc.posterior_histogram(ib)):
        assert np.array_equal(edges, np.linspace(q[c, 0], np.nextafter(q[c, -1], np.inf), 51)) and abs(mass.sum() - 1.0) < 1e-12
    ib.close()


def test_results_do_not_depend_on_the_launch(monkeypatch):
    """SMC_THETA_GROUPS caps the workgroups of the streaming kernels: 1 (one workgroup strides over the whole cloud), 2 and the
    default give identical bits; so does a run under SMC_RES_NP (which the IBIS kernels do not read)"""
    M, d = 773, 3
    fams = ref.families(M, d, 99)
    h = scalar_handle(M, d, fams["random"][0])
    for name in ("random", "dead", "ties"):
        theta, logw = fams[name]
        h.set_theta(theta)
        h.set_logw(logw)
        p = levels_of(theta, logw)
        monkeypatch.delenv("SMC_THETA_GROUPS", raising=False)
        monkeypatch.delenv("SMC_RES_NP", raising=False)
        base = h.theta_quantiles(p)
        bh = h.theta_histogram(0, -1.0, 1.5, 256)
        assert same(base, L.host_theta_quantiles(theta, logw, p))
        for key, val in (("SMC_THETA_GROUPS", "1"), ("SMC_THETA_GROUPS", "2"), ("SMC_RES_NP", "2")):
            monkeypatch.setenv(key, val)
            assert same(h.theta_quantiles(p), base), (name, key, val)
            ch = h.theta_histogram(0, -1.0, 1.5, 256)
            assert ch[1] == bh[1] and np.array_equal(ch[0], bh[0]), (name, key, val)
            monkeypatch.delenv(key)
    h.close()
