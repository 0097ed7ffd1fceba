"""CPU tests of the IBIS sampler's host side: the public surface (no GPU needed to construct), and the CPU restatement of
src/ibis.jl (tests/ibis_reference.py) that the GPU tests compare against bit for bit - pinned here against an exact posterior."""
import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from ibis_reference import IbisReference, case_one_parameter, case_readme, grid_posterior_A, LG_TRUE, Y_SEED

K_SEEDS = 16


def _y(T=100):
    return smc.simulate(smc.UnivariateLinearGaussian(**LG_TRUE), T, seed=Y_SEED)[1]


def test_ibis_api_surface():
    """smc.IBIS constructs without a GPU (no device call before the first sampler call) with the cloud SMC draws for the same
    seed; what a GPU cannot evaluate is refused with a TypeError that says why."""
    tmap, prior, model = case_readme(smc)
    ib = smc.IBIS(512, model, prior, 3, 0.5, seed=7, theta_map=tmap)
    s = smc.SMC(64, 512, model, prior, 3, 0.5, seed=7, theta_map=tmap)
    assert ib._h is None and np.array_equal(ib.theta, s.theta)
    assert ib.ess == 512.0 and ib.ess_min == 256.0 and ib.acc_ratio == 0.0 and ib.t == 0
    assert np.array_equal(ib.x, np.zeros(512)) and np.array_equal(ib.Sigma, np.ones(512)) and np.array_equal(ib.logZ, np.zeros(512))
    assert np.array_equal(ib.omega, np.full(512, 1.0 / 512))
    # a bare one-component prior is a prior too
    one = smc.IBIS(16, None, smc.TruncatedNormal(0, 1, -1, 1), 2, 0.5, theta_map=case_one_parameter(smc)[0])
    assert one.theta.shape == (16, 1)
    with pytest.raises(TypeError, match="LG1D"):
        smc.IBIS(16, model, prior, 3, 0.5, theta_map=smc.ThetaMap(3, [0, 0, 1, 2, 2], [0.0] * 5))
    with pytest.raises(TypeError, match="LG1D"):
        smc.IBIS(16, model, prior, 3, 0.5)

    class Closure:
        def rand(self, rng):
            return np.array([0.1, 1.0, 1.0])
    with pytest.raises(TypeError, match="enumerated"):
        smc.IBIS(16, model, Closure(), 3, 0.5, theta_map=tmap)
    for name in ("smc2", "smc2_step", "smc2_run", "resample_", "rejuvenate_", "expected_parameters", "density_tempered"):
        assert callable(getattr(smc, name))


def test_restatement_recovers_the_exact_posterior():
    """The restatement alone, one-parameter case (theta = A): over K seeds the mean of E[A] is within 4 standard errors of the
    posterior mean computed by quadrature, and every run rejuvenated at least twice (so it is the rejuvenation path that is
    pinned)."""
    y = _y()
    tmap, prior, _ = case_one_parameter(smc)
    mean, sd = grid_posterior_A(y)
    est, nrej = [], []
    for seed in range(1, K_SEEDS + 1):
        r = IbisReference(512, tmap, prior, 3, 0.5, seed=seed).run(y)
        est.append(r.expected_parameters()[0])
        nrej.append(r.n_rejuvenations)
    est = np.array(est)
    se = est.std(ddof=1) / np.sqrt(K_SEEDS)
    print("grid E[A] = %.6f sd = %.6f; restatement mean = %.6f, SE = %.6f, rejuvenations = %s" % (mean, sd, est.mean(), se, nrej))
    assert sum(n >= 2 for n in nrej) == K_SEEDS
    assert abs(est.mean() - mean) <= 4.0 * se


@pytest.mark.parametrize("predict_first", [False, True])
def test_restatement_online_logZ_is_the_whole_series_logZ(ob, predict_first):
    """after the last step logZ[m] equals the whole-series Kalman log-likelihood of theta[m], bit for bit, for both flag values"""
    y = _y()
    tmap, prior, _ = case_readme(smc)
    r = IbisReference(77, tmap, prior, 3, 0.5, seed=3, predict_first=predict_first).run(y)
    assert r.n_rejuvenations >= 2
    for m in range(r.M):
        x, S, z = ob.kalman_log_likelihood(tmap.rows(r.theta[m][None, :])[0], y, predict_first=predict_first)
        assert (x, S, z) == (r.x[m], r.S[m], r.logZ[m])
