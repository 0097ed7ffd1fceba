"""GPU tests of the IBIS sampler's device moves (IBIS(..., device_moves=True); csrc/smc_ibis_kernels.h): the ESS walk, the index
draw of resample! and the moments of the theta cloud on the device against their host functions, every array compared with ==.
Shapes: a segment of 8, a wave of 64, a workgroup or a scan tile of 256 partial or crossed, and 2^17 + 5 for the scans that
need more than one workgroup."""
import math

import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
from ibis_reference import LG_TRUE, Y_SEED, case_one_parameter, case_readme, grid_posterior_A
from test_ibis_host import K_SEEDS

pytestmark = pytest.mark.gpu

CASES = {"readme": case_readme, "one": case_one_parameter}
SIZES = [1, 2, 7, 8, 9, 63, 64, 65, 513, 1000, 4099, 2 ** 17 + 5]
SEEDS = [(5 << 20) + 1, 0x9E3779B97F4A7C15]
NAMES = ("theta", "x", "S", "logZ", "logw")


def _y(T=100):
    return smc.simulate(smc.UnivariateLinearGaussian(**LG_TRUE), T, seed=Y_SEED)[1]


def _ibis(case, M, seed, **kw):
    tmap, prior, model = CASES[case](smc)
    return smc.IBIS(M, model, prior, 3, 0.5, seed=seed, theta_map=tmap, **kw)


def _handle(ib):
    """a fresh handle on the sampler's initial cloud (a twin of ib._handle())"""
    fam, par = ib.prior_spec
    h = L.IbisHandle(ib.M, ib._theta0.shape[1], fam, par, ib.theta_map.raw_from, ib.theta_map.raw_const, seed=ib.seed)
    h.set_theta(ib._theta0)
    return h


def _state(h):
    return h.get(theta=True, x=True, S=True, logZ=True, logw=True)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _same_state(h, g):
    sa, sb = _state(h), _state(g)
    for name in NAMES:
        assert _same(sa[name], sb[name]), name


def logw_patterns(M, rng):
    """the outer log-weights the tests set: name -> logw [M]"""
    nseg = (M + 7) // 8
    seg = np.arange(M) // 8
    out = {"equal": np.zeros(M), "all_dead": np.full(M, -np.inf), "wide": 30.0 * rng.normal(size=M)}
    one = np.full(M, -np.inf)
    one[M // 2] = 0.3
    out["one_live"] = one
    mix = rng.normal(size=M)
    mix[np.arange(M) % 5 == 1] = -np.inf
    mix[np.arange(M) % 7 == 2] = np.nan
    mix[np.arange(M) % 11 == 3] = 8e8
    mix[np.arange(M) % 13 == 4] = -8e8
    out["mix"] = mix
    # groups of segments 43, 58 and 72 binary orders below the first: their shifted sums are small, 0, and 0 by the shift's limit
    out["groups"] = rng.normal(size=M) - np.array([0.0, 30.0, 40.0, 50.0])[seg % 4]
    last = rng.normal(size=M)
    last[seg == nseg - 1] = -np.inf                     # the last segment (short unless 8 | M) entirely dead
    out["dead_tail"] = last
    return out


@pytest.mark.parametrize("M", SIZES)
def test_resample_equals_host_draw_and_permute(M):
    """a_out == host_outer_resample(logw, M, seed) for the logw read from the same handle, and the state after the call == the
    state of a twin after permute(a), for every pattern and two seeds; no live particle: the identity"""
    y = _y(3)
    ib = _ibis("readme", M, 3)
    h, g = _handle(ib), _handle(ib)
    for name, lw in logw_patterns(M, np.random.default_rng(M)).items():
        for seed in SEEDS:
            for hh in (h, g):
                hh.set_theta(ib._theta0)
                hh.window(y)
                hh.commit(3)                              # distinct x, S, logZ per particle
                hh.set_logw(lw)
            logw = h.get(logw=True)["logw"]
            assert _same(logw, lw)
            a = h.resample(seed, want_a=True)
            ref = L.host_outer_resample(logw, M, seed)
            assert np.array_equal(a, ref), (name, seed)
            if name == "all_dead":
                assert np.array_equal(a, np.arange(M))
            if name == "one_live":
                assert np.array_equal(a, np.full(M, M // 2))
            g.permute(ref)
            _same_state(h, g)
    assert h.resample(SEEDS[0]) is None                   # a_out = NULL
    h.close()
    g.close()


@pytest.mark.parametrize("M", SIZES)
def test_window_ess_equals_host_walk(M):
    """(ess, j) == host_outer_walk on the records smc_ibis_window returns for the same state; the state after commit(j) and the
    rows of the summaries of the kept steps are those of the records path; then the same again from the committed state"""
    y = _y(128)
    ib = _ibis("readme", M, 4)
    h, g = _handle(ib), _handle(ib)
    for hh in (h, g):
        hh.set_summaries(True, 0)
    cut = []
    for k in (1, 16, 64):
        for ess_min in (0.0, M / 2.0, M + 1.0):
            for hh in (h, g):
                hh.set_theta(ib._theta0)
            lo = 0
            for _ in range(2):
                ess, j = h.window_ess(y[lo:lo + k], ess_min)
                rec, _ = g.window(y[lo:lo + k])
                ref, jr = L.host_outer_walk(rec, M, ess_min)
                assert j == jr and np.array_equal(ess, ref), (k, ess_min, lo)
                assert j == (1 if ess_min > M else k) or ess_min == M / 2.0
                assert np.array_equal(h.get_summaries(j), g.get_summaries(j), equal_nan=True)
                h.commit(j)
                g.commit(j)
                _same_state(h, g)
                cut.append(0 < j < k)
                lo += j
    assert M < 64 or any(cut)                             # a walk that stops inside a window is among the cases
    h.close()
    g.close()


def _normal_handle(M, d, theta):
    fam = np.full(d, L.PRIOR_NORMAL, dtype=np.int32)
    par = np.tile([0.0, 1.0, 0.0, 0.0, 0.0], (d, 1))
    h = L.IbisHandle(M, d, fam, par, [0, -1, -1, -1, -1, -1], [0.0, 1.0, 0.9, 0.8, 0.0, 1.0])
    h.set_theta(theta)
    return h


@pytest.mark.parametrize("d", [1, 3, 8])
@pytest.mark.parametrize("M", SIZES)
def test_theta_moments_equal_host_twin(M, d):
    """smc_ibis_theta_moments == smc_host_theta_moments on the arrays read back, both modes; dead particles hold NaN; after a
    permute (duplicated rows) again"""
    rng = np.random.default_rng(1000 * d + M)
    theta = 1e3 + rng.normal(size=(M, d))
    pats = logw_patterns(M, rng)
    pats["low"] = rng.normal(size=M) - 1e4               # exp(logw) far below the smallest double: only p 2^k can carry it
    h = _normal_handle(M, d, theta)
    mean, cov = h.theta_moments(weighted=False)
    rm, rc = L.host_theta_moments(theta)
    assert _same(mean, rm) and _same(cov, rc)
    assert M > 1 or np.isnan(cov).all()
    for name, lw in pats.items():
        th = theta.copy()
        alive = np.isfinite(lw) & (np.abs(lw) <= 7e8)
        th[~alive] = np.nan
        h.set_theta(th)
        h.set_logw(lw)
        mean, cov = h.theta_moments(weighted=True)
        rm, rc = L.host_theta_moments(th, lw, weighted=True)
        assert _same(mean, rm) and _same(cov, rc), name
        assert np.isnan(mean).all() == (not alive.any()) and np.isnan(mean).any() == (not alive.any())
        if name == "one_live":
            assert np.array_equal(mean, th[M // 2]) and np.array_equal(cov, np.zeros((d, d)))
    a = np.sort(rng.integers(0, M, size=M)).astype(np.int32)
    h.set_theta(theta)
    h.set_logw(pats["wide"])
    h.permute(a)
    for weighted in (False, True):
        mean, cov = h.theta_moments(weighted=weighted)
        rm, rc = L.host_theta_moments(theta[a], pats["wide"][a], weighted=weighted)
        assert _same(mean, rm) and _same(cov, rc), weighted
    h.close()


@pytest.mark.parametrize("M", [7, 77, 513])
def test_get_moved_equals_the_mask_rejuvenate_returns(M):
    y = _y(20)
    ib = _ibis("readme", M, 6)
    h, g = _handle(ib), _handle(ib)
    with pytest.raises(L.SmcError):
        h.get_moved()                                      # no rejuvenation yet
    Lf, _ = L.host_rw_factor(ib._theta0)
    s = 0.5 * np.arange(3, 0, -1)
    for hh in (h, g):
        hh.window(y[:10])
        hh.commit(10)
    n1, moved = g.rejuvenate(y[:10], 1.0, Lf, s, 99)
    n2, none = h.rejuvenate(y[:10], 1.0, Lf, s, 99, want_moved=False)
    assert none is None and n1 == n2 == int(moved.sum()) and (n1 > 0 or M < 77)
    assert np.array_equal(h.get_moved(), moved)
    _same_state(h, g)
    h.close()
    g.close()


class _Trace:
    """records what every window of a sampler returned, with the number of rejuvenations before it"""

    def __init__(self, monkeypatch):
        self.ess, self.nrej = [], []
        inner = smc.ibis._window

        def window(ibis, y, ess_min, t=None):
            ess, j = inner(ibis, y, ess_min, t)
            self.ess.extend(float(e) for e in ess[:j])
            self.nrej.extend([ibis.n_rejuvenations] * j)
            return ess, j
        monkeypatch.setattr(smc.ibis, "_window", window)


def _hand_driven(ib0, y, window=16):
    """the online run of smc2 + smc2_run(window) with device moves, call by call on a handle, with every device result
    checked against its host function on the arrays read back at that point"""
    M, chain, T = ib0.M, ib0.chain, len(y)
    h = _handle(ib0)
    calls = [0]

    def next_seed():
        calls[0] += 1
        return (ib0.seed << 20) + calls[0]
    trace, nrej, accepted, acc_ratio = [], 0, np.zeros(M, dtype=bool), 0.0
    ess, j = h.window_ess(y[:1], 0.0)
    h.commit(j)
    trace.extend(ess.tolist())
    cur, t = float(ess[0]), 2
    while t <= T:
        if cur < ib0.ess_min:
            logw = h.get(logw=True)["logw"]
            seed = next_seed()
            a = h.resample(seed, want_a=True)
            assert np.array_equal(a, L.host_outer_resample(logw, M, seed))
            theta = h.get(theta=True)["theta"]
            mean, cov = h.theta_moments(weighted=False)
            rm, rc = L.host_theta_moments(theta)
            assert np.array_equal(mean, rm) and np.array_equal(cov, rc)
            # the serial index-order covariance differs by rounding only: each order meets the stated bound against the exact value
            sm = theta.mean(axis=0)
            sc = np.atleast_2d(np.cov(theta.T))
            for i in range(theta.shape[1]):
                assert abs(cov[i, i] - sc[i, i]) <= 2.0 * (1e-9 * sc[i, i] + (1e-11 * sm[i]) ** 2)
            Lf, uni = L.host_rw_factor_cov(cov)
            scales = 0.5 * np.arange(chain, 0, -1)
            n, _ = h.rejuvenate(y[:t - 1], 1.0, Lf, scales * scales if uni else scales, next_seed(), want_moved=False)
            accepted, acc_ratio, nrej = h.get_moved(), float(n) / M, nrej + 1
        k = max(1, min(window, 64, T - t + 1))
        ess, j = h.window_ess(y[t - 1:t - 1 + k], ib0.ess_min)
        h.commit(j)
        trace.extend(ess.tolist())
        cur = float(ess[-1])
        t += j
    st = _state(h)
    h.close()
    return st, trace, nrej, accepted, acc_ratio


@pytest.mark.parametrize("case", ["readme", "one"])
@pytest.mark.parametrize("M", [77, 512])
def test_online_run_with_device_moves(case, M, monkeypatch):
    y = _y(100)
    st, trace, nrej, accepted, acc_ratio = _hand_driven(_ibis(case, M, 5), y)
    assert nrej >= 2
    tr = _Trace(monkeypatch)
    ib = _ibis(case, M, 5, device_moves=True)
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, len(y), verbose=False)
    assert ib.t == len(y) and ib.n_rejuvenations == nrej and tr.ess == trace and ib.ess == trace[-1]
    for name, attr in zip(NAMES, ("theta", "x", "Sigma", "logZ", "logw")):
        assert np.array_equal(getattr(ib, attr), st[name]), name
    assert np.array_equal(ib.accepted, accepted) and ib.acc_ratio == acc_ratio
    # the walk and the index draw are the same functions on both paths: up to the first rejuvenation the default path agrees
    first = tr.nrej.index(1)
    tr2 = _Trace(monkeypatch)
    ref = _ibis(case, M, 5)
    smc.smc2(ref, y)
    smc.smc2_run(ref, y, 2, len(y), verbose=False)
    assert tr2.nrej.index(1) == first and tr2.ess[:first] == trace[:first] and ref.n_rejuvenations >= 2
    mean, cov = smc.posterior_moments(ib)
    assert np.allclose(mean, smc.expected_parameters(ib), rtol=1e-12, atol=0.0)
    th, w = ib.theta, ib.omega
    dv = th - (th * w[:, None]).sum(axis=0)
    assert np.allclose(cov, (dv * w[:, None]).T @ dv, rtol=1e-9, atol=1e-9 * float(np.diag(cov).max()))
    ib.close()
    ref.close()


def test_posterior_mean_recovers_the_exact_posterior():
    """one-parameter case, M = 512, device moves: over the K seeds of test_ibis_host the mean of posterior_moments' E[A] is
    within 4 standard errors of the quadrature value, with at least two rejuvenations in every run (the derivation of
    test_ibis_host.test_restatement_recovers_the_exact_posterior, on the device path)"""
    y = _y()
    mean, sd = grid_posterior_A(y)
    est, nrej = [], []
    for seed in range(1, K_SEEDS + 1):
        ib = _ibis("one", 512, seed, device_moves=True)
        smc.smc2(ib, y)
        smc.smc2_run(ib, y, 2, len(y), verbose=False)
        m, c = smc.posterior_moments(ib)
        assert abs(m[0] - smc.expected_parameters(ib)[0]) <= 1e-12 * abs(m[0]) and 0.0 < c[0, 0] < 1.0
        est.append(m[0])
        nrej.append(ib.n_rejuvenations)
        ib.close()
    est = np.array(est)
    se = est.std(ddof=1) / math.sqrt(K_SEEDS)
    print("grid E[A] = %.6f sd = %.6f; device moves mean = %.6f, SE = %.6f, rejuvenations = %s" % (mean, sd, est.mean(), se, nrej))
    assert sum(n >= 2 for n in nrej) == K_SEEDS
    assert abs(est.mean() - mean) <= 4.0 * se


def test_density_tempered_with_device_moves():
    """the tempering loop with the resample-move of every stage on the device: the ladder's exponents end at 1, every stage
    rejuvenates from the covariance of the device, and the posterior mean agrees with the default path's within the two runs'
    Monte Carlo error (4 posterior-sd / sqrt(ess) each)"""
    y = _y()
    res = []
    for flag in (False, True):
        ib = _ibis("readme", 512, 4, device_moves=flag)
        stages = smc.density_tempered(ib, y, verbose=False)
        assert stages[-1][0] == 1.0 and ib.n_rejuvenations >= 2
        m, c = smc.posterior_moments(ib)
        res.append((m[0], math.sqrt(c[0, 0]), ib.ess, stages[0][:2]))
        ib.close()
    assert res[0][3] == res[1][3]                          # the first stage: the same bisection on the same logZ
    assert abs(res[0][0] - res[1][0]) <= 4.0 * res[0][1] / math.sqrt(res[0][2]) + 4.0 * res[1][1] / math.sqrt(res[1][2])


def test_default_path_makes_the_calls_it_made(monkeypatch):
    """IBIS(...) without the flag: the flag is off, the windows go through the records and the host walk, and none of the new
    entry points is called"""
    def refuse(*a, **k):
        raise AssertionError("a device-moves entry point was called without the flag")
    for name in ("window_ess", "resample", "theta_moments", "get_moved"):
        monkeypatch.setattr(L.IbisHandle, name, refuse)
    walks = []
    walk = L.host_outer_walk
    monkeypatch.setattr(L, "host_outer_walk", lambda rec, n, e: walks.append(rec.shape) or walk(rec, n, e))
    y = _y(60)
    ib = _ibis("readme", 77, 5)
    assert ib.device_moves is False
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, len(y), verbose=False)
    assert ib.n_rejuvenations >= 1 and walks and all(s[1:] == (10, 4) for s in walks)
    ess, j = smc.ibis._window(ib, y[:2], 0.0)
    assert j == 2 and walks[-1] == (2, 10, 4)
    ib.close()


def test_accepted_stays_readable_and_one_particle_is_refused():
    """the mask left on the device survives close() and a second smc2 (which resets the handle); rejuvenate_ of a cloud of one
    particle is an error on this path as on the default one (no covariance)"""
    y = _y(60)
    ib = _ibis("readme", 77, 5, device_moves=True)
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, len(y), verbose=False)
    assert ib.n_rejuvenations >= 1
    mask = ib._h.get_moved()
    ib._accepted = None                                    # as rejuvenate_ leaves it
    smc.smc2(ib, y)
    assert np.array_equal(ib.accepted, mask)
    ib._accepted = None
    ib._h.rejuvenate(y[:1], 1.0, np.eye(3), 0.5 * np.arange(3, 0, -1), 7, want_moved=False)
    mask = ib._h.get_moved()
    ib.close()
    assert ib._h is None and np.array_equal(ib.accepted, mask)
    one = _ibis("readme", 1, 5, device_moves=True)
    smc.smc2(one, y)
    with pytest.raises(ValueError, match="M >= 2"):
        smc.rejuvenate_(one, y[:1])
    with pytest.raises(L.SmcError):
        smc.rejuvenate_(_ibis("readme", 1, 5), y[:1])      # the default path: smc_host_rw_factor refuses n < 2
    one.close()
