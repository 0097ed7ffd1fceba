"""The lag-one pair moments on the host (smc_host_smooth_pairs, em_mstep) against references that share no
arithmetic with the library (tests/pairs_reference.py).  No GPU.

  * the host twin against the recursion in long double with exact sums, within the bound of the smoother's twin applied to the
    absolute terms: recorded clouds of the three families, the sharp-observation record, the planted clouds
  * identities: ws, mean, var are smc_host_smooth's bits; T = 1 is empty; a collapsed filter reads NaN; states on particles of
    weight 0 change nothing
  * the lag-one covariance against the exact RTS one (the criterion of the path tests, without paths)
  * em_mstep against a direct Kalman-EM step, and on synthetic moments with a known minimiser
"""
import numpy as np
import pytest

import conditional_reference as CR
import pairs_reference as PR
import paths_reference as PA
import smoother_planted as P
import smoother_reference as R

EPS = 2.0 ** -52
CH = 128
LG_README = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
SHARP = [0.5, 1.0, 0.9, 1e-4, 0.0, 1.0]
ROWS = {R.LG1D: LG_README, R.SV1D: [-1.0, 0.95, 0.3], R.UCSV3D: [0.2, 0.3, 1.0, -1.0, -0.5]}
WORST = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def check_against_reference(L, model, raw, x, w, label):
    """For every entry S of cross[t] and resid2[t], t = 0 .. T-2, with h_ij its term and P_ij the pair probability:
        |S - ref| <= (T - t) (2 (CH + n / CH) + 200) eps sum_ij P_ij |h_ij|  +  4 eps sum_ij P_ij |h_ij| (|logf_ij| + |logD_j|)
    The first term is the bound of the smoother's twin (test_smoother_host.py) applied to the absolute terms: the error of
    ws_{t+1} carried into every term, the two chunked summations (over j, over i), a few ulps of sp_exp.  The second is what that
    form leaves out, the conditioning of the exponential: p_ij = ws_j sp_exp(logf_ij - logD_j), and the fma chain of logf_ij is
    known to 3 eps |logf_ij| only (d = x - m rounded once, eps / 2 relative, so d d to eps; the product d d and the fma, eps / 2
    each; the rounded centre m, eps |s| |m| |d|, below the eps |d d s| of d itself whenever |m| <= |d| and a few eps otherwise on
    every record here), logD_j = M_j + sp_log(S_j) to 3 eps |M_j| + eps |logD_j| / 2 the same way: p_ij to 4 eps (|logf_ij| +
    |logD_j|) relative.  For the smoothed weights that error is diluted by the target's weight, and the smoother's bound never
    needed the term.  A pair moment weighs a far target by its own distance: on the lone target of smoother_planted.far_apart
    (60 scales away: logf and logD near -1800, h = d d near 3600 scales^2) the first term alone is exceeded - SV1D, n = 65, t = T - 2:
    1.07 of it - and every other case stays below 0.62 of it; on filter records |logf| + |logD| is a few units and the second term
    is a few percent of the first.  The largest fraction of the whole bound, and of its first term alone, is printed per case."""
    T, n = w.shape
    ws, mean, var, cross, resid2 = L.host_smooth_pairs(model, raw, x, w)
    rc, rr, ac, ar, cc, cr = PR.pairs_ref(model, raw, x, w)
    unit = (2 * (CH + n / CH) + 200) * EPS
    worst, worst1 = 0.0, 0.0
    for t in range(T - 1):
        for got, ref, mag, cond in ((cross[t], rc[t], ac[t], cc[t]), (resid2[t], rr[t], ar[t], cr[t])):
            err = np.abs(got.astype(R.LD) - ref).astype(np.float64)
            tol1 = ((T - t) * unit * mag).astype(np.float64)
            tol = tol1 + (4 * EPS * cond).astype(np.float64)
            worst, worst1 = max(worst, float(np.max(err / tol))), max(worst1, float(np.max(err / tol1)))
            assert np.all(err <= tol), (label, model, n, T, t, err, tol)
    WORST[label] = max(WORST.get(label, 0.0), worst)
    print("%s model %d n %d T %d: worst |S - ref| / bound %.4f (/ its first term alone %.4f)" % (label, model, n, T, worst, worst1))
    return ws, mean, var, cross, resid2


@pytest.mark.parametrize("T", [2, 12])
@pytest.mark.parametrize("n", [1, 65, 300])
@pytest.mark.parametrize("model", [R.LG1D, R.SV1D, R.UCSV3D])
def test_host_pairs_against_longdouble(L, ob, model, n, T):
    x, w = PA.recorded_clouds(L, ob, model, ROWS[model], n, T)
    assert np.all((w > 0).any(axis=1))
    ws, mean, var, cross, resid2 = check_against_reference(L, model, ROWS[model], x, w, "recorded")
    hs, hm, hv = L.host_smooth(model, ROWS[model], x, w)
    assert same(ws, hs) and same(mean, hm) and same(var, hv)           # ws, mean, var: smc_host_smooth's bits
    d = R.DIM[model]
    assert cross.shape == (T - 1, d, d) and resid2.shape == (T - 1, d) and np.all(resid2 >= 0)


@pytest.mark.parametrize("n", [65, 300])
def test_host_pairs_sharp_observation(L, ob, n):
    x, w = PA.recorded_clouds(L, ob, R.LG1D, SHARP, n, 12)
    assert (w == 0).mean() > 0.5
    out = check_against_reference(L, R.LG1D, SHARP, x, w, "sharp")
    assert all(np.all(np.isfinite(a)) for a in out)
    # a NaN state on every particle of weight 0 (a source at t, a target at t + 1) changes nothing
    xn, _ = P.nan_on_zero(x, w)
    assert all(same(a, b) for a, b in zip(out, L.host_smooth_pairs(R.LG1D, SHARP, xn, w)))


PLANTED = [(model, ROWS[model], name) for model in (R.LG1D, R.SV1D, R.UCSV3D) for name in P.ALIVE]
PLANTED += [(R.LG1D, SHARP, name) for name in P.ON_ZERO + P.ALIVE]


@pytest.mark.parametrize("n", [65, 300])
@pytest.mark.parametrize("model,raw,name", PLANTED, ids=lambda v: v if isinstance(v, str) else ("sharp" if v is SHARP else None))
def test_host_pairs_planted_clouds(L, ob, model, raw, name, n):
    x, w = PA.recorded_clouds(L, ob, model, raw, n, 6)
    px, pw = P.variant(name, model, raw, x, w)
    out = check_against_reference(L, model, raw, px, pw, "planted")
    assert all(np.all(np.isfinite(a)) for a in out)
    if name in P.ON_ZERO:                                             # left out whatever their states: the bits of the plain record
        assert all(same(a, b) for a, b in zip(out, L.host_smooth_pairs(model, raw, x, w)))


@pytest.mark.parametrize("model", [R.LG1D, R.SV1D, R.UCSV3D])
def test_identities(L, ob, model):
    raw, d = ROWS[model], R.DIM[model]
    x, w = PA.recorded_clouds(L, ob, model, raw, 300, 6)
    ws, mean, var, cross, resid2 = L.host_smooth_pairs(model, raw, x[:1], w[:1])      # T = 1: nothing to pair
    assert cross.shape == (0, d, d) and resid2.shape == (0, d) and same(ws, w[:1])
    assert same(mean, L.host_smooth(model, raw, x[:1], w[:1])[1])
    for t_dead in P.dead_steps(6):
        px, pw = P.dead_at(x, w, t_dead)
        assert all(np.all(np.isnan(a)) for a in L.host_smooth_pairs(model, raw, px, pw)), t_dead
        assert all(np.all(np.isnan(a.astype(np.float64))) for a in PR.pairs_ref(model, raw, px, pw))
    # the row sums of p_ij are ws_t and its column sums ws_{t+1}: resid2 of a row whose centre is the state itself is the smoothed
    # second moment of the increment, E x_{t+1}^2 - 2 cross + E x_t^2
    if model == R.UCSV3D:
        ws, mean, var, cross, resid2 = L.host_smooth_pairs(model, raw, x, w)
        e2 = var + mean ** 2
        for c in range(d):
            inc = e2[1:, c] - 2 * cross[:, c, c] + e2[:-1, c]
            assert np.allclose(resid2[:, c], inc, rtol=1e-9, atol=1e-12)
    with pytest.raises(L.SmcError):
        L.host_smooth_pairs(L.MODEL_UCSV_RB, ROWS[R.UCSV3D], np.zeros((2, 4, 2)), np.full((2, 2), 0.5))


def test_lag_one_covariance_against_rts(L, ob):
    """LG1D, README row, 24 filters of 512 particles, T = 12: lag1_cov[t] = cross[t] - mean[t] mean[t + 1] of every filter, its
    average over the filters against the exact C_t = G_t Ps_{t+1} of the RTS smoother: z = |avg - exact| / (sd / sqrt(24)) <= 4.5 at
    every t, the criterion of the path tests (test_paths_host.py) - here without a single path.  The z-scores against 0 are printed
    for contrast: independent marginals would have covariance 0."""
    K, n, T = 24, 512, 12
    _, y = L.simulate(R.LG1D, LG_README, T, 1998)
    _, _, C_rts = CR.exact_moments(LG_README, y)
    lag = np.zeros((K, T - 1))
    for k in range(K):
        x, w = PA.recorded_clouds(L, ob, R.LG1D, LG_README, n, T, seed=300 + k)
        _, mean, _, cross, _ = L.host_smooth_pairs(R.LG1D, LG_README, x, w)
        lag[k] = cross[:, 0, 0] - mean[:-1, 0] * mean[1:, 0]
    z, z0 = PA.z_scores(lag, C_rts), PA.z_scores(lag, 0.0)
    print("max z of the lag-one covariances %.2f; against 0: %s" % (z.max(), np.round(z0, 1)))
    assert np.all(z <= 4.5), z


def test_em_mstep_linear_gaussian_equals_kalman_em():
    """fed the exact RTS moments of the README row, em_mstep is the Kalman-EM step, to 1e-12 relative"""
    import sequential_monte_carlo_amd as smc
    T = 40
    m = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
    _, y = smc.simulate(m, T, seed=1998)
    ms, Ps, cr = PR.kalman_em_moments(m.raw(), y)
    s = {"mean": ms, "var": Ps, "cross": cr, "resid2": np.zeros(T - 1)}
    want = PR.kalman_em_step(m.raw(), y)
    m1 = smc.em_mstep(m, y, s)
    got = np.array([m1.A, m1.Q, m1.R])
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (got, want)
    assert (m1.B, m1.x0, m1.sigma0) == (m.B, m.x0, m.sigma0)
    assert not np.allclose(got, [m.A, m.Q, m.R], rtol=1e-3)           # a step was taken
    # free: the others stay; Q uses the A in force
    mq = smc.em_mstep(m, y, s, free=["Q"])
    e2 = Ps + ms ** 2
    assert (mq.A, mq.R) == (m.A, m.R)
    assert abs(mq.Q - (e2[1:].sum() - 2 * m.A * cr.sum() + m.A ** 2 * e2[:-1].sum()) / (T - 1)) <= 1e-12 * mq.Q
    # a gap: R from the observed periods only
    yg = y.copy()
    yg[[3, 17]] = np.nan
    keep = np.isfinite(yg)
    mr = smc.em_mstep(m, yg, s, free=["R"], missing=True)
    assert abs(mr.R - np.mean((y[keep] - ms[keep]) ** 2 + Ps[keep])) <= 1e-12 * mr.R
    with pytest.raises(ValueError):
        smc.em_mstep(m, yg, s)
    with pytest.raises(ValueError):
        smc.em_mstep(m, y, s, free=["B"])
    with pytest.raises(ValueError):
        smc.em_mstep(m, y, dict(s, cross=cr[:-1]))
    with pytest.raises(TypeError):
        smc.em_mstep(smc.MarginalUCSV((0.2, 0.3), 1.0, (-1.0, -0.5)), y, s)


def test_em_mstep_synthetic_moments():
    """SV and UCSV on moments with a known minimiser: the moments of a degenerate law on ONE path (var = 0, cross and resid2 its
    products) make the M-step the least-squares fit of that path"""
    import sequential_monte_carlo_amd as smc
    rng = np.random.default_rng(7)
    T = 50
    mu, rho, sigma = -0.7, 0.9, 0.25
    x = np.zeros(T)
    x[0] = mu
    for t in range(1, T):
        x[t] = mu + rho * (x[t - 1] - mu) + sigma * rng.normal()
    y = rng.normal(size=T)
    sv0 = smc.StochasticVolatility(0.0, 0.5, 1.0)
    s = {"mean": x, "var": np.zeros(T), "cross": x[:-1] * x[1:], "resid2": np.zeros(T - 1)}
    sv = smc.em_mstep(sv0, y, s)
    G = np.stack([np.ones(T - 1), x[:-1]], axis=1)
    (al, rh), res, _, _ = np.linalg.lstsq(G, x[1:], rcond=None)
    assert abs(sv.rho - rh) <= 1e-10 and abs(sv.mu - al / (1 - rh)) <= 1e-10
    assert abs(sv.sigma - np.sqrt(res[0] / (T - 1))) <= 1e-10
    # one held: the other's conditional minimiser, by a scan of the objective
    obj = lambda m_, r_: np.sum((x[1:] - m_ - r_ * (x[:-1] - m_)) ** 2)
    s1 = smc.em_mstep(sv0, y, s, free=["rho"])
    assert s1.mu == 0.0 and s1.sigma == 1.0
    assert all(obj(0.0, s1.rho) <= obj(0.0, s1.rho + e) for e in (-1e-4, 1e-4))
    s2 = smc.em_mstep(sv0, y, s, free=["mu"])
    assert s2.rho == 0.5 and all(obj(s2.mu, 0.5) <= obj(s2.mu + e, 0.5) for e in (-1e-4, 1e-4))
    s3 = smc.em_mstep(sv0, y, s, free=["sigma"])
    assert abs(s3.sigma ** 2 - obj(0.0, 0.5) / (T - 1)) <= 1e-12
    # UCSV: gamma_c^2 = (var_0 + (mean_0 - l0)^2 + sum resid2) / T
    uc = smc.UCSV((0.2, 0.3), 1.0, (-1.0, -0.5))
    mean, var = rng.normal(size=(T, 3)), rng.uniform(0.1, 0.2, size=(T, 3))
    resid2 = rng.uniform(0.01, 0.05, size=(T - 1, 3))
    su = {"mean": mean, "var": var, "cross": np.zeros((T - 1, 3, 3)), "resid2": resid2}
    u1 = smc.em_mstep(uc, y, su)
    for k, c in ((0, 1), (1, 2)):
        want = (var[0, c] + (mean[0, c] - uc.log_sigma0[k]) ** 2 + resid2[:, c].sum()) / T
        assert abs(u1.gamma[k] ** 2 - want) <= 1e-12 * want
    assert (u1.x0, u1.log_sigma0) == (uc.x0, uc.log_sigma0)
    u2 = smc.em_mstep(uc, y, su, free=["gamma_eta"])
    assert u2.gamma[0] == uc.gamma[0] and u2.gamma[1] == u1.gamma[1]


def test_worst_fraction_of_the_bound():
    """the figure DESIGN.md 2m quotes (runs after the cases above; a fraction above 1 would have failed there)"""
    print("worst fraction of the bound:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())
