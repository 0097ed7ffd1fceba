"""The marginal (Rao-Blackwellised) UCSV family on the host (no GPU): smc_host_rb_step against the closed forms in longdouble
(tests/rbpf_reference.py) within propagated rounding bounds, the invariants of the Kalman rows, and the interface."""
import numpy as np
import pytest

import rbpf_reference as R

UC, RB = 3, 4
N_CASES = 4000


def cases(seed=14):
    """(raw, sp, z, y, first): first and later steps, trend levels up to 1e5, log-volatilities in [-12, 4], zero and -0.0 normals"""
    r = np.random.default_rng(seed)
    for i in range(N_CASES):
        level = [0.0, 3.0, 1e2, 1e5][i % 4] * [1.0, -1.0][(i // 4) % 2]
        first = (i // 8) % 3 == 0
        raw = [r.uniform(0.05, 0.5), r.uniform(0.05, 0.5), level + r.normal(), r.uniform(-12, 4), r.uniform(-12, 4)]
        lse, lsn = r.uniform(-12, 4), r.uniform(-12, 4)
        # P: a filtered variance lies below the observation variance that produced it; spread it over eight decades below exp(4)
        sp = [level + r.normal(), lse, lsn, np.exp(r.uniform(-14, 4))]
        z = r.normal(size=2)
        if i % 16 == 5:
            z[0] = 0.0
        if i % 16 == 9:
            z[1] = -0.0
        if i % 64 == 33:
            z[:] = [-0.0, 0.0]
        centre = raw[2] if first else sp[0]
        yield raw, sp, z, centre + r.normal() * 3, first


def test_rb_step_against_longdouble(L):
    """4000 cases.  Bound: rbpf_reference.bounds (one u = 2^-52 per rounded operation, 2u per sp_exp, 2 ulp per sp_log, propagated
    through model_marginal_step's order of operations).  Every output inside its bound; on every case the invariants
    0 < P' <= min(P-, R) (P-, R as the specification computes them), m' between m and y (inclusive), logw finite.
    Measured on the host twin: largest |state - ref| / bound = 0.495, largest |logw - ref| / bound = 0.352 (largest
    absolute logw error 6.3e-11)."""
    lib = L.lib()
    worst_s = worst_w = worst_abs = 0.0
    nfirst = 0
    for raw, sp, z, y, first in cases():
        s, lw = L.host_rb_step(raw, sp, z, y, first)
        nfirst += first
        bs, bw = R.bounds(raw, sp, z, y, first, s)
        l1, l2 = R.vols(raw, sp, z, first)
        m1, P1, ref_lw = R.step(raw, sp, y, first, s[2])
        es = np.abs(np.array([float(R.ld(s[0]) - m1), float(R.ld(s[1]) - l1), float(R.ld(s[2]) - l2), float(R.ld(s[3]) - P1)]))
        ew = abs(float(R.ld(lw) - ref_lw))
        worst_s = max(worst_s, float(np.max(es / np.maximum(bs, 1e-300))))
        worst_w, worst_abs = max(worst_w, ew / bw), max(worst_abs, ew)
        assert np.all(es <= bs) and ew <= bw, (raw, sp, z, y, first, es, bs, ew, bw)
        # invariants, with P- and R in the specification's own arithmetic
        Q = lib.smc_host_exp(float(raw[3] if first else sp[1]))
        Pm = Q if first else float(sp[3]) + Q
        Rn = lib.smc_host_exp(float(s[2]))
        m0 = raw[2] if first else sp[0]
        assert 0.0 < s[3] <= min(Pm, Rn), (raw, sp, z, y, first, s[3], Pm, Rn)
        assert min(m0, y) <= s[0] <= max(m0, y), (raw, sp, z, y, first, s[0])
        assert np.isfinite(lw)
        if z[0] == 0.0:                       # zero and -0.0 normals leave the volatility where it was, bit for bit
            assert s[1] == (raw[3] if first else sp[1])
        if z[1] == 0.0:
            assert s[2] == (raw[4] if first else sp[2])
    assert 1000 < nfirst < 2000
    print("RB step: max |state - ref| / bound %.3f, max |logw - ref| / bound %.3f, max |logw - ref| %.3g" % (worst_s, worst_w, worst_abs))


def test_first_step_does_not_read_the_state(L):
    raw = [0.2, 0.3, 3.0, -1.0, 0.5]
    a, la = L.host_rb_step(raw, [0.0] * 4, [0.3, -0.4], 2.5, True)
    b, lb = L.host_rb_step(raw, [1e9, 7.0, -7.0, 123.0], [0.3, -0.4], 2.5, True)
    assert np.array_equal(a, b) and la == lb
    # ... and it is the later step from the state (x0, lse0, lsn0, P = 0)
    c, lc = L.host_rb_step(raw, [3.0, -1.0, 0.5, 0.0], [0.3, -0.4], 2.5, False)
    assert np.array_equal(a, c) and la == lc


def test_series_of_host_steps_is_the_numpy_filter_of_one_particle(L):
    """one particle through 40 steps with given normals: the recursion of oracle/rbpf_ucsv.py (P - K P form there) to 1e-12"""
    r = np.random.default_rng(2)
    raw = [0.2, 0.2, 3.0, 0.0, 0.0]
    y = 3.0 + np.cumsum(r.normal(size=40))
    s = np.zeros(4)
    lse, lsn, m, P, tot, ref = 0.0, 0.0, 3.0, 0.0, 0.0, 0.0
    for t in range(40):
        z = r.normal(size=2)
        s, lw = L.host_rb_step(raw, s, z, y[t], t == 0)
        P = np.exp(0.0) if t == 0 else P + np.exp(lse)
        lse, lsn = lse + 0.2 * z[0], lsn + 0.2 * z[1]
        S = P + np.exp(lsn)
        ref += -0.5 * (np.log(2 * np.pi) + np.log(S) + (y[t] - m) ** 2 / S)
        K = P / S
        m, P = m + K * (y[t] - m), P - K * P
        tot += lw
        assert np.allclose(s, [m, lse, lsn, P], rtol=1e-12, atol=0)
    assert abs(tot - ref) <= 1e-12 * abs(ref)


def test_dims_and_refusals(L):
    lib = L.lib()
    assert L.MODEL_UCSV_RB == RB
    assert lib.smc_model_dim(RB) == 4 and lib.smc_model_nraw(RB) == 5
    assert lib.smc_model_dim(UC) == 3 and lib.smc_model_dim(5) == -1 and lib.smc_model_nraw(5) == -1
    # the guided twins know no proposal for the family
    a, o, lw = np.zeros(4), np.zeros(4), np.zeros(1)
    raw = np.array([0.2, 0.2, 3.0, 0.0, 0.0])
    for kind in (1, 2):
        assert lib.smc_host_guided_step(RB, L._d(raw), kind, None, L._d(a), L._d(a), 0.1, L._d(o), L._d(lw)) == -1
    assert lib.smc_host_rb_step(None, L._d(a), L._d(a), 0.1, 0, L._d(o), L._d(lw)) == -1
    assert lib.smc_auto_seg(RB, 2048) == 2048 and lib.smc_auto_seg(RB, 4096) == 256 and lib.smc_auto_seg(UC, 4096) == 4096
    # the data-generating model is UCSV: the same series
    xu, yu = L.simulate(UC, raw, 30, 5)
    xr, yr = L.simulate(RB, raw, 30, 5)
    assert np.array_equal(yu, yr) and np.array_equal(xu, xr)


def test_python_types():
    import sequential_monte_carlo_amd as smc
    m = smc.MarginalUCSV((0.2, 0.3), 3.0, (0.0, -1.0))
    assert m.model_id == 4 and m.dim == 4 and m.raw() == [0.2, 0.3, 3.0, 0.0, -1.0]
    u = smc.unobserved_components_stochastic_volatility(x0=3.0, gamma_eps=0.2, gamma_eta=0.3, log_sigma_eps=0.0, log_sigma_eta=-1.0)
    r = smc.unobserved_components_stochastic_volatility(x0=3.0, gamma_eps=0.2, gamma_eta=0.3, log_sigma_eps=0.0, log_sigma_eta=-1.0,
                                                        marginal=True)
    assert type(u) is smc.UCSV and type(r) is smc.MarginalUCSV and u.raw() == r.raw()
    with pytest.raises(ValueError):
        smc.MarginalUCSV((0.0, 0.3), 3.0, (0.0, -1.0))
    with pytest.raises(ValueError):
        smc.MarginalUCSV((0.2, -0.3), 3.0, (0.0, -1.0))
    x, y = smc.simulate(r, 20, seed=3)
    xu, yu = smc.simulate(u, 20, seed=3)
    assert x.shape == (20, 3) and np.array_equal(y, yu) and np.array_equal(x, xu)
    t = smc.ThetaMap(4, [0, 0, 1, 2, 3], [0.0] * 5)
    assert t.model_id == 4 and t.rows([[0.2, 3.0, 0.0, -1.0]]).tolist() == [[0.2, 0.2, 3.0, 0.0, -1.0]]


def test_trend_moments():
    import sequential_monte_carlo_amd as smc
    r = np.random.default_rng(8)
    m, P, w = r.normal(size=500) + 3, np.exp(r.normal(size=500)), r.uniform(size=500)
    w /= w.sum()
    cloud = np.stack([m, r.normal(size=500), r.normal(size=500), P])
    mean = cloud @ w
    var = ((cloud - mean[:, None]) ** 2) @ w
    tm, tv = smc.trend_moments(mean, var)
    # the mixture sum_i w_i N(m_i, P_i): its variance by the second moment about the mixture mean
    assert tm == mean[0]
    assert np.isclose(tv, w @ (P + (m - mean[0]) ** 2), rtol=1e-13)
    bm, bv = smc.trend_moments(np.tile(mean, (5, 1)), np.tile(var, (5, 1)))            # [n_theta][4], or [T][4]
    assert bm.shape == (5,) and np.all(bv == tv)
    with pytest.raises(ValueError):
        smc.trend_moments(mean[:3], var[:3])


def test_oracle_backend_refuses_the_family(ob):
    """the CPU oracle has no such family, and its backend says so instead of running some other filter: oracle.binding.Filter
    looks the model id up in its table of families (KeyError: 4) before anything is created.  The refusal is the oracle's own -
    nothing was added for it."""
    from oracle_backend import OracleBackend
    import sequential_monte_carlo_amd as smc
    assert 4 not in ob.MODEL_DIM and 4 not in ob.MODEL_NRAW
    b = OracleBackend()
    models = smc.smc_samplers.RawModels(4, [[0.2, 0.2, 3.0, 0.0, 0.0]])
    with pytest.raises(KeyError, match="4"):
        b.init(models, 256, 0.1, 1, np.arange(1))
    with pytest.raises(KeyError, match="4"):
        b.log_likelihood(models, 256, np.zeros(3), 1, np.arange(1))
    with pytest.raises(KeyError, match="4"):
        ob.Filter(4, [0.2, 0.2, 3.0, 0.0, 0.0], 256)


def test_numpy_filter_stays_inside_the_kalman_pin_bound(L):
    """the bound of tests/test_gpu_rbpf.py::test_kalman_pin, checked on the CPU first: with gamma = 1e-10 and T = 100 the numpy
    filter of oracle/rbpf_ucsv.py equals the exact Kalman log-likelihood of the local-level model within 10 T gamma sqrt(T) = 1e-6
    (measured: 5.7e-10 and 4.2e-9)"""
    from oracle import kalman, rbpf_ucsv
    g, T = 1e-10, 100
    _, y = L.simulate(UC, [0.2, 0.2, 3.0, 0.0, 0.0], T, 7)
    for lse0, lsn0 in ((0.0, 0.0), (-1.0, 0.5)):
        z = rbpf_ucsv.log_likelihood(y, g, g, 3.0, lse0, lsn0, n=1024, rng=np.random.default_rng(1))
        kf = kalman.log_likelihood(y, 1.0, 1.0, np.exp(lse0), np.exp(lsn0), x0=3.0, sigma0=np.exp(lse0))[2]
        print("numpy filter - Kalman: %.3g" % (z - kf))
        assert abs(z - kf) <= 10 * T * g * np.sqrt(T), (z, kf)
