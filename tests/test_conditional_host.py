"""The conditional particle filter on the CPU (no GPU): (a) the slot rule smc_host_conditional_slot against a Python
restatement from the Philox words, its range and its uniformity; (b) smc_host_logobs is the log-weight of the whole step's host twin,
bit for bit; (c) the composed reference (tests/conditional_reference.py) with one backward-simulated path per sweep
(smc_host_sample_paths) leaves the exact posterior of the linear-Gaussian model invariant - and the same harness with the override
switched off does not."""
import ctypes as C

import numpy as np
import pytest
from scipy.stats import chi2

import composed_reference as CR
import conditional_reference as CF

LG = CF.README_LG
SV = [0.0, 0.95, 0.3]
UC = [0.2, 0.2, 3.0, 0.0, 0.0]
RAW = {1: LG, 2: SV, 3: UC}
SLOT_COND = 38


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def slot_restated(L, seed, stream, t, n):
    """mulhi64(u, n) with u = word 1 << 32 | word 0 of philox4x32_10(ctr = (pair 0, stream, t, SLOT_COND), key = the seed's halves)"""
    out = (C.c_uint32 * 4)()
    L.lib().smc_host_philox4x32_10((C.c_uint32 * 4)(0, stream, t, SLOT_COND), (C.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32), out)
    return (((out[1] << 32) | out[0]) * n) >> 64


# ---- (a) the slot rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 1 << 20])
def test_slot_rule_is_the_restatement_and_in_range(L, n):
    for seed in (1, 0x9E3779B97F4A7C15, (1 << 64) - 1):
        for stream in (0, 3, 0xFFFFFFFF):
            for t in (0, 1, 11, 4000000000):
                k = L.host_conditional_slot(seed, stream, t, n)
                assert k == slot_restated(L, seed, stream, t, n), (seed, stream, t, n)
                assert 0 <= k < n
    with pytest.raises(L.SmcError):
        L.host_conditional_slot(1, 0, 0, 0)


def test_slot_rule_is_uniform(L):
    """n = 7 over the 2^14 pairs (stream, t) in 128 x 128 under one seed: the two-sided chi-square band of tests/test_oracle.py"""
    ks = np.array([L.host_conditional_slot(20260, s, t, 7) for s in range(128) for t in range(128)])
    cnt = np.bincount(ks, minlength=7)
    stat = float(np.sum((cnt - len(ks) / 7.0) ** 2 / (len(ks) / 7.0)))
    print("slot counts", cnt, "chi-square", stat)
    assert 0.0005 < chi2.cdf(stat, 6) < 0.9995, (cnt, stat)
    # ... and a slot depends on the step and on the stream
    assert len(set(ks[:128])) > 1 and len(set(ks[::128])) > 1


# ---- (b) the log-weight of the reference row -------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 2, 3])
def test_host_logobs_is_the_steps_logw(L, ob, model):
    d, n, raw = CF.ROWS[model], 64, RAW[model]
    for first, y in ((True, 0.37), (False, -1.9), (False, 2.5e3)):
        z = np.stack([ob.state_normals(5, 2, 3, ob.SLOT_NORMAL0 + k, n) for k in range(d)])
        xp = None if first else np.stack([ob.state_normals(6, 1, 2, ob.SLOT_NORMAL0 + k, n) for k in range(d)])
        x, logw = L.host_filter_steps(model, raw, CR.NONE, None, xp, z, y, first=first)
        got = np.array([L.host_logobs(model, raw, x[:, i], y) for i in range(n)])
        assert np.array_equal(bits(got), bits(logw)), (model, first, y)
    with pytest.raises(L.SmcError):
        L.host_logobs(4, UC, np.zeros(4), 0.1)                 # the marginal family has no observation density of its rows alone


# ---- (c) invariance ----------------------------------------------------------------------------------------------------------------
T, N, CHAINS, SWEEPS = 6, 4, 2048, 4


def sweeps(L, ob, y, start, override):
    """SWEEPS sweeps of CHAINS chains (streams 0 .. CHAINS - 1) from start [CHAINS][T]: the conditional filter of the composed reference
    under the filter seed 100 + k, then ONE backward-simulated path under the path seed 900 + k -> the paths [CHAINS][T]"""
    paths = start.copy()
    for k in range(1, SWEEPS + 1):
        for c in range(CHAINS):
            f = CF.ConditionalFilter(L, ob, 1, LG, N, paths[c].reshape(T, 1), seed=100 + k, stream=c, override=override, record=True)
            for t in range(T):
                f.init(y[t]) if t == 0 else f.step(y[t])
            x, w = f.record()
            idx, xs = L.host_sample_paths(1, LG, x, w, 1, 900 + k, stream=c)
            assert np.all(idx >= 0)
            paths[c] = xs[:, 0, 0]
    return paths


def test_conditional_sweeps_leave_the_posterior_invariant(L, ob):
    """The README LG row, T = 6, N = 4, 2048 chains started from exact posterior draws (a numpy Kalman backward sampler), 4 sweeps:
    every smoothed mean stays within 4.5 standard errors of the RTS mean (standard errors from the exact smoothed variances) - and
    so do the variances and the lag-1 covariances, with the standard errors of normal samples (conditional_reference.worst_z).
    The same harness with the override switched off - a bootstrap filter and one backward path, which forgets its start - leaves
    that band: the bias of backward simulation at N = 4 sits in the spread of the paths (the variances), less in their means."""
    _, y = ob.simulate(1, LG, T, 1998)
    start = CF.exact_posterior_draws(LG, y, CHAINS, np.random.default_rng(7))
    z0 = CF.worst_z(start, LG, y)
    print("exact draws: worst |z| of means %.2f, variances %.2f, lag-1 covariances %.2f" % z0)
    assert z0[0] <= 4.5
    got = CF.worst_z(sweeps(L, ob, y, start, True), LG, y)
    print("conditional, %d sweeps: worst |z| of means %.2f, variances %.2f, lag-1 covariances %.2f" % ((SWEEPS,) + got))
    assert max(got) <= 4.5, got
    ctl = CF.worst_z(sweeps(L, ob, y, start, False), LG, y)
    print("override off, %d sweeps: worst |z| of means %.2f, variances %.2f, lag-1 covariances %.2f" % ((SWEEPS,) + ctl))
    assert max(ctl) > 4.5, ctl
