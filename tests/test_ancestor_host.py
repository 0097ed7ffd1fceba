"""Ancestor sampling on the CPU (no GPU): the host twin smc_host_ancestor_sweep of ONE filter.
  a. every ancestor draw J_t lies where the exact CDF (np.longdouble, tests/paths_reference.py) puts the uniform of the draw, rebuilt
     here from the Philox words, within check_indices' own tolerance (n + 1) 2^-40 + 1000 eps
  b. the trace: the last index is backward simulation's (smc_host_sample_paths, M = 1, the same path seed), the earlier ones follow the
     trace rule restated in Python, and the new reference is the record's states bit for bit
  c. planted clouds: zero-weight sources are never drawn; a reference out of every source's reach keeps the ancestor it had; a last
     step without a live particle is a dead filter
  d. invariance: the composed conditional filter (tests/conditional_reference.py) with the twin as its sweep leaves the exact
     posterior of the linear-Gaussian model invariant and moves nearly every entry of the path; the same loop with J_t drawn from
     the weights alone does not (at 8192 chains: the count the control needed to leave the band)
"""
import numpy as np
import pytest

import ancestor_reference as AR
import conditional_reference as CF

LG = CF.README_LG
SV = [0.0, 0.95, 0.3]
UC = [0.2, 0.2, 3.0, 0.0, 0.0]
RAW = {1: LG, 2: SV, 3: UC}
T5, SEED, PATH_SEED, STREAM = 5, 11, 0xC0FFEE, 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def case(L, ob, model, n):
    return AR.arbitrary_case(L, ob, model, RAW[model], n, T5, np.random.default_rng(100 * model + n))


# ---- a. the draw against the CDF ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 2, 3])
@pytest.mark.parametrize("n", [2, 5, 64, 65, 300])
def test_draws_lie_on_the_exact_cdf(L, ob, model, n):
    x, w, a, xref = case(L, ob, model, n)
    J, idx, out = L.host_ancestor_sweep(model, RAW[model], x, w, a, xref, SEED, PATH_SEED, STREAM)
    worst = AR.check_draws(L, model, RAW[model], x, w, xref, J, SEED, STREAM)
    print("model %d n %d: largest distance outside the exact cell %.3g" % (model, n, worst))


# ---- b. the trace -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 2, 3])
@pytest.mark.parametrize("n", [2, 5, 64, 65, 300])
def test_trace_and_new_reference(L, ob, model, n):
    x, w, a, xref = case(L, ob, model, n)
    J, idx, out = L.host_ancestor_sweep(model, RAW[model], x, w, a, xref, SEED, PATH_SEED, STREAM)
    last = L.host_sample_paths(model, RAW[model], x, w, 1, PATH_SEED, stream=STREAM, want_x=False)[0][T5 - 1, 0]
    assert idx[T5 - 1] == last and 0 <= last < n
    assert np.array_equal(idx, AR.trace(L, J, a, int(last), SEED, STREAM, n)), (model, n, idx, J)
    for t in range(T5):
        assert np.array_equal(bits(out[t]), bits(x[t][:, idx[t]])), (model, n, t)


def test_trace_takes_J_at_the_retained_slot(L, ob):
    """every branch of the rule is met: over the seeds some path passes through a retained slot (and takes J_t there, not the
    recorded ancestor), and some step does not"""
    model, n = 1, 5
    x, w, a, xref = case(L, ob, model, n)
    through, beside = 0, 0
    for seed in range(40):
        J, idx, out = L.host_ancestor_sweep(model, RAW[model], x, w, a, xref, seed, PATH_SEED + seed, STREAM)
        for t in range(1, T5):
            if idx[t] == L.host_conditional_slot(seed, STREAM, t, n):
                through += 1
                assert idx[t - 1] == J[t]
            else:
                beside += 1
                assert idx[t - 1] == a[t][idx[t]]
    assert through > 0 and beside > 0, (through, beside)


# ---- c. planted clouds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 2, 3])
def test_zero_weight_sources_are_never_drawn(L, ob, model):
    """half of the sources of every step get the weight 0 and the most attractive state there is - the reference row itself - or a
    state that is not finite"""
    n = 64
    x, w, a, xref = case(L, ob, model, n)
    x, w = x.copy(), w.copy()
    off = np.arange(n) % 2 == 0
    for t in range(T5 - 1):
        w[t, off] = 0.0
        x[t][:, off] = xref[t + 1][:, None]
        x[t][:, off & (np.arange(n) % 4 == 0)] = np.nan
    for seed in range(25):
        J, idx, out = L.host_ancestor_sweep(model, RAW[model], x, w, a, xref, seed, PATH_SEED, STREAM)
        assert not np.any(off[J[1:]]), (model, seed, J)
        AR.check_draws(L, model, RAW[model], x, w, xref, J, seed, STREAM)


@pytest.mark.parametrize("model", [1, 2, 3])
def test_unreachable_reference_keeps_its_ancestor(L, ob, model):
    """xref[2] = 1e200 in every row: every b_l is -inf, S = 0, and J_2 is the retained slot of step 1; the other draws are as ever"""
    n = 65
    x, w, a, xref = case(L, ob, model, n)
    far = xref.copy()
    far[2] = 1e200
    J0 = L.host_ancestor_sweep(model, RAW[model], x, w, a, xref, SEED, PATH_SEED, STREAM)[0]
    J, idx, out = L.host_ancestor_sweep(model, RAW[model], x, w, a, far, SEED, PATH_SEED, STREAM)
    assert J[2] == L.host_conditional_slot(SEED, STREAM, 1, n)
    assert np.array_equal(np.delete(J, 2), np.delete(J0, 2))
    assert np.all(idx >= 0)


def test_dead_last_step_keeps_the_reference(L, ob):
    n = 5
    x, w, a, xref = case(L, ob, 1, n)
    w = w.copy()
    w[T5 - 1] = 0.0
    J, idx, out = L.host_ancestor_sweep(1, LG, x, w, a, xref, SEED, PATH_SEED, STREAM)
    assert np.all(idx == -1) and np.array_equal(bits(out), bits(xref))
    assert J[0] == -1 and np.all(J[1:] >= 0)                       # the draws themselves do not depend on the last step


def test_refusals(L, ob):
    x, w, a, xref = case(L, ob, 1, 5)
    bad = a.copy()
    bad[2, 1] = 5
    for args in ((1, LG, x, w, bad, xref), (1, [0.9, 1.0, -1.0, 0.8, 0.0, 1.0], x, w, a, xref)):   # not a particle; Q < 0
        with pytest.raises(L.SmcError, match="error -1"):
            L.host_ancestor_sweep(*args, SEED, PATH_SEED, STREAM)


# ---- d. invariance -----------------------------------------------------------------------------------------------------------------------
T, N, CHAINS, SWEEPS = 6, 4, 2048, 4
CONTROL_CHAINS = 8192   # the control leaves the band from this count on: worst |z| 2.65 at 2048, 5.92 at 8192, 7.73 at 16384


def sweeps(L, ob, y, start, control):
    """SWEEPS sweeps of len(start) chains (streams 0, 1, ...) from start [chains][T]: the conditional filter of the composed
    reference under the filter seed 100 + k with its clouds and ancestors recorded, then the host twin under the path seed 900 + k.
    control: the same trace with J_t drawn from w_{t-1} alone (ancestor_reference.weights_only_draw) -> the paths [chains][T]"""
    paths = start.copy()
    for k in range(1, SWEEPS + 1):
        for c in range(len(start)):
            f = CF.ConditionalFilter(L, ob, 1, LG, N, paths[c].reshape(T, 1), seed=100 + k, stream=c, record=True)
            a = np.zeros((T, N), dtype=np.int32)
            for t in range(T):
                f.init(y[t]) if t == 0 else f.step(y[t])
                a[t] = -1 if t == 0 else f.snapshot()[2]
            x, w = f.record()
            J, idx, out = L.host_ancestor_sweep(1, LG, x, w, a, paths[c].reshape(T, 1), 100 + k, 900 + k, c)
            assert np.all(idx >= 0)
            if control:
                Jc = np.array([-1] + [AR.weights_only_draw(L, w[t - 1], 100 + k, c, t) for t in range(1, T)])
                idx = AR.trace(L, Jc, a, int(idx[T - 1]), 100 + k, c, N)
                out = np.array([x[t][:, idx[t]] for t in range(T)])
            paths[c] = out[:, 0]
    return paths


def test_ancestor_sampling_leaves_the_posterior_invariant(L, ob):
    """The README LG row, T = 6, N = 4, 2048 chains started from exact posterior draws, 4 sweeps, fixed seeds: means, variances and
    lag-1 covariances stay within 5 standard errors of the exact smoothed moments (conditional_reference.worst_z, the criterion of
    tests/test_gpu_conditional.py), and at least 0.9 of the path entries differ from the start (tracing the lineages without the
    ancestor draws changes 0.64 of them)."""
    _, y = ob.simulate(1, LG, T, 1998)
    start = CF.exact_posterior_draws(LG, y, CHAINS, np.random.default_rng(7))
    got = sweeps(L, ob, y, start, False)
    z = CF.worst_z(got, LG, y)
    moved = float(np.mean(got != start))
    print("ancestor sampling, %d sweeps: worst |z| of means %.2f, variances %.2f, lag-1 covariances %.2f; moved %.3f" % ((SWEEPS,) + z + (moved,)))
    assert max(z) <= 5.0, z
    assert moved >= 0.9, moved


def test_draws_from_the_weights_alone_are_not_invariant(L, ob):
    """The control: the same loop with J_t drawn from w_{t-1} alone, the transition density left out.  Its bias is small after 4 sweeps
    from exact draws: at 2048 chains it stays inside the band (worst |z| 2.65), at 8192 it leaves it (5.92; 7.73 at 16384), so the
    control runs 8192 chains - and so does the correct version beside it, which stays inside (1.59; 1.86 at 16384)."""
    _, y = ob.simulate(1, LG, T, 1998)
    start = CF.exact_posterior_draws(LG, y, CONTROL_CHAINS, np.random.default_rng(7))
    z = CF.worst_z(sweeps(L, ob, y, start, False), LG, y)
    print("ancestor sampling, %d chains: worst |z| of means %.2f, variances %.2f, lag-1 covariances %.2f" % ((CONTROL_CHAINS,) + z))
    assert max(z) <= 5.0, z
    ctl = CF.worst_z(sweeps(L, ob, y, start, True), LG, y)
    print("J from the weights alone, %d chains: worst |z| of means %.2f, variances %.2f, lag-1 covariances %.2f" % ((CONTROL_CHAINS,) + ctl))
    assert max(ctl) > 5.0, ctl
