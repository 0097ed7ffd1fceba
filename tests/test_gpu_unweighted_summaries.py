"""The unweighted summary mode (smc_set_summary_mode, SMC_SUMM_UNWEIGHTED) on every launch path that computes summaries
(pytest -m gpu): the type-7 quantile(x, p) and the corrected var(x) of the cloud, whatever its weights.

The reference is the published definition in numpy (tests/quantile7_reference.py), NOT the oracle, which does not know the mode.
Device quantiles equal the helper applied to the cloud BIT FOR BIT; moments hold the bounds of tests/summary_reference.py with
weights 1/n.  The cloud after each step comes from a twin handle driven through the step API, as in tests/test_gpu_summaries.py
(whose data table and shapes are used here); the paths are asserted with path_of:
  R       k_resident<UNW>, per step            window  k_resident<WIN, UNW> (step_window)
  once    k_summ_once<UNW> (moments() / quantiles() between steps)
  S       SMC_FLAG_NO_RESIDENT, M1, M2, G: the k_ms_*<UNW> chain, k_ms_succ, k_ms_interp (two-level: SMC_MS_TWO_LEVEL and a
          filter beyond 2^21 particles)
"""
import math

import numpy as np
import pytest

from quantile7_reference import check_sample_moments, cross_bound, quantile7, same_bits
from summary_reference import VAR_LEVEL, VAR_REL
from test_gpu_paths import path_of
from test_gpu_summaries import CASES_D1, DATA, IDS_D1, NO_RESIDENT, PS, UC, UC_LEVEL, lg_level, series, twin_states

pytestmark = pytest.mark.gpu

assert {"lgc1e8", "lge", "lge1e6"} <= {name for _, _, name, _ in CASES_D1}      # the cluster and all-equal clouds


def check_rows_unw(q, mean, var, x, comp, ps, ctx):
    """per-filter unweighted summaries of one step (q [nth][np], mean / var [d][nth]) against the helper on the cloud x [d][nth][n]"""
    for th in range(x.shape[1]):
        if q is not None:
            ref = quantile7(x[comp, th], ps)
            assert same_bits(q[th], ref), ("quantiles",) + ctx + (th, q[th], ref)
        if mean is not None:
            for c in range(x.shape[0]):
                check_sample_moments(mean[c, th], var[c, th], x[c, th], ctx + (th, c))


def run_per_step_unw(L, pid, model, raws, n, seg=0, flags=0, T=6, ps=PS, comp=0, seed=23, y=None, once=True):
    """per-step unweighted summaries of one log_likelihood call on path pid, and (once) the stand-alone ones of the twin"""
    raws = np.atleast_2d(np.asarray(raws, dtype=np.float64))
    if y is None:
        y = series(model, raws[0], T)
    h = L.Handle(model, len(raws), n, seg=seg, seed=seed, flags=flags)
    assert path_of(h) == pid, (pid, n, seg, h.nseg, h.resident)
    h.set_params(raws)
    h.set_summary_mode("unweighted")
    h.set_summaries(ps, comp, moments=True)
    _, lm, _ = h.log_likelihood(y, trace=True)
    q, mean, var = h.get_summaries(len(y))
    once_rows = {}

    def stand_alone(ht, t):
        ht.set_summary_mode("unweighted")
        once_rows[t] = (ht.quantiles(ps, comp), ht.moments())
        ht.set_summary_mode("weighted")

    states = twin_states(L, model, raws, n, seg, flags, seed, y, stand_alone if once else None)
    for t, (lmt, x, _) in enumerate(states):
        assert same_bits(lmt, lm[t]), (pid, n, t)          # the twin holds the state of the call's step t
        check_rows_unw(q[t], mean[t], var[t], x, comp, ps, (pid, n, t))
        if once:
            qo, (mo, vo) = once_rows[t]
            check_rows_unw(qo, mo, vo, x, comp, ps, (pid, "once", n, t))
    h.close()
    return q, mean, var, states


@pytest.mark.parametrize("pid,shape,name,raw", CASES_D1, ids=IDS_D1)
def test_unweighted_exact_d1(L, pid, shape, name, raw):
    """d = 1 on every path, every data set: per-step rows and the stand-alone summaries between steps"""
    model, n, seg, flags = shape
    run_per_step_unw(L, pid, model, [raw], n, seg, flags)


@pytest.mark.parametrize("pid,n,seg,raw", [("R", 512, 0, UC), ("R", 4096, 0, UC_LEVEL), ("S", 2048, 0, UC_LEVEL), ("M1", 3000, 512, UC_LEVEL),
                                           ("M2", 33000, 256, UC_LEVEL), ("G", 67000, 256, UC_LEVEL)],
                         ids=["R-512", "R-4096-level", "S-2048-level", "M1-3000-level", "M2-33000-level", "G-67000-level"])
def test_unweighted_exact_ucsv(L, pid, n, seg, raw):
    """UCSV (d = 3): all three coordinates' moments, the quantiles of the trend (component 0) and of component 1"""
    flags = NO_RESIDENT if pid == "S" else 0
    for comp in (0, 1):
        run_per_step_unw(L, pid, 3, [raw], n, seg, flags, T=5, comp=comp, once=comp == 0)


def test_unweighted_exact_batch_of_600(L):
    """600 filters of 1024 particles with mixed parameters: the resident kernel's 256-thread x two-pair variant"""
    raws = np.tile(lg_level(1e4), (600, 1))
    raws[:, 2] *= 1.0 + np.arange(600) / 600.0        # distinct Q per filter
    run_per_step_unw(L, "R", 1, raws, 1024, T=4, ps=[0.1, 0.5, 0.9], y=series(1, lg_level(1e4), 4), once=False)


@pytest.mark.parametrize("n", [1024, 4096])
@pytest.mark.parametrize("name", ["lg", "lg1e6q", "lg1e8", "lgc1e8", "lge1e6"])
def test_unweighted_exact_window(L, n, name):
    """step_window: the window kernel's per-step unweighted summaries after a first log_likelihood call"""
    raw = dict(DATA)[name]
    y = series(1, raw, 10)
    h = L.Handle(1, 1, n, seed=23)
    assert path_of(h) == "R" and h.can_window
    h.set_params([raw])
    h.log_likelihood(y[:4])
    h.set_summary_mode("unweighted")
    h.set_summaries(PS, 0, moments=True)
    lmw, _ = h.step_window(y[4:])
    q, mean, var = h.get_summaries(6)
    for t, (lmt, x, _) in enumerate(twin_states(L, 1, [raw], n, 0, 0, 23, y)):
        if t >= 4:
            assert same_bits(lmt, lmw[t - 4])
            check_rows_unw(q[t - 4], mean[t - 4], var[t - 4], x, 0, PS, ("window", n, name, t))
    h.close()


@pytest.mark.parametrize("name", ["lg", "lg1e6q", "lgc1e8", "lge", "lge1e6"])
def test_unweighted_exact_two_level(L, name, monkeypatch):
    """the second level of the multi-segment selection (filters beyond 2^21 particles) at a small size, through its knob"""
    monkeypatch.setenv("SMC_MS_TWO_LEVEL", "1000")
    run_per_step_unw(L, "M1", 1, [dict(DATA)[name]], 9000, 1024, T=4)


@pytest.mark.parametrize("name", ["lg", "lg1e6q"])
def test_unweighted_exact_beyond_two_level_size(L, name):
    """one real filter above 2^21 particles (ragged): the two-level selection without the knob"""
    n = (1 << 21) + 4097
    run_per_step_unw(L, "G", 1, [dict(DATA)[name]], n, T=3, ps=[0.05, 0.5, 0.95], once=False)


@pytest.mark.parametrize("pid,n,seg,flags", [("R", 1024, 0, 0), ("R", 1000, 0, 0), ("S", 1024, 0, NO_RESIDENT), ("M1", 9000, 1024, 0),
                                             ("G", 70000, 256, 0)])
def test_collapsed_filter_has_finite_unweighted_summaries(L, pid, n, seg, flags):
    """a step after which every weight is 0: the cloud is still there - finite unweighted summaries equal to the helper's (checked
    by run_per_step_unw like every other step), while the weighted ones of the same step are NaN"""
    raw = lg_level(1e6)
    raws = [raw, lg_level(1e6, Q=2.0)]
    y = series(1, raw, 5)
    y[2] = 1e200                                       # (y - x)^2 / R overflows: every log-weight is -inf
    q, mean, var, states = run_per_step_unw(L, pid, 1, raws, n, seg, flags, y=y)
    assert np.all(states[2][2] == 0)                   # the twin's weights after that step: collapsed
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
    h = L.Handle(1, 2, n, seg=seg, seed=23, flags=flags)
    h.set_params(raws)
    h.set_summaries(PS, 0, moments=True)
    h.log_likelihood(y)
    qw, mw, vw = h.get_summaries(5)
    h.close()
    assert np.all(np.isnan(qw[2])) and np.all(np.isnan(mw[2])) and np.all(np.isnan(vw[2]))


MODE_SHAPES = [("R", 1024, 0, 0), ("S", 1024, 0, NO_RESIDENT), ("M1", 9000, 1024, 0), ("G", 70000, 256, 0)]


@pytest.mark.parametrize("pid,n,seg,flags", MODE_SHAPES)
def test_weighted_results_survive_a_detour(L, pid, n, seg, flags):
    """weighted per-step rows and stand-alone summaries of a handle: bit-identical before and after a detour through the
    unweighted mode; an unknown mode is refused and changes nothing"""
    raw = lg_level(1e4)
    y = series(1, raw, 5)
    h = L.Handle(1, 2, n, seg=seg, seed=23, flags=flags)
    assert path_of(h) == pid
    h.set_params([raw, lg_level(1e4, Q=2.0)])
    h.set_summaries(PS, 0, moments=True)

    def weighted():
        h.log_likelihood(y)
        return h.get_summaries(5) + (h.quantiles(PS, 0),) + h.moments()

    before = weighted()
    h.set_summary_mode("unweighted")
    h.log_likelihood(y)
    qu = h.get_summaries(5)[0]
    assert not same_bits(qu, before[0])                # (the detour did compute something else)
    qo = h.quantiles(PS, 0)
    h.set_summary_mode("weighted")
    with pytest.raises(L.SmcError):
        L.check(L.lib().smc_set_summary_mode(h._h, 7))
    after = weighted()
    for a, b in zip(before, after):
        assert same_bits(a, b)
    x, _, _ = h.state(want_anc=False)
    for th in range(2):
        assert same_bits(qo[th], quantile7(x[0, th], PS))
    h.close()


def test_recycled_handle_starts_weighted(L):
    """a handle destroyed in unweighted mode and recreated from the bundle cache (same shape) starts weighted"""
    raw = lg_level(1e4)
    y = series(1, raw, 4)

    def rows(mode):
        h = L.Handle(1, 3, 1024, seed=23)
        h.set_params(np.tile(raw, (3, 1)))
        if mode:
            h.set_summary_mode(mode)
        h.set_summaries(PS, 0, moments=True)
        h.log_likelihood(y)
        out = h.get_summaries(4) + (h.quantiles(PS, 0),)
        h.close()
        return out

    first = rows(None)
    unw = rows("unweighted")
    again = rows(None)                                 # the recycled bundle of the handle closed in unweighted mode
    assert not same_bits(unw[0], first[0])
    for a, b in zip(first, again):
        assert same_bits(a, b)


@pytest.mark.parametrize("pid,n,seg,flags", MODE_SHAPES)
def test_skipped_filters_have_nan_rows_in_both_modes(L, pid, n, seg, flags):
    raw = lg_level(1e4)
    y = series(1, raw, 4)
    skip = np.array([0, 1, 0, 1, 1], dtype=np.uint8)
    for mode in ("weighted", "unweighted"):
        h = L.Handle(1, 5, n, seg=seg, seed=23, flags=flags)
        assert path_of(h) == pid
        h.set_params(np.tile(raw, (5, 1)))
        h.set_summary_mode(mode)
        h.set_summaries(PS, 0, moments=True)
        h.set_skip(skip)
        h.log_likelihood(y)
        q, mean, var = h.get_summaries(4)
        h.close()
        for m in range(5):
            rows = (q[:, m], mean[:, :, m], var[:, :, m])
            assert all(np.all(np.isnan(r)) if skip[m] else np.all(np.isfinite(r)) for r in rows), (mode, m)


def test_readme_loop_matches_numpy(L):
    """log_likelihood(1024, y, m, quantiles=[.25, .5, .75], weighted=False): step by step np.quantile of the twin's cloud, within
    the cross-check bound of tests/quantile7_reference.py - the README loop, pinned to something outside this repository"""
    import sequential_monte_carlo_amd as smc
    ps = [0.25, 0.5, 0.75]
    m = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8, x0=0.0, sigma0=1.0)
    _, y = smc.simulate(m, 30, seed=1998)
    x, w, logZ, extra = smc.log_likelihood(1024, y, m, seed=9, quantiles=ps, moments=True, weighted=False)
    assert x._f.h.summary_mode == "weighted"           # restored
    q = extra["quantiles"]
    states = twin_states(L, 1, [m.raw()], 1024, 0, 0, 9, y)
    for t, (_, xt, _) in enumerate(states):
        ref = np.quantile(xt[0, 0], ps)
        for j, p in enumerate(ps):
            assert abs(q[t, j] - ref[j]) <= cross_bound(xt[0, 0], p), (t, p, q[t, j], ref[j])
        assert same_bits(q[t], quantile7(xt[0, 0], ps))
        check_sample_moments(extra["mean"][t], extra["var"][t], xt[0, 0], ("readme", t))
    # the views between steps: Particles.quantile / moments with weighted=False, and the weighted default untouched
    xs = np.asarray(x)
    assert same_bits(x.quantile(ps, weighted=False), quantile7(xs, ps))
    mu, var = x.moments(weighted=False)
    check_sample_moments(float(mu), float(var), xs, ("view",))
    assert same_bits(x.quantile(ps), x._f.h.quantiles(ps)[0])


def test_filtered_summaries_literal():
    """filtered_summaries(smc, literal=True) after smc2 + smc2_run: the omega-weighted sum, in index order, of the helper applied
    to each filter's cloud read back with state(); smc2_run(..., summaries=, literal=True) records the same per step"""
    import io
    import sequential_monte_carlo_amd as smc
    from quantile7_reference import sample_moments
    ps = [0.25, 0.5, 0.75]
    prior = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(), smc.LogNormal()])
    tmap = smc.ThetaMap(1, [0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    _, y = smc.simulate(smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8), 24, seed=1998)
    s = smc.SMC(128, 16, lambda th: smc.UnivariateLinearGaussian(A=th[0], B=1.0, Q=th[1], R=th[2]), prior, 2, 0.6, seed=22, theta_map=tmap)
    smc.smc2(s, y[:16])
    smc.smc2_run(s, y, 17, 22, window=4, verbose=False, out=io.StringIO(), summaries=ps, literal=True)
    q, v = smc.filtered_summaries(s, ps, literal=True)
    assert s._main.summary_mode == "weighted"
    x, _, _ = s._main.state(want_anc=False)
    om = np.asarray(s.omega, dtype=np.float64)
    rows = np.array([np.concatenate([quantile7(x[0, m], ps), [0.0]]) for m in range(s.M)])
    qsum = np.add.reduce(om[om > 0, None] * rows[om > 0], axis=0)[:-1]
    assert same_bits(q, qsum), (q, qsum)
    refs = [sample_moments(x[0, m]) for m in range(s.M)]
    V = math.fsum(om[m] * refs[m][1] for m in range(s.M) if om[m] > 0)
    slack = math.fsum(om[m] * (VAR_LEVEL * refs[m][0]) ** 2 for m in range(s.M) if om[m] > 0)
    assert abs(v - V) <= VAR_REL * V + slack, (v, V)          # the bound of tests/summary_reference.py, integrated
    t_last, q_last, v_last = s.summary_trace[-1]
    assert t_last == 22 and same_bits(q_last, q) and v_last == v
    qw, _ = smc.filtered_summaries(s, ps)
    assert not same_bits(qw, q)
