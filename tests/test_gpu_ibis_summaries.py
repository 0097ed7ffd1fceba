"""GPU tests of the IBIS summaries (smc.observation_dist, estimated_trend, quantile, filtered_state, smc2_run(summaries=);
csrc/smc_ibis_kernels.h k_ibis_sum_chunks / k_ibis_sum_combine / k_ibis_window<.., SUMM>): the device against the host twin of
the same specification with ==, never approx; the recording inside windows against the stand-alone reduction; and the forecast
mean against a quadrature."""
import io
import signal

import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
import ibis_summary_reference as ref
from ibis_reference import LG_TRUE, Y_SEED, case_one_parameter, case_readme

pytestmark = pytest.mark.gpu

CASES = {"readme": case_readme, "one": case_one_parameter}

# Monte-Carlo error of the one-step forecast mean (observation_dist(ibis, ahead=1)[0]) in case_one_parameter, T = 100, from the
# CPU restatement of src/ibis.jl at M = 512 over the seeds 1..16, printed by
#     python scripts/dbg/ibis_forecast_se.py
#   grid forecast mean 0.036600 (E[A] 0.485332); restatement mean 0.036958, sd over seeds 0.001647, SE of the mean of 16 seeds 0.000412
FORECAST_SEEDS = list(range(1, 17))
FORECAST_SD_OVER_SEEDS = 0.001647
FORECAST_SE = 0.000412


@pytest.fixture(autouse=True)
def _time_limit():
    """every test of this file ends after 300 s (the discipline of test_a_million_parameter_particles)"""
    def too_long(*_):
        raise TimeoutError("an IBIS summary test exceeded its time limit")
    old = signal.signal(signal.SIGALRM, too_long)
    signal.alarm(300)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def _y(T=100):
    return smc.simulate(smc.UnivariateLinearGaussian(**LG_TRUE), T, seed=Y_SEED)[1]


def _load(rows, logw):
    """a device cloud with the given rows, (x, S) = (rows[:, 4], rows[:, 5]) and log-weights: theta IS the row"""
    M = rows.shape[0]
    h = L.IbisHandle(M, 6, [L.PRIOR_NORMAL] * 6, np.tile([0.0, 1.0, 0.0, 0.0, 0.0], (6, 1)), [0, 1, 2, 3, 4, 5], [0.0] * 6)
    h.set_theta(rows)
    h.set_logw(logw)
    return h


def _same(a, b):
    """bit for bit, NaN == NaN included"""
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _ibis(case, M, predict_first, seed):
    tmap, prior, model = CASES[case](smc)
    return smc.IBIS(M, model, prior, 3, 0.5, seed=seed, theta_map=tmap, predict_first=predict_first), tmap


def _host(ib, tmap, ahead):
    return L.host_ibis_summary(tmap.rows(ib.theta), ib.x, ib.Sigma, ib.logw, ahead)


@pytest.mark.parametrize("M", ref.SIZES)
@pytest.mark.parametrize("shape", sorted(ref.CLOUDS))
def test_device_equals_host_twin(shape, M):
    """the clouds of test_ibis_summaries_host, both values of ahead: all eight outputs bit for bit"""
    for ahead in (0, 1):
        rows, x, S, logw = ref.CLOUDS[shape](M, 11 * M + ahead)
        rows[:, 4], rows[:, 5] = x, S
        h = _load(rows, logw)
        assert _same(h.summary(ahead), L.host_ibis_summary(rows, x, S, logw, ahead)), ahead
        h.close()


def test_device_equals_host_twin_on_degenerate_clouds():
    """equal weights; one particle with all the weight (between exactly 0); -inf / NaN log-weights on particles whose state is
    NaN (they contribute nothing); no live particle at all (NaN)"""
    rows, x, S, logw = ref.random_cloud(4099, 8)
    one = np.full(4099, -np.inf)
    one[77] = 2.5
    far = np.full(4099, -5000.0)
    far[4098] = 2.5
    dead = logw.copy()
    idx = np.random.default_rng(1).choice(4099, 700, replace=False)
    dead[idx[:600]], dead[idx[600:]] = -np.inf, np.nan
    rows_nan = rows.copy()
    rows_nan[idx[::2], 4], rows_nan[idx[::3], 5] = np.nan, np.inf
    for name, r, lw in (("equal", rows, np.full(4099, -731.25)), ("one", rows, one), ("far", rows, far), ("dead", rows_nan, dead),
                        ("none", rows, np.full(4099, -np.inf))):
        h = _load(r, lw)
        for ahead in (0, 1):
            got = h.summary(ahead)
            assert _same(got, L.host_ibis_summary(r, r[:, 4], r[:, 5], lw, ahead)), (name, ahead)
            if name in ("one", "far"):
                assert got[2] == 0.0 and got[5] == 0.0
            if name == "dead":
                assert np.isfinite(got[:6]).all() and _same(got, L.host_ibis_summary(rows, rows[:, 4], rows[:, 5], lw, ahead))
            if name == "none":
                assert np.isnan(got[:6]).all()
        h.close()


@pytest.mark.parametrize("case,predict_first", [(c, pf) for c in ("readme", "one") for pf in (False, True)])
def test_device_equals_host_twin_after_sampler_steps(case, predict_first):
    """after smc2 and after every smc2_step of a run with rejuvenations (M = 1000: the last chunk is short): the device
    reduction of the resident cloud == the host twin on the arrays read back, and the public functions return those numbers"""
    y = _y(60)
    ib, tmap = _ibis(case, 1000, predict_first, 5)
    smc.smc2(ib, y)
    for t in range(2, len(y) + 1):
        smc.smc2_step(ib, y, t, verbose=False)
        if t % 4 == 0 or t == len(y):
            for ahead in (0, 1):
                host = _host(ib, tmap, ahead)
                assert _same(ib._h.summary(ahead), host), (t, ahead)
                assert smc.observation_dist(ib, ahead=ahead, between=True) == tuple(host[:3])
            assert smc.filtered_state(ib) == tuple(host[3:6]) and smc.estimated_trend(ib) == _host(ib, tmap, 0)[0]
    assert ib.n_rejuvenations >= 1
    ib.close()


def _stepwise_trace(case, M, y, ahead, p):
    """smc2 + smc2_step with the stand-alone calls after every period -> (trace, ess sequence, final state, rejuvenations)"""
    ib, _ = _ibis(case, M, False, 5)
    trace, ess = [], []
    smc.smc2(ib, y)
    for t in range(1, len(y) + 1):
        if t > 1:
            smc.smc2_step(ib, y, t, verbose=False)
        ess.append(ib.ess)
        yy, Sig, btw = smc.observation_dist(ib, ahead=ahead, between=True)
        xbar, Sbar, _ = smc.filtered_state(ib)
        trace.append((t, yy, Sig, btw, xbar, Sbar, None if p is None else smc.quantile(ib, p, ahead=ahead)))
    state = [getattr(ib, n) for n in ("theta", "x", "Sigma", "logZ", "logw")]
    n = ib.n_rejuvenations
    ib.close()
    return trace, ess, state, n


def _same_trace(a, b):
    assert len(a) == len(b)
    for ea, eb in zip(a, b):
        assert ea[0] == eb[0] and _same(np.array(ea[1:6]), np.array(eb[1:6])), (ea, eb)
        assert (ea[6] is None and eb[6] is None) or _same(ea[6], eb[6]), (ea, eb)


@pytest.mark.parametrize("ahead,p", [(1, None), (0, [0.9, 0.1, 0.5])])
def test_window_recording_equals_stepwise_summaries(ahead, p):
    """smc2_run(summaries=) with windows of 1, 5, 16 and 64 steps over T = 200 with at least 3 resample-moves cutting windows
    short: the same summary_trace for every window length, equal bit for bit to smc2_step followed by observation_dist /
    filtered_state / quantile at every period; no period twice; the state at the end is the stepwise run's"""
    y = _y(200)
    want, _, state, nrej = _stepwise_trace("readme", 512, y, ahead, p)
    assert nrej >= 3
    for window in (1, 5, 16, 64):
        ib, _ = _ibis("readme", 512, False, 5)
        ib.set_summaries(True if p is None else p, ahead)             # (smc2 records period 1)
        smc.smc2(ib, y)
        ib.set_summaries(None)
        smc.smc2_run(ib, y, 2, len(y), window=window, verbose=False, summaries=True if p is None else p, ahead=ahead)
        assert ib.n_rejuvenations == nrej and [e[0] for e in ib.summary_trace] == list(range(1, len(y) + 1))
        _same_trace(ib.summary_trace, want)
        for name, refv in zip(("theta", "x", "Sigma", "logZ", "logw"), state):
            assert np.array_equal(getattr(ib, name), refv), (window, name)
        ib.close()


def test_steps_append_their_period_when_switched_on():
    """ibis.set_summaries: smc2 and smc2_step append their own period; switched off, nothing is appended"""
    y = _y(40)
    want, _, _, _ = _stepwise_trace("one", 77, y, 0, None)
    ib, _ = _ibis("one", 77, False, 5)
    ib.set_summaries(True)
    smc.smc2(ib, y)
    for t in range(2, 31):
        smc.smc2_step(ib, y, t, verbose=False)
    ib.set_summaries(None)
    for t in range(31, 41):
        smc.smc2_step(ib, y, t, verbose=False)
    _same_trace(ib.summary_trace, want[:30])
    ib.close()


def test_summaries_leave_the_run_unchanged():
    """the same run with and without summaries: theta, x, Sigma, logZ, logw and the ESS of every period bit-identical, step by
    step and through windows (the ESS sequence of smc2_run is its verbose log)"""
    y = _y(200)
    _, ess0, state0, nrej = _stepwise_trace("readme", 512, y, 0, None)
    assert nrej >= 3
    ib, _ = _ibis("readme", 512, False, 5)                              # stepwise, no summary call at all
    smc.smc2(ib, y)
    ess = [ib.ess]
    for t in range(2, len(y) + 1):
        smc.smc2_step(ib, y, t, verbose=False)
        ess.append(ib.ess)
    assert ess == ess0 and ib.summary_trace == []
    for name, refv in zip(("theta", "x", "Sigma", "logZ", "logw"), state0):
        assert np.array_equal(getattr(ib, name), refv), name
    ib.close()
    logs = []
    for summaries in (None, [0.05, 0.95]):
        ib, _ = _ibis("readme", 512, False, 5)
        out = io.StringIO()
        smc.smc2(ib, y)
        smc.smc2_run(ib, y, 2, len(y), window=16, verbose=True, out=out, summaries=summaries, ahead=1)
        logs.append(out.getvalue())
        assert ib.ess == ess0[-1] and len(ib.summary_trace) == (0 if summaries is None else len(y) - 1)
        for name, refv in zip(("theta", "x", "Sigma", "logZ", "logw"), state0):
            assert np.array_equal(getattr(ib, name), refv), (summaries, name)
        ib.close()
    assert logs[0] == logs[1] and logs[0].count("ess") >= len(y) - 1


def test_forecast_mean_against_the_grid_posterior():
    """case_one_parameter, M = 2^16, T = 100: observation_dist(ibis, ahead=1)[0] against the posterior predictive mean by
    quadrature (the grid of grid_posterior_A).  Allowed: 5 Monte-Carlo standard errors, FORECAST_SE - the standard error of the
    mean of 16 independent runs of the CPU restatement at M = 512, i.e. the Monte-Carlo sd of an estimate from 8192 particles;
    this run has 8 times as many, so the bound is conservative by about sqrt(8)."""
    from ibis_reference import grid_posterior_A
    y = _y(100)
    grid, grid_A = ref.grid_predictive_mean(y)
    assert grid_A == pytest.approx(grid_posterior_A(y)[0], abs=1e-12)
    ib, _ = _ibis("one", 2 ** 16, False, 1)
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, len(y), window=16, verbose=False, summaries=True, ahead=1)
    got = smc.observation_dist(ib, ahead=1)[0]
    print("forecast mean %.6f, grid %.6f, difference %.2e, allowed %.2e; rejuvenations %d" % (got, grid, got - grid, 5 * FORECAST_SE, ib.n_rejuvenations))
    assert ib.summary_trace[-1][1] == got
    assert abs(got - grid) <= 5.0 * FORECAST_SE
    ib.close()


def test_a_million_particles_with_summaries():
    """M = 2^20, T = 50 through windows with the recording on: T entries, all finite, Sigma > 0"""
    y = _y(50)
    ib, _ = _ibis("one", 2 ** 20, False, 1)
    ib.set_summaries([0.05, 0.5, 0.95], 1)
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, len(y), window=16, verbose=False)
    tr = ib.summary_trace
    assert [e[0] for e in tr] == list(range(1, 51))
    num = np.array([e[1:6] for e in tr])
    assert np.isfinite(num).all() and (num[:, 1] > 0).all() and (num[:, 2] >= 0).all() and (num[:, 4] > 0).all()
    assert all(np.isfinite(e[6]).all() and e[6][0] < e[6][1] < e[6][2] for e in tr)
    assert _same(np.array(smc.observation_dist(ib, ahead=1, between=True)), num[-1, :3])
    ib.close()
