"""The filtered summaries against exact references, on every launch path that computes them (pytest -m gpu).

Mean and variance of every state coordinate are checked against StatsBase's uncorrected weighted moments with exactly rounded
sums, the weighted quantiles by the masses below / at them (tests/summary_reference.py states the tolerances) - NOT against the
oracle, whose arithmetic the kernels mirror.  The state after each step comes from a twin handle driven through the step API
(bit-identical to the whole-series call: its logmu trace is asserted equal); only the state comes from there.

The data give the state a level (LG with A = 1 and x0 up to 1e8, UCSV with its trend at 1e5): there sum w x^2 - mean^2 loses
about eps mean^2 / var of its accuracy.  Paths (tests/test_gpu_paths.py path_of):
  R       k_resident, per step (log_likelihood with set_summaries)     window  k_resident<WIN> (step_window)
  once    k_summ_once (moments() / quantiles() between steps)         S       SMC_FLAG_NO_RESIDENT: the k_ms_* kernels per step
  M1, M2, G   filters of several segments: the k_ms_* kernels (two-level: SMC_MS_TWO_LEVEL, and a filter beyond 2^21 particles)
"""
import math

import numpy as np
import pytest

from summary_reference import VAR_REL, VAR_LEVEL, check_moments, check_quantiles, quantile_delta, ref_moments
from test_gpu_paths import path_of

pytestmark = pytest.mark.gpu

PS = [0.0, 0.05, 0.25, 0.5, 0.75, 0.999, 1.0]
LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
UC = [0.2, 0.2, 3.0, 0.0, 0.0]
UC_LEVEL = [0.2, 0.2, 1e5, 0.0, 0.0]        # UCSV with its trend at 1e5


def lg_level(x0, Q=1.0, R=1.0):
    return [1.0, 1.0, Q, R, x0, 1.0]


# d = 1 data: (name, raw)
DATA = [
    ("lg", LG),
    ("lg1e4", lg_level(1e4)),
    ("lg1e4q", lg_level(1e4, Q=1e-6)),
    ("lg1e6", lg_level(1e6)),
    ("lg1e6q", lg_level(1e6, Q=1e-6)),
    ("lg1e8", lg_level(1e8)),
    ("lg1e8q", lg_level(1e8, Q=1e-6)),
    ("lgm1e6q", lg_level(-1e6, Q=1e-6)),
    ("sharp1e6", lg_level(1e6, Q=1.0, R=1e-6)),
    ("lgc1e8", [1.0, 1.0, 1e-24, 0.01, 1e8, 1.0]),    # spread below one ulp of the level: clusters of equal values (select fallback)
    ("lge", [0.5, 1.0, 0.0, 0.01, 0.3, 0.0]),         # every particle holds the same value: var 0
    ("lge1e6", [1.0, 1.0, 0.0, 0.01, 1e6, 0.0]),
]

# path -> (model, n, seg, flags) shapes of one filter
NO_RESIDENT = 2
SHAPES_D1 = {
    "R": [(1, 2, 0, 0), (1, 3, 0, 0), (1, 1000, 0, 0), (1, 1024, 0, 0), (1, 4096, 0, 0), (1, 8192, 0, 0)],
    "S": [(1, 1024, 0, NO_RESIDENT)],
    "M1": [(1, 9000, 1024, 0)],
    "M2": [(1, 33000, 256, 0)],
    "G": [(1, 70000, 256, 0)],
}
CASES_D1 = [(pid, sh, name, raw) for pid, shs in SHAPES_D1.items() for sh in shs for name, raw in DATA]
IDS_D1 = ["%s-n%d-%s" % (pid, sh[1], name) for pid, sh, name, _ in CASES_D1]


def series(model, raw, T, seed=5):
    from sequential_monte_carlo_amd import _lib as L
    return L.simulate(model, raw, T, seed)[1]


def twin_states(L, model, raws, n, seg, flags, seed, y, on_step=None):
    """the state after each step of a twin handle driven through the step API: [(logmu [nth], x [d][nth][n], w [nth][n])];
    on_step(h, t) runs after step t (the stand-alone summaries between steps)"""
    h = L.Handle(model, len(raws), n, seg=seg, seed=seed, flags=flags)
    h.set_params(raws)
    out = []
    for t in range(len(y)):
        lm = h.init(float(y[0])) if t == 0 else h.step(float(y[t]))[0]
        x, w, _ = h.state(want_anc=False)
        out.append((lm, x, w))
        if on_step:
            on_step(h, t)
    h.close()
    return out


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def check_rows(h, q, mean, var, x, w, comp, ps, ctx):
    """per-filter summaries of one step (q [nth][np], mean / var [d][nth]) against the references of the state (x, w)"""
    for th in range(x.shape[1]):
        for c in range(x.shape[0]):
            check_moments(mean[c, th], var[c, th], x[c, th], w[th], ctx + (th, c))
        if q is not None:
            delta = quantile_delta(h.n_x, h.nseg, h.seg, math.fsum(w[th]))
            check_quantiles(q[th], ps, x[comp, th], w[th], delta, ctx + (th,))


def run_per_step(L, pid, model, raws, n, seg=0, flags=0, T=6, ps=PS, comp=0, seed=23, y=None, once=True):
    """per-step summaries of one log_likelihood call on path pid, and (once) the stand-alone summaries of the twin between steps"""
    raws = np.atleast_2d(np.asarray(raws, dtype=np.float64))
    if y is None:
        y = series(model, raws[0], T)
    h = L.Handle(model, len(raws), n, seg=seg, seed=seed, flags=flags)
    assert path_of(h) == pid, (pid, n, seg, h.nseg, h.resident)
    h.set_params(raws)
    h.set_summaries(ps, comp, moments=True)
    _, lm, _ = h.log_likelihood(y, trace=True)
    q, mean, var = h.get_summaries(len(y))
    once_rows = {}

    def stand_alone(ht, t):
        once_rows[t] = (ht.quantiles(ps, comp), ht.moments())

    states = twin_states(L, model, raws, n, seg, flags, seed, y, stand_alone if once else None)
    for t, (lmt, x, w) in enumerate(states):
        assert same(lmt, lm[t]), (pid, n, t)          # the twin holds the state of the call's step t
        check_rows(h, q[t], mean[t], var[t], x, w, comp, ps, (pid, n, t))
        if once:
            qo, (mo, vo) = once_rows[t]
            check_rows(h, qo, mo, vo, x, w, comp, ps, (pid, "once", n, t))
    h.close()
    return q, mean, var


@pytest.mark.parametrize("pid,shape,name,raw", CASES_D1, ids=IDS_D1)
def test_summaries_exact_d1(L, pid, shape, name, raw):
    """d = 1 on every path, every data set: per-step rows and the stand-alone summaries between steps"""
    model, n, seg, flags = shape
    run_per_step(L, pid, model, [raw], n, seg, flags)


@pytest.mark.parametrize("pid,n,seg,raw", [("R", 512, 0, UC), ("R", 512, 0, UC_LEVEL), ("R", 4096, 0, UC), ("R", 4096, 0, UC_LEVEL),
                                           ("S", 2048, 0, UC_LEVEL), ("M1", 3000, 512, UC_LEVEL), ("M2", 33000, 256, UC_LEVEL),
                                           ("G", 67000, 256, UC_LEVEL)],
                         ids=["R-512", "R-512-level", "R-4096", "R-4096-level", "S-2048-level", "M1-3000-level", "M2-33000-level", "G-67000-level"])
def test_summaries_exact_ucsv(L, pid, n, seg, raw):
    """UCSV (d = 3): all three coordinates' moments, the quantiles of the trend and of a log-volatility"""
    flags = NO_RESIDENT if pid == "S" else 0
    for comp in (0, 2):
        run_per_step(L, pid, 3, [raw], n, seg, flags, T=5, comp=comp, once=comp == 0)


def test_summaries_exact_batch_of_600(L):
    """600 filters of 1024 particles: the resident kernel's 256-thread x two-pair variant (another loop in resident_summaries)"""
    raws = np.tile(lg_level(1e4), (600, 1))
    raws[:, 2] *= 1.0 + np.arange(600) / 600.0        # distinct Q per filter
    run_per_step(L, "R", 1, raws, 1024, T=4, ps=[0.1, 0.5, 0.9], y=series(1, lg_level(1e4), 4), once=False)


@pytest.mark.parametrize("n", [1024, 4096])
@pytest.mark.parametrize("name", ["lg", "lg1e6q", "lg1e8", "lge1e6"])
def test_summaries_exact_window(L, n, name):
    """step_window: the window kernel's per-step summaries after a first log_likelihood call"""
    raw = dict(DATA)[name]
    y = series(1, raw, 10)
    h = L.Handle(1, 1, n, seed=23)
    assert path_of(h) == "R" and h.can_window
    h.set_params([raw])
    h.log_likelihood(y[:4])
    h.set_summaries(PS, 0, moments=True)
    lmw, _ = h.step_window(y[4:])
    q, mean, var = h.get_summaries(6)
    for t, (lmt, x, w) in enumerate(twin_states(L, 1, [raw], n, 0, 0, 23, y)):
        if t >= 4:
            assert same(lmt, lmw[t - 4])
            check_rows(h, q[t - 4], mean[t - 4], var[t - 4], x, w, 0, PS, ("window", n, name, t))
    h.close()


@pytest.mark.parametrize("name", ["lg", "lg1e6q", "lgc1e8"])
def test_summaries_exact_two_level(L, name, monkeypatch):
    """the second level of the multi-segment selection (filters beyond 2^21 particles) at a small size, through its knob"""
    monkeypatch.setenv("SMC_MS_TWO_LEVEL", "1000")
    run_per_step(L, "M1", 1, [dict(DATA)[name]], 9000, 1024, T=4)


@pytest.mark.parametrize("name", ["lg", "lg1e6q"])
def test_summaries_exact_beyond_two_level_size(L, name):
    """one real filter above 2^21 particles (ragged): the two-level selection without the knob"""
    n = (1 << 21) + 4097
    run_per_step(L, "G", 1, [dict(DATA)[name]], n, T=3, ps=[0.05, 0.5, 0.95], once=False)


@pytest.mark.parametrize("pid,n,seg,flags", [("R", 1024, 0, 0), ("R", 1000, 0, 0), ("S", 1024, 0, NO_RESIDENT), ("M1", 9000, 1024, 0),
                                             ("G", 70000, 256, 0)])
def test_collapsed_filter_has_nan_summaries(L, pid, n, seg, flags):
    """a step after which every weight is 0: NaN mean, var and quantiles - in the per-step rows and from moments() / quantiles()
    between steps; the steps around it are exact"""
    raw = lg_level(1e6)
    y = series(1, raw, 5)
    y[2] = 1e200                                       # (y - x)^2 / R overflows: every log-weight is -inf
    q, mean, var = run_per_step(L, pid, 1, [raw, lg_level(1e6, Q=2.0)], n, seg, flags, y=y)
    assert np.all(np.isnan(q[2])) and np.all(np.isnan(mean[2])) and np.all(np.isnan(var[2]))
    assert np.all(np.isfinite(mean[[0, 1, 3, 4]])) and np.all(np.isfinite(var[[0, 1, 3, 4]]))


def test_large_offset_filtered_variance_matches_kalman(L):
    """LG with A = 1, 2^18 particles (several segments), at level 0 and 1e6 with the series shifted by the same constant: the
    filtered variance averaged over the steps equals the exact Kalman variance within the Monte-Carlo error, and the two levels
    agree.  Bound: a weighted variance of ESS effective draws has relative sd about sqrt(2 / ESS) per step; the steps are not
    independent, so no credit is taken for the average: |mean_t(var_t / P_t) - 1| <= 5 sqrt(2 / min ESS)."""
    import sequential_monte_carlo_amd as smc
    T, n = 16, 1 << 18
    base = smc.UnivariateLinearGaussian(A=1.0, B=1.0, Q=1.0, R=1.0, x0=0.0, sigma0=1.0)
    _, y0 = smc.simulate(base, T, seed=77)
    ratios, bounds = {}, []
    for off in (0.0, 1e6):
        m = smc.UnivariateLinearGaussian(A=1.0, B=1.0, Q=1.0, R=1.0, x0=off, sigma0=1.0)
        y = y0 + off
        h = L.Handle(1, 1, n, seed=5)
        assert path_of(h) in ("M1", "M2", "G")
        h.set_params([m.raw()])
        h.set_summaries(None, moments=True)
        _, _, ess = h.log_likelihood(y, trace=True)
        _, mean, var = h.get_summaries(T)
        h.close()
        P = np.array([smc.log_likelihood_kalman(y[:t + 1], m)[1] for t in range(T)])
        xk = np.array([smc.log_likelihood_kalman(y[:t + 1], m)[0] for t in range(T)])
        assert np.all(var[:, 0, 0] > 0)
        r = var[:, 0, 0] / P
        bound = 5 * math.sqrt(2.0 / ess.min())
        assert abs(r.mean() - 1) <= bound, (off, r, bound)
        assert np.all(np.abs(mean[:, 0, 0] - xk) <= 6 * np.sqrt(P / ess[:, 0]) + 1e-9 * abs(off)), off
        ratios[off] = r.mean()
        bounds.append(bound)
    assert abs(ratios[0.0] - ratios[1e6]) <= max(bounds), (ratios, bounds)


def test_filtered_summaries_after_smc2_step_at_a_level():
    """filtered_summaries after smc2_step for LG with A = 1 and x0 = 1e6 held constant (the level does not decay): the integrated
    variance is sum_m omega_m v_m of the per-filter references, within the variance tolerance"""
    import sequential_monte_carlo_amd as smc
    tmap = smc.ThetaMap(1, [-1, -1, 0, 1, -1, -1], [1.0, 1.0, 0.0, 0.0, 1e6, 1.0])

    def mod(th):
        return smc.UnivariateLinearGaussian(A=1.0, B=1.0, Q=th[0], R=th[1], x0=1e6, sigma0=1.0)

    prior = smc.product_distribution([smc.LogNormal(), smc.LogNormal()])
    _, y = smc.simulate(mod([0.5, 0.5]), 8, seed=1998)
    s = smc.SMC(512, 16, mod, prior, 2, 0.5, seed=7, theta_map=tmap)
    smc.smc2(s, y)
    for t in range(2, 6):
        smc.smc2_step(s, y, t, verbose=False)
    q, v = smc.filtered_summaries(s, [0.1, 0.5, 0.9])
    x, w, _ = s._main.state(want_anc=False)
    om = np.asarray(s.omega)
    refs = [ref_moments(x[0, m], w[m]) for m in range(s.M)]
    V = math.fsum(om[m] * refs[m][1] for m in range(s.M) if om[m] > 0)
    slack = math.fsum(om[m] * (VAR_LEVEL * refs[m][0]) ** 2 for m in range(s.M) if om[m] > 0)
    assert np.all(np.isfinite(q)) and v >= 0
    assert abs(v - V) <= VAR_REL * V + slack, (v, V)
    trend = smc.estimated_trend(s)
    assert abs(trend - math.fsum(om[m] * refs[m][0] for m in range(s.M) if om[m] > 0)) <= 1e-11 * 1e6
