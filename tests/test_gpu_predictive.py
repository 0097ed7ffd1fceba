"""Predictive checks on the GPU (pytest -m gpu; csrc/smc_spec.h "predictive checks").

  * smc_device_normcdf == smc_host_normcdf bit for bit on the grid of the CPU test
  * smc_get_predictive == smc_host_predictive on the smc_get_state cloud, bit for bit: three families, 1 and 3 filters with distinct
    rows, ragged and padded clouds, both sides of the small / large switch (and the large launches forced at small sizes), both
    resamplers, a flagged handle at a gap
  * smc_predictive over a record == the rows smc_get_predictive gave step by step; the filter is the filter that never asked
  * the refusals and what they leave; the Python layer's shapes
  * meaning: the rows of 64 independent LG1D filters against the exact Kalman rows, self-normalising
  * smc_kalman_predictive_flags == its host twin
(the host twins are pinned to independent references by tests/test_predictive_host.py)
"""
import math
import os

import numpy as np
import pytest

import predictive_reference as ref
import test_gpu_smoother as G

pytestmark = pytest.mark.gpu

RAW = G.RAW
same, rows_for = G.same, G.rows_for
SYSTEMATIC = G.SYSTEMATIC
EINVAL, ESTATE = -1, -3


class small_max:
    """the switch between the one-workgroup kernel and the launches per level, lowered for the calls inside"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.old = os.environ.get("SMC_PRED_SMALL_MAX")
        os.environ["SMC_PRED_SMALL_MAX"] = str(self.v)

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["SMC_PRED_SMALL_MAX"]
        else:
            os.environ["SMC_PRED_SMALL_MAX"] = self.old


def handle(L, model, rows, n, seg=0, flags=0, seed=11, proposal=0):
    rows = np.atleast_2d(rows)
    h = L.Handle(model, rows.shape[0], n, seg=seg, seed=seed, flags=flags)
    h.set_params(rows)
    h.set_streams(np.arange(rows.shape[0]))
    if proposal:
        h.set_proposal(proposal)
    return h


def check_current(L, h, model, rows, y_t, nan_pit=False):
    """smc_get_predictive of the handle == the host twin on the cloud smc_get_state hands over -> the rows"""
    got = np.array(h.predictive(y_t))                        # [3][n_theta]
    x, _, _ = h.state(want_w=False, want_anc=False)          # [d][n_theta][n]
    for th in range(h.n_theta):
        want = L.host_predictive(model, rows[th], x[:, th, :], y_t)
        if nan_pit:
            assert got[0, th] != got[0, th] and want[0] != want[0]
            assert same(got[1:, th], want[1:]), th
        else:
            assert same(got[:, th], want), (th, got[:, th], want)
    return got


def test_device_normcdf_equals_host(L):
    z = ref.normcdf_grid()
    d, h = L.device_normcdf(z), L.host_normcdf(z)
    nan = z != z
    assert same(d[~nan], h[~nan]) and np.all(d[nan] != d[nan])
    assert np.all((d[~nan] >= 0.0) & (d[~nan] <= 1.0))


# (n_x, seg): the automatic segment; 1025 in segments of 256 (five segments, the rows padded to 1280)
SHAPES = [(2, 0), (127, 0), (129, 0), (1000, 0), (1025, 256)]


@pytest.mark.parametrize("model", [1, 2, 3])
@pytest.mark.parametrize("nth", [1, 3])
@pytest.mark.parametrize("n,seg", SHAPES)
def test_current_state_equals_host_twin(L, model, nth, n, seg):
    rows = rows_for(RAW[model], nth)
    _, y = L.simulate(model, RAW[model], 3, 1998)
    flags = SYSTEMATIC if (n + nth) % 2 else 0                # both resamplers, each with every family
    h = handle(L, model, rows, n, seg, flags)
    h.init(float(y[0]))
    a = check_current(L, h, model, rows, float(y[0]))
    h.step(float(y[1]))
    h.step(float(y[2]))
    b = check_current(L, h, model, rows, float(y[2]))
    assert np.all((b[0] >= 0) & (b[0] <= 1)) and np.all(b[2] > 0) and not same(a, b)
    with small_max(0):                                        # the launches per level on the same cloud: the same bits
        assert same(np.array(h.predictive(float(y[2]))), b)
    h.close()


@pytest.mark.parametrize("model", [1, 3])
def test_both_sides_of_the_switch(L, model):
    """the largest cloud the library finishes in one workgroup and the first it gives a launch per level; the same at the most one
    workgroup can hold, 128^2, whose successor has three levels of sums (129 partials, then 2, then 1)"""
    top, chunk = L.predictive_constants()
    assert top == 4096 and chunk == 128
    _, y = L.simulate(model, RAW[model], 2, 1998)
    for n in (top, top + 1, chunk * chunk, chunk * chunk + 1):
        h = handle(L, model, RAW[model], n, 1024)
        h.init(float(y[0]))
        h.step(float(y[1]))
        got = check_current(L, h, model, np.atleast_2d(RAW[model]), float(y[1]))
        if n in (top, chunk * chunk):                         # the other kernel on the same cloud
            with small_max(chunk * chunk if n > top else 1024):
                assert L.predictive_constants()[0] == (chunk * chunk if n > top else 1024)
                assert same(np.array(h.predictive(float(y[1]))), got)
        h.close()


def test_gap_of_a_flagged_handle(L):
    """a NaN y: a NaN pit beside the forecast moments of the unobserved y_t, on a handle that takes the missing step"""
    rows = rows_for(RAW[1], 3)
    _, y = L.simulate(1, RAW[1], 3, 1998)
    h = handle(L, 1, rows, 300, 256, L.FLAG_NAN_MISSING)
    h.init(float(y[0]))
    h.step(math.nan)
    got = check_current(L, h, 1, rows, math.nan, nan_pit=True)
    assert np.all(np.isfinite(got[1:]))
    h.step(float(y[2]))
    check_current(L, h, 1, rows, float(y[2]))
    check_current(L, h, 1, rows, math.inf)
    assert same(np.array(h.predictive(-math.inf))[0], np.zeros(3))
    h.close()


def run(L, model, rows, n, seg, y, ask, record=False, flags=0):
    """T steps of the step API; ask: smc_get_predictive after every step -> (handle, per-step rows or None, per-step logmu)"""
    h = handle(L, model, rows, n, seg, flags)
    if record:
        h.history_begin(len(y) + 1)                           # (room for one step more: the caller compares the step that follows)
    out, lms = [], []
    for t, yt in enumerate(y):
        lms.append(h.init(float(yt)) if t == 0 else h.step(float(yt))[0])
        if ask:
            out.append(np.array(h.predictive(float(yt))))
    return h, (np.array(out) if ask else None), np.array(lms)


@pytest.mark.parametrize("model,n,seg", [(1, 300, 256), (2, 1000, 0), (3, 129, 0)])
def test_record_equals_step_by_step_and_nothing_changes(L, model, n, seg):
    rows = rows_for(RAW[model], 3)
    _, y = L.simulate(model, RAW[model], 7, 1998)
    ha, asked, lma = run(L, model, rows, n, seg, y[:6], ask=True, record=True)
    pit, m, v = ha.predictive_record(y[:6])                   # [T][n_theta] each, one launch
    assert pit.shape == (6, 3)
    assert same(pit, asked[:, 0]) and same(m, asked[:, 1]) and same(v, asked[:, 2])
    with small_max(128):
        assert all(same(u, w) for u, w in zip(ha.predictive_record(y[:6]), (pit, m, v)))
    hb, _, lmb = run(L, model, rows, n, seg, y[:6], ask=False, record=True)
    xa, wa, _ = ha.state(want_anc=False)
    xb, wb, _ = hb.state(want_anc=False)
    assert same(xa, xb) and same(wa, wb) and same(lma, lmb) and same(ha.logZ()[0], hb.logZ()[0])
    la, lb = ha.step(float(y[6])), hb.step(float(y[6]))       # the next step's logmu and ess
    assert same(la[0], lb[0]) and same(la[1], lb[1])
    ha.close()
    hb.close()


def test_refusals(L):
    lib, dp = L.lib(), L._d
    _, y = L.simulate(1, RAW[1], 4, 1998)
    yy, out = np.ascontiguousarray(y), np.zeros((3, 4, 2))

    def get(h):
        return lib.smc_get_predictive(h._h, float(y[0]), dp(out[0]), dp(out[1]), dp(out[2]))

    def rec(h, T):
        return lib.smc_predictive(h._h, dp(yy), T, dp(out[0]), dp(out[1]), dp(out[2]))

    # a proposal, the conditional flag, the marginal family: SMC_EINVAL with the reason, and the next step is the step of a twin
    guided = [handle(L, 1, rows_for(RAW[1], 2), 300, 256, proposal=G.OPTIMAL) for _ in range(2)]
    cond = [handle(L, 1, rows_for(RAW[1], 2), 300, 256, L.FLAG_CONDITIONAL) for _ in range(2)]
    marg = [handle(L, 4, rows_for(RAW[3], 2), 300, 256) for _ in range(2)]
    for (h, twin), word in ((guided, "proposal"), (cond, "conditional"), (marg, "UCSV_RB")):
        for k in (h, twin):
            if k in cond:
                k.set_reference(np.zeros((4, 1, 2)))
            k.history_begin(4)
            k.init(float(y[0]))
        assert get(h) == EINVAL and word in lib.smc_last_error().decode()
        assert rec(h, 1) == EINVAL and word in lib.smc_last_error().decode()
        a, b = h.step(float(y[1])), twin.step(float(y[1]))
        assert same(a[0], b[0]) and same(h.state(want_anc=False)[0], twin.state(want_anc=False)[0])
        h.close()
        twin.close()
    # state rules: not initialised; no record; a record of another length
    h = handle(L, 1, rows_for(RAW[1], 2), 300, 256)
    assert get(h) == ESTATE
    h.init(float(y[0]))
    assert get(h) == 0
    assert rec(h, 1) == ESTATE                                # not armed
    h.close()
    h = handle(L, 1, rows_for(RAW[1], 2), 300, 256)
    h.history_begin(4)
    assert rec(h, 0) == ESTATE                                # armed, nothing recorded
    h.init(float(y[0]))
    h.step(float(y[1]))
    assert rec(h, 3) == EINVAL and rec(h, 1) == EINVAL and rec(h, 2) == 0
    assert lib.smc_get_predictive(h._h, float(y[1]), None, None, None) == 0       # any NULL
    h.close()


def test_python_shapes(L):
    import sequential_monte_carlo_amd as smc
    m1, m2 = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8), smc.UnivariateLinearGaussian(A=0.7, B=1.0, Q=0.5, R=0.8)
    _, y = smc.simulate(m1, 8)
    x, w, logZ, s = smc.log_likelihood(256, y, m1, seed=5, predictive=True)
    assert isinstance(logZ, float) and all(s[k].shape == (8,) for k in ("pit", "obs_mean", "obs_var"))
    pit, om, ov = x.predictive(y[-1])
    assert pit == s["pit"][-1] and om == s["obs_mean"][-1] and ov == s["obs_var"][-1]
    _, _, z2, s2 = smc.smoother(256, y, m1, seed=5, predictive=True)       # the record in one launch: the same filter, the same bits
    assert z2 == logZ and all(same(s2[k], s[k]) for k in ("pit", "obs_mean", "obs_var"))
    _, _, zl, lm, es, sl = smc.log_likelihood(256, y, [m1, m2], seed=5, trace=True, predictive=True)
    assert zl.shape == (2,) and lm.shape == (8, 2) and all(sl[k].shape == (8, 2) for k in ("pit", "obs_mean", "obs_var"))
    assert same(sl["pit"][:, 0], s["pit"])
    k1 = smc.kalman_predictive(y, smc.LinearModel(0.5, 1.0, 0.9, 0.8))
    k2 = smc.kalman_predictive(y, [smc.LinearModel(0.5, 1.0, 0.9, 0.8), smc.LinearModel(0.7, 1.0, 0.5, 0.8)])
    assert all(a.shape == (8,) for a in k1) and all(a.shape == (8, 2) for a in k2) and same(k2[0][:, 0], k1[0])
    assert np.all(np.isfinite(smc.pit_residuals(s["pit"])))
    yg = y.copy()
    yg[3] = math.nan
    kg = smc.kalman_predictive(yg, smc.LinearModel(0.5, 1.0, 0.9, 0.8), missing=True)
    assert kg[0][3] != kg[0][3] and np.isfinite(kg[1][3]) and np.isfinite(kg[0][4])


def test_meaning_against_the_exact_kalman_rows(L):
    """LG1D, the README row, T = 40, 64 independent filters of 512 particles in one handle.  For each of pit, obs_mean, obs_var:
    max_t |mean over filters - Kalman| / (sd over filters / 8) <= 5.  A numpy bootstrap filter of the same sizes gave maxima
    between 1.8 and 3.3 in nine runs; the chance of 5 among 120 normal scores is below 1e-4."""
    T, K, n = 40, 64, 512
    rows = np.tile(np.asarray(RAW[1], dtype=float), (K, 1))
    _, y = L.simulate(1, RAW[1], T, 1998)
    h, asked, _ = run(L, 1, rows, n, 0, y, ask=True)          # [T][3][K]
    h.close()
    exact = np.array(L.kalman_predictive(np.asarray(RAW[1], dtype=float), y))[:, :, 0]      # [3][T]
    for q, name in enumerate(("pit", "obs_mean", "obs_var")):
        score = np.abs(asked[:, q].mean(axis=1) - exact[q]) / (asked[:, q].std(axis=1, ddof=1) / 8.0)
        print("%s: largest score %.2f at t = %d" % (name, score.max(), int(score.argmax())))
        assert score.max() <= 5.0, (name, score.max())


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("nth", [1, 65, 130])
def test_kalman_rows_equal_host_twin(L, nth, gaps):
    rng = np.random.default_rng(nth)
    rows = np.tile(np.asarray(ref.README_ROW), (nth, 1))
    rows[:, 0] = rng.uniform(-0.95, 0.999, nth)
    rows[:, 2:4] *= rng.uniform(0.2, 3.0, (nth, 2))
    rows[:, 4] = rng.normal(size=nth)
    _, y = L.simulate(1, ref.README_ROW, 30, 7)
    if gaps:
        y[[0, 5, 6, 29]] = math.nan
    for pf in (False, True):
        dev = L.kalman_predictive(rows, y, predict_first=pf, missing=gaps)
        for m in range(nth):
            host = L.host_kalman_predictive(rows[m], y, predict_first=pf, missing=gaps)
            for q in range(3):
                assert ref.same_or_both_nan(dev[q][:, m], host[q]), (m, q)
        assert np.all(np.isnan(dev[0][np.isnan(y)])) and np.all(np.isfinite(dev[0][~np.isnan(y)]))
