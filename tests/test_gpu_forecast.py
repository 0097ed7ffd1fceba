"""Forecasts on the device (smc_forecast, smc_forecast_cloud; pytest -m gpu): the propagated clouds against the host twin bit for
bit, the per-horizon summaries against exact references computed from those clouds, the handle read and never written, a collapsed
filter, a guided handle, the Python layer, the argument errors and the exact Kalman one-step prediction.

Shapes (include/smc_hip.h "forecasts"; the smallest at which the kernel can go wrong): seg = 256 with n_x = 301 (one segment, odd
count, half-valid last pair, padding), seg = 256 with n_x = 805 (four segments, the last partial and odd), automatic seg with
n_x = 1024 (the resident-path geometry); three filters with distinct parameter rows and the streams (5, 0, 9); T = 6 filter steps
first; H in {1, 5}."""
import math

import numpy as np
import pytest

import nonfinite_inputs as NF
from summary_reference import MEAN_REL, MEAN_SD, VAR_LEVEL, VAR_REL, check_moments, check_quantiles, quantile_delta, ref_moments

pytestmark = pytest.mark.gpu

LG1D, SV1D, UCSV3D, UCSV_RB = 1, 2, 3, 4
MODELS = [LG1D, SV1D, UCSV3D, UCSV_RB]
RAWS = {
    LG1D: [[0.5, 1.0, 0.9, 0.8, 0.0, 1.0], [0.9, 0.7, 0.3, 1.2, 0.5, 2.0], [-0.6, 1.5, 1.1, 0.5, -1.0, 0.5]],
    SV1D: [[-1.0, 0.95, 0.25], [0.5, 0.8, 0.4], [-0.3, -0.5, 0.6]],
    UCSV3D: [[0.2, 0.2, 3.0, 0.0, 0.0], [0.3, 0.1, 1.0, -0.5, 0.2], [-0.25, 0.15, -2.0, 0.3, -0.4]],
}
RAWS[UCSV_RB] = RAWS[UCSV3D]
SHAPES = [(256, 301), (256, 805), (0, 1024)]
SHAPE_IDS = ["seg256-n301", "seg256-n805", "auto-n1024"]
STREAMS = [5, 0, 9]
T, FSEED = 6, 0x5EEDF0CA57
PS = [0.0, 0.05, 0.5, 0.9, 1.0]
_Y = {}


def series(L, model):
    if model not in _Y:
        _Y[model] = L.simulate(model, RAWS[model][0], T + 2, 5)[1]
    return _Y[model]


def filtered(L, model, seg, n, raws=None, seed=3, steps=T, history=0, proposal=None):
    """a batch of three filters after `steps` steps of the step API"""
    raws = RAWS[model] if raws is None else raws
    h = L.Handle(model, len(raws), n, seg=seg, seed=seed)
    h.set_params(raws)
    h.set_streams(STREAMS[:len(raws)])
    if proposal is not None:
        h.set_proposal(proposal)
    if history:
        h.history_begin(history)
    y = series(L, model)
    h.init(float(y[0]))
    for t in range(1, steps):
        h.step(float(y[t]))
    return h


def same(a, b):
    return NF.same_nan(a, b)


def host_twin(L, model, raws, x, H, seed=FSEED):
    """smc_host_forecast of every filter of a batch on the device's own state x [d][nth][n]: (xf [H][d][nth][n], yf, ym, yv [H][nth][n])"""
    per = [L.host_forecast(model, raws[th], x[:, th], H, seed, stream=STREAMS[th]) for th in range(x.shape[1])]
    return tuple(np.stack([p[k] for p in per], axis=2 if k == 0 else 1) for k in range(4))


# ---- 1. clouds == host twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg,n", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("model", MODELS)
def test_clouds_equal_the_host_twin(L, monkeypatch, model, seg, n):
    """smc_forecast_cloud == smc_host_forecast on the x of smc_get_state, bit for bit, for every filter, H in {1, 5} and horizon
    blocks of 1, 2 (5 is no multiple of it) and the default"""
    h = filtered(L, model, seg, n)
    x, _, _ = h.state(want_w=False, want_anc=False)
    ref_x, ref_y, _, _ = host_twin(L, model, RAWS[model], x, 5)
    for block in ("1", "2", None):
        if block is None:
            monkeypatch.delenv("SMC_FORECAST_BLOCK", raising=False)
        else:
            monkeypatch.setenv("SMC_FORECAST_BLOCK", block)
        for H in (1, 5):
            xf, yf = h.forecast_cloud(H, FSEED)
            assert xf.shape == (H, h.d, 3, n) and yf.shape == (H, 3, n)
            assert same(xf, ref_x[:H]) and same(yf, ref_y[:H]), (model, n, block, H)
    xf_only, none = h.forecast_cloud(2, FSEED, want_y=False)
    assert none is None and same(xf_only, ref_x[:2])
    h.close()


# ---- 2. summaries against exact references ---------------------------------------------------------------------------------------
def check_forecast_rows(L, h, model, f, H, comp):
    x, w, _ = h.state(want_anc=False)
    xf, yf = h.forecast_cloud(H, FSEED)
    _, _, ym, yv = host_twin(L, model, RAWS[model], x, H)        # (the clouds are the twin's: test 1; ym, yv come from it)
    for k in range(H):
        for th in range(3):
            ctx = (model, h.n_x, k, th)
            for c in range(h.d):
                check_moments(f["mean"][k, c, th], f["var"][k, c, th], xf[k, c, th], w[th], ctx + (c,))
            delta = quantile_delta(h.n_x, h.nseg, h.seg, math.fsum(w[th]))
            check_quantiles(f["q"][k, th], PS, xf[k, comp, th], w[th], delta, ctx + ("q",))
            check_quantiles(f["obs_q"][k, th], PS, yf[k, th], w[th], delta, ctx + ("obs_q",))
            m1, v1 = ref_moments(ym[k, th], w[th])
            m2, v2 = ref_moments(yv[k, th], w[th])
            om, ov = f["obs_mean"][k, th], f["obs_var"][k, th]
            assert abs(om - m1) <= MEAN_REL * abs(m1) + MEAN_SD * math.sqrt(v1), ctx + ("obs_mean", om, m1)
            # obs_var = (variance of ym) + (mean of yv): the sum of the bounds of its two terms
            bound = (VAR_REL * v1 + (VAR_LEVEL * m1) ** 2) + (MEAN_REL * abs(m2) + MEAN_SD * math.sqrt(v2))
            assert math.isfinite(ov) and ov >= 0 and abs(ov - (v1 + m2)) <= bound, ctx + ("obs_var", ov, v1 + m2, bound)


@pytest.mark.parametrize("seg,n", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("model", MODELS)
def test_summaries_against_exact_references(L, model, seg, n):
    h = filtered(L, model, seg, n)
    comp = min(1, h.d - 1)
    for H in (1, 5):
        f = h.forecast(H, FSEED, p=PS, component=comp)
        assert f["mean"].shape == (H, h.d, 3) and f["q"].shape == (H, 3, len(PS)) and f["obs_var"].shape == (H, 3)
        check_forecast_rows(L, h, model, f, H, comp)
    h.close()


@pytest.mark.parametrize("model", MODELS)
def test_summaries_two_level_selection(L, monkeypatch, model):
    """the multi-segment shape with SMC_MS_TWO_LEVEL=0: the second cut of the chosen bins at 805 particles"""
    monkeypatch.setenv("SMC_MS_TWO_LEVEL", "0")
    h = filtered(L, model, 256, 805)
    f = h.forecast(5, FSEED, p=PS, component=0)
    check_forecast_rows(L, h, model, f, 5, 0)
    h.close()


def test_outputs_are_optional(L):
    h = filtered(L, LG1D, 256, 805)
    full = h.forecast(3, FSEED, p=PS)
    nobs = h.forecast(3, FSEED, p=PS, obs=False)
    assert set(nobs) == {"mean", "var", "q"} and all(same(nobs[k], full[k]) for k in nobs)
    noq = h.forecast(3, FSEED)
    assert "q" not in noq and "obs_q" not in noq and all(same(noq[k], full[k]) for k in noq)
    h.close()


# ---- 3. the handle is read, never written ------------------------------------------------------------------------------------------
def snapshot(h):
    x, w, _ = h.state(want_anc=False)
    return (x, w) + tuple(h.weights_raw()) + tuple(h.logZ())


def same_snapshot(a, b):
    return all(np.array_equal(p, q) if p.dtype.kind in "iu" else same(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("seg,n", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("model", MODELS)
def test_forecast_leaves_the_handle_alone(L, model, seg, n):
    h, twin = filtered(L, model, seg, n), filtered(L, model, seg, n)
    before = snapshot(h)
    h.forecast(5, FSEED, p=PS)
    h.forecast_cloud(5, FSEED)
    assert same_snapshot(before, snapshot(h))
    y = series(L, model)
    for t in (T, T + 1):
        a, b = h.step(float(y[t])), twin.step(float(y[t]))
        assert same(a[0], b[0]) and same(a[1], b[1])
    assert same_snapshot(snapshot(h), snapshot(twin))
    h.close(); twin.close()


@pytest.mark.parametrize("model", MODELS)
def test_forecast_between_window_and_commit(L, model):
    """a pending window (smc_step_window) survives a forecast: the commit gives the twin's bits"""
    h, twin = filtered(L, model, 0, 1024), filtered(L, model, 0, 1024)
    assert h.can_window
    y = series(L, model)[T:T + 2]
    a, b = h.step_window(y), twin.step_window(y)
    assert same(a[0], b[0]) and same(a[1], b[1])
    f1 = h.forecast(5, FSEED, p=PS)
    h.forecast_cloud(5, FSEED)
    h.step_commit(2); twin.step_commit(2)
    assert same_snapshot(snapshot(h), snapshot(twin))
    f2 = twin.forecast(5, FSEED, p=PS)
    assert not same(f1["mean"], f2["mean"])          # (the forecast saw the state BEFORE the window, the twin's the one after)
    h.close(); twin.close()


@pytest.mark.parametrize("model", MODELS)
def test_forecast_of_a_recording_handle(L, model):
    """history_begin mode: the record is neither read nor extended by a forecast"""
    h, twin = filtered(L, model, 256, 805, history=T + 2), filtered(L, model, 256, 805, history=T + 2)
    h.forecast(5, FSEED, p=PS)
    h.forecast_cloud(5, FSEED)
    assert h.history_len() == twin.history_len() == T
    y = series(L, model)
    for t in (T, T + 1):
        h.step(float(y[t])); twin.step(float(y[t]))
    assert h.history_len() == twin.history_len() == T + 2
    for t in range(T + 2):
        a, b = h.history_get(t), twin.history_get(t)
        assert same(a[0], b[0]) and same(a[1], b[1]), t
    assert same_snapshot(snapshot(h), snapshot(twin))
    h.history_end(); twin.history_end()
    h.close(); twin.close()


# ---- 4. a collapsed filter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg,n", SHAPES[:2], ids=SHAPE_IDS[:2])
def test_collapsed_filter_reads_nan(L, seg, n):
    bad = [r for r in NF.BAD_ROWS if r[0] == "lg-R<0"][0][2]
    good = RAWS[LG1D]
    hb, hg = filtered(L, LG1D, seg, n, raws=[good[0], bad, good[2]]), filtered(L, LG1D, seg, n)
    assert np.all(hb.state(want_anc=False)[1][1] == 0)                     # every weight of the middle filter is 0
    fb, fg = hb.forecast(5, FSEED, p=PS), hg.forecast(5, FSEED, p=PS)
    for key in ("mean", "var"):
        assert np.all(np.isnan(fb[key][:, :, 1])), key
        assert same(fb[key][:, :, [0, 2]], fg[key][:, :, [0, 2]]), key
    for key in ("q", "obs_q", "obs_mean", "obs_var"):
        assert np.all(np.isnan(fb[key][:, 1])), key
        assert same(fb[key][:, [0, 2]], fg[key][:, [0, 2]]), key
    xb, yb = hb.forecast_cloud(5, FSEED)
    xg, yg = hg.forecast_cloud(5, FSEED)
    assert same(xb[:, :, [0, 2]], xg[:, :, [0, 2]]) and same(yb[:, [0, 2]], yg[:, [0, 2]])
    hb.close(); hg.close()


# ---- 5. a guided handle forecasts by the transition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seg,n", SHAPES, ids=SHAPE_IDS)
def test_guided_handle_forecasts_by_the_transition(L, seg, n):
    g = filtered(L, LG1D, seg, n, proposal=L.PROP_OPTIMAL)
    b = filtered(L, LG1D, seg, n)
    assert not same(g.state(want_anc=False)[0], b.state(want_anc=False)[0])
    b.copy_from(g, [1, 1, 1])                                              # the bootstrap handle holds the guided one's state
    assert same_snapshot(snapshot(g)[:2], snapshot(b)[:2])            # x and w
    xg, yg = g.forecast_cloud(5, FSEED)
    xb, yb = b.forecast_cloud(5, FSEED)
    assert same(xg, xb) and same(yg, yb)
    fg, fb = g.forecast(5, FSEED, p=PS), b.forecast(5, FSEED, p=PS)
    assert all(same(fg[k], fb[k]) for k in fg)
    ref_x, _, _, _ = host_twin(L, LG1D, RAWS[LG1D], g.state(want_anc=False)[0], 5)
    assert same(xg, ref_x)
    g.close(); b.close()


# ---- 6. the Python layer -----------------------------------------------------------------------------------------------------------
def test_python_forecast_shapes(L):
    import sequential_monte_carlo_amd as smc
    y = series(L, UCSV3D)[:T]
    r0 = RAWS[UCSV3D][0]
    m = smc.UCSV((r0[0], r0[1]), r0[2], (r0[3], r0[4]))
    x, w, _ = smc.log_likelihood(301, y, m, seed=4, seg=256)
    f = smc.forecast(x, w, 5, quantiles=[0.1, 0.5, 0.9], component=1, clouds=True)
    assert f["mean"].shape == f["var"].shape == (5, 3) and f["quantiles"].shape == f["obs_quantiles"].shape == (5, 3)
    assert f["obs_mean"].shape == f["obs_var"].shape == (5,) and f["x"].shape == (5, 301, 3) and f["y"].shape == (5, 301)
    ww = np.asarray(w)
    assert abs(float(np.sum(ww * f["x"][2, :, 0])) - f["mean"][2, 0]) <= 1e-9 * (1 + abs(f["mean"][2, 0]))
    again = smc.forecast(x, w, 3, quantiles=[0.1, 0.5, 0.9], component=1)
    assert "x" not in again and same(again["mean"], f["mean"][:3]) and same(again["obs_quantiles"], f["obs_quantiles"][:3])
    assert not same(smc.forecast(x, w, 3, seed=99)["mean"], again["mean"])
    ms = [smc.UnivariateLinearGaussian(A=r[0], B=r[1], Q=r[2], R=r[3], x0=r[4], sigma0=r[5]) for r in RAWS[LG1D]]
    xs, ws, _ = smc.log_likelihood(805, series(L, LG1D)[:T], ms, seed=4, seg=256)
    fb = smc.forecast(xs, ws, 2, quantiles=[0.5], clouds=True)
    assert fb["mean"].shape == fb["var"].shape == fb["obs_mean"].shape == (2, 3) and fb["quantiles"].shape == (2, 3, 1)
    assert fb["x"].shape == fb["y"].shape == (2, 3, 805)
    none = smc.forecast(xs, ws, 2)
    assert "quantiles" not in none and "obs_quantiles" not in none
    rb = smc.MarginalUCSV((r0[0], r0[1]), r0[2], (r0[3], r0[4]))
    xr, wr, _ = smc.log_likelihood(301, y, rb, seed=4, seg=256)
    fr = smc.forecast(xr, wr, 2)
    tm, tv = smc.trend_moments(fr["mean"][1], fr["var"][1])
    assert tm == fr["mean"][1, 0] and tv == fr["var"][1, 0] + fr["mean"][1, 3]
    assert abs(fr["obs_mean"][1] - tm) <= 1e-12 * (1 + abs(tm))            # E[y] is the trend's mean
    with pytest.raises(ValueError):
        smc.forecast(x, wr, 2)


def test_forecast_state_integrates_over_theta(L):
    """smc.forecast_state on SMC(256, 24, ...) over T = 20 == the integration recomputed in numpy from the per-filter
    Handle.forecast outputs and s.omega; an IBIS sampler is refused with a pointer to ahead=1"""
    import sequential_monte_carlo_amd as smc
    y = NF.sampler_series()
    tmap = smc.ThetaMap(LG1D, [0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    prior = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(), smc.LogNormal()])
    s = smc.SMC(NF.SAMPLER_N, NF.SAMPLER_M, NF.sampler_model, prior, 2, 0.5, seed=7, theta_map=tmap)
    with pytest.raises(ValueError):
        smc.forecast_state(s, 3)
    smc.smc2(s, y)
    import io
    smc.smc2_run(s, y, 2, NF.SAMPLER_T, window=4, verbose=False, out=io.StringIO())
    H, ps, seed = 4, [0.25, 0.5, 0.75], 4242
    before = snapshot(s._main)
    f = smc.forecast_state(s, H, quantiles=ps, seed=seed)
    assert same_snapshot(before, snapshot(s._main))
    r = s._main.forecast(H, seed, p=ps)
    om = np.asarray(s.omega)
    assert abs(om.sum() - 1) < 1e-12
    mean = (om * r["mean"][:, 0]).sum(axis=1)
    var = (om * r["var"][:, 0]).sum(axis=1) + (om * (r["mean"][:, 0] - mean[:, None]) ** 2).sum(axis=1)
    omean = (om * r["obs_mean"]).sum(axis=1)
    ovar = (om * r["obs_var"]).sum(axis=1) + (om * (r["obs_mean"] - omean[:, None]) ** 2).sum(axis=1)
    q = (om[None, :, None] * r["q"]).sum(axis=1)
    oq = (om[None, :, None] * r["obs_q"]).sum(axis=1)
    for key, ref in (("mean", mean), ("var", var), ("obs_mean", omean), ("obs_var", ovar), ("quantiles", q), ("obs_quantiles", oq)):
        assert f[key].shape == ref.shape, key
        assert np.allclose(f[key], ref, rtol=1e-12, atol=1e-13), key
    assert np.all(f["var"] > 0) and np.all(f["obs_var"] > f["var"] * 0)
    assert "quantiles" not in smc.forecast_state(s, 2)
    s.backend.close()


def test_forecast_state_refuses_ibis(L):
    import sequential_monte_carlo_amd as smc
    prior = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(), smc.LogNormal()])
    tmap = smc.ThetaMap(LG1D, [0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    ib = smc.IBIS(16, lambda th: smc.UnivariateLinearGaussian(A=th[0], B=1.0, Q=th[1], R=th[2]), prior, 2, 0.5, seed=3, theta_map=tmap)
    with pytest.raises(TypeError, match="ahead=1"):
        smc.forecast_state(ib, 3)


# ---- 7. argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_next_forecast_unchanged(L):
    lib = L.lib()
    EINVAL, ESTATE = -1, -3
    fresh = L.Handle(LG1D, 3, 301, seg=256, seed=3)
    fresh.set_params(RAWS[LG1D])
    out = np.zeros(5 * 3 * 8)
    p = np.asarray(PS)
    assert lib.smc_forecast(fresh._h, 5, FSEED, 0, None, 0, L._d(out), None, None, None, None, None) == ESTATE
    assert lib.smc_forecast_cloud(fresh._h, 5, FSEED, None, None) == ESTATE
    fresh.close()
    h = filtered(L, UCSV3D, 256, 301)
    ref = h.forecast(5, FSEED, p=PS, component=1)
    ref_cloud = h.forecast_cloud(5, FSEED)
    before = snapshot(h)
    calls = [
        lambda: lib.smc_forecast(h._h, 0, FSEED, 0, None, 0, L._d(out), None, None, None, None, None),            # H < 1
        lambda: lib.smc_forecast(h._h, -3, FSEED, 0, None, 0, L._d(out), None, None, None, None, None),
        lambda: lib.smc_forecast(h._h, 5, FSEED, 0, L._d(p), -1, L._d(out), None, None, None, None, None),        # np outside 0..8
        lambda: lib.smc_forecast(h._h, 5, FSEED, 0, L._d(np.zeros(9)), 9, L._d(out), None, None, None, None, None),
        lambda: lib.smc_forecast(h._h, 5, FSEED, 3, L._d(p), p.size, None, None, L._d(out), None, None, None),    # component outside [0, d)
        lambda: lib.smc_forecast(h._h, 5, FSEED, -1, L._d(p), p.size, None, None, L._d(out), None, None, None),
        lambda: lib.smc_forecast(h._h, 5, FSEED, 0, None, 3, None, None, L._d(out), None, None, None),            # levels missing
        lambda: lib.smc_forecast_cloud(h._h, 0, FSEED, None, None),
        lambda: lib.smc_forecast(None, 5, FSEED, 0, None, 0, L._d(out), None, None, None, None, None),
        lambda: lib.smc_forecast_cloud(None, 5, FSEED, None, None),
    ]
    for i, call in enumerate(calls):
        assert call() == EINVAL, i
        assert lib.smc_last_error()
        got = h.forecast(5, FSEED, p=PS, component=1)
        assert all(same(got[k], ref[k]) for k in ref), i
    got_cloud = h.forecast_cloud(5, FSEED)
    assert same(got_cloud[0], ref_cloud[0]) and same(got_cloud[1], ref_cloud[1])
    assert same_snapshot(before, snapshot(h))
    h.close()


# ---- 8. the exact one-step prediction --------------------------------------------------------------------------------------------------
def test_lg_one_step_prediction_is_kalmans(L):
    """LG1D, horizon 1, n_x = 4096: obs_mean and obs_var over K = 32 independent filter seeds against the exact Kalman one-step
    prediction (x_T, S_T of smc_kalman_log_likelihood, then A x, A^2 S + Q, B, R), each within 5 standard errors of the K values"""
    K, n = 32, 4096
    raw = RAWS[LG1D][1]
    A, B, Q, R = raw[:4]
    y = L.simulate(LG1D, raw, 12, 17)[1]
    xT, ST, _ = L.kalman_log_likelihood(raw, y)[0]
    mean_x, var_x = A * xT, A * A * ST + Q
    exact = {"mean": mean_x, "var": var_x, "obs_mean": B * mean_x, "obs_var": B * B * var_x + R}
    got = {k: [] for k in exact}
    for seed in range(1, K + 1):
        h = L.Handle(LG1D, 1, n, seed=seed)
        h.set_params(raw)
        h.log_likelihood(y)
        f = h.forecast(1, FSEED + seed)
        for k in exact:
            got[k].append(float(np.ravel(f[k])[0]))
        h.close()
    for k, ex in exact.items():
        v = np.asarray(got[k])
        se = v.std(ddof=1) / math.sqrt(K)
        print("%s: mean of K %.6f exact %.6f, %.2f se" % (k, v.mean(), ex, abs(v.mean() - ex) / se))
        assert abs(v.mean() - ex) <= 5.0 * se, (k, v.mean(), ex, se)
