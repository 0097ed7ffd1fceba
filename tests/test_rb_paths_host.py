"""Rao-Blackwellised backward simulation on the host (smc_host_rb_sample_paths; smc_spec.h "Rao-Blackwellised backward
simulation") against references that share neither arithmetic nor the backward recursion with the library
(tests/rb_paths_reference.py).  No GPU.

  * the law: every index of every path against the long-double CDF built FORWARD (Kalman predictive densities of the later
    observations through the path's own later volatilities) and the path's own uniform, rebuilt from the Philox export
  * the trend pass against a long-double Kalman / RTS pass, the local-level limit, and the joint draw's first two moments
  * the summary columns against numpy and, bit for bit, against a Python restatement of the chunked order
  * the same posterior as the 3-row UCSV model smoothed by FFBS
  * every refusal
"""
import numpy as np
import pytest

import paths_reference as PR
import rb_paths_reference as RB
import smoother_reference as R

ROW = [0.2, 0.3, 1.0, -1.0, -0.5]                 # (g_eps, g_eta, x0, lse0, lsn0)
ROW_SHARP = [0.2, 0.3, 1.0, -1.0, -9.0]           # sharp observations: lsn around -9
SEED, STREAM = 0x5EEDC0FFEE12345, 3
MEAN_REL, MEAN_SD, VAR_REL, VAR_LEVEL = 1e-11, 1e-12, 1e-9, 1e-11     # the moment bounds of DESIGN.md section 2 (as 2e uses them)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def series(L, T, raw=ROW):
    return L.simulate(R.UCSV3D, raw, max(T, 2), 1998)[1][:T]


def gather_vol(x, idx):
    """vol [T][2][M] of the clouds x [T][4][n] at idx [T][M]"""
    return np.array([x[t][1:3][:, idx[t]] for t in range(idx.shape[0])])


@pytest.mark.parametrize("M", [1, 65])
@pytest.mark.parametrize("T", [1, 2, 12])
@pytest.mark.parametrize("n", [1, 65, 300])
@pytest.mark.parametrize("raw", [ROW, ROW_SHARP], ids=["plain", "sharp"])
def test_indices_against_forward_longdouble_cdf(L, raw, n, T, M):
    """F_{i-1} - tol <= u / 2^64 < F_i + tol for every path and step with 2f's tol = (n + 1) 2^-40 + 1000 eps, the CDF built
    without any backward recursion.  Measured at tolerance 0 over all the cases below: see DESIGN.md 2h."""
    y = series(L, T, raw)
    x, w = RB.rb_clouds(L, raw, n, T, y)
    r = L.host_rb_sample_paths(raw, x, w, y, M, SEED, STREAM)
    idx, vol = r["idx"], r["vol"]
    assert np.array_equal(bits(vol), bits(gather_vol(x, idx)))
    worst = RB.check_indices(L, raw, x, w, y, idx, vol, SEED, STREAM)
    print("raw %s n %d T %d M %d: largest distance of a u outside its exact interval %.3e" % (raw[4], n, T, M, worst))
    assert np.all(w[np.arange(T)[:, None], idx] > 0)


def planted(x, w, name):
    x, w = x.copy(), w.copy()
    T, _, n = x.shape
    t = (T - 1) // 2
    if name == "nan_on_zero":                     # every second particle of every step: weight 0 and NaN states
        for s in range(T):
            w[s, 1::2] = 0.0
            w[s] /= w[s].sum()
            x[s][:, 1::2] = np.nan
    elif name == "one_alive":
        top = int(np.argmax(w[t]))
        w[t] = 0.0
        w[t, top] = 1.0
    return x, w


@pytest.mark.parametrize("n", [65, 300])
@pytest.mark.parametrize("name", ["nan_on_zero", "one_alive"])
def test_planted_clouds_against_forward_cdf(L, name, n):
    T, M = 6, 65
    y = series(L, T)
    x, w = planted(*RB.rb_clouds(L, ROW, n, T, y), name)
    r = L.host_rb_sample_paths(ROW, x, w, y, M, SEED, STREAM)
    RB.check_indices(L, ROW, x, w, y, r["idx"], r["vol"], SEED, STREAM)
    assert np.all(w[np.arange(T)[:, None], r["idx"]] > 0)             # zero-weight sources are never chosen, whatever their states
    assert np.all(np.isfinite(r["tmean"])) and np.all(np.isfinite(r["tvar"])) and np.all(np.isfinite(r["tdraw"]))
    assert np.all(r["out"][:, 7] == M)
    if name == "one_alive":
        assert np.all(r["idx"][(T - 1) // 2] == int(np.argmax(w[(T - 1) // 2])))


def test_collapsed_filter_has_no_paths(L):
    T = 6
    y = series(L, T)
    x, w = RB.rb_clouds(L, ROW, 65, T, y)
    for t_dead in (0, 2, T - 1):
        w2 = w.copy()
        w2[t_dead] = 0.0
        r = L.host_rb_sample_paths(ROW, x, w2, y, 65, SEED, STREAM)
        assert np.all(r["idx"] == -1)
        for k in ("vol", "tmean", "tvar", "tdraw"):
            assert np.all(np.isnan(r[k])), (t_dead, k)
        assert np.all(np.isnan(r["out"][:, :7])) and np.all(r["out"][:, 7] == 0)


def test_a_path_ends_where_no_source_reaches_it(L):
    """T = 2, two sources whose log-volatilities lie so far from the only target that the squared distance overflows: every
    log-weight is -inf, the path has its last step and reads -1 / NaN before it; its trend is NaN at every step"""
    x = np.array([[[0.0, 0.0], [1e200, 1e200], [0.0, 0.0], [1.0, 1.0]], [[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [1.0, 1.0]]])
    w = np.full((2, 2), 0.5)
    r = L.host_rb_sample_paths(ROW, x, w, [0.5, 0.7], 5, SEED, STREAM)
    assert np.all(r["idx"][1] >= 0) and np.all(r["idx"][0] == -1)
    assert np.all(np.isnan(r["vol"][0])) and np.all(r["vol"][1] == 0.0)
    assert np.all(np.isnan(r["tmean"])) and np.all(np.isnan(r["tdraw"]))
    assert np.all(r["out"][:, 7] == 0)


def test_invariants(L):
    T = 12
    y = series(L, T)
    x, w = RB.rb_clouds(L, ROW, 300, T, y)
    a = L.host_rb_sample_paths(ROW, x, w, y, 300, SEED, STREAM)
    b = L.host_rb_sample_paths(ROW, x, w, y, 65, SEED, STREAM)
    for k in ("idx", "vol", "tmean", "tvar", "tdraw"):                # path p does not depend on M
        assert np.array_equal(a[k][..., :65], b[k]) and not np.any(np.isnan(b[k].astype(float))), k
    assert not np.array_equal(L.host_rb_sample_paths(ROW, x, w, y, 65, SEED + 1, STREAM)["idx"], b["idx"])
    assert not np.array_equal(L.host_rb_sample_paths(ROW, x, w, y, 65, SEED, STREAM + 1)["idx"], b["idx"])
    c = L.host_rb_sample_paths(ROW, x, w, y, 65, SEED, STREAM, draws=False, summary=False)
    assert np.array_equal(c["idx"], b["idx"]) and np.array_equal(bits(c["tmean"]), bits(b["tmean"])) and "tdraw" not in c
    assert len({tuple(a["idx"][:, p]) for p in range(300)}) > 100


def trend_bound(T, scale):
    """A forward step rounds at most 16 times (two sp_exp of 2 u each, the sum, the reciprocal, three products, the fma, the
    minimum picks one of two values), a backward step as often, and every step inherits the relative error of the variance it
    starts from, itself at most 16 u per step behind it: 16 u (1 + 2 + .. + 2 T) <= 32 T (T + 1) u + 16 T u relative to the
    scale of the quantity - the level max(|x0|, max |y|, 1) for a mean (the gains are at most 1: convex combinations do not
    amplify), the value itself for a variance (sums and products of positive terms only)."""
    return (32 * T * (T + 1) + 16 * T) * RB.EPS * scale


@pytest.mark.parametrize("raw", [ROW, ROW_SHARP], ids=["plain", "sharp"])
@pytest.mark.parametrize("T", [1, 2, 12])
def test_trend_pass_against_longdouble_rts(L, raw, T):
    n, M = 65, 65
    y = series(L, T, raw)
    x, w = RB.rb_clouds(L, raw, n, T, y)
    r = L.host_rb_sample_paths(raw, x, w, y, M, SEED, STREAM)
    level = max(abs(raw[2]), float(np.max(np.abs(y))), 1.0)
    worst = 0.0
    for p in range(M):
        mean, var, _, _, _ = RB.trend(raw, y, r["vol"][:, 0, p], r["vol"][:, 1, p])
        em = np.abs((r["tmean"][:, p].astype(RB.LD) - mean).astype(float))
        ev = np.abs((r["tvar"][:, p].astype(RB.LD) - var).astype(float))
        bm, bv = trend_bound(T, level), trend_bound(T, var.astype(float))
        worst = max(worst, float(np.max(em / bm)), float(np.max(ev / bv)))
        assert np.all(em <= bm) and np.all(ev <= bv), (p, em, bm, ev, bv)
        assert np.all(r["tvar"][:, p] > 0)
    print("T %d lsn0 %s: largest error / bound %.4f" % (T, raw[4], worst))


def test_trend_pass_is_the_local_level_smoother_when_the_volatilities_stand_still(L):
    """gamma_eps = gamma_eta = 1e-9: the volatilities move by about 6e-9 sqrt(T), so every path's trend is the exact smoother of
    the local-level model (A = B = 1, Q = e^lse0, R = e^lsn0, x0, sigma0 = e^lse0) within 1e-6 (1 + |value|).  The exact smoother
    is the library's RTS specification on the host (smc_host_ibis_smooth, the twin of what smc.kalman_smoother runs on the
    device; the GPU test repeats this against smc.kalman_smoother itself)."""
    T, n, M = 12, 65, 65
    raw = [1e-9, 1e-9, 1.0, -1.0, -0.5]
    y = series(L, T)
    x, w = RB.rb_clouds(L, raw, n, T, y)
    r = L.host_rb_sample_paths(raw, x, w, y, M, SEED, STREAM)
    row = [1.0, 1.0, np.exp(raw[3]), np.exp(raw[4]), raw[2], np.exp(raw[3])]
    _, xs, Ps = L.host_ibis_smooth([row], [0.0], y, states=True)
    assert np.all(np.abs(r["tmean"] - xs) <= 1e-6 * (1 + np.abs(xs)))
    assert np.all(np.abs(r["tvar"] - Ps) <= 1e-6 * (1 + np.abs(Ps)))
    assert np.all(np.abs(r["out"][:, 0] - xs[:, 0]) <= 1e-6 * (1 + np.abs(xs[:, 0])))


def test_trend_draws_have_the_rts_moments(L):
    """tdraw given the volatility path is Gaussian with the per-path RTS mean and lag-one covariance G_t Ps_{t+1}: over M = 4096
    paths the standardised residuals (tdraw - tmean) / sd have mean 0 and the products of consecutive residuals have the mean
    the per-path lag-one correlations give, within 4.5 standard errors; the normals are those of slot 37"""
    T, n, M = 12, 65, 4096
    y = series(L, T)
    x, w = RB.rb_clouds(L, ROW, n, T, y)
    r = L.host_rb_sample_paths(ROW, x, w, y, M, SEED, STREAM)
    res = (r["tdraw"] - r["tmean"]) / np.sqrt(r["tvar"])
    zm = np.abs(res.mean(axis=1)) * np.sqrt(M)
    zv = np.abs((res * res).mean(axis=1) - 1.0) * np.sqrt(M / 2.0)
    rho = np.zeros((T - 1, M))
    for p in range(M):
        _, var, _, Pf, Pm = RB.trend(ROW, y, r["vol"][:, 0, p], r["vol"][:, 1, p])
        G = (Pf[:-1] / Pm[1:]).astype(float)
        rho[:, p] = G * np.sqrt(r["tvar"][1:, p] / r["tvar"][:-1, p])
    prod = res[:-1] * res[1:] - rho
    zc = np.abs(prod.mean(axis=1)) / (prod.std(axis=1, ddof=1) / np.sqrt(M))
    print("max z: mean %.2f, variance %.2f, lag-one %.2f" % (zm.max(), zv.max(), zc.max()))
    assert np.all(zm <= 4.5) and np.all(zv <= 4.5) and np.all(zc <= 4.5)
    assert np.mean(np.abs(rho)) > 0.1
    # the last step's draw, from the Philox export: m + sqrt(P) z
    for p in (0, 1, 64, 4095):
        z = RB.trend_normal(L, SEED, p, STREAM, T - 1)
        assert abs(r["tdraw"][T - 1, p] - (r["tmean"][T - 1, p] + np.sqrt(r["tvar"][T - 1, p]) * z)) <= 1e-12 * (1 + abs(r["tdraw"][T - 1, p]))


@pytest.mark.parametrize("M", [1, 65, 300])
def test_summary_columns(L, M):
    """the eight columns against exactly rounded numpy moments within the bounds of DESIGN.md section 2, and bit for bit against
    the chunked order restated in Python; with incomplete paths left out"""
    T, n = 6, 65
    y = series(L, T)
    x, w = RB.rb_clouds(L, ROW, n, T, y)
    r = L.host_rb_sample_paths(ROW, x, w, y, M, SEED, STREAM)
    for t in range(T):
        ref = RB.summary(r["idx"][0], r["tmean"][t], r["tvar"][t], r["vol"][t, 0], r["vol"][t, 1])
        assert np.array_equal(bits(r["out"][t]), bits(ref)), (t, r["out"][t], ref)
        uni = np.full(M, 1.0 / M)
        for v, cm, cv in ((r["tmean"][t], 0, 2), (r["vol"][t, 0], 3, 4), (r["vol"][t, 1], 5, 6)):
            m, var = R.exact_moments(v, uni)
            assert abs(r["out"][t, cm] - m) <= MEAN_REL * abs(m) + MEAN_SD * np.sqrt(var)
            assert r["out"][t, cv] >= 0 and abs(r["out"][t, cv] - var) <= VAR_REL * var + (VAR_LEVEL * m) ** 2
        m, _ = R.exact_moments(r["tvar"][t], uni)
        assert abs(r["out"][t, 1] - m) <= MEAN_REL * abs(m)
        assert r["out"][t, 7] == M


def test_summary_leaves_incomplete_paths_out(L):
    """T = 2: half the particles of the last step carry lse = 1e200, which no source of step 0 reaches (the squared distance
    overflows).  The paths that chose one of them end there: -1 / NaN at step 0, NaN trend at every step, and they are left out
    of the summary, whose count is the number of complete paths; bit for bit the Python restatement"""
    n, M = 4, 65
    x = np.zeros((2, 4, n))
    x[:, 3] = 1.0
    x[1, 1, 2:] = 1e200
    w = np.full((2, n), 0.25)
    y = [0.5, 0.7]
    r = L.host_rb_sample_paths(ROW, x, w, y, M, SEED, STREAM)
    ended = r["idx"][1] >= 2
    assert 0 < ended.sum() < M
    assert np.all(r["idx"][0][ended] == -1) and np.all(r["idx"][0][~ended] >= 0)
    assert np.all(np.isnan(r["vol"][0][:, ended])) and np.all(r["vol"][1][0, ended] == 1e200)
    for k in ("tmean", "tvar", "tdraw"):
        assert np.all(np.isnan(r[k][:, ended])) and np.all(np.isfinite(r[k][:, ~ended])), k
    for t in range(2):
        ref = RB.summary(r["idx"][0], r["tmean"][t], r["tvar"][t], r["vol"][t, 0], r["vol"][t, 1])
        assert np.array_equal(bits(r["out"][t]), bits(ref)) and r["out"][t, 7] == (~ended).sum()
        assert np.all(np.isfinite(r["out"][t])) and abs(r["out"][t, 0] - r["tmean"][t, ~ended].mean()) <= 1e-12


def test_same_posterior_as_the_three_row_model(L, ob):
    """K = 32 independent filters of n = 256, T = 12, M = 256: the smoothed means of trend, lse and lsn from Rao-Blackwellised
    backward simulation over marginal-filter clouds against the FFBS smoothed means (smc_host_smooth) of bootstrap UCSV3D clouds
    on the same series: |difference of the averages over filters| <= 4.5 combined standard errors at every t"""
    K, n, T, M = 32, 256, 12, 256
    y = series(L, T)
    a, b = np.zeros((K, T, 3)), np.zeros((K, T, 3))
    for k in range(K):
        x, w = RB.rb_clouds(L, ROW, n, T, y, seed=300 + k)
        o = L.host_rb_sample_paths(ROW, x, w, y, M, 9000 + k, 0, draws=False)["out"]
        assert np.all(o[:, 7] == M)
        a[k] = o[:, [0, 3, 5]]
        x3, w3 = PR.recorded_clouds(L, ob, R.UCSV3D, ROW, n, T, seed=300 + k)
        _, mean, _ = L.host_smooth(R.UCSV3D, ROW, x3, w3)
        b[k] = mean
    se = np.sqrt(a.var(axis=0, ddof=1) / K + b.var(axis=0, ddof=1) / K)
    z = np.abs(a.mean(axis=0) - b.mean(axis=0)) / se
    print("max z per coordinate (trend, lse, lsn): %s" % np.round(z.max(axis=0), 2))
    assert np.all(z <= 4.5), z


def test_refusals(L):
    lib = L.lib()
    T, n, M = 2, 3, 4
    x, w, y = np.zeros((T, 4, n)), np.full((T, n), 1.0 / 3), np.array([0.1, 0.2])
    with pytest.raises(L.SmcError):
        L.host_rb_sample_paths(ROW, x, w, [0.1, np.nan], M, 1)
    with pytest.raises(L.SmcError):
        L.host_rb_sample_paths(ROW, x, w, [np.inf, 0.2], M, 1)
    for k in (0, 1):
        for bad in (0.0, -1.0, np.nan, np.inf):
            raw = list(ROW)
            raw[k] = bad
            with pytest.raises(L.SmcError):
                L.host_rb_sample_paths(raw, x, w, y, M, 1)
    for Mbad in (0, -3, (1 << 30) + 1):
        idx = np.zeros(1, dtype=np.int32)
        one = np.zeros(64)
        assert lib.smc_host_rb_sample_paths(L._d(np.array(ROW)), T, n, L._d(x), L._d(w), L._d(y), Mbad, 1, 0, idx.ctypes.data_as(L._i32p),
                                            L._d(one), L._d(one), L._d(one), None, None) == -1
    idx = np.zeros(T * M, dtype=np.int32)
    ip = idx.ctypes.data_as(L._i32p)
    vol, tm, tv = np.zeros(T * 2 * M), np.zeros(T * M), np.zeros(T * M)
    args = dict(raw=L._d(np.array(ROW)), x=L._d(x), w=L._d(w), y=L._d(y))

    def call(raw=args["raw"], T_=T, n_=n, x_=args["x"], w_=args["w"], y_=args["y"], M_=M, idx_=ip, vol_=L._d(vol), tm_=L._d(tm), tv_=L._d(tv)):
        return lib.smc_host_rb_sample_paths(raw, T_, n_, x_, w_, y_, M_, 1, 0, idx_, vol_, tm_, tv_, None, None)
    assert call() == 0
    assert call(n_=(1 << 20) + 1) == -1                                # n > 2^20, before any read
    assert call(T_=0) == -1 and call(n_=0) == -1
    assert call(raw=None) == -1 and call(x_=None) == -1 and call(w_=None) == -1 and call(y_=None) == -1
    assert call(idx_=None) == -1 and call(vol_=None) == -1 and call(tm_=None) == -1 and call(tv_=None) == -1
    # the entry points that refuse the family keep refusing it
    with pytest.raises(L.SmcError):
        L.host_sample_paths(L.MODEL_UCSV_RB, ROW, x, w, M, 1)
    with pytest.raises(L.SmcError):
        L.host_transition_logpdf(L.MODEL_UCSV_RB, ROW, np.zeros(4), np.zeros(4))
    assert lib.smc_last_error()
