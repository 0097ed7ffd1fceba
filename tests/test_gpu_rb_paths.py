"""Rao-Blackwellised backward simulation on the GPU (pytest -m gpu): smc_rb_sample_paths over the record of a step-by-step run of
the marginal UCSV filter.

  * smc_rb_sample_paths == smc_host_rb_sample_paths on the recorded clouds: the indices as integers; the volatilities, the trend
    moments, the trend draws and the summary bit for bit (the host twin is pinned to a forward long-double CDF, a long-double
    RTS pass and the FFBS posterior of the 3-row model by tests/test_rb_paths_host.py)
  * both selection shapes, the row-maximum launch, counts, planted clouds through smc_history_put, the systematic resampler
  * a filter alone == the same filter inside a batch; repeated calls; one more recorded step
  * every refusal and state rule of include/smc_hip.h, the handle unchanged; the refusals the family had before
  * the Python layer: rb_smoother, rb_smoothed_state
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UC = [0.2, 0.3, 1.0, -1.0, -0.5]
RB, SYSTEMATIC = 4, 4
SEED = 0x5EEDC0FFEE12345
KEYS = ("vol", "tmean", "tvar", "tdraw", "out")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def rows_for(nth):
    r = np.tile(np.asarray(UC, dtype=float), (nth, 1))
    r[:, 0] *= 1.0 + 0.15 * np.arange(nth)
    r[:, 1] *= 1.0 + 0.10 * np.arange(nth)
    return r


def series(L, T):
    return L.simulate(3, UC, max(T, 2), 1998)[1][:T]


def run_recorded(L, rows, n, seg, T, flags=0, seed=11, streams=None, cap=None):
    rows = np.atleast_2d(rows)
    h = L.Handle(RB, rows.shape[0], n, seg=seg, seed=seed, flags=flags)
    h.set_params(rows)
    if streams is not None:
        h.set_streams(streams)
    y = series(L, T)
    h.history_begin(T if cap is None else cap)
    for t in range(T):
        h.init(float(y[0])) if t == 0 else h.step(float(y[t]))
    assert h.history_len() == T
    return h, y


def clouds(h):
    xs, ws = zip(*[h.history_get(t) for t in range(h.history_len())])
    return np.array(xs), np.array(ws)      # [T][4][ntheta][n], [T][ntheta][n]


def take(r, m):
    """filter m of a device result in the host twin's layout"""
    return {"idx": r["idx"][:, m], "vol": r["vol"][:, :, m], "tmean": r["tmean"][:, m], "tvar": r["tvar"][:, m], "tdraw": r["tdraw"][:, m],
            "out": r["out"][:, m]}


def compare_with_host(L, h, rows, y, M, seed=SEED, filters=None, streams=None):
    x, w = clouds(h)
    r = h.rb_sample_paths(y, M, seed, draws=True)
    rows = np.atleast_2d(rows)
    T, nth = x.shape[0], rows.shape[0]
    assert r["idx"].shape == (T, nth, M) and r["vol"].shape == (T, 2, nth, M) and r["out"].shape == (T, nth, 8)
    for m in (range(nth) if filters is None else filters):
        ref = L.host_rb_sample_paths(rows[m], x[:, :, m, :], w[:, m, :], y, M, seed, m if streams is None else streams[m])
        got = take(r, m)
        assert np.array_equal(got["idx"], ref["idx"]), ("indices", m)
        for k in KEYS:
            assert same(got[k], ref[k]), (k, m)
    return x, w, r


# (flags, n, seg, n_theta, T, M): one particle, a partial chunk (65), two segments with padding (300 / 256), 9 chunks (more than
# SMOOTH_MAX_DIRECT: the row-maximum launch) with a partial one (1100 / 256), whole tiles (1024); M = 1, either side of a wave
# (63, 65), a partial tile (300)
CASES = [
    (0, 1, 0, 3, 12, 65),
    (0, 65, 0, 3, 12, 63),
    (0, 65, 0, 3, 12, 300),
    (0, 300, 256, 3, 12, 300),
    (0, 1100, 256, 3, 12, 65),
    (0, 1100, 256, 1, 2, 300),
    (0, 1024, 0, 3, 2, 1),
    (0, 300, 256, 1, 1, 65),
    (0, 300, 256, 3, 1, 300),
    (0, 65, 0, 1, 1, 1),
    (0, 300, 256, 1, 2, 63),
    (SYSTEMATIC, 300, 256, 3, 12, 65),
]


@pytest.mark.parametrize("flags,n,seg,nth,T,M", CASES)
def test_paths_equal_host_twin(L, flags, n, seg, nth, T, M):
    rows = rows_for(nth)
    h, y = run_recorded(L, rows, n, seg, T, flags)
    x, w, r = compare_with_host(L, h, rows, y, M)
    assert np.all(r["idx"] >= 0) and all(np.all(np.isfinite(r[k])) for k in KEYS) and np.all(r["out"][..., 7] == M)
    for m in range(nth):                                              # vol is the gather of the record, zero weights never chosen
        for t in range(T):
            assert same(r["vol"][t, :, m], x[t, 1:3, m][:, r["idx"][t, m]]) and np.all(w[t, m][r["idx"][t, m]] > 0)
    h.close()


def test_many_paths_equal_host_twin(L):
    """n_theta M = 32 x 8192 = 262144 paths: the selection takes one thread per path instead of one wave (PATH_WAVE_SELECT); the
    same results - three filters against the host twin, all against a call just below the threshold, which takes the wave shape"""
    rows = rows_for(32)
    h, y = run_recorded(L, rows, 64, 0, 3)
    _, _, r = compare_with_host(L, h, rows, y, 8192, filters=(0, 13, 31))
    r2 = h.rb_sample_paths(y, 8191, SEED, draws=True)
    assert np.array_equal(r2["idx"], r["idx"][..., :8191])
    for k in ("vol", "tmean", "tvar", "tdraw"):
        assert same(r2[k], r[k][..., :8191]), k
    h.close()


def test_counts(L):
    """a batch of 3 distinct rows with counts = [M, 0, 7]: the slots below a count are those of the uniform call, the slots above
    read -1 / NaN, and the summary is that of the host twin with M = the count"""
    M, T = 65, 6
    rows = rows_for(3)
    h, y = run_recorded(L, rows, 300, 256, T)
    x, w, full = compare_with_host(L, h, rows, y, M)
    counts = np.array([M, 0, 7], dtype=np.int32)
    r = h.rb_sample_paths(y, M, SEED, counts=counts, draws=True)
    for m, c in enumerate(counts):
        assert np.array_equal(r["idx"][:, m, :c], full["idx"][:, m, :c]) and np.all(r["idx"][:, m, c:] == -1)
        for k in ("vol", "tmean", "tvar", "tdraw"):
            assert same(r[k][..., m, :c], full[k][..., m, :c]) and np.all(np.isnan(r[k][..., m, c:])), (k, m)
        if c:
            ref = L.host_rb_sample_paths(rows[m], x[:, :, m, :], w[:, m, :], y, int(c), SEED, m)
            assert same(r["out"][:, m], ref["out"]), m
        else:
            assert np.all(np.isnan(r["out"][:, m, :7])) and np.all(r["out"][:, m, 7] == 0)
    h.close()


@pytest.mark.parametrize("name", ["nan_on_zero", "one_alive", "collapsed"])
def test_planted_clouds_equal_host_twin(L, name):
    """clouds no filter leaves, put into the record of filter 1 of a batch of two: device == host, filter 0 as before"""
    T, n, M = 6, 300, 65
    rows = rows_for(2)
    h, y = run_recorded(L, rows, n, 256, T)
    before = h.rb_sample_paths(y, M, SEED, draws=True)
    x, w = clouds(h)
    tm = (T - 1) // 2
    for t in range(T):
        xt, wt = x[t].copy(), w[t].copy()
        if name == "nan_on_zero":
            wt[1, 1::2] = 0.0
            wt[1] /= wt[1].sum()
            xt[:, 1, 1::2] = np.nan
        elif name == "one_alive" and t == tm:
            top = int(np.argmax(wt[1]))
            wt[1] = 0.0
            wt[1, top] = 1.0
        elif name == "collapsed" and t == tm:
            wt[1] = 0.0
        h.history_put(t, xt, wt)
    _, w2, r = compare_with_host(L, h, rows, y, M)
    assert np.array_equal(r["idx"][:, 0], before["idx"][:, 0]) and all(same(r[k][..., 0, :], before[k][..., 0, :]) for k in KEYS)
    if name == "collapsed":
        assert np.all(r["idx"][:, 1] == -1) and all(np.all(np.isnan(r[k][..., 1, :])) for k in ("vol", "tmean", "tvar", "tdraw"))
        assert np.all(np.isnan(r["out"][:, 1, :7])) and np.all(r["out"][:, 1, 7] == 0)
    else:
        assert np.all(r["idx"] >= 0) and np.all(np.isfinite(r["tmean"]))
        for t in range(T):
            assert np.all(w2[t, 1][r["idx"][t, 1]] > 0)
    if name == "one_alive":
        assert np.all(r["idx"][tm, 1] == int(np.argmax(w2[tm, 1])))
    h.close()


def test_incomplete_paths_equal_host_twin(L):
    """every second particle of the last step of filter 1 carries lse = 1e200, which no source reaches: the paths through them
    end there (-1 / NaN before, NaN trend), the others are complete, and the summary leaves the former out: device == host"""
    M = 300
    rows = rows_for(2)
    h, y = run_recorded(L, rows, 65, 0, 3)
    x, _ = h.history_get(2)
    x[1, 1, 1::2] = 1e200
    h.history_put(2, x, None)
    _, _, r = compare_with_host(L, h, rows, y, M)
    ended = r["idx"][2, 1] % 2 == 1
    assert 0 < ended.sum() < M and np.all(r["idx"][:2, 1][:, ended] == -1) and np.all(r["idx"][:, 1][:, ~ended] >= 0)
    assert np.all(np.isnan(r["tmean"][:, 1][:, ended])) and np.all(np.isfinite(r["tmean"][:, 1][:, ~ended]))
    assert np.all(r["out"][:, 1, 7] == (~ended).sum()) and np.all(r["out"][:, 0, 7] == M) and np.all(np.isfinite(r["out"]))
    h.close()


def test_position_independence_repeatability_more_steps(L):
    rows = rows_for(3)
    M, T = 65, 12
    hb, y = run_recorded(L, rows, 300, 256, T, streams=[0, 1, 2], cap=T + 1)
    a = hb.rb_sample_paths(y, M, SEED, draws=True)
    state0 = hb.state()
    b = hb.rb_sample_paths(y, M, SEED, draws=True)                     # the same handle again
    assert np.array_equal(a["idx"], b["idx"]) and all(same(a[k], b[k]) for k in KEYS)
    assert all(np.array_equal(u, v) for u, v in zip(state0, hb.state()))          # nothing on the handle is disturbed
    assert not np.array_equal(hb.rb_sample_paths(y, M, SEED + 1)["idx"], a["idx"])
    for m in range(3):                                                # a filter alone, on its stream
        h1, _ = run_recorded(L, rows[m], 300, 256, T, streams=[m])
        c = h1.rb_sample_paths(y, M, SEED, draws=True)
        assert np.array_equal(c["idx"][:, 0], a["idx"][:, m]) and all(same(c[k][..., 0, :], a[k][..., m, :]) for k in KEYS), m
        h1.close()
    big = hb.rb_sample_paths(y, 300, SEED, draws=True)                # the first paths of a larger M are those of a smaller one
    assert np.array_equal(big["idx"][..., :M], a["idx"]) and all(same(big[k][..., :M], a[k]) for k in ("vol", "tmean", "tvar", "tdraw"))
    # outputs that are not asked for change nothing
    c = hb.rb_sample_paths(y, M, SEED, draws=False, per_path=False)
    assert set(c) == {"out"} and same(c["out"], a["out"])
    # one more recorded step: the paths use the longer series
    y13 = np.append(y, y[-1] + 0.3)
    hb.step(float(y13[-1]))
    _, _, d = compare_with_host(L, hb, rows, y13, M, streams=[0, 1, 2])
    assert d["idx"].shape[0] == T + 1 and not np.array_equal(d["idx"][:T], a["idx"])
    hb.close()


def test_refusals_and_state_rules(L):
    lib = L.lib()
    EINVAL, ESTATE = -1, -3
    ip = L._i32p
    y = series(L, 4)

    def call(h, y_=y[:2], T=2, M=4, counts=None):
        return lib.smc_rb_sample_paths(h._h if h is not None else None, L._d(np.ascontiguousarray(y_)) if y_ is not None else None, T, M, 1,
                                       counts.ctypes.data_as(ip) if counts is not None else None, None, None, None, None, None, None)
    h = L.Handle(RB, 2, 300, seg=256, seed=3)
    h.set_params(rows_for(2))
    assert call(h) == ESTATE                                                     # not armed
    h.history_begin(3)
    assert call(h) == ESTATE                                                     # armed, nothing recorded
    h.init(float(y[0]))
    h.step(float(y[1]))
    good = h.rb_sample_paths(y[:2], 4, 1, draws=True)
    state0 = h.state()
    assert call(h) == 0                                                          # no output asked for: allowed
    assert call(None) == EINVAL
    assert call(h, T=1) == EINVAL and call(h, T=3, y_=y[:3]) == EINVAL           # T is not smc_history_len
    assert call(h, y_=None) == EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        assert call(h, y_=np.array([y[0], bad])) == EINVAL
    for M in (0, -1, (1 << 30) + 1):
        assert call(h, M=M) == EINVAL
    for bad in ([5, 0], [0, -1]):
        assert call(h, counts=np.array(bad, dtype=np.int32)) == EINVAL
    for col in (0, 1):
        for v in (0.0, -1.0, np.nan, np.inf):
            badrows = rows_for(2)
            badrows[1, col] = v
            h.set_params(badrows)
            assert call(h) == EINVAL
    h.set_params(rows_for(2))
    again = h.rb_sample_paths(y[:2], 4, 1, draws=True)                           # the refusals changed nothing
    assert np.array_equal(good["idx"], again["idx"]) and all(same(good[k], again[k]) for k in KEYS)
    assert all(np.array_equal(u, v) for u, v in zip(state0, h.state())) and h.history_len() == 2
    # the entry points that refused the family refuse it as before
    assert lib.smc_sample_paths(h._h, 4, 1, None, None, None) == EINVAL
    assert lib.smc_smooth(h._h, None, None, None) == EINVAL
    h.history_end()
    assert call(h) == ESTATE
    h.close()
    for model, raw in ((1, [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]), (3, UC)):            # a handle of another family
        o = L.Handle(model, 1, 64, seed=3)
        o.set_params(np.array([raw]))
        o.history_begin(2)
        o.init(0.3)
        assert call(o, T=1, y_=y[:1]) == EINVAL
        o.close()
    big = L.Handle(RB, 1, (1 << 20) + 1, seed=3)                                 # n_x > 2^20
    big.set_params(np.array([UC]))
    big.history_begin(1)
    big.init(float(y[0]))
    assert call(big, T=1, y_=y[:1]) == EINVAL and b"2^20" in lib.smc_last_error()
    big.close()


def test_rb_smoother_python_shapes(L):
    import sequential_monte_carlo_amd as smc
    T, N, M = 6, 300, 40
    mu = smc.MarginalUCSV((0.2, 0.3), 1.0, (-1.0, -0.5))
    y = series(L, T)
    x, w, logZ, s = smc.rb_smoother(N, y, mu, paths=M, seed=5, draws=True, per_path=True)
    for k in ("trend_mean", "trend_var", "n_paths", "logmu", "ess"):
        assert s[k].shape == (T,), k
    assert s["vol_mean"].shape == (T, 2) and s["vol_var"].shape == (T, 2) and np.all(s["n_paths"] == M)
    assert s["path_index"].shape == (T, M) and s["path_index"].dtype == np.int32 and s["vol_paths"].shape == (T, M, 2)
    assert s["path_trend_mean"].shape == (T, M) and s["path_trend_var"].shape == (T, M) and s["paths"].shape == (T, M, 3)
    assert same(s["paths"][..., 1:], s["vol_paths"])
    assert np.allclose(s["trend_mean"], s["path_trend_mean"].mean(axis=1), rtol=1e-12, atol=0)
    assert np.allclose(s["trend_var"], s["path_trend_var"].mean(axis=1) + s["path_trend_mean"].var(axis=1), rtol=1e-10, atol=0)
    assert np.allclose(s["vol_mean"], s["vol_paths"].mean(axis=1), rtol=1e-12, atol=0)
    _, _, logZ1 = smc.log_likelihood(N, y, mu, seed=5)[:3]             # the filter is log_likelihood's
    assert abs(logZ - logZ1) <= 1e-9 * abs(logZ1)
    _, _, _, s0 = smc.rb_smoother(N, y, mu, paths=M, seed=5)           # the default path seed is a function of the filter seed
    assert same(s0["trend_mean"], s["trend_mean"]) and "paths" not in s0 and "path_index" not in s0
    _, _, _, s1 = smc.rb_smoother(N, y, mu, paths=M, seed=5, path_seed=123)
    assert not same(s1["trend_mean"], s["trend_mean"])
    ms = [smc.MarginalUCSV((0.2, g), 1.0, (-1.0, -0.5)) for g in (0.25, 0.3, 0.35)]
    _, _, lz, sb = smc.rb_smoother(N, y, ms, paths=M, seed=5, draws=True, per_path=True, path_counts=[M, 0, 7])
    assert lz.shape == (3,) and sb["trend_mean"].shape == (T, 3) and sb["vol_mean"].shape == (T, 3, 2) and sb["logmu"].shape == (T, 3)
    assert sb["paths"].shape == (T, 3, M, 3) and sb["path_index"].shape == (T, 3, M) and sb["vol_paths"].shape == (T, 3, M, 2)
    assert np.all(sb["n_paths"] == np.array([M, 0, 7])) and np.all(np.isnan(sb["trend_mean"][:, 1])) and np.all(sb["path_index"][:, 2, 7:] == -1)
    with pytest.raises(TypeError):
        smc.rb_smoother(N, y, smc.UCSV((0.2, 0.3), 1.0, (-1.0, -0.5)), paths=M)
    with pytest.raises(L.SmcError):                                    # smc.smoother refuses the family as before
        smc.smoother(N, y, mu, seed=5)


def test_local_level_limit_against_kalman_smoother(L):
    """gamma_eps = gamma_eta = 1e-9: the trend of every path is smc.kalman_smoother's of the local-level model within
    1e-6 (1 + |value|)"""
    import sequential_monte_carlo_amd as smc
    T, N, M = 12, 300, 65
    y = series(L, T)
    _, _, _, s = smc.rb_smoother(N, y, smc.MarginalUCSV((1e-9, 1e-9), 1.0, (-1.0, -0.5)), paths=M, seed=5, per_path=True)
    xs, Ps = smc.kalman_smoother(y, smc.LinearModel(1.0, 1.0, np.exp(-1.0), np.exp(-0.5), 1.0, np.exp(-1.0)))
    assert np.all(np.abs(s["path_trend_mean"] - xs[:, None]) <= 1e-6 * (1 + np.abs(xs[:, None])))
    assert np.all(np.abs(s["path_trend_var"] - Ps[:, None]) <= 1e-6 * (1 + np.abs(Ps[:, None])))
    assert np.all(np.abs(s["trend_mean"] - xs) <= 1e-6 * (1 + np.abs(xs))) and np.all(np.abs(s["trend_var"] - Ps) <= 1e-6 * (1 + Ps))


def test_rb_smoothed_state_of_a_sampler(L):
    import sequential_monte_carlo_amd as smc
    Mth, N, T, M = 6, 64, 8, 50
    y = series(L, T)
    prior = smc.product_distribution([smc.LogNormal(), smc.LogNormal()])
    model = lambda th: smc.MarginalUCSV((th[0], th[1]), 1.0, (-1.0, -0.5))   # noqa: E731
    s = smc.SMC(N, Mth, model, prior, 2, 0.5, seed=23)
    smc.smc2(s, y[:1])
    r = smc.rb_smoothed_state(s, y, M, seed=99)
    assert r["trend_mean"].shape == (T,) and r["trend_var"].shape == (T,) and r["vol_mean"].shape == (T, 2) and r["vol_var"].shape == (T, 2)
    assert np.all(r["n_paths"] == M) and all(np.all(np.isfinite(v)) for v in r.values())
    one = smc.rb_smoothed_state(s, y, M, seed=99, max_bytes=1)        # one parameter particle per block: the same bits
    assert all(same(r[k], one[k]) for k in r)
    assert not same(r["trend_mean"], smc.rb_smoothed_state(s, y, M, seed=100)["trend_mean"])
    # by hand: the ancestors of the library's outer resampler, then each drawn parameter particle alone
    anc = L.host_outer_resample(s.logw, M, 99 + 1)
    num, tot, per = np.zeros(T), 0, []
    for m in np.unique(anc):
        c = int((anc == m).sum())
        _, _, _, sm = smc.rb_smoother(N, y, model(s.theta[m]), seed=99, streams=[m], paths=c, path_seed=99 + 2, per_path=True)
        per.append((c, sm))
        num += sm["path_trend_mean"].sum(axis=1)
        tot += c
    assert tot == M
    mean = num / M
    allm = np.concatenate([sm["path_trend_mean"] for _, sm in per], axis=1)
    allv = np.concatenate([sm["path_trend_var"] for _, sm in per], axis=1)
    alll = np.concatenate([sm["vol_paths"] for _, sm in per], axis=1)
    assert np.allclose(r["trend_mean"], mean, rtol=1e-11, atol=0)
    assert np.allclose(r["trend_var"], allv.mean(axis=1) + allm.var(axis=1), rtol=1e-9, atol=0)
    assert np.allclose(r["vol_mean"], alll.mean(axis=1), rtol=1e-11, atol=0) and np.allclose(r["vol_var"], alll.var(axis=1), rtol=1e-8, atol=0)
    s.backend.close()
    su = smc.SMC(N, 4, lambda th: smc.UCSV((th[0], th[1]), 1.0, (-1.0, -0.5)), prior, 2, 0.5, seed=23)
    smc.smc2(su, y[:1])
    with pytest.raises(TypeError):
        smc.rb_smoothed_state(su, y, 9)
    su.backend.close()
