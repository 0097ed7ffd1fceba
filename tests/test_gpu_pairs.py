"""The lag-one pair moments on the GPU (pytest -m gpu): smc_smooth_pairs over the record of a step-by-step run.

  * device == host twin (smc_host_smooth_pairs), bit for bit: cross, resid2, ws, mean, var, on every launch route - one particle,
    a partial chunk, the 64- and the 256-owner tile, more than SMOOTH_MAX_DIRECT chunks - and on guided, systematic, gapped,
    conditional, collapsed and planted records (the twin is pinned to a long-double recursion by tests/test_pairs_host.py)
  * a filter alone == the same filter in a batch; a repeated call; a call after one more step
  * smc_smooth and smc_sample_paths on the same handle return their own bits before and after
  * particle EM against the exact Kalman-EM step; the UCSV M-step against the same statistic from backward-simulated paths
  * the refusals
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pairs_reference as PR
import smoother_planted as P
import test_gpu_smoother as G

pytestmark = pytest.mark.gpu

LG, LG_SHARP, SV, UC = G.LG, G.LG_SHARP, G.SV, G.UC
RAW = G.RAW
same, rows_for, run_recorded, clouds = G.same, G.rows_for, G.run_recorded, G.clouds


def same_all(a, b):
    return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))


def pick(out, m):
    """filter m of (ws, mean, var, cross, resid2) in the host twin's layouts"""
    ws, mean, var, cross, resid2 = out
    return ws[:, m], mean[:, :, m], var[:, :, m], cross[:, :, :, m], resid2[:, :, m]


def check_against_twin(L, model, rows, x, w, out, filters):
    rows = np.atleast_2d(rows)
    with ThreadPoolExecutor(max_workers=8) as pool:
        twins = list(pool.map(lambda m: L.host_smooth_pairs(model, rows[m], x[:, :, m, :], w[:, m, :]), filters))
    for m, tw in zip(filters, twins):
        for name, dev, host in zip(("ws", "mean", "var", "cross", "resid2"), pick(out, m), tw):
            assert same(dev, host), (name, m)


def check_handle(L, h, model, rows, filters=None):
    """smc_smooth_pairs of the handle == the twin on its record; its ws, mean, var == smc_smooth's; -> its output"""
    x, w = clouds(h)
    out = h.smooth(pairs=True)
    T, d, nth = x.shape[0], x.shape[1], x.shape[2]
    assert out[3].shape == (T - 1, d, d, nth) and out[4].shape == (T - 1, d, nth)
    check_against_twin(L, model, rows, x, w, out, range(nth) if filters is None else filters)
    assert same_all(out[:3], h.smooth())
    return out


# (n, T, n_theta): one particle; a partial chunk in tiles of one wave; three chunks over twelve steps; nine chunks (more than
# SMOOTH_MAX_DIRECT: the k_smooth_rowmax route); 1024 workgroups of 256 owners (the long tile)
SHAPES = [(1, 2, 1), (65, 3, 3), (300, 12, 3), (1100, 3, 1), (1024, 3, 8)]


@pytest.mark.parametrize("n,T,nth", SHAPES)
@pytest.mark.parametrize("model", [1, 2, 3])
def test_pairs_equal_host_twin(L, model, n, T, nth):
    rows = rows_for(RAW[model], nth)
    h = run_recorded(L, model, rows, n, 256 if n in (300, 1100) else 0, T, streams=np.arange(nth))
    out = check_handle(L, h, model, rows)
    assert all(np.all(np.isfinite(a)) for a in out) and np.all(out[4] >= 0)
    h.close()


def test_position_repeat_and_one_more_step(L):
    rows = rows_for(UC, 3)
    hb = run_recorded(L, 3, rows, 300, 256, 6, streams=[0, 1, 2])
    out = hb.smooth(pairs=True)
    assert same_all(out, hb.smooth(pairs=True))                   # the same handle again
    for m in range(3):
        h1 = run_recorded(L, 3, rows[m], 300, 256, 6, streams=[m])
        assert same_all(pick(h1.smooth(pairs=True), 0), pick(out, m)), m
        h1.close()
    hb.close()
    # five steps of a longer record, then one more: each time the twin on the record so far; cross and resid2 alone (ws, mean, var NULL)
    _, y = L.simulate(1, LG, 7, 1998)
    h = L.Handle(1, 2, 300, seg=256, seed=11)
    r2 = rows_for(LG, 2)
    h.set_params(r2)
    h.history_begin(7)
    h.init(float(y[0]))
    for t in range(1, 5):
        h.step(float(y[t]))
    first = check_handle(L, h, 1, r2)
    h.step(float(y[5]))
    second = check_handle(L, h, 1, r2)
    assert second[3].shape[0] == first[3].shape[0] + 1 and not same(second[3][:4], first[3])
    cross, resid2 = np.zeros_like(second[3]), np.zeros_like(second[4])
    assert L.lib().smc_smooth_pairs(h._h, None, None, None, L._d(cross), None) == 0 and same(cross, second[3])
    assert L.lib().smc_smooth_pairs(h._h, None, None, None, None, L._d(resid2)) == 0 and same(resid2, second[4])
    h.close()
    # T = 1: nothing to pair, and nothing is written
    h = run_recorded(L, 1, r2, 300, 256, 1)
    out = h.smooth(pairs=True)
    assert out[3].shape == (0, 1, 1, 2) and out[4].shape == (0, 1, 2) and same_all(out[:3], h.smooth())
    h.close()


def plant(xt, wt, px, pw):
    """one recorded step with filter 1 replaced by (px [d][n], pw [n])"""
    xt, wt = xt.copy(), wt.copy()
    xt[:, 1, :], wt[1] = px, pw
    return xt, wt


def test_collapsed_and_planted_records(L):
    """filter 1 of a batch of three through smc_history_put: dead at the first, a middle and the last step (NaN everywhere for it,
    the neighbours' bits unchanged), then every planted cloud of tests/smoother_planted.py against the twin"""
    for model, raw, names in ((1, LG_SHARP, P.ON_ZERO + P.ALIVE), (2, SV, P.ALIVE), (3, UC, P.ALIVE)):
        T, nth = 6, 3
        rows = rows_for(raw, nth)
        h = run_recorded(L, model, rows, 300, 256, T, streams=np.arange(nth))
        x, w = clouds(h)
        base = check_handle(L, h, model, rows)

        def put(px, pw):
            for t in range(T):
                h.history_put(t, *plant(x[t], w[t], px[t], pw[t]))

        if model == 1:
            for t_dead in P.dead_steps(T):
                put(*P.dead_at(x[:, :, 1, :], w[:, 1, :], t_dead))
                out = h.smooth(pairs=True)
                assert all(np.all(np.isnan(a)) for a in pick(out, 1)), t_dead
                assert all(same_all(pick(out, m), pick(base, m)) for m in (0, 2)), t_dead
        for name in names:
            px, pw = P.variant(name, model, rows[1], x[:, :, 1, :], w[:, 1, :])
            put(px, pw)
            out = h.smooth(pairs=True)
            x2, w2 = x.copy(), w.copy()
            x2[:, :, 1, :], w2[:, 1, :] = px, pw
            check_against_twin(L, model, rows, x2, w2, out, [1])
            assert all(same_all(pick(out, m), pick(base, m)) for m in (0, 2)), name
            assert all(np.all(np.isfinite(a)) for a in pick(out, 1)), name
            if name in P.ON_ZERO:                                     # a state that is not finite on a particle of weight 0 changes nothing
                assert same_all(out, base), name
        put(x[:, :, 1, :], w[:, 1, :])
        assert same_all(h.smooth(pairs=True), base)
        h.close()


def test_guided_systematic_gapped_and_conditional_records(L):
    n, T, nth = 300, 6, 3
    for model, raw, proposal, flags in ((1, LG, G.OPTIMAL, 0), (3, UC, G.OPTIMAL, 0), (1, LG, G.NONE, G.SYSTEMATIC), (2, SV, G.NONE, G.SYSTEMATIC)):
        rows = rows_for(raw, nth)
        h = run_recorded(L, model, rows, n, 256, T, proposal, flags)
        check_handle(L, h, model, rows)
        h.close()
    # a record with a gap (two in a row, and the first period)
    for model, raw in ((1, LG), (3, UC)):
        rows = rows_for(raw, nth)
        _, y = L.simulate(model, raw, T, 1998)
        y[[0, 3, 4]] = np.nan
        h = L.Handle(model, nth, n, seg=256, seed=11, flags=L.FLAG_NAN_MISSING)
        h.set_params(rows)
        h.history_begin(T)
        for t in range(T):
            h.init(float(y[0])) if t == 0 else h.step(float(y[t]))
        check_handle(L, h, model, rows)
        h.close()
    # a conditional record: one slot of every step pinned to a reference path
    for model, raw in ((1, LG), (3, UC)):
        rows = rows_for(raw, nth)
        xs, y = L.simulate(model, raw, T, 1998)
        xref = np.ascontiguousarray(np.repeat(np.asarray(xs).reshape(-1, T).T[:, :, None], nth, axis=2))      # [T][d][n_theta]
        h = L.Handle(model, nth, n, seg=256, seed=11, flags=L.FLAG_CONDITIONAL)
        h.set_params(rows)
        h.set_reference(xref)
        h.history_begin(T)
        for t in range(T):
            h.init(float(y[0])) if t == 0 else h.step(float(y[t]))
        check_handle(L, h, model, rows)
        h.close()


def test_nothing_else_moves(L):
    """smc_smooth and smc_sample_paths on the same handle: their own bits before smc_smooth_pairs and after it"""
    rows = rows_for(UC, 3)
    h = run_recorded(L, 3, rows, 300, 256, 6)
    s0, p0 = h.smooth(), h.sample_paths(32, 17)
    out = h.smooth(pairs=True)
    s1, p1 = h.smooth(), h.sample_paths(32, 17)
    assert same_all(s0, s1) and same_all(out[:3], s0)
    assert np.array_equal(p0[0], p1[0]) and same(p0[1], p1[1])
    assert same_all(h.smooth(pairs=True), out)
    h.close()
    fresh = run_recorded(L, 3, rows, 300, 256, 6)                   # a handle that never asked for pairs
    assert same_all(fresh.smooth(), s0)
    fresh.close()


def test_smoother_python_pairs_and_refusals(L):
    import sequential_monte_carlo_amd as smc
    T, N = 6, 300
    m1 = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
    _, y = smc.simulate(m1, T, seed=1998)
    _, _, _, s = smc.smoother(N, y, m1, seed=5, pairs=True)
    _, _, _, s0 = smc.smoother(N, y, m1, seed=5)
    assert s["cross"].shape == (T - 1,) and s["resid2"].shape == (T - 1,) and s["lag1_cov"].shape == (T - 1,)
    assert same(s["mean"], s0["mean"]) and same(s["var"], s0["var"]) and "cross" not in s0
    assert same(s["lag1_cov"], s["cross"] - s["mean"][:-1] * s["mean"][1:])
    # |corr| <= 1, and Q's update with A held is the mean of resid2 (the centre is A x under the parameters of the run)
    assert np.all(np.abs(s["lag1_cov"]) <= np.sqrt(s["var"][:-1] * s["var"][1:]))
    assert abs(smc.em_mstep(m1, y, s, free=["Q"]).Q - s["resid2"].mean()) <= 1e-9
    ms = [smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=q, R=0.8) for q in (0.7, 0.9, 1.1)]
    _, _, _, sb = smc.smoother(N, y, ms, seed=5, pairs=True)
    assert sb["cross"].shape == (T - 1, 3) and sb["resid2"].shape == (T - 1, 3) and sb["lag1_cov"].shape == (T - 1, 3)
    uc = smc.UCSV((0.2, 0.3), 1.0, (-1.0, -0.5))
    _, _, _, s3 = smc.smoother(N, y, uc, seed=5, pairs=True)
    assert s3["cross"].shape == (T - 1, 3, 3) and s3["resid2"].shape == (T - 1, 3) and s3["lag1_cov"].shape == (T - 1, 3, 3)
    assert same(s3["lag1_cov"], s3["cross"] - s3["mean"][:-1, :, None] * s3["mean"][1:, None, :])
    _, _, _, s3b = smc.smoother(N, y, [uc, uc], seed=5, pairs=True)
    assert s3b["cross"].shape == (T - 1, 2, 3, 3) and s3b["resid2"].shape == (T - 1, 2, 3)
    assert same(s3b["cross"][:, 0], s3["cross"]) and same(s3b["lag1_cov"][:, 0], s3["lag1_cov"])
    _, _, _, s1 = smc.smoother(N, y[:1], m1, seed=5, pairs=True)
    assert s1["cross"].shape == (0,) and s1["lag1_cov"].shape == (0,)
    # refusals
    mu = smc.MarginalUCSV((0.2, 0.3), 1.0, (-1.0, -0.5))
    with pytest.raises(L.SmcError):
        smc.smoother(N, y, mu, seed=5, pairs=True)
    with pytest.raises(TypeError):
        smc.particle_em(N, y, mu, 1, seed=5)
    with pytest.raises(ValueError):
        smc.smoother(N, y, m1, seed=5, pairs=True, smooth=False, paths=4)
    rb = L.Handle(L.MODEL_UCSV_RB, 1, 300, seed=3)
    rb.set_params(np.array([UC]))
    rb.history_begin(2)
    rb.init(0.3)
    z = np.zeros(16)
    assert L.lib().smc_smooth_pairs(rb._h, None, None, None, L._d(z), L._d(z)) == -1
    rb.close()
    h = L.Handle(1, 1, 300, seed=3)
    assert L.lib().smc_smooth_pairs(h._h, None, None, None, L._d(z), L._d(z)) == -3       # nothing recorded
    h.close()


def test_particle_em_against_kalman_em(L):
    """LG1D, README row, N = 512, T = 40, 24 seeds: ONE particle_em iteration against the exact Kalman-EM step, the mean over the
    seeds within 4.5 standard errors for A, Q and R (a numpy rehearsal of the same experiment gave |z| <= 1.3)"""
    import sequential_monte_carlo_amd as smc
    K, N, T = 24, 512, 40
    m0 = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
    _, y = smc.simulate(m0, T, seed=1998)
    want = PR.kalman_em_step(m0.raw(), y)
    th = np.zeros((K, 3))
    for k in range(K):
        r = smc.particle_em(N, y, m0, 1, seed=500 + k)
        assert r["theta"].shape == (2, 3) and r["logZ"].shape == (1,) and len(r["models"]) == 2
        assert np.array_equal(r["theta"][0], [0.5, 0.9, 0.8])
        th[k] = r["theta"][1]
    z = np.abs(th.mean(axis=0) - want) / (th.std(axis=0, ddof=1) / np.sqrt(K))
    print("exact step %s, mean of the particle steps %s, z %s" % (want, th.mean(axis=0), np.round(z, 2)))
    assert np.all(z <= 4.5), z
    # the pieces: iteration 0 is smoother(seed) + em_mstep; a list runs one chain per model, chain 0 on stream 0 as the single model
    _, _, lz, s = smc.smoother(N, y, m0, seed=500, pairs=True)
    m1 = smc.em_mstep(m0, y, s)
    r = smc.particle_em(N, y, m0, 2, seed=500, free=["A", "Q"])
    assert r["theta"].shape == (3, 2) and r["logZ"][0] == lz and r["models"][1].R == 0.8
    assert r["theta"][1, 0] == m1.A and r["theta"][1, 1] == m1.Q
    rb = smc.particle_em(N, y, [m0, smc.UnivariateLinearGaussian(A=0.3, B=1.0, Q=1.2, R=0.8)], 2, seed=500, free=["A", "Q"])
    assert rb["theta"].shape == (3, 2, 2) and rb["logZ"].shape == (2, 2) and len(rb["models"][2]) == 2
    assert np.array_equal(rb["theta"][:, 0], r["theta"]) and np.array_equal(rb["logZ"][:, 0], r["logZ"])


def test_ucsv_mstep_against_backward_simulated_paths(L):
    """UCSV3D, N = 512, T = 40, 24 seeds: the gamma_eps^2 update from the pair moments against the same statistic with sum_t
    resid2[t][lse] replaced by the mean over 512 backward-simulated paths of the same run of sum_t (lse_{t+1} - lse_t)^2: the mean
    difference within 4.5 standard errors"""
    import sequential_monte_carlo_amd as smc
    K, N, T = 24, 512, 40
    uc = smc.UCSV((0.2, 0.3), 1.0, (-1.0, -0.5))
    _, y = smc.simulate(uc, T, seed=1998)
    diff, g2 = np.zeros(K), np.zeros(K)
    for k in range(K):
        _, _, _, s = smc.smoother(N, y, uc, seed=700 + k, pairs=True, paths=512)
        g2[k] = smc.em_mstep(uc, y, s, free=["gamma_eps"]).gamma[0] ** 2
        lse = s["paths"][:, :, 1]                                     # [T][M]
        head = s["var"][0, 1] + (s["mean"][0, 1] - uc.log_sigma0[0]) ** 2
        diff[k] = g2[k] - (head + (np.diff(lse, axis=0) ** 2).sum(axis=0).mean()) / T
    z = abs(diff.mean()) / (diff.std(ddof=1) / np.sqrt(K))
    print("gamma_eps^2: mean update %.5f (from 0.04), mean difference to the paths %.3g, z %.2f" % (g2.mean(), diff.mean(), z))
    assert z <= 4.5, z
