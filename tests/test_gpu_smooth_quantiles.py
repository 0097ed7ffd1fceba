"""Weighted quantiles of the smoothed state on the GPU (pytest -m gpu): smc_smooth_quantiles over the record of a
step-by-step run.

  * device == host twin (smc_host_smooth_quantiles on the x of smc_history_get and the ws the same call returned), bit for bit:
    every density family and state coordinate, a lone lane, ragged waves, the staged and the unstaged path of the kernel, one
    and several filters, steps and levels; guided, systematic, gapped and conditional records; planted clouds (the twin is
    pinned to a restatement in Python integers by tests/test_smooth_quantiles_host.py)
  * ws, mean, var, cross, resid2 are smc_smooth_pairs'; a filter alone == the same filter in a batch; a repeated call;
    smc_smooth and smc_sample_paths return their own bits before and after; a handle that never asks holds no quantile block
  * the refusals, each leaving the handle as it was
  * the Python layer: smoother(quantiles=...), smoothed_quantiles
  * the smoothed median and 5 % point of LG1D against the exact Kalman smoother, self-normalising
"""
import numpy as np
import pytest

import smooth_quantiles_reference as ref
import smoother_planted as P
import test_gpu_smoother as G

pytestmark = pytest.mark.gpu

LG, LG_SHARP, SV, UC = G.LG, G.LG_SHARP, G.SV, G.UC
RAW = G.RAW
same, rows_for, run_recorded, clouds = G.same, G.rows_for, G.run_recorded, G.clouds
LEVELS = ref.LEVELS


def same_all(a, b):
    return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))


def check_handle(L, h, comp, p, pairs=False, x=None):
    """smooth(quantiles=(comp, p)) of the handle == the twin on its record and the ws of the same call -> the call's output"""
    if x is None:
        x, _ = clouds(h)
    out = h.smooth(pairs=pairs, quantiles=(comp, p))
    ws, q = out[0], out[-1]
    T, nth = ws.shape[0], ws.shape[1]
    assert q.shape == (T, nth, len(p))
    for m in range(nth):
        assert same(q[:, m], L.host_smooth_quantiles(x[:, comp, m, :], ws[:, m, :], p)), (comp, m)
    return out


def seg_of(n):
    return 256 if n in (257, 1000) else (1024 if n > 4096 else 0)


def lds_max(L):
    return L.smooth_quantiles_constants()[1]


# (n, n_theta, T, np) per family: a lone lane, ragged waves around 64, more than one round of the workgroup (257, 1000), the
# largest staged cloud and the first unstaged one (n = None, None + 1: SMOOTH_Q_LDS_MAX); 1 and 3 filters with distinct rows,
# 1, 2 and 5 steps, 1, 3 and 8 levels, each value with every family somewhere
SHAPES = {
    1: [(1, 3, 2, 8), (63, 1, 5, 3), (64, 3, 1, 1), (65, 3, 5, 8), (257, 1, 2, 3), (1000, 3, 5, 8), ("max", 1, 2, 3), ("max+1", 3, 2, 8)],
    2: [(1, 1, 1, 3), (63, 3, 2, 8), (64, 1, 5, 3), (65, 1, 2, 1), (257, 3, 5, 8), (1000, 1, 1, 3), ("max", 3, 2, 8), ("max+1", 1, 5, 1)],
    3: [(1, 3, 5, 1), (63, 3, 1, 8), (64, 3, 2, 3), (65, 1, 5, 8), (257, 3, 2, 1), (1000, 3, 2, 3), ("max", 1, 2, 8), ("max+1", 1, 2, 3)],
}


@pytest.mark.parametrize("model,shape", [(m, s) for m in (1, 2, 3) for s in SHAPES[m]])
def test_quantiles_equal_host_twin(L, model, shape):
    n, nth, T, nq = shape
    n = {"max": lds_max(L), "max+1": lds_max(L) + 1}.get(n, n)
    rows = rows_for(RAW[model], nth)
    h = run_recorded(L, model, rows, n, seg_of(n), T, streams=np.arange(nth))
    x, _ = clouds(h)
    for comp in range(h.d):                                    # UCSV3D: the trend and both log-volatilities
        ws, mean, var, q = check_handle(L, h, comp, LEVELS[nq], x=x)
        assert np.all(np.isfinite(q))
        if nq == 8 and n <= 1000:                              # p = 0, 1: the extremes of the particles that carry (integer) weight
            for m in range(nth):
                for t in range(T):
                    live = np.array(ref.integer_weights(ws[t, m])[0]) > 0
                    assert q[t, m, 0] == x[t, comp, m][live].min() and q[t, m, 1] == x[t, comp, m][live].max()
        if nq == 3 and n >= 63:                                # the band brackets nothing absurd: q25 <= q50 <= q75, inside mean +- 10 sd
            assert np.all(np.diff(q, axis=2) >= 0)
            assert np.all(np.abs(q[:, :, 1] - mean[:, comp]) <= 10 * np.sqrt(var[:, comp]) + 1e-300)
    h.close()


def test_guided_systematic_gapped_and_conditional_records(L):
    n, T, nth, p = 300, 5, 3, LEVELS[3]
    for model, raw, proposal, flags in ((1, LG, G.OPTIMAL, 0), (3, UC, G.OPTIMAL, 0), (1, LG, G.NONE, G.SYSTEMATIC), (2, SV, G.NONE, G.SYSTEMATIC)):
        h = run_recorded(L, model, rows_for(raw, nth), n, 256, T, proposal, flags)
        check_handle(L, h, h.d - 1, p)
        h.close()
    for model, raw in ((1, LG), (3, UC)):                       # a record with a gap (two in a row, and the first period)
        _, y = L.simulate(model, raw, T, 1998)
        y[[0, 2, 3]] = np.nan
        h = L.Handle(model, nth, n, seg=256, seed=11, flags=L.FLAG_NAN_MISSING)
        h.set_params(rows_for(raw, nth))
        h.history_begin(T)
        for t in range(T):
            h.init(float(y[0])) if t == 0 else h.step(float(y[t]))
        check_handle(L, h, 0, p)
        h.close()
    for model, raw in ((1, LG), (3, UC)):                       # a conditional record: one slot of every step pinned to a path
        xs, y = L.simulate(model, raw, T, 1998)
        xref = np.ascontiguousarray(np.repeat(np.asarray(xs).reshape(-1, T).T[:, :, None], nth, axis=2))      # [T][d][n_theta]
        h = L.Handle(model, nth, n, seg=256, seed=11, flags=L.FLAG_CONDITIONAL)
        h.set_params(rows_for(raw, nth))
        h.set_reference(xref)
        h.history_begin(T)
        for t in range(T):
            h.init(float(y[0])) if t == 0 else h.step(float(y[t]))
        check_handle(L, h, 0, p)
        h.close()


def plant(xt, wt, px, pw):
    """one recorded step with filter 1 replaced by (px [d][n], pw [n])"""
    xt, wt = xt.copy(), wt.copy()
    xt[:, 1, :], wt[1] = px, pw
    return xt, wt


def test_collapsed_and_planted_records(L):
    """filter 1 of a batch of three through smc_history_put: dead at the first, a middle and the last step (NaN at every level
    of every step for it, the neighbours' bits unchanged), then every planted cloud of tests/smoother_planted.py against the twin
    - states that are not finite on particles of weight 0, ties, subnormal weights, one particle alive"""
    p = LEVELS[8]
    for model, raw, names in ((1, LG_SHARP, P.ON_ZERO + P.ALIVE), (2, SV, P.ALIVE), (3, UC, P.ALIVE)):
        T, nth = 5, 3
        rows = rows_for(raw, nth)
        h = run_recorded(L, model, rows, 300, 256, T, streams=np.arange(nth))
        comp = h.d - 1                                          # (UCSV3D: the row the planted clouds move)
        x, w = clouds(h)
        base = check_handle(L, h, comp, p, x=x)

        def put(px, pw):
            for t in range(T):
                h.history_put(t, *plant(x[t], w[t], px[t], pw[t]))

        if model == 1:
            for t_dead in P.dead_steps(T):
                put(*P.dead_at(x[:, :, 1, :], w[:, 1, :], t_dead))
                out = h.smooth(quantiles=(comp, p))
                assert same(out[-1][:, 1], np.full((T, len(p)), np.nan)), t_dead
                assert same(out[-1][:, [0, 2]], base[-1][:, [0, 2]]), t_dead
        for name in names:
            px, pw = P.variant(name, model, rows[1], x[:, :, 1, :], w[:, 1, :])
            put(px, pw)
            x2 = x.copy()
            x2[:, :, 1, :] = px
            out = check_handle(L, h, comp, p, x=x2)
            assert same(out[-1][:, [0, 2]], base[-1][:, [0, 2]]), name
            assert np.all(np.isfinite(out[-1][:, 1])), name
            if name in P.ON_ZERO:                               # a state that is not finite on a particle of weight 0 changes nothing
                assert same_all(out, base), name
            if name == "one_alive":                             # every level is the state of the one particle that is alive
                t = P.mid(T)
                assert same(out[-1][t, 1], np.repeat(px[t, comp, int(np.argmax(pw[t]))], len(p)))
        put(x[:, :, 1, :], w[:, 1, :])
        assert same_all(h.smooth(quantiles=(comp, p)), base)
        h.close()


def test_superset_position_repeat_and_nothing_else_moves(L):
    rows = rows_for(UC, 3)
    p = LEVELS[3]
    h = run_recorded(L, 3, rows, 300, 256, 5, streams=[0, 1, 2])
    assert h.smooth_quantiles_scratch() == 0
    s0, p0, pr0 = h.smooth(), h.sample_paths(32, 17), h.smooth(pairs=True)
    assert h.smooth_quantiles_scratch() == 0                    # nobody asked for quantiles yet: no block
    out = check_handle(L, h, 1, p, pairs=True)
    assert h.smooth_quantiles_scratch() > 0
    assert same_all(out[:5], pr0) and same_all(out[:3], s0)     # ws, mean, var, cross, resid2 are smc_smooth_pairs', bit for bit
    again = h.smooth(pairs=True, quantiles=(1, p))
    assert same_all(again, out)                                 # the same handle again
    plain = h.smooth(quantiles=(1, p))                          # without the pair moments: the same quantiles, smc_smooth's results
    assert same(plain[-1], out[-1]) and same_all(plain[:3], s0)
    q_only = np.zeros_like(out[-1])                             # every other output NULL
    pp = np.asarray(p)
    assert L.lib().smc_smooth_quantiles(h._h, None, None, None, None, None, 1, L._d(pp), 3, L._d(q_only)) == 0 and same(q_only, out[-1])
    s1, p1, pr1 = h.smooth(), h.sample_paths(32, 17), h.smooth(pairs=True)
    assert same_all(s0, s1) and same_all(pr0, pr1) and np.array_equal(p0[0], p1[0]) and same(p0[1], p1[1])
    for m in range(3):                                          # a filter alone == the same filter in the batch
        h1 = run_recorded(L, 3, rows[m], 300, 256, 5, streams=[m])
        alone = h1.smooth(pairs=True, quantiles=(1, p))
        assert same(alone[-1][:, 0], out[-1][:, m]) and same(alone[0][:, 0], out[0][:, m]), m
        h1.close()
    h.close()
    fresh = run_recorded(L, 3, rows, 300, 256, 5, streams=[0, 1, 2])    # a handle that never asks for quantiles
    assert same_all(fresh.smooth(), s0) and same_all(fresh.smooth(pairs=True), pr0) and fresh.smooth_quantiles_scratch() == 0
    fresh.close()


def test_one_more_step(L):
    _, y = L.simulate(1, LG, 7, 1998)
    h = L.Handle(1, 2, 300, seg=256, seed=11)
    h.set_params(rows_for(LG, 2))
    h.history_begin(7)
    h.init(float(y[0]))
    for t in range(1, 5):
        h.step(float(y[t]))
    first = check_handle(L, h, 0, LEVELS[3])
    h.step(float(y[5]))
    second = check_handle(L, h, 0, LEVELS[3])
    assert second[-1].shape[0] == first[-1].shape[0] + 1
    h.close()


def test_refusals_leave_the_handle_unchanged(L):
    lib = L.lib()
    rows = rows_for(UC, 2)
    h = run_recorded(L, 3, rows, 300, 256, 4)
    before = h.smooth(pairs=True)
    q = np.full((4, 2, 9), 7.0)
    ok, wide, far = np.array([0.25, 0.5, 0.75]), np.full(9, 0.5), np.array([0.5, 1.5])
    for comp, p, np_ in ((0, ok, 0), (0, wide, 9), (3, ok, 3), (-1, ok, 3), (0, far, 2), (0, np.array([-0.1]), 1), (0, np.array([np.nan]), 1)):
        assert lib.smc_smooth_quantiles(h._h, None, None, None, None, None, comp, L._d(p), np_, L._d(q)) == -1, (comp, np_)
    assert lib.smc_smooth_quantiles(h._h, None, None, None, None, None, 0, None, 3, L._d(q)) == -1
    assert lib.smc_smooth_quantiles(h._h, None, None, None, None, None, 0, L._d(ok), 3, None) == -1
    assert np.all(q == 7.0) and h.smooth_quantiles_scratch() == 0 and h.history_len() == 4
    assert same_all(h.smooth(pairs=True), before)
    check_handle(L, h, 2, ok)                                  # ... and a correct call afterwards
    h.close()
    rb = L.Handle(L.MODEL_UCSV_RB, 1, 300, seed=3)
    rb.set_params(np.array([UC]))
    rb.history_begin(2)
    rb.init(0.3)
    assert lib.smc_smooth_quantiles(rb._h, None, None, None, None, None, 0, L._d(ok), 3, L._d(q)) == -1
    assert rb.smooth_quantiles_scratch() == 0 and rb.history_len() == 1
    rb.close()
    h = L.Handle(1, 1, 300, seed=3)
    assert lib.smc_smooth_quantiles(h._h, None, None, None, None, None, 0, L._d(ok), 3, L._d(q)) == -3       # nothing recorded
    h.history_begin(3)
    assert lib.smc_smooth_quantiles(h._h, None, None, None, None, None, 0, L._d(ok), 3, L._d(q)) == -3       # armed, no step yet
    assert h.smooth_quantiles_scratch() == 0 and np.all(q == 7.0)
    h.close()


def test_python_smoother_quantiles(L):
    import sequential_monte_carlo_amd as smc
    T, N, p = 6, 300, [0.25, 0.5, 0.75]
    m1 = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
    _, y = smc.simulate(m1, T, seed=1998)
    _, _, _, s = smc.smoother(N, y, m1, seed=5, quantiles=p, weights=True)
    assert s["quantiles"].shape == (T, 3) and same(s["quantiles"], ref.quantiles(s["x"], s["weights"], p))
    _, _, _, s0 = smc.smoother(N, y, m1, seed=5)
    assert "quantiles" not in s0 and same(s0["mean"], s["mean"]) and same(s0["var"], s["var"])
    _, _, _, sp = smc.smoother(N, y, m1, seed=5, quantiles=p, pairs=True)
    assert same(sp["quantiles"], s["quantiles"]) and sp["cross"].shape == (T - 1,)
    ms = [smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=q, R=0.8) for q in (0.7, 0.9, 1.1)]
    _, _, _, sb = smc.smoother(N, y, ms, seed=5, quantiles=p, weights=True)
    assert sb["quantiles"].shape == (T, 3, 3)
    for m in range(3):
        assert same(sb["quantiles"][:, m], ref.quantiles(sb["x"][:, m], sb["weights"][:, m], p)), m
    uc = smc.UCSV((0.2, 0.3), 1.0, (-1.0, -0.5))
    _, _, _, s3 = smc.smoother(N, y, [uc, uc], seed=5, quantiles=[0.5], component=2, weights=True, missing=False)
    assert s3["quantiles"].shape == (T, 2, 1)
    assert same(s3["quantiles"][:, 1], ref.quantiles(s3["x"][:, 1, :, 2], s3["weights"][:, 1], [0.5]))
    mu = smc.MarginalUCSV((0.2, 0.3), 1.0, (-1.0, -0.5))
    with pytest.raises(L.SmcError):
        smc.smoother(N, y, mu, seed=5, quantiles=p)


def test_smoothed_quantiles_of_a_sampler(L):
    """smoothed_quantiles == the omega-average, formed by hand, of per-filter smoother(..., rows=..., quantiles=p) results in
    OTHER blocks than its own (two, forced by max_bytes): the filters' streams make the blocks immaterial"""
    import sequential_monte_carlo_amd as smc
    from sequential_monte_carlo_amd import smc_samplers
    from ibis_reference import case_readme
    tmap, prior, model = case_readme(smc)
    _, y = smc.simulate(smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8), 8, seed=4)
    s = smc.SMC(64, 8, model, prior, 2, 0.6, seed=22, theta_map=tmap)                   # 64 state particles, 8 parameter particles
    smc.smc2(s, y)
    p, N, M, seed = [0.25, 0.5, 0.75], 64, 8, 991
    per_theta = y.size * N * 3 * 8
    got = smc.smoothed_quantiles(s, y, p, seed=seed, max_bytes=4 * per_theta)           # two blocks of 4
    assert got.shape == (y.size, 3) and np.all(np.diff(got, axis=1) >= 0)
    mid, raw = smc_samplers._rows(s._models(s.theta))
    om = np.asarray(s.omega, dtype=np.float64)
    assert raw.shape[0] == M and om.shape == (M,)
    want = np.zeros((y.size, 3))
    for m0 in range(0, M, 2):                                                           # four blocks of 2, summed in index order
        _, _, _, sm = smc.smoother(N, y, None, rows=(int(mid), raw[m0:m0 + 2]), seed=seed, streams=np.arange(m0, m0 + 2, dtype=np.uint32), quantiles=p)
        for k in range(2):
            if om[m0 + k] > 0:
                want += om[m0 + k] * sm["quantiles"][:, k]
    assert same(got, want)
    assert same(got, smc.smoothed_quantiles(s, y, p, seed=seed))                         # one block
    mean, _ = smc.smoothed_state(s, y, seed=seed, max_bytes=4 * per_theta)               # the same records: the band belongs to this mean
    assert np.all(np.abs(got[:, 1] - mean) < 1.0)
    s.backend.close()


def test_median_and_tail_against_the_kalman_smoother(L):
    """LG1D, the README's parameters, N = 1024, T = 20, seeds 1..16: z_t = (q50_t - xs_t) / sqrt(Ps_t) with (xs, Ps) of the exact
    Kalman smoother; the mean of z over seeds and t within 4 standard errors, the standard error from the spread of the 16
    per-seed means; the same for q(0.05) against xs_t - 1.6449 sqrt(Ps_t).  No tolerance fixed in advance."""
    import sequential_monte_carlo_amd as smc
    K, N, T = 16, 1024, 20
    m0 = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
    _, y = smc.simulate(m0, T, seed=1998)
    xs, Ps = smc.kalman_smoother(y, m0)
    z = np.zeros((K, 2))
    for k in range(K):
        _, _, _, s = smc.smoother(N, y, m0, seed=1 + k, quantiles=[0.5, 0.05])
        z[k, 0] = np.mean((s["quantiles"][:, 0] - xs) / np.sqrt(Ps))
        z[k, 1] = np.mean((s["quantiles"][:, 1] - (xs - 1.6449 * np.sqrt(Ps))) / np.sqrt(Ps))
    mean, se = z.mean(axis=0), z.std(axis=0, ddof=1) / np.sqrt(K)
    print("median: mean z %.5f, se %.5f (%.2f se); 5 %% point: mean z %.5f, se %.5f (%.2f se)" % (
        mean[0], se[0], mean[0] / se[0], mean[1], se[1], mean[1] / se[1]))
    assert np.all(np.abs(mean) <= 4 * se), (mean, se)
