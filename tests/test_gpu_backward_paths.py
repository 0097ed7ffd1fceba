"""Backward simulation on the GPU (pytest -m gpu): smc_sample_paths over the record of a step-by-step run.

  * smc_sample_paths == smc_host_sample_paths on the recorded clouds: the indices equal as integers, the states bit for bit (the
    host twin is pinned to a long-double CDF, to the smoothed weights and to the RTS joint law by tests/test_paths_host.py)
  * planted clouds through smc_history_put: device == host
  * a filter alone == the same filter inside a batch; repeated calls and runs; counts; independence of smc_smooth
  * the Rauch-Tung-Striebel pin of the joint law and the chi-square of the marginals against the device's own smc_smooth
  * every refusal and state rule of include/smc_hip.h; the Python layer (smoother(paths=...), smoothed_paths)
"""
import numpy as np
import pytest

import paths_reference as PR
import smoother_planted as P
import smoother_reference as R

pytestmark = pytest.mark.gpu

LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
LG_SHARP = [0.5, 1.0, 0.9, 1e-4, 0.0, 1.0]
SV = [-1.0, 0.95, 0.3]
UC = [0.2, 0.3, 1.0, -1.0, -0.5]
RAW = {1: LG, 2: SV, 3: UC}
NONE, OPTIMAL = 0, 2
SYSTEMATIC = 4
SEED = 0x5EEDC0FFEE12345


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def rows_for(raw, nth):
    """nth distinct parameter rows around raw (the transition scales differ)"""
    r = np.tile(np.asarray(raw, dtype=float), (nth, 1))
    k = 2 if len(raw) != 5 else 0
    r[:, k] *= 1.0 + 0.15 * np.arange(nth)
    return r


def run_recorded(L, model, rows, n, seg, T, proposal=NONE, flags=0, seed=11, streams=None):
    """a handle after T recorded steps of the step API"""
    rows = np.atleast_2d(rows)
    h = L.Handle(model, rows.shape[0], n, seg=seg, seed=seed, flags=flags)
    h.set_params(rows)
    if streams is not None:
        h.set_streams(streams)
    if proposal != NONE:
        h.set_proposal(proposal)
    _, y = L.simulate(model, RAW[model], max(T, 2), 1998)
    h.history_begin(T)
    for t in range(T):
        h.init(float(y[0])) if t == 0 else h.step(float(y[t]))
    assert h.history_len() == T
    return h


def clouds(h):
    T = h.history_len()
    xs, ws = zip(*[h.history_get(t) for t in range(T)])
    return np.array(xs), np.array(ws)      # [T][d][ntheta][n], [T][ntheta][n]


def compare_with_host(L, h, model, rows, M, seed=SEED, filters=None):
    """the device's paths of the chosen filters against the host twin on the recorded clouds; returns (x, w, idx, xs)"""
    x, w = clouds(h)
    idx, xs = h.sample_paths(M, seed)
    rows = np.atleast_2d(rows)
    assert idx.shape == (x.shape[0], rows.shape[0], M) and xs.shape == (x.shape[0], x.shape[1], rows.shape[0], M)
    for m in (range(rows.shape[0]) if filters is None else filters):
        hi, hx = L.host_sample_paths(model, rows[m], x[:, :, m, :], w[:, m, :], M, seed, m)      # (filter m draws on stream m)
        assert np.array_equal(idx[:, m], hi), ("indices", m)
        assert same(xs[:, :, m], hx), ("states", m)
    return x, w, idx, xs


# (model, row, proposal, flags, n, seg, n_theta, T, M): the smallest shapes that can go wrong - one particle, a partial chunk (65),
# two segments with padding (300 / 256), 11 chunks (more than SMOOTH_MAX_DIRECT: the row-maximum launch) with a partial one
# (1300 / 256), whole tiles (1024); M = 1, a partial wave either side of 64 (63, 65), a partial tile (300), M > n and M < n
CASES = [
    (1, LG, NONE, 0, 1, 0, 3, 12, 65),
    (1, LG, NONE, 0, 65, 0, 3, 12, 63),
    (1, LG, NONE, 0, 65, 0, 3, 12, 300),
    (1, LG, NONE, 0, 300, 256, 3, 12, 300),
    (1, LG, NONE, 0, 1300, 256, 3, 12, 65),
    (1, LG, NONE, 0, 1024, 0, 1, 12, 300),
    (1, LG, NONE, 0, 1024, 0, 3, 2, 1),
    (1, LG, NONE, 0, 300, 256, 1, 1, 65),
    (1, LG, NONE, 0, 300, 256, 3, 1, 300),
    (1, LG, NONE, 0, 300, 256, 1, 2, 63),
    (1, LG_SHARP, NONE, 0, 300, 256, 3, 12, 300),
    (1, LG_SHARP, NONE, 0, 1024, 0, 1, 12, 65),
    (1, LG, NONE, SYSTEMATIC, 300, 256, 3, 12, 65),
    (1, LG, OPTIMAL, 0, 300, 256, 3, 12, 65),
    (2, SV, NONE, 0, 65, 0, 3, 12, 300),
    (2, SV, NONE, 0, 300, 256, 1, 12, 63),
    (2, SV, NONE, 0, 1300, 256, 1, 2, 300),
    (3, UC, NONE, 0, 1, 0, 3, 2, 65),
    (3, UC, NONE, 0, 65, 0, 3, 12, 300),
    (3, UC, NONE, 0, 300, 256, 3, 12, 63),
    (3, UC, NONE, 0, 1300, 256, 1, 2, 65),
    (3, UC, NONE, 0, 1024, 0, 1, 2, 1),
    (3, UC, OPTIMAL, 0, 300, 256, 3, 12, 65),
]


@pytest.mark.parametrize("model,raw,proposal,flags,n,seg,nth,T,M", CASES)
def test_paths_equal_host_twin(L, model, raw, proposal, flags, n, seg, nth, T, M):
    rows = rows_for(raw, nth)
    h = run_recorded(L, model, rows, n, seg, T, proposal, flags)
    x, w, idx, xs = compare_with_host(L, h, model, rows, M)
    assert np.all(idx >= 0) and np.all(np.isfinite(xs))
    for m in range(nth):                                              # xs is the gather of the record, zero weights never chosen
        for t in range(T):
            assert same(xs[t, :, m], x[t, :, m][:, idx[t, m]]) and np.all(w[t, m][idx[t, m]] > 0)
    if raw is LG_SHARP:
        assert (w == 0).mean() > 0.5
    h.close()


def test_wide_tiles_equal_host_twin(L):
    """32 filters of 11 chunks and 3 tiles of 256 paths: 1056 workgroups, the launch takes tiles of 256 threads (a lone filter
    takes one wave per tile); three filters of the batch against the host twin, one against the same filter alone"""
    rows = rows_for(LG, 32)
    h = run_recorded(L, 1, rows, 1300, 256, 2)
    _, _, idx, xs = compare_with_host(L, h, 1, rows, 768, filters=(0, 17, 31))
    h1 = run_recorded(L, 1, rows[5], 1300, 256, 2, streams=[5])
    i1, x1 = h1.sample_paths(768, SEED)
    assert np.array_equal(i1[:, 0], idx[:, 5]) and same(x1[:, :, 0], xs[:, :, 5])
    h.close(); h1.close()


@pytest.mark.parametrize("model,raw", [(1, LG), (3, UC)])
def test_many_paths_equal_host_twin(L, model, raw):
    """n_theta M = 32 x 8192 = 262144 paths: the selection takes one thread per path instead of one wave (PATH_WAVE_SELECT of
    csrc/smc_path_kernels.h); the same indices - three filters against the host twin, all against a call just below the
    threshold, which takes the wave shape"""
    rows = rows_for(raw, 32)
    h = run_recorded(L, model, rows, 300, 256, 3)
    _, _, idx, xs = compare_with_host(L, h, model, rows, 8192, filters=(0, 13, 31))
    i2, x2 = h.sample_paths(8191, SEED)
    assert np.array_equal(i2, idx[:, :, :8191]) and same(x2, xs[:, :, :, :8191])
    h.close()


PLANTED = [(1, LG_SHARP, "nan_on_zero"), (1, LG_SHARP, "inf_on_zero"), (1, LG, "tiny_weights"), (1, LG, "far_apart"),
           (3, UC, "tiny_weights"), (3, UC, "far_apart"), (2, SV, "far_apart"), (1, LG, "one_alive")]


@pytest.mark.parametrize("model,raw,name", PLANTED, ids=[p[2] + "-m%d" % p[0] for p in PLANTED])
def test_planted_clouds_equal_host_twin(L, model, raw, name):
    """clouds no filter leaves (tests/smoother_planted.py), put into the record of filter 1 of a batch of two: device == host"""
    T, n, M = 6, 300, 65
    rows = rows_for(raw, 2)
    h = run_recorded(L, model, rows, n, 256, T)
    x, w = clouds(h)
    px, pw = P.variant(name, model, rows[1], x[:, :, 1, :], w[:, 1, :])
    for t in range(T):
        xt, wt = x[t].copy(), w[t].copy()
        xt[:, 1], wt[1] = px[t], pw[t]
        h.history_put(t, xt, wt)
    before = None
    if name in P.ON_ZERO:
        assert (pw == 0).mean() > 0.5 and not np.all(np.isfinite(px))
        before = L.host_sample_paths(model, rows[1], x[:, :, 1, :], w[:, 1, :], M, SEED, 1)
    _, _, idx, xs = compare_with_host(L, h, model, rows, M)
    assert np.all(idx >= 0) and np.all(np.isfinite(xs))
    if before is not None:                                            # states on zero-weight particles change nothing
        assert np.array_equal(idx[:, 1], before[0]) and same(xs[:, :, 1], before[1])
    h.close()


@pytest.mark.parametrize("model,raw", [(1, LG), (3, UC)])
def test_collapsed_step_has_no_paths(L, model, raw):
    """every weight of one recorded step of filter 0 is 0: -1 / NaN at every step of that filter, filter 1 as before"""
    T, n, M = 6, 300, 65
    rows = rows_for(raw, 2)
    h = run_recorded(L, model, rows, n, 256, T)
    i0, x0 = h.sample_paths(M, SEED)
    for t_dead in P.dead_steps(T):
        x, w = h.history_get(t_dead)
        wd = w.copy()
        wd[0] = 0.0
        h.history_put(t_dead, None, wd)
        _, _, idx, xs = compare_with_host(L, h, model, rows, M)
        assert np.all(idx[:, 0] == -1) and np.all(np.isnan(xs[:, :, 0]))
        assert np.array_equal(idx[:, 1], i0[:, 1]) and same(xs[:, :, 1], x0[:, :, 1])
        h.history_put(t_dead, None, w)
    h.close()


def test_a_path_ends_where_no_source_reaches_it(L):
    """a planted target whose distance to every source overflows when squared: the path has its last step, -1 / NaN before it"""
    rows = rows_for(LG, 2)
    h = run_recorded(L, 1, rows, 65, 0, 3)
    x, w = h.history_get(2)
    x[0, 1, :] = 1e200
    h.history_put(2, x, None)
    _, _, idx, xs = compare_with_host(L, h, 1, rows, 65)
    assert np.all(idx[2] >= 0) and np.all(idx[:2, 1] == -1) and np.all(idx[:2, 0] >= 0)
    assert np.all(np.isnan(xs[:2, :, 1])) and np.all(xs[2, :, 1] == 1e200)
    h.close()


def test_position_independence_repeatability_counts(L):
    rows = rows_for(LG, 3)
    M = 65
    hb = run_recorded(L, 1, rows, 300, 256, 12, streams=[0, 1, 2])
    ib, xb = hb.sample_paths(M, SEED)
    i2, x2 = hb.sample_paths(M, SEED)                          # the same handle again
    assert np.array_equal(ib, i2) and same(xb, x2)
    assert not np.array_equal(hb.sample_paths(M, SEED + 1)[0], ib)    # another seed: other paths
    hb2 = run_recorded(L, 1, rows, 300, 256, 12, streams=[0, 1, 2])
    i3, x3 = hb2.sample_paths(M, SEED)                         # a second run
    assert np.array_equal(ib, i3) and same(xb, x3)
    for m in range(3):                                         # a filter alone, on its stream
        h1 = run_recorded(L, 1, rows[m], 300, 256, 12, streams=[m])
        i1, x1 = h1.sample_paths(M, SEED)
        assert np.array_equal(i1[:, 0], ib[:, m]) and same(x1[:, :, 0], xb[:, :, m]), m
        h1.close()
    # the first paths of a larger M are those of a smaller one
    i300, x300 = hb.sample_paths(300, SEED)
    assert np.array_equal(i300[:, :, :M], ib) and same(x300[:, :, :, :M], xb)
    # counts: the slots below the count are those of the uniform call, the slots above read -1 / NaN, 0 leaves a filter out
    counts = np.array([M, 0, 17], dtype=np.int32)
    ic, xc = hb.sample_paths(M, SEED, counts=counts)
    for m, c in enumerate(counts):
        assert np.array_equal(ic[:, m, :c], ib[:, m, :c]) and same(xc[:, :, m, :c], xb[:, :, m, :c]), m
        assert np.all(ic[:, m, c:] == -1) and np.all(np.isnan(xc[:, :, m, c:])), m
    assert hb.sample_paths(M, SEED, want_x=False)[1] is None and np.array_equal(hb.sample_paths(M, SEED, want_x=False)[0], ib)
    for hh in (hb, hb2):
        hh.close()


def test_independent_of_smc_smooth_and_more_steps(L):
    rows = rows_for(UC, 2)
    M = 63
    ha = run_recorded(L, 3, rows, 300, 256, 6)                 # never smoothed
    ia, xa = ha.sample_paths(M, SEED)
    hs = run_recorded(L, 3, rows, 300, 256, 6)
    ws0 = hs.smooth()[0]                                       # smoothed before
    ib, xb = hs.sample_paths(M, SEED)
    ws1 = hs.smooth()[0]                                       # and after: the same weights, the same paths
    ic, xc = hs.sample_paths(M, SEED)
    assert np.array_equal(ia, ib) and same(xa, xb) and np.array_equal(ia, ic) and same(xa, xc)
    assert same(ws0, ws1) and same(ws0, ha.smooth()[0])
    ha.close(); hs.close()
    # one more recorded step: the paths use the longer series
    _, y = L.simulate(1, LG, 14, 1998)
    h = L.Handle(1, 1, 300, seg=256, seed=11)
    h.set_params(rows_for(LG, 1))
    h.history_begin(14)
    h.init(float(y[0]))
    for t in range(1, 12):
        h.step(float(y[t]))
    i12, _ = h.sample_paths(M, SEED)
    assert i12.shape[0] == 12
    h.step(float(y[12]))
    _, _, i13, _ = compare_with_host(L, h, 1, rows_for(LG, 1), M)
    assert i13.shape[0] == 13 and not np.array_equal(i13[:12], i12)
    h.close()


def test_rts_pin_on_the_device(L):
    """tests/test_paths_host.py's joint law at n = 1024, M = 1024, T = 24, K = 32 filters (streams 0..31 of one handle): the path
    means and the lag-one covariances over the paths, averaged over the filters, within 4.5 standard errors of the exact RTS
    values at every t; the covariances are far from 0 (independent draws from the marginals would not pass)"""
    T, K, n, M = 24, 32, 1024, 1024
    _, y = L.simulate(1, LG, T, 1998)
    m_rts, _ = R.rts_smoother(LG, y)
    C_rts = PR.rts_lag_one(LG, y)
    h = L.Handle(1, K, n, seed=77)
    h.set_params(np.tile(LG, (K, 1)))
    h.history_begin(T)
    for t in range(T):
        h.init(float(y[0])) if t == 0 else h.step(float(y[t]))
    idx, xs = h.sample_paths(M, SEED)
    assert np.all(idx >= 0)
    mc = [PR.path_moments(xs[:, 0, k, :]) for k in range(K)]
    means, covs = np.array([m for m, _ in mc]), np.array([c for _, c in mc])
    zm, zc, z0 = PR.z_scores(means, m_rts), PR.z_scores(covs, C_rts), PR.z_scores(covs, 0.0)
    print("max z of the means %.2f, of the covariances %.2f; the covariances against 0: min z %.1f" % (zm.max(), zc.max(), z0.min()))
    assert np.all(zm <= 4.5), zm
    assert np.all(zc <= 4.5), zc
    assert (z0 > 4.5).sum() > (T - 1) // 2, z0
    h.close()


def test_marginals_against_the_device_smoother(L):
    """n = 64, T = 6, M = 20000, LG1D and UCSV3D: the counts of idx[t] against M ws_t of the device's own smc_smooth at two steps,
    chi-square below the 1 - 1e-6 quantile; against the filter weights of step 0 it is above"""
    n, T, M = 64, 6, 20000
    for model in (1, 3):
        h = run_recorded(L, model, RAW[model], n, 0, T)
        ws = h.smooth()[0][:, 0]
        w = clouds(h)[1][:, 0]
        idx, _ = h.sample_paths(M, 20260117, want_x=False)
        for t in (0, 3):
            counts = np.bincount(idx[t, 0], minlength=n)
            stat, cells = PR.chi2_cells(counts, M * ws[t])
            print("model %d t %d: chi2 %.1f (%d cells, bound %.1f)" % (model, t, stat, cells, PR.chi2_bound(cells - 1)))
            assert stat <= PR.chi2_bound(cells - 1), (model, t, stat)
        fstat, fcells = PR.chi2_cells(np.bincount(idx[0, 0], minlength=n), M * w[0])
        assert fstat > PR.chi2_bound(fcells - 1), (model, fstat)
        h.close()


def test_refusals_and_state_rules(L):
    lib = L.lib()
    EINVAL, ESTATE = -1, -3
    ip = L._i32p
    _, y = L.simulate(1, LG, 4, 1998)
    h = L.Handle(1, 2, 300, seg=256, seed=3)
    h.set_params(rows_for(LG, 2))
    assert lib.smc_sample_paths(h._h, 4, 1, None, None, None) == ESTATE          # not armed
    h.history_begin(3)
    assert lib.smc_sample_paths(h._h, 4, 1, None, None, None) == ESTATE          # armed, nothing recorded
    with pytest.raises(L.SmcError):
        h.sample_paths(4, 1)
    h.init(float(y[0]))
    h.step(float(y[1]))
    assert lib.smc_sample_paths(h._h, 4, 1, None, None, None) == 0               # no output asked for: allowed
    for M in (0, -1, (1 << 30) + 1):
        assert lib.smc_sample_paths(h._h, M, 1, None, None, None) == EINVAL
    for bad in ([5, 0], [0, -1]):
        c = np.array(bad, dtype=np.int32)
        assert lib.smc_sample_paths(h._h, 4, 1, c.ctypes.data_as(ip), None, None) == EINVAL
    assert lib.smc_sample_paths(None, 4, 1, None, None, None) == EINVAL
    good = h.sample_paths(4, 1)
    badrows = rows_for(LG, 2)
    for v in (0.0, -1.0, np.nan, np.inf):
        badrows[1, 2] = v
        h.set_params(badrows)
        assert lib.smc_sample_paths(h._h, 4, 1, None, None, None) == EINVAL
    h.set_params(rows_for(LG, 2))
    again = h.sample_paths(4, 1)                                                 # the refusals changed nothing
    assert np.array_equal(good[0], again[0]) and same(good[1], again[1])
    h.history_end()
    assert lib.smc_sample_paths(h._h, 4, 1, None, None, None) == ESTATE
    h.close()
    rb = L.Handle(L.MODEL_UCSV_RB, 1, 300, seed=3)
    rb.set_params(np.array([UC]))
    rb.history_begin(2)
    rb.init(0.3)
    assert lib.smc_sample_paths(rb._h, 4, 1, None, None, None) == EINVAL
    rb.close()
    big = L.Handle(1, 1, (1 << 20) + 1, seed=3)                                  # n_x > 2^20: the integer sum of a step could pass 2^61
    big.set_params(np.array([LG]))
    big.history_begin(1)
    big.init(float(y[0]))
    assert big.history_len() == 1
    assert lib.smc_sample_paths(big._h, 4, 1, None, None, None) == EINVAL and b"2^20" in lib.smc_last_error()
    big.close()


def test_smoother_paths_python_shapes(L):
    import sequential_monte_carlo_amd as smc
    T, N, M = 6, 300, 40
    m1 = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
    _, y = smc.simulate(m1, T, seed=1998)
    x, w, logZ, s = smc.smoother(N, y, m1, seed=5, weights=True, paths=M)
    assert s["paths"].shape == (T, M) and s["path_index"].shape == (T, M) and s["path_index"].dtype == np.int32
    assert s["mean"].shape == (T,) and s["weights"].shape == (T, N)
    assert same(s["paths"], np.take_along_axis(s["x"], s["path_index"].astype(np.int64), axis=1))
    _, _, logZ0, s0 = smc.smoother(N, y, m1, seed=5, weights=True)               # weights / mean / var unchanged by paths=
    assert logZ0 == logZ and same(s0["weights"], s["weights"]) and same(s0["mean"], s["mean"]) and same(s0["var"], s["var"])
    assert "paths" not in s0
    _, _, _, s2 = smc.smoother(N, y, m1, seed=5, paths=M)                        # the default seed is a function of the filter seed
    assert same(s2["paths"], s["paths"])
    _, _, _, s2 = smc.smoother(N, y, m1, seed=5, paths=M, path_seed=123)
    assert not same(s2["paths"], s["paths"])
    ms = [smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=q, R=0.8) for q in (0.7, 0.9, 1.1)]
    _, _, _, s = smc.smoother(N, y, ms, seed=5, paths=M)
    assert s["paths"].shape == (T, 3, M) and s["path_index"].shape == (T, 3, M)
    uc = smc.UCSV((0.2, 0.3), 1.0, (-1.0, -0.5))
    _, _, _, s3 = smc.smoother(N, y, uc, seed=5, paths=M, weights=True)
    assert s3["paths"].shape == (T, M, 3) and s3["path_index"].shape == (T, M)
    assert same(s3["paths"], np.take_along_axis(s3["x"], s3["path_index"].astype(np.int64)[:, :, None], axis=1))
    _, _, _, s3 = smc.smoother(N, y, [uc, uc], seed=5, paths=M)
    assert s3["paths"].shape == (T, 2, M, 3) and s3["path_index"].shape == (T, 2, M)
    # smooth=False leaves the backward pass of the marginals out; path_counts draws only the first paths of each filter
    _, _, _, sf = smc.smoother(N, y, ms, seed=5, paths=M, smooth=False, path_counts=[M, 0, 7])
    assert "mean" not in sf and "var" not in sf and "weights" not in sf and sf["logmu"].shape == (T, 3)
    assert np.array_equal(sf["path_index"][:, 0], s["path_index"][:, 0]) and same(sf["paths"][:, 2, :7], s["paths"][:, 2, :7])
    assert np.all(sf["path_index"][:, 1] == -1) and np.all(np.isnan(sf["paths"][:, 2, 7:]))
    with pytest.raises(L.SmcError):
        smc.smoother(N, y, smc.MarginalUCSV((0.2, 0.3), 1.0, (-1.0, -0.5)), seed=5, paths=M, smooth=False)


def test_smoothed_paths_of_a_sampler(L):
    import sequential_monte_carlo_amd as smc
    Mth, N, T, M = 8, 64, 12, 50
    m0 = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
    _, y = smc.simulate(m0, T, seed=1998)
    prior = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(), smc.LogNormal()])
    s = smc.SMC(N, Mth, lambda th: smc.UnivariateLinearGaussian(A=th[0], B=1.0, Q=th[1], R=th[2]), prior, 2, 0.5, seed=22)
    smc.smc2(s, y[:1])
    for t in range(2, 6):
        smc.smc2_step(s, y, t, verbose=False)
    paths = smc.smoothed_paths(s, y, M, seed=99)
    assert paths.shape == (T, M) and np.all(np.isfinite(paths))
    assert same(paths, smc.smoothed_paths(s, y, M, seed=99, max_bytes=1))         # one parameter particle per block: the same bits
    assert same(paths, smc.smoothed_paths(s, y, M, seed=99))
    assert not same(paths, smc.smoothed_paths(s, y, M, seed=100))
    # by hand: the ancestors of the library's outer resampler, then the paths of each drawn parameter particle alone
    anc = L.host_outer_resample(s.logw, M, 99 + 1)
    models = [s.model(th) for th in s.theta]
    k = 0
    for m in np.unique(anc):
        c = int((anc == m).sum())
        _, _, _, sm = smc.smoother(N, y, models[m], seed=99, streams=[m], paths=c, path_seed=99 + 2)
        assert same(paths[:, k:k + c], sm["paths"]), m
        k += c
    # parameter particles of weight 0 are never drawn: all the weight on two of them
    keep = s.logw.copy()
    s._set_logw(np.where(np.isin(np.arange(Mth), (2, 5)), 0.0, -np.inf))
    anc2 = L.host_outer_resample(s.logw, M, 7 + 1)
    assert set(np.unique(anc2)) <= {2, 5}
    p2 = smc.smoothed_paths(s, y, M, seed=7)
    k = 0
    for m in np.unique(anc2):
        c = int((anc2 == m).sum())
        _, _, _, sm = smc.smoother(N, y, models[m], seed=7, streams=[m], paths=c, path_seed=7 + 2)
        assert same(p2[:, k:k + c], sm["paths"]), m
        k += c
    assert k == M
    s._set_logw(keep)
    # a state of three coordinates
    su = smc.SMC(N, 4, lambda th: smc.UCSV((th[0], th[1]), 1.0, (-1.0, -0.5)), smc.product_distribution([smc.LogNormal(), smc.LogNormal()]),
                 2, 0.5, seed=23)
    smc.smc2(su, y[:1])
    assert smc.smoothed_paths(su, y, 9, seed=3).shape == (T, 9, 3)
    su.backend.close()
    # IBIS: out of scope, refused by type before anything runs
    tmap = smc.ThetaMap(1, [0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    ib = smc.IBIS(16, lambda th: smc.LinearModel(th[0], 1.0, th[1], th[2], 0.0, 1.0), prior, 2, 0.5, seed=3, theta_map=tmap)
    with pytest.raises(TypeError, match="RTS"):
        smc.smoothed_paths(ib, y, 4)
    ib.close()
    s.backend.close()
