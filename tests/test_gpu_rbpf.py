"""The marginal (Rao-Blackwellised) UCSV family on the GPU (pytest -m gpu): SMC_MODEL_UCSV_RB on every launch path.

  1. the device twin of the step equals the host twin bit for bit
  2. the launch paths agree among themselves bit for bit; a one-step audit recomputes every particle with the host twin
  3. Kalman pin: with (nearly) frozen volatilities logZ is the exact Kalman log-likelihood of the local-level model
  4. unbiased for the same p(y) as bootstrap UCSV and as oracle/rbpf_ucsv.py
  5. the variance it is for: below bootstrap UCSV's and OPTIMAL-guided UCSV's at equal Nx
  6. summaries of all four rows in both modes against exact host sums; trend_moments
  7. the samplers with ThetaMap(MODEL_UCSV_RB, ...)
  8. handle state: recycled bundles, smc_set_params after a run
"""
import ctypes as C
import io
import math

import numpy as np
import pytest

import step_edge_inputs
import test_gpu_guided as TG
from quantile7_reference import check_sample_moments, quantile7
from summary_reference import check_moments, check_quantiles, quantile_delta

pytestmark = pytest.mark.gpu

UC, RB = 3, 4
ROW = [0.2, 0.2, 3.0, 0.0, 0.0]
NO_RESIDENT = 2
same, bits, snapshot, assert_same_snapshot, PATHS = TG.same, TG.bits, TG.snapshot, TG.assert_same_snapshot, TG.PATHS


def raws_for(nth):
    r = np.tile(ROW, (nth, 1)).astype(float)
    r[:, 0] *= 1.0 - 0.3 * np.arange(nth) / max(nth, 1)
    r[:, 3] -= 0.5 * np.arange(nth)
    return r


def series(T, seed=1998, row=ROW):
    from sequential_monte_carlo_amd import _lib as L
    return L.simulate(UC, row, T, seed)[1]


def run(L, path, model=RB, seed=7, T=12, nth=3):
    """one series on one path of test_gpu_guided.PATHS: (logmu trace, ess trace, snapshot)"""
    n, seg, flags, how, skip = PATHS[path]
    if n > (1 << 20):
        nth, T, skip = 1, 4, None
    y = series(T)
    h = L.Handle(model, nth, n, seg=seg, seed=seed, flags=flags | L.FLAG_ANCESTORS)
    h.set_params(raws_for(nth))
    if how == "ll":
        if skip is not None:
            h.init(y[0])
            h.set_skip(skip)
        _, lm, es = h.log_likelihood(y, trace=True)
    elif how == "step":
        lm, es = np.zeros((T, nth)), np.zeros((T, nth))
        lm[0] = h.init(y[0])
        _, es[0] = h.logZ()
        for t in range(1, T):
            lm[t], es[t] = h.step(y[t])
    else:                                      # windows of 5 of which 3 are kept (j < k), then the rest
        lm, es = np.zeros((T, nth)), np.zeros((T, nth))
        lm[0] = h.init(y[0])
        _, es[0] = h.logZ()
        t = 1
        while t < T:
            k = min(5, T - t)
            j = 3 if k == 5 else k
            wl, we = h.step_window(y[t:t + k])
            h.step_commit(j)
            lm[t:t + j], es[t:t + j] = wl[:j], we[:j]
            t += j
    out = (lm, es, snapshot(h), (h.seg, h.nseg, h.resident, h.d))
    h.close()
    return out


# ---- 1. device twin == host twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [False, True])
def test_device_rb_step_equals_host(L, first):
    raw, sp, z, y = step_edge_inputs.rb(first)
    s, lw = L.device_rb_step(raw, sp, z, y, first)
    for i in range(sp.shape[1]):
        hs, hl = L.host_rb_step(raw, sp[:, i], z[:, i], 0.7, first)
        assert same(s[:, i], hs) and same([lw[i]], [hl]), (i, s[:, i], hs, lw[i], hl)


# ---- 2. launch paths ---------------------------------------------------------------------------------------------------
GROUPS = TG.GROUPS


@pytest.mark.parametrize("group", list(GROUPS))
def test_paths_agree(L, group):
    """x, w, ancestors, the raw fixed-point weights, logZ, ess and the traces, bit for bit within a group of paths that share
    geometry, law and seed; the family is not UCSV run by another name (its logZ differs from the bootstrap filter's)"""
    ref = None
    for path in GROUPS[group]:
        out = run(L, path)
        assert out[3][3] == 4
        if group == "one-segment":
            assert out[3][1] == 1 and out[3][2] == (path != "no-resident"), (path, out[3])
        if ref is None:
            ref = out
            boot = run(L, path, model=UC)
            assert not same(boot[0], out[0])
            continue
        assert same(ref[0], out[0]), (path, "logmu")
        assert same(ref[1], out[1]) if path != "window" else same(ref[1][-1], out[1][-1]), (path, "ess")
        assert_same_snapshot(ref[2], out[2], (path,))


def test_every_other_path_runs(L):
    """ragged, two records per thread, systematic, skip masks and a filter above 2^20: a finite logZ close to the bootstrap
    filter's (both estimate log p(y)), P > 0 everywhere, skipped filters not run and their state kept"""
    for path in ("resident-ragged", "two-records", "systematic", "systematic-multi", "skip", "skip-multi", "above-2^20"):
        g = run(L, path)
        b = run(L, path, model=UC)
        z, x = g[2][-2], g[2][0]
        skip = PATHS[path][4]
        if skip is not None:
            n, seg, flags = PATHS[path][:3]
            k = L.Handle(RB, 3, n, seg=seg, seed=7, flags=flags | L.FLAG_ANCESTORS)
            k.set_params(raws_for(3))
            k.init(series(12)[0])
            kept = snapshot(k)
            k.close()
        for th in range(len(z)):
            if skip is not None and skip[th]:
                assert z[th] == -np.inf, (path, th)
                assert same(x[:, th], kept[0][:, th]) and same(g[2][1][th], kept[1][th]), (path, th, "a skipped filter keeps its state")
            else:
                assert np.isfinite(z[th]) and abs(z[th] - b[2][-2][th]) < 3.0, (path, th, z[th], b[2][-2][th])
                assert np.all(x[3, th] > 0) and np.all(np.isfinite(x[:, th])), (path, th)


def normals(L, seed, stream, t, slot, n):
    """the state normals of slot `slot` at step t of the particles 0..n-1 of a filter: Philox counter (pair, stream, t, slot),
    key = the seed's halves; Box-Muller's first value for particle 2p, the second for 2p + 1 (smc_spec.h)"""
    lib = L.lib()
    u32 = C.c_uint32 * 4
    key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32)
    out = u32()
    z = np.zeros(n + (n & 1))
    z0, z1 = C.c_double(), C.c_double()
    for p in range((n + 1) // 2):
        lib.smc_host_philox4x32_10(u32(p, stream, t, slot), key, out)
        lib.smc_host_box_muller(out, C.byref(z0), C.byref(z1))
        z[2 * p], z[2 * p + 1] = z0.value, z1.value
    return z[:n]


@pytest.mark.parametrize("n,seg", [(1000, 0), (10000, 256)], ids=["one-segment-ragged", "multi-segment"])
def test_one_step_audit(L, n, seg):
    """(x_old, ancestors, x_new) around the first step and around a later smc_step: every particle recomputed by the host twin from
    its ancestor's state, the observation and its two normals (Philox slots 1 and 2 of the particle's pair) - the same bits in all
    four rows; the weights are the normalisation of the twin's log-weights (the oracle-pinned normalize: to 1e-12 here)"""
    seed, stream = 23, 5
    y = series(3)
    raw = np.asarray(ROW)
    h = L.Handle(RB, 1, n, seg=seg, seed=seed, flags=L.FLAG_ANCESTORS)
    h.set_params(raw[None, :])
    h.set_streams(np.array([stream], dtype=np.uint32))
    h.init(y[0])
    x1, w1, _ = h.state()
    h.step(y[1])
    x_old, _, _ = h.state()
    h.step(y[2])
    x_new, w_new, anc = h.state()
    h.close()
    for t, xo, xn, wn, a in ((0, None, x1, w1, np.arange(n)[None]), (2, x_old, x_new, w_new, anc)):
        za, zb = normals(L, seed, stream, t, 1, n), normals(L, seed, stream, t, 2, n)
        lw = np.zeros(n)
        for i in range(n):
            sp = np.zeros(4) if t == 0 else xo[:, 0, a[0, i]]
            s, lw[i] = L.host_rb_step(raw, sp, [za[i], zb[i]], y[t], t == 0)
            assert same(s, xn[:, 0, i]), (t, i, s, xn[:, 0, i])
        u = np.exp(lw - lw.max())
        assert np.allclose(wn[0], u / u.sum(), rtol=1e-9, atol=1e-15), t


# ---- 3. Kalman pin -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lse0,lsn0", [(0.0, 0.0), (-1.0, 0.5)])
@pytest.mark.parametrize("path", ["resident", "no-resident", "multi-seg256"])
def test_kalman_pin(L, path, lse0, lsn0):
    """gamma = 1e-10, T = 100: the volatilities stay within gamma sqrt(T) of (lse0, lsn0), every particle carries the Kalman filter
    of unobserved_components(sigma_eps = exp(lse0), sigma_eta = exp(lsn0), x0), and logZ is its exact log-likelihood
    (predict_first=False) within the first-order bound 10 T gamma sqrt(T) = 1e-6 (|d logZ / d log Q|, |d logZ / d log R| are O(1)
    per step; 10 is headroom).  tests/test_rbpf_host.py checks the numpy filter of oracle/rbpf_ucsv.py against the same bound."""
    import sequential_monte_carlo_amd as smc
    g, T = 1e-10, 100
    n, seg, flags = PATHS[path][:3]
    y = series(T, seed=7)
    kf = smc.log_likelihood_kalman(y, smc.unobserved_components(sigma_eps=math.exp(lse0), sigma_eta=math.exp(lsn0), x0=3.0), predict_first=False)[2]
    h = L.Handle(RB, 2, n, seg=seg, seed=3, flags=flags)
    h.set_params(np.tile([g, g, 3.0, lse0, lsn0], (2, 1)))
    z = h.log_likelihood(y)
    x, w, _ = h.state(want_anc=False)
    h.close()
    bound = 10 * T * g * math.sqrt(T)
    print("kalman pin %s (%g, %g): logZ - KF = %s, bound %.3g" % (path, lse0, lsn0, z - kf, bound))
    assert np.all(np.abs(z - kf) <= bound), (z, kf)
    assert np.ptp(x[0]) <= 1e-6 and np.ptp(x[3]) <= 1e-6          # one Kalman filter in every particle


# ---- 4. unbiased for the same p(y) ---------------------------------------------------------------------------------------
def many_logZ(L, model, raw, y, K, N, kind=0, seed=5):
    return TG.many_logZ(L, model, raw, y, K, N, kind, None, seed)


def log_mean_exp(z):
    """(log mean exp z, its standard error by the delta method)"""
    c = z.max()
    r = np.exp(z - c)
    return c + math.log(r.mean()), r.std(ddof=1) / math.sqrt(len(r)) / r.mean()


def test_unbiased_for_the_same_likelihood(L):
    """UCSV row (0.2, 0.2, 3, 0, 0), T = 50, Nx = 1024, K = 256 independent filters each of bootstrap UCSV, the new family and the
    numpy filter oracle/rbpf_ucsv.py: log-mean-exp of logZ within 4 combined standard errors (delta method), pairwise.
    K chosen on the CPU with the two references alone (the C oracle's bootstrap filter, seeds 5 / streams 0..255, against the
    numpy filter, default_rng(12)): log-mean-exp -69.1213 (se 0.027) against -69.1233 (se 0.016), z = 0.06;
    var(logZ) 0.196 against 0.062.  Measured on an MI355X: bootstrap -69.1213 (se 0.027), marginal -69.1137 (se 0.016), numpy
    -69.1233 (se 0.016); z = 0.24 against bootstrap, 0.43 against numpy; var(logZ) 0.196 / 0.0625 / 0.0624."""
    from oracle import rbpf_ucsv
    K, N = 256, 1024
    y = series(50)
    zb = many_logZ(L, UC, ROW, y, K, N)
    zr = many_logZ(L, RB, ROW, y, K, N)
    rng = np.random.default_rng(12)
    zn = np.array([rbpf_ucsv.log_likelihood(y, *ROW, n=N, rng=rng) for _ in range(K)])
    (b, sb), (r, sr), (o, so) = log_mean_exp(zb), log_mean_exp(zr), log_mean_exp(zn)
    z1, z2 = (r - b) / math.hypot(sr, sb), (r - o) / math.hypot(sr, so)
    print("unbiased: bootstrap %.4f (se %.4f), marginal %.4f (se %.4f), numpy %.4f (se %.4f); z = %.2f against bootstrap, %.2f against numpy; "
          "var(logZ) %.4f / %.4f / %.4f" % (b, sb, r, sr, o, so, z1, z2, zb.var(ddof=1), zr.var(ddof=1), zn.var(ddof=1)))
    assert abs(z1) <= 4 and abs(z2) <= 4, (z1, z2)


# ---- 5. the variance it is for -------------------------------------------------------------------------------------------
def test_variance_ordering(L):
    """var(logZ) at equal Nx = 1024 over K = 1024 independent filters each, T = 50: the new family below bootstrap UCSV and below
    OPTIMAL-guided UCSV.  Only the ordering is asserted; the numbers live in profiles/rbpf_cost.log.  K: the one-sided F-test at
    1e-3 rejects equality for a ratio below exp(-3.09 sqrt(4 / (K - 1))) = 0.82 (log of a ratio of two sample variances of
    near-normal logZ has variance about 4 / (K - 1)).  Expected from the CPU references: 0.32 against bootstrap (the C oracle's
    filter against oracle/rbpf_ucsv.py, K = 256), and with guided / bootstrap = 0.42-0.60 (profiles/guided_cost.log) about 0.5-0.75
    against guided.
    Measured on an MI355X: bootstrap 0.1856, guided 0.1306, marginal 0.0655; ratios 0.353 and 0.501, both below 0.824."""
    K, N = 1024, 1024
    y = series(50)
    vb = many_logZ(L, UC, ROW, y, K, N).var(ddof=1)
    vg = many_logZ(L, UC, ROW, y, K, N, kind=TG.OPTIMAL).var(ddof=1)
    vr = many_logZ(L, RB, ROW, y, K, N).var(ddof=1)
    crit = math.exp(-3.09 * math.sqrt(4.0 / (K - 1)))
    print("var(logZ), Nx = %d, K = %d: bootstrap %.4f, guided %.4f, marginal %.4f; ratios %.3f, %.3f (significant below %.3f)"
          % (N, K, vb, vg, vr, vr / vb, vr / vg, crit))
    assert vr < vb and vr < vg, (vr, vb, vg)


# ---- 6. summaries --------------------------------------------------------------------------------------------------------
PS = [0.0, 0.05, 0.5, 0.95, 1.0]


@pytest.mark.parametrize("mode", ["weighted", "unweighted"])
@pytest.mark.parametrize("n,seg,flags", [(1024, 0, 0), (2048, 0, 0), (1000, 0, 0), (1024, 0, NO_RESIDENT), (3000, 256, 0), (40000, 256, 0)],
                         ids=["R-1024", "R-2048", "R-1000", "S-1024", "M-3000", "M-40000"])
def test_summaries_exact(L, n, seg, flags, mode):
    """per-step rows of one log_likelihood call, the window's rows and the stand-alone summaries between steps, all four state rows
    (quantiles of each of the four rows in turn), against exact host sums of the cloud a twin handle reads back: the accuracy contracts
    of smc_get_moments / smc_get_quantiles (weighted: tests/summary_reference.py; unweighted: tests/quantile7_reference.py, the
    type-7 quantiles bit for bit).  trend_moments == the variance of the mixture of the cloud."""
    import sequential_monte_carlo_amd as smc
    row = [0.2, 0.2, 1e5, 0.0, 0.0]            # the trend at a level: a variance by sum w x^2 - mean^2 would lose it
    T = 5
    y = series(T, seed=5, row=row)
    raws = np.array([row, [0.3, 0.1, 1e5, -1.0, 0.5]])
    for comp in (0, 1, 2, 3):
        h = L.Handle(RB, 2, n, seg=seg, seed=23, flags=flags)
        h.set_params(raws)
        h.set_summary_mode(mode)
        h.set_summaries(PS, comp, moments=True)
        _, lm, _ = h.log_likelihood(y, trace=True)
        q, mean, var = h.get_summaries(T)
        assert mean.shape == (T, 4, 2)
        k = L.Handle(RB, 2, n, seg=seg, seed=23, flags=flags)
        k.set_params(raws)
        k.set_summary_mode(mode)
        for t in range(T):
            lmt = k.init(y[0]) if t == 0 else k.step(y[t])[0]
            assert same(lmt, lm[t])
            x, w, _ = k.state(want_anc=False)
            qo, (mo, vo) = k.quantiles(PS, comp), k.moments()
            for qq, mm, vv, ctx in ((q[t], mean[t], var[t], "per-step"), (qo, mo, vo, "once")):
                for th in range(2):
                    for c in range(4):
                        if mode == "weighted":
                            check_moments(mm[c, th], vv[c, th], x[c, th], w[th], (ctx, n, t, th, c))
                        else:
                            check_sample_moments(mm[c, th], vv[c, th], x[c, th], (ctx, n, t, th, c))
                    if mode == "weighted":
                        check_quantiles(qq[th], PS, x[comp, th], w[th], quantile_delta(k.n_x, k.nseg, k.seg, math.fsum(w[th])), (ctx, n, t, th))
                    else:
                        assert same(qq[th], quantile7(x[comp, th], PS)), (ctx, n, t, th)
            if mode == "weighted" and comp == 0:
                tm, tv = smc.trend_moments(mean[t].T, var[t].T)            # [n_theta][4] -> [n_theta]
                for th in range(2):
                    m0 = math.fsum(w[th] * x[0, th]) / math.fsum(w[th])
                    mix = math.fsum(w[th] * (x[3, th] + (x[0, th] - m0) ** 2)) / math.fsum(w[th])
                    assert abs(tm[th] - m0) <= 1e-11 * abs(m0) and abs(tv[th] - mix) <= 1e-9 * mix, (n, t, th, tv[th], mix)
        if k.can_window:                        # the window's per-step rows are the step loop's
            g = L.Handle(RB, 2, n, seg=seg, seed=23, flags=flags)
            g.set_params(raws)
            g.set_summary_mode(mode)
            g.set_summaries(PS, comp, moments=True)
            g.init(y[0])
            g.step_window(y[1:])
            qw, mw, vw = g.get_summaries(T - 1)
            assert same(qw, q[1:]) and same(mw, mean[1:]) and same(vw, var[1:]), (n, mode, comp)
            g.close()
        h.close()
        k.close()


def test_python_surface(L):
    """log_likelihood / the step API through the package with a MarginalUCSV model; moments in the shapes trend_moments takes;
    a proposal is refused with the library's message"""
    import sequential_monte_carlo_amd as smc
    y = series(20)
    m = smc.unobserved_components_stochastic_volatility(x0=3.0, gamma_eps=0.2, gamma_eta=0.2, log_sigma_eps=0.0, log_sigma_eta=0.0, marginal=True)
    x, w, logZ, s = smc.log_likelihood(1024, y, m, seed=3, moments=True)
    assert np.asarray(x).shape == (1024, 4) and s["mean"].shape == (20, 4)
    tm, tv = smc.trend_moments(*x.moments())
    tm2, tv2 = smc.trend_moments(s["mean"][-1], s["var"][-1])
    assert same([tm, tv], [tm2, tv2]) and tv > 0
    xs, ws, l0 = smc.bootstrap_filter(1024, y[0], m, seed=3)
    tot = l0
    for t in range(1, 20):
        lm, ws, _ = smc.bootstrap_filter_(xs, ws, y[t], m)
        tot += lm
    assert abs(tot - logZ) <= 1e-9 and same(np.asarray(xs), np.asarray(x))
    _, _, zu = smc.log_likelihood(1024, y, smc.UCSV((0.2, 0.2), 3.0, (0.0, 0.0)), seed=3)
    assert abs(zu - logZ) < 3.0 and zu != logZ
    with pytest.raises(L.SmcError, match="takes no proposal"):
        smc.log_likelihood(1024, y, m, seed=3, proposal=smc.OptimalProposal())
    h = L.Handle(RB, 1, 1024)
    with pytest.raises(L.SmcError):
        h.set_proposal(1, np.array([[0.0, 1.0, 0.0, 1.0]]))
    h.set_proposal(0)
    h.close()


# ---- 7. samplers ---------------------------------------------------------------------------------------------------------
def sampler_setup(model_id):
    import sequential_monte_carlo_amd as smc
    prior = smc.product_distribution([smc.Uniform(0.02, 0.6), smc.Uniform(0.02, 0.6)])      # a narrow support: proposals leave it
    tmap = smc.ThetaMap(model_id, [0, 1, -1, -1, -1], [0.0, 0.0, 3.0, 0.0, 0.0])
    cls = smc.MarginalUCSV if model_id == RB else smc.UCSV
    return prior, tmap, (lambda th: cls((th[0], th[1]), 3.0, (0.0, 0.0)))


def run_dt(model_id, N, M, y, seed=3, seg=0, flags=0, chain=3, ess_threshold=0.95):
    import sequential_monte_carlo_amd as smc
    prior, tmap, mod = sampler_setup(model_id)
    b = smc.smc_samplers.HipBackend(seg=seg)
    b.flags |= flags
    s = smc.SMC(N, M, mod, prior, chain, ess_threshold, seed=seed, backend=b, theta_map=tmap)
    assert s.device_pmmh
    stages = smc.density_tempered(s, y, verbose=True, out=io.StringIO())
    out = (s.theta.copy(), s.logZ.copy(), s.logw.copy(), s.ess, s.psteps_skipped, stages)
    b.close()
    return out


def run_online(model_id, N, M, y, seed=5, seg=0, flags=0, window=8, min_ar=-1.0, ess_threshold=0.95):
    """-> (theta, logZ, logw, x, w, N, resample-moves made by smc2_run, its verbose text, estimated_trend, particle-steps skipped).
    The ESS threshold (of run_dt's ladder as well) is
    high (0.95 M): the series carries little information on the gammas, and at 0.5 M the outer ESS never falls below the threshold
    within these few periods - no resample-move, and with it no exchange!, would run."""
    import sequential_monte_carlo_amd as smc
    prior, tmap, mod = sampler_setup(model_id)
    b = smc.smc_samplers.HipBackend(seg=seg)
    b.flags |= flags
    s = smc.SMC(N, M, mod, prior, 2, ess_threshold, min_ar=min_ar, seed=seed, backend=b, theta_map=tmap)
    smc.smc2(s, y)
    text = io.StringIO()
    smc.smc2_run(s, y, 2, len(y), window=window, verbose=True, out=text)
    x, w, _ = s._main.state()
    moves = text.getvalue().count("[rejuvenating]")
    out = (s.theta.copy(), s.logZ.copy(), s.logw.copy(), x, w, s.N, moves, text.getvalue(), smc.estimated_trend(s), s.psteps_skipped)
    b.close()
    return out


def test_samplers(L):
    """density_tempered and smc2 + smc2_run with ThetaMap(MODEL_UCSV_RB, ...) on theta = (gamma_eps, gamma_eta), Uniform(0.02, 0.6)
    priors (proposals outside the support: skipped filters, asserted through the sampler's count of particle-steps it did not run;
    test_pmmh_skips_proposals_outside_the_support checks what a skipped particle keeps), and a forced exchange! (min_ar = 2).  The same seed gives the same bits
    twice on each of: one resident segment, one segment without the resident kernels, several segments (seg = 256); resident
    and not are the same bits (the segment length is part of the random-number contract: another seg is another stream).
    Posterior mean of gamma: within 4 posterior-sd / sqrt(ESS) (of this run alone: the reference run's own error is not added) of a bootstrap-UCSV run on the same data with four
    times the parameter particles and Nx = 2048.  Measured on an MI355X: z = (1.84, -0.90), ESS 71 of 128."""
    import sequential_monte_carlo_amd as smc
    y = series(40, seed=11)
    runs = {}
    for name, seg, flags in (("resident", 0, 0), ("no-resident", 0, NO_RESIDENT), ("seg256", 256, 0)):
        a = run_dt(RB, 512, 32, y, seg=seg, flags=flags)
        b = run_dt(RB, 512, 32, y, seg=seg, flags=flags)
        for u, v in zip(a[:3], b[:3]):
            assert same(u, v), (name, "density_tempered twice")
        assert a[5][-1][0] == 1.0 and np.all(np.isfinite(a[1]))
        assert any(st[2] is not None for st in a[5]), (name, "no stage rejuvenated", a[5])
        assert a[4] > 0, (name, "no PMMH proposal left the support: no filter was skipped")
        runs[name] = a
        o1 = run_online(RB, 256, 24, y[:24], seg=seg, flags=flags)
        o2 = run_online(RB, 256, 24, y[:24], seg=seg, flags=flags)
        for u, v in zip(o1[:5], o2[:5]):
            assert same(u, v), (name, "online twice")
        assert o1[6] >= 1, (name, "no resample-move ran", o1[7])
        assert np.all(np.isfinite(o1[1])) and np.isfinite(o1[8])
        assert o1[9] > 0, (name, "no PMMH proposal left the support: no filter was skipped")
        runs["online-" + name] = o1
    for key in ("", "online-"):
        for u, v in zip(runs[key + "resident"][:3], runs[key + "no-resident"][:3]):
            assert same(u, v), (key, "resident == no-resident")
    # windows == the step loop
    o0 = run_online(RB, 256, 24, y[:24], window=1)
    for u, v in zip(runs["online-resident"][:5], o0[:5]):
        assert same(u, v), "windowed == step by step"
    # exchange!: the state particles double after a rejuvenation whose acceptance ratio is below min_ar
    e1 = run_online(RB, 256, 24, y[:24], min_ar=2.0)
    e2 = run_online(RB, 256, 24, y[:24], min_ar=2.0)
    assert e1[5] > 256 and e1[5] % 256 == 0 and "particles added" in e1[7], (e1[5], e1[7])
    assert e1[3].shape == (4, 24, e1[5]) and np.all(np.isfinite(e1[1]))
    for u, v in zip(e1[:5], e2[:5]):
        assert same(u, v), "exchange twice"
    # posterior of gamma against bootstrap UCSV
    # (threshold 0.5 M here: on this series the ladder then reaches xi = 1 in one stage without a resample-move, and the posterior
    #  is the prior cloud weighted by exp(logZ) - the comparison tests the likelihood estimates and nothing else)
    g = run_dt(RB, 512, 128, y, seed=1, chain=5, ess_threshold=0.5)
    ref = run_dt(UC, 2048, 512, y, seed=2, chain=5, ess_threshold=0.5)

    def post(o):
        w = smc._lib.host_reweight(o[2])[1]
        m = w @ o[0]
        return m, np.sqrt(w @ (o[0] - m) ** 2), 1.0 / np.sum(w * w)
    (mg, sg, eg), (mr, sr, er) = post(g), post(ref)
    zs = (mg - mr) / (sg / math.sqrt(eg))
    print("posterior mean of gamma: marginal %s (sd %s, ESS %.1f), bootstrap UCSV %s (sd %s, ESS %.1f); z = %s" % (mg, sg, eg, mr, sr, er, zs))
    assert np.all(np.abs(zs) <= 4), zs


@pytest.mark.parametrize("n,flags", [(512, 0), (512, NO_RESIDENT), (3000, 0)], ids=["resident", "no-resident", "multi-segment"])
def test_pmmh_skips_proposals_outside_the_support(L, n, flags):
    """smc_pmmh_rejuvenate on the family, theta = (gamma_eps, gamma_eta), one chain position.
    (a) a prior whose support no proposal can reach (width 2e-12 around the common theta): no filter runs, nothing is accepted, and
        theta, logZ and the four-row state, weights and raw weights of every main filter are what they were, bit for bit;
    (b) Uniform(0.02, 0.6) with a wide random walk: some proposals leave the support and their filters are not run
        (0 < filters run < M); a particle that did not move keeps theta, logZ and its state bit for bit, a particle that moved has
        a finite logZ, a proposal inside the support and the proposal filter's state (P > 0)."""
    import sequential_monte_carlo_amd as smc
    M = 48
    y = series(15, seed=11)
    raw_from, raw_const = [0, 1, -1, -1, -1], [0.0, 0.0, 3.0, 0.0, 0.0]
    tmap = smc.ThetaMap(RB, raw_from, raw_const)
    r = np.random.default_rng(3)
    for case in ("a", "b"):
        theta = np.full((M, 2), 0.3) if case == "a" else r.uniform(0.03, 0.59, size=(M, 2))
        lo, hi = (0.3 - 1e-12, 0.3 + 1e-12) if case == "a" else (0.02, 0.6)
        spec = smc.product_distribution([smc.Uniform(lo, hi), smc.Uniform(lo, hi)]).spec()
        main = L.Handle(RB, M, n, seed=9, flags=flags)
        main.set_params(tmap.rows(theta))
        logZ = main.log_likelihood(y)
        before = snapshot_no_anc(main)
        prop = L.Handle(RB, M, n, seed=10, flags=flags)
        prop.set_streams(np.arange(M, dtype=np.uint32))
        prop.pmmh_configure(spec[0], spec[1], raw_from, raw_const)
        th2, lz2, acc, nrun = prop.pmmh_rejuvenate(main, y, 1.0, 0.25 * np.eye(2), [1.0], [77], 78, theta, logZ)
        after = snapshot_no_anc(main)
        if case == "a":
            assert nrun == 0 and not acc.any()
        else:
            assert 0 < nrun < M, nrun
            assert acc.any() and not acc.all()
        for m in range(M):
            if not acc[m]:
                assert same(th2[m], theta[m]) and same([lz2[m]], [logZ[m]]), (case, m)
                for u, v in zip(before, after):
                    assert np.array_equal(u[..., m, :] if u.ndim == 3 else u[m], v[..., m, :] if v.ndim == 3 else v[m]), (case, m)
            else:
                assert np.isfinite(lz2[m]) and np.all((th2[m] >= lo) & (th2[m] <= hi)) and not same(th2[m], theta[m]), (case, m)
                assert np.all(after[0][3, m] > 0) and not same(after[0][:, m], before[0][:, m]), (case, m)
        main.close()
        prop.close()


def snapshot_no_anc(h):
    """(x [4][M][n], w [M][n], C, kb, S, S2hi, S2lo) as unsigned words where they are doubles"""
    x, w, _ = h.state(want_anc=False)
    return (bits(x), bits(w)) + tuple(bits(a) if a.dtype == np.float64 else a for a in h.weights_raw())


# ---- 8. handle state -----------------------------------------------------------------------------------------------------
def test_recycled_bundles_and_set_params(L):
    y = series(10)
    r1, r2 = raws_for(3), raws_for(3) * np.array([1.3, 0.8, 1.0, 1.0, 1.0]) + np.array([0, 0, 0.5, -0.3, 0.2])

    def fresh(model, raw, n=1024, prop=False):
        h = L.Handle(model, 3, n, seed=31)
        h.set_params(raw)
        if prop:
            h.set_proposal(TG.OPTIMAL)
        z = h.log_likelihood(y)
        x, w, _ = h.state(want_anc=False)
        h.close()
        return z, x, w
    first = fresh(RB, r1)
    fresh(UC, r1, n=1365, prop=True)        # a guided three-row handle whose slab fits the next request: its bundle is recycled
    again = fresh(RB, r1)
    for u, v in zip(first, again):
        assert same(u, v)
    u1 = fresh(UC, r1)
    fresh(RB, r1)
    u2 = fresh(UC, r1)                      # a three-row handle out of a four-row handle's bundle
    for u, v in zip(u1, u2):
        assert same(u, v)
    h = L.Handle(RB, 3, 1024, seed=31)
    h.set_params(r1)
    z1 = h.log_likelihood(y)
    h.set_params(r2)
    z2 = h.log_likelihood(y)
    x2, w2, _ = h.state(want_anc=False)
    h.init(y[0])                            # and through the step API after a whole-series call
    for t in range(1, 10):
        h.step(y[t])
    z3, _ = h.logZ()
    h.close()
    ref = fresh(RB, r2)
    assert same(z1, first[0]) and same(z2, ref[0]) and same(x2, ref[1]) and same(w2, ref[2]) and same(z3, ref[0])
