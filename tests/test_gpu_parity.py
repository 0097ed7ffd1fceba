"""GPU parity tests (pytest -m gpu): the HIP path, called through the C ABI, against the CPU
oracle on the same seeded inputs -- BIT-EXACT (logZ, per-step logmu/ess, states, weights,
ancestor indices and the raw fixed-point weight state) -- against the committed golden vectors,
and at BASELINE.json's full sizes through size-independent properties.
Tolerance statement: every comparison with the oracle below is exact equality of the IEEE bit
patterns (tolerance 0 ulp, tighter than north_star's "states within 1 ulp")."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
SV = [-1.0, 0.95, 0.25]
UC = [0.2, 0.2, 3.0, 0.0, 0.0]
RAW = {1: LG, 2: SV, 3: UC}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def test_device_math_is_bit_exact(L, ob):
    rng = np.random.default_rng(0)
    n = 1 << 18
    x = np.concatenate([rng.uniform(-708, 5, n), rng.uniform(-2, 2, n), [0.0, -745.0, 709.5, np.inf, -np.inf, np.nan]])
    g = L.device_math(0, x)
    host = np.array([L.lib().smc_host_exp(float(v)) for v in x[:5000]])
    assert same(g[:5000], host) and same(g[-6:-1], ob.exp(x[-6:-1])) and np.isnan(g[-1])
    x = np.concatenate([rng.uniform(0, 1, n), np.exp(rng.uniform(-740, 700, n)), [1.0, 0.0, 5e-324, np.inf]])
    g = L.device_math(1, x)
    assert same(g[:5000], ob.log(x[:5000])) and same(g[-4:], ob.log(x[-4:]))
    x = np.exp(rng.uniform(-300, 300, n))
    assert same(L.device_math(2, x), np.sqrt(x))                      # IEEE sqrt
    a = rng.normal(size=n) * np.exp(rng.uniform(-100, 100, n))
    b = rng.normal(size=n) * np.exp(rng.uniform(-100, 100, n))
    assert same(L.device_math(5, a, b), a / b)                        # IEEE divide
    wa = rng.integers(0, 2**64, 4000, dtype=np.uint64)
    wb = rng.integers(0, 2**64, 4000, dtype=np.uint64)
    # the corners of Box-Muller: u1 = 1 (radius -0.0: the square root's refinement alone would give NaN), u1 = 2^-53, the
    # carry of (lo >> 11) + 1 into the high word, mantissas next to sqrt 2, and u2 on / next to every octant boundary
    edge_a = [2**64 - 1, 0, 2**32 - 1, (2**32 - 1) << 11, 0x6A09E667F3BCD << 11 | 0x7FF, (0x6A09E667F3BCD + 1) << 11, 1 << 63, (1 << 63) - 1]
    edge_b = [k << 61 for k in range(8)] + [(k << 61) - (1 << 11) for k in range(1, 8)] + [(k << 61) + (1 << 11) for k in range(8)] + [2**64 - 1]
    wa[:len(edge_a)] = np.array(edge_a, dtype=np.uint64)
    wb[100:100 + len(edge_b)] = np.array(edge_b, dtype=np.uint64)
    wa[100:100 + len(edge_b)] = np.uint64(2**64 - 1) >> np.uint64(3)
    wb[:len(edge_a)] = np.array([k << 61 for k in range(8)], dtype=np.uint64)
    z0 = L.device_math(3, wa.view(np.float64), wb.view(np.float64))
    z1 = L.device_math(4, wa.view(np.float64), wb.view(np.float64))
    ref = np.array([ob.box_muller([int(p) & 0xFFFFFFFF, int(p) >> 32, int(q) & 0xFFFFFFFF, int(q) >> 32])
                    for p, q in zip(wa, wb)])
    assert same(z0, ref[:, 0]) and same(z1, ref[:, 1])


def run_and_compare(L, ob, model, n, T, seg, ntheta=1, flags=0, seed=7, raws=None):
    raws = np.tile(RAW[model], (ntheta, 1)) if raws is None else np.asarray(raws, dtype=float)
    _, y = ob.simulate(model, RAW[model], T, 1998)
    h = L.Handle(model, ntheta, n, seg=seg, seed=seed, flags=flags | L.FLAG_ANCESTORS)
    h.set_params(raws)
    logZ, lm, es = h.log_likelihood(y, trace=True)
    x, w, a = h.state()
    C, m, S, hi, lo = h.weights_raw()
    for th in range(ntheta):
        f = ob.Filter(model, raws[th], n, seg=seg, seed=seed, stream=th)
        z, olm, oes = f.log_likelihood(y, trace=True)
        ox, ow, oa, _ = f.state()
        oC, om, oS, ohi, olo = f.weights_raw()
        assert bits([logZ[th]])[0] == bits([z])[0]
        assert same(lm[:, th], olm) and same(es[:, th], oes)
        assert same(x[:, th], ox) and same(w[th], ow) and np.array_equal(a[th], oa)
        assert np.array_equal(C[th], oC) and same(m[th], om) and np.array_equal(S[th], oS)
        assert np.array_equal(hi[th], ohi) and np.array_equal(lo[th], olo)
    res = h.resident
    h.close()
    return res


@pytest.mark.parametrize("model", [1, 2, 3])
@pytest.mark.parametrize("resident", [False, True])
def test_single_segment_filters_bit_exact(L, ob, model, resident):
    flags = 0 if resident else L.FLAG_NO_RESIDENT
    for n, seg, T in ((1024, 0, 40), (1000, 0, 15), (300, 512, 15), (2048, 0, 15), (4096, 0, 8), (1, 0, 5), (3, 0, 5)):
        assert run_and_compare(L, ob, model, n, T, seg, flags=flags) == resident
    if model != 3:
        assert run_and_compare(L, ob, model, 8192, 6, 0, flags=flags) == resident


@pytest.mark.parametrize("model", [1, 2, 3])
def test_multi_segment_filters_bit_exact(L, ob, model):
    for n, seg, T in ((5000, 256, 12), (10000, 1024, 8), (65536, 2048, 6), (20000, 4096, 6), (30000, 8192, 5),
                      (9000, 512, 8), (1025, 1024, 6)):
        assert run_and_compare(L, ob, model, n, T, seg) is False


def test_batched_filters_with_distinct_parameters(L, ob):
    """A8: n_theta independent filters with per-theta parameters (smc.model(theta[m]))."""
    rng = np.random.default_rng(3)
    nth = 9
    raws = np.tile(LG, (nth, 1))
    raws[:, 0] = rng.uniform(-0.9, 0.9, nth)
    raws[:, 2] = rng.lognormal(size=nth)
    raws[:, 3] = rng.lognormal(size=nth)
    for flags in (0, L.FLAG_NO_RESIDENT):
        run_and_compare(L, ob, 1, 1024, 25, 0, ntheta=nth, flags=flags, raws=raws)
    run_and_compare(L, ob, 1, 3000, 10, 1024, ntheta=nth, raws=raws)
    raws = np.tile(UC, (4, 1))
    raws[:, 0] = raws[:, 1] = [0.1, 0.2, 0.3, 0.4]
    run_and_compare(L, ob, 3, 1024, 20, 0, ntheta=4, raws=raws)


def test_golden_vectors(L):
    meta = json.load(open(os.path.join(GOLDEN, "filter_vectors.json")))
    g = np.load(os.path.join(GOLDEN, "filter_vectors.npz"))
    for name, m in meta.items():
        for flags in (L.FLAG_ANCESTORS, L.FLAG_ANCESTORS | L.FLAG_NO_RESIDENT):
            h = L.Handle(m["model"], 1, m["n"], seg=m["seg"], seed=m["seed"], flags=flags)
            h.set_params(m["raw"])
            h.set_streams([m["stream"]])
            logZ, lm, es = h.log_likelihood(g[name + "/y"], trace=True)
            x, w, a = h.state()
            C, mm, S, hi, lo = h.weights_raw()
            assert float(logZ[0]).hex() == m["logZ"], name
            assert same(lm[:, 0], g[name + "/logmu"]) and same(es[:, 0], g[name + "/ess"]), name
            assert same(x[:, 0], g[name + "/x"]) and same(w[0], g[name + "/w"]), name
            assert np.array_equal(a[0], g[name + "/anc"]) and np.array_equal(C[0], g[name + "/C"]), name
            assert np.array_equal(S[0], g[name + "/S"]) and np.array_equal(hi[0], g[name + "/S2hi"]), name
            h.close()
    lmu, w, ess = L.normalize(g["normalize/logw"])
    assert same(w, g["normalize/w"]) and same([lmu, ess], g["normalize/out"])
    assert np.array_equal(L.resample(w, 2000, seed=17, stream=2, t=9), g["resample/a"])


def test_step_api_matches_whole_series(L, ob):
    """bootstrap_filter / bootstrap_filter! one call per observation (README.md:33-61) gives the
    same bits as log_likelihood, and the same as the oracle's step loop."""
    _, y = ob.simulate(1, LG, 30, 1998)
    for n, seg in ((1024, 0), (5000, 1024)):
        h = L.Handle(1, 2, n, seg=seg, seed=5, flags=L.FLAG_ANCESTORS)
        h.set_params(np.tile(LG, (2, 1)))
        fs = [ob.Filter(1, LG, n, seg=seg, seed=5, stream=th) for th in range(2)]
        lm = h.init(y[0])
        assert same(lm, [f.bootstrap_filter(y[0]) for f in fs])
        acc = lm.copy()
        for t in range(1, 30):
            lm, ess = h.step(y[t])
            ref = [f.step(y[t]) for f in fs]
            assert same(lm, [r[0] for r in ref]) and same(ess, [r[1] for r in ref])
            acc += lm
            if t in (1, 7, 29):
                x, w, a = h.state()
                for th in range(2):
                    ox, ow, oa, _ = fs[th].state()
                    assert same(x[:, th], ox) and same(w[th], ow) and np.array_equal(a[th], oa)
        z, e = h.logZ()
        assert same(z, acc)
        h2 = L.Handle(1, 2, n, seg=seg, seed=5)
        h2.set_params(np.tile(LG, (2, 1)))
        assert same(h2.log_likelihood(y), z)
        h.close(); h2.close()


def test_standalone_normalize_resample(L, ob):
    rng = np.random.default_rng(11)
    for n in (1, 2, 63, 512, 4096, 16384, 16385, 65536, 65537, 100000, 1 << 20, (1 << 21) + 5):      # > 16384 (normalize), > 65536 (resample): the grid-wide kernels
        logw = rng.normal(size=n) * 5 - 100
        if n > 10:
            logw[3] = -np.inf
            logw[7] = np.nan
        lmu, w, ess = L.normalize(logw)
        olmu, ow, oess = ob.normalize(logw)
        assert same(w, ow) and same([lmu, ess], [olmu, oess])
        a = L.resample(ow, 3 * n + 1, seed=4, stream=2, t=n % 100)
        assert np.array_equal(a, ob.resample(ow, 3 * n + 1, seed=4, stream=2, t=n % 100))
    dead = np.full(20000, -np.inf)                                 # no live entry at all, long vector
    lmu, w, ess = L.normalize(dead)
    olmu, ow, oess = ob.normalize(dead)
    assert same(w, ow) and same([lmu, ess], [olmu, oess])
    with pytest.raises(L.SmcError):
        L.resample(np.zeros(8))


def test_permute_is_value_copy(L, ob):
    """resample!(smc) (smc_samplers.jl:74-84) with value-copy semantics; slots keep their streams."""
    _, y = ob.simulate(1, LG, 12, 1998)
    nth, n = 6, 1024
    h = L.Handle(1, nth, n, seed=9, flags=L.FLAG_ANCESTORS)
    h.set_params(np.tile(LG, (nth, 1)))
    h.init(y[0])
    for t in range(1, 6):
        h.step(y[t])
    x0, w0, _ = h.state()
    z0, e0 = h.logZ()
    a = np.array([3, 3, 0, 5, 1, 1], dtype=np.int32)
    h.permute(a)
    x1, w1, _ = h.state()
    z1, e1 = h.logZ()
    assert same(x1, x0[:, a]) and same(w1, w0[a]) and same(z1, z0[a]) and same(e1, e0[a])
    lm, _ = h.step(y[6])
    assert lm[0] != lm[1]          # duplicated theta-particles evolve with different noise
    # oracle: a filter that takes over slot 3's state but draws with stream 0 -- emulate by comparing
    # slot 3 (unchanged: a[3]=5? no) -> only check the untouched law: weights still normalised
    _, w2, _ = h.state()
    assert np.allclose(w2.sum(axis=1), 1.0, atol=1e-12)
    h.close()


def test_errors(L):
    h = L.Handle(1, 1, 64)
    with pytest.raises(L.SmcError):
        h.init(0.0)                 # params not set
    h.set_params(LG)
    with pytest.raises(L.SmcError):
        h.step(0.0)                 # not initialised
    with pytest.raises(L.SmcError):
        h.state(want_anc=True)      # also not initialised
    h.init(0.3)
    with pytest.raises(L.SmcError):
        h.state(want_anc=True)      # created without FLAG_ANCESTORS
    h.close()
    with pytest.raises(L.SmcError):
        L.Handle(1, 1, 64, device=99)


def test_collapse_and_recovery(L, ob):
    h = L.Handle(2, 1, 64, seed=4, flags=L.FLAG_ANCESTORS)
    h.set_params(SV)
    f = ob.Filter(2, SV, 64, seed=4)
    assert same(h.init(0.1), [f.bootstrap_filter(0.1)])
    lm, ess = h.step(1e200)
    assert lm[0] == -np.inf and ess[0] == 0.0 and f.step(1e200) == (-np.inf, 0.0)
    lm, ess = h.step(0.1)
    olm, oess = f.step(0.1)
    assert same(lm, [olm]) and same(ess, [oess]) and np.array_equal(h.state()[2][0], np.arange(64))
    h.close()


# ---- BASELINE.json full sizes: size-independent properties -------------------------------------
def test_full_size_c2_properties(L):
    """C2: LG, Nx = 2^20, T = 1000 on one GPU.  logZ against the exact Kalman likelihood of the
    reference (kalman_filter.jl:29-70; fixture), weights normalised, ancestors in range, ESS in
    [1, Nx], determinism, seed sensitivity."""
    k = json.load(open(os.path.join(GOLDEN, "kalman_lg.json")))
    n, T = 1 << 20, 1000
    _, y = L.simulate(1, LG, T, 1998)
    assert [float(v).hex() for v in y[:8]] == k["cases"]["T1000"]["y_head"]
    h = L.Handle(1, 1, n, seed=1, flags=L.FLAG_ANCESTORS)
    h.set_params(LG)
    logZ, lm, es = h.log_likelihood(y, trace=True)
    # sd of logZ at Nx=2^20 is ~0.03 (Var ~ c T / Nx); 0.25 is > 8 sd
    assert abs(logZ[0] - k["cases"]["T1000"]["logZ_kf"]) < 0.25
    assert logZ[0] == pytest.approx(lm[:, 0].sum(), rel=1e-13)
    assert np.all(es >= 1.0) and np.all(es <= n) and es.mean() > 0.3 * n
    x, w, a = h.state()
    assert abs(w.sum() - 1.0) < 1e-10 and w.min() >= 0
    assert a.min() >= 0 and a.max() < n and len(np.unique(a)) > 0.4 * n
    assert np.any(np.diff(a[0].astype(np.int64)) < 0)                   # iid inside a block: not globally sorted
    # the resampling law at full size: one more step from these weights; children counts per ancestor segment
    # against N p (chi-square, 511 dof), and the children ordered by block of the weight CDF
    from scipy.stats import chi2
    w_prev = w[0].copy()
    h.step(0.3)
    a2 = h.state(want_w=False)[2][0].astype(np.int64)
    seg = h.seg
    cnt = np.bincount(a2 // seg, minlength=n // seg).astype(np.float64)
    p = w_prev.reshape(-1, seg).sum(axis=1)
    stat = float(np.sum((cnt - n * p) ** 2 / (n * p)))
    assert 0.0005 < chi2.cdf(stat, n // seg - 1) < 0.9995, stat
    blocks = a2.reshape(-1, seg)
    assert np.all(blocks[:-1].max(axis=1) <= blocks[1:].min(axis=1))
    # filtered mean against the Kalman filtered mean
    from_pf = float(np.sum(w[0] * x[0, 0]))
    A, B, Q, R = LG[:4]
    xm, S = LG[4], LG[5]
    for t, yt in enumerate(y):
        if t > 0:
            xm, S = A * xm, A * A * S + Q
        s = B * B * S + R
        xm, S = xm + S * B / s * (yt - B * xm), S - (S * B) ** 2 / s
    assert abs(from_pf - xm) < 6 * np.sqrt(S / n) + 1e-3
    assert same(h.log_likelihood(y), logZ)                              # deterministic replay (also after the extra step)
    h.reseed(2)
    assert h.log_likelihood(y)[0] != logZ[0]
    h.close()


def test_full_size_c3_sv_properties(L):
    """C3 at its real size: stochastic volatility, Nx = 2^20, T = 5000 (BASELINE configs[2]).  The series
    crosses the 1024-step break-point window of log_likelihood four times and the 64-step window of the
    step API 78 times; both walks must give the same bits (particles.jl:141-144: logZ = sum of logmu_t)."""
    n, T = 1 << 20, 5000
    _, y = L.simulate(2, SV, T, 1998)
    h = L.Handle(2, 1, n, seed=1, flags=L.FLAG_ANCESTORS)
    h.set_params(SV)
    logZ, lm, es = h.log_likelihood(y, trace=True)
    assert np.isfinite(logZ[0]) and np.all(np.isfinite(lm)) and np.all(es >= 1.0) and np.all(es <= n)
    assert es.mean() > 0.3 * n and logZ[0] == pytest.approx(lm[:, 0].sum(), rel=1e-12)
    x, w, a = h.state()
    assert abs(w.sum() - 1.0) < 1e-10 and a.min() >= 0 and a.max() < n
    assert same(h.log_likelihood(y), logZ)                               # deterministic replay
    # the step API over the same series (a refill every 64 steps instead of every 1024): same bits
    lm0 = h.init(y[0])
    acc, ok = lm0.copy(), same(lm0, lm[0])
    for t in range(1, T):
        l1, e1 = h.step(y[t])
        ok &= l1[0] == lm[t, 0] and e1[0] == es[t, 0]
        acc += l1
    assert ok and same(acc, logZ) and same(h.logZ()[0], logZ)
    x2, w2, a2 = h.state()
    assert same(x2, x) and same(w2, w) and np.array_equal(a2, a)
    h2 = L.Handle(2, 1, n // 2, seed=5)
    h2.set_params(SV)
    z2 = h2.log_likelihood(y)[0]
    # sd(logZ) ~ sqrt(c T / Nx): a few tenths at T = 5000, Nx = 2^19..2^20
    assert abs(z2 - logZ[0]) < 2.5                                      # Nx-doubling convergence
    h.close(); h2.close()


def test_break_point_window_refill_against_oracle(L, ob):
    """The break points of multi-segment filters are prepared by k_breaks for a WINDOW of steps (<= 1024 per
    launch for log_likelihood, 64 for the step API; smc_capi.hip ensure_breaks) and re-computed with a new
    origin when the series runs past it.  T = 1100 crosses the first boundary; bit-exact against the oracle
    (which knows no windows) on every per-step output and the final state."""
    n, seg, T, nth = 5000, 1024, 1100, 2
    _, y = ob.simulate(1, LG, T, 1998)
    h = L.Handle(1, nth, n, seg=seg, seed=31, flags=L.FLAG_ANCESTORS)
    h.set_params(np.tile(LG, (nth, 1)))
    logZ, lm, es = h.log_likelihood(y, trace=True)
    x, w, a = h.state()
    for th in range(nth):
        f = ob.Filter(1, LG, n, seg=seg, seed=31, stream=th)
        z, olm, oes = f.log_likelihood(y, trace=True)
        ox, ow, oa, _ = f.state()
        assert bits([logZ[th]])[0] == bits([z])[0] and same(lm[:, th], olm) and same(es[:, th], oes)
        assert same(x[:, th], ox) and same(w[th], ow) and np.array_equal(a[th], oa)
    h.close()


def test_step_api_window_refill_reseed_and_streams_mid_window(L, ob):
    """smc_step on multi-segment filters for 150 steps (break-point windows [1,65), [65,129), [129,..)), with
    smc_reseed at t = 40 and smc_set_streams at t = 100 - both in the middle of a window, both invalidate the
    cached break points - against the oracle step by step."""
    n, seg, nth, T = 3000, 1024, 2, 150
    _, y = ob.simulate(2, SV, T, 5)
    h = L.Handle(2, nth, n, seg=seg, seed=17, flags=L.FLAG_ANCESTORS)
    h.set_params(np.tile(SV, (nth, 1)))
    fs = [ob.Filter(2, SV, n, seg=seg, seed=17, stream=th) for th in range(nth)]
    assert same(h.init(y[0]), [f.bootstrap_filter(y[0]) for f in fs])
    streams = [0, 1]
    for t in range(1, T):
        if t == 40:
            h.reseed(99)
            for f, st in zip(fs, streams):
                f.set_rng(99, st)
        if t == 100:
            streams = [7, 11]
            h.set_streams(streams)
            for f, st in zip(fs, streams):
                f.set_rng(99, st)
        lm, ess = h.step(y[t])
        ref = [f.step(y[t]) for f in fs]
        assert same(lm, [r[0] for r in ref]) and same(ess, [r[1] for r in ref]), t
        if t in (39, 40, 64, 65, 100, 128, 129, T - 1):
            x, w, a = h.state()
            for th in range(nth):
                ox, ow, oa, _ = fs[th].state()
                assert same(x[:, th], ox) and same(w[th], ow) and np.array_equal(a[th], oa), (t, th)
    h.close()


def test_break_point_capacity_below_series_length(L):
    """4096 segments: one step of break points is 32 KiB, so the 32 MiB buffer holds 1023 steps and a
    T = 1040 series re-fills it once; log_likelihood (window 1023) and the step API (window 64) agree bit
    for bit, i.e. the result does not depend on where the windows fall.  (The oracle would need 10^9
    particle-steps here: property test.)"""
    n, seg, T = 4096 * 256, 256, 1040
    _, y = L.simulate(1, LG, T, 1998)
    h = L.Handle(1, 1, n, seg=seg, seed=3)
    h.set_params(LG)
    assert h.nseg == 4096
    logZ, lm, es = h.log_likelihood(y, trace=True)
    l0 = h.init(y[0])
    ok = l0[0] == lm[0, 0]
    for t in range(1, T):
        l1, e1 = h.step(y[t])
        ok &= l1[0] == lm[t, 0] and e1[0] == es[t, 0]
    assert ok and same(h.logZ()[0], logZ)
    h.close()


def test_full_size_c4_batched_properties(L):
    """C4 shape: N_theta = 512 x Nx = 1024, T = 200; resident and step paths agree bit for bit,
    and the logZ of identical-parameter filters scatter around Kalman like the oracle does."""
    k = json.load(open(os.path.join(GOLDEN, "kalman_lg.json")))
    nth, n, T = 512, 1024, 200
    _, y = L.simulate(1, LG, T, 1998)
    h = L.Handle(1, nth, n, seed=1)
    h.set_params(np.tile(LG, (nth, 1)))
    assert h.resident
    z = h.log_likelihood(y)
    h2 = L.Handle(1, nth, n, seed=1, flags=L.FLAG_NO_RESIDENT)
    h2.set_params(np.tile(LG, (nth, 1)))
    assert same(h2.log_likelihood(y), z)
    kf = k["cases"]["T200"]["logZ_kf"]
    se = z.std(ddof=1) / np.sqrt(nth)
    assert abs(z.mean() + 0.5 * z.var(ddof=1) - kf) < 5 * se
    r = np.exp(z - kf)
    assert abs(r.mean() - 1) < 5 * r.std(ddof=1) / np.sqrt(nth)
    h.close(); h2.close()


def test_full_size_c5_ucsv_shape(L):
    """C5 per-GPU shard: UCSV, N_theta = 512 x Nx = 1024, T = 200."""
    nth, n, T = 512, 1024, 200
    _, y = L.simulate(3, UC, T, 1998)
    rng = np.random.default_rng(0)
    raws = np.tile(UC, (nth, 1))
    raws[:, 0] = raws[:, 1] = rng.uniform(0.05, 0.6, nth)
    h = L.Handle(3, nth, n, seed=1)
    h.set_params(raws)
    z, lm, es = h.log_likelihood(y, trace=True)
    assert np.all(np.isfinite(z)) and np.all(es >= 1) and np.all(es <= n)
    # the data were generated with gamma = 0.2: the likelihood surface must prefer it to the extremes
    near = z[np.abs(raws[:, 0] - 0.2) < 0.05].mean()
    assert near > z[raws[:, 0] > 0.5].mean() and near > z[raws[:, 0] < 0.08].mean()
    h.close()


def test_uneven_weights_far_segments(L, ob):
    """Very informative observations (tiny R) make the weights wildly uneven: most segments get a
    handful of children, a few get hundreds, so one workgroup's children span more segments than it
    stages in LDS and the global-memory fallback of the segment search runs.  Still bit-exact."""
    for R, n, seg in ((1e-4, 5000, 256), (1e-6, 20000, 256), (1e-3, 40000, 1024), (1e-5, 70000, 2048)):
        raw = [0.9, 1.0, 1.0, R, 0.0, 4.0]
        _, y = ob.simulate(1, [0.9, 1.0, 1.0, 0.5, 0.0, 4.0], 12, 7)
        h = L.Handle(1, 2, n, seg=seg, seed=13, flags=L.FLAG_ANCESTORS)
        h.set_params(np.tile(raw, (2, 1)))
        logZ, lm, es = h.log_likelihood(y, trace=True)
        x, w, a = h.state()
        assert es.min() < 0.02 * n                      # the weights really are degenerate
        for th in range(2):
            f = ob.Filter(1, raw, n, seg=seg, seed=13, stream=th)
            z, olm, oes = f.log_likelihood(y, trace=True)
            ox, ow, oa, _ = f.state()
            assert bits([logZ[th]])[0] == bits([z])[0] and same(lm[:, th], olm) and same(es[:, th], oes)
            assert same(x[:, th], ox) and same(w[th], ow) and np.array_equal(a[th], oa)
            # children come out sorted by BLOCK of the weight CDF (iid inside a block): no ancestor of
            # block w+1 precedes an ancestor of block w
            blocks = [a[th][k:k + seg] for k in range(0, n, seg)]
            assert all(blocks[k].max() <= blocks[k + 1].min() for k in range(len(blocks) - 1))
        h.close()


def test_many_segments_per_thread_bit_exact(L, ob):
    """More segments than threads in a workgroup (several table entries per thread in the segment-table
    and offsets prologues): 586 and 1172 segments of 256, and 700 segments of 2048; still bit-exact."""
    for model, raw, n, seg, T in ((1, LG, 150000, 256, 4), (2, SV, 300000, 256, 3), (1, LG, 700 * 2048 - 77, 2048, 3)):
        _, y = ob.simulate(model, raw, T, 3)
        h = L.Handle(model, 1, n, seg=seg, seed=5, flags=L.FLAG_ANCESTORS)
        h.set_params(raw)
        logZ, lm, es = h.log_likelihood(y, trace=True)
        x, w, a = h.state()
        f = ob.Filter(model, raw, n, seg=seg, seed=5)
        z, olm, oes = f.log_likelihood(y, trace=True)
        ox, ow, oa, _ = f.state()
        assert bits([logZ[0]])[0] == bits([z])[0] and same(lm[:, 0], olm) and same(es[:, 0], oes), (model, n, seg)
        assert same(x[:, 0], ox) and same(w[0], ow) and np.array_equal(a[0], oa), (model, n, seg)
        assert np.array_equal(h.quantiles([0.1, 0.5, 0.9]).view(np.uint64)[0], f.quantiles([0.1, 0.5, 0.9]).view(np.uint64))
        h.close()


def test_global_segment_table_paths(L, ob):
    """Filters with more segments than a workgroup has threads: up to twice as many, the window prologue holds two records per
    thread; beyond, the segment table comes from global memory (k_table builds it once per step, k_step<..., GTAB> reads its window
    and the total).  Both: without traces (the previous step emitted from the totals), with
    them, batches with distinct parameters, three state coordinates, ragged sizes, wildly uneven weights (targets outside the
    speculative window: the searches walk the GLOBAL table), the systematic resampler, the step API with a permutation in between -
    bit-exact against the oracle every way."""
    # (model, raw, n, seg, ntheta, flags)
    UC = RAW[3]
    # up to twice as many segments as threads: the window prologue with two records per thread (the first five cases); beyond: k_table
    cases = ((1, LG, 40000, 256, 2, 0), (3, UC, 33000, 256, 1, 0), (1, [0.9, 1.0, 1.0, 1e-6, 0.0, 4.0], 60000, 256, 1, 0),
             (1, LG, 300 * 512 - 5, 512, 1, L.FLAG_SYSTEMATIC), (2, SV, 700 * 1024, 1024, 1, 0),
             (1, LG, 70000, 256, 2, 0), (3, UC, 67000, 256, 1, 0), (1, [0.9, 1.0, 1.0, 1e-6, 0.0, 4.0], 90000, 256, 1, 0),
             (1, LG, 600 * 512 - 5, 512, 1, L.FLAG_SYSTEMATIC), (2, SV, 1030 * 1024, 1024, 1, 0))
    for model, raw, n, seg, nth, flags in cases:
        T = 6 if n < 500000 else 3
        _, y = ob.simulate(model, RAW[model], T, 11)
        raws = np.tile(raw, (nth, 1))
        if nth > 1:
            raws[1, 0] *= 0.8
        h = L.Handle(model, nth, n, seg=seg, seed=9, flags=flags | L.FLAG_ANCESTORS)
        assert h.nseg > (seg // 2 if seg <= 1024 else 512)        # more segments than threads
        h.set_params(raws)
        z0 = h.log_likelihood(y)                                      # no traces: emission from the totals
        x0, w0, a0 = h.state()
        z1, lm, es = h.log_likelihood(y, trace=True)                  # full emission at every step
        assert same(z0, z1)
        for th in range(nth):
            f = ob.Filter(model, raws[th], n, seg=seg, seed=9, stream=th, systematic=bool(flags & L.FLAG_SYSTEMATIC))
            z, olm, oes = f.log_likelihood(y, trace=True)
            ox, ow, oa, _ = f.state()
            assert bits([z0[th]])[0] == bits([z])[0] and same(lm[:, th], olm) and same(es[:, th], oes), (model, n, seg)
            assert same(x0[:, th], ox) and same(w0[th], ow) and np.array_equal(a0[th], oa), (model, n, seg)
        h.close()
    # the step API: init, steps, a permutation of the filter slots, more steps (two records per thread; k_table)
    for n, seg in ((50000, 256), (80000, 256)):
        _, y = ob.simulate(1, LG, 8, 4)
        h = L.Handle(1, 2, n, seg=seg, seed=21)
        h.set_params(np.tile(LG, (2, 1)))
        fs = [ob.Filter(1, LG, n, seg=seg, seed=21, stream=th) for th in range(2)]
        assert same(h.init(float(y[0])), [f.bootstrap_filter(float(y[0])) for f in fs])
        for t in range(1, 8):
            if t == 4:
                h.permute(np.array([1, 1], dtype=np.int32))     # slot 0 becomes a value copy of slot 1 (keeps its own stream)
                fs[0].copy_state_from(fs[1])
            lm, es = h.step(float(y[t]))
            ref = [f.step(float(y[t])) for f in fs]
            assert same(lm, [r[0] for r in ref]) and same(es, [r[1] for r in ref]), t
        x, w, _ = h.state(want_anc=False)
        for th in range(2):
            ox, ow, _, _ = fs[th].state()
            assert same(x[:, th], ox) and same(w[th], ow)
        h.close()


def test_large_filters_beyond_2_pow_20(L):
    """Nx = 2^22 (2048 segments of 2048: the global segment table) - properties that do not depend on the size: the Kalman pin,
    determinism, normalised weights, ancestors in range."""
    from oracle import kalman
    n, T = 1 << 22, 40
    _, y = L.simulate(1, LG, T, 1998)
    kf = kalman.log_likelihood(y, *LG[:4], x0=LG[4], sigma0=LG[5], predict_first=False)[2]
    h = L.Handle(1, 1, n, seed=3, flags=L.FLAG_ANCESTORS)
    assert h.seg == 2048 and h.nseg == 2048
    h.set_params(LG)
    z = h.log_likelihood(y)
    x, w, a = h.state()
    z2 = h.log_likelihood(y)
    assert bits(z)[0] == bits(z2)[0]
    assert abs(z[0] - kf) < 8 * np.sqrt(T / n) + 1e-3
    assert abs(w[0].sum() - 1) < 1e-9 and a[0].min() >= 0 and a[0].max() < n
    h.close()


# ---- opt-in systematic resampling (SMC_FLAG_SYSTEMATIC) ------------------------------------------
def test_systematic_targets_on_device_are_exact(L):
    rng = np.random.default_rng(11)
    cases = [((1 << 63) - 1, (1 << 31) - 1, 2**64 - 1, (1 << 31) - 1 - 8192, 8192), ((1 << 62) + 12345, 1 << 20, 987654321987654321, 4096, 4096),
             (5, 3, 2**63 + 11, 0, 3), (0, 1000, 77, 0, 1000)]
    for _ in range(40):
        n = int(rng.integers(1, 1 << 31)) if rng.random() < 0.7 else 1 << int(rng.integers(0, 31))
        D = int(rng.integers(0, 1 << 63)) >> int(rng.integers(0, 62))
        nk = int(min(n, rng.integers(1, 8193)))
        cases.append((D, n, int(rng.integers(0, 1 << 64, dtype=np.uint64)), int(rng.integers(0, n - nk + 1)), nk))
    for D, n, u, j0, nk in cases:
        v0 = (u * D) >> 64
        want = [((j0 + k) * D + v0) // n for k in range(nk)]
        assert [int(g) for g in L.sys_targets(D, n, u, j0, nk, device=0)] == want, (D, n, u, j0, nk)


def test_systematic_filters_bit_exact(L, ob):
    """SMC_FLAG_SYSTEMATIC == the oracle's systematic resampler, bit for bit: resident and step kernels,
    one and many segments, power-of-two and awkward Nx, all three models, degenerate weights."""
    cfgs = [(1, LG, 1024, 0, 0), (1, LG, 1024, 0, L.FLAG_NO_RESIDENT), (1, LG, 1000, 256, 0), (2, SV, 777, 256, 0),
            (3, UC, 3000, 1024, 0), (3, UC, 512, 0, 0), (1, LG, 5000, 2048, 0), (2, SV, 70001, 2048, 0), (1, LG, 65536, 1024, 0),
            (1, [0.9, 1.0, 1.0, 1e-5, 0.0, 4.0], 40000, 1024, 0)]
    for model, raw, n, seg, fl in cfgs:
        _, y = ob.simulate(model, raw if raw[3:4] != [1e-5] else [0.9, 1.0, 1.0, 0.5, 0.0, 4.0], 9, 7)
        h = L.Handle(model, 2, n, seg=seg, seed=23, flags=L.FLAG_ANCESTORS | L.FLAG_SYSTEMATIC | fl)
        h.set_params(np.tile(raw, (2, 1)))
        logZ, lm, es = h.log_likelihood(y, trace=True)
        x, w, a = h.state()
        for th in range(2):
            f = ob.Filter(model, raw, n, seg=seg, seed=23, stream=th, systematic=True)
            z, olm, oes = f.log_likelihood(y, trace=True)
            ox, ow, oa, _ = f.state()
            ctx = (model, n, seg, fl, th)
            assert bits([logZ[th]])[0] == bits([z])[0] and same(lm[:, th], olm) and same(es[:, th], oes), ctx
            assert same(x[:, th], ox) and same(w[th], ow) and np.array_equal(a[th], oa), ctx
            assert np.all(np.diff(a[th]) >= 0), ctx                       # children fully sorted by ancestor
        h.close()
    # the step API, and the defining property of systematic resampling: #children in {floor, ceil}(N w)
    n = 6000
    _, y = ob.simulate(1, LG, 5, 3)
    h = L.Handle(1, 1, n, seg=1024, seed=5, flags=L.FLAG_ANCESTORS | L.FLAG_SYSTEMATIC)
    h.set_params(LG)
    f = ob.Filter(1, LG, n, seg=1024, seed=5, systematic=True)
    assert same(h.init(y[0]), [f.bootstrap_filter(y[0])])
    for t in range(1, 5):
        _, w_before, _ = h.state(want_anc=False)
        lm, ess = h.step(y[t])
        olm, oess = f.step(y[t])
        assert same(lm, [olm]) and same(ess, [oess])
        cnt = np.bincount(h.state()[2][0], minlength=n)
        assert np.all(cnt >= np.floor(n * w_before[0] - 1e-6)) and np.all(cnt <= np.ceil(n * w_before[0] + 1e-6))
    h.close()


def test_systematic_is_unbiased_against_kalman(L):
    """The systematic kernels against the reference's exact Kalman likelihood (tests/golden/kalman_lg.json):
    E[exp(logZ - logZ_KF)] = 1, and no more variance than the multinomial kernels at the same size."""
    import json, os
    from conftest import GOLDEN
    kf = json.load(open(os.path.join(GOLDEN, "kalman_lg.json")))["cases"]["T100"]["logZ_kf"]
    _, y = L.simulate(1, LG, 100, 1998)
    K = 256
    out = {}
    for name, fl in (("sys", L.FLAG_SYSTEMATIC), ("mult", 0)):
        zs = []
        for seg, seed in ((0, 50), (256, 51)):       # resident single segment; four segments through k_step
            h = L.Handle(1, K, 1024, seg=seg, seed=seed, flags=fl)
            h.set_params(np.tile(LG, (K, 1)))
            zs.append(h.log_likelihood(y))
            h.close()
        out[name] = zs
    for z in out["sys"]:
        r = np.exp(z - kf)
        assert abs(r.mean() - 1.0) < 4.5 * r.std(ddof=1) / np.sqrt(K)
        assert abs(z.mean() + 0.5 * z.var(ddof=1) - kf) < 4.5 * z.std(ddof=1) / np.sqrt(K)
    assert np.concatenate(out["sys"]).var(ddof=1) < 1.2 * np.concatenate(out["mult"]).var(ddof=1)
    # full size (C2 shape, T shortened): against the exact likelihood, ancestors sorted, weights normalised
    from oracle import kalman
    n, T = 1 << 20, 200
    _, y2 = L.simulate(1, LG, T, 1998)
    h = L.Handle(1, 1, n, seed=9, flags=L.FLAG_SYSTEMATIC | L.FLAG_ANCESTORS)
    h.set_params(LG)
    z = h.log_likelihood(y2)[0]
    assert abs(z - kalman.log_likelihood(y2, *LG[:4], x0=LG[4], sigma0=LG[5], predict_first=False)[2]) < 0.05
    _, w, a = h.state()
    assert np.all(np.diff(a[0].astype(np.int64)) >= 0) and abs(w.sum() - 1.0) < 1e-10
    h.close()


def test_step_api_multi_segment_with_permute_and_copy(L, ob):
    """smc_step on multi-segment filters interleaved with smc_permute / smc_copy_from."""
    _, y = ob.simulate(1, LG, 10, 1998)
    n, seg, nth = 3000, 1024, 3
    h = L.Handle(1, nth, n, seg=seg, seed=21)
    g = L.Handle(1, nth, n, seg=seg, seed=22)
    for hh in (h, g):
        hh.set_params(np.tile(LG, (nth, 1)))
        hh.init(y[0])
        for t in range(1, 4):
            hh.step(y[t])
    xg, wg, _ = g.state(want_anc=False)
    zg, _ = g.logZ()
    h.copy_from(g, [1, 0, 1])
    x, w, _ = h.state(want_anc=False)
    z, _ = h.logZ()
    assert same(x[:, 0], xg[:, 0]) and same(x[:, 2], xg[:, 2]) and not same(x[:, 1], xg[:, 1])
    assert same(w[0], wg[0]) and z[0] == zg[0] and z[2] == zg[2]
    h.permute(np.array([2, 2, 1], dtype=np.int32))
    x2, w2, _ = h.state(want_anc=False)
    assert same(x2[:, 0], x[:, 2]) and same(x2[:, 1], x[:, 2]) and same(x2[:, 2], x[:, 1])
    lm, ess = h.step(y[4])
    assert np.all(np.isfinite(lm)) and lm[0] != lm[1]
    _, w3, _ = h.state(want_anc=False)
    assert np.allclose(w3.sum(axis=1), 1.0, atol=1e-12)
    h.close(); g.close()


def test_time_step_kernel_runs(L):
    _, y = L.simulate(1, LG, 40, 1998)
    h = L.Handle(1, 1, 1 << 16, seed=1)
    h.set_params(LG)
    avg, mn = h.time_step_kernel(y, nsample=8)
    assert 0 < mn <= avg < 5.0
    h.close()


def test_randomized_configurations(L, ob):
    """Fuzz: random model family / parameters / Nx / seg / n_theta / T / seed / streams, resident or
    not -- every one bit-exact against the oracle (logZ, traces, states, weights, ancestors)."""
    import os
    iters = int(os.environ.get("SMC_FUZZ_ITERS", "40"))           # more on demand (same seeds first)
    rng = np.random.default_rng(20260401)
    for it in range(iters):
        model = int(rng.integers(1, 4))
        seg = int(rng.choice([0, 256, 512, 1024, 2048]))
        n = int(rng.integers(1, 9000))
        if seg and rng.random() < 0.3:
            n = int(rng.integers(1, seg + 1))            # single segment on purpose
        nth = int(rng.integers(1, 4))
        T = int(rng.integers(1, 9))
        seed = int(rng.integers(1, 2**62))
        flags = L.FLAG_ANCESTORS | (L.FLAG_NO_RESIDENT if rng.random() < 0.5 else 0)
        systematic = it >= 40 and rng.random() < 0.35           # (iterations 0..39 keep their original draws)
        if it >= 40 and rng.random() < 0.15:
            n = int(rng.integers(9000, 90000))
        if systematic:
            flags |= L.FLAG_SYSTEMATIC
        if model == 1:
            raws = np.column_stack([rng.uniform(-1, 1, nth), rng.uniform(0.5, 2, nth), rng.lognormal(0, 1, nth),
                                    rng.lognormal(-1, 1.5, nth), rng.normal(0, 2, nth), rng.lognormal(0, 1, nth)])
            sim = [0.7, 1.0, 1.0, 0.5, 0.0, 1.0]
        elif model == 2:
            raws = np.column_stack([rng.normal(-1, 1, nth), rng.uniform(-0.98, 0.98, nth), rng.lognormal(-1, 0.5, nth)])
            sim = SV
        else:
            raws = np.column_stack([rng.uniform(0.02, 0.8, nth), rng.uniform(0.02, 0.8, nth), rng.normal(3, 2, nth),
                                    rng.uniform(-2, 2, nth), rng.uniform(-2, 2, nth)])
            sim = UC
        _, y = ob.simulate(model, sim, T, int(rng.integers(1, 1000)))
        streams = rng.integers(0, 2**32, nth, dtype=np.uint64).astype(np.uint32)
        h = L.Handle(model, nth, n, seg=seg, seed=seed, flags=flags)
        h.set_params(raws)
        h.set_streams(streams)
        logZ, lm, es = h.log_likelihood(y, trace=True)
        x, w, a = h.state()
        for th in range(nth):
            f = ob.Filter(model, raws[th], n, seg=seg, seed=seed, stream=int(streams[th]), systematic=systematic)
            z, olm, oes = f.log_likelihood(y, trace=True)
            ox, ow, oa, _ = f.state()
            ctx = (it, model, n, seg, nth, T, th, systematic)
            assert bits([logZ[th]])[0] == bits([z])[0], ctx
            assert same(lm[:, th], olm) and same(es[:, th], oes), ctx
            assert same(x[:, th], ox) and same(w[th], ow) and np.array_equal(a[th], oa), ctx
        # the same series without traces: no sums of squares are accumulated on the way and (logmu) of every step comes from
        # the totals of the window prologue (emit_from_totals) - the same logZ, bit for bit
        assert same(h.log_likelihood(y), logZ), (it, model, n, seg, nth, T, systematic)
        h.close()


def test_step_window_equals_single_steps(L, ob):
    """smc_step_window (k bootstrap_filter! steps in one LDS-resident launch, nothing kept) + smc_step_commit(j):
    (logmu, ess) of every step and the state after the kept prefix are those of j smc_step calls / of the oracle,
    for every model, one or two particle pairs per thread, multinomial and systematic resampling."""
    for model, n, seg, fl in ((1, 1024, 0, 0), (1, 1000, 0, 0), (2, 2048, 0, 0), (3, 1024, 0, 0), (3, 300, 512, 0),
                              (1, 1024, 0, L.FLAG_SYSTEMATIC), (3, 777, 0, L.FLAG_SYSTEMATIC), (1, 8192, 0, 0)):
        raw, nth, T = RAW[model], 3, 26
        _, y = ob.simulate(model, raw, T, 11)
        h = L.Handle(model, nth, n, seg=seg, seed=41, flags=fl | L.FLAG_ANCESTORS)
        assert h.can_window
        h.set_params(np.tile(raw, (nth, 1)))
        fs = [ob.Filter(model, raw, n, seg=seg, seed=41, stream=th, systematic=bool(fl & L.FLAG_SYSTEMATIC)) for th in range(nth)]
        acc = h.init(y[0]).copy()
        assert same(acc, [f.bootstrap_filter(y[0]) for f in fs])
        t = 1
        for k, j in ((5, 5), (8, 3), (4, 0), (1, 1), (9, 9), (6, 1)):
            x0, w0, _ = h.state(want_anc=False)
            lm, es = h.step_window(y[t:t + k])
            x1, w1, _ = h.state(want_anc=False)
            assert same(x1, x0) and same(w1, w0)                   # a window does not move the filters ...
            h.step_commit(j)                                       # ... until a prefix of it is kept
            for i in range(j):
                ref = [f.step(y[t + i]) for f in fs]
                assert same(lm[i], [r[0] for r in ref]) and same(es[i], [r[1] for r in ref]), (model, n, k, j, i)
                acc += lm[i]
            t += j
            x, w, a = h.state()
            for th in range(nth):
                ox, ow, oa, _ = fs[th].state()
                assert same(x[:, th], ox) and same(w[th], ow), (model, n, k, j, th)
                if j:
                    assert np.array_equal(a[th], oa)
            assert same(h.logZ()[0], acc)
        lm1, es1 = h.step(y[t])                                    # and the single-step API goes on from there
        ref = [f.step(y[t]) for f in fs]
        assert same(lm1, [r[0] for r in ref]) and same(es1, [r[1] for r in ref])
        h.close()
    h = L.Handle(1, 1, 5000, seg=1024, seed=1)
    h.set_params(LG)
    h.init(0.1)
    assert not h.can_window
    with pytest.raises(L.SmcError):
        h.step_window([0.1, 0.2])
    h.close()


def test_launch_geometry_knobs_do_not_change_results(L, ob):
    """SMC_NP (particle pairs per thread of k_init/k_step, read by smc_create) and SMC_RES_NP (of the LDS-resident
    kernels, read at launch) are tuning knobs: any admissible value gives the oracle's bits."""
    import os
    _, y = ob.simulate(1, LG, 12, 1998)
    try:
        for knob, vals, cfgs in (("SMC_NP", ("1", "2", "4"), ((5000, 1024, L.FLAG_NO_RESIDENT), (1024, 0, L.FLAG_NO_RESIDENT), (40000, 2048, 0))),
                                 ("SMC_RES_NP", ("1", "2", "4"), ((1024, 0, 0), (2048, 0, 0), (700, 1024, 0)))):
            for n, seg, fl in cfgs:
                f = ob.Filter(1, LG, n, seg=seg, seed=3)
                z, olm, oes = f.log_likelihood(y, trace=True)
                ox, ow, oa, _ = f.state()
                for v in vals:
                    os.environ[knob] = v
                    h = L.Handle(1, 1, n, seg=seg, seed=3, flags=fl | L.FLAG_ANCESTORS)
                    h.set_params(LG)
                    logZ, lm, es = h.log_likelihood(y, trace=True)
                    x, w, a = h.state()
                    assert bits([logZ[0]])[0] == bits([z])[0] and same(lm[:, 0], olm) and same(es[:, 0], oes), (knob, v, n, seg)
                    assert same(x[:, 0], ox) and same(w[0], ow) and np.array_equal(a[0], oa), (knob, v, n, seg)
                    h.close()
            os.environ.pop(knob, None)
    finally:
        os.environ.pop("SMC_NP", None)
        os.environ.pop("SMC_RES_NP", None)


def test_multi_segment_series_leaves_no_residue_on_the_handle(L, ob):
    """The default whole-series path of multi-segment filters (one k_step launch per step) on shapes with uneven weights that
    leave the staged window, a ragged last segment, several filters per handle and every model family.  A handle that has run
    log_likelihood(y) and then runs a second, shorter series gives the bits of a fresh handle that runs the shorter series alone
    (logZ, state, raw weights C): the cached break points, the flipped buffers and the segment records of the first call leave
    no residue.  Where the oracle is quick enough (n <= 20000), logZ, x and w of the whole series against the oracle as well."""
    cases = ((1, LG, 20000, 256, 2, 14), (1, LG, 300000, 1024, 1, 40), (2, SV, 70000, 512, 1, 25), (3, UC, 50000, 1024, 2, 20),
             (1, [0.9, 1.0, 1.0, 1e-5, 0.0, 4.0], 70000, 2048, 1, 12))
    for model, raw, n, seg, nth, T in cases:
        _, y = ob.simulate(model, raw if raw[3:4] != [1e-5] else [0.9, 1.0, 1.0, 0.5, 0.0, 4.0], T, 7)
        res = []
        for used in (True, False):
            h = L.Handle(model, nth, n, seg=seg, seed=13)
            h.set_params(np.tile(raw, (nth, 1)))
            if used:
                h.log_likelihood(y)
            z2 = h.log_likelihood(y[: T - 3])
            x, w, _ = h.state(want_anc=False)
            Craw = h.weights_raw()[0]
            res.append((z2, x, w, Craw))
            h.close()
        for a, b in zip(res[0], res[1]):
            assert np.array_equal(a.view(np.uint64) if a.dtype != np.uint64 else a, b.view(np.uint64) if b.dtype != np.uint64 else b), (model, n, seg)
        if n <= 20000:
            h = L.Handle(model, nth, n, seg=seg, seed=13)
            h.set_params(np.tile(raw, (nth, 1)))
            z = h.log_likelihood(y)
            x, w, _ = h.state(want_anc=False)
            for th in range(nth):
                f = ob.Filter(model, raw, n, seg=seg, seed=13, stream=th)
                oz = f.log_likelihood(y)
                ox, ow, _, _ = f.state()
                assert bits([z[th]])[0] == bits([oz])[0] and same(x[:, th], ox) and same(w[th], ow)
            h.close()


def test_sv_full_size_against_grid_filter(L):
    """C3's model at Nx = 2^20 against the deterministic grid filter (oracle/grid_filter.py; the known answer for the
    non-Gaussian model, as the Kalman likelihood is for C2): sd(logZ) at this size is ~0.01-0.02, 0.08 is > 4 sd."""
    from oracle import grid_filter
    T = 200
    _, y = L.simulate(2, SV, T, 1998)
    g = grid_filter.sv_log_likelihood(y, *SV, n_grid=3001)
    zs = []
    for seed in (1, 2):
        h = L.Handle(2, 1, 1 << 20, seed=seed)
        h.set_params(SV)
        zs.append(h.log_likelihood(y)[0])
        h.close()
    assert abs(zs[0] - g) < 0.08 and abs(zs[1] - g) < 0.08 and zs[0] != zs[1], (zs, g)
    # and 256 batched 1024-particle filters (the LDS-resident kernel): unbiased for the same number
    h = L.Handle(2, 256, 1024, seed=9)
    h.set_params(np.tile(SV, (256, 1)))
    z = h.log_likelihood(y[:60])
    g60 = grid_filter.sv_log_likelihood(y[:60], *SV, n_grid=3001)
    r = np.exp(z - g60)
    assert abs(r.mean() - 1.0) < 4.5 * r.std(ddof=1) / 16 and abs(z.mean() + 0.5 * z.var(ddof=1) - g60) < 4.5 * z.std(ddof=1) / 16
    h.close()
