"""Missing observations on the CPU (no GPU): the host twin of the whole step (smc_host_filter_steps) and the composed reference
built on it (tests/missing_reference.py).  (a) with a finite series the twin's ordinary step is the oracle's bootstrap filter and
the composed guided / marginal filters, bit for bit; (b) the missing step's arithmetic, exactly; (c) a gap adds +0.0 to logZ and
leaves ess = n; (d) the filter through gaps estimates the likelihood of the model WITH the gaps (a Kalman filter with skipped
updates), not of the model with the periods left out."""
import numpy as np
import pytest

import composed_reference as CR
import missing_reference as MR
import step_edge_inputs
from test_composed_host import TRACKS

LG = MR.README_LG
SV = [0.0, 0.95, 0.3]
UC = [0.2, 0.2, 3.0, 0.0, 0.0]
RAW = {1: LG, 2: SV, 3: UC, 4: UC}
POOR = [0.3, 0.2, 0.1, 2.0]
NAN = float("nan")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- (a) the twin's ordinary step -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,n,seg,systematic,T", [t for t in TRACKS if t[1] <= 5000])
@pytest.mark.parametrize("missing", [False, True])
def test_finite_series_is_the_oracle_filter(L, ob, model, n, seg, systematic, T, missing):
    """kind = 0 and a finite series: x, w, ancestors, the raw weights, logmu and ess of ob.Filter after every step (with the
    flag as without: no NaN, no difference)"""
    _, y = ob.simulate(model, RAW[model], T, 11)
    b = ob.Filter(model, RAW[model], n, seg=seg, seed=9, stream=2, systematic=systematic)
    f = MR.MissingFilter(L, ob, model, RAW[model], n, seg=seg, seed=9, stream=2, systematic=systematic, missing=missing)
    assert (f.seg, f.nseg) == (b.seg, b.nseg)
    for t in range(T):
        if t == 0:
            lm, ess = b.bootstrap_filter(y[0]), b.ess()
            got = f.init(y[0])
        else:
            lm, ess = b.step(y[t])
            got = f.step(y[t])
        assert same(got, [lm, ess]), t
        ref = b.state()[:3] + b.weights_raw()
        assert MR.first_mismatch(f.snapshot(), ref) is None, (t, MR.first_mismatch(f.snapshot(), ref))
        assert same(f.f.state()[3], b.state()[3]), (t, "logw")


@pytest.mark.parametrize("model,kind,par", [(1, CR.AFFINE, POOR), (1, CR.OPTIMAL, None), (3, CR.OPTIMAL, None), (4, CR.NONE, None)])
@pytest.mark.parametrize("systematic", [False, True])
def test_finite_series_is_the_composed_filter(L, ob, model, kind, par, systematic):
    """guided and marginal series: tests/composed_reference.py (its twins are pinned against extended precision)"""
    y = L.simulate(3 if model == 4 else model, RAW[model], 10, 1998)[1]
    raws = np.array([RAW[model], RAW[model]])
    raws[1, 0] *= 0.7
    pars = None if par is None else [par, par]
    c = CR.run_series(L, ob, model, raws, 1000, 256, 7, y, kind=kind, pars=pars, systematic=systematic)
    m = MR.run_series(L, ob, model, raws, 1000, 256, 7, y, kind=kind, pars=pars, systematic=systematic)
    assert same(m["lm"], c["lm"]) and same(m["es"], c["es"]) and same(m["logZ"], c["logZ"])
    assert MR.first_mismatch(m["snap"], c["snap"]) is None, MR.first_mismatch(m["snap"], c["snap"])


# ---- (b) the missing step's arithmetic -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,kind", [(1, CR.NONE), (2, CR.NONE), (3, CR.NONE), (1, CR.AFFINE), (1, CR.OPTIMAL), (3, CR.OPTIMAL)])
@pytest.mark.parametrize("first", [False, True])
def test_missing_step_is_the_bootstrap_move(L, model, kind, first):
    """x of the missing step = x of the bootstrap twin's ordinary step on the same (xp, z) with any finite y, at t = 0 too, for
    bootstrap and guided handles alike; logw = +0.0 everywhere (sign bit clear)"""
    raw, par, xp, z, _ = step_edge_inputs.guided(3 if model == 3 else 1, kind if kind else CR.OPTIMAL)
    raw, par = (SV if model == 2 else raw), (par if kind == CR.AFFINE else None)
    xm, lwm = L.host_filter_steps(model, raw, kind, par, xp, z, NAN, first=first, missing=True)
    for y in (0.7, -3e4):
        xo, lwo = L.host_filter_steps(model, raw, CR.NONE, None, xp, z, y, first=first)
        assert same(xm, xo), y
        assert not np.any(bits(lwo) == 0)                      # (the ordinary step does weigh)
    assert np.all(bits(lwm) == 0)
    # without the switch a NaN is a NaN: the step's weights die
    _, lwn = L.host_filter_steps(model, raw, kind, par, xp, z, NAN, first=first, missing=False)
    assert np.all(np.isnan(lwn))
    # +-inf is not a gap
    _, lwi = L.host_filter_steps(model, raw, kind, par, xp, z, np.inf, first=first, missing=True)
    assert not np.any(bits(lwi) == 0)


@pytest.mark.parametrize("first", [False, True])
def test_missing_step_marginal_family(L, ob, first):
    """rows 1, 2 = the ordinary step's; row 0 = sp[0] (x0 at t = 0); rows 0 and 3 = rows 0 and 3 of the forecast at H = 1 from the
    same cloud (they do not depend on the normals); logw = +0.0"""
    raw, sp, z, y = step_edge_inputs.rb(first)
    sm, lwm = L.host_filter_steps(4, raw, CR.NONE, None, sp, z, NAN, first=first, missing=True)
    so, lwo = L.host_filter_steps(4, raw, CR.NONE, None, sp, z, y, first=first)
    ro, rlw = L.host_rb_steps(raw, sp, z, y, first)
    assert same(so, ro) and same(lwo, rlw)                     # the twin's ordinary step is the pinned marginal twin
    assert same(sm[1:3], so[1:3])
    assert np.all(bits(lwm) == 0)
    if first:
        assert same(sm[0], np.full(sp.shape[1], raw[2])) and same(sm[3], np.full(sp.shape[1], ob.exp(raw[3])))
    else:
        assert same(sm[0], sp[0])
        xf = L.host_forecast(4, raw, sp, 1, 99)[0]
        assert same(sm[0], xf[0, 0]) and same(sm[3], xf[0, 3])
    assert not same(sm[0], so[0]) and not same(sm[3], so[3])


def test_twin_refusals(L):
    z = np.zeros((1, 4))
    for args in ((2, SV, CR.OPTIMAL, None), (4, UC, CR.OPTIMAL, None), (1, LG, CR.AFFINE, None), (1, LG, CR.NONE, POOR), (9, LG, CR.NONE, None)):
        with pytest.raises(L.SmcError):
            L.host_filter_steps(args[0], args[1], args[2], args[3], None, np.zeros((2 if args[0] == 4 else 1, 4)), 0.1, first=True)
    with pytest.raises(L.SmcError):
        L.host_filter_steps(1, LG, CR.NONE, None, None, z[:, :0], 0.1, first=True)


# ---- (c) a gap adds nothing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,kind,n,seg,systematic", [(1, CR.NONE, 1000, 0, False), (2, CR.NONE, 3000, 256, False), (3, CR.NONE, 3000, 256, True),
                                                         (4, CR.NONE, 1024, 0, False), (1, CR.OPTIMAL, 5000, 1024, True), (3, CR.OPTIMAL, 1000, 0, False)])
def test_gap_adds_plus_zero(L, ob, model, kind, n, seg, systematic):
    """logmu = +0.0 and ess = n exactly at every gap, the weights are 1 / n; k trailing NaNs leave the bits of logZ alone"""
    y0 = L.simulate(3 if model == 4 else model, RAW[model], 12, 5)[1]
    gaps = (0, 4, 5, 11) if model != 4 else (3, 4, 11)         # (the marginal family carries y_1 into the state: keep it observed once)
    y = MR.with_gaps(y0, gaps)
    f = MR.MissingFilter(L, ob, model, RAW[model], n, seg=seg, seed=4, stream=1, kind=kind, systematic=systematic)
    for t in range(len(y)):
        lm, ess = f.init(y[t]) if t == 0 else f.step(y[t])
        if t in gaps:
            assert bits([lm])[0] == 0 and ess == float(n), (t, lm, ess)
            assert np.all(f.f.state()[1] == 1.0 / n)
        else:
            assert lm != 0.0 and ess < n
    assert np.isfinite(f.logZ)
    z = f.logZ
    for _ in range(3):
        f.step(NAN)
        assert same([f.logZ], [z])
    # the same series on a filter without the switch dies at its first NaN
    g = MR.MissingFilter(L, ob, model, RAW[model], n, seg=seg, seed=4, stream=1, kind=kind, systematic=systematic, missing=False)
    for t in range(len(y)):
        g.init(y[t]) if t == 0 else g.step(y[t])
    assert g.logZ == -np.inf


def test_collapsed_filter_at_a_gap(L, ob):
    """a filter that is collapsed when it meets a gap: identity ancestors, then uniform weights; logZ stays -inf"""
    y = [0.3, np.inf, NAN, 0.2]
    f = MR.MissingFilter(L, ob, 1, LG, 1000, seed=4)
    f.init(y[0])
    lm, ess = f.step(y[1])
    assert lm == -np.inf and ess == 0.0
    lm, ess = f.step(y[2])
    assert np.array_equal(f.f.state()[2], np.arange(1000)) and bits([lm])[0] == 0 and ess == 1000.0 and f.logZ == -np.inf
    lm, _ = f.step(y[3])
    assert np.isfinite(lm) and f.logZ == -np.inf


# ---- (d) the right model ----------------------------------------------------------------------------------------------------------
def test_unbiased_for_the_model_with_gaps_not_for_the_series_without_them(L, ob):
    """LG1D, the README row, T = 40, the eight gaps of MR.GAPS40, 256 filters of 1024 particles (streams 0..255): the mean of
    exp(logZ_k - KF) is within 4 sample standard errors of 1 for KF = the Kalman filter with the update skipped at the gaps, and
    outside that band for the Kalman value of the series with the gaps left out"""
    _, y0 = ob.simulate(1, LG, 40, 1998)
    y = MR.with_gaps(y0, MR.GAPS40)
    kf, kf_drop = MR.kalman_gaps(LG, y)[0], MR.kalman_gaps(LG, y, drop=True)[0]
    r = MR.run_series(L, ob, 1, np.tile(LG, (256, 1)), 1024, 0, 17, y)
    for name, ref, inside in (("gaps propagated", kf, True), ("gaps left out", kf_drop, False)):
        e = np.exp(r["logZ"] - ref)
        se = e.std(ddof=1) / np.sqrt(len(e))
        print("%s: KF %.4f  mean exp(logZ - KF) = %.4f +- %.4f" % (name, ref, e.mean(), se))
        assert (abs(e.mean() - 1.0) <= 4 * se) == inside, (name, e.mean(), se)


@pytest.mark.parametrize("lse0,lsn0", [(0.0, 0.0), (-1.0, 0.5)])
def test_marginal_family_with_frozen_volatilities_is_the_kalman_filter_with_gaps(L, ob, lse0, lsn0):
    """gamma_eps = gamma_eta = 0: every particle carries the exact Kalman recursion (A = B = 1, Q = exp(lse0), R = exp(lsn0), x_1 ~
    N(x0, Q)).  At a gap rows 0 and 3 are its predictive mean and variance; logZ is its log-likelihood with skipped updates.
    Tolerances: logZ to 1e-6, the bound of the frozen-volatility test of tests/test_composed_host.py; the moments to 1e-9
    relative (both recursions round a few ulp per step, 40 steps; sp_exp against numpy's exp: one ulp)"""
    T = 40
    y0 = L.simulate(3, UC, T, 7)[1]
    y = MR.with_gaps(y0, (3, 4, 5, 17, 39))
    Q, R = np.exp(lse0), np.exp(lsn0)
    ll, mp, Pp, mf, Pf = MR.kalman_gaps([1.0, 1.0, Q, R, 3.0, Q], y)
    f = MR.MissingFilter(L, ob, 4, [0.0, 0.0, 3.0, lse0, lsn0], 256, seed=3)
    for t in range(T):
        f.init(y[t]) if t == 0 else f.step(y[t])
        m, P = (mp[t], Pp[t]) if np.isnan(y[t]) else (mf[t], Pf[t])
        assert np.ptp(f.x[0]) == 0 and np.ptp(f.x[3]) == 0
        assert abs(f.x[0, 0] - m) <= 1e-9 * max(1.0, abs(m)) and abs(f.x[3, 0] - P) <= 1e-9 * P, (t, f.x[0, 0], m, f.x[3, 0], P)
    print("marginal family, frozen volatilities: logZ - Kalman = %.3g" % (f.logZ - ll))
    assert abs(f.logZ - ll) <= 1e-6, (f.logZ, ll)
