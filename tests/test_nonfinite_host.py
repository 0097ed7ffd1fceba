"""Non-finite observations and out-of-domain parameter rows on the CPU (no GPU): the references the GPU tests of
tests/test_gpu_nonfinite.py compare with stay within their own conditions on these inputs, and say what the contract is.

1. The oracle (oracle/smc_oracle.c) reproduces the table of tests/nonfinite_inputs.py as PROPERTIES: the dead steps are exactly the
   tagged ones, logZ = -inf iff a step is dead, after a dead step every weight is 0 and the next step's ancestors are the
   identity, and a bootstrap filter weighs again at the next finite observation.  If the oracle breaks one, the table is wrong.
2. The host twins of the guided and the marginal step (smc_host_guided_step(s), smc_host_rb_step(s)) on the edge inputs of
   tests/step_edge_inputs.py extended by y in BAD_Y, by a NaN, +inf and -inf planted in every row of the ancestor's state, and
   (marginal family) by P = 0 and P = +inf: batched == one particle; no usable log-weight when y is not finite; a particle
   whose own inputs are finite keeps its value.
3. tests/composed_reference.py over the bad series and rows: which guided / marginal filters weigh again after a bad observation.
   RESULT (asserted below): none does, once the bad observation has reached a guided or marginal step.

       family                       bad y_1 (t = 0)          bad y_t, t >= 1
       bootstrap LG1D / SV1D / UCSV recovers at t = 1        recovers at t + 1
       LG1D AFFINE (c2 = 0.1)       recovers (bootstrap      dead from t on (x = NaN or +-inf)
       LG1D AFFINE (c2 = 0)           first step)            dead from t on: fma(0, y, c0) is NaN for a non-finite y
       LG1D OPTIMAL                 recovers                 dead from t on
       UCSV OPTIMAL                 recovers                 dead from t on (row 0 NaN or +-inf)
       UCSV_RB (marginal)           dead from 0 on           dead from t on (the Kalman mean m)

4. The summaries' references on clouds that hold NaN and +-inf: what smc_host_quantile7, smc_host_sample_moments,
   tests/quantile7_reference.py and tests/summary_reference.py return.  CONTRACT of the unweighted mode (the device meets it in
   tests/test_gpu_nonfinite.py):
     * quantiles order the values by the IEEE total order of their bits, so a NaN sorts by its SIGN BIT: below -inf when it is
       set, above +inf when it is not.  A cloud that is all NaN has NaN quantiles at every level; a cloud with some NaNs has
       numbers at the levels whose two neighbours are numbers.  The twin and the Python reference agree on that bit for bit.
       np.quantile / Julia's quantile differ: they return NaN at EVERY level (Julia: an error) as soon as one value is NaN.
       The library keeps the total order (it is what makes the radix select and the sort agree) - a caller who wants numpy's
       answer has it from the NaN mean of the same summary row;
     * mean and variance are NaN as soon as one value is NaN; a cloud that holds infinities of one sign has that infinity as its
       mean and a NaN variance, as np.mean / np.var and Julia's mean / var.  (smc_host_sample_moments used to return a NaN mean
       there - inf - inf in its correction term - and disagreed with tests/quantile7_reference.py; settled in favour of np.mean.)
   Weighted mode: a particle without weight does not enter, whatever its state; a filter without weights has NaN summaries.
"""
import io
import math
import warnings

import numpy as np
import pytest

import composed_reference as CR
import nonfinite_inputs as NF
import quantile7_reference as Q7
import step_edge_inputs
import summary_reference as SR
from nonfinite_inputs import same_nan

N, SEG, SEED = 300, 256, 5


def finite_series(ob, model, seed=1998):
    m = NF.UCSV3D if model == NF.UCSV_RB else model
    return ob.simulate(m, NF.HEALTHY[m], NF.T, seed)[1]


def check_dead_properties(lm, es, logZ, dead, ctx):
    assert np.array_equal(np.isneginf(lm), dead), ctx + ("dead steps", lm)
    assert not np.any(np.isnan(lm)) and not np.any(np.isposinf(lm)), ctx + (lm,)
    assert np.all(es[dead] == 0) and np.all(es[~dead] > 0), ctx + (es,)
    assert (logZ == -np.inf) == bool(dead.any()) and (dead.any() or np.isfinite(logZ)), ctx + (logZ,)


def walk_oracle(ob, model, raw, y, dead, ctx):
    """the oracle step by step: after a dead step every weight is 0 and the next step's ancestors are the identity"""
    f = ob.Filter(model, raw, N, seg=SEG, seed=SEED)
    lm, es = [], []
    for t in range(len(y)):
        if t == 0:
            lm.append(f.bootstrap_filter(float(y[0])))
            es.append(f.ess())
        else:
            l, e = f.step(float(y[t]))
            lm.append(l)
            es.append(e)
        x, w, a, _ = f.state()
        if dead[t]:
            assert np.all(w == 0), ctx + (t, "weights after a dead step")
        else:
            assert abs(w.sum() - 1) < 1e-12 and np.all(w >= 0), ctx + (t, w.sum())
        if t > 0 and dead[t - 1]:
            assert np.array_equal(a, np.arange(N)), ctx + (t, "ancestors after a dead step")
    return np.array(lm), np.array(es), f


@pytest.mark.parametrize("bad", NF.BAD_Y, ids=NF.BAD_Y_IDS)
@pytest.mark.parametrize("model", [NF.LG1D, NF.SV1D, NF.UCSV3D])
def test_oracle_bad_observations(ob, model, bad):
    y0 = finite_series(ob, model)
    for pos in NF.POSITIONS:
        ctx = (model, bad, pos)
        y = NF.bad_series(y0, pos, bad)
        dead = np.zeros(NF.T, dtype=bool)
        dead[list(pos)] = True
        lm, es, f = walk_oracle(ob, model, NF.HEALTHY[model], y, dead, ctx)
        z, lm2, es2 = ob.Filter(model, NF.HEALTHY[model], N, seg=SEG, seed=SEED).log_likelihood(y, trace=True)
        assert same_nan(lm, lm2) and same_nan(es, es2)
        check_dead_properties(lm, es, z, dead, ctx)
        x = f.state()[0]
        assert np.all(np.isfinite(x)), ctx + ("a bootstrap filter keeps finite states through a bad observation",)
        for p in pos:                                              # ... and weighs again at the next finite observation
            if p + 1 < NF.T and not dead[p + 1]:
                assert np.isfinite(lm[p + 1]), ctx


@pytest.mark.parametrize("rid,model,raw,tag", NF.BOOTSTRAP_ROWS, ids=[r[0] for r in NF.BOOTSTRAP_ROWS])
def test_oracle_bad_rows(ob, rid, model, raw, tag):
    y = finite_series(ob, model)
    dead = NF.dead_steps(NF.T, tag)
    lm, es, f = walk_oracle(ob, model, raw, y, dead, (rid,))
    z, lm2, es2 = ob.Filter(model, raw, N, seg=SEG, seed=SEED).log_likelihood(y, trace=True)
    assert same_nan(lm, lm2) and same_nan(es, es2)
    check_dead_properties(lm, es, z, dead, (rid,))
    if tag is NF.ALIVE:
        assert np.all(np.isfinite(f.state()[0]))


def test_same_nan_is_exact():
    """the comparison of every test here and in tests/test_gpu_nonfinite.py: NaNs of any sign and payload match each other and
    nothing else; everywhere else one differing bit (the sign of a zero, one ulp) is a mismatch"""
    a = np.array([1.0, NF.NAN, -0.0, NF.INF])
    neg_nan = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]
    assert same_nan(a, [1.0, neg_nan, -0.0, NF.INF]) and same_nan(NF.NAN, neg_nan) and same_nan(-NF.INF, -NF.INF)
    assert not same_nan(a, [1.0, NF.NAN, 0.0, NF.INF]) and not same_nan(a, [np.nextafter(1.0, 2.0), NF.NAN, -0.0, NF.INF])
    assert not same_nan(a, [NF.NAN, 1.0, -0.0, NF.INF]) and not same_nan(a, [1.0, NF.INF, -0.0, NF.INF]) and not same_nan(a, a[:3])
    assert not same_nan(NF.NAN, -NF.INF) and not same_nan(NF.INF, -NF.INF)


# ---- 2. host twins ---------------------------------------------------------------------------------------------------------
def lw_alive(l):
    l = np.asarray(l, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ~np.isnan(l) & (np.abs(l) <= 7e8)


@pytest.mark.parametrize("fam", ["lg-affine", "lg-optimal", "uc-optimal"])
def test_guided_twins_on_extended_edge_inputs(L, fam):
    model, kind, _ = NF.COMPOSED[fam]
    raw, par, xp0, z, y0 = step_edge_inputs.guided(model, kind)
    xp, planted = NF.plant(xp0)
    base_x, base_lw = L.host_guided_steps(model, raw, kind, par, xp0, z, y0)
    for y in (y0,) + NF.BAD_Y:
        x, lw = L.host_guided_steps(model, raw, kind, par, xp, z, y)
        for i in range(xp.shape[1]):
            hx, hl = L.host_guided_step(model, raw, kind, par, xp[:, i], z[:, i], y)
            assert same_nan(x[:, i], hx) and same_nan(lw[i], hl), (fam, y, i, x[:, i], hx, lw[i], hl)
        if not math.isfinite(y):
            assert not lw_alive(lw).any(), (fam, y)
        else:                                                      # a particle whose own inputs are finite keeps its value
            keep = ~planted
            assert same_nan(x[:, keep], base_x[:, keep]) and same_nan(lw[keep], base_lw[keep]), fam
            assert np.array_equal(x[:, keep].view(np.uint64), base_x[:, keep].view(np.uint64))
            assert not lw_alive(lw[planted]).all(), fam          # (some planted values do kill their particle)


@pytest.mark.parametrize("first", [False, True])
def test_rb_twins_on_extended_edge_inputs(L, first):
    raw, sp0, z, y0 = step_edge_inputs.rb(first)
    sp, planted = NF.plant(sp0, variance_row=3)
    base_s, base_lw = L.host_rb_steps(raw, sp0, z, y0, first)
    for y in (y0,) + NF.BAD_Y:
        s, lw = L.host_rb_steps(raw, sp, z, y, first)
        for i in range(sp.shape[1]):
            hs, hl = L.host_rb_step(raw, sp[:, i], z[:, i], y, first)
            assert same_nan(s[:, i], hs) and same_nan(lw[i], hl), (first, y, i, s[:, i], hs, lw[i], hl)
        if not math.isfinite(y):
            assert not lw_alive(lw).any(), (first, y)
        else:
            keep = np.ones_like(planted) if first else ~planted    # (the first step does not read the state)
            assert np.array_equal(s[:, keep].view(np.uint64), base_s[:, keep].view(np.uint64)) and same_nan(lw[keep], base_lw[keep])


# ---- 3. whole series of the guided and the marginal filters ----------------------------------------------------------------
def run_composed(L, ob, fam, raw, y):
    model, kind, par = NF.COMPOSED[fam]
    f = CR.ComposedFilter(L, ob, model, raw, N, seg=SEG, seed=SEED, kind=kind, par=par)
    f.init(float(y[0]))
    for t in range(1, len(y)):
        a_before = f.f.state()[1]
        f.step(float(y[t]))
        if np.all(a_before == 0):
            assert np.array_equal(f.f.state()[2], np.arange(N))
    return np.array(f.lm), np.array(f.es), f.logZ, f


@pytest.mark.parametrize("fam", list(NF.COMPOSED))
def test_composed_filters_recover_or_stay_dead(L, ob, fam):
    model = NF.COMPOSED[fam][0]
    y0 = finite_series(ob, model)
    for bad in NF.BAD_Y:
        for pos in NF.POSITIONS:
            dead = NF.dead_steps(NF.T, NF.composed_y_tag(fam, pos))
            lm, es, z, f = run_composed(L, ob, fam, NF.HEALTHY[model], NF.bad_series(y0, pos, bad))
            check_dead_properties(lm, es, z, dead, (fam, bad, pos))
            if dead[-1] and min(pos) > 0:                          # what keeps it dead: y went into row 0 of the state
                assert not np.isfinite(f.x[0]).any(), (fam, bad, pos)
    for rid, m, raw, tag in NF.rows_of(model):
        dead = NF.dead_steps(NF.T, NF.composed_row_tag(fam, rid, tag))
        lm, es, z, _ = run_composed(L, ob, fam, raw, y0)
        check_dead_properties(lm, es, z, dead, (fam, rid))


# ---- 4. summaries on clouds that hold NaN and +-inf -------------------------------------------------------------------------
PS = [0.0, 0.25, 0.5, 0.75, 1.0]
NEG_NAN = float(np.uint64(0xFFF8000000000000).view(np.float64))
POS_NAN = float(np.uint64(0x7FF8000000000000).view(np.float64))


def clouds():
    x = np.random.default_rng(1).normal(size=301)
    out = {"all-nan": np.full(301, POS_NAN), "all-nan-mixed-signs": np.where(np.arange(301) % 2, POS_NAN, NEG_NAN)}
    for name, idx, val in (("one+nan", [5], POS_NAN), ("one-nan", [5], NEG_NAN), ("+inf", [5], np.inf), ("-inf", [5, 9], -np.inf),
                           ("both-inf", [5, 7], None), ("nan-and-inf", [3, 4, 5], None)):
        c = x.copy()
        c[idx] = val if val is not None else ([-np.inf, np.inf] if name == "both-inf" else [NEG_NAN, np.inf, POS_NAN])
        out[name] = c
    return out


@pytest.mark.parametrize("name", list(clouds()))
def test_unweighted_references_on_nonfinite_clouds(L, name):
    c = clouds()[name]
    q = L.host_quantile7(c, PS)
    with np.errstate(invalid="ignore"):
        ref = Q7.quantile7(c, PS)
    assert same_nan(q, ref), (name, q, ref)                                # twin == Python reference, NaN-aware and bit for bit
    nan = np.isnan(c)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        npq, npm = np.quantile(c, PS), np.mean(c)
        npv = np.var(c, ddof=1)
    if nan.all():
        assert np.isnan(q).all()
    elif nan.any():
        # the total order: a NaN with the sign bit sorts below -inf, one without above +inf; numpy gives NaN at every level
        assert np.isnan(npq).all() and not np.isnan(q).all(), (name, q)
        lo_nan, hi_nan = np.signbit(c[nan]).sum(), (~np.signbit(c[nan])).sum()
        assert np.isnan(q[0]) == bool(lo_nan) and np.isnan(q[-1]) == bool(hi_nan), (name, q)
        with np.errstate(invalid="ignore"):
            assert same_nan(q[1:4], Q7.quantile7(np.concatenate([np.full(lo_nan, -np.inf), c[~nan], np.full(hi_nan, np.inf)]), PS)[1:4])
    else:
        fin = np.isfinite(npq)                                             # (numpy's lerp gives NaN next to an infinity)
        assert np.array_equal(q[~fin & ~np.isnan(npq)], npq[~fin & ~np.isnan(npq)])
        for j in np.flatnonzero(fin):
            assert abs(q[j] - npq[j]) <= Q7.cross_bound(c, PS[j]), (name, j)
    m, v = L.host_sample_moments(c)
    assert same_nan(m, npm) or (np.isfinite(npm) and abs(m - npm) <= 1e-12 * max(1.0, abs(npm))), (name, m, npm)
    assert np.isnan(v) and np.isnan(npv), (name, v, npv)                   # every cloud here holds a NaN or an infinity
    if not (np.isposinf(c).any() and np.isneginf(c).any()):               # (math.fsum refuses inf - inf)
        with np.errstate(invalid="ignore"):
            rm, rv = Q7.sample_moments(c)
        assert same_nan(m, rm) and np.isnan(rv), (name, m, rm)


def test_weighted_references_on_nonfinite_clouds(ob):
    """a dead filter (every weight 0) has NaN weighted summaries whatever its states hold; the oracle and the exact references
    agree; a filter that died on a bad observation and weighs again has ordinary ones"""
    for rid, model, raw, tag in NF.BOOTSTRAP_ROWS:
        if tag is NF.ALIVE:
            continue
        f = ob.Filter(model, raw, N, seg=SEG, seed=SEED)
        f.log_likelihood(finite_series(ob, model))
        x, w, _, _ = f.state()
        assert np.all(w == 0)
        assert np.isnan(f.quantiles([0.25, 0.5, 0.75])).all() and np.isnan(f.moments()[0]).all() and np.isnan(f.moments()[1]).all()
        SR.check_quantiles(f.quantiles([0.25, 0.5]), [0.25, 0.5], x[0], w, 0.0, (rid,))
        SR.check_moments(f.moments()[0][0], f.moments()[1][0], x[0], w, (rid,))
    y = NF.bad_series(finite_series(ob, NF.LG1D), (2,), NF.NAN)
    f = ob.Filter(NF.LG1D, NF.LG, N, seg=SEG, seed=SEED)
    f.log_likelihood(y[:3])
    assert np.isnan(f.quantiles([0.5])).all()
    f.step(float(y[3]))
    x, w, _, _ = f.state()
    ps = [0.25, 0.5, 0.75]
    SR.check_quantiles(f.quantiles(ps), ps, x[0], w, SR.quantile_delta(N, 2, SEG, math.fsum(w)), ("recovered",))
    SR.check_moments(f.moments()[0][0], f.moments()[1][0], x[0], w, ("recovered",))


# ---- 5. samplers that reach invalid rows (the conditions of tests/test_gpu_nonfinite.py, on the reference side) -----------
@pytest.mark.parametrize("online", [False, True], ids=["density_tempered", "online"])
def test_sampler_conditions_hold_on_the_oracle_backend(ob, online):
    from oracle_backend import OracleBackend
    s, text, _, rec, theta0 = NF.run_sampler(OracleBackend(), online, replay=ob)
    NF.sampler_conditions(rec, theta0)
    NF.sampler_properties(s, rec)
    assert "[rejuvenating]" in text


def test_python_models_refuse_out_of_domain_parameters():
    """device=False builds the Python model per theta: its constructor refuses what the ThetaMap route lets through"""
    import sequential_monte_carlo_amd as smc
    from oracle_backend import OracleBackend
    for kw in (dict(Q=-0.1), dict(Q=0.0), dict(R=-1.0)):
        with pytest.raises(ValueError):
            smc.UnivariateLinearGaussian(**{**dict(A=0.5, B=1.0, Q=0.9, R=0.8), **kw})
    s = smc.SMC(NF.SAMPLER_N, NF.SAMPLER_M, NF.sampler_model, NF.sampler_prior(), 2, 0.5, seed=NF.SAMPLER_SEED[False], backend=OracleBackend())
    assert not s.device_pmmh and np.any(s.theta[:, 1] <= 0)
    with pytest.raises(ValueError):
        smc.density_tempered(s, NF.sampler_series(), verbose=False, out=io.StringIO())
