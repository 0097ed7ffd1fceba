"""Missing observations on every launch path (pytest -m gpu): handles created with FLAG_NAN_MISSING read a NaN observation as a
period without one.  The reference is tests/missing_reference.py (composed from the oracle's track, resampler and
normals and the host twin of the whole step; tests/test_missing_host.py pins it on the CPU).  Comparisons are exact (the same bits;
array_equal for ancestors and the raw fixed-point weights) except the moments of the summaries, which carry the bounds of
tests/summary_reference.py / tests/quantile7_reference.py, and the two statistical statements, which use 4 sample standard errors.

  a. bit-exact on every path of tests/test_gpu_paths.py (first and last shape), all four families and the three proposals: gaps
     at the first, a middle and the last step, and two in a row; smc_log_likelihood with and without traces, the step API after
     every step, smc_step_window / smc_step_commit before, at and after a gap; systematic resampling, ragged last segments
  b. a flagged handle on a NaN-free series == an unflagged one; +inf kills the step of both alike
  c. trailing gaps leave logZ alone; skip masks
  d. per-step summaries at a gap
  e. the record: smc_smooth, smc_sample_paths == their host twins; the smoothed mean at a gap against the RTS smoother with
     skipped updates; smc_rb_sample_paths refuses
  f. smc_device_filter_steps == smc_host_filter_steps
  g. the samplers
"""
import io
import math

import numpy as np
import pytest

import composed_reference as CR
import missing_reference as MR
import nonfinite_inputs as NF
import quantile7_reference as Q7
import step_edge_inputs
import summary_reference as SR
import test_gpu_paths as TP
from nonfinite_inputs import same_nan

pytestmark = pytest.mark.gpu

T, NTH, SEED = NF.T, 3, 5
NAN = float("nan")
POOR = [0.3, 0.2, 0.1, 2.0]
SHAPES = []
for _pid, _cs in TP.PATHS.items():
    for _c in (_cs[0], _cs[-1]):
        SHAPES.append((_pid, _c))
# (family tag, model id of the handle, proposal kind): what runs on a shape of model m
FAMILIES = {1: (("lg", 1, CR.NONE), ("lg-affine", 1, CR.AFFINE), ("lg-optimal", 1, CR.OPTIMAL)), 2: (("sv", 2, CR.NONE),),
            3: (("ucsv", 3, CR.NONE), ("ucsv-optimal", 3, CR.OPTIMAL), ("ucsv-rb", 4, CR.NONE))}
VARIANTS = [(pid, c, fam) for pid, c in SHAPES for fam in FAMILIES[c[0]]]
VARIANT_IDS = ["%s-n%d-%s" % (pid, c[1], fam[0]) for pid, c, fam in VARIANTS]
# first + middle + last, and two in a row
GAP_SETS = ((0, 2, T - 1), (2, 3))


def series(model, gaps, seed=1998, length=T):
    from oracle import binding as ob
    m = 3 if model == 4 else model
    return MR.with_gaps(ob.simulate(m, TP.RAW[m], length, seed)[1], gaps)


def make(L, pid, case, fam, nth=NTH, flags=None, seed=SEED):
    """the handle of a variant, flagged unless flags says otherwise; (handle, raws, proposal rows or None)"""
    _, model, kind = fam
    flags = L.FLAG_NAN_MISSING if flags is None else flags
    raws = TP.raws_for(3 if model == 4 else model, nth)
    h = L.Handle(model, nth, case[1], seg=case[2], seed=seed, flags=case[3] | flags | L.FLAG_ANCESTORS)
    assert TP.path_of(h) == pid, (pid, case, fam, h.seg, h.nseg, h.resident)
    h.set_params(raws)
    pars = np.tile(POOR, (nth, 1)) if kind == CR.AFFINE else None
    if kind != CR.NONE:
        h.set_proposal(kind, pars)
    return h, raws, pars


def snap(h):
    return h.state() + h.weights_raw()


def reference(L, ob, case, fam, raws, pars, y, systematic=False, missing=True):
    return MR.run_series(L, ob, fam[1], raws, case[1], case[2], SEED, y, kind=fam[2], pars=pars, systematic=systematic, missing=missing,
                         every=True)


def check_series(h, r, y, ctx):
    """smc_log_likelihood with traces, without traces, and the step API after every step"""
    h.reseed(SEED)
    z, lm, es = h.log_likelihood(y, trace=True)
    assert TP.same(z, r["logZ"]) and TP.same(lm, r["lm"]) and TP.same(es, r["es"]), ctx + ("traces", z, r["logZ"], lm, r["lm"])
    assert MR.first_mismatch(snap(h), r["snap"]) is None, ctx + ("traces", MR.first_mismatch(snap(h), r["snap"]))
    h.reseed(SEED)
    z = h.log_likelihood(y)
    assert TP.same(z, r["logZ"]), ctx + ("no traces", z, r["logZ"])
    assert MR.first_mismatch(snap(h), r["snap"]) is None, ctx + ("no traces", MR.first_mismatch(snap(h), r["snap"]))
    h.reseed(SEED)
    for t in range(len(y)):
        if t == 0:
            l, e = h.init(float(y[0])), h.logZ()[1]
        else:
            l, e = h.step(float(y[t]))
        assert TP.same(l, r["lm"][t]) and TP.same(e, r["es"][t]), ctx + ("step API", t, l, r["lm"][t], e, r["es"][t])
        assert MR.first_mismatch(snap(h), r["snaps"][t]) is None, ctx + ("step API", t, MR.first_mismatch(snap(h), r["snaps"][t]))
    assert TP.same(h.logZ()[0], r["logZ"]), ctx + ("logZ of the step API",)


# ---- a. every path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid,case,fam", VARIANTS, ids=VARIANT_IDS)
def test_gaps_on_every_path(L, ob, pid, case, fam):
    h, raws, pars = make(L, pid, case, fam)
    assert h.missing
    for gaps in GAP_SETS:
        y = series(fam[1], gaps)
        r = reference(L, ob, case, fam, raws, pars, y)
        for t in gaps:
            assert np.all(r["lm"][t].view(np.uint64) == 0) and np.all(r["es"][t] == case[1])
        assert np.all(np.isfinite(r["logZ"]))
        check_series(h, r, y, (pid, case, fam[0], gaps))
    h.close()


@pytest.mark.parametrize("pid,case,fam", [v for v in VARIANTS if v[0] == "R"], ids=[i for v, i in zip(VARIANTS, VARIANT_IDS) if v[0] == "R"])
def test_gaps_inside_a_step_window(L, ob, pid, case, fam):
    """init, then a window of five, kept to j = 1, 2, 4 steps: with the gaps at (2, 3) that commits before, at and after a gap,
    with (0, 2, 5) after a missing first step.  The window's (logmu, ess) and the state after the kept prefix are the reference's."""
    h, raws, pars = make(L, pid, case, fam)
    assert h.can_window
    for gaps in GAP_SETS:
        y = series(fam[1], gaps)
        r = reference(L, ob, case, fam, raws, pars, y)
        for j in (1, 2, 4):
            ctx = (pid, case, fam[0], gaps, j)
            h.reseed(SEED)
            h.init(float(y[0]))
            lm, es = h.step_window(y[1:])
            assert TP.same(lm, r["lm"][1:]) and TP.same(es, r["es"][1:]), ctx + ("window", lm, r["lm"][1:])
            x0, w0, _ = h.state()                                  # (a window does not move the filters; the ancestor vector is the launch's)
            assert TP.same(x0, r["snaps"][0][0]) and TP.same(w0, r["snaps"][0][1]), ctx + ("a window moved the filter",)
            h.step_commit(j)
            assert MR.first_mismatch(snap(h), r["snaps"][j]) is None, ctx + ("after commit", MR.first_mismatch(snap(h), r["snaps"][j]))
            z = r["lm"][0].copy()
            for t in range(1, j + 1):
                z = z + r["lm"][t]
            assert TP.same(h.logZ()[0], z), ctx + ("logZ after commit", h.logZ()[0], z)
    h.close()


SYS_CASES = [((1, 1000, 0, 0), ("lg", 1, CR.NONE)), ((1, 1000, 0, TP.NO_RESIDENT), ("lg-optimal", 1, CR.OPTIMAL)), ((3, 3000, 512, 0), ("ucsv", 3, CR.NONE)),
             ((3, 3000, 512, 0), ("ucsv-rb", 4, CR.NONE)), ((3, 1000, 0, 0), ("ucsv-optimal", 3, CR.OPTIMAL)), ((2, 40000, 256, 0), ("sv", 2, CR.NONE))]


@pytest.mark.parametrize("case,fam", SYS_CASES, ids=["%s-n%d-%d" % (f[0], c[1], c[3]) for c, f in SYS_CASES])
def test_gaps_with_systematic_resampling_and_ragged_segments(L, ob, case, fam):
    """FLAG_SYSTEMATIC, n no multiple of the segment: resident, single-segment step, multi-segment and two-record shapes"""
    raws = TP.raws_for(3 if fam[1] == 4 else fam[1], NTH)
    h = L.Handle(fam[1], NTH, case[1], seg=case[2], seed=SEED, flags=case[3] | L.FLAG_SYSTEMATIC | L.FLAG_ANCESTORS | L.FLAG_NAN_MISSING)
    assert h.nseg * h.seg != case[1]
    h.set_params(raws)
    if fam[2] != CR.NONE:
        h.set_proposal(fam[2], None)
    for gaps in GAP_SETS:
        y = series(fam[1], gaps)
        r = reference(L, ob, case, fam, raws, None, y, systematic=True)
        check_series(h, r, y, ("systematic", case, fam[0], gaps))
    h.close()


# ---- b. the flag alone changes nothing ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid,case,fam", VARIANTS, ids=VARIANT_IDS)
def test_flag_without_nan_is_the_unflagged_handle(L, ob, pid, case, fam):
    """a NaN-free series, and one with +inf at step 2 (which kills the step of both): traces, logZ, the state - through
    smc_log_likelihood and the step API"""
    hf, _, _ = make(L, pid, case, fam)
    hu, _, _ = make(L, pid, case, fam, flags=0)
    assert hf.missing and not hu.missing
    y0 = series(fam[1], ())
    for y in (y0, NF.bad_series(y0, (2,), NF.INF)):
        out = []
        for h in (hf, hu):
            h.reseed(SEED)
            z, lm, es = h.log_likelihood(y, trace=True)
            s1 = snap(h)
            h.reseed(SEED)
            ls = [h.init(float(y[0]))] + [h.step(float(v))[0] for v in y[1:]]
            out.append((z, lm, es, np.array(ls), h.logZ()[0]) + s1 + snap(h))
        for k, (a, b) in enumerate(zip(*out)):
            assert np.array_equal(a, b) if np.asarray(a).dtype.kind in "iu" else same_nan(a, b), (pid, case, fam[0], k)
        if not np.all(np.isfinite(y)):
            assert np.all(out[0][0] == -np.inf) and np.all(np.isneginf(out[0][1][2]))
            if pid in ("R",):
                for h in (hf, hu):
                    h.reseed(SEED)
                    h.init(float(y[0]))
                    out.append(h.step_window(y[1:]))
                assert same_nan(out[-1][0], out[-2][0]) and same_nan(out[-1][1], out[-2][1])
    hf.close()
    hu.close()


@pytest.mark.parametrize("pid,case,fam", [v for v in VARIANTS if v[1][1] in (1024, 3000, 40000)],
                         ids=[i for v, i in zip(VARIANTS, VARIANT_IDS) if v[1][1] in (1024, 3000, 40000)])
def test_collapsed_filter_meets_a_gap(L, ob, pid, case, fam):
    """+inf at step 1 collapses every filter, the gap at step 2 finds it collapsed: identity ancestors, then uniform weights (the
    guided and marginal families carry NaN states from the +inf on); logZ stays -inf; the reference's bits, NaN positions included"""
    h, raws, pars = make(L, pid, case, fam)
    y = series(fam[1], (2,))
    y[1] = np.inf
    r = reference(L, ob, case, fam, raws, pars, y)
    assert np.all(np.isneginf(r["lm"][1])) and np.all(r["lm"][2].view(np.uint64) == 0) and np.all(r["es"][2] == case[1]) and np.all(r["logZ"] == -np.inf)
    assert np.array_equal(r["snaps"][2][2], np.tile(np.arange(case[1]), (NTH, 1)))
    for trace in (True, False):
        h.reseed(SEED)
        out = h.log_likelihood(y, trace=trace)
        if trace:
            assert same_nan(out[1], r["lm"]) and same_nan(out[2], r["es"]), (pid, case, fam[0])
        assert np.all((out[0] if trace else out) == -np.inf)
        for k, (a, b) in enumerate(zip(snap(h), r["snap"])):
            assert np.array_equal(a, b) if np.asarray(a).dtype.kind in "iu" else same_nan(a, b), (pid, case, fam[0], trace, k)
    h.reseed(SEED)
    h.init(float(y[0]))
    for t in range(1, T):
        l, e = h.step(float(y[t]))
        assert same_nan(l, r["lm"][t]) and same_nan(e, r["es"][t]), (pid, case, fam[0], t)
        for k, (a, b) in enumerate(zip(snap(h), r["snaps"][t])):
            assert np.array_equal(a, b) if np.asarray(a).dtype.kind in "iu" else same_nan(a, b), (pid, case, fam[0], "step API", t, k)
    h.close()


# ---- c. trailing gaps, skip masks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid,case", SHAPES, ids=["%s-m%d-n%d" % (p, c[0], c[1]) for p, c in SHAPES])
def test_trailing_gaps_and_skip_masks(L, ob, pid, case):
    fam = FAMILIES[case[0]][0]
    h, raws, _ = make(L, pid, case, fam)
    y = series(fam[1], (1, 3))
    h.reseed(SEED)
    z = h.log_likelihood(y)
    full = snap(h)
    for k in (1, 3):
        h.reseed(SEED)
        zk, lm, es = h.log_likelihood(np.concatenate([y, np.full(k, NAN)]), trace=True)
        assert TP.same(zk, z), (pid, case, k, zk, z)
        assert np.all(lm[T:].view(np.uint64) == 0) and np.all(es[T:] == case[1])
    # a skip mask: the active slots are those of the unskipped run, the skipped one keeps its state and reads -inf
    h.reseed(SEED)
    h.log_likelihood(y)
    h.set_skip([0, 1, 0])
    h.reseed(SEED)
    zs = h.log_likelihood(y)
    h.set_skip(None)
    got = snap(h)
    assert zs[1] == -np.inf and TP.same(zs[[0, 2]], z[[0, 2]])
    for k, (a, b) in enumerate(zip(got, full)):
        a, b = (a[:, [0, 2]], b[:, [0, 2]]) if k == 0 else (a[[0, 2]], b[[0, 2]])
        assert np.array_equal(a, b) if a.dtype.kind in "iu" else TP.same(a, b), (pid, case, "skip", k)
    h.close()


# ---- d. summaries at a gap -----------------------------------------------------------------------------------------------------------
PS = [0.25, 0.5, 0.75]


@pytest.mark.parametrize("mode", ["weighted", "unweighted"])
@pytest.mark.parametrize("pid,case", [("R", (1, 1000, 0, 0)), ("M1", (1, 5000, 1024, 0))], ids=["R", "M1"])
def test_summaries_at_a_gap(L, ob, pid, case, mode):
    """per-step quantiles and moments inside smc_log_likelihood on a series with gaps at (0, 2, 3): at every step, the gaps
    included, the references on the reference's cloud within the bounds of their modules; weighted quantiles also the oracle's
    bit for bit"""
    fam = FAMILIES[1][0]
    h, raws, _ = make(L, pid, case, fam)
    y = series(1, (0, 2, 3))
    h.set_summary_mode(mode)
    h.set_summaries(PS, 0, moments=True)
    h.reseed(SEED)
    h.log_likelihood(y)
    q, mean, var = h.get_summaries(T)
    n = case[1]
    for th in range(NTH):
        f = MR.MissingFilter(L, ob, 1, raws[th], n, seg=case[2], seed=SEED, stream=th)
        for t in range(T):
            f.init(y[t]) if t == 0 else f.step(y[t])
            ctx = (pid, mode, th, t)
            x, w = f.x[0], f.f.state()[1]
            if mode == "weighted":
                assert TP.same(q[t, th], f.f.quantiles(PS)), ctx + (q[t, th], f.f.quantiles(PS))
                SR.check_quantiles(q[t, th], PS, x, w, SR.quantile_delta(n, h.nseg, h.seg, math.fsum(w)), ctx)
                SR.check_moments(mean[t, 0, th], var[t, 0, th], x, w, ctx)
            else:
                assert Q7.same_bits(q[t, th], Q7.quantile7(x, PS)), ctx + (q[t, th], Q7.quantile7(x, PS))
                Q7.check_sample_moments(mean[t, 0, th], var[t, 0, th], x, ctx)
    h.set_summaries()
    h.close()


# ---- e. the record ---------------------------------------------------------------------------------------------------------------------
def recorded_run(L, model, raws, y, n, seg=0, streams=None):
    h = L.Handle(model, len(raws), n, seg=seg, seed=SEED, flags=L.FLAG_ANCESTORS | L.FLAG_NAN_MISSING)
    h.set_params(raws)
    if streams is not None:
        h.set_streams(streams)
    h.history_begin(len(y))
    h.init(float(y[0]))
    for t in range(1, len(y)):
        h.step(float(y[t]))
    rec = [h.history_get(t) for t in range(len(y))]
    return h, np.stack([r[0] for r in rec]), np.stack([r[1] for r in rec])        # x [T][d][nth][n], w [T][nth][n]


@pytest.mark.parametrize("model", [1, 3])
def test_record_with_gaps_equals_the_host_twins(L, ob, model):
    raws = TP.raws_for(model, NTH)
    y = series(model, (0, 2, 3))
    h, xs, ws = recorded_run(L, model, raws, y, 300, 256)
    assert np.all(ws[[0, 2, 3]] == 1.0 / 300) and np.all(np.isfinite(xs))
    sw, mean, var = h.smooth()
    idx, px = h.sample_paths(64, 17)
    for th in range(NTH):
        hw, hm, hv = L.host_smooth(model, raws[th], xs[:, :, th], ws[:, th])
        assert TP.same(sw[:, th], hw) and TP.same(mean[:, :, th], hm) and TP.same(var[:, :, th], hv), (model, th, "smc_smooth")
        hi, hx = L.host_sample_paths(model, raws[th], xs[:, :, th], ws[:, th], 64, 17, stream=th)
        assert np.array_equal(idx[:, th], hi) and TP.same(px[:, :, th], hx) and np.all(hi >= 0), (model, th, "smc_sample_paths")
    h.close()


def test_smoothed_mean_at_the_gaps_is_the_interpolation(L, ob):
    """LG1D, N = 1024, T = 30, gaps at (7, 15, 16): the mean over 32 filters (streams 0..31) of the smoothed mean at each gap within
    4 standard errors (from the 32) of the RTS smoother with skipped updates"""
    gaps = (7, 15, 16)
    y = series(1, gaps, length=30)
    raws = np.tile(MR.README_LG, (32, 1))
    h, _, _ = recorded_run(L, 1, raws, y, 1024)
    _, mean, _ = h.smooth(weights=False)
    ms, _ = MR.rts_gaps(MR.README_LG, y)
    for t in gaps:
        m = mean[t, 0]
        se = m.std(ddof=1) / np.sqrt(len(m))
        print("gap %d: smoothed mean %.4f +- %.4f, RTS %.4f" % (t, m.mean(), se, ms[t]))
        assert abs(m.mean() - ms[t]) <= 4 * se, (t, m.mean(), se, ms[t])
    h.close()


def test_rb_sample_paths_refuses_a_gap(L, ob):
    raws = TP.raws_for(3, NTH)
    y = series(4, (2,))
    h, _, _ = recorded_run(L, 4, raws, y, 300, 256)
    with pytest.raises(L.SmcError):
        h.rb_sample_paths(y, 16, 19)
    r = h.rb_sample_paths(series(4, ()), 16, 19)                      # (a finite y is taken as ever)
    assert np.all(r["idx"] >= 0)
    h.close()


# ---- f. the one-step twins --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("y", [0.7, NAN, np.inf])
def test_device_filter_steps_equals_host(L, y, first):
    for model, kind in ((1, CR.NONE), (2, CR.NONE), (3, CR.NONE), (1, CR.AFFINE), (1, CR.OPTIMAL), (3, CR.OPTIMAL)):
        raw, par, xp, z, _ = step_edge_inputs.guided(3 if model == 3 else 1, kind if kind else CR.OPTIMAL)
        raw, par = ([0.0, 0.95, 0.3] if model == 2 else raw), (par if kind == CR.AFFINE else None)
        for missing in (False, True):
            hx, hl = L.host_filter_steps(model, raw, kind, par, xp, z, y, first=first, missing=missing)
            dx, dl = L.device_filter_steps(model, raw, kind, par, xp, z, y, first=first, missing=missing)
            assert same_nan(dx, hx) and same_nan(dl, hl), (model, kind, y, first, missing)
    raw, sp, z, _ = step_edge_inputs.rb(first)
    for missing in (False, True):
        hx, hl = L.host_filter_steps(4, raw, CR.NONE, None, sp, z, y, first=first, missing=missing)
        dx, dl = L.device_filter_steps(4, raw, CR.NONE, None, sp, z, y, first=first, missing=missing)
        assert same_nan(dx, hx) and same_nan(dl, hl), ("rb", y, first, missing)


# ---- g. the samplers ------------------------------------------------------------------------------------------------------------------
def sampler(missing, seed=22):
    import sequential_monte_carlo_amd as smc
    prior = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(), smc.LogNormal()])
    tmap = smc.ThetaMap(1, [0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    return smc.SMC(256, 64, lambda th: smc.UnivariateLinearGaussian(A=th[0], B=1.0, Q=th[1], R=th[2]), prior, 2, 0.6, seed=seed, theta_map=tmap,
                   missing=missing)


def run_sampler(s, y, online):
    import sequential_monte_carlo_amd as smc
    if online:
        smc.smc2(s, y)
        smc.smc2_run(s, y, 2, len(y), window=4, verbose=False, out=io.StringIO())
    else:
        smc.density_tempered(s, y, verbose=False, out=io.StringIO())
    return s.theta.copy(), s.logZ.copy(), np.asarray(s.omega).copy()


@pytest.mark.parametrize("online", [False, True], ids=["density_tempered", "smc2"])
def test_samplers(ob, online):
    """NaN-free: SMC(..., missing=True) is the unflagged sampler bit for bit (theta, logZ, omega).  With the eight gaps of
    MR.GAPS40: every logZ_m is finite and the mean over m of exp(logZ_m - KF(theta_m)), KF the Kalman filter with skipped updates,
    is within 4 sample standard errors of 1"""
    y0 = ob.simulate(1, MR.README_LG, 40, 1998)[1]
    res = []
    for missing in (False, True):
        s = sampler(missing)
        res.append(run_sampler(s, y0, online))
        s.backend.close()
    for a, b in zip(*res):
        assert TP.same(a, b)
    y = MR.with_gaps(y0, MR.GAPS40)
    s = sampler(True)
    theta, logZ, _ = run_sampler(s, y, online)
    s.backend.close()
    assert np.all(np.isfinite(logZ)), logZ
    kf = np.array([MR.kalman_gaps([th[0], 1.0, th[1], th[2], 0.0, 1.0], y)[0] for th in theta])
    e = np.exp(logZ - kf)
    se = e.std(ddof=1) / np.sqrt(len(e))
    print("%s: mean exp(logZ_m - KF(theta_m)) = %.4f +- %.4f" % ("smc2" if online else "density_tempered", e.mean(), se))
    assert abs(e.mean() - 1.0) <= 4 * se, (e.mean(), se)


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------
def test_python_keyword(L, ob):
    """missing=True on bootstrap_filter (its _ steps read it from the handle behind x), particle_filter, log_likelihood and smoother
    is the flagged handle; without it a NaN kills the step; rb_smoother(missing=True) raises on a NaN; forecast is unaffected"""
    import sequential_monte_carlo_amd as smc
    model = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
    y = series(1, (0, 3, 4), length=12)
    r = MR.run_series(L, ob, 1, [MR.README_LG], 1000, 0, 7, y)
    x, w, logZ, lm, es = smc.log_likelihood(1000, y, model, seed=7, trace=True, missing=True)
    assert TP.same([logZ], r["logZ"]) and TP.same(lm, r["lm"][:, 0]) and TP.same(es, r["es"][:, 0]) and x._f.h.missing
    assert TP.same(np.asarray(x), r["snap"][0][0, 0]) and TP.same(np.asarray(w), r["snap"][1][0])
    f = smc.forecast(x, w, 3, seed=11)
    assert np.all(np.isfinite(f["mean"]))
    assert smc.log_likelihood(1000, y, model, seed=7)[2] == -np.inf
    for prop, kind in ((None, CR.NONE), (smc.OptimalProposal(), CR.OPTIMAL)):
        rp = MR.run_series(L, ob, 1, [MR.README_LG], 1000, 0, 7, y, kind=kind)
        if prop is None:
            x, w, l0 = smc.bootstrap_filter(1000, y[0], model, seed=7, missing=True)
        else:
            x, w, l0 = smc.particle_filter(1000, y[0], model, prop, seed=7, missing=True)
        ls = [l0]
        for t in range(1, len(y)):
            l, w, _ = smc.bootstrap_filter_(x, w, y[t], model) if prop is None else smc.particle_filter_(x, w, y[t], model, prop)
            ls.append(l)
        assert TP.same(ls, rp["lm"][:, 0]), (kind, ls, rp["lm"][:, 0])
    _, _, z, s = smc.smoother(1000, y, model, seed=7, missing=True)
    assert TP.same([z], r["logZ"]) and np.all(np.isfinite(s["mean"])) and np.all(s["ess"][[0, 3, 4]] == 1000.0)
    rb = smc.unobserved_components_stochastic_volatility(x0=3.0, gamma_eps=0.2, gamma_eta=0.2, log_sigma_eps=0.0, log_sigma_eta=0.0, marginal=True)
    yu = series(4, (2,), length=8)
    with pytest.raises(L.SmcError):
        smc.rb_smoother(300, yu, rb, paths=16, seed=7, missing=True)
    out = smc.rb_smoother(300, series(4, (), length=8), rb, paths=16, seed=7, missing=True)
    assert np.all(np.isfinite(out[3]["trend_mean"]))
    with pytest.raises(ValueError):
        smc.SMC(64, 8, lambda th: model, smc.product_distribution([smc.LogNormal()]), 1, 0.5, backend=smc.smc_samplers.HipBackend(), missing=True)
