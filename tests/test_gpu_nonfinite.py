"""Non-finite observations and out-of-domain parameter rows on every launch path (pytest -m gpu).

The tables are tests/nonfinite_inputs.py; tests/test_nonfinite_host.py shows on the CPU that the references used here (the
oracle, tests/composed_reference.py, the host twins) are well defined on them and states the contract.  Every comparison is exact:
same_nan for doubles (the NaN positions coincide, everything else is the same bits - x86 and the GPU produce NaNs of different
sign and payload), array_equal for the ancestors and the raw fixed-point weights.  The one place with bounds is the moments of
the summaries, which carry the bounds of tests/summary_reference.py as everywhere in the suite.

  a. observations: NaN, +inf, -inf at the first, a middle and the last step and twice in a row, on the first and the last shape
     of every launch path of tests/test_gpu_paths.py: smc_log_likelihood with and without traces, the step API after every step,
     smc_step_window / smc_step_commit on the resident shapes, systematic resampling
  b. rows: every bootstrap entry of BAD_ROWS in slot 0, 1, 2 of a batch of three == the oracle slot by slot; the healthy slots
     are bit-identical to the batch without the bad row; healthy rows on the same handle afterwards == a fresh handle
     (the UCSV_RB entries run against their own reference in c.)
  c. the guided handles and the marginal family against tests/composed_reference.py; the one-step device twins == the host twins
  d. per-step summaries, weighted and unweighted
  e. the record: smc_smooth, smc_sample_paths, smc_rb_sample_paths == their host twins
  f. density_tempered and the online sampler with a Normal prior on a variance: HipBackend == OracleBackend
  g. the Kalman likelihood and the IBIS window
"""
import functools
import io
import math

import numpy as np
import pytest

import composed_reference as CR
import nonfinite_inputs as NF
import quantile7_reference as Q7
import step_edge_inputs
import summary_reference as SR
import test_gpu_paths as TP
from nonfinite_inputs import first_diff, same_nan, same_slot

pytestmark = pytest.mark.gpu

T, NTH, SEED = NF.T, 3, 5
NO_RESIDENT = TP.NO_RESIDENT
SHAPES = []
for _pid, _cs in TP.PATHS.items():
    for _c in (_cs[0], _cs[-1]):
        SHAPES.append((_pid, _c))
SHAPE_IDS = ["%s-m%d-n%d" % (pid, c[0], c[1]) for pid, c in SHAPES]


def finite_series(model, seed=1998):
    from oracle import binding as ob
    m = NF.UCSV3D if model == NF.UCSV_RB else model
    return ob.simulate(m, NF.HEALTHY[m], T, seed)[1]


@functools.lru_cache(maxsize=24)
def oracle_walk(model, rawkey, n, seg, seed, stream, ykey, systematic=False):
    """the oracle step by step: [(logmu, ess, slot)] after every step; logZ is the running sum"""
    from oracle import binding as ob
    f = ob.Filter(model, np.array(rawkey), n, seg=seg, seed=seed, stream=stream, systematic=systematic)
    out, z = [], 0.0
    for t, y in enumerate(ykey):
        if t == 0:
            lm = f.bootstrap_filter(y)
            es = f.ess()
            z = lm
        else:
            lm, es = f.step(y)
            z = z + lm
        out.append((lm, es, z, TP.orc_slot(f)))
    return out


def walks(case, raws, y, seed=SEED, systematic=False):
    model, n, seg, _ = case
    yk = tuple(float(v) for v in y)
    return [oracle_walk(model, tuple(float(v) for v in raws[th]), n, seg, seed, th, yk, systematic) for th in range(len(raws))]


def assert_slots(h, ws, t, ctx):
    for th, d in enumerate(TP.dev_slots(h)):
        o = ws[th][t][3]
        assert same_slot(d, o), ctx + (th, "state after step", t, first_diff(d, o))


def check_series(h, case, raws, y, ctx, systematic=False):
    """smc_log_likelihood with traces, without traces, and the step API after every step, against the oracle's walk"""
    ws = walks(case, raws, y, systematic=systematic)
    nth, Tn = len(raws), len(y)
    elm = np.array([[ws[th][t][0] for th in range(nth)] for t in range(Tn)])
    ees = np.array([[ws[th][t][1] for th in range(nth)] for t in range(Tn)])
    ez = np.array([ws[th][-1][2] for th in range(nth)])
    h.reseed(SEED)
    z, lm, es = h.log_likelihood(y, trace=True)
    assert same_nan(z, ez), ctx + ("logZ", z, ez)
    assert same_nan(lm, elm), ctx + ("logmu trace", lm, elm)
    assert same_nan(es, ees), ctx + ("ess trace", es, ees)
    assert same_nan(h.logZ()[0], ez) and same_nan(h.logZ()[1], ees[-1]), ctx + ("smc_get_logZ",)
    assert_slots(h, ws, Tn - 1, ctx + ("traces",))
    h.reseed(SEED)
    z2 = h.log_likelihood(y)                                       # no traces: (logmu) from the totals alone (emit_from_totals)
    assert same_nan(z2, ez), ctx + ("logZ without traces", z2, ez)
    assert_slots(h, ws, Tn - 1, ctx + ("no traces",))
    h.reseed(SEED)
    l0 = h.init(float(y[0]))
    assert same_nan(l0, elm[0]) and same_nan(h.logZ()[1], ees[0]), ctx + ("smc_init", l0, elm[0])
    assert_slots(h, ws, 0, ctx + ("step API",))
    for t in range(1, Tn):
        l, e = h.step(float(y[t]))
        assert same_nan(l, elm[t]) and same_nan(e, ees[t]), ctx + ("smc_step", t, l, elm[t], e, ees[t])
        assert_slots(h, ws, t, ctx + ("step API",))
    assert same_nan(h.logZ()[0], ez), ctx + ("logZ of the step API",)
    return ws, elm, ees, ez


# ---- a. observations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", NF.BAD_Y, ids=NF.BAD_Y_IDS)
@pytest.mark.parametrize("pid,case", SHAPES, ids=SHAPE_IDS)
def test_bad_observations_on_every_path(L, ob, pid, case, bad):
    model = case[0]
    raws = TP.raws_for(model, NTH)
    y0 = finite_series(model)
    h = TP.make(L, pid, case, NTH, seed=SEED)
    for pos in NF.POSITIONS:
        y = NF.bad_series(y0, pos, bad)
        _, elm, _, ez = check_series(h, case, raws, y, (pid, case, bad, pos))
        dead = np.zeros(T, dtype=bool)
        dead[list(pos)] = True
        assert np.array_equal(np.isneginf(elm), np.repeat(dead[:, None], NTH, axis=1)) and np.all(ez == -np.inf)
    h.close()


@pytest.mark.parametrize("bad", NF.BAD_Y, ids=NF.BAD_Y_IDS)
@pytest.mark.parametrize("pid,case", [s for s in SHAPES if s[0] == "R"], ids=[i for s, i in zip(SHAPES, SHAPE_IDS) if s[0] == "R"])
def test_bad_observation_inside_a_step_window(L, ob, pid, case, bad):
    """init, then a window of four whose SECOND observation is bad, kept to j = 1, 2, 4: the window's (logmu, ess) and the state
    after the kept prefix are those of single steps / of the oracle; a window does not move the filters"""
    model = case[0]
    raws = TP.raws_for(model, NTH)
    y = NF.bad_series(finite_series(model)[:5], (2,), bad)       # y[1:5] is the window; its second entry is y[2]
    ws = walks(case, raws, y)
    h = TP.make(L, pid, case, NTH, seed=SEED)
    assert h.can_window
    for j in (1, 2, 4):
        ctx = (pid, case, bad, j)
        h.reseed(SEED)
        h.init(float(y[0]))
        before = TP.dev_slots(h)
        lm, es = h.step_window(y[1:5])
        for th, d in enumerate(TP.dev_slots(h)):
            assert same_nan(d[0], before[th][0]) and same_nan(d[1], before[th][1]), ctx + (th, "a window moved the filter")
        for i in range(4):
            assert same_nan(lm[i], [ws[th][1 + i][0] for th in range(NTH)]), ctx + ("window logmu", i)
            assert same_nan(es[i], [ws[th][1 + i][1] for th in range(NTH)]), ctx + ("window ess", i)
        h.step_commit(j)
        assert_slots(h, ws, j, ctx + ("after commit",))
        assert same_nan(h.logZ()[0], [ws[th][j][2] for th in range(NTH)]), ctx + ("logZ after commit",)
        g = TP.make(L, pid, case, NTH, seed=SEED)                  # == single steps
        g.init(float(y[0]))
        for t in range(1, j + 1):
            g.step(float(y[t]))
        for th, (d, s) in enumerate(zip(TP.dev_slots(h), TP.dev_slots(g))):
            assert same_slot(d, s), ctx + (th, "window + commit != single steps", first_diff(d, s))
        g.close()
    h.close()


@pytest.mark.parametrize("case", [(1, 1000, 0, 0), (3, 3000, 512, 0)], ids=["single-segment", "multi-segment"])
def test_bad_observations_with_systematic_resampling(L, ob, case):
    model = case[0]
    raws = TP.raws_for(model, NTH)
    h = L.Handle(model, NTH, case[1], seg=case[2], seed=SEED, flags=L.FLAG_SYSTEMATIC | L.FLAG_ANCESTORS)
    assert (h.nseg == 1) == (case[2] == 0)
    h.set_params(raws)
    for bad in NF.BAD_Y:
        y = NF.bad_series(finite_series(model), (2,), bad)
        check_series(h, case, raws, y, ("systematic", case, bad), systematic=True)
    h.close()


# ---- b. rows, and isolation inside a batch -------------------------------------------------------------------------------------
ROW_SHAPES = {
    NF.LG1D: (("R", (1, 1000, 0, 0)), ("S", (1, 1000, 0, NO_RESIDENT)), ("M1", (1, 5000, 1024, 0))),
    NF.SV1D: (("R", (2, 1000, 0, 0)), ("S", (2, 1000, 0, NO_RESIDENT)), ("M1", (2, 3000, 512, 0))),
    NF.UCSV3D: (("R", (3, 512, 0, 0)), ("S", (3, 512, 0, NO_RESIDENT)), ("M1", (3, 3000, 512, 0))),
}


def run_ll(h, y):
    h.reseed(SEED)
    z, lm, es = h.log_likelihood(y, trace=True)
    return z, lm, es, TP.dev_slots(h)


@pytest.mark.parametrize("rid,model,raw,tag", NF.BOOTSTRAP_ROWS, ids=[r[0] for r in NF.BOOTSTRAP_ROWS])
def test_bad_row_in_a_batch(L, ob, rid, model, raw, tag):
    y = finite_series(model)
    healthy = TP.raws_for(model, NTH)
    dead = NF.dead_steps(T, tag)
    for pid, case in ROW_SHAPES[model]:
        g = TP.make(L, pid, case, NTH, seed=SEED)                  # the batch without the bad row, on a handle of its own
        zg, lmg, esg, sg = run_ll(g, y)
        g.close()
        assert np.all(np.isfinite(zg))
        h = TP.make(L, pid, case, NTH, seed=SEED)
        for slot in range(NTH):
            ctx = (rid, pid, case, slot)
            raws = healthy.copy()
            raws[slot] = raw
            h.set_params(raws)
            ws = walks(case, raws, y)
            z, lm, es, sl = run_ll(h, y)
            for th in range(NTH):
                assert same_nan(z[th], ws[th][-1][2]), ctx + (th, "logZ", z[th], ws[th][-1][2])
                assert same_nan(lm[:, th], [w[0] for w in ws[th]]) and same_nan(es[:, th], [w[1] for w in ws[th]]), ctx + (th, "traces", lm[:, th])
                assert same_slot(sl[th], ws[th][-1][3]), ctx + (th, first_diff(sl[th], ws[th][-1][3]))
                if th != slot:                                     # the neighbours: the bits of the batch without the bad row
                    assert same_nan(z[th], zg[th]) and np.isfinite(z[th]), ctx + (th, "neighbour logZ")
                    assert same_nan(lm[:, th], lmg[:, th]) and same_nan(es[:, th], esg[:, th]), ctx + (th, "neighbour traces")
                    assert same_slot(sl[th], sg[th]), ctx + (th, "neighbour state", first_diff(sl[th], sg[th]))
            assert np.array_equal(np.isneginf(lm[:, slot]), dead) and (z[slot] == -np.inf) == bool(dead.any()), ctx + (lm[:, slot],)
        h.set_params(healthy)                                      # a dead filter leaves nothing behind on the handle
        z, lm, es, sl = run_ll(h, y)
        assert same_nan(z, zg) and same_nan(lm, lmg) and same_nan(es, esg), (rid, pid, "healthy rows after the bad ones")
        for th in range(NTH):
            assert same_slot(sl[th], sg[th]), (rid, pid, th, "healthy rows after the bad ones", first_diff(sl[th], sg[th]))
        h.close()


@pytest.mark.parametrize("rid,model,raw,tag", NF.BOOTSTRAP_ROWS, ids=[r[0] for r in NF.BOOTSTRAP_ROWS])
def test_bad_row_of_a_single_filter_step_by_step(L, ob, rid, model, raw, tag):
    """one filter per handle and one k_step launch per step: the launches take the filter's row by value (hot.prm0, the host's copy
    of row 0).  A bad row, then a healthy one, then the bad one again on the same handle - the step API after every step and the
    whole-series call - on one segment and on several"""
    y = finite_series(model)
    for pid, case in ROW_SHAPES[model][1:]:
        h = TP.make(L, pid, case, 1, seed=SEED)
        for row in (raw, NF.HEALTHY[model], raw):
            raws = np.array([row], dtype=np.float64)
            h.set_params(raws)
            assert h.step_by_value and not h.resident
            check_series(h, case, raws, y, (rid, pid, "single filter"))
        h.close()


# ---- c. guided and marginal filters ---------------------------------------------------------------------------------------------
def composed_shapes(model):
    if model == NF.LG1D:
        return ((1000, 0, 0), (1000, 0, NO_RESIDENT), (3000, 256, 0))
    return ((512, 0, 0), (512, 0, NO_RESIDENT), (3000, 256, 0))


def composed_rows(model, nth):
    r = np.tile(NF.HEALTHY[model], (nth, 1)).astype(float)
    r[:, 0] *= 1.0 - 0.3 * np.arange(nth) / nth
    return r


def guided_handle(L, fam, raws, n, seg, flags):
    model, kind, par = NF.COMPOSED[fam]
    h = L.Handle(model, len(raws), n, seg=seg, seed=SEED, flags=flags | L.FLAG_ANCESTORS)
    h.set_params(raws)
    if kind != NF.NONE:
        h.set_proposal(kind, par)
    return h


def check_composed(L, ob, h, fam, raws, n, seg, y, ctx):
    model, kind, par = NF.COMPOSED[fam]
    nth = len(raws)
    ref = CR.run_series(L, ob, model, raws, n, seg, SEED, y, kind=kind, pars=None if par is None else np.tile(par, (nth, 1)))
    assert (h.seg, h.nseg) == (ref["seg"], ref["nseg"])
    h.reseed(SEED)
    z, lm, es = h.log_likelihood(y, trace=True)
    assert same_nan(lm, ref["lm"]), ctx + ("logmu trace", lm, ref["lm"])
    assert same_nan(es, ref["es"]), ctx + ("ess trace", es, ref["es"])
    assert same_nan(z, ref["logZ"]), ctx + ("logZ", z, ref["logZ"])
    x, w, a = h.state()
    dev = (x, w, a) + tuple(h.weights_raw())
    for th in range(nth):
        d = tuple(dev[k][:, th] if k == 0 else dev[k][th] for k in range(8))
        o = tuple(ref["snap"][k][:, th] if k == 0 else ref["snap"][k][th] for k in range(8))
        assert same_slot(d, o), ctx + (th, first_diff(d, o))
    h.reseed(SEED)                                                 # ... and the step API
    l0 = h.init(float(y[0]))
    assert same_nan(l0, ref["lm"][0]), ctx + ("smc_init",)
    for t in range(1, len(y)):
        l, e = h.step(float(y[t]))
        assert same_nan(l, ref["lm"][t]) and same_nan(e, ref["es"][t]), ctx + ("smc_step", t, l, ref["lm"][t])
    return ref


@pytest.mark.parametrize("fam", ["lg-affine", "lg-optimal", "uc-optimal", "rb"])
def test_guided_and_marginal_filters_on_bad_observations(L, ob, fam):
    model = NF.COMPOSED[fam][0]
    raws = composed_rows(model, NTH)
    y0 = finite_series(model)
    for n, seg, flags in composed_shapes(model):
        h = guided_handle(L, fam, raws, n, seg, flags)
        for bad in NF.BAD_Y:
            for pos in ((0,), (2,), (2, 3)):
                ref = check_composed(L, ob, h, fam, raws, n, seg, NF.bad_series(y0, pos, bad), (fam, n, seg, flags, bad, pos))
                dead = NF.dead_steps(T, NF.composed_y_tag(fam, pos))
                assert np.array_equal(np.isneginf(ref["lm"]), np.repeat(dead[:, None], NTH, axis=1)), (fam, bad, pos, ref["lm"])
        h.close()


@pytest.mark.parametrize("fam", ["lg-affine", "lg-optimal", "uc-optimal", "rb"])
def test_guided_and_marginal_filters_on_bad_rows(L, ob, fam):
    model = NF.COMPOSED[fam][0]
    healthy = composed_rows(model, NTH)
    y = finite_series(model)
    for n, seg, flags in composed_shapes(model):
        h = guided_handle(L, fam, healthy, n, seg, flags)
        base = check_composed(L, ob, h, fam, healthy, n, seg, y, (fam, n, seg, flags, "healthy"))
        for k, (rid, _, raw, tag) in enumerate(NF.rows_of(model)):
            slot = k % NTH
            raws = healthy.copy()
            raws[slot] = raw
            h.set_params(raws)
            ref = check_composed(L, ob, h, fam, raws, n, seg, y, (fam, n, seg, flags, rid, slot))
            dead = NF.dead_steps(T, NF.composed_row_tag(fam, rid, tag))
            assert np.array_equal(np.isneginf(ref["lm"][:, slot]), dead), (fam, rid, ref["lm"][:, slot])
            for th in range(NTH):
                if th != slot:
                    assert same_nan(ref["lm"][:, th], base["lm"][:, th]) and np.isfinite(ref["logZ"][th])
        h.set_params(healthy)
        check_composed(L, ob, h, fam, healthy, n, seg, y, (fam, n, seg, flags, "healthy again"))
        h.close()


@pytest.mark.parametrize("fam", ["lg-affine", "lg-optimal", "uc-optimal"])
def test_device_guided_twin_on_extended_edge_inputs(L, fam):
    model, kind, _ = NF.COMPOSED[fam]
    raw, par, xp0, z, y0 = step_edge_inputs.guided(model, kind)
    xp, _ = NF.plant(xp0)
    for y in (y0,) + NF.BAD_Y:
        x, lw = L.device_guided_step(model, raw, kind, par, xp, z, y)
        hx, hl = L.host_guided_steps(model, raw, kind, par, xp, z, y)
        bad = [i for i in range(xp.shape[1]) if not (same_nan(x[:, i], hx[:, i]) and same_nan(lw[i], hl[i]))]
        assert not bad, (fam, y, bad[:5], x[:, bad[0]], hx[:, bad[0]], lw[bad[0]], hl[bad[0]], xp[:, bad[0]], z[:, bad[0]])


@pytest.mark.parametrize("first", [False, True])
def test_device_rb_twin_on_extended_edge_inputs(L, first):
    raw, sp0, z, y0 = step_edge_inputs.rb(first)
    sp, _ = NF.plant(sp0, variance_row=3)
    for y in (y0,) + NF.BAD_Y:
        s, lw = L.device_rb_step(raw, sp, z, y, first)
        hs, hl = L.host_rb_steps(raw, sp, z, y, first)
        bad = [i for i in range(sp.shape[1]) if not (same_nan(s[:, i], hs[:, i]) and same_nan(lw[i], hl[i]))]
        assert not bad, (first, y, bad[:5], s[:, bad[0]], hs[:, bad[0]], lw[bad[0]], hl[bad[0]], sp[:, bad[0]], z[:, bad[0]])


# ---- d. summaries ---------------------------------------------------------------------------------------------------------------
PS = [0.25, 0.5, 0.75]
SUMMARY_SHAPES = (("R", (1, 1000, 0, 0)), ("M1", (1, 5000, 1024, 0)))


def oracle_clouds(case, raws, y):
    """[th][t] -> (x [d][n], w [n]) of the oracle after every step"""
    return [[(w[3][0], w[3][1]) for w in ws] for ws in walks(case, raws, y)]


@pytest.mark.parametrize("which", ["bad-y", "bad-row"])
@pytest.mark.parametrize("mode", ["weighted", "unweighted"])
@pytest.mark.parametrize("pid,case", SUMMARY_SHAPES, ids=[s[0] for s in SUMMARY_SHAPES])
def test_summaries(L, ob, pid, case, mode, which):
    """quantiles [0.25, 0.5, 0.75] and moments recorded inside smc_log_likelihood, read once after the run.  Weighted: NaN rows
    exactly at the dead steps; elsewhere the oracle's quantiles bit for bit and the moments within tests/summary_reference.py.
    Unweighted: the type-7 quantiles of tests/quantile7_reference.py bit for bit on the cloud (a collapsed filter has ordinary,
    finite ones; a cloud of NaN states has NaN quantiles, mean and variance), the moments within the same bounds."""
    from oracle import binding as ob_
    model, n, seg, _ = case
    raws = TP.raws_for(model, NTH)
    y = finite_series(model)
    if which == "bad-y":
        y = NF.bad_series(y, (2,), NF.NAN)
        dead = np.zeros((T, NTH), dtype=bool)
        dead[2] = True
    else:
        raws[1] = NF.BAD_ROWS[0][2]                                # lg-Q<0: dead from step 1 on, every state NaN
        dead = np.zeros((T, NTH), dtype=bool)
        dead[1:, 1] = True
    clouds = oracle_clouds(case, raws, y)
    h = TP.make(L, pid, case, NTH, seed=SEED)
    h.set_params(raws)
    h.set_summary_mode(mode)
    h.set_summaries(PS, 0, moments=True)
    h.reseed(SEED)
    _, lm, _ = h.log_likelihood(y, trace=True)
    q, mean, var = h.get_summaries(T)
    assert np.array_equal(np.isneginf(lm), dead)
    for th in range(NTH):
        f = ob_.Filter(model, raws[th], n, seg=seg, seed=SEED, stream=th)
        for t in range(T):
            f.bootstrap_filter(float(y[0])) if t == 0 else f.step(float(y[t]))
            ctx = (pid, mode, which, th, t)
            x, w = clouds[th][t]
            assert same_nan(f.state()[0], x)
            if mode == "weighted":
                assert np.isnan(q[t, th]).all() == bool(dead[t, th]) and np.isnan(mean[t, 0, th]) == bool(dead[t, th]), ctx + (q[t, th],)
                assert same_nan(q[t, th], f.quantiles(PS)), ctx + (q[t, th], f.quantiles(PS))
                SR.check_quantiles(q[t, th], PS, x[0], w, SR.quantile_delta(n, h.nseg, h.seg, math.fsum(w)), ctx)
                SR.check_moments(mean[t, 0, th], var[t, 0, th], x[0], w, ctx)
            elif np.isnan(x[0]).all():                             # the contract of a NaN cloud (tests/test_nonfinite_host.py)
                assert np.isnan(q[t, th]).all() and np.isnan(mean[t, 0, th]) and np.isnan(var[t, 0, th]), ctx + (q[t, th], mean[t, 0, th])
            else:
                assert np.all(np.isfinite(x[0]))
                assert Q7.same_bits(q[t, th], Q7.quantile7(x[0], PS)), ctx + (q[t, th], Q7.quantile7(x[0], PS))
                assert Q7.same_bits(q[t, th], L.host_quantile7(x[0], PS)), ctx
                Q7.check_sample_moments(mean[t, 0, th], var[t, 0, th], x[0], ctx)
    h.close()


@pytest.mark.parametrize("pid,case", SUMMARY_SHAPES, ids=[s[0] for s in SUMMARY_SHAPES])
def test_unweighted_summaries_of_a_partly_nan_cloud(L, ob, pid, case):
    """lg-Q=inf in slot 1: from the second step on its cloud holds NaN next to +inf and -inf (inf - inf where the signs differ).
    The README loop in unweighted mode - smc_get_quantiles / smc_get_moments after every step - against the references on the
    cloud the DEVICE holds (the sign bit of its NaNs decides where they sort): quantiles NaN-aware and bit for bit, NaN mean and
    variance; the neighbours have ordinary summaries"""
    model, n, seg, _ = case
    raws = TP.raws_for(model, NTH)
    raws[1] = dict((r[0], r[2]) for r in NF.BAD_ROWS)["lg-Q=inf"]
    y = finite_series(model)
    ws = walks(case, raws, y)
    h = TP.make(L, pid, case, NTH, seed=SEED)
    h.set_params(raws)
    h.set_summary_mode("unweighted")
    h.reseed(SEED)
    mixed = 0
    for t in range(T):
        h.init(float(y[0])) if t == 0 else h.step(float(y[t]))
        xd = h.state()[0]
        q = h.quantiles(PS)
        mean, var = h.moments()
        for th in range(NTH):
            ctx = (pid, th, t)
            c = xd[0, th]
            assert same_nan(c, ws[th][t][3][0][0]), ctx
            assert same_nan(q[th], Q7.quantile7(c, PS)) and same_nan(q[th], L.host_quantile7(c, PS)), ctx + (q[th], Q7.quantile7(c, PS))
            if np.all(np.isfinite(c)):
                assert th != 1 or t == 0
                Q7.check_sample_moments(mean[0, th], var[0, th], c, ctx)
            else:
                assert th == 1 and np.isinf(c).any(), ctx                  # (+inf and -inf at t = 1, NaN next to them from t = 2 on)
                assert np.isnan(mean[0, th]) and np.isnan(var[0, th]), ctx + (mean[0, th], var[0, th])
                mixed += 1
    assert mixed == T - 1 and np.isnan(xd[0, 1]).any()
    h.close()


# ---- e. the record ----------------------------------------------------------------------------------------------------------------
def recorded_run(L, model, raws, y, n=300, seg=256):
    h = L.Handle(model, len(raws), n, seg=seg, seed=SEED, flags=L.FLAG_ANCESTORS)
    h.set_params(raws)
    h.history_begin(len(y))
    h.init(float(y[0]))
    for t in range(1, len(y)):
        h.step(float(y[t]))
    assert h.history_len() == len(y)
    rec = [h.history_get(t) for t in range(len(y))]
    return h, np.stack([r[0] for r in rec]), np.stack([r[1] for r in rec])        # x [T][d][nth][n], w [T][nth][n]


def check_record(L, h, model, raws, xs, ws, dead_filters, ctx, M=64):
    sw, mean, var = h.smooth()
    idx, px = h.sample_paths(M, 17)
    for th in range(len(raws)):
        hw, hm, hv = L.host_smooth(model, raws[th], xs[:, :, th], ws[:, th])
        assert same_nan(sw[:, th], hw) and same_nan(mean[:, :, th], hm) and same_nan(var[:, :, th], hv), ctx + (th, "smc_smooth")
        hi, hx = L.host_sample_paths(model, raws[th], xs[:, :, th], ws[:, th], M, 17, stream=th)
        assert np.array_equal(idx[:, th], hi) and same_nan(px[:, :, th], hx), ctx + (th, "smc_sample_paths")
        if th in dead_filters:
            assert np.isnan(sw[:, th]).all() and np.isnan(mean[:, :, th]).all() and np.all(idx[:, th] == -1) and np.isnan(px[:, :, th]).all(), ctx + (th,)
        else:
            assert np.all(np.isfinite(sw[:, th])) and np.all(idx[:, th] >= 0), ctx + (th,)
    return sw, mean, var, idx, px


def test_record_with_a_bad_observation(L, ob):
    """a step-by-step run under smc_history_begin whose third observation is NaN: every filter of the batch collapsed at a
    recorded step, so its smoothed weights and moments are NaN and its paths -1 / NaN at every step (include/smc_hip.h) - on the
    device as by the host twins, and whatever the finite states of the record hold"""
    for model in (NF.LG1D, NF.UCSV3D):
        raws = TP.raws_for(model, NTH)
        y = NF.bad_series(finite_series(model), (2,), NF.NAN)
        h, xs, ws = recorded_run(L, model, raws, y)
        assert np.all(ws[2] == 0) and np.all(np.isfinite(xs))
        check_record(L, h, model, raws, xs, ws, {0, 1, 2}, ("bad y", model))
        h.close()


def test_record_with_a_dead_filter_in_the_batch(L, ob):
    """lg-R<0 in slot 1 (dead from the first step; its transition scale Q is valid, so the smoother accepts the row): NaN / -1
    for it, and for its neighbours the bits of the batch without it.  A row whose transition scale is not a positive finite
    number (lg-Q<0) is refused by smc_smooth and smc_sample_paths with SMC_EINVAL, as the header says, and the handle stays
    usable."""
    model = NF.LG1D
    y = finite_series(model)
    healthy = TP.raws_for(model, NTH)
    g, xg, wg = recorded_run(L, model, healthy, y)
    base = check_record(L, g, model, healthy, xg, wg, set(), ("healthy",))
    g.close()
    raws = healthy.copy()
    raws[1] = dict((r[0], r[2]) for r in NF.BAD_ROWS)["lg-R<0"]
    h, xs, ws = recorded_run(L, model, raws, y)
    got = check_record(L, h, model, raws, xs, ws, {1}, ("lg-R<0",))
    for th in (0, 2):
        for k, (a, b) in enumerate(zip(got, base)):
            u, v = (a[:, th], b[:, th]) if k in (0, 3) else (a[:, :, th], b[:, :, th])
            assert np.array_equal(u, v) if u.dtype.kind == "i" else same_nan(u, v), ("neighbour", th, k)
    raws[1] = NF.BAD_ROWS[0][2]                                    # lg-Q<0
    h.set_params(raws)
    with pytest.raises(L.SmcError):
        h.smooth()
    with pytest.raises(L.SmcError):
        h.sample_paths(8, 17)
    h.set_params(healthy)                                          # (the record is that of the lg-R<0 run: filter 1 is still dead)
    check_record(L, h, model, healthy, xs, ws, {1}, ("after the refusal",))
    h.close()


def test_rb_record_with_a_bad_observation(L, ob):
    """smc_rb_sample_paths on the record of a marginal handle that was stepped with a NaN third observation; the call's own y is
    finite: every filter collapsed at a recorded step, -1 / NaN everywhere, as smc_host_rb_sample_paths"""
    raws = composed_rows(NF.UCSV_RB, NTH)
    y0 = finite_series(NF.UCSV_RB)
    h, xs, ws = recorded_run(L, NF.UCSV_RB, raws, NF.bad_series(y0, (2,), NF.NAN))
    assert np.all(ws[2:] == 0) and np.isnan(xs[2:, 0]).all()
    r = h.rb_sample_paths(y0, 32, 19, draws=True)
    for th in range(NTH):
        o = L.host_rb_sample_paths(raws[th], xs[:, :, th], ws[:, th], y0, 32, 19, stream=th)
        assert np.array_equal(r["idx"][:, th], o["idx"]) and np.all(o["idx"] == -1)
        for key in ("vol", "tmean", "tvar", "tdraw", "out"):
            u = r[key][:, :, th] if key == "vol" else r[key][:, th]
            assert same_nan(u, o[key]), (th, key, u, o[key])
    h.close()


# ---- f. samplers that reach invalid rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("online", [False, True], ids=["density_tempered", "online"])
def test_samplers_with_a_normal_prior_on_a_variance(ob, online):
    import sequential_monte_carlo_amd as smc
    from oracle_backend import OracleBackend
    so, to, ro, reco, theta0 = NF.run_sampler(OracleBackend(), online, replay=ob)
    NF.sampler_conditions(reco, theta0)                            # on the reference side; the seed was chosen on the CPU
    NF.sampler_properties(so, reco)
    sh, th, rh, rech, theta0h = NF.run_sampler(smc.smc_samplers.HipBackend(), online)
    assert np.array_equal(theta0, theta0h)
    NF.sampler_properties(sh, rech)
    assert th == to and "[rejuvenating]" in th
    assert same_nan(sh.theta, so.theta) and same_nan(sh.logZ, so.logZ) and same_nan(sh.omega, so.omega)
    assert sh.psteps == so.psteps and sh.psteps_skipped == so.psteps_skipped
    assert {k: rech[k] for k in ("moves", "accepted")} == {k: reco[k] for k in ("moves", "accepted")}
    if online:
        assert same_nan(rh[0], ro[0]) and same_nan(rh[1], ro[1])
    else:
        assert rh == ro
    sh.backend.close()


def test_marginal_sampler_with_a_normal_prior_on_the_gammas(L):
    """UCSV_RB with Normal(0.2, 0.3) on both gammas: about a quarter of the draws are negative.  The sign of a gamma only flips a
    normal, so nothing dies and nothing is skipped (the support is the whole line): every logZ is finite, and the same seed gives
    the same bits twice"""
    import sequential_monte_carlo_amd as smc
    u = smc.UCSV((0.2, 0.2), 3.0, (0.0, 0.0))
    _, y = smc.simulate(u, 20, seed=1998)
    tmap = smc.ThetaMap(NF.UCSV_RB, [0, 1, -1, -1, -1], [0.0, 0.0, 3.0, 0.0, 0.0])
    runs = []
    for _ in range(2):
        b = smc.smc_samplers.HipBackend()
        prior = smc.product_distribution([smc.Normal(0.2, 0.3), smc.Normal(0.2, 0.3)])
        s = smc.SMC(256, 24, lambda t: smc.MarginalUCSV((t[0], t[1]), 3.0, (0.0, 0.0)), prior, 2, 0.95, seed=3, backend=b, theta_map=tmap)
        assert s.device_pmmh and np.any(s.theta < 0) and np.any(np.all(s.theta > 0, axis=1))
        stages = smc.density_tempered(s, y, verbose=False, out=io.StringIO())
        assert np.all(np.isfinite(s.logZ)) and s.psteps_skipped == 0 and stages[-1][0] == 1.0
        assert any(st[2] is not None for st in stages), stages
        runs.append((s.theta.copy(), s.logZ.copy(), s.omega.copy()))
        b.close()
    assert np.any(runs[0][0] < 0)                                  # negative gammas survive: they are as good as positive ones
    for u_, v_ in zip(*runs):
        assert np.array_equal(u_.view(np.uint64), v_.view(np.uint64))


# ---- g. Kalman inside ---------------------------------------------------------------------------------------------------------------
def test_kalman_likelihood_on_bad_rows_and_observations(L, ob):
    y0 = finite_series(NF.LG1D)
    rows = np.array([NF.LG] + [r[2] for r in NF.rows_of(NF.LG1D)], dtype=np.float64)
    series = [y0] + [NF.bad_series(y0, pos, bad) for bad in NF.BAD_Y for pos in NF.POSITIONS]
    for y in series:
        for pf in (False, True):
            out = np.asarray(L.kalman_log_likelihood(rows, y, pf)).reshape(len(rows), 3)
            for k, raw in enumerate(rows):
                ref = ob.kalman_log_likelihood(raw, y, pf)
                assert same_nan(out[k], ref), (k, raw, y, pf, out[k], ref)
            if not np.all(np.isfinite(y)):
                assert not np.isfinite(out[:, 2]).any()


@pytest.mark.parametrize("M", [77, 513])
def test_ibis_window_with_a_bad_observation(M):
    """smc_ibis_window over a window whose second observation is bad: the records == smc_host_outer_window on the lik the call
    returned, smc_ibis_window_ess == the host walk on those records; then the same from the committed state"""
    import test_gpu_ibis as TI
    from sequential_monte_carlo_amd import _lib as L
    y0 = TI._y(12)
    for bad in NF.BAD_Y:
        ib = TI._ibis("readme", M, False, 11)
        h = ib._handle()
        lo = 0
        for k, keep in ((4, 1), (4, 4), (3, 3)):
            y = NF.bad_series(y0[lo:lo + k], (1,), bad)
            logw = ib.logw
            rec, lik = h.window(y, want_lik=True)
            assert rec.shape == (k, (M + 7) // 8, 4)
            assert np.array_equal(rec, L.host_outer_window(logw, lik)), (M, bad, lo, "records")
            assert not np.isfinite(lik[1]).any()
            for ess_min in (0.0, M / 2.0):
                ess, j = h.window_ess(y, ess_min)
                ref, jr = L.host_outer_walk(rec, M, ess_min)
                assert j == jr and same_nan(ess, ref), (M, bad, lo, ess_min, ess, ref)
            rec2, _ = h.window(y, want_lik=True)
            assert np.array_equal(rec2, rec)
            h.commit(keep)
            adv = L.host_outer_advance(logw, np.zeros(M), lik, keep)[0]
            assert same_nan(ib.logw, adv), (M, bad, lo, "logw after commit")
            lo += keep
        ib.close()
