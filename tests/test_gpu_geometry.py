"""Every launch geometry of every kernel object against the oracle (pytest -m gpu), bit for bit: == on the uint64 view of every
double, array_equal for ancestors and the raw fixed-point weights.  No tolerances, except the moments and weighted quantiles of the
per-step summaries, which carry the bounds of tests/summary_reference.py / tests/quantile7_reference.py as everywhere.

The cases come from tests/geometry_cases.py (tests/test_geometry_cases_host.py checks their coverage on the CPU).  Every handle is
created under SMC_NP resp. launched under SMC_RES_NP and asserts the geometry (Handle.launch_geometry) and the launch path it names.

  1. the step kernels: k_init, k_step / k_step_miss / k_step_cond at the 13 geometries in shapes S, M1, M2, G; multinomial,
     systematic, by value and through the view
  2. at 256 threads and fewer: degenerate weights in M2 and G, the step API with a permutation, smc_copy_from between handles of
     different np, a handle on the recycled bundle of another geometry
  3. k_forecast at the 13 geometries
  4. the LDS-resident whole-series and window kernels under SMC_RES_NP
  5. the n_theta rule of resident_np without any knob

References (all independent of the geometry): ob.Filter for plain LG1D / SV1D / UCSV3D, composed_reference for the marginal UCSV
family and the guided filters, missing_reference for flagged handles, conditional_reference for conditional ones.
"""
import math

import numpy as np
import pytest

import composed_reference as CR
import conditional_reference as CF
import geometry_cases as GC
import missing_reference as MR
import test_gpu_forecast as TF
import test_gpu_paths as TP
from quantile7_reference import check_sample_moments, quantile7, same_bits
from summary_reference import check_moments, check_quantiles, quantile_delta

pytestmark = pytest.mark.gpu

SEED = 5
POOR = [0.3, 0.2, 0.1, 2.0]
same = TP.same


def base(model):
    return 3 if model == 4 else model


def raws_for(model, nth):
    return TP.raws_for(base(model), nth)


def series(model, T, seed=1998):
    from oracle import binding as ob
    return ob.simulate(base(model), TP.RAW[base(model)], T, seed)[1]


def gap_series(model, T):
    """the two series of a flagged handle: a gap inside, and a missing first observation (the only launch of the missing init)"""
    y = series(model, T)
    return MR.with_gaps(y, (T - 2,)), MR.with_gaps(y, (0,))


def pars_for(kind, nth):
    return np.tile(POOR, (nth, 1)) if kind == GC.AFFINE else None


def flags_of(L, variant, systematic=False, no_resident=False):
    f = L.FLAG_ANCESTORS | (L.FLAG_SYSTEMATIC if systematic else 0) | (L.FLAG_NO_RESIDENT if no_resident else 0)
    if variant in ("missing", "missing_guided"):
        f |= L.FLAG_NAN_MISSING
    if variant == "cond":
        f |= L.FLAG_CONDITIONAL
    return f


def snap(h):
    return h.state() + h.weights_raw()


def make(L, monkeypatch, variant, model, kind, threads, k, n, nth, shape, systematic=False, seed=SEED, by_value=None):
    """a handle of (threads, k) on the path `shape`, asserting both"""
    monkeypatch.setenv("SMC_NP", str(k))
    if by_value is False:
        monkeypatch.setenv("SMC_STEP_BY_VALUE", "0")
    else:
        monkeypatch.delenv("SMC_STEP_BY_VALUE", raising=False)
    seg = GC.seg_of(threads, k)
    h = L.Handle(model, nth, n, seg=seg, seed=seed, flags=flags_of(L, variant, systematic, shape == "S"))
    ctx = (variant, model, threads, k, shape, n)
    assert h.launch_geometry()[:2] == (threads, k), ctx + (h.launch_geometry(),)
    assert h.seg == seg and GC.shape_of(n, h.seg, threads, not h.resident) == shape, ctx + (h.seg, h.nseg, h.resident)
    assert h.nseg == -(-n // seg)
    h.set_params(raws_for(model, nth))
    if kind != GC.NONE:
        h.set_proposal(kind, pars_for(kind, nth))
    if by_value is not None:
        assert h.step_by_value == by_value, ctx
    return h


def reference(L, ob, variant, model, kind, n, seg, nth, y, systematic=False, every=False):
    """dict(lm [T][nth], es, logZ [nth], snap) of the series on a handle made by make()"""
    raws = raws_for(model, nth)
    if variant in ("missing", "missing_guided"):
        return MR.run_series(L, ob, model, raws, n, seg, SEED, y, kind=kind, pars=pars_for(kind, nth), systematic=systematic, every=every)
    if variant == "guided" or model == 4:
        return CR.run_series(L, ob, model, raws, n, seg, SEED, y, kind=kind, pars=pars_for(kind, nth), systematic=systematic)
    assert variant == "plain"
    T = len(y)
    lm, es, logZ, snaps = np.zeros((T, nth)), np.zeros((T, nth)), np.zeros(nth), []
    for th in range(nth):
        f = ob.Filter(model, raws[th], n, seg=seg, seed=SEED, stream=th, systematic=systematic)
        logZ[th], lm[:, th], es[:, th] = f.log_likelihood(y, trace=True)
        snaps.append(TP.orc_slot(f))
    return dict(lm=lm, es=es, logZ=logZ, snap=CR.stack(snaps))


def first_filter(r):
    """the reference of filter 0 alone (raws_for gives it the same row whatever the batch)"""
    return dict(lm=r["lm"][:, :1], es=r["es"][:, :1], logZ=r["logZ"][:1], snap=tuple(a[:, :1] if k == 0 else a[:1] for k, a in enumerate(r["snap"])))


def check_ll(h, y, r, ctx):
    """smc_log_likelihood with traces against the reference, then without traces: the same logZ and state"""
    h.reseed(SEED)
    z, lm, es = h.log_likelihood(y, trace=True)
    assert same(z, r["logZ"]) and same(lm, r["lm"]) and same(es, r["es"]), ctx + ("traces", z, r["logZ"])
    assert CR.first_mismatch(snap(h), r["snap"]) is None, ctx + ("traces", CR.first_mismatch(snap(h), r["snap"]))
    h.reseed(SEED)
    z0 = h.log_likelihood(y)
    assert same(z0, r["logZ"]), ctx + ("no traces", z0, r["logZ"])
    assert CR.first_mismatch(snap(h), r["snap"]) is None, ctx + ("no traces", CR.first_mismatch(snap(h), r["snap"]))


def xrefs_for(model, nth, T):
    import test_gpu_conditional as TC
    return TC.references(model, nth, T)


def check_cond(L, ob, h, c, ctx):
    """the conditional filter: one launch per step, every step's logmu, ess, state, ancestors and raw weights"""
    y, xref = series(c.model, c.T), xrefs_for(c.model, c.nth, c.T)
    r = CF.run_series(L, ob, c.model, raws_for(c.model, c.nth), c.n, c.seg, SEED, y, xref)
    assert h.conditional and (h.seg, h.nseg) == (r["seg"], r["nseg"])
    h.set_reference(xref)
    for t in range(c.T):
        lm, es = (h.init(float(y[0])), h.logZ()[1]) if t == 0 else h.step(float(y[t]))
        assert same(lm, r["lm"][t]) and same(es, r["es"][t]), ctx + (t, lm, r["lm"][t])
        assert CF.first_mismatch(snap(h), r["snaps"][t]) is None, ctx + (t, CF.first_mismatch(snap(h), r["snaps"][t]))


def run_case(L, ob, monkeypatch, c, refs):
    """one case of geometry_cases.step_cases(); refs: the references of the function's cases, shared between modes"""
    ctx = tuple(c)
    sysm = c.mode == "sys"
    if c.variant == "cond":
        h = make(L, monkeypatch, c.variant, c.model, c.kind, c.threads, c.np, c.n, c.nth, c.shape)
        check_cond(L, ob, h, c, ctx)
        h.close()
        return
    ys = gap_series(c.model, c.T) if c.variant in ("missing", "missing_guided") else (series(c.model, c.T),)
    # by value (one filter, STEP_BYV) or through the view; the large shapes of one filter run both below 2^19 particles
    if c.nth == 1 and GC.STEP_BYV[c.variant]:
        ways = (True, False) if c.mode == "one" and c.n <= (1 << 19) else (True,)
    else:
        ways = (None,)
    for way in ways:
        h = make(L, monkeypatch, c.variant, c.model, c.kind, c.threads, c.np, c.n, c.nth, c.shape, systematic=sysm, by_value=way)
        assert c.nth == 1 or not h.step_by_value
        for j, y in enumerate(ys):
            key = (c.variant, c.model, c.kind, c.n, c.seg, sysm, j)
            if key not in refs:
                refs[key] = reference(L, ob, c.variant, c.model, c.kind, c.n, c.seg, 2 if c.shape in ("S", "M1") else 1, y, systematic=sysm)
            r = refs[key]
            check_ll(h, y, first_filter(r) if c.nth == 1 and r["lm"].shape[1] > 1 else r, ctx + (way, j))
        h.close()


# ---- 1. the step kernels ------------------------------------------------------------------------------------------------------------
CASES = GC.step_cases()
OBJECT_IDS = ["%s.%d" % o for o in GC.OBJECTS]


@pytest.mark.parametrize("variant,model", GC.OBJECTS, ids=OBJECT_IDS)
def test_one_segment_and_three_segments(L, ob, monkeypatch, variant, model):
    """shapes S and M1 of one object at all 13 geometries: multinomial and systematic with two filters of distinct rows, one filter
    by value; a flagged handle runs a series with a gap inside and one whose first observation is missing"""
    refs = {}
    mine = [c for c in CASES if (c.variant, c.model) == (variant, model) and c.shape in ("S", "M1")]
    assert {(c.threads, c.np) for c in mine} == set(GC.GEOMETRIES)
    for c in mine:
        run_case(L, ob, monkeypatch, c, refs)


SMALL = [(v, m, s) for v, m in GC.OBJECTS if v != "missing_guided" for s in ("M2", "G")]


@pytest.mark.parametrize("variant,model,shape", SMALL, ids=["%s.%d-%s" % x for x in SMALL])
def test_two_records_and_global_table_up_to_256_threads(L, ob, monkeypatch, variant, model, shape):
    """shapes M2 (two records per thread) and G (k_table, k_step<..., GTAB>) at the seven geometries of at most 256 threads"""
    refs = {}
    mine = [c for c in CASES if (c.variant, c.model, c.shape) == (variant, model, shape) and c.threads <= 256]
    assert len(mine) == 7 - sum(1 for u in GC.UNREACHABLE if u[:2] == (variant, model) and u[4] == shape and u[2] <= 256)
    for c in mine:
        run_case(L, ob, monkeypatch, c, refs)


LARGE = [c for c in CASES if c.shape in ("M2", "G") and c.threads >= 512]


@pytest.mark.parametrize("c", LARGE, ids=["%s.%d-%dx%d-%s" % (c.variant, c.model, c.threads, c.np, c.shape) for c in LARGE])
def test_two_records_and_global_table_from_512_threads(L, ob, monkeypatch, c):
    """... at 512 and 1024 threads, for the objects geometry_cases keeps there (the oracle's CPU cost; the exclusions are listed)"""
    run_case(L, ob, monkeypatch, c, {})


# ---- 2. at 256 threads and fewer ----------------------------------------------------------------------------------------------------
UP_TO_256 = [g for g in GC.GEOMETRIES if g[0] <= 256]


@pytest.mark.parametrize("shape", ["M2", "G"])
def test_degenerate_weights(L, ob, monkeypatch, shape):
    """the sharp LG1D row of test_gpu_parity.py::test_uneven_weights_far_segments (R = 1e-4, sigma0 = 4): a workgroup's children span
    more segments than it stages, the searches leave the staged window"""
    raw = [0.9, 1.0, 1.0, 1e-4, 0.0, 4.0]
    y = ob.simulate(1, [0.9, 1.0, 1.0, 0.5, 0.0, 4.0], 4, 7)[1]
    for threads, k in UP_TO_256:
        n, seg = GC.n_of(shape, threads, k), GC.seg_of(threads, k)
        h = make(L, monkeypatch, "plain", 1, GC.NONE, threads, k, n, 1, shape)
        h.set_params(raw)
        z, lm, es = h.log_likelihood(y, trace=True)
        assert es.min() < 0.02 * n                                       # the weights really are degenerate
        f = ob.Filter(1, raw, n, seg=seg, seed=SEED, stream=0)
        oz, olm, oes = f.log_likelihood(y, trace=True)
        assert same(z, [oz]) and same(lm[:, 0], olm) and same(es[:, 0], oes), (shape, threads, k)
        assert CR.first_mismatch(snap(h), CR.stack([TP.orc_slot(f)])) is None, (shape, threads, k)
        h.close()


@pytest.mark.parametrize("shape", ["M2", "G"])
def test_step_api_with_a_permutation(L, ob, monkeypatch, shape):
    """init, two steps, smc_permute (slot 0 becomes a value copy of slot 1), two more steps"""
    y = series(1, 5, seed=4)
    for threads, k in UP_TO_256:
        n, seg = GC.n_of(shape, threads, k), GC.seg_of(threads, k)
        h = make(L, monkeypatch, "plain", 1, GC.NONE, threads, k, n, 2, shape, seed=21)
        raws = raws_for(1, 2)
        fs = [ob.Filter(1, raws[th], n, seg=seg, seed=21, stream=th) for th in range(2)]
        assert same(h.init(float(y[0])), [f.bootstrap_filter(float(y[0])) for f in fs])
        for t in range(1, 5):
            if t == 3:
                h.permute(np.array([1, 1], dtype=np.int32))
                fs[0].copy_state_from(fs[1])
            lm, es = h.step(float(y[t]))
            ref = [f.step(float(y[t])) for f in fs]
            assert same(lm, [r[0] for r in ref]) and same(es, [r[1] for r in ref]), (shape, threads, k, t)
        x, w, _ = h.state(want_anc=False)
        for th in range(2):
            ox, ow, _, _ = fs[th].state()
            assert same(x[:, th], ox) and same(w[th], ow), (shape, threads, k, th)
        h.close()


# (seg, nseg): nseg_p2 = 2 threads of the larger workgroup = 4 threads of the smaller one: M2 there, G here
PAIRS = [(256, (64, 2), (128, 1), 150), (512, (128, 2), (256, 1), 300), (1024, (128, 4), (256, 2), 300)]


@pytest.mark.parametrize("seg,ga,gb,nseg", PAIRS, ids=["seg%d" % p[0] for p in PAIRS])
def test_copy_from_between_geometries(L, ob, monkeypatch, seg, ga, gb, nseg):
    """smc_copy_from between two handles of the same segment length and different np, in both directions: one has the global
    segment table in its slab, the other does not"""
    n = nseg * seg - 5
    y = series(1, 5, seed=9)
    raws = raws_for(1, 2)
    for gd, gs in ((ga, gb), (gb, ga)):
        hs, fs = [], []
        for (threads, k), seed in ((gd, 21), (gs, 22)):
            shape = GC.shape_of(n, seg, threads, False)
            hs.append(make(L, monkeypatch, "plain", 1, GC.NONE, threads, k, n, 2, shape, seed=seed))
            fs.append([ob.Filter(1, raws[th], n, seg=seg, seed=seed, stream=th) for th in range(2)])
        assert {GC.shape_of(n, seg, g[0], False) for g in (gd, gs)} == {"M2", "G"}
        for h, ff in zip(hs, fs):
            assert same(h.init(float(y[0])), [f.bootstrap_filter(float(y[0])) for f in ff])
            for t in (1, 2):
                lm, _ = h.step(float(y[t]))
                assert same(lm, [f.step(float(y[t]))[0] for f in ff])
        hs[0].copy_from(hs[1], np.array([0, 1], dtype=np.uint8))
        fs[0][1].copy_state_from(fs[1][1])
        for t in (3, 4):
            lm, es = hs[0].step(float(y[t]))
            ref = [f.step(float(y[t])) for f in fs[0]]
            assert same(lm, [r[0] for r in ref]) and same(es, [r[1] for r in ref]), (seg, gd, gs, t)
        assert CR.first_mismatch(snap(hs[0]), CR.stack([TP.orc_slot(f) for f in fs[0]])) is None, (seg, gd, gs)
        hs[0].close(); hs[1].close()


@pytest.mark.parametrize("seg,ga,gb,nseg", PAIRS, ids=["seg%d" % p[0] for p in PAIRS])
def test_recycled_bundle_of_another_geometry(L, ob, monkeypatch, seg, ga, gb, nseg):
    """create, run, destroy under one geometry; the same filter under the other one takes the destroyed handle's slab (whose layout
    differs: with and without the global segment table) and gives the bits of a handle on other memory, and the oracle's"""
    n = nseg * seg - 5
    y = series(1, 4, seed=13)
    r = reference(L, ob, "plain", 1, GC.NONE, n, seg, 2, y)
    for first, second in ((ga, gb), (gb, ga)):
        h = make(L, monkeypatch, "plain", 1, GC.NONE, first[0], first[1], n, 2, GC.shape_of(n, seg, first[0], False))
        assert np.all(np.isfinite(h.log_likelihood(y)))
        h.close()
        h = make(L, monkeypatch, "plain", 1, GC.NONE, second[0], second[1], n, 2, GC.shape_of(n, seg, second[0], False))
        g = make(L, monkeypatch, "plain", 1, GC.NONE, second[0], second[1], n, 2, GC.shape_of(n, seg, second[0], False))   # (h holds the recycled bundle)
        check_ll(h, y, r, (seg, first, second, "recycled"))
        check_ll(g, y, r, (seg, first, second, "other memory"))
        assert CR.first_mismatch(snap(h), snap(g)) is None
        h.close(); g.close()


# ---- 3. forecasts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", TF.MODELS)
def test_forecast_clouds_at_every_geometry(L, monkeypatch, model):
    """k_forecast<MODEL, THREADS, NP> at the 13 geometries, n = seg - 3 and 2 seg + 5, three filters, H = 3: the clouds and the
    per-particle predictive moments behind the summaries against smc_host_forecast on the device's own state"""
    H = 3
    for threads, k in GC.GEOMETRIES:
        seg = GC.seg_of(threads, k)
        monkeypatch.setenv("SMC_NP", str(k))
        for n in (seg - 3, 2 * seg + 5):
            h = TF.filtered(L, model, seg, n, steps=3)
            assert h.launch_geometry()[:2] == (threads, k) and h.seg == seg, (model, threads, k, h.launch_geometry())
            x, w, _ = h.state(want_anc=False)
            ref_x, ref_y, _, _ = TF.host_twin(L, model, TF.RAWS[model], x, H)
            xf, yf = h.forecast_cloud(H, TF.FSEED)
            assert xf.shape == (H, h.d, 3, n) and TF.same(xf, ref_x) and TF.same(yf, ref_y), (model, threads, k, n)
            comp = min(1, h.d - 1)                                       # the summaries, whose predictive rows no cloud call returns
            TF.check_forecast_rows(L, h, model, h.forecast(H, TF.FSEED, p=TF.PS, component=comp), H, comp)
            h.close()


# ---- 4. the LDS-resident kernels ----------------------------------------------------------------------------------------------------
# (variant, model, proposal): the objects with resident and window kernels
RES_OBJECTS = [("plain", m, GC.NONE) for m in GC.FAMILIES["plain"]] + [("guided", 1, GC.AFFINE), ("guided", 1, GC.OPTIMAL), ("guided", 3, GC.OPTIMAL)] + \
              [("missing", m, GC.NONE) for m in GC.FAMILIES["missing"]] + [("missing_guided", 1, GC.OPTIMAL), ("missing_guided", 3, GC.OPTIMAL)]
RES_T, RES_NTH, PS3 = 6, 3, [0.1, 0.5, 0.9]


def res_series(variant, model, ragged):
    y = series(model, RES_T, seed=11)
    if variant in ("missing", "missing_guided"):
        y = MR.with_gaps(y, (0, 2) if ragged else (3,))
    return y


def res_handle(L, variant, model, kind, n, seg, rnp, systematic=False):
    h = L.Handle(model, RES_NTH, n, seg=seg, seed=SEED, flags=flags_of(L, variant, systematic))
    assert h.nseg == 1 and h.resident and h.can_window and h.seg == seg, (variant, model, n, seg)
    if rnp is not None:
        assert h.launch_geometry()[2] == rnp, (h.launch_geometry(), rnp)
    h.set_params(raws_for(model, RES_NTH))
    if kind != GC.NONE:
        h.set_proposal(kind, pars_for(kind, RES_NTH))
    return h


def single_steps(L, variant, model, kind, n, seg, y):
    """the same filters through the step API (one k_step launch per step): [(logmu, ess, x, w)] per step, and the snapshot and logZ
    after step 3"""
    h = res_handle(L, variant, model, kind, n, seg, None)
    out, at3 = [], None
    for t in range(len(y)):
        lm, es = (h.init(float(y[0])), h.logZ()[1]) if t == 0 else h.step(float(y[t]))
        x, w, _ = h.state(want_anc=False)
        out.append((lm, es, x, w))
        if t == 3:
            at3 = (snap(h), h.logZ()[0])
    h.close()
    return out, at3


# segments of 4096 for up to three state rows, of 8192 for one (resident_supported): the others have no resident launch
RES_CASES = [(seg,) + o for seg in GC.RESIDENT_SEGS for o in RES_OBJECTS if GC.resident_fits(o[1], seg)]


@pytest.mark.parametrize("seg,variant,model,kind", RES_CASES, ids=["%d-%s.%d-%d" % c for c in RES_CASES])
def test_resident_and_window_kernels(L, ob, monkeypatch, seg, variant, model, kind):
    """k_resident and its window twin under SMC_RES_NP = 1, 2, 4 (a value without a kernel at the segment length runs the table's
    neighbour): n = seg and seg - 77, three filters with distinct rows, T = 6; the whole series with traces, with systematic
    resampling, with per-step summaries in both modes, and a window of five of which three are kept"""
    comp = min(1, GC.DIM[model] - 1)
    for n in (seg, seg - 77):
        y = res_series(variant, model, n != seg)
        monkeypatch.delenv("SMC_RES_NP", raising=False)
        r = reference(L, ob, variant, model, kind, n, seg, RES_NTH, y)
        rs = reference(L, ob, variant, model, kind, n, seg, RES_NTH, y, systematic=True)
        steps, at3 = single_steps(L, variant, model, kind, n, seg, y)
        for t, (lm, es, _, _) in enumerate(steps):
            assert same(lm, r["lm"][t]) and same(es, r["es"][t]), (variant, model, n, t, "single steps")
        for rnp in (1, 2, 4):
            ctx = (variant, model, kind, seg, n, rnp)
            monkeypatch.setenv("SMC_RES_NP", str(rnp))
            h = res_handle(L, variant, model, kind, n, seg, rnp)
            check_ll(h, y, r, ctx)
            # a window of five after the first step, three of them kept
            h.reseed(SEED)
            h.init(float(y[0]))
            wl, we = h.step_window(y[1:])
            assert same(wl, r["lm"][1:]) and same(we, r["es"][1:]), ctx + ("window",)
            h.step_commit(3)
            assert CR.first_mismatch(snap(h), at3[0]) is None and same(h.logZ()[0], at3[1]), ctx + ("commit", CR.first_mismatch(snap(h), at3[0]))
            # per-step summaries, weighted and unweighted
            for mode in ("weighted", "unweighted"):
                h.reseed(SEED)
                h.set_summary_mode(mode)
                h.set_summaries(PS3, comp, moments=True)
                z, lm, es = h.log_likelihood(y, trace=True)
                assert same(z, r["logZ"]) and same(lm, r["lm"]) and same(es, r["es"]), ctx + (mode,)
                q, mean, var = h.get_summaries(RES_T)
                for t, (_, _, x, w) in enumerate(steps):
                    for th in range(RES_NTH):
                        for cc in range(h.d):
                            if mode == "weighted":
                                check_moments(mean[t, cc, th], var[t, cc, th], x[cc, th], w[th], ctx + (mode, t, th, cc))
                            else:
                                check_sample_moments(mean[t, cc, th], var[t, cc, th], x[cc, th], ctx + (mode, t, th, cc))
                        if mode == "weighted":
                            check_quantiles(q[t, th], PS3, x[comp, th], w[th], quantile_delta(n, 1, seg, math.fsum(w[th])), ctx + (mode, t, th))
                        else:
                            assert same_bits(q[t, th], quantile7(x[comp, th], PS3)), ctx + (mode, t, th)
                h.set_summaries(None)
                h.set_summary_mode("weighted")
            h.close()
            hs = res_handle(L, variant, model, kind, n, seg, rnp, systematic=True)
            check_ll(hs, y, rs, ctx + ("systematic",))
            hs.close()


# ---- 5. the n_theta rule ------------------------------------------------------------------------------------------------------------
RULE = [("plain", 1, GC.NONE), ("plain", 4, GC.NONE), ("guided", 3, GC.OPTIMAL), ("missing", 1, GC.NONE)]


@pytest.mark.parametrize("variant,model,kind", RULE, ids=["%s.%d" % o[:2] for o in RULE])
def test_more_than_512_filters_take_two_pairs_per_thread(L, ob, monkeypatch, variant, model, kind):
    """513 filters of 1024 particles, no knob: resident_np answers 0, which is (256, 2) - the shape of the large batches"""
    monkeypatch.delenv("SMC_RES_NP", raising=False)
    monkeypatch.delenv("SMC_NP", raising=False)
    nth, n, T = 513, 1024, 4
    y = series(model, T, seed=11)
    if variant == "missing":
        y = MR.with_gaps(y, (2,))
    raws = raws_for(model, nth)
    h = L.Handle(model, nth, n, seg=1024, seed=SEED, flags=flags_of(L, variant))
    assert h.launch_geometry() == (512, 1, 0) and GC.resident_geo(1024, 0) == (256, 2) and h.resident
    small = L.Handle(model, 512, n, seg=1024, seed=SEED, flags=flags_of(L, variant))
    assert small.launch_geometry() == (512, 1, 1)
    small.close()
    h.set_params(raws)
    if kind != GC.NONE:
        h.set_proposal(kind, None)
    z, lm, es = h.log_likelihood(y, trace=True)
    x, w, a = h.state()
    raw = h.weights_raw()
    if variant == "missing":
        r = MR.run_series(L, ob, model, raws, n, 1024, SEED, y)
    elif variant == "guided" or model == 4:
        r = CR.run_series(L, ob, model, raws, n, 1024, SEED, y, kind=kind)
    else:
        r = None
    for th in range(nth):
        if r is None:
            f = ob.Filter(model, raws[th], n, seg=1024, seed=SEED, stream=th)
            oz, olm, oes = f.log_likelihood(y, trace=True)
            ref = TP.orc_slot(f)
        else:
            oz, olm, oes = r["logZ"][th], r["lm"][:, th], r["es"][:, th]
            ref = tuple(s[:, th] if k == 0 else s[th] for k, s in enumerate(r["snap"]))
        assert same([z[th]], [oz]) and same(lm[:, th], olm) and same(es[:, th], oes), (variant, model, th)
        dev = (x[:, th], w[th], a[th]) + tuple(q[th] for q in raw)
        assert CR.first_mismatch(dev, ref) is None, (variant, model, th, CR.first_mismatch(dev, ref))
    if (variant, model) == ("plain", 1):                                # ... and one window of the same batch against single steps
        h.reseed(SEED)
        h.init(float(y[0]))
        wl, we = h.step_window(y[1:])
        assert same(wl, lm[1:]) and same(we, es[1:])
        h.step_commit(T - 1)
        assert CR.first_mismatch(snap(h), (x, w, a) + tuple(raw)) is None and same(h.logZ()[0], z)
    h.close()
