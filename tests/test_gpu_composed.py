"""The guided filters and the marginal UCSV family against the composed whole-series reference (pytest -m gpu), bit for bit.

tests/composed_reference.py runs every step on the CPU as: the oracle's resampler at the filter's time index -> gather of all
rows of the ancestor's state -> the particle's normals (pair i >> 1, element i & 1, slot SLOT_NORMAL0 + k, step t) -> the
library's host twin of the step -> the oracle's normalisation.  Compared on every launch path of test_gpu_guided.PATHS and for
the four laws lg-optimal, lg-poor, ucsv-optimal and rb: the logmu trace, the ess trace at every kept step, logZ, x in all rows,
w, ancestors and the raw fixed-point weights C, m, S, S2hi, S2lo.  No tolerances.  tests/test_composed_host.py ties the pieces
and the driver to the pinned oracle on the CPU."""
import time

import numpy as np
import pytest

import composed_reference as CR
import test_gpu_guided as TG
import test_gpu_rbpf as TR

pytestmark = pytest.mark.gpu

PATHS, same, bits = TG.PATHS, TG.same, TG.bits
SYSTEMATIC = TG.SYSTEMATIC
LAWS = dict(TG.PROPOSALS)                      # name -> (model, kind, rows(raw) or None)
LAWS["rb"] = (CR.RB, CR.NONE, None)
SEED = 7
_REF = {}


def law_inputs(L, law, nth, T):
    """(model, kind, parameter rows, proposal rows or None, series): what run() of the two modules gives a handle"""
    model, kind, rows = LAWS[law]
    if model == CR.RB:
        return model, kind, TR.raws_for(nth), None, TR.series(T)
    raw = TG.raws_for(model, nth)
    return model, kind, raw, (rows(raw) if callable(rows) else rows), TG.series(model, T)


def reference(L, ob, law, n, seg, systematic, nth, T, seed=SEED):
    """computed once per (law, geometry, resampler): the launch paths that share them share it; never modified"""
    key = (law, n, seg, bool(systematic), nth, T, seed)
    if key not in _REF:
        model, kind, raw, pars, y = law_inputs(L, law, nth, T)
        _REF[key] = CR.run_series(L, ob, model, raw, n, seg, seed, y, kind=kind, pars=pars, systematic=systematic)
    return _REF[key]


def assert_filter(dev, ref, th, ctx, first=False):
    """the state of filter th: x in all rows, w, ancestors (when the handle keeps them), C, m, S, S2hi, S2lo"""
    rs = ref["first" if first else "snap"]
    names = ["x", "w", "ancestors", "C", "m", "S", "S2hi", "S2lo"]
    assert all(dev[k] is not None for k in range(8) if k != 2), ctx + (th, "a quantity is missing")
    keep = [k for k in range(8) if k != 2 or dev[2] is not None]      # ancestors: only of a handle with FLAG_ANCESTORS
    got = [dev[k][:, th] if k == 0 else dev[k][th] for k in keep]
    exp = [rs[k][:, th] if k == 0 else rs[k][th] for k in keep]
    bad = CR.first_mismatch(got, exp, [names[k] for k in keep])
    assert bad is None, ctx + (th, bad)


def assert_series(dev, ref, ctx, skip=None, traces=True):
    """dev = (logmu trace, ess trace, snapshot + (logZ, ess)) of a handle against the reference of its filters"""
    lm, es, snap = dev[:3]
    z, e = snap[-2], snap[-1]
    for th in range(len(z)):
        if skip is not None and skip[th]:
            assert z[th] == -np.inf, ctx + (th, "logZ of a skipped filter")
            assert_filter(snap, ref, th, ctx + ("skipped: the state after the first step",), first=True)
            continue
        if traces:
            assert same(lm[:, th], ref["lm"][:, th]), ctx + (th, "logmu trace", int(np.argmax(bits(lm[:, th]) != bits(ref["lm"][:, th]))))
            assert same(es[:, th], ref["es"][:, th]), ctx + (th, "ess trace", int(np.argmax(bits(es[:, th]) != bits(ref["es"][:, th]))))
        assert same([z[th]], [ref["logZ"][th]]), ctx + (th, "logZ", z[th], ref["logZ"][th])
        assert same([e[th]], [ref["es"][-1, th]]), ctx + (th, "last ess")
        assert_filter(snap, ref, th, ctx)


# ---- every law on every launch path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("law", list(LAWS))
def test_every_path_equals_the_composed_reference(L, ob, law, path):
    """run() of test_gpu_guided / test_gpu_rbpf (three filters with their own parameter rows, T = 12; above 2^20 one filter and
    T = 4).  Skipped filters: logZ = -inf and the state the reference has after its first step."""
    n, seg, flags, how, skip = PATHS[path]
    nth, T = (1, 4) if n > (1 << 20) else (3, 12)
    t0 = time.perf_counter()
    dev = TR.run(L, path) if law == "rb" else TG.run(L, LAWS[law][0], path, LAWS[law][1], LAWS[law][2])
    t1 = time.perf_counter()
    ref = reference(L, ob, law, n, seg, flags & SYSTEMATIC, nth, T)
    t2 = time.perf_counter()
    print("composed %s / %s: device %.2f s, reference %.2f s" % (law, path, t1 - t0, t2 - t1))
    if law == "rb":
        assert dev[3][:2] == (ref["seg"], ref["nseg"]) and dev[3][3] == 4
    assert_series(dev, ref, (law, path), skip=None if n > (1 << 20) else skip)


def series_on(L, law, n, seg, flags, nth, T, seed=SEED, trace=True, pars=None, raws=None):
    """one log_likelihood call of a handle built as run() builds it, outside PATHS"""
    model, kind, raw, rows, y = law_inputs(L, law, nth, T)
    raw, rows = (raw if raws is None else raws), (rows if pars is None else pars)
    h = L.Handle(model, nth, n, seg=seg, seed=seed, flags=flags | (L.FLAG_ANCESTORS if trace else 0))
    h.set_params(raw)
    if kind != CR.NONE:
        h.set_proposal(kind, rows)
    if trace:
        _, lm, es = h.log_likelihood(y, trace=True)
    else:
        h.log_likelihood(y)
        lm = es = None
    x, w, a = h.state()
    out = (lm, es, (x, w, a) + tuple(h.weights_raw()) + h.logZ(), (h.seg, h.nseg))
    h.close()
    return out


# ---- more than 512 segments: the global segment table --------------------------------------------------------------------
@pytest.mark.parametrize("law", list(LAWS))
def test_global_segment_table(L, ob, law):
    """513 segments of 256: the table of the segments comes from global memory (k_table), as in
    test_gpu_parity.test_global_segment_table_paths for the bootstrap families; one filter, T = 4"""
    n, seg, T = 513 * 256, 256, 4
    dev = series_on(L, law, n, seg, 0, 1, T)
    assert dev[3] == (256, 513)
    assert_series(dev, reference(L, ob, law, n, seg, False, 1, T), (law, "513 segments"))


# ---- the step API with state changes in the middle of a series ----------------------------------------------------------------
@pytest.mark.parametrize("law", ["lg-poor", "rb"])
def test_step_api_with_state_changes(L, ob, law):
    """n = 1024, three filters, T = 12: set_streams before step 4, reseed before step 6, set_params (and a new proposal row per
    filter) before step 8; the reference follows through orc_filter_set_rng and its own new rows"""
    n, nth, T = 1024, 3, 12
    model, kind, raw, rows, y = law_inputs(L, law, nth, T)
    streams = np.array([5, 0xFFFFFFFF, 2], dtype=np.uint32)
    raw2 = raw * np.array([1.2, 1.0, 0.8] + [1.0] * (raw.shape[1] - 3)) + (0.0 if model == 1 else np.array([0, 0.05, 0.5, -0.3, 0.2]))
    rows2 = np.array([[0.1, 0.4, 0.2, 1.5], [-0.2, 0.3, 0.3, 0.9], [0.0, 0.5, 0.1, 1.1]]) if kind == CR.AFFINE else None
    h = L.Handle(model, nth, n, seed=SEED, flags=L.FLAG_ANCESTORS)
    h.set_params(raw)
    if kind != CR.NONE:
        h.set_proposal(kind, rows)
    fs = [CR.ComposedFilter(L, ob, model, raw[th], n, seed=SEED, stream=th, kind=kind, par=None if rows is None else rows[th])
          for th in range(nth)]
    assert same(h.init(y[0]), [f.init(y[0])[0] for f in fs])
    for t in range(1, T):
        if t == 4:
            h.set_streams(streams)
            for f, s in zip(fs, streams):
                f.set_rng(SEED, s)
        if t == 6:
            h.reseed(99)
            for f, s in zip(fs, streams):
                f.set_rng(99, s)
        if t == 8:
            h.set_params(raw2)
            if kind != CR.NONE:
                h.set_proposal(kind, rows2)
            for th, f in enumerate(fs):
                f.set_params(raw2[th], None if rows2 is None else rows2[th])
        lm, es = h.step(y[t])
        r = [f.step(y[t]) for f in fs]
        assert same(lm, [q[0] for q in r]) and same(es, [q[1] for q in r]), (law, t)
        if t in (4, 6, 8, T - 1):
            snap = TG.snapshot(h)
            ref = dict(snap=CR.stack([f.snapshot() for f in fs]))
            for th in range(nth):
                assert_filter(snap, ref, th, (law, t))
            assert same(snap[-2], [f.logZ for f in fs]), (law, t, "logZ")
    h.close()


# ---- a proposal row per filter of a batch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, TG.NO_RESIDENT], ids=["resident", "no-resident"])
def test_batched_proposal_rows(L, ob, flags):
    """nine filters of 1024 particles, each with its own parameter row and its own AFFINE row: a row read from another filter's
    slot gives that filter another draw and other weights"""
    nth, n, T = 9, 1024, 12
    k = np.arange(nth)
    rows = np.stack([0.05 * k - 0.2, 0.1 + 0.08 * k, 0.05 + 0.03 * k, 0.6 + 0.2 * k], axis=1)
    raws = TG.raws_for(1, nth)
    dev = series_on(L, "lg-poor", n, 0, flags, nth, T, pars=rows, raws=raws)
    key = ("batched-rows", n, nth, T)
    if key not in _REF:
        _REF[key] = CR.run_series(L, ob, 1, raws, n, 0, SEED, TG.series(1, T), kind=CR.AFFINE, pars=rows)
    assert_series(dev, _REF[key], ("batched rows", flags))


# ---- several segments, no traces, no ancestors -----------------------------------------------------------------------------------
@pytest.mark.parametrize("law", list(LAWS))
def test_multi_segment_series_without_traces(L, ob, law):
    """the whole-series call of a multi-segment handle that keeps neither traces nor ancestors (the geometry of the path
    "multi-seg256", which records both): no step but the last accumulates the sum of squares, and (logmu, 0) of the steps before
    follow from the totals alone.  Every law gives the reference's bits."""
    n, seg, nth, T = 3000, 256, 3, 12
    dev = series_on(L, law, n, seg, 0, nth, T, trace=False)
    assert_series(dev, reference(L, ob, law, n, seg, False, nth, T), (law, "no traces"), traces=False)
