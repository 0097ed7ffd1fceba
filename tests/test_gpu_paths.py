"""Every per-filter option on every launch path (pytest -m gpu), bit-exact against the CPU oracle.

The kernels a handle launches depend on (n, seg, flags); the options (skip mask, stream ids, reseed, the step API,
permute / copy_from, per-step summaries, traces, short series, reused handles) are handled in each of those kernels
separately.  PATHS names one table entry per launch path and asserts the geometry it claims; every test below is
parametrised over all of them.  The oracle side of a skipped filter is "not run": its state stays, its logZ is -inf.

  R   one segment, the LDS-resident whole-series kernel (k_resident)
  S   one segment, SMC_FLAG_NO_RESIDENT: one k_step launch per step, k_finalize emits
  M1  2 <= nseg, nseg_p2 <= threads: k_step builds the segment table in its prologue (one record per thread)
  M2  threads < nseg_p2 <= 2 threads: two records per thread
  G   nseg_p2 > 2 threads: k_table builds the table in global memory once per step and emits
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
SV = [-1.0, 0.95, 0.25]
UC = [0.2, 0.2, 3.0, 0.0, 0.0]
RAW = {1: LG, 2: SV, 3: UC}
NO_RESIDENT = 2                                                   # SMC_FLAG_NO_RESIDENT
THREADS = {256: 128, 512: 256, 1024: 512, 2048: 512, 4096: 1024, 8192: 1024}   # threads per workgroup of k_step (geo_default)

# path id -> (model, n, seg, flags)
PATHS = {
    "R": ((1, 1024, 0, 0), (1, 1000, 0, 0), (3, 512, 0, 0), (2, 8192, 0, 0)),
    "S": ((1, 1024, 0, NO_RESIDENT), (3, 2048, 0, NO_RESIDENT)),
    "M1": ((1, 5000, 1024, 0), (3, 3000, 512, 0)),
    "M2": ((1, 40000, 256, 0), (3, 33000, 256, 0)),
    "G": ((1, 70000, 256, 0), (3, 67000, 256, 0), (2, 140000, 256, 0)),
}
CASES = [(pid, c) for pid, cs in PATHS.items() for c in cs]
CASE_IDS = ["%s-m%d-n%d" % (pid, c[0], c[1]) for pid, c in CASES]
FIRST = [(pid, cs[0]) for pid, cs in PATHS.items()]              # one shape per path: the costlier options
FIRST_IDS = list(PATHS)
LAST = [(pid, cs[-1]) for pid, cs in PATHS.items()]               # ... and another model family on every path


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def path_of(h):
    """the launch path of a handle, from its geometry (smc_create / enqueue_log_likelihood)"""
    if h.nseg == 1:
        return "R" if h.resident else "S"
    p2 = 1 << (h.nseg - 1).bit_length()
    th = THREADS[h.seg]
    return "M1" if p2 <= th else ("M2" if p2 <= 2 * th else "G")


def raws_for(model, nth):
    """distinct parameter rows, so that slots cannot stand in for one another"""
    r = np.tile(RAW[model], (nth, 1)).astype(float)
    r[:, 0] *= 1.0 - 0.3 * np.arange(nth) / max(nth, 1)
    return r


def series(model, T, seed=1998):
    from oracle import binding as ob
    return ob.simulate(model, RAW[model], T, seed)[1]


def make(L, pid, case, nth, seed, flags=0):
    model, n, seg, fl = case
    h = L.Handle(model, nth, n, seg=seg, seed=seed, flags=fl | flags | L.FLAG_ANCESTORS)
    assert path_of(h) == pid, (pid, case, h.seg, h.nseg, h.resident)
    h.set_params(raws_for(model, nth))
    return h


def dev_slots(h):
    """per-slot state of a handle: x, w, ancestors and the raw fixed-point weights"""
    x, w, a = h.state()
    C, m, S, hi, lo = h.weights_raw()
    return [(x[:, th], w[th], a[th], C[th], m[th], S[th], hi[th], lo[th]) for th in range(h.n_theta)]


def orc_slot(f):
    x, w, a, _ = f.state()
    return (x, w, a) + tuple(f.weights_raw())


def assert_slot(d, o, ctx):
    assert same(d[0], o[0]) and same(d[1], o[1]) and np.array_equal(d[2], o[2]), ctx
    assert np.array_equal(d[3], o[3]) and same(d[4], o[4]) and np.array_equal(d[5], o[5]), ctx
    assert np.array_equal(d[6], o[6]) and np.array_equal(d[7], o[7]), ctx


@functools.lru_cache(maxsize=48)
def oracle_ll(case, nth, th, seed, stream, ykey):
    """the oracle's log_likelihood of filter th of a handle made by make(): (logZ, logmu trace, ess trace, slot state)"""
    from oracle import binding as ob
    model, n, seg, _ = case
    f = ob.Filter(model, raws_for(model, nth)[th], n, seg=seg, seed=seed, stream=stream)
    z, lm, es = f.log_likelihood(np.array(ykey), trace=True)
    return z, lm, es, orc_slot(f)


def expect_ll(case, nth, seed, y, skip=None, streams=None):
    """what smc_log_likelihood returns: skipped filters are not run (logZ -inf, NaN traces, state None = untouched)"""
    T = len(y)
    z, lm, es, st = np.full(nth, -np.inf), np.full((T, nth), np.nan), np.full((T, nth), np.nan), [None] * nth
    for th in range(nth):
        if skip is not None and skip[th]:
            continue
        s = th if streams is None else int(streams[th])
        z[th], lm[:, th], es[:, th], st[th] = oracle_ll(case, nth, th, seed, s, tuple(float(v) for v in y))
    return z, lm, es, st


def assert_ll(h, y, exp, before=None, ctx=()):
    """one smc_log_likelihood call with traces against expect_ll; skipped slots must hold `before` (the slots before the call)"""
    z, lm, es = h.log_likelihood(y, trace=True)
    ez, elm, ees, est = exp
    assert same(z, ez), ctx + ("logZ", z, ez)
    zq, _ = h.logZ()
    assert same(zq, ez), ctx + ("smc_get_logZ", zq, ez)
    for th in range(h.n_theta):
        if est[th] is None:
            assert np.all(np.isnan(lm[:, th])) and np.all(np.isnan(es[:, th])), ctx + ("trace of a skipped filter", th)
        else:
            assert same(lm[:, th], elm[:, th]) and same(es[:, th], ees[:, th]), ctx + ("traces", th)
    slots = dev_slots(h)
    for th in range(h.n_theta):
        if est[th] is not None:
            assert_slot(slots[th], est[th], ctx + ("state", th))
        elif before is not None:
            assert_slot(slots[th], before[th], ctx + ("state of a skipped filter", th))
    return slots


MASKS = (("none", [0, 0, 0], 3), ("first", [1, 0, 0], 1), ("last", [0, 0, 1], 2), ("alternating", [1, 0, 1], 3), ("all", [1, 1, 1], 2))


@pytest.mark.parametrize("pid,case", CASES, ids=CASE_IDS)
def test_skip_mask(L, ob, pid, case):
    """run unskipped (the pinned mirror holds finite values), reseed + mask + run (T = 1, 2, 3: the series ends in either state
    buffer), clear + reseed + run: skipped filters read -inf / NaN and keep their state bit for bit, active filters are the
    unskipped run of the same seed"""
    model, nth = case[0], 3
    y0, y1 = series(model, 3), series(model, 3, seed=7)
    h = make(L, pid, case, nth, seed=5)
    for name, mask, T in MASKS:
        ctx = (pid, case, name, T)
        h.reseed(5)
        before = assert_ll(h, y0, expect_ll(case, nth, 5, y0), ctx=ctx + ("unskipped",))
        h.reseed(6)
        h.set_skip(mask)
        assert_ll(h, y1[:T], expect_ll(case, nth, 6, y1[:T], skip=mask), before=before, ctx=ctx + ("masked",))
        h.set_skip(None)
        h.reseed(6)
        assert_ll(h, y1[:T], expect_ll(case, nth, 6, y1[:T]), ctx=ctx + ("cleared",))
    h.close()


@pytest.mark.parametrize("pid,case", FIRST, ids=FIRST_IDS)
def test_skip_mask_first_call_on_a_reused_bundle(L, ob, pid, case):
    """create + unskipped run + destroy, then the same geometry again (the destroyed handle's pinned mirror and slab are reused)
    and a skipped first call: -inf, not the previous handle's value"""
    model, nth = case[0], 3
    y = series(model, 4)
    h = make(L, pid, case, nth, seed=5)
    assert np.all(np.isfinite(h.log_likelihood(y)))
    h.close()
    h = make(L, pid, case, nth, seed=5)
    mask = [0, 1, 1]
    h.set_skip(mask)
    z, lm, es = h.log_likelihood(y, trace=True)
    ez, elm, ees, _ = expect_ll(case, nth, 5, y, skip=mask)
    assert same(z, ez) and same(h.logZ()[0], ez), (pid, z)
    assert np.all(np.isnan(lm[:, 1:])) and same(lm[:, 0], elm[:, 0]) and same(es[:, 0], ees[:, 0])
    h.close()


def test_skip_mask_large_batch_resident_order(L, ob):
    """600 filters, a random 40 % left out: the resident kernel runs the active ones first (order / n_active)"""
    pid, case = "R", PATHS["R"][0]
    nth = 600
    rng = np.random.default_rng(600)
    mask = (rng.random(nth) < 0.4).astype(np.uint8)
    y0, y1 = series(1, 3), series(1, 2, seed=7)
    h = make(L, pid, case, nth, seed=5)
    fs = [ob.Filter(1, r, case[1], seg=case[2], seed=5, stream=th) for th, r in enumerate(raws_for(1, nth))]
    z0 = h.log_likelihood(y0)
    before = dev_slots(h)
    for th in np.flatnonzero(mask):
        assert bits([z0[th]])[0] == bits([fs[th].log_likelihood(y0)])[0]
        assert_slot(before[th], orc_slot(fs[th]), ("before", th))
    h.reseed(6)
    h.set_skip(mask)
    z1, lm, es = h.log_likelihood(y1, trace=True)
    slots = dev_slots(h)
    assert np.all(z1[mask == 1] == -np.inf) and np.all(np.isnan(lm[:, mask == 1])) and np.all(np.isnan(es[:, mask == 1]))
    for th in range(nth):
        if mask[th]:
            assert_slot(slots[th], before[th], ("skipped", th))
            continue
        fs[th].reseed(6, th)
        z, olm, oes = fs[th].log_likelihood(y1, trace=True)
        assert bits([z1[th]])[0] == bits([z])[0] and same(lm[:, th], olm) and same(es[:, th], oes), th
        assert_slot(slots[th], orc_slot(fs[th]), ("active", th))
    h.close()


@pytest.mark.parametrize("pid,case", CASES, ids=CASE_IDS)
def test_series_length_edges(L, ob, pid, case):
    """T = 1, 2, 3 with traces on and off: the first_emit / want_s2 branches of every path"""
    model, nth = case[0], 2
    y = series(model, 3, seed=7)
    h = make(L, pid, case, nth, seed=6)
    for T in (1, 2, 3):
        exp = expect_ll(case, nth, 6, y[:T])
        assert_ll(h, y[:T], exp, ctx=(pid, case, T))
        z = h.log_likelihood(y[:T])                               # no traces
        assert same(z, exp[0]), (pid, case, T, z, exp[0])
        for th, d in enumerate(dev_slots(h)):
            assert_slot(d, exp[3][th], (pid, case, T, "untraced", th))
    h.close()


@pytest.mark.parametrize("pid,case", LAST, ids=FIRST_IDS)
def test_streams_and_reseed_on_a_used_handle(L, ob, pid, case):
    """arbitrary 32-bit stream ids, a run, reseed, a second run: the second run is a fresh handle's run and the oracle's run after
    set_rng"""
    model, nth = case[0], 3
    streams = np.array([0xFFFFFFFF, 7, 0x9E3779B9], dtype=np.uint32)
    y = series(model, 4, seed=3)
    h = make(L, pid, case, nth, seed=11)
    h.set_streams(streams)
    assert_ll(h, y, expect_ll(case, nth, 11, y, streams=streams), ctx=(pid, "first"))
    h.reseed(12)
    z2, lm2, es2 = h.log_likelihood(y, trace=True)
    s2 = dev_slots(h)
    g = make(L, pid, case, nth, seed=12)
    g.set_streams(streams)
    zg, lmg, esg = g.log_likelihood(y, trace=True)
    sg = dev_slots(g)
    assert same(z2, zg) and same(lm2, lmg) and same(es2, esg)
    for th in range(nth):
        assert_slot(s2[th], sg[th], (pid, "fresh handle", th))
        f = ob.Filter(model, raws_for(model, nth)[th], case[1], seg=case[2], seed=11, stream=int(streams[th]))
        f.log_likelihood(y)
        f.set_rng(12, int(streams[th]))
        z, olm, oes = f.log_likelihood(y, trace=True)
        assert bits([z2[th]])[0] == bits([z])[0] and same(lm2[:, th], olm) and same(es2[:, th], oes), (pid, th)
        assert_slot(s2[th], orc_slot(f), (pid, "set_rng", th))
    h.close(); g.close()


@pytest.mark.parametrize("nth", [64, 65])
@pytest.mark.parametrize("pid,case", FIRST, ids=FIRST_IDS)
def test_step_api_permute_copy_from(L, ob, pid, case, nth):
    """init -> steps -> permute (with duplicates) -> copy_from a second handle under a mask -> steps; 64 filters wait on pinned
    tickets, 65 on the stream.  The oracle follows the slots K (the permutation keeps their sources inside K)."""
    model, n, seg, _ = case
    y = series(model, 5, seed=9)
    K = [0, 1, 2, nth - 2, nth - 1]
    a = np.arange(nth, dtype=np.int32)
    a[0], a[1], a[nth - 1], a[2] = nth - 1, nth - 1, 2, 0            # duplicates; sources inside K
    mask = np.zeros(nth, dtype=np.uint8)
    mask[[0, nth - 2, 5]] = 1
    h, g = make(L, pid, case, nth, seed=21), make(L, pid, case, nth, seed=22)
    raws = raws_for(model, nth)
    fs = {th: ob.Filter(model, raws[th], n, seg=seg, seed=21, stream=th) for th in K}
    gs = {th: ob.Filter(model, raws[th], n, seg=seg, seed=22, stream=th) for th in K}

    def check_step(dev, orc, t):
        lm, es = dev
        assert np.all(np.isfinite(lm)), (pid, nth, t)
        for th in K:
            assert bits([lm[th]])[0] == bits([orc[th][0]])[0] and bits([es[th]])[0] == bits([orc[th][1]])[0], (pid, nth, t, th)

    for hh, ff in ((h, fs), (g, gs)):
        lm = hh.init(float(y[0]))
        for th in K:
            assert bits([lm[th]])[0] == bits([ff[th].bootstrap_filter(float(y[0]))])[0], (pid, nth, th)
        for t in (1, 2):
            check_step(hh.step(float(y[t])), {th: ff[th].step(float(y[t])) for th in K}, t)
    h.permute(a)
    src = {th: ob.Filter(model, raws[th], n, seg=seg, seed=21, stream=th) for th in K}
    for th in K:
        src[th].copy_state_from(fs[th])
    for th in K:
        fs[th].copy_state_from(src[int(a[th])])                     # value copy; the slot keeps its stream
    h.copy_from(g, mask)
    for th in K:
        if mask[th]:
            fs[th].copy_state_from(gs[th])
    for t in (3, 4):
        check_step(h.step(float(y[t])), {th: fs[th].step(float(y[t])) for th in K}, t)
    slots = dev_slots(h)
    z, _ = h.logZ()
    for th in K:
        assert_slot(slots[th], orc_slot(fs[th]), (pid, nth, "final", th))
    assert np.all(np.isfinite(z))
    h.close(); g.close()


@pytest.mark.parametrize("pid,case", LAST, ids=FIRST_IDS)
def test_summaries_with_skip_mask(L, ob, pid, case):
    """set_summaries(ps, comp, moments=True): active filters' quantile rows are those of the unskipped run (and the oracle's, bit for
    bit; moments to rounding), skipped filters' rows are NaN; logZ, traces and state as without summaries"""
    model, n, seg, _ = case
    nth, T = 3, 4
    ps = [0.05, 0.25, 0.5, 0.75]
    comp = 2 if model == 3 else 0
    y = series(model, T, seed=5)
    h = make(L, pid, case, nth, seed=23)
    h.set_summaries(ps, comp, moments=True)
    z0 = h.log_likelihood(y)
    q0, m0, v0 = h.get_summaries(T)
    before = dev_slots(h)
    mask = [0, 1, 0]
    h.set_skip(mask)
    assert_ll(h, y, expect_ll(case, nth, 23, y, skip=mask), before=before, ctx=(pid, "summaries"))
    q1, m1, v1 = h.get_summaries(T)
    assert np.all(np.isnan(q1[:, 1])) and np.all(np.isnan(m1[:, :, 1])) and np.all(np.isnan(v1[:, :, 1]))
    for th in (0, 2):
        assert same(q1[:, th], q0[:, th]) and same(m1[:, :, th], m0[:, :, th]) and same(v1[:, :, th], v0[:, :, th]), (pid, th)
        assert np.isfinite(z0[th])
        f = ob.Filter(model, raws_for(model, nth)[th], n, seg=seg, seed=23, stream=th)
        for t in range(T):
            f.bootstrap_filter(float(y[0])) if t == 0 else f.step(float(y[t]))
            assert same(q1[t, th], f.quantiles(ps, comp)), (pid, th, t)
            om, ov = f.moments()
            assert np.allclose(m1[t, :, th], om, rtol=1e-11, atol=1e-13) and np.allclose(v1[t, :, th], ov, rtol=1e-8, atol=1e-12)
    h.set_skip(None)                                              # the mask belongs to the call: an unskipped call has no NaN rows
    h.log_likelihood(y)
    q2, m2, _ = h.get_summaries(T)
    assert same(q2, q0) and same(m2, m0)
    h.close()


@pytest.mark.parametrize("pid", list(PATHS))
def test_handle_reuse_cycles(L, ob, pid):
    """eight create -> run -> destroy cycles alternating two geometries of the path (the bundles of destroyed handles are recycled
    between them): every cycle gives the same bits, the first of each the oracle's"""
    cases = PATHS[pid]
    geos = [(cases[0], 2), (cases[1], 2) if len(cases) > 1 else (cases[0], 3)]
    ref = {}
    for cyc in range(8):
        case, nth = geos[cyc % 2]
        y = series(case[0], 4, seed=13)
        h = make(L, pid, case, nth, seed=31)
        z, lm, es = h.log_likelihood(y, trace=True)
        got = (z, lm, es, dev_slots(h))
        h.close()
        if cyc < 2:
            ez, elm, ees, est = expect_ll(case, nth, 31, y)
            assert same(z, ez) and same(lm, elm) and same(es, ees), (pid, cyc)
            for th in range(nth):
                assert_slot(got[3][th], est[th], (pid, cyc, th))
            ref[cyc % 2] = got
            continue
        r = ref[cyc % 2]
        assert same(z, r[0]) and same(lm, r[1]) and same(es, r[2]), (pid, cyc)
        for th in range(nth):
            assert_slot(got[3][th], r[3][th], (pid, cyc, th))
