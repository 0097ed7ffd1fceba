"""The pieces of tests/composed_reference.py on the CPU (no GPU): the oracle's model-free weight track reproduces the oracle's own
filters, its state normals are Philox + Box-Muller pair by pair, the four-row segment rule is the library's, the batched host
twins are the one-particle twins, and the composed driver is tied to the pinned bootstrap filter (AFFINE identity row) and to
the exact Kalman log-likelihood (marginal family with frozen volatilities)."""
import numpy as np
import pytest

import composed_reference as CR
import step_edge_inputs

LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
SV = [0.0, 0.95, 0.3]
UC = [0.2, 0.2, 3.0, 0.0, 0.0]
RAW = {1: LG, 2: SV, 3: UC}
POOR = [0.3, 0.2, 0.1, 2.0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def assert_same_track(e, b, ctx):
    """x, w, ancestors, logw and the raw fixed-point weights (C, m, S, S2hi, S2lo) of two oracle filters"""
    for k, (u, v) in enumerate(zip(e.state() + e.weights_raw(), b.state() + b.weights_raw())):
        assert same(u, v) if u.dtype == np.float64 else np.array_equal(u, v), ctx + (k,)


# (model, n, seg, systematic, T): single and several segments, a ragged last segment, two break-point records per thread's worth
# of segments (40000 / 256), more than 512 segments (131328 / 256), both resamplers, every family of the oracle
TRACKS = [(1, 1000, 0, False, 12), (3, 3000, 256, False, 12), (2, 3000, 256, False, 8), (1, 40000, 256, False, 8),
          (1, 5000, 1024, True, 8), (3, 1024, 0, True, 8), (2, 1000, 0, True, 8), (1, 131328, 256, False, 4)]


@pytest.mark.parametrize("model,n,seg,systematic,T", TRACKS)
def test_external_track_reproduces_the_filter(ob, model, n, seg, systematic, T):
    """an external filter fed the states and log-weights of an ordinary ob.Filter draws that filter's ancestors and reproduces
    its logmu, ess, weights and raw weights at every step: the resampler reads only the weight state and (seed, stream, t)"""
    _, y = ob.simulate(model, RAW[model], T, 11)
    b = ob.Filter(model, RAW[model], n, seg=seg, seed=9, stream=2, systematic=systematic)
    e = ob.ExternalFilter(ob.MODEL_DIM[model], n, seg=seg, seed=9, stream=2, systematic=systematic)
    assert (e.seg, e.nseg) == (b.seg, b.nseg)
    with pytest.raises(ValueError):
        e.draw_ancestors()                                  # no weights before the first step
    for t in range(T):
        if t == 0:
            lm, ess = b.bootstrap_filter(y[0]), b.ess()
        else:
            a = e.draw_ancestors()
            lm, ess = b.step(y[t])
            assert np.array_equal(a, b.state()[2]), (t, "ancestors")
        x, _, _, logw = b.state()
        elm, eess = e.put_step(x, logw)
        assert same([elm, eess], [lm, ess]) and eess == e.ess(), t
        assert_same_track(e, b, (t,))
    # export / import and set_rng act on the track as on a filter
    g = ob.ExternalFilter(ob.MODEL_DIM[model], n, seg=seg, seed=9, stream=2, systematic=systematic)
    g.import_state(e.export_state())
    assert_same_track(g, e, ("import",))
    assert np.array_equal(g.draw_ancestors(), e.draw_ancestors())
    b.set_rng(77, 5)
    e.set_rng(77, 5)
    a = e.draw_ancestors()
    b.step(y[0])
    assert np.array_equal(a, b.state()[2]) and not np.array_equal(a, g.draw_ancestors())
    with pytest.raises(TypeError):
        e.step(y[0])


@pytest.mark.parametrize("n", [1, 7, 8])
def test_state_normals_pair_by_pair(ob, n):
    seed, stream, t, slot = (5 << 32) + 123, 0x9E3779B9, 6, 2
    z = ob.state_normals(seed, stream, t, slot, n)
    assert z.shape == (n,)
    for p in range((n + 1) // 2):
        z0, z1 = ob.box_muller(ob.philox([p, stream, t, slot], [seed & 0xFFFFFFFF, seed >> 32]))
        assert same([z[2 * p]], [z0])
        if 2 * p + 1 < n:
            assert same([z[2 * p + 1]], [z1])


def test_segment_rule_by_rows(L, ob):
    """seg = 0 of an external filter: the library's rule for d rows (smc_auto_seg by the family's state dimension), four rows
    included; around every threshold of the rule and on a geometric sweep"""
    lib, olib = L.lib(), ob.lib()
    edges = [2048, 4096, 8192, 1 << 15, 1 << 17, 1 << 19, 16384 * 1024, 16384 * 2048, 16384 * 4096]
    ns = sorted({1, 2, 255, 256, 257, 1000} | {e + k for e in edges for k in (-1, 0, 1)} | {int(1.37 ** k) for k in range(1, 68)})
    for model, d in ((1, 1), (2, 1), (3, 3), (4, 4)):
        for n in ns:
            assert olib.orc_auto_seg_rows(d, n) == lib.smc_auto_seg(model, n), (model, n)
            if model != 4:
                assert olib.orc_auto_seg(model, n) == lib.smc_auto_seg(model, n), (model, n)
    assert ob.ExternalFilter(4, 2048).seg == 2048 and ob.ExternalFilter(4, 2049).seg == 256 and ob.ExternalFilter(3, 4096).seg == 4096


@pytest.mark.parametrize("model,kind", [(1, CR.AFFINE), (1, CR.OPTIMAL), (3, CR.OPTIMAL)])
def test_batched_guided_twin_is_the_one_particle_twin(L, model, kind):
    """the edge inputs of test_gpu_guided.test_device_guided_step_equals_host (tests/step_edge_inputs.py)"""
    raw, par, xp, z, y = step_edge_inputs.guided(model, kind)
    assert y == 0.7
    x, lw = L.host_guided_steps(model, raw, kind, par, xp, z, 0.7)
    for i in range(xp.shape[1]):
        hx, hl = L.host_guided_step(model, raw, kind, par, xp[:, i], z[:, i], 0.7)
        assert same(x[:, i], hx) and same([lw[i]], [hl]), (i, x[:, i], hx, lw[i], hl)
    x1, lw1 = L.host_guided_steps(model, raw, kind, par, xp[:, :1], z[:, :1], 0.7)         # n = 1
    assert same(x1[:, 0], x[:, 0]) and same(lw1, lw[:1])
    assert L.lib().smc_host_guided_steps(4, L._d(np.array(UC)), 2, None, L._d(xp), L._d(z), 0.7, 1, L._d(x), L._d(lw)) == -1


@pytest.mark.parametrize("first", [False, True])
def test_batched_rb_twin_is_the_one_particle_twin(L, first):
    """the edge inputs of test_gpu_rbpf.test_device_rb_step_equals_host (tests/step_edge_inputs.py)"""
    raw, sp, z, y = step_edge_inputs.rb(first)
    assert y == 0.7
    s, lw = L.host_rb_steps(raw, sp, z, 0.7, first)
    for i in range(sp.shape[1]):
        hs, hl = L.host_rb_step(raw, sp[:, i], z[:, i], 0.7, first)
        assert same(s[:, i], hs) and same([lw[i]], [hl]), (i, s[:, i], hs, lw[i], hl)


def with_nonfinite(a):
    """the first 257 columns of an edge input with particles 0, 1, 2 at +inf, -inf and NaN in the first row"""
    a = a[:, :257].copy()
    a[0, :3] = [np.inf, -np.inf, np.nan]
    return a


def step_sizes(n_all):
    """the column sets of the step-probe comparisons: n = 1 (each non-finite particle and a finite one alone), 63, 257"""
    return [slice(i, i + 1) for i in range(4)] + [slice(0, 63), slice(0, n_all)]


@pytest.mark.parametrize("model,kind", [(1, CR.AFFINE), (1, CR.OPTIMAL), (3, CR.OPTIMAL)])
def test_guided_steps_are_the_filter_steps(L, model, kind):
    """smc_host_guided_steps == smc_host_filter_steps(kind, first=0, nan_missing=0) bit for bit, non-finite states and normals
    included: one gather / step / scatter loop serves both exports"""
    raw, par, xp, z, y = step_edge_inputs.guided(model, kind)
    for xq, zq in ((with_nonfinite(xp), z[:, :257]), (xp[:, :257], with_nonfinite(z))):
        for s in step_sizes(257):
            gx, gl = L.host_guided_steps(model, raw, kind, par, xq[:, s], zq[:, s], y)
            fx, fl = L.host_filter_steps(model, raw, kind, par, xq[:, s], zq[:, s], y, first=False, missing=False)
            assert same(gx, fx) and same(gl, fl), (s, gx, fx, gl, fl)
            if s.stop - s.start == 1:   # ... and the one-particle twin, whose loop is its own
                hx, hl = L.host_guided_step(model, raw, kind, par, xq[:, s.start], zq[:, s.start], y)
                assert same(gx[:, 0], hx) and same(gl, [hl]), (s, gx, hx, gl, hl)


@pytest.mark.parametrize("first", [False, True])
def test_rb_steps_are_the_filter_steps(L, first):
    """smc_host_rb_steps == smc_host_filter_steps(MODEL_UCSV_RB, PROP_NONE, first) bit for bit, non-finite states and normals included"""
    raw, sp, z, y = step_edge_inputs.rb(first)
    for sq, zq in ((with_nonfinite(sp), z[:, :257]), (sp[:, :257], with_nonfinite(z))):
        for s in step_sizes(257):
            rs, rl = L.host_rb_steps(raw, sq[:, s], zq[:, s], y, first)
            fs, fl = L.host_filter_steps(L.MODEL_UCSV_RB, raw, L.PROP_NONE, None, sq[:, s], zq[:, s], y, first=first, missing=False)
            assert same(rs, fs) and same(rl, fl), (s, rs, fs, rl, fl)
            if s.stop - s.start == 1:
                hs, hl = L.host_rb_step(raw, sq[:, s.start], zq[:, s.start], y, first)
                assert same(rs[:, 0], hs) and same(rl, [hl]), (s, rs, hs, rl, hl)


@pytest.mark.parametrize("n,seg,systematic", [(1000, 0, False), (3000, 256, False), (5000, 1024, True)])
def test_composed_identity_row_is_the_bootstrap_filter(L, ob, n, seg, systematic):
    """the composed LG1D filter with the AFFINE row (0, A, 0, Q) against ob.Filter's bootstrap run, two filters with their own rows
    and streams: traces, logZ, x, w, ancestors and the raw weights.  Ties the driver's order of gather, normals and time index
    to the pinned oracle."""
    T = 12
    _, y = ob.simulate(1, LG, T, 1998)
    raws = np.array([LG, [0.35, 1.0, 0.99, 0.8, 0.0, 1.0]])
    rows = np.stack([np.zeros(2), raws[:, 0], np.zeros(2), raws[:, 2]], axis=1)
    c = CR.run_series(L, ob, 1, raws, n, seg, 7, y, kind=CR.AFFINE, pars=rows, systematic=systematic)
    for th in range(2):
        b = ob.Filter(1, raws[th], n, seg=seg, seed=7, stream=th, systematic=systematic)
        z, lm, es = b.log_likelihood(y, trace=True)
        assert same([c["logZ"][th]], [z]) and same(c["lm"][:, th], lm) and same(c["es"][:, th], es), th
        ref = b.state()[:3] + b.weights_raw()
        got = tuple(q[:, th] if k == 0 else q[th] for k, q in enumerate(c["snap"]))
        assert CR.first_mismatch(got, ref) is None, (th, CR.first_mismatch(got, ref))
    # the identity row is not what makes it pass: another row is another filter
    p = CR.run_series(L, ob, 1, raws[:1], n, seg, 7, y, kind=CR.AFFINE, pars=[POOR], systematic=systematic)
    assert not same(p["lm"][1:, 0], c["lm"][1:, 0]) and same(p["lm"][0, 0], c["lm"][0, 0])


@pytest.mark.parametrize("lse0,lsn0", [(0.0, 0.0), (-1.0, 0.5)])
def test_composed_rb_filter_inside_the_kalman_pin_bound(L, ob, lse0, lsn0):
    """the setting and the bound 10 T gamma sqrt(T) = 1e-6 of test_rbpf_host.test_numpy_filter_stays_inside_the_kalman_pin_bound,
    n = 256"""
    from oracle import kalman
    g, T = 1e-10, 100
    _, y = L.simulate(3, UC, T, 7)
    f = CR.ComposedFilter(L, ob, CR.RB, [g, g, 3.0, lse0, lsn0], 256, seed=3)
    f.init(y[0])
    for t in range(1, T):
        f.step(y[t])
    kf = kalman.log_likelihood(y, 1.0, 1.0, np.exp(lse0), np.exp(lsn0), x0=3.0, sigma0=np.exp(lse0))[2]
    print("composed RB - Kalman: %.3g" % (f.logZ - kf))
    assert abs(f.logZ - kf) <= 10 * T * g * np.sqrt(T), (f.logZ, kf)
    x = f.snapshot()[0]
    assert np.ptp(x[0]) <= 1e-6 and np.ptp(x[3]) <= 1e-6 and np.all(x[3] > 0)


# ---- the comparison has teeth: three deliberately wrong drivers ----------------------------------------------------------------
class SlotPlusOne(CR.ComposedFilter):
    """normals taken from slot + 1"""
    def _normals(self, k):
        return self.ob.state_normals(self.seed, self.stream, self.t, self.ob.SLOT_NORMAL0 + k + 1, self.n)


class LastRowNotGathered(CR.ComposedFilter):
    """the last state row stays with the child's index instead of coming from the ancestor"""
    def _gather(self, a):
        xp = self.x[:, a].copy()
        xp[-1] = self.x[-1]
        return xp


class TimeOffAfterCommit(CR.ComposedFilter):
    """the window path of test_gpu_guided.run keeps 3 of the 5 steps of its first window (t = 1..3): from t = 4 on the time index
    of the normals is one too far"""
    def _normals(self, k):
        t = self.t + (1 if self.t >= 4 else 0)
        return self.ob.state_normals(self.seed, self.stream, t, self.ob.SLOT_NORMAL0 + k, self.n)


WRONG = {"slot+1": SlotPlusOne, "last-row": LastRowNotGathered, "t+1": TimeOffAfterCommit}
# (model, kind, proposal row, parameter row, the first step whose logmu differs under each wrong driver).  lg-optimal: the weight of
# the locally optimal proposal does not depend on the draw, so a wrong draw shows in logmu one step later (in x at once)
TEETH = {"lg-optimal": (1, CR.OPTIMAL, None, LG, {"slot+1": 2, "last-row": 1, "t+1": 5}),
         "lg-poor": (1, CR.AFFINE, POOR, LG, {"slot+1": 1, "last-row": 1, "t+1": 4}),
         "ucsv-optimal": (3, CR.OPTIMAL, None, UC, {"slot+1": 1, "last-row": 1, "t+1": 4}),
         "rb": (CR.RB, CR.NONE, None, UC, {"slot+1": 0, "last-row": 1, "t+1": 4})}


def first_difference(got, ref):
    """(the first step at which the logmu traces differ, the first snapshot quantity that differs)"""
    d = bits(got["lm"][:, 0]) != bits(ref["lm"][:, 0])
    return (int(np.argmax(d)) if d.any() else None), CR.first_mismatch(got["snap"], ref["snap"])


@pytest.mark.parametrize("law", list(TEETH))
def test_wrong_drivers_are_reported(L, ob, law):
    """n = 1024, T = 12, the geometry of the window path: against the composed reference each wrong driver differs in the logmu
    trace from the step the defect first acts on (one step later where the weight does not depend on the draw), in logZ and in
    the final x; the right driver run twice does not differ.  tests/test_gpu_composed.py compares the GPU with the right one."""
    model, kind, par, raw, first = TEETH[law]
    y = L.simulate(3 if model == CR.RB else model, raw, 12, 1998)[1]

    def run(cls):
        return CR.run_series(L, ob, model, [raw], 1024, 0, 7, y, kind=kind, pars=None if par is None else [par], cls=cls)
    ref = run(CR.ComposedFilter)
    assert first_difference(run(CR.ComposedFilter), ref) == (None, None)
    for name, cls in WRONG.items():
        got = run(cls)
        step, quantity = first_difference(got, ref)
        assert step == first[name] and quantity == "x", (law, name, step, quantity)
        assert same(got["lm"][:step], ref["lm"][:step]) and not same(got["logZ"], ref["logZ"]), (law, name)
