"""GPU tests (pytest -m gpu) of the addresses k_step takes BY VALUE at the head of its kernel arguments (StepLead / StepEarly,
csrc/smc_kernels.h): the break-point row of the step, the segment records (or the global segment table), C of the buffer being
resampled and the particle count, derived by the host at every launch (step_hot, csrc/smc_capi.hip).  A wrong address shows as
wrong bits, so everything here is compared BIT-EXACT (tolerance 0 ulp) with the CPU oracle - logZ, the per-step traces, x, w,
ancestors, the raw weight state - at the smallest shapes at which each address matters: a break-point buffer refilled in
mid-series, batched launches (the kernel adds its filter's offsets), the global table, the step API with everything that changes
what the view's pointers mean between two steps, a handle on a recycled bundle, and a guided handle."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
UC = [0.2, 0.2, 3.0, 0.0, 0.0]
RAW = {1: LG, 3: UC}
N, SEG = 3 * 256 + 5, 256     # four segments of 256, the last one ragged (5 particles)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def raws_for(model, nth):
    """distinct parameter rows, so that filters cannot stand in for one another"""
    r = np.tile(RAW[model], (nth, 1)).astype(float)
    r[:, 0] *= 1.0 - 0.3 * np.arange(nth) / max(nth, 1)
    return r


def pointer_handle(L, *args, **kw):
    """a handle whose step launches read stream id, parameter row and observation through the view (the switch is read at creation)"""
    os.environ["SMC_STEP_BY_VALUE"] = "0"
    try:
        h = L.Handle(*args, **kw)
    finally:
        del os.environ["SMC_STEP_BY_VALUE"]
    assert not h.step_by_value
    return h


def snapshot(h, logZ=None, lm=None, es=None):
    x, w, a = h.state()
    return (logZ, lm, es, x, w, a) + tuple(h.weights_raw())


def assert_same_snapshot(p, q):
    for u, v in zip(p, q):
        if u is None or v is None:
            assert u is None and v is None
        elif u.dtype.kind == "f":
            assert same(u, v)
        else:
            assert np.array_equal(u, v)


def oracle_snapshot(ob, model, raw, n, seg, seed, stream, y, systematic=False):
    f = ob.Filter(model, raw, n, seg=seg, seed=seed, stream=stream, systematic=systematic)
    z, lm, es = f.log_likelihood(y, trace=True)
    return (np.array([z]), lm, es) + oracle_state(f)


def oracle_state(f):
    x, w, a, _ = f.state()
    return (x, w, a) + tuple(f.weights_raw())


def assert_state_matches_oracle(snap, ostate, th=0):
    x, w, a, C, m, S, hi, lo = snap
    ox, ow, oa, oC, om, oS, ohi, olo = ostate
    assert same(x[:, th], ox) and same(w[th], ow) and np.array_equal(a[th], oa)
    assert np.array_equal(C[th], oC) and same(m[th], om) and np.array_equal(S[th], oS)
    assert np.array_equal(hi[th], ohi) and np.array_equal(lo[th], olo)


def assert_matches_oracle(snap, osnap, th=0):
    logZ, lm, es = snap[:3]
    oz, olm, oes = osnap[:3]
    assert bits([logZ[th]])[0] == bits(oz)[0]
    assert same(lm[:, th], olm) and same(es[:, th], oes)
    assert_state_matches_oracle(snap[3:], osnap[3:], th)


def run(h, y):
    logZ, lm, es = h.log_likelihood(y, trace=True)
    return snapshot(h, logZ, lm, es)


def test_break_row_address_across_a_refill(L, ob):
    """one filter, T = 1030: the break-point buffer holds 1024 steps, so it is refilled and brk_t0 moves in mid-series - the row
    address the host hands over follows; by value and through the pointers"""
    T, seed = 1030, 7
    _, y = ob.simulate(1, LG, T, 1998)
    flags = L.FLAG_ANCESTORS | L.FLAG_NO_RESIDENT
    osnap = oracle_snapshot(ob, 1, LG, N, SEG, seed, 0, y)
    for make in (L.Handle, lambda *a, **k: pointer_handle(L, *a, **k)):
        h = make(1, 1, N, seg=SEG, seed=seed, flags=flags)
        h.set_params(LG)
        assert h.step_by_value == (make is L.Handle) and (h.seg, h.nseg) == (SEG, 4) and not h.resident
        assert_matches_oracle(run(h, y), osnap)
        h.close()


@pytest.mark.parametrize("model,systematic", [(1, False), (3, False), (1, True)])
def test_batched_offsets(L, ob, model, systematic):
    """three filters with distinct rows and stream ids, T = 7 (both parities of the buffer): the kernel adds th (nseg + 1), th nseg and
    th npad to the launch's addresses"""
    T, seed, nth = 7, 11, 3
    raws = raws_for(model, nth)
    streams = np.array([4, 0, 9], dtype=np.uint32)
    _, y = ob.simulate(model, RAW[model], T, 1998)
    flags = L.FLAG_ANCESTORS | L.FLAG_NO_RESIDENT | (L.FLAG_SYSTEMATIC if systematic else 0)
    h = L.Handle(model, nth, N, seg=SEG, seed=seed, flags=flags)
    h.set_params(raws)
    h.set_streams(streams)
    assert not h.step_by_value and (h.seg, h.nseg) == (SEG, 4)
    s = run(h, y)
    h.close()
    for th in range(nth):
        assert_matches_oracle(s, oracle_snapshot(ob, model, raws[th], N, SEG, seed, int(streams[th]), y, systematic=systematic), th)


def test_batched_global_table(L, ob):
    """two filters of 2^17 particles in segments of 256: 512 segments, k_table's table read through the by-value slots with the
    filter's offset (th nseg_p2)"""
    n, T, seed, nth = 1 << 17, 3, 13, 2
    raws = raws_for(1, nth)
    streams = np.array([6, 1], dtype=np.uint32)
    _, y = ob.simulate(1, LG, T, 1998)
    h = L.Handle(1, nth, n, seg=SEG, seed=seed, flags=L.FLAG_ANCESTORS)
    h.set_params(raws)
    h.set_streams(streams)
    assert (h.seg, h.nseg) == (SEG, 512)
    s = run(h, y)
    h.close()
    for th in range(nth):
        assert_matches_oracle(s, oracle_snapshot(ob, 1, raws[th], n, SEG, seed, int(streams[th]), y), th)


@pytest.mark.parametrize("nth", [1, 2])
def test_step_api_between_steps(L, ob, nth):
    """init, steps, and between steps everything that changes what the launch's addresses or by-value words must be: reseed,
    set_streams, a permute, a slot copy from another handle, an unpack_slots.  Every step's (logmu, ess) and the final state equal
    the oracle's (set_rng, copy_state_from), by value and through the pointers"""
    torch = pytest.importorskip("torch")
    T = 9
    _, y = ob.simulate(1, LG, T, 1998)
    raws, graws = raws_for(1, nth), raws_for(1, nth)[::-1].copy()
    flags = L.FLAG_ANCESTORS | L.FLAG_NO_RESIDENT
    perm = np.array([0] if nth == 1 else [1, 1], dtype=np.int32)
    mask = np.array([1, 0][:nth], dtype=np.uint8)
    new_streams = [5, 9][:nth]

    def start(make, rows, seed, steps):
        h = make(1, nth, N, seg=SEG, seed=seed, flags=flags)
        h.set_params(rows)
        out = [(h.init(float(y[0])), None)]
        out += [h.step(float(y[t])) for t in range(1, steps)]
        return h, out

    def ostart(rows, seed, steps):
        fs = [ob.Filter(1, rows[th], N, seg=SEG, seed=seed, stream=th) for th in range(nth)]
        out = [([f.bootstrap_filter(float(y[0])) for f in fs], None)]
        for t in range(1, steps):
            r = [f.step(float(y[t])) for f in fs]
            out.append(([q[0] for q in r], [q[1] for q in r]))
        return fs, out

    def ostep(fs, t):
        r = [f.step(float(y[t])) for f in fs]
        return [q[0] for q in r], [q[1] for q in r]

    # the sources of the slot copy and of the packed slot: another series (other rows, another seed) at the same step as the
    # receiver (the oracle's copy carries the step number along)
    gs6, _ = ostart(graws, 31, 6)
    gs7, _ = ostart(graws, 31, 7)
    fs, ref = ostart(raws, 21, 3)
    for f, th in zip(fs, range(nth)):
        f.set_rng(99, th)
    ref.append(ostep(fs, 3))
    for f, st in zip(fs, new_streams):
        f.set_rng(99, st)
    ref.append(ostep(fs, 4))
    if nth == 2:
        fs[0].copy_state_from(fs[1])          # value copy; the slot keeps its stream and its parameter row
    ref.append(ostep(fs, 5))
    for th in range(nth):
        if mask[th]:
            fs[th].copy_state_from(gs6[th])
    ref.append(ostep(fs, 6))
    fs[nth - 1].copy_state_from(gs7[0])
    ref.append(ostep(fs, 7))
    ref.append(ostep(fs, 8))

    snaps = []
    for make in (L.Handle, lambda *a, **k: pointer_handle(L, *a, **k)):
        g, _ = start(L.Handle, graws, 31, 6)
        h, out = start(make, raws, 21, 3)
        h.reseed(99)
        out.append(h.step(float(y[3])))
        h.set_streams(new_streams)
        out.append(h.step(float(y[4])))
        h.permute(perm)
        out.append(h.step(float(y[5])))
        h.copy_from(g, mask)
        out.append(h.step(float(y[6])))
        g.step(float(y[6]))
        buf = torch.empty((1, g.slot_bytes() // 8), dtype=torch.int64, device="cuda")
        g.pack_slots([0], buf.data_ptr())
        torch.cuda.synchronize()
        h.unpack_slots([nth - 1], buf.data_ptr())
        out.append(h.step(float(y[7])))
        out.append(h.step(float(y[8])))
        for t, ((lm, es), (olm, oes)) in enumerate(zip(out, ref)):
            assert same(lm, olm), (t, "logmu")
            assert es is None or same(es, oes), (t, "ess")
        s = snapshot(h)
        for th in range(nth):
            assert_state_matches_oracle(s[3:], oracle_state(fs[th]), th)
        snaps.append(s)
        h.close()
        g.close()
    assert_same_snapshot(snaps[0], snaps[1])


def test_recycled_handle(L, ob):
    """a handle of eight segments of 256 closed, then one of four segments of 512 created (the kept bundle fits it and is taken
    over: other buffers behind the same view fields), T = 7: the oracle's bits"""
    T, seed = 7, 17
    _, y = ob.simulate(1, LG, T, 1998)
    flags = L.FLAG_ANCESTORS | L.FLAG_NO_RESIDENT
    for n, seg, nseg in ((8 * 256, 256, 8), (3 * 512 + 5, 512, 4)):
        h = L.Handle(1, 1, n, seg=seg, seed=seed, flags=flags)
        h.set_params(LG)
        assert h.step_by_value and (h.seg, h.nseg) == (seg, nseg)
        s = run(h, y)
        h.close()
        assert_matches_oracle(s, oracle_snapshot(ob, 1, LG, n, seg, seed, 0, y))


def test_guided_handle_identity_row(L, ob):
    """a guided handle with the AFFINE identity row (0, A, 0, Q) is the bootstrap filter (tests/test_gpu_guided.py states the
    identity): the guided kernels take the same addresses by value and give the oracle's bootstrap bits"""
    T, seed = 7, 19
    _, y = ob.simulate(1, LG, T, 1998)
    h = L.Handle(1, 1, N, seg=SEG, seed=seed, flags=L.FLAG_ANCESTORS | L.FLAG_NO_RESIDENT)
    h.set_params(LG)
    h.set_proposal(L.PROP_AFFINE, [0.0, LG[0], 0.0, LG[2]])
    s = run(h, y)
    h.close()
    assert_matches_oracle(s, oracle_snapshot(ob, 1, LG, N, SEG, seed, 0, y))
