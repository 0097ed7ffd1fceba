"""GPU tests (pytest -m gpu) of the step launches that take a single filter's stream id, parameter row and observation BY VALUE
in the kernel arguments (StepHot, csrc/smc_kernels.h) instead of through the view's device pointers: every launch path of k_step
on both routes against the CPU oracle, BIT-EXACT (tolerance 0 ulp, as tests/test_gpu_parity.py), and the host's decision when the
route is legal - stale host copies, a skip mask and batched handles must go through the pointers and give the same bits."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
SV = [-1.0, 0.95, 0.25]
UC = [0.2, 0.2, 3.0, 0.0, 0.0]
RAW = {1: LG, 2: SV, 3: UC}
LG_B = [-0.3, 1.0, 0.5, 1.3, 0.0, 1.0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def pointer_handle(L, *args, **kw):
    """a handle whose step launches always go through the pointers (the switch is read when the handle is created)"""
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
    x, w, a, _ = f.state()
    return (np.array([z]), lm, es, x, w, a) + tuple(f.weights_raw())


def assert_matches_oracle(snap, osnap, th=0):
    logZ, lm, es, x, w, a, C, m, S, hi, lo = snap
    oz, olm, oes, ox, ow, oa, oC, om, oS, ohi, olo = osnap
    assert bits([logZ[th]])[0] == bits(oz)[0]
    assert same(lm[:, th], olm) and same(es[:, th], oes)
    assert same(x[:, th], ox) and same(w[th], ow) and np.array_equal(a[th], oa)
    assert np.array_equal(C[th], oC) and same(m[th], om) and np.array_equal(S[th], oS)
    assert np.array_equal(hi[th], ohi) and np.array_equal(lo[th], olo)


def run(h, y):
    logZ, lm, es = h.log_likelihood(y, trace=True)
    return snapshot(h, logZ, lm, es)


def check_single(L, ob, model, n, T, seg, flags=0, seed=7):
    """one filter: by value == oracle == the same handle through the pointers"""
    _, y = ob.simulate(model, RAW[model], T, 1998)
    flags |= L.FLAG_ANCESTORS
    osnap = oracle_snapshot(ob, model, RAW[model], n, seg, seed, 0, y, systematic=bool(flags & L.FLAG_SYSTEMATIC))
    h = L.Handle(model, 1, n, seg=seg, seed=seed, flags=flags)
    h.set_params(RAW[model])
    assert h.step_by_value and not h.resident
    s = run(h, y)
    assert_matches_oracle(s, osnap)
    geo = (h.seg, h.nseg)
    h.close()
    p = pointer_handle(L, model, 1, n, seg=seg, seed=seed, flags=flags)
    p.set_params(RAW[model])
    assert_same_snapshot(run(p, y), s)
    p.close()
    return geo


@pytest.mark.parametrize("model", [1, 2, 3])
def test_multi_segment_ragged_by_value(L, ob, model):
    """four segments of 256, the last one ragged (5 particles): the window prologue, staging and the ragged branch"""
    assert check_single(L, ob, model, 3 * 256 + 5, 6, 256, flags=L.FLAG_NO_RESIDENT) == (256, 4)


@pytest.mark.parametrize("model", [1, 2, 3])
def test_single_segment_by_value(L, ob, model):
    """n_x = 200 without the resident kernel: the single-segment k_step (MULTI = false), one ragged workgroup"""
    seg, nseg = check_single(L, ob, model, 200, 6, 0, flags=L.FLAG_NO_RESIDENT)
    assert nseg == 1


def test_global_table_by_value(L, ob):
    """2^17 particles in segments of 256: 512 segments, more than twice a workgroup's 128 threads - k_table builds the segment
    table and k_step reads it from global memory (GTAB)"""
    assert check_single(L, ob, 1, 1 << 17, 3, 256) == (256, 512)


def test_two_records_per_thread_by_value(L, ob):
    """200 segments of 256 (128 threads): the window prologue with two records per thread (RPT = 2), ragged last block"""
    assert check_single(L, ob, 1, 200 * 256 - 11, 3, 256) == (256, 200)


@pytest.mark.parametrize("n,seg", [(3 * 256 + 5, 256), (200, 0)])
def test_systematic_by_value(L, ob, n, seg):
    check_single(L, ob, 1, n, 6, seg, flags=L.FLAG_SYSTEMATIC | L.FLAG_NO_RESIDENT)


def test_batched_handle_goes_through_the_pointers(L, ob):
    """three filters with distinct rows and stream ids: not by value, unchanged"""
    n, seg, T, seed = 3 * 256 + 5, 256, 6, 11
    raws = np.array([LG, LG_B, [0.8, 1.0, 0.2, 0.4, 0.0, 1.0]])
    streams = np.array([4, 0, 9], dtype=np.uint32)
    _, y = ob.simulate(1, LG, T, 1998)
    h = L.Handle(1, 3, n, seg=seg, seed=seed, flags=L.FLAG_ANCESTORS | L.FLAG_NO_RESIDENT)
    h.set_params(raws)
    h.set_streams(streams)
    assert not h.step_by_value
    s = run(h, y)
    for th in range(3):
        assert_matches_oracle(s, oracle_snapshot(ob, 1, raws[th], n, seg, seed, int(streams[th]), y), th)
    h.close()


def test_host_copies_follow_set_params_and_set_streams(L, ob):
    """one handle: parameters A, run; parameters B, run; another stream id, run - each run is the run of a fresh handle"""
    n, seg, T, seed = 3 * 256 + 5, 256, 6, 13
    _, y = ob.simulate(1, LG, T, 1998)
    flags = L.FLAG_ANCESTORS | L.FLAG_NO_RESIDENT
    h = L.Handle(1, 1, n, seg=seg, seed=seed, flags=flags)
    for raw, stream in ((LG, None), (LG_B, None), (LG_B, 5)):
        h.set_params(raw) if stream is None else h.set_streams([stream])
        assert h.step_by_value
        s = run(h, y)
        f = L.Handle(1, 1, n, seg=seg, seed=seed, flags=flags)
        f.set_params(raw)
        if stream is not None:
            f.set_streams([stream])
        assert_same_snapshot(run(f, y), s)
        f.close()
        assert_matches_oracle(s, oracle_snapshot(ob, 1, raw, n, seg, seed, stream or 0, y))
    h.close()


def test_slots_rewritten_on_the_device_invalidate_the_host_copies(L, ob):
    """slot 0 of a handle with other parameters unpacked into the handle: its launches leave the by-value route (until the next
    set_params / set_streams) and equal those of a handle that never took it"""
    torch = pytest.importorskip("torch")
    n, seg, seed = 3 * 256 + 5, 256, 17
    _, y = ob.simulate(1, LG, 10, 1998)
    flags = L.FLAG_ANCESTORS | L.FLAG_NO_RESIDENT

    def start(make, raw):
        h = make(1, 1, n, seg=seg, seed=seed, flags=flags)
        h.set_params(raw)
        h.init(y[0])
        for t in range(1, 4):
            h.step(y[t])
        return h
    src = start(L.Handle, LG_B)
    buf = torch.empty((1, src.slot_bytes() // 8), dtype=torch.int64, device="cuda")
    src.pack_slots([0], buf.data_ptr())
    torch.cuda.synchronize()
    outs = []
    for make in (L.Handle, lambda *a, **k: pointer_handle(L, *a, **k)):
        h = start(make, LG)
        assert h.step_by_value == (make is L.Handle)
        h.unpack_slots([0], buf.data_ptr())
        assert not h.step_by_value
        res = [h.step(y[t]) for t in range(4, 10)]
        outs.append(snapshot(h) + (np.array(res),))
        if make is L.Handle:      # the next set_params / set_streams make the copies current again
            h.set_params(LG)
            assert not h.step_by_value
            h.set_streams([0])
            assert h.step_by_value
        h.close()
    src.close()
    assert_same_snapshot(outs[0], outs[1])


@pytest.mark.parametrize("n,seg", [(3 * 256 + 5, 256), (200, 0)])
def test_step_api_passes_the_observation_by_value(L, ob, n, seg):
    """smc_init / smc_step (no series on the device) == the whole-series call on the same inputs == the oracle"""
    T, seed = 6, 19
    _, y = ob.simulate(1, LG, T, 1998)
    flags = L.FLAG_ANCESTORS | L.FLAG_NO_RESIDENT
    a = L.Handle(1, 1, n, seg=seg, seed=seed, flags=flags)
    a.set_params(LG)
    whole = run(a, y)
    a.close()
    assert_matches_oracle(whole, oracle_snapshot(ob, 1, LG, n, seg, seed, 0, y))
    b = L.Handle(1, 1, n, seg=seg, seed=seed, flags=flags)
    b.set_params(LG)
    assert b.step_by_value
    lm, es = [b.init(y[0])[0]], [None]
    for t in range(1, T):
        l, e = b.step(y[t])
        lm.append(l[0])
        es.append(e[0])
    assert same(lm, whole[1][:, 0]) and same(es[1:], whole[2][1:, 0])
    assert_same_snapshot(snapshot(b), (None, None, None) + whole[3:])
    b.close()


def test_skip_mask_goes_through_the_pointers(L, ob):
    """one filter with its skip bit set: the pointer route (which reads the mask), logZ = -inf; without the mask by value again"""
    n, seg, T, seed = 3 * 256 + 5, 256, 6, 23
    _, y = ob.simulate(1, LG, T, 1998)
    h = L.Handle(1, 1, n, seg=seg, seed=seed, flags=L.FLAG_ANCESTORS | L.FLAG_NO_RESIDENT)
    h.set_params(LG)
    h.set_skip([1])
    assert not h.step_by_value
    assert h.log_likelihood(y)[0] == -np.inf
    h.set_skip([0])      # a mask in force that skips nobody: still the pointers, the ordinary result
    assert not h.step_by_value
    osnap = oracle_snapshot(ob, 1, LG, n, seg, seed, 0, y)
    assert_matches_oracle(run(h, y), osnap)
    h.set_skip(None)
    assert h.step_by_value
    assert_matches_oracle(run(h, y), osnap)
    h.close()
