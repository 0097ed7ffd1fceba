"""GPU tests (pytest -m gpu) of the Box-Muller that k_step runs under its LDS ancestor search (step_body, csrc/smc_kernels.h: the
slices of the last pair's normals, csrc/smc_spec.h bm_slice, one share per level of the search).  A slice that ran twice, not at
all, or out of order gives other normals, and a search disturbed by what runs inside it gives other ancestors, so everything here is
compared BIT-EXACT (tolerance 0 ulp) with the CPU oracle - logZ, the per-step traces, x, w, ancestors, the raw weight state - at
the smallest shapes that reach each form of the interleave: every level count (segments of 256 to 2048), every number of probes per
level (1, 2 and 4 pairs per thread), both search loops, the paths that leave the staged search or replace its result, and the two
routes that keep their normals where they were (three state coordinates, systematic resampling).  T = 7: both parities of the buffers."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
SV = [-1.0, 0.95, 0.25]
UC = [0.2, 0.2, 3.0, 0.0, 0.0]
RAW = {1: LG, 2: SV, 3: UC}
T = 7


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def raws_for(model, nth):
    """distinct parameter rows, so that filters cannot stand in for one another"""
    r = np.tile(RAW[model], (nth, 1)).astype(float)
    r[:, 1 if model == 2 else 0] *= 1.0 - 0.3 * np.arange(nth) / max(nth, 1)
    return r


def handle_with_env(L, env, *args, **kw):
    """a handle created under switches that smc_create reads (SMC_STEP_BY_VALUE, SMC_NP)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return L.Handle(*args, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def run(h, y):
    logZ, lm, es = h.log_likelihood(y, trace=True)
    x, w, a = h.state()
    return (logZ, lm, es, x, w, a) + tuple(h.weights_raw())


def oracle_run(ob, model, raw, n, seg, seed, stream, y, systematic=False):
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


def flags_of(L, systematic=False):
    return L.FLAG_NO_RESIDENT | L.FLAG_ANCESTORS | (L.FLAG_SYSTEMATIC if systematic else 0)


# ---- 1. the flagship geometry at its smallest -------------------------------------------------------------------------------------
SEG_F, N_F = 2048, 3 * 2048 + 5      # four segments of 2048 (512 threads x 2 pairs), the last one ragged


@pytest.fixture(scope="module")
def series(ob):
    return {m: ob.simulate(m, RAW[m], T, 1998)[1] for m in RAW}


@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("route", ["by_value", "pointers"])
def test_flagship_geometry_one_filter(L, ob, series, model, route):
    """segments of 2048, eleven levels, four probes per level: one filter by value and the same filter through the view"""
    seed = 7
    env = {} if route == "by_value" else {"SMC_STEP_BY_VALUE": "0"}
    h = handle_with_env(L, env, model, 1, N_F, seg=SEG_F, seed=seed, flags=flags_of(L))
    h.set_params(RAW[model])
    assert h.step_by_value == (route == "by_value") and (h.seg, h.nseg) == (SEG_F, 4) and h.launch_geometry()[:2] == (512, 2)
    s = run(h, series[model])
    h.close()
    assert_matches_oracle(s, oracle_run(ob, model, RAW[model], N_F, SEG_F, seed, 0, series[model]))


@pytest.mark.parametrize("model", [1, 2])
def test_flagship_geometry_batched(L, ob, series, model):
    """three filters with distinct rows and stream ids in one launch"""
    seed, nth = 11, 3
    raws = raws_for(model, nth)
    streams = np.array([4, 0, 9], dtype=np.uint32)
    h = L.Handle(model, nth, N_F, seg=SEG_F, seed=seed, flags=flags_of(L))
    h.set_params(raws)
    h.set_streams(streams)
    assert not h.step_by_value and (h.seg, h.nseg) == (SEG_F, 4)
    s = run(h, series[model])
    h.close()
    for th in range(nth):
        assert_matches_oracle(s, oracle_run(ob, model, raws[th], N_F, SEG_F, seed, int(streams[th]), series[model]), th)


# ---- 2. every unroll count of the interleave ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg,np_env,geo", [(256, None, (128, 1)), (512, None, (256, 1)), (1024, None, (512, 1)),
                                            (2048, "1", (1024, 1)), (2048, "4", (256, 4))])
def test_every_level_count_and_probe_count(L, ob, series, seg, np_env, geo):
    """8, 9, 10 and 11 levels (the slice maps of segments of 256 to 2048) and 2, 4 and 8 probes per level (SMC_NP = 1, 2, 4; the
    flagship's 4 above)"""
    seed, n = 13, 3 * seg + 5
    h = handle_with_env(L, {"SMC_NP": np_env} if np_env else {}, 1, 1, n, seg=seg, seed=seed, flags=flags_of(L))
    h.set_params(LG)
    assert (h.seg, h.nseg) == (seg, 4) and h.launch_geometry()[:2] == geo
    s = run(h, series[1])
    h.close()
    assert_matches_oracle(s, oracle_run(ob, 1, LG, n, seg, seed, 0, series[1]))


# ---- 3. the search left early or replaced -----------------------------------------------------------------------------------------
SEG_S, N_S = 256, 3 * 256 + 5


def test_window_miss_and_far_lanes(L, ob):
    """Very informative observations (R = 1e-4 against a state noise of 1: the recipe of test_uneven_weights_far_segments,
    tests/test_gpu_parity.py) in eight segments of 256: the weights pile into a handful of particles, whole blocks of children
    descend from segments outside the three their workgroup staged (the window misses: the table is re-run, the window reloaded),
    and the children of one block span more than three segments (far lanes: the search in global memory).  Both are read off the
    oracle's ancestors of every step - a block whose ancestors leave [spec_lo, spec_lo + 2] cannot have passed the window test, one
    whose ancestors span more than NSTAGE = 3 segments cannot have staged them all - and then the oracle's bits."""
    seed, seg, nseg = 13, SEG_S, 8
    n = 7 * seg + 5
    raw = [0.9, 1.0, 1.0, 1e-4, 0.0, 4.0]
    _, y = ob.simulate(1, [0.9, 1.0, 1.0, 0.5, 0.0, 4.0], T, 7)
    miss, far = [], []
    for steps in range(2, T + 1):      # the ancestors of step steps - 1
        a = oracle_run(ob, 1, raw, n, seg, seed, 0, y[:steps])[5]
        m = f = 0
        for sb in range(nseg):
            segs = a[sb * seg:(sb + 1) * seg] // seg
            spec_lo = min(max(sb - 1, 0), nseg - 3)
            m += bool(segs.min() < spec_lo or segs.max() > spec_lo + 2)
            f += bool(segs.max() - segs.min() + 1 > 3)
        miss.append(m)
        far.append(f)
    assert sum(1 for m in miss if m) >= 2 and sum(far) >= 1, (miss, far)      # windows miss at several steps; far lanes at one at least
    h = L.Handle(1, 1, n, seg=seg, seed=seed, flags=flags_of(L))
    h.set_params(raw)
    assert (h.seg, h.nseg) == (seg, nseg)
    s = run(h, y)
    h.close()
    assert_matches_oracle(s, oracle_run(ob, 1, raw, n, seg, seed, 0, y))


def test_collapsed_filter(L, ob, series):
    """y[3] = 1e200 kills every weight: the step after it takes identity ancestors in place of the search's result, with the same
    normals (x is the oracle's); then the series to its end"""
    seed = 19
    y = series[1].copy()
    y[3] = 1e200
    for steps in (5, T):
        h = L.Handle(1, 1, N_S, seg=SEG_S, seed=seed, flags=flags_of(L))
        h.set_params(LG)
        s = run(h, y[:steps])
        h.close()
        o = oracle_run(ob, 1, LG, N_S, SEG_S, seed, 0, y[:steps])
        assert o[1][3] == -np.inf
        if steps == 5:
            assert np.array_equal(o[5], np.arange(N_S))
        assert_matches_oracle(s, o)


# ---- 4. one segment, not resident -------------------------------------------------------------------------------------------------
def test_single_segment(L, ob, series):
    """1000 particles in one segment of 1024: the search loop of the single-segment kernel"""
    seed, n, seg = 23, 1000, 1024
    h = L.Handle(1, 1, n, seg=seg, seed=seed, flags=flags_of(L))
    h.set_params(LG)
    assert (h.seg, h.nseg) == (seg, 1) and not h.resident
    s = run(h, series[1])
    h.close()
    assert_matches_oracle(s, oracle_run(ob, 1, LG, n, seg, seed, 0, series[1]))


# ---- 5. the routes that did not move ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,systematic", [(3, False), (1, True)])
def test_unchanged_routes(L, ob, series, model, systematic):
    """UCSV (three state coordinates: every normal is computed whole, at the head at this geometry and next to its use with more
    pairs per thread) and systematic resampling (the normals stay at the head, under the loads)"""
    seed = 29
    h = L.Handle(model, 1, N_S, seg=SEG_S, seed=seed, flags=flags_of(L, systematic))
    h.set_params(RAW[model])
    s = run(h, series[model])
    h.close()
    assert_matches_oracle(s, oracle_run(ob, model, RAW[model], N_S, SEG_S, seed, 0, series[model], systematic=systematic))
