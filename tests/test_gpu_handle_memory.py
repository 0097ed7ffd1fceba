"""The memory of the handles (pytest -m gpu): every device and pinned allocation is an owning block (csrc/smc_host.h, DESIGN.md
"Memory of a handle"), and nothing a caller sees depends on what a block held before.

  a. grow, shrink, regrow: each block's owner call at a small size, a larger one and the small one again on ONE handle equals, bit
     for bit, the same call on a handle that only ever saw that size
  b. recycling: a handle built on the cached bundle of a destroyed, larger one equals a handle built on fresh memory
  c. no leak: smc_live_bytes after twenty create / use / destroy cycles equals smc_live_bytes after ten, both components
  d. SMC_ENOMEM leaves the handle and smc_live_bytes as they were

Shapes: n_theta in {2, 3}, n_x in {64, 300} with seg = 256 (one segment: the LDS-resident kernels; two segments: one launch per
step); T <= 40 except where a recycled series buffer has to grow (60).
"""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
UC = [0.2, 0.3, 1.0, -1.0, -0.5]
LG1D, UCSV_RB = 1, 4
SHAPES = [(2, 64), (3, 64), (2, 300), (3, 300)]
IBIS_M = [2, 3, 64, 300]
LEVELS = [0.25, 0.5, 0.75]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """bit for bit, over whatever a call returns: arrays (floats by their bits), None, and tuples / dicts of them"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)


def rows_for(raw, nth):
    """nth distinct parameter rows around raw"""
    r = np.tile(np.asarray(raw, dtype=float), (nth, 1))
    r[:, 2 if len(raw) != 5 else 0] *= 1.0 + 0.15 * np.arange(nth)
    return r


@pytest.fixture(scope="module")
def series(L):
    return {LG1D: L.simulate(LG1D, LG, 60, 1998)[1], UCSV_RB: L.simulate(UCSV_RB, UC, 60, 1998)[1]}


def handle(L, nth, n, model=LG1D, flags=0):
    h = L.Handle(model, nth, n, seg=256, seed=7, flags=flags)
    h.set_params(rows_for(LG if model == LG1D else UC, nth))
    return h


def record(h, y, cap):
    """a record of `cap` steps of the step API, full"""
    h.history_begin(cap)
    for t in range(cap):
        h.init(float(y[0])) if t == 0 else h.step(float(y[t]))


def sizes_agree(L, make, call, sizes):
    """call(h, size) at every size in turn on ONE handle == call on a handle that only ever saw that size"""
    one = make()
    for s in sizes:
        got = call(one, s)
        fresh = make()
        want = call(fresh, s)
        fresh.close()
        assert same(got, want), s
    one.close()


# ---- a. grow, shrink, regrow -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nth,n", SHAPES)
def test_log_likelihood_trace_and_summaries(L, series, nth, n):
    """d_y, the traces, the per-step records (one segment) and the summary traces: T = 5 / 40 / 5"""
    def make():
        h = handle(L, nth, n)
        h.set_summaries(LEVELS, moments=True)
        return h

    def call(h, T):
        return h.log_likelihood(series[LG1D][:T], trace=True), h.get_summaries(T)

    sizes_agree(L, make, call, (5, 40, 5))


@pytest.mark.parametrize("nth,n", SHAPES)
def test_smooth_pairs_over_two_capacities(L, series, nth, n):
    """the record, the smoother's scratch and results and the pair moments: history capacities 3 / 12 / 3"""
    def call(h, cap):
        record(h, series[LG1D], cap)
        return h.smooth(pairs=True)

    sizes_agree(L, lambda: handle(L, nth, n), call, (3, 12, 3))


@pytest.mark.parametrize("nth,n", SHAPES)
def test_sample_paths(L, series, nth, n):
    """the block of the backward walk: M = 4 / 64 / 4"""
    def make():
        h = handle(L, nth, n)
        record(h, series[LG1D], 6)
        return h

    sizes_agree(L, make, lambda h, M: h.sample_paths(M, 5), (4, 64, 4))


@pytest.mark.parametrize("nth,n", SHAPES)
def test_rb_sample_paths(L, series, nth, n):
    """the same block with the tail of the Rao-Blackwellised walk, on a MODEL_UCSV_RB handle: M = 4 / 64 / 4"""
    y = series[UCSV_RB][:6]

    def make():
        h = handle(L, nth, n, model=UCSV_RB)
        record(h, y, 6)
        return h

    sizes_agree(L, make, lambda h, M: h.rb_sample_paths(y, M, 5, draws=True), (4, 64, 4))


@pytest.mark.parametrize("nth,n", SHAPES)
def test_forecast(L, series, nth, n):
    """the forecast block: H = 2 / 20 / 2"""
    def make():
        h = handle(L, nth, n)
        h.log_likelihood(series[LG1D][:10])
        return h

    sizes_agree(L, make, lambda h, H: h.forecast(H, 3, p=LEVELS), (2, 20, 2))


@pytest.mark.parametrize("nth,n", SHAPES)
def test_set_reference_then_step(L, series, nth, n):
    """the reference of a conditional handle, T = 4 / 12 / 4, and the steps that read it"""
    y = series[LG1D]
    xref = np.random.default_rng(3).normal(size=(12, 1, nth))

    def call(h, T):
        h.set_reference(xref[:T])
        first = h.init(float(y[0]))
        second = h.step(float(y[1]))
        return first, second, h.state(want_anc=False), h.get_reference()

    sizes_agree(L, lambda: handle(L, nth, n, flags=L.FLAG_CONDITIONAL), call, (4, 12, 4))


def ibis_handle(L, M):
    h = L.IbisHandle(M, 1, [L.PRIOR_NORMAL], [[0.0, 1.0, 0.0, 0.0, 0.0]], [0, -1, -1, -1, -1, -1], [0.0, 1.0, 0.9, 0.8, 0.0, 1.0])
    h.set_theta(np.linspace(-0.9, 0.9, M).reshape(M, 1))
    return h


@pytest.mark.parametrize("M", IBIS_M)
def test_ibis_window_with_lik(L, series, M):
    """the series, record and likelihood blocks of an IBIS handle: windows of k = 2 / 8 / 2 (none kept: the state stays)"""
    def call(h, k):
        out = h.window(series[LG1D][:k], want_lik=True)
        h.commit(0)
        return out

    sizes_agree(L, lambda: ibis_handle(L, M), call, (2, 8, 2))


# ---- b. recycling ----------------------------------------------------------------------------------------------------------
def slab_bytes(nth, n, seg=256, d=1):
    """smc_create's slab for a handle without ancestors and without a segment table: every array rounded up to 256 bytes"""
    up = lambda b: (b + 255) & ~255
    nseg = (n + seg - 1) // seg
    cloud, segs = nth * nseg * seg, nth * nseg
    head = up(nth * 128) + up(nth * 4) + up(nth * 4) + up(nth * 8)           # parameter rows, stream ids, permutation, logZ scratch
    buffers = 2 * (up(cloud * d * 8) + up(cloud * 8) + 4 * up(segs * 8))     # x, C and the four segment records, twice
    return head + buffers + 5 * up(nth * 8)                                  # logZ, last_logmu, last_ess, last_K, last_D


@pytest.mark.parametrize("n", [64, 300])
def test_recycled_bundle(L, series, n):
    """a 2 x n handle created after a 3 x n handle was destroyed (its bundle fits: take's rule, below) computes what a 2 x n handle
    on memory of its own computes, also where the recycled series buffer and records have to grow (T = 60)"""
    y = series[LG1D]
    own = handle(L, 2, n)                       # before anything here is destroyed: nothing of this test is in the cache yet
    big = handle(L, 3, n)
    big.log_likelihood(y[:40], trace=True)
    have, want = slab_bytes(3, n), slab_bytes(2, n)
    assert want <= have <= 2 * want + 4096      # BundleCache::take: the slab is large enough and at most twice too large
    assert 4 * 3 * 8 >= 4 * 2 * 8               # ... and so is the pinned mirror
    big.close()
    rec = handle(L, 2, n)
    for T in (40, 60):
        assert same(rec.log_likelihood(y[:T], trace=True), own.log_likelihood(y[:T], trace=True)), T
        assert same(rec.state(want_anc=False), own.state(want_anc=False)), T
    rec.close()
    own.close()


# ---- c. no leak ------------------------------------------------------------------------------------------------------------
def one_cycle(L, series):
    """one handle of each kind, every block of (a) used once, everything closed"""
    y, nth, n = series[LG1D], 2, 64
    h = handle(L, nth, n)
    h.set_summaries(LEVELS, moments=True)
    h.log_likelihood(y[:12], trace=True)
    h.get_summaries(12)
    h.forecast(3, 3, p=LEVELS)
    h.state(want_anc=False)
    h.moments()
    record(h, y, 4)
    h.smooth(pairs=True)
    h.sample_paths(8, 5)
    h.close()
    rb = handle(L, nth, n, model=UCSV_RB)
    record(rb, series[UCSV_RB], 4)
    rb.rb_sample_paths(series[UCSV_RB][:4], 8, 5, draws=True)
    rb.close()
    c = handle(L, nth, n, flags=L.FLAG_CONDITIONAL)
    c.set_reference(np.zeros((4, 1, nth)))
    c.init(float(y[0]))
    c.step(float(y[1]))
    c.close()
    ib = ibis_handle(L, 64)
    ib.window(y[:4], want_lik=True)
    ib.commit(4)
    ib.summary()
    ib.resample(9)
    ib.theta_moments(weighted=True)
    ib.close()


def test_no_leak_over_twenty_cycles(L, series):
    """only differences inside this test count (other tests leave handles to the garbage collector, and the bundle cache keeps what
    it holds): the cache is saturated by these shapes from the second cycle on, so cycles 11 .. 20 must leave nothing behind"""
    at = {}
    for cycle in range(1, 21):
        one_cycle(L, series)
        if cycle in (10, 20):
            gc.collect()
            at[cycle] = L.live_bytes()
    assert at[20] == at[10], (at[10], at[20])


# ---- d. SMC_ENOMEM ---------------------------------------------------------------------------------------------------------
def test_enomem_leaves_handle_and_live_bytes(L, series):
    y = series[LG1D]
    h = handle(L, 2, 300)
    record(h, y, 3)
    before = L.live_bytes()
    assert L.lib().smc_history_begin(h._h, 1 << 50) == -4      # SMC_ENOMEM: an absurd capacity
    assert L.live_bytes() == before
    assert h.history_len() == 3                                # the handle is as it was: the record, and what smooths it
    fresh = handle(L, 2, 300)
    record(fresh, y, 3)
    assert same(h.smooth(), fresh.smooth())
    fresh.close()
    h.close()
