"""The device paths of the FFBS smoother that a filter run of the sizes in tests/test_gpu_smoother.py never reaches (pytest -m gpu):

  * tiles of 256 owners (only half of the workgroup stages the chunk), bit for bit against smc_host_smooth, and the same filter
    under both tile lengths and alone
  * collapsed filters: a natural collapse, and one filter of a batch planted dead (smc_history_put) next to untouched neighbours
  * the planted clouds of tests/smoother_planted.py, device == host twin bit for bit (the twin is pinned to the long-double
    recursion on the same clouds by tests/test_smoother_host.py)
  * more than 256 chunks (the strided chunk loop of the moments, the row maxima), against exact sums
  * a handle that is armed again and again; the rules of smc_history_put; the refusal of more than 65535 chunks
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import smoother_planted as P
import smoother_reference as R
import test_gpu_smoother as G

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LG, LG_SHARP, SV, UC = G.LG, G.LG_SHARP, G.SV, G.UC
same, rows_for, run_recorded, clouds = G.same, G.rows_for, G.run_recorded, G.clouds
OK, EINVAL, ESTATE = 0, -1, -3


def host_twins(L, model, rows, x, w, filters):
    """{m: (ws, mean, var)} of smc_host_smooth on the clouds of the filters asked for (the calls are independent: a few threads)"""
    with ThreadPoolExecutor(max_workers=8) as pool:
        res = pool.map(lambda m: L.host_smooth(model, rows[m], x[:, :, m, :], w[:, m, :]), filters)
        return dict(zip(filters, res))


def check_moments(x, ws, mean, var):
    """mean, var [T][d] of one filter against exactly rounded sums, the bounds of DESIGN.md section 2"""
    for t in range(x.shape[0]):
        for r in range(x.shape[1]):
            em, ev = R.exact_moments(x[t, r], ws[t])
            assert abs(mean[t, r] - em) <= G.MEAN_REL * abs(em) + G.MEAN_SD * np.sqrt(ev), (t, r)
            assert var[t, r] >= 0 and abs(var[t, r] - ev) <= G.VAR_REL * ev + (G.VAR_LEVEL * em) ** 2, (t, r)


def check_against_twin(L, model, rows, x, w, out, filters):
    """weights and moments of the device == the host twin's, bit for bit, for the filters asked for; moments against exact sums"""
    ws, mean, var = out
    twins = host_twins(L, model, rows, x, w, filters)
    for m in filters:
        hs, hm, hv = twins[m]
        assert same(ws[:, m], hs), ("weights", m)
        assert same(mean[:, :, m], hm) and same(var[:, :, m], hv), ("moments", m)
        assert np.all(np.isfinite(ws[:, m]))
        check_moments(x[:, :, m, :], ws[:, m], mean[:, :, m], var[:, :, m])


def put_filter(h, m, x, w, px, pw):
    """the clouds (px [T][d][n], pw [T][n]) into filter m of every recorded step, the other filters as recorded in (x, w)"""
    for t in range(x.shape[0]):
        xt, wt = x[t].copy(), w[t].copy()
        xt[:, m, :], wt[m] = px[t], pw[t]
        h.history_put(t, xt, wt)


def same_out(a, b, filters=None):
    if filters is None:
        return all(same(u, v) for u, v in zip(a, b))
    return all(same(a[0][:, m], b[0][:, m]) and same(a[1][:, :, m], b[1][:, :, m]) and same(a[2][:, :, m], b[2][:, :, m]) for m in filters)


# ---- a. tiles of 256 owners ---------------------------------------------------------------------------------------------------
# (model, row, n, seg, n_theta, T): a ragged last tile and a partial last chunk in a batch (1300 / 256); many filters of two tiles
# and three chunks; one long filter whose last tile has 168 owners and whose last chunk has 40 particles, more than
# SMOOTH_MAX_DIRECT chunks; the smallest launch that takes the long tile, whole tiles only
WIDE = [
    (1, LG, 1300, 256, 16, 3),
    (3, UC, 300, 256, 171, 3),
    (1, LG, 5800, 0, 1, 2),
    (2, SV, 1024, 0, 32, 2),
]


@pytest.mark.parametrize("model,raw,n,seg,nth,T", WIDE)
def test_wide_tiles_equal_host_twin(L, model, raw, n, seg, nth, T):
    rows = rows_for(raw, nth)
    h = run_recorded(L, model, rows, n, seg, T, streams=np.arange(nth))
    x, w = clouds(h)
    out = h.smooth()
    check_against_twin(L, model, rows, x, w, out, range(nth))
    assert same(out[0][T - 1], w[T - 1])
    assert same_out(out, h.smooth())
    if model == 3:
        # the same filters in a batch one smaller, which is cut into tiles of one wave, and three of them alone: the same bits
        hb = run_recorded(L, model, rows[:nth - 1], n, seg, T, streams=np.arange(nth - 1))
        assert same_out(hb.smooth(), out, range(nth - 1))
        hb.close()
        for m in (0, nth // 2, nth - 2):
            h1 = run_recorded(L, model, rows[m], n, seg, T, streams=[m])
            o1 = h1.smooth()
            assert same(o1[0][:, 0], out[0][:, m]) and same(o1[1][:, :, 0], out[1][:, :, m]) and same(o1[2][:, :, 0], out[2][:, :, m]), m
            h1.close()
    h.close()


# ---- b. collapse ----------------------------------------------------------------------------------------------------------------
def test_natural_collapse_is_nan_everywhere(L):
    """an observation no particle explains at t = 3, ordinary steps after it (the filter recovers): NaN at every t"""
    T, nth = 6, 3
    rows = rows_for(SV, nth)
    _, y = L.simulate(2, SV, T, 1998)
    h = L.Handle(2, nth, 300, seg=256, seed=11)
    h.set_params(rows)
    h.history_begin(T)
    for t in range(T):
        yt = 1e200 if t == 3 else float(y[t])
        h.init(yt) if t == 0 else h.step(yt)
    _, w = clouds(h)
    assert not (w[3] > 0).any() and np.all((w[[0, 1, 2, 4, 5]] > 0).any(axis=2))
    ws, mean, var = np.zeros((T, nth, 300)), np.zeros((T, 1, nth)), np.zeros((T, 1, nth))
    assert L.lib().smc_smooth(h._h, L._d(ws), L._d(mean), L._d(var)) == OK
    assert np.all(np.isnan(ws)) and np.all(np.isnan(mean)) and np.all(np.isnan(var))
    h.close()


@pytest.mark.parametrize("n,seg,nth,T", [(300, 256, 3, 6), (1300, 256, 16, 3)])
def test_one_dead_filter_of_a_batch(L, n, seg, nth, T):
    """filter 1 planted dead at the first, a middle and the last step: NaN everywhere for it, the bits of the plain run for its
    neighbours; with the step put back, its own bits again (the flags are cleared by every call)"""
    rows = rows_for(LG, nth)
    h = run_recorded(L, 1, rows, n, seg, T, streams=np.arange(nth))
    x, w = clouds(h)
    base = h.smooth()
    assert np.all(np.isfinite(base[0])) and np.all(np.isfinite(base[1])) and np.all(np.isfinite(base[2]))
    others = [m for m in range(nth) if m != 1]
    for t_dead in P.dead_steps(T):
        wd = w[t_dead].copy()
        wd[1] = 0.0
        h.history_put(t_dead, w=wd)
        out = h.smooth()
        assert np.all(np.isnan(out[0][:, 1])) and np.all(np.isnan(out[1][:, :, 1])) and np.all(np.isnan(out[2][:, :, 1])), t_dead
        assert same_out(out, base, others), t_dead
        h.history_put(t_dead, w=w[t_dead])
        assert same_out(h.smooth(), base), t_dead
    h.close()


# ---- c. planted clouds ------------------------------------------------------------------------------------------------------------
PLANTED = [
    (1, LG, 300, 256, 3, 6, P.ALIVE),
    (1, LG_SHARP, 300, 256, 3, 6, P.ON_ZERO + P.ALIVE),
    (2, SV, 300, 256, 3, 6, P.ALIVE),
    (3, UC, 300, 256, 3, 6, P.ALIVE),
    (1, LG, 1300, 256, 16, 3, P.ALIVE),
    (1, LG_SHARP, 1300, 256, 16, 3, P.ON_ZERO + P.ALIVE),
]


@pytest.mark.parametrize("model,raw,n,seg,nth,T,names", PLANTED)
def test_planted_clouds_equal_host_twin(L, model, raw, n, seg, nth, T, names):
    rows = rows_for(raw, nth)
    h = run_recorded(L, model, rows, n, seg, T, streams=np.arange(nth))
    x, w = clouds(h)
    base = h.smooth()
    check_against_twin(L, model, rows, x, w, base, [1])
    others = [m for m in range(nth) if m != 1]
    for name in names:
        px, pw = P.variant(name, model, rows[1], x[:, :, 1, :], w[:, 1, :])
        put_filter(h, 1, x, w, px, pw)
        out = h.smooth()
        assert same_out(out, base, others), name
        x2, w2 = x.copy(), w.copy()
        x2[:, :, 1, :], w2[:, 1, :] = px, pw
        check_against_twin(L, model, rows, x2, w2, out, [1])
        assert np.all(out[0][:, 1][pw == 0] == 0), name
        if name in P.ON_ZERO:
            assert (pw == 0).mean() > 0.5 and not np.all(np.isfinite(px))
            assert same_out(out, base), name            # left out whatever their states
        else:
            assert not same(out[0][:, 1], base[0][:, 1]), name
    put_filter(h, 1, x, w, x[:, :, 1, :], w[:, 1, :])
    assert same_out(h.smooth(), base)
    h.close()


# ---- d. more than 256 chunks ---------------------------------------------------------------------------------------------------
def test_more_chunks_than_threads(L):
    """n = 32833: 257 chunks, the last of 65 particles, so one thread of the moments' workgroup takes two chunks.  The host twin
    would take minutes, so the properties that need no twin: ws_T = w_T, the zeros, the sum within the twin's own bound against
    the long-double recursion, exact moments, repeatability"""
    n, T = 32833, 2
    assert -(-n // L.SMOOTH_CH) == 257 and n % L.SMOOTH_CH != 0
    h = run_recorded(L, 1, np.array([LG]), n, 0, T)
    x, w = clouds(h)
    out = h.smooth()
    ws, mean, var = out
    assert same(ws[1], w[1])
    assert np.all(np.isfinite(ws[0])) and np.all(ws[0] >= 0) and np.all(ws[0][w[0] == 0] == 0)
    tot = float(abs(R.exact_sum(ws[0, 0], 0) - 1))
    bound = (2 * (L.SMOOTH_CH + n / L.SMOOTH_CH) + 200) * EPS
    print("|sum ws_0 - 1| = %.3g, bound %.3g" % (tot, bound))
    assert tot <= bound
    check_moments(x[:, :, 0, :], ws[:, 0], mean[:, :, 0], var[:, :, 0])
    assert same_out(h.smooth(), out)
    h.close()


# ---- e. arming an armed handle ---------------------------------------------------------------------------------------------------
def test_rearmed_handle_equals_fresh_handles(L):
    """records of 3, 14 and 2 steps on one handle (the smoothed weights and the moments share one allocation that is sized by
    the longest record so far), and a short smooth inside the long record before it grows: each the bits of a fresh handle"""
    n, seg, nth = 300, 256, 2
    rows = rows_for(LG, nth)
    _, y = L.simulate(1, LG, 14, 1998)
    fresh = {}
    for T in (2, 3, 14):
        hf = run_recorded(L, 1, rows, n, seg, T)
        fresh[T] = hf.smooth()
        hf.close()
    h = L.Handle(1, nth, n, seg=seg, seed=11)
    h.set_params(rows)
    for cap in (3, 14, 2):
        h.history_begin(cap)
        assert h.history_len() == 0
        for t in range(cap):
            h.init(float(y[0])) if t == 0 else h.step(float(y[t]))
            if cap == 14 and t == 1:
                assert same_out(h.smooth(), fresh[2])
        assert h.history_len() == cap
        assert same_out(h.smooth(), fresh[cap]), cap
    h.close()


# ---- f. smc_history_put ---------------------------------------------------------------------------------------------------------
def test_history_put_rules(L):
    lib = L.lib()
    _, y = L.simulate(1, LG, 3, 1998)
    h = L.Handle(1, 2, 300, seg=256, seed=3)
    h.set_params(rows_for(LG, 2))
    z = np.zeros((1, 2, 300))
    assert lib.smc_history_put(h._h, 0, L._d(z), None) == ESTATE      # not armed
    h.history_begin(4)
    assert lib.smc_history_put(h._h, 0, L._d(z), None) == EINVAL      # armed, nothing recorded: t = len
    h.init(float(y[0]))
    h.step(float(y[1]))
    snap = h.state(want_anc=False)
    rec = [h.history_get(t) for t in range(2)]
    assert lib.smc_history_put(h._h, 2, L._d(z), None) == EINVAL      # t = len
    assert lib.smc_history_put(h._h, -1, L._d(z), None) == EINVAL
    assert lib.smc_history_put(h._h, 1, None, None) == OK             # nothing to put
    rng = np.random.default_rng(7)
    px, pw = rng.normal(size=(1, 2, 300)), rng.uniform(size=(2, 300))
    px[0, 0, :3] = [np.nan, np.inf, -0.0]
    pw[1, :3] = [0.0, 2.0 ** -1074, 1.0]
    h.history_put(1, x=px)                                            # x alone: w stays
    gx, gw = h.history_get(1)
    assert same(gx, px) and same(gw, rec[1][1])
    h.history_put(0, w=pw)                                            # w alone: x stays
    gx, gw = h.history_get(0)
    assert same(gx, rec[0][0]) and same(gw, pw)
    h.history_put(1, px, pw)
    gx, gw = h.history_get(1)
    assert same(gx, px) and same(gw, pw)
    gx, gw = h.history_get(0)
    assert same(gx, rec[0][0]) and same(gw, pw)                       # the other step is untouched
    st = h.state(want_anc=False)
    assert same(st[0], snap[0]) and same(st[1], snap[1]) and h.history_len() == 2
    with pytest.raises(ValueError):
        h.history_put(0, x=np.zeros((1, 2, 299)))
    # the filter goes on from its own state, not from the record
    h.history_put(0, *rec[0])
    h.history_put(1, *rec[1])
    h.step(float(y[2]))
    ref = run_recorded(L, 1, rows_for(LG, 2), 300, 256, 3, seed=3)
    assert same(h.state(want_anc=False)[0], ref.state(want_anc=False)[0]) and same_out(h.smooth(), ref.smooth())
    h.history_end()
    assert lib.smc_history_put(h._h, 0, L._d(z), None) == ESTATE
    for hh in (h, ref):
        hh.close()


# ---- g. more chunks than a launch can index ----------------------------------------------------------------------------------
def test_too_many_chunks_are_refused(L):
    """65535 chunks is the most the grid of the pair kernels holds: one particle more is refused before anything is launched or
    allocated, whatever the number of recorded steps, and the handle is as it was"""
    lib = L.lib()
    n = 65535 * L.SMOOTH_CH + 1
    h = L.Handle(1, 1, n, seed=3)
    h.set_params(np.array([LG]))
    h.history_begin(1)
    h.init(0.3)
    snap = h.state(want_anc=False)
    ws = np.full((1, 1, n), -1.0)
    assert lib.smc_smooth(h._h, L._d(ws), None, None) == EINVAL
    assert b"65535 chunks" in lib.smc_last_error() and np.all(ws == -1.0)
    st = h.state(want_anc=False)
    assert same(st[0], snap[0]) and same(st[1], snap[1]) and h.history_len() == 1
    assert same(h.history_get(0)[1], snap[1])
    h.close()
