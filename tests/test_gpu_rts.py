"""GPU tests of the RTS smoother of an IBIS cloud (csrc/smc_ibis_smooth_kernels.h: k_ibis_rts_forward / k_ibis_rts_backward /
k_ibis_rts_paths; smc.rts_smoothed_state, rts_quantile, rts_smoothed_paths, kalman_smoother): the device against the host twins
of the same specification with ==, never approx (the twins are pinned to long-double references by tests/test_rts_host.py); the
handle is left as it was; and the exact smoother against the particle smoother of the same cloud."""
import io

import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
from ibis_reference import LG_TRUE, Y_SEED, case_readme

pytestmark = pytest.mark.gpu


def _same(a, b):
    """bit for bit, NaN == NaN included"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _y(T):
    return smc.simulate(smc.UnivariateLinearGaussian(**LG_TRUE), T, seed=Y_SEED)[1]


def _rows(M, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(-0.99, 1.0, M), rng.uniform(0.5, 2.0, M), np.exp(rng.normal(-1, 1, M)), np.exp(rng.normal(-1, 1, M)),
                            rng.normal(0, 1, M), np.exp(rng.normal(0, 0.5, M))])


def _load(rows, logw=None, predict_first=False):
    """a device cloud with the given rows and log-weights: theta IS the row"""
    M = rows.shape[0]
    h = L.IbisHandle(M, 6, [L.PRIOR_NORMAL] * 6, np.tile([0.0, 1.0, 0.0, 0.0, 0.0], (6, 1)), [0, 1, 2, 3, 4, 5], [0.0] * 6,
                     predict_first=predict_first)
    h.set_theta(rows)
    if logw is not None:
        h.set_logw(logw)
    return h


def _check_smooth(h, rows, logw, y, predict_first):
    got = h.smooth(y, states=True)
    want = L.host_ibis_smooth(rows, logw, y, predict_first, states=True)
    for g, w, name in zip(got, want, ("out", "xs", "Ps")):
        assert _same(g, w), name
    assert _same(h.smooth(y), want[0])                                      # the kernel that stores no states


@pytest.mark.parametrize("M", [1, 63, 64, 65, 300, 4097])
def test_smooth_equals_host_twin(M):
    """a lone lane, either side of a chunk, a tail, many chunks; T = 1, 2, 12; both predict_first: out, xs, Ps bit for bit"""
    rows = _rows(M, 100 + M)
    logw = np.random.default_rng(M).normal(0, 3, M)
    for predict_first in (False, True):
        h = _load(rows, None, predict_first)
        _check_smooth(h, rows, np.zeros(M), _y(12), predict_first)          # the cloud after set_theta
        h.set_logw(logw)
        for T in (1, 2, 12):
            _check_smooth(h, rows, logw, _y(T), predict_first)
        h.close()


def test_smooth_with_dead_particles():
    """set_logw with -inf and NaN entries, and with every entry dead: out, xs, Ps bit for bit.  Then rows no filter could run on
    planted on the dead particles: out keeps its bits, the live particles' xs, Ps keep theirs (what the dead ones hold there is
    NaN on both sides; which NaN is the processor's choice, not the specification's)"""
    M = 300
    rows = _rows(M, 9)
    rng = np.random.default_rng(10)
    logw = rng.normal(0, 3, M)
    dead = rng.uniform(size=M) < 0.4
    dead[[0, 63, 64, M - 1]] = True
    dead[128:192] = True                                                   # a whole chunk
    logw[dead] = -np.inf
    logw[dead & (np.arange(M) % 3 == 0)] = np.nan
    y = _y(12)
    h = _load(rows, logw)
    _check_smooth(h, rows, logw, y, False)
    out, xs, Ps = h.smooth(y, states=True)
    assert np.isfinite(out).all()
    h.set_logw(np.full(M, -np.inf))                                        # no live particle
    _check_smooth(h, rows, np.full(M, -np.inf), y, False)
    assert np.isnan(h.smooth(y)[:, :6]).all()
    h.close()
    planted = rows.copy()
    planted[dead, 0], planted[dead, 5] = np.nan, np.inf
    h = _load(planted, logw)
    pout, pxs, pPs = h.smooth(y, states=True)
    assert _same(pout, out) and _same(pout, L.host_ibis_smooth(planted, logw, y))
    assert _same(pxs[:, ~dead], xs[:, ~dead]) and _same(pPs[:, ~dead], Ps[:, ~dead]) and np.isnan(pxs[:, dead]).all()
    h.close()


def _sampler(M, predict_first, device_moves, seed=5):
    tmap, prior, model = case_readme(smc)
    return smc.IBIS(M, model, prior, 3, 0.5, seed=seed, theta_map=tmap, predict_first=predict_first, device_moves=device_moves), tmap


@pytest.mark.parametrize("device_moves,predict_first", [(False, False), (True, False), (False, True)])
def test_smooth_after_a_sampler_run(device_moves, predict_first):
    """a real smc2_run with rejuvenations (M = 300: the last chunk is short): the device against the twin on the arrays read
    back; the last row is the filtered cloud; nothing of the sampler changes, and the run goes on as if never asked"""
    T = 40
    y = _y(60)
    ib, tmap = _sampler(300, predict_first, device_moves)
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, T, verbose=False, out=io.StringIO())
    assert ib.n_rejuvenations > 0
    before = ib._h.get(theta=True, x=True, S=True, logZ=True, logw=True)
    rows = tmap.rows(before["theta"])
    _check_smooth(ib._h, rows, before["logw"], y[:T], predict_first)
    out = ib._h.smooth(y[:T])
    assert _same(out[T - 1], ib._h.summary(0))
    mean, var = smc.rts_smoothed_state(ib, y[:T])
    assert _same(mean, out[:, 3]) and _same(var, out[:, 4] + out[:, 5])
    paths = smc.rts_smoothed_paths(ib, y[:T], 65)
    which = L.host_outer_resample(before["logw"], 65, ((5 << 20) | 0x4754B) + 1)
    assert np.all(np.diff(which) >= 0)
    assert _same(paths, L.host_ibis_sample_paths(rows, y[:T], which, ((5 << 20) | 0x4754B) + 2, predict_first))
    after = ib._h.get(theta=True, x=True, S=True, logZ=True, logw=True)
    for k in before:
        assert _same(before[k], after[k]), k
    other, _ = _sampler(300, predict_first, device_moves)                  # the same run without the calls
    smc.smc2(other, y)
    smc.smc2_run(other, y, 2, T, verbose=False, out=io.StringIO())
    for s in (ib, other):
        smc.smc2_run(s, y, T + 1, 60, verbose=False, out=io.StringIO())
    assert _same(ib.theta, other.theta) and _same(ib.logw, other.logw) and _same(ib.logZ, other.logZ) and _same(ib.x, other.x)
    assert ib.n_rejuvenations == other.n_rejuvenations and ib.rng.bit_generator.state == other.rng.bit_generator.state
    ib.close()
    other.close()


@pytest.mark.parametrize("predict_first", [False, True])
def test_sample_paths_equals_host_twin(predict_first):
    """Mp = 1, 63, 65, 300; `which` with repeats and the last particle; path p alone == path p in a batch"""
    M, T, seed = 130, 12, 0x9E3779B97F4A7C15
    rows = _rows(M, 11)
    y = _y(T)
    h = _load(rows, None, predict_first)
    which = np.sort(np.random.default_rng(12).integers(0, M, 300)).astype(np.int32)
    which[-3:] = M - 1
    which[:4] = 0
    assert len(np.unique(which)) < 300
    batch = h.sample_paths(y, which, seed)
    assert _same(batch, L.host_ibis_sample_paths(rows, y, which, seed, predict_first))
    for Mp in (1, 63, 65):
        got = h.sample_paths(y, which[:Mp], seed)
        assert _same(got, batch[:, :Mp]), Mp
    assert _same(h.sample_paths(y[:1], which, seed), L.host_ibis_sample_paths(rows, y[:1], which, seed, predict_first))
    assert _same(h.sample_paths(y[:2], which[::-1].copy(), seed), L.host_ibis_sample_paths(rows, y[:2], which[::-1].copy(), seed, predict_first))
    assert _same(h.sample_paths(y, which, seed), batch)                     # again: the same bits
    assert not _same(h.sample_paths(y, which, seed + 1), batch)
    h.close()


@pytest.mark.parametrize("predict_first", [False, True])
def test_kalman_smooth_is_the_per_particle_half(predict_first):
    M = 300
    rows = _rows(M, 13)
    h = _load(rows, None, predict_first)
    for T in (1, 12):
        y = _y(T)
        _, xs, Ps = h.smooth(y, states=True)
        kx, kP = L.kalman_smooth(rows, y, predict_first)
        assert _same(kx, xs) and _same(kP, Ps)
    h.close()


def test_python_layer_shapes():
    T, M = 12, 200
    y = _y(T)
    ib, tmap = _sampler(M, False, False)
    for started in (False, True):                                          # before the first sampler call: the host twin
        if started:
            smc.smc2(ib, y)
            smc.smc2_run(ib, y, 2, T, verbose=False, out=io.StringIO())
        mean, var = smc.rts_smoothed_state(ib, y)
        assert mean.shape == var.shape == (T,) and np.all(var > 0)
        parts = smc.rts_smoothed_state(ib, y, parts=True)
        assert sorted(parts) == sorted(["y", "Sigma", "between", "xbar", "Sbar", "between_x"]) and all(v.shape == (T,) for v in parts.values())
        assert _same(parts["xbar"], mean) and _same(parts["Sbar"] + parts["between_x"], var)
        q = smc.rts_quantile(ib, y, [0.75, 0.25, 0.5])
        assert q.shape == (T, 3) and np.all(np.diff(q, axis=1) > 0) and np.allclose(q[:, 1], mean)
        assert smc.rts_quantile(ib, y, 0.5).shape == (T,)
        assert np.all(smc.rts_quantile(ib, y, 0.75, total=False) <= q[:, 2])
        paths = smc.rts_smoothed_paths(ib, y, 77)
        assert paths.shape == (T, 77) and np.isfinite(paths).all()
        assert _same(paths, smc.rts_smoothed_paths(ib, y, 77)) and not _same(paths, smc.rts_smoothed_paths(ib, y, 77, seed=3))
    ib.close()
    models = [smc.UnivariateLinearGaussian(A=0.5 + 0.1 * i, B=1.0, Q=0.9, R=0.8) for i in range(3)]
    xs, Ps = smc.kalman_smoother(y, models)
    assert xs.shape == Ps.shape == (T, 3)
    x0, P0 = smc.kalman_smoother(y, models[0])
    assert x0.shape == (T,) and _same(x0, xs[:, 0]) and _same(P0, Ps[:, 0])
    x1, _ = smc.kalman_smoother(y, models[1], predict_first=True)
    assert not _same(x1, xs[:, 1])
    with pytest.raises(TypeError):
        smc.kalman_smoother(y, smc.StochasticVolatility(0.0, 0.9, 0.3))


def test_exact_smoother_against_the_particle_smoother():
    """An SMC sampler and an IBIS sampler with the same theta cloud (the same seed draws it) and the same outer weights:
    smoothed_state(SMC, N = 1024), the FFBS particle smoother of every parameter particle, over 8 filter seeds, against
    rts_smoothed_state: |mean over the seeds - exact| <= 4.5 SE at every t, SE = sd over the seeds / sqrt(8)."""
    T, M, N, K = 12, 16, 1024, 8
    y = _y(T)
    tmap, prior, model = case_readme(smc)
    ib = smc.IBIS(M, model, prior, 3, 0.5, seed=7, theta_map=tmap)
    sm = smc.SMC(N, M, model, prior, 3, 0.5, seed=7, theta_map=tmap)
    assert _same(ib.theta, sm.theta)
    logw = np.random.default_rng(70).normal(0, 1, M)
    ib._handle().set_logw(logw)
    sm._set_logw(logw)
    exact, exact_var = smc.rts_smoothed_state(ib, y)
    means = np.array([smc.smoothed_state(sm, y, N=N, seed=1000 + k)[0] for k in range(K)])
    se = means.std(axis=0, ddof=1) / np.sqrt(K)
    z = np.abs(means.mean(axis=0) - exact) / se
    print("z of the particle smoother against the exact one: %s (SE / sd of the state: %s)" % (np.round(z, 2), np.round(se / np.sqrt(exact_var), 4)))
    assert np.all(z <= 4.5), z
    ib.close()
    sm.backend.close()


def test_error_paths():
    M = 65
    rows = _rows(M, 14)
    y = _y(12)
    h = _load(rows)
    which = np.zeros(5, dtype=np.int32)
    h.window(y[:3])                                                        # a pending window: refused, nothing changes
    with pytest.raises(L.SmcError, match="error -3"):
        h.smooth(y)
    with pytest.raises(L.SmcError, match="error -3"):
        h.sample_paths(y, which, 1)
    h.commit(3)
    with pytest.raises(L.SmcError, match="error -3"):                      # nothing timed yet
        h.last_elapsed_ms()
    out = h.smooth(y)
    assert h.last_elapsed_ms() > 0
    for bad in ([M], [-1], [0, 1, M, 2]):
        with pytest.raises(L.SmcError, match="error -1"):
            h.sample_paths(y, np.array(bad, dtype=np.int32), 1)
    with pytest.raises(L.SmcError, match="error -1"):
        h.sample_paths(y, np.zeros(0, dtype=np.int32), 1)
    with pytest.raises(L.SmcError, match="error -1"):
        h.smooth(np.zeros(0))
    with pytest.raises(L.SmcError, match="error -1"):
        h.sample_paths(np.zeros(0), which, 1)
    with pytest.raises(L.SmcError, match="error -1"):
        L.kalman_smooth(rows, np.zeros(0))
    assert _same(h.smooth(y), out)
    h.close()
    fresh = L.IbisHandle(M, 6, [L.PRIOR_NORMAL] * 6, np.tile([0.0, 1.0, 0.0, 0.0, 0.0], (6, 1)), [0, 1, 2, 3, 4, 5], [0.0] * 6)
    with pytest.raises(L.SmcError, match="error -3"):                      # no theta yet
        fresh.smooth(y)
    fresh.close()
