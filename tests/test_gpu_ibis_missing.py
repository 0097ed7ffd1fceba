"""GPU tests of missing observations on the exact-Kalman side (IBIS(..., missing=True), smc_ibis_set_flags, the *_flags calls;
DESIGN.md 2j): every kernel that loops kalman_step, through a NaN, against the host twins (smc_host_kalman_steps,
smc_host_ibis_smooth_flags, smc_host_ibis_sample_paths_flags, smc_host_outer_window / _walk, smc_host_ibis_summary) and against
the restatement of tests/ibis_missing_reference.py - every float64 array with ==.

Shapes: T = 12; M over the outer segment of 8 and the wave / workgroup / summary chunk of 64, partial and crossed; both
predict_first settings; the gap sets none, first, last, the first two, an inner run, all."""
import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
from ibis_reference import LG_TRUE, Y_SEED, case_readme
from ibis_missing_reference import IbisMissingReference, with_gaps
import test_gpu_ibis_device_moves as DM

pytestmark = pytest.mark.gpu

T = 12
SIZES = [1, 7, 8, 9, 63, 64, 65, 130, 513]
GAP_SETS = [(), (0,), (T - 1,), (0, 1), (3, 4, 5), tuple(range(T))]
FLAG = L.FLAG_NAN_MISSING
NAMES = ("theta", "x", "S", "logZ", "logw")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _y(n=T):
    return smc.simulate(smc.UnivariateLinearGaussian(**LG_TRUE), n, seed=Y_SEED)[1]


def _ibis(M, predict_first=False, seed=5, missing=True, **kw):
    tmap, prior, model = case_readme(smc)
    return smc.IBIS(M, model, prior, 3, 0.5, seed=seed, theta_map=tmap, predict_first=predict_first, missing=missing, **kw)


def _handle(ib, flags=FLAG):
    """a fresh handle on the sampler's initial cloud"""
    fam, par = ib.prior_spec
    h = L.IbisHandle(ib.M, ib._theta0.shape[1], fam, par, ib.theta_map.raw_from, ib.theta_map.raw_const, seed=ib.seed,
                     predict_first=ib.predict_first, flags=flags)
    h.set_theta(ib._theta0)
    return h


def _state(h):
    return h.get(theta=True, x=True, S=True, logZ=True, logw=True)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


_HOST = {}


def host_record(ib, y, missing=True):
    """(rows [M][6], xf, Sf, lik [T][M]) of the host twin of the step loop, one row at a time; computed once per case"""
    key = (ib.M, ib.predict_first, ib.seed, bits(y).tobytes(), missing)
    if key not in _HOST:
        rows = ib.theta_map.rows(ib._theta0)
        rec = [L.host_kalman_steps(r, y, ib.predict_first, missing=missing) for r in rows]
        _HOST[key] = (rows,) + tuple(np.ascontiguousarray(np.stack([r[i] for r in rec], axis=1)) for i in range(3))
    return _HOST[key]


def run_sum(lik):
    """logw / logZ after the steps of lik [k][M] from 0.0, in step order"""
    z = np.zeros(lik.shape[1])
    for l in lik:
        z = z + l
    return z


@pytest.mark.parametrize("predict_first", [False, True])
@pytest.mark.parametrize("gaps", GAP_SETS, ids=str)
@pytest.mark.parametrize("M", SIZES)
def test_windows_equal_host_twins(M, gaps, predict_first):
    """smc_ibis_window (lik, records, the rows of the summaries at ahead = 0) and smc_ibis_window_ess (ess, j, the rows at ahead
    = 1) over the series in windows of 1, 5 and 12: lik == the host twin's, rec == smc_host_outer_window on the log-weights
    before the window, (ess, j) == smc_host_outer_walk, every row == smc_host_ibis_summary on the host record, the committed
    state == the host record; lik at a gap is +0.0 (the bits) and the ESS of a gap is the previous step's"""
    y = with_gaps(_y(), gaps)
    ib = _ibis(M, predict_first)
    rows, xf, Sf, lik = host_record(ib, y)
    assert np.all(np.isfinite(xf)) and not bits(lik[list(gaps)]).any()
    h, g = _handle(ib), _handle(ib)
    h.set_summaries(True, 0)
    g.set_summaries(True, 1)
    for k in (1, 5, 12):
        for hh in (h, g):
            hh.set_theta(ib._theta0)
        logw, trace = np.zeros(M), []
        for lo in range(0, T, k):
            n = min(k, T - lo)
            rec, dl = h.window(y[lo:lo + n], want_lik=True)
            assert np.array_equal(bits(dl), bits(lik[lo:lo + n])), (k, lo)
            assert np.array_equal(rec, L.host_outer_window(logw, dl)), (k, lo)
            ref, jr = L.host_outer_walk(rec, M, 0.0)
            ess, j = g.window_ess(y[lo:lo + n], 0.0)
            assert j == jr == n and np.array_equal(ess, ref), (k, lo)
            trace.extend(ess.tolist())
            s0, s1 = h.get_summaries(n), g.get_summaries(n)
            for i in range(n):
                logw = logw + lik[lo + i]
                assert _same(s0[i], L.host_ibis_summary(rows, xf[lo + i], Sf[lo + i], logw, 0)), (k, lo, i)
                assert _same(s1[i], L.host_ibis_summary(rows, xf[lo + i], Sf[lo + i], logw, 1)), (k, lo, i)
            for hh in (h, g):
                hh.commit(n)
                st = _state(hh)
                assert np.array_equal(st["x"], xf[lo + n - 1]) and np.array_equal(st["S"], Sf[lo + n - 1]), (k, lo)
                assert np.array_equal(bits(st["logw"]), bits(logw)) and np.array_equal(bits(st["logZ"]), bits(logw)), (k, lo)
        for t in gaps:
            assert trace[t] == (trace[t - 1] if t > 0 else float(M)), (k, t)
    h.close()
    g.close()


@pytest.mark.parametrize("predict_first", [False, True])
@pytest.mark.parametrize("M", [9, 65, 513])
def test_cut_window_then_a_window_of_gaps(M, predict_first):
    """a window of 5 of which 3 steps are kept (the prefix is re-run in place), so the next window begins with a gap - and is
    all gaps (3, 4, 5); then the rest: the same state as the host record, whatever the windows were"""
    y = with_gaps(_y(), (3, 4, 5))
    ib = _ibis(M, predict_first)
    rows, xf, Sf, lik = host_record(ib, y)
    h = _handle(ib)
    h.window(y[:5])
    h.commit(3)
    st = _state(h)
    assert np.array_equal(st["x"], xf[2]) and np.array_equal(st["S"], Sf[2]) and np.array_equal(st["logZ"], run_sum(lik[:3]))
    rec, dl = h.window(y[3:6], want_lik=True)
    assert not bits(dl).any()
    assert np.array_equal(rec, L.host_outer_window(st["logw"], dl)) and np.array_equal(rec[0], rec[1]) and np.array_equal(rec[0], rec[2])
    h.commit(3)
    st2 = _state(h)
    assert np.array_equal(bits(st2["logZ"]), bits(st["logZ"])) and np.array_equal(bits(st2["logw"]), bits(st["logw"]))
    assert np.array_equal(st2["x"], xf[5]) and np.array_equal(st2["S"], Sf[5])
    h.window(y[6:])
    h.commit(T - 6)
    st3 = _state(h)
    assert np.array_equal(st3["x"], xf[-1]) and np.array_equal(st3["S"], Sf[-1]) and np.array_equal(st3["logZ"], run_sum(lik))
    h.close()


@pytest.mark.parametrize("predict_first", [False, True])
@pytest.mark.parametrize("gaps", GAP_SETS, ids=str)
@pytest.mark.parametrize("M", [7, 65, 513])
def test_filter_and_batched_kalman_equal_the_online_state(M, gaps, predict_first):
    """smc_ibis_filter and the flagged smc_kalman_log_likelihood: (x, S, logZ) == the per-particle online state == the host"""
    y = with_gaps(_y(), gaps)
    ib = _ibis(M, predict_first)
    rows, xf, Sf, lik = host_record(ib, y)
    h = _handle(ib)
    h.window(y)
    h.commit(T)
    on = _state(h)
    h.filter(y)
    st = _state(h)
    out = L.kalman_log_likelihood(rows, y, predict_first, missing=True)
    for name, col, ref in (("x", 0, xf[-1]), ("S", 1, Sf[-1]), ("logZ", 2, run_sum(lik))):
        assert np.array_equal(st[name], on[name]) and np.array_equal(out[:, col], on[name]) and np.array_equal(on[name], ref), name
    assert np.array_equal(st["logw"], st["logZ"])
    h.close()


def test_rejuvenate_with_gaps_equals_restatement():
    """resample_ and rejuvenate_ after 8 online steps of a series with gaps (the re-filter of y[0:8) per proposal skips the same
    updates): theta, x, Sigma, logZ, logw and the moved mask == the restatement; then one more step from the moved cloud"""
    y = with_gaps(_y(), (0, 3, 4))
    tmap, prior, _ = case_readme(smc)
    r = IbisMissingReference(77, tmap, prior, 3, 0.5, seed=9)
    ib = _ibis(77, seed=9)
    r.smc2(y)
    smc.smc2(ib, y)
    for t in range(2, 9):
        r._propagate(float(y[t - 1]), True)
        smc.ibis._window(ib, y[t - 1:t], 0.0)
    assert np.array_equal(smc.resample_(ib), r.resample())
    r.rejuvenate(y[:8])
    smc.rejuvenate_(ib, y[:8])
    assert r.n_accepted >= 1 and r.n_out_of_support >= 1
    r._propagate(float(y[8]), True)
    smc.ibis._window(ib, y[8:9], 0.0)
    for name, ref in (("theta", r.theta), ("x", r.x), ("Sigma", r.S), ("logZ", r.logZ), ("logw", r.logw)):
        assert np.array_equal(getattr(ib, name), ref), name
    assert np.array_equal(ib.accepted, r.accepted) and ib.acc_ratio == r.acc_ratio
    # the re-filter and the online filter of the same observations: the same number, with gaps as without
    z = L.kalman_log_likelihood(tmap.rows(ib.theta), y[:9], False, missing=True)
    assert np.array_equal(z[:, 2], ib.logZ) and np.array_equal(z[:, 0], ib.x)
    ib.close()


# ---- the sampler against the restatement: T = 40, gaps at the first and last period, a pair and a single one ------------------
T_RUN, GAPS_RUN = 40, (0, 7, 8, 20, 39)
_REF = {}


def _y_run():
    return with_gaps(_y(T_RUN), GAPS_RUN)


def reference_run(M):
    """the restatement's online run, once per M, with the branches a comparison must exercise asserted on it first"""
    if M not in _REF:
        tmap, prior, _ = case_readme(smc)
        r = IbisMissingReference(M, tmap, prior, 3, 0.5, seed=5).run(_y_run())
        assert r.n_rejuvenations >= 2 and r.n_out_of_support >= 1 and r.n_accepted >= 1, (r.n_rejuvenations, r.n_out_of_support, r.n_accepted)
        _REF[M] = r
    return _REF[M]


def _same_sampler(ib, r):
    for name, ref in (("theta", r.theta), ("x", r.x), ("Sigma", r.S), ("logZ", r.logZ), ("logw", r.logw)):
        got = getattr(ib, name)
        assert got.shape == ref.shape and np.array_equal(got, ref), name
    assert ib.ess == r.ess and ib.acc_ratio == r.acc_ratio and np.array_equal(ib.accepted, r.accepted)
    assert ib.n_rejuvenations == r.n_rejuvenations


class _Trace:
    """the ESS of every step a sampler kept, with the number of rejuvenations before it"""

    def __init__(self, monkeypatch):
        self.ess, self.nrej = [], []
        inner = smc.ibis._window

        def window(ibis, y, ess_min, t=None):
            ess, j = inner(ibis, y, ess_min, t)
            self.ess.extend(float(e) for e in ess[:j])
            self.nrej.extend([ibis.n_rejuvenations] * j)
            return ess, j
        monkeypatch.setattr(smc.ibis, "_window", window)


@pytest.mark.parametrize("window", [1, 7, 16])
@pytest.mark.parametrize("M", [77, 512])
def test_online_run_equals_restatement(M, window, monkeypatch):
    """smc2 + smc2_run over the series with gaps: the ESS of every step and every array at the end == the restatement"""
    y, r = _y_run(), reference_run(M)
    tr = _Trace(monkeypatch)
    ib = _ibis(M)
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, T_RUN, window=window, verbose=False)
    assert ib.t == T_RUN and tr.ess == r.ess_trace
    for t in GAPS_RUN[1:]:
        assert tr.ess[t] == tr.ess[t - 1] or tr.nrej[t] != tr.nrej[t - 1]
    _same_sampler(ib, r)
    ib.close()


@pytest.mark.parametrize("M", [77, 512])
def test_online_run_with_device_moves(M, monkeypatch):
    """device_moves=True: the walk and the index draw are the host route's functions, so up to the first rejuvenation the ESS of
    every step == the restatement's (afterwards the covariance is summed in the device's order: the existing device-moves
    tests assert no more); and the whole run == the same calls made one by one on a flagged handle"""
    y, r = _y_run(), reference_run(M)
    tr = _Trace(monkeypatch)
    ib = _ibis(M, device_moves=True)
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, T_RUN, window=16, verbose=False)
    first = tr.nrej.index(1)
    assert first > GAPS_RUN[0] and tr.ess[:first] == r.ess_trace[:first] and ib.n_rejuvenations >= 2
    assert np.all(np.isfinite(ib.logZ)) and np.all(np.isfinite(ib.x)) and np.all(np.isfinite(smc.expected_parameters(ib)))
    # the same run call by call on a flagged handle, every device result checked against its host function on the way
    # (test_gpu_ibis_device_moves._hand_driven): every array and the whole ESS trace ==
    monkeypatch.setattr(DM, "_handle", _handle)
    st, trace, nrej, accepted, acc_ratio = DM._hand_driven(_ibis(M), y)
    assert ib.t == T_RUN and ib.n_rejuvenations == nrej and tr.ess == trace and ib.ess == trace[-1]
    for name, attr in zip(NAMES, ("theta", "x", "Sigma", "logZ", "logw")):
        assert np.array_equal(getattr(ib, attr), st[name]), name
    assert np.array_equal(ib.accepted, accepted) and ib.acc_ratio == acc_ratio
    ib.close()


def test_density_tempered_equals_restatement():
    y = _y_run()
    tmap, prior, _ = case_readme(smc)
    r = IbisMissingReference(512, tmap, prior, 3, 0.5, seed=4)
    ladder = r.density_tempered(y)
    assert r.n_rejuvenations >= 2 and r.n_out_of_support >= 1 and r.n_accepted >= 1
    ib = _ibis(512, seed=4)
    stages = smc.density_tempered(ib, y, verbose=False)
    assert stages == ladder
    _same_sampler(ib, r)
    assert np.array_equal(smc.expected_parameters(ib), r.expected_parameters())
    ib.close()
    dm = _ibis(512, seed=4, device_moves=True)
    st = smc.density_tempered(dm, y, verbose=False)
    assert st[0][:2] == ladder[0][:2] and st[-1][0] == 1.0 and np.all(np.isfinite(dm.logZ))      # the first stage: the same bisection
    dm.close()


# ---- the RTS smoother and the paths -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("predict_first", [False, True])
@pytest.mark.parametrize("gaps", GAP_SETS, ids=str)
@pytest.mark.parametrize("M", [1, 9, 65, 513])
def test_smoother_and_paths_equal_host_twins(M, gaps, predict_first):
    """smc_ibis_smooth (out, xs, Ps), the flagged smc_kalman_smooth and smc_ibis_sample_paths == their flagged host twins"""
    y = with_gaps(_y(), gaps)
    ib = _ibis(M, predict_first)
    rows = ib.theta_map.rows(ib._theta0)
    h = _handle(ib)
    lw = np.linspace(-2.0, 0.0, M)
    h.set_logw(lw)
    out, xs, Ps = h.smooth(y, states=True)
    rout, rxs, rPs = L.host_ibis_smooth(rows, lw, y, predict_first, states=True, missing=True)
    assert np.all(np.isfinite(rxs)) and np.all(rPs > 0)
    assert _same(out, rout) and np.array_equal(xs, rxs) and np.array_equal(Ps, rPs)
    kx, kP = L.kalman_smooth(rows, y, predict_first, missing=True)
    assert np.array_equal(kx, rxs) and np.array_equal(kP, rPs)
    which = (np.arange(70) * 7 % M).astype(np.int32)
    assert np.array_equal(h.sample_paths(y, which, 31), L.host_ibis_sample_paths(rows, y, which, 31, predict_first, missing=True))
    h.close()


@pytest.mark.parametrize("gaps", GAP_SETS[1:], ids=str)
def test_path_mean_at_the_gaps(gaps):
    """Mp = 4096 paths under ONE row: at every gap their mean is within 4 standard errors of the exact smoothed mean xs_t, the
    standard error sqrt(Ps_t / Mp) from the exact smoothed variance"""
    Mp = 4096
    y = with_gaps(_y(), gaps)
    ib = _ibis(9)
    rows = ib.theta_map.rows(ib._theta0)
    h = _handle(ib)
    _, xs, Ps = h.smooth(y, states=True)
    paths = h.sample_paths(y, np.full(Mp, 4, dtype=np.int32), 77)
    for t in gaps:
        err, se = abs(paths[t].mean() - xs[t, 4]), np.sqrt(Ps[t, 4] / Mp)
        print("gap %d: |mean - xs| = %.3g, se = %.3g" % (t, err, se))
        assert err <= 4.0 * se, t
    h.close()


@pytest.mark.parametrize("M", [9, 130, 513])
def test_flagged_handle_without_nan_equals_unflagged(M):
    """a flagged handle on a NaN-free series (it launches the kernels of an unflagged one): every array == the unflagged handle's"""
    y = _y()
    ib = _ibis(M)
    f, u = _handle(ib, FLAG), _handle(ib, 0)
    assert f.flags == FLAG and u.flags == 0
    Lf, _ = L.host_rw_factor(ib._theta0) if M > 1 else (np.eye(3), False)
    s = 0.5 * np.arange(3, 0, -1)
    which = (np.arange(40) % M).astype(np.int32)
    res = []
    for h in (f, u):
        h.set_summaries(True, 1)
        rec, lik = h.window(y[:7], want_lik=True)
        got = [rec, lik, h.get_summaries(7)]
        h.commit(4)
        got.extend(h.window_ess(y[4:], 0.0))
        h.commit(T - 4)
        got.extend(_state(h)[n] for n in NAMES)
        got.extend(h.rejuvenate(y, 1.0, Lf, s, 99))
        got.extend(_state(h)[n] for n in NAMES)
        got.extend(h.smooth(y, states=True))
        got.append(h.sample_paths(y, which, 5))
        h.filter(y)
        got.extend(_state(h)[n] for n in NAMES)
        res.append(got)
        h.close()
    assert len(res[0]) == len(res[1])
    for i, (a, b) in enumerate(zip(*res)):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), i


def test_flags_errors_and_a_nan_without_the_flag():
    y = with_gaps(_y(), (4,))
    ib = _ibis(65)
    h = _handle(ib, 0)
    lib = L.lib()
    assert lib.smc_ibis_set_flags(h._h, 32) == -1 and lib.smc_ibis_set_flags(h._h, FLAG | 1) == -1          # SMC_EINVAL
    assert h.flags == 0
    h.set_flags(FLAG)
    h.set_flags(0)
    h.window(y[:2])
    assert lib.smc_ibis_set_flags(h._h, FLAG) == -3                                                          # SMC_ESTATE: a window is pending
    h.commit(2)
    assert lib.smc_ibis_set_flags(h._h, FLAG) == -3 and h.flags == 0                                         # SMC_ESTATE: t = 2
    h.set_theta(ib._theta0)                                                                                  # t = 0 again
    h.window(y)
    h.commit(T)
    st = _state(h)
    assert np.all(np.isnan(st["x"])) and np.all(np.isnan(st["logZ"])) and np.all(np.isnan(st["logw"]))      # as it always was
    rows = ib.theta_map.rows(ib._theta0)
    assert np.all(np.isnan(L.kalman_log_likelihood(rows, y, False)[:, 2]))
    h.close()


def test_foreign_flag_bits_are_refused_by_the_device_calls():
    rows = np.ascontiguousarray([[0.5, 1.0, 0.9, 0.8, 0.0, 1.0]])
    y, out, xs, Ps = _y(), np.zeros((1, 3)), np.zeros((T, 1)), np.zeros((T, 1))
    lib = L.lib()
    assert lib.smc_kalman_log_likelihood_flags(L._d(rows), 1, L._d(y), T, 0, L._d(out), 0, 32) == -1
    assert lib.smc_kalman_smooth_flags(L._d(rows), 1, L._d(y), T, 0, L._d(xs), L._d(Ps), 0, 32) == -1


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def test_python_surface():
    """IBIS(..., missing=True) runs the README loop on a series with gaps; every summary reads the flag from the sampler;
    without the keyword the same series gives NaN as it always did"""
    y = _y_run()
    ib = _ibis(512)
    assert ib.missing is True
    mean0, var0 = smc.rts_smoothed_state(ib, y)                       # before the first sampler call: the host twins, flagged
    assert np.all(np.isfinite(mean0)) and np.all(var0 > 0)
    assert np.all(np.isfinite(smc.rts_smoothed_paths(ib, y, 8, seed=3)))
    ib.set_summaries([0.05, 0.95])
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, len(y), verbose=False)
    assert ib._h.flags == FLAG and ib.n_rejuvenations >= 2
    assert np.all(np.isfinite(smc.expected_parameters(ib)))
    assert len(ib.summary_trace) == T_RUN and all(np.isfinite(e[1]) and np.all(np.isfinite(e[6])) for e in ib.summary_trace)
    mean, var = smc.rts_smoothed_state(ib, y)
    assert np.all(np.isfinite(mean[list(GAPS_RUN)])) and np.all(var[list(GAPS_RUN)] > 0)
    assert np.all(np.isfinite(smc.rts_quantile(ib, y, [0.05, 0.5, 0.95])))
    assert np.all(np.isfinite(smc.rts_smoothed_paths(ib, y, 16, seed=3)))
    assert all(np.isfinite(v) for v in smc.observation_dist(ib) + smc.filtered_state(ib)) and np.all(np.isfinite(smc.quantile(ib, [0.1, 0.9], ahead=1)))
    _, prior, model = case_readme(smc)
    mods = [model(t) for t in ib.theta[:5]]
    x, S, z = smc.log_likelihood_kalman(y, mods, missing=True)
    assert np.array_equal(z, ib.logZ[:5]) and np.array_equal(x, ib.x[:5]) and np.array_equal(S, ib.Sigma[:5])
    xs, Ps = smc.kalman_smoother(y, mods[0], missing=True)
    assert xs.shape == (T_RUN,) and np.all(np.isfinite(xs)) and np.all(Ps > 0)
    assert np.isnan(smc.log_likelihood_kalman(y, mods[0])[2]) and np.all(np.isnan(smc.kalman_smoother(y, mods[0])[0]))
    ib.close()
    plain = _ibis(64, missing=False)
    smc.smc2(plain, y)
    assert plain._h.flags == 0 and np.all(np.isnan(plain.logZ)) and np.all(np.isnan(plain.x))      # the gap at t = 0 without the keyword
    plain.close()
