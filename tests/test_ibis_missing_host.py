"""CPU tests of missing observations on the exact-Kalman side (SMC_FLAG_NAN_MISSING for IBIS / Kalman / RTS): the
host twins smc_host_kalman_steps, smc_host_ibis_smooth_flags and smc_host_ibis_sample_paths_flags - the specification the
device equals bit for bit (tests/test_gpu_ibis_missing.py) - against the restatement from the unchanged oracle
(tests/ibis_missing_reference.py) with ==, and against the independent numpy filter / smoother of tests/missing_reference.py."""
import numpy as np
import pytest

import ibis_missing_reference as IM
import missing_reference as MR

# (A, B, Q, R, x0, sigma0): the rows of tests/test_rts_host.py
ROWS = np.array([
    [1.0, 1.0, 0.3, 0.5, 0.0, 1.0],
    [0.9, 1.0, 0.2, 1.0, 0.5, 2.0],
    [-0.7, 1.0, 0.5, 0.4, 0.0, 1.0],
    [0.95, 2.5, 0.1, 0.3, 1.0, 0.5],
    [1.0, 1.0, 1e-3, 10.0, 0.0, 1.0],
    [1.0, 1.0, 10.0, 1e-3, 0.0, 1.0],
    [0.8, 0.4, 1e-2, 1e2, -1.0, 3.0],
    [-0.5, 1.5, 1e2, 1e-2, 2.0, 0.1],
])
T = 40
GAP_SETS = [(), (0,), (T - 1,), (0, 1), (3, 4, 5), MR.GAPS40, tuple(range(T))]
FLAG, BAD_FLAG = 8, 32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def series(L, n=T, seed=1998):
    return L.simulate(L.MODEL_LG1D, [0.9, 1.0, 0.5, 0.8, 0.0, 1.0], n, seed)[1]


def log_z(lik):
    z = 0.0
    for l in lik:
        z = z + float(l)
    return z


@pytest.mark.parametrize("predict_first", [False, True])
def test_flag_on_a_series_without_nan_changes_no_bit(L, predict_first):
    y = series(L)
    logw = np.linspace(-3.0, 0.0, len(ROWS))
    for r in ROWS:
        for a, b in zip(L.host_kalman_steps(r, y, predict_first, missing=True), L.host_kalman_steps(r, y, predict_first)):
            assert same_bits(a, b)
    f = L.host_ibis_smooth(ROWS, logw, y, predict_first, states=True, filtered=True, missing=True)
    u = L.host_ibis_smooth(ROWS, logw, y, predict_first, states=True, filtered=True)
    assert len(f) == len(u) == 5 and all(same_bits(a, b) for a, b in zip(f, u))       # out, xs, Ps, xf, Sf
    which = np.arange(33, dtype=np.int32) % len(ROWS)
    assert same_bits(L.host_ibis_sample_paths(ROWS, y, which, 7, predict_first, missing=True), L.host_ibis_sample_paths(ROWS, y, which, 7, predict_first))


@pytest.mark.parametrize("predict_first", [False, True])
@pytest.mark.parametrize("gaps", GAP_SETS[1:], ids=str)
def test_record_with_gaps_equals_restatement(L, gaps, predict_first):
    """lik is +0.0 (the bits) at every gap; xf, Sf, lik == the restatement from the oracle; the forward record of the smoother
    and of the paths twin is the same record"""
    y = IM.with_gaps(series(L), gaps)
    for r in ROWS:
        xf, Sf, lik = L.host_kalman_steps(r, y, predict_first, missing=True)
        assert not bits(lik[list(gaps)]).any()
        _, _, _, rxf, rSf, rlik = IM.gap_series(r, y, predict_first, record=True)
        assert np.array_equal(xf, rxf) and np.array_equal(Sf, rSf) and same_bits(lik, rlik)
        _, xs, Ps, sxf, sSf = L.host_ibis_smooth(r[None], np.zeros(1), y, predict_first, states=True, filtered=True, missing=True)
        assert same_bits(sxf[:, 0], xf) and same_bits(sSf[:, 0], Sf)
        assert np.all(np.isfinite(xs)) and np.all(Ps > 0)
        assert xs[T - 1, 0] == xf[T - 1] and Ps[T - 1, 0] == Sf[T - 1]


def test_leading_gap_is_the_series_without_it(L):
    """predict_first = 0 and a gap at t = 0: the state stays (x0, sigma0), so everything after equals the unflagged run on y[1:]
    with predict_first = 1"""
    y = IM.with_gaps(series(L), (0,))
    for r in ROWS:
        xf, Sf, lik = L.host_kalman_steps(r, y, False, missing=True)
        assert xf[0] == r[4] and Sf[0] == r[5] and not bits(lik[:1]).any()
        uxf, uSf, ulik = L.host_kalman_steps(r, y[1:], True)
        assert same_bits(xf[1:], uxf) and same_bits(Sf[1:], uSf) and same_bits(lik[1:], ulik)
        assert bits(log_z(lik)) == bits(log_z(ulik))


@pytest.mark.parametrize("predict_first", [False, True])
@pytest.mark.parametrize("gaps", GAP_SETS[1:-1], ids=str)
def test_static_level_drops_its_gaps(L, gaps, predict_first):
    """A = 1, Q = 0: the prediction is the identity, so gaps anywhere leave the final (x, S, logZ) of the series without them"""
    y = IM.with_gaps(series(L), gaps)
    for r in ([1.0, 1.0, 0.0, 0.5, 0.3, 1.0], [1.0, 2.5, 0.0, 3.0, -1.0, 0.2]):
        xf, Sf, lik = L.host_kalman_steps(r, y, predict_first, missing=True)
        uxf, uSf, ulik = L.host_kalman_steps(r, y[~np.isnan(y)], predict_first)
        assert bits(xf[-1]) == bits(uxf[-1]) and bits(Sf[-1]) == bits(uSf[-1]) and bits(log_z(lik)) == bits(log_z(ulik))


@pytest.mark.parametrize("k", [1, 3])
def test_trailing_gaps_leave_logZ(L, k):
    y = series(L)
    yk = np.concatenate([y, np.full(k, np.nan)])
    for r in ROWS:
        xf, Sf, lik = L.host_kalman_steps(r, yk, False, missing=True)
        _, _, ulik = L.host_kalman_steps(r, y, False)
        assert same_bits(lik[:T], ulik) and bits(log_z(lik)) == bits(log_z(ulik))
        assert Sf[-1] > Sf[T - 1] or r[2] == 0.0


@pytest.mark.parametrize("predict_first", [False, True])
def test_all_nan_series_is_the_pure_prediction(L, predict_first):
    y = np.full(9, np.nan)
    for r in ROWS:
        xf, Sf, lik = L.host_kalman_steps(r, y, predict_first, missing=True)
        assert not bits(lik).any() and bits(log_z(lik)) == 0
        x, S = r[4], r[5]
        for t in range(9):
            if predict_first or t > 0:
                x, S = r[0] * x, (r[0] * r[0]) * S + r[2]
            assert xf[t] == x and Sf[t] == S


# The unflagged host twins against kalman_gaps / rts_gaps on ROWS and the NaN-free series of this file (T = 40), measured on the
# CPU with the unflagged calls, whose body is the parent's: means (xf, xs) as |got - ref| / (max |ref| + sqrt(max P)) per row,
# variances and logZ as |got - ref| / |ref|: xf 2.98e-16, Sf 3.198e-12, logZ 0, xs 3.72e-16, Ps 3.198e-12.  The largest is
# 3.198e-12 (the reference's P - K B P cancels at Q / R = 1e4); times 4 for the extra prediction per gap.
MEASURED_UNFLAGGED = 3.198e-12
TOL = 4 * MEASURED_UNFLAGGED


def _deviation(L, y, missing):
    worst = {}

    def keep(name, v):
        worst[name] = max(worst.get(name, 0.0), float(v))
    for r in ROWS:
        xf, Sf, lik = L.host_kalman_steps(r, y, False, missing=missing)
        _, xs, Ps = L.host_ibis_smooth(r[None], np.zeros(1), y, False, states=True, missing=missing)
        ll, _, _, mf, Pf = MR.kalman_gaps(r, y)
        ms, Pss = MR.rts_gaps(r, y)
        keep("xf", np.abs(xf - mf).max() / (np.abs(mf).max() + np.sqrt(Pf.max())))
        keep("Sf", (np.abs(Sf - Pf) / Pf).max())
        keep("logZ", abs(log_z(lik) - ll) / abs(ll))
        keep("xs", np.abs(xs[:, 0] - ms).max() / (np.abs(ms).max() + np.sqrt(Pss.max())))
        keep("Ps", (np.abs(Ps[:, 0] - Pss) / Pss).max())
    return worst


@pytest.mark.parametrize("gaps", [(), (0,), (T - 1,), (0, 1), (3, 4, 5), MR.GAPS40], ids=str)
def test_against_the_independent_filter_and_smoother(L, gaps):
    """xf, Sf, logZ against missing_reference.kalman_gaps and xs, Ps against rts_gaps - numpy recursions with skipped updates in
    another association, so no equality: within TOL = 4 x 3.198e-12, the unflagged twins' own largest deviation from them on
    the NaN-free series (the derivation above).  Measured with gaps: at most 7.11e-12 (Sf, Ps), 1.7e-16 (xf), 3.2e-16 (xs),
    1.5e-16 (logZ)."""
    w = _deviation(L, IM.with_gaps(series(L), gaps), missing=len(gaps) > 0)
    print(gaps, " ".join("%s %.3g" % kv for kv in sorted(w.items())))
    if not gaps:
        assert max(w.values()) <= MEASURED_UNFLAGGED
    assert max(w.values()) <= TOL


def test_paths_twin_through_gaps(L):
    """the paths twin with gaps: path p is rts_path_* over the flagged record, with the normals it reports - finite through
    the gaps, and the unflagged call on the same series is poisoned as it always was"""
    y = IM.with_gaps(series(L, 12), (3, 4, 5))
    which = np.arange(16, dtype=np.int32) % len(ROWS)
    p = L.host_ibis_sample_paths(ROWS, y, which, 11, False, missing=True)
    assert p.shape == (12, 16) and np.all(np.isfinite(p))
    assert np.all(np.isnan(L.host_ibis_sample_paths(ROWS, y, which, 11, False)[3:]))


def test_errors_and_a_nan_without_the_flag(L):
    y = IM.with_gaps(series(L, 12), (4,))
    xf, Sf, lik = L.host_kalman_steps(ROWS[0], y, False)
    assert np.all(np.isfinite(xf[:4])) and np.all(np.isnan(xf[4:])) and np.all(np.isnan(lik[4:]))      # (Sigma never reads y)
    assert same_bits(Sf, L.host_kalman_steps(ROWS[0], series(L, 12), False)[1])
    _, xs, Ps = L.host_ibis_smooth(ROWS, np.zeros(len(ROWS)), y, False, states=True)
    assert np.all(np.isnan(xs)) and np.all(np.isfinite(Ps))
    lib = L.lib()
    out = np.zeros(12)
    assert lib.smc_host_kalman_steps(L._d(ROWS[0].copy()), L._d(y), 12, 0, BAD_FLAG, L._d(out), None, None) == -1
    assert lib.smc_host_kalman_steps(L._d(ROWS[0].copy()), L._d(y), 12, 0, FLAG | 1, L._d(out), None, None) == -1
    o8, w = np.zeros((12, 8)), np.zeros(len(ROWS))
    rows = np.ascontiguousarray(ROWS)
    assert lib.smc_host_ibis_smooth_flags(L._d(rows), L._d(w), len(ROWS), L._d(y), 12, 0, L._d(o8), None, None, None, None, BAD_FLAG) == -1
    which, paths = np.zeros(2, dtype=np.int32), np.zeros((12, 2))
    assert lib.smc_host_ibis_sample_paths_flags(L._d(rows), len(ROWS), L._d(y), 12, 0, 2, 1, which.ctypes.data_as(L._i32p), L._d(paths), None,
                                                BAD_FLAG) == -1
    assert L.FLAG_NAN_MISSING == FLAG
