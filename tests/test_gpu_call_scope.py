"""GPU tests of the scope every entry point without a handle opens (DeviceCall, csrc/smc_host.h): one device check, the calling
thread's non-blocking stream, and ONE allocation per call - the thread's cached scratch (the ten calls of smc_util.hip) or a block
of the call's own (smc_kalman_smooth, smc_kalman2_*).  Every float64 array is compared bit for bit with the host twin or the
oracle (NaN == NaN), never approx."""
import numpy as np
import pytest

from sequential_monte_carlo_amd import _lib as L
import kalman2_reference as k2
import step_edge_inputs

pytestmark = pytest.mark.gpu

KALMAN_THREADS = 64          # csrc/smc_kalman_rows.h: rows per workgroup of the exact-Kalman kernels
LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
EINVAL = -1


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float64:
        return a.shape == b.shape and np.array_equal(a, b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def same_all(got, want):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    return len(got) == len(want) and all(same(np.atleast_1d(g), np.atleast_1d(w)) for g, w in zip(got, want))


def run_sum(lik):
    z = 0.0
    for v in lik:
        z = z + float(v)
    return z


def lg_rows(n, seed):
    rng = np.random.default_rng(seed)
    rows = np.tile(LG, (n, 1))
    rows[:, 0] = rng.uniform(-0.95, 0.95, n)
    rows[:, 2:4] = rng.lognormal(size=(n, 2))
    return rows


def series(T, gap=False):
    y = np.random.default_rng(5).normal(size=T)
    if gap:
        y[min(2, T - 1)] = np.nan
    return y


# ---- a. the ten calls on the thread's scratch ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scratch_calls(ob):
    """[(name, the device call, what it must return)] in the order of the issue: sizes on both sides of normalize's and
    resample's one-workgroup limits, a growing and a shrinking plan after each other.  The references are computed once."""
    rng = np.random.default_rng(23)
    calls = []

    def logw_of(n):
        lw = rng.normal(size=n) * 5 - 100
        if n > 10:
            lw[3], lw[7] = -np.inf, np.nan
        return lw

    def normalize(n):
        lw = logw_of(n)
        calls.append(("normalize %d" % n, lambda: L.normalize(lw), ob.normalize(lw)))

    def resample(n, ndraw):
        w = ob.normalize(logw_of(n))[1]
        calls.append(("resample %d / %d" % (n, ndraw), lambda: L.resample(w, ndraw, seed=4, stream=2, t=9),
                      ob.resample(w, ndraw, seed=4, stream=2, t=9).astype(np.int32)))

    normalize(63)
    resample(65537, 1)
    rows, y = lg_rows(KALMAN_THREADS + 1, 2), series(5, gap=True)
    want = np.array([(xf[-1], Sf[-1], run_sum(lik)) for xf, Sf, lik in (L.host_kalman_steps(r, y, False, missing=True) for r in rows)])
    calls.append(("kalman_log_likelihood", lambda: L.kalman_log_likelihood(rows, y, False, missing=True), want))
    v = rng.uniform(-700, 5, 257)
    calls.append(("device_math 257", lambda: L.device_math(0, v), ob.exp(v)))
    normalize(16385)
    resample(63, 190)
    raw, sp, z, yy = step_edge_inputs.rb(False)
    sp, z = sp[:, :257].copy(), z[:, :257].copy()
    calls.append(("device_filter_steps RB 257", lambda: L.device_filter_steps(L.MODEL_UCSV_RB, raw, L.PROP_NONE, None, sp, z, yy),
                  L.host_filter_steps(L.MODEL_UCSV_RB, raw, L.PROP_NONE, None, sp, z, yy)))
    calls.append(("device_normcdf 1", lambda: L.device_normcdf(np.array([-1.25])), L.host_normcdf(np.array([-1.25]))))
    rows2, y1 = lg_rows(2, 3), series(1)
    host = [L.host_kalman_predictive(r, y1, False) for r in rows2]
    calls.append(("kalman_predictive 2 x 1", lambda: L.kalman_predictive(rows2, y1, False),
                  tuple(np.stack([h[k] for h in host], axis=1) for k in range(3))))
    D, n, u, j0 = (1 << 62) + 12345, 1 << 20, 987654321987654321, 4096
    calls.append(("sys_targets 1", lambda: L.sys_targets(D, n, u, j0, 1, device=0), np.array([(j0 * D + ((u * D) >> 64)) // n], dtype=np.uint64)))
    return calls


def test_one_scratch_is_reused_and_grown(scratch_calls):
    """the list forwards, then backwards, on one thread: every result is the reference's each time (a stale offset, or an array
    planned after the allocation, would show here), and nothing of it is counted by smc_live_bytes"""
    live = L.live_bytes()
    for rnd, order in enumerate((scratch_calls, scratch_calls[::-1])):
        for name, call, want in order:
            assert same_all(call(), want), (rnd, name)
    assert L.live_bytes() == live


# ---- b. the three calls that own their block --------------------------------------------------------------------------------
SIZES = [(n, T) for n in (1, KALMAN_THREADS + 1) for T in (1, 5)]
_OWN = {}


def own_case(n, T):
    """the inputs and the host twins of one size, computed once: name -> (the device call, what it must return)"""
    if (n, T) not in _OWN:
        rows, rows2, zero = lg_rows(n, 7), k2.random_pd_rows(n, seed=13), np.zeros(n)
        case = {}
        for missing in (False, True):
            y = series(T, gap=missing)
            _, xs, Ps = L.host_ibis_smooth(rows, zero, y, False, states=True, missing=missing)
            for m, r in enumerate(rows):          # the smoothed state of the last period is the filtered one
                xf, Sf, _ = L.host_kalman_steps(r, y, False, missing=missing)
                assert same([xs[-1, m], Ps[-1, m]], [xf[-1], Sf[-1]])
            case["kalman_smooth" + (" flagged" if missing else "")] = (
                lambda y=y, missing=missing: L.kalman_smooth(rows, y, False, missing=missing), (xs, Ps))
        y = series(T)
        out, x2, P2 = np.zeros((n, 6)), np.zeros((T, n, 2)), np.zeros((T, n, 3))
        for i, r in enumerate(rows2):
            xf, Sf, lik = L.host_kalman2_steps(r, y, True)
            out[i] = (*xf[-1], *Sf[-1], run_sum(lik))
            x2[:, i], P2[:, i] = L.host_kalman2_smooth(r, y, True)
        case["kalman2_log_likelihood"] = (lambda: L.kalman2_log_likelihood(rows2, y, True), out)
        case["kalman2_smooth"] = (lambda: L.kalman2_smooth(rows2, y, True), (x2, P2))
        _OWN[(n, T)] = case
    return _OWN[(n, T)]


@pytest.mark.parametrize("n,T", SIZES)
def test_own_block_calls_equal_host_twins_and_free_their_block(n, T):
    for name, (call, want) in own_case(n, T).items():
        live = L.live_bytes()
        assert same_all(call(), want), name
        assert L.live_bytes() == live, name


# ---- c. not the null stream ----------------------------------------------------------------------------------------------------
def test_no_call_needs_the_null_stream():
    """with work queued on PyTorch's default (null) stream, the three calls that used to run there return the bits of (b): they
    own their memory and wait for their own stream.  No timing is asserted."""
    import torch
    n, T = KALMAN_THREADS + 1, 5
    case = own_case(n, T)
    with torch.cuda.stream(torch.cuda.default_stream()):
        a = torch.zeros(1 << 26, device="cuda")
        for _ in range(200):          # (elementwise: tens of milliseconds of queued work, no BLAS library to load)
            a += 1.0
        for name, (call, want) in case.items():
            assert same_all(call(), want), name
    torch.cuda.synchronize()
    assert float(a[0]) == 200.0 and float(a[-1]) == 200.0


# ---- d. a device index that does not exist -------------------------------------------------------------------------------------
def bad_device_calls(dev):
    """the thirteen calls with valid arguments and the device index dev"""
    rows, rows2, y = lg_rows(3, 1), k2.random_pd_rows(3, seed=13), series(5)
    raw, par, xp, z, yy = step_edge_inputs.guided(1, step_edge_inputs.AFFINE)
    rraw, sp, rz, _ = step_edge_inputs.rb(False)
    w = np.full(8, 0.125)
    return {
        "smc_normalize": lambda: L.normalize(np.zeros(8), device=dev),
        "smc_resample": lambda: L.resample(w, device=dev),
        "smc_kalman_log_likelihood": lambda: L.kalman_log_likelihood(rows, y, device=dev),
        "smc_kalman_predictive": lambda: L.kalman_predictive(rows, y, device=dev),
        "smc_device_normcdf": lambda: L.device_normcdf(np.zeros(4), device=dev),
        "smc_sys_targets": lambda: L.sys_targets(5, 3, 11, 0, 3, device=dev),
        "smc_device_guided_step": lambda: L.device_guided_step(1, raw, step_edge_inputs.AFFINE, par, xp[:, :8], z[:, :8], yy, device=dev),
        "smc_device_rb_step": lambda: L.device_rb_step(rraw, sp[:, :8], rz[:, :8], yy, device=dev),
        "smc_device_filter_steps": lambda: L.device_filter_steps(1, raw, L.PROP_NONE, None, xp[:, :8], z[:, :8], yy, device=dev),
        "smc_device_math": lambda: L.device_math(0, np.zeros(4), device=dev),
        "smc_kalman_smooth": lambda: L.kalman_smooth(rows, y, device=dev),
        "smc_kalman2_log_likelihood": lambda: L.kalman2_log_likelihood(rows2, y, device=dev),
        "smc_kalman2_smooth": lambda: L.kalman2_smooth(rows2, y, device=dev),
    }


def test_a_bad_device_is_refused_by_every_call(ob):
    """device = the device count, and -1 (smc_sys_targets reads a negative index as "on the host"): SMC_EINVAL "<who>: bad
    device" from the argument check, before any runtime call sees the index; the next call of the thread is served"""
    v = np.linspace(-3.0, 3.0, 63)
    want = ob.exp(v)
    for dev in (L.device_count(), -1):
        calls = bad_device_calls(dev)
        assert len(calls) == 13
        for who, call in calls.items():
            if dev < 0 and who == "smc_sys_targets":
                continue
            with pytest.raises(L.SmcError, match=r"error %d: %s: bad device" % (EINVAL, who)):
                call()
            assert same(L.device_math(0, v), want), who
