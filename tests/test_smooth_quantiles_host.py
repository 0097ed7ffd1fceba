"""CPU tests of smc_host_smooth_quantiles (csrc/smc_spec.h "quantiles of the smoothed state") against the restatement
in Python integers of tests/smooth_quantiles_reference.py, compared bit for bit; the accuracy of the integer weights against the
dense ones by a derived bound; and what the Python layer refuses before any device call."""
import math

import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
import smooth_quantiles_reference as ref

SIZES = [1, 2, 63, 64, 65, 1000]
P = ref.LEVELS8
TINY = 2.0 ** -1074
NEG_NAN = float(np.array([0xfff8000000000000], dtype=np.uint64).view(np.float64)[0])


def check(x, ws, p=P):
    """the twin on x, ws [T][n] == the restatement, bit for bit -> the twin's output"""
    x, ws = np.atleast_2d(np.asarray(x, dtype=np.float64)), np.atleast_2d(np.asarray(ws, dtype=np.float64))
    out = L.host_smooth_quantiles(x, ws, p)
    want = ref.quantiles(x, ws, p)
    assert ref.same(out, want), (out, want)
    return out


def test_constants():
    bits, lds_max = L.smooth_quantiles_constants()
    assert bits == ref.Q_BITS and bits >= 31
    assert 65535 * 128 * 2 ** bits < 2 ** 63                  # W fits 63 bits at the largest cloud the smoother admits
    assert lds_max >= 1024


@pytest.mark.parametrize("n", SIZES)
def test_random_clouds(n):
    """three steps of a random cloud: unnormalised weights of very different scales per step; ties on half the values"""
    rng = np.random.default_rng(100 + n)
    x = rng.normal(size=(3, n)) * np.array([[1.0], [1e-6], [1e8]])
    ws = rng.exponential(size=(3, n)) * np.array([[1.0], [1e-200], [3e150]])
    out = check(x, ws)
    for t in range(3):                                       # p = 0: the smallest value, p = 1: the largest (every weight is positive)
        assert out[t, 0] == x[t].min() and out[t, 1] == x[t].max()
        assert np.all(np.diff(out[t][[0, 3, 7, 5, 2, 6, 4, 1]]) >= 0)      # monotone in p
    tied = x.copy()
    tied[:, : n // 2] = tied[:, :1]                          # heavy ties: half the values are equal
    check(tied, ws)
    check(np.repeat(x[:, :1], n, axis=1), ws)                # one distinct value
    for j in range(len(P)):                                  # one level at a time gives the same column
        assert ref.same(L.host_smooth_quantiles(x, ws, P[j:j + 1]), out[:, j:j + 1])


def test_order_of_special_values():
    rng = np.random.default_rng(7)
    vals = np.array([-0.0, 0.0, -1.5, 2.5, 5e-324, -5e-324, 1e-310, -1e-310, 2.0 ** -1022, -np.inf, np.inf])
    for n in (2, 11, 64, 300):
        x = vals[rng.integers(0, vals.size, size=(4, n))]
        check(x, rng.exponential(size=(4, n)))
    # -0.0 sorts below +0.0: the lower half of the weight is on -0.0
    out = check([[0.0, -0.0]], [[1.0, 1.0]], [0.0, 0.25, 0.5, 1.0])
    assert [math.copysign(1.0, v) for v in out[0]] == [-1.0, -1.0, 1.0, 1.0] and not out.any()
    out = check([[np.inf, 3.0, -np.inf]], [[1.0, 2.0, 1.0]], [0.0, 0.5, 1.0])
    assert out[0].tolist() == [-np.inf, 3.0, np.inf]


def test_who_takes_part():
    # a particle of weight 0 is left out whatever its state, NaN included; so is one of weight +inf
    out = check([[np.nan, 1.0, 2.0, NEG_NAN, 3.0]], [[0.0, 1.0, 1.0, 0.0, np.inf]], [0.0, 0.5, 1.0])
    assert out[0].tolist() == [1.0, 2.0, 2.0]
    # a NaN state that carries weight sorts by its sign bit: -NaN below -inf, +NaN above +inf
    out = check([[np.nan, 1.0, -np.inf, NEG_NAN, np.inf]], [[1.0] * 5], [0.0, 0.3, 0.5, 0.7, 1.0])
    assert ref.same(out[0], [NEG_NAN, -np.inf, 1.0, np.inf, np.nan])
    # nobody takes part: NaN; one NaN weight: NaN at every level, the other steps untouched
    x = np.arange(12.0).reshape(3, 4)
    ws = np.ones((3, 4))
    ws[1] = 0.0
    out = check(x, ws)
    assert np.isnan(out[1]).all() and np.isfinite(out[[0, 2]]).all()
    ws[1] = [1.0, np.nan, 1.0, 1.0]
    ws[2] = [0.0, -1.0, -np.inf, np.inf]                     # negative and infinite weights do not take part either: nobody
    out = check(x, ws)
    assert np.isnan(out[1:]).all() and np.isfinite(out[0]).all()
    assert ref.same(out[1:], np.full((2, len(P)), np.nan))    # the one quiet NaN of the specification


def test_subnormal_and_wide_weights():
    rng = np.random.default_rng(3)
    for n in (3, 65, 300):
        x = rng.normal(size=(5, n))
        ws = np.zeros((5, n))
        ws[0] = TINY * (1 + np.arange(n) % 7)                              # every weight a subnormal (1 .. 7 units): K = -1071
        ws[1] = TINY * (1 + np.arange(n) % 7)
        ws[1, n // 2] = 1.0                                                # tests/smoother_planted.py tiny_weights: one particle has it all
        ws[2] = 2.0 ** rng.integers(-1074, -1000, size=n) * (1 + rng.integers(0, 2 ** 20, size=n) / 2.0 ** 20)
        ws[3] = 2.0 ** -rng.integers(0, 2 * ref.Q_BITS, size=n).astype(float) * rng.uniform(0.5, 1.0, size=n)   # spanning more than 2^BITS
        ws[4] = 2.0 ** rng.integers(-1074, 1024, size=n).astype(float)     # the whole range of a double
        out = check(x, ws)
        assert out[1].tolist() == [x[1, n // 2]] * len(P)
        q, K = ref.integer_weights(ws[0])
        assert n < 7 or (K == -1071 and q[0] == 2 ** (ref.Q_BITS - 3))   # 7 units = 0.875 2^-1071; one unit = 2^(-1074 + 1071) of the scale
        q, K = ref.integer_weights(ws[3])
        assert min(q) == 0 or n == 3                                       # the small ones become 0 ...
    # ... at exactly half a unit the tie goes to even (K = 0, a unit is 2^-BITS): 1/2 -> 0, 3/2 -> 2, just above 1/2 -> 1
    h = 2.0 ** -(ref.Q_BITS + 1)
    ws = np.array([[0.5, h, 3.0 * h, h * (1 + 2.0 ** -52)]])
    assert ref.integer_weights(ws[0])[0] == [2 ** (ref.Q_BITS - 1), 0, 2, 1]
    out = check([[5.0, 1.0, 2.0, 3.0]], ws, [0.0, 1.0])
    assert out[0].tolist() == [2.0, 5.0]                                   # the particle that rounds to 0 carries no weight


@pytest.mark.parametrize("n", SIZES)
def test_accuracy_against_the_dense_weights(n):
    """The returned v at level p against the CDF of the dense weights, taken by math.fsum: cdf(v) >= p - delta and cdf(v-) <=
    p + delta with delta = n 2^(2 - SMOOTH_Q_BITS).  Derivation: with s = 2^(BITS - K) every q_i is within 1/2 of s ws_i, so the
    integer mass Q_A of any set A of particles is within n / 2 of s w_A, and W within n / 2 of s w_tot; the particle with the
    largest exponent has ws 2^-K >= 1/2, so s w_tot >= 2^(BITS - 1).  T = floor(floor(p 2^64) W / 2^64) lies in (p W - 2, p W].
    The definition gives Q(<= v) > T and Q(< v) <= T, so
        s w(<= v) >= Q(<= v) - n / 2 > p W - 2 - n / 2 >= p (s w_tot - n / 2) - 2 - n / 2 >= p s w_tot - (n + 2),
        s w(< v)  <= Q(< v) + n / 2 <= p W + n / 2 <= p (s w_tot + n / 2) + n / 2 <= p s w_tot + n,
    and dividing by s w_tot >= 2^(BITS - 1): cdf(v) > p - (n + 2) 2^(1 - BITS), cdf(v-) <= p + n 2^(1 - BITS); (n + 2) <= 2 n from
    n = 2 on, and one particle has cdf(v) = 1, cdf(v-) = 0.  A bound from the specification, not from what the code returns."""
    rng = np.random.default_rng(500 + n)
    delta = n * 2.0 ** (2 - ref.Q_BITS)
    worst = 0.0
    for ws in (rng.exponential(size=n), rng.exponential(size=n) ** 8 * 1e-30, np.full(n, 0.3), 2.0 ** -rng.integers(0, 50, size=n).astype(float)):
        x = np.round(rng.normal(size=n), 1)                  # (ties)
        p = np.concatenate([[0.0, 1.0, 0.5], rng.uniform(size=5)])
        out = L.host_smooth_quantiles(x[None], ws[None], p)[0]
        tot = math.fsum(ws)
        for pj, v in zip(p, out):
            at, below = math.fsum(ws[x <= v]) / tot, math.fsum(ws[x < v]) / tot
            worst = max(worst, pj - at, below - pj)
            assert at >= pj - delta and below <= pj + delta, (pj, v, below, at, delta)
    print("n = %d: worst excess %.3g against delta = %.3g" % (n, worst, delta))


def test_invalid_arguments():
    x, ws = np.zeros((2, 4)), np.ones((2, 4))
    for bad in ([], [0.5] * 9, [-1e-9], [1.0000001], [1.5], [np.nan]):
        with pytest.raises(L.SmcError):
            L.host_smooth_quantiles(x, ws, bad)
    lib = L.lib()
    one = np.array([0.5])
    assert lib.smc_host_smooth_quantiles(2, 4, None, None, None, 1, None) != 0
    assert lib.smc_host_smooth_quantiles(0, 4, L._d(x), L._d(ws), L._d(one), 1, L._d(np.zeros(2))) != 0
    assert lib.smc_host_smooth_quantiles(2, 0, L._d(x), L._d(ws), L._d(one), 1, L._d(np.zeros(2))) != 0
    assert lib.smc_smooth_quantiles(None, None, None, None, None, None, 0, L._d(one), 1, L._d(np.zeros(2))) != 0


def test_python_refusals_before_any_device_call(monkeypatch):
    """too many levels, a level outside [0, 1], smooth=False, a bad component, MarginalUCSV and IBIS: each raises before a handle
    exists (creating one is made an error for the length of the test)"""
    def no_device(*a, **k):
        raise AssertionError("a device call")
    monkeypatch.setattr(L, "Handle", no_device)
    m1 = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
    uc = smc.UCSV((0.2, 0.3), 1.0, (-1.0, -0.5))
    y = np.linspace(-1.0, 1.0, 6)
    for kw in (dict(quantiles=[0.1] * 9), dict(quantiles=[]), dict(quantiles=[0.5, 1.5]), dict(quantiles=[-0.1]), dict(quantiles=[np.nan]),
               dict(quantiles=[0.5], smooth=False, paths=4), dict(quantiles=[0.5], component=1), dict(quantiles=[0.5], component=-1)):
        with pytest.raises(ValueError):
            smc.smoother(64, y, m1, seed=5, **kw)
    with pytest.raises(ValueError):
        smc.smoother(64, y, [uc, uc], seed=5, quantiles=[0.5], component=3)
    with pytest.raises(ValueError):
        smc.smoother(64, y, None, rows=(L.MODEL_SV1D, np.array([[-1.0, 0.95, 0.3]])), seed=5, quantiles=[2.0])
    mu = smc.MarginalUCSV((0.2, 0.3), 1.0, (-1.0, -0.5))
    with pytest.raises(L.SmcError, match="rb_smoother"):      # the error class smoother refuses the family with
        smc.smoother(64, y, mu, seed=5, quantiles=[0.5])
    with pytest.raises(AssertionError, match="a device call"):     # (valid arguments do reach the device)
        smc.smoother(64, y, m1, seed=5, quantiles=[0.25, 0.5, 0.75])
    # smoothed_quantiles: IBIS names its own exact quantile; an SMC sampler checks the levels first
    from ibis_reference import case_readme
    from oracle_backend import OracleBackend
    tmap, prior, model = case_readme(smc)
    ib = smc.IBIS(16, model, prior, 3, 0.5, seed=7, theta_map=tmap)
    with pytest.raises(TypeError, match="rts_quantile"):
        smc.smoothed_quantiles(ib, y, [0.5])
    s = smc.SMC(16, 16, model, prior, 2, 0.6, seed=22, backend=OracleBackend(), theta_map=tmap)
    for bad, comp in (([0.1] * 9, 0), ([1.5], 0), ([], 0), ([0.5], 1)):
        with pytest.raises(ValueError):
            smc.smoothed_quantiles(s, y, bad, component=comp)
    with pytest.raises(AssertionError, match="a device call"):
        smc.smoothed_quantiles(s, y, [0.5])
