"""An independent restatement in numpy of csrc/smc_spec.h "quantiles and histograms of the theta cloud": the integer weights q come
from smc_host_theta_weights, everything after them is restated here - a stable argsort on the total-order key, an exact cumsum
in uint64 and the definition; np.add.at for the histogram.  A second, float-only check trusts no integer: float_bounds.
Shared by test_theta_quantiles_host.py (the host twins) and test_gpu_theta_quantiles.py (the device calls)."""
import numpy as np

Q_BITS = 32                        # THETA_Q_BITS


def order_key(x):
    """the IEEE total order as uint64: -NaN < -inf < .. < -0.0 < +0.0 < .. < +inf < +NaN"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def p64(p):
    """floor(p 2^64) clamped to [0, 2^64 - 1] (exact: p 2^64 is a power-of-two scaling)"""
    if not p > 0.0:
        return 0
    if p >= 1.0:
        return (1 << 64) - 1
    return int(p * 2.0 ** 64)


def quantiles(L, theta, logw, p):
    """out [d][np] by sort and cumsum over the integer weights"""
    theta = np.asarray(theta, dtype=np.float64)
    q, _, W = L.host_theta_weights(logw)
    M, d = theta.shape
    out = np.full((d, len(p)), np.nan)
    if W == 0:
        return out
    for i in range(d):
        col = theta[:, i]
        idx = np.argsort(order_key(col), kind="stable")
        cum = np.cumsum(q[idx], dtype=np.uint64)
        assert int(cum[-1]) == W
        for j, pj in enumerate(p):
            T = (p64(float(pj)) * W) >> 64
            a = int(np.searchsorted(cum, np.uint64(T), side="right"))      # the first index with cum > T
            out[i, j] = col[idx[a]]
    return out


def histogram(L, theta, logw, component, lo, hi, nbins):
    """(counts [nbins + 3] = under | bins | over | nan, W)"""
    q, _, W = L.host_theta_weights(logw)
    v = np.asarray(theta, dtype=np.float64)[:, component]
    scale = float(nbins) / (hi - lo)
    slot = np.zeros(v.size, dtype=np.int64)
    nan = v != v
    inside = ~nan & (v >= lo) & (v < hi)
    with np.errstate(invalid="ignore", over="ignore"):
        b = np.where(inside, (v - lo) * scale, 0.0).astype(np.int64)
    slot[inside] = 1 + np.minimum(b[inside], nbins - 1)
    slot[~nan & (v >= hi)] = nbins + 1
    slot[nan] = nbins + 2
    counts = np.zeros(nbins + 3, dtype=np.uint64)
    np.add.at(counts, slot, q)
    return counts, W


def boundary_levels(L, theta, logw, i=0):
    """a level just below and one just above a cumulative boundary of coordinate i (0.5 twice when there is none)"""
    q, _, W = L.host_theta_weights(logw)
    live = np.flatnonzero(q)
    if live.size < 2:
        return 0.5, 0.5
    idx = live[np.argsort(order_key(np.asarray(theta)[live, i]), kind="stable")]
    c = int(np.cumsum(q[idx], dtype=np.uint64)[live.size // 2 - 1]) / W
    return float(np.nextafter(c, 0.0)), float(np.nextafter(c, 1.0))


def float_bounds(col, logw, p, v):
    """The float-only check of one returned value v at level p: with w = exp(logw - max) in double,
        below = sum{w : theta < v} / sum w,   at_or_below = sum{w : theta <= v} / sum w
    it must hold that  below - eps <= p <= at_or_below + eps,  eps = M 2^-31.
    Why: q_m = rint(s w_m) for one scale s, so every partial sum of q is within M / 2 of s times the partial sum of w, and W is
    within M / 2 of s sum w: a mass differs by at most (M / 2 + M / 2) / W, and W >= 0.707 2^Q_BITS > 2^(Q_BITS - 1) because the
    particle with the largest exponent has p >= 0.707.  The quantile's own definition puts p between the two integer masses."""
    M = col.size
    eps = M * 2.0 ** -(Q_BITS - 1)
    alive = np.isfinite(logw) & (np.abs(logw) <= 7e8)
    w = np.zeros(M)
    w[alive] = np.exp(logw[alive] - logw[alive].max())
    below = w[col < v].sum() / w.sum()
    at = w[col <= v].sum() / w.sum()
    return below - eps <= p <= at + eps, (below, p, at, eps)


def families(M, d, seed):
    """name -> (theta [M][d], logw [M]): the clouds both test files run"""
    rng = np.random.default_rng(seed)
    out = {}
    base = rng.normal(size=(M, d)) * np.array([1.0, 1e-3, 50.0, 1.0, 7.0, 1e5, 1e-8, 2.0])[:d] + np.arange(d)
    out["random"] = (base.copy(), rng.normal(size=M))
    out["spread"] = (base.copy(), rng.uniform(-600.0, 600.0, size=M))          # most weights round to 0
    out["equal"] = (base.copy(), np.full(M, -3.25))
    one = np.full(M, -np.inf)
    one[M // 2] = 1.5
    out["one"] = (base.copy(), one)
    # dead particles of every kind carrying NaN and huge theta: they must not appear in any result
    th, lw = base.copy(), rng.normal(size=M)
    kind = np.arange(M) % 7
    for k, dead in ((1, -np.inf), (2, np.nan), (3, 8e8), (4, -8e8)):
        lw[kind == k] = dead
    th[kind == 1] = np.nan
    th[kind == 2] = 1e300
    th[kind == 3] = -1e300
    th[kind == 4] = -np.nan
    out["dead"] = (th, lw)
    # the cloud right after a resample: 5 distinct rows
    rows = rng.normal(size=(5, d))
    out["ties"] = (rows[rng.integers(0, 5, size=M)], rng.normal(size=M))
    # the order of the keys: signed zeros, both signs, denormals
    vals = np.array([-0.0, 0.0, -1.5, 2.5, 5e-324, -5e-324, 1e-310, -1e-310, 2.0 ** -1022, -np.inf, np.inf])
    out["signed"] = (vals[rng.integers(0, vals.size, size=(M, d))], rng.normal(size=M))
    out["none"] = (base.copy(), np.where(np.arange(M) % 2 == 0, -np.inf, np.nan))
    return out
