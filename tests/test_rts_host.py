"""CPU tests of the RTS smoother of an IBIS cloud: the host twins smc_host_ibis_smooth / smc_host_ibis_sample_paths (the
specification the device equals bit for bit, tests/test_gpu_rts.py) against the long-double references of tests/rts_reference.py."""
import numpy as np
import pytest

import rts_reference as RR

EPS = RR.EPS
# (A, B, Q, R, x0, sigma0): the local level, |A| < 1, a negative A, B != 1, Q / R from 1e-4 to 1e4
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
WELL = ROWS[:4]
# The backward pass against the long-double recursion over the twin's own filtered record, every case below (T up to 200):
# measured 4.32 eps (xs) and 7.60 eps (Ps) for the twin (x86-64, glibc's libm; both at T = 200 or 12); the bounds are 8 times
# that, headroom across libm and compilers.  The paths, the same way: measured 2.52 eps (T = 200).
BOUND_XS, BOUND_PS, BOUND_PATH = 8 * 4.32 * EPS, 8 * 7.60 * EPS, 8 * 2.52 * EPS


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def series(L, T, seed=1998):
    return L.simulate(L.MODEL_LG1D, [0.9, 1.0, 0.5, 0.8, 0.0, 1.0], T, seed)[1]


def random_rows(M, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(-0.99, 1.0, M), rng.uniform(0.5, 2.0, M), np.exp(rng.normal(-1, 1, M)), np.exp(rng.normal(-1, 1, M)),
                            rng.normal(0, 1, M), np.exp(rng.normal(0, 0.5, M))])


def scaled_error(got, ref, Ps):
    """largest |got - ref| / (max |ref| + sqrt(max Ps)) per column (one parameter particle or path), over the columns"""
    ref = np.asarray(ref, dtype=RR.LD)
    scale = np.abs(ref).max(axis=0) + np.sqrt(np.asarray(Ps, dtype=RR.LD).max(axis=0))
    return float((np.abs(np.asarray(got, dtype=RR.LD) - ref).max(axis=0) / scale).max())


@pytest.mark.parametrize("predict_first", [False, True])
@pytest.mark.parametrize("T", [1, 2, 12, 200])
def test_backward_pass_against_longdouble_recursion(L, T, predict_first):
    y = series(L, T)
    _, xs, Ps, xf, Sf = L.host_ibis_smooth(ROWS, np.zeros(len(ROWS)), y, predict_first, states=True, filtered=True)
    rx, rP, _, _ = RR.backward(ROWS, xf, Sf)
    ex = scaled_error(xs, rx, rP)
    eP = float((np.abs(Ps.astype(RR.LD) - rP) / rP).max())
    print("T %d predict_first %d: xs %.2f eps, Ps %.2f eps" % (T, predict_first, ex / EPS, eP / EPS))
    assert np.array_equal(bits(xs[T - 1]), bits(xf[T - 1])) and np.array_equal(bits(Ps[T - 1]), bits(Sf[T - 1]))
    assert ex <= BOUND_XS and eP <= BOUND_PS
    assert np.all(Ps > 0) and np.all(Ps <= Sf * (1 + 4 * EPS))          # smoothing never adds variance


@pytest.mark.parametrize("predict_first", [False, True])
def test_against_dense_gaussian_conditioning(L, predict_first):
    """the whole chain (the forward filter included) against a reference that shares no recursion with it: rel <= 1e-9"""
    T = 12
    y = series(L, T)
    _, xs, Ps = L.host_ibis_smooth(WELL, np.zeros(len(WELL)), y, predict_first, states=True)
    for m, row in enumerate(WELL):
        mean, var, _ = RR.dense(row, y, predict_first)
        ex = scaled_error(xs[:, m:m + 1], mean[:, None], var[:, None])
        eP = float((np.abs(Ps[:, m].astype(RR.LD) - var) / var).max())
        print("row %d: xs %.2e, Ps %.2e" % (m, ex, eP))
        assert ex <= 1e-9 and eP <= 1e-9


@pytest.mark.parametrize("M", [1, 65, 300])
def test_rows_are_the_summaries_of_the_smoothed_cloud(L, M):
    rows = random_rows(M, 5)
    logw = np.random.default_rng(6).normal(0, 3, M)
    y = series(L, 12)
    out, xs, Ps, xf, Sf = L.host_ibis_smooth(rows, logw, y, states=True, filtered=True)
    for t in range(12):
        assert np.array_equal(bits(out[t]), bits(L.host_ibis_summary(rows, xs[t], Ps[t], logw, 0))), t
    assert np.array_equal(bits(out[11]), bits(L.host_ibis_summary(rows, xf[11], Sf[11], logw, 0)))   # the filtered cloud
    assert np.array_equal(bits(L.host_ibis_smooth(rows, logw, y)), bits(out))                         # without the optional outputs


def test_dead_particles_change_nothing(L):
    M, T = 300, 12
    rows = random_rows(M, 7)
    rng = np.random.default_rng(8)
    logw = rng.normal(0, 3, M)
    dead = rng.uniform(size=M) < 0.4
    dead[[0, 63, 64, M - 1]] = True
    dead[128:192] = True                                                   # a whole chunk
    logw[dead] = -np.inf
    y = series(L, T)
    out = L.host_ibis_smooth(rows, logw, y)
    assert np.all(np.isfinite(out))
    planted = rows.copy()
    planted[dead] = np.nan
    planted[dead & (np.arange(M) % 2 == 0), 2] = np.inf
    assert np.array_equal(bits(L.host_ibis_smooth(planted, logw, y)), bits(out))
    nanw = logw.copy()
    nanw[dead] = np.nan                                                    # a NaN log-weight is dead as well
    assert np.array_equal(bits(L.host_ibis_smooth(planted, nanw, y)), bits(out))
    alive = ~dead                                                          # and the rows are those of the live particles alone
    ref = L.host_ibis_smooth(rows[alive], logw[alive], y)
    assert np.allclose(out[:, :6], ref[:, :6], rtol=1e-12, atol=0)
    none = L.host_ibis_smooth(rows, np.full(M, -np.inf), y)
    assert np.all(np.isnan(none[:, :6])) and np.all(none[:, 6] == -np.inf) and np.all(none[:, 7] == 0)


def test_bad_arguments(L):
    with pytest.raises(L.SmcError):
        L.host_ibis_smooth(ROWS, np.zeros(len(ROWS)), np.zeros(0))
    with pytest.raises(L.SmcError):
        L.host_ibis_sample_paths(ROWS, np.zeros(3), [len(ROWS)], 1)
    with pytest.raises(L.SmcError):
        L.host_ibis_sample_paths(ROWS, np.zeros(3), [-1], 1)
    with pytest.raises(L.SmcError):
        L.host_ibis_sample_paths(ROWS, np.zeros(3), np.zeros(0, dtype=np.int32), 1)
    with pytest.raises(L.SmcError):
        L.host_ibis_sample_paths(ROWS, np.zeros(0), [0], 1)


# ---- paths ---------------------------------------------------------------------------------------------------------------------
SEED = 0x9E3779B97F4A7C15


@pytest.mark.parametrize("predict_first", [False, True])
@pytest.mark.parametrize("T", [1, 2, 12, 200])
def test_paths_against_longdouble(L, T, predict_first):
    y = series(L, T)
    which = np.array([0, 0, 1, 2, 3, 3, 3, 4, 5, 6, 7, 7, 2, 0], dtype=np.int32)
    _, _, _, xf, Sf = L.host_ibis_smooth(ROWS, np.zeros(len(ROWS)), y, predict_first, states=True, filtered=True)
    paths, z = L.host_ibis_sample_paths(ROWS, y, which, SEED, predict_first, want_z=True)
    ref = RR.paths(ROWS, which, xf, Sf, z)
    e = scaled_error(paths, ref, Sf[:, which])
    print("T %d predict_first %d: paths %.2f eps" % (T, predict_first, e / EPS))
    assert e <= BOUND_PATH


def test_normals_are_the_philox_draws_of_the_specification(L):
    T = 5
    y = series(L, T)
    which = np.array([7, 0, 3, 3, 7, 1, 2], dtype=np.int32)
    _, z = L.host_ibis_sample_paths(ROWS, y, which, SEED, want_z=True)
    for p, t in [(0, 0), (0, 4), (1, 4), (2, 1), (3, 2), (4, 0), (5, 3), (6, 4)]:
        assert z[t, p] == RR.normal(L, SEED, p, int(which[p]), t), (p, t)
        for slot in RR.OTHER_SLOTS:                                        # a slot of its own: no other draw's number
            assert z[t, p] != RR.normal(L, SEED, p, int(which[p]), t, slot)
    assert z[4, 0] != z[4, 1] and RR.normal(L, SEED, 0, 7, 4) != RR.normal(L, SEED, 1, 7, 4)      # the two halves of one draw
    assert RR.SLOT_RTS not in RR.OTHER_SLOTS


def test_a_path_does_not_depend_on_the_other_paths(L):
    y = series(L, 12)
    which = (np.arange(300) * 7 % len(ROWS)).astype(np.int32)
    p300 = L.host_ibis_sample_paths(ROWS, y, which, SEED)
    p65 = L.host_ibis_sample_paths(ROWS, y, which[:65], SEED)
    assert np.array_equal(bits(p300[:, :65]), bits(p65))
    cloud = np.vstack([ROWS, random_rows(50, 3)])                           # nor on the rest of the cloud
    assert np.array_equal(bits(L.host_ibis_sample_paths(cloud, y, which, SEED)), bits(p300))
    assert not np.array_equal(L.host_ibis_sample_paths(ROWS, y, which[:65], SEED + 1), p65)
    other = which[:65].copy()
    other[10] = (other[10] + 1) % len(ROWS)
    q = L.host_ibis_sample_paths(ROWS, y, other, SEED)
    same = np.arange(65) != 10
    assert np.array_equal(bits(q[:, same]), bits(p65[:, same])) and not np.array_equal(q[:, 10], p65[:, 10])


def test_joint_law_of_the_paths(L):
    """one row, Mp = 20000 paths, T = 8: the paths are iid draws of a Gaussian vector whose means are xs, variances Ps and lag-one
    covariances C_t = G_t Ps_{t+1}, so the standard errors are exact: sqrt(Ps / Mp) for a mean, Ps sqrt(2 / (Mp - 1)) for a
    variance, sqrt((Ps_t Ps_{t+1} + C_t^2) / (Mp - 1)) for a covariance.  Largest |z| below 4.5 (the criterion of
    test_paths_host.py); the covariances against 0 - what independent draws from the marginals would give - at z > 10."""
    T, Mp, seed = 8, 20000, 20260301
    row = ROWS[1:2]
    y = series(L, T)
    _, xs, Ps, xf, Sf = L.host_ibis_smooth(row, np.zeros(1), y, states=True, filtered=True)
    xs, Ps = xs[:, 0], Ps[:, 0]
    _, _, G, _ = RR.backward(row, xf, Sf)
    Cov = (G[:-1, 0] * Ps[1:]).astype(np.float64)
    assert np.allclose(Cov, RR.dense(row[0], y, False)[2].astype(np.float64), rtol=1e-9)
    x = L.host_ibis_sample_paths(row, y, np.zeros(Mp, dtype=np.int32), seed)
    d = x - x.mean(axis=1, keepdims=True)
    var = (d * d).sum(axis=1) / (Mp - 1)
    cov = (d[:-1] * d[1:]).sum(axis=1) / (Mp - 1)
    zm = np.abs(x.mean(axis=1) - xs) / np.sqrt(Ps / Mp)
    zv = np.abs(var - Ps) / (Ps * np.sqrt(2.0 / (Mp - 1)))
    zc = np.abs(cov - Cov) / np.sqrt((Ps[:-1] * Ps[1:] + Cov * Cov) / (Mp - 1))
    z0 = np.abs(cov) / np.sqrt(Ps[:-1] * Ps[1:] / (Mp - 1))
    print("largest z: means %.2f, variances %.2f, covariances %.2f; covariances against 0: %s" % (zm.max(), zv.max(), zc.max(), np.round(z0, 1)))
    assert max(zm.max(), zv.max(), zc.max()) < 4.5
    assert np.all(z0 > 10)
