"""Backward simulation on the host (smc_host_sample_paths; smc_spec.h "backward simulation") against references
that share no arithmetic with the library (tests/paths_reference.py).  No GPU.

  * every index of every path against the long-double CDF of its step and the path's own uniform, rebuilt from the Philox export
  * the law of the marginal: P(idx_t = i) is the FFBS smoothed weight (chi-square against smc_host_smooth; the filter weights fail)
  * the joint law of LG1D against the exact Rauch-Tung-Striebel means and lag-one covariances
  * invariants (a path does not depend on M; seeds and streams; xs is the gather), planted clouds, every refusal
"""
import numpy as np
import pytest

import paths_reference as PR
import smoother_planted as P
import smoother_reference as R

LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
LG_SHARP = [0.5, 1.0, 0.9, 1e-4, 0.0, 1.0]
ROWS = {R.LG1D: LG, R.SV1D: [-1.0, 0.95, 0.3], R.UCSV3D: [0.2, 0.3, 1.0, -1.0, -0.5]}
SEED, STREAM = 0x5EEDC0FFEE12345, 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def gather(x, idx):
    """xs [T][d][M] of the clouds x [T][d][n] at idx [T][M]"""
    return np.array([x[t][:, idx[t]] for t in range(idx.shape[0])])


@pytest.mark.parametrize("M", [1, 65])
@pytest.mark.parametrize("T", [1, 2, 12])
@pytest.mark.parametrize("n", [1, 65, 300])
@pytest.mark.parametrize("model,raw", [(R.LG1D, LG), (R.SV1D, ROWS[R.SV1D]), (R.UCSV3D, ROWS[R.UCSV3D]), (R.LG1D, LG_SHARP)],
                         ids=["lg", "sv", "ucsv", "lg_sharp"])
def test_indices_against_longdouble_cdf(L, ob, model, raw, n, T, M):
    """F_{i-1} - tol <= u / 2^64 < F_i + tol for every path and step, tol = (n + 1) 2^-40 + 1000 eps: each q_l is off by at most
    half a unit of 2^-40 plus the relative error of sp_exp and of the fma chain (a few hundred eps at these magnitudes), their
    total is at least one unit, and the floor in r costs one more.  Observed: in every case below the index is the one the exact
    CDF picks (no u outside [F_{i-1}, F_i) at all; tol is 2.7e-10 at n = 300); see DESIGN.md 2f."""
    x, w = PR.recorded_clouds(L, ob, model, raw, n, T, stream=STREAM)
    assert np.all((w > 0).any(axis=1))
    if raw is LG_SHARP and n >= 65 and T > 1:
        assert (w == 0).mean() > 0.5
    idx, xs = L.host_sample_paths(model, raw, x, w, M, SEED, STREAM)
    worst = PR.check_indices(L, model, raw, x, w, idx, SEED, STREAM)
    print("model %d n %d T %d M %d: largest distance of a u outside its exact interval %.3e" % (model, n, T, M, worst))
    assert np.array_equal(bits(xs), bits(gather(x, idx)))
    assert np.all(w[np.arange(T)[:, None], idx] > 0)                   # zero-weight particles are never chosen


@pytest.mark.parametrize("model", [R.LG1D, R.UCSV3D])
def test_marginal_law_is_the_smoothed_weight(L, ob, model):
    """n = 64, T = 6, M = 20000: the counts of idx[t] against M ws_t of smc_host_smooth, Pearson's chi-square below the 1 - 1e-6
    quantile at every t; the same statistic against the FILTER weights exceeds it at some t < T - 1"""
    n, T, M = 64, 6, 20000
    raw = ROWS[model]
    x, w = PR.recorded_clouds(L, ob, model, raw, n, T)
    ws, _, _ = L.host_smooth(model, raw, x, w, moments=False)
    idx, _ = L.host_sample_paths(model, raw, x, w, M, 20260117, 0, want_x=False)
    told = False
    for t in range(T):
        counts = np.bincount(idx[t], minlength=n)
        stat, cells = PR.chi2_cells(counts, M * ws[t])
        bound = PR.chi2_bound(cells - 1)
        fstat, fcells = PR.chi2_cells(counts, M * w[t])
        print("t %d: chi2 %.1f (%d cells, bound %.1f); against the filter weights %.1f" % (t, stat, cells, bound, fstat))
        assert stat <= bound, (t, stat, bound)
        if t < T - 1 and fstat > PR.chi2_bound(fcells - 1):
            told = True
    assert told


def test_joint_law_against_rts(L, ob):
    """LG1D, K = 32 independent filters of n = 256, T = 12, M = 256 paths each: the path means of x_t and the sample covariances
    of (x_t, x_{t+1}) over the paths, averaged over the filters, against the exact RTS mean and lag-one covariance:
    z = |avg - exact| / (sd over filters / sqrt(K)) <= 4.5 at every t.  Independent draws from the marginals would have
    covariance 0: the same statistic against 0 exceeds 4.5 at most steps."""
    K, n, T, M = 32, 256, 12, 256
    _, y = L.simulate(R.LG1D, LG, T, 1998)
    m_rts, _ = R.rts_smoother(LG, y)
    C_rts = PR.rts_lag_one(LG, y)
    means, covs = np.zeros((K, T)), np.zeros((K, T - 1))
    for k in range(K):
        x, w = PR.recorded_clouds(L, ob, R.LG1D, LG, n, T, seed=300 + k)
        _, xs = L.host_sample_paths(R.LG1D, LG, x, w, M, 9000 + k, 0)
        means[k], covs[k] = PR.path_moments(xs[:, 0, :])
    zm, zc, z0 = PR.z_scores(means, m_rts), PR.z_scores(covs, C_rts), PR.z_scores(covs, 0.0)
    print("max z of the means %.2f, of the covariances %.2f; covariances against 0: %s" % (zm.max(), zc.max(), np.round(z0, 1)))
    assert np.all(zm <= 4.5), zm
    assert np.all(zc <= 4.5), zc
    assert (z0 > 4.5).sum() > (T - 1) // 2, z0


@pytest.mark.parametrize("model", [R.LG1D, R.SV1D, R.UCSV3D])
def test_invariants(L, ob, model):
    raw = ROWS[model]
    x, w = PR.recorded_clouds(L, ob, model, raw, 300, 12)
    i300, x300 = L.host_sample_paths(model, raw, x, w, 300, SEED, STREAM)
    i65, x65 = L.host_sample_paths(model, raw, x, w, 65, SEED, STREAM)
    assert np.array_equal(i300[:, :65], i65) and np.array_equal(bits(x300[:, :, :65]), bits(x65))   # path p does not depend on M
    assert np.array_equal(bits(x300), bits(gather(x, i300)))
    assert not np.array_equal(L.host_sample_paths(model, raw, x, w, 65, SEED + 1, STREAM)[0], i65)
    assert not np.array_equal(L.host_sample_paths(model, raw, x, w, 65, SEED, STREAM + 1)[0], i65)
    assert np.array_equal(L.host_sample_paths(model, raw, x, w, 65, SEED, STREAM, want_x=False)[0], i65)
    assert len({tuple(i300[:, p]) for p in range(300)}) > 100          # the paths differ from one another


def test_zero_weight_particles_are_never_chosen(L, ob):
    x, w = PR.recorded_clouds(L, ob, R.LG1D, LG_SHARP, 300, 12)
    assert (w == 0).mean() > 0.5
    idx, xs = L.host_sample_paths(R.LG1D, LG_SHARP, x, w, 300, SEED, STREAM)
    assert np.all(w[np.arange(12)[:, None], idx] > 0)
    for name in P.ON_ZERO:                                            # NaN / inf states on them change nothing
        px, pw = P.variant(name, R.LG1D, LG_SHARP, x, w)
        assert not np.all(np.isfinite(px))
        i2, x2 = L.host_sample_paths(R.LG1D, LG_SHARP, px, pw, 300, SEED, STREAM)
        assert np.array_equal(i2, idx) and np.array_equal(bits(x2), bits(xs))


@pytest.mark.parametrize("n", [65, 300])
@pytest.mark.parametrize("name", P.ALIVE)
@pytest.mark.parametrize("model", [R.LG1D, R.SV1D, R.UCSV3D])
def test_planted_clouds_against_longdouble_cdf(L, ob, model, name, n):
    """far_apart (cross terms that underflow, a target 60 scales from every source), ties, subnormal weights, one particle alive:
    every index within the bound of the plain records, every path complete"""
    T, M = 6, 65
    raw = ROWS[model]
    x, w = PR.recorded_clouds(L, ob, model, raw, n, T)
    px, pw = P.variant(name, model, raw, x, w)
    idx, xs = L.host_sample_paths(model, raw, px, pw, M, SEED, STREAM)
    PR.check_indices(L, model, raw, px, pw, idx, SEED, STREAM)
    assert np.array_equal(bits(xs), bits(gather(px, idx)))
    assert np.all(pw[np.arange(T)[:, None], idx] > 0)
    if name == "one_alive":
        assert np.all(idx[P.mid(T)] == int(np.argmax(pw[P.mid(T)])))


@pytest.mark.parametrize("model", [R.LG1D, R.UCSV3D])
def test_collapsed_filter_has_no_paths(L, ob, model):
    T = 6
    x, w = PR.recorded_clouds(L, ob, model, ROWS[model], 65, T)
    for t_dead in P.dead_steps(T):
        px, pw = P.dead_at(x, w, t_dead)
        idx, xs = L.host_sample_paths(model, ROWS[model], px, pw, 65, SEED, STREAM)
        assert np.all(idx == -1) and np.all(np.isnan(xs)), t_dead


def test_a_path_ends_where_no_source_reaches_it(L):
    """T = 2, two sources whose transition density at the only target is exactly 0 in the log domain (a distance whose square
    overflows): every log-weight is -inf, the path has its last step and reads -1 / NaN before it"""
    x = np.array([[[0.0, 1.0]], [[1e200, 1e200]]])
    w = np.full((2, 2), 0.5)
    idx, xs = L.host_sample_paths(R.LG1D, LG, x, w, 5, SEED, STREAM)
    assert np.all(idx[1] >= 0) and np.all(idx[0] == -1)
    assert np.all(np.isnan(xs[0])) and np.all(xs[1] == 1e200)


def test_refusals(L):
    x, w = np.zeros((1, 1, 2)), np.full((1, 2), 0.5)
    with pytest.raises(L.SmcError):
        L.host_sample_paths(L.MODEL_UCSV_RB, ROWS[R.UCSV3D], np.zeros((1, 4, 2)), w, 4, 1)
    for model, k in ((R.LG1D, 2), (R.SV1D, 2), (R.UCSV3D, 0), (R.UCSV3D, 1)):
        for bad in (0.0, -1.0, np.nan, np.inf):
            raw = list(ROWS[model])
            raw[k] = bad
            with pytest.raises(L.SmcError):
                L.host_sample_paths(model, raw, np.zeros((1, R.DIM[model], 2)), w, 4, 1)
    for M in (0, -3):
        with pytest.raises(L.SmcError):
            L.host_sample_paths(R.LG1D, LG, x, w, M, 1)
    lib = L.lib()
    idx = np.zeros(4, dtype=np.int32)
    args = (L._d(np.array(LG)), L._d(x.ravel()), L._d(w.ravel()))
    ip = idx.ctypes.data_as(L._i32p)
    assert lib.smc_host_sample_paths(1, args[0], 1, (1 << 20) + 1, args[1], args[2], 1, 1, 0, ip, None) == -1    # n > 2^20, before any read
    assert lib.smc_host_sample_paths(1, args[0], 0, 2, args[1], args[2], 1, 1, 0, ip, None) == -1
    assert lib.smc_host_sample_paths(1, args[0], 1, 0, args[1], args[2], 1, 1, 0, ip, None) == -1
    assert lib.smc_host_sample_paths(1, None, 1, 2, args[1], args[2], 1, 1, 0, ip, None) == -1
    assert lib.smc_host_sample_paths(1, args[0], 1, 2, args[1], args[2], 1, 1, 0, None, None) == -1
    assert lib.smc_host_sample_paths(1, args[0], 1, 2, args[1], args[2], 2, 1, 0, ip, None) == 0
