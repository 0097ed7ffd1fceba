"""GPU tests of the IBIS sampler (smc.IBIS; csrc/smc_ibis_kernels.h) against the CPU restatement of src/ibis.jl
(tests/ibis_reference.py): every float64 array compared with ==, never approx."""
import signal

import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
from oracle import binding as ob
from ibis_reference import IbisReference, LG_TRUE, Y_SEED, case_one_parameter, case_readme, grid_posterior_A

pytestmark = pytest.mark.gpu

CASES = {"readme": case_readme, "one": case_one_parameter}
# standard error of the mean of E[A] over the K = 16 seeds of test_ibis_host.test_restatement_recovers_the_exact_posterior (M = 512)
SE_K_SEEDS = 0.001507


def _y(T=100):
    return smc.simulate(smc.UnivariateLinearGaussian(**LG_TRUE), T, seed=Y_SEED)[1]


def reference_run(case, M, predict_first, seed, y):
    """the restatement's online run, with the branches a comparison must exercise asserted on it first"""
    tmap, prior, _ = CASES[case](smc)
    r = IbisReference(M, tmap, prior, 3, 0.5, seed=seed, predict_first=predict_first).run(y)
    assert r.n_rejuvenations >= 2 and r.n_out_of_support >= 1 and r.n_accepted >= 1, (r.n_rejuvenations, r.n_out_of_support, r.n_accepted)
    return r


def _ibis(case, M, predict_first, seed):
    tmap, prior, model = CASES[case](smc)
    return smc.IBIS(M, model, prior, 3, 0.5, seed=seed, theta_map=tmap, predict_first=predict_first)


def _same_state(ib, r):
    for name, ref in (("theta", r.theta), ("x", r.x), ("Sigma", r.S), ("logZ", r.logZ), ("logw", r.logw)):
        got = getattr(ib, name)
        assert got.shape == ref.shape and np.array_equal(got, ref), name
    assert ib.ess == r.ess and ib.acc_ratio == r.acc_ratio and np.array_equal(ib.accepted, r.accepted)
    assert ib.n_rejuvenations == r.n_rejuvenations


ONLINE = [(c, M, pf) for c in ("readme", "one") for M in (512, 1000, 77) for pf in (False, True)]


@pytest.mark.parametrize("case,M,predict_first", ONLINE)
def test_online_steps_equal_restatement(case, M, predict_first):
    """smc2 + smc2_step over T = 100: the ESS of every step, and theta, x, Sigma, logZ, logw, the accepted mask and acc_ratio at
    the end, bit for bit; M not a multiple of the workgroup or of the outer segment included"""
    y = _y()
    r = reference_run(case, M, predict_first, 5, y)
    ib = _ibis(case, M, predict_first, 5)
    ess = []
    smc.smc2(ib, y)
    ess.append(ib.ess)
    for t in range(2, len(y) + 1):
        smc.smc2_step(ib, y, t, verbose=False)
        ess.append(ib.ess)
    assert ess == r.ess_trace
    _same_state(ib, r)
    ib.close()


@pytest.mark.parametrize("window", [1, 7, 16])
def test_run_windows_equal_steps(window):
    """smc2_run with windows 1, 7, 16 over T = 100 (a multiple of neither 7 nor 16) == the step-by-step run == the restatement"""
    y = _y()
    r = reference_run("readme", 77, False, 5, y)
    ib = _ibis("readme", 77, False, 5)
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, len(y), window=window, verbose=False)
    assert ib.t == len(y)
    _same_state(ib, r)
    ib.close()


@pytest.mark.parametrize("M", [77, 512, 2 ** 16 + 5])
def test_device_records_equal_host_records(M):
    """the segment records the window kernel computes == smc_host_outer_window on the lik the same call returned, bit for bit
    (they are integers), from zero log-weights and from the log-weights a kept window left"""
    y = _y(24)
    ib = _ibis("readme", M, False, 11)
    h = ib._handle()
    for lo, k, keep in ((0, 1, 1), (1, 7, 4), (5, 16, 16), (21, 3, 3)):
        logw = ib.logw
        rec, lik = h.window(y[lo:lo + k], want_lik=True)
        assert rec.shape == (k, (M + 7) // 8, 4)
        assert np.array_equal(rec, L.host_outer_window(logw, lik))
        h.commit(keep)
        assert np.array_equal(ib.logw, L.host_outer_advance(logw, np.zeros(M), lik, keep)[0])
    ib.close()


def test_resample_is_a_value_copy():
    """resample_ alone: the gather equals the restatement's; copies of one ancestor are independent afterwards (a rejuvenation
    gives them distinct theta rows, a step then moves each by its own row)"""
    y = _y(12)
    tmap, prior, _ = case_readme(smc)
    r = IbisReference(77, tmap, prior, 3, 0.5, seed=9)
    ib = _ibis("readme", 77, False, 9)
    r.smc2(y)
    smc.smc2(ib, y)
    for t in range(2, 9):
        r._propagate(float(y[t - 1]), True)
        ess, _ = smc.ibis._window(ib, y[t - 1:t], 0.0)
    a = r.resample()
    assert np.array_equal(smc.resample_(ib), a) and len(set(a.tolist())) < 77
    for name, ref in (("theta", r.theta), ("x", r.x), ("Sigma", r.S), ("logZ", r.logZ), ("logw", r.logw)):
        assert np.array_equal(getattr(ib, name), ref), name
    r.rejuvenate(y[:8])
    smc.rejuvenate_(ib, y[:8])
    r._propagate(float(y[8]), True)
    smc.ibis._window(ib, y[8:9], 0.0)
    th, x = ib.theta, ib.x
    dup = [(i, i + 1) for i in range(76) if a[i] == a[i + 1]]
    assert dup and any(not np.array_equal(th[i], th[j]) and x[i] != x[j] for i, j in dup)
    for name, ref in (("theta", r.theta), ("x", r.x), ("Sigma", r.S), ("logZ", r.logZ), ("logw", r.logw)):
        assert np.array_equal(getattr(ib, name), ref), name
    ib.close()


# ---- every d of the (row kind, d) dispatch: theta[i] is row entry i for i < min(d, 6), the rest of the row is constant ---------
FIRST_D_CHAIN = 2


def case_first_d(d):
    """theta = the first d of (A, B, Q, R, x0, sigma0, -, -): with d = 7, 8 the surplus parameters reach no row entry and act
    through the prior only.  Bounded priors on A and on the seventh parameter, a LogNormal on Q, R and sigma0"""
    parts = [smc.TruncatedNormal(0, 1, -1, 1), smc.Normal(1.0, 0.2), smc.LogNormal(), smc.LogNormal(), smc.Normal(0.0, 1.0), smc.LogNormal(),
             smc.Uniform(-1.0, 1.0), smc.Normal(0.0, 1.0)]
    tmap = smc.ThetaMap(L.MODEL_LG1D, [i if i < d else -1 for i in range(6)], [0.5, 1.0, 0.9, 0.8, 0.0, 1.0])
    return tmap, smc.product_distribution(parts[:d])


def _snapshot(r):
    return {name: getattr(r, name).copy() for name in ("theta", "x", "S", "logZ", "logw")}


def restate_first_d(d, M, monkeypatch):
    """the restatement alone (no GPU), T = 6, chain 2: its cloud after the filter, after the rejuvenation, and lik of a window of 2
    steps after a permutation with repeats.  The factor of the random walk is the restatement's own; a cloud of one particle has
    none, and takes 0.1 I"""
    tmap, prior = case_first_d(d)
    y = _y(8)
    r = IbisReference(M, tmap, prior, FIRST_D_CHAIN, 0.5, seed=7)
    out = {"r": r, "tmap": tmap, "prior": prior, "theta0": r.theta.copy(), "y": y}
    for m in range(M):
        r.x[m], r.S[m], r.logZ[m] = ob.kalman_log_likelihood(r._row(r.theta[m]), y[:6], predict_first=False)
    r.logw = r.logZ.copy()
    out["filtered"] = _snapshot(r)
    chol, uni = ob.rw_factor(r.theta) if M >= 2 else (0.1 * np.eye(d), d == 1)
    scales = 0.5 * np.arange(FIRST_D_CHAIN, 0, -1)
    out["chol"], out["s"] = chol, (scales * scales if uni else scales)
    out["move_seed"] = (r.seed << 20) + r._calls + 1                      # the restatement's next seed
    with monkeypatch.context() as mp:
        mp.setattr(ob, "rw_factor", lambda theta: (chol, uni))
        r.rejuvenate(y[:6])
    out["moved"] = _snapshot(r)
    out["n_rejected"] = M * FIRST_D_CHAIN - r.n_accepted - r.n_out_of_support
    out["a"] = a = np.array([(3 * m) % M if m % 4 else (M - 1 - m) // 2 for m in range(M)], dtype=np.int32)
    for name in ("theta", "x", "S", "logZ", "logw"):
        setattr(r, name, getattr(r, name)[a].copy())
    out["wlik"] = np.zeros((2, M))
    for m in range(M):                                                    # the host twin from the copied state on the copied row
        row = np.array(r._row(r.theta[m]))
        row[4], row[5] = r.x[m], r.S[m]
        out["wlik"][:, m] = L.host_kalman_steps(row, y[6:8], True)[2]
    return out


def _same_arrays(h, snap):
    g = h.get(theta=True, x=True, S=True, logZ=True, logw=True)
    for name, ref in snap.items():
        assert g[name].shape == ref.shape and np.array_equal(g[name], ref), name


@pytest.mark.parametrize("M", [1, 65])
@pytest.mark.parametrize("d", range(1, 9))
def test_every_d_equals_restatement(d, M, monkeypatch):
    """the dispatch on d for scalar rows, a lone lane and a ragged second wave: theta, x, S, logZ, logw after set_theta + filter and
    after rejuvenate (with moved and its count) are the restatement's, and a window after a permutation with repeats gives the
    twin's lik on the copied rows.  At M = 65 the restatement alone must hold accepted and rejected moves"""
    w = restate_first_d(d, M, monkeypatch)
    r, y = w["r"], w["y"]
    assert M == 1 or (r.n_accepted >= 1 and w["n_rejected"] >= 1), (r.n_accepted, w["n_rejected"], r.n_out_of_support)
    fam, par = w["prior"].spec()
    h = L.IbisHandle(M, d, np.atleast_1d(fam), np.atleast_2d(par), w["tmap"].raw_from, w["tmap"].raw_const, seed=7)
    h.set_theta(w["theta0"])
    h.filter(y[:6])
    _same_arrays(h, w["filtered"])
    n, moved = h.rejuvenate(y[:6], 1.0, w["chol"], w["s"], w["move_seed"])
    _same_arrays(h, w["moved"])
    assert np.array_equal(moved, r.accepted) and n == int(r.accepted.sum())
    h.permute(w["a"])
    _, lik = h.window(y[6:8], want_lik=True)
    assert np.array_equal(lik, w["wlik"])
    h.close()


@pytest.mark.parametrize("case,predict_first", [("readme", False), ("readme", True)])
def test_density_tempered_equals_restatement(case, predict_first):
    y = _y()
    tmap, prior, _ = CASES[case](smc)
    r = IbisReference(512, tmap, prior, 3, 0.5, seed=4, predict_first=predict_first)
    ladder = r.density_tempered(y)
    assert r.n_rejuvenations >= 2 and r.n_accepted >= 1
    ib = _ibis(case, 512, predict_first, 4)
    stages = smc.density_tempered(ib, y, verbose=False)
    assert stages == ladder
    _same_state(ib, r)
    assert np.array_equal(smc.expected_parameters(ib), r.expected_parameters())
    ib.close()


@pytest.mark.parametrize("predict_first", [False, True])
def test_online_logZ_is_the_batched_kalman_logZ(predict_first):
    """after a run with rejuvenations the online logZ[m] is smc.log_likelihood_kalman(y[:t], model(theta[m])) bit for bit"""
    y = _y()
    tmap, prior, model = case_readme(smc)
    ib = _ibis("readme", 1000, predict_first, 5)
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, 60, window=16, verbose=False)
    assert ib.n_rejuvenations >= 1 and ib.t == 60
    th = ib.theta
    x, S, z = smc.log_likelihood_kalman(y[:60], [model(t) for t in th], predict_first=predict_first)
    assert np.array_equal(ib.logZ, z) and np.array_equal(ib.x, x) and np.array_equal(ib.Sigma, S)
    ib.close()


def test_a_million_parameter_particles():
    """M = 2^20, T = 200, theta = A: the weights sum to one, the ESS is in range, and the posterior mean of A is within
    4 posterior-sd / sqrt(ess at the end) + the K-seed standard error of the restatement (test_ibis_host) of the grid value"""
    def too_long(*_):
        raise TimeoutError("the 2^20-particle run exceeded its time limit")
    old = signal.signal(signal.SIGALRM, too_long)
    signal.alarm(300)
    try:
        M = 2 ** 20
        y = _y(200)
        mean, sd = grid_posterior_A(y)
        ib = _ibis("one", M, False, 1)
        smc.smc2(ib, y)
        smc.smc2_run(ib, y, 2, len(y), window=16, verbose=False)
        w = ib.omega
        est = smc.expected_parameters(ib)[0]
        print("M = 2^20: ess = %.1f, rejuvenations = %d, E[A] = %.6f, grid = %.6f (sd %.6f)" % (ib.ess, ib.n_rejuvenations, est, mean, sd))
        assert abs(w.sum() - 1.0) <= 1e-12 and 1.0 <= ib.ess <= M
        assert abs(est - mean) <= 4.0 * sd / np.sqrt(ib.ess) + SE_K_SEEDS
        ib.close()
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)
