"""GPU tests of the IBIS sampler over two-state rows (smc_ibis_create_rows with MODEL_LG2D; the kernels of
csrc/smc_ibis_kernels.h with Row = Lg2Row) against compositions of the host twin smc_host_kalman2_steps and the restatement of src/ibis.jl
over it (tests/ibis2_reference.py): every float64 array compared bit for bit, never approx - the posterior mean is the one
statistical check."""
import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
import ibis2_reference as r2
from ibis_reference import case_readme

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 130, 515)     # a lone lane, a full wave, a ragged last wave, several workgroups, no multiple of the outer segment of 8
CASES = {"hp1": r2.case_hp_one, "ar2": r2.case_ar2_three}
Y = r2.y_hp()
# standard error of the mean of E[theta] of the restatement over its seeds 1..16 (M = 512, case hp1, online run): the term
# test_gpu_ibis adds to 4 posterior-sd / sqrt(ess) for its one-parameter case
SE_K_SEEDS = 0.000455


def make(case, M, predict_first=False, seed=7):
    """(handle, restatement) of the same initial cloud"""
    tmap, prior, _ = CASES[case](smc)
    r = r2.Ibis2Reference(M, tmap, prior, 3, 0.5, seed=seed, predict_first=predict_first)
    fam, par = prior.spec()
    h = L.IbisHandle(M, r.d, np.atleast_1d(fam), np.atleast_2d(par), tmap.raw_from, tmap.raw_const, seed=seed, predict_first=predict_first,
                     row_id=L.MODEL_LG2D)
    h.set_theta(r.theta)
    return h, r


def twin_window(r, y, predict0):
    """lik [k][M] and the end state of k steps from the restatement's state, by the host twin"""
    k = len(y)
    lik, x, S = np.zeros((k, r.M)), r.x.copy(), r.S.copy()
    for m in range(r.M):
        row = np.array(r._row(r.theta[m]))
        row[10:12], row[12:15] = r.x[m], r.S[m]
        xf, Sf, lik[:, m] = L.host_kalman2_steps(row, y, predict0)
        x[m], S[m] = xf[-1], Sf[-1]
    return lik, x, S


def same_state(h, r):
    g = h.get(theta=True, x=True, S=True, logZ=True, logw=True)
    for name, ref in (("theta", r.theta), ("x", r.x), ("S", r.S), ("logZ", r.logZ), ("logw", r.logw)):
        assert g[name].shape == ref.shape and np.array_equal(g[name], ref), name


@pytest.mark.parametrize("predict_first", [False, True])
@pytest.mark.parametrize("k", [1, 5, 64])
@pytest.mark.parametrize("M", SIZES)
def test_window_records_commit_and_device_walk(M, k, predict_first):
    """(b) lik [k][M] of smc_ibis_window is the twin's, rec is smc_host_outer_window of that lik; smc_ibis_commit(j), j < k, leaves
    the state of a window of j; smc_ibis_window_ess gives the ess and j of smc_host_outer_walk on those records"""
    y = np.resize(Y, k + 3)
    h, r = make("ar2", M, predict_first)
    rec, lik = h.window(y[:k], want_lik=True)
    wlik, _, _ = twin_window(r, y[:k], predict_first)
    assert np.array_equal(lik, wlik)
    wrec = L.host_outer_window(r.logw, wlik)
    assert rec.shape == (k, (M + 7) // 8, 4) and np.array_equal(rec, wrec)
    j = max(k // 2, 1) if k > 1 else 1
    h.commit(j)
    _, r.x, r.S = twin_window(r, y[:j], predict_first)
    r.logw, r.logZ = L.host_outer_advance(r.logw, r.logZ, wlik, j)
    same_state(h, r)
    # a second window from the committed state, walked on the device
    wlik2, _, _ = twin_window(r, y[j:j + 3], True)
    wrec2 = L.host_outer_window(r.logw, wlik2)
    ess_min = 0.9 * M
    wess, wj = L.host_outer_walk(wrec2, M, ess_min)
    ess, jj = h.window_ess(y[j:j + 3], ess_min)
    assert jj == wj and np.array_equal(ess, wess)
    h.commit(0)
    same_state(h, r)
    h.close()


@pytest.mark.parametrize("xi", [1.0, 0.3])
@pytest.mark.parametrize("case,M,T", [(c, M, 37) for c in ("hp1", "ar2") for M in SIZES] + [(c, 130, T) for c in ("hp1", "ar2") for T in (1, 2)])
def test_rejuvenate_equals_restatement(case, M, T, xi):
    """(c) smc_ibis_rejuvenate (the whole chain in one launch) against the restatement: theta, logZ, x, S, logw and moved.  Where
    the case can show all three branches (a cloud of at least a wave; for hp1 more than two observations - its likelihood does not
    depend on Q11 before the third) the restatement must hold accepted moves, rejected moves and out-of-support proposals, at
    least 5 % of M x chain each"""
    h, r = make(case, M)
    y = Y[:T]
    h.filter(y)
    for m in range(M):
        r.x[m], r.S[m], r.logZ[m] = r2.kalman2(r._row(r.theta[m]), y, False)
    r.logw = r.logZ.copy()
    same_state(h, r)
    if M >= 2:
        chol, uni = L.host_rw_factor(r.theta)
    else:
        chol, uni = 0.1 * np.eye(r.d), r.d == 1
    scales = 0.5 * np.arange(3, 0, -1)
    s = scales * scales if uni else scales
    n, moved = h.rejuvenate(y, xi, chol, s, 1234)
    r.rejuvenate(y, xi, move_seed=1234, chol=chol, s=s)
    if M >= 63 and (case == "ar2" or T == 37):
        need = 0.05 * M * 3
        assert min(r.n_accepted, r.n_rejected, r.n_out_of_support) >= need, (r.n_accepted, r.n_rejected, r.n_out_of_support)
    same_state(h, r)
    assert np.array_equal(moved, r.accepted) and n == int(r.accepted.sum()) and np.array_equal(h.get_moved(), r.accepted)
    h.close()


# ---- every d of the (row kind, d) dispatch: theta[i] is row entry i for i < d, the rest of the row is constant ------------------
FIRST_D_CONST = np.array([0.5, -0.2, 1.0, 0.0, 1.0, 0.0, 0.4, 0.0, 0.3, 1.0, 0.0, 0.0, 4.0, 0.0, 4.0])
FIRST_D_CHAIN = 2


def case_first_d(d):
    """theta = the first d of (A11, A12, A21, A22, B1, B2, Q11, Q21): bounded priors on A11, A12 and Q21 (proposals leave the
    support at every d), a LogNormal on the variance Q11"""
    parts = [smc.TruncatedNormal(0.5, 0.3, -1.0, 1.0), smc.Uniform(-0.6, 0.2), smc.Normal(1.0, 0.1), smc.Normal(0.0, 0.1), smc.Normal(1.0, 0.1),
             smc.Normal(0.0, 0.1), smc.LogNormal(-1.0, 0.5), smc.Uniform(-0.05, 0.05)]
    tmap = smc.ThetaMap(L.MODEL_LG2D, [i if i < d else -1 for i in range(L.LG2_NRAW)], FIRST_D_CONST)
    return tmap, smc.product_distribution(parts[:d])


def _snapshot(r):
    return {name: getattr(r, name).copy() for name in ("theta", "x", "S", "logZ", "logw")}


def restate_first_d(d, M):
    """the restatement alone (no GPU), T = 6, chain 2: its cloud after the filter, after the rejuvenation, and lik of a window of 2
    steps after a permutation with repeats"""
    tmap, prior = case_first_d(d)
    r = r2.Ibis2Reference(M, tmap, prior, FIRST_D_CHAIN, 0.5, seed=7)
    out = {"r": r, "tmap": tmap, "prior": prior, "theta0": r.theta.copy()}
    y = Y[:6]
    for m in range(M):
        r.x[m], r.S[m], r.logZ[m] = r2.kalman2(r._row(r.theta[m]), y, False)
    r.logw = r.logZ.copy()
    out["filtered"] = _snapshot(r)
    chol, uni = L.host_rw_factor(r.theta) if M >= 2 else (0.1 * np.eye(d), d == 1)
    scales = 0.5 * np.arange(FIRST_D_CHAIN, 0, -1)
    out["chol"], out["s"] = chol, (scales * scales if uni else scales)
    r.rejuvenate(y, 1.0, move_seed=1234, chol=chol, s=out["s"])
    out["moved"] = _snapshot(r)
    out["a"] = a = np.array([(3 * m) % M if m % 4 else (M - 1 - m) // 2 for m in range(M)], dtype=np.int32)
    for name in ("theta", "x", "S", "logZ", "logw"):
        setattr(r, name, getattr(r, name)[a].copy())
    out["wlik"], _, _ = twin_window(r, Y[6:8], True)
    return out


def _same_arrays(h, snap):
    g = h.get(theta=True, x=True, S=True, logZ=True, logw=True)
    for name, ref in snap.items():
        assert g[name].shape == ref.shape and np.array_equal(g[name], ref), name


@pytest.mark.parametrize("M", [1, 65])
@pytest.mark.parametrize("d", range(1, 9))
def test_every_d_equals_restatement(d, M):
    """the dispatch on d for two-state rows, a lone lane and a ragged second wave: theta, x, S, logZ, logw after set_theta + filter
    and after rejuvenate (with moved and its count) are the restatement's, and a window after a permutation with repeats gives the
    twin's lik on the copied rows.  At M = 65 the restatement alone must hold accepted and rejected moves"""
    w = restate_first_d(d, M)
    r = w["r"]
    assert M == 1 or (r.n_accepted >= 1 and r.n_rejected >= 1), (r.n_accepted, r.n_rejected, r.n_out_of_support)
    fam, par = w["prior"].spec()
    h = L.IbisHandle(M, d, np.atleast_1d(fam), np.atleast_2d(par), w["tmap"].raw_from, w["tmap"].raw_const, seed=7, row_id=L.MODEL_LG2D)
    h.set_theta(w["theta0"])
    h.filter(Y[:6])
    _same_arrays(h, w["filtered"])
    n, moved = h.rejuvenate(Y[:6], 1.0, w["chol"], w["s"], 1234)
    _same_arrays(h, w["moved"])
    assert np.array_equal(moved, r.accepted) and n == int(r.accepted.sum())
    h.permute(w["a"])
    _, lik = h.window(Y[6:8], want_lik=True)
    assert np.array_equal(lik, w["wlik"])
    h.close()


@pytest.mark.parametrize("M", SIZES)
def test_permute_resample_and_get_are_value_copies(M):
    """(d) a permutation with repeats copies all of (theta, row, x [2], S [3], logZ, logw): the state afterwards, and the steps
    that follow (which read the copied rows); smc_ibis_resample draws the ancestors of smc_host_outer_resample and gathers"""
    h, r = make("ar2", M)
    h.filter(Y[:5])
    for m in range(M):
        r.x[m], r.S[m], r.logZ[m] = r2.kalman2(r._row(r.theta[m]), Y[:5], False)
    r.logw = r.logZ.copy()
    a = np.array([(3 * m) % M if m % 4 else (M - 1 - m) // 2 for m in range(M)], dtype=np.int32)
    assert M < 3 or len(set(a.tolist())) < M
    h.permute(a)
    for name in ("theta", "x", "S", "logZ", "logw"):
        setattr(r, name, getattr(r, name)[a].copy())
    same_state(h, r)
    wa = np.asarray(L.host_outer_resample(r.logw, M, 99))
    got = h.resample(99, want_a=True)
    assert np.array_equal(got, wa)
    for name in ("theta", "x", "S", "logZ", "logw"):
        setattr(r, name, getattr(r, name)[wa].copy())
    same_state(h, r)
    rec, lik = h.window(Y[5:8], want_lik=True)             # the rows were copied too: the next steps are the twin's on them
    wlik, r.x, r.S = twin_window(r, Y[5:8], True)
    assert np.array_equal(lik, wlik)
    h.commit(3)
    r.logw, r.logZ = L.host_outer_advance(r.logw, r.logZ, wlik, 3)
    same_state(h, r)
    mean, cov = h.theta_moments(weighted=True)             # a dimension-free call on a two-state handle
    wm, wc = L.host_theta_moments(r.theta, r.logw, weighted=True)
    assert np.array_equal(mean, wm) and np.array_equal(cov, wc)
    h.close()


def _ibis(M=512, seed=3, **kw):
    tmap, prior, model = r2.case_hp_one(smc)
    return smc.IBIS(M, model, prior, 3, 0.5, seed=seed, theta_map=tmap, **kw)


def _same_sampler(ib, r):
    assert np.array_equal(ib.theta, r.theta) and np.array_equal(ib.logZ, r.logZ) and np.array_equal(ib.logw, r.logw)
    assert ib.x.shape == (r.M, 2) and ib.Sigma.shape == (r.M, 2, 2) and np.array_equal(ib.x, r.x)
    S = ib.Sigma
    assert np.array_equal(S[:, 0, 0], r.S[:, 0]) and np.array_equal(S[:, 1, 0], r.S[:, 1]) and np.array_equal(S[:, 0, 1], r.S[:, 1])
    assert np.array_equal(S[:, 1, 1], r.S[:, 2])
    assert ib.ess == r.ess and ib.acc_ratio == r.acc_ratio and np.array_equal(ib.accepted, r.accepted) and ib.n_rejuvenations == r.n_rejuvenations


@pytest.mark.parametrize("window", [1, 16])
def test_online_run_equals_restatement_and_recovers_the_posterior(window):
    """(e) smc2 + smc2_run, M = 512, chain 3, threshold 0.5, the one-parameter HP case, T = 60: the final ESS, theta, logZ, x, S,
    logw bit for bit with at least one rejuvenation (window 1 and 16: the same bits), and the weighted posterior mean of theta within 4 posterior-sd / sqrt(ess) +
    the restatement's K-seed standard error of the grid quadrature of the exact posterior"""
    tmap, prior, _ = r2.case_hp_one(smc)
    r = r2.Ibis2Reference(512, tmap, prior, 3, 0.5, seed=3).run(Y)
    assert r.n_rejuvenations >= 1 and r.n_accepted >= 1 and r.n_out_of_support >= 1
    ib = _ibis()
    smc.smc2(ib, Y)
    smc.smc2_run(ib, Y, 2, len(Y), window=window, verbose=False)
    assert ib.t == len(Y)
    _same_sampler(ib, r)
    est, want = smc.expected_parameters(ib)[0], r.expected_parameters()[0]
    assert est == want
    mean, sd = r2.grid_posterior_q(Y)
    pm, pc = smc.posterior_moments(ib)
    print("E[theta] = %.6f, grid %.6f (sd %.6f), ess %.1f" % (est, mean, sd, ib.ess))
    assert abs(est - mean) <= 4.0 * sd / np.sqrt(ib.ess) + SE_K_SEEDS
    assert abs(pm[0] - est) <= 1e-12 and pc.shape == (1, 1)
    ib.close()


def test_step_by_step_ess_trace():
    """(e) smc2 + smc2_step: the ESS of every step is the restatement's"""
    tmap, prior, _ = r2.case_hp_one(smc)
    r = r2.Ibis2Reference(512, tmap, prior, 3, 0.5, seed=3).run(Y)
    ib = _ibis()
    smc.smc2(ib, Y)
    ess = [ib.ess]
    for t in range(2, len(Y) + 1):
        smc.smc2_step(ib, Y, t, verbose=False)
        ess.append(ib.ess)
    assert ess == r.ess_trace
    _same_sampler(ib, r)
    ib.close()


def test_density_tempered_equals_restatement():
    """(e) density_tempered: the xi ladder, the ESS of every stage and the final cloud, with at least one rejuvenation"""
    tmap, prior, _ = r2.case_hp_one(smc)
    r = r2.Ibis2Reference(512, tmap, prior, 3, 0.5, seed=3)
    ladder = r.density_tempered(Y)
    assert r.n_rejuvenations >= 1 and r.n_accepted >= 1
    ib = _ibis()
    stages = smc.density_tempered(ib, Y, verbose=False)
    assert stages == ladder
    _same_sampler(ib, r)
    assert np.array_equal(smc.expected_parameters(ib), r.expected_parameters())
    mean, sd = r2.grid_posterior_q(Y)
    assert abs(smc.expected_parameters(ib)[0] - mean) <= 4.0 * sd / np.sqrt(ib.ess) + SE_K_SEEDS
    ib.close()


def test_device_moves_same_walk_and_ancestors_up_to_the_first_rejuvenation():
    """(e) device_moves=True: the ESS walk and the ancestors of the first resample! are those of the default path (the same
    integer functions); after the first rejuvenation the two paths differ by the rounding of the covariance only"""
    tmap, prior, _ = r2.case_hp_one(smc)
    r = r2.Ibis2Reference(512, tmap, prior, 3, 0.5, seed=3)
    r.smc2(Y)
    t = 1
    while r.ess >= r.ess_min:
        t += 1
        r._propagate(float(Y[t - 1]), True)
    ib = _ibis(device_moves=True)
    smc.smc2(ib, Y)
    smc.smc2_run(ib, Y, 2, t, window=16, verbose=False)
    assert ib.t == t and ib.ess == r.ess and ib.n_rejuvenations == 0
    assert np.array_equal(ib.logw, r.logw) and np.array_equal(ib.logZ, r.logZ) and np.array_equal(ib.x, r.x)
    a = r.resample()
    got = ib._handle().resample(ib._next_seed(), want_a=True)
    assert np.array_equal(got, a) and np.array_equal(ib.theta, r.theta) and np.array_equal(ib.x, r.x)
    smc.rejuvenate_(ib, Y[:t])                               # the fused launch from the device's covariance
    assert ib.n_rejuvenations == 1 and 0.0 < ib.acc_ratio <= 1.0 and np.all(ib.logw == 0.0)
    assert int(ib.accepted.sum()) == round(ib.acc_ratio * ib.M)
    ib.close()


def test_refusals_leave_the_handle_unchanged_next_to_a_scalar_handle():
    """(f) every refusal of a two-state handle is SMC_EINVAL with a message naming what is missing, and a following window gives
    the bits it gave before; a scalar handle interleaved with it in the same process gives its own results"""
    lib = L.lib()
    h, r = make("ar2", 130)
    tmap1, prior1, _ = case_readme(smc)
    fam, par = prior1.spec()
    th1 = np.ascontiguousarray(prior1.rand_many(np.random.default_rng(2), 130), dtype=np.float64)

    def scalar():
        s = L.IbisHandle(130, 3, np.atleast_1d(fam), np.atleast_2d(par), tmap1.raw_from, tmap1.raw_const, seed=2)
        s.set_theta(th1)
        return s

    alone = scalar()                                        # the scalar results with no two-state call in between
    rec_a, lik_a = alone.window(Y[:6], want_lik=True)
    alone.commit(6)
    st_a = alone.get(x=True, S=True, logZ=True, logw=True)
    alone.close()

    s = scalar()
    rec0, lik0 = h.window(Y[:4], want_lik=True)
    rec_s, lik_s = s.window(Y[:6], want_lik=True)
    y, out8, which, paths = Y[:4].copy(), np.zeros((4, 8)), np.zeros(2, dtype=np.int32), np.zeros((4, 2))
    refused = [
        (lambda: lib.smc_ibis_set_flags(h._h, L.FLAG_NAN_MISSING), "SMC_FLAG_NAN_MISSING"),
        (lambda: lib.smc_ibis_summary(h._h, 0, L._d(out8)), "summary"),
        (lambda: lib.smc_ibis_set_summaries(h._h, 1, 0), "summary"),
        (lambda: lib.smc_ibis_get_summaries(h._h, 0, L._d(out8)), "summary"),
        (lambda: lib.smc_ibis_smooth(h._h, L._d(y), 4, L._d(out8), None, None), "RTS smoother"),
        (lambda: lib.smc_ibis_sample_paths(h._h, L._d(y), 4, 2, 5, which.ctypes.data_as(L._i32p), L._d(paths)), "paths"),
    ]
    for call, word in refused:
        assert call() == -1
        msg = lib.smc_last_error().decode()
        assert word in msg and "two-state" in msg, msg
    assert h.flags == 0
    h.commit(4)                                             # the window that was pending is still pending
    s.commit(6)
    rec1, lik1 = h.window(Y[:4], want_lik=True)             # ... and the same window from the start gives the same bits
    h2, _ = make("ar2", 130)
    rec2, lik2 = h2.window(Y[:4], want_lik=True)
    assert np.array_equal(rec0, rec2) and np.array_equal(lik0, lik2)
    h2.commit(4)
    rec3, lik3 = h2.window(Y[:4], want_lik=True)
    assert np.array_equal(rec1, rec3) and np.array_equal(lik1, lik3)
    st_s = s.get(x=True, S=True, logZ=True, logw=True)
    assert np.array_equal(rec_s, rec_a) and np.array_equal(lik_s, lik_a)
    for name in st_a:
        assert st_s[name].shape == (130,) and np.array_equal(st_s[name], st_a[name]), name
    wlik, _, _ = twin_window(r, Y[:4], False)
    assert np.array_equal(lik0, wlik)
    for x in (h, h2, s):
        x.close()
