"""The guided particle filter on the GPU (pytest -m gpu): smc_set_proposal on every launch path.

  * the device twin of the guided step equals the host twin bit for bit
  * LG1D AFFINE (0, A, 0, Q) IS the bootstrap filter, bit for bit, on every path (which ties the guided kernels to the oracle
    that pins the bootstrap ones)
  * the paths agree among themselves for real proposals; summaries in both modes
  * a one-step audit of draw and weights from (x_old, ancestors, x_new, w_new) against tests/guided_reference.py
  * Kalman / bootstrap pins of logZ: unbiased, and the variance the proposal is for
  * handle state: recycling, smc_set_params, slot moves; the samplers with HipBackend(proposal=...)
"""
import numpy as np
import pytest

import guided_reference as G
import step_edge_inputs

pytestmark = pytest.mark.gpu

LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
UC = [0.2, 0.2, 3.0, 0.0, 0.0]
RAW = {1: LG, 3: UC}
NONE, AFFINE, OPTIMAL = 0, 1, 2
POOR = [0.3, 0.2, 0.1, 2.0]
NO_RESIDENT, SYSTEMATIC = 2, 4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def raws_for(model, nth):
    r = np.tile(RAW[model], (nth, 1)).astype(float)
    r[:, 0] *= 1.0 - 0.3 * np.arange(nth) / max(nth, 1)
    if model == 1:
        r[:, 2] *= 1.0 + 0.1 * np.arange(nth)
    return r


def series(model, T, seed=1998):
    from sequential_monte_carlo_amd import _lib as L
    return L.simulate(model, RAW[model], T, seed)[1]


def identity_rows(raw):
    return np.stack([np.zeros(len(raw)), raw[:, 0], np.zeros(len(raw)), raw[:, 2]], axis=1)


def snapshot(h):
    x, w, a = h.state()
    z, e = h.logZ()
    return (x, w, a) + tuple(h.weights_raw()) + (z, e)


def assert_same_snapshot(a, b, ctx):
    for k, (u, v) in enumerate(zip(a, b)):
        if u.dtype == np.float64:
            assert same(u, v), ctx + (k,)
        else:
            assert np.array_equal(u, v), ctx + (k,)


# launch paths: name -> (n, seg, flags, how the series is run, skip mask or None)
PATHS = {
    "resident": (1024, 0, 0, "ll", None),
    "resident-ragged": (1000, 0, 0, "ll", None),
    "no-resident": (1024, 0, NO_RESIDENT, "ll", None),
    "step-api": (1024, 0, 0, "step", None),
    "window": (1024, 0, 0, "win", None),
    "multi-seg256": (3000, 256, 0, "ll", None),
    "multi-seg256-step": (3000, 256, 0, "step", None),
    "two-records": (40000, 256, 0, "ll", None),
    "systematic": (1024, 0, SYSTEMATIC, "ll", None),
    "systematic-multi": (5000, 1024, SYSTEMATIC, "ll", None),
    "skip": (1024, 0, 0, "ll", [0, 1, 0]),
    "skip-multi": (3000, 256, 0, "ll", [1, 0, 0]),
    "above-2^20": ((1 << 20) + 4096, 0, 0, "ll", None),
}


def run(L, model, path, kind, rows, seed=7, T=12, nth=3):
    """one series on one path: (logmu trace, ess trace, snapshot)"""
    n, seg, flags, how, skip = PATHS[path]
    if n > (1 << 20):
        nth, T = 1, 4
        skip = None
    y = series(model, T)
    h = L.Handle(model, nth, n, seg=seg, seed=seed, flags=flags | L.FLAG_ANCESTORS)
    raw = raws_for(model, nth)
    h.set_params(raw)
    if kind != NONE:
        h.set_proposal(kind, rows(raw) if callable(rows) else rows)
    if how == "ll":
        if skip is not None:
            h.init(y[0])                       # the skipped filters keep this state
            h.set_skip(skip)
        _, lm, es = h.log_likelihood(y, trace=True)
    elif how == "step":
        lm, es = np.zeros((T, nth)), np.zeros((T, nth))
        lm[0] = h.init(y[0])
        _, es[0] = h.logZ()
        for t in range(1, T):
            lm[t], es[t] = h.step(y[t])
    else:                                      # windows of 5 of which 3 are kept (j < k), then the rest
        lm, es = np.zeros((T, nth)), np.zeros((T, nth))
        lm[0] = h.init(y[0])
        _, es[0] = h.logZ()
        t = 1
        while t < T:
            k = min(5, T - t)
            j = 3 if k == 5 else k
            wl, we = h.step_window(y[t:t + k])
            h.step_commit(j)
            lm[t:t + j], es[t:t + j] = wl[:j], we[:j]
            t += j
    out = (lm, es, snapshot(h))
    h.close()
    return out


# ---- 4. device twin == host twin ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model,kind", [(1, AFFINE), (1, OPTIMAL), (3, OPTIMAL)])
def test_device_guided_step_equals_host(L, model, kind):
    raw, par, xp, z, y = step_edge_inputs.guided(model, kind)
    x, lw = L.device_guided_step(model, raw, kind, par, xp, z, y)
    for i in range(xp.shape[1]):
        hx, hl = L.host_guided_step(model, raw, kind, par, xp[:, i], z[:, i], y)
        assert same(x[:, i], hx) and same([lw[i]], [hl]), (i, x[:, i], hx, lw[i], hl)


# ---- 5. identity: AFFINE (0, A, 0, Q) is the bootstrap filter ------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_identity_row_is_the_bootstrap_filter(L, path):
    """x, w, ancestors, the raw fixed-point weights, logZ, ess and the logmu / ess traces.  The mean of the proposal is
    fma(A, xp, -0.0): the rounded product A xp with its sign of zero, so the draw is the transition's for every operand
    (tests/test_guided_host.py::test_affine_identity_on_the_host checks the signed zeros one by one)."""
    a = run(L, 1, path, NONE, None)
    b = run(L, 1, path, AFFINE, identity_rows)
    assert same(a[0], b[0]) and same(a[1], b[1]), (path, "traces")
    assert_same_snapshot(a[2], b[2], (path,))


# ---- 6. the paths agree among themselves ---------------------------------------------------------------------------------
PROPOSALS = {"lg-optimal": (1, OPTIMAL, None), "lg-poor": (1, AFFINE, lambda raw: np.tile(POOR, (len(raw), 1))), "ucsv-optimal": (3, OPTIMAL, None)}
GROUPS = {   # the same geometry, law and seed on different launch paths
    "one-segment": ("resident", "no-resident", "step-api", "window"),
    "multi-segment": ("multi-seg256", "multi-seg256-step"),
}


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("prop", list(PROPOSALS))
def test_paths_agree(L, prop, group):
    model, kind, rows = PROPOSALS[prop]
    ref = None
    for path in GROUPS[group]:
        out = run(L, model, path, kind, rows)
        if ref is None:
            ref = out
            boot = run(L, model, path, NONE, None)
            assert not same(boot[0], out[0]), "the proposal changes the filter"
            continue
        assert same(ref[0], out[0]), (prop, path, "logmu")
        assert same(ref[1][-1], out[1][-1]), (prop, path, "last ess")
        assert_same_snapshot(ref[2], out[2], (prop, path))


@pytest.mark.parametrize("prop", list(PROPOSALS))
def test_every_other_path_runs_guided(L, prop):
    """ragged, two records per thread, systematic, skip masks and a filter above 2^20: finite logZ that differs from the
    bootstrap filter's; skipped filters are not run"""
    model, kind, rows = PROPOSALS[prop]
    for path in ("resident-ragged", "two-records", "systematic", "systematic-multi", "skip", "skip-multi", "above-2^20"):
        g = run(L, model, path, kind, rows)
        b = run(L, model, path, NONE, None)
        z = g[2][-2]
        skip = PATHS[path][4]
        for th in range(len(z)):
            if skip is not None and skip[th] and path in ("skip", "skip-multi"):
                assert z[th] == -np.inf, (prop, path, th)
                assert same(g[2][0][:, th], b[2][0][:, th]), (prop, path, th, "a skipped filter keeps its state")
            else:
                assert np.isfinite(z[th]) and z[th] != b[2][-2][th], (prop, path, th, z[th])
                assert abs(z[th] - b[2][-2][th]) < 3.0, (prop, path, th, z[th], b[2][-2][th])


@pytest.mark.parametrize("mode", ["weighted", "unweighted"])
@pytest.mark.parametrize("prop", list(PROPOSALS))
def test_summaries_of_guided_filters(L, prop, mode):
    """per-step summaries (resident SUMM kernels, the window, one launch per step) are recorded for guided filters and their last
    row equals the stand-alone quantiles / moments of the state the call leaves"""
    model, kind, rows = PROPOSALS[prop]
    p = [0.1, 0.5, 0.9]
    y = series(model, 10)
    outs = []
    for flags, how in ((0, "ll"), (NO_RESIDENT, "ll"), (0, "win")):
        h = L.Handle(model, 3, 1024, seed=11, flags=flags)
        raw = raws_for(model, 3)
        h.set_params(raw)
        h.set_proposal(kind, rows(raw) if callable(rows) else rows)
        h.set_summary_mode(mode)
        h.set_summaries(p, 0, True)
        if how == "ll":
            z = h.log_likelihood(y)
            q, mean, var = h.get_summaries(len(y))
        else:
            h.init(y[0])
            h.step_window(y[1:])
            q, mean, var = h.get_summaries(len(y) - 1)
            h.step_commit(len(y) - 1)
            z, _ = h.logZ()
        h.set_summaries()
        assert same(q[-1], h.quantiles(p, 0)), (prop, mode, flags, how)
        m1, v1 = h.moments()
        assert same(mean[-1], m1) and same(var[-1], v1), (prop, mode, flags, how)
        outs.append((z, q[-1], mean[-1], var[-1]))
        h.close()
    for o in outs[1:]:
        for u, v in zip(outs[0], o):
            assert same(u, v), (prop, mode)
    plain = run(L, model, "resident", kind, rows, seed=11, T=10)
    assert same(plain[2][-2], outs[0][0]), "summaries do not change the filter"


# ---- 7. one-step audit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prop", list(PROPOSALS))
def test_one_step_audit(L, prop):
    """(x_old, ancestors, x_new, w_new) around one guided smc_step, N = 2^16; needs no knowledge of the random numbers.
    Weights: with l_i the reference's log-weight at (x_old[a_i], x_new_i, y), u_i = exp(l_i - max l) and w_i = u_i / sum u, the
    device's integer weight of particle i is rint(p 2^(48 + k - kb)) with exp(l) = p 2^k, p in [0.707, 1.415]: a relative error
    eps_i (the bound of the step's log-weight from guided_reference, plus 4u for sp_exp and the scaling) and an absolute quantum
    of 2^-47 of its segment's largest weight; the segment table of a filter of 2^16 particles shifts by two more bits and
    floors (x 2^3): eta = 2^-44 relative to the largest weight.  Hence
        |w_dev_i - w_i| <= 2 w_i (eps_max + N eta / sum u) + 2 eta / sum u + 4 u w_i.
    Draw: (x_new - m) / sqrt(s2) has mean and variance within 5 standard errors of 0 and 1 (sd of the mean 1/sqrt(N), of the
    variance sqrt(2/N))."""
    model, kind, rows = PROPOSALS[prop]
    N = 1 << 16
    y = series(model, 3)
    raw = np.asarray(RAW[model], dtype=float)
    h = L.Handle(model, 1, N, seed=23, flags=L.FLAG_ANCESTORS)
    h.set_params(raw[None, :])
    h.set_proposal(kind, np.asarray([POOR]) if kind == AFFINE else None)
    h.init(y[0])
    h.step(y[1])
    x_old, _, _ = h.state()
    h.step(y[2])
    x_new, w_new, anc = h.state()
    h.close()
    xp = x_old[:, 0, :][:, anc[0]]
    xn = x_new[:, 0, :]
    if model == 1:
        par = POOR if kind == AFFINE else L.host_optimal_proposal(1, raw)
        lw = G.lg_logw(raw, par, xp[0], xn[0], y[2])
        m, s = G.lg_mean(par, xp[0], y[2]), np.sqrt(G.LD(par[3]))
        zhat = ((G.ld(xn[0]) - m) / s).astype(float)
        _, blw = G.lg_bounds(raw, par, xp[0], zhat, y[2], xn[0])
    else:
        Q, R = np.exp(G.ld(xp[1])), np.exp(G.ld(xn[2]))
        K = Q / (Q + R)
        _, lw = G.ucsv_draw_logw(xp, 0.0, y[2], xn[2])
        zhat = ((G.ld(xn[0]) - (G.ld(xp[0]) + K * (G.ld(y[2]) - G.ld(xp[0])))) / np.sqrt(K * R)).astype(float)
        _, blw = G.ucsv_bounds(raw, xp, np.stack([zhat, zhat, zhat]), y[2], xn)
        for c, g in ((1, raw[0]), (2, raw[1])):             # the volatilities moved by the transition
            zc = (xn[c] - xp[c]) / g
            assert abs(zc.mean()) <= 5 / np.sqrt(N) and abs(zc.var() - 1) <= 5 * np.sqrt(2.0 / N), (prop, c)
    u = np.exp(lw - lw.max())
    su = float(u.sum())
    w_ref = (u / su).astype(float)
    eps = float(np.max(blw)) + 4 * G.U
    eta = 2.0 ** -44
    bound = 2 * w_ref * (eps + N * eta / su) + 2 * eta / su + 4 * G.U * w_ref
    err = np.abs(w_new[0] - w_ref)
    print("one-step audit %s: max |w - ref| / bound = %.3g, max |w - ref| = %.3g" % (prop, float(np.max(err / bound)), float(err.max())))
    assert np.all(err <= bound), (prop, float(np.max(err / bound)))
    assert abs(zhat.mean()) <= 5 / np.sqrt(N), (prop, zhat.mean())
    assert abs(zhat.var() - 1) <= 5 * np.sqrt(2.0 / N), (prop, zhat.var())


# ---- 8. Kalman pin ------------------------------------------------------------------------------------------------------
LG_ROWS = {"readme": [0.5, 1.0, 0.9, 0.8, 0.0, 1.0], "local-level": [1.0, 1.0, 0.5, 0.05, 0.0, 1.0], "sharp": [0.9, 1.0, 1.0, 0.1, 0.0, 1.0]}


def many_logZ(L, model, raw, y, K, N, kind, par=None, seed=5):
    h = L.Handle(model, K, N, seed=seed)
    h.set_params(np.tile(raw, (K, 1)))
    h.set_streams(np.arange(K, dtype=np.uint32))
    if kind != NONE:
        h.set_proposal(kind, None if par is None else np.tile(par, (K, 1)))
    z = h.log_likelihood(y)
    h.close()
    return z


def unbiased_within(z, c, nse=5.0):
    r = np.exp(z - c)
    return abs(r.mean() - 1.0) <= nse * r.std(ddof=1) / np.sqrt(len(r)), r.mean(), r.std(ddof=1) / np.sqrt(len(r))


@pytest.mark.parametrize("name", list(LG_ROWS))
def test_kalman_pin_lg_optimal(L, name):
    """K = 512 filters of N = 256, T = 100: var(logZ) <= 0.25, mean(exp(logZ - logZ_KF)) within 5 standard errors of 1, and a third
    of the bootstrap filter's variance at most; a poor AFFINE row is unbiased too (N = 4096).
    The poor row here is (0.3, 0.8 A, 0.1, 2.0): shifted, shrunk, hardly looking at y, with 2 to 40 times the optimal variance -
    but tied to A.  An importance sampler is only usable when the proposal covers transition x likelihood: the fixed row
    (0.3, 0.2, 0.1, 2.0) of the path tests puts its mean 0.8 |xp| / sqrt(2) proposal standard deviations from the transition's
    on the local-level model (A = 1), whose state walks to |xp| ~ 10 within T = 100; its weights then have no usable variance
    (measured there: mean(exp(logZ - logZ_KF)) = 2e-43), which says nothing about the arithmetic."""
    from oracle import kalman
    raw = LG_ROWS[name]
    _, y = L.simulate(1, raw, 100, 2024)
    kf = kalman.log_likelihood(y, *raw[:4], x0=raw[4], sigma0=raw[5])[2]
    zg = many_logZ(L, 1, raw, y, 512, 256, OPTIMAL)
    zb = many_logZ(L, 1, raw, y, 512, 256, NONE)
    vg, vb = zg.var(ddof=1), zb.var(ddof=1)
    ok, mean, se = unbiased_within(zg, kf)
    print("kalman pin %s: var guided %.4f, var bootstrap %.4f, mean ratio %.4f +- %.4f" % (name, vg, vb, mean, se))
    assert vg <= 0.25, (name, vg)
    assert ok, (name, mean, se)
    assert vg <= vb / 3.0, (name, vg, vb)
    zp = many_logZ(L, 1, raw, y, 512, 4096, AFFINE, [0.3, 0.8 * raw[0], 0.1, 2.0])
    ok, mean, se = unbiased_within(zp, kf)
    print("kalman pin %s, poor row: var %.4f, mean ratio %.4f +- %.4f" % (name, zp.var(ddof=1), mean, se))
    assert ok, (name, "poor row", mean, se)


# ---- 9. UCSV pin --------------------------------------------------------------------------------------------------------
def test_ucsv_pin_against_bootstrap(L):
    """128 guided filters of N = 1024 against 128 bootstrap filters of N = 8192 (the pinned path), UCSV gamma = (0.2, 0.2), x0 = 0,
    log sigma0 = (-1, -2), T = 50: both variances of logZ below 0.5, the means of exp(logZ - c) within 5 combined standard errors."""
    raw = [0.2, 0.2, 0.0, -1.0, -2.0]
    _, y = L.simulate(3, raw, 50, 77)
    zg = many_logZ(L, 3, raw, y, 128, 1024, OPTIMAL)
    zb = many_logZ(L, 3, raw, y, 128, 8192, NONE)
    vg, vb = zg.var(ddof=1), zb.var(ddof=1)
    c = zb.mean()
    rg, rb = np.exp(zg - c), np.exp(zb - c)
    se = np.sqrt(rg.var(ddof=1) / len(rg) + rb.var(ddof=1) / len(rb))
    print("ucsv pin: var guided(1024) %.4f, var bootstrap(8192) %.4f, means %.4f %.4f, combined se %.4f" % (vg, vb, rg.mean(), rb.mean(), se))
    assert vg < 0.5 and vb < 0.5, (vg, vb)
    assert abs(rg.mean() - rb.mean()) <= 5 * se, (rg.mean(), rb.mean(), se)


# ---- 10. state management -------------------------------------------------------------------------------------------------
def test_recycled_handle_is_a_bootstrap_handle(L):
    y = series(1, 8)
    raw = raws_for(1, 3)

    def fresh(guided):
        h = L.Handle(1, 3, 1024, seed=31)
        h.set_params(raw)
        if guided:
            h.set_proposal(OPTIMAL)
        z = h.log_likelihood(y)
        x, w, _ = h.state(want_anc=False)
        h.close()
        return z, x, w
    never = fresh(False)
    guided = fresh(True)                # destroyed: its buffers go to the cache
    again = fresh(False)                # same geometry: a recycled bundle
    assert not same(never[0], guided[0])
    for u, v in zip(never, again):
        assert same(u, v)


def test_set_params_rederives_the_optimal_proposal(L):
    y = series(1, 8)
    r1, r2 = raws_for(1, 2), raws_for(1, 2) * np.array([0.9, 1.0, 1.4, 0.7, 1.0, 1.0])
    h = L.Handle(1, 2, 1024, seed=41)
    h.set_params(r1)
    h.set_proposal(OPTIMAL)
    h.log_likelihood(y)
    h.set_params(r2)
    z = h.log_likelihood(y)
    h.close()
    g = L.Handle(1, 2, 1024, seed=41)
    g.set_params(r2)
    g.set_proposal(AFFINE, np.stack([L.host_optimal_proposal(1, r) for r in r2]))     # the same four doubles: the same bits
    z2 = g.log_likelihood(y)
    g.set_proposal(NONE)
    z3 = g.log_likelihood(y)
    g.close()
    assert same(z, z2) and not same(z, z3)


def test_refused_proposals_leave_the_handle_unchanged(L):
    y = series(1, 8)
    h = L.Handle(1, 2, 1024, seed=43)
    h.set_params(raws_for(1, 2))
    h.set_proposal(OPTIMAL)
    z = h.log_likelihood(y)
    for kind, par in ((3, None), (AFFINE, None), (OPTIMAL, np.tile(POOR, (2, 1))), (AFFINE, np.array([POOR, [0, 1, 0, -1.0]])),
                      (AFFINE, np.array([POOR, [0, np.nan, 0, 1.0]]))):
        with pytest.raises(L.SmcError):
            h.set_proposal(kind, par)
    assert same(z, h.log_likelihood(y))
    h.close()
    for model, kind, par in ((2, OPTIMAL, None), (2, AFFINE, POOR), (3, AFFINE, POOR)):
        s = L.Handle(model, 1, 1024, seed=1)
        with pytest.raises(L.SmcError):
            s.set_proposal(kind, None if par is None else np.asarray([par]))
        s.close()


def test_proposal_stays_with_its_slot(L):
    """smc_permute and pack / unpack move the state; parameters, stream ids and proposals stay with the slot"""
    import torch
    y = series(1, 10)
    raw = raws_for(1, 3)
    rows = np.array([POOR, [0.0, 0.4, 0.3, 0.7], [0.1, 0.1, 0.5, 1.1]])
    perm = np.array([2, 0, 0], dtype=np.int32)

    def start():
        h = L.Handle(1, 3, 1024, seed=51)
        h.set_params(raw)
        h.set_proposal(AFFINE, rows)
        h.init(y[0])
        for t in range(1, 5):
            h.step(y[t])
        return h
    a = start()
    a.permute(perm)
    b = start()
    buf = torch.empty((3, b.slot_bytes() // 8), dtype=torch.int64, device="cuda")
    b.pack_slots(perm, buf.data_ptr())
    b.unpack_slots(np.arange(3, dtype=np.int32), buf.data_ptr())
    outs = []
    for h in (a, b):
        for t in range(5, 10):
            h.step(y[t])
        outs.append(snapshot(h))
        h.close()
    # an expectation that uses no slot move: slot 1 receives the state of slot 0.  A handle whose slot 1 is a copy of slot 0 from
    # the start (its row, proposal and stream id) and becomes slot 1 proper (row 1, proposal 1, stream 1) after step 4
    e = L.Handle(1, 3, 1024, seed=51)
    e.set_params(raw[[0, 0, 2]])
    e.set_proposal(AFFINE, rows[[0, 0, 2]])
    e.set_streams(np.array([0, 0, 2], dtype=np.uint32))
    e.init(y[0])
    for t in range(1, 5):
        e.step(y[t])
    e.set_params(raw)
    e.set_proposal(AFFINE, rows)
    e.set_streams(np.arange(3, dtype=np.uint32))
    for t in range(5, 10):
        e.step(y[t])
    xe, we, _ = e.state(want_anc=False)
    e.close()
    for o in outs:
        assert same(o[0][:, 1], xe[:, 1]) and same(o[1][1], we[1])
    assert_same_snapshot(outs[0][:2], outs[1][:2], ("permute == pack/unpack",))
    # and it is the proposal of the DESTINATION slot that ran: with the rows permuted too the result differs
    c = start()
    c.permute(perm)
    c.set_proposal(AFFINE, rows[perm])
    for t in range(5, 10):
        c.step(y[t])
    assert not same(c.state(want_anc=False)[0][:, 0], outs[0][0][:, 0])
    c.close()


# ---- 11. samplers ---------------------------------------------------------------------------------------------------------
def test_samplers_with_guided_inner_filters(L):
    """density_tempered and smc2 + smc2_run with HipBackend(proposal=OptimalProposal()) and a ThetaMap (device PMMH).  For three
    parameter particles a stand-alone guided log_likelihood with the particle's theta, one of the stream ids and one of the seeds
    the sampler issued reproduces its logZ bit for bit, and the bootstrap filter with the same seeds does not.
    Posterior mean of (A, Q, R), density_tempered M = 32, T = 25: guided N = 128 against five bootstrap N = 1024 runs (seeds 1..5),
    inside [min - spread, max + spread] of the five.  Measured on an MI355X: bootstrap min (0.0997, 0.5623, 0.6238), max
    (0.3972, 0.7483, 0.9767); guided (0.1719, 0.8115, 0.7827)."""
    import sequential_monte_carlo_amd as smc
    from sequential_monte_carlo_amd.smc_samplers import HipBackend
    from test_samplers_cpu import LG as LGK, lg_mod, run_dt, run_online
    _, y = smc.simulate(smc.UnivariateLinearGaussian(**LGK), 25, seed=1998)
    s, stages, _ = run_dt(device=True, backend=HipBackend(proposal=smc.OptimalProposal()))
    assert stages[-1][0] == 1.0

    def reproduces(s, y, m, proposal):
        # the stream id is the slot the filter ran in, which resampling may have left behind: every slot, every seed issued
        for c in range(1, s._calls + 1):
            _, _, z = smc.log_likelihood(s.N, y, [lg_mod(s.theta[m])] * s.M, seed=(s.seed << 20) + c, streams=np.arange(s.M),
                                         proposal=proposal)
            if np.any(bits(z) == bits([s.logZ[m]])[0]):
                return True
        return False
    for m in (0, 7, 19):
        assert reproduces(s, y, m, smc.OptimalProposal()), m
        assert not reproduces(s, y, m, None), m
    _, y30 = smc.simulate(smc.UnivariateLinearGaussian(**LGK), 30, seed=1998)
    o, moves, x, w = run_online(device=True, window=8, backend=HipBackend(proposal=smc.OptimalProposal()))
    ob_, _, xb, _ = run_online(device=True, window=8)
    assert moves >= 1 and np.all(np.isfinite(o.logZ)) and not same(x, xb)
    o1, _, x1, w1 = run_online(device=True, window=0, backend=HipBackend(proposal=smc.OptimalProposal()))
    assert same(x, x1) and same(w, w1) and same(o.theta, o1.theta)      # windows == the step loop, guided as bootstrap
    means = []
    for seed in range(1, 6):
        b, _, _ = run_dt(N=1024, seed=seed, device=True)
        means.append(smc.expected_parameters(b))
    means = np.array(means)
    g, _, _ = run_dt(N=128, seed=1, device=True, backend=HipBackend(proposal=smc.OptimalProposal()))
    gm = np.asarray(smc.expected_parameters(g))
    lo, hi = means.min(axis=0), means.max(axis=0)
    spread = hi - lo
    print("posterior means: bootstrap N=1024 min %s max %s; guided N=128 %s" % (lo, hi, gm))
    assert np.all(gm >= lo - spread) and np.all(gm <= hi + spread), (gm, lo, hi)
