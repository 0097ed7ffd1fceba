"""The FFBS particle smoother on the GPU (pytest -m gpu): the record of a step-by-step run and smc_smooth over it.

  * smc_history_get == smc_get_state after every step, bit for bit
  * smc_smooth's weights == smc_host_smooth on the recorded clouds, bit for bit (the host twin is pinned to a long-double
    recursion by tests/test_smoother_host.py): bootstrap and guided filters, both resamplers, ragged and multi-segment shapes
  * a filter alone == the same filter inside a batch; two runs agree
  * moments against exact sums; the Rauch-Tung-Striebel pin on the device
  * every refusal and state rule of include/smc_hip.h; the Python layer (smoother, smoothed_state)
"""
import numpy as np
import pytest

import smoother_reference as R

pytestmark = pytest.mark.gpu

LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
LG_SHARP = [0.5, 1.0, 0.9, 1e-4, 0.0, 1.0]
SV = [-1.0, 0.95, 0.3]
UC = [0.2, 0.3, 1.0, -1.0, -0.5]
RAW = {1: LG, 2: SV, 3: UC}
NONE, OPTIMAL = 0, 2
SYSTEMATIC = 4
MEAN_REL, MEAN_SD, VAR_REL, VAR_LEVEL = 1e-11, 1e-12, 1e-9, 1e-11   # the bounds of smc_get_moments


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def rows_for(raw, nth):
    """nth distinct parameter rows around raw (the transition scales differ)"""
    r = np.tile(np.asarray(raw, dtype=float), (nth, 1))
    k = 2 if len(raw) != 5 else 0
    r[:, k] *= 1.0 + 0.15 * np.arange(nth)
    return r


def run_recorded(L, model, rows, n, seg, T, proposal=NONE, flags=0, seed=11, streams=None, check_state=False):
    """a handle after T recorded steps of the step API; with check_state the record is compared with smc_get_state on the way"""
    rows = np.atleast_2d(rows)
    h = L.Handle(model, rows.shape[0], n, seg=seg, seed=seed, flags=flags)
    h.set_params(rows)
    if streams is not None:
        h.set_streams(streams)
    if proposal != NONE:
        h.set_proposal(proposal)
    _, y = L.simulate(model, RAW[model], max(T, 2), 1998)
    h.history_begin(T)
    states = []
    for t in range(T):
        h.init(float(y[0])) if t == 0 else h.step(float(y[t]))
        if check_state:
            x, w, _ = h.state(want_anc=False)
            states.append((x, w))
    assert h.history_len() == T
    for t, (x, w) in enumerate(states):
        hx, hw = h.history_get(t)
        assert same(hx, x) and same(hw, w), t
    return h


def clouds(h):
    T = h.history_len()
    xs, ws = zip(*[h.history_get(t) for t in range(T)])
    return np.array(xs), np.array(ws)      # [T][d][ntheta][n], [T][ntheta][n]


def compare_with_host(L, h, model, rows):
    x, w = clouds(h)
    ws, mean, var = h.smooth()
    rows = np.atleast_2d(rows)
    for m in range(rows.shape[0]):
        hs, hm, hv = L.host_smooth(model, rows[m], x[:, :, m, :], w[:, m, :])
        assert same(ws[:, m], hs), ("weights", m)
        assert np.all(np.isfinite(ws[:, m]))
        for t in range(x.shape[0]):
            for r in range(x.shape[1]):
                em, ev = R.exact_moments(x[t, r, m], ws[t, m])
                assert abs(mean[t, r, m] - em) <= MEAN_REL * abs(em) + MEAN_SD * np.sqrt(ev), (t, r, m)
                assert var[t, r, m] >= 0 and abs(var[t, r, m] - ev) <= VAR_REL * ev + (VAR_LEVEL * em) ** 2, (t, r, m)
    return x, w, ws


# (model, row, proposal, flags, n, seg, n_theta, T): the smallest shapes that can go wrong - one particle, a partial chunk (65),
# two segments with padding (300 / 256), several segments with a partial chunk and a partial tile (1300 / 256), whole tiles (1024)
CASES = [
    (1, LG, NONE, 0, 1, 0, 3, 12),
    (1, LG, NONE, 0, 65, 0, 3, 12),
    (1, LG, NONE, 0, 300, 256, 3, 12),
    (1, LG, NONE, 0, 1300, 256, 3, 12),
    (1, LG, NONE, 0, 1024, 0, 1, 12),
    (1, LG, NONE, 0, 1024, 0, 3, 2),
    (1, LG, NONE, 0, 300, 256, 1, 1),
    (1, LG, NONE, 0, 300, 256, 3, 1),
    (1, LG, NONE, 0, 300, 256, 1, 2),
    (1, LG_SHARP, NONE, 0, 300, 256, 3, 12),
    (1, LG_SHARP, NONE, 0, 1024, 0, 1, 12),
    (1, LG, NONE, SYSTEMATIC, 300, 256, 3, 12),
    (1, LG, OPTIMAL, 0, 300, 256, 3, 12),
    (1, LG, OPTIMAL, 0, 1024, 0, 1, 2),
    (2, SV, NONE, 0, 65, 0, 3, 12),
    (2, SV, NONE, 0, 300, 256, 1, 12),
    (2, SV, NONE, 0, 1300, 256, 1, 2),
    (3, UC, NONE, 0, 1, 0, 3, 2),
    (3, UC, NONE, 0, 65, 0, 3, 12),
    (3, UC, NONE, 0, 300, 256, 3, 12),
    (3, UC, NONE, 0, 1300, 256, 1, 2),
    (3, UC, NONE, 0, 1024, 0, 1, 2),
    (3, UC, OPTIMAL, 0, 300, 256, 3, 12),
    (3, UC, OPTIMAL, 0, 65, 0, 1, 1),
]


@pytest.mark.parametrize("model,raw,proposal,flags,n,seg,nth,T", CASES)
def test_smooth_equals_host_twin(L, model, raw, proposal, flags, n, seg, nth, T):
    rows = rows_for(raw, nth)
    h = run_recorded(L, model, rows, n, seg, T, proposal, flags, check_state=True)
    _, w, ws = compare_with_host(L, h, model, rows)
    assert same(ws[T - 1], w[T - 1])
    if raw is LG_SHARP:
        assert (w == 0).mean() > 0.5
    h.close()


def test_position_independence_and_repeatability(L):
    rows = rows_for(LG, 3)
    hb = run_recorded(L, 1, rows, 300, 256, 12, streams=[0, 1, 2])
    wb = hb.smooth()[0]
    assert same(wb, hb.smooth()[0])                           # the same handle again
    hb2 = run_recorded(L, 1, rows, 300, 256, 12, streams=[0, 1, 2])
    assert same(wb, hb2.smooth()[0])                          # a second run
    for m in range(3):
        h1 = run_recorded(L, 1, rows[m], 300, 256, 12, streams=[m])
        assert same(h1.smooth()[0][:, 0], wb[:, m]), m
        h1.close()
    # more steps, then again: the first 12 filter clouds are the same, the smoothed weights use the longer series
    _, y = L.simulate(1, LG, 14, 1998)
    h = L.Handle(1, 1, 300, seg=256, seed=11)
    h.set_params(rows[0])
    h.history_begin(14)
    h.init(float(y[0]))
    for t in range(1, 12):
        h.step(float(y[t]))
    assert same(h.smooth()[0][:, 0], wb[:, 0])
    h.step(float(y[12]))
    x, w = clouds(h)
    assert same(h.smooth()[0][:, 0], L.host_smooth(1, rows[0], x[:, :, 0], w[:, 0])[0])
    for hh in (hb, hb2, h):
        hh.close()


def test_rts_pin_on_the_device(L):
    """n_x = 1024, 16 independent filters (streams 0..15 of one handle): the smoothed mean within 4 standard errors of the exact
    RTS mean at every t, the averaged smoothed variance within 10 % of the RTS variance; the filtered means miss"""
    T, K = 24, 16
    _, y = L.simulate(1, LG, T, 1998)
    m_rts, P_rts = R.rts_smoother(LG, y)
    h = L.Handle(1, K, 1024, seed=77)
    h.set_params(np.tile(LG, (K, 1)))
    h.history_begin(T)
    fm = np.zeros((T, K))
    for t in range(T):
        h.init(float(y[0])) if t == 0 else h.step(float(y[t]))
        fm[t] = h.moments()[0][0]
    _, mean, var = h.smooth(weights=False)
    sm, sv = mean[:, 0, :], var[:, 0, :]
    z = np.abs(sm.mean(axis=1) - m_rts) / (sm.std(axis=1, ddof=1) / np.sqrt(K))
    ratio = sv.mean(axis=1) / P_rts
    print("max |z| %.2f, variance ratio %.3f .. %.3f" % (z.max(), ratio.min(), ratio.max()))
    assert np.all(z <= 4.0), z
    assert np.all(np.abs(ratio - 1) <= 0.10), ratio
    zf = np.abs(fm.mean(axis=1) - m_rts) / (fm.std(axis=1, ddof=1) / np.sqrt(K))
    assert (zf[:T - 1] > 4.0).sum() >= 12, zf
    h.close()


def test_refusals_and_state_rules(L):
    lib = L.lib()
    _, y = L.simulate(1, LG, 8, 1998)
    h = L.Handle(1, 2, 300, seg=256, seed=3)
    h.set_params(rows_for(LG, 2))
    assert h.history_len() == 0
    with pytest.raises(L.SmcError):
        h.smooth()                                            # nothing recorded: not armed
    with pytest.raises(L.SmcError):
        h.history_get(0)
    h.history_begin(3)
    with pytest.raises(L.SmcError):
        h.smooth()                                            # armed, still nothing recorded
    assert lib.smc_smooth(h._h, None, None, None) == -3       # SMC_ESTATE
    h.init(float(y[0]))
    h.step(float(y[1]))
    snap = h.state(want_anc=False)
    other = L.Handle(1, 2, 300, seg=256, seed=4)
    other.set_params(rows_for(LG, 2))
    other.init(float(y[0]))
    ESTATE = -3
    yy = np.ascontiguousarray(y)
    z = np.zeros(2)
    dp = L._d
    assert lib.smc_log_likelihood(h._h, dp(yy), 8, dp(z), None, None) == ESTATE
    assert lib.smc_step_window(h._h, dp(yy), 2, dp(np.zeros((2, 2))), None) == ESTATE
    assert lib.smc_step_commit(h._h, 1) == ESTATE
    perm = np.array([1, 0], dtype=np.int32)
    assert lib.smc_permute(h._h, perm.ctypes.data_as(L._i32p)) == ESTATE
    mask = np.ones(2, dtype=np.uint8)
    assert lib.smc_copy_from(h._h, other._h, mask.ctypes.data_as(L.C.POINTER(L.C.c_uint8))) == ESTATE
    import torch
    idx = np.array([0], dtype=np.int32)
    buf = torch.empty((1, other.slot_bytes() // 8), dtype=torch.int64, device="cuda")
    other.pack_slots(idx, buf.data_ptr())                     # a real packed slot: the refusal is the handle's, not the buffer's
    assert lib.smc_unpack_slots(h._h, idx.ctypes.data_as(L._i32p), 1, L.C.c_void_p(buf.data_ptr())) == ESTATE
    h.pack_slots(idx, buf.data_ptr())                         # packing reads only: allowed
    ta, tm = L.C.c_double(), L.C.c_double()
    assert lib.smc_time_step_kernel(h._h, dp(yy), 8, 1, L.C.byref(ta), L.C.byref(tm)) == ESTATE
    # the device PMMH: configured, so that the refusal is the record's and not "not configured"; as proposal handle and as main
    import sequential_monte_carlo_amd as smc
    fam, par = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(), smc.LogNormal()]).spec()
    tmap = ([0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    h.pmmh_configure(fam, par, *tmap)
    other.pmmh_configure(fam, par, *tmap)
    theta, lz = np.tile([0.5, 0.9, 0.8], (2, 1)), np.zeros(2)
    chol, scales, seeds = np.eye(3) * 0.01, np.ones(1), np.array([7], dtype=np.uint64)
    for prop, main in ((h, other), (other, h)):
        rc = lib.smc_pmmh_rejuvenate(prop._h, main._h, dp(yy), 8, 1.0, dp(chol), dp(scales), 1, seeds.ctypes.data_as(L._u64p), 5,
                                     dp(theta), dp(lz), None, None)
        assert rc == ESTATE and b"records its steps" in lib.smc_last_error()
    st = h.state(want_anc=False)
    assert same(st[0], snap[0]) and same(st[1], snap[1]) and h.history_len() == 2       # nothing changed
    h.step(float(y[2]))
    assert lib.smc_step(h._h, float(y[3]), dp(z), None) == ESTATE                          # beyond T_cap
    assert h.history_len() == 3
    assert lib.smc_history_get(h._h, 3, None, None) == -1                                  # SMC_EINVAL: outside the record
    ws3 = h.smooth()[0]
    h.init(float(y[0]))                                       # smc_init restarts the record
    assert h.history_len() == 1
    assert same(h.smooth()[0][0], h.state(want_anc=False)[1])                              # T = 1: ws = w
    assert ws3.shape == (3, 2, 300)
    # a transition scale that is not positive and finite; the family without a transition density
    bad = rows_for(LG, 2)
    bad[1, 2] = 0.0
    h.set_params(bad)
    assert lib.smc_smooth(h._h, None, None, None) == -1
    h.set_params(rows_for(LG, 2))
    h.history_end()
    assert h.history_len() == 0
    with pytest.raises(L.SmcError):
        h.history_get(0)
    rb = L.Handle(L.MODEL_UCSV_RB, 1, 300, seed=3)
    rb.set_params(np.array([UC]))
    rb.history_begin(2)
    rb.init(0.3)
    assert lib.smc_smooth(rb._h, None, None, None) == -1
    rb.close()
    # an absurd capacity: SMC_ENOMEM, and the handle is as it was
    assert lib.smc_history_begin(h._h, 1 << 50) == -4
    assert h.history_len() == 0
    # after smc_history_end the handle's log_likelihood is that of a handle that was never armed
    fresh = L.Handle(1, 2, 300, seg=256, seed=3)
    fresh.set_params(rows_for(LG, 2))
    assert same(h.log_likelihood(y), fresh.log_likelihood(y))
    a, b = h.state(want_anc=False), fresh.state(want_anc=False)
    assert same(a[0], b[0]) and same(a[1], b[1])
    # a handle recycled from a destroyed, ARMED one comes back disarmed
    arm = L.Handle(1, 2, 700, seg=256, seed=9)
    arm.set_params(rows_for(LG, 2))
    arm.history_begin(4)
    arm.init(float(y[0]))
    arm.close()
    again = L.Handle(1, 2, 700, seg=256, seed=9)
    again.set_params(rows_for(LG, 2))
    assert again.history_len() == 0
    ref = L.Handle(1, 2, 700, seg=256, seed=9)
    ref.set_params(rows_for(LG, 2))
    assert same(again.log_likelihood(y), ref.log_likelihood(y))
    for hh in (h, other, fresh, again, ref):
        hh.close()


def test_smoother_python_shapes(L):
    import sequential_monte_carlo_amd as smc
    T, N = 6, 300
    m1 = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
    _, y = smc.simulate(m1, T, seed=1998)
    x, w, logZ, s = smc.smoother(N, y, m1, seed=5, weights=True)
    assert isinstance(logZ, float) and np.asarray(x).shape == (N,) and np.asarray(w).shape == (N,)
    assert s["mean"].shape == (T,) and s["var"].shape == (T,) and s["logmu"].shape == (T,) and s["ess"].shape == (T,)
    assert s["weights"].shape == (T, N) and s["x"].shape == (T, N)
    assert abs(logZ - s["logmu"].sum()) <= 1e-9 * abs(logZ) and np.all(s["ess"] > 0)
    # the same numbers as log_likelihood's filter (the smoother does not disturb it), and the last smoothed row is the filtered one
    x2, w2, logZ2, lm2, es2 = smc.log_likelihood(N, y, m1, seed=5, trace=True)
    assert logZ2 == logZ and same(np.asarray(w2), np.asarray(w)) and same(lm2, s["logmu"]) and same(es2, s["ess"])
    assert same(s["weights"][T - 1], np.asarray(w)) and same(s["x"][T - 1], np.asarray(x))
    ms = [smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=q, R=0.8) for q in (0.7, 0.9, 1.1)]
    x, w, logZ, s = smc.smoother(N, y, ms, seed=5, weights=True)
    assert logZ.shape == (3,) and np.asarray(x).shape == (3, N)
    assert s["mean"].shape == (T, 3) and s["ess"].shape == (T, 3) and s["weights"].shape == (T, 3, N) and s["x"].shape == (T, 3, N)
    # a state of three coordinates: the coordinate axis comes last
    uc = smc.UCSV((0.2, 0.3), 1.0, (-1.0, -0.5))
    _, _, _, s3 = smc.smoother(N, y, uc, seed=5)
    assert s3["mean"].shape == (T, 3) and s3["var"].shape == (T, 3) and "weights" not in s3
    _, _, _, s3 = smc.smoother(N, y, [uc, uc], seed=5, weights=True)
    assert s3["mean"].shape == (T, 2, 3) and s3["weights"].shape == (T, 2, N) and s3["x"].shape == (T, 2, N, 3)
    with pytest.raises(L.SmcError):
        smc.smoother(N, y, smc.MarginalUCSV((0.2, 0.3), 1.0, (-1.0, -0.5)), seed=5)
    # IBIS: out of scope (its exact smoother is RTS); refused by type before anything runs
    prior = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(), smc.LogNormal()])
    tmap = smc.ThetaMap(1, [0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    ib = smc.IBIS(16, lambda th: smc.LinearModel(th[0], 1.0, th[1], th[2], 0.0, 1.0), prior, 2, 0.5, seed=3, theta_map=tmap)
    with pytest.raises(TypeError, match="RTS"):
        smc.smoothed_state(ib, y)
    ib.close()


def test_smoothed_state_integrates_the_smoothers(L):
    import sequential_monte_carlo_amd as smc
    M, N, T = 8, 256, 12
    m0 = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
    _, y = smc.simulate(m0, T, seed=1998)
    prior = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(), smc.LogNormal()])
    s = smc.SMC(N, M, lambda th: smc.UnivariateLinearGaussian(A=th[0], B=1.0, Q=th[1], R=th[2]), prior, 2, 0.5, seed=22)
    smc.smc2(s, y[:1])
    for t in range(2, 6):
        smc.smc2_step(s, y, t, verbose=False)
    om = np.asarray(s.omega)
    mean, var = smc.smoothed_state(s, y, seed=99)
    assert mean.shape == (T,) and var.shape == (T,)
    # by hand from smoother outputs, in two blocks of other sizes than smoothed_state's
    models = [s.model(th) for th in s.theta]
    parts = [smc.smoother(N, y, models[a:b], seed=99, streams=np.arange(a, b, dtype=np.uint32))[3] for a, b in ((0, 3), (3, 8))]
    mm = np.concatenate([p["mean"] for p in parts], axis=1)
    vv = np.concatenate([p["var"] for p in parts], axis=1)
    keep = om > 0
    em = np.add.reduce(om[keep][None, :] * mm[:, keep], axis=1)
    ev = np.add.reduce(om[keep][None, :] * vv[:, keep], axis=1) + np.add.reduce(om[keep][None, :] * (mm[:, keep] - em[:, None]) ** 2, axis=1)
    assert same(mean, em) and same(var, ev)
    assert same(mean, smc.smoothed_state(s, y, seed=99, max_bytes=1)[0])        # one parameter particle per block: the same bits
    assert np.all(var > 0)
    s.backend.close()
