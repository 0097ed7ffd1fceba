"""The conditional particle filter on the device (pytest -m gpu): handles created with FLAG_CONDITIONAL pin one slot of
every step to a reference trajectory.  The reference is tests/conditional_reference.py (composed from the oracle's track, resampler
and normals, the host twin of the whole step and the host's slot rule and log-weight; tests/test_conditional_host.py pins it on the
CPU).  Comparisons are exact (the same bits; array_equal for ancestors and the raw fixed-point weights) except the statistical
statement, which uses 5 standard errors of normal samples from the exact moments.

  a. bit-exact after every step: logmu, ess, x, w, ancestors, the raw weights and the record, for LG1D, SV1D and UCSV3D, one filter
     (the by-value shape) and three with distinct rows, streams and references, on (n_x, seg) = (4, auto), (5, auto) - the ragged pair
     beside a masked sibling -, (600, 256) - three ragged segments - and (1024, auto); the retained trajectory is in the record
  b. smc_reference_from_paths == the gather of smc_sample_paths' own states; a planted dead path keeps the old reference
  c. every refusal, each leaving the handle usable
  d. invariance: ParticleGibbs on 4096 chains of 4 particles from exact posterior draws
  e. smoother(reference=...) == ParticleGibbs.sweep() on the first sweep
"""
import numpy as np
import pytest

import conditional_reference as CF
import smoother_planted as SP
import test_gpu_paths as TP

pytestmark = pytest.mark.gpu

T, SEED = 12, 5
SHAPES = [(4, 0), (5, 0), (600, 256), (1024, 0)]
STREAMS = {1: [4], 3: [7, 2, 11]}


def series(model, length=T, seed=1998):
    from oracle import binding as ob
    return ob.simulate(model, TP.RAW[model], length, seed)[1]


def references(model, nth, length=T, seed=3):
    """distinct finite references [T][d][n_theta] near the model's states (a simulated trajectory per filter, shifted)"""
    from oracle import binding as ob
    out = np.zeros((length, CF.ROWS[model], nth))
    for th in range(nth):
        out[:, :, th] = ob.simulate(model, TP.RAW[model], length, seed + th)[0].T + 0.125 * th
    return out


def make(L, model, nth, n, seg, seed=SEED, flags=0):
    h = L.Handle(model, nth, n, seg=seg, seed=seed, flags=L.FLAG_CONDITIONAL | L.FLAG_ANCESTORS | flags)
    h.set_params(TP.raws_for(model, nth))
    h.set_streams(STREAMS[nth])
    return h


def snap(h):
    return h.state() + h.weights_raw()


# ---- a. bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 2, 3])
@pytest.mark.parametrize("n,seg", SHAPES)
@pytest.mark.parametrize("nth", [1, 3])
def test_bits_after_every_step(L, ob, model, n, seg, nth):
    y, xref = series(model), references(model, nth)
    r = CF.run_series(L, ob, model, TP.raws_for(model, nth), n, seg, SEED, y, xref, streams=STREAMS[nth])
    h = make(L, model, nth, n, seg)
    assert h.conditional and (h.seg, h.nseg) == (r["seg"], r["nseg"])
    if (n, seg) == (600, 256):
        assert h.nseg == 3 and len({int(k) // 256 for k in r["ks"].ravel()}) == 3      # the retained slot visits every block
    h.set_reference(xref)
    assert TP.same(h.get_reference(), xref)
    h.history_begin(T)
    for t in range(T):
        ctx = (model, n, seg, nth, t)
        if t == 0:
            lm, es = h.init(float(y[0])), h.logZ()[1]
        else:
            lm, es = h.step(float(y[t]))
        assert TP.same(lm, r["lm"][t]) and TP.same(es, r["es"][t]), ctx + (lm, r["lm"][t], es, r["es"][t])
        assert CF.first_mismatch(snap(h), r["snaps"][t]) is None, ctx + (CF.first_mismatch(snap(h), r["snaps"][t]),)
    for t in range(T):
        hx, hw = h.history_get(t)
        assert TP.same(hx, r["clouds"][t][0]) and TP.same(hw, r["clouds"][t][1]), (model, n, seg, nth, t, "record")
        for th in range(nth):                                      # the retained trajectory is in the record, bit for bit
            assert TP.same(hx[:, th, r["ks"][t, th]], xref[t, :, th]), (model, n, seg, nth, t, th, "retained slot")
    h.history_end()
    h.close()


@pytest.mark.parametrize("model,n,seg,pid", [(1, 5000, 1024, "M1"), (3, 33000, 256, "M2"), (2, 140000, 256, "G"), (1, 20000, 8192, "M1")])
def test_bits_on_every_step_launch_path(L, ob, model, n, seg, pid):
    """the other geometries of a step launch (tests/test_gpu_paths.py): one record per thread with a ragged last segment, two records
    per thread, the segment table from k_table, and the longest segment; one filter, four steps"""
    Tn = 4
    y, xref = series(model, Tn), references(model, 1, Tn)
    r = CF.run_series(L, ob, model, TP.raws_for(model, 1), n, seg, SEED, y, xref, streams=STREAMS[1])
    h = make(L, model, 1, n, seg)
    assert TP.path_of(h) == pid and (h.seg, h.nseg) == (r["seg"], r["nseg"])
    h.set_reference(xref)
    for t in range(Tn):
        lm, es = (h.init(float(y[0])), h.logZ()[1]) if t == 0 else h.step(float(y[t]))
        assert TP.same(lm, r["lm"][t]) and TP.same(es, r["es"][t]), (pid, t, lm, r["lm"][t], es, r["es"][t])
        assert CF.first_mismatch(snap(h), r["snaps"][t]) is None, (pid, t, CF.first_mismatch(snap(h), r["snaps"][t]))
    h.close()


# ---- b. the reference from a path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,n,seg", [(1, 600, 256), (3, 300, 0)])
def test_reference_from_paths_is_the_gather(L, model, n, seg):
    nth, Tn = 3, 8
    y, xref = series(model, Tn), references(model, nth, Tn)
    h = make(L, model, nth, n, seg)
    h.set_reference(xref)
    h.history_begin(Tn)
    h.init(float(y[0]))
    for t in range(1, Tn):
        h.step(float(y[t]))
    with pytest.raises(L.SmcError, match="error -3"):              # no walk yet
        h.reference_from_paths(0)
    idx, xs = h.sample_paths(2, 77)                                # xs [T][d][n_theta][M]
    assert np.all(idx >= 0)
    with pytest.raises(L.SmcError, match="error -1"):
        h.reference_from_paths(2)
    assert h.reference_from_paths(1) == 0
    assert TP.same(h.get_reference(), xs[:, :, :, 1])
    # a planted dead path: filter 1 collapses at the middle step of the record (tests/smoother_planted.py)
    hx, hw = h.history_get(SP.mid(Tn))
    hw[1] = 0.0
    h.history_put(SP.mid(Tn), w=hw)
    before = h.get_reference()
    idx, xs = h.sample_paths(1, 78)
    assert np.all(idx[:, 1] == -1) and np.all(idx[:, [0, 2]] >= 0)
    assert h.reference_from_paths(0) == 1
    got = h.get_reference()
    assert TP.same(got[:, :, 1], before[:, :, 1]) and TP.same(got[:, :, [0, 2]], xs[:, :, [0, 2], 0])
    # a reference of another length has nothing for the dead filter to keep: refused, nothing changes
    h.set_reference(before[:5])
    with pytest.raises(L.SmcError, match="error -3"):
        h.reference_from_paths(0)
    assert TP.same(h.get_reference(), before[:5])
    h.history_end()
    h.close()


# ---- c. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(L, ob):
    CO = L.FLAG_CONDITIONAL
    for args in ((1, 2, 64, CO | L.FLAG_SYSTEMATIC), (1, 2, 64, CO | L.FLAG_NAN_MISSING), (4, 2, 64, CO), (1, 1, (1 << 20) + 1, CO)):
        with pytest.raises(L.SmcError, match="error -1"):
            L.Handle(args[0], args[1], args[2], flags=args[3])
    L.Handle(1, 1, 1 << 20, flags=CO).close()                      # the limit itself is accepted
    nth, n, Tn = 2, 64, 6
    y, xref = series(1, Tn), references(1, nth, Tn)
    raws = TP.raws_for(1, nth)
    r = CF.run_series(L, ob, 1, raws, n, 0, SEED, y, xref)

    def runs(h):
        """the handle still runs the conditional filter, bit for bit"""
        h.reseed(SEED)
        lm = [h.init(float(y[0]))] + [h.step(float(v))[0] for v in y[1:]]
        assert TP.same(np.array(lm), r["lm"]) and CF.first_mismatch(snap(h), r["snaps"][-1]) is None

    h = L.Handle(1, nth, n, seed=SEED, flags=CO | L.FLAG_ANCESTORS)
    assert not h.resident
    h.set_params(raws)
    with pytest.raises(L.SmcError, match="error -3"):              # no reference yet
        h.init(float(y[0]))
    for bad in (np.nan, np.inf):
        xb = xref.copy()
        xb[2, 0, 1] = bad
        with pytest.raises(L.SmcError, match="error -1"):
            h.set_reference(xb)
    h.set_reference(xref)
    runs(h)
    with pytest.raises(L.SmcError, match="error -3"):              # the reference ends here
        h.step(0.1)
    for kind, par in ((L.PROP_OPTIMAL, None), (L.PROP_AFFINE, np.tile([0.3, 0.2, 0.1, 2.0], (nth, 1)))):
        with pytest.raises(L.SmcError, match="error -1"):
            h.set_proposal(kind, par)
    h.set_proposal(L.PROP_NONE)
    before = snap(h)
    with pytest.raises(L.SmcError, match="error -3"):
        h.log_likelihood(y)
    with pytest.raises(L.SmcError, match="error -3"):
        h.log_likelihood(y, trace=True)
    with pytest.raises(L.SmcError, match="error -3"):
        h.step_window(y[:3])
    with pytest.raises(L.SmcError, match="error -3"):
        h.step_commit(1)
    with pytest.raises(L.SmcError, match="error -3"):
        h.time_step_kernel(y)
    # PMMH, either role: the conditional handle as the proposal filters, and as the main filters of a plain handle
    plain = L.Handle(1, nth, n, seed=SEED, flags=L.FLAG_ANCESTORS)
    plain.set_params(raws)
    plain.init(float(y[0]))
    pm = ([1], [[0.0, 1.0, 0, 0, 0]], [0, -1, -1, -1, -1, -1], [0.0, 1.0, 0.9, 0.8, 0.0, 1.0])
    for prop, main in ((h, None), (h, plain), (plain, h)):
        prop.pmmh_configure(*pm)
        with pytest.raises(L.SmcError, match="error -3"):
            prop.pmmh_rejuvenate(main, y, 1.0, np.eye(1), [1.0], [9], 11, np.full((nth, 1), 0.5), np.zeros(nth))
    plain.close()
    assert CF.first_mismatch(snap(h), before) is None              # the refused calls changed nothing
    runs(h)
    # the reference calls on a handle without the flag
    g = L.Handle(1, nth, n, seed=SEED)
    for call in (lambda: g.set_reference(xref), g.get_reference, lambda: g.reference_from_paths(0)):
        with pytest.raises(L.SmcError, match="error -3"):
            call()
    g.close()
    h.close()
    # a recycled handle has no reference
    h2 = L.Handle(1, nth, n, seed=SEED, flags=CO | L.FLAG_ANCESTORS)
    h2.set_params(raws)
    with pytest.raises(L.SmcError, match="error -3"):
        h2.init(float(y[0]))
    h2.close()


# ---- d. invariance on the device --------------------------------------------------------------------------------------------------
def test_particle_gibbs_leaves_the_posterior_invariant(L, ob):
    """ParticleGibbs, the README LG row, T = 6, 4096 chains of 4 particles started from exact posterior draws, 4 sweeps: means,
    variances and lag-1 covariances within 5 standard errors of the exact smoothed moments (the standard errors of normal samples,
    from the exact moments: conditional_reference.worst_z).  The seeds are fixed."""
    import sequential_monte_carlo_amd as smc
    chains, Tn = 4096, 6
    _, y = ob.simulate(1, CF.README_LG, Tn, 1998)
    start = CF.exact_posterior_draws(CF.README_LG, y, chains, np.random.default_rng(11))
    pg = smc.ParticleGibbs(4, y, None, reference=start.T, seed=2026, rows=(1, np.tile(CF.README_LG, (chains, 1))))
    for k in range(4):
        path = pg.sweep()
        assert path.shape == (Tn, chains) and pg.kept == 0 and pg.sweeps == k + 1
    z = CF.worst_z(path.T, CF.README_LG, y)
    print("ParticleGibbs, 4096 chains x 4 particles, 4 sweeps: worst |z| of means %.2f, variances %.2f, lag-1 covariances %.2f" % z)
    assert max(z) <= 5.0, z
    assert pg.logmu.shape == (Tn, chains) and pg.ess.shape == (Tn, chains) and np.all(pg.ess >= 1.0) and np.all(pg.ess <= 4.0)
    # the chains moved: a sweep that returned its reference would pass the band above
    assert np.mean(path.T != start) > 0.5
    pg.close()


# ---- e. the two public routes agree ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,single", [(1, True), (3, False)])
def test_smoother_with_reference_is_the_first_sweep(L, model, single):
    import sequential_monte_carlo_amd as smc
    nth, Tn, n = (1 if single else 3), 10, 200
    y, xref = series(model, Tn), references(model, nth, Tn)
    rows = (model, TP.raws_for(model, nth))
    ref = np.moveaxis(xref, 1, -1)                                  # [T][n_theta][d]
    ref = ref[..., 0] if model == 1 else ref
    if single:
        from sequential_monte_carlo_amd.models import LinearModel
        mdl, rows, ref = LinearModel(*TP.RAW[1]), None, ref[:, 0]
    else:
        mdl = None
    pg = smc.ParticleGibbs(n, y, mdl, reference=ref, seed=41, streams=STREAMS[nth], rows=rows)
    assert TP.same(pg.path, ref)
    p1 = pg.sweep()
    x, w, logZ, s = smc.smoother(n, y, mdl, seed=pg.sweep_seed(1), streams=STREAMS[nth], rows=rows, paths=1, smooth=False, reference=ref)
    sp = s["paths"][:, 0] if single else s["paths"][:, :, 0]
    assert p1.shape == ref.shape and TP.same(p1, sp)
    assert TP.same(pg.logmu, s["logmu"]) and TP.same(pg.ess, s["ess"])
    # the second sweep starts from the first one's path under fresh counters
    p2 = pg.sweep()
    x, w, logZ, s = smc.smoother(n, y, mdl, seed=pg.sweep_seed(2), streams=STREAMS[nth], rows=rows, paths=1, smooth=False, reference=p1)
    assert TP.same(p2, s["paths"][:, 0] if single else s["paths"][:, :, 0]) and not TP.same(p2, p1)
    pg.close()
