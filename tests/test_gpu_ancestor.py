"""Ancestor sampling on the device (pytest -m gpu): handles created with FLAG_CONDITIONAL | FLAG_ANCESTOR_SAMPLING keep
the ancestor vectors in their record, and smc_ancestor_sweep draws the next reference from it without a backward walk.  The reference
is the host twin smc_host_ancestor_sweep, which tests/test_ancestor_host.py pins on the CPU against the exact CDF and a restated trace.
Comparisons are exact (the same bits) except the statistical statement.

  a. J, idx and the new reference == the host twin fed this run's record, ancestor plane and old reference: LG1D, SV1D, UCSV3D, one
     filter and three, (n_x, seg) = (4, auto), (5, auto), (600, 256), (1024, auto) - one wave per (step, filter) and four -, and two
     clouds of more sources than one pass of a workgroup with ragged tails
  b. the ancestor plane == the ancestor vector read after every step, and
  c. the flag changes no step bits: a flagged handle against one created with CONDITIONAL | ANCESTORS
  d. planted records (history_put / history_put_ancestors): zero-weight sources, a reference out of reach, a dead filter
  e. every refusal, with a correct sweep afterwards; smc_live_bytes returns
  f. invariance: ParticleGibbs(ancestor_sampling=True) on 4096 chains of 4 particles from exact posterior draws
  g. ParticleGibbs.sweep() == Handle.ancestor_sweep on a hand-driven handle
"""
import ctypes as C
import gc

import numpy as np
import pytest

import conditional_reference as CF
import test_gpu_conditional as TC
import test_gpu_paths as TP

pytestmark = pytest.mark.gpu

T, SEED, PATH_SEED = 7, 5, 0xA5CE5707
STREAMS = TC.STREAMS


def make(L, model, nth, n, seg, seed=SEED, sampling=True):
    h = L.Handle(model, nth, n, seg=seg, seed=seed,
                 flags=L.FLAG_CONDITIONAL | (L.FLAG_ANCESTOR_SAMPLING if sampling else L.FLAG_ANCESTORS))
    h.set_params(TP.raws_for(model, nth))
    h.set_streams(STREAMS[nth])
    return h


def run(h, y, xref):
    """the recorded conditional run over y: (logmu, ess, the snapshot and the ancestors after every step)"""
    h.set_reference(xref)
    h.history_begin(len(y))
    out = []
    for t in range(len(y)):
        lm, es = (h.init(float(y[0])), h.logZ()[1]) if t == 0 else h.step(float(y[t]))
        out.append((lm, es, TC.snap(h)))
    return out


def record_of(h):
    """(x [T][d][n_theta][n], w [T][n_theta][n], a [T][n_theta][n]) of the handle's record"""
    Tn = h.history_len()
    rec = [h.history_get(t) for t in range(Tn)]
    return np.stack([r[0] for r in rec]), np.stack([r[1] for r in rec]), np.stack([h.history_get_ancestors(t) for t in range(Tn)])


def twin(L, model, nth, rec, xold, seed, path_seed):
    """the host twin per filter -> (J [T][n_theta], idx [T][n_theta], xref [T][d][n_theta])"""
    x, w, a = rec
    raws = TP.raws_for(model, nth)
    res = [L.host_ancestor_sweep(model, raws[th], x[:, :, th], w[:, th], a[:, th], xold[:, :, th], seed, path_seed, STREAMS[nth][th])
           for th in range(nth)]
    return np.stack([r[0] for r in res], axis=1), np.stack([r[1] for r in res], axis=1), np.stack([r[2] for r in res], axis=2)


def check_sweep(L, h, model, nth, xold, seed=SEED, path_seed=PATH_SEED, kept_want=0):
    rec = record_of(h)
    J, idx, kept = h.ancestor_sweep(path_seed)
    hJ, hidx, href = twin(L, model, nth, rec, xold, seed, path_seed)
    assert np.array_equal(J, hJ), (model, nth, np.argwhere(J != hJ)[:4])
    assert np.array_equal(idx, hidx), (model, nth, np.argwhere(idx != hidx)[:4])
    assert TP.same(h.get_reference(), href) and kept == kept_want, (model, nth, kept)
    return J, idx


# ---- a. bits against the host twin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 2, 3])
@pytest.mark.parametrize("n,seg", TC.SHAPES)
@pytest.mark.parametrize("nth", [1, 3])
def test_sweep_is_the_host_twin(L, model, n, seg, nth):
    y, xref = TC.series(model, T), TC.references(model, nth, T)
    h = make(L, model, nth, n, seg)
    run(h, y, xref)
    J, idx = check_sweep(L, h, model, nth, xref)
    assert np.all(J[0] == -1) and np.all(J[1:] >= 0) and np.all(idx >= 0) and np.all(idx < n)
    assert not TP.same(h.get_reference(), xref)
    h.close()


@pytest.mark.parametrize("model,n,seg", [(1, 5000, 1024), (3, 33000, 256)])
def test_sweep_over_many_tiles(L, model, n, seg):
    """more sources than one pass of a workgroup of 256, ragged last tiles (5000 = 19 x 256 + 136, 33000 = 128 x 256 + 232)"""
    y, xref = TC.series(model, T), TC.references(model, 1, T)
    h = make(L, model, 1, n, seg)
    run(h, y, xref)
    check_sweep(L, h, model, 1, xref)
    h.close()


# ---- b, c. the ancestor plane; the flag changes no step bits ---------------------------------------------------------------------
@pytest.mark.parametrize("model,n,seg,nth", [(1, 600, 256, 3), (3, 5, 0, 1), (2, 1024, 0, 3)])
def test_flag_changes_no_step_and_records_the_ancestors(L, model, n, seg, nth):
    y, xref = TC.series(model, T), TC.references(model, nth, T)
    h, g = make(L, model, nth, n, seg), make(L, model, nth, n, seg, sampling=False)
    f = C.c_uint32()
    assert L.lib().smc_get_flags(h._h, C.byref(f)) == 0
    assert f.value == L.FLAG_CONDITIONAL | L.FLAG_ANCESTOR_SAMPLING | L.FLAG_ANCESTORS and h.ancestor_sampling and not g.ancestor_sampling
    a, b = run(h, y, xref), run(g, y, xref)
    for t in range(T):
        assert TP.same(a[t][0], b[t][0]) and TP.same(a[t][1], b[t][1]), (model, n, t)
        assert CF.first_mismatch(a[t][2], b[t][2]) is None, (model, n, t, CF.first_mismatch(a[t][2], b[t][2]))
        hx, hw = h.history_get(t)
        gx, gw = g.history_get(t)
        assert TP.same(hx, gx) and TP.same(hw, gw)
        want = a[t][2][2] if t else np.full((nth, n), -1, dtype=np.int32)      # state()'s ancestors after step t
        assert np.array_equal(h.history_get_ancestors(t), want), (model, n, t)
    h.close()
    g.close()


# ---- d. planted records ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 3])
def test_planted_records(L, model):
    """filter 0: a reference row out of every source's reach (S = 0: J_2 is the retained slot of step 1); filter 1: every last
    weight 0 (dead: idx = -1, it keeps its reference, kept counts it); filter 2: half the sources of every step have the weight 0
    and the reference row itself, or NaN, as their state; and random ancestor vectors everywhere"""
    nth, n = 3, 64
    y, xref = TC.series(model, T), TC.references(model, nth, T)
    h = make(L, model, nth, n, 0)
    run(h, y, xref)
    rng = np.random.default_rng(17)
    far = xref.copy()
    far[2, :, 0] = 1e200
    off = np.arange(n) % 2 == 0
    for t in range(T):
        x, w = h.history_get(t)
        if t < T - 1:
            w[2, off] = 0.0
            x[:, 2, off] = far[t + 1, :, 2][:, None]
            x[:, 2, off & (np.arange(n) % 4 == 0)] = np.nan
        else:
            w[1] = 0.0
        h.history_put(t, x, w)
        if t:
            h.history_put_ancestors(t, rng.integers(0, n, size=(nth, n)))
    h.set_reference(far)
    J, idx = check_sweep(L, h, model, nth, far, kept_want=1)
    assert J[2, 0] == L.host_conditional_slot(SEED, STREAMS[nth][0], 1, n)
    assert np.all(idx[:, 1] == -1) and np.all(idx[:, [0, 2]] >= 0)
    assert not np.any(off[J[1:, 2]])
    got = h.get_reference()
    assert TP.same(got[:, :, 1], far[:, :, 1]) and not TP.same(got[:, :, 2], far[:, :, 2])
    h.close()


# ---- e. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(L):
    AS, CO = L.FLAG_ANCESTOR_SAMPLING, L.FLAG_CONDITIONAL
    model, nth, n = 1, 3, 64
    y, xref = TC.series(model, T), TC.references(model, nth, T)

    def cycle(disturb):
        for flags in ((AS,), (AS | L.FLAG_ANCESTORS,)) if disturb else ():
            with pytest.raises(L.SmcError, match="error -1.*CONDITIONAL"):      # the flag alone
                L.Handle(model, nth, n, flags=flags[0])
        h = make(L, model, nth, n, 0)
        if disturb:
            plain = make(L, model, nth, n, 0, sampling=False)              # CONDITIONAL | ANCESTORS: no plane, no sweep
            run(plain, y, xref)
            for call in (lambda: plain.history_get_ancestors(1), lambda: plain.history_put_ancestors(1, np.zeros((nth, n), dtype=np.int32)),
                         lambda: plain.ancestor_sweep(1)):
                with pytest.raises(L.SmcError, match="error -3.*ANCESTOR_SAMPLING"):
                    call()
            plain.close()
            with pytest.raises(L.SmcError, match="error -3.*reference"):       # no reference
                h.ancestor_sweep(1)
            h.set_reference(xref)
            for call in (lambda: h.ancestor_sweep(1), lambda: h.history_get_ancestors(0)):
                with pytest.raises(L.SmcError, match="error -3.*record"):      # not armed
                    call()
        run(h, y[:4], xref[:4])                                            # a run over a shorter reference first
        if disturb:
            h.set_reference(xref)
            with pytest.raises(L.SmcError, match="error -3.*4 steps"):         # the record is not the reference's length
                h.ancestor_sweep(1)
            for t in (-1, 4):
                with pytest.raises(L.SmcError, match="error -1.*range"):
                    h.history_get_ancestors(t)
            for bad in (-1, n):
                a = h.history_get_ancestors(2)
                a[1, 7] = bad
                with pytest.raises(L.SmcError, match="error -1.*particle"):
                    h.history_put_ancestors(2, a)
        h.reseed(SEED)
        run(h, y, xref)
        res = h.ancestor_sweep(PATH_SEED) + (h.get_reference(),)
        h.close()
        return res

    first = cycle(True)                                                    # (it also fills the cache of recycled bundles)
    gc.collect()
    at = L.live_bytes()
    clean = cycle(False)
    gc.collect()
    assert L.live_bytes() == at, (at, L.live_bytes())
    assert np.array_equal(first[0], clean[0]) and np.array_equal(first[1], clean[1]) and first[2] == clean[2] == 0
    assert TP.same(first[3], clean[3])
    again = cycle(True)
    gc.collect()
    assert L.live_bytes() == at and TP.same(again[3], clean[3])


# ---- f. invariance on the device ------------------------------------------------------------------------------------------------------
def test_particle_gibbs_with_ancestor_sampling_leaves_the_posterior_invariant(L, ob):
    """ParticleGibbs(ancestor_sampling=True), the README LG row, T = 6, 4096 chains of 4 particles started from exact posterior draws,
    4 sweeps, fixed seeds: means, variances and lag-1 covariances within 5 standard errors of the exact smoothed moments
    (conditional_reference.worst_z), no dead filter, and at least 0.9 of the path entries moved (a trace that ignored J moves 0.64)"""
    import sequential_monte_carlo_amd as smc
    chains, Tn = 4096, 6
    _, y = ob.simulate(1, CF.README_LG, Tn, 1998)
    start = CF.exact_posterior_draws(CF.README_LG, y, chains, np.random.default_rng(11))
    pg = smc.ParticleGibbs(4, y, None, reference=start.T, seed=2026, rows=(1, np.tile(CF.README_LG, (chains, 1))), ancestor_sampling=True)
    assert pg.ancestor_sampling and pg._f.h.ancestor_sampling
    for k in range(4):
        path = pg.sweep()
        assert path.shape == (Tn, chains) and pg.kept == 0 and pg.sweeps == k + 1
    z = CF.worst_z(path.T, CF.README_LG, y)
    moved = float(np.mean(path.T != start))
    print("ParticleGibbs with ancestor sampling, 4096 chains x 4 particles, 4 sweeps: worst |z| of means %.2f, variances %.2f, "
          "lag-1 covariances %.2f; moved %.3f" % (z + (moved,)))
    assert max(z) <= 5.0, z
    assert moved >= 0.9, moved
    assert pg.logmu.shape == (Tn, chains) and pg.ess.shape == (Tn, chains)
    pg.close()


# ---- g. the public route is the C route ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,single", [(1, True), (3, False)])
def test_particle_gibbs_sweep_is_the_handles_sweep(L, model, single):
    import sequential_monte_carlo_amd as smc
    from sequential_monte_carlo_amd.particles import _path_seed
    nth, Tn, n = (1 if single else 3), 10, 200
    y, xref = TC.series(model, Tn), TC.references(model, nth, Tn)
    rows = (model, TP.raws_for(model, nth))
    ref = np.moveaxis(xref, 1, -1)                                  # [T][n_theta][d]
    ref = ref[..., 0] if model == 1 else ref
    if single:
        from sequential_monte_carlo_amd.models import LinearModel
        mdl, rows, ref = LinearModel(*TP.RAW[1]), None, ref[:, 0]
    else:
        mdl = None
    pg = smc.ParticleGibbs(n, y, mdl, reference=ref, seed=41, streams=STREAMS[nth], rows=rows, ancestor_sampling=True)
    off = smc.ParticleGibbs(n, y, mdl, reference=ref, seed=41, streams=STREAMS[nth], rows=rows)
    assert pg.ancestor_sampling and not off.ancestor_sampling and not off._f.h.ancestor_sampling
    h = make(L, model, nth, n, 0, seed=pg.sweep_seed(1))
    h.set_reference(xref)
    for k in (1, 2):
        sd = pg.sweep_seed(k)
        h.reseed(sd)
        steps = run(h, y, h.get_reference())
        J, idx, kept = h.ancestor_sweep(_path_seed(sd))
        want = np.moveaxis(h.get_reference(), 1, -1)
        want = want[..., 0] if model == 1 else want
        p = pg.sweep()
        assert p.shape == ref.shape and TP.same(p, want[:, 0] if single else want) and pg.kept == kept == 0 and pg.sweeps == k
        lm = np.array([s[0] for s in steps])
        assert TP.same(pg.logmu, lm[:, 0] if single else lm)
    assert not TP.same(off.sweep(), ref) and off.kept == 0             # the default chain still draws by backward simulation
    h.close()
    pg.close()
    off.close()
