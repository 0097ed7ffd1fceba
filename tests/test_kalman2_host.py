"""CPU tests of the two-state exact Kalman side: the host twins smc_host_kalman2_steps / smc_host_kalman2_smooth /
smc_simulate_lg2 - the specification every two-state kernel is compared with bit for bit in test_gpu_kalman2 / test_gpu_ibis2 -
against the extended-precision restatement of src/kalman_filter.jl:3-27 (tests/kalman2_reference.py), the scalar filter, and the
penalised-least-squares Hodrick-Prescott trend; the constructors; the API surface.  No GPU."""
import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
import kalman2_reference as k2

# profiles/kalman2_accuracy.log (scripts/dbg/kalman2_accuracy.py): the measured maxima of (|d logZ| / |logZ|, |d xf|, |d Sf|,
# |d Sf| / max |Sf|) of smc_host_kalman2_steps against numpy longdouble.  The tests assert 16 x these.
MEASURED = {
    "hp init_cov=1000": (1.640e-15, 4.352e-14, 1.645e-13, 8.220e-16),
    "hp init_cov=1e+06": (5.438e-13, 6.748e-11, 2.413e-10, 1.207e-15),
    "pd": (5.494e-16, 1.322e-15, 2.275e-15, 2.357e-15),
}
SLACK = 16.0
# the bound "of (a)" for checks (b) and (c), whose rows are as well conditioned as the positive-definite group
REL_LOGZ, ABS_X, ABS_S, REL_S = (SLACK * v for v in MEASURED["pd"])


def test_twin_against_extended_precision():
    """(a) HP with lam = 1600, init_cov 1e3 and 1e6, T = 200 (the first updates cancel values of the size of init_cov down to
    about 1) and twenty random positive-definite rows, T = 50, both predict_first values: the four figures stay within 16 x the
    maxima measured into profiles/kalman2_accuracy.log"""
    got = k2.measure_accuracy(L.host_kalman2_steps)
    assert set(got) == set(MEASURED)
    for g, v in got.items():
        print("%-18s logZ rel %.3e   xf abs %.3e   Sf abs %.3e   Sf rel %.3e" % ((g,) + v))
    for g, v in got.items():
        for name, a, m in zip(("logZ rel", "xf abs", "Sf abs", "Sf rel"), v, MEASURED[g]):
            assert a <= SLACK * m, (g, name, a, m)


@pytest.mark.parametrize("predict_first", [False, True])
def test_reduction_to_the_scalar_filter(predict_first):
    """(b) A = diag(a, 0), B = (b, 0), Q = diag(q, 0), Sigma0 = diag(s0, 0), x0 = (m, 0) has the likelihood of the LG1D row
    (a, b, q, R, m, s0); the second state and S21, S22 stay exactly 0; the predicted covariance is singular at every step, so
    the smoother reports its documented rule: the last period is the filtered state, every earlier one NaN"""
    a, b, q, R, m, s0 = 0.8, 1.3, 0.7, 0.5, 0.4, 2.0
    y = k2.pd_series(40)
    row = k2.embedded_scalar_row(a, b, q, R, m, s0)
    xf, Sf, lik = L.host_kalman2_steps(row, y, predict_first)
    x1, S1, lik1 = L.host_kalman_steps([a, b, q, R, m, s0], y, predict_first)
    assert np.all(xf[:, 1] == 0.0) and np.all(Sf[:, 1] == 0.0) and np.all(Sf[:, 2] == 0.0)
    print("max |d lik| %.3e (bound %.3e)  |d x| %.3e  |d S| %.3e" % (np.abs(lik - lik1).max(), REL_LOGZ * abs(lik1.sum()), np.abs(xf[:, 0] - x1).max(),
                                                                 np.abs(Sf[:, 0] - S1).max()))
    assert np.abs(lik - lik1).max() <= REL_LOGZ * abs(lik1.sum())
    assert np.abs(xf[:, 0] - x1).max() <= ABS_X and np.abs(Sf[:, 0] - S1).max() <= ABS_S
    xs, Ps = L.host_kalman2_smooth(row, y, predict_first)
    assert np.array_equal(xs[-1], xf[-1]) and np.array_equal(Ps[-1], Sf[-1])
    assert np.all(np.isnan(xs[:-1])) and np.all(np.isnan(Ps[:-1]))


@pytest.mark.parametrize("predict_first", [False, True])
def test_smoother_decoupled_states(predict_first):
    """(c) two decoupled AR(1) states, B = (1, 0), everything positive definite: component 0 of (xs, Ps) is the scalar RTS record
    (smc_host_ibis_smooth) of the first state, component 1 its own unconditional prediction, the cross term 0"""
    a1, a2, q1, q2, R, m1, m2, s1, s2 = 0.85, 0.6, 0.5, 0.3, 0.7, 0.2, -1.1, 1.5, 0.9
    y = k2.pd_series(40)
    row = np.array([a1, 0.0, 0.0, a2, 1.0, 0.0, q1, 0.0, q2, R, m1, m2, s1, 0.0, s2])
    xs, Ps = L.host_kalman2_smooth(row, y, predict_first)
    _, xs1, Ps1 = L.host_ibis_smooth(np.array([[a1, 1.0, q1, R, m1, s1]]), np.zeros(1), y, predict_first, states=True)
    print("|d xs0| %.3e  |d Ps0| %.3e" % (np.abs(xs[:, 0] - xs1[:, 0]).max(), np.abs(Ps[:, 0] - Ps1[:, 0]).max()))
    assert np.abs(xs[:, 0] - xs1[:, 0]).max() <= ABS_X and np.abs(Ps[:, 0] - Ps1[:, 0]).max() <= ABS_S
    mu, v, want_x, want_P = np.longdouble(m2), np.longdouble(s2), [], []
    for t in range(len(y)):
        if t > 0 or predict_first:
            mu, v = a2 * mu, a2 * a2 * v + q2
        want_x.append(mu)
        want_P.append(v)
    assert np.abs(xs[:, 1] - np.array(want_x)).max() <= ABS_X and np.abs(Ps[:, 2] - np.array(want_P)).max() <= ABS_S
    assert np.abs(Ps[:, 1]).max() <= ABS_S
    rx, rP = k2.smooth_ld(row, y, predict_first)
    assert np.abs(xs - rx).max() <= ABS_X and np.abs(Ps - rP).max() <= ABS_S


@pytest.mark.parametrize("predict_first", [False, True])
def test_hodrick_prescott_identity(predict_first):
    """(c) the smoothed first state of hodrick_prescott(lam = 1600, init_cov = 1e6) is the penalised-least-squares trend
    (I + lam D'D)^-1 y to 1e-6 (the difference falls as 1 / init_cov: 7.9e-8 / 9.9e-8 at 1e6 in binary64 numpy, so the bound
    leaves 10 x for another order of operations)"""
    y = k2.hp_series(60)
    xs, _ = L.host_kalman2_smooth(smc.hodrick_prescott(lam=1600, y=y, init_cov=1e6).raw(), y, predict_first)
    d = np.abs(xs[:, 0] - k2.hp_trend(y, 1600.0)).max()
    print("HP identity, predict_first=%s: %.3e" % (predict_first, d))
    assert d <= 1e-6


def test_constructors_refuse():
    """(d) every refusal of the constructors"""
    ok = dict(A=[[0.5, 0.1], [0.0, 0.3]], B=[[1.0, 0.0]], Q=[[1.0, 0.2], [0.2, 0.5]], R=[1.0])
    smc.MultivariateLinearGaussian(**ok)
    bad = [
        (dict(ok, A=np.eye(3) * 0.5, B=[[1.0, 0.0, 0.0]], Q=np.eye(3)), "state dimension 3"),
        (dict(ok, A=[[0.5]], B=[[1.0]], Q=[[1.0]]), "state dimension 1"),
        (dict(ok, B=[[1.0, 0.0], [0.0, 1.0]], R=np.eye(2)), "observation dimension 2"),
        (dict(ok, Q=[[1.0, 0.2], [0.1, 0.5]]), "Q is not symmetric"),
        (dict(ok, Sigma0=[[1.0, 0.2], [0.1, 0.5]]), "Sigma0 is not symmetric"),
        (dict(ok, Q=[[1.0, 2.0], [2.0, 1.0]]), "Q is not positive semi-definite"),
        (dict(ok, Sigma0=[[-1.0, 0.0], [0.0, 1.0]]), "Sigma0 is not positive semi-definite"),
        (dict(ok, R=[0.0]), "R is a variance"),
        (dict(ok, R=[-1.0]), "R is a variance"),
        (dict(ok, A=[[np.nan, 0.1], [0.0, 0.3]]), "not finite"),
        (dict(ok, X0=[np.inf, 0.0]), "not finite"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            smc.MultivariateLinearGaussian(**kw)
    smc.MultivariateLinearGaussian(**dict(ok, Q=[[1.0, 0.0], [0.0, 0.0]]))          # singular is fine
    smc.MultivariateLinearGaussian(**dict(ok, Q=[[1.0, 1.0], [1.0, 1.0]]))


def test_hodrick_prescott_row_and_defaults():
    """(d) hodrick_prescott gives the reference's literal row; MultivariateLinearGaussian the reference's defaults"""
    y = k2.hp_series(10)
    m = smc.hodrick_prescott(lam=1600, y=y)
    assert m.model_id == L.MODEL_LG2D == 16 and m.dim == 2
    assert m.raw() == [2.0, -1.0, 1.0, 0.0, 1.0, 0.0, 1 / 1600, 0.0, 0.0, 1.0, 3 * y[0] - 2 * y[1], 2 * y[0] - y[1], 1000.0, 0.0, 1000.0]
    assert np.array_equal(m.raw(), k2.hp_row(y, 1600.0, 1000.0))
    d = smc.MultivariateLinearGaussian(A=[[0.5, 0.1], [0.0, 0.3]], B=[1.0, 0.5], Q=np.eye(2), R=2.0)
    assert d.raw() == [0.5, 0.1, 0.0, 0.3, 1.0, 0.5, 1.0, 0.0, 1.0, 2.0, 0.0, 0.0, 1.0, 0.0, 1.0]


def test_simulate_is_the_restated_recursion():
    """(d) simulate is reproducible, and equals the recursion restated on its own normals (Philox slots SLOT_NORMAL0,
    SLOT_NORMAL0 + 1 and SLOT_OBS of stream SIM_STREAM; the lower factor of a singular covariance)"""
    import ctypes as C
    lib = L.lib()
    u32 = C.c_uint32 * 4

    def normal(seed, t, slot):                              # box_muller(draw(seed, 0, SIM_STREAM, t, slot)), first output
        ctr, key, out = u32(0, 0xFFFFFFFF, t, slot), (C.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32), u32()
        lib.smc_host_philox4x32_10(ctr, key, out)
        z0, z1 = C.c_double(), C.c_double()
        lib.smc_host_box_muller(out, C.byref(z0), C.byref(z1))
        return z0.value

    def factor(c11, c21, c22):
        l11 = np.sqrt(c11)
        l21 = c21 / l11 if c11 > 0 else 0.0
        return l11, l21, np.sqrt(max(c22 - l21 * l21, 0.0))

    y0 = k2.hp_series(10)
    for model in (smc.hodrick_prescott(lam=4.0, y=y0, init_cov=2.0),
                  smc.MultivariateLinearGaussian(A=[[0.5, 0.1], [-0.2, 0.3]], B=[1.0, 0.5], Q=[[1.0, 0.3], [0.3, 0.5]], R=0.4, X0=[1.0, -1.0],
                                                 Sigma0=[[2.0, -0.5], [-0.5, 1.0]])):
        x, y = smc.simulate(model, 30, seed=77)
        x2, y2 = smc.simulate(model, 30, seed=77)
        assert x.shape == (30, 2) and y.shape == (30,) and np.array_equal(x, x2) and np.array_equal(y, y2)
        assert not np.array_equal(y, smc.simulate(model, 30, seed=78)[1])
        r = model.raw()
        want_x, want_y = np.zeros((30, 2)), np.zeros(30)
        xa = xb = 0.0
        for t in range(30):
            z0, z1, e = normal(77, t, 1), normal(77, t, 2), normal(77, t, 8)
            if t == 0:
                (l11, l21, l22), m1, m2 = factor(r[12], r[13], r[14]), r[10], r[11]
            else:
                (l11, l21, l22), m1, m2 = factor(r[6], r[7], r[8]), r[0] * xa + r[1] * xb, r[2] * xa + r[3] * xb
            xa, xb = m1 + l11 * z0, m2 + l21 * z0 + l22 * z1
            want_x[t], want_y[t] = (xa, xb), r[4] * xa + r[5] * xb + np.sqrt(r[9]) * e
        scale = max(1.0, np.abs(want_x).max())
        assert np.abs(x - want_x).max() <= 64 * np.finfo(float).eps * scale * 30 and np.abs(y - want_y).max() <= 64 * np.finfo(float).eps * scale * 30
    # the singular transition of hodrick_prescott: the second state is the first one lagged, exactly
    x, _ = smc.simulate(smc.hodrick_prescott(lam=4.0, y=y0, init_cov=2.0), 30, seed=77)
    assert np.array_equal(x[1:, 1], x[:-1, 0])


def test_kalman_entry_points_type_rules():
    """(e) a list holds one kind only; missing=True raises for a two-state model; junk is a TypeError (all before any device call)"""
    y = k2.hp_series(10)
    hp, lg = smc.hodrick_prescott(lam=1600, y=y), smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=1.0, R=1.0)
    for fn in (smc.log_likelihood_kalman, smc.kalman_smoother):
        with pytest.raises(TypeError, match="one kind"):
            fn(y, [hp, lg])
        with pytest.raises(TypeError):
            fn(y, [hp, "x"])
        with pytest.raises(ValueError, match="scalar LinearModel only"):
            fn(y, hp, missing=True)


def test_particle_entry_points_refuse():
    """(e) the particle-filter entry points raise a TypeError that names log_likelihood_kalman and IBIS (before any device call)"""
    y = k2.hp_series(10)
    hp = smc.hodrick_prescott(lam=1600, y=y)
    tmap = smc.ThetaMap(L.MODEL_LG2D, [-1] * 6 + [0] + [-1] * 8, hp.raw())
    prior = smc.product_distribution([smc.LogNormal()])
    calls = [lambda: smc.bootstrap_filter(64, y, hp), lambda: smc.particle_filter(64, y, hp), lambda: smc.log_likelihood(64, y, hp),
             lambda: smc.smoother(64, y, hp), lambda: smc.models.params_matrix([hp]),
             lambda: smc.SMC(8, 64, lambda th: hp, prior, 2, 0.5, theta_map=tmap)]
    for call in calls:
        with pytest.raises(TypeError) as e:
            call()
        assert "log_likelihood_kalman" in str(e.value) and "IBIS" in str(e.value)


def test_ibis_accepts_the_two_state_map_and_names_its_limits():
    """(e) IBIS takes ThetaMap(MODEL_LG2D, raw_from[15], raw_const[15]); missing=True, summaries and the scalar-only reductions
    raise a ValueError that says so.  No device call is made: the initial cloud is read from the host."""
    y = k2.hp_series(10)
    hp = smc.hodrick_prescott(lam=1600, y=y)
    tmap = smc.ThetaMap(L.MODEL_LG2D, [-1] * 6 + [0] + [-1] * 8, hp.raw())
    prior = smc.product_distribution([smc.LogNormal()])
    model = lambda th: smc.hodrick_prescott(lam=1 / th[0], y=y)
    ib = smc.IBIS(16, model, prior, 3, 0.5, theta_map=tmap)
    assert ib.two_state and ib.x.shape == (16, 2) and ib.Sigma.shape == (16, 2, 2)
    assert np.array_equal(ib.x, np.tile(hp.X0, (16, 1))) and np.array_equal(ib.Sigma, np.tile(hp.Sigma0, (16, 1, 1)))
    with pytest.raises(ValueError, match="scalar LinearModel only"):
        smc.IBIS(16, model, prior, 3, 0.5, theta_map=tmap, missing=True)
    with pytest.raises(ValueError, match="15 row entries"):
        smc.IBIS(16, model, prior, 3, 0.5, theta_map=smc.ThetaMap(L.MODEL_LG2D, [0, -1, -1, -1, -1, -1], [0.0] * 6))
    for call in (lambda: ib.set_summaries(True), lambda: smc.smc2_run(ib, y, 2, 5, summaries=True), lambda: smc.observation_dist(ib),
                 lambda: smc.estimated_trend(ib), lambda: smc.quantile(ib, 0.5), lambda: smc.filtered_state(ib),
                 lambda: smc.rts_smoothed_state(ib, y), lambda: smc.rts_quantile(ib, y, 0.5), lambda: smc.rts_smoothed_paths(ib, y, 4)):
        with pytest.raises(ValueError, match="scalar LinearModel only"):
            call()
    assert ib._h is None


def test_exports_and_refused_ids():
    """the new symbols are exported; the row id is no particle-filter family (smc_model_dim / smc_model_nraw / smc_simulate)"""
    lib = L.lib()
    for name in ("smc_kalman2_log_likelihood", "smc_kalman2_smooth", "smc_host_kalman2_steps", "smc_host_kalman2_smooth", "smc_simulate_lg2",
                 "smc_ibis_create_rows"):
        assert name in L.EXPORTS and getattr(lib, name)
    assert lib.smc_model_dim(L.MODEL_LG2D) == -1 and lib.smc_model_nraw(L.MODEL_LG2D) == -1
    assert lib.smc_simulate_dim(L.MODEL_LG2D) == -1
    assert lib.smc_simulate(L.MODEL_LG2D, L._d(np.zeros(15)), 5, 1, None, L._d(np.zeros(5))) == -1
