"""GPU tests of the batched two-state Kalman filter and RTS smoother (smc_kalman2_log_likelihood, smc_kalman2_smooth;
csrc/smc_kalman2_kernels.h) against the host twins smc_host_kalman2_steps / smc_host_kalman2_smooth: every float64 array
compared bit for bit (NaN == NaN), never approx.  Rows of three kinds are mixed in one call - Hodrick-Prescott (singular Q),
positive definite, and the embedded scalar row whose predicted covariance is singular, so the smoother's NaN rule is hit by one
lane beside healthy ones."""
import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
import kalman2_reference as k2

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 130, 515)     # a lone lane, a full wave, a ragged last wave, several workgroups
STEPS = (1, 2, 37)
Y = k2.hp_series(40)


def mixed_rows(n):
    """row i: HP (i % 3 == 0; lam and init_cov vary), positive definite (1), the embedded scalar row (2)"""
    pd = k2.random_pd_rows(n, seed=13)
    rows = []
    for i in range(n):
        if i % 3 == 0:
            rows.append(k2.hp_row(Y, 100.0 * (1 + i), 1e3 if i % 2 else 1e6))
        elif i % 3 == 1:
            rows.append(pd[i])
        else:
            rows.append(k2.embedded_scalar_row(0.5 + 0.4 * (i % 7) / 7, 1.0 + 0.01 * i, 0.3 + 0.001 * i, 0.8, 0.1, 1.5))
    return np.array(rows)


_HOST = {}


def host(n, T, pf):
    """the host twins of the first n mixed rows, computed once per (T, predict_first) at the largest n"""
    key = (T, pf)
    if key not in _HOST:
        rows = mixed_rows(max(SIZES))
        out, xs, Ps = np.zeros((len(rows), 6)), np.zeros((T, len(rows), 2)), np.zeros((T, len(rows), 3))
        for i, r in enumerate(rows):
            xf, Sf, lik = L.host_kalman2_steps(r, Y[:T], pf)
            z = 0.0
            for v in lik:
                z = z + float(v)
            out[i] = (*xf[-1], *Sf[-1], z)
            xs[:, i], Ps[:, i] = L.host_kalman2_smooth(r, Y[:T], pf)
        _HOST[key] = (out, xs, Ps)
    out, xs, Ps = _HOST[key]
    return out[:n], xs[:, :n], Ps[:, :n]


@pytest.mark.parametrize("predict_first", [False, True])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("n", SIZES)
def test_filter_and_smoother_equal_host_twins(n, T, predict_first):
    rows = mixed_rows(max(SIZES))[:n]
    want, wxs, wPs = host(n, T, predict_first)
    got = L.kalman2_log_likelihood(rows, Y[:T], predict_first)
    assert np.array_equal(got, want, equal_nan=True)
    xs, Ps = L.kalman2_smooth(rows, Y[:T], predict_first)
    assert xs.shape == (T, n, 2) and Ps.shape == (T, n, 3)
    assert np.array_equal(xs, wxs, equal_nan=True) and np.array_equal(Ps, wPs, equal_nan=True)
    if T > 1 and n >= 3:                                  # the singular rule beside healthy lanes
        assert np.all(np.isnan(xs[:-1, 2])) and np.all(np.isfinite(xs[:, 0])) and np.all(np.isfinite(xs[:, 1]))
        assert np.all(np.isfinite(xs[-1]))


def test_python_entry_points_shapes_and_values():
    """log_likelihood_kalman / kalman_smoother on two-state models: shapes with and without the batch axis, the values of the
    C calls, the HP trend through the public path"""
    y = k2.hp_series(60)
    hp = smc.hodrick_prescott(lam=1600, y=y, init_cov=1e6)
    other = smc.MultivariateLinearGaussian(A=[[0.5, 0.1], [-0.2, 0.3]], B=[1.0, 0.5], Q=[[1.0, 0.3], [0.3, 0.5]], R=0.4)
    x, S, z = smc.log_likelihood_kalman(y, hp)
    assert x.shape == (2,) and S.shape == (2, 2) and isinstance(z, float)
    xb, Sb, zb = smc.log_likelihood_kalman(y, [hp, other])
    assert xb.shape == (2, 2) and Sb.shape == (2, 2, 2) and zb.shape == (2,)
    assert np.array_equal(xb[0], x) and np.array_equal(Sb[0], S) and zb[0] == z and np.array_equal(Sb[:, 0, 1], Sb[:, 1, 0])
    raw = L.kalman2_log_likelihood([hp.raw(), other.raw()], y)
    assert np.array_equal(raw[:, 5], zb) and np.array_equal(raw[:, 3], Sb[:, 1, 0])
    xs, Ps = smc.kalman_smoother(y, hp)
    assert xs.shape == (60, 2) and Ps.shape == (60, 2, 2)
    assert np.abs(xs[:, 0] - k2.hp_trend(y, 1600.0)).max() <= 1e-6
    xsb, Psb = smc.kalman_smoother(y, [hp, other], predict_first=True)
    assert xsb.shape == (2, 60, 2) and Psb.shape == (2, 60, 2, 2)
    hx, hP = L.host_kalman2_smooth(other.raw(), y, True)
    assert np.array_equal(xsb[1], hx) and np.array_equal(Psb[1][:, 1, 0], hP[:, 1]) and np.array_equal(Psb[1][:, 1, 1], hP[:, 2])


def test_bad_arguments_are_refused():
    lib = L.lib()
    rows, y, out = mixed_rows(4), Y[:5].copy(), np.zeros((4, 6))
    assert lib.smc_kalman2_log_likelihood(L._d(rows), 0, L._d(y), 5, 0, L._d(out), 0) == -1
    assert lib.smc_kalman2_log_likelihood(L._d(rows), 4, L._d(y), 0, 0, L._d(out), 0) == -1
    assert lib.smc_kalman2_log_likelihood(L._d(rows), 4, L._d(y), 5, 0, L._d(out), 99) == -1
    assert lib.smc_kalman2_smooth(L._d(rows), 4, L._d(y), 5, 0, None, None, 0) == -1
    h = L.C.c_void_p()
    assert lib.smc_create(L.MODEL_LG2D, 1, 256, 0, 1, 0, 0, L.C.byref(h)) == -1
    assert lib.smc_ibis_create_rows(8, 1, 0, 0, 2, L.C.byref(h)) == -1
