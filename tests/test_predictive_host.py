"""CPU tests of the predictive checks (csrc/smc_spec.h "predictive checks"): sp_normcdf against mpmath at 50 digits,
smc_host_predictive against an independent reference under a DERIVED bound and bit for bit against its restatement in Python
floats, smc_host_kalman_predictive against the recursion in mpmath, and what the Python layer refuses or shapes before any device
call.  References: tests/predictive_reference.py."""
import math

import mpmath as mp
import numpy as np
import pytest

import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
import predictive_reference as ref

U = 2.0 ** -53
SIZES = [1, 2, 127, 128, 129, 1000, 16385]
ROWS = {L.MODEL_LG1D: ref.README_ROW, L.MODEL_SV1D: [-1.0, 0.95, 0.3], L.MODEL_UCSV3D: [0.2, 0.3, 1.0, -1.0, -0.5]}


def cloud(model_id, n, seed):
    rng = np.random.default_rng(seed)
    if model_id == L.MODEL_UCSV3D:
        return np.stack([1.0 + rng.normal(size=n), rng.normal(size=n) - 1.0, 0.7 * rng.normal(size=n) - 0.5])
    return (rng.normal(size=n) - (1.0 if model_id == L.MODEL_SV1D else 0.0)).reshape(1, n)


def test_normcdf_against_mpmath():
    """absolute error at most 1e-15 over the whole line (the contract), at most the number written beside the function (the
    measurement: 1.886e-16 at z = 0.326); the range; the end points"""
    z = ref.normcdf_grid(with_nan=False)
    f = L.host_normcdf(z)
    assert np.all((f >= 0.0) & (f <= 1.0))
    worst, at = mp.mpf(0), None
    for zi, fi in zip(z, f):
        e = abs(mp.mpf(float(fi)) - ref.mp_normcdf(zi))
        if e > worst:
            worst, at = e, zi
    print("sp_normcdf: largest absolute error %s at z = %r" % (mp.nstr(worst, 5), at))
    assert worst <= 1e-15
    assert worst <= ref.header_max_err() <= 1e-15
    fn = L.lib().smc_host_normcdf
    assert ref.same(fn(-math.inf), 0.0) and fn(math.inf) == 1.0 and fn(math.nan) != fn(math.nan)
    assert fn(0.0) == fn(-0.0) and abs(fn(0.0) - 0.5) <= 2 * U
    assert fn(-40.0) == 0.0 and fn(40.0) == 1.0 and fn(5e-324) >= fn(-5e-324)


@pytest.mark.parametrize("model_id", sorted(ROWS))
@pytest.mark.parametrize("n", SIZES)
def test_host_predictive(model_id, n):
    """bit for bit the restatement; within the derived bound of the exact row.  pred_sum has at most 4 levels of at most
    SMOOTH_CH adds: |err| <= (4 SMOOTH_CH + 4) 2^-53 sum |term| for every sum, plus 1e-15 (sp_normcdf) for pit"""
    raw = ROWS[model_id]
    x = cloud(model_id, n, 1000 * model_id + n)
    y = 0.37
    got = L.host_predictive(model_id, raw, x, y)
    assert ref.same(got, ref.restated_row(model_id, raw, x, y))
    (pit, mean, var), (s_cdf, s_ym, s_var) = ref.exact_row(model_id, raw, x, y)
    k = (4 * ref.CH + 4) * U
    print("n %d model %d: errors %.3e %.3e %.3e" % (n, model_id, abs(got[0] - pit), abs(got[1] - mean), abs(got[2] - var)))
    assert abs(got[0] - pit) <= k * s_cdf / n + 1e-15
    assert abs(got[1] - mean) <= k * s_ym / n
    assert abs(got[2] - var) <= k * s_var / n
    assert 0.0 <= got[0] <= 1.0 and got[2] >= 0.0


def test_pred_sum_is_smooth_sum_up_to_two_levels():
    """one chunk: the serial sum; beyond SMOOTH_CH^2 a third level appears (16385 = 128 * 128 + 1 terms: 129 partials, then 2)"""
    t = list(np.random.default_rng(3).normal(size=16385))
    s = 0.0
    for v in t[:128]:
        s += v
    assert ref.pred_sum(t[:128]) == s
    parts = [ref.pred_sum(t[c:c + 128]) for c in range(0, 16385, 128)]
    assert len(parts) == 129 and ref.pred_sum(t) == ref.pred_sum(parts[:128]) + parts[128]
    x = np.array(t).reshape(1, -1)
    assert ref.same(L.host_predictive(L.MODEL_LG1D, ref.README_ROW, x, 0.1)[1], ref.pred_sum(t) / 16385.0)


@pytest.mark.parametrize("y", [math.nan, math.inf, -math.inf])
@pytest.mark.parametrize("model_id", sorted(ROWS))
def test_host_predictive_special_observations(model_id, y):
    """no rule for non-finite values: a NaN y gives a NaN pit beside ordinary moments, an infinite y gives 0 or 1"""
    raw, x = ROWS[model_id], cloud(model_id, 300, 5)
    got = L.host_predictive(model_id, raw, x, y)
    assert ref.same_or_both_nan(got, ref.restated_row(model_id, raw, x, y))
    fin = L.host_predictive(model_id, raw, x, 0.0)
    assert ref.same(got[1:], fin[1:])
    if y != y:
        assert got[0] != got[0]
    else:
        assert got[0] == (1.0 if y > 0 else 0.0)


def test_host_predictive_planted_states():
    """a NaN state poisons what reads it; an SV state of -1500 has sd = 0: z is +-inf, its Phi is 0 or 1, the row stays finite"""
    x = cloud(L.MODEL_LG1D, 200, 9)
    x[0, 77] = math.nan
    got = L.host_predictive(L.MODEL_LG1D, ref.README_ROW, x, 0.2)
    assert all(v != v for v in got)
    u = cloud(L.MODEL_UCSV3D, 200, 9)
    u[2, 5] = math.nan                                    # the log-variance: pit and obs_var read it, obs_mean does not
    got = L.host_predictive(L.MODEL_UCSV3D, ROWS[L.MODEL_UCSV3D], u, 0.2)
    assert got[0] != got[0] and got[1] == got[1] and got[2] != got[2]
    s = cloud(L.MODEL_SV1D, 129, 9)
    s[0, 128] = -1500.0
    for y in (0.3, -0.3):
        got = L.host_predictive(L.MODEL_SV1D, ROWS[L.MODEL_SV1D], s, y)
        assert ref.same(got, ref.restated_row(L.MODEL_SV1D, ROWS[L.MODEL_SV1D], s, y)) and all(math.isfinite(v) for v in got)
    got0 = L.host_predictive(L.MODEL_SV1D, ROWS[L.MODEL_SV1D], s, 0.0)       # 0 * inf: IEEE's NaN, as the formula gives it
    assert got0[0] != got0[0] and got0[1] == 0.0


def _gaps(y):
    y = y.copy()
    y[[3, 4, 17, 59]] = math.nan
    return y


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("row", [ref.README_ROW, ref.NEAR_UNIT_ROW])
def test_host_kalman_predictive(row, gaps):
    """against the recursion at 50 digits, T = 60.  The bound: 4 times the largest error the filtered record of smc_host_kalman_steps
    (xf, Sf) shows against the same recursion - both are the rounding of the same few operations.  Measured on the host over the
    four cases: the record's largest error between 1.96e-16 and 2.90e-16, the rows' largest error (pit, ym, yv together)
    between 1.73e-16 and 2.79e-16 - at most 1.4 times the record's, against the 4 allowed."""
    _, y = L.simulate(L.MODEL_LG1D, row, 60, 11)
    if gaps:
        y = _gaps(y)
    xf, Sf, _ = L.host_kalman_steps(row, y, missing=gaps)
    mxf, mSf, mpit, mym, myv = ref.mp_kalman(row, y, missing=gaps)
    rec = max(max(abs(mp.mpf(float(a)) - b) for a, b in zip(xf, mxf)), max(abs(mp.mpf(float(a)) - b) for a, b in zip(Sf, mSf)))
    assert rec > 0
    pit, ym, yv = L.host_kalman_predictive(row, y, missing=gaps)
    worst = mp.mpf(0)
    for t in range(60):
        if y[t] != y[t]:
            assert pit[t] != pit[t]
        else:
            worst = max(worst, abs(mp.mpf(float(pit[t])) - mpit[t]))
        worst = max(worst, abs(mp.mpf(float(ym[t])) - mym[t]), abs(mp.mpf(float(yv[t])) - myv[t]))
    print("record %s rows %s" % (mp.nstr(rec, 4), mp.nstr(worst, 4)))
    assert worst <= 4 * rec
    # the first step with predict_first = 0 reads (x0, sigma0); the filter behind the rows is the filter that never asked
    assert ym[0] == row[1] * row[4] and yv[0] == row[1] * row[1] * row[5] + row[3]
    p1 = L.host_kalman_predictive(row, y, predict_first=True, missing=gaps)
    assert p1[1][0] == row[1] * (row[0] * row[4])


def test_python_surface():
    lg, sv = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8), smc.StochasticVolatility(-1.0, 0.95, 0.3)
    y = np.linspace(-1.0, 1.0, 5)
    with pytest.raises(ValueError, match="proposal"):
        smc.log_likelihood(64, y, lg, proposal=smc.OptimalProposal(), predictive=True)
    with pytest.raises(ValueError, match="proposal"):
        smc.smoother(64, y, lg, proposal=smc.OptimalProposal(), predictive=True)
    with pytest.raises(ValueError, match="reference"):
        smc.smoother(64, y, lg, reference=np.zeros(5), predictive=True)
    with pytest.raises(TypeError, match="predictive pair"):
        smc.log_likelihood(64, y, smc.MarginalUCSV((0.2, 0.3), 1.0, (-1.0, -0.5)), predictive=True)
    with pytest.raises(ValueError, match="step by step"):
        smc.log_likelihood(64, y, sv, predictive=True, moments=True)
    with pytest.raises(TypeError):
        smc.kalman_predictive(y, sv)
    r = smc.pit_residuals([0.0, 1.0, math.nan, 0.5, 0.975])
    assert r[0] == -math.inf and r[1] == math.inf and r[2] != r[2] and r[3] == 0.0 and abs(r[4] - 1.959963984540054) < 1e-12
    assert smc.pit_residuals(np.full((2, 3), 0.5)).shape == (2, 3)
    small_max, chunk = L.predictive_constants()
    assert chunk == ref.CH and 0 <= small_max <= chunk * chunk
