"""Host mirror of src/kalman_filter.jl for the univariate LinearModel, batched on the GPU.

    log_likelihood_kalman(y, model)   -> (x_T, Sigma_T, logZ)       kalman_filter.jl:55-70
    kalman_smoother(y, model)         -> (xs [T], Ps [T])           the exact RTS smoother over the same filter
    kalman_predictive(y, model)       -> (pit, obs_mean, obs_var)   the one-step predictive law of y_t and its PIT
and of kalman_filter.jl:3-27 for two-state models with a scalar observation (MultivariateLinearGaussian, hodrick_prescott;
DESIGN.md 2n): (x_T [2], Sigma_T [2][2], logZ) and (xs [T][2], Ps [T][2][2]).

`model` may be a list of LinearModels (one lane per parameter row): the O(1)-per-theta inner "filter"
of the IBIS sampler (src/ibis.jl:134-189).  predict_first=True reproduces the reference loop literally
(it predicts before the first update); the default starts from x_1 ~ N(x0, sigma0) like
bootstrap_filter, so that it is the exact value the particle estimate converges to.
"""
import numpy as np

from . import _lib
from .models import LinearModel, LinearModel2D


def _batch(model, who):
    """(single, models, two_state): one model or a list of ONE kind - LinearModel or LinearModel2D"""
    single = isinstance(model, (LinearModel, LinearModel2D))
    models = [model] if single else list(model)
    if (who == "smoother" and not models) or not all(isinstance(m, (LinearModel, LinearModel2D)) for m in models):
        raise TypeError("the Kalman %s needs LinearModel(s) or two-state LinearModel2D(s)" % who)
    two = bool(models) and isinstance(models[0], LinearModel2D)
    if any(isinstance(m, LinearModel2D) != two for m in models):
        raise TypeError("the Kalman %s takes a list of one kind: scalar LinearModels or two-state LinearModel2Ds, not both" % who)
    return single, models, two


def _lower_to_full(S):
    """[..., 3] lower triangles (S11, S21, S22) -> [..., 2, 2]"""
    return np.stack([np.stack([S[..., 0], S[..., 1]], axis=-1), np.stack([S[..., 1], S[..., 2]], axis=-1)], axis=-2)


def _no_gaps(missing, who):
    if missing:
        raise ValueError("%s: missing=True (NaN gaps) is implemented for the scalar LinearModel only" % who)


def log_likelihood_kalman(y, model, predict_first=False, device=0, missing=False):
    """missing=True (opt-in): a NaN in y is a period without an observation - the prediction alone, +0.0 to logZ.
    Two-state models (MultivariateLinearGaussian, hodrick_prescott): (x_T [2], Sigma_T [2][2], logZ), with a leading batch axis
    for a list."""
    single, models, two = _batch(model, "filter")
    if two:
        _no_gaps(missing, "log_likelihood_kalman")
        out = _lib.kalman2_log_likelihood(np.array([m.raw() for m in models]), y, predict_first, device)
        x, S, logZ = out[:, 0:2].copy(), _lower_to_full(out[:, 2:5]), out[:, 5].copy()
        return (x[0], S[0], float(logZ[0])) if single else (x, S, logZ)
    out = _lib.kalman_log_likelihood(np.array([m.raw() for m in models]), y, predict_first, device, missing=missing)
    if single:
        return float(out[0, 0]), float(out[0, 1]), float(out[0, 2])
    return out[:, 0], out[:, 1], out[:, 2]


def kalman_predictive(y, model_or_list, missing=False, predict_first=False, device=0):
    """(pit, obs_mean, obs_var): the exact one-step predictive law of every y_t under a LinearModel, N(B x-, B^2 S- + R) from the
    predicted pair of the Kalman step, and its probability integral transform pit_t = Phi((y_t - obs_mean_t) / sqrt(obs_var_t)):
    iid uniform under a correct model; pit_residuals(pit) are the standardised innovations.  [T] each; for a list
    of LinearModels [T][n], one lane per parameter row (smc_kalman_predictive_flags).  missing=True: at a NaN y the pit is NaN
    beside the forecast of the unobserved y_t.  What a particle filter's predictive=True estimates."""
    single, models, two = _batch(model_or_list, "predictive check")
    if two or not models:
        raise TypeError("kalman_predictive: the scalar LinearModel only (two-state rows have no predictive check yet)")
    pit, ym, yv = _lib.kalman_predictive(np.array([m.raw() for m in models]), y, predict_first, device, missing=missing)
    return (pit[:, 0].copy(), ym[:, 0].copy(), yv[:, 0].copy()) if single else (pit, ym, yv)


def kalman_smoother(y, model, predict_first=False, device=0, missing=False):
    """(xs, Ps): mean and variance of p(x_t | y_1:T) for a LinearModel, [T] each; for a list of LinearModels [T][n], one lane per
    parameter row (smc_kalman_smooth).  predict_first and missing as in log_likelihood_kalman: the smoothed state at a gap is
    the interpolation."""
    single, models, two = _batch(model, "smoother")
    if two:                                    # (xs [T][2], Ps [T][2][2]); for a list [n][T][2] and [n][T][2][2]
        _no_gaps(missing, "kalman_smoother")
        xs, Ps = _lib.kalman2_smooth(np.array([m.raw() for m in models]), y, predict_first, device)
        xs, Ps = np.ascontiguousarray(xs.transpose(1, 0, 2)), _lower_to_full(Ps.transpose(1, 0, 2))
        return (xs[0], Ps[0]) if single else (xs, Ps)
    xs, Ps = _lib.kalman_smooth(np.array([m.raw() for m in models]), y, predict_first, device, missing=missing)
    return (xs[:, 0].copy(), Ps[:, 0].copy()) if single else (xs, Ps)
