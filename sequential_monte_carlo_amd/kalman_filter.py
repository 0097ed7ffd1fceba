"""Host mirror of src/kalman_filter.jl for the univariate LinearModel, batched on the GPU.

    log_likelihood_kalman(y, model)   -> (x_T, Sigma_T, logZ)       kalman_filter.jl:55-70
    kalman_smoother(y, model)         -> (xs [T], Ps [T])           the exact RTS smoother over the same filter

`model` may be a list of LinearModels (one lane per parameter row): the O(1)-per-theta inner "filter"
of the IBIS sampler (src/ibis.jl:134-189).  predict_first=True reproduces the reference loop literally
(it predicts before the first update); the default starts from x_1 ~ N(x0, sigma0) like
bootstrap_filter, so that it is the exact value the particle estimate converges to.
"""
import numpy as np

from . import _lib
from .models import LinearModel


def log_likelihood_kalman(y, model, predict_first=False, device=0, missing=False):
    """missing=True (opt-in): a NaN in y is a period without an observation - the prediction alone, +0.0 to logZ"""
    single = isinstance(model, LinearModel)
    models = [model] if single else list(model)
    if not all(isinstance(m, LinearModel) for m in models):
        raise TypeError("the Kalman filter needs LinearModel(s)")
    out = _lib.kalman_log_likelihood(np.array([m.raw() for m in models]), y, predict_first, device, missing=missing)
    if single:
        return float(out[0, 0]), float(out[0, 1]), float(out[0, 2])
    return out[:, 0], out[:, 1], out[:, 2]


def kalman_smoother(y, model, predict_first=False, device=0, missing=False):
    """(xs, Ps): mean and variance of p(x_t | y_1:T) for a LinearModel, [T] each; for a list of LinearModels [T][n], one lane per
    parameter row (smc_kalman_smooth).  predict_first and missing as in log_likelihood_kalman: the smoothed state at a gap is
    the interpolation."""
    single = isinstance(model, LinearModel)
    models = [model] if single else list(model)
    if not models or not all(isinstance(m, LinearModel) for m in models):
        raise TypeError("the Kalman smoother needs LinearModel(s)")
    xs, Ps = _lib.kalman_smooth(np.array([m.raw() for m in models]), y, predict_first, device, missing=missing)
    return (xs[:, 0].copy(), Ps[:, 0].copy()) if single else (xs, Ps)
