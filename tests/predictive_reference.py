"""Independent references for the predictive checks (csrc/smc_spec.h "predictive checks").  No GPU.

  normcdf_grid()         the inputs every test of sp_normcdf runs over
  mp_normcdf(z)          Phi at 50 digits
  pred_sum(terms)        the order of summation restated over Python floats (plain IEEE adds)
  restated_row(...)      the row of one cloud restated term by term over smc_host_normcdf / smc_host_exp: the bits the library gives
  exact_row(...)         the same row from mpmath terms and math.fsum, with sum |term| of each sum (the scale of the derived bound)
  mp_kalman(...)         the Kalman recursion and its predictive rows at 50 digits
"""
import math
import os
import re

import mpmath as mp
import numpy as np

from sequential_monte_carlo_amd import _lib as L

mp.mp.dps = 50
CH = 128                       # SMOOTH_CH
JOINTS = (0.0, 9.0, -9.0)      # where the pieces of sp_normcdf meet
README_ROW = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
NEAR_UNIT_ROW = [0.999, 1.0, 0.01, 0.5, 0.0, 1.0]


def header_max_err():
    """SP_NORMCDF_MAX_ERR as written beside the function"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sequential_monte_carlo_amd", "csrc", "smc_spec.h")
    with open(path) as f:
        m = re.search(r"SP_NORMCDF_MAX_ERR\s*=\s*([0-9.eE+-]+)\s*;", f.read())
    return float(m.group(1))


def normcdf_grid(with_nan=True):
    z = [np.linspace(-40.0, 40.0, 200001)]
    extra = []
    for j in JOINTS:
        up = dn = j
        extra.append(j)
        for _ in range(4):
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
            extra += [up, dn]
    extra += [0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.0 ** -1022, -2.0 ** -1022, np.inf, -np.inf]
    if with_nan:
        extra.append(np.nan)
    z.append(np.array(extra))
    return np.concatenate(z)


def mp_normcdf(z):
    z = float(z)
    if z != z:
        return mp.nan
    if z == math.inf:
        return mp.mpf(1)
    if z == -math.inf:
        return mp.mpf(0)
    return mp.erfc(-mp.mpf(z) / mp.sqrt(2)) / 2


def pred_sum(terms):
    """chunks of CH in ascending order from +0.0, then the partials CH at a time, until one number is left"""
    level = [float(v) for v in terms]
    while True:
        nxt = []
        for c0 in range(0, len(level), CH):
            s = 0.0
            for v in level[c0:c0 + CH]:
                s += v
            nxt.append(s)
        level = nxt
        if len(level) == 1:
            return level[0]


def _hexp(v):
    return L.lib().smc_host_exp(float(v))


def _terms_restated(model_id, raw, x, y):
    """(Phi(z_i), ym_i, sd_i^2) with the library's own exp and normal CDF, every other operation a Python float operation"""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    n = x.shape[1]
    cdf, ym, s2 = [], [], []
    ncdf = L.lib().smc_host_normcdf
    for i in range(n):
        if model_id == L.MODEL_LG1D:
            sR = math.sqrt(raw[3])
            m, sd = raw[1] * float(x[0, i]), sR
            z = (y - raw[1] * float(x[0, i])) * (1.0 / sR)
        elif model_id == L.MODEL_SV1D:
            m, sd = 0.0, _hexp(0.5 * float(x[0, i]))
            z = y * _hexp(-0.5 * float(x[0, i]))
        else:
            m, sd = float(x[0, i]), _hexp(0.5 * float(x[2, i]))
            z = (y - float(x[0, i])) * _hexp(-0.5 * float(x[2, i]))
        cdf.append(ncdf(float(z)))
        ym.append(m)
        s2.append(sd * sd)
    return cdf, ym, s2


def restated_row(model_id, raw, x, y):
    raw, y = [float(v) for v in raw], float(y)
    cdf, ym, s2 = _terms_restated(model_id, raw, x, y)
    n = float(len(cdf))
    pit = pred_sum(cdf) / n
    mean = pred_sum(ym) / n
    var = pred_sum(s2) / n + pred_sum([(m - mean) * (m - mean) for m in ym]) / n
    return pit, mean, var


def exact_row(model_id, raw, x, y):
    """((pit, mean, var), (sum |Phi|, sum |ym|, sum sd^2 + sum (ym - mean)^2)): mpmath terms from the double inputs, math.fsum"""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    n = x.shape[1]
    y = mp.mpf(float(y))
    cdf, ym, s2 = [], [], []
    for i in range(n):
        x0 = mp.mpf(float(x[0, i]))
        if model_id == L.MODEL_LG1D:
            m, v = mp.mpf(float(raw[1])) * x0, mp.mpf(float(raw[3]))
        elif model_id == L.MODEL_SV1D:
            m, v = mp.mpf(0), mp.exp(x0)
        else:
            m, v = x0, mp.exp(mp.mpf(float(x[2, i])))
        cdf.append(mp.erfc(-((y - m) / mp.sqrt(v)) / mp.sqrt(2)) / 2)
        ym.append(m)
        s2.append(v)
    pit = math.fsum(float(c) for c in cdf) / n
    mean_mp = mp.fsum(ym) / n
    mean = math.fsum(float(m) for m in ym) / n
    cen = [(m - mean_mp) ** 2 for m in ym]
    var = (math.fsum(float(v) for v in s2) + math.fsum(float(c) for c in cen)) / n
    scale = (math.fsum(abs(float(c)) for c in cdf), math.fsum(abs(float(m)) for m in ym),
             math.fsum(float(v) for v in s2) + math.fsum(float(c) for c in cen))
    return (pit, mean, var), scale


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.ndim else a.reshape(1).view(np.uint64),
                                                 b.view(np.uint64) if b.ndim else b.reshape(1).view(np.uint64))


def same_or_both_nan(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return a.shape == b.shape and all((u != u and v != v) or same(u, v) for u, v in zip(a, b))


def mp_kalman(row, y, predict_first=False, missing=False):
    """the recursion of kalman_step at 50 digits: (xf, Sf, pit, ym, yv), lists of mpf (pit NaN at a gap or a NaN y)"""
    A, B, Q, R, x, S = [mp.mpf(float(v)) for v in row]
    xf, Sf, pit, ym, yv = [], [], [], [], []
    for t, yt in enumerate(np.asarray(y, dtype=np.float64)):
        if predict_first or t > 0:
            x, S = A * x, A * A * S + Q
        m, v = B * x, B * B * S + R
        ym.append(m)
        yv.append(v)
        if yt != yt:
            pit.append(mp.nan)
            if not missing:
                x, S = mp.nan, mp.nan
        else:
            yy = mp.mpf(float(yt))
            pit.append(mp.erfc(-((yy - m) / mp.sqrt(v)) / mp.sqrt(2)) / 2)
            K = S * B / v
            x, S = x + K * (yy - m), S - K * K * v
        xf.append(x)
        Sf.append(S)
    return xf, Sf, pit, ym, yv
