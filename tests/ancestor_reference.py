"""References of the ancestor-sampling tests (smc_ancestor_sweep, smc_host_ancestor_sweep), independent of the
library's arithmetic:

    anc_uniform      the 64-bit uniform of the ancestor draw of step t, rebuilt from smc_host_philox4x32_10 alone: counter (0, stream,
                     t, SLOT_ANC = 39), key = the two halves of the seed, word 1 << 32 | word 0
    check_draws      every J_t against the CDF of its draw, paths_reference.step_cdf(model, raw, x[t-1], w[t-1], xref[t]) in
                     np.longdouble: F_{J-1} - tol <= u / 2^64 < F_J + tol with paths_reference.check_indices' own tolerance
    trace            the trace rule in plain Python from J, the ancestor vectors, the last index and smc_host_conditional_slot
    arbitrary_case   a record (paths_reference.recorded_clouds), random valid ancestor vectors and a finite reference near the clouds
    weights_only_draw   the control of the invariance tests: J_t drawn from w_{t-1} alone, the transition density left out
"""
import ctypes as C

import numpy as np

import paths_reference as PR

LD = np.longdouble
SLOT_ANC = 39


def anc_uniform(L, seed, stream, t):
    out = (C.c_uint32 * 4)()
    ctr = (C.c_uint32 * 4)(0, stream & 0xFFFFFFFF, t, SLOT_ANC)
    key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    L.lib().smc_host_philox4x32_10(ctr, key, out)
    return out[1] << 32 | out[0]


def check_draws(L, model, raw, x, w, xref, J, seed, stream):
    """asserts the bound for every t >= 1 and J[0] == -1; returns the largest distance by which a u lies OUTSIDE [F_{J-1}, F_J)"""
    T, n = w.shape
    tol = LD((n + 1) * 2.0 ** -PR.PATH_BITS + 1000 * PR.EPS)
    worst = LD(0)
    assert J[0] == -1 and np.all(J[1:] >= 0) and np.all(J[1:] < n)
    for t in range(1, T):
        F = PR.step_cdf(model, raw, x[t - 1], w[t - 1], xref[t])
        i = int(J[t])
        U = LD(anc_uniform(L, seed, stream, t)) / LD(2) ** 64
        lo = F[i - 1] if i > 0 else LD(0)
        assert lo - tol <= U < F[i] + tol, (model, n, t, i, float(lo), float(U), float(F[i]))
        worst = max(worst, lo - U, U - F[i])
    return float(worst)


def trace(L, J, a, last, seed, stream, n):
    """idx [T] from the last index: idx[t-1] = J[t] where idx[t] is the retained slot k*_t, else a[t][idx[t]]; all -1 when last < 0"""
    T = len(J)
    idx = np.full(T, -1, dtype=np.int64)
    if last < 0:
        return idx
    idx[T - 1] = last
    for t in range(T - 1, 0, -1):
        kstar = L.host_conditional_slot(seed, stream, t, n)
        idx[t - 1] = J[t] if idx[t] == kstar else a[t][idx[t]]
    return idx


def arbitrary_case(L, ob, model, raw, n, T, rng):
    """(x [T][d][n], w [T][n], a [T][n] int32 with row 0 = -1, xref [T][d]): the oracle's clouds, random valid ancestors, and a
    reference that is some particle's state moved a little (finite, arbitrary, within reach of the sources)"""
    x, w = PR.recorded_clouds(L, ob, model, raw, n, T)
    a = rng.integers(0, n, size=(T, n)).astype(np.int32)
    a[0] = -1
    pick = rng.integers(0, n, size=T)
    xref = np.stack([x[t][:, pick[t]] for t in range(T)]) + 0.05 * rng.standard_normal((T, x.shape[1]))
    return x, w, a, xref


def weights_only_draw(L, w_prev, seed, stream, t):
    """the control: the smallest i whose running sum of w_{t-1} passes u / 2^64 - a draw that ignores where the reference sits"""
    U = float(anc_uniform(L, seed, stream, t)) / 2.0 ** 64
    c = np.cumsum(w_prev / w_prev.sum())
    return int(min(np.searchsorted(c, U, side="right"), len(c) - 1))
