"""A whole-series reference for filters that read a NaN observation as a missing one (SMC_FLAG_NAN_MISSING), for
every family (LG1D, SV1D, UCSV3D, marginal UCSV), the three proposals and both resamplers.  Composed like
tests/composed_reference.py from pieces that are pinned on their own, with no step arithmetic written down here:

  1. the track      ob.ExternalFilter: the oracle's resampler, segmented fixed-point normalisation and time index
  2. ancestors      its draw_ancestors at the filter's time index (at a gap too: the resampling is the ordinary step's)
  3. normals        ob.state_normals: particle i takes element i & 1 of the pair i >> 1 at (stream, t, SLOT_NORMAL0 + k)
  4. the step       the library's host twin of the whole step, smc_host_filter_steps: with a finite y the ordinary step
                    (tests/test_missing_host.py pins it to ob.Filter and to composed_reference), with a NaN y the missing step
  5. put_step       closes the step: at a gap it normalises n log-weights +0.0

Also here: the exact references of the linear-Gaussian case with skipped updates (a numpy Kalman filter and RTS smoother).
"""
import numpy as np

import composed_reference as CR

NONE, AFFINE, OPTIMAL = CR.NONE, CR.AFFINE, CR.OPTIMAL
LG, SV, UC, RB = 1, 2, 3, 4
ROWS = {LG: 1, SV: 1, UC: 3, RB: 4}
NORMALS = {LG: 1, SV: 1, UC: 3, RB: 2}
# the eight gaps of the statistical tests in a series of 40: first, last, a double and a triple included
GAPS40 = (0, 5, 6, 13, 20, 21, 22, 39)
README_LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]


class MissingFilter:
    """one filter: init(y0), step(y); the traces lm / es, logZ as the running sum in step order, snapshot(); clouds (record=True):
    the (x, w) after every step"""

    def __init__(self, L, ob, model, raw, n, seg=0, seed=1, stream=0, kind=NONE, par=None, systematic=False, missing=True, record=False):
        assert kind == NONE or (model == LG and kind in (AFFINE, OPTIMAL)) or (model == UC and kind == OPTIMAL)
        self.L, self.ob, self.model, self.kind, self.missing = L, ob, model, kind, bool(missing)
        self.d, self.nz, self.n = ROWS[model], NORMALS[model], int(n)
        self.seed, self.stream = int(seed), int(stream)
        self.f = ob.ExternalFilter(self.d, self.n, seg, self.seed, self.stream, systematic)
        self.seg, self.nseg = self.f.seg, self.f.nseg
        self.raw = np.array(raw, dtype=np.float64)
        self.par = None if par is None else np.array(par, dtype=np.float64)
        assert (kind == AFFINE) == (self.par is not None)
        self.t, self.x, self.logZ, self.lm, self.es = 0, None, 0.0, [], []
        self.clouds = [] if record else None

    def _advance(self, y, first):
        xp = None if first else np.ascontiguousarray(self.x[:, self.f.draw_ancestors()])
        z = np.stack([self.ob.state_normals(self.seed, self.stream, self.t, self.ob.SLOT_NORMAL0 + k, self.n) for k in range(self.nz)])
        x, logw = self.L.host_filter_steps(self.model, self.raw, self.kind, self.par, xp, z, y, first=first, missing=self.missing)
        lm, ess = self.f.put_step(x, logw)
        self.x = x
        self.logZ = lm if first else self.logZ + lm
        self.t += 1
        self.lm.append(lm)
        self.es.append(ess)
        if self.clouds is not None:
            self.clouds.append((x.copy(), self.f.state()[1].copy()))
        return lm, ess

    def init(self, y0):
        assert self.t == 0
        return self._advance(float(y0), True)

    def step(self, y):
        return self._advance(float(y), False)

    def snapshot(self):
        """(x [d][n], w [n], ancestors [n], C, m, S, S2hi, S2lo): the per-filter slices of a handle's state"""
        x, w, a, _ = self.f.state()
        return (x, w, a) + tuple(self.f.weights_raw())


def run_series(L, ob, model, raws, n, seg, seed, y, kind=NONE, pars=None, systematic=False, streams=None, missing=True, every=False):
    """a batched handle's series: parameter row (and proposal row) per filter, stream = the filter's index unless streams says
    otherwise -> dict(lm [T][n_theta], es [T][n_theta], logZ [n_theta], snap = stacked snapshot after the last step; every=True:
    snaps = the stacked snapshot after every step)"""
    raws = np.atleast_2d(np.asarray(raws, dtype=np.float64))
    nth, T = len(raws), len(y)
    lm, es, logZ, per = np.zeros((T, nth)), np.zeros((T, nth)), np.zeros(nth), [[] for _ in range(T)]
    fs = []
    for th in range(nth):
        f = MissingFilter(L, ob, model, raws[th], n, seg=seg, seed=seed, stream=th if streams is None else int(streams[th]), kind=kind,
                          par=None if pars is None else np.atleast_2d(pars)[th], systematic=systematic, missing=missing, record=True)
        for t in range(T):
            f.init(y[t]) if t == 0 else f.step(y[t])
            if every or t == T - 1:
                per[t].append(f.snapshot())
        lm[:, th], es[:, th], logZ[th] = f.lm, f.es, f.logZ
        fs.append(f)
    out = dict(lm=lm, es=es, logZ=logZ, snap=CR.stack(per[T - 1]), seg=f.seg, nseg=f.nseg, filters=fs)
    if every:
        out["snaps"] = [CR.stack(p) for p in per]
    return out


first_mismatch = CR.first_mismatch


def with_gaps(y, gaps):
    y = np.array(y, dtype=np.float64)
    y[list(gaps)] = np.nan
    return y


# ---- the linear-Gaussian case, exactly: x_1 ~ N(x0, V0), x_t = A x_{t-1} + N(0, Q), y_t = B x_t + N(0, R) --------------------------
def kalman_gaps(raw, y, drop=False):
    """raw = (A, B, Q, R, x0, V0) with variances Q, R, V0 (the LG1D row).  The update is skipped where y is NaN (drop=True: those periods are LEFT OUT of the
    series instead - another model).  -> (log-likelihood, predictive mean [T], predictive variance [T], filtered mean, variance)"""
    A, B, Q, R, x0, V0 = (float(v) for v in raw[:6])
    y = np.asarray(y, dtype=np.float64)
    if drop:
        y = y[~np.isnan(y)]
    T = len(y)
    mp, Pp, mf, Pf = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T)
    ll, m, P = 0.0, x0, V0
    for t in range(T):
        if t > 0:
            m, P = A * m, A * A * P + Q
        mp[t], Pp[t] = m, P
        if not np.isnan(y[t]):
            S = B * B * P + R
            e = y[t] - B * m
            ll += -0.5 * (np.log(2 * np.pi * S) + e * e / S)
            K = P * B / S
            m, P = m + K * e, P - K * B * P
        mf[t], Pf[t] = m, P
    return ll, mp, Pp, mf, Pf


def rts_gaps(raw, y):
    """the smoothed mean and variance [T] of the same model (Rauch-Tung-Striebel over kalman_gaps)"""
    A, Q = float(raw[0]), float(raw[2])
    _, mp, Pp, mf, Pf = kalman_gaps(raw, y)
    ms, Ps = mf.copy(), Pf.copy()
    for t in range(len(mf) - 2, -1, -1):
        G = Pf[t] * A / Pp[t + 1]
        ms[t] = mf[t] + G * (ms[t + 1] - mp[t + 1])
        Ps[t] = Pf[t] + G * G * (Ps[t + 1] - Pp[t + 1])
    return ms, Ps
