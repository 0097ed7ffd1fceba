"""A whole-series reference for the conditional particle filter (SMC_FLAG_CONDITIONAL) of the bootstrap families with a
transition density (LG1D, SV1D, UCSV3D).  Composed like tests/missing_reference.py from pieces that are pinned on their own, with no
step arithmetic written down here:

  1. the track      ob.ExternalFilter: the oracle's resampler, segmented fixed-point normalisation and time index
  2. ancestors      its draw_ancestors at the filter's time index
  3. normals        ob.state_normals: particle i takes element i & 1 of the pair i >> 1 at (stream, t, SLOT_NORMAL0 + k)
  4. the step       the library's host twin of the whole step, smc_host_filter_steps (tests/test_missing_host.py pins it)
  5. the override   slot k*_t = smc_host_conditional_slot(seed, stream, t, n) takes the reference row xref[t] and the log-weight
                    smc_host_logobs(xref[t], y_t) (tests/test_conditional_host.py pins both); its ancestor is patched to k*_{t-1}
  6. put_step       closes the step

override=False is the same filter without step 5: the control of the invariance tests.  Also here: the exact joint posterior draws
of the linear-Gaussian case (a numpy Kalman backward sampler) and the exact smoothed moments the statistical tests compare against.
"""
import numpy as np

import composed_reference as CR
import missing_reference as MR

LG, SV, UC = 1, 2, 3
ROWS = {LG: 1, SV: 1, UC: 3}
README_LG = MR.README_LG
first_mismatch = CR.first_mismatch


class ConditionalFilter:
    """one filter: init(y0), step(y); xref [T][d]; the traces lm / es / ks (the retained slots), snapshot(); clouds (record=True):
    the (x, w) after every step"""

    def __init__(self, L, ob, model, raw, n, xref, seg=0, seed=1, stream=0, override=True, record=False):
        self.L, self.ob, self.model, self.override = L, ob, model, bool(override)
        self.d, self.n = ROWS[model], int(n)
        self.seed, self.stream = int(seed), int(stream)
        self.f = ob.ExternalFilter(self.d, self.n, seg, self.seed, self.stream, False)
        self.seg, self.nseg = self.f.seg, self.f.nseg
        self.raw = np.array(raw, dtype=np.float64)
        self.xref = np.asarray(xref, dtype=np.float64).reshape(-1, self.d)
        self.t, self.x, self.lm, self.es, self.ks = 0, None, [], [], []
        self.clouds = [] if record else None

    def _advance(self, y, first):
        xp = None if first else np.ascontiguousarray(self.x[:, self.f.draw_ancestors()])
        z = np.stack([self.ob.state_normals(self.seed, self.stream, self.t, self.ob.SLOT_NORMAL0 + k, self.n) for k in range(self.d)])
        x, logw = self.L.host_filter_steps(self.model, self.raw, CR.NONE, None, xp, z, y, first=first)
        if self.override:
            k = self.L.host_conditional_slot(self.seed, self.stream, self.t, self.n)
            x[:, k] = self.xref[self.t]
            logw[k] = self.L.host_logobs(self.model, self.raw, self.xref[self.t], y)
            self.ks.append(k)
        lm, ess = self.f.put_step(x, logw)
        self.x = x
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
        """(x [d][n], w [n], ancestors [n], C, m, S, S2hi, S2lo): the per-filter slices of a handle's state; the retained slot
        descends from the retained slot of the step before (from itself at the first step)"""
        x, w, a, _ = self.f.state()
        if self.override:
            a = a.copy()
            a[self.ks[-1]] = self.ks[-2] if len(self.ks) > 1 else self.ks[-1]
        return (x, w, a) + tuple(self.f.weights_raw())

    def record(self):
        """(x [T][d][n], w [T][n]) of the steps so far"""
        return np.stack([c[0] for c in self.clouds]), np.stack([c[1] for c in self.clouds])


def run_series(L, ob, model, raws, n, seg, seed, y, xrefs, streams=None, override=True):
    """a batched handle's series: xrefs [T][d][n_theta] as the handle takes it, parameter row per filter, stream = the filter's
    index unless streams says otherwise -> dict(lm [T][n_theta], es, snaps = the stacked snapshot after every step, clouds = per
    step (x [d][n_theta][n], w [n_theta][n]), ks [T][n_theta], filters)"""
    raws = np.atleast_2d(np.asarray(raws, dtype=np.float64))
    xrefs = np.asarray(xrefs, dtype=np.float64)
    nth, T = len(raws), len(y)
    lm, es, ks, per, fs = np.zeros((T, nth)), np.zeros((T, nth)), np.zeros((T, nth), dtype=np.int64), [[] for _ in range(T)], []
    for th in range(nth):
        f = ConditionalFilter(L, ob, model, raws[th], n, xrefs[:, :, th], seg=seg, seed=seed, stream=th if streams is None else int(streams[th]),
                              override=override, record=True)
        for t in range(T):
            f.init(y[t]) if t == 0 else f.step(y[t])
            per[t].append(f.snapshot())
        lm[:, th], es[:, th] = f.lm, f.es
        if override:
            ks[:, th] = f.ks
        fs.append(f)
    clouds = [(np.stack([f.clouds[t][0] for f in fs], axis=1), np.stack([f.clouds[t][1] for f in fs])) for t in range(T)]
    return dict(lm=lm, es=es, ks=ks, snaps=[CR.stack(p) for p in per], clouds=clouds, seg=fs[0].seg, nseg=fs[0].nseg, filters=fs)


# ---- the linear-Gaussian case, exactly ---------------------------------------------------------------------------------------------
def exact_posterior_draws(raw, y, count, rng):
    """count joint draws [count][T] from p(x_1:T | y_1:T) of the LG1D row raw = (A, B, Q, R, x0, V0): forward Kalman filter
    (missing_reference.kalman_gaps), then backward sampling x_t | x_{t+1}, y_1:t"""
    A, Q = float(raw[0]), float(raw[2])
    _, mp, Pp, mf, Pf = MR.kalman_gaps(raw, y)
    T = len(mf)
    x = np.zeros((count, T))
    x[:, T - 1] = mf[T - 1] + np.sqrt(Pf[T - 1]) * rng.standard_normal(count)
    for t in range(T - 2, -1, -1):
        G = Pf[t] * A / Pp[t + 1]
        x[:, t] = mf[t] + G * (x[:, t + 1] - mp[t + 1]) + np.sqrt(Pf[t] - G * G * Pp[t + 1]) * rng.standard_normal(count)
    return x


def exact_moments(raw, y):
    """(mean [T], var [T], lag-1 covariance [T - 1]) of p(x_1:T | y_1:T): the RTS smoother (missing_reference.rts_gaps), and
    Cov(x_t, x_{t+1} | y) = G_t Var(x_{t+1} | y) with the smoother gain G_t = Pf_t A / Pp_{t+1}"""
    A = float(raw[0])
    _, mp, Pp, mf, Pf = MR.kalman_gaps(raw, y)
    ms, Ps = MR.rts_gaps(raw, y)
    G = Pf[:-1] * A / Pp[1:]
    return ms, Ps, G * Ps[1:]


def worst_z(paths, raw, y):
    """the worst |z| of a sample of paths [count][T] against the exact posterior, with the standard errors of NORMAL samples from
    the exact moments: means sd / sqrt(K); variances var sqrt(2 / K); lag-1 covariances sqrt((var_t var_{t+1} + cov^2) / K).
    The sample moments are taken about the EXACT means (K terms, no degree of freedom lost).  -> (z mean, z var, z cov)"""
    ms, Ps, Cs = exact_moments(raw, y)
    K = paths.shape[0]
    d = paths - ms
    zm = np.abs(d.mean(axis=0)) / np.sqrt(Ps / K)
    zv = np.abs((d * d).mean(axis=0) - Ps) / (Ps * np.sqrt(2.0 / K))
    zc = np.abs((d[:, :-1] * d[:, 1:]).mean(axis=0) - Cs) / np.sqrt((Ps[:-1] * Ps[1:] + Cs * Cs) / K)
    return float(zm.max()), float(zv.max()), float(zc.max())
