"""Host mirror of src/ibis.jl: the IBIS sampler - Chopin's SMC² with the exact scalar Kalman filter as the inner "filter" - for
the univariate LinearModel (UnivariateLinearGaussian, unobserved_components), and with the exact two-state filter of
kalman_filter.jl:3-27 for MultivariateLinearGaussian / hodrick_prescott rows (theta_map=ThetaMap(MODEL_LG2D, raw_from[15],
raw_const[15])): the same sampler calls, ib.x [M][2] and ib.Sigma [M][2][2]; gaps, the cloud summaries and the rts_*
calls are scalar-only.

    IBIS(M, model, prior, chain, ess_threshold, min_ar=-1.0)        ibis.jl:26-58
    smc2 / smc2_step / smc2_run, resample_, rejuvenate_, expected_parameters, density_tempered   (smc_samplers.py dispatches here)
    posterior_moments: the weighted mean and covariance of the theta cloud, reduced on the device
    posterior_quantiles, posterior_histogram: weighted quantiles and marginal histograms of the theta cloud, selected on the device
    observation_dist, estimated_trend, quantile (plotting_utils.jl:94-137), filtered_state: reductions over the cloud on the device
    rts_smoothed_state, rts_quantile, rts_smoothed_paths: the exact RTS smoother of every parameter particle, integrated over the
    cloud per period, and trajectories by backward sampling - the smoothed trend and trend paths

A parameter particle owns O(1) state - theta, its model row, (x, Sigma), logZ, logw - and all of it lives on the device for the
life of the sampler (smc_ibis_*, csrc/smc_ibis_kernels.h): an online step is one Kalman update per particle, a window of steps
one launch that also computes the outer reweight's segment records, and rejuvenate! one launch for the whole chain of moves,
re-filters included.  So the cloud can be very large (M = 2^20 is 16 MB of state).  The host keeps what the reference keeps
outside the loop over m: the ESS decision, the index draw of resample! and the random-walk factor (one read of theta per
rejuvenation), all by the library's outer-level routines, as for SMC.

device_moves=True keeps those three on the device as well (smc_ibis_window_ess, smc_ibis_resample, smc_ibis_theta_moments): a
whole smc2_run then reads no array of length M and no record array - per window ess [k] and j, per resample-move d + d^2
doubles and the acceptance count, and the rows of the summaries when they are recorded.  The ESS walk and the index draw are
the same integer functions on both paths, the same bits; the covariance of the random-walk factor is summed in the device's
order (chunks of 64, a tree within, chunks left to right) instead of the host's index order, so after the first rejuvenation
the two paths agree up to that rounding only.  That is why the flag is opt-in; the default makes the calls it always made.

`model` is the reference's closure and is kept for the caller; the device evaluates `theta_map` (ThetaMap to LG1D rows) and a
prior of the enumerated families instead - a GPU cannot call a closure, so both are required.

missing=True (opt-in, as for SMC): a NaN in y is a period without an observation.  Every Kalman step of the sampler - online,
in the re-filters of rejuvenate_ and density_tempered, in the RTS smoother and the paths - is then the missing step at a NaN:
the prediction alone, +0.0 to logZ and logw, so the ESS of a gap is the previous period's and a gap never starts a
resample-move by itself.  Every function of this module reads the flag from the sampler.

predict_first: the reference's smc²(ibis, y) runs kalman_filter on y[1], which predicts before the first update
(kalman_filter.jl:39-40).  As in log_likelihood_kalman the default (False) starts from x_1 ~ N(x0, sigma0), the limit of the
particle filters; True is the literal loop.  The flag holds online and in every re-filter alike, so logZ[m] always equals
log_likelihood_kalman(y[:t], model(theta[m])) with the same flag.
"""
import math
import statistics
import sys

import numpy as np

from . import _lib


_SCALAR_ONLY = ("%s is implemented for the scalar LinearModel only, not for a sampler over two-state rows "
                "(MultivariateLinearGaussian, hodrick_prescott): gaps, cloud summaries and smoothed paths of two-state rows are not "
                "built yet")


def _scalar_only(ibis, what):
    if getattr(ibis, "two_state", False):
        raise ValueError(_SCALAR_ONLY % what)


class IBIS:
    """IBIS(M, model, prior, chain, ess_threshold, min_ar=-1.0)   ibis.jl:3-58.  M parameter particles; theta is drawn exactly
    as SMC draws it (the same cloud for the same seed).  Arrays (theta, x, Sigma, logZ, logw, omega) are read from the device
    on access; no device call is made before the first sampler call."""

    def __init__(self, M, model, prior, chain, ess_threshold, min_ar=-1.0, seed=1, theta_map=None, device=0, predict_first=False,
                 device_moves=False, missing=False):
        self.M, self.model, self.prior, self.chain = int(M), model, prior, int(chain)
        if theta_map is None or getattr(theta_map, "model_id", None) not in (_lib.MODEL_LG1D, _lib.MODEL_LG2D):
            raise TypeError("IBIS needs theta_map=ThetaMap(LG1D rows) or ThetaMap(MODEL_LG2D, two-state rows of 15 entries): the Kalman "
                            "filter inside runs on the GPU, which cannot call the `model` closure, and it is exact for linear "
                            "Gaussian models only")
        self.two_state = theta_map.model_id == _lib.MODEL_LG2D
        if theta_map.raw_from.size != (_lib.LG2_NRAW if self.two_state else 6):
            raise ValueError("theta_map needs %d row entries for this family" % (_lib.LG2_NRAW if self.two_state else 6))
        if self.two_state and missing:
            raise ValueError(_SCALAR_ONLY % "missing=True")
        spec = prior.spec() if hasattr(prior, "spec") else None
        if spec is None:
            raise TypeError("IBIS needs a prior of the enumerated families (Uniform, Normal, TruncatedNormal, LogNormal or their "
                            "product_distribution): the GPU evaluates insupport / logpdf from prior.spec(), not from a closure")
        self.theta_map = theta_map
        self.prior_spec = (np.atleast_1d(np.asarray(spec[0], dtype=np.int32)), np.atleast_2d(np.asarray(spec[1], dtype=np.float64)))
        self.rng = np.random.default_rng(seed)
        self.seed = int(seed)
        if hasattr(prior, "rand_many"):
            self._theta0 = np.ascontiguousarray(prior.rand_many(self.rng, self.M), dtype=np.float64)
        else:
            self._theta0 = np.array([np.atleast_1d(prior.rand(self.rng)) for _ in range(self.M)], dtype=np.float64)
        if self._theta0.shape[1] != len(self.prior_spec[0]) or self._theta0.shape[1] > _lib.MAX_DTHETA:
            raise TypeError("the prior's spec() must describe every component of theta (at most %d)" % _lib.MAX_DTHETA)
        if self.chain > 64:
            raise ValueError("chain <= 64")
        self.device, self.predict_first, self.device_moves = int(device), bool(predict_first), bool(device_moves)
        self.missing = bool(missing)
        self.ess = float(self.M)
        self.ess_min = self.M * float(ess_threshold)
        self.acc_threshold, self.acc_ratio = float(min_ar), 0.0
        self.accepted = np.zeros(self.M, dtype=bool)      # acc_array of the last rejuvenate! (ibis.jl:87)
        self.n_rejuvenations = 0
        self._calls = 0
        self._h = None
        self.t = 0
        self._summ = None              # {"p": levels or None, "ahead": 0 | 1} while every period's summaries are recorded
        self.summary_trace = []        # [(t, y, Sigma, between, xbar, Sbar, quantiles or None)], one entry per period kept

    # -- the device half ------------------------------------------------------------------------------
    def _handle(self):
        if self._h is None:
            fam, par = self.prior_spec
            self._h = _lib.IbisHandle(self.M, self._theta0.shape[1], fam, par, self.theta_map.raw_from, self.theta_map.raw_const,
                                      seed=self.seed, device=self.device, predict_first=self.predict_first,
                                      flags=_lib.FLAG_NAN_MISSING if self.missing else 0,
                                      row_id=_lib.MODEL_LG2D if self.two_state else _lib.MODEL_LG1D)
            self._h.set_theta(self._theta0)
        return self._h

    def close(self):
        if self._h is not None:
            self._keep_accepted()
            self._h.close()
            self._h = None

    def _next_seed(self):
        self._calls += 1
        return (self.seed << 20) + self._calls

    def _get(self, name):
        if self._h is None:                # nothing has run: the initial cloud (ibis.jl:35-43)
            if name == "theta":
                return self._theta0.copy()
            rows = self.theta_map.rows(self._theta0)
            if self.two_state:
                return {"x": rows[:, 10:12].copy(), "S": _full2(rows[:, 12:15])}.get(name, np.zeros(self.M))
            return {"x": rows[:, 4].copy(), "S": rows[:, 5].copy()}.get(name, np.zeros(self.M))
        out = self._h.get(**{name: True})[name]
        return _full2(out) if self.two_state and name == "S" else out      # two-state: x [M][2], Sigma [M][2][2]

    @property
    def accepted(self):
        """acc_array of the last rejuvenate! (ibis.jl:87); with device_moves the mask stays on the device until it is asked for"""
        if self._accepted is None:
            self._accepted = self._h.get_moved() if self._h is not None else np.zeros(self.M, dtype=bool)
        return self._accepted

    def _keep_accepted(self):
        """fetch a mask that is still on the device, before the handle forgets it (close, a new set_theta)"""
        if self._accepted is None and self._h is not None:
            try:
                self._accepted = self._h.get_moved()
            except _lib.SmcError:                          # the handle was reset behind the sampler's back: no mask to keep
                self._accepted = np.zeros(self.M, dtype=bool)

    @accepted.setter
    def accepted(self, value):
        self._accepted = value

    theta = property(lambda self: self._get("theta"))
    x = property(lambda self: self._get("x"))
    Sigma = property(lambda self: self._get("S"))
    logZ = property(lambda self: self._get("logZ"))
    logw = property(lambda self: self._get("logw"))

    @property
    def omega(self):
        """the normalised outer weights (ibis.ω after reweight)"""
        return _lib.host_reweight(self.logw)[1]

    def set_summaries(self, summaries=True, ahead=0):
        """record observation_dist / filtered_state of every period from now on into summary_trace (smc2, smc2_step and
        smc2_run append their periods; on the device, inside the step's launch).  summaries: True, a list of quantile levels,
        or None / False to switch the recording off."""
        if summaries is None or summaries is False:
            self._summ = None
        else:
            _scalar_only(self, "summaries=")
            if ahead not in (0, 1):
                raise ValueError("ahead is 0 (the filtered observation) or 1 (the one-step forecast)")
            self._summ = {"p": None if summaries is True else [float(v) for v in np.atleast_1d(summaries)], "ahead": int(ahead)}
        return self

    def __repr__(self):
        w = self.omega
        return "ess     = %.3f\nmean(theta) = %s" % (self.ess, np.array2string((self.theta * w[:, None]).sum(axis=0)))


def _full2(S):
    """[M][3] lower triangles (S11, S21, S22) -> [M][2][2]"""
    S = np.asarray(S)
    return np.stack([np.stack([S[:, 0], S[:, 1]], axis=-1), np.stack([S[:, 1], S[:, 2]], axis=-1)], axis=-2)


def _window(ibis, y, ess_min, t=None):
    """k = len(y) steps of smc²! in one launch; the host walks the k x nseg records the device computed and keeps the steps up to
    the first whose ESS is below ess_min -> (ess [j], j).  With summaries switched on the same launch records every step's row
    and the rows of the j kept steps (periods t .. t + j - 1) go to summary_trace: the dropped steps are redone by a later
    window, which records them then."""
    h = ibis._handle()
    summ = ibis._summ if t is not None else None
    want = (summ is not None, summ["ahead"] if summ else 0)
    if want != getattr(h, "_recording", (False, 0)):       # (a run without summaries makes the calls it made before)
        h.set_summaries(*want)
        h._recording = want
    if ibis.device_moves:
        ess, j = h.window_ess(y, ess_min)                  # the same walk, on three integers per step reduced on the device
    else:
        rec, _ = h.window(y)
        ess, j = _lib.host_outer_walk(rec, ibis.M, ess_min)
    if summ is not None:
        for i, r in enumerate(h.get_summaries(j)):
            q = None if summ["p"] is None else _normal_quantiles(r[0], r[1], summ["p"])
            ibis.summary_trace.append((t + i, float(r[0]), float(r[1]), float(r[2]), float(r[3]), float(r[4]), q))
    h.commit(j)
    return ess, j


def _summary(ibis, ahead=0):
    """(y, Sigma, between, xbar, Sbar, between_x, K, D): smc_ibis_summary on the resident cloud; before the first sampler call
    the same specification on the host (smc_host_ibis_summary) over the initial cloud - no device call"""
    _scalar_only(ibis, "observation_dist / estimated_trend / quantile / filtered_state")
    if ahead not in (0, 1):
        raise ValueError("ahead is 0 (the filtered observation) or 1 (the one-step forecast)")
    if ibis._h is None:
        rows = ibis.theta_map.rows(ibis._theta0)
        return _lib.host_ibis_summary(rows, rows[:, 4], rows[:, 5], np.zeros(ibis.M), ahead)
    return ibis._h.summary(ahead)


def observation_dist(ibis, ahead=0, between=False):
    """observation_dist(ibis)   plotting_utils.jl:94-112 -> (y, Sigma) = (sum omega B x, sum omega (B Sigma_m B' + R)), reduced on
    the device.  ahead=1: after one Kalman prediction per particle (the one-step forecast; :126-127).  between=True adds
    sum omega (ym - y)^2, the spread of the component means that the reference's Sigma leaves out: Sigma + between is the variance
    of the mixture."""
    r = _summary(ibis, ahead)
    return (float(r[0]), float(r[1]), float(r[2])) if between else (float(r[0]), float(r[1]))


def estimated_trend(ibis):
    """estimated_trend(ibis) = observation_dist(ibis)[1]   plotting_utils.jl:114 (1-based there: the mean)"""
    return observation_dist(ibis)[0]


def filtered_state(ibis):
    """(xbar, Sbar, between) = (sum omega x, sum omega Sigma_m, sum omega (x - xbar)^2): the filtered state of the mixture"""
    r = _summary(ibis, 0)
    return float(r[3]), float(r[4]), float(r[5])


def _normal_quantiles(mean, var, p):
    """quantile(Normal(mean, sqrt(var)), p) for the levels p in ascending order (a copy is sorted), on the host"""
    out = np.empty(len(p))
    for i, v in enumerate(sorted(p)):
        if not 0.0 <= v <= 1.0:
            raise ValueError("quantile levels lie in [0, 1]")
        if not (math.isfinite(mean) and var >= 0.0 and math.isfinite(var)):
            out[i] = math.nan
        elif v in (0.0, 1.0) or var == 0.0:
            out[i] = mean if var == 0.0 else (-math.inf if v == 0.0 else math.inf)
        else:
            out[i] = statistics.NormalDist(mean, math.sqrt(var)).inv_cdf(v)
    return out


def quantile(ibis, p, ahead=0, total=False):
    """quantile(ibis, p)   plotting_utils.jl:128-137: the quantiles of Normal(y, sqrt(Sigma)), (y, Sigma) = observation_dist(ibis,
    ahead), at the levels p in ascending order.  The caller's p is left as it is (the reference sorts it in place, :132).
    total=True: Normal(y, sqrt(Sigma + between)), the moment-matched normal of the mixture.  A scalar p gives a float."""
    y, S, b = observation_dist(ibis, ahead, between=True)
    q = _normal_quantiles(y, S + b if total else S, [float(v) for v in np.atleast_1d(p)])
    return float(q[0]) if np.ndim(p) == 0 else q


_U64 = 0xFFFFFFFFFFFFFFFF
_RTS_COLUMNS = ("y", "Sigma", "between", "xbar", "Sbar", "between_x")


def _rts_rows(ibis, y):
    """out [T][8] of smc_ibis_smooth on the resident cloud; before the first sampler call the host twin over the initial cloud"""
    _scalar_only(ibis, "rts_smoothed_state / rts_quantile")
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    if y.size < 1:
        raise ValueError("y must hold at least one observation")
    if ibis._h is None:
        return _lib.host_ibis_smooth(ibis.theta_map.rows(ibis._theta0), np.zeros(ibis.M), y, ibis.predict_first, missing=ibis.missing)
    return ibis._h.smooth(y)


def rts_smoothed_state(ibis, y, parts=False):
    """(mean [T], var [T]) of p(x_t | y_1:T) integrated over the sampler's current parameter cloud, exactly: the RTS smoother of
    every parameter particle over y (a Kalman re-filter from (x0, sigma0) and one backward recursion, O(T) per particle) and one
    reduction over the cloud per period, all on the device (smc_ibis_smooth).  mean = sum omega xs_m = xbar and var = Sbar +
    between_x, within plus between, as smoothed_state combines a mixture.  parts=True: a dict of the six columns per period,
    y, Sigma, between (the smoothed fitted observation B x, as observation_dist names them) and xbar, Sbar, between_x.
    y is the caller's series (the sampler keeps none): pass the observations the cloud has seen, y[:ibis.t].  The sampler is
    not changed."""
    r = _rts_rows(ibis, y)
    if parts:
        return {name: r[:, i].copy() for i, name in enumerate(_RTS_COLUMNS)}
    return r[:, 3].copy(), r[:, 4] + r[:, 5]


def rts_quantile(ibis, y, p, total=True):
    """quantiles of the smoothed state per period, [T][len(p)] at the levels p in ascending order ([T] for a scalar p; the caller's
    p is left as it is, as in quantile(ibis, p)): of Normal(xbar_t, sqrt(Sbar_t + between_x_t)), the moment-matched normal of the
    mixture (total=True), or of Normal(xbar_t, sqrt(Sbar_t)) (total=False)."""
    r = _rts_rows(ibis, y)
    levels = [float(v) for v in np.atleast_1d(p)]
    q = np.array([_normal_quantiles(float(row[3]), float(row[4] + row[5]) if total else float(row[4]), levels) for row in r])
    return q[:, 0].copy() if np.ndim(p) == 0 else q


def rts_smoothed_paths(ibis, y, M, seed=None):
    """M trajectories [T][M] from p(x_1:T | y_1:T) integrated over the sampler's current parameter cloud: the parameter particle of
    every path is drawn from omega through the library's own outer resampler (host_outer_resample(logw, M, seed + 1): ascending,
    exactly as smoothed_paths draws them; particles with omega = 0 are never drawn), and every path is drawn exactly by backward
    sampling under its particle's row (smc_ibis_sample_paths, Philox seed + 2).  seed: default derived from the sampler's seed;
    the sampler's own rng and state are not touched."""
    _scalar_only(ibis, "rts_smoothed_paths")
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    M = int(M)
    if M < 1:
        raise ValueError("M must be positive")
    if y.size < 1:
        raise ValueError("y must hold at least one observation")
    seed = (((ibis.seed << 20) | 0x4754B) if seed is None else int(seed)) & _U64
    which = np.asarray(_lib.host_outer_resample(ibis.logw, M, (seed + 1) & _U64), dtype=np.int32)
    if ibis._h is None:
        return _lib.host_ibis_sample_paths(ibis.theta_map.rows(ibis._theta0), y, which, (seed + 2) & _U64, ibis.predict_first,
                                           missing=ibis.missing)
    return ibis._h.sample_paths(y, which, (seed + 2) & _U64)


def smc2(ibis, y):
    """smc²(ibis, y)   ibis.jl:134-147"""
    y = np.asarray(y, dtype=np.float64)
    h = ibis._handle()
    if ibis.t != 0:
        ibis._keep_accepted()
        h.set_theta(ibis.theta)           # again from (x0, sigma0), logZ = logw = 0
    ibis.summary_trace = []
    ess, _ = _window(ibis, y[:1], 0.0, 1)
    ibis.ess = float(ess[0])
    ibis.t = 1
    return ibis


def resample_(ibis, logw=None):
    """resample!(ibis)   ibis.jl:73-84 - value copies (the reference's aliasing of equal ancestors is not inherited).
    With device_moves the draw and the gather stay on the device (given log-weights are set first) and None is returned."""
    if ibis.device_moves:
        if logw is not None:
            ibis._handle().set_logw(logw)
        ibis._handle().resample(ibis._next_seed())
        return None
    lw = ibis.logw if logw is None else logw
    a = np.asarray(_lib.host_outer_resample(lw, ibis.M, ibis._next_seed()), dtype=np.int32)
    ibis._handle().permute(a)
    return a


def rejuvenate_(ibis, y, xi=1.0, verbose=False, out=sys.stdout):
    """rejuvenate!(ibis, y, xi, verbose)   ibis.jl:86-125 in one launch"""
    from .smc_samplers import random_walk_factor
    y = np.asarray(y, dtype=np.float64)
    if verbose:
        out.write("\t[rejuvenating]")
    scales = 0.5 * np.arange(ibis.chain, 0, -1)                                     # 0.5*reverse(1:chain)
    if ibis.device_moves:                                  # ibis.kernel(ibis.θ) from d + d^2 doubles: the covariance summed on the device
        if ibis.M < 2:
            raise ValueError("rejuvenate_ needs M >= 2: the covariance of one parameter particle is undefined")
        L, uni = _lib.host_rw_factor_cov(ibis._handle().theta_moments(weighted=False)[1])
        s = scales * scales if uni else scales
    else:
        L, s = random_walk_factor(ibis.theta, scales)                               # ibis.kernel(ibis.θ)
    n, ibis.accepted = ibis._handle().rejuvenate(y, float(xi), L, s, ibis._next_seed(), want_moved=not ibis.device_moves)
    ibis.acc_ratio = float(n) / ibis.M
    ibis.n_rejuvenations += 1
    if verbose:
        out.write("\tacc_rate: %1.5f" % ibis.acc_ratio)
    return ibis


def smc2_step(ibis, y, t, verbose=True, out=sys.stdout):
    """smc²!(ibis, y, t)   ibis.jl:154-189 (1-based t, t >= 2)"""
    y = np.asarray(y, dtype=np.float64)
    if verbose:
        out.write("t = %4d\tess = %4.3f" % (t - 1, ibis.ess))
    if ibis.ess < ibis.ess_min:
        resample_(ibis)
        rejuvenate_(ibis, y[: t - 1], 1.0, verbose, out)
    ess, _ = _window(ibis, y[t - 1: t], 0.0, t)
    ibis.ess = float(ess[0])
    ibis.t = t
    if verbose:
        out.write("\n")
    return ibis


def smc2_run(ibis, y, t_from, t_to, window=16, verbose=True, out=sys.stdout, summaries=None, ahead=0):
    """for t in t_from:t_to  smc²!(ibis, y, t)  end, the same results bit for bit, with up to `window` steps per launch: the
    device computes the reweight records of every step, the host finds the first step whose ESS falls below the threshold,
    the steps up to it are kept and the rest redone after the resample-move.
    summaries=True or a list of quantile levels: ibis.summary_trace gets one entry per period kept,
    (t, y, Sigma, between, xbar, Sbar, quantiles or None) with (y, Sigma, between) = observation_dist(ibis, ahead, between=True)
    and (xbar, Sbar) of filtered_state(ibis) after that period - recorded inside the window launches, bit for bit what those
    calls give after every smc2_step, with no read of the cloud.  (Without the argument: as switched by ibis.set_summaries.)"""
    y = np.asarray(y, dtype=np.float64)
    t = int(t_from)
    if summaries is not None:
        keep = ibis._summ
        ibis.set_summaries(summaries, ahead)
        ibis.summary_trace = [e for e in ibis.summary_trace if e[0] < t]
        try:
            return smc2_run(ibis, y, t_from, t_to, window, verbose, out)
        finally:
            ibis._summ = keep
    while t <= t_to:
        if verbose:
            out.write("t = %4d\tess = %4.3f" % (t - 1, ibis.ess))
        if ibis.ess < ibis.ess_min:
            resample_(ibis)
            rejuvenate_(ibis, y[: t - 1], 1.0, verbose, out)
        k = max(1, min(int(window), 64, t_to - t + 1))
        ess, j = _window(ibis, y[t - 1: t - 1 + k], ibis.ess_min, t)
        ibis.ess = float(ess[-1])
        ibis.t = t + j - 1
        if verbose:
            out.write("\n" + "".join("t = %4d\tess = %4.3f\n" % (t + i, ess[i]) for i in range(j - 1)))
        t += j
    return ibis


def expected_parameters(ibis):
    """sum_m theta[m] * omega[m]   ibis.jl:60-64"""
    w = ibis.omega
    return (ibis.theta * w[:, None]).sum(axis=0)


def posterior_moments(ibis):
    """(mean [d], cov [d][d]) of theta under the normalised outer weights: mean = sum omega theta (expected_parameters up to
    rounding), cov = sum omega (theta - mean)(theta - mean)' (uncorrected), reduced on the device - d + d^2 doubles come back
    (smc_ibis_theta_moments).  Before the first sampler call: the same specification on the host over the initial cloud."""
    if ibis._h is None:
        return _lib.host_theta_moments(ibis._theta0, np.zeros(ibis.M), weighted=True)
    return ibis._h.theta_moments(weighted=True)


def _cloud_calls(ibis):
    """(quantiles(p [np]) -> [d][np], histogram(component, lo, hi, bins) -> (counts, W), d) of the sampler's theta cloud: the
    device calls, or before the first sampler call their host twins over the initial cloud"""
    if ibis._h is None:
        theta, logw = ibis._theta0, np.zeros(ibis.M)
        return (lambda p: _lib.host_theta_quantiles(theta, logw, p),
                lambda c, lo, hi, bins: _lib.host_theta_histogram(theta, logw, c, lo, hi, bins), theta.shape[1])
    return ibis._h.theta_quantiles, ibis._h.theta_histogram, ibis._h.d


def quantiles_from(quantiles, p):
    """the shape rule of posterior_quantiles over a quantiles(p [np]) -> [d][np] call: [d] for a scalar level, [d][len(p)] for a
    list; more than 8 levels take several calls"""
    levels = np.atleast_1d(np.asarray(p, dtype=np.float64))
    if levels.ndim != 1 or levels.size == 0:
        raise ValueError("posterior_quantiles: p is a level or a non-empty list of levels")
    out = np.concatenate([quantiles(levels[i:i + 8]) for i in range(0, levels.size, 8)], axis=1)
    return out[:, 0] if np.ndim(p) == 0 else out


def histogram_from(quantiles, histogram, d, component=None, bins=50, range=None, outside=False):
    """posterior_histogram over the two calls of a cloud (_cloud_calls)"""
    if component is None:
        return [histogram_from(quantiles, histogram, d, c, bins, range, outside) for c in np.arange(d)]
    component = int(component)
    if not 0 <= component < d:
        raise ValueError("posterior_histogram: component outside [0, d)")
    if range is None:
        lo, hi = quantiles(np.array([0.0, 1.0]))[component]
        if lo != lo:
            raise ValueError("posterior_histogram: no particle carries weight, so there is no range to take")
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5                  # all the weight on one value: numpy's rule
        else:
            hi = np.nextafter(hi, np.inf)               # [lo, hi) with the largest value in the last bin
    else:
        lo, hi = float(range[0]), float(range[1])
    counts, W = histogram(component, lo, hi, int(bins))
    if W == 0:
        raise ValueError("posterior_histogram: no particle carries weight")
    mass = counts.astype(np.float64) / float(W)
    edges = np.linspace(lo, hi, int(bins) + 1)
    if outside:
        return mass[1:-2], edges, (mass[0], mass[-2], mass[-1])
    return mass[1:-2], edges


def posterior_quantiles(ibis, p):
    """the weighted quantiles of every parameter under the normalised outer weights: [d] for a level p, [d][len(p)] for a list -
    the median and the ends of a credible interval without a read of the cloud.  For coordinate i the smallest theta[m][i] with
    the weight at or below it above p (no interpolation; p = 0 and p = 1: the smallest and the largest value that carries
    weight), on integer weights, so the same bits from every run and from the host (smc_ibis_theta_quantiles).
    Before the first sampler call: the same specification on the host over the initial cloud."""
    return quantiles_from(_cloud_calls(ibis)[0], p)


def posterior_histogram(ibis, component=None, bins=50, range=None, outside=False):
    """(mass [bins], edges [bins + 1]) of the marginal posterior of one parameter, or a list of d such pairs (component=None):
    what construct_histograms (plotting_utils.jl:5-37) plots, binned on the device (smc_ibis_theta_histogram).  mass sums the
    normalised weights per bin over [lo, hi) = range; range=None takes the smallest and the largest value that carries weight
    (the largest falls in the last bin), and (v - 0.5, v + 0.5) for a cloud whose weight sits on one value v.  outside=True
    also returns (under, over, nan): the mass below lo, at or above hi, and on NaN."""
    return histogram_from(*_cloud_calls(ibis), component, bins, range, outside)


def density_tempered(ibis, y, verbose=True, out=sys.stdout):
    """density_tempered(ibis, y): the loop of smc_samplers.jl:222-281 with logZ from one whole-series Kalman pass per particle
    (ibis.jl exports the name and has rejuvenate!(ibis, y, ξ, verbose) for it).  With device_moves the resample-move of every
    stage stays on the device; the bisection for the next exponent still reads logZ once per stage (not moved to the device)."""
    y = np.asarray(y, dtype=np.float64)
    h = ibis._handle()
    h.filter(y)
    ibis.t = len(y)
    logZ = ibis.logZ
    _, _, ibis.ess = _lib.host_reweight(logZ, want_w=False)                  # :232
    xi = 0.0
    stages = []
    while xi < 1.0:
        xi, ibis.ess, resample_flag, logw = _lib.host_outer_temper(logZ, xi, ibis.ess_min)     # :240-266
        if verbose:
            out.write("ξ = %1.5f\tess = %4.3f" % (xi, ibis.ess))
        if resample_flag:
            resample_(ibis, logw)
            rejuvenate_(ibis, y, xi, verbose, out)
            logZ = ibis.logZ
        else:
            h.set_logw(logw)
        stages.append((xi, ibis.ess, ibis.acc_ratio if resample_flag else None))
        if verbose:
            out.write("\n")
    return stages
