"""Host mirror of src/particles.jl over the HIP library: same names, argument meaning, return tuples.

    normalize(logw)                      -> (logmu, w, ess)     particles.jl:5-15
    resample(w, N=len(w))                -> indices (0-based)   particles.jl:17-19
    bootstrap_filter(N, y1, model)       -> (x, w, logmu)       particles.jl:87-105
    bootstrap_filter_(x, w, y, model)    -> (logmu, w, ess)     particles.jl:107-129   ("bootstrap_filter!")
    log_likelihood(N, y, model)          -> (x, w, logZ)        particles.jl:132-147
    smoother(N, y, model)                -> (x, w, logZ, s)     (no counterpart: the FFBS particle smoother)
    ParticleGibbs(N, y, model)           -> sampler             (no counterpart: the conditional particle filter)
    particle_em(N, y, model, iters)      -> dict                (no counterpart: maximum likelihood by particle EM on the smoother's
    em_mstep(model, y, s)                -> model                lag-one pair moments)
    forecast(x, w, H)                    -> dict                (no counterpart: the cloud propagated H steps ahead)
    particle_filter(N, y1, model, proposal)       -> (x, w, logmu)     particles.jl:28-52
    particle_filter_(x, w, y, model, proposal)    -> (logmu, w, ess)   particles.jl:54-84    ("particle_filter!")

A proposal is AffineGaussianProposal(c0, c1, c2, s2) (UnivariateLinearGaussian), OptimalProposal() (UnivariateLinearGaussian,
UCSV) or None, "leave the proposal argument empty" of the reference's README: the bootstrap filter.

`model` may be one StateSpaceModel or a list of them (the batched callers smc_samplers.jl:112-121,
223-229,289-295,325-335): then logmu / logZ / ess are arrays over the list.
x and w are views of device-resident state (`Particles`, `Weights`): they convert to numpy arrays
on demand (np.asarray) and are updated in place by bootstrap_filter_, like the reference's x.
Everything runs on the GPU; there is no CPU path.
"""
import itertools

import numpy as np

from . import _lib
from .models import params_matrix

_seed_counter = itertools.count(1)


def normalize(logw, device=0):
    """(logmu, w, ess) with logmu = log(mean(exp(logw)))   particles.jl:5-15"""
    return _lib.normalize(np.asarray(logw, dtype=np.float64), device)


reweight = normalize   # the samplers' name for it (smc_samplers.jl:232,249,265,298,338)


def resample(w, N=None, seed=None, stream=0, t=0, device=0):
    """N iid draws from Categorical(w), unsorted (sample(1:n, Weights(w), N), particles.jl:17-19).
    0-based indices."""
    if seed is None:
        seed = next(_seed_counter) + (1 << 40)
    return _lib.resample(np.asarray(w, dtype=np.float64), N, seed, stream, t, device)


class AffineGaussianProposal:
    """x ~ Normal(c0 + c1*xp + c2*y, sqrt(s2)) for UnivariateLinearGaussian models (s2 a variance, like Q).  One proposal, or a
    list of them beside a list of models.  AffineGaussianProposal(0, A, 0, Q) is the bootstrap filter bit for bit."""

    def __init__(self, c0, c1, c2, s2):
        self.row = (float(c0), float(c1), float(c2), float(s2))


class OptimalProposal:
    """the locally optimal proposal p(x | xp, y), derived from the model on the device: UnivariateLinearGaussian (all of the
    state) and UCSV (the trend, given the volatilities, which move by the transition)."""


def optimal_proposal(model):
    """the locally optimal proposal of a UnivariateLinearGaussian model as an AffineGaussianProposal (the row OptimalProposal()
    uses); OptimalProposal() itself for a UCSV model, whose proposal has no parameters"""
    mid, raw = params_matrix(model)
    if mid == _lib.MODEL_UCSV3D:
        return OptimalProposal()
    return AffineGaussianProposal(*_lib.host_optimal_proposal(mid, raw[0]))


def proposal_rows(proposal, n_theta):
    """(kind, rows or None) of a proposal argument for a handle of n_theta filters (Handle.set_proposal)"""
    if proposal is None:
        return _lib.PROP_NONE, None
    if isinstance(proposal, OptimalProposal):
        return _lib.PROP_OPTIMAL, None
    if isinstance(proposal, AffineGaussianProposal):
        return _lib.PROP_AFFINE, np.tile(np.asarray(proposal.row), (n_theta, 1))
    if isinstance(proposal, (list, tuple)) and len(proposal) == n_theta and all(isinstance(p, AffineGaussianProposal) for p in proposal):
        return _lib.PROP_AFFINE, np.asarray([p.row for p in proposal])
    raise ValueError("proposal must be None, OptimalProposal(), an AffineGaussianProposal or a list of them, one per model")


def trend_moments(mean, var):
    """(mean, variance) of the trend x under a MarginalUCSV filter from the moments of its state rows (m, lse, lsn, P): the mean
    of m, and the variance of the mixture of the particles' Gaussians - between (the variance of m) plus within (the mean of
    P).  `mean`, `var` are what Particles.moments() returns, or s["mean"][t], s["var"][t] of log_likelihood(..., moments=True):
    the state rows on the LAST axis ([4], or [n_theta][4])."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    if mean.shape != var.shape or mean.shape[-1] != 4:
        raise ValueError("trend_moments takes the moments of the four state rows of a MarginalUCSV filter")
    return mean[..., 0], var[..., 0] + mean[..., 3]


class _Filters:
    """Device state shared by the Particles / Weights views of one bootstrap_filter call."""

    def __init__(self, N, models, seed, seg, device, streams, ancestors, resampler="multinomial", proposal=None, rows=None, missing=False,
                 conditional=False, ancestor_sampling=False):
        """rows=(model id, [n_theta][n_raw] parameter rows): a batch given as rows instead of `models` (then None)
        missing=True: a NaN observation is a missing one (FLAG_NAN_MISSING)
        conditional=True: the conditional particle filter (FLAG_CONDITIONAL): the caller sets the reference
        ancestor_sampling=True (with conditional): the record keeps the ancestors (FLAG_ANCESTOR_SAMPLING)"""
        if rows is not None:
            mid, raw = int(rows[0]), np.ascontiguousarray(rows[1], dtype=np.float64)
        else:
            mid, raw = params_matrix(models)
        self.single = rows is None and not isinstance(models, (list, tuple))
        if resampler not in ("multinomial", "systematic"):
            raise ValueError("resampler must be 'multinomial' (the reference's law) or 'systematic' (opt-in)")
        flags = (_lib.FLAG_ANCESTORS if ancestors else 0) | (_lib.FLAG_SYSTEMATIC if resampler == "systematic" else 0) | (
            _lib.FLAG_NAN_MISSING if missing else 0) | (_lib.FLAG_CONDITIONAL if conditional else 0) | (
            _lib.FLAG_ANCESTOR_SAMPLING if ancestor_sampling else 0)
        self.h = _lib.Handle(mid, raw.shape[0], N, seg=seg, seed=seed, device=device, flags=flags)
        self.h.set_params(raw)
        if streams is not None:
            self.h.set_streams(streams)
        self.model_id, self.raw = mid, raw
        self.seed = int(seed)
        self.proposal = None
        self.set_proposal(proposal)

    def set_proposal(self, proposal):
        kind, rows = proposal_rows(proposal, self.h.n_theta)
        if kind != _lib.PROP_NONE or self.proposal is not None:
            self.h.set_proposal(kind, rows)
        self.proposal = None if kind == _lib.PROP_NONE else (kind, rows)

    def check_proposal(self, proposal):
        kind, rows = proposal_rows(proposal, self.h.n_theta)
        new = None if kind == _lib.PROP_NONE else (kind, rows)
        same = (new is None and self.proposal is None) or (
            new is not None and self.proposal is not None and new[0] == self.proposal[0] and np.array_equal(new[1], self.proposal[1]))
        if not same:
            self.set_proposal(proposal)

    def check_model(self, models):
        mid, raw = params_matrix(models)
        if mid != self.model_id or raw.shape != self.raw.shape:
            raise ValueError("model family / batch size differs from the one the particles were created with")
        if not np.array_equal(raw, self.raw):
            self.h.set_params(raw)
            self.raw = raw

    def out(self, a):
        return float(a[0]) if self.single else a


class _summary_mode:
    """the handle in the summary mode of one call (weighted=False: the unweighted mode), restored afterwards"""

    def __init__(self, h, weighted):
        self.h, self.mode = h, "weighted" if weighted else "unweighted"

    def __enter__(self):
        self.old = self.h.summary_mode
        if self.mode != self.old:
            self.h.set_summary_mode(self.mode)

    def __exit__(self, *exc):
        if self.mode != self.old:
            self.h.set_summary_mode(self.old)


class Particles:
    """x: the particle states, resident on the GPU.  np.asarray(x) -> [N] (scalar state), [N, d], or with
    a leading batch axis for a list of models."""

    def __init__(self, f):
        self._f = f

    def __array__(self, dtype=None, copy=None):
        x, _, _ = self._f.h.state(want_w=False, want_anc=False)      # [d][n_theta][N]
        x = np.moveaxis(x, 0, -1)                                   # [n_theta][N][d]
        if x.shape[-1] == 1:
            x = x[..., 0]
        return x[0] if self._f.single else x

    def __len__(self):
        return self._f.h.n_x

    def moments(self, weighted=True):
        """(mean, variance) of the filtered state under the current weights, computed on the device.  weighted=False: the sample
        mean and the corrected variance of the cloud itself, mean(x) and var(x) (README.md:33-61 of the reference)."""
        with _summary_mode(self._f.h, weighted):
            m, v = self._f.h.moments()       # [d][n_theta]
        m, v = m.T, v.T
        if m.shape[-1] == 1:
            m, v = m[..., 0], v[..., 0]
        return (m[0], v[0]) if self._f.single else (m, v)

    def quantile(self, p, component=0, weighted=True):
        """Quantiles of the filtered state, computed on the device.  [len(p)] or [n_theta][len(p)].
        weighted=True: the inverse of the weighted empirical CDF (no interpolation between particles).
        weighted=False: `quantile(x, p)` of the cloud whatever its weights, as the reference's README loop and UCSV example
        compute it (Statistics.quantile: Hyndman-Fan type 7, interpolating; numpy's default method), bit for bit.
        Not offered: StatsBase's weighted *interpolating* `quantile(x, weights(w), p)` of get_quantiles_uc
        (examples/inflation_example.jl:45) - StatsBase is not part of the reference tree, so it cannot be pinned."""
        with _summary_mode(self._f.h, weighted):
            q = self._f.h.quantiles(p, component)
        return q[0] if self._f.single else q

    def ancestors(self):
        _, _, a = self._f.h.state(want_w=False, want_anc=True)
        return a[0] if self._f.single else a

    def predictive(self, y_t):
        """(pit, obs_mean, obs_var) for the observation y_t the last step assimilated: pit = P(Y_t <= y_t | y_1:t-1), uniform under
        a correct model, and the mean and variance of the one-step predictive law of y_t - computed on the device from the cloud
        whatever its weights (a bootstrap step resamples first, so the cloud it leaves is a sample of p(x_t | y_1:t-1); DESIGN.md
        2r).  Scalars, or [n_theta] for a list of models.  Bootstrap filters only."""
        _predictive_check(self._f.model_id, self._f.proposal, "x.predictive")
        pit, m, v = self._f.h.predictive(float(y_t))
        return self._f.out(pit), self._f.out(m), self._f.out(v)


class Weights:
    """w: the normalised weights of normalize() (particles.jl:11), resident on the GPU."""

    def __init__(self, f):
        self._f = f

    def __array__(self, dtype=None, copy=None):
        _, w, _ = self._f.h.state(want_w=True, want_anc=False)
        return w[0] if self._f.single else w

    def __len__(self):
        return self._f.h.n_x


def _predictive_check(model_id, proposal, who):
    """predictive checks are defined for bootstrap filters whose rows are a sample of the state: refused without a
    device call"""
    if model_id == _lib.MODEL_UCSV_RB:
        raise TypeError("%s: MarginalUCSV keeps the UPDATED Kalman pair (m, P) of the trend in its rows; the predictive pair of y_t, "
                        "formed inside the step, is not kept - use UCSV for predictive checks" % who)
    if proposal is not None:
        raise ValueError("%s: a guided filter's cloud is drawn from the proposal and is not a sample of p(x_t | y_1:t-1); "
                         "predictive checks need the bootstrap filter (proposal=None)" % who)


def _predictive_out(f, rows):
    """(pit, obs_mean, obs_var) [T][n_theta] each -> the dict entries, [T] for a single model"""
    keys = ("pit", "obs_mean", "obs_var")
    return {k: (r[:, 0] if f.single else r) for k, r in zip(keys, rows)}


def pit_residuals(pit):
    """Phi^-1(pit): the normalised forecast residuals, iid N(0, 1) under a correct model (their correlogram shows a wrong
    persistence, their variance a wrong observation noise).  statistics.NormalDist().inv_cdf elementwise; 0 -> -inf, 1 -> +inf,
    NaN (a gap) stays NaN."""
    import statistics
    inv = statistics.NormalDist().inv_cdf
    p = np.asarray(pit, dtype=np.float64)

    def one(u):
        if u != u:
            return np.nan
        if u <= 0.0:
            return -np.inf
        if u >= 1.0:
            return np.inf
        return inv(u)
    return np.array([one(float(u)) for u in p.ravel()]).reshape(p.shape)


def bootstrap_filter(N, y, model, seed=None, seg=0, device=0, streams=None, ancestors=False, resampler="multinomial", missing=False):
    """x, w, logmu = bootstrap_filter(N, y[1], model)   particles.jl:87-105
    resampler="systematic" (opt-in, not the reference's law) applies to the following bootstrap_filter_ steps.
    missing=True (opt-in): a NaN observation, here and in the bootstrap_filter_ steps that follow (they read it from the handle
    behind x), is a period without an observation - the cloud moves by the transition, the weights become uniform, logmu = 0
    (DESIGN.md 2j).  Without it a NaN kills its step."""
    if seed is None:
        seed = next(_seed_counter)
    f = _Filters(int(N), model, seed, seg, device, streams, ancestors, resampler, missing=missing)
    logmu = f.h.init(float(y))
    return Particles(f), Weights(f), f.out(logmu)


def bootstrap_filter_(states, weights, y, model):
    """logmu, w, ess = bootstrap_filter!(x, w, y[t], model)   particles.jl:107-129
    `states` is updated in place (device resident); the returned w is the new weight view."""
    f = states._f
    if weights._f is not f:
        raise ValueError("states and weights belong to different filters")
    f.check_model(model)
    logmu, ess = f.h.step(float(y))
    return f.out(logmu), Weights(f), f.out(ess)


def particle_filter(N, y, model, proposal=None, seed=None, seg=0, device=0, streams=None, ancestors=False, resampler="multinomial",
                    missing=False):
    """x, w, logmu = particle_filter(N, y[1], model, proposal)   particles.jl:28-52
    The first step draws from initial_dist and weights by the observation density, exactly bootstrap_filter (the reference
    adds logpdf(initial_dist, x) there, a slip: DESIGN.md "Guided filters"); the proposal applies to the particle_filter_ steps
    that follow.  proposal=None is bootstrap_filter.  missing=True: as in bootstrap_filter; a missing step moves the particles by
    the transition, not by the proposal (a proposal has no role without y)."""
    if seed is None:
        seed = next(_seed_counter)
    f = _Filters(int(N), model, seed, seg, device, streams, ancestors, resampler, proposal, missing=missing)
    logmu = f.h.init(float(y))
    return Particles(f), Weights(f), f.out(logmu)


def particle_filter_(states, weights, y, model, proposal=None):
    """logmu, w, ess = particle_filter!(x, w, y[t], model, proposal)   particles.jl:54-84
    x = rand(proposal(xp, y)), logw = logpdf(observation(x), y) + logpdf(transition(xp), x) - logpdf(proposal(xp, y), x);
    proposal=None is bootstrap_filter_."""
    f = states._f
    if weights._f is not f:
        raise ValueError("states and weights belong to different filters")
    f.check_model(model)
    f.check_proposal(proposal)
    logmu, ess = f.h.step(float(y))
    return f.out(logmu), Weights(f), f.out(ess)


def _summaries_out(f, T):
    """per-step summaries of the call just made, in the shapes of the README loop: quantiles [T][len(p)], mean / var [T] (scalar
    state) or [T][d]; with a list of models a batch axis follows T"""
    q, mean, var = f.h.get_summaries(T)
    out = {}
    if q is not None:
        out["quantiles"] = q[:, 0, :] if f.single else q
    if mean is not None:
        mean, var = np.moveaxis(mean, 1, -1), np.moveaxis(var, 1, -1)      # [T][n_theta][d]
        if mean.shape[-1] == 1:
            mean, var = mean[..., 0], var[..., 0]
        out["mean"], out["var"] = (mean[:, 0], var[:, 0]) if f.single else (mean, var)
    return out


def log_likelihood(N, y, model, seed=None, seg=0, device=0, streams=None, ancestors=False, trace=False,
                   resampler="multinomial", quantiles=None, component=0, moments=False, weighted=True, proposal=None, missing=False,
                   predictive=False):
    """x, w, logZ = log_likelihood(N, y, model)   particles.jl:132-147
    trace=True additionally returns the per-step (logmu_t, ess_t).  resampler="systematic": opt-in systematic
    resampling (same expectation, lower variance, one launch per step for big filters; not the reference's law).
    quantiles=[...] / moments=True: the README loop (README.md:33-61: bootstrap_filter!, then quantile(x, ...) at every
    observation) as ONE call - the per-step quantiles of state coordinate `component` and / or mean and variance are computed
    on the device inside the filter loop and returned as a dict behind the usual results.  weighted=False gives the README's own
    numbers: the unweighted type-7 `quantile(x, p)` and the corrected `var(x)` of the cloud (see Particles.quantile);
    weighted=True (the default) the weighted inverse CDF and the uncorrected weighted variance.
    proposal: the guided filter (particle_filter_ at every step after the first) instead of the bootstrap filter.
    missing=True (opt-in): NaN entries of y are periods without an observation: they add nothing to logZ, and the
    per-step summaries there are those of the propagated cloud.
    predictive=True: predictive checks - a dict s behind the usual results with s["pit"], s["obs_mean"],
    s["obs_var"], each [T] (a batch axis follows T): the probability integral transform of every y_t under its one-step predictive
    law, and that law's mean and variance (see Particles.predictive; pit_residuals(s["pit"]) are the normalised residuals).  The
    filter then runs step by step, one launch more per step, and keeps no record.  Bootstrap filters only; not together with
    quantiles= / moments=.  At a gap (missing=True) the pit is NaN and the moments are the forecast of the unobserved y_t."""
    if predictive:
        if quantiles is not None or moments:
            raise ValueError("predictive=True runs step by step; the per-step summaries (quantiles=, moments=) belong to the whole-series call")
        _predictive_check(params_matrix(model)[0], proposal, "log_likelihood(predictive=True)")
    if seed is None:
        seed = next(_seed_counter)
    f = _Filters(int(N), model, seed, seg, device, streams, ancestors, resampler, proposal, missing=missing)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if predictive:
        y = y.ravel()
        lm, es, rows = np.zeros((y.size, f.h.n_theta)), np.zeros((y.size, f.h.n_theta)), np.zeros((3, y.size, f.h.n_theta))
        for t in range(y.size):
            if t == 0:
                lm[0] = f.h.init(float(y[0]))
                es[0] = f.h.logZ()[1]
            else:
                lm[t], es[t] = f.h.step(float(y[t]))
            rows[0, t], rows[1, t], rows[2, t] = f.h.predictive(float(y[t]))
        logZ = f.h.logZ()[0]
        extra = _predictive_out(f, rows)
        if trace:
            if f.single:
                lm, es = lm[:, 0], es[:, 0]
            return Particles(f), Weights(f), f.out(logZ), lm, es, extra
        return Particles(f), Weights(f), f.out(logZ), extra
    summ = quantiles is not None or moments
    if summ:
        f.h.set_summaries(quantiles, component, moments)
        try:
            with _summary_mode(f.h, weighted):
                res = f.h.log_likelihood(y, trace=trace)
                extra = _summaries_out(f, y.size)
        finally:
            f.h.set_summaries()
        if trace:
            logZ, lm, es = res
            if f.single:
                lm, es = lm[:, 0], es[:, 0]
            return Particles(f), Weights(f), f.out(logZ), lm, es, extra
        return Particles(f), Weights(f), f.out(res), extra
    if trace:
        logZ, lm, es = f.h.log_likelihood(y, trace=True)
        if f.single:
            lm, es = lm[:, 0], es[:, 0]
        return Particles(f), Weights(f), f.out(logZ), lm, es
    logZ = f.h.log_likelihood(y)
    return Particles(f), Weights(f), f.out(logZ)


def _path_seed(seed):
    """the default path seed of a filter seed: another 64-bit word, so that the walk's draws are not the filter's"""
    return (int(seed) * 0x9E3779B97F4A7C15 + 0xBAC4) & 0xFFFFFFFFFFFFFFFF


def _forecast_seed(seed):
    """the default forecast seed of a filter seed: another 64-bit word again, so that the forecast draws are neither the filter's
    nor the backward walk's"""
    return (int(seed) * 0xD1342543DE82EF95 + 0xF0CA) & 0xFFFFFFFFFFFFFFFF


def _state_last(a, single):
    """[H][d][n_theta] -> [H][n_theta][d], the state axis dropped for a scalar state and the batch axis for a single model"""
    a = np.moveaxis(a, 1, -1)
    if a.shape[-1] == 1:
        a = a[..., 0]
    return a[:, 0] if single else a


def forecast(x, w, H, quantiles=None, component=0, seed=None, clouds=False):
    """f = forecast(x, w, H): the forecast fan of the filter behind the Particles / Weights of any filter call (one model or a list,
    any family, any proposal, either resampler) - p(x_{T+k} | y_1:T) and p(y_{T+k} | y_1:T), k = 1..H, by propagating the
    weighted cloud on the device (smc_forecast): every particle moves by the transition law and keeps its weight;
    nothing is resampled, and the filter is left exactly as it was.  f[...][k] belongs to horizon k + 1:
        f["mean"], f["var"]           weighted mean and variance of the state, [H] (scalar state) or [H][d]
        f["quantiles"]                (quantiles=[...], at most 8 levels) weighted quantiles of state coordinate `component`, [H][len(p)]
        f["obs_mean"], f["obs_var"]   mean and variance of the predictive law of y, [H]: sum w E[y | particle], and the variance of
                                      the mixture - within (sum w Var[y | particle]) plus between
        f["obs_quantiles"]            weighted quantiles of one predictive draw of y per particle, [H][len(p)]
        f["x"], f["y"]                (clouds=True) the propagated clouds [H][N] or [H][N][d] and the predictive draws [H][N]:
                                      with np.asarray(w) they are weighted trajectories (particle i is ONE path over the horizons)
    With a list of models a batch axis follows H everywhere.  seed: the Philox seed of the forecast draws (default: derived from
    the filter's seed); trajectory i depends on it, on the particle and on its filter's stream alone, not on H.
    MarginalUCSV: the state rows are (m, lse, lsn, P), and trend_moments(f["mean"][k], f["var"][k]) is the forecast trend: the
    mean of row 0, and the variance of row 0 plus the mean of row 3."""
    f = x._f
    if w._f is not f:
        raise ValueError("states and weights belong to different filters")
    H = int(H)
    if H < 1:
        raise ValueError("forecast needs H >= 1")
    seed = _forecast_seed(f.seed) if seed is None else int(seed)
    r = f.h.forecast(H, seed, p=quantiles, component=component, obs=True)
    out = {"mean": _state_last(r["mean"], f.single), "var": _state_last(r["var"], f.single)}
    pick = (lambda a: a[:, 0]) if f.single else (lambda a: a)
    out["obs_mean"], out["obs_var"] = pick(r["obs_mean"]), pick(r["obs_var"])
    if "q" in r:
        out["quantiles"], out["obs_quantiles"] = pick(r["q"]), pick(r["obs_q"])
    if clouds:
        xf, yf = f.h.forecast_cloud(H, seed)
        xf = np.moveaxis(xf, 1, -1)                                    # [H][n_theta][N][d]
        if xf.shape[-1] == 1:
            xf = xf[..., 0]
        out["x"], out["y"] = pick(xf), pick(yf)
    return out


def _paths_out(idx, xs, single):
    """sample_paths' arrays in the shapes of s["x"]: index [T][M], states [T][M] or [T][M][d]; a batch axis follows T"""
    xs = np.moveaxis(xs, 1, -1)                                        # [T][n_theta][M][d]
    if xs.shape[-1] == 1:
        xs = xs[..., 0]
    return (idx[:, 0], xs[:, 0]) if single else (idx, xs)


def _run_recorded(h, y):
    """the filter of log_likelihood over y step by step on a handle that records (history_begin by the caller, who also ends it):
    the per-step (logmu [T][n_theta], ess [T][n_theta]) and logZ [n_theta]"""
    lm, es = np.zeros((y.size, h.n_theta)), np.zeros((y.size, h.n_theta))
    lm[0] = h.init(float(y[0]))
    es[0] = h.logZ()[1]
    for t in range(1, y.size):
        lm[t], es[t] = h.step(float(y[t]))
    return lm, es, h.logZ()[0]


def _reference_in(reference, f, T):
    """a reference trajectory as the callers give it - [T] or [T][d]; with a list of models a batch axis after T: [T][n_theta] or
    [T][n_theta][d], the shape of s["paths"][:, ..., 0, ...] - as the handle takes it: [T][d][n_theta]"""
    r = np.asarray(reference, dtype=np.float64)
    d, nt = f.h.d, f.h.n_theta
    want = (T,) + (() if f.single else (nt,)) + (() if d == 1 else (d,))
    if r.shape != want:
        raise ValueError("reference must have the shape %r (time, then the batch, then the state), not %r" % (want, r.shape))
    return np.ascontiguousarray(np.moveaxis(r.reshape(T, nt, d), 1, -1))


def _reference_out(xref, single):
    """[T][d][n_theta] -> [T] or [T][d]; a batch axis follows T"""
    r = np.moveaxis(xref, 1, -1)                                       # [T][n_theta][d]
    if r.shape[-1] == 1:
        r = r[..., 0]
    return r[:, 0] if single else r


def _smooth_quantile_args(quantiles, component, model, rows):
    """the levels of smoother(quantiles=...) as a float64 vector, checked without a device call: 1 to 8 levels in [0, 1], a
    coordinate the state has, a family with a transition density"""
    p = np.ascontiguousarray(quantiles, dtype=np.float64).ravel()
    if p.size < 1 or p.size > 8:
        raise ValueError("quantiles: between 1 and 8 levels in one call, not %d" % p.size)
    if not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError("quantiles: every level must lie in [0, 1]")
    mid = int(rows[0]) if rows is not None else params_matrix(model)[0]
    if mid == _lib.MODEL_UCSV_RB:
        raise _lib.SmcError("smoother(quantiles=...): MarginalUCSV has no smoother of this kind (its state rows have no transition "
                            "density): rb_smoother is its smoother")
    d = _lib.lib().smc_model_dim(int(mid))
    if int(component) != component or not 0 <= int(component) < d:
        raise ValueError("component must be one of the state's %d coordinates (0-based)" % d)
    return p


def smoother(N, y, model, seed=None, seg=0, device=0, streams=None, resampler="multinomial", proposal=None, weights=False, rows=None,
             paths=0, path_seed=None, path_counts=None, smooth=True, missing=False, reference=None, pairs=False, quantiles=None, component=0,
             predictive=False):
    """x, w, logZ, s = smoother(N, y, model): the particle filter of log_likelihood run step by step with its clouds recorded on
    the device, then the FFBS backward pass over them (forward filtering, backward smoothing).  x, w, logZ are the
    filter's, as log_likelihood returns them; s describes p(x_t | y_1:T):
        s["mean"][t], s["var"][t]   smoothed mean and variance of the state, shaped like the per-step summaries of log_likelihood
                                    ([T], or [T][d]; with a list of models a batch axis follows T)
        s["logmu"], s["ess"]        the filter's per-step log-likelihood increments and effective sample sizes, [T] or [T][n_theta]
        s["weights"], s["x"]        (weights=True) the smoothed weights [T][N] and the recorded clouds [T][N] or [T][N][d] they
                                    belong to (batch axis after T)
        s["paths"], s["path_index"] (paths=M > 0) M trajectories drawn from p(x_1:T | y_1:T) by backward simulation:
                                    their states [T][M] or [T][M][d] and the particles they pass through [T][M] (int32; batch
                                    axis after T).  Unlike the marginals they carry the dependence between times: differences,
                                    lag covariances, whole-path functionals.  path_seed: the seed of the walk's draws (default:
                                    derived from the filter seed); path_counts [n_theta]: draw only that many paths of each filter
                                    (the other slots read -1 / NaN); smooth=False skips the backward pass of the marginals (no
                                    s["mean"], s["var"]).  A batch holds T n_theta M entries: keep M small there.
        s["cross"], s["resid2"], s["lag1_cov"]  (pairs=True) the lag-one pair moments of the backward pass itself, no
                                    paths and none of their noise: cross[t] = E[x_t x_{t+1} | y_1:T], [T-1] or [T-1][d][d] (row:
                                    the coordinate of x_t); resid2[t] = E[(x_{t+1} - m(x_t))^2 | y_1:T] with m the transition's
                                    centre, [T-1] or [T-1][d]; lag1_cov[t] = cross[t] - mean[t] (x) mean[t+1].  The batch axis
                                    follows T, as in s["mean"].  They are the E-step of em_mstep / particle_em.
        s["quantiles"]              (quantiles=[p, ...], up to 8 levels in [0, 1]) [T][len(p)]: the weighted quantiles of state coordinate
                                    `component` under the smoothed weights, selected on the device in the same backward pass
                                    (DESIGN.md 2q): the 25 / 50 / 75 % band of p(x_t | y_1:T) without a copy of the weights.  The
                                    definition of log_likelihood's quantiles=: no interpolation.  The batch axis follows T.
        s["pit"], s["obs_mean"], s["obs_var"]  (predictive=True) predictive checks of the FILTER over the recorded clouds, in one launch
                                    (the keys of log_likelihood(predictive=True), the same bits).  Bootstrap filters
                                    only: ValueError with a proposal or a reference.
    The backward pass costs 2 N^2 (T - 1) transition densities per filter.  Any proposal, either resampler; MarginalUCSV has no
    smoother of this kind (its state rows have no transition density): rb_smoother is its smoother.
    rows=(model id, parameter rows [n_theta][n_raw]) with model=None: a batch given as rows (what the samplers hold).
    missing=True (opt-in): NaN entries of y are periods without an observation; s["mean"], s["var"] and the paths
    there are the interpolated state.
    reference=[T] or [T][d] (a batch axis after T, as in s["paths"]): the run is the CONDITIONAL particle filter - one
    slot of every step is pinned to that trajectory; everything returned is shaped as ever, but logZ is not a likelihood estimate.
    One path of it (paths=1) is one sweep of particle Gibbs: ParticleGibbs keeps the handle between sweeps."""
    if pairs and not smooth:
        raise ValueError("pairs=True needs the backward pass of the marginals (smooth=True): the pair moments are formed inside it")
    if quantiles is not None:
        if not smooth:
            raise ValueError("quantiles=... needs the backward pass of the marginals (smooth=True): they are selected under its weights")
        quantiles = _smooth_quantile_args(quantiles, component, model, rows)
    if predictive:
        _predictive_check(int(rows[0]) if rows is not None else params_matrix(model)[0], proposal, "smoother(predictive=True)")
        if reference is not None:
            raise ValueError("smoother(predictive=True): a conditional filter's cloud holds the pinned reference and is not a predictive sample")
    if seed is None:
        seed = next(_seed_counter)
    f = _Filters(int(N), model, seed, seg, device, streams, False, resampler, proposal, rows=rows, missing=missing,
                 conditional=reference is not None)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    T, h = y.size, f.h
    if T < 1:
        raise ValueError("smoother needs at least one observation")
    if reference is not None:
        h.set_reference(_reference_in(reference, f, T))
    h.history_begin(T)
    try:
        lm, es, logZ = _run_recorded(h, y)
        s = {}
        if smooth or weights:
            ws, mean, var, *pm = h.smooth(weights=weights, moments=True, pairs=pairs,
                                          quantiles=None if quantiles is None else (int(component), quantiles))
            if quantiles is not None:
                q = pm.pop()                                                   # [T][n_theta][np]
                s["quantiles"] = q[:, 0] if f.single else q
            mean, var = np.moveaxis(mean, 1, -1), np.moveaxis(var, 1, -1)      # [T][n_theta][d]
            if mean.shape[-1] == 1:
                mean, var = mean[..., 0], var[..., 0]
            s["mean"], s["var"] = (mean[:, 0], var[:, 0]) if f.single else (mean, var)
            if pairs:
                cross, resid2 = np.moveaxis(pm[0], 3, 1), np.moveaxis(pm[1], 1, -1)   # [T-1][n_theta][d][d], [T-1][n_theta][d]
                if h.d == 1:
                    cross, resid2 = cross[..., 0, 0], resid2[..., 0]
                    outer = mean[:-1] * mean[1:]
                else:
                    outer = mean[:-1][..., :, None] * mean[1:][..., None, :]
                lag = cross - outer
                s["cross"], s["resid2"], s["lag1_cov"] = (cross[:, 0], resid2[:, 0], lag[:, 0]) if f.single else (cross, resid2, lag)
        if paths:
            idx, xp = h.sample_paths(int(paths), _path_seed(seed) if path_seed is None else int(path_seed), counts=path_counts)
            s["path_index"], s["paths"] = _paths_out(idx, xp, f.single)
        s["logmu"], s["ess"] = (lm[:, 0], es[:, 0]) if f.single else (lm, es)
        if predictive:
            s.update(_predictive_out(f, h.predictive_record(y)))
        if weights:
            xs = np.array([h.history_get(t)[0] for t in range(T)])        # [T][d][n_theta][N]
            xs = np.moveaxis(xs, 1, -1)                                    # [T][n_theta][N][d]
            if xs.shape[-1] == 1:
                xs = xs[..., 0]
            s["weights"], s["x"] = (ws[:, 0], xs[:, 0]) if f.single else (ws, xs)
    finally:
        h.history_end()
    return Particles(f), Weights(f), f.out(logZ), s


class ParticleGibbs:
    """pg = ParticleGibbs(N, y, model): particle Gibbs with backward simulation (Andrieu, Doucet and Holenstein 2010; Whiteley;
    Lindsten and Schoen) for one model or a list of them (one chain each), on ONE conditional handle that lives as
    long as the sampler.  pg.sweep() runs the conditional particle filter over y with the current path pinned, draws ONE
    backward-simulated path per filter and adopts it on the device: a Markov kernel that leaves p(x_1:T | y_1:T, theta) invariant
    for any N >= 2.  Alternate it with the user's own draw of theta given pg.path, handed back with pg.set_model(...).
        reference        the starting path, [T] or [T][d] (a batch axis after T); None: one path of an unconditional
                         smoother(paths=1, smooth=False) under sweep_seed(0)
        pg.sweep()       -> the new path, shaped like reference; sweep k (1, 2, ...) runs under the filter seed pg.sweep_seed(k) and the
                         path seed derived from it as smoother derives it, so smoother(..., seed=pg.sweep_seed(k), reference=previous
                         path, paths=1) reproduces it bit for bit
        pg.set_model(m)  a model, a list of them, or parameter rows [n_theta][n_raw]: theta for the next sweep
        pg.path, pg.logmu, pg.ess, pg.sweeps, pg.kept   the current path; the last sweep's per-step increments and effective sample
                         sizes; sweeps done; filters whose path was dead in the last sweep and that kept their path (0 in practice)
        ancestor_sampling=True   particle Gibbs with ANCESTOR SAMPLING (Lindsten, Jordan and Schoen 2014) instead of
                         backward simulation: at every step the pinned particle redraws its ancestor given the old path, and the new
                         path is the ancestor lineage of one particle drawn from the last weights.  The same invariance for any
                         N >= 2, without the T dependent rounds of the backward walk: one launch over (step, filter) and T lookups per
                         filter (Handle.ancestor_sweep under the path seed of the sweep).  Another kernel on paths: its sweeps are not
                         those of the default.  pg.ancestor_sampling tells which one the chain uses.  Out of scope:
                         smoother(reference=..., ancestor_sampling=...) and a Julia binding.
    Bootstrap families with a transition density (UnivariateLinearGaussian, StochasticVolatility, UCSV), multinomial resampling."""

    def __init__(self, N, y, model, reference=None, seed=None, seg=0, device=0, streams=None, rows=None, ancestor_sampling=False):
        self.seed = next(_seed_counter) if seed is None else int(seed)
        self.y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        T = self.y.size
        if T < 1:
            raise ValueError("ParticleGibbs needs at least one observation")
        if reference is None:
            reference = smoother(N, self.y, model, seed=self.sweep_seed(0), seg=seg, device=device, streams=streams, rows=rows, paths=1,
                                 smooth=False)[3]["paths"]
            reference = reference[:, 0] if rows is None and not isinstance(model, (list, tuple)) else reference[:, :, 0]
        self.ancestor_sampling = bool(ancestor_sampling)
        self._f = _Filters(int(N), model, self.sweep_seed(1), seg, device, streams, False, rows=rows, conditional=True,
                           ancestor_sampling=self.ancestor_sampling)
        h = self._f.h
        h.set_reference(_reference_in(reference, self._f, T))
        h.history_begin(T)
        self.sweeps, self.kept = 0, 0
        self.logmu = self.ess = None

    def sweep_seed(self, k):
        """the filter seed of sweep k (k = 0: the unconditional start): seed + k * 0x9E3779B97F4A7C15 mod 2^64, so that every sweep
        draws from fresh Philox counters"""
        return (self.seed + int(k) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF

    def sweep(self):
        h = self._f.h
        sd = self.sweep_seed(self.sweeps + 1)
        h.reseed(sd)
        lm, es, _ = _run_recorded(h, self.y)                           # (smc_init restarts the record)
        if self.ancestor_sampling:
            self.kept = h.ancestor_sweep(_path_seed(sd))[2]
        else:
            h.sample_paths(1, _path_seed(sd), want_x=False)
            self.kept = h.reference_from_paths(0)
        self.sweeps += 1
        pick = (lambda a: a[:, 0]) if self._f.single else (lambda a: a)
        self.logmu, self.ess = pick(lm), pick(es)
        return self.path

    @property
    def path(self):
        return _reference_out(self._f.h.get_reference(), self._f.single)

    def set_model(self, model):
        if isinstance(model, np.ndarray):
            raw = np.ascontiguousarray(model, dtype=np.float64).reshape(self._f.h.n_theta, -1)
            self._f.h.set_params(raw)
            self._f.raw = raw
        else:
            self._f.check_model(model)

    def close(self):
        self._f.h.close()


EM_FREE = {_lib.MODEL_LG1D: ("A", "Q", "R"), _lib.MODEL_SV1D: ("mu", "rho", "sigma"), _lib.MODEL_UCSV3D: ("gamma_eps", "gamma_eta")}


def _em_free(model, free):
    """the names em_mstep updates, in the order of EM_FREE (the order of the columns of particle_em's theta)"""
    from .models import MarginalUCSV
    if isinstance(model, MarginalUCSV) or getattr(model, "model_id", None) not in EM_FREE:
        raise TypeError("em_mstep: UnivariateLinearGaussian, StochasticVolatility and UCSV have a closed-form M-step on the pair moments; "
                        "MarginalUCSV has no pair moments (its state rows have no transition density)")
    names = EM_FREE[model.model_id]
    if free is None:
        return names
    free = (free,) if isinstance(free, str) else tuple(free)
    bad = [p for p in free if p not in names]
    if bad:
        raise ValueError("em_mstep: %r is not among the parameters of this family that the M-step updates, %r" % (bad, names))
    return tuple(p for p in names if p in free)


def _em_theta(model, names):
    get = {"A": lambda m: m.A, "Q": lambda m: m.Q, "R": lambda m: m.R, "mu": lambda m: m.mu, "rho": lambda m: m.rho,
           "sigma": lambda m: m.sigma, "gamma_eps": lambda m: m.gamma[0], "gamma_eta": lambda m: m.gamma[1]}
    return np.array([get[p](model) for p in names])


def em_mstep(model, y, s, free=None, missing=False):
    """The M-step of particle EM as a pure function (no GPU): the model whose parameters `free` maximise the expected complete-data
    log-likelihood under the smoothed law that s describes - s of smoother(N, y, model, pairs=True) for ONE model: s["mean"],
    s["var"], s["cross"], s["resid2"] (or the exact moments of a Kalman / RTS pass in the same shapes).  free: the names to update,
    default all of the family's; every other parameter stays.  With E x_t^2 = var_t + mean_t^2,
    S00 = sum_{t<T-1} E x_t^2, S11 = sum_{t>=1} E x_t^2, S10 = sum_t cross[t], m0 = sum_{t<T-1} mean_t, m1 = sum_{t>=1} mean_t:
        UnivariateLinearGaussian {A, Q, R}:  A = S10 / S00;  Q = (S11 - 2 A S10 + A^2 S00) / (T - 1) with the A in force;  R = the
            mean over the observed periods of (y_t - B mean_t)^2 + B^2 var_t (missing=True: a NaN in y is a period without one)
        StochasticVolatility {mu, rho, sigma}:  least squares of x_{t+1} on (1, x_t): rho = ((T-1) S10 - m0 m1) / ((T-1) S00 - m0^2),
            alpha = (m1 - rho m0) / (T - 1), mu = alpha / (1 - rho) (with one of the two held, the other one's conditional
            minimiser), sigma^2 = the mean residual square with the (mu, rho) in force.  The single term of the stationary initial
            law, log N(x_1; mu, sigma^2 / (1 - rho^2)), is LEFT OUT of the M-step: with it the maximiser has no closed form, and
            its weight is 1 / T of the whole.
        UCSV {gamma_eps, gamma_eta}:  gamma_c^2 = (var_0^c + (mean_0^c - l0_c)^2 + sum_t resid2[t][c]) / T for c = lse, lsn (the
            centre of a log-volatility is the previous one whatever the parameters, so resid2 is the whole statistic): exact.
    MarginalUCSV: TypeError.  B, x0, sigma0 and the initial laws are not estimated."""
    from .models import UCSV, LinearModel, StochasticVolatility
    names = _em_free(model, free)
    y = np.asarray(y, dtype=np.float64).ravel()
    T = y.size
    mean, var = np.asarray(s["mean"], dtype=np.float64), np.asarray(s["var"], dtype=np.float64)
    cross, resid2 = np.asarray(s["cross"], dtype=np.float64), np.asarray(s["resid2"], dtype=np.float64)
    d = model.dim
    want = {"mean": (T,) + (() if d == 1 else (d,)), "cross": (T - 1,) + (() if d == 1 else (d, d)), "resid2": (T - 1,) + (() if d == 1 else (d,))}
    for key, a in (("mean", mean), ("var", var), ("cross", cross), ("resid2", resid2)):
        if a.shape != want["mean" if key == "var" else key]:
            raise ValueError("em_mstep: s[%r] has the shape %r, not %r (the moments of ONE model over y)" % (key, a.shape, want["mean" if key == "var" else key]))
    seen = np.isfinite(y)
    if not missing and not seen.all():
        raise ValueError("em_mstep: y holds a value that is not finite (missing=True reads a NaN as a period without an observation)")
    if model.model_id == _lib.MODEL_UCSV3D:
        g = list(model.gamma)
        for k, (name, c) in enumerate((("gamma_eps", 1), ("gamma_eta", 2))):
            if name in names:
                g[k] = float(np.sqrt((var[0, c] + (mean[0, c] - model.log_sigma0[k]) ** 2 + resid2[:, c].sum()) / T))
        return UCSV(tuple(g), model.x0, model.log_sigma0)
    if T < 2:
        raise ValueError("em_mstep: the transition parameters need at least two periods")
    n = T - 1
    ex2 = var + mean * mean
    S00, S11, S10, m0, m1 = ex2[:-1].sum(), ex2[1:].sum(), cross.sum(), mean[:-1].sum(), mean[1:].sum()
    if model.model_id == _lib.MODEL_LG1D:
        A, Q, R = model.A, model.Q, model.R
        if "A" in names:
            A = S10 / S00
        if "Q" in names:
            Q = (S11 - 2.0 * A * S10 + A * A * S00) / n
        if "R" in names:
            if not seen.any():
                raise ValueError("em_mstep: no observed period to estimate R from")
            B = model.B
            R = float(np.mean((y[seen] - B * mean[seen]) ** 2 + B * B * var[seen]))
        return LinearModel(float(A), model.B, float(Q), float(R), model.x0, model.sigma0)
    mu, rho, sigma = model.mu, model.rho, model.sigma
    if "mu" in names and "rho" in names:
        rho = (n * S10 - m0 * m1) / (n * S00 - m0 * m0)
        mu = (m1 - rho * m0) / n / (1.0 - rho)
    elif "rho" in names:
        rho = (S10 - mu * (m0 + m1) + n * mu * mu) / (S00 - 2.0 * mu * m0 + n * mu * mu)
    elif "mu" in names:
        mu = (m1 - rho * m0) / n / (1.0 - rho)
    if "sigma" in names:
        al = mu * (1.0 - rho)
        sigma = np.sqrt((S11 - 2.0 * al * m1 - 2.0 * rho * S10 + n * al * al + 2.0 * al * rho * m0 + rho * rho * S00) / n)
    return StochasticVolatility(float(mu), float(rho), float(sigma))


def particle_em(N, y, model, iters, seed=None, free=None, missing=False, **filter_kw):
    """r = particle_em(N, y, model, iters): maximum likelihood by particle EM for one model, or a list of models with
    one EM chain each (one batch on the device).  Iteration k = 0 .. iters-1 runs smoother(N, y, model_k, pairs=True, seed=seed_k,
    missing=missing, **filter_kw) - the E-step: the smoothed marginals and the lag-one pair moments of the FFBS backward pass - and
    then em_mstep(model_k, y, s, free, missing) per chain.  seed_k = seed + k * 0x9E3779B97F4A7C15 mod 2^64, as
    ParticleGibbs.sweep_seed derives its own: every iteration draws from fresh Philox counters, and iteration 0 is smoother(...,
    seed=seed) itself.
        r["models"]  [iters + 1]: the starting model and the one after every iteration (lists of chains, given a list)
        r["theta"]   [iters + 1][n_free]: their free parameters in the family's order ([iters + 1][n_chains][n_free], given a list)
        r["logZ"]    [iters]: the filter's log-likelihood estimate at model_k, the model each E-step ran under ([iters][n_chains])
    The estimate carries the Monte-Carlo noise of N particles per iteration: it settles around the MLE, it does not converge to it;
    average the last iterations, or raise N.  filter_kw: smoother's filter keywords (seg, device, streams, resampler, proposal)."""
    single = not isinstance(model, (list, tuple))
    chain = [model] if single else list(model)
    names = _em_free(chain[0], free)
    for m in chain:
        _em_free(m, free)
    seed = next(_seed_counter) if seed is None else int(seed)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    models, theta, logZ = [chain], [np.array([_em_theta(m, names) for m in chain])], []
    for k in range(int(iters)):
        sd = (seed + k * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        _, _, lz, s = smoother(N, y, chain, seed=sd, pairs=True, missing=missing, **filter_kw)
        chain = [em_mstep(m, y, {key: s[key][:, c] for key in ("mean", "var", "cross", "resid2")}, names, missing)
                 for c, m in enumerate(chain)]
        models.append(chain)
        theta.append(np.array([_em_theta(m, names) for m in chain]))
        logZ.append(np.asarray(lz, dtype=np.float64))
    theta = np.array(theta)
    logZ = np.array(logZ).reshape(int(iters), len(chain))
    if single:
        return {"models": [c[0] for c in models], "theta": theta[:, 0], "logZ": logZ[:, 0]}
    return {"models": models, "theta": theta, "logZ": logZ}


def rb_smoother(N, y, model, paths=256, seed=None, path_seed=None, draws=False, per_path=False, path_counts=None, seg=0, device=0,
                streams=None, resampler="multinomial", rows=None, missing=False):
    """x, w, logZ, s = rb_smoother(N, y, model, paths=M): the smoother of MarginalUCSV (one model or a list of them).  The marginal
    filter of log_likelihood is run step by step with its clouds recorded on the device; then M volatility paths per filter are
    drawn from p(lse_1:T, lsn_1:T | y_1:T) by Rao-Blackwellised backward simulation, and the trend comes exactly given each path
    from a Kalman filter and an RTS pass along it.  x, w, logZ are the filter's; s describes the smoothed law:
        s["trend_mean"][t], s["trend_var"][t]  mean and variance of p(x_t | y_1:T): the mean over the paths of the per-path mean,
                                    and within (mean of the per-path variances) + between (variance of the per-path means)
        s["vol_mean"], s["vol_var"] [T][2]: smoothed mean and variance of (lse, lsn)
        s["n_paths"]                [T]: the number of complete paths behind them
        s["logmu"], s["ess"]        the filter's per-step log-likelihood increments and effective sample sizes
        per_path=True:  s["path_index"] [T][M] int32, s["vol_paths"] [T][M][2], s["path_trend_mean"], s["path_trend_var"] [T][M]
        draws=True:     s["paths"] [T][M][3]: joint draws of (x, lse, lsn) from p(x_1:T, lse_1:T, lsn_1:T | y_1:T)
    With a list of models a batch axis follows T everywhere, as in smoother.  path_seed: the seed of the walk's draws (default:
    derived from the filter seed); path_counts [n_theta]: draw only that many paths of each filter.  Either resampler.
    rows=(model id, parameter rows [n_theta][5]) with model=None: a batch given as rows (what the samplers hold).
    missing=True: the filter reads NaN as missing, but the Kalman / RTS pass along a path has no rule for a gap yet: a NaN in y
    raises (SmcError)."""
    if seed is None:
        seed = next(_seed_counter)
    f = _Filters(int(N), model, seed, seg, device, streams, False, resampler, None, rows=rows, missing=missing)
    if f.model_id != _lib.MODEL_UCSV_RB:
        raise TypeError("rb_smoother is the smoother of MarginalUCSV; the other families have a transition density: smoother")
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    T, h = y.size, f.h
    if T < 1:
        raise ValueError("rb_smoother needs at least one observation")
    h.history_begin(T)
    try:
        lm, es, logZ = _run_recorded(h, y)
        r = h.rb_sample_paths(y, int(paths), _path_seed(seed) if path_seed is None else int(path_seed), counts=path_counts, draws=draws,
                              per_path=per_path)
    finally:
        h.history_end()
    pick = (lambda a: a[:, 0]) if f.single else (lambda a: a)
    o = r["out"]
    s = {"trend_mean": pick(o[..., 0]), "trend_var": pick(o[..., 1] + o[..., 2]), "vol_mean": pick(o[..., [3, 5]]), "vol_var": pick(o[..., [4, 6]]),
         "n_paths": pick(o[..., 7]), "logmu": pick(lm), "ess": pick(es)}
    if per_path:
        s["path_index"], s["path_trend_mean"], s["path_trend_var"] = pick(r["idx"]), pick(r["tmean"]), pick(r["tvar"])
        s["vol_paths"] = pick(np.moveaxis(r["vol"], 1, -1))                          # [T][n_theta][M][2]
    if draws:
        s["paths"] = pick(np.concatenate([r["tdraw"][..., None], np.moveaxis(r["vol"], 1, -1)], axis=-1))   # [T][n_theta][M][3]
    return Particles(f), Weights(f), f.out(logZ), s
