"""Host mirror of src/smc_samplers.jl: SMC, density_tempered, smc2 ("smc²"), smc2_step ("smc²!"), smc2_run (the
`for t in 2:T smc²!(smc,y,t) end` loop, several steps per device call), rejuvenate_, resample_, exchange!, and the
summaries of plotting_utils.jl / the example script (estimated_trend, filtered_summaries).

The O(n_theta) outer logic (bisection for the tempering exponent, resample!, the random-walk kernel) stays on the host as in
the reference, but its arithmetic is ONE specification shared by every host (csrc/smc_outer.hip, include/smc_hip.h "the OUTER
level"): `reweight` is the inner filter's integer normalize over segments of 8 parameter particles, so its sums do not depend
on the order of evaluation or on how theta is dealt out to ranks; the sampler carries the un-normalised outer log-weights
`logw` (`omega` = their normalisation, on demand); resample! draws its indices from Philox through the integer weight CDF.
Every particle filter the reference runs inside `Threads.@threads for m in 1:M` (smc_samplers.jl:112-121,174-180,223-229) or
serially (:289-295,:325-335) becomes ONE batched call on the GPU (theta axis = workgroups).

PMMH rejuvenation (rejuvenate!, smc_samplers.jl:103-146) runs entirely on the device when the sampler is given
what a GPU can evaluate instead of closures: `theta_map=ThetaMap(...)` for smc.model(theta) and a prior made of the
enumerated families (distributions.py spec()).  Then one smc_pmmh_rejuvenate call does the whole chain loop for
the rank's parameter particles - proposals, insupport, prior ratio, the proposal filters, the accept test, and the
overwrite of theta / logZ / x / w - with Philox draws keyed by the GLOBAL theta index, and no collective inside.
With arbitrary Python closures / priors the same loop stays on the host (numpy random numbers) and only the filters
are batched on the GPU.  Either way a proposal outside the prior's support is never filtered (:116).

theta sharding (multi-GPU): pass `comm=ThetaComm(...)` (distributed.py).  A rank *filters* its own contiguous slice of theta
and does the outer arithmetic of that slice; what every rank must agree on (the ESS of a step, the ancestors of a resample!,
the random-walk factor) is computed from exchanged integers or from the same counter-based random numbers, so all ranks take
identical decisions.  Collectives: one all-gather of the logZ slices per batched evaluation, one all-gather of the
moved (theta, logZ, accepted) slices per rejuvenation, one all-gather of the SEGMENT RECORDS (32 bytes per 8 parameter
particles and step) per window of online steps, one all-gather of the (logw, logZ) slices and one all-to-all of filter slots
per resample! of the online sampler.  Results do not depend on the number of ranks: filter m always uses Philox stream id m,
and the outer sums are integer sums over fixed segments.
"""
import math
import sys

import numpy as np

from . import _lib
from . import ibis as _ibis
from .ibis import IBIS
from .models import params_matrix


class RawModels:
    """A batch of models of one family given directly as parameter rows (see SMC(raw_fn=...))."""

    def __init__(self, model_id, raw):
        self.model_id, self.rows = int(model_id), np.ascontiguousarray(raw, dtype=np.float64)


def _rows(models):
    return (models.model_id, models.rows) if isinstance(models, RawModels) else params_matrix(models)


class ThetaMap:
    """smc.model(theta) in a form the device can evaluate: parameter row k of the model family `model_id` is
    theta[raw_from[k]] when raw_from[k] >= 0, else the constant raw_const[k].
    README.md:75-79 (LinearGaussian(theta1, 1.0, theta2, theta3, 0.0)):  ThetaMap(LG, [0,-1,1,2,-1,-1], [0,1,0,0,0,1]);
    examples/inflation_example.jl:227-230 (UCSV(theta1, theta2, (theta3, theta4))):  ThetaMap(UCSV, [0,0,1,2,3], [0]*5);
    the same map with MODEL_UCSV_RB runs the Rao-Blackwellised filter (models.MarginalUCSV) on the same parameter rows."""

    def __init__(self, model_id, raw_from, raw_const):
        self.model_id = int(model_id)
        self.raw_from = np.ascontiguousarray(raw_from, dtype=np.int32)
        self.raw_const = np.ascontiguousarray(raw_const, dtype=np.float64)
        if self.raw_from.size != self.raw_const.size:
            raise ValueError("raw_from and raw_const must have one entry per parameter of the model row")

    def rows(self, thetas):
        """[m, n_raw] parameter rows of the m parameter vectors in `thetas`"""
        thetas = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        out = np.tile(self.raw_const, (thetas.shape[0], 1))
        use = self.raw_from >= 0
        out[:, use] = thetas[:, self.raw_from[use]]
        return out


# ---- filter backends ---------------------------------------------------------------------------
class LibOuter:
    """The outer level (reweight, window walk, tempering bisection, resample!, random-walk factor) by the library's host
    routines (csrc/smc_outer.hip).  `window_walk` is where theta sharding shows: a rank whose slice consists of whole
    segments computes the segment records of its own parameter particles and the ranks exchange records; otherwise the
    log-likelihood increments are exchanged and every rank walks the whole vector - the same bits either way."""

    reweight = staticmethod(_lib.host_reweight)
    temper = staticmethod(_lib.host_outer_temper)
    resample = staticmethod(_lib.host_outer_resample)
    rw_factor = staticmethod(_lib.host_rw_factor)

    def window_walk(self, smc, lik_local, ess_min):
        """the host half of k = len(lik_local) smc²! steps (smc_samplers.jl:323-338): advances smc.logw / smc.logZ by the
        steps walked and returns (ess [j], j)"""
        lik_local = np.ascontiguousarray(lik_local, dtype=np.float64)
        k, per = lik_local.shape
        lo, hi = smc.lo, smc.hi
        if smc.comm is None or (per % _lib.OUTER_SEG == 0):
            rec = _lib.host_outer_window(smc.logw[lo:hi], lik_local)                  # [k][nseg_local][4]
            if smc.comm is not None:
                nsl = rec.shape[1]
                allr = smc.comm.all_gather(rec.view(np.float64).ravel()).view(np.uint64)   # 8-byte words, no arithmetic on the way
                rec = np.ascontiguousarray(allr.reshape(-1, k, nsl, 4).transpose(1, 0, 2, 3).reshape(k, -1, 4))
            ess, j = _lib.host_outer_walk(rec, smc.M, ess_min)
            smc.logw[lo:hi], smc.logZ[lo:hi] = _lib.host_outer_advance(smc.logw[lo:hi], smc.logZ[lo:hi], lik_local, j)
            smc._outer_local = smc.comm is not None          # the other ranks' slices are stale until _sync_outer
        else:
            smc._sync_outer()
            lik = smc._gather(lik_local.ravel()).reshape(-1, k, per).transpose(1, 0, 2).reshape(k, smc.M)
            rec = _lib.host_outer_window(smc.logw, lik)
            ess, j = _lib.host_outer_walk(rec, smc.M, ess_min)
            smc.logw, smc.logZ = _lib.host_outer_advance(smc.logw, smc.logZ, lik, j)
        return ess, j


class HipBackend:
    """Runs the batched inner filters on one GPU through the C ABI (no CPU fallback).
    proposal: OptimalProposal() or an AffineGaussianProposal (particles.py) makes every inner filter - the main, proposal and
    exchange handles alike, and the device PMMH - a guided particle filter; None (the default) the bootstrap filter.
    missing=True (opt-in): every inner filter reads a NaN observation as a missing one (FLAG_NAN_MISSING)."""

    outer = LibOuter()

    def __init__(self, device=0, seg=0, resampler="multinomial", proposal=None, missing=False):
        self.device, self.seg = device, seg
        self.proposal = proposal
        self.missing = bool(missing)
        self.flags = _lib.FLAG_SYSTEMATIC if resampler == "systematic" else 0   # opt-in; default = the reference's law
        self.flags |= _lib.FLAG_NAN_MISSING if self.missing else 0
        self._handles = {}

    def _handle(self, key, model_id, n_theta, N, seed):
        k = (key, model_id, n_theta, N)
        h = self._handles.get(k)
        if h is None:
            h = _lib.Handle(model_id, n_theta, N, seg=self.seg, seed=seed, device=self.device, flags=self.flags)
            if self.proposal is not None:
                from .particles import proposal_rows
                h.set_proposal(*proposal_rows(self.proposal, n_theta))
            self._handles[k] = h
        h.reseed(seed)
        return h

    def init(self, models, N, y1, seed, streams, key="main"):
        mid, raw = _rows(models)
        h = self._handle(key, mid, raw.shape[0], N, seed)
        h.set_params(raw)
        h.set_streams(streams)
        return h.init(y1), h

    def log_likelihood(self, models, N, y, seed, streams, key="prop", skip=None):
        """skip[m] = True: filter m is not run (proposal outside the prior's support, smc_samplers.jl:116); logZ = -inf"""
        mid, raw = _rows(models)
        h = self._handle(key, mid, raw.shape[0], N, seed)
        h.set_params(raw)
        h.set_streams(streams)
        h.set_skip(skip if skip is not None and np.any(skip) else None)
        try:
            out = h.log_likelihood(y)
        finally:
            h.set_skip(None)     # whatever happened: the mask must not outlive this evaluation on the cached handle
        return out, h

    def rejuvenate(self, tmap, prior_spec, N, y, xi, chol, scales, filter_seeds, move_seed, streams, theta, logZ, main):
        """rejuvenate! for this rank's parameter particles on the device (smc_pmmh_rejuvenate).
        -> (theta, logZ, accepted, filters_run)"""
        h = self._handle("prop", tmap.model_id, theta.shape[0], N, int(filter_seeds[0]))
        h.set_streams(streams)
        cfg = (tmap.raw_from.tobytes(), tmap.raw_const.tobytes(), np.asarray(prior_spec[0]).tobytes(), np.asarray(prior_spec[1]).tobytes())   # by content
        if getattr(h, "_pmmh_cfg", None) != cfg:
            h.pmmh_configure(prior_spec[0], prior_spec[1], tmap.raw_from, tmap.raw_const)
            h._pmmh_cfg = cfg
        return h.pmmh_rejuvenate(main, y, xi, chol, scales, filter_seeds, move_seed, theta, logZ)

    def release(self, h):
        """close one handle (a superseded set of online filters, exchange!)"""
        for k, v in list(self._handles.items()):
            if v is h:
                v.close()
                del self._handles[k]

    def close(self):
        for h in self._handles.values():
            h.close()
        self._handles = {}


class SMC:
    """SMC(N, M, model, prior, chain, ess_threshold, min_ar=-1.0)   smc_samplers.jl:5-59
    N state particles per filter, M parameter particles.  `model` maps a parameter vector to a
    StateSpaceModel (the reference's closure smc.model(theta))."""

    def __init__(self, N, M, model, prior, chain, ess_threshold, min_ar=-1.0, seed=1, backend=None, comm=None,
                 raw_fn=None, theta_map=None, missing=False):
        """missing=True (opt-in): NaN entries of the series are periods without an observation in every inner
        filter; the default backend is created that way, a backend given by the caller must have been (HipBackend(missing=True)).
        theta_map (optional): ThetaMap, the device-evaluable form of `model`; with a prior of enumerated families it
        moves rejuvenate! onto the device.  raw_fn (optional): vectorised shortcut for `model`: maps an [m, d_theta]
        array to (model_id, [m, n_raw] parameter rows) without building m model objects per evaluation."""
        self.N, self.M, self.model, self.prior, self.chain = int(N), int(M), model, prior, int(chain)
        if theta_map is not None and getattr(theta_map, "model_id", None) == _lib.MODEL_LG2D:
            from .models import _KALMAN_ONLY
            raise TypeError(_KALMAN_ONLY % "SMC")
        self.theta_map = theta_map
        if raw_fn is None and theta_map is not None:
            def raw_fn(th, _t=theta_map):
                return _t.model_id, _t.rows(th)
        self.raw_fn = raw_fn
        self.rng = np.random.default_rng(seed)
        self.seed = int(seed)
        if hasattr(prior, "rand_many"):
            self.theta = np.ascontiguousarray(prior.rand_many(self.rng, self.M), dtype=np.float64)
        else:
            self.theta = np.array([np.atleast_1d(prior.rand(self.rng)) for _ in range(self.M)], dtype=np.float64)
        self.logw = np.zeros(self.M)        # un-normalised outer log-weights; omega = their normalisation (property)
        self.logZ = np.zeros(self.M)
        self.ess = float(self.M)
        self.ess_min = self.M * float(ess_threshold)
        self.acc_threshold, self.acc_ratio = float(min_ar), 0.0
        self.backend = backend if backend is not None else HipBackend(missing=missing)
        if bool(missing) != bool(getattr(self.backend, "missing", False)):
            raise ValueError("SMC(missing=...) and the backend disagree: create the backend with the same missing=")
        self.missing = bool(missing)
        self.outer = getattr(self.backend, "outer", None) or LibOuter()
        self._outer_local = False           # True: only this rank's slice of logw / logZ is current (sharded online steps)
        self.prior_spec = prior.spec() if hasattr(prior, "spec") else None
        self.device_pmmh = (theta_map is not None and self.prior_spec is not None and hasattr(self.backend, "rejuvenate")
                            and self.theta.shape[1] == len(self.prior_spec[0]))
        self.comm = comm
        self.lo, self.hi = (0, self.M) if comm is None else comm.slice(self.M)
        self._calls = 0          # evaluation counter -> fresh Philox seed per batched evaluation
        self.psteps = 0          # executed inner particle-steps (all ranks), SURVEY 8(d)
        self.psteps_skipped = 0  # particle-steps of proposals outside the prior's support: never run (smc_samplers.jl:116)
        self.psteps_speculated = 0   # particle-steps the windows of smc2_run ran beyond the kept ones (dropped steps + the re-run prefix)
        self._main = None        # device handle of the online filters (smc2)
        self._theta_dev = None   # (handle, theta slice) whose parameter rows are on the device
        self.t = 0

    # -- batched inner filters --------------------------------------------------------------------
    def _next_seed(self):
        self._calls += 1
        return (self.seed << 20) + self._calls

    def _streams(self):
        return np.arange(self.lo, self.hi, dtype=np.uint32)

    def _gather(self, local):
        return local if self.comm is None else self.comm.all_gather(local)

    def _sync_outer(self):
        """after sharded online steps every rank has advanced only its own slice of logw / logZ: ONE all-gather brings the
        full vectors up to date everywhere (before resample!, summaries, and when a public call returns)"""
        if self._outer_local:
            per = self.hi - self.lo
            both = self._gather(np.concatenate([self.logw[self.lo:self.hi], self.logZ[self.lo:self.hi]])).reshape(-1, 2, per)
            self.logw = np.ascontiguousarray(both[:, 0, :].ravel())
            self.logZ = np.ascontiguousarray(both[:, 1, :].ravel())
            self._outer_local = False

    def _set_logw(self, logw):
        """reweight(logw) (smc_samplers.jl:232,298): the sampler's outer weights become exp(logw), normalised"""
        self.logw = np.array(logw, dtype=np.float64)
        self._outer_local = False
        _, _, self.ess = self.outer.reweight(self.logw, want_w=False)

    @property
    def omega(self):
        """the normalised outer weights (the reference's smc.ω after reweight): reweight(logw)[1]"""
        self._sync_outer()
        return self.outer.reweight(self.logw)[1]

    def _models(self, thetas):
        """smc.model(theta[m]) for a block of parameter particles (objects, or parameter rows via raw_fn)."""
        if self.raw_fn is not None:
            return RawModels(*self.raw_fn(np.asarray(thetas, dtype=np.float64)))
        return [self.model(th) for th in thetas]

    def _filter_all(self, thetas, y, key="prop", skip=None):
        """logZ[m] = log_likelihood(N, y, model(theta[m])) for every m: ONE batched GPU call per rank.
        skip[m]: that filter is not run (its logZ reads -inf) and not counted."""
        models = self._models(thetas[self.lo:self.hi])
        sk = None if skip is None else np.asarray(skip[self.lo:self.hi], dtype=bool)
        local, h = self.backend.log_likelihood(models, self.N, np.asarray(y, dtype=np.float64), self._next_seed(),
                                               self._streams(), key=key, skip=sk)
        nskip = 0 if skip is None else int(np.sum(skip))
        self.psteps += (self.M - nskip) * self.N * len(y)
        self.psteps_skipped += nskip * self.N * len(y)
        return self._gather(np.asarray(local)), h

    def __repr__(self):
        return "ess     = %.3f\nmean(theta) = %s" % (self.ess, np.array2string(expected_parameters(self)))


def expected_parameters(smc):
    """sum_m theta[m] * omega[m]   (smc_samplers.jl:61-65; omega normalised)"""
    if isinstance(smc, IBIS):
        return _ibis.expected_parameters(smc)
    w = smc.omega
    return (smc.theta * w[:, None]).sum(axis=0)


def posterior_moments(ibis):
    """(mean [d], cov [d][d]) of theta under the normalised outer weights of an IBIS sampler, reduced on the device (ibis.py)"""
    if not isinstance(ibis, IBIS):
        raise TypeError("posterior_moments is defined for an IBIS sampler")
    return _ibis.posterior_moments(ibis)


def _host_cloud_calls(smc):
    """the host twins over an SMC sampler's cloud: its theta lives on the host, its weights are log(omega)"""
    if not (hasattr(smc, "theta") and hasattr(smc, "omega")):
        raise TypeError("posterior_quantiles / posterior_histogram are defined for an IBIS or an SMC sampler")
    theta = np.ascontiguousarray(smc.theta, dtype=np.float64)
    with np.errstate(divide="ignore"):
        logw = np.log(smc.omega)
    return (lambda p: _lib.host_theta_quantiles(theta, logw, p),
            lambda c, lo, hi, bins: _lib.host_theta_histogram(theta, logw, c, lo, hi, bins), theta.shape[1])


def posterior_quantiles(smc, p):
    """the weighted quantiles of every parameter: [d] for a level p, [d][len(p)] for a list.  IBIS: selected on the device
    (ibis.py); SMC: the same specification on the host over smc.theta and log(smc.omega)"""
    if isinstance(smc, IBIS):
        return _ibis.posterior_quantiles(smc, p)
    return _ibis.quantiles_from(_host_cloud_calls(smc)[0], p)


def posterior_histogram(smc, component=None, bins=50, range=None, outside=False):
    """(mass [bins], edges [bins + 1]) of the marginal posterior of one parameter, or a list of d pairs (ibis.py
    posterior_histogram); SMC: the host twin over smc.theta and log(smc.omega)"""
    if isinstance(smc, IBIS):
        return _ibis.posterior_histogram(smc, component, bins, range, outside)
    return _ibis.histogram_from(*_host_cloud_calls(smc), component, bins, range, outside)


def _per_theta(smc, local):
    """[M_local, k] rows of per-filter summaries of this rank -> [M, k] on every rank"""
    local = np.ascontiguousarray(local, dtype=np.float64)
    if smc.comm is None:
        return local
    k = local.shape[1]
    return smc._gather(local.ravel()).reshape(smc.M, k)


class _literal_mode:
    """the online filters' handle in the unweighted summary mode (literal=True) for one block, weighted again afterwards"""

    def __init__(self, main, literal):
        self.main, self.literal = main, bool(literal)
        if self.literal and not hasattr(main, "set_summary_mode"):
            raise NotImplementedError("literal=True needs the device's unweighted summary mode (smc_set_summary_mode)")

    def __enter__(self):
        if self.literal:
            self.main.set_summary_mode("unweighted")

    def __exit__(self, *exc):
        if self.literal:
            self.main.set_summary_mode("weighted")


def filtered_summaries(smc, p=(0.25, 0.5, 0.75), component=0, literal=False):
    """(quantiles [len(p)], variance) of the filtered state of the online sampler, integrated over the parameter particles:
    per theta-particle the quantiles and variance of its x cloud, then their omega-weighted means.
    literal=False: the w-weighted summaries per filter (the inverse of the weighted empirical CDF in the filter's integer
    weights, smc_get_quantiles, and the uncorrected weighted variance) - the statistic of get_quantiles_uc
    (examples/inflation_example.jl:39-55), except that StatsBase's weighted quantile there INTERPOLATES between particles;
    that variant is not offered (StatsBase is not part of the reference tree, so it cannot be pinned).
    literal=True: get_quantiles_ucsv (:241-252) - per filter the UNWEIGHTED type-7 quantile(x_cloud, p) and the corrected
    var(x_cloud) of the cloud as the filter leaves it (the device's unweighted summary mode, smc_set_summary_mode).
    Either way the per-filter summaries are computed on the device: no cloud leaves the GPU.  One deviation remains in both:
    omega is the normalised one (the example multiplies by the raw smc.ω, all ones right after rejuvenate!: its sum is then M
    times the mean)."""
    if smc._main is None:
        raise ValueError("filtered_summaries needs the online sampler's filters (call smc2 first)")
    with _literal_mode(smc._main, literal):
        q = np.asarray(smc._main.quantiles(list(p), component))        # [M_local][len(p)]
        _, var = smc._main.moments()                                   # [d][M_local]
    return _integrate(smc.omega, _per_theta(smc, np.column_stack([q, np.asarray(var)[component]])))


def observation_dist(ibis, ahead=0, between=False):
    """observation_dist(ibis)   src/plotting_utils.jl:94-112 (an IBIS sampler only: ibis.py)"""
    if not isinstance(ibis, IBIS):
        raise TypeError("observation_dist is defined for an IBIS sampler (plotting_utils.jl:94)")
    return _ibis.observation_dist(ibis, ahead, between)


def quantile(ibis, p, ahead=0, total=False):
    """quantile(ibis, p)   src/plotting_utils.jl:128-137 (an IBIS sampler only: ibis.py; for SMC see filtered_summaries)"""
    if not isinstance(ibis, IBIS):
        raise TypeError("quantile is defined for an IBIS sampler (plotting_utils.jl:128); for SMC use filtered_summaries")
    return _ibis.quantile(ibis, p, ahead, total)


def filtered_state(ibis):
    """(xbar, Sbar, between) of an IBIS sampler's filtered state (ibis.py)"""
    if not isinstance(ibis, IBIS):
        raise TypeError("filtered_state is defined for an IBIS sampler")
    return _ibis.filtered_state(ibis)


def estimated_trend(smc):
    """estimated_trend(smc)   src/plotting_utils.jl:116-124:  sum_m omega[m] * mean(observation(model(theta[m]), w[m]' x[m])),
    with the NORMALISED omega (the reference uses smc.ω as it stands - all ones right after rejuvenate!; stated deviation).
    The filtered means w[m]' x[m] come from the device; mean(observation(.)) is B x for the linear model (ssm.jl:96-103),
    x[1] for UCSV (:244-247) and 0 for the stochastic-volatility model."""
    if isinstance(smc, IBIS):
        return _ibis.estimated_trend(smc)                              # plotting_utils.jl:114
    if smc._main is None:
        raise ValueError("estimated_trend needs the online sampler's filters (call smc2 first)")
    mean, _ = smc._main.moments()                                      # [d][M_local]
    mid, rows = _rows(smc._models(smc.theta[smc.lo:smc.hi]))
    if mid == _lib.MODEL_LG1D:
        obs = rows[:, 1] * np.asarray(mean)[0]
    elif mid in (_lib.MODEL_UCSV3D, _lib.MODEL_UCSV_RB):    # (the marginal family: row 0 is the trend's filtered mean)
        obs = np.asarray(mean)[0]
    else:
        obs = np.zeros(rows.shape[0])
    allobs = _per_theta(smc, obs[:, None])[:, 0]
    w = np.asarray(smc.omega, dtype=np.float64)
    keep = w > 0                     # a filter of no weight may have a NaN mean (collapsed): it does not enter (0 * NaN is NaN)
    return float(w[keep] @ allobs[keep])


def resample_(smc):
    """resample!(smc)   smc_samplers.jl:74-84 -- value-copy semantics."""
    if isinstance(smc, IBIS):
        return _ibis.resample_(smc)
    smc._sync_outer()
    # iid multinomial (sample(1:M, Weights(w), M)) through the integer CDF of the outer weights, pick numbers from Philox keyed
    # by the evaluation counter (the same on every rank).  The order of the resampled population carries no information (the
    # reference's `sample` returns it unsorted); taken in ascending order slot m inherits from an ancestor close to m, so with
    # theta sharded over GPUs most of the filter copies of the online sampler stay on their rank and only the drift of the
    # offspring counts crosses the links.
    a = np.asarray(smc.outer.resample(smc.logw, smc.M, smc._next_seed()), dtype=np.int64)
    smc.theta = smc.theta[a].copy()
    smc.logw = smc.logw[a].copy()
    smc.logZ = smc.logZ[a].copy()
    if smc._main is not None:
        if smc.comm is not None:
            smc.comm.exchange_slots(smc._main, a, smc.M)      # filters move between GPUs: one all-to-all
        else:
            smc._main.permute(a.astype(np.int32))
    return a


def random_walk_factor(theta, scales, outer=None):
    """(L, s) such that the proposal of chain position c is  theta' = theta + sqrt(s[c]) * L z,  z ~ N(0, I):
    multivariate theta (smc_samplers.jl:95-100): MvNormal(x, scale * Sigma), Sigma = 2.83^2/d * cov(theta) + 1e-10 I
      (1e-2 I when the cloud has collapsed, norm(cov) < 1e-8)  ->  L = chol(Sigma), s = scales;
    univariate theta (:87-92): Normal(x, scale * sigma) with sigma = 2.83^2 * var(theta) + 1e-10 (1e-2 when collapsed)
      handed over as the STANDARD DEVIATION  ->  L = [[sigma]], s = scales^2  (sqrt(s) = scale).
    Covariance and factorisation in the library's fixed order of operations (smc_host_rw_factor): the same bits on every rank."""
    scales = np.asarray(scales, dtype=np.float64)
    L, univariate = (outer or LibOuter).rw_factor(np.ascontiguousarray(theta, dtype=np.float64))
    return L, (scales * scales if univariate else scales)


def random_walk_kernel(theta, outer=None):
    """random_walk_kernel(theta)   smc_samplers.jl:87-101
    returns f(x, scale, rng) -> a draw of the reference's Normal(x, scale*sigma) / MvNormal(x, scale*Sigma)."""
    d = theta.shape[1]
    L, _ = random_walk_factor(theta, [1.0], outer)     # fixed now: theta is updated in place during the chain

    def eff(scale):
        return scale * scale if d == 1 else scale

    def kernel(x, scale, rng):
        return x + math.sqrt(eff(scale)) * (L @ rng.standard_normal(d))

    def many(th, scale, rng):
        """one proposal per row of th: the same normals, in the same order, as M calls of kernel()"""
        z = rng.standard_normal((th.shape[0], d))
        return th + math.sqrt(eff(scale)) * (z @ L.T)

    kernel.many = many
    return kernel


def rejuvenate_(smc, y, xi=1.0, verbose=False, out=sys.stdout):
    """rejuvenate!(smc, y, xi)   smc_samplers.jl:103-146 -- PMMH moves, `chain` per parameter particle.
    On the device in one call per rank when the sampler has a ThetaMap and an enumerated prior; otherwise the
    loop below with all M proposals of one chain position filtered in one batched call."""
    if isinstance(smc, IBIS):
        return _ibis.rejuvenate_(smc, y, xi, verbose, out)
    y = np.asarray(y, dtype=np.float64)
    if verbose:
        out.write("\t[rejuvenating]")
    if smc.device_pmmh:
        accepted = _rejuvenate_device(smc, y, xi)
    else:
        accepted = _rejuvenate_host(smc, y, xi)
    smc.logw = np.zeros(smc.M)          # smc.ω = ones(M): the moved particles are equally weighted
    smc._outer_local = False
    smc.acc_ratio = float(accepted.sum()) / smc.M
    if verbose:
        out.write("\tacc_rate: %1.5f" % smc.acc_ratio)
    return smc


def _rejuvenate_device(smc, y, xi):
    """The whole `for m ... for c in 1:chain` loop (smc_samplers.jl:112-138) in one smc_pmmh_rejuvenate call per rank;
    the host contributes the random-walk factor (:95-100, from the full theta cloud every rank holds) and, with
    sharded theta, ONE all-gather of the moved (theta, logZ, accepted) slices afterwards."""
    L, s = random_walk_factor(smc.theta, 0.5 * np.arange(smc.chain, 0, -1), smc.outer)     # 0.5*reverse(1:chain)
    seeds = np.array([smc._next_seed() for _ in range(smc.chain)], dtype=np.uint64)
    move_seed = smc._next_seed()
    lo, hi = smc.lo, smc.hi
    th, lz, acc, nrun = smc.backend.rejuvenate(smc.theta_map, smc.prior_spec, smc.N, y, float(xi), L, s, seeds, move_seed,
                                               smc._streams(), smc.theta[lo:hi], smc.logZ[lo:hi], smc._main)
    d = smc.theta.shape[1]
    packed = np.concatenate([np.asarray(th, dtype=np.float64).ravel(), lz, acc.astype(np.float64), [float(nrun)]])
    allp = smc._gather(packed).reshape(-1, packed.size)
    per = hi - lo
    smc.theta = np.ascontiguousarray(allp[:, :per * d].reshape(-1, d))
    smc.logZ = np.ascontiguousarray(allp[:, per * d:per * (d + 1)].ravel())
    accepted = allp[:, per * (d + 1):per * (d + 2)].ravel() != 0.0
    nrun_all = int(round(allp[:, -1].sum()))
    smc.psteps += nrun_all * smc.N * len(y)
    smc.psteps_skipped += (smc.M * smc.chain - nrun_all) * smc.N * len(y)
    return accepted


def _rejuvenate_host(smc, y, xi):
    kernel = random_walk_kernel(smc.theta, smc.outer)
    scales = 0.5 * np.arange(smc.chain, 0, -1)          # 0.5*reverse(1:chain)
    accepted = np.zeros(smc.M, dtype=bool)
    many = hasattr(smc.prior, "logpdf_many")
    for c in range(smc.chain):
        prop = kernel.many(smc.theta, scales[c], smc.rng)      # all M proposals of this chain position
        u = smc.rng.random(smc.M)
        if many:
            ok = smc.prior.insupport_many(prop)
            lp_prop, lp_cur = smc.prior.logpdf_many(np.where(ok[:, None], prop, smc.theta)), smc.prior.logpdf_many(smc.theta)
        else:
            ok = np.array([smc.prior.insupport(p) for p in prop])
            lp_prop = np.array([smc.prior.logpdf(p) if o else -math.inf for p, o in zip(prop, ok)])
            lp_cur = np.array([smc.prior.logpdf(q) for q in smc.theta])
        # a proposal outside the support is never filtered (smc_samplers.jl:116): its slot is skipped on the device
        # (the parameter row handed over for it is the current, valid theta; it is not read)
        safe = np.where(ok[:, None], prop, smc.theta)
        logZ_prop, hprop = smc._filter_all(safe, y, skip=~ok)
        with np.errstate(invalid="ignore"):
            acc_ratio = xi * (logZ_prop - smc.logZ) + (lp_prop - lp_cur)
        with np.errstate(divide="ignore"):
            acc = ok & (logZ_prop + lp_prop > -math.inf) & (np.log(u) < acc_ratio)
        smc.theta[acc] = prop[acc]
        smc.logZ[acc] = logZ_prop[acc]
        if smc._main is not None and acc[smc.lo:smc.hi].any():
            smc._main.copy_from(hprop, acc[smc.lo:smc.hi])      # x[m], w[m] <- x_prop, w_prop on the device
        accepted |= acc
    return accepted


def density_tempered(smc, y, verbose=True, out=sys.stdout):
    """density_tempered(smc, y)   smc_samplers.jl:222-281 (Duan & Fulop)."""
    if isinstance(smc, IBIS):
        return _ibis.density_tempered(smc, y, verbose, out)
    y = np.asarray(y, dtype=np.float64)
    smc.logZ, _ = smc._filter_all(smc.theta, y)
    smc._set_logw(smc.logZ)                               # :232
    xi = 0.0
    stages = []
    while xi < 1.0:
        # the bisection for the next exponent (:240-258) and the corner solution (:261-266), one library call:
        # ess == ess_min ends it, ess < ess_min lowers the upper end, else the lower end rises, until they are 1e-6 apart
        xi, smc.ess, resample_flag, smc.logw = smc.outer.temper(smc.logZ, xi, smc.ess_min)
        if verbose:
            out.write("ξ = %1.5f\tess = %4.3f" % (xi, smc.ess))
        if resample_flag:
            resample_(smc)
            rejuvenate_(smc, y, xi, verbose, out)
        stages.append((xi, smc.ess, smc.acc_ratio if resample_flag else None))
        if verbose:
            out.write("\n")
    return stages


def smc2(smc, y):
    """smc²(smc, y): initialisation at t = 1   smc_samplers.jl:288-301"""
    if isinstance(smc, IBIS):
        return _ibis.smc2(smc, y)
    y = np.asarray(y, dtype=np.float64)
    models = smc._models(smc.theta[smc.lo:smc.hi])
    logmu, smc._main = smc.backend.init(models, smc.N, float(y[0]), smc._next_seed(), smc._streams(), key="main")
    smc.psteps += smc.M * smc.N
    smc.logZ = smc._gather(np.asarray(logmu, dtype=np.float64)).copy()
    smc._set_logw(smc.logZ)                               # :297-298
    smc.t = 1
    return smc


def smc2_step(smc, y, t, verbose=True, out=sys.stdout):
    """smc²!(smc, y, t): online step for observation y[t] (1-based t as in the reference, t >= 2)
    smc_samplers.jl:308-340"""
    if isinstance(smc, IBIS):
        return _ibis.smc2_step(smc, y, t, verbose, out)
    y = np.asarray(y, dtype=np.float64)
    if verbose:
        out.write("t = %4d\tess = %4.3f" % (t - 1, smc.ess))
    if smc.ess < smc.ess_min:
        resample_(smc)
        rejuvenate_(smc, y[: t - 1], 1.0, verbose, out)
        _exchange(smc, y[: t - 1], verbose, out)
    _step_only(smc, y, t, verbose, out)
    smc._sync_outer()
    return smc


def _smoothed_blocks(smc, y, N, max_bytes, seed, **smoother_kw):
    """the s of particles.smoother for the sampler's current parameter cloud, block of parameter particles after block (their
    batch axes concatenate to [T][M]...): N particles per parameter particle (None: the sampler's N), blocks whose recorded
    history stays under max_bytes, filter m on Philox stream m under `seed` (None: derived from the sampler's seed).  The ONE
    block loop of smoothed_state and smoothed_quantiles: the same records, blocks and seeds for both."""
    from .particles import smoother
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    N = smc.N if N is None else int(N)
    mid, raw = _rows(smc._models(smc.theta))
    d = _lib.lib().smc_model_dim(int(mid))
    per_theta = y.size * N * (d + 2) * 8                  # recorded x and w, and the smoothed weights
    blk = max(1, min(smc.M, int(max_bytes) // max(per_theta, 1)))
    seed = ((smc.seed << 20) | 0xF5B00) if seed is None else int(seed)
    for m0 in range(0, smc.M, blk):
        m1 = min(smc.M, m0 + blk)
        yield smoother(N, y, None, rows=(int(mid), raw[m0:m1]), seed=seed, device=getattr(smc.backend, "device", 0),
                       streams=np.arange(m0, m1, dtype=np.uint32), **smoother_kw)[3]


def smoothed_quantiles(smc, y, p, component=0, N=None, max_bytes=2 ** 31, seed=None):
    """[T][len(p)]: per period, the omega-weighted average over the sampler's current parameter cloud of the per-filter weighted
    quantiles of state coordinate `component` under the smoothed weights (particles.smoother(..., quantiles=p): selected on the
    device in the backward pass) - the rule by which get_quantiles_ucsv (examples/inflation_example.jl:241-252) and
    filtered_summaries integrate the filtered ones, here for p(x_t | y_1:T).  Up to 8 levels in [0, 1].  Filters of omega = 0 are
    left out.  The records, blocks and seeds are smoothed_state's (N, max_bytes, seed as there), so the band belongs to its mean.
    IBIS is out of scope: its smoothed law is a mixture of normals with an exact quantile (rts_quantile)."""
    if isinstance(smc, IBIS):
        raise TypeError("smoothed_quantiles: IBIS is out of scope: its smoothed law is a mixture of normals, whose quantile is exact "
                        "(rts_quantile)")
    from .particles import _smooth_quantile_args
    mid, _ = _rows(smc._models(smc.theta))
    p = _smooth_quantile_args(p, component, None, (int(mid), None))
    q = np.concatenate([s["quantiles"] for s in _smoothed_blocks(smc, y, N, max_bytes, seed, quantiles=p, component=int(component))],
                       axis=1)                                                       # [T][M][np]
    om = np.asarray(smc.omega, dtype=np.float64)
    keep = om > 0
    return np.add.reduce(om[keep][None, :, None] * q[:, keep], axis=1)


def smoothed_state(smc, y, N=None, max_bytes=2 ** 31, seed=None):
    """(mean [T], var [T]) of p(x_t | y_1:T, theta) integrated over the sampler's current parameter cloud ([T][d] for a state of d
    coordinates): fresh batched smoothers (particles.smoother: a particle filter of N particles per parameter particle, default
    the sampler's N, and the FFBS backward pass) at the current theta, in blocks of parameter particles whose recorded history
    stays under max_bytes, then mean = sum_m omega_m mean_m and var = sum_m omega_m var_m (within) + sum_m omega_m (mean_m - mean)^2
    (between), as trend_moments combines a mixture.  Filters with omega = 0 are left out, as in filtered_summaries.  Filter m uses
    Philox stream m, so the result does not depend on the blocks; seed: the Philox seed of the filters (default: derived from the
    sampler's seed; the sampler's own state is not touched).  All parameter particles are smoothed on this process's GPU.
    IBIS is out of scope: its exact smoother is RTS, a different feature (rts_smoothed_state)."""
    if isinstance(smc, IBIS):
        raise TypeError("smoothed_state: IBIS is out of scope: its exact smoother is RTS, a different feature (rts_smoothed_state)")
    blocks = list(_smoothed_blocks(smc, y, N, max_bytes, seed))
    om = np.asarray(smc.omega, dtype=np.float64)
    mean_m = np.concatenate([s["mean"] for s in blocks], axis=1)                     # [T][M] or [T][M][d]
    var_m = np.concatenate([s["var"] for s in blocks], axis=1)
    keep = om > 0
    wk = om[keep].reshape((1, -1) + (1,) * (mean_m.ndim - 2))
    mean = np.add.reduce(wk * mean_m[:, keep], axis=1)
    within = np.add.reduce(wk * var_m[:, keep], axis=1)
    dev = mean_m[:, keep] - mean[:, None]
    between = np.add.reduce(wk * (dev * dev), axis=1)
    return mean, within + between


_U64 = 0xFFFFFFFFFFFFFFFF


def forecast_state(smc, H, quantiles=None, component=0, seed=None):
    """The forecast fan of an SMC sampler after smc2 / smc2_run, integrated over its parameter cloud: every online filter
    (smc._main) propagates its cloud H steps ahead on the device (particles.forecast) and the per-filter forecasts
    are combined with the normalised omega exactly as smoothed_state / filtered_summaries combine theirs.  A dict, [k] = horizon k + 1:
        "mean", "var"                [H] or [H][d]: mean = sum_m omega_m mean_m, var = within (sum_m omega_m var_m) + between
                                     (sum_m omega_m (mean_m - mean)^2)
        "obs_mean", "obs_var"        [H]: the predictive law of y, combined the same way
        "quantiles", "obs_quantiles" (quantiles=[...]) [H][len(p)]: the omega-weighted means of the per-filter weighted quantiles of
                                     state coordinate `component` / of the predictive draws (the statistic of filtered_summaries)
    The deviation stated at filtered_summaries holds here too: omega is the normalised one (the example multiplies by the raw
    smc.ω).  Filters of omega = 0 do not enter (a collapsed filter has NaN rows).  Filter m draws with Philox stream m, so the
    result does not depend on how theta is sharded; seed: the Philox seed of the forecast draws (default: derived from the
    sampler's seed).  The sampler and its filters are left as they were.
    An IBIS sampler has the exact one-step prediction instead: ahead=1 of observation_dist / quantile / smc2_run; a multi-step
    IBIS forecast is not offered."""
    if isinstance(smc, IBIS):
        raise TypeError("forecast_state is defined for an SMC sampler; IBIS has the exact one-step Kalman prediction: ahead=1 "
                        "(observation_dist, quantile, smc2_run)")
    if smc._main is None:
        raise ValueError("forecast_state needs the online sampler's filters (call smc2 first)")
    if not hasattr(smc._main, "forecast"):
        raise NotImplementedError("forecast_state needs the device's forecast (smc_forecast)")
    H = int(H)
    seed = (((smc.seed << 20) | 0xF0CA5) if seed is None else int(seed)) & _U64
    p = [] if quantiles is None else list(quantiles)
    r = smc._main.forecast(H, seed, p=p or None, component=component, obs=True)
    d, per, nq = r["mean"].shape[1], r["mean"].shape[2], len(p)
    # per filter: mean [H][d] | var [H][d] | obs_mean [H] | obs_var [H] | q [H][nq] | obs_q [H][nq]
    cols = [np.moveaxis(r["mean"], 2, 0).reshape(per, H * d), np.moveaxis(r["var"], 2, 0).reshape(per, H * d), r["obs_mean"].T, r["obs_var"].T]
    if nq:
        cols += [np.moveaxis(r["q"], 1, 0).reshape(per, H * nq), np.moveaxis(r["obs_q"], 1, 0).reshape(per, H * nq)]
    rows = _per_theta(smc, np.column_stack(cols))                       # [M][...]
    om = np.asarray(smc.omega, dtype=np.float64)
    head, last = _integrate(om, rows)
    tot = np.append(head, last)
    o = np.cumsum([0, H * d, H * d, H, H, H * nq, H * nq])
    mean, within = tot[o[0]:o[1]], tot[o[1]:o[2]]
    omean, owithin = tot[o[2]:o[3]], tot[o[3]:o[4]]
    keep = om > 0
    dev = rows[keep][:, o[0]:o[1]] - mean
    odev = rows[keep][:, o[2]:o[3]] - omean
    between = np.add.reduce(om[keep, None] * (dev * dev), axis=0)
    obetween = np.add.reduce(om[keep, None] * (odev * odev), axis=0)
    shape = (H,) if d == 1 else (H, d)
    out = {"mean": mean.reshape(shape), "var": (within + between).reshape(shape), "obs_mean": omean, "obs_var": owithin + obetween}
    if nq:
        out["quantiles"], out["obs_quantiles"] = tot[o[4]:o[5]].reshape(H, nq), tot[o[5]:o[6]].reshape(H, nq)
    return out


def _path_counts(smc, M, seed):
    """(counts [smc.M] int32, the parameter particles with a positive count): the parameter particle of each of M paths drawn from
    omega through the library's own outer resampler (M ancestors in ascending order)"""
    smc._sync_outer()
    anc = np.asarray(_lib.host_outer_resample(smc.logw, M, (seed + 1) & _U64), dtype=np.int64)
    counts = np.bincount(anc, minlength=smc.M).astype(np.int32)
    return counts, np.flatnonzero(counts)


def _greedy_blocks(counts, nbytes, max_bytes):
    """yields (b0, b1, cmax): consecutive blocks of the filters with path counts `counts`, each as long as nbytes(filters, largest
    count) stays within max_bytes (a block holds at least one filter); every filter of a block holds cmax path slots"""
    b0 = 0
    while b0 < counts.size:
        b1, cmax = b0, 0
        while b1 < counts.size:
            c = max(cmax, int(counts[b1]))
            if b1 > b0 and nbytes(b1 + 1 - b0, c) > int(max_bytes):
                break
            b1, cmax = b1 + 1, c
        yield b0, b1, cmax
        b0 = b1


def smoothed_paths(smc, y, M, N=None, max_bytes=2 ** 31, seed=None):
    """M trajectories [T][M] ([T][M][d] for a state of d coordinates) from p(x_1:T | y_1:T) integrated over the sampler's current
    parameter cloud, by backward simulation (particles.smoother(paths=...)): the parameter particle of every path
    is drawn from omega through the library's own outer resampler (host_outer_resample: M ancestors in ascending order, so the
    paths of one parameter particle are neighbours), which gives a count per parameter particle; fresh batched recorded filters
    (N particles each, default the sampler's N) run only over the parameter particles with a positive count, in blocks whose
    record and paths stay under max_bytes, and filter m draws its count of paths.  Filter m uses Philox stream m, so the result
    does not depend on the blocks; particles with omega = 0 are never drawn.  seed: the Philox seed of the filters, of the
    ancestors and of the walk (default: derived from the sampler's seed; the sampler's own state is not touched).
    IBIS is out of scope: its exact smoother is RTS, a different feature (rts_smoothed_paths)."""
    if isinstance(smc, IBIS):
        raise TypeError("smoothed_paths: IBIS is out of scope: its exact smoother is RTS, a different feature (rts_smoothed_paths)")
    from .particles import smoother
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    M = int(M)
    if M < 1:
        raise ValueError("M must be positive")
    N = smc.N if N is None else int(N)
    seed = (((smc.seed << 20) | 0xBAC45) if seed is None else int(seed)) & _U64       # (one 64-bit word for the filters as well)
    counts, used = _path_counts(smc, M, seed)
    mid, raw = _rows(smc._models(smc.theta))
    d = _lib.lib().smc_model_dim(int(mid))
    out = np.zeros((y.size, M, d))
    first = np.concatenate([[0], np.cumsum(counts)])                  # path slots of parameter particle m: first[m] .. first[m + 1]
    for b0, b1, cmax in _greedy_blocks(counts[used], lambda k, c: k * y.size * (N * (d + 1) * 8 + c * (4 + 8 * d)), max_bytes):
        ms = used[b0:b1]
        _, _, _, s = smoother(N, y, None, rows=(int(mid), raw[ms]), seed=seed, device=getattr(smc.backend, "device", 0),
                              streams=ms.astype(np.uint32), paths=cmax, path_seed=(seed + 2) & _U64, path_counts=counts[ms], smooth=False)
        xs = s["paths"].reshape(y.size, ms.size, cmax, d)
        for k, m in enumerate(ms):
            out[:, first[m]:first[m + 1]] = xs[:, k, :counts[m]]
    return out[..., 0] if d == 1 else out


def rb_smoothed_state(smc, y, M, N=None, max_bytes=2 ** 31, seed=None):
    """The smoothed trend and volatilities of a sampler over MarginalUCSV, integrated over its current parameter cloud by
    Rao-Blackwellised backward simulation (particles.rb_smoother): a dict with "trend_mean", "trend_var" [T],
    "vol_mean", "vol_var" [T][2] and "n_paths" [T].  The parameter particle of each of the M paths is drawn from omega through the
    library's own outer resampler, as smoothed_paths draws it, which gives a count per parameter particle; fresh batched recorded
    filters (N particles each, default the sampler's N) run over the parameter particles with a positive count, in blocks whose
    record and paths stay under max_bytes, and filter m draws its count of paths.  Every complete path weighs the same: with
    c_m complete paths of parameter particle m, mean = sum c_m mean_m / sum c_m and var = within + between of that mixture, for
    the trend var = sum c_m (within_m + between_m + (mean_m - mean)^2) / sum c_m.  Filter m uses Philox stream m, so the result
    does not depend on the blocks.  seed: the Philox seed of the filters, the ancestors and the walk (default: derived from the
    sampler's seed; the sampler's own state is not touched)."""
    if isinstance(smc, IBIS):
        raise TypeError("rb_smoothed_state: IBIS is out of scope: its exact smoother is RTS (rts_smoothed_state)")
    from .particles import rb_smoother
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    M = int(M)
    if M < 1:
        raise ValueError("M must be positive")
    N = smc.N if N is None else int(N)
    mid, raw = _rows(smc._models(smc.theta))
    if int(mid) != _lib.MODEL_UCSV_RB:
        raise TypeError("rb_smoothed_state needs a sampler over MarginalUCSV; the other families have smoothed_state")
    seed = (((smc.seed << 20) | 0x4B5A7) if seed is None else int(seed)) & _U64
    counts, used = _path_counts(smc, M, seed)
    T = y.size
    outs = np.zeros((T, used.size, 8))
    for b0, b1, cmax in _greedy_blocks(counts[used], lambda k, c: k * T * (N * 5 * 8 + c * (4 + 8 * 4)), max_bytes):
        ms = used[b0:b1]
        h_res = rb_smoother(N, y, None, rows=(int(mid), raw[ms]), seed=seed, device=getattr(smc.backend, "device", 0),
                            streams=ms.astype(np.uint32), paths=cmax, path_seed=(seed + 2) & _U64, path_counts=counts[ms])[3]
        outs[:, b0:b1, 0] = h_res["trend_mean"]
        outs[:, b0:b1, 1] = h_res["trend_var"]
        outs[:, b0:b1, [3, 5]] = h_res["vol_mean"]
        outs[:, b0:b1, [4, 6]] = h_res["vol_var"]
        outs[:, b0:b1, 7] = h_res["n_paths"]
    return _rb_combine(outs)


def _rb_combine(outs):
    """the mixture over filters of per-filter (mean, variance) pairs weighted by their numbers of complete paths; outs [T][K][8]:
    columns 0, 1 the trend's mean and total variance, (3, 4) and (5, 6) those of lse and lsn, 7 the count.  Summed in index order"""
    c = outs[..., 7]
    keep = c > 0                                                      # (a filter without a complete path has NaN moments)
    tot = np.add.reduce(c, axis=1)
    res = {"n_paths": tot}
    cols = {}
    for name, (im, iv) in (("trend", (0, 1)), ("lse", (3, 4)), ("lsn", (5, 6))):
        mk, vk = np.where(keep, outs[..., im], 0.0), np.where(keep, outs[..., iv], 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.add.reduce(c * mk, axis=1) / tot
            dev = np.where(keep, mk - mean[:, None], 0.0)
            var = np.add.reduce(c * (vk + dev * dev), axis=1) / tot
        cols[name] = (mean, var)
    res["trend_mean"], res["trend_var"] = cols["trend"]
    res["vol_mean"] = np.stack([cols["lse"][0], cols["lsn"][0]], axis=-1)
    res["vol_var"] = np.stack([cols["lse"][1], cols["lsn"][1]], axis=-1)
    return res


def _integrate(w, rows):
    """[M][np + 1] per-filter (quantiles | variance) rows of every rank -> their omega-weighted means (quantiles [np], variance);
    the products summed over the parameter particles in index order (one definition for every caller: no BLAS in between).
    Only filters with omega > 0 enter: a filter of no weight may have NaN rows (a collapsed filter), and 0 * NaN is NaN"""
    w = np.asarray(w, dtype=np.float64)
    keep = w > 0
    tot = np.add.reduce(w[keep, None] * np.ascontiguousarray(rows, dtype=np.float64)[keep], axis=0)
    return tot[:-1], float(tot[-1])


def _window_summaries(smc, t, lik_local, j, logw_local):
    """the integrated filtered summaries (filtered_summaries) after each of the j kept steps of a window, from the per-step
    per-filter summaries the window launch recorded on the device: [(t + i, quantiles [np], variance)] - what the loop
    `smc²!(smc, y, t); push!(..., get_quantiles_uc(smc))` of examples/inflation_example.jl:39-55,78-86 collects per period.
    logw_local: this rank's outer log-weights BEFORE the window (the weights of step i follow by the window's own additions)."""
    comp = smc._summ["component"]
    q, _, var = smc._main.get_summaries(j)                      # [j][M_local][np], [j][d][M_local]
    nq, per = q.shape[2], q.shape[1]
    lw = np.array(logw_local, dtype=np.float64)
    blocks = []
    for i in range(j):
        lw = lw + lik_local[i]                                   # == smc_host_outer_advance, step by step
        blocks.append(np.concatenate([lw, q[i].ravel(), var[i][comp]]))
    flat = np.concatenate(blocks)
    allf = smc._gather(flat).reshape(-1, j, per * (nq + 2))      # [ranks][j][...]
    rows = []
    for i in range(j):
        logw = np.concatenate([allf[r, i, :per] for r in range(allf.shape[0])])
        qq = np.concatenate([allf[r, i, per:per * (nq + 1)].reshape(per, nq) for r in range(allf.shape[0])])
        vv = np.concatenate([allf[r, i, per * (nq + 1):] for r in range(allf.shape[0])])
        qi, vi = _integrate(smc.outer.reweight(logw)[1], np.column_stack([qq, vv]))
        rows.append((t + i, qi, vi))
    return rows


def smc2_run(smc, y, t_from, t_to, window=16, verbose=True, out=sys.stdout, summaries=None, component=0, literal=False, ahead=0):
    """for t in t_from:t_to  smc²!(smc, y, t)  end   (the online loop of smc_samplers.jl:308-340 / README.md:93-101),
    with the same results bit for bit, but up to `window` propagation steps per device call: between two
    resample-move decisions the inner filters only need y[t], so a window of steps runs in ONE launch with the particle
    clouds resident in LDS (smc_step_window), the host then walks through the window's outer ESS values exactly as
    smc²! would, and keeps the steps up to (and including) the first one whose ESS falls below the threshold
    (smc_step_commit; the speculated steps behind it are dropped and redone after the resample-move).
    With sharded theta a window costs ONE all-gather of segment records (LibOuter.window_walk) instead of one exchange per step.
    summaries=[p...] (optional): additionally collect, after every step, what the example's loop collects per period
    (examples/inflation_example.jl:78-86: get_quantiles_uc(smc) after each smc²!) - filtered_summaries(smc, p, component) -
    from per-step summaries recorded on the device inside the window launches; returned as smc.summary_trace =
    [(t, quantiles [len(p)], variance)], bit-identical to calling filtered_summaries after every smc2_step.
    literal=True: the summaries are filtered_summaries(..., literal=True) (unweighted per-filter quantiles, corrected variance)."""
    if isinstance(smc, IBIS):
        return _ibis.smc2_run(smc, y, t_from, t_to, window, verbose, out, summaries, ahead)   # (summaries: observation_dist per period)
    y = np.asarray(y, dtype=np.float64)
    t = int(t_from)
    smc._summ = None if summaries is None else {"p": [float(v) for v in summaries], "component": int(component), "literal": bool(literal)}
    if smc._summ and literal and smc._main is not None:
        _literal_mode(smc._main, True)                                   # (fails here, not mid-run, where the mode does not exist)
    smc.summary_trace = []
    while t <= t_to:
        k = min(int(window), t_to - t + 1)
        if k <= 1 or not getattr(smc._main, "can_window", False):
            smc2_step(smc, y, t, verbose, out)
            if smc._summ:
                qq, vv = filtered_summaries(smc, smc._summ["p"], smc._summ["component"], smc._summ["literal"])
                smc.summary_trace.append((t, qq, vv))
            t += 1
            continue
        if verbose:
            out.write("t = %4d\tess = %4.3f" % (t - 1, smc.ess))
        if smc.ess < smc.ess_min:
            resample_(smc)
            rejuvenate_(smc, y[: t - 1], 1.0, verbose, out)
            _exchange(smc, y[: t - 1], verbose, out)
            if not getattr(smc._main, "can_window", False):     # exchange! may have outgrown the resident kernel
                _step_only(smc, y, t, verbose, out)
                if smc._summ:
                    smc._sync_outer()
                    qq, vv = filtered_summaries(smc, smc._summ["p"], smc._summ["component"], smc._summ["literal"])
                    smc.summary_trace.append((t, qq, vv))
                t += 1
                continue
        _sync_params(smc)
        if smc._summ:
            smc._main.set_summaries(smc._summ["p"], smc._summ["component"], moments=True)
        try:
            with _literal_mode(smc._main, smc._summ is not None and smc._summ["literal"]):
                lik, _ = smc._main.step_window(y[t - 1: t - 1 + k])      # [k][M_local]
                lik = np.asarray(lik, dtype=np.float64)
                logw_before = smc.logw[smc.lo:smc.hi].copy()
                ess, j = smc.outer.window_walk(smc, lik, smc.ess_min)
                if smc._summ:
                    smc.summary_trace.extend(_window_summaries(smc, t, lik, j, logw_before))
        finally:
            if smc._summ:
                smc._main.set_summaries()                                # (the traces are read: recording off again)
        smc.ess = float(ess[-1])
        smc.t = t + j - 1
        if verbose:
            out.write("\n" + "".join("t = %4d\tess = %4.3f\n" % (t + i, ess[i]) for i in range(j - 1)))
        smc._main.step_commit(j)
        smc.psteps += smc.M * smc.N * j
        smc.psteps_speculated += smc.M * smc.N * ((k - j) + (j if j < k else 0))   # dropped steps + the prefix smc_step_commit re-runs
        t += j
    smc._sync_outer()
    return smc


def _sync_params(smc):
    """the parameter rows on the device follow theta (resample!/rejuvenate! change it); unchanged -> no upload"""
    th_loc = smc.theta[smc.lo:smc.hi]
    if smc._theta_dev is None or smc._theta_dev[0] is not smc._main or not np.array_equal(smc._theta_dev[1], th_loc):
        smc._main.set_params(_rows(smc._models(th_loc))[1])
        smc._theta_dev = (smc._main, th_loc.copy())


def _step_only(smc, y, t, verbose, out):
    """the propagation half of smc²! (smc_samplers.jl:323-338), without the degeneracy check"""
    _sync_params(smc)
    lik, _ = smc._main.step(float(y[t - 1]))
    smc.psteps += smc.M * smc.N
    ess, _ = smc.outer.window_walk(smc, np.asarray(lik, dtype=np.float64)[None, :], 0.0)
    smc.ess = float(ess[0])
    smc.t = t
    if verbose:
        out.write("\n")
    return smc


def _exchange(smc, y, verbose, out):
    """exchange!(smc, y)   smc_samplers.jl:163-189 (off unless min_ar > acceptance ratio; default -1)."""
    if smc.acc_ratio < smc.acc_threshold:
        if smc.N <= 4096:
            smc.N *= 2
            if verbose:
                out.write("\t%d particles added" % smc.N)
            models = smc._models(smc.theta[smc.lo:smc.hi])
            new_logZ, h = smc.backend.log_likelihood(models, smc.N, y, smc._next_seed(), smc._streams(), key="main")
            new_logZ = smc._gather(np.asarray(new_logZ, dtype=np.float64))
            smc.psteps += smc.M * smc.N * len(y)
            old, smc._main = smc._main, h
            smc._theta_dev = None
            if old is not None and old is not h and hasattr(smc.backend, "release"):
                smc.backend.release(old)          # the superseded N-particle filters
            smc._sync_outer()
            smc._set_logw(np.asarray(new_logZ) - smc.logZ)          # :183
            smc.logZ = np.asarray(new_logZ, dtype=np.float64).copy()
        else:
            out.write("\n\t[cannot exceed max state particles]")
