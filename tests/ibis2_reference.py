"""TEST INFRASTRUCTURE: tests/ibis_reference.py (src/ibis.jl statement by statement) for a sampler over two-state rows, with the
library's own host twins as the pieces: smc_host_kalman2_steps is the filter, smc_host_pmmh_propose / smc_host_pmmh_log_uniform /
smc_host_prior_logpdf / smc_host_rw_factor the move, smc_host_outer_* the outer level.  Python loops over m and c; nothing is
vectorised that could change an order of operations.  No GPU.  Never imported by the product."""
import numpy as np

from sequential_monte_carlo_amd import _lib as L
import kalman2_reference as k2


def pmmh_propose(move_seed, m, c, theta, chol, scale):
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    chol = np.ascontiguousarray(chol, dtype=np.float64)
    prop = np.zeros(theta.size)
    L.check(L.lib().smc_host_pmmh_propose(theta.size, int(move_seed), int(m), int(c), L._d(theta), L._d(chol), float(scale), L._d(prop)))
    return prop


def pmmh_log_uniform(move_seed, m, c):
    return L.lib().smc_host_pmmh_log_uniform(int(move_seed), int(m), int(c))


def prior_logpdf(fam, par, x):
    """logpdf of one component, -inf outside its support"""
    par = np.ascontiguousarray(par, dtype=np.float64)
    return L.lib().smc_host_prior_logpdf(int(fam), L._d(par), float(x))


def kalman2(row, y, predict_first, state=None):
    """(x [2], S [3], logZ): the steps of y from the row's initial state, or from `state` = (x, S) - logZ the step values summed in
    step order from 0.0"""
    row = np.array(row, dtype=np.float64)
    if state is not None:
        row[10:12], row[12:15] = state
    xf, Sf, lik = L.host_kalman2_steps(row, y, predict_first)
    z = 0.0
    for v in lik:
        z = z + float(v)
    return xf[-1].copy(), Sf[-1].copy(), z


class Ibis2Reference:
    def __init__(self, M, tmap, prior, chain, ess_threshold, seed=1, predict_first=False):
        self.M, self.tmap, self.chain, self.predict_first = int(M), tmap, int(chain), bool(predict_first)
        spec = prior.spec()
        self.fam, self.par = np.atleast_1d(spec[0]), np.atleast_2d(spec[1])
        rng = np.random.default_rng(seed)                                            # the cloud of smc.IBIS for this seed
        if hasattr(prior, "rand_many"):
            self.theta = np.ascontiguousarray(prior.rand_many(rng, self.M), dtype=np.float64)
        else:
            self.theta = np.array([np.atleast_1d(prior.rand(rng)) for _ in range(self.M)], dtype=np.float64)   # ibis.jl:35
        self.d = self.theta.shape[1]
        rows = tmap.rows(self.theta)                                                  # mods = model.(θ)            :38
        self.x, self.S = rows[:, 10:12].copy(), rows[:, 12:15].copy()                 # :39-40
        self.logZ, self.logw = np.zeros(self.M), np.zeros(self.M)                     # :42
        self.ess, self.ess_min = float(self.M), self.M * float(ess_threshold)         # :43-44
        self.seed, self._calls = int(seed), 0
        self.acc_ratio, self.accepted = 0.0, np.zeros(self.M, dtype=bool)
        self.ess_trace = []
        self.n_rejuvenations = self.n_out_of_support = self.n_accepted = self.n_rejected = 0
        self.first_ancestors = None          # the ancestors of the first resample!
        self.t = 0

    def _next_seed(self):
        self._calls += 1
        return (self.seed << 20) + self._calls

    def _row(self, th):
        return self.tmap.rows(np.asarray(th, dtype=np.float64)[None, :])[0]

    def _propagate(self, y_t, predict):
        """:135-141 / :171-181 - one Kalman step per parameter particle, then reweight (:144 / :187)"""
        lik = np.zeros(self.M)
        for m in range(self.M):
            self.x[m], self.S[m], lik[m] = kalman2(self._row(self.theta[m]), [y_t], predict, (self.x[m], self.S[m]))
        rec = L.host_outer_window(self.logw, lik[None, :])                            # logω += lik; logZ += lik; reweight
        ess, _ = L.host_outer_walk(rec, self.M, 0.0)
        self.logw, self.logZ = L.host_outer_advance(self.logw, self.logZ, lik[None, :], 1)
        self.ess = float(ess[0])
        self.ess_trace.append(self.ess)

    def smc2(self, y):                                                                # smc²(ibis, y)   :134-147
        self._propagate(float(y[0]), self.predict_first)
        self.t = 1

    def resample(self, logw=None):                                                    # resample!       :73-84
        a = np.asarray(L.host_outer_resample(self.logw if logw is None else logw, self.M, self._next_seed()))
        if self.first_ancestors is None:
            self.first_ancestors = a.copy()
        self.theta, self.logw = self.theta[a].copy(), self.logw[a].copy()
        self.x, self.S, self.logZ = self.x[a].copy(), self.S[a].copy(), self.logZ[a].copy()
        return a

    def rejuvenate(self, y, xi=1.0, move_seed=None, chol=None, s=None):               # rejuvenate!     :86-125
        y = np.asarray(y, dtype=np.float64)
        acc_array = np.zeros(self.M, dtype=bool)                                      # :87
        if chol is None:
            chol, uni = L.host_rw_factor(self.theta)                                  # pmmh_kernel = ibis.kernel(ibis.θ)   :90
            scales = 0.5 * np.arange(self.chain, 0, -1)                               # :91
            s = scales * scales if uni else scales
        move_seed = self._next_seed() if move_seed is None else move_seed
        for m in range(self.M):                                                       # :95
            for c in range(self.chain):                                               # :96
                prop = pmmh_propose(move_seed, m, c, self.theta[m], chol, s[c])       # :97
                lps = [prior_logpdf(self.fam[i], self.par[i], prop[i]) for i in range(self.d)]
                if not all(v > -np.inf for v in lps):                                 # insupport      :99
                    self.n_out_of_support += 1
                    continue
                x_prop, s_prop, logZ_prop = kalman2(self._row(prop), y, self.predict_first)       # :100
                lp_prop = lp_cur = 0.0
                for i in range(self.d):
                    lp_prop = lp_prop + lps[i]
                    lp_cur = lp_cur + prior_logpdf(self.fam[i], self.par[i], self.theta[m, i])
                prior_ratio = lp_prop - lp_cur                                        # :102
                likelihood_ratio = xi * (logZ_prop - self.logZ[m])                    # :103
                log_post_prop = logZ_prop + lp_prop                                   # :105
                acc_ratio = likelihood_ratio + prior_ratio                            # :106
                if log_post_prop > -np.inf and pmmh_log_uniform(move_seed, m, c) < acc_ratio:     # :108
                    self.logZ[m] = logZ_prop                                          # :109-112
                    self.theta[m] = prop
                    self.x[m] = x_prop
                    self.S[m] = s_prop
                    acc_array[m] = True                                               # :114
                    self.n_accepted += 1
                else:
                    self.n_rejected += 1
            self.logw[m] = 0.0                                                        # ibis.ω[m] = 1.0   :118
        self.accepted = acc_array
        self.acc_ratio = float(acc_array.sum()) / self.M                              # :121
        self.n_rejuvenations += 1

    def smc2_step(self, y, t):                                                        # smc²!(ibis, y, t)   :154-189
        if self.ess < self.ess_min:                                                   # :158
            self.resample()                                                           # :160
            self.rejuvenate(y[: t - 1])                                               # :163
        self._propagate(float(y[t - 1]), True)                                        # :166-187
        self.t = t

    def run(self, y):
        self.smc2(y)
        for t in range(2, len(y) + 1):
            self.smc2_step(y, t)
        return self

    def density_tempered(self, y):
        """the loop of smc_samplers.jl:222-281 with the exact Kalman log-likelihood per parameter particle -> the ξ ladder"""
        y = np.asarray(y, dtype=np.float64)
        for m in range(self.M):
            self.x[m], self.S[m], self.logZ[m] = kalman2(self._row(self.theta[m]), y, self.predict_first)
        self.logw = self.logZ.copy()
        _, _, self.ess = L.host_reweight(self.logZ, want_w=False)                     # :232
        self.t = len(y)
        xi, ladder = 0.0, []
        while xi < 1.0:
            xi, self.ess, flag, logw = L.host_outer_temper(self.logZ, xi, self.ess_min)   # :240-266
            if flag:
                self.resample(logw)
                self.rejuvenate(y, xi)
            else:
                self.logw = logw
            ladder.append((xi, self.ess, self.acc_ratio if flag else None))
        return ladder

    def expected_parameters(self):
        w = L.host_reweight(self.logw)[1]
        return (self.theta * w[:, None]).sum(axis=0)


# ---- the cases the two-state IBIS tests share -------------------------------------------------------------------------------
T_HP = 60


def y_hp():
    return k2.hp_series(T_HP)


def case_hp_one(smc):
    """theta = Q11 = 1 / lambda of the Hodrick-Prescott row of y_hp() (init_cov 1000); everything else fixed in the ThetaMap.
    Prior Uniform(0, 0.6): the posterior is computable on a grid, and a random walk started near either end of the support
    proposes outside it"""
    y = y_hp()
    const = k2.hp_row(y, 1600.0, 1000.0)
    const[6] = 0.0
    tmap = smc.ThetaMap(L.MODEL_LG2D, [-1] * 6 + [0] + [-1] * 8, const)
    return tmap, smc.product_distribution([smc.Uniform(0.0, 0.6)]), (lambda th: smc.hodrick_prescott(lam=1.0 / th[0], y=y))


def case_ar2_three(smc):
    """theta = (A11, A12, Q11) of an AR(2) trend observed with noise: A = [A11 A12; 1 0], B = (1, 0), Q = diag(Q11, 0), R = 1,
    x0 = 0, Sigma0 = 4 I; a Uniform prior on A12"""
    const = np.array([0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 4.0, 0.0, 4.0])
    tmap = smc.ThetaMap(L.MODEL_LG2D, [0, 1, -1, -1, -1, -1, 2] + [-1] * 8, const)
    prior = smc.product_distribution([smc.TruncatedNormal(0.5, 0.5, -1.5, 1.5), smc.Uniform(-0.6, 0.2), smc.LogNormal(-1.0, 0.7)])
    model = lambda th: smc.MultivariateLinearGaussian(A=[[th[0], th[1]], [1.0, 0.0]], B=[[1.0, 0.0]], Q=[[th[2], 0.0], [0.0, 0.0]], R=[1.0],
                                                      Sigma0=4.0 * np.eye(2))
    return tmap, prior, model


def grid_posterior_q(y, n=1201, lo=0.0, hi=0.6):
    """posterior mean and sd of theta = Q11 in case_hp_one by trapezoid quadrature on a grid, the likelihood from the longdouble
    restatement (all grid rows in one elementwise pass); the prior is flat on [lo, hi]"""
    grid = np.linspace(lo, hi, n).astype(np.longdouble)
    row = [np.full(n, v, dtype=np.longdouble) for v in k2.hp_row(y, 1600.0, 1000.0)]
    row[6] = grid
    lp = k2.filter_ld(row, y, False)[2].sum(axis=0)
    w = np.exp(lp - lp.max())
    w[0] *= 0.5
    w[-1] *= 0.5
    w /= w.sum()
    mean = float(w @ grid)
    return mean, float(np.sqrt(w @ (grid - mean) ** 2))
