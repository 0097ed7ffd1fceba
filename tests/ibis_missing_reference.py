"""TEST INFRASTRUCTURE: IbisReference (tests/ibis_reference.py) restated with gaps - a NaN observation is a period without one
(SMC_FLAG_NAN_MISSING on the exact-Kalman side) - bit for bit, from the unchanged oracle.

  an observed step   ob.kalman_log_likelihood([A, B, Q, R, x, S], [y_t], predict), as IbisReference takes it
  a gap              the oracle's own prediction, taken from its step with an INFINITE observation variance:
                     ob.kalman_log_likelihood([A, B, Q, inf, x, S], [0.0], True)[:2] - s = inf, so the gain times 1 / s is 0 and the
                     update adds 0 to x and takes 0 from S: (A x, (A A) S + Q) bit for bit, up to the sign of an exact zero
                     (x = 0, A < 0), which == treats alike.  The step's value is replaced by +0.0.  With predict false: nothing.

A series is the loop of these steps with logZ summed in step order from 0.0 - for a series without a NaN the number the
oracle's whole-series call gives.  Never imported by the product."""
import math

import numpy as np

from oracle import binding as ob
from ibis_reference import IbisReference


def gap_step(row, x, S, y_t, predict):
    """one step of the flagged filter from (x, S) under row = (A, B, Q, R, ..) -> (x, S, value)"""
    if y_t != y_t:
        if not predict:
            return x, S, 0.0
        xp, Sp, _ = ob.kalman_log_likelihood([row[0], row[1], row[2], math.inf, x, S], [0.0], predict_first=True)
        return xp, Sp, 0.0
    return ob.kalman_log_likelihood([row[0], row[1], row[2], row[3], x, S], [y_t], predict_first=predict)


def gap_series(row, y, predict_first, record=False):
    """(x_T, S_T, logZ) of the flagged filter over y from (x0, sigma0) = row[4:6]; record=True: also xf, Sf, lik [T]"""
    x, S, logZ = float(row[4]), float(row[5]), 0.0
    xf, Sf, lik = np.zeros(len(y)), np.zeros(len(y)), np.zeros(len(y))
    for t, y_t in enumerate(y):
        x, S, l = gap_step(row, x, S, float(y_t), bool(predict_first) or t > 0)
        logZ = logZ + l
        xf[t], Sf[t], lik[t] = x, S, l
    return (x, S, logZ, xf, Sf, lik) if record else (x, S, logZ)


class IbisMissingReference(IbisReference):
    """IbisReference with every Kalman step replaced by gap_step: online, in the re-filter of rejuvenate! and in the first pass
    of density_tempered.  Nothing else differs (the statements below are IbisReference's)."""

    def _propagate(self, y_t, predict):
        lik = np.zeros(self.M)
        for m in range(self.M):
            self.x[m], self.S[m], lik[m] = gap_step(self._row(self.theta[m]), self.x[m], self.S[m], y_t, predict)
        self.logw, self.logZ, ess, _ = ob.outer_steps(self.logw, self.logZ, lik[None, :], 0.0)
        self.ess = float(ess[0])
        self.ess_trace.append(self.ess)

    def rejuvenate(self, y, xi=1.0):
        y = np.asarray(y, dtype=np.float64)
        acc_array = np.zeros(self.M, dtype=bool)
        L, uni = ob.rw_factor(self.theta)
        scales = 0.5 * np.arange(self.chain, 0, -1)
        s = scales * scales if uni else scales
        move_seed = self._next_seed()
        for m in range(self.M):
            for c in range(self.chain):
                prop = ob.pmmh_propose(move_seed, m, c, self.theta[m], L, s[c])
                if not all(ob.prior_insupport(self.fam[i], self.par[i], prop[i]) for i in range(self.d)):
                    self.n_out_of_support += 1
                    continue
                x_prop, s_prop, logZ_prop = gap_series(self._row(prop), y, self.predict_first)
                lp_prop = lp_cur = 0.0
                for i in range(self.d):
                    lp_prop = lp_prop + ob.prior_logpdf(self.fam[i], self.par[i], prop[i])
                    lp_cur = lp_cur + ob.prior_logpdf(self.fam[i], self.par[i], self.theta[m, i])
                prior_ratio = lp_prop - lp_cur
                likelihood_ratio = xi * (logZ_prop - self.logZ[m])
                log_post_prop = logZ_prop + lp_prop
                acc_ratio = likelihood_ratio + prior_ratio
                if log_post_prop > -np.inf and ob.pmmh_log_uniform(move_seed, m, c) < acc_ratio:
                    self.logZ[m] = logZ_prop
                    self.theta[m] = prop
                    self.x[m] = x_prop
                    self.S[m] = s_prop
                    acc_array[m] = True
                    self.n_accepted += 1
            self.logw[m] = 0.0
        self.accepted = acc_array
        self.acc_ratio = float(acc_array.sum()) / self.M
        self.n_rejuvenations += 1

    def density_tempered(self, y):
        y = np.asarray(y, dtype=np.float64)
        for m in range(self.M):
            self.x[m], self.S[m], self.logZ[m] = gap_series(self._row(self.theta[m]), y, self.predict_first)
        self.logw = self.logZ.copy()
        _, _, self.ess = ob.outer_reweight(self.logZ, False)
        self.t = len(y)
        xi, ladder = 0.0, []
        while xi < 1.0:
            xi, self.ess, flag, logw = ob.outer_temper(self.logZ, xi, self.ess_min)
            if flag:
                self.resample(logw)
                self.rejuvenate(y, xi)
            else:
                self.logw = logw
            ladder.append((xi, self.ess, self.acc_ratio if flag else None))
        return ladder


def with_gaps(y, gaps):
    y = np.array(y, dtype=np.float64)
    if len(gaps):
        y[list(gaps)] = np.nan
    return y
