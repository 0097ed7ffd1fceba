"""State-space model families of the reference (src/state_space_models.jl), as parameter holders.

The reference's contract is 4 generic functions per model (preallocate / initial_dist / transition /
observation, ssm.jl:30-42) returning Distributions.jl objects that the filters call per particle.
A GPU cannot call host closures, so the drop-in boundary is "enumerated family + parameter row":
each class below carries `model_id` and `raw()` (the row handed to smc_set_params); the per-particle
arithmetic lives in csrc/smc_spec.h (model_initial / model_transition / model_logobs).
"""
import numpy as np

from . import _lib


class StateSpaceModel:
    """abstract type StateSpaceModel   (ssm.jl:9)"""
    model_id = None
    dim = None

    def raw(self):
        raise NotImplementedError


class LinearModel(StateSpaceModel):
    """LinearModel{Float64,...} (ssm.jl:46-58): x[t] ~ N(A x[t-1], Q), y[t] ~ N(B x[t], R),
    x[1] ~ N(x0, sigma0).  Q, R, sigma0 are VARIANCES (ssm.jl:93,102,108)."""
    model_id = _lib.MODEL_LG1D
    dim = 1

    def __init__(self, A, B, Q, R, x0=0.0, sigma0=1.0):
        self.A, self.B, self.Q, self.R, self.x0, self.sigma0 = map(float, (A, B, Q, R, x0, sigma0))
        if not (self.Q > 0 and self.R > 0 and self.sigma0 > 0):
            raise ValueError("Q, R and sigma0 are variances and must be positive")

    def raw(self):
        return [self.A, self.B, self.Q, self.R, self.x0, self.sigma0]


def UnivariateLinearGaussian(*, A, B, Q, R, x0=0.0, sigma0=1.0):
    """UnivariateLinearGaussian(;A,B,Q,R,x0=0.0,sigma0=1.0)   (ssm.jl:74-77)"""
    return LinearModel(A, B, Q, R, x0, sigma0)


def unobserved_components(*, sigma_eps, sigma_eta, x0):
    """local-level UC model (ssm.jl:119-128): A = B = 1, Q = sigma_eps, R = sigma_eta, sigma0 = sigma_eps."""
    return LinearModel(1.0, 1.0, sigma_eps, sigma_eta, x0, sigma_eps)


class StochasticVolatility(StateSpaceModel):
    """x[1] ~ N(mu, sigma^2/(1-rho^2)), x[t] ~ N(mu + rho (x[t-1]-mu), sigma), y[t] ~ N(0, exp(x[t]/2)).
    Not in the reference's src/ (BASELINE config 3; SURVEY A7'); observation follows ssm.jl:244-247."""
    model_id = _lib.MODEL_SV1D
    dim = 1

    def __init__(self, mu, rho, sigma):
        self.mu, self.rho, self.sigma = map(float, (mu, rho, sigma))
        if not (abs(self.rho) < 1 and self.sigma > 0):
            raise ValueError("need |rho| < 1 and sigma > 0")

    def raw(self):
        return [self.mu, self.rho, self.sigma]


class UCSV(StateSpaceModel):
    """UCSV (ssm.jl:215-263): state (x, log s_eps, log s_eta); x' ~ N(x, exp(log_s_eps/2)) with the
    PREVIOUS log-volatility, log-vols random walks with STD-DEV gamma; y ~ N(x, exp(log_s_eta/2))."""
    model_id = _lib.MODEL_UCSV3D
    dim = 3

    def __init__(self, gamma, x0, log_sigma0):
        self.gamma = (float(gamma[0]), float(gamma[1]))
        self.x0 = float(x0)
        self.log_sigma0 = (float(log_sigma0[0]), float(log_sigma0[1]))
        if not (self.gamma[0] > 0 and self.gamma[1] > 0):
            raise ValueError("gamma must be positive")

    def raw(self):
        return [self.gamma[0], self.gamma[1], self.x0, self.log_sigma0[0], self.log_sigma0[1]]


class MarginalUCSV(UCSV):
    """The same model with the trend integrated out (Rao-Blackwellised): given the two log-volatility paths (x, y) is
    linear-Gaussian, so every particle carries (m, log s_eps, log s_eta, P) - the exact Kalman mean and variance of the trend
    beside the volatilities it samples - and is weighted by the one-step predictive density N(y; m, P + exp(log s_eps_prev) +
    exp(log s_eta)).  An unbiased estimator of the same p(y) as the UCSV filter in which the trend adds no Monte-Carlo variance; same parameter row.
    Takes no proposal.  particles.trend_moments gives the trend's filtered mean and variance."""
    model_id = _lib.MODEL_UCSV_RB
    dim = 4


def unobserved_components_stochastic_volatility(*, x0, gamma_eps, gamma_eta, log_sigma_eps, log_sigma_eta, marginal=False):
    """unobserved_components_stochastic_volatility(;x0,γε,γη,log_σε,log_ση)   (ssm.jl:225-227)
    marginal=True: the MarginalUCSV filter family for the same model"""
    return (MarginalUCSV if marginal else UCSV)((gamma_eps, gamma_eta), x0, (log_sigma_eps, log_sigma_eta))


_KALMAN_ONLY = ("%s: a two-state linear model (MultivariateLinearGaussian, hodrick_prescott) is not a particle-filter family - its "
                "transition covariance may be singular, so it has no transition density; run it through the exact Kalman "
                "filter: log_likelihood_kalman / kalman_smoother, and IBIS for its parameters")


class LinearModel2D(StateSpaceModel):
    """LinearModel with a 2 x 2 transition and a scalar observation (ssm.jl:137-185): x[t] ~ N(A x[t-1], Q), y[t] ~ N(B x[t], R),
    x[1] ~ N(X0, Sigma0).  Q and Sigma0 are symmetric positive SEMI-definite (hodrick_prescott's Q is singular).  A row of the
    exact-Kalman side only: log_likelihood_kalman, kalman_smoother, IBIS, simulate.  raw() is the row of 15 entries
    (A11,A12,A21,A22, B1,B2, Q11,Q21,Q22, R, x01,x02, S11,S21,S22), the covariances as their lower triangle."""
    model_id = _lib.MODEL_LG2D
    dim = 2

    def __init__(self, A, B, Q, R, X0=None, Sigma0=None):
        A = np.asarray(A, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("A must be a square matrix")
        d = A.shape[0]
        if d != 2:
            raise ValueError("state dimension %d: only two-state models (A 2 x 2) are implemented" % d)
        B = np.asarray(B, dtype=np.float64)
        if B.ndim == 1:
            B = B[None, :]
        if B.ndim != 2 or B.shape[1] != d:
            raise ValueError("B must have one column per state")
        R = np.asarray(R, dtype=np.float64)
        if B.shape[0] != 1 or R.size != 1:
            raise ValueError("observation dimension %d: only a scalar observation (B 1 x 2, R a number) is implemented" % max(B.shape[0], R.shape[0] if R.ndim else 1))
        Q = np.asarray(Q, dtype=np.float64)
        X0 = np.zeros(d) if X0 is None else np.asarray(X0, dtype=np.float64).ravel()
        Sigma0 = np.eye(d) if Sigma0 is None else np.asarray(Sigma0, dtype=np.float64)
        if Q.shape != (d, d) or Sigma0.shape != (d, d) or X0.shape != (d,):
            raise ValueError("Q and Sigma0 must be 2 x 2 and X0 of length 2")
        for name, v in (("A", A), ("B", B), ("Q", Q), ("R", R), ("X0", X0), ("Sigma0", Sigma0)):
            if not np.all(np.isfinite(v)):
                raise ValueError("%s has an entry that is not finite" % name)
        for name, C in (("Q", Q), ("Sigma0", Sigma0)):
            if C[0, 1] != C[1, 0]:
                raise ValueError("%s is not symmetric" % name)
            # positive semi-definite: both diagonal entries and the determinant non-negative (the determinant up to its rounding)
            if C[0, 0] < 0 or C[1, 1] < 0 or C[0, 0] * C[1, 1] - C[1, 0] * C[1, 0] < -4 * np.finfo(float).eps * C[0, 0] * C[1, 1]:
                raise ValueError("%s is not positive semi-definite" % name)
        self.R = float(R.ravel()[0])
        if not self.R > 0:
            raise ValueError("R is a variance and must be positive")
        self.A, self.B, self.Q, self.X0, self.Sigma0 = A.copy(), B.copy(), Q.copy(), X0.copy(), Sigma0.copy()

    def raw(self):
        A, B, Q, S = self.A, self.B, self.Q, self.Sigma0
        return [A[0, 0], A[0, 1], A[1, 0], A[1, 1], B[0, 0], B[0, 1], Q[0, 0], Q[1, 0], Q[1, 1], self.R, self.X0[0], self.X0[1],
                S[0, 0], S[1, 0], S[1, 1]]


def MultivariateLinearGaussian(*, A, B, Q, R, X0=None, Sigma0=None):
    """MultivariateLinearGaussian(;A,B,Q,R,X0=zeros,Σ0=I)   (ssm.jl:137-153), for two states and a scalar observation"""
    return LinearModel2D(A, B, Q, R, X0, Sigma0)


def hodrick_prescott(*, lam, y, init_cov=1000.0):
    """hodrick_prescott(;λ,y,init_cov=1000.0)   (ssm.jl:193-202): x[t] ~ N(2 x[t-1] - x[t-2], 1/λ), y[t] ~ N(x[t], 1).  The
    smoothed first state, kalman_smoother(y, model)[0][:, 0], is the Hodrick-Prescott trend of y."""
    y = np.asarray(y, dtype=np.float64).ravel()
    if y.size < 2:
        raise ValueError("hodrick_prescott needs y[0] and y[1] for the initial state")
    lam = float(lam)
    if not lam > 0:
        raise ValueError("lam must be positive")
    return MultivariateLinearGaussian(A=[[2.0, -1.0], [1.0, 0.0]], B=[[1.0, 0.0]], Q=[[1 / lam, 0.0], [0.0, 0.0]], R=[1.0],
                                      X0=[3 * y[0] - 2 * y[1], 2 * y[0] - y[1]], Sigma0=float(init_cov) * np.eye(2))


def simulate(model, T, seed=1998):
    """simulate(rng, model, T) -> (x, y)   (ssm.jl:11-26).  x is [T] for scalar states, [T, d] otherwise.
    Host code (no GPU): the spec's Philox / Box-Muller stream keyed by `seed`."""
    if isinstance(model, LinearModel2D):
        x, y = _lib.simulate_lg2(model.raw(), int(T), int(seed))
        return x.T.copy(), y
    x, y = _lib.simulate(model.model_id, model.raw(), int(T), int(seed))    # (MarginalUCSV: UCSV's states, [T, 3])
    return (x[0] if model.dim == 1 else x.T.copy()), y


def params_matrix(models):
    """[n_theta][n_raw] parameter rows of a list of models of one family."""
    if isinstance(models, StateSpaceModel):
        models = [models]
    if any(isinstance(m, LinearModel2D) for m in models):
        raise TypeError(_KALMAN_ONLY % "params_matrix")
    ids = {m.model_id for m in models}
    if len(ids) != 1:
        raise ValueError("all models of a batch must belong to one family")
    return ids.pop(), np.array([m.raw() for m in models], dtype=np.float64)
