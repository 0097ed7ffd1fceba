"""sequential_monte_carlo_amd -- MI355X-native particle-filter hot path of
charlesknipp/sequential_monte_carlo behind the reference's own API names.

Hand-written HIP kernels for gfx950 (csrc/) behind a C ABI (include/smc_hip.h); this package is the
host-side mirror of src/particles.jl, src/state_space_models.jl, src/smc_samplers.jl and src/ibis.jl.
There is no CPU fallback: importing works anywhere, running a filter needs the GPU library.
"""
from .distributions import LogNormal, Normal, TruncatedNormal, Uniform, product_distribution  # noqa: F401
from .ibis import IBIS  # noqa: F401
from .ibis import rts_quantile, rts_smoothed_paths, rts_smoothed_state  # noqa: F401
from .kalman_filter import kalman_predictive, kalman_smoother, log_likelihood_kalman  # noqa: F401
from .models import (UCSV, LinearModel, LinearModel2D, MarginalUCSV, MultivariateLinearGaussian, hodrick_prescott, StateSpaceModel, StochasticVolatility, UnivariateLinearGaussian,  # noqa: F401
                     simulate, unobserved_components, unobserved_components_stochastic_volatility)
from .particles import (AffineGaussianProposal, OptimalProposal, ParticleGibbs, bootstrap_filter, bootstrap_filter_, forecast, log_likelihood, normalize,  # noqa: F401
                        optimal_proposal, particle_filter, particle_filter_, rb_smoother, resample, reweight, smoother, trend_moments)
from .particles import em_mstep, particle_em, pit_residuals  # noqa: F401
from .smc_samplers import (SMC, ThetaMap, density_tempered, estimated_trend, expected_parameters, filtered_state, forecast_state,  # noqa: F401
                           filtered_summaries, observation_dist, posterior_histogram, posterior_moments, posterior_quantiles, quantile, rejuvenate_, resample_, smc2, smc2_run, smc2_step,
                           rb_smoothed_state, smoothed_paths, smoothed_quantiles, smoothed_state)

__version__ = "0.1.0"
