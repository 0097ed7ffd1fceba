"""Non-finite observations and out-of-domain parameter rows, shared by tests/test_nonfinite_host.py (the CPU oracle and the host
twins stay within their conditions on them) and tests/test_gpu_nonfinite.py (every launch path equals the oracle on them).

The contract the tables state (include/smc_hip.h "non-finite inputs"):
  * a step whose observation is NaN or +-inf leaves no particle with a usable log-weight: logmu = -inf, ess = 0, every weight 0,
    logZ = -inf from then on; the ancestors of the step after it are the identity (weights_resample of a collapsed filter);
  * the bootstrap families keep finite states through such a step and weigh again at the next finite observation;
  * a parameter row outside its model's domain (a negative variance, |rho| >= 1, a NaN anywhere) is not refused: the filter is
    dead from the step DEAD_FROM of its entry on, and its neighbours in the batch are untouched;
  * the sign of a UCSV gamma only flips a normal: such a filter is alive.

Every comparison of the tests built on this file is exact: same_nan for doubles (x86 and the GPU produce NaNs of different sign
and payload, so the NaN positions must coincide and everything else must be the same bits), array_equal for the integer arrays
(ancestors, the raw fixed-point C, S, S2hi, S2lo).
"""
import numpy as np

NAN, INF = float("nan"), float("inf")
LG1D, SV1D, UCSV3D, UCSV_RB = 1, 2, 3, 4
BAD_Y = (NAN, INF, -INF)
BAD_Y_IDS = ("nan", "+inf", "-inf")
T = 6
POSITIONS = ((0,), (2,), (T - 1,), (2, 3))          # the first step (smc_init), a middle step, the last one, two in a row
ALIVE = None                                         # tag of a row whose filter never dies

# healthy rows of the families (tests/test_gpu_paths.py RAW; UCSV_RB reads the UCSV row)
LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]                  # A, B, Q, R, x0, sigma0 (Q, R, sigma0 variances)
SV = [-1.0, 0.95, 0.25]                              # mu, rho, sigma
UC = [0.2, 0.2, 3.0, 0.0, 0.0]                       # gamma_eps, gamma_eta, x0, lse0, lsn0
HEALTHY = {LG1D: LG, SV1D: SV, UCSV3D: UC, UCSV_RB: UC}


def _row(base, k, v):
    r = list(base)
    r[k] = v
    return r


# (id, model, raw, tag): tag = DEAD_FROM, the filter's steps t >= DEAD_FROM read logmu = -inf / ess = 0; ALIVE: none does; a tuple
# names the dead steps one by one.  The tags of the LG1D / SV1D / UCSV3D rows are the bootstrap filter's (the CPU oracle), those
# of the UCSV_RB rows the marginal filter's (tests/composed_reference.py).
BAD_ROWS = (
    ("lg-Q<0", LG1D, _row(LG, 2, -0.9), 1),          # sqrt(Q) = NaN enters at the first transition
    ("lg-A=nan", LG1D, _row(LG, 0, NAN), 1),
    ("lg-R=0", LG1D, _row(LG, 3, 0.0), 0),           # 1/sqrt(R) = inf, log sqrt(R) = -inf
    ("lg-R<0", LG1D, _row(LG, 3, -0.8), 0),
    ("lg-sigma0=0", LG1D, _row(LG, 5, 0.0), ALIVE),  # valid: x_1 = x0 for every particle
    ("lg-Q=inf", LG1D, _row(LG, 2, INF), 1),
    ("lg-B=nan", LG1D, _row(LG, 1, NAN), 0),
    ("sv-rho=1", SV1D, _row(SV, 1, 1.0), 0),         # sigma / sqrt(1 - rho^2) = inf
    ("sv-rho=1.5", SV1D, _row(SV, 1, 1.5), 0),
    ("sv-sigma=nan", SV1D, _row(SV, 2, NAN), 0),
    ("sv-rho=-1", SV1D, _row(SV, 1, -1.0), 0),
    ("uc-lse0=inf", UCSV3D, _row(UC, 3, INF), 0),
    ("uc-x0=nan", UCSV3D, _row(UC, 2, NAN), 0),
    ("uc-geps<0", UCSV3D, _row(UC, 0, -0.2), ALIVE),
    ("uc-lsn0=-inf", UCSV3D, _row(UC, 4, -INF), 0),
    ("rb-lse0=inf", UCSV_RB, _row(UC, 3, INF), 0),
    ("rb-x0=nan", UCSV_RB, _row(UC, 2, NAN), 0),
    ("rb-geps<0", UCSV_RB, _row(UC, 0, -0.2), ALIVE),
    ("rb-lsn0=-inf", UCSV_RB, _row(UC, 4, -INF), ALIVE),   # R = exp(-inf) = 0: the Kalman step runs without measurement noise
)
BAD_ROW_IDS = tuple(r[0] for r in BAD_ROWS)
BOOTSTRAP_ROWS = tuple(r for r in BAD_ROWS if r[1] != UCSV_RB)


def rows_of(model):
    return tuple(r for r in BAD_ROWS if r[1] == model)


def bad_series(y, positions, bad):
    """a copy of the finite series y with `bad` planted at the positions"""
    y = np.array(y, dtype=np.float64)
    assert np.all(np.isfinite(y))
    y[list(positions)] = bad
    return y


def dead_steps(T_, tag):
    """the mask [T] of the dead steps of a tag"""
    m = np.zeros(T_, dtype=bool)
    if isinstance(tag, tuple):
        m[list(tag)] = True
    elif tag is not ALIVE:
        m[tag:] = True
    return m


# ---- guided and marginal filters (tests/composed_reference.py is their whole-series reference) --------------------------------
# The first step of a guided filter is the bootstrap first step, so a bad y_1 costs that step alone.  Every later guided step and
# every marginal step puts y into the state - LG1D through k = fma(c2, y, c0) (AFFINE with c2 = 0 too: 0 * y is NaN for a
# non-finite y), UCSV OPTIMAL through x[0] = fma(K, y - xp[0], xp[0]), the marginal family through its Kalman (m, P) - so these
# filters do not weigh again after a bad observation: dead from that step on.
NONE, AFFINE, OPTIMAL = 0, 1, 2
POOR = [0.3, 0.2, 0.1, 2.0]                          # tests/step_edge_inputs.py POOR
POOR_C2_0 = [0.3, 0.2, 0.0, 2.0]                     # the same proposal without its y term
# id -> (model, kind, proposal row or None)
COMPOSED = {
    "lg-affine": (LG1D, AFFINE, POOR),
    "lg-affine-c2=0": (LG1D, AFFINE, POOR_C2_0),
    "lg-optimal": (LG1D, OPTIMAL, None),
    "uc-optimal": (UCSV3D, OPTIMAL, None),
    "rb": (UCSV_RB, NONE, None),
}
# rows whose tag under a guided handle is not the bootstrap filter's: the guided UCSV step reads R = exp(lsn) = 0 as an
# observation without noise and weighs on; only the (bootstrap) first step is dead
GUIDED_TAG = {"uc-lsn0=-inf": (0,)}


def composed_y_tag(fam, positions):
    """the dead steps of a guided / marginal filter on a series with bad observations at `positions`"""
    first = min(positions)
    if COMPOSED[fam][1] != NONE and first == 0:
        rest = [p for p in positions if p > 0]
        return (0,) if not rest else (0,) + tuple(range(min(rest), T))
    return first


def composed_row_tag(fam, rid, tag):
    return GUIDED_TAG.get(rid, tag) if COMPOSED[fam][1] != NONE else tag


def _f64(a):
    return np.atleast_1d(np.ascontiguousarray(a, dtype=np.float64))


def same_nan(a, b):
    """a and b (doubles) have their NaNs at the same positions and the same IEEE bit patterns everywhere else"""
    a, b = _f64(a), _f64(b)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~na]))


def same_slot(d, o):
    """two per-filter snapshots (x, w, ancestors, C, m, S, S2hi, S2lo): doubles by same_nan, integers by array_equal"""
    return (same_nan(d[0], o[0]) and same_nan(d[1], o[1]) and np.array_equal(d[2], o[2]) and np.array_equal(d[3], o[3])
            and same_nan(d[4], o[4]) and np.array_equal(d[5], o[5]) and np.array_equal(d[6], o[6]) and np.array_equal(d[7], o[7]))


def first_diff(d, o, names=("x", "w", "ancestors", "C", "m", "S", "S2hi", "S2lo")):
    """the name of the first member of two snapshots that differs, or None (for assertion messages)"""
    for k, name in enumerate(names):
        ok = np.array_equal(d[k], o[k]) if np.asarray(d[k]).dtype.kind in "iu" else same_nan(d[k], o[k])
        if not ok:
            return name
    return None


def plant(xp, variance_row=None):
    """xp [d][n] with a NaN, +inf and -inf planted in every row, each in a particle of its own (particle 100 + 3 r + k holds value k
    in row r), and - variance_row, the marginal family's P - a 0.0 and a +inf in two more -> (the copy, mask [n] of those particles)"""
    xp = np.array(xp, dtype=np.float64)
    touched = np.zeros(xp.shape[1], dtype=bool)
    for r in range(xp.shape[0]):
        for k, v in enumerate(BAD_Y):
            xp[r, 100 + 3 * r + k] = v
            touched[100 + 3 * r + k] = True
    if variance_row is not None:
        xp[variance_row, 200], xp[variance_row, 201] = 0.0, INF
        touched[200:202] = True
    return xp, touched


# ---- samplers that reach invalid rows ------------------------------------------------------------------------------------------
# density_tempered and the online smc2 + smc2_step loop over LG1D with theta = (A, Q, R) and a Normal prior on the variance Q:
# about a fifth of the draws from the prior, and of the PMMH proposals, have Q < 0 inside the prior's support.  The device route
# (ThetaMap) builds their parameter rows without a constructor; their filters are dead and the accept test must refuse them.
SAMPLER_N, SAMPLER_M, SAMPLER_T = 256, 24, 20
SAMPLER_SEED = {False: 7, True: 7}                   # density_tempered / online: chosen on the CPU so that sampler_conditions holds


def sampler_prior():
    import sequential_monte_carlo_amd as smc
    return smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.Normal(0.5, 0.6), smc.LogNormal()])


def sampler_model(theta):
    import sequential_monte_carlo_amd as smc
    return smc.UnivariateLinearGaussian(A=theta[0], B=1.0, Q=theta[1], R=theta[2])


def sampler_series():
    import sequential_monte_carlo_amd as smc
    return smc.simulate(smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8), SAMPLER_T, seed=1998)[1]


def watch(backend, replay=None):
    """record what the backend's rejuvenate calls do: accepted moves with Q <= 0 or without a finite logZ, and - replay: the oracle
    binding - the proposals of the first chain position that lie in the prior's support with Q <= 0 -> the record (a dict)"""
    rec = dict(moves=0, accepted=0, accepted_bad_Q=0, accepted_dead=0, proposed_bad_Q=0)
    inner = backend.rejuvenate

    def rejuvenate(tmap, prior_spec, N, y, xi, chol, scales, filter_seeds, move_seed, streams, theta, logZ, main):
        theta0 = np.array(theta, dtype=np.float64)
        if replay is not None:
            fam, par = prior_spec
            for m in range(theta0.shape[0]):
                prop = replay.pmmh_propose(move_seed, int(streams[m]), 0, theta0[m], chol, scales[0])
                if all(replay.prior_insupport(fam[i], par[i], prop[i]) for i in range(len(fam))) and prop[1] <= 0:
                    rec["proposed_bad_Q"] += 1
        th, lz, acc, nrun = inner(tmap, prior_spec, N, y, xi, chol, scales, filter_seeds, move_seed, streams, theta, logZ, main)
        th, lz, acc = np.asarray(th, dtype=np.float64).reshape(theta0.shape), np.asarray(lz, dtype=np.float64), np.asarray(acc, dtype=bool)
        rec["moves"] += 1
        rec["accepted"] += int(acc.sum())
        rec["accepted_bad_Q"] += int(np.sum(th[acc][:, 1] <= 0))
        rec["accepted_dead"] += int(np.sum(~(lz[acc] > -INF)))
        return th, lz, acc, nrun

    backend.rejuvenate = rejuvenate
    return rec


def run_sampler(backend, online, replay=None):
    """-> (the sampler, its printed trace, the stages (density_tempered) or the main filters' (x, w) (online), the record of
    watch(), the initial parameter cloud)"""
    import io
    import sequential_monte_carlo_amd as smc
    tmap = smc.ThetaMap(LG1D, [0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    rec = watch(backend, replay)
    y = sampler_series()
    s = smc.SMC(SAMPLER_N, SAMPLER_M, sampler_model, sampler_prior(), 2, 0.5, seed=SAMPLER_SEED[online], backend=backend, theta_map=tmap)
    assert s.device_pmmh
    theta0 = s.theta.copy()
    buf = io.StringIO()
    if online:
        smc.smc2(s, y)
        for t in range(2, SAMPLER_T + 1):
            smc.smc2_step(s, y, t, verbose=True, out=buf)
        x, w, _ = s._main.state()
        return s, buf.getvalue(), (x, w), rec, theta0
    stages = smc.density_tempered(s, y, verbose=True, out=buf)
    return s, buf.getvalue(), stages, rec, theta0


def sampler_conditions(rec, theta0):
    """what makes the run a test (asserted on the reference side): the prior cloud holds Q <= 0 and Q > 0, a rejuvenation proposed
    Q <= 0 inside the prior's support"""
    assert np.any(theta0[:, 1] <= 0) and np.any(theta0[:, 1] > 0), theta0[:, 1]
    assert rec["moves"] >= 1 and rec["accepted"] >= 1 and rec["proposed_bad_Q"] >= 1, rec


def sampler_properties(s, rec):
    """no move to Q <= 0 or to a dead filter was accepted; every parameter particle that carries weight has Q > 0"""
    assert rec["accepted_bad_Q"] == 0 and rec["accepted_dead"] == 0, rec
    om = np.asarray(s.omega)
    assert np.all(s.theta[om > 0, 1] > 0), (s.theta[:, 1], om)
    assert np.any(om > 0) and abs(om.sum() - 1) < 1e-9
