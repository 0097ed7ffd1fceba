"""The FFBS smoother's specification on the host (smc_host_transition_logpdf, smc_host_smooth) against references
that share no arithmetic with the library (tests/smoother_reference.py).  No GPU."""
import numpy as np
import pytest

import smoother_planted as P
import smoother_reference as R

EPS = 2.0 ** -52
CH = 128                                    # SMOOTH_CH of csrc/smc_spec.h; the library's copy is checked below
LG_README = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]  # README.md: UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
ROWS = {
    R.LG1D: LG_README,
    R.SV1D: [-1.0, 0.95, 0.3],
    R.UCSV3D: [0.2, 0.3, 1.0, -1.0, -0.5],
}
# moments: the bounds DESIGN.md section 2 states for smc_get_moments, against exactly rounded sums
MEAN_REL, MEAN_SD, VAR_REL, VAR_LEVEL = 1e-11, 1e-12, 1e-9, 1e-11


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_chunk_length_is_the_documented_one(L):
    assert L.SMOOTH_CH == CH


def test_transition_logpdf_against_longdouble(L):
    """10^4 random rows and states per family, tolerance 8 eps (|logf| + 1).  The ranges keep the evaluation well conditioned
    against the formula in long double: the centre A xp (rho (xp - mu) + mu) is rounded before x - centre, an absolute error of
    eps |centre| / 2 in d, i.e. eps d |centre| / (2 Q) in logf, which stays below 8 eps + 4 eps d^2 / Q for |centre| <= 22 sqrt(Q):
    Q >= 0.2 with |A xp| <= 9, sigma >= 0.5 with |centre| + |xp - mu| <= 9.  UCSV3D subtracts the states themselves (exact to half
    an ulp); gammas in [0.2, 1] and |lse| <= 2 keep its constant below 4, so that the sum of the magnitudes of its terms stays
    within |logf| + 8 and a few roundings of each term within the tolerance."""
    rng = np.random.default_rng(20260101)
    N = 10000
    for model in (R.LG1D, R.SV1D, R.UCSV3D):
        d = R.DIM[model]
        worst = 0.0
        for _ in range(N):
            if model == R.LG1D:
                raw = [rng.uniform(-1, 1), 1.0, rng.uniform(0.2, 2.0), 0.8, 0.0, 1.0]
                xp, x = rng.uniform(-9, 9, 1), rng.uniform(-9, 9, 1)
            elif model == R.SV1D:
                raw = [rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.5, 1.5)]
                xp, x = rng.uniform(-3, 3, 1), rng.uniform(-3, 3, 1)
            else:
                raw = [rng.uniform(0.2, 1.0), rng.uniform(0.2, 1.0), 0.0, 0.0, 0.0]
                xp = np.array([rng.uniform(-5, 5), rng.uniform(-2, 2), rng.uniform(-2, 2)])
                x = xp + np.array([rng.normal() * np.exp(0.5 * xp[1]), rng.normal() * raw[0], rng.normal() * raw[1]]) * 2.0
            got = L.host_transition_logpdf(model, raw, xp, x)
            ref = R.logf_ref(model, raw, [xp[r] for r in range(d)], [x[r] for r in range(d)])
            err = abs(float(R.LD(got) - ref))
            tol = 8 * EPS * (abs(float(ref)) + 1.0)
            worst = max(worst, err / tol)
            assert err <= tol, (model, raw, xp, x, got, float(ref))
        print("model %d: worst error / tolerance %.3f" % (model, worst))


def test_transition_logpdf_refusals(L):
    with pytest.raises(L.SmcError):
        L.host_transition_logpdf(L.MODEL_UCSV_RB, ROWS[R.UCSV3D], np.zeros(4), np.zeros(4))
    for model, k in ((R.LG1D, 2), (R.SV1D, 2), (R.UCSV3D, 0), (R.UCSV3D, 1)):
        for bad in (0.0, -1.0, np.nan, np.inf):
            raw = list(ROWS[model])
            raw[k] = bad
            with pytest.raises(L.SmcError):
                L.host_transition_logpdf(model, raw, np.zeros(R.DIM[model]), np.zeros(R.DIM[model]))
            with pytest.raises(L.SmcError):
                L.host_smooth(model, raw, np.zeros((1, R.DIM[model], 2)), np.full((1, 2), 0.5))


_CLOUDS = {}


def recorded_clouds(L, ob, model, raw, n, T, seed=5):
    """(x [T][d][n], w [T][n]) of the oracle's bootstrap filter, state() after every step; computed once per case"""
    key = (model, tuple(raw), n, T, seed)
    if key not in _CLOUDS:
        _, y = L.simulate(model, raw, T, 1998)
        f = ob.Filter(model, raw, n, seed=seed)
        xs, wsv = [], []
        for t in range(T):
            f.bootstrap_filter(float(y[0])) if t == 0 else f.step(float(y[t]))
            x, w, _, _ = f.state()
            xs.append(x.copy())
            wsv.append(w.copy())
        _CLOUDS[key] = (np.array(xs), np.array(wsv))
    return _CLOUDS[key]


def check_against_reference(L, model, raw, x, w):
    T, n = w.shape
    ws, mean, var = L.host_smooth(model, raw, x, w)
    ref = R.ffbs_ref(model, raw, x, w)
    assert np.array_equal(bits(ws[T - 1]), bits(w[T - 1]))            # ws_T = w_T, bit for bit
    unit = (2 * (CH + n / CH) + 200) * EPS
    worst = 0.0
    for t in range(T):
        tol = (T - 1 - t) * unit
        err = float(R.exact_sum(np.abs(ws[t].astype(R.LD) - ref[t]), 0))
        tot = float(abs(R.exact_sum(ws[t], 0) - 1))
        worst = max(worst, err / tol if tol else 0.0, tot / tol if tol else 0.0)
        assert err <= tol, (model, n, T, t, err, tol)
        # (at the last step the recursion has done nothing and the bound is 0: ws_T = w_T bit for bit, checked above, is the
        # statement there - the sum of the filter's own weights differs from 1 by their rounding, which is not the smoother's)
        if t < T - 1:
            assert tot <= tol, (model, n, T, t, tot, tol)
        for r in range(R.DIM[model]):
            m, v = R.exact_moments(x[t, r], ws[t])
            assert abs(mean[t, r] - m) <= MEAN_REL * abs(m) + MEAN_SD * np.sqrt(v), (t, r, mean[t, r], m)
            assert var[t, r] >= 0 and abs(var[t, r] - v) <= VAR_REL * v + (VAR_LEVEL * m) ** 2, (t, r, var[t, r], v)
    print("model %d n %d T %d: worst (sum |ws - ref| or |sum ws - 1|) / tolerance %.4f" % (model, n, T, worst))
    return ws


@pytest.mark.parametrize("T", [1, 2, 12, 64])
@pytest.mark.parametrize("n", [1, 2, 65, 300, 520])
@pytest.mark.parametrize("model", [R.LG1D, R.SV1D, R.UCSV3D])
def test_host_smooth_against_longdouble_recursion(L, ob, model, n, T):
    x, w = recorded_clouds(L, ob, model, ROWS[model], n, T)
    if not np.all((w > 0).any(axis=1)):
        pytest.fail("the recorded filter collapsed: pick another seed for this case")
    check_against_reference(L, model, ROWS[model], x, w)


@pytest.mark.parametrize("n,T", [(65, 12), (300, 12), (520, 64)])
def test_host_smooth_sharp_observation(L, ob, n, T):
    """R = 1e-4: most filter weights are exactly 0 after every step; the log domain with the row maximum keeps every
    denominator away from 0 / 0"""
    raw = [0.5, 1.0, 0.9, 1e-4, 0.0, 1.0]
    x, w = recorded_clouds(L, ob, R.LG1D, raw, n, T)
    assert np.all((w > 0).any(axis=1))
    if n >= 65:
        assert (w == 0).mean() > 0.5
    ws = check_against_reference(L, R.LG1D, raw, x, w)
    assert np.all(np.isfinite(ws))


SHARP = [0.5, 1.0, 0.9, 1e-4, 0.0, 1.0]
PLANTED = [(model, ROWS[model], name) for model in (R.LG1D, R.SV1D, R.UCSV3D) for name in P.ALIVE]
PLANTED += [(R.LG1D, SHARP, name) for name in P.ON_ZERO + P.ALIVE]


@pytest.mark.parametrize("n", [65, 300])
@pytest.mark.parametrize("model,raw,name", PLANTED, ids=lambda v: v if isinstance(v, str) else ("sharp" if v is SHARP else None))
def test_planted_clouds_against_longdouble_recursion(L, ob, model, raw, name, n):
    """tests/smoother_planted.py: clouds no filter leaves (states that are not finite on zero-weight particles, two groups whose
    cross terms underflow, a target far from every source, tied states, subnormal weights, one particle alive), host twin against
    the long-double recursion with the bounds of every other record"""
    T = 6
    x, w = recorded_clouds(L, ob, model, raw, n, T)
    assert np.all((w > 0).any(axis=1))
    px, pw = P.variant(name, model, raw, x, w)
    assert np.all((pw > 0).any(axis=1))
    if name in P.ON_ZERO:
        assert (pw == 0).mean() > 0.5 and not np.all(np.isfinite(px))
    if name == "tiny_weights":
        assert (pw[P.mid(T)] > 0).sum() >= 2 and np.sort(pw[P.mid(T)])[-2] < 2.0 ** -1022
    if name == "one_alive":
        assert (pw[P.mid(T)] > 0).sum() == 1
    ref = R.ffbs_ref(model, raw, px, pw)
    assert np.all(np.isfinite(ref.astype(np.float64)))                # the reference itself stays finite
    ws = check_against_reference(L, model, raw, px, pw)
    assert np.all(np.isfinite(ws)) and np.all(ws[pw == 0] == 0)
    if name in P.ON_ZERO:                                             # left out whatever their states: the bits of the plain record
        ws0, mean0, var0 = L.host_smooth(model, raw, x, w)
        ws1, mean1, var1 = L.host_smooth(model, raw, px, pw)
        assert np.array_equal(bits(ws0), bits(ws1)) and np.array_equal(bits(mean0), bits(mean1)) and np.array_equal(bits(var0), bits(var1))
    if name == "far_apart":                                           # the planted distances do what they are there for
        ts, d = max(T // 2 - 1, 0), R.DIM[model]
        F = R.logf_ref(model, raw, [px[ts, r][:, None] for r in range(d)], [px[ts + 1, r][None, :] for r in range(d)])
        group = (np.arange(n) // P.BLOCK) % 2
        cross = group[:, None] != group[None, :]
        assert np.all(np.isfinite(F.astype(np.float64)))
        with np.errstate(divide="ignore"):
            A = np.log(pw[ts].astype(R.LD))[:, None] + F
        assert np.all((A - A.max(axis=0)[None, :])[cross] < -746)      # every cross term underflows against the row maximum: exp(-746) = 0
        if raw is not SHARP:                                          # both groups are alive on both sides
            assert all((pw[ts][group == g] > 0).any() and (pw[ts + 1][group == g] > 0).any() for g in (0, 1))
        j = int(np.argmax(w[T - 1]))
        Fl = R.logf_ref(model, raw, [px[T - 2, r] for r in range(d)], [px[T - 1, r, j] for r in range(d)])
        assert np.all(Fl < -1000) and np.all(np.isfinite(Fl.astype(np.float64)))


@pytest.mark.parametrize("n", [65, 300])
@pytest.mark.parametrize("model", [R.LG1D, R.SV1D, R.UCSV3D])
def test_planted_dead_steps(L, ob, model, n):
    """a step at which every weight is 0, at the first, a middle and the last step: NaN everywhere, in the twin and the reference"""
    T = 6
    x, w = recorded_clouds(L, ob, model, ROWS[model], n, T)
    for t_dead in P.dead_steps(T):
        px, pw = P.dead_at(x, w, t_dead)
        ws, mean, var = L.host_smooth(model, ROWS[model], px, pw)
        assert np.all(np.isnan(ws)) and np.all(np.isnan(mean)) and np.all(np.isnan(var)), t_dead
        assert np.all(np.isnan(R.ffbs_ref(model, ROWS[model], px, pw).astype(np.float64))), t_dead


def test_rts_pin(L, ob):
    """the smoothed mean of LG1D against the exact Rauch-Tung-Striebel smoother: README parameters, simulate seed 1998, T = 24,
    n = 256, 24 seeds: within 4 standard errors at every t, the seed-averaged smoothed variance within 10 % of the RTS variance.
    The FILTERED means of the same runs miss the RTS means: the test tells a smoother from a filter."""
    raw, T, n, K = LG_README, 24, 256, 24
    _, y = L.simulate(L.MODEL_LG1D, raw, T, 1998)
    m_rts, P_rts = R.rts_smoother(raw, y)
    sm, sv, fm = np.zeros((K, T)), np.zeros((K, T)), np.zeros((K, T))
    for k in range(K):
        x, w = recorded_clouds(L, ob, R.LG1D, raw, n, T, seed=100 + k)
        _, mean, var = L.host_smooth(R.LG1D, raw, x, w)
        sm[k], sv[k] = mean[:, 0], var[:, 0]
        fm[k] = (w * x[:, 0, :]).sum(axis=1)
    se = sm.std(axis=0, ddof=1) / np.sqrt(K)
    z = np.abs(sm.mean(axis=0) - m_rts) / se
    ratio = sv.mean(axis=0) / P_rts
    print("smoothed: max |z| %.2f; variance ratio %.3f .. %.3f" % (z.max(), ratio.min(), ratio.max()))
    assert np.all(z <= 4.0), z
    assert np.all(np.abs(ratio - 1) <= 0.10), ratio
    zf = np.abs(fm.mean(axis=0) - m_rts) / (fm.std(axis=0, ddof=1) / np.sqrt(K))
    assert (zf[:T - 1] > 4.0).sum() >= 12, zf      # the filtered means are not the smoothed ones


def test_collapse_and_left_out_particles(L, ob):
    raw = [0.5, 1.0, 0.9, 1e-4, 0.0, 1.0]
    x, w = recorded_clouds(L, ob, R.LG1D, raw, 300, 12)
    ws, mean, var = L.host_smooth(R.LG1D, raw, x, w)
    # zero-weight particles never enter a sum: a NaN state planted on every one of them changes nothing
    assert (w == 0).any() and (ws == 0).any()
    xn = x.copy()
    xn[:, 0, :][w == 0] = np.nan
    ws2, mean2, var2 = L.host_smooth(R.LG1D, raw, xn, w)
    assert np.array_equal(bits(ws), bits(ws2)) and np.array_equal(bits(mean), bits(mean2)) and np.array_equal(bits(var), bits(var2))
    assert np.all(ws[w == 0] == 0)
    # a step at which every weight is 0: NaN at every t
    for t_dead in (0, 5, 11):
        wd = w.copy()
        wd[t_dead] = 0.0
        ws3, mean3, var3 = L.host_smooth(R.LG1D, raw, x, wd)
        assert np.all(np.isnan(ws3)) and np.all(np.isnan(mean3)) and np.all(np.isnan(var3))
        assert np.all(np.isnan(R.ffbs_ref(R.LG1D, raw, x, wd).astype(np.float64)))
