"""The guided particle step on the host (smc_host_guided_step, smc_host_optimal_proposal; no GPU): against the closed forms in
longdouble (tests/guided_reference.py) within propagated rounding bounds, and the argument checks of the proposal interface."""
import numpy as np
import pytest

import guided_reference as G

LG, SV, UC = 1, 2, 3
NONE, AFFINE, OPTIMAL = 0, 1, 2
N_CASES = 4000


def fma(a, b, c):
    """a * b + c with one rounding, signed zeros as IEEE-754 has them (exact rationals; Fraction -> float rounds correctly)"""
    from fractions import Fraction
    a, b, c = float(a), float(b), float(c)
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r != 0:
        return float(r)
    if (a == 0.0 or b == 0.0) and c == 0.0:     # a zero product plus a zero: -0.0 only if both are
        neg_prod = (np.signbit(a) != np.signbit(b))
        return -0.0 if (neg_prod and np.signbit(c)) else 0.0
    return 0.0                                   # exact cancellation


def lg_cases(seed=5):
    r = np.random.default_rng(seed)
    for i in range(N_CASES):
        level = [0.0, 1.0, 1e2, 1e5][i % 4]
        raw = [r.uniform(-1.1, 1.1), r.uniform(0.2, 2.0), np.exp(r.uniform(-6, 2)), np.exp(r.uniform(-6, 2)), 0.0, 1.0]
        par = [r.normal() * 0.3, r.uniform(-1, 1), r.uniform(-1, 1), np.exp(r.uniform(-6, 2))]
        xp = level + r.normal() * 2
        yield raw, par, xp, r.normal(), raw[1] * xp + r.normal() * 2


def ucsv_cases(seed=6):
    r = np.random.default_rng(seed)
    for i in range(N_CASES):
        level = [0.0, 3.0, 1e2, 1e5][i % 4]
        raw = [r.uniform(0.05, 0.5), r.uniform(0.05, 0.5), 0.0, 0.0, 0.0]
        xp = [level + r.normal(), r.uniform(-12, 4), r.uniform(-12, 4)]
        yield raw, xp, r.normal(size=3), xp[0] + r.normal() * 3


def test_lg_guided_step_against_longdouble(L):
    """LG1D, AFFINE and OPTIMAL rows, levels up to 1e5, variances exp(-6..2).  Bound: guided_reference.lg_bounds (one u = 2^-52 per
    rounded operation, 2 ulp per sp_log, propagated through smc_spec.h's order of operations).
    Measured on the host twin (4000 cases x 2 kinds): largest |x - ref| / bound = 0.441, largest |logw - ref| / bound = 0.316
    (largest absolute logw error 0.0158, on a log-weight of -1e12: a random row at the level 1e5 proposes far from y)."""
    worst_x = worst_w = worst_abs = 0.0
    for raw, par, xp, z, y in lg_cases():
        for kind, row in ((AFFINE, par), (OPTIMAL, None)):
            x, lw = L.host_guided_step(LG, raw, kind, row, [xp], [z], y)
            ref_row = par if kind == AFFINE else L.host_optimal_proposal(LG, raw)
            bx, bw = G.lg_bounds(raw, ref_row, xp, z, y, x[0])
            ex = abs(float(G.ld(x[0]) - G.lg_draw(ref_row, xp, z, y)))
            ew = abs(float(G.ld(lw) - G.lg_logw(raw, ref_row, xp, x[0], y)))
            worst_x, worst_w, worst_abs = max(worst_x, ex / bx), max(worst_w, ew / bw), max(worst_abs, ew)
            assert ex <= bx and ew <= bw, (raw, row, xp, z, y, ex, bx, ew, bw)
    print("LG guided step: max |x - ref| / bound %.3f, max |logw - ref| / bound %.3f, max |logw - ref| %.3g" % (worst_x, worst_w, worst_abs))


def test_ucsv_guided_step_against_longdouble(L):
    """UCSV OPTIMAL, trend levels up to 1e5, log-volatilities in [-12, 4].  Bound: guided_reference.ucsv_bounds.
    Measured on the host twin (4000 cases): largest |x[c] - ref| / bound = 0.490, largest |logw - ref| / bound = 0.257
    (largest absolute logw error 7.8e-11).  The reference's three-term expression agrees with the closed form to 1e-9 relative."""
    worst_x = worst_w = worst_abs = 0.0
    for raw, xp, z, y in ucsv_cases():
        x, lw = L.host_guided_step(UC, raw, OPTIMAL, None, xp, z, y)
        bx, bw = G.ucsv_bounds(raw, xp, z, y, x)
        x1, x2 = G.ucsv_vols(raw, xp, z)
        x0, ref_lw = G.ucsv_draw_logw(xp, z[0], y, x[2])
        ex = np.abs(np.array([float(G.ld(x[0]) - x0), float(G.ld(x[1]) - x1), float(G.ld(x[2]) - x2)]))
        ew = abs(float(G.ld(lw) - ref_lw))
        worst_x, worst_w, worst_abs = max(worst_x, float(np.max(ex / np.maximum(bx, 1e-300)))), max(worst_w, ew / bw), max(worst_abs, ew)
        assert np.all(ex <= bx) and ew <= bw, (raw, xp, z, y, ex, bx, ew, bw)
        three = G.ucsv_logw_three_terms(xp, [x0, x1, x[2]], y)
        assert abs(float(three - ref_lw)) <= 1e-9 * (1.0 + abs(float(ref_lw)))
    print("UCSV guided step: max |x - ref| / bound %.3f, max |logw - ref| / bound %.3f, max |logw - ref| %.3g" % (worst_x, worst_w, worst_abs))


def test_optimal_proposal_row_and_full_adaptation(L):
    """smc_host_optimal_proposal within 2 ulp of the formula per entry; with that row the three-term log-weight does not depend
    on z (it is log N(y; B A xp, B^2 Q + R)) up to the bound of the step."""
    r = np.random.default_rng(9)
    for i in range(500):
        raw = [r.uniform(-1.1, 1.1), r.uniform(0.2, 2.0), np.exp(r.uniform(-6, 2)), np.exp(r.uniform(-6, 2)), 0.0, 1.0]
        row = L.host_optimal_proposal(LG, raw)
        ref = G.lg_optimal_row(raw)
        assert row[0] == 0.0
        for k in range(1, 4):
            assert abs(float(G.ld(row[k]) - ref[k])) <= 2 * np.spacing(abs(float(ref[k]))), (raw, k, row[k], ref[k])
        xp, y = [0.0, 1e3][i % 2] + r.normal(), r.normal() * 2
        y += raw[1] * raw[0] * xp
        A, B, Q, R = raw[:4]
        const = float(G.logn(y, G.LD(B) * G.LD(A) * G.LD(xp), G.LD(B) ** 2 * G.LD(Q) + G.LD(R)))
        for z in r.normal(size=8):
            x, lw = L.host_guided_step(LG, raw, OPTIMAL, None, [xp], [z], y)
            _, bw = G.lg_bounds(raw, row, xp, z, y, x[0])
            # the longdouble three-term value at the returned x differs from the constant by the rounding of the ROW (2 ulp per
            # entry moves m and s2): second-order in logw around the optimum, first-order in the variance term
            assert abs(lw - const) <= bw + 16 * G.U * (1.0 + abs(const)), (raw, xp, z, y, lw, const, bw)


def test_affine_identity_on_the_host(L):
    """the row (0, A, 0, Q): the guided step is the transition and its weight the observation log-density, bit for bit - the
    mean is fma(A, xp, -0.0), the rounded product with its sign of zero, and the bracket evaluates to +0.0"""
    r = np.random.default_rng(3)
    lib = L.lib()
    for i in range(2000):
        raw = [r.uniform(-1.1, 1.1), r.uniform(0.2, 2.0), np.exp(r.uniform(-6, 2)), np.exp(r.uniform(-6, 2)), 0.0, 1.0]
        xp = [0.0, -0.0, 1e5, r.normal()][i % 4]
        z = [0.0, -0.0, r.normal(), r.normal()][(i // 4) % 4]
        y = r.normal() if i % 7 else 0.0
        x, lw = L.host_guided_step(LG, raw, AFFINE, [0.0, raw[0], 0.0, raw[2]], [xp], [z], y)
        sQ, sR = np.sqrt(raw[2]), np.sqrt(raw[3])
        xb = fma(sQ, z, raw[0] * xp)
        assert np.float64(x[0]).view(np.uint64) == np.float64(xb).view(np.uint64), (raw, xp, z, x[0], xb)
        zo = (y - raw[1] * xb) * (1.0 / sR)
        lb = fma(-0.5 * zo, zo, -float.fromhex('0x1.d67f1c864beb5p-1') - lib.smc_host_log(float(sR)))
        assert lw == lb, (raw, xp, z, y, lw, lb)


@pytest.mark.parametrize("model,kind,par", [
    (SV, AFFINE, [0.0, 0.5, 0.1, 1.0]), (SV, OPTIMAL, None), (UC, AFFINE, [0.0, 0.5, 0.1, 1.0]),     # pairs without a proposal
    (LG, 3, None), (LG, -1, None), (LG, NONE, None),                                                  # no such kind / nothing guided
    (LG, AFFINE, None), (LG, OPTIMAL, [0.0, 0.5, 0.1, 1.0]),                                          # rows with AFFINE and only then
    (LG, AFFINE, [0.0, 0.5, 0.1, 0.0]), (LG, AFFINE, [0.0, 0.5, 0.1, -1.0]), (LG, AFFINE, [0.0, 0.5, 0.1, np.nan]),
    (LG, AFFINE, [np.inf, 0.5, 0.1, 1.0]), (LG, AFFINE, [0.0, np.nan, 0.1, 1.0]), (LG, AFFINE, [0.0, 0.5, -np.inf, 1.0]),
    (7, OPTIMAL, None),
])
def test_refused_combinations(L, model, kind, par):
    raw = {LG: [0.5, 1.0, 0.9, 0.8, 0.0, 1.0], SV: [-1.0, 0.95, 0.25], UC: [0.2, 0.2, 3.0, 0.0, 0.0], 7: [0.0] * 6}[model]
    lib = L.lib()
    d = 3 if model == UC else 1
    a = np.zeros(d)
    out, lw = np.zeros(d), np.zeros(1)
    p = None if par is None else np.asarray(par, dtype=float)
    rc = lib.smc_host_guided_step(model, L._d(np.asarray(raw, dtype=float)), kind, L._d(p), L._d(a), L._d(a), 0.1, L._d(out), L._d(lw))
    assert rc == -1, rc                                    # SMC_EINVAL
    assert lib.smc_last_error()


def test_optimal_proposal_is_lg_only(L):
    lib = L.lib()
    par = np.zeros(4)
    for model, raw in ((SV, [-1.0, 0.95, 0.25]), (UC, [0.2, 0.2, 3.0, 0.0, 0.0])):
        assert lib.smc_host_optimal_proposal(model, L._d(np.asarray(raw, dtype=float)), L._d(par)) == -1
    assert lib.smc_host_optimal_proposal(LG, None, L._d(par)) == -1


def test_python_proposal_types():
    import sequential_monte_carlo_amd as smc
    from sequential_monte_carlo_amd import particles as P
    m = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
    p = smc.optimal_proposal(m)
    assert isinstance(p, smc.AffineGaussianProposal)
    ref = G.lg_optimal_row([0.5, 1.0, 0.9, 0.8])
    assert np.allclose(p.row, ref.astype(float), rtol=1e-15)
    assert P.proposal_rows(None, 3) == (0, None)
    assert P.proposal_rows(smc.OptimalProposal(), 3) == (2, None)
    kind, rows = P.proposal_rows(p, 3)
    assert kind == 1 and rows.shape == (3, 4)
    with pytest.raises(ValueError):
        P.proposal_rows("optimal", 1)
