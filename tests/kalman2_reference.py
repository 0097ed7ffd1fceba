"""TEST INFRASTRUCTURE: src/kalman_filter.jl:3-27 (the matrix method, d = 2, scalar y) and the RTS backward pass restated in
numpy longdouble with plain loops over t, in the textbook association - not the library's order of operations.  A row is the
library's (A11,A12,A21,A22, B1,B2, Q11,Q21,Q22, R, x01,x02, S11,S21,S22); every entry may be an array (one filter per entry,
elementwise), which is how the grid quadrature of the IBIS tests evaluates a few hundred rows.  Never imported by the product."""
import numpy as np

LD = np.longdouble
LOG2PI = LD("1.8378770664093454835606594728112352797227949472755668")


def _ld(row):
    return [np.asarray(v, dtype=LD) for v in row]


def filter_ld(row, y, predict_first=False):
    """-> xf [T][2], Sf [T][3] (S11, S21, S22), lik [T]  (each with the rows' own trailing shape), longdouble"""
    a11, a12, a21, a22, b1, b2, q11, q21, q22, R, x1, x2, s11, s21, s22 = _ld(row)
    xf, Sf, lik = [], [], []
    for t, yt in enumerate(np.asarray(y, dtype=LD)):
        if t > 0 or predict_first:                                   # xt = A*xt; Σt = A*Σt*A' + Q           :13-14
            x1, x2 = a11 * x1 + a12 * x2, a21 * x1 + a22 * x2
            m11, m12 = a11 * s11 + a12 * s21, a11 * s21 + a12 * s22
            m21, m22 = a21 * s11 + a22 * s21, a21 * s21 + a22 * s22
            s11, s21, s22 = m11 * a11 + m12 * a12 + q11, m21 * a11 + m22 * a12 + q21, m21 * a21 + m22 * a22 + q22
        k1, k2 = s11 * b1 + s21 * b2, s21 * b1 + s22 * b2           # Σt*B'
        sig = b1 * k1 + b2 * k2 + R                                  # σt = B*Σt*B' + R                      :16
        e = yt - (b1 * x1 + b2 * x2)                                 # Δyt                                   :17
        x1, x2 = x1 + k1 * e / sig, x2 + k2 * e / sig                # :20
        s11, s21, s22 = s11 - k1 * k1 / sig, s21 - k2 * k1 / sig, s22 - k2 * k2 / sig     # :21
        lik.append(-(LOG2PI + np.log(sig) + e * e / sig) / 2)        # :24-26
        xf.append(np.stack([x1, x2]))
        Sf.append(np.stack([s11, s21, s22]))
    return np.stack(xf), np.stack(Sf), np.stack(lik)


def smooth_ld(row, y, predict_first=False):
    """RTS: xs [T][2], Ps [T][3], longdouble (one row).  G = Sf A' P^-1; xs = xf + G (xs' - A xf); Ps = Sf + G (Ps' - P) G'"""
    r = _ld(row)
    A = np.array([[r[0], r[1]], [r[2], r[3]]], dtype=LD)
    Q = np.array([[r[6], r[7]], [r[7], r[8]]], dtype=LD)
    xf, Sf, _ = filter_ld(row, y, predict_first)
    full = lambda s: np.array([[s[0], s[1]], [s[1], s[2]]], dtype=LD)
    T = len(xf)
    xs, Ps = [None] * T, [None] * T
    xs[-1], Ps[-1] = xf[-1].copy(), full(Sf[-1])
    for t in range(T - 2, -1, -1):
        F = full(Sf[t])
        P = A @ F @ A.T + Q
        det = P[0, 0] * P[1, 1] - P[0, 1] * P[1, 0]
        Pinv = np.array([[P[1, 1], -P[0, 1]], [-P[1, 0], P[0, 0]]], dtype=LD) / det
        G = F @ A.T @ Pinv
        xs[t] = xf[t] + G @ (xs[t + 1] - A @ xf[t])
        Ps[t] = F + G @ (Ps[t + 1] - P) @ G.T
    return np.stack(xs), np.stack([np.array([p[0, 0], p[1, 0], p[1, 1]]) for p in Ps])


# ---- the rows the two-state tests share ---------------------------------------------------------------------------------
def hp_series(T=60):
    """the series of the Hodrick-Prescott identity"""
    rng = np.random.default_rng(3)
    return 0.5 * np.cumsum(rng.normal(size=T)) + rng.normal(size=T)


def hp_row(y, lam=1600.0, init_cov=1000.0):
    """hodrick_prescott(lam, y, init_cov) as a row, written out (state_space_models.jl:193-202)"""
    return np.array([2.0, -1.0, 1.0, 0.0, 1.0, 0.0, 1.0 / lam, 0.0, 0.0, 1.0, 3 * y[0] - 2 * y[1], 2 * y[0] - y[1], init_cov, 0.0, init_cov])


def random_pd_rows(n, seed=7):
    """n rows with |eig A| < 1 and positive-definite Q, Sigma0"""
    rng = np.random.default_rng(seed)
    rows = []
    while len(rows) < n:
        A = rng.normal(size=(2, 2)) * 0.6
        if np.abs(np.linalg.eigvals(A)).max() >= 0.95:
            continue
        LQ, LS = np.tril(rng.normal(size=(2, 2))) + np.diag([0.8, 0.8]), np.tril(rng.normal(size=(2, 2))) + np.diag([0.8, 0.8])
        Q, S = LQ @ LQ.T, LS @ LS.T
        B = rng.normal(size=2)
        rows.append([A[0, 0], A[0, 1], A[1, 0], A[1, 1], B[0], B[1], Q[0, 0], Q[1, 0], Q[1, 1], 0.3 + rng.random(), rng.normal(), rng.normal(),
                     S[0, 0], S[1, 0], S[1, 1]])
    return np.array(rows)


def embedded_scalar_row(a, b, q, R, m, s0):
    """the LG1D row (a, b, q, R, m, s0) as a two-state row whose second state is identically zero"""
    return np.array([a, 0.0, 0.0, 0.0, b, 0.0, q, 0.0, 0.0, R, m, 0.0, s0, 0.0, 0.0])


def pd_series(T, seed=11):
    return np.random.default_rng(seed).normal(size=T) * 1.5


def hp_trend(y, lam=1600.0):
    """the penalised-least-squares trend (I + lam D'D)^-1 y, D the second-difference matrix"""
    n = len(y)
    D = np.zeros((n - 2, n))
    for i in range(n - 2):
        D[i, i:i + 3] = [1.0, -2.0, 1.0]
    return np.linalg.solve(np.eye(n) + lam * D.T @ D, np.asarray(y, dtype=np.float64))


# ---- accuracy of the library's host twin against this restatement (test_kalman2_host (a); scripts/dbg/kalman2_accuracy.py) ----
def accuracy_cases():
    """(name, row, y) of check (a): HP with lam = 1600 at init_cov 1e3 and 1e6 over T = 200, twenty random positive-definite rows
    over T = 50"""
    rng = np.random.default_rng(5)
    yhp = 0.5 * np.cumsum(rng.normal(size=200)) + rng.normal(size=200)
    cases = [("hp init_cov=%g" % ic, hp_row(yhp, 1600.0, ic), yhp) for ic in (1e3, 1e6)]
    ypd = pd_series(50)
    return cases + [("pd %d" % i, r, ypd) for i, r in enumerate(random_pd_rows(20))]


def measure_accuracy(host_kalman2_steps):
    """{group: (|d logZ| / |logZ|, |d xf|, |d Sf|, |d Sf| / max |Sf|)}, group = each HP case and "pd", the maxima over the group's cases and both predict_first
    values, of host_kalman2_steps(row, y, predict_first) -> (xf, Sf, lik) against filter_ld"""
    out = {}
    for name, row, y in accuracy_cases():
        g = name if name.startswith("hp") else "pd"
        for pf in (False, True):
            xf, Sf, lik = host_kalman2_steps(row, y, pf)
            rx, rS, rl = filter_ld(row, y, pf)
            z, rz = LD(0), rl.sum()
            for v in lik:                                  # the library's logZ: the step values summed in step order
                z = LD(float(np.float64(z) + v))
            d = (float(abs(z - rz) / abs(rz)), float(np.abs(xf - rx).max()), float(np.abs(Sf - rS).max()),
                 float(np.abs(Sf - rS).max() / np.abs(rS).max()))
            out[g] = tuple(max(a, b) for a, b in zip(out.get(g, (0.0,) * 4), d))
    return out
