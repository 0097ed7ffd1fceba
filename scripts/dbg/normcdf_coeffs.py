"""Derives the constants of sp_normcdf (smc_spec.h "predictive checks") with mpmath and prints them as C hex floats.

The upper tail Q(a) = 1 - Phi(a), a >= 0, is written exp(-a^2 / 2) * H(s) with
    t = 1 / (1 + a / 4),   s = (t - tc) / th  in [-1, 1]  for a in [0, AMAX],
H(s) = Q / exp(-a^2 / 2) = Mills' ratio / sqrt(2 pi): smooth on the whole interval, interpolated at the N + 1 Chebyshev nodes and
converted to the monomial basis in s (the coefficients stay below 1 in magnitude: Horner's rule loses nothing).  Beyond AMAX the
argument of H is clamped: Q(AMAX) < 1.2e-19 bounds what that costs.

    python scripts/dbg/normcdf_coeffs.py            # the constants and the error of the polynomial itself (before rounding)
"""
import mpmath as mp

mp.mp.dps = 60
N = 20          # degree
P = mp.mpf(1) / 4
AMAX = 9


def tail_over_exp(a):
    return mp.erfc(a / mp.sqrt(2)) / 2 / mp.exp(-a * a / 2)


def derive():
    tlo = 1 / (1 + P * AMAX)
    tc, th = (1 + tlo) / 2, (1 - tlo) / 2
    M = N + 1
    nodes = [mp.cos(mp.pi * (k + mp.mpf(1) / 2) / M) for k in range(M)]
    fv = [tail_over_exp((1 / (tc + th * x) - 1) / P) for x in nodes]
    cheb = [2 / mp.mpf(M) * sum(fv[k] * mp.cos(mp.pi * j * (k + mp.mpf(1) / 2) / M) for k in range(M)) for j in range(M)]
    cheb[0] /= 2
    T = [[mp.mpf(1)], [mp.mpf(0), mp.mpf(1)]]
    for _ in range(2, M):
        nxt = [mp.mpf(0)] + [2 * v for v in T[-1]]
        for i, v in enumerate(T[-2]):
            nxt[i] -= v
        T.append(nxt)
    mono = [mp.mpf(0)] * M
    for j in range(M):
        for i, v in enumerate(T[j]):
            mono[i] += cheb[j] * v
    return tc, th, mono


def main():
    tc, th, mono = derive()
    print("S1 = %s   (1 / th)" % float(1 / th).hex())
    print("S0 = %s   (-tc / th)" % float(-tc / th).hex())
    for k in range(N, -1, -1):
        print("c[%2d] = %s" % (k, float(mono[k]).hex()))
    worst = mp.mpf(0)
    for i in range(4001):
        a = mp.mpf(AMAX) * i / 4000
        s = (1 / (1 + P * a) - tc) / th
        worst = max(worst, abs(mp.exp(-a * a / 2) * (mp.polyval(mono[::-1], s) - tail_over_exp(a))))
    print("largest |exp(-a^2/2) (H - polynomial)| on [0, %d] before any rounding: %s" % (AMAX, mp.nstr(worst, 3)))
    print("Q(%d) = %s" % (AMAX, mp.nstr(mp.erfc(AMAX / mp.sqrt(2)) / 2, 3)))


if __name__ == "__main__":
    main()
