"""An independent restatement of csrc/smc_spec.h "quantiles of the smoothed state" in Python integers: math.frexp for the parts
of a weight, round-half-even by hand, struct for the order key, a sort and a running sum for the definition.  It takes nothing
from the library.  Shared by test_smooth_quantiles_host.py (the host twin) and test_gpu_smooth_quantiles.py (the device call)."""
import math
import struct

import numpy as np

Q_BITS = 40                        # SMOOTH_Q_BITS
NAN = float("nan")
M64 = (1 << 64) - 1


def order_key(v):
    """the IEEE total order as an integer: -NaN < -inf < .. < -0.0 < +0.0 < .. < +inf < +NaN"""
    b = struct.unpack("<Q", struct.pack("<d", v))[0]
    return (~b & M64) if b >> 63 else b | (1 << 63)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def p64(p):
    """floor(p 2^64) clamped to [0, 2^64 - 1] (exact: p 2^64 is a power-of-two scaling)"""
    if not p > 0.0:
        return 0
    if p >= 1.0:
        return M64
    return int(p * 2.0 ** 64)


def takes_part(w):
    return 0.0 < w < math.inf          # (False for NaN)


def integer_weights(ws, bits_=Q_BITS):
    """(q [n] Python integers, K) of one cloud; K None when nobody takes part.  q_i = rint(ws_i 2^(bits - K)), ties to even, in
    exact integer arithmetic: ws_i = m 2^(e - 53) with the 53-bit integer m = f 2^53 of math.frexp (exact for subnormals too)"""
    parts = [math.frexp(float(w)) if takes_part(w) else None for w in ws]
    es = [fe[1] for fe in parts if fe is not None]
    if not es:
        return [0] * len(parts), None
    K = max(es)
    q = []
    for fe in parts:
        if fe is None:
            q.append(0)
            continue
        f, e = fe
        assert 0.5 <= f < 1.0
        m = int(f * 2.0 ** 53)                     # exact
        r = 53 - bits_ + (K - e)                   # q = m / 2^r, r >= 53 - bits > 0
        assert r > 0
        lo, rem, half = m >> r, m & ((1 << r) - 1), 1 << (r - 1)
        q.append(lo + (1 if rem > half or (rem == half and lo & 1) else 0))
    return q, K


def cloud_quantiles(x, ws, p, bits_=Q_BITS):
    """the quantiles of ONE cloud (x [n], ws [n]) at the levels p: a list of floats"""
    x, ws = [float(v) for v in x], [float(w) for w in ws]
    if any(w != w for w in ws):
        return [NAN] * len(p)
    q, K = integer_weights(ws, bits_)
    if K is None:
        return [NAN] * len(p)
    kv = sorted((order_key(v), qi, v) for v, qi in zip(x, q) if qi)
    W = sum(qi for _, qi, _ in kv)
    out = []
    for pj in p:
        T = (p64(float(pj)) * W) >> 64
        c = 0
        for _, qi, v in kv:                         # the first entry at which the running sum passes T; equal keys are adjacent
            c += qi
            if c > T:
                break
        # the value of the LAST entry with that key has the weight of all of them at or below it: the same value (equal keys are
        # equal bits), so v is the smallest value with the weight at or below it above T
        out.append(v)
    return out


def quantiles(x, ws, p, bits_=Q_BITS):
    """x, ws [T][n] -> [T][len(p)]"""
    x, ws = np.asarray(x, dtype=np.float64), np.asarray(ws, dtype=np.float64)
    return np.array([cloud_quantiles(x[t], ws[t], p, bits_) for t in range(ws.shape[0])], dtype=np.float64).reshape(ws.shape[0], len(p))


LEVELS8 = [0.0, 1.0, 0.5, 1e-300, 1.0 - 2.0 ** -53, 0.25, 0.75, 0.05]
LEVELS = {1: [0.5], 3: [0.25, 0.5, 0.75], 8: LEVELS8}
