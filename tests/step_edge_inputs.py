"""The edge inputs of the one-step twin tests, shared by the GPU tests (device twin == host twin) and the CPU tests (batched host
twin == one-particle twin): signed zeros in states and normals, levels up to 1e5, log-volatilities in [-12, 4]."""
import numpy as np

UC = [0.2, 0.2, 3.0, 0.0, 0.0]
POOR = [0.3, 0.2, 0.1, 2.0]
AFFINE = 1
N = 4096


def guided(model, kind):
    """-> (raw, proposal row or None, xp [d][N], z [d][N], y)"""
    r = np.random.default_rng(100 * model + kind)
    n, d = N, (3 if model == 3 else 1)
    raw = [0.93, 1.3, 0.37, 0.11, 0.0, 1.0] if model == 1 else UC
    par = POOR if kind == AFFINE else None
    xp = r.normal(size=(d, n)) * 2
    xp[0] += np.repeat([0.0, 1e2, 1e5, -1e5], n // 4)
    if model == 3:
        xp[1:] = r.uniform(-12, 4, size=(2, n))
    z = r.normal(size=(d, n))
    z[:, :8] = 0.0
    z[:, 8:12] = -0.0
    xp[0, :4] = 0.0
    xp[0, 8:10] = -0.0
    return raw, par, xp, z, 0.7


def rb(first):
    """-> (raw, sp [4][N], z [2][N], y)"""
    r = np.random.default_rng(40 + first)
    n = N
    sp = np.stack([r.normal(size=n) * 2 + np.repeat([0.0, 1e2, 1e5, -1e5], n // 4), r.uniform(-12, 4, size=n), r.uniform(-12, 4, size=n),
                   np.exp(r.uniform(-14, 4, size=n))])
    z = r.normal(size=(2, n))
    z[:, :8] = 0.0
    z[:, 8:12] = -0.0
    sp[0, :4] = 0.0
    sp[0, 8:10] = -0.0
    raw = [0.2, 0.35, 1e5 if first else 3.0, -11.5, 3.5]
    return raw, sp, z, 0.7
