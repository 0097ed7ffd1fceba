"""Planted clouds for the smoother tests, shared by the CPU tests (host twin against the long-double recursion,
tests/test_smoother_host.py) and the GPU tests (device == host twin, tests/test_gpu_smoother_edges.py): the recorded clouds
(x [T][d][n], w [T][n]) of ONE filter, changed where no filter run would put them.  Every variant is a function of its input alone.

The magnitudes.  The host twin rounds the centre m_l of a source before it subtracts (smc_spec.h "the smoother"), an error of
eps |m| |d| / (2 scale^2) in logf that the long-double reference does not make, and d = x - m is rounded once, eps d^2 / scale^2.
The twin's bound against the reference, (2 (CH + n / CH) + 200) eps per backward step, is a few hundred eps, so the planted
centres stay within a few tens of transition scales of 0 and the planted distances within about 80 scales:
  * the two groups of far_apart lie SEP = 64 scales apart (+-32): a cloud of SV1D is some 20 scales wide, so a cross term is at
    most about exp(-0.5 44^2) = exp(-968) against the row maximum, below the smallest subnormal exp(-745): exactly +0.0 in
    sp_exp, while (x_j - m_l)^2 s stays above -4000;
  * the lone target of far_apart lies FAR = 60 scales from the cloud: logD_j near -1800, far inside the range of a double and
    of the long double the reference works in.
The scale of a family is its transition's standard deviation in the row that is moved: sqrt(Q); sigma; gamma_eta (UCSV3D is
split in its third row, the log-volatility of the measurement noise, whose centre m = xp is exact, and the lone target is moved
there as well).
"""
import numpy as np

LG1D, SV1D, UCSV3D = 1, 2, 3
SEP, FAR, BLOCK = 64.0, 60.0, 50
TINY = 2.0 ** -1074                       # the smallest subnormal


def mid(T):
    """the step the one-step variants change: the middle, never the last of a record of more than one step"""
    return (T - 1) // 2


def _scale_row_gain(model, raw):
    """(transition sd, the state row that is moved, d centre / d source) of the row moved"""
    if model == LG1D:
        return float(np.sqrt(raw[2])), 0, float(raw[0])
    if model == SV1D:
        return float(raw[2]), 0, float(raw[1])
    return float(raw[1]), 2, 1.0


def nan_on_zero(x, w, value=np.nan):
    """`value` in every state row of every particle whose weight is 0"""
    x = x.copy()
    for r in range(x.shape[1]):
        x[:, r, :][w == 0] = value
    return x, w.copy()


def inf_on_zero(x, w):
    return nan_on_zero(x, w, np.inf)


def far_apart(model, raw, x, w):
    """steps ts and ts + 1 (ts = max(T // 2 - 1, 0)): blocks of BLOCK consecutive particles alternate between two groups, the
    targets SEP scales apart and the sources moved so that their centres are: a target's terms from the other group underflow.
    Last step: the heaviest particle lies FAR scales from where it was (as a target, from every source)."""
    x, w = x.copy(), w.copy()
    T, _, n = x.shape
    sd, r, gain = _scale_row_gain(model, raw)
    side = np.where((np.arange(n) // BLOCK) % 2 == 0, -0.5, 0.5) * SEP * sd
    if T >= 2:
        ts = max(T // 2 - 1, 0)
        x[ts + 1, r] += side
        x[ts, r] += side / gain
    x[T - 1, r, int(np.argmax(w[T - 1]))] += FAR * sd
    return x, w


def ties(x, w):
    """every particle of step mid(T) carries the state of the first: every pair term of that step ties up to the weights"""
    x = x.copy()
    t = mid(x.shape[0])
    x[t] = x[t, :, :1]
    return x, w.copy()


def tiny_weights(x, w):
    """step mid(T): the heaviest particle gets weight 1, every other positive weight becomes a subnormal (1 .. 7 units of the
    smallest one, by index); their sum is far below half an ulp of 1"""
    w = w.copy()
    t = mid(w.shape[0])
    pos = np.flatnonzero(w[t] > 0)
    top = int(np.argmax(w[t]))
    w[t, pos] = TINY * (1 + pos % 7)
    w[t, top] = 1.0
    return x.copy(), w


def one_alive(x, w):
    """step mid(T): the heaviest particle gets weight 1, every other weight is 0"""
    w = w.copy()
    t = mid(w.shape[0])
    top = int(np.argmax(w[t]))
    w[t] = 0.0
    w[t, top] = 1.0
    return x.copy(), w


def dead_at(x, w, t):
    """every weight of step t is 0: a collapsed filter"""
    w = w.copy()
    w[t] = 0.0
    return x.copy(), w


def dead_steps(T):
    return sorted({0, mid(T), T - 1})


ALIVE = ("far_apart", "ties", "tiny_weights", "one_alive")     # apply to every record
ON_ZERO = ("nan_on_zero", "inf_on_zero")                       # need weights that are exactly 0: a sharp-observation record


def variant(name, model, raw, x, w):
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    if name == "far_apart":
        return far_apart(model, raw, x, w)
    return {"nan_on_zero": nan_on_zero, "inf_on_zero": inf_on_zero, "ties": ties, "tiny_weights": tiny_weights,
            "one_alive": one_alive}[name](x, w)
