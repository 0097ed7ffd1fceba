"""TEST INFRASTRUCTURE: random call sequences on a filter handle, and a stateful CPU reference for them.

A filter handle (smc_filter_s, csrc/smc_host.h) is a state machine: beside the device buffers it keeps host-side caches and flags
(cur, t, emitted, the pending window, the cached break points, the by-value copies of row 0, the pinned twins, the recycled
bundle) that every call must leave consistent.  This module walks many call orders over it:

  ops        small tuples (name, target, args...) of plain data; target 0 / 1 is one of TWO handles of the same geometry, so that
             slot copies have a source that walks a sequence of its own.  A failing sequence prints as something to paste back.
  Model      the legality model: the contract of include/smc_hip.h ("THE PENDING WINDOW", "REFUSED CALLS") written down -
             which ops drop a pending window, which keep it, and which error a call must give in which state.
  sequence   (profile, seed, length) -> ops, deterministic (numpy.random.default_rng only).  Every sequence works through its
             share of a PLAN: the table of ordered pairs (op that drops or moves something -> next consuming op) and of the
             triples window -> setter -> commit(j class), so that the committed seed list covers the whole table.
  replay     drives anything with the interface of sequential_monte_carlo_amd._lib.Handle and hands every op's result (return
             values, error code, snapshot of the target handle) to a callback.
  ReferenceHandle   tests/oracle_backend.py::OracleHandle plus what the C ABI has and it lacks: reseed, set_streams, traces,
             weights_raw, logZ, a handle-wide time index, the skip mask, slot packing, the window contract, the refusals.

A log_likelihood op may carry a skip mask (set_skip, the call, set_skip(None)) and a step_window op the flag for per-step
summaries (set_summaries, the call, get_summaries, set_summaries()); the summaries are checked against the reference's clouds
under the bounds of tests/summary_reference.py, everything else bit for bit.  The readers moments, quantiles, forecast,
forecast_cloud and predictive are checked for "changes nothing" only.

Needs no GPU and no library beyond numpy.  Not covered (follow-ups): guided / missing / conditional / marginal-UCSV handles, the
record and the smoothers, smc_pmmh_rejuvenate, the IBIS handle, smc_comm_exchange_slots."""
import re
import zlib

import numpy as np

from oracle import binding as ob
from oracle_backend import OracleHandle
from sequential_monte_carlo_amd._lib import SmcError

EINVAL, ESTATE = -1, -3        # SMC_EINVAL, SMC_ESTATE (include/smc_hip.h)
WIN_MAX = 64

RAW = {1: [0.5, 1.0, 0.9, 0.8, 0.0, 1.0], 2: [-1.0, 0.95, 0.25], 3: [0.2, 0.2, 3.0, 0.0, 0.0]}
Y_CENTRE = {1: 0.0, 2: 0.0, 3: 2.5}


# ---- profiles: the smallest shapes at which each host path differs ------------------------------------------------------------
def _p(name, nth, n, seg, models=(1, 2, 3), systematic=False, no_resident=False, pointer=False):
    return dict(name=name, n_theta=nth, n=n, seg=seg, models=models, systematic=systematic, no_resident=no_resident,
                pointer=pointer, windows=n <= seg)


PROFILES = {p["name"]: p for p in (
    _p("one-multi", 1, 3 * 256 + 5, 256),                      # four segments, ragged tail, by-value launches, break-point cache
    _p("one-multi-ptr", 1, 3 * 256 + 5, 256, models=(1,), pointer=True),   # the same through the pointers
    _p("one-res", 1, 300, 512),                                # LDS-resident, windows, by value
    _p("one-nores", 1, 300, 512, no_resident=True),            # SMC_FLAG_NO_RESIDENT
    _p("batch-res", 3, 253, 256),                              # distinct rows and streams per slot, windows
    _p("batch-sync", 65, 100, 256, models=(1,)),               # above the 64-filter ticket limit: stream synchronisation
    _p("batch-multi", 3, 2 * 256 + 5, 256),                    # multi-segment batch
    _p("sys-batch-res", 3, 253, 256, systematic=True),         # the same shapes with SMC_FLAG_SYSTEMATIC
    _p("sys-one-multi", 1, 3 * 256 + 5, 256, systematic=True),
)}
SEEDS = tuple(range(8))        # the committed seed list of every profile
LENGTH = 72                    # ops per sequence (the coverage condition of tests/test_handle_sequences_host.py needs them)


def rows(model, nth, rid):
    """parameter rows [nth][nraw]: distinct per filter (filters cannot stand in for one another) and per rid"""
    out = np.tile(np.array(RAW[model], dtype=np.float64), (nth, 1))
    f = 1.0 - 0.3 * np.arange(nth) / nth
    g = 0.8 + 0.05 * (rid % 8)
    if model == 1:
        out[:, 0] *= f * g
        out[:, 3] *= g
    elif model == 2:
        out[:, 0] *= g
        out[:, 1] *= f
    else:
        out[:, 0] *= g
        out[:, 2] *= f
    return out


# ---- the vocabulary ----------------------------------------------------------------------------------------------------------
SETTERS = ("set_params", "set_streams", "reseed")
MUTATORS = SETTERS + ("init", "step", "log_likelihood", "step_window", "step_commit", "permute", "copy_from", "pack_unpack", "recreate")
CONSUMERS = ("step", "step_window", "step_commit", "log_likelihood", "permute", "copy_from")
READERS = ("state", "weights_raw", "logZ", "moments", "quantiles", "forecast", "forecast_cloud", "predictive", "pack_slots",
           "slot_bytes", "launch_geometry", "step_by_value", "synchronize")
REFUSED = ("commit_none", "commit_over", "commit_neg", "window_k0", "window_k65", "window_multi", "permute_oob", "unpack_oob",
           "copy_other_n", "copy_self")
J_CLASSES = ("zero", "mid", "all")
SUMM_P = [0.25, 0.5, 0.75]     # the levels of the per-step summaries inside a window
# the refused calls a handle with a pending window can be given: each must leave the window pending
KEPT_REFUSALS = ("commit_over", "commit_neg", "window_k0", "window_k65", "permute_oob", "unpack_oob", "copy_other_n", "copy_self")


def mutated_handle(op):
    """the handle whose filters, rows, seed or streams the op changes (its target; pack_unpack: the receiver)"""
    return op[3] if op[0] == "pack_unpack" else op[1]


def j_class(j, k):
    return "zero" if j == 0 else ("all" if j == k else "mid")


class Model:
    """What the contract lets a caller know about ONE handle without looking at the device."""

    def __init__(self, profile):
        self.single = profile["windows"]
        self.n_theta = profile["n_theta"]
        self.have_params = self.inited = False
        self.win_k = 0         # steps of the pending window, 0 = none
        self.t = 0
        self.streams = None    # the ids of the last set_streams (None: none yet on this handle)


def outcome(st, op):
    """0 when the library must accept op in the states st = [Model, Model], the error code when it must refuse it, None when the
    op is outside the vocabulary in that state (the generator never emits it)."""
    name, tgt = op[0], op[1]
    s = st[tgt]
    if name == "set_streams":
        # _lib.Handle.set_streams does not hand ids to the library that equal the ones it set last: such a call changes nothing
        # and keeps a pending window.  It is outside the vocabulary: the generator never repeats ids.
        return 0 if len(op[2]) == s.n_theta and tuple(op[2]) != s.streams else None
    if name in ("set_params", "reseed", "recreate"):
        return 0
    if name == "init":
        return 0 if s.have_params else None
    if name == "log_likelihood":
        if len(op) > 4 and not (s.inited and len(op[4]) == s.n_theta):   # with a skip mask: the skipped filters keep a state
            return None
        return 0 if s.have_params and 2 <= len(op[2]) <= 5 else None
    if name == "step":
        return 0 if s.inited else None
    if name == "step_window":
        return 0 if s.inited and s.single and 1 <= len(op[2]) <= WIN_MAX else None
    if name == "step_commit":                       # after a setter (or any other op that dropped the window): ESTATE
        if not s.win_k:
            return ESTATE
        return 0 if 0 <= op[2] <= s.win_k else None
    if name == "permute":
        return 0 if s.inited and all(0 <= a < s.n_theta for a in op[2]) else None
    if name == "copy_from":
        return 0 if s.inited and st[1 - tgt].inited else None
    if name == "pack_unpack":
        src, pidx, dst, didx = op[1:]
        ok = st[src].inited and st[dst].inited and len(didx) <= len(pidx) and len(set(didx)) == len(didx) and len(pidx) >= 1
        return 0 if ok and all(0 <= i < s.n_theta for i in list(pidx) + list(didx)) else None
    if name == "read":
        return 0 if s.inited and op[2] in READERS else None
    if name == "refuse":
        kind = op[2]
        if not s.inited:
            return None
        if kind == "commit_none":
            return ESTATE if not s.win_k else None
        if kind in ("commit_over", "commit_neg"):
            return EINVAL if s.win_k else None
        if kind in ("window_k0", "window_k65"):
            return EINVAL
        if kind == "window_multi":
            return EINVAL if not s.single else None
        if kind in ("permute_oob", "unpack_oob", "copy_other_n", "copy_self"):
            return EINVAL
    return None


def legal(st, op):
    return outcome(st, op) is not None


def apply(st, op):
    """the states after op (in place).  THE CONTRACT: what changes rows, seed, streams or the filters drops a pending window; what
    only reads, and every refused call, keeps it."""
    rc = outcome(st, op)
    assert rc is not None, ("illegal op", op)
    if rc:
        return rc
    name, tgt = op[0], op[1]
    s = st[tgt]
    if name in SETTERS:
        s.win_k = 0
        if name == "set_params":
            s.have_params = True
        if name == "set_streams":
            s.streams = tuple(op[2])
    elif name == "init":
        s.win_k, s.inited, s.t = 0, True, 1
    elif name == "step":
        s.win_k, s.t = 0, s.t + 1
    elif name == "log_likelihood":
        s.win_k, s.inited, s.t = 0, True, len(op[2])
    elif name == "step_window":
        s.win_k = len(op[2])
    elif name == "step_commit":
        s.win_k, s.t = 0, s.t + op[2]
    elif name == "permute":
        s.win_k = 0
    elif name == "copy_from":
        s.win_k, s.t = 0, st[1 - tgt].t             # the destination takes the source's time index, whatever the mask
    elif name == "pack_unpack":
        st[op[3]].win_k = 0                          # the receiver; the packed handle only reads
    elif name == "recreate":
        st[tgt] = Model.__new__(Model)
        st[tgt].__dict__.update(single=s.single, n_theta=s.n_theta, have_params=True, inited=True, win_k=0, t=1, streams=None)
    return 0


# ---- the plan: what the seed list of a profile must cover -----------------------------------------------------------------------
def pair_table(profile):
    """every ordered pair (mutator -> next consuming op on the same handle), every (setter between step_window and step_commit,
    j class), and every reader and refused call between a step_window and the step_commit that it must not disturb; without the
    window ops on profiles that have no windows.  ("keep", "copy_source"): a copy_from INTO the other handle with this one, its
    window pending, as the source - a reader of this handle."""
    win = profile["windows"]
    skip = () if win else ("step_window", "step_commit")
    pairs = [("pair", a, b) for a in MUTATORS if a not in skip for b in CONSUMERS if b not in skip]
    trip = [("win", s, j) for s in SETTERS for j in J_CLASSES] if win else []
    keep = [("keep", k) for k in READERS + KEPT_REFUSALS + ("copy_source",)] if win else []
    return pairs + trip + keep


def covered(profile, ops):
    """the items of pair_table(profile) that the sequence ops contains"""
    got = set()
    last = {0: None, 1: None}       # per handle: the last mutator
    chain = {0: None, 1: None}      # per handle: (setter,) once a setter has followed a step_window directly
    kwin = {0: 0, 1: 0}
    pend = {0: None, 1: None}       # per handle: the readers and refused calls since a step_window that still pends
    st = [Model(profile), Model(profile)]
    for op in ops:
        name = op[0]
        rc = apply(st, op)
        if name in ("read", "refuse"):
            if pend[op[1]] is not None:
                pend[op[1]].append(op[2])
            continue
        h = mutated_handle(op)
        if name == "copy_from" and pend[1 - h] is not None:
            pend[1 - h].append("copy_source")
        if name == "pack_unpack" and op[1] != h and pend[op[1]] is not None:
            pend[op[1]].append("pack_slots")
        if name == "step_commit" and pend[h] is not None:
            got.update(("keep", k) for k in pend[h])
        pend[h] = [] if name == "step_window" else None
        if name in CONSUMERS and last[h] is not None:
            got.add(("pair", last[h], name))
        if name == "step_commit" and chain[h] is not None:
            got.add(("win", chain[h], j_class(op[2], kwin[h])))
        chain[h] = name if (name in SETTERS and last[h] == "step_window") else None
        if name == "step_window":
            kwin[h] = len(op[2])
        if rc == 0:                 # a refused commit consumes (it shows that the window is gone) but has moved nothing
            last[h] = name
    return got & set(pair_table(profile))


def _crc(s):
    return zlib.crc32(s.encode())


def sequence(profile, seed, length=LENGTH, model=1):
    """The ops of (profile, seed): a prologue that brings both handles to life, then this seed's share of the plan (every
    len(SEEDS)-th item of the profile's shuffled table), each item as `a, [a reader or a refused call], b`, with whatever makes a
    and b legal in front.  Cut at `length`."""
    if isinstance(profile, str):
        profile = PROFILES[profile]
    nth, win = profile["n_theta"], profile["windows"]
    table = pair_table(profile)
    order = np.random.default_rng([_crc(profile["name"]), 0xC0FFEE]).permutation(len(table))
    mine = [table[i] for i in order[seed % len(SEEDS)::len(SEEDS)]]
    rng = np.random.default_rng([_crc(profile["name"]), seed, model])
    st = [Model(profile), Model(profile)]
    ops = []
    counter = [0, 0]
    lastk = [2, 2]

    def obs(k=None):
        y = np.round(Y_CENTRE[model] + 0.8 * rng.standard_normal(k or 1), 3)
        return [float(v) for v in y] if k else float(y[0])

    def emit(op):
        assert legal(st, op), op
        ops.append(op)
        apply(st, op)

    def fresh():
        counter[0] += 1
        return counter[0]

    def ensure(tgt, inited=True, window=False):
        if not st[tgt].have_params:
            emit(("set_params", tgt, fresh()))
        if inited and not st[tgt].inited:
            emit(("init", tgt, obs()))
        if window and not st[tgt].win_k:
            make("step_window", tgt)

    def pick_j(tgt):
        k = st[tgt].win_k or lastk[tgt]
        cls = J_CLASSES[int(rng.integers(3))]
        return 0 if cls == "zero" else (k if cls == "all" else int(rng.integers(1, k)))

    def make(name, tgt, j=None):
        if name == "set_params":
            emit((name, tgt, fresh()))
        elif name == "set_streams":
            ids = st[tgt].streams
            while ids == st[tgt].streams:                           # never the ids of the last call (they would not reach the library)
                ids = tuple(int(v) for v in rng.choice(4096, nth, replace=False))
            emit((name, tgt, list(ids)))
        elif name == "reseed":
            emit((name, tgt, int(rng.integers(1, 1 << 31))))
        elif name == "init":
            ensure(tgt, inited=False)
            emit((name, tgt, obs()))
        elif name == "step":
            ensure(tgt)
            emit((name, tgt, obs()))
        elif name == "log_likelihood":
            ensure(tgt, inited=False)
            op = (name, tgt, obs(int(rng.integers(2, 6))), bool(rng.integers(2)))
            if st[tgt].inited and rng.integers(2) == 0:             # set_skip, log_likelihood, set_skip(None)
                counter[1] += 1
                mask = [int(v) for v in rng.integers(0, 2, nth)]
                if nth > 1:                                         # some skipped, some run
                    i, j = rng.permutation(nth)[:2]
                    mask[i], mask[j] = 1, 0
                op += ([1] * nth if (seed + counter[1]) % 3 == 0 else mask,)
            emit(op)
        elif name == "step_window":
            ensure(tgt)
            lastk[tgt] = int(rng.integers(2, 6))
            # (every third with set_summaries, get_summaries around it; the systematic resampler has windows without summaries)
            emit((name, tgt, obs(lastk[tgt])) + ((True,) if not profile["systematic"] and rng.integers(3) == 0 else ()))
        elif name == "step_commit":
            emit((name, tgt, pick_j(tgt) if j is None else j))
        elif name == "permute":
            ensure(tgt)
            a = list(range(nth)) if rng.integers(4) == 0 else [int(v) for v in rng.integers(0, nth, nth)]
            emit((name, tgt, a))
        elif name == "copy_from":
            ensure(tgt)
            ensure(1 - tgt)
            c = int(rng.integers(4))
            mask = [0] * nth if c == 0 else ([1] * nth if c == 1 else [int(v) for v in rng.integers(0, 2, nth)])
            emit((name, tgt, mask))
        elif name == "pack_unpack":
            src = tgt if rng.integers(2) else 1 - tgt
            ensure(tgt)
            ensure(src)
            kp = int(rng.integers(1, nth + 3))                    # repeats allowed, k > n_theta included
            pidx = [int(v) for v in rng.integers(0, nth, kp)]
            didx = [int(v) for v in rng.permutation(nth)[:int(rng.integers(1, min(kp, nth) + 1))]]
            emit((name, src, pidx, tgt, didx))
        elif name == "recreate":
            ensure(tgt)
            if st[tgt].t < 2:                                       # the handle that goes has done some work: its bundle is not fresh
                emit(("step", tgt, obs()))
            emit((name, tgt, int(rng.integers(1, 1 << 31)), fresh(), obs()))
        else:
            raise ValueError(name)

    def filler(tgt):
        """a reader or a refused call on tgt (both must leave everything as it is, a pending window included)"""
        if not st[tgt].inited:
            return
        c = int(rng.integers(4))
        if c == 0:
            return
        if c == 1:
            emit(("read", tgt, READERS[int(rng.integers(len(READERS)))]))
            return
        if c == 2 and st[1 - tgt].inited and not st[1 - tgt].win_k and rng.integers(2):
            make("copy_from", 1 - tgt)                              # this handle as the SOURCE of a copy: it only reads
            return
        kinds = [k for k in REFUSED if legal(st, ("refuse", tgt, k))]
        kind = kinds[int(rng.integers(len(kinds)))]
        emit(("refuse", tgt, kind) + ((st[tgt].win_k + 1,) if kind == "commit_over" else ()))

    def free_walk(tgt):
        """between two items of the plan: a window that readers and refused calls must leave pending, or any mutator"""
        c = int(rng.integers(8))
        if c < (5 if win else 2):
            return
        if win and c < 7:
            make("step_window", tgt)
            for _ in range(int(rng.integers(1, 4))):
                filler(tgt)
            make("step_commit", tgt)
            return
        names = [m for m in MUTATORS if win or m not in ("step_window", "step_commit")]
        make(names[int(rng.integers(len(names)))], tgt)
        filler(tgt)

    make("set_params", 0)
    make("init", 0)
    make("set_params", 1)
    make("init", 1)
    for item in mine:
        tgt = 0 if rng.integers(4) else 1
        if item[0] == "keep":                                       # window, reader or refused call, commit: the commit goes through
            make("step_window", tgt)
            kind = item[1]
            if kind == "copy_source":
                make("copy_from", 1 - tgt)
                make("step_commit", tgt)
                continue
            emit(("read", tgt, kind) if kind in READERS else ("refuse", tgt, kind) + ((st[tgt].win_k + 1,) if kind == "commit_over" else ()))
            make("step_commit", tgt)
            continue
        if item[0] == "win":                                        # window, setter, commit(j class): the commit must be refused
            _, setter, cls = item
            make("step_window", tgt)
            k = st[tgt].win_k
            if rng.integers(2):
                filler(tgt)
                if not st[tgt].win_k:                               # (a copy into the other handle cannot drop it; kept as a guard)
                    make("step_window", tgt)
                    k = st[tgt].win_k
            make(setter, tgt)
            make("step_commit", tgt, 0 if cls == "zero" else (k if cls == "all" else int(rng.integers(1, k))))
            continue
        _, a, b = item
        if a == "step_commit":
            ensure(tgt, window=True)
        elif win and b == "step_commit" and a != "step_window" and a != "recreate":
            ensure(tgt, window=True)                                # window, a, commit: a must have dropped the window
        if a == "copy_from" or a == "pack_unpack":
            ensure(1 - tgt)
        if a == "step_window" and st[tgt].win_k:
            make("step_commit", tgt)
        make(a, tgt)
        filler(tgt)                                                 # (it leaves this handle alone: b is the next op that consumes a)
        make(b, tgt)
        free_walk(tgt)
    return ops[:length]


# ---- replay -------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(u, v):
    """bit for bit; floats through the uint64 view, a NaN equal to a NaN whatever its payload"""
    if u is None or v is None:
        return u is None and v is None
    u, v = np.asarray(u), np.asarray(v)
    if u.shape != v.shape:
        return False
    if u.dtype.kind == "f" or v.dtype.kind == "f":
        bu, bv = bits(u), bits(v)
        return bool(np.all((bu == bv) | (np.isnan(u) & np.isnan(v))))
    return bool(np.array_equal(u, v))


SNAP_KEYS = ("x", "w", "C", "m", "S", "S2hi", "S2lo", "logZ", "ess")


def snapshot(h):
    """what a caller can read of the filters: state() x and w, weights_raw(), logZ(); None before the first init"""
    try:
        x, w, a = h.state()
    except SmcError:
        return None, None
    C, m, S, hi, lo = h.weights_raw()
    z, e = h.logZ()
    return dict(zip(SNAP_KEYS, (x, w, C, m, S, hi, lo, z, e))), a


def snap_diff(p, q):
    if p is None or q is None:
        return [] if p is None and q is None else ["snapshot"]
    return [k for k in SNAP_KEYS if not same(p[k], q[k])]


def err_code(e):
    m = re.match(r"libsmchip error (-?\d+)", str(e))
    assert m, e
    return int(m.group(1))


def _ptr(buf):
    return buf.data_ptr() if hasattr(buf, "data_ptr") else buf


def replay(handle_like, other_like, ops, check, make=None, alloc=None, prefix=None, model=1):
    """Drive handle_like (target 0) and other_like (target 1) through ops[:prefix] and call check(i, op, result) after every op.
    result: ret (a tuple of the call's arrays, or None), err (the code of the SmcError the call raised, or None), snap (the
    snapshot of the handle the op concerns, after it), anc (its ancestors, after init / step / log_likelihood only; with a skip
    mask those of the filters that ran), anc_kept (with a skip mask: the skipped filters' ancestors equal this handle's own of
    before the call), unchanged (readers and refused calls: the snapshot equals the one before; a copy_from or a pack_unpack
    between two handles: the SOURCE's does).
    make(which, seed) -> a new handle-like of the same model, shape and flags for which = 0, 1 (recreate), and one of ANOTHER n_x
    for which = 2; alloc(h, k) -> a buffer of k packed slots of h (anything with data_ptr(), or what the handle-like takes)."""
    H = [handle_like, other_like]
    nth = handle_like.n_theta
    other_n = [None]
    snaps = [snapshot(H[0])[0], snapshot(H[1])[0]]
    ancs = [None, None]                              # the ancestors each handle read last
    for i, op in enumerate(ops[:prefix]):
        name, tgt = op[0], op[1]
        h = H[tgt]
        ret = err = anc = summ = anc_kept = None
        concern = mutated_handle(op)
        try:
            if name == "set_params":
                h.set_params(rows(model, nth, op[2]))
            elif name == "set_streams":
                h.set_streams(np.array(op[2], dtype=np.uint32))
            elif name == "reseed":
                h.reseed(op[2])
            elif name == "init":
                ret = (h.init(op[2]),)
            elif name == "step":
                ret = h.step(op[2])
            elif name == "log_likelihood":
                if len(op) > 4:
                    h.set_skip(np.array(op[4], dtype=np.uint8))
                try:
                    ret = h.log_likelihood(np.array(op[2]), trace=True) if op[3] else (h.log_likelihood(np.array(op[2])),)
                finally:
                    if len(op) > 4:
                        h.set_skip(None)
            elif name == "step_window":
                if len(op) > 3 and op[3]:
                    h.set_summaries(SUMM_P, 0, True)
                    try:
                        ret = h.step_window(np.array(op[2]))
                        summ = h.get_summaries(len(op[2]))
                    finally:
                        h.set_summaries()
                else:
                    ret = h.step_window(np.array(op[2]))
            elif name == "step_commit":
                h.step_commit(op[2])
            elif name == "permute":
                h.permute(np.array(op[2], dtype=np.int32))
            elif name == "copy_from":
                h.copy_from(H[1 - tgt], np.array(op[2], dtype=np.uint8))
            elif name == "pack_unpack":
                src, pidx, dst, didx = op[1:]
                buf = alloc(H[src], len(pidx))
                H[src].pack_slots(np.array(pidx, dtype=np.int32), _ptr(buf))
                H[src].synchronize()
                H[dst].unpack_slots(np.array(didx, dtype=np.int32), _ptr(buf))
                H[dst].synchronize()
                del buf
            elif name == "recreate":
                h.close()
                H[tgt] = h = make(tgt, op[2])
                h.set_params(rows(model, nth, op[3]))
                ret = (h.init(op[4]),)
            elif name == "read":
                _read(h, H[1 - tgt], op[2], alloc)
            elif name == "refuse":
                _refuse(h, op, alloc, make, other_n, model)
            else:
                raise ValueError(op)
        except SmcError as e:
            err = err_code(e)
            if err not in (EINVAL, ESTATE):          # a HIP or memory error is no refusal: the replay ends here
                raise
        snap, a = snapshot(H[concern])
        if name in ("init", "step", "log_likelihood", "recreate") and err is None:
            anc = a                                  # (the ancestors belong to the last launch; a skipped filter had none in it)
            if name == "log_likelihood" and len(op) > 4:
                skipped = np.array(op[4]) != 0   # ... and keeps the ones it had: against this handle's own ancestors of before
                anc = a[~skipped]
                anc_kept = same(a[skipped], ancs[concern][skipped])
        unchanged = None
        if name in ("read", "refuse") or err is not None:
            unchanged = not snap_diff(snaps[concern], snap)
        elif name == "copy_from" or (name == "pack_unpack" and op[1] != concern):
            src = 1 - concern                        # the SOURCE of a slot move only reads: its snapshot is the one of before
            unchanged = not snap_diff(snaps[src], snapshot(H[src])[0])
        snaps[concern], ancs[concern] = snap, a
        check(i, op, dict(ret=ret, err=err, snap=snap, anc=anc, unchanged=unchanged, summ=summ, anc_kept=anc_kept))
    if other_n[0] is not None:
        other_n[0].close()
    return H


def _read(h, other, kind, alloc):
    if kind == "state":
        h.state()
    elif kind == "weights_raw":
        h.weights_raw()
    elif kind == "logZ":
        h.logZ()
    elif kind == "moments":
        h.moments()
    elif kind == "quantiles":
        h.quantiles([0.1, 0.5, 0.9])
    elif kind == "forecast":
        h.forecast(2, 77, p=[0.25, 0.75])
    elif kind == "forecast_cloud":
        h.forecast_cloud(2, 78)
    elif kind == "predictive":
        h.predictive(0.3)
    elif kind == "pack_slots":
        buf = alloc(h, 2)
        h.pack_slots(np.array([h.n_theta - 1, 0], dtype=np.int32), _ptr(buf))
        h.synchronize()
    elif kind == "slot_bytes":
        assert h.slot_bytes() > 0
    elif kind == "launch_geometry":
        h.launch_geometry()
    elif kind == "step_by_value":
        h.step_by_value
    elif kind == "synchronize":
        h.synchronize()
    else:
        raise ValueError(kind)


def _refuse(h, op, alloc, make, other_n, model):
    nth, kind = h.n_theta, op[2]
    if kind == "commit_none":
        h.step_commit(1)
    elif kind == "commit_over":
        h.step_commit(op[3])                # k + 1
    elif kind == "commit_neg":
        h.step_commit(-1)
    elif kind == "window_k0":
        h.step_window(np.zeros(0))
    elif kind == "window_k65":
        h.step_window(np.zeros(WIN_MAX + 1))
    elif kind == "window_multi":
        h.step_window(np.zeros(2))
    elif kind == "permute_oob":
        a = np.arange(nth, dtype=np.int32)
        a[-1] = nth
        h.permute(a)
    elif kind == "unpack_oob":
        buf = alloc(h, 1)
        h.pack_slots(np.array([0], dtype=np.int32), _ptr(buf))
        h.synchronize()
        h.unpack_slots(np.array([nth], dtype=np.int32), _ptr(buf))
    elif kind == "copy_other_n":
        if other_n[0] is None:
            other_n[0] = make(2, 5)
            other_n[0].set_params(rows(model, nth, 0))
            other_n[0].init(0.25)
        h.copy_from(other_n[0], np.ones(nth, dtype=np.uint8))
    elif kind == "copy_self":
        h.copy_from(h, np.ones(nth, dtype=np.uint8))
    else:
        raise ValueError(kind)
    raise AssertionError("the refused call %r was accepted" % kind)


def result_diff(p, q):
    """the compared quantities in which two results of the same op differ"""
    out = []
    if p["err"] != q["err"]:
        out.append("err")
    if (p["ret"] is None) != (q["ret"] is None):
        out.append("ret")
    elif p["ret"] is not None and len(p["ret"]) != len(q["ret"]):
        out.append("ret")
    elif p["ret"] is not None:
        out += ["ret[%d]" % k for k, (u, v) in enumerate(zip(p["ret"], q["ret"])) if not same(u, v)]
    out += snap_diff(p["snap"], q["snap"])
    if p["anc"] is not None and q["anc"] is not None and not same(p["anc"], q["anc"]):
        out.append("anc")
    if p["unchanged"] != q["unchanged"]:
        out.append("unchanged")
    if p["anc_kept"] != q["anc_kept"]:
        out.append("anc_kept")
    if (p["summ"] is None) != (q["summ"] is None):
        out.append("summ")
    elif p["summ"] is not None:
        out += summ_diff(p["summ"], q["summ"])
    return out


def summ_diff(a, b):
    """the per-step summaries of a window.  A reference handle hands over the clouds themselves, a list of (x [d][n_theta][n], w
    [n_theta][n]) per step; the library (q [k][n_theta][np], mean, var [k][d][n_theta]), checked against the clouds under the
    bounds of tests/summary_reference.py as everywhere"""
    if isinstance(b, list):
        a, b = b, a
    if isinstance(b, list):                                          # two references: the same clouds
        ok = len(a) == len(b) and all(same(u[0], v[0]) and same(u[1], v[1]) for u, v in zip(a, b))
        return [] if ok else ["summ"]
    import math
    from summary_reference import check_moments, check_quantiles, quantile_delta
    q, mean, var = b
    try:
        assert q.shape[0] == mean.shape[0] == var.shape[0] == len(a)
        for t, (x, w) in enumerate(a):
            d, nth, n = x.shape
            seg = 256
            while seg < n:
                seg <<= 1
            for m in range(nth):
                for c in range(d):
                    check_moments(mean[t, c, m], var[t, c, m], x[c, m], w[m], (t, m, c))
                check_quantiles(q[t, m], SUMM_P, x[0, m], w[m], quantile_delta(n, 1, seg, math.fsum(w[m])), (t, m))
    except AssertionError as e:
        return ["summ: %s" % (e,)]
    return []


# ---- the reference --------------------------------------------------------------------------------------------------------------
def _refuse_ref(code, msg):
    raise SmcError("libsmchip error %d: %s" % (code, msg))


def _t_word(f):
    """where an exported oracle filter keeps its time index (oracle/smc_oracle.c orc_filter_export: x, logw, a, C, five segment
    records, K, Dtot, Rtot, logmu, ess, t)"""
    return f.d * f.n + 2 * f.n + f.nseg * f.seg + 5 * f.nseg + 5


class ReferenceHandle(OracleHandle):
    """OracleHandle with the C ABI's contract: created without rows, one time index for the whole handle, logZ kept per filter and
    moved with the slots, a window that leaves the filters where they stand until it is committed and that every call that
    changes rows, seed, streams or the filters drops, and the library's refusals (SmcError with the same code)."""

    def __init__(self, model_id, n_theta, N, seg, seed, systematic=False):
        blank = np.tile(np.array(self._blank_raw(model_id), dtype=np.float64), (n_theta, 1))
        OracleHandle.__init__(self, model_id, blank, N, seg, seed, np.arange(n_theta), systematic)
        self.n_x = N
        self.d = ob.MODEL_DIM[model_id]
        self.raws, self.seed = blank, seed
        self.streams = np.arange(n_theta, dtype=np.uint32)
        self._streams_set = None
        self.have_params = self.inited = False
        self.t = 0
        self.ft = [0] * n_theta          # the time index each oracle filter carries (a value copy brings its source's along)
        self.z = np.zeros(n_theta)
        self.win = None                  # the pending window: (y, filters run ahead, logmu [k][n_theta])
        self.skip = None                 # smc_set_skip: the filters the following log_likelihood calls leave out
        self._clouds = []

    @staticmethod
    def _blank_raw(model_id):
        return [0.5, 1, 1, 1, 0, 1] if model_id == 1 else ([0, 0.5, 1] if model_id == 2 else [1, 1, 0, 0, 0])

    def close(self):
        self.f = None

    def synchronize(self):
        pass

    # -- helpers
    def _twin(self, m):
        """a filter of slot m's rows, seed and stream holding a copy of its state"""
        g = ob.Filter(self.model_id, self.raws[m], self.N, seg=self.seg, seed=self.seed, stream=int(self.streams[m]), systematic=self.systematic)
        g.copy_state_from(self.f[m])
        return g

    def _sync_t(self):
        """ONE time index per handle (smc_filter_s::t): every filter takes it, whatever its state's source carried"""
        for m, f in enumerate(self.f):
            if self.ft[m] != self.t:
                b = f.export_state()
                b[_t_word(f)] = self.t
                f.import_state(b)
                self.ft[m] = self.t

    def _need_init(self, who):
        if not self.inited:
            _refuse_ref(ESTATE, who + ": filter not initialised")

    # -- setters: each drops a pending window
    def set_params(self, raws):
        self.win = None
        self.raws = np.array(raws, dtype=np.float64).reshape(self.n_theta, -1)
        OracleHandle.set_params(self, self.raws)
        self.have_params = True

    def set_streams(self, streams):
        s = np.ascontiguousarray(streams, dtype=np.uint32)
        if self._streams_set is not None and np.array_equal(self._streams_set, s):
            return                       # (as _lib.Handle.set_streams: unchanged ids are not handed to the library, so nothing
                                         # is dropped; Model keeps such a call out of the vocabulary)
        self.win = None
        self.streams = self._streams_set = s.copy()
        for m, f in enumerate(self.f):
            f.set_rng(self.seed, int(s[m]))

    def reseed(self, seed):
        self.win = None
        self.seed = int(seed)
        for m, f in enumerate(self.f):
            f.set_rng(self.seed, int(self.streams[m]))

    # -- the steps
    def init(self, y1):
        if not self.have_params:
            _refuse_ref(ESTATE, "smc_init: smc_set_params has not been called")
        self.win = None
        lm = OracleHandle.init(self, float(y1))
        self.z = lm.copy()
        self.inited, self.t, self.ft = True, 1, [1] * self.n_theta
        return lm

    def step(self, y):
        self._need_init("smc_step")
        self.win = None
        lm, es = OracleHandle.step(self, float(y))
        self.z = self.z + lm
        self.t += 1
        self.ft = [self.t] * self.n_theta
        return lm, es

    def log_likelihood(self, y, trace=False):
        if not self.have_params:
            _refuse_ref(ESTATE, "smc_log_likelihood: smc_set_params has not been called")
        self.win = None
        y = np.ascontiguousarray(y, dtype=np.float64)
        if self.skip is not None and np.any(self.skip):
            return self._log_likelihood_skip(y, trace)
        r = [f.log_likelihood(y, trace=True) for f in self.f]
        self.z = np.array([a for a, _, _ in r])
        self.inited, self.t, self.ft = True, y.size, [y.size] * self.n_theta
        if trace:
            return self.z.copy(), np.stack([b for _, b, _ in r], axis=1), np.stack([c for _, _, c in r], axis=1)
        return self.z.copy()

    def set_skip(self, skip):
        self.skip = None if skip is None else np.array(skip, dtype=np.uint8)

    def _log_likelihood_skip(self, y, trace):
        """a skipped filter reads logZ = -inf and NaN in its trace columns and keeps x, w and raw weights; the handle's time index
        moves on for it too (include/smc_hip.h, smc_set_skip)"""
        self._need_init("smc_log_likelihood with a skip mask (the skipped filters keep a state)")
        lm, es = np.full((y.size, self.n_theta), np.nan), np.full((y.size, self.n_theta), np.nan)
        for m, f in enumerate(self.f):
            if self.skip[m]:
                self.z[m] = -np.inf
                continue
            self.z[m], lm[:, m], es[:, m] = f.log_likelihood(y, trace=True)
            self.ft[m] = y.size
        self.t = y.size
        self._sync_t()
        return (self.z.copy(), lm, es) if trace else self.z.copy()

    # -- the window: the filters stay where they stand until the commit
    def step_window(self, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        self._need_init("smc_step_window")
        if y.size < 1 or y.size > WIN_MAX:
            _refuse_ref(EINVAL, "smc_step_window: 1 <= k <= 64")
        if self.f[0].nseg != 1:
            _refuse_ref(EINVAL, "smc_step_window: needs filters that fit the LDS-resident kernel (one segment); use smc_step")
        ahead = [self._twin(m) for m in range(self.n_theta)]
        lm, es = np.zeros((y.size, self.n_theta)), np.zeros((y.size, self.n_theta))
        self._clouds = []
        for t, v in enumerate(y):
            for m, g in enumerate(ahead):
                lm[t, m], es[t, m] = g.step(float(v))
            if self._summ:
                s = [g.state() for g in ahead]
                self._clouds.append((np.stack([q[0] for q in s], axis=1), np.stack([q[1] for q in s])))
        self.win = (y, ahead, lm)
        return lm, es

    def step_commit(self, j):
        if self.win is None:
            _refuse_ref(ESTATE, "smc_step_commit: no window pending (smc_step_window)")
        y, ahead, lm = self.win
        if j < 0 or j > y.size:
            _refuse_ref(EINVAL, "smc_step_commit: 0 <= j <= steps of the window")
        self.win = None
        if j == 0:
            return
        if j == y.size:
            for f, g in zip(self.f, ahead):
                f.copy_state_from(g)
        else:
            for v in y[:j]:
                for f in self.f:
                    f.step(float(v))
        for t in range(j):
            self.z = self.z + lm[t]
        self.t += int(j)
        self.ft = [self.t] * self.n_theta

    # -- slot moves
    def permute(self, a):
        self._need_init("smc_permute")
        a = [int(v) for v in a]
        if any(v < 0 or v >= self.n_theta for v in a):
            _refuse_ref(EINVAL, "smc_permute: index out of range")
        self.win = None
        OracleHandle.permute(self, a)
        self.z = self.z[a]
        self.ft = [self.ft[v] for v in a]
        self._sync_t()

    def copy_from(self, src, mask):
        if src is self:
            _refuse_ref(EINVAL, "smc_copy_from: dst and src are the same handle")
        if not self.inited or not src.inited:
            _refuse_ref(ESTATE, "smc_copy_from: filter not initialised")
        if (self.model_id, self.N, self.seg, self.n_theta) != (src.model_id, src.N, src.seg, src.n_theta):
            _refuse_ref(EINVAL, "smc_copy_from: handles differ in model, geometry or device")
        self.win = None
        OracleHandle.copy_from(self, src, mask)
        for m in range(self.n_theta):
            if mask[m]:
                self.z[m] = src.z[m]
                self.ft[m] = src.ft[m]
        self.t = src.t                   # the destination takes the source's time index, whatever the mask (include/smc_hip.h)
        self._sync_t()

    def slot_bytes(self):
        return 8 * int(ob.lib().orc_filter_state_words(self.f[0]._h))

    def pack_slots(self, idx, buf):
        self._need_init("smc_pack/unpack_slots")
        idx = [int(v) for v in idx]
        if any(v < 0 or v >= self.n_theta for v in idx):
            _refuse_ref(EINVAL, "smc_pack/unpack_slots: index out of range")
        buf[:] = [(self.f[v].export_state(), self.z[v]) for v in idx]

    def unpack_slots(self, idx, buf):
        self._need_init("smc_pack/unpack_slots")
        idx = [int(v) for v in idx]
        if any(v < 0 or v >= self.n_theta for v in idx):
            _refuse_ref(EINVAL, "smc_pack/unpack_slots: index out of range")
        self.win = None
        for k, v in enumerate(idx):
            self.f[v].import_state(buf[k][0])
            self.z[v] = buf[k][1]
            self.ft[v] = int(buf[k][0][_t_word(self.f[v])])
        self._sync_t()                   # a packed slot carries no time index: the receiver's holds

    # -- readers
    def state(self, want_w=True, want_anc=None):
        self._need_init("smc_get_state")
        xs = [f.state() for f in self.f]
        return (np.stack([x[0] for x in xs], axis=1), np.stack([x[1] for x in xs]),
                np.stack([x[2] for x in xs]).astype(np.int32))

    def weights_raw(self):
        self._need_init("smc_get_weights_raw")
        r = [f.weights_raw() for f in self.f]
        return tuple(np.stack([q[k] for q in r]) for k in range(5))

    def logZ(self):
        self._need_init("smc_get_logZ")
        return self.z.copy(), np.array([f.ess() for f in self.f])

    def moments(self):
        self._need_init("smc_get_moments")
        return OracleHandle.moments(self)

    def quantiles(self, p, component=0):
        self._need_init("smc_get_quantiles")
        return OracleHandle.quantiles(self, p, component)

    def get_summaries(self, T):
        """the clouds (x, w) after each of the first T steps of the last window: what summ_diff checks the library's rows against"""
        if not self._summ or T < 1 or T > len(self._clouds):
            _refuse_ref(ESTATE, "smc_get_summaries: more steps than the last multi-step call recorded")
        return self._clouds[:T]

    # (no cheap stateful reference: checked for "changes nothing" only)
    def forecast(self, H, seed, p=None, component=0, obs=True):
        self._need_init("smc_forecast")

    def forecast_cloud(self, H, seed, want_y=True):
        self._need_init("smc_forecast_cloud")

    def predictive(self, y_t):
        self._need_init("smc_get_predictive")

    def launch_geometry(self):
        return None

    @property
    def step_by_value(self):
        return None


def reference_pair(profile, model, seed0=21, cls=None):
    """(make, alloc) for replay over reference handles of a profile"""
    cls = cls or ReferenceHandle

    def make(which, seed):
        n = profile["n"] + (1 if which == 2 else 0)
        return cls(model, profile["n_theta"], n, profile["seg"], seed, profile["systematic"])

    def alloc(h, k):
        return [None] * k

    return make, alloc


def reference_results(profile, model, ops, cls=None, prefix=None):
    """replay ops over two fresh reference handles -> the list of results"""
    make, alloc = reference_pair(profile, model, cls=cls)
    out = []
    replay(make(0, 21), make(1, 31), ops, lambda i, op, r: out.append(r), make=make, alloc=alloc, prefix=prefix, model=model)
    return out
