"""CPU tests (no GPU) of tests/handle_sequences.py: the generated call sequences are legal under the contract's model, the
committed seed list of every profile covers the whole table of (op that drops or moves something -> next consuming op), the
reference handle is pinned by straight-line oracle filters and not by itself, and the sequences can tell a list of deliberately
wrong reference handles from the right one.  No wrong code runs on a GPU: the GPU test compares the library with ReferenceHandle."""
import numpy as np
import pytest

import handle_sequences as hs

PROFILE_NAMES = sorted(hs.PROFILES)


# ---- legality ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PROFILE_NAMES)
def test_sequences_are_legal_and_deterministic(name):
    p = hs.PROFILES[name]
    for model in p["models"]:
        for seed in hs.SEEDS:
            ops = hs.sequence(p, seed, model=model)
            assert ops == hs.sequence(name, seed, model=model) and 8 <= len(ops) <= hs.LENGTH
            st = [hs.Model(p), hs.Model(p)]
            for i, op in enumerate(ops):
                assert isinstance(op, tuple) and eval(repr(op)) == op, (i, op)       # plain data: pastes back
                assert hs.legal(st, op), (name, model, seed, i, op)
                hs.apply(st, op)
                if not p["windows"]:
                    assert not st[0].win_k and not st[1].win_k


def test_model_states_the_window_contract():
    """the legality model IS the contract of include/smc_hip.h: which ops drop a pending window, which keep it"""
    p = hs.PROFILES["batch-res"]
    nth = p["n_theta"]

    def pending():
        st = [hs.Model(p), hs.Model(p)]
        for op in (("set_params", 0, 1), ("init", 0, 0.1), ("set_params", 1, 2), ("init", 1, 0.2), ("step_window", 0, [0.1, 0.2, 0.3])):
            hs.apply(st, op)
        return st

    drop = [("set_params", 0, 3), ("set_streams", 0, [5, 6, 7]), ("reseed", 0, 9), ("init", 0, 0.0), ("step", 0, 0.0),
            ("log_likelihood", 0, [0.0, 0.1], False), ("permute", 0, [0] * nth), ("copy_from", 0, [1] * nth),
            ("pack_unpack", 1, [0], 0, [1]), ("step_commit", 0, 1), ("recreate", 0, 3, 4, 0.0)]
    keep = [("read", 0, k) for k in hs.READERS] + [("refuse", 0, k) for k in hs.KEPT_REFUSALS]
    keep += [("copy_from", 1, [1] * nth), ("pack_unpack", 0, [0], 1, [1])]          # the handle as the SOURCE only reads
    for op in drop:
        st = pending()
        assert hs.apply(st, op) == 0 and st[0].win_k == 0, op
        assert hs.outcome(st, ("step_commit", 0, 1)) == hs.ESTATE
    for op in keep:
        st = pending()
        rc = hs.apply(st, op)
        assert st[0].win_k == 3 and (rc != 0) == (op[0] == "refuse"), op
        assert hs.outcome(st, ("step_commit", 0, 2)) == 0
    st = pending()
    hs.apply(st, ("step_window", 0, [0.5, 0.6]))                                      # a second window replaces the first
    assert st[0].win_k == 2
    # the ids of the last set_streams again: _lib.Handle.set_streams hands nothing to the library, so nothing is dropped - the
    # model keeps such a call out of the vocabulary (the legality test shows that the generator never emits one)
    st = pending()
    hs.apply(st, ("set_streams", 0, [5, 6, 7]))
    assert not hs.legal(st, ("set_streams", 0, [5, 6, 7])) and hs.legal(st, ("set_streams", 0, [5, 6, 8]))
    hs.apply(st, ("recreate", 0, 3, 4, 0.0))
    assert hs.legal(st, ("set_streams", 0, [5, 6, 7]))                                # a new handle has set none yet


# ---- coverage: a condition, not a measurement --------------------------------------------------------------------------------------
def test_table_is_the_one_written_here():
    """the table: each mutator followed by each consuming op, each setter between step_window and step_commit for each j class,
    each reader and refused call inside a window (profiles without windows: without the window ops)"""
    mut = ["set_params", "set_streams", "reseed", "init", "step", "log_likelihood", "step_window", "step_commit", "permute",
           "copy_from", "pack_unpack", "recreate"]
    con = ["step", "step_window", "step_commit", "log_likelihood", "permute", "copy_from"]
    full = {("pair", a, b) for a in mut for b in con}
    full |= {("win", s, j) for s in ("set_params", "set_streams", "reseed") for j in ("zero", "mid", "all")}
    full |= {("keep", k) for k in hs.READERS + hs.KEPT_REFUSALS + ("copy_source",)}     # (copy_source: copy_from with this handle as the source)
    assert set(hs.pair_table(hs.PROFILES["batch-res"])) == full and len(full) == 72 + 9 + 22
    nowin = {i for i in full if i[0] == "pair" and "step_window" not in i and "step_commit" not in i}
    assert set(hs.pair_table(hs.PROFILES["batch-multi"])) == nowin and len(nowin) == 40


@pytest.mark.parametrize("name", PROFILE_NAMES)
def test_seed_list_covers_the_table(name):
    p = hs.PROFILES[name]
    table = set(hs.pair_table(p))
    for model in p["models"]:
        got = set()
        for seed in hs.SEEDS:
            got |= hs.covered(p, hs.sequence(p, seed, model=model))
        assert not table - got, (name, model, sorted(table - got))
    if p["windows"]:          # every refused call of the vocabulary occurs somewhere, window_multi and commit_none included elsewhere
        assert {"commit_over", "permute_oob"} <= {i[1] for i in table if i[0] == "keep"}


def test_every_refused_call_and_reader_occurs():
    seen = set()
    for name in PROFILE_NAMES:
        p = hs.PROFILES[name]
        for seed in hs.SEEDS:
            seen |= {op[2] for op in hs.sequence(p, seed) if op[0] in ("read", "refuse")}
    assert seen == set(hs.READERS) | set(hs.REFUSED)


# ---- the reference is pinned by the oracle -------------------------------------------------------------------------------------------
SLOT_MOVES = ("permute", "copy_from", "pack_unpack", "recreate")


def straight_line(ob, p, model, ops):
    """one ob.Filter per slot of each handle, driven in a straight line by the ops (no slot moves among them) under the contract's
    model: -> per op the (ret, x, w, raw weights, logZ, ess) of the handle the op concerns"""
    nth = p["n_theta"]
    blank = hs.ReferenceHandle._blank_raw(model)
    F = [[ob.Filter(model, blank, p["n"], seg=p["seg"], seed=s, stream=m, systematic=p["systematic"]) for m in range(nth)] for s in (21, 31)]
    seeds, streams = [21, 31], [list(range(nth)), list(range(nth))]
    Z = [np.zeros(nth), np.zeros(nth)]
    win = [None, None]
    st = [hs.Model(p), hs.Model(p)]
    out = []
    for op in ops:
        name, tgt = op[0], op[1]
        rc = hs.apply(st, op)
        f, ret = F[tgt], None
        if rc == 0:
            if name == "set_params":
                for m, r in enumerate(hs.rows(model, nth, op[2])):
                    f[m].set_params(r)
            elif name == "set_streams":
                streams[tgt] = op[2]
            elif name == "reseed":
                seeds[tgt] = op[2]
            if name in ("set_streams", "reseed"):
                for m in range(nth):
                    f[m].set_rng(seeds[tgt], streams[tgt][m])
            if name == "init":
                ret = (np.array([g.bootstrap_filter(op[2]) for g in f]),)
                Z[tgt] = ret[0].copy()
            elif name == "step":
                r = [g.step(op[2]) for g in f]
                ret = (np.array([a for a, _ in r]), np.array([b for _, b in r]))
                Z[tgt] = Z[tgt] + ret[0]
            elif name == "log_likelihood":
                r = [g.log_likelihood(np.array(op[2]), trace=True) for g in f]
                Z[tgt] = np.array([a for a, _, _ in r])
                ret = (Z[tgt],) + ((np.stack([b for _, b, _ in r], 1), np.stack([c for _, _, c in r], 1)) if op[3] else ())
            elif name == "step_window":
                win[tgt] = op[2]                       # k steps ahead: the straight line takes them at the commit
            elif name == "step_commit":
                for v in win[tgt][:op[2]]:
                    Z[tgt] = Z[tgt] + np.array([g.step(v)[0] for g in f])
            if name != "step_window" and name not in ("read", "refuse"):
                win[tgt] = None
        s = [g.state() for g in f]
        raw = [g.weights_raw() for g in f]
        snap = dict(x=np.stack([q[0] for q in s], 1), w=np.stack([q[1] for q in s]), logZ=Z[tgt].copy(), ess=np.array([g.ess() for g in f]))
        for k, key in enumerate(("C", "m", "S", "S2hi", "S2lo")):
            snap[key] = np.stack([q[k] for q in raw])
        out.append((rc, ret, snap))
    return out


def st_inited(ops, tgt, p):
    st = [hs.Model(p), hs.Model(p)]
    for op in ops:
        hs.apply(st, op)
    return st[tgt].inited


@pytest.mark.parametrize("name", PROFILE_NAMES)
def test_reference_equals_straight_line_oracle_filters(ob, name):
    p = hs.PROFILES[name]
    model = p["models"][-1]
    for seed in hs.SEEDS[:3]:
        ops, st = [], [hs.Model(p), hs.Model(p)]
        for op in hs.sequence(p, seed, model=model):   # without the slot moves, and without what is no longer legal without them
            op = op[:4] if op[0] == "log_likelihood" else op       # (without skip masks: a skipped filter's time index moves on)
            if op[0] not in SLOT_MOVES and not (op[0] == "refuse" and op[2] in ("unpack_oob", "copy_other_n")) and hs.legal(st, op):
                ops.append(op)
                hs.apply(st, op)
        ref = hs.reference_results(p, model, ops)
        line = straight_line(ob, p, model, ops)
        assert len(ref) == len(line) == len(ops)
        windows = 0
        for i, (r, (rc, ret, snap)) in enumerate(zip(ref, line)):
            where = (name, seed, i, ops[:i + 1])
            assert (r["err"] or 0) == rc, where
            if ops[i][0] == "step_window" and rc == 0:
                windows += 1                           # the window's rows are checked through the commit's logZ and state
            elif ret is not None:
                assert all(hs.same(u, v) for u, v in zip(r["ret"], ret)) and len(r["ret"]) == len(ret), where
            if r["snap"] is None:                      # before the first init there is nothing to read
                assert not st_inited(ops[:i + 1], ops[i][1], p), where
                continue
            assert not hs.snap_diff(r["snap"], snap), (hs.snap_diff(r["snap"], snap), where)
            assert r["unchanged"] in (None, True), where
        assert windows or not p["windows"]


@pytest.mark.parametrize("name", PROFILE_NAMES)
def test_reference_follows_the_model(ob, name):
    """on every sequence of the seed list the reference refuses exactly where the contract's model says, with its code, and a
    reader or a refused call leaves its snapshot as it was"""
    p = hs.PROFILES[name]
    for seed in hs.SEEDS:
        ops, ref = _reference(name, seed)
        st = [hs.Model(p), hs.Model(p)]
        for i, (op, r) in enumerate(zip(ops, ref)):
            assert (r["err"] or 0) == hs.apply(st, op), (name, seed, i, ops[:i + 1])
            assert r["unchanged"] in (None, True) and r["anc_kept"] in (None, True), (name, seed, i, ops[:i + 1])
            if op[0] == "copy_from" and r["err"] is None:
                assert r["unchanged"] is True          # (the source of a copy is looked at as well)


def test_reference_has_one_time_index_per_handle(ob):
    """a value copy brings its source's time index along (orc_filter_copy_state); the handle's own holds for every filter, as
    smc_filter_s::t does: after a masked copy from a handle further on, and after an unpack, every oracle filter carries it"""
    p = hs.PROFILES["batch-multi"]
    make, alloc = hs.reference_pair(p, 1)
    a, b = make(0, 21), make(1, 31)
    for h, steps in ((a, 1), (b, 4)):
        h.set_params(hs.rows(1, 3, 1))
        h.init(0.3)
        for _ in range(steps):
            h.step(0.1)

    def carried(h):
        return [int(f.export_state()[hs._t_word(f)]) for f in h.f]

    assert carried(a) == [2] * 3 and carried(b) == [5] * 3
    a.copy_from(b, [0, 1, 0])
    assert a.t == 5 and carried(a) == [5] * 3
    buf = alloc(a, 1)
    a.pack_slots([2], buf)
    b.step(0.2)
    b.unpack_slots([0], buf)
    assert b.t == 6 and carried(b) == [6] * 3
    g = ob.Filter(1, hs.rows(1, 3, 1)[1], p["n"], seg=p["seg"], seed=31, stream=1)          # slot 1 of b, never touched by a copy
    g.bootstrap_filter(0.3)
    for v in (0.1, 0.1, 0.1, 0.1, 0.2):
        g.step(v)
    assert hs.same(g.state()[0], b.f[1].state()[0])


def test_skip_masks_and_window_summaries_occur():
    for name in PROFILE_NAMES:
        p = hs.PROFILES[name]
        ops = [op for seed in hs.SEEDS for op in hs.sequence(p, seed)]
        masks = [op[4] for op in ops if op[0] == "log_likelihood" and len(op) > 4]
        assert masks and all(len(m) == p["n_theta"] for m in masks), name
        if p["n_theta"] > 1:
            assert any(0 < sum(m) < len(m) for m in masks) and any(sum(m) == len(m) for m in masks), name
        summ = [op for op in ops if op[0] == "step_window" and len(op) > 3]
        assert bool(summ) == (p["windows"] and not p["systematic"]), name


def test_reference_skip_mask(ob):
    """a skipped filter of the reference: logZ = -inf, NaN trace columns, x, w and raw weights as before; the others as without
    the mask; the mask is gone after set_skip(None)"""
    p = hs.PROFILES["batch-multi"]
    make, _ = hs.reference_pair(p, 1)
    a, b = make(0, 21), make(0, 21)
    y = [0.2, -0.1, 0.4]
    for h in (a, b):
        h.set_params(hs.rows(1, 3, 1))
        h.init(0.3)
    before = hs.snapshot(a)[0]
    a.set_skip([0, 1, 0])
    z, lm, es = a.log_likelihood(y, trace=True)
    a.set_skip(None)
    zb, lmb, esb = b.log_likelihood(y, trace=True)
    after = hs.snapshot(a)[0]
    assert z[1] == -np.inf and np.all(np.isnan(lm[:, 1])) and np.all(np.isnan(es[:, 1])) and a.t == 3
    assert hs.same(z[[0, 2]], zb[[0, 2]]) and hs.same(lm[:, [0, 2]], lmb[:, [0, 2]]) and hs.same(es[:, [0, 2]], esb[:, [0, 2]])
    for k in ("x", "w", "C", "m", "S", "S2hi", "S2lo", "ess"):
        sl = (slice(None), 1) if k == "x" else 1
        assert hs.same(after[k][sl], before[k][sl]), k
    assert hs.same(a.log_likelihood(y), zb)


def test_summary_check_accepts_the_oracle_and_rejects_an_offset(ob):
    """summ_diff: the oracle's own moments and quantiles of the clouds a reference window hands over pass the bounds of
    tests/summary_reference.py; a mean off by 1e-9 relative, or a quantile one particle off, does not"""
    p = hs.PROFILES["batch-res"]
    make, _ = hs.reference_pair(p, 1)
    a = make(0, 21)
    a.set_params(hs.rows(1, 3, 1))
    a.init(0.3)
    a.set_summaries(hs.SUMM_P, 0, True)
    a.step_window([0.1, -0.4, 0.9])
    clouds = a.get_summaries(3)
    ahead = [a._twin(m) for m in range(3)]
    q, mean, var = np.zeros((3, 3, 3)), np.zeros((3, 1, 3)), np.zeros((3, 1, 3))
    for t, v in enumerate([0.1, -0.4, 0.9]):
        for m, g in enumerate(ahead):
            g.step(v)
            q[t, m] = g.quantiles(hs.SUMM_P)
            mean[t, :, m], var[t, :, m] = g.moments()
    assert hs.summ_diff(clouds, (q, mean, var)) == [] and hs.summ_diff((q, mean, var), clouds) == []
    assert hs.summ_diff(clouds, clouds) == [] and hs.summ_diff(clouds, clouds[:2]) == ["summ"]
    bad = mean.copy()
    bad[1, 0, 2] *= 1 + 1e-9
    assert hs.summ_diff(clouds, (q, bad, var))
    x, w = clouds[2]
    bad = q.copy()
    bad[2, 0, 1] = np.sort(x[0, 0])[np.searchsorted(np.sort(x[0, 0]), q[2, 0, 1]) + 40]
    assert hs.summ_diff(clouds, (bad, mean, var))


def test_window_rows_equal_single_steps(ob):
    """the [k][n_theta] rows a reference window reports are those of k single steps, and the filters have not moved"""
    p = hs.PROFILES["batch-res"]
    make, _ = hs.reference_pair(p, 2)
    a, b = make(0, 21), make(0, 21)
    for h in (a, b):
        h.set_params(hs.rows(2, 3, 1))
        h.init(0.3)
    before = hs.snapshot(a)[0]
    y = [0.1, -0.4, 0.9, 0.2]
    lm, es = a.step_window(y)
    assert not hs.snap_diff(before, hs.snapshot(a)[0])
    for t, v in enumerate(y):
        l1, e1 = b.step(v)
        assert hs.same(lm[t], l1) and hs.same(es[t], e1)
    a.step_commit(4)
    assert not hs.snap_diff(hs.snapshot(a)[0], hs.snapshot(b)[0])


# ---- sensitivity: deliberately wrong reference handles ---------------------------------------------------------------------------------
class LateReseed(hs.ReferenceHandle):
    """reseed takes effect one launch late"""
    _late = None

    def reseed(self, seed):
        self.win = None
        self._late = seed

    def _flush(self):
        if self._late is not None:
            hs.ReferenceHandle.reseed(self, self._late)
            self._late = None

    def init(self, y1):
        r = hs.ReferenceHandle.init(self, y1)
        self._flush()
        return r

    def step(self, y):
        r = hs.ReferenceHandle.step(self, y)
        self._flush()
        return r

    def step_window(self, y):
        r = hs.ReferenceHandle.step_window(self, y)
        w = self.win
        self._flush()
        self.win = w
        return r

    def log_likelihood(self, y, trace=False):
        r = hs.ReferenceHandle.log_likelihood(self, y, trace)
        self._flush()
        return r


class StreamsIgnoredSlot0(hs.ReferenceHandle):
    """set_streams ignored for slot 0 (a stale by-value copy of the stream id)"""

    def set_streams(self, streams):
        s = np.array(streams, dtype=np.uint32)
        s[0] = self.streams[0]
        hs.ReferenceHandle.set_streams(self, s)


class CommitKeepsAll(hs.ReferenceHandle):
    """commit(j < k) keeps the end state of all k steps"""

    def step_commit(self, j):
        if self.win is not None and 0 < j < self.win[0].size:
            y, ahead, lm = self.win
            hs.ReferenceHandle.step_commit(self, j)
            for f, g in zip(self.f, ahead):
                f.copy_state_from(g)
            self.ft = [y.size + self.t - j] * self.n_theta
            self._sync_t()
            return
        hs.ReferenceHandle.step_commit(self, j)


class PermuteForgetsRecords(hs.ReferenceHandle):
    """permute forgets the segment records (m, S, S2hi, S2lo) of slot 0"""

    def permute(self, a):
        old = self.f[0].export_state() if self.inited else None
        hs.ReferenceHandle.permute(self, a)
        ns = self.f[0].nseg
        o = self.d * self.N + 2 * self.N + ns * self.f[0].seg
        new = self.f[0].export_state()
        new[o:o + 4 * ns] = old[o:o + 4 * ns]
        self.f[0].import_state(new)


class CopyIgnoresMask(hs.ReferenceHandle):
    def copy_from(self, src, mask):
        hs.ReferenceHandle.copy_from(self, src, np.ones(self.n_theta, dtype=np.uint8))


class SetterKeepsWindow(hs.ReferenceHandle):
    """smc_set_params as it was: a pending window stands"""

    def set_params(self, raws):
        w = self.win
        hs.ReferenceHandle.set_params(self, raws)
        self.win = w


class RefusedPermuteDropsWindow(hs.ReferenceHandle):
    """smc_permute as it was: the window goes before the indices are looked at"""

    def permute(self, a):
        if self.inited and any(int(v) < 0 or int(v) >= self.n_theta for v in a):
            self.win = None
        hs.ReferenceHandle.permute(self, a)


class RecreateKeepsT(hs.ReferenceHandle):
    """a handle on a recycled bundle that goes on with the time index of the handle before it"""
    stale = None

    def close(self):
        RecreateKeepsT.stale = self.t
        hs.ReferenceHandle.close(self)

    def init(self, y1):
        r = hs.ReferenceHandle.init(self, y1)
        if RecreateKeepsT.stale is not None:
            self.t, RecreateKeepsT.stale = RecreateKeepsT.stale, None
            self._sync_t()
        return r


WRONG = [(LateReseed, False), (StreamsIgnoredSlot0, False), (CommitKeepsAll, True), (PermuteForgetsRecords, False), (CopyIgnoresMask, False),
         (SetterKeepsWindow, True), (RefusedPermuteDropsWindow, True), (RecreateKeepsT, False)]     # (class, needs windows)

_ref_cache = {}


def _reference(name, seed):
    if (name, seed) not in _ref_cache:
        p = hs.PROFILES[name]
        ops = hs.sequence(p, seed, model=p["models"][0])
        _ref_cache[name, seed] = (ops, hs.reference_results(p, p["models"][0], ops))
    return _ref_cache[name, seed]


@pytest.mark.parametrize("cls,needs_windows", WRONG, ids=[c.__name__ for c, _ in WRONG])
def test_sequences_tell_a_wrong_handle_apart(ob, cls, needs_windows):
    """each wrong handle differs from ReferenceHandle in a compared quantity on a seed of every profile whose vocabulary has the op
    (the only permutation of a one-filter profile is the identity, which moves no records; a profile without windows has no
    window.  A one-filter profile does have masks: a copy under the mask [0] must leave its filter alone)"""
    for name in PROFILE_NAMES:
        p = hs.PROFILES[name]
        if needs_windows and not p["windows"]:
            continue
        if cls is PermuteForgetsRecords and p["n_theta"] == 1:
            continue
        RecreateKeepsT.stale = None
        found = None
        for seed in hs.SEEDS:
            ops, ref = _reference(name, seed)
            got = hs.reference_results(p, p["models"][0], ops, cls=cls)
            d = [(i, hs.result_diff(r, g)) for i, (r, g) in enumerate(zip(ref, got)) if hs.result_diff(r, g)]
            if d:
                found = (seed, d[0])
                break
        assert found, (cls.__name__, name)
