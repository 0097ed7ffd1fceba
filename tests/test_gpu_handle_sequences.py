"""GPU tests (pytest -m gpu): random call sequences on a filter handle (tests/handle_sequences.py) replayed on the library and
compared after EVERY op with the stateful CPU reference (ReferenceHandle over oracle filters), bit for bit: the values each call
returns (logmu, ess, logZ, the traces, the window's [k][n_theta] rows), the error codes, and the snapshot of the handle the op
concerns - state() x and w, weights_raw() C, m, S, S2hi, S2lo, logZ() - with the ancestors after init / step / log_likelihood
only (they belong to the last launch).  After a reader or a refused call the snapshot must equal the one before, and a pending
window must still be pending (the sequences commit it next).  A failure names profile, model, seed, op index and the ops up to
there: `replay(..., prefix=i + 1)` reproduces it.

Two scripted regressions keep the two findings named that the sequences were written for: a setter between step_window and
step_commit drops the window (the commit is SMC_ESTATE), and a refused call leaves a pending window standing."""
import numpy as np
import pytest

import handle_sequences as hs
from test_gpu_step_early_args import pointer_handle

pytestmark = pytest.mark.gpu

CASES = [(name, model, seed) for name in sorted(hs.PROFILES) for model in hs.PROFILES[name]["models"] for seed in hs.SEEDS]


def gpu_pair(L, p, model):
    """(make, alloc) for replay over library handles of a profile; flags always include SMC_FLAG_ANCESTORS"""
    torch = pytest.importorskip("torch")
    flags = L.FLAG_ANCESTORS | (L.FLAG_SYSTEMATIC if p["systematic"] else 0) | (L.FLAG_NO_RESIDENT if p["no_resident"] else 0)

    def make(which, seed):
        n = p["n"] + (1 if which == 2 else 0)
        if p["pointer"]:
            return pointer_handle(L, model, p["n_theta"], n, seg=p["seg"], seed=seed, flags=flags)
        return L.Handle(model, p["n_theta"], n, seg=p["seg"], seed=seed, flags=flags)

    def alloc(h, k):
        return torch.empty((k, h.slot_bytes() // 8), dtype=torch.int64, device="cuda")

    return make, alloc


def run_case(L, p, model, ops, label):
    """replay ops on the reference (CPU), then on the library, comparing after every op"""
    ref = hs.reference_results(p, model, ops)
    st = [hs.Model(p), hs.Model(p)]
    make, alloc = gpu_pair(L, p, model)

    def check(i, op, r):
        where = "%s: op %d of %r" % (label, i, list(ops[:i + 1]))
        want = hs.apply(st, op)
        assert (r["err"] or 0) == want, "error code %r, the contract says %r; %s" % (r["err"], want, where)
        assert r["unchanged"] in (None, True), "a reader, a refused call or a slot move changed the handle it only reads; %s" % where
        assert r["anc_kept"] in (None, True), "a skipped filter lost the ancestors it had before the call; %s" % where
        d = hs.result_diff(ref[i], r)
        assert not d, "differs from the reference in %s; %s" % (d, where)

    a, b = make(0, 21), make(1, 31)
    assert (a.nseg == 1) == p["windows"] and a.resident == (p["windows"] and not p["no_resident"])
    H = [a, b]
    try:
        H = hs.replay(a, b, ops, check, make=make, alloc=alloc, model=model)
    finally:
        for h in H:
            h.close()


@pytest.mark.parametrize("name,model,seed", CASES, ids=["%s-m%d-s%d" % c for c in CASES])
def test_random_sequence_equals_reference(L, ob, name, model, seed):
    p = hs.PROFILES[name]
    run_case(L, p, model, hs.sequence(p, seed, model=model), "profile %s, model %d, seed %d" % (name, model, seed))


def test_time_step_kernel_drops_the_window(L, ob):
    """smc_time_step_kernel runs a series of its own over the filters and the window's observations: a pending window is gone
    after it (step_commit: SMC_ESTATE), and the handle goes on from the series it ran"""
    p = hs.PROFILES["batch-res"]
    make, _ = gpu_pair(L, p, 1)
    h = make(0, 21)
    try:
        h.set_params(hs.rows(1, p["n_theta"], 1))
        h.init(0.4)
        h.step_window(np.array(Y4))
        h.time_step_kernel(np.array([0.4, -0.2, 0.6, 0.1, 0.3]), nsample=2)
        with pytest.raises(L.SmcError) as e:
            h.step_commit(2)
        assert hs.err_code(e.value) == hs.ESTATE
        before = hs.snapshot(h)[0]
        h.synchronize()
        assert not hs.snap_diff(before, hs.snapshot(h)[0])
        h.step(0.6)
    finally:
        h.close()


# ---- the two findings, scripted ---------------------------------------------------------------------------------------------------
Y4 = [0.31, -0.52, 0.87, -0.11]
START = [("set_params", 0, 1), ("init", 0, 0.4), ("step", 0, -0.2), ("set_params", 1, 2), ("init", 1, 0.1)]
SETTER_OPS = {"set_params": ("set_params", 0, 5), "set_streams": ("set_streams", 0, [9, 4, 7]), "reseed": ("reseed", 0, 4242)}


@pytest.mark.parametrize("name", ["batch-res", "one-res"])
@pytest.mark.parametrize("j", [0, 1, 4])
@pytest.mark.parametrize("setter", sorted(SETTER_OPS))
def test_setter_between_window_and_commit(L, ob, name, setter, j):
    """step_window(k = 4), a setter, step_commit(j): the commit is SMC_ESTATE ("no window pending"), the state is the one of
    before the window, and the following step equals the reference under the new rows / streams / seed"""
    p = hs.PROFILES[name]
    op = SETTER_OPS[setter]
    if setter == "set_streams":
        op = op[:2] + (op[2][:p["n_theta"]],)
    ops = START + [("read", 0, "state"), ("step_window", 0, Y4), op, ("step_commit", 0, j), ("step", 0, 0.6)]
    ref = hs.reference_results(p, 1, ops)
    assert ref[-2]["err"] == hs.ESTATE and ref[-2]["unchanged"]
    assert not hs.snap_diff(ref[5]["snap"], ref[-2]["snap"])                  # the state of before the window
    run_case(L, p, 1, ops, "setter %s, j %d on %s" % (setter, j, name))


@pytest.mark.parametrize("name", ["batch-res", "one-res"])
@pytest.mark.parametrize("kind", hs.KEPT_REFUSALS)
def test_refused_call_keeps_the_window(L, ob, name, kind):
    """step_window(k = 4), a refused call, step_commit(2): the refusal changes nothing and the commit gives the reference's state"""
    p = hs.PROFILES[name]
    ops = START + [("step_window", 0, Y4), ("refuse", 0, kind) + ((5,) if kind == "commit_over" else ()), ("step_commit", 0, 2), ("step", 0, 0.6)]
    ref = hs.reference_results(p, 1, ops)
    assert ref[-3]["err"] in (hs.EINVAL, hs.ESTATE) and ref[-2]["err"] is None
    run_case(L, p, 1, ops, "refused %s on %s" % (kind, name))
