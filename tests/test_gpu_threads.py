"""Host threads on the GPU (pytest -m gpu; DESIGN.md "Host threads"): one handle per thread equals the serial run, bit for bit.

Every other GPU test drives the library from one host thread.  Here 8 threads of one pool (tests/thread_pool.py) enter it
together, for 3 rounds, each on handles of its own:

  a. whole series on every launch path, with create / destroy churn (the bundle cache hands the slab, stream, events and
     pinned mirrors of a handle destroyed in one thread to a create in another)
  b. the step API with summaries in both modes read after every step (the summary scratch is allocated in the middle of the run)
  c. one handle that moves from thread to thread between calls
  d. the stand-alone entry points with their per-thread scratch, threads that end while others are launching, and new threads
  e. the Python layer: both smoothers, IBIS with device moves, density_tempered with the device PMMH

The property is that concurrency changes no bit, so every reference is the same call made serially by the main thread before
the pool starts, and every comparison is equality of IEEE bit patterns or integers.  The serial result is itself pinned: to the
CPU oracle or to tests/composed_reference.py where the case is small enough, else by the test named beside the case."""
import io
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import composed_reference as CR
from thread_pool import ROUNDS, WORKERS, assert_same, run_threads

pytestmark = pytest.mark.gpu

LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
SV = [-1.0, 0.95, 0.25]
UC = [0.2, 0.2, 3.0, 0.0, 0.0]
NO_RESIDENT, SYSTEMATIC = 2, 4
SIM = {1: (1, LG), 2: (2, SV), 3: (3, UC), 4: (3, UC)}      # the series of the marginal family is UCSV's


def rows_for(raw, nth):
    """a parameter row per filter: the first entry differs, so that a row read from another filter's slot shows"""
    r = np.tile(raw, (nth, 1)).astype(float)
    r[:, 0] *= 1.0 - 0.2 * np.arange(nth) / nth
    return r


def series(L, model, T, seed=1998):
    m, raw = SIM[model]
    return L.simulate(m, raw, T, seed)[1]


# ---- a. whole series, one handle per thread, create / destroy churn ---------------------------------------------------------
# name, model, n, seg, n_theta, T, flags, proposal, seed, what pins the serial bits
CASES = [
    ("resident LG", 1, 1024, 0, 3, 40, 0, 0, 11, "oracle"),
    ("resident ragged UCSV", 3, 1000, 0, 2, 15, 0, 0, 12, "oracle"),
    # (the same geometry as "guided LG OPTIMAL" under another seed: either takes the bundle the other gave back)
    ("no-resident SV", 2, 1024, 0, 1, 15, NO_RESIDENT, 0, 13, "oracle"),
    ("multi-segment LG", 1, 5000, 256, 1, 12, 0, 0, 14, "oracle"),                    # break points allocated in the run
    # more than 2^9 segments: k_table.  n > 5000: the serial run, whose bits
    # test_gpu_parity.py::test_global_segment_table_paths pins to the oracle at this shape
    ("global segment table LG", 1, 70000, 256, 2, 6, 0, 0, 15, "serial"),
    ("systematic LG", 1, 3000, 1024, 1, 10, SYSTEMATIC, 0, 16, "oracle"),
    ("guided LG OPTIMAL", 1, 1024, 0, 1, 15, 0, CR.OPTIMAL, 17, "composed"),
    ("marginal UCSV", 4, 3000, 256, 1, 8, 0, 0, 18, "composed"),
]
SERIES_NAMES = ("logZ", "logmu", "ess", "x", "w", "ancestors", "C", "m", "S", "S2hi", "S2lo")


def device_series(L, case, seed=None):
    """create, set the rows, one whole-series call with traces, read everything, destroy"""
    name, model, n, seg, nth, T, flags, prop, seed0, _ = case
    h = L.Handle(model, nth, n, seg=seg, seed=seed0 if seed is None else seed, flags=flags | L.FLAG_ANCESTORS)
    try:
        h.set_params(rows_for(SIM[model][1], nth))
        if prop:
            h.set_proposal(prop)
        _, lm, es = h.log_likelihood(series(L, model, T), trace=True)
        x, w, a = h.state()
        return (h.logZ()[0], lm, es, x, w, a.astype(np.int64)) + tuple(h.weights_raw())
    finally:
        h.close()


def pinned_series(L, ob, case):
    """the reference of a case in device_series' layout"""
    name, model, n, seg, nth, T, flags, prop, seed, pin = case
    raws, y = rows_for(SIM[model][1], nth), series(L, model, T)
    if pin == "serial":
        return device_series(L, case)
    if pin == "composed":
        r = CR.run_series(L, ob, model, raws, n, seg, seed, y, kind=prop, systematic=bool(flags & SYSTEMATIC))
        s = r["snap"]
        return (r["logZ"], r["lm"], r["es"], s[0], s[1], np.asarray(s[2], dtype=np.int64)) + tuple(s[3:])
    per = []
    for th in range(nth):
        f = ob.Filter(model, raws[th], n, seg=seg, seed=seed, stream=th, systematic=bool(flags & SYSTEMATIC))
        z, lm, es = f.log_likelihood(y, trace=True)
        x, w, a, _ = f.state()
        per.append((z, lm, es, x, w, a) + tuple(f.weights_raw()))
    col = lambda k: [p[k] for p in per]                                                # noqa: E731
    return (np.array(col(0)), np.stack(col(1), axis=1), np.stack(col(2), axis=1), np.stack(col(3), axis=1)) + \
        tuple(np.stack(col(k)) for k in range(4, 11))


def test_whole_series_one_handle_per_thread(L, ob):
    assert len(CASES) == WORKERS
    refs = [dict(zip(SERIES_NAMES, pinned_series(L, ob, c))) for c in CASES]
    for c, ref in zip(CASES, refs):                       # the serial device run equals its pin
        assert_same(dict(zip(SERIES_NAMES, device_series(L, c))), ref, c[0] + " (serial)")

    def work(k, r):
        i = (k + 3 * r) % WORKERS                          # the cases rotate over the threads between the rounds
        t0 = time.perf_counter()
        got = device_series(L, CASES[i])
        assert_same(dict(zip(SERIES_NAMES, got)), refs[i], "%s (thread %d, round %d)" % (CASES[i][0], k, r))
        return time.perf_counter() - t0

    run_threads(work)


# ---- b. the step API with summaries, interleaved -------------------------------------------------------------------------------
# model, n, seg, seed.  The summaries of the serial loop are pinned by test_gpu_summaries.py::test_summaries_exact_d1 /
# test_summaries_exact_ucsv (weighted) and test_gpu_unweighted_summaries.py::test_unweighted_exact_d1 / _ucsv, the change of mode
# in the middle of a run by test_gpu_unweighted_summaries.py::test_weighted_results_survive_a_detour, the marginal family's by
# test_gpu_rbpf.py; logmu, ess and the states are pinned below.
STEP_HANDLES = [(1, 1024, 0, 21), (1, 5000, 256, 22), (3, 300, 256, 23), (4, 1000, 0, 24),
                (1, 1024, 0, 31), (1, 5000, 256, 32), (3, 300, 256, 33), (4, 1000, 0, 34)]
STEPS = 30
LEVELS = [0.25, 0.5, 0.75]


def step_loop(L, spec):
    model, n, seg, seed = spec
    y = series(L, model, STEPS + 1)
    h = L.Handle(model, 1, n, seg=seg, seed=seed, flags=L.FLAG_ANCESTORS)
    try:
        h.set_params(SIM[model][1])
        out = {"logmu": [h.init(y[0])], "ess": [], "moments": [], "quantiles": [], "state": []}
        for t in range(1, STEPS + 1):
            lm, es = h.step(y[t])
            h.set_summary_mode("weighted" if t % 2 == 0 else "unweighted")
            out["logmu"].append(lm)
            out["ess"].append(es)
            out["moments"].append(h.moments())
            out["quantiles"].append(h.quantiles(LEVELS))
            if t % 10 == 0:
                out["state"].append(h.state())
        out["logZ"] = h.logZ()
        return out
    finally:
        h.close()


def pinned_step_trace(L, ob, spec):
    """(logmu [STEPS + 1], ess [STEPS], [(x, w) at every tenth step]) of the oracle (bootstrap) or the composed reference"""
    model, n, seg, seed = spec
    y = series(L, model, STEPS + 1)
    if model == 4:
        f = CR.ComposedFilter(L, ob, CR.RB, UC, n, seg=seg, seed=seed)
        lm, es, st = [f.init(y[0])[0]], [], []
        step, state = f.step, (lambda: f.snapshot()[:2])
    else:
        f = ob.Filter(model, SIM[model][1], n, seg=seg, seed=seed)
        lm, es, st = [f.bootstrap_filter(y[0])], [], []
        step, state = f.step, (lambda: f.state()[:2])
    for t in range(1, STEPS + 1):
        a, b = step(y[t])
        lm.append(a)
        es.append(b)
        if t % 10 == 0:
            st.append(state())
    return lm, es, st


def test_step_api_with_summaries_interleaved(L, ob):
    assert len(STEP_HANDLES) == WORKERS
    refs = [step_loop(L, s) for s in STEP_HANDLES]
    for s, ref in zip(STEP_HANDLES, refs):
        lm, es, st = pinned_step_trace(L, ob, s)
        assert_same(np.ravel(ref["logmu"]), np.array(lm), "%r logmu (serial against its pin)" % (s,))
        assert_same(np.ravel(ref["ess"]), np.array(es), "%r ess (serial against its pin)" % (s,))
        for (x, w, _), (ox, ow) in zip(ref["state"], st):
            assert_same((x[:, 0], w[0]), (ox, ow), "%r state (serial against its pin)" % (s,))

    def work(k, r):
        i = (k + 3 * r) % WORKERS
        assert_same(step_loop(L, STEP_HANDLES[i]), refs[i], "%r (thread %d, round %d)" % (STEP_HANDLES[i], k, r))

    run_threads(work)


# ---- c. a handle that migrates ------------------------------------------------------------------------------------------------------
def migrate_stages(L, n, seg, nth, perm, seed):
    """the four stages of one handle's life; box carries it from one to the next"""
    y = series(L, 1, 11)
    box = {"logmu": [], "ess": []}

    def create():
        box["h"] = h = L.Handle(1, nth, n, seg=seg, seed=seed, flags=L.FLAG_ANCESTORS)
        h.set_params(rows_for(LG, nth))
        box["logmu"].append(h.init(y[0]))

    def steps(t0):
        def f():
            for t in range(t0, t0 + 5):
                lm, es = box["h"].step(y[t])
                box["logmu"].append(lm)
                box["ess"].append(es)
        return f

    def permute_and_steps():
        box["h"].permute(np.array(perm, dtype=np.int32))
        steps(6)()

    def read():
        h = box.pop("h")
        try:
            x, w, a = h.state()
            return {"logmu": np.array(box["logmu"]), "ess": np.array(box["ess"]), "x": x, "w": w, "ancestors": a,
                    "logZ": h.logZ(), "raw": h.weights_raw()}
        finally:
            h.close()

    return [create, steps(1), permute_and_steps], read


def oracle_migration(L, ob, n, seg, nth, perm, seed):
    y, raws = series(L, 1, 11), rows_for(LG, nth)
    fs = [ob.Filter(1, raws[th], n, seg=seg, seed=seed, stream=th) for th in range(nth)]
    lm, es = [[f.bootstrap_filter(y[0]) for f in fs]], []
    for t in range(1, 11):
        if t == 6:                                        # a value copy of the state; every slot keeps its row and its stream
            bufs = [f.export_state() for f in fs]
            for th, f in enumerate(fs):
                f.import_state(bufs[perm[th]])
        r = [f.step(y[t]) for f in fs]
        lm.append([q[0] for q in r])
        es.append([q[1] for q in r])
    st = [f.state() for f in fs]
    return {"logmu": np.array(lm), "ess": np.array(es), "x": np.stack([s[0] for s in st], axis=1), "w": np.stack([s[1] for s in st])}


@pytest.mark.parametrize("n,seg,nth,perm", [(1024, 0, 6, [3, 3, 0, 5, 1, 1]), (5000, 256, 2, [1, 1])], ids=["lg1024x6", "lg5000seg256"])
def test_a_handle_moves_between_threads(L, ob, n, seg, nth, perm):
    """created and initialised in thread A, five steps in thread B, smc_permute and five more steps in thread C, read and destroyed
    in the main thread.  The threads hand over strictly one after another (a barrier after every stage): one caller at a time,
    which is what the contract asks for."""
    stages, read = migrate_stages(L, n, seg, nth, perm, 41)
    for f in stages:
        f()
    ref = read()                                          # the same sequence in one thread ...
    pin = oracle_migration(L, ob, n, seg, nth, perm, 41)  # ... which is the oracle's
    assert_same({k: ref[k] for k in pin}, pin, "serial against the oracle")
    for r in range(ROUNDS):
        stages, read = migrate_stages(L, n, seg, nth, perm, 41)
        gate = threading.Barrier(len(stages))

        def body(k, stages=stages, gate=gate):
            try:
                for turn in range(len(stages)):
                    if turn == k:
                        stages[k]()
                    gate.wait()
            except BaseException:
                gate.abort()
                raise

        with ThreadPoolExecutor(max_workers=WORKERS) as pool:
            for f in [pool.submit(body, k) for k in range(len(stages))]:
                f.result()
        assert_same(read(), ref, "round %d" % r)


# ---- d. the stand-alone entry points and thread exit --------------------------------------------------------------------------------
# sizes on both sides of 16384 (normalize: one workgroup / grid-wide) and 65536 (resample); the serial bits are the oracle's
# (test_gpu_parity.py::test_standalone_normalize_resample, test_device_math_is_bit_exact; test_gpu_api.py for the Kalman filter)
LADDER = (1, 63, 4096, 16384, 16385, 65536, 65537, 100000)
SHORT_LADDER = (63, 16385, 65537)
KALMAN_ROWS, KALMAN_T = 65, 20


def standalone_inputs(ob):
    rng = np.random.default_rng(11)
    inp = {}
    for n in LADDER:
        logw = rng.normal(size=n) * 5 - 100
        if n > 10:
            logw[3], logw[7] = -np.inf, np.nan
        lm, w, ess = ob.normalize(logw)
        inp[n] = (logw, (lm, w, ess), ob.resample(w, n + 1, seed=4, stream=2, t=n % 100).astype(np.int32))
    raws = np.tile(LG, (KALMAN_ROWS, 1))
    raws[:, 0] = rng.uniform(-0.95, 0.95, KALMAN_ROWS)
    raws[:, 2:4] = rng.lognormal(size=(KALMAN_ROWS, 2))
    y = rng.normal(size=KALMAN_T)
    kal = np.array([ob.kalman_log_likelihood(r, y) for r in raws])
    v = rng.uniform(-700, 5, 1000)
    return inp, (raws, y, kal), (v, ob.exp(v))


def standalone_at(L, n, inp, kalman, math, ctx):
    logw, norm, anc = inp[n]
    lm, w, ess = L.normalize(logw)
    assert_same((lm, w, ess), norm, "normalize %d %s" % (n, ctx))
    assert_same(L.resample(w, n + 1, seed=4, stream=2, t=n % 100), anc, "resample %d %s" % (n, ctx))
    assert_same(L.kalman_log_likelihood(kalman[0], kalman[1]), kalman[2], "kalman after %d %s" % (n, ctx))
    assert_same(L.device_math(0, math[0]), math[1], "exp after %d %s" % (n, ctx))


def test_standalone_calls_and_thread_exit(L, ob):
    inp, kalman, math = standalone_inputs(ob)

    def ladder_of(sizes):
        def work(k, r):
            order = list(sizes[(k + r) % len(sizes):] + sizes[:(k + r) % len(sizes)])       # the scratch of every thread grows and
            if k % 2:                                                                      # is refitted in an order of its own
                order.reverse()
            for n in order:
                standalone_at(L, n, inp, kalman, math, "(thread %d, round %d)" % (k, r))
        return work

    for n in SHORT_LADDER:
        standalone_at(L, n, inp, kalman, math, "(main thread, before the pools)")
    pool1 = ThreadPoolExecutor(max_workers=WORKERS)
    try:
        run_threads(ladder_of(LADDER), pool=pool1)
    finally:
        pool1.shutdown(wait=False)           # its threads end now, and their scratch is freed at their exit ...
    for n in LADDER:                         # ... while the main thread goes on launching
        standalone_at(L, n, inp, kalman, math, "(main thread, pool 1 ending)")
    pool1.shutdown(wait=True)
    run_threads(ladder_of(SHORT_LADDER))     # new threads, new scratch
    for n in SHORT_LADDER:
        standalone_at(L, n, inp, kalman, math, "(main thread, after the pools)")


# ---- e. mixed families through the Python layer ------------------------------------------------------------------------------------
def python_jobs():
    """8 jobs without arguments, each shape twice under different seeds; every seed is given (the module's seed counter in
    particles.py is shared by the threads and is not relied on)"""
    import sequential_monte_carlo_amd as smc
    from ibis_reference import case_readme
    from test_samplers_cpu import LG as LGD, LG_TMAP, lg_mod, lg_prior
    y = smc.simulate(smc.UnivariateLinearGaussian(**LGD), 30, seed=1998)[1]
    uc = smc.unobserved_components_stochastic_volatility(x0=3.0, gamma_eps=0.2, gamma_eta=0.2, log_sigma_eps=0.0, log_sigma_eta=0.0,
                                                         marginal=True)
    yu = smc.simulate(uc, 8, seed=1998)[1]
    three = [smc.UnivariateLinearGaussian(A=a, B=1.0, Q=0.9, R=0.8) for a in (0.1, 0.5, 0.9)]

    def smoother(seed):
        # (the device smoother and its paths: test_gpu_smoother.py::test_smooth_equals_host_twin, test_gpu_backward_paths.py)
        x, w, logZ, s = smc.smoother(300, y[:12], three, seed=seed, seg=256, paths=64, path_seed=seed + 100)
        return np.asarray(x), np.asarray(w), logZ, s

    def rb_smoother(seed):
        # (test_gpu_rb_paths.py::test_paths_equal_host_twin)
        x, w, logZ, s = smc.rb_smoother(300, yu, uc, paths=32, seed=seed, path_seed=seed + 100)
        return np.asarray(x), np.asarray(w), logZ, s

    def ibis(seed):
        # (test_gpu_ibis_device_moves.py::test_online_run_with_device_moves, test_gpu_rts.py::test_smooth_after_a_sampler_run)
        tmap, prior, model = case_readme(smc)
        ib = smc.IBIS(300, model, prior, 3, 0.5, seed=seed, theta_map=tmap, device_moves=True)
        try:
            smc.smc2(ib, y)
            smc.smc2_run(ib, y, 2, 30, verbose=False)
            return {"theta": ib.theta, "logZ": ib.logZ, "logw": ib.logw, "omega": ib.omega, "accepted": np.asarray(ib.accepted),
                    "acc_ratio": ib.acc_ratio, "n_rejuvenations": ib.n_rejuvenations, "ess": ib.ess,
                    "rts": smc.rts_smoothed_state(ib, y)}
        finally:
            ib.close()

    def tempered(seed):
        # (test_gpu_api.py::test_density_tempered_hip_equals_oracle_backend[True], at its shapes)
        backend = smc.smc_samplers.HipBackend()
        try:
            s = smc.SMC(256, 24, lg_mod, lg_prior(), 2, 0.5, seed=seed, backend=backend, theta_map=LG_TMAP)
            assert s.device_pmmh
            buf = io.StringIO()
            stages = smc.density_tempered(s, y[:24], verbose=True, out=buf)
            return {"theta": s.theta, "logZ": s.logZ, "logw": s.logw, "omega": s.omega, "stages": stages, "log": buf.getvalue(),
                    "psteps": s.psteps, "psteps_skipped": s.psteps_skipped}
        finally:
            backend.close()

    jobs = []
    for k, f in enumerate((smoother, rb_smoother, ibis, tempered)):
        for seed in (5 + k, 77 + k):
            jobs.append((f.__name__ + " seed %d" % seed, (lambda f=f, seed=seed: f(seed))))
    return jobs


def test_python_layer_mixed_families(L):
    jobs = python_jobs()
    assert len(jobs) == WORKERS
    refs = [f() for _, f in jobs]
    assert all(r["n_rejuvenations"] >= 1 for (name, _), r in zip(jobs, refs) if name.startswith("ibis"))

    def work(k, r):
        i = (k + 3 * r) % WORKERS
        assert_same(jobs[i][1](), refs[i], "%s (thread %d, round %d)" % (jobs[i][0], k, r))

    run_threads(work)
