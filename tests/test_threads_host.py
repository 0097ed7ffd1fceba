"""Host threads, the part that needs no GPU (DESIGN.md "Host threads").

  a. the host twins (smc_host_*) and smc_simulate called from 8 threads at once, every thread in an order of its own, give the
     bits of the same calls made one after another: none of them keeps state between calls or shares a buffer
  b. smc_last_error is per thread: two threads that fail with different argument errors, interleaved step by step, each read
     their own message afterwards, and a thread that never failed reads neither

The references are the serial calls of the main thread, made before the pool starts; what pins the serial bits themselves is
named beside each call.  Every comparison is exact (tests/thread_pool.py)."""
import ctypes as C
import random
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from thread_pool import ROUNDS, WORKERS, assert_same, run_threads

LG = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
SV = [-1.0, 0.95, 0.25]
UC = [0.2, 0.2, 3.0, 0.0, 0.0]
AFFINE, OPTIMAL = 1, 2
POOR = [0.3, 0.2, 0.1, 2.0]
T = 6


def host_calls(L, n, rng):
    """name -> a call without arguments of one host entry point on inputs of n particles (parameter particles, entries) over T
    steps; the inputs are drawn once, here, and only read afterwards"""
    def cloud(d):
        w = rng.dirichlet(np.ones(n), size=T)
        w[1, n // 3] = 0.0                                                   # a particle without weight
        return rng.normal(size=(T, d, n)), w

    x1, w1 = cloud(1)
    xs, wsv = cloud(1)
    x4, w4 = cloud(4)
    x4[:, 1:3] *= 0.5
    x4[:, 3] = np.exp(0.5 * x4[:, 3])                                        # the trend's variance row is positive
    y = 3.0 + rng.normal(size=T)
    xp3, z3 = rng.normal(size=(3, n)), rng.normal(size=(3, n))
    sp, z2 = x4[2].copy(), rng.normal(size=(2, n))
    rows = np.tile(LG, (n, 1))
    rows[:, 0] = rng.uniform(-0.9, 0.9, n)
    rows[:, 2:4] = rng.lognormal(size=(n, 2))
    logw = 3.0 * rng.normal(size=n) - 50.0
    logz = logw.copy()                                                       # (finite: the tempering ladder multiplies it)
    logw[n // 2] = -np.inf
    which = rng.integers(0, n, 40).astype(np.int32)
    theta = rng.normal(size=(n, 3)) * [1.0, 0.1, 10.0] + [0.0, 2.0, -5.0]
    rec = L.host_outer_records(logw)
    return {
        # tests/test_guided_host.py pins the guided twins to extended precision, tests/test_rbpf_host.py the marginal one
        "guided_steps lg optimal": lambda: L.host_guided_steps(1, LG, OPTIMAL, None, x1[0], x1[1], 0.3),
        "guided_steps lg affine": lambda: L.host_guided_steps(1, LG, AFFINE, POOR, x1[2], x1[3], -0.7),
        "guided_steps ucsv optimal": lambda: L.host_guided_steps(3, UC, OPTIMAL, None, xp3, z3, 2.9),
        "rb_steps first": lambda: L.host_rb_steps(UC, sp, z2, 3.1, True),
        "rb_steps": lambda: L.host_rb_steps(UC, sp, z2, 2.6, False),
        # tests/test_smoother_host.py (smoother_reference.py), tests/test_paths_host.py, tests/test_rb_paths_host.py
        "smooth lg": lambda: L.host_smooth(1, LG, x1, w1),
        "smooth sv": lambda: L.host_smooth(2, SV, xs, wsv),
        "sample_paths lg": lambda: L.host_sample_paths(1, LG, x1, w1, 32, 99, stream=3),
        "sample_paths sv": lambda: L.host_sample_paths(2, SV, xs, wsv, 7, 2 ** 63 + 5, stream=0),
        "rb_sample_paths": lambda: L.host_rb_sample_paths(UC, x4, w4, y, 16, 5, stream=1, draws=True),
        # tests/test_rts_host.py (rts_reference.py)
        "ibis_smooth": lambda: L.host_ibis_smooth(rows, logw, y, states=True, filtered=True),
        "ibis_sample_paths": lambda: L.host_ibis_sample_paths(rows, y, which, 77, want_z=True),
        # tests/test_host.py and tests/test_samplers_cpu.py pin the outer level to the oracle's orc_outer_*
        "outer_records": lambda: L.host_outer_records(logw),
        "outer_combine": lambda: L.host_outer_combine(rec, n),
        "outer_temper": lambda: L.host_outer_temper(logz, 0.1, 0.5 * n),
        "outer_resample": lambda: L.host_outer_resample(logw, n + 1, 123),
        "rw_factor": lambda: L.host_rw_factor(theta),
        # tests/test_ibis_device_moves_host.py
        "theta_moments": lambda: L.host_theta_moments(theta),
        "theta_moments weighted": lambda: L.host_theta_moments(theta, logw, weighted=True),
        # tests/test_host.py: smc_simulate against the oracle's orc_simulate
        "simulate lg": lambda: L.simulate(1, LG, T + n, 1998),
        "simulate sv": lambda: L.simulate(2, SV, T + n, 7),
        "simulate ucsv": lambda: L.simulate(3, UC, T + n, 11),
    }


def test_host_twins_from_eight_threads_equal_their_serial_results(L):
    rng = np.random.default_rng(2024)
    calls = {}
    for n in (65, 300):                      # a partial chunk of the smoother's sums, and more than two of them
        for name, f in host_calls(L, n, rng).items():
            calls["%s, n = %d" % (name, n)] = f
    ref = {name: f() for name, f in calls.items()}               # serially, in the main thread, before the pool starts
    again = {name: f() for name, f in calls.items()}
    for name in calls:
        assert_same(again[name], ref[name], name + " (serial, twice)")

    def work(k, r):
        order = list(calls)
        random.Random(100 * r + k).shuffle(order)                 # every thread, every round: an order of its own
        for name in order:
            assert_same(calls[name](), ref[name], "%s (thread %d, round %d)" % (name, k, r))
        return len(order)

    done = run_threads(work)
    assert done == [[len(calls)] * ROUNDS] * WORKERS


def test_last_error_is_per_thread(L):
    """A: smc_create with seg = 300 (refused on its arguments, before any device call); then B: smc_host_quantile7 with the level
    1.5; only then do both read smc_last_error.  A shared string would hand A the message of B.  Argument errors only."""
    lib = L.lib()
    gate = threading.Barrier(3)
    main_before = lib.smc_last_error()

    def stepped(f):
        def body():
            try:
                return f()
            except BaseException:
                gate.abort()
                raise
        return body

    def thread_a():
        gate.wait()
        h = C.c_void_p()
        rc = lib.smc_create(L.MODEL_LG1D, 1, 1024, 300, 1, 0, 0, C.byref(h))
        gate.wait()                          # A has failed
        gate.wait()                          # B has failed
        return rc, h.value, lib.smc_last_error().decode()

    def thread_b():
        gate.wait()
        gate.wait()
        x, p, out = np.arange(3.0), np.array([1.5]), np.zeros(1)
        rc = lib.smc_host_quantile7(x.ctypes.data_as(L._dp), 3, p.ctypes.data_as(L._dp), 1, out.ctypes.data_as(L._dp))
        gate.wait()
        return rc, None, lib.smc_last_error().decode()

    def thread_c():
        for _ in range(3):
            gate.wait()
        return 0, None, lib.smc_last_error().decode()

    with ThreadPoolExecutor(max_workers=WORKERS) as pool:
        fa, fb, fc = (pool.submit(stepped(f)) for f in (thread_a, thread_b, thread_c))
        (rc_a, h_a, msg_a), (rc_b, _, msg_b), (rc_c, _, msg_c) = fa.result(), fb.result(), fc.result()
    assert rc_a != 0 and h_a is None and rc_b != 0 and rc_c == 0
    assert msg_a == "smc_create: seg must be a power of two in [256,8192]", msg_a
    assert msg_b == "smc_host_quantile7: levels must lie in [0, 1]", msg_b
    assert msg_c not in (msg_a, msg_b) and "smc_create" not in msg_c and "quantile7" not in msg_c, msg_c
    assert lib.smc_last_error() == main_before                   # nor has the main thread's message changed
