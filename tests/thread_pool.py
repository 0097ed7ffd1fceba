"""TEST INFRASTRUCTURE of the host-thread tests (tests/test_threads_host.py, tests/test_gpu_threads.py): a fixed pool of host
threads that enter the library together, and exact comparison of whatever a call returns.

ctypes.CDLL releases the GIL for the length of every call, so Python threads are concurrent inside the library.  The property
the tests state is "concurrency changes no bit": every reference is the same call made serially before the pool starts, and
every comparison is equality of IEEE bit patterns or of integers.  Never imported by the product."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

WORKERS = 8      # a constant: never derived from the machine's CPU count
ROUNDS = 3       # a fixed number of rounds: nothing loops until something fails


def leaves(r, path=""):
    """a nested result (tuples, lists, dicts, arrays, scalars, strings, None) as a flat list of (path, leaf)"""
    if isinstance(r, dict):
        out = []
        for k in sorted(r):
            out += leaves(r[k], "%s[%r]" % (path, k))
        return out
    if isinstance(r, (tuple, list)):
        out = []
        for i, v in enumerate(r):
            out += leaves(v, "%s[%d]" % (path, i))
        return out
    return [(path, r)]


def mismatch(got, ref):
    """where two results differ - the path of the first leaf whose type, shape, dtype, bits (floats, NaN payloads included) or
    values (everything else) are not the same - or None"""
    a, b = leaves(got), leaves(ref)
    if [p for p, _ in a] != [p for p, _ in b]:
        return "structure: %s != %s" % ([p for p, _ in a], [p for p, _ in b])
    for (p, u), (_, v) in zip(a, b):
        if u is None or v is None or isinstance(u, (str, bytes)) or isinstance(v, (str, bytes)):
            if type(u) is not type(v) or u != v:
                return "%s: %r != %r" % (p, u, v)
            continue
        u, v = np.asarray(u), np.asarray(v)
        if u.shape != v.shape or u.dtype != v.dtype:
            return "%s: %s %s != %s %s" % (p, u.dtype, u.shape, v.dtype, v.shape)
        if u.dtype == np.float64:
            u, v = np.ascontiguousarray(u).view(np.uint64), np.ascontiguousarray(v).view(np.uint64)
        if not np.array_equal(u, v):
            bad = np.flatnonzero(np.ravel(u != v))
            return "%s: %d of %d entries differ, the first at flat index %d" % (p, bad.size, u.size, int(bad[0]))
    return None


def assert_same(got, ref, ctx):
    bad = mismatch(got, ref)
    assert bad is None, "%s: %s" % (ctx, bad)


def run_threads(work, workers=WORKERS, rounds=ROUNDS, pool=None):
    """work(k, r) for k < workers in `workers` threads of one pool, r = 0 .. rounds - 1: a barrier at the head of every round lets
    the threads enter the library together.  work asserts for itself; the first failure breaks the barrier (no thread is left
    waiting for one that has gone) and is raised here.  -> [k][r] what work returned.  pool: an executor the caller keeps"""
    barrier = threading.Barrier(workers)

    def body(k):
        try:
            out = []
            for r in range(rounds):
                barrier.wait()
                out.append(work(k, r))
            return out
        except BaseException:
            barrier.abort()
            raise

    own = pool is None
    if own:
        pool = ThreadPoolExecutor(max_workers=workers)
    try:
        futures = [pool.submit(body, k) for k in range(workers)]
        results, errors = [], []
        for f in futures:
            try:
                results.append(f.result())
            except threading.BrokenBarrierError:      # a sibling failed first: its error is the finding
                results.append(None)
            except BaseException as e:                # noqa: BLE001
                results.append(None)
                errors.append(e)
    finally:
        if own:
            pool.shutdown(wait=True)
    if errors:
        raise errors[0]
    assert all(r is not None for r in results), "a barrier broke without an error"
    return results
