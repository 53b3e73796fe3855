"""The profiler has a lock of its own (cs_core.hip: g_prof_mu), apart from the buffer pool's.

cs_prof_reset and cs_prof_get wait for the events of the launches they account for while they hold the profiler's lock.
When that lock was the pool's, every allocation of every thread waited with them.  Here one thread resets and reads the
profile in a loop while another runs 200 lower() calls on a stream of its own, each of which allocates from the pool
and ends a ProfScope (`k_lower_write`): both threads finish, and every result is the one a single thread gets."""
import ctypes as C
import threading

import numpy as np
import pytest

import gpuutil

pytestmark = pytest.mark.gpu

ROWS = 1000
CALLS = 200


def test_prof_reset_and_get_beside_ops_on_another_thread():
    import torch

    from custrings_amd import nvstrings

    L = gpuutil.lib()
    g = gpuutil.synth(2, 0, ROWS)
    want = gpuutil.to_col(g.lower())  # single-threaded, profiling off
    assert want.rows == ROWS

    stream = torch.cuda.Stream()
    results, errors = [], []
    done = threading.Event()
    polls = [0]

    def poll():  # thread A
        try:
            ms, n = C.c_double(), C.c_int64()
            while not done.is_set():
                L.check(L.lib.cs_prof_reset())
                L.check(L.lib.cs_prof_get(b"k_lower_write", C.byref(ms), C.byref(n)))
                polls[0] += 1
        except Exception as e:  # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    def work():  # thread B
        try:
            h = C.c_void_p(stream.cuda_stream)
            for _ in range(CALLS):
                out = C.c_void_p()
                L.check(L.lib.cs_lower(g.m_cptr, h, C.byref(out)))
                results.append(nvstrings.nvstrings(out.value))
        except Exception as e:  # noqa: BLE001
            errors.append(e)
        finally:
            done.set()

    L.lib.cs_prof_enable(1)
    try:
        a, b = threading.Thread(target=poll), threading.Thread(target=work)
        a.start()
        b.start()
        b.join(120)
        done.set()
        a.join(120)
        assert not a.is_alive() and not b.is_alive(), "a thread did not finish: the profiler and the pool wait for each other"
    finally:
        L.lib.cs_prof_enable(0)
        L.lib.cs_prof_reset()
    assert errors == []
    assert polls[0] >= 1 and len(results) == CALLS
    stream.synchronize()
    for i, r in enumerate(results):
        got = gpuutil.to_col(r)
        assert got.rows == want.rows, i
        assert np.array_equal(got.bitmask(), want.bitmask()), i
        assert np.array_equal(got.offsets, want.offsets) and np.array_equal(got.chars, want.chars), i
