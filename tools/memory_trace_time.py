#!/usr/bin/env python3
"""tools/memory_trace_time.py -- zkm_memory_trace (csrc/memory_trace.hip) at 2^16 / 2^18 / 2^20 / 2^22 operations: the sizing call, the
trace call from device-resident operations, the trace call from pinned host memory, the library's per-kernel records of the device
call, and the CPU oracle's zko_memory_trace.  Operations as tests/test_oracle_tables.random_memory_ops (vectorised here: 2 contexts,
5 segments, 40 addresses, distinct timestamps).  Prints one line per size; times are medians of `reps` calls."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402
from oracle.oracle_py import Oracle  # noqa: E402


def make_ops(k, seed):
    rng = np.random.default_rng(seed)
    ops = np.zeros((k, 6), dtype=np.uint64)
    ops[:, 0] = rng.integers(0, 2, k)
    ops[:, 1] = rng.integers(0, 5, k)
    ops[:, 2] = rng.integers(0, 40, k) * 4
    ops[:, 3] = rng.permutation(k) * 3 + 1
    ops[:, 4] = rng.integers(0, 2, k)
    ops[:, 5] = rng.integers(0, 1 << 32, k)
    return ops


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    reps = int(os.environ.get("REPS", "5"))
    ctx = zkm_amd.Context(0)
    oracle = Oracle()
    for lk in (16, 18, 20, 22):
        k = 1 << lk
        ops = make_ops(k, lk)
        dev = ctx.alloc(ops.size).upload(ops)
        pinned = ctx.pinned_array(ops.size)
        pinned[:] = ops.reshape(-1)
        _, natural = ctx.memory_trace(dev)               # warm-up (allocator, code objects)
        log_n = natural.bit_length() - 1
        out = ctx.alloc(zkm_amd.MEMORY_COLS << log_n)
        ctx.memory_trace(dev, log_n, out)
        nat, err = C.c_size_t(), C.c_char_p()

        def sizing():
            zkm_amd._check(ctx.L.zkm_memory_trace(ctx.h, C.c_void_p(dev.ptr), k, 0, None, C.byref(nat), C.byref(err)), err)
        t_size = median_ms(sizing, reps)
        t_dev = median_ms(lambda: ctx.memory_trace(dev, log_n, out), reps)
        t_host = median_ms(lambda: ctx.memory_trace(pinned, log_n, out), reps)
        ctx.profile(True)
        ctx.profile_reset()
        ctx.memory_trace(dev, log_n, out)
        ctx.synchronize()
        recs = ctx.profile_records()
        ctx.profile(False)
        got = out.download()
        t0 = time.perf_counter()
        want, wnat = oracle.memory_trace(ops, log_n)
        t_cpu = (time.perf_counter() - t0) * 1e3
        assert wnat == natural and (got == want).all(), "GPU table differs from the oracle's"
        kern = "; ".join("%s %.3f" % (name.split("/", 1)[-1], ms) for name, (_, ms) in recs.items() if name.startswith("memory_trace/"))
        print("2^%d ops -> 2^%d rows: sizing %.2f ms, device-resident %.2f ms, pinned host %.2f ms, oracle %.0f ms | kernels (ms): %s"
              % (lk, log_n, t_size, t_dev, t_host, t_cpu, kern), flush=True)
        out.free()
        dev.free()
        ctx.free_pinned(pinned)
    ctx.close()


if __name__ == "__main__":
    main()
