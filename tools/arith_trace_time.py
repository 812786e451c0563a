#!/usr/bin/env python3
"""tools/arith_trace_time.py -- zkm_arithmetic_trace (csrc/arithmetic_trace.hip) at 2^16 / 2^18 / 2^20 / 2^21 operations, two mixes
(all 26 operators uniformly, and all DIV: two rows each and the modular helper): the sizing call, the trace call from device-resident
operations, the trace call from pinned host memory, the library's per-kernel records of the device call, and
tests/arith_fixtures.generate_trace (the CPU figure, 2^16 and 2^18 only).  The store floor is 432 B per output row (54 words) at
the HBM rate this tool measures with a device-to-device copy.  Operations as tests/test_gpu_arithmetic_trace.valid_ops.  Prints one
line per mix and size; times are medians of `reps` calls."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402
from tests import arith_fixtures as A  # noqa: E402
from tests.test_gpu_arithmetic_trace import valid_ops  # noqa: E402


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def hbm_rate(reps):
    """Bytes read + written per second by a 2 GiB device-to-device copy (torch, device events)."""
    import torch
    x = torch.empty(1 << 28, dtype=torch.int64, device="cuda")
    y = torch.empty_like(x)
    y.copy_(x)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        y.copy_(x)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    rate = 2 * x.numel() * 8 / float(np.median(ts))
    del x, y
    torch.cuda.empty_cache()
    return rate


def packed(ops):
    flat = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1)
    if flat.size & 1:
        flat = np.concatenate([flat, np.zeros(1, dtype=np.uint32)])
    return flat.view(np.uint64)


def main():
    reps = int(os.environ.get("REPS", "5"))
    rate = hbm_rate(reps)
    print("HBM copy rate %.2f TB/s" % (rate / 1e12), flush=True)
    ctx = zkm_amd.Context(0)
    for mix, which in (("uniform", None), ("div", [A.IS_DIV])):
        for lk in (16, 18, 20, 21):
            k = 1 << lk
            ops = valid_ops(lk, k, which)
            words = packed(ops)
            dev = ctx.alloc(words.size).upload(words)
            pinned = ctx.pinned_array(words.size)
            pinned[:] = words
            buf, natural = ctx.arithmetic_trace(dev, nops=k)    # warm-up (allocator, code objects)
            buf.free()
            log_n = natural.bit_length() - 1
            out = ctx.alloc(zkm_amd.ARITHMETIC_COLS << log_n)
            nat, err = C.c_size_t(), C.c_char_p()

            def call(src, n_log, o):
                zkm_amd._check(ctx.L.zkm_arithmetic_trace(ctx.h, src, k, n_log, o, C.byref(nat), C.byref(err)), err)
            dptr, hptr, optr = C.c_void_p(dev.ptr), pinned.ctypes.data_as(C.c_void_p), C.c_void_p(out.ptr)
            t_size = median_ms(lambda: call(dptr, 0, None), reps)
            t_dev = median_ms(lambda: call(dptr, log_n, optr), reps)
            t_host = median_ms(lambda: call(hptr, log_n, optr), reps)
            ctx.profile(True)
            ctx.profile_reset()
            call(dptr, log_n, optr)
            ctx.synchronize()
            recs = ctx.profile_records()
            ctx.profile(False)
            floor_ms = 432 * (1 << log_n) / rate * 1e3
            cpu = ""
            if lk <= 18:
                t0 = time.perf_counter()
                want = A.generate_trace([tuple(int(v) for v in o) for o in ops], log_n)
                cpu = ", fixture %.0f ms" % ((time.perf_counter() - t0) * 1e3)
                assert (out.download() == want).all(), "GPU table differs from the fixture's"
            kern = "; ".join("%s %.3f" % (name.split("/", 1)[-1], ms) for name, (_, ms) in recs.items()
                             if name.startswith("arithmetic_trace/"))
            print("%s 2^%d ops -> 2^%d rows: sizing %.3f ms, device-resident %.3f ms (store floor %.3f ms: %.0f %%), pinned host %.3f ms%s"
                  " | kernels (ms): %s" % (mix, lk, log_n, t_size, t_dev, floor_ms, 100 * floor_ms / t_dev, t_host, cpu, kern), flush=True)
            out.free()
            dev.free()
            ctx.free_pinned(pinned)
    ctx.close()


if __name__ == "__main__":
    main()
