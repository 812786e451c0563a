#!/usr/bin/env python3
"""tools/segments_ops_time.py -- K segments built from their raw operations in one set of launches and proven in lock-step
(zkm_segments_tables / zkm_prove_segments_ops / zkm_segment_ops_stage, csrc/segment_ops.hip) against the composition the
single-segment entry points allow, timed in the same run: the tools/bench_segment.HEIGHTS[16] shape, random valid operations
(tests/segment_ops_fixtures.random_segment_ops) with the sample program's CPU rows tiled to 2^16 (a proven segment needs 0 / 1 lookup
filters), medians and ranges of REPS (default 7) timed calls after warm-up, every leg checked against the single-segment words after
the clock.
  build     eight segments, device-resident lists: eight zkm_segment_tables calls against one zkm_segments_tables call, with the
            kernel time by scope of each;
  one       one context, eight segments a call, lists in pinned host memory: eight zkm_segment_tables then zkm_prove_segments, against
            zkm_prove_segments_ops on operations staged during the previous call;
  many      CONTEXTS (default 8) contexts x eight segments a call: finished tables in HBM, finished tables staged from pinned memory
            (tools/bench_segment.lockstep_segment_rate), operations staged from pinned memory;
  --one     a single zkm_segment_tables call from pinned memory after warm-up and nothing else: the run to put under a kernel trace.
Prints one JSON object; LEGS=build,one,many chooses."""
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402
from tests import segment_ops_fixtures as SF  # noqa: E402
from tools.bench_segment import HEIGHTS, lockstep_segment_rate  # noqa: E402

K = 8
LG = HEIGHTS[16]
WIDTHS = [54, 259, 262, 110, 2431, 470, 78, 76, 224, 127, 69, 13]
TABLE_BYTES = 8 * sum(w << lg for w, lg in zip(WIDTHS, LG))


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def timed(fn, reps, sync):
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def raws(n, seed=100):
    from oracle.oracle_py import Oracle
    rows = SF.build_segment_ops(Oracle())[0]["cpu_rows"].reshape(-1, 259)
    cpu = np.ascontiguousarray(np.tile(rows, ((1 << LG[1]) // len(rows) + 1, 1))[:1 << LG[1]])
    return [dict(SF.random_segment_ops(LG, seed=seed + s), cpu_rows=cpu) for s in range(n)]


def ops_bytes(ops):
    return int(sum(v.nbytes for v in ops.lists.values() if isinstance(v, np.ndarray)))


def free_pinned(ctx, ops):
    for k, v in ops.lists.items():
        if not k.endswith("_off"):
            ctx.free_pinned(v)


def scopes(ctx, fn, reps):
    """kernel milliseconds by scope per call of fn (event profile; the generation scopes only)"""
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        fn()
    recs = ctx.profile_records()
    ctx.profile(False)
    return {k: {"launches_per_call": n / reps, "ms_per_call": round(ms / reps, 4)} for k, (n, ms) in sorted(recs.items())
            if not k.startswith("stage/")}


def leg_build(ctx, reps):
    dev = [SF.segment_ops(zkm_amd, r).to_device(ctx) for r in raws(K)]

    def alone():
        for o in dev:
            ctx.segment_tables(o)[0].free()

    def batched():
        for st, _ in ctx.segments_tables(dev):
            st.free()
    alone(), batched()
    res = {"segments": K, "eight_segment_tables_calls": stats(timed(alone, reps, ctx.synchronize)),
           "one_segments_tables_call": stats(timed(batched, reps, ctx.synchronize)),
           "kernels_alone": scopes(ctx, alone, reps), "kernels_batched": scopes(ctx, batched, reps)}
    same = True
    built = ctx.segments_tables(dev)
    for o, (st, lg) in zip(dev, built):
        one, lg1 = ctx.segment_tables(o)
        same &= lg == lg1
        for a, b, w, l in zip(st.tables(), one.tables(), WIDTHS, lg):
            va, vb = zkm_amd.DeviceBuffer.__new__(zkm_amd.DeviceBuffer), zkm_amd.DeviceBuffer.__new__(zkm_amd.DeviceBuffer)
            va.ctx, va.words, va.ptr = ctx, w << l, a
            vb.ctx, vb.words, vb.ptr = ctx, w << l, b
            same &= bool((va.download() == vb.download()).all())
        one.free()
        st.free()
    res["batched_equals_alone"] = same
    for o in dev:
        o.free()
    return res


def staged_loop(ctx, pinned, pubs, sizes, reps, results=None, per_call=None):
    """reps calls of prove_segments_ops, each on lists staged during the call before it"""
    cur = [ctx.stage_segment_ops(o) for o in pinned]
    for _ in range(reps):
        t0 = time.perf_counter()
        nxt = [ctx.stage_segment_ops(o) for o in pinned]
        out = ctx.prove_segments_ops([s.ops() for s in cur], public_values=pubs, sizes=sizes)
        for s in cur:
            s.free()
        cur = nxt
        if per_call is not None:
            per_call.append((time.perf_counter() - t0) * 1e3)
        if results is not None:
            results.append(out)
    for s in cur:
        s.free()


def leg_one(ctx, reps):
    pinned = [SF.segment_ops(zkm_amd, r).to_pinned(ctx) for r in raws(K)]
    pubs = [[1, 2, 3, s] for s in range(K)]

    def composed():
        built = [ctx.segment_tables(o) for o in pinned]
        out = ctx.prove_segments([(st.tables(), lg, pub) for (st, lg), pub in zip(built, pubs)])
        for st, _ in built:
            st.free()
        return out
    want = composed()
    sizes = [o for _, _, o in want]
    staged_loop(ctx, pinned, pubs, sizes, 2)
    base = timed(composed, reps, ctx.synchronize)
    new, got = [], []
    ctx.synchronize()
    staged_loop(ctx, pinned, pubs, sizes, reps, results=got, per_call=new)
    ctx.synchronize()
    same = all((p == pw).all() and (c == cw).all() for call in got for (p, c, _), (pw, cw, _) in zip(call, want))
    alone = ctx.prove_segment_ops(pinned[3], public_values=pubs[3])
    same &= bool((alone[0] == want[3][0]).all())
    res = {"segments_per_call": K, "eight_segment_tables_then_prove_segments": stats(base), "prove_segments_ops_staged": stats(new),
           "segments_per_s": {"composed": round(K * 1e3 / float(np.median(base)), 1), "staged_ops": round(K * 1e3 / float(np.median(new)), 1)},
           "bytes_over_link_per_segment": ops_bytes(pinned[0]), "equal_single_segment_words": bool(same)}
    for o in pinned:
        free_pinned(ctx, o)
    return res


def leg_many(nctx, reps):
    device = int(os.environ.get("ZKM_BENCH_DEVICE", "0"))
    res = {"contexts": nctx, "segments_per_call": K}
    for name, host in (("tables_in_hbm", 0), ("tables_staged_from_pinned", 2)):
        r = lockstep_segment_rate(device, 16, nctx, K, reps=reps, host=host)
        res[name] = {k: r[k] for k in ("segments_per_s", "ms_per_call", "calls_per_context", "traces")}
    res["tables_staged_from_pinned"]["bytes_over_link_per_segment"] = TABLE_BYTES
    ctxs = [zkm_amd.Context(device) for _ in range(nctx)]
    raw = raws(1)[0]
    pinned = [[SF.segment_ops(zkm_amd, raw).to_pinned(c)] * K for c in ctxs]      # (a call's segments share their lists, as the tables legs do)
    pubs = [[[1, 2, 3, i, j] for j in range(K)] for i in range(nctx)]
    want = ctxs[0].prove_segment_ops(pinned[0][0], public_values=pubs[0][0])
    sizes = [want[2]] * K
    for c, p, pv in zip(ctxs, pinned, pubs):
        staged_loop(c, p, pv, sizes, 2)
        c.synchronize()
    start = threading.Barrier(nctx + 1)
    got = [[] for _ in ctxs]

    def work(i):
        start.wait()
        staged_loop(ctxs[i], pinned[i], pubs[i], sizes, reps, results=got[i])
        ctxs[i].synchronize()
    th = [threading.Thread(target=work, args=(i,)) for i in range(nctx)]
    for t in th:
        t.start()
    start.wait()
    t0 = time.perf_counter()
    for t in th:
        t.join()
    wall = time.perf_counter() - t0
    res["ops_staged_from_pinned"] = {"segments_per_s": round(nctx * K * reps / wall, 1), "wall_s": round(wall, 3), "segments": nctx * K * reps,
                                     "bytes_over_link_per_segment": ops_bytes(pinned[0][0]),
                                     "equal_single_segment_words": bool((got[0][-1][0][0] == want[0]).all() and (got[0][-1][0][1] == want[1]).all())}
    for c, p in zip(ctxs, pinned):
        free_pinned(c, p[0])
        c.close()
    return res


def main():
    reps = int(os.environ.get("REPS", "7"))
    if "--one" in sys.argv:
        ctx = zkm_amd.Context(0)
        pinned = SF.segment_ops(zkm_amd, raws(1)[0]).to_pinned(ctx)
        for _ in range(3):
            ctx.segment_tables(pinned)[0].free()
        ctx.synchronize()
        print(json.dumps({"tool": "segments_ops_time --one", "segment_tables_pinned_ms": stats(timed(lambda: ctx.segment_tables(pinned)[0].free(), 1, ctx.synchronize))}))
        free_pinned(ctx, pinned)
        ctx.close()
        return
    legs = os.environ.get("LEGS", "build,one,many").split(",")
    out = {"tool": "segments_ops_time", "reps": reps, "log_heights": LG}
    if "build" in legs or "one" in legs:
        ctx = zkm_amd.Context(0)
        if "build" in legs:
            out["build"] = leg_build(ctx, reps)
        if "one" in legs:
            out["one"] = leg_one(ctx, reps)
        ctx.close()
    if "many" in legs:
        out["many"] = leg_many(int(os.environ.get("CONTEXTS", "8")), max(3, reps // 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
