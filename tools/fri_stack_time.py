#!/usr/bin/env python3
"""tools/fri_stack_time.py -- what stacking buys the general FRI pair, timed in one run on one context.
The instance is the PLONK shape of tests/test_gpu_fri_verify.py at 2^12 rows: four oracles of 7, 9, 5 and 4 columns, one batch at zeta
over all of them and one at g zeta over two of one; rate_bits 3, cap_height 4, arity_bits 4, final_poly_bits 5; six queries as in the
tests, and 28 (standard_recursion_config) beside them.  K = 8 claims, each with its own polynomials, points and challenger.
  (a) ONE Context.fri_prove_stack call on four stacks of 8 against the EIGHT Context.fri_prove calls on single commitments that the
      same work took before; the K blobs are compared word for word before anything is timed;
  (b) PolynomialBatchStack.from_values (9 columns) and .from_coeffs (4 columns) of 8 members against eight PolynomialBatch
      constructors, sources in host memory; every constructor ends with its caps on the host, so the clock stops behind the device.
The two sides of a comparison run in the same process, alternating (the order swaps every round), REPS (default 20) timed rounds after a
warm-up round; a figure is the median with min and max.  Host waits are zkm_ctx_host_waits around the call(s); launch scopes are the
records of zkm_profile_* in one extra round with the profiler on (a scope is one launch or a small group of launches), outside the timed
rounds.  Writes profiles/fri_stack_time.json (or OUT).  LOG_N (default 12) is the height; ZKM_HIP_LIB, as everywhere, the library: the
"single" arms of runs on two builds are how profiles/fri_single_path_time.json compares the single call before and after it became
the stacked body at one claim (tools/fri_single_path_compare.py)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402

P = zkm_amd.P
K, LOG_N, COLS = 8, int(os.environ.get("LOG_N", "12")), [7, 9, 5, 4]
LISTS = [[(o, c) for o in range(4) for c in range(COLS[o])], [(2, 0), (2, 1)]]


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "rounds": len(ms)}


def challengers(seed):
    out = []
    for k in range(K):
        ch = zkm_amd.challenger_new()
        zkm_amd.challenger_observe(ch, [seed, k])
        out.append(ch)
    return out


def alternating(ctx, sides, reps):
    """sides = {name: callable, returning what is to be freed}: every round runs each once, the order swapping; returns {name: (stats, host waits seen, launch scopes)}"""
    names = list(sides)
    ms, waits, scopes = {n: [] for n in names}, {n: set() for n in names}, {}
    for rnd in range(reps + 1):
        for n in (names if rnd % 2 == 0 else names[::-1]):
            ctx.synchronize()
            w0, t0 = ctx.host_waits(), time.perf_counter()
            made = sides[n]()
            dt, w = (time.perf_counter() - t0) * 1e3, ctx.host_waits() - w0
            for b in made or ():       # (what a side made is freed behind the clock)
                b.free()
            if rnd:
                ms[n].append(dt)
                waits[n].add(w)
    ctx.profile(True)
    for n in names:
        ctx.profile_reset()
        for b in sides[n]() or ():
            b.free()
        scopes[n] = int(sum(v[0] for name, v in ctx.profile_records().items() if not name.startswith("stage/")))
    ctx.profile(False)
    return {n: {"ms": stats(ms[n]), "host_waits": sorted(waits[n]), "launch_scopes": scopes[n]} for n in names}


def ratio(r, stacked, single):
    a, b = r[stacked]["ms"], r[single]["ms"]
    return {"stacked_over_single_median": round(a["median_ms"] / b["median_ms"], 3),
            "stacked_no_slower_beyond_the_spread": bool(a["median_ms"] <= b["max_ms"])}


def main():
    reps = int(os.environ.get("REPS", "20"))
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "fri_stack_time.json"))
    ctx = zkm_amd.Context(0)
    rng = np.random.default_rng(4100)
    values = [[rng.integers(0, P, c << LOG_N, dtype=np.uint64) for c in COLS] for _ in range(K)]
    points = [[(24680 + LOG_N + 1000 * k, 13579 + 7 * k), (97531 + k, 86420 + 3 * k)] for k in range(K)]
    out = {"about": "tools/fri_stack_time.py: one fri_prove_stack call of K claims against K fri_prove calls, and the stack constructors against "
                    "K single constructors; same process, alternating, median [min, max] of `reps` rounds after a warm-up",
           "reps": reps, "K": K, "log_n": LOG_N, "columns": COLS, "batches": [len(l) for l in LISTS], "rate_bits": 3, "prove": [], "commit": {}}
    for nq in (6, 28):
        cfg = ctx.standard_config()
        cfg.rate_bits, cfg.cap_height, cfg.arity_bits, cfg.final_poly_bits, cfg.num_queries = 3, 4, 4, 5, nq
        singles = [[zkm_amd.PolynomialBatch.from_values(ctx, v[o], COLS[o], LOG_N, 3, 4) for o in range(4)] for v in values]
        stacks = [zkm_amd.PolynomialBatchStack.from_values(ctx, [v[o] for v in values], COLS[o], LOG_N, 3, 4) for o in range(4)]
        got = {}

        def stacked():
            got["stacked"] = ctx.fri_prove_stack(stacks, LISTS, points, challengers(nq), cfg)

        def single():
            chs = challengers(nq)
            got["single"] = [ctx.fri_prove(singles[k], list(zip(points[k], LISTS)), chs[k], cfg) for k in range(K)]

        stacked()
        single()
        assert all(np.array_equal(a, b) for a, b in zip(got["stacked"], got["single"])), "the stacked blobs are not the single calls'"
        r = alternating(ctx, {"fri_prove_stack_x1": stacked, "fri_prove_x8": single}, reps)
        out["prove"].append({"num_queries": nq, "pow_bits": int(cfg.pow_bits), **r, **ratio(r, "fri_prove_stack_x1", "fri_prove_x8")})
        for b in stacks + [b for s in singles for b in s]:
            b.free()
    for what, o, single_ctor, stack_ctor in (("from_values", 1, zkm_amd.PolynomialBatch.from_values, zkm_amd.PolynomialBatchStack.from_values),
                                             ("from_coeffs", 3, zkm_amd.PolynomialBatch.from_coeffs, zkm_amd.PolynomialBatchStack.from_coeffs)):
        members = [v[o] for v in values]

        def stacked():
            return [stack_ctor(ctx, members, COLS[o], LOG_N, 3, 4)]

        def single():
            return [single_ctor(ctx, m, COLS[o], LOG_N, 3, 4) for m in members]

        r = alternating(ctx, {"stack_x1": stacked, "single_x8": single}, reps)
        out["commit"][what] = {"columns": COLS[o], **r, **ratio(r, "stack_x1", "single_x8")}
    ctx.close()
    text = json.dumps(out, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
