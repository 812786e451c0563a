#!/usr/bin/env python3
"""tools/verify_time.py -- what verify_proof on the device costs, in one run: zkm_verify_segments on 8 proofs of the 2^16-cycle
segment (tests/segment_ops_fixtures.build_segment_ops, repeat=128) and on 1, blobs in host memory; against what it replaces -- the
oracle's verify_all (the restated sequential verifier, `kind: port`) on the same 8 blobs spread over the CPUs the process may use, one
blob per thread -- and against what it follows: zkm_prove_segments of the same 8 segments, and the same call with "verify" at 1.
Wall clock around calls that end synchronised (a verify call ends in its one download), every shape warmed first, at least a second
of timed work per figure.  Writes profiles/verify_time.json and prints it.  --one: a single warmed verify call of 8 and nothing else
(the run to put under a kernel trace); --one-prove: the same for the prove call of 8.  --ab: only the figures two builds are compared
by -- verify of 8, verify of 1, prove of 8 -- printed, nothing written."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402
from bench import cpu_quota  # noqa: E402
from oracle.oracle_py import Oracle  # noqa: E402
from tests import segment_ops_fixtures as SF  # noqa: E402

K = 8
PUB = [1, 2]


def timed(fn, min_s=1.0, min_calls=5):
    fn()
    ms = []
    while sum(ms) < min_s * 1e3 or len(ms) < min_calls:
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def main():
    oracle = Oracle()
    ctx = zkm_amd.Context(0)
    raw, tables, ctls = SF.build_segment_ops(oracle, repeat=128)
    lg = [t[3] for t in tables]
    segments = [([t[1] for t in tables], lg, PUB)] * K
    proven = ctx.prove_segments(segments)
    proofs, chals = [p for p, _, _ in proven], [c for _, c, _ in proven]

    def verify(k):
        reps = ctx.verify_segments(proofs[:k], [PUB] * k, chals[:k])
        assert all(r.code == 0 and r.host_waits == 1 for r in reps)

    def prove():
        ctx.prove_segments(segments)
        ctx.synchronize()
    if "--one" in sys.argv:
        verify(K), verify(K)
        return
    if "--one-prove" in sys.argv:
        prove(), prove()
        return
    if "--ab" in sys.argv:
        print(json.dumps({"verify_segments_8": timed(lambda: verify(K)), "verify_segments_1": timed(lambda: verify(1)), "prove_segments_8": timed(prove)}))
        return
    threads = max(1, min(16, os.cpu_count() or 1, cpu_quota() or 16))
    oracle.set_threads(1)

    def cpu():
        with ThreadPoolExecutor(threads) as pool:       # (ctypes releases the GIL for the call)
            assert list(pool.map(lambda i: oracle.verify_all(tables, ctls, proofs[i], chals[i], PUB), range(K))) == [0] * K
    res = {"segment": {"log_n": lg, "proof_words": int(proofs[0].size)}, "segments": K,
           "verify_segments_8": timed(lambda: verify(K)), "verify_segments_1": timed(lambda: verify(1)),
           "oracle_verify_all_8": dict(timed(cpu), kind="port", threads=threads), "prove_segments_8": timed(prove)}
    ctx.set_tuning("verify", 1)
    try:
        res["prove_segments_8_verify_key"] = timed(prove)
    finally:
        ctx.set_tuning("verify", 0)
    ctx.profile(True)
    ctx.profile_reset()
    verify(K)
    res["kernels_8"] = {k: round(ms, 4) for k, (n, ms) in sorted(ctx.profile_records().items()) if k.startswith("verify/")}
    ctx.profile(False)
    res["device_not_slower_than_cpu"] = res["verify_segments_8"]["median_ms"] <= res["oracle_verify_all_8"]["median_ms"]
    res["verify_share_of_prove"] = round(res["verify_segments_8"]["median_ms"] / res["prove_segments_8"]["median_ms"], 4)
    ctx.close()
    json.dump(res, open(os.path.join(ROOT, "profiles", "verify_time.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
