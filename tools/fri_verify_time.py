#!/usr/bin/env python3
"""tools/fri_verify_time.py -- what zkm_fri_verify costs, timed in one run on one context:
  (a) K = 1 and K = 8 proofs of the STARK instance at 2^16 rows (13 + 4 + 4 columns, batches at zeta, g zeta and 1; the standard
      configuration, 37 queries) in ONE call, against the CPU oracle's zko_verify_openings on the same blobs, one after the other, on the
      oracle's threads (the machine's CPU quota, 16 on the GPU machines).  The oracle's call also replays compact / zeta / observe_openings,
      a few dozen permutations of its hundreds;
  (b) one PLONK-shaped instance at 2^12 rows (four oracles of 7, 9, 5 and 4 columns, one batch at zeta over all of them and one at g zeta
      over two of one; standard_recursion_config: rate_bits 3, cap_height 4, arity_bits 4, final_poly_bits 5, 28 queries, 16 proof-of-work
      bits).  This instance has NO CPU baseline: the oracle restates only the STARK instance.
Each figure is the median of REPS (default 20) calls after one warm-up, with min and max, and the host waits of each call.  The claims
are prepared once (blobs, caps and openings as host arrays); a timed call is Context.fri_verify, i.e. marshalling, the host transcript
replay, one upload, the launches and one download.  Every timed call must accept.  Writes profiles/fri_verify_time.json (or OUT)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402
from oracle.oracle_py import Oracle  # noqa: E402

P = zkm_amd.P
W, A, Q, Z = 13, 4, 4, 2


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def copy_of(ch):
    return zkm_amd.Challenger.from_buffer_copy(ch)


def stark_claim(ctx, oracle, log_n, seed):
    """A prove_openings blob of random polynomials -> (the STARK blob for the oracle, its challenger seed, the FriClaim parts)"""
    import ctypes as C
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    tv, av, qc = (rng.integers(0, P, k * n, dtype=np.uint64) for k in (W, A, Q))
    tb, ab = zkm_amd.PolynomialBatch.from_values(ctx, tv, W, log_n), zkm_amd.PolynomialBatch.from_values(ctx, av, A, log_n)
    qb = zkm_amd.PolynomialBatch.from_coeffs(ctx, qc, Q, log_n)
    ch = zkm_amd.challenger_new()
    zkm_amd.challenger_observe(ch, [seed])
    blob = ctx.prove_openings(tb, ab, qb, Z, challenger=ch)
    for b in (tb, ab, qb):
        b.free()
    lay, _ = zkm_amd.proof_layout(blob)
    ch = zkm_amd.challenger_new()                     # the transcript up to the alpha draw (proof.rs:199, :336-367)
    zkm_amd.challenger_observe(ch, [seed])
    st = np.zeros(12, dtype=np.uint64)
    zkm_amd.load().zkm_challenger_compact(C.byref(ch), st.ctypes.data_as(C.POINTER(C.c_uint64)))
    zeta = (int(zkm_amd.challenger_get(ch)), int(zkm_amd.challenger_get(ch)))
    g = oracle.root_of_unity(log_n)
    sec = lambda off, words: blob[int(off):int(off) + words]
    local, aux, quot = sec(lay.local_values, 2 * W), sec(lay.aux_polys, 2 * A), sec(lay.quotient_polys_open, 2 * Q)
    nxt, aux_next = sec(lay.next_values, 2 * W), sec(lay.aux_polys_next, 2 * A)
    first = np.array([w for z in sec(lay.ctl_zs_first, Z) for w in (int(z), 0)], dtype=np.uint64)
    for words in (local, aux, quot, nxt, aux_next, first):
        zkm_amd.challenger_observe(ch, words)
    cap_words = 4 << int(lay.cap_height)
    header = np.zeros(24, dtype=np.uint64)
    header[:9] = [int.from_bytes(b"ZKMFRIPF", "little"), log_n, 3, int(lay.cap_height), int(lay.fri_layers), int(lay.final_poly_len),
                  int(lay.num_queries), int(lay.rate_bits), int(lay.arity_bits)]
    header[16:19] = [W, A, Q]
    batches = [(zeta, [(0, c) for c in range(W)] + [(1, c) for c in range(A)] + [(2, c) for c in range(Q)]),
               ((zeta[0] * g % P, zeta[1] * g % P), [(0, c) for c in range(W)] + [(1, c) for c in range(A)]), ((1, 0), [(1, c) for c in range(A - Z, A)])]
    parts = dict(proof=np.concatenate([header, blob[int(lay.commit_phase_merkle_caps):]]), log_n=log_n, oracle_cols=[W, A, Q],
                 oracle_caps=[sec(off, cap_words).copy() for off in (lay.trace_cap, lay.aux_cap, lay.quotient_cap)], batches=batches,
                 opened=[np.concatenate([local, aux, quot]), np.concatenate([nxt, aux_next]), first])
    return blob, seed, parts, ch


def plonk_claim(ctx, cfg, log_n, seed):
    cols = [7, 9, 5, 4]
    rng = np.random.default_rng(seed)
    oracles = [zkm_amd.PolynomialBatch.from_values(ctx, rng.integers(0, P, k << log_n, dtype=np.uint64), k, log_n, cfg.rate_bits, cfg.cap_height)
               for k in cols]
    g = Oracle().root_of_unity(log_n)
    zeta = (1234567, 7654321)
    batches = [(zeta, [(o, c) for o in range(4) for c in range(cols[o])]), ((zeta[0] * g % P, zeta[1] * g % P), [(2, 0), (2, 1)])]
    ch = zkm_amd.challenger_new()
    zkm_amd.challenger_observe(ch, [seed])
    ch0 = copy_of(ch)
    blob = ctx.fri_prove(oracles, batches, ch, cfg)
    opened = []
    for pt, polys in batches:
        values = {o: ctx.eval_openings(oracles[o], pt) for o in {o for o, _ in polys}}
        opened.append(np.concatenate([values[o][2 * p:2 * p + 2] for o, p in polys]))
    parts = dict(proof=blob, log_n=log_n, oracle_cols=cols, oracle_caps=[b.cap() for b in oracles], batches=batches, opened=opened)
    for b in oracles:
        b.free()
    return parts, ch0


def timed_verify(ctx, cfg, claims, reps):
    """claims = [(parts, challenger at the alpha draw)]; the median of `reps` accepted calls after one warm-up, and the calls' host waits"""
    ms, waits = [], set()
    for rep in range(reps + 1):
        dev = [zkm_amd.FriClaim(challenger=copy_of(ch), **parts) for parts, ch in claims]
        w0, t0 = ctx.host_waits(), time.perf_counter()
        reports = ctx.fri_verify(dev, cfg)
        dt = (time.perf_counter() - t0) * 1e3
        assert all(r.code == 0 for r in reports), [r.name for r in reports]
        if rep:
            ms.append(dt)
            waits.add(ctx.host_waits() - w0)
    return stats(ms), sorted(waits)


def main():
    reps = int(os.environ.get("REPS", "20"))
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "fri_verify_time.json"))
    from bench import cpu_quota
    threads = max(1, min(16, os.cpu_count() or 1, cpu_quota() or 16))
    oracle = Oracle()
    oracle.set_threads(threads)
    ctx = zkm_amd.Context(0)
    cfg = ctx.standard_config()
    out = {"about": "tools/fri_verify_time.py: Context.fri_verify (zkm_fri_verify) on K claims in one call; the CPU oracle's zko_verify_openings "
                    "on the same blobs one after the other; median of `reps` calls after one warm-up",
           "reps": reps, "oracle_threads": threads, "stark_2_16": [], "plonk_2_12": None}
    log_n = 16
    made = [stark_claim(ctx, oracle, log_n, 500 + k) for k in range(8)]
    for K in (1, 8):
        device, waits = timed_verify(ctx, cfg, [(parts, ch) for _, _, parts, ch in made[:K]], reps)
        cpu = []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            for blob, seed, _, _ in made[:K]:
                ch = oracle.challenger()
                oracle.observe(ch, [seed])
                assert oracle.verify_openings(blob, W, A, Z, challenger=ch, cfg=None) == 0
            if rep:
                cpu.append((time.perf_counter() - t0) * 1e3)
        cpu = stats(cpu)
        out["stark_2_16"].append({"K": K, "log_n": log_n, "columns": [W, A, Q], "num_queries": int(cfg.num_queries), "device_ms": device,
                                  "host_waits_per_call": waits, "cpu_oracle_ms": cpu,
                                  "cpu_over_device": round(cpu["median_ms"] / device["median_ms"], 2)})
    pcfg = ctx.standard_config()
    pcfg.rate_bits, pcfg.cap_height, pcfg.arity_bits, pcfg.final_poly_bits, pcfg.num_queries, pcfg.pow_bits = 3, 4, 4, 5, 28, 16
    device, waits = timed_verify(ctx, pcfg, [plonk_claim(ctx, pcfg, 12, 600)], reps)
    out["plonk_2_12"] = {"K": 1, "log_n": 12, "columns": [7, 9, 5, 4], "batches": 2, "rate_bits": 3, "num_queries": 28, "device_ms": device,
                         "host_waits_per_call": waits, "cpu_oracle_ms": None,
                         "note": "no CPU baseline: the oracle restates only the STARK instance"}
    ctx.close()
    text = json.dumps(out, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
