#!/usr/bin/env python3
"""tools/image_hash_time.py -- what hashing a memory image's dirty pages costs on the device (zkm_image_hash / zkm_images_hash) against
one CPU thread, timed in one run on one context, for PAGES (default 8, 16, 64, 256, 1024, 4096; 8 is there to show the side on which
the host wins) dirty pages and K (default 1, 8) images a call.  The dirty pages of an image are consecutive (N pages under ceil(N / 128) L1 pages), nothing is known: every hash page is fresh.
  call_host_ms     the whole call with the dirty pages in (pageable) host memory and the hash pages returned to host memory -- what an
                   emulator that keeps its pages on the host pays;
  call_device_ms   the whole call with the dirty pages and the hash pages in device memory;
  levels_ms        the four level launches alone (profile scope image_hash/level of a device-memory call), per lane form: "row" (a 16-lane
                   row a chain, "image_hash_form" 1), "quad" (a quad of lanes a chain, 2), and "auto" (0);
  level0_ms        the dirty pages' launch alone, per form, estimated as levels_ms minus three quarters of levels_ms of ONE dirty page (there
                   every one of the four launches is a single chain);
  cpu_ms           kind "port, 1 thread": the same pages hashed level by level on one CPU thread of the same box with the oracle's C
                   permutation (oracle/poseidon.c), one sponge after the other.  It stands in for the emulator's Rust, which does
                   not run here; its root and image id must equal the device's.
  scan             SCAN (default 4096x2, 4096x3, 4096x4, 4096x6: pages x images) more chain counts between the shapes, levels_ms and level0_ms
                   only: where the quad form overtakes the row form.
REPS (default 3) timed calls after one warm-up each; every figure as median [min, max].  CPU figures of more than CPU_FULL_REPS_CHAINS
(default 8192) chains are timed once.  Writes profiles/image_hash_time.json (or OUT) and prints it."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402
from bench import code_fingerprint  # noqa: E402
from oracle.oracle_py import Oracle  # noqa: E402

LIBRARY_ROW_MAX_CHAINS = 8192          # zkm_ctx::image_hash_row_max (csrc/zkm_internal.h), set from this tool's scan
PAD = np.array([1, 0, 0, 0, 0, 0, 0, 0x80000000], dtype=np.uint64)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


class CpuPort:
    """update_page_hash + compute_image_id on numpy arrays; every sponge is one call of the oracle's scalar C code (zko_poseidon_hash_no_pad
    over the page's words and the padding block: overwrite mode, eight words a permutation), one after the other on the calling thread."""

    def __init__(self, oracle):
        self.fn = oracle.lib.zko_poseidon_hash_no_pad
        self.consts, page = [], np.zeros((1, 1024), dtype=np.uint32)
        for _ in range(3):
            d = self.hash_pages(page)[0]
            self.consts.append(d)
            page = np.tile(d, 128)[None, :]

    def sponges(self, elems):
        """elems: n x m uint64, m a multiple of 8 -> n x 4 digests"""
        elems = np.ascontiguousarray(elems, dtype=np.uint64)
        n, m = elems.shape
        out = np.zeros((n, 4), dtype=np.uint64)
        src, dst = elems.ctypes.data, out.ctypes.data
        for i in range(n):
            self.fn(C.c_void_p(src + 8 * m * i), C.c_size_t(m), C.c_void_p(dst + 32 * i))
        return out

    def hash_pages(self, pages):
        n = len(pages)
        elems = np.empty((n, 1032), dtype=np.uint64)
        elems[:, :1024] = pages
        elems[:, 1024:] = PAD
        return self.sponges(elems).view(np.uint32).reshape(n, 8)

    def split(self, idx, words, pc, registers):
        """(root bytes, image id bytes) of a memory with no hash pages yet."""
        level_idx, level_words = np.asarray(idx, dtype=np.int64), words
        for level in range(3):
            digests = self.hash_pages(level_words)
            addr = 0x80000000 + (level_idx << 5)
            parent, slot = addr >> 12, (addr & 0xFFF) >> 5
            level_idx, pos = np.unique(parent, return_inverse=True)
            level_words = np.tile(self.consts[level], (len(level_idx), 128)).reshape(len(level_idx), 128, 8)
            level_words[pos, slot] = digests
            level_words = level_words.reshape(len(level_idx), 1024)
        level_words[0, 256:256 + 39] = np.frombuffer(registers, dtype="<u4")
        root = self.hash_pages(level_words)[0]
        final = np.concatenate([root.byteswap().astype(np.uint64), [pc, 1, 0, 0, 0, 0, 0, 0x80000000]]).astype(np.uint64)
        return root.tobytes(), self.sponges(final[None, :])[0].tobytes()


def summarise(result):
    """The three figures the shapes are measured for: from which page count the device call beats the CPU thread (and where the host
    is faster), where the quad form overtakes the row form, and whether the library's automatic choice (the row form up to
    LIBRARY_ROW_MAX_CHAINS chains of a level, zkm_ctx::image_hash_row_max) is the faster form at every measured chain count."""
    k1 = [s for s in result["shapes"] if s["K"] == 1]
    result["device_call_first_beats_cpu_thread_at_pages"] = next((s["pages"] for s in k1 if s["device_faster_than_cpu"]), None)
    result["host_faster_at_pages"] = [s["pages"] for s in k1 if not s["device_faster_than_cpu"]]
    by_chains = sorted(result["shapes"] + result["scan"], key=lambda s: s["chains_level0"])
    result["quad_form_first_faster_at_chains"] = next((s["chains_level0"] for s in by_chains if s["level0_ms"]["quad"] < s["level0_ms"]["row"]), None)
    result["row_form_last_faster_at_chains"] = max((s["chains_level0"] for s in by_chains if s["level0_ms"]["row"] <= s["level0_ms"]["quad"]), default=None)
    result["automatic_form_switches_above_chains"] = LIBRARY_ROW_MAX_CHAINS
    result["automatic_form_within_3_percent_of_the_faster_everywhere"] = all(
        s["levels_ms"]["auto"]["median_ms"] <= 1.03 * min(s["levels_ms"]["row"]["median_ms"], s["levels_ms"]["quad"]["median_ms"]) for s in by_chains)


def to_device(ctx, a):
    a = np.ascontiguousarray(a).reshape(-1)
    return ctx.alloc(a.nbytes // 8).upload(a.view(np.uint64))


def main():
    pages = [int(x) for x in os.environ.get("PAGES", "8,16,64,256,1024,4096").split(",")]
    ks = [int(x) for x in os.environ.get("K", "1,8").split(",")]
    reps = int(os.environ.get("REPS", "3"))
    scan = [tuple(int(v) for v in x.split("x")) for x in os.environ.get("SCAN", "4096x2,4096x3,4096x4,4096x6").split(",") if x]
    cpu_full = int(os.environ.get("CPU_FULL_REPS_CHAINS", "8192"))
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "image_hash_time.json"))
    oracle = Oracle()
    oracle.set_threads(1)
    cpu = CpuPort(oracle)
    ctx = zkm_amd.Context(0)
    rng = np.random.default_rng(7)
    registers = bytes(range(156))
    result = {"about": "tools/image_hash_time.py: zkm_image[s]_hash against one CPU thread (kind: port, 1 thread -- the oracle's C permutation, "
                       "not the emulator's Rust); median [min, max] of `reps` calls", "code_fingerprint": code_fingerprint(), "reps": reps,
              "shapes": [], "scan": []}

    def levels(images, outs, form):
        ctx.set_tuning("image_hash_form", form)
        try:
            ctx.images_hash(images, outs=outs)
            ms = []
            for _ in range(reps):
                ctx.profile_reset()
                ctx.images_hash(images, outs=outs)
                ms.append(ctx.profile_records()["image_hash/level"][1])
        finally:
            ctx.set_tuning("image_hash_form", 0)
        return ms

    def wall(fn):
        fn()
        ms = []
        for _ in range(reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    one = {}
    for n, k, full in [(1, 1, True)] + [(n, k, True) for n in pages for k in ks] + [(n, k, False) for n, k in scan]:
        idx = [np.arange(0x8000 * (m + 1), 0x8000 * (m + 1) + n, dtype=np.uint32) for m in range(k)]
        words = [rng.integers(0, 1 << 32, (n, 1024), dtype=np.uint64).astype(np.uint32) for _ in range(k)]
        nplan = len(zkm_amd.image_hash_plan(idx[0]))
        host = [((idx[m], words[m]), None, 0x1000 + m, registers) for m in range(k)]
        dwords, douts = [to_device(ctx, w) for w in words], [ctx.alloc(nplan * 512) for _ in range(k)]
        dev = [((idx[m], dwords[m]), None, 0x1000 + m, registers) for m in range(k)]
        if full:
            t_host = wall(lambda: ctx.images_hash(host))
            t_dev = wall(lambda: ctx.images_hash(dev, outs=douts))
            got = ctx.images_hash(host)
        ctx.profile(True)
        lv = {name: levels(dev, douts, form) for name, form in (("row", 1), ("quad", 2), ("auto", 0))}
        ctx.profile(False)
        for b in dwords + douts:
            b.free()
        if n == 1:
            one = {f: float(np.median(v)) for f, v in lv.items()}
            result["one_page_levels_ms"] = {f: stats(v) for f, v in lv.items()}
            continue
        level0 = {f: round(float(np.median(lv[f])) - 0.75 * one[f], 3) for f in ("row", "quad")}
        if not full:
            result["scan"].append({"pages": n, "K": k, "chains_level0": n * k, "levels_ms": {f: stats(v) for f, v in lv.items()},
                                   "level0_ms": level0})
            print(json.dumps(result["scan"][-1]), flush=True)
            continue
        t_cpu = []
        for _ in range(reps if n * k <= cpu_full else 1):
            t0 = time.perf_counter()
            want = [cpu.split(idx[m], words[m], 0x1000 + m, registers) for m in range(k)]
            t_cpu.append((time.perf_counter() - t0) * 1e3)
        assert [(g[2], g[3]) for g in got] == want, "the device and the CPU port disagree"
        shape = {"pages": n, "K": k, "chains_level0": n * k, "plan_pages_per_image": nplan, "call_host_ms": stats(t_host),
                 "call_device_ms": stats(t_dev), "levels_ms": {f: stats(v) for f, v in lv.items()},
                 "level0_ms": level0, "cpu_ms": dict(stats(t_cpu), kind="port, 1 thread"),
                 "cpu_us_per_permutation": round(float(np.median(t_cpu)) * 1e3 / (k * ((n + nplan) * 129 + 2)), 2),
                 "device_faster_than_cpu": float(np.median(t_host)) < float(np.median(t_cpu))}
        result["shapes"].append(shape)
        print(json.dumps(shape), flush=True)
    summarise(result)
    ctx.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
