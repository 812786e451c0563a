#!/usr/bin/env python3
"""tools/boot_time.py -- what building a segment's bootstrap kernel on the device from its image costs against uploading it as lists,
timed in one run on one context, for images of PAGES (default 16, 64, 256) data pages and K (default 1, 8) segments a call:
  (a) zkm_segments_tables_boot: the image (8 bytes a word) and what simulate_cpu pushed, from pinned memory;
  (b) zkm_segments_tables on the bootstrap's prebuilt lists joined with the same few operations on the host, from pinned memory --
      the only path without the *_boot calls.  The time to GENERATE those lists on the host is not in (b): the reference's Rust does not
      run here, the lists are what zkm_boot_witness wrote (tests/test_gpu_boot.py holds them to the model word for word).  The
      PoseidonSponge table of (b) is NOT the reference's: zkm_segment_ops reads word i of a sponge operation at virt_base + i, the
      bootstrap's addresses step by 4.  Only the time is comparable;
  (c) the chain kernel alone (profile scope of a zkm_boot_witness call), permutation across a 16-lane row and across a quad;
  (d) call (a) on a profiled context, which keeps the chains on the compute stream: (d) - (a) is what the side stream hides.
REPS (default 3) timed calls after one warm-up each, (a) and (b) alternating; every figure with its min and max.  The images are
self-consistent (hash words, root and image id computed by the device in two unchecked passes) and the timed calls check them.
Writes profiles/boot_time.json (or OUT) and prints it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402

HASH_BASE, ROOT_PAGE = 0x80000000, 0x81020000


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def pinned(ctx, a):
    p = ctx.pinned_array((a.nbytes + 7) // 8)
    p.view(np.uint8)[:a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return p.view(a.dtype)[:a.size]


def make_image(ctx, npages, seed):
    """A checked BootImage of npages full data pages below 0x80000000 (none whose hash words would start a page of their own), their
    hash words, and a root page of five words."""
    rng = np.random.default_rng(seed)
    numbers = [n for n in range(0x7FE00, 0x80000) if n % 128][-npages:]
    image = {}
    for n in numbers:
        image.update(zip(range(n << 12, (n + 1) << 12, 4), (int(v) for v in rng.integers(0, 1 << 32, 1024, dtype=np.uint64))))
        image.update({HASH_BASE + (n << 5) + 4 * i: 0 for i in range(8)})
    image.update({ROOT_PAGE + 4 * i: 0x1000 + i for i in range(5)})
    entry = 0x00401000
    digests = ctx.boot_witness(zkm_amd.BootImage.from_dict(image, bytes(32), bytes(32), entry, check=False))[4]
    for n, d in zip(numbers, digests):
        image.update({HASH_BASE + (n << 5) + 4 * i: int(w) for i, w in enumerate(d.view(np.uint32))})
    root = digests[len(numbers)].tobytes()
    image_id = ctx.boot_witness(zkm_amd.BootImage.from_dict(image, root, bytes(32), entry, check=False))[4][-1].tobytes()
    addrs = sorted(image)
    return zkm_amd.BootImage(pinned(ctx, np.array(addrs, dtype=np.uint32)), pinned(ctx, np.array([image[a] for a in addrs], dtype=np.uint32)),
                             root, image_id, entry, check=True)


def exec_lists(nboot):
    """What simulate_cpu pushed, kept tiny: zero CPU rows up to the next power of two and three memory operations."""
    rows = (1 << int(nboot).bit_length()) - nboot
    mem = np.array([[0, 4, 5, 10 * nboot, 0, 7], [0, 4, 5, 10 * nboot + 10, 1, 7], [0, 4, 9, 10 * nboot + 20, 0, 11]], dtype=np.uint64)
    return np.zeros((rows, 259), dtype=np.uint64), mem


def main():
    pages = [int(x) for x in os.environ.get("PAGES", "16,64,256").split(",")]
    ks = [int(x) for x in os.environ.get("K", "1,8").split(",")]
    reps = int(os.environ.get("REPS", "3"))
    out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "boot_time.json"))
    ctx = zkm_amd.Context(0)
    result = {"about": "tools/boot_time.py: (a) zkm_segments_tables_boot from the image, (b) zkm_segments_tables on the bootstrap's prebuilt "
                       "lists (host generation time not included; its PoseidonSponge table is not the reference's), (c) the chain kernel alone",
              "reps": reps, "shapes": []}
    for npages in pages:
        im = make_image(ctx, npages, seed=npages)
        nboot, nmem, npo, nops, _ = im.counts()
        cpu, mem = exec_lists(nboot)
        exec_ops = zkm_amd.SegmentOps(cpu, mem).to_pinned(ctx)
        # (c) and the lists of (b), from the kernels alone
        ctx.profile(True)
        chain = {}
        for quad, scope in ((0, "bootstrap/chain_row"), (1, "bootstrap/chain_quad")):
            ctx.set_tuning("boot_chain_quad", quad)
            lists = ctx.boot_witness(im)                      # warm-up (and the lists themselves)
            ms = []
            for _ in range(reps):
                ctx.profile_reset()
                ctx.boot_witness(im)
                ms.append(ctx.profile_records()[scope][1])
            chain[scope.split("_")[-1]] = stats(ms)
        ctx.set_tuning("boot_chain_quad", 0)
        ctx.profile(False)
        b_rows, b_mem, b_po, b_ts, _ = lists
        words = np.zeros((nops, 1024), dtype=np.uint32)       # the sponge operations in the contiguous-address form: their bytes
        page_addr = im.addrs[(im.addrs & 0xFFF) == 0]
        for c, a in enumerate(page_addr):
            lo = np.searchsorted(im.addrs, a)
            sel = im.addrs[lo:lo + 1024]
            sel = sel[sel < int(a) + 4096]
            words[c, (sel - a) // 4] = im.values[lo:lo + sel.size]
        words[nops - 1, :8] = np.frombuffer(im.root, dtype=">u4")
        words[nops - 1, 8] = im.entry
        lens = np.array([4096] * (nops - 1) + [36], dtype=np.uint64)
        sp_bytes = np.concatenate([words[c].view(np.uint8)[:int(lens[c])] for c in range(nops)])
        sp_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        sp_meta = np.zeros((nops, 4), dtype=np.uint64)
        sp_meta[:, 2] = list(page_addr) + [0x81021000]
        sp_meta[:, 3] = [10 * (nboot - 3 - (nops - 1) + c) for c in range(nops - 1)] + [10 * (nboot - 1)]
        joined = zkm_amd.SegmentOps(np.concatenate([b_rows, cpu]), np.concatenate([b_mem, mem]), poseidon=(b_po, b_ts),
                                    poseidon_sponge=(sp_bytes, sp_off, sp_meta)).to_pinned(ctx)
        bytes_a = int(im.addrs.nbytes + im.values.nbytes + cpu.nbytes + mem.nbytes)
        bytes_b = int(sum(v.nbytes for v in joined.lists.values()))
        for k in ks:
            def run_a():
                for st, _ in ctx.segments_tables_boot([im] * k, [exec_ops] * k):
                    st.free()

            def run_b():
                for st, _ in ctx.segments_tables([joined] * k):
                    st.free()
            heights_a = ctx.segment_tables_boot(im, exec_ops, sizing=True)
            heights_b = ctx.segment_heights(joined)
            assert heights_a == heights_b, (heights_a, heights_b)
            run_a()
            run_b()
            ta, tb = [], []
            for _ in range(reps):                              # alternating: both see the same neighbours on the machine
                for fn, acc in ((run_a, ta), (run_b, tb)):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    ctx.synchronize()
                    acc.append((time.perf_counter() - t0) * 1e3)
            ctx.profile(True)                                  # profiled, the chains stay on the compute stream: the same call, nothing overlapped
            run_a()
            tser = []
            for _ in range(reps):
                ctx.profile_reset()
                ctx.synchronize()
                t0 = time.perf_counter()
                run_a()
                ctx.synchronize()
                tser.append((time.perf_counter() - t0) * 1e3)
            chain_in_call = ctx.profile_records()["bootstrap/chain_row"][1]
            ctx.profile(False)
            a, b, ser = stats(ta), stats(tb), stats(tser)
            result["shapes"].append({
                "pages": npages, "K": k, "boot_cpu_rows": nboot, "boot_memory_ops": nmem, "boot_poseidon_inputs": npo, "log_heights": heights_a,
                "a_image_ms": a, "b_lists_ms": b, "a_bytes_uploaded_per_segment": bytes_a, "b_bytes_uploaded_per_segment": bytes_b,
                "a_not_slower": a["median_ms"] <= b["median_ms"], "a_max_below_b_min": a["max_ms"] <= b["min_ms"],
                "chain_alone_ms": chain, "chain_share_of_a": round(chain["row"]["median_ms"] / a["median_ms"], 3),
                # the overlap: the same call with the chains on the compute stream (a profiled context; its event records are in the
                # figure), the chains' launch in that call (all K segments' chains), and how much of it the side stream hides
                "a_chain_serial_ms": ser, "chain_in_call_ms": round(chain_in_call, 3),
                "chain_hidden_ms": round(ser["median_ms"] - a["median_ms"], 3),
                "chain_hidden_share": round((ser["median_ms"] - a["median_ms"]) / chain_in_call, 3)})
            print(json.dumps(result["shapes"][-1]), flush=True)
    result["chain_form_adopted"] = "row" if all(s["chain_alone_ms"]["row"]["median_ms"] <= s["chain_alone_ms"]["quad"]["median_ms"]
                                                for s in result["shapes"]) else "see chain_alone_ms"
    ctx.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
