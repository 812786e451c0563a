"""CPU suite: the three exports of the I/O calls' expansion (include/zkm_hip.h "the I/O syscalls' rows from their bytes") as far as they
need no GPU -- declared alike everywhere, the four kinds' constants with one value in the header, the binding and the Rust block, the
counts, the RAW records and clocks of zkm_io_calls_steps against the model, and every refusal with the list and the call it names;
zkm_io_calls_witness makes the same refusals before it misses its context."""
import ctypes as C
import re

import numpy as np
import pytest

from . import io_calls_model as IO
from .test_abi import declared_alike, prototypes, read

NEW = ["zkm_io_calls_counts", "zkm_io_calls_steps", "zkm_io_calls_witness"]
LENGTHS = (0, 1, 3, 4, 5, 32, 33, 36, 64, 68)
MAP = IO.PREIMAGE_MAP


def test_symbols_are_exported_and_declared_alike(zkm):
    protos = prototypes()
    for fn in NEW:
        declared_alike(zkm, fn)
    assert protos["zkm_io_calls_witness"][1][0] == ("zkm_ctx*", "ctx")
    assert all(ty != "zkm_ctx*" for fn in NEW[:2] for ty, _ in protos[fn][1])          # pure: no context
    for method in ("io_calls_witness", "io_calls_witness_into", "calls_expand"):
        assert callable(getattr(zkm.Context, method))
    assert callable(zkm.io_calls_counts) and callable(zkm.io_calls_steps)
    import inspect
    assert inspect.signature(zkm.Context.calls_expand).parameters["io"].default is None
    assert "io_calls.hip" in read("zkm_amd", "csrc", "Makefile")


def test_the_kinds_have_one_value_everywhere(zkm):
    want = {"hint_read": 0, "commit": 1, "verify": 2, "preimage": 3}
    assert zkm.IO_KINDS == want == IO.KINDS
    assert {k: v for k, v in zkm.abi.constants().items() if k.startswith("ZKM_IO_")} == {"ZKM_IO_" + k.upper(): v for k, v in want.items()}
    rust = re.sub(r"//[^\n]*", "", read("integration", "rust", "zkm_hip_sys.rs"))
    assert {n: int(v) for n, v in re.findall(r"pub const ZKM_IO_(\w+): u32 = (\w+);", rust)} == {k.upper(): v for k, v in want.items()}
    # no step kind and no SYSCALL sub-kind came with them
    assert len(zkm.STEP_KINDS) == 29 and 4 not in zkm.SYSCALL_KINDS.values()


def offsets(lengths, first=0):
    return (first + np.cumsum([0] + list(lengths))).astype(np.uint64)


def good_meta(kind, k=0):
    return (0, 0, MAP if kind == IO.PREIMAGE else 0x10000 + 0x1000 * k, 10 * (200 + 100 * k))


def data_length(kind, L):
    """The bytes a call of `kind` hands over for the length L of the issue's list: a hint read L itself, a commit its whole words, a
    verify its 32, a preimage the hash in front of L content bytes."""
    return {IO.HINT_READ: L, IO.COMMIT: (L + 3) // 4 * 4, IO.VERIFY: 32, IO.PREIMAGE: 32 + L}[kind]


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("kind", sorted(IO.KINDS.values()), ids=sorted(IO.KINDS, key=IO.KINDS.get))
def test_counts_records_masks_and_clocks_of_one_call(zkm, kind, L):
    n = data_length(kind, L)
    kinds, off, meta = np.array([kind], dtype=np.uint32), offsets([n], first=12), np.array([good_meta(kind)], dtype=np.uint64)
    x = IO.Expansion()
    x.call(kind, bytes(n), meta[0])
    assert zkm.io_calls_counts(kinds, off) == (len(x.rows), x.memory_ops())
    steps, clocks = zkm.io_calls_steps(kinds, off, meta, raw_base=5)
    assert clocks.tolist() == list(range(200, 200 + len(x.rows))) == x.clocks
    assert steps["reads"][:, 1].tolist() == x.masks
    assert steps["reads"][:, 0].tolist() == list(range(5, 5 + len(x.rows))) and (steps["kind"] == zkm.STEP["RAW"]).all()
    assert not steps["reads"][:, 2:].any() and not any(steps[f].any() for f in ("pc", "next_pc", "insn", "flags", "context"))
    want_steps, want_clocks = IO.steps(x, raw_base=5)
    assert steps.tobytes() == want_steps.tobytes() and (clocks == want_clocks).all()
    # the counts by their formulas, independent of the model's loops
    W = {IO.HINT_READ: (L + 3) // 4, IO.COMMIT: (L + 3) // 4, IO.VERIFY: 8, IO.PREIMAGE: 1 + (L + 3) // 4}[kind]
    lead = 1 if kind == IO.PREIMAGE else 0
    assert zkm.io_calls_counts(kinds, off) == (lead + max(1, (W + 7) // 8), 8 * lead + W)


def test_four_calls_of_the_four_kinds(zkm):
    calls = [(IO.HINT_READ, bytes(37), good_meta(IO.HINT_READ, 0)), (IO.COMMIT, bytes(36), good_meta(IO.COMMIT, 1)),
             (IO.VERIFY, bytes(32), good_meta(IO.VERIFY, 2)), (IO.PREIMAGE, bytes(32 + 29), good_meta(IO.PREIMAGE, 3))]
    kinds, data, off, meta = IO.lists(calls)
    assert zkm.io_calls_counts(kinds, off) == (2 + 2 + 1 + 3, 10 + 9 + 8 + 8 + 9)
    steps, clocks = zkm.io_calls_steps(kinds, off, meta, raw_base=2)
    x = IO.expand(kinds, data, off, meta)
    want_steps, want_clocks = IO.steps(x, raw_base=2)
    assert len(steps) == 8 and steps.tobytes() == want_steps.tobytes() and (clocks == want_clocks).all()
    assert clocks.tolist() == [200, 201, 300, 301, 400, 500, 501, 502]
    assert steps["reads"][:, 1].tolist() == [0xFF, 0x03, 0xFF, 0x01, 0xFF, 0xFF, 0xFF, 0x01]
    L = zkm.load()
    assert L.zkm_io_calls_counts(kinds.ctypes.data, off.ctypes.data, 4, None, None, None) == 0      # any out pointer may be NULL
    assert zkm.io_calls_counts([], [0]) == (0, 0)


GOOD = (0, 0, 0x1000, 100)


def meta_(**kw):
    m = list(GOOD)
    for k, v in kw.items():
        m[("context", "segment", "address", "timestamp").index(k)] = v
    return tuple(m)


H, CM, V, P = IO.HINT_READ, IO.COMMIT, IO.VERIFY, IO.PREIMAGE
# (the list named, kind of the bad call (call 1), lengths of the three calls, the bad call's meta, the message behind "<list>: call 1: ")
REFUSED = [
    ("kinds", 4, [8, 8, 8], GOOD, r"unknown kind 4"),
    ("kinds", 0xFFFFFFFF, [8, 8, 8], GOOD, r"unknown kind 4294967295"),
    ("data_off", H, [8, -4, 8], GOOD, r"the offsets decrease \(8 then 4\)"),
    ("data_off", V, [8, 31, 8], GOOD, r"a verify call of 31 bytes \(the claim digest is 32\)"),
    ("data_off", V, [8, 36, 8], GOOD, r"a verify call of 36 bytes"),
    ("data_off", CM, [8, 6, 8], GOOD, r"a commit call of 6 bytes is not a multiple of 4"),
    ("data_off", P, [8, 31, 8], meta_(address=MAP), r"a preimage call of 31 bytes is shorter than its 32 hash bytes"),
    ("meta", P, [8, 40, 8], meta_(address=MAP + 4), r"address 0x31000004 of a preimage call is not 0x31000000"),
    ("meta", H, [8, 8, 8], meta_(address=0x1002), r"address 0x1002 is not aligned to 4 bytes"),
    ("meta", CM, [8, 8, 8], meta_(address=0x1001), r"address 0x1001 is not aligned to 4 bytes"),
    ("meta", V, [8, 32, 8], meta_(address=0x1003), r"address 0x1003 is not aligned to 4 bytes"),
    ("meta", H, [8, 9, 8], meta_(address=0xFFFFFFF8), r"address 0xfffffff8: the last word of the hint read \(3 words\) does not fit in 32 bits"),
    ("meta", CM, [8, 12, 8], meta_(address=0xFFFFFFF8), r"address 0xfffffff8: the last word of the commit \(3 words\) does not fit in 32 bits"),
    ("meta", V, [8, 32, 8], meta_(address=0xFFFFFFE4), r"address 0xffffffe4: the last word of the verify \(8 words\) does not fit in 32 bits"),
    ("meta", H, [8, 0, 8], meta_(address=1 << 32), r"address 0x100000000: the last word of the hint read \(0 words\) does not fit in 32 bits"),
    ("meta", H, [8, 8, 8], meta_(context=1 << 32), r"context 4294967296 does not fit in 32 bits"),
    ("meta", H, [8, 8, 8], meta_(segment=1 << 40), r"segment 1099511627776 does not fit in 32 bits"),
    ("meta", H, [8, 8, 8], meta_(timestamp=105), r"timestamp 105 is not a multiple of 10 \(NUM_CHANNELS\)"),
]


def witness_without_context(zkm, kinds, off, meta, data=True, out=True):
    """zkm_io_calls_witness with no context: the message it fails with."""
    L = zkm.load()
    n = len(kinds)
    bytes_ = np.zeros(8, dtype=np.uint8)             # never read,
    rows = np.zeros(8, dtype=np.uint64)              # never written: the call fails on the host
    err = C.c_char_p()
    assert L.zkm_io_calls_witness(None, kinds.ctypes.data if n else None, bytes_.ctypes.data if data else None, off.ctypes.data if n else None,
                                  meta.ctypes.data if n else None, n, rows.ctypes.data if out else None, C.byref(err)) == 1
    return err.value.decode()


@pytest.mark.parametrize("which,kind,lengths,bad,message", REFUSED, ids=["%s-%d" % (r[0], i) for i, r in enumerate(REFUSED)])
def test_every_refusal_names_the_list_and_the_call(zkm, which, kind, lengths, bad, message):
    kinds = np.array([H, kind, H], dtype=np.uint32)
    off = offsets(lengths)
    meta = np.array([GOOD, bad, GOOD], dtype=np.uint64)
    at = "%s: call 1: " % which
    # (the export itself: the binding sizes its buffers with zkm_io_calls_counts, which refuses the kinds and the offsets first)
    steps, clocks, err = np.zeros(64, dtype=zkm.CPU_STEP_DT), np.zeros(64, dtype=np.uint64), C.c_char_p()
    assert zkm.load().zkm_io_calls_steps(kinds.ctypes.data, off.ctypes.data, meta.ctypes.data, 3, 0, steps.ctypes.data, clocks.ctypes.data, C.byref(err)) == 1
    assert re.match("^zkm_io_calls_steps: " + at + message, err.value.decode()), err.value
    assert not steps["kind"].any()
    with pytest.raises(zkm.ZkmError, match="^zkm_io_calls_(steps|counts): " + at + message):
        zkm.io_calls_steps(kinds, off, meta)
    assert re.match("^zkm_io_calls_witness: " + at + message, witness_without_context(zkm, kinds, off, meta))
    if which != "meta":
        with pytest.raises(zkm.ZkmError, match="^zkm_io_calls_counts: " + at + message):
            zkm.io_calls_counts(kinds, off)


def test_the_boundaries_are_accepted(zkm):
    """The highest addresses that fit, timestamp 0, the largest context and segment."""
    top = 0xFFFFFFFF
    kinds = np.array([H, CM, V, H, P], dtype=np.uint32)
    off = offsets([9, 12, 32, 0, 32 + 5])
    meta = np.array([(top, top, 0xFFFFFFF4, 0), (top, top, 0xFFFFFFF4, 10), (top, top, 0xFFFFFFE0, 20), (top, top, 0xFFFFFFFC, 30), (top, top, MAP, 40)],
                    dtype=np.uint64)
    steps, clocks = zkm.io_calls_steps(kinds, off, meta)
    assert clocks.tolist() == [0, 1, 2, 3, 4, 5] and steps["reads"][:, 1].tolist() == [7, 7, 0xFF, 0, 0xFF, 7]
    assert witness_without_context(zkm, kinds, off, meta) == "zkm_io_calls_witness: null argument"
    for k in range(3):
        bad = meta.copy()
        bad[k, 2] += 4
        assert ("meta: call %d: address " % k) in witness_without_context(zkm, kinds, off, bad)
    # the largest preimage whose last word fits: Q words from 0x31000000 to 0xFFFFFFFC; one word more does not
    q = (0x100000000 - MAP) // 4
    fits = np.array([0, 32 + 4 * (q - 1)], dtype=np.uint64)
    one, m = np.array([P], dtype=np.uint32), np.array([(0, 0, MAP, 0)], dtype=np.uint64)
    assert zkm.io_calls_counts(one, fits) == (1 + q // 8, 8 + q)
    assert witness_without_context(zkm, one, fits, m, data=False) == "zkm_io_calls_witness: data: NULL with %d bytes to read" % int(fits[1])
    fits[1] += 1
    assert witness_without_context(zkm, one, fits, m) == \
        "zkm_io_calls_witness: meta: call 0: address 0x31000000: the last word of the preimage (%d words) does not fit in 32 bits" % (q + 1)


def test_null_lists_outputs_and_raw_base(zkm):
    L = zkm.load()
    err = C.c_char_p()
    kinds, off = np.array([H, CM], dtype=np.uint32), offsets([37, 68])
    meta = np.array([GOOD, meta_(timestamp=300)], dtype=np.uint64)
    steps, clocks = np.zeros(10, dtype=zkm.CPU_STEP_DT), np.zeros(10, dtype=np.uint64)
    k, o, m, s, c = kinds.ctypes.data, off.ctypes.data, meta.ctypes.data, steps.ctypes.data, clocks.ctypes.data
    assert L.zkm_io_calls_counts(None, o, 2, None, None, C.byref(err)) == 1
    assert err.value == b"zkm_io_calls_counts: kinds: NULL with a count of 2"
    assert L.zkm_io_calls_counts(k, None, 2, None, None, C.byref(err)) == 1
    assert err.value == b"zkm_io_calls_counts: data_off: NULL with a count of 2"
    assert L.zkm_io_calls_steps(None, o, m, 2, 0, s, c, C.byref(err)) == 1
    assert err.value == b"zkm_io_calls_steps: kinds: NULL with a count of 2"
    assert L.zkm_io_calls_steps(k, None, m, 2, 0, s, c, C.byref(err)) == 1
    assert err.value == b"zkm_io_calls_steps: data_off: NULL with a count of 2"
    assert L.zkm_io_calls_steps(k, o, None, 2, 0, s, c, C.byref(err)) == 1
    assert err.value == b"zkm_io_calls_steps: meta: NULL with a count of 2"
    assert L.zkm_io_calls_steps(k, o, m, 2, 0, None, c, C.byref(err)) == 1
    assert err.value == b"zkm_io_calls_steps: null argument"
    assert L.zkm_io_calls_steps(k, o, m, 2, 0, s, None, C.byref(err)) == 1
    assert err.value == b"zkm_io_calls_steps: null argument"
    assert L.zkm_io_calls_steps(k, o, m, 2, (1 << 32) - 4, s, c, C.byref(err)) == 1
    assert b"raw_base 4294967292: a RAW index does not fit in 32 bits" in err.value
    assert L.zkm_io_calls_steps(k, o, m, 2, (1 << 32) - 5, s, c, C.byref(err)) == 0          # 2 + 3 rows: the last index is 2^32 - 1
    assert L.zkm_io_calls_steps(None, None, None, 0, 0, None, None, None) == 0
    # the witness call: lists and the output, all before the missing context
    data, out = np.zeros(105, dtype=np.uint8), np.zeros(8, dtype=np.uint64)
    p = out.ctypes.data
    args = [None, k, data.ctypes.data, o, m, 2, p]
    for pos, message in ((1, b"kinds: NULL with a count of 2"), (2, b"data: NULL with 105 bytes to read"), (3, b"data_off: NULL with a count of 2"),
                         (4, b"meta: NULL with a count of 2"), (6, b"raw_rows_out_dev: NULL with 5 rows to write")):
        bad = list(args)
        bad[pos] = None
        assert L.zkm_io_calls_witness(*bad, C.byref(err)) == 1
        assert err.value == b"zkm_io_calls_witness: " + message, err.value
    bad = list(args)
    bad[6] = p + 4                                                          # an output that is not aligned to its words
    assert L.zkm_io_calls_witness(*bad, C.byref(err)) == 1 and err.value == b"zkm_io_calls_witness: raw_rows_out_dev is not aligned to its words (8 bytes)"
    # nothing to refuse: the missing context is what is left
    assert L.zkm_io_calls_witness(*args, C.byref(err)) == 1 and err.value == b"zkm_io_calls_witness: null argument"
    assert L.zkm_io_calls_witness(None, None, None, None, None, 0, None, C.byref(err)) == 1
    assert err.value == b"zkm_io_calls_witness: null argument"
    # calls that hold no byte need no data
    empty = np.array([H, CM], dtype=np.uint32), offsets([0, 0])
    assert L.zkm_io_calls_witness(None, empty[0].ctypes.data, None, empty[1].ctypes.data, m, 2, p, C.byref(err)) == 1
    assert err.value == b"zkm_io_calls_witness: null argument"


def test_the_rust_recorder_calls_the_three_exports_as_declared(zkm):
    """integration/rust/io_calls_hip.rs (uncompiled here): every library call passes as many arguments as the header declares, the
    recorder's entry points are the ones INTEGRATION.md shows, and every kind is recorded under its constant."""
    from .test_rust_names import call_arities, fn_arity, strip_comments
    src = strip_comments(read("integration", "rust", "io_calls_hip.rs"))
    protos = prototypes()
    for fn in NEW + ["zkm_dev_alloc", "zkm_dev_upload"]:
        assert call_arities(src, fn) and set(call_arities(src, fn)) == {len(protos[fn][1])}, fn
    for name in ("ZKM_IO_HINT_READ", "ZKM_IO_COMMIT", "ZKM_IO_VERIFY", "ZKM_IO_PREIMAGE", "ZKM_STEP_RAW"):
        assert name in src, name
    assert [fn_arity(src, f) for f in ("record_hint_read", "record_commit", "record_verify", "record_preimage", "finish")] == [4, 4, 4, 4, 2]      # (self aside)
    integ = read("INTEGRATION.md")
    for call in ("record_preimage(&mut state.step_log, clock, &hash_bytes, &content)", "record_hint_read(&mut state.step_log, clock, addr, &vec)",
                 "record_verify(&mut state.step_log, clock, addr, &claim_digest)", "record_commit(&mut state.step_log, clock, addr, &words)",
                 "io_log.finish(ctx, &mut state.step_log)"):
        assert call in integ, call
