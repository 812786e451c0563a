"""CPU suite: the three exports of the SYSKECCAK precompile expansion (include/zkm_hip.h "SYSKECCAK precompile calls from their input
bytes") as far as they need no GPU -- declared alike everywhere, the counts, the RAW records and clocks of zkm_keccak_calls_steps against
the model, and every refusal with the list and the call it names; zkm_keccak_calls_witness makes the same refusals before it misses its
context."""
import ctypes as C
import re

import numpy as np
import pytest

from . import keccak_calls_model as K
from .test_abi import declared_alike, prototypes, read

NEW = ["zkm_keccak_calls_counts", "zkm_keccak_calls_steps", "zkm_keccak_calls_witness"]
FLAG = K.FLAG


def test_symbols_are_exported_and_declared_alike(zkm):
    protos = prototypes()
    for fn in NEW:
        declared_alike(zkm, fn)
    assert protos["zkm_keccak_calls_witness"][1][0] == ("zkm_ctx*", "ctx")
    assert all(ty != "zkm_ctx*" for fn in NEW[:2] for ty, _ in protos[fn][1])          # pure: no context
    for method in ("keccak_calls_witness", "keccak_calls_witness_into", "calls_expand", "sha_calls_expand"):
        assert callable(getattr(zkm.Context, method))
    assert "keccak_calls.hip" in read("zkm_amd", "csrc", "Makefile")
    assert zkm.SPONGE_BYTE_ADDRESSED == FLAG == zkm.abi.constants()["ZKM_SPONGE_BYTE_ADDRESSED"]
    assert "pub const ZKM_SPONGE_BYTE_ADDRESSED: u64 = 0x8000000000000000;" in read("integration", "rust", "zkm_hip_sys.rs")
    assert "KECCAK_CALL" not in read("include", "zkm_hip.h")                             # no constant, struct, kind or handle but the flag


def offsets(lengths, first=0):
    return (first + np.cumsum([0] + list(lengths))).astype(np.uint64)


def metas(lengths, **kw):
    """One good meta per length: disjoint addresses, clocks far enough apart."""
    return np.array([(0, 0, (0x10000 + 0x1000 * k) | FLAG, 10 * (200 + 100 * k)) for k in range(len(lengths))], dtype=np.uint64).reshape(-1, 4)


@pytest.mark.parametrize("L", [4, 32, 36, 132, 136, 140, 272])
def test_counts_records_masks_and_clocks_of_one_call(zkm, L):
    W = L // 4
    R, B = (W + 7) // 8, L // 136 + 1
    off, meta = offsets([L], first=12), metas([L])
    assert zkm.keccak_calls_counts(off) == (R + 2, L, 34 * B, B)
    steps, clocks = zkm.keccak_calls_steps(off, meta, raw_base=5)
    S = 200
    assert clocks.tolist() == list(range(S - R, S + 2))
    tail = W - 8 * (R - 1)
    assert steps["reads"][:, 1].tolist() == [0xFF] * (R - 1) + [(1 << tail) - 1, 0, 0xFF]
    assert steps["reads"][:, 0].tolist() == list(range(5, 5 + R + 2)) and (steps["kind"] == zkm.STEP["RAW"]).all()
    assert not steps["reads"][:, 2:].any() and not any(steps[f].any() for f in ("pc", "next_pc", "insn", "flags", "context"))
    # and the model says the same
    x = K.Expansion()
    x.keccak(bytes(L), meta[0], 0x40000)
    want_steps, want_clocks = K.steps(x, raw_base=5)
    assert steps.tobytes() == want_steps.tobytes() and (clocks == want_clocks).all()


def test_three_calls_of_different_lengths(zkm):
    lengths = [4, 140, 36]
    off, meta = offsets(lengths), metas(lengths)
    assert zkm.keccak_calls_counts(off) == (3 + 7 + 4, 180, 34 * 4, 4)
    steps, clocks = zkm.keccak_calls_steps(off, meta, raw_base=2)
    x = K.expand(np.zeros(180, dtype=np.uint8), off, meta, [0x40000, 0x40040, 0x40080])
    want_steps, want_clocks = K.steps(x, raw_base=2)
    assert len(steps) == 14 and steps.tobytes() == want_steps.tobytes() and (clocks == want_clocks).all()
    assert clocks.tolist() == [199, 200, 201] + list(range(295, 302)) + [398, 399, 400, 401]
    assert steps["reads"][:, 1].tolist() == [1, 0, 0xFF] + [0xFF] * 4 + [7, 0, 0xFF] + [0xFF, 1, 0, 0xFF]
    L = zkm.load()
    assert L.zkm_keccak_calls_counts(off.ctypes.data, 3, None, None, None, None, None) == 0      # any out pointer may be NULL
    assert zkm.keccak_calls_counts([0]) == (0, 0, 0, 0)


GOOD = (0, 0, 0x1000 | FLAG, 100)


def meta_(**kw):
    m = list(GOOD)
    for k, v in kw.items():
        m[("context", "segment", "address", "timestamp").index(k)] = v
    return tuple(m)


# (lengths of the three calls, the bad call's meta (call 1), the message behind "<list>: call 1: ")
REFUSED = [
    ("input_off", [8, 0, 8], GOOD, r"length 0 is not a positive multiple of 4"),
    ("input_off", [8, 6, 8], GOOD, r"length 6 is not a positive multiple of 4 \(the other bytes of the last memory word follow from no list"),
    ("input_off", [8, -4, 8], GOOD, r"the offsets do not increase \(8 then 4\)"),
    ("meta", [8, 8, 8], meta_(address=0x1000), r"virt_base 0x1000 lacks ZKM_SPONGE_BYTE_ADDRESSED"),
    ("meta", [8, 8, 8], meta_(timestamp=105), r"timestamp 105 is not a multiple of 10 \(NUM_CHANNELS\)"),
    ("meta", [8, 72, 8], meta_(timestamp=20), r"timestamp 20 puts the first read row before clock 0"),
    ("meta", [8, 12, 8], meta_(address=0xFFFFFFF8 | FLAG), r"address of word 0 0xfffffff8: word 2 does not fit in 32 bits"),
    ("meta", [8, 8, 8], meta_(address=(1 << 32) | FLAG), r"address of word 0 0x100000000: word 1 does not fit in 32 bits"),
    ("meta", [8, 8, 8], meta_(context=1 << 32), r"context 4294967296 does not fit in 32 bits"),
    ("meta", [8, 8, 8], meta_(segment=1 << 40), r"segment 1099511627776 does not fit in 32 bits"),
]


def witness_without_context(zkm, off, meta, daddrs, inputs=True, outs=None):
    """zkm_keccak_calls_witness with no context: the message it fails with."""
    L = zkm.load()
    n = len(meta)
    data = np.zeros(max(int(off.max()), 8), dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)              # never written: the call fails on the host
    outs = outs if outs is not None else [out.ctypes.data] * 5
    err = C.c_char_p()
    assert L.zkm_keccak_calls_witness(None, data.ctypes.data if inputs else None, off.ctypes.data, meta.ctypes.data if n else None,
                                      daddrs.ctypes.data if n else None, n, *outs, C.byref(err)) == 1
    return err.value.decode()


@pytest.mark.parametrize("which,lengths,bad,message", REFUSED, ids=["%s-%d" % (r[0], i) for i, r in enumerate(REFUSED)])
def test_every_refusal_names_the_list_and_the_call(zkm, which, lengths, bad, message):
    off = offsets(lengths)
    meta = np.array([GOOD, bad, GOOD], dtype=np.uint64)
    daddrs = np.array([0x2000, 0x2040, 0x2080], dtype=np.uint64)
    at = "%s: call 1: " % which
    # (the export itself: the binding sizes its buffers with zkm_keccak_calls_counts, which refuses the offsets first)
    steps, clocks, err = np.zeros(64, dtype=zkm.CPU_STEP_DT), np.zeros(64, dtype=np.uint64), C.c_char_p()
    assert zkm.load().zkm_keccak_calls_steps(off.ctypes.data, meta.ctypes.data, 3, 0, steps.ctypes.data, clocks.ctypes.data, C.byref(err)) == 1
    assert re.match("^zkm_keccak_calls_steps: " + at + message, err.value.decode()), err.value
    assert not steps["kind"].any()
    with pytest.raises(zkm.ZkmError, match="^zkm_keccak_calls_(steps|counts): " + at + message):
        zkm.keccak_calls_steps(off, meta)
    assert re.match("^zkm_keccak_calls_witness: " + at + message, witness_without_context(zkm, off, meta, daddrs))
    if which == "input_off":
        with pytest.raises(zkm.ZkmError, match="^zkm_keccak_calls_counts: " + at + message):
            zkm.keccak_calls_counts(off)


def test_the_boundaries_are_accepted(zkm):
    """The highest addresses that fit, the smallest timestamp, the largest context and segment."""
    off = offsets([72])
    meta = np.array([(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFB8 | FLAG, 30)], dtype=np.uint64)        # 18 words: the last at 0xFFFFFFFC; three read rows
    steps, clocks = zkm.keccak_calls_steps(off, meta)
    assert clocks.tolist() == [0, 1, 2, 3, 4]
    daddrs = np.array([0xFFFFFFE3], dtype=np.uint64)
    assert witness_without_context(zkm, off, meta, daddrs) == "zkm_keccak_calls_witness: null argument"
    daddrs[0] += 1
    assert witness_without_context(zkm, off, meta, daddrs) == \
        "zkm_keccak_calls_witness: digest_addrs: call 0: address 0xffffffe4: the digest's eighth word does not fit in 32 bits"


def test_null_lists_outputs_and_raw_base(zkm):
    L = zkm.load()
    err = C.c_char_p()
    off, meta, daddrs = offsets([8, 140]), np.array([GOOD, meta_(timestamp=300)], dtype=np.uint64), np.array([0x2000, 0x2040], dtype=np.uint64)
    steps, clocks = np.zeros(10, dtype=zkm.CPU_STEP_DT), np.zeros(10, dtype=np.uint64)
    o, m, s, c = off.ctypes.data, meta.ctypes.data, steps.ctypes.data, clocks.ctypes.data
    assert L.zkm_keccak_calls_counts(None, 2, None, None, None, None, C.byref(err)) == 1
    assert err.value == b"zkm_keccak_calls_counts: input_off: NULL with a count of 2"
    assert L.zkm_keccak_calls_steps(None, m, 2, 0, s, c, C.byref(err)) == 1
    assert err.value == b"zkm_keccak_calls_steps: input_off: NULL with a count of 2"
    assert L.zkm_keccak_calls_steps(o, None, 2, 0, s, c, C.byref(err)) == 1
    assert err.value == b"zkm_keccak_calls_steps: meta: NULL with a count of 2"
    assert L.zkm_keccak_calls_steps(o, m, 2, 0, None, c, C.byref(err)) == 1
    assert err.value == b"zkm_keccak_calls_steps: null argument"
    assert L.zkm_keccak_calls_steps(o, m, 2, (1 << 32) - 9, s, c, C.byref(err)) == 1
    assert b"raw_base 4294967287: a RAW index does not fit in 32 bits" in err.value
    assert L.zkm_keccak_calls_steps(o, m, 2, (1 << 32) - 10, s, c, C.byref(err)) == 0          # 3 + 7 rows: the last index is 2^32 - 1
    assert L.zkm_keccak_calls_steps(None, None, 0, 0, None, None, None) == 0
    # the witness call: lists and outputs, all before the missing context
    data, out = np.zeros(148, dtype=np.uint8), np.zeros(8, dtype=np.uint64)
    p = out.ctypes.data
    args = [None, data.ctypes.data, o, m, daddrs.ctypes.data, 2, p, p, p, p, p]
    for pos, message in ((1, b"inputs: NULL with a count of 2"), (2, b"input_off: NULL with a count of 2"), (3, b"meta: NULL with a count of 2"),
                         (4, b"digest_addrs: NULL with a count of 2"), (6, b"raw_rows_out_dev: NULL with 10 rows to write"),
                         (7, b"memory_ops_out_dev: NULL with 148 operations to write"), (8, b"logic_ops_out_dev: NULL with 102 operations to write"),
                         (9, b"keccak_inputs_out_dev: NULL with 3 permutations to write"),
                         (10, b"keccak_timestamps_out_dev: NULL with 3 permutations to write")):
        bad = list(args)
        bad[pos] = None
        assert L.zkm_keccak_calls_witness(*bad, C.byref(err)) == 1
        assert err.value == b"zkm_keccak_calls_witness: " + message, err.value
    for pos, shift in ((6, 4), (7, 4), (8, 2), (9, 4), (10, 4)):        # an output that is not aligned to its words
        bad = list(args)
        bad[pos] = p + shift
        assert L.zkm_keccak_calls_witness(*bad, C.byref(err)) == 1 and err.value.startswith(b"zkm_keccak_calls_witness: an output is not aligned"), err.value
    # nothing to refuse: the missing context is what is left
    assert L.zkm_keccak_calls_witness(*args, C.byref(err)) == 1 and err.value == b"zkm_keccak_calls_witness: null argument"
    assert L.zkm_keccak_calls_witness(None, None, None, None, None, 0, None, None, None, None, None, C.byref(err)) == 1
    assert err.value == b"zkm_keccak_calls_witness: null argument"


def test_the_rust_recorder_calls_the_three_exports_as_declared(zkm):
    """integration/rust/keccak_calls_hip.rs (uncompiled here): every library call passes as many arguments as the header declares, the
    recorder's entry points are the ones INTEGRATION.md shows, and sponge_lists takes steps of 1 and of 4."""
    from .test_rust_names import call_arities, fn_arity, strip_comments
    src = strip_comments(read("integration", "rust", "keccak_calls_hip.rs"))
    protos = prototypes()
    for fn in NEW + ["zkm_dev_alloc", "zkm_dev_upload"]:
        assert set(call_arities(src, fn)) == {len(protos[fn][1])}, fn
    assert "ZKM_SPONGE_BYTE_ADDRESSED" in src
    assert fn_arity(src, "record_keccak") == 5 and fn_arity(src, "finish") == 4
    integ = read("INTEGRATION.md")
    assert "record_keccak(&mut state.step_log, clock, addr, &input, ptr)" in integ and "keccak_log.finish(ctx, &mut state.step_log" in integ
    seg = strip_comments(read("integration", "rust", "segment_hip.rs"))
    assert "ZKM_SPONGE_BYTE_ADDRESSED" in seg
