"""CPU suite: the three exports of the SHA-256 precompile expansion (include/zkm_hip.h "SHA-256 precompile calls from their inputs") as
far as they need no GPU -- declared alike everywhere, the counts, the RAW records and clocks of zkm_sha_calls_steps against the model,
and every refusal with the list and the call it names; zkm_sha_calls_witness makes the same refusals before it misses its context."""
import ctypes as C

import numpy as np
import pytest

from . import sha_calls_model as S
from .test_abi import declared_alike, prototypes, read

NEW = ["zkm_sha_calls_counts", "zkm_sha_calls_steps", "zkm_sha_calls_witness"]


def test_symbols_are_exported_and_declared_alike(zkm):
    protos = prototypes()
    for fn in NEW:
        declared_alike(zkm, fn)
    assert protos["zkm_sha_calls_counts"][0] == "void" and protos["zkm_sha_calls_witness"][1][0] == ("zkm_ctx*", "ctx")
    assert all(ty != "zkm_ctx*" for fn in NEW[:2] for ty, _ in protos[fn][1])          # pure: no context
    for method in ("sha_calls_witness", "sha_calls_expand"):
        assert callable(getattr(zkm.Context, method))
    assert "sha_calls.hip" in read("zkm_amd", "csrc", "Makefile")
    assert "SHA_CALL" not in read("include", "zkm_hip.h")                               # no constant, struct, kind or handle was added


@pytest.mark.parametrize("E,C_", [(0, 0), (1, 0), (0, 1), (3, 2)])
def test_counts(zkm, E, C_):
    assert zkm.sha_calls_counts(E, C_) == (96 * E + 11 * C_, 768 * E + 288 * C_, 192 * E + 768 * C_, 48 * E)
    zkm.load().zkm_sha_calls_counts(E, C_, None, None, None, None)                    # any out pointer may be NULL


def calls_3_2(seed=9):
    rng = np.random.default_rng(seed)
    emeta = np.array([(0, 0, 0x10000 + 0x400 * e, 10 * (20 + 100 * e)) for e in range(3)], dtype=np.uint64)
    cmeta = np.array([(0, 0, 0x20000 + 0x400 * c, 10 * (400 + 20 * c), 0x30000 + 0x400 * c, 0, 0, 0) for c in range(2)], dtype=np.uint64)
    e = (rng.integers(0, 1 << 32, (3, 16), dtype=np.uint64).astype(np.uint32), emeta)
    c = (rng.integers(0, 1 << 32, (2, 8), dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, (2, 64), dtype=np.uint64).astype(np.uint32), cmeta)
    return e, c


def test_steps_equal_the_models_records_and_clocks(zkm):
    e, c = calls_3_2()
    want_steps, want_clocks = S.steps(S.expand(e, c), raw_base=2)
    steps, clocks = zkm.sha_calls_steps(e[1], c[2], raw_base=2)
    assert len(steps) == 310 and steps.tobytes() == want_steps.tobytes()
    assert (clocks == want_clocks).all()
    assert steps["reads"][0].tolist() == [2, 0x1F, 0, 0, 0, 0] and steps["reads"][3 * 96 + 9].tolist() == [2 + 297, 0, 0, 0, 0, 0]


EXT = (0, 0, 0x1000, 100)
CMP = (0, 0, 0x2000, 200, 0x3000, 0, 0, 0)


def ext(**kw):
    m = list(EXT)
    for k, v in kw.items():
        m[("context", "segment", "address", "timestamp").index(k)] = v
    return tuple(m)


def cmp_(**kw):
    m = list(CMP)
    for k, v in kw.items():
        m[("context", "segment", "address", "timestamp", "w_address", "w_segment", "w_context").index(k)] = v
    return tuple(m)


# (list, the bad call's meta, the message behind "<list>_meta: call <position>: ")
REFUSED = [
    ("extend", ext(timestamp=105), r"timestamp 105 is not a multiple of 10 \(NUM_CHANNELS\)"),
    ("extend", ext(timestamp=0), r"timestamp 0 puts the first read row before clock 0"),
    ("extend", ext(address=0xFFFFFF04), r"address of w\[0\] 0xffffff04: w\[63\] does not fit in 32 bits"),
    ("extend", ext(context=1 << 32), r"context 4294967296 does not fit in 32 bits"),
    ("extend", ext(segment=1 << 40), r"segment 1099511627776 does not fit in 32 bits"),
    ("compress", cmp_(timestamp=207), r"timestamp 207 is not a multiple of 10 \(NUM_CHANNELS\)"),
    ("compress", cmp_(timestamp=80), r"timestamp 80 puts the hx row before clock 0"),
    ("compress", cmp_(address=0xFFFFFFE4), r"address of hx\[0\] 0xffffffe4: hx\[7\] does not fit in 32 bits"),
    ("compress", cmp_(w_address=0xFFFFFF00), r"address of w\[0\] 0xffffff00: the 65th round's dummy address w \+ 256 does not fit in 32 bits"),
    ("compress", cmp_(context=1 << 32), r"context 4294967296 does not fit in 32 bits"),
    ("compress", cmp_(segment=1 << 32), r"segment 4294967296 does not fit in 32 bits"),
    ("compress", cmp_(w_segment=1 << 32), r"segment of w 4294967296 does not fit in 32 bits"),
    ("compress", cmp_(w_context=1 << 33), r"context of w 8589934592 does not fit in 32 bits"),
]


def witness_without_context(zkm, emeta, cmeta):
    """zkm_sha_calls_witness with good data lists and no context: the message it fails with."""
    L = zkm.load()
    w16, hx, w = np.zeros((len(emeta), 16), dtype=np.uint32), np.zeros((len(cmeta), 8), dtype=np.uint32), np.zeros((len(cmeta), 64), dtype=np.uint32)
    out = np.zeros(8, dtype=np.uint64)              # never written: the call fails on the host
    err = C.c_char_p()
    p = lambda a: a.ctypes.data if a.size else None
    assert L.zkm_sha_calls_witness(None, p(w16), p(emeta), len(emeta), p(hx), p(w), p(cmeta), len(cmeta), out.ctypes.data, out.ctypes.data,
                                   out.ctypes.data, out.ctypes.data, out.ctypes.data, C.byref(err)) == 1
    return err.value.decode()


@pytest.mark.parametrize("which,bad,message", REFUSED, ids=["%s-%d" % (w, i) for i, (w, _, _) in enumerate(REFUSED)])
def test_every_refusal_names_the_list_and_the_call(zkm, which, bad, message):
    emeta = np.array([EXT, EXT, bad] if which == "extend" else [EXT], dtype=np.uint64)
    cmeta = np.array([CMP, bad, CMP] if which == "compress" else [CMP], dtype=np.uint64)
    at = "%s_meta: call %d: " % (which, 2 if which == "extend" else 1)
    with pytest.raises(zkm.ZkmError, match="^zkm_sha_calls_steps: " + at + message):
        zkm.sha_calls_steps(emeta, cmeta)
    import re
    assert re.match("^zkm_sha_calls_witness: " + at + message, witness_without_context(zkm, emeta, cmeta))
    # the boundary itself is accepted: the highest addresses that fit, the smallest timestamps
    good_e = np.array([ext(address=0xFFFFFF03, timestamp=10, context=0xFFFFFFFF, segment=0xFFFFFFFF)], dtype=np.uint64)
    good_c = np.array([cmp_(address=0xFFFFFFE3, w_address=0xFFFFFEFF, timestamp=90, w_context=0xFFFFFFFF, w_segment=0xFFFFFFFF)], dtype=np.uint64)
    steps, clocks = zkm.sha_calls_steps(good_e, good_c)
    assert clocks[0] == 0 and clocks[96] == 0


def test_null_lists_and_outputs(zkm):
    L = zkm.load()
    err = C.c_char_p()
    one_e, one_c = np.array([EXT], dtype=np.uint64), np.array([CMP], dtype=np.uint64)
    steps, clocks = np.zeros(107, dtype=zkm.CPU_STEP_DT), np.zeros(107, dtype=np.uint64)
    assert L.zkm_sha_calls_steps(None, 3, None, 0, 0, steps.ctypes.data, clocks.ctypes.data, C.byref(err)) == 1
    assert err.value == b"zkm_sha_calls_steps: extend_meta: NULL with a count of 3"
    assert L.zkm_sha_calls_steps(one_e.ctypes.data, 1, None, 2, 0, steps.ctypes.data, clocks.ctypes.data, C.byref(err)) == 1
    assert err.value == b"zkm_sha_calls_steps: compress_meta: NULL with a count of 2"
    assert L.zkm_sha_calls_steps(one_e.ctypes.data, 1, one_c.ctypes.data, 1, 0, None, clocks.ctypes.data, C.byref(err)) == 1
    assert err.value == b"zkm_sha_calls_steps: null argument"
    assert L.zkm_sha_calls_steps(one_e.ctypes.data, 1, one_c.ctypes.data, 1, (1 << 32) - 100, steps.ctypes.data, clocks.ctypes.data, C.byref(err)) == 1
    assert b"raw_base 4294967196: a RAW index does not fit in 32 bits" in err.value
    assert L.zkm_sha_calls_steps(None, 0, None, 0, 0, None, None, None) == 0
    # the witness call: data lists and outputs, all before the missing context
    w16, hx, w, out = np.zeros(16, dtype=np.uint32), np.zeros(8, dtype=np.uint32), np.zeros(64, dtype=np.uint32), np.zeros(8, dtype=np.uint64)
    o = out.ctypes.data
    args = [None, w16.ctypes.data, one_e.ctypes.data, 1, hx.ctypes.data, w.ctypes.data, one_c.ctypes.data, 1, o, o, o, o, o]
    for pos, message in ((1, b"extend_w16: NULL with a count of 1"), (4, b"compress_hx: NULL with a count of 1"), (5, b"compress_w: NULL with a count of 1"),
                         (8, b"raw_rows_out_dev: NULL with 107 rows to write"), (9, b"memory_ops_out_dev: NULL with 1056 operations to write"),
                         (10, b"logic_ops_out_dev: NULL with 960 operations to write"), (11, b"sha_extend_inputs_out_dev: NULL with 48 rows to write"),
                         (12, b"sha_extend_timestamps_out_dev: NULL with 48 rows to write")):
        bad = list(args)
        bad[pos] = None
        assert L.zkm_sha_calls_witness(*bad, C.byref(err)) == 1
        assert err.value == b"zkm_sha_calls_witness: " + message, err.value
    for pos, off in ((8, 4), (9, 4), (10, 2), (11, 1), (12, 4)):        # an output that is not aligned to its words
        bad = list(args)
        bad[pos] = o + off
        assert L.zkm_sha_calls_witness(*bad, C.byref(err)) == 1 and err.value.startswith(b"zkm_sha_calls_witness: an output is not aligned"), err.value
    # nothing to refuse: the missing context is what is left
    assert L.zkm_sha_calls_witness(*args, C.byref(err)) == 1 and err.value == b"zkm_sha_calls_witness: null argument"
    assert witness_without_context(zkm, one_e[:0], one_c[:0]) == "zkm_sha_calls_witness: null argument"


def test_the_rust_recorder_calls_the_three_exports_as_declared(zkm):
    """integration/rust/sha_calls_hip.rs (uncompiled here): every library call passes as many arguments as the header declares, and the
    recorder's two entry points are the ones INTEGRATION.md shows."""
    from .test_rust_names import call_arities, fn_arity, strip_comments
    src = strip_comments(read("integration", "rust", "sha_calls_hip.rs"))
    protos = prototypes()
    for fn in NEW + ["zkm_dev_alloc", "zkm_dev_upload"]:
        assert call_arities(src, fn) == [len(protos[fn][1])], fn
    assert fn_arity(src, "record_sha_extend") == 4 and fn_arity(src, "record_sha_compress") == 6 and fn_arity(src, "finish") == 4
    cpu_steps = strip_comments(read("integration", "rust", "cpu_steps_hip.rs"))
    assert "pub struct StepLog" in cpu_steps and "pub steps: Vec<zkm_cpu_step>" in cpu_steps and "pub raw_rows: Vec<u64>" in cpu_steps
    integ = read("INTEGRATION.md")
    assert "record_sha_extend(&mut state.step_log, clock, w_ptr, &w16)" in integ and "sha_log.finish(ctx, &mut state.step_log" in integ
