"""CPU suite: what is particular to zkm_segments_check / zkm_segment_check and the tuning key "check_witness" (tests/test_abi.py holds
every declaration of the C ABI): the header, the ctypes binding, the Rust block and the Makefile name the new items; every refusal is
made on the host without a context, with its exact message; the key is accepted by the library and documented in the header."""
import ctypes as C
import re

import numpy as np

from zkm_amd import tables as T

from .test_abi import declared_alike, prototypes, read, rust_sys_text

NEW = ["zkm_segments_check", "zkm_segment_check"]


def test_both_functions_are_declared_alike_in_header_ctypes_and_rust_block(zkm):
    lib, protos = zkm.load(), prototypes()
    for fn in NEW:
        declared_alike(zkm, fn)
        ret, params = protos[fn]
        assert params[0] == ("zkm_ctx*", "ctx") and params[-1] == ("char**", "err"), params
        assert ret == "int" and getattr(lib, fn).restype is C.c_int
    assert protos["zkm_segments_check"][1][1:8] == [("size_t", "nseg"), ("const uint64_t* const* const*", "traces"), ("const unsigned* const*", "log_n"),
                                                    ("uint64_t*", "verdicts"), ("uint64_t*", "witness_findings"), ("uint64_t*", "lookup_findings"),
                                                    ("zkm_ctl_report*", "ctl_reports")]
    # one segment: zkm_segment_check_ctls' way of taking it, then the same outputs
    assert protos["zkm_segment_check"][1][1:3] == protos["zkm_segment_check_ctls"][1][1:3]
    assert [ty for ty, _ in protos["zkm_segment_check"][1][3:7]] == [ty for ty, _ in protos["zkm_segments_check"][1][4:8]]
    # the K-segment call takes its segments as zkm_prove_segments does
    assert protos["zkm_segments_check"][1][2:4] == protos["zkm_prove_segments"][1][3:5]
    assert re.search(r"^SRCS :=.*\bsegment_check\.hip\b", read("zkm_amd", "csrc", "Makefile"), flags=re.M)
    wrapper = read("integration", "rust", "segment_check_hip.rs")
    assert all(fn + "(" in wrapper for fn in NEW) and "ZKM_SEGMENT_VERDICT_WORDS" in wrapper and "Result<" in wrapper
    # no struct and no handle came with the feature: verdicts and findings are plain words, the report is check_ctls'
    header = read("include", "zkm_hip.h")
    assert not re.search(r"typedef struct\s+\w*segment_check", header) and "zkm_segment_verdict" not in header
    assert zkm.abi.constants()["ZKM_SEGMENT_VERDICT_WORDS"] == 2 == zkm.SEGMENT_VERDICT_WORDS
    assert re.search(r"pub const ZKM_SEGMENT_VERDICT_WORDS: usize = 2;", rust_sys_text())
    assert all(hasattr(zkm.Context, m) for m in ("segments_check", "segment_check"))


def call(zkm, segments, nseg=None, traces=True, log_n=True):
    """zkm_segments_check without a context on segments = [(twelve arrays or None / None, twelve heights / None)]; the message."""
    k = len(segments)
    keep_t = [None if tr is None else (C.c_void_p * 12)(*[None if t is None else t.ctypes.data for t in tr]) for tr, _ in segments]
    keep_l = [None if lg is None else (C.c_uint * 12)(*lg) for _, lg in segments]
    tp = (C.c_void_p * max(k, 1))(*[None if p is None else C.addressof(p) for p in keep_t])
    lp = (C.c_void_p * max(k, 1))(*[None if p is None else C.addressof(p) for p in keep_l])
    verdicts, err = (C.c_uint64 * (2 * max(k, 1)))(*([77] * (2 * max(k, 1)))), C.c_char_p()
    rc = zkm.load().zkm_segments_check(None, k if nseg is None else nseg, tp if traces else None, lp if log_n else None, verdicts, None, None, None,
                                       C.byref(err))
    assert rc != 0 and set(verdicts) == {77}                    # refused: nothing written
    return err.value.decode()


def call_one(zkm, tr, lg):
    ptrs = None if tr is None else (C.c_void_p * 12)(*[None if t is None else t.ctypes.data for t in tr])
    lgc = None if lg is None else (C.c_uint * 12)(*lg)
    err = C.c_char_p()
    assert zkm.load().zkm_segment_check(None, ptrs, lgc, None, None, None, None, C.byref(err)) != 0
    return err.value.decode()


def test_every_refusal_is_made_without_a_context(zkm):
    traces = [np.zeros(T.WIDTH[tid] << 3, dtype=np.uint64) for tid in T.TABLE_ENUM_ORDER]
    lg = [3] * 12
    good = (traces, lg)
    assert call(zkm, [good], nseg=0) == "zkm_segments_check: nseg: no segment"
    assert call(zkm, [good], traces=False) == "zkm_segments_check: traces: null argument"
    assert call(zkm, [good], log_n=False) == "zkm_segments_check: log_n: null argument"
    assert call(zkm, [good, (None, lg)]) == "zkm_segments_check: segment 1: traces: null argument"
    assert call(zkm, [good, good, (traces, None)]) == "zkm_segments_check: segment 2: log_n: null argument"
    assert call(zkm, [good, (traces[:10] + [None] + traces[11:], lg)]) == "zkm_segments_check: segment 1: Logic: trace: null argument"
    assert call(zkm, [(traces[:1] + [None] + traces[2:], lg), good]) == "zkm_segments_check: segment 0: Cpu: trace: null argument"
    assert call(zkm, [good, (traces, lg[:5] + [31] + lg[6:])]) == "zkm_segments_check: segment 1: KeccakSponge: log_n 31 above 30"
    assert call(zkm, [good, (traces, [26] + lg[1:])]) == "zkm_segments_check: segment 1: Arithmetic: 19 x 2^26 records above 2^30"
    # the lowest segment's refusal is the one reported
    assert call(zkm, [(traces, lg[:11] + [31]), (None, lg)]) == "zkm_segments_check: segment 0: Memory: log_n 31 above 30"
    # nothing to refuse: the missing context is what is left
    assert call(zkm, [good, good]) == "zkm_segments_check: null argument"
    # the one-segment form names itself
    assert call_one(zkm, None, lg) == "zkm_segment_check: traces: null argument"
    assert call_one(zkm, traces, None) == "zkm_segment_check: log_n: null argument"
    assert call_one(zkm, traces[:10] + [None] + traces[11:], lg) == "zkm_segment_check: segment 0: Logic: trace: null argument"
    assert call_one(zkm, traces, lg[:1] + [31] + lg[2:]) == "zkm_segment_check: segment 0: Cpu: log_n 31 above 30"
    assert call_one(zkm, traces, lg) == "zkm_segment_check: null argument"
    # no error slot: still a status, no crash
    assert zkm.load().zkm_segments_check(None, 0, None, None, None, None, None, None, None) != 0
    assert zkm.load().zkm_segment_check(None, None, None, None, None, None, None, None) != 0


def test_check_witness_is_accepted_and_documented():
    core = read("zkm_amd", "csrc", "core.hip")
    body = core[core.index("int zkm_ctx_set_tuning("):]
    body = body[:body.index("\n}\n")]
    assert 'k == "check_witness"' in body
    header = read("include", "zkm_hip.h")
    doc = header[header.index(' *   "check_witness"'):header.index(' *   "verify"')]
    assert "zkm_segments_check" in doc and "check_witness: segment <position in the call>" in doc and "Default 0" in doc
    assert '"check_ctls"' in doc                                  # what happens when both keys are set
    # the pool passes any key on unchanged
    pool = read("zkm_amd", "csrc", "pool.hip")
    assert "check_witness" not in pool and "zkm_ctx_set_tuning(" in pool
