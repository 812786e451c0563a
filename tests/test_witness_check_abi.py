"""CPU suite: what is particular to zkm_witness_check / zkm_segment_witness_check (tests/test_abi.py holds every declaration of the C
ABI): the header, the Rust block and the Makefile name the new items, the argument order, the words of a finding, and the refusals --
each made on the host, naming its argument, before the missing context is looked at."""
import ctypes as C
import re

import numpy as np

from zkm_amd import tables as T

from .test_abi import declared_alike, prototypes, read, rust_sys_text

NEW = ["zkm_witness_check", "zkm_segment_witness_check"]


def test_header_rust_block_and_makefile_name_the_new_items(zkm):
    lib, protos = zkm.load(), prototypes()
    for fn in NEW:
        declared_alike(zkm, fn)
        ret, params = protos[fn]
        assert params[0] == ("zkm_ctx*", "ctx") and params[-1] == ("char**", "err"), params
        assert ret == "int" and getattr(lib, fn).restype is C.c_int
    assert protos["zkm_witness_check"][1][1:6] == [("int", "table_id"), ("const uint64_t*", "trace"), ("size_t", "ncols"), ("unsigned", "log_n"),
                                                   ("uint64_t*", "finding")]
    # zkm_segment_check_ctls' way of taking a segment
    assert protos["zkm_segment_witness_check"][1][1:4] == protos["zkm_segment_check_ctls"][1][1:3] + [("uint64_t*", "findings")]
    makefile = read("zkm_amd", "csrc", "Makefile")
    assert re.search(r"^SRCS :=.*\bwitness_check\.hip\b", makefile, flags=re.M)
    wrapper = read("integration", "rust", "witness_check_hip.rs")
    assert all(fn + "(" in wrapper for fn in NEW) and "ZKM_WITNESS_FINDING_WORDS" in wrapper
    # no struct and no handle came with the feature: a finding is plain words
    header = read("include", "zkm_hip.h")
    assert not re.search(r"typedef struct\s+\w*witness", header) and "zkm_witness_finding" not in header
    # the header says what the check leaves to the other two
    doc = header[header.index("/* The table's OWN constraints"):header.index("#define ZKM_WITNESS_FINDING_WORDS")]
    assert "zkm_check_constraints" in doc and "zkm_check_ctls" in doc and "range-check lookups" in doc


def test_finding_words_is_five_in_both_mirrors(zkm):
    assert zkm.abi.constants()["ZKM_WITNESS_FINDING_WORDS"] == 5 and zkm.WITNESS_FINDING_WORDS == 5
    assert re.search(r"pub const ZKM_WITNESS_FINDING_WORDS: usize = 5;", rust_sys_text())


def call_one(zkm, table_id, trace, ncols, log_n, finding=True):
    words, err = (C.c_uint64 * 5)(*([77] * 5)), C.c_char_p()
    rc = zkm.load().zkm_witness_check(None, table_id, None if trace is None else trace.ctypes.data, ncols, log_n, words if finding else None,
                                      C.byref(err))
    assert rc != 0 and list(words) == [77] * 5                  # refused: nothing written
    return err.value.decode()


def call_segment(zkm, traces, log_n, findings=True):
    words, err = (C.c_uint64 * 60)(), C.c_char_p()
    ptrs = None if traces is None else (C.c_void_p * 12)(*[None if t is None else t.ctypes.data for t in traces])
    lg = None if log_n is None else (C.c_uint * 12)(*log_n)
    rc = zkm.load().zkm_segment_witness_check(None, ptrs, lg, words if findings else None, C.byref(err))
    assert rc != 0
    return err.value.decode()


def test_calls_refuse_on_the_host(zkm):
    W = T.WIDTH[T.TABLE_ARITHMETIC]
    trace = np.zeros(W << 3, dtype=np.uint64)
    assert call_one(zkm, 99, trace, W, 3) == "zkm_witness_check: unknown table id 99"
    assert call_one(zkm, -1, trace, W, 3) == "zkm_witness_check: unknown table id -1"
    assert call_one(zkm, T.TABLE_ARITHMETIC, None, W, 3) == "zkm_witness_check: trace: null argument"
    assert call_one(zkm, T.TABLE_ARITHMETIC, trace, W, 3, finding=False) == "zkm_witness_check: finding: null argument"
    assert call_one(zkm, T.TABLE_ARITHMETIC, trace, W - 1, 3) == "zkm_witness_check: ncols 53: Arithmetic has 54 columns"
    assert call_one(zkm, T.TABLE_ARITHMETIC, trace, W, 31) == "zkm_witness_check: log_n 31 above 30"
    # nothing to refuse: the missing context is what is left
    assert call_one(zkm, T.TABLE_ARITHMETIC, trace, W, 3) == "zkm_witness_check: null argument"

    traces = [np.zeros(T.WIDTH[tid] << 3, dtype=np.uint64) for tid in T.TABLE_ENUM_ORDER]
    lg = [3] * 12
    assert call_segment(zkm, None, lg) == "zkm_segment_witness_check: traces: null argument"
    assert call_segment(zkm, traces, None) == "zkm_segment_witness_check: log_n: null argument"
    assert call_segment(zkm, traces, lg, findings=False) == "zkm_segment_witness_check: findings: null argument"
    assert call_segment(zkm, traces[:1] + [None] + traces[2:], lg) == "zkm_segment_witness_check: Cpu: trace: null argument"
    assert call_segment(zkm, traces, lg[:5] + [31] + lg[6:]) == "zkm_segment_witness_check: KeccakSponge: log_n 31 above 30"
    assert call_segment(zkm, traces, lg) == "zkm_segment_witness_check: null argument"
    # no error slot: still a status, no crash
    assert zkm.load().zkm_segment_witness_check(None, None, None, None, None) != 0
    assert zkm.load().zkm_witness_check(None, 0, None, 0, 0, None, None) != 0
