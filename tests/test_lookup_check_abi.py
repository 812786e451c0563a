"""CPU suite: what is particular to zkm_lookup_check / zkm_segment_lookup_check (tests/test_abi.py holds every declaration of the C ABI):
the header, the Rust block, the wrapper and the Makefile name the new items, the argument order, the words of a finding, and the
refusals -- each made on the host, naming its argument, before the missing context is looked at, with nothing written to the finding."""
import ctypes as C
import re

import numpy as np

from zkm_amd import tables as T

from .test_abi import declared_alike, prototypes, read, rust_sys_text

NEW = ["zkm_lookup_check", "zkm_segment_lookup_check"]
WORDS = 9


def test_header_rust_block_wrapper_and_makefile_name_the_new_items(zkm):
    lib, protos = zkm.load(), prototypes()
    for fn in NEW:
        declared_alike(zkm, fn)
        ret, params = protos[fn]
        assert params[0] == ("zkm_ctx*", "ctx") and params[-1] == ("char**", "err"), params
        assert ret == "int" and getattr(lib, fn).restype is C.c_int
    # zkm_witness_check's arguments with `finding`; zkm_segment_check_ctls' way of taking a segment
    assert protos["zkm_lookup_check"][1][1:6] == protos["zkm_witness_check"][1][1:6]
    assert protos["zkm_lookup_check"][1][5] == ("uint64_t*", "finding")
    assert protos["zkm_segment_lookup_check"][1][1:4] == protos["zkm_segment_check_ctls"][1][1:3] + [("uint64_t*", "findings")]
    makefile = read("zkm_amd", "csrc", "Makefile")
    assert re.search(r"^SRCS :=.*\blookup_check\.hip\b", makefile, flags=re.M)
    wrapper = read("integration", "rust", "lookup_check_hip.rs")
    assert all(fn + "(" in wrapper for fn in NEW) and "ZKM_LOOKUP_FINDING_WORDS" in wrapper
    assert "LookupFinding" in wrapper and "fn lookup_check_hip" in wrapper and "fn segment_lookup_check_hip" in wrapper
    assert 'starts_with("Lookup failed in ")' in wrapper
    # no struct and no handle came with the feature: a finding is plain words
    header = read("include", "zkm_hip.h")
    assert not re.search(r"typedef struct\s+\w*lookup_(check|finding)", header) and "zkm_lookup_finding" not in header


def test_finding_words_is_nine_in_every_mirror(zkm):
    assert zkm.abi.constants()["ZKM_LOOKUP_FINDING_WORDS"] == WORDS and zkm.LOOKUP_FINDING_WORDS == WORDS
    assert re.search(r"pub const ZKM_LOOKUP_FINDING_WORDS: usize = 9;", rust_sys_text())


def call_one(zkm, table_id, trace, ncols, log_n, finding=True):
    words, err = (C.c_uint64 * WORDS)(*([77] * WORDS)), C.c_char_p()
    rc = zkm.load().zkm_lookup_check(None, table_id, None if trace is None else trace.ctypes.data, ncols, log_n, words if finding else None,
                                     C.byref(err))
    assert rc != 0 and list(words) == [77] * WORDS                 # refused: nothing written
    return err.value.decode()


def call_segment(zkm, traces, log_n, findings=True):
    words, err = (C.c_uint64 * (12 * WORDS))(*([77] * (12 * WORDS))), C.c_char_p()
    ptrs = None if traces is None else (C.c_void_p * 12)(*[None if t is None else t.ctypes.data for t in traces])
    lg = None if log_n is None else (C.c_uint * 12)(*log_n)
    rc = zkm.load().zkm_segment_lookup_check(None, ptrs, lg, words if findings else None, C.byref(err))
    assert rc != 0 and list(words) == [77] * (12 * WORDS)
    return err.value.decode()


def test_calls_refuse_on_the_host(zkm):
    W = T.WIDTH[T.TABLE_ARITHMETIC]
    trace = np.zeros(W << 3, dtype=np.uint64)
    assert call_one(zkm, 99, trace, W, 3) == "zkm_lookup_check: unknown table id 99"
    assert call_one(zkm, -1, trace, W, 3) == "zkm_lookup_check: unknown table id -1"
    assert call_one(zkm, T.TABLE_ARITHMETIC, None, W, 3) == "zkm_lookup_check: trace: null argument"
    assert call_one(zkm, T.TABLE_ARITHMETIC, trace, W, 3, finding=False) == "zkm_lookup_check: finding: null argument"
    assert call_one(zkm, T.TABLE_ARITHMETIC, trace, W - 1, 3) == "zkm_lookup_check: ncols 53: Arithmetic has 54 columns"
    assert call_one(zkm, T.TABLE_ARITHMETIC, trace, W, 31) == "zkm_lookup_check: log_n 31 above 30"
    # the records of a lookup, rows x (looking columns + 1), are bounded by 2^30 (the trace is not read: the refusal comes first)
    assert call_one(zkm, T.TABLE_ARITHMETIC, trace, W, 26) == "zkm_lookup_check: Arithmetic: 19 x 2^26 records above 2^30"
    assert call_one(zkm, T.TABLE_ARITHMETIC, trace, W, 30) == "zkm_lookup_check: Arithmetic: 19 x 2^30 records above 2^30"
    assert call_one(zkm, T.TABLE_MEMORY, trace, T.WIDTH[T.TABLE_MEMORY], 30) == "zkm_lookup_check: Memory: 2 x 2^30 records above 2^30"
    # nothing to refuse: the missing context is what is left (19 x 2^25 and 2 x 2^29 records are within the bound; a table without lookups
    # has no such bound)
    assert call_one(zkm, T.TABLE_ARITHMETIC, trace, W, 3) == "zkm_lookup_check: null argument"
    assert call_one(zkm, T.TABLE_ARITHMETIC, trace, W, 25) == "zkm_lookup_check: null argument"
    assert call_one(zkm, T.TABLE_MEMORY, trace, T.WIDTH[T.TABLE_MEMORY], 29) == "zkm_lookup_check: null argument"
    assert call_one(zkm, T.TABLE_CPU, trace, T.WIDTH[T.TABLE_CPU], 30) == "zkm_lookup_check: null argument"

    traces = [np.zeros(T.WIDTH[tid] << 3, dtype=np.uint64) for tid in T.TABLE_ENUM_ORDER]
    lg = [3] * 12
    assert call_segment(zkm, None, lg) == "zkm_segment_lookup_check: traces: null argument"
    assert call_segment(zkm, traces, None) == "zkm_segment_lookup_check: log_n: null argument"
    assert call_segment(zkm, traces, lg, findings=False) == "zkm_segment_lookup_check: findings: null argument"
    assert call_segment(zkm, traces[:1] + [None] + traces[2:], lg) == "zkm_segment_lookup_check: Cpu: trace: null argument"
    assert call_segment(zkm, traces, lg[:5] + [31] + lg[6:]) == "zkm_segment_lookup_check: KeccakSponge: log_n 31 above 30"
    assert call_segment(zkm, traces, [26] + lg[1:]) == "zkm_segment_lookup_check: Arithmetic: 19 x 2^26 records above 2^30"
    assert call_segment(zkm, traces, lg[:11] + [30]) == "zkm_segment_lookup_check: Memory: 2 x 2^30 records above 2^30"
    assert call_segment(zkm, traces, lg) == "zkm_segment_lookup_check: null argument"
    # no error slot: still a status, no crash
    assert zkm.load().zkm_segment_lookup_check(None, None, None, None, None) != 0
    assert zkm.load().zkm_lookup_check(None, 0, None, 0, 0, None, None) != 0
