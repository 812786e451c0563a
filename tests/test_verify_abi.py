"""CPU suite: what is particular to zkm_verify_proofs / zkm_verify_segments / zkm_verify_single_table (tests/test_abi.py holds every
declaration and layout of the C ABI): the argument orders mirror the provers', the report's fields and codes are the contract's, and
what needs no GPU: a null context, null blob pointers and nseg 0 are FAILED through the error channel, never a crash."""
import ctypes as C
import re

import numpy as np

from .test_abi import c_layouts, declared_alike, header_text, prototypes, read, rust_sys_text

NEW = ["zkm_verify_proofs", "zkm_verify_segments", "zkm_verify_single_table"]
CODES = ["OK", "SHAPE", "TRANSCRIPT_STATE", "CTL_CHALLENGES", "QUOTIENT", "POW", "INITIAL_MERKLE", "FRI_EVAL", "FRI_MERKLE", "FINAL_POLY", "CTL_SUM",
         "FAILED"]


def test_symbols_are_exported_and_declared_alike(zkm):
    lib, protos = zkm.load(), prototypes()
    names = lambda fn: [name for _, name in protos[fn][1]]
    for fn in NEW:
        declared_alike(zkm, fn)
        ret, params = protos[fn]
        assert params[0] == ("zkm_ctx*", "ctx") and params[-1] == ("char**", "err") and params[-2][0] == "zkm_verify_report*", params
        assert params[-2][1].startswith("report") and ret == "int" and getattr(lib, fn).restype is C.c_int
    # the general form mirrors zkm_prove_with_traces, the single-table form zkm_prove_single_table
    assert names("zkm_verify_proofs")[1:9] == names("zkm_prove_with_traces")[1:9]
    assert names("zkm_verify_proofs")[9:12] == ["proofs", "proof_words", "ctl_challenges"]
    assert names("zkm_verify_segments")[1:8] == ["cfg", "nseg", "proofs", "proof_words", "public_values", "npublic", "ctl_challenges"]
    assert names("zkm_verify_single_table")[1:10] == ["table_id", "cfg", "proof", "proof_words", "ncols", "naux", "num_helpers", "nctl_zs", "challenger"]


def test_report_fields_and_codes_are_the_contracts(zkm):
    want = c_layouts()["zkm_verify_report"]["fields"]
    assert [f[0] for f in want] == ["code", "table", "challenge", "query", "tree", "layer", "ctl", "host_waits"]
    # the codes: header, Python and Rust number the checks alike, in the reference's order of checks
    header, rust_text = header_text(), rust_sys_text()
    for value, name in enumerate(CODES):
        assert re.search(r"#define ZKM_VERIFY_%s %d\b" % (name, value), header), name
        assert getattr(zkm, "VERIFY_" + name) == value and zkm.VERIFY_CODES[value] == name
        assert re.search(r"pub const ZKM_VERIFY_%s: u32 = %d;" % (name, value), rust_text), name
    assert len(zkm.VERIFY_CODES) == len(CODES)
    # no opaque handle was added
    assert not re.search(r"typedef struct zkm_verify\w* zkm_verify\w*;\s*$", header.split("typedef struct zkm_verify_report")[0])


def calls(zkm):
    L = zkm.load()
    cfg = zkm.StarkConfig()
    L.zkm_standard_config(C.byref(cfg))
    return L, cfg


def test_null_context_and_null_blobs_are_failed_not_a_crash(zkm):
    L, cfg = calls(zkm)
    blob = np.zeros(64, dtype=np.uint64)
    pp, pw = (C.c_void_p * 1)(blob.ctypes.data), (C.c_size_t * 1)(blob.size)
    for args in ((None, C.byref(cfg), 1, pp, pw), (None, None, 0, None, None)):
        rep, err = zkm.VerifyReport(), C.c_char_p()
        rc = L.zkm_verify_segments(*args, None, None, None, C.byref(rep) if args[2] else None, C.byref(err))
        assert rc != 0 and b"null argument" in err.value
        assert not args[2] or rep.code == zkm.VERIFY_FAILED
    # no report, no error slot: still a status
    assert L.zkm_verify_segments(None, None, 0, None, None, None, None, None, None, None) != 0
    rep, err = zkm.VerifyReport(), C.c_char_p()
    assert L.zkm_verify_proofs(None, C.byref(cfg), None, 0, None, None, 0, None, 0, None, 0, None, C.byref(rep), C.byref(err)) != 0
    assert rep.code == zkm.VERIFY_FAILED and b"null argument" in err.value
    rep, err = zkm.VerifyReport(), C.c_char_p()
    ch = zkm.Challenger()
    assert L.zkm_verify_single_table(None, 0, C.byref(cfg), None, 0, 262, 4, None, 2, C.byref(ch), C.byref(rep), C.byref(err)) != 0
    assert rep.code == zkm.VERIFY_FAILED and b"null argument" in err.value
    assert bytes(ch) == bytes(zkm.Challenger())


def test_the_keys_are_documented_and_the_hook_is_guarded():
    core = read("zkm_amd", "csrc", "core.hip")
    assert 'k == "verify"' in core
    branch = core[core.index('k == "debug_verify_flip"'):]
    branch = branch[:branch.index("else if")]
    assert 'getenv("ZKM_ENABLE_TEST_HOOKS")' in branch and "unknown key" in branch
    header = read("include", "zkm_hip.h")
    assert "ZKM_ENABLE_TEST_HOOKS=1" in header[header.index('"debug_verify_flip"'):][:400]
    doc = header[header.index('"verify" '):header.index('"debug_verify_flip"')]
    assert "Default 0" in doc and "no proof word is handed out" in doc
    assert "verify.hip" in read("zkm_amd", "csrc", "Makefile")
