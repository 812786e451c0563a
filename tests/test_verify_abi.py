"""CPU suite: the C ABI of zkm_verify_proofs / zkm_verify_segments / zkm_verify_single_table -- exported and declared alike in the
header, the Rust block and the ctypes signatures; zkm_verify_report's layout as the C compiler, ctypes and the Rust mirror see it; and
what needs no GPU: a null context, null blob pointers and nseg 0 are FAILED through the error channel, never a crash."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np

from .test_check_ctls_abi import header_params, read, rust_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["zkm_verify_proofs", "zkm_verify_segments", "zkm_verify_single_table"]
CODES = ["OK", "SHAPE", "TRANSCRIPT_STATE", "CTL_CHALLENGES", "QUOTIENT", "POW", "INITIAL_MERKLE", "FRI_EVAL", "FRI_MERKLE", "FINAL_POLY", "CTL_SUM",
         "FAILED"]


def test_symbols_are_exported_and_declared_alike(zkm):
    lib = zkm.load()
    rust = read("integration", "rust", "zkm_hip_sys.rs")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "zkm_amd", "csrc", "libzkmhip.so")]).decode()
    for fn in NEW:
        assert hasattr(lib, fn) and fn in zkm.EXPORTS and re.search(r" T %s\b" % fn, exported)
        params = header_params(fn)
        assert params[0] == "zkm_ctx* ctx" and params[-1] == "char** err" and params[-2].startswith("zkm_verify_report* report"), params
        assert len(getattr(lib, fn).argtypes) == len(params) and getattr(lib, fn).restype is C.c_int
        r_args = re.search(r"pub fn %s\(([^)]*)\)\s*->\s*c_int;" % fn, rust).group(1).split(",")
        assert [a.split(":")[0].strip() for a in r_args] == [p.split()[-1].lstrip("*") for p in params], fn
    # the general form mirrors zkm_prove_with_traces, the single-table form zkm_prove_single_table
    assert [p.split()[-1] for p in header_params("zkm_verify_proofs")[1:9]] == [p.split()[-1] for p in header_params("zkm_prove_with_traces")[1:9]]
    assert [p.split()[-1] for p in header_params("zkm_verify_proofs")[9:12]] == ["proofs", "proof_words", "ctl_challenges"]
    assert [p.split()[-1] for p in header_params("zkm_verify_segments")[1:8]] == ["cfg", "nseg", "proofs", "proof_words", "public_values", "npublic",
                                                                                 "ctl_challenges"]
    assert [p.split()[-1] for p in header_params("zkm_verify_single_table")[1:10]] == ["table_id", "cfg", "proof", "proof_words", "ncols", "naux",
                                                                                      "num_helpers", "nctl_zs", "challenger"]


def test_report_layout_and_codes_agree(zkm, tmp_path):
    exe = str(tmp_path / "abi_layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "abi_layout.c")])
    lay = json.loads(subprocess.check_output([exe, "verify"]))
    assert set(lay) == {"zkm_verify_report"} == set(zkm.abi_mirrors_verify())
    want = [tuple(f) for f in lay["zkm_verify_report"]["fields"]]
    assert [f[0] for f in want] == ["code", "table", "challenge", "query", "tree", "layer", "ctl", "host_waits"]
    header = re.sub(r"/\*.*?\*/", " ", read("include", "zkm_hip.h"), flags=re.S)
    body = re.search(r"typedef struct zkm_verify_report \{(.*?)\} zkm_verify_report;", header, flags=re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == [f[0] for f in want]
    m = zkm.VerifyReport
    assert [(f, getattr(m, f).offset, getattr(m, f).size) for f, _ in m._fields_] == want
    assert C.sizeof(m) == lay["zkm_verify_report"]["size"] and C.alignment(m) == lay["zkm_verify_report"]["align"]
    rust_text = re.sub(r"//[^\n]*", "", read("integration", "rust", "zkm_hip_sys.rs"))
    assert re.search(r"pub type zkm_verify_report = ZkmVerifyReport;", rust_text)
    size, align, fields = rust_layout("ZkmVerifyReport", rust_text, {})
    assert fields == want and (size, align) == (lay["zkm_verify_report"]["size"], lay["zkm_verify_report"]["align"])
    # the codes: header, Python and Rust number the checks alike, in the reference's order of checks
    for value, name in enumerate(CODES):
        assert re.search(r"#define ZKM_VERIFY_%s %d\b" % (name, value), header), name
        assert getattr(zkm, "VERIFY_" + name) == value and zkm.VERIFY_CODES[value] == name
        assert re.search(r"pub const ZKM_VERIFY_%s: u32 = %d;" % (name, value), rust_text), name
    # the plain output of the tool is the fixed set it always printed; no opaque handle was added
    plain = json.loads(subprocess.check_output([exe]))
    assert "zkm_verify_report" not in plain and "zkm_segment_ops" in plain
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
