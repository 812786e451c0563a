"""CPU suite: what is particular to zkm_check_ctls / zkm_segment_check_ctls (tests/test_abi.py holds every declaration and layout of the
C ABI): the argument order, what the report carries, and the refusals that need no GPU: a null context, a lookup whose sides differ in
width, a column-set index out of range -- each through the error channel with kind 3."""
import ctypes as C
import re

import numpy as np

from .test_abi import c_layouts, declared_alike, prototypes, read

NEW = ["zkm_check_ctls", "zkm_segment_check_ctls"]


def test_symbols_are_exported_and_declared_alike(zkm):
    lib, protos = zkm.load(), prototypes()
    for fn in NEW:
        declared_alike(zkm, fn)
        ret, params = protos[fn]
        assert params[0] == ("zkm_ctx*", "ctx") and params[-2:] == [("zkm_ctl_report*", "report"), ("char**", "err")], params
        assert ret == "int" and getattr(lib, fn).restype is C.c_int
    assert [name for _, name in protos["zkm_check_ctls"][1][1:6]] == ["tables", "ntables", "ctls", "sides", "nctls"]   # zkm_prove_with_traces' order
    assert [name for _, name in protos["zkm_segment_check_ctls"][1][1:3]] == ["traces", "log_n"]


def test_report_carries_what_the_contract_asks(zkm):
    lay = c_layouts()
    rep, loc = lay["zkm_ctl_report"], lay["zkm_ctl_location"]
    fields = {f[0]: (f[1], f[2]) for f in rep["fields"]}
    assert {"kind", "ctl", "attempts", "host_waits", "side", "table", "row", "filter_value", "width", "tuple", "looking_count", "looked_count",
            "looking", "looked"} <= set(fields)
    assert fields["tuple"][1] >= 64 * 8                                              # up to 64 canonical words
    assert fields["looking"][1] >= 8 * loc["size"] and fields["looked"][1] >= 8 * loc["size"]   # at least 8 locations a side
    assert [f[0] for f in loc["fields"]] == ["side", "table", "row"]
    # no opaque handle was added for the feature
    assert not re.search(r"typedef struct zkm_ctl\w* zkm_ctl\w*;", read("include", "zkm_hip.h"))


def small_tables(zkm, widths=(2, 2)):
    """Two one-column-set tables of 8 rows and the lookup between them."""
    from zkm_amd import ctl as zc
    tables = []
    for t, w in enumerate(widths):
        ct = zc.CtlTable()
        ct.singles_set(list(range(w)), filter_col=2)
        tables.append((t, np.zeros(3 * 8, dtype=np.uint64), 3, 3, ct))
    return tables, [([(0, 0)], (1, 0))]


def raw_check(zkm, tables, ctls, ctx=None):
    from zkm_amd import ctl as zc
    tarr, keep = zc.pack_tables([(tid, tr.ctypes.data, ncols, log_n, ct) for tid, tr, ncols, log_n, ct in tables])
    carr, sides = zc.pack_ctls(ctls)
    rep, err = zkm.CtlReport(), C.c_char_p()
    rep.kind = 77
    rc = zkm.load().zkm_check_ctls(ctx, tarr, len(tables), carr.ctypes.data, sides.ctypes.data, len(carr), C.byref(rep), C.byref(err))
    return rc, rep, (err.value or b"").decode()


def test_null_context_is_refused_with_kind_3(zkm):
    tables, ctls = small_tables(zkm)
    rc, rep, msg = raw_check(zkm, tables, ctls)
    assert rc != 0 and rep.kind == 3 and "null argument" in msg
    rep, err = zkm.CtlReport(), C.c_char_p()
    assert zkm.load().zkm_segment_check_ctls(None, None, None, C.byref(rep), C.byref(err)) != 0
    assert rep.kind == 3 and b"null argument" in err.value
    # no report, no error slot: still a status, no crash
    assert zkm.load().zkm_segment_check_ctls(None, None, None, None, None) != 0


def test_unequal_widths_and_bad_indices_are_refused_with_kind_3(zkm):
    tables, ctls = small_tables(zkm, widths=(2, 1))
    rc, rep, msg = raw_check(zkm, tables, ctls)
    assert rc != 0 and rep.kind == 3 and "CTL #0" in msg and "width" in msg, msg
    tables, ctls = small_tables(zkm)
    rc, rep, msg = raw_check(zkm, tables, [([(0, 5)], (1, 0))])
    assert rc != 0 and rep.kind == 3 and "column-set index out of range" in msg, msg
    rc, rep, msg = raw_check(zkm, tables, [([(0, 0)], (7, 0))])
    assert rc != 0 and rep.kind == 3 and "table index out of range" in msg, msg


def test_the_test_hook_is_guarded_and_documented():
    """debug_ctl_key_bits is accepted only under ZKM_ENABLE_TEST_HOOKS=1 (tests/test_gpu_check_ctls.py sets it on a context; here: the
    guard is in the code and the header says so, as for debug_fail_allocs)."""
    core = read("zkm_amd", "csrc", "core.hip")
    branch = core[core.index('k == "debug_ctl_key_bits"'):]
    branch = branch[:branch.index("else if")]
    assert 'getenv("ZKM_ENABLE_TEST_HOOKS")' in branch and "unknown key" in branch
    header = read("include", "zkm_hip.h")
    doc = header[header.index('"debug_ctl_key_bits"'):]
    assert "ZKM_ENABLE_TEST_HOOKS=1" in doc[:400] and '"check_ctls"' in header
