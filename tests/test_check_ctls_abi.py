"""CPU suite: the C ABI of zkm_check_ctls / zkm_segment_check_ctls -- exported and declared alike in the header, the Rust block and the
ctypes signatures; the report's layout as the C compiler, ctypes and the Rust mirror see it; and the refusals that need no GPU: a null
context, a lookup whose sides differ in width, a column-set index out of range -- each through the error channel with kind 3."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["zkm_check_ctls", "zkm_segment_check_ctls"]


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def header_params(fn):
    text = re.sub(r"/\*.*?\*/", " ", read("include", "zkm_hip.h"), flags=re.S)
    return [a.strip() for a in re.search(r"\bint\s+%s\(([^)]*)\)\s*;" % fn, text).group(1).split(",")]


def test_symbols_are_exported_and_declared_alike(zkm):
    lib = zkm.load()
    rust = read("integration", "rust", "zkm_hip_sys.rs")
    for fn in NEW:
        assert hasattr(lib, fn) and fn in zkm.EXPORTS
        params = header_params(fn)
        assert params[0] == "zkm_ctx* ctx" and params[-2:] == ["zkm_ctl_report* report", "char** err"], params
        assert len(getattr(lib, fn).argtypes) == len(params) and getattr(lib, fn).restype is C.c_int
        r_args = re.search(r"pub fn %s\(([^)]*)\)\s*->\s*c_int;" % fn, rust).group(1).split(",")
        assert [a.split(":")[0].strip() for a in r_args] == [p.split()[-1].lstrip("*") for p in params], fn
    assert [p.split()[-1] for p in header_params("zkm_check_ctls")[1:6]] == ["tables", "ntables", "ctls", "sides", "nctls"]   # zkm_prove_with_traces' order
    assert [p.split()[-1] for p in header_params("zkm_segment_check_ctls")[1:3]] == ["traces", "log_n"]


RUST_PRIM = {"u64": (8, 8), "u32": (4, 4)}


def rust_layout(name, text, memo):
    """(size, align, [(field, offset, size)]) of a #[repr(C)] struct of zkm_hip_sys.rs by the repr(C) rules."""
    if name not in memo:
        body = re.search(r"#\[repr\(C\)\][^{;]*?pub struct %s\s*\{(.*?)\}" % name, text, flags=re.S).group(1)
        off, align, fields = 0, 1, []
        for f, ty in re.findall(r"pub ([a-z_]+):\s*([^,]+?)\s*(?:,(?![^\[]*\])|$)", body.strip()):
            arr = re.match(r"\[(\w+);\s*(\d+)\]$", ty)
            base, count = (arr.group(1), int(arr.group(2))) if arr else (ty, 1)
            s, a = RUST_PRIM[base] if base in RUST_PRIM else rust_layout(base, text, memo)[:2]
            off = (off + a - 1) // a * a
            fields.append((f, off, s * count))
            off += s * count
            align = max(align, a)
        memo[name] = ((off + align - 1) // align * align, align, fields)
    return memo[name]


def test_report_layout_agrees_and_carries_what_the_contract_asks(zkm, tmp_path):
    """The two structs of zkm_check_ctls as the C compiler lays them out (`abi_layout check_ctls`), against the ctypes mirrors and the
    Rust mirrors: total size, alignment, and name, offset and size of every field in declaration order."""
    exe = str(tmp_path / "abi_layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "abi_layout.c")])
    lay = json.loads(subprocess.check_output([exe, "check_ctls"]))
    assert set(lay) == {"zkm_ctl_report", "zkm_ctl_location"} == set(zkm.abi_mirrors_check_ctls())
    rep, loc = lay["zkm_ctl_report"], lay["zkm_ctl_location"]
    # every field of the header's two structs is listed, in order
    header = re.sub(r"/\*.*?\*/", " ", read("include", "zkm_hip.h"), flags=re.S)
    for name in lay:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", re.sub(r"\[[^\]]*\]", "", part))[-1]
                 for decl in filter(None, (d.strip() for d in body.split(";"))) for part in decl.split(",")]
        assert [f[0] for f in lay[name]["fields"]] == names, name
    rust_text = re.sub(r"//[^\n]*", "", read("integration", "rust", "zkm_hip_sys.rs"))
    memo = {}
    for name, m in zkm.abi_mirrors_check_ctls().items():
        want = [tuple(f) for f in lay[name]["fields"]]
        assert [(f, getattr(m, f).offset, getattr(m, f).size) for f, _ in m._fields_] == want, name
        assert C.sizeof(m) == lay[name]["size"] and C.alignment(m) == lay[name]["align"], name
        rust_name = "".join(w.capitalize() for w in name.split("_"))
        assert re.search(r"pub type %s = %s;" % (name, rust_name), rust_text)
        size, align, fields = rust_layout(rust_name, rust_text, memo)
        assert fields == want and (size, align) == (lay[name]["size"], lay[name]["align"]), (name, fields, want)
    fields = {f[0]: (f[1], f[2]) for f in rep["fields"]}
    assert {"kind", "ctl", "attempts", "host_waits", "side", "table", "row", "filter_value", "width", "tuple", "looking_count", "looked_count",
            "looking", "looked"} <= set(fields)
    assert fields["tuple"][1] >= 64 * 8                                              # up to 64 canonical words
    assert fields["looking"][1] >= 8 * loc["size"] and fields["looked"][1] >= 8 * loc["size"]   # at least 8 locations a side
    assert [f[0] for f in loc["fields"]] == ["side", "table", "row"]
    # the plain output of the tool is the fixed set it always printed
    plain = json.loads(subprocess.check_output([exe]))
    assert not set(plain) & set(lay) and "zkm_segment_ops" in plain
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
