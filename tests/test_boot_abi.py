"""CPU suite: the C ABI of the zkm_*_boot calls -- exported and declared alike in the header, the Rust block and the ctypes signatures;
zkm_boot_image's layout as the C compiler, ctypes and the Rust mirror see it; and what needs no GPU: null arguments fail through the error
channel."""
import ctypes as C
import json
import os
import re
import subprocess

from .test_check_ctls_abi import read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["zkm_segment_tables_boot", "zkm_segments_tables_boot", "zkm_prove_segment_ops_boot", "zkm_prove_segments_ops_boot", "zkm_boot_witness"]
FIELDS = ["addrs", "values", "nwords", "npages", "entry", "check", "pre_hash_root", "pre_image_id"]


def header_params(fn, ret="int"):
    text = re.sub(r"/\*.*?\*/", " ", read("include", "zkm_hip.h"), flags=re.S)
    return [a.strip() for a in re.search(r"\b%s\s+%s\(([^)]*)\)\s*;" % (ret, fn), text).group(1).split(",")]


def rust_layout(name, text):
    """(size, align, [(field, offset, size)]) of a #[repr(C)] struct of pointers, usize, u32 and byte arrays, by the repr(C) rules."""
    prim = {"usize": (8, 8), "u32": (4, 4), "u8": (1, 1), "u64": (8, 8)}
    body = re.search(r"#\[repr\(C\)\][^{;]*?pub struct %s\s*\{(.*?)\}" % name, text, flags=re.S).group(1)
    off, align, fields = 0, 1, []
    for f, ty in re.findall(r"pub ([a-z_]+):\s*([^,]+?)\s*(?:,(?![^\[]*\])|$)", body.strip()):
        arr = re.match(r"\[(\w+);\s*(\d+)\]$", ty)
        base, count = (arr.group(1), int(arr.group(2))) if arr else (ty, 1)
        s, a = (8, 8) if base.startswith("*") else prim[base]
        off = (off + a - 1) // a * a
        fields.append((f, off, s * count))
        off += s * count
        align = max(align, a)
    return (off + align - 1) // align * align, align, fields


def test_symbols_are_exported_and_declared_alike(zkm):
    lib = zkm.load()
    rust = read("integration", "rust", "zkm_hip_sys.rs")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "zkm_amd", "csrc", "libzkmhip.so")]).decode()
    for fn in NEW + ["zkm_boot_counts"]:
        assert hasattr(lib, fn) and fn in zkm.EXPORTS and re.search(r" T %s\b" % fn, exported)
        params = header_params(fn, "void" if fn == "zkm_boot_counts" else "int")
        assert len(getattr(lib, fn).argtypes) == len(params), fn
        r_args = re.search(r"pub fn %s\(([^)]*)\)" % fn, rust).group(1).split(",")
        assert [a.split(":")[0].strip() for a in r_args] == [p.split()[-1].lstrip("*") for p in params], fn
    for fn in NEW:
        params = header_params(fn)
        assert params[0] == "zkm_ctx* ctx" and params[-1] == "char** err" and getattr(lib, fn).restype is C.c_int
    # each *_boot call is its plain call with the image(s) in front of ops
    for boot, plain in (("zkm_segment_tables_boot", "zkm_segment_tables"), ("zkm_segments_tables_boot", "zkm_segments_tables"),
                        ("zkm_prove_segment_ops_boot", "zkm_prove_segment_ops"), ("zkm_prove_segments_ops_boot", "zkm_prove_segments_ops")):
        b, p = header_params(boot), header_params(plain)
        k = [x.split()[-1] for x in p].index("ops")
        assert b[:k] == p[:k] and b[k + 1:] == p[k:] and b[k].startswith("const zkm_boot_image* image"), boot


def test_image_layout_agrees(zkm, tmp_path):
    exe = str(tmp_path / "abi_layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "abi_layout.c")])
    lay = json.loads(subprocess.check_output([exe, "boot"]))
    assert set(lay) == {"zkm_boot_image"} == set(zkm.abi_mirrors_boot())
    want = [tuple(f) for f in lay["zkm_boot_image"]["fields"]]
    assert [f[0] for f in want] == FIELDS
    m = zkm.BootImageStruct
    assert [(f, getattr(m, f).offset, getattr(m, f).size) for f, _ in m._fields_] == want
    assert C.sizeof(m) == lay["zkm_boot_image"]["size"] and C.alignment(m) == lay["zkm_boot_image"]["align"]
    rust_text = re.sub(r"//[^\n]*", "", read("integration", "rust", "zkm_hip_sys.rs"))
    assert re.search(r"pub type zkm_boot_image = ZkmBootImage;", rust_text)
    size, align, fields = rust_layout("ZkmBootImage", rust_text)
    assert fields == want and (size, align) == (lay["zkm_boot_image"]["size"], lay["zkm_boot_image"]["align"])
    # the plain output of the tool is the fixed set it always printed
    assert "zkm_boot_image" not in json.loads(subprocess.check_output([exe]))


def test_null_arguments_fail_through_the_error_channel(zkm):
    L = zkm.load()
    cfg = zkm.StarkConfig()
    L.zkm_standard_config(C.byref(cfg))
    im, ops, lg = zkm.BootImageStruct(), zkm.SegmentOpsStruct(), (C.c_uint * 12)()
    for call in (lambda e: L.zkm_segment_tables_boot(None, C.byref(cfg), C.byref(im), C.byref(ops), lg, None, e),
                 lambda e: L.zkm_segments_tables_boot(None, C.byref(cfg), 1, None, None, lg, None, e),
                 lambda e: L.zkm_prove_segment_ops_boot(None, C.byref(cfg), None, C.byref(ops), None, 0, None, None, None, e),
                 lambda e: L.zkm_prove_segments_ops_boot(None, C.byref(cfg), 0, None, None, None, None, None, None, None, e),
                 lambda e: L.zkm_boot_witness(None, C.byref(im), None, None, None, None, None, e)):
        err = C.c_char_p()
        assert call(C.byref(err)) != 0 and b"null argument" in err.value
        assert call(None) != 0


def test_the_key_and_the_file_are_wired():
    core = read("zkm_amd", "csrc", "core.hip")
    assert 'k == "boot_chain_quad"' in core and '"boot_chain_quad"' in read("include", "zkm_hip.h")
    assert "bootstrap.hip" in read("zkm_amd", "csrc", "Makefile")
