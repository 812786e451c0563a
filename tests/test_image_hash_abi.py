"""CPU suite: the C ABI of zkm_image_hash_plan / zkm_image_hash / zkm_images_hash -- exported and declared alike in the header, the Rust
block and the ctypes signatures; zkm_image_pages' layout as the C compiler, ctypes and the Rust mirror see it; and what needs no GPU: null
arguments fail through the error channel."""
import ctypes as C
import json
import os
import re
import subprocess

from .test_boot_abi import header_params, rust_layout
from .test_check_ctls_abi import read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["zkm_image_hash", "zkm_images_hash"]
FIELDS = ["dirty_index", "ndirty", "dirty_words", "known_index", "nknown", "known_words", "pc", "registers"]


def test_symbols_are_exported_and_declared_alike(zkm):
    lib = zkm.load()
    rust = read("integration", "rust", "zkm_hip_sys.rs")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "zkm_amd", "csrc", "libzkmhip.so")]).decode()
    for fn in CALLS + ["zkm_image_hash_plan"]:
        assert hasattr(lib, fn) and fn in zkm.EXPORTS and re.search(r" T %s\b" % fn, exported)
        params = header_params(fn, "size_t" if fn == "zkm_image_hash_plan" else "int")
        assert len(getattr(lib, fn).argtypes) == len(params), fn
        r_args = re.search(r"pub fn %s\(([^)]*)\)" % fn, rust).group(1).split(",")
        # (`in` is a keyword of Rust: the block spells it r#in)
        assert [a.split(":")[0].strip().replace("r#", "") for a in r_args] == [re.sub(r"\[\d+\]", "", p.split()[-1]).lstrip("*") for p in params], fn
    for fn in CALLS:
        params = header_params(fn)
        assert params[0] == "zkm_ctx* ctx" and params[-1] == "char** err" and getattr(lib, fn).restype is C.c_int
    assert lib.zkm_image_hash_plan.restype is C.c_size_t
    # zkm_images_hash is zkm_image_hash with the count in front and one output each per image
    one, many = header_params("zkm_image_hash"), header_params("zkm_images_hash")
    assert many[1] == "size_t nimg" and many[2] == one[1] == "const zkm_image_pages* in" and many[3] == "uint32_t* const* hash_words_out"


def test_pages_layout_agrees(zkm, tmp_path):
    exe = str(tmp_path / "abi_layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "abi_layout.c")])
    lay = json.loads(subprocess.check_output([exe, "image"]))
    assert set(lay) == {"zkm_image_pages"} == set(zkm.abi_mirrors_image_hash())
    want = [tuple(f) for f in lay["zkm_image_pages"]["fields"]]
    assert [f[0] for f in want] == FIELDS
    m = zkm.ImagePagesStruct
    assert [(f, getattr(m, f).offset, getattr(m, f).size) for f, _ in m._fields_] == want
    assert C.sizeof(m) == lay["zkm_image_pages"]["size"] and C.alignment(m) == lay["zkm_image_pages"]["align"]
    assert dict((f[0], f[2]) for f in want)["registers"] == 39 * 4
    rust_text = re.sub(r"//[^\n]*", "", read("integration", "rust", "zkm_hip_sys.rs"))
    assert re.search(r"pub type zkm_image_pages = ZkmImagePages;", rust_text)
    size, align, fields = rust_layout("ZkmImagePages", rust_text)
    assert fields == want and (size, align) == (lay["zkm_image_pages"]["size"], lay["zkm_image_pages"]["align"])
    # the plain output of the tool is the fixed set it always printed
    assert "zkm_image_pages" not in json.loads(subprocess.check_output([exe]))


def test_null_arguments_fail_through_the_error_channel(zkm):
    L = zkm.load()
    pages = zkm.ImagePagesStruct()
    out = (C.c_uint32 * 1024)()
    root, image_id = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
    for call in (lambda e: L.zkm_image_hash(None, C.byref(pages), out, root, image_id, e),
                 lambda e: L.zkm_image_hash(None, None, None, None, None, e),
                 lambda e: L.zkm_images_hash(None, 1, None, None, None, None, e)):
        err = C.c_char_p()
        assert call(C.byref(err)) != 0 and b"null argument" in err.value
        assert call(None) != 0


def test_the_key_and_the_file_are_wired():
    core = read("zkm_amd", "csrc", "core.hip")
    assert 'k == "image_hash_form"' in core and '"image_hash_form"' in read("include", "zkm_hip.h")
    assert "image_hash.hip" in read("zkm_amd", "csrc", "Makefile")
