"""CPU suite: the C ABI of the step log -- the four entry points exported and declared alike in the header, the Rust block and the ctypes
signatures; zkm_cpu_step's and zkm_cpu_steps' layout as the C compiler, numpy / ctypes and the Rust mirror see it; the file wired into
the build."""
import ctypes as C
import json
import os
import re
import subprocess

from .test_boot_abi import header_params, rust_layout
from .test_check_ctls_abi import read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["zkm_cpu_steps_counts", "zkm_cpu_witness", "zkm_segments_tables_steps", "zkm_prove_segments_ops_steps"]


def test_symbols_are_exported_and_declared_alike(zkm):
    lib = zkm.load()
    rust = read("integration", "rust", "zkm_hip_sys.rs")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "zkm_amd", "csrc", "libzkmhip.so")]).decode()
    for fn in NEW:
        assert hasattr(lib, fn) and fn in zkm.EXPORTS and re.search(r" T %s\b" % fn, exported)
        params = header_params(fn)
        assert len(getattr(lib, fn).argtypes) == len(params) and getattr(lib, fn).restype is C.c_int, fn
        r_args = re.search(r"pub fn %s\(([^)]*)\)" % fn, rust).group(1).split(",")
        assert [a.split(":")[0].strip() for a in r_args] == [p.split()[-1].lstrip("*") for p in params], fn
        assert params[-1] == "char** err"
    # each *_steps call is its *_boot call with the step lists between the images and ops
    for steps, boot in (("zkm_segments_tables_steps", "zkm_segments_tables_boot"), ("zkm_prove_segments_ops_steps", "zkm_prove_segments_ops_boot")):
        s, b = header_params(steps), header_params(boot)
        k = [x.split()[-1] for x in b].index("ops")
        assert s[:k] == b[:k] and s[k + 1:] == b[k:] and s[k] == "const zkm_cpu_steps* steps", steps
    for method in ("cpu_witness", "segments_tables_steps", "prove_segments_ops_steps", "cpu_steps_counts"):
        assert callable(getattr(zkm.Context, method))
    assert callable(zkm.cpu_steps_counts)


def test_step_layouts_agree(zkm, tmp_path):
    exe = str(tmp_path / "abi_layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "abi_layout.c")])
    lay = json.loads(subprocess.check_output([exe, "steps"]))
    mirrors = zkm.abi_mirrors_cpu_steps()
    assert set(lay) == {"zkm_cpu_step", "zkm_cpu_steps"} == set(mirrors)
    assert lay["zkm_cpu_step"]["size"] == 48                 # three 16-byte loads a record
    step = [tuple(f) for f in lay["zkm_cpu_step"]["fields"]]
    assert [f[0] for f in step] == ["pc", "next_pc", "insn", "kind", "flags", "context", "reads"]
    dt = mirrors["zkm_cpu_step"]
    assert [(f, dt.fields[f][1], dt.fields[f][0].itemsize) for f in dt.names] == step and dt.itemsize == 48
    lst = [tuple(f) for f in lay["zkm_cpu_steps"]["fields"]]
    m = mirrors["zkm_cpu_steps"]
    assert [(f, getattr(m, f).offset, getattr(m, f).size) for f, _ in m._fields_] == lst
    assert C.sizeof(m) == lay["zkm_cpu_steps"]["size"] and C.alignment(m) == lay["zkm_cpu_steps"]["align"]
    rust_text = re.sub(r"//[^\n]*", "", read("integration", "rust", "zkm_hip_sys.rs"))
    for name, rust_name, want in (("zkm_cpu_step", "ZkmCpuStep", step), ("zkm_cpu_steps", "ZkmCpuSteps", lst)):
        assert re.search(r"pub type %s = %s;" % (name, rust_name), rust_text)
        size, align, fields = rust_layout(rust_name, rust_text)
        assert fields == want and (size, align) == (lay[name]["size"], lay[name]["align"]), name
    assert "u16" not in re.search(r"pub struct ZkmCpuStep \{(.*?)\}", rust_text, flags=re.S).group(1)
    # the plain output of the tool is the fixed set it always printed
    assert not set(lay) & set(json.loads(subprocess.check_output([exe])))


def test_the_file_is_wired_into_the_build():
    assert "cpu_steps.hip" in read("zkm_amd", "csrc", "Makefile") and "cpu_steps_dev.h" in read("zkm_amd", "csrc", "Makefile")
