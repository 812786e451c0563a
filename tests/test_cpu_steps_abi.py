"""CPU suite: what is particular to the step log (tests/test_abi.py holds every declaration and layout of the C ABI): each *_steps call
is its *_boot call with the step lists between the images and `ops`, a step is 48 bytes of 32-bit words, the file wired into the build."""
import ctypes as C
import re

from .test_abi import c_layouts, declared_alike, prototypes, read, rust_sys_text

NEW = ["zkm_cpu_steps_counts", "zkm_cpu_witness", "zkm_segments_tables_steps", "zkm_prove_segments_ops_steps"]


def test_symbols_are_exported_and_declared_alike(zkm):
    lib, protos = zkm.load(), prototypes()
    for fn in NEW:
        declared_alike(zkm, fn)
        assert protos[fn][0] == "int" and getattr(lib, fn).restype is C.c_int and protos[fn][1][-1] == ("char**", "err"), fn
    for steps, boot in (("zkm_segments_tables_steps", "zkm_segments_tables_boot"), ("zkm_prove_segments_ops_steps", "zkm_prove_segments_ops_boot")):
        s, b = protos[steps][1], protos[boot][1]
        k = [name for _, name in b].index("ops")
        assert s[:k] == b[:k] and s[k + 1:] == b[k:] and s[k] == ("const zkm_cpu_steps*", "steps"), steps
    for method in ("cpu_witness", "segments_tables_steps", "prove_segments_ops_steps", "cpu_steps_counts"):
        assert callable(getattr(zkm.Context, method))
    assert callable(zkm.cpu_steps_counts)


def test_a_step_is_48_bytes_of_words(zkm):
    step = c_layouts()["zkm_cpu_step"]
    assert step["size"] == 48 == zkm.CPU_STEP_DT.itemsize                 # three 16-byte loads a record
    assert [f[0] for f in step["fields"]] == ["pc", "next_pc", "insn", "kind", "flags", "context", "reads"]
    assert "u16" not in re.search(r"pub struct ZkmCpuStep \{(.*?)\}", rust_sys_text(), flags=re.S).group(1)


def test_the_file_is_wired_into_the_build():
    assert "cpu_steps.hip" in read("zkm_amd", "csrc", "Makefile") and "cpu_steps_dev.h" in read("zkm_amd", "csrc", "Makefile")
