"""The K-segment additions to integration/rust: zkm_hip_sys.rs declares the new exports with the header's argument names and pointer
shapes, and segment_hip.rs -- prove_segments_ops_hip(&[Traces]), the StagedOps owner with Drop, the pool call -- names only library
items that zkm_hip_sys.rs declares and only the reference items tests/test_rust_segment_names.py already resolves (that test runs on
the whole file, new code included, and stays as it is)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_rust_names import crate_imports, strip_comments  # noqa: E402

NEW = ["zkm_segments_tables", "zkm_prove_segments_ops", "zkm_pool_prove_segments_ops", "zkm_segment_ops_stage", "zkm_staged_ops_get",
       "zkm_staged_ops_ready", "zkm_staged_ops_free"]
C_TO_RUST = {"zkm_ctx*": "*mut zkm_ctx", "zkm_pool*": "*mut zkm_pool", "const zkm_stark_config*": "*const zkm_stark_config", "size_t": "usize",
             "int": "c_int", "const zkm_segment_ops*": "*const zkm_segment_ops", "zkm_segment_ops*": "*mut zkm_segment_ops",
             "unsigned*": "*mut c_uint", "zkm_staged**": "*mut *mut zkm_staged", "zkm_staged_ops**": "*mut *mut zkm_staged_ops",
             "zkm_staged_ops*": "*mut zkm_staged_ops", "char**": "*mut *mut c_char", "const uint64_t* const*": "*const *const u64",
             "const size_t*": "*const usize", "uint64_t* const*": "*const *mut u64", "size_t*": "*mut usize"}


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_sys_declarations_match_the_header():
    header = re.sub(r"/\*.*?\*/", " ", read("include", "zkm_hip.h"), flags=re.S)
    rust = strip_comments(read("integration", "rust", "zkm_hip_sys.rs"))
    assert re.search(r"pub (enum|struct) zkm_staged_ops\b", rust)
    for fn in NEW:
        ret, c_args = re.search(r"\b(int|void)\s+%s\(([^)]*)\)\s*;" % fn, header).groups()
        r_args, r_ret = re.search(r"pub fn %s\(([^)]*)\)\s*(->\s*c_int)?\s*;" % fn, rust).groups()
        assert bool(r_ret) == (ret == "int"), fn
        c_params = [re.match(r"\s*(.*?)(\w+)\s*$", a, flags=re.S).groups() for a in c_args.split(",")]
        r_params = [re.match(r"\s*(\w+):\s*(.+?)\s*$", a, flags=re.S).groups() for a in r_args.split(",")]
        assert [n for _, n in c_params] == [n for n, _ in r_params], fn
        assert [C_TO_RUST[re.sub(r"\s+", " ", t).strip()] for t, _ in c_params] == [t for _, t in r_params], fn


def test_segment_hip_names_only_declared_library_items():
    sys_rs = strip_comments(read("integration", "rust", "zkm_hip_sys.rs"))
    declared = set(re.findall(r"pub fn (zkm_\w+)\s*\(", sys_rs)) | set(re.findall(r"pub (?:struct|enum) (zkm_\w+)", sys_rs))
    src = strip_comments(read("integration", "rust", "segment_hip.rs"))
    used = set(re.findall(r"\b(zkm_[a-z0-9_]+)\b", src))
    assert used <= declared, used - declared
    assert {"zkm_prove_segments_ops", "zkm_pool_prove_segments_ops", "zkm_segment_ops_stage", "zkm_staged_ops_get", "zkm_staged_ops_ready",
            "zkm_staged_ops_free"} <= used


def test_the_new_wrappers_exist_with_the_shapes_the_issue_names():
    src = strip_comments(read("integration", "rust", "segment_hip.rs"))
    assert re.search(r"pub fn prove_segments_ops_hip<F: PrimeField64>\(ctx: \*mut zkm_ctx, segments: &\[Traces<F>\]", src)
    assert re.search(r"pub struct StagedOps\(\*mut zkm_staged_ops\);", src)
    drop = re.search(r"impl Drop for StagedOps \{(.*?)\n\}", src, flags=re.S).group(1)
    assert "zkm_staged_ops_free(self.0)" in drop
    assert re.search(r"pub fn prove_segments_ops_pool_hip<F: PrimeField64>\(pool: \*mut zkm_pool, segments: &\[Traces<F>\]", src)
    # sizing, then proving: both calls of every K-segment entry point go through one helper
    assert src.count("size_then_prove(") == 3
    # no reference item beyond the ones the single-segment file already uses
    paths = {(p, i) for p, i in crate_imports(src)}
    assert paths == {(("arithmetic_hip",), "arithmetic_op_words"), (("memory_hip",), "memory_op_words"),
                     (("witness", "memory"), "MemoryAddress"), (("witness", "traces"), "Traces")}, paths
