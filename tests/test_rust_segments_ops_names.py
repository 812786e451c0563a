"""The K-segment additions to integration/rust: segment_hip.rs -- prove_segments_ops_hip(&[Traces]), the StagedOps owner with Drop, the
pool call -- calls the K-segment entry points (tests/test_abi.py holds their declarations in zkm_hip_sys.rs and that every wrapper names
only declared items) and names only the reference items tests/test_rust_segment_names.py already resolves (that test runs on
the whole file, new code included, and stays as it is)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_rust_names import crate_imports, strip_comments  # noqa: E402


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_segment_hip_names_only_declared_library_items():
    src = strip_comments(read("integration", "rust", "segment_hip.rs"))
    used = set(re.findall(r"\b(zkm_[a-z0-9_]+)\b", src))
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
