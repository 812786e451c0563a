"""CPU suite: the MemoryStark witness entry point (zkm_memory_trace) agrees with the oracle's table width, and the Rust wrapper packs a
MemoryOp into the 6-word layout the oracle and the kernel read."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_memory_cols_is_the_oracle_width(zkm, oracle):
    header = open(os.path.join(ROOT, "include", "zkm_hip.h")).read()
    assert int(re.search(r"#define ZKM_MEMORY_COLS (\d+)", header).group(1)) == 13
    assert zkm.MEMORY_COLS == 13
    assert hasattr(zkm.load(), "zkm_memory_trace") and "zkm_memory_trace" in zkm.EXPORTS
    ops = np.array([(0, 1, 8, 5, 0, 77), (0, 1, 8, 6, 1, 77)], dtype=np.uint64)
    for log_n in (1, 3):
        trace, natural = oracle.memory_trace(ops, log_n)
        assert trace.size == zkm.MEMORY_COLS << log_n and natural == 2
    rust = open(os.path.join(ROOT, "integration", "rust", "zkm_hip_sys.rs")).read()
    assert re.search(r"pub const ZKM_MEMORY_COLS: usize = 13;", rust)


def test_rust_sys_declaration_matches_the_header():
    from .test_abi import prototypes, rust_functions
    c, r = prototypes()["zkm_memory_trace"][1], rust_functions()["zkm_memory_trace"][1]
    assert [n for _, n in c] == [n for _, n in r] == ["ctx", "ops", "nops", "log_n", "out_dev", "natural_rows_out", "err"]


def test_rust_wrapper_packs_fields_in_the_oracle_order():
    """memory_op_words (integration/rust/memory_hip.rs): {context, segment, virt, timestamp, is_read, value} per op -- the order of
    zko_memory_trace / Oracle.memory_trace -- with is_read = (kind == MemoryOpKind::Read), and filter-false ops refused."""
    src = open(os.path.join(ROOT, "integration", "rust", "memory_hip.rs")).read()
    body = src[src.index("pub fn memory_op_words"):]
    body = body[:body.index("\n}\n")]
    packed = re.search(r"extend_from_slice\(&\[(.*?)\]\)", body, flags=re.S).group(1)
    fields = [f.strip() for f in re.split(r",\s*\n", packed) if f.strip()]
    assert fields == ["op.address.context as u64", "op.address.segment as u64", "op.address.virt as u64", "op.timestamp as u64",
                      "matches!(op.kind, MemoryOpKind::Read) as u64", "op.value as u64"]
    assert re.search(r"ensure!\(op\.filter", body)
    oracle_doc = open(os.path.join(ROOT, "oracle", "oracle_py.py")).read()
    assert "ops: nops x 6 (context, segment, virt, timestamp, is_read, value)" in oracle_doc
    # both Rust entry points go through the packing, the sizing call and the trace call
    for fn in ("memory_trace_dev", "memory_trace_hip"):
        assert re.search(r"pub fn %s\b" % fn, src)
    dev = src[src.index("pub fn memory_trace_dev"):]
    dev = dev[:dev.index("\n}\n")]
    assert dev.count("zkm_memory_trace(") == 2 and "std::ptr::null_mut(), &mut natural" in dev
