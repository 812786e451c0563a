"""CPU suite: the ArithmeticStark witness entry point (zkm_arithmetic_trace) has the fixture's table width and is exported, its Rust
declaration matches the header, and the Rust wrapper packs an Operation into the 3-word layout the kernel reads."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arithmetic_cols_is_the_fixture_width(zkm):
    from . import arith_fixtures as A
    header = open(os.path.join(ROOT, "include", "zkm_hip.h")).read()
    assert {int(v) for v in re.findall(r"#define ZKM_ARITHMETIC_COLS (\d+)", header)} == {54} == {A.NCOLS}
    assert int(re.search(r"#define ZKM_ARITHMETIC_MAX_LOG_N (\d+)", header).group(1)) == 28
    assert zkm.ARITHMETIC_COLS == 54
    rust = open(os.path.join(ROOT, "integration", "rust", "zkm_hip_sys.rs")).read()
    assert re.search(r"pub const ZKM_ARITHMETIC_COLS: usize = 54;", rust)


def test_symbol_is_exported(zkm):
    L = zkm.load()
    assert hasattr(L, "zkm_arithmetic_trace") and "zkm_arithmetic_trace" in zkm.EXPORTS
    assert C.CDLL(zkm._LIB_PATH).zkm_arithmetic_trace


def test_rust_sys_declaration_matches_the_header():
    from .test_abi import prototypes, rust_functions
    c, r = prototypes()["zkm_arithmetic_trace"][1], rust_functions()["zkm_arithmetic_trace"][1]
    assert [n for _, n in c] == [n for _, n in r] == ["ctx", "ops", "nops", "log_n", "out_dev", "natural_rows_out", "err"]
    assert ("const uint32_t*", "ops") in c and ("*const u32", "ops") in r


def test_rust_wrapper_packs_filter_and_inputs():
    """arithmetic_op_words (integration/rust/arithmetic_hip.rs): {operator.row_filter(), input0, input1} per op -- the order of
    arith_fixtures.generate_trace's (op, a, b) -- and both Rust entry points go through it, the sizing call and the trace call."""
    src = open(os.path.join(ROOT, "integration", "rust", "arithmetic_hip.rs")).read()
    body = src[src.index("pub fn arithmetic_op_words"):]
    body = body[:body.index("\n}\n")]
    packed = re.search(r"extend_from_slice\(&\[(.*?)\]\)", body, flags=re.S).group(1)
    fields = [f.strip() for f in re.split(r",\s*\n", packed) if f.strip().rstrip(",")]
    assert [f.rstrip(",") for f in fields] == ["operator.row_filter() as u32", "*input0", "*input1"]
    for fn in ("arithmetic_trace_dev", "arithmetic_trace_hip"):
        assert re.search(r"pub fn %s\b" % fn, src)
    dev = src[src.index("pub fn arithmetic_trace_dev"):]
    dev = dev[:dev.index("\n}\n")]
    assert dev.count("zkm_arithmetic_trace(") == 2 and "std::ptr::null_mut(), &mut natural" in dev
    assert "arithmetic_op_words(arithmetic_ops)" in dev
    hip = src[src.index("pub fn arithmetic_trace_hip"):]
    assert "arithmetic_trace_dev(ctx, arithmetic_ops)" in hip[:hip.index("\n}\n")]
