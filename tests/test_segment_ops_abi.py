"""CPU suite: zkm_segment_tables / zkm_prove_segment_ops -- exported, one zkm_segment_ops layout in the header, the Rust #[repr(C)] mirror
and the ctypes mirror, Rust declarations that match the header -- and the fixture segment built from raw lists proves under the oracle."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
C_WIDTH = {"const uint64_t*": 8, "const uint32_t*": 8, "const uint8_t*": 8, "size_t": 8}
RUST_WIDTH = {"*const u64": 8, "*const u32": 8, "*const u8": 8, "usize": 8}


def header_fields():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "zkm_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} zkm_segment_ops;", text).group(1)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ty, name = re.match(r"(const \w+\*|size_t)\s*(\w+)$", decl).groups()
        out.append((name, ty))
    return out


def rust_fields():
    from .test_abi import rust_structs
    return rust_structs()["zkm_segment_ops"]


def test_symbols_are_exported(zkm):
    L = zkm.load()
    for name in ("zkm_segment_tables", "zkm_prove_segment_ops"):
        assert hasattr(L, name) and name in zkm.EXPORTS
        assert getattr(C.CDLL(zkm._LIB_PATH), name)


def test_struct_fields_agree_in_header_rust_and_ctypes(zkm):
    """Same fields, same order, same widths: the header, the Rust mirror and the ctypes mirror; one pointer group and one count per field
    of the reference's Traces, in its order."""
    from .test_abi import c_to_rust
    hdr = header_fields()
    rust = rust_fields()
    assert [n for n, _ in hdr] == [n for n, _ in rust] == [n for n, _ in zkm.SegmentOpsStruct._fields_]
    assert [c_to_rust(t, ()) for _, t in hdr] == [t for _, t in rust]
    assert [C_WIDTH[t] for _, t in hdr] == [RUST_WIDTH[t] for _, t in rust] == \
        [getattr(zkm.SegmentOpsStruct, n).size for n, _ in zkm.SegmentOpsStruct._fields_]
    assert C.sizeof(zkm.SegmentOpsStruct) == 8 * len(hdr)
    counts = [n for n, t in hdr if t == "size_t"]
    assert counts == ["ncpu_rows", "narithmetic", "nlogic", "nmemory", "nposeidon", "nposeidon_sponge", "nkeccak", "nkeccak_sponge",
                      "nsha_extend", "nsha_extend_sponge", "nsha_compress", "nsha_compress_sponge"]


def test_rust_declarations_match_the_header():
    from .test_abi import prototypes, rust_functions
    for fn, want in (("zkm_segment_tables", ["ctx", "cfg", "ops", "log_n_out", "out", "err"]),
                     ("zkm_prove_segment_ops", ["ctx", "cfg", "ops", "public_values", "npublic", "proofs_out", "proof_offsets_out",
                                                "ctl_challenges_out", "err"])):
        c, r = prototypes()[fn][1], rust_functions()[fn][1]
        assert [n for _, n in c] == [n for _, n in r] == want, fn
        assert ("const zkm_segment_ops*", "ops") in c and ("*const zkm_segment_ops", "ops") in r


def test_sizing_needs_a_context(zkm):
    """Both calls refuse a null context (the heights need the device) through the error channel."""
    from . import segment_ops_fixtures as SF
    import numpy as np
    L = zkm.load()
    ops = zkm.SegmentOps(np.zeros((64, 259), dtype=np.uint64), np.zeros((1, 6), dtype=np.uint64))
    cfg = zkm.StarkConfig()
    L.zkm_standard_config(C.byref(cfg))
    st, lg, err = ops.struct(), (C.c_uint * 12)(), C.c_char_p()
    assert L.zkm_segment_tables(None, C.byref(cfg), C.byref(st), lg, None, C.byref(err)) == 1
    assert b"zkm_segment_tables: null argument" in err.value
    offs = (C.c_size_t * 13)()
    assert L.zkm_prove_segment_ops(None, C.byref(cfg), C.byref(st), None, 0, None, offs, None, C.byref(err)) == 1
    assert SF.log2_height(0, 64) == 6 and SF.log2_height(65, 64) == 7 and SF.log2_height(64, 64) == 6


def test_fixture_tables_prove_under_the_oracle(oracle):
    """Fixture infrastructure: the twelve tables written from the raw lists at the reference's heights are consistent (all fifteen
    lookups) and the oracle's proof of them verifies."""
    from . import segment_ops_fixtures as SF
    raw, tables, ctls = SF.build_segment_ops(oracle)
    assert [t[3] for t in tables] == SF.reference_log_ns(raw)
    assert all(t[1].size == t[2] << t[3] for t in tables)
    assert oracle.check_ctls(tables, ctls) == 0
    proofs, chal, offs = oracle.prove_with_traces(tables, ctls, public_values=[1, 2, 3])
    assert oracle.verify_all(tables, ctls, proofs, chal, public_values=[1, 2, 3]) == 0
