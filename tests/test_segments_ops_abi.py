"""CPU suite: the K-segment operations entry points -- zkm_segments_tables, zkm_prove_segments_ops, zkm_pool_prove_segments_ops and the
staged operations (zkm_segment_ops_stage, zkm_staged_ops_get / _ready / _free) -- are declared in the header, exported by the library,
bound in Python with the declared argument types, and refuse their bad arguments through the error channel without a GPU; no existing
struct of the C ABI changed its size."""
import ctypes as C
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
NEW = ["zkm_segments_tables", "zkm_prove_segments_ops", "zkm_pool_prove_segments_ops", "zkm_segment_ops_stage", "zkm_staged_ops_get",
       "zkm_staged_ops_ready", "zkm_staged_ops_free"]
# sizeof of every struct tools/abi_layout.c printed before these entry points existed (zkm_segment_ops: locked, 36 x 8)
SIZES = {"zkm_challenger": 232, "zkm_stark_config": 28, "zkm_proof_layout": 216, "zkm_proof_query_layout": 464, "zkm_column": 24,
         "zkm_colset": 32, "zkm_ctl_table": 72, "zkm_ctl_z": 32, "zkm_ctl_side": 8, "zkm_cross_table_lookup": 16, "zkm_table_input": 48,
         "zkm_fri_poly": 8, "zkm_fri_batch": 32, "zkm_segment_ops": 288}


def header_prototypes():
    """{name: (return type, [(type, name)])} of the new exports, from the header text."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "zkm_hip.h")).read(), flags=re.S)
    out = {}
    for name in NEW:
        ret, args = re.search(r"\b(int|void)\s+%s\(([^)]*)\)\s*;" % name, text).groups()
        params = []
        for a in args.split(","):
            ty, arg = re.match(r"\s*(.*?)(\w+)\s*$", a, flags=re.S).groups()
            params.append((re.sub(r"\s+", " ", ty).strip(), arg))
        out[name] = (ret, params)
    return out


def test_header_declares_them_and_the_library_exports_them(zkm):
    protos = header_prototypes()
    assert protos["zkm_segments_tables"][1] == [("zkm_ctx*", "ctx"), ("const zkm_stark_config*", "cfg"), ("size_t", "nseg"),
                                                ("const zkm_segment_ops*", "ops"), ("unsigned*", "log_n_out"), ("zkm_staged**", "out"),
                                                ("char**", "err")]
    assert [n for _, n in protos["zkm_prove_segments_ops"][1]] == ["ctx", "cfg", "nseg", "ops", "public_values", "npublic", "proofs_out",
                                                                   "proof_offsets_out", "ctl_challenges_out", "err"]
    assert [n for _, n in protos["zkm_pool_prove_segments_ops"][1]] == ["pool", "cfg", "nseg", "max_stack", "ops", "public_values", "npublic",
                                                                        "proofs_out", "proof_offsets_out", "ctl_challenges_out", "err"]
    assert "typedef struct zkm_staged_ops zkm_staged_ops;" in open(os.path.join(ROOT, "include", "zkm_hip.h")).read()
    dynamic = subprocess.check_output(["nm", "-D", "--defined-only", zkm._LIB_PATH], text=True)
    exported = set(re.findall(r" T (zkm_\w+)", dynamic))
    assert set(NEW) <= exported, set(NEW) - exported
    assert set(NEW) <= set(zkm.EXPORTS)


def test_python_binding_has_the_declared_argument_types(zkm):
    L = zkm.load()
    pointer = lambda t: t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer)
    for name, (ret, params) in header_prototypes().items():
        fn = getattr(L, name)
        assert fn.restype is (C.c_int if ret == "int" else None), name
        assert len(fn.argtypes) == len(params), name
        for got, (ty, arg) in zip(fn.argtypes, params):
            if ty == "size_t":
                assert got is C.c_size_t, (name, arg)
            elif ty == "int":
                assert got is C.c_int, (name, arg)
            else:
                assert ty.endswith("*") and pointer(got), (name, arg)
            if ty == "const zkm_segment_ops*" or ty == "zkm_segment_ops*":
                assert got._type_ is zkm.SegmentOpsStruct, (name, arg)
    for method in ("segments_tables", "prove_segments_ops", "stage_segment_ops"):
        assert callable(getattr(zkm.Context, method))
    assert callable(zkm.Pool.prove_segments_ops)
    assert all(callable(getattr(zkm.StagedOps, m)) for m in ("ops", "ready", "free", "__enter__", "__exit__"))


def test_existing_struct_sizes_are_unchanged(tmp_path):
    exe = str(tmp_path / "abi_layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "abi_layout.c")])
    lay = json.loads(subprocess.check_output([exe]))
    assert {k: v["size"] for k, v in lay.items()} == SIZES
    # the file also holds the new prototypes to their argument types (a mismatch would have failed the build above)
    text = open(os.path.join(ROOT, "tools", "abi_layout.c")).read()
    assert all("= %s)" % name in text for name in NEW)


def test_bad_arguments_are_refused_without_a_gpu(zkm):
    """Null contexts, pools and handles end in the error channel (or the documented status), not in a crash."""
    import numpy as np
    L = zkm.load()
    ops = zkm.SegmentOps(np.zeros((64, 259), dtype=np.uint64), np.zeros((1, 6), dtype=np.uint64))
    cfg = zkm.StarkConfig()
    L.zkm_standard_config(C.byref(cfg))
    st, lg, err = ops.struct(), (C.c_uint * 12)(), C.c_char_p()
    assert L.zkm_segments_tables(None, C.byref(cfg), 1, C.byref(st), lg, None, C.byref(err)) == 1
    assert b"zkm_segments_tables: null argument" in err.value
    offs = (C.c_size_t * 13)()
    assert L.zkm_prove_segments_ops(None, C.byref(cfg), 1, C.byref(st), None, None, None, offs, None, C.byref(err)) == 1
    assert b"zkm_prove_segments_ops: null argument" in err.value
    assert L.zkm_pool_prove_segments_ops(None, C.byref(cfg), 1, 0, C.byref(st), None, None, None, offs, None, C.byref(err)) == 1
    assert b"zkm_pool_prove_segments_ops: null argument" in err.value
    h = C.c_void_p()
    assert L.zkm_segment_ops_stage(None, C.byref(st), C.byref(h), C.byref(err)) == 1 and not h.value
    out = zkm.SegmentOpsStruct()
    assert L.zkm_staged_ops_get(None, C.byref(out)) == 1 and L.zkm_staged_ops_ready(None, 0) == 1
    L.zkm_staged_ops_free(None)
