"""CPU suite: what is particular to the K-segment operations entry points -- zkm_segments_tables, zkm_prove_segments_ops,
zkm_pool_prove_segments_ops and the staged operations (zkm_segment_ops_stage, zkm_staged_ops_get / _ready / _free); tests/test_abi.py
holds every declaration and layout of the C ABI.  They take the arguments the contract names, are bound in Python, and refuse their bad
arguments through the error channel without a GPU."""
import ctypes as C

from .test_abi import declared_alike, prototypes, read

NEW = ["zkm_segments_tables", "zkm_prove_segments_ops", "zkm_pool_prove_segments_ops", "zkm_segment_ops_stage", "zkm_staged_ops_get",
       "zkm_staged_ops_ready", "zkm_staged_ops_free"]


def test_header_declares_them_and_the_library_exports_them(zkm):
    protos = prototypes()
    assert protos["zkm_segments_tables"][1] == [("zkm_ctx*", "ctx"), ("const zkm_stark_config*", "cfg"), ("size_t", "nseg"),
                                                ("const zkm_segment_ops*", "ops"), ("unsigned*", "log_n_out"), ("zkm_staged**", "out"),
                                                ("char**", "err")]
    assert [n for _, n in protos["zkm_prove_segments_ops"][1]] == ["ctx", "cfg", "nseg", "ops", "public_values", "npublic", "proofs_out",
                                                                   "proof_offsets_out", "ctl_challenges_out", "err"]
    assert [n for _, n in protos["zkm_pool_prove_segments_ops"][1]] == ["pool", "cfg", "nseg", "max_stack", "ops", "public_values", "npublic",
                                                                        "proofs_out", "proof_offsets_out", "ctl_challenges_out", "err"]
    assert "typedef struct zkm_staged_ops zkm_staged_ops;" in read("include", "zkm_hip.h")
    for name in NEW:
        declared_alike(zkm, name)


def test_python_binding_has_the_declared_argument_types(zkm):
    L, protos = zkm.load(), prototypes()
    pointer = lambda t: t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer)
    for name in NEW:
        ret, params = protos[name]
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
            if ty in ("const zkm_segment_ops*", "zkm_segment_ops*"):
                assert got._type_ is zkm.SegmentOpsStruct, (name, arg)
    for method in ("segments_tables", "prove_segments_ops", "stage_segment_ops"):
        assert callable(getattr(zkm.Context, method))
    assert callable(zkm.Pool.prove_segments_ops)
    assert all(callable(getattr(zkm.StagedOps, m)) for m in ("ops", "ready", "free", "__enter__", "__exit__"))


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
