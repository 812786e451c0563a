"""CPU suite: what is particular to the zkm_*_boot calls (tests/test_abi.py holds every declaration and layout of the C ABI): each call
is its plain call with the image in front of `ops`, zkm_boot_image has the fields the contract names, and what needs no GPU: null
arguments fail through the error channel."""
import ctypes as C

from .test_abi import c_layouts, declared_alike, prototypes, read

NEW = ["zkm_segment_tables_boot", "zkm_segments_tables_boot", "zkm_prove_segment_ops_boot", "zkm_prove_segments_ops_boot", "zkm_boot_witness"]
FIELDS = ["addrs", "values", "nwords", "npages", "entry", "check", "pre_hash_root", "pre_image_id"]


def test_symbols_are_exported_and_declared_alike(zkm):
    lib, protos = zkm.load(), prototypes()
    for fn in NEW + ["zkm_boot_counts"]:
        declared_alike(zkm, fn)
    for fn in NEW:
        ret, params = protos[fn]
        assert params[0] == ("zkm_ctx*", "ctx") and params[-1] == ("char**", "err") and ret == "int" and getattr(lib, fn).restype is C.c_int
    assert protos["zkm_boot_counts"][0] == "void"
    for boot, plain in (("zkm_segment_tables_boot", "zkm_segment_tables"), ("zkm_segments_tables_boot", "zkm_segments_tables"),
                        ("zkm_prove_segment_ops_boot", "zkm_prove_segment_ops"), ("zkm_prove_segments_ops_boot", "zkm_prove_segments_ops")):
        b, p = protos[boot][1], protos[plain][1]
        k = [name for _, name in p].index("ops")
        assert b[:k] == p[:k] and b[k + 1:] == p[k:] and b[k][0] == "const zkm_boot_image*" and b[k][1].startswith("image"), boot


def test_image_fields_are_the_contracts(zkm):
    assert [f[0] for f in c_layouts()["zkm_boot_image"]["fields"]] == FIELDS == [f for f, _ in zkm.BootImageStruct._fields_]


def test_null_arguments_fail_through_the_error_channel(zkm):
    L = zkm.load()
    cfg = zkm.StarkConfig()
    L.zkm_standard_config(C.byref(cfg))
    im, ops, lg = zkm.BootImageStruct(), zkm.SegmentOpsStruct(), (C.c_uint * 12)()
    for call in (lambda e: L.zkm_segment_tables_boot(None, C.byref(cfg), C.byref(im), C.byref(ops), lg, None, e),
                 lambda e: L.zkm_segments_tables_boot(None, C.byref(cfg), 1, None, None, lg, None, e),
                 lambda e: L.zkm_prove_segment_ops_boot(None, C.byref(cfg), None, C.byref(ops), None, 0, None, None, None, e),
                 lambda e: L.zkm_prove_segments_ops_boot(None, C.byref(cfg), 0, None, None, None, None, None, None, None, e),
                 lambda e: L.zkm_boot_witness(None, C.byref(im), None, None, None, None, None, e)):
        err = C.c_char_p()
        assert call(C.byref(err)) != 0 and b"null argument" in err.value
        assert call(None) != 0


def test_the_key_and_the_file_are_wired():
    core = read("zkm_amd", "csrc", "core.hip")
    assert 'k == "boot_chain_quad"' in core and '"boot_chain_quad"' in read("include", "zkm_hip.h")
    assert "bootstrap.hip" in read("zkm_amd", "csrc", "Makefile")
