"""CPU suite: what is particular to zkm_image_hash_plan / zkm_image_hash / zkm_images_hash (tests/test_abi.py holds every declaration and
layout of the C ABI): the many-image call is the one-image call with the count in front, zkm_image_pages has the fields the contract
names, and what needs no GPU: null arguments fail through the error channel."""
import ctypes as C

from .test_abi import c_layouts, declared_alike, prototypes, read

CALLS = ["zkm_image_hash", "zkm_images_hash"]
FIELDS = ["dirty_index", "ndirty", "dirty_words", "known_index", "nknown", "known_words", "pc", "registers"]


def test_symbols_are_exported_and_declared_alike(zkm):
    lib, protos = zkm.load(), prototypes()
    for fn in CALLS + ["zkm_image_hash_plan"]:
        declared_alike(zkm, fn)
    for fn in CALLS:
        ret, params = protos[fn]
        assert params[0] == ("zkm_ctx*", "ctx") and params[-1] == ("char**", "err") and ret == "int" and getattr(lib, fn).restype is C.c_int
    assert protos["zkm_image_hash_plan"][0] == "size_t" and lib.zkm_image_hash_plan.restype is C.c_size_t
    one, many = protos["zkm_image_hash"][1], protos["zkm_images_hash"][1]
    assert many[1] == ("size_t", "nimg") and many[2] == one[1] == ("const zkm_image_pages*", "in") and many[3] == ("uint32_t* const*", "hash_words_out")


def test_pages_fields_are_the_contracts(zkm):
    want = c_layouts()["zkm_image_pages"]["fields"]
    assert [f[0] for f in want] == FIELDS == [f for f, _ in zkm.ImagePagesStruct._fields_]
    assert dict((f[0], f[2]) for f in want)["registers"] == 39 * 4


def test_null_arguments_fail_through_the_error_channel(zkm):
    L = zkm.load()
    pages = zkm.ImagePagesStruct()
    out = (C.c_uint32 * 1024)()
    root, image_id = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
    for call in (lambda e: L.zkm_image_hash(None, C.byref(pages), out, root, image_id, e),
                 lambda e: L.zkm_image_hash(None, None, None, None, None, e),
                 lambda e: L.zkm_images_hash(None, 1, None, None, None, None, e)):
        err = C.c_char_p()
        assert call(C.byref(err)) != 0 and b"null argument" in err.value
        assert call(None) != 0


def test_the_key_and_the_file_are_wired():
    core = read("zkm_amd", "csrc", "core.hip")
    assert 'k == "image_hash_form"' in core and '"image_hash_form"' in read("include", "zkm_hip.h")
    assert "image_hash.hip" in read("zkm_amd", "csrc", "Makefile")
