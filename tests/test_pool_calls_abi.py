"""CPU suite: the pool takes segments as the emulator records them (zkm_pool_prove_segments_calls, include/zkm_hip.h "one process, many
GPUs").  The prototype in the header, the linker's list, the binding and the Rust block; the refusals the entry point makes before it
looks at a device; the tuning key that chooses how a worker serves its groups; the Rust wrapper's names."""
import ctypes as C
import re
import subprocess

from . import calls_entry_fixtures as F
from .test_abi import declared_alike, header_text, prototypes, read
from .test_rust_names import strip_comments

NAME = "zkm_pool_prove_segments_calls"


def test_the_header_declares_the_prototype_the_issue_gives(zkm):
    ret, params = prototypes()[NAME]
    assert ret == "int" and params == [
        ("zkm_pool*", "pool"), ("const zkm_stark_config*", "cfg"), ("size_t", "nseg"), ("size_t", "max_stack"), ("const zkm_boot_image*", "images"),
        ("const void*", "calls"), ("const uint64_t* const*", "public_values"), ("const size_t*", "npublic"),
        ("uint64_t* const*", "proofs_out"), ("size_t*", "proof_offsets_out"), ("uint64_t* const*", "ctl_challenges_out"), ("char**", "err")], params
    assert re.search(r"\bint %s\(zkm_pool\* pool,[^;]*const struct zkm_segment_calls\* calls,[^;]*char\*\* err\);" % NAME, header_text())


def test_the_entry_point_is_exported_bound_and_declared_in_the_rust_block(zkm):
    declared_alike(zkm, NAME)
    dynamic = subprocess.check_output(["nm", "-D", "--defined-only", zkm._LIB_PATH], text=True)
    assert re.search(r" T %s$" % NAME, dynamic, flags=re.M)
    # what the workers call across the library's files stays out of the exported names
    assert not re.search(r" T zkm_\w*(calls_stage|calls_get|ops_steps|ops_calls)_entry$", dynamic, flags=re.M)
    assert callable(zkm.Pool.prove_segments_calls) and callable(zkm.Pool.memory) and callable(zkm.Pool.resident_bytes)


def call(zkm, pool=None, cfg=True, nseg=1, max_stack=0, calls=True, proofs=False, offsets=True, challenges=False):
    """The entry point with a NULL pool (or `pool`) and the other arguments present or NULL: (status, message)."""
    L = zkm.load()
    c = zkm.StarkConfig()
    L.zkm_standard_config(C.byref(c))
    arr = zkm.Context._calls_array([zkm.SegmentCalls(**F.segment(zkm, "two")["kw"])])
    out = (C.c_void_p * 1)()
    offs = (C.c_size_t * 13)()
    err = C.c_char_p()
    rc = L.zkm_pool_prove_segments_calls(pool, C.byref(c) if cfg else None, nseg, max_stack, None, C.addressof(arr) if calls else None, None, None,
                                         out if proofs else None, offs if offsets else None, out if challenges else None, C.byref(err))
    return rc, (err.value or b"").decode()


def test_the_host_refusals_come_before_any_device_and_begin_with_the_functions_name(zkm):
    """Each refusal of the header's list that needs no device, with a NULL pool: nonzero, and the message begins with the name."""
    for kw in (dict(), dict(cfg=False), dict(calls=False), dict(nseg=0), dict(max_stack=33), dict(proofs=True), dict(offsets=False),
               dict(proofs=True, offsets=False, challenges=False)):
        rc, msg = call(zkm, **kw)
        assert rc != 0 and msg.startswith(NAME + ": "), (kw, msg)
    assert call(zkm)[1] == NAME + ": null argument"


class FakePool(C.Structure):
    """Never dereferenced: the refusals below are made before the pool is looked into."""
    _fields_ = [("words", C.c_uint64 * 16)]


def test_the_refusals_come_in_the_headers_order(zkm):
    """NULL pool / cfg / calls and the output rules, then no segments, then max_stack beyond 32 -- the later ones with a pool that is
    not NULL (a block of zero words: an empty pool, which no refusal reads)."""
    pool = C.cast(C.pointer(FakePool()), C.c_void_p)
    assert call(zkm, pool, cfg=False, nseg=0, max_stack=33)[1] == NAME + ": null argument"
    assert call(zkm, pool, calls=False, nseg=0, max_stack=33)[1] == NAME + ": null argument"
    assert call(zkm, pool, proofs=True, nseg=0, max_stack=33)[1] == NAME + ": null argument"          # proofs without challenges
    assert call(zkm, pool, offsets=False, nseg=0, max_stack=33)[1] == NAME + ": null argument"        # neither proofs nor offsets
    assert call(zkm, pool, nseg=0, max_stack=33)[1] == NAME + ": no segments"
    assert call(zkm, pool, nseg=1, max_stack=33)[1] == NAME + ": max_stack beyond 32"
    assert call(zkm, pool, nseg=1, max_stack=33, proofs=True, challenges=True)[1] == NAME + ": max_stack beyond 32"


def test_the_tuning_key_is_accepted_and_documented():
    header = read("include", "zkm_hip.h")
    assert re.search(r'^ \*   "pool_stage_ahead"\s', header, flags=re.M)
    assert 'k == "pool_stage_ahead"' in read("zkm_amd", "csrc", "core.hip")
    assert "int pool_stage_ahead = 1;" in read("zkm_amd", "csrc", "zkm_internal.h")          # staged ahead unless told otherwise
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = read(doc)
        assert NAME in text and "pool_stage_ahead" in text, doc


def test_the_pool_stays_host_only_and_the_workers_hold_two_handles_at_most():
    src = strip_comments(read("zkm_amd", "csrc", "pool.hip"))
    assert "__global__" not in src and "hipLaunchKernelGGL" not in src and "<<<" not in src
    # the staged loop composes the merged entry points' bodies; a handle is owned, so every path out of a worker frees it
    for fn in ("zkm_segments_calls_stage_entry(", "zkm_staged_calls_get_entry(", "zkm_prove_segments_ops_steps_entry(", "zkm_prove_segments_ops_calls_entry(",
               "zkm_staged_calls_free"):
        assert fn in src, fn
    assert src.count("staged_group cur, ahead;") == 1


def test_the_rust_wrapper_names_only_declared_items():
    src, sys_rs = strip_comments(read("integration", "rust", "calls_hip.rs")), strip_comments(read("integration", "rust", "zkm_hip_sys.rs"))
    assert "pub fn prove_segments_calls_pool_hip(" in src and re.search(r"\b%s\(pool, config, " % NAME, src)
    assert re.search(r"pub fn %s\(" % NAME, sys_rs)
    declared = set(re.findall(r"pub fn (zkm_\w+)\s*\(", sys_rs)) | set(re.findall(r"pub (?:struct|enum|type) (zkm_\w+)", sys_rs)) | \
        set(re.findall(r"pub const (ZKM_\w+):", sys_rs))
    used = set(re.findall(r"\b(zkm_[a-z0-9_]+|ZKM_[A-Z0-9_]+)\b", src))
    assert NAME in used and used <= declared, used - declared
