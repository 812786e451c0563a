"""CPU suite: the host half of the staged steps (include/zkm_hip.h "Staged steps").  The five entry points are exported, bound and
declared in the Rust block with the header's parameter names; the refusals zkm_cpu_steps_scan and zkm_cpu_steps_stage make on the host
come before anything that needs a device -- without a context what is left is the missing context; the handle's functions take NULL;
the header documents every new function and the wrappers name only what the library declares."""
import ctypes as C
import os
import re

from . import cpu_steps_model as M
from .test_abi import declared_alike

NEW = ("zkm_cpu_steps_scan", "zkm_cpu_steps_stage", "zkm_staged_steps_ready", "zkm_staged_steps_get", "zkm_staged_steps_free")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_exported_bound_and_declared_in_the_rust_block(zkm):
    for fn in NEW:
        declared_alike(zkm, fn)
    for method in ("cpu_steps_scan", "cpu_steps_stage"):
        assert callable(getattr(zkm.Context, method))
    for method in ("get", "ready", "free", "__enter__", "__exit__", "__del__", "__len__"):
        assert callable(getattr(zkm.StagedSteps, method))


def calls(zkm, nseg, sl, with_outputs=True):
    """Both entry points without a context; returns their messages."""
    L = zkm.load()
    counts, out, msgs = (C.c_size_t * (3 * max(nseg, 1)))(), C.c_void_p(), []
    for call in (lambda e: L.zkm_cpu_steps_scan(None, nseg, sl, counts if with_outputs else None, None, e),
                 lambda e: L.zkm_cpu_steps_stage(None, nseg, sl, C.byref(out) if with_outputs else None, e)):
        err = C.c_char_p()
        assert call(C.byref(err)) == 1 and not out.value
        msgs.append(err.value.decode())
    return msgs


def test_the_hosts_refusals_come_before_the_missing_context(zkm):
    m = M.sample()
    good = zkm.CpuSteps(m.step_array(), m.raw_array())
    names = ("zkm_cpu_steps_scan", "zkm_cpu_steps_stage")
    arr = lambda *structs: (zkm.CpuStepsStruct * len(structs))(*structs)
    for name, msg in zip(names, calls(zkm, 1, None)):
        assert msg == name + ": null argument"
    for name, msg in zip(names, calls(zkm, 0, arr(good.struct()))):
        assert msg == name + ": no segments"
    for bad in (zkm.CpuStepsStruct(None, 3, None, 0), zkm.CpuStepsStruct(None, 0, None, 2)):
        for name, msg in zip(names, calls(zkm, 2, arr(good.struct(), bad))):
            assert msg == name + ": segment 1: null pointer with a nonzero count"
    big = good.struct()
    big.nsteps = (1 << 28) + 1        # (refused by its count: the records are not read)
    for name, msg in zip(names, calls(zkm, 3, arr(good.struct(), good.struct(), big))):
        assert msg == name + ": segment 2: 268435457 steps, more than 2^28"
    at_limit = good.struct()
    at_limit.nsteps = 1 << 28
    # nothing to refuse on the host (2^28 steps are allowed; an empty segment is; a step the walk would refuse is the device's to find):
    # what is left is the missing output, then the missing context
    bad_step = m.step_array()[:4].copy()
    bad_step["kind"][2] = 77
    for sl in (arr(at_limit), arr(zkm.CpuStepsStruct(None, 0, None, 0)), arr(zkm.CpuSteps(bad_step, m.raw_array()).struct())):
        for with_outputs in (False, True):
            for name, msg in zip(names, calls(zkm, 1, sl, with_outputs)):
                assert msg == name + ": null argument"


def test_the_handles_functions_take_null(zkm):
    L = zkm.load()
    L.zkm_staged_steps_free(None)
    assert L.zkm_staged_steps_ready(None, 0) == 1 and L.zkm_staged_steps_ready(None, 1) == 1
    err, st = C.c_char_p(), zkm.CpuStepsStruct()
    assert L.zkm_staged_steps_get(None, 0, C.byref(st), None, None, None, C.byref(err)) == 1
    assert err.value == b"zkm_staged_steps_get: null argument"


def test_the_refusal_texts_stand_once_and_the_host_walk_is_as_it_was(zkm):
    """zkm_cpu_steps_counts and the unstaged calls are as they were: the same counts, the same messages (tests/test_cpu_steps.py holds
    them); the message texts now stand once, for the host walk and the device's verdicts."""
    m = M.sample()
    assert zkm.cpu_steps_counts(m.cpu_steps(zkm)) == (598, 4, 9)
    src = open(os.path.join(ROOT, "zkm_amd", "csrc", "cpu_steps.hip")).read()
    assert src.count("uses the channels") == 1 and src.count("does not take the encoding") == 1
    walk = open(os.path.join(ROOT, "zkm_amd", "csrc", "cpu_steps_walk.hip")).read()
    assert "zkm_cpu_step_refusal(" in walk and "uses the channels" not in walk


def test_the_header_documents_every_new_function_and_what_is_still_not_staged(zkm):
    text = open(os.path.join(ROOT, "include", "zkm_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    for fn in NEW:
        assert re.search(r"\b%s\b" % fn, comments), fn
    assert "Steps are not staged" not in text and "mismatch is NOT detected" not in text
    assert "The pool still takes no steps; images and calls (zkm_segments_calls_expand) are still not staged" in comments
    # the new handle adds no typedef: an address to the bindings
    assert "zkm_staged_steps" not in zkm.abi.opaque() and not re.search(r"typedef\s+struct\s+zkm_staged_steps", text)


def test_the_rust_wrappers_name_only_declared_items():
    src = open(os.path.join(ROOT, "integration", "rust", "cpu_steps_hip.rs")).read()
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "zkm_hip_sys.rs")).read()
    assert "pub struct StagedSteps" in src and "impl Drop for StagedSteps" in src
    for fn in ("zkm_cpu_steps_stage", "zkm_staged_steps_ready", "zkm_staged_steps_get", "zkm_staged_steps_free"):
        assert re.search(r"\b%s\(" % fn, src) and re.search(r"pub fn %s\(" % fn, sys_rs), fn
    assert "pub fn prove_segments_ops_steps_staged(" in src and "pub fn segments_tables_steps_staged(" in src
