"""CPU suite: the C ABI of the stacked commitments and the lock-step FRI pair (zkm_batch_commit_values_stack / _coeffs_stack,
zkm_batch_stack_*, zkm_eval_openings_stack, zkm_fri_prove_stack).  The declarations agree in header, binding and Rust block, and every
refusal that precedes the context carries its message without a GPU."""
import ctypes as C

import numpy as np
import pytest

from .test_abi import declared_alike

NEW = ("zkm_batch_commit_values_stack", "zkm_batch_commit_coeffs_stack", "zkm_batch_stack_size", "zkm_batch_stack_cap", "zkm_batch_stack_coeffs",
       "zkm_batch_stack_merkle_path", "zkm_eval_openings_stack", "zkm_fri_prove_stack")
CONSTRUCTORS = ("zkm_batch_commit_values_stack", "zkm_batch_commit_coeffs_stack")


@pytest.mark.parametrize("fn", NEW)
def test_declared_alike(zkm, fn):
    declared_alike(zkm, fn)


def commit(zkm, fn, members, ncols, log_n, rate_bits=2, cap_height=4, out=True):
    """the constructor with a NULL context: (status, message).  Whatever it refuses before the context is refused here too."""
    ptrs = (C.c_void_p * max(len(members), 1))(*members) if members is not None else None
    h, err = C.c_void_p(), C.c_char_p()
    rc = getattr(zkm.load(), fn)(None, ptrs, len(members or ()), ncols, log_n, rate_bits, cap_height, C.byref(h) if out else None, C.byref(err))
    assert h.value is None
    return rc, (err.value or b"").decode()


@pytest.mark.parametrize("fn", CONSTRUCTORS)
def test_constructors_refuse_on_the_host(zkm, fn):
    words = np.zeros(3 << 5, dtype=np.uint64)
    good = [words.ctypes.data] * 2
    for members, ncols, log_n, rate, cap, out, want in (
            (None, 3, 5, 2, 4, True, "null argument"),
            (good, 3, 5, 2, 4, False, "null argument"),
            ([], 3, 5, 2, 4, True, "1..32 members"),
            ([words.ctypes.data] * 33, 3, 5, 2, 4, True, "1..32 members"),
            (good, 0, 5, 2, 4, True, "empty polynomial batch"),
            (good, 32768, 5, 2, 4, True, "members x columns <= 65535"),
            ([words.ctypes.data] * 32, 2048, 5, 2, 4, True, "members x columns <= 65535"),
            (good, 3, 29, 2, 4, True, "polynomial batch too large"),
            (good, 3, 5, 2, 8, True, "cap_height exceeds LDE size"),
            ([words.ctypes.data, None, words.ctypes.data], 3, 5, 2, 4, True, "member 1: null pointer")):
        rc, msg = commit(zkm, fn, members, ncols, log_n, rate, cap, out)
        assert rc == 1 and msg.startswith(fn + ": ") and want in msg, (want, msg)
    # what passes every host check reaches the context, and a NULL context is what is left to refuse
    rc, msg = commit(zkm, fn, good, 3, 5)
    assert rc == 1 and msg == fn + ": null argument"
    rc, msg = commit(zkm, fn, [words.ctypes.data] * 32, 2047, 5)
    assert rc == 1 and msg == fn + ": null argument"


def test_accessors_and_entry_points_refuse_null(zkm):
    lib = zkm.load()
    out = np.zeros(64, dtype=np.uint64)
    assert lib.zkm_batch_stack_size(None) == 0
    assert lib.zkm_batch_stack_cap(None, 0, out.ctypes.data) == 1
    assert lib.zkm_batch_stack_coeffs(None, 0, out.ctypes.data) == 1
    assert lib.zkm_batch_stack_merkle_path(None, 0, 0, out.ctypes.data, out.ctypes.data) == 1
    err = C.c_char_p()
    assert lib.zkm_eval_openings_stack(None, None, None, None, C.byref(err)) == 1 and err.value == b"zkm_eval_openings_stack: null argument"
    cfg = zkm.StarkConfig()
    lib.zkm_standard_config(C.byref(cfg))
    assert lib.zkm_fri_prove_stack(None, C.byref(cfg), None, 0, None, 0, None, None, None, C.byref(err)) == 1
    assert err.value == b"zkm_fri_prove_stack: null argument"
