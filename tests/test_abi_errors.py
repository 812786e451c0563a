"""CPU suite: the C ABI's error boundary.  Every export that takes a handle (zkm_ctx*, zkm_batch*, zkm_staged*, zkm_pool*) answers a
null handle with its failure value -- and a message where it has an `err` -- instead of crashing the caller's process; and the message
writer in csrc/zkm_internal.h is the only code that writes *err."""
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = re.compile(r"^(const\s+)?zkm_(ctx|batch|staged|pool)\s*\*\s*(const\s+)?\w+$")

# Failure values of a null handle that are not the default of the return type (status 1, size 0, NULL, nothing for void)
SPECIAL = {"zkm_staged_ready": 1, "zkm_pool_device": -1}


def handle_functions():
    """name -> (parameter names, index of the handle parameters) for every header function with a handle parameter."""
    text = open(os.path.join(ROOT, "include", "zkm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for name, params in re.findall(r"\b(zkm_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", text):
        ps = [" ".join(p.split()) for p in params.split(",")] if params.strip() not in ("", "void") else []
        names = [re.sub(r"\[.*\]$", "", p).split()[-1].lstrip("*") for p in ps]
        handles = [i for i, p in enumerate(ps) if HANDLE.match(re.sub(r"\s*\*\s*", "* ", p).replace("* *", "**"))]
        if handles:
            out[name] = (names, handles)
    return out


CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
import zkm_amd
lib = zkm_amd.load()
libc = C.CDLL(None)
libc.free.argtypes = [C.c_void_p]
funcs = json.loads(sys.argv[2])
results = {}
for name, (pnames, _) in sorted(funcs.items()):
    fn = getattr(lib, name)
    msg = C.c_char_p()
    args = [C.byref(msg) if p == "err" else (None if isinstance(t, type) and issubclass(t, (C._Pointer, C.c_void_p, C.c_char_p)) else 0)
            for p, t in zip(pnames, fn.argtypes)]
    print(name, flush=True)
    r = fn(*args)
    addr = C.cast(msg, C.c_void_p).value
    text = C.string_at(addr).decode() if addr else None
    if addr:
        libc.free(addr)
    results[name] = {"ret": r, "msg": text, "has_err": "err" in pnames}
print("RESULTS " + json.dumps(results), flush=True)
"""


def test_null_handles_fail_with_status_not_crash(zkm):
    lib = zkm.load()
    funcs = handle_functions()
    assert {"zkm_ctx_synchronize", "zkm_batch_cap", "zkm_staged_ready", "zkm_pool_set_tuning", "zkm_memory_trace"} <= set(funcs)
    for name, (pnames, _) in funcs.items():
        assert len(getattr(lib, name).argtypes) == len(pnames), name
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(funcs)], capture_output=True, text=True, timeout=300)
    called = [l for l in r.stdout.splitlines() if not l.startswith("RESULTS ")]
    assert r.returncode == 0, "child died (%d) in %s\n%s" % (r.returncode, called[-1] if called else "?", r.stderr[-2000:])
    results = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULTS ")][0][len("RESULTS "):])
    assert set(results) == set(funcs)
    for name, got in results.items():
        restype = getattr(lib, name).restype
        if name in SPECIAL:
            want = SPECIAL[name]
        elif restype is None:
            want = None
        elif restype is zkm.C.c_int:
            want = 1
        elif restype is zkm.C.c_size_t:
            want = 0
        else:
            want = None   # pointer: NULL
        assert got["ret"] == want, (name, got, want)
        if got["has_err"]:
            assert got["msg"], "%s failed without a message" % name


def test_only_the_boundary_writes_err():
    csrc = os.path.join(ROOT, "zkm_amd", "csrc")
    writers = []
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.inc"))):
        if os.path.basename(path) == "zkm_internal.h":
            continue
        for i, line in enumerate(open(path).read().splitlines(), 1):
            if re.search(r"\*\s*err\s*=(?!=)|strdup\(", line):
                writers.append("%s:%d" % (os.path.basename(path), i))
    assert not writers, writers
