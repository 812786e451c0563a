"""CPU suite: how csrc/ holds device resources.  The proving drivers (ctl.hip, stark.hip) take device blocks, pooled events and batches
from the scoped owners of csrc/zkm_internal.h instead of acquiring and returning them by hand; batches are made by zkm_batch_new only;
and one helper raises a kernel's dynamic-LDS limit."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkm_amd", "csrc")


def code(path):
    """The file's text without // and /* */ comments."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc")))


def test_drivers_hold_blocks_events_and_batches_through_owners():
    banned = ["->alloc(", "->release(", "get_event(", "event_pool", "zkm_batch_free(", "new zkm_batch"]
    found = []
    for name in ("ctl.hip", "stark.hip"):
        text = code(os.path.join(CSRC, name))
        found += ["%s: %s" % (name, b) for b in banned if b in text]
    assert not found, found


def test_batches_are_made_by_zkm_batch_new_only():
    makers = []
    for path in sources():
        name = os.path.basename(path)
        if name == "zkm_internal.h":
            continue
        text = code(path)
        if name == "core.hip":
            body = re.search(r"\nzkm_batch_ptr zkm_batch_new\([^)]*\)\s*\{.*?\n\}\n", text, flags=re.S)
            assert body, "core.hip defines zkm_batch_new"
            text = text.replace(body.group(0), "\n")
        if re.search(r"\bnew\s+zkm_batch\b", text):
            makers.append(name)
    assert not makers, makers


def test_one_helper_raises_the_dynamic_lds_limit():
    callers = [os.path.basename(p) for p in sources() if os.path.basename(p) != "zkm_internal.h" and re.search(r"\bhipFuncSetAttribute\s*\(", code(p))]
    assert not callers, callers
    assert re.search(r"\bhipFuncSetAttribute\s*\([^;]*MaxDynamicSharedMemorySize", code(os.path.join(CSRC, "zkm_internal.h")))
