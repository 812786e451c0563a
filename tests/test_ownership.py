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


def others():
    """(name, code) of every source but zkm_internal.h, where the owners are defined."""
    return [(os.path.basename(p), code(p)) for p in sources() if os.path.basename(p) != "zkm_internal.h"]


def test_staged_input_follows_the_one_copy_fence():
    """Input put into HBM behind the current work (the staged traces, operations, steps and calls) follows zkm_copy_fence: nobody else asks an
    event whether it has ended, keeps a guard of its own for copies in flight, or puts BOTH copy streams behind an event."""
    fence = re.search(r"\nstruct zkm_copy_fence \{.*?\n\};\n", code(os.path.join(CSRC, "zkm_internal.h")), flags=re.S)
    assert fence, "zkm_internal.h defines zkm_copy_fence"
    assert "hipEventQuery(" in fence.group(0) and "zkm_event done[2]" in fence.group(0)
    found = []
    for name, text in others():
        if "hipEventQuery(" in text:
            found.append("%s: hipEventQuery(" % name)
        if re.search(r"\bcopy_join\b", text):
            found.append("%s: copy_join" % name)
        # The copy streams ordered behind the compute stream.  Only staging uses the SECOND copy stream, so that one is pinned: nobody but
        # the fence creates it, and no statement makes it wait for an event or waits for it on the host -- under its own name or under
        # a local name it was given (`up2 = c->copy_stream2`, also as a branch of ?:).  Statements may still QUEUE work on it.  What this
        # cannot see: a stream passed on as a function argument and waited for inside the callee.
        if name == "core.hip":
            continue
        names = {"copy_stream2"} | set(re.findall(r"\b(\w+)\s*=[^;=]*\bcopy_stream2\b", text))
        for stmt in re.findall(r"[^;{}]+", text):
            if re.search(r"ensure_copy_stream\s*\(\s*1", stmt):
                found.append("%s: %s" % (name, " ".join(stmt.split())))
            for call in re.findall(r"hip(?:StreamWaitEvent|StreamSynchronize)\s*\(\s*([^,)]*)", stmt):
                if set(re.findall(r"\w+", call)) & names:
                    found.append("%s: %s" % (name, " ".join(stmt.split())))
    assert not found, found
    # core.hip owns the streams themselves (creation, trim, destruction): there the second copy stream waits for no event
    core = code(os.path.join(CSRC, "core.hip"))
    assert not re.search(r"hipStreamWaitEvent\s*\([^;]*copy_stream2", core)
    assert not re.search(r"ensure_copy_stream\s*\(\s*1\s*\)", core)


def test_staged_traces_are_held_by_owners():
    core = code(os.path.join(CSRC, "core.hip"))
    news = re.findall(r"[^;{}]*\bnew\s+zkm_staged\b[^;{}]*", core)
    assert news and all("std::unique_ptr<zkm_staged>" in s for s in news), news
    assert not re.search(r"\bdelete\s+s\b", core)
    body = re.search(r"\nstruct zkm_staged \{.*?\n\};\n", core, flags=re.S).group(0)
    assert "zkm_scratch block;" in body and "zkm_copy_fence fence;" in body and "hipEvent_t" not in body
    assert body.index("zkm_scratch block;") < body.index("zkm_copy_fence fence;"), "the fence goes, and has waited, before the block it guards"
    for b in ("->release(", "event_pool", "get_event("):
        staged = core[core.index("struct zkm_staged {"):core.index("zkm_staged* zkm_staged_from_segment")]
        assert b not in staged, b


def test_one_helper_raises_the_dynamic_lds_limit():
    callers = [os.path.basename(p) for p in sources() if os.path.basename(p) != "zkm_internal.h" and re.search(r"\bhipFuncSetAttribute\s*\(", code(p))]
    assert not callers, callers
    assert re.search(r"\bhipFuncSetAttribute\s*\([^;]*MaxDynamicSharedMemorySize", code(os.path.join(CSRC, "zkm_internal.h")))
