"""GPU suite: K segments' calls staged behind the current proofs (zkm_segments_calls_stage, zkm_staged_calls_ready / _get / _free): the
expansions, the placement of the records and the walk on the device, with no host wait in the stage.  The judge is the merged one-entry
expansion -- every word the stage leaves in device memory (the patched steps, the row block, every list, the counts) equals
segments_calls_expand(...).download(s); proofs and tables of the builder on the staged outputs equal prove_segments_ops_calls /
segments_tables_calls on the same SegmentCalls; a refusal the device finds reads as zkm_segments_calls_expand's for the same input."""
import ctypes as C
import gc
import re

import numpy as np
import pytest

from . import boot_fixtures as BF
from . import calls_entry_fixtures as F
from . import cpu_steps_model as M
from .test_gpu_calls_entry import DEVICE_LISTS, THREE, assert_expansions_equal
from .test_gpu_segment_ops import assert_tables_equal, tables_of

pytestmark = pytest.mark.gpu

GET = "zkm_staged_calls_get: segment %d: "
_WANT = {}


def wanted(ctx, zkm, name, own=False):
    """(kw, the one-entry expansion's outputs) for a segment of the suite: computed once, shared, not to be changed."""
    if (name, own) not in _WANT:
        kw = dict(F.segment(zkm, name)["kw"], **(F.own_operations() if own else {}))
        with ctx.segments_calls_expand([zkm.SegmentCalls(**kw)]) as x:
            _WANT[name, own] = (kw, x.download(0))
    return _WANT[name, own]


def outputs(h, segments=None):
    """(steps, ops, images or None) of the handle's segments, as the builder's entry points take them."""
    got = [h.get(s) for s in (range(len(h)) if segments is None else segments)]
    images = [im for _, _, im in got]
    return [st for st, _, _ in got], [o for _, o, _ in got], (None if images[0] is None else images)


def assert_same_proofs(got, want):
    assert len(got) == len(want)
    for s, ((p, c, o), (wp, wc, wo)) in enumerate(zip(got, want)):
        assert o == wo and (c == wc).all(), s
        bad = np.nonzero(p != wp)[0]
        assert bad.size == 0, "segment %d: first differing proof word %d" % (s, bad[0])


def assert_same_tables(ctx, got, want):
    for (st, lg), (wst, wlg) in zip(got, want):
        assert lg == wlg
        assert_tables_equal(tables_of(st, lg, ctx), tables_of(wst, wlg, ctx))
        st.free()
        wst.free()


# ---------------------------------------------------------------- 1. one segment, word for word
def case_1(ctx, zkm):
    kw, want = wanted(ctx, zkm, "all", own=True)
    with ctx.segments_calls_stage([zkm.SegmentCalls(**kw)]) as h:
        got = h.download(0)
        steps, _, image = h.get(0)
        assert image is None and len(h) == 1
        assert want["counts"]["nkeccak"] == 2 + 2 and want["counts"]["narithmetic"] == 2 + 11 and want["counts"]["nsha_extend"] == 48
        assert_expansions_equal(got, want, "K = 1")
        # the walk ran over the patched list with every ready-made row in device memory: the device's scan of that list gives the host
        # walk's counts and base triples, and the builder takes the staged segment with them (cases 4 and 5 compare its tables)
        patched = zkm.CpuSteps(got["steps"], got["raw_rows"])
        (counts,), (bases,) = ctx.cpu_steps_scan([patched], bases=True)
        assert counts == zkm.cpu_steps_counts(patched)
        (dev_counts,), (dev_bases,) = ctx.cpu_steps_scan([DeviceRows(zkm, got["steps"], steps.struct())], bases=True)
        assert dev_counts == counts and (dev_bases == bases).all()


class DeviceRows:
    """A host step list over the ready-made rows a staged segment holds in device memory."""

    def __init__(self, zkm, steps, st):
        self.steps, self.st = np.ascontiguousarray(steps), zkm.CpuStepsStruct(None, st.nsteps, st.raw_rows, st.nraw)
        self.st.steps = self.steps.ctypes.data

    def struct(self):
        return self.st


def test_one_segment_with_all_four_kinds_and_own_operations_equals_the_expansion(ctx, zkm):
    case_1(ctx, zkm)


# ---------------------------------------------------------------- 2. three segments, the waits, the memory
def test_three_segments_in_one_stage_no_host_wait_and_memory_back_after_free(ctx, zkm):
    pairs = [wanted(ctx, zkm, name) for name in THREE]
    calls = [zkm.SegmentCalls(**kw) for kw, _ in pairs]
    live, w0 = ctx.memory()[0], ctx.host_waits()
    h = ctx.segments_calls_stage(calls)
    w1 = ctx.host_waits()
    h.get(0)
    w2 = ctx.host_waits()
    h.get(1), h.get(2), h.get(0)
    w3 = ctx.host_waits()
    assert w1 - w0 == 0 and w2 - w1 <= 1 and w3 - w2 == 0
    assert h.ready() is True and ctx.memory()[0] > live and len(h) == 3
    for s, (_, want) in enumerate(pairs):
        assert_expansions_equal(h.download(s), want, "segment %d" % s)
    h.free()
    assert ctx.memory()[0] == live
    # kinds with no item in any segment (here: everything but I/O) must not break the layout
    with ctx.segments_calls_stage(calls[:2]) as h:
        for s in range(2):
            assert_expansions_equal(h.download(s), pairs[s][1], "segment %d of two" % s)
    # dropped without free(): the blocks come back
    h = ctx.segments_calls_stage(calls)
    del h
    gc.collect()
    assert ctx.memory()[0] == live


# ---------------------------------------------------------------- 3. mixed list locations
def test_a_segment_with_its_lists_in_device_memory_between_two_with_host_lists(ctx, zkm):
    from zkm_amd import _as_words
    names = (THREE[0], "all", THREE[2])
    pairs = [wanted(ctx, zkm, name) for name in names]
    calls = [zkm.SegmentCalls(**kw) for kw, _ in pairs]
    assert all(name in calls[1].lists and calls[1].lists[name].size for name in DEVICE_LISTS)
    bufs = []
    try:
        for name in DEVICE_LISTS:
            a = calls[1].lists[name]
            bufs.append(ctx.alloc((a.nbytes + 7) // 8).upload(_as_words(a)))
            calls[1].lists[name] = bufs[-1]
        with ctx.segments_calls_stage(calls) as h:
            for s, (_, want) in enumerate(pairs):
                assert_expansions_equal(h.download(s), want, "segment %d (%s)" % (s, names[s]))
            # a payload list the caller has in device memory is referenced where it lies
            _, ops = h.structs(1)
            assert ops.sha_compress_hx == bufs[DEVICE_LISTS.index("compress_hx")].ptr
    finally:
        for b in bufs:
            b.free()


# ---------------------------------------------------------------- 4. proofs and tables
@pytest.fixture(scope="module")
def proven(ctx, zkm):
    """The unstaged entries on the three segments: computed once, shared, not to be changed."""
    kws = [wanted(ctx, zkm, name)[0] for name in THREE]
    pubs = [[1, 2, 3 + s] for s in range(3)]
    calls = [zkm.SegmentCalls(**kw) for kw in kws]
    return kws, pubs, ctx.prove_segments_ops_calls(calls, public_values=pubs)


def test_proofs_and_tables_of_the_staged_outputs_equal_the_calls_entries(ctx, zkm, proven):
    kws, pubs, want = proven
    calls = [zkm.SegmentCalls(**kw) for kw in kws]
    live = ctx.memory()[0]
    want_tables = ctx.segments_tables_calls(calls)       # (the first builder call may grow the download area)
    with ctx.segments_calls_stage(calls) as h:
        steps, ops, images = outputs(h)
        assert images is None
        w0 = ctx.host_waits()
        got_tables = ctx.segments_tables_steps(steps, ops)
        assert ctx.host_waits() - w0 == 3
        assert ctx.segments_tables_steps(steps, ops, sizing=True) == [lg for _, lg in want_tables]
        assert_same_tables(ctx, got_tables, want_tables)
        got = ctx.prove_segments_ops_steps(steps, ops, public_values=pubs)
        assert_same_proofs(got, want)
        reports = ctx.verify_segments([p for p, _, _ in got], pubs, [ch for _, ch, _ in got])
        assert [r.code for r in reports] == [0] * 3, [r.message for r in reports]
    assert ctx.memory()[0] == live


# ---------------------------------------------------------------- 5. behind two boot images; 6. 257 rows
class BootRecorder(M.StepRecorder, BF.BootMachine):
    pass


def test_behind_two_boot_images_that_are_staged_too(ctx, zkm, oracle):
    kws, images = [], []
    for name, spec in (("b", dict(hint_len=300, keccak=False, compress=False, seed=21)), ("a", dict(io=("hint_read",), compress=False, seed=22))):
        seg = BF.segment(oracle, name)
        s = F.record(zkm, BootRecorder(seg["model"], raw_boot=False), **spec)
        assert s["kw"]["first_clock"] == len(seg["model"].cpu_rows) > 0
        kws.append(s["kw"])
        images.append(BF.boot_image(zkm, seg["image"]))
    assert [kw["first_clock"] for kw in kws] == [4, 135]
    calls = [zkm.SegmentCalls(**kw) for kw in kws]
    pubs = [[1, 2, 3], [4, 5, 6]]
    want = ctx.prove_segments_ops_calls(calls, images=images, public_values=pubs)
    live = ctx.memory()[0]
    want_tables = ctx.segments_tables_calls(calls, images=images)
    with ctx.segments_calls_stage(calls, images=images) as h:
        steps, ops, staged_images = outputs(h)
        for im, src in zip(staged_images, images):
            st = im.struct()
            assert (st.nwords, st.npages, st.entry) == (src.nwords, src.npages, src.entry) and bytes(st.pre_hash_root) == src.root
            assert st.addrs not in (None, src.addrs.ctypes.data) and st.values not in (None, src.values.ctypes.data)
            words = np.zeros(src.nwords, dtype=np.uint32)
            err = C.c_char_p()
            assert ctx.L.zkm_dev_download(ctx.h, words.ctypes.data, st.values, words.nbytes, C.byref(err)) == 0 and (words == src.values).all()
        assert_same_tables(ctx, ctx.segments_tables_steps(steps, ops, images=staged_images), want_tables)
        assert_same_proofs(ctx.prove_segments_ops_steps(steps, ops, images=staged_images, public_values=pubs), want)
        # the caller's own images beside the staged steps and operations are as good
        assert_same_proofs(ctx.prove_segments_ops_steps(steps, ops, images=images, public_values=pubs), want)
    assert ctx.memory()[0] == live


def test_more_rows_than_one_workgroup_of_the_placement_and_no_multiple_of_64(ctx, zkm, oracle):
    """A hint read of 8,200 bytes is 2,050 words: 257 rows, one more than a workgroup of the placement kernel takes.  Recorded behind a
    boot image's rows (the fixtures' recorder keeps segments without one at 2^8 rows), so first_clock is nonzero as well."""
    seg = BF.segment(oracle, "b")
    s = F.record(zkm, BootRecorder(seg["model"], raw_boot=False), io=("hint_read",), hint_len=8200, keccak=False, compress=False, seed=23)
    calls = zkm.SegmentCalls(**s["kw"])
    assert zkm.segment_calls_steps(calls)[1]["io_rows"] == 257 and s["kw"]["first_clock"] == 4
    with ctx.segments_calls_expand([calls]) as x:
        want = x.download(0)
    with ctx.segments_calls_stage([calls]) as h:
        assert_expansions_equal(h.download(0), want, "257 rows")


# ---------------------------------------------------------------- 7. more than one group of segments
def test_thirty_three_segments_in_one_stage_still_no_host_wait(ctx, zkm):
    kw, want = wanted(ctx, zkm, "two")
    other, want_other = wanted(ctx, zkm, "io-long")
    calls = [zkm.SegmentCalls(**kw) for _ in range(33)]
    calls[31] = zkm.SegmentCalls(**other)                     # (the first group's last segment differs from its neighbours)
    live, w0 = ctx.memory()[0], ctx.host_waits()
    with ctx.segments_calls_stage(calls) as h:
        w1 = ctx.host_waits()
        for s in range(33):
            h.get(s)
        assert w1 - w0 == 0 and ctx.host_waits() - w1 == 1 and len(h) == 33
        for s in (0, 31, 32):
            assert_expansions_equal(h.download(s), want_other if s == 31 else want, "segment %d" % s)
    assert ctx.memory()[0] == live


# ---------------------------------------------------------------- 8. ordering
def pinned_copy(ctx, a, pins):
    """The array's words in page-locked memory, with its dtype and shape."""
    a = np.ascontiguousarray(a)
    words = ctx.pinned_array(max((a.nbytes + 7) // 8, 1))
    pins.append(words)
    out = words.view(np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def test_staged_from_pinned_memory_and_consumed_at_once(ctx, zkm, proven):
    kws, pubs, want = proven
    pins, calls = [], []
    try:
        for kw in kws:
            p = dict(kw)
            p["steps"] = zkm.CpuSteps(pinned_copy(ctx, kw["steps"].steps, pins), pinned_copy(ctx, kw["steps"].raw_rows, pins))
            for name in ("extend", "compress", "keccak", "io", "insns"):
                if kw[name] is not None:
                    p[name] = tuple(pinned_copy(ctx, a, pins) for a in kw[name])
            calls.append(zkm.SegmentCalls(**p))
        pinned = {a.ctypes.data for a in pins}
        assert all(q.steps.steps.ctypes.data in pinned and q.steps.raw_rows.ctypes.data in pinned for q in calls)      # (the pinned words themselves)
        assert all(a.ctypes.data in pinned for q in calls for a in q.lists.values() if a.size)
        # no ready(wait) between the stage and the call that consumes it
        with ctx.segments_calls_stage(calls) as h:
            steps, ops, _ = outputs(h)
            assert_same_proofs(ctx.prove_segments_ops_steps(steps, ops, public_values=pubs), want)
        # the sources may be reused once ready() says so: overwritten before the call, the results are unchanged
        with ctx.segments_calls_stage(calls) as h:
            assert h.ready(wait=True) is True and h.ready() is True
            for a in pins:
                a[:] = np.uint64(0xDEADBEEFDEADBEEF)
            steps, ops, _ = outputs(h)
            assert_same_proofs(ctx.prove_segments_ops_steps(steps, ops, public_values=pubs), want)
    finally:
        for a in pins:
            ctx.free_pinned(a)


# ---------------------------------------------------------------- 9. refusals found on the device
def expansions_refusal(ctx, zkm, calls):
    """What zkm_segments_calls_expand says of these segments, behind its own name: "segment <s>: ..."."""
    with pytest.raises(zkm.ZkmError) as e:
        ctx.segments_calls_expand(calls)
    text = str(e.value)
    assert text.startswith("zkm_segments_calls_expand: segment ")
    return text[len("zkm_segments_calls_expand: "):]


def device_refusals(zkm):
    """{id: (the kw of a segment the placement refuses, what the text holds)} on the fixtures' "four"."""
    kw = F.segment(zkm, "four")["kw"]
    io, q = kw["io"], kw["insns"]
    end = kw["first_clock"] + len(kw["steps"].steps)
    twice = q[1].copy()
    twice[7] = twice[6]
    late = q[1].copy()
    late[5] = end
    on_a_call = q[1].copy()
    on_a_call[0] = io[3][0, 3] // 10
    io_late = io[3].copy()
    io_late[1, 3] = 10 * end
    return {"two-on-one-clock": (dict(kw, insns=(q[0], twice)), r"instruction record row 7 \(clock %d\): two records on one clock" % twice[7]),
            "clock-below": (dict(kw, first_clock=kw["first_clock"] + 1000), r"row 0 \(clock \d+\) lies outside the step list \(first_clock 1000, "),
            "clock-at-the-end": (dict(kw, insns=(q[0], late)), r"instruction record row 5 \(clock %d\) lies outside the step list" % end),
            "two-kinds-on-one-clock": (dict(kw, insns=(q[0], on_a_call)), r"instruction record row 0 \(clock %d\): two records on one clock" % on_a_call[0]),
            "two-bad-rows-of-two-kinds": (dict(kw, io=(io[0], io[1], io[2], io_late), insns=(q[0], late)), r"I/O call row \d+ \(clock %d\) lies outside" % end)}


@pytest.mark.parametrize("case", ["two-on-one-clock", "clock-below", "clock-at-the-end", "two-kinds-on-one-clock", "two-bad-rows-of-two-kinds"])
def test_a_refusal_the_placement_finds_reads_as_the_expansions(ctx, zkm, proven, case):
    kws, pubs, want = proven
    bad, pattern = device_refusals(zkm)[case]
    calls = [zkm.SegmentCalls(**kw) for kw in (kws[0], bad, kws[2])]
    text = expansions_refusal(ctx, zkm, calls)
    assert re.match(r"segment 1: .*" + pattern, text), text
    live = ctx.memory()[0]
    with ctx.segments_calls_stage(calls) as h:
        with pytest.raises(zkm.ZkmError) as e:
            h.get(1)
        assert str(e.value) == "zkm_staged_calls_get: " + text
        with pytest.raises(zkm.ZkmError, match="zkm_staged_calls_get: no segment 3: the handle holds 3"):
            h.get(3)
        if case == "two-on-one-clock":      # the other segments of the handle stay usable
            steps, ops, _ = outputs(h, (0, 2))
            assert_same_proofs(ctx.prove_segments_ops_steps(steps, ops, public_values=[pubs[0], pubs[2]]), [want[0], want[2]])
    assert ctx.memory()[0] == live


def test_a_bad_step_of_the_segments_own_reads_as_the_host_walks_and_the_context_passes_case_1(ctx, zkm):
    kws = [wanted(ctx, zkm, name)[0] for name in THREE]
    steps = kws[0]["steps"]
    bad_steps = steps.steps.copy()
    at = len(bad_steps) - 1                    # (padding: no call's record lands there)
    assert bad_steps["kind"][at] == M.KIND["PAD"]
    bad_steps["kind"][at] = 99
    bad = dict(kws[0], steps=zkm.CpuSteps(bad_steps, steps.raw_rows))
    live = ctx.memory()[0]
    with ctx.segments_calls_stage([zkm.SegmentCalls(**kw) for kw in (kws[1], kws[2], bad)]) as h:
        with pytest.raises(zkm.ZkmError) as e:
            h.get(2)
        assert str(e.value) == GET % 2 + "step %d: unknown kind 99" % at
        for s in (0, 1):
            assert_expansions_equal(h.download(s), wanted(ctx, zkm, THREE[s + 1])[1], "segment %d" % s)
    assert ctx.memory()[0] == live
    case_1(ctx, zkm)


# ---------------------------------------------------------------- 10. refusals at the consuming calls
def test_refusals_at_the_consuming_calls(ctx, zkm):
    kws = [wanted(ctx, zkm, name)[0] for name in THREE]
    calls = [zkm.SegmentCalls(**kw) for kw in kws]
    live = ctx.memory()[0]
    other = zkm.Context(0)
    try:
        with other.segments_calls_stage(calls) as h:
            steps, ops, _ = outputs(h)
            for call in (lambda: ctx.segments_tables_steps(steps, ops), lambda: ctx.prove_segments_ops_steps(steps, ops)):
                with pytest.raises(zkm.ZkmError, match="segment 0: Cpu: the steps were staged on another context"):
                    call()
    finally:
        other.close()
    want_tables = ctx.segments_tables_calls(calls)
    with ctx.segments_calls_stage(calls) as h:
        steps, ops, _ = outputs(h)
        cut = h.get(0)[0]
        cut.struct().nsteps -= 1
        with pytest.raises(zkm.ZkmError, match="segment 0: Cpu: staged steps are taken as zkm_staged_steps_get hands them out"):
            ctx.segments_tables_steps([cut] + steps[1:], ops)
        moved = h.get(2)[0]
        moved.struct().raw_rows += 8
        with pytest.raises(zkm.ZkmError, match="segment 2: Cpu: staged steps are taken as zkm_staged_steps_get hands them out"):
            ctx.segments_tables_steps(steps[:2] + [moved], ops)
        # after every refusal the context builds the tables from the same handle
        assert_same_tables(ctx, ctx.segments_tables_steps(steps, ops), want_tables)
    assert ctx.memory()[0] == live
