"""GPU suite: K segments' calls expanded in one set of launches behind one C entry (zkm_segments_calls_expand, zkm_segments_tables_calls,
zkm_prove_segments_ops_calls).  The judge is Context.calls_expand -- the per-segment, per-kind composition in the binding, itself held
against the models by the four per-kind suites: every word the one-entry expansion writes (the patched steps, the row block, every
list) equals what calls_expand writes for that segment alone; proofs through the new entry equal prove_segments_ops_steps on
calls_expand's outputs; and the counts the issue states hold: one host wait, one launch per kind, live memory as before after free."""
import ctypes as C

import numpy as np
import pytest

from . import boot_fixtures as BF
from . import calls_entry_fixtures as F
from . import cpu_steps_model as M
from .test_gpu_segment_ops import assert_tables_equal, tables_of

pytestmark = pytest.mark.gpu

LISTS = ("raw_rows", "memory_ops", "logic_ops", "keccak_inputs", "keccak_timestamps", "sha_extend_inputs", "sha_extend_timestamps", "arithmetic_ops")
SCOPES = ("sha_calls/rows_lists", "keccak_calls/rows_lists", "io_calls/rows", "insn_rows/rows")


def yardstick(ctx, zkm, kw):
    """What Context.calls_expand writes for one segment, downloaded: the dict ExpandedCalls.download gives."""
    steps, ops = ctx.calls_expand(**kw)
    try:
        c = ops.counts
        words = lambda name: ops.lists[name].download() if name in ops.lists and isinstance(ops.lists[name], zkm.DeviceBuffer) else np.zeros(0, dtype=np.uint64)
        got = {"steps": steps.steps, "nraw": steps.nraw,
               "raw_rows": (steps.raw_rows.download()[:steps.nraw * 259] if isinstance(steps.raw_rows, zkm.DeviceBuffer) else steps.raw_rows).reshape(-1, 259),
               "memory_ops": words("memory_ops")[:c["nmemory"] * 6].reshape(-1, 6), "logic_ops": words("logic_ops").view(np.uint32)[:c["nlogic"] * 3].reshape(-1, 3),
               "keccak_inputs": words("keccak_inputs")[:c["nkeccak"] * 25].reshape(-1, 25), "keccak_timestamps": words("keccak_timestamps")[:c["nkeccak"]],
               "sha_extend_inputs": words("sha_extend_inputs").view(np.uint8)[:c["nsha_extend"] * 16].reshape(-1, 16),
               "sha_extend_timestamps": words("sha_extend_timestamps")[:c["nsha_extend"]], "counts": dict(c)}
        if kw.get("insns") is not None:
            got["arithmetic_ops"] = words("arithmetic_ops").view(np.uint32)[:c["narithmetic"] * 3].reshape(-1, 3)
        return got
    finally:
        if isinstance(steps.raw_rows, zkm.DeviceBuffer):
            steps.raw_rows.free()
        ops.free()


def assert_expansions_equal(got, want, what=""):
    assert got["nraw"] == want["nraw"], what
    assert got["steps"].tobytes() == want["steps"].tobytes(), what + ": the patched steps differ"
    assert {k: v for k, v in got["counts"].items() if v or want["counts"].get(k)} == {k: v for k, v in want["counts"].items() if v}, what
    for name in LISTS:
        assert (name in got) == (name in want), (what, name)
        if name in got:
            a, b = got[name], want[name]
            assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape)
            bad = np.argwhere(a != b)
            assert bad.size == 0, "%s %s: first differing word at %s: %d, expected %d" % (what, name, bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


_WANT = {}


def wanted(ctx, zkm, name, own=False):
    """calls_expand's outputs for a segment of the suite, computed once and left unchanged."""
    if (name, own) not in _WANT:
        kw = dict(F.segment(zkm, name)["kw"], **(F.own_operations() if own else {}))
        _WANT[name, own] = (kw, yardstick(ctx, zkm, kw))
    return _WANT[name, own]


def case_1(ctx, zkm):
    kw, want = wanted(ctx, zkm, "all", own=True)
    with ctx.segments_calls_expand([zkm.SegmentCalls(**kw)]) as x:
        got = x.download(0)
    assert want["counts"]["nkeccak"] == 2 + 2 and want["counts"]["narithmetic"] == 2 + 11 and want["counts"]["nsha_extend"] == 48
    assert_expansions_equal(got, want, "K = 1")


def test_one_segment_with_all_four_kinds_and_own_operations_equals_calls_expand(ctx, zkm):
    case_1(ctx, zkm)


THREE = ("io-long", "plain", "four")


def test_three_segments_in_one_call_one_wait_one_launch_a_kind(ctx, zkm):
    """The grid's largest extent and the zero extents fall on different segments per kind: I/O is widest in segment 0 (25 rows: four
    workgroups; a hint read of ten rows spans two) and zero in segment 1; the other kinds are zero in segments 0 and 1."""
    pairs = [wanted(ctx, zkm, name) for name in THREE]
    calls = [zkm.SegmentCalls(**kw) for kw, _ in pairs]
    assert zkm.segment_calls_steps(calls[0])[1]["io_rows"] == 25 and zkm.segment_calls_steps(calls[2])[1]["insn_rows"] == 19
    live = ctx.memory()[0]
    ctx.profile(True)
    ctx.profile_reset()
    try:
        waits = ctx.host_waits()
        x = ctx.segments_calls_expand(calls)
        assert ctx.host_waits() - waits == 1
        rec = ctx.profile_records()
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    assert [rec[s][0] for s in SCOPES] == [1, 1, 1, 1], rec
    for s, (_, want) in enumerate(pairs):
        assert_expansions_equal(x.download(s), want, "segment %d" % s)
    assert ctx.memory()[0] > live
    x.free()
    assert ctx.memory()[0] == live
    # a kind no segment uses is not launched
    ctx.profile(True)
    ctx.profile_reset()
    try:
        with ctx.segments_calls_expand(calls[:2]) as x:
            rec = ctx.profile_records()
            assert_expansions_equal(x.download(0), pairs[0][1], "segment 0 of two")
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    assert rec["io_calls/rows"][0] == 1 and not any(s in rec for s in SCOPES if s != "io_calls/rows"), rec


DEVICE_LISTS = ("extend_w16", "compress_hx", "compress_w", "keccak_inputs", "keccak_digest_addrs", "io_data")


def test_a_segment_with_its_lists_in_device_memory_between_two_with_host_lists(ctx, zkm):
    """Which lists go up differs between the segments of one launch, and where the last segment's lists lie in the scratch block depends
    on it.  THREE's middle segment has no calls, so the middle one here is "all" -- the segment with a call of every kind that takes
    lists in device memory -- with every such list there (whole: the byte lists are indexed by absolute offsets in device memory);
    "io-long" in front and "four" behind keep their lists on the host."""
    from zkm_amd import _as_words
    names = (THREE[0], "all", THREE[2])
    pairs = [wanted(ctx, zkm, name) for name in names]
    calls = [zkm.SegmentCalls(**kw) for kw, _ in pairs]
    assert all(name in calls[1].lists for name in DEVICE_LISTS) and all(calls[1].lists[name].size for name in DEVICE_LISTS)
    assert any(name in calls[0].lists for name in DEVICE_LISTS) and sum(name in calls[2].lists for name in DEVICE_LISTS) >= 5
    bufs = []
    try:
        for name in DEVICE_LISTS:
            a = calls[1].lists[name]
            bufs.append(ctx.alloc((a.nbytes + 7) // 8).upload(_as_words(a)))
            calls[1].lists[name] = bufs[-1]
        ctx.profile(True)
        ctx.profile_reset()
        try:
            x = ctx.segments_calls_expand(calls)
            rec = ctx.profile_records()
        finally:
            ctx.profile(False)
            ctx.profile_reset()
        with x:
            assert [rec[s][0] for s in SCOPES] == [1, 1, 1, 1], rec
            for s, (_, want) in enumerate(pairs):
                assert_expansions_equal(x.download(s), want, "segment %d (%s)" % (s, names[s]))
    finally:
        for b in bufs:
            b.free()


def composed(ctx, zkm, kws):
    pairs = [ctx.calls_expand(**kw) for kw in kws]
    return [s for s, _ in pairs], [o for _, o in pairs]


def free_composed(zkm, steps, ops):
    for s, o in zip(steps, ops):
        if isinstance(s.raw_rows, zkm.DeviceBuffer):
            s.raw_rows.free()
        o.free()


def prove_both_ways(ctx, zkm, kws, images=None):
    """prove_segments_ops_calls, and prove_segments_ops_steps on calls_expand's outputs; segments_tables_calls and its tables."""
    K = len(kws)
    pubs = [[1, 2, 3 + s] for s in range(K)]
    steps, ops = composed(ctx, zkm, kws)
    try:
        want = ctx.prove_segments_ops_steps(steps, ops, images=images, public_values=pubs)
        want_tables = ctx.segments_tables_steps(steps, ops, images=images)
    finally:
        free_composed(zkm, steps, ops)
    calls = [zkm.SegmentCalls(**kw) for kw in kws]
    live = ctx.memory()[0]
    got = ctx.prove_segments_ops_calls(calls, images=images, public_values=pubs)
    assert ctx.memory()[0] == live
    for s, ((p, ch, o), (wp, wch, wo)) in enumerate(zip(got, want)):
        assert o == wo and (ch == wch).all(), s
        bad = np.nonzero(p != wp)[0]
        assert bad.size == 0, "segment %d: first differing proof word %d" % (s, bad[0])
    reports = ctx.verify_segments([p for p, _, _ in got], pubs, [ch for _, ch, _ in got])
    assert [r.code for r in reports] == [0] * K, [r.message for r in reports]
    got_tables = ctx.segments_tables_calls(calls, images=images)
    assert ctx.segments_tables_calls(calls, images=images, sizing=True) == [lg for _, lg in want_tables]
    for (st, lg), (wst, wlg) in zip(got_tables, want_tables):
        assert lg == wlg
        assert_tables_equal(tables_of(st, lg, ctx), tables_of(wst, wlg, ctx))
        report = ctx.segment_check_ctls(st, lg)
        assert report.kind == 0, report.message
        st.free()
        wst.free()


def test_proofs_and_tables_of_the_three_segments_equal_the_steps_entries_on_calls_expands_outputs(ctx, zkm):
    prove_both_ways(ctx, zkm, [wanted(ctx, zkm, name)[0] for name in THREE])


def test_behind_bootstrap_images_the_first_clocks_are_the_bootstraps_rows(ctx, zkm, oracle):
    """Two segments with calls, each behind a boot image of its own (4 and 135 bootstrap rows): first_clock is nonzero and differs."""
    class BootRecorder(M.StepRecorder, BF.BootMachine):
        pass
    kws, images = [], []
    for name, spec in (("b", dict(hint_len=300, keccak=False, compress=False, seed=21)), ("a", dict(io=("hint_read",), compress=False, seed=22))):
        seg = BF.segment(oracle, name)
        s = F.record(zkm, BootRecorder(seg["model"], raw_boot=False), **spec)
        assert s["kw"]["first_clock"] == len(seg["model"].cpu_rows) > 0
        kws.append(s["kw"])
        images.append(BF.boot_image(zkm, seg["image"]))
    assert kws[0]["first_clock"] != kws[1]["first_clock"]
    prove_both_ways(ctx, zkm, kws, images=images)


def test_thirty_three_segments_are_expanded_in_two_groups(ctx, zkm):
    kw, want = wanted(ctx, zkm, "two")
    other, want_other = wanted(ctx, zkm, "io-long")
    calls = [zkm.SegmentCalls(**kw) for _ in range(33)]
    calls[31] = zkm.SegmentCalls(**other)                     # (the first group's last segment differs from its neighbours)
    live, waits = ctx.memory()[0], ctx.host_waits()
    with ctx.segments_calls_expand(calls) as x:
        assert ctx.host_waits() - waits == 2 and len(x) == 33
        for s in (0, 31, 32):
            assert_expansions_equal(x.download(s), want_other if s == 31 else want, "segment %d" % s)
    assert ctx.memory()[0] == live


def test_a_refused_call_leaves_live_memory_alone_and_the_context_passes_case_1(ctx, zkm):
    kws = [wanted(ctx, zkm, name)[0] for name in THREE]
    q = kws[2]["insns"]
    twice = q[1].copy()
    twice[7] = twice[6]
    bad = dict(kws[2], insns=(q[0], twice))
    live, waits = ctx.memory()[0], ctx.host_waits()
    with pytest.raises(zkm.ZkmError, match=r"zkm_segments_calls_expand: segment 1: instruction record row 7 \(clock %d\): two records on one clock" % twice[7]):
        ctx.segments_calls_expand([zkm.SegmentCalls(**kw) for kw in (kws[0], bad, kws[2])])
    with pytest.raises(zkm.ZkmError, match=r"zkm_prove_segments_ops_calls: segment 1: instruction record row 7"):
        ctx.prove_segments_ops_calls([zkm.SegmentCalls(**kw) for kw in (kws[0], bad, kws[2])])
    assert ctx.memory()[0] == live and ctx.host_waits() == waits      # every refusal on the host, before any device work
    # the segment's own rows, or a list the host reads, in device memory
    steps = kws[0]["steps"]
    dev = ctx.alloc(max(steps.raw_rows.size, 1)).upload(steps.raw_rows.reshape(-1))
    waits = ctx.host_waits()
    try:
        with pytest.raises(zkm.ZkmError, match=r"zkm_segments_calls_expand: segment 0: steps.raw_rows: device memory"):
            ctx.segments_calls_expand([zkm.SegmentCalls(**dict(kws[0], steps=zkm.CpuSteps(steps.steps, dev, nraw=steps.nraw)))])
        st = zkm.SegmentCalls(**kws[0]).struct()
        st.io_meta = dev.ptr
        arr = (zkm.SegmentCallsStruct * 2)(zkm.SegmentCalls(**kws[1]).struct(), st)
        h, err = C.c_void_p(), C.c_char_p()
        assert ctx.L.zkm_segments_calls_expand(ctx.h, 2, C.addressof(arr), C.byref(h), C.byref(err)) != 0 and h.value is None
        assert err.value.decode().startswith("zkm_segments_calls_expand: segment 1: io_meta: device memory")
        assert ctx.host_waits() == waits
    finally:
        dev.free()
    assert ctx.memory()[0] == live
    case_1(ctx, zkm)
