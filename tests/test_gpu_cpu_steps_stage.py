"""GPU suite: step logs walked on the device (zkm_cpu_steps_scan) and staged behind the current proofs (zkm_cpu_steps_stage,
zkm_staged_steps_get; csrc/cpu_steps_walk.hip).  The judges are those of tests/test_gpu_cpu_steps.py: the recorded sample program of
tests/cpu_steps_model.py, the host walk through zkm_cpu_steps_counts -- its counts, its counts of the prefixes steps[:256 k] for the
base triples, its messages character for character -- and the unstaged *_steps calls, word for word.  Nothing above 2^10 rows."""
import ctypes as C

import numpy as np
import pytest

from . import boot_fixtures as BF
from . import cpu_fixtures as CF
from . import cpu_steps_model as M
from .test_cpu_steps import step
from .test_gpu_cpu_steps import own_ops, segment_pair, two  # noqa: F401  (two: a module-scoped fixture)
from .test_gpu_segment_ops import assert_tables_equal, tables_of

pytestmark = pytest.mark.gpu

P = CF.P
COUNTS = "zkm_cpu_steps_counts: "
SCAN = "zkm_cpu_steps_scan: segment %d: "


def steps_of(zkm, n):
    """A list of n steps of the sample program recorded four times over: cut where it is longer, PAD-filled where it is shorter."""
    m = M.sample(4)
    arr = m.step_array()
    assert len(arr) > 3 * 256 + 17
    out = np.zeros(n, dtype=M.STEP_DT)
    out["kind"] = M.KIND["PAD"]
    out[:min(n, len(arr))] = arr[:n]
    return zkm.CpuSteps(out, m.raw_array())


def host_bases(zkm, st):
    """The base triples the host walk uploads: the counts of the prefixes steps[:256 k], from the pure function."""
    return np.array([zkm.cpu_steps_counts(zkm.CpuSteps(st.steps[:256 * k], st.raw_rows)) for k in range((st.steps.size + 255) // 256)],
                    dtype=np.uint32).reshape(-1, 3)


def host_refusal(zkm, st):
    """The host walk's message for a refused list, without the entry point's prefix."""
    with pytest.raises(zkm.ZkmError) as e:
        zkm.cpu_steps_counts(st)
    assert str(e.value).startswith(COUNTS)
    return str(e.value)[len(COUNTS):]


def scan_refusal(zkm, ctx, lists):
    with pytest.raises(zkm.ZkmError) as e:
        ctx.cpu_steps_scan(lists)
    return str(e.value)


# ---------------------------------------------------------------- counts and bases
@pytest.mark.parametrize("n", [1, 64, 65, 255, 256, 257, 3 * 256 + 17])
def test_counts_and_bases_equal_the_host_walk(ctx, zkm, n):
    st = steps_of(zkm, n)
    counts, bases = ctx.cpu_steps_scan([st], bases=True)
    assert counts == [zkm.cpu_steps_counts(st)]
    assert bases[0].shape == ((n + 255) // 256, 3) and (bases[0] == host_bases(zkm, st)).all()


def test_three_segments_of_different_lengths_in_one_call(ctx, zkm):
    """The grid is the longest segment's (four workgroups); the others' spare workgroups write nothing -- every output is poisoned
    first, the base arrays are all as long as the longest segment's, and what lies behind a segment's own triples stays poison."""
    lists = [steps_of(zkm, n) for n in (257, 1, 785)]
    poison = np.uint32(0xA5A5A5A5)
    bases = [np.full((4, 3), poison, dtype=np.uint32) for _ in lists]
    counts, _ = ctx.cpu_steps_scan(lists, bases=bases)
    for st, c, b in zip(lists, counts, bases):
        k = (st.steps.size + 255) // 256
        assert c == zkm.cpu_steps_counts(st)
        assert (b[:k] == host_bases(zkm, st)).all() and (b[k:] == poison).all()
    # entries of base_out may be NULL, and so may the array
    counts2, some = ctx.cpu_steps_scan(lists, bases=[None, np.full((1, 3), poison, dtype=np.uint32), None])
    assert counts2 == counts == ctx.cpu_steps_scan(lists) and (some[1] == 0).all()
    # records in device memory are read in place
    dev = ctx.alloc(lists[2].steps.size * 6).upload(lists[2].steps.view(np.uint64))
    try:
        assert ctx.cpu_steps_scan([DeviceSteps(zkm, dev.ptr, lists[2])]) == counts[2:]
    finally:
        dev.free()


class DeviceSteps:
    """A step list whose records lie in device memory at `ptr` (no staged handle owns them)."""

    def __init__(self, zkm, ptr, like):
        self.st = like.struct()
        self.st.steps = ptr
        self.keep = like

    def struct(self):
        return self.st


# ---------------------------------------------------------------- refusals
def refused_list(zkm, bad, at, n=512):
    """n steps of the sample (twice over, PAD-filled) with the record `bad` at position `at`."""
    m = M.sample(2)
    out = np.zeros(n, dtype=M.STEP_DT)
    out["kind"] = M.KIND["PAD"]
    arr = m.step_array()
    out[:len(arr)] = arr
    for a, b in zip(np.atleast_1d(at), bad if isinstance(bad, list) else [bad]):
        out[a] = b[0]
    return zkm.CpuSteps(out, m.raw_array())


def bad_steps(nraw):
    return {"unknown kind": step(77), "encoding": step("BINARY_OP", 0x18, (1, 2)), "syscall flags": step("SYSCALL", 0xC, (0, 0, 0, 0), flags=1 | 4 << 8),
            "teq of equal operands": step("TEQ", 0x34, (7, 7)), "raw index": step("RAW", 0, (nraw, 0)), "raw mask above the channels": step("RAW", 0, (1, 0x100))}


@pytest.mark.parametrize("kind", list(bad_steps(0)))
def test_every_refusal_at_every_position_reads_as_the_host_walks(ctx, zkm, kind):
    bad = bad_steps(len(M.sample(2).raw_rows))[kind]
    for at in (0, 511, 255, 256):
        st = refused_list(zkm, bad, at)
        want = host_refusal(zkm, st)
        assert want.startswith("step %d: " % at)
        assert scan_refusal(zkm, ctx, [st]) == SCAN % 0 + want


def test_the_lower_of_two_bad_steps_and_a_bad_step_in_segment_one_of_three(ctx, zkm):
    b = bad_steps(len(M.sample(2).raw_rows))
    for at, bad in (((300, 40), [b["unknown kind"], b["teq of equal operands"]]), ((63, 64), [b["encoding"], b["raw index"]]),
                    ((256, 255), [b["syscall flags"], b["raw mask above the channels"]])):
        st = refused_list(zkm, bad, at)
        want = host_refusal(zkm, st)
        assert want.startswith("step %d: " % min(at))
        assert scan_refusal(zkm, ctx, [st]) == SCAN % 0 + want
    good = [steps_of(zkm, 257), steps_of(zkm, 1)]
    st = refused_list(zkm, b["encoding"], 17)
    assert scan_refusal(zkm, ctx, [good[0], st, good[1]]) == SCAN % 1 + host_refusal(zkm, st)
    assert ctx.cpu_steps_scan(good) == [zkm.cpu_steps_counts(g) for g in good]       # the context is as usable as before


def test_a_device_row_whose_used_cells_disagree_with_the_mask_is_refused(ctx, zkm):
    """The hole the host walk leaves: it cannot read rows in device memory.  The device walk can -- the text is the one the host walk
    gives for the same rows in host memory, words >= p among the cells included."""
    m = M.sample(2)
    steps, raw = m.step_array(), m.raw_array().copy()
    raw[raw < (1 << 32) - 1] += np.uint64(P)
    at = [i for i in range(len(steps)) if steps["kind"][i] == M.KIND["RAW"]]
    assert len(at) >= 3 and steps["reads"][at[0], 1] == 0b111
    dev = ctx.alloc(raw.size).upload(raw)
    try:
        on_device = lambda s: zkm.CpuSteps(s, dev, nraw=len(raw))
        assert ctx.cpu_steps_scan([on_device(steps)]) == [zkm.cpu_steps_counts(zkm.CpuSteps(steps, raw))]
        for i, mask in ((at[0], 0b011), (at[1], 0b1), (at[-1], steps["reads"][at[-1], 1] ^ 0x80)):
            bad = steps.copy()
            bad["reads"][i, 1] = mask
            want = host_refusal(zkm, zkm.CpuSteps(bad, raw))
            assert "RAW row %d uses the channels" % bad["reads"][i, 0] in want
            assert scan_refusal(zkm, ctx, [on_device(bad)]) == SCAN % 0 + want
            assert scan_refusal(zkm, ctx, [zkm.CpuSteps(bad, raw)]) == SCAN % 0 + want          # host rows go up with the records
            with ctx.cpu_steps_stage([on_device(bad)]) as h:
                with pytest.raises(zkm.ZkmError) as e:
                    h.get(0)
                assert str(e.value) == "zkm_staged_steps_get: segment 0: " + want
    finally:
        dev.free()


# ---------------------------------------------------------------- staged equals unstaged, word for word
def assert_same_tables(ctx, got, want, free_want=False):
    for (st, lg), (wst, wlg) in zip(got, want):
        assert lg == wlg
        assert_tables_equal(tables_of(st, lg, ctx), tables_of(wst, wlg, ctx))
        st.free()
        if free_want:
            wst.free()


def test_tables_of_staged_steps_equal_the_unstaged_call(ctx, zkm, two):
    segs = two["own"]
    steps, ops = [s for s, _, _ in segs], [o for _, o, _ in segs]
    live = ctx.memory()[0]
    want = ctx.segments_tables_steps(steps, ops)
    assert [lg[1] for _, lg in want] == [8, 9]
    with ctx.cpu_steps_stage(steps) as h:
        staged = [h.get(0), h.get(1)]
        assert [s.counts() for s in staged] == [zkm.cpu_steps_counts(s) for s in steps]
        assert_same_tables(ctx, ctx.segments_tables_steps(staged, ops), want)
        assert ctx.segments_tables_steps(staged, ops, sizing=True) == [lg for _, lg in want]
        # one segment staged and one not, either way round
        assert_same_tables(ctx, ctx.segments_tables_steps([staged[0], steps[1]], ops), want)
        assert_same_tables(ctx, ctx.segments_tables_steps([steps[0], staged[1]], ops), want)
        # the own lists staged through zkm_segment_ops_stage in the same call (that call stages CPU rows too: one row that the *_steps
        # call is not handed -- cpu_rows NULL, ncpu_rows 0 -- beside the staged lists)
        handles, staged_ops = [], []
        for _, o, _ in segs:
            with_row = zkm.SegmentOps(np.zeros((1, CF.W), dtype=np.uint64), o.lists["memory_ops"], arithmetic_ops=o.lists["arithmetic_ops"],
                                      logic_ops=o.lists["logic_ops"])
            handles.append(ctx.stage_segment_ops(with_row))
            so = handles[-1].ops()
            so._staged_struct.cpu_rows, so._staged_struct.ncpu_rows = None, 0
            staged_ops.append(so)
        assert_same_tables(ctx, ctx.segments_tables_steps(staged, staged_ops), want)
        assert_same_tables(ctx, ctx.segments_tables_steps([steps[0], staged[1]], [ops[0], staged_ops[1]]), want, free_want=True)
        for sh in handles:
            sh.free()
    assert ctx.memory()[0] == live


def test_staged_steps_behind_a_bootstrap_image(ctx, zkm, oracle):
    class BootRecorder(M.StepRecorder, BF.BootMachine):
        pass
    images, steps, beside = [], [], []
    for name, own in (("b", own_ops(3, 10 << 8)), ("a", None)):
        seg = BF.segment(oracle, name)
        model = seg["model"]
        m = CF.sample_program(BootRecorder(model, raw_boot=False))
        nboot = len(model.cpu_rows)
        s, o, _ = segment_pair(zkm, m, int(len(m.rows) - 1).bit_length(), own, nboot=nboot, boot_mem=len(model.memory_ops))
        images.append(BF.boot_image(zkm, seg["image"]))
        steps.append(s), beside.append(o)
    want = ctx.segments_tables_steps(steps, beside, images=images)
    assert [lg[1] for _, lg in want] == [8, 9]
    with ctx.cpu_steps_stage(steps) as h:
        assert_same_tables(ctx, ctx.segments_tables_steps([h.get(0), h.get(1)], beside, images=images), want)
        assert_same_tables(ctx, ctx.segments_tables_steps([steps[0], h.get(1)], beside, images=images), want, free_want=True)


def assert_same_proofs(got, want):
    for s, ((p, c, o), (wp, wc, wo)) in enumerate(zip(got, want)):
        assert o == wo and (c == wc).all(), s
        bad = np.nonzero(p != wp)[0]
        assert bad.size == 0, "segment %d: first differing proof word %d" % (s, bad[0])


@pytest.fixture(scope="module")
def proven(ctx, two):
    """The unstaged proving call on the `two` fixture's bare segments: computed once, shared, not to be changed."""
    segs = two["bare"]
    pubs = [[1, 2, 3], [7, 1]]
    return segs, pubs, ctx.prove_segments_ops_steps([s for s, _, _ in segs], [o for _, o, _ in segs], public_values=pubs)


def test_proofs_of_staged_steps_equal_the_unstaged_call(ctx, zkm, proven):
    segs, pubs, want = proven
    ops = [o for _, o, _ in segs]
    with ctx.cpu_steps_stage([s for s, _, _ in segs]) as h:
        assert_same_proofs(ctx.prove_segments_ops_steps([h.get(0), h.get(1)], ops, public_values=pubs), want)
        assert_same_proofs(ctx.prove_segments_ops_steps([h.get(0), segs[1][0]], ops, public_values=pubs), want)


# ---------------------------------------------------------------- ordering
def pinned_steps(zkm, ctx, st):
    """The same list with records and rows in page-locked memory; returns (CpuSteps, the pinned arrays)."""
    rec = ctx.pinned_array(st.steps.size * 6)
    rec[:] = st.steps.view(np.uint64)
    raw = ctx.pinned_array(max(st.raw_rows.size, 1))
    raw[:st.raw_rows.size] = st.raw_rows.reshape(-1)
    return zkm.CpuSteps(rec.view(M.STEP_DT), raw[:st.raw_rows.size].reshape(-1, CF.W)), (rec, raw)


def test_staged_from_pinned_memory_and_consumed_at_once(ctx, zkm, proven):
    segs, pubs, want = proven
    ops = [o for _, o, _ in segs]
    pins = [pinned_steps(zkm, ctx, s) for s, _, _ in segs]
    try:
        assert all(p.steps.ctypes.data == arrs[0].ctypes.data for p, arrs in pins)       # (the pinned words themselves are staged)
        # no ready(wait) between the stage and the call that consumes it
        with ctx.cpu_steps_stage([p for p, _ in pins]) as h:
            assert_same_proofs(ctx.prove_segments_ops_steps([h.get(0), h.get(1)], ops, public_values=pubs), want)
        # the source may be reused once ready() says so: overwritten before the call, the results are unchanged
        with ctx.cpu_steps_stage([p for p, _ in pins]) as h:
            assert h.ready(wait=True) is True and h.ready() is True
            for _, (rec, raw) in pins:
                rec[:] = np.uint64(0xDEADBEEFDEADBEEF)
                raw[:] = np.uint64(P - 1)
            assert_same_proofs(ctx.prove_segments_ops_steps([h.get(0), h.get(1)], ops, public_values=pubs), want)
    finally:
        for _, arrs in pins:
            for a in arrs:
                ctx.free_pinned(a)


# ---------------------------------------------------------------- host waits
def test_host_waits_of_the_stage_the_get_and_the_builder(ctx, zkm, two):
    segs = two["own"]
    steps, ops = [s for s, _, _ in segs], [o for _, o, _ in segs]
    for st, _ in ctx.segments_tables_steps(steps, ops):      # (the first call may grow the download area)
        st.free()
    w0 = ctx.host_waits()
    h = ctx.cpu_steps_stage(steps)
    w1 = ctx.host_waits()
    staged = [h.get(0), h.get(1), h.get(0)]
    w2 = ctx.host_waits()
    got = ctx.segments_tables_steps(staged[:2], ops)
    w3 = ctx.host_waits()
    assert (w1 - w0, w3 - w2) == (0, 3) and w2 - w1 <= 1
    for st, _ in got:
        st.free()
    h.free()
    w4 = ctx.host_waits()
    assert ctx.cpu_steps_scan(steps) == [zkm.cpu_steps_counts(s) for s in steps] and ctx.host_waits() - w4 == 1


# ---------------------------------------------------------------- handles, and refusals at the entry points
def test_a_refused_segment_leaves_the_others_and_the_context_usable(ctx, zkm, two):
    segs = two["own"]
    steps, ops = [s for s, _, _ in segs], [o for _, o, _ in segs]
    bad = zkm.CpuSteps(steps[0].steps.copy(), steps[0].raw_rows)
    bad.steps["kind"][200] = 99
    live = ctx.memory()[0]
    want = ctx.segments_tables_steps(steps, ops)
    with ctx.cpu_steps_stage([steps[0], bad, steps[1]]) as h:
        assert len(h) == 3
        with pytest.raises(zkm.ZkmError) as e:
            h.get(1)
        assert str(e.value) == "zkm_staged_steps_get: segment 1: step 200: unknown kind 99" == "zkm_staged_steps_get: segment 1: " + host_refusal(zkm, bad)
        with pytest.raises(zkm.ZkmError, match="zkm_staged_steps_get: no segment 3: the handle holds 3"):
            h.get(3)
        assert_same_tables(ctx, ctx.segments_tables_steps([h.get(0), h.get(2)], ops), want, free_want=True)
    assert ctx.memory()[0] == live
    # freed with the upload possibly still in flight, and dropped without free(): the block comes back
    ctx.cpu_steps_stage(steps).free()
    h = ctx.cpu_steps_stage(steps)
    del h
    import gc
    gc.collect()
    assert ctx.memory()[0] == live


def test_refusals_at_the_entry_points(ctx, zkm, two):
    segs = two["own"]
    steps, ops = [s for s, _, _ in segs], [o for _, o, _ in segs]
    live = ctx.memory()[0]
    want = ctx.segments_tables_steps(steps, ops)
    # a handle staged on another context
    other = zkm.Context(0)
    try:
        with other.cpu_steps_stage(steps) as h:
            for call in (lambda s: ctx.segments_tables_steps(s, ops), lambda s: ctx.prove_segments_ops_steps(s, ops)):
                with pytest.raises(zkm.ZkmError, match="segment 1: Cpu: the steps were staged on another context"):
                    call([steps[0], h.get(1)])
    finally:
        other.close()
    # records in device memory that no handle owns
    dev = ctx.alloc(steps[0].steps.size * 6).upload(steps[0].steps.view(np.uint64))
    try:
        with pytest.raises(zkm.ZkmError, match="segment 0: Cpu: steps in device memory that no staged handle owns"):
            ctx.segments_tables_steps([DeviceSteps(zkm, dev.ptr, steps[0]), steps[1]], ops)
    finally:
        dev.free()
    with ctx.cpu_steps_stage(steps) as h:
        # what get hands out is taken as it is
        cut = h.get(0)
        cut.struct().nsteps -= 128
        with pytest.raises(zkm.ZkmError, match="segment 0: Cpu: staged steps are taken as zkm_staged_steps_get hands them out"):
            ctx.segments_tables_steps([cut, steps[1]], ops)
        # the host's refusals, made before any device work
        L, err, out = ctx.L, C.c_char_p(), C.c_void_p()
        sl = (zkm.CpuStepsStruct * 2)(steps[0].struct(), zkm.CpuStepsStruct(None, 0, None, 3))
        assert L.zkm_cpu_steps_stage(ctx.h, 2, sl, C.byref(out), C.byref(err)) == 1 and not out.value
        assert err.value == b"zkm_cpu_steps_stage: segment 1: null pointer with a nonzero count"
        sl[1] = zkm.CpuStepsStruct(steps[0].steps.ctypes.data, (1 << 28) + 1, None, 0)
        assert L.zkm_cpu_steps_stage(ctx.h, 2, sl, C.byref(out), C.byref(err)) == 1 and not out.value
        assert err.value == b"zkm_cpu_steps_stage: segment 1: 268435457 steps, more than 2^28"
        assert L.zkm_cpu_steps_stage(ctx.h, 0, sl, C.byref(out), C.byref(err)) == 1 and err.value == b"zkm_cpu_steps_stage: no segments"
        # after every refusal the context builds the good lists, staged or not
        assert_same_tables(ctx, ctx.segments_tables_steps([h.get(0), h.get(1)], ops), want, free_want=True)
    assert ctx.memory()[0] == live
