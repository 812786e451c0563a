"""GPU suite: the pool proves segments as the emulator records them (zkm_pool_prove_segments_calls), its workers keeping one group staged
ahead of the proofs ("pool_stage_ahead" 1, the default) or expanding each group in its call (0).  The judge is always
Context.prove_segments_ops_calls on one plain context with the same list: proofs, challenges and offsets word for word, whatever the
worker count, max_stack or mode.  A refusal -- found on the host, or by the placement on the device -- names the worker, the device and
the segment's position in the pool call, frees every handle and leaves every worker's memory as it was."""
import ctypes as C

import numpy as np
import pytest

from . import boot_fixtures as BF
from . import calls_entry_fixtures as F
from .test_gpu_calls_stage import BootRecorder, assert_same_proofs

pytestmark = pytest.mark.gpu

PUBS = [[1, 2, 3 + s] for s in range(5)]


def own_operations():
    """Operations of the segment's own for every list the calls append to, as calls_entry_fixtures.own_operations() gives them to the
    suites that compare the expansion's words -- but here the segment is PROVEN, and the judge refuses that fixture's random words
    ("Logic: op code out of range"): the same lists with the same counts, holding operations the tables take (two words written and
    read back, an and / an xor / an or, the fixture's own arithmetic operations and Keccak inputs)."""
    fixture = F.own_operations()
    memory = np.array([(0, 0, 0x70000, 100, 0, 7), (0, 0, 0x70000, 110, 1, 7), (0, 0, 0x70004, 120, 0, 9), (0, 0, 0x70004, 130, 1, 9),
                       (0, 0, 0x70008, 140, 0, 11)], dtype=np.uint64)
    logic = np.array([(0, 0xF0F0F0F0, 0x0FF00FF0), (2, 5, 6), (1, 0x80000001, 0x7FFFFFFE)], dtype=np.uint32)
    assert memory.shape == fixture["memory_ops"].shape and logic.shape == fixture["logic_ops"].shape
    return dict(fixture, memory_ops=memory, logic_ops=logic)


def kws_of(zkm):
    """L of the suite: I/O alone, no calls at all (a plain step log), all four kinds, every kind with operations of its own, two calls."""
    return [F.segment(zkm, "io-long")["kw"], F.segment(zkm, "plain")["kw"], F.segment(zkm, "four")["kw"],
            dict(F.segment(zkm, "all")["kw"], **own_operations()), F.segment(zkm, "two")["kw"]]


def calls_of(zkm, kws):
    return [zkm.SegmentCalls(**kw) for kw in kws]


@pytest.fixture(scope="module")
def judged(ctx, zkm):
    """The judge on the five segments: computed once, shared, not to be changed."""
    kws = kws_of(zkm)
    assert zkm.segment_calls_steps(zkm.SegmentCalls(**kws[1]))[1]["nraw"] == kws[1]["steps"].nraw      # "plain": a step log without calls
    return kws, ctx.prove_segments_ops_calls(calls_of(zkm, kws), public_values=PUBS)


@pytest.fixture(scope="module")
def pool1(zkm):
    p = zkm.Pool((0,), 1)
    yield p
    p.close()


@pytest.fixture(scope="module")
def pool2(zkm):
    p = zkm.Pool((0,), 2)
    yield p
    p.close()


def memories(pool):
    """Every worker context's live memory, read through the pool's contexts, without the tables a context keeps for reuse (twiddles,
    power tables: a worker that proves a height for the first time keeps them, as every suite of the project counts)."""
    return [pool.memory(w)[0] - pool.resident_bytes(w) for w in range(pool.workers())]


# ---------------------------------------------------------------- 1. one worker, three groups
def test_one_worker_stages_ahead_twice_and_both_modes_equal_the_judge(zkm, judged, pool1):
    kws, want = judged
    assert zkm.pool_plan(5, 1, 2) == [2, 2, 1]
    live = memories(pool1)
    try:
        for mode in (1, 0):
            pool1.set_tuning("pool_stage_ahead", mode)
            assert_same_proofs(pool1.prove_segments_calls(calls_of(zkm, kws), public_values=PUBS, max_stack=2), want)
            assert [pool1.last_assignment(s) for s in range(5)] == [(0, 0), (0, 0), (0, 1), (0, 1), (0, 2)]
            assert memories(pool1) == live
    finally:
        pool1.set_tuning("pool_stage_ahead", 1)


# ---------------------------------------------------------------- 2. two workers, four groups
def test_two_workers_four_groups_equal_the_judge(zkm, judged, pool2):
    kws, want = judged
    plan = zkm.pool_plan(5, 2, 2)
    assert plan == [2, 1, 1, 1]
    live = memories(pool2)
    assert_same_proofs(pool2.prove_segments_calls(calls_of(zkm, kws), public_values=PUBS, max_stack=2), want)
    who = [pool2.last_assignment(s) for s in range(5)]
    assert {w for w, _ in who} <= {0, 1}
    assert [g for _, g in who] == [0, 0, 1, 2, 3] and len({g for _, g in who}) == len(plan)
    assert memories(pool2) == live


# ---------------------------------------------------------------- 3. boot images
def test_behind_boot_images_and_a_plain_step_log_in_both_modes(ctx, zkm, oracle, judged, pool1):
    """Two segments behind boot images of their own (4 and 135 bootstrap rows), one group staged ahead of the other.  "plain" was not
    recorded behind an image (its first_clock is 0), so it is proven in a call of its own, without images."""
    kws, images = [], []
    for name, spec in (("b", dict(hint_len=300, keccak=False, compress=False, seed=21)), ("a", dict(io=("hint_read",), compress=False, seed=22))):
        seg = BF.segment(oracle, name)
        kws.append(F.record(zkm, BootRecorder(seg["model"], raw_boot=False), **spec)["kw"])
        images.append(BF.boot_image(zkm, seg["image"]))
    assert [kw["first_clock"] for kw in kws] == [4, 135]
    pubs = [[1, 2, 3], [4, 5, 6]]
    want = ctx.prove_segments_ops_calls(calls_of(zkm, kws), images=images, public_values=pubs)
    plain, want_plain = judged[0][1:2], judged[1][1:2]
    live = memories(pool1)
    try:
        for mode in (1, 0):
            pool1.set_tuning("pool_stage_ahead", mode)
            assert_same_proofs(pool1.prove_segments_calls(calls_of(zkm, kws), images=images, public_values=pubs, max_stack=1), want)
            assert_same_proofs(pool1.prove_segments_calls(calls_of(zkm, plain), public_values=PUBS[1:2]), want_plain)
            assert memories(pool1) == live
    finally:
        pool1.set_tuning("pool_stage_ahead", 1)


# ---------------------------------------------------------------- 4. and 5. refusals
def alone(ctx, zkm, bad):
    """What the judge says of the bad segment alone, behind "segment 0: "."""
    with pytest.raises(zkm.ZkmError) as e:
        ctx.prove_segments_ops_calls([zkm.SegmentCalls(**bad)])
    text = str(e.value)
    assert text.startswith("zkm_prove_segments_ops_calls: segment 0: ")
    return text[len("zkm_prove_segments_ops_calls: segment 0: "):]


def refused(zkm, pool, kws, bad, mode):
    """The five segments with `bad` at position 3, through the pool: the message; memory back; handles gone."""
    live = memories(pool)
    pool.set_tuning("pool_stage_ahead", mode)
    try:
        with pytest.raises(zkm.ZkmError) as e:
            pool.prove_segments_calls(calls_of(zkm, kws[:3] + [bad] + kws[4:]), public_values=PUBS, max_stack=2)
    finally:
        pool.set_tuning("pool_stage_ahead", 1)
    msg = str(e.value)
    assert msg.startswith("worker ") and "(device 0), segments 3..3: " in msg and "segment 3: " in msg, msg
    assert memories(pool) == live
    with pytest.raises(zkm.ZkmError, match="was not proven"):      # the refused group's segment stays unassigned
        pool.last_assignment(3)
    return msg.split("segments 3..3: ", 1)[1]


@pytest.mark.parametrize("mode", [1, 0])
def test_a_refusal_found_on_the_host_names_worker_device_and_position(ctx, zkm, judged, pool2, mode):
    kws, want = judged
    k = F.segment(zkm, "four")["kw"]["keccak"]
    bad_off = k[1].copy()
    bad_off[-1] -= 2                                                   # a Keccak call of 138 bytes
    bad = dict(F.segment(zkm, "four")["kw"], keccak=(k[0], bad_off, k[2], k[3]))
    reason = alone(ctx, zkm, bad)
    assert "length 138 is not a positive multiple of 4" in reason
    inner = refused(zkm, pool2, kws, bad, mode)
    name = "zkm_segments_calls_stage" if mode else "zkm_pool_prove_segments_calls"
    assert inner == name + ": segment 3: " + reason, inner
    # the same pool then proves the good list
    pool2.set_tuning("pool_stage_ahead", mode)
    try:
        assert_same_proofs(pool2.prove_segments_calls(calls_of(zkm, kws), public_values=PUBS, max_stack=2), want)
    finally:
        pool2.set_tuning("pool_stage_ahead", 1)


@pytest.mark.parametrize("mode", [1, 0])
def test_a_refusal_found_on_the_device_reads_as_the_gets_or_the_expansions(ctx, zkm, judged, pool2, mode):
    """Two records on one clock: the placement kernel finds it where a worker stages ahead (zkm_staged_calls_get reports it), the
    expansion's host loop where it does not -- in the same words."""
    kws, want = judged
    q = F.segment(zkm, "four")["kw"]["insns"]
    twice = q[1].copy()
    twice[7] = twice[6]
    bad = dict(F.segment(zkm, "four")["kw"], insns=(q[0], twice))
    reason = alone(ctx, zkm, bad)
    assert reason == "instruction record row 7 (clock %d): two records on one clock" % twice[7]
    inner = refused(zkm, pool2, kws, bad, mode)
    name = "zkm_staged_calls_get" if mode else "zkm_pool_prove_segments_calls"
    assert inner == name + ": segment 3: " + reason, inner
    assert_same_proofs(pool2.prove_segments_calls(calls_of(zkm, kws), public_values=PUBS, max_stack=2), want)


# ---------------------------------------------------------------- 6. sizing alone
def test_the_sizing_call_gives_the_offsets_the_proving_call_reproduces(zkm, judged, pool2):
    kws, want = judged
    live = memories(pool2)
    sizes = pool2.prove_segments_calls(calls_of(zkm, kws), public_values=PUBS, max_stack=2, sizing=True)
    assert sizes == [o for _, _, o in want] and all(len(o) == 13 and o[12] > 0 for o in sizes)
    assert {pool2.last_assignment(s)[1] for s in range(5)} == {0, 1, 2, 3}
    # the proving call alone, on buffers of those sizes
    m = zkm._marshal_ops([q.own for q in calls_of(zkm, kws)], PUBS, pool2.standard_config())
    m.offs[:] = [x for o in sizes for x in o]
    m.alloc()
    m.offs[:] = [0] * len(m.offs)
    calls = calls_of(zkm, kws)
    arr, err, cfg = zkm.Context._calls_array(calls), C.c_char_p(), pool2.standard_config()
    rc = pool2.L.zkm_pool_prove_segments_calls(pool2.h, C.byref(cfg), 5, 2, None, C.addressof(arr), m.pv, m.npv, m.po, m.offs, m.co, C.byref(err))
    assert rc == 0, err.value
    assert [list(m.offs[13 * s:13 * s + 13]) for s in range(5)] == sizes
    assert_same_proofs(m.results(), want)
    assert memories(pool2) == live
