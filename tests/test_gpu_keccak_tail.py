"""GPU suite: SYSKECCAK calls of any byte length expanded on the device (ZKM_SPONGE_PADDED_TAIL).  The judge is
tests/keccak_tail_model.py, a restatement of generate_keccak and keccak_sponge_log for any length written from the reference's text:
all five outputs of zkm_keccak_calls_witness equal it word for word for every length at which the last word, the read rows or the
blocks take another shape; whole segments built from the recorded calls equal, table by table and proof word by proof word, the same
segments host-expanded from the model; zkm_segment_check -- code that shares nothing with the model -- finds those tables consistent,
and names the Memory table when the host-expanded read rows hold a zero-extended last word instead of the padded one; the staged
entry and the pool give the one-context call's proofs."""
import numpy as np
import pytest

from . import keccak_tail_fixtures as TF
from . import keccak_tail_model as TM
from .test_gpu_calls_stage import assert_same_proofs, outputs
from .test_gpu_keccak_calls import assert_outputs_equal
from .test_gpu_segment_ops import assert_tables_equal, tables_of

pytestmark = pytest.mark.gpu

FLAG, TAIL = np.uint64(TM.FLAG), np.uint64(TM.TAIL)
PUBS = [[1, 2, 3], [4, 5, 6], [7, 8, 9]]


# ---------------------------------------------------------------- the kernel's outputs against the model
def test_every_length_in_one_list_equals_the_model(ctx, zkm):
    lists, want = TF.all_lengths()
    assert (want[0].shape[0], want[1].shape[0], want[2].shape[0], want[3].shape[0]) == zkm.keccak_calls_counts(lists[1], lists[2])
    assert_outputs_equal(ctx.keccak_calls_witness(*lists), want)


def test_lists_in_device_memory_inside_a_block_of_ff_bytes(ctx, zkm):
    """The inputs lie in device memory from an unaligned offset on, every call whose length is no multiple of 4 is followed by 0xFF
    bytes, and behind the last call (273 bytes) the caller's block goes on with 0xFF: a lane that loads a byte at or beyond the end of
    a call writes a wrong word."""
    from zkm_amd import _as_words
    (inputs, off, meta, daddrs), want = TF.all_lengths()
    n = len(meta)
    assert int(off[-1] - off[-2]) % 4 and all(inputs[int(off[k + 1])] == 0xFF for k in range(n - 1) if int(off[k + 1] - off[k]) % 4)
    lead = 13
    block = np.full(lead + inputs.size + 243, 0xFF, dtype=np.uint8)
    block[lead:lead + inputs.size] = inputs
    rows, mem, logic, perms = zkm.keccak_calls_counts(off + lead, meta)
    outs = [ctx.alloc(w) for w in (rows * 259, mem * 6, (logic * 3 + 1) // 2, perms * 25, perms)]
    dev = [ctx.alloc((a.nbytes + 7) // 8).upload(_as_words(a)) for a in (block, daddrs)]

    def download():
        return (outs[0].download().reshape(rows, 259), outs[1].download().reshape(mem, 6), outs[2].download().view(np.uint32)[:logic * 3].reshape(logic, 3),
                outs[3].download().reshape(perms, 25), outs[4].download())
    try:
        ctx.keccak_calls_witness_into((dev[0], off + lead, meta, dev[1]), n, *[b.ptr for b in outs])
        assert_outputs_equal(download(), want)
        for b in outs:
            b.upload(np.zeros(b.words, dtype=np.uint64))
        ctx.keccak_calls_witness_into((block, off + lead, meta, daddrs), n, *[b.ptr for b in outs])      # the same from host memory
        assert_outputs_equal(download(), want)
        # metas in device memory are not read by the host: such a list takes multiples of 4 only, as before
        dev_meta = ctx.alloc(4 * n).upload(_as_words(meta))
        try:
            with pytest.raises(zkm.ZkmError, match=r"zkm_keccak_calls_witness: input_off: call 0: length 1 is not a positive multiple of 4"):
                ctx.keccak_calls_witness_into((dev[0], off + lead, dev_meta, dev[1]), n, *[b.ptr for b in outs])
        finally:
            dev_meta.free()
    finally:
        for b in dev + outs:
            b.free()


def test_a_mixed_list_and_a_refused_call_that_leaves_the_context_usable(ctx, zkm):
    """A flagged call of 35 bytes, an unflagged one of 36 and a flagged one of 136 in one list; then the first call without its flag."""
    lists = TF.calls([35, 36, 136], flags=[1, 0, 1], seed=4)
    assert [int(m) >> 62 for m in lists[2][:, 2]] == [3, 2, 3]
    want = TM.expand(*lists).arrays()
    assert_outputs_equal(ctx.keccak_calls_witness(*lists), want)
    live = ctx.memory()[0]
    bare = lists[2].copy()
    bare[0, 2] &= ~TAIL
    with pytest.raises(zkm.ZkmError, match=r"zkm_keccak_calls_counts: input_off: call 0: length 35 is not a positive multiple of 4"):
        ctx.keccak_calls_witness(lists[0], lists[1], bare, lists[3])
    out = ctx.alloc(8)
    try:
        with pytest.raises(zkm.ZkmError, match=r"zkm_keccak_calls_witness: input_off: call 0: length 35 is not a positive multiple of 4"):
            ctx.keccak_calls_witness_into((lists[0], lists[1], bare, lists[3]), 3, out.ptr, out.ptr, out.ptr, out.ptr, out.ptr)
    finally:
        out.free()
    assert ctx.memory()[0] == live
    assert_outputs_equal(ctx.keccak_calls_witness(*lists), want)


# ---------------------------------------------------------------- whole segments
@pytest.fixture(scope="module")
def judged(ctx, zkm):
    """The recorded segment with calls of 35, 135, 137 and 1 bytes, a plain segment of another height, and the first once more,
    host-expanded from the model and proven by the step entry: computed once, shared, not to be changed."""
    segs = [TF.segment(zkm), TF.plain_segment(zkm), TF.segment(zkm)]
    assert segs[0]["log_n"] != segs[1]["log_n"] and segs[0]["log_n"] <= 10
    want = ctx.prove_segments_ops_steps([s["host"][0] for s in segs], [s["host"][1] for s in segs], public_values=PUBS)
    return segs, want


def calls_of(zkm, segs):
    return [zkm.SegmentCalls(**s["kw"]) for s in segs]


def test_composed_tables_equal_the_host_expanded_ones_and_every_check_holds(ctx, zkm, judged):
    segs = judged[0][:2]
    want = ctx.segments_tables_steps([s["host"][0] for s in segs], [s["host"][1] for s in segs])
    got = ctx.segments_tables_calls(calls_of(zkm, segs))
    try:
        for (st, lg), (wst, wlg) in zip(got, want):
            assert lg == wlg
            assert_tables_equal(tables_of(st, lg, ctx), tables_of(wst, wlg, ctx))
        for st, lg in got:
            verdict, _, _, report = ctx.segment_check(st.tables(), lg)      # the table constraints, the range lookups, the CTLs
            assert verdict == (0, 0) and ctx.check_message is None and report.kind == 0, ctx.check_message
    finally:
        for st, _ in got + want:
            st.free()


def test_proofs_equal_the_host_expanded_call_and_verify(ctx, zkm, judged):
    segs, want = judged
    got = ctx.prove_segments_ops_calls(calls_of(zkm, segs[:2]), public_values=PUBS[:2])
    assert_same_proofs(got, want[:2])
    reports = ctx.verify_segments([p for p, _, _ in got], PUBS[:2], [ch for _, ch, _ in got])
    assert [r.code for r in reports] == [0, 0], [r.message for r in reports]


def test_a_zero_extended_last_word_is_named_in_the_memory_table(ctx, zkm):
    """The host-expanded segment whose read rows hold the remaining bytes and zeros in the last word: the sponge's reads of the same
    address carry the padded word, so the Memory table cannot hold both.  A failing check, not a fault."""
    bad = TF.segment(zkm, "zero-extended")
    good = TF.segment(zkm)
    assert bad["kw"]["keccak"][0].tobytes() == good["kw"]["keccak"][0].tobytes()
    differ = np.argwhere(bad["host"][0].raw_rows != good["host"][0].raw_rows)
    assert len(differ) == len(TF.SEGMENT_LENGTHS)                           # one word a call: the last read channel's value
    (st, lg), = ctx.segments_tables_steps([bad["host"][0]], [bad["host"][1]])
    try:
        verdict = ctx.segment_check(st.tables(), lg)[0]
        assert verdict[0] != 0 and "Memory" in ctx.check_message, (verdict, ctx.check_message)
    finally:
        st.free()


def test_the_staged_entry_gives_the_same_proofs(ctx, zkm, judged):
    segs, want = judged
    live = ctx.memory()[0]
    with ctx.segments_calls_stage(calls_of(zkm, segs[:2])) as h:
        steps, ops, images = outputs(h)
        assert images is None
        assert_same_proofs(ctx.prove_segments_ops_steps(steps, ops, public_values=PUBS[:2]), want[:2])
    assert ctx.memory()[0] == live


def test_two_pool_workers_in_both_modes_give_the_one_context_proofs(ctx, zkm, judged):
    segs, want = judged
    one = ctx.prove_segments_ops_calls(calls_of(zkm, segs), public_values=PUBS)
    assert_same_proofs(one, want)
    pool = zkm.Pool((0,), 2)
    try:
        for mode in (0, 1):
            pool.set_tuning("pool_stage_ahead", mode)
            assert_same_proofs(pool.prove_segments_calls(calls_of(zkm, segs), public_values=PUBS, max_stack=2), one)
    finally:
        pool.close()
