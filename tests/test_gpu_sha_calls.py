"""GPU suite: SHA-256 precompile calls expanded on the device (zkm_sha_calls_witness, Context.sha_calls_expand).  The judge is
tests/sha_calls_model.py, itself held against the sponge fixtures and the oracle's CPU constraints on the CPU side: all five outputs of
the kernel equal the model word for word; whole segments built through sha_calls_expand equal, table by table and proof word by proof
word, the same entry points fed the model's host-expanded rows and lists; and check_ctls -- code that shares nothing with the model --
finds the fifteen lookups of those tables consistent.  Shapes: one call of either kind (one workgroup), 3 + 2 calls (five workgroups,
the offsets of both kinds in every list), the words that wrap every add, the highest addresses that fit."""
import numpy as np
import pytest

from . import boot_fixtures as BF
from . import cpu_fixtures as CF
from . import cpu_steps_model as M
from . import sha_calls_model as S
from .test_gpu_segment_ops import assert_tables_equal, tables_of

pytestmark = pytest.mark.gpu

NAMES = ("raw_rows", "memory_ops", "logic_ops", "sha_extend_inputs", "sha_extend_timestamps")
ONES = 0xFFFFFFFF


def u32(rng, *shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def calls(E, C, seed=1, ectx=(0, 0), hctx=(0, 0), wctx=None, top=False):
    """E extend and C compress calls on seeded random words, at disjoint addresses and clocks.  ectx / hctx / wctx: (context, segment) of
    w of an extend call, of hx, of a compress call's w (default: hx's); top: the highest addresses that fit."""
    rng = np.random.default_rng(seed)
    wctx = wctx or hctx
    emeta = np.array([(ectx[0], ectx[1], 0xFFFFFF03 if top else 0x10000 + 0x400 * e, 10 * (1 + 100 * e)) for e in range(E)], dtype=np.uint64).reshape(-1, 4)
    cmeta = np.array([(hctx[0], hctx[1], 0xFFFFFFE3 if top else 0x20000 + 0x400 * c, 10 * (9 + 100 * E + 20 * c), 0xFFFFFEFF if top else 0x30000 + 0x400 * c,
                       wctx[1], wctx[0], 0) for c in range(C)], dtype=np.uint64).reshape(-1, 8)
    return ((u32(rng, E, 16), emeta) if E else None), ((u32(rng, C, 8), u32(rng, C, 64), cmeta) if C else None)


def filled(lists, value):
    """The same calls with every data word `value`."""
    return tuple(None if grp is None else tuple(np.full_like(a, value) for a in grp[:-1]) + (grp[-1],) for grp in lists)


def assert_outputs_equal(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, "%s: first differing word at %s: %d, expected %d" % (name, bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


CASES = {
    "1-0": lambda: calls(1, 0),
    "0-1": lambda: calls(0, 1),
    "3-2": lambda: calls(3, 2, seed=2),
    "w16-ones": lambda: filled(calls(1, 0), ONES),
    "w16-zeros": lambda: filled(calls(1, 0), 0),
    "hx-w-ones": lambda: filled(calls(0, 1), ONES),            # wraps every add of the rounds and of hx + state
    "context-segment": lambda: calls(1, 1, seed=3, ectx=(7, 2), hctx=(5, 1)),
    "w-context-segment": lambda: calls(0, 2, seed=4, hctx=(5, 1), wctx=(0xFFFFFFFF, 0xFFFFFFFE)),
    "highest-addresses": lambda: calls(1, 1, seed=5, top=True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_witness_equals_the_model(ctx, zkm, case):
    e, c = CASES[case]()
    want = S.expand(e, c).arrays()
    assert want[0].shape[0] == zkm.sha_calls_counts(len(e[1]) if e else 0, len(c[2]) if c else 0)[0]
    assert_outputs_equal(ctx.sha_calls_witness(e, c), want)


def test_lists_in_device_memory(ctx, zkm):
    e, c = calls(3, 2, seed=2)
    want = S.expand(e, c).arrays()
    from zkm_amd import _as_words
    dev = [ctx.alloc((a.nbytes + 7) // 8).upload(_as_words(a)) for a in e + c]
    rows, mem, logic, ext = zkm.sha_calls_counts(3, 2)
    outs = [ctx.alloc(n) for n in (rows * 259, mem * 6, (logic * 3 + 1) // 2, ext * 2, ext)]
    try:
        before = ctx.host_waits()
        ctx.sha_calls_witness_into(tuple(dev[:2]), tuple(dev[2:]), 3, 2, *[b.ptr for b in outs])
        assert ctx.host_waits() - before == 1                      # the call returns once the outputs are complete: one wait
        got = (outs[0].download().reshape(rows, 259), outs[1].download().reshape(mem, 6), outs[2].download().view(np.uint32)[:logic * 3].reshape(logic, 3),
               outs[3].download().view(np.uint8).reshape(ext, 16), outs[4].download())
        assert_outputs_equal(got, want)
    finally:
        for b in dev + outs:
            b.free()


def test_outputs_aimed_into_larger_blocks_leave_the_other_words_alone(ctx, zkm):
    """2 rows / 5 operations in front, the same behind: what the call writes equals the model, every other word keeps its pattern."""
    e, c = calls(1, 1, seed=6)
    want = S.expand(e, c).arrays()
    rows, mem, logic, ext = zkm.sha_calls_counts(1, 1)
    PAT = 0xA5A5A5A5A5A5A5A5
    # (words written, words in front) of each block, in uint64 words but for the logic operations (uint32) and the inputs (bytes)
    lead = (2 * 259, 5 * 6, 5 * 3, 5 * 16, 5)
    unit = (8, 8, 4, 1, 8)
    size = (rows * 259, mem * 6, logic * 3, ext * 16, ext)
    bufs = []
    for ld, u, sz in zip(lead, unit, size):
        words = ((2 * ld + sz) * u + 7) // 8
        bufs.append(ctx.alloc(words).upload(np.full(words, PAT, dtype=np.uint64)))
    try:
        ctx.sha_calls_witness_into(e, c, 1, 1, *[b.ptr + ld * u for b, ld, u in zip(bufs, lead, unit)])
        for name, b, ld, u, sz, w in zip(NAMES, bufs, lead, unit, size, want):
            flat = b.download().view({8: np.uint64, 4: np.uint32, 1: np.uint8}[u])
            assert (flat[ld:ld + sz] == w.reshape(-1)).all(), name
            rest = np.concatenate([flat[:ld], flat[ld + sz:]])
            assert (rest == np.full(1, PAT, dtype=np.uint64).view(rest.dtype)[0]).all(), name
    finally:
        for b in bufs:
            b.free()


def test_a_refused_call_leaves_the_context_usable(ctx, zkm):
    e, c = calls(1, 1, seed=7)
    live = ctx.memory()[0]
    bad = (e[0], e[1].copy())
    bad[1][0, 3] += 5
    with pytest.raises(zkm.ZkmError, match=r"zkm_sha_calls_witness: extend_meta: call 0: timestamp 15 is not a multiple of 10"):
        ctx.sha_calls_witness(bad, c)
    out = ctx.alloc(8)
    with pytest.raises(zkm.ZkmError, match=r"zkm_sha_calls_witness: memory_ops_out_dev: NULL with 1056 operations to write"):
        ctx.sha_calls_witness_into(e, c, 1, 1, out.ptr, None, out.ptr, out.ptr, out.ptr)
    out.free()
    assert ctx.memory()[0] == live
    assert_outputs_equal(ctx.sha_calls_witness(e, c), S.expand(e, c).arrays())


# ---------------------------------------------------------------- whole segments
def own_ops(seed, first_ts):
    """A few memory and logic operations of the caller's own, in front of the generated ones: addresses no row touches."""
    rng = np.random.default_rng(seed)
    mem = np.zeros((7, 6), dtype=np.uint64)
    mem[:, 1], mem[:, 2], mem[:, 3], mem[:, 4], mem[:, 5] = 2, rng.integers(0, 64, 7), first_ts + np.arange(7), rng.integers(0, 2, 7), rng.integers(0, 1 << 32, 7)
    logic = np.stack([rng.integers(0, 4, 5), rng.integers(0, 1 << 32, 5), rng.integers(0, 1 << 32, 5)], axis=1).astype(np.uint32)
    return mem, logic


def program_with_calls(m, seed=11):
    """The sample program, then a SYSCALL row and an extend call, a SYSCALL row and a compress call (of the schedule the extend call
    wrote), each spliced in at its clocks."""
    rng = np.random.default_rng(seed)
    CF.sample_program(m)
    rec = S.CallRecorder(m)
    w16 = [int(x) for x in rng.integers(0, 1 << 32, 16)]
    w = S.Expansion().extend(w16, (0, 0, 0x20000, 10))
    for kind in ("extend", "compress"):
        for reg, v in ((4, 0x20000), (5, 0x30000), (6, 0x40), (37, 0x40000000)):
            m.set_reg(reg, v)
        m.syscall("other")
        if kind == "extend":
            rec.sha_extend(0x20000, w16)
        else:
            rec.sha_compress(0x20000, 0x30000, [int(x) for x in rng.integers(0, 1 << 32, 8)], w)
        m.nop()
    return rec


def both_ways(ctx, zkm, m, rec, own, nboot=0, boot_mem=0):
    """(composed, host-expanded) as (CpuSteps, SegmentOps) pairs of a recorded Machine with calls, padded to a power of two: the device's
    expansion through sha_calls_expand, and the model's rows and lists in numpy arrays."""
    x = rec.finish()
    log_n = int(len(m.rows)).bit_length()
    m.pad((1 << log_n) - len(m.rows))
    mem, logic, arith = M.expected_lists(m, mem_from=boot_mem)      # what the Machine's own rows push: derived from the steps, not handed over
    omem, ologic = own if own is not None else (np.zeros((0, 6), dtype=np.uint64), np.zeros((0, 3), dtype=np.uint32))
    e, c = rec.lists()
    steps = m.cpu_steps(zkm)
    composed = ctx.sha_calls_expand(steps, first_clock=m.first_clock, extend=e, compress=c, memory_ops=omem, logic_ops=ologic)
    rows, xmem, xlogic, ext_in, ext_ts = x.arrays()
    records, clocks = S.steps(x, raw_base=steps.nraw)
    patched = steps.steps.copy()
    patched[clocks.astype(np.int64) - m.first_clock] = records
    host = (zkm.CpuSteps(patched, np.concatenate([steps.raw_rows.reshape(-1, 259), rows])),
            zkm.SegmentOps(None, np.concatenate([omem, xmem]), logic_ops=np.concatenate([ologic, xlogic]), sha_extend=(ext_in, ext_ts),
                           sha_extend_sponge=e, sha_compress=c, sha_compress_sponge=c))
    return composed, host, log_n


def free_composed(composed):
    composed[0].raw_rows.free()
    composed[1].free()


def plain_segment(zkm, log_n=8):
    m = M.Recorder()
    CF.sample_program(m)
    m.pad((1 << log_n) - len(m.rows))
    return m.cpu_steps(zkm), zkm.SegmentOps(None, None)


def test_two_segments_one_with_calls_equal_the_host_expanded_call_and_balance_every_lookup(ctx, zkm):
    m = M.Recorder()
    rec = program_with_calls(m)
    composed, host, log_n = both_ways(ctx, zkm, m, rec, own_ops(1, 10 << 9))
    assert log_n == 9 and composed[0].nraw == host[0].nraw
    plain = plain_segment(zkm)
    try:
        want = ctx.segments_tables_steps([host[0], plain[0]], [host[1], plain[1]])
        got = ctx.segments_tables_steps([composed[0], plain[0]], [composed[1], plain[1]])
        for (st, lg), (wst, wlg) in zip(got, want):
            assert lg == wlg
            assert_tables_equal(tables_of(st, lg, ctx), tables_of(wst, wlg, ctx))
        # the tables of the segment with calls hold what the calls made: 48 ShaExtend rows, one compression
        assert got[0][1][6] >= 6 and got[0][1][8] >= 7
        for st, _ in got + want:
            st.free()
    finally:
        free_composed(composed)
    # the lookups, judged by check_ctls: without the caller's own operations (nothing reads those), all fifteen balance
    m = M.Recorder()
    rec = program_with_calls(m)
    composed, _, _ = both_ways(ctx, zkm, m, rec, None)
    try:
        (st, lg), = ctx.segments_tables_steps([composed[0]], [composed[1]])
        report = ctx.segment_check_ctls(st, lg)
        assert report.kind == 0, report.message
        st.free()
    finally:
        free_composed(composed)


def test_behind_a_bootstrap_image_the_first_clock_is_nonzero(ctx, zkm, oracle):
    class BootRecorder(M.StepRecorder, BF.BootMachine):
        pass
    seg = BF.segment(oracle, "b")
    model = seg["model"]
    m = BootRecorder(model, raw_boot=False)
    nboot = len(model.cpu_rows)
    rec = program_with_calls(m)
    assert m.first_clock == nboot > 0
    composed, host, log_n = both_ways(ctx, zkm, m, rec, None, nboot=nboot, boot_mem=len(model.memory_ops))
    image = BF.boot_image(zkm, seg["image"])
    try:
        (wst, wlg), = ctx.segments_tables_steps([host[0]], [host[1]], images=[image])
        (st, lg), = ctx.segments_tables_steps([composed[0]], [composed[1]], images=[image])
        assert lg == wlg and lg[1] == log_n
        assert_tables_equal(tables_of(st, lg, ctx), tables_of(wst, wlg, ctx))
        report = ctx.segment_check_ctls(st, lg)
        assert report.kind == 0, report.message
        st.free()
        wst.free()
    finally:
        free_composed(composed)


def test_proofs_equal_the_host_expanded_call(ctx, zkm):
    m = M.Recorder()
    rec = program_with_calls(m)
    composed, host, _ = both_ways(ctx, zkm, m, rec, None)
    pubs = [[1, 2, 3]]
    ctx.set_tuning("check_ctls", 1)
    ctx.set_tuning("verify", 1)
    try:
        want = ctx.prove_segments_ops_steps([host[0]], [host[1]], public_values=pubs)
        got = ctx.prove_segments_ops_steps([composed[0]], [composed[1]], public_values=pubs, sizes=[want[0][2]])
    finally:
        ctx.set_tuning("check_ctls", 0)
        ctx.set_tuning("verify", 0)
        free_composed(composed)
    (p, ch, o), (wp, wch, wo) = got[0], want[0]
    assert o == wo and (ch == wch).all()
    bad = np.nonzero(p != wp)[0]
    assert bad.size == 0, "first differing proof word %d" % bad[0]
