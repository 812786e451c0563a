"""GPU suite: byte-addressed sponge operations (ZKM_SPONGE_BYTE_ADDRESSED) and SYSKECCAK precompile calls expanded on the device
(zkm_keccak_calls_witness, Context.calls_expand).  The sponge writers are held to the oracle's tables with only the address columns
rewritten.  The judge of the expansion is tests/keccak_calls_model.py, itself held against the Keccak-f vectors, the oracle's sponge
table and the oracle's CPU constraints on the CPU side: all five outputs of the kernel equal the model word for word; whole segments
built through calls_expand equal, table by table and proof word by proof word, the same entry points fed the model's host-expanded rows
and lists; and check_ctls -- code that shares nothing with the model -- finds the fifteen lookups of those tables consistent.  Lengths:
every one at which the rows, the blocks or the padding take another shape (4, 32, 36, 132, 136, 140, 272), and three calls of different
lengths in one launch."""
import numpy as np
import pytest

from zkm_amd import tables as T

from . import boot_fixtures as BF
from . import cpu_fixtures as CF
from . import cpu_steps_model as M
from . import keccak_calls_model as K
from . import sha_calls_model as S
from .test_gpu_segment_ops import assert_tables_equal, tables_of

pytestmark = pytest.mark.gpu

NAMES = ("raw_rows", "memory_ops", "logic_ops", "keccak_inputs", "keccak_timestamps")
FLAG = np.uint64(K.FLAG)


# ---------------------------------------------------------------- the sponge writers and the flag
def sponge_ops(seed=7):
    """Five operations of 1 .. 300 bytes (one, two and three rows; lengths that are no multiple of 4), unflagged."""
    rng = np.random.default_rng(seed)
    lens = [1, 34, 136, 200, 300]
    off = np.cumsum([0] + lens).astype(np.uint64)
    data = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    meta = np.array([(0, 3, 0x1000 * (k + 1), 10 * (k + 1)) for k in range(len(lens))], dtype=np.uint64)
    return data, off, meta, lens


def rewritten(table, width, log_n, virt0, nvirt, block, off, meta, flagged):
    """The oracle's table with the address columns of the flagged operations rewritten from virt_base + w to virt_base + 4 w."""
    cols = table.reshape(width, 1 << log_n).copy()
    r = 0
    for k in range(len(meta)):
        L = int(off[k + 1] - off[k])
        for b in range(L // block + 1):
            for i in range(nvirt):
                w = nvirt * b + i
                if w < (L + 3) // 4 and flagged[k]:
                    assert cols[virt0 + i, r] == int(meta[k, 2]) + w
                    cols[virt0 + i, r] = int(meta[k, 2]) + 4 * w
            r += 1
    return cols.reshape(-1)


@pytest.mark.parametrize("flagged", [(1, 1, 1, 1, 1), (0, 0, 0, 0, 0), (1, 0, 1, 0, 1)], ids=["flagged", "unflagged", "mixed"])
def test_both_sponge_writers_read_the_flag_per_operation(ctx, oracle, flagged):
    data, off, meta, lens = sponge_ops()
    sent = meta.copy()
    sent[:, 2] |= np.array(flagged, dtype=np.uint64) * FLAG
    log_n = 4
    want, used = oracle.keccak_sponge_trace(data, off, meta.reshape(-1), log_n)
    buf, gused = ctx.keccak_sponge_trace(data, off, sent.reshape(-1), log_n)
    got = buf.download()
    buf.free()
    want = rewritten(want, 470, log_n, T.KS_VIRT, 34, 136, off, meta, flagged)
    assert gused == used and (got == want).all()
    if not any(flagged):
        assert (got == oracle.keccak_sponge_trace(data, off, meta.reshape(-1), log_n)[0]).all()      # exactly the oracle's table
    log_n = 6
    want, used = oracle.poseidon_sponge_trace(data, off, meta.reshape(-1), log_n)
    buf, gused = ctx.poseidon_sponge_trace(data, off, sent.reshape(-1), log_n)
    got = buf.download()
    buf.free()
    want = rewritten(want, 110, log_n, 3, 8, 32, off, meta, flagged)
    assert gused == used and (got == want).all()


# ---------------------------------------------------------------- the kernel's outputs against the model
def calls(lengths, seed=1, fill=None, ctx_seg=(0, 0), top=False):
    """One call per length on seeded bytes (or all `fill`), at disjoint addresses and clocks; top: the highest addresses that fit."""
    rng = np.random.default_rng(seed)
    out = []
    for k, L in enumerate(lengths):
        data = bytes([fill] * L) if fill is not None else rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        base = 0x100000000 - L if top else 0x10000 + 0x1000 * k
        out.append((data, (ctx_seg[0], ctx_seg[1], base | K.FLAG, 10 * (40 + 50 * k)), 0xFFFFFFE3 if top else 0x80000 + 0x40 * k))
    return K.lists(out)


def assert_outputs_equal(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, "%s: first differing word at %s: %d, expected %d" % (name, bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


CASES = {
    "L4": lambda: calls([4]),                                  # one word, one row, mask 0x01
    "L32": lambda: calls([32]),                                # exactly one full read row
    "L36": lambda: calls([36]),                                # a second row with one channel
    "L132": lambda: calls([132]),                              # both padding bytes in the unread last word
    "L136": lambda: calls([136]),                              # an empty final block: the sponge row's address 0, a block of pure padding
    "L140": lambda: calls([140]),
    "L272": lambda: calls([272]),
    "4-140-36": lambda: calls([4, 140, 36], seed=2),           # every prefix offset
    "ones": lambda: calls([140], fill=0xFF),
    "zeros": lambda: calls([140], fill=0),
    "context-segment": lambda: calls([36, 136], seed=3, ctx_seg=(7, 2)),
    "highest-addresses": lambda: calls([72], seed=5, ctx_seg=(0xFFFFFFFF, 0xFFFFFFFF), top=True),
}
_WANT = {}


def model(case):
    if case not in _WANT:
        lists = CASES[case]()
        _WANT[case] = (lists, K.expand(*lists).arrays())
    return _WANT[case]


@pytest.mark.parametrize("case", list(CASES))
def test_witness_equals_the_model(ctx, zkm, case):
    lists, want = model(case)
    assert (want[0].shape[0], want[1].shape[0], want[2].shape[0], want[3].shape[0]) == zkm.keccak_calls_counts(lists[1])
    assert_outputs_equal(ctx.keccak_calls_witness(*lists), want)


def test_lists_in_device_memory_and_a_nonzero_first_offset(ctx, zkm):
    (inputs, off, meta, daddrs), want = model("4-140-36")
    from zkm_amd import _as_words
    lead = 13                                                      # the calls' bytes begin in the middle of the caller's list, unaligned
    shifted = np.concatenate([np.full(lead, 0xEE, dtype=np.uint8), inputs])
    rows, mem, logic, perms = zkm.keccak_calls_counts(off + lead)
    outs = [ctx.alloc(n) for n in (rows * 259, mem * 6, (logic * 3 + 1) // 2, perms * 25, perms)]
    dev = [ctx.alloc((a.nbytes + 7) // 8).upload(_as_words(a)) for a in (shifted, meta, daddrs)]

    def download():
        return (outs[0].download().reshape(rows, 259), outs[1].download().reshape(mem, 6), outs[2].download().view(np.uint32)[:logic * 3].reshape(logic, 3),
                outs[3].download().reshape(perms, 25), outs[4].download())
    try:
        before = ctx.host_waits()
        ctx.keccak_calls_witness_into((dev[0], off + lead, dev[1], dev[2]), 3, *[b.ptr for b in outs])
        assert ctx.host_waits() - before == 1                      # the call returns once the outputs are complete: one wait
        assert_outputs_equal(download(), want)
        for b in outs:
            b.upload(np.zeros(b.words, dtype=np.uint64))
        ctx.keccak_calls_witness_into((shifted, off + lead, meta, daddrs), 3, *[b.ptr for b in outs])      # the same from host memory
        assert_outputs_equal(download(), want)
    finally:
        for b in dev + outs:
            b.free()


def test_outputs_aimed_into_larger_blocks_leave_the_other_words_alone(ctx, zkm):
    lists, want = model("4-140-36")
    rows, mem, logic, perms = zkm.keccak_calls_counts(lists[1])
    PAT = 0xA5A5A5A5A5A5A5A5
    lead = (2 * 259, 5 * 6, 5 * 3, 5 * 25, 5)                      # words in front of (and behind) what the call writes
    unit = (8, 8, 4, 8, 8)
    size = (rows * 259, mem * 6, logic * 3, perms * 25, perms)
    bufs = []
    for ld, u, sz in zip(lead, unit, size):
        words = ((2 * ld + sz) * u + 7) // 8
        bufs.append(ctx.alloc(words).upload(np.full(words, PAT, dtype=np.uint64)))
    try:
        ctx.keccak_calls_witness_into(lists, 3, *[b.ptr + ld * u for b, ld, u in zip(bufs, lead, unit)])
        for name, b, ld, u, sz, w in zip(NAMES, bufs, lead, unit, size, want):
            flat = b.download().view({8: np.uint64, 4: np.uint32}[u])
            assert (flat[ld:ld + sz] == w.reshape(-1)).all(), name
            rest = np.concatenate([flat[:ld], flat[ld + sz:]])
            assert (rest == np.full(1, PAT, dtype=np.uint64).view(rest.dtype)[0]).all(), name
    finally:
        for b in bufs:
            b.free()


def test_a_refused_call_leaves_the_context_usable(ctx, zkm):
    lists, want = model("L36")
    live = ctx.memory()[0]
    bad = lists[2].copy()
    bad[0, 2] &= ~FLAG
    with pytest.raises(zkm.ZkmError, match=r"zkm_keccak_calls_witness: meta: call 0: virt_base 0x10000 lacks ZKM_SPONGE_BYTE_ADDRESSED"):
        ctx.keccak_calls_witness(lists[0], lists[1], bad, lists[3])
    with pytest.raises(zkm.ZkmError, match=r"zkm_keccak_calls_counts: input_off: call 0: length 35 is not a positive multiple of 4"):
        ctx.keccak_calls_witness(lists[0][:35], np.array([0, 35], dtype=np.uint64), lists[2], lists[3])
    out = ctx.alloc(8)
    with pytest.raises(zkm.ZkmError, match=r"zkm_keccak_calls_witness: memory_ops_out_dev: NULL with 36 operations to write"):
        ctx.keccak_calls_witness_into(lists, 1, out.ptr, None, out.ptr, out.ptr, out.ptr)
    dev_off = ctx.alloc(2).upload(lists[1])
    with pytest.raises(zkm.ZkmError, match=r"zkm_keccak_calls_witness: input_off: device memory"):
        ctx.keccak_calls_witness_into((lists[0], dev_off, lists[2], lists[3]), 1, out.ptr, out.ptr, out.ptr, out.ptr, out.ptr)
    dev_off.free()
    out.free()
    assert ctx.memory()[0] == live
    assert_outputs_equal(ctx.keccak_calls_witness(*lists), want)


# ---------------------------------------------------------------- whole segments
def program_with_calls(m, lengths=(140, 36), sha=False, seed=11):
    """The sample program, then a SYSCALL row and a Keccak call per length (and, with sha, one extend and one compress call), each
    spliced in at its clocks."""
    rng = np.random.default_rng(seed)
    CF.sample_program(m)
    rec = K.CallRecorder(m)
    for k, L in enumerate(lengths):
        addr, ptr = 0x50000 + 0x1000 * k, 0x60000 + 0x40 * k
        for reg, v in ((4, addr), (5, L), (6, ptr), (37, 0x40000000)):
            m.set_reg(reg, v)
        m.syscall("other")
        rec.keccak(addr, rng.integers(0, 256, L, dtype=np.uint8).tobytes(), ptr)
        m.nop()
    if sha:
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


def both_ways(ctx, zkm, m, rec):
    """(composed, host-expanded) as (CpuSteps, SegmentOps) pairs of a recorded Machine with calls, padded to a power of two: the device's
    expansion through calls_expand, and the models' rows and lists in numpy arrays."""
    sx, kx = rec.finish()
    log_n = int(len(m.rows)).bit_length()
    m.pad((1 << log_n) - len(m.rows))
    e, c = rec.lists()
    k = rec.keccak_lists()
    steps = m.cpu_steps(zkm)
    composed = ctx.calls_expand(steps, first_clock=m.first_clock, extend=e, compress=c, keccak=k)
    srows, smem, slogic, ext_in, ext_ts = sx.arrays()
    krows, kmem, klogic, perm_in, perm_ts = kx.arrays()
    patched = steps.steps.copy()
    for x, base in ((sx, steps.nraw), (kx, steps.nraw + len(srows))):
        if x.rows:
            records, clocks = (S if x is sx else K).steps(x, raw_base=base)
            patched[clocks.astype(np.int64) - m.first_clock] = records
    host = (zkm.CpuSteps(patched, np.concatenate([steps.raw_rows.reshape(-1, 259), srows, krows])),
            zkm.SegmentOps(None, np.concatenate([smem, kmem]), logic_ops=np.concatenate([slogic, klogic]),
                           sha_extend=(ext_in, ext_ts) if len(ext_ts) else None, sha_extend_sponge=e, sha_compress=c, sha_compress_sponge=c,
                           keccak=(perm_in, perm_ts), keccak_sponge=k[:3]))
    return composed, host, log_n


def free_composed(composed):
    composed[0].raw_rows.free()
    composed[1].free()


def plain_segment(zkm, log_n=8):
    m = M.Recorder()
    CF.sample_program(m)
    m.pad((1 << log_n) - len(m.rows))
    return m.cpu_steps(zkm), zkm.SegmentOps(None, None)


def test_two_segments_of_different_heights_equal_the_host_expanded_call_and_balance_every_lookup(ctx, zkm):
    m = M.Recorder()
    rec = program_with_calls(m, lengths=(140, 36, 272))
    composed, host, log_n = both_ways(ctx, zkm, m, rec)
    assert log_n == 9 and composed[0].nraw == host[0].nraw
    plain = plain_segment(zkm)
    try:
        want = ctx.segments_tables_steps([host[0], plain[0]], [host[1], plain[1]])
        got = ctx.segments_tables_steps([composed[0], plain[0]], [composed[1], plain[1]])
        for (st, lg), (wst, wlg) in zip(got, want):
            assert lg == wlg
            assert_tables_equal(tables_of(st, lg, ctx), tables_of(wst, wlg, ctx))
        report = ctx.segment_check_ctls(*got[0])
        assert report.kind == 0, report.message
        for st, _ in got + want:
            st.free()
    finally:
        free_composed(composed)


def test_together_with_one_sha_extend_and_one_compress_call(ctx, zkm):
    m = M.Recorder()
    rec = program_with_calls(m, lengths=(136, 4), sha=True)
    composed, host, log_n = both_ways(ctx, zkm, m, rec)
    try:
        (wst, wlg), = ctx.segments_tables_steps([host[0]], [host[1]])
        (st, lg), = ctx.segments_tables_steps([composed[0]], [composed[1]])
        assert lg == wlg and log_n <= 10
        assert_tables_equal(tables_of(st, lg, ctx), tables_of(wst, wlg, ctx))
        report = ctx.segment_check_ctls(st, lg)
        assert report.kind == 0, report.message
        st.free()
        wst.free()
    finally:
        free_composed(composed)


def test_behind_a_bootstrap_image_the_first_clock_is_nonzero(ctx, zkm, oracle):
    class BootRecorder(M.StepRecorder, BF.BootMachine):
        pass
    seg = BF.segment(oracle, "b")
    model_ = seg["model"]
    m = BootRecorder(model_, raw_boot=False)
    nboot = len(model_.cpu_rows)
    rec = program_with_calls(m)
    assert m.first_clock == nboot > 0
    composed, host, log_n = both_ways(ctx, zkm, m, rec)
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
    composed, host, _ = both_ways(ctx, zkm, m, rec)
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
