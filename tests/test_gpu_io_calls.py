"""GPU suite: the I/O syscalls' rows expanded on the device (zkm_io_calls_witness, Context.calls_expand(io=...)).  The judge is
tests/io_calls_model.py, itself held against hand-computed rows and the oracle's CPU constraints on the CPU side: raw_rows equals the
model word for word; whole segments built through calls_expand equal, table by table and proof word by proof word, the same entry points
fed the model's host-expanded rows; and check_ctls -- code that shares nothing with the model -- finds the fifteen lookups of those tables
consistent.  Lengths: every one at which the rows, the last word or the preimage's closing bit take another shape, and one call of 257
rows, more than any workgroup's span."""
import numpy as np
import pytest

from . import cpu_steps_model as M
from . import io_calls_model as IO
from . import sha_calls_model as S
from .test_gpu_segment_ops import assert_tables_equal, tables_of

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 3, 4, 5, 32, 33, 36, 64, 68)
CONTENTS = (0, 1, 3, 4, 27, 28, 29, 31, 32, 35, 61)     # both sides of `% 32 + 4 > 32` and of the eight-word row, counting the length word
MAP = IO.PREIMAGE_MAP
H, CM, V, P = IO.HINT_READ, IO.COMMIT, IO.VERIFY, IO.PREIMAGE


def call(kind, L, k=0, seed=1, fill=None, ctx_seg=(0, 0), addr=None):
    """One call of `kind` on L seeded bytes (or all `fill`), at an address and a clock of its own."""
    data = bytes([fill] * L) if fill is not None else np.random.default_rng(1000 * seed + 10 * L + kind).integers(0, 256, L, dtype=np.uint8).tobytes()
    addr = addr if addr is not None else MAP if kind == P else 0x10000 + 0x1000 * k
    return kind, data, (ctx_seg[0], ctx_seg[1], addr, 10 * (40 + 50 * k))


def each_kind(L, **kw):
    """A call of each kind for the length L of the issue's list: the hint read L itself, the commit its whole words, the verify its 32
    bytes, the preimage L content bytes."""
    return [call(H, L, 0, **kw), call(CM, (L + 3) // 4 * 4, 1, **kw), call(V, 32, 2, **kw), call(P, 32 + L, 3, **kw)]


def top(kind, L):
    """The highest addresses that fit (a preimage's are fixed), the largest context and segment."""
    W = {H: (L + 3) // 4, CM: L // 4, V: 8}[kind]
    return call(kind, L, seed=5, ctx_seg=(0xFFFFFFFF, 0xFFFFFFFF), addr=0x100000000 - 4 * max(W, 1))


CASES = {"L%d" % L: (lambda L=L: each_kind(L)) for L in LENGTHS}
CASES.update({"C%d" % c: (lambda c=c: [call(P, 32 + c, seed=2)]) for c in CONTENTS})
CASES.update({
    "four-kinds": lambda: [call(H, 37, 0, seed=3), call(CM, 36, 1, seed=3), call(V, 32, 2, seed=3), call(P, 32 + 29, 3, seed=3)],
    "257-rows": lambda: [call(CM, 8, 0, seed=4), call(H, 8196, 1, seed=4), call(V, 32, 2, seed=4)],    # a long call between two of one row
    "ones": lambda: each_kind(37, fill=0xFF) + [call(P, 32 + 29, 4, fill=0xFF)],
    "zeros": lambda: each_kind(37, fill=0) + [call(P, 32 + 31, 4, fill=0)],
    "context-segment": lambda: each_kind(33, seed=6, ctx_seg=(7, 2)),
    "highest-addresses": lambda: [top(H, 37), top(CM, 36), top(V, 32), top(H, 0), call(P, 32 + 5, seed=5, ctx_seg=(0xFFFFFFFF, 0xFFFFFFFF))],
})
_WANT = {}


def model(case):
    if case not in _WANT:
        lists = IO.lists(CASES[case]())
        x = IO.expand(*lists)
        _WANT[case] = (lists, x.array(), x)
    return _WANT[case]


def assert_rows_equal(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "raw_rows: first differing word at %s: %d, expected %d" % (bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("case", list(CASES))
def test_witness_equals_the_model(ctx, zkm, case):
    lists, want, x = model(case)
    assert (want.shape[0], x.memory_ops()) == zkm.io_calls_counts(lists[0], lists[2])
    if case == "257-rows":
        assert want.shape[0] == 1 + 257 + 1
    assert_rows_equal(ctx.io_calls_witness(*lists), want)


def test_lists_in_device_memory_and_a_nonzero_first_offset(ctx, zkm):
    (kinds, data, off, meta), want, _ = model("four-kinds")
    from zkm_amd import _as_words
    lead = 13                                                      # the calls' bytes begin in the middle of the caller's list, unaligned
    shifted = np.concatenate([np.full(lead, 0xEE, dtype=np.uint8), data])
    rows = zkm.io_calls_counts(kinds, off + lead)[0]
    out = ctx.alloc(rows * 259)
    dev = [ctx.alloc((a.nbytes + 7) // 8).upload(_as_words(a)) for a in (shifted, meta)]
    try:
        before = ctx.host_waits()
        ctx.io_calls_witness_into((kinds, dev[0], off + lead, dev[1]), 4, out.ptr)
        assert ctx.host_waits() - before == 1                      # the call returns once the rows are complete: one wait
        assert_rows_equal(out.download().reshape(rows, 259), want)
        out.upload(np.full(out.words, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64))   # (the kernel writes every word: no zero-fill in front)
        ctx.io_calls_witness_into((kinds, shifted, off + lead, meta), 4, out.ptr)      # the same from host memory
        assert_rows_equal(out.download().reshape(rows, 259), want)
        assert_rows_equal(ctx.io_calls_witness(kinds, dev[0], off + lead, dev[1]), want)
    finally:
        for b in dev + [out]:
            b.free()


def test_an_output_aimed_into_a_larger_block_leaves_the_other_words_alone(ctx, zkm):
    (lists, want, _) = model("257-rows")
    rows = want.shape[0]
    PAT = 0xA5A5A5A5A5A5A5A5
    for lead in (2 * 259, 3 * 259 + 1):                            # rows in front; and a start that is 8- but not 16-byte aligned
        buf = ctx.alloc(2 * lead + rows * 259).upload(np.full(2 * lead + rows * 259, PAT, dtype=np.uint64))
        try:
            ctx.io_calls_witness_into(lists, len(lists[0]), buf.ptr + 8 * lead)
            flat = buf.download()
            assert_rows_equal(flat[lead:lead + rows * 259].reshape(rows, 259), want)
            assert (flat[:lead] == PAT).all() and (flat[lead + rows * 259:] == PAT).all()
        finally:
            buf.free()


def test_a_refused_call_leaves_the_context_usable(ctx, zkm):
    (kinds, data, off, meta), want, _ = model("four-kinds")
    live = ctx.memory()[0]
    bad = meta.copy()
    bad[1, 2] += 2
    with pytest.raises(zkm.ZkmError, match=r"zkm_io_calls_witness: meta: call 1: address 0x11002 is not aligned to 4 bytes"):
        ctx.io_calls_witness(kinds, data, off, bad)
    with pytest.raises(zkm.ZkmError, match=r"zkm_io_calls_counts: kinds: call 2: unknown kind 9"):
        ctx.io_calls_witness(np.array([H, CM, 9, P], dtype=np.uint32), data, off, meta)
    with pytest.raises(zkm.ZkmError, match=r"zkm_io_calls_witness: raw_rows_out_dev: NULL with 8 rows to write"):
        ctx.io_calls_witness_into((kinds, data, off, meta), 4, None)
    dev = ctx.alloc(8).upload(off)
    with pytest.raises(zkm.ZkmError, match=r"zkm_io_calls_witness: data_off: device memory"):
        ctx.io_calls_witness_into((kinds, data, dev, meta), 4, dev.ptr)
    with pytest.raises(zkm.ZkmError, match=r"zkm_io_calls_witness: kinds: device memory"):
        ctx.io_calls_witness_into((dev, data, off, meta), 4, dev.ptr)
    dev.free()
    assert ctx.memory()[0] == live
    assert_rows_equal(ctx.io_calls_witness(kinds, data, off, meta), want)


# ---------------------------------------------------------------- whole segments
def program_with_calls(m, others=False, seed=11):
    """The Recorder's bootstrap, then one I/O call of each kind behind a SYSCALL row with its argument registers loaded (and, with
    others, one Keccak and one SHA compress call), each spliced in at its clocks.  The hint read comes first and the commit reads what
    it wrote.  (The sample program alone is 252 rows and the same both ways: without it every segment here fits a 2^8-row CPU table.)"""
    rng = np.random.default_rng(seed)
    rec = IO.CallRecorder(m)
    vec = rng.integers(0, 256, 37, dtype=np.uint8).tobytes()
    for kind, addr, data in (("hint_read", 0x50000, vec), ("commit", 0x50000, vec[:36]), ("verify", 0x51000, rng.integers(0, 256, 32, dtype=np.uint8).tobytes()),
                             ("preimage", MAP, rng.integers(0, 256, 32 + 61, dtype=np.uint8).tobytes())):
        for reg, v in ((4, addr), (5, len(data)), (6, 0x30000), (37, 0x40000000)):
            m.set_reg(reg, v)
        m.syscall("other")
        rec.io(kind, addr, data)
        m.nop()
    if others:
        for reg, v in ((4, 0x52000), (5, 140), (6, 0x60000), (37, 0x40000000)):
            m.set_reg(reg, v)
        m.syscall("other")
        rec.keccak(0x52000, rng.integers(0, 256, 140, dtype=np.uint8).tobytes(), 0x60000)
        m.nop()
        w = S.Expansion().extend([int(x) for x in rng.integers(0, 1 << 32, 16)], (0, 0, 0x20000, 10))
        for reg, v in ((4, 0x20000), (5, 0x30000), (6, 0x40), (37, 0x40000000)):
            m.set_reg(reg, v)
        m.syscall("other")
        rec.sha_compress(0x20000, 0x30000, [int(x) for x in rng.integers(0, 1 << 32, 8)], w)
        m.nop()
    return rec


def both_ways(ctx, zkm, m, rec):
    """(composed, host-expanded) as (CpuSteps, SegmentOps) pairs of a recorded Machine with calls, padded to a power of two: the device's
    expansion through calls_expand, and the models' rows and lists in numpy arrays."""
    from . import keccak_calls_model as K
    sx, kx, ix = rec.finish()
    log_n = int(len(m.rows)).bit_length()
    m.pad((1 << log_n) - len(m.rows))
    e, c = rec.lists()
    k = rec.keccak_lists()
    steps = m.cpu_steps(zkm)
    composed = ctx.calls_expand(steps, first_clock=m.first_clock, extend=e, compress=c, keccak=k, io=rec.io_lists())
    srows, smem, slogic, ext_in, ext_ts = sx.arrays()
    if kx.rows:
        krows, kmem, klogic, perm_in, perm_ts = kx.arrays()
    else:
        krows, kmem, klogic = np.zeros((0, 259), dtype=np.uint64), np.zeros((0, 6), dtype=np.uint64), np.zeros((0, 3), dtype=np.uint32)
    irows = ix.array()
    patched = steps.steps.copy()
    base = steps.nraw
    for x, mod in ((sx, S), (kx, K), (ix, IO)):
        if x.rows:
            records, clocks = mod.steps(x, raw_base=base)
            patched[clocks.astype(np.int64) - m.first_clock] = records
        base += len(x.rows)
    host = (zkm.CpuSteps(patched, np.concatenate([steps.raw_rows.reshape(-1, 259), srows, krows, irows])),
            zkm.SegmentOps(None, np.concatenate([smem, kmem]) if len(smem) + len(kmem) else None,
                           logic_ops=np.concatenate([slogic, klogic]) if len(slogic) + len(klogic) else None,
                           sha_extend=(ext_in, ext_ts) if len(ext_ts) else None, sha_extend_sponge=e, sha_compress=c, sha_compress_sponge=c,
                           keccak=(perm_in, perm_ts) if kx.rows else None, keccak_sponge=k[:3] if k else None))
    return composed, host, log_n


def free_composed(composed):
    composed[0].raw_rows.free()
    composed[1].free()


@pytest.mark.parametrize("others", [False, True], ids=["io-alone", "with-keccak-and-sha"])
def test_a_segment_equals_the_host_expanded_call_and_balances_every_lookup(ctx, zkm, others):
    m = M.Recorder()
    rec = program_with_calls(m, others=others)
    composed, host, log_n = both_ways(ctx, zkm, m, rec)
    assert composed[0].nraw == host[0].nraw and log_n <= 8
    assert composed[0].steps.tobytes() == host[0].steps.tobytes()
    try:
        (wst, wlg), = ctx.segments_tables_steps([host[0]], [host[1]])
        (st, lg), = ctx.segments_tables_steps([composed[0]], [composed[1]])
        assert lg == wlg
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
