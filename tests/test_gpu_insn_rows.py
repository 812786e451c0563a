"""GPU suite: the rows of the thirteen instructions no step kind takes, expanded on the device (zkm_insn_rows_witness,
Context.calls_expand(insns=...)).  The judge is tests/insn_rows_model.py, itself held against hand-computed rows, the oracle's CPU
constraints and the lookup model on the CPU side: raw_rows and the arithmetic list equal the model word for word; a whole segment built
through calls_expand equals, table by table and proof word by proof word, the same entry points fed the model's host-expanded RAW rows
and a host arithmetic list; and the device's witness, lookup and cross-table checks -- code that shares nothing with the model -- hold on
its tables.  Record counts: every one at which a workgroup's span (ROWS_PER_WG rows) ends or a second and third workgroup begin."""
import numpy as np
import pytest

from . import cpu_steps_model as M
from . import insn_rows_model as I
from . import lookup_model as LM
from .test_gpu_segment_ops import assert_tables_equal, tables_of

pytestmark = pytest.mark.gpu

R = I.ROWS_PER_WG
EDGES = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
REGS = {8: 0xFFFFFFF9, 9: 2, 10: 0x80000000, 11: 0x7FFFFFFF, 22: 0x10C, I.REG_LO: 5, I.REG_HI: 6}


def recorder(**kw):
    m = I.InsnRecorder()
    for reg, v in REGS.items():
        m.set_reg(reg, v)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


ONE = {"LUI": lambda m: I.lui(m, 3, 17, 0x1234), "MUL": lambda m: I.binary(m, "MUL", 8, 9, 16, sa=5), "MULT": lambda m: I.hilo(m, "MULT", 8, 10, rd=3),
       "MULTU": lambda m: I.hilo(m, "MULTU", 8, 10), "DIV": lambda m: I.hilo(m, "DIV", 10, 8), "DIVU": lambda m: I.hilo(m, "DIVU", 10, 8, sa=1),
       "MFHI": lambda m: I.binary(m, "MFHI", rd=18, rs=4), "MTHI": lambda m: I.binary(m, "MTHI", rs=8, rt=2), "MFLO": lambda m: I.binary(m, "MFLO", rd=19),
       "MTLO": lambda m: I.binary(m, "MTLO", rs=9, rd=7), "SDC1": lambda m: I.sdc1(m, 22, 8, 0xFFF6), "SYNC": lambda m: I.nop_like(m, "SYNC", rs=1, sa=31),
       "PREF": lambda m: I.nop_like(m, "PREF", rs=22, rt=30, imm=0xFFFF)}
assert list(ONE) == list(I.KINDS)


def one(kind):
    m = recorder()
    ONE[kind](m)
    return m


def pairs(kind):
    """Every pair of the edge operands on both sides, minus the pairs the library refuses."""
    m = recorder()
    for a in EDGES:
        for b in EDGES:
            if kind in ("DIV", "DIVU") and (b == 0 or (kind == "DIV" and (a, b) == (0x80000000, 0xFFFFFFFF))):
                continue
            m.set_reg(8, a)
            m.set_reg(9, b)
            if kind == "MUL":
                I.binary(m, "MUL", 8, 9, 16)
            else:
                I.hilo(m, kind, 8, 9)
    assert len(m.insns) == {"DIV": 19, "DIVU": 20}.get(kind, 25)
    return m


def cycle(n, **kw):
    """n records cycling through pushing and non-pushing kinds with a period that is no divisor of a workgroup's span."""
    m = recorder(**kw)
    ops = [lambda: I.binary(m, "MUL", 8, 9, 16), lambda: I.nop_like(m, "SYNC"), lambda: I.lui(m, 0, 17, 0x9234), lambda: I.sdc1(m, 22, 8, 0xFFF4),
           lambda: I.hilo(m, "DIV", 8, 9), lambda: I.nop_like(m, "PREF", rs=22), lambda: I.binary(m, "MFHI", rd=18), lambda: I.hilo(m, "MULTU", 10, 8),
           lambda: I.sdc1(m, 22, 10, 0xFFFB), lambda: I.binary(m, "MTLO", rs=9), lambda: I.hilo(m, "MULT", 8, 10)]
    for k in range(n):
        ops[k % len(ops)]()
    assert len(m.insns) == n
    return m


def mix():
    """Runs of SYNC, PREF and SDC1 records between pushing ones: the workgroups' bases in the arithmetic list are 2, 2, 5 and 13, and
    one workgroup pushes nothing."""
    m = recorder()
    quiet = [lambda: I.nop_like(m, "SYNC"), lambda: I.nop_like(m, "PREF", imm=4), lambda: I.sdc1(m, 22, 9, 0xFFF9)]
    loud = [lambda: I.binary(m, "MUL", 8, 10, 16), lambda: I.lui(m, 0, 17, 0x8001), lambda: I.hilo(m, "DIVU", 8, 9), lambda: I.binary(m, "MFLO", rd=20)]
    pushing = {0, 15, 2 * R, 2 * R + 1, 2 * R + 15} | set(range(3 * R, 3 * R + 8, 1)) | {4 * R + 3}
    for k in range(4 * R + 5):
        (loud[k % 4] if k in pushing else quiet[k % 3])()
    flags = [x["arith"] is not None for x in m.insns]
    assert [sum(flags[:g * R]) for g in range(5)] == [0, 2, 2, 5, 13]
    return m


def lui_immediates():
    m = recorder()
    for imm in (0, 0x7FFF, 0x8000, 0xFFFF):
        I.lui(m, 0, 16, imm)
    I.lui(m, 21, 16, 0x8000)
    return m


def destination_0():
    m = recorder()
    I.binary(m, "MUL", 8, 9, 0)
    I.binary(m, "MFHI", rd=0)
    I.binary(m, "MFLO", rd=0)
    I.lui(m, 0, 0, 0xABCD)
    I.lui(m, 5, 0, 0xABCD)
    return m


def div_signs():
    m = recorder()
    for a, b in ((7, 2), (0xFFFFFFF9, 2), (7, 0xFFFFFFFE), (0xFFFFFFF9, 0xFFFFFFFE)):
        m.set_reg(8, a)
        m.set_reg(9, b)
        I.hilo(m, "DIV", 8, 9)
    return m


def sdc1_low_bits(**kw):
    m = recorder(**kw)
    for offset in (0xFFF4, 0xFFF5, 0xFFFA, 0xFFFF):
        I.sdc1(m, 22, 8, offset)
    return m


def last_clock():
    m = recorder()
    m.clock_offset = (1 << 32) - 1 - len(m.rows)
    I.binary(m, "MUL", 8, 9, 16)
    assert m.insns[0]["clock"] == (1 << 32) - 1
    return m


def both_kernel_flags():
    m = cycle(5, kernel=0)
    m.kernel = 1
    I.hilo(m, "MULT", 8, 10)
    assert [x["record"][4] for x in m.insns] == [0] * 5 + [1]
    return m


CASES = {"one-" + k: (lambda k=k: one(k)) for k in I.KINDS}
CASES.update({"pairs-" + k: (lambda k=k: pairs(k)) for k in ("MUL", "MULT", "MULTU", "DIV", "DIVU")})
CASES.update({"n%d" % n: (lambda n=n: cycle(n)) for n in (1, R - 1, R, R + 1, 2 * R + 3)})
CASES.update({"div-signs": div_signs, "lui-immediates": lui_immediates, "destination-0": destination_0, "sdc1-low-bits": sdc1_low_bits,
              "kernel-flag": both_kernel_flags, "context": lambda: cycle(R + 2, context=7), "sdc1-context": lambda: sdc1_low_bits(context=0xFFFFFFFF),
              "last-clock": last_clock, "mix": mix})
_WANT = {}


def model(case):
    """(records, clocks), the expected rows, the expected arithmetic list and the recorder of a case, built once."""
    if case not in _WANT:
        m = CASES[case]()
        _WANT[case] = (m.insn_lists(), m.insn_rows(), m.insn_arith(), m)
    return _WANT[case]


def assert_rows_equal(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "raw_rows: first differing word at %s: %d, expected %d" % (bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def assert_arith_equal(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "arithmetic_ops: first differing word at %s: %d, expected %d" % (bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("case", list(CASES))
def test_witness_equals_the_model(ctx, zkm, case):
    (records, clocks), want_rows, want_arith, m = model(case)
    assert zkm.insn_rows_counts(records) == (m.insn_memory_ops(), len(want_arith))
    rows, arith = ctx.insn_rows_witness(records, clocks)
    assert_rows_equal(rows, want_rows)
    assert_arith_equal(arith, want_arith)


def test_outputs_aimed_into_larger_blocks_leave_the_other_words_alone(ctx, zkm):
    (records, clocks), want_rows, want_arith, _ = model("mix")
    n, na = len(records), len(want_arith)
    PAT = 0xA5A5A5A5A5A5A5A5
    for lead, alead in ((2 * 259, 6), (3 * 259, 3)):               # rows in front; then a start that is 8- but not 16-byte aligned, and a
        assert (8 * lead) % 16 == (0 if lead == 2 * 259 else 8)    # list that is 4- but not 8-byte aligned
        buf = ctx.alloc(2 * lead + n * 259).upload(np.full(2 * lead + n * 259, PAT, dtype=np.uint64))
        ops = ctx.alloc(8 + (3 * na + 1) // 2).upload(np.full(8 + (3 * na + 1) // 2, PAT, dtype=np.uint64))
        try:
            before = ctx.host_waits()
            ctx.insn_rows_witness_into((records, clocks), n, buf.ptr + 8 * lead, ops.ptr + 4 * alead)
            assert ctx.host_waits() - before == 1                      # the call returns once both outputs are complete: one wait
            flat = buf.download()
            assert_rows_equal(flat[lead:lead + n * 259].reshape(n, 259), want_rows)
            assert (flat[:lead] == PAT).all() and (flat[lead + n * 259:] == PAT).all()
            words = ops.download().view(np.uint32)
            assert_arith_equal(words[alead:alead + 3 * na].reshape(na, 3), want_arith)
            assert (words[:alead] == 0xA5A5A5A5).all() and (words[alead + 3 * na:] == 0xA5A5A5A5).all()
        finally:
            buf.free()
            ops.free()


def test_a_refused_call_leaves_the_context_usable(ctx, zkm):
    (records, clocks), want_rows, want_arith, _ = model("n%d" % (R + 1))
    live = ctx.memory()[0]
    D = R - 1                                                          # record R - 1, the first workgroup's last, is a DIV
    bad = records.copy()
    bad["reads"][D, 1] = 0
    assert bad["kind"][D] == I.KIND["DIV"] and bad["kind"][3] == I.KIND["SDC1"]
    with pytest.raises(zkm.ZkmError, match=r"zkm_insn_rows_counts: record %d: DIV by zero" % D):
        ctx.insn_rows_witness(bad, clocks)
    out = ctx.alloc(len(records) * 259 + 64)
    try:
        out.upload(np.full(out.words, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64))
        waits = ctx.host_waits()
        with pytest.raises(zkm.ZkmError, match=r"zkm_insn_rows_witness: record %d: DIV by zero" % D):
            ctx.insn_rows_witness_into((bad, clocks), len(bad), out.ptr, out.ptr + 8 * len(records) * 259)
        bad = records.copy()
        bad["insn"][3] ^= 1 << 26
        with pytest.raises(zkm.ZkmError, match=r"zkm_insn_rows_witness: record 3: SDC1 does not take the encoding 0x"):
            ctx.insn_rows_witness_into((bad, clocks), len(bad), out.ptr, out.ptr + 8 * len(records) * 259)
        late = clocks.copy()
        late[1] = 1 << 32
        with pytest.raises(zkm.ZkmError, match=r"zkm_insn_rows_witness: record 1: clock 4294967296 does not fit in 32 bits"):
            ctx.insn_rows_witness_into((records, late), len(records), out.ptr, out.ptr + 8 * len(records) * 259)
        with pytest.raises(zkm.ZkmError, match=r"zkm_insn_rows_witness: raw_rows_out_dev: NULL with %d rows to write" % len(records)):
            ctx.insn_rows_witness_into((records, clocks), len(records), None, out.ptr)
        with pytest.raises(zkm.ZkmError, match=r"zkm_insn_rows_witness: arithmetic_ops_out_dev: NULL with %d operations to write" % len(want_arith)):
            ctx.insn_rows_witness_into((records, clocks), len(records), out.ptr, None)
        with pytest.raises(zkm.ZkmError, match=r"zkm_insn_rows_witness: raw_rows_out_dev is not aligned to its words \(8 bytes\)"):
            ctx.insn_rows_witness_into((records, clocks), len(records), out.ptr + 4, out.ptr + 8 * len(records) * 259)
        assert ctx.host_waits() == waits                               # every refusal was made on the host, before any device work
        assert (out.download() == 0x5A5A5A5A5A5A5A5A).all()            # ... and nothing was written
    finally:
        out.free()
    assert ctx.memory()[0] == live
    rows, arith = ctx.insn_rows_witness(records, clocks)
    assert_rows_equal(rows, want_rows)
    assert_arith_equal(arith, want_arith)


# ---------------------------------------------------------------- a whole segment
def program(m):
    """The thirteen kinds between ordinary steps (insn_rows_model.sample_insns), then more step kinds that read what the instructions
    wrote: a branch on a product, a store of hi, a count of lo's leading zeros, an immediate logic operation."""
    I.sample_insns(m)
    I.hilo(m, "MULT", 8, 13)
    I.binary(m, "MFHI", rd=26)
    I.binary(m, "MFLO", rd=27)
    m.branch("ne", 26, 27, 0x0010)
    m.nop()
    m.store("sw", 22, 26, 0xFFF8)
    m.count("clz", 27, 28)
    M.logic_imm(m, "ori", 27, 28, 0xF0F0)
    I.lui(m, 0, 28, 0xBEEF)
    m.binary_imm("addiu", 9, 28, 28, 0x1234, lambda a, b: a + b)
    m.nop()
    return m


_SEGMENT = {}


def segment(zkm):
    """The recorded program, padded to a power of two, with its host-expanded (CpuSteps, SegmentOps) pair: the model's rows behind the
    program's own RAW rows and the model's arithmetic list in numpy arrays.  Built once and not to be changed."""
    if not _SEGMENT:
        m = program(I.InsnRecorder())
        log_n = int(len(m.rows)).bit_length()
        m.pad((1 << log_n) - len(m.rows))
        steps = m.cpu_steps(zkm)
        records, clocks = m.insn_lists()
        patched = steps.steps.copy()
        patched[clocks.astype(np.int64) - m.first_clock] = I.steps(m, raw_base=steps.nraw)
        host = (zkm.CpuSteps(patched, np.concatenate([steps.raw_rows.reshape(-1, 259), m.insn_rows()])), zkm.SegmentOps(None, None, arithmetic_ops=m.insn_arith()))
        _SEGMENT.update(m=m, log_n=log_n, steps=steps, lists=(records, clocks), host=host)
    return _SEGMENT


def both_ways(ctx, zkm):
    """(composed, host-expanded): the device's expansion through calls_expand, and the segment's host pair."""
    s = segment(zkm)
    composed = ctx.calls_expand(s["steps"], first_clock=s["m"].first_clock, insns=s["lists"])
    return composed, s["host"], s["log_n"], s["m"]


def free_composed(composed):
    composed[0].raw_rows.free()
    composed[1].free()


def test_a_segment_equals_the_host_expanded_call_and_passes_the_three_device_checks(ctx, zkm):
    composed, host, log_n, m = both_ways(ctx, zkm)
    assert {x["kind"] for x in m.insns} == set(I.KINDS) and log_n <= 8
    assert composed[0].nraw == host[0].nraw and composed[0].steps.tobytes() == host[0].steps.tobytes()
    assert composed[1].counts["narithmetic"] == len(m.insn_arith())
    try:
        (wst, wlg), = ctx.segments_tables_steps([host[0]], [host[1]])
        waits = ctx.host_waits()
        (st, lg), = ctx.segments_tables_steps([composed[0]], [composed[1]])
        assert ctx.host_waits() - waits == 3                           # the tables call's waits are unchanged
        assert lg == wlg
        assert_tables_equal(tables_of(st, lg, ctx), tables_of(wst, wlg, ctx))
        assert all(f[0] is None for f in ctx.segment_witness_check(st, lg)) and ctx.witness_message is None, ctx.witness_message
        assert ctx.segment_lookup_check(st, lg) == [LM.HOLDS] * 12 and ctx.lookup_message is None, ctx.lookup_message
        report = ctx.segment_check_ctls(st, lg)
        assert report.kind == 0, report.message
        st.free()
        wst.free()
    finally:
        free_composed(composed)


def test_own_arithmetic_operations_stay_in_front_of_the_generated_ones(ctx, zkm):
    s = segment(zkm)
    m = s["m"]
    own =np.array([(1, 5, 6), (8, 3, 4)], dtype=np.uint32)            # {IS_ADDU, 5, 6}, {IS_MUL, 3, 4}: any operations of the caller's
    composed = ctx.calls_expand(s["steps"], first_clock=m.first_clock, insns=s["lists"], arithmetic_ops=own)
    try:
        want = np.concatenate([own, m.insn_arith()])
        assert composed[1].counts["narithmetic"] == len(want)
        got = composed[1].lists["arithmetic_ops"].download().view(np.uint32)[:3 * len(want)].reshape(-1, 3)
        assert_arith_equal(got, want)
    finally:
        free_composed(composed)


def test_proofs_equal_the_host_expanded_call(ctx, zkm):
    composed, host, _, _ = both_ways(ctx, zkm)
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
