"""GPU suite: a segment's CPU table and the operations its rows push, built on the device from the compact step log (zkm_cpu_witness,
zkm_segments_tables_steps, zkm_prove_segments_ops_steps).  The judge is cpu_fixtures.Machine: the recorder of tests/cpu_steps_model.py
logs what the Machine read while it filled its rows, and everything the device makes of that log -- the table, the three lists in push
order, whole segments and their proofs -- must equal what the Machine (or the calls without steps, on the Machine's rows and lists)
gives, word for word.  Shapes: 2^8 rows (one workgroup of steps), 2^9 (two workgroups, eight waves: the list offsets cross both), a
handful of PAD rows at a nonzero first clock, K = 2 of different heights, with and without a bootstrap image."""
import numpy as np
import pytest

from zkm_amd import tables as T

from . import boot_fixtures as BF
from . import cpu_fixtures as CF
from . import cpu_steps_model as M
from .test_gpu_segment_ops import assert_tables_equal, tables_of

pytestmark = pytest.mark.gpu

P = CF.P


def assert_lists_equal(got, m, mem_from=0):
    for name, g, w in zip(("memory", "logic", "arithmetic"), got, M.expected_lists(m, mem_from)):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, "%s operations: first differing word at %s" % (name, bad[0])


def assert_table_equals_rows(table, rows, log_n, first=0):
    """The column-major 2^log_n-row table against the Machine's rows from row `first` on, zero elsewhere."""
    want = np.zeros((CF.W, 1 << log_n), dtype=np.uint64)
    want[:, first:first + len(rows)] = M.rows_array(rows).T
    bad = np.argwhere(table.reshape(CF.W, -1) != want)
    assert bad.size == 0, "first differing cell (column, row) %s: %d, expected %d" % (bad[0], table.reshape(CF.W, -1)[tuple(bad[0])], want[tuple(bad[0])])


def test_one_segment_equals_the_machine_and_passes_the_constraints(ctx, zkm):
    m = M.sample()
    table, mem, logic, arith = ctx.cpu_witness(m.cpu_steps(zkm), 8)
    assert (table == m.trace(8)).all()
    assert_table_equals_rows(table, m.rows, 8)
    assert_lists_equal((mem, logic, arith), m)
    # a second judge: the CPU constraints hold on the device-built table (the fake CTL shape: no column sets)
    for alphas in ([0x1234567 % P], [0x1234567 % P, 0xFEDCBA9876543210 % P]):
        assert ctx.check_constraints(table, 8, np.zeros(4 << 8, dtype=np.uint64), None, [1, 1], None, alphas, ncols=CF.W, table_id=T.TABLE_CPU) is None


def test_list_offsets_across_workgroups_and_waves(ctx, zkm):
    m = M.sample(2)
    assert 256 < len(m.steps) <= 512
    table, mem, logic, arith = ctx.cpu_witness(m.cpu_steps(zkm), 9)
    assert_lists_equal((mem, logic, arith), m)
    assert_table_equals_rows(table, m.rows, 9)
    # RAW rows in device memory, words above p among them: the same table
    raw = m.raw_array().copy()
    raw[raw < (1 << 32) - 1] += np.uint64(P)
    dev = ctx.alloc(raw.size).upload(raw)
    table2, mem2, _, _ = ctx.cpu_witness(zkm.CpuSteps(m.step_array(), dev, nraw=len(raw)), 9)
    dev.free()
    assert (table2 == table).all() and (mem2 == mem).all()


def test_pad_rows_and_a_nonzero_first_clock(ctx, zkm):
    steps = np.zeros(5, dtype=M.STEP_DT)
    steps["kind"] = M.KIND["PAD"]
    steps["pc"], steps["next_pc"], steps["context"] = 0x4321, 0x4325, [0, 0, 7, 7, 7]
    steps["insn"], steps["flags"] = 0xFFFFFFFF, 1            # a PAD row takes nothing else from its record
    steps["reads"] = 0xABCD
    table, mem, logic, arith = ctx.cpu_witness(zkm.CpuSteps(steps), 4, first_clock=9)
    assert mem.size == 0 and logic.size == 0 and arith.size == 0
    want = np.zeros((CF.W, 16), dtype=np.uint64)
    for i in range(5):                                       # the five assignments of generation/mod.rs:171-176
        row = 9 + i
        want[CF.CLOCK, row] = row
        want[CF.CONTEXT, row] = steps["context"][i]
        want[CF.PC, row] = 0x4321
        want[CF.NEXT_PC, row] = 0x4325
        want[CF.IS_EXIT, row] = 1
    assert (table.reshape(CF.W, 16) == want).all()
    with pytest.raises(zkm.ZkmError, match=r"zkm_cpu_witness: rows \[12, 17\) do not fit in 2\^4"):
        ctx.cpu_witness(zkm.CpuSteps(steps), 4, first_clock=12)
    # real rows behind a nonzero first clock carry it in their timestamps
    m = M.Recorder()
    m.set_reg(8, 3)
    m.binary("addu", 8, 8, 9, 0x21, lambda a, b: a + b)
    table, mem, _, arith = ctx.cpu_witness(zkm.CpuSteps(m.step_array()[2:], m.raw_array()), 3, first_clock=2)
    assert_table_equals_rows(table, m.rows[2:], 3, first=2)
    assert (mem == M.expected_lists(m, mem_from=3)[0]).all() and arith.tolist() == [[M.ARITH_FLAG["addu"], 3, 3]]


def test_extra_operand_cases_judged_by_the_machine(ctx, zkm):
    m = M.extra_program(M.Recorder())
    kinds = {M.KINDS[s[3]] for s in m.steps}
    assert {"BINARY_OP", "BINARY_IMM_OP", "BRANCH", "LOGIC_OP", "M_OP_LOAD", "JUMPS"} <= kinds
    taken = {(r[CF.BR["is_eq"]], r[CF.BR["is_ne"]], r[CF.BR["is_le"]], r[CF.BR["is_gt"]], r[CF.BR["is_lt"]], r[CF.BR["is_ge"]], r[CF.BR["should_jump"]])
             for r in m.rows if r[CF.OP["branch"]]}
    assert len(taken) == 12                                  # six kinds, each taken and not taken
    assert any(r[CF.OP["binary_op"]] and not r[CF.ch(2, 0)] for r in m.rows)      # a write to register 0
    log_n = 7
    assert len(m.rows) <= 1 << log_n
    table, mem, logic, arith = ctx.cpu_witness(m.cpu_steps(zkm), log_n)
    assert_table_equals_rows(table, m.rows, log_n)
    assert_lists_equal((mem, logic, arith), m)
    # a BGEZ whose channel 1 names register 0 (the Machine's choice once register 1 holds a value; the reference's always): flag bit 1
    m2 = M.Recorder()
    m2.set_reg(1, 7)
    m2.set_reg(9, 3)
    m2.branch("ge", 9, 0, 4)
    m2.nop()
    assert [M.KINDS[s[3]] for s in m2.steps[-2:]] == ["BRANCH", "NOP"] and m2.steps[-2][4] == 3 and m2.rows[-2][CF.ch(1, 4)] == 0
    table, mem, _, _ = ctx.cpu_witness(m2.cpu_steps(zkm), 3)
    assert_table_equals_rows(table, m2.rows, 3)
    assert (mem == M.expected_lists(m2)[0]).all()


def test_logic_immediates_against_the_restated_generator_and_the_constraints(ctx, zkm):
    m = M.Recorder()
    m.set_reg(8, 0x12345678)
    m.set_reg(9, 0xFFFF0F0F)
    for name in ("andi", "ori", "xori"):
        for rs, rt, imm in ((8, 16, 0xFF00), (9, 17, 0xFFFF), (8, 0, 0x8001), (0, 18, 0x00F0)):     # (a write to register 0; a read of it)
            M.logic_imm(m, name, rs, rt, imm)
    m.nop()
    assert {M.KINDS[s[3]] for s in m.steps[4:]} == {"LOGIC_IMM_OP", "NOP"} and not m.logic_ops
    assert len(m.rows) == 17
    table, mem, logic, arith = ctx.cpu_witness(m.cpu_steps(zkm), 5)
    assert_table_equals_rows(table, m.rows, 5)
    assert_lists_equal((mem, logic, arith), m)
    for alphas in ([0x1234567 % P], [0x1234567 % P, 0xFEDCBA9876543210 % P]):
        assert ctx.check_constraints(table, 5, np.zeros(4 << 5, dtype=np.uint64), None, [1, 1], None, alphas, ncols=CF.W, table_id=T.TABLE_CPU) is None


def test_user_mode_and_a_nonzero_context(ctx, zkm):
    """The Machine runs in kernel mode with context 0.  A store and a load logged in user mode with context 5: the rows are the
    Machine's with is_kernel_mode cleared, the context cell set and the context of the code-segment channels set (registers keep
    context 0), and so are their memory operations."""
    m = M.Recorder()
    m.set_reg(22, 0x100)
    m.set_reg(9, 0xA1B2C3D4)
    m.store("sb", 22, 9, 1)
    m.load("lh", 22, 23, 2)
    steps = m.step_array()
    steps["context"][-2:], steps["flags"][-2:] = 5, 0
    rows = [list(r) for r in m.rows]
    for r, code_channels in ((rows[-2], (2, 3)), (rows[-1], (2,))):
        r[CF.KERNEL], r[CF.CONTEXT] = 0, 5
        for i in code_channels:
            assert r[CF.ch(i, 0)] == 1 and r[CF.ch(i, 3)] == CF.SEG_CODE
            r[CF.ch(i, 2)] = 5
    mem_want = M.expected_lists(m)[0]
    late = (mem_want[:, 3] >= 10 * (len(rows) - 2)) & (mem_want[:, 1] == CF.SEG_CODE)
    assert late.sum() == 3
    mem_want[late, 0] = 5
    table, mem, _, _ = ctx.cpu_witness(zkm.CpuSteps(steps, m.raw_array()), 3)
    assert_table_equals_rows(table, rows, 3)
    assert (mem == mem_want).all()


# ---------------------------------------------------------------- whole segments
def own_ops(seed, first_ts):
    """A few operations of the caller's own, behind the steps' in the joined lists: memory at addresses the program does not touch."""
    rng = np.random.default_rng(seed)
    n = 9
    mem = np.zeros((n, 6), dtype=np.uint64)
    mem[:, 1], mem[:, 2], mem[:, 3], mem[:, 4], mem[:, 5] = 2, rng.integers(0, 64, n), first_ts + np.arange(n), rng.integers(0, 2, n), rng.integers(0, 1 << 32, n)
    logic = np.stack([rng.integers(0, 4, 5), rng.integers(0, 1 << 32, 5), rng.integers(0, 1 << 32, 5)], axis=1).astype(np.uint32)
    arith = np.array([(M.ARITH_FLAG["addu"], 1, 2), (M.ARITH_FLAG["srl"], 0x80000000, 3), (M.ARITH_FLAG["sltu"], 5, 4)], dtype=np.uint32)
    return mem, logic, arith


def segment_pair(zkm, m, log_n, own, nboot=0, boot_mem=0):
    """(CpuSteps, the SegmentOps beside them, the expanded SegmentOps of the call without steps) of a recorded Machine padded to
    2^log_n rows.  own: (memory, logic, arithmetic) of the caller, or None."""
    m.pad((1 << log_n) - len(m.rows))
    mem, logic, arith = M.expected_lists(m, mem_from=boot_mem)
    e = lambda w, dt: np.zeros((0, w), dtype=dt)
    omem, ologic, oarith = own if own is not None else (e(6, np.uint64), e(3, np.uint32), e(3, np.uint32))
    beside = zkm.SegmentOps(None, omem if len(omem) else None, arithmetic_ops=oarith if len(oarith) else None,
                            logic_ops=ologic if len(ologic) else None)
    expanded = zkm.SegmentOps(M.rows_array(m.rows[nboot:]), np.concatenate([mem, omem]), arithmetic_ops=np.concatenate([arith, oarith]),
                              logic_ops=np.concatenate([logic, ologic]))
    return m.cpu_steps(zkm), beside, expanded


@pytest.fixture(scope="module")
def two(zkm):
    """Two segments of different heights, 2^8 and 2^9, PAD-filled: without and with operations of the caller's own."""
    out = {}
    for key, own in (("bare", False), ("own", True)):
        a, b = M.Recorder(), M.Recorder()
        CF.sample_program(a)
        CF.sample_program(CF.sample_program(b))
        out[key] = [segment_pair(zkm, a, 8, own_ops(1, 10 * 256) if own else None), segment_pair(zkm, b, 9, own_ops(2, 10 * 512) if own else None)]
    return out


def test_two_segments_of_different_heights_equal_the_call_on_rows(ctx, zkm, two):
    segs = two["own"]
    live = ctx.memory()[0]
    want = ctx.segments_tables([e for _, _, e in segs])
    assert ctx.segments_tables_steps([s for s, _, _ in segs], [o for _, o, _ in segs], sizing=True) == [lg for _, lg in want]
    for st, _ in ctx.segments_tables_steps([s for s, _, _ in segs], [o for _, o, _ in segs]):      # (the first call may grow the download area)
        st.free()
    before = ctx.host_waits()
    got = ctx.segments_tables_steps([s for s, _, _ in segs], [o for _, o, _ in segs])
    assert ctx.host_waits() - before == 3
    assert [lg[1] for _, lg in got] == [8, 9]
    for (st, lg), (wst, wlg) in zip(got, want):
        assert lg == wlg
        assert_tables_equal(tables_of(st, lg, ctx), tables_of(wst, wlg, ctx))
        st.free()
        wst.free()
    assert ctx.memory()[0] == live
    # the step kernel wrote the table; the transpose of rows was not launched for these segments
    ctx.profile(True)
    try:
        ctx.profile_reset()
        for st, _ in ctx.segments_tables_steps([s for s, _, _ in segs], [o for _, o, _ in segs]):
            st.free()
        rec = ctx.profile_records()
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    assert rec["cpu_steps/lists"][0] == 1 and rec["cpu_steps/rows"][0] == 1 and "segment_ops/cpu_rows_to_cols" not in rec


def test_two_segments_each_with_a_bootstrap_image_in_front_of_the_steps(ctx, zkm, oracle):
    """K = 2 with different heights and different bootstraps: image b (4 bootstrap rows, no page; 2^8 rows with the program) and
    image a (135 bootstrap rows, two pages; 2^9), so each segment has its own first clock and its own offsets into the joined lists,
    and the shorter segment's grid is the taller one's."""
    class BootRecorder(M.StepRecorder, BF.BootMachine):
        pass
    images, steps, beside, expanded, heights = [], [], [], [], []
    for k, (name, own) in enumerate((("b", own_ops(3, 10 << 8)), ("a", None))):
        seg = BF.segment(oracle, name)
        model = seg["model"]
        m = CF.sample_program(BootRecorder(model, raw_boot=False))
        nboot = len(model.cpu_rows)
        assert m.first_clock == nboot and len(m.steps) == len(m.rows) - nboot
        log_n = int(len(m.rows) - 1).bit_length()
        s, o, e = segment_pair(zkm, m, log_n, own, nboot=nboot, boot_mem=len(model.memory_ops))
        images.append(BF.boot_image(zkm, seg["image"]))
        steps.append(s), beside.append(o), expanded.append(e), heights.append(log_n)
    assert heights == [8, 9]
    want = ctx.segments_tables_boot(images, expanded)
    got = ctx.segments_tables_steps(steps, beside, images=images)
    for (st, lg), (wst, wlg) in zip(got, want):
        assert lg == wlg
        assert_tables_equal(tables_of(st, lg, ctx), tables_of(wst, wlg, ctx))
        st.free()
        wst.free()
    # ... and in the other order (the taller segment first), one segment alone
    got = ctx.segments_tables_steps(steps[::-1], beside[::-1], images=images[::-1])
    alone = ctx.segments_tables_steps(steps[1:], beside[1:], images=images[1:])
    assert [lg for _, lg in got] == [lg for _, lg in want][::-1]
    assert_tables_equal(tables_of(*got[0], ctx), tables_of(*alone[0], ctx))
    for st, _ in got + alone:
        st.free()


def test_proofs_equal_the_call_on_rows(ctx, zkm, two):
    segs = two["bare"]
    pubs = [[1, 2, 3], [7, 1]]
    want = ctx.prove_segments_ops([e for _, _, e in segs], public_values=pubs)
    got = ctx.prove_segments_ops_steps([s for s, _, _ in segs], [o for _, o, _ in segs], public_values=pubs)
    ctx.set_tuning("check_ctls", 1)      # ... and the lists derived on the device balance every CPU lookup
    try:
        checked = ctx.prove_segments_ops_steps([segs[0][0]], [segs[0][1]], public_values=pubs[:1])
    finally:
        ctx.set_tuning("check_ctls", 0)
    for s, ((p, c, o), (wp, wc, wo)) in enumerate(zip(got + checked, want + want[:1])):
        assert o == wo and (c == wc).all(), s
        bad = np.nonzero(p != wp)[0]
        assert bad.size == 0, "segment %d: first differing proof word %d" % (s, bad[0])
