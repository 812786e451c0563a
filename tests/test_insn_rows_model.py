"""CPU suite: the model of the thirteen instructions' rows (tests/insn_rows_model.py) held against judges it shares nothing with -- rows
computed by hand from the reference's generators (witness/operation.rs:286-433, :1804-1928), the oracle's CPU constraints on a small
program, and the lookup model (tests/check_ctls_model.py) with the oracle's check_ctls on the CPU table's three lookups, beside the
Arithmetic table of the program's operations and the Memory table of its memory operations."""
import numpy as np
import pytest

from zkm_amd import tables as T

from . import arith_fixtures as A
from . import check_ctls_model as CM
from . import cpu_fixtures as CF
from . import insn_rows_model as I

REG = CF.SEG_REG


def by_hand(clock, pc, insn, flag, channels, extra=()):
    """A row written out cell by cell: the fixed part, one op flag, the six cells of the channels given, the extra cells."""
    r = [0] * CF.W
    r[CF.CLOCK], r[CF.PC], r[CF.NEXT_PC], r[CF.KERNEL], r[CF.OP[flag]] = clock, pc, pc + 4, 1, 1
    fields = ((insn >> 26) & 63, 6), ((insn >> 21) & 31, 5), ((insn >> 16) & 31, 5), ((insn >> 11) & 31, 5), ((insn >> 6) & 31, 5), (insn & 63, 6)
    col = 50
    for value, width in fields:                             # opcode, rs, rt, rd, shamt, func from column 50, each from its low bit
        for i in range(width):
            r[col + i] = (value >> i) & 1
        col += width
    assert col == 82
    for i, cells in channels.items():
        r[205 + 6 * i:211 + 6 * i] = cells                  # used, is_read, context, segment, virtual, value
    for c, v in extra:
        r[c] = v
    return r


def machine(**regs):
    m = I.InsnRecorder()
    for reg, v in regs.items():
        m.set_reg(int(reg[1:]), v)
    return m


def last(m):
    x = m.insns[-1]
    return x["row"], x["mask"], x["arith"], x["record"]


def test_lui_of_0x8000_into_register_0_by_hand():
    m = machine()
    clock, pc = m.clock, m.pc
    I.lui(m, 0, 0, 0x8000)
    row, mask, arith, record = last(m)
    # three writes to register 0: the channels are filled with used = 0, nothing is pushed but the arithmetic operation
    want = by_hand(clock, pc, 0x3C008000, "binary_imm_op", {0: [0, 0, 0, REG, 0, 0xFFFF8000], 1: [0, 0, 0, REG, 0, 0x10000], 2: [0, 0, 0, REG, 0, 0x80000000]})
    assert row == want and mask == 0 and arith == (A.IS_LUI, 0xFFFF8000, 0x10000)
    assert record == (pc, pc + 4, 0x3C008000, I.KIND["LUI"], 1, 0, [0] * 6) and m.regs[0] == 0
    # rs and rt that are registers: the reference writes sext(imm) to rs, then 1 << 16 and the result to rt
    clock, pc = m.clock, m.pc
    I.lui(m, 17, 18, 0x7FFF)
    row, mask, arith, _ = last(m)
    want = by_hand(clock, pc, 0x3C000000 | 17 << 21 | 18 << 16 | 0x7FFF, "binary_imm_op",
                   {0: [1, 0, 0, REG, 17, 0x7FFF], 1: [1, 0, 0, REG, 18, 0x10000], 2: [1, 0, 0, REG, 18, 0x7FFF0000]})
    assert row == want and mask == 7 and arith == (A.IS_LUI, 0x7FFF, 0x10000) and (m.regs[17], m.regs[18]) == (0x7FFF, 0x7FFF0000)


def test_mult_of_two_negative_operands_by_hand():
    for a, b, lo, hi in ((0xFFFFFFF9, 0xFFFFFFFD, 21, 0), (0x80000000, 0x80000000, 0, 0x40000000), (0xFFFFFFFF, 0x80000000, 0x80000000, 0)):
        m = machine(r8=a, r9=b)
        clock, pc = m.clock, m.pc
        I.hilo(m, "MULT", 8, 9)
        row, mask, arith, record = last(m)
        want = by_hand(clock, pc, 8 << 21 | 9 << 16 | 0x18, "binary_op", {0: [1, 1, 0, REG, 8, a], 1: [1, 1, 0, REG, 9, b], 2: [1, 0, 0, REG, 32, lo], 3: [1, 0, 0, REG, 33, hi]})
        assert row == want and mask == 0xF and arith == (A.IS_MULT, a, b) and record[6] == [a, b, 0, 0, 0, 0]
    # the same operands unsigned
    m = machine(r8=0xFFFFFFF9, r9=0xFFFFFFFD)
    I.hilo(m, "MULTU", 8, 9)
    row = last(m)[0]
    assert (row[CF.ch(2, 5)], row[CF.ch(3, 5)]) == (21, 0xFFFFFFF6) and 0xFFFFFFF9 * 0xFFFFFFFD == 0xFFFFFFF6 << 32 | 21


def test_div_of_minus_7_by_2_by_hand():
    m = machine(r8=0xFFFFFFF9, r9=2)
    clock, pc = m.clock, m.pc
    I.hilo(m, "DIV", 8, 9)
    row, mask, arith, _ = last(m)
    # Rust's / truncates toward zero (-3) and % takes the dividend's sign (-1)
    want = by_hand(clock, pc, 8 << 21 | 9 << 16 | 0x1A, "binary_op",
                   {0: [1, 1, 0, REG, 8, 0xFFFFFFF9], 1: [1, 1, 0, REG, 9, 2], 2: [1, 0, 0, REG, 32, 0xFFFFFFFD], 3: [1, 0, 0, REG, 33, 0xFFFFFFFF]})
    assert row == want and mask == 0xF and arith == (A.IS_DIV, 0xFFFFFFF9, 2)
    for a, b, lo, hi in ((7, 0xFFFFFFFE, 0xFFFFFFFD, 1), (0xFFFFFFF9, 0xFFFFFFFE, 3, 0xFFFFFFFF), (0x80000000, 2, 0xC0000000, 0), (7, 2, 3, 1)):
        assert I.result("DIV", a, b) == (lo, hi), (a, b)
    assert I.result("DIVU", 0xFFFFFFF9, 2) == (0x7FFFFFFC, 1)


def test_mfhi_into_register_0_by_hand():
    m = machine(r33=6)
    clock, pc = m.clock, m.pc
    I.binary(m, "MFHI", rd=0)
    row, mask, arith, record = last(m)
    want = by_hand(clock, pc, 0x10, "binary_op", {0: [1, 1, 0, REG, 33, 6], 1: [1, 1, 0, REG, 0, 0], 2: [0, 0, 0, REG, 0, 6]})
    assert row == want and mask == 3 and arith == (A.IS_MFHI, 6, 0) and record[6] == [6, 0, 0, 0, 0, 0]
    # MTLO writes register 32 from rs
    m = machine(r13=0x12345678)
    clock, pc = m.clock, m.pc
    I.binary(m, "MTLO", rs=13)
    row, mask, arith, _ = last(m)
    want = by_hand(clock, pc, 13 << 21 | 0x13, "binary_op", {0: [1, 1, 0, REG, 13, 0x12345678], 1: [1, 1, 0, REG, 0, 0], 2: [1, 0, 0, REG, 32, 0x12345678]})
    assert row == want and mask == 7 and arith == (A.IS_MTLO, 0x12345678, 0) and m.regs[32] == 0x12345678


def test_sdc1_and_the_nops_by_hand():
    m = machine(r22=0x10C, r13=0x80000001)
    clock, pc = m.clock, m.pc
    I.sdc1(m, 22, 13, 0xFFFF)                               # 0x10C - 1 = 0x10B: the word at 0x108 (0x33 from the bootstrap), low bits 11
    row, mask, arith, record = last(m)
    bits = [(86 + i, 1) for i in range(32) if (0x10B >> i) & 1] + [(86 + 32 + i, 1) for i in (0, 31)] + [(86 + 64 + i, 1) for i in (0, 1, 4, 5)]
    want = by_hand(clock, pc, 0x3D << 26 | 22 << 21 | 13 << 16 | 0xFFFF, "m_op_store",
                   {0: [1, 1, 0, REG, 22, 0x10C], 1: [1, 1, 0, REG, 13, 0x80000001], 2: [1, 1, 0, 0, 0x108, 0x33], 3: [1, 0, 0, 0, 0x108, 0]},
                   extra=bits + [(188 + 13, 1), (188 + 15, 1)])                        # is_sdc1, aux_filter; aux_rs0_mul_rs1 (column 182) stays 0
    assert row == want and row[86 + 96] == 0 and mask == 0xF and arith is None and record[6] == [0x10C, 0x80000001, 0x33, 0, 0, 0]
    assert m.mem[(CF.SEG_CODE, 0x108)] == 0
    for name, insn, kw in (("SYNC", 0x0F, {}), ("SYNC", 1 << 21 | 2 << 16 | 3 << 11 | 4 << 6 | 0x0F, dict(rs=1, rt=2, rd=3, sa=4)),
                           ("PREF", 0x33 << 26 | 22 << 21 | 1 << 16 | 0x8010, dict(rs=22, rt=1, imm=0x8010))):
        clock, pc = m.clock, m.pc
        I.nop_like(m, name, **kw)
        row, mask, arith, record = last(m)
        assert row == by_hand(clock, pc, insn, "nop", {}) and mask == 0 and arith is None and record[2:4] == (insn, I.KIND[name])


# ---------------------------------------------------------------- the judges: the oracle's constraints and the lookups
_PROGRAM = {}


def program():
    """The sample of the thirteen kinds, padded to a power of two; built once and not to be changed."""
    if not _PROGRAM:
        m = I.sample_insns(I.InsnRecorder())
        log_n = len(m.rows).bit_length()
        m.pad((1 << log_n) - len(m.rows))
        _PROGRAM.update(m=m, log_n=log_n, trace=m.trace(log_n))
    return _PROGRAM["m"], _PROGRAM["log_n"], _PROGRAM["trace"]


def first_of_each_kind(m):
    first = {}
    for x in m.insns:
        first.setdefault(x["kind"], x)
    assert list(sorted(first)) == sorted(I.KINDS)
    return first


def test_model_rows_pass_the_oracles_cpu_constraints(oracle):
    m, log_n, trace = program()
    assert {x["kind"] for x in m.insns} == set(I.KINDS) and log_n <= 8
    count, bad = oracle.debug_constraints(T.TABLE_CPU, trace, 259, log_n)
    assert count == 741 and bad is None, bad
    cols = trace.reshape(259, -1)
    assert (cols[CF.CLOCK] == np.arange(1 << log_n)).all()
    assert all((cols[:, x["clock"]] == np.array(x["row"], dtype=np.uint64)).all() for x in m.insns)


def lookup_tables(oracle, m, log_n, trace):
    """CPU, Memory, Logic and Arithmetic with the three lookups the CPU table takes part in (cpu_fixtures.build_cpu_segment's)."""
    from zkm_amd.ctl import CtlTable
    code = {"and": T.OP_AND, "or": T.OP_OR, "xor": T.OP_XOR, "nor": T.OP_NOR}
    logic = oracle.logic_trace(np.array([(code[name], a, b) for name, a, b, _ in m.logic_ops], dtype=np.uint32), 3)
    arith = A.generate_trace(I.arith_flags(m))
    mem_ops = np.array([(ctx, seg, virt, ts, is_read, value) for is_read, ctx, seg, virt, value, ts in m.mem_ops], dtype=np.uint64)
    log_mem = int(np.ceil(np.log2(len(mem_ops)))) + 1
    memory, _ = oracle.memory_trace(mem_ops, log_mem)
    cc, cm, cl, ca = CtlTable(), CtlTable(), CtlTable(), CtlTable()
    tables = [(T.TABLE_CPU, trace, 259, log_n, cc), (T.TABLE_MEMORY, memory, 13, log_mem, cm), (T.TABLE_LOGIC, logic, 69, 3, cl),
              (T.TABLE_ARITHMETIC, arith, 54, 16, ca)]
    ctls = [T.ctl_arithmetic(0, 3, cc, ca), (T.logic_lookers_cpu(0, cc), (2, T.logic_ctl_data(cl))), (T.memory_lookers_cpu(0, cc), (1, T.memory_ctl_data(cm)))]
    return tables, ctls


def test_model_rows_balance_every_lookup_of_the_cpu_table(oracle):
    m, log_n, trace = program()
    tables, ctls = lookup_tables(oracle, m, log_n, trace)
    for tid, tr, width, lg, _ in tables[1:]:                # the other three tables are valid tables
        assert oracle.debug_constraints(tid, tr, width, lg)[1] is None, tid
    assert CM.Model().check(tables, ctls) is None
    assert oracle.check_ctls(tables, ctls) == 0
    # the lookups have teeth: a result that is off by one leaves the Arithmetic lookup (0) unbalanced, for each of the ten kinds that
    # push an operation, and a stored word that is off by one the Memory lookup (2)
    model = CM.Model()
    for kind, x in first_of_each_kind(m).items():
        if x["arith"] is None and kind != "SDC1":
            continue
        cell = CF.ch(3 if kind == "SDC1" else 2, 5)
        bad = CM.bump(tables, 0, cell * (1 << log_n) + x["clock"])
        found = model.check(bad, ctls)
        assert found is not None and found["kind"] == 2 and found["ctl"] == (2 if kind == "SDC1" else 0), (kind, found)
        assert CM.verdict_of_code(oracle.check_ctls(bad, ctls)) == (2, found["ctl"]), kind


@pytest.mark.parametrize("kind", I.KINDS)
def test_one_flipped_cell_per_kind_is_named_by_the_oracle(oracle, kind):
    """The rows are live under the constraints: a channel whose `used` cell is no bit is refused at the instruction's row -- and SDC1's
    stored value and address bits, which the CPU constraints speak about, are held too."""
    m, log_n, trace = program()
    x = first_of_each_kind(m)[kind]
    cells = [(CF.ch(0, 0), 2)]
    if kind == "SDC1":
        cells += [(CF.ch(3, 5), 5), (CF.GEN, 1 - x["row"][CF.GEN])]
    for col, v in cells:
        flipped = trace.reshape(259, -1).copy()
        flipped[col, x["clock"]] = v
        bad = oracle.debug_constraints(T.TABLE_CPU, flipped.reshape(-1), 259, log_n)[1]
        assert bad is not None and bad[0] == x["clock"], (kind, col, bad)
