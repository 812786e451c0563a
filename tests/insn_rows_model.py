"""The thirteen instructions decode() accepts (witness/transition.rs:42-312) and no step kind takes, on the host (test infrastructure):
their generators restated from the reference on top of cpu_fixtures.Machine, the way cpu_steps_model.logic_imm adds one --
  lui                          generate_lui (witness/operation.rs:405-433)
  binary (MUL MFHI MTHI MFLO MTLO)   generate_binary_arithmetic_op (:286-318) with the operands decode hands it
  hilo (MULT MULTU DIV DIVU)   generate_binary_arithmetic_hilo_op (:320-375)
  sdc1                         generate_mstore_general with MemOp::SDC1 (:1804-1928)
  nop_like (SYNC PREF)         generate_nop
with results as BinaryOperator::result computes them (arithmetic/mod.rs:48-133).  On an InsnRecorder each such row is recorded as a
ZKM_INSN_* record with its clock, the expected row, the mask of its used channels and the arithmetic triple it pushes, and leaves a
placeholder in the step list; on a plain Machine the row is pushed like any other.  Everything the device makes of the records
(zkm_insn_rows_counts, zkm_insn_rows_steps, zkm_insn_rows_witness) must equal this word for word; the model itself is held against
hand-computed rows, the oracle's CPU constraints and the lookup model in tests/test_insn_rows_model.py."""
import numpy as np

from . import arith_fixtures as A
from . import cpu_fixtures as CF
from . import cpu_steps_model as M

KINDS = ("LUI", "MUL", "MULT", "MULTU", "DIV", "DIVU", "MFHI", "MTHI", "MFLO", "MTLO", "SDC1", "SYNC", "PREF")
KIND = {name: k for k, name in enumerate(KINDS)}
FILTER = {"LUI": A.IS_LUI, "MUL": A.IS_MUL, "MULT": A.IS_MULT, "MULTU": A.IS_MULTU, "DIV": A.IS_DIV, "DIVU": A.IS_DIVU, "MFHI": A.IS_MFHI,
          "MTHI": A.IS_MTHI, "MFLO": A.IS_MFLO, "MTLO": A.IS_MTLO}
REG_LO, REG_HI = 32, 33
MASK32 = 0xFFFFFFFF
ROWS_PER_WG = 16          # the rows a workgroup of k_insn_rows takes (csrc/insn_rows.hip)


def s32(x):
    return x - (1 << 32) if x & 0x80000000 else x


def result(name, a, b):
    """BinaryOperator::result (arithmetic/mod.rs:48-133) of the ten operators: (result0, result1) = (lo, hi)."""
    if name == "MUL":
        return (a * b) & MASK32, 0
    if name == "LUI":
        return (CF.sext(a, 16) << 16) & MASK32, 0
    if name in ("MULT", "MULTU"):
        out = (s32(a) * s32(b) if name == "MULT" else a * b) & ((1 << 64) - 1)
        return out & MASK32, out >> 32
    if name == "DIV":                                       # Rust's / truncates toward zero and % takes the dividend's sign
        x, y = s32(a), s32(b)
        q = abs(x) // abs(y) * (1 if (x < 0) == (y < 0) else -1)
        return q & MASK32, (x - q * y) & MASK32
    if name == "DIVU":
        return a // b, a % b
    assert name in ("MFHI", "MTHI", "MFLO", "MTLO"), name
    return a, 0


# ---------------------------------------------------------------- the generators
def _row(m, insn):
    """The row's fixed part: Machine.new_row's, with the kernel flag and the context of a machine that has them set."""
    r = m.new_row(insn)
    r[CF.KERNEL], r[CF.CONTEXT] = getattr(m, "kernel", 1), getattr(m, "context", 0)
    return r


def _push(m, r, kind, arith):
    if hasattr(m, "push_insn"):
        m.push_insn(r, kind, arith)
    else:
        m.push(r)


def lui(m, rs, rt, imm):
    """LUI (opcode 0x0F): generate_lui(rs, rt, imm) -- channel 0 writes sext(imm) to register rs, push_no_write fills channel 1 with
    1 << 16 before reg_write_with_log writes it to rt there, channel 2 writes the result to rt."""
    r = _row(m, CF.enc_i(0x0F, rs, rt, imm))
    r[CF.OP["binary_imm_op"]] = 1
    in0, in1 = CF.sext(imm, 16), 1 << 16
    m.reg_write(r, 0, rs, in0)
    m.channel(r, 1, 0, 0, 0, 0, in1)
    m.reg_write(r, 1, rt, in1)
    m.reg_write(r, 2, rt, result("LUI", in0, in1)[0])
    _push(m, r, "LUI", (A.IS_LUI, in0, in1))


def binary(m, name, rs=0, rt=0, rd=0, sa=0):
    """MUL (0x1C, 0x02) and the four moves (0, 0x10 .. 0x13): generate_binary_arithmetic_op with decode's operands
    (transition.rs:135-188): MUL (rs, rt, rd); MFHI (33, 0, rd); MTHI (rs, 0, 33); MFLO (32, 0, rd); MTLO (rs, 0, 32)."""
    op, fn = (0x1C, 0x02) if name == "MUL" else (0, {"MFHI": 0x10, "MTHI": 0x11, "MFLO": 0x12, "MTLO": 0x13}[name])
    src0, src1, dest = {"MUL": (rs, rt, rd), "MFHI": (REG_HI, 0, rd), "MTHI": (rs, 0, REG_HI), "MFLO": (REG_LO, 0, rd), "MTLO": (rs, 0, REG_LO)}[name]
    r = _row(m, CF.enc_r(op, rs, rt, rd, sa, fn))
    r[CF.OP["binary_op"]] = 1
    in0, in1 = m.reg_read(r, 0, src0), m.reg_read(r, 1, src1)
    m.reg_write(r, 2, dest, result(name, in0, in1)[0])
    _push(m, r, name, (FILTER[name], in0, in1))


def hilo(m, name, rs, rt, rd=0, sa=0):
    """MULT MULTU DIV DIVU (0, 0x18 .. 0x1B): generate_binary_arithmetic_hilo_op -- lo to register 32 on channel 2, hi to 33 on 3."""
    r = _row(m, CF.enc_r(0, rs, rt, rd, sa, {"MULT": 0x18, "MULTU": 0x19, "DIV": 0x1A, "DIVU": 0x1B}[name]))
    r[CF.OP["binary_op"]] = 1
    in0, in1 = m.reg_read(r, 0, rs), m.reg_read(r, 1, rt)
    lo, hi = result(name, in0, in1)
    m.reg_write(r, 2, REG_LO, lo)
    m.reg_write(r, 3, REG_HI, hi)
    _push(m, r, name, (FILTER[name], in0, in1))


def _mem(m, r, i, is_read, virt, value=None):
    """mem_read_gp_with_log_and_fill / mem_write_gp_log_and_fill at (the machine's context, Segment::Code, virt)."""
    ctx = getattr(m, "context", 0)
    if ctx == 0:
        return m.mem_read(r, i, virt) if is_read else m.mem_write(r, i, virt, value)
    key = (ctx, CF.SEG_CODE, virt)                          # (the Machine's own memory is context 0)
    if is_read:
        value = m.mem.setdefault(key, 0)
        m._cur["reads"].append(value)
    m.mem[key] = value
    m.channel(r, i, 1, is_read, CF.SEG_CODE, virt, value, ctx=ctx)
    return value


def sdc1(m, base, rt, offset):
    """SDC1 (opcode 0x3D): generate_mstore_general(MemOp::SDC1, rs, rt, offset) -- channels 0 and 1 read base and rt, channel 2 reads the
    word, the three bit decompositions, aux_filter = m_op_store * opcode_bits[5], is_sdc1, (aux_a, val) = (0, 0), channel 3 stores val."""
    r = _row(m, CF.enc_i(0x3D, base, rt, offset))
    r[CF.OP["m_op_store"]] = 1
    a, b = m.reg_read(r, 0, base), m.reg_read(r, 1, rt)
    raw = (a + CF.sext(offset, 16)) & MASK32
    virt = raw & 0xFFFFFFFC
    mem = _mem(m, r, 2, 1, virt)
    for i in range(32):
        r[CF.GEN + i], r[CF.GEN + 32 + i], r[CF.GEN + 64 + i] = (raw >> i) & 1, (b >> i) & 1, (mem >> i) & 1       # rs_le, rt_le, mem_le
    r[CF.MEMIO["aux_filter"]] = r[CF.OP["m_op_store"]] * r[CF.OPCODE_BITS + 5]
    r[CF.MEMIO["sdc1"]] = 1
    r[CF.GEN + 96] = 0                                      # aux_rs0_mul_rs1 = aux_a
    _mem(m, r, 3, 0, virt, 0)
    _push(m, r, "SDC1", None)


def nop_like(m, name, rs=0, rt=0, rd=0, sa=0, imm=0):
    """SYNC (0, 0x0F) and PREF (opcode 0x33): decode makes both Operation::Nop; generate_nop pushes the row with its op flag alone."""
    r = _row(m, CF.enc_r(0, rs, rt, rd, sa, 0x0F) if name == "SYNC" else CF.enc_i(0x33, rs, rt, imm))
    r[CF.OP["nop"]] = 1
    _push(m, r, name, None)


# ---------------------------------------------------------------- the recorder
class InsnRecorder(M.Recorder):
    """cpu_steps_model.Recorder on which the generators above record instead of pushing a step: .insns holds, per instruction, the
    ZKM_INSN_* record, the clock, the expected row, the mask and the arithmetic triple (None: nothing pushed).  .kernel, .context: the
    kernel flag and the context of the rows that follow; .clock_offset moves the clock of the rows that follow."""

    def __init__(self, *args, **kw):
        self.insns, self.kernel, self.context, self.clock_offset = [], 1, 0, 0
        super().__init__(*args, **kw)

    @property
    def clock(self):
        return len(self.rows) + self.clock_offset

    def push_insn(self, r, kind, arith):
        cur = self._cur
        reads = cur["reads"]
        assert len(reads) <= 6 and len([c for c in range(7, 40) if r[c]]) == 1
        mask = sum(1 << i for i in range(8) if r[CF.ch(i, 0)])
        self.insns.append({"record": (cur["pc"], cur["npc"], cur["insn"], KIND[kind], r[CF.KERNEL], r[CF.CONTEXT], reads + [0] * (6 - len(reads))),
                           "clock": r[CF.CLOCK], "row": [v % CF.P for v in r], "mask": mask, "arith": arith, "kind": kind})
        self.steps.append((0, 0, 0, M.KIND["RAW"], 0, 0, [0] * 6))          # the placeholder zkm_insn_rows_steps' record replaces
        CF.Machine.push(self, r)

    # ---- as the library takes and writes them
    def insn_lists(self):
        """(records, clocks): zkm_insn_rows_*'s two lists."""
        out = np.zeros(len(self.insns), dtype=M.STEP_DT)
        for k, x in enumerate(self.insns):
            out[k] = x["record"]
        return out, np.array([x["clock"] for x in self.insns], dtype=np.uint64)

    def insn_rows(self):
        return np.array([x["row"] for x in self.insns], dtype=np.uint64).reshape(-1, CF.W)

    def insn_masks(self):
        return [x["mask"] for x in self.insns]

    def insn_arith(self):
        return np.array([x["arith"] for x in self.insns if x["arith"] is not None], dtype=np.uint32).reshape(-1, 3)

    def insn_memory_ops(self):
        return sum(bin(x["mask"]).count("1") for x in self.insns)


def steps(m, raw_base):
    """The RAW records of an InsnRecorder's instruction rows as zkm_insn_rows_steps writes them: kind 28, reads[0] = raw_base + k,
    reads[1] = the mask, every other field 0."""
    out = np.zeros(len(m.insns), dtype=M.STEP_DT)
    out["kind"] = M.KIND["RAW"]
    out["reads"][:, 0] = raw_base + np.arange(len(m.insns))
    out["reads"][:, 1] = m.insn_masks()
    return out


def sample_insns(m):
    """Every one of the thirteen kinds between ordinary steps, on operands of both signs: products and quotients of negatives, the
    largest operands, register 0 as a destination, SDC1 at the four low-address-bit values through a negative offset (into the words the
    Machine's bootstrap wrote).  Every register is written before it is read."""
    for reg, v in {8: 0xFFFFFFF9, 9: 2, 10: 0x80000000, 11: 0xFFFFFFFF, 12: 0x7FFFFFFF, 13: 0x12345678, 22: 0x10C, REG_LO: 5, REG_HI: 6}.items():
        m.set_reg(reg, v)
    lui(m, 0, 16, 0x8000)
    lui(m, 0, 0, 0x8000)
    lui(m, 17, 18, 0x7FFF)
    m.binary("addu", 16, 18, 19, 0x21, lambda a, b: a + b)
    lui(m, 0, 16, 0xFFFF)
    lui(m, 0, 16, 0)
    binary(m, "MUL", 8, 9, 20)
    binary(m, "MUL", 10, 11, 0)
    binary(m, "MUL", 12, 12, 20, sa=3)
    for name, rs, rt in (("MULT", 8, 11), ("MULT", 10, 10), ("MULT", 12, 8), ("MULTU", 11, 11), ("MULTU", 12, 9)):
        hilo(m, name, rs, rt)
        binary(m, "MFHI", rd=21)
        binary(m, "MFLO", rd=23)
    m.logic("xor", 21, 23, 19)
    binary(m, "MFHI", rd=0)
    binary(m, "MFLO", rd=0, rs=5, rt=6)                     # (the free fields go into the row's bits)
    for name, rs, rt in (("DIV", 8, 9), ("DIV", 9, 8), ("DIV", 8, 8), ("DIV", 10, 9), ("DIV", 12, 11), ("DIVU", 11, 9), ("DIVU", 9, 11), ("DIVU", 10, 12)):
        hilo(m, name, rs, rt, rd=7)
        binary(m, "MFLO", rd=24)
    binary(m, "MTHI", rs=13)
    binary(m, "MTLO", rs=12)
    binary(m, "MFHI", rd=24)
    binary(m, "MFLO", rd=25)
    m.shift_imm("sll", 24, 25, 4)
    nop_like(m, "SYNC")
    nop_like(m, "SYNC", rs=1, rt=2, rd=3, sa=4)
    nop_like(m, "PREF", rs=22, rt=1, imm=0x8010)
    for offset in (0xFFF4, 0xFFF5, 0xFFFA, 0xFFFF):         # 0x10C - 12, - 11, - 6, - 1
        sdc1(m, 22, 13, offset)
    m.load("lw", 22, 23, 0xFFF4)                            # reads the 0 the first SDC1 stored
    m.nop()
    return m


def arith_flags(m):
    """(row filter, in0, in1) of every arithmetic operation of a Machine run with these instructions, as the segment's joined list
    holds them: the step kinds' operations first, the instructions' behind."""
    own = [(M.ARITH_FLAG[name], a, b) for name, a, b, _, _ in m.arith_ops]
    return own + [x["arith"] for x in getattr(m, "insns", []) if x["arith"] is not None]
