"""The compact step log of a cpu_fixtures.Machine run (test infrastructure): a recorder that emits one zkm_cpu_step per row the Machine
pushes -- pc, next_pc, the instruction word, the kind of its op flag and the values it read through the memory channels, in the order
it read them -- beside the rows, memory, logic and arithmetic operations the Machine itself produces.  The Machine's outputs are the
expected values of everything the device builds from the steps.

RAW steps (a ready-made row): the bootstrap rows of the plain Machine and `set_reg`.  `logic_imm` adds the one op flag class of the
step kinds that the Machine has no method for.  A BGEZ whose channel 1 names register 0 carries
flag bit 1.  The recorder is a mixin, so that it also records a boot_fixtures.BootMachine."""
import numpy as np

from . import arith_fixtures as A
from . import cpu_fixtures as CF

P = CF.P
KINDS = ("BINARY_OP", "BINARY_IMM_OP", "LOGIC_OP", "LOGIC_IMM_OP", "SHIFT", "SHIFT_IMM", "BRANCH", "JUMPS", "JUMPI", "JUMPDIRECT", "M_OP_LOAD",
         "M_OP_STORE", "NOP", "CLZ_OP", "CLO_OP", "SIGNEXT8", "SIGNEXT16", "SWAPHALF", "RDHWR", "MOVZ_OP", "MOVN_OP", "TEQ", "EXT", "INS", "ROR",
         "MADDU", "SYSCALL", "PAD", "RAW")
KIND = {name: k for k, name in enumerate(KINDS)}
STEP_DT = np.dtype([("pc", "<u4"), ("next_pc", "<u4"), ("insn", "<u4"), ("kind", "<u4"), ("flags", "<u4"), ("context", "<u4"), ("reads", "<u4", (6,))])
ARITH_FLAG = {"add": A.IS_ADD, "addu": A.IS_ADDU, "addi": A.IS_ADDI, "addiu": A.IS_ADDIU, "sub": A.IS_SUB, "subu": A.IS_SUBU, "sllv": A.IS_SLLV,
              "srlv": A.IS_SRLV, "srav": A.IS_SRAV, "sll": A.IS_SLL, "srl": A.IS_SRL, "sra": A.IS_SRA, "slt": A.IS_SLT, "sltu": A.IS_SLTU,
              "slti": A.IS_SLTI, "sltiu": A.IS_SLTIU}
LOGIC_CODE = {"and": 0, "or": 1, "xor": 2, "nor": 3}


class StepRecorder:
    """Mixin in front of a cpu_fixtures.Machine: .steps is the step list of the rows pushed so far, .raw_rows the rows of its RAW steps.
    raw_boot: the rows that exist once the Machine is constructed (its bootstrap) are recorded as RAW steps; False leaves them out (they
    come from a boot image)."""

    def __init__(self, *args, raw_boot=True, **kw):
        self.steps, self.raw_rows, self.max_reads = [], [], 0
        self._cur, self._force_raw = None, False
        super().__init__(*args, **kw)
        self.first_clock = 0 if raw_boot else len(self.rows)
        if raw_boot:
            for r in self.rows:
                self._emit_raw(r, r[CF.PC], r[CF.NEXT_PC])

    # ---- what a row read, in order
    def new_row(self, insn=None):
        self._cur = {"insn": insn or 0, "pc": self.pc, "npc": self.npc, "reads": [], "regs": {}}
        return super().new_row(insn)

    def reg_read(self, r, i, reg):
        v = super().reg_read(r, i, reg)
        self._cur["reads"].append(v)
        self._cur["regs"][i] = reg
        return v

    def mem_read(self, r, i, virt, seg=CF.SEG_CODE):
        v = super().mem_read(r, i, virt, seg)
        self._cur["reads"].append(v)
        return v

    def set_reg(self, reg, value):
        self._force_raw = True
        super().set_reg(reg, value)

    # ---- one step per pushed row
    def _emit_raw(self, r, pc, npc):
        mask = sum(1 << i for i in range(8) if r[CF.ch(i, 0)])
        self.steps.append((pc, npc, 0, KIND["RAW"], 0, 0, [len(self.raw_rows), mask, 0, 0, 0, 0]))
        self.raw_rows.append([v % P for v in r])

    def push(self, r, target=None):
        cur, raw = self._cur, self._force_raw
        self._force_raw = False
        flags = [c for c in range(7, 40) if r[c]]
        assert len(flags) == 1, flags
        name = CF.OPS[flags[0] - 7]
        r0 = name == "branch" and cur["regs"][1] != (cur["insn"] >> 16) & 31
        assert not r0 or cur["regs"][1] == 0
        if raw:
            self._emit_raw(r, cur["pc"], cur["npc"])
        else:
            sub = 0
            if name == "syscall":
                hit = [k for k in range(1, 9) if r[CF.GEN + 12 + k]]
                assert len(hit) <= 1
                sub = hit[0] if hit else 0
            reads = cur["reads"]
            assert len(reads) <= 6
            self.max_reads = max(self.max_reads, len(reads))
            self.steps.append((cur["pc"], cur["npc"], cur["insn"], KIND[name.upper()], r[CF.KERNEL] | (2 if r0 else 0) | (sub << 8), 0, reads + [0] * (6 - len(reads))))
        super().push(r, target)

    # ---- outputs
    def pad(self, count):
        """`count` PAD steps and the rows simulate_cpu appends for them (generation/mod.rs:170-185): clock, context, pc, next_pc and
        is_exit_kernel = 1, nothing else."""
        for _ in range(count):
            r = [0] * CF.W
            r[CF.CLOCK], r[CF.CONTEXT], r[CF.PC], r[CF.NEXT_PC], r[CF.IS_EXIT] = self.clock, 0, self.pc, self.npc, 1
            self.steps.append((self.pc, self.npc, 0, KIND["PAD"], 0, 0, [0] * 6))
            self.rows.append(r)

    def step_array(self):
        out = np.zeros(len(self.steps), dtype=STEP_DT)
        for k, (pc, npc, insn, kind, flags, context, reads) in enumerate(self.steps):
            out[k] = (pc, npc, insn, kind, flags, context, reads)
        return out

    def raw_array(self):
        return np.array(self.raw_rows, dtype=np.uint64).reshape(-1, CF.W)

    def cpu_steps(self, zkm):
        return zkm.CpuSteps(self.step_array(), self.raw_array())


class Recorder(StepRecorder, CF.Machine):
    pass


def logic_imm(m, name, rs, rt, imm):
    """ANDI / ORI / XORI, which cpu_fixtures.Machine leaves out, restated from generate_binary_logic_imm_op (witness/operation.rs:260-284,
    called with (op, rs, rt, insn & 0xffff), transition.rs:280-282, 409-411): channel 0 reads rs, channel 2 writes rt, the immediate is
    zero-extended, and no logic operation is pushed (the reference's push_logic is commented out)."""
    op = {"andi": 0x0C, "ori": 0x0D, "xori": 0x0E}[name]
    r = m.new_row(CF.enc_i(op, rs, rt, imm))
    r[CF.OP["logic_imm_op"]] = 1
    a = m.reg_read(r, 0, rs)
    imm &= 0xFFFF
    m.reg_write(r, 2, rt, {"andi": a & imm, "ori": a | imm, "xori": a ^ imm}[name])
    m.push(r)


def expected_lists(m, mem_from=0):
    """The Machine's three lists as the device writes them: memory n x 6 uint64 {context, segment, virt, timestamp, is_read, value},
    logic and arithmetic n x 3 uint32 {op, in0, in1}."""
    mem = np.array([(ctx, seg, virt, ts, is_read, value) for is_read, ctx, seg, virt, value, ts in m.mem_ops[mem_from:]], dtype=np.uint64).reshape(-1, 6)
    logic = np.array([(LOGIC_CODE[name], a, b) for name, a, b, _ in m.logic_ops], dtype=np.uint32).reshape(-1, 3)
    arith = np.array([(ARITH_FLAG[name], a, b) for name, a, b, _, _ in m.arith_ops], dtype=np.uint32).reshape(-1, 3)
    return mem, logic, arith


def rows_array(rows):
    """Machine rows as an n x 259 uint64 array (canonical)."""
    return np.array([[v % P for v in r] for r in rows], dtype=np.uint64).reshape(-1, CF.W)


_SAMPLE = {}


def sample(repeat=1):
    """The sample program recorded `repeat` times over, built once per process and not to be changed."""
    if repeat not in _SAMPLE:
        m = Recorder()
        for _ in range(repeat):
            CF.sample_program(m)
        _SAMPLE[repeat] = m
    return _SAMPLE[repeat]


def extra_program(m):
    """Operand cases the sample program leaves out: signed and unsigned compares in registers and immediates, overflowing adds, every
    branch kind taken and not taken on operands of both signs, writes to register 0, a jump and link that discards its link."""
    vals = {8: 0x7FFFFFFF, 9: 0x80000001, 10: 5, 11: 0xFFFFFFFB, 12: 5, 13: 0}
    for reg, v in vals.items():
        m.set_reg(reg, v)
    for name, func, fn in (("add", 0x20, lambda a, b: a + b), ("sub", 0x22, lambda a, b: a - b),
                           ("slt", 0x2A, lambda a, b: int(a - (a >> 31 << 32) < b - (b >> 31 << 32))), ("sltu", 0x2B, lambda a, b: int(a < b))):
        for rs, rt in ((8, 9), (9, 8), (10, 11), (11, 10), (10, 12)):
            m.binary(name, rs, rt, 16, func, fn)
    for name, op, fn in (("addi", 8, lambda a, b: a + b), ("slti", 0xA, lambda a, b: int(a - (a >> 31 << 32) < b - (b >> 31 << 32))),
                         ("sltiu", 0xB, lambda a, b: int(a < b))):
        for rs, imm in ((8, 1), (9, 0xFFFF), (10, 5), (11, 0x8000), (10, 6)):
            m.binary_imm(name, op, rs, 17, imm, fn)
    m.binary("addu", 8, 9, 0, 0x21, lambda a, b: a + b)            # writes to register 0: the channel is filled, nothing is pushed
    m.binary_imm("addiu", 9, 8, 0, 0x1234, lambda a, b: a + b)
    m.logic("xor", 8, 9, 0)
    m.load("lw", 13, 0, 0x100)
    m.jr(13, rd=0)
    m.nop()
    for kind, pairs in (("eq", ((8, 8), (8, 9), (10, 12))), ("ne", ((8, 8), (8, 9), (11, 10))), ("le", ((9, 0), (13, 0), (10, 0), (8, 0))),
                        ("gt", ((9, 0), (13, 0), (10, 0))), ("lt", ((9, 0), (13, 0), (10, 0), (11, 0))), ("ge", ((9, 0), (13, 0), (8, 0)))):
        for rs, rt in pairs:
            m.branch(kind, rs, rt, 0x7FFF if rs != 9 else 0x8000)
            m.nop()
    return m
