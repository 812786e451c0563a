"""CPU suite: the compact step log (include/zkm_hip.h zkm_cpu_step) on the host -- the recorded sample program against the Machine's own
list lengths through zkm_cpu_steps_counts, every refusal of the host walk with the step it names, and the refusals of the *_steps
calls that need no device."""
import ctypes as C

import numpy as np
import pytest

from . import cpu_steps_model as M


def test_sample_program_counts_equal_the_machines_lists(zkm):
    m = M.sample()
    assert len(m.rows) == 252 and len(m.steps) == 252 and m.first_clock == 0
    assert [s[3] for s in m.steps[:2]] == [M.KIND["RAW"]] * 2      # the two bootstrap rows; the other 250 went through push
    assert m.max_reads == 5
    assert (len(m.mem_ops), len(m.logic_ops), len(m.arith_ops)) == (598, 4, 9)
    assert zkm.cpu_steps_counts(m.cpu_steps(zkm)) == (598, 4, 9)
    twice = M.sample(2)
    assert zkm.cpu_steps_counts(twice.cpu_steps(zkm)) == (len(twice.mem_ops), len(twice.logic_ops), len(twice.arith_ops))
    # PAD steps push nothing; the kinds and ZKM_STEP_* agree
    twice_padded = np.concatenate([twice.step_array(), np.zeros(3, dtype=M.STEP_DT)])
    twice_padded["kind"][-3:] = M.KIND["PAD"]
    assert zkm.cpu_steps_counts(zkm.CpuSteps(twice_padded, twice.raw_array())) == (len(twice.mem_ops), len(twice.logic_ops), len(twice.arith_ops))
    assert M.KINDS == zkm.STEP_KINDS and M.STEP_DT == zkm.CPU_STEP_DT
    header = open(zkm.__file__.replace("zkm_amd/__init__.py", "include/zkm_hip.h")).read()
    for name, k in M.KIND.items():
        assert "#define ZKM_STEP_%s %d\n" % (name, k) in header


def step(kind, insn=0, reads=(), flags=1, pc=0x1000):
    s = np.zeros(1, dtype=M.STEP_DT)
    s["pc"], s["next_pc"], s["insn"], s["kind"], s["flags"] = pc, pc + 4, insn, M.KIND[kind] if isinstance(kind, str) else kind, flags
    s["reads"][0, :len(reads)] = reads
    return s


REFUSED = [
    ("unknown kind 29", step(29)),
    ("unknown kind 4000000000", step(4000000000)),
    ("BINARY_OP does not take the encoding 0x00000018", step("BINARY_OP", 0x18, (1, 2))),                 # MULT
    ("BINARY_IMM_OP does not take the encoding 0x3c010001", step("BINARY_IMM_OP", 0x3C010001, (1,))),    # LUI
    ("LOGIC_OP does not take the encoding", step("LOGIC_OP", 0x21, (1, 2))),
    ("LOGIC_IMM_OP does not take the encoding", step("LOGIC_IMM_OP", 0x0F << 26, (1,))),                   # LUI
    ("SHIFT_IMM does not take the encoding", step("SHIFT_IMM", (1 << 21) | 2, (1, 2))),                  # ROTR is ROR's
    ("BRANCH does not take the encoding", step("BRANCH", (1 << 26) | (2 << 16), (0, 0))),                # REGIMM rt = 2
    ("BRANCH does not take the encoding", step("BRANCH", 4 << 26, (0, 0), flags=3)),                     # BEQ reads rt itself
    ("JUMPDIRECT does not take the encoding", step("JUMPDIRECT", (1 << 26) | (0x10 << 16))),
    ("M_OP_LOAD does not take the encoding", step("M_OP_LOAD", 0x2B << 26, (0, 0, 0))),                  # SW
    ("M_OP_STORE does not take the encoding", step("M_OP_STORE", 0x23 << 26, (0, 0, 0))),                # LW
    ("NOP does not take the encoding", step("NOP", 1 << 6)),
    ("EXT does not take the encoding", step("EXT", (0x1F << 26) | (20 << 11) | (20 << 6), (5,))),        # lsb + size > 32
    ("INS does not take the encoding", step("INS", (0x1F << 26) | (3 << 11) | (9 << 6) | 4, (5, 6))),    # msb < lsb
    ("TEQ does not take these operands", step("TEQ", 0x34, (7, 7))),
    ("SYSCALL does not take the encoding 0x0000000c with flags 0x00000401", step("SYSCALL", 0xC, (0, 0, 0, 0), flags=1 | 4 << 8)),
    ("SYSCALL does not take the encoding", step("SYSCALL", 0xD, (0, 0, 0, 0))),
    ("RAW index 2, raw_rows holds 2", step("RAW", 0, (2, 0))),
    ("RAW does not take the encoding 0x00000000 with the channel mask 0x00000100", step("RAW", 0, (1, 0x100))),
]


@pytest.mark.parametrize("message,bad", REFUSED, ids=[m.split(" does")[0].split(",")[0] for m, _ in REFUSED])
def test_every_refusal_names_its_step(zkm, message, bad):
    good = M.sample().step_array()[10:15]        # addu, subu, addiu, and, or: all accepted
    raw = np.zeros((2, 259), dtype=np.uint64)
    assert (good["kind"] != M.KIND["RAW"]).all()
    steps = np.concatenate([good, bad, good])
    with pytest.raises(zkm.ZkmError, match=r"zkm_cpu_steps_counts: step %d: .*%s" % (len(good), message.replace("(", r"\("))):
        zkm.cpu_steps_counts(zkm.CpuSteps(steps, raw))
    assert zkm.cpu_steps_counts(zkm.CpuSteps(np.concatenate([good, good]), raw))[0] >= 0


def test_a_raw_mask_that_is_not_its_host_rows_is_refused(zkm):
    m = M.sample()
    steps, raw = m.step_array()[:4].copy(), m.raw_array()
    assert steps["reads"][0, 1] == 0b111 and steps["reads"][1, 1] == 0      # the bootstrap row that writes three words, the one that writes none
    assert zkm.cpu_steps_counts(zkm.CpuSteps(steps, raw))[0] == 5
    for at, mask in ((0, 0b011), (1, 0b1), (2, 0)):
        bad = steps.copy()
        bad["reads"][at, 1] = mask
        with pytest.raises(zkm.ZkmError, match=r"step %d: RAW row %d uses the channels 0x%08x, the step's mask is 0x%08x" % (at, at, steps["reads"][at, 1], mask)):
            zkm.cpu_steps_counts(zkm.CpuSteps(bad, raw))


def test_null_pointers_with_nonzero_counts(zkm):
    L = zkm.load()
    for st in (zkm.CpuStepsStruct(None, 3, None, 0), zkm.CpuStepsStruct(None, 0, None, 2)):
        err = C.c_char_p()
        assert L.zkm_cpu_steps_counts(C.byref(st), None, None, None, C.byref(err)) == 1
        assert b"zkm_cpu_steps_counts: null pointer with a nonzero count" in err.value
    err = C.c_char_p()
    assert L.zkm_cpu_steps_counts(None, None, None, None, C.byref(err)) == 1 and b"null argument" in err.value
    n = [C.c_size_t(7) for _ in range(3)]
    empty = zkm.CpuStepsStruct(None, 0, None, 0)
    assert L.zkm_cpu_steps_counts(C.byref(empty), *[C.byref(x) for x in n], None) == 0 and [x.value for x in n] == [0, 0, 0]
    assert L.zkm_cpu_witness(None, C.byref(empty), 0, 4, None, None, None, None, C.byref(err)) == 1 and b"zkm_cpu_witness: null argument" in err.value


def steps_calls(zkm, steps_list, ops_list):
    """Both *_steps calls without a context: the host's refusals come before the missing context's."""
    L = zkm.load()
    cfg = zkm.StarkConfig()
    L.zkm_standard_config(C.byref(cfg))
    K = len(ops_list)
    sl = (zkm.CpuStepsStruct * K)(*[s.struct() for s in steps_list])
    st = (zkm.SegmentOpsStruct * K)(*[o.struct() for o in ops_list])
    lg, offs = (C.c_uint * (12 * K))(), (C.c_size_t * (13 * K))()
    out = []
    for call in (lambda e: L.zkm_segments_tables_steps(None, C.byref(cfg), K, None, sl, st, lg, None, e),
                 lambda e: L.zkm_prove_segments_ops_steps(None, C.byref(cfg), K, None, sl, st, None, None, None, offs, None, e)):
        err = C.c_char_p()
        assert call(C.byref(err)) == 1
        out.append(err.value.decode())
    return out


def test_steps_calls_refuse_on_the_host(zkm):
    m = M.sample()
    good = m.cpu_steps(zkm)                                     # 252 steps: not a power of two
    four = zkm.CpuSteps(m.step_array()[:4], m.raw_array())      # the two bootstrap rows and two register writes: RAW steps
    none = zkm.SegmentOps(None, None)
    rows = zkm.SegmentOps(np.zeros((4, 259), dtype=np.uint64), None)
    for name, msg in zip(("zkm_segments_tables_steps", "zkm_prove_segments_ops_steps"), steps_calls(zkm, [four, four], [none, rows])):
        assert msg == name + ": segment 1: Cpu: cpu_rows must be NULL with ncpu_rows 0: the steps take their place"
    for name, msg in zip(("zkm_segments_tables_steps", "zkm_prove_segments_ops_steps"), steps_calls(zkm, [four, good], [none, none])):
        assert msg == name + ": segment 1: Cpu: 252 rows: not a power of two of at most 2^28"
    bad = m.step_array()[:4].copy()
    bad["kind"][2] = 77
    for name, msg in zip(("zkm_segments_tables_steps", "zkm_prove_segments_ops_steps"),
                         steps_calls(zkm, [zkm.CpuSteps(bad, m.raw_array())], [none])):
        assert msg == name + ": segment 0: Cpu: step 2: unknown kind 77"
    # nothing to refuse: the missing context is what is left
    for name, msg in zip(("zkm_segments_tables_steps", "zkm_prove_segments_ops_steps"), steps_calls(zkm, [four], [none])):
        assert msg == name + ": null argument"
