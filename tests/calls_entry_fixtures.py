"""Segments with calls of several kinds for the suites of the one-entry expansion (tests/test_calls_entry_abi.py,
tests/test_gpu_calls_entry.py): recorded with the Recorders and CallRecorders the per-kind suites use, each at most 2^8 CPU rows.  A
segment is a dict: "kw" -- the arguments Context.calls_expand and zkm.SegmentCalls both take; "m" the Machine; "models" the three
Expansions (SHA, Keccak, I/O) whose rows the calls' clocks were taken from."""
import numpy as np

from . import cpu_fixtures as CF
from . import cpu_steps_model as M
from . import insn_rows_model as I
from . import io_calls_model as IO
from . import sha_calls_model as S

MAP = IO.PREIMAGE_MAP
INSN_OPS = (lambda m: I.binary(m, "MUL", 8, 9, 16), lambda m: I.nop_like(m, "SYNC"), lambda m: I.lui(m, 0, 17, 0x9234), lambda m: I.sdc1(m, 22, 8, 0xFFF4),
            lambda m: I.hilo(m, "DIV", 8, 9), lambda m: I.nop_like(m, "PREF", rs=22), lambda m: I.binary(m, "MFHI", rd=18))


def record(zkm, m, io=("hint_read", "commit", "verify", "preimage"), hint_len=37, keccak=True, compress=True, extend=False, ninsns=0, seed=11,
           program=None):
    """Record on the Machine m (an InsnRecorder when ninsns > 0): the I/O calls named, each behind a SYSCALL row with its argument registers
    loaded (the hint read, hint_len bytes, comes first and the commit reads what it wrote); a Keccak call of 140 bytes; a SHA compress
    call; a SHA extend call; ninsns instruction records cycling through pushing and non-pushing kinds -- all behind `program`, if
    given.  Padded to a power of two."""
    rng = np.random.default_rng(seed)
    if program:
        program(m)
    rec = IO.CallRecorder(m)
    vec = rng.integers(0, 256, hint_len, dtype=np.uint8).tobytes()
    data = {"hint_read": (0x50000, vec), "commit": (0x50000, vec[:len(vec) // 4 * 4]), "verify": (0x51000, rng.integers(0, 256, 32, dtype=np.uint8).tobytes()),
            "preimage": (MAP, rng.integers(0, 256, 32 + 61, dtype=np.uint8).tobytes())}

    def syscall(a0, a1, a2):
        for reg, v in ((4, a0), (5, a1), (6, a2), (37, 0x40000000)):
            m.set_reg(reg, v)
        m.syscall("other")
    for kind in io:
        addr, bytes_ = data[kind]
        syscall(addr, len(bytes_), 0x30000)
        rec.io(kind, addr, bytes_)
        m.nop()
    if keccak:
        syscall(0x52000, 140, 0x60000)
        rec.keccak(0x52000, rng.integers(0, 256, 140, dtype=np.uint8).tobytes(), 0x60000)
        m.nop()
    w16 = [int(x) for x in rng.integers(0, 1 << 32, 16)]
    if compress:
        syscall(0x20000, 0x30000, 0x40)
        rec.sha_compress(0x20000, 0x30000, [int(x) for x in rng.integers(0, 1 << 32, 8)], S.Expansion().extend(w16, (0, 0, 0x20000, 10)))
        m.nop()
    if extend:
        syscall(0x20000, 0x30000, 0x40)
        rec.sha_extend(0x20000, w16)
        m.nop()
    if ninsns:
        for reg, v in {8: 0xFFFFFFF9, 9: 2, 22: 0x10C, I.REG_LO: 5, I.REG_HI: 6}.items():
            m.set_reg(reg, v)
        for k in range(ninsns):
            INSN_OPS[k % len(INSN_OPS)](m)
        m.nop()
    models = rec.finish()
    log_n = int(len(m.rows)).bit_length()
    m.pad((1 << log_n) - len(m.rows))
    assert log_n <= 8 or m.first_clock, "a segment of the suite is at most 2^8 CPU rows"
    e, c = rec.lists()
    kw = dict(steps=m.cpu_steps(zkm), first_clock=m.first_clock, extend=e, compress=c, keccak=rec.keccak_lists() if keccak else None,
              io=rec.io_lists() if io else None, insns=m.insn_lists() if ninsns else None)
    return {"kw": kw, "m": m, "models": models, "log_n": log_n}


def own_operations(seed=5):
    """Operations of the segment's own for every list the calls append to (any words: the expansion copies them)."""
    rng = np.random.default_rng(seed)
    return dict(memory_ops=rng.integers(0, 1 << 32, (5, 6), dtype=np.uint64), logic_ops=rng.integers(0, 1 << 32, (3, 3), dtype=np.uint32),
                arithmetic_ops=np.array([(1, 5, 6), (8, 3, 4)], dtype=np.uint32),
                keccak_perms=(rng.integers(0, 1 << 63, (2, 25), dtype=np.uint64), np.array([70, 80], dtype=np.uint64)))


_BUILT = {}


def segment(zkm, name):
    """The suite's segments, built once and not to be changed:
      all        one call of every kind (the four I/O kinds, Keccak, SHA compress and extend) and 19 instruction records
      io-long    I/O alone, its hint read 300 bytes: ten rows, more than the eight of one I/O workgroup
      plain      no calls at all: cpu_fixtures' sample program
      four       all four kinds (no SHA extend: its 96 rows) with 19 instruction records: more than 16, and no multiple of 16
      two        two calls: a hint read and a Keccak call"""
    if name not in _BUILT:
        if name == "all":
            s = record(zkm, I.InsnRecorder(), extend=True, ninsns=19)
        elif name == "io-long":
            s = record(zkm, M.Recorder(), hint_len=300, keccak=False, compress=False, seed=12)
        elif name == "plain":
            s = record(zkm, M.Recorder(), io=(), keccak=False, compress=False, seed=13, program=CF.sample_program)
        elif name == "four":
            s = record(zkm, I.InsnRecorder(), ninsns=19, seed=14)
        else:
            assert name == "two"
            s = record(zkm, M.Recorder(), io=("hint_read",), compress=False, seed=15)
        _BUILT[name] = s
    return _BUILT[name]
