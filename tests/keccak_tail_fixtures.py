"""Lists and segments with SYSKECCAK calls of any length for tests/test_keccak_tail_abi.py and tests/test_gpu_keccak_tail.py: built once,
shared, not to be changed.  The expectations come from tests/keccak_tail_model.py."""
import numpy as np

from . import cpu_fixtures as CF
from . import cpu_steps_model as M
from . import keccak_calls_model as K
from . import keccak_tail_model as TM

FLAG, TAIL = TM.FLAG, TM.TAIL
SEGMENT_LENGTHS = (35, 135, 137, 1)


def calls(lengths, flags=None, seed=1):
    """One call per length at disjoint addresses and clocks, as (inputs, off, meta, digest_addrs).  flags[k]: whether call k carries
    ZKM_SPONGE_PADDED_TAIL (default: the calls whose length is no multiple of 4).  The bytes of the call behind a call whose length is
    no multiple of 4 begin with 0xFF: a kernel that reads the rest of the last word from the input shows a wrong word."""
    rng = np.random.default_rng(seed)
    out = []
    for k, L in enumerate(lengths):
        data = bytearray(rng.integers(0, 256, L, dtype=np.uint8).tobytes())
        if k and lengths[k - 1] % 4:
            data[:4] = b"\xff" * min(4, L)
        tail = TAIL if (flags[k] if flags is not None else L % 4) else 0
        out.append((bytes(data), (0, 0, (0x10000 + 0x1000 * k) | FLAG | tail, 10 * (40 + 50 * k)), 0x80000 + 0x40 * k))
    return K.lists(out)


_BUILT = {}


def all_lengths():
    """(lists, the model's five arrays) for TM.LENGTHS in one list."""
    if "all" not in _BUILT:
        lists = calls(TM.LENGTHS)
        _BUILT["all"] = (lists, TM.expand(*lists).arrays())
    return _BUILT["all"]


def program_with_calls(m, lengths=SEGMENT_LENGTHS, seed=11):
    """The sample program, then a SYSCALL row and a Keccak call per length, each spliced in at its clocks (as
    tests/test_gpu_keccak_calls.py's program_with_calls, with the recorder for any length)."""
    rng = np.random.default_rng(seed)
    CF.sample_program(m)
    rec = TM.CallRecorder(m)
    for k, L in enumerate(lengths):
        addr, ptr = 0x50000 + 0x1000 * k, 0x60000 + 0x40 * k
        for reg, v in ((4, addr), (5, L), (6, ptr), (37, 0x40000000)):
            m.set_reg(reg, v)
        m.syscall("other")
        rec.keccak(addr, rng.integers(0, 256, L, dtype=np.uint8).tobytes(), ptr)
        m.nop()
    return rec


def zero_extended(data):
    """The words a call would read if its last memory word held the remaining bytes and zeros -- no padding."""
    words = TM.runtime_words(data)
    if len(data) % 4:
        words[-1] = K.be(bytes(data[len(data) // 4 * 4:]) + bytes(4 - len(data) % 4))
    return words


def segment(zkm, name="tail"):
    """A recorded segment with calls of SEGMENT_LENGTHS: {"kw": what zkm.SegmentCalls takes, "host": (CpuSteps, SegmentOps) with the model's
    rows and lists in numpy arrays, "log_n", "model": the Keccak Expansion}.  "zero-extended": the same, the host-expanded read rows
    holding the zero-extended last word (the sponge's reads carry the padded word whatever memory holds: util.rs:515-519)."""
    if name not in _BUILT:
        m = M.Recorder()
        rec = program_with_calls(m)
        memories = [zero_extended(d) for d, _, _ in rec.keccaks] if name == "zero-extended" else None
        sx, kx = rec.finish(memories=memories)
        log_n = int(len(m.rows)).bit_length()
        m.pad((1 << log_n) - len(m.rows))
        k = rec.keccak_lists()
        steps = m.cpu_steps(zkm)
        krows, kmem, klogic, perm_in, perm_ts = kx.arrays()
        patched = steps.steps.copy()
        records, clocks = K.steps(kx, raw_base=steps.nraw)
        patched[clocks.astype(np.int64) - m.first_clock] = records
        host = (zkm.CpuSteps(patched, np.concatenate([steps.raw_rows.reshape(-1, 259), krows])),
                zkm.SegmentOps(None, kmem, logic_ops=klogic, keccak=(perm_in, perm_ts), keccak_sponge=k[:3]))
        kw = dict(steps=steps, first_clock=m.first_clock, extend=None, compress=None, keccak=k, io=None, insns=None)
        _BUILT[name] = {"kw": kw, "host": host, "log_n": log_n, "model": kx}
    return _BUILT[name]


def plain_segment(zkm, log_n=8):
    """A step log without calls, of another height."""
    if ("plain", log_n) not in _BUILT:
        m = M.Recorder()
        CF.sample_program(m)
        m.pad((1 << log_n) - len(m.rows))
        kw = dict(steps=m.cpu_steps(zkm), first_clock=m.first_clock, extend=None, compress=None, keccak=None, io=None, insns=None)
        _BUILT["plain", log_n] = {"kw": kw, "host": (m.cpu_steps(zkm), zkm.SegmentOps(None, None)), "log_n": log_n}
    return _BUILT["plain", log_n]
