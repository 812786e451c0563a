"""CPU suite: the model of the SHA-256 precompile calls (tests/sha_calls_model.py) held against judges it did not write -- the sponge
fixtures of tests/logic_fixtures.py, which read the memory operations, logic operations and ShaExtend rows off the ORACLE's sponge tables,
and the oracle's CPU constraints on a Machine run with one call of each kind spliced in."""
import numpy as np

from zkm_amd import tables as T

from . import cpu_fixtures as CF
from . import cpu_steps_model as M
from . import logic_fixtures as LF
from . import sha_calls_model as S


def sorted_ops(ops):
    return sorted(tuple(int(v) for v in op) for op in ops)


def test_extend_lists_equal_the_sponge_fixtures(oracle):
    _, _, (w16, meta, inputs, ts, ops, mem_ops) = LF.build_sha_extend_path(oracle, nblocks=2, ts=lambda n: 10 * (5 + 200 * np.arange(n, dtype=np.uint64)))
    x = S.expand(extend=(w16, meta))
    rows, mem, logic, ext_in, ext_ts = x.arrays()
    assert rows.shape == (192, 259) and mem.shape == (1536, 6) and logic.shape == (384, 3) and len(ext_ts) == 96
    assert (mem == mem_ops).all()
    assert (ext_in == inputs).all() and (ext_ts == ts).all()
    assert sorted_ops(logic) == sorted_ops(ops)                  # (the fixtures shuffle)
    assert x.masks == [0x1F, 0] * 96


def test_compress_lists_equal_the_sponge_fixtures(oracle):
    _, _, (hx, w, meta, ops, mem_ops) = LF.build_sha_compress_path(oracle, ncomp=2, ts=lambda n: 10 * (30 + 40 * np.arange(n, dtype=np.uint64)))
    x = S.expand(compress=(hx, w, meta))
    rows, mem, logic, ext_in, ext_ts = x.arrays()
    assert rows.shape == (22, 259) and mem.shape == (576, 6) and logic.shape == (1536, 3) and len(ext_in) == 0 and len(ext_ts) == 0
    assert (mem == mem_ops).all()
    assert sorted_ops(logic) == sorted_ops(ops)
    assert x.masks == ([0xFF] * 9 + [0, 0xFF]) * 2
    assert x.clocks[:11] == list(range(30 - 9, 30 + 2))


def machine_with_calls(seed=5):
    """The sample program with a SYSCALL row and an extend call, then a SYSCALL row and a compress call, spliced in behind it; padded."""
    rng = np.random.default_rng(seed)
    m = M.Recorder()
    CF.sample_program(m)
    calls = S.CallRecorder(m)
    for kind in ("extend", "compress"):
        for reg, v in ((4, 0x20000), (5, 0x30000), (6, 0x40), (37, 0x40000000)):
            m.set_reg(reg, v)
        m.syscall("other")
        if kind == "extend":
            calls.sha_extend(0x20000, rng.integers(0, 1 << 32, 16))
        else:
            calls.sha_compress(0x20000, 0x30000, rng.integers(0, 1 << 32, 8), rng.integers(0, 1 << 32, 64))
        m.nop()
    return m, calls


def test_model_rows_pass_the_oracles_cpu_constraints(oracle):
    m, calls = machine_with_calls()
    x = calls.finish()
    assert len(x.rows) == 107
    log_n = len(m.rows).bit_length()
    m.pad((1 << log_n) - len(m.rows))
    trace = m.trace(log_n)
    count, bad = oracle.debug_constraints(T.TABLE_CPU, trace, 259, log_n)
    assert count == 741 and bad is None, bad
    cols = trace.reshape(259, -1)
    assert cols[S.IS_SHA_EXTEND_SPONGE].sum() == 48 and cols[S.IS_SHA_COMPRESS_SPONGE].sum() == 1
    assert (cols[CF.CLOCK] == np.arange(1 << log_n)).all()      # every call row sits at its clock
    # the rows are live under the constraints: a read row whose channel 0 is used "twice" is refused at that row
    at = x.clocks[0]
    cols[CF.ch(0, 0), at] = 2
    assert oracle.debug_constraints(T.TABLE_CPU, cols.reshape(-1), 259, log_n)[1][0] == at
