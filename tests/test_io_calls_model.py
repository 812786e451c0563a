"""CPU suite: the model of the I/O syscalls' rows (tests/io_calls_model.py) held against judges it did not write -- rows computed by hand
from the reference's four helpers (witness/operation.rs:908-1099) and the oracle's CPU constraints on a Machine run with one call of each
kind spliced in behind a SYSCALL row."""
import numpy as np

from zkm_amd import tables as T

from . import cpu_fixtures as CF
from . import cpu_steps_model as M
from . import io_calls_model as IO

GOOD = (0, 0, 0x2000, 70)


def channels(r):
    """[(is_read, address, value)] of a row's used channels, which must be the low ones."""
    used = [r[CF.ch(i, 0)] for i in range(8)]
    n = sum(used)
    assert used == [1] * n + [0] * (8 - n)
    return [(r[CF.ch(i, 1)], r[CF.ch(i, 4)], r[CF.ch(i, 5)]) for i in range(n)]


def only_clock_and_channels(x):
    """Every cell of every row but the clock and the cells of the used channels is 0, and the clock counts up."""
    for j, (r, mask, clock) in enumerate(zip(x.rows, x.masks, x.clocks)):
        keep = {CF.CLOCK} | {CF.ch(i, f) for i in range(8) if (mask >> i) & 1 for f in range(6)}
        assert all(v == 0 for c, v in enumerate(r) if c not in keep) and r[CF.CLOCK] == clock == x.clocks[0] + j


def test_preimage_of_five_bytes_by_hand():
    x = IO.Expansion()
    x.preimage(bytes(range(0xA0, 0xC0)) + bytes([1, 2, 3, 4, 5]), (0, 0, 0x31000000, 70))
    assert x.masks == [0xFF, 0b111] and x.clocks == [7, 8]
    assert channels(x.rows[0]) == [(1, 0x30001000 + 4 * i, int.from_bytes(bytes(range(0xA0 + 4 * i, 0xA4 + 4 * i)), "big")) for i in range(8)]
    assert channels(x.rows[1]) == [(0, 0x31000000, 5), (0, 0x31000004, 0x01020304), (0, 0x31000008, 0x05010000)]
    only_clock_and_channels(x)


def test_preimage_last_words_by_hand():
    for b in (0x00, 0x7F, 0xE5):
        x = IO.Expansion()
        x.preimage(bytes(32) + bytes(range(1, 29)) + bytes([b]), (0, 0, 0x31000000, 0))        # 29 bytes: 29 % 32 + 4 > 32
        assert x.masks == [0xFF, 0xFF, 0x01] and x.clocks == [0, 1, 2]                            # length + 8 words: the eighth opens a row
        assert channels(x.rows[2]) == [(0, 0x31000000 + 4 * 8, b << 24 | 0x010080)]
        assert channels(x.rows[1])[0] == (0, 0x31000000, 29) and channels(x.rows[1])[7] == (0, 0x3100001C, 0x191A1B1C)
    # 27 bytes: three bytes in the last word, 27 % 32 + 4 = 31: no closing bit; 31 bytes: three bytes and the closing bit beside the 1
    x = IO.Expansion()
    x.preimage(bytes(32) + bytes(24) + bytes([0xAA, 0xBB, 0xCC]), (0, 0, 0x31000000, 0))
    assert x.masks == [0xFF, 0xFF] and channels(x.rows[1])[7] == (0, 0x3100001C, 0xAABBCC01)
    x = IO.Expansion()
    x.preimage(bytes(32) + bytes(28) + bytes([0xAA, 0xBB, 0xCC]), (0, 0, 0x31000000, 0))
    assert x.masks == [0xFF, 0xFF, 0x01] and channels(x.rows[2]) == [(0, 0x31000020, 0xAABBCC81)]
    # no content: the length word alone; whole words: no marker at all
    x = IO.Expansion()
    x.preimage(bytes(32), (0, 0, 0x31000000, 0))
    assert x.masks == [0xFF, 0x01] and channels(x.rows[1]) == [(0, 0x31000000, 0)]
    x = IO.Expansion()
    x.preimage(bytes(32) + bytes([0xDE, 0xAD, 0xBE, 0xEF]), (0, 0, 0x31000000, 0))
    assert x.masks == [0xFF, 0x03] and channels(x.rows[1]) == [(0, 0x31000000, 4), (0, 0x31000004, 0xDEADBEEF)]


def test_hint_reads_by_hand():
    x = IO.Expansion()
    x.hint_read(b"", GOOD)
    assert x.masks == [0] and x.clocks == [7] and len(x.rows) == 1                               # a call of 0 bytes still pushes one row
    only_clock_and_channels(x)
    data = bytes(range(100, 137))
    x = IO.Expansion()
    x.hint_read(data, (7, 2, 0x2000, 70))
    assert x.masks == [0xFF, 0x03] and x.clocks == [7, 8]
    assert channels(x.rows[0]) == [(0, 0x2000 + 4 * i, int.from_bytes(data[4 * i:4 * i + 4], "big")) for i in range(8)]
    assert channels(x.rows[1]) == [(0, 0x2020, int.from_bytes(data[32:36], "big")), (0, 0x2024, data[36] << 24)]
    assert all(r[CF.ch(i, 2)] == 7 and r[CF.ch(i, 3)] == 2 for r in x.rows for i in range(8) if r[CF.ch(i, 0)])
    only_clock_and_channels(x)
    assert x.memory_ops() == 10 and len(x.channel_ops()) == 10 and x.channel_ops()[9] == (7, 2, 0x2024, 80, 0, data[36] << 24)


def test_commit_and_verify_by_hand():
    data = bytes(range(1, 37))
    x = IO.Expansion()
    x.commit(data, GOOD)
    assert x.masks == [0xFF, 0x01] and x.clocks == [7, 8]
    assert channels(x.rows[0])[1] == (1, 0x2004, 0x05060708) and channels(x.rows[1]) == [(1, 0x2020, 0x21222324)]
    x = IO.Expansion()
    x.commit(b"", GOOD)
    assert x.masks == [0] and len(x.rows) == 1
    x = IO.Expansion()
    x.verify(data[:32], GOOD)
    assert x.masks == [0xFF] and channels(x.rows[0]) == [(1, 0x2000 + 4 * i, int.from_bytes(data[4 * i:4 * i + 4], "big")) for i in range(8)]
    only_clock_and_channels(x)


def test_lists_expand_and_the_row_counts():
    calls = [(IO.HINT_READ, bytes(5), (0, 0, 0x1000, 10)), (IO.PREIMAGE, bytes(32 + 61), (0, 0, 0x31000000, 50)), (IO.VERIFY, bytes(32), (0, 0, 0x3000, 100)),
             (IO.COMMIT, bytes(68), (0, 0, 0x4000, 200))]
    kinds, data, off, meta = IO.lists(calls)
    assert off.tolist() == [0, 5, 98, 130, 198] and kinds.tolist() == [0, 3, 2, 1]
    x = IO.expand(kinds, data, off, meta)
    # the preimage: the hash row, then the length and 16 content words in three rows (the 17th word opens the third)
    assert x.clocks == [1, 5, 6, 7, 8, 10, 20, 21, 22] and x.masks == [0x03, 0xFF, 0xFF, 0xFF, 0x01, 0xFF, 0xFF, 0xFF, 0x01]
    assert [IO.row_count(k, len(d)) for k, d, _ in calls] == [1, 4, 1, 3]
    records, clocks = IO.steps(x, raw_base=4)
    assert records["reads"][:, 0].tolist() == list(range(4, 13)) and clocks.tolist() == x.clocks
    # what 1 MiB of input costs the link host-expanded: 32,768 rows of 2,072 bytes
    assert IO.row_count(IO.HINT_READ, 1 << 20) == 32768 and 32768 * CF.W * 8 == 67895296


def machine_with_calls(seed=5):
    """The sample program, then one call of each kind behind a SYSCALL row."""
    rng = np.random.default_rng(seed)
    m = M.Recorder()
    CF.sample_program(m)
    calls = IO.CallRecorder(m)
    for kind, addr, L in (("hint_read", 0x20000, 37), ("commit", 0x20000, 36), ("verify", 0x20000, 32), ("preimage", 0x31000000, 32 + 29)):
        for reg, v in ((4, addr), (5, L), (6, 0x30000), (37, 0x40000000)):
            m.set_reg(reg, v)
        m.syscall("other")
        calls.io(kind, addr, rng.integers(0, 256, L, dtype=np.uint8).tobytes())
        m.nop()
    return m, calls


def test_model_rows_pass_the_oracles_cpu_constraints(oracle):
    m, calls = machine_with_calls()
    _, _, x = calls.finish()
    assert len(x.rows) == 2 + 2 + 1 + 3 and x.masks == [0xFF, 0x03, 0xFF, 0x01, 0xFF, 0xFF, 0xFF, 0x01]
    log_n = len(m.rows).bit_length()
    m.pad((1 << log_n) - len(m.rows))
    trace = m.trace(log_n)
    count, bad = oracle.debug_constraints(T.TABLE_CPU, trace, 259, log_n)
    assert count == 741 and bad is None, bad
    cols = trace.reshape(259, -1)
    assert (cols[CF.CLOCK] == np.arange(1 << log_n)).all()      # every call row sits at its clock
    # the rows are live under the constraints: a row whose channel 0 is used "twice" is refused at that row
    for at in (x.clocks[0], x.clocks[-1]):
        flipped = cols.copy()
        flipped[CF.ch(0, 0), at] = 2
        assert oracle.debug_constraints(T.TABLE_CPU, flipped.reshape(-1), 259, log_n)[1][0] == at
