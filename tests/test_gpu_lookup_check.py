"""GPU suite: zkm_lookup_check / zkm_segment_lookup_check -- a table's own range-check lookups from the trace alone, naming the smallest
value whose looking count differs from its frequency.  Every expectation -- the nine words and the exact message -- comes from
tests/lookup_model.py (held to lookup.rs by tests/test_lookup_model.py).

* every named case of tests/lookup_fixtures.py at shapes chosen by what can go wrong in the record pipeline (a radix tile is 2048 records):
  Memory 2^3 rows (16 records: part of a wave), 2^7 (256), 2^10 (2048: exactly one tile), 2^11 (4096: two tiles); Arithmetic 2^3 (152),
  2^7 (2432: a tile and a part), 2^11 (38912: 19 tiles); at Arithmetic 2^11 one value that fills nine tiles of looking cells;
* the golden segment (Arithmetic at its real 2^16 rows): all twelve tables hold with one host wait; one RC_FREQUENCIES cell and one Memory
  RANGE_CHECK cell changed; the ten tables without lookups;
* host arrays, DeviceBuffers, device pointers and the block zkm_segment_tables builds give the same words; the context after a finding;
  a table without lookups costs no host wait."""
import ctypes as C
import os

import numpy as np
import pytest

from zkm_amd import tables as T

from . import lookup_fixtures as LF
from . import lookup_model as LM
from . import segment_ops_fixtures as SF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = LM.P
NAMES = ["Arithmetic", "Cpu", "Poseidon", "PoseidonSponge", "Keccak", "KeccakSponge", "ShaExtend", "ShaExtendSponge", "ShaCompress",
         "ShaCompressSponge", "Logic", "Memory"]                    # Table::all()
ARITHMETIC, CPU, MEMORY = 0, 1, 11
SHAPES = [("Memory", 3), ("Memory", 7), ("Memory", 10), ("Memory", 11), ("Arithmetic", 3), ("Arithmetic", 7), ("Arithmetic", 11)]
RECORDS = [16, 256, 2048, 4096, 152, 2432, 38912]


def model_finding(position, m):
    """The model's finding for the table at `position` of Table::all(): the two tables with a lookup have one each."""
    if NAMES[position] not in LF.SHAPES:
        return LM.HOLDS
    return LM.finding(m, *LF.SHAPES[NAMES[position]].lookup())


def check_one(ctx, shape, m):
    """One table through zkm_lookup_check against the model: the words, the message."""
    want = LM.finding(m, *shape.lookup())
    got = ctx.lookup_check(shape.table_id, m, m.shape[1].bit_length() - 1)
    print(shape.name, m.shape, "model", want, "device", got)
    assert got == want
    assert ctx.lookup_message == LM.message(shape.name, want)
    return got


def test_shapes_are_the_record_counts_they_claim():
    assert [LF.SHAPES[s].records(lg) for s, lg in SHAPES] == RECORDS


# ---- 1. the named cases
@pytest.mark.parametrize("name", sorted(LF.CASES))
@pytest.mark.parametrize("shape,log_n", SHAPES, ids=["%s-%d" % s for s in SHAPES])
def test_named_case_gives_the_models_finding(ctx, shape, log_n, name):
    s = LF.SHAPES[shape]
    m, holds = LF.case(s, log_n, name)
    got = check_one(ctx, s, m)
    assert (got == LM.HOLDS) == holds


@pytest.mark.parametrize("off", [False, True], ids=["balanced", "off_by_one"])
def test_one_value_that_fills_more_than_a_tile(ctx, off):
    s = LF.ARITHMETIC
    m = LF.frequent_value(s, 11, off)
    assert int((LM.canonical(m[s.cols]) == 0).sum()) > 2048
    got = check_one(ctx, s, m)
    assert (got != LM.HOLDS) == off and (not off or (got[1], got[8]) == (0, 1))


# ---- 2. the golden segment
@pytest.fixture(scope="module")
def golden():
    """[(table id, W x n matrix, width, log_n)] of tests/golden/segment12.npz in Table::all() order."""
    seg = np.load(os.path.join(ROOT, "tests", "golden", "segment12.npz"))
    out = []
    for i in range(12):
        tid = T.TABLE_ENUM_ORDER[i]
        W, lg = T.WIDTH[tid], int(seg["log_n"][i])
        out.append((tid, seg["t%d" % i].reshape(W, 1 << lg), W, lg))
    assert out[ARITHMETIC][0] == T.TABLE_ARITHMETIC and out[ARITHMETIC][3] == 16 and out[MEMORY][0] == T.TABLE_MEMORY and out[CPU][0] == T.TABLE_CPU
    return out


def test_golden_segment_holds_with_one_host_wait(ctx, golden):
    lg = [t[3] for t in golden]
    assert [model_finding(i, t[1]) for i, t in enumerate(golden)] == [LM.HOLDS] * 12
    waits = ctx.host_waits()
    findings = ctx.segment_lookup_check([t[1] for t in golden], lg)
    assert ctx.host_waits() - waits == 1
    assert findings == [LM.HOLDS] * 12 and ctx.lookup_message is None


def test_two_tables_of_the_segment_changed_at_once(ctx, golden):
    lg = [t[3] for t in golden]
    tables = [t[1] for t in golden]
    tables[ARITHMETIC] = tables[ARITHMETIC].copy()
    tables[MEMORY] = tables[MEMORY].copy()
    LF.bump(tables[ARITHMETIC], LF.ARITHMETIC.freq_col, 300, 1)
    LF.bump(tables[MEMORY], LF.MEMORY.cols[0], 70, 1)
    want = [model_finding(i, m) for i, m in enumerate(tables)]
    assert want[ARITHMETIC] != LM.HOLDS and want[MEMORY] != LM.HOLDS and want.count(LM.HOLDS) == 10
    waits = ctx.host_waits()
    got = ctx.segment_lookup_check(tables, lg)
    assert ctx.host_waits() - waits == 1
    print("model", want[ARITHMETIC], want[MEMORY], "device", got[ARITHMETIC], got[MEMORY])
    assert got == want
    assert ctx.lookup_message == LM.message("Arithmetic", want[ARITHMETIC])
    # each of the two on its own
    assert ctx.lookup_check(T.TABLE_MEMORY, tables[MEMORY], lg[MEMORY]) == want[MEMORY]
    assert ctx.lookup_message == LM.message("Memory", want[MEMORY])


def test_table_without_lookups_costs_no_wait(ctx, golden):
    tid, m, W, log_n = golden[CPU]
    waits = ctx.host_waits()
    assert ctx.lookup_check(tid, m, log_n) == LM.HOLDS
    assert ctx.host_waits() == waits and ctx.lookup_message is None


# ---- 3. pointer kinds, and the context after a finding
def test_device_tables_give_the_host_tables_findings_and_the_context_stays_usable(ctx, golden):
    lg = [t[3] for t in golden]
    tables = [t[1] for t in golden]
    tables[MEMORY] = tables[MEMORY].copy()
    LF.bump(tables[MEMORY], LF.MEMORY.freq_col, 5, -1)
    want = [model_finding(i, m) for i, m in enumerate(tables)]
    assert want[MEMORY] != LM.HOLDS
    host = ctx.segment_lookup_check(tables, lg)
    assert host == want
    bufs = []
    try:
        for m in tables:
            bufs.append(ctx.alloc(m.size).upload(m.reshape(-1)))
        live = ctx.memory()[0]
        waits = ctx.host_waits()
        assert ctx.segment_lookup_check(bufs, lg) == host
        assert ctx.host_waits() - waits == 1 and ctx.memory()[0] == live          # nothing copied, the scratch went back
        assert ctx.lookup_message == LM.message("Memory", want[MEMORY])
        assert ctx.segment_lookup_check([b.ptr for b in bufs], lg) == host
        assert ctx.lookup_check(T.TABLE_MEMORY, bufs[MEMORY], lg[MEMORY]) == want[MEMORY]
        # after the findings: a valid call on the same context holds, and the live memory is what it was
        assert ctx.lookup_check(T.TABLE_ARITHMETIC, bufs[ARITHMETIC], lg[ARITHMETIC]) == LM.HOLDS and ctx.lookup_message is None
        assert ctx.memory()[0] == live
    finally:
        for b in bufs:
            b.free()


def test_block_of_segment_tables_is_checked_in_place(ctx, zkm, oracle):
    """The StagedTrace zkm_segment_tables builds from a segment's raw operations: every lookup holds; then one RC_FREQUENCIES cell
    overwritten through zkm_dev_upload, and the same words as from the host table, a DeviceBuffer and the twelve pointers."""
    raw, tables, ctls = SF.build_segment_ops(oracle)
    lg = [t[3] for t in tables]
    with ctx.segment_tables(SF.segment_ops(zkm, raw))[0] as staged:
        ptrs = staged.tables()
        assert ctx.segment_lookup_check(staged, lg) == [LM.HOLDS] * 12
        tid, trace, W, log_n = tables[ARITHMETIC][:4]
        n = 1 << log_n
        bad = trace.reshape(W, n).copy()
        LF.bump(bad, LF.ARITHMETIC.freq_col, 77, 2)
        want = LM.finding(bad, *LF.ARITHMETIC.lookup())
        assert want[1] == 77 and want[8] == 1
        word, err = np.array([bad[LF.ARITHMETIC.freq_col, 77]], dtype=np.uint64), C.c_char_p()
        assert ctx.L.zkm_dev_upload(ctx.h, ptrs[ARITHMETIC] + 8 * (LF.ARITHMETIC.freq_col * n + 77), word.ctypes.data, 8, C.byref(err)) == 0, err.value
        got = ctx.segment_lookup_check(staged, lg)
        assert got[ARITHMETIC] == want and got.count(LM.HOLDS) == 11
        assert ctx.lookup_message == LM.message("Arithmetic", want)
        assert ctx.segment_lookup_check(ptrs, lg) == got
        assert ctx.lookup_check(tid, bad, log_n) == want
        buf = ctx.alloc(bad.size).upload(bad.reshape(-1))
        try:
            assert ctx.lookup_check(tid, buf, log_n) == want
        finally:
            buf.free()
