"""GPU suite: zkm_witness_check / zkm_segment_witness_check -- each table's own constraints on every row of the trace, from the trace
alone, naming the first failure: the lowest failing row, the lowest nonzero constraint on it, its canonical value, the number of failing
rows and the number of constraints a row emits.  Every expectation comes from the oracle: oracle.debug_constraints gives the first
finding and the count of constraints, oracle.row_constraints the value and, row by row, the number of failing rows.

* the valid golden segment through both calls (and the one host wait of the segment call);
* rows that satisfy nothing (quotient_fixtures.invalid_trace), all twelve tables, at 2^3 rows (part of a wave), 2^7 (two waves) and
  2^9 (two workgroups);
* one cell of a valid table changed, at the rows around the wave and workgroup boundaries and at both ends of the table, then two rows
  of different workgroups (or waves) at once;
* two tables of the segment changed at once; device-resident tables, also the block zkm_segment_tables builds.

The columns of the third part were chosen on a CPU with the oracle alone: for every table and every row position used here at least one
of its columns gives a finding (the test asserts it again); where both kinds exist, one column whose first finding is on the changed
row and one whose first finding is on the row before it, through a constraint that reads the next row."""
import ctypes as C
import os

import numpy as np
import pytest

from zkm_amd import tables as T

from . import quotient_fixtures as Q
from . import segment_ops_fixtures as SF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = Q.P
NAMES = ["Arithmetic", "Cpu", "Poseidon", "PoseidonSponge", "Keccak", "KeccakSponge", "ShaExtend", "ShaExtendSponge", "ShaCompress",
         "ShaCompressSponge", "Logic", "Memory"]                    # Table::all()
ARITHMETIC, CPU, LOGIC, MEMORY = 0, 1, 10, 11
# position in Table::all() -> the columns of part 3 (golden segment12.npz)
COLUMNS = {0: (6, 44), 1: (3, 0), 2: (1, 12), 3: (0, 14), 4: (0, 28), 5: (0, 40), 6: (8, 40), 7: (0, 11), 8: (92, 0), 9: (126,), 10: (3, 68),
           11: (3, 4)}


@pytest.fixture(scope="module")
def golden():
    """[(table id, W x n matrix, width, log_n)] of tests/golden/segment12.npz in Table::all() order."""
    seg = np.load(os.path.join(ROOT, "tests", "golden", "segment12.npz"))
    out = []
    for i in range(12):
        tid = T.TABLE_ENUM_ORDER[i]
        W, lg = T.WIDTH[tid], int(seg["log_n"][i])
        out.append((tid, seg["t%d" % i].reshape(W, 1 << lg), W, lg))
    assert [Q.NAMES[t[0]] for t in out] == NAMES
    return out


@pytest.fixture(scope="module")
def golden_counts(oracle, golden):
    """The oracle's verdict on the golden tables, once: every constraint holds; the constraints a row emits."""
    counts = []
    for tid, m, W, lg in golden:
        count, first = oracle.debug_constraints(tid, m.reshape(-1), W, lg)
        assert first is None and 0 < count < 1 << 16
        counts.append(count)
    return counts


def row_values(oracle, tid, m, r):
    n = m.shape[1]
    return oracle.row_constraints(tid, m[:, r], m[:, (r + 1) % n], r == 0, r == n - 1)


def oracle_finding(oracle, tid, m, rows=None):
    """(row or None, index, value, failing rows, constraints per row) as the oracle sees the W x n matrix m; the failing rows are counted
    row by row over `rows` (default: all) -- the caller passes the rows that can fail when every other row is known to hold."""
    W, n = m.shape
    count, first = oracle.debug_constraints(tid, m.reshape(-1), W, n.bit_length() - 1)
    failing = sum(1 for r in (range(n) if rows is None else sorted(set(rows))) if row_values(oracle, tid, m, r).any())
    if first is None:
        assert failing == 0
        return (None, 0, 0, 0, count)
    row, index = first
    value = int(row_values(oracle, tid, m, row)[index])
    assert value != 0 and failing >= 1
    return (row, index, value, failing, count)


def check_message(msg, name, finding, n):
    row, index, value, failing, count = finding
    assert msg == "Constraint failed in %sStark: row %d, constraint %d of %d = %#x (%d of %d rows fail)" % (name, row, index, count, value, failing, n)


def bumped(m, cells):
    out = m.copy()
    for c, r in cells:
        out[c, r] = (int(out[c, r]) + 1) % P
    return out


def touched(cells, n):
    """The rows whose (local, next) pair holds one of the cells."""
    return [x for _, r in cells for x in ((r - 1) % n, r)]


# ---- 1. the valid segment
def test_valid_segment_holds_in_both_calls_with_one_host_wait(ctx, golden, golden_counts):
    lg = [t[3] for t in golden]
    waits = ctx.host_waits()
    findings = ctx.segment_witness_check([t[1] for t in golden], lg)
    assert ctx.host_waits() - waits == 1
    assert ctx.witness_message is None
    assert findings == [(None, 0, 0, 0, count) for count in golden_counts]
    for (tid, m, W, log_n), count in zip(golden, golden_counts):
        assert ctx.witness_check(tid, m, log_n) == (None, 0, 0, 0, count), Q.NAMES[tid]
        assert ctx.witness_message is None


# ---- 2. rows that satisfy nothing
@pytest.mark.parametrize("log_n", [3, 7, 9])
@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("table_id", sorted(T.WIDTH), ids=lambda t: Q.NAMES[t])
def test_invalid_rows_are_named_as_the_oracle_names_them(ctx, oracle, table_id, kind, log_n):
    W = T.WIDTH[table_id]
    m = Q.invalid_trace(table_id, kind, log_n).reshape(W, 1 << log_n)
    want = oracle_finding(oracle, table_id, m)
    assert want[0] is not None, "vacuous case"
    got = ctx.witness_check(table_id, m, log_n)
    print(Q.NAMES[table_id], kind, log_n, "oracle", want, "device", got)
    assert got == want
    check_message(ctx.witness_message, Q.NAMES[table_id], want, 1 << log_n)


# ---- 3. one wrong cell in a valid table
@pytest.mark.parametrize("t", range(12), ids=NAMES)
def test_one_wrong_cell_of_a_valid_table(ctx, oracle, golden, golden_counts, t):
    tid, m, W, log_n = golden[t]
    n = 1 << log_n
    positions = sorted({r for r in (0, 63, 64, 255, 256, n - 2, n - 1) if 0 <= r < n})
    seen = {r: 0 for r in positions}
    for col in COLUMNS[t]:
        for r in positions:
            bad = bumped(m, [(col, r)])
            want = oracle_finding(oracle, tid, bad, touched([(col, r)], n))
            if want[0] is None:
                continue                      # the oracle sees nothing in this cell at this row
            seen[r] += 1
            got = ctx.witness_check(tid, bad, log_n)
            assert got == want, (NAMES[t], col, r, got, want)
            check_message(ctx.witness_message, NAMES[t], want, n)
    assert all(seen.values()), (NAMES[t], seen)
    # two rows at once, a workgroup (256 rows) apart where the table is tall enough, else a wave apart
    if n >= 128:
        a, b = (40, 300) if n >= 512 else (5, 70)
        cells = [(COLUMNS[t][0], b), (COLUMNS[t][-1], a)]
        bad = bumped(m, cells)
        want = oracle_finding(oracle, tid, bad, touched(cells, n))
        assert want[0] is not None and want[0] <= a and want[3] >= 2
        got = ctx.witness_check(tid, bad, log_n)
        assert got == want, (NAMES[t], cells, got, want)


# ---- 4. two tables of the segment at once
def test_segment_call_names_the_first_failing_table(ctx, oracle, golden, golden_counts):
    lg = [t[3] for t in golden]
    tables = [t[1] for t in golden]
    cells = {LOGIC: [(COLUMNS[LOGIC][0], 300)], CPU: [(COLUMNS[CPU][0], 64)]}
    want = [(None, 0, 0, 0, count) for count in golden_counts]
    for t, cs in cells.items():
        tables[t] = bumped(tables[t], cs)
        want[t] = oracle_finding(oracle, golden[t][0], tables[t], touched(cs, 1 << lg[t]))
        assert want[t][0] is not None
    waits = ctx.host_waits()
    got = ctx.segment_witness_check(tables, lg)
    assert ctx.host_waits() - waits == 1
    assert got == want
    check_message(ctx.witness_message, "Cpu", want[CPU], 1 << lg[CPU])


# ---- 5. device-resident tables
def test_device_tables_give_the_host_tables_findings(ctx, zkm, oracle, golden, golden_counts):
    lg = [t[3] for t in golden]
    tables = [t[1] for t in golden]
    cells = [(COLUMNS[MEMORY][0], 256)]
    tables[MEMORY] = bumped(tables[MEMORY], cells)
    want = oracle_finding(oracle, golden[MEMORY][0], tables[MEMORY], touched(cells, 1 << lg[MEMORY]))
    assert want[0] is not None
    host = ctx.segment_witness_check(tables, lg)
    assert host[MEMORY] == want and [f[0] for f in host].count(None) == 11
    bufs = []
    try:
        for m in tables:
            bufs.append(ctx.alloc(m.size).upload(m.reshape(-1)))
        live = ctx.memory()[0]
        waits = ctx.host_waits()
        assert ctx.segment_witness_check(bufs, lg) == host
        assert ctx.host_waits() - waits == 1 and ctx.memory()[0] == live          # nothing copied, the scratch went back
        assert ctx.segment_witness_check([b.ptr for b in bufs], lg) == host
        assert ctx.witness_check(golden[MEMORY][0], bufs[MEMORY], lg[MEMORY]) == want
        check_message(ctx.witness_message, "Memory", want, 1 << lg[MEMORY])
    finally:
        for b in bufs:
            b.free()


def test_block_of_segment_tables_is_checked_in_place(ctx, zkm, oracle):
    """The twelve pointers of zkm_staged_segment_ptrs for a block zkm_segment_tables built: every constraint holds; then one cell
    overwritten through zkm_dev_upload, and the same finding as from the downloaded table."""
    raw, tables, ctls = SF.build_segment_ops(oracle)
    lg = [t[3] for t in tables]
    counts = [oracle.debug_constraints(t[0], t[1], t[2], t[3]) for t in tables]
    assert all(first is None for _, first in counts)
    with ctx.segment_tables(SF.segment_ops(zkm, raw))[0] as staged:
        ptrs = staged.tables()
        assert ctx.segment_witness_check(staged, lg) == [(None, 0, 0, 0, count) for count, _ in counts]
        tid, trace, W, log_n = tables[LOGIC][:4]
        n = 1 << log_n
        cells = [(3, 1)]
        bad = bumped(trace.reshape(W, n), cells)
        want = oracle_finding(oracle, tid, bad, touched(cells, n))
        assert want[0] is not None
        word, err = np.array([bad[3, 1]], dtype=np.uint64), C.c_char_p()
        assert ctx.L.zkm_dev_upload(ctx.h, ptrs[LOGIC] + 8 * (3 * n + 1), word.ctypes.data, 8, C.byref(err)) == 0, err.value
        got = ctx.segment_witness_check(ptrs, lg)
        assert got[LOGIC] == want and [f[0] for f in got].count(None) == 11
        check_message(ctx.witness_message, "Logic", want, n)
        assert ctx.witness_check(tid, bad, log_n) == want
