"""GPU suite: zkm_segments_check / zkm_segment_check -- the table constraints, the range-check lookups and the cross-table lookups of K
segments in one set of launches and two host waits -- and the gate "check_witness" in front of the prove calls.

Every expectation is what the three per-segment entry points (zkm_segment_witness_check, zkm_segment_lookup_check,
zkm_segment_check_ctls) give on the same tables, which their own suites hold to the oracle and the lookup model; the verdicts are
derived from those outputs by the rule of include/zkm_hip.h; one test consults the oracle directly.  Shapes: the golden segment (heights
2^3 .. 2^16), the sample program's segment and the one twice as long, and junk tables of 2^3, 2^7 and 2^9 rows (part of a wave, two waves,
two workgroups), K = 1, 2, 3 and 33 (two groups of ZKM_MAX_SEG segments).

The all-padding segment of tests/test_gpu_segments_ops.py is NOT a consistent witness -- its 2^6 CPU rows are the sample program cut short
(a Cpu constraint fails on the last row) and their memory channels have no rows in its three-operation Memory table -- so the third
consistent segment here is the sample program run twice, and the all-padding segment travels with the junk segments as the smallest
shape whose tables are mostly zero."""
import ctypes as C
import os

import numpy as np
import pytest

from zkm_amd import tables as T

from . import arith_fixtures as A
from . import check_ctls_model as M
from . import cpu_fixtures as CF
from . import cpu_steps_model as SM
from . import lookup_fixtures as LF
from . import quotient_fixtures as Q
from . import segment_ops_fixtures as SF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = Q.P
NAMES = ["Arithmetic", "Cpu", "Poseidon", "PoseidonSponge", "Keccak", "KeccakSponge", "ShaExtend", "ShaExtendSponge", "ShaCompress",
         "ShaCompressSponge", "Logic", "Memory"]                    # Table::all()
ARITHMETIC, CPU, KECCAK, LOGIC, MEMORY = 0, 1, 4, 10, 11
WIDTHS = [T.WIDTH[tid] for tid in T.TABLE_ENUM_ORDER]
MEM_FILTER, MEM_VALUE = 0, 6                 # memory/columns.rs
CPU_COLUMNS, LOGIC_COLUMN = (3, 0), 3        # the columns tests/test_gpu_witness_check.py changes in the golden Cpu and Logic tables


# ---------------------------------------------------------------- segments: (twelve flat column-major arrays, twelve heights)
def golden_segment():
    seg = np.load(os.path.join(ROOT, "tests", "golden", "segment12.npz"))
    return [np.ascontiguousarray(seg["t%d" % i]).reshape(-1) for i in range(12)], [int(x) for x in seg["log_n"]]


def empty_segment(oracle):
    """An all-padding segment but for 2^6 CPU rows of the sample program and three memory operations (the oracle's tables): well formed,
    provable, and inconsistent (see the head of this file)."""
    rows = SF.build_segment_ops(oracle)[0]["cpu_rows"].reshape(-1, 259)
    rows = np.ascontiguousarray(np.tile(rows, ((64 + len(rows) - 1) // len(rows), 1))[:64])
    mem = np.array([[0, 2, 5, 1, 0, 7], [0, 2, 5, 2, 1, 7], [0, 2, 9, 3, 0, 11]], dtype=np.uint64)
    zeros = lambda w: np.zeros(w << 6, np.uint64)
    tables = [A.generate_trace([], 16), np.ascontiguousarray(SF.canonical(rows).T).reshape(-1),
              oracle.poseidon_trace_inputs(np.zeros((0, 12), np.uint64), np.zeros(0, np.uint64), 6), zeros(110), zeros(2431), zeros(470),
              zeros(78), zeros(76), zeros(224), zeros(127), zeros(69), oracle.memory_trace(mem, 2)[0]]
    return [np.ascontiguousarray(t, dtype=np.uint64).reshape(-1) for t in tables], [16, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 2]


@pytest.fixture(scope="module")
def built(oracle):
    """(raw, tables, ctls) of the sample program's segment, and of the one twice as long."""
    return [SF.build_segment_ops(oracle, repeat=r) for r in (1, 2)]


@pytest.fixture(scope="module")
def three(oracle, built):
    """Three consistent segments of different heights: the sample program's, the golden one, the sample program run twice."""
    segs = [([t[1] for t in built[0][1]], [t[3] for t in built[0][1]]), golden_segment(), ([t[1] for t in built[1][1]], [t[3] for t in built[1][1]])]
    assert len({tuple(lg) for _, lg in segs}) == 3
    return segs


def junk_segment(heights, kind):
    return [Q.invalid_trace(tid, kind, lg) for tid, lg in zip(T.TABLE_ENUM_ORDER, heights)], list(heights)


def changed(seg, t, cells):
    """The segment with cells (column, row) of table t increased by one mod p."""
    traces, lg = seg
    m = traces[t].copy().reshape(WIDTHS[t], 1 << lg[t])
    for c, r in cells:
        m[c, r] = (int(m[c, r]) + 1) % P
    return traces[:t] + [m.reshape(-1)] + traces[t + 1:], lg


# ---------------------------------------------------------------- the expectation: the three per-segment entry points
def report_key(rep):
    return (rep.kind, rep.ctl if rep.kind else 0, M.report_fields(rep))


def alone(ctx, seg):
    """(verdict, witness findings, lookup findings, report key, message) of one segment from the three per-segment calls."""
    traces, lg = seg
    wf = ctx.segment_witness_check(traces, lg)
    w_msg = ctx.witness_message
    lf = ctx.segment_lookup_check(traces, lg)
    l_msg = ctx.lookup_message
    rep = ctx.segment_check_ctls(traces, lg)
    w_bad = [t for t, f in enumerate(wf) if f[0] is not None]
    l_bad = [t for t, f in enumerate(lf) if f[0] is not None]
    if w_bad:
        verdict, msg = (1, w_bad[0]), w_msg
    elif l_bad:
        verdict, msg = (2, l_bad[0]), l_msg
    elif rep.kind:
        verdict, msg = (3, rep.ctl), rep.message
    else:
        verdict, msg = (0, 0), None
    return verdict, wf, lf, report_key(rep), msg


def assert_call_equals_alone(ctx, segs, want, name="zkm_segments_check"):
    """One K-segment call against the per-segment expectations `want`; returns the host waits it made."""
    waits = ctx.host_waits()
    got = ctx.segments_check(segs)
    waits = ctx.host_waits() - waits
    assert len(got) == len(segs)
    for s, ((verdict, wf, lf, rep), (w_verdict, w_wf, w_lf, w_rep, _)) in enumerate(zip(got, want)):
        assert verdict == w_verdict, (s, verdict, w_verdict)
        assert wf == w_wf, (s, wf, w_wf)
        assert lf == w_lf, (s, lf, w_lf)
        assert report_key(rep) == w_rep, (s, report_key(rep), w_rep)
    assert len({(rep.attempts, rep.host_waits) for _, _, _, rep in got}) == 1               # the call's, in every report
    first = [s for s, w in enumerate(want) if w[0][0]]
    if first:
        assert ctx.check_message == "%s: segment %d: %s" % (name, first[0], want[first[0]][4])
    else:
        assert ctx.check_message is None
    return waits


# ---- 1. three consistent segments of different heights
def test_three_consistent_segments_from_host_device_and_built_blocks(ctx, zkm, oracle, three, built):
    want = [alone(ctx, seg) for seg in three]
    assert [w[0] for w in want] == [(0, 0)] * 3, [w[4] for w in want]
    ctx.segments_check(three)                                       # (the first call may grow the download area)
    assert assert_call_equals_alone(ctx, three, want) == 2
    assert ctx.check_message is None
    for s, seg in enumerate(three):
        waits = ctx.host_waits()
        got = ctx.segment_check(*seg)
        assert ctx.host_waits() - waits == 2 and ctx.check_message is None
        assert (got[0], got[1], got[2], report_key(got[3])) == want[s][:4]
    # device buffers: nothing is copied, and the scratch goes back
    bufs = [[ctx.alloc(t.size).upload(t) for t in traces] for traces, _ in three]
    try:
        dev = [(b, lg) for b, (_, lg) in zip(bufs, three)]
        ctx.segments_check(dev)
        live = ctx.memory()[0]
        assert assert_call_equals_alone(ctx, dev, want) == 2
        assert ctx.memory()[0] == live
        mixed = [dev[0], three[1], ([b.ptr for b in bufs[2]], three[2][1])]
        assert assert_call_equals_alone(ctx, mixed, want) == 2
        assert ctx.memory()[0] == live
    finally:
        for b in sum(bufs, []):
            b.free()
    # the blocks zkm_segments_tables built
    ops = [SF.segment_ops(zkm, raw) for raw, _, _ in built]
    staged = ctx.segments_tables(ops)
    try:
        segs = [(st, lg) for st, lg in staged]
        w2 = [alone(ctx, (st.tables(), lg)) for st, lg in staged]
        assert [w[0] for w in w2] == [(0, 0)] * 2
        live = ctx.memory()[0]
        assert assert_call_equals_alone(ctx, segs, w2) == 2
        assert ctx.memory()[0] == live
    finally:
        for st, _ in staged:
            st.free()


# ---- 2. a finding must not cross segments
def test_a_finding_of_one_segment_leaves_the_others_all_hold(ctx, three):
    clean = [alone(ctx, seg) for seg in three]
    n = 1 << three[1][1][CPU]
    positions = sorted({r for r in (0, 63, 64, 255, 256, n - 2, n - 1) if 0 <= r < n})
    seen = {r: 0 for r in positions}
    for col in CPU_COLUMNS:
        for r in positions:
            bad = changed(three[1], CPU, [(col, r)])
            want = alone(ctx, bad)
            if want[1][CPU][0] is None:
                continue                          # the single-segment call sees nothing in this cell at this row
            seen[r] += 1
            assert want[0] == (1, 1) and want[4].startswith("Constraint failed in CpuStark: ")
            assert assert_call_equals_alone(ctx, [three[0], bad, three[2]], [clean[0], want, clean[2]]) == 2, (col, r)
            assert ctx.check_message.startswith("zkm_segments_check: segment 1: Constraint failed in CpuStark: ")
    assert all(seen.values()), seen


# ---- 3. precedence and completeness
def test_precedence_of_the_kinds_and_every_segment_checked_to_the_end(ctx, oracle, three, built):
    (tr0, lg0), tables0 = three[0], built[0][1]
    nm = 1 << lg0[MEMORY]
    # a filtered Memory row whose value no Memory constraint reads back (chosen with the oracle on the CPU), and a FREQUENCIES cell
    mem = tr0[MEMORY].reshape(WIDTHS[MEMORY], nm)
    row = None
    for r in (int(x) for x in np.nonzero(mem[MEM_FILTER] == 1)[0]):
        m = mem.copy()
        m[MEM_VALUE, r] = (int(m[MEM_VALUE, r]) + 1) % P
        if oracle.debug_constraints(T.TABLE_MEMORY, m.reshape(-1), WIDTHS[MEMORY], lg0[MEMORY])[1] is None:
            row = r
            break
    assert row is not None
    seg0 = changed(changed(three[0], MEMORY, [(MEM_VALUE, row)]), MEMORY, [(LF.MEMORY.freq_col, 0)])
    seg1 = changed(three[1], LOGIC, [(LOGIC_COLUMN, 300)])
    n2 = 1 << three[2][1][CPU]
    col2 = next(c for c in range(WIDTHS[CPU])                                 # (a column the oracle sees at row 5, chosen on the CPU)
                if oracle.debug_constraints(T.TABLE_CPU, changed(three[2], CPU, [(c, 5)])[0][CPU], WIDTHS[CPU], three[2][1][CPU])[1] is not None)
    seg2 = changed(three[2], CPU, [(col2, 5)])
    assert n2 > 5
    segs = [seg0, seg1, seg2]
    want = [alone(ctx, s) for s in segs]
    assert [w[0][0] for w in want] == [2, 1, 1], [w[0] for w in want]         # segment 0: the lookup before the CTL
    assert want[0][0] == (2, MEMORY) and want[0][3][0] == 2 and want[1][0] == (1, LOGIC) and want[2][0] == (1, CPU)
    assert assert_call_equals_alone(ctx, segs, want) == 3                     # ... and one wait for the report
    assert ctx.check_message.startswith("zkm_segments_check: segment 0: Lookup failed in MemoryStark: ")


# ---- 4. junk segments
JUNK_HEIGHTS = [[3, 7, 9, 3, 7, 9, 3, 7, 9, 3, 7, 9], [9, 3, 7, 7, 9, 3, 3, 3, 7, 9, 9, 7], [7, 9, 3, 9, 3, 7, 9, 7, 3, 7, 3, 3]]


def assert_all_kinds_present(want):
    assert any(f[0] is not None for w in want for f in w[1])                  # constraints
    assert any(f[0] is not None for w in want for f in w[2])                  # range-check lookups
    kinds = {w[3][0] for w in want}
    assert 1 in kinds and 0 not in kinds, kinds                               # non-binary filters among the reports


def test_three_junk_segments_of_mixed_heights_and_an_all_padding_one(ctx, oracle):
    segs = [junk_segment(h, kind) for h, kind in zip(JUNK_HEIGHTS, ("random", "constant", "random"))]
    want = [alone(ctx, s) for s in segs]
    assert_all_kinds_present(want)
    assert_call_equals_alone(ctx, segs, want)
    segs.insert(1, empty_segment(oracle))
    want.insert(1, alone(ctx, segs[1]))
    assert want[1][0] == (1, CPU) and want[1][3][0] == 2                      # the cut program's last row; a memory channel without its row
    assert_call_equals_alone(ctx, segs, want)


def test_thirty_three_junk_segments_in_two_groups(ctx):
    kinds = [junk_segment([3] * 12, kind) for kind in ("random", "constant")]
    alone_kinds = [alone(ctx, s) for s in kinds]
    order = [(s * 7 + s // 3) % 2 for s in range(33)]
    assert_all_kinds_present(alone_kinds)
    assert_call_equals_alone(ctx, [kinds[k] for k in order], [alone_kinds[k] for k in order])


# ---- 5. launch accounting
def test_launches_do_not_grow_with_the_segments(ctx, three):
    small = junk_segment([3] * 12, "random")
    ctx.profile(True)
    try:
        def run(segs):
            ctx.profile_reset()
            ctx.segments_check(segs)
            ctx.synchronize()
            return {k: v[0] for k, v in ctx.profile_records().items() if k.split("/")[0] in ("witness_check", "lookup_check", "check_ctls")}
        one, two, thr = run([three[1]]), run([three[1], three[0]]), run(three)
        j1, j3 = run([small]), run([small] * 3)
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    print(one, two, thr)
    for a, b in ((one, thr), (j1, j3)):
        assert a["witness_check/rows"] == b["witness_check/rows"] == 12 and a["witness_check/name"] == b["witness_check/name"] == 12
        for k in (k for k in a if k.startswith("lookup_check/")):
            assert a[k] == b[k], (k, a, b)                                    # 2 and 6 jobs: one group
    cc = [k for k in one if k.startswith("check_ctls/")]
    assert len(cc) >= 10 and {k for k in two if k.startswith("check_ctls/")} == set(cc)
    for k in cc:
        assert two[k] == one[k], (k, one, two)                                # 30 jobs: one group
        assert thr[k] == 2 * one[k], (k, one, thr)                            # 45 jobs: two groups


# ---- 6. the oracle anchor
def test_junk_findings_are_the_oracles(ctx, oracle):
    seg = junk_segment(JUNK_HEIGHTS[0], "random")
    got = ctx.segments_check([junk_segment(JUNK_HEIGHTS[1], "constant"), seg])[1]
    for t in (CPU, KECCAK):
        tid, lg = T.TABLE_ENUM_ORDER[t], seg[1][t]
        m = seg[0][t].reshape(WIDTHS[t], 1 << lg)
        n = 1 << lg
        count, first = oracle.debug_constraints(tid, m.reshape(-1), WIDTHS[t], lg)
        values = [oracle.row_constraints(tid, m[:, r], m[:, (r + 1) % n], r == 0, r == n - 1) for r in range(n)]
        assert first is not None
        row, index = first
        assert got[1][t] == (row, index, int(values[row][index]), sum(1 for v in values if v.any()), count), NAMES[t]
    assert got[0][0] == 1                                                     # a table constraint comes first


# ---- 7. the gate
def broken_cpu_rows(raw):
    """One value word of a used memory channel changed in a CPU row: every table is still well formed."""
    rows = raw["cpu_rows"].copy()
    r = int(np.nonzero(rows[:, CF.ch(1, 0)] == 1)[0][3])
    rows[r, CF.ch(1, 5)] = (int(rows[r, CF.ch(1, 5)]) + 1) % (1 << 32)
    return dict(raw, cpu_rows=rows)


def broken_logic(oracle, seg):
    """The segment with one Logic cell of row 1 changed that is no lookup filter (a prover without the gate still proves it): the first
    column behind the four operation flags in which the oracle, on the CPU, sees a failing constraint."""
    for col in range(4, WIDTHS[LOGIC]):
        bad = changed(seg, LOGIC, [(col, 1)])
        if oracle.debug_constraints(T.TABLE_LOGIC, bad[0][LOGIC], WIDTHS[LOGIC], seg[1][LOGIC])[1] is not None:
            return bad
    raise AssertionError("no Logic column gives a finding at row 1")


def assert_same_proofs(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_check_witness_guards_every_prove_call(ctx, zkm, oracle, three, built):
    raw, tables, ctls = built[0]
    traces, lg = three[0]
    ops = lambda r=raw: SF.segment_ops(zkm, r)
    good_tr = ctx.prove_segment(traces, lg, public_values=[1, 2])
    good_ops = ctx.prove_segments_ops([ops(), ops(), ops()], public_values=[[1, 2]] * 3)
    rec = SM.Recorder()
    CF.sample_program(rec)
    rec.pad((1 << 8) - len(rec.rows))
    steps, beside = rec.cpu_steps(zkm), zkm.SegmentOps(None, None, arithmetic_ops=None, logic_ops=None)
    good_steps = ctx.prove_segments_ops_steps([steps], [beside], public_values=[[3]])
    bad_logic = broken_logic(oracle, three[0])
    assert alone(ctx, bad_logic)[0] == (1, LOGIC)
    bad_freq = changed(three[0], ARITHMETIC, [(LF.ARITHMETIC.freq_col, 0)])
    assert alone(ctx, bad_freq)[0] == (2, ARITHMETIC)
    bad_raw = broken_cpu_rows(raw)
    ctx.prove_segment(bad_logic[0], lg)                             # key 0: a prover does not verify; twelve blobs come back
    cfg = ctx.standard_config()
    try:
        ctx.set_tuning("check_witness", 1)
        # consistent input: the same words
        assert_same_proofs(good_tr, ctx.prove_segment(traces, lg, public_values=[1, 2]))
        for a, b in zip(good_ops, ctx.prove_segments_ops([ops(), ops(), ops()], public_values=[[1, 2]] * 3)):
            assert_same_proofs(a, b)
        for a, b in zip(good_steps, ctx.prove_segments_ops_steps([steps], [beside], public_values=[[3]])):
            assert_same_proofs(a, b)
        # zkm_prove_segment on a changed Logic cell: the constraint is named and no proof or challenge word is written
        proofs = np.zeros(good_tr[2][12], dtype=np.uint64)
        chal = np.zeros(2 * cfg.num_challenges, dtype=np.uint64)
        ptrs = (C.c_void_p * 12)(*[t.ctypes.data for t in bad_logic[0]])
        lgc = (C.c_uint * 12)(*lg)
        offs, err = (C.c_size_t * 13)(), C.c_char_p()
        rc = ctx.L.zkm_prove_segment(ctx.h, C.byref(cfg), ptrs, lgc, None, 0, proofs.ctypes.data_as(zkm.u64p), offs, chal.ctypes.data_as(zkm.u64p),
                                     C.byref(err))
        assert rc != 0 and err.value.startswith(b"check_witness: segment 0: Constraint failed in LogicStark"), err.value
        assert not proofs.any() and not chal.any()
        # three segments from their operations, the middle one's CPU rows broken
        with pytest.raises(zkm.ZkmError, match=r"check_witness: segment 1: CTL #\d+"):
            ctx.prove_segments_ops([ops(), ops(bad_raw), ops()])
        # a changed RC_FREQUENCIES cell through zkm_prove_segments
        with pytest.raises(zkm.ZkmError, match=r"check_witness: segment 1: Lookup failed in ArithmeticStark"):
            ctx.prove_segments([(traces, lg, ()), (bad_freq[0], lg, ())])
        # with "check_ctls" also set: the same message, and the cross-table lookups are checked once
        ctx.set_tuning("check_ctls", 1)
        ctx.profile(True)
        try:
            ctx.profile_reset()
            with pytest.raises(zkm.ZkmError, match=r"check_witness: segment 1: Lookup failed in ArithmeticStark"):
                ctx.prove_segments([(traces, lg, ()), (bad_freq[0], lg, ())])
            ctx.synchronize()
            assert ctx.profile_records()["check_ctls/count"][0] == 1
        finally:
            ctx.profile(False)
            ctx.profile_reset()
            ctx.set_tuning("check_ctls", 0)
        # zkm_prove_with_traces on the AllStark description
        bad_tables = [(t[0], b, t[2], t[3], t[4]) for t, b in zip(tables, bad_logic[0])]
        with pytest.raises(zkm.ZkmError, match=r"check_witness: segment 0: Constraint failed in LogicStark"):
            ctx.prove_with_traces(bad_tables, ctls)
    finally:
        ctx.set_tuning("check_witness", 0)
        ctx.set_tuning("check_ctls", 0)
    assert_same_proofs(good_tr, ctx.prove_segment(traces, lg, public_values=[1, 2]))
    ctx.prove_segment(bad_logic[0], lg)                             # off again: the broken input proves


def test_a_pool_names_the_bad_segment_by_its_position_in_the_pool_call(zkm, oracle, three):
    traces, lg = three[0]
    bad = broken_logic(oracle, three[0])
    pool = zkm.Pool((0,), 2)
    try:
        pool.set_tuning("check_witness", 1)
        with pytest.raises(zkm.ZkmError, match=r"check_witness: segment 2: Constraint failed in LogicStark"):
            pool.prove_segments([(traces, lg, ()), (traces, lg, ()), (bad[0], lg, ())], max_stack=1)
        pool.set_tuning("check_witness", 0)
        assert len(pool.prove_segments([(traces, lg, ()), (bad[0], lg, ())], max_stack=1)) == 2
    finally:
        pool.close()
