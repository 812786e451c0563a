"""GPU suite: zkm_check_ctls / zkm_segment_check_ctls -- testutils::check_ctls (cross_table_lookup.rs:1486-1581) on the device.  The
oracle's check_ctls judges every verdict (kind 0 <=> code 0, kind 1 and lookup c <=> 200 + c, kind 2 and lookup c <=> 300 + c); the
content of a report -- which row, which tuple, which locations -- is predicted by the host model of the contract
(tests/check_ctls_model.py).  Then the collision path through its test hook, the check in front of the prove calls ("check_ctls"), and the
launch accounting."""
import ctypes as C
import os

import numpy as np
import pytest

from . import check_ctls_model as M
from . import cpu_fixtures as CF
from . import segment_ops_fixtures as SF

pytestmark = pytest.mark.gpu

P = SF.P
MEMORY, LOGIC, CPU = 11, 10, 1               # positions in Table::all()
MEM_FILTER, MEM_VALUE = 0, 6                 # memory/columns.rs


@pytest.fixture(scope="module")
def seg(oracle):
    return SF.build_segment_ops(oracle)


@pytest.fixture(scope="module")
def model():
    return M.Model()


def judged(ctx, oracle, tables, ctls):
    """The device's report, after the oracle has judged its verdict."""
    rep = ctx.check_ctls(tables, ctls)
    kind, c = M.verdict_of_code(oracle.check_ctls(tables, ctls))
    print("oracle: kind %d lookup %s; device: kind %d lookup %d attempts %d waits %d  %s" % (kind, c, rep.kind, rep.ctl, rep.attempts,
                                                                                             rep.host_waits, rep.message))
    assert rep.kind == kind and (kind == 0 or rep.ctl == c), (rep.kind, rep.ctl, kind, c)
    assert (rep.message is None) == (kind == 0)
    if kind:
        assert "CTL #%d" % c in rep.message
        assert ("Non-binary filter?" in rep.message) == (kind == 1)
    return rep


def word(tables, t, col, row):
    return (col << tables[t][3]) + row


def filtered_memory_row(tables, k=0):
    """The k-th row of the Memory table whose filter is 1."""
    n = 1 << tables[MEMORY][3]
    return int(np.nonzero(tables[MEMORY][1][MEM_FILTER * n:(MEM_FILTER + 1) * n] == 1)[0][k])


def tuple_at(model, tables, t, colset, row):
    """The tuple of a filtered row of one side, evaluated on the host."""
    f, rows, tuples = model.side(tables, t, colset)
    assert f[row] == 1
    return [int(x) for x in tuples[int(np.searchsorted(rows, row))]]


def simple_filter_column(ct, colset):
    """The trace column of a column set whose filter is one single-column term with coefficient 1 (Filter::new_simple(Column::single)),
    or None."""
    width, col_off, has_filter, nprod, prod_off, nconst, const_off, _ = ct._sets[colset]
    if not has_filter or nprod or nconst != 1:
        return None
    n_local, n_next, off, _, constant = ct._cols[ct._fidx[const_off]]
    return ct._tc[off] if (n_local, n_next, constant) == (1, 0, 0) and ct._tf[off] == 1 else None


def report_cases(seg, model):
    """(name, tables, lookups) of the cases whose reports the contract fixes completely."""
    raw, tables, ctls = seg
    cases = []
    r = filtered_memory_row(tables, 5)
    cases.append(("looked row changed", M.bump(tables, MEMORY, word(tables, MEMORY, MEM_VALUE, r)), ctls))
    # a looking row's filter switched off: the first looking side with a single-column filter that holds a 1
    done = False
    for c, (looking, looked) in enumerate(ctls):
        for t, cs in looking:
            col = simple_filter_column(tables[t][4], cs)
            if col is None or done:
                continue
            n = 1 << tables[t][3]
            on = np.nonzero(tables[t][1][col * n:(col + 1) * n] == 1)[0]
            if on.size:
                cases.append(("looking filter off (lookup %d)" % c, M.bump(tables, t, word(tables, t, col, int(on[-1])), 0), ctls))
                done = True
    assert done
    # a tuple twice on one side: Memory row a's lookup columns copied over row b's (both filtered)
    a, b = filtered_memory_row(tables, 2), filtered_memory_row(tables, 9)
    n = 1 << tables[MEMORY][3]
    tr = tables[MEMORY][1].copy()
    for col in range(1, 7):
        tr[col * n + b] = tr[col * n + a]
    twice = list(tables)
    twice[MEMORY] = tables[MEMORY][:1] + (tr,) + tables[MEMORY][2:]
    cases.append(("tuple twice on the looked side", twice, ctls))
    # a filter of 2 on two rows of two sides of one lookup (and with it a difference in that lookup): the smaller (side, row) is named
    for c, (looking, looked) in enumerate(ctls):
        lcol = simple_filter_column(tables[looked[0]][4], looked[1])
        picks = [(t, simple_filter_column(tables[t][4], cs)) for t, cs in looking]
        picks = [(t, col) for t, col in picks if col is not None and t != looked[0]]
        if lcol is None or not picks:
            continue
        t, col = picks[-1]
        nl, nt = 1 << tables[looked[0]][3], 1 << tables[t][3]
        on_l = np.nonzero(tables[looked[0]][1][lcol * nl:(lcol + 1) * nl] == 1)[0]
        on_t = np.nonzero(tables[t][1][col * nt:(col + 1) * nt] == 1)[0]
        if on_l.size and on_t.size:
            two = M.bump(M.bump(tables, looked[0], word(tables, looked[0], lcol, int(on_l[0])), 2), t, word(tables, t, col, int(on_t[-1])), 2)
            cases.append(("filter 2 on two sides (lookup %d)" % c, two, ctls))
            break
    else:
        raise AssertionError("no lookup with single-column filters on both sides")
    # two lookups broken: the Memory lookup (14) and the Logic lookup (13)
    nlg = 1 << tables[LOGIC][3]
    both = M.bump(cases[0][1], LOGIC, word(tables, LOGIC, 10, 0))    # an input bit of the first Logic operation
    cases.append(("two lookups broken", both, ctls))
    # two rows of the Logic table exchanged: a multiset does not see order
    m = tables[LOGIC][1].reshape(-1, nlg).copy()
    m[:, [0, 3]] = m[:, [3, 0]]
    assert (m != tables[LOGIC][1].reshape(-1, nlg)).any()
    swapped = list(tables)
    swapped[LOGIC] = tables[LOGIC][:1] + (m.reshape(-1),) + tables[LOGIC][2:]
    cases.append(("two Logic rows exchanged", swapped, ctls))
    return cases


def differential_cases(tables):
    return [(t, int(i)) for t in range(12) for i in np.random.default_rng(t).integers(0, tables[t][1].size, 6)]


def device_copies(ctx, tables):
    bufs = []
    for t in tables:
        b = ctx.alloc(t[1].size)
        b.upload(t[1])
        bufs.append(b)
    return bufs


# ---- 1. the consistent fixture from every kind of input
def test_consistent_segment_is_accepted_from_host_device_and_built_tables(ctx, zkm, oracle, seg):
    raw, tables, ctls = seg
    lg = [t[3] for t in tables]
    rep = judged(ctx, oracle, tables, ctls)
    assert rep.kind == 0 and rep.attempts == 1
    assert ctx.segment_check_ctls([t[1] for t in tables], lg).kind == 0
    by_columns = [(tid, [c for c in tr.reshape(ncols, -1)], ncols, log_n, ct) for tid, tr, ncols, log_n, ct in tables]
    assert ctx.check_ctls(by_columns, ctls).kind == 0
    bufs = device_copies(ctx, tables)
    try:
        live = ctx.memory()[0]
        assert ctx.check_ctls([(t[0], b, t[2], t[3], t[4]) for t, b in zip(tables, bufs)], ctls).kind == 0
        assert ctx.segment_check_ctls(bufs, lg).kind == 0
        assert ctx.memory()[0] == live                     # the scratch went back to the allocator
    finally:
        for b in bufs:
            b.free()
    with ctx.segment_tables(SF.segment_ops(zkm, raw))[0] as staged:
        assert ctx.segment_check_ctls(staged, lg).kind == 0
        assert ctx.segment_check_ctls(staged.tables(), lg).kind == 0


# ---- 2. a 2^16-cycle segment
def test_large_segment_accepted_and_a_changed_memory_row_named(ctx, oracle, model):
    raw, tables, ctls = SF.build_segment_ops(oracle, repeat=128)
    lg = [t[3] for t in tables]
    assert lg[0] == 16 and lg[CPU] == 15 and lg[LOGIC] == 11 and lg[MEMORY] == 17, lg
    assert judged(ctx, oracle, tables, ctls).kind == 0
    n = 1 << lg[MEMORY]
    r = filtered_memory_row(tables, 1000)
    old = tuple_at(model, tables, MEMORY, ctls[14][1][1], r)
    rep = judged(ctx, oracle, M.bump(tables, MEMORY, MEM_VALUE * n + r), ctls)
    assert (rep.kind, rep.ctl) == (2, 14)
    assert rep.tuple_words() == old and (rep.looking_count, rep.looked_count) == (1, 0)     # timestamps make Memory tuples unique
    assert rep.looked_locations() == [] and len(rep.looking_locations()) == 1
    side, table, row = rep.looking_locations()[0]
    assert side < len(ctls[14][0]) and ctls[14][0][side][0] == table
    # the looking location named still holds the tuple, with filter 1 (evaluated on the host)
    f, rows, tuples = model.side(tables, table, ctls[14][0][side][1])
    assert f[row] == 1 and tuple_at(model, tables, table, ctls[14][0][side][1], row) == old


# ---- 3. the differential slice: 72 single-word changes, every one judged by the oracle
def test_differential_slice_agrees_with_the_oracle(ctx, oracle, seg, model):
    raw, tables, ctls = seg
    kinds, lookups, accepted = set(), set(), 0
    cases = differential_cases(tables)
    assert len(cases) == 72
    for t, i in cases:
        changed = M.bump(tables, t, i)
        rep = judged(ctx, oracle, changed, ctls)
        assert M.report_fields(rep) == model.check(changed, ctls), (t, i)
        if rep.kind:
            kinds.add(rep.kind)
            lookups.add(rep.ctl)
        else:
            accepted += 1
    assert 72 - accepted >= 18 and accepted >= 10 and kinds == {1, 2} and len(lookups) >= 5, (accepted, kinds, lookups)


# ---- 4. the content of the report
def test_report_content_is_the_contracts(ctx, oracle, seg, model):
    raw, tables, ctls = seg
    got = {}
    for name, changed, lookups in report_cases(seg, model):
        rep = judged(ctx, oracle, changed, lookups)
        want = model.check(changed, lookups)
        assert M.report_fields(rep) == want, (name, M.report_fields(rep), want)
        got[name] = want
    r = filtered_memory_row(tables, 5)
    old = tuple_at(model, tables, MEMORY, ctls[14][1][1], r)
    w = got["looked row changed"]
    assert (w["kind"], w["ctl"], w["tuple"], w["looking_count"], w["looked_count"]) == (2, 14, old, 1, 0) and len(w["looking"]) == 1
    w = [v for k, v in got.items() if k.startswith("looking filter off")][0]
    assert w["kind"] == 2 and (w["looking_count"], w["looked_count"]) == (0, 1)
    w = got["tuple twice on the looked side"]
    assert w["kind"] == 2 and w["ctl"] == 14
    w = [v for k, v in got.items() if k.startswith("filter 2 on two sides")][0]
    assert w["kind"] == 1 and w["filter_value"] == 2 and w["side"] < len(ctls[w["ctl"]][0])      # the looking side comes first
    assert got["two lookups broken"]["ctl"] == 13
    assert got["two Logic rows exchanged"] is None


# ---- 5. determinism
def test_the_same_call_twice_gives_the_same_bytes(ctx, seg, model):
    for name, changed, lookups in report_cases(seg, model)[:4]:
        a, b = ctx.check_ctls(changed, lookups), ctx.check_ctls(changed, lookups)
        assert bytes(a) == bytes(b) and a.message == b.message, name


# ---- 6. the collision path
def test_truncated_keys_collide_and_the_second_attempt_gives_the_same_reports(ctx, zkm, seg, model):
    raw, tables, ctls = seg
    cases = [("consistent", tables, ctls)] + report_cases(seg, model) + [("slice %d %d" % c, M.bump(tables, *c), ctls)
                                                                           for c in differential_cases(tables)]
    plain = [ctx.check_ctls(t, l) for _, t, l in cases]
    assert all(r.attempts == 1 for r in plain)
    os.environ.pop("ZKM_ENABLE_TEST_HOOKS", None)
    with pytest.raises(zkm.ZkmError, match="unknown key"):
        ctx.set_tuning("debug_ctl_key_bits", 4)
    os.environ["ZKM_ENABLE_TEST_HOOKS"] = "1"
    try:
        ctx.set_tuning("debug_ctl_key_bits", 4)
        for (name, t, l), want in zip(cases, plain):
            rep = ctx.check_ctls(t, l)
            assert rep.attempts == 2 and rep.host_waits == want.host_waits + 1, (name, rep.attempts)
            assert M.report_fields(rep) == M.report_fields(want) and rep.message == want.message, name
    finally:
        ctx.set_tuning("debug_ctl_key_bits", 0)
        os.environ.pop("ZKM_ENABLE_TEST_HOOKS", None)
    assert ctx.check_ctls(tables, ctls).attempts == 1


# ---- 7. the check in front of the prove calls
def broken_cpu_rows(raw):
    """One value word of a used memory channel changed in a CPU row: every table is still well formed."""
    rows = raw["cpu_rows"].copy()
    r = int(np.nonzero(rows[:, CF.ch(1, 0)] == 1)[0][3])
    rows[r, CF.ch(1, 5)] = (int(rows[r, CF.ch(1, 5)]) + 1) % (1 << 32)
    return dict(raw, cpu_rows=rows)


def test_check_ctls_tuning_guards_every_prove_call(ctx, zkm, oracle, seg):
    raw, tables, ctls = seg
    lg = [t[3] for t in tables]
    bad_tables = M.bump(tables, MEMORY, word(tables, MEMORY, MEM_VALUE, filtered_memory_row(tables, 5)))
    bad_raw = broken_cpu_rows(raw)
    as_built = list(tables)
    as_built[CPU] = tables[CPU][:1] + (np.ascontiguousarray(SF.canonical(bad_raw["cpu_rows"]).T).reshape(-1),) + tables[CPU][2:]
    kind, c = M.verdict_of_code(oracle.check_ctls(as_built, ctls))
    assert kind == 2
    good = ctx.prove_segment_ops(SF.segment_ops(zkm, raw), public_values=[1, 2])
    good_tr = ctx.prove_segment([t[1] for t in tables], lg, public_values=[1, 2])
    ctx.prove_segment_ops(SF.segment_ops(zkm, bad_raw))          # key 0: a prover does not verify; twelve blobs come back
    cfg = ctx.standard_config()
    try:
        ctx.set_tuning("check_ctls", 1)
        # consistent input: the same words
        for a, b in zip(good, ctx.prove_segment_ops(SF.segment_ops(zkm, raw), public_values=[1, 2])):
            assert np.array_equal(np.asarray(a), np.asarray(b))
        for a, b in zip(good_tr, ctx.prove_segment([t[1] for t in tables], lg, public_values=[1, 2])):
            assert np.array_equal(np.asarray(a), np.asarray(b))
        # zkm_prove_segment on broken tables: the lookup is named and no proof word is written
        proofs = np.zeros(good_tr[2][12], dtype=np.uint64)
        chal = np.zeros(2 * cfg.num_challenges, dtype=np.uint64)
        ptrs = (C.c_void_p * 12)(*[t[1].ctypes.data for t in bad_tables])
        lgc = (C.c_uint * 12)(*lg)
        offs, err = (C.c_size_t * 13)(), C.c_char_p()
        rc = ctx.L.zkm_prove_segment(ctx.h, C.byref(cfg), ptrs, lgc, None, 0, proofs.ctypes.data_as(zkm.u64p), offs, chal.ctypes.data_as(zkm.u64p),
                                     C.byref(err))
        assert rc != 0 and b"segment 0" in err.value and b"CTL #14" in err.value and b"is present 1 times in the looking tables" in err.value
        assert not proofs.any() and not chal.any()
        with pytest.raises(zkm.ZkmError, match="CTL #14"):
            ctx.prove_with_traces(bad_tables, ctls)
        # zkm_prove_segment_ops on broken operations
        ops = SF.segment_ops(zkm, bad_raw)
        st = ops.struct()
        proofs = np.zeros(good[2][12], dtype=np.uint64)
        rc = ctx.L.zkm_prove_segment_ops(ctx.h, C.byref(cfg), C.byref(st), None, 0, proofs.ctypes.data_as(zkm.u64p), offs,
                                         chal.ctypes.data_as(zkm.u64p), C.byref(err))
        assert rc != 0 and ("CTL #%d" % c).encode() in err.value and b"segment 0" in err.value, err.value
        assert not proofs.any() and not chal.any()
        # three segments, the second broken
        with pytest.raises(zkm.ZkmError, match=r"segment 1: CTL #%d" % c):
            ctx.prove_segments_ops([SF.segment_ops(zkm, raw), SF.segment_ops(zkm, bad_raw), SF.segment_ops(zkm, raw)])
        with pytest.raises(zkm.ZkmError, match=r"segment 1: CTL #14"):
            ctx.prove_segments([([t[1] for t in tb], lg, ()) for tb in (tables, bad_tables, tables)])
        three = ctx.prove_segments_ops([SF.segment_ops(zkm, raw)] * 3, public_values=[[1, 2]] * 3)
        for s in range(3):
            for a, b in zip(good, three[s]):
                assert np.array_equal(np.asarray(a), np.asarray(b))
    finally:
        ctx.set_tuning("check_ctls", 0)
    ctx.prove_segment_ops(SF.segment_ops(zkm, bad_raw))          # off again: no check


# ---- 8. launch accounting
def test_every_launch_serves_all_lookups_and_the_host_waits_do_not_depend_on_them(ctx, seg):
    raw, tables, ctls = seg
    ctx.profile(True)
    try:
        def run(lookups):
            ctx.profile_reset()
            rep = ctx.check_ctls(tables, lookups)
            ctx.synchronize()
            return rep, {k: v[0] for k, v in ctx.profile_records().items() if k.startswith("check_ctls/")}
        rep15, rec15 = run(ctls)
        rep1, rec1 = run(ctls[13:14])
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    print(rec15, rep15.host_waits)
    assert len(ctls) == 15 and rep15.kind == 0 and rep1.kind == 0
    for k in ("check_ctls/radix_upsweep", "check_ctls/radix_scan", "check_ctls/radix_downsweep"):
        assert rec15[k] == 16 and rec1[k] == 16, (k, rec15, rec1)       # 128-bit keys, 8 bits a pass: once per pass for the whole call
    for k in ("check_ctls/count", "check_ctls/emit", "check_ctls/keys", "check_ctls/flags", "check_ctls/mark", "check_ctls/verdict"):
        assert rec15[k] == 1 and rec1[k] == 1, (k, rec15, rec1)
    assert rec15 == rec1
    assert rep15.host_waits == rep1.host_waits == 2                      # the record counts, the verdict
    bad = ctx.check_ctls(M.bump(tables, MEMORY, word(tables, MEMORY, MEM_VALUE, filtered_memory_row(tables, 5))), ctls)
    assert bad.kind == 2 and bad.host_waits == 3                         # ... and the report
