"""GPU suite: zkm_segments_tables / zkm_prove_segments_ops / zkm_segment_ops_stage / zkm_pool_prove_segments_ops -- K segments built from
their raw operations in one set of launches and proven in lock-step in the same call.  Every result is defined as "word for word what
the single-segment call returns for that segment alone", so every comparison here is exact: heights, tables, proof offsets,
challenges and proof words against zkm_segment_tables / zkm_prove_segment_ops (and, once, the oracle); the launch count against the
single-segment builds; every kind of input memory; staged lists consumed while their upload is in flight; every refusal with the
segment's position; waves; the pool.

A segment that is PROVEN needs CPU rows whose lookup filters are 0 or 1 (the prover refuses "Non-binary filter?" otherwise, as the
reference does), which random 64-bit CPU words are not: the proven segments below take the CPU rows of the sample program
(real_cpu_rows), tiled to the height they need.  Segments that are only built keep random CPU words."""

import numpy as np
import pytest

from . import arith_fixtures as A
from . import segment_ops_fixtures as SF
from .test_gpu_segment_ops import assert_tables_equal, tables_of

pytestmark = pytest.mark.gpu

P = SF.P
SMALL = [16, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 7]     # the least heights random_segment_ops gives


def empty_segment_raw(log_cpu=6):
    """A segment whose precompile, Logic and Arithmetic lists are all empty: three memory operations and random CPU rows."""
    rng = np.random.default_rng(3)
    e8, e64 = np.zeros(0, np.uint8), np.zeros(0, np.uint64)
    mem = np.array([[0, 2, 5, 1, 0, 7], [0, 2, 5, 2, 1, 7], [0, 2, 9, 3, 0, 11]], dtype=np.uint64)
    three = (np.zeros((0, 8), np.uint32), np.zeros((0, 64), np.uint32), np.zeros((0, 8), np.uint64))
    return {"cpu_rows": rng.integers(0, 1 << 64, (1 << log_cpu, 259), dtype=np.uint64), "arithmetic": np.zeros((0, 3), np.uint32),
            "logic": np.zeros((0, 3), np.uint32), "memory": mem, "poseidon": (np.zeros((0, 12), np.uint64), e64),
            "poseidon_sponge": (e8, np.zeros(1, np.uint64), np.zeros((0, 4), np.uint64)), "keccak": (np.zeros((0, 25), np.uint64), e64),
            "keccak_sponge": (e8, np.zeros(1, np.uint64), np.zeros((0, 4), np.uint64)), "sha_extend": (np.zeros((0, 16), np.uint8), e64),
            "sha_extend_sponge": (np.zeros((0, 16), np.uint32), np.zeros((0, 4), np.uint64)), "sha_compress": three,
            "sha_compress_sponge": three, "log_arithmetic": 16, "log_memory": 2}


_REAL = {}


def real_cpu_rows(oracle, nrows):
    """nrows CPU rows of the sample program, repeated as often as it takes (every row's lookup filters are 0 or 1)."""
    if "rows" not in _REAL:
        _REAL["rows"] = SF.build_segment_ops(oracle)[0]["cpu_rows"].reshape(-1, 259)
    rows = _REAL["rows"]
    return np.ascontiguousarray(np.tile(rows, ((nrows + len(rows) - 1) // len(rows), 1))[:nrows])


def provable(oracle, raw):
    return dict(raw, cpu_rows=real_cpu_rows(oracle, len(raw["cpu_rows"])))


def empty_segment_tables(oracle, raw):
    """The oracle's twelve tables of empty_segment_raw (padding only, but for the CPU rows and the Memory table)."""
    zeros = lambda w: np.zeros(w << 6, np.uint64)
    return [A.generate_trace([], 16), np.ascontiguousarray(SF.canonical(raw["cpu_rows"]).T).reshape(-1),
            oracle.poseidon_trace_inputs(np.zeros((0, 12), np.uint64), np.zeros(0, np.uint64), 6), zeros(110), zeros(2431), zeros(470),
            zeros(78), zeros(76), zeros(224), zeros(127), zeros(69), oracle.memory_trace(raw["memory"], 2)[0]]


@pytest.fixture(scope="module")
def three(oracle):
    """Three segments of different heights: (raw, the oracle's tables, log_ns) each, and the first one's (tables, ctls) for the oracle."""
    out = []
    full = None
    for repeat in (1, 2):
        raw, tables, ctls = SF.build_segment_ops(oracle, repeat=repeat)
        full = full or (tables, ctls)
        out.append((raw, [t[1] for t in tables], [t[3] for t in tables]))
    raw = provable(oracle, empty_segment_raw())
    out.append((raw, empty_segment_tables(oracle, raw), SF.reference_log_ns(raw)))
    assert len({tuple(lg) for _, _, lg in out}) == 3
    return out, full


PUBS = [[1, 2, 3], [7, 1], [9]]


def test_three_segments_of_different_heights_in_one_call(ctx, zkm, three):
    segs, _ = three
    ops = [SF.segment_ops(zkm, raw) for raw, _, _ in segs]
    assert ctx.segments_heights(ops) == [lg for _, _, lg in segs] == [SF.reference_log_ns(raw) for raw, _, _ in segs]
    alone = []
    for o, (_, _, lg) in zip(ops, segs):
        st, got_lg = ctx.segment_tables(o)
        assert got_lg == lg
        alone.append(tables_of(st, lg, ctx))
        st.free()
    live = ctx.memory()[0]
    built = ctx.segments_tables(ops)
    assert len(built) == 3
    for (st, lg), (_, want, want_lg), one in zip(built, segs, alone):
        assert lg == want_lg and st.ready()
        got = tables_of(st, lg, ctx)
        assert_tables_equal(got, want)
        assert_tables_equal(got, one)
    for st, _ in reversed(built):          # each handle is a block of its own
        st.free()
    assert ctx.memory()[0] == live


def test_proofs_equal_the_single_segment_call_and_the_oracle(ctx, zkm, oracle, three):
    segs, (tables, ctls) = three
    ops = [SF.segment_ops(zkm, raw) for raw, _, _ in segs]
    alone = [ctx.prove_segment_ops(o, public_values=pub) for o, pub in zip(ops, PUBS)]
    got = ctx.prove_segments_ops(ops, public_values=PUBS)
    assert ctx.prove_segments_ops_sizes(ops, public_values=PUBS) == [o for _, _, o in got] == [o for _, _, o in alone]
    for s, ((p, c, o), (pa, ca, oa)) in enumerate(zip(got, alone)):
        assert o == oa and (c == ca).all(), s
        bad = np.nonzero(p != pa)[0]
        assert bad.size == 0, "segment %d: first differing proof word %d" % (s, bad[0])
    want, wchal, woffs = oracle.prove_with_traces(tables, ctls, public_values=PUBS[0])
    assert got[0][2] == woffs and (got[0][1] == wchal).all() and (got[0][0] == want).all()
    assert oracle.verify_all(tables, ctls, got[0][0], got[0][1], public_values=PUBS[0]) == 0
    (p1, c1, o1), = ctx.prove_segments_ops(ops[1:2], public_values=PUBS[1:2])
    assert o1 == alone[1][2] and (c1 == alone[1][1]).all() and (p1 == alone[1][0]).all()


SCOPES = ("memory_trace/", "arithmetic_trace/", "segment_ops/cpu_rows_to_cols", "poseidon_trace", "poseidon_sponge_trace", "keccak_trace",
          "keccak_sponge_trace", "sha_extend_trace", "sha_extend_sponge_trace", "sha_compress_trace", "sha_compress_sponge_trace", "logic_trace")


def build_records(ctx, ops_list):
    """Profile records (scope -> count) of one segments_tables call, the generation scopes only."""
    ctx.profile_reset()
    for st, _ in ctx.segments_tables(ops_list):
        st.free()
    return {k: n for k, (n, _) in ctx.profile_records().items() if k.startswith(SCOPES)}


def test_launches_do_not_grow_with_the_number_of_segments(ctx, zkm, three):
    segs, _ = three
    raws = [raw for raw, _, _ in segs] + [SF.random_segment_ops(SMALL, seed=21)]
    dev = [SF.segment_ops(zkm, raw).to_device(ctx) for raw in raws]
    ctx.profile(True)
    try:
        alone = [build_records(ctx, [o]) for o in dev]
        four = build_records(ctx, dev)
    finally:
        ctx.profile(False)
        for o in dev:
            o.free()
    scopes = set().union(*alone)
    assert {"memory_trace/sort", "memory_trace/rows", "arithmetic_trace/rows", "segment_ops/cpu_rows_to_cols", "keccak_trace", "logic_trace",
            "keccak_sponge_trace", "poseidon_sponge_trace"} <= scopes
    assert set(four) == scopes
    for k in sorted(scopes):
        most = max(a.get(k, 0) for a in alone)
        print("%-32s four segments %d, most alone %d" % (k, four[k], most))
        assert 1 <= four[k] <= most, k


def test_pageable_pinned_and_device_lists_in_one_call(ctx, zkm, three):
    segs, _ = three
    raws = []
    for raw, _, _ in segs:                  # GoldilocksField words x + p for x < 2^32 - 1 (a u64 that is not reduced): the same table
        cpu = raw["cpu_rows"].copy()
        small = cpu < np.uint64((1 << 32) - 1)
        cpu[small] += np.uint64(P)
        assert small.any() and (cpu[small] >= np.uint64(P)).all()
        raws.append(dict(raw, cpu_rows=cpu))
    pageable = SF.segment_ops(zkm, raws[0])
    pinned = SF.segment_ops(zkm, raws[1]).to_pinned(ctx)
    dev = SF.segment_ops(zkm, raws[2]).to_device(ctx)
    try:
        built = ctx.segments_tables([pageable, pinned, dev])
        for (st, lg), (_, want, want_lg) in zip(built, segs):
            assert lg == want_lg
            assert_tables_equal(tables_of(st, lg, ctx), want)
            st.free()
    finally:
        dev.free()
        for k, v in pinned.lists.items():
            if not k.endswith("_off"):
                ctx.free_pinned(v)


def test_staged_operations_consumed_while_their_upload_is_in_flight(ctx, zkm, oracle):
    """Two segments of the 2^16-cycle shape in pinned memory, staged and proven at once (no ready(wait=True) between): the shape of the
    race found for staged tables -- pinned memory, the upload still in flight, the lanes starting.  Run once, judged by its words.
    Then the handle owns all it hands out: the caller's lists, offsets included, are overwritten and the tables do not change."""
    from tools.bench_segment import HEIGHTS
    raws = [provable(oracle, SF.random_segment_ops(HEIGHTS[16], seed=s)) for s in (31, 32)]
    for raw in raws:                        # (to_pinned shares the offset arrays with its source: own copies, to overwrite below)
        for g in ("poseidon_sponge", "keccak_sponge"):
            raw[g] = (raw[g][0], raw[g][1].copy(), raw[g][2])
    pinned = [SF.segment_ops(zkm, raw).to_pinned(ctx) for raw in raws]
    pubs = [[3, 1], [3, 2]]
    try:
        direct = ctx.prove_segments_ops(pinned, public_values=pubs)
        staged = [ctx.stage_segment_ops(o) for o in pinned]
        got = ctx.prove_segments_ops([s.ops() for s in staged], public_values=pubs)
        for s, ((p, c, o), (pd, cd, od)) in enumerate(zip(got, direct)):
            assert o == od and (c == cd).all(), s
            bad = np.nonzero(p != pd)[0]
            assert bad.size == 0, "segment %d: first differing proof word %d" % (s, bad[0])
        assert all(s.ready(wait=True) for s in staged)

        def tables():
            out = []
            for st, lg in ctx.segments_tables([s.ops() for s in staged]):
                assert lg == HEIGHTS[16]
                out.append(tables_of(st, lg, ctx))
                st.free()
            return out
        before = tables()
        for o in pinned:
            for v in o.lists.values():
                v[...] = 0xFF if v.dtype == np.uint8 else 0xFFFFFFFF
        after = tables()
        for b, a in zip(before, after):
            assert_tables_equal(a, b)
        for s in staged:
            s.free()
    finally:
        for o in pinned:
            for k, v in o.lists.items():
                if not k.endswith("_off"):
                    ctx.free_pinned(v)


class RawOps:
    """A zkm_segment_ops filled in by hand (what SegmentOps cannot express: a device pointer where host memory is required)."""

    def __init__(self, st, keep):
        self.st, self.keep = st, keep

    def struct(self):
        return self.st


def test_refusals_name_the_segment_and_leave_nothing_behind(ctx, zkm, oracle):
    base = provable(oracle, empty_segment_raw())
    good = [SF.segment_ops(zkm, provable(oracle, SF.random_segment_ops(SMALL, seed=41))), SF.segment_ops(zkm, base)]
    want = [ctx.prove_segment_ops(o, public_values=[5]) for o in good]
    mem_p = base["memory"].copy()
    mem_p[1, 2] = P
    dev_off = ctx.alloc(2).upload(np.array([0, 8], np.uint64))
    keep = SF.segment_ops(zkm, dict(base, poseidon_sponge=(np.zeros(8, np.uint8), np.array([0, 8], np.uint64), np.zeros((1, 4), np.uint64))))
    st = keep.struct()
    st.poseidon_sponge_off = dev_off.ptr
    cases = [("Logic", SF.segment_ops(zkm, dict(base, logic=np.array([[1, 2, 3], [4, 5, 6]], np.uint32)))),
             ("Memory", SF.segment_ops(zkm, dict(base, memory=mem_p))),
             ("KeccakSponge", SF.segment_ops(zkm, dict(base, keccak_sponge=(np.zeros(8, np.uint8), np.array([0, 8, 8], np.uint64), np.zeros((2, 4), np.uint64))))),
             ("Cpu", SF.segment_ops(zkm, dict(base, cpu_rows=base["cpu_rows"][:48]))),
             ("PoseidonSponge", RawOps(st, keep)),
             ("Memory", SF.segment_ops(zkm, dict(base, memory=np.zeros((0, 6), np.uint64))))]
    ctx.prove_segments_ops(good, public_values=[[5], [5]])      # (the tables a lock-step call keeps resident exist from here on)
    live = ctx.memory()[0]
    for table, bad in cases:
        ops = [good[0], bad, good[1]]
        for call in (lambda: ctx.segments_tables(ops), lambda: ctx.prove_segments_ops(ops, public_values=[[5], [5], [5]])):
            with pytest.raises(zkm.ZkmError, match="segment 1: %s" % table):
                call()
            assert ctx.memory()[0] == live, table
        got = ctx.prove_segments_ops(good, public_values=[[5], [5]])
        for (p, c, o), (pa, ca, oa) in zip(got, want):
            assert o == oa and (c == ca).all() and (p == pa).all(), table
        assert ctx.memory()[0] == live, table
    for call in (lambda: ctx.segments_tables([]), lambda: ctx.prove_segments_ops([], public_values=[])):
        with pytest.raises(zkm.ZkmError, match="no segments"):
            call()
    # a staged handle belongs to its context
    other = zkm.Context(0)
    try:
        with ctx.stage_segment_ops(good[1]) as staged:
            with pytest.raises(zkm.ZkmError, match="another context"):
                other.segments_tables([staged.ops()])
            ctx.segments_tables([staged.ops()])[0][0].free()
    finally:
        other.close()
    assert ctx.memory()[0] == live
    dev_off.free()


def test_waves_do_not_change_the_words(ctx, zkm, three):
    segs, _ = three
    ops = [SF.segment_ops(zkm, raw) for raw, _, _ in segs]
    want = ctx.prove_segments_ops(ops, public_values=PUBS)
    for key, value, back in (("segments_memory_budget", 1, 0), ("max_stack", 2, 32)):
        ctx.set_tuning(key, value)
        try:
            got = ctx.prove_segments_ops(ops, public_values=PUBS)
        finally:
            ctx.set_tuning(key, back)
        for (p, c, o), (pa, ca, oa) in zip(got, want):
            assert o == oa and (c == ca).all() and (p == pa).all(), key


def test_pool_takes_operations(ctx, zkm, oracle):
    raws = [provable(oracle, SF.random_segment_ops(SMALL, seed=50 + s)) for s in range(5)]
    ops = [SF.segment_ops(zkm, raw) for raw in raws]
    pubs = [[s, 4] for s in range(5)]
    want = [ctx.prove_segment_ops(o, public_values=pub) for o, pub in zip(ops, pubs)]
    pool = zkm.Pool((0,), 2)
    try:
        got = pool.prove_segments_ops(ops, public_values=pubs, max_stack=2)
        for s, ((p, c, o), (pa, ca, oa)) in enumerate(zip(got, want)):
            assert o == oa and (c == ca).all() and (p == pa).all(), s
        placed = [pool.last_assignment(s) for s in range(5)]
        assert {w for w, _ in placed} <= {0, 1} and len({g for _, g in placed}) == len(zkm.pool_plan(5, 2, 2))
        bad = SF.segment_ops(zkm, dict(raws[3], logic=np.array([[1, 2, 3], [4, 5, 6]], np.uint32)))
        with pytest.raises(zkm.ZkmError, match=r"worker \d+ \(device 0\), segments \d+\.\.\d+: .*segment 3: Logic"):
            pool.prove_segments_ops(ops[:3] + [bad] + ops[4:], public_values=pubs, max_stack=2)
        got = pool.prove_segments_ops(ops, public_values=pubs, max_stack=2)
        assert all((p == pa).all() for (p, _, _), (pa, _, _) in zip(got, want))
    finally:
        pool.close()
