"""GPU suite: zkm_segment_tables / zkm_prove_segment_ops -- a whole segment's twelve tables built on the device from its raw operations
(Traces::into_tables, witness/traces.rs:230-320) against the oracle's generators at the reference's heights, its proof against the
oracle's and prove_segment's, every kind of input memory, lock-step proving of built segments, padding-only tables, the 2^16-cycle
shape against the per-table entry points, and every refusal."""
import numpy as np
import pytest

from . import segment_ops_fixtures as SF

pytestmark = pytest.mark.gpu

P = SF.P
WIDTHS = [54, 259, 262, 110, 2431, 470, 78, 76, 224, 127, 69, 13]


@pytest.fixture(scope="module")
def seg(oracle):
    return SF.build_segment_ops(oracle)


def tables_of(staged, log_ns, ctx):
    """The twelve device matrices of a built segment, downloaded."""
    from zkm_amd import DeviceBuffer
    out = []
    for ptr, w, lg in zip(staged.tables(), WIDTHS, log_ns):
        buf = DeviceBuffer.__new__(DeviceBuffer)
        buf.ctx, buf.words, buf.ptr = ctx, w << lg, ptr
        out.append(buf.download())
    return out


def assert_tables_equal(got, want):
    for t, (g, w) in enumerate(zip(got, want)):
        assert g.size == w.size, t
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "table %d (Table::all() order): first differing word %d" % (t, bad[0])


def test_full_segment_tables_word_for_word(ctx, zkm, seg):
    raw, tables, _ = seg
    ops = SF.segment_ops(zkm, raw)
    assert ctx.segment_heights(ops) == [t[3] for t in tables] == SF.reference_log_ns(raw)
    live = ctx.memory()[0]
    with ctx.segment_tables(ops)[0] as staged:
        assert staged.ready() and staged.ready(wait=True)
        assert_tables_equal(tables_of(staged, [t[3] for t in tables], ctx), [t[1] for t in tables])
    assert ctx.memory()[0] == live


def test_prove_segment_ops_equals_the_oracle_and_prove_segment(ctx, zkm, oracle, seg):
    raw, tables, ctls = seg
    want, wchal, woffs = oracle.prove_with_traces(tables, ctls, public_values=[1, 2, 3])
    got, chal, offs = ctx.prove_segment_ops(SF.segment_ops(zkm, raw), public_values=[1, 2, 3])
    assert offs == woffs and (chal == wchal).all()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first differing word %d" % bad[0]
    p2, c2, o2 = ctx.prove_segment([t[1] for t in tables], [t[3] for t in tables], public_values=[1, 2, 3])
    assert o2 == offs and (c2 == chal).all() and (p2 == got).all()
    assert oracle.verify_all(tables, ctls, got, chal, public_values=[1, 2, 3]) == 0


def test_pageable_pinned_and_device_inputs_and_noncanonical_cpu_words(ctx, zkm, seg):
    raw, tables, _ = seg
    lg = [t[3] for t in tables]
    ops = SF.segment_ops(zkm, raw)
    want = [t[1] for t in tables]
    pinned = ops.to_pinned(ctx)
    dev = ops.to_device(ctx)
    try:
        for o in (pinned, dev):
            st, got_lg = ctx.segment_tables(o)
            assert got_lg == lg
            assert_tables_equal(tables_of(st, lg, ctx), want)
            st.free()
    finally:
        dev.free()
        for k, v in pinned.lists.items():
            if not k.endswith("_off"):
                ctx.free_pinned(v)
    # GoldilocksField words x + p for x < 2^32 - 1 (a u64 that is not reduced): the same table
    cpu = raw["cpu_rows"].copy()
    small = cpu < np.uint64((1 << 32) - 1)
    cpu[small] += np.uint64(P)
    assert small.any() and (cpu[small] >= np.uint64(P)).all()
    raw2 = dict(raw, cpu_rows=cpu)
    for o in (SF.segment_ops(zkm, raw2), SF.segment_ops(zkm, raw2).to_device(ctx)):
        st, _ = ctx.segment_tables(o)
        assert (tables_of(st, lg, ctx)[1] == want[1]).all()
        st.free()
        o.free()


def test_two_built_segments_proven_in_lock_step(ctx, zkm, oracle, seg):
    raw1, tables1, _ = seg
    raw2, tables2, _ = SF.build_segment_ops(oracle, repeat=2)
    assert [t[3] for t in tables1] != [t[3] for t in tables2]
    ops = [SF.segment_ops(zkm, raw1), SF.segment_ops(zkm, raw2)]
    alone = [ctx.prove_segment_ops(o, public_values=[7, s]) for s, o in enumerate(ops)]
    built = [ctx.segment_tables(o) for o in ops]
    res = ctx.prove_segments([(st.tables(), lg, [7, s]) for s, (st, lg) in enumerate(built)])
    for (st, _), (p, c, o), (pa, ca, oa) in zip(built, res, alone):
        assert o == oa and (c == ca).all() and (p == pa).all()
        st.free()


def empty_segment_raw(log_cpu=6):
    rng = np.random.default_rng(3)
    e8, e64 = np.zeros(0, np.uint8), np.zeros(0, np.uint64)
    mem = np.array([[0, 2, 5, 1, 0, 7], [0, 2, 5, 2, 1, 7], [0, 2, 9, 3, 0, 11]], dtype=np.uint64)
    return {"cpu_rows": rng.integers(0, 1 << 64, (1 << log_cpu, 259), dtype=np.uint64), "arithmetic": np.zeros((0, 3), np.uint32),
            "logic": np.zeros((0, 3), np.uint32), "memory": mem, "poseidon": (np.zeros((0, 12), np.uint64), e64),
            "poseidon_sponge": (e8, np.zeros(1, np.uint64), np.zeros((0, 4), np.uint64)), "keccak": (np.zeros((0, 25), np.uint64), e64),
            "keccak_sponge": (e8, np.zeros(1, np.uint64), np.zeros((0, 4), np.uint64)), "sha_extend": (np.zeros((0, 16), np.uint8), e64),
            "sha_extend_sponge": (np.zeros((0, 16), np.uint32), np.zeros((0, 4), np.uint64)),
            "sha_compress": (np.zeros((0, 8), np.uint32), np.zeros((0, 64), np.uint32), np.zeros((0, 8), np.uint64)),
            "sha_compress_sponge": (np.zeros((0, 8), np.uint32), np.zeros((0, 64), np.uint32), np.zeros((0, 8), np.uint64))}


def test_empty_precompile_lists_give_padding_tables(ctx, zkm, oracle):
    from . import arith_fixtures as A
    raw = empty_segment_raw()
    staged, lg = ctx.segment_tables(SF.segment_ops(zkm, raw))
    memory, natural = oracle.memory_trace(raw["memory"], 6)
    assert natural == 4
    assert lg == [16, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 2]
    want = [A.generate_trace([], 16), np.ascontiguousarray(SF.canonical(raw["cpu_rows"]).T).reshape(-1),
            oracle.poseidon_trace_inputs(np.zeros((0, 12), np.uint64), np.zeros(0, np.uint64), 6),
            np.zeros(110 << 6, np.uint64), np.zeros(2431 << 6, np.uint64), np.zeros(470 << 6, np.uint64), np.zeros(78 << 6, np.uint64),
            np.zeros(76 << 6, np.uint64), np.zeros(224 << 6, np.uint64), np.zeros(127 << 6, np.uint64), np.zeros(69 << 6, np.uint64),
            oracle.memory_trace(raw["memory"], 2)[0]]
    got = tables_of(staged, lg, ctx)
    staged.free()
    assert_tables_equal(got, want)
    po = got[2].reshape(262, 64)
    assert (po[0] == 0).all() and (po[13:25] != 0).any()          # filter 0, the permutation of zero in every row
    assert (po[:, 0] == po[:, 63]).all()


def per_table(ctx, raw, lg):
    """The eleven per-table entry points at the heights lg, plus the CPU rows transposed in numpy: the path a caller takes today."""
    out = [ctx.arithmetic_trace(raw["arithmetic"], lg[0])[0], None, ctx.poseidon_trace_inputs(*raw["poseidon"], lg[2]),
           ctx.poseidon_sponge_trace(*raw["poseidon_sponge"], lg[3])[0], ctx.keccak_trace(*raw["keccak"], lg[4]),
           ctx.keccak_sponge_trace(*raw["keccak_sponge"], lg[5])[0], ctx.sha_extend_trace(*raw["sha_extend"], lg[6]),
           ctx.sha_extend_sponge_trace(*raw["sha_extend_sponge"], lg[7]), ctx.sha_compress_trace(*raw["sha_compress"], lg[8]),
           ctx.sha_compress_sponge_trace(*raw["sha_compress_sponge"], lg[9]), ctx.logic_trace(raw["logic"], lg[10]),
           ctx.memory_trace(raw["memory"], lg[11])[0]]
    host = []
    for t, b in enumerate(out):
        if b is None:
            host.append(np.ascontiguousarray(SF.canonical(raw["cpu_rows"]).T).reshape(-1))
        else:
            host.append(b.download())
            b.free()
    return host


def test_bench_shape_equals_the_per_table_calls(ctx, zkm):
    from tools.bench_segment import HEIGHTS
    raw = SF.random_segment_ops(HEIGHTS[16], seed=11)
    ops = SF.segment_ops(zkm, raw)
    staged, lg = ctx.segment_tables(ops)
    assert lg == HEIGHTS[16]
    got = tables_of(staged, lg, ctx)
    staged.free()
    assert_tables_equal(got, per_table(ctx, raw, lg))


def refusal_cases():
    base = empty_segment_raw()
    yield "Cpu", dict(base, cpu_rows=base["cpu_rows"][:48])
    yield "Cpu", dict(base, cpu_rows=base["cpu_rows"][:0])
    yield "Memory", dict(base, memory=np.zeros((0, 6), np.uint64))
    yield "Logic", dict(base, logic=np.array([[1, 2, 3], [4, 5, 6]], np.uint32))
    yield "Arithmetic", dict(base, arithmetic=np.array([[0, 1, 2], [26, 1, 2]], np.uint32))
    yield "KeccakSponge", dict(base, keccak_sponge=(np.zeros(8, np.uint8), np.array([0, 8, 8], np.uint64), np.zeros((2, 4), np.uint64)))
    yield "PoseidonSponge", dict(base, poseidon_sponge=(np.zeros(8, np.uint8), np.array([0, 0], np.uint64), np.zeros((1, 4), np.uint64)))


def test_refusals_name_the_table_and_leave_nothing_behind(ctx, zkm):
    import ctypes as C
    good = SF.segment_ops(zkm, empty_segment_raw())
    ctx.segment_tables(good)[0].free()
    live = ctx.memory()[0]
    for table, raw in refusal_cases():
        ops = SF.segment_ops(zkm, raw)
        for call in (lambda: ctx.segment_tables(ops), lambda: ctx.prove_segment_ops(ops)):
            with pytest.raises(zkm.ZkmError, match=table):
                call()
            assert ctx.memory()[0] == live, table
            ctx.segment_tables(good)[0].free()
    # a null pointer with a nonzero count, more CPU rows than 2^28 and, for every other table with a data-parallel writer, a count that
    # by itself needs more than 2^28 rows (every one refused before a list is read: the pointers only have to be non-null)
    somewhere = good.struct().cpu_rows
    cases = [("Keccak: null pointer with a nonzero count", dict(keccak_inputs=None, nkeccak=3)), ("Cpu", dict(ncpu_rows=1 << 29))]
    for table, group, rows_per_op in (("Poseidon", "poseidon", 1), ("Keccak", "keccak", 24), ("ShaExtend", "sha_extend", 1),
                                      ("ShaExtendSponge", "sha_extend_sponge", 48), ("ShaCompress", "sha_compress", 65),
                                      ("ShaCompressSponge", "sha_compress_sponge", 1), ("Logic", "logic", 1)):
        lists, count = next((ptrs, count) for name, ptrs, count in zkm.SEGMENT_OPS_GROUPS if name == group)
        fields = {name: somewhere for name, _ in lists}
        fields[count] = (1 << 28) // rows_per_op + 1
        cases.append((table + ": the operations need more than 2^28 rows", fields))
    for text, fields in cases:
        st = good.struct()
        for name, value in fields.items():
            setattr(st, name, value)
        lg, h, err = (C.c_uint * 12)(), C.c_void_p(), C.c_char_p()
        cfg = ctx.standard_config()
        assert ctx.L.zkm_segment_tables(ctx.h, C.byref(cfg), C.byref(st), lg, C.byref(h), C.byref(err)) == 1
        assert text in err.value.decode() and not h.value
        assert ctx.memory()[0] == live
    ctx.segment_tables(good)[0].free()
