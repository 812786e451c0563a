"""GPU suite: zkm_arithmetic_trace (csrc/arithmetic_trace.hip), ArithmeticStark::generate_trace (arithmetic_stark.rs:127-185) from the
raw operations, word for word against arith_fixtures.generate_trace -- every operator, the 2^16 boundary, host and device input,
the reference's basic_trace test, every failure -- and the GPU table in the range-check lookup and in segment proofs."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from . import arith_fixtures as A
from . import cpu_fixtures as CF

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EDGES = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xFFFF8000]
IMM_OPS = (A.IS_ADDI, A.IS_ADDIU, A.IS_SLTI, A.IS_SLTIU)
SHIFT_CAPPED = (A.IS_SLL, A.IS_SRL, A.IS_SRA, A.IS_SRAV)
TWO_ROWS = (A.IS_DIV, A.IS_DIVU, A.IS_SRL, A.IS_SRLV, A.IS_SRA, A.IS_SRAV)


def valid_ops(seed, count, which=None):
    """count x 3 uint32 operations in the reference's domain: sign-extended immediates, shifts below 32 where result() needs them,
    no zero divisor and no i32::MIN / -1; edge values on both inputs, SLLV / SRLV shifts of 32 and more."""
    rng = np.random.default_rng(seed)
    which = np.arange(26) if which is None else np.asarray(which)
    op = which[rng.integers(0, len(which), count)].astype(np.uint32)
    a = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
    edge_a, edge_b = rng.random(count) < 0.25, rng.random(count) < 0.25
    a[edge_a] = rng.choice(EDGES, int(edge_a.sum()))
    b[edge_b] = rng.choice(EDGES, int(edge_b.sum()))
    imm = np.isin(op, IMM_OPS)
    b[imm] = (b[imm] & 0xFFFF).astype(np.int16).astype(np.int32).astype(np.uint32)
    capped = np.isin(op, SHIFT_CAPPED)
    b[capped] &= 31
    var = np.isin(op, (A.IS_SLLV, A.IS_SRLV))
    small = var & (rng.random(count) < 0.5)
    b[small] &= 63                                    # half of SLLV / SRLV shifts in 0 .. 63: 32 and more included
    div = np.isin(op, (A.IS_DIV, A.IS_DIVU))
    b[div & (b == 0)] = 3
    b[(op == A.IS_DIV) & (a == 0x80000000) & (b == 0xFFFFFFFF)] = 7
    return np.ascontiguousarray(np.stack([op, a, b], axis=1))


def to_device(ctx, ops):
    """ops packed into a DeviceBuffer of ceil(3 nops / 2) words."""
    flat = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1)
    if flat.size & 1:
        flat = np.concatenate([flat, np.zeros(1, dtype=np.uint32)])
    words = flat.view(np.uint64)
    return ctx.alloc(max(words.size, 1)).upload(words)


def gpu_table(ctx, ops, log_n=None, device=False):
    src = to_device(ctx, ops) if device else ops
    try:
        buf, natural = ctx.arithmetic_trace(src, log_n, nops=len(ops) if device else None)
    finally:
        if device:
            src.free()
    got = buf.download()
    buf.free()
    return got, natural


def fixture_rows(ops):
    return sum(2 if int(o) in TWO_ROWS else 1 for o in np.asarray(ops).reshape(-1, 3)[:, 0])


def natural_of(rows):
    return max(1 << 16, 1 << max(rows - 1, 0).bit_length())


def check_equal(got, want, log_n):
    assert got.size == want.size == 54 << log_n
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first differing word: column %d row %d (%d differ)" % (bad[0] >> log_n, bad[0] & ((1 << log_n) - 1), bad.size)


def check_against_fixture(ctx, ops, log_n=None, devices=(False, True)):
    rows = fixture_rows(ops)
    ln = log_n if log_n is not None else natural_of(rows).bit_length() - 1
    want = A.generate_trace([tuple(int(v) for v in o) for o in ops], ln)
    for device in devices:
        got, natural = gpu_table(ctx, ops, log_n, device)
        assert natural == natural_of(rows)
        check_equal(got, want, ln)
    return want.reshape(54, -1)


@pytest.mark.parametrize("op", range(26))
def test_each_operator(ctx, op):
    ops = valid_ops(100 + op, 700, [op])
    check_against_fixture(ctx, ops)


@pytest.mark.parametrize("nops", [0, 1, 2, 1000, 1 << 15, (1 << 16) - 1, 1 << 16])
def test_mixed_ops(ctx, nops):
    ops = valid_ops(nops, nops)
    tr = check_against_fixture(ctx, ops)
    if nops == (1 << 16) - 1:
        assert fixture_rows(ops) > 1 << 16 and tr.shape[1] == 1 << 17   # rows spill past 2^16


def test_log_n_above_natural(ctx):
    ops = valid_ops(7, 3000)
    check_against_fixture(ctx, ops, log_n=18)
    check_against_fixture(ctx, np.zeros((0, 3), dtype=np.uint32), log_n=17, devices=(False,))


def test_reference_basic_trace_kat(ctx):
    """arithmetic_stark.rs basic_trace: eight operations, OUTPUT limbs at rows 0, 1, 2, 4, 6, 8, 9, 10 of a 2^16-row table."""
    kat = json.load(open(os.path.join(HERE, "golden", "arithmetic_basic_trace.json")))
    ops = np.array(kat["ops"], dtype=np.uint32)
    got, natural = gpu_table(ctx, ops)
    assert natural == 1 << 16
    tr = got.reshape(54, -1)
    for row, limbs in kat["expected_output"]:
        assert list(tr[32:34, row]) == limbs, row
    check_against_fixture(ctx, ops)


def raw_call(ctx, ops, nops, log_n, out):
    """zkm_arithmetic_trace through ctypes: (status, natural_rows_out, message)."""
    natural = C.c_size_t(12345)
    err = C.c_char_p()
    rc = ctx.L.zkm_arithmetic_trace(ctx.h, ops, nops, log_n, out, C.byref(natural), C.byref(err))
    return rc, natural.value, (err.value or b"").decode()


def test_sizing_call(ctx):
    """out_dev NULL: max(2^16, next_pow2(rows)), log_n ignored -- including a two-row op whose second row is row 2^16."""
    for ops in (np.zeros((0, 3), dtype=np.uint32), valid_ops(3, 10), valid_ops(4, 40000)):
        rc, natural, msg = raw_call(ctx, ops.ctypes.data_as(C.c_void_p), len(ops), 99, None)
        assert rc == 0 and natural == natural_of(fixture_rows(ops)), msg
    ones = valid_ops(5, (1 << 16) - 1, [A.IS_ADD])
    for last, want in ((A.IS_ADD, 1 << 16), (A.IS_DIVU, 1 << 17)):
        ops = np.concatenate([ones, np.array([[last, 9, 4]], dtype=np.uint32)])
        rc, natural, msg = raw_call(ctx, ops.ctypes.data_as(C.c_void_p), len(ops), 0, None)
        assert rc == 0 and natural == want == natural_of(fixture_rows(ops))
        dev = to_device(ctx, ops)
        try:
            rc, natural, msg = raw_call(ctx, C.c_void_p(dev.ptr), len(ops), 0, None)
            assert rc == 0 and natural == want
        finally:
            dev.free()
    check_against_fixture(ctx, ops)   # (the DIVU's second row is row 2^16)


def _transient(ctx):
    return ctx.memory()[0] - ctx.resident_bytes()


def test_failures_leave_the_context_usable(ctx, zkm):
    """Each rule of zkm_hip.h as one failing call; after each the context still builds a correct table and its transient memory is
    unchanged.  (The shared-column rule, the assert of generate_range_checks, has no input in the domain that reaches it.)"""
    ok = valid_ops(9, 300)
    want = A.generate_trace([tuple(int(v) for v in o) for o in ok])

    def still_works():
        got, _ = gpu_table(ctx, ok)
        check_equal(got, want, 16)

    def refused(ops, match, log_n=16):
        before = _transient(ctx)
        with pytest.raises(zkm.ZkmError, match=match):
            ctx.arithmetic_trace(ops, log_n)
        assert _transient(ctx) == before
        if log_n is not None:
            with pytest.raises(zkm.ZkmError, match=match):
                ctx.arithmetic_trace(ops)
            assert _transient(ctx) == before
        still_works()

    still_works()
    small = ctx.alloc(54 << 16)
    ptr = C.c_void_p(small.ptr)
    try:
        # log_n outside [16, 28]
        for ln in (15, 29):
            rc, _, msg = raw_call(ctx, ok.ctypes.data_as(C.c_void_p), len(ok), ln, ptr)
            assert rc != 0 and "log_n" in msg
            still_works()
        # rows that do not fit: natural_rows_out is still written
        big = valid_ops(11, 40000, [A.IS_DIVU])
        rc, natural, msg = raw_call(ctx, big.ctypes.data_as(C.c_void_p), len(big), 16, ptr)
        assert rc != 0 and natural == 1 << 17 and "131072 rows" in msg
        still_works()
        cases = [((26, 1, 2), "above 25"), ((0xFFFFFFFF, 1, 2), "above 25"),
                 ((A.IS_DIV, 5, 0), "by zero"), ((A.IS_DIVU, 5, 0), "by zero"),
                 ((A.IS_DIV, 0x80000000, 0xFFFFFFFF), "overflows")]
        cases += [((op, 5, b), "immediate") for op in IMM_OPS for b in (0x8000, 0x10000, 0xFFFF7FFF)]
        cases += [((op, 5, b), "shift amount") for op in SHIFT_CAPPED for b in (32, 0xFFFFFFFF)]
        for bad_op, match in cases:
            ops = ok.copy()
            ops[123] = bad_op
            refused(ops, match)
        # out must be a device pointer
        host_out = np.zeros(54 << 16, dtype=np.uint64)
        rc, _, msg = raw_call(ctx, ok.ctypes.data_as(C.c_void_p), len(ok), 16, host_out.ctypes.data_as(C.c_void_p))
        assert rc != 0 and "device pointer" in msg and not host_out.any()
        still_works()
    finally:
        small.free()
    # the domain edges that are accepted
    edge = np.array([[A.IS_SLLV, 0x12345678, 32], [A.IS_SRLV, 0x87654321, 0xFFFFFFFF], [A.IS_SRLV, 0x87654321, 33],
                     [A.IS_LUI, 0xFFFF8001, 0], [A.IS_LUI, 0x12345678, 0], [A.IS_ADDI, 7, 0xFFFF8000], [A.IS_SLTIU, 7, 0x7FFF],
                     [A.IS_DIV, 0x80000000, 1], [A.IS_DIV, 0x7FFFFFFF, 0xFFFFFFFF], [A.IS_SRAV, 0x80000000, 31],
                     [A.IS_SRA, 0x80000000, 0], [A.IS_SLL, 0xFFFFFFFF, 31]], dtype=np.uint32)
    check_against_fixture(ctx, edge)


def layout_of(ops):
    """Each op's first row (the reference's push order) and the row count."""
    rows = np.where(np.isin(ops[:, 0], TWO_ROWS), 2, 1).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(rows)])
    return start[:-1], int(start[-1])


@pytest.mark.parametrize("log_ops", [20, 21])
def test_large_tables(ctx, zkm, log_ops):
    """2^20 and 2^21 device-resident ops, checked without the full fixture: sampled ops' rows, the padding rows, RANGE_COUNTER, and
    RC_FREQUENCIES against a bincount of the GPU table's own shared columns; at 2^20 every constraint with the range-check lookup."""
    from zkm_amd import tables as T
    from zkm_amd.ctl import CtlTable, make_zs
    nops = 1 << log_ops
    ops = valid_ops(log_ops, nops)
    start, rows = layout_of(ops)
    got, natural = gpu_table(ctx, ops, device=True)
    assert natural == natural_of(rows)
    log_n = natural.bit_length() - 1
    n = 1 << log_n
    tr = got.reshape(54, n)
    rng = np.random.default_rng(log_ops)
    for i in np.concatenate([rng.integers(0, nops, 3000), [0, nops - 1]]):
        r1, r2 = A.rows_for(*(int(v) for v in ops[i]))
        r = int(start[i])
        for k, want in enumerate([r1] + ([r2] if r2 is not None else [])):
            w = np.array(want, dtype=np.uint64)
            keep = np.ones(54, dtype=bool)
            keep[[A.RANGE_COUNTER, A.RC_FREQ]] = False
            assert (tr[keep, r + k] == w[keep]).all(), (i, k)
    idx = np.arange(n, dtype=np.uint64)
    keep = np.ones(54, dtype=bool)
    keep[[A.RANGE_COUNTER, A.RC_FREQ]] = False
    for c in np.nonzero(keep)[0]:
        assert not tr[c, rows:].any(), c
    assert (tr[A.RANGE_COUNTER] == np.minimum(idx, 65535)).all()
    shared = tr[26:44].reshape(-1)
    assert int(shared.max()) < 1 << 16
    freq = np.bincount(shared.astype(np.int64), minlength=n)[:n].astype(np.uint64)
    assert (tr[A.RC_FREQ] == freq).all()
    if log_ops != 20:
        return
    trace = np.ascontiguousarray(got)
    del tr, shared, freq, got
    t = CtlTable()
    cs = T.arithmetic_ctl_rows(t)
    zs, ids = make_zs([([cs], 3, 5), ([cs], 7, 11)])
    ctl_aux = ctx.ctl_data(t, zs, ids, trace, 54, log_n)
    betas = [0x1234567, 0x89ABCDEF01]
    lt = CtlTable()
    looking = [lt.colset([lt.single(c)]) for c in range(26, 44)]
    lk = [ctx.lookup_helper_columns(lt, looking, lt.single(A.RANGE_COUNTER), lt.single(A.RC_FREQ), b, trace, 54, log_n) for b in betas]
    aux = np.concatenate(lk + [ctl_aux])
    assert ctx.check_constraints(trace, log_n, aux, t, zs, ids, [5, 7], ncols=54, table_id=T.TABLE_ARITHMETIC,
                                 lookup_challenges=betas) is None
    # one challenge: the first challenge's lookup columns, then the CTL columns of its (beta, gamma)
    zs1, ids1 = make_zs([([cs], 3, 5)])
    aux1 = np.concatenate([lk[0], ctx.ctl_data(t, zs1, ids1, trace, 54, log_n)])
    assert ctx.check_constraints(trace, log_n, aux1, t, zs1, ids1, [5], ncols=54, table_id=T.TABLE_ARITHMETIC,
                                 lookup_challenges=betas[:1]) is None


FLAG = {"addu": A.IS_ADDU, "subu": A.IS_SUBU, "addiu": A.IS_ADDIU, "sll": A.IS_SLL, "srl": A.IS_SRL, "sra": A.IS_SRA,
        "sllv": A.IS_SLLV, "srlv": A.IS_SRLV, "srav": A.IS_SRAV}


def machine_ops(m):
    return np.array([(FLAG[name], a, b) for name, a, b, _, _ in m.arith_ops], dtype=np.uint32)


def test_cpu_segment_with_gpu_arithmetic_table(ctx, oracle):
    """build_cpu_segment's Arithmetic table rebuilt by the GPU from the ops the Machine pushed (device-resident) and proved from HBM:
    the proofs equal those from the fixture's table, and the oracle verifier accepts them."""
    tables, ctls, m = CF.build_cpu_segment(oracle)
    tid, arith, ncols, log_a, ct = tables[3]
    dev = to_device(ctx, machine_ops(m))
    buf, natural = ctx.arithmetic_trace(dev, nops=len(m.arith_ops))
    dev.free()
    try:
        assert natural == 1 << log_a and (buf.download() == arith).all()
        want, wchal, woffs = oracle.prove_with_traces(tables, ctls)
        got, chal, offs = ctx.prove_with_traces(tables[:3] + [(tid, buf, ncols, log_a, ct)], ctls)
        assert offs == woffs and (chal == wchal).all() and (got == want).all()
        assert oracle.verify_all(tables, ctls, got, chal) == 0
    finally:
        buf.free()


def test_full_segment_with_gpu_arithmetic_table(ctx, oracle):
    """build_full_segment's Arithmetic table rebuilt by the GPU (ops re-derived by running sample_program again) and passed as a
    DeviceBuffer to prove_with_traces and to prove_segment: the proofs equal those from the fixture's table."""
    from zkm_amd import tables as T
    tables, ctls = CF.build_full_segment(oracle)
    tid, arith, ncols, log_a, ct = tables[0]
    assert tid == T.TABLE_ARITHMETIC
    dev = to_device(ctx, machine_ops(CF.sample_program(CF.Machine())))
    buf, natural = ctx.arithmetic_trace(dev, log_a)
    dev.free()
    try:
        assert (buf.download() == arith).all()
        want, wchal, woffs = oracle.prove_with_traces(tables, ctls, public_values=[1, 2, 3])
        got, chal, offs = ctx.prove_with_traces([(tid, buf, ncols, log_a, ct)] + tables[1:], ctls, public_values=[1, 2, 3])
        assert offs == woffs and (chal == wchal).all() and (got == want).all()
        assert oracle.verify_all(tables, ctls, got, chal, public_values=[1, 2, 3]) == 0
        traces = [buf] + [t[1] for t in tables[1:]]
        got2, chal2, offs2 = ctx.prove_segment(traces, [t[3] for t in tables], public_values=[1, 2, 3])
        assert offs2 == offs and (chal2 == chal).all() and (got2 == got).all()
    finally:
        buf.free()
