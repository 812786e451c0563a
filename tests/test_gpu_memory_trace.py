"""GPU suite: zkm_memory_trace (csrc/memory_trace.hip), MemoryStark::generate_trace (memory_stark.rs:135-248) from the raw memory
operations, word for word against the CPU oracle's zko_memory_trace -- sorting with equal keys in push order, fill_gaps at its
boundaries, the padding rows wherever the last operation pushed lands, multi-word keys, every failure -- and the GPU table in
segment proofs and in the range-check lookup."""
import ctypes as C

import numpy as np
import pytest

from . import cpu_fixtures as CF
from .test_oracle_tables import random_memory_ops

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001


def gpu_trace(ctx, oracle, ops, log_n=None, device=False):
    """The GPU table (host or device input) equals the oracle's at the same height; returns (trace, natural rows)."""
    ops = np.ascontiguousarray(ops, dtype=np.uint64).reshape(-1, 6)
    src = ctx.alloc(ops.size).upload(ops) if device else ops
    try:
        buf, natural = ctx.memory_trace(src, log_n)
    finally:
        if device:
            src.free()
    got = buf.download()
    buf.free()
    ln = log_n if log_n is not None else natural.bit_length() - 1
    assert got.size == 13 << ln
    want, wnat = oracle.memory_trace(ops, ln)
    assert natural == wnat
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first differing word: column %d row %d (%d differ)" % (bad[0] >> ln, bad[0] & ((1 << ln) - 1), bad.size)
    return got.reshape(13, -1), natural


def _transient(ctx):
    """Live bytes of the context that are not resident tables (twiddles and the like): a failed call must leave them as it found them."""
    return ctx.memory()[0] - ctx.resident_bytes()


def raw_call(ctx, ops, nops, log_n, out):
    """zkm_memory_trace through ctypes: (status, natural_rows_out, message)."""
    natural = C.c_size_t(12345)
    err = C.c_char_p()
    rc = ctx.L.zkm_memory_trace(ctx.h, ops, nops, log_n, out, C.byref(natural), C.byref(err))
    return rc, natural.value, (err.value or b"").decode()


@pytest.mark.parametrize("k", [16, 200, 1000, 1 << 12, (1 << 16) - 3, 1 << 20])
@pytest.mark.parametrize("device", [False, True])
def test_random_ops(ctx, oracle, k, device):
    gpu_trace(ctx, oracle, random_memory_ops(k, k), device=device)


def test_random_ops_2_22(ctx, oracle):
    ops = random_memory_ops(22, 1 << 22)
    tr, natural = gpu_trace(ctx, oracle, ops, device=True)
    assert natural >= 1 << 22 and int(tr[0].sum()) == 1 << 22
    gpu_trace(ctx, oracle, ops, device=False)


def test_equal_keys_keep_push_order(ctx, oracle):
    """Every op of one CPU row carries timestamp clock * NUM_CHANNELS (witness/memory.rs:78-92): equal (context, segment, virt,
    timestamp) keys in push order, different values -- only a stable sort gives the oracle's rows."""
    rng = np.random.default_rng(5)
    rows = []
    for clock in range(3000):
        for _ in range(int(rng.integers(1, 6))):
            rows.append((0, int(rng.integers(0, 2)), 4 * int(rng.integers(0, 12)), clock * 10, int(rng.integers(0, 2)),
                         int(rng.integers(0, 1 << 32))))
    ops = np.array(rows, dtype=np.uint64)
    tr, _ = gpu_trace(ctx, oracle, ops)
    keys = tr[[3, 4, 5, 1]].T
    same = (keys[1:] == keys[:-1]).all(axis=1) & (tr[0][1:] == 1) & (tr[0][:-1] == 1)
    assert same.sum() > 200 and (tr[6][1:][same] != tr[6][:-1][same]).any()   # the case is exercised
    gpu_trace(ctx, oracle, ops, device=True)


@pytest.mark.parametrize("nops", [4, 1000])
def test_gap_boundaries(ctx, oracle, nops):
    """virt and timestamp gaps at, one below and one above max_rc / max_rc + 1 (fill_gaps :175-204), and gaps that need many dummies."""
    M = (1 << int(np.ceil(np.log2(nops)))) - 1
    for d in (M - 1, M, M + 1, M + 2, M + 3, 2 * M + 1, 2 * M + 2, 2 * M + 3, 7 * M + 5):
        pre = [(0, 1, 0, 1, 0, 5), (0, 1, d, 2, 1, 6), (0, 1, d, 2 + d, 0, 7), (0, 1, d, 3 + d, 1, 7)]
        fill = [(1, 2, 4 * (i // 3), 10 + i, 1, 0) for i in range(nops - len(pre))]
        ops = np.array(pre + fill, dtype=np.uint64)
        tr, natural = gpu_trace(ctx, oracle, ops)
        gpu_trace(ctx, oracle, ops, log_n=natural.bit_length(), device=True)


def test_padding_position(ctx, oracle):
    """The padding copies the last op pushed (pad_memory_ops :206-224) and sorts in right behind it: mid-table when the last pair with
    dummies is not the last pair, at the end when it is, behind the last sorted op when nothing needed dummies."""
    mid = [(0, 1, 0, 1, 0, 3), (0, 1, 0, 100, 1, 3), (1, 0, 8, 2, 0, 4), (1, 0, 8, 3, 1, 4), (1, 0, 12, 5, 0, 9)]
    end = [(0, 1, 0, 1, 0, 3), (0, 1, 0, 2, 1, 3), (1, 0, 8, 2, 0, 4), (1, 0, 8, 3, 1, 4), (1, 0, 900, 5, 0, 9)]
    none = [(0, 1, 0, 1, 0, 3), (0, 1, 0, 2, 1, 3), (1, 0, 8, 2, 0, 4), (1, 0, 8, 3, 1, 4), (1, 0, 12, 5, 0, (1 << 40) + 9)]
    for ops, where in ((mid, "mid"), (end, "end"), (none, "none")):
        tr, natural = gpu_trace(ctx, oracle, np.array(ops, dtype=np.uint64), log_n=7)
        key = tr[[3, 4, 5, 1]]
        pads = np.nonzero((tr[0][1:] == 0) & (key[:, 1:] == key[:, :-1]).all(axis=0))[0] + 1   # filter-0 copies of the row above
        assert pads.size and (np.diff(pads) == 1).all()
        last = {"mid": int(np.argmax(tr[3] == 1)) - 2, "end": 126, "none": 127}[where]
        assert pads.max() == last, (where, pads.min(), pads.max())


def test_log_n_above_natural(ctx, oracle):
    ops = random_memory_ops(3, 300)
    _, natural = gpu_trace(ctx, oracle, ops)
    for extra in (1, 3):
        gpu_trace(ctx, oracle, ops, log_n=natural.bit_length() - 1 + extra)


def test_r0_rule_and_value_truncation(ctx, oracle):
    """into_row (:68-76): a write to (context 0, segment 4, virt 0) stores 0; values are u32 (MemoryOp.value)."""
    ops = np.array([(0, 4, 0, 10, 0, 77), (0, 4, 0, 20, 1, 0), (0, 4, 0, 30, 0, (1 << 40) + 5), (0, 4, 4, 5, 0, (1 << 63) + 3),
                    (0, 4, 4, 6, 1, 3), (1, 4, 0, 7, 0, 11), (0, 3, 0, 8, 0, 12)], dtype=np.uint64)
    tr, _ = gpu_trace(ctx, oracle, ops)
    assert (tr[6] < (1 << 32)).all()
    r0 = (tr[0] == 1) & (tr[2] == 0) & (tr[3] == 0) & (tr[4] == 4) & (tr[5] == 0)
    assert r0.sum() == 2 and (tr[6][r0] == 0).all()
    gpu_trace(ctx, oracle, ops, log_n=6, device=True)


@pytest.mark.parametrize("hi", [40, 63])
def test_multi_word_keys(ctx, oracle, hi):
    """Key fields of 40+ bits: (context, segment, virt, timestamp) take 3 or 4 key words."""
    rng = np.random.default_rng(hi)
    k = 5000
    base = [(1 << hi) - 7, (1 << (hi - 1)) + 3, (1 << hi) + 11 if hi < 63 else P - 1000, (1 << (hi - 2)) + 5]
    ops = np.zeros((k, 6), dtype=np.uint64)
    ops[:, 0] = base[0] + rng.integers(0, 2, k)
    ops[:, 1] = base[1] + rng.integers(0, 3, k)
    ops[:, 2] = np.uint64(base[2]) - rng.integers(0, 64, k).astype(np.uint64) * np.uint64(4)
    ops[:, 3] = base[3] + rng.integers(0, 20000, k)
    ops[:, 4] = rng.integers(0, 2, k)
    ops[:, 5] = rng.integers(0, 1 << 63, k)
    assert (ops[:, :4] < P).all()
    gpu_trace(ctx, oracle, ops)
    gpu_trace(ctx, oracle, ops, device=True)


def test_one_and_two_ops(ctx, oracle):
    for ops in ([(3, 2, 40, 7, 0, 9)], [(3, 2, 40, 7, 1, 9), (3, 2, 40, 7, 0, 8)], [(0, 4, 0, 1, 0, 5), (0, 4, 0, 9, 1, 0)],
                [(0, 1, 0, 1, 0, 5), (0, 1, 40, 1, 0, 6)]):
        ops = np.array(ops, dtype=np.uint64)
        _, natural = gpu_trace(ctx, oracle, ops)
        for extra in (1, 2):
            gpu_trace(ctx, oracle, ops, log_n=natural.bit_length() - 1 + extra, device=True)


def test_sizing_mode_matches_oracle(ctx, oracle):
    for seed, k in ((1, 5), (2, 100), (3, 4096), (4, 70000)):
        ops = random_memory_ops(seed, k)
        ops[::7, 3] += np.uint64(5 * k)                 # timestamp gaps that need dummies
        rc, natural, msg = raw_call(ctx, ops.ctypes.data_as(C.c_void_p), k, 99, None)
        assert rc == 0, msg
        _, want = oracle.memory_trace(ops, natural.bit_length())
        assert natural == want
        gpu_trace(ctx, oracle, ops)


def test_failures_leave_the_context_usable(ctx, zkm, oracle):
    ok = random_memory_ops(9, 50)

    def still_works():
        gpu_trace(ctx, oracle, ok)

    small = ctx.alloc(64)
    ptr = C.c_void_p(small.ptr)
    try:
        # no ops (memory_stark.rs: "No memory ops?")
        rc, _, msg = raw_call(ctx, ptr, 0, 4, ptr)
        assert rc != 0 and "No memory ops" in msg
        still_works()
        # 2^32 ops, log_n above the cap: refused before anything is read or written
        rc, _, msg = raw_call(ctx, ptr, 1 << 32, 4, ptr)
        assert rc != 0 and "2^32" in msg
        still_works()
        rc, _, msg = raw_call(ctx, ptr, 2, 29, ptr)
        assert rc != 0 and "cap" in msg
        still_works()
        # more rows than 2^log_n: the message names them and natural_rows_out is written
        ops = np.array([(0, 0, 0, i, 0, i) for i in range(5)], dtype=np.uint64)
        rc, natural, msg = raw_call(ctx, ops.ctypes.data_as(C.c_void_p), 5, 2, ptr)
        assert rc != 0 and natural == 8 and "8 rows" in msg
        with pytest.raises(RuntimeError):
            oracle.memory_trace(ops, 2)
        still_works()
        # a key word >= p
        for f in range(4):
            bad = ok.copy()
            bad[17, f] = P + (f == 3)
            with pytest.raises(zkm.ZkmError, match="below p"):
                ctx.memory_trace(bad, 8)
            with pytest.raises(zkm.ZkmError, match="below p"):
                ctx.memory_trace(bad)
            still_works()
        # a context gap and a segment gap whose range check is >= 2^log_n (the oracle rejects them too)
        for gap in ([(0, 1, 0, 1, 0, 5), (100, 1, 0, 1, 0, 6)], [(2, 0, 0, 1, 0, 5), (2, 4, 0, 1, 0, 6)]):
            g = np.array(gap, dtype=np.uint64)
            before = _transient(ctx)
            with pytest.raises(zkm.ZkmError, match="range check"):
                ctx.memory_trace(g, 1)
            assert _transient(ctx) == before   # (the check fails after the whole table is built: every block went back)
            with pytest.raises(RuntimeError):
                oracle.memory_trace(g, 1)
            still_works()
        # one timestamp gap of 2^40 (M = 1): 2^40 - 1 dummy rows -- sized, then refused for the table; 2^62: refused when sizing
        g = np.array([(0, 1, 0, 0, 0, 5), (0, 1, 0, 1 << 40, 1, 5)], dtype=np.uint64)
        rc, natural, msg = raw_call(ctx, g.ctypes.data_as(C.c_void_p), 2, 0, None)
        assert rc == 0 and natural == 1 << 41
        with pytest.raises(zkm.ZkmError, match="rows"):
            ctx.memory_trace(g, 10)
        still_works()
        g[1, 3] = (1 << 62) + 5
        rc, natural, msg = raw_call(ctx, g.ctypes.data_as(C.c_void_p), 2, 0, None)
        assert rc != 0 and "do not fit" in msg
        with pytest.raises(zkm.ZkmError, match="do not fit"):
            ctx.memory_trace(g, 10)
        still_works()
        # out must be a device pointer
        host_out = np.zeros(13 << 6, dtype=np.uint64)
        rc, _, msg = raw_call(ctx, ok.ctypes.data_as(C.c_void_p), len(ok), 6, host_out.ctypes.data_as(C.c_void_p))
        assert rc != 0 and "device pointer" in msg and not host_out.any()
        still_works()
    finally:
        small.free()


def scrambled_push_order(trace, log_n, seed):
    """The real ops of a Memory table (filter 1, in sorted order), pushed in a different order that keeps equal keys in theirs."""
    tr = trace.reshape(13, 1 << log_n)
    real = tr[0] == 1
    ops = np.stack([tr[3][real], tr[4][real], tr[5][real], tr[1][real], tr[2][real], tr[6][real]], axis=1)
    key = ops[:, :4]
    group = np.concatenate([[0], np.cumsum((key[1:] != key[:-1]).any(axis=1))])
    perm = np.random.default_rng(seed).permutation(group[-1] + 1)
    return np.ascontiguousarray(ops[np.argsort(perm[group], kind="stable")])


def test_cpu_segment_with_gpu_memory_table(ctx, oracle):
    """build_cpu_segment's Memory table rebuilt by the GPU from the ops the Machine pushed (device-resident) and proved from HBM:
    the proofs equal those from the oracle's table, and the oracle verifier accepts them."""
    tables, ctls, m = CF.build_cpu_segment(oracle)
    tid, memory, ncols, log_mem, ct = tables[1]
    ops = np.array([(c, s, v, ts, r, val) for r, c, s, v, val, ts in m.mem_ops], dtype=np.uint64)
    buf, natural = ctx.memory_trace(ops, log_mem)
    try:
        assert (buf.download() == memory).all()
        want, wchal, woffs = oracle.prove_with_traces(tables, ctls)
        gpu_tables = [tables[0], (tid, buf, ncols, log_mem, ct)] + tables[2:]
        got, chal, offs = ctx.prove_with_traces(gpu_tables, ctls)
        assert offs == woffs and (chal == wchal).all() and (got == want).all()
        assert oracle.verify_all(tables, ctls, got, chal) == 0
    finally:
        buf.free()


def test_full_segment_with_gpu_memory_table(ctx, oracle):
    """build_full_segment's Memory table rebuilt by the GPU (its ops re-derived from the table, pushed in another order) and passed
    as a DeviceBuffer to prove_with_traces and to prove_segment: the proofs equal those from the oracle's table."""
    from zkm_amd import tables as T
    tables, ctls = CF.build_full_segment(oracle)
    tid, memory, ncols, log_mem, ct = tables[11]
    assert tid == T.TABLE_MEMORY
    ops = scrambled_push_order(memory, log_mem, 3)
    dev_ops = ctx.alloc(ops.size).upload(ops)
    buf, natural = ctx.memory_trace(dev_ops, log_mem)
    dev_ops.free()
    try:
        assert (buf.download() == memory).all()
        want, wchal, woffs = oracle.prove_with_traces(tables, ctls, public_values=[1, 2, 3])
        got, chal, offs = ctx.prove_with_traces(tables[:11] + [(tid, buf, ncols, log_mem, ct)], ctls, public_values=[1, 2, 3])
        assert offs == woffs and (chal == wchal).all() and (got == want).all()
        assert oracle.verify_all(tables, ctls, got, chal, public_values=[1, 2, 3]) == 0
        traces = [t[1] for t in tables[:11]] + [buf]
        got2, chal2, offs2 = ctx.prove_segment(traces, [t[3] for t in tables], public_values=[1, 2, 3])
        assert offs2 == offs and (chal2 == chal).all() and (got2 == got).all()
    finally:
        buf.free()


def test_2_20_table_range_check_lookup(ctx, zkm, oracle):
    """A 2^20-row GPU Memory table satisfies every MemoryStark constraint with its range-check lookup (RANGE_CHECK in COUNTER with
    FREQUENCIES, memory_stark.rs:476-483) and its CTL columns (check_constraints, prover.rs:793-910)."""
    from zkm_amd import tables as T
    from zkm_amd.ctl import CtlTable, make_zs
    log_n = 20
    n = 1 << log_n
    trace, natural = gpu_trace(ctx, oracle, random_memory_ops(20, n - 5), device=True)
    assert natural == n
    trace = np.ascontiguousarray(trace.reshape(-1))
    t = CtlTable()
    cs = T.memory_ctl_data(t)
    zs, ids = make_zs([([cs], 3, 5), ([cs], 7, 11)])
    ctl_aux = ctx.ctl_data(t, zs, ids, trace, 13, log_n)
    betas = [3, 7]
    lt = CtlTable()
    looking = lt.colset([lt.single(10)])
    lk = [ctx.lookup_helper_columns(lt, [looking], lt.single(11), lt.single(12), b, trace, 13, log_n) for b in betas]
    aux = np.concatenate(lk + [ctl_aux])
    assert ctx.check_constraints(trace, log_n, aux, t, zs, ids, [5, 7], ncols=13, table_id=T.TABLE_MEMORY, lookup_challenges=betas) is None
    # one challenge: the first challenge's lookup columns, then the CTL columns of its (beta, gamma)
    zs1, ids1 = make_zs([([cs], 3, 5)])
    aux1 = np.concatenate([lk[0], ctx.ctl_data(t, zs1, ids1, trace, 13, log_n)])
    assert ctx.check_constraints(trace, log_n, aux1, t, zs1, ids1, [5], ncols=13, table_id=T.TABLE_MEMORY, lookup_challenges=betas[:1]) is None
