"""CPU suite: the model of the SYSKECCAK precompile calls (tests/keccak_calls_model.py) held against judges it did not write -- the Keccak-f
test vectors, the ORACLE's KeccakSponge table (its digest bytes, and the memory operations, XORs and Keccak-f inputs that
tests/logic_fixtures.py reads off it) and the oracle's CPU constraints on a Machine run with a call spliced in."""
import json
import os

import numpy as np

from zkm_amd import tables as T

from . import cpu_fixtures as CF
from . import cpu_steps_model as M
from . import keccak_calls_model as K
from . import logic_fixtures as LF

GOLD = os.path.join(os.path.dirname(__file__), "golden")
LENGTHS = (4, 32, 36, 132, 136, 140, 272)


def sorted_ops(ops):
    return sorted(tuple(int(v) for v in op) for op in ops)


def test_keccakf_equals_the_test_vectors():
    kat = json.load(open(os.path.join(GOLD, "keccakf_kat.json")))
    assert kat["keccakf"]
    for v in kat["keccakf"]:
        keys = sorted(v)
        state = [int(x, 16) if isinstance(x, str) else int(x) for x in v[[k for k in keys if "in" in k][0]]]
        want = [int(x, 16) if isinstance(x, str) else int(x) for x in v[[k for k in keys if "out" in k][0]]]
        assert K.keccakf(state) == want
    for v in kat["keccak256"]:                                    # and the sponge around it, on the vectors whose length the calls take
        msg = bytes.fromhex(v["msg_hex"])
        if msg and len(msg) % 4 == 0:
            assert K.Expansion().sponge(msg, 0, 0, [0] * (len(msg) // 4), 0).hex() == v["digest_hex"]


def calls_of(lengths, seed=3, first=(1, 2, 3, 0)):
    """One call per length on seeded bytes (the first begins 1, 2, 3, 0), at disjoint addresses and clocks."""
    rng = np.random.default_rng(seed)
    calls = []
    for k, L in enumerate(lengths):
        data = bytearray(rng.integers(0, 256, L, dtype=np.uint8).tobytes())
        if k == 0:
            data[:4] = bytes(first)
        calls.append((bytes(data), (0, 1, (0x10000 + 0x1000 * k) | K.FLAG, 10 * (50 + 60 * k)), 0x80000 + 0x40 * k))
    return calls


def oracle_table(oracle, inputs, off, meta, log_n=4):
    """The oracle's KeccakSponge table of the calls' operations (its addresses are virt_base + w) with the KS_VIRT columns rewritten to
    base + 4 w: what the table of a flagged operation holds."""
    plain = meta.copy()
    plain[:, 2] &= ~np.uint64(K.FLAG)
    trace, used = oracle.keccak_sponge_trace(inputs, off, plain.reshape(-1), log_n)
    cols = trace.reshape(470, 1 << log_n).copy()
    r = 0
    for k in range(len(meta)):
        L = int(off[k + 1] - off[k])
        for b in range(L // 136 + 1):
            for i in range(34):
                w = 34 * b + i
                assert cols[T.KS_VIRT + i, r] == (int(plain[k, 2]) + w if w < (L + 3) // 4 else 0)
                cols[T.KS_VIRT + i, r] = int(plain[k, 2]) + 4 * w if w < (L + 3) // 4 else 0
            r += 1
    assert r == used
    return cols.reshape(-1), used


def test_lists_and_digests_equal_the_oracles_sponge_table(oracle):
    inputs, off, meta, daddrs = K.lists(calls_of(LENGTHS))
    x = K.expand(inputs, off, meta, daddrs)
    rows, mem, logic, perm_in, perm_ts = x.arrays()
    B = [L // 136 + 1 for L in LENGTHS]
    assert rows.shape[0] == sum((L // 4 + 7) // 8 + 2 for L in LENGTHS) and mem.shape[0] == sum(LENGTHS) and logic.shape[0] == 34 * sum(B) and len(perm_ts) == sum(B)
    log_n = 4
    table, used = oracle_table(oracle, inputs, off, meta, log_n)
    assert used == sum(B)
    cols = table.reshape(470, 1 << log_n)
    last = np.cumsum(B) - 1
    for k in range(len(LENGTHS)):
        assert bytes(int(cols[T.KS_DIGEST + b, last[k]]) for b in range(32)) == x.digests[k]
        assert x.digests[k] == oracle.keccak256(inputs[int(off[k]):int(off[k + 1])].tobytes())
    assert (mem == LF.memory_ops_from_sponge(table, log_n, used)).all()
    assert sorted_ops(logic) == sorted_ops(LF.logic_ops_from_sponge(table, log_n, used))          # (the fixtures shuffle)
    want_in, want_ts = LF.keccak_inputs_from_sponge(table, log_n, used)
    assert (perm_in == want_in).all() and (perm_ts == want_ts).all()


def test_rows_masks_and_clocks():
    (data, meta, daddr), = calls_of([36], first=(1, 2, 3, 0))
    x = K.Expansion()
    digest = x.keccak(data, meta, daddr)
    S = meta[3] // 10
    assert x.masks == [0xFF, 0x01, 0, 0xFF] and x.clocks == [S - 2, S - 1, S, S + 1]
    r0, r1, sp, wr = x.rows
    assert [r0[CF.ch(i, 4)] for i in range(8)] == [0x10000 + 4 * i for i in range(8)] and r0[CF.ch(0, 5)] == 0x01020300
    assert r1[CF.ch(0, 4)] == 0x10020 and r1[CF.ch(1, 0)] == 0
    assert sp[K.IS_KECCAK_SPONGE] == 1 and [sp[CF.ch(i, 5)] for i in range(4)] == [0, 1, 0x10000, 36] and sp[CF.ch(0, 0)] == 0
    assert [sp[CF.GEN + i] for i in range(8)] == [int.from_bytes(digest[4 * (7 - i):4 * (7 - i) + 4], "big") for i in range(8)]
    assert [wr[CF.ch(i, 4)] for i in range(8)] == [daddr + 4 * i for i in range(8)] and wr[CF.ch(7, 1)] == 0
    # the sponge row's address: the first word of the final block, 0 where the input ends in front of it
    for L, want in ((132, 0x10000), (136, 0), (140, 0x10000 + 136), (272, 0)):
        (data, meta, daddr), = calls_of([L])
        x = K.Expansion()
        x.keccak(data, meta, daddr)
        assert x.rows[-2][CF.ch(2, 5)] == want and x.rows[-2][CF.ch(3, 5)] == L
    # what a call costs the link host-expanded: (R + 2) rows of 2,072 bytes, L reads of 48, 34 B XORs of 12, B inputs of 208
    assert K.call_bytes(64) == (8288, 3072, 408, 208) and sum(K.call_bytes(64)) == 11976
    assert K.call_bytes(1024) == (34 * 2072, 1024 * 48, 34 * 8 * 12, 8 * 208) and sum(K.call_bytes(1024)) == 124528


def machine_with_call(seed=5, L=140):
    """The sample program with a SYSCALL row and a Keccak call spliced in behind it."""
    rng = np.random.default_rng(seed)
    m = M.Recorder()
    CF.sample_program(m)
    calls = K.CallRecorder(m)
    for reg, v in ((4, 0x20000), (5, L), (6, 0x30000), (37, 0x40000000)):
        m.set_reg(reg, v)
    m.syscall("other")
    calls.keccak(0x20000, rng.integers(0, 256, L, dtype=np.uint8).tobytes(), 0x30000)
    m.nop()
    return m, calls


def test_model_rows_pass_the_oracles_cpu_constraints(oracle):
    m, calls = machine_with_call()
    _, x = calls.finish()
    assert len(x.rows) == 5 + 2
    log_n = len(m.rows).bit_length()
    m.pad((1 << log_n) - len(m.rows))
    trace = m.trace(log_n)
    count, bad = oracle.debug_constraints(T.TABLE_CPU, trace, 259, log_n)
    assert count == 741 and bad is None, bad
    cols = trace.reshape(259, -1)
    assert cols[K.IS_KECCAK_SPONGE].sum() == 1
    assert (cols[CF.CLOCK] == np.arange(1 << log_n)).all()      # every call row sits at its clock
    # the rows are live under the constraints: a read row whose channel 0 is used "twice" is refused at that row
    at = x.clocks[0]
    cols[CF.ch(0, 0), at] = 2
    assert oracle.debug_constraints(T.TABLE_CPU, cols.reshape(-1), 259, log_n)[1][0] == at
