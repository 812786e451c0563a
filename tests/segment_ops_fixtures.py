"""cpu_fixtures.build_full_segment's segment with every raw list kept: the CPU rows (row-major, zero-padded to a power of two) and the
operations of the other eleven tables, as zkm_segment_ops takes them, plus the twelve tables the oracle's generators write at the
reference's heights (Traces::into_tables, witness/traces.rs:230-320: min_rows = max(2^cap_height, MIN_TRACE_LEN = 64))."""
import numpy as np

from zkm_amd import tables as T

from . import arith_fixtures as A
from . import cpu_fixtures as CF
from . import logic_fixtures as LF
from .sponge_fixtures import ops_for_rows

P = CF.P
ORDER = [T.TABLE_ARITHMETIC, T.TABLE_CPU, T.TABLE_POSEIDON, T.TABLE_POSEIDON_SPONGE, T.TABLE_KECCAK, T.TABLE_KECCAK_SPONGE, T.TABLE_SHA_EXTEND,
         T.TABLE_SHA_EXTEND_SPONGE, T.TABLE_SHA_COMPRESS, T.TABLE_SHA_COMPRESS_SPONGE, T.TABLE_LOGIC, T.TABLE_MEMORY]   # Table::all()


def canonical(words):
    """uint64 words reduced mod p (every word is below 2p)."""
    return np.where(words >= np.uint64(P), words - np.uint64(P), words)


def log2_height(rows, min_rows):
    """log2 of max(rows, min_rows).next_power_of_two()."""
    return int(max(rows, min_rows) - 1).bit_length()


def reference_log_ns(raw, cap_height=4):
    """The heights of into_tables restated (an independent check of the library's): Arithmetic and Memory come from their tables."""
    min_rows = max(1 << cap_height, 64)
    ps_rows = int(np.sum(np.diff(raw["poseidon_sponge"][1].astype(np.int64)) // 32 + 1)) if raw["poseidon_sponge"][1].size > 1 else 0
    ks_rows = int(np.sum(np.diff(raw["keccak_sponge"][1].astype(np.int64)) // 136 + 1)) if raw["keccak_sponge"][1].size > 1 else 0
    return [raw["log_arithmetic"], int(len(raw["cpu_rows"])).bit_length() - 1,
            log2_height(len(raw["poseidon"][0]), min_rows), log2_height(ps_rows, min_rows),
            log2_height(24 * len(raw["keccak"][0]), min_rows), log2_height(ks_rows, min_rows),
            log2_height(len(raw["sha_extend"][0]), min_rows), log2_height(48 * len(raw["sha_extend_sponge"][0]), min_rows),
            log2_height(65 * len(raw["sha_compress"][0]), min_rows), log2_height(len(raw["sha_compress_sponge"][0]), min_rows),
            log2_height(len(raw["logic"]), min_rows), raw["log_memory"]]


def build_segment_ops(oracle, repeat=1):
    """(raw, tables, ctls): raw = the segment's raw lists (dict), tables = the twelve (table_id, trace, ncols, log_n, CtlTable) at the
    reference heights in Table::all() order, ctls = the fifteen lookups.  repeat: the sample program runs this many times (a taller CPU
    table, more Logic, Arithmetic and Memory operations)."""
    m = CF.Machine()
    for _ in range(repeat):
        CF.sample_program(m)
    clock = [len(m.rows) + 2]

    def schedule(stride, rec=None):
        def ts(count):
            out = np.array([10 * (clock[0] + stride * k) for k in range(count)], dtype=np.uint64)
            clock[0] += stride * count + 2
            if rec is not None:
                rec.append(out)
            return out
        return ts
    krec = []
    kt, _, (kops, kin, kts, kmem) = LF.build4(oracle, log_sponge=3, ts=schedule(2, krec))
    pt, _, (pdata, poff, pmeta, pin, pts, pmem) = LF.build_poseidon_path(oracle, log_sponge=4, ts=schedule(2))
    ct, _, (chx, cw, cmeta, cops, cmem) = LF.build_sha_compress_path(oracle, ncomp=1, ts=schedule(2))
    et, _, (ew16, emeta, ein, ets, eops, emem) = LF.build_sha_extend_path(oracle, nblocks=1, ts=schedule(96))
    # the KeccakSponge operations build4 made (seed 23, 7 rows), with the timestamps it drew and its address / context rules
    kdata, koff, kmeta, _, knops = ops_for_rows(23, (1 << 3) - 1)
    kmeta = kmeta.reshape(-1, 4).copy()
    kmeta[:, 2] = np.arange(knops) * 512
    kmeta[:, 3] = krec[0]
    kmeta[:, 0], kmeta[:, 1] = 0, 1

    flag_rows = {}

    def add(ts, flag, chans, values):
        c, rem = divmod(int(ts), 10)
        assert rem == 0 and c not in flag_rows
        flag_rows[c] = (flag, [int(v) for v in chans], [int(v) for v in values])
    tr = kt[0][1].reshape(470, -1)
    for r in np.nonzero(tr[T.KS_FINAL_LEN:T.KS_FINAL_LEN + 136].sum(axis=0))[0]:
        words = [sum(int(tr[T.KS_DIGEST + 4 * i + j, r]) << (24 - 8 * j) for j in range(4)) for i in reversed(range(8))]
        add(tr[T.KS_TIMESTAMP, r], T.CPU_IS_KECCAK_SPONGE, [tr[T.KS_CONTEXT, r], tr[T.KS_SEGMENT, r], tr[T.KS_VIRT, r], tr[T.KS_LEN, r]], words)
    tr = pt[0][1].reshape(110, -1)
    for r in np.nonzero(tr[T.PS_FINAL_LEN:T.PS_FINAL_LEN + 32].sum(axis=0))[0]:
        add(tr[T.PS_TIMESTAMP, r], T.CPU_IS_POSEIDON_SPONGE, [tr[T.PS_CONTEXT, r], tr[T.PS_SEGMENT, r], tr[T.PS_VIRT, r], tr[T.PS_LEN, r]],
            tr[T.PS_DIGEST:T.PS_DIGEST + 4, r])
    tr = ct[0][1].reshape(127, -1)
    for r in np.nonzero(tr[T.SCS_IS_REAL])[0]:
        words = [sum(int(tr[T.SCS_OUT_HX + 6 * i + j, r]) << (8 * j) for j in range(4)) for i in range(8)]
        add(tr[T.SCS_TIMESTAMP, r], T.CPU_IS_SHA_COMPRESS_SPONGE, [tr[T.SCS_CONTEXT, r], tr[T.SCS_SEGMENT, r], tr[T.SCS_HX_VIRT, r]], words)
    tr = et[0][1].reshape(76, -1)
    for r in np.nonzero(tr[T.SES_ROUND:T.SES_ROUND + 48].sum(axis=0))[0]:
        w_i = sum(int(tr[T.SES_W_I + j, r]) << (8 * j) for j in range(4))
        add(tr[T.SES_TIMESTAMP, r], T.CPU_IS_SHA_EXTEND_SPONGE, [tr[T.SES_CONTEXT, r], tr[T.SES_SEGMENT, r], tr[T.SES_OUT_VIRT, r]], [w_i])
    while m.clock <= max(flag_rows):
        r = [0] * CF.W
        r[CF.CLOCK] = m.clock
        if m.clock in flag_rows:
            flag, chans, values = flag_rows[m.clock]
            r[flag] = 1
            for i, v in enumerate(chans):
                r[CF.ch(i, 5)] = v
            for i, v in enumerate(values):
                r[CF.GEN + i] = v
        m.rows.append(r)
    log_cpu = int(np.ceil(np.log2(len(m.rows) + 1)))
    cpu_rows = np.zeros((1 << log_cpu, CF.W), dtype=np.uint64)
    cpu_rows[:len(m.rows)] = np.array([[v % P for v in r] for r in m.rows], dtype=np.uint64)

    code = {"and": T.OP_AND, "or": T.OP_OR, "xor": T.OP_XOR, "nor": T.OP_NOR}
    lops = np.concatenate([np.array([(code[name], a, b) for name, a, b, _ in m.logic_ops], dtype=np.uint32).reshape(-1, 3), kops, eops, cops])
    np.random.default_rng(78).shuffle(lops, axis=0)
    flag = {"addu": A.IS_ADDU, "subu": A.IS_SUBU, "addiu": A.IS_ADDIU, "sll": A.IS_SLL, "srl": A.IS_SRL, "sra": A.IS_SRA,
            "sllv": A.IS_SLLV, "srlv": A.IS_SRLV, "srav": A.IS_SRAV}
    aops = np.array([(flag[name], a, b) for name, a, b, _, _ in m.arith_ops], dtype=np.uint32).reshape(-1, 3)
    arows = sum(2 if op in (A.IS_DIV, A.IS_DIVU, A.IS_SRL, A.IS_SRLV, A.IS_SRA, A.IS_SRAV) else 1 for op, _, _ in aops)
    log_arith = max(16, int(arows - 1).bit_length())
    cpu_mem = np.array([(ctx, seg, virt, ts, is_read, value) for is_read, ctx, seg, virt, value, ts in m.mem_ops], dtype=np.uint64)
    mem_ops = np.concatenate([cpu_mem, kmem, pmem, emem, cmem])
    log_mem = int(np.ceil(np.log2(len(mem_ops))))
    while True:                                   # the natural height: the smallest table the operations and their gap rows fit
        try:
            memory, natural = oracle.memory_trace(mem_ops, log_mem)
            break
        except RuntimeError:
            log_mem += 1
    assert natural == 1 << log_mem

    raw = {"cpu_rows": cpu_rows, "arithmetic": aops, "logic": lops, "memory": mem_ops,
           "poseidon": (np.ascontiguousarray(pin, dtype=np.uint64).reshape(-1, 12), np.ascontiguousarray(pts, dtype=np.uint64)),
           "poseidon_sponge": (pdata, poff, np.asarray(pmeta, dtype=np.uint64).reshape(-1, 4)),
           "keccak": (np.ascontiguousarray(kin, dtype=np.uint64).reshape(-1, 25), np.ascontiguousarray(kts, dtype=np.uint64)),
           "keccak_sponge": (kdata, koff, kmeta),
           "sha_extend": (np.ascontiguousarray(ein, dtype=np.uint8).reshape(-1, 16), np.ascontiguousarray(ets, dtype=np.uint64)),
           "sha_extend_sponge": (ew16, emeta),
           "sha_compress": (chx, cw, cmeta), "sha_compress_sponge": (chx, cw, cmeta),
           "log_arithmetic": log_arith, "log_memory": log_mem}
    lg = reference_log_ns(raw)
    tables_by_pos = [
        A.generate_trace([tuple(int(x) for x in op) for op in aops], lg[0]),
        cpu_rows.T.copy().reshape(-1),
        oracle.poseidon_trace_inputs(raw["poseidon"][0], raw["poseidon"][1], lg[2]),
        oracle.poseidon_sponge_trace(pdata, poff, pmeta, lg[3])[0],
        oracle.keccak_trace(raw["keccak"][0], raw["keccak"][1], lg[4]),
        oracle.keccak_sponge_trace(kdata, koff, kmeta.reshape(-1), lg[5])[0],
        oracle.sha_extend_trace(raw["sha_extend"][0], raw["sha_extend"][1], lg[6]),
        oracle.sha_extend_sponge_trace(ew16, emeta, lg[7])[0],
        oracle.sha_compress_trace(chx, cw, cmeta, lg[8]),
        oracle.sha_compress_sponge_trace(chx, cw, cmeta, lg[9]),
        oracle.logic_trace(lops, lg[10]),
        memory,
    ]
    c, ctls = T.all_cross_table_lookups()
    tables = [(ORDER[i], tables_by_pos[i], T.WIDTH[ORDER[i]], lg[i], c[i]) for i in range(12)]
    return raw, tables, ctls


def segment_ops(zkm, raw):
    """The raw lists as a zkm_amd.SegmentOps."""
    return zkm.SegmentOps(raw["cpu_rows"], raw["memory"], arithmetic_ops=raw["arithmetic"], logic_ops=raw["logic"], poseidon=raw["poseidon"],
                          poseidon_sponge=raw["poseidon_sponge"], keccak=raw["keccak"], keccak_sponge=raw["keccak_sponge"],
                          sha_extend=raw["sha_extend"], sha_extend_sponge=raw["sha_extend_sponge"], sha_compress=raw["sha_compress"],
                          sha_compress_sponge=raw["sha_compress_sponge"])


def random_segment_ops(log_ns, seed=5):
    """Random valid operations that give the heights log_ns (Table::all() order; Arithmetic >= 16, Memory >= 7, the rest >= 6): every
    table but the CPU's filled to between half and all of its rows.  CPU rows are random 64-bit words (some above p).  Returns the raw
    lists in the form build_segment_ops gives them."""
    rng = np.random.default_rng(seed)
    n = [1 << x for x in log_ns]
    half = lambda t, per=1: max(1, (n[t] // 2) // per + 1)
    from .test_gpu_arithmetic_trace import valid_ops
    aops = valid_ops(seed, half(0))
    while sum(2 if op in (A.IS_DIV, A.IS_DIVU, A.IS_SRL, A.IS_SRLV, A.IS_SRA, A.IS_SRAV) else 1 for op, _, _ in aops) > n[0]:
        aops = aops[: len(aops) * 7 // 8]
    cpu = rng.integers(0, 1 << 64, (n[1], CF.W), dtype=np.uint64)
    pin = rng.integers(0, P, (half(2), 12), dtype=np.uint64)
    pts = np.arange(len(pin), dtype=np.uint64) * 3
    pdata, poff, pmeta, _, _ = LF.poseidon_sponge_ops(seed + 1, n[3] - 1)
    kin = rng.integers(0, 1 << 64, (half(4, 24), 25), dtype=np.uint64)
    while 24 * len(kin) > n[4]:
        kin = kin[:-1]
    kts = np.arange(len(kin), dtype=np.uint64) * 5
    kdata, koff, kmeta, _, _ = ops_for_rows(seed + 2, n[5])
    ein = rng.integers(0, 256, (half(6), 16), dtype=np.uint8)
    ets = np.arange(len(ein), dtype=np.uint64) * 7
    ew16 = rng.integers(0, 1 << 32, (max(1, n[7] // 48), 16), dtype=np.uint64).astype(np.uint32)
    emeta = np.zeros((len(ew16), 4), dtype=np.uint64)
    emeta[:, 1], emeta[:, 2], emeta[:, 3] = 1, (1 << 22) + np.arange(len(ew16)) * 1024, np.arange(len(ew16)) * 2000 + 7
    nc = max(1, n[8] // 65)
    chx = rng.integers(0, 1 << 32, (nc, 8), dtype=np.uint64).astype(np.uint32)
    cw = rng.integers(0, 1 << 32, (nc, 64), dtype=np.uint64).astype(np.uint32)
    cmeta = np.zeros((nc, 8), dtype=np.uint64)
    cmeta[:, 2], cmeta[:, 3], cmeta[:, 4] = (1 << 23) + np.arange(nc) * 2048, 30 + np.arange(nc) * 10, (1 << 23) + np.arange(nc) * 2048 + 512
    ns = min(half(9), nc) if n[9] > 64 else min(nc, 64)
    lops = np.stack([rng.integers(0, 4, half(10)), rng.integers(0, 1 << 32, half(10)), rng.integers(0, 1 << 32, half(10))], axis=1).astype(np.uint32)
    nm = (n[11] // 2) + 1
    mem = np.zeros((nm, 6), dtype=np.uint64)          # no gap rows: virt and timestamp steps stay below next_pow2(nops)
    mem[:, 1] = rng.integers(0, 3, nm)
    mem[:, 2] = rng.integers(0, 4096, nm)
    mem[:, 3] = rng.permutation(nm).astype(np.uint64)
    mem[:, 4] = rng.integers(0, 2, nm)
    mem[:, 5] = rng.integers(0, 1 << 32, nm)
    return {"cpu_rows": cpu, "arithmetic": aops, "logic": lops, "memory": mem, "poseidon": (pin, pts),
            "poseidon_sponge": (pdata, poff, np.asarray(pmeta, dtype=np.uint64).reshape(-1, 4)), "keccak": (kin, kts),
            "keccak_sponge": (kdata, koff, kmeta.reshape(-1, 4)), "sha_extend": (ein, ets), "sha_extend_sponge": (ew16, emeta),
            "sha_compress": (chx, cw, cmeta), "sha_compress_sponge": (chx[:ns], cw[:ns], cmeta[:ns])}
