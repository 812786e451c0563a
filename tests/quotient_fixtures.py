"""Invalid traces for tests/test_gpu_quotient_tables.py: rows that satisfy nothing, so that every constraint of a table is nonzero and the
quotient words (or, for the two tables with lookups of their own, the proof words) check every expression and its place in the alpha
order at once.  Everything here is host-side Python: the conditions on the inputs (no vacuous case, no zero denominator, filters that
cross_table_lookup_data admits) can be checked without a GPU."""
import numpy as np

from zkm_amd import tables as T

from .test_gpu_quotient_loose import EDGE       # the edge words are that module's: imported, not copied

P = 0xFFFFFFFF00000001
NAMES = {T.TABLE_POSEIDON: "Poseidon", T.TABLE_LOGIC: "Logic", T.TABLE_KECCAK_SPONGE: "KeccakSponge", T.TABLE_KECCAK: "Keccak", T.TABLE_MEMORY: "Memory",
         T.TABLE_POSEIDON_SPONGE: "PoseidonSponge", T.TABLE_SHA_EXTEND: "ShaExtend", T.TABLE_SHA_EXTEND_SPONGE: "ShaExtendSponge",
         T.TABLE_SHA_COMPRESS: "ShaCompress", T.TABLE_SHA_COMPRESS_SPONGE: "ShaCompressSponge", T.TABLE_ARITHMETIC: "Arithmetic", T.TABLE_CPU: "Cpu"}
LOOKUP_TABLES = (T.TABLE_MEMORY, T.TABLE_ARITHMETIC)
LOOKUP_FREE = [t for t in sorted(T.WIDTH) if t not in LOOKUP_TABLES]
KINDS = ("random", "constant")
# the fake CTL shapes of the suite (helper columns, no column sets): one Z -> one chunk -> k_quotient_ctl; two Zs -> two chunks -> a short
# table takes k_quotient_ctl_chunk + k_quotient_ctl_sum (stark.hip launch_ctl_checks)
CTL_SHAPES = {"ctl_one_thread[2]": [2], "ctl_chunked[1,1]": [1, 1]}
# a table's own logUp lookup (Stark::lookups()): looking columns, table column, frequencies column
LOOKUPS = {T.TABLE_MEMORY: ([10], 11, 12),                      # memory_stark.rs:476-483
           T.TABLE_ARITHMETIC: (list(range(26, 44)), 44, 45)}   # arithmetic_stark.rs:269-276
LOOKUP_CHALLENGES = [0x1234567, 0x89ABCDEF01]
CTL_CHALLENGES = [(3, 5), (7, 11)]
SEED = 20


def rng_for(table_id, kind, log_n, what=0):
    return np.random.default_rng([SEED, table_id, KINDS.index(kind), log_n, what])


def columns(rng, kind, ncols, n):
    """ncols columns of n rows, column-major: uniform in [0, p), or every column one edge word."""
    if kind == "random":
        return rng.integers(0, P, ncols * n, dtype=np.uint64)
    return np.repeat(np.array(EDGE, dtype=np.uint64)[rng.integers(0, len(EDGE), ncols)], n)


def invalid_trace(table_id, kind, log_n):
    return columns(rng_for(table_id, kind, log_n), kind, T.WIDTH[table_id], 1 << log_n)


def fake_aux(table_id, kind, log_n, num_helpers):
    return columns(rng_for(table_id, kind, log_n, 1 + len(num_helpers)), kind, sum(num_helpers) + len(num_helpers), 1 << log_n)


def challenge_pairs(table_id, kind, log_n):
    """The pairs of the Poseidon test and one random pair."""
    r = rng_for(table_id, kind, log_n, 9).integers(0, P, 2, dtype=np.uint64)
    return [(P - 1, 2**32 - 1), (1, 0), (P - 1, P - 1), (int(r[0]), int(r[1]))]


def first_difference(got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return "none" if bad.size == 0 else "word %d: %#x, expected %#x (%d words differ)" % (bad[0], int(got[bad[0]]), int(want[bad[0]]), bad.size)


# ---- Memory and Arithmetic: cross_table_lookup_data refuses a filter that is not 0 or 1 on some row ("Non-binary filter?",
# cross_table_lookup.rs:741), in the reference and on the device alike, so the filter of the real column set is pinned to 1 on every row and
# everything else is as above.  Memory's filter is one column (memory_stark.rs:41-43); Arithmetic's is the sum of the 26 operator flags
# (arithmetic_stark.rs:118-125): the flags stay uniformly random / edge words, only their sum is chosen.
ZERO_SUMS = [[0], [1, P - 1], [2, P - 2], [2**32, P - 2**32], [2**32 - 1, P - 2**32, 1], [2**32 - 2, P - 2**32, 2], [2**63, 2**63 - 1, P - 2**32, 2]]


def edge_words_summing_to_one(rng, count):
    """`count` edge words whose sum is 1 mod p, in random order: the word 1 and groups of edge words that cancel."""
    words = [1]
    while len(words) < count:
        g = ZERO_SUMS[int(rng.integers(0, len(ZERO_SUMS)))]
        if len(words) + len(g) <= count:
            words += g
    assert sum(words) % P == 1 and set(words) <= set(EDGE)
    return np.array(words, dtype=np.uint64)[rng.permutation(count)]


def invalid_lookup_table_trace(table_id, kind, log_n):
    n = 1 << log_n
    rng = rng_for(table_id, kind, log_n)
    t = columns(rng, kind, T.WIDTH[table_id], n).reshape(T.WIDTH[table_id], n)
    if table_id == T.TABLE_MEMORY:
        t[T.MEM_FILTER] = 1
    elif kind == "constant":
        t[:26] = edge_words_summing_to_one(rng, 26)[:, None]
    else:
        others = t[:25].astype(object).sum(axis=0)
        t[25] = np.array([(1 - int(s)) % P for s in others], dtype=np.uint64)
    return t.reshape(-1)


def eval_column(ct, ci, t, row):
    """Column::eval_table (cross_table_lookup.rs:313-333) of column ci of a CtlTable on row `row` of the n-row trace t (W x n), in Python
    integers; next-row terms count as 0 on the last row."""
    n_local, n_next, off, _, const = ct._cols[ci]
    acc = const + sum(int(t[ct._tc[off + k]][row]) * ct._tf[off + k] for k in range(n_local))
    if row + 1 < t.shape[1]:
        acc += sum(int(t[ct._tc[off + n_local + k]][row + 1]) * ct._tf[off + n_local + k] for k in range(n_next))
    return acc % P


def colset_rows(ct, cs, t, beta, gamma):
    """(filter, sum_i column_i beta^i + gamma) of column set cs on every row."""
    ncols, col0, has_filter, nprod, poff, nconst, coff, _ = ct._sets[cs]
    out = []
    for row in range(t.shape[1]):
        f = 1
        if has_filter:
            f = sum(eval_column(ct, ct._fidx[poff + 2 * k], t, row) * eval_column(ct, ct._fidx[poff + 2 * k + 1], t, row) for k in range(nprod))
            f = (f + sum(eval_column(ct, ct._fidx[coff + k], t, row) for k in range(nconst))) % P
        out.append((f, (sum(eval_column(ct, col0 + i, t, row) * pow(beta, i, P) for i in range(ncols)) + gamma) % P))
    return out


def assert_no_zero_denominator(table_id, trace, log_n, ct, cs):
    """No beta + word of the table's logUp lookup and no combination of the CTL column set is 0, and the filter is 1: every inverse the
    two provers take is of a nonzero word, for the words of this trace and for every edge word."""
    t = trace.reshape(T.WIDTH[table_id], 1 << log_n)
    looking, table_col, _ = LOOKUPS[table_id]
    for beta in LOOKUP_CHALLENGES:
        assert all((beta + w) % P for w in EDGE)
        for c in looking + [table_col]:
            assert ((t[c].astype(object) + beta) % P != 0).all(), (beta, c)
    for beta, gamma in CTL_CHALLENGES:
        for f, combined in colset_rows(ct, cs, t, beta, gamma):
            assert f == 1 and combined != 0
