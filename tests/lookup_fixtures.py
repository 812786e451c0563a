"""Tables for the lookup check (tests/lookup_model.py, zkm_lookup_check): Memory-shaped (13 columns: RANGE_CHECK 10 looked up in COUNTER 11
with FREQUENCIES 12) and Arithmetic-shaped (54 columns: the shared columns 26..43 in RANGE_COUNTER 44 with RC_FREQUENCIES 45) matrices of
any height.  Only the lookup's columns matter to the check: the other columns are random canonical words (a small Arithmetic-shaped table
is fine here although the prover never sees one).  The starting point is balanced: looking cells random in [0, n), the table column
0 .. n - 1, the frequencies their counts.  CASES are the named cases built from it: name -> (builder, holds)."""
import numpy as np

from zkm_amd import tables as T

P = 0xFFFFFFFF00000001
BIG = (1 << 40) + 3            # a value above 2^32: the sort's passes 4 and 5


class Shape:
    def __init__(self, name, table_id, cols, table_col, freq_col):
        self.name, self.table_id, self.width = name, table_id, T.WIDTH[table_id]
        self.cols, self.table_col, self.freq_col = list(cols), table_col, freq_col

    def lookup(self):
        return self.cols, self.table_col, self.freq_col

    def records(self, log_n):
        return (len(self.cols) + 1) << log_n


MEMORY = Shape("Memory", T.TABLE_MEMORY, [10], 11, 12)                    # memory_stark.rs:476-483
ARITHMETIC = Shape("Arithmetic", T.TABLE_ARITHMETIC, range(26, 44), 44, 45)   # arithmetic_stark.rs:269-276
SHAPES = {"Memory": MEMORY, "Arithmetic": ARITHMETIC}


def rebalance(m, shape):
    """The frequencies of a table column of DISTINCT values: each row's count of looking cells that hold its value."""
    table = [int(x) % P for x in m[shape.table_col]]
    assert len(set(table)) == len(table)
    values, count = np.unique(m[shape.cols], return_counts=True)
    by_value = dict(zip(values.tolist(), count.tolist()))
    m[shape.freq_col] = np.array([by_value.get(v, 0) for v in table], dtype=np.uint64)
    return m


def balanced(shape, log_n, seed=1):
    n = 1 << log_n
    rng = np.random.default_rng([seed, shape.table_id, log_n])
    m = rng.integers(0, P, (shape.width, n), dtype=np.uint64)
    m[shape.cols] = rng.integers(0, n, (len(shape.cols), n), dtype=np.uint64)
    m[shape.table_col] = np.arange(n, dtype=np.uint64)
    return rebalance(m, shape)


def move_cells(m, shape, value, to):
    """Every looking cell that holds `value` now holds `to`."""
    cells = m[shape.cols]
    cells[cells == np.uint64(value)] = np.uint64(to)
    m[shape.cols] = cells


def bump(m, c, r, d):
    m[c, r] = np.uint64((int(m[c, r]) + d) % P)


# ---- the named cases: each takes the balanced table (its own copy) and the shape; rows I, J < 8 <= n
I, J = 1, 6


def looking_to_missing(m, s):
    """a looking cell moved to a value the table lacks (the value it left fails too)"""
    m[s.cols[0], 2] = m.shape[1] + 5


def looking_to_other(m, s):
    """a looking cell moved to another table value: two values fail, the lower is reported"""
    m[s.cols[-1], 3] = (int(m[s.cols[-1], 3]) + 1) % m.shape[1]


def frequency_plus_one(m, s):
    bump(m, s.freq_col, m.shape[1] - 1, 1)


def frequency_minus_one_at_zero(m, s):
    """a frequency - 1 on a value with frequency 0: p - 1 on a value nobody looks up"""
    move_cells(m, s, J, I)
    rebalance(m, s)
    assert m[s.freq_col, J] == 0
    bump(m, s.freq_col, J, -1)
    assert m[s.freq_col, J] == P - 1


def share(m, s):
    """rows I and J both hold the value I; whoever looked J up looks I up now, at least one cell does.  Returns the value's count."""
    move_cells(m, s, J, I)
    m[s.cols[0], 0] = I
    rebalance(m, s)
    count = int(m[s.freq_col, I])
    assert count >= 1 and m[s.freq_col, J] == 0
    m[s.table_col, J] = I
    return count


def shared_value_split(m, s):
    count = share(m, s)
    m[s.freq_col, I], m[s.freq_col, J] = count // 2, count - count // 2


def shared_value_wrapping(m, s):
    """frequencies p - 1 and count + 1: field elements, balanced"""
    count = share(m, s)
    m[s.freq_col, I], m[s.freq_col, J] = P - 1, count + 1


def shared_value_wrapping_off(m, s):
    count = share(m, s)
    m[s.freq_col, I], m[s.freq_col, J] = P - 1, count + 2


def big_values(m, s):
    """BIG and p - 1 on both sides, in rows I and J"""
    move_cells(m, s, I, BIG)
    move_cells(m, s, J, P - 1)
    m[s.cols[0], 4], m[s.cols[-1], 5] = BIG, P - 1
    m[s.table_col, I], m[s.table_col, J] = BIG, P - 1
    rebalance(m, s)
    assert m[s.freq_col, I] >= 1 and m[s.freq_col, J] >= 1


def big_value_looking_only(m, s):
    big_values(m, s)
    m[s.table_col, J], m[s.freq_col, J] = J, 0


def big_value_table_only(m, s):
    big_values(m, s)
    move_cells(m, s, BIG, 0)
    count = int(m[s.freq_col, I])
    bump(m, s.freq_col, 0, count)


def noncanonical_word(m, s):
    """the word p + 3 in a looking cell where the table holds 3"""
    m[s.cols[0], 7] = 3
    rebalance(m, s)
    m[s.cols[0], 7] = P + 3


def table_only_value(m, s):
    """a value only the table holds, with a nonzero frequency"""
    move_cells(m, s, I, 0)
    rebalance(m, s)
    m[s.table_col, I], m[s.freq_col, I] = m.shape[1] + 9, 2


def looking_only_value(m, s):
    """a value only the looking side holds (the value it left is balanced again)"""
    c, r = s.cols[0], 2
    bump(m, s.freq_col, int(m[c, r]), -1)
    m[c, r] = m.shape[1] + 5


CASES = {"balanced": (lambda m, s: None, True), "looking_to_missing": (looking_to_missing, False), "looking_to_other": (looking_to_other, False),
         "frequency_plus_one": (frequency_plus_one, False), "frequency_minus_one_at_zero": (frequency_minus_one_at_zero, False),
         "shared_value_split": (shared_value_split, True), "shared_value_wrapping": (shared_value_wrapping, True),
         "shared_value_wrapping_off": (shared_value_wrapping_off, False), "big_values": (big_values, True),
         "big_value_looking_only": (big_value_looking_only, False), "big_value_table_only": (big_value_table_only, False),
         "noncanonical_word": (noncanonical_word, True), "table_only_value": (table_only_value, False),
         "looking_only_value": (looking_only_value, False)}


def case(shape, log_n, name):
    """(W x n matrix, holds) of a named case; every case fits from 2^3 rows."""
    assert log_n >= 3
    m = balanced(shape, log_n)
    build, holds = CASES[name]
    build(m, shape)
    return m, holds


def frequent_value(shape, log_n, off):
    """Half the looking cells hold 0 (at Arithmetic 2^11 rows: 18432 cells, nine radix tiles of one value), balanced; off: one more."""
    m = balanced(shape, log_n)
    cells = m[shape.cols]
    cells[:, ::2] = 0
    m[shape.cols] = cells
    rebalance(m, shape)
    if off:
        bump(m, shape.freq_col, 0, 1)
    return m
