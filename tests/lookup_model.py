"""The model of zkm_lookup_check (include/zkm_hip.h), in Python integers and numpy.unique: for a W x n matrix and a lookup (looking columns,
table column, frequencies column), words read as field elements,

    looking(v)   = the cells (c in cols, row r) with m[c][r] == v                          (an integer)
    frequency(v) = the sum of m[freq_col][r] over the rows r with m[table_col][r] == v     (mod p)

the lookup holds iff looking(v) == frequency(v) (mod p) for every v; the finding names the smallest unbalanced value.  Findings are the
tuples Context.lookup_check returns: (lookup, value, looking, frequency, table rows, column, row, table row, failing values), None for
"holds" in word 0 and for a location that does not exist; HOLDS when every lookup holds."""
import numpy as np

P = 0xFFFFFFFF00000001
HOLDS = (None, 0, 0, 0, 0, 0, 0, 0, 0)


def canonical(words):
    words = np.asarray(words, dtype=np.uint64)
    return np.where(words >= np.uint64(P), words - np.uint64(P), words)


def counts(m, cols, table_col, freq_col):
    """{value: [looking, frequency, table rows, first looking cell (column, row) or None, first table row or None]} of every value on
    either side."""
    m = np.asarray(m, dtype=np.uint64)
    n = m.shape[1]
    out = {}
    cells = canonical(m[list(cols)]).reshape(-1)                       # the lookup's column order, then rows
    values, first, count = np.unique(cells, return_index=True, return_counts=True)
    for v, i, k in zip(values.tolist(), first.tolist(), count.tolist()):
        out[v] = [k, 0, 0, (cols[i // n], i % n), None]
    table, freq = canonical(m[table_col]).tolist(), canonical(m[freq_col]).tolist()
    for r in range(n):
        e = out.setdefault(table[r], [0, 0, 0, None, None])
        e[1] = (e[1] + freq[r]) % P
        e[2] += 1
        if e[4] is None:
            e[4] = r
    return out


def finding(m, cols, table_col, freq_col, lookup=0):
    """The nine words for ONE lookup of a table."""
    by_value = counts(m, list(cols), table_col, freq_col)
    bad = sorted(v for v, e in by_value.items() if e[0] % P != e[1])
    if not bad:
        return HOLDS
    looking, frequency, rows, cell, table_row = by_value[bad[0]]
    column, row = cell if cell is not None else (None, None)
    return (lookup, bad[0], looking, frequency, rows, column, row, table_row, len(bad))


def message(name, f):
    """The call's message for a table's finding (None when the lookup holds)."""
    if f[0] is None:
        return None
    cell = "none" if f[5] is None else "column %d, row %d" % (f[5], f[6])
    table_row = "none" if f[7] is None else "row %d" % f[7]
    return "Lookup failed in %sStark: lookup %d: value %#x is looked up %d times (first: %s) and has frequency %#x in %d table rows (first: %s); %d values fail" % (
        name, f[0], f[1], f[2], cell, f[3], f[4], table_row, f[8])
