"""A host model of zkm_check_ctls' CONTRACT (include/zkm_hip.h), for the tests that predict a report's content: the lookups evaluated
with numpy from the CtlTable descriptions, the multisets kept in Python dicts in first-occurrence order.  The oracle's check_ctls stays
the judge of every verdict; this model only says WHICH finding the contract picks: the lowest failing lookup, a non-binary filter before a
multiset difference, the smallest (side, row), the unbalanced tuple whose first occurrence comes first (looking sides in order, the
looked side last), locations in that order."""
import numpy as np

P = 0xFFFFFFFF00000001


def _column(ct, ci, m):
    """Column ci of description ct on every row of the (ncols, n) matrix m: eval_table (cross_table_lookup.rs:266-285)."""
    n_local, n_next, off, _, constant = ct._cols[ci]
    n = m.shape[1]
    acc = np.full(n, constant, dtype=object)
    for k in range(n_local + n_next):
        col, coeff = ct._tc[off + k], ct._tf[off + k]
        v = m[col].astype(object)
        if k >= n_local:
            v = np.concatenate([v[1:], [0]])          # the next row's value; nothing on the last row
        acc = acc + v * coeff
    return acc % P


class Model:
    def __init__(self):
        self.cache = {}

    def side(self, tables, t, colset):
        """(filter values, tuples (n, width)) of one side, cached per table array."""
        tid, trace, ncols, log_n, ct = tables[t]
        key = (id(trace), t, colset)
        if key not in self.cache:
            m = np.asarray(trace).reshape(ncols, 1 << log_n)
            width, col_off, has_filter, nprod, prod_off, nconst, const_off, _ = ct._sets[colset]
            if has_filter:
                f = np.zeros(m.shape[1], dtype=object)
                for k in range(nprod):
                    f = f + _column(ct, ct._fidx[prod_off + 2 * k], m) * _column(ct, ct._fidx[prod_off + 2 * k + 1], m)
                for k in range(nconst):
                    f = f + _column(ct, ct._fidx[const_off + k], m)
                f = f % P
            else:
                f = np.ones(m.shape[1], dtype=object)
            rows = np.nonzero(f == 1)[0]
            cols = [_column(ct, col_off + k, m)[rows] for k in range(width)]
            tuples = [tuple(int(c[i]) for c in cols) for i in range(len(rows))]
            self.cache[key] = (f, rows, tuples, trace)    # (the trace is kept alive: its id is the key)
        return self.cache[key][:3]

    def check(self, tables, ctls):
        """None when every lookup holds, else a dict with the fields of the report the contract fixes."""
        for c, (looking, looked) in enumerate(ctls):
            sides = list(looking) + [looked]
            bad = None
            seen = {}                                    # tuple -> ([looking locations], [looked locations]), insertion = first occurrence
            for s, (t, colset) in enumerate(sides):
                f, rows, tuples = self.side(tables, t, colset)
                nb = np.nonzero((f != 0) & (f != 1))[0]
                if nb.size and bad is None:
                    bad = dict(kind=1, ctl=c, side=s, table=t, row=int(nb[0]), filter_value=int(f[nb[0]]))
                for r, tup in zip(rows, tuples):
                    seen.setdefault(tup, ([], []))[1 if s == len(sides) - 1 else 0].append((s, t, int(r)))
            if bad:
                return bad
            for tup, (a, b) in seen.items():
                if len(a) != len(b):
                    return dict(kind=2, ctl=c, tuple=list(tup), looking_count=len(a), looked_count=len(b), looking=a[:8], looked=b[:8])
        return None


def report_fields(rep):
    """The same fields read from a zkm_amd.CtlReport."""
    if rep.kind == 0:
        return None
    if rep.kind == 1:
        return dict(kind=1, ctl=rep.ctl, side=rep.side, table=rep.table, row=rep.row, filter_value=rep.filter_value)
    return dict(kind=2, ctl=rep.ctl, tuple=rep.tuple_words(), looking_count=rep.looking_count, looked_count=rep.looked_count,
                looking=rep.looking_locations(), looked=rep.looked_locations())


def verdict_of_code(code):
    """The oracle's check_ctls code as (kind, lookup): 0 -> (0, None), 200 + c -> (1, c), 300 + c -> (2, c)."""
    if code == 0:
        return 0, None
    assert 200 <= code < 400, code
    return (1, code - 200) if code < 300 else (2, code - 300)


def bump(tables, t, i, value=None):
    """The tables with word i of table t (Table::all() position) set to `value`, or increased by one mod p."""
    tr = tables[t][1].copy()
    tr[i] = np.uint64((int(tr[i]) + 1) % P if value is None else value)
    out = list(tables)
    out[t] = (tables[t][0], tr, tables[t][2], tables[t][3], tables[t][4])
    return out
