"""CPU suite: the semantics of zkm_lookup_check pinned to lookup.rs as the oracle restates it.  tests/lookup_model.py says a lookup holds
iff looking(v) == frequency(v) (mod p) for every value v; the logUp argument says it holds iff the running sum closes,

    Z[n-1] + sum_j h_j[n-1] - freq[n-1] * inv(challenge + table[n-1]) == 0        (lookup.rs:106-121, 183-194: Z starts at 0 and the
                                                                                   transition is emitted on the last row too)

for the challenge.  Every named case of tests/lookup_fixtures.py, both shapes, 2^3 and 2^7 rows, two fixed challenges for which no
denominator vanishes on the fixture: the two verdicts agree, and agree with what the case was built to be."""
import numpy as np
import pytest

from zkm_amd.ctl import CtlTable

from . import lookup_fixtures as LF
from . import lookup_model as LM

P = LM.P
CHALLENGES = [0x1234567, 0x89ABCDEF01]


def inv(x):
    return pow(x % P, P - 2, P)


def logup_closes(oracle, shape, m, challenge):
    W, n = m.shape
    cols, table_col, freq_col = shape.lookup()
    canon = LM.canonical(m)
    assert all((challenge + int(v)) % P for c in cols + [table_col] for v in canon[c]), "a denominator vanishes: choose another challenge"
    t = CtlTable()
    sets = [t.colset([t.single(c)]) for c in cols]
    out = oracle.lookup_helper_columns(t, sets, t.single(table_col), t.single(freq_col), challenge, np.ascontiguousarray(m.reshape(-1)), W,
                                       n.bit_length() - 1).reshape(-1, n)
    assert out.shape[0] == (len(cols) + 1) // 2 + 1                       # the helper columns, then Z
    last = sum(int(h[n - 1]) for h in out)
    return (last - int(canon[freq_col][n - 1]) * inv(challenge + int(canon[table_col][n - 1]))) % P == 0


@pytest.mark.parametrize("log_n", [3, 7])
@pytest.mark.parametrize("name", sorted(LF.CASES))
@pytest.mark.parametrize("shape", sorted(LF.SHAPES))
def test_model_verdict_is_the_logup_arguments(oracle, shape, name, log_n):
    s = LF.SHAPES[shape]
    m, holds = LF.case(s, log_n, name)
    f = LM.finding(m, *s.lookup())
    assert (f == LM.HOLDS) == holds, (f, holds)
    for challenge in CHALLENGES:
        assert logup_closes(oracle, s, m, challenge) == holds, (shape, name, log_n, hex(challenge))
    assert (LM.message(s.name, f) is None) == holds


def test_named_cases_are_what_their_names_say():
    """The findings the cases were built for, at 2^3 rows of the Memory shape (the model alone)."""
    s, n = LF.MEMORY, 8

    def f(name):
        return LM.finding(LF.case(s, 3, name)[0], *s.lookup())
    assert f("looking_to_other")[8] == 2 and f("looking_to_other")[1] < n
    assert f("looking_to_missing")[8] == 2
    assert f("frequency_plus_one")[1] == n - 1 and f("frequency_plus_one")[8] == 1
    assert f("frequency_minus_one_at_zero")[1:5] == (LF.J, 0, P - 1, 1) and f("frequency_minus_one_at_zero")[5:7] == (None, None)
    got = f("shared_value_wrapping_off")
    assert got[1] == LF.I and got[3] == (got[2] + 1) % P and got[4] == 2 and got[7] == LF.I
    assert f("big_value_looking_only")[1] == P - 1 and f("big_value_looking_only")[7] is None and f("big_value_looking_only")[4] == 0
    assert f("big_value_table_only")[1] == LF.BIG and f("big_value_table_only")[2] == 0 and f("big_value_table_only")[5:7] == (None, None)
    assert f("table_only_value")[1:8] == (n + 9, 0, 2, 1, None, None, LF.I)
    assert f("looking_only_value")[1:9] == (n + 5, 1, 0, 0, s.cols[0], 2, None, 1)
    m = LF.frequent_value(LF.ARITHMETIC, 11, True)
    got = LM.finding(m, *LF.ARITHMETIC.lookup())
    assert got[1] == 0 and got[2] >= 18 << 10 and got[3] == got[2] + 1 and got[8] == 1
    assert LM.finding(LF.frequent_value(LF.ARITHMETIC, 11, False), *LF.ARITHMETIC.lookup()) == LM.HOLDS
    assert LM.message("Memory", f("looking_only_value")) == ("Lookup failed in MemoryStark: lookup 0: value 0xd is looked up 1 times (first: column 10, row 2) "
                                                              "and has frequency 0x0 in 0 table rows (first: none); 1 values fail")
