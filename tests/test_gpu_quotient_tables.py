"""The quotient kernels of all twelve tables against the oracle as POLYNOMIALS: on rows that satisfy nothing every constraint is nonzero,
so the words check every expression of constraints_dev.h and its place in the alpha order at once -- also the terms behind a flag, a
selector or an auxiliary column that is zero on every row of every valid fixture of the suite, which no proof of a valid trace can see.

* The ten tables without lookups of their own: ctx.quotient against oracle.quotient on uniformly random columns and on constant columns
  of edge words, with the suite's two fake CTL shapes ([2]: one thread per point runs all CTL checks; [1, 1]: two chunks, the chunked CTL
  kernels of a short table), with two challenges and with one (separate kernels), at 2^5 rows (64 points: a quarter of a workgroup) and,
  random columns only, at 2^8 rows (512 points: two workgroups, the next row of a point lies in the other one).  Keccak also with its
  25-threads-per-point form forced on and off.  (The two kinds complement each other: a constant column's next row equals its local
  row, so only the random kind sees a local / next swap; only the constant kind puts chosen edge words in front of the evaluator.)
* Memory and Arithmetic, whose quotient entry point takes no lookup challenges: single-table proofs of such traces with the real CTL
  column set and the table's range-check lookup, byte for byte against the oracle's -- the blob carries the quotient's cap and openings.
  The prover does not judge its witness; the oracle's verifier and check_constraints do, and both must reject.

The inputs are fixed by quotient_fixtures.SEED.  For that seed the oracle's side was computed on a CPU, for every table, kind and shape
used here: no quotient is zero (want.any()), and each table's quotient with the challenge 1 differs from the one with a second challenge
(more than one live constraint), for Poseidon, Logic, KeccakSponge, Keccak, PoseidonSponge, ShaExtend, ShaExtendSponge, ShaCompress,
ShaCompressSponge and Cpu; for Memory and Arithmetic the oracle's verifier rejects every proof, no beta + word of a lookup and no
combination of a CTL column set is zero, and every filter is 1.  The tests assert all of it again.
"""
import numpy as np
import pytest

from zkm_amd import tables as T
from zkm_amd.ctl import CtlTable, make_zs

from . import quotient_fixtures as Q

pytestmark = pytest.mark.gpu
P = Q.P
SHAPES = [("random", 5), ("constant", 5), ("random", 8)]
_oracle_batches = {}


def oracle_batch(oracle, key, make, ncols, log_n):
    """The oracle's commitment to one input, built once and shared by the cases that read it."""
    if key not in _oracle_batches:
        _oracle_batches[key] = oracle.batch_from_values(make(), ncols, log_n)
    return _oracle_batches[key]


def compare_quotients(c, zkm, oracle, table_id, kind, log_n, shape, what=""):
    """ctx.quotient == oracle.quotient for the four challenge pairs, with two challenges and with one.  Returns the device's words."""
    W, nh = T.WIDTH[table_id], Q.CTL_SHAPES[shape]
    A = sum(nh) + len(nh)
    trace, aux = Q.invalid_trace(table_id, kind, log_n), Q.fake_aux(table_id, kind, log_n, nh)
    otb = oracle_batch(oracle, (table_id, kind, log_n), lambda: trace, W, log_n)
    oab = oracle_batch(oracle, (table_id, kind, log_n, shape), lambda: aux, A, log_n)
    tb, ab = zkm.PolynomialBatch.from_values(c, trace, W, log_n), zkm.PolynomialBatch.from_values(c, aux, A, log_n)
    gots = []
    try:
        for pair in Q.challenge_pairs(table_id, kind, log_n):
            for alphas in (pair, pair[:1]):
                want = oracle.quotient(otb, oab, nh, alphas, table_id=table_id)
                got = c.quotient(tb, ab, nh, alphas, table_id=table_id)
                where = "%s%s, %s columns, 2^%d rows, %s, challenges %s" % (Q.NAMES[table_id], what, kind, log_n, shape, [hex(a) for a in alphas])
                assert want.any(), "vacuous case: " + where
                assert got.shape == want.shape and (got == want).all(), "%s: first differing %s" % (where, Q.first_difference(got, want))
                gots.append(got)
    finally:
        tb.free()
        ab.free()
    return gots


@pytest.mark.parametrize("shape", list(Q.CTL_SHAPES))
@pytest.mark.parametrize("kind,log_n", SHAPES)
@pytest.mark.parametrize("table_id", Q.LOOKUP_FREE, ids=lambda t: Q.NAMES[t])
def test_quotient_of_invalid_rows_matches_oracle(ctx, zkm, oracle, table_id, kind, log_n, shape):
    compare_quotients(ctx, zkm, oracle, table_id, kind, log_n, shape)


@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("table_id", Q.LOOKUP_FREE, ids=lambda t: Q.NAMES[t])
def test_inputs_have_more_than_one_live_constraint(oracle, table_id, kind):
    """A condition on the inputs, not on the device: the oracle's quotient with the challenge 1 (the plain sum of the constraints) differs
    from the one with another challenge, so the comparison above is not one constraint's."""
    log_n, shape = 5, "ctl_one_thread[2]"
    W, nh = T.WIDTH[table_id], Q.CTL_SHAPES[shape]
    otb = oracle_batch(oracle, (table_id, kind, log_n), lambda: Q.invalid_trace(table_id, kind, log_n), W, log_n)
    oab = oracle_batch(oracle, (table_id, kind, log_n, shape), lambda: Q.fake_aux(table_id, kind, log_n, nh), 3, log_n)
    one, other = (oracle.quotient(otb, oab, nh, [a], table_id=table_id) for a in (1, Q.challenge_pairs(table_id, kind, log_n)[3][0]))
    assert one.any() and other.any() and (one != other).any(), (Q.NAMES[table_id], kind)


@pytest.mark.parametrize("kind", Q.KINDS)
def test_keccak_quotient_forms_on_invalid_rows(zkm, oracle, kind):
    """eval_keccak_constraints_part restates the 797 constraints in 25 parts (the default up to 2^15 points); eval_keccak_constraints is
    the one-thread form.  Both forced at 2^5 rows, in contexts of the test's own: equal to the oracle and to each other."""
    words = []
    for max_points in (1 << 15, 0):
        c = zkm.Context(0)
        try:
            c.set_tuning("keccak_parts_max_points", max_points)
            words.append([compare_quotients(c, zkm, oracle, T.TABLE_KECCAK, kind, 5, shape, " (keccak_parts_max_points %d)" % max_points)
                          for shape in Q.CTL_SHAPES])
        finally:
            c.close()
    for shape, parts, one in zip(Q.CTL_SHAPES, *words):
        for a, b in zip(parts, one):
            assert (a == b).all(), "Keccak, %s columns, %s: 25 parts against one thread, first differing %s" % (kind, shape, Q.first_difference(a, b))


def real_ctl(table_id):
    t = CtlTable()
    cs = T.memory_ctl_data(t) if table_id == T.TABLE_MEMORY else T.arithmetic_ctl_rows(t)
    zs, ids = make_zs([([cs], beta, gamma) for beta, gamma in Q.CTL_CHALLENGES])
    return t, cs, zs, ids


@pytest.mark.parametrize("log_n", [5, 8])
@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("table_id", Q.LOOKUP_TABLES, ids=lambda t: Q.NAMES[t])
def test_lookup_table_proof_of_invalid_rows_is_bit_exact(ctx, zkm, oracle, table_id, kind, log_n):
    """Memory (13 columns) and Arithmetic (54): the single-table proof of an invalid trace, with the table's real CTL column set and its
    logUp range check, equals the oracle's word for word -- equal quotient caps and openings, so equal quotient polynomials.  The filter
    of the column set is 1 on every row (quotient_fixtures: cross_table_lookup_data admits no other); prove_single_table_ctl admits
    both heights."""
    W = T.WIDTH[table_id]
    name = "%s, %s columns, 2^%d rows" % (Q.NAMES[table_id], kind, log_n)
    trace = Q.invalid_lookup_table_trace(table_id, kind, log_n)
    t, cs, zs, ids = real_ctl(table_id)
    Q.assert_no_zero_denominator(table_id, trace, log_n, t, cs)
    aux = ctx.ctl_data(t, zs, ids, trace, W, log_n)
    want_aux = oracle.ctl_data(t, zs, ids, trace, W, log_n)
    assert (aux == want_aux).all(), "%s: CTL columns, first differing %s" % (name, Q.first_difference(aux, want_aux))
    lk = Q.LOOKUP_CHALLENGES
    want = oracle.prove_ctl(trace, log_n, aux, t, zs, ids, ncols=W, table_id=table_id, lookup_challenges=lk)
    got = ctx.prove_single_table_ctl(trace, log_n, aux, t, zs, ids, ncols=W, table_id=table_id, lookup_challenges=lk)
    assert got.shape == want.shape and (got == want).all(), "%s, lookup challenges %s, CTL challenges %s: first differing %s" % (
        name, [hex(x) for x in lk], Q.CTL_CHALLENGES, Q.first_difference(got, want))
    # the case really is invalid: the oracle's verifier rejects the proof, and the device's check_constraints names one of the first rows
    naux = int(got[3])
    assert oracle.verify_ctl(got, len(zs), t, zs, ids, ncols=W, table_id=table_id, lookup_challenges=lk) != 0, name
    looking, table_col, freq_col = Q.LOOKUPS[table_id]
    lt = CtlTable()
    sets = [lt.colset([lt.single(c)]) for c in looking]
    tc, fc = lt.single(table_col), lt.single(freq_col)
    all_aux = np.concatenate([ctx.lookup_helper_columns(lt, sets, tc, fc, b, trace, W, log_n) for b in lk] + [aux])
    assert all_aux.size == naux << log_n
    row = ctx.check_constraints(trace, log_n, all_aux, t, zs, ids, [5, 7], ncols=W, table_id=table_id, lookup_challenges=lk)
    assert row in (0, 1), "%s: check_constraints returned %s" % (name, row)
