"""GPU parity: the proof-of-work search (k_pow_search, fri_proof_of_work) beyond its first launch, word for word against the CPU oracle.

A launch tries 2^pow_round_log candidates a round and 64 rounds, so with the default 17 every witness the suite meets lies in the first
launch.  Here "pow_round_log" is 8 -- a launch spans 2^14 candidates, launch index w >> 14, round (w >> 8) & 63 -- so that witnesses of
16-bit searches need the second and later launches: the advancing base, the `done` flags of a lock-step stack, the host loop that keeps
the first result of each proof, and the result slot the launch leaves ready for the next one.  The oracle searches 0, 1, 2, ... and stops at
the first hit, so a blob equal to the oracle's carries the SMALLEST witness.

The transcripts are PoseidonStark proofs of 2^5 or 2^6 rows (witness seed 5, 2^log_n - 3 permutations) behind the transcript prefix
[k, 17].  The k below were chosen with the oracle on the CPU; each test asserts from the oracle's witnesses that the launches and rounds
it is about do occur, so that a change of fixtures cannot hollow it out.

Not covered: the refusal "Proof of work failed" beyond base 2^40 -- reaching it takes 2^40 permutations.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROUND_LOG = 8                      # the smallest "pow_round_log"
LAUNCH_LOG = ROUND_LOG + 6         # 64 rounds a launch
POW_BITS = 16
# transcript prefix k -> the oracle's witness at 2^5 rows, pow_bits 16 (launch index w >> 14, round (w >> 8) & 63):
#   184 -> 112 (0, 0)       4 -> 9659 (0, 37)      31 -> 4404 (0, 17)     0 -> 20769 (1, 17)     9 -> 33010 (2, 0)     8 -> 36969 (2, 16)
#   3 -> 65062 (3, 62)      14 -> 65978 (4, 1)     29 -> 210966 (12, 56)
SINGLE = [184, 4, 0, 9, 3, 29]
STACKS = {2: [184, 29],3: [3, 0, 184], 5: [0, 9, 4, 3, 8], 8: [3, 0, 9, 29, 4, 184, 14, 31]}

_TRACES, _ORACLE, _ALONE = {}, {}, {}


def launch(w):
    return w >> LAUNCH_LOG


def trace_of(oracle, log_n):
    if log_n not in _TRACES:
        _TRACES[log_n] = oracle.poseidon_trace(5, (1 << log_n) - 3, log_n)
    return _TRACES[log_n]


def configured(cfg, over):
    cfg.pow_bits = POW_BITS
    for k, v in over:
        setattr(cfg, k, v)
    return cfg


def oracle_proof(oracle, k, log_n=5, over=()):
    """the oracle's proof behind prefix [k, 17], made once a module run"""
    key = (k, log_n, over)
    if key not in _ORACLE:
        ch = oracle.challenger()
        oracle.observe(ch, [k, 17])
        aux = np.zeros(4 << log_n, dtype=np.uint64)
        _ORACLE[key] = (oracle.prove(trace_of(oracle, log_n), log_n, aux, [1, 1], challenger=ch, cfg=configured(oracle.standard_config(), over)), ch)
    return _ORACLE[key]


def witness(zkm, blob):
    lay, _ = zkm.proof_layout(blob)
    return int(blob[lay.pow_witness])


def oracle_witness(oracle, zkm, k, log_n=5, over=()):
    return witness(zkm, oracle_proof(oracle, k, log_n, over)[0])


def prove(c, zkm, oracle, k, log_n=5, over=()):
    """(blob, challenger after) of one proof on context c"""
    ch = zkm.challenger_new()
    zkm.challenger_observe(ch, [k, 17])
    aux = np.zeros(4 << log_n, dtype=np.uint64)
    return c.prove_single_table(trace_of(oracle, log_n), log_n, aux, [1, 1], challenger=ch, cfg=configured(c.standard_config(), over)), ch


def same_state(ch, och):
    return list(ch.state) == list(och.state) and ch.n_in == och.n_in and ch.n_out == och.n_out


def equals_oracle(got, oracle, k, log_n=5, over=()):
    blob, ch = got
    want, och = oracle_proof(oracle, k, log_n, over)
    bad = np.nonzero(blob != want)[0] if blob.size == want.size else np.array([-1])
    assert bad.size == 0, "prefix %d: first differing proof word %d of %d" % (k, bad[0], want.size)
    assert same_state(ch, och), k


def tuned(zkm, round_log):
    c = zkm.Context(0)
    if round_log is not None:
        c.set_tuning("pow_round_log", round_log)
    return c


def searches(c, zkm, oracle, k):
    """(number of search launches, blob) of one proof on context c"""
    c.profile(True)
    try:
        c.profile_reset()
        got = prove(c, zkm, oracle, k)
        n = c.profile_records()["fri_pow_search"][0]
    finally:
        c.profile(False)
    equals_oracle(got, oracle, k)
    return n, got[0]


def test_one_proof_finds_the_smallest_witness_in_a_later_launch(zkm, oracle):
    ws = [oracle_witness(oracle, zkm, k) for k in SINGLE]
    assert any(launch(w) == 0 for w in ws) and any(launch(w) == 1 for w in ws) and any(launch(w) >= 3 for w in ws)
    rounds = [(w >> ROUND_LOG) & 63 for w in ws]
    assert 0 in rounds and any(r >= 32 for r in rounds)
    assert any(launch(w) == 0 and (w >> ROUND_LOG) & 63 >= 32 for w in ws)       # a late round of the first launch, too
    c = tuned(zkm, ROUND_LOG)
    try:
        for k in SINGLE:
            equals_oracle(prove(c, zkm, oracle, k), oracle, k)
    finally:
        c.close()


def test_the_launch_count_is_what_the_tuning_says(zkm, oracle):
    """The records of the scope "fri_pow_search" count the launches exactly (one record a launch).  A library that ignored "pow_round_log"
    would search with rounds of 2^17: the witness 65062 lies in its first launch, the count would be 1 where 4 is asserted."""
    k = 3
    w = oracle_witness(oracle, zkm, k)
    assert launch(w) >= 2
    blobs = []
    for value, want in ((8, launch(w) + 1), (3, launch(w) + 1), (0, launch(w) + 1), (None, 1), (22, 1), (40, 1)):    # (the clamp to 8 .. 22)
        c = tuned(zkm, value)
        try:
            n, blob = searches(c, zkm, oracle, k)
        finally:
            c.close()
        assert n == want, (value, n, want)
        blobs.append(blob)
    assert all((b == blobs[0]).all() for b in blobs)


@pytest.mark.parametrize("K", list(STACKS))
def test_stacks_keep_each_proofs_own_witness(ctx, zkm, oracle, K):
    """K searches in lock-step: a proof whose witness is known sits out the later launches (`done`), the others go on, and each blob gets
    its own first result.  pow_round_log 8: launches of 2^14 whatever K; the default and 13: one launch, rounds of 2^16, 2^15, 2^14, 2^14
    and of 2^12 (the floor) for K = 2, 3, 5, 8."""
    ks = STACKS[K]
    assert len(ks) == K
    ls = [launch(oracle_witness(oracle, zkm, k)) for k in ks]
    assert len(set(ls)) >= 2
    assert min(ls) == 0 and max(ls) >= 2                       # one proof is done after the first launch, another needs two more at least
    if K == 2:
        assert ls.index(min(ls)) == 0 and ls.count(min(ls)) == 1      # the first to finish is the first of the stack ...
    if K == 3:
        assert ls.index(min(ls)) == K - 1 and ls.count(min(ls)) == 1  # ... and the last of it
    for k in ks:
        if k not in _ALONE:
            _ALONE[k] = prove(ctx, zkm, oracle, k)[0]
    aux = np.zeros(4 << 5, dtype=np.uint64)
    for round_log in (ROUND_LOG, None, 13):
        c = tuned(zkm, round_log)
        try:
            chs = [zkm.challenger_new() for _ in ks]
            for ch, k in zip(chs, ks):
                zkm.challenger_observe(ch, [k, 17])
            got = c.prove_single_tables([trace_of(oracle, 5)] * K, 5, aux, [1, 1], cfg=configured(c.standard_config(), ()), challengers=chs)
        finally:
            c.close()
        for blob, ch, k in zip(got, chs, ks):
            assert (blob == _ALONE[k]).all(), (round_log, k, witness(zkm, blob), witness(zkm, _ALONE[k]))
            equals_oracle((blob, ch), oracle, k)


@pytest.mark.parametrize("final_poly_bits,log_n,k,position", [(0, 6, 0, 2), (1, 5, 0, 4), (2, 6, 1, 0)])
def test_the_candidate_goes_to_the_word_after_the_final_polynomial(zkm, oracle, final_poly_bits, log_n, k, position):
    """The candidate is written to word n_in of the transcript's input buffer: 2 final_poly_len mod 8 words after the final polynomial
    has been observed.  Arity 4 and cap height 1 fold down to 1, 2 and 4 coefficients: words 2, 4 and 0.
    The oracle's witnesses: 44811, 30904, 101879 (launch 2, 1, 6)."""
    over = (("arity_bits", 2), ("final_poly_bits", final_poly_bits), ("cap_height", 1))
    want, _ = oracle_proof(oracle, k, log_n, over)
    lay, _ = zkm.proof_layout(want)
    assert int(lay.final_poly_len) == 1 << final_poly_bits and 2 * int(lay.final_poly_len) % 8 == position
    assert launch(int(want[lay.pow_witness])) >= 1
    c = tuned(zkm, ROUND_LOG)
    try:
        equals_oracle(prove(c, zkm, oracle, k, log_n, over), oracle, k, log_n, over)
    finally:
        c.close()


def test_a_context_keeps_working_between_searches_of_many_launches(zkm, oracle):
    """After every launch the result words are all ones again and the ticket is 0: a search of many launches, then what else uses the
    pinned result slot (a search of one launch, a short commitment whose tree tail delivers its cap), then searches of many launches."""
    assert launch(oracle_witness(oracle, zkm, 3)) >= 3 and launch(oracle_witness(oracle, zkm, 9)) == 2
    rng = np.random.default_rng(81)
    vals = rng.integers(0, 0xFFFFFFFF00000001, 9 << 6, dtype=np.uint64)
    c = tuned(zkm, ROUND_LOG)
    try:
        equals_oracle(prove(c, zkm, oracle, 3), oracle, 3)
        c.set_tuning("pow_round_log", 17)
        equals_oracle(prove(c, zkm, oracle, 0), oracle, 0)
        b = zkm.PolynomialBatch.from_values(c, vals, 9, 6)
        assert (b.cap() == oracle.batch_from_values(vals, 9, 6).cap()).all()
        b.free()
        c.set_tuning("pow_round_log", ROUND_LOG)
        equals_oracle(prove(c, zkm, oracle, 9), oracle, 9)
        equals_oracle(prove(c, zkm, oracle, 3), oracle, 3)
    finally:
        c.close()
