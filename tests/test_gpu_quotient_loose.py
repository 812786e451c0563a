"""The Poseidon table's constraint evaluator works on loose words (any uint64 standing for its residue) and runs the partial rounds in
the fused textbook form; its consumer sums runs of constraints unreduced.  Two checks that the stored words did not change:

* ctx.quotient against the oracle's quotient_poseidon word for word -- on a valid witness, on uniformly random columns (no row satisfies
  anything: the fused partial rounds must be the same POLYNOMIAL as the reference's sparse form, not only agree on valid rows) and on
  constant columns of edge words (a constant column's LDE is that constant at every point: the only way to put chosen words in front of
  the evaluator through the public path), with edge challenges;
* the consumer alone (zkm_consumer_selftest) against Python integers, on terms and challenges the trace never holds.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
EDGE = [w % P for w in (0, 1, 2, P - 1, P - 2, 2**32 - 1, 2**32 - 2, 2**32, P - 2**32, 2**63, 2**63 - 1, 2**64 - 2**32, 2**64 - 2**33 + 1)]
RUN = 8  # consumer_t::RUN (constraints_dev.h)


def constant_columns(rng, ncols, n):
    words = np.array(EDGE, dtype=np.uint64)[rng.integers(0, len(EDGE), ncols)]
    return np.repeat(words, n)


def traces(oracle, kind, log_n):
    """(trace, aux for [1, 1], aux for [3]) of one kind, column-major."""
    n = 1 << log_n
    rng = np.random.default_rng(1000 * log_n + len(kind))
    if kind == "valid":
        return oracle.poseidon_trace(11, n - 2, log_n), rng.integers(0, P, 4 * n, dtype=np.uint64), rng.integers(0, P, 4 * n, dtype=np.uint64)
    if kind == "random":
        return tuple(rng.integers(0, P, c * n, dtype=np.uint64) for c in (262, 4, 4))
    return tuple(constant_columns(rng, c, n) for c in (262, 4, 4))


@pytest.mark.parametrize("kind", ["valid", "random", "constant"])
@pytest.mark.parametrize("log_n", [5, 7])
def test_quotient_on_loose_words_matches_oracle(ctx, zkm, oracle, log_n, kind):
    trace, aux2, aux3 = traces(oracle, kind, log_n)
    rng = np.random.default_rng(77 + log_n)
    pairs = [(P - 1, 2**32 - 1), (1, 0), (P - 1, P - 1), tuple(int(x) for x in rng.integers(0, P, 2, dtype=np.uint64))]
    tb = zkm.PolynomialBatch.from_values(ctx, trace, 262, log_n)
    ab2 = zkm.PolynomialBatch.from_values(ctx, aux2, 4, log_n)
    ab3 = zkm.PolynomialBatch.from_values(ctx, aux3, 4, log_n)
    otb = oracle.batch_from_values(trace, 262, log_n)
    oab2, oab3 = oracle.batch_from_values(aux2, 4, log_n), oracle.batch_from_values(aux3, 4, log_n)
    for pair in pairs:
        alphas = np.array(pair, dtype=np.uint64)
        got, want = ctx.quotient(tb, ab2, [1, 1], alphas), oracle.quotient_poseidon(otb, oab2, [1, 1], alphas)
        assert (got == want).all(), "two challenges %s" % (pair,)
        got, want = ctx.quotient(tb, ab3, [3], alphas[:1]), oracle.quotient_poseidon(otb, oab3, [3], alphas[:1])
        assert (got == want).all(), "one challenge %s" % (pair[:1],)
        if kind != "valid":
            assert want.any()   # (the oracle's side is not trivially zero on these traces)
    for b in (tb, ab2, ab3):
        b.free()


LANES = 64 + 37   # one full wave and one partly filled wave


def terms_of(kind, K, rng):
    if kind == "random":
        return rng.integers(0, 1 << 64, (K, LANES), dtype=np.uint64)
    col = {"max": [M64] * K, "p": [P] * K, "p-1": [P - 1] * K, "alternating": [0 if i % 2 == 0 else M64 for i in range(K)]}[kind]
    return np.repeat(np.array(col, dtype=np.uint64)[:, None], LANES, axis=1)


def horner(terms, alpha):
    """sum_k terms[k] alpha^(K-1-k) mod p per lane, in Python integers (identical lanes computed once)."""
    cols = {}
    out = []
    for lane in range(terms.shape[1]):
        key = terms[:, lane].tobytes()
        if key not in cols:
            acc = 0
            for t in terms[:, lane].tolist():
                acc = (acc * alpha + t) % P
            cols[key] = acc
        out.append(cols[key])
    return out


@pytest.mark.parametrize("K", [1, RUN - 1, RUN, RUN + 1, 2 * RUN + 1, 248, 797])
def test_consumer_on_loose_terms(ctx, K):
    rng = np.random.default_rng(K)
    r = [int(x) for x in rng.integers(0, P, 3, dtype=np.uint64)]
    challenge_sets = [[0, 1], [P - 1, 2**32], [r[0], r[1]], [r[2]], [2**32], [M64, P]]
    for kind in ("max", "p", "p-1", "alternating", "random"):
        terms = terms_of(kind, K, rng)
        for alphas in challenge_sets:
            want = np.array([horner(terms, a % P) for a in alphas], dtype=np.uint64)
            for run in (RUN, 1, 5):
                got = ctx.consumer_selftest(alphas, terms, run)
                assert got.shape == want.shape and (got == want).all(), "K %d, %s terms, challenges %s, runs of %d" % (K, kind, alphas, run)


def test_consumer_selftest_rejects_bad_arguments(ctx, zkm):
    terms = np.zeros((3, 4), dtype=np.uint64)
    for alphas, run in (([1], 0), ([1], RUN + 1), ([1, 2, 3], RUN)):
        with pytest.raises(zkm.ZkmError):
            ctx.consumer_selftest(alphas, terms, run)
    with pytest.raises(zkm.ZkmError):
        ctx.consumer_selftest([1], np.zeros((0, 4), dtype=np.uint64))
