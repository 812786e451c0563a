"""GPU parity of the four-round partial groups of the one-lane permutation (csrc/poseidon_dev.h poseidon_partial_group_t<4>,
poseidon_fold_wide) through zkm_poseidon_selftest, against the textbook rounds of tests/poseidon_model.py (the groups: tests/poseidon_group4_model.py) -- bit for bit where the device
promises canonical words, mod p where its output is loose -- and of the commitments that run on the one-lane kernels, against the oracle.

The inputs are the ones on which a half-sum of an M^4 row passes 2^64: twelve words of all ones (both half-sums of every row), all-ones
high or low halves (one of them), the words around p and 2^32 in uniform, alternating and one-hot states, one all-ones state alone in a
wave of field data (the corrections are branched on per wave and applied per lane), and a partly filled last wave."""
import functools

import numpy as np
import pytest

from . import poseidon_group4_model as g4
from . import poseidon_model as pm

pytestmark = pytest.mark.gpu
P = pm.P
_U64_P = np.uint64(P)
ALL, CAPACITY, DIGEST = 0, 1, 2
CUT = 64 * 5 + 17 + 1       # the list cut just behind the lone all-ones state: lane 17 is the last live lane of its wave


@functools.lru_cache(maxsize=None)
def inputs():
    a = np.array(g4.group4_states(), dtype=np.uint64)
    a.setflags(write=False)
    return a


def model_array(fn):
    a = np.array([fn(list(s)) for s in g4.group4_states()], dtype=np.uint64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want_group4(g):
    return model_array(lambda s: g4.group4(s, g))


@functools.lru_cache(maxsize=None)
def want_permute():
    return model_array(pm.permute)


def reduce(got):
    return np.where(got >= _U64_P, got - _U64_P, got)


def compare(what, got, want, words=range(12), canonical=False):
    words = list(words)
    src = inputs()[:len(got)]
    g, w = got[:, words], want[:len(got), words]
    bad = np.argwhere((g if canonical else reduce(g)) != w)
    if len(bad):
        i, k = int(bad[0][0]), words[int(bad[0][1])]
        raise AssertionError("%s: state %d word %d: got %#x, want %#x%s; %d words differ; input state %s" % (
            what, i, k, int(got[i, k]), int(want[i, k]), "" if canonical else " (mod p)", len(bad), [hex(int(x)) for x in src[i]]))


def check(ctx, probe, arg, want, **kw):
    """The whole list (its last wave holds 37 states), and the list cut behind the lone all-ones state."""
    assert len(inputs()) == g4.GROUP4_CUT and CUT == g4.GROUP4_LONE + 1
    for n in (len(inputs()), CUT):
        got = ctx.poseidon_selftest(probe, arg, inputs()[:n])
        assert got.shape == (n, 12)
        compare("%s arg %d (%d states)" % (probe, arg, n), got, want, **kw)
    return got


@pytest.mark.parametrize("g", range(5))
def test_four_round_group(ctx, g):
    check(ctx, "GROUP4", g, want_group4(g))


def test_wide_fold(ctx):
    vec = g4.fold_wide_vectors()
    want = [g4.fold_wide_value(*v) for v in vec]
    for n in (len(vec), len(vec) - (len(vec) - 5) % 64):
        got = ctx.poseidon_selftest("FOLD_WIDE", 0, np.array(vec[:n], dtype=np.uint64))
        assert got.shape == (n,)
        bad = [i for i in range(n) if int(got[i]) % P != want[i]]
        assert not bad, "triple %d (%#x, %#x, carries %d): got %#x, want %#x (mod p); %d triples differ" % (
            (bad[0],) + tuple(vec[bad[0]]) + (int(got[bad[0]]), want[bad[0]], len(bad)))


@pytest.mark.parametrize("probe", ["PERMUTE_LANE", "PERMUTE_LANE_MFMA"])
def test_whole_permutation_in_the_three_output_modes(ctx, probe):
    full = check(ctx, probe, ALL, want_permute(), canonical=True)
    assert (full < _U64_P).all()
    check(ctx, probe, CAPACITY, want_permute(), words=range(8, 12))
    check(ctx, probe, DIGEST, want_permute(), words=range(0, 4), canonical=True)


def test_selftest_rejects_a_group_that_does_not_exist(ctx, zkm):
    one = np.zeros(12, dtype=np.uint64)
    for probe, arg, words in (("GROUP4", 5, one), ("FOLD_WIDE", 1, one), (16, 0, one), (19, 0, one)):
        with pytest.raises(zkm.ZkmError):
            ctx.poseidon_selftest(probe, arg, words)
    with pytest.raises(ValueError):
        ctx.poseidon_selftest("FOLD_WIDE", 0, np.zeros(4, dtype=np.uint64))


# ---------------------------------------------------------------- commitments on the one-lane kernels
#   W = 262: 33 absorbs, the last of 6 words; 13: one full and one ragged absorb; 9: the capacity carried into a one-word absorb
SHAPES = [(log_n, W) for log_n in (5, 8) for W in (262, 13, 9)]
_WANT = {}


@pytest.fixture(scope="module", params=[1, 0], ids=["mfma", "valu"])
def lane_ctx(zkm, request):
    c = zkm.Context(0)
    for k in ("wide_max_hashes", "quad_max_hashes"):   # the latency forms off: small launches take the one-lane kernels too
        c.set_tuning(k, 0)
    c.set_tuning("leaf_mfma", request.param)
    yield c
    c.close()


def values(log_n, W):
    return np.random.default_rng(9500 + 16 * W + log_n).integers(0, P, W << log_n, dtype=np.uint64)


@pytest.mark.parametrize("log_n,W", SHAPES)
def test_from_values_commitments_match_the_oracle(lane_ctx, zkm, oracle, log_n, W):
    """PolynomialBatch.from_values: the cap and every digest layer, level 0 (the leaf digests) included."""
    vals = values(log_n, W)
    if (log_n, W) not in _WANT:
        ob = oracle.batch_from_values(vals, W, log_n)
        _WANT[(log_n, W)] = (ob.cap().copy(), [ob.digest_layer(l).copy() for l in range(ob.lde_bits - ob.cap_height + 1)])
    cap, layers = _WANT[(log_n, W)]
    b = zkm.PolynomialBatch.from_values(lane_ctx, vals, W, log_n)
    try:
        assert (b.cap() == cap).all()
        assert len(layers) == b.lde_bits - b.cap_height + 1
        for level, layer in enumerate(layers):
            assert (b.digest_layer(level) == layer).all(), level
    finally:
        b.free()


def test_fri_layer_commitments_match_the_oracle(lane_ctx, zkm, oracle):
    """prove_openings at 2^8 rows: the FRI layers' leaves (pairs of extension-field values) are committed by the one-lane ext kernels; the
    proof carries every layer's cap and the opened paths."""
    log_n, W, A, Q, Z = 8, 13, 4, 4, 2
    rng = np.random.default_rng(9600)
    tv, av, qc = (rng.integers(0, P, k << log_n, dtype=np.uint64) for k in (W, A, Q))
    if "openings" not in _WANT:
        otb, oab, oqb = oracle.batch_from_values(tv, W, log_n), oracle.batch_from_values(av, A, log_n), oracle.batch_from_coeffs(qc, Q, log_n)
        _WANT["openings"] = oracle.prove_openings(otb, oab, oqb, Z).copy()
    tb, ab = zkm.PolynomialBatch.from_values(lane_ctx, tv, W, log_n), zkm.PolynomialBatch.from_values(lane_ctx, av, A, log_n)
    qb = zkm.PolynomialBatch.from_coeffs(lane_ctx, qc, Q, log_n)
    try:
        assert (lane_ctx.prove_openings(tb, ab, qb, Z) == _WANT["openings"]).all()
    finally:
        for b in (tb, ab, qb):
            b.free()
