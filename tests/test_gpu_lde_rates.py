"""GPU parity: low-degree extensions at rates other than 4, word for word against the CPU oracle.

zkm_lde_bitrev has its fast paths (the coset split, the one-workgroup transform) for rate_bits 2 only; a commitment at rate 2 or 8 goes
through the general multi-pass transform, whose first pass reads the zero-padded input through bounds-checked loads.  The sizes below
take every plan of that transform under 2^19 points -- one pass, two passes with and without the six-stage last pass, both three-pass
splits (2^17: 5 + 6 + 6, 2^18: 6 + 6 + 6) -- and both sides of the switch to one-leaf-per-lane hashing above 2^14 LDE rows.  EVERY LDE
word is judged: the whole bottom digest layer is compared, since each word feeds one leaf.

The second part proves the STARK opening instance at rate 8 (plonky2's standard_recursion_config rate) with zkm_fri_prove and compares
it with the oracle's prove_openings blob from the first FRI cap on; the oracle's rate-8 proof is itself judged by the Python model of
verify_fri_proof (tests/fri_verify_model.py)."""
import ctypes as C

import numpy as np
import pytest

from . import fri_verify_model as M
from .test_gpu_primitives import EDGE

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001

# (rate_bits, log_n, ncols): transform lengths 2^7 .. 2^18 at rate 8, 2^4 .. 2^18 at rate 2.  Nine columns (a ragged sponge chunk behind
# a whole one) at least once per number of passes; one or three columns at most of the large sizes, where the oracle's hashing is the cost.
SIZES = [(3, 4, 9), (3, 5, 3), (3, 6, 1), (3, 7, 9), (3, 9, 3), (3, 11, 9), (3, 12, 1), (3, 13, 9), (3, 14, 9), (3, 15, 3),
         (1, 3, 3), (1, 7, 9), (1, 8, 9), (1, 11, 1), (1, 13, 3), (1, 15, 9), (1, 16, 1), (1, 17, 3)]
CAP_HEIGHT = 4


def passes(L):
    return (L + 7) // 8


def plan(L):
    """the stages of each pass over 2^L points (make_plan of ntt.hip: the larger radices last, a six-stage last pass where the others
    can absorb the rest)"""
    np_ = passes(L)
    S = [L // np_ + (1 if i >= np_ - L % np_ else 0) for i in range(np_)]
    k, rest = np_ - 1, L - 6
    if np_ >= 2 and 3 * k <= rest <= 8 * k:
        S = [rest // k + (1 if i >= k - rest % k else 0) for i in range(k)] + [6]
    assert sum(S) == L
    return tuple(S)


def test_the_sizes_cover_every_plan():
    for rate_bits, log_ns in ((3, [4, 5, 6, 7, 9, 11, 12, 13, 14, 15]), (1, [3, 7, 8, 11, 13, 15, 16, 17])):
        assert [s[1] for s in SIZES if s[0] == rate_bits] == log_ns
    Ls = {r + n for r, n, _ in SIZES}
    assert Ls == {4, 7, 8, 9, 10, 12, 14, 15, 16, 17, 18}
    plans = {plan(L) for L in Ls}
    assert {len(p) for p in plans} == {1, 2, 3}
    assert any(len(p) == 2 and p[1] == 6 for p in plans) and any(len(p) == 2 and p[1] != 6 for p in plans)
    assert {(5, 6, 6), (6, 6, 6)} <= plans
    assert any(L <= 14 for L in Ls) and any(L > 14 for L in Ls)                    # both leaf kernels
    assert {passes(r + n) for r, n, c in SIZES if c == 9} == {1, 2, 3}
    assert all(c in (1, 3, 9) for _, _, c in SIZES) and any(c != 9 for r, n, c in SIZES if r + n >= 17)


def values(rate_bits, log_n, ncols):
    rng = np.random.default_rng(9000 + 100 * rate_bits + log_n)
    vals = rng.integers(0, P, ncols << log_n, dtype=np.uint64)
    k = min(len(EDGE), vals.size)
    vals[:k] = EDGE[:k]
    return vals


def rows_to_open(N):
    """0, 1, N / 2 + 3, N - 1 and the first row of every eighth of N (the block boundaries of the bit-reversed order)"""
    return sorted({0, 1, N // 2 + 3, N - 1} | {j * N // 8 for j in range(1, 8)})


def same_commitment(b, ob, what):
    got, want = b.digest_layer(0), ob.digest_layer(0)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d leaf digests differ, the first is leaf %d" % (what, len(set(bad // 4)), bad[0] // 4)
    assert (b.cap() == ob.cap()).all(), what
    for i in rows_to_open(1 << b.lde_bits):
        assert (b.lde_row(i) == ob.lde_row(i)).all(), (what, i)
        assert (b.leaf(i) == ob.leaf(i)).all(), (what, i)
        assert (b.merkle_path(i) == ob.merkle_path(i)).all(), (what, i)


@pytest.mark.parametrize("rate_bits,log_n,ncols", SIZES)
def test_commitment_at_another_rate(ctx, zkm, oracle, rate_bits, log_n, ncols):
    vals = values(rate_bits, log_n, ncols)
    ob = oracle.batch_from_values(vals, ncols, log_n, rate_bits, CAP_HEIGHT)
    b = zkm.PolynomialBatch.from_values(ctx, vals, ncols, log_n, rate_bits, CAP_HEIGHT)
    try:
        assert (b.coeffs() == ob.coeffs()).all()
        same_commitment(b, ob, "from_values")
    finally:
        b.free()


@pytest.mark.parametrize("rate_bits,log_n,ncols", [(3, 11, 9), (1, 15, 9)])
def test_commitment_from_coefficients_at_another_rate(ctx, zkm, oracle, rate_bits, log_n, ncols):
    ob = oracle.batch_from_values(values(rate_bits, log_n, ncols), ncols, log_n, rate_bits, CAP_HEIGHT)
    b = zkm.PolynomialBatch.from_coeffs(ctx, ob.coeffs(), ncols, log_n, rate_bits, CAP_HEIGHT)
    try:
        assert (b.coeffs() == ob.coeffs()).all()
        same_commitment(b, ob, "from_coeffs")
    finally:
        b.free()


@pytest.mark.parametrize("rate_bits,log_n,ncols", [(3, 9, 3), (1, 11, 1)])
def test_the_lde_does_not_depend_on_the_inverse_transforms_plan(zkm, oracle, rate_bits, log_n, ncols):
    """small_ntt 0: the inverse transform of 2^9 .. 2^13 values is two passes instead of one workgroup; the LDE must not change"""
    vals = values(rate_bits, log_n, ncols)
    ob = oracle.batch_from_values(vals, ncols, log_n, rate_bits, CAP_HEIGHT)
    c = zkm.Context(0)
    try:
        c.set_tuning("small_ntt", 0)
        b = zkm.PolynomialBatch.from_values(c, vals, ncols, log_n, rate_bits, CAP_HEIGHT)
        assert (b.coeffs() == ob.coeffs()).all()
        same_commitment(b, ob, "small_ntt 0")
        b.free()
    finally:
        c.close()


@pytest.mark.parametrize("log_n", [9, 13])
def test_fri_proof_at_rate_8_equals_the_oracles(ctx, zkm, oracle, log_n):
    """The STARK instance of test_generic_fri_instance_equals_the_stark_instance (13 + 4 + 4 polynomials, two Z) under rate_bits 3.
    zkm_prove_openings refuses that rate, so the transcript is replayed from the ORACLE's blob up to the draw of alpha; zkm_fri_prove on
    the three rate-8 commitments must then give the oracle's FRI part word for word -- caps, final polynomial, witness, all query rounds --
    and leave the challenger in the oracle's state.  The oracle's blob is accepted by its own verifier and by the Python model."""
    from .test_fri_verify_model import SEED_WORDS, claim_of_stark_blob, params_of
    W, A, Q, Z = 13, 4, 4, 2
    rng = np.random.default_rng(8300 + log_n)
    n = 1 << log_n
    tv, av, qc = (rng.integers(0, P, k * n, dtype=np.uint64) for k in (W, A, Q))
    cfg, ocfg = ctx.standard_config(), oracle.standard_config()
    cfg.rate_bits = ocfg.rate_bits = 3
    otb, oab = oracle.batch_from_values(tv, W, log_n, 3, ocfg.cap_height), oracle.batch_from_values(av, A, log_n, 3, ocfg.cap_height)
    oqb = oracle.batch_from_coeffs(qc, Q, log_n, 3, ocfg.cap_height)
    och = oracle.challenger()
    oracle.observe(och, SEED_WORDS)
    blob = oracle.prove_openings(otb, oab, oqb, Z, challenger=och, cfg=ocfg)
    lay, _ = zkm.proof_layout(blob)
    assert int(lay.rate_bits) == 3 and int(lay.degree_bits) == log_n
    # the oracle's rate-8 proof before two independent judges
    vch = oracle.challenger()
    oracle.observe(vch, SEED_WORDS)
    assert oracle.verify_openings(blob, W, A, Z, challenger=vch, cfg=ocfg) == 0
    params = params_of(ocfg)
    caps, batches, opened, fri_words, mch = claim_of_stark_blob(zkm, params, log_n, blob)
    assert M.verify(params, log_n, [W, A, Q], caps, batches, opened, fri_words, mch) == (M.OK, 0, 0, 0)
    # the device: the commitments, then the FRI part behind the replayed transcript (proof.rs:336-367)
    tb, ab = zkm.PolynomialBatch.from_values(ctx, tv, W, log_n, 3, cfg.cap_height), zkm.PolynomialBatch.from_values(ctx, av, A, log_n, 3, cfg.cap_height)
    qb = zkm.PolynomialBatch.from_coeffs(ctx, qc, Q, log_n, 3, cfg.cap_height)
    try:
        for b, off in ((tb, lay.trace_cap), (ab, lay.aux_cap), (qb, lay.quotient_cap)):
            assert (b.cap() == blob[off:off + (4 << cfg.cap_height)]).all()
        ch = zkm.challenger_new()
        zkm.challenger_observe(ch, SEED_WORDS)
        st = np.zeros(12, dtype=np.uint64)
        zkm.load().zkm_challenger_compact(C.byref(ch), st.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert (st == blob[lay.init_challenger_state:lay.init_challenger_state + 12]).all()
        zeta = (int(zkm.challenger_get(ch)), int(zkm.challenger_get(ch)))
        g = oracle.root_of_unity(log_n)
        zeta_next = (zeta[0] * g % P, zeta[1] * g % P)
        for off, words in ((lay.local_values, 2 * W), (lay.aux_polys, 2 * A), (lay.quotient_polys_open, 2 * Q), (lay.next_values, 2 * W),
                           (lay.aux_polys_next, 2 * A)):
            zkm.challenger_observe(ch, blob[off:off + words])
        for i in range(Z):
            zkm.challenger_observe(ch, [int(blob[lay.ctl_zs_first + i]), 0])
        assert batches == [(zeta, batches[0][1]), (zeta_next, batches[1][1]), ((1, 0), batches[2][1])]      # (the model's replay agrees)
        fri = ctx.fri_prove([tb, ab, qb], batches, ch, cfg)
        assert int(fri[0]) == int.from_bytes(b"ZKMFRIPF", "little")
        assert [int(x) for x in fri[1:9]] == [log_n, 3, 4, int(lay.fri_layers), int(lay.final_poly_len), 37, 3, 4]
        assert [int(x) for x in fri[16:19]] == [W, A, Q]
        want = blob[lay.commit_phase_merkle_caps:]
        assert fri.size - 24 == want.size
        bad = np.nonzero(fri[24:] != want)[0]
        assert bad.size == 0, "first differing word of the FRI part: %d of %d (the witness is word %d)" % (
            bad[0], want.size, int(lay.pow_witness) - int(lay.commit_phase_merkle_caps))
        assert list(ch.state) == list(och.state) and ch.n_in == och.n_in and ch.n_out == och.n_out
    finally:
        for b in (tb, ab, qb):
            b.free()
