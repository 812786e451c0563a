"""The one-lane leaf kernels after the sponge's linear layers were re-formed (constants as the addend of each sum's first multiply-add,
poseidon_dev.h / gl_dev.h gl_mad_imm_sc): k_merkle_leaves[_mfma], k_merkle_leaves_ext[_mfma] and k_merkle_leaves_chunk[_mfma] against the
CPU oracle, digest for digest.  Every context here has the latency forms switched off (wide_max_hashes = quad_max_hashes = 0), so that
small launches take the one-lane kernels, once with the MDS layers of the full rounds on the matrix core (leaf_mfma 1) and once on the
vector ALU (leaf_mfma 0)."""
import numpy as np
import pytest

P = 0xFFFFFFFF00000001
# words at the edges of the 32-bit halves the linear layers work on
CONSTANTS = (0, 1, 2**32 - 1, 2**32, P - 2**32, P - 1)
#   W = 5: one ragged absorb; 8: exactly one chunk; 9: the capacity is carried into a second permutation; 262: 33 absorbs, the last of 6 words
#   log_n = 4: 64 leaves = one wave, three idle waves in its workgroup (MFMA ignores EXEC); log_n = 7: two workgroups
SHAPES = [(log_n, W) for log_n in (4, 7) for W in (5, 8, 9, 262)]


def one_lane_context(zkm, mfma):
    c = zkm.Context(0)
    for k in ("wide_max_hashes", "quad_max_hashes"):
        c.set_tuning(k, 0)
    c.set_tuning("leaf_mfma", mfma)
    return c


@pytest.fixture(scope="module", params=[1, 0], ids=["mfma", "valu"])
def lane_ctx(zkm, request):
    c = one_lane_context(zkm, request.param)
    yield c
    c.close()


def traces(log_n, W):
    """uniform words below p, and a trace whose columns are the constants"""
    n = 1 << log_n
    rng = np.random.default_rng(9100 + 16 * W + log_n)
    uniform = rng.integers(0, P, W * n, dtype=np.uint64)
    const = np.repeat(np.array([CONSTANTS[j % len(CONSTANTS)] for j in range(W)], dtype=np.uint64), n)   # column-major: column j is words [j n, (j + 1) n)
    return {"uniform": uniform, "constants": const}


_WANT = {}


def oracle_layers(oracle, log_n, W):
    """(cap, [digest layer 0 .. top]) of both traces of a shape, computed once and shared by the two forms"""
    if (log_n, W) not in _WANT:
        out = {}
        for name, vals in traces(log_n, W).items():
            ob = oracle.batch_from_values(vals, W, log_n)
            out[name] = (ob.cap().copy(), [ob.digest_layer(l).copy() for l in range(ob.lde_bits - ob.cap_height + 1)])
        _WANT[(log_n, W)] = out
    return _WANT[(log_n, W)]


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,W", SHAPES)
def test_one_lane_leaves_match_the_oracle(lane_ctx, zkm, oracle, log_n, W):
    """PolynomialBatch.from_values: the cap and every digest layer, level 0 (the leaf digests) included."""
    want = oracle_layers(oracle, log_n, W)
    for name, vals in traces(log_n, W).items():
        cap, layers = want[name]
        b = zkm.PolynomialBatch.from_values(lane_ctx, vals, W, log_n)
        try:
            assert (b.cap() == cap).all(), name
            assert len(layers) == b.lde_bits - b.cap_height + 1
            for level, layer in enumerate(layers):
                assert (b.digest_layer(level) == layer).all(), (name, level)
        finally:
            b.free()


@pytest.mark.gpu
def test_openings_proof_on_one_lane_kernels_matches_the_oracle(lane_ctx, zkm, oracle):
    """prove_openings at 2^7 rows: the FRI layers' leaves (pairs of extension-field values) go through k_merkle_leaves_ext[_mfma]."""
    log_n, W, A, Q, Z = 7, 13, 4, 4, 2
    n = 1 << log_n
    rng = np.random.default_rng(9300)
    tv, av, qc = (rng.integers(0, P, k * n, dtype=np.uint64) for k in (W, A, Q))
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


@pytest.mark.gpu
@pytest.mark.parametrize("mfma", [1, 0], ids=["mfma", "valu"])
def test_chunked_host_ingest_on_one_lane_kernels_matches_the_oracle(zkm, oracle, mfma):
    """A host-resident 70 x 2^13 matrix absorbed in column chunks of 32 (k_merkle_leaves_chunk[_mfma]): 32 + 32 + a ragged chunk of 6."""
    log_n, W = 13, 70
    vals = np.random.default_rng(9400).integers(0, P, W << log_n, dtype=np.uint64)
    if "chunk" not in _WANT:
        ob = oracle.batch_from_values(vals, W, log_n)
        _WANT["chunk"] = (ob.cap().copy(), ob.digest_layer(0).copy())
    cap, leaves = _WANT["chunk"]
    c = one_lane_context(zkm, mfma)
    try:
        c.set_tuning("ingest_chunk_cols", 32)
        b = zkm.PolynomialBatch.from_values(c, vals, W, log_n)
        assert (b.cap() == cap).all()
        assert (b.digest_layer(0) == leaves).all()
        b.free()
    finally:
        c.close()
