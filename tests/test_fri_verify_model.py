"""CPU suite: tests/fri_verify_model.py, the Python model of plonky2's verify_fri_proof, pinned to the CPU oracle where the oracle
reaches: the STARK instance (three oracles; batches at zeta, g zeta and 1).

The oracle makes a prove_openings blob (W, A, Q, Z = 13, 4, 4, 2; log_n 6 and 9; standard config with six queries); its FRI part, cut
out behind a "ZKMFRIPF" header (tests/test_gpu_prove.py shows the correspondence), its caps and its openings are the claim, and the
transcript is replayed on the model's challenger to the point where alpha is drawn.  The model must accept, and for one changed word of
each kind of field it must accept exactly when zko_verify_openings does."""
import numpy as np
import pytest

from . import fri_verify_model as M

P = M.P
W, A, Q, Z = 13, 4, 4, 2
SEED_WORDS = [7, 8, 9]


def params_of(cfg):
    return {k: int(getattr(cfg, k)) for k in ("rate_bits", "cap_height", "pow_bits", "num_queries", "arity_bits", "final_poly_bits")}


def stark_batches(zeta, zeta_next):
    polys0 = [(0, c) for c in range(W)] + [(1, c) for c in range(A)] + [(2, c) for c in range(Q)]
    polys1 = [(0, c) for c in range(W)] + [(1, c) for c in range(A)]
    return [(zeta, polys0), (zeta_next, polys1), ((1, 0), [(1, c) for c in range(A - Z, A)])]


def claim_of_stark_blob(zkm, params, log_n, blob):
    """The STARK blob of prove_openings -> what verify_fri_proof takes: (caps, batches, opened, FRI blob, challenger at the alpha draw)"""
    lay, _ = zkm.proof_layout(blob)
    sec = lambda off, words: [int(x) for x in blob[int(off):int(off) + words]]
    ch = M.Challenger()
    ch.observe(SEED_WORDS)
    if ch.inputs:               # Challenger::compact
        ch._duplex()
    ch.outputs = []
    assert ch.state == sec(lay.init_challenger_state, 12)
    zeta = ch.get_ext()
    g = M.root_of_unity(log_n)
    local, aux, quot = sec(lay.local_values, 2 * W), sec(lay.aux_polys, 2 * A), sec(lay.quotient_polys_open, 2 * Q)
    nxt, aux_next = sec(lay.next_values, 2 * W), sec(lay.aux_polys_next, 2 * A)
    first = [w for z in sec(lay.ctl_zs_first, Z) for w in (z, 0)]
    for words in (local, aux, quot, nxt, aux_next, first):      # observe_openings (proof.rs:336-367)
        ch.observe(words)
    cap_words = 4 << params["cap_height"]
    caps = [sec(off, cap_words) for off in (lay.trace_cap, lay.aux_cap, lay.quotient_cap)]
    o = M.offsets(params, log_n, [W, A, Q])
    header = [M.MAGIC, log_n, 3, params["cap_height"], o["L"], o["F"], params["num_queries"], params["rate_bits"], params["arity_bits"]] + [0] * 7 + \
        [W, A, Q] + [0] * 5
    fri = header + [int(x) for x in blob[int(lay.commit_phase_merkle_caps):]]
    batches = stark_batches(zeta, (zeta[0] * g % P, zeta[1] * g % P))
    return caps, batches, [local + aux + quot, nxt + aux_next, first], fri, ch


@pytest.fixture(scope="module", params=[6, 9])
def proven(request, oracle, zkm):
    log_n = request.param
    n = 1 << log_n
    rng = np.random.default_rng(4100 + log_n)
    tv, av, qc = (rng.integers(0, P, k * n, dtype=np.uint64) for k in (W, A, Q))
    cfg = oracle.standard_config()
    cfg.num_queries = 6
    ch = oracle.challenger()
    oracle.observe(ch, SEED_WORDS)
    tb, ab, qb = oracle.batch_from_values(tv, W, log_n), oracle.batch_from_values(av, A, log_n), oracle.batch_from_coeffs(qc, Q, log_n)
    blob = oracle.prove_openings(tb, ab, qb, Z, challenger=ch, cfg=cfg).copy()
    return log_n, cfg, blob


def oracle_accepts(oracle, cfg, blob):
    ch = oracle.challenger()
    oracle.observe(ch, SEED_WORDS)
    return oracle.verify_openings(blob, W, A, Z, challenger=ch, cfg=cfg) == 0


def model_code(zkm, cfg, log_n, blob):
    params = params_of(cfg)
    caps, batches, opened, fri, ch = claim_of_stark_blob(zkm, params, log_n, blob)
    return M.verify(params, log_n, [W, A, Q], caps, batches, opened, fri, ch)


def test_the_model_accepts_what_the_oracle_proves(proven, oracle, zkm):
    log_n, cfg, blob = proven
    assert oracle_accepts(oracle, cfg, blob)
    assert model_code(zkm, cfg, log_n, blob) == (M.OK, 0, 0, 0)


def field_words(zkm, cfg, log_n, blob):
    """{kind of field: word of the STARK blob} for one word of each kind, in the second query's round where the kind lies in one"""
    lay, q = zkm.proof_layout(blob)
    params = params_of(cfg)
    caps, batches, opened, fri, ch = claim_of_stark_blob(zkm, params, log_n, blob)
    _, _, _, indices = M.fri_challenges(params, log_n, M.parse(params, log_n, [W, A, Q], fri), ch)
    k = 1
    entry = indices[k] >> (log_n + params["rate_bits"] - params["cap_height"])      # the cap entry query k's paths end in
    base = int(lay.query_round_proofs) + k * int(lay.query_round_words)
    out = {"oracle row": base + int(q.oracle_evals[1]) + 2, "oracle sibling": base + int(q.oracle_siblings[0]) + 5,
           "final polynomial": int(lay.final_poly) + 3, "pow witness": int(lay.pow_witness), "opened value": int(lay.aux_polys) + 1,
           "opened value at g zeta": int(lay.next_values) + 4, "ctl_zs_first": int(lay.ctl_zs_first), "oracle cap": int(lay.quotient_cap) + 4 * entry + 2}
    if int(lay.fri_layers):
        within = indices[k] & ((1 << params["arity_bits"]) - 1)
        out["layer value at the queried position"] = base + int(q.layer_evals[0]) + 2 * within
        out["another value of the same coset"] = base + int(q.layer_evals[0]) + 2 * (within ^ 5) + 1
        out["layer cap"] = int(lay.commit_phase_merkle_caps) + 4 * entry + 1
        if int(q.layer_siblings_count[0]):
            out["layer sibling"] = base + int(q.layer_siblings[0]) + 1
    return out


def test_the_model_rejects_what_the_oracle_rejects(proven, oracle, zkm):
    log_n, cfg, blob = proven
    words = field_words(zkm, cfg, log_n, blob)
    assert {"oracle row", "oracle sibling", "layer value at the queried position", "another value of the same coset", "layer cap",
            "final polynomial", "pow witness", "opened value", "oracle cap"} <= set(words)
    assert log_n == 6 or "layer sibling" in words      # (2^6 rows: the layer's tree is its cap)
    for kind, at in words.items():
        bad = blob.copy()
        bad[at] = (int(bad[at]) + 1) % P
        code = model_code(zkm, cfg, log_n, bad)
        assert (code[0] == M.OK) == oracle_accepts(oracle, cfg, bad), (kind, code)
        assert code[0] != M.OK, kind


def test_the_challenger_is_the_librarys(zkm):
    """the model's duplex challenger against zkm_challenger_* over a mixed sequence of observations and draws"""
    ch, mine = zkm.challenger_new(), M.Challenger()
    rng = np.random.default_rng(4200)
    for step in range(40):
        words = [int(x) for x in rng.integers(0, P, int(rng.integers(0, 12)), dtype=np.uint64)]
        zkm.challenger_observe(ch, words)
        mine.observe(words)
        for _ in range(int(rng.integers(0, 11))):
            assert int(zkm.challenger_get(ch)) == mine.get(), step
    assert list(ch.state) == mine.state and list(ch.in_buf)[:ch.n_in] == mine.inputs and list(ch.out_buf)[:ch.n_out] == mine.outputs
