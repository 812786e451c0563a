"""GPU suite: zkm_verify_segments / zkm_verify_proofs / zkm_verify_single_table -- verify_proof (verifier.rs:27-176) on the device.
The judge of every verdict is the oracle's sequential verifier (oracle.verify_all / oracle.verify): its return code is translated by
`expected` below and the device's report must name the same check, table, tree and lookup; `query` and `layer` are predicted from
where the test changed the blob.  Then hostile blobs, the launch accounting, and the "verify" key in front of the prove calls.
The rejections here touch four tables, two queries and the quad form of the chain kernel; tests/test_gpu_verify_sweep.py sweeps all
twelve tables, every query, layer and chain in both forms of that kernel, and blobs with more than one finding."""
import ctypes as C
import os

import numpy as np
import pytest

from . import check_ctls_model as M
from . import segment_ops_fixtures as SF

pytestmark = pytest.mark.gpu

P = SF.P
ARITHMETIC, CPU, KECCAK, LOGIC, MEMORY = 0, 1, 4, 10, 11      # positions in Table::all()
MEM_FILTER = 0
PUB = [1, 2]


def expected(code):
    """oracle code -> (report code name, table, tree, ctl); None where the oracle's code does not fix the field."""
    if code == 0:
        return ("OK", None, None, None)
    if code == 40:
        return ("CTL_CHALLENGES", None, None, None)
    if 50 <= code < 1000:
        return ("CTL_SUM", None, None, code - 50)
    t, r = (code // 1000 - 1, code % 1000) if code >= 1000 else (None, code)
    if r in (1, 2, 3):
        return ("SHAPE", t, None, None)
    if 20 <= r < 23:
        return ("INITIAL_MERKLE", t, r - 20, None)
    name = {4: "TRANSCRIPT_STATE", 10: "QUOTIENT", 11: "POW", 30: "FRI_EVAL", 31: "FRI_MERKLE", 32: "FINAL_POLY"}[r]
    return (name, t, None, None)


def judged(rep, code):
    """Assert that a device report says what the oracle's code says; returns the (code name, tree) pair seen."""
    name, table, tree, ctl = expected(code)
    print("oracle %d -> %s; device: %s table %d challenge %d query %d tree %d layer %d ctl %d waits %d  %s" % (
        code, name, rep.name, rep.table, rep.challenge, rep.query, rep.tree, rep.layer, rep.ctl, rep.host_waits, rep.message))
    assert rep.name == name, (rep.name, name)
    assert table is None or rep.table == table
    assert tree is None or rep.tree == tree
    assert ctl is None or rep.ctl == ctl
    assert (rep.message is None) == (code == 0)
    return (name, rep.tree if name == "INITIAL_MERKLE" else 0)


@pytest.fixture(scope="module")
def seg(oracle):
    return SF.build_segment_ops(oracle)


@pytest.fixture(scope="module")
def big(oracle):
    return SF.build_segment_ops(oracle, repeat=128)


@pytest.fixture(scope="module")
def proven(ctx, zkm, seg):
    raw, tables, ctls = seg
    return ctx.prove_segment_ops(SF.segment_ops(zkm, raw), public_values=PUB)


@pytest.fixture(scope="module")
def proven_big(ctx, zkm, big):
    raw, tables, ctls = big
    return ctx.prove_segment_ops(SF.segment_ops(zkm, raw), public_values=PUB)


def bumped(proofs, i):
    out = proofs.copy()
    out[i] = (int(out[i]) + 1) % P
    return out


# ---- 1. accepts what the library proves
def test_accepts_the_fixture_segment_by_every_prove_call(ctx, zkm, oracle, seg, proven):
    raw, tables, ctls = seg
    lg = [t[3] for t in tables]
    proofs, chal, offs = proven
    assert [int(x) for x in SF.reference_log_ns(raw)] == lg
    assert oracle.verify_all(tables, ctls, proofs, chal, PUB) == 0
    for claimed in ([chal], None):
        rep, = ctx.verify_segments([proofs], public_values=[PUB], ctl_challenges=claimed)
        judged(rep, 0)
        assert rep.host_waits == 1
    by_traces = ctx.prove_segment([t[1] for t in tables], lg, public_values=PUB)
    assert np.array_equal(by_traces[0], proofs)
    judged(ctx.verify_segments([by_traces[0]], [PUB], [by_traces[1]])[0], 0)
    three = ctx.prove_segments_ops([SF.segment_ops(zkm, raw)] * 3, public_values=[PUB] * 3)
    reps = ctx.verify_segments([p for p, _, _ in three], [PUB] * 3, [c for _, c, _ in three])
    for rep in reps:
        judged(rep, 0)
    # the general form, heights given by the caller
    judged(ctx.verify_proofs(tables, ctls, proofs, PUB, chal), 0)
    judged(ctx.verify_proofs(tables, ctls, proofs, PUB), 0)
    # another public value: the transcript differs from the first word on
    code = oracle.verify_all(tables, ctls, proofs, chal, PUB + [3])
    assert code == 40
    judged(ctx.verify_segments([proofs], [PUB + [3]], [chal])[0], code)


def test_accepts_the_large_segment_and_a_mixed_call(ctx, oracle, big, proven, proven_big):
    raw, tables, ctls = big
    proofs, chal, offs = proven_big
    assert [t[3] for t in tables][:2] == [16, 15] and tables[MEMORY][3] == 17
    assert oracle.verify_all(tables, ctls, proofs, chal, PUB) == 0
    judged(ctx.verify_segments([proofs], [PUB], [chal])[0], 0)
    reps = ctx.verify_segments([proven[0], proofs, proven[0]], [PUB] * 3, [proven[1], chal, None])   # different heights in one call
    for rep in reps:
        judged(rep, 0)
    # a rejected segment between accepted ones: each report is its own
    lay, _ = ctx_layout(proofs)
    bad = bumped(proofs, lay.quotient_polys_open)
    reps = ctx.verify_segments([proven[0], bad, proven[0]], [PUB] * 3, [proven[1], chal, proven[1]])
    assert [r.name for r in reps] == ["OK", "QUOTIENT", "OK"] and reps[1].table == 0
    assert "segment 1" in reps[1].message and "Arithmetic" in reps[1].message


def ctx_layout(blob):
    import zkm_amd
    return zkm_amd.proof_layout(blob)


def ch_key(ch):
    return (list(ch.state), list(ch.in_buf[:ch.n_in]), list(ch.out_buf[:ch.n_out]))


@pytest.mark.parametrize("log_n", [5, 6, 12])
def test_single_table_proof_and_the_challenger_it_leaves(ctx, zkm, oracle, log_n):
    """Under the standard configuration the three heights are the three shapes of a query round: 5 has no FRI layer (and a final
    polynomial of 32 coefficients), 6 one layer whose tree is already at its cap (no siblings; 4 coefficients), 12 two layers."""
    n = 1 << log_n
    trace = ctx.poseidon_trace(seed=11, num_perms=n - 5, log_n=log_n)
    aux = np.zeros(4 * n, dtype=np.uint64)
    proof = ctx.prove_single_table(trace, log_n, aux, [1, 1])
    trace.free()
    lay, q = ctx_layout(proof)
    assert (lay.fri_layers, lay.final_poly_len) == {5: (0, 32), 6: (1, 4), 12: (2, 16)}[log_n]
    assert log_n != 6 or q.layer_siblings_count[0] == 0
    from oracle.oracle_py import Challenger as OCh
    och, dch = OCh(), zkm.Challenger()
    assert oracle.verify(proof, 4, [1, 1], challenger=och) == 0
    rep = ctx.verify_single_table(proof, [1, 1], challenger=dch)
    judged(rep, 0)
    assert ch_key(och) == ch_key(dch)                    # the transcript stands where the oracle's stands
    # one word of every kind of field, at positions taken from the blob's own layout
    kinds = {"trace cap word", "local value", "ctl_zs_first word", "quotient opening", "final polynomial word", "pow witness", "FRI cap word",
             "last word of the last query"}
    cases = [c for c in tamper_cases(proof, [0, proof.size], 0) if c[0] in kinds] + [("first word of the first query", lay.query_round_proofs, 0, None)]
    assert len(cases) == 8 + (1 if lay.fri_layers else 0)
    for name, i, query, layer in cases:
        bad = bumped(proof, i)
        dch2 = zkm.Challenger()
        code = oracle.verify(bad, 4, [1, 1])
        print("%-32s" % name, end=" ")
        rep = ctx.verify_single_table(bad, [1, 1], challenger=dch2)
        assert code != 0
        if judged(rep, code)[0] in ("INITIAL_MERKLE", "FRI_EVAL", "FRI_MERKLE") and query is not None:
            assert rep.query == query
        assert bytes(dch2) == bytes(zkm.Challenger())    # a rejection leaves the caller's challenger alone


# ---- 2. rejects, and names the same check as the oracle
def tamper_cases(proofs, offs, t):
    """(name, word index in the segment's blobs, predicted query or None, predicted layer or None) for table t."""
    blob = proofs[offs[t]:offs[t + 1]]
    lay, q = ctx_layout(blob)
    o = offs[t]
    cases = [("trace cap word", o + lay.trace_cap + 5, None, None), ("local value", o + lay.local_values + 2, None, None),
             ("next value", o + lay.next_values + 1, None, None), ("auxiliary opening", o + lay.aux_polys, None, None),
             ("ctl_zs_first word", o + lay.ctl_zs_first, None, None), ("quotient opening", o + lay.quotient_polys_open + 3, None, None),
             ("final polynomial word", o + lay.final_poly + 1, None, None), ("pow witness", o + lay.pow_witness, None, None)]
    if lay.fri_layers:
        cases.append(("FRI cap word", o + lay.commit_phase_merkle_caps + 2, None, None))
    for k in (0, 5):
        r = o + lay.query_round_proofs + k * lay.query_round_words
        cases += [("query %d trace evaluation" % k, r + q.oracle_evals[0] + 1, k, None), ("query %d trace sibling" % k, r + q.oracle_siblings[0] + 2, k, None),
                  ("query %d auxiliary evaluation" % k, r + q.oracle_evals[1], k, None), ("query %d quotient evaluation" % k, r + q.oracle_evals[2] + 1, k, None)]
        if lay.fri_layers:
            cases.append(("query %d layer-0 evaluation" % k, r + q.layer_evals[0], k, 0))
            if q.layer_siblings_count[0]:
                cases.append(("query %d layer-0 sibling" % k, r + q.layer_siblings[0] + 1, k, 0))
    cases.append(("last word of the last query", o + lay.total_words - 1, lay.num_queries - 1, max(int(lay.fri_layers) - 1, 0)))
    return cases


def test_rejects_and_names_the_check_the_oracle_names(ctx, oracle, seg, proven):
    raw, tables, ctls = seg
    proofs, chal, offs = proven
    seen = set()

    def run(name, bad, claimed=chal, pub=PUB, query=None, layer=None):
        code = oracle.verify_all(tables, ctls, bad, claimed, pub)
        print("%-44s" % name, end=" ")
        rep = ctx.verify_segments([bad], [pub], [claimed])[0]
        pair = judged(rep, code)
        seen.add(pair)
        assert code != 0
        if pair[0] in ("INITIAL_MERKLE", "FRI_EVAL", "FRI_MERKLE") and query is not None:
            assert rep.query == query
            if pair[0] != "INITIAL_MERKLE" and layer is not None:
                assert rep.layer == layer
        return rep

    for t in (ARITHMETIC, CPU, KECCAK, MEMORY):
        for name, i, query, layer in tamper_cases(proofs, offs, t):
            run("table %d %s" % (t, name), bumped(proofs, i), query=query, layer=layer)
    # the layer-0 evaluation AT the queried position of query 0 (Arithmetic): the one word of a query round whose change is not caught
    # by a Merkle path first.  The position is x mod 16: the oracle says which of the sixteen it is.
    lay, q = ctx_layout(proofs[offs[0]:offs[1]])
    r = offs[0] + lay.query_round_proofs + q.layer_evals[0]
    hits = [j for j in range(16) if oracle.verify_all(tables, ctls, bumped(proofs, r + 2 * j), chal, PUB) == 1030]
    assert len(hits) == 1
    rep = run("table 0 query 0 layer-0 evaluation at x", bumped(proofs, r + 2 * hits[0]), query=0, layer=0)
    assert rep.name == "FRI_EVAL"
    run("magic", bumped(proofs, offs[2]))
    run("claimed CTL challenge", proofs, claimed=bumped(chal, 1))
    run("public value added", proofs, pub=PUB + [7])
    # the trace-cap case without claimed challenges moves on to a per-table finding (the oracle's binding cannot pass a null there)
    rep = ctx.verify_segments([bumped(proofs, offs[0] + 16 + 12 + 5)], [PUB], None)[0]
    print("trace cap word, no claimed challenges:", rep.name, rep.table, rep.message)
    assert rep.code != 0 and rep.table == 0 and rep.name != "CTL_CHALLENGES"
    want = {("CTL_CHALLENGES", 0), ("QUOTIENT", 0), ("POW", 0), ("INITIAL_MERKLE", 0), ("INITIAL_MERKLE", 1), ("INITIAL_MERKLE", 2),
            ("FRI_EVAL", 0), ("FRI_MERKLE", 0), ("SHAPE", 0)}
    assert want <= seen, want - seen


# ---- 3. CTL_SUM: tables that are each well formed but inconsistent with each other
def test_ctl_sum_names_the_lookup(ctx, oracle, seg):
    raw, tables, ctls = seg
    n = 1 << tables[MEMORY][3]
    last = int(np.nonzero(tables[MEMORY][1][MEM_FILTER * n:(MEM_FILTER + 1) * n] == 1)[0][-1])
    no_filter = M.bump(tables, MEMORY, (MEM_FILTER << tables[MEMORY][3]) + last, 0)
    nl = 1 << tables[LOGIC][3]
    m = tables[LOGIC][1].reshape(-1, nl).copy()
    m[:, 0] = 0
    no_logic = list(tables)
    no_logic[LOGIC] = tables[LOGIC][:1] + (m.reshape(-1),) + tables[LOGIC][2:]
    for bad_tables, code, ctl in ((no_filter, 64, 14), (no_logic, 63, 13)):
        proofs, chal, offs = ctx.prove_with_traces(bad_tables, ctls, PUB)     # "check_ctls" is 0: a prover does not check
        assert oracle.verify_all(bad_tables, ctls, proofs, chal, PUB) == code
        rep = ctx.verify_segments([proofs], [PUB], [chal])[0]
        judged(rep, code)
        assert rep.name == "CTL_SUM" and rep.ctl == ctl
        assert ctx.verify_proofs(bad_tables, ctls, proofs, PUB, chal).key() == rep.key()


# ---- 4. hostile blobs do no harm
def test_hostile_blobs_are_refused_on_the_host(ctx, zkm, proven):
    proofs, chal, offs = proven
    lay, _ = ctx_layout(proofs[:offs[1]])
    cases = [("one word short", proofs[:-1])]
    for w in range(1, 12):
        for v in (0, 1 << 32, 1 << 63):
            if int(proofs[w]) != v:
                bad = proofs.copy()
                bad[w] = v
                cases.append(("header word %d = %d" % (w, v), bad))
    bad = proofs.copy()
    bad[lay.local_values + 3] = P
    cases.append(("a field word = p", bad))
    bad = proofs.copy()
    bad[offs[11] + lay.init_challenger_state] = P + 5
    cases.append(("a field word above p in the last blob", bad))
    cases.append(("zeros", np.zeros(proofs.size, dtype=np.uint64)))
    cases.append(("sixteen words", proofs[:16].copy()))
    cases.append(("three words", proofs[:3].copy()))
    before = ctx.memory()[0]
    ctx.profile(True)
    try:
        for name, blob in cases:
            ctx.profile_reset()
            rep = ctx.verify_segments([blob], [PUB], [chal])[0]
            launched = [k for k in ctx.profile_records() if k.startswith("verify/")]
            print("%-40s %s table %d  %s" % (name, rep.name, rep.table, rep.message))
            assert rep.name == "SHAPE" and rep.message and not launched, (name, rep.name, launched)
        # a refused blob beside a good one: the good one is verified, the refused one is not launched
        reps = ctx.verify_segments([cases[0][1], proofs], [PUB, PUB], [chal, chal])
        assert [r.name for r in reps] == ["SHAPE", "OK"]
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    rep, err = zkm.VerifyReport(), C.c_char_p()
    rc = ctx.L.zkm_verify_segments(ctx.h, C.byref(ctx.standard_config()), 1, None, None, None, None, None, C.byref(rep), C.byref(err))
    assert rc != 0 and b"null argument" in err.value and rep.code == zkm.VERIFY_FAILED      # reports are filled either way
    # blobs in device memory are refused (the transcript is replayed on the host), and so is a configuration the library does not support:
    # bad arguments are FAILED, not a property of the blob
    dev = ctx.alloc(proofs.size)
    dev.upload(proofs)
    rep, err = zkm.VerifyReport(), C.c_char_p()
    rc = ctx.L.zkm_verify_segments(ctx.h, C.byref(ctx.standard_config()), 1, (C.c_void_p * 1)(zkm._data_ptr(dev).value), (C.c_size_t * 1)(proofs.size),
                                   None, None, None, C.byref(rep), C.byref(err))
    dev.free()
    assert rc != 0 and b"host memory" in err.value and rep.code == zkm.VERIFY_FAILED
    cfg = ctx.standard_config()
    cfg.rate_bits = 3
    with pytest.raises(zkm.ZkmError, match="rate_bits"):
        ctx.verify_segments([proofs], [PUB], [chal], cfg=cfg)
    assert ctx.verify_segments([proofs], [PUB], [chal])[0].name == "OK"        # the context is as good as before
    assert ctx.memory()[0] == before


# ---- 5. K segments in one set of launches, one host wait
def test_launches_and_host_waits_do_not_depend_on_the_segments(ctx, proven):
    proofs, chal, offs = proven
    before = ctx.memory()[0]
    ctx.profile(True)
    try:
        def run(k):
            ctx.profile_reset()
            reps = ctx.verify_segments([proofs] * k, [PUB] * k, [chal] * k)
            ctx.synchronize()
            return reps, {name: v[0] for name, v in ctx.profile_records().items() if name.startswith("verify/")}
        reps1, rec1 = run(1)
        reps8, rec8 = run(8)
        again8, _ = run(8)
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    print(rec8)
    assert rec1 == rec8 and len(rec1) == 16 and all(v == 1 for v in rec1.values())    # rows, twelve tables, chains, queries, reduce
    assert {k for k in rec1 if k.startswith("verify/line_")} == {"verify/line_rows"} | {"verify/line_" + name for name in (
        "poseidon", "logic", "keccak_sponge", "keccak", "memory", "poseidon_sponge", "sha_extend", "sha_extend_sponge", "sha_compress",
        "sha_compress_sponge", "arithmetic", "cpu")}
    assert all(r.host_waits == 1 and r.name == "OK" for r in reps1 + reps8)
    assert [bytes(r) for r in reps8] == [bytes(r) for r in again8] == [bytes(reps1[0])] * 8
    assert ctx.memory()[0] == before


# ---- 6. "verify" in front of the hand-out
def test_verify_tuning_guards_every_prove_call(ctx, zkm, seg, proven):
    raw, tables, ctls = seg
    lg = [t[3] for t in tables]
    by_traces = ctx.prove_segment([t[1] for t in tables], lg, public_values=PUB)
    general = ctx.prove_with_traces(tables, ctls, PUB)
    cfg = ctx.standard_config()
    lay, _ = ctx_layout(proven[0][:proven[2][1]])
    os.environ["ZKM_ENABLE_TEST_HOOKS"] = "1"
    try:
        ctx.set_tuning("verify", 1)
        for want, got in ((proven, ctx.prove_segment_ops(SF.segment_ops(zkm, raw), public_values=PUB)),
                          (by_traces, ctx.prove_segment([t[1] for t in tables], lg, public_values=PUB)),
                          (general, ctx.prove_with_traces(tables, ctls, PUB))):
            for a, b in zip(want, got):
                assert np.array_equal(np.asarray(a), np.asarray(b))
        for got in ctx.prove_segments_ops([SF.segment_ops(zkm, raw)] * 3, public_values=[PUB] * 3):
            for a, b in zip(proven, got):
                assert np.array_equal(np.asarray(a), np.asarray(b))
        # one word of the second segment's blobs changes between proving and verifying
        ctx.set_tuning("debug_verify_flip", int(lay.quotient_polys_open))
        with pytest.raises(zkm.ZkmError, match=r"verify: segment 1: .*Arithmetic.*quotient"):
            ctx.prove_segments_ops([SF.segment_ops(zkm, raw)] * 3, public_values=[PUB] * 3)
        # ... and of a single segment: the call fails and no word is handed out
        st = SF.segment_ops(zkm, raw).struct()
        pub = np.array(PUB, dtype=np.uint64)
        out = np.zeros(proven[2][12], dtype=np.uint64)
        chal = np.zeros(2 * cfg.num_challenges, dtype=np.uint64)
        offs, err = (C.c_size_t * 13)(), C.c_char_p()
        rc = ctx.L.zkm_prove_segment_ops(ctx.h, C.byref(cfg), C.byref(st), pub.ctypes.data_as(zkm.u64p), 2, out.ctypes.data_as(zkm.u64p), offs,
                                         chal.ctypes.data_as(zkm.u64p), C.byref(err))
        assert rc != 0 and b"verify: segment 0" in err.value and b"Arithmetic" in err.value, err.value
        assert not out.any() and not chal.any()
        ctx.set_tuning("debug_verify_flip", 0)
        assert np.array_equal(ctx.prove_segment_ops(SF.segment_ops(zkm, raw), public_values=PUB)[0], proven[0])
    finally:
        ctx.set_tuning("debug_verify_flip", 0)
        ctx.set_tuning("verify", 0)
        os.environ.pop("ZKM_ENABLE_TEST_HOOKS", None)
    with pytest.raises(zkm.ZkmError, match="unknown key"):
        ctx.set_tuning("debug_verify_flip", 1)
