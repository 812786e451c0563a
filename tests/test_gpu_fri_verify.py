"""GPU suite: zkm_fri_verify (Context.fri_verify), plonky2's verify_fri_proof for any FriInstanceInfo on the device, judged by the Python
model tests/fri_verify_model.py (pinned to the CPU oracle by tests/test_fri_verify_model.py).

Proofs are made by Context.fri_prove on random polynomials with openings from eval_openings, six queries unless a case says otherwise:
this is also the first independent judge of zkm_fri_prove's general path.  Every accept case and every changed claim runs in both forms
of the Merkle kernel ("quad_max_hashes" 0: one lane a chain; above the call's chains: four lanes a chain).  A changed claim's report must
equal the model's (code, query, tree, layer); the model must reject every changed claim (a changed proof-of-work witness is accepted with
probability 2^-pow_bits: such a case would get another seed, it is not skipped -- the sweep was run with the seeds below and none was
accepted).  The changed claims of a shape travel in ONE call a form, which is also what the feature is for."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import fri_verify_model as M
from .test_abi import declared_alike

pytestmark = pytest.mark.gpu

P = M.P
FORMS = {"one_lane": 0, "quad": 1 << 30}


def config(ctx, **over):
    cfg = ctx.standard_config()
    cfg.num_queries = 6
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def params_of(cfg):
    return {k: int(getattr(cfg, k)) for k in ("rate_bits", "cap_height", "pow_bits", "num_queries", "arity_bits", "final_poly_bits")}


def copy_challenger(zkm, ch):
    return zkm.Challenger.from_buffer_copy(ch)


def challenger_key(ch):
    return (tuple(ch.state), tuple(ch.in_buf)[:ch.n_in], tuple(ch.out_buf)[:ch.n_out])


def model_challenger(ch):
    return M.Challenger(list(ch.state), list(ch.in_buf)[:ch.n_in], list(ch.out_buf)[:ch.n_out])


class Claim:
    """A claim as plain data (lists of Python integers), so that a case is a copy with a few words changed."""

    def __init__(self, cfg, log_n, cols, caps, batches, opened, blob, ch0, ch1=None):
        self.cfg, self.log_n, self.cols, self.caps, self.batches, self.opened, self.blob, self.ch0, self.ch1 = \
            cfg, log_n, cols, caps, batches, opened, blob, ch0, ch1

    def changed(self, **fields):
        c = Claim(self.cfg, self.log_n, self.cols, [list(x) for x in self.caps], list(self.batches), [list(x) for x in self.opened], list(self.blob),
                  self.ch0)
        for k, v in fields.items():
            setattr(c, k, v)
        return c

    def bump(self, what, *at):
        """a copy with one word increased by one (mod p): what = "blob", "caps", "opened", "point" or "challenger\""""
        c = self.changed()
        if what == "blob":
            c.blob[at[0]] = (c.blob[at[0]] + 1) % P
        elif what in ("caps", "opened"):
            getattr(c, what)[at[0]][at[1]] = (getattr(c, what)[at[0]][at[1]] + 1) % P
        elif what == "point":
            pt, polys = c.batches[at[0]]
            c.batches[at[0]] = (((pt[0] + 1) % P, pt[1]) if at[1] == 0 else (pt[0], (pt[1] + 1) % P), polys)
        else:
            c.ch0 = c.ch0.__class__.from_buffer_copy(c.ch0)
            c.ch0.state[at[0]] = (c.ch0.state[at[0]] + 1) % P
        return c

    def for_device(self, zkm):
        return zkm.FriClaim(np.array(self.blob, dtype=np.uint64), self.log_n, self.cols, self.caps, self.batches, self.opened,
                            copy_challenger(zkm, self.ch0))

    def judged(self):
        return M.verify(params_of(self.cfg), self.log_n, self.cols, self.caps, self.batches, self.opened, self.blob, model_challenger(self.ch0))


def prove(ctx, zkm, cfg, log_n, cols, batches, seed):
    """fri_prove on random polynomials -> the Claim, with the challenger before and after"""
    rng = np.random.default_rng(seed)
    oracles = [zkm.PolynomialBatch.from_values(ctx, rng.integers(0, P, k << log_n, dtype=np.uint64), k, log_n, cfg.rate_bits, cfg.cap_height)
               for k in cols]
    try:
        ch = zkm.challenger_new()
        zkm.challenger_observe(ch, [seed, 1, 2])
        ch0 = copy_challenger(zkm, ch)
        blob = ctx.fri_prove(oracles, batches, ch, cfg)
        values = {}
        opened = []
        for pt, polys in batches:
            for o in {o for o, _ in polys}:
                if (o, pt) not in values:
                    values[(o, pt)] = [int(x) for x in ctx.eval_openings(oracles[o], pt)]
            opened.append([w for o, p in polys for w in values[(o, pt)][2 * p:2 * p + 2]])
        caps = [[int(x) for x in b.cap()] for b in oracles]
    finally:
        for b in oracles:
            b.free()
    return Claim(cfg, log_n, list(cols), caps, list(batches), opened, [int(x) for x in blob], ch0, ch)


# ---------------------------------------------------------------- the shapes
def stark_shape(ctx):
    W, A, Q, Z = 13, 4, 4, 2
    zeta, g = (123456789, 987654321), M.root_of_unity(9)
    batches = [(zeta, [(0, c) for c in range(W)] + [(1, c) for c in range(A)] + [(2, c) for c in range(Q)]),
               ((zeta[0] * g % P, zeta[1] * g % P), [(0, c) for c in range(W)] + [(1, c) for c in range(A)]), ((1, 0), [(1, c) for c in range(A - Z, A)])]
    return config(ctx), 9, [W, A, Q], batches


def plonk_shape(ctx, log_n):
    """four oracles (constants and sigmas, wires, Z and partial products, quotient), one batch at zeta over all of them and one at
    g zeta over part of one; standard_recursion_config: rate_bits 3, cap_height 4, arity_bits 4, final_poly_bits 5"""
    cols = [7, 9, 5, 4]
    zeta, g = (24680 + log_n, 13579), M.root_of_unity(log_n)
    batches = [(zeta, [(o, c) for o in range(4) for c in range(cols[o])]), ((zeta[0] * g % P, zeta[1] * g % P), [(2, c) for c in range(2)])]
    return config(ctx, rate_bits=3, cap_height=4, arity_bits=4, final_poly_bits=5), log_n, cols, batches


def wide_shape(ctx):
    """8 oracles x 8 batches: leaves of 1, 4 (their own digest), 5, 9 (ragged absorb), 8, 16 (whole absorbs), 3, 2 columns; polynomial (4, 0) in
    three batches; a batch of one polynomial; lists not in oracle order; points in the base field and in the extension"""
    cols = [1, 4, 5, 8, 9, 3, 16, 2]
    batches = [((5, 6), [(4, 0), (0, 0), (6, 15), (1, 3)]), ((77, 0), [(7, 1), (4, 0), (2, 4)]), ((9, 1), [(3, 7)]),
               ((3, 0), [(6, c) for c in range(15, -1, -1)]), ((11, 12), [(5, 2), (4, 8), (4, 0), (5, 0)]), ((1, 0), [(1, 0), (1, 1), (0, 0)]),
               ((P - 1, P - 2), [(2, 0), (3, 0), (7, 0)]), ((0, 0), [(4, 3), (6, 1)])]
    return config(ctx), 8, cols, batches


SHAPES = {"stark": stark_shape, "plonk7": lambda ctx: plonk_shape(ctx, 7), "plonk12": lambda ctx: plonk_shape(ctx, 12), "wide": wide_shape}
_PROVEN = {}


def proven(ctx, zkm, name):
    """the shape's proof, made once a module run"""
    if name not in _PROVEN:
        cfg, log_n, cols, batches = SHAPES[name](ctx)
        _PROVEN[name] = prove(ctx, zkm, cfg, log_n, cols, batches, 7000 + list(SHAPES).index(name))
    return _PROVEN[name]


@pytest.fixture(params=list(FORMS))
def form_ctx(request, zkm):
    """a context that takes the named form of the Merkle kernel whatever the call's chains"""
    c = zkm.Context(0)
    c.set_tuning("quad_max_hashes", FORMS[request.param])
    yield c
    c.close()


def verify(c, zkm, claims):
    """(reports, device claims): the reports of one call on the claims (all of one configuration)"""
    dev = [cl.for_device(zkm) for cl in claims]
    return c.fri_verify(dev, claims[0].cfg), dev


def key(rep):
    return (rep.code, rep.query, rep.tree, rep.layer)


def accepted(c, zkm, claim):
    (rep,), (dev,) = verify(c, zkm, [claim])
    assert key(rep) == (M.OK, 0, 0, 0) and rep.table == 0 and rep.host_waits == 1, (rep.name, rep.message)
    assert claim.judged() == (M.OK, 0, 0, 0)
    assert challenger_key(dev.challenger) == challenger_key(claim.ch1)       # advanced to where fri_prove left its own


# ---------------------------------------------------------------- accepted
def test_declared_alike(zkm):
    declared_alike(zkm, "zkm_fri_verify")


@pytest.mark.parametrize("name", list(SHAPES))
def test_accepts_what_fri_prove_proves(ctx, form_ctx, zkm, name):
    """(a) the STARK shape at 2^9, (b) the PLONK shape at 2^7 and 2^12, (c) 8 oracles x 8 batches at 2^8"""
    accepted(form_ctx, zkm, proven(ctx, zkm, name))


def test_accepts_a_proof_without_layers(ctx, form_ctx, zkm):
    """(d) log_n <= final_poly_bits: the final polynomial is the whole proof, a query has noracles + 1 verdicts"""
    cfg, _, cols, batches = wide_shape(ctx)
    claim = prove(ctx, zkm, cfg, 5, cols, batches, 7100)
    assert M.num_layers(params_of(cfg), 5) == 0
    accepted(form_ctx, zkm, claim)


@pytest.mark.parametrize("arity_bits", [2, 3, 4, 5, 6])
def test_accepts_every_arity(ctx, form_ctx, zkm, arity_bits):
    """(e) two layers of each arity at the smallest height that gives them (final_poly_bits 2)"""
    cfg = config(ctx, arity_bits=arity_bits, final_poly_bits=2)
    log_n = next(n for n in range(1, 20) if M.num_layers(params_of(cfg), n) == 2)
    claim = prove(ctx, zkm, cfg, log_n, [3, 6], [((5, 9), [(1, 5), (0, 1)]), ((8, 0), [(0, 0), (1, 0), (1, 1)])], 7200 + arity_bits)
    accepted(form_ctx, zkm, claim)


def test_accepts_queries_across_a_wave(ctx, form_ctx, zkm):
    """(f) 70 queries: the query kernel's second workgroup, the chains' second and later waves"""
    cfg = config(ctx, num_queries=70)
    claim = prove(ctx, zkm, cfg, 7, [5, 2], [((5, 9), [(1, 1), (0, 4)]), ((8, 3), [(0, 0)])], 7300)
    accepted(form_ctx, zkm, claim)
    (rep,), _ = verify(form_ctx, zkm, [claim.bump("blob", len(claim.blob) - 1)])      # the last query's last sibling
    assert key(rep) == claim.bump("blob", len(claim.blob) - 1).judged() and rep.query == 69 and rep.name == "FRI_MERKLE"


def test_accepts_a_tree_that_is_its_cap(ctx, form_ctx, zkm):
    """(g) lde_bits == cap_height, which zkm_fri_prove admits (2^3 rows, a cap of 2^5 digests): every path has zero siblings, the leaf's
    digest -- of one word: the word itself; of six: a ragged absorb -- is compared with its cap entry.  No layer fits above such a cap."""
    cfg = config(ctx, cap_height=5)
    claim = prove(ctx, zkm, cfg, 3, [1, 6], [((5, 9), [(1, 5), (0, 0)]), ((8, 0), [(1, 0)])], 7400)
    o = M.offsets(params_of(cfg), 3, [1, 6])
    assert o["L"] == 0 and o["round"] == 7
    accepted(form_ctx, zkm, claim)
    bad = [claim.bump("blob", o["queries"] + 2 * o["round"]), claim.bump("blob", o["queries"] + 4 * o["round"] + 3)]
    reports, _ = verify(form_ctx, zkm, bad)
    assert [key(r) for r in reports] == [c.judged() for c in bad] == [(M.INITIAL_MERKLE, 2, 0, 0), (M.INITIAL_MERKLE, 4, 1, 0)]


# ---------------------------------------------------------------- verdict for verdict
def cases_of(claim):
    """[(name, changed claim)]: one word of each kind of field, at the first, a middle and the last query, on every oracle and every
    layer; the caps at an entry a query reaches; every batch's opened values and point; the challenger"""
    params = params_of(claim.cfg)
    o = M.offsets(params, claim.log_n, claim.cols)
    _, _, _, indices = M.fri_challenges(params, claim.log_n, M.parse(params, claim.log_n, claim.cols, claim.blob), model_challenger(claim.ch0))
    nq, ab, out = params["num_queries"], params["arity_bits"], []
    nsib = o["lde_bits"] - params["cap_height"]
    for q in sorted({0, nq // 2, nq - 1}):
        base = o["queries"] + q * o["round"]
        for k, (evals, sibs) in enumerate(o["oracle"]):
            out.append(("query %d oracle %d row" % (q, k), claim.bump("blob", base + evals + (q + k) % claim.cols[k])))
            if nsib:
                out.append(("query %d oracle %d sibling" % (q, k), claim.bump("blob", base + sibs + (3 * q + k) % (4 * nsib))))
        for l, (evals, sibs, count) in enumerate(o["layer"]):
            within = (indices[q] >> (ab * l)) & ((1 << ab) - 1)
            out.append(("query %d layer %d queried value" % (q, l), claim.bump("blob", base + evals + 2 * within + q % 2)))
            out.append(("query %d layer %d other value" % (q, l), claim.bump("blob", base + evals + 2 * (within ^ (1 + q)) + 1)))
            if count:
                out.append(("query %d layer %d sibling" % (q, l), claim.bump("blob", base + sibs + (q + l) % (4 * count))))
    entry = indices[nq - 1] >> nsib
    for l, cap in enumerate(o["caps"]):
        out.append(("layer %d cap" % l, claim.bump("blob", cap + 4 * entry + l % 4)))
    out.append(("final polynomial", claim.bump("blob", o["final"] + 1)))
    out.append(("pow witness", claim.bump("blob", o["pow"])))
    for k in range(len(claim.cols)):
        out.append(("oracle %d cap" % k, claim.bump("caps", k, 4 * entry + k % 4)))
    for b in range(len(claim.batches)):
        out.append(("batch %d opened value" % b, claim.bump("opened", b, len(claim.opened[b]) - 1 - b % 2)))
        # (a base-field point stays in the base field: moved into the extension it could not be refused as lying on the coset)
        out.append(("batch %d point" % b, claim.bump("point", b, b % 2 if claim.batches[b][0][1] else 0)))
    out.append(("challenger", claim.bump("challenger", 3)))
    return out


@functools.lru_cache(maxsize=None)
def judged_cases(name):
    return [(what, cl, cl.judged()) for what, cl in cases_of(_PROVEN[name])]


@pytest.mark.parametrize("name", ["stark", "plonk7", "wide"])
def test_every_changed_field_gets_the_models_verdict(ctx, form_ctx, zkm, name):
    proven(ctx, zkm, name)
    cases = judged_cases(name)
    assert len(cases) > 30
    for what, _, want in cases:
        assert want[0] != M.OK, (what, "the model accepts: take another seed")
    reports, _ = verify(form_ctx, zkm, [cl for _, cl, _ in cases])
    assert [key(r) for r in reports] == [want for _, _, want in cases], \
        [(what, r.name, key(r), want) for (what, _, want), r in zip(cases, reports) if key(r) != want]
    assert all(r.host_waits == 1 and r.table == 0 for r in reports)
    first = next(r for r in reports if r.code)
    assert first.message.startswith("zkm_fri_verify: proof 0: ") and first.message.endswith("[%s]" % first.name)
    # every kind of finding the query phase has was met
    assert {r.name for r in reports} >= {"POW", "INITIAL_MERKLE", "FRI_EVAL", "FRI_MERKLE"}


def test_the_first_of_several_findings_is_reported(ctx, form_ctx, zkm):
    """Several changes in one blob: the report is the first in plonky2's order -- lowest query; inside it the oracles in order, per layer
    the evaluation before the path, then the final polynomial"""
    claim = proven(ctx, zkm, "wide")
    params = params_of(claim.cfg)
    o = M.offsets(params, claim.log_n, claim.cols)
    _, _, _, indices = M.fri_challenges(params, claim.log_n, M.parse(params, claim.log_n, claim.cols, claim.blob), model_challenger(claim.ch0))
    rnd = lambda q: o["queries"] + q * o["round"]
    within = lambda q: indices[q] & ((1 << params["arity_bits"]) - 1)
    lay = o["layer"][0]

    def many(*at):
        c = claim.changed()
        for i in at:
            c.blob[i] = (c.blob[i] + 1) % P
        return c
    cases = [
        # query 3: oracle 5 and oracle 2; query 1: layer 0's path -> query 1 wins
        (many(rnd(3) + o["oracle"][5][0], rnd(3) + o["oracle"][2][0], rnd(1) + lay[1]), (M.FRI_MERKLE, 1, 0, 0)),
        # one query: oracle 6's sibling, oracle 2's row, layer 0's queried value -> the lower oracle
        (many(rnd(4) + o["oracle"][6][1], rnd(4) + o["oracle"][2][0], rnd(4) + lay[0] + 2 * within(4)), (M.INITIAL_MERKLE, 4, 2, 0)),
        # one layer: the queried value (evaluation check and path) -> the evaluation check
        (many(rnd(2) + lay[0] + 2 * within(2), rnd(2) + lay[1] + 3), (M.FRI_EVAL, 2, 0, 0)),
        # the queried value of query 5 and a row of query 5's oracle 7 with the last query's path -> query 5's oracle
        (many(rnd(5) + lay[0] + 2 * within(5), rnd(5) + o["oracle"][7][0]), (M.INITIAL_MERKLE, 5, 7, 0)),
    ]
    reports, _ = verify(form_ctx, zkm, [c for c, _ in cases])
    for (c, want), rep in zip(cases, reports):
        assert key(rep) == want == c.judged(), (rep.name, key(rep), want)


# ---------------------------------------------------------------- one call, many claims
@pytest.mark.parametrize("nclaims", [1, 5, 33])
def test_many_claims_share_a_call(ctx, form_ctx, zkm, nclaims):
    """Claims of mixed shapes and heights in one call, some changed, one refused on the host: every report equals the single-claim
    call's, one host wait for the launched claims and none for the refused one, and the challengers move only where accepted."""
    good = [proven(ctx, zkm, n) for n in ("wide", "stark")]         # (one configuration a call: these two share the standard one)
    pool = []
    for claim in good:
        pool += [claim] + [cl for _, cl in cases_of(claim)[::7]]
    short = good[0].changed()
    short.blob = short.blob[:-1]                                      # proof_words below the blob's size: SHAPE on the host
    claims = [pool[(5 * i) % len(pool)] for i in range(nclaims)]
    if nclaims > 1:
        claims[nclaims // 2] = short
    waits = form_ctx.host_waits()
    reports, dev = verify(form_ctx, zkm, claims)
    assert form_ctx.host_waits() - waits == 1
    singles = {}
    for cl, rep, d in zip(claims, reports, dev):
        if id(cl) not in singles:
            (one,), _ = verify(form_ctx, zkm, [cl])
            singles[id(cl)] = one.key()
        assert rep.key() == singles[id(cl)], (rep.name, rep.key(), singles[id(cl)])
        if cl is short:
            assert rep.name == "SHAPE" and rep.host_waits == 0
        else:
            assert rep.host_waits == 1
        assert challenger_key(d.challenger) == challenger_key(cl.ch1 if rep.code == 0 else cl.ch0)
    assert nclaims == 1 or {r.code for r in reports} >= {0, 1}
    assert any(r.code > 1 for r in reports) or nclaims == 1


# ---------------------------------------------------------------- host findings
def test_host_findings_carry_their_messages_and_leave_the_context_usable(ctx, zkm):
    claim = proven(ctx, zkm, "stark")
    accepted(ctx, zkm, claim)                                         # (the tables this shape keeps resident exist from here on)
    resident = ctx.resident_bytes()
    o = M.offsets(params_of(claim.cfg), claim.log_n, claim.cols)

    def blob_with(i, v):
        c = claim.changed()
        c.blob[i] = v
        return c

    def point_at(b, pt):
        c = claim.changed()
        c.batches[b] = (pt, c.batches[b][1])
        return c
    short = claim.changed()
    short.blob = short.blob[:-1]
    stub = claim.changed()
    stub.blob = stub.blob[:10]
    shape = [(blob_with(0, claim.blob[0] ^ 1), "magic"), (short, "proof_words too short"), (stub, "proof_words too short for the header"),
             (claim.changed(log_n=claim.log_n + 1), "header word 1 "), (claim.changed(cols=[13, 4, 5]), "header word 18 "),
             (claim.changed(cols=[13, 4], caps=claim.caps[:2], batches=[(pt, [(o_, p) for o_, p in polys if o_ < 2]) for pt, polys in claim.batches],
                            opened=[x[:2 * sum(1 for o_, _ in polys if o_ < 2)] for x, (_, polys) in zip(claim.opened, claim.batches)]), "header word 2 "),
             (blob_with(8, 3), "header word 8 "), (blob_with(o["pow"], P), "word %d is not a canonical" % o["pow"]),
             (blob_with(len(claim.blob) - 1, (1 << 64) - 1), "word %d is not a canonical" % (len(claim.blob) - 1))]
    bad_open = claim.changed()
    bad_open.opened[1][2] = P
    bad_cap = claim.changed()
    bad_cap.caps[2][5] = P + 5
    shape += [(bad_open, "opened values of batch 1"), (bad_cap, "cap of oracle 2"), (point_at(0, (P, 3)), "point of batch 0")]
    for c, text in shape:
        (rep,), (dev,) = verify(ctx, zkm, [c])
        assert rep.name == "SHAPE" and rep.host_waits == 0 and text in rep.message and rep.message.endswith("[SHAPE]"), (text, rep.name, rep.message)
        assert challenger_key(dev.challenger) == challenger_key(claim.ch0)
    other_cfg = config(ctx, num_queries=7)
    (rep,), _ = verify(ctx, zkm, [claim.changed(cfg=other_cfg)])
    assert rep.name == "SHAPE" and "header word 6 " in rep.message

    g = M.MULTIPLICATIVE_GROUP_GENERATOR
    on_coset = g * pow(M.root_of_unity(claim.log_n + 2), 5, P) % P
    nine = [claim.batches[0]] * 9
    failed = [(claim.changed(batches=[(claim.batches[0][0], [(3, 0)])], opened=[[1, 2]]), "polynomial index out of range"),
              (claim.changed(batches=[(claim.batches[0][0], [(1, 4)])], opened=[[1, 2]]), "polynomial index out of range"),
              (claim.changed(batches=nine, opened=[claim.opened[0]] * 9), "1..8 opening batches"),
              (claim.changed(cols=[1] * 9, caps=[claim.caps[0]] * 9), "1..8 oracles"),
              (point_at(2, (on_coset, 0)), "lies on the LDE coset"),
              (claim.changed(cfg=config(ctx, arity_bits=7)), "arity_bits"), (claim.changed(cfg=config(ctx, rate_bits=5)), "rate_bits")]
    for c, text in failed:
        with pytest.raises(zkm.ZkmError, match=text) as e:      # (the good claim first: the refusal of a later claim fails the call)
            ctx.fri_verify([claim.for_device(zkm), c.for_device(zkm)], c.cfg)
        assert [r.name for r in e.value.reports] == ["FAILED", "FAILED"]
    with pytest.raises(zkm.ZkmError, match="nothing to verify|null argument"):
        ctx.fri_verify([], claim.cfg)
    # an empty batch, a NULL pointer and a device pointer, through the C entry point
    L, dev = zkm.load(), claim.for_device(zkm)
    empty = claim.changed(batches=[claim.batches[0], (claim.batches[1][0], [])], opened=claim.opened[:2])
    with pytest.raises(zkm.ZkmError, match="empty batch"):
        verify(ctx, zkm, [empty])
    buf = ctx.alloc(len(claim.blob)).upload(np.array(claim.blob, dtype=np.uint64))
    try:
        for proof_ptr, text in ((None, "null argument"), (buf.ptr, "host memory")):
            cfg = claim.cfg
            keep = [np.array(x, dtype=np.uint64) for x in claim.caps + claim.opened]
            caps = (C.c_void_p * 3)(*[k.ctypes.data for k in keep[:3]])
            opened = (C.c_void_p * 3)(*[k.ctypes.data for k in keep[3:]])
            polys = [np.array(p, dtype=np.uint32).reshape(-1, 2) for _, p in claim.batches]
            barr = (zkm.FriBatch * 3)(*[zkm.FriBatch((C.c_uint64 * 2)(*pt), a.ctypes.data, len(a)) for (pt, _), a in zip(claim.batches, polys)])
            one = lambda ty, v: (ty * 1)(v)
            cols = (C.c_size_t * 3)(*claim.cols)
            rep, err = zkm.VerifyReport(), C.c_char_p()
            rc = L.zkm_fri_verify(ctx.h, C.byref(cfg), 1, one(C.c_void_p, proof_ptr), one(C.c_size_t, len(claim.blob)), one(C.c_uint, claim.log_n),
                                  one(C.c_void_p, C.addressof(cols)), one(C.c_size_t, 3), one(C.c_void_p, C.addressof(caps)),
                                  one(C.c_void_p, C.addressof(barr)), one(C.c_size_t, 3), one(C.c_void_p, C.addressof(opened)),
                                  one(C.c_void_p, C.addressof(dev.challenger)), C.byref(rep), C.byref(err))
            assert rc != 0 and rep.name == "FAILED" and text in err.value.decode(), (text, err.value)
    finally:
        buf.free()
    assert ctx.resident_bytes() == resident
    accepted(ctx, zkm, claim)
