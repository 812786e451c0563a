"""GPU suite: the rejections of zkm_verify_segments swept over every table, query, FRI layer and Merkle chain, in both forms of the
chain kernel (k_verify_chains_quad up to "quad_max_hashes" chains a call, k_verify_chains -- one chain per lane -- beyond), and with more
than one finding in a blob.  tests/test_gpu_verify.py holds the accept cases, the hostile blobs and the launch accounting; its helpers
(expected, judged, bumped, ctx_layout, tamper_cases) are used here.

Every changed blob stays well formed (every word below p, the header untouched): it reaches the device.  The judge is the oracle's
sequential verifier (oracle.verify_all, plain C that shares nothing with verify.hip): `judged` translates its return code into the report's
check, table and tree.  `query` and `layer` come from where the test changed the blob, and so does the whole expected report of the cases
the oracle is not asked about; the oracle confirms that rule on at least one case per (table, chain) and (table, layer), at each table's
lowest and highest query, and on every case whose report does not follow from the position alone.

What the position does not say is which of a layer's sixteen evaluations is the queried one: a change to that one is FRI_EVAL, to any
other FRI_MERKLE.  `Segment.query_indices` therefore replays one table's transcript from the challenger state its blob records
(proof_blob.h "the transcript, step by step"; plonky2 get_challenges) on the ORACLE's challenger; the replay is held to the proof of
work of the untouched blob (the response to the recorded witness has its pow_bits leading zeros), and the oracle judges every case
predicted FRI_EVAL that way.

The oracle's cost, measured on an x86 host with 8 oracle threads and no GPU (median of 5 calls after one warm call): verify_all takes 0.24 s on
the fixture segment and 0.29 s on the repeat=128 segment when it accepts.  A rejection returns at the failing table: 0.02 s at table 0
(Arithmetic), 0.05 s at table 2, 0.13 s at table 4 (Keccak, 2431 columns), 0.21 s at table 11 (Memory).  Each blob is judged once per
module run (`Segment.code` keeps the codes), so the second form of a parametrised test costs no oracle time.  The oracle's share of one
test stays under about 3 s at those figures: section 1 asks for every case of tamper_cases on every table (22 or 23 cases a table, up to
4.8 s at table 11) and is therefore split per table and into the proof's fields / the query rounds (at most 14 cases, 2.9 s); section 2 per
table judges the minimum the rule needs (at most 7 cases, 1.5 s); section 3 per table at most 3; sections 4 and 5 ten to seventeen
(1.6 s at most).  The whole module: 96 tests in 60 s on an MI355X machine, the slowest 1.9 s.

The final polynomial: a changed coefficient is named POW, not FINAL_POLY, by the sequential verifier and by the device alike.  The
coefficients are observed before the proof-of-work witness (plonky2 fri_challenges: observe_extension_elements(&final_poly.coeffs), then
the witness, then the query indices; get_challenges.rs:225, verifier.rs:27-176 draws the challenges before any check), so the response
to the recorded witness changes and keeps its sixteen leading zeros with probability 2^-16; a witness found again would move every
query index off the paths the blob holds.  FINAL_POLY cannot be reached by changing a blob; those cases are judged by the oracle like
every other, and the report must say what it says."""
import numpy as np
import pytest

from . import segment_ops_fixtures as SF
from .test_gpu_verify import PUB, bumped, ctx_layout, expected, judged, tamper_cases

pytestmark = pytest.mark.gpu

P = SF.P
FORMS = ("quad", "one_lane")
MEMORY = 11
QUAD_MAX_DEFAULT, QUAD_MAX_THROUGHPUT = 32768, 4096          # zkm_ctx::quad_max_hashes, and under "throughput_profile"
PER_CALL = 16


class Case:
    """One changed blob: `edits` = ((word index, new value), ...); what the report must say (None: not fixed by the position; `names`
    lists the checks the position allows); judge: the oracle is asked."""

    def __init__(self, name, edits, names=None, table=None, query=None, tree=None, layer=None, judge=False):
        self.name, self.edits, self.judge = name, tuple(edits), judge
        self.names = (names,) if isinstance(names, str) else names
        self.table, self.query, self.tree, self.layer = table, query, tree, layer

    def check(self, rep):
        where = "%s: %s table %d query %d tree %d layer %d" % (self.name, rep.name, rep.table, rep.query, rep.tree, rep.layer)
        assert rep.code != 0, where
        assert self.names is None or rep.name in self.names, (where, self.names)
        assert self.table is None or rep.table == self.table, where
        if rep.name in ("INITIAL_MERKLE", "FRI_EVAL", "FRI_MERKLE", "FINAL_POLY"):
            assert self.query is None or rep.query == self.query, where
        if rep.name == "INITIAL_MERKLE":
            assert self.tree is None or rep.tree == self.tree, where
        if rep.name in ("FRI_EVAL", "FRI_MERKLE"):
            assert self.layer is None or rep.layer == self.layer, where


class Segment:
    """A proven segment: what the oracle needs to judge its blobs, the layout of each of the twelve, and the oracle's codes so far."""

    def __init__(self, oracle, tables, ctls, proofs, chal, offs):
        self.oracle, self.tables, self.ctls = oracle, tables, ctls
        self.proofs, self.chal, self.offs = np.ascontiguousarray(proofs, dtype=np.uint64), chal, [int(o) for o in offs]
        self.lay = [ctx_layout(self.proofs[self.offs[t]:self.offs[t + 1]]) for t in range(12)]
        for lay, q in self.lay:       # a chain's siblings follow its leaf (chain_setup relies on it)
            assert all(q.oracle_siblings[c] == q.oracle_evals[c] + q.oracle_cols[c] for c in range(3))
            assert all(q.layer_siblings[l] == q.layer_evals[l] + (2 << lay.arity_bits) for l in range(lay.fri_layers))
        self.codes, self.xs = {}, {}

    def L(self, t):
        return int(self.lay[t][0].fri_layers)

    def chains(self):
        """Merkle chains of the segment: what the host compares with quad_max_hashes (verify.hip `nchains`)."""
        return sum(int(lay.num_queries) * (3 + int(lay.fri_layers)) for lay, _ in self.lay)

    def blob(self, edits):
        out = self.proofs.copy()
        for i, v in edits:
            assert 0 <= v < P and int(out[i]) != v
            out[i] = v
        return out

    def code(self, edits):
        """The sequential verifier's code for the blob with `edits` (asked once)."""
        edits = tuple(edits)
        if edits not in self.codes:
            self.codes[edits] = self.oracle.verify_all(self.tables, self.ctls, self.blob(edits), self.chal, PUB)
        return self.codes[edits]

    def plus1(self, *idx):
        return tuple((int(i), (int(self.proofs[i]) + 1) % P) for i in idx)

    def put(self, at, words):
        """Edits that write `words` from word `at` on (the words that change only)."""
        return tuple((int(at) + j, int(w)) for j, w in enumerate(words) if int(self.proofs[int(at) + j]) != int(w))

    def field(self, t, name):
        return self.offs[t] + int(getattr(self.lay[t][0], name))

    def query(self, t, k):
        lay, _ = self.lay[t]
        return self.offs[t] + int(lay.query_round_proofs) + k * int(lay.query_round_words)

    def chain(self, t, k, c):
        """(first leaf word, leaf words, first sibling word, sibling digests) of chain c of query k: c = 0..2 the trace, auxiliary and
        quotient tree, 3 + l the tree of FRI layer l."""
        lay, q = self.lay[t]
        r = self.query(t, k)
        if c < 3:
            return r + int(q.oracle_evals[c]), int(q.oracle_cols[c]), r + int(q.oracle_siblings[c]), int(q.initial_siblings)
        return r + int(q.layer_evals[c - 3]), 2 << int(lay.arity_bits), r + int(q.layer_siblings[c - 3]), int(q.layer_siblings_count[c - 3])

    def layer_pairs(self, t, k, l):
        """The words of the sixteen evaluation pairs of layer l in query k."""
        at, n, _, _ = self.chain(t, k, 3 + l)
        return range(at, at + n)

    def query_indices(self, t):
        """Table t's query indices x (before any fold), from its blob alone: see the module docstring."""
        if t not in self.xs:
            lay, _ = self.lay[t]
            o, b = self.oracle, self.proofs[self.offs[t]:self.offs[t + 1]]
            cap = 4 << int(lay.cap_height)
            W, A, Q, Z = (int(v) for v in (lay.trace_cols, lay.aux_cols, lay.quotient_polys, lay.ctl_zs))
            ch = o.challenger()
            ch.state[:] = [int(v) for v in b[lay.init_challenger_state:lay.init_challenger_state + 12]]
            o.observe(ch, b[lay.aux_cap:lay.aux_cap + cap])
            for _ in range(2):                                     # alphas (num_challenges = 2)
                o.challenge(ch)
            o.observe(ch, b[lay.quotient_cap:lay.quotient_cap + cap])
            for _ in range(2):                                     # zeta
                o.challenge(ch)
            for at, n in ((lay.local_values, 2 * W), (lay.aux_polys, 2 * A), (lay.quotient_polys_open, 2 * Q), (lay.next_values, 2 * W),
                          (lay.aux_polys_next, 2 * A)):
                o.observe(ch, b[at:at + n])
            for i in range(Z):
                o.observe(ch, [int(b[lay.ctl_zs_first + i]), 0])
            for _ in range(2):                                     # fri_alpha
                o.challenge(ch)
            for l in range(int(lay.fri_layers)):
                o.observe(ch, b[lay.commit_phase_merkle_caps + l * cap:lay.commit_phase_merkle_caps + (l + 1) * cap])
                for _ in range(2):                                 # beta of layer l
                    o.challenge(ch)
            o.observe(ch, b[lay.final_poly:lay.final_poly + 2 * int(lay.final_poly_len)])
            o.observe(ch, b[lay.pow_witness:lay.pow_witness + 1])
            assert o.challenge(ch) >> (64 - o.standard_config().pow_bits) == 0, "the replay does not reproduce table %d's proof of work" % t
            bits = int(lay.degree_bits) + int(lay.rate_bits)
            self.xs[t] = [o.challenge(ch) % (1 << bits) for _ in range(int(lay.num_queries))]
        return self.xs[t]

    def within(self, t, k, l):
        """Which of layer l's sixteen pairs query k asks for."""
        a = int(self.lay[t][0].arity_bits)
        return (self.query_indices(t)[k] >> (a * l)) & ((1 << a) - 1)


def prove(oracle, ctx, zkm, repeat):
    raw, tables, ctls = SF.build_segment_ops(oracle, repeat=repeat)
    proofs, chal, offs = ctx.prove_segment_ops(SF.segment_ops(zkm, raw), public_values=PUB)
    return Segment(oracle, tables, ctls, proofs, chal, offs)


@pytest.fixture(scope="module")
def small(oracle, ctx, zkm):
    return prove(oracle, ctx, zkm, 1)


@pytest.fixture(scope="module")
def large(oracle, ctx, zkm):
    S = prove(oracle, ctx, zkm, 128)
    assert max(S.L(t) for t in range(12)) == 3
    return S


@pytest.fixture(scope="module")
def lanes(ctx, zkm):
    """form -> context.  The shared context keeps its default threshold (a call of one segment, about 2,000 chains, takes the quad
    form); the one-lane form gets a context of this module's own with "quad_max_hashes" at 0."""
    own = zkm.Context(0)
    try:
        own.set_tuning("quad_max_hashes", 0)
        yield {"quad": ctx, "one_lane": own}
    finally:
        own.close()


def verify_each(c, S, blobs):
    """One report per blob, PER_CALL blobs to a call."""
    reps = []
    for i in range(0, len(blobs), PER_CALL):
        part = blobs[i:i + PER_CALL]
        reps += c.verify_segments(part, [PUB] * len(part), [S.chal] * len(part))
    assert len(reps) == len(blobs)
    return reps


def sweep(c, S, cases):
    """Verify the cases' blobs PER_CALL to a call and hold every report to its case.  A judged case is verified in a call of its own as
    well (the message belongs to a call's first rejection): the two reports are the same bytes, and `judged` compares with the oracle."""
    reps = verify_each(c, S, [S.blob(case.edits) for case in cases])
    for case, rep in zip(cases, reps):
        case.check(rep)
        if case.judge:
            own, = c.verify_segments([S.blob(case.edits)], [PUB], [S.chal])
            assert bytes(own) == bytes(rep), case.name
            code = S.code(case.edits)
            print("%-56s" % case.name, end=" ")
            assert code != 0, "%s: the oracle accepts this blob" % case.name
            judged(own, code)
    return reps


# ---- 1. both chain forms, accept and reject
@pytest.mark.parametrize("form", FORMS)
def test_each_form_accepts_valid_segments(lanes, small, large, form):
    other = lanes[FORMS[1 - FORMS.index(form)]]
    blobs, chals = [small.proofs, large.proofs, small.proofs, small.proofs], [small.chal, large.chal, small.chal, None]
    reps = lanes[form].verify_segments(blobs, [PUB] * 4, chals)
    for rep in reps:
        judged(rep, 0)
        assert rep.host_waits == 1
    assert [bytes(r) for r in reps] == [bytes(r) for r in other.verify_segments(blobs, [PUB] * 4, chals)]


@pytest.mark.parametrize("part", ("proof", "queries"))
@pytest.mark.parametrize("t", range(12))
@pytest.mark.parametrize("form", FORMS)
def test_each_form_rejects_what_the_oracle_rejects_on_every_table(lanes, small, form, t, part):
    """tests/test_gpu_verify.py's tamper_cases on each of the twelve tables: the fields of the proof (query None), or the query rounds."""
    other = lanes[FORMS[1 - FORMS.index(form)]]
    cases = [c for c in tamper_cases(small.proofs, small.offs, t) if (c[2] is None) == (part == "proof")]
    assert len(cases) >= 8
    for name, i, query, layer in cases:
        bad = bumped(small.proofs, i)
        rep, = lanes[form].verify_segments([bad], [PUB], [small.chal])
        assert bytes(rep) == bytes(other.verify_segments([bad], [PUB], [small.chal])[0])
        code = small.code(small.plus1(i))
        print("table %2d %-34s" % (t, name), end=" ")
        assert code != 0
        pair = judged(rep, code)
        assert rep.table == t or pair[0] == "CTL_CHALLENGES"
        if pair[0] in ("INITIAL_MERKLE", "FRI_EVAL", "FRI_MERKLE") and query is not None:
            assert rep.query == query
            if pair[0] != "INITIAL_MERKLE" and layer is not None:
                assert rep.layer == layer


def a_memory_trace_sibling(S, k):
    _, _, sib, nsib = S.chain(MEMORY, k, 0)
    return Case("Memory query %d trace sibling" % k, S.plus1(sib + 4 * (nsib // 2) + 1), "INITIAL_MERKLE", MEMORY, k, tree=0, judge=True)


def test_many_segments_in_one_call_take_the_one_lane_form(ctx, small):
    """No tuning key: K segments whose chains together pass the default threshold."""
    per = small.chains()
    K = QUAD_MAX_DEFAULT // per + 1
    assert K * per > QUAD_MAX_DEFAULT >= (K - 1) * per and per == sum(37 * (3 + small.L(t)) for t in range(12))
    _, n, sib, _ = small.chain(4, 36, 1)
    bad = {0: a_memory_trace_sibling(small, 20),
           K // 2: Case("Keccak query 36 auxiliary leaf", small.plus1(sib - 1), "INITIAL_MERKLE", 4, 36, tree=1, judge=True),
           K - 1: Case("Arithmetic query 3 layer 2", small.plus1(*small.layer_pairs(0, 3, 2)), "FRI_EVAL", 0, 3, layer=2, judge=True)}
    assert len(bad) == 3
    blobs = [small.blob(bad[s].edits) if s in bad else small.proofs for s in range(K)]
    reps = ctx.verify_segments(blobs, [PUB] * K, [small.chal] * K)
    for s, rep in enumerate(reps):
        if s not in bad:
            assert rep.name == "OK", (s, rep.name)
            continue
        bad[s].check(rep)
        own, = ctx.verify_segments([blobs[s]], [PUB], [small.chal])      # (a call of its own: the quad form)
        assert bytes(own) == bytes(rep)
        judged(own, small.code(bad[s].edits))
    assert "segment 0" in reps[0].message


def test_throughput_profile_verifies_three_segments_one_lane(zkm, small):
    """Under "throughput_profile" the threshold is 4096 chains.  Two segments of the fixture's size are 2 x 1924 = 3848 chains and
    still take the quad form (so do the fixture and the repeat=128 segment together, 1924 + 2035); the third segment crosses.  Both
    calls are made, the last blob changed in a Memory trace sibling."""
    per = small.chains()
    K = QUAD_MAX_THROUGHPUT // per + 1
    assert K * per > QUAD_MAX_THROUGHPUT >= (K - 1) * per and K == 3
    case = a_memory_trace_sibling(small, 9)
    c = zkm.Context(0)
    try:
        c.set_tuning("throughput_profile", 1)
        for n in (2, K):
            reps = c.verify_segments([small.proofs] * (n - 1) + [small.blob(case.edits)], [PUB] * n, [small.chal] * n)
            assert [r.name for r in reps[:-1]] == ["OK"] * (n - 1)
            case.check(reps[-1])
            assert judged(reps[-1], small.code(case.edits)) == ("INITIAL_MERKLE", 0)
            assert [r.name for r in c.verify_segments([small.proofs] * n, [PUB] * n, [small.chal] * n)] == ["OK"] * n
    finally:
        c.close()


# ---- 2. every (table, query): the Merkle chains
WORDS = ("leaf's first word", "leaf's last word", "first sibling", "last sibling")


def chain_cases(S):
    """One case per (table, query).  The chain is (t + k) mod the table's 3 + L, the word one of WORDS, stepping each time the chains
    have gone round: with 37 queries and at most six chains every (table, chain, word) comes up.  A chain without siblings (a layer
    whose tree is its cap) has its leaf's words only.  The cases the oracle judges: see the module docstring."""
    cases = []
    for t in range(12):
        nch = 3 + S.L(t)
        mine = []
        for k in range(int(S.lay[t][0].num_queries)):
            c, w = (t + k) % nch, ((t + k) // nch) % 4
            leaf, n, sib, nsib = S.chain(t, k, c)
            if nsib == 0:
                w %= 2
            i = (leaf, leaf + n - 1, sib + 1, sib + 4 * (nsib - 1) + 2)[w]
            name = "table %d query %d chain %d %s" % (t, k, c, WORDS[w])
            if c < 3:
                case = Case(name, S.plus1(i), "INITIAL_MERKLE", t, k, tree=c)
            else:      # the queried evaluation is compared before the layer's path is walked
                at_x = w < 2 and (i - leaf) // 2 == S.within(t, k, c - 3)
                case = Case(name, S.plus1(i), "FRI_EVAL" if at_x else "FRI_MERKLE", t, k, layer=c - 3, judge=at_x)
            case.chain, case.word = c, w
            mine.append(case)
        mine[0].judge = mine[-1].judge = True
        for c in range(nch):
            if not any(case.judge for case in mine if case.chain == c):
                next(case for case in mine if case.chain == c).judge = True
        assert {(case.chain, case.word) for case in mine} >= {(c, w) for c in range(nch) for w in range(2)}
        cases += mine
    return cases


@pytest.fixture(scope="module")
def all_chain_cases(small):
    cases = chain_cases(small)
    assert len(cases) == 12 * 37 and {(c.table, c.query) for c in cases} == {(t, k) for t in range(12) for k in range(37)}
    for t in range(12):
        judged_here = [c for c in cases if c.table == t and c.judge]
        assert {c.chain for c in judged_here} == set(range(3 + small.L(t))) and {0, 36} <= {c.query for c in judged_here}
    return cases


@pytest.mark.parametrize("t", range(12))
@pytest.mark.parametrize("form", FORMS)
def test_every_table_and_query_names_the_changed_chain(lanes, small, all_chain_cases, form, t):
    cases = [c for c in all_chain_cases if c.table == t]
    assert len(cases) == 37 and [c.query for c in cases] == list(range(37))
    sweep(lanes[form], small, cases)


# ---- 3. every (table, query, layer): the FRI arithmetic
def layer_cases(S, t, queries, judge):
    """All sixteen pairs of layer l in query k plus 1: whichever of them is the queried one, the evaluation check of that layer fails,
    and its slot precedes the slot of the layer's Merkle path.  judge(k, l) -> whether the oracle is asked."""
    return [Case("table %d query %d layer %d evaluations" % (t, k, l), S.plus1(*S.layer_pairs(t, k, l)), "FRI_EVAL", t, k, layer=l, judge=judge(k, l))
            for k in queries for l in range(S.L(t))]


@pytest.mark.parametrize("t", range(12))
def test_every_table_query_and_layer_names_the_changed_evaluations(ctx, small, t):
    assert small.L(t) >= 1
    cases = layer_cases(small, t, range(37), lambda k, l: k == (5 * t + 17 * l) % 37)
    assert {(c.query, c.layer) for c in cases} == {(k, l) for k in range(37) for l in range(small.L(t))} and len(cases) == 37 * small.L(t)
    assert sorted(c.layer for c in cases if c.judge) == list(range(small.L(t)))
    sweep(ctx, small, cases)


def test_three_layers_name_the_changed_evaluations(ctx, large):
    """The repeat=128 segment's Cpu table (2^15 rows, L = 3; not the call's first table, so its verdicts do not start at 0)."""
    t = 1
    assert large.L(t) == 3
    cases = layer_cases(large, t, (0, 18, 36), lambda k, l: True)
    assert len(cases) == 9
    sweep(ctx, large, cases)


def test_final_polynomial_changes_are_named_as_the_oracle_names_them(ctx, small):
    """Every coefficient of Arithmetic's final polynomial in turn, and the highest coefficient of every table.  The oracle judges all of
    them; it names POW (module docstring: FINAL_POLY cannot be reached by changing a blob)."""
    F = int(small.lay[0][0].final_poly_len)
    cases = [Case("table 0 final polynomial coefficient %d" % i, small.plus1(small.field(0, "final_poly") + 2 * i + (i & 1)), table=0, judge=True)
             for i in range(F)]
    cases += [Case("table %d highest final polynomial coefficient" % t,
                   small.plus1(small.field(t, "final_poly") + 2 * int(small.lay[t][0].final_poly_len) - 2), table=t, judge=True) for t in range(1, 12)]
    assert len(cases) == F + 11 and F == 16
    sweep(ctx, small, cases)
    assert {expected(small.code(c.edits))[0] for c in cases} == {"POW"}


# ---- 4. more than one finding: the first in the sequential verifier's order is named
def first_word(S, t, k, c):
    return S.chain(t, k, c)[0]


def a_sibling(S, t, k, c):
    _, _, sib, nsib = S.chain(t, k, c)
    assert nsib >= 1
    return sib + 4 * (nsib - 1) + 3


def multi_cases_small(S):
    cpu, mem = 1, MEMORY
    assert S.L(cpu) >= 1 and S.L(mem) == 2
    both = lambda *parts: tuple(e for p in parts for e in p)
    quot7, pow5 = S.plus1(S.field(7, "quotient_polys_open") + 1), S.plus1(S.field(5, "pow_witness"))
    return [
        Case("lower query, later slot", both(S.plus1(a_sibling(S, cpu, 3, 3)), S.plus1(first_word(S, cpu, 20, 0))), "FRI_MERKLE", cpu, 3, layer=0),
        Case("lower query, first slot", both(S.plus1(first_word(S, cpu, 3, 0)), S.plus1(a_sibling(S, cpu, 20, 3))), "INITIAL_MERKLE", cpu, 3, tree=0),
        Case("neighbouring queries", both(S.plus1(a_sibling(S, mem, 7, 4)), S.plus1(first_word(S, mem, 8, 0))), "FRI_MERKLE", mem, 7, layer=1),
        Case("one query: auxiliary tree and layer-1 evaluations", both(S.plus1(first_word(S, mem, 12, 1)), S.plus1(*S.layer_pairs(mem, 12, 1))),
             "INITIAL_MERKLE", mem, 12, tree=1),
        Case("one query: trace tree and layer-1 evaluations", both(S.plus1(a_sibling(S, mem, 36, 0)), S.plus1(*S.layer_pairs(mem, 36, 1))),
             "INITIAL_MERKLE", mem, 36, tree=0),
        Case("one query: quotient tree and layer-0 path", both(S.plus1(first_word(S, mem, 2, 2) + 3), S.plus1(a_sibling(S, mem, 2, 3))),
             "INITIAL_MERKLE", mem, 2, tree=2),
        Case("FRI in table 2, quotient opening in table 7", both(S.plus1(*S.layer_pairs(2, 9, 0)), quot7), "FRI_EVAL", 2, 9, layer=0),
        Case("quotient opening in table 7, Merkle in table 2", both(quot7, S.plus1(first_word(S, 2, 0, 0))), "INITIAL_MERKLE", 2, 0, tree=0),
        Case("Merkle in tables 9 and 3", both(S.plus1(first_word(S, 9, 0, 0)), S.plus1(a_sibling(S, 3, 36, 2))), "INITIAL_MERKLE", 3, 36, tree=2),
        Case("proof of work and a query of one table", both(pow5, S.plus1(first_word(S, 5, 0, 0))), "POW", 5),
    ]


def multi_cases_large(S, t=1):
    """Findings placed by their verdict index query * slots + slot in a table of ten slots (L = 3): k_verify_reduce strides 256 threads
    over the 370 verdicts, so indices 256 apart belong to one thread.  Slot 0..2 the trees, 3 + 2 l the evaluation of layer l, 4 + 2 l
    its path."""
    slots = 4 + 2 * S.L(t)
    assert slots == 10 and 37 * slots > 256

    def at(k, slot):
        return S.plus1(first_word(S, t, k, slot) if slot < 3 else a_sibling(S, t, k, 3 + (slot - 4) // 2))

    def case(name, first, *more):
        idx = [k * slots + s for k, s in (first,) + more]
        assert idx[0] == min(idx)
        k, s = first
        assert all(s < 3 or s % 2 == 0 for _, s in (first,) + more)          # (tree and path slots)
        edits = tuple(e for f in (first,) + more for e in at(*f))
        if s < 3:
            return Case(name, edits, "INITIAL_MERKLE", t, k, tree=s), idx
        return Case(name, edits, "FRI_MERKLE", t, k, layer=(s - 4) // 2), idx
    out = []
    c, idx = case("one thread: verdicts 44 and 300", (4, 4), (30, 0))
    assert idx == [44, 300] and idx[1] - idx[0] == 256
    out.append(c)
    c, idx = case("one thread: verdicts 26 and 282", (2, 6), (28, 2))
    assert idx[1] - idx[0] == 256
    out.append(c)
    c, idx = case("the larger verdict on the lower thread", (5, 0), (30, 0))
    assert idx[1] % 256 < idx[0] % 256
    out.append(c)
    c, idx = case("three findings", (4, 4), (30, 0), (31, 1))
    assert idx == [44, 300, 311]
    out.append(c)
    c, idx = case("the table's last path verdicts", (36, 6), (36, 8))
    assert idx == [366, 368]
    out.append(c)
    return out


@pytest.mark.parametrize("form", FORMS)
def test_two_findings_in_one_segment_name_the_first(lanes, small, form):
    cases = multi_cases_small(small)
    for c in cases:
        c.judge = True
    sweep(lanes[form], small, cases)


@pytest.mark.parametrize("form", FORMS)
def test_findings_256_verdicts_apart_name_the_first(lanes, large, form):
    cases = multi_cases_large(large)
    for c in cases:
        c.judge = True
    sweep(lanes[form], large, cases)


# ---- 5. changes other than plus 1
def other_cases(S):
    """Each judged by the oracle; a change that leaves the blob as it was (equal words exchanged) moves on to the next position."""
    cases = []
    for t, k, c, value in ((0, 1, 0, 0), (0, 1, 0, P - 1), (4, 2, 0, 0), (4, 2, 0, P - 1), (8, 30, 2, 0), (8, 30, 2, P - 1), (MEMORY, 17, 4, 0),
                           (MEMORY, 17, 4, P - 1)):
        leaf, n, _, _ = S.chain(t, k, c)
        i = next(i for i in range(leaf + n - 1, leaf - 1, -1) if int(S.proofs[i]) != value)
        within = c >= 3 and (i - leaf) // 2 == S.within(t, k, c - 3)
        cases.append(Case("table %d query %d chain %d: a leaf word = %s" % (t, k, c, "0" if value == 0 else "p - 1"), ((i, value),),
                          ("INITIAL_MERKLE",) if c < 3 else ("FRI_EVAL",) if within else ("FRI_MERKLE",), t, k, tree=c, layer=c - 3))
    for t, k, c in ((1, 6, 0), (0, 6, 3), (MEMORY, 0, 1)):      # two_to_one(left, right): neighbouring siblings of one path exchanged
        _, _, sib, nsib = S.chain(t, k, c)
        j = next(j for j in range(nsib - 1) if list(S.proofs[sib + 4 * j:sib + 4 * j + 4]) != list(S.proofs[sib + 4 * j + 4:sib + 4 * j + 8]))
        swapped = np.concatenate([S.proofs[sib + 4 * j + 4:sib + 4 * j + 8], S.proofs[sib + 4 * j:sib + 4 * j + 4]])
        cases.append(Case("table %d query %d chain %d: siblings %d and %d exchanged" % (t, k, c, j, j + 1), S.put(sib + 4 * j, swapped),
                          "INITIAL_MERKLE" if c < 3 else "FRI_MERKLE", t, k, tree=c, layer=c - 3))
    for t, name in ((3, "trace_cap"), (0, "commit_phase_merkle_caps")):      # observed by the transcript: the oracle alone says what is named
        cap = S.field(t, name)
        j = next(j for j in range(15) if list(S.proofs[cap + 4 * j:cap + 4 * j + 4]) != list(S.proofs[cap + 4 * j + 4:cap + 4 * j + 8]))
        swapped = np.concatenate([S.proofs[cap + 4 * j + 4:cap + 4 * j + 8], S.proofs[cap + 4 * j:cap + 4 * j + 4]])
        cases.append(Case("table %d %s: entries %d and %d exchanged" % (t, name, j, j + 1), S.put(cap + 4 * j, swapped)))
    for t in (1, 10):        # two whole query rounds exchanged: valid paths, for another x
        xs = S.query_indices(t)
        k = next(k for k in range(10, 36) if xs[k] != xs[k + 1])
        n = int(S.lay[t][0].query_round_words)
        a = S.query(t, k)
        cases.append(Case("table %d: queries %d and %d exchanged" % (t, k, k + 1), S.put(a, np.concatenate([S.proofs[a + n:a + 2 * n], S.proofs[a:a + n]])),
                          "INITIAL_MERKLE", t, k))
    for t, k, l in ((0, 8, 1), (5, 22, 0)):       # a layer's sixteen pairs moved on by one
        pairs = S.layer_pairs(t, k, l)
        w = 2 * S.within(t, k, l)
        moved = np.roll(S.proofs[pairs[0]:pairs[-1] + 1], 2)
        assert list(moved[w:w + 2]) != list(S.proofs[pairs[w]:pairs[w] + 2])
        cases.append(Case("table %d query %d layer %d: evaluations rotated" % (t, k, l), S.put(pairs[0], moved),
                          "FRI_EVAL", t, k, layer=l))
    for c in cases:
        c.judge = True
    return cases


@pytest.mark.parametrize("form", FORMS)
def test_other_changes_are_named_as_the_oracle_names_them(lanes, small, form):
    cases = other_cases(small)
    assert len(cases) == 17 and all(c.edits for c in cases)
    sweep(lanes[form], small, cases)
