"""GPU suite: stacked commitments (PolynomialBatchStack), their openings (Context.eval_openings_stack) and K opening proofs in lock-step
(Context.fri_prove_stack, zkm_fri_prove_stack).  The single and the stacked entry points are one body (the single call: one claim), so
"the stack equals the single calls" holds that body at K members against itself at one -- member strides, per-claim indexing; what
judges the body itself is the Python model here and the oracle's blobs in tests/test_gpu_prove.py and tests/test_gpu_lde_rates.py.
The judge of every case is the single call on single commitments of the same words:
member k of a stack is PolynomialBatch of member k's words, claim k of a stacked proof is fri_prove on those -- caps, polynomials,
Merkle paths, openings, blobs and final challenger states word for word.  The stacked blobs then go through fri_verify as K claims of one
call, and one claim a shape through the Python model (tests/fri_verify_model.py).  Six queries, random polynomials; shapes, `prove` and
`Claim` are those of tests/test_gpu_fri_verify.py."""
import numpy as np
import pytest

from . import fri_verify_model as M
from .test_gpu_fri_verify import SHAPES, challenger_key, config, key, prove, verify

pytestmark = pytest.mark.gpu

P = M.P


def member_values(seed, cols, log_n):
    """the values `prove` commits for this seed: one array an oracle"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, P, k << log_n, dtype=np.uint64) for k in cols]


def claim_batches(batches, k):
    """claim k's instance: the shape's polynomial lists at points of its own (claim 0: the shape's)"""
    return [(((pt[0] + 1000 * k) % P, (pt[1] + 7 * k) % P), polys) for pt, polys in batches]


def start_challenger(zkm, seed):
    ch = zkm.challenger_new()
    zkm.challenger_observe(ch, [seed, 1, 2])     # (where `prove` starts its own)
    return ch


def commit_stacks(ctx, zkm, cfg, log_n, cols, values):
    """values[k][o] -> one stack an oracle"""
    return [zkm.PolynomialBatchStack.from_values(ctx, [v[o] for v in values], cols[o], log_n, cfg.rate_bits, cfg.cap_height) for o in range(len(cols))]


def prove_stack(ctx, zkm, cfg, log_n, cols, batches, seeds, values=None):
    """(blobs, final challengers) of one fri_prove_stack call: claim k on the polynomials of seeds[k] at claim_batches(batches, k)"""
    values = values or [member_values(s, cols, log_n) for s in seeds]
    stacks = commit_stacks(ctx, zkm, cfg, log_n, cols, values)
    try:
        chs = [start_challenger(zkm, s) for s in seeds]
        points = [[pt for pt, _ in claim_batches(batches, k)] for k in range(len(seeds))]
        blobs = ctx.fri_prove_stack(stacks, [polys for _, polys in batches], points, chs, cfg)
    finally:
        for s in stacks:
            s.free()
    return blobs, chs


def check_against_single_calls(ctx, zkm, cfg, log_n, cols, batches, seeds, model=True):
    blobs, chs = prove_stack(ctx, zkm, cfg, log_n, cols, batches, seeds)
    singles = [prove(ctx, zkm, cfg, log_n, cols, claim_batches(batches, k), s) for k, s in enumerate(seeds)]
    for k, (blob, ch, one) in enumerate(zip(blobs, chs, singles)):
        assert [int(x) for x in blob] == one.blob, "claim %d: the blob differs from the single call's" % k
        assert challenger_key(ch) == challenger_key(one.ch1), "claim %d: the challenger differs from the single call's" % k
    stacked = [one.changed(blob=[int(x) for x in blob]) for one, blob in zip(singles, blobs)]
    reports, dev = verify(ctx, zkm, stacked)
    for k, (rep, d, one) in enumerate(zip(reports, dev, singles)):
        assert key(rep) == (M.OK, 0, 0, 0), (k, rep.name, rep.message)
        assert challenger_key(d.challenger) == challenger_key(one.ch1)
    if model:
        assert stacked[-1].judged() == (M.OK, 0, 0, 0)


# ---------------------------------------------------------------- 1. commitments
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("log_n,ncols,rate_bits,cap_height", [(5, 3, 2, 4), (7, 9, 3, 4), (9, 13, 2, 4)])
def test_stack_members_are_the_single_commitments(ctx, zkm, log_n, ncols, rate_bits, cap_height, K):
    """from values and from coefficients, sources in host and in device memory: every member's cap, polynomials, and leaf + Merkle path at
    the first, a middle and the last leaf are the single commitment's"""
    rng = np.random.default_rng(100 * log_n + K)
    words = [rng.integers(0, P, ncols << log_n, dtype=np.uint64) for _ in range(K)]
    N = 1 << (log_n + rate_bits)
    leaves = (0, N // 2 + 1, N - 1)
    bufs = [ctx.alloc(w.size).upload(w) for w in words]
    try:
        for single, stack in ((zkm.PolynomialBatch.from_values, zkm.PolynomialBatchStack.from_values),
                              (zkm.PolynomialBatch.from_coeffs, zkm.PolynomialBatchStack.from_coeffs)):
            want = []
            for w in words:
                b = single(ctx, w, ncols, log_n, rate_bits, cap_height)
                want.append((b.cap(), b.coeffs(), [(b.leaf(i), b.merkle_path(i)) for i in leaves]))
                b.free()
            for sources in (words, bufs):
                with stack(ctx, sources, ncols, log_n, rate_bits, cap_height) as s:
                    assert len(s) == K == s.nstack
                    for k, (cap, coeffs, paths) in enumerate(want):
                        assert np.array_equal(s.cap(k), cap), k
                        assert np.array_equal(s.coeffs(k), coeffs), k
                        for i, (leaf, path) in zip(leaves, paths):
                            got_leaf, got_path = s.merkle_path(k, i)
                            assert np.array_equal(got_leaf, leaf) and np.array_equal(got_path, path), (k, i)
                    with pytest.raises(zkm.ZkmError):
                        s.cap(K)
                    with pytest.raises(zkm.ZkmError):
                        s.merkle_path(K - 1, N)
    finally:
        for b in bufs:
            b.free()


def test_single_constructors_make_stacks_of_one(ctx, zkm):
    b = zkm.PolynomialBatch.from_values(ctx, np.arange(3 << 5, dtype=np.uint64), 3, 5)
    assert ctx.L.zkm_batch_stack_size(b.h) == 1
    b.free()


def test_single_accessors_on_a_stack_read_member_0_and_nothing_more(ctx, zkm):
    """the accessors that take no member, called through the C ABI on a stack of 3: each writes what it writes for the single commitment
    of member 0's words -- zkm_batch_cap 4 << cap_height words, not the three caps -- and leaves the words behind them alone.  Every
    buffer is (members + 1) times what one member needs, so neither answer leaves it."""
    log_n, ncols, rate_bits, cap_height, K = 5, 3, 2, 4, 3
    rng = np.random.default_rng(9000)
    words = [rng.integers(0, P, ncols << log_n, dtype=np.uint64) for _ in range(K)]
    leaf = (1 << (log_n + rate_bits)) // 2 + 1
    one = zkm.PolynomialBatch.from_values(ctx, words[0], ncols, log_n, rate_bits, cap_height)
    want = {"cap": one.cap(), "coeffs": one.coeffs(), "leaf": one.leaf(leaf), "merkle_path": one.merkle_path(leaf), "digest_layer": one.digest_layer(0)}
    one.free()
    assert want["cap"].size == 4 << cap_height
    sentinel = np.uint64(0xA5A55A5AC3C33C3C)
    with zkm.PolynomialBatchStack.from_values(ctx, words, ncols, log_n, rate_bits, cap_height) as s:
        L = ctx.L
        for name, call in (("cap", lambda out: L.zkm_batch_cap(s.h, out)), ("coeffs", lambda out: L.zkm_batch_coeffs(s.h, out)),
                           ("leaf", lambda out: L.zkm_batch_leaf(s.h, leaf, out)), ("merkle_path", lambda out: L.zkm_batch_merkle_path(s.h, leaf, out)),
                           ("digest_layer", lambda out: L.zkm_batch_digest_layer(s.h, 0, out))):
            size = want[name].size
            buf = np.full((K + 1) * size, sentinel, dtype=np.uint64)
            assert call(buf.ctypes.data) == 0, name
            assert np.array_equal(buf[:size], want[name]), "%s: not member 0's" % name
            assert (buf[size:] == sentinel).all(), "%s: words behind the answer were written" % name


# ---------------------------------------------------------------- 2. openings
@pytest.mark.parametrize("log_n,ncols,K,rate_bits", [(7, 9, 5, 3), (18, 2, 2, 2)])
def test_openings_of_a_stack(ctx, zkm, log_n, ncols, K, rate_bits):
    """a different extension point a member; 2^18 rows at rate 4 is the height where the batch keeps its coefficients in the digit layout"""
    rng = np.random.default_rng(200 + log_n)
    words = [rng.integers(0, P, ncols << log_n, dtype=np.uint64) for _ in range(K)]
    zetas = [tuple(int(x) for x in rng.integers(0, P, 2, dtype=np.uint64)) for _ in range(K)]
    want = []
    for w, z in zip(words, zetas):
        b = zkm.PolynomialBatch.from_values(ctx, w, ncols, log_n, rate_bits, 4)
        want.append(ctx.eval_openings(b, z))
        b.free()
    with zkm.PolynomialBatchStack.from_values(ctx, words, ncols, log_n, rate_bits, 4) as s:
        w0 = ctx.host_waits()
        got = ctx.eval_openings_stack(s, zetas)
        assert ctx.host_waits() - w0 == 1
    assert got.shape == (K, 2 * ncols)
    for k in range(K):
        assert np.array_equal(got[k], want[k]), k


# ---------------------------------------------------------------- 3. proofs
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("name", list(SHAPES))
def test_stacked_proofs_are_the_single_calls(ctx, zkm, name, K):
    """the STARK shape at 2^9 (rate 4, three batches), the PLONK shape at 2^7 and 2^12 (rate 8), 8 oracles x 8 batches with repeated and
    reordered polynomials: own seed, own points and own starting challenger a claim"""
    cfg, log_n, cols, batches = SHAPES[name](ctx)
    seeds = [8000 + 100 * list(SHAPES).index(name) + 10 * K + k for k in range(K)]
    check_against_single_calls(ctx, zkm, cfg, log_n, cols, batches, seeds, model=K in (1, 2))   # (the model: one claim at K = 1 -- the single
                                                                                                # entry's own blob -- and one at K = 2, a shape)


def test_a_full_stack_of_32(ctx, zkm):
    cfg, log_n, cols, batches = SHAPES["plonk7"](ctx)
    check_against_single_calls(ctx, zkm, cfg, log_n, cols, batches, [8500 + k for k in range(32)], model=False)


def test_stacked_proofs_in_the_digit_layout(ctx, zkm):
    """2^18 rows at rate 4: the oracles keep their coefficients in the digit layout, the composites come out in it"""
    batches = [((13, 17), [(0, 1), (1, 0), (0, 0)]), ((19, 0), [(1, 0)])]
    check_against_single_calls(ctx, zkm, config(ctx), 18, [2, 1], batches, [8600, 8601])


# ---------------------------------------------------------------- 4. a changed word is the right claim's
def test_a_changed_polynomial_changes_its_own_claim_only(ctx, zkm):
    cfg, log_n, cols, batches = SHAPES["plonk7"](ctx)
    seeds = [8700 + k for k in range(5)]
    values = [member_values(s, cols, log_n) for s in seeds]
    blobs, chs = prove_stack(ctx, zkm, cfg, log_n, cols, batches, seeds, values)
    values[3][1][4 << log_n] = (int(values[3][1][4 << log_n]) + 1) % P       # member 3, oracle 1, polynomial 4, first value
    blobs2, chs2 = prove_stack(ctx, zkm, cfg, log_n, cols, batches, seeds, values)
    for k in range(5):
        same = np.array_equal(blobs[k], blobs2[k]) and challenger_key(chs[k]) == challenger_key(chs2[k])
        assert same == (k != 3), k


# ---------------------------------------------------------------- 5. host waits
def test_a_stacked_call_waits_as_often_as_one_single_call(ctx, zkm):
    """K single calls that wait W1 times each (a proof-of-work search may need a second launch: such a seed is passed over) against the
    stacked call of the same K claims: W1 too"""
    cfg, log_n, cols, batches = SHAPES["plonk7"](ctx)
    K, seeds, waits = 5, [], {}
    for seed in range(8800, 8830):
        oracles = [zkm.PolynomialBatch.from_values(ctx, v, k, log_n, cfg.rate_bits, cfg.cap_height) for v, k in zip(member_values(seed, cols, log_n), cols)]
        w0 = ctx.host_waits()
        ctx.fri_prove(oracles, claim_batches(batches, 0), start_challenger(zkm, seed), cfg)
        waits[seed] = ctx.host_waits() - w0
        for b in oracles:
            b.free()
        seeds = [s for s in waits if waits[s] == min(waits.values())]
        if len(seeds) >= K:
            break
    assert len(seeds) >= K, waits
    seeds, W1 = seeds[:K], min(waits.values())
    values = [member_values(s, cols, log_n) for s in seeds]
    stacks = commit_stacks(ctx, zkm, cfg, log_n, cols, values)
    chs = [start_challenger(zkm, s) for s in seeds]
    w0 = ctx.host_waits()
    ctx.fri_prove_stack(stacks, [polys for _, polys in batches], [[pt for pt, _ in claim_batches(batches, k)] for k in range(K)], chs, cfg)
    got = ctx.host_waits() - w0
    for s in stacks:
        s.free()
    assert got == W1, (got, W1)


# the waits of one fri_prove call at the plonk7 shape, by seed, measured on the parent commit 791000c ("Lock-step FRI for any instance"),
# where the single entry had its own body
WAITS_OF_A_SINGLE_CALL_AT_791000C = {8800: 4, 8801: 4, 8802: 4}


def test_a_single_call_waits_no_more_often_than_it_did(ctx, zkm):
    cfg, log_n, cols, batches = SHAPES["plonk7"](ctx)
    for seed, parent in WAITS_OF_A_SINGLE_CALL_AT_791000C.items():
        oracles = [zkm.PolynomialBatch.from_values(ctx, v, k, log_n, cfg.rate_bits, cfg.cap_height) for v, k in zip(member_values(seed, cols, log_n), cols)]
        w0 = ctx.host_waits()
        ctx.fri_prove(oracles, claim_batches(batches, 0), start_challenger(zkm, seed), cfg)
        got = ctx.host_waits() - w0
        for b in oracles:
            b.free()
        assert got <= parent, (seed, got, parent)


# ---------------------------------------------------------------- 6. refusals and atomicity
def test_the_single_entries_refuse_a_stack(ctx, zkm):
    """zkm_fri_prove and zkm_eval_openings given stacks of 2: refused in their own words, the challenger bit for bit and the context's
    memory as they were"""
    cfg, log_n, cols = config(ctx), 5, [3, 2]
    rng = np.random.default_rng(9100)
    words = [[rng.integers(0, P, c << log_n, dtype=np.uint64) for c in cols] for _ in range(2)]
    stacks = commit_stacks(ctx, zkm, cfg, log_n, cols, words)
    batches = [((5, 6), [(0, 0), (1, 1), (0, 2)]), ((7, 8), [(1, 0)])]
    for call, want in ((lambda ch: ctx.fri_prove(stacks, batches, ch, cfg), "zkm_fri_prove: stacked batches are internal"),
                       (lambda ch: ctx.eval_openings(stacks[0], (5, 6)), "zkm_eval_openings: stacked batches are internal")):
        ch = start_challenger(zkm, 9100)
        before, memory = bytes(ch), ctx.memory()
        with pytest.raises(zkm.ZkmError) as e:
            call(ch)
        assert want in str(e.value), (want, str(e.value))
        assert bytes(ch) == before
        assert ctx.memory() == memory
    for s in stacks:
        s.free()


def test_refusals_leave_challengers_memory_and_context_as_they_were(ctx, zkm):
    """a stack of 33 (refused where a stack is made: the claims of a call ARE its oracles' members), oracles of different stack sizes, a
    polynomial index out of range, a non-canonical point in claim 2; after each the callers' challengers and the context's live bytes are
    what they were, and a good call succeeds"""
    cfg, log_n, cols = config(ctx), 5, [3, 2]
    lists = [[(0, 0), (1, 1), (0, 2)], [(1, 0)]]
    K = 3
    rng = np.random.default_rng(8900)
    words = [[rng.integers(0, P, c << log_n, dtype=np.uint64) for c in cols] for _ in range(K)]
    stacks = commit_stacks(ctx, zkm, cfg, log_n, cols, words)
    short = zkm.PolynomialBatchStack.from_values(ctx, [w[1] for w in words[:2]], cols[1], log_n, cfg.rate_bits, cfg.cap_height)
    points = [[(5 + k, 6), (7, 8 + k)] for k in range(K)]
    bad_points = [list(p) for p in points]
    bad_points[2][1] = (7, P)

    def good():
        chs = [start_challenger(zkm, 8900 + k) for k in range(K)]
        before = [challenger_key(ch) for ch in chs]
        blobs = ctx.fri_prove_stack(stacks, lists, points, chs, cfg)
        assert len(blobs) == K and all(challenger_key(ch) != b for ch, b in zip(chs, before))
        return blobs

    first = good()
    for call, want in (
            (lambda chs: zkm.PolynomialBatchStack.from_values(ctx, [words[0][0]] * 33, cols[0], log_n, cfg.rate_bits, cfg.cap_height), "1..32 members"),
            (lambda chs: ctx.fri_prove_stack([stacks[0], short], lists, points, chs, cfg), "zkm_fri_prove_stack: oracles must be stacks of one size"),
            (lambda chs: ctx.fri_prove_stack(stacks, [lists[0], [(1, 2)]], points, chs, cfg), "zkm_fri_prove_stack: polynomial index out of range"),
            (lambda chs: ctx.fri_prove_stack(stacks, [lists[0], [(2, 0)]], points, chs, cfg), "zkm_fri_prove_stack: polynomial index out of range"),
            (lambda chs: ctx.fri_prove_stack(stacks, [lists[0], []], points, chs, cfg), "zkm_fri_prove_stack: empty batch"),
            (lambda chs: ctx.fri_prove_stack(stacks, lists, bad_points, chs, cfg), "zkm_fri_prove_stack: claim 2: non-canonical opening point")):
        chs = [start_challenger(zkm, 8900 + k) for k in range(K)]
        before, live = [challenger_key(ch) for ch in chs], ctx.memory()[0]
        with pytest.raises(zkm.ZkmError) as e:
            call(chs)
        assert want in str(e.value), (want, str(e.value))
        assert [challenger_key(ch) for ch in chs] == before
        assert ctx.memory()[0] == live
        again = good()
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    short.free()
    for s in stacks:
        s.free()
