"""GPU parity: every device form of the Poseidon permutation, and every layer, group and fold they are made of, on worst-case loose
words -- through zkm_poseidon_selftest, against the textbook permutation in Python integers (tests/poseidon_model.py).

Leaf hashing feeds these kernels the LDE of field data: a word >= p once in 2^32, never a state whose 32-bit halves are all ones or whose
byte planes are all 0xFF / 0x00 / 0x80.  Those are the inputs that maximise every accumulator the kernels' comments make range claims
about (poseidon_fold, poseidon_fold_ty, the matrix-core layer's 32-bit partial sums, gl_add_lc, the second correction of gl_sub_rr).
There is no tolerance: one differing word fails, and the message names probe, arg, state, word and the input state in hex."""
import functools
import json
import os

import numpy as np
import pytest

from . import poseidon_model as pm

pytestmark = pytest.mark.gpu
P = pm.P
ALL, CAPACITY, DIGEST = 0, 1, 2
FORMS = ["PERMUTE_LANE", "PERMUTE_LANE_MFMA", "PERMUTE_QUAD", "PERMUTE_WIDE"]
ONE_LANE = FORMS[:2]
_U64_P = np.uint64(P)


def as_array(states):
    return np.array(states, dtype=np.uint64).reshape(len(states), -1)


@functools.lru_cache(maxsize=None)
def inputs():
    a = as_array(pm.state_list())
    a.setflags(write=False)
    return a


def model_array(fn):
    """fn over every state of the list, once: an (n, 12) array that nobody writes to."""
    a = as_array([fn(list(s)) for s in pm.state_list()])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want_mds():
    return model_array(pm.mds)


@functools.lru_cache(maxsize=None)
def want_layer(nxt):
    rc = np.array(pm.round_constants(nxt), dtype=object)
    a = as_array([[int(x) for x in row] for row in (want_mds().astype(object) + rc) % P])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want_group3(g):
    return model_array(lambda s: pm.group3(s, g))


@functools.lru_cache(maxsize=None)
def want_group2():
    return model_array(pm.group2)


@functools.lru_cache(maxsize=None)
def want_permute():
    return model_array(pm.permute)


def cut_length(n):
    """The largest length <= n that is 5 mod 64."""
    return n - (n - 5) % 64


def reduce(got):
    return np.where(got >= _U64_P, got - _U64_P, got)


def compare(probe, arg, got, want, src, words=range(12), canonical=False):
    """got == want (mod p; as words and < p where the kernel promises canonical output) on the given words of every state."""
    words = list(words)
    assert got.shape[0] == want.shape[0] == src.shape[0]
    g, w = got[:, words], want[:, words]
    bad = np.argwhere((g if canonical else reduce(g)) != w)
    if len(bad):
        i, k = int(bad[0][0]), words[int(bad[0][1])]
        raise AssertionError("%s arg %d: state %d word %d: got %#x, want %#x%s; %d words differ; input state %s" % (
            probe, arg, i, k, int(got[i, k]), int(want[i, k]), "" if canonical else " (mod p)", len(bad), [hex(int(x)) for x in src[i]]))


@functools.lru_cache(maxsize=None)
def _launch(ctx, probe, arg, n):
    out = ctx.poseidon_selftest(probe, arg, inputs()[:n])
    out.setflags(write=False)
    return out


def run_both(ctx, probe, arg):
    """The probe on the whole list, and once more on the list cut to a length that is 5 mod 64 (a partly filled last wave and workgroup in
    every form); the cut run must reproduce the whole run's words."""
    full, cut = _launch(ctx, probe, arg, len(pm.state_list())), _launch(ctx, probe, arg, pm.TRUNCATED)
    assert full.shape == (len(pm.state_list()), 12) and cut.shape == (pm.TRUNCATED, 12)
    return full, cut


def check_both(ctx, probe, arg, want, **kw):
    full, cut = run_both(ctx, probe, arg)
    compare(probe, arg, full, want, inputs(), **kw)
    compare(probe + " (cut list)", arg, cut, want[:pm.TRUNCATED], inputs()[:pm.TRUNCATED], **kw)
    return full


# ---------------------------------------------------------------- 1. layers and groups
@pytest.mark.parametrize("nxt", pm.MDS_NEXT)
@pytest.mark.parametrize("probe", ["MDS_VALU", "MDS_MFMA", "MDS_QUAD"])
def test_full_round_layer(ctx, probe, nxt):
    check_both(ctx, probe, nxt, want_layer(nxt))


@pytest.mark.parametrize("nxt", pm.MDS_NEXT)
def test_matrix_core_layer_agrees_with_the_vector_layer(ctx, nxt):
    a, b = _launch(ctx, "MDS_VALU", nxt, len(pm.state_list())), _launch(ctx, "MDS_MFMA", nxt, len(pm.state_list()))
    compare("MDS_MFMA against MDS_VALU", nxt, b, reduce(a), inputs())


@pytest.mark.parametrize("rows", [0, 1])
def test_last_layer_rows(ctx, rows):
    check_both(ctx, "MDS_ROWS", rows, want_mds(), words=range(0, 4) if rows == 0 else range(8, 12))


@pytest.mark.parametrize("g", range(7))
@pytest.mark.parametrize("probe", ["GROUP3", "GROUP3_QUAD"])
def test_fused_group_of_three_partial_rounds(ctx, probe, g):
    check_both(ctx, probe, g, want_group3(g))


def test_fused_tail_group_of_two_partial_rounds(ctx):
    check_both(ctx, "GROUP2", 0, want_group2())


# ---------------------------------------------------------------- 2. the folds
@pytest.mark.parametrize("probe", ["FOLD", "FOLD_TY"])
def test_folds(ctx, probe):
    vec = pm.fold_vectors() if probe == "FOLD" else pm.fold_ty_vectors()
    shift = 32 if probe == "FOLD" else 48
    want = [(a + (b << shift)) % P for a, b in vec]
    for n in (len(vec), cut_length(len(vec))):
        got = ctx.poseidon_selftest(probe, 0, as_array(vec[:n]))
        assert got.shape == (n,)
        bad = [i for i in range(n) if int(got[i]) % P != want[i]]
        assert not bad, "%s: pair %d (%#x, %#x): got %#x, want %#x (mod p); %d pairs differ" % (
            probe, bad[0], vec[bad[0]][0], vec[bad[0]][1], int(got[bad[0]]), want[bad[0]], len(bad))


# ---------------------------------------------------------------- 3. word-wise pieces
@pytest.mark.parametrize("probe", ["SBOX7", "SBOX_DELTA", "ADD_RC0"])
def test_wordwise_pieces(ctx, probe):
    rc0 = pm.round_constants(0)
    fn = {"SBOX7": lambda s: [pm.sbox(x) for x in s],
          "SBOX_DELTA": lambda s: [(pm.sbox(x) - x) % P for x in s],
          "ADD_RC0": lambda s: [(x + c) % P for x, c in zip(s, rc0)]}[probe]
    check_both(ctx, probe, 0, model_array(fn))


# ---------------------------------------------------------------- 4. whole permutations
@pytest.mark.parametrize("probe", FORMS)
def test_whole_permutation(ctx, probe):
    full = check_both(ctx, probe, ALL, want_permute(), canonical=True)
    assert (full < _U64_P).all()


@pytest.mark.parametrize("probe", ONE_LANE)
def test_capacity_and_digest_outputs(ctx, probe):
    check_both(ctx, probe, CAPACITY, want_permute(), words=range(8, 12))
    full = check_both(ctx, probe, DIGEST, want_permute(), words=range(0, 4), canonical=True)
    assert (full[:, :4] < _U64_P).all()


def test_the_four_forms_agree_word_for_word(ctx):
    outs = [_launch(ctx, probe, ALL, len(pm.state_list())) for probe in FORMS]
    for probe, out in zip(FORMS[1:], outs[1:]):
        compare(probe + " against " + FORMS[0], ALL, out, outs[0], inputs(), canonical=True)


SPONGE_STATES = 640      # the extreme states, the wave-uniform-branch block and 256 states of random words


@functools.lru_cache(maxsize=None)
def sponge_fresh_words():
    """Eight fresh edge words per state for the second absorb step (a different window of EDGE for every state)."""
    a = as_array([[pm.EDGE[(i + 5 * k) % len(pm.EDGE)] for k in range(8)] for i in range(SPONGE_STATES)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want_sponge():
    cap = want_permute()[:SPONGE_STATES, 8:12]
    a = as_array([pm.permute([int(x) for x in fresh] + [int(x) for x in c]) for fresh, c in zip(sponge_fresh_words(), cap)])
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("probe", FORMS)
def test_two_step_sponge(ctx, probe):
    """What the leaf kernels do between two chunks of a row: a permutation that only produces the capacity words -- loose, they may be >= p
    -- whose RAW words go into the next permutation together with eight fresh words; then the digest."""
    src = inputs()[:SPONGE_STATES]
    first = ctx.poseidon_selftest(probe, CAPACITY, src)
    compare(probe, CAPACITY, first, want_permute()[:SPONGE_STATES], src, words=range(8, 12))
    second_in = np.concatenate([sponge_fresh_words(), first[:, 8:12]], axis=1)
    second = ctx.poseidon_selftest(probe, DIGEST, second_in)
    compare(probe + " (second step)", DIGEST, second, want_sponge(), second_in, words=range(0, 4), canonical=True)


# ---------------------------------------------------------------- 5. crafted interior states
@functools.lru_cache(maxsize=None)
def crafted():
    """Inputs whose state after the first s-box layer is a chosen extreme state (all p - 1, all 2^32 - 1, alternating, one-hot ...): the
    extreme halves and byte planes arrive at the first MDS layer INSIDE the real permutation of every form."""
    src = as_array([pm.craft_first_layer(v) for v in pm.canonical_extreme_states()])
    want = as_array([pm.permute([int(x) for x in s]) for s in src])
    src.setflags(write=False)
    want.setflags(write=False)
    return src, want


@pytest.mark.parametrize("probe", FORMS)
def test_crafted_interior_states(ctx, probe):
    src, want = crafted()
    assert len(src) > 64
    for n in (len(src), cut_length(len(src))):
        got = ctx.poseidon_selftest(probe, ALL, src[:n])
        compare(probe + " (crafted)", ALL, got, want[:n], src[:n], canonical=True)


# ---------------------------------------------------------------- the entry point's own checks
def test_selftest_rejects_what_it_must_never_launch(ctx, zkm):
    one = np.zeros(12, dtype=np.uint64)
    for probe, arg in ((16, 0), (0xFFFFFFFF, 0), ("PERMUTE_LANE", 3), ("PERMUTE_WIDE", 7), ("MDS_VALU", 0), ("MDS_MFMA", 4), ("MDS_MFMA", 31),
                       ("MDS_QUAD", 26), ("MDS_ROWS", 2), ("GROUP3", 7), ("GROUP3_QUAD", 8), ("GROUP2", 1), ("FOLD", 1), ("SBOX7", 2)):
        with pytest.raises(zkm.ZkmError):
            ctx.poseidon_selftest(probe, arg, one)
    with pytest.raises(zkm.ZkmError):
        ctx.poseidon_selftest("PERMUTE_LANE", ALL, np.zeros(0, dtype=np.uint64))
    # ... and the context is still good
    kat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "poseidon_kat.json")))["vectors"][0]
    assert [int(x) for x in ctx.poseidon_selftest("PERMUTE_QUAD", ALL, np.array(kat["in"], dtype=np.uint64))[0]] == kat["out"]
