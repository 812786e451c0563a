"""CPU suite: tests/poseidon_model.py -- the textbook permutation the device Poseidon probes are compared with -- is the permutation,
and the input lists it builds for the fold probes stay inside the preconditions those folds document."""
import json
import os

import numpy as np

from . import poseidon_model as pm

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_model_reproduces_the_known_answers():
    kat = json.load(open(os.path.join(GOLD, "poseidon_kat.json")))
    assert kat["vectors"]
    for v in kat["vectors"]:
        assert pm.permute(v["in"]) == v["out"]


def test_model_equals_the_oracles_textbook_permutation(oracle):
    rng = np.random.default_rng(200)
    for _ in range(200):
        st = rng.integers(0, pm.P, 12, dtype=np.uint64)
        assert pm.permute([int(x) for x in st]) == [int(x) for x in oracle.poseidon_permute(st, naive=True)]


def test_model_parameters_are_the_tables_parameters():
    assert pm.CIRC == pm.INC["ZKM_POSEIDON_MDS_CIRC"] and pm.DIAG == pm.INC["ZKM_POSEIDON_MDS_DIAG"]
    assert pm.INC["ZKM_POSEIDON_RC"][360:] == [0] * 12


def test_groups_and_layers_compose_to_the_permutation():
    """The pieces the layer probes are compared with, chained the way the kernels chain them, are the whole permutation: constant add, four
    s-box layers with three full-round layers between them, seven groups of three partial rounds each followed by the word-0 s-box, the
    group of two, and four more full rounds."""
    rng = np.random.default_rng(201)
    states = [[int(x) for x in rng.integers(0, pm.P, 12, dtype=np.uint64)] for _ in range(20)] + pm.canonical_extreme_states()[:40]
    for st in states:
        s = [(x + c) % pm.P for x, c in zip(st, pm.round_constants(0))]
        for r in range(8):
            s = [pm.sbox(x) for x in s]
            if r == 3:
                for g in range(7):
                    s = pm.group3(s, g)
                    s[0] = pm.sbox(s[0])
                s = pm.group2(s)
            else:
                s = pm.linear_layer(s, (r if r < 3 else 22 + r) + 1)
        assert s == pm.permute(st)


def test_crafted_inputs_put_the_chosen_state_behind_the_first_sbox_layer():
    states = pm.canonical_extreme_states()
    assert len(states) > 50 and [pm.P - 1] * 12 in states and [0xFFFFFFFF] * 12 in states
    for v in states:
        s = pm.craft_first_layer(v)                       # (asserts the property itself)
        assert all(0 <= x < pm.P for x in s)


def test_state_list_layout():
    st = pm.state_list()
    assert len(st) == 1884 and all(len(s) == 12 and all(0 <= x <= pm.M64 for x in s) for s in st)
    assert st[:294] == tuple(tuple(s) for s in pm.extreme_states())
    # whole waves of extreme states in every form (64, 16 and 4 hashes per wave), the lone all-ones state in an otherwise canonical wave
    assert pm.WAVE_BLOCK % 64 == 0 and all(s == (pm.M64,) * 12 for s in st[294:pm.WAVE_BLOCK])
    block = st[pm.WAVE_BLOCK:pm.WAVE_BLOCK + 64]
    assert block[37] == (pm.M64,) * 12 and all(max(s) < pm.P for i, s in enumerate(block) if i != 37)
    assert pm.TRUNCATED % 64 == 5
    assert all(max(s) < pm.P for s in st[1384:])


def test_fold_inputs_satisfy_the_folds_precondition():
    v = pm.fold_vectors()
    assert len(v) > 2000
    for al, ah in v:
        assert 0 <= al < pm.FOLD_AL_BOUND and 0 <= ah < pm.FOLD_AH_BOUND, (hex(al), hex(ah))
    # the list does reach the second carry (hs = s1_hi + ah_lo >= 2^32) and the largest s1_hi
    assert any((((ah >> 32) * 0xFFFFFFFF + al) >> 32) + (ah & 0xFFFFFFFF) >= 1 << 32 for al, ah in v)
    assert ((1 << 59) - 1, (((1 << 27) - 1) << 32) | 0xFFFFFFFF) in v


def test_fold_ty_inputs_satisfy_the_folds_precondition():
    v = pm.fold_ty_vectors()
    assert len(v) > 2000
    for t, y in v:
        assert 0 <= t < pm.FOLD_T_BOUND and 0 <= y < pm.FOLD_Y_BOUND, (hex(t), hex(y))
    assert any((((y >> 16) * 0xFFFFFFFF + t) >> 32) + ((y & 0xFFFF) << 16) >= 1 << 32 for t, y in v)


def test_matrix_core_arithmetic_model_is_the_linear_layer():
    """mfma_layer_ty (the source of the FOLD_TY probe's layer-made inputs) follows the matrix-core layer's integer arithmetic; at every
    extreme state and every `next` its (T, Y) are inside the fold's precondition and T + 2^48 Y is the layer."""
    states = [list(s) for s in pm.state_list()[:pm.WAVE_BLOCK]] + [list(s) for s in pm.state_list()[384:414]]
    for nxt in pm.MDS_NEXT:
        for s in states:
            ty = pm.mfma_layer_ty(s, nxt)
            assert all(t < pm.FOLD_T_BOUND and y < pm.FOLD_Y_BOUND for t, y in ty), (nxt, [hex(x) for x in s])
            assert [(t + (y << 48)) % pm.P for t, y in ty] == pm.linear_layer(s, nxt), (nxt, [hex(x) for x in s])
