"""The four-round partial groups of the one-lane permutation (csrc/poseidon_dev.h poseidon_partial_group_t<4>, poseidon_fold_wide), without
a GPU: the HOST build of the header, compiled here behind a pipe (tests/poseidon_host_driver.cpp), against the plonky2 test vectors, the
oracle's permutation and the textbook rounds of tests/poseidon_model.py / poseidon_group4_model.py; and the generator's tables -- its three bounds, and that a re-run
writes every generated file byte for byte."""
import importlib.util
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from . import poseidon_group4_model as g4
from . import poseidon_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkm_amd", "csrc")
P = pm.P
ALL, CAPACITY, DIGEST = 0, 1, 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("poseidon_host") / "driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "poseidon_host_driver.cpp")])

    def run(mode, arg, words):
        a = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
        out = subprocess.run([exe, mode, str(arg)], input=a.tobytes(), stdout=subprocess.PIPE, check=True).stdout
        return np.frombuffer(out, dtype=np.uint64)
    return run


def states():
    """The four-round-group list, the extreme states and the wave-uniform-branch block of the GPU suite, and random canonical states."""
    return np.array(g4.group4_states() + pm.state_list()[:384] + pm.state_list()[1384:1584], dtype=np.uint64)


def test_host_build_reproduces_the_plonky2_vectors(driver):
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_kat.json")))["vectors"]
    got = driver("permute", ALL, [v["in"] for v in kat]).reshape(-1, 12)
    assert [[int(x) for x in row] for row in got] == [v["out"] for v in kat]


def test_host_build_matches_the_oracle_permutation(driver, oracle):
    src = states()
    want = oracle.poseidon_permute_batch(np.where(src >= np.uint64(P), src - np.uint64(P), src)).reshape(-1, 12)   # (a loose word stands for its residue)
    got = driver("permute", ALL, src).reshape(-1, 12)
    assert (got == want).all(), "state %d" % int(np.argwhere(got != want)[0][0])
    cap = driver("permute", CAPACITY, src).reshape(-1, 12)[:, 8:12]
    assert (np.where(cap >= np.uint64(P), cap - np.uint64(P), cap) == want[:, 8:12]).all()
    assert (driver("permute", DIGEST, src).reshape(-1, 12)[:, :4] == want[:, :4]).all()


@pytest.mark.parametrize("g", range(5))
def test_host_four_round_group_matches_the_textbook_rounds(driver, g):
    src = g4.group4_states()
    got = driver("group4", g, src).reshape(-1, 12)
    for i, s in enumerate(src):
        assert [int(x) % P for x in got[i]] == g4.group4(list(s), g), (g, i)


def test_host_three_round_tail_group_matches_the_textbook_rounds(driver):
    src = g4.group4_states()
    got = driver("group3tail", 0, src).reshape(-1, 12)
    for i, s in enumerate(src):
        assert [int(x) % P for x in got[i]] == g4.group3_tail(list(s)), i


def test_groups_compose_to_the_partial_round_section():
    """The model's own bookkeeping: five four-round groups, each followed by the next round's word-0 s-box, and the three-round group
    are the linear layers of rounds 3 .. 25 with the s-boxes of rounds 4 .. 25."""
    for s in g4.group4_states()[300:310]:
        x = list(s)
        for g in range(5):
            x = g4.group4(x, g)
            x[0] = pm.sbox(x[0])
        assert g4.group3_tail(x) == pm.partial_rounds(list(s), 4, 23)


def test_host_wide_fold(driver):
    vec = g4.fold_wide_vectors()
    got = driver("foldwide", 0, vec)
    assert got.shape == (len(vec),)
    bad = [i for i, v in enumerate(vec) if int(got[i]) % P != g4.fold_wide_value(*v)]
    assert not bad, "triple %d %s: got %#x" % (bad[0], [hex(x) for x in vec[bad[0]]], int(got[bad[0]]))


# ---------------------------------------------------------------- the generator
def generator():
    spec = importlib.util.spec_from_file_location("gen_poseidon_constants", os.path.join(ROOT, "tools", "gen_poseidon_constants.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_generator_bounds():
    """(a) every entry of M^4 < 2^32; (b) a half-sum is exact before its last multiply-add; (c) the complete half-sum is < 2^65 -- from the
    matrix written out in tests/poseidon_model.py, through the generator's own bound function, and as static_asserts in the include."""
    gen = generator()
    m = [[pm.CIRC[(j - i) % 12] + (pm.DIAG[i] if i == j else 0) for j in range(12)] for i in range(12)]
    mul = lambda a, b: [[sum(a[i][t] * b[t][j] for t in range(12)) for j in range(12)] for i in range(12)]
    m2 = mul(m, m)
    m3 = mul(m2, m)
    m4 = mul(m3, m)
    a, b, c = gen.group4_bounds(m, m2, m3, m4)
    assert a == 381558488 and a < 1 << 32
    assert b < 1 << 64
    assert 1 << 64 <= c < 1 << 65                      # the carry is real: the plain fold's 2^59 does not hold
    assert max(sum(r) for r in m4) == 4466052512 and min(min(r) for r in m4) == 357057728
    assert max(max(r) for r in mul(m4, m)) >= 1 << 32   # ... and five rounds do not fit a 32-bit multiplier
    inc = gen.parse_inc_arrays  # (tables of the include: the M^4 rows are uint32 tables, read here by pattern)
    text = open(os.path.join(CSRC, "poseidon_group4.inc")).read()
    assert text.count("static_assert(") == 2 and "zkm_poseidon_group4_bounds()" in text
    rows = [[int(x) for x in r.replace("u", "").split(",")] for r in __import__("re").findall(r"\{([0-9u, ]+)\},", text.split("ZKM_POSEIDON_G4_DCOL")[0])]
    assert rows == m4
    tables = inc(text)
    # the constants of group 1 (rounds 8 .. 11) against the rounds
    c4 = tables["ZKM_POSEIDON_G4_C4"][12:24]
    x = [0] * 12
    heads = []
    for k in range(4):   # the same rounds with the s-boxes left out: what the constants alone contribute
        x = pm.linear_layer(x, 8 + k)
        heads.append(x[0])
    assert c4 == x and [tables["ZKM_POSEIDON_G4_C1"][1], tables["ZKM_POSEIDON_G4_C2"][1], tables["ZKM_POSEIDON_G4_C3"][1]] == heads[:3]


def test_generator_rerun_is_byte_identical(tmp_path, monkeypatch):
    """A re-run writes poseidon_constants.inc (both copies) and poseidon_group4.inc exactly as they are committed."""
    gen = generator()
    committed = list(gen.OUTS) + [gen.OUT_GROUP4]
    outs = [str(tmp_path / ("out%d.inc" % i)) for i in range(len(committed))]
    shutil.copy(committed[0], outs[0])    # (without a reference checkout the generator reads the parameters from its first output)
    monkeypatch.setattr(gen, "OUTS", outs[:-1])
    monkeypatch.setattr(gen, "OUT_GROUP4", outs[-1])
    monkeypatch.setattr(gen, "REF", str(tmp_path / "no-reference"))
    gen.main()
    for want, got in zip(committed, outs):
        assert open(want, "rb").read() == open(got, "rb").read(), os.path.relpath(want, ROOT)
