"""The Goldilocks Poseidon permutation (width 12, 4 + 22 + 4 rounds, x^7) as the textbook says it, in Python integers: the reference
of tests/test_gpu_poseidon_forms.py, and the input lists of that file (built here so that the CPU suite can check their preconditions).

Nothing here is shared with the kernels: no fused or fast form, no M^2 / M^3, no fused constants.  The only table read is the list
of round constants (ZKM_POSEIDON_RC of oracle/poseidon_constants.inc); the MDS row and diagonal are the public parameters of the hash,
written out below.  A partial-round group is written as ROUNDS (matrix, constants, word-0 s-box), so the kernels' regrouping and their
FUSED_C1 / C2 / C3 tables are checked against it, not assumed.

The one exception, on purpose: mfma_layer_ty() restates the integer arithmetic of the matrix-core layer (csrc/poseidon_mfma_dev.h) --
it exists to produce the (T, Y) pairs that layer hands to its fold at extreme states, as inputs of the FOLD_TY probe."""
import functools
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
WIDTH, ROUNDS, HALF_FULL, PARTIAL = 12, 30, 4, 22
CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]     # first row of the circulant MDS matrix
DIAG = [8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]                # plus this diagonal
SBOX_INV = pow(7, -1, P - 1)                               # x -> x^SBOX_INV undoes x -> x^7


def _load_inc():
    spec = importlib.util.spec_from_file_location("gen_poseidon_constants", os.path.join(ROOT, "tools", "gen_poseidon_constants.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.parse_inc_arrays(open(os.path.join(ROOT, "oracle", "poseidon_constants.inc")).read())


INC = _load_inc()
RC = INC["ZKM_POSEIDON_RC"][:WIDTH * ROUNDS]
assert len(RC) == WIDTH * ROUNDS and all(0 <= c < P for c in RC)


def round_constants(r):
    """The twelve constants of round r; r = 30: none ("after the last round")."""
    return RC[12 * r:12 * r + 12] if r < ROUNDS else [0] * 12


def sbox(x):
    return pow(x, 7, P)


def mds(s):
    """out[r] = sum_i CIRC[i] s[(i + r) mod 12] + DIAG[r] s[r]  (mod p)"""
    return [(sum(CIRC[i] * s[(i + r) % 12] for i in range(12)) + DIAG[r] * s[r]) % P for r in range(12)]


def linear_layer(s, nxt):
    """One linear layer as the full rounds apply it: M s + the constants of round `nxt` (30: none)."""
    return [(a + c) % P for a, c in zip(mds(s), round_constants(nxt))]


def permute(s):
    s = [x % P for x in s]
    for r in range(ROUNDS):
        s = [(x + c) % P for x, c in zip(s, round_constants(r))]
        if r < HALF_FULL or r >= HALF_FULL + PARTIAL:
            s = [sbox(x) for x in s]
        else:
            s[0] = sbox(s[0])
        s = mds(s)
    return s


def partial_rounds(s, first, count):
    """`count` linear layers starting with the one that closes round first - 1: M s + constants of round `first`, then the word-0 s-box
    of round `first`, and so on; the s-box after the last layer is left to the caller (as in the kernels' groups)."""
    s = [x % P for x in s]
    for k in range(count):
        s = linear_layer(s, first + k)
        if k + 1 < count:
            s[0] = sbox(s[0])
    return s


def group3(s, g):
    """Fused group g = 0..6 of the kernels: the linear layers of rounds 3g+3 .. 3g+5 and the word-0 s-boxes of rounds 3g+4, 3g+5."""
    return partial_rounds(s, 3 * g + 4, 3)


def group2(s):
    """The tail group: the linear layers of rounds 24 and 25 with the word-0 s-box of round 25 between them."""
    return partial_rounds(s, 25, 2)


def craft_first_layer(v):
    """The input whose state after the first s-box layer is exactly v (v canonical): in[i] = v[i]^(1/7) - RC[i]."""
    assert all(0 <= x < P for x in v)
    s = [(pow(x, SBOX_INV, P) - c) % P for x, c in zip(v, round_constants(0))]
    assert [sbox((x + c) % P) for x, c in zip(s, round_constants(0))] == list(v)
    return s


# ---------------------------------------------------------------- the matrix-core layer's integer arithmetic (inputs of FOLD_TY)
def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def mfma_layer_ty(s, nxt):
    """(T, Y) per row as csrc/poseidon_mfma_dev.h builds them from any twelve uint64 words: D_b = M (byte b of every word, as int8
    after ^ 0x80); X = D0 + 2^8 D1, Z = D2 + 2^8 D3, U = D4 + 2^8 D5 and Y = y0 + D6 + 2^8 D7 in 32-bit registers;
    T = t0 + sext(X) + 2^16 sext(Z) with U added to its high word.  M s + c == T + 2^48 Y (mod p)."""
    out = []
    for r in range(12):
        c = round_constants(nxt)[r]
        off = 128 * 264 if r == 0 else 128 * 256
        t0 = (c & 0xFFFFFFFF) + off * 0x01010101 + ((((c >> 32) & 0xFFFF) + off * 0x0101) << 32)
        y0 = ((c >> 48) + off * 0x0101) & 0xFFFFFFFF
        D = []
        for b in range(8):
            # (byte ^ 0x80 read as int8 is byte - 128)
            D.append(sum((CIRC[(j - r) % 12] + (DIAG[r] if j == r else 0)) * (((s[j] >> (8 * b)) & 0xFF) - 128) for j in range(12)))
        X = (D[0] + (D[1] << 8)) & 0xFFFFFFFF
        Z = (D[2] + (D[3] << 8)) & 0xFFFFFFFF
        U = (D[4] + (D[5] << 8)) & 0xFFFFFFFF
        Y = (y0 + D[6] + (D[7] << 8)) & 0xFFFFFFFF
        acc = (t0 + _i32(X) + (_i32(Z) << 16)) & M64
        T = ((((acc >> 32) + U) & 0xFFFFFFFF) << 32) | (acc & 0xFFFFFFFF)
        out.append((T, Y))
    return out


# ---------------------------------------------------------------- input lists
# Edge words.  The byte patterns: each matrix-core instruction sees ONE byte position of all twelve words as int8 after ^ 0x80 -- all 0xFF is
# the most positive plane, all 0x00 the most negative, 0x80 is zero, alternating planes drive X = D0 + 2^8 D1 and its neighbours to
# opposite signs.
EDGE = [0, 1, P - 2, P - 1, P, P + 1, P + 0xFFFFFFFE, M64 - 1, M64, 0xFFFFFFFF, 1 << 32, (1 << 32) + 1, 0x7FFFFFFFFFFFFFFF, 1 << 63,
        0xFFFF0000FFFF0000, 0x0000FFFF0000FFFF, 0xFF00FF00FF00FF00, 0x00FF00FF00FF00FF, 0x8080808080808080, 0x7F7F7F7F7F7F7F7F,
        0x0101010101010101]
assert len(EDGE) == 21
ONE_HOT = [(M64, 0), (0, M64), (P - 1, 1), (0xFFFFFFFF, 0xFFFFFFFF00000000)]
WAVE_BLOCK = 320          # first state of the wave-uniform-branch block (a multiple of 64)
TRUNCATED = 389           # 5 mod 64: the edge lists, the wave-uniform-branch block and five random states


def extreme_states():
    """Uniform, alternating and one-hot states of edge words."""
    st = [[e] * 12 for e in EDGE]
    alt = EDGE[:9] + EDGE[-6:]
    st += [[e if i % 2 == 0 else f for i in range(12)] for e in alt for f in alt]
    st += [[e if i == pos else f for i in range(12)] for e, f in ONE_HOT for pos in range(12)]
    return st


@functools.lru_cache(maxsize=None)
def state_list():
    """Every state of the GPU tests, in launch order (a tuple of 12-tuples):
      [0, 294)      extreme states; [294, 320) all 2^64 - 1 -- so states 0..319 are five whole waves of extreme states in the one-lane
                    forms (64 hashes per wave), and whole waves in the quad (16) and 16-lane (4) forms too
      [320, 384)    64 random canonical states of which only state 320 + 37 is all 2^64 - 1: the improbable corrections are branched on
                    per wave and applied per lane
      [384, 1384)   random uint64 words, not reduced
      [1384, 1884)  random canonical states"""
    rng = np.random.default_rng(20261017)
    st = extreme_states()
    assert len(st) == 21 + 225 + 48
    st += [[M64] * 12 for _ in range(WAVE_BLOCK - len(st))]
    block = [[int(x) for x in row] for row in rng.integers(0, P, (64, 12), dtype=np.uint64)]
    block[37] = [M64] * 12
    st += block
    st += [[int(x) for x in row] for row in rng.integers(0, 1 << 64, (1000, 12), dtype=np.uint64)]
    st += [[int(x) for x in row] for row in rng.integers(0, P, (500, 12), dtype=np.uint64)]
    assert len(st) == 1884 and TRUNCATED % 64 == 5 and WAVE_BLOCK + 64 <= TRUNCATED
    return tuple(tuple(s) for s in st)


def canonical_extreme_states():
    """The extreme states made of canonical words only (inputs of craft_first_layer)."""
    return [list(s) for s in extreme_states() if all(x < P for x in s)]


FOLD_AL_BOUND = FOLD_AH_BOUND = 1 << 59        # poseidon_fold: al, ah < 2^59
FOLD_T_BOUND, FOLD_Y_BOUND = 1 << 57, 1 << 27  # poseidon_fold_ty: T < 2^57, Y < 2^27
MDS_NEXT = [1, 2, 3, 27, 28, 29, 30]           # the `next` values the permutation passes to a full-round layer


@functools.lru_cache(maxsize=None)
def fold_vectors():
    """(al, ah) inputs of the FOLD probe; reference (al + 2^32 ah) mod p."""
    rng = np.random.default_rng(59)
    B = 1 << 59
    corner = [0, 1, (1 << 32) - 1, 1 << 32, B - (1 << 32), B - 1]
    v = [(a, h) for a in corner for h in corner]
    # the second carry: s1 = al + EPS ah_hi, hs = s1_hi + ah_lo carries out of 32 bits when ah_lo is (nearly) all ones; s1_hi is at its
    # maximum with al = 2^59 - 1 and ah_hi = 2^27 - 1
    for lo in (0xFFFFFFFF, 0xFFFFFFFE, 0xF8000000, 0xF7FFFFFF, 0x80000000):
        for hi in (0, 1, (1 << 26), (1 << 27) - 2, (1 << 27) - 1):
            for al in (0, 1, (1 << 32) - 1, 1 << 32, (1 << 58), B - (1 << 32), B - 2, B - 1):
                v.append((al, (hi << 32) | lo))
    v += [(int(a), int(h)) for a, h in rng.integers(0, B, (2000, 2), dtype=np.uint64)]
    return tuple(v)


@functools.lru_cache(maxsize=None)
def fold_ty_vectors():
    """(T, Y) inputs of the FOLD_TY probe; reference (T + 2^48 Y) mod p."""
    rng = np.random.default_rng(57)
    BT, BY = 1 << 57, 1 << 27
    tc = [0, 1, (1 << 32) - 1, 1 << 32, BT - (1 << 32), BT - 1]
    yc = [0, 1, (1 << 16) - 1, 1 << 16, BY - (1 << 16), BY - 1]
    v = [(t, y) for t in tc for y in yc]
    # the second carry: t = T + EPS (Y >> 16), and t_hi + ((Y mod 2^16) << 16) carries out of 32 bits when Y mod 2^16 is (nearly) all ones
    # and T >= 2^48; t_hi is at its maximum with T = 2^57 - 1 and Y >> 16 = 2^11 - 1
    for ylo in (0xFFFF, 0xFFFE, 0xFE00, 0xFDFF, 0x8000):
        for yhi in (0, 1, 1 << 10, (1 << 11) - 2, (1 << 11) - 1):
            for t in (0, 1, (1 << 48) - 1, 1 << 48, 1 << 56, BT - (1 << 32), BT - 2, BT - 1):
                v.append((t, (yhi << 16) | ylo))
    v += [(int(t), int(y)) for t, y in zip(rng.integers(0, BT, 2000, dtype=np.uint64), rng.integers(0, BY, 2000, dtype=np.uint64))]
    # what the matrix-core layer hands to the fold at the states whose byte planes are all most positive / all most negative / zero
    for word in (M64, 0, 0x8080808080808080, 0xFF00FF00FF00FF00, 0x00FF00FF00FF00FF):
        for nxt in MDS_NEXT:
            v += mfma_layer_ty([word] * 12, nxt)
    return tuple(v)
