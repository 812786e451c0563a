"""The four-round partial groups of the one-lane permutation (csrc/poseidon_dev.h poseidon_partial_group_t<4>: the 23 linear layers of
rounds 3 .. 25 as 4+4+4+4+4+3) as the textbook says them, and the input lists of their tests -- an extension of tests/poseidon_model.py,
whose rounds it uses and whose rules it keeps: groups are written as ROUNDS (matrix, constants, word-0 s-box), nothing is shared with the
kernels.  The one exception, on purpose: fold_wide_vectors() builds M^4 in integers to produce the half-sums a row of M^4 hands to its
fold at the all-ones state, as INPUTS of the FOLD_WIDE probe."""
import functools

import numpy as np

from .poseidon_model import CIRC, DIAG, M64, P, partial_rounds


def group4(s, g):
    """Four-round group g = 0..4: the linear layers of rounds 4g+3 .. 4g+6 and the word-0 s-boxes of rounds 4g+4 .. 4g+6."""
    return partial_rounds(s, 4 * g + 4, 4)


def group3_tail(s):
    """The three-round group that closes the section: the linear layers of rounds 23 .. 25 and the word-0 s-boxes of rounds 24, 25."""
    return partial_rounds(s, 24, 3)


HALF_HI, HALF_LO = 0xFFFFFFFF00000000, 0x00000000FFFFFFFF
GROUP4_WORDS = [P - 1, P, P + 1, 0, (1 << 32) - 1]
GROUP4_LONE = 320 + 17        # the all-ones state in lane 17 of a wave of canonical random states
GROUP4_CUT = 64 * 6 + 37      # a partly filled last wave


@functools.lru_cache(maxsize=None)
def group4_states():
    """The states of the four-round-group tests, in launch order (a tuple of 12-tuples):
      [0, 3)      twelve words of 2^64 - 1 (both half-sums of every M^4 row carry), of 0xFFFFFFFF00000000 and of 0x00000000FFFFFFFF (one does)
      [3, 273)    p - 1, p, p + 1, 0 and 2^32 - 1 as uniform (5), alternating (25) and one-hot (240) states
      [273, 320)  random uint64 words, not reduced
      [320, 384)  one wave of random canonical states of which only lane 17 is all 2^64 - 1: the carry corrections are branched on per wave
                  and applied per lane
      [384, 421)  random canonical states: 37 lanes of a last wave"""
    rng = np.random.default_rng(20261020)
    W = GROUP4_WORDS
    st = [[M64] * 12, [HALF_HI] * 12, [HALF_LO] * 12]
    st += [[e] * 12 for e in W]
    st += [[e if i % 2 == 0 else f for i in range(12)] for e in W for f in W]
    st += [[e if i == pos else f for i in range(12)] for e in W for f in W if e != f for pos in range(12)]
    assert len(st) == 273
    st += [[int(x) for x in row] for row in rng.integers(0, 1 << 64, (320 - len(st), 12), dtype=np.uint64)]
    wave = [[int(x) for x in row] for row in rng.integers(0, P, (64, 12), dtype=np.uint64)]
    wave[17] = [M64] * 12
    st += wave
    st += [[int(x) for x in row] for row in rng.integers(0, P, (GROUP4_CUT - len(st), 12), dtype=np.uint64)]
    assert len(st) == GROUP4_CUT and st[GROUP4_LONE] == [M64] * 12 and GROUP4_CUT % 64 == 37
    return tuple(tuple(s) for s in st)


def fold_wide_value(al, ah, carries):
    """(al + 2^64 cl) + 2^32 (ah + 2^64 ch) mod p, carries = cl + 2 ch."""
    return (al + ((carries & 1) << 64) + ((ah + ((carries >> 1) << 64)) << 32)) % P


@functools.lru_cache(maxsize=None)
def fold_wide_vectors():
    """(al, ah, cl + 2 ch) inputs of the FOLD_WIDE probe: any al, ah < 2^64 with any carries."""
    rng = np.random.default_rng(64)
    corner = [0, 1 << 59, M64, (1 << 64) - (1 << 32), 0xFFFFFFFF]
    v = [(a, h, c) for a in corner for h in corner for c in range(4)]
    # the fold's own wraps.  w1: al + EPS ah_hi passes 2^64;  w2: (al + EPS ah_hi + EPS w1)_hi + ah_lo passes 2^32
    alone = [(M64, 1 << 32),                  # w1 alone: t = EPS - 1 after the wrap, ah_lo = 0
             ((1 << 64) - (1 << 32), 1),      # w2 alone: ah_hi = 0, t_hi = 2^32 - 1, ah_lo = 1
             (M64, M64),                      # both, each at its maximum: t' = 2^64 - 2^32 - 1, hs = 2^33 - 3
             (1 << 63, (1 << 63) | 0x80000000),   # both, mid-range
             (M64, 0),                        # neither; r = 2^64 - 1, so r + EPS cl wraps in the correction
             (0, 0),                          # neither; r = 0, so r - ch borrows in the correction
             (P, 0), (P - 1, 0), (0xFFFFFFFF, 0), (0, 0xFFFFFFFF), (1, 0xFFFFFFFF), (0, 0xFFFFFFFF00000000)]
    v += [(a, h, c) for a, h in alone for c in range(4)]
    # what the rows of M^4 hand over at the all-ones state: the complete half-sums (2^32 - 1) (w_i + 1) with both carries
    m = [[CIRC[(j - i) % 12] + (DIAG[i] if i == j else 0) for j in range(12)] for i in range(12)]
    mul = lambda a, b: [[sum(a[i][t] * b[t][j] for t in range(12)) for j in range(12)] for i in range(12)]
    m2 = mul(m, m)
    m3 = mul(m2, m)
    m4 = mul(m3, m)
    for i in range(12):
        full = 0xFFFFFFFF * (sum(m4[i]) + m[i][0] + m2[i][0] + m3[i][0] + 1)
        assert 1 << 64 <= full < 1 << 65
        v.append((full & M64, full & M64, 3))
    v += [(int(a), int(h), int(c)) for a, h, c in zip(rng.integers(0, 1 << 64, 2000, dtype=np.uint64), rng.integers(0, 1 << 64, 2000, dtype=np.uint64),
                                                      rng.integers(0, 4, 2000))]
    return tuple(v)
