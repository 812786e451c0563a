"""CPU suite: SYSKECCAK calls of any byte length (ZKM_SPONGE_PADDED_TAIL) as far as they need no GPU -- the constant declared alike
everywhere, zkm_keccak_calls_counts_meta and zkm_keccak_calls_steps against tests/keccak_tail_model.py for every length at which the
last word, the read rows or the blocks take another shape, multiples of 4 unchanged with and without the flag, a segment's counts
through zkm_segment_calls_steps, and the refusals: a length that is no multiple of 4 without the flag in the words it always had, a
length of 0 whatever the flag says, and the address check on the last word of ceil(L / 4)."""
import ctypes as C
import re

import numpy as np
import pytest

from . import keccak_calls_model as K
from . import keccak_tail_fixtures as TF
from . import keccak_tail_model as TM
from .test_abi import declared_alike, prototypes, read
from .test_keccak_calls_abi import metas, offsets, witness_without_context

FLAG, TAIL = TM.FLAG, TM.TAIL
ODD = r"length %d is not a positive multiple of 4 \(the other bytes of the last memory word follow from no list"


def test_the_constant_and_the_export_are_declared_alike(zkm):
    declared_alike(zkm, "zkm_keccak_calls_counts_meta")
    assert all(ty != "zkm_ctx*" for ty, _ in prototypes()["zkm_keccak_calls_counts_meta"][1])           # pure: no context
    assert [arg for _, arg in prototypes()["zkm_keccak_calls_counts_meta"][1]][:3] == ["input_off", "meta", "ncalls"]
    assert zkm.SPONGE_PADDED_TAIL == TAIL == zkm.abi.constants()["ZKM_SPONGE_PADDED_TAIL"] == 1 << 62
    assert "pub const ZKM_SPONGE_PADDED_TAIL: u64 = 0x4000000000000000;" in read("integration", "rust", "zkm_hip_sys.rs")
    assert TAIL & FLAG == 0 and TAIL >> 32
    from .test_rust_names import call_arities, strip_comments
    src = strip_comments(read("integration", "rust", "keccak_calls_hip.rs"))
    assert set(call_arities(src, "zkm_keccak_calls_counts_meta")) == {len(prototypes()["zkm_keccak_calls_counts_meta"][1])}
    assert "ZKM_SPONGE_PADDED_TAIL" in src


@pytest.mark.parametrize("L", TM.LENGTHS)
def test_the_runtime_and_the_sponge_agree_on_the_last_word(L):
    """The model's two statements of the last memory word -- what the guest runtime writes (io.rs:128-144) and what the sponge's reads
    of the remainder carry (rem_data, util.rs:515-519) -- are one word, and it is the padded message's."""
    data = np.random.default_rng(L).integers(0, 256, L, dtype=np.uint8).tobytes()
    words, reads = TM.runtime_words(data), TM.sponge_read_words(data)
    assert len(reads) == L and len(words) == (L + 3) // 4
    assert all(reads[i] == words[i // 4] for i in range(L))
    padded = b"".join(K.padded_blocks(data))
    assert all(words[w] == K.be(padded[4 * w:4 * w + 4]) for w in range(len(words)))
    if L % 136 == 135:
        assert words[-1] & 0xFF == 0x81
    elif L % 4 and L % 136 > 132:
        assert words[-1] & 0xFF == 0x80


def flagged(lengths, base=None):
    m = metas(lengths) if base is None else base.copy()
    m[:, 2] |= np.uint64(TAIL)
    return m


@pytest.mark.parametrize("L", TM.LENGTHS)
def test_counts_masks_clocks_and_raw_indices_of_one_call_equal_the_model(zkm, L):
    off, meta = offsets([L], first=12), flagged([L])
    x = TM.Expansion()
    x.keccak(bytes(L), meta[0], 0x40000)
    rows, mem, logic, perms = zkm.keccak_calls_counts(off, meta)
    assert (rows, mem, logic, perms) == (len(x.rows), len(x.mem), len(x.logic), len(x.perm_ts)) == TM.counts([L])
    steps, clocks = zkm.keccak_calls_steps(off, meta, raw_base=5)
    want_steps, want_clocks = K.steps(x, raw_base=5)
    assert steps.tobytes() == want_steps.tobytes() and (clocks == want_clocks).all()
    W = (L + 3) // 4
    R = (W + 7) // 8
    assert clocks.tolist() == list(range(200 - R, 202))
    assert steps["reads"][:, 1].tolist() == [0xFF] * (R - 1) + [(1 << (W - 8 * (R - 1))) - 1, 0, 0xFF]
    assert steps["reads"][:, 0].tolist() == list(range(5, 5 + R + 2))


def test_all_lengths_in_one_list_equal_the_model(zkm):
    (inputs, off, meta, daddrs), want = TF.all_lengths()
    assert zkm.keccak_calls_counts(off, meta) == (want[0].shape[0], want[1].shape[0], want[2].shape[0], want[3].shape[0]) == TM.counts(TM.LENGTHS)
    steps, clocks = zkm.keccak_calls_steps(off, meta, raw_base=3)
    want_steps, want_clocks = K.steps(TM.expand(inputs, off, meta, daddrs), raw_base=3)
    assert steps.tobytes() == want_steps.tobytes() and (clocks == want_clocks).all()
    # the export itself, with any out pointer NULL; without metas it is zkm_keccak_calls_counts
    lib, err = zkm.load(), C.c_char_p()
    assert lib.zkm_keccak_calls_counts_meta(off.ctypes.data, meta.ctypes.data, len(meta), None, None, None, None, C.byref(err)) == 0
    assert lib.zkm_keccak_calls_counts_meta(off.ctypes.data, None, len(meta), None, None, None, None, C.byref(err)) == 1
    assert re.match("^zkm_keccak_calls_counts: input_off: call 0: " + ODD % 1, err.value.decode())
    assert lib.zkm_keccak_calls_counts_meta(None, None, 0, None, None, None, None, None) == 0


@pytest.mark.parametrize("lengths", [[4], [32, 36, 132], [136, 140, 272]])
def test_multiples_of_4_are_unchanged_with_and_without_the_flag(zkm, lengths):
    off, plain = offsets(lengths, first=8), metas(lengths)
    want = zkm.keccak_calls_counts(off)
    want_steps, want_clocks = zkm.keccak_calls_steps(off, plain, raw_base=2)
    out, err = [C.c_size_t() for _ in range(4)], C.c_char_p()
    for meta in (plain, flagged(lengths)):
        assert zkm.keccak_calls_counts(off, meta) == want
        steps, clocks = zkm.keccak_calls_steps(off, meta, raw_base=2)
        assert steps.tobytes() == want_steps.tobytes() and (clocks == want_clocks).all()
    assert zkm.load().zkm_keccak_calls_counts_meta(off.ctypes.data, None, len(lengths), *[C.byref(x) for x in out], C.byref(err)) == 0
    assert tuple(x.value for x in out) == want
    x = K.expand(np.zeros(int(off[-1]), dtype=np.uint8), off, plain, [0x40000] * len(lengths))
    y = TM.expand(np.zeros(int(off[-1]), dtype=np.uint8), off, flagged(lengths), [0x40000] * len(lengths))
    for a, b in zip(x.arrays(), y.arrays()):                                  # and the two models are one on these lengths
        assert (a == b).all()


def test_a_segment_with_flagged_calls_counts_as_the_model(zkm):
    s = TF.segment(zkm)
    kx = s["model"]
    patched, counts = zkm.segment_calls_steps(zkm.SegmentCalls(**s["kw"]))
    rows, mem, logic, perms = TM.counts(TF.SEGMENT_LENGTHS)
    assert (counts["keccak_rows"], counts["memory_ops"], counts["logic_ops"], counts["keccak_perms"]) == (rows, mem, logic, perms)
    assert (len(kx.rows), len(kx.mem), len(kx.logic), len(kx.perm_ts)) == (rows, mem, logic, perms)
    assert counts["nraw"] == s["kw"]["steps"].nraw + rows and counts["sha_rows"] == counts["io_rows"] == counts["insn_rows"] == 0
    assert patched.tobytes() == s["host"][0].steps.tobytes()                   # the records, at the model's clocks
    assert [int(m[2]) >> 62 for m in s["kw"]["keccak"][2]] == [3, 3, 3, 3] and s["log_n"] <= 10


def test_every_entry_refuses_an_unflagged_length_in_the_words_it_always_had(zkm):
    from .test_calls_entry_abi import expand_without_a_context
    lengths = [8, 35, 8]
    off, meta, daddrs = offsets(lengths), metas(lengths), np.array([0x2000, 0x2040, 0x2080], dtype=np.uint64)
    at = "input_off: call 1: " + ODD % 35
    with pytest.raises(zkm.ZkmError, match="^zkm_keccak_calls_counts: " + at):
        zkm.keccak_calls_counts(off)
    with pytest.raises(zkm.ZkmError, match="^zkm_keccak_calls_counts: " + at):
        zkm.keccak_calls_counts(off, meta)
    steps, clocks, err = np.zeros(64, dtype=zkm.CPU_STEP_DT), np.zeros(64, dtype=np.uint64), C.c_char_p()
    assert zkm.load().zkm_keccak_calls_steps(off.ctypes.data, meta.ctypes.data, 3, 0, steps.ctypes.data, clocks.ctypes.data, C.byref(err)) == 1
    assert re.match("^zkm_keccak_calls_steps: " + at, err.value.decode()) and not steps["kind"].any()
    assert re.match("^zkm_keccak_calls_witness: " + at, witness_without_context(zkm, off, meta, daddrs))
    # the flag on another call does not carry over
    other = meta.copy()
    other[0, 2] |= np.uint64(TAIL)
    other[2, 2] |= np.uint64(TAIL)
    assert re.match("^zkm_keccak_calls_witness: " + at, witness_without_context(zkm, off, other, daddrs))
    # with the flag, the same lists pass every host check: the missing context is what is left
    meta[1, 2] |= np.uint64(TAIL)
    assert witness_without_context(zkm, off, meta, daddrs) == "zkm_keccak_calls_witness: null argument"
    # a segment: the flag taken off one call of the recorded segment
    kw = dict(TF.segment(zkm)["kw"])
    k = kw["keccak"]
    bare = k[2].copy()
    bare[1, 2] &= ~np.uint64(TAIL)
    bad = zkm.SegmentCalls(**dict(kw, keccak=(k[0], k[1], bare, k[3])))
    message = "zkm_keccak_calls_counts: input_off: call 1: " + ODD % 135
    with pytest.raises(zkm.ZkmError, match="^zkm_segment_calls_steps: " + message):
        zkm.segment_calls_steps(bad)
    assert re.match("^zkm_segments_calls_expand: segment 1: " + message, expand_without_a_context(zkm, [zkm.SegmentCalls(**kw), bad]))


def test_a_length_of_zero_is_refused_with_the_flag(zkm):
    lengths = [8, 0, 8]
    off, meta, daddrs = offsets(lengths), flagged(lengths), np.array([0x2000, 0x2040, 0x2080], dtype=np.uint64)
    at = "input_off: call 1: length 0 is not a positive multiple of 4"
    with pytest.raises(zkm.ZkmError, match="^zkm_keccak_calls_counts: " + at):
        zkm.keccak_calls_counts(off, meta)
    with pytest.raises(zkm.ZkmError, match="^zkm_keccak_calls_(steps|counts): " + at):
        zkm.keccak_calls_steps(off, meta)
    assert re.match("^zkm_keccak_calls_witness: " + at, witness_without_context(zkm, off, meta, daddrs))


def test_the_address_check_is_on_the_last_word_of_ceil(zkm):
    """9 bytes are three words: with word 0 at 0xFFFFFFF8 the third lies at 2^32; two words (5 .. 8 bytes) still fit."""
    daddrs = np.array([0x2000], dtype=np.uint64)
    for L, fits in ((5, True), (8, True), (9, False), (12, False)):
        off = offsets([L])
        meta = np.array([(0, 0, 0xFFFFFFF8 | FLAG | TAIL, 100)], dtype=np.uint64)
        got = witness_without_context(zkm, off, meta, daddrs)
        if fits:
            assert got == "zkm_keccak_calls_witness: null argument", (L, got)
            zkm.keccak_calls_steps(off, meta)
        else:
            assert got == "zkm_keccak_calls_witness: meta: call 0: address of word 0 0xfffffff8: word 2 does not fit in 32 bits", (L, got)
            with pytest.raises(zkm.ZkmError, match="^zkm_keccak_calls_steps: meta: call 0: address of word 0 0xfffffff8: word 2 does not fit"):
                zkm.keccak_calls_steps(off, meta)
    # the flag is no part of the address
    meta = np.array([(0, 0, (1 << 32) | FLAG | TAIL, 100)], dtype=np.uint64)
    assert "address of word 0 0x100000000: word 1 does not fit in 32 bits" in witness_without_context(zkm, offsets([5]), meta, daddrs)
    # the smallest timestamp counts the read rows of ceil: 33 bytes are nine words, two read rows
    meta = np.array([(0, 0, 0x1000 | FLAG | TAIL, 10)], dtype=np.uint64)
    assert "timestamp 10 puts the first read row before clock 0" in witness_without_context(zkm, offsets([33]), meta, daddrs)
    meta[0, 3] = 20
    assert zkm.keccak_calls_steps(offsets([33]), meta)[1].tolist() == [0, 1, 2, 3]
