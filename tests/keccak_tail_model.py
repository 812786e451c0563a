"""SYSKECCAK calls of ANY positive length on the host (test infrastructure): generate_keccak (witness/operation.rs:1101-1181) and
keccak_sponge_log (witness/util.rs:471-557) restated once more for lengths that are no multiple of 4, from the reference's text.  What
differs from tests/keccak_calls_model.py (whose Keccak-f and block padding -- held to golden/keccakf_kat.json -- are reused) is the
call's last memory word:

  * generate_keccak reads ceil(len / 4) words from memory (:1118-1134) and copies only the first len - i bytes of the last one into the
    hashed input.  What memory holds there is what the guest runtime wrote (runtime/precompiles/src/io.rs:128-144): the remaining
    bytes, 0x01, zeros, and 0x80 ORed into the fourth byte when len % 136 + 4 > 136 (`runtime_words`);
  * keccak_sponge_log reads, for every byte of the remainder, the aligned word of rem_data (:515-519: the remainder, rem_data[rem.len()]
    = 1, rem_data[135] |= 0x80) and for every byte of a full block the aligned word of the block (`Expansion.sponge`).

Both give the same word (tests/test_keccak_tail_abi.py checks it for every length the suites use), which is why a recorder may vouch
for it with ZKM_SPONGE_PADDED_TAIL.  Nothing here calls the library's placement code."""
import numpy as np

from . import cpu_fixtures as CF
from . import keccak_calls_model as K

FLAG, TAIL = K.FLAG, 1 << 62         # ZKM_SPONGE_BYTE_ADDRESSED, ZKM_SPONGE_PADDED_TAIL
RATE, RATE_U32 = K.RATE, K.RATE_U32
LENGTHS = [1, 2, 3, 5, 31, 33, 133, 134, 135, 136, 137, 139, 271, 273]


def runtime_words(data):
    """The u32 words the guest runtime hands to the syscall (io.rs:128-144), as memory holds them."""
    n, out = len(data), []
    for i in range(0, n, 4):
        if i + 4 <= n:
            out.append(K.be(data[i:i + 4]))
        else:
            chunk = bytearray(4)
            chunk[:n - i] = data[i:]
            chunk[n - i] = 1
            if n % RATE + 4 > RATE:
                chunk[3] |= 0x80
            out.append(K.be(chunk))
    return out


def sponge_read_words(data):
    """The value of each of the sponge's len(data) reads (util.rs:488-505 for the full blocks, :513-535 for the remainder)."""
    full = len(data) // RATE * RATE
    out = []
    for start in range(0, full, RATE):
        block = data[start:start + RATE]
        for i in range(RATE):
            align = i // 4 * 4
            out.append(K.be(block[align:align + 4]))       # u32::from_le_bytes(..).to_be(): the bytes in memory order
    rem = data[full:]
    rem_data = bytearray(RATE)
    rem_data[:len(rem)] = rem
    rem_data[len(rem)] = 1
    rem_data[RATE - 1] |= 0x80
    for i in range(len(rem)):
        align = i // 4 * 4
        out.append(K.be(rem_data[align:align + 4]))
    return out


class Expansion(K.Expansion):
    """K.Expansion for calls of any positive length."""

    def sponge(self, data, ctx, seg, addrs, ts):
        for i, value in enumerate(sponge_read_words(data)):       # one read a byte, at base_address[absorbed_bytes / 4]
            self.mem.append((ctx, seg, addrs[i // 4], ts, 1, value))
        state = [0] * 25
        for block in K.padded_blocks(data):
            for i in range(RATE_U32):                              # xor_into_sponge
                lhs = (state[i // 2] >> (32 * (i & 1))) & 0xFFFFFFFF
                self.logic.append((K.XOR, lhs, int.from_bytes(block[4 * i:4 * i + 4], "little")))
            for i in range(RATE // 8):
                state[i] ^= int.from_bytes(block[8 * i:8 * i + 8], "little")
            self.perm_inputs.append(list(state))
            self.perm_ts.append(ts)
            state = K.keccakf(state)
        return b"".join(v.to_bytes(8, "little") for v in state[:4])

    def keccak(self, data, meta, digest_addr, memory=None):
        """memory: the words the call reads (default: what the runtime wrote)."""
        ctx, seg, base, ts = (int(x) for x in meta)
        data = bytes(bytearray(data))
        L = len(data)
        assert base & FLAG and ts % 10 == 0 and L > 0 and (L % 4 == 0 or base & TAIL)
        base &= ~(FLAG | TAIL)
        words = runtime_words(data) if memory is None else list(memory)
        W = len(words)
        assert W == (L + 3) // 4
        R = (W + 7) // 8
        clock = ts // 10 - R
        addrs = [base + 4 * w for w in range(W)]
        hashed = bytearray(L)
        for w in range(W):                                         # for i in (0..len).step_by(WORD_SIZE)
            if w % 8 == 0:
                r = self.row(clock)
                clock += 1
            self.channel(r, w % 8, 1, ctx, seg, addrs[w], words[w])
            final_len = min(4, L - 4 * w)
            hashed[4 * w:4 * w + final_len] = words[w].to_bytes(4, "big")[:final_len]
        assert clock == ts // 10 and bytes(hashed) == data
        r = self.row(clock)
        r[K.IS_KECCAK_SPONGE] = 1
        final = L // RATE * RATE_U32
        r[CF.ch(0, 5)], r[CF.ch(1, 5)], r[CF.ch(2, 5)], r[CF.ch(3, 5)] = ctx, seg, (addrs[final] if final < W else 0), L
        digest = self.sponge(data, ctx, seg, addrs, ts)
        out = [K.be(digest[4 * i:4 * i + 4]) for i in range(8)]
        for i in range(8):
            r[CF.GEN + i] = out[7 - i]                             # general.khash.value, reversed
        clock += 1
        r = self.row(clock)
        for i in range(8):
            self.channel(r, i, 0, ctx, seg, digest_addr + 4 * i, out[i])
        self.digests.append(digest)
        return digest


def expand(inputs, off, meta, digest_addrs, memories=None):
    """All calls in list order: the lists of zkm_keccak_calls_witness.  memories: per call, the words it reads (None: the runtime's)."""
    x = Expansion()
    data, off = bytes(bytearray(np.asarray(inputs, dtype=np.uint8))), [int(o) for o in off]
    for k, (m, d) in enumerate(zip(np.asarray(meta).reshape(-1, 4), digest_addrs)):
        x.keccak(data[off[k]:off[k + 1]], m, int(d), memory=memories[k] if memories else None)
    return x


def counts(lengths):
    """(cpu_rows, memory_ops, logic_ops, keccak_perms) of calls of these lengths, from the reference's loops: a read row every eight words
    of ceil(L / 4), one sponge read a byte, 34 XORs and one permutation a block of L / 136 + 1."""
    rows = sum((((L + 3) // 4) + 7) // 8 + 2 for L in lengths)
    blocks = sum(L // RATE + 1 for L in lengths)
    return rows, sum(lengths), RATE_U32 * blocks, blocks


def call_bytes(L):
    """What one call of L input bytes costs the link host-expanded: (CPU rows, sponge reads, XORs, Keccak-f inputs with timestamps)."""
    W = (L + 3) // 4
    return ((W + 7) // 8 + 2) * CF.W * 8, L * 48, 34 * (L // RATE + 1) * 12, (L // RATE + 1) * 208


class CallRecorder(K.CallRecorder):
    """keccak_calls_model.CallRecorder for calls of any length: R from ceil(L / 4) words, ZKM_SPONGE_PADDED_TAIL on a call whose length is
    no multiple of 4 (flag_all: on every call), the Keccak rows from this module's Expansion."""

    def __init__(self, m, flag_all=False):
        super().__init__(m)
        self.flag_all = flag_all

    def keccak(self, addr, data, ptr, ctx=0, seg=CF.SEG_CODE):
        data = bytes(bytearray(data))
        R = ((len(data) + 3) // 4 + 7) // 8
        tail = TAIL if len(data) % 4 or self.flag_all else 0
        self.keccaks.append((data, (ctx, seg, addr | FLAG | tail, 10 * (self.m.clock + R)), ptr))
        self._reserve(R + 2)

    def finish(self, memories=None):
        """Fill the reserved rows from the models; returns (the SHA Expansion, the Keccak Expansion)."""
        from . import sha_calls_model as S
        sx = S.expand(*self.lists())
        kx = expand(*self.keccak_lists(), memories=memories) if self.keccaks else Expansion()
        for x in (sx, kx):
            for r, clock in zip(x.rows, x.clocks):
                assert self.m.rows[clock] is None
                self.m.rows[clock] = r
        assert all(r is not None for r in self.m.rows)
        return sx, kx
