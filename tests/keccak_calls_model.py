"""The SYSKECCAK precompile calls on the host (test infrastructure): a Python restatement of generate_keccak (witness/operation.rs:1101-1181)
and of its helper keccak_sponge_log (witness/util.rs:471-557, with xor_into_sponge, :724-741) in Python integers, with a Keccak-f of its
own -- the CPU rows a call pushes, with the channel mask and the clock of each, and the lists the helper pushes: the sponge's memory
reads, the XORs of every absorption, the Keccak-f inputs and timestamps.  Everything the device makes of the same lists
(zkm_keccak_calls_steps, zkm_keccak_calls_witness) must equal this word for word; the model itself is held against the Keccak-f test
vectors, the oracle's KeccakSponge table and the oracle's CPU constraints in tests/test_keccak_calls_model.py.

A call is described as the KeccakSponge table takes it -- its input bytes and meta {context, segment, address of word 0 with
ZKM_SPONGE_BYTE_ADDRESSED set, timestamp of the sponge row} -- and the address its digest is written to.  The reference's context is 0
and its segment Code; the model takes both from the meta.  Lengths are positive multiples of 4 (include/zkm_hip.h says why)."""
import numpy as np

from . import cpu_fixtures as CF

M64 = (1 << 64) - 1
XOR = 2                              # zkm_logic_trace's code
IS_KECCAK_SPONGE = 83
FLAG = 1 << 63                       # ZKM_SPONGE_BYTE_ADDRESSED
RATE, RATE_U32 = 136, 34


# ---- Keccak-f[1600] from FIPS 202: the round constants from the LFSR, the rotation offsets from the (x, y) walk
def _round_constants():
    out, r = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            r = ((r << 1) ^ ((r >> 7) * 0x71)) & 0xFF
            if r & 2:
                rc |= 1 << ((1 << j) - 1)
        out.append(rc)
    return out


def _rotations():
    rot, (x, y) = [[0] * 5 for _ in range(5)], (1, 0)
    for t in range(24):
        rot[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rot


RC, ROT = _round_constants(), _rotations()


def rol(v, n):
    return ((v << n) | (v >> (64 - n))) & M64 if n else v


def keccakf(state):
    """state: 25 lanes, A(x, y) = state[5 y + x]; returns the permuted state."""
    a = [[state[5 * y + x] for y in range(5)] for x in range(5)]
    for rc in RC:
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x - 1) % 5] ^ rol(c[(x + 1) % 5], 1) for x in range(5)]
        a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
        b = [[0] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = rol(a[x][y], ROT[x][y])
        a = [[b[x][y] ^ (~b[(x + 1) % 5][y] & M64 & b[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        a[0][0] ^= rc
    return [a[x][y] for y in range(5) for x in range(5)]


def be(b4):
    return int.from_bytes(bytes(b4), "big")


def padded_blocks(data):
    """The input in 136-byte blocks, the last one (possibly holding nothing else) with pad10*1."""
    B = len(data) // RATE + 1
    p = bytearray(data) + bytearray(RATE * B - len(data))
    p[len(data)] |= 0x01
    p[-1] |= 0x80
    return [bytes(p[RATE * b:RATE * (b + 1)]) for b in range(B)]


class Expansion:
    """What a list of calls pushes, in push order: rows (259-word lists) with masks and clocks, mem (the sponge's reads: context,
    segment, virt, timestamp, is_read, value), logic (op, in0, in1), perm_inputs (25 words), perm_ts; digests (32 bytes a call)."""

    def __init__(self):
        self.rows, self.masks, self.clocks, self.mem, self.logic, self.perm_inputs, self.perm_ts, self.digests = [], [], [], [], [], [], [], []

    def row(self, clock):
        r = [0] * CF.W                   # CpuColumnsView::default()
        r[CF.CLOCK] = clock
        self.rows.append(r)
        self.masks.append(0)
        self.clocks.append(clock)
        return r

    def channel(self, r, i, is_read, ctx, seg, virt, value):
        r[CF.ch(i, 0)], r[CF.ch(i, 1)], r[CF.ch(i, 2)], r[CF.ch(i, 3)], r[CF.ch(i, 4)], r[CF.ch(i, 5)] = 1, is_read, ctx, seg, virt, value
        self.masks[-1] |= 1 << i

    # ---- keccak_sponge_log: the reads, the absorptions; returns the digest
    def sponge(self, data, ctx, seg, addrs, ts):
        for i in range(len(data)):                                 # one read a byte, of the word that holds it
            w = i // 4
            self.mem.append((ctx, seg, addrs[w], ts, 1, be(data[4 * w:4 * w + 4])))
        state = [0] * 25
        for block in padded_blocks(data):
            for i in range(RATE_U32):                              # xor_into_sponge
                lhs = (state[i // 2] >> (32 * (i & 1))) & 0xFFFFFFFF
                self.logic.append((XOR, lhs, int.from_bytes(block[4 * i:4 * i + 4], "little")))
            for i in range(RATE // 8):
                state[i] ^= int.from_bytes(block[8 * i:8 * i + 8], "little")
            self.perm_inputs.append(list(state))
            self.perm_ts.append(ts)
            state = keccakf(state)
        return b"".join(v.to_bytes(8, "little") for v in state[:4])

    # ---- generate_keccak
    def keccak(self, data, meta, digest_addr):
        ctx, seg, base, ts = (int(x) for x in meta)
        assert base & FLAG and ts % 10 == 0 and len(data) % 4 == 0 and len(data) > 0
        base &= ~FLAG
        data = bytes(bytearray(data))
        L, W = len(data), len(data) // 4
        R = (W + 7) // 8
        clock = ts // 10 - R
        addrs = [base + 4 * w for w in range(W)]
        for w in range(W):
            if w % 8 == 0:
                r = self.row(clock)
                clock += 1
            self.channel(r, w % 8, 1, ctx, seg, addrs[w], be(data[4 * w:4 * w + 4]))
        assert clock == ts // 10
        r = self.row(clock)
        r[IS_KECCAK_SPONGE] = 1
        final = L // RATE * RATE_U32
        r[CF.ch(0, 5)], r[CF.ch(1, 5)], r[CF.ch(2, 5)], r[CF.ch(3, 5)] = ctx, seg, (addrs[final] if final < W else 0), L
        digest = self.sponge(data, ctx, seg, addrs, ts)
        words = [be(digest[4 * i:4 * i + 4]) for i in range(8)]
        for i in range(8):
            r[CF.GEN + i] = words[7 - i]                           # general.khash.value, reversed
        clock += 1
        r = self.row(clock)
        for i in range(8):
            self.channel(r, i, 0, ctx, seg, digest_addr + 4 * i, words[i])
        self.digests.append(digest)
        return digest

    # ---- as the device writes them
    def arrays(self):
        return (np.array(self.rows, dtype=np.uint64).reshape(-1, CF.W), np.array(self.mem, dtype=np.uint64).reshape(-1, 6),
                np.array(self.logic, dtype=np.uint32).reshape(-1, 3), np.array(self.perm_inputs, dtype=np.uint64).reshape(-1, 25),
                np.array(self.perm_ts, dtype=np.uint64))


def expand(inputs, off, meta, digest_addrs):
    """All calls in list order: the lists of zkm_keccak_calls_witness."""
    x = Expansion()
    data, off = bytes(bytearray(np.asarray(inputs, dtype=np.uint8))), [int(o) for o in off]
    for k, (m, d) in enumerate(zip(np.asarray(meta).reshape(-1, 4), digest_addrs)):
        x.keccak(data[off[k]:off[k + 1]], m, int(d))
    return x


def lists(calls):
    """[(data bytes, meta, digest_addr)] as (inputs u8, off, meta n x 4, digest_addrs)."""
    off = np.cumsum([0] + [len(d) for d, _, _ in calls]).astype(np.uint64)
    return (np.frombuffer(b"".join(bytes(bytearray(d)) for d, _, _ in calls), dtype=np.uint8).copy(), off,
            np.array([m for _, m, _ in calls], dtype=np.uint64).reshape(-1, 4), np.array([a for _, _, a in calls], dtype=np.uint64))


def steps(x, raw_base):
    """The RAW records of an Expansion's rows as zkm_keccak_calls_steps writes them: (kind 28, reads[0] = raw_base + j, reads[1] = mask)."""
    from .cpu_steps_model import KIND, STEP_DT
    out = np.zeros(len(x.rows), dtype=STEP_DT)
    out["kind"] = KIND["RAW"]
    out["reads"][:, 0] = raw_base + np.arange(len(x.rows))
    out["reads"][:, 1] = x.masks
    return out, np.array(x.clocks, dtype=np.uint64)


def call_bytes(L):
    """What one call of L input bytes costs the link host-expanded: (CPU rows, sponge reads, XORs, Keccak-f inputs with timestamps)."""
    W = L // 4
    return ((W + 7) // 8 + 2) * CF.W * 8, L * 48, 34 * (L // RATE + 1) * 12, (L // RATE + 1) * 208


# ---- a Machine run with calls spliced in at their clocks
from .sha_calls_model import CallRecorder as _ShaCallRecorder  # noqa: E402


class CallRecorder(_ShaCallRecorder):
    """sha_calls_model.CallRecorder with SYSKECCAK calls: .keccak(addr, data, ptr) takes the clocks that follow the Machine's last row."""

    def __init__(self, m):
        super().__init__(m)
        self.keccaks = []

    def keccak(self, addr, data, ptr, ctx=0, seg=CF.SEG_CODE):
        data = bytes(bytearray(data))
        R = (len(data) // 4 + 7) // 8
        self.keccaks.append((data, (ctx, seg, addr | FLAG, 10 * (self.m.clock + R)), ptr))
        self._reserve(R + 2)

    def keccak_lists(self):
        return lists(self.keccaks) if self.keccaks else None

    def finish(self):
        """Fill the reserved rows from the models; returns (the SHA Expansion, the Keccak Expansion)."""
        from . import sha_calls_model as S
        sx, kx = S.expand(*self.lists()), expand(*self.keccak_lists()) if self.keccaks else Expansion()
        for x in (sx, kx):
            for r, clock in zip(x.rows, x.clocks):
                assert self.m.rows[clock] is None
                self.m.rows[clock] = r
        assert all(r is not None for r in self.m.rows)
        return sx, kx
