"""The I/O syscalls' rows on the host (test infrastructure): a Python restatement, in Python integers, of the four data-moving helpers
that generate_syscall calls behind its own row (witness/operation.rs:1660-1673) -- load_input (:1024-1067, SYSHINTREAD), commit
(:1069-1099, SYSWRITE to FD_PUBLIC_VALUES), verify (:991-1022, SYSVERIFY) and load_preimage (:908-989, SYSGETPID) -- the CPU rows a call
pushes, with the channel mask and the clock of each.  Everything the device makes of the same lists (zkm_io_calls_steps,
zkm_io_calls_witness) must equal this word for word; the model itself is held against hand-computed rows and the oracle's CPU
constraints in tests/test_io_calls_model.py.

A call is (kind, its bytes, meta {context, segment, address, timestamp of its first row}).  The bytes: the input-stream vector of a hint
read; the memory words a commit or a verify reads, as big-endian bytes; a preimage's 32 hash bytes and then the file's content.  The
reference's context is 0 and its segment Code; the model takes both from the meta.  The memory operations are those of the rows' channels
(the RAW steps push them): the helpers push no list of their own."""
import numpy as np

from . import cpu_fixtures as CF

HINT_READ, COMMIT, VERIFY, PREIMAGE = 0, 1, 2, 3
KINDS = {"hint_read": HINT_READ, "commit": COMMIT, "verify": VERIFY, "preimage": PREIMAGE}
PREIMAGE_HASH, PREIMAGE_MAP = 0x30001000, 0x31000000
WORD_SIZE, POSEIDON_RATE_BYTES = 4, 32


def be(b4):
    return int.from_bytes(bytes(b4), "big")


class Expansion:
    """What a list of calls pushes, in push order: rows (259-word lists) with masks and clocks."""

    def __init__(self):
        self.rows, self.masks, self.clocks = [], [], []

    def row(self, clock):
        r = [0] * CF.W                   # CpuColumnsView::default()
        r[CF.CLOCK] = clock
        self.rows.append(r)
        self.masks.append(0)
        self.clocks.append(clock)
        return r

    def channel(self, r, i, is_read, ctx, seg, virt, value):
        """mem_read_gp_with_log_and_fill / mem_write_gp_log_and_fill (util.rs:304-349): the channel's six cells; the operation itself is
        pushed by the row's RAW step."""
        assert 0 <= value < 1 << 32 and not r[CF.ch(i, 0)]
        r[CF.ch(i, 0)], r[CF.ch(i, 1)], r[CF.ch(i, 2)], r[CF.ch(i, 3)], r[CF.ch(i, 4)], r[CF.ch(i, 5)] = 1, is_read, ctx, seg, virt, value
        self.masks[-1] |= 1 << i

    # ---- load_input: the vector written to memory, eight words a row
    def hint_read(self, vec, meta):
        ctx, seg, addr, ts = (int(x) for x in meta)
        assert ts % 10 == 0 and addr % 4 == 0
        clock = ts // 10
        r, j = self.row(clock), 0
        for i in range(0, len(vec), 4):
            word = be((list(vec[i:i + 4]) + [0, 0, 0])[:4])           # right-padded with 0
            if j == 8:
                clock += 1
                r, j = self.row(clock), 0
            self.channel(r, j, 0, ctx, seg, addr + i, word)
            j += 1

    # ---- commit: the words read, eight a row
    def commit(self, words_be, meta):
        ctx, seg, addr, ts = (int(x) for x in meta)
        assert ts % 10 == 0 and len(words_be) % 4 == 0
        clock = ts // 10
        r, j = self.row(clock), 0
        for i in range(0, len(words_be), 4):
            if j == 8:
                clock += 1
                r, j = self.row(clock), 0
            self.channel(r, j, 1, ctx, seg, addr + i, be(words_be[i:i + 4]))
            j += 1

    # ---- verify: one row of eight reads
    def verify(self, digest, meta):
        ctx, seg, addr, ts = (int(x) for x in meta)
        assert ts % 10 == 0 and len(digest) == 32
        r = self.row(ts // 10)
        for i in range(8):
            self.channel(r, i, 1, ctx, seg, addr + 4 * i, be(digest[4 * i:4 * i + 4]))

    # ---- load_preimage: the hash read, then the length and the padded content written
    def preimage(self, data, meta):
        ctx, seg, addr, ts = (int(x) for x in meta)
        assert ts % 10 == 0 and len(data) >= 32 and addr == PREIMAGE_MAP
        hash_bytes, content = data[:32], data[32:]
        clock = ts // 10
        r = self.row(clock)
        for i in range(8):
            self.channel(r, i, 1, ctx, seg, PREIMAGE_HASH + 4 * i, be(hash_bytes[4 * i:4 * i + 4]))
        clock += 1
        r = self.row(clock)
        self.channel(r, 0, 0, ctx, seg, addr, len(content))
        map_addr, j = addr + 4, 1
        for i in range(0, len(content), WORD_SIZE):
            if j == 8:
                clock += 1
                r, j = self.row(clock), 0
            word = 0
            n = min(len(content) - i, WORD_SIZE)
            for k in range(n):
                word |= content[i + k] << (8 * k)
            if n < WORD_SIZE:
                end = len(content) % POSEIDON_RATE_BYTES
                word |= 1 << (8 * n)
                if end + 4 > POSEIDON_RATE_BYTES:
                    word |= 0b10000000 << 24
            self.channel(r, j, 0, ctx, seg, map_addr, int.from_bytes(word.to_bytes(4, "little"), "big"))      # word.to_be()
            map_addr += 4
            j += 1

    def call(self, kind, data, meta):
        data = bytes(bytearray(data))
        (self.hint_read, self.commit, self.verify, self.preimage)[kind](data, meta)

    # ---- as the device writes them
    def array(self):
        return np.array(self.rows, dtype=np.uint64).reshape(-1, CF.W)

    def memory_ops(self):
        return sum(bin(m).count("1") for m in self.masks)

    def channel_ops(self):
        """The memory operations the rows' RAW steps push: the masked channels in ascending order, at the row's own clock."""
        return [(r[CF.ch(i, 2)], r[CF.ch(i, 3)], r[CF.ch(i, 4)], r[CF.CLOCK] * 10, r[CF.ch(i, 1)], r[CF.ch(i, 5)])
                for r, mask in zip(self.rows, self.masks) for i in range(8) if (mask >> i) & 1]


def expand(kinds, data, off, meta):
    """All calls in list order: the rows of zkm_io_calls_witness."""
    x = Expansion()
    data, off = bytes(bytearray(np.asarray(data, dtype=np.uint8))), [int(o) for o in off]
    for k, (kind, m) in enumerate(zip(kinds, np.asarray(meta).reshape(-1, 4))):
        x.call(int(kind), data[off[k]:off[k + 1]], m)
    return x


def lists(calls):
    """[(kind, data bytes, meta)] as (kinds u32, data u8, data_off, meta n x 4)."""
    off = np.cumsum([0] + [len(d) for _, d, _ in calls]).astype(np.uint64)
    return (np.array([k for k, _, _ in calls], dtype=np.uint32), np.frombuffer(b"".join(bytes(bytearray(d)) for _, d, _ in calls), dtype=np.uint8).copy(),
            off, np.array([m for _, _, m in calls], dtype=np.uint64).reshape(-1, 4))


def steps(x, raw_base):
    """The RAW records of an Expansion's rows as zkm_io_calls_steps writes them: (kind 28, reads[0] = raw_base + j, reads[1] = mask)."""
    from .cpu_steps_model import KIND, STEP_DT
    out = np.zeros(len(x.rows), dtype=STEP_DT)
    out["kind"] = KIND["RAW"]
    out["reads"][:, 0] = raw_base + np.arange(len(x.rows))
    out["reads"][:, 1] = x.masks
    return out, np.array(x.clocks, dtype=np.uint64)


def row_count(kind, L):
    """The rows a call of L bytes pushes, counted from the generators' loops (not from the library's formulas)."""
    x = Expansion()
    x.call(kind, bytes(L), (0, 0, PREIMAGE_MAP if kind == PREIMAGE else 0x1000, 0))
    return len(x.rows)


# ---- a Machine run with calls spliced in at their clocks
from .keccak_calls_model import CallRecorder as _KeccakCallRecorder  # noqa: E402


class CallRecorder(_KeccakCallRecorder):
    """keccak_calls_model.CallRecorder with I/O calls: .io(kind, address, data) takes the clocks that follow the Machine's last row (the
    SYSCALL row, in a real program)."""

    def __init__(self, m):
        super().__init__(m)
        self.ios = []

    def io(self, kind, addr, data, ctx=0, seg=CF.SEG_CODE):
        kind = KINDS.get(kind, kind)
        data = bytes(bytearray(data))
        self.ios.append((kind, data, (ctx, seg, addr, 10 * self.m.clock)))
        self._reserve(row_count(kind, len(data)))

    def io_lists(self):
        return lists(self.ios) if self.ios else None

    def finish(self):
        """Fill the reserved rows from the models; returns (the SHA Expansion, the Keccak Expansion, the I/O Expansion)."""
        ix = expand(*self.io_lists()) if self.ios else Expansion()
        for r, clock in zip(ix.rows, ix.clocks):
            assert self.m.rows[clock] is None
            self.m.rows[clock] = r
        sx, kx = super().finish()
        return sx, kx, ix
