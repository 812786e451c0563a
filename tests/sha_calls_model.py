"""The SHA-256 precompile calls on the host (test infrastructure): a Python restatement of generate_sha_extend and generate_sha_compress
(witness/operation.rs:1183-1285, :1298-1458) and of their helpers sha_extend_sponge_log and sha_compress_sponge_log
(witness/util.rs:559-694) -- the CPU rows a call pushes, with the channel mask and the clock of each, and the lists the helpers push: the
sponge's memory reads, the logic operations, the ShaExtend inputs and timestamps.  Everything the device makes of the same lists
(zkm_sha_calls_steps, zkm_sha_calls_witness) must equal this word for word; the model itself is held against the sponge fixtures and the
oracle's CPU constraints in tests/test_sha_calls_model.py.

A call is described as the sponge tables take it: extend = w[0..16] and meta {context, segment, address of w[0], timestamp of round 0's
sponge row}; compress = hx[0..8], w[0..64] and meta {context, segment, address of hx[0], timestamp, address of w[0], segment of w,
context of w, unused}.  The reference's context is 0 and its segment Code; the model takes both from the meta."""
import numpy as np

from . import cpu_fixtures as CF

M32 = 0xFFFFFFFF
AND, XOR = 0, 2                      # zkm_logic_trace's codes
IS_SHA_EXTEND_SPONGE, IS_SHA_COMPRESS_SPONGE = 84, 85
K = [0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
     0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
     0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
     0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
     0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
     0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]


def ror(x, r):
    return ((x >> r) | (x << (32 - r))) & M32


class Expansion:
    """What a list of calls pushes, in push order: rows (259-word lists) with masks and clocks, mem (the sponge's reads: context,
    segment, virt, timestamp, is_read, value), logic (op, in0, in1), ext_inputs (16 bytes), ext_ts."""

    def __init__(self):
        self.rows, self.masks, self.clocks, self.mem, self.logic, self.ext_inputs, self.ext_ts = [], [], [], [], [], [], []

    def row(self, clock):
        r = [0] * CF.W                   # CpuColumnsView::default()
        r[CF.CLOCK] = clock
        self.rows.append(r)
        self.masks.append(0)
        self.clocks.append(clock)
        return r

    def channel(self, r, i, is_read, ctx, seg, virt, value):
        """mem_read_gp_with_log_and_fill / mem_write_gp_log_and_fill: the channel's six cells; the operation itself is pushed by the
        row's RAW step."""
        r[CF.ch(i, 0)], r[CF.ch(i, 1)], r[CF.ch(i, 2)], r[CF.ch(i, 3)], r[CF.ch(i, 4)], r[CF.ch(i, 5)] = 1, is_read, ctx, seg, virt, value
        self.masks[-1] |= 1 << i

    def read4(self, ctx, seg, virt, ts, value):
        self.mem += [(ctx, seg, virt, ts, 1, value)] * 4

    # ---- generate_sha_extend + sha_extend_sponge_log
    def extend(self, w16, meta):
        ctx, seg, addr, ts = (int(x) for x in meta)
        assert ts % 10 == 0
        w = [int(x) for x in w16] + [0] * 48
        clock = ts // 10 - 1
        for i in range(16, 64):
            r = self.row(clock)
            srcs = (i - 15, i - 2, i - 16, i - 7)
            for ch, j in enumerate(srcs):
                self.channel(r, ch, 1, ctx, seg, addr + 4 * j, w[j])
            w15, w2 = w[i - 15], w[i - 2]
            s0_inter = ror(w15, 7) ^ ror(w15, 18)
            self.logic.append((XOR, ror(w15, 7), ror(w15, 18)))
            s0 = s0_inter ^ (w15 >> 3)
            self.logic.append((XOR, s0_inter, w15 >> 3))
            s1_inter = ror(w2, 17) ^ ror(w2, 19)
            self.logic.append((XOR, ror(w2, 17), ror(w2, 19)))
            s1 = s1_inter ^ (w2 >> 10)
            self.logic.append((XOR, s1_inter, w2 >> 10))
            w[i] = (s1 + w[i - 16] + s0 + w[i - 7]) & M32
            self.channel(r, 4, 0, ctx, seg, addr + 4 * i, w[i])
            clock += 1
            r = self.row(clock)
            r[IS_SHA_EXTEND_SPONGE] = 1
            r[CF.ch(0, 5)], r[CF.ch(1, 5)], r[CF.ch(2, 5)] = ctx, seg, addr + 4 * i
            r[CF.GEN] = w[i]                                   # general.element.value
            for j in srcs:                                     # sha_extend_sponge_log, at this row's clock
                self.read4(ctx, seg, addr + 4 * j, clock * 10, w[j])
            self.ext_inputs.append([b for j in srcs for b in w[j].to_bytes(4, "little")])
            self.ext_ts.append(clock * 10)
            clock += 1
        return w

    # ---- generate_sha_compress + sha_compress_sponge_log
    def compress(self, hx, w, meta):
        hctx, hseg, haddr, ts, waddr, wseg, wctx = (int(x) for x in meta[:7])
        assert ts % 10 == 0
        hx, w = [int(x) for x in hx], [int(x) for x in w]
        clock = ts // 10 - 9
        r = self.row(clock)
        for q in range(8):
            self.channel(r, q, 1, hctx, hseg, haddr + 4 * q, hx[q])
        clock += 1
        a, b, c, d, e, f, g, h = hx
        logic = []
        for i in range(64):
            if i % 8 == 0:
                r = self.row(clock)
                clock += 1
            self.channel(r, i % 8, 1, wctx, wseg, waddr + 4 * i, w[i])
            s1_inter = ror(e, 6) ^ ror(e, 11)
            s1 = s1_inter ^ ror(e, 25)
            e_not = ~e & M32
            ch = (e & f) ^ (e_not & g)
            t1 = (h + s1 + ch + K[i] + w[i]) & M32
            s0_inter = ror(a, 2) ^ ror(a, 13)
            s0 = s0_inter ^ ror(a, 22)
            maj_inter = (a & b) ^ (a & c)
            maj = maj_inter ^ (b & c)
            t2 = (s0 + maj) & M32
            logic += [(XOR, ror(e, 6), ror(e, 11)), (XOR, s1_inter, ror(e, 25)), (AND, e, f), (AND, e_not, g), (XOR, e & f, e_not & g),
                      (XOR, ror(a, 2), ror(a, 13)), (XOR, s0_inter, ror(a, 22)), (AND, a, b), (AND, a, c), (AND, b, c), (XOR, a & b, a & c),
                      (XOR, maj_inter, b & c)]
            a, b, c, d, e, f, g, h = (t1 + t2) & M32, a, b, c, (d + t1) & M32, e, f, g
        self.logic += logic
        out = [(x + y) & M32 for x, y in zip(hx, (a, b, c, d, e, f, g, h))]
        assert clock == ts // 10
        r = self.row(clock)
        r[IS_SHA_COMPRESS_SPONGE] = 1
        r[CF.ch(0, 5)], r[CF.ch(1, 5)], r[CF.ch(2, 5)] = hctx, hseg, haddr
        for q in range(8):
            r[CF.GEN + q] = out[q]                             # general.shash.value
        for q in range(8):                                     # sha_compress_sponge_log, at the sponge row's clock
            self.read4(hctx, hseg, haddr + 4 * q, ts, hx[q])
        for i in range(64):
            self.read4(wctx, wseg, waddr + 4 * i, ts, w[i])
        clock += 1
        r = self.row(clock)
        for q in range(8):
            self.channel(r, q, 0, hctx, hseg, haddr + 4 * q, out[q])
        return out

    # ---- as the device writes them
    def arrays(self):
        return (np.array(self.rows, dtype=np.uint64).reshape(-1, CF.W), np.array(self.mem, dtype=np.uint64).reshape(-1, 6),
                np.array(self.logic, dtype=np.uint32).reshape(-1, 3), np.array(self.ext_inputs, dtype=np.uint8).reshape(-1, 16),
                np.array(self.ext_ts, dtype=np.uint64))

    def channel_ops(self):
        """The memory operations the rows' RAW steps push: the masked channels in ascending order, at the row's own clock."""
        return [(r[CF.ch(i, 2)], r[CF.ch(i, 3)], r[CF.ch(i, 4)], r[CF.CLOCK] * 10, r[CF.ch(i, 1)], r[CF.ch(i, 5)])
                for r, mask in zip(self.rows, self.masks) for i in range(8) if (mask >> i) & 1]


def expand(extend=None, compress=None):
    """All extend calls in list order, then all compress calls: extend = (w16 n x 16, meta n x 4), compress = (hx, w, meta n x 8)."""
    x = Expansion()
    if extend is not None:
        for w16, meta in zip(np.asarray(extend[0]).reshape(-1, 16), np.asarray(extend[1]).reshape(-1, 4)):
            x.extend(w16, meta)
    if compress is not None:
        for hx, w, meta in zip(np.asarray(compress[0]).reshape(-1, 8), np.asarray(compress[1]).reshape(-1, 64), np.asarray(compress[2]).reshape(-1, 8)):
            x.compress(hx, w, meta)
    return x


def steps(x, raw_base):
    """The RAW records of an Expansion's rows as zkm_sha_calls_steps writes them: (kind 28, reads[0] = raw_base + j, reads[1] = mask)."""
    from .cpu_steps_model import KIND, STEP_DT
    out = np.zeros(len(x.rows), dtype=STEP_DT)
    out["kind"] = KIND["RAW"]
    out["reads"][:, 0] = raw_base + np.arange(len(x.rows))
    out["reads"][:, 1] = x.masks
    return out, np.array(x.clocks, dtype=np.uint64)


# ---- a Machine run with calls spliced in at their clocks
class CallRecorder:
    """Calls made between the instructions of a cpu_steps_model.Recorder: each takes the clocks that follow the Machine's last row, and
    leaves placeholders in the step list where its rows belong.  own=False: the Machine's rows alone (the segment without calls)."""

    def __init__(self, m):
        self.m, self.extends, self.compresses, self.at = m, [], [], []

    def _reserve(self, count):
        from .cpu_steps_model import KIND
        self.at.append((len(self.m.rows), count))
        for _ in range(count):
            self.m.steps.append((0, 0, 0, KIND["RAW"], 0, 0, [0] * 6))
            self.m.rows.append(None)

    def sha_extend(self, w_ptr, w16, ctx=0, seg=CF.SEG_CODE):
        self.extends.append((list(w16), (ctx, seg, w_ptr, 10 * (self.m.clock + 1))))
        self._reserve(96)

    def sha_compress(self, w_ptr, h_ptr, hx, w, ctx=0, seg=CF.SEG_CODE):
        self.compresses.append((list(hx), list(w), (ctx, seg, h_ptr, 10 * (self.m.clock + 9), w_ptr, seg, ctx, 0)))
        self._reserve(11)

    def lists(self):
        e = (np.array([w for w, _ in self.extends], dtype=np.uint32).reshape(-1, 16), np.array([m for _, m in self.extends], dtype=np.uint64).reshape(-1, 4))
        c = (np.array([h for h, _, _ in self.compresses], dtype=np.uint32).reshape(-1, 8),
             np.array([w for _, w, _ in self.compresses], dtype=np.uint32).reshape(-1, 64),
             np.array([m for _, _, m in self.compresses], dtype=np.uint64).reshape(-1, 8))
        return (e if self.extends else None), (c if self.compresses else None)

    def finish(self):
        """Fill the reserved rows from the model; returns the Expansion."""
        x = expand(*self.lists())
        for r, clock in zip(x.rows, x.clocks):
            assert self.m.rows[clock] is None
            self.m.rows[clock] = r
        assert all(r is not None for r in self.m.rows)
        return x
