"""The bootstrap kernel of a segment in Python integers (test infrastructure).

Restated from the reference's generate_bootstrap_kernel (prover/src/cpu/bootstrap_kernel.rs:26-306) and poseidon_sponge_log
(witness/util.rs:370-469): everything the bootstrap pushes into Traces -- CPU rows, memory operations, Poseidon inputs with their
timestamps, PoseidonSponge operations (here already as the rows of PoseidonSpongeStark::generate_trace) and the digests -- as a
function of the image {addr: value}, the 32 root bytes, the 32 image-id bytes and the entry pc.  `make_image` builds self-consistent
images: it computes the page hash words, the root and the image id itself.
"""
import numpy as np

from .poseidon_model import permute

W = 259                       # CpuColumnsView
IS_BOOT, IS_POSEIDON_SPONGE, GEN, CLOCK, CH0 = 0, 82, 86, 204, 205
NUM_CHANNELS = 10
PS_W = 110                    # PoseidonSponge columns
HASH_BASE, ROOT_PAGE, ID_BASE = 0x80000000, 0x81020000, 0x81021000


def bswap32(v):
    return int.from_bytes(int(v).to_bytes(4, "little"), "big")


def sponge_blocks(words, nbytes):
    """The eight-word rate blocks of a message of nbytes bytes given as LE u32 words, the pad10*1 block included."""
    data = b"".join(int(w).to_bytes(4, "little") for w in words)[:nbytes]
    full, rem = divmod(nbytes, 32)
    last = bytearray(32)
    last[:rem] = data[32 * full:]
    if rem == 31:
        last[31] = 0x81
    else:
        last[rem] = 1
        last[31] = 0x80
    data = data[:32 * full] + bytes(last)
    return [[int.from_bytes(data[32 * b + 4 * i:32 * b + 4 * i + 4], "little") for i in range(8)] for b in range(full + 1)]


def sponge(words, nbytes):
    """(states before each permutation, states after it, digest) of the overwrite-mode sponge (poseidon_sponge_stark.rs poseidon())."""
    st, states, posts = [0] * 12, [], []
    for blk in sponge_blocks(words, nbytes):
        st = blk + st[8:]
        states.append(list(st))
        st = permute(st)
        posts.append(list(st))
    return states, posts, st[:4]


def digest_bytes(d):
    return b"".join(int(x).to_bytes(8, "little") for x in d)


def page_words(image, addr):
    return [image.get((addr + 4 * i) & 0xFFFFFFFF, 0) for i in range(1024)]


def id_words(root, entry):
    return [int.from_bytes(root[4 * i:4 * i + 4], "big") for i in range(8)] + [entry]


class BootError(AssertionError):
    pass


class Boot:
    """The bootstrap's part of Traces.  cpu_rows nboot x 259, memory_ops n x 6 {context, segment, virt, timestamp, is_read, value}
    (the layout of zkm_memory_trace), poseidon_inputs n x 12 with poseidon_ts, sponge_rows n x 110, digests (P + 1) x 4."""

    def __init__(self, image, root, image_id, entry, check=True):
        addrs = sorted(image)
        self.rows, self.mem, self.po, self.po_ts, self.ps, self.digests = [], [], [], [], [], []
        for k in range(0, len(addrs), 8):
            self.write_row([(a, image[a]) for a in addrs[k:k + 8]])
        self.pages = [a for a in addrs if a & 0xFFF == 0]
        for a in self.pages:
            d = self.sponge_row([a + 4 * i for i in range(1024)], page_words(image, a), 4096, 0)
            if a == ROOT_PAGE:
                want = bytes(root)
            else:
                h = HASH_BASE + ((a >> 12) << 5)
                if any(h + 4 * i not in image for i in range(8)):
                    raise BootError("missing hash word of page 0x%08x" % a)
                want = b"".join(image[h + 4 * i].to_bytes(4, "little") for i in range(8))
            if check and digest_bytes(d) != want:
                raise BootError("page hash mismatch at 0x%08x" % a)
        ids = id_words(root, entry)
        self.write_row([(ID_BASE + 4 * i, ids[i]) for i in range(8)])
        self.write_row([(ID_BASE + 32, ids[8])])
        d = self.sponge_row([ID_BASE + 4 * i for i in range(9)], ids, 36, ID_BASE + 32)
        if check and digest_bytes(d) != bytes(image_id):
            raise BootError("image id mismatch")
        self.cpu_rows = np.array(self.rows, dtype=np.uint64).reshape(-1, W)
        self.memory_ops = np.array(self.mem, dtype=np.uint64).reshape(-1, 6)
        self.poseidon_inputs = np.array(self.po, dtype=np.uint64).reshape(-1, 12)
        self.poseidon_ts = np.array(self.po_ts, dtype=np.uint64)
        self.sponge_rows = np.array(self.ps, dtype=np.uint64).reshape(-1, PS_W)
        self.digests = np.array(self.digests, dtype=np.uint64).reshape(-1, 4)

    @property
    def clock(self):
        return len(self.rows)

    def new_row(self):
        r = [0] * W
        r[CLOCK], r[IS_BOOT] = self.clock, 1
        return r

    def write_row(self, pairs):
        r = self.new_row()
        for k, (a, v) in enumerate(pairs):
            r[CH0 + 6 * k:CH0 + 6 * k + 6] = [1, 0, 0, 0, a, bswap32(v)]
            self.mem.append([0, 0, a, self.clock * NUM_CHANNELS, 0, bswap32(v)])
        self.rows.append(r)

    def sponge_row(self, base, words, nbytes, final_virt):
        ts = self.clock * NUM_CHANNELS
        states, posts, digest = sponge(words, nbytes)
        for b, st in enumerate(states):
            here = min(32, nbytes - 32 * b)
            for i in range(max(here, 0)):
                w = 8 * b + i // 4
                self.mem.append([0, 0, base[w], ts, 1, bswap32(words[w])])
            self.po.append(st)
            self.po_ts.append(ts)
            # PoseidonSpongeStark::generate_trace (poseidon_sponge_stark.rs:186-381; columns.rs:17-66)
            row, full, rem = [0] * PS_W, here == 32, max(here, 0)
            if full:
                row[0] = 1
            else:
                row[14 + rem] = 1
            for i in range(8):
                if 8 * b + i < len(base):
                    row[3 + i] = base[8 * b + i]
            row[11], row[12], row[13] = ts, nbytes, 32 * b
            row[46:58] = posts[b - 1] if b else [0] * 12
            for i in range(8):
                row[58 + 4 * i:62 + 4 * i] = list(int(st[i]).to_bytes(4, "little"))
                row[90 + i] = st[i]
            row[98:106], row[106:110] = posts[b][4:], posts[b][:4]
            self.ps.append(row)
        r = self.new_row()
        r[IS_POSEIDON_SPONGE] = 1
        r[CH0 + 5], r[CH0 + 11], r[CH0 + 17], r[CH0 + 23] = 0, 0, final_virt, nbytes
        r[GEN:GEN + 4] = digest
        self.rows.append(r)
        self.digests.append(digest)
        return digest

    def counts(self):
        return (len(self.rows), len(self.mem), len(self.po), len(self.digests), len(self.ps))


def make_image(data, entry=0x00401000):
    """A self-consistent image from {addr: value}: the hash words of every page-aligned address in `data` (other than the root page's),
    then the root and the image id.  Words of the root page in `data` are kept as they are.  Returns (image, root, image_id, entry)."""
    image = dict(data)
    for a in sorted(a for a in data if a & 0xFFF == 0 and a != ROOT_PAGE):
        d = digest_bytes(sponge(page_words(image, a), 4096)[2])
        h = HASH_BASE + ((a >> 12) << 5)
        for i in range(8):
            image[h + 4 * i] = int.from_bytes(d[4 * i:4 * i + 4], "little")
    root = digest_bytes(sponge(page_words(image, ROOT_PAGE), 4096)[2]) if ROOT_PAGE in image else bytes(32)
    image_id = digest_bytes(sponge(id_words(root, entry), 36)[2])
    return image, root, image_id, entry


def _data_page(addr, seed):
    rng = np.random.default_rng(seed)
    return {addr + 4 * i: int(v) for i, v in enumerate(rng.integers(0, 1 << 32, 1024, dtype=np.uint64))}


def image_a():
    """One data page at 0x7FFFF000 (its hash words at 0x80FFFFE0 lie in a page whose first word is absent), five words of the root
    page: 1037 words, a last row of five channels, P = 2, nboot = 135."""
    d = _data_page(0x7FFFF000, 1)
    d.update({ROOT_PAGE + 4 * i: 0x1000 + i for i in range(5)})
    return make_image(d)


def image_b():
    """Three words, none page-aligned: P = 0."""
    return make_image({0x7FFFF004: 0x11, 0x7FFFF008: 0x22, 0x7FFFF010: 0xDEADBEEF})


def image_c():
    """Five data pages 0x7FFFB000 .. 0x7FFFF000 (one sparse: words 0 and 1023 only), their hash words, the root: P = 6."""
    d = {}
    for k in range(5):
        a = 0x7FFFB000 + 0x1000 * k
        if k == 2:
            d.update({a: 0xA5A5A5A5, a + 4092: 0x5A5A5A5A})
        else:
            d.update(_data_page(a, 10 + k))
    d[ROOT_PAGE] = 7
    return make_image(d)


def arrays(image):
    """(addrs, values) as the C ABI takes them: ascending addresses."""
    addrs = sorted(image)
    return np.array(addrs, dtype=np.uint32), np.array([image[a] for a in addrs], dtype=np.uint32)
