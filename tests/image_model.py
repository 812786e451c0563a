"""The emulator's split-time hashing in Python integers (test infrastructure).

Restated from the reference's Memory::update_page_hash, set_hash_range, alloc_hash_page / CONST_HASH_PAGES and compute_image_id
(emulator/src/memory.rs:81-118, 378-471) on boot_model.sponge (memory.rs:43-79 poseidon).  `Memory` is stateful -- a dict of hash pages
that outlives a split -- so that consecutive splits can be modelled: a hash page that exists keeps its words, one that does not is
allocated as the constant page of its level.  The permutation is poseidon_model.permute (Python integers) unless a batched one is handed
in (the oracle's C permutation, for the larger cases; tests/test_image_model.py holds the two paths equal)."""
import numpy as np

from . import boot_model as BM
from .poseidon_model import permute

L1_BASE, L2_BASE, ROOT_INDEX, MAIN_PAGES = 0x80000, 0x81000, 0x81020, 0x80000
REGISTERS_OFFSET = 0x400


def python_batch(states):
    return [permute(list(st)) for st in states]


def oracle_batch(oracle):
    """states -> permuted states through the oracle's batched C permutation."""
    def run(states):
        out = oracle.poseidon_permute_batch(np.array(states, dtype=np.uint64).reshape(-1, 12))
        return [[int(v) for v in row] for row in out.reshape(-1, 12)]
    return run


def hash_pages(pages, batch=python_batch):
    """hash_page of each 1024-word page: its digest as eight LE words (word 2j the low half of digest word j).  The sponges advance in
    lock-step, one batched permutation a block."""
    pages = [list(p) for p in pages]
    if not pages:
        return []
    blocks = [BM.sponge_blocks(p, 4096) for p in pages]
    states = [[0] * 12 for _ in pages]
    for b in range(129):
        states = batch([blocks[i][b] + states[i][8:] for i in range(len(pages))])
    out = []
    for st in states:
        d = BM.digest_bytes(st[:4])
        out.append([int.from_bytes(d[4 * i:4 * i + 4], "little") for i in range(8)])
    return out


def const_digests(batch=python_batch):
    """The fill of a fresh L1, L2 and root page (compute_const_hash_pages): the zero page's digest, then the digest of a page filled with
    the one before."""
    out, page = [], [0] * 1024
    for _ in range(3):
        d = hash_pages([page], batch)[0]
        out.append(d)
        page = d * 128
    return out


def plan(dirty):
    """The ascending hash pages update_page_hash writes for these dirty page indices: L1 pages, L2 pages, the root."""
    dirty = sorted(dirty)
    return sorted({L1_BASE + (p >> 7) for p in dirty}) + sorted({L2_BASE + (p >> 14) for p in dirty}) + [ROOT_INDEX]


class Memory:
    """The hash pages of one emulated memory, {page index: 1024 words}."""

    def __init__(self, batch=python_batch, consts=None):
        self.batch = batch
        self.consts = consts if consts is not None else const_digests(batch)
        self.pages = {}

    def _set_hash_range(self, index, digest, level):
        addr = 0x80000000 + (index << 5)
        page, off = addr >> 12, (addr & 0xFFF) // 4
        if page not in self.pages:
            self.pages[page] = self.consts[level] * 128         # alloc_hash_page
        self.pages[page][off:off + 8] = digest
        return page

    def split(self, dirty, pc, registers):
        """dirty: {page index < 0x80000: 1024 words}.  update_page_hash, then compute_image_id(pc, registers).  Returns
        (plan, [the plan pages as they are left], root bytes, image id bytes)."""
        assert all(0 <= p < MAIN_PAGES for p in dirty) and len(bytes(registers)) == 156
        level_pages = sorted(dirty)
        words = [dirty[p] for p in level_pages]
        for level in range(3):
            digests = hash_pages(words, self.batch)
            parents = sorted({self._set_hash_range(p, d, level) for p, d in zip(level_pages, digests)})
            level_pages, words = parents, [self.pages[q] for q in parents]
        if ROOT_INDEX not in self.pages:
            raise BM.BootError("compute image ID fail")
        regs = bytes(registers)
        root_page = self.pages[ROOT_INDEX]
        root_page[REGISTERS_OFFSET // 4:REGISTERS_OFFSET // 4 + 39] = [int.from_bytes(regs[4 * i:4 * i + 4], "little") for i in range(39)]
        root_words = hash_pages([root_page], self.batch)[0]
        root = b"".join(w.to_bytes(4, "little") for w in root_words)
        # final_data: the root's words as big-endian bytes, then pc little-endian; read back as LE words by the sponge
        st = [0] * 12
        for blk in BM.sponge_blocks(BM.id_words(root, pc), 36):
            st = self.batch([blk + st[8:]])[0]
        pl = plan(dirty)
        return pl, [list(self.pages[q]) for q in pl], root, BM.digest_bytes(st[:4])


def boot_image(dirty, pl, pages):
    """{addr: value} of a memory that holds the dirty pages and the plan pages: what boot_model.Boot takes."""
    image = {}
    for index, words in list(dirty.items()) + list(zip(pl, pages)):
        image.update({(index << 12) + 4 * i: int(w) for i, w in enumerate(words)})
    return image


# ---- the cases of the issue, shared by the CPU and the GPU tests (built once per process, not to be changed)
def random_page(seed):
    return [int(v) for v in np.random.default_rng(seed).integers(0, 1 << 32, 1024, dtype=np.uint64)]


def registers(seed):
    return bytes(int(v) for v in np.random.default_rng(seed).integers(0, 256, 156))


CASE_A = {"dirty": {0x7FFFF: random_page(100)}, "pc": 0x00401234, "registers": registers(1)}
CASE_B = {"dirty": {0: random_page(200), 1: [0xFFFFFFFF] * 1024, 0x7F: random_page(201), 0x80: [0] * 1024, 0x4000: random_page(202),
                    0x7FFFF: random_page(203)}, "pc": 0x00402000, "registers": registers(2)}
CASE_C2 = {"dirty": {1: random_page(300), 0x81: random_page(301), 0x12345: random_page(302)}, "pc": 0x00403004, "registers": registers(3)}
CASE_D2 = {"dirty": {}, "pc": 0x00404008, "registers": registers(4)}
CASE_E = [{"dirty": {0x300: random_page(400)}, "pc": 0x1000, "registers": registers(5)},
          {"dirty": {0x1280 + i: random_page(410 + i) for i in range(17)}, "pc": 0x2000, "registers": registers(6)},
          {"dirty": {0x7FF00 + 40 * i: random_page(430 + i) for i in range(6)}, "pc": 0x3000, "registers": registers(7)}]

_CACHE = {}


def solved(name, oracle=None):
    """The model's results of a named case, cached per process: "a" (Python integers), "a_c" (the same through the oracle), "b", "c"
    (B then C2 on the same memory: a list of the two results), "d" (B then no dirty page, new registers and pc), "e0" .. "e2".  Every
    name but "a" needs the oracle."""
    if name in _CACHE:
        return _CACHE[name]
    batch = python_batch if name == "a" else oracle_batch(oracle)
    if "consts" not in _CACHE and name != "a":
        _CACHE["consts"] = const_digests(batch)
    mem = Memory(batch, None if name == "a" else _CACHE["consts"])
    run = lambda case: mem.split(case["dirty"], case["pc"], case["registers"])
    if name in ("a", "a_c"):
        out = run(CASE_A)
    elif name == "b":
        out = run(CASE_B)
        _CACHE["b_pages"] = {q: list(w) for q, w in mem.pages.items()}
    elif name in ("c", "d"):
        first = solved("b", oracle)
        mem.pages = {q: list(w) for q, w in _CACHE["b_pages"].items()}       # the memory as the first split left it
        out = [first, run(CASE_C2 if name == "c" else CASE_D2)]
    else:
        out = run(CASE_E[int(name[1])])
    _CACHE[name] = out
    return out
