"""A whole segment that opens with the real bootstrap kernel (tests/boot_model.py) and then runs cpu_fixtures.sample_program: the joined
lists, what simulate_cpu pushed alone (the `ops` of the zkm_*_boot calls) and the twelve tables at the heights of into_tables on the
joined lists.  The Memory table comes from oracle.memory_trace, the Poseidon table from oracle.poseidon_trace_inputs, the PoseidonSponge
table from the model's rows (the oracle's generator reads word i of an operation at virt_base + i; the bootstrap's step by 4); the
precompile tables are padding."""
import numpy as np

from zkm_amd import tables as T

from . import arith_fixtures as A
from . import boot_model as BM
from . import cpu_fixtures as CF
from . import segment_ops_fixtures as SF

P = CF.P
STACK = 0x7FFFE000          # where the sample program's loads and stores go: beside the data pages, not 2^31 below them


class BootMachine(CF.Machine):
    """cpu_fixtures.Machine whose boot() installs the model's rows and memory operations."""

    def __init__(self, boot):
        self.model = boot
        super().__init__()

    def boot(self, words):
        self.rows = [[int(v) for v in r] for r in self.model.cpu_rows]
        for ctx, seg, virt, ts, is_read, value in self.model.memory_ops.tolist():
            self.mem_ops.append((is_read, ctx, seg, virt, value, ts))
            if not is_read:
                self.mem[(seg, virt)] = value

    def set_reg(self, reg, value):
        # the base register of the sample program's loads and stores (0x100, 0x10C): moved up so that Memory needs no 2^17 gap rows
        super().set_reg(reg, value + STACK if reg == 22 else value)


def columns(rows, log_n):
    """Row-major rows, zero-padded to 2^log_n, as a flat column-major table."""
    rows = np.asarray(rows, dtype=np.uint64)
    t = np.zeros((1 << log_n, rows.shape[1]), dtype=np.uint64)
    t[:len(rows)] = rows
    return np.ascontiguousarray(t.T).reshape(-1)


def build_boot_segment(oracle, image, check=True):
    """image: (dict, root, image_id, entry) as boot_model.make_image gives it.  Returns a dict: model (boot_model.Boot), raw (the joined
    lists, segment_ops_fixtures form), exec (what simulate_cpu pushed), tables (the twelve, Table::all() order), ctls, log_ns."""
    model = BM.Boot(*image, check=check)
    m = CF.sample_program(BootMachine(model))
    nboot = len(model.cpu_rows)
    log_cpu = int(np.ceil(np.log2(len(m.rows) + 1)))
    cpu_rows = np.zeros((1 << log_cpu, CF.W), dtype=np.uint64)
    cpu_rows[:len(m.rows)] = np.array([[v % P for v in r] for r in m.rows], dtype=np.uint64)
    code = {"and": T.OP_AND, "or": T.OP_OR, "xor": T.OP_XOR, "nor": T.OP_NOR}
    lops = np.array([(code[name], a, b) for name, a, b, _ in m.logic_ops], dtype=np.uint32).reshape(-1, 3)
    flag = {"addu": A.IS_ADDU, "subu": A.IS_SUBU, "addiu": A.IS_ADDIU, "sll": A.IS_SLL, "srl": A.IS_SRL, "sra": A.IS_SRA,
            "sllv": A.IS_SLLV, "srlv": A.IS_SRLV, "srav": A.IS_SRAV}
    aops = np.array([(flag[name], a, b) for name, a, b, _, _ in m.arith_ops], dtype=np.uint32).reshape(-1, 3)
    mem_ops = np.array([(ctx, seg, virt, ts, is_read, value) for is_read, ctx, seg, virt, value, ts in m.mem_ops], dtype=np.uint64)
    assert (mem_ops[:len(model.memory_ops)] == model.memory_ops).all()
    log_mem = int(np.ceil(np.log2(len(mem_ops))))
    while True:
        try:
            memory, natural = oracle.memory_trace(mem_ops, log_mem)
            break
        except RuntimeError:
            log_mem += 1
    assert natural == 1 << log_mem
    e8, e64 = np.zeros(0, np.uint8), np.zeros(0, np.uint64)
    three = (np.zeros((0, 8), np.uint32), np.zeros((0, 64), np.uint32), np.zeros((0, 8), np.uint64))
    empty = {"poseidon_sponge": (e8, np.zeros(1, np.uint64), np.zeros((0, 4), np.uint64)), "keccak": (np.zeros((0, 25), np.uint64), e64),
             "keccak_sponge": (e8, np.zeros(1, np.uint64), np.zeros((0, 4), np.uint64)), "sha_extend": (np.zeros((0, 16), np.uint8), e64),
             "sha_extend_sponge": (np.zeros((0, 16), np.uint32), np.zeros((0, 4), np.uint64)), "sha_compress": three, "sha_compress_sponge": three}
    raw = dict(empty, cpu_rows=cpu_rows, arithmetic=aops, logic=lops, memory=mem_ops, poseidon=(model.poseidon_inputs, model.poseidon_ts),
               log_arithmetic=16, log_memory=log_mem)
    execd = dict(empty, cpu_rows=np.ascontiguousarray(cpu_rows[nboot:]), arithmetic=aops, logic=lops,
                 memory=np.ascontiguousarray(mem_ops[len(model.memory_ops):]), poseidon=(np.zeros((0, 12), np.uint64), e64))
    lg = SF.reference_log_ns(raw)
    lg[3] = SF.log2_height(len(model.sponge_rows), 64)
    zeros = lambda w, l: np.zeros(w << l, np.uint64)
    by_pos = [A.generate_trace([tuple(int(x) for x in op) for op in aops], lg[0]), cpu_rows.T.copy().reshape(-1),
              oracle.poseidon_trace_inputs(model.poseidon_inputs, model.poseidon_ts, lg[2]), columns(model.sponge_rows, lg[3]),
              zeros(2431, lg[4]), zeros(470, lg[5]), zeros(78, lg[6]), zeros(76, lg[7]), zeros(224, lg[8]), zeros(127, lg[9]),
              oracle.logic_trace(lops, lg[10]), memory]
    c, ctls = T.all_cross_table_lookups()
    tables = [(SF.ORDER[i], by_pos[i], T.WIDTH[SF.ORDER[i]], lg[i], c[i]) for i in range(12)]
    return {"model": model, "raw": raw, "exec": execd, "tables": tables, "ctls": ctls, "log_ns": lg, "nboot": nboot}


_CACHE = {}


def segment(oracle, name):
    """build_boot_segment of boot_model.image_a / _b / _c (name "a", "b", "c"), built once per process and not to be changed."""
    if name not in _CACHE:
        image = getattr(BM, "image_" + name)()
        _CACHE[name] = dict(build_boot_segment(oracle, image), image=image)
    return _CACHE[name]


def boot_image(zkm, image, check=True, **kw):
    """boot_model.make_image's tuple as a zkm_amd.BootImage."""
    d, root, image_id, entry = image
    return zkm.BootImage.from_dict(d, root, image_id, entry, check=check, **kw)
