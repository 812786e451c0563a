"""zkm_amd -- MI355X-native STARK/FRI hot path of the zkMIPS prover.

Thin ctypes binding of the C-ABI library `zkm_amd/csrc/libzkmhip.so` (see include/zkm_hip.h).  The class
and method names mirror the plonky2 / zkm-prover items the library replaces (PolynomialBatch.from_values,
.merkle_tree.cap, get_lde_values, Challenger, prove_single_table; reference prover/src/prover.rs:441-641)
so the parity tests read like the reference's own.  There is NO CPU fallback: if the HIP extension is
missing or no GPU is present, every compute entry point raises.
"""
import ctypes as C
import os
import re
import subprocess
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_LIB_PATH = os.environ.get("ZKM_HIP_LIB") or os.path.join(_CSRC, "libzkmhip.so")   # (ZKM_HIP_LIB: A/B builds of the same in-tree sources)

P = 0xFFFFFFFF00000001


class ZkmError(RuntimeError):
    pass


from . import abi  # noqa: E402  (abi raises ZkmError)

# the constants below restate nothing: each is read from its #define in include/zkm_hip.h (a name the header lacks fails the import)
_H = abi.constants("ZKM_")
POSEIDON_COLS, KECCAK_SPONGE_COLS, LOGIC_COLS, MEMORY_COLS, ARITHMETIC_COLS, KECCAK_COLS, POSEIDON_SPONGE_COLS = (
    _H[n + "_COLS"] for n in ("POSEIDON", "KECCAK_SPONGE", "LOGIC", "MEMORY", "ARITHMETIC", "KECCAK", "POSEIDON_SPONGE"))
TABLE_POSEIDON, TABLE_LOGIC, TABLE_KECCAK_SPONGE, TABLE_KECCAK, TABLE_MEMORY, TABLE_POSEIDON_SPONGE = 0, 1, 2, 3, 4, 5
TABLE_SHA_EXTEND, TABLE_SHA_EXTEND_SPONGE, TABLE_SHA_COMPRESS, TABLE_SHA_COMPRESS_SPONGE, TABLE_ARITHMETIC, TABLE_CPU = 6, 7, 8, 9, 10, 11
# zkm_poseidon_selftest: ZKM_POSEIDON_OUT_* and ZKM_POSEIDON_PROBE_*
POSEIDON_OUT_ALL, POSEIDON_OUT_CAPACITY, POSEIDON_OUT_DIGEST = (_H["POSEIDON_OUT_" + n] for n in ("ALL", "CAPACITY", "DIGEST"))
POSEIDON_PROBE = abi.constants("ZKM_POSEIDON_PROBE_")
WITNESS_FINDING_WORDS = _H["WITNESS_FINDING_WORDS"]   # zkm_witness_check: row, constraint index, value, failing rows, constraints per row
# zkm_lookup_check: failing lookup, value, looking count, frequency, table rows, first looking cell (column, row), first table row, failing values
LOOKUP_FINDING_WORDS = _H["LOOKUP_FINDING_WORDS"]
SEGMENT_VERDICT_WORDS = _H["SEGMENT_VERDICT_WORDS"]   # zkm_segments_check: kind of the first finding, its table position or lookup index
u64p = C.POINTER(C.c_uint64)

EXPORTS = [name for name, _, _ in abi.prototypes()]


def build(force=False):
    """Compile libzkmhip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", _CSRC, "-j8", "-s"]
    if force:
        subprocess.check_call(["make", "-C", _CSRC, "clean", "-s"])
    subprocess.check_call(args)
    return _LIB_PATH


class Challenger(C.Structure):
    """plonky2 Challenger<F, PoseidonHash> state (host side)."""
    _fields_ = [("state", C.c_uint64 * 12), ("in_buf", C.c_uint64 * 8), ("out_buf", C.c_uint64 * 8),
                ("n_in", C.c_uint32), ("n_out", C.c_uint32)]


class ProofLayout(C.Structure):
    """zkm_proof_layout (include/zkm_hip.h): word offsets of the fields of one proof blob."""
    _fields_ = [(n, C.c_uint64) for n in ("degree_bits", "trace_cols", "aux_cols", "quotient_polys", "ctl_zs", "cap_height", "fri_layers",
                                          "final_poly_len", "num_queries", "rate_bits", "arity_bits")] + \
               [(n, C.c_size_t) for n in ("total_words", "init_challenger_state", "trace_cap", "aux_cap", "quotient_cap", "local_values",
                                          "next_values", "aux_polys", "aux_polys_next", "ctl_zs_first", "quotient_polys_open",
                                          "commit_phase_merkle_caps", "final_poly", "pow_witness", "query_round_proofs",
                                          "query_round_words")]


class ProofQueryLayout(C.Structure):
    """zkm_proof_query_layout: offsets inside one FRI query round."""
    _fields_ = [("oracle_evals", C.c_size_t * 3), ("oracle_cols", C.c_size_t * 3), ("oracle_siblings", C.c_size_t * 3),
                ("initial_siblings", C.c_size_t), ("layer_evals", C.c_size_t * 16), ("layer_siblings", C.c_size_t * 16),
                ("layer_siblings_count", C.c_size_t * 16)]


class StarkConfig(C.Structure):
    _fields_ = [(n, C.c_uint) for n in
                ("rate_bits", "cap_height", "pow_bits", "num_challenges", "num_queries", "arity_bits", "final_poly_bits")]


class FriPoly(C.Structure):
    """zkm_fri_poly: one polynomial of a FRI batch = (oracle index, column index)."""
    _fields_ = [("oracle", C.c_uint32), ("poly", C.c_uint32)]


class FriBatch(C.Structure):
    """zkm_fri_batch: the polynomials opened at one point (FriBatchInfo, stark.rs:127-148)."""
    _fields_ = [("point", C.c_uint64 * 2), ("polys", C.c_void_p), ("npolys", C.c_size_t)]


class FriClaim:
    """One claim of Context.fri_verify (zkm_fri_verify): the FRI proof blob of fri_prove, the instance it was made for -- log_n, the
    columns and the cap of each oracle, batches as fri_prove takes them -- the opened values (opened[b] = 2 * npolys words, the claimed
    p(point) of batch b's polynomials in the batch's order) and the challenger fri_prove was entered with (in/out)."""

    def __init__(self, proof, log_n, oracle_cols, oracle_caps, batches, opened, challenger, proof_words=None):
        self.proof, self.log_n, self.oracle_cols, self.oracle_caps = proof, log_n, list(oracle_cols), list(oracle_caps)
        self.batches, self.opened, self.challenger, self.proof_words = list(batches), list(opened), challenger, proof_words


# zkm_segment_ops (include/zkm_hip.h): per group of fields, the data pointers (with the bytes of one item of each) and the count
SEGMENT_OPS_GROUPS = [
    ("cpu_rows", [("cpu_rows", 259 * 8)], "ncpu_rows"),
    ("arithmetic", [("arithmetic_ops", 12)], "narithmetic"),
    ("logic", [("logic_ops", 12)], "nlogic"),
    ("memory", [("memory_ops", 48)], "nmemory"),
    ("poseidon", [("poseidon_inputs", 96), ("poseidon_timestamps", 8)], "nposeidon"),
    ("poseidon_sponge", [("poseidon_sponge_inputs", 0), ("poseidon_sponge_off", 0), ("poseidon_sponge_meta", 32)], "nposeidon_sponge"),
    ("keccak", [("keccak_inputs", 200), ("keccak_timestamps", 8)], "nkeccak"),
    ("keccak_sponge", [("keccak_sponge_inputs", 0), ("keccak_sponge_off", 0), ("keccak_sponge_meta", 32)], "nkeccak_sponge"),
    ("sha_extend", [("sha_extend_inputs", 16), ("sha_extend_timestamps", 8)], "nsha_extend"),
    ("sha_extend_sponge", [("sha_extend_sponge_w16", 64), ("sha_extend_sponge_meta", 32)], "nsha_extend_sponge"),
    ("sha_compress", [("sha_compress_hx", 32), ("sha_compress_w", 256), ("sha_compress_meta", 64)], "nsha_compress"),
    ("sha_compress_sponge", [("sha_compress_sponge_hx", 32), ("sha_compress_sponge_w", 256), ("sha_compress_sponge_meta", 64)],
     "nsha_compress_sponge"),
]


class SegmentOpsStruct(C.Structure):
    """zkm_segment_ops: a segment's raw operations, one group per field of the reference's Traces (witness/traces.rs:47-62)."""
    _fields_ = [f for _, ptrs, count in SEGMENT_OPS_GROUPS for f in [(name, C.c_void_p) for name, _ in ptrs] + [(count, C.c_size_t)]]


class BootImageStruct(C.Structure):
    """zkm_boot_image: a segment's memory image with its root, image id and entry pc (include/zkm_hip.h)."""
    _fields_ = [("addrs", C.c_void_p), ("values", C.c_void_p), ("nwords", C.c_size_t), ("npages", C.c_size_t), ("entry", C.c_uint32),
                ("check", C.c_uint32), ("pre_hash_root", C.c_uint8 * 32), ("pre_image_id", C.c_uint8 * 32)]


class ImagePagesStruct(C.Structure):
    """zkm_image_pages: the dirty pages of a split, the hash pages that exist already, pc and the registers (include/zkm_hip.h)."""
    _fields_ = [("dirty_index", C.c_void_p), ("ndirty", C.c_size_t), ("dirty_words", C.c_void_p), ("known_index", C.c_void_p),
                ("nknown", C.c_size_t), ("known_words", C.c_void_p), ("pc", C.c_uint32), ("registers", C.c_uint8 * 156)]


# zkm_cpu_step (include/zkm_hip.h): one cycle of the compact step log; STEP_KINDS[k] names ZKM_STEP_<k>, SYSCALL_KINDS the ZKM_SYSCALL_*
CPU_STEP_DT = np.dtype([("pc", "<u4"), ("next_pc", "<u4"), ("insn", "<u4"), ("kind", "<u4"), ("flags", "<u4"), ("context", "<u4"),
                        ("reads", "<u4", (6,))])
STEP = {n: v for n, v in abi.constants("ZKM_STEP_").items() if not n.startswith("FLAG_")}
STEP_KINDS = tuple(STEP)
assert list(STEP.values()) == list(range(len(STEP)))      # STEP_KINDS[k] names kind k
SYSCALL_KINDS = {n.lower(): v for n, v in abi.constants("ZKM_SYSCALL_").items()}


class CpuStepsStruct(C.Structure):
    """zkm_cpu_steps: a segment's step list and the ready-made rows its RAW steps index."""
    _fields_ = [("steps", C.c_void_p), ("nsteps", C.c_size_t), ("raw_rows", C.c_void_p), ("nraw", C.c_size_t)]


class CpuSteps:
    """A segment's compact step log for Context.cpu_witness / segments_tables_steps / prove_segments_ops_steps (include/zkm_hip.h
    zkm_cpu_steps).  steps: a CPU_STEP_DT array (host memory); raw_rows: nraw x 259 uint64 (numpy, or a DeviceBuffer with nraw given)."""

    def __init__(self, steps, raw_rows=None, nraw=None):
        self.steps = np.ascontiguousarray(steps, dtype=CPU_STEP_DT).reshape(-1)
        if raw_rows is None:
            raw_rows = np.zeros((0, 259), dtype=np.uint64)
        self.raw_rows = raw_rows if isinstance(raw_rows, DeviceBuffer) else np.ascontiguousarray(raw_rows, dtype=np.uint64).reshape(-1, 259)
        self.nraw = int(nraw) if nraw is not None else len(self.raw_rows)

    def struct(self):
        st = CpuStepsStruct()
        st.steps, st.nsteps = (self.steps.ctypes.data if self.steps.size else None), self.steps.size
        st.raw_rows = self.raw_rows.ptr if isinstance(self.raw_rows, DeviceBuffer) else (self.raw_rows.ctypes.data if self.nraw else None)
        st.nraw = self.nraw
        return st

    def counts(self):
        """zkm_cpu_steps_counts: (memory_ops, logic_ops, arithmetic_ops) the steps push; needs no GPU."""
        return cpu_steps_counts(self)


def cpu_steps_counts(steps):
    """zkm_cpu_steps_counts on a CpuSteps: the lengths of the three lists its steps push.  Every refusal of the host walk (an unknown
    kind, an encoding the kind does not take, a RAW index out of range) raises ZkmError naming the step."""
    out, err, st = [C.c_size_t() for _ in range(3)], C.c_char_p(), steps.struct()
    _check(load().zkm_cpu_steps_counts(C.byref(st), *[C.byref(x) for x in out], C.byref(err)), err)
    return tuple(int(x.value) for x in out)


def sha_calls_counts(nextend, ncompress):
    """zkm_sha_calls_counts: (cpu_rows, memory_ops, logic_ops, sha_extend_rows) that nextend SYSSHAEXTEND and ncompress SYSSHACOMPRESS calls
    expand into; needs no GPU."""
    out = [C.c_size_t() for _ in range(4)]
    load().zkm_sha_calls_counts(nextend, ncompress, *[C.byref(x) for x in out])
    return tuple(int(x.value) for x in out)


def _sha_meta(meta, width):
    return np.ascontiguousarray(meta if meta is not None else [], dtype=np.uint64).reshape(-1, width)


def sha_calls_steps(extend_meta=None, compress_meta=None, raw_base=0):
    """zkm_sha_calls_steps: the RAW step records (a CPU_STEP_DT array) of the calls' rows and the clock each belongs at (uint64); needs no
    GPU.  extend_meta n x 4, compress_meta n x 8 uint64, as the sponge tables take them.  Every refusal raises ZkmError naming the list
    and the call."""
    em, cm = _sha_meta(extend_meta, 4), _sha_meta(compress_meta, 8)
    rows = sha_calls_counts(len(em), len(cm))[0]
    steps, clocks, err = np.zeros(rows, dtype=CPU_STEP_DT), np.zeros(rows, dtype=np.uint64), C.c_char_p()
    _check(load().zkm_sha_calls_steps(em.ctypes.data if len(em) else None, len(em), cm.ctypes.data if len(cm) else None, len(cm), raw_base,
                                      steps.ctypes.data if rows else None, clocks.ctypes.data if rows else None, C.byref(err)), err)
    return steps, clocks


def keccak_calls_counts(input_off, meta=None):
    """zkm_keccak_calls_counts: (cpu_rows, memory_ops, logic_ops, keccak_perms) that the SYSKECCAK calls with these ncalls + 1 input
    offsets expand into; needs no GPU.  A length that is 0 or not a multiple of 4 raises ZkmError naming the call.  With meta (ncalls x
    4 uint64; anything but a numpy array or a list counts as device memory, which the host does not read) it is
    zkm_keccak_calls_counts_meta: a call whose meta carries ZKM_SPONGE_PADDED_TAIL may have any positive length."""
    off = np.ascontiguousarray(input_off, dtype=np.uint64).reshape(-1)
    out, err = [C.c_size_t() for _ in range(4)], C.c_char_p()
    n = max(off.size, 1) - 1
    if meta is None or not isinstance(meta, (np.ndarray, list, tuple)):
        _check(load().zkm_keccak_calls_counts(off.ctypes.data if n else None, n, *[C.byref(x) for x in out], C.byref(err)), err)
    else:
        m = _sha_meta(meta, 4)
        assert len(m) == n, "one meta per call"
        _check(load().zkm_keccak_calls_counts_meta(off.ctypes.data if n else None, m.ctypes.data if n else None, n, *[C.byref(x) for x in out],
                                                   C.byref(err)), err)
    return tuple(int(x.value) for x in out)


def keccak_calls_steps(input_off, meta, raw_base=0):
    """zkm_keccak_calls_steps: the RAW step records (a CPU_STEP_DT array) of the calls' rows and the clock each belongs at (uint64); needs
    no GPU.  input_off ncalls + 1, meta ncalls x 4 uint64 with ZKM_SPONGE_BYTE_ADDRESSED in word 2, as the KeccakSponge table takes
    them.  Every refusal raises ZkmError naming the list and the call."""
    off, m = np.ascontiguousarray(input_off, dtype=np.uint64).reshape(-1), _sha_meta(meta, 4)
    n = len(m)
    assert off.size == n + 1, "one offset more than calls"
    rows = keccak_calls_counts(off, m)[0]
    steps, clocks, err = np.zeros(rows, dtype=CPU_STEP_DT), np.zeros(rows, dtype=np.uint64), C.c_char_p()
    _check(load().zkm_keccak_calls_steps(off.ctypes.data if n else None, m.ctypes.data if n else None, n, raw_base,
                                         steps.ctypes.data if rows else None, clocks.ctypes.data if rows else None, C.byref(err)), err)
    return steps, clocks


SPONGE_BYTE_ADDRESSED = _H["SPONGE_BYTE_ADDRESSED"]
SPONGE_PADDED_TAIL = _H["SPONGE_PADDED_TAIL"]           # beside it on a SYSKECCAK call: the last memory word is the padded message's
# the kinds of the I/O calls (ZKM_IO_*): hint_read, commit, verify, preimage
IO_KINDS = {n.lower(): v for n, v in abi.constants("ZKM_IO_").items()}


def _io_lists(io):
    """(kinds u32 n, data u8 or device memory, data_off n + 1, meta n x 4 or device memory) with the host lists as contiguous numpy
    arrays, and the number of calls; None, 0 without calls."""
    if io is None:
        return None, 0
    kinds, data, off, meta = io
    host = lambda x, dt: np.ascontiguousarray(x if x is not None else [], dtype=dt) if not isinstance(x, DeviceBuffer) else x
    k = (np.ascontiguousarray(kinds, dtype=np.uint32).reshape(-1), host(data, np.uint8), np.ascontiguousarray(off, dtype=np.uint64).reshape(-1),
         _sha_meta(meta, 4) if not isinstance(meta, DeviceBuffer) else meta)
    n = k[0].size
    assert k[2].size == n + 1 and (isinstance(k[3], DeviceBuffer) or len(k[3]) == n), "one kind and one meta per call, and one offset more"
    return (k if n else None), n


def io_calls_counts(kinds, data_off):
    """zkm_io_calls_counts: (cpu_rows, memory_ops) that the I/O calls of these kinds (IO_KINDS) with these ncalls + 1 offsets expand
    into; needs no GPU.  An unknown kind or a length the kind does not take raises ZkmError naming the list and the call."""
    kd, off = np.ascontiguousarray(kinds, dtype=np.uint32).reshape(-1), np.ascontiguousarray(data_off, dtype=np.uint64).reshape(-1)
    assert off.size == kd.size + 1 or kd.size == 0, "one offset more than calls"
    out, err = [C.c_size_t() for _ in range(2)], C.c_char_p()
    _check(load().zkm_io_calls_counts(kd.ctypes.data if kd.size else None, off.ctypes.data if kd.size else None, kd.size,
                                      *[C.byref(x) for x in out], C.byref(err)), err)
    return tuple(int(x.value) for x in out)


def io_calls_steps(kinds, data_off, meta, raw_base=0):
    """zkm_io_calls_steps: the RAW step records (a CPU_STEP_DT array) of the calls' rows and the clock each belongs at (uint64); needs no
    GPU.  kinds ncalls, data_off ncalls + 1, meta ncalls x 4 uint64 (context, segment, address, the first row's timestamp).  Every refusal
    raises ZkmError naming the list and the call."""
    kd, off, m = np.ascontiguousarray(kinds, dtype=np.uint32).reshape(-1), np.ascontiguousarray(data_off, dtype=np.uint64).reshape(-1), _sha_meta(meta, 4)
    n = kd.size
    assert off.size == n + 1 and len(m) == n, "one meta per call, and one offset more"
    rows = io_calls_counts(kd, off)[0]
    steps, clocks, err = np.zeros(rows, dtype=CPU_STEP_DT), np.zeros(rows, dtype=np.uint64), C.c_char_p()
    _check(load().zkm_io_calls_steps(kd.ctypes.data if n else None, off.ctypes.data if n else None, m.ctypes.data if n else None, n, raw_base,
                                     steps.ctypes.data if rows else None, clocks.ctypes.data if rows else None, C.byref(err)), err)
    return steps, clocks


# the kinds of the instruction rows (ZKM_INSN_*): lui, mul, mult, multu, div, divu, mfhi, mthi, mflo, mtlo, sdc1, sync, pref
INSN_KINDS = {n.lower(): v for n, v in abi.constants("ZKM_INSN_").items()}


def _insn_lists(insns):
    """(records CPU_STEP_DT n, clocks u64 n) as contiguous numpy arrays, and the number of records; None, 0 without records."""
    if insns is None:
        return None, 0
    records, clocks = insns
    k = (np.ascontiguousarray(records, dtype=CPU_STEP_DT).reshape(-1), np.ascontiguousarray(clocks, dtype=np.uint64).reshape(-1))
    assert k[0].size == k[1].size, "one clock per record"
    return (k if k[0].size else None), k[0].size


def insn_rows_counts(records):
    """zkm_insn_rows_counts: (memory_ops, arithmetic_ops) that the rows of these instruction records (a CPU_STEP_DT array, kind one of
    INSN_KINDS) push; needs no GPU.  Every refusal of the host walk raises ZkmError naming the record."""
    r = np.ascontiguousarray(records, dtype=CPU_STEP_DT).reshape(-1)
    out, err = [C.c_size_t() for _ in range(2)], C.c_char_p()
    _check(load().zkm_insn_rows_counts(r.ctypes.data if r.size else None, r.size, *[C.byref(x) for x in out], C.byref(err)), err)
    return tuple(int(x.value) for x in out)


def insn_rows_steps(records, raw_base=0):
    """zkm_insn_rows_steps: the RAW step records (a CPU_STEP_DT array) of the instruction records' rows, record k for the position
    clocks[k] - first_clock of the step list; needs no GPU.  Every refusal raises ZkmError naming the record."""
    r = np.ascontiguousarray(records, dtype=CPU_STEP_DT).reshape(-1)
    steps, err = np.zeros(r.size, dtype=CPU_STEP_DT), C.c_char_p()
    _check(load().zkm_insn_rows_steps(r.ctypes.data if r.size else None, r.size, raw_base, steps.ctypes.data if r.size else None, C.byref(err)), err)
    return steps


CALLS_COUNTS = ("sha_rows", "keccak_rows", "io_rows", "insn_rows", "nraw", "memory_ops", "logic_ops", "arithmetic_ops", "sha_extend_rows",
                "keccak_perms", "row_memory_ops")
assert len(CALLS_COUNTS) == _H["CALLS_COUNTS"]


class SegmentCallsStruct(C.Structure):
    """struct zkm_segment_calls: one segment as the emulator records it (include/zkm_hip.h "K segments' calls expanded in one set of
    launches")."""
    _fields_ = [("steps", CpuStepsStruct), ("first_clock", C.c_uint64), ("own", SegmentOpsStruct)] + \
               [(n, C.c_size_t if n.startswith("n") else C.c_void_p) for n in
                ("extend_w16", "extend_meta", "nextend", "compress_hx", "compress_w", "compress_meta", "ncompress", "keccak_inputs",
                 "keccak_input_off", "keccak_meta", "keccak_digest_addrs", "nkeccak", "io_kinds", "io_data", "io_data_off", "io_meta", "nio",
                 "insns", "insn_clocks", "ninsns")]


def abi_tagged_mirrors():
    """Every tagged struct of include/zkm_hip.h (abi.tagged()) -> its ctypes mirror; tests/test_calls_entry_abi.py compares each with what
    the C compiler says, as tests/test_abi.py does for abi_mirrors()."""
    return {"zkm_segment_calls": SegmentCallsStruct}


class SegmentCalls:
    """One segment with its calls, for segment_calls_steps and Context.segments_calls_expand / segments_tables_calls /
    prove_segments_ops_calls (include/zkm_hip.h struct zkm_segment_calls).  The arguments are Context.calls_expand's: steps, a CpuSteps
    with the segment's own RAW rows (host memory) and a placeholder at every row of a call; extend = (w16, meta), compress = (hx, w,
    meta), keccak = (inputs, input_off, meta, digest_addrs), io = (kinds, data, data_off, meta), insns = (records, clocks); memory_ops /
    logic_ops / arithmetic_ops / keccak_perms = (inputs, timestamps): the segment's own operations; groups: the other groups of
    SegmentOps, passed on."""

    def __init__(self, steps, first_clock=0, extend=None, compress=None, keccak=None, memory_ops=None, logic_ops=None, keccak_perms=None,
                 io=None, insns=None, arithmetic_ops=None, **groups):
        self.steps, self.first_clock = steps, int(first_clock)
        self.own = SegmentOps(None, memory_ops, arithmetic_ops=arithmetic_ops, logic_ops=logic_ops, keccak=keccak_perms, **groups)
        e, c, ne, nc = Context._sha_lists(extend, compress)
        k, nk = Context._keccak_lists(keccak)
        i, ni = _io_lists(io)
        q, nq = _insn_lists(insns)
        self.lists = {}
        for names, vals in ((("extend_w16", "extend_meta"), e), (("compress_hx", "compress_w", "compress_meta"), c),
                            (("keccak_inputs", "keccak_input_off", "keccak_meta", "keccak_digest_addrs"), k),
                            (("io_kinds", "io_data", "io_data_off", "io_meta"), i), (("insns", "insn_clocks"), q)):
            if vals is not None:
                self.lists.update(zip(names, vals))
        self.counts = {"nextend": ne, "ncompress": nc, "nkeccak": nk, "nio": ni, "ninsns": nq}

    def struct(self):
        st = SegmentCallsStruct()
        st.steps, st.first_clock, st.own = self.steps.struct(), self.first_clock, self.own.struct()
        for name, v in self.lists.items():
            setattr(st, name, v.ptr if isinstance(v, DeviceBuffer) else (v.ctypes.data if v.size else None))
        for name, n in self.counts.items():
            setattr(st, name, n)
        return st


def segment_calls_steps(calls):
    """zkm_segment_calls_steps on a SegmentCalls: the host half of the expansion; needs no GPU.  Returns (the patched step list, a
    CPU_STEP_DT array with every call's RAW record at clock - first_clock; {name: count} for CALLS_COUNTS).  Every refusal raises
    ZkmError."""
    st, err = calls.struct(), C.c_char_p()
    steps, counts = np.zeros(calls.steps.steps.size, dtype=CPU_STEP_DT), (C.c_size_t * len(CALLS_COUNTS))()
    _check(load().zkm_segment_calls_steps(C.addressof(st), steps.ctypes.data if steps.size else None, counts, C.byref(err)), err)
    return steps, dict(zip(CALLS_COUNTS, (int(x) for x in counts)))


class CtlLocation(C.Structure):
    """zkm_ctl_location: one occurrence of a reported tuple (side of the lookup, index of the table, row)."""
    _fields_ = [("side", C.c_uint32), ("table", C.c_uint32), ("row", C.c_uint64)]


class CtlReport(C.Structure):
    """zkm_ctl_report (include/zkm_hip.h): what zkm_check_ctls found.  kind 0 consistent, 1 non-binary filter, 2 multisets differ,
    3 the check could not be made; .message holds the text of the error channel (None when consistent)."""
    _fields_ = [("kind", C.c_uint32), ("ctl", C.c_uint32), ("attempts", C.c_uint32), ("host_waits", C.c_uint32),
                ("side", C.c_uint32), ("table", C.c_uint32), ("row", C.c_uint64), ("filter_value", C.c_uint64),
                ("width", C.c_uint32), ("nwords", C.c_uint32), ("tuple", C.c_uint64 * 64),
                ("looking_count", C.c_uint64), ("looked_count", C.c_uint64),
                ("nlooking_locations", C.c_uint32), ("nlooked_locations", C.c_uint32),
                ("looking", CtlLocation * 8), ("looked", CtlLocation * 8)]
    message = None

    def tuple_words(self):
        return [int(self.tuple[k]) for k in range(self.nwords)]

    def looking_locations(self):
        return [(l.side, l.table, l.row) for l in self.looking[:self.nlooking_locations]]

    def looked_locations(self):
        return [(l.side, l.table, l.row) for l in self.looked[:self.nlooked_locations]]


VERIFY_CODES = tuple(abi.constants("ZKM_VERIFY_"))
(VERIFY_OK, VERIFY_SHAPE, VERIFY_TRANSCRIPT_STATE, VERIFY_CTL_CHALLENGES, VERIFY_QUOTIENT, VERIFY_POW, VERIFY_INITIAL_MERKLE, VERIFY_FRI_EVAL,
 VERIFY_FRI_MERKLE, VERIFY_FINAL_POLY, VERIFY_CTL_SUM, VERIFY_FAILED) = (_H["VERIFY_" + n] for n in VERIFY_CODES)
assert VERIFY_FAILED == len(VERIFY_CODES) - 1


class VerifyReport(C.Structure):
    """zkm_verify_report (include/zkm_hip.h): the verdict of zkm_verify_* on one proof.  code = VERIFY_* (the check that failed, 0 when
    the proof is accepted); .message holds the text of the error channel for the first rejected proof of a call (None otherwise)."""
    _fields_ = [(n, C.c_uint32) for n in ("code", "table", "challenge", "query", "tree", "layer", "ctl", "host_waits")]
    message = None

    @property
    def name(self):
        return VERIFY_CODES[self.code] if self.code < len(VERIFY_CODES) else "?%d" % self.code

    def key(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


def abi_mirrors():
    """Every struct of include/zkm_hip.h -> its Python mirror (a ctypes Structure or a numpy dtype); tests/test_abi.py compares
    size, alignment and field offsets of each with what the C compiler says (abi.layout_probe_source)."""
    from . import ctl
    return {"zkm_challenger": Challenger, "zkm_stark_config": StarkConfig, "zkm_proof_layout": ProofLayout,
            "zkm_proof_query_layout": ProofQueryLayout, "zkm_column": ctl.COLUMN_DT, "zkm_colset": ctl.COLSET_DT,
            "zkm_ctl_table": ctl.CtlTableStruct, "zkm_ctl_z": ctl.CTLZ_DT, "zkm_ctl_side": ctl.SIDE_DT,
            "zkm_cross_table_lookup": ctl.CTL_DT, "zkm_table_input": ctl.TableInputStruct, "zkm_fri_poly": FriPoly,
            "zkm_fri_batch": FriBatch, "zkm_segment_ops": SegmentOpsStruct, "zkm_boot_image": BootImageStruct,
            "zkm_cpu_step": CPU_STEP_DT, "zkm_cpu_steps": CpuStepsStruct, "zkm_image_pages": ImagePagesStruct,
            "zkm_ctl_location": CtlLocation, "zkm_ctl_report": CtlReport, "zkm_verify_report": VerifyReport}


# the structs the binding passes by reference: a pointer to one of them is POINTER(its mirror); every other struct pointer (arrays packed
# by zkm_amd/ctl.py, handles) is a plain address
BY_REFERENCE = ("zkm_stark_config", "zkm_challenger", "zkm_segment_ops", "zkm_boot_image", "zkm_cpu_steps", "zkm_image_pages", "zkm_ctl_report",
                "zkm_verify_report", "zkm_proof_layout", "zkm_proof_query_layout")
_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
_COUNTS = {"size_t": C.c_size_t, "unsigned": C.c_uint, "int": C.c_int, "double": C.c_double}    # pointees that stay typed: never device memory
_DATA = ("void", "uint8_t", "uint32_t", "uint64_t")    # device addresses as integers, host arrays as casts: c_void_p takes both


def _ctype(text, mirrors, ret=False):
    """The ctypes type of a parameter or return type of the header; a type the rules below do not name raises ZkmError."""
    base = " ".join(w for w in text.replace("*", " ").split() if w != "const")
    stars = text.count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 0 and base == "void" and ret:
        return None
    if base == "char" and stars in (1, 2) and (stars == 2 or text.startswith("const ")):
        return C.c_char_p if stars == 1 else C.POINTER(C.c_char_p)
    known = base in _SCALARS or base in _COUNTS or base in _DATA or base in abi.structs() or base in abi.opaque()
    if stars and known and ret:
        return C.c_void_p
    if stars >= 2 and known:
        return C.POINTER(C.c_void_p)
    if stars == 1 and base in _COUNTS:
        return C.POINTER(_COUNTS[base])
    if stars == 1 and base in BY_REFERENCE:
        return C.POINTER(mirrors[base])
    if stars == 1 and known:
        return C.c_void_p
    raise ZkmError("include/zkm_hip.h: no ctypes binding for the C type %r" % text)


_lib = None


def load():
    """Load the extension (no GPU needed just to load and resolve symbols) and give every function of include/zkm_hip.h its argument and
    return types."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ZkmError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % _LIB_PATH)
    L = C.CDLL(_LIB_PATH)
    mirrors = abi_mirrors()
    for name, ret, params in abi.prototypes():
        fn = getattr(L, name, None)
        if fn is None:
            raise ZkmError("%s does not export %s, which include/zkm_hip.h declares: rebuild it" % (_LIB_PATH, name))
        fn.restype = _ctype(ret, mirrors, ret=True)
        fn.argtypes = [_ctype(ty, mirrors) for ty, _ in params]
    _lib = L
    return L


def _np_ptr(a):
    assert isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def _check(rc, err):
    if rc != 0:
        msg = err.value.decode() if err.value else "error %d" % rc
        # message was malloc'd by the library (reference convention: caller frees)
        raise ZkmError(msg)


class DeviceBuffer:
    """A chunk of HBM owned by a Context (uint64 words)."""

    def __init__(self, ctx, words):
        self.ctx, self.words = ctx, words
        p = C.c_void_p()
        err = C.c_char_p()
        _check(ctx.L.zkm_dev_alloc(ctx.h, words * 8, C.byref(p), C.byref(err)), err)
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        assert arr.size <= self.words
        err = C.c_char_p()
        _check(self.ctx.L.zkm_dev_upload(self.ctx.h, self.ptr, _np_ptr(arr), arr.size * 8, C.byref(err)), err)
        return self

    def download(self, words=None, offset=0):
        words = self.words - offset if words is None else words
        out = np.empty(words, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.ctx.L.zkm_dev_download(self.ctx.h, _np_ptr(out), self.ptr + 8 * offset, words * 8, C.byref(err)), err)
        return out

    def free(self):
        if self.ptr:
            self.ctx.L.zkm_dev_free(self.ctx.h, self.ptr)
            self.ptr = None


class _StagedHandle:
    """The lifetime every handle of input put into HBM shares (StagedTrace, StagedOps, StagedSteps, ExpandedCalls, StagedCalls): the
    context keeps track of it (Context.close() frees what is outstanding), and it is freed when dropped, at the end of a `with` block
    or by free(), once.  A subclass names the C function that frees the handle: _free."""
    _free = None

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle
        ctx._staged.add(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def free(self):
        """Waits for the queued work and returns the handle's blocks (see include/zkm_hip.h); the host source may go after this.  A no-op on
        a handle that has been freed, by the caller or by Context.close()."""
        if self.h:
            h, self.h = self.h, None
            self.ctx._staged.discard(self)
            if self.ctx.h:
                getattr(self.ctx.L, self._free)(h)


class _InFlightHandle(_StagedHandle):
    """... of a handle whose work may still be in flight when the call that made it returns: ready() asks the C function _ready."""
    _ready = None

    def ready(self, wait=False):
        """Has the queued work ended?  wait=True blocks until it has."""
        r = getattr(self.ctx.L, self._ready)(self.h, 1 if wait else 0)
        if r < 0:
            raise ZkmError("%s: runtime error" % self._ready)
        return bool(r)


class StagedTrace(_InFlightHandle):
    """zkm_staged: a host matrix on its way into HBM behind the context's current work (include/zkm_hip.h "staged traces").  Pass it
    wherever a prove call of the SAME context takes a trace; free() after that call has returned.  A handle that is dropped, leaves a
    `with` block or outlives Context.close() is freed then (free() after close() is a no-op: the context freed it)."""

    _free, _ready = "zkm_staged_free", "zkm_staged_ready"

    def __init__(self, ctx, handle, words):
        _StagedHandle.__init__(self, ctx, handle)
        self.words = words

    @property
    def ptr(self):
        p = self.ctx.L.zkm_staged_ptr(self.h)
        if not p:
            raise ZkmError("zkm_staged_ptr: the upload could not be ordered before the compute stream")
        return p

    def tables(self):
        """A staged SEGMENT's twelve device matrices (integers), ordered behind the upload: traces[s] of prove_segments."""
        out = (C.c_void_p * 12)()
        if self.ctx.L.zkm_staged_segment_ptrs(self.h, out) != 0:
            raise ZkmError("zkm_staged_segment_ptrs: not a staged segment, or the upload could not be ordered before the compute stream")
        return [int(out[t]) for t in range(12)]


def _data_ptr(x):
    """Accept numpy host arrays, DeviceBuffers, staged traces, raw integer device pointers or torch CUDA tensors."""
    if isinstance(x, (DeviceBuffer, StagedTrace)):
        return C.c_void_p(x.ptr)
    if isinstance(x, np.ndarray):
        return _np_ptr(x)
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    raise TypeError("unsupported buffer type %r" % type(x))


class SegmentOps:
    """A segment's raw operations -- the reference's Traces (witness/traces.rs:47-62) -- for Context.segment_tables / prove_segment_ops.
    Every list has the layout of its per-table entry point (include/zkm_hip.h zkm_segment_ops) and is a numpy array (pageable, or a
    view of Context.pinned_array memory) or a DeviceBuffer; the sponge offsets stay numpy.  Groups given as tuples:
      poseidon            (inputs n x 12 u64, timestamps n u64)
      poseidon_sponge     (inputs u8, off n + 1 u64, meta n x 4 u64)               keccak_sponge   the same
      keccak              (inputs n x 25 u64, timestamps n u64)
      sha_extend          (inputs n x 16 u8, timestamps n u64)                     sha_extend_sponge   (w16 n x 16 u32, meta n x 4 u64)
      sha_compress        (hx n x 8 u32, w n x 64 u32, meta n x 8 u64)            sha_compress_sponge the same
    cpu_rows: ncpu_rows x 259 u64, row-major (any shape); arithmetic / logic: n x 3 u32; memory: n x 6 u64.  Counts come from the sizes
    (a DeviceBuffer holds ceil(bytes / 8) words)."""

    DTYPES = {"cpu_rows": np.uint64, "arithmetic_ops": np.uint32, "logic_ops": np.uint32, "memory_ops": np.uint64, "poseidon_inputs": np.uint64,
              "poseidon_timestamps": np.uint64, "poseidon_sponge_inputs": np.uint8, "poseidon_sponge_off": np.uint64,
              "poseidon_sponge_meta": np.uint64, "keccak_inputs": np.uint64, "keccak_timestamps": np.uint64, "keccak_sponge_inputs": np.uint8,
              "keccak_sponge_off": np.uint64, "keccak_sponge_meta": np.uint64, "sha_extend_inputs": np.uint8, "sha_extend_timestamps": np.uint64,
              "sha_extend_sponge_w16": np.uint32, "sha_extend_sponge_meta": np.uint64, "sha_compress_hx": np.uint32, "sha_compress_w": np.uint32,
              "sha_compress_meta": np.uint64, "sha_compress_sponge_hx": np.uint32, "sha_compress_sponge_w": np.uint32,
              "sha_compress_sponge_meta": np.uint64}

    def __init__(self, cpu_rows, memory_ops, arithmetic_ops=None, logic_ops=None, poseidon=None, poseidon_sponge=None, keccak=None,
                 keccak_sponge=None, sha_extend=None, sha_extend_sponge=None, sha_compress=None, sha_compress_sponge=None):
        given = {"cpu_rows": (cpu_rows,), "memory": (memory_ops,), "arithmetic": (arithmetic_ops,), "logic": (logic_ops,),
                 "poseidon": poseidon, "poseidon_sponge": poseidon_sponge, "keccak": keccak, "keccak_sponge": keccak_sponge,
                 "sha_extend": sha_extend, "sha_extend_sponge": sha_extend_sponge, "sha_compress": sha_compress,
                 "sha_compress_sponge": sha_compress_sponge}
        self.lists, self.counts = {}, {}
        for group, ptrs, count in SEGMENT_OPS_GROUPS:
            vals = given[group] if given[group] is not None else (None,) * len(ptrs)
            assert len(vals) == len(ptrs), group
            n = 0
            for (name, item), v in zip(ptrs, vals):
                if v is None:
                    continue
                if not isinstance(v, DeviceBuffer):
                    v = np.ascontiguousarray(v, dtype=self.DTYPES[name]).reshape(-1)
                self.lists[name] = v
                if name.endswith("_off"):               # a sponge group: counted by its offsets
                    n = v.size - 1
                elif name == ptrs[0][0] and item:       # any other group: by its first list
                    n = (v.words * 8 if isinstance(v, DeviceBuffer) else v.nbytes) // item
            self.counts[count] = n

    def to_device(self, ctx):
        """The same operations with every list (the sponge offsets excepted) copied into DeviceBuffers of ctx."""
        return self._copy(lambda a: ctx.alloc((a.nbytes + 7) // 8).upload(_as_words(a)))

    def to_pinned(self, ctx):
        """The same operations with every list copied into page-locked host memory (Context.pinned_array)."""
        def pin(a):
            p = ctx.pinned_array((a.nbytes + 7) // 8)
            p.view(np.uint8)[:a.nbytes] = a.view(np.uint8)
            return p.view(a.dtype)[:a.size]
        return self._copy(pin)

    def _copy(self, fn):
        out = SegmentOps.__new__(SegmentOps)
        out.lists = {k: (v if k.endswith("_off") or isinstance(v, DeviceBuffer) else fn(v)) for k, v in self.lists.items()}
        out.counts = dict(self.counts)
        return out

    def free(self):
        """Free the DeviceBuffers (to_device's copies)."""
        for v in self.lists.values():
            if isinstance(v, DeviceBuffer):
                v.free()

    def struct(self):
        if getattr(self, "_staged_struct", None) is not None:    # StagedOps.ops(): device pointers the library handed out
            return self._staged_struct
        st = SegmentOpsStruct()
        for name, v in self.lists.items():
            setattr(st, name, v.ptr if isinstance(v, DeviceBuffer) else v.ctypes.data)
        for count, n in self.counts.items():
            setattr(st, count, n)
        return st


class BootImage:
    """A segment's memory image for the *_boot calls (include/zkm_hip.h zkm_boot_image): the bootstrap kernel's CPU rows, memory
    operations, Poseidon inputs and sponge rows are built from it on the device.  addrs / values: uint32 numpy arrays (or DeviceBuffers
    with nwords given) in ascending address order; root / image_id: 32 bytes each; npages: the page-aligned addresses, counted here
    when the addresses are a numpy array.  check: refuse a page hash, root hash or image id that does not match."""

    def __init__(self, addrs, values, root, image_id, entry, check=True, npages=None, nwords=None):
        host = not isinstance(addrs, DeviceBuffer)
        self.addrs = np.ascontiguousarray(addrs, dtype=np.uint32).reshape(-1) if host else addrs
        self.values = values if isinstance(values, DeviceBuffer) else np.ascontiguousarray(values, dtype=np.uint32).reshape(-1)
        self.nwords = int(self.addrs.size if host else nwords)
        self.npages = int(np.count_nonzero((self.addrs & 0xFFF) == 0)) if npages is None else int(npages)
        self.root, self.image_id, self.entry, self.check = bytes(root), bytes(image_id), int(entry), bool(check)
        assert len(self.root) == 32 and len(self.image_id) == 32

    @classmethod
    def from_dict(cls, image, root, image_id, entry, **kw):
        """image: {addr: value} (the reference's BTreeMap<u32, u32>)."""
        addrs = sorted(image)
        return cls(np.array(addrs, dtype=np.uint32), np.array([image[a] for a in addrs], dtype=np.uint32), root, image_id, entry, **kw)

    def struct(self):
        st = BootImageStruct()
        st.addrs = self.addrs.ptr if isinstance(self.addrs, DeviceBuffer) else self.addrs.ctypes.data
        st.values = self.values.ptr if isinstance(self.values, DeviceBuffer) else self.values.ctypes.data
        st.nwords, st.npages, st.entry, st.check = self.nwords, self.npages, self.entry, int(self.check)
        st.pre_hash_root[:] = self.root
        st.pre_image_id[:] = self.image_id
        return st

    def counts(self):
        """zkm_boot_counts: (cpu_rows, memory_ops, poseidon_inputs, sponge_ops, sponge_rows) of the bootstrap."""
        out = [C.c_size_t() for _ in range(5)]
        load().zkm_boot_counts(C.byref(self.struct()), *[C.byref(x) for x in out])
        return tuple(int(x.value) for x in out)


def image_hash_plan(indices):
    """zkm_image_hash_plan: the ascending hash pages (L1 pages, L2 pages, the root 0x81020) that hashing these ascending dirty page
    indices writes, as a uint32 array."""
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    L = load()
    n = L.zkm_image_hash_plan(idx.ctypes.data, idx.size, None, 0)
    out = np.zeros(n, dtype=np.uint32)
    L.zkm_image_hash_plan(idx.ctypes.data, idx.size, out.ctypes.data, n)
    return out


def _pages_ptr(words, n):
    """Page words for zkm_image_pages: a host array of n x 1024 uint32 (returned too: it must outlive the call) or device memory."""
    if words is None or isinstance(words, (np.ndarray, list, tuple)):
        a = np.ascontiguousarray(words if words is not None else [], dtype=np.uint32).reshape(-1)
        assert a.size == 1024 * n, "%d page words for %d pages" % (a.size, n)
        return a.ctypes.data if n else None, a
    return _data_ptr(words).value, words


def boot_image_from_pages(dirty, plan, hash_pages, root, image_id, entry, check=True):
    """The BootImage of a memory that holds the dirty pages (indices, n x 1024 words) and the hash pages of an image_hash result: every
    word of every page as addrs / values, pre_hash_root and pre_image_id from the call."""
    index = np.concatenate([np.asarray(dirty[0], dtype=np.uint32).reshape(-1), np.asarray(plan, dtype=np.uint32).reshape(-1)])
    words = np.concatenate([np.asarray(dirty[1], dtype=np.uint32).reshape(-1, 1024), np.asarray(hash_pages, dtype=np.uint32).reshape(-1, 1024)])
    assert len(index) == len(words) and (np.diff(index.astype(np.int64)) > 0).all()
    addrs = ((index.astype(np.uint64)[:, None] << np.uint64(12)) + np.arange(0, 4096, 4, dtype=np.uint64)[None, :]).astype(np.uint32)
    return BootImage(addrs.reshape(-1), words.reshape(-1), root, image_id, entry, check=check)


class StagedOps(_InFlightHandle):
    """zkm_staged_ops: a segment's raw operations on their way into HBM behind the context's current work (include/zkm_hip.h "Staged
    operations").  ops() is the same segment with device pointers, for segment[s]_tables / prove_segment[s]_ops of the SAME context;
    free() after that call has returned.  Freed like a StagedTrace when dropped, at the end of a `with` block or by Context.close()."""

    _free, _ready = "zkm_staged_ops_free", "zkm_staged_ops_ready"

    def ops(self):
        """A SegmentOps of device pointers, ordered behind the upload on the device (no host wait)."""
        st = SegmentOpsStruct()
        if not self.h or self.ctx.L.zkm_staged_ops_get(self.h, C.byref(st)) != 0:
            raise ZkmError("zkm_staged_ops_get: freed handle, or the upload could not be ordered before the compute stream")
        out = SegmentOps.__new__(SegmentOps)
        out.lists, out.counts, out._staged_struct, out._owner = {}, {}, st, self
        return out


class _StagedStepsSegment:
    """A segment's staged step log as StagedSteps.get hands it out: device pointers the handle owns, and the three list lengths."""

    def __init__(self, st, counts, owner):
        self._st, self._owner, self.counts_, self.nsteps, self.nraw = st, owner, counts, st.nsteps, st.nraw

    def struct(self):
        return self._st

    def counts(self):
        return self.counts_


class StagedSteps(_InFlightHandle):
    """The handle of zkm_cpu_steps_stage: K segments' step logs on their way into HBM behind the context's current work, walked on the
    device behind the upload (include/zkm_hip.h "Staged steps").  get(s) is what segments_tables_steps / prove_segments_ops_steps of
    the SAME context take for segment s; free() after those calls have returned.  The CpuSteps it was staged from are kept alive by
    the handle, and their arrays must stay as they are until ready() is true.  Freed when dropped, at the end of a `with` block or by
    Context.close()."""

    _free, _ready = "zkm_staged_steps_free", "zkm_staged_steps_ready"

    def __init__(self, ctx, handle, steps_list):
        _StagedHandle.__init__(self, ctx, handle)
        self.steps_list = list(steps_list)

    def __len__(self):
        return len(self.steps_list)

    def get(self, s):
        """zkm_staged_steps_get: segment s with device pointers (waits on the host for the walk the first time, one wait a handle at
        most); a segment the walk refused raises ZkmError with the host walk's message."""
        if not self.h:
            raise ZkmError("zkm_staged_steps_get: freed handle")
        st, n, err = CpuStepsStruct(), [C.c_size_t() for _ in range(3)], C.c_char_p()
        _check(self.ctx.L.zkm_staged_steps_get(self.h, s, C.byref(st), *[C.byref(x) for x in n], C.byref(err)), err)
        return _StagedStepsSegment(st, tuple(int(x.value) for x in n), self)


class _ExpandedSteps:
    """A segment's patched step list as ExpandedCalls hands it out: .steps a numpy copy, raw_rows on the device (the handle's)."""

    def __init__(self, st, owner):
        self._st, self._owner, self.nraw, self.raw_rows_ptr = st, owner, st.nraw, st.raw_rows
        self.steps = np.ctypeslib.as_array(C.cast(st.steps, C.POINTER(C.c_uint8)), (st.nsteps * 48,)).view(CPU_STEP_DT).copy() if st.nsteps \
            else np.zeros(0, dtype=CPU_STEP_DT)

    def struct(self):
        return self._st


class ExpandedCalls(_StagedHandle):
    """struct zkm_expanded_calls: the expanded calls of K segments (Context.segments_calls_expand).  segment(s) gives what
    segments_tables_steps / prove_segments_ops_steps take for segment s; the SegmentCalls' lists must stay as they are until free().
    Freed like a StagedTrace when dropped, at the end of a `with` block or by Context.close()."""

    _free = "zkm_expanded_calls_free"

    def __init__(self, ctx, handle, calls):
        _StagedHandle.__init__(self, ctx, handle)
        self.calls = list(calls)

    def __len__(self):
        return len(self.calls)

    def structs(self, s):
        """(CpuStepsStruct, SegmentOpsStruct) of segment s, as zkm_expanded_calls_get fills them."""
        st, ops = CpuStepsStruct(), SegmentOpsStruct()
        if not self.h or self.ctx.L.zkm_expanded_calls_get(self.h, s, C.byref(st), C.byref(ops)) != 0:
            raise ZkmError("zkm_expanded_calls_get: freed handle, or no segment %d" % s)
        return st, ops

    def segment(self, s):
        """(steps, ops) of segment s for segments_tables_steps / prove_segments_ops_steps: device pointers the handle owns."""
        st, o = self.structs(s)
        ops = SegmentOps.__new__(SegmentOps)
        ops.lists, ops.counts, ops._staged_struct, ops._owner = {}, {}, o, self
        return _ExpandedSteps(st, self), ops

    def download(self, s):
        """Segment s's outputs as numpy arrays, for comparisons: steps, nraw, raw_rows (nraw x 259) and every list of the operations that
        lies in device memory, under its zkm_segment_ops name; "counts": every count of the operations."""
        st, o = self.structs(s)
        return self._download(st, o, s)

    def _download(self, st, o, s):
        def down(ptr, n, dtype, shape):
            out = np.zeros(n, dtype=dtype)
            if n:
                err = C.c_char_p()
                _check(self.ctx.L.zkm_dev_download(self.ctx.h, out.ctypes.data, ptr, out.nbytes, C.byref(err)), err)
            return out.reshape(shape)
        got = {"steps": _ExpandedSteps(st, self).steps, "nraw": st.nraw, "raw_rows": down(st.raw_rows, st.nraw * 259, np.uint64, (-1, 259)),
               "memory_ops": down(o.memory_ops, o.nmemory * 6, np.uint64, (-1, 6)), "logic_ops": down(o.logic_ops, o.nlogic * 3, np.uint32, (-1, 3)),
               "keccak_inputs": down(o.keccak_inputs, o.nkeccak * 25, np.uint64, (-1, 25)), "keccak_timestamps": down(o.keccak_timestamps, o.nkeccak, np.uint64, (-1,)),
               "sha_extend_inputs": down(o.sha_extend_inputs, o.nsha_extend * 16, np.uint8, (-1, 16)),
               "sha_extend_timestamps": down(o.sha_extend_timestamps, o.nsha_extend, np.uint64, (-1,)),
               "counts": {count: getattr(o, count) for _, _, count in SEGMENT_OPS_GROUPS}}
        if self.calls[s].counts["ninsns"]:
            got["arithmetic_ops"] = down(o.arithmetic_ops, o.narithmetic * 3, np.uint32, (-1, 3))
        return got


class _StagedImage:
    """A segment's boot image as StagedCalls.get hands it out: addrs / values in device memory (the handle's)."""

    def __init__(self, st, owner):
        self._st, self._owner, self.nwords = st, owner, st.nwords

    def struct(self):
        return self._st


class StagedCalls(ExpandedCalls, _InFlightHandle):
    """The handle of zkm_segments_calls_stage: K segments' calls on their way into HBM behind the context's current work -- expanded,
    their records placed into the step list and the list walked on the device (include/zkm_hip.h "Staged calls").  get(s) is what
    segments_tables_steps / prove_segments_ops_steps of the SAME context take for segment s; free() after those calls have returned.
    The SegmentCalls (and BootImages) it was staged from are kept alive by the handle, and their arrays must stay as they are until
    ready() is true.  Freed when dropped, at the end of a `with` block or by Context.close()."""

    _free, _ready = "zkm_staged_calls_free", "zkm_staged_calls_ready"

    def __init__(self, ctx, handle, calls, images=None):
        ExpandedCalls.__init__(self, ctx, handle, calls)
        self.images = None if images is None else list(images)

    def structs(self, s, image=False):
        """(CpuStepsStruct, SegmentOpsStruct[, BootImageStruct]) of segment s, as zkm_staged_calls_get fills them (waits on the host for
        the handle's events the first time, one wait a handle at most); a refused segment raises ZkmError with the refusal's text."""
        if not self.h:
            raise ZkmError("zkm_staged_calls_get: freed handle")
        st, ops, im, err = CpuStepsStruct(), SegmentOpsStruct(), BootImageStruct(), C.c_char_p()
        _check(self.ctx.L.zkm_staged_calls_get(self.h, s, C.byref(st), C.byref(ops), C.byref(im), C.byref(err)), err)
        return (st, ops, im) if image else (st, ops)

    def get(self, s):
        """(steps, ops, image) of segment s for segments_tables_steps / prove_segments_ops_steps: device pointers the handle owns; image is
        None when the calls were staged without images."""
        st, o, im = self.structs(s, image=True)
        ops = SegmentOps.__new__(SegmentOps)
        ops.lists, ops.counts, ops._staged_struct, ops._owner = {}, {}, o, self
        n = _StagedStepsSegment(st, None, self)
        return n, ops, (None if self.images is None else _StagedImage(im, self))

    def segment(self, s):
        return self.get(s)[:2]

    def download(self, s):
        """As ExpandedCalls.download, the patched steps from device memory too."""
        st, o = self.structs(s)
        steps = np.zeros(st.nsteps, dtype=CPU_STEP_DT)
        if st.nsteps:
            err = C.c_char_p()
            _check(self.ctx.L.zkm_dev_download(self.ctx.h, steps.ctypes.data, st.steps, steps.nbytes, C.byref(err)), err)
        host = CpuStepsStruct(steps.ctypes.data, st.nsteps, st.raw_rows, st.nraw)
        return self._download(host, o, s)


class _marshal_ops:
    """The argument arrays of zkm_[pool_]prove_segments_ops for a list of SegmentOps and one array of public values per segment."""

    def __init__(self, ops_list, public_values, cfg, images=None):
        K = len(ops_list)
        self.keep = list(ops_list)
        if images is not None:
            assert len(images) == K, "one image per segment"
            self.im = (BootImageStruct * max(K, 1))(*[i.struct() for i in images])
        self.st = (SegmentOpsStruct * max(K, 1))(*[o.struct() for o in ops_list])
        pv = list(public_values) if public_values is not None else [()] * K
        assert len(pv) == K, "one array of public values per segment"
        self.pubs = [np.ascontiguousarray(p, dtype=np.uint64) for p in pv]
        self.pv = (C.c_void_p * max(K, 1))(*[p.ctypes.data for p in self.pubs])
        self.npv = (C.c_size_t * max(K, 1))(*[p.size for p in self.pubs])
        self.offs = (C.c_size_t * (13 * max(K, 1)))()
        self.K, self.cfg = K, cfg

    def alloc(self):
        """After the sizing call: the output buffers."""
        K = self.K
        self.sizes = [list(self.offs[13 * s:13 * s + 13]) for s in range(K)]
        self.proofs = [np.zeros(o[12], dtype=np.uint64) for o in self.sizes]
        self.chals = [np.zeros(2 * self.cfg.num_challenges, dtype=np.uint64) for _ in range(K)]
        self.po = (C.c_void_p * max(K, 1))(*[p.ctypes.data for p in self.proofs])
        self.co = (C.c_void_p * max(K, 1))(*[p.ctypes.data for p in self.chals])

    def results(self):
        return [(self.proofs[i], self.chals[i], self.sizes[i]) for i in range(self.K)]


def _as_words(a):
    """The bytes of a numpy array as uint64 words (zero-padded to a multiple of 8)."""
    b = np.zeros(((a.nbytes + 7) // 8) * 8, dtype=np.uint8)
    b[:a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return b.view(np.uint64)


class _marshal_segments:
    """The argument arrays of zkm_prove_segments[_columns] / zkm_pool_prove_segments[_columns] for segments = list of (traces, log_ns,
    public_values): traces[t] either one block per table or a list of per-column arrays (each its own allocation, like
    Vec<PolynomialValues<F>>).  Output buffers are sized with the sizing pass of zkm_prove_segment[_columns] (no context needed)."""

    def __init__(self, L, segments, cfg):
        K = len(segments)
        self.keep, self.ptr_arrays, self.log_arrays, self.pubs, self.sizes, self.col_arrays = [], [], [], [], [], []
        err = C.c_char_p()
        self.by_columns = all(isinstance(t, (list, tuple)) for seg in segments for t in seg[0])
        for traces, log_ns, public_values in segments:
            assert len(traces) == 12 and len(log_ns) == 12
            if self.by_columns:
                k = [[c if isinstance(c, (DeviceBuffer, StagedTrace)) else np.ascontiguousarray(c, dtype=np.uint64) for c in t] for t in traces]
                cols = [(C.c_void_p * len(t))(*[_data_ptr(c).value for c in t]) for t in k]
                self.col_arrays.append(cols)
                self.keep.append(k)
                self.ptr_arrays.append((C.c_void_p * 12)(*[C.addressof(c) for c in cols]))
            else:
                k = [t if isinstance(t, (DeviceBuffer, StagedTrace, int)) else np.ascontiguousarray(t, dtype=np.uint64) for t in traces]
                self.keep.append(k)
                self.ptr_arrays.append((C.c_void_p * 12)(*[_data_ptr(t).value for t in k]))
            self.log_arrays.append((C.c_uint * 12)(*[int(x) for x in log_ns]))
            self.pubs.append(np.ascontiguousarray(public_values, dtype=np.uint64))
            offs = (C.c_size_t * 13)()
            sizer = L.zkm_prove_segment_columns if self.by_columns else L.zkm_prove_segment
            _check(sizer(None, C.byref(cfg), self.ptr_arrays[-1], self.log_arrays[-1], self.pubs[-1].ctypes.data_as(u64p), self.pubs[-1].size, None,
                         offs, None, C.byref(err)), err)
            self.sizes.append(list(offs))
        self.proofs = [np.zeros(o[12], dtype=np.uint64) for o in self.sizes]
        self.chals = [np.zeros(2 * cfg.num_challenges, dtype=np.uint64) for _ in range(K)]
        self.tr = (C.c_void_p * K)(*[C.addressof(a) for a in self.ptr_arrays])
        self.lg = (C.c_void_p * K)(*[C.addressof(a) for a in self.log_arrays])
        self.pv = (C.c_void_p * K)(*[p.ctypes.data for p in self.pubs])
        self.npv = (C.c_size_t * K)(*[p.size for p in self.pubs])
        self.po = (C.c_void_p * K)(*[p.ctypes.data for p in self.proofs])
        self.co = (C.c_void_p * K)(*[p.ctypes.data for p in self.chals])

    def results(self):
        return [(self.proofs[i], self.chals[i], self.sizes[i]) for i in range(len(self.proofs))]


def pool_plan(nseg, workers, max_stack=0):
    """zkm_pool_plan: the sizes of the lock-step groups a pool call of nseg segments is cut into (a pure function of the library)."""
    L = load()
    n = L.zkm_pool_plan(nseg, workers, max_stack, None, 0)
    out = (C.c_size_t * max(1, n))()
    L.zkm_pool_plan(nseg, workers, max_stack, out, n)
    return [int(out[i]) for i in range(n)]


class Pool:
    """zkm_pool: `contexts_per_device` contexts on each of `devices`, one worker thread per context inside ONE process; a call cuts its
    segments into lock-step groups of at most max_stack and the workers pull them from a queue (include/zkm_hip.h).  The reference's
    one-process segment loop (prover/examples/utils/src/utils.rs:57-68, 105-133) over N GPUs."""

    def __init__(self, devices=(0,), contexts_per_device=1):
        self.L = load()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h, err = C.c_void_p(), C.c_char_p()
        _check(self.L.zkm_pool_create(devs, len(devices), contexts_per_device, C.byref(h), C.byref(err)), err)
        self.h = h

    def close(self):
        if self.h:
            self.L.zkm_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workers(self):
        return int(self.L.zkm_pool_workers(self.h))

    def device(self, worker):
        return int(self.L.zkm_pool_device(self.h, worker))

    def set_tuning(self, key, value):
        err = C.c_char_p()
        _check(self.L.zkm_pool_set_tuning(self.h, key.encode(), int(value), C.byref(err)), err)

    def standard_config(self):
        cfg = StarkConfig()
        self.L.zkm_standard_config(C.byref(cfg))
        return cfg

    def prove_segments(self, segments, max_stack=0, cfg=None):
        """zkm_pool_prove_segments[_columns]: segments as Context.prove_segments takes them (HOST arrays unless the pool has one device).
        Returns the list of (proofs, ctl_challenges, offsets), one per segment."""
        cfg = cfg or self.standard_config()
        m = _marshal_segments(self.L, segments, cfg)
        err = C.c_char_p()
        fn = self.L.zkm_pool_prove_segments_columns if m.by_columns else self.L.zkm_pool_prove_segments
        _check(fn(self.h, C.byref(cfg), len(segments), max_stack, m.tr, m.lg, m.pv, m.npv, m.po, m.co, C.byref(err)), err)
        return m.results()

    def prove_segments_ops(self, ops_list, public_values=None, max_stack=0, cfg=None):
        """zkm_pool_prove_segments_ops: one SegmentOps per segment (HOST lists unless the pool has one device), one array of public values
        per segment.  Each group is built and proven on its worker's context.  Returns (proofs, ctl_challenges, offsets) per segment."""
        cfg = cfg or self.standard_config()
        m, err = _marshal_ops(ops_list, public_values, cfg), C.c_char_p()
        _check(self.L.zkm_pool_prove_segments_ops(self.h, C.byref(cfg), m.K, max_stack, m.st, m.pv, m.npv, None, m.offs, None, C.byref(err)), err)
        m.alloc()
        _check(self.L.zkm_pool_prove_segments_ops(self.h, C.byref(cfg), m.K, max_stack, m.st, m.pv, m.npv, m.po, m.offs, m.co, C.byref(err)), err)
        return m.results()

    def prove_segments_calls(self, calls_list, images=None, public_values=None, max_stack=0, cfg=None, sizing=False):
        """zkm_pool_prove_segments_calls: one SegmentCalls per segment as Context.prove_segments_ops_calls takes them (HOST lists unless the
        pool has one device), behind one BootImage each where images is given.  Each worker keeps its next group staged behind the current
        proofs ("pool_stage_ahead", the default) or expands each group in its call.  Returns (proofs, ctl_challenges, offsets) per segment;
        sizing: the sizing call alone, the offsets per segment."""
        cfg = cfg or self.standard_config()
        m, err = _marshal_ops([q.own for q in calls_list], public_values, cfg, images), C.c_char_p()
        im = m.im if images is not None else None
        arr = Context._calls_array(calls_list)
        fn = self.L.zkm_pool_prove_segments_calls
        _check(fn(self.h, C.byref(cfg), m.K, max_stack, im, C.addressof(arr), m.pv, m.npv, None, m.offs, None, C.byref(err)), err)
        m.alloc()
        if sizing:
            return m.sizes
        _check(fn(self.h, C.byref(cfg), m.K, max_stack, im, C.addressof(arr), m.pv, m.npv, m.po, m.offs, m.co, C.byref(err)), err)
        return m.results()

    def memory(self, worker):
        """(live bytes, cached bytes) of worker w's context (zkm_pool_context, zkm_ctx_memory)."""
        live, cached = C.c_size_t(), C.c_size_t()
        self.L.zkm_ctx_memory(self.L.zkm_pool_context(self.h, worker), C.byref(live), C.byref(cached))
        return live.value, cached.value

    def resident_bytes(self, worker):
        """Bytes of the tables worker w's context keeps for reuse (zkm_ctx_resident_bytes): part of its live bytes."""
        return self.L.zkm_ctx_resident_bytes(self.L.zkm_pool_context(self.h, worker))

    def last_assignment(self, segment):
        """(worker, group) that proved `segment` in the last call."""
        w, g = C.c_size_t(), C.c_size_t()
        if self.L.zkm_pool_last_assignment(self.h, segment, C.byref(w), C.byref(g)) != 0:
            raise ZkmError("zkm_pool_last_assignment: segment %d was not proven by the last call" % segment)
        return int(w.value), int(g.value)


class Context:
    """One GPU context (single-owner, like the reference's &mut Challenger / &mut TimingTree threading)."""

    def __init__(self, device=0):
        self.L = load()
        h = C.c_void_p()
        err = C.c_char_p()
        _check(self.L.zkm_ctx_create(device, C.byref(h), C.byref(err)), err)
        self.h = h
        self._staged = weakref.WeakSet()     # outstanding StagedTraces: freed by close() before the context goes
        self.witness_message = None          # the message of the last witness_check / segment_witness_check (None: every constraint held)
        self.lookup_message = None           # ... of the last lookup_check / segment_lookup_check (None: every lookup held)
        self.check_message = None            # ... of the last segments_check / segment_check (None: every segment consistent)

    def close(self):
        if self.h:
            for st in list(getattr(self, "_staged", ())):    # (first: their uploads may read pinned arrays freed below)
                st.free()
            for p in list(getattr(self, "_pinned", {}).values()):
                self.L.zkm_host_free(self.h, p)
            self._pinned = {}
            self.L.zkm_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def memory(self):
        """(live bytes, cached bytes) of the context's device allocator."""
        live, cached = C.c_size_t(), C.c_size_t()
        self.L.zkm_ctx_memory(self.h, C.byref(live), C.byref(cached))
        return live.value, cached.value

    def host_waits(self):
        """zkm_ctx_host_waits: how often a host thread has waited for this context's stream so far."""
        return int(self.L.zkm_ctx_host_waits(self.h))

    def resident_bytes(self):
        """Of the live bytes: tables kept for reuse (twiddles, power tables; the commit lanes' included)."""
        return self.L.zkm_ctx_resident_bytes(self.h)

    def pinned_array(self, words):
        """A uint64 ndarray in page-locked host memory (zkm_host_alloc): uploads from it overlap with compute.  Freed with the
        context (or explicitly with free_pinned)."""
        p, err = C.c_void_p(), C.c_char_p()
        _check(self.L.zkm_host_alloc(self.h, words * 8, C.byref(p), C.byref(err)), err)
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(words,))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def free_pinned(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None:
            self.L.zkm_host_free(self.h, p)

    def trim(self):
        """Return the allocator's cached blocks to the device."""
        self.L.zkm_ctx_trim(self.h)

    def set_tuning(self, key, value):
        """Kernel-selection thresholds (include/zkm_hip.h: zkm_ctx_set_tuning); every setting yields the same words."""
        err = C.c_char_p()
        _check(self.L.zkm_ctx_set_tuning(self.h, key.encode(), int(value), C.byref(err)), err)

    def synchronize(self):
        err = C.c_char_p()
        _check(self.L.zkm_ctx_synchronize(self.h, C.byref(err)), err)

    @property
    def stream(self):
        return self.L.zkm_ctx_stream(self.h)

    def alloc(self, words):
        return DeviceBuffer(self, words)

    # ---- primitives
    def ntt(self, cols, ncols, log_n, inverse=False, coset_shift=0):
        """In-place batched NTT (natural order in/out).  `cols`: host ndarray or device buffer."""
        err = C.c_char_p()
        _check(self.L.zkm_ntt(self.h, _data_ptr(cols), ncols, log_n, int(inverse), coset_shift, C.byref(err)), err)
        return cols

    def field_selftest(self, a, b):
        """(a + b, a - b, a 2^24, a 2^48, a 2^72, a b, a b [branch-free product]) mod p through the device's loose-arithmetic primitives,
        for arbitrary 64-bit words."""
        a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
        out = np.zeros(7 * a.size, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.L.zkm_field_selftest(self.h, a.ctypes.data_as(u64p), b.ctypes.data_as(u64p), a.size, out.ctypes.data_as(u64p), C.byref(err)), err)
        return out.reshape(7, -1)

    def poseidon_selftest(self, probe, arg, words):
        """One piece of the device's Poseidon permutation on chosen words (zkm_poseidon_selftest; probe: POSEIDON_PROBE[name] or its number).
        `words`: n states of 12 words -- n pairs for FOLD / FOLD_TY, n triples (al, ah, cl + 2 ch) for FOLD_WIDE -- of any uint64.  Returns
        the raw words the device produced: an (n, 12) array, or n words for the folds."""
        probe = POSEIDON_PROBE[probe] if isinstance(probe, str) else int(probe)
        words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
        triples = probe == POSEIDON_PROBE["FOLD_WIDE"]
        pairs = triples or probe in (POSEIDON_PROBE["FOLD"], POSEIDON_PROBE["FOLD_TY"])
        per = 3 if triples else 2 if pairs else 12
        if words.size % per:
            raise ValueError("poseidon_selftest: %d words are not a whole number of %s" % (words.size, "triples" if triples else "pairs" if pairs else "states"))
        n = words.size // per
        out = np.zeros(n if pairs else 12 * n, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.L.zkm_poseidon_selftest(self.h, probe, int(arg), words.ctypes.data_as(u64p), n, out.ctypes.data_as(u64p), C.byref(err)), err)
        return out if pairs else out.reshape(-1, 12)

    def consumer_selftest(self, alphas, terms, run=8):
        """The quotient kernels' constraint consumer on chosen words (zkm_consumer_selftest): `terms` is a (K, n) array of any uint64
        -- lane l takes terms[:, l] in order, `run` at a time -- and `alphas` 1 or 2 challenges (any uint64).  Returns the
        (len(alphas), n) canonical accumulators sum_k terms[k] alpha^(K-1-k) mod p."""
        alphas = np.ascontiguousarray(alphas, dtype=np.uint64).reshape(-1)
        terms = np.ascontiguousarray(terms, dtype=np.uint64)
        if terms.ndim != 2:
            raise ValueError("consumer_selftest: terms must be a (K, n) array")
        K, n = terms.shape
        out = np.zeros(alphas.size * n, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.L.zkm_consumer_selftest(self.h, alphas.ctypes.data_as(u64p), alphas.size, terms.ctypes.data_as(u64p), K, n, int(run),
                                            out.ctypes.data_as(u64p), C.byref(err)), err)
        return out.reshape(alphas.size, n)

    def poseidon_permute_batch(self, states):
        k = (states.size if isinstance(states, np.ndarray) else states.words) // 12
        err = C.c_char_p()
        _check(self.L.zkm_poseidon_permute_batch(self.h, _data_ptr(states), k, C.byref(err)), err)
        return states

    def keccakf_batch(self, states):
        k = (states.size if isinstance(states, np.ndarray) else states.words) // 25
        err = C.c_char_p()
        _check(self.L.zkm_keccakf_batch(self.h, _data_ptr(states), k, C.byref(err)), err)
        return states

    def poseidon_trace(self, seed, num_perms, log_n, out=None):
        """PoseidonStark::generate_trace on the GPU; returns a DeviceBuffer of 262 x 2^log_n words."""
        out = out or self.alloc(POSEIDON_COLS << log_n)
        err = C.c_char_p()
        _check(self.L.zkm_poseidon_trace(self.h, seed, num_perms, log_n, _data_ptr(out), C.byref(err)), err)
        return out

    def keccak_sponge_trace(self, inputs, input_off, meta, log_n, out=None):
        """KeccakSpongeStark::generate_trace on the GPU (keccak_sponge_stark.rs:222-444).  inputs: uint8 array of all
        operations' bytes, input_off: nops+1 offsets, meta: nops x 4 (context, segment, virt_base, timestamp).
        Returns (DeviceBuffer of 470 x 2^log_n words, rows used)."""
        if isinstance(inputs, DeviceBuffer):      # message bytes already in HBM (packed into a word buffer): no upload inside the call
            in_ptr = C.c_void_p(inputs.ptr)
        else:
            inputs = np.ascontiguousarray(inputs, dtype=np.uint8)
            in_ptr = inputs.ctypes.data_as(C.c_void_p)
        input_off = np.ascontiguousarray(input_off, dtype=np.uint64)
        meta = np.ascontiguousarray(meta, dtype=np.uint64)
        nops = input_off.size - 1
        out = out or self.alloc(KECCAK_SPONGE_COLS << log_n)
        used = C.c_size_t()
        err = C.c_char_p()
        _check(self.L.zkm_keccak_sponge_trace(self.h, in_ptr, input_off.ctypes.data_as(u64p),
                                              meta.ctypes.data_as(u64p), nops, log_n, _data_ptr(out), C.byref(used), C.byref(err)), err)
        return out, used.value

    def poseidon_sponge_trace(self, inputs, input_off, meta, log_n, out=None):
        """PoseidonSpongeStark::generate_trace on the GPU (poseidon_sponge_stark.rs:186-381); arguments as keccak_sponge_trace.
        Returns (DeviceBuffer of 110 x 2^log_n words, rows used)."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint8)
        input_off = np.ascontiguousarray(input_off, dtype=np.uint64)
        meta = np.ascontiguousarray(meta, dtype=np.uint64)
        out = out or self.alloc(POSEIDON_SPONGE_COLS << log_n)
        used = C.c_size_t()
        err = C.c_char_p()
        _check(self.L.zkm_poseidon_sponge_trace(self.h, inputs.ctypes.data_as(C.c_void_p), input_off.ctypes.data_as(u64p),
                                                meta.ctypes.data_as(u64p), input_off.size - 1, log_n, _data_ptr(out), C.byref(used),
                                                C.byref(err)), err)
        return out, used.value

    def poseidon_trace_inputs(self, inputs, timestamps, log_n, out=None):
        """PoseidonStark::generate_trace for explicit inputs (num_perms x 12) and timestamps; DeviceBuffer of 262 x 2^log_n."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1, 12)
        timestamps = np.ascontiguousarray(timestamps, dtype=np.uint64)
        out = out or self.alloc(POSEIDON_COLS << log_n)
        err = C.c_char_p()
        _check(self.L.zkm_poseidon_trace_inputs(self.h, _data_ptr(inputs), _data_ptr(timestamps), len(inputs), log_n, _data_ptr(out),
                                                C.byref(err)), err)
        return out

    def sha_extend_trace(self, inputs, timestamps, log_n, out=None):
        """ShaExtendStark::generate_trace on the GPU: inputs nrows x 16 bytes, one timestamp per row; 78 x 2^log_n words."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint8).reshape(-1, 16)
        timestamps = np.ascontiguousarray(timestamps, dtype=np.uint64)
        out = out or self.alloc(78 << log_n)
        err = C.c_char_p()
        _check(self.L.zkm_sha_extend_trace(self.h, inputs.ctypes.data_as(C.c_void_p), _data_ptr(timestamps), len(inputs), log_n,
                                           _data_ptr(out), C.byref(err)), err)
        return out

    def sha_extend_sponge_trace(self, w16, meta, log_n, out=None):
        """ShaExtendSpongeStark::generate_trace on the GPU for complete schedules: w16 nblocks x 16 uint32, meta nblocks x 4."""
        w16 = np.ascontiguousarray(w16, dtype=np.uint32).reshape(-1, 16)
        meta = np.ascontiguousarray(meta, dtype=np.uint64).reshape(-1, 4)
        out = out or self.alloc(76 << log_n)
        err = C.c_char_p()
        _check(self.L.zkm_sha_extend_sponge_trace(self.h, w16.ctypes.data_as(C.c_void_p), _data_ptr(meta), len(w16), log_n,
                                                  _data_ptr(out), C.byref(err)), err)
        return out

    def _sha_compress(self, fn, cols, hx, w, meta, log_n, out):
        hx = np.ascontiguousarray(hx, dtype=np.uint32).reshape(-1, 8)
        w = np.ascontiguousarray(w, dtype=np.uint32).reshape(-1, 64)
        meta = np.ascontiguousarray(meta, dtype=np.uint64).reshape(-1, 8)
        out = out or self.alloc(cols << log_n)
        err = C.c_char_p()
        _check(fn(self.h, hx.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), _data_ptr(meta), len(hx), log_n, _data_ptr(out),
                  C.byref(err)), err)
        return out

    def sha_compress_trace(self, hx, w, meta, log_n, out=None):
        """ShaCompressStark::generate_trace on the GPU: 65 rows per compression, 224 x 2^log_n words."""
        return self._sha_compress(self.L.zkm_sha_compress_trace, 224, hx, w, meta, log_n, out)

    def sha_compress_sponge_trace(self, hx, w, meta, log_n, out=None):
        """ShaCompressSpongeStark::generate_trace on the GPU: one row per compression, 127 x 2^log_n words."""
        return self._sha_compress(self.L.zkm_sha_compress_sponge_trace, 127, hx, w, meta, log_n, out)

    def keccak_trace(self, inputs, timestamps, log_n, out=None):
        """KeccakStark::generate_trace on the GPU (keccak/keccak_stark.rs:62-236).  inputs: nperms x 25 uint64, timestamps:
        nperms uint64 (ndarrays or DeviceBuffers).  Returns a DeviceBuffer of 2431 x 2^log_n words."""
        if isinstance(inputs, DeviceBuffer):
            nperms = inputs.words // 25
        else:
            inputs = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1, 25)
            nperms = len(inputs)
        if not isinstance(timestamps, DeviceBuffer):
            timestamps = np.ascontiguousarray(timestamps, dtype=np.uint64)
        out = out or self.alloc(KECCAK_COLS << log_n)
        err = C.c_char_p()
        _check(self.L.zkm_keccak_trace(self.h, _data_ptr(inputs), _data_ptr(timestamps), nperms, log_n, _data_ptr(out), C.byref(err)), err)
        return out

    def logic_trace(self, ops, log_n, out=None):
        """LogicStark::generate_trace on the GPU (logic.rs:150-183).  ops: nops x 3 uint32 (op, input0, input1).
        Returns a DeviceBuffer of 69 x 2^log_n words."""
        ops = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1, 3)
        out = out or self.alloc(LOGIC_COLS << log_n)
        err = C.c_char_p()
        _check(self.L.zkm_logic_trace(self.h, ops.ctypes.data_as(C.c_void_p), len(ops), log_n, _data_ptr(out), C.byref(err)), err)
        return out

    def memory_trace(self, ops, log_n=None, out=None):
        """MemoryStark::generate_trace on the GPU (memory_stark.rs:135-248) from the raw operations.  ops: nops x 6 uint64 (context,
        segment, virt, timestamp, is_read, value), an ndarray or a DeviceBuffer.  log_n=None: the reference's height (a sizing call
        first).  Returns (DeviceBuffer of 13 x 2^log_n words, natural rows = next_pow2(nops + dummy rows))."""
        if isinstance(ops, DeviceBuffer):
            nops = ops.words // 6
        else:
            ops = np.ascontiguousarray(ops, dtype=np.uint64).reshape(-1, 6)
            nops = len(ops)
        natural = C.c_size_t()
        err = C.c_char_p()
        if log_n is None:
            _check(self.L.zkm_memory_trace(self.h, _data_ptr(ops), nops, 0, None, C.byref(natural), C.byref(err)), err)
            log_n = natural.value.bit_length() - 1
        mine = out is None
        out = out or self.alloc(MEMORY_COLS << log_n)
        rc = self.L.zkm_memory_trace(self.h, _data_ptr(ops), nops, log_n, _data_ptr(out), C.byref(natural), C.byref(err))
        if rc != 0 and mine:
            out.free()
        _check(rc, err)
        return out, natural.value

    def arithmetic_trace(self, ops, log_n=None, out=None, nops=None):
        """ArithmeticStark::generate_trace on the GPU (arithmetic_stark.rs:155-185) from the raw operations.  ops: nops x 3 uint32
        (op = row filter IS_ADD 0 .. IS_MTLO 25, input0, input1), an ndarray or a DeviceBuffer holding them packed (ceil(3 nops / 2)
        words; nops=None takes that many from its size).  log_n=None: the reference's height (a sizing call first).  Returns
        (DeviceBuffer of 54 x 2^log_n words, natural rows = max(2^16, next_pow2(rows)))."""
        if isinstance(ops, DeviceBuffer):
            nops = ops.words * 2 // 3 if nops is None else nops
        else:
            ops = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1, 3)
            nops = len(ops)
        src = _data_ptr(ops) if isinstance(ops, DeviceBuffer) else ops.ctypes.data_as(C.c_void_p)
        natural = C.c_size_t()
        err = C.c_char_p()
        if log_n is None:
            _check(self.L.zkm_arithmetic_trace(self.h, src, nops, 0, None, C.byref(natural), C.byref(err)), err)
            log_n = natural.value.bit_length() - 1
        mine = out is None
        out = out or self.alloc(ARITHMETIC_COLS << log_n)
        rc = self.L.zkm_arithmetic_trace(self.h, src, nops, log_n, _data_ptr(out), C.byref(natural), C.byref(err))
        if rc != 0 and mine:
            out.free()
        _check(rc, err)
        return out, natural.value

    # ---- profiling
    def profile(self, on=True):
        self.L.zkm_profile_enable(self.h, int(on))

    def profile_reset(self):
        self.L.zkm_profile_reset(self.h)

    def profile_records(self):
        out = {}
        for i in range(self.L.zkm_profile_count(self.h)):
            name, n, ms = C.c_char_p(), C.c_uint64(), C.c_double()
            self.L.zkm_profile_get(self.h, i, C.byref(name), C.byref(n), C.byref(ms))
            out[name.value.decode()] = (n.value, ms.value)
        return out

    # ---- STARK
    def standard_config(self):
        cfg = StarkConfig()
        self.L.zkm_standard_config(C.byref(cfg))
        return cfg

    def proof_words(self, cfg, log_n, ncols, naux, nctl):
        return self.L.zkm_proof_words(C.byref(cfg), log_n, ncols, naux, nctl)

    def stage_trace(self, values, ncols, log_n, canonical=True):
        """zkm_trace_stage[_columns]: queue the upload of a host matrix (one array, or a list of per-column arrays) on the copy streams and
        return at once; the StagedTrace goes where a prove call of this context takes a trace.  The host arrays must stay alive and
        unchanged until ready() or free()."""
        h, err = C.c_void_p(), C.c_char_p()
        if isinstance(values, (list, tuple)):
            keep = [np.ascontiguousarray(c, dtype=np.uint64) for c in values]
            cols = (C.c_void_p * len(keep))(*[c.ctypes.data for c in keep])
            _check(self.L.zkm_trace_stage_columns(self.h, cols, ncols, log_n, 1 if canonical else 0, C.byref(h), C.byref(err)), err)
        else:
            keep = np.ascontiguousarray(values, dtype=np.uint64)
            assert keep.size == ncols << log_n
            _check(self.L.zkm_trace_stage(self.h, _np_ptr(keep), ncols, log_n, 1 if canonical else 0, C.byref(h), C.byref(err)), err)
        st = StagedTrace(self, h, ncols << log_n)
        st._keep = keep
        return st

    def stage_segment(self, traces, log_ns, canonical=True):
        """zkm_segment_stage[_columns]: all twelve tables of one segment (host arrays, or lists of per-column arrays) in ONE call.  Returns a
        StagedTrace whose .tables() are the twelve device pointers to hand to prove_segments as that segment's traces."""
        assert len(traces) == 12 and len(log_ns) == 12
        h, err = C.c_void_p(), C.c_char_p()
        lg = (C.c_uint * 12)(*[int(x) for x in log_ns])
        if all(isinstance(t, (list, tuple)) for t in traces):
            keep = [[np.ascontiguousarray(c, dtype=np.uint64) for c in t] for t in traces]
            cols = [(C.c_void_p * len(t))(*[c.ctypes.data for c in t]) for t in keep]
            tabs = (C.c_void_p * 12)(*[C.addressof(c) for c in cols])
            keep = (keep, cols)
            _check(self.L.zkm_segment_stage_columns(self.h, tabs, lg, 1 if canonical else 0, C.byref(h), C.byref(err)), err)
        else:
            keep = [np.ascontiguousarray(t, dtype=np.uint64) for t in traces]
            tabs = (C.c_void_p * 12)(*[t.ctypes.data for t in keep])
            _check(self.L.zkm_segment_stage(self.h, tabs, lg, 1 if canonical else 0, C.byref(h), C.byref(err)), err)
        st = StagedTrace(self, h, 0)
        st._keep = keep
        return st

    def segment_tables(self, ops, cfg=None):
        """zkm_segment_tables: Traces::into_tables (witness/traces.rs:230-320) on the device.  ops: a SegmentOps.  Returns (staged,
        log_ns): a StagedTrace whose .tables() are the twelve device matrices (Table::all() order) -- traces[s] of prove_segments -- and
        the reference's heights, as the library computes them."""
        cfg = cfg or self.standard_config()
        st, lg, h, err = ops.struct(), (C.c_uint * 12)(), C.c_void_p(), C.c_char_p()
        _check(self.L.zkm_segment_tables(self.h, C.byref(cfg), C.byref(st), lg, C.byref(h), C.byref(err)), err)
        staged = StagedTrace(self, h, 0)
        return staged, list(lg)

    def segment_heights(self, ops, cfg=None):
        """zkm_segment_tables' sizing mode: the twelve log heights only, nothing allocated."""
        cfg = cfg or self.standard_config()
        st, lg, err = ops.struct(), (C.c_uint * 12)(), C.c_char_p()
        _check(self.L.zkm_segment_tables(self.h, C.byref(cfg), C.byref(st), lg, None, C.byref(err)), err)
        return list(lg)

    def segments_tables(self, ops_list, cfg=None):
        """zkm_segments_tables: the tables of K segments, every generation kernel launched once for all of them and three host waits for
        the call.  ops_list: SegmentOps (host lists, device lists, StagedOps.ops(), mixed).  Returns [(staged, log_ns)] as
        segment_tables gives them, one per segment; each staged is freed on its own."""
        cfg = cfg or self.standard_config()
        K = len(ops_list)
        st = (SegmentOpsStruct * max(K, 1))(*[o.struct() for o in ops_list])
        lg, hs, err = (C.c_uint * (12 * max(K, 1)))(), (C.c_void_p * max(K, 1))(), C.c_char_p()
        _check(self.L.zkm_segments_tables(self.h, C.byref(cfg), K, st, lg, hs, C.byref(err)), err)
        return [(StagedTrace(self, C.c_void_p(hs[s]), 0), list(lg[12 * s:12 * s + 12])) for s in range(K)]

    def segments_heights(self, ops_list, cfg=None):
        """zkm_segments_tables' sizing mode: the twelve log heights of each segment, nothing allocated."""
        cfg = cfg or self.standard_config()
        K = len(ops_list)
        st = (SegmentOpsStruct * max(K, 1))(*[o.struct() for o in ops_list])
        lg, err = (C.c_uint * (12 * max(K, 1)))(), C.c_char_p()
        _check(self.L.zkm_segments_tables(self.h, C.byref(cfg), K, st, lg, None, C.byref(err)), err)
        return [list(lg[12 * s:12 * s + 12]) for s in range(K)]

    def prove_segments_ops(self, ops_list, public_values=None, cfg=None, sizes=None):
        """zkm_prove_segments_ops: K segments built from their raw operations in one set of launches and proven in lock-step.
        public_values: one array per segment.  Returns [(proofs, ctl_challenges, offsets)] as prove_segment_ops gives them.
        sizes: the offsets an earlier call returned for segments of the same heights -- the sizing call (which finds the heights on the
        device) is then skipped."""
        cfg = cfg or self.standard_config()
        m, err = _marshal_ops(ops_list, public_values, cfg), C.c_char_p()
        if sizes is None:
            _check(self.L.zkm_prove_segments_ops(self.h, C.byref(cfg), m.K, m.st, m.pv, m.npv, None, m.offs, None, C.byref(err)), err)
        else:
            m.offs[:] = [x for o in sizes for x in o]
        m.alloc()
        _check(self.L.zkm_prove_segments_ops(self.h, C.byref(cfg), m.K, m.st, m.pv, m.npv, m.po, m.offs, m.co, C.byref(err)), err)
        return m.results()

    def prove_segments_ops_sizes(self, ops_list, public_values=None, cfg=None):
        """The sizing call of zkm_prove_segments_ops alone: the thirteen proof offsets of each segment."""
        cfg = cfg or self.standard_config()
        m, err = _marshal_ops(ops_list, public_values, cfg), C.c_char_p()
        _check(self.L.zkm_prove_segments_ops(self.h, C.byref(cfg), m.K, m.st, m.pv, m.npv, None, m.offs, None, C.byref(err)), err)
        return [list(m.offs[13 * s:13 * s + 13]) for s in range(m.K)]

    # ---- the same calls with each segment's bootstrap kernel built from its image (include/zkm_hip.h "a segment's bootstrap kernel")
    def boot_witness(self, image):
        """zkm_boot_witness: the bootstrap's kernels alone.  Returns numpy (cpu_rows nboot x 259, memory_ops n x 6, poseidon_inputs
        n x 12, poseidon_timestamps n, digests (npages + 1) x 4)."""
        rows, mem, po, _, _ = image.counts()
        bufs = [self.alloc(max(n, 1)) for n in (rows * 259, mem * 6, po * 12, po, (image.npages + 1) * 4)]
        try:
            st, err = image.struct(), C.c_char_p()
            _check(self.L.zkm_boot_witness(self.h, C.byref(st), *[C.c_void_p(b.ptr) for b in bufs], C.byref(err)), err)
            shapes = ((rows, 259), (mem, 6), (po, 12), (po,), (image.npages + 1, 4))
            return tuple(b.download()[:int(np.prod(sh))].reshape(sh) for b, sh in zip(bufs, shapes))
        finally:
            for b in bufs:
                b.free()

    # ---- what the emulator hashes between two segments (include/zkm_hip.h "a memory image's hash pages, root and image id")
    def images_hash(self, images, outs=None):
        """zkm_images_hash: `images` is a list of (dirty, known, pc, registers) -- dirty and known each (indices, words) with words an
        n x 1024 uint32 array or device memory (DeviceBuffer, torch tensor, integer pointer), known may be None, registers 156 bytes.
        outs[m], where given, is device memory for image m's hash pages and is returned in their place.  Returns a list of
        (plan, hash_pages nplan x 1024 uint32, root 32 bytes, image_id 32 bytes)."""
        K = len(images)
        outs = list(outs) if outs is not None else [None] * K
        st, keep, plans, pages = (ImagePagesStruct * max(K, 1))(), [], [], []
        for m, (dirty, known, pc, registers) in enumerate(images):
            d_idx = np.ascontiguousarray(dirty[0] if dirty is not None else [], dtype=np.uint32).reshape(-1)
            k_idx = np.ascontiguousarray(known[0] if known is not None else [], dtype=np.uint32).reshape(-1)
            d_ptr, d_keep = _pages_ptr(dirty[1] if dirty is not None else None, d_idx.size)
            k_ptr, k_keep = _pages_ptr(known[1] if known is not None else None, k_idx.size)
            keep += [d_idx, k_idx, d_keep, k_keep]
            st[m].dirty_index, st[m].ndirty, st[m].dirty_words = d_idx.ctypes.data if d_idx.size else None, d_idx.size, d_ptr
            st[m].known_index, st[m].nknown, st[m].known_words = k_idx.ctypes.data if k_idx.size else None, k_idx.size, k_ptr
            st[m].pc = int(pc)
            registers = bytes(registers)
            assert len(registers) == 156
            st[m].registers[:] = registers
            plans.append(self.L.zkm_image_hash_plan(d_idx.ctypes.data, d_idx.size, None, 0))
            pages.append(np.zeros((plans[-1], 1024), dtype=np.uint32) if outs[m] is None else outs[m])
        out_ptrs = (C.c_void_p * max(K, 1))(*[p.ctypes.data if isinstance(p, np.ndarray) else _data_ptr(p).value for p in pages])
        roots, ids, err = np.zeros(32 * K, dtype=np.uint8), np.zeros(32 * K, dtype=np.uint8), C.c_char_p()
        if K == 1:
            rc = self.L.zkm_image_hash(self.h, C.byref(st[0]), out_ptrs[0], roots.ctypes.data, ids.ctypes.data, C.byref(err))
        else:
            rc = self.L.zkm_images_hash(self.h, K, st, out_ptrs, roots.ctypes.data, ids.ctypes.data, C.byref(err))
        _check(rc, err)
        return [(image_hash_plan(images[m][0][0] if images[m][0] is not None else []), pages[m], roots[32 * m:32 * m + 32].tobytes(),
                 ids[32 * m:32 * m + 32].tobytes()) for m in range(K)]

    def image_hash(self, dirty, known=None, pc=0, registers=bytes(156), out=None):
        """zkm_image_hash: one memory (images_hash with one image).  Returns (plan, hash_pages, root, image_id)."""
        return self.images_hash([(dirty, known, pc, registers)], outs=[out])[0]

    def segment_tables_boot(self, image, ops, cfg=None, sizing=False):
        """zkm_segment_tables_boot: segment_tables with the bootstrap of `image` (a BootImage) in front of ops.  Returns (staged,
        log_ns); sizing=True: the log heights only."""
        cfg = cfg or self.standard_config()
        im, st, lg, h, err = image.struct(), ops.struct(), (C.c_uint * 12)(), C.c_void_p(), C.c_char_p()
        _check(self.L.zkm_segment_tables_boot(self.h, C.byref(cfg), C.byref(im), C.byref(st), lg, None if sizing else C.byref(h), C.byref(err)), err)
        return list(lg) if sizing else (StagedTrace(self, h, 0), list(lg))

    def segments_tables_boot(self, images, ops_list, cfg=None):
        """zkm_segments_tables_boot: K segments in one call.  Returns [(staged, log_ns)], each staged freed on its own."""
        cfg = cfg or self.standard_config()
        K = len(ops_list)
        assert len(images) == K, "one image per segment"
        im = (BootImageStruct * max(K, 1))(*[i.struct() for i in images])
        st = (SegmentOpsStruct * max(K, 1))(*[o.struct() for o in ops_list])
        lg, hs, err = (C.c_uint * (12 * max(K, 1)))(), (C.c_void_p * max(K, 1))(), C.c_char_p()
        _check(self.L.zkm_segments_tables_boot(self.h, C.byref(cfg), K, im, st, lg, hs, C.byref(err)), err)
        return [(StagedTrace(self, C.c_void_p(hs[s]), 0), list(lg[12 * s:12 * s + 12])) for s in range(K)]

    def prove_segment_ops_boot(self, image, ops, public_values=(), cfg=None):
        """zkm_prove_segment_ops_boot: prove_segment_ops with the bootstrap of `image` in front of ops."""
        cfg = cfg or self.standard_config()
        im, st, err = image.struct(), ops.struct(), C.c_char_p()
        pub = np.ascontiguousarray(public_values, dtype=np.uint64)
        offs = (C.c_size_t * 13)()
        _check(self.L.zkm_prove_segment_ops_boot(self.h, C.byref(cfg), C.byref(im), C.byref(st), pub.ctypes.data_as(u64p), pub.size, None, offs,
                                                 None, C.byref(err)), err)
        proofs = np.zeros(offs[12], dtype=np.uint64)
        chal = np.zeros(2 * cfg.num_challenges, dtype=np.uint64)
        _check(self.L.zkm_prove_segment_ops_boot(self.h, C.byref(cfg), C.byref(im), C.byref(st), pub.ctypes.data_as(u64p), pub.size,
                                                 proofs.ctypes.data_as(u64p), offs, chal.ctypes.data_as(u64p), C.byref(err)), err)
        return proofs, chal, list(offs)

    def prove_segments_ops_boot(self, images, ops_list, public_values=None, cfg=None):
        """zkm_prove_segments_ops_boot: K segments, each with its bootstrap, built in one set of launches and proven in lock-step."""
        cfg = cfg or self.standard_config()
        m, err = _marshal_ops(ops_list, public_values, cfg, images), C.c_char_p()
        _check(self.L.zkm_prove_segments_ops_boot(self.h, C.byref(cfg), m.K, m.im, m.st, m.pv, m.npv, None, m.offs, None, C.byref(err)), err)
        m.alloc()
        _check(self.L.zkm_prove_segments_ops_boot(self.h, C.byref(cfg), m.K, m.im, m.st, m.pv, m.npv, m.po, m.offs, m.co, C.byref(err)), err)
        return m.results()

    # ---- the same calls with the CPU rows built from a compact step log (include/zkm_hip.h "a segment's CPU table from a compact step log")
    def cpu_witness(self, steps, log_n, first_clock=0):
        """zkm_cpu_witness: the step kernel alone.  steps: a CpuSteps.  Returns numpy (cpu table 259 * 2^log_n words column-major,
        memory_ops n x 6 uint64, logic_ops n x 3 uint32, arithmetic_ops n x 3 uint32)."""
        nm, nl, na = steps.counts()
        bufs = [self.alloc(max(n, 1)) for n in (259 << log_n, nm * 6, (nl * 3 + 1) // 2, (na * 3 + 1) // 2)]
        try:
            st, err = steps.struct(), C.c_char_p()
            _check(self.L.zkm_cpu_witness(self.h, C.byref(st), first_clock, log_n, *[C.c_void_p(b.ptr) for b in bufs], C.byref(err)), err)
            return (bufs[0].download()[:259 << log_n], bufs[1].download()[:nm * 6].reshape(nm, 6),
                    bufs[2].download().view(np.uint32)[:nl * 3].reshape(nl, 3), bufs[3].download().view(np.uint32)[:na * 3].reshape(na, 3))
        finally:
            for b in bufs:
                b.free()

    def cpu_steps_counts(self, steps):
        """zkm_cpu_steps_counts (module-level cpu_steps_counts: no GPU is involved)."""
        return cpu_steps_counts(steps)

    def cpu_steps_scan(self, steps_list, bases=False):
        """zkm_cpu_steps_scan: the walk over K step logs on the device, alone.  Returns [(memory_ops, logic_ops, arithmetic_ops)] per
        segment; bases=True: ([counts], [the base triples of segment s, an (n, 3) uint32 array with one row per 256 steps]); bases may
        also be the arrays to fill, one per segment (C-contiguous uint32 of at least that size, or None to skip a segment).  A refusal
        raises ZkmError with the host walk's message behind "zkm_cpu_steps_scan: segment <s>: "."""
        K = len(steps_list)
        sl = (CpuStepsStruct * max(K, 1))(*[x.struct() for x in steps_list])
        counts, err = (C.c_size_t * (3 * max(K, 1)))(), C.c_char_p()
        base = [np.zeros(((sl[s].nsteps + 255) // 256, 3), dtype=np.uint32) for s in range(K)] if bases is True else list(bases or [])
        assert not base or (len(base) == K and all(b is None or (b.dtype == np.uint32 and b.flags["C_CONTIGUOUS"] and
                                                                 b.size >= 3 * ((sl[s].nsteps + 255) // 256)) for s, b in enumerate(base)))
        ptrs = (C.c_void_p * max(K, 1))(*[None if b is None else b.ctypes.data for b in base]) if base else None
        _check(self.L.zkm_cpu_steps_scan(self.h, K, sl, counts, ptrs, C.byref(err)), err)
        out = [tuple(int(x) for x in counts[3 * s:3 * s + 3]) for s in range(K)]
        return (out, base) if bases else out

    def cpu_steps_stage(self, steps_list):
        """zkm_cpu_steps_stage: queue the upload and the device walk of K step logs behind the context's current work and return a
        StagedSteps at once (no host wait)."""
        K = len(steps_list)
        sl = (CpuStepsStruct * max(K, 1))(*[x.struct() for x in steps_list])
        h, err = C.c_void_p(), C.c_char_p()
        _check(self.L.zkm_cpu_steps_stage(self.h, K, sl, C.byref(h), C.byref(err)), err)
        return StagedSteps(self, h, steps_list)

    def segments_tables_steps(self, steps_list, ops_list, images=None, cfg=None, sizing=False):
        """zkm_segments_tables_steps: segments_tables[_boot] with each segment's CPU rows built from its CpuSteps; the SegmentOps carry no
        cpu_rows.  images: one BootImage per segment, or None.  Returns [(staged, log_ns)]; sizing=True: the log heights only."""
        cfg = cfg or self.standard_config()
        K = len(ops_list)
        assert len(steps_list) == K and (images is None or len(images) == K), "one step list (and image) per segment"
        im = (BootImageStruct * max(K, 1))(*[i.struct() for i in images]) if images is not None else None
        sl = (CpuStepsStruct * max(K, 1))(*[x.struct() for x in steps_list])
        st = (SegmentOpsStruct * max(K, 1))(*[o.struct() for o in ops_list])
        lg, hs, err = (C.c_uint * (12 * max(K, 1)))(), (C.c_void_p * max(K, 1))(), C.c_char_p()
        _check(self.L.zkm_segments_tables_steps(self.h, C.byref(cfg), K, im, sl, st, lg, None if sizing else hs, C.byref(err)), err)
        if sizing:
            return [list(lg[12 * s:12 * s + 12]) for s in range(K)]
        return [(StagedTrace(self, C.c_void_p(hs[s]), 0), list(lg[12 * s:12 * s + 12])) for s in range(K)]

    def prove_segments_ops_steps(self, steps_list, ops_list, images=None, public_values=None, cfg=None, sizes=None):
        """zkm_prove_segments_ops_steps: prove_segments_ops[_boot] with each segment's CPU rows built from its CpuSteps.  sizes: as
        prove_segments_ops takes them (the sizing call is skipped)."""
        cfg = cfg or self.standard_config()
        m, err = _marshal_ops(ops_list, public_values, cfg, images), C.c_char_p()
        assert len(steps_list) == m.K, "one step list per segment"
        im = m.im if images is not None else None
        sl = (CpuStepsStruct * max(m.K, 1))(*[x.struct() for x in steps_list])
        if sizes is None:
            _check(self.L.zkm_prove_segments_ops_steps(self.h, C.byref(cfg), m.K, im, sl, m.st, m.pv, m.npv, None, m.offs, None, C.byref(err)), err)
        else:
            m.offs[:] = [x for o in sizes for x in o]
        m.alloc()
        _check(self.L.zkm_prove_segments_ops_steps(self.h, C.byref(cfg), m.K, im, sl, m.st, m.pv, m.npv, m.po, m.offs, m.co, C.byref(err)), err)
        return m.results()

    # ---- SHA-256 precompile calls expanded on the device (include/zkm_hip.h "SHA-256 precompile calls from their inputs")
    def sha_calls_witness_into(self, extend, compress, nextend, ncompress, raw_rows, memory_ops, logic_ops, sha_extend_inputs, sha_extend_timestamps):
        """zkm_sha_calls_witness as it is: extend = (w16, meta) and compress = (hx, w, meta), each list a numpy array of the right dtype
        or device memory (or None with a count of 0); the five outputs are device addresses (integers) or None."""
        ptr = lambda x: None if x is None else x.ctypes.data if isinstance(x, np.ndarray) else _data_ptr(x).value
        lists = [ptr(x) for x in (tuple(extend or (None, None)) + tuple(compress or (None, None, None)))]
        err = C.c_char_p()
        _check(self.L.zkm_sha_calls_witness(self.h, lists[0], lists[1], nextend, lists[2], lists[3], lists[4], ncompress, raw_rows, memory_ops,
                                            logic_ops, sha_extend_inputs, sha_extend_timestamps, C.byref(err)), err)

    @staticmethod
    def _sha_lists(extend, compress):
        """((w16, meta), (hx, w, meta), nextend, ncompress) as contiguous numpy arrays."""
        e = (np.ascontiguousarray(extend[0], dtype=np.uint32).reshape(-1, 16), _sha_meta(extend[1], 4)) if extend is not None else None
        c = (np.ascontiguousarray(compress[0], dtype=np.uint32).reshape(-1, 8), np.ascontiguousarray(compress[1], dtype=np.uint32).reshape(-1, 64),
             _sha_meta(compress[2], 8)) if compress is not None else None
        ne, nc = (len(e[1]) if e else 0), (len(c[2]) if c else 0)
        assert (not e or len(e[0]) == ne) and (not c or len(c[0]) == len(c[1]) == nc), "one entry of every list per call"
        return (e if ne else None), (c if nc else None), ne, nc

    def sha_calls_witness(self, extend=None, compress=None):
        """zkm_sha_calls_witness into buffers of its own.  Returns numpy (raw_rows n x 259 uint64, memory_ops n x 6 uint64, logic_ops n x 3
        uint32, sha_extend_inputs n x 16 uint8, sha_extend_timestamps n uint64)."""
        e, c, ne, nc = self._sha_lists(extend, compress)
        rows, mem, logic, ext = sha_calls_counts(ne, nc)
        bufs = [self.alloc(max(n, 1)) for n in (rows * 259, mem * 6, (logic * 3 + 1) // 2, ext * 2, ext)]
        try:
            self.sha_calls_witness_into(e, c, ne, nc, *[b.ptr for b in bufs])
            return (bufs[0].download()[:rows * 259].reshape(rows, 259), bufs[1].download()[:mem * 6].reshape(mem, 6),
                    bufs[2].download().view(np.uint32)[:logic * 3].reshape(logic, 3), bufs[3].download().view(np.uint8)[:ext * 16].reshape(ext, 16),
                    bufs[4].download()[:ext])
        finally:
            for b in bufs:
                b.free()

    def sha_calls_expand(self, steps, first_clock=0, extend=None, compress=None, memory_ops=None, logic_ops=None, **groups):
        """calls_expand for a segment whose only calls are SHA calls; groups: the other groups of SegmentOps, passed on (keccak = the
        segment's own permutations)."""
        assert "sha_extend" not in groups
        return self.calls_expand(steps, first_clock, extend=extend, compress=compress, memory_ops=memory_ops, logic_ops=logic_ops,
                                 keccak_perms=groups.pop("keccak", None), **groups)

    # ---- SYSKECCAK precompile calls expanded on the device (include/zkm_hip.h "SYSKECCAK precompile calls from their input bytes")
    @staticmethod
    def _keccak_lists(keccak):
        """(inputs u8, off n + 1, meta n x 4, digest_addrs n) as contiguous numpy arrays and the number of calls; None, 0 without calls."""
        if keccak is None:
            return None, 0
        inputs, off, meta, digest_addrs = keccak
        k = (np.ascontiguousarray(inputs, dtype=np.uint8).reshape(-1), np.ascontiguousarray(off, dtype=np.uint64).reshape(-1), _sha_meta(meta, 4),
             np.ascontiguousarray(digest_addrs, dtype=np.uint64).reshape(-1))
        n = len(k[2])
        assert k[1].size == n + 1 and k[3].size == n, "one meta and one digest address per call, and one offset more"
        return (k if n else None), n

    def keccak_calls_witness_into(self, keccak, ncalls, raw_rows, memory_ops, logic_ops, keccak_inputs, keccak_timestamps):
        """zkm_keccak_calls_witness as it is: keccak = (inputs, input_off, meta, digest_addrs), input_off a numpy array, the others numpy
        arrays of the right dtype or device memory (or None with a count of 0); the five outputs are device addresses (integers) or None."""
        ptr = lambda x: None if x is None else x.ctypes.data if isinstance(x, np.ndarray) else _data_ptr(x).value
        lists = [ptr(x) for x in tuple(keccak or (None,) * 4)]
        err = C.c_char_p()
        _check(self.L.zkm_keccak_calls_witness(self.h, *lists, ncalls, raw_rows, memory_ops, logic_ops, keccak_inputs, keccak_timestamps,
                                               C.byref(err)), err)

    def keccak_calls_witness(self, inputs, input_off, meta, digest_addrs):
        """zkm_keccak_calls_witness into buffers of its own.  Returns numpy (raw_rows n x 259 uint64, memory_ops n x 6 uint64, logic_ops
        n x 3 uint32, keccak_inputs n x 25 uint64, keccak_timestamps n uint64)."""
        k, n = self._keccak_lists((inputs, input_off, meta, digest_addrs))
        rows, mem, logic, perms = keccak_calls_counts(k[1], k[2]) if n else (0, 0, 0, 0)
        bufs = [self.alloc(max(w, 1)) for w in (rows * 259, mem * 6, (logic * 3 + 1) // 2, perms * 25, perms)]
        try:
            self.keccak_calls_witness_into(k, n, *[b.ptr for b in bufs])
            return (bufs[0].download()[:rows * 259].reshape(rows, 259), bufs[1].download()[:mem * 6].reshape(mem, 6),
                    bufs[2].download().view(np.uint32)[:logic * 3].reshape(logic, 3), bufs[3].download()[:perms * 25].reshape(perms, 25),
                    bufs[4].download()[:perms])
        finally:
            for b in bufs:
                b.free()

    # ---- the I/O syscalls' rows expanded on the device (include/zkm_hip.h "the I/O syscalls' rows from their bytes")
    def io_calls_witness_into(self, io, ncalls, raw_rows):
        """zkm_io_calls_witness as it is: io = (kinds, data, data_off, meta), kinds and data_off numpy arrays, data and meta numpy arrays
        of the right dtype or device memory (or None with a count of 0); raw_rows is a device address (an integer) or None."""
        ptr = lambda x: None if x is None else x.ctypes.data if isinstance(x, np.ndarray) else _data_ptr(x).value
        lists = [ptr(x) for x in tuple(io or (None,) * 4)]
        err = C.c_char_p()
        _check(self.L.zkm_io_calls_witness(self.h, *lists, ncalls, raw_rows, C.byref(err)), err)

    def io_calls_witness(self, kinds, data, data_off, meta):
        """zkm_io_calls_witness into a buffer of its own.  Returns numpy raw_rows n x 259 uint64."""
        k, n = _io_lists((kinds, data, data_off, meta))
        rows = io_calls_counts(k[0], k[2])[0] if n else 0
        buf = self.alloc(max(rows * 259, 1))
        try:
            self.io_calls_witness_into(k, n, buf.ptr)
            return buf.download()[:rows * 259].reshape(rows, 259)
        finally:
            buf.free()

    # ---- the instructions the step kinds refuse, as rows (include/zkm_hip.h "the instructions the step kinds refuse, as rows")
    def insn_rows_witness_into(self, insns, ninsns, raw_rows, arithmetic_ops):
        """zkm_insn_rows_witness as it is: insns = (records, clocks), numpy arrays of CPU_STEP_DT and uint64 (or None with a count of 0);
        raw_rows and arithmetic_ops are device addresses (integers) or None."""
        ptr = lambda x: None if x is None else x.ctypes.data if isinstance(x, np.ndarray) else _data_ptr(x).value
        lists = [ptr(x) for x in tuple(insns or (None, None))]
        err = C.c_char_p()
        _check(self.L.zkm_insn_rows_witness(self.h, *lists, ninsns, raw_rows, arithmetic_ops, C.byref(err)), err)

    def insn_rows_witness(self, records, clocks):
        """zkm_insn_rows_witness into buffers of its own.  Returns numpy (raw_rows n x 259 uint64, arithmetic_ops n x 3 uint32)."""
        k, n = _insn_lists((records, clocks))
        arith = insn_rows_counts(k[0])[1] if n else 0
        bufs = [self.alloc(max(w, 1)) for w in (n * 259, (arith * 3 + 1) // 2)]
        try:
            self.insn_rows_witness_into(k, n, bufs[0].ptr, bufs[1].ptr if arith else None)
            return bufs[0].download()[:n * 259].reshape(n, 259), bufs[1].download().view(np.uint32)[:arith * 3].reshape(arith, 3)
        finally:
            for b in bufs:
                b.free()

    def calls_expand(self, steps, first_clock=0, extend=None, compress=None, keccak=None, memory_ops=None, logic_ops=None, keccak_perms=None,
                     io=None, insns=None, arithmetic_ops=None, **groups):
        """A segment with precompile and I/O calls made ready for segments_tables_steps / prove_segments_ops_steps.  steps: a CpuSteps with
        the segment's own RAW rows (host memory) whose list holds a placeholder at the position of every row of a call (sha_calls_steps,
        keccak_calls_steps and io_calls_steps say which: clock - first_clock); extend = (w16, meta), compress = (hx, w, meta), keccak =
        (inputs, input_off, meta, digest_addrs), io = (kinds, data, data_off, meta): the calls; insns = (records, clocks): the
        instructions no step kind takes (insn_rows_steps; their placeholders sit at clocks - first_clock); memory_ops / logic_ops /
        arithmetic_ops / keccak_perms = (inputs, timestamps): the segment's own operations; groups: the other groups of SegmentOps, passed
        on.  Returns (CpuSteps, SegmentOps): the steps with the calls' RAW records in place and raw_rows a DeviceBuffer of own rows, then
        the SHA calls', then the Keccak calls', then the I/O calls', then the instructions'; the operations with memory_ops, logic_ops,
        sha_extend and keccak (and, with insns, arithmetic_ops) in device memory (own items in front, the generated ones behind in the
        same order) and the sponge groups set from the calls.  Free with ops.free() and steps.raw_rows.free()."""
        e, c, ne, nc = self._sha_lists(extend, compress)
        k, nk = self._keccak_lists(keccak)
        i, ni = _io_lists(io)
        q, nq = _insn_lists(insns)
        rows, mem, logic, ext = sha_calls_counts(ne, nc)
        krows, kmem, klogic, kperms = keccak_calls_counts(k[1], k[2]) if nk else (0, 0, 0, 0)
        irows = io_calls_counts(i[0], i[2])[0] if ni else 0
        qarith = insn_rows_counts(q[0])[1] if nq else 0
        assert not isinstance(steps.raw_rows, DeviceBuffer) and not {"sha_extend", "keccak_sponge"} & set(groups)
        own_raw = steps.raw_rows.reshape(-1)
        own_mem = np.ascontiguousarray(memory_ops if memory_ops is not None else [], dtype=np.uint64).reshape(-1)
        own_logic = np.ascontiguousarray(logic_ops if logic_ops is not None else [], dtype=np.uint32).reshape(-1)
        own_arith = np.ascontiguousarray(arithmetic_ops if arithmetic_ops is not None else [], dtype=np.uint32).reshape(-1)
        own_perms = [np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for a in (keccak_perms if keccak_perms is not None else ([], []))]
        assert own_perms[0].size == 25 * own_perms[1].size, "25 words and one timestamp per permutation"
        records, clocks = sha_calls_steps(e[1] if e else None, c[2] if c else None, raw_base=steps.nraw)
        if nk:
            krecords, kclocks = keccak_calls_steps(k[1], k[2], raw_base=steps.nraw + rows)
            records, clocks = (np.concatenate([records, krecords]), np.concatenate([clocks, kclocks])) if rows else (krecords, kclocks)
        if ni:
            assert not isinstance(i[3], DeviceBuffer), "the records' clocks are read on the host: meta in host memory"
            irecords, iclocks = io_calls_steps(i[0], i[2], i[3], raw_base=steps.nraw + rows + krows)
            records, clocks = (np.concatenate([records, irecords]), np.concatenate([clocks, iclocks])) if rows + krows else (irecords, iclocks)
        if nq:
            qrecords = insn_rows_steps(q[0], raw_base=steps.nraw + rows + krows + irows)
            records, clocks = (np.concatenate([records, qrecords]), np.concatenate([clocks, q[1]])) if rows + krows + irows else (qrecords, q[1])
        at = clocks.astype(np.int64) - first_clock
        taken = np.zeros(steps.steps.size, dtype=bool)
        if at.size and at.min() >= 0 and at.max() < taken.size:
            taken[at] = True
        assert np.count_nonzero(taken) == at.size, "a call's rows lie outside the step list, or two rows share a clock"
        # (the records as rows of twelve words: numpy copies and scatters a plain matrix several times faster than a structured array)
        patched = steps.steps.view(np.uint32).reshape(-1, 12).copy()
        words = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 12)
        if at.size and at[-1] - at[0] + 1 == at.size and (np.diff(at) == 1).all():
            patched[at[0]:at[0] + at.size] = words            # one run of clocks (one long call): a plain copy
        else:
            patched[at] = words
        patched = patched.reshape(-1).view(CPU_STEP_DT)
        # one device block a list: own items in front, the generated ones behind
        sizes = (own_raw.size + (rows + krows + irows + nq) * 259, own_mem.size + (mem + kmem) * 6, (own_logic.size + (logic + klogic) * 3 + 1) // 2, ext * 2, ext,
                 own_perms[0].size + kperms * 25, own_perms[1].size + kperms, (own_arith.size + qarith * 3 + 1) // 2 if nq else 0)
        bufs = [self.alloc(n) if n else None for n in sizes]
        try:
            for buf, own in zip(bufs, (own_raw, own_mem, own_logic, None, None, own_perms[0], own_perms[1], own_arith if nq else None)):
                if own is not None and own.size:
                    buf.upload(_as_words(own))
            if rows:
                self.sha_calls_witness_into(e, c, ne, nc, bufs[0].ptr + 8 * own_raw.size, bufs[1].ptr + 8 * own_mem.size, bufs[2].ptr + 4 * own_logic.size,
                                            bufs[3].ptr if ext else None, bufs[4].ptr if ext else None)
            if nk:
                self.keccak_calls_witness_into(k, nk, bufs[0].ptr + 8 * (own_raw.size + rows * 259), bufs[1].ptr + 8 * (own_mem.size + mem * 6),
                                               bufs[2].ptr + 4 * (own_logic.size + logic * 3), bufs[5].ptr + 8 * own_perms[0].size,
                                               bufs[6].ptr + 8 * own_perms[1].size)
            if ni:
                self.io_calls_witness_into(i, ni, bufs[0].ptr + 8 * (own_raw.size + (rows + krows) * 259))
            if nq:
                self.insn_rows_witness_into(q, nq, bufs[0].ptr + 8 * (own_raw.size + (rows + krows + irows) * 259),
                                            bufs[7].ptr + 4 * own_arith.size if qarith else None)
        except Exception:
            for b in bufs:
                if b is not None:
                    b.free()
            raise
        ops = SegmentOps(None, bufs[1], logic_ops=bufs[2], sha_extend=(bufs[3], bufs[4]) if ext else None, sha_extend_sponge=e, sha_compress=c,
                         sha_compress_sponge=c, keccak=(bufs[5], bufs[6]) if bufs[5] is not None else None, keccak_sponge=k[:3] if nk else None,
                         arithmetic_ops=bufs[7] if nq else arithmetic_ops, **groups)
        ops.counts["nlogic"] = own_logic.size // 3 + logic + klogic     # (a DeviceBuffer is counted in whole words)
        if nq:
            ops.counts["narithmetic"] = own_arith.size // 3 + qarith
        return CpuSteps(patched, bufs[0] if bufs[0] is not None else None, nraw=steps.nraw + rows + krows + irows + nq), ops

    # ---- K segments' calls in one set of launches (include/zkm_hip.h "K segments' calls expanded in one set of launches")
    @staticmethod
    def _calls_array(calls_list):
        structs = [q.struct() for q in calls_list]
        return (SegmentCallsStruct * max(len(structs), 1))(*structs)

    def segments_calls_expand(self, calls_list):
        """zkm_segments_calls_expand: the calls of all the SegmentCalls expanded -- per 32 segments one scratch block, at most one launch per
        kind and one host wait.  Returns an ExpandedCalls; every word is what calls_expand gives for that segment alone."""
        arr, h, err = self._calls_array(calls_list), C.c_void_p(), C.c_char_p()
        _check(self.L.zkm_segments_calls_expand(self.h, len(calls_list), C.addressof(arr), C.byref(h), C.byref(err)), err)
        return ExpandedCalls(self, h, calls_list)

    def segments_calls_stage(self, calls_list, images=None):
        """zkm_segments_calls_stage: queue the uploads, the expansions, the placement of the records and the device walk of K segments'
        calls (and the upload of their BootImages) behind the context's current work and return a StagedCalls at once (no host wait)."""
        K = len(calls_list)
        assert images is None or len(images) == K, "one image per segment"
        im = (BootImageStruct * max(K, 1))(*[i.struct() for i in images]) if images is not None else None
        arr, h, err = self._calls_array(calls_list), C.c_void_p(), C.c_char_p()
        _check(self.L.zkm_segments_calls_stage(self.h, K, C.addressof(arr), im, C.byref(h), C.byref(err)), err)
        return StagedCalls(self, h, calls_list, images)

    def segments_tables_calls(self, calls_list, images=None, cfg=None, sizing=False):
        """zkm_segments_tables_calls: segments_calls_expand, segments_tables_steps on its outputs, the free.  Returns as
        segments_tables_steps."""
        cfg = cfg or self.standard_config()
        K = len(calls_list)
        assert images is None or len(images) == K, "one image per segment"
        im = (BootImageStruct * max(K, 1))(*[i.struct() for i in images]) if images is not None else None
        arr = self._calls_array(calls_list)
        lg, hs, err = (C.c_uint * (12 * max(K, 1)))(), (C.c_void_p * max(K, 1))(), C.c_char_p()
        _check(self.L.zkm_segments_tables_calls(self.h, C.byref(cfg), K, im, C.addressof(arr), lg, None if sizing else hs, C.byref(err)), err)
        if sizing:
            return [list(lg[12 * s:12 * s + 12]) for s in range(K)]
        return [(StagedTrace(self, C.c_void_p(hs[s]), 0), list(lg[12 * s:12 * s + 12])) for s in range(K)]

    def prove_segments_ops_calls(self, calls_list, images=None, public_values=None, cfg=None, sizes=None):
        """zkm_prove_segments_ops_calls: segments_calls_expand, prove_segments_ops_steps on its outputs, the free.  sizes: as
        prove_segments_ops takes them (the sizing call, which expands the calls too, is skipped)."""
        cfg = cfg or self.standard_config()
        m, err = _marshal_ops([q.own for q in calls_list], public_values, cfg, images), C.c_char_p()
        im = m.im if images is not None else None
        arr = self._calls_array(calls_list)
        if sizes is None:
            _check(self.L.zkm_prove_segments_ops_calls(self.h, C.byref(cfg), m.K, im, C.addressof(arr), m.pv, m.npv, None, m.offs, None, C.byref(err)), err)
        else:
            m.offs[:] = [x for o in sizes for x in o]
        m.alloc()
        _check(self.L.zkm_prove_segments_ops_calls(self.h, C.byref(cfg), m.K, im, C.addressof(arr), m.pv, m.npv, m.po, m.offs, m.co, C.byref(err)), err)
        return m.results()

    def stage_segment_ops(self, ops):
        """zkm_segment_ops_stage: queue the upload of a segment's lists behind the context's current work and return at once.  The
        lists (ideally Context.pinned_array memory) must stay as they are until .ready() says so."""
        st, h, err = ops.struct(), C.c_void_p(), C.c_char_p()
        _check(self.L.zkm_segment_ops_stage(self.h, C.byref(st), C.byref(h), C.byref(err)), err)
        staged = StagedOps(self, h)
        staged._keep = ops
        return staged

    def prove_segment_ops(self, ops, public_values=(), cfg=None):
        """zkm_prove_segment_ops: the segment's tables built on the device from its raw operations and proven (into_tables +
        prove_with_traces).  Returns (proofs, ctl_challenges, offsets) as prove_segment does."""
        cfg = cfg or self.standard_config()
        st, err = ops.struct(), C.c_char_p()
        pub = np.ascontiguousarray(public_values, dtype=np.uint64)
        offs = (C.c_size_t * 13)()
        _check(self.L.zkm_prove_segment_ops(self.h, C.byref(cfg), C.byref(st), pub.ctypes.data_as(u64p), pub.size, None, offs, None, C.byref(err)),
               err)
        proofs = np.zeros(offs[12], dtype=np.uint64)
        chal = np.zeros(2 * cfg.num_challenges, dtype=np.uint64)
        _check(self.L.zkm_prove_segment_ops(self.h, C.byref(cfg), C.byref(st), pub.ctypes.data_as(u64p), pub.size, proofs.ctypes.data_as(u64p),
                                            offs, chal.ctypes.data_as(u64p), C.byref(err)), err)
        return proofs, chal, list(offs)

    def prove_single_table(self, trace, log_n, aux, num_helpers, challenger=None, cfg=None, ncols=POSEIDON_COLS,
                           trace_batch=None, naux=None, table_id=TABLE_POSEIDON):
        """prove_single_table (prover.rs:441-641).  Returns the flat proof (include/zkm_hip.h layout)."""
        cfg = cfg or self.standard_config()
        ch = challenger if challenger is not None else Challenger()
        if naux is None:
            naux = (aux.size if isinstance(aux, np.ndarray) else aux.words) >> log_n
        nh = (C.c_uint32 * len(num_helpers))(*num_helpers)
        proof = np.zeros(self.proof_words(cfg, log_n, ncols, naux, len(num_helpers)), dtype=np.uint64)
        err = C.c_char_p()
        _check(self.L.zkm_prove_single_table(self.h, table_id, C.byref(cfg), _data_ptr(trace) if trace is not None else None,
                                             ncols, log_n, trace_batch.h if trace_batch is not None else None, _data_ptr(aux),
                                             naux, nh, len(num_helpers), C.byref(ch), proof.ctypes.data_as(u64p),
                                             C.byref(err)), err)
        return proof

    def prove_single_tables(self, traces, log_n, auxs, num_helpers, cfg=None, ncols=POSEIDON_COLS, table_id=TABLE_POSEIDON, challengers=None):
        """zkm_prove_single_tables: K proofs of the same table in lock-step.  traces[k] / auxs[k] as prove_single_table takes them
        (auxs may be ONE array used for every proof).  Returns the list of K proof blobs."""
        cfg = cfg or self.standard_config()
        K = len(traces)
        if not isinstance(auxs, (list, tuple)):
            auxs = [auxs] * K
        chs = challengers if challengers is not None else [Challenger() for _ in range(K)]
        naux = (auxs[0].size if isinstance(auxs[0], np.ndarray) else auxs[0].words) >> log_n
        nh = (C.c_uint32 * len(num_helpers))(*num_helpers)
        words = self.proof_words(cfg, log_n, ncols, naux, len(num_helpers))
        proofs = [np.zeros(words, dtype=np.uint64) for _ in range(K)]
        tp = (C.c_void_p * K)(*[_data_ptr(t).value for t in traces])
        ap = (C.c_void_p * K)(*[_data_ptr(a).value for a in auxs])
        cp_ = (C.c_void_p * K)(*[C.addressof(ch) for ch in chs])
        pp = (C.c_void_p * K)(*[p.ctypes.data for p in proofs])
        err = C.c_char_p()
        _check(self.L.zkm_prove_single_tables(self.h, table_id, C.byref(cfg), K, tp, ncols, log_n, ap, naux, nh, len(num_helpers), cp_, pp,
                                              C.byref(err)), err)
        return proofs

    # ---- cross-table lookups (descriptor builders: zkm_amd/ctl.py)
    def ctl_data(self, ctl_table, zs, colset_ids, trace, ncols, log_n, out=None):
        """cross_table_lookup_data for one table (cross_table_lookup.rs:634-872): helper columns ++ Z columns."""
        naux = int(zs["num_helpers"].sum()) + len(zs)
        host_out = out is None
        if host_out:
            out = np.zeros(naux << log_n, dtype=np.uint64)
        st = ctl_table.pack()
        err = C.c_char_p()
        _check(self.L.zkm_ctl_data(self.h, C.addressof(st), zs.ctypes.data, colset_ids.ctypes.data, len(zs), _data_ptr(trace), ncols,
                                   log_n, _data_ptr(out), C.byref(err)), err)
        return out

    def lookup_helper_columns(self, ctl_table, colset_ids, table_col, freq_col, challenge, trace, ncols, log_n):
        """lookup_helper_columns (lookup.rs:46-124) for one Lookup and one challenge: helper columns then Z."""
        ids = np.ascontiguousarray(colset_ids, dtype=np.uint32)
        out = np.zeros(((len(ids) + 1) // 2 + 1) << log_n, dtype=np.uint64)
        st = ctl_table.pack()
        err = C.c_char_p()
        _check(self.L.zkm_lookup_helper_columns(self.h, C.addressof(st), ids.ctypes.data, len(ids), table_col, freq_col, challenge,
                                                _data_ptr(trace), ncols, log_n, _np_ptr(out), C.byref(err)), err)
        return out

    def prove_single_table_ctl(self, trace, log_n, aux, ctl_table, zs, colset_ids, challenger=None, cfg=None, ncols=POSEIDON_COLS,
                               trace_batch=None, table_id=TABLE_POSEIDON, lookup_challenges=None):
        """lookup_challenges: the CTL betas, required for tables with their own lookups (Memory)."""
        cfg = cfg or self.standard_config()
        ch = challenger if challenger is not None else Challenger()
        naux = (aux.size if isinstance(aux, np.ndarray) else aux.words) >> log_n
        nl = self.L.zkm_num_lookup_columns(table_id, C.byref(cfg))
        proof = np.zeros(self.proof_words(cfg, log_n, ncols, naux + nl, len(zs)), dtype=np.uint64)
        st = ctl_table.pack()
        err = C.c_char_p()
        lk = None if lookup_challenges is None else np.ascontiguousarray(lookup_challenges, dtype=np.uint64)
        _check(self.L.zkm_prove_single_table_ctl(self.h, table_id, C.byref(cfg), _data_ptr(trace) if trace is not None else None, ncols,
                                                 log_n, trace_batch.h if trace_batch is not None else None, _data_ptr(aux), naux,
                                                 C.addressof(st), zs.ctypes.data, colset_ids.ctypes.data, len(zs),
                                                 None if lk is None else lk.ctypes.data_as(u64p), C.byref(ch),
                                                 proof.ctypes.data_as(u64p), C.byref(err)), err)
        return proof

    def check_constraints(self, trace, log_n, aux, ctl_table, zs, colset_ids, alphas, cfg=None, ncols=POSEIDON_COLS, table_id=TABLE_POSEIDON,
                          lookup_challenges=None):
        """check_constraints (prover.rs:793-910): the table's whole vanishing polynomial on every row of the trace domain.  aux = all
        auxiliary columns (lookup helper columns ++ CTL helper columns ++ Zs).  Returns None when every constraint holds, else the
        first failing row."""
        cfg = cfg or self.standard_config()
        naux = (aux.size if isinstance(aux, np.ndarray) else aux.words) >> log_n
        al = np.ascontiguousarray(alphas, dtype=np.uint64)
        lk = None if lookup_challenges is None else np.ascontiguousarray(lookup_challenges, dtype=np.uint64)
        first = C.c_uint64(0)
        err = C.c_char_p()
        if ctl_table is not None:
            st = ctl_table.pack()
            tp, zp, ip, nz = C.addressof(st), zs.ctypes.data, colset_ids.ctypes.data, len(zs)
        else:     # fake CTL shape: zs = num_helpers list
            from . import ctl as zc
            z = np.zeros(len(zs), dtype=zc.CTLZ_DT)
            z["num_helpers"] = zs
            tp, zp, ip, nz = None, z.ctypes.data, None, len(zs)
        rc = self.L.zkm_check_constraints(self.h, table_id, C.byref(cfg), _data_ptr(trace), ncols, log_n, _data_ptr(aux), naux, tp, zp, ip, nz,
                                          None if lk is None else lk.ctypes.data_as(u64p), al.ctypes.data_as(u64p), al.size, C.byref(first),
                                          C.byref(err))
        if rc == 0:
            return None
        msg = err.value.decode() if err.value else ""
        if "Constraint failed" not in msg:
            _check(rc, err)
        return int(first.value)

    @staticmethod
    def _ctl_report(rc, rep, err):
        """The report of a check_ctls call; a call that could not be made (kind 3) raises."""
        rep.message = err.value.decode() if err.value else None
        if rc != 0 and rep.kind in (0, 3):
            raise ZkmError(rep.message or "check_ctls: error %d" % rc)
        return rep

    def check_ctls(self, tables, ctls):
        """zkm_check_ctls: testutils::check_ctls (cross_table_lookup.rs:1486-1581) on the device.  tables / ctls as prove_with_traces
        takes them (arrays, DeviceBuffers, device pointers, or a list of per-column arrays).  Returns the CtlReport: .kind 0 when every
        lookup holds, else the finding with .message in the reference's wording."""
        from . import ctl as zc
        packed = [(tid, [_data_ptr(col).value for col in tr] if isinstance(tr, (list, tuple)) else _data_ptr(tr).value, ncols, log_n, ct)
                  for (tid, tr, ncols, log_n, ct) in tables]
        tarr, keep = zc.pack_tables(packed)
        carr, sides = zc.pack_ctls(ctls)
        rep, err = CtlReport(), C.c_char_p()
        rc = self.L.zkm_check_ctls(self.h, tarr, len(tables), carr.ctypes.data, sides.ctypes.data, len(carr), C.byref(rep), C.byref(err))
        return self._ctl_report(rc, rep, err)

    def segment_check_ctls(self, traces, log_ns):
        """zkm_segment_check_ctls: check_ctls for the AllStark inside the library.  traces: twelve arrays / DeviceBuffers / device
        pointers in Table::all() order, or a staged segment (segment_tables' StagedTrace); log_ns their heights."""
        if isinstance(traces, StagedTrace):
            traces = traces.tables()
        assert len(traces) == 12 and len(log_ns) == 12
        keep = [t if isinstance(t, (DeviceBuffer, StagedTrace, int)) else np.ascontiguousarray(t, dtype=np.uint64) for t in traces]
        ptrs = (C.c_void_p * 12)(*[_data_ptr(t).value for t in keep])
        lg = (C.c_uint * 12)(*[int(x) for x in log_ns])
        rep, err = CtlReport(), C.c_char_p()
        rc = self.L.zkm_segment_check_ctls(self.h, ptrs, lg, C.byref(rep), C.byref(err))
        return self._ctl_report(rc, rep, err)

    @staticmethod
    def _witness_findings(rc, words, err):
        """The findings of a witness check as tuples (row or None, constraint index, value, failing rows, constraints per row); a call
        that could not be made raises.  The message (None when every constraint holds) belongs to the first failing table."""
        msg = err.value.decode() if err.value else None
        if rc != 0 and "Constraint failed" not in (msg or ""):
            raise ZkmError(msg or "witness_check: error %d" % rc)
        w = [int(x) for x in words]
        none = (1 << 64) - 1
        return [(None if w[i] == none else w[i],) + tuple(w[i + 1:i + WITNESS_FINDING_WORDS]) for i in range(0, len(w), WITNESS_FINDING_WORDS)], msg

    def witness_check(self, table_id, trace, log_n):
        """zkm_witness_check: the table's own constraints on every row of the trace (an array, a DeviceBuffer or a device pointer), from the
        trace alone.  Returns (row, constraint index, canonical value, failing rows, constraints per row) of the first failure -- the
        lowest row, within it the lowest index -- with row None when every constraint holds; .witness_message holds the call's message."""
        words, err = (C.c_uint64 * WITNESS_FINDING_WORDS)(), C.c_char_p()
        keep = trace if isinstance(trace, (DeviceBuffer, StagedTrace, int)) else np.ascontiguousarray(trace, dtype=np.uint64)
        rc = self.L.zkm_witness_check(self.h, table_id, _data_ptr(keep), self.L.zkm_table_width(table_id), log_n, words, C.byref(err))
        findings, self.witness_message = self._witness_findings(rc, words, err)
        return findings[0]

    def segment_witness_check(self, traces, log_ns):
        """zkm_segment_witness_check: witness_check on the twelve tables of a segment (Table::all() order; arrays, DeviceBuffers, device
        pointers, or a staged segment) in one set of launches and one host wait.  Returns the twelve findings; .witness_message names
        the first failing table (None when all hold)."""
        if isinstance(traces, StagedTrace):
            traces = traces.tables()
        assert len(traces) == 12 and len(log_ns) == 12
        keep = [t if isinstance(t, (DeviceBuffer, StagedTrace, int)) else np.ascontiguousarray(t, dtype=np.uint64) for t in traces]
        ptrs = (C.c_void_p * 12)(*[_data_ptr(t).value for t in keep])
        lg = (C.c_uint * 12)(*[int(x) for x in log_ns])
        words, err = (C.c_uint64 * (12 * WITNESS_FINDING_WORDS))(), C.c_char_p()
        rc = self.L.zkm_segment_witness_check(self.h, ptrs, lg, words, C.byref(err))
        findings, self.witness_message = self._witness_findings(rc, words, err)
        return findings

    @staticmethod
    def _lookup_findings(rc, words, err):
        """The findings of a lookup check as tuples (lookup or None, value, looking count, frequency, table rows, column and row of the first
        looking cell, first table row, failing values), a location that does not exist as None; a call that could not be made raises.  The
        message (None when every lookup holds) belongs to the first failing table."""
        msg = err.value.decode() if err.value else None
        if rc != 0 and not (msg or "").startswith("Lookup failed in "):
            raise ZkmError(msg or "lookup_check: error %d" % rc)
        w = [int(x) for x in words]
        none = (1 << 64) - 1
        out = []
        for i in range(0, len(w), LOOKUP_FINDING_WORDS):
            f = w[i:i + LOOKUP_FINDING_WORDS]
            out.append(tuple(None if k in (0, 5, 6, 7) and x == none else x for k, x in enumerate(f)))
        return out, msg

    def lookup_check(self, table_id, trace, log_n):
        """zkm_lookup_check: the table's own range-check lookups (Memory, Arithmetic) from the trace alone (an array, a DeviceBuffer, a
        device pointer or a StagedTrace).  Returns the nine words of the finding -- the smallest unbalanced value of the lowest failing
        lookup -- with the lookup None when every lookup holds (and for a table without lookups); .lookup_message holds the call's message."""
        words, err = (C.c_uint64 * LOOKUP_FINDING_WORDS)(), C.c_char_p()
        keep = trace if isinstance(trace, (DeviceBuffer, StagedTrace, int)) else np.ascontiguousarray(trace, dtype=np.uint64)
        rc = self.L.zkm_lookup_check(self.h, table_id, _data_ptr(keep), self.L.zkm_table_width(table_id), log_n, words, C.byref(err))
        findings, self.lookup_message = self._lookup_findings(rc, words, err)
        return findings[0]

    def segment_lookup_check(self, traces, log_ns):
        """zkm_segment_lookup_check: lookup_check on the twelve tables of a segment (Table::all() order; arrays, DeviceBuffers, device
        pointers, or a staged segment): the tables with lookups in one set of launches and one host wait.  Returns the twelve findings;
        .lookup_message names the first failing table (None when all hold)."""
        if isinstance(traces, StagedTrace):
            traces = traces.tables()
        assert len(traces) == 12 and len(log_ns) == 12
        keep = [t if isinstance(t, (DeviceBuffer, StagedTrace, int)) else np.ascontiguousarray(t, dtype=np.uint64) for t in traces]
        ptrs = (C.c_void_p * 12)(*[_data_ptr(t).value for t in keep])
        lg = (C.c_uint * 12)(*[int(x) for x in log_ns])
        words, err = (C.c_uint64 * (12 * LOOKUP_FINDING_WORDS))(), C.c_char_p()
        rc = self.L.zkm_segment_lookup_check(self.h, ptrs, lg, words, C.byref(err))
        findings, self.lookup_message = self._lookup_findings(rc, words, err)
        return findings

    def segments_check(self, segments):
        """zkm_segments_check: the three checks -- table constraints, range-check lookups, cross-table lookups -- on K segments in one set
        of launches and two host waits.  segments: a list of (traces, log_ns), traces as segment_witness_check takes them.  Returns per
        segment (verdict, witness findings, lookup findings, CtlReport): verdict = (kind, index) of the segment's first finding (kind 0
        consistent, 1 a table constraint, 2 a range-check lookup, 3 a cross-table lookup), the rest in the shapes of
        segment_witness_check, segment_lookup_check and segment_check_ctls.  .check_message holds the call's message: None when every
        segment is consistent, else "zkm_segments_check: segment <s>: ..." for the lowest segment with a finding."""
        return self._segments_check(segments, False)

    def segment_check(self, traces, log_ns):
        """zkm_segment_check: segments_check on one segment; returns its (verdict, witness findings, lookup findings, CtlReport)."""
        return self._segments_check([(traces, log_ns)], True)[0]

    def _segments_check(self, segments, single):
        k = len(segments)
        keep, seg_ptrs, seg_lgs = [], [], []
        for traces, log_ns in segments:
            if isinstance(traces, StagedTrace):
                traces = traces.tables()
            assert len(traces) == 12 and len(log_ns) == 12
            held = [t if isinstance(t, (DeviceBuffer, StagedTrace, int)) else np.ascontiguousarray(t, dtype=np.uint64) for t in traces]
            keep.append(held)
            seg_ptrs.append((C.c_void_p * 12)(*[_data_ptr(t).value for t in held]))
            seg_lgs.append((C.c_uint * 12)(*[int(x) for x in log_ns]))
        tp = (C.c_void_p * max(k, 1))(*[C.addressof(p) for p in seg_ptrs])
        lp = (C.c_void_p * max(k, 1))(*[C.addressof(p) for p in seg_lgs])
        verdicts = (C.c_uint64 * (SEGMENT_VERDICT_WORDS * max(k, 1)))()
        wf = (C.c_uint64 * (12 * WITNESS_FINDING_WORDS * max(k, 1)))()
        lf = (C.c_uint64 * (12 * LOOKUP_FINDING_WORDS * max(k, 1)))()
        reps, err = (CtlReport * max(k, 1))(), C.c_char_p()
        if single:
            rc = self.L.zkm_segment_check(self.h, seg_ptrs[0], seg_lgs[0], verdicts, wf, lf, reps, C.byref(err))
        else:
            rc = self.L.zkm_segments_check(self.h, k, tp, lp, verdicts, wf, lf, reps, C.byref(err))
        msg = err.value.decode() if err.value else None
        if rc != 0 and not re.match(r"zkm_segments?_check: segment \d+: (Constraint failed in |Lookup failed in |CTL #)", msg or ""):
            raise ZkmError(msg or "segments_check: error %d" % rc)
        self.check_message = msg
        witness, _ = self._witness_findings(0, wf, C.c_char_p())
        lookups, _ = self._lookup_findings(0, lf, C.c_char_p())
        out = []
        for s in range(k):
            rep = CtlReport.from_buffer_copy(reps[s])
            rep.message = None
            out.append(((int(verdicts[2 * s]), int(verdicts[2 * s + 1])), witness[12 * s:12 * s + 12], lookups[12 * s:12 * s + 12], rep))
        return out

    @staticmethod
    def _verify_reports(rc, reps, err):
        """The reports of a verify call; a call that could not be made (FAILED) raises.  The message belongs to the first rejection."""
        msg = err.value.decode() if err.value else None
        if rc != 0 and (not reps or all(r.code in (VERIFY_OK, VERIFY_FAILED) for r in reps)):
            e = ZkmError(msg or "verify: error %d" % rc)
            e.reports = reps
            raise e
        for r in reps:
            if r.code != VERIFY_OK:
                r.message = msg
                break
        return reps

    def verify_segments(self, proofs, public_values=None, ctl_challenges=None, cfg=None):
        """zkm_verify_segments: verify_proof (verifier.rs:27-176) on the device for K segments proven with the built-in AllStark.
        proofs: one uint64 array per segment (the twelve blobs as prove_segment* returns them); public_values / ctl_challenges: one
        array per segment, or None (a ctl_challenges entry may be None too).  Returns one VerifyReport per segment."""
        cfg = cfg or self.standard_config()
        K = len(proofs)
        keep = [np.ascontiguousarray(p, dtype=np.uint64) for p in proofs]
        pp = (C.c_void_p * K)(*[k.ctypes.data for k in keep])
        pw = (C.c_size_t * K)(*[k.size for k in keep])
        pubs = [np.ascontiguousarray(v, dtype=np.uint64) for v in public_values] if public_values is not None else None
        pv = (C.c_void_p * K)(*[v.ctypes.data if v.size else None for v in pubs]) if pubs is not None else None
        npv = (C.c_size_t * K)(*[v.size for v in pubs]) if pubs is not None else None
        chs = [None if v is None else np.ascontiguousarray(v, dtype=np.uint64) for v in ctl_challenges] if ctl_challenges is not None else None
        cc = (C.c_void_p * K)(*[None if v is None else v.ctypes.data for v in chs]) if chs is not None else None
        reps, err = (VerifyReport * K)(), C.c_char_p()
        rc = self.L.zkm_verify_segments(self.h, C.byref(cfg), K, pp, pw, pv, npv, cc, reps, C.byref(err))
        return self._verify_reports(rc, list(reps), err)

    def verify_proofs(self, tables, ctls, proofs, public_values=(), ctl_challenges=None, cfg=None):
        """zkm_verify_proofs: the general form, the mirror of prove_with_traces -- tables / ctls as that call takes them (a table's trace
        may be None: it is ignored), proofs = its concatenated blobs.  Returns the VerifyReport."""
        from . import ctl as zc
        cfg = cfg or self.standard_config()
        tarr, keep = zc.pack_tables([(tid, None, ncols, log_n, ct) for (tid, _tr, ncols, log_n, ct) in tables])
        carr, sides = zc.pack_ctls(ctls)
        proofs = np.ascontiguousarray(proofs, dtype=np.uint64)
        pub = np.ascontiguousarray(public_values, dtype=np.uint64)
        ch = None if ctl_challenges is None else np.ascontiguousarray(ctl_challenges, dtype=np.uint64)
        rep, err = VerifyReport(), C.c_char_p()
        rc = self.L.zkm_verify_proofs(self.h, C.byref(cfg), tarr, len(tables), carr.ctypes.data, sides.ctypes.data, len(carr),
                                      pub.ctypes.data_as(u64p), pub.size, proofs.ctypes.data_as(u64p), proofs.size,
                                      None if ch is None else ch.ctypes.data_as(u64p), C.byref(rep), C.byref(err))
        return self._verify_reports(rc, [rep], err)[0]

    def verify_single_table(self, proof, num_helpers, challenger=None, cfg=None, ncols=POSEIDON_COLS, table_id=TABLE_POSEIDON, naux=None):
        """zkm_verify_single_table: the mirror of prove_single_table (the benchmark's fake CtlData shape).  challenger: in/out like
        the prove call (advanced only when the proof is accepted).  Returns the VerifyReport."""
        cfg = cfg or self.standard_config()
        ch = challenger if challenger is not None else Challenger()
        if naux is None:
            naux = sum(int(h) + 1 for h in num_helpers)
        nh = (C.c_uint32 * len(num_helpers))(*num_helpers)
        proof = np.ascontiguousarray(proof, dtype=np.uint64)
        rep, err = VerifyReport(), C.c_char_p()
        rc = self.L.zkm_verify_single_table(self.h, table_id, C.byref(cfg), proof.ctypes.data_as(u64p), proof.size, ncols, naux, nh,
                                            len(num_helpers), C.byref(ch), C.byref(rep), C.byref(err))
        return self._verify_reports(rc, [rep], err)[0]

    def prove_with_traces(self, tables, ctls, public_values=(), cfg=None):
        """prove_with_traces (prover.rs:130-232).  tables: list of (table_id, trace (ndarray | DeviceBuffer), ncols, log_n, CtlTable);
        ctls: list of (looking=[(table, colset)..], looked=(table, colset)).  Returns (proofs, ctl_challenges, offsets)."""
        from . import ctl as zc
        cfg = cfg or self.standard_config()
        # (a trace given as a LIST of per-column arrays goes through zkm_table_input.columns: one pointer per column)
        packed = [(tid, [_data_ptr(col).value for col in tr] if isinstance(tr, (list, tuple)) else _data_ptr(tr).value, ncols, log_n, ct)
                  for (tid, tr, ncols, log_n, ct) in tables]
        tarr, keep = zc.pack_tables(packed)
        carr, sides = zc.pack_ctls(ctls)
        offs = (C.c_size_t * (len(tables) + 1))()
        total = self.L.zkm_all_proof_words(C.byref(cfg), tarr, len(tables), carr.ctypes.data, sides.ctypes.data, len(carr), offs)
        if total == 0 and len(tables):
            raise ZkmError("malformed cross-table lookups")
        proofs = np.zeros(total, dtype=np.uint64)
        chal = np.zeros(2 * cfg.num_challenges, dtype=np.uint64)
        pub = np.ascontiguousarray(public_values, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.L.zkm_prove_with_traces(self.h, C.byref(cfg), tarr, len(tables), carr.ctypes.data, sides.ctypes.data, len(carr),
                                            pub.ctypes.data_as(u64p), pub.size, proofs.ctypes.data_as(u64p), chal.ctypes.data_as(u64p),
                                            C.byref(err)), err)
        return proofs, chal, list(offs)

    def prove_segment(self, traces, log_ns, public_values=(), cfg=None):
        """prove_with_traces (prover.rs:130-232) on the twelve tables of Table::all() (all_stark.rs:117-134) with the AllStark
        description that ships inside the library: traces[t] = ndarray or DeviceBuffer of table t in enum order, log_ns[t] its
        height.  Returns (proofs, ctl_challenges, offsets)."""
        cfg = cfg or self.standard_config()
        assert len(traces) == 12 and len(log_ns) == 12
        if all(isinstance(t, (list, tuple)) for t in traces):
            return self._prove_segment_columns(traces, log_ns, public_values, cfg)
        keep = [t if isinstance(t, (DeviceBuffer, StagedTrace)) else np.ascontiguousarray(t, dtype=np.uint64) for t in traces]
        ptrs = (C.c_void_p * 12)(*[_data_ptr(t).value for t in keep])
        lg = (C.c_uint * 12)(*[int(x) for x in log_ns])
        pub = np.ascontiguousarray(public_values, dtype=np.uint64)
        offs = (C.c_size_t * 13)()
        err = C.c_char_p()
        _check(self.L.zkm_prove_segment(None, C.byref(cfg), ptrs, lg, pub.ctypes.data_as(u64p), pub.size, None, offs, None, C.byref(err)), err)
        proofs = np.zeros(offs[12], dtype=np.uint64)
        chal = np.zeros(2 * cfg.num_challenges, dtype=np.uint64)
        _check(self.L.zkm_prove_segment(self.h, C.byref(cfg), ptrs, lg, pub.ctypes.data_as(u64p), pub.size, proofs.ctypes.data_as(u64p), offs,
                                        chal.ctypes.data_as(u64p), C.byref(err)), err)
        return proofs, chal, list(offs)

    def prove_segments(self, segments, cfg=None):
        """zkm_prove_segments: K independent segments in lock-step (one launch per stage for all segments whose table has the same
        height).  segments = list of (traces, log_ns, public_values) as prove_segment takes them.  Returns a list of
        (proofs, ctl_challenges, offsets), one per segment -- each equal to prove_segment's result for that segment alone."""
        cfg = cfg or self.standard_config()
        m = _marshal_segments(self.L, segments, cfg)
        err = C.c_char_p()
        fn = self.L.zkm_prove_segments_columns if m.by_columns else self.L.zkm_prove_segments
        _check(fn(self.h, C.byref(cfg), len(segments), m.tr, m.lg, m.pv, m.npv, m.po, m.co, C.byref(err)), err)
        return m.results()

    def _prove_segment_columns(self, traces, log_ns, public_values, cfg):
        """zkm_prove_segment_columns: traces[t] = list of per-column arrays (each its own allocation, like Vec<PolynomialValues<F>>)."""
        keep = [[c if isinstance(c, (DeviceBuffer, StagedTrace)) else np.ascontiguousarray(c, dtype=np.uint64) for c in t] for t in traces]
        cols = [(C.c_void_p * len(t))(*[_data_ptr(c).value for c in t]) for t in keep]
        tabs = (C.c_void_p * 12)(*[C.addressof(c) for c in cols])
        lg = (C.c_uint * 12)(*[int(x) for x in log_ns])
        pub = np.ascontiguousarray(public_values, dtype=np.uint64)
        offs = (C.c_size_t * 13)()
        err = C.c_char_p()
        _check(self.L.zkm_prove_segment_columns(None, C.byref(cfg), tabs, lg, pub.ctypes.data_as(u64p), pub.size, None, offs, None, C.byref(err)), err)
        proofs = np.zeros(offs[12], dtype=np.uint64)
        chal = np.zeros(2 * cfg.num_challenges, dtype=np.uint64)
        _check(self.L.zkm_prove_segment_columns(self.h, C.byref(cfg), tabs, lg, pub.ctypes.data_as(u64p), pub.size, proofs.ctypes.data_as(u64p),
                                                offs, chal.ctypes.data_as(u64p), C.byref(err)), err)
        return proofs, chal, list(offs)

    def prove_segment_image(self, image, cfg=None):
        """Prove every table of a ZKMTRACE segment image (see segment_image()).  Returns (proofs, ctl_challenges, offsets)."""
        cfg = cfg or self.standard_config()
        image = np.ascontiguousarray(image, dtype=np.uint64)
        ntables = int(image[2]) if image.size > 2 else 0
        offs = (C.c_size_t * (ntables + 1))()
        total = C.c_size_t()
        err = C.c_char_p()
        _check(self.L.zkm_prove_segment_image(self.h, C.byref(cfg), image.ctypes.data_as(u64p), image.size, None, C.byref(total), offs,
                                              None, C.byref(err)), err)
        proofs = np.zeros(total.value, dtype=np.uint64)
        chal = np.zeros(2 * cfg.num_challenges, dtype=np.uint64)
        _check(self.L.zkm_prove_segment_image(self.h, C.byref(cfg), image.ctypes.data_as(u64p), image.size, proofs.ctypes.data_as(u64p),
                                              C.byref(total), offs, chal.ctypes.data_as(u64p), C.byref(err)), err)
        return proofs, chal, list(offs)

    def _fri_instance(self, oracles, batches, cfg):
        """what zkm_fri_prove and zkm_fri_prove_stack take of a FRI instance: (oracle handles, number of proof words, FriBatch array, the
        arrays it points into); batches = [((c0, c1), polynomial list), ...]"""
        orc = (C.c_void_p * len(oracles))(*[o.h.value for o in oracles])
        cols = (C.c_size_t * len(oracles))(*[o.ncols for o in oracles])
        words = self.L.zkm_fri_proof_words(C.byref(cfg), oracles[0].log_n, cols, len(oracles))
        if not words:
            raise ZkmError("zkm_fri_proof_words: unsupported configuration")
        keep, arr = [], (FriBatch * len(batches))()
        for i, (pt, polys) in enumerate(batches):
            a = np.array(polys, dtype=np.uint32).reshape(-1, 2)
            keep.append(a)
            arr[i] = FriBatch((C.c_uint64 * 2)(int(pt[0]), int(pt[1])), a.ctypes.data, len(a))
        return C.cast(orc, C.POINTER(C.c_void_p)), words, C.cast(arr, C.c_void_p), (orc, arr, keep)

    def fri_prove(self, oracles, batches, challenger, cfg=None):
        """PolynomialBatch::prove_openings for an arbitrary FriInstanceInfo: oracles = list of PolynomialBatch, batches = list of
        ((point_c0, point_c1), [(oracle_index, polynomial_index), ...]).  Returns the FRI proof blob (layout in zkm_hip.h)."""
        cfg = cfg or self.standard_config()
        orc, words, arr, keep = self._fri_instance(oracles, batches, cfg)
        out = np.zeros(words, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.L.zkm_fri_prove(self.h, C.byref(cfg), orc, len(oracles), arr, len(batches), C.byref(challenger), out.ctypes.data_as(u64p),
                                    C.byref(err)), err)
        return out

    def fri_prove_stack(self, oracles, batches, points, challengers, cfg=None):
        """zkm_fri_prove_stack: K opening proofs of one instance in lock-step.  oracles = list of PolynomialBatchStack of one size K;
        batches = the polynomial lists [[(oracle_index, polynomial_index), ...], ...] the K claims share; points[k][b] = claim k's
        (c0, c1) of batch b; challengers = K Challenger, in/out.  Returns the K FRI proof blobs: blob k is fri_prove's on member k of
        every oracle."""
        cfg = cfg or self.standard_config()
        K = len(challengers)
        orc, words, arr, keep = self._fri_instance(oracles, [((0, 0), polys) for polys in batches], cfg)
        pts = np.ascontiguousarray([[int(w) for w in pt] for claim in points for pt in claim], dtype=np.uint64).reshape(-1)
        if pts.size != K * len(batches) * 2:
            raise ZkmError("fri_prove_stack: points must be K x nbatches x 2 words")
        out = np.zeros((K, words), dtype=np.uint64)
        chs = (C.c_void_p * K)(*[C.addressof(ch) for ch in challengers])
        outs = (C.c_void_p * K)(*[out[k].ctypes.data for k in range(K)])
        err = C.c_char_p()
        _check(self.L.zkm_fri_prove_stack(self.h, C.byref(cfg), orc, len(oracles), arr, len(batches), pts.ctypes.data, chs, outs,
                                          C.byref(err)), err)
        return list(out)

    def fri_verify(self, claims, cfg=None):
        """zkm_fri_verify: plonky2's verify_fri_proof for any FriInstanceInfo, on all claims in one set of launches.  claims = list of
        FriClaim.  Returns one VerifyReport per claim (the first rejected one carries .message); a call that could not be made raises
        ZkmError.  An accepted claim's challenger is advanced to the state fri_prove left; a rejected claim's is untouched."""
        cfg = cfg or self.standard_config()
        K = len(claims)
        keep = []

        def words(a):
            keep.append(np.ascontiguousarray(a, dtype=np.uint64))
            return keep[-1].ctypes.data

        def pointers(addresses):
            keep.append((C.c_void_p * len(addresses))(*addresses))
            return C.addressof(keep[-1])
        proofs = [np.ascontiguousarray(cl.proof, dtype=np.uint64) for cl in claims]
        pp = (C.c_void_p * K)(*[p.ctypes.data for p in proofs])
        pw = (C.c_size_t * K)(*[p.size if cl.proof_words is None else cl.proof_words for p, cl in zip(proofs, claims)])
        lg = (C.c_uint * K)(*[int(cl.log_n) for cl in claims])
        cols = [(C.c_size_t * len(cl.oracle_cols))(*cl.oracle_cols) for cl in claims]
        cc = (C.c_void_p * K)(*[C.addressof(a) for a in cols])
        no = (C.c_size_t * K)(*[len(cl.oracle_cols) for cl in claims])
        caps = (C.c_void_p * K)(*[pointers([words(cap) for cap in cl.oracle_caps]) for cl in claims])
        barrs = []
        for cl in claims:
            arr = (FriBatch * len(cl.batches))()
            for i, (pt, polys) in enumerate(cl.batches):
                a = np.array(polys, dtype=np.uint32).reshape(-1, 2)
                keep.append(a)
                arr[i] = FriBatch((C.c_uint64 * 2)(int(pt[0]), int(pt[1])), a.ctypes.data, len(a))
            barrs.append(arr)
        bb = (C.c_void_p * K)(*[C.addressof(a) for a in barrs])
        nb = (C.c_size_t * K)(*[len(cl.batches) for cl in claims])
        opened = (C.c_void_p * K)(*[pointers([words(o) for o in cl.opened]) for cl in claims])
        chs = (C.c_void_p * K)(*[C.addressof(cl.challenger) for cl in claims])
        reps, err = (VerifyReport * K)(), C.c_char_p()
        rc = self.L.zkm_fri_verify(self.h, C.byref(cfg), K, pp, pw, lg, cc, no, caps, bb, nb, opened, chs, reps, C.byref(err))
        return self._verify_reports(rc, list(reps), err)

    def prove_openings(self, trace_batch, aux_batch, quot_batch, nctl_zs, challenger=None, cfg=None):
        """PolynomialBatch::prove_openings for the STARK FRI instance on three existing commitments (BASELINE config 4)."""
        cfg = cfg or self.standard_config()
        ch = challenger if challenger is not None else Challenger()
        proof = np.zeros(self.proof_words(cfg, trace_batch.log_n, trace_batch.ncols, aux_batch.ncols, nctl_zs), dtype=np.uint64)
        err = C.c_char_p()
        _check(self.L.zkm_prove_openings(self.h, C.byref(cfg), trace_batch.h, aux_batch.h, quot_batch.h, nctl_zs, C.byref(ch),
                                         proof.ctypes.data_as(u64p), C.byref(err)), err)
        return proof

    def quotient(self, trace_batch, aux_batch, num_helpers, alphas, table_id=TABLE_POSEIDON):
        nh = (C.c_uint32 * len(num_helpers))(*num_helpers)
        al = np.ascontiguousarray(alphas, dtype=np.uint64)
        out = np.zeros(al.size * (2 << trace_batch.log_n), dtype=np.uint64)
        err = C.c_char_p()
        _check(self.L.zkm_quotient(self.h, table_id, trace_batch.h, aux_batch.h, nh, len(num_helpers),
                                   al.ctypes.data_as(u64p), al.size, _np_ptr(out), C.byref(err)), err)
        return out

    def eval_openings(self, batch, zeta):
        z = np.array(zeta, dtype=np.uint64)
        out = np.zeros(2 * batch.ncols, dtype=np.uint64)
        err = C.c_char_p()
        _check(self.L.zkm_eval_openings(self.h, batch.h, z.ctypes.data_as(u64p), out.ctypes.data_as(u64p), C.byref(err)), err)
        return out

    def eval_openings_stack(self, stack, zetas):
        """zkm_eval_openings_stack: member k's polynomials at zetas[k] = (c0, c1); returns nstack x (2 ncols) words"""
        z = np.ascontiguousarray([[int(w) for w in zeta] for zeta in zetas], dtype=np.uint64).reshape(-1)
        if z.size != 2 * stack.nstack:
            raise ZkmError("eval_openings_stack: one point per member")
        out = np.zeros((stack.nstack, 2 * stack.ncols), dtype=np.uint64)
        err = C.c_char_p()
        _check(self.L.zkm_eval_openings_stack(self.h, stack.h, z.ctypes.data, out.ctypes.data, C.byref(err)), err)
        return out


class _BatchHandle:
    """owner of one zkm_batch handle -- a single commitment or a stack of them"""

    def __init__(self, ctx, h, ncols, log_n, rate_bits, cap_height):
        self.ctx, self.h, self.ncols, self.log_n, self.rate_bits, self.cap_height = ctx, h, ncols, log_n, rate_bits, cap_height

    @staticmethod
    def _commit(call):
        """the handle one zkm_batch_commit_* entry makes: call(&handle, &err) -> status"""
        h, err = C.c_void_p(), C.c_char_p()
        _check(call(C.byref(h), C.byref(err)), err)
        return h

    def free(self):
        if self.h:
            self.ctx.L.zkm_batch_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            if self.ctx.h:
                self.free()
        except Exception:
            pass

    @property
    def lde_bits(self):
        return self.log_n + self.rate_bits


class PolynomialBatch(_BatchHandle):
    """== plonky2 PolynomialBatch<F, PoseidonGoldilocksConfig, 2> living in HBM."""

    @classmethod
    def from_values(cls, ctx, values, ncols, log_n, rate_bits=2, cap_height=4):
        h = cls._commit(lambda h, err: ctx.L.zkm_batch_commit_values(ctx.h, _data_ptr(values), ncols, log_n, rate_bits, cap_height, h, err))
        return cls(ctx, h, ncols, log_n, rate_bits, cap_height)

    @classmethod
    def from_columns(cls, ctx, columns, log_n, values=True, rate_bits=2, cap_height=4):
        """from_values / from_coeffs from one array per column (zkm_batch_commit_columns): the shape of the reference's
        Vec<PolynomialValues<F>> -- nothing is flattened on the host."""
        keep = [c if isinstance(c, (DeviceBuffer, StagedTrace)) else np.ascontiguousarray(c, dtype=np.uint64) for c in columns]
        ptrs = (C.c_void_p * len(keep))(*[_data_ptr(c).value for c in keep])
        h = cls._commit(lambda h, err: ctx.L.zkm_batch_commit_columns(ctx.h, ptrs, len(keep), log_n, int(bool(values)), rate_bits, cap_height, h, err))
        return cls(ctx, h, len(keep), log_n, rate_bits, cap_height)

    @classmethod
    def from_coeffs(cls, ctx, coeffs, ncols, log_n, rate_bits=2, cap_height=4):
        h = cls._commit(lambda h, err: ctx.L.zkm_batch_commit_coeffs(ctx.h, _data_ptr(coeffs), ncols, log_n, rate_bits, cap_height, h, err))
        return cls(ctx, h, ncols, log_n, rate_bits, cap_height)

    def cap(self):
        out = np.zeros(4 << self.cap_height, dtype=np.uint64)
        assert self.ctx.L.zkm_batch_cap(self.h, out.ctypes.data_as(u64p)) == 0
        return out

    def coeffs(self):
        out = np.zeros(self.ncols << self.log_n, dtype=np.uint64)
        assert self.ctx.L.zkm_batch_coeffs(self.h, _np_ptr(out)) == 0
        return out

    def lde_row(self, natural_index):
        out = np.zeros(self.ncols, dtype=np.uint64)
        assert self.ctx.L.zkm_batch_lde_row(self.h, natural_index, out.ctypes.data_as(u64p)) == 0
        return out

    def lde_rows(self, index_start, step, count):
        """get_lde_values_packed(index_start, step) for `count` consecutive indices: count x ncols."""
        out = np.zeros(count * self.ncols, dtype=np.uint64)
        if self.ctx.L.zkm_batch_lde_rows(self.h, index_start, step, count, _np_ptr(out)) != 0:
            raise ZkmError("zkm_batch_lde_rows failed")
        return out.reshape(count, self.ncols)

    def leaf(self, i):
        out = np.zeros(self.ncols, dtype=np.uint64)
        assert self.ctx.L.zkm_batch_leaf(self.h, i, out.ctypes.data_as(u64p)) == 0
        return out

    def merkle_path(self, i):
        out = np.zeros(4 * (self.lde_bits - self.cap_height), dtype=np.uint64)
        assert self.ctx.L.zkm_batch_merkle_path(self.h, i, out.ctypes.data_as(u64p)) == 0
        return out

    def digest_layer(self, level):
        out = np.zeros(4 << (self.lde_bits - level), dtype=np.uint64)
        assert self.ctx.L.zkm_batch_digest_layer(self.h, level, out.ctypes.data_as(u64p)) == 0
        return out


class PolynomialBatchStack(_BatchHandle):
    """nstack same-shaped PolynomialBatch in one handle, built in one set of launches (zkm_batch_commit_values_stack / _coeffs_stack):
    the oracles of Context.fri_prove_stack and eval_openings_stack.  Member k is the single PolynomialBatch of the same words."""

    def __init__(self, ctx, h, nstack, ncols, log_n, rate_bits, cap_height):
        super().__init__(ctx, h, ncols, log_n, rate_bits, cap_height)
        self.nstack = nstack

    @classmethod
    def _commit_members(cls, fn, ctx, members, ncols, log_n, rate_bits, cap_height):
        keep = [np.ascontiguousarray(m, dtype=np.uint64) if isinstance(m, (np.ndarray, list, tuple)) else m for m in members]
        ptrs = (C.c_void_p * len(keep))(*[None if m is None else _data_ptr(m).value for m in keep])
        h = cls._commit(lambda h, err: fn(ctx.h, ptrs, len(keep), ncols, log_n, rate_bits, cap_height, h, err))
        return cls(ctx, h, len(keep), ncols, log_n, rate_bits, cap_height)

    @classmethod
    def from_values(cls, ctx, values, ncols, log_n, rate_bits=2, cap_height=4):
        """values = one array (or DeviceBuffer) of ncols << log_n words per member"""
        return cls._commit_members(ctx.L.zkm_batch_commit_values_stack, ctx, values, ncols, log_n, rate_bits, cap_height)

    @classmethod
    def from_coeffs(cls, ctx, coeffs, ncols, log_n, rate_bits=2, cap_height=4):
        return cls._commit_members(ctx.L.zkm_batch_commit_coeffs_stack, ctx, coeffs, ncols, log_n, rate_bits, cap_height)

    def __len__(self):
        return int(self.ctx.L.zkm_batch_stack_size(self.h))

    def cap(self, k):
        out = np.zeros(4 << self.cap_height, dtype=np.uint64)
        if self.ctx.L.zkm_batch_stack_cap(self.h, k, out.ctypes.data) != 0:
            raise ZkmError("zkm_batch_stack_cap failed")
        return out

    def coeffs(self, k):
        out = np.zeros(self.ncols << self.log_n, dtype=np.uint64)
        if self.ctx.L.zkm_batch_stack_coeffs(self.h, k, _np_ptr(out)) != 0:
            raise ZkmError("zkm_batch_stack_coeffs failed")
        return out

    def merkle_path(self, k, i):
        """(leaf i of member k's tree, its Merkle path)"""
        leaf, sib = np.zeros(self.ncols, dtype=np.uint64), np.zeros(4 * (self.lde_bits - self.cap_height), dtype=np.uint64)
        if self.ctx.L.zkm_batch_stack_merkle_path(self.h, k, i, leaf.ctypes.data, sib.ctypes.data) != 0:
            raise ZkmError("zkm_batch_stack_merkle_path failed")
        return leaf, sib


def challenger_new():
    ch = Challenger()
    load().zkm_challenger_init(C.byref(ch))
    return ch


def challenger_observe(ch, elems):
    a = np.ascontiguousarray(elems, dtype=np.uint64)
    load().zkm_challenger_observe(C.byref(ch), a.ctypes.data_as(u64p), a.size)


def challenger_get(ch):
    return load().zkm_challenger_get(C.byref(ch))


def proof_layout(proof):
    """Field offsets of a proof blob (zkm_proof_get_layout / zkm_proof_get_query_layout).  No GPU needed."""
    L = load()
    proof = np.ascontiguousarray(proof, dtype=np.uint64)
    lay, q = ProofLayout(), ProofQueryLayout()
    if L.zkm_proof_get_layout(proof.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(lay)) or \
            L.zkm_proof_get_query_layout(proof.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(q)):
        raise ZkmError("not a proof blob")
    return lay, q


def segment_image(tables, ctls, public_values=()):
    """Serialise a segment (host traces + cross-table lookups, same arguments as Context.prove_with_traces) into one ZKMTRACE image
    (zkm_segment_image_write).  No GPU needed."""
    from . import ctl as zc
    L = load()
    packed = [(tid, _data_ptr(tr).value, ncols, log_n, ct) for (tid, tr, ncols, log_n, ct) in tables]
    tarr, keep = zc.pack_tables(packed)
    carr, sides = zc.pack_ctls(ctls)
    pub = np.ascontiguousarray(public_values, dtype=np.uint64)
    words = L.zkm_segment_image_words(tarr, len(tables), carr.ctypes.data, sides.ctypes.data, len(carr), pub.size)
    img = np.zeros(words, dtype=np.uint64)
    err = C.c_char_p()
    u64p = C.POINTER(C.c_uint64)
    _check(L.zkm_segment_image_write(tarr, len(tables), carr.ctypes.data, sides.ctypes.data, len(carr), pub.ctypes.data_as(u64p), pub.size,
                                     img.ctypes.data_as(u64p), C.byref(err)), err)
    return img
