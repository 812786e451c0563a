"""CPU suite: the lock on the C ABI.  include/zkm_hip.h is its only statement (zkm_amd/abi.py reads it, the ctypes binding is derived from
it); three independent judges are held against it here, for every function, struct and constant at once: the C compiler (the layout
probe), the linker (`nm -D` of libzkmhip.so) and the hand-written Rust block integration/rust/zkm_hip_sys.rs.  Below that: host-side
transcript code (no GPU needed) agrees with the oracle."""
import ctypes as C
import functools
import glob
import itertools
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUST_SYS = os.path.join(ROOT, "integration", "rust", "zkm_hip_sys.rs")


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def header_text():
    """include/zkm_hip.h without its comments."""
    return re.sub(r"/\*.*?\*/", " ", read("include", "zkm_hip.h"), flags=re.S)


def prototypes():
    """{function: (return type, [(parameter type, parameter name)])} of the header."""
    from zkm_amd import abi
    return {name: (ret, params) for name, ret, params in abi.prototypes()}


def rust_sys_text():
    return re.sub(r"//[^\n]*", "", open(RUST_SYS).read())


# extern "C" functions one file of csrc/ calls in another (csrc/zkm_internal.h): visible to the linker, no part of the C ABI
LINKAGE_ONLY = {"zkm_prove_segments_entry", "zkm_prove_segments_ops_entry", "zkm_staged_from_segment"}


def test_library_exports_every_declared_symbol(zkm):
    """The linker's list of the library's zkm_* functions, the header's prototypes and the binding's EXPORTS are one set; the header
    reader saw every `typedef struct` (a struct or a handle it skipped would leave the locks below with a hole)."""
    lib = zkm.load()
    names = [n for n, _, _ in zkm.abi.prototypes()]
    assert len(names) == len(set(names)) >= 129 and names == zkm.EXPORTS
    dynamic = subprocess.check_output(["nm", "-D", "--defined-only", zkm._LIB_PATH], text=True)
    assert set(re.findall(r" T (zkm_\w+)", dynamic)) - LINKAGE_ONLY == set(names), (set(re.findall(r" T (zkm_\w+)", dynamic)) - LINKAGE_ONLY) ^ set(names)
    assert len(re.findall(r"\btypedef\s+struct\b", header_text())) == len(zkm.abi.structs()) + len(zkm.abi.opaque())
    assert zkm.abi.opaque() == ["zkm_ctx", "zkm_batch", "zkm_staged", "zkm_staged_ops", "zkm_pool"]
    assert b"gfx950" in lib.zkm_version()


# the binding's own statement of the C types, independent of zkm_amd's: scalars and returns exactly, pointers by kind
C_TO_CTYPES = {"int": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "void": None}
C_TYPED_POINTEES = {"size_t": C.c_size_t, "unsigned": C.c_uint, "int": C.c_int, "double": C.c_double}


def test_python_binding_has_the_headers_types_for_every_function(zkm):
    """restype and every argtype of the ctypes binding against the header, by a table of this file's own: scalars and scalar returns exactly;
    `const char*` is c_char_p; a pointer return is c_void_p; every pointer parameter is c_void_p or a ctypes pointer, typed where the
    pointee is a count (size_t / unsigned / int / double), the struct's mirror where the struct is passed by reference, and never typed
    where it is a data word (device addresses are passed as integers)."""
    lib, mirrors = zkm.load(), zkm.abi_mirrors()
    checked = 0
    for name, (ret, params) in prototypes().items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(params), name
        if "*" not in ret:
            assert fn.restype is C_TO_CTYPES[ret], (name, ret)
        else:
            assert fn.restype is (C.c_char_p if ret == "const char*" else C.c_void_p), (name, ret)
        for got, (ty, arg) in zip(fn.argtypes, params):
            base, stars = ty.replace("const ", "").replace(" const", "").rstrip("*"), ty.count("*")
            if stars == 0:
                assert got is C_TO_CTYPES[base] and got is not None, (name, arg, ty)
            elif base == "char":
                assert got is {"const char*": C.c_char_p, "char**": C.POINTER(C.c_char_p), "const char**": C.POINTER(C.c_char_p)}[ty], (name, arg)
            elif stars > 1:
                assert got is C.POINTER(C.c_void_p), (name, arg, ty)
            elif base in C_TYPED_POINTEES:
                assert got is C.POINTER(C_TYPED_POINTEES[base]), (name, arg, ty)
            elif base in zkm.BY_REFERENCE:
                assert issubclass(got, C._Pointer) and got._type_ is mirrors[base], (name, arg, ty)
            else:
                assert got is C.c_void_p and (base in ("void", "uint8_t", "uint32_t", "uint64_t") or base in mirrors or base in zkm.abi.opaque()), (name, arg, ty)
            checked += 1
    assert checked >= 737


def test_no_gpu_fails_loudly(zkm):
    import torch
    if torch.cuda.is_available():
        return
    try:
        zkm.Context(0)
    except zkm.ZkmError as e:
        assert "hip" in str(e).lower()
    else:
        raise AssertionError("Context creation must fail without a GPU (no CPU fallback)")


def test_host_challenger_matches_oracle(zkm, oracle):
    rng = np.random.default_rng(11)
    a, b = zkm.challenger_new(), oracle.challenger()
    for step in range(40):
        k = int(rng.integers(0, 20))
        elems = rng.integers(0, zkm.P, k, dtype=np.uint64)
        zkm.challenger_observe(a, elems)
        oracle.observe(b, elems)
        for _ in range(int(rng.integers(0, 11))):
            assert zkm.challenger_get(a) == oracle.challenge(b)
    assert list(a.state) == list(b.state)


def test_host_permutation_edge_states_match_oracle(zkm, oracle):
    """The host-side permutation (csrc/host_poseidon.hip: sparse partial rounds, 128-bit accumulation, vectorised MDS) on the states
    that exercise its carries and borrows: all-zero, all p - 1, single words at the limb boundaries, long runs of random blocks --
    through the Challenger (the only way host code reaches it), against the oracle's independent permutation."""
    P = zkm.P
    edge = [0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, P - 1, P - 2, P - (1 << 32), (1 << 63), (1 << 63) - 1, P >> 1]
    rng = np.random.default_rng(12)
    blocks = [[e] * 8 for e in edge]
    blocks += [[edge[(i + k) % len(edge)] for k in range(8)] for i in range(len(edge))]
    blocks += [[int(x) for x in rng.integers(0, P, 8, dtype=np.uint64)] for _ in range(3000)]
    a, b = zkm.challenger_new(), oracle.challenger()
    for i, blk in enumerate(blocks):
        zkm.challenger_observe(a, blk)
        oracle.observe(b, blk)
        if i % 64 == 0 or i < 30:
            assert list(a.state) == list(b.state), i
    assert list(a.state) == list(b.state)
    for _ in range(8):
        assert zkm.challenger_get(a) == oracle.challenge(b)


def fri_num_layers(log_n, rate_bits, cap_height, arity_bits, final_poly_bits):
    """FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits) (plonky2 fri/reduction_strategies.rs): reduce by
    arity_bits while the degree is above final_poly_bits and the next layer's tree still reaches down to its cap."""
    layers, d = 0, log_n
    while d > final_poly_bits and d + rate_bits - arity_bits >= cap_height:
        assert d >= arity_bits
        d -= arity_bits
        layers += 1
    return layers


def test_proof_layout_sizes_agree(zkm, oracle):
    """Three statements of the blob's size agree on a grid of configurations, heights and table shapes: zkm_proof_words (from the
    configuration), the oracle's proof_words, and zkm_proof_get_layout on a header written here.  The public layout's fields tile the
    blob in the order and with the sizes include/zkm_hip.h states, and so do the fields of a query round."""
    cfg_o = oracle.standard_config()
    cfg = zkm.StarkConfig()
    zkm.load().zkm_standard_config(C.byref(cfg))
    for f, _ in cfg._fields_:
        assert getattr(cfg, f) == getattr(cfg_o, f)
    lib = zkm.load()
    for log_n in (5, 7, 12, 16, 20, 22):
        assert lib.zkm_proof_words(C.byref(cfg), log_n, 262, 4, 2) == oracle.proof_words(cfg_o, log_n, 262, 4, 2)
    magic = int.from_bytes(b"FOORPMKZ", "little")          # "ZKMPROOF" read as a big-endian word
    cases = 0
    for cap, arity_bits, nq, nch in itertools.product((0, 2, 4), (2, 3, 4), (1, 37), (1, 2)):
        for c in (cfg, cfg_o):
            c.cap_height, c.arity_bits, c.num_queries, c.num_challenges, c.final_poly_bits = cap, arity_bits, nq, nch, 5
        rate = cfg.rate_bits
        for log_n, (W, A, Z) in itertools.product((2, 5, 6, 9, 10, 13, 16, 22), ((262, 4, 2), (9, 3, 1), (2431, 61, 20))):
            L = fri_num_layers(log_n, rate, cap, arity_bits, 5)
            F, Q, C4, lde_bits = 1 << (log_n - L * arity_bits), 2 * nch, 4 << cap, log_n + rate
            header = np.array([magic, log_n, W, A, Q, Z, cap, L, F, nq, rate, arity_bits, 0, 0, 0, 0], dtype=np.uint64)
            lay, q = zkm.proof_layout(header)
            words = lib.zkm_proof_words(C.byref(cfg), log_n, W, A, Z)
            assert words != 0 and words == oracle.proof_words(cfg_o, log_n, W, A, Z) == lay.total_words, (cap, arity_bits, nq, nch, log_n, W)
            at = 16
            for name, size in (("init_challenger_state", 12), ("trace_cap", C4), ("aux_cap", C4), ("quotient_cap", C4), ("local_values", 2 * W),
                               ("next_values", 2 * W), ("aux_polys", 2 * A), ("aux_polys_next", 2 * A), ("ctl_zs_first", Z),
                               ("quotient_polys_open", 2 * Q), ("commit_phase_merkle_caps", L * C4), ("final_poly", 2 * F), ("pow_witness", 1),
                               ("query_round_proofs", nq * lay.query_round_words)):
                assert getattr(lay, name) == at, (name, cap, arity_bits, nq, nch, log_n, W)
                at += size
            assert at == lay.total_words
            at = 0
            assert q.initial_siblings == lde_bits - cap
            for k, cols in enumerate((W, A, Q)):
                assert (q.oracle_evals[k], q.oracle_cols[k], q.oracle_siblings[k]) == (at, cols, at + cols)
                at += cols + 4 * (lde_bits - cap)
            for i in range(L):
                count = lde_bits - arity_bits * (i + 1) - cap
                assert (q.layer_evals[i], q.layer_siblings[i], q.layer_siblings_count[i]) == (at, at + (2 << arity_bits), count)
                at += (2 << arity_bits) + 4 * count
            assert at == lay.query_round_words
            cases += 1
    assert cases == 864


def test_all_stark_ctl_inc_is_current():
    """csrc/all_stark_ctl.inc (the AllStark lookups compiled into the library) is generated from zkm_amd/tables.py."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_all_stark_ctl", os.path.join(ROOT, "tools", "gen_all_stark_ctl.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.render() == open(os.path.join(ROOT, "zkm_amd", "csrc", "all_stark_ctl.inc")).read(), "run tools/gen_all_stark_ctl.py"


def test_all_stark_looking_side_order_is_the_references():
    """The looking sides of every lookup come in the order the reference chains them (all_stark.rs): a consumer that indexes them
    positionally (verify_cross_table_lookups, the recursion circuits) must see the same sequence.  ctl_memory (:479-542): the CPU's
    NUM_GP_CHANNELS memory channels, then KeccakSponge (136 rate bytes), PoseidonSponge (32), ShaExtendSponge, ShaCompressSponge,
    ShaCompress (4); ctl_logic (:340-477): CPU, KeccakSponge, ShaExtend, ShaCompress."""
    from zkm_amd import tables as T
    AR, CPU, PO, PS, KK, KS, SE, SES, SC, SCS, LO, ME = range(12)
    _, ctls = T.all_cross_table_lookups()
    assert len(ctls) == 15

    def runs(sides):
        out = []
        for t, _ in sides:
            if out and out[-1][0] == t:
                out[-1][1] += 1
            else:
                out.append([t, 1])
        return [tuple(r) for r in out]
    mem_looking, mem_looked = ctls[14]
    assert mem_looked[0] == ME
    r = runs(mem_looking)
    assert [t for t, _ in r] == [CPU, KS, PS, SES, SCS, SC], r
    assert dict(r)[KS] == 136 and dict(r)[PS] == 32 and dict(r)[SC] == 4
    logic_looking, logic_looked = ctls[13]
    assert logic_looked[0] == LO and [t for t, _ in runs(logic_looking)] == [CPU, KS, SE, SC]
    # the looked tables of the fifteen lookups, in all_cross_table_lookups() order (all_stark.rs:137-155)
    assert [looked[0] for _, looked in ctls] == [AR, PS, PO, PO, KS, KK, KK, SES, SE, SE, SCS, SC, SC, LO, ME]


def test_prove_segment_sizing_and_descriptors(zkm, oracle):
    """zkm_prove_segment sizes a whole AllStark segment without a GPU, from the description inside the library; it agrees with the
    oracle's sizing of the same tables + lookups built through zkm_amd/tables.py, and the exported lookups are the fifteen of
    all_cross_table_lookups() (all_stark.rs:136-155)."""
    from zkm_amd import tables as T
    lib = zkm.load()
    seg = np.load(os.path.join(ROOT, "tests", "golden", "segment12.npz"))
    log_n = [int(x) for x in seg["log_n"]]
    ctl_tables, ctls = T.all_cross_table_lookups()
    tables = [(T.TABLE_ENUM_ORDER[i], seg["t%d" % i], T.WIDTH[T.TABLE_ENUM_ORDER[i]], log_n[i], ctl_tables[i]) for i in range(12)]
    want_total, want_offs = oracle.all_proof_words(tables, ctls)
    cfg = zkm.StarkConfig()
    lib.zkm_standard_config(C.byref(cfg))
    ptrs = (C.c_void_p * 12)(*[t[1].ctypes.data for t in tables])
    lg = (C.c_uint * 12)(*log_n)
    offs = (C.c_size_t * 13)()
    err = C.c_char_p()
    assert lib.zkm_prove_segment(None, C.byref(cfg), ptrs, lg, None, 0, None, offs, None, C.byref(err)) == 0
    assert list(offs) == list(want_offs) and offs[12] == want_total
    n, ns = C.c_size_t(), C.c_size_t()
    assert lib.zkm_all_stark_ctls(None, C.byref(n), None, C.byref(ns)) == 0
    assert n.value == 15 and ns.value == sum(len(looking) for looking, _ in ctls)
    assert [lib.zkm_table_enum_index(t) for t in T.TABLE_ENUM_ORDER] == list(range(12)) and lib.zkm_table_enum_index(99) == -1
    # the library's registry of the tables against the Python model's own copy: widths, order, own lookups
    assert sorted(T.TABLE_ENUM_ORDER) == list(range(12))
    for tid in range(12):
        assert lib.zkm_table_width(tid) == T.WIDTH[tid], tid
        # ((ncols + 1) / 2 + 1) helper and Z columns per challenge: Memory looks up 1 column, Arithmetic 18
        want = {T.TABLE_MEMORY: 2, T.TABLE_ARITHMETIC: 10}.get(tid, 0) * cfg.num_challenges
        assert lib.zkm_num_lookup_columns(tid, C.byref(cfg)) == want, tid
    for tid in (-1, 12, 99):
        assert lib.zkm_table_width(tid) == 0 and lib.zkm_table_enum_index(tid) == -1 and lib.zkm_num_lookup_columns(tid, C.byref(cfg)) == 0
    for name, tid in (("POSEIDON", T.TABLE_POSEIDON), ("KECCAK_SPONGE", T.TABLE_KECCAK_SPONGE), ("LOGIC", T.TABLE_LOGIC), ("MEMORY", T.TABLE_MEMORY),
                      ("ARITHMETIC", T.TABLE_ARITHMETIC), ("KECCAK", T.TABLE_KECCAK), ("POSEIDON_SPONGE", T.TABLE_POSEIDON_SPONGE)):
        assert getattr(zkm, name + "_COLS") == lib.zkm_table_width(tid), name
    assert lib.zkm_all_stark_ctl_table(99) is None and lib.zkm_all_stark_ctl_table(T.TABLE_CPU) is not None
    lg[1] = 99  # a table height the library cannot size
    assert lib.zkm_prove_segment(None, C.byref(cfg), ptrs, lg, None, 0, None, offs, None, C.byref(err)) != 0


# ------------------------------------------------------------------ struct layouts: header == ctypes / numpy mirrors == Rust mirror
# sizeof of every struct of the header, in bytes: a struct that grows or shrinks is a decision, made here
SIZES = {"zkm_challenger": 232, "zkm_stark_config": 28, "zkm_proof_layout": 216, "zkm_proof_query_layout": 464, "zkm_column": 24,
         "zkm_colset": 32, "zkm_ctl_table": 72, "zkm_ctl_z": 32, "zkm_ctl_side": 8, "zkm_cross_table_lookup": 16, "zkm_table_input": 48,
         "zkm_segment_ops": 288, "zkm_boot_image": 104, "zkm_cpu_step": 48, "zkm_cpu_steps": 32, "zkm_image_pages": 208, "zkm_fri_poly": 8,
         "zkm_fri_batch": 32, "zkm_ctl_location": 16, "zkm_ctl_report": 840, "zkm_verify_report": 32}


@functools.lru_cache(maxsize=None)
def c_layouts():
    """{struct: {"size", "align", "fields": [[name, offset, size]]}} of every struct of include/zkm_hip.h, from the C compiler: the probe
    zkm_amd/abi.py generates from the header, built as pedantic C99 in a temporary directory and run."""
    from zkm_amd import abi
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "abi_layout.c"), os.path.join(tmp, "abi_layout")
        open(src, "w").write(abi.layout_probe_source())
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-o", exe, src])
        return json.loads(subprocess.check_output([exe]))


def test_the_compiler_lays_out_every_header_struct(zkm):
    """Every struct the header declares, tagged or not, with every field in order; the fields tile the struct without overlap; and no
    struct changed its size."""
    lay = c_layouts()
    assert {name: [f[0] for f in v["fields"]] for name, v in lay.items()} == zkm.abi.structs()
    for name, v in lay.items():
        end = 0
        for _, off, size in v["fields"]:
            assert off >= end and size > 0, name
            end = off + size
        assert end <= v["size"] and v["size"] % v["align"] == 0, name
    assert {name: v["size"] for name, v in lay.items()} == SIZES


def test_python_mirrors_match_the_c_layout(zkm):
    """The ctypes Structures and numpy dtypes that cross the C ABI (zkm_amd/__init__.py, zkm_amd/ctl.py) against the compiler's layout:
    total size, alignment, and name, offset and size of every field in declaration order."""
    lay = c_layouts()
    mirrors = zkm.abi_mirrors()
    assert set(mirrors) == set(lay), set(mirrors) ^ set(lay)
    assert set(zkm.BY_REFERENCE) <= set(mirrors) and all(issubclass(mirrors[n], C.Structure) for n in zkm.BY_REFERENCE)
    for name, m in mirrors.items():
        want = [tuple(f) for f in lay[name]["fields"]]
        if isinstance(m, np.dtype):
            got = [(f, m.fields[f][1], m.fields[f][0].itemsize) for f in m.names]
            size, align = m.itemsize, max(m.fields[f][0].base.alignment for f in m.names)    # (the dtypes are packed: what their fields need)
            if name == "zkm_cross_table_lookup":      # the nested zkm_ctl_side `looked` is flattened into two u32 in the dtype
                assert m.names[2:] == ("looked_table", "looked_colset") and got[2][2] + got[3][2] == lay["zkm_ctl_side"]["size"]
                got = got[:2] + [("looked", got[2][1], got[2][2] + got[3][2])]
        else:
            got = [(f, getattr(m, f).offset, getattr(m, f).size) for f, _ in m._fields_]
            size, align = C.sizeof(m), C.alignment(m)
        assert got == want, (name, got, want)
        assert (size, align) == (lay[name]["size"], lay[name]["align"]), (name, size, align)


RUST_PRIM = {"u64": (8, 8), "usize": (8, 8), "u32": (4, 4), "c_uint": (4, 4), "c_int": (4, 4), "i32": (4, 4), "u8": (1, 1)}


def rust_structs():
    """{name: [(field, type text)]} of the #[repr(C)] structs in integration/rust/zkm_hip_sys.rs (uncompiled here: parsed), under their
    C names: a struct with a Rust-style name answers to its alias (`pub type zkm_boot_image = ZkmBootImage;`) too."""
    text = rust_sys_text()
    out = {}
    for m in re.finditer(r"#\[repr\(C\)\][^{;]*?pub struct (\w+)\s*\{(.*?)\}", text, flags=re.S):
        fields = []
        for f in filter(None, (x.strip() for x in re.split(r",(?![^\[]*\])", m.group(2)))):
            fm = re.match(r"(?:pub\s+)?([A-Za-z_][A-Za-z0-9_]*)\s*:\s*(.+)$", f, flags=re.S)
            assert fm, (m.group(1), f)
            fields.append((fm.group(1), " ".join(fm.group(2).split())))
        out[m.group(1)] = fields
    for alias, name in re.findall(r"pub type (zkm_\w+) = (\w+);", text):
        out[alias] = out[name]
    return out


def rust_type_layout(ty, structs, memo):
    """(size, align) of a Rust type under repr(C) on x86-64 / LP64."""
    if ty.startswith("*const") or ty.startswith("*mut"):
        return 8, 8
    arr = re.match(r"\[(.+);\s*(\d+)\]$", ty)
    if arr:
        s, a = rust_type_layout(arr.group(1).strip(), structs, memo)
        return s * int(arr.group(2)), a
    if ty in RUST_PRIM:
        return RUST_PRIM[ty]
    assert ty in structs, "unknown Rust type %r" % ty
    return rust_struct_layout(ty, structs, memo)[:2]


def rust_struct_layout(name, structs, memo):
    if name not in memo:
        off, align, fields = 0, 1, []
        for f, ty in structs[name]:
            s, a = rust_type_layout(ty, structs, memo)
            off = (off + a - 1) // a * a
            fields.append((f, off, s))
            off += s
            align = max(align, a)
        memo[name] = ((off + align - 1) // align * align, align, fields)
    return memo[name]


def test_rust_mirror_matches_the_c_layout():
    """The #[repr(C)] structs of integration/rust/zkm_hip_sys.rs, laid out by the repr(C) rules (fields in order, each aligned to its
    type, size rounded to the struct's alignment), against the compiler's layout of the header -- names, offsets, sizes, total size,
    alignment -- for every struct of the header."""
    lay = c_layouts()
    structs = rust_structs()
    opaque = {k for k, v in structs.items() if [f for f, _ in v] == ["_p"]}
    assert opaque == {"zkm_ctx", "zkm_batch", "zkm_pool", "zkm_staged"}
    assert {k for k in structs if k.startswith("zkm_")} - opaque == set(lay), ({k for k in structs if k.startswith("zkm_")} - opaque) ^ set(lay)
    memo = {}
    for name in lay:
        size, align, fields = rust_struct_layout(name, structs, memo)
        assert [list(f) for f in fields] == lay[name]["fields"], (name, fields, lay[name]["fields"])
        assert (size, align) == (lay[name]["size"], lay[name]["align"]), name


# ------------------------------------------------------------------ declarations: header == Rust extern block, for every function
C_TO_RUST = {"int": "c_int", "unsigned": "c_uint", "size_t": "usize", "uint8_t": "u8", "uint32_t": "u32", "uint64_t": "u64",
             "double": "c_double", "char": "c_char", "void": "c_void"}
# constants of the header that the Rust block does not declare (a new one is a decision: declare it there, or list it here)
HEADER_ONLY = {"ZKM_ARITHMETIC_MAX_LOG_N", "ZKM_CPU_COLS", "ZKM_CTL_REPORT_LOCATIONS", "ZKM_CTL_REPORT_WORDS", "ZKM_KECCAK_COLS",
               "ZKM_KECCAK_SPONGE_COLS", "ZKM_LOGIC_COLS", "ZKM_MEMORY_MAX_LOG_N", "ZKM_POSEIDON_COLS", "ZKM_POSEIDON_SPONGE_COLS",
               "ZKM_SHA_COMPRESS_COLS", "ZKM_SHA_COMPRESS_SPONGE_COLS", "ZKM_SHA_EXTEND_COLS", "ZKM_SHA_EXTEND_SPONGE_COLS",
               "ZKM_PROOF_MAGIC", "ZKM_FRI_PROOF_MAGIC"}


def c_to_rust(ty, known):
    """`const uint64_t* const*` -> `*const *const u64`: each pointer is *const or *mut by the constness of what it points to."""
    m = re.fullmatch(r"(const )?(\w+)((?:\*(?: const)?)*)", ty)
    assert m and (m.group(2) in C_TO_RUST or m.group(2) in known), "no Rust spelling for the C type %r" % ty
    out, const = C_TO_RUST.get(m.group(2), m.group(2)), bool(m.group(1))
    for qualifier in re.findall(r"\*( const)?", m.group(3)):
        out, const = ("*const " if const else "*mut ") + out, bool(qualifier)
    return out


def rust_functions():
    """{function: (return type, [(parameter type, parameter name)])} of the extern block, in Rust's spelling (f64 read as c_double, the
    keyword `in` without its r#)."""
    rust = {}
    for name, args, ret in re.findall(r"pub fn (zkm_\w+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+?)\s*)?;", rust_sys_text()):
        assert name not in rust, name
        params = [tuple(x.strip() for x in a.split(":")) for a in args.split(",") if a.strip()]
        rust[name] = (ret.replace("f64", "c_double"), [(" ".join(ty.split()).replace("f64", "c_double"), arg.replace("r#", "")) for arg, ty in params])
    return rust


def declared_alike(zkm, fn):
    """One function is exported, bound, and named in the extern block with the header's parameter names (the whole-ABI tests of this file
    hold the same, and the types, for every function; the per-feature tests call this for the functions they are about)."""
    assert hasattr(zkm.load(), fn) and fn in zkm.EXPORTS, fn
    assert [arg for _, arg in rust_functions()[fn][1]] == [arg for _, arg in prototypes()[fn][1]], fn


def test_every_function_and_constant_is_declared_alike_in_the_rust_block(zkm):
    """Every prototype of the header against its `pub fn` in the extern block: the parameter names in order, every parameter type and the
    return type (`in` is a keyword of Rust: the block spells it r#in).  Every function that reports through the error channel takes
    `char** err` last and returns int.  Every integer constant the block declares has the header's value."""
    text = rust_sys_text()
    known = set(zkm.abi.structs()) | set(zkm.abi.opaque())
    rust, protos = rust_functions(), prototypes()
    assert set(rust) == set(protos), set(rust) ^ set(protos)
    assert all(re.search(r"pub (enum|struct) %s\b" % handle, text) for handle in zkm.abi.opaque())
    for name, (ret, params) in protos.items():
        want = ("" if ret == "void" else c_to_rust(ret, known), [(c_to_rust(ty, known), arg) for ty, arg in params])
        assert rust[name] == want, (name, rust[name], want)
        if any(ty == "char**" for ty, _ in params):
            assert params[-1] == ("char**", "err") and ret == "int" and [ty for ty, _ in params].count("char**") == 1, name
        if params and params[0][0] == "zkm_ctx*":
            assert params[0][1] == "ctx", name
    consts = zkm.abi.constants()
    declared = {name: int(value, 0) for name, value in re.findall(r"pub const (ZKM_\w+): \w+ = (\w+);", text)}
    assert declared == {k: v for k, v in consts.items() if k not in HEADER_ONLY}
    assert HEADER_ONLY <= set(consts)
    magic = re.search(r"pub const ZKM_PROOF_MAGIC: u64 = (\w+);", read("integration", "rust", "proof_blob.rs")).group(1)   # (the wrapper's own copy)
    assert int(magic.replace("_", ""), 0) == consts["ZKM_PROOF_MAGIC"]


# what a wrapper may name that the extern block does not declare: the two converters prove_hip.rs defines (and the files that call them),
# the header's magic that proof_blob.rs restates
WRAPPER_ITEMS = {"prove_hip.rs": {"zkm_table_id", "zkm_config"}, "check_ctls_hip.rs": {"zkm_table_id"}, "verify_hip.rs": {"zkm_config"},
                 "proof_blob.rs": {"ZKM_PROOF_MAGIC"}}
WRAPPERS = sorted(os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "integration", "rust", "*.rs")) if f != RUST_SYS)


@pytest.mark.parametrize("wrapper", WRAPPERS)
def test_the_rust_wrappers_name_only_declared_library_items(wrapper):
    """Every zkm_* function, struct or handle and every ZKM_* constant a file of integration/rust names is declared in the extern block
    (or is one of the few items the wrappers define themselves)."""
    from .test_rust_names import strip_comments
    sys_rs = strip_comments(open(RUST_SYS).read())
    declared = set(re.findall(r"pub fn (zkm_\w+)\s*\(", sys_rs)) | set(re.findall(r"pub (?:struct|enum|type) (zkm_\w+)", sys_rs)) | \
        set(re.findall(r"pub const (ZKM_\w+):", sys_rs))
    src = strip_comments(read("integration", "rust", wrapper))
    used = set(re.findall(r"\b(zkm_[a-z0-9_]+|ZKM_[A-Z0-9_]+)\b", src))
    assert used - WRAPPER_ITEMS.get(wrapper, set()) <= declared, (wrapper, used - declared)


def build_c_smoke(tmp_path):
    exe = str(tmp_path / "c_smoke")
    libdir = os.path.join(ROOT, "zkm_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "c_smoke.c"), "-L" + libdir, "-lzkmhip", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    return exe


def test_pure_c_caller_builds_and_reports_errors(zkm, oracle, tmp_path):
    """tools/c_smoke.c: the header used from pedantic C99 and linked against libzkmhip.so with no Python in the process.  Without a GPU
    the run must end in the library's error channel (nonzero status + malloc'd message), not in a crash."""
    from zkm_amd import tables as T
    exe = build_c_smoke(tmp_path)
    seg = np.load(os.path.join(ROOT, "tests", "golden", "segment12.npz"))
    log_n = [int(x) for x in seg["log_n"]]
    ctl_tables, ctls = T.all_cross_table_lookups()
    tables = [(T.TABLE_ENUM_ORDER[i], seg["t%d" % i], T.WIDTH[T.TABLE_ENUM_ORDER[i]], log_n[i], ctl_tables[i]) for i in range(12)]
    img = zkm.segment_image(tables, ctls, public_values=[1, 2, 3])
    path = tmp_path / "segment.zkmtrace"
    img.tofile(path)
    r = subprocess.run([exe, str(path), str(tmp_path / "proofs.bin")], capture_output=True, text=True, timeout=120)
    import torch
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "c_smoke: zkm_ctx_create:" in r.stderr, (r.returncode, r.stderr)
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"NOTATRACE" + b"\0" * 119)
    r = subprocess.run([exe, str(bad), str(tmp_path / "p.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "magic" in r.stderr


def test_every_tuning_key_is_documented_in_the_header():
    """zkm_ctx_set_tuning: the keys the library accepts (csrc/core.hip) are exactly the keys include/zkm_hip.h documents -- a knob added to
    one side only fails here -- and INTEGRATION.md names no key that does not exist."""
    core = open(os.path.join(ROOT, "zkm_amd", "csrc", "core.hip")).read()
    accepted = set(re.findall(r'k == "([a-z_0-9]+)"', core))
    body = core[core.index("int zkm_ctx_set_tuning("):]
    body = body[:body.index("\n}\n")]   # the function ends at the first closing brace in column 0
    code_keys = set(re.findall(r'k == "([a-z_0-9]+)"', body))
    header = open(os.path.join(ROOT, "include", "zkm_hip.h")).read()
    documented = set(re.findall(r'\*\s+"([a-z_0-9]+)"\s', header))
    doc_keys = set(re.findall(r'^ \*   "([a-z_0-9]+)"', header, flags=re.M))
    assert accepted and accepted == documented, (sorted(accepted - documented), sorted(documented - accepted))
    assert code_keys and code_keys == doc_keys, (sorted(code_keys - doc_keys), sorted(doc_keys - code_keys))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    named = set(re.findall(r'zkm_ctx_set_tuning\([^)]*?"([a-z_0-9]+)"', integ)) | set(re.findall(r'set_tuning\("([a-z_0-9]+)"', integ))
    assert named <= code_keys, sorted(named - code_keys)
