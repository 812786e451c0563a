"""The reference items integration/rust/segment_hip.rs uses -- the fields of Traces (witness/traces.rs:47-62), of the four sponge
operation structs, of MemoryAddress, the #[repr(C)] of CpuColumnsView, the input widths of the SHA / Keccak tables -- exist in the
reference with the visibility and types the file relies on; and logic::Operation keeps its fields private, the reason for the one
addition to logic.rs the file documents.  The facts are stored in tests/golden/reference_segment_api.json, so the suite needs no
reference tree; with ZKM_REFERENCE_ROOT naming a checkout the checks read that tree instead, and
`python tests/test_rust_segment_names.py <reference checkout>` rewrites the JSON file from it."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_rust_names import crate_imports, item_visibility, strip_comments, struct_fields  # noqa: E402

FILE = os.path.join(ROOT, "integration", "rust", "segment_hip.rs")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_segment_api.json")
SRC = {"traces": "prover/src/witness/traces.rs", "memory": "prover/src/witness/memory.rs", "witness": "prover/src/witness/mod.rs",
       "keccak_sponge": "prover/src/keccak_sponge/keccak_sponge_stark.rs", "poseidon_sponge": "prover/src/poseidon_sponge/poseidon_sponge_stark.rs",
       "sha_extend_sponge": "prover/src/sha_extend_sponge/sha_extend_sponge_stark.rs",
       "sha_compress_sponge": "prover/src/sha_compress_sponge/sha_compress_sponge_stark.rs", "logic": "prover/src/logic.rs",
       "cpu_columns": "prover/src/cpu/columns/mod.rs", "sha_extend": "prover/src/sha_extend/sha_extend_stark.rs",
       "sha_compress": "prover/src/sha_compress/sha_compress_stark.rs", "keccak": "prover/src/keccak/keccak_stark.rs"}
OPS = {"KeccakSpongeOp": "keccak_sponge", "PoseidonSpongeOp": "poseidon_sponge", "ShaExtendSpongeOp": "sha_extend_sponge",
       "ShaCompressSpongeOp": "sha_compress_sponge"}
# integration modules of this repository (not reference items): their own tests cover them
OWN_MODULES = {("arithmetic_hip",), ("memory_hip",)}


def eval_product(term):
    out = 1
    for x in term.split("*"):
        out *= int(x)
    return out


def reference_facts(root):
    src = {k: strip_comments(open(os.path.join(root, p)).read()) for k, p in SRC.items()}
    fields = lambda s, n: {f: [vis, re.sub(r"\s+", " ", ty)] for f, (vis, ty) in (struct_fields(s, n) or {}).items()}
    def const(s):   # NUM_INPUTS = a literal sum of products, e.g. 10 * 4 + 1
        expr = re.search(r"pub(?:\(crate\))? const NUM_INPUTS: usize = ([0-9 *+]+);", s).group(1)
        return sum(eval_product(t) for t in expr.split("+"))
    return {
        "files": SRC,
        "visibility": {"Traces": item_visibility(src["traces"], "Traces"), "MemoryAddress": item_visibility(src["memory"], "MemoryAddress"),
                       "traces_module": item_visibility(src["witness"], "traces"), "memory_module": item_visibility(src["witness"], "memory")},
        "traces_fields": fields(src["traces"], "Traces"),
        "op_fields": {n: fields(src[k], n) for n, k in OPS.items()},
        "memory_address_fields": fields(src["memory"], "MemoryAddress"),
        "logic_operation_fields": fields(src["logic"], "Operation"),
        "cpu_columns_repr_c": bool(re.search(r"#\[repr\(C\)\]\s*(#\[[^\]]*\]\s*)*pub struct CpuColumnsView\b", src["cpu_columns"])),
        "num_inputs": {k: const(src[k]) for k in ("sha_extend", "sha_compress", "keccak")},
    }


def facts():
    root = os.environ.get("ZKM_REFERENCE_ROOT")
    return reference_facts(root) if root else json.load(open(FIXTURE))["facts"]


def source():
    return strip_comments(open(FILE).read())


def test_crate_imports_resolve_in_the_reference():
    f = facts()
    imports = crate_imports(source())
    assert ("witness", "traces") in [p for p, _ in imports] and ("witness", "memory") in [p for p, _ in imports]
    for path, item in imports:
        if path in OWN_MODULES:
            continue
        assert (path, item) in ((("witness", "traces"), "Traces"), (("witness", "memory"), "MemoryAddress")), (path, item)
        assert f["visibility"][item] in ("pub", "pub(crate)")
    assert f["visibility"]["traces_module"] in ("pub", "pub(crate)") and f["visibility"]["memory_module"] in ("pub", "pub(crate)")


def test_every_traces_field_is_packed_and_exists():
    """segment_hip.rs reads traces.<field> for all twelve fields of Traces and nothing else; each is visible to the crate."""
    f = facts()
    used = set(re.findall(r"\btraces\.([a-z_][a-z0-9_]*)\b", source()))
    assert used == set(f["traces_fields"]), used ^ set(f["traces_fields"])
    assert all(vis == "pub(crate)" or vis == "pub" for vis, _ in f["traces_fields"].values())
    assert f["traces_fields"]["cpu"][1].startswith("Vec<CpuColumnsView<T>>") and f["cpu_columns_repr_c"]
    assert f["traces_fields"]["sha_compress_inputs"][1].startswith("Vec<([u8; sha_compress_stark::NUM_INPUTS], MemoryAddress, usize)>")


def test_sponge_op_and_address_fields_exist():
    f = facts()
    src = source()
    ops = f["op_fields"]
    for name in ("KeccakSpongeOp", "PoseidonSpongeOp"):
        assert set(ops[name]) == {"base_address", "timestamp", "input"}
    assert {"base_address", "timestamp", "input", "i", "output_address"} <= set(ops["ShaExtendSpongeOp"])
    assert {"base_address", "timestamp", "input", "w_i_s"} <= set(ops["ShaCompressSpongeOp"])
    assert ops["ShaCompressSpongeOp"]["w_i_s"][1] == "Vec<[u8; 4]>" and ops["ShaExtendSpongeOp"]["i"][1] == "usize"
    every = set().union(*[set(v) for v in ops.values()])
    used = set(re.findall(r"\b(?:o|op|rounds\[0\])\.([a-z_][a-z0-9_]*)\b", src)) - {"hip_words"}
    assert used <= every, used - every
    assert all(vis in ("pub", "pub(crate)") for v in ops.values() for vis, _ in v.values())
    addr = f["memory_address_fields"]
    assert set(re.findall(r"\ba\.([a-z_]+) as u64", src)) == set(addr) == {"context", "segment", "virt"}
    assert all(vis in ("pub", "pub(crate)") for vis, _ in addr.values())
    assert f["num_inputs"] == {"sha_extend": 16, "sha_compress": 41, "keccak": 25}


def test_logic_fields_are_private_and_the_addition_is_documented():
    f = facts()
    assert {k: v[0] for k, v in f["logic_operation_fields"].items() if k != "result"} == {"operator": "private", "input0": "private",
                                                                                        "input1": "private"}
    raw = open(FILE).read()
    assert "pub(crate) fn hip_words(&self) -> [u32; 3]" in raw and "op.hip_words()" in raw
    assert not re.search(r"\bop\.(operator|input0|input1)\b", source())


if __name__ == "__main__":
    ref = sys.argv[1]
    with open(FIXTURE, "w") as fh:
        json.dump({"about": "facts about the reference's Traces, sponge operations, MemoryAddress and logic::Operation used by "
                            "tests/test_rust_segment_names.py; regenerate with `python tests/test_rust_segment_names.py <reference checkout>`",
                   "facts": reference_facts(ref)}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("facts ->", FIXTURE)
